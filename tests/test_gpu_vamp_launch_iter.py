"""GPU: every iteration of the VAMP LAUNCH engine (vamp_k1 / vamp_k2<BN, KK> / vamp_r of amp_vamp.hip,
the bodies of amp_vamp_launch.h, the y~ gemm_store) against float64 steps on the engine's own state
(tests/vamp_launch_iter_ref.py, tests/vamp_launch_iter_gpu.py).

This engine takes every shape the persistent engine refuses (k < N, odd n, odd k, a partial last
column tile, N > 256, M = 128), the trial batches, the trial-sharded mode and the grid rescue; the
suite's other tests hold it by counting metrics, VER / SER within 1e-3 and bit equality between the
project's own paths, none of which would see a y~ off in the sixth digit at odd n, a last odd-k column
of w weighted wrongly in GEMM2, a second 512-float reduction chunk mis-indexed, a stale alpha in the
r epilogue or a wrong column in the 128 + 64 partial tile.  Here, per case of vamp_launch_iter_ref.CASES,
forwards of 1, 2, 3 and 4 iterations on the same inputs through VAMP(cfg, engine=ENGINE_LAUNCHES) (gemm
AUTO); the state after iteration t is the (t + 1)-iteration forward's r, xmmse, var and status with
its workspace's y~ and w (columns < 2k of a row of wld floats):

1. route and hygiene: amp_vamp_select_engine answers LAUNCHES, T == iterations, no stop, nan_state 0,
   status.gemm f32, no NaN anywhere; w's pad floats are exactly 0 after every forward; y~ is bit-equal
   across the four forwards;
2. scalars: persist_linear_ref.scalar_chain on mean_var_f32 of the engine's own var outputs gives
   every prefix forward's status.last_scalar (sigma2_tilde, alpha, sigma2, dxdr) bit for bit;
3. y~ against ytil_f64;  4. w_t against w_f64 on the engine's own state of t - 1 (the Tracker's at
   t = 0) and its own y~;  5. r_t against r_f64 on the engine's own w_t: e_rms and the worst
   32 x 64 block rms at most K_RMS = 3, e_max at most K_MAX = 6 times the same statistic of the
   numpy c64 step on identical inputs (products padded to 16 rows at B = 1), no absolute floor;
6. xmmse_t, var_t against denoise_f64 on the engine's own r_t with the chain's sigma2:
   |x - ref| <= 3e-6 + 4e-7 max|xi|, |var - ref| <= 1e-4 |ref| + the same;
7. exit (two cases, iterations = 20): status.T and `stopped` equal the first t at which
   torch_close_f32(var_t, var_{t-1}) holds everywhere on the engine's own prefix-forward outputs; T
   is printed beside the oracle's, not tied to it;
8. the trial-sharded stages vamp_xr1 .. vamp_xr4: the 2N = 192 case as two slices of 24 through
   ShardedVAMP (two threads, shard_threads.run_slices), prefix forwards 1 .. 4; each slice is held to
   2, 5 and 6 with the var mean over all 48 trials.

Also: a launch-engine forward at k = N = 64 with GEMM_AUTO reports f32 (status.gemm, Loss.arithmetic);
vamp_make_status used to say bf16x3 there while f32 tiles ran.

First measured (MI355X), the kernels missed two bars at Nt512-Nr1024 and were changed, not the bars:
y~ over 2n = 2048 floats at 4.10x / 4.65x / 7.91x numpy (rms / block / max) and GEMM2 over 2k = 1024
at 3.07x in its worst block, gemm_tile chaining one float32 accumulator through the whole reduction
(the ratio grew with its length: 1.2x at 30 floats, 2.0x at 640, 2.5x at 1024).  gemm_store_kernel and
GEMM2 now sum long reductions per 512-float chunk (amp_gemm.h gemm_tile SEG); worst ratios since:
y~ 2.48 / 2.56 / 3.56, w 2.42 / 2.65 / 3.40, r 2.11 / 2.16 / 4.20.

Measured ratios: profiles/vamp_launch_iter_err.txt (tools/vamp_launch_iter_err.py).
"""
import ctypes as C

import pytest
import torch

import vamp_launch_iter_gpu as vig
import vamp_launch_iter_ref as vir

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case', vir.CASES, ids=[vir.case_id(c) for c in vir.CASES])
def test_iterations_against_float64(device, case):
    vir.assert_bars(*vig.measure(device, case))


@pytest.mark.parametrize('case', vir.EXIT_CASES, ids=[vir.case_id(c) for c in vir.EXIT_CASES])
def test_exit_matches_own_outputs(device, case):
    T, T_oracle = vig.check_exit(device, case)
    print(f'{vir.case_id(case)}: stopped at T = {T} (the oracle: {T_oracle})')
    assert T < vir.EXIT_ITERS


def test_sharded_slices_against_float64(device, monkeypatch):
    for rec in vig.measure_sharded(device, monkeypatch):
        vir.assert_bars(*rec)


def test_launch_engine_reports_f32_at_a_persistent_shape(device):
    """k = N = 64, engine = LAUNCHES, gemm = AUTO: the arithmetic that ran is f32."""
    import amp_native as nat
    from vamp import VAMP
    case = vir.ROUTE_CASE
    cfg = vir.make_config(case)
    d = cfg.dims()
    k = vir.geometry(case).k
    assert nat.lib().amp_vamp_select_engine(C.byref(d), k, nat.ENGINE_AUTO) == nat.ENGINE_PERSISTENT
    assert nat.lib().amp_vamp_select_engine(C.byref(d), k, nat.ENGINE_LAUNCHES) == nat.ENGINE_LAUNCHES
    inp = vir.inputs(case)
    U, s, Vh, y, x = (inp.t[n].to(device) for n in ('U', 's', 'Vh', 'y', 'x'))
    det = VAMP(cfg, engine=nat.ENGINE_LAUNCHES, gemm=nat.GEMM_AUTO)
    L = det(U, s, Vh, y, inp.SNR, x, inp.sym, inp.idx)
    assert L.arithmetic == 'f32'
    torch.cuda.synchronize()
    st = det.last.status()
    assert (st.gemm, st.nan_state) == (nat.GEMM_F32, 0), (st.gemm, st.nan_state)
