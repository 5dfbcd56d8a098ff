"""Cases, inputs and capture arithmetic of the per-iteration tests of the VAMP LAUNCH engine
(test_vamp_launch_iter_cpu.py, test_gpu_vamp_launch_iter.py, tools/vamp_launch_iter_err.py): vamp_k1 /
vamp_k2<BN, KK> / vamp_r of csrc/amp_vamp.hip, the bodies of csrc/amp_vamp_launch.h and the y~
gemm_store.  numpy only, no GPU here.

The float64 steps, the numpy c64 yardstick, the float32 scalar chain and the bars are
persist_linear_ref's and persist_denoiser_cases', by import; the block statistic and the denoiser
record are launch_iter_ref's.  What is new here is the launch engine's own shapes (k < N, odd n, odd
k, a partial last column tile, N > 256, M = 128) and how a forward's state is read: the state after
iteration t is the (t + 1)-iteration forward's r, xmmse, var and status, its workspace y~
(amp_vamp_debug_offsets[4]) and w (amp_vamp_debug_launch_offsets: row stride wld = 2k rounded up to 4,
columns < 2k the value).  Per iteration t, with the chain run on the engine's own var means:

  y~   against ytil_f64                                                       (the gemm_store launch)
  w_t  against w_f64 on the engine's x_{t-1}, r_{t-1} (the Tracker's at 0) and its own y~    (vamp_k1)
  r_t  against r_f64 on the engine's own w_t                                  (vamp_k2's GEMM + epilogue)
  xmmse_t, var_t against denoise_f64 on the engine's own r_t, tau = the chain's sigma2     (vamp_k2)

Linear bars: rms and the worst 32 x 64 block rms at most K_RMS, max at most K_MAX times the same
statistic of the c64 step on identical inputs (products padded to 16 rows at B = 1); no floors.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import launch_iter_ref as lir
from oracle.amp_oracle import C64, F32
from persist_denoiser_cases import AMP_DANGER, VAR_RTOL, denoise_f64, logit_slack, torch_close_f32, xtol  # noqa: F401
from persist_linear_ref import (K_MAX, K_RMS, mean_var_f32, r_c64, r_f64, ratios, round_sig, rt_c64, rt_f64,  # noqa: F401
                                scalar_chain, stats, w_c64, w_f64, ytil_c64, ytil_f64)

# amp_native.GEMM_* / ENGINE_* (restated: this module imports without the built library)
GEMM_AUTO, GEMM_F32 = 0, 1
ENGINE_LAUNCHES = 1

SEED, ITERS = lir.SEED, 4      # both var buffers; vamp_output_kernel copies at T = 2, 4, not at 1, 3
PAD = lir.PAD
GBM, TILE = 32, 128            # amp_gemm.h: trials per row tile, floats per column tile of vamp_k1 / gemm_store
KC = 512                       # amp_gemm.h GKC: reduction floats staged per chunk
Case = lir.Case

# (Nt, Na, Nr, Lin, Lh, B, alphabet, EbN0)
#   6,3,5,3,1       N = 18, n = k = 15: odd n (pair loader on y), odd k (padded w row), k < N, N % 4 == 2
#   12,3,5,2,2      N = 24, n = k = 15 with a complex alphabet
#   8,2,11,1,1      n = 11 odd > N = k = 8
#   48,6,12,2,2     2N = 192: column tiles 128 + 64; k = 36 < N; and at B = 1: one valid row of 32
#   96,6,100,1,1    k = N = 96 with the partial tile, n != 2N, two full row tiles + 6 rows, grid denoiser
#   168,84,73,3,2   M = 2, 2N = 1008, n = k = 292, a partial 32-row tile
#   64,4,32,8,3     N = 512, n = k = 320: two 512-float reduction chunks in GEMM1, M = 16
#   512,32,1024,1,1 k = N = 512 (never persistent), y~ over 2n = 2048 (four chunks), eight column tiles
#   256,2,512,1,1   M = 128: the BN = 256 instantiation of vamp_k2 (no persistent test reaches it); at
#                   0 dB, where a 16-bit Vh still shows in w (test_vamp_launch_iter_cpu.py, c.)
CASES = [Case(6, 3, 5, 3, 1, 48, 'OOK', 8.0), Case(12, 3, 5, 2, 2, 48, 'QPSK', 10.0),
         Case(8, 2, 11, 1, 1, 48, 'BPSK', 6.0), Case(48, 6, 12, 2, 2, 48, 'OOK', 8.0),
         Case(48, 6, 12, 2, 2, 1, 'OOK', 8.0), Case(96, 6, 100, 1, 1, 70, '16QAM', 6.0),
         Case(168, 84, 73, 3, 2, 35, '8PSK', 11.0), Case(64, 4, 32, 8, 3, 35, '16QAM', 8.0),
         Case(512, 32, 1024, 1, 1, 35, '16QAM', 6.0), Case(256, 2, 512, 1, 1, 35, '16QAM', 0.0)]
# what the table above claims of each case (test_vamp_launch_iter_cpu.py asserts it of `geometry`)
CLAIMS = {
    CASES[0]: dict(N=18, n=15, k=15, n_odd=True, k_odd=True, k_lt_N=True, N_mod4=2),   # 2N = 36: N % 4 == 2
    CASES[1]: dict(N=24, n=15, k=15, n_odd=True, k_odd=True, k_lt_N=True),
    CASES[2]: dict(N=8, n=11, k=8, n_odd=True, k_odd=False, k_lt_N=False),
    CASES[3]: dict(N=96, n=36, k=36, col_tiles2=2, last_tile2=64, k_lt_N=True, row_tiles=2),
    CASES[4]: dict(N=96, n=36, k=36, col_tiles2=2, last_tile2=64, k_lt_N=True, row_tiles=1, last_rows=1),
    CASES[5]: dict(N=96, n=100, k=96, col_tiles2=2, last_tile2=64, k_lt_N=False, row_tiles=3, last_rows=6, grid=True),
    CASES[6]: dict(N=504, n=292, k=292, M=2, col_tiles2=8, last_tile2=112, row_tiles=2, last_rows=3),
    CASES[7]: dict(N=512, n=320, k=320, M=16, chunks1=2, row_tiles=2, last_rows=3),
    CASES[8]: dict(N=512, n=1024, k=512, chunks0=4, col_tiles2=8, last_tile2=128, persist_shape=False),
    CASES[9]: dict(N=256, n=512, k=256, M=128, bn2=256, persist_shape=True),
}
# allclose exits (iterations = 20): the oracle stops at T = 5 and at T = 3
EXIT_CASES = [Case(48, 6, 12, 2, 2, 48, 'OOK', 12.0), Case(96, 6, 100, 1, 1, 70, 'QPSK', 10.0)]
EXIT_ITERS = 20
# assertion 5 of the launch engine's status fix: k = N = 64 on the launch engine with GEMM_AUTO
ROUTE_CASE = Case(64, 8, 128, 1, 1, 35, 'QPSK', 2.0)
# the trial-sharded stages (vamp_xr1 .. vamp_xr4): two slices of 24
SHARD_CASE, SHARD_ROWS = CASES[3], 24

case_id = lir.case_id
make_config = lir.make_config
oracle_config = lir.oracle_config


def geometry(case):
    """The launch engine's view of a case (amp_vamp.h vamp_geometry, amp_host.h section_bn / vamp_wld)."""
    N, n = case.Nt * case.Lin, case.Nr * (case.Lin + case.Lh - 1)
    k, M = min(n, N), case.Nt // case.Na
    bn2 = 128 if 2 * M <= 128 else 256
    ct2 = -(-2 * N // bn2)
    return SimpleNamespace(N=N, n=n, k=k, M=M, L=case.Na * case.Lin, n_odd=n % 2 == 1, k_odd=k % 2 == 1, k_lt_N=k < N,
                           N_mod4=N % 4, wld=(2 * k + 3) & ~3, bn2=bn2, col_tiles2=ct2,
                           last_tile2=2 * N - (ct2 - 1) * bn2, col_tiles1=-(-2 * k // TILE),
                           row_tiles=-(-case.B // GBM), last_rows=case.B - (-(-case.B // GBM) - 1) * GBM,
                           chunks0=-(-2 * n // KC), chunks1=-(-2 * N // KC), chunks2=-(-2 * k // KC),
                           grid=case.alphabet == '16QAM', persist_shape=k == N and N in (64, 128, 256))


# ----------------------------------------------------------------------------- inputs
_INPUTS = {}


def inputs(case):
    """The case's operating point as launch_iter_ref.inputs draws it (seed 0, the repository's
    Channel / Data generators in the reference's call order), with the message and its labels kept
    (the sharded forward decides) and A's factors from torch.linalg.svd(A, full_matrices=False).
    Built once per case, left unchanged."""
    if case not in _INPUTS:
        import torch
        from channel import Channel
        from data import Data
        cfg = make_config(case, device='cpu')
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        x, sym, idx = da.generate_message()
        SNR = cfg.snr(case.ebn0)
        y = A @ x + ch.awgn(SNR)
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        U, s, Vh = U.contiguous(), s.contiguous(), Vh.resolve_conj().contiguous()
        _INPUTS[case] = SimpleNamespace(t=dict(U=U, s=s, Vh=Vh, y=y, x=x), sym=sym, idx=idx, SNR=float(SNR),
                                        U=U.numpy().astype(C64), s=s.numpy().astype(F32), Vh=Vh.numpy().astype(C64),
                                        y=y.numpy()[..., 0].astype(C64))
    return _INPUTS[case]


def problem(case):
    """p, eta = k / N, noise_var = (Na / Nr) / SNR and s^2 (float32 and exact)."""
    inp = inputs(case)
    s = inp.s
    return SimpleNamespace(p=case.Na / case.Nt, eta=s.shape[0] / inp.Vh.shape[1],
                           noise_var=(case.Na / case.Nr) / inp.SNR, s2=(s * s).astype(F32),
                           s2_64=s.astype(np.float64) ** 2, symbols=oracle_config(case).symbols)


_TRACES = {}


def oracle_trace(case, iterations: int = ITERS):
    """(result, trace) of oracle.vamp_detect on the case, computed once."""
    key = (case, iterations)
    if key not in _TRACES:
        import oracle.amp_oracle as O
        inp = inputs(case)
        tr = []
        out = O.vamp_detect(inp.U, inp.s, inp.Vh, inp.y, inp.SNR, oracle_config(case, iterations), trace=tr)
        _TRACES[key] = (out, tr)
    return _TRACES[key]


def tracker_state(pb, shape):
    """(xmmse, r) of vamp.py:22-25: r~ = p in every position."""
    return np.full(shape, F32(pb.p), dtype=C64), np.zeros(shape, dtype=C64)


# ----------------------------------------------------------------------------- scalars and the exit
def chain_of(case, var_means):
    pb = problem(case)
    return scalar_chain(pb.s2, pb.noise_var, pb.p, pb.eta, list(var_means))


def last_scalars(chain, T: int, stopped: int):
    """amp_status.last_scalar of a forward that ended after T iterations: sigma2_tilde, alpha, sigma2
    that drove iteration T - 1 and the dxdr it left (on an allclose stop: the one it was driven by)."""
    last = chain[T - 1]
    return np.array([last.s2t32, last.alpha, last.sigma2, last.dxdr_prev if stopped else last.dxdr], dtype=F32)


def first_close(variances):
    """The first t (from 1) at which torch_close_f32(var_t, var_{t-1}) holds everywhere (var_0 = 1:
    vamp.py:24), or None."""
    prev = np.ones_like(np.asarray(variances[0], F32))
    for t, cur in enumerate(variances, 1):
        if bool(np.all(torch_close_f32(cur, prev))):
            return t
        prev = cur
    return None


# ----------------------------------------------------------------------------- records
def linear_record(what, t, got, yard, ref):
    """The engine's and the yardstick's (e_max, e_rms) against the float64 value and their ratios
    (persist_linear_ref.ratios), plus the ratio of launch_iter_ref's worst-block rms."""
    mx, rms, g, y = ratios(got, yard, ref)
    return SimpleNamespace(what=what, t=t, rms=rms, max=mx, blk=lir.xstats(got, ref).blk / lir.xstats(yard, ref).blk,
                           got=g, yard=y)


linear_ok = lir.linear_ok
denoiser_ok = lir.denoiser_ok


def records(case, fws, chain, rows=slice(None), linear_half: bool = True, pad: int = PAD):
    """fws[t]: the state after iteration t (complex64 r, x [B, N], float32 var [B, N], complex64
    w [B, k] and, with linear_half, ytil [B, k]) of the trials `rows` of the case; chain: chain_of on the
    var means of the WHOLE batch.  Returns (linear records, denoiser records); without linear_half
    (a slice of a sharded batch) y~ and w are not judged, r and the denoiser are."""
    inp, pb = inputs(case), problem(case)
    g = geometry(case)
    y = inp.y[rows]
    lin, den = [], []
    if linear_half:
        lin.append(linear_record('y~', 0, fws[-1].ytil, ytil_c64(inp.U, inp.s, y, pad), ytil_f64(inp.U, inp.s, y)))
    for t, fw in enumerate(fws):
        it = chain[t]
        x, r = (fws[t - 1].x, fws[t - 1].r) if t else tracker_state(pb, (y.shape[0], g.N))
        rt64, rtc = rt_f64(x, r, it.dxdr_prev, it.ns_prev), rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        if linear_half:
            lin.append(linear_record('w', t, fw.w, w_c64(rtc, inp.Vh, fw.ytil, pb.s2, it.vr, pad),
                                     w_f64(rt64, inp.Vh, fw.ytil, pb.s2_64, it.vr)))
        lin.append(linear_record('r', t, fw.r, r_c64(fw.w, inp.Vh, rtc, it.alpha, pad),
                                 r_f64(fw.w, inp.Vh, rt64, it.alpha)))            # the engine's own w: GEMM2 alone
        ref = denoise_f64(fw.r, np.float64(it.sigma2), pb.symbols, g.L, g.M)      # the engine's own r
        den.append(lir.denoiser_record('xmmse/var', t, fw.x, fw.var, ref))
    return lin, den


def show(who, lin, den):
    for r in lin:
        print(f'{who} {r.what:2s} t={r.t}: e_rms {r.got[1]:.3e} (numpy {r.yard[1]:.3e}, x{r.rms:.2f})  '
              f'e_max {r.got[0]:.3e} (numpy {r.yard[0]:.3e}, x{r.max:.2f})  block x{r.blk:.2f}')
    for r in den:
        print(f'{who} {r.what} t={r.t}: fraction of the bar: x {r.x:.3f}  var {r.var:.3f}  (max|xi| {r.max_abs_xi:.1f})')


def assert_bars(who, lin, den):
    bad = [f'{r.what} t={r.t} rms x{r.rms:.2f} block x{r.blk:.2f} max x{r.max:.2f}' for r in lin if not linear_ok(r)]
    bad += [f'{r.what} t={r.t} x {r.x:.2f} var {r.var:.2f}' for r in den if not denoiser_ok(r)]
    assert not bad, f'{who}: ' + '; '.join(bad)


# ----------------------------------------------------------------------------- mutants (sensitivity)
# name -> the phase it hits.  Each is a defect of ONE float64 step on the healthy state:
#   lastk  the last column of w dropped from GEMM2                                  (odd k)
#   lastn  y's last entry dropped from y~                                            (odd n)
#   tile   the output columns of GEMM2's partial last column tile shifted by one complex column
#   chunk  reduction terms beyond the first 512 floats dropped: GEMM1 at N = 512, y~ at n >= 512
#   vh16   Vh rounded to 16 significand bits (both GEMMs)
#   alpha  the r epilogue with the previous iteration's alpha                        (t >= 1)
#   pad    w's pad float read as 1.0 where the operator's pad row repeats its last row (odd k):
#          the pad sits where Re of a column k would, so Im's row 2k - 1 of V takes 1.0 more
MUTANTS = ('lastk', 'lastn', 'tile', 'chunk', 'vh16', 'alpha', 'pad')


def applies(mut, case, t: int = 1) -> bool:
    g = geometry(case)
    return {'lastk': g.k_odd, 'pad': g.k_odd, 'lastn': g.n_odd, 'tile': 2 * g.N in (192, 1008),
            'chunk': g.N == 512 or g.n >= 512, 'vh16': True, 'alpha': t >= 1}[mut]


def _head(a, cols):
    out = np.zeros_like(a)
    out[:, :cols] = a[:, :cols]
    return out


def mutant_ytil(mut, case, inp, y):
    """y~ under the mutant (float64), or None where the mutant does not touch it."""
    g = geometry(case)
    if mut == 'lastn':
        return ytil_f64(inp.U, inp.s, _head(np.asarray(y, np.complex128), g.n - 1))
    if mut == 'chunk' and g.n >= 512:
        return ytil_f64(inp.U, inp.s, _head(np.asarray(y, np.complex128), KC // 2))
    return None


def mutant_w(mut, case, inp, pb, rt64, ytil, it):
    g = geometry(case)
    if mut == 'vh16':
        return w_f64(rt64, round_sig(inp.Vh, 16), ytil, pb.s2_64, it.vr)
    if mut == 'chunk' and g.N == 512:
        return w_f64(_head(rt64, KC // 2), inp.Vh, ytil, pb.s2_64, it.vr)
    return None


def mutant_r(mut, case, inp, w, rt64, it, prev_alpha):
    g = geometry(case)
    w = np.asarray(w, np.complex128)
    if mut == 'vh16':
        return r_f64(w, round_sig(inp.Vh, 16), rt64, it.alpha)
    if mut == 'lastk':
        return r_f64(_head(w, g.k - 1), inp.Vh, rt64, it.alpha)
    if mut == 'pad':
        wp = w.copy()
        wp[:, -1] += 1.0j
        return r_f64(wp, inp.Vh, rt64, it.alpha)
    if mut == 'alpha' and prev_alpha is not None:
        return r_f64(w, inp.Vh, rt64, prev_alpha)
    if mut == 'tile':
        r = r_f64(w, inp.Vh, rt64, it.alpha)
        c0 = (g.col_tiles2 - 1) * g.bn2 // 2
        r[:, c0:] = np.roll(r[:, c0:], 1, axis=1)
        return r
    return None
