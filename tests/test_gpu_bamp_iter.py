"""GPU: every iteration of the BAMP launch engine (amp_bamp.hip, the epilogues of amp_bamp.h) against
one float64 step on the engine's own outputs (tests/launch_iter_ref.py).

The suite's other BAMP tests hold end results: decision counts, VER / SER within 1e-3 and T; the trial
and sharded engines are tied bit for bit to this engine's forwards.  None would see an operand that
lost its low bits, an Onsager term taken with the wrong u, a column tile that drops its last columns
or a band range [kb, ke) one granule short at a shape whose counting metrics survive it.  Here, per
case and arithmetic, forwards of 1, 2, 3 and 4 iterations on the same inputs (public contract only:
BAMP(cfg_t).detect) give the state after every iteration, and step t is checked as follows:

1. status: T == t, stopped == 0, nan_state == 0, status.gemm the arithmetic asked for; no NaN;
2. xmap_t against bamp_step_f64 on the engine's xmmse_{t-1}, var_{t-1} (z, u carried in float64):
   rms, worst 32 x 64 block rms and max of the error over the rms of xmap, each at most K_RMS (rms,
   block) or K_MAX (max) times the same statistic of the numpy c64 step on the identical inputs
   (persist_linear_ref's K_RMS = 3, K_MAX = 6; test_launch_iter_cpu.py holds every mutant of the
   step at >= 2 K_RMS);
3. xmmse_t, var_t against the float64 denoiser on the engine's own xmap_t with the float64 cov / 2:
   |x - ref| <= 3e-6 + 4e-7 max|xi|, |var - ref| <= 1e-4 |ref| + the same (persist_denoiser_cases).

Shapes (launch_iter_ref.BAMP_CASES): N % 4 == 2 with odd n, a partial last column tile, banded ISI
with QPSK and 16QAM, N = 512 / n = 320 at B = 35 (f32, bf16x3 and fp16x2 tiles), M = 2 at 2N = 1008,
one valid row, and two ISI channels with one nonzero entry far outside the band (the data-derived
band range of that column tile must widen to it: in the f32 tiles, and at N = 512 / n = 320 in the
bf16x3 and fp16x2 tiles as well).

Exit: at the g11 isi3 shape, 10 dB, the 20-iteration forward stops by allclose; its T equals the
first t at which oracle.allclose_f32(var_t, var_{t-1}) holds on the engine's own swept outputs, and
the forward of T iterations equals it bit for bit.

Measured ratios: profiles/launch_iter_err.txt (tools/launch_iter_err.py).
"""
import pytest

import launch_iter_gpu as lig
import launch_iter_ref as lir

pytestmark = pytest.mark.gpu

CASES = [(c, g) for c in lir.BAMP_CASES for g in lir.bamp_arithmetics(c)]
IDS = [f'{lir.case_id(c)}-{lir.ARITH_NAMES[g]}' for c, g in CASES]


@pytest.mark.parametrize('case,gemm', CASES, ids=IDS)
def test_iterations_against_float64(device, case, gemm):
    lir.assert_bars(*lig.measure_bamp(device, case, gemm))


def test_exit_matches_own_outputs(device):
    """The in-kernel allclose count at a shape with a partial row tile, judged on the engine's own
    var_t alone (no reference trajectory)."""
    lig.check_exit(lambda t: lig.bamp_forward(device, lir.EXIT_CASE, lir.GEMM_F32, t), bitwise=True)
