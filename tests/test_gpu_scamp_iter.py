"""GPU: every iteration of the SCAMP launch engine (ENGINE_LAUNCHES: amp_scamp.hip, the epilogues of
amp_scamp.h) against one float64 step on the engine's own outputs (tests/launch_iter_ref.py).

Per case and arithmetic, forwards of 1, 2, 3 and 4 iterations on the same inputs (public contract
only: SCAMP(cfg_t, ENGINE_LAUNCHES, gemm).detect) give the state after every iteration; step t:

1. status: T == t, stopped == 0, nan_state == 0, status.gemm the arithmetic asked for, and
   amp_scamp_select_engine answers ENGINE_LAUNCHES; no NaN;
2. xmap_t against scamp_step_f64 on the engine's xmmse_{t-1}, psi_{t-1} (z, phi carried in float64):
   rms, worst 32 x 64 block rms and max of the error over the rms of xmap at most K_RMS (rms, block)
   or K_MAX (max) times the numpy c64 step's on the identical inputs (K_RMS = 3, K_MAX = 6 of
   persist_linear_ref; test_launch_iter_cpu.py holds every mutant of the step at >= 2 K_RMS);
3. xmmse_t against the float64 mean-only denoiser on the engine's own xmap_t with the float64
   tau / 2: |x - ref| <= 3e-6 + 4e-7 max|xi| (persist_denoiser_cases.xtol);
4. psi_t against 1 - sum |xmmse_t|^2 / Na in float64 from the engine's own xmmse_t, the error taken
   over the rms of the subtracted sum (psi itself goes to 0), under the same K_RMS / K_MAX against
   the oracle's float32 line (at B = 1: the forward's psi values of all iterations together,
   launch_iter_ref.scamp_records).

Shapes (launch_iter_ref.SCAMP_CASES): N % 4 == 2 with odd n, a partial last column tile, banded
ISI with QPSK and 16QAM, N = 512 / n = 320 at B = 35 (f32 and bf16x3 tiles), a coupling block wider
than a column tile (Nt = 192) and one valid row.  16QAM runs at 0 dB: from 1 dB the reference's
float64 denoiser underflows to 0 / 0 within three iterations at this shape.

Exit: at the g11 isi3 shape, 10 dB, the 20-iteration forward stops by allclose(psi); its T equals the
first t at which oracle.allclose_f32(psi_t, psi_{t-1}) holds on the engine's own swept outputs, and
the forward of T iterations equals it bit for bit.

Measured ratios: profiles/launch_iter_err.txt (tools/launch_iter_err.py).
"""
import pytest

import launch_iter_gpu as lig
import launch_iter_ref as lir

pytestmark = pytest.mark.gpu

ENGINE = lir.ENGINE_LAUNCHES
CASES = [(c, g) for c in lir.SCAMP_CASES for g in lir.scamp_arithmetics(c)]
IDS = [f'{lir.case_id(c)}-{lir.ARITH_NAMES[g]}' for c, g in CASES]


@pytest.mark.parametrize('case,gemm', CASES, ids=IDS)
def test_iterations_against_float64(device, case, gemm):
    lir.assert_bars(*lig.measure_scamp(device, case, gemm, ENGINE))


def test_exit_matches_own_outputs(device):
    """The in-kernel allclose(psi) count at a shape with a partial row tile, judged on the engine's
    own psi_t alone (no reference trajectory)."""
    lig.check_exit(lambda t: lig.scamp_forward(device, lir.EXIT_CASE, lir.GEMM_F32, t, ENGINE), bitwise=True)
