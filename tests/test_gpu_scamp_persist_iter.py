"""GPU: every iteration of the persistent SCAMP engine (ENGINE_PERSISTENT: amp_scamp_persist*.hip,
amp_scamp_persist_kernel.h) against one float64 step on the engine's own outputs
(tests/launch_iter_ref.py).  The engine was held by curve points and engine-against-engine
comparisons only.

The method, assertions and bars are those of the launch engine's test (test_gpu_scamp_iter.py):
forwards of 1 .. 4 iterations through SCAMP(cfg_t, ENGINE_PERSISTENT, gemm).detect; xmap and psi
under K_RMS / K_MAX against the numpy c64 step, xmmse under the float32-logit denoiser's bar, with
amp_scamp_select_engine asserted to answer ENGINE_PERSISTENT and status.gemm the arithmetic asked
for.  At B = 1 psi is one value per iteration: the forward's four are judged together
(launch_iter_ref.scamp_records, where the figures are).  Cases: the engine's three shapes
(2N, 2n) = (128, 256), (256, 512), (256, 256) (Nt / Nr = 64 / 128, 128 / 256, 128 / 128 at Na = 8,
Lin = Lh = 1), QPSK at 2 dB and 16QAM at 0 dB (from 3 dB the reference's float64 denoiser underflows
to 0 / 0 by the third iteration), B = 35 (workgroups of 16, 16 and 3 trials) and B = 1, in f32 MFMA,
bf16x3 and fp16x2.

Exit: Nt 128, Nr 256, QPSK, 8 dB, B = 35: the 20-iteration forward's T equals the first t at which
oracle.allclose_f32(psi_t, psi_{t-1}) holds on the engine's own swept outputs.

Measured ratios: profiles/launch_iter_err.txt (tools/launch_iter_err.py).
"""
import pytest

import launch_iter_gpu as lig
import launch_iter_ref as lir

pytestmark = pytest.mark.gpu

ENGINE = lir.ENGINE_PERSISTENT
CASES = [(c, g) for c in lir.PERSIST_CASES for g in (lir.GEMM_F32, lir.GEMM_X3, lir.GEMM_H2)]
IDS = [f'{lir.case_id(c)}-{lir.ARITH_NAMES[g]}' for c, g in CASES]


@pytest.mark.parametrize('case,gemm', CASES, ids=IDS)
def test_iterations_against_float64(device, case, gemm):
    lir.assert_bars(*lig.measure_scamp(device, case, gemm, ENGINE))


@pytest.mark.parametrize('gemm', [lir.GEMM_F32, lir.GEMM_X3], ids=['f32', 'bf16x3'])
def test_exit_matches_own_outputs(device, gemm):
    """The in-kernel allclose(psi) exit with a partial last workgroup, judged on the engine's own
    psi_t alone."""
    lig.check_exit(lambda t: lig.scamp_forward(device, lir.EXIT_CASE_PERSIST, gemm, t, ENGINE), bitwise=False)
