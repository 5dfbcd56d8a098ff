"""No GPU: the float64 reference and the numpy yardstick of tests/test_gpu_persist_linear.py, and the
conditions that keep that test's bars honest (tests/persist_linear_ref.py).

a. Consistency: chained over oracle.amp_oracle.vamp_detect's trace, the restated c64 steps and the
   restated float32 scalar chain reproduce the oracle's r~, r and scalars bit for bit.
b. Sensitivity: for every case of the table, every iteration and both GEMM phases, a float64 step
   whose Vh operand is rounded to 16 significand bits (a lost bf16x3 low plane) errs by at least
   2 K_RMS times the numpy c64 restatement's e_rms on the same inputs, so the GPU test's rms bar
   K_RMS sits at most half way between a healthy engine and that defect; the same for y~ with U
   rounded.  A second mutant mis-signs ONE imaginary cross term of the third bf16 plane alone (a
   quarter of the products, a plane of <= 2^-18 of the element): at least 2 K_RMS in the r phase at
   every iteration; in the w phase, where y~ / (s^2 + vr) carries most of w and does not pass
   through Vh, over K_RMS at iteration 0 in every case (the operand is packed once per forward, so
   one iteration over the bar fails the GPU test).  Measured here (seed 0, 2 dB, B = 35), e_rms over
   numpy's: 16-bit mutant w 7.6-39x, r 19-38x, y~ 26-37x; cross-term mutant w 2.9-14x (iteration 0:
   4.8-13x), r 7.7-14x.
c. Preconditions of the case table, from the oracle: T == 3, no NaN, alpha and dxdr strictly inside
   their clamps at every iteration and alpha <= 0.95.  At 8 dB (the denoiser tests' point) QPSK
   drives alpha to its clamp by iteration 1 and r = (x~ - alpha r~) / (1 - alpha) is dominated by
   cancellation: numpy's own error in r grows to 1e-5 .. 1e-2 of max|r| and hides the GEMMs.
"""
import numpy as np
import pytest

import persist_linear_ref as plr
from oracle.amp_oracle import VAR_RATIO_MAX, VAR_RATIO_MIN

IDS = [plr.case_id(c) for c in plr.CASES]
B1_CASES = [(c, 1) for c in plr.B1_CASES]
ALL = [(c, plr.B) for c in plr.CASES] + B1_CASES
ALL_IDS = IDS + [plr.case_id(c) + '-B1' for c, _ in B1_CASES]


def _steps(case, batch=plr.B):
    """Per iteration of the oracle's trace: the inputs of the iteration's linear half (the previous
    iteration's xmmse and r, the Tracker's at t = 0) and the chain's scalars."""
    inp = plr.inputs(case, batch)
    pb = plr.problem(case, inp)
    out, tr = plr.oracle_trace(case, batch)
    chain = plr.scalar_chain(pb.s2, pb.noise_var, pb.p, pb.eta, [plr.mean_var_f32(t['var']) for t in tr])
    steps = []
    for t in range(len(tr)):
        if t == 0:
            x = np.full_like(tr[0]['r'], np.float32(pb.p))
            r = np.zeros_like(x)
        else:
            x, r = tr[t - 1]['xmmse'], tr[t - 1]['r']
        steps.append((chain[t], x, r))
    return inp, pb, out, tr, steps


@pytest.mark.parametrize('case,batch', ALL, ids=ALL_IDS)
def test_restatement_reproduces_the_oracle(case, batch):
    """a. bit identity of the c64 steps and the float32 chain with vamp_detect's trace."""
    inp, pb, out, tr, steps = _steps(case, batch)
    ytil = plr.ytil_c64(inp.U, inp.s, inp.y)
    for t, (it, x, r) in enumerate(steps):
        for name, got in (('alpha', it.alpha), ('sigma2', it.sigma2), ('dxdr', it.dxdr), ('sigma2_tilde', it.s2t_next)):
            assert np.float32(got).tobytes() == np.float32(tr[t][name]).tobytes(), (t, name, got, tr[t][name])
        rt = plr.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        if t:
            assert np.array_equal(rt.view(np.uint32), tr[t - 1]['r_tilde'].view(np.uint32)), t
        w = plr.w_c64(rt, inp.Vh, ytil, pb.s2, it.vr)
        got = plr.r_c64(w, inp.Vh, rt, it.alpha)
        assert np.array_equal(got.view(np.uint32), tr[t]['r'].view(np.uint32)), t
    assert np.array_equal(tr[-1]['r'].view(np.uint32), out['r'].view(np.uint32))


@pytest.mark.parametrize('case,batch', ALL, ids=ALL_IDS)
def test_case_preconditions(case, batch):
    """c. the operating point keeps the GEMMs visible."""
    _, _, out, tr, steps = _steps(case, batch)
    assert out['T'] == plr.ITERS and len(tr) == plr.ITERS
    for t, (it, _, _) in enumerate(steps):
        assert not np.isnan(tr[t]['r']).any() and not np.isnan(tr[t]['var']).any(), t
        assert it.alpha == it.alpha_raw and VAR_RATIO_MIN < it.alpha < VAR_RATIO_MAX, (t, it.alpha)
        assert it.sigma2 == it.sigma2_raw, (t, it.sigma2)
        assert it.dxdr == it.dxdr_raw and VAR_RATIO_MIN < it.dxdr < VAR_RATIO_MAX, (t, it.dxdr)
        assert it.alpha <= 0.95, (t, it.alpha)


@pytest.mark.parametrize('case,batch', ALL, ids=ALL_IDS)
def test_bars_see_a_16_bit_operand(case, batch):
    """b. the mutants against the numpy restatement, on the oracle's own iterates; the yardstick as
    the GPU test forms it (a B = 1 batch padded to the 16-row tile: persist_linear_ref._mm_c64)."""
    inp, pb, _, tr, steps = _steps(case, batch)
    pad = plr.PBM
    y64 = plr.ytil_f64(inp.U, inp.s, inp.y)
    yc = plr.ytil_c64(inp.U, inp.s, inp.y, pad)
    ny = plr.stats(yc, y64)
    my = plr.stats(plr.ytil_f64(plr.round_sig(inp.U, 16), inp.s, inp.y), y64)
    print(f'{plr.case_id(case)} B={batch} y~: numpy e_rms {ny[1]:.2e}  16-bit U x{my[1] / ny[1]:.1f}')
    assert my[1] >= 2 * plr.K_RMS * ny[1], ('y~', my, ny)
    V16 = plr.round_sig(inp.Vh, 16)
    for t, (it, x, r) in enumerate(steps):
        rt64, rtc = plr.rt_f64(x, r, it.dxdr_prev, it.ns_prev), plr.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        w64 = plr.w_f64(rt64, inp.Vh, yc, pb.s2_64, it.vr)
        wc = plr.w_c64(rtc, inp.Vh, yc, pb.s2, it.vr, pad)
        r64 = plr.r_f64(wc, inp.Vh, rt64, it.alpha)            # own w: GEMM2 alone
        rc = plr.r_c64(wc, inp.Vh, rtc, it.alpha, pad)
        nw, nr = plr.stats(wc, w64), plr.stats(rc, r64)
        mw = plr.stats(plr.w_f64(rt64, V16, yc, pb.s2_64, it.vr), w64)
        mr = plr.stats(plr.r_f64(wc, V16, rt64, it.alpha), r64)
        xw = plr.stats(plr.w_f64(rt64, inp.Vh, yc, pb.s2_64, it.vr, mm=plr.cross_sign_product), w64)
        xr = plr.stats(plr.r_f64(wc, inp.Vh, rt64, it.alpha, mm=plr.cross_sign_product), r64)
        print(f'  t={t} alpha {it.alpha:.3f}: w numpy e_rms {nw[1]:.2e} 16-bit x{mw[1] / nw[1]:.1f} cross x{xw[1] / nw[1]:.1f}'
              f' | r numpy e_rms {nr[1]:.2e} 16-bit x{mr[1] / nr[1]:.1f} cross x{xr[1] / nr[1]:.1f}')
        assert mw[1] >= 2 * plr.K_RMS * nw[1], (t, 'w', mw, nw)
        assert mr[1] >= 2 * plr.K_RMS * nr[1], (t, 'r', mr, nr)
        assert xr[1] >= 2 * plr.K_RMS * nr[1], (t, 'r cross', xr, nr)
        if t == 0:
            assert xw[1] > plr.K_RMS * nw[1], (t, 'w cross', xw, nw)


def test_round_sig_and_planes():
    """The mutants' tools: round_sig keeps `bits` significand bits (RNE on the scaled value), and the
    three bf16 planes of a float32 value add back to it exactly."""
    v = np.array([1.0 + 2.0 ** -16, 1.0 + 2.0 ** -15, -3.0 - 2.0 ** -14 - 2.0 ** -15, 0.0])
    assert np.array_equal(plr.round_sig(v, 16), np.array([1.0, 1.0 + 2.0 ** -15, -3.0 - 2.0 ** -13, 0.0]))
    a = np.random.default_rng(0).standard_normal(4096).astype(np.float32)
    b = plr.x3_planes(a)
    assert np.array_equal((b[0] + b[1] + b[2]).astype(np.float32), a)
    assert np.abs(b[2]).max() <= 2.0 ** -17 * np.abs(a).max()
