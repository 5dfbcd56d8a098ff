"""No GPU: the float64 step, the numpy yardstick and the operating points of the per-iteration
BAMP / SCAMP tests (tests/launch_iter_ref.py; test_gpu_bamp_iter.py, test_gpu_scamp_iter.py,
test_gpu_scamp_persist_iter.py), with oracle.bamp_detect / scamp_detect standing in for the engine.

a. Consistency: the restated c64 step, iterated on its own outputs through the oracle's denoiser,
   reproduces the oracle's trace (xmap, z, xmmse, var / psi) bit for bit at every case.
b. Preconditions of every operating point, on the oracle: four iterations without an allclose
   exit (the fourth included), no NaN, and every section's normaliser finite and positive in the
   float64 denoiser, so that the engines' exact-float64 section path is not entered.  The oracle's own
   records sit inside the GPU tests' bars (its linear ratios are 1 by construction at B > 1).
   SCAMP with 16QAM is run at 0 dB: from 1 dB (ISI shape) / 3 dB (persistent shapes) the reference's
   float64 denoiser underflows to 0 / 0 by iteration 2 or 3 (max |xi| > 5000).
c. Sensitivity: each defect of the float64 step, applied in ONE iteration to the healthy state,
   errs in xmap by at least 2 K_RMS times the c64 step's rms on the same inputs in the iteration
   where it first acts (and is printed for every iteration):
     h16      the operator rounded to 16 significand bits          t = 1   16.7 - 81 x
     onsager  the Onsager term with the new u / phi                BAMP t = 2 (y - z_0 = 0 at t = 1),
                                                                   SCAMP t = 1         > 2e6 x
     lastcol  the last column of |H|^2 missing from v (BAMP)       t = 1   6.8e3 - 4.9e5 x
     granule  64 reduction floats of the first column tile's band  t = 1   3.2e4 - 2.5e6 x
              dropped from the A^H product (ISI cases)
     offband  the band cases' extra entry ignored                  t = 1   3.2e4 - 1.1e5 x
     tau1e5   one coupling block's tau off by 1e-5 (SCAMP)         t = 1   20 - 99 x
   and `tau = cov` in place of cov / 2 in the denoiser moves xmmse by 24 - 1e5 times the
   denoiser bar; psi formed from an xmmse rounded to 16 significand bits errs by 30 - 125 times the
   oracle's float32 line (forwards with fewer than 16 psi values: over all iterations at once, as
   launch_iter_ref.scamp_records judges them).  Later iterations stay above 2 K_RMS as well except `lastcol` at iteration 4 of
   Nt64-Lin8-B35 (4.3 x): var has converged to ~0 there and v with it; the mutant is caught at
   iterations 1 to 3 (> 2.8e3 x).  `tau1e5` stays above 10 x and `h16` above 16 x at every iteration.
"""
import numpy as np
import pytest

import launch_iter_ref as lir
from oracle.amp_oracle import C64, F32, block_denoise, scamp_denoise
from persist_denoiser_cases import denoise_f64

BAMP = [(c, 'bamp') for c in lir.BAMP_CASES]
SCAMP = [(c, 'scamp') for c in lir.SCAMP_CASES + lir.PERSIST_CASES]
ALL = BAMP + SCAMP
IDS = [f'{a}-{lir.case_id(c)}' for c, a in ALL]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _start(case, algo, inp):
    B, N = inp.y.shape[0], inp.A.shape[1]
    return np.zeros((B, N), C64), (np.ones((B, N), F32) if algo == 'bamp' else np.ones((B, case.Lin), F32))


def _outs(case, algo):
    out, tr = lir.oracle_trace(case, algo)
    key = 'var' if algo == 'bamp' else 'psi'
    return out, tr, [(t['xmap'], t['xmmse'], t[key]) for t in tr]


@pytest.mark.parametrize('case,algo', ALL, ids=IDS)
def test_restatement_reproduces_the_oracle(case, algo):
    """a. bit identity of the iterated c64 step with the oracle's trace."""
    inp = lir.inputs(case)
    cfg = lir.oracle_config(case)
    out, tr, _ = _outs(case, algo)
    xm, sv = _start(case, algo, inp)
    st = (lir.bamp_state if algo == 'bamp' else lir.scamp_state)(inp.y, C64)
    for t, rec in enumerate(tr):
        if algo == 'bamp':
            st = lir.bamp_step_c64(inp.A, inp.y, inp.noise_var, xm, sv, st)
            xm, sv = block_denoise(st.xmap, (st.cov / F32(2)).astype(F32), cfg)
            assert np.array_equal(_bits(st.u), _bits(rec['u'])), t
            assert np.array_equal(_bits(sv), _bits(rec['var'])), t
        else:
            st = lir.scamp_step_c64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, sv, st)
            xm = scamp_denoise(st.xmap, (st.tau / F32(2)).astype(F32), cfg)
            sv = lir.psi_c64(xm, case)
            assert np.array_equal(_bits(sv), _bits(rec['psi'])), t
        assert np.array_equal(_bits(st.xmap), _bits(rec['xmap'])), t
        assert np.array_equal(_bits(st.z), _bits(rec['z'])), t
        assert np.array_equal(_bits(xm), _bits(rec['xmmse'])), t
    assert np.array_equal(_bits(tr[-1]['xmap']), _bits(out['xmap']))


@pytest.mark.parametrize('case,algo', ALL, ids=IDS)
def test_case_preconditions(case, algo):
    """b. the operating point runs four full iterations on the ordinary denoiser path, and the
    oracle itself passes the GPU tests' bars."""
    inp = lir.inputs(case)
    out, tr, outs = _outs(case, algo)
    assert out['T'] == lir.T and len(tr) == lir.T
    _, sv0 = _start(case, algo, inp)
    assert lir.first_close([o[2] for o in outs], sv0) is None
    for t, o in enumerate(outs):
        assert not any(np.isnan(a).any() for a in o), t
    lin, den = (lir.bamp_records if algo == 'bamp' else lir.scamp_records)(case, outs)
    lir.show(f'{algo} {lir.case_id(case)} oracle', lin, den)
    # the normalisers, on the float64 step's cov / tau (what the GPU tests' denoiser reference takes)
    xm, sv = _start(case, algo, inp)
    st = (lir.bamp_state if algo == 'bamp' else lir.scamp_state)(inp.y, np.complex128)
    for t, (xmap, xmmse, s_t) in enumerate(outs):
        if algo == 'bamp':
            st = lir.bamp_step_f64(inp.A, inp.y, inp.noise_var, xm, sv, st)
            tau = st.cov / 2.0
        else:
            st = lir.scamp_step_f64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, sv, st)
            tau = st.tau / 2.0
        assert lir.normalisers_ok(xmap, tau, case), t
        xm, sv = xmmse, s_t
    lir.assert_bars(f'{algo} {lir.case_id(case)} oracle', lin, den)


def _applies(mut, case, inp):
    if mut == 'granule':     # a band, and a first column tile whose band holds more than one granule
        return case.Lin > 1 and case.Lh < case.Lin and case.Nr * case.Lh > 32 and inp.A.shape[1] >= 64
    if mut == 'offband':
        return case.band
    return True


def _first_acts(mut, algo):
    return 2 if (mut == 'onsager' and algo == 'bamp') else 1


@pytest.mark.parametrize('case,algo', ALL, ids=IDS)
def test_bars_see_the_mutants(case, algo):
    """c. every mutant of the float64 step against the c64 step's own error, on the oracle's
    iterates; the yardstick as the GPU tests form it (B = 1 padded to PAD rows)."""
    inp = lir.inputs(case)
    _, _, outs = _outs(case, algo)
    sym = lir.oracle_config(case).symbols
    L, M = case.Na * case.Lin, case.Nt // case.Na
    muts = [m for m in (lir.BAMP_MUTANTS if algo == 'bamp' else lir.SCAMP_MUTANTS) if _applies(m, case, inp)]
    xm, sv = _start(case, algo, inp)
    new = lir.bamp_state if algo == 'bamp' else lir.scamp_state
    s64, s32 = new(inp.y, np.complex128), new(inp.y, C64)
    pooled = algo == 'scamp' and inp.y.shape[0] * case.Lin < lir.PAD
    ey, em = [], []
    for t, (xmap, xmmse, s_t) in enumerate(outs, 1):
        if algo == 'bamp':
            step = lambda mut=None: lir.bamp_step_f64(inp.A, inp.y, inp.noise_var, xm, sv, s64, mut, case)   # noqa: E731
            s32 = lir.bamp_step_c64(inp.A, inp.y, inp.noise_var, xm, sv, s32, lir.PAD)
        else:
            step = lambda mut=None: lir.scamp_step_f64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, sv, s64, mut)   # noqa: E731
            s32 = lir.scamp_step_c64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, sv, s32, lir.PAD)
        h = step()
        yard = lir.xstats(s32.xmap, h.xmap)
        row = []
        for m in muts:
            ratio = lir.xstats(step(m).xmap, h.xmap).rms / yard.rms
            row.append(f'{m} x{ratio:.3g}')
            if t == _first_acts(m, algo):
                assert ratio >= 2 * lir.K_RMS, (m, t, ratio)
        # the denoiser with tau = cov (tau_use) where the reference halves it
        tau = h.cov if algo == 'bamp' else h.tau
        ref, mut = denoise_f64(xmap, tau / 2.0, sym, L, M), denoise_f64(xmap, tau, sym, L, M)
        d = lir.denoiser_record('tau', t, mut.x, mut.var if algo == 'bamp' else None, ref)
        row.append(f'tau=cov x{d.x:.3g} of the denoiser bar')
        assert d.x >= 2 * lir.K_RMS, (t, d.x)
        if algo == 'scamp':      # psi from an xmmse rounded to 16 significand bits
            p64, sub = lir.psi_f64(xmmse, case)
            ey.append(lir.psi_yardstick(xmmse, case, lir.PAD))
            em.append(lir.psi_errors(lir.psi_f64(lir.round_sig(xmmse, 16), case)[0], p64, sub))
            if not pooled:
                ratio = lir.psi_stats(em[-1]).rms / lir.psi_stats(ey[-1]).rms
                row.append(f'psi xm16 x{ratio:.3g}')
                assert ratio >= 2 * lir.K_RMS, (t, ratio)
        print(f'{algo} {lir.case_id(case)} t={t}: numpy rms {yard.rms:.2e}  ' + '  '.join(row))
        s64 = h
        xm, sv = xmmse, s_t
    if pooled:                   # one psi record per forward, as scamp_records forms it
        ratio = lir.psi_stats(np.concatenate(em)).rms / lir.psi_stats(np.concatenate(ey)).rms
        print(f'{algo} {lir.case_id(case)} all iterations: psi xm16 x{ratio:.3g}')
        assert ratio >= 2 * lir.K_RMS, ratio


def test_statistics():
    """The block statistic finds a defect confined to one edge block that the global rms averages
    away, and the psi statistic is relative to the subtracted sum."""
    rng = np.random.default_rng(0)
    ref = rng.standard_normal((70, 200)) + 1j * rng.standard_normal((70, 200))
    noise = 1e-7 * (rng.standard_normal(ref.shape) + 1j * rng.standard_normal(ref.shape))
    bad = noise.copy()
    bad[64:, 192:] *= 10                      # the last (6 x 8) block
    a, b = lir.xstats(ref + noise, ref), lir.xstats(ref + bad, ref)
    assert b.rms < 1.2 * a.rms and b.blk > 5 * a.blk
    r = lir.record('xmap', 1, b, a)
    assert not lir.linear_ok(r) and lir.linear_ok(lir.record('xmap', 1, a, a))
    s = lir.psi_stats(lir.psi_errors(np.array([[1e-9 + 1e-8]]), np.array([[1e-9]]), np.array([[1.0]])))
    assert abs(s.rms - 1e-8) < 1e-15 and abs(s.max - 1e-8) < 1e-15
