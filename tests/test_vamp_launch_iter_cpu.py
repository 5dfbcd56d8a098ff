"""No GPU: the cases, the scalar chain at eta < 1 and the bars of tests/test_gpu_vamp_launch_iter.py
(tests/vamp_launch_iter_ref.py), with oracle.vamp_detect standing in for the engine.

a. Preconditions of every case, on the oracle: four iterations without an allclose exit (the fourth
   included), no NaN; alpha, sigma2 and dxdr strictly inside their clamps; every section's max logit
   at least 100 above the engines' danger line (-700 + logit_slack below the batch's max |xi|,
   amp_common.h part_danger), so the exact-float64 section path is not entered and the float32
   logits' own error (4e-7 max |xi|) cannot move a section across it; and the shape facts the case
   table claims (parities, k < N, column / row tile counts, reduction chunks, BN = 256 at M = 128).
   The two exit cases stop by allclose before 20 iterations.
b. The restated c64 steps and persist_linear_ref.scalar_chain, run on the oracle's var means,
   reproduce the oracle's r and its alpha / sigma2 / dxdr / sigma2_tilde bit for bit at every case:
   eta = k / N < 1 at five of them (persist_linear_ref's own cases all have eta = 1).
c. Sensitivity: every mutant of vamp_launch_iter_ref.MUTANTS, applied to ONE float64 step on the
   oracle's iterates, errs by at least 2 K_RMS times the c64 step's e_rms on the same inputs in the
   phase it hits, at every case and iteration where it applies (printed per case: the mutant table).
   `vh16` is a defect of an operand that is packed once per forward and used by every iteration, and
   the GPU test holds every iteration to the bar: it is caught when ANY iteration's record crosses
   it, so per phase (w: Wt1, r: Wt2) its largest ratio over the iterations is held to 2 K_RMS (every
   ratio is printed).  Late iterations cannot carry that: where alpha passes 0.95 the r epilogue's
   1 / (1 - alpha) amplifies numpy's own error to 1e-7 .. 2e-6 and a 2^-17 operand error sinks to
   1.4 - 5 x of it (Nt8 BPSK t = 2, 3; Nt48 OOK t = 3), as test_persist_linear_cpu.py records for its
   own cases.  The M = 128 case runs at 0 dB, not at the 6 dB first chosen for it: with Na = 2 r~ is
   so small beside y~ / (s^2 + vr) that at 6 dB a 16-bit Vh moves w by 5.1 / 3.9 / 3.5 / 3.1 x numpy's
   error only (no iteration over 2 K_RMS = 6); at 0 dB it is 2.9 / 7.4 / 6.9 / 7.1 x (r: 22 - 28 x).
"""
from types import SimpleNamespace

import numpy as np
import pytest

import vamp_launch_iter_ref as vir
from oracle.amp_oracle import C64, VAR_RATIO_MAX, VAR_RATIO_MIN

IDS = [vir.case_id(c) for c in vir.CASES]
MARGIN = 100.0        # logits: how far above the danger line every section's max must stay
STATIC = ('vh16',)    # defects of an operand that is packed once per forward (vamp_pack_f32: Wt1, Wt2)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _steps(case):
    """Per iteration of the oracle's trace: the chain's record and the inputs of the linear half
    (the previous iteration's xmmse and r, the Tracker's at t = 0)."""
    inp, pb = vir.inputs(case), vir.problem(case)
    out, tr = vir.oracle_trace(case)
    chain = vir.chain_of(case, [vir.mean_var_f32(t['var']) for t in tr])
    steps = []
    for t in range(len(tr)):
        x, r = (tr[t - 1]['xmmse'], tr[t - 1]['r']) if t else vir.tracker_state(pb, tr[0]['r'].shape)
        steps.append((chain[t], x, r))
    return inp, pb, out, tr, steps


@pytest.mark.parametrize('case', vir.CASES, ids=IDS)
def test_case_preconditions(case):
    """a."""
    g = vir.geometry(case)
    for key, want in vir.CLAIMS[case].items():
        assert getattr(g, key) == want, (key, getattr(g, key), want)
    assert g.k == min(g.n, g.N) and g.N % 2 == 0
    _, pb, out, tr, steps = _steps(case)
    assert out['T'] == vir.ITERS and len(tr) == vir.ITERS
    assert vir.first_close([t['var'] for t in tr]) is None
    margins = []
    for t, (it, _, _) in enumerate(steps):
        for name in ('r', 'xmmse', 'var'):
            assert not np.isnan(tr[t][name]).any(), (t, name)
        assert it.alpha == it.alpha_raw and VAR_RATIO_MIN < it.alpha < VAR_RATIO_MAX, (t, it.alpha)
        assert it.sigma2 == it.sigma2_raw, (t, it.sigma2)
        assert it.dxdr == it.dxdr_raw and VAR_RATIO_MIN < it.dxdr < VAR_RATIO_MAX, (t, it.dxdr)
        ref = vir.denoise_f64(tr[t]['r'], np.float64(it.sigma2), pb.symbols, g.L, g.M)
        G = ref.max_abs_xi
        margins.append(float(ref.secmax.min()) - G - (vir.AMP_DANGER + vir.logit_slack(G)))
        assert margins[-1] >= MARGIN, (t, float(ref.secmax.min()), G)
    print(f'{vir.case_id(case)}: alpha {[round(float(s[0].alpha), 4) for s in steps]}  '
          f'section max above the danger line by {[round(m, 1) for m in margins]}')


@pytest.mark.parametrize('case', vir.EXIT_CASES, ids=[vir.case_id(c) for c in vir.EXIT_CASES])
def test_exit_cases_stop_early(case):
    out, tr = vir.oracle_trace(case, vir.EXIT_ITERS)
    T = vir.first_close([t['var'] for t in tr])
    print(f'{vir.case_id(case)}: the oracle stops at T = {out["T"]}')
    assert T == out['T'] and 1 < T < vir.EXIT_ITERS and not np.isnan(out['r']).any()


@pytest.mark.parametrize('case', vir.CASES, ids=IDS)
def test_restatement_and_chain_reproduce_the_oracle(case):
    """b. bit identity with vamp_detect's trace, eta < 1 included."""
    inp, pb, out, tr, steps = _steps(case)
    ytil = vir.ytil_c64(inp.U, inp.s, inp.y)
    for t, (it, x, r) in enumerate(steps):
        for name, got in (('alpha', it.alpha), ('sigma2', it.sigma2), ('dxdr', it.dxdr), ('sigma2_tilde', it.s2t_next)):
            assert np.float32(got).tobytes() == np.float32(tr[t][name]).tobytes(), (t, name, got, tr[t][name])
        rt = vir.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        if t:
            assert np.array_equal(_bits(rt), _bits(tr[t - 1]['r_tilde'])), t
        got = vir.r_c64(vir.w_c64(rt, inp.Vh, ytil, pb.s2, it.vr), inp.Vh, rt, it.alpha)
        assert np.array_equal(_bits(got), _bits(tr[t]['r'])), t
    assert np.array_equal(_bits(tr[-1]['r']), _bits(out['r']))
    assert vir.first_close([t['var'] for t in tr]) is None


@pytest.mark.parametrize('case', vir.CASES, ids=IDS)
def test_oracle_passes_the_gpu_bars(case):
    """The GPU test's own arithmetic (vamp_launch_iter_ref.records, last_scalars, first_close) with
    the oracle's iterates as the engine's state: inside every bar, scalars bit for bit."""
    inp, pb, out, tr, steps = _steps(case)
    ytil = vir.ytil_c64(inp.U, inp.s, inp.y)
    fws = []
    for t, (it, x, r) in enumerate(steps):
        w = vir.w_c64(vir.rt_c64(x, r, it.dxdr_prev, it.ns_prev), inp.Vh, ytil, pb.s2, it.vr)
        fws.append(SimpleNamespace(r=tr[t]['r'], x=tr[t]['xmmse'], var=tr[t]['var'], w=w, ytil=ytil))
    chain = vir.chain_of(case, [vir.mean_var_f32(fw.var) for fw in fws])
    for T in range(1, vir.ITERS + 1):
        want = [tr[T - 1]['sigma2'], tr[T - 1]['dxdr']]
        assert np.array_equal(_bits(vir.last_scalars(chain, T, 0)[2:]), _bits(np.array(want, np.float32))), T
    lin, den = vir.records(case, fws, chain)
    vir.show(f'oracle {vir.case_id(case)}', lin, den)
    assert len(lin) == 1 + 2 * vir.ITERS and len(den) == vir.ITERS
    vir.assert_bars(f'oracle {vir.case_id(case)}', lin, den)
    if case == vir.SHARD_CASE:      # a slice: r and the denoiser only, the chain from the whole batch's means
        rows = slice(vir.SHARD_ROWS, 2 * vir.SHARD_ROWS)
        part = [SimpleNamespace(r=f.r[rows], x=f.x[rows], var=f.var[rows], w=f.w[rows]) for f in fws]
        lin, den = vir.records(case, part, chain, rows=rows, linear_half=False)
        assert [r.what for r in lin] == ['r'] * vir.ITERS
        vir.assert_bars(f'oracle slice {vir.case_id(case)}', lin, den)


def mutant_table(case):
    """[(mutant, phase, t, e_rms of the mutant over the c64 step's)] over every applicable mutant."""
    inp, pb, _, tr, steps = _steps(case)
    pad = vir.PAD
    rows = []
    y64 = vir.ytil_f64(inp.U, inp.s, inp.y)
    yc = vir.ytil_c64(inp.U, inp.s, inp.y, pad)
    ny = vir.stats(yc, y64)[1]
    assert ny > 0
    for m in vir.MUTANTS:
        ym = vir.mutant_ytil(m, case, inp, inp.y) if vir.applies(m, case) else None
        if ym is not None:
            rows.append((m, 'y~', 0, vir.stats(ym, y64)[1] / ny, ny))
    for t, (it, x, r) in enumerate(steps):
        rt64, rtc = vir.rt_f64(x, r, it.dxdr_prev, it.ns_prev), vir.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        w64 = vir.w_f64(rt64, inp.Vh, yc, pb.s2_64, it.vr)
        wc = vir.w_c64(rtc, inp.Vh, yc, pb.s2, it.vr, pad)
        r64 = vir.r_f64(wc, inp.Vh, rt64, it.alpha)               # the step's own w: GEMM2 alone
        rc = vir.r_c64(wc, inp.Vh, rtc, it.alpha, pad)
        nw, nr = vir.stats(wc, w64)[1], vir.stats(rc, r64)[1]
        assert nw > 0 and nr > 0
        prev_alpha = steps[t - 1][0].alpha if t else None
        for m in vir.MUTANTS:
            if not vir.applies(m, case, t):
                continue
            wm = vir.mutant_w(m, case, inp, pb, rt64, yc, it)
            if wm is not None:
                rows.append((m, 'w', t, vir.stats(wm, w64)[1] / nw, nw))
            rm = vir.mutant_r(m, case, inp, wc, rt64, it, prev_alpha)
            if rm is not None:
                rows.append((m, 'r', t, vir.stats(rm, r64)[1] / nr, nr))
    return rows


@pytest.mark.parametrize('case', vir.CASES, ids=IDS)
def test_bars_see_the_mutants(case):
    """c."""
    rows = mutant_table(case)
    seen = {m for m, *_ in rows}
    assert seen == {m for m in vir.MUTANTS if vir.applies(m, case)}, seen
    for m, phase, t, ratio, yard in rows:
        print(f'{vir.case_id(case)} {m:5s} {phase:2s} t={t}: x{ratio:.3g} of numpy\'s e_rms {yard:.2e}')
    bad = [(m, phase, t, ratio) for m, phase, t, ratio, _ in rows if m not in STATIC and not ratio >= 2 * vir.K_RMS]
    assert not bad, bad
    for m in STATIC:
        for phase in ('w', 'r'):
            best = max(ratio for mm, ph, _, ratio, _ in rows if (mm, ph) == (m, phase))
            assert best >= 2 * vir.K_RMS, (m, phase, best)


def test_yardstick_pads_a_single_row():
    """The c64 products of a B = 1 batch are matrix products of PAD rows, first row returned."""
    case = vir.CASES[4]
    assert case.B == 1
    inp = vir.inputs(case)
    a = vir.ytil_c64(inp.U, inp.s, inp.y, vir.PAD)
    yp = np.zeros((vir.PAD, inp.y.shape[1]), C64)
    yp[:1] = inp.y
    assert a.shape == (1, inp.U.shape[1]) and np.array_equal(_bits(a), _bits(vir.ytil_c64(inp.U, inp.s, yp)[:1]))
