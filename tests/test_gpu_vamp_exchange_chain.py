"""GPU: the eight-wave bf16x3 VAMP engine with the key forms of its exchange reduction
(amp_persist.h part_publish_keys / part_gather_keys: max|xi| and the minimum section maximum as
integer extremes over fkey keys wherever no NaN is among them; amp_vamp.h vamp_advance_head_pow2:
the mean's quotient by a power of two as a scaling) computes the bits it computed before.

A building forward and the reuse forward after it must equal, bit for bit, what the commit before
the change computed on an MI355X, against tests/golden/exchange_chain_bits.part*.npz, recorded on
that commit, through its library, with

  python tools/record_forward_bits.py --stem exchange_chain_bits --share-channel --dump \\
      --cases "256,8,512,17,16QAM;256,8,512,29,16QAM;256,8,512,32,16QAM;256,8,512,24,QPSK;256,8,512,19,8PSK;\\
256,8,512,18,16QAM;256,8,512,20,16QAM;256,8,512,21,16QAM;256,8,512,22,16QAM;256,8,512,23,16QAM;256,8,512,25,16QAM" \\
      --ebn0 ";;;;;16;4;;;;" --nan-row ";;;;;;;5;;;" --inf-entry ";;;;;;;;3,11;;" --scale-y ";;;;;;;;;4.25;4.5"

Nt = 256, Na = 8, Nr = 512, persistent bf16x3 (eight waves), one channel, two or three workgroups:
  16-QAM B = 17, 29: a partial last workgroup, Bmean N not a power of two (the division);
  16-QAM B = 32: Bmean N = 2^13 (the scaling);
  QPSK B = 24 and 8-PSK B = 19: the K = 4 kernel and one that is no product grid (K = 8);
  16-QAM B = 18 at 16 dB stops at T = 2, B = 20 at 4 dB runs to the cap T = 20;
  16-QAM B = 21 with row 5 of y NaN, B = 22 with y[3, 11] = +inf: the gates' shared path and the
      all-NaN rule (nan_state 1);
  16-QAM B = 25 with y scaled by 4.5: iteration 1 of the dumped reuse forward is in danger with a
      finite max|xi|, so the exact-float64 rare path runs (and, as in the reference, leaves sections
      whose softmax underflows NaN: the all-NaN rule from iteration 2 on); B = 23 with y scaled by
      4.25, the smallest factor tried on the parent that reaches the rare path at all (4 does not):
      its building forward does and ends NaN (nan_state 1), its reuse forward stays clear and finite.
T and nan_state are asserted on the fixture itself.  Compared: r, xmmse, var, T, nan_state and the 13
counters of both forwards, and from the reuse forward's state dump every iteration's var, wave sums
and exchange records.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_forward_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEM = 'exchange_chain_bits'
# (case, T of both forwards, nan_state of both forwards)
CASES = [((256, 8, 512, 17, '16QAM'), (20, 20), (0, 0)), ((256, 8, 512, 29, '16QAM'), (20, 20), (0, 0)),
         ((256, 8, 512, 32, '16QAM'), (20, 20), (0, 0)), ((256, 8, 512, 24, 'QPSK'), (2, 2), (0, 0)),
         ((256, 8, 512, 19, '8PSK'), (20, 20), (0, 0)), ((256, 8, 512, 18, '16QAM'), (2, 2), (0, 0)),
         ((256, 8, 512, 20, '16QAM'), (20, 20), (0, 0)), ((256, 8, 512, 21, '16QAM'), (20, 20), (1, 1)),
         ((256, 8, 512, 22, '16QAM'), (20, 20), (1, 1)), ((256, 8, 512, 23, '16QAM'), (20, 20), (1, 0)),
         ((256, 8, 512, 25, '16QAM'), (20, 20), (1, 1))]
NAN_CASE, NAN_ROW = CASES[7][0], 5
INF_CASE, INF_ROW, INF_COL = CASES[8][0], 3, 11
RARE_CASE, RARE_NAN_CASE = CASES[9][0], CASES[10][0]
FIELDS = ('r', 'xmmse', 'var', 'T', 'nan_state', 'counts')
DUMPED = ('it_var', 'it_wsum', 'it_gran')

_FIX = {}


def _fixture():
    """{case or 'shared': {field: array}} of the parts, row blocks ('field@i') joined (read once)."""
    if not _FIX:
        raw, k = {}, 0
        while os.path.exists(os.path.join(GOLDEN, f'{STEM}.part{k}.npz')):
            z = np.load(os.path.join(GOLDEN, f'{STEM}.part{k}.npz'))
            raw.update({n: z[n] for n in z.files})
            k += 1
        assert k, 'no fixture parts'
        blocks = {}
        for n, a in raw.items():
            base, _, i = n.partition('@')
            blocks.setdefault(base, []).append((int(i or 0), a))
        for base, bl in blocks.items():
            case, field = base.split('/', 1)
            bl.sort(key=lambda p: p[0])
            _FIX.setdefault(case, {})[field] = bl[0][1] if len(bl) == 1 else np.concatenate([a for _, a in bl], axis=0)
    return _FIX


def _diff(got, want, names):
    """Every differing array and its first differing index (bitwise)."""
    bad = []
    for name in names:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}')
            continue
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            bad.append(f'{name}: first difference at flat index {i} of {a.size} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r}), {int(ne.sum())} bytes differ')
    return bad


def _extremes(gran):
    """(max|xi|, min section max) per iteration over the workgroups' records, float64."""
    return (gran[..., 4].copy().view(np.float32).astype(np.float64).max(axis=1),
            gran[..., 5].copy().view(np.float32).astype(np.float64).min(axis=1))


def test_the_fixture_holds_the_cases_it_is_for():
    fix = _fixture()
    for case, T, ns in CASES:
        fx = fix[rec.case_name(*case)]
        assert case[3] <= 3 * rec.PBM
        for i in range(2):
            assert int(fx[f'f{i}_T'][0]) == T[i] and int(fx[f'f{i}_nan_state'][0]) == ns[i], (case, i)
        assert fx['f1_it_gran'].shape == (T[1], -(-case[3] // rec.PBM), 8)
        for i in range(2):   # a forward ends NaN exactly when its nan_state says so
            finite = all(np.isfinite(fx[f'f{i}_{k}']).all() for k in ('r', 'xmmse', 'var'))
            assert finite == (ns[i] == 0), (case, i)
    N = 256
    assert [rec_pow2(c[3] * N) for c, _, _ in CASES[:3]] == [False, False, True]
    for i in range(2):
        y = fix[rec.case_name(*NAN_CASE)][f'f{i}_y'].reshape(NAN_CASE[3], -1)
        assert np.isnan(y[NAN_ROW]).all() and np.isfinite(np.delete(y, NAN_ROW, 0)).all()
        y = fix[rec.case_name(*INF_CASE)][f'f{i}_y'].reshape(INF_CASE[3], -1)
        assert np.isposinf(y[INF_ROW, INF_COL].real) and np.isfinite(np.delete(y.reshape(-1), INF_ROW * y.shape[1] + INF_COL)).all()
    # the NaN and inf cases publish a NaN max|xi| in every iteration (the gates' shared path)
    for c in (NAN_CASE, INF_CASE):
        assert np.isnan(_extremes(fix[rec.case_name(*c)]['f1_it_gran'])[0]).all()
    mx, mn = _extremes(fix[rec.case_name(*RARE_CASE)]['f1_it_gran'])
    assert np.isfinite(mx).all() and not (mn - mx < -700.0 + 1e-5 * mx + 2.0).any()
    # the 4.5 case: iteration 1 is in danger with a finite max|xi| (the exact path runs), NaN from 2 on
    mx, mn = _extremes(fix[rec.case_name(*RARE_NAN_CASE)]['f1_it_gran'])
    assert np.isfinite(mx[:2]).all() and mn[1] - mx[1] < -700.0 + 1e-5 * mx[1] + 2.0 and np.isnan(mx[2:]).all()
    # 16 dB and 4 dB carry their own SNR
    assert 'SNR' in fix[rec.case_name(*CASES[5][0])] and 'SNR' in fix[rec.case_name(*CASES[6][0])]


def rec_pow2(v):
    return v > 0 and v & (v - 1) == 0


@pytest.mark.parametrize('case', [c for c, _, _ in CASES], ids=[rec.case_name(*c) for c, _, _ in CASES])
def test_forward_bits_equal_the_parent_commits(device, case):
    fix = _fixture()
    fx = fix[rec.case_name(*case)]
    ch = fix['shared']
    snr = fx['SNR'] if 'SNR' in fx else ch['SNR']       # its own Eb/N0, or the channel's
    inp = dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
               SNR=float(snr[0]),
               eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                         y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(2)])
    res = rec.run_case(case, inp, device, dump=True)
    bad = []
    for i, (made, got) in enumerate(res):
        want_made = tuple(int(v) for v in fx[f'f{i}_made'])
        assert made == want_made == ((1, 0), (0, 1))[i], (i, made, want_made)
        names = FIELDS + (DUMPED if i == 1 else ())
        want = {k: fx[f'f{i}_{k}'] for k in names}
        if i == 1:
            # words 3 and 7 of a record are the launch's generation tag (it counts the process's
            # forwards): equal to each other and non-zero, and left out of the comparison
            g = got['it_gran']
            assert (g[..., 3] == g[..., 7]).all() and (g[..., 3] != 0).all()
            got['it_gran'], want['it_gran'] = g.copy(), want['it_gran'].copy()
            got['it_gran'][..., [3, 7]] = 0
            want['it_gran'][..., [3, 7]] = 0
        print(f'forward {i}: T {int(got["T"][0])} (fixture {int(want["T"][0])})')
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want, names)]
    assert not bad, '\n'.join(bad)
