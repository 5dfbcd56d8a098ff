"""GPU: the eight-wave bf16x3 VAMP engine with the position-pair denoiser step (amp_denoise.h
denoise_step_grid2_pair: at M = 32 a lane holds positions 2j, 2j + 1 of one section instead of one
position of two sections) computes the bits it computed before.

Every per-position operation keeps its operands, type and order, the section reductions keep their
trees and the float64 var sums their chains, so a building forward and the reuse forward after it
must equal, bit for bit, what the commit before the change computed on an MI355X, against
tests/golden/pair_step_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem pair_step_bits --share-channel --dump \\
      --cases "256,8,512,17,16QAM;256,8,512,24,16QAM;256,8,512,29,16QAM;256,8,512,18,16QAM;256,8,512,19,16QAM;256,8,512,21,16QAM" \\
      --ebn0 ";;;4;16;" --nan-row ";;;;;5"

Nt = 256, Na = 8, Nr = 512, 16-QAM (the reference's table), persistent bf16x3, one channel:
  B = 17, 24, 29  the last workgroup has 1, 8 and 13 valid rows (8, 64 and 104 sections over eight
                  waves of four sections a step): one round that only two waves run, two full rounds,
                  three full rounds and a fourth that two waves run;
  B = 18 at 4 dB  runs to T = 20 (asserted on the fixture);
  B = 19 at 16 dB stops before the cap (asserted on the fixture: T = 2 building, 10 reuse);
  B = 21, y row 5 NaN: a NaN reaches the denoiser through r; the all-NaN rule fills every iteration.
Compared: r, xmmse, var, T and the 13 counters of both forwards; from the reuse forward's
per-iteration state dump every iteration's var, each wave's float64 var sum and the exchange records
(sumvar, notclose, max |logit|, min section max): the values the float32 mean would hide.
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
STEM = 'pair_step_bits'
CASES = [(256, 8, 512, B, '16QAM') for B in (17, 24, 29, 18, 19, 21)]
LOW, EARLY, NANROW = CASES[3], CASES[4], CASES[5]
NAN_ROW = 5
FIELDS = ('r', 'xmmse', 'var', 'T', 'counts')
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


def test_the_fixture_holds_the_cases_it_is_for():
    fix = _fixture()
    low, early, nan = (fix[rec.case_name(*c)] for c in (LOW, EARLY, NANROW))
    assert int(low['f0_T'][0]) == 20 and int(low['f1_T'][0]) == 20
    assert int(early['f0_T'][0]) < 20 and 1 < int(early['f1_T'][0]) < 20, (early['f0_T'], early['f1_T'])
    assert early['f1_it_var'].shape[0] == int(early['f1_T'][0])
    for i in range(2):
        assert np.isnan(nan[f'f{i}_y'][NAN_ROW]).all() and np.isfinite(np.delete(nan[f'f{i}_y'], NAN_ROW, 0)).all()
        # the reference's rule: one non-finite logit makes every section of the batch NaN
        assert np.isnan(nan[f'f{i}_xmmse']).all() and np.isnan(nan[f'f{i}_var']).all() and int(nan[f'f{i}_T'][0]) == 20
    # the dump holds what the denoiser stored, before that rule's fill: the NaN row from the first
    # iteration on, every row once the batch scalars are NaN
    assert np.isnan(nan['f1_it_var'][:, NAN_ROW]).all() and np.isnan(nan['f1_it_var'][-1]).all()
    assert np.isfinite(np.delete(nan['f1_it_var'][0], NAN_ROW, 0)).all()
    for c in CASES[:5]:
        fx = fix[rec.case_name(*c)]
        assert np.isfinite(fx['f1_it_var']).all() and np.isfinite(fx['f1_it_wsum']).all(), c
        # the dumped wave sums are the float64 sums of the float32 var of that workgroup's rows
        T, nwg = fx['f1_it_wsum'].shape[:2]
        for w in range(nwg):
            want = fx['f1_it_var'][:, 16 * w:16 * (w + 1)].astype(np.float64).sum(axis=(1, 2))
            assert np.allclose(fx['f1_it_wsum'][:, w].sum(axis=1), want, rtol=1e-12, atol=0), (c, w)


@pytest.mark.parametrize('case', CASES, ids=[rec.case_name(*c) for c in CASES])
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
