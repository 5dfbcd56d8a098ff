"""GPU: the eight-wave bf16x3 VAMP engine with the item forms of the A-operand writers
(amp_persist.h x3_store8_item / x3_store_acc_item: the bf16 split without per-value finite tests,
one wave-uniform branch per item, plane and row offsets as DS immediates) computes the bits it
computed before.

The pieces of a finite value are unchanged and a wave that holds a non-finite value runs the
former instructions, so a building forward and the reuse forward after it must equal, bit for
bit, what the commit before the change computed on an MI355X, against
tests/golden/a_operand_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem a_operand_bits --share-channel --dump --dump-wr \\
      --cases "256,8,512,17,16QAM;256,8,512,20,QPSK;256,4,512,24,16QAM;256,16,512,24,16QAM" \\
      --inf-entry "3,11;;;"

Nt = 256, Nr = 512, persistent bf16x3 (eight waves), one channel:
  16-QAM, Na = 8, B = 17, y[3, 11] = +inf: y~ and so w are non-finite in row 3 alone at iteration 0
                  (asserted on the fixture): the masked form in some waves beside the unmasked one;
  QPSK, Na = 8, B = 20: another eight-wave alphabet through the same two writers;
  16-QAM, Na = 4 and Na = 16, B = 24: other section lengths (M = 64, 16).
Compared: r, xmmse, var, T and the 13 counters of both forwards, and from both forwards' state
dumps every iteration's var, wave sums and exchange records, the GEMM1 epilogue's w and the GEMM2
epilogue's r (the first two iterations whole, every iteration as a CRC-32 per trial row, with
the finiteness of every w row).
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
STEM = 'a_operand_bits'
CASES = [(256, 8, 512, 17, '16QAM'), (256, 8, 512, 20, 'QPSK'), (256, 4, 512, 24, '16QAM'), (256, 16, 512, 24, '16QAM')]
INF_CASE, INF_ROW, INF_COL = CASES[0], 3, 11
FIELDS = ('r', 'xmmse', 'var', 'T', 'counts')
DUMPED = ('it_var', 'it_wsum', 'it_gran', 'it_w', 'it_r', 'it_wcrc', 'it_rcrc', 'it_wfin')

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
    inf = fix[rec.case_name(*INF_CASE)]
    for i in range(2):
        y = inf[f'f{i}_y'].reshape(INF_CASE[3], -1)
        assert np.isposinf(y[INF_ROW, INF_COL].real) and np.isfinite(np.delete(y.reshape(-1), INF_ROW * y.shape[1] + INF_COL)).all()
        # iteration 0: w of row 3 is non-finite (the masked form runs in the waves that hold it),
        # every other row of the batch is finite (their waves stay on the unmasked form)
        wfin = inf[f'f{i}_it_wfin']
        assert not wfin[0, INF_ROW] and np.delete(wfin[0], INF_ROW).all(), wfin[0]
        w0 = inf[f'f{i}_it_w'][0]
        assert not np.isfinite(w0[INF_ROW]).all() and np.isfinite(np.delete(w0, INF_ROW, 0)).all()
        assert np.array_equal(rec.row_crc(inf[f'f{i}_it_w']), inf[f'f{i}_it_wcrc'][:rec.WR_FULL])
    for c in CASES[1:]:
        fx = fix[rec.case_name(*c)]
        for i in range(2):
            assert fx[f'f{i}_it_wfin'].all() and np.isfinite(fx[f'f{i}_r']).all(), (c, i)
            assert fx[f'f{i}_it_wcrc'].shape == (int(fx[f'f{i}_T'][0]), c[3])


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
    res = rec.run_case(case, inp, device, dump=True, wr=True)
    bad = []
    for i, (made, got) in enumerate(res):
        want_made = tuple(int(v) for v in fx[f'f{i}_made'])
        assert made == want_made == ((1, 0), (0, 1))[i], (i, made, want_made)
        names = FIELDS + DUMPED
        want = {k: fx[f'f{i}_{k}'] for k in names}
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
