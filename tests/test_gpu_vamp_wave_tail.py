"""GPU: the eight-wave bf16x3 VAMP engine at one workgroup per CU with the LMMSE scalar tail formed by
one wave per workgroup (AMP_SCALAR_TAIL = 2: vamp_advance_tail in one wave's GEMM1, the record
{vr, alpha, inv1ma, sigma2, inv_sigma2} and the 256 reciprocals 1 / (s^2 + vr) handed to the other
waves through LDS behind GEMM1's closing barrier, the w epilogue's scale read from that table
instead of divided again) computes the bits it computed before.

Every floating-point operation keeps its operands, its type and its order, so a building forward
and the two reuse forwards after it must equal, bit for bit, what the commit before the change
computed on an MI355X: r, xmmse and var bits, T, all 13 counters and status.last_scalar, and from
the state dump (amp_vamp_debug_dump), per iteration, every trial row of the GEMM1 epilogue's w (one
CRC-32 per row; w carries vr and the reciprocal of its column) and every workgroup's 1 / sigma2 as
its denoiser took it.  A wave that read the hand-off early or late would damage only its own 32
columns of one iteration's w, or its own part of one denoiser pass: the dump is where that shows.
Against tests/golden/wave_tail_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem wave_tail_bits --share-channel --tail --forwards 3 \\
      --cases "256,8,512,17,16QAM;256,8,512,32,QPSK;256,8,512,24,16PSK;256,8,512,17,16QAM;256,8,512,17,16QAM;256,8,512,17,16QAM;256,8,512,17,16QAM" \\
      --ebn0 ";0;10;;;16;" --iters ";;;1;2;;" --tags ";;;it1;it2;db16;nan" --nan-row ";;;;;;5"

(the Nt=256, Nr=512 cases on one channel, stored once).
  16QAM_256_8_512_17        the flagship's instantiation, 20 iterations; the second workgroup has one valid row;
  QPSK_256_8_512_32         the KK = 4 sibling at 0 dB, where the recorded forwards stop before the cap
                            (asserted: fixture T < 20); the stop record carries no tail;
  16PSK_256_8_512_24        the non-grid eight-wave instantiation;
  16QAM_256_8_512_17#it1    iterations = 1: no tail ever (iteration 0's record is vamp_first_iter's);
  16QAM_256_8_512_17#it2    iterations = 2: exactly one tail; on a reuse forward, which has no GEMM1 at
                            t = 0, it stands in the first GEMM1 of the launch;
  16QAM_256_8_512_17#db16   16 dB: the building and the first reuse forward stop at T = 2 (asserted; the
                            second reuse forward, on its own y, runs to the cap);
  16QAM_256_8_512_17#nan    row 5 of y is NaN: vr, the record and the reciprocals are not finite from
                            iteration 1 on and go through the table as they are (asserted: the fixture's
                            1 / sigma2 is NaN in some iteration).
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
STEM = 'wave_tail_bits'
QAM = (256, 8, 512, 17, '16QAM')
# (case, tag, iteration cap)
CASES = [(QAM, '', 20), ((256, 8, 512, 32, 'QPSK'), '', 20), ((256, 8, 512, 24, '16PSK'), '', 20),
         (QAM, 'it1', 1), (QAM, 'it2', 2), (QAM, 'db16', 20), (QAM, 'nan', 20)]
FORWARDS = 3
FIELDS = ('r', 'xmmse', 'var', 'T', 'counts', 'last_scalar', 'it_wcrc', 'it_wfin', 'it_inv')

_FIX = {}


def _name(case, tag):
    return rec.case_name(*case) + (f'#{tag}' if tag else '')


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


def _diff(got, want):
    """Every differing array and its first differing index (bitwise)."""
    bad = []
    for name in FIELDS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}')
            continue
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            where = f' = [iteration, row or workgroup] {np.unravel_index(i, a.shape)}' if name.startswith('it_') else ''
            bad.append(f'{name}: first difference at flat index {i} of {a.size}{where} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r})')
    return bad


def test_the_fixture_holds_the_cases_it_is_for():
    fix = _fixture()
    T = {_name(c, tag): [int(fix[_name(c, tag)][f'f{i}_T'][0]) for i in range(FORWARDS)] for c, tag, _ in CASES}
    print(T)
    assert T[_name(QAM, '')] == [20] * FORWARDS
    assert all(t < 20 for t in T[_name((256, 8, 512, 32, 'QPSK'), '')])
    assert T[_name(QAM, 'it1')] == [1] * FORWARDS and T[_name(QAM, 'it2')] == [2] * FORWARDS
    assert T[_name(QAM, 'db16')][:2] == [2, 2], 'the building and the first reuse forward stop at T = 2'
    nan = fix[_name(QAM, 'nan')]
    for i in range(FORWARDS):
        assert np.isnan(nan[f'f{i}_y'].reshape(QAM[3], -1)[5]).all()
        assert np.isnan(nan[f'f{i}_it_inv']).any() and not nan[f'f{i}_it_wfin'].all()
    for c, tag, _ in CASES:   # one record per (iteration, trial) and per (iteration, workgroup)
        fx = fix[_name(c, tag)]
        for i in range(FORWARDS):
            t = int(fx[f'f{i}_T'][0])
            assert fx[f'f{i}_it_wcrc'].shape == (t, c[3]) and fx[f'f{i}_it_inv'].shape == (t, -(-c[3] // rec.PBM))


@pytest.mark.parametrize('case,tag,iters', CASES, ids=[_name(c, tag) for c, tag, _ in CASES])
def test_forward_and_dump_bits_equal_the_parent_commits(device, case, tag, iters):
    fix = _fixture()
    fx = fix[_name(case, tag)]
    ch = fx if 'U' in fx else fix['shared']             # its own channel, or the shared one
    snr = fx['SNR'] if 'SNR' in fx else ch['SNR']       # its own Eb/N0, or the channel's
    inp = dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
               SNR=float(snr[0]),
               eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                         y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(FORWARDS)])
    res = rec.run_case(case, inp, device, tail=True, iters=iters)
    bad = []
    for i, (made, got) in enumerate(res):
        want_made = tuple(int(v) for v in fx[f'f{i}_made'])
        assert made == want_made == ((1, 0), (0, 1), (0, 1))[i], (i, made, want_made)
        want = {k: fx[f'f{i}_{k}'] for k in FIELDS}
        print(f'forward {i}: T {int(got["T"][0])} (fixture {int(want["T"][0])})')
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want)]
    assert not bad, '\n'.join(bad)
