"""GPU: the bf16x3 VAMP engine at one workgroup per CU, with vamp_advance in two parts (amp_vamp.h
vamp_advance_head in the exchange, vamp_advance_tail inside the next iteration's GEMM1), the four
LMMSE reciprocals formed together and eta taken from the host, computes the bits it computed before.

Every floating-point operation keeps its operands, its type and its order, so a building forward
and the reuse forward after it must equal, bit for bit, what the commit before the change computed
on an MI355X: r, xmmse and var bits, T and all 13 counters, against
tests/golden/scalar_tail_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem scalar_tail_bits --share-channel \\
      --cases "256,8,512,17,16QAM;256,8,512,32,QPSK;128,4,256,24,16QAM" --ebn0 ";<dB>;"

(the two Nt=256, Nr=512 cases on one channel, stored once; the third draws its own).  20 iterations.
  256,8,512,17,16QAM  the flagship's instantiation (eight waves); the second workgroup has one valid row;
  256,8,512,32,QPSK   the KK = 4 instantiation of the same engine, at an Eb/N0 where the recorded
                      forwards stop before the cap: the stop record (nx = cur) and the status'
                      last_scalar with the head and the tail apart (asserted: fixture T < 20);
  128,4,256,24,16QAM  the four-wave build.  k = 128: two of the four terms of the LMMSE sum are
                      invalid in every lane (the +0.0 path of the select); the last workgroup is partial.
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
STEM = 'scalar_tail_bits'
CASES = [(256, 8, 512, 17, '16QAM'), (256, 8, 512, 32, 'QPSK'), (128, 4, 256, 24, '16QAM')]
EARLY = (256, 8, 512, 32, 'QPSK')   # the case whose recorded forwards stop before the cap

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


def _diff(got, want):
    """Every differing array and its first differing index (bitwise), r / xmmse / var first."""
    bad = []
    for name in ('r', 'xmmse', 'var', 'T', 'counts'):
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}')
            continue
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            bad.append(f'{name}: first difference at flat index {i} of {a.size} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r})')
    return bad


def test_the_fixture_has_a_forward_that_stops_before_the_cap():
    fx = _fixture()[rec.case_name(*EARLY)]
    assert int(fx['f0_T'][0]) < 20 and int(fx['f1_T'][0]) < 20, (fx['f0_T'], fx['f1_T'])


@pytest.mark.parametrize('case', CASES, ids=[rec.case_name(*c) for c in CASES])
def test_forward_bits_equal_the_parent_commits(device, case):
    fix = _fixture()
    fx = fix[rec.case_name(*case)]
    ch = fx if 'U' in fx else fix['shared']             # its own channel, or the shared one
    snr = fx['SNR'] if 'SNR' in fx else ch['SNR']       # its own Eb/N0, or the channel's
    inp = dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
               SNR=float(snr[0]),
               eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                         y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(2)])
    res = rec.run_case(case, inp, device)
    bad = []
    for i, (made, got) in enumerate(res):
        want_made = tuple(int(v) for v in fx[f'f{i}_made'])
        assert made == want_made == ((1, 0), (0, 1))[i], (i, made, want_made)
        want = {k: fx[f'f{i}_{k}'] for k in ('r', 'xmmse', 'var', 'T', 'counts')}
        print(f'forward {i}: T {int(got["T"][0])} (fixture {int(want["T"][0])})')
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want)]
    assert not bad, '\n'.join(bad)
