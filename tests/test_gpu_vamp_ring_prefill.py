"""GPU: the bf16x3 VAMP engine with its GEMMs' operator rings filled one phase ahead computes the
bits it computed before (amp_persist.h x3_ring_fill / gemm_x3_ring).

Only the time at which operator loads are issued changed, so a building forward and the reuse
forward after it (new y, same channel objects: the q0_load branch with its own V fill) must equal,
bit for bit, what the commit before the change computed on an MI355X: r, xmmse and var bits, T and
all 13 counters, against tests/golden/ring_prefill_bits.part*.npz (tools/record_forward_bits.py,
recorded on that commit; the inputs are stored with the results).

Shapes: Nt=64 Na=4 Nr=128 B=40, 16-QAM and QPSK (G3 = 2: prefill, steady state and the
next-operator refill meet in two groups; the last workgroup has 8 valid rows); Nt=128 Na=4 Nr=256
B=16 (G3 = 4); Nt=256 Na=8 Nr=512 B=32 (two workgroups of the eight-wave cfg4 instantiation).
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

_FIX = {}


def _fixture():
    """{case: {field: array}} of the parts, row blocks ('field@i') joined again (read once)."""
    if not _FIX:
        raw, k = {}, 0
        while os.path.exists(os.path.join(GOLDEN, f'{rec.STEM}.part{k}.npz')):
            z = np.load(os.path.join(GOLDEN, f'{rec.STEM}.part{k}.npz'))
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


@pytest.mark.parametrize('case', rec.CASES, ids=[rec.case_name(*c) for c in rec.CASES])
def test_forward_bits_equal_the_parent_commits(device, case):
    fx = _fixture()[rec.case_name(*case)]
    inp = dict(U=torch.from_numpy(fx['U']), s=torch.from_numpy(fx['s']), Vh=torch.from_numpy(fx['Vh']),
               SNR=float(fx['SNR'][0]),
               eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                         y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(2)])
    res = rec.run_case(case, inp, device)
    bad = []
    for i, (made, got) in enumerate(res):
        want_made = tuple(int(v) for v in fx[f'f{i}_made'])
        assert made == want_made == ((1, 0), (0, 1))[i], (i, made, want_made)
        want = {k: fx[f'f{i}_{k}'] for k in ('r', 'xmmse', 'var', 'T', 'counts')}
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want)]
    assert not bad, '\n'.join(bad)
