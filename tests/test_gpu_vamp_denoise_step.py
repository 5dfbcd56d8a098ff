"""GPU: the eight-wave bf16x3 VAMP engine with the full-round form of its packed denoiser step
(amp_denoise.h denoise_step_grid2_full) and the narrowed decision scan of its epilogue
(amp_decide.h decide_section NARROW) computes the bits it computed before.

Neither change touches the arithmetic, so a building forward and the reuse forward after it must
equal, bit for bit, what the commit before the change computed on an MI355X: r, xmmse and var
bits, T and all 13 counters, against tests/golden/denoise_step_bits.part*.npz, recorded on that
commit with

  python tools/record_forward_bits.py --stem denoise_step_bits --share-channel \\
      --cases "256,8,512,17,16QAM;256,8,512,24,16QAM;256,8,512,29,16QAM;256,4,512,16,16QAM;256,16,512,16,16QAM"

(one Nt=256, Nr=512 channel, stored once with the inputs of every case).  All cases are 16-QAM, 20
iterations.  A workgroup holds 16 rows and its eight waves take 32 sections per round at Na=8:
  B=17  the second workgroup has one valid row, 8 sections: only the masked step runs there, most
        waves have no section at all (and its epilogue decides 8 sections);
  B=24  8 rows in the second workgroup: two full rounds;
  B=29  13 rows: three full rounds and a partial one, full-round and masked step in one call;
  Na=4  (M=64: one section per lane group of 64, two per wave step) and Na=16 (M=16: four sections
        per 64 lanes) at B=16.
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
STEM = 'denoise_step_bits'
CASES = [(256, 8, 512, 17, '16QAM'), (256, 8, 512, 24, '16QAM'), (256, 8, 512, 29, '16QAM'),
         (256, 4, 512, 16, '16QAM'), (256, 16, 512, 16, '16QAM')]

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


@pytest.mark.parametrize('case', CASES, ids=[rec.case_name(*c) for c in CASES])
def test_forward_bits_equal_the_parent_commits(device, case):
    fix = _fixture()
    ch, fx = fix['shared'], fix[rec.case_name(*case)]
    inp = dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
               SNR=float(ch['SNR'][0]),
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
