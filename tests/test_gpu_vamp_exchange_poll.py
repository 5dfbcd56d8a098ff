"""GPU: the eight-wave bf16x3 VAMP engine over many workgroups, with the sweep and retry loop of its
exchange's gather (amp_persist.h part_gather_keys POLL: a sweep's loads issued together, the abort
word's load and the clock read issued with each sweep), computes the bits it computed before.

Nt = 256, Na = 8, Nr = 512, 16-QAM on the channel tests/golden/exchange_chain_bits.part*.npz stores;
B = 1040, 2064 and 4096: 65, 129 and 256 workgroups, so that a lane of the gather holds two, three
and four granule pairs (B = 4096 takes the power-of-two mean).  Each batch is a tiling of the 40
stored trials (row b is trial b % 40).  An output row depends on its own y and on the batch scalars
alone, so every tile of r, xmmse and var must equal the 40 rows the commit before the change
computed for that batch on an MI355X, bit for bit, in a building forward and in the reuse forward
after it; T, nan_state and the 13 counters of both forwards are compared too.  Fixture:
tests/golden/exchange_poll_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_exchange_poll_bits.py
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_exchange_poll_bits as rp  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
_FIX = {}


def _fixture():
    if not _FIX:
        import torch
        fx = rp.load_parts(GOLDEN, rp.STEM)
        _FIX['fx'] = fx
        _FIX['ch'] = rp.channel(GOLDEN)
        _FIX['ep'] = dict(x=torch.from_numpy(fx['x']), y=torch.from_numpy(fx['y']), sym=fx['sym'], idx=fx['idx'])
    return _FIX


def test_the_fixture_holds_the_cases_it_is_for():
    fx = _fixture()['fx']
    assert fx['y'].shape[0] == rp.ROWS and fx['x'].shape[0] == rp.ROWS and len(fx['idx']) == rp.ROWS * rp.NA
    assert [-(-B // 16) for B in rp.BATCHES] == [65, 129, 256]
    assert [(B * rp.NT) & (B * rp.NT - 1) == 0 for B in rp.BATCHES] == [False, False, True]
    for B in rp.BATCHES:
        for k in rp.FIELDS:
            assert fx[f'B{B}/{k}'].shape[0] == rp.ROWS and np.isfinite(fx[f'B{B}/{k}']).all()
        for i in range(2):
            assert int(fx[f'B{B}/f{i}_T'][0]) == 20 and int(fx[f'B{B}/f{i}_nan_state'][0]) == 0
    # the batch scalars differ between the batches: each one's rows are its own
    assert not np.array_equal(fx['B1040/var'], fx['B4096/var'])


@pytest.mark.parametrize('B', rp.BATCHES)
def test_every_tile_equals_the_parent_commits_rows(device, B):
    f = _fixture()
    fx = f['fx']
    res = rp.run_batch(f['ch'], f['ep'], B, device)
    bad = []
    for i, (made, got) in enumerate(res):
        assert made == ((1, 0), (0, 1))[i], (i, made)
        name = 'building' if i == 0 else 'reuse'
        for k in rp.FIELDS:
            want = np.ascontiguousarray(fx[f'B{B}/{k}'])
            a = np.ascontiguousarray(got[k])
            assert a.shape == (B,) + want.shape[1:] and a.dtype == want.dtype, (k, a.shape, a.dtype)
            ne = (a.view(np.uint8).reshape(B, -1) != want.view(np.uint8).reshape(rp.ROWS, -1)[np.arange(B) % rp.ROWS]).any(axis=1)
            print(f'forward {i} ({name}) {k}: {int(ne.sum())} of {B} rows differ')
            if ne.any():
                bad.append(f'forward {i} ({name}) {k}: {int(ne.sum())} of {B} rows differ, first row {int(np.flatnonzero(ne)[0])}')
        for k in ('T', 'nan_state', 'counts'):
            if not np.array_equal(np.asarray(got[k]), fx[f'B{B}/f{i}_{k}']):
                bad.append(f'forward {i} ({name}) {k}: {np.asarray(got[k]).tolist()} != {fx[f"B{B}/f{i}_{k}"].tolist()}')
    assert not bad, '\n'.join(bad)
