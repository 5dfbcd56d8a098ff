"""GPU: the gather of the eight-wave bf16x3 VAMP kernel's exchange with the kernel's retry loop
(amp_persist.h part_gather_keys as vamp_persist calls it), through amp_exchange_poll_debug: one
launch of one workgroup of eight waves per case, on granule pairs whose tags the test sets.

  every tag present, ngran = 1, 63, 64, 65, 255, 256 (a lane's second, third and fourth granule slot,
      full and partial): the gather is ok after one sweep and its record is the numpy restatement's
      (tests/exchange_reduce_ref.py gather_new, as tests/test_exchange_reduce_cpu.py checks it);
  the abort word already raised and one tag absent: the gather gives up after its first sweep, far
      below its 2 s bound, and leaves the word raised; raised with every tag present: ok.
No case waits for a tag that never comes: the entry point looks at the tags first and does not run a
gather that would wait (code 2), which the last test checks.
"""
import ctypes as C

import numpy as np
import pytest

import exchange_reduce_ref as ref

pytestmark = pytest.mark.gpu

NGRAN = (1, 63, 64, 65, 255, 256)
TAG = 0x01230457
OUT = np.dtype([('rec', ref.REC), ('abort', '<u4'), ('sweeps', '<u4'), ('code', '<u4'), ('pad', '<u4'), ('ticks', '<u8'),
                ('pad2', '<u8')])
# one sweep is a handful of memory round trips (a few us); 100 us = 10^4 ticks of 10 ns is 20000 times
# below the gather's own bound of 2 s, and far above anything one sweep can take
ONE_SWEEP_TICKS = 10000


def grans(n, seed):
    """n granule pairs in the ranges of ref.gran_cases(), every tag set."""
    rng = np.random.default_rng(seed)
    g = np.zeros((n, 8), dtype=np.uint32)
    sv = (rng.random(n) * np.exp2(rng.integers(-10, 20, n))).view(np.uint64)
    g[:, 0], g[:, 1] = sv & np.uint64(0xffffffff), sv >> np.uint64(32)
    g[:, 2] = rng.integers(0, 1 << 24, n)
    g[:, 4] = (rng.random(n).astype(np.float32) * np.exp2(rng.integers(-15, 15, n)).astype(np.float32)).view(np.uint32)
    g[:, 5] = (rng.standard_normal(n).astype(np.float32) * np.exp2(rng.integers(-15, 15, n)).astype(np.float32)).view(np.uint32)
    g[:, 3] = g[:, 7] = TAG
    return g


def run(device, g, raised, tag=TAG):
    import torch
    import amp_native as nat
    assert OUT.itemsize == 64
    d = torch.from_numpy(np.ascontiguousarray(g).view(np.uint8).reshape(-1)).to(device)
    out = torch.full((64,), 0xa5, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    nat.check(nat.lib().amp_exchange_poll_debug(C.c_void_p(d.data_ptr()), len(g), tag, raised, C.c_void_p(out.data_ptr()),
                                                C.c_void_p(st)), 'amp_exchange_poll_debug')
    torch.cuda.synchronize()
    return out.cpu().numpy().view(OUT)[0]


@pytest.mark.parametrize('n', NGRAN)
def test_every_tag_present(device, n):
    g = grans(n, 7000 + n)
    o = run(device, g, 0)
    print(f'ngran {n}: sweeps {o["sweeps"]}, {o["ticks"] / 100:.2f} us')
    assert o['code'] == 0 and o['rec']['pad'] == 1 and o['abort'] == 0 and o['sweeps'] == 1
    host, gate = ref.gather_new(g)
    assert not gate
    assert ref.bits(o['rec']['sumvar']) == ref.bits(host['sumvar']) and o['rec']['notclose'] == host['notclose']
    for f in ('maxabs', 'minsecmax'):
        assert ref.bits(o['rec'][f]) == ref.bits(host[f]), (n, f, o['rec'][f], host[f])


@pytest.mark.parametrize('n,absent,word', [(1, 0, 3), (65, 64, 7), (200, 137, 3), (256, 255, 7), (256, 0, 3)])
def test_raised_word_ends_the_gather_with_its_first_sweep(device, n, absent, word):
    g = grans(n, 7100 + n + absent)
    g[absent, word] = TAG - 1                       # the tag of the iteration before
    o = run(device, g, 1)
    print(f'ngran {n}, tag {absent}.{word} absent: sweeps {o["sweeps"]}, {o["ticks"] / 100:.2f} us')
    assert o['code'] == 0 and o['rec']['pad'] == 0 and o['abort'] == 1
    assert o['sweeps'] == 1 and o['ticks'] < ONE_SWEEP_TICKS


def test_raised_word_with_every_tag_present_is_ok(device):
    g = grans(129, 7200)
    o = run(device, g, 1)
    assert o['code'] == 0 and o['rec']['pad'] == 1 and o['abort'] == 1 and o['sweeps'] == 1
    assert ref.bits(o['rec']['sumvar']) == ref.bits(ref.gather_new(g)[0]['sumvar'])


def test_a_gather_that_would_wait_is_not_run(device):
    import torch
    import amp_native as nat
    g = grans(64, 7300)
    g[5, 3] = 0
    o = run(device, g, 0)
    assert o['code'] == 2 and o['sweeps'] == 0
    z = torch.zeros(64 * 32, dtype=torch.uint8, device=device)
    p = C.c_void_p(z.data_ptr())
    for n in (0, 257):
        assert nat.lib().amp_exchange_poll_debug(p, n, TAG, 0, p, None) != 0
    assert nat.lib().amp_exchange_poll_debug(p, 1, 0, 0, p, None) != 0
    assert nat.lib().amp_exchange_poll_debug(None, 1, TAG, 0, p, None) != 0
