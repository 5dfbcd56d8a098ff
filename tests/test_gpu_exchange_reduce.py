"""GPU: the reduction chain of the persistent VAMP engine's exchange through amp_exchange_reduce_debug
(one launch of one workgroup of eight waves per case), on the inputs of
tests/test_exchange_reduce_cpu.py: the key forms of the eight-wave bf16x3 kernel
(part_publish_keys, part_gather_keys, var_mean_pow2) equal the shared forms (part_publish,
part_gather, the IEEE division) bit for bit, except for the documented sign of a zero extreme, and
both equal the numpy restatement (tests/exchange_reduce_ref.py).  Against numpy a NaN is compared
as a NaN: which operand's payload an addition of two NaNs keeps is not part of the restatement
(between the two device forms NaNs are compared bitwise: a NaN sends the key form through the
shared code).
"""
import ctypes as C

import numpy as np
import pytest

import exchange_reduce_ref as ref

pytestmark = pytest.mark.gpu

WAVES = ref.wave_cases()
GRANS = ref.gran_cases()
_OUT = {}


def run(device, vals, gran, sums, divs):
    import torch
    import amp_native as nat
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(device)  # noqa: E731
    v, g, s, d = t(vals), t(gran), t(sums), t(divs)
    out = torch.full((ref.OUT_BYTES,), 0xa5, dtype=torch.uint8, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    nat.check(nat.lib().amp_exchange_reduce_debug(C.c_void_p(v.data_ptr()), C.c_void_p(g.data_ptr()), len(gran),
                                                  C.c_void_p(s.data_ptr()), C.c_void_p(d.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(st)), 'amp_exchange_reduce_debug')
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    return dict(pub=[o[ref.O_PUB + 32 * f:ref.O_PUB + 32 * f + 32].view(np.uint32) for f in range(2)],
                waves=[o[ref.O_WAVES + 256 * f:ref.O_WAVES + 256 * f + 256].view(ref.REC) for f in range(2)],
                gather=[o[ref.O_GATHER + 32 * f:ref.O_GATHER + 32 * f + 32].view(ref.REC)[0] for f in range(2)],
                abort=int(o[ref.O_FLAGS:ref.O_FLAGS + 4].view(np.uint32)[0]),
                mean=[o[ref.O_MEAN + 4096 * f:ref.O_MEAN + 4096 * f + 4096].view(np.float64) for f in range(2)])


def outputs(device):
    """Every wave case beside a granule case (cycled), launched once for all tests."""
    if not _OUT:
        sums, divs = ref.mean_cases()
        wn, gn = list(WAVES), list(GRANS)
        for i in range(max(len(wn), len(gn))):
            w, g = wn[i % len(wn)], gn[i % len(gn)]
            o = run(device, WAVES[w].reshape(-1), GRANS[g], sums, divs)
            _OUT.setdefault(('w', w), o)
            _OUT.setdefault(('g', g), o)
    return _OUT


@pytest.mark.parametrize('name', list(WAVES))
def test_wave_tree_and_wave_fold(device, name):
    o = outputs(device)[('w', name)]
    r = WAVES[name]
    old, new = o['waves']
    assert (old['sumvar'].view(np.uint64) == new['sumvar'].view(np.uint64)).all() and (old['notclose'] == new['notclose']).all()
    nan_wave = ref.wave_gate(r)
    for f in ('maxabs', 'minsecmax'):
        assert ref.same_extreme(old[f], new[f]), (name, f, old[f], new[f])
        assert (ref.bits(old[f])[nan_wave] == ref.bits(new[f])[nan_wave]).all()
    g_old, g_new = o['pub']
    assert (g_old[[0, 1, 2, 3, 6, 7]] == g_new[[0, 1, 2, 3, 6, 7]]).all(), (g_old, g_new)
    assert ref.same_extreme(g_old[4:6].view(np.float32), g_new[4:6].view(np.float32)), (g_old, g_new)
    if nan_wave.any():
        assert (g_old == g_new).all(), (g_old, g_new)
    # both against numpy
    n_old, n_new = ref.wave_tree_old(r), ref.wave_tree_new(r)[0]
    for dev, host in ((old, n_old), (new, n_new)):
        assert ref.same_or_both_nan(dev['sumvar'], host['sumvar']) and (dev['notclose'] == host['notclose']).all()
        for f in ('maxabs', 'minsecmax'):
            assert ref.same_or_both_nan(dev[f], host[f]), (name, f, dev[f], host[f])
    for dev, host in ((g_old, ref.publish_old(r)[0]), (g_new, ref.publish_new(r)[0])):
        assert (dev[[0, 1, 2, 3, 6, 7]] == host[[0, 1, 2, 3, 6, 7]]).all(), (name, dev, host)
        assert ref.same_or_both_nan(dev[4:6].view(np.float32), host[4:6].view(np.float32)), (name, dev, host)


@pytest.mark.parametrize('name', list(GRANS))
def test_gather(device, name):
    o = outputs(device)[('g', name)]
    g = GRANS[name]
    assert o['abort'] == 0
    old, new = o['gather']
    assert old['pad'] == 1 and new['pad'] == 1                       # both sweeps completed
    assert ref.bits(old['sumvar']) == ref.bits(new['sumvar']) and old['notclose'] == new['notclose']
    for f in ('maxabs', 'minsecmax'):
        assert ref.same_extreme(old[f], new[f]), (name, f, old[f], new[f])
        if ref.gather_gate(g):
            assert ref.bits(old[f]) == ref.bits(new[f])
    for dev, host in ((old, ref.gather_old(g)), (new, ref.gather_new(g)[0])):
        assert ref.bits(dev['sumvar']) == ref.bits(host['sumvar']) and dev['notclose'] == host['notclose']
        for f in ('maxabs', 'minsecmax'):
            assert ref.same_or_both_nan(dev[f], host[f]), (name, f, dev[f], host[f])


def test_quotient(device):
    o = next(iter(outputs(device).values()))
    sums, divs = ref.mean_cases()
    old, new = o['mean']
    assert (ref.bits(old) == ref.bits(new)).all(), np.flatnonzero(ref.bits(old) != ref.bits(new))
    host = np.array([ref.var_mean_div(s, b, n) for s, (b, n) in zip(sums, divs)])
    assert ref.same_or_both_nan(old, host)


def test_arguments_are_checked(device):
    import torch
    import amp_native as nat
    z = torch.zeros(ref.OUT_BYTES, dtype=torch.uint8, device=device)
    p = C.c_void_p(z.data_ptr())
    for n in (0, 257):
        assert nat.lib().amp_exchange_reduce_debug(p, p, n, p, p, p, None) != 0
    assert nat.lib().amp_exchange_reduce_debug(None, p, 1, p, p, p, None) != 0
