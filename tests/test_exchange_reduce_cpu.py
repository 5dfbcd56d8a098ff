"""The key forms of the persistent VAMP engine's exchange reduction against the shared forms, in
numpy (tests/exchange_reduce_ref.py restates both): the eight-wave bf16x3 kernel takes max|xi| and
the minimum section maximum as integer extremes over order-preserving keys wherever no NaN is among
them, and the mean's quotient by a power of two as a scaling.

  the NaN gates fire exactly when a NaN is present (a lane of a wave, a wave of the fold, a granule);
  sumvar and notclose are bit-equal always;
  the extremes are bit-equal whenever the extreme is nonzero and equal as numbers otherwise (the
  key order puts -0 below +0; the float64 forms keep whichever zero the pairing leaves);
  x / 2^k == ldexp(x, -k) bit for bit, k = 0 ... 40, subnormal quotients, inf and NaN included.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import exchange_reduce_ref as ref  # noqa: E402

WAVES = ref.wave_cases()
GRANS = ref.gran_cases()


def test_keys_order_floats_and_mark_nans():
    v = np.array([-np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 2.5, np.inf], dtype=np.float32)
    k = ref.fkey(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert (ref.bits(ref.funkey(k)) == ref.bits(v)).all()
    assert k[0] == ref.FKEY_NINF and k[-1] == ref.FKEY_PINF and not ref.key_is_nan(k).any()
    nans = np.array(ref.NANS32, dtype=np.uint32).view(np.float32)
    assert ref.key_is_nan(ref.fkey(nans)).all()


@pytest.mark.parametrize('name', list(WAVES))
def test_wave_tree_and_wave_fold(name):
    r = WAVES[name]
    has_nan = np.isnan(r['maxabs']) | np.isnan(r['minsecmax'])
    old = ref.wave_tree_old(r)
    new, keys, gate = ref.wave_tree_new(r)
    assert (gate == has_nan.any(axis=1)).all()
    assert name.startswith('nan') == bool(gate.any())
    assert (ref.bits(old['sumvar']) == ref.bits(new['sumvar'])).all() and (old['notclose'] == new['notclose']).all()
    for f in ('maxabs', 'minsecmax'):
        assert ref.same_extreme(old[f], new[f]), (name, f, old[f], new[f])
        nz = old[f] != 0
        assert (ref.bits(old[f])[nz] == ref.bits(new[f])[nz]).all()
    assert (ref.key_is_nan(keys).any(axis=1) == gate).all()          # the fold sees every NaN wave
    g_old, w_old = ref.publish_old(r)
    g_new, w_new, _, fold_gate = ref.publish_new(r)
    assert fold_gate == bool(has_nan.any())
    assert (g_old[[0, 1, 2, 3, 6, 7]] == g_new[[0, 1, 2, 3, 6, 7]]).all()
    assert ref.same_extreme(g_old[4:6].view(np.float32), g_new[4:6].view(np.float32)), (name, g_old, g_new)
    if fold_gate:
        assert (g_old == g_new).all()


def test_zero_extremes_differ_in_sign_only():
    """The documented case is in the inputs: both zeros present and the extreme a zero."""
    r = WAVES['zeros']
    old, (new, _, _) = ref.wave_tree_old(r), ref.wave_tree_new(r)
    assert (old['maxabs'] == 0).all() and (new['maxabs'] == 0).all()
    assert not np.signbit(new['maxabs'][:6]).any() and np.signbit(new['minsecmax'][[0, 1, 2, 3, 4, 6, 7]]).all()


@pytest.mark.parametrize('name', list(GRANS))
def test_gather(name):
    g = GRANS[name]
    old = ref.gather_old(g)
    new, gate = ref.gather_new(g)
    has_nan = bool(np.isnan(g[:, 4:6].copy().view(np.float32)).any())
    assert gate == has_nan == name.startswith('nan')
    assert ref.bits(old['sumvar']) == ref.bits(new['sumvar']) and old['notclose'] == new['notclose']
    for f in ('maxabs', 'minsecmax'):
        assert ref.same_extreme(old[f], new[f]), (name, f, old[f], new[f])
        if gate:
            assert ref.bits(old[f]) == ref.bits(new[f])


def test_power_of_two_products():
    assert ref.mean_pow2(4096, 256) == (True, 20)
    assert ref.mean_pow2(32, 256) == (True, 13)
    assert ref.mean_pow2(17, 256)[0] is False
    assert ref.mean_pow2(1, 1) == (True, 0)
    assert ref.mean_pow2(1 << 20, 1 << 14) == (True, 34)             # above 2^32: the product is formed in 64 bits
    assert ref.mean_pow2(3 << 20, 1 << 14)[0] is False
    assert ref.mean_pow2(0, 256)[0] is False


def test_quotient_by_a_power_of_two_is_a_scaling():
    rng = np.random.default_rng(7)
    x = np.concatenate([rng.standard_normal(4000) * np.exp2(rng.integers(-60, 60, 4000)),
                        rng.standard_normal(2000) * np.exp2(rng.integers(-1074, -1000, 2000).astype(np.float64)),
                        ref.mean_cases()[0]])
    for k in range(41):
        with np.errstate(all='ignore'):
            q, s = x / np.float64(2.0 ** k), np.ldexp(x, -k)
        assert (ref.bits(q) == ref.bits(s)).all(), k
        assert k < 10 or (np.abs(q[np.isfinite(q)]) < 2.2250738585072014e-308).any()   # subnormal quotients among them
    sums, divs = ref.mean_cases()
    for s, (b, n) in zip(sums, divs):
        assert ref.bits(ref.var_mean_div(s, b, n)) == ref.bits(ref.var_mean_pow2(s, b, n)), (s, b, n)
