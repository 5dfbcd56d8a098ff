"""CPU: the LMMSE sum of vamp_advance_tail (amp_vamp.h) has the bits of vamp_lmmse_scalars' sum.

The old form adds a lane's term only where i = lane + 64 j < k:
    ss = 0.0;  for j in 0..3:  if (i < k) ss += (double)(1.0f / (s2[i] + vr))
the new one forms all four float32 quotients and adds them with a select:
    ss += (i < k) ? (double)q[j] : 0.0
An invalid lane adds +0.0 to a sum that starts at +0.0 and only ever receives terms added in
round-to-nearest, so it is never -0.0 and x + 0.0 has x's bits (also for inf and NaN).  Checked here
in numpy (IEEE float32 / float64, the same operations) on random (s^2, vr) draws, then through the
64-lane reduction, whose operands are then the same bits.
"""
import numpy as np
import pytest

DRAWS = 100000   # lanes per k: DRAWS / 64 waves of 64 lanes


def _terms(k, seed):
    """[waves, 64, 4] float32 s^2 as s2_lane holds it (0 where i >= k), [waves] float32 vr, valid mask."""
    rng = np.random.default_rng(seed)
    waves = DRAWS // 64 + 1
    i = np.arange(64)[:, None] + 64 * np.arange(4)[None, :]
    valid = np.broadcast_to(i < k, (waves, 64, 4))
    s = np.exp(rng.uniform(np.log(1e-3), np.log(30.0), size=(waves, 64, 4))).astype(np.float32)
    s2 = np.where(valid, s * s, np.float32(0))
    vr = np.exp(rng.uniform(np.log(1e-12), np.log(1e6), size=waves)).astype(np.float32)
    # edge values of vr: the denormal range, huge, zero (invalid lanes divide by it: inf), inf, NaN
    vr[:8] = np.array([1e-45, 1e-39, 3e38, 0.0, np.inf, np.nan, 1e-30, 1.0], dtype=np.float32)
    return s2.astype(np.float32), vr, valid


def _branchy(s2, vr, valid):
    ss = np.zeros(s2.shape[:2], dtype=np.float64)
    for j in range(4):
        q = (np.float32(1) / (s2[:, :, j] + vr[:, None])).astype(np.float32)
        ss = np.where(valid[:, :, j], ss + q.astype(np.float64), ss)      # not added at all where invalid
    return ss


def _select(s2, vr, valid):
    q = (np.float32(1) / (s2 + vr[:, None, None])).astype(np.float32)      # all four, unconditionally
    ss = np.zeros(s2.shape[:2], dtype=np.float64)
    for j in range(4):
        ss = ss + np.where(valid[:, :, j], q[:, :, j].astype(np.float64), np.float64(0.0))
    return ss


@pytest.mark.parametrize('k', [256, 128, 200, 70, 64, 2])
def test_select_sum_has_the_branchy_sums_bits(k):
    s2, vr, valid = _terms(k, seed=1000 + k)
    assert s2.shape[0] * 64 >= DRAWS
    with np.errstate(all='ignore'):
        a, b = _branchy(s2, vr, valid), _select(s2, vr, valid)
    assert a.dtype == b.dtype == np.float64
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    assert not np.any(np.signbit(b) & (b == 0))          # never -0.0: the argument's premise
    # the wave's sum (a fixed-order tree over the 64 lanes) from identical operands
    ta, tb = a.copy(), b.copy()
    with np.errstate(all='ignore'):
        for sh in (1, 2, 4, 8, 16, 32):
            ta = ta + ta[:, np.arange(64) ^ sh]
            tb = tb + tb[:, np.arange(64) ^ sh]
    assert np.array_equal(ta.view(np.uint64), tb.view(np.uint64))


def test_the_discarded_quotient_of_an_invalid_lane_never_reaches_the_sum():
    """s2_lane holds 0 at an invalid lane: its quotient is 1 / vr (inf at vr = 0, NaN at vr = NaN)."""
    s2, vr, valid = _terms(128, seed=7)
    with np.errstate(all='ignore'):
        q = (np.float32(1) / (s2 + vr[:, None, None])).astype(np.float32)
        b = _select(s2, vr, valid)
        only_valid = q[:, :, :2].astype(np.float64)
        want = (np.zeros(b.shape) + only_valid[:, :, 0]) + only_valid[:, :, 1]
    assert np.isinf(q[3, :, 2:]).all()                   # vr = 0: discarded infs
    assert np.array_equal(b.view(np.uint64), want.view(np.uint64))
