"""CPU: the position-pair denoiser step (amp_denoise.h denoise_step_grid2_pair, M = 32) forms its
section reductions and its float64 var sums in the order of the step it replaces.

numpy restatements of the two lane maps of one wave (64 lanes, four sections of 32 positions a step):

  old   lane l = gid * 32 + g holds position g of sections base + gid (u = 0) and base + 2 + gid
        (u = 1); group_fmax_c<32> / group_sum_excl_c<32> run per u over xor 1, 2, 4, 8, 16; the lane
        adds var[u = 0], then var[u = 1] into its float64 sum; part_wave_reduce folds the wave over
        xor 1, 2, 4, 8, 16, 32 and the waves are added in order;
  pair  lane n holds positions 2j, 2j + 1 (j = n & 15) of section base + (n >> 4): the first
        butterfly step in the lane, then distances 1, 2, 4, 8 over j; one v_permlane32_swap of
        (var.x, var.y) gives lanes < 32 the even positions' chain and lanes >= 32 the odd positions',
        and pair_acc_out moves the sums back to the old lanes before the same fold.

Asserted bit for bit (a NaN compares equal to a NaN: which of two NaN operands an addition returns
is not what the order is about): Z and every position's exclusive sum (float32), smax / sabs, the
waves' and the workgroup's sumvar (float64), for one wave step and for a whole iteration of one
workgroup (128 sections, eight waves, four rounds).  Inputs that make the order visible: values over
30 binades, exact zeros, one +inf, a NaN in an even and in an odd position.  Mutation: the pair map
with its distances in another order differs on the wide-range input.
"""
import numpy as np
import pytest

G, POS = 32, 32
LANES = np.arange(64)


# ---- the primitives both maps share (amp_common.h) ----
def fkey(f):
    b = np.asarray(f, np.float32).view(np.int32)
    return b ^ ((b >> 31) & 0x7fffffff)


def funkey(k):
    k = np.asarray(k, np.int32)
    return (k ^ ((k >> 31) & 0x7fffffff)).view(np.float32)


def xl(v, o):
    """Every lane's partner value at xor distance o."""
    return v[LANES ^ o]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


# ---- old map: one position of two sections per lane ----
def old_step(zt, lmx, lab, var, acc):
    """zt, lmx, lab, var: [4 sections, 32 positions] float32; acc: [64] float64 per-lane sums.
    Returns Z [4], excl [4, 32], smax [4], sabs [4] and the updated acc."""
    gid, g = LANES // G, LANES % G
    Z, excl = np.empty(4, np.float32), np.empty((4, POS), np.float32)
    smax, sabs = np.empty(4, np.float32), np.empty(4, np.float32)
    acc = acc.copy()
    with np.errstate(all='ignore'):
        for u in range(2):
            sec = 2 * u + gid                                    # base + u * gpw + gid
            for src, dst in ((lmx, smax), (lab, sabs)):
                k = fkey(src[sec, g])
                for o in (1, 2, 4, 8, 16):
                    k = np.maximum(k, xl(k, o))
                dst[sec] = funkey(k)
            tot = zt[sec, g].astype(np.float32)
            ex = np.zeros(64, np.float32)
            for o in (1, 2, 4, 8, 16):                           # group_sum_excl_c<32>
                p = xl(tot, o)
                ex = ex + p
                tot = tot + p
            Z[sec] = tot
            excl[sec, g] = ex
            acc = acc + var[sec, g].astype(np.float64)           # u = 0, then u = 1
    return Z, excl, smax, sabs, acc


def wave_fold(acc):
    """part_wave_reduce's float64 butterfly; every lane ends with the same bits."""
    v = acc.copy()
    with np.errstate(all='ignore'):
        for o in (1, 2, 4, 8, 16, 32):
            v = v + xl(v, o)
    assert same_bits(v, np.full(64, v[0]))
    return v[0]


# ---- pair map: two positions of one section per lane ----
def pair_acc_in(acc_old):
    n = LANES
    return acc_old[((n >> 4) & 1) * 32 + 2 * (n & 15) + (n >> 5)]


def pair_acc_out(acc_pair):
    l = LANES
    return acc_pair[(l & 1) * 32 + (l >> 5) * 16 + ((l & 31) >> 1)]


def pair_step(zt, lmx, lab, var, acc, dist=(1, 2, 4, 8)):
    """The same step in the pair map; acc: [64] float64 per pair lane."""
    sec, j = LANES >> 4, LANES & 15
    smax, sabs = np.empty(4, np.float32), np.empty(4, np.float32)
    with np.errstate(all='ignore'):
        for src, dst in ((lmx, smax), (lab, sabs)):
            k = np.maximum(fkey(src[sec, 2 * j]), fkey(src[sec, 2 * j + 1]))   # in the lane: an integer max
            for o in dist:
                k = np.maximum(k, xl(k, o))
            dst[sec] = funkey(k)
        a, b = zt[sec, 2 * j].astype(np.float32), zt[sec, 2 * j + 1].astype(np.float32)
        ex_a, ex_b = np.float32(0) + b, np.float32(0) + a
        tot = a + b
        for o in dist:
            p = xl(tot, o)
            ex_a, ex_b = ex_a + p, ex_b + p
            tot = tot + p
        Z = np.empty(4, np.float32)
        Z[sec] = tot
        excl = np.empty((4, POS), np.float32)
        excl[sec, 2 * j], excl[sec, 2 * j + 1] = ex_a, ex_b
        # v_permlane32_swap(var.x, var.y): lanes < 32 get (x of lane n, x of lane n + 32), lanes >= 32
        # (y of lane n - 32, y of lane n)
        vx, vy = var[sec, 2 * j], var[sec, 2 * j + 1]
        lo = LANES < 32
        first = np.where(lo, vx, vy[LANES - 32 * ~lo])
        second = np.where(lo, vx[(LANES + 32) % 64], vy)
        acc = acc + first.astype(np.float64)
        acc = acc + second.astype(np.float64)
    return Z, excl, smax, sabs, acc


# ---- inputs ----
def wide(rng, shape):
    """Positive float32 over 30 binades."""
    return (np.exp2(rng.uniform(-15, 15, shape)) * rng.uniform(1, 2, shape)).astype(np.float32)


def make_inputs(kind, nsec, seed=7):
    rng = np.random.default_rng(seed)
    zt, var = wide(rng, (nsec, POS)), wide(rng, (nsec, POS))
    lmx = (rng.standard_normal((nsec, POS)) * np.exp2(rng.uniform(-10, 10, (nsec, POS)))).astype(np.float32)
    lab = np.maximum(lmx, (np.abs(lmx) * rng.uniform(0.5, 2, (nsec, POS))).astype(np.float32))
    if kind == 'zeros':
        m = rng.random((nsec, POS)) < 0.4
        zt[m], var[m] = 0, 0
        lmx[rng.random((nsec, POS)) < 0.2] = -0.0
    elif kind == 'inf':
        zt[1, 6] = var[2, 9] = lmx[0, 3] = lab[3, 30] = np.inf
    elif kind in ('nan_even', 'nan_odd'):
        p = 12 if kind == 'nan_even' else 13
        for a in (zt, var, lmx, lab):
            a[1, p] = np.nan
            a[nsec - 1, p + 4] = np.nan
    else:
        assert kind == 'wide'
    return zt, lmx, lab, var


KINDS = ['wide', 'zeros', 'inf', 'nan_even', 'nan_odd']


@pytest.mark.parametrize('kind', KINDS)
def test_one_wave_step(kind):
    zt, lmx, lab, var = make_inputs(kind, 4)
    acc0 = wide(np.random.default_rng(3), 64).astype(np.float64)     # sums of earlier steps
    Zo, eo, so, ao, acc_o = old_step(zt, lmx, lab, var, acc0)
    Zp, ep, sp, ap, acc_p = pair_step(zt, lmx, lab, var, pair_acc_in(acc0))
    assert same_bits(Zo, Zp)
    assert same_bits(eo, ep)
    assert same_bits(so, sp) and same_bits(ao, ap)
    assert same_bits(acc_o, pair_acc_out(acc_p))                       # every lane's chain
    assert same_bits(np.array([wave_fold(acc_o)]), np.array([wave_fold(pair_acc_out(acc_p))]))
    if kind.startswith('nan'):
        assert np.isnan(Zo[1]) and np.isnan(so[1]) and np.isnan(ao[1]) and not np.isnan(Zo[0])


def test_the_lane_moves_are_inverse_permutations():
    v = np.arange(64, dtype=np.float64)
    assert np.array_equal(pair_acc_out(pair_acc_in(v)), v) and np.array_equal(pair_acc_in(pair_acc_out(v)), v)
    assert sorted(pair_acc_in(v)) == list(v)


def workgroup(step, to_map, from_map, zt, lmx, lab, var, nsec):
    """One iteration of an eight-wave workgroup: wave w runs sections 4 w + 32 r .. + 3 in round r."""
    out = dict(Z=np.zeros(128, np.float32), excl=np.zeros((128, POS), np.float32), smax=np.zeros(128, np.float32),
               sabs=np.zeros(128, np.float32), wave=np.zeros(8))
    for w in range(8):
        acc = to_map(np.zeros(64))
        for base in range(4 * w, nsec, 32):
            s = slice(base, base + 4)
            Z, ex, sm, sa, acc = step(zt[s], lmx[s], lab[s], var[s], acc)
            out['Z'][s], out['excl'][s], out['smax'][s], out['sabs'][s] = Z, ex, sm, sa
        out['wave'][w] = wave_fold(from_map(acc))
    tot = out['wave'][0]
    with np.errstate(all='ignore'):
        for w in range(1, 8):                                            # part_publish: the waves in order
            tot = tot + out['wave'][w]
    out['wg'] = np.array([tot])
    return out


@pytest.mark.parametrize('nsec', [128, 104, 8])      # 16, 13 and 1 valid rows of eight sections
@pytest.mark.parametrize('kind', KINDS)
def test_one_workgroup_iteration(kind, nsec):
    zt, lmx, lab, var = make_inputs(kind, 128)
    ident = lambda a: a   # noqa: E731
    o = workgroup(old_step, ident, ident, zt, lmx, lab, var, nsec)
    p = workgroup(pair_step, pair_acc_in, pair_acc_out, zt, lmx, lab, var, nsec)
    for name in ('Z', 'excl', 'smax', 'sabs', 'wave', 'wg'):
        assert same_bits(o[name], p[name]), name


def test_another_distance_order_is_seen():
    zt, lmx, lab, var = make_inputs('wide', 128)
    differs = 0
    for base in range(0, 128, 4):
        s = slice(base, base + 4)
        Zo, eo, *_ = old_step(zt[s], lmx[s], lab[s], var[s], np.zeros(64))
        Zm, em, *_ = pair_step(zt[s], lmx[s], lab[s], var[s], np.zeros(64), dist=(8, 4, 2, 1))
        differs += not (same_bits(Zo, Zm) and same_bits(eo, em))
    assert differs >= 30, differs          # of 32 wave steps
    # and so is the order of the two additions per step in the float64 chain
    acc_o = np.zeros(64)
    acc_s = np.zeros(64)
    for base in range(0, 128, 4):
        s = slice(base, base + 4)
        *_, acc_o = old_step(zt[s], lmx[s], lab[s], var[s], acc_o)
        *_, acc_s = pair_step(zt[s], lmx[s], lab[s], var[s][[2, 3, 0, 1]], acc_s)   # u = 1 before u = 0
    assert not same_bits(acc_o, pair_acc_out(acc_s))
