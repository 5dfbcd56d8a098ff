"""numpy restatement of the reduction chain of the persistent VAMP engine's per-iteration exchange
(csrc/amp_common.h part_wave_reduce / part_wave_reduce_keys, csrc/amp_persist.h part_publish /
part_publish_keys and part_gather / part_gather_keys, csrc/amp_vamp.h var_mean_div / var_mean_pow2),
and the inputs the CPU and GPU tests share.

A record is (sumvar float64, maxabs float64, minsecmax float64, notclose uint32); maxabs and
minsecmax are float32 values widened, or NaN.  The butterfly runs the group sizes 2, 4, ... 64 with
op(self, partner) in every lane; lane 0, whose result is the one consumed, is in the even half at
every level, so its value is op(even half, odd half) all the way up.  The lanes of a half hold one
value only up to the sign of a zero (nan_max(+0, -0) is its second operand), so the partner maps
are the hardware's own (the mirrors of the 8- and 16-lane levels included).
"""
import numpy as np

WAVE, NW, WG, MAXG = 64, 8, 512, 256
FKEY_PINF, FKEY_NINF = np.int32(0x7f800000), np.int32(0x807fffff - (1 << 32))
OUT_BYTES = 17056
O_PUB, O_WAVES, O_GATHER, O_FLAGS, O_MEAN = 0, 64, 576, 640, 672

REC = np.dtype([('sumvar', '<f8'), ('maxabs', '<f8'), ('minsecmax', '<f8'), ('notclose', '<u4'), ('pad', '<u4')])


def bits(a):
    shape = np.shape(a)
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).reshape(shape)


def nan_max(a, b):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a > b, a, b))


def nan_min(a, b):
    with np.errstate(invalid='ignore'):
        return np.where(np.isnan(a) | np.isnan(b), a + b, np.where(a < b, a, b))


_LANES = np.arange(WAVE)
# the partner of every lane per level (amp_common.h xl_i32): quad_perm [1,0,3,2] and [2,3,0,1],
# row_half_mirror (i <-> 7 - i within 8 lanes), row_mirror (i <-> 15 - i within 16), then the
# permlane16 / permlane32 swaps (lane ^ 16, lane ^ 32)
PARTNERS = (_LANES ^ 1, _LANES ^ 2, (_LANES & ~7) | (7 - (_LANES & 7)), (_LANES & ~15) | (15 - (_LANES & 15)),
            _LANES ^ 16, _LANES ^ 32)


def butterfly(v, op):
    """[..., 64] -> [...]: lane 0 of the six-level butterfly op(self, partner)."""
    v = np.array(v)
    for partner in PARTNERS:
        v = op(v, v[..., partner])
    return v[..., 0]


def pair_tree(v, op):
    """[..., 64] -> [...]: adjacent blocks paired level by level, op(even block, odd block).  What lane 0
    of the butterfly holds for a commutative op whose result has one bit pattern (an addition of
    non-NaN values): every lane of a block then holds the block's value, whichever partner map pairs
    the blocks."""
    v = np.array(v)
    while v.shape[-1] > 1:
        v = op(v[..., 0::2], v[..., 1::2])
    return v[..., 0]


def add(a, b):
    with np.errstate(over='ignore', invalid='ignore'):
        return a + b


def fkey(f):
    b = np.ascontiguousarray(f, dtype=np.float32).view(np.int32).reshape(np.shape(f))
    return b ^ ((b >> 31) & np.int32(0x7fffffff))


def funkey(k):
    k = np.asarray(k, dtype=np.int32)
    return np.ascontiguousarray(k ^ ((k >> 31) & np.int32(0x7fffffff))).view(np.float32).reshape(k.shape)


def key_is_nan(k):
    return (k > FKEY_PINF) | (k < FKEY_NINF)


# ---- wave tree -----------------------------------------------------------------------------------
def wave_tree_old(r):
    """r: REC [..., 64] -> REC [...] (lane 0's result)."""
    o = np.zeros(r.shape[:-1], dtype=REC)
    o['sumvar'] = butterfly(r['sumvar'], add)
    o['maxabs'] = butterfly(r['maxabs'], nan_max)
    o['minsecmax'] = butterfly(r['minsecmax'], nan_min)
    o['notclose'] = butterfly(r['notclose'], add)
    return o


def wave_gate(r):
    """True where a wave holds a NaN in either extreme of any lane."""
    return (np.isnan(r['maxabs']) | np.isnan(r['minsecmax'])).any(axis=-1)


def wave_tree_new(r):
    """-> (REC [...], keys int32 [..., 2], gate bool [...])."""
    old = wave_tree_old(r)
    gate = wave_gate(r)
    o = np.zeros(r.shape[:-1], dtype=REC)
    o['sumvar'] = pair_tree(r['sumvar'], add)       # group_sum in both forms, restated as the plain tree
    o['notclose'] = pair_tree(r['notclose'], add)
    with np.errstate(invalid='ignore'):
        kx = fkey(r['maxabs'].astype(np.float32)).max(axis=-1)
        kn = fkey(r['minsecmax'].astype(np.float32)).min(axis=-1)
        okx = fkey(old['maxabs'].astype(np.float32))
        okn = fkey(old['minsecmax'].astype(np.float32))
    o['maxabs'] = np.where(gate, old['maxabs'], funkey(kx).astype(np.float64))
    o['minsecmax'] = np.where(gate, old['minsecmax'], funkey(kn).astype(np.float64))
    keys = np.stack([np.where(gate, okx, kx), np.where(gate, okn, kn)], axis=-1).astype(np.int32)
    return o, keys, gate


# ---- thread 0's fold over the eight waves and the two granules -----------------------------------
def _granules(sv, fx, fn, nc):
    g = np.zeros(8, dtype=np.uint32)
    b = int(bits(np.float64(sv)))
    g[0], g[1], g[2] = b & 0xffffffff, b >> 32, nc
    g[4], g[5] = bits(np.float32(fx)), bits(np.float32(fn))
    return g


def _fold_sums(w):
    sv, nc = w['sumvar'][0], w['notclose'][0]
    for i in range(1, len(w)):
        sv, nc = add(sv, w['sumvar'][i]), add(nc, w['notclose'][i])
    return sv, nc


def _fold_extremes_old(w):
    mx, mn = w['maxabs'][0], w['minsecmax'][0]
    for i in range(1, len(w)):
        mx, mn = nan_max(mx, w['maxabs'][i]), nan_min(mn, w['minsecmax'][i])
    with np.errstate(invalid='ignore'):
        return np.float32(mx), np.float32(mn)


def publish_old(r):
    """r: REC [8, 64] -> (granule words uint32 [8], the waves' REC [8])."""
    w = wave_tree_old(r)
    sv, nc = _fold_sums(w)
    fx, fn = _fold_extremes_old(w)
    return _granules(sv, fx, fn, nc), w


def publish_new(r):
    """-> (granule words, the waves' REC [8], wave gates [8], whether the fold took the old loop)."""
    w, keys, gate = wave_tree_new(r)
    with np.errstate(over='ignore', invalid='ignore'):   # s[0] + s[1] + ... + s[7], restated as running sums
        sv, nc = np.cumsum(w['sumvar'])[-1], np.cumsum(w['notclose'], dtype=np.uint32)[-1]
    fold_gate = bool(key_is_nan(keys).any())
    if fold_gate:
        fx, fn = _fold_extremes_old(w)
    else:
        fx, fn = funkey(keys[:, 0].max()), funkey(keys[:, 1].min())
    return _granules(sv, fx, fn, nc), w, gate, fold_gate


# ---- gather: the lane fold over lane + 64 q, then the tree ---------------------------------------
def _lane_records(gran):
    """gran uint32 [n, 8] -> (sumvar f64 [4, 64], maxabs f32, minsecmax f32, notclose u32, valid)."""
    n = len(gran)
    g = np.zeros((4 * WAVE, 8), dtype=np.uint32)
    g[:n] = gran
    valid = (np.arange(4 * WAVE) < n).reshape(4, WAVE)
    sv = (g[:, 0].astype(np.uint64) | (g[:, 1].astype(np.uint64) << np.uint64(32))).view(np.float64).reshape(4, WAVE)
    return sv, g[:, 4].copy().view(np.float32).reshape(4, WAVE), g[:, 5].copy().view(np.float32).reshape(4, WAVE), \
        g[:, 2].reshape(4, WAVE), valid


def _lane_sums(sv, nc, valid):
    s, c = np.zeros(WAVE), np.zeros(WAVE, dtype=np.uint32)
    for q in range(4):
        s = np.where(valid[q], add(s, sv[q]), s)
        c = np.where(valid[q], add(c, nc[q]), c)
    return s, c


def gather_old(gran):
    sv, fx, fn, nc, valid = _lane_records(gran)
    r = np.zeros(WAVE, dtype=REC)
    r['sumvar'], r['notclose'] = _lane_sums(sv, nc, valid)
    mx, mn = np.zeros(WAVE), np.full(WAVE, np.inf)
    for q in range(4):
        with np.errstate(invalid='ignore'):
            wx, wn = fx[q].astype(np.float64), fn[q].astype(np.float64)
        mx = np.where(valid[q], nan_max(mx, wx), mx)
        mn = np.where(valid[q], nan_min(mn, wn), mn)
    r['maxabs'], r['minsecmax'] = mx, mn
    return wave_tree_old(r)


def gather_gate(gran):
    _, fx, fn, _, valid = _lane_records(gran)
    return bool(((np.isnan(fx) | np.isnan(fn)) & valid).any())


def gather_new(gran):
    """-> (REC scalar, whether the sweep took the old fold)."""
    if gather_gate(gran):
        return gather_old(gran), True
    sv, fx, fn, nc, valid = _lane_records(gran)
    o = np.zeros((), dtype=REC)
    # 0.0 + g0 + g1 + g2 + g3 with +0.0 for a missing granule (the running sum starts at +0.0 and so is
    # never -0.0: adding +0.0 leaves its bits), then the plain tree
    s, c = np.zeros(WAVE), np.zeros(WAVE, dtype=np.uint32)
    for q in range(4):
        s, c = add(s, np.where(valid[q], sv[q], 0.0)), add(c, np.where(valid[q], nc[q], np.uint32(0)))
    o['sumvar'], o['notclose'] = pair_tree(s, add), pair_tree(c, add)
    kx = np.where(valid, fkey(fx), np.int32(0)).max()                 # fkey(0.0f): PartAcc's initial maxabs
    kn = np.where(valid, fkey(fn), FKEY_PINF).min()                  # fkey(inf): its initial minsecmax
    o['maxabs'], o['minsecmax'] = np.float64(funkey(max(kx, np.int32(0)))), np.float64(funkey(min(kn, FKEY_PINF)))
    return o, False


# ---- the mean's quotient -------------------------------------------------------------------------
def mean_pow2(bmean, n):
    """(whether the integer product is a power of two 2^k, k)."""
    bn = int(bmean) * int(n)
    return bn > 0 and bn & (bn - 1) == 0, max(bn, 1).bit_length() - 1


def var_mean_div(s, bmean, n):
    with np.errstate(all='ignore'):
        return np.float64(s) / (np.float64(bmean) * np.float64(n))


def var_mean_pow2(s, bmean, n):
    p2, k = mean_pow2(bmean, n)
    with np.errstate(all='ignore'):
        return np.ldexp(np.float64(s), -k) if p2 else var_mean_div(s, bmean, n)


# ---- comparisons ---------------------------------------------------------------------------------
def same_extreme(a, b):
    """Bit-equal, or zeros of either sign on both sides (the documented difference)."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((bits(a) == bits(b)) | ((a == 0) & (b == 0))))


def same_or_both_nan(a, b):
    """Bit-equal, or NaN on both sides (an addition of two NaNs may keep either payload)."""
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


# ---- inputs --------------------------------------------------------------------------------------
NANS32 = (0x7fc00000, 0xffc00000, 0x7fc12345, 0xffe00001, 0x7f800001, 0xff923456)


def _f32(u):
    return np.array([u], dtype=np.uint32).view(np.float32)[0]


def wave_cases():
    """{name: REC [8, 64]}: one workgroup's per-thread records."""
    rng = np.random.default_rng(20251)
    cases = {}

    def base(lo=-15, hi=15):
        r = np.zeros((NW, WAVE), dtype=REC)
        r['sumvar'] = rng.standard_normal((NW, WAVE)) * np.exp2(rng.integers(-20, 20, (NW, WAVE)))
        r['maxabs'] = (rng.random((NW, WAVE)).astype(np.float32) * np.exp2(rng.integers(lo, hi, (NW, WAVE))).astype(np.float32))
        r['minsecmax'] = (rng.standard_normal((NW, WAVE)).astype(np.float32)
                          * np.exp2(rng.integers(lo, hi, (NW, WAVE))).astype(np.float32))
        r['notclose'] = rng.integers(0, 1 << 20, (NW, WAVE))
        return r

    cases['binades'] = base()
    r = base()
    r['maxabs'][1, 7] = np.inf
    r['minsecmax'][2, 9] = -np.inf
    r['minsecmax'][3] = np.inf
    r['sumvar'][4, 4] = np.inf
    cases['inf'] = r
    r = base(-149, -126)
    cases['denormals'] = r
    r = base()
    r['maxabs'][:] = np.float32(3.5)
    r['minsecmax'][:] = np.float32(-1.25)
    r['notclose'][:] = 0xffffffff
    cases['equal'] = r
    r = np.zeros((NW, WAVE), dtype=REC)
    r['minsecmax'] = np.where(rng.random((NW, WAVE)) < 0.5, 0.0, -0.0)
    r['maxabs'] = np.where(rng.random((NW, WAVE)) < 0.5, 0.0, -0.0)
    r['minsecmax'][5] = 0.0
    r['maxabs'][6] = -0.0
    cases['zeros'] = r
    r = base()
    r['minsecmax'] = np.abs(r['minsecmax'])
    r['minsecmax'][0, 3], r['minsecmax'][0, 40] = -0.0, 0.0
    r['maxabs'][:] = 0.0
    r['maxabs'][2, 1] = -0.0
    cases['zero_extremes'] = r
    for i, u in enumerate(NANS32):
        r = base()
        r['maxabs' if i % 2 == 0 else 'minsecmax'][i % NW, (11 * i + 5) % WAVE] = np.float64(_f32(u))
        cases[f'nan_lane_{u:08x}'] = r
    r = base()
    r['maxabs'][3] = np.array([0x7ff8000000000000], dtype=np.uint64).view(np.float64)[0]   # DenStat's float64 NaN
    cases['nan_wave_f64'] = r
    r = base()
    r['maxabs'][1, 2] = np.float64(_f32(0x7fc00001))
    r['maxabs'][1, 3] = np.float64(_f32(0xffc00002))
    r['minsecmax'][6, 60] = np.float64(_f32(0xffc00003))
    cases['nan_several'] = r
    return cases


def gran_cases():
    """{name: uint32 [n, 8]}: granule pairs as published (tag words 0)."""
    rng = np.random.default_rng(20252)
    cases = {}

    def base(n):
        g = np.zeros((n, 8), dtype=np.uint32)
        sv = (rng.random(n) * np.exp2(rng.integers(-10, 20, n))).view(np.uint64)
        g[:, 0], g[:, 1] = sv & np.uint64(0xffffffff), sv >> np.uint64(32)
        g[:, 2] = rng.integers(0, 1 << 24, n)
        g[:, 4] = (rng.random(n).astype(np.float32) * np.exp2(rng.integers(-15, 15, n)).astype(np.float32)).view(np.uint32)
        g[:, 5] = (rng.standard_normal(n).astype(np.float32) * np.exp2(rng.integers(-15, 15, n)).astype(np.float32)).view(np.uint32)
        return g

    for n in (1, 2, 63, 64, 65, 200, 256):
        cases[f'n{n}'] = base(n)
    g = base(256)
    g[17, 4], g[99, 5], g[255, 5] = bits(np.float32(np.inf)), bits(np.float32(-np.inf)), bits(np.float32(np.inf))
    cases['inf'] = g
    g = base(130)
    g[:, 4] = (rng.random(130).astype(np.float32) * np.float32(2.0 ** -140)).view(np.uint32)
    g[:, 5] = (rng.standard_normal(130).astype(np.float32) * np.float32(2.0 ** -140)).view(np.uint32)
    cases['denormals'] = g
    g = base(256)
    g[:, 4], g[:, 5] = bits(np.float32(7.0)), bits(np.float32(-2.0))
    cases['equal'] = g
    g = base(100)
    g[:, 4] = np.where(rng.random(100) < 0.5, 0, 0x80000000)
    g[:, 5] = np.where(rng.random(100) < 0.5, 0, 0x80000000)
    cases['zeros'] = g
    for i, u in enumerate(NANS32):
        g = base(256 if i % 2 else 70)
        g[(37 * i + 3) % len(g), 4 + i % 2] = u
        cases[f'nan_{u:08x}'] = g
    return cases


def mean_cases():
    """(sums float64 [512], divs int32 [512, 2]): k = 0 ... 40 and other products per thread."""
    rng = np.random.default_rng(20253)
    sums = rng.standard_normal(WG) * np.exp2(rng.integers(-30, 30, WG))
    sums[:8] = [0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308]
    sums[8:16] = np.array([0x7ff8000000012345, 0xfff8000000000001, 0x7ff0000000000001, 0x000fffffffffffff,
                           0x0010000000000001, 0x8000000000000003, 0x0000000000000001, 0x001fffffffffffff],
                          dtype=np.uint64).view(np.float64)
    sums[16:64] = rng.standard_normal(48) * np.exp2(rng.integers(-1074, -1000, 48).astype(np.float64))   # subnormal quotients
    divs = np.zeros((WG, 2), dtype=np.int32)
    for i in range(WG):
        k = i % 41
        a = rng.integers(max(0, k - 30), min(k, 30) + 1)
        divs[i] = (1 << a, 1 << (k - a))
    divs[400:] = rng.integers(1, 5000, (WG - 400, 2))
    divs[400:405] = [(4096, 256), (32, 256), (17, 256), (1, 1), (1 << 20, 1 << 14)]
    return sums, divs
