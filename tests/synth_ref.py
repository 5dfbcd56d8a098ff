"""numpy restatement of the trial-input synthesis (include/amp_sparc.h, amp_synth_channels /
amp_synth_trials): Philox4x32-10, the Box-Muller normals, the channel taps and their placement,
the message and the noise.  `f32=False` evaluates the real-valued steps in float64 (the
reference the kernels are held to), `f32=True` in float32 arithmetic step by step as the
kernels write them (numpy's libm: its deviation from the float64 form sizes the tests' bar).
"""
from __future__ import annotations

import numpy as np

TAPS, MESSAGE, NOISE = 0, 1, 2
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(c0, c1, c2, c3, k0: int, k1: int):
    """The four output words (uint32 arrays) of counter (c0, c1, c2, c3), key (k0, k1)."""
    c0, c1, c2, c3 = (np.asarray(np.broadcast_arrays(c0, c1, c2, c3)[i]).astype(np.uint64) for i in range(4))
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        hi0, lo0, hi1, lo1 = p0 >> _S32, p0 & _LO, p1 >> _S32, p1 & _LO
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def draw(seed: int, stream: int, ident, index):
    """Words of the block (seed, stream, id, index): key = seed's halves, counter = (index, id low,
    id high, stream).  ident / index broadcast."""
    ident = np.asarray(ident, dtype=np.uint64)
    return philox4x32_10(np.asarray(index, dtype=np.uint64), ident & _LO, ident >> _S32, np.uint64(stream),
                         seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)


def normals(w0, w1, f32: bool = False):
    """(re, im) unit normals of a block's first two words."""
    if f32:
        u1 = ((w0 >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
        u2 = (w1 >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
        r = np.sqrt(np.float32(-2.0) * np.log(u1))
        ang = np.float32(2.0 * np.pi) * u2
        return r * np.cos(ang), r * np.sin(ang)
    u1 = ((w0 >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u2 = (w1 >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)


def mulhi32(w, m: int):
    return ((w.astype(np.uint64) * np.uint64(m)) >> _S32).astype(np.int64)


def taps(seed: int, channel: int, Nr: int, Nt: int, Lh: int, f32: bool = False):
    """Unit-normal taps (re, im) [Nr, Nt, Lh] of one channel: tap (r, t, l) has index (r Nt + t) Lh + l."""
    index = np.arange(Nr * Nt * Lh, dtype=np.uint64).reshape(Nr, Nt, Lh)
    w = draw(seed, TAPS, channel, index)
    return normals(w[0], w[1], f32)


def channel(seed: int, ident: int, sw, Nt: int, Na: int, Nr: int, Lh: int, Lin: int, f32: bool = False):
    """A [Nr Lout, Nt Lin] of channel `ident`: block (o, i), l = o - i in [0, Lh), holds
    f32(sw)[o, i] h[:, :, l] with h = (re + i im) / sqrt(2 Na Lin); zeros elsewhere.  complex128
    (f32: complex64, products rounded as the kernel's s * (z * scale))."""
    sw = np.asarray(sw, dtype=np.float32)
    Lout = sw.shape[0]
    re, im = taps(seed, ident, Nr, Nt, Lh, f32)
    A = np.zeros((Nr * Lout, Nt * Lin), dtype=np.complex64 if f32 else np.complex128)
    if f32:
        scale = np.float32(1.0 / np.sqrt(2.0 * Na * Lin))
        re, im = re * scale, im * scale
    else:
        re, im = re / np.sqrt(2.0 * Na * Lin), im / np.sqrt(2.0 * Na * Lin)
    for l in range(Lh):
        for i in range(Lin):
            o = i + l
            if o >= Lout:
                continue
            s = sw[o, i] if f32 else np.float64(sw[o, i])
            A[o * Nr:(o + 1) * Nr, i * Nt:(i + 1) * Nt] = s * re[:, :, l] + 1j * (s * im[:, :, l])
    return A


def channel_mask(Lout: int, Nt: int, Nr: int, Lh: int, Lin: int):
    """True on the blocks (o, i) with o - i in [0, Lh)."""
    o = np.arange(Nr * Lout)[:, None] // Nr
    i = np.arange(Nt * Lin)[None, :] // Nt
    return (o - i >= 0) & (o - i < Lh)


def sections(seed: int, trial0: int, E: int, L: int, M: int, K: int):
    """(pos, k) int64 [E, L]: section s of trial e takes the block (MESSAGE, trial0 + e, s)."""
    ident = (np.uint64(trial0) + np.arange(E, dtype=np.uint64))[:, None]
    w = draw(seed, MESSAGE, ident, np.arange(L, dtype=np.uint64)[None, :])
    return mulhi32(w[0], M), mulhi32(w[1], K)


def message(seed: int, trial0: int, E: int, L: int, M: int, symbols, gray):
    """(x c64 [E, L M], sym int64 [E, L], idx int64 [E, L]) as data.py:82-90 places them."""
    sym_tab = np.asarray(symbols).astype(np.complex128).astype(np.complex64)
    pos, k = sections(seed, trial0, E, L, M, len(sym_tab))
    idx = np.arange(L, dtype=np.int64)[None, :] * M + pos
    x = np.zeros((E, L * M), dtype=np.complex64)
    np.put_along_axis(x, idx, sym_tab[k], axis=1)
    return x, np.asarray(gray, dtype=np.int64)[k], idx


def unit_noise(seed: int, trial0: int, E: int, n: int, f32: bool = False):
    """Unit normals (re, im) [E, n]: row j of trial e takes the block (NOISE, trial0 + e, j)."""
    ident = (np.uint64(trial0) + np.arange(E, dtype=np.uint64))[:, None]
    w = draw(seed, NOISE, ident, np.arange(n, dtype=np.uint64)[None, :])
    return normals(w[0], w[1], f32)


def noise_std(Na: int, Nr: int, SNR: float) -> float:
    return float(np.sqrt(Na / Nr / SNR / 2))          # channel.py:153
