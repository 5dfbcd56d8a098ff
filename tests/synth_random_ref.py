"""numpy restatement of the 'random' message of the trial-input synthesis (include/amp_sparc.h,
amp_synth_args.message = 1; Data.random, data.py:55-72): per channel use an exactly uniform
Na-subset of the Nt antennas by Floyd's sampling on stream 1 and one symbol for all of them.

Channel use u of trial `ident`: for j = 0 .. Na - 1, with J = Nt - Na + j, t = mulhi32(w0 of the block
at index u Na + j, J + 1); antenna t is taken unless already chosen, else antenna J.  The symbol is
k = mulhi32(w1 of the block at index u Na, K).  (Floyd: after step j the chosen set is a uniform
(j + 1)-subset of {0 .. J}; mulhi32 of a uniform word is uniform up to 2^-32 (J + 1).)
"""
from __future__ import annotations

import numpy as np

import synth_ref as sr


def subsets(seed: int, trial0: int, E: int, Lin: int, Nt: int, Na: int, K: int):
    """(ant int64 [E, Lin, Na] ascending per channel use, k int64 [E, Lin])."""
    ident = (np.uint64(trial0) + np.arange(E, dtype=np.uint64))[:, None]
    w = sr.draw(seed, sr.MESSAGE, ident, np.arange(Lin * Na, dtype=np.uint64)[None, :])
    w0 = w[0].reshape(E, Lin, Na)
    k = sr.mulhi32(w[1].reshape(E, Lin, Na)[:, :, 0], K)
    ant = np.empty((E, Lin, Na), dtype=np.int64)
    for j in range(Na):
        J = Nt - Na + j
        t = sr.mulhi32(w0[:, :, j], J + 1)
        taken = (ant[:, :, :j] == t[:, :, None]).any(axis=2)
        ant[:, :, j] = np.where(taken, J, t)
    return np.sort(ant, axis=2), k


def message(seed: int, trial0: int, E: int, Lin: int, Nt: int, Na: int, symbols, gray):
    """(x c64 [E, Lin Nt], sym int64 [E, Lin Na], idx int64 [E, Lin Na]) as data.py:61-65 returns them:
    idx the flat nonzero positions in ascending order, sym the gray label at each."""
    sym_tab = np.asarray(symbols).astype(np.complex128).astype(np.complex64)
    ant, k = subsets(seed, trial0, E, Lin, Nt, Na, len(sym_tab))
    idx = (np.arange(Lin, dtype=np.int64)[None, :, None] * Nt + ant).reshape(E, Lin * Na)
    kk = np.repeat(k, Na, axis=1)
    x = np.zeros((E, Lin * Nt), dtype=np.complex64)
    np.put_along_axis(x, idx, sym_tab[kk], axis=1)
    return x, np.asarray(gray, dtype=np.int64)[kk], idx
