"""The 'random' message of the trial-input synthesis (amp_synth_args.message = 1) on the CPU.

* tests/synth_random_ref.py, the numpy restatement of the draw (Floyd's sampling on stream 1), at a
  fixed seed over 20000 channel uses of (Nt, Na) = (16, 3): every subset has Na distinct positions
  in range, the position counts pass a chi-square test against uniform (below the 99.9 % quantile
  for 15 degrees of freedom, 37.697; the run is deterministic: the statistic is 28.95 here; seeds 1 .. 12 at trial 0 give
  6.5 .. 18.0), and the
  symbol is shared by the channel use's Na positions.  Positions of one subset are negatively
  correlated, which only shrinks the statistic's spread against independent placements: the
  chi-square quantile is a conservative bar.
* Floyd's rule itself: over all words the (j + 1)-subsets of {0 .. J} come out equally often
  (enumerated exactly for Nt = 5, Na = 3 with the words replaced by every value of t).
* the struct keeps its size and the field the old pad's offset; amp_synth_trials refuses a message
  outside {0, 1}; TrialSynth takes a 'random' config and still refuses real alphabets.
"""
import itertools

import numpy as np
import pytest

import synth_random_ref as srr
import synth_ref as sr

SEED, TR0 = 11, (1 << 32) + 7
CHI2_15_999 = 37.697          # 99.9 % quantile of chi-square with 15 degrees of freedom


def test_subsets_distinct_uniform_and_one_symbol():
    Nt, Na, K, E, Lin = 16, 3, 4, 200, 100                      # 20000 channel uses
    ant, k = srr.subsets(SEED, TR0, E, Lin, Nt, Na, K)
    assert ant.shape == (E, Lin, Na) and k.shape == (E, Lin)
    assert ant.min() >= 0 and ant.max() < Nt
    assert (np.diff(ant, axis=2) > 0).all()                     # ascending, hence distinct
    counts = np.bincount(ant.ravel(), minlength=Nt)
    expect = E * Lin * Na / Nt
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print('position counts', counts.tolist(), 'chi-square', chi2)
    assert chi2 < CHI2_15_999
    kc = np.bincount(k.ravel(), minlength=K)
    chi2k = float(((kc - E * Lin / K) ** 2 / (E * Lin / K)).sum())
    assert chi2k < 16.266                                       # 99.9 % quantile, 3 degrees of freedom
    # the message: Na nonzeros per channel use, all the same symbol, labels and indices in ascending order
    symbols = np.array([1, 1j, -1, -1j])
    gray = [0, 1, 3, 2]
    x, sym, idx = srr.message(SEED, TR0, E, Lin, Nt, Na, symbols, gray)
    assert x.shape == (E, Lin * Nt) and sym.shape == idx.shape == (E, Lin * Na)
    xr = x.reshape(E, Lin, Nt)
    assert ((xr != 0).sum(axis=2) == Na).all()
    assert (np.diff(idx, axis=1) > 0).all()
    for e in (0, E - 1):
        assert np.array_equal(np.flatnonzero(x[e]), idx[e])
    vals = np.take_along_axis(x, idx, axis=1).reshape(E, Lin, Na)
    assert (vals == vals[:, :, :1]).all()                       # one symbol per channel use
    assert np.array_equal(vals[:, :, 0], symbols.astype(np.complex64)[k])
    assert np.array_equal(sym.reshape(E, Lin, Na), np.broadcast_to(np.asarray(gray)[k][:, :, None], (E, Lin, Na)))


def test_draw_does_not_depend_on_the_grouping():
    a = srr.message(SEED, TR0, 6, 3, 16, 2, [1, 1j, -1, -1j], [0, 1, 3, 2])
    b = srr.message(SEED, TR0 + 4, 2, 3, 16, 2, [1, 1j, -1, -1j], [0, 1, 3, 2])
    for u, v in zip(a, b):
        assert np.array_equal(u[4:], v)
    c = srr.message(SEED + 1, TR0, 6, 3, 16, 2, [1, 1j, -1, -1j], [0, 1, 3, 2])
    assert not np.array_equal(a[2], c[2])


def test_floyd_rule_is_exactly_uniform():
    Nt, Na = 5, 3
    seen = {}
    for ts in itertools.product(*[range(Nt - Na + j + 1) for j in range(Na)]):
        chosen = []
        for j, t in enumerate(ts):
            chosen.append(Nt - Na + j if t in chosen else t)
        key = tuple(sorted(chosen))
        seen[key] = seen.get(key, 0) + 1
    assert len(seen) == 10 and len(set(seen.values())) == 1      # C(5, 3) subsets, equally often


def test_mulhi_draws_cover_the_range():
    w = np.array([0, 2 ** 32 - 1, 2 ** 31], dtype=np.uint32)
    assert sr.mulhi32(w, 14).tolist() == [0, 13, 7]


def test_message_field_keeps_the_struct():
    import ctypes as C
    import amp_native as nat
    import os
    assert C.sizeof(nat.AmpSynthArgs) == 104
    assert nat.AmpSynthArgs.message.offset == 60 and nat.AmpSynthArgs.x.offset == 64
    assert nat.AmpSynthArgs().message == 0                      # what every earlier caller passes
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'amp_sparc.h')).read()
    assert 'int32_t message;' in header


def _cfg(mode='random', alphabet='QPSK', is_complex=True):
    from config import Config
    return Config(16, 2, 7, 2, 3, batch=1, generator_mode=mode, iterations=5, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', is_complex=is_complex, device='cpu')


def test_synth_trials_refuses_an_unknown_message():
    import ctypes as C
    import amp_native as nat
    lib = nat.lib()
    cfg = _cfg()
    cst, d = cfg.constellation(), cfg.dims(batch=1)
    a = nat.AmpSynthArgs()
    for k in ('sw', 'A', 'At', 'x', 'sym', 'idx', 'y'):
        setattr(a, k, 256)                                       # never read: the call is refused first
    for bad in (2, -1):
        a.message = bad
        rc = lib.amp_synth_trials(C.byref(d), C.byref(cst), C.byref(a), 4, 2, None)
        assert rc == -1 and 'message' in lib.amp_last_error().decode()


def test_trial_synth_takes_random_configs():
    from synth import TrialSynth
    assert TrialSynth(_cfg(), 3).config.mode == 'random'
    with pytest.raises(ValueError, match='complex'):
        TrialSynth(_cfg(alphabet='OOK', is_complex=False), 3)
