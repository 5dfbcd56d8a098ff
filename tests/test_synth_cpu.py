"""Trial-input synthesis, the parts that need no GPU.

* tests/synth_ref.py's Philox4x32-10 reproduces the Random123 known answers.
* The restated normals (noise, seed 11, 64 trials x 528 rows) have the moments of a unit normal
  within 6 sigma: mean, variance, re.im correlation, the |z| > 3 share; float64 and float32 forms.
* pos and k over 64 x 160 sections at M = 16, K = 4 are uniform: chi-square below 45 (15 degrees
  of freedom) and 25 (3 degrees of freedom).
* The library exports and the binding declares amp_synth_channels / amp_synth_trials; both answer
  AMP_E_ARG with a message to bad arguments before anything is launched.
* Model(synth_trials=True) raises with rng='host', with B > 1 and without group_trials; with a
  stand-in TrialSynth and detector it makes the calls, and hands out the ids, that the grouping
  promises: trial id = (point << 32) + epoch, channel id = (point << 32) + epoch // res, whatever
  group_trials / trial_channels.
"""
import math
import os

import numpy as np
import pytest
import torch

import synth_ref as sr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hex(words):
    return ' '.join(f'{int(w):08x}' for w in words)


@pytest.mark.parametrize('ctr, key, want', [
    ((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     'd16cfe09 94fdcceb 5001e420 24126ea1')])
def test_philox_known_answers(ctr, key, want):
    out = sr.philox4x32_10(*[np.uint64(c) for c in ctr], *key)
    assert _hex(out) == want
    # vectorised: the same block inside an array of counters
    c0 = np.array([1, ctr[0], 2], dtype=np.uint64)
    out = sr.philox4x32_10(c0, np.uint64(ctr[1]), np.uint64(ctr[2]), np.uint64(ctr[3]), *key)
    assert _hex(w[1] for w in out) == want


def test_draw_is_counter_index_id_stream():
    seed, ident = 0x299f31d0a4093822, 0x13198a2e85a308d3
    w = sr.draw(seed, 0x03707344, ident, 0x243f6a88)
    assert _hex(w) == 'd16cfe09 94fdcceb 5001e420 24126ea1'


@pytest.mark.parametrize('f32', [False, True])
def test_normal_moments(f32):
    re, im = sr.unit_noise(11, 0, 64, 528, f32=f32)
    re, im = re.astype(np.float64).ravel(), im.astype(np.float64).ravel()
    z = np.concatenate([re, im])
    n2, n1 = z.size, re.size
    p3 = math.erfc(3 / math.sqrt(2))
    figures = {'mean': (z.mean(), 0.0, 1 / math.sqrt(n2)),
               'variance': (z.var(), 1.0, math.sqrt(2 / n2)),
               're.im': ((re * im).mean(), 0.0, 1 / math.sqrt(n1)),
               '|z|>3': ((np.abs(z) > 3).mean(), p3, math.sqrt(p3 * (1 - p3) / n2))}
    for name, (got, want, sigma) in figures.items():
        print(f'{name}: {got:.6f} (expected {want:.6f}, {(got - want) / sigma:+.2f} sigma)')
    for name, (got, want, sigma) in figures.items():
        assert abs(got - want) <= 6 * sigma, name
    assert np.isfinite(z).all()


def test_float32_normals_stay_close_to_float64():
    a = sr.unit_noise(11, 0, 64, 528, f32=True)
    b = sr.unit_noise(11, 0, 64, 528, f32=False)
    dev = max(float(np.max(np.abs(a[i].astype(np.float64) - b[i]))) for i in range(2))
    print('largest float32 deviation of a unit normal:', dev)
    assert 0 < dev and 4 * dev <= 1e-5        # the GPU tests' bar (4 x this) may never exceed 1e-5


def test_sections_uniform():
    pos, k = sr.sections(11, 0, 64, 160, 16, 4)
    assert pos.shape == k.shape == (64, 160)
    assert pos.min() == 0 and pos.max() == 15 and k.min() == 0 and k.max() == 3
    chi = {}
    for name, v, m in (('pos', pos, 16), ('k', k, 4)):
        cnt = np.bincount(v.ravel(), minlength=m).astype(np.float64)
        exp = v.size / m
        chi[name] = float(((cnt - exp) ** 2 / exp).sum())
    print('chi-square', chi)
    assert chi['pos'] < 45 and chi['k'] < 25


def test_message_places_one_symbol_per_section():
    from config import Config
    cfg = Config(16, 2, 7, 4, 3, batch=1, generator_mode='segmented', alphabet='QPSK', channel_profile='uniform',
                 channel_truncation='tail', device='cpu')
    L, M = cfg.Na * cfg.Lin, cfg.Nt // cfg.Na
    x, sym, idx = sr.message(3, 5, 4, L, M, cfg.symbols, cfg.gray)
    assert x.shape == (4, L * M) and sym.shape == idx.shape == (4, L)
    for e in range(4):
        assert np.array_equal(np.flatnonzero(x[e]), idx[e])
        assert np.array_equal(idx[e] // M, np.arange(L))
    # ids, not positions in a call: trial 7 is the same alone and as the third of a call from 5
    x1, sym1, idx1 = sr.message(3, 7, 1, L, M, cfg.symbols, cfg.gray)
    assert np.array_equal(x1[0], x[2]) and np.array_equal(sym1[0], sym[2]) and np.array_equal(idx1[0], idx[2])


def test_channel_restatement_blocks():
    Nt, Na, Nr, Lh, Lin = 16, 2, 7, 3, 4
    Lout = Lin + Lh - 1
    sw = np.sqrt(np.arange(1, Lout * Lin + 1, dtype=np.float64).reshape(Lout, Lin)).astype(np.float32)
    A = sr.channel(9, 2, sw, Nt, Na, Nr, Lh, Lin)
    mask = sr.channel_mask(Lout, Nt, Nr, Lh, Lin)
    assert A.shape == mask.shape == (Nr * Lout, Nt * Lin)
    assert not A[~mask].any() and (A[mask] != 0).all()
    re, im = sr.taps(9, 2, Nr, Nt, Lh)
    h = (re + 1j * im) / np.sqrt(2 * Na * Lin)
    assert np.array_equal(A[2 * Nr:3 * Nr, Nt:2 * Nt], np.float64(sw[2, 1]) * h[:, :, 1])
    A32 = sr.channel(9, 2, sw, Nt, Na, Nr, Lh, Lin, f32=True)
    assert A32.dtype == np.complex64 and np.max(np.abs(A32 - A)) < 1e-5 * np.max(sw)


def test_synth_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in ('amp_synth_channels', 'amp_synth_trials'):
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    assert 'typedef struct amp_synth_args' in header


def test_synth_entry_points_refuse_bad_arguments():
    """AMP_E_ARG with a message, before anything is launched (no device is touched here: the pointers
    below are never read)."""
    import ctypes as C
    import amp_native as nat
    from config import Config
    lib = nat.lib()
    cfg = _cfg()
    cst = cfg.constellation()

    def args(**kw):
        a = nat.AmpSynthArgs()
        for k in ('sw', 'A', 'At', 'x', 'sym', 'idx', 'y'):
            setattr(a, k, 256)
        a.Lh = cfg.Lh
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def channels(d, a, G):
        return lib.amp_synth_channels(C.byref(d), C.byref(a), G, None), lib.amp_last_error().decode()

    def trials(d, a, E, R, c=cst):
        return lib.amp_synth_trials(C.byref(d), C.byref(c), C.byref(a), E, R, None), lib.amp_last_error().decode()

    d = cfg.dims(batch=1)
    odd = cfg.dims(batch=1)
    odd.N += 1
    long = Config(16, 2, 7, 2100, 3, batch=1, generator_mode='segmented', alphabet='QPSK', channel_profile='uniform',
                  channel_truncation='tail', device='cpu').dims()
    k32 = nat.AmpConstellation()
    k32.K = 32
    for (rc, msg), word in [(channels(cfg.dims(batch=2), args(), 1), 'one trial'),
                            (channels(odd, args(), 1), 'inconsistent'),
                            (channels(d, args(A=None), 1), 'null pointer'),
                            (channels(d, args(), 0), 'channels'),
                            (channels(d, args(), 70000), 'channels'),
                            (channels(d, args(Lh=0), 1), 'Lh'),
                            (channels(d, args(Lh=d.Lout + 1), 1), 'Lh'),
                            (trials(cfg.dims(batch=2), args(), 4, 2), 'one trial'),
                            (trials(d, args(y=None), 4, 2), 'null pointer'),
                            (trials(d, args(), 0, 1), 'trials'),
                            (trials(d, args(), 4, 0), 'per_channel'),
                            (trials(d, args(), 70000, 1), 'channels'),
                            (trials(d, args(band_blocks=-1), 4, 2), 'band_blocks'),
                            (trials(d, args(), 4, 2, k32), 'constellation'),
                            (trials(long, args(), 4, 2), 'LDS')]:
        assert rc == -1 and word in msg, (rc, msg, word)


# ---- Model(synth_trials=True) with stand-ins ----

def _cfg(B=1, mode='segmented'):
    from config import Config
    return Config(16, 2, 7, 4, 3, batch=B, generator_mode=mode, iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


class FakeSynth:
    """TrialSynth's two calls on the host: tensors that carry their ids."""

    def __init__(self, cfg):
        self.d = cfg.dims(batch=1)
        self.log = []

    def channels(self, G, channel0):
        self.log.append(('channels', G, channel0))
        d = self.d
        ids = torch.arange(G, dtype=torch.float32) + float(channel0 % 2 ** 20)
        A = ids.view(G, 1, 1).expand(G, d.n, d.N).to(torch.complex64).contiguous()
        return torch.ones(d.Lout, d.Lin), A, A.transpose(1, 2).contiguous()

    def trials(self, At, E, per_channel, SNR, trial0, band=True, want_noise=False):
        self.log.append(('trials', E, per_channel, trial0))
        d = self.d
        assert At.shape == (-(-E // per_channel), d.N, d.n)
        ids = torch.arange(E, dtype=torch.float32) + float(trial0 % 2 ** 20)
        y = ids.view(E, 1).expand(E, d.n).to(torch.complex64).contiguous()
        return (torch.zeros(E, d.N, dtype=torch.complex64), torch.zeros(E, d.L, dtype=torch.int64),
                torch.zeros(E, d.L, dtype=torch.int64), y)


class FakeBamp:
    """BAMP's forward_trials: each trial's Loss carries its own y and its own channel."""

    def __init__(self, cfg):
        from loss import Loss
        self.Loss, self.config = Loss, cfg
        self.seen = []

    def __call__(self, *a):
        raise AssertionError('synth_trials detects every call through forward_trials')

    def forward_trials(self, H, ys, SNR, xs, syms, idxs, per_channel=None):
        E = len(ys)
        assert E == len(xs) == len(syms) == len(idxs)
        if per_channel is None:
            assert H.dim() == 2
            chans = [H] * E
        else:
            assert H.dim() == 3 and H.shape[0] == -(-E // per_channel) > 1
            chans = [H[e // per_channel] for e in range(E)]
        out = []
        for y, ch in zip(ys, chans):
            self.seen.append((float(y[0].real), float(ch[0, 0].real)))
            L = self.Loss(self.config)
            v = float(y[0].real) + 0.01 * float(ch[0, 0].real)
            L.record([v % 1.0] + [v] * 13, 3)
            out.append(L)
        return out


def test_model_synth_trials_refusals(tmp_path):
    from model import Model
    cfg = _cfg()
    kw = dict(path=str(tmp_path), amp=FakeBamp(cfg), seed=3)
    with pytest.raises(ValueError, match='synth_trials'):
        Model(cfg, 'bamp', rng='host', group_trials=8, synth_trials=True, **kw)
    with pytest.raises(ValueError, match='synth_trials'):
        Model(cfg, 'bamp', rng='device', synth_trials=True, **kw)                   # no group_trials
    with pytest.raises(ValueError):
        Model(_cfg(B=2), 'bamp', rng='device', group_trials=8, synth_trials=True, path=str(tmp_path),
              amp=FakeBamp(_cfg(B=2)), seed=3)
    m = Model(cfg, 'bamp', rng='device', group_trials=8, synth_trials=True, **kw)
    assert m.synth is not None and m.synth.seed == 3
    assert Model(cfg, 'bamp', rng='device', group_trials=8, **kw).synth is None     # opt-in


P1 = 1 << 32
# (res, group_trials, trial_channels) -> TrialSynth's calls at the first SNR point over 10 epochs
SYNTH_CASES = {
    (4, 8, 2): [('channels', 2, 0), ('trials', 8, 4, 0), ('channels', 1, 2), ('trials', 2, 2, 8)],
    (1, 8, 8): [('channels', 8, 0), ('trials', 8, 1, 0), ('channels', 2, 8), ('trials', 2, 1, 8)],
    (3, 7, 4): [('channels', 2, 0), ('trials', 6, 3, 0), ('channels', 2, 2), ('trials', 4, 3, 6)],
    (4, 3, 0): [('channels', 1, 0), ('trials', 3, 3, 0), ('trials', 1, 1, 3),        # a block longer than n:
                ('channels', 1, 1), ('trials', 3, 3, 4), ('trials', 1, 1, 7),        # its channel drawn once
                ('channels', 1, 2), ('trials', 2, 2, 8)],
    (4, 3, 2): [('channels', 1, 0), ('trials', 3, 3, 0), ('trials', 1, 1, 3),
                ('channels', 1, 1), ('trials', 3, 3, 4), ('trials', 1, 1, 7),
                ('channels', 1, 2), ('trials', 2, 2, 8)],
}


@pytest.mark.parametrize('case', sorted(SYNTH_CASES))
def test_model_synth_trials_calls_and_ids(tmp_path, case):
    import json
    from model import Model
    res, gt, tcap = case
    cfg = _cfg()
    runs = {}
    for key, kw in (('one', dict(group_trials=1)), ('grouped', dict(group_trials=gt, trial_channels=tcap))):
        amp = FakeBamp(cfg)
        m = Model(cfg, 'bamp', path=str(tmp_path / key), amp=amp, seed=11, rng='device', synth_trials=True, **kw)
        m.synth = FakeSynth(cfg)
        runs[key] = (amp, m.synth, m.simulate(epochs=10, start=0, final=1.0, step=1, res=res))
    amp, synth, points = runs['grouped']
    want = SYNTH_CASES[case]
    shift = [(c[0], c[1], c[2] + P1) if c[0] == 'channels' else (c[0], c[1], c[2], c[3] + P1) for c in want]
    assert synth.log == want + shift                                        # the second point: ids + (1 << 32)
    # every epoch detected once, in order, with the channel of its block, however it was grouped
    assert amp.seen == [(float(i), float(i // res)) for i in range(10)] * 2
    assert runs['one'][0].seen == amp.seen
    assert json.dumps(runs['one'][2], sort_keys=True) == json.dumps(points, sort_keys=True)
    for p in ('0.0.json', '1.0.json'):
        assert open(tmp_path / 'one' / p, 'rb').read() == open(tmp_path / 'grouped' / p, 'rb').read()


def test_model_synth_trials_counts_the_transposes(tmp_path):
    """trials_ws_limit caps the channels per call on the workspace query plus At's bytes."""
    from model import Model
    cfg = _cfg()
    d = cfg.dims(batch=1)
    at = 8 * d.N * d.n
    amp = FakeBamp(cfg)
    amp.trials_workspace_bytes = lambda trials, per: 1000 * (-(-trials // per))
    m = Model(cfg, 'bamp', path=str(tmp_path), amp=amp, seed=2, rng='device', synth_trials=True, group_trials=8,
              trial_channels=8, trials_ws_limit=3 * (1000 + at) + 500)
    m.synth = FakeSynth(cfg)
    m.simulate(epochs=10, start=0, final=0.0, step=1, res=1)
    assert [c[1] for c in m.synth.log if c[0] == 'channels'] == [3, 3, 3, 1]
