"""The 'random' message of the trial-input synthesis on the GPU (amp_synth_trials with
amp_synth_args.message = 1, through synth.TrialSynth on a generator_mode='random' config) against
tests/synth_random_ref.py, at (Nt, Na, Nr, Lin, Lh) = (16, 2, 7, 2, 3) QPSK and (32, 4, 12, 3, 2)
16-QAM, E = 37 trials at per_channel R in {1, 5} (37 and 8 channels, a short last one).

1. x, sym and idx equal the numpy restatement bit for bit; every channel use has Na nonzeros.
2. y - noise agrees with a float64 A x formed from the kernel's own A and x, per element within
   (Na Lh + 4) 2^-24 sum |A_jc| |s_c| + 2^-24 |y_j| (test_gpu_synth.py item 3's bound).
3. the noise is within test_gpu_synth.py item 2's bar of the float64 restatement (4 x the float32
   restatement's own largest deviation, never above 1e-5).
4. one call of E trials equals two calls with trial0 advanced, bit for bit.
5. message = 0 is untouched: in the same run a 'segmented' TrialSynth of the same shape, seed and
   ids returns the segmented restatement's x / sym / idx (tests/synth_ref.py, as before), the same
   channels bit for bit and the same noise bit for bit (the noise stream does not see the message).
6. Model(cfg, 'bamp', rng='device', group_trials=g, trial_channels=c, synth_trials=True) in 'random'
   mode, 24 epochs at res = 4: identical metrics and files for (g, c) = (8, 2), (24, 6), (4, 0).
"""
import functools
import json

import numpy as np
import pytest
import torch

import synth_random_ref as srr
import synth_ref as sr

pytestmark = pytest.mark.gpu

# name: (Nt, Na, Nr, Lin, Lh, alphabet)
CASES = {'qpsk_16': (16, 2, 7, 2, 3, 'QPSK'), 'qam_32': (32, 4, 12, 3, 2, '16QAM')}
E = 37
SEED, CH0, TR0, SNR = 11, (3 << 32) + 5, (1 << 32) + 7, 10.0
U24 = 2.0 ** -24


def _config(name, mode='random'):
    from config import Config
    Nt, Na, Nr, Lin, Lh, alpha = CASES[name]
    return Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode=mode, iterations=20, alphabet=alpha,
                  channel_profile='uniform', channel_truncation='tail', device='cuda')


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def point(name, R, mode='random'):
    """One synthesis of the case on the GPU.  Computed once, shared, never modified."""
    from synth import TrialSynth
    cfg = _config(name, mode)
    G = -(-E // R)
    syn = TrialSynth(cfg, SEED)
    W, A, At = syn.channels(G, CH0)
    x, sym, idx, y, noise = syn.trials(At, E, R, SNR, TR0, want_noise=True)
    torch.cuda.synchronize()
    return dict(cfg=cfg, syn=syn, G=G, R=R, A=A, At=At, x=x, sym=sym, idx=idx, y=y, noise=noise)


@pytest.mark.parametrize('R', [1, 5])
@pytest.mark.parametrize('name', sorted(CASES))
def test_random_message_equals_restatement(device, name, R):                         # 1.
    p = point(name, R)
    cfg = p['cfg']
    x, sym, idx = srr.message(SEED, TR0, E, cfg.Lin, cfg.Nt, cfg.Na, cfg.symbols, cfg.gray)
    assert p['x'].shape == (E, cfg.Lin * cfg.Nt) and p['sym'].shape == p['idx'].shape == (E, cfg.Lin * cfg.Na)
    assert p['sym'].dtype == p['idx'].dtype == torch.int64
    assert np.array_equal(_np(p['x']).view(np.float32), x.view(np.float32))
    assert np.array_equal(_np(p['sym']), sym)
    assert np.array_equal(_np(p['idx']), idx)
    assert ((_np(p['x']).reshape(E, cfg.Lin, cfg.Nt) != 0).sum(axis=2) == cfg.Na).all()


@pytest.mark.parametrize('R', [1, 5])
@pytest.mark.parametrize('name', sorted(CASES))
def test_random_y_is_A_x_plus_noise(device, name, R):                                # 2.
    p = point(name, R)
    Nt, Na, Nr, Lin, Lh, _ = CASES[name]
    A = _np(p['A']).astype(np.complex128)
    x = _np(p['x']).astype(np.complex128)
    y, noise = _np(p['y']), _np(p['noise'])
    worst = 0.0
    for e in range(E):
        g = e // R
        ref = A[g] @ x[e]
        bound = (Na * Lh + 4) * U24 * (np.abs(A[g]) @ np.abs(x[e])) + U24 * np.abs(y[e])
        err = np.abs((y[e].astype(np.complex128) - noise[e].astype(np.complex128)) - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (e, float(np.max(err / bound)))
    print(f'{name} R = {R}: largest |y - noise - A x| / bound = {worst:.3f}')
    assert np.isfinite(y.view(np.float32)).all()
    # the band ranges skip only zero blocks: every section summed gives numerically the same y
    y_full = p['syn'].trials(p['At'], E, R, SNR, TR0, band=False)[3]
    assert np.array_equal(y, _np(y_full))


@pytest.mark.parametrize('name', sorted(CASES))
def test_random_noise(device, name):                                                 # 3.
    p = point(name, 5)
    cfg = p['cfg']
    n = cfg.Nr * cfg.Lout
    std = sr.noise_std(cfg.Na, cfg.Nr, SNR)
    re, im = sr.unit_noise(SEED, TR0, E, n)
    re32, im32 = sr.unit_noise(SEED, TR0, E, n, f32=True)
    s32 = np.float32(std)
    ref = (re + 1j * im) * std
    ref32 = ((re32 * s32).astype(np.float64) + 1j * (im32 * s32).astype(np.float64))
    dev = float(np.max(np.abs(ref32 - ref))) / std
    bar = 4 * dev
    got = float(np.max(np.abs(_np(p['noise']).astype(np.complex128) - ref))) / std
    print(f'{name} noise: float32 restatement deviates {dev:.3e} per unit normal, bar {bar:.3e}, kernel {got:.3e}')
    assert 0 < bar <= 1e-5
    assert got <= bar


def _same(a, b):
    return torch.equal(torch.view_as_real(a) if a.is_complex() else a, torch.view_as_real(b) if b.is_complex() else b)


@pytest.mark.parametrize('R', [1, 5])
@pytest.mark.parametrize('name', sorted(CASES))
def test_random_call_grouping(device, name, R):                                      # 4.
    p = point(name, R)
    syn, At = p['syn'], p['At']
    h = 4 * R                                                # a split on a channel boundary
    first = syn.trials(At[:4], h, R, SNR, TR0, want_noise=True)
    rest = syn.trials(At[4:], E - h, R, SNR, TR0 + h, want_noise=True)
    for key, a, b in zip(('x', 'sym', 'idx', 'y', 'noise'), first, rest):
        assert _same(torch.cat([a, b]), p[key]), key


@pytest.mark.parametrize('name', sorted(CASES))
def test_segmented_message_is_untouched(device, name):                               # 5.
    p, q = point(name, 5), point(name, 5, 'segmented')
    cfg = q['cfg']
    L, M = cfg.Na * cfg.Lin, cfg.Nt // cfg.Na
    x, sym, idx = sr.message(SEED, TR0, E, L, M, cfg.symbols, cfg.gray)
    assert np.array_equal(_np(q['x']).view(np.float32), x.view(np.float32))
    assert np.array_equal(_np(q['sym']), sym) and np.array_equal(_np(q['idx']), idx)
    assert _same(q['A'], p['A']) and _same(q['At'], p['At']) and _same(q['noise'], p['noise'])
    assert not _same(q['x'], p['x'])                         # the two messages are different draws
    A, xs = _np(q['A']).astype(np.complex128), _np(q['x']).astype(np.complex128)
    y, noise = _np(q['y']), _np(q['noise'])
    Nt, Na, Nr, Lin, Lh, _ = CASES[name]
    for e in range(E):
        g = e // 5
        bound = (Na * Lh + 4) * U24 * (np.abs(A[g]) @ np.abs(xs[e])) + U24 * np.abs(y[e])
        err = np.abs((y[e].astype(np.complex128) - noise[e].astype(np.complex128)) - A[g] @ xs[e])
        assert (err <= bound).all(), e


def test_model_random_mode_grouping_does_not_change_the_metrics(device, tmp_path):   # 6.
    from bamp import BAMP
    from model import Model
    out = {}
    for gt, tc in ((8, 2), (24, 6), (4, 0)):
        m = Model(_config('qpsk_16'), 'bamp', path=str(tmp_path / f'{gt}_{tc}'), seed=5, rng='device', group_trials=gt,
                  trial_channels=tc, synth_trials=True)
        assert isinstance(m.amp, BAMP) and m.amp.random_trials
        out[gt, tc] = m.simulate(epochs=24, start=4.0, final=5.0, step=1, res=4)
    base = out[8, 2]
    assert len(base) == 2                                   # two points: the ids carry the point index
    assert base[0]['ver'] != base[1]['ver'] or base[0]['nMSE'] != base[1]['nMSE']
    assert base[1]['ver'] < 0.9                             # a detector at work (the reference: 10 of 40 frames wrong at 4 dB)
    for key in ((24, 6), (4, 0)):
        assert json.dumps(out[key], sort_keys=True) == json.dumps(base, sort_keys=True), key
        for pt in base:
            f = f"{pt['EbN0dB']}.json"
            assert open(tmp_path / '8_2' / f, 'rb').read() == open(tmp_path / f'{key[0]}_{key[1]}' / f, 'rb').read()
