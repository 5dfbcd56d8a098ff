"""Trial-input synthesis on the GPU (amp_synth_channels / amp_synth_trials through synth.TrialSynth)
against tests/synth_ref.py, at shapes (Nt, Na, Nr, Lh, Lin):
(6,3,5,1,1) OOK E = 3; (16,2,7,3,4) QPSK E = 5, R = 2 (G = 3, a short last channel);
(64,4,8,1,1) 16-QAM E = 4; (128,8,24,3,20) OOK E = 33, R = 32 (G = 2, rows beyond one 256-row
workgroup, 32-wide tiles with partial edges).

1. x, sym and idx equal the restatement exactly.
2. Channels: zero blocks of A exactly zero, At bitwise A transposed, non-zero blocks within the bar
   of f32(sw) h_ref.  The bar, per unit normal: 4 x the float32 restatement's own largest deviation
   from the float64 one (computed here, on the same draws; the 4 allows for device libm differing
   by ulps), and never above 1e-5.  The same bar for the noise.
3. y - noise agrees with a float64 A x formed from the kernel's own A and x, per element within
   (Na Lh + 4) 2^-24 sum |A_jc| |s_c| + 2^-24 |y_j|.
4. band=True and band=False give numerically equal y on a synthesized channel.
5. band=False on a dense random A (At from torch) satisfies 3.
6. One call of E trials equals two calls with trial0 advanced, bit for bit; another seed gives the
   restatement's outputs for that seed and changes every normal.
7. Model, BAMP, (16,2,7,2,3) QPSK 'segmented': 24 epochs at res = 4 export identical metrics for
   (group_trials, trial_channels) = (8, 2), (24, 6), (4, 0); VER and SER of 1600 synthesized trials
   lie within 6 sigma + 1e-3 of the rng='host' sweep's over 400 trials at EbN0 = EBN0 dB (see there).
8. forward_trials on the synthesized stacks equals sequential forwards on their rows (BAMP, SCAMP,
   VAMP; one small point each).
"""
import functools
import json

import numpy as np
import pytest
import torch

import synth_ref as sr

pytestmark = pytest.mark.gpu

# name: (Nt, Na, Nr, Lh, Lin, alphabet, E, R)   R = E: one channel
CASES = {'ook_6': (6, 3, 5, 1, 1, 'OOK', 3, 3),
         'qpsk_16': (16, 2, 7, 3, 4, 'QPSK', 5, 2),
         'qam_64': (64, 4, 8, 1, 1, '16QAM', 4, 4),
         'ook_128': (128, 8, 24, 3, 20, 'OOK', 33, 32)}
SEED, CH0, TR0, SNR = 11, (3 << 32) + 5, (1 << 32) + 7, 10.0
U24 = 2.0 ** -24


def _config(name, mode='segmented', iterations=20):
    from config import Config
    Nt, Na, Nr, Lh, Lin, alpha, _, _ = CASES[name]
    return Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode=mode, iterations=iterations, alphabet=alpha,
                  channel_profile='uniform', channel_truncation='tail', device='cuda')


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def point(name, seed=SEED):
    """One synthesis of the case on the GPU and its restatement.  Computed once, shared, never modified."""
    from channel import Channel
    from synth import TrialSynth
    cfg = _config(name)
    Nt, Na, Nr, Lh, Lin, _, E, R = CASES[name]
    G = -(-E // R)
    syn = TrialSynth(cfg, seed)
    W, A, At = syn.channels(G, CH0)
    x, sym, idx, y, noise = syn.trials(At, E, R, SNR, TR0, want_noise=True)
    y_full = syn.trials(At, E, R, SNR, TR0, band=False)[3]
    torch.cuda.synchronize()
    sw = np.sqrt(Channel(cfg)._base_matrix()).astype(np.float32)
    return dict(cfg=cfg, syn=syn, G=G, E=E, R=R, W=W, A=A, At=At, x=x, sym=sym, idx=idx, y=y, noise=noise,
                y_full=y_full, sw=sw)


def _unit_scale(name, sw):
    """|f32(sw)[o, i]| / sqrt(2 Na Lin) on every element of A's band, 0 off it: what one unit of a
    tap's normal is worth in A."""
    Nt, Na, Nr, Lh, Lin, *_ = CASES[name]
    Lout = sw.shape[0]
    o = np.arange(Nr * Lout)[:, None] // Nr
    i = np.arange(Nt * Lin)[None, :] // Nt
    mask = sr.channel_mask(Lout, Nt, Nr, Lh, Lin)
    return np.where(mask, sw.astype(np.float64)[o, i] / np.sqrt(2.0 * Na * Lin), 0.0), mask


def _product_bound(name, absA, absx, y):
    Nt, Na, Nr, Lh, Lin, *_ = CASES[name]
    return (Na * Lh + 4) * U24 * (absA @ absx) + U24 * np.abs(y)


@pytest.mark.parametrize('name', sorted(CASES))
def test_message_equals_restatement(device, name):                                   # 1.
    p = point(name)
    cfg = p['cfg']
    L, M = cfg.Na * cfg.Lin, cfg.Nt // cfg.Na
    x, sym, idx = sr.message(SEED, TR0, p['E'], L, M, cfg.symbols, cfg.gray)
    assert p['x'].shape == (p['E'], L * M) and p['sym'].shape == p['idx'].shape == (p['E'], L)
    assert p['sym'].dtype == p['idx'].dtype == torch.int64
    assert np.array_equal(_np(p['x']).view(np.float32), x.view(np.float32))
    assert np.array_equal(_np(p['sym']), sym)
    assert np.array_equal(_np(p['idx']), idx)


@pytest.mark.parametrize('name', sorted(CASES))
def test_channels(device, name):                                                     # 2.
    p = point(name)
    Nt, Na, Nr, Lh, Lin, *_ = CASES[name]
    A, At = _np(p['A']), _np(p['At'])
    assert A.shape == (p['G'], Nr * (Lin + Lh - 1), Nt * Lin)
    assert np.array_equal(At.view(np.float32), np.ascontiguousarray(A.transpose(0, 2, 1)).view(np.float32))
    unit, mask = _unit_scale(name, p['sw'])
    W = np.asarray(_np(p['W']), dtype=np.float64)
    assert np.array_equal(np.float32(np.sqrt(W)) != 0, p['sw'] != 0)
    for g in range(p['G']):
        assert not A[g][~mask].view(np.float32).any()                                # exact zeros (no -0 either)
        ref = sr.channel(SEED, CH0 + g, p['sw'], Nt, Na, Nr, Lh, Lin)
        ref32 = sr.channel(SEED, CH0 + g, p['sw'], Nt, Na, Nr, Lh, Lin, f32=True)
        dev = float(np.max(np.abs(ref32.astype(np.complex128) - ref)[mask] / unit[mask]))
        bar = 4 * dev
        got = float(np.max(np.abs(A[g].astype(np.complex128) - ref)[mask] / unit[mask]))
        print(f'{name} channel {g}: float32 restatement deviates {dev:.3e} per unit normal, bar {bar:.3e}, '
              f'kernel {got:.3e}')
        assert 0 < bar <= 1e-5
        assert got <= bar
        assert (A[g][mask] != 0).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_noise(device, name):                                                        # 2. (noise)
    p = point(name)
    cfg = p['cfg']
    n = cfg.Nr * cfg.Lout
    std = sr.noise_std(cfg.Na, cfg.Nr, SNR)
    re, im = sr.unit_noise(SEED, TR0, p['E'], n)
    re32, im32 = sr.unit_noise(SEED, TR0, p['E'], n, f32=True)
    s32 = np.float32(std)
    ref = (re + 1j * im) * std
    ref32 = ((re32 * s32).astype(np.float64) + 1j * (im32 * s32).astype(np.float64))
    dev = float(np.max(np.abs(ref32 - ref))) / std
    bar = 4 * dev
    got = float(np.max(np.abs(_np(p['noise']).astype(np.complex128) - ref))) / std
    print(f'{name} noise: float32 restatement deviates {dev:.3e} per unit normal, bar {bar:.3e}, kernel {got:.3e}')
    assert 0 < bar <= 1e-5
    assert got <= bar


@pytest.mark.parametrize('name', sorted(CASES))
def test_y_is_A_x_plus_noise(device, name):                                          # 3. and 4.
    p = point(name)
    A = _np(p['A']).astype(np.complex128)
    x = _np(p['x']).astype(np.complex128)
    y, noise = _np(p['y']), _np(p['noise'])
    worst = 0.0
    for e in range(p['E']):
        g = e // p['R']
        ref = A[g] @ x[e]
        bound = _product_bound(name, np.abs(A[g]), np.abs(x[e]), y[e])
        err = np.abs((y[e].astype(np.complex128) - noise[e].astype(np.complex128)) - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert (err <= bound).all(), (e, float(np.max(err / bound)))
    print(f'{name}: largest |y - noise - A x| / bound = {worst:.3f}')
    assert np.array_equal(y, _np(p['y_full']))                                       # 4. (-0 == 0)
    assert np.isfinite(y.view(np.float32)).all()


@pytest.mark.parametrize('name', sorted(CASES))
def test_dense_channel_without_band(device, name):                                   # 5.
    p = point(name)
    cfg = p['cfg']
    n, N = cfg.Nr * cfg.Lout, cfg.Nt * cfg.Lin
    gen = torch.Generator(device='cuda').manual_seed(4)
    A = torch.randn(p['G'], n, N, dtype=torch.complex64, device='cuda', generator=gen) / np.sqrt(cfg.Na * cfg.Lin)
    At = A.transpose(1, 2).contiguous()
    x, sym, idx, y, noise = p['syn'].trials(At, p['E'], p['R'], SNR, TR0, band=False, want_noise=True)
    assert torch.equal(x, p['x']) and torch.equal(noise, p['noise'])                 # the draws do not see A
    A64, x64, y, noise = _np(A).astype(np.complex128), _np(x).astype(np.complex128), _np(y), _np(noise)
    for e in range(p['E']):
        g = e // p['R']
        bound = _product_bound(name, np.abs(A64[g]), np.abs(x64[e]), y[e])
        err = np.abs((y[e].astype(np.complex128) - noise[e].astype(np.complex128)) - A64[g] @ x64[e])
        assert (err <= bound).all(), (e, float(np.max(err / bound)))


@pytest.mark.parametrize('name', sorted(CASES))
def test_call_grouping_and_seed(device, name):                                       # 6.
    p = point(name)
    E, R, syn, At = p['E'], p['R'], p['syn'], p['At']
    h = R if R < E else E // 2                              # a split on a channel boundary
    first = syn.trials(At[:1] if R < E else At, h, R if R < E else h, SNR, TR0, want_noise=True)
    rest = syn.trials(At[h // R:] if R < E else At, E - h, R if R < E else E - h, SNR, TR0 + h, want_noise=True)
    for key, a, b in zip(('x', 'sym', 'idx', 'y', 'noise'), first, rest):
        both = torch.cat([a, b])
        assert torch.equal(torch.view_as_real(both) if both.is_complex() else both,
                           torch.view_as_real(p[key]) if both.is_complex() else p[key]), key
    _, A1, At1 = syn.channels(1, CH0 + p['G'] - 1)          # the last channel alone
    assert torch.equal(torch.view_as_real(A1[0]), torch.view_as_real(p['A'][-1]))
    assert torch.equal(torch.view_as_real(At1[0]), torch.view_as_real(At[-1]))
    # another seed: the restatement's message for that seed, and no normal left as it was
    q = point(name, seed=SEED + 1)
    cfg = p['cfg']
    L, M = cfg.Na * cfg.Lin, cfg.Nt // cfg.Na
    x, sym, idx = sr.message(SEED + 1, TR0, E, L, M, cfg.symbols, cfg.gray)
    assert np.array_equal(_np(q['x']).view(np.float32), x.view(np.float32))
    assert np.array_equal(_np(q['sym']), sym) and np.array_equal(_np(q['idx']), idx)
    if M ** (E * L) >= 2 ** 64:                             # a chance coincidence of all positions is negligible
        assert not torch.equal(q['idx'], p['idx'])
    _, mask = _unit_scale(name, p['sw'])
    m = torch.from_numpy(mask).to('cuda')
    assert bool((torch.view_as_real(q['A'])[:, m] != torch.view_as_real(p['A'])[:, m]).all())
    assert bool((torch.view_as_real(q['noise']) != torch.view_as_real(p['noise'])).all())
    assert bool((torch.view_as_real(q['y']) != torch.view_as_real(p['y'])).all())


# ---- 7. Model ----

# The point of the statistical comparison: the rng='host' sweep of this shape (BAMP, 200 trials per point,
# res = 1, seed 5) gave VER 0.665 / 0.430 / 0.218 / 0.080 at EbN0 = 0 / 2 / 4 / 6 dB, so 2 dB is mid-range.
EBN0 = 2.0


def _model_cfg():
    from config import Config
    return Config(16, 2, 7, 3, 2, batch=1, generator_mode='segmented', iterations=20, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cuda')


def test_model_grouping_does_not_change_the_metrics(device, tmp_path):
    from model import Model
    out = {}
    for gt, tc in ((8, 2), (24, 6), (4, 0)):
        m = Model(_model_cfg(), 'bamp', path=str(tmp_path / f'{gt}_{tc}'), seed=5, rng='device', group_trials=gt,
                  trial_channels=tc, synth_trials=True)
        out[gt, tc] = m.simulate(epochs=24, start=EBN0, final=EBN0 + 1, step=1, res=4)
    base = out[8, 2]
    assert len(base) == 2                                   # two points: the ids carry the point index
    assert base[0]['ver'] != base[1]['ver'] or base[0]['nMSE'] != base[1]['nMSE']
    for key in ((24, 6), (4, 0)):
        assert json.dumps(out[key], sort_keys=True) == json.dumps(base, sort_keys=True), key
        for pt in base:
            f = f"{pt['EbN0dB']}.json"
            assert open(tmp_path / '8_2' / f, 'rb').read() == open(tmp_path / f'{key[0]}_{key[1]}' / f, 'rb').read()


def test_model_statistics(device, tmp_path):
    """VER and SER of the synthesized sweep against the rng='host' sweep.  res = 1: every trial has its own
    channel, so the trials are independent; a trial's error fraction lies in [0, 1] with mean p, so its
    variance is at most p (1 - p) and the difference of the two sweeps' means has
    sigma <= sqrt(p (1 - p) (1 / 400 + 1 / 1600)), p the host sweep's value.
    Measured on an MI355X at 2 dB: host VER 0.4358 SER 0.2067, synthesized VER 0.4740 SER 0.2251
    (1.4 and 0.8 sigma)."""
    from model import Model
    host = Model(_model_cfg(), 'bamp', path=str(tmp_path / 'host'), seed=5, rng='host', group_trials=8,
                 trial_channels=8).simulate(epochs=400, start=EBN0, final=EBN0, step=1, res=1)[0]
    syn = Model(_model_cfg(), 'bamp', path=str(tmp_path / 'synth'), seed=5, rng='device', group_trials=64,
                trial_channels=64, synth_trials=True).simulate(epochs=1600, start=EBN0, final=EBN0, step=1, res=1)[0]
    print(f"EbN0 {EBN0} dB: host VER {host['ver']:.4f} SER {host['ser']:.4f} FER {host['fer']:.4f}; "
          f"synthesized VER {syn['ver']:.4f} SER {syn['ser']:.4f} FER {syn['fer']:.4f}")
    assert 0.2 <= host['ver'] <= 0.8, host['ver']           # the point is mid-range
    for k in ('ver', 'ser'):
        p = host[k]
        sigma = np.sqrt(p * (1 - p) * (1 / 400 + 1 / 1600))
        assert abs(syn[k] - p) <= 6 * sigma + 1e-3, (k, syn[k], p, sigma)


# ---- 8. forward_trials on the stacks ----

def _record(L):
    from loss import counts_to_vector
    return int(L.loss['T']), [float(v) for v in counts_to_vector(L.last_counts)]


@pytest.mark.parametrize('algo', ['bamp', 'scamp', 'vamp'])
def test_forward_trials_on_the_stacks(device, algo):
    import amp_native as nat
    from model import svd_gram
    p = point('qpsk_16')
    cfg = _config('qpsk_16', mode='sparc')
    E, R, G = p['E'], p['R'], p['G']
    n, N = cfg.Nr * cfg.Lout, cfg.Nt * cfg.Lin
    if algo == 'bamp':
        from bamp import BAMP
        det, chans = BAMP(cfg), (p['A'],)
        one = lambda g: (p['A'][g],)                                                 # noqa: E731
    elif algo == 'scamp':
        from scamp import SCAMP
        det, chans = SCAMP(cfg, engine=nat.ENGINE_LAUNCHES), (p['W'], p['A'])
        one = lambda g: (p['W'], p['A'][g])                                          # noqa: E731
    else:
        from vamp import VAMP
        det = VAMP(cfg, engine=nat.ENGINE_LAUNCHES)
        chans = tuple(t.resolve_conj().contiguous() for t in svd_gram(p['A']))
        assert chans[0].shape == (G, n, min(n, N))
        one = lambda g: tuple(t[g] for t in chans)                                   # noqa: E731
    got = [_record(L) for L in det.forward_trials(*chans, p['y'], SNR, p['x'], p['sym'], p['idx'], per_channel=R)]
    for e in range(E):
        L = det(*one(e // R), p['y'][e].reshape(1, n, 1), SNR, p['x'][e].reshape(1, N, 1), p['sym'][e], p['idx'][e])
        ref = _record(L)
        assert got[e][0] == ref[0], (e, got[e][0], ref[0])
        assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(got[e][1], ref[1])), (e, got[e], ref)
