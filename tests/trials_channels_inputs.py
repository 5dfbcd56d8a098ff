"""Inputs of the trial-batch tests over several channels.

* g18 (tests/golden/make_g18_trials_channels.py: the reference at batch = 1, the channel redrawn
  every res = 5 epochs, 40 epochs) regenerated with the build's host RNG replica in the reference's
  call order: np.random.seed / torch.manual_seed, then per epoch Channel.generate_as_sparc when
  i % res == 0, Data.generate_message, A @ x + Channel.awgn(SNR) (golden_inputs).
* per test point (g13 / g14 / g16 shapes): 40 channels, 40 messages and 40 noise vectors drawn once
  from a seed; for a given R, trial e uses channel e // R, so y_e = A[e // R] x_e + noise_e
  (point_inputs).  Computed once per point and shared (read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g18_trials_channels.json')) as f:
    G18 = json.load(f)
with open(os.path.join(gio.GOLDEN, 'g13_trials.json')) as f:
    _G13 = json.load(f)
with open(os.path.join(gio.GOLDEN, 'g14_scamp_trials.json')) as f:
    _G14 = json.load(f)
with open(os.path.join(gio.GOLDEN, 'g16_bamp_wide.json')) as f:
    _G16 = json.load(f)

E = 40
GOLDEN_POINTS = sorted(G18)
# (detector, point, source): the smallest shapes that reach every tile case
POINTS = [('scamp', 'scamp_OOK_Nt16', _G14), ('scamp', 'scamp_QPSK_Nt32', _G14), ('scamp', 'scamp_OOK_Nt128', _G14),
          ('bamp', 'bamp_OOK_Nt16', _G13), ('bamp', 'bamp_QPSK_Nt32', _G13), ('bamp', 'trials_OOK_Nt6', _G16)]
POINT_IDS = [p[1] for p in POINTS]
_SRC = {p[1]: (p[0], p[2][p[1]]) for p in POINTS}


def algo_of(name):
    return _SRC[name][0] if name in _SRC else G18[name]['algo']


def _entry(name, golden):
    return G18[name] if golden else _SRC[name][1]


def config_of(name, device='cpu', iterations=None, golden=False, batch=1):
    from config import Config
    e = _entry(name, golden)
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=batch, generator_mode=e.get('mode', 'segmented'),
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def golden_inputs(name):
    """g18's epochs: dict(W, A[E] (the epoch's channel), SNR, x[E], sym[E], idx[E], y[E]) on the CPU."""
    from channel import Channel
    from data import Data
    e = G18[name]
    cfg = config_of(name, golden=True)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(e['EbN0'])
    As, xs, syms, idxs, ys = [], [], [], [], []
    for i in range(E):
        if i % e['res'] == 0:
            W, A = ch.generate_as_sparc()
        x, sym, idx = da.generate_message()
        As.append(A); xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(W=W, A=As, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys, res=e['res'])


@functools.lru_cache(maxsize=None)
def point_inputs(name):
    """dict(W, A[E] channels, SNR, x[E], sym[E], idx[E], noise[E]) on the CPU, drawn once from the
    point's seed."""
    from channel import Channel
    from data import Data
    e = _entry(name, False)
    cfg = config_of(name)
    np.random.seed(e['seed'] + 18)
    torch.manual_seed(e['seed'] + 18)
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(e['EbN0'])
    As = []
    for _ in range(E):
        W, A = ch.generate_as_sparc()
        As.append(A)
    xs, syms, idxs, ns = [], [], [], []
    for _ in range(E):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ns.append(ch.awgn(SNR))
    return dict(W=W, A=As, SNR=SNR, x=xs, sym=syms, idx=idxs, noise=ns)


@functools.lru_cache(maxsize=None)
def device_point(name, device='cuda'):
    h = point_inputs(name)
    out = dict(h)
    out['W'] = h['W'].to(device)
    for k in ('A', 'x', 'noise'):
        out[k] = [t.to(device) for t in h[k]]
    return out


def received(inp, e, g):
    """y of trial e through channel g (same device as the inputs)."""
    return inp['A'][g] @ inp['x'][e] + inp['noise'][e]
