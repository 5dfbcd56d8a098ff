"""Inputs of the g14 SCAMP independent-trial points (tests/golden/make_g14_scamp_trials.py),
regenerated with the build's host RNG replica in the reference's call order: np.random.seed /
torch.manual_seed, ONE Channel.generate_as_sparc, then E x (Data.generate_message,
A @ x + Channel.awgn(SNR)).  Computed once per point and shared (read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g14_scamp_trials.json')) as f:
    G14 = json.load(f)
POINTS = sorted(G14)
E_G14 = 40


def config_of(name, device='cpu', iterations=None, mode='segmented', batch=1):
    from config import Config
    e = G14[name]
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=batch, generator_mode=mode,
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    """dict(W, A, SNR, x[E], sym[E], idx[E], y[E]) on the CPU."""
    from channel import Channel
    from data import Data
    e = G14[name]
    cfg = config_of(name)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    SNR = cfg.snr(e['EbN0'])
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E_G14):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(W=W, A=A, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys)


@functools.lru_cache(maxsize=None)
def device_inputs(name, device='cuda'):
    h = host_inputs(name)
    out = dict(h)
    out['W'], out['A'] = h['W'].to(device), h['A'].to(device)
    out['x'] = [t.to(device) for t in h['x']]
    out['y'] = [t.to(device) for t in h['y']]
    return out
