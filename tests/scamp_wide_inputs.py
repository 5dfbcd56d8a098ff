"""Inputs of the g15 SCAMP points (tests/golden/make_g15_scamp_wide.py: coupling blocks wider than
128 and Nt that is no power of two), regenerated with the build's host RNG replica in the
reference's call order.  Trial points: np.random.seed / torch.manual_seed, ONE
Channel.generate_as_sparc, then E x (Data.generate_message, A @ x + Channel.awgn(SNR)) at batch = 1.
Batch points: the same with one message of B = 48 trials.  Computed once per point and shared
(read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g15_scamp_wide.json')) as f:
    G15 = json.load(f)
TRIAL_POINTS = sorted(k for k, e in G15.items() if e['kind'] == 'trials')
BATCH_POINTS = sorted(k for k, e in G15.items() if e['kind'] == 'batch')
E_G15 = 40
# the reference's driver (scamp_model.py): OOK, batch = 1, 100 iterations
DRIVER = dict(Nt=1344, Na=84, Nr=73, Lin=32, Lh=6, alphabet='OOK', iterations=100)


def config_of(name, device='cpu', batch=None, iterations=None):
    from config import Config
    e = G15[name]
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=batch or e['B'], generator_mode=e['mode'],
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


def driver_config(device='cpu', mode='sparc'):
    from config import Config
    s = DRIVER
    return Config(s['Nt'], s['Na'], s['Nr'], s['Lin'], s['Lh'], batch=1, generator_mode=mode,
                  iterations=s['iterations'], alphabet=s['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    """Trial point: dict(W, A, SNR, x[E], sym[E], idx[E], y[E]); batch point: dict(W, A, SNR, x, sym, idx, y).
    CPU tensors."""
    from channel import Channel
    from data import Data
    e = G15[name]
    cfg = config_of(name)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    SNR = cfg.snr(e['EbN0'])
    if e['kind'] == 'batch':
        x, sym, idx = da.generate_message()
        return dict(W=W, A=A, SNR=SNR, x=x, sym=sym, idx=idx, y=A @ x + ch.awgn(SNR))
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E_G15):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(W=W, A=A, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys)


@functools.lru_cache(maxsize=None)
def device_inputs(name, device='cuda'):
    h = host_inputs(name)
    out = dict(h)
    out['W'], out['A'] = h['W'].to(device), h['A'].to(device)
    if G15[name]['kind'] == 'batch':
        out['x'], out['y'] = h['x'].to(device), h['y'].to(device)
    else:
        out['x'] = [t.to(device) for t in h['x']]
        out['y'] = [t.to(device) for t in h['y']]
    return out
