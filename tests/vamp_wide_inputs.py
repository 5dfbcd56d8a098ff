"""Inputs of the g17 VAMP points (tests/golden/make_g17_vamp_wide.py: odd n, odd k, a partial last
column tile), regenerated with the build's host RNG replica in the reference's call order.
Trial points: np.random.seed / torch.manual_seed, ONE Channel.generate_as_sparc, torch.linalg.svd,
then E x (Data.generate_message, A @ x + Channel.awgn(SNR)) at batch = 1.  Batch points: the same
with one message of B = 48 trials.  Computed once per point and shared (read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g17_vamp_wide.json')) as f:
    G17 = json.load(f)
TRIAL_POINTS = sorted(k for k, e in G17.items() if e['kind'] == 'trials')
BATCH_POINTS = sorted(k for k, e in G17.items() if e['kind'] == 'batch')
E_G17 = 40
# the reference's published VAMP curve (Simulations/VAMP/OOK,segmented/uniform,tail/
# Nt=1344,Na=84,Nr=73,Lh=6,Lin=32; vamp_model.py: batch = 1, 100 iterations)
PUBLISHED = dict(Nt=1344, Na=84, Nr=73, Lin=32, Lh=6, alphabet='OOK', iterations=100)


def config_of(name, device='cpu', batch=None, iterations=None):
    from config import Config
    e = G17[name]
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=batch or e['B'], generator_mode=e['mode'],
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


def published_config(device='cpu', mode='segmented', iterations=None, batch=1):
    from config import Config
    s = PUBLISHED
    return Config(s['Nt'], s['Na'], s['Nr'], s['Lin'], s['Lh'], batch=batch, generator_mode=mode,
                  iterations=iterations or s['iterations'], alphabet=s['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    """Trial point: dict(A, U, s, Vh, SNR, x[E], sym[E], idx[E], y[E]); batch point:
    dict(A, U, s, Vh, SNR, x, sym, idx, y).  CPU tensors."""
    from channel import Channel
    from data import Data
    e = G17[name]
    cfg = config_of(name)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    U, s, Vh = torch.linalg.svd(A, full_matrices=False)
    SNR = cfg.snr(e['EbN0'])
    if e['kind'] == 'batch':
        x, sym, idx = da.generate_message()
        return dict(A=A, U=U, s=s, Vh=Vh, SNR=SNR, x=x, sym=sym, idx=idx, y=A @ x + ch.awgn(SNR))
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E_G17):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(A=A, U=U, s=s, Vh=Vh, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys)


@functools.lru_cache(maxsize=None)
def device_inputs(name, device='cuda'):
    h = host_inputs(name)
    out = dict(h)
    for k in ('A', 'U', 's', 'Vh'):
        out[k] = h[k].to(device)
    if G17[name]['kind'] == 'batch':
        out['x'], out['y'] = h['x'].to(device), h['y'].to(device)
    else:
        out['x'] = [t.to(device) for t in h['x']]
        out['y'] = [t.to(device) for t in h['y']]
    return out
