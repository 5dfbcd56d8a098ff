"""Inputs of the g13 independent-trial points (tests/golden/make_g13_trials.py), regenerated with
the build's host RNG replica in the reference's call order: np.random.seed / torch.manual_seed,
ONE Channel.generate_as_sparc (+ torch.linalg.svd for VAMP), then E x (Data.generate_message,
A @ x + Channel.awgn(SNR)).  Computed once per point and shared (read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g13_trials.json')) as f:
    G13 = json.load(f)
POINTS = sorted(G13)
E_G13 = 40


def config_of(name, device='cpu', iterations=None, mode='segmented'):
    from config import Config
    e = G13[name]
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=1, generator_mode=mode,
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def host_inputs(name):
    """dict(A, U, s, Vh, SNR, x[E], sym[E], idx[E], y[E]) on the CPU (U / s / Vh: VAMP points)."""
    from channel import Channel
    from data import Data
    e = G13[name]
    cfg = config_of(name)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    U = s = Vh = None
    if e['algo'] == 'vamp':
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
    SNR = cfg.snr(e['EbN0'])
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E_G13):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(A=A, U=U, s=s, Vh=Vh, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys)


@functools.lru_cache(maxsize=None)
def device_inputs(name, device='cuda'):
    h = host_inputs(name)
    mv = lambda t: t.to(device) if t is not None else None   # noqa: E731
    out = dict(h)
    for k in ('A', 'U', 's', 'Vh'):
        out[k] = mv(h[k])
    out['x'] = [mv(t) for t in h['x']]
    out['y'] = [mv(t) for t in h['y']]
    return out
