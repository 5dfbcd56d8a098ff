"""Inputs of the generator_mode='random' trial batches (BAMP(config, random_trials=True)).

* g20 (tests/golden/make_g20_bamp_random_trials.py): per point np.random.seed / torch.manual_seed,
  ONE Channel.generate_as_sparc, then 40 x (Data.generate_message = Data.random,
  A @ x + Channel.awgn(SNR)), regenerated with the build's host RNG replica in the reference's call
  order.
* the shapes of the GPU bit-equality tests: per shape 33 channels, 33 messages and 33 noise vectors
  drawn once from a seed; for a given per_channel R, trial e uses channel e // R.

Computed once per point and shared (read-only) by the tests."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g20_bamp_random_trials.json')) as f:
    G20 = json.load(f)
POINTS = sorted(G20)
E_G20 = 40

# (Nt, Na, Nr, Lin, Lh, alphabet, EbN0): N = 96, n = 48, one partial column tile | 2N = 640, several
# column tiles (several partial slots per row) | N = 18 (N % 4 == 2), n = 15 (odd)
SHAPES = {'16QAM_Nt32': (32, 4, 12, 3, 2, '16QAM', 12.0),
          'QPSK_Nt64': (64, 4, 16, 5, 2, 'QPSK', 8.0),
          'QPSK_Nt6': (6, 3, 5, 3, 1, 'QPSK', 12.0)}
E = 33


def make_config(Nt, Na, Nr, Lin, Lh, alphabet, device='cpu', iterations=20, batch=1, mode='random'):
    from config import Config
    return Config(Nt, Na, Nr, Lin, Lh, batch=batch, generator_mode=mode, iterations=iterations, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', device=device)


def golden_config(name, device='cpu'):
    e = G20[name]
    return make_config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], e['alphabet'], device, e['iterations'])


def shape_config(name, device='cpu', iterations=20):
    return make_config(*SHAPES[name][:6], device=device, iterations=iterations)


@functools.lru_cache(maxsize=None)
def golden_inputs(name):
    """dict(A, SNR, x[E], sym[E], idx[E], y[E]) on the CPU, the reference's draws of the g20 point."""
    from channel import Channel
    from data import Data
    e = G20[name]
    cfg = golden_config(name)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    _, A = ch.generate_as_sparc()
    SNR = cfg.snr(e['EbN0'])
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E_G20):
        x, sym, idx = da.generate_message()
        xs.append(x); syms.append(sym); idxs.append(idx)
        ys.append(A @ x + ch.awgn(SNR))
    return dict(A=A, SNR=SNR, x=xs, sym=syms, idx=idxs, y=ys)


@functools.lru_cache(maxsize=None)
def shape_point(name, device='cuda'):
    """dict(A[E], SNR, x[E], sym[E], idx[E], noise[E]) on `device`: E channels, messages and noise vectors."""
    from channel import Channel
    from data import Data
    cfg = shape_config(name)
    np.random.seed(20)
    torch.manual_seed(20)
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(SHAPES[name][6])
    As, xs, syms, idxs, ns = [], [], [], [], []
    for _ in range(E):
        As.append(ch.generate_as_sparc()[1].to(device))
        x, sym, idx = da.generate_message()
        xs.append(x.to(device)); syms.append(sym); idxs.append(idx)
        ns.append(ch.awgn(SNR).to(device))
    return dict(A=As, SNR=SNR, x=xs, sym=syms, idx=idxs, noise=ns)


def received(inp, e, g):
    """y of trial e through channel g: A_g x_e + noise_e ([1, n, 1])."""
    return inp['A'][g] @ inp['x'][e] + inp['noise'][e]
