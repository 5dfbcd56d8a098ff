"""Inputs of the VAMP trial-batch tests over several channels.

* g19 (tests/golden/make_g19_vamp_trials_channels.py: the reference's VAMP at batch = 1, the channel
  and its SVD redrawn every res = 5 epochs, 40 epochs) regenerated with the build's host RNG replica
  in the reference's call order: np.random.seed / torch.manual_seed, then per epoch
  Channel.generate_as_sparc + torch.linalg.svd when i % res == 0, Data.generate_message,
  A @ x + Channel.awgn(SNR) (golden_inputs).
* per test point: 40 channels with their torch.linalg.svd, 40 messages and 40 noise vectors drawn
  once from the point's seed + 19; for a given R, trial e uses channel e // R, so
  y_e = A[e // R] x_e + noise_e (point_inputs).  Computed once per point and shared (read-only).

The points, the smallest shapes that reach every tile case (N / n / k; GEMM2 column tile width):
  vamp_OOK_Nt16    g13   64 / 60 / 60   one 128-wide tile, k < N
  vamp_QPSK_Nt32   g13   32 / 64 / 32   128-wide, n > N
  trials_OOK_Nt6   g17   18 / 15 / 15   128-wide, odd k, N % 4 == 2
  trials_BPSK_Nt8  g17    8 / 11 /  8   128-wide, odd n >= N: the pair loader on y from an odd first row
  trials_OOK_Nt48  g17   96 / 36 / 36   128-wide, column tiles 128 + 64 (a partial last tile)
  wide_OOK_Nt256   here 256 / 24 / 24   256-wide (M = Nt / Na = 128 > 64), two column tiles
No g13 or g17 trial point has M > 64, the only case in which vamp_geometry picks the 256-wide tile
(section_bn), so the last point is defined here; it needs no golden: its tests compare with the
sequential launch-engine forwards on the same inputs."""
import functools
import json
import os

import numpy as np
import torch

import golden_io as gio

with open(os.path.join(gio.GOLDEN, 'g19_vamp_trials_channels.json')) as f:
    G19 = json.load(f)
with open(os.path.join(gio.GOLDEN, 'g13_trials.json')) as f:
    _G13 = json.load(f)
with open(os.path.join(gio.GOLDEN, 'g17_vamp_wide.json')) as f:
    _G17 = json.load(f)

E = 40
GOLDEN_POINTS = sorted(G19)
_WIDE = dict(Nt=256, Na=2, Nr=24, Lin=1, Lh=1, alphabet='OOK', mode='segmented', EbN0=6.0, seed=3, iterations=20)
_SRC = {'vamp_OOK_Nt16': _G13['vamp_OOK_Nt16'], 'vamp_QPSK_Nt32': _G13['vamp_QPSK_Nt32'],
        'trials_OOK_Nt6': _G17['trials_OOK_Nt6'], 'trials_BPSK_Nt8': _G17['trials_BPSK_Nt8'],
        'trials_OOK_Nt48': _G17['trials_OOK_Nt48'], 'wide_OOK_Nt256': _WIDE}
POINT_IDS = list(_SRC)


def _entry(name, golden):
    return G19[name] if golden else _SRC[name]


def config_of(name, device='cpu', iterations=None, golden=False, batch=1):
    from config import Config
    e = _entry(name, golden)
    return Config(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], batch=batch, generator_mode=e.get('mode', 'segmented'),
                  iterations=iterations or e['iterations'], alphabet=e['alphabet'], channel_profile='uniform',
                  channel_truncation='tail', device=device)


@functools.lru_cache(maxsize=None)
def golden_inputs(name):
    """g19's epochs: dict(A[E], U[E], s[E], Vh[E] (the epoch's channel and its factors: the same
    objects within a block), SNR, x[E], sym[E], idx[E], y[E], res) on the CPU."""
    from channel import Channel
    from data import Data
    e = G19[name]
    cfg = config_of(name, golden=True)
    np.random.seed(e['seed'])
    torch.manual_seed(e['seed'])
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(e['EbN0'])
    out = dict(A=[], U=[], s=[], Vh=[], x=[], sym=[], idx=[], y=[])
    for i in range(E):
        if i % e['res'] == 0:
            W, A = ch.generate_as_sparc()
            U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        x, sym, idx = da.generate_message()
        y = A @ x + ch.awgn(SNR)
        for k, v in (('A', A), ('U', U), ('s', s), ('Vh', Vh), ('x', x), ('sym', sym), ('idx', idx), ('y', y)):
            out[k].append(v)
    out.update(SNR=SNR, res=e['res'])
    return out


@functools.lru_cache(maxsize=None)
def point_inputs(name):
    """dict(A[E], U[E], s[E], Vh[E] channels and their factors, SNR, x[E], sym[E], idx[E], noise[E])
    on the CPU, drawn once from the point's seed + 19."""
    from channel import Channel
    from data import Data
    e = _entry(name, False)
    cfg = config_of(name)
    np.random.seed(e['seed'] + 19)
    torch.manual_seed(e['seed'] + 19)
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(e['EbN0'])
    out = dict(A=[], U=[], s=[], Vh=[], x=[], sym=[], idx=[], noise=[])
    for _ in range(E):
        W, A = ch.generate_as_sparc()
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        for k, v in (('A', A), ('U', U), ('s', s), ('Vh', Vh)):
            out[k].append(v)
    for _ in range(E):
        x, sym, idx = da.generate_message()
        out['x'].append(x); out['sym'].append(sym); out['idx'].append(idx)
        out['noise'].append(ch.awgn(SNR))
    out['SNR'] = SNR
    return out


@functools.lru_cache(maxsize=None)
def device_point(name, device='cuda'):
    h = point_inputs(name)
    out = dict(h)
    for k in ('A', 'U', 's', 'Vh', 'x', 'noise'):
        out[k] = [t.to(device) for t in h[k]]
    return out


def received(inp, e, g):
    """y of trial e through channel g (same device as the inputs)."""
    return inp['A'][g] @ inp['x'][e] + inp['noise'][e]


def factors(inp, gs):
    """(Us, ss, Vhs) of the channels `gs`, as forward_trials(..., per_channel=R) takes them."""
    return [inp['U'][g] for g in gs], [inp['s'][g] for g in gs], [inp['Vh'][g] for g in gs]
