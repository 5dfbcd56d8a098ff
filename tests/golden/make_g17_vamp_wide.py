#!/usr/bin/env python3
"""Generate g17_vamp_wide.json by RUNNING THE REFERENCE (build container only, on the CPU), like
make_g16_bamp_wide.py: the reference is imported flat from AMP_REFERENCE with bytecode writing
disabled, and only the Loss dicts it produces are committed.

g17: VAMP at odd n = Nr * Lout (so odd k = min(n, N) where n < N), at an odd n >= N (k even, only
y has odd rows) and at a partial last column tile (2N no multiple of the 128-wide tile), the shapes
the VAMP launch engines refused: the Nt / Na / Nr of the reference's published VAMP curve
(Simulations/VAMP/OOK,segmented/uniform,tail/Nt=1344,Na=84,Nr=73,Lh=6,Lin=32) at small Lin.  All
points: iterations=20, uniform profile, tail truncation.

* trial points: batch = 1, seed 3, ONE Channel.generate_as_sparc, torch.linalg.svd, then E = 40
  times (Data.generate_message, A @ x + Channel.awgn(SNR), VAMP.forward) on one detector object (the
  reference's driver order, vamp_model.py); each trial's Loss dict (T included) is stored;
* batch points: B = 48, generator_mode='sparc', one forward, its Loss dict.

Tests regenerate the inputs with the build's RNG replica (tests/vamp_wide_inputs.py).

The file is written only if the numpy oracle (oracle.vamp_detect + loss_dict), run on the same
inputs, equals the reference on every counting metric of every trial, and equals it in VER and SER
at every batch point: the reference alone then meets every bound the tests set.  Every listed point
passed the guard at the EbN0 and seed given here; none had to be moved.

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g17_vamp_wide.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('AMP_REFERENCE')
if not REF:
    raise SystemExit('set AMP_REFERENCE to a checkout of AhmedKishki/AMP-SPARC-SpatialModulation')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))   # the oracle package (numpy only)
sys.path.insert(0, REF)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from config import Config    # noqa: E402  (reference module)
from channel import Channel  # noqa: E402
from data import Data        # noqa: E402
import vamp as ref_vamp      # noqa: E402

from oracle import OracleConfig, vamp_detect, loss_dict   # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

COUNT_KEYS = ['fer', 'ver', 'verf', 'verm', 'verL', 'ber', 'iber', 'sber', 'ier', 'ser']   # golden_io.COUNT_KEYS
ITER, E, TRIAL_SEED, BATCH = 20, 40, 3, 48
# (alphabet, (Nt, Na, Nr, Lin, Lh), generator_mode, EbN0 dB)                     N / n / k
TRIAL_POINTS = [('OOK', (6, 3, 5, 3, 1), 'segmented', 8.0),        # 18 / 15 / 15: odd k, N % 4 = 2
                ('QPSK', (16, 4, 3, 2, 2), 'sparc', 10.0),         # 32 / 9 / 9: k % 4 = 1
                ('QPSK', (12, 3, 5, 2, 2), 'sparc', 10.0),         # 24 / 15 / 15: K = 4, ragged T
                ('OOK', (16, 2, 7, 4, 2), 'segmented', 6.0),       # 64 / 35 / 35: k % 4 = 3
                ('BPSK', (8, 2, 11, 1, 1), 'sparc', 6.0),          # 8 / 11 / 8: n odd >= N, the pair loader on y
                ('OOK', (48, 6, 12, 2, 2), 'segmented', 7.0),      # 96 / 36 / 36: column tiles 128 + 64
                ('8PSK', (168, 84, 73, 3, 2), 'sparc', 9.0),       # 504 / 292 / 292: partial last tile of eight
                ('QPSK', (480, 30, 57, 2, 2), 'sparc', 5.0),       # 960 / 171 / 171: a published family, odd k
                ('OOK', (1344, 84, 73, 2, 2), 'segmented', 9.0)]   # 2688 / 219 / 219: the published Nt / Na / Nr
# (alphabet, (Nt, Na, Nr, Lin, Lh), seed, EbN0 dB), generator_mode='sparc', B = 48
BATCH_POINTS = [('OOK', (6, 3, 5, 3, 1), 0, 8.0),
                ('QPSK', (16, 4, 3, 2, 2), 0, 10.0),
                ('OOK', (16, 2, 7, 4, 2), 0, 6.0),
                ('BPSK', (8, 2, 11, 1, 1), 0, 6.0),
                ('OOK', (48, 6, 12, 2, 2), 1, 8.0),
                ('8PSK', (168, 84, 73, 3, 2), 1, 11.0),
                ('QPSK', (480, 30, 57, 2, 2), 0, 5.0),
                ('OOK', (1344, 84, 73, 2, 2), 0, 11.0)]


def loss_to_json(loss):
    """The Loss dict; the four nMSE values (float32 in the reference, compared by no test) at 7
    significant digits, which with the compact separators keeps the file below g16's size."""
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
        if k.startswith('nMSE'):
            out[k] = float('%.7g' % out[k])
    return out


def config(alph, shape, mode, batch):
    Nt, Na, Nr, Lin, Lh = shape
    return Config(Nt, Na, Nr, Lin, Lh, batch=batch, generator_mode=mode, iterations=ITER, alphabet=alph,
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


def oracle_loss(U, s, Vh, y, SNR, x, sym, idx, alph, shape, mode, batch):
    Nt, Na, Nr, Lin, Lh = shape
    oc = OracleConfig(Nt, Na, Nr, Lin=Lin, Lh=Lh, B=batch, alphabet=alph, mode=mode, iterations=ITER)
    c = lambda t: t.numpy().reshape(batch, -1)   # noqa: E731
    o = vamp_detect(U.numpy(), s.numpy(), Vh.numpy(), c(y), SNR, oc)
    return loss_dict(o['r'], o['xmmse'], c(x), sym, idx, o['T'], oc)


def main():
    out = {}
    for alph, shape, mode, EbN0 in TRIAL_POINTS:
        cfg = config(alph, shape, mode, 1)
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(TRIAL_SEED)
        torch.manual_seed(TRIAL_SEED)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        det = ref_vamp.VAMP(cfg)
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        trials, bad, tdiff = [], {}, 0
        for j in range(E):
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            ref = loss_to_json(det(U, s, Vh, y, SNR, x, sym, idx).loss)
            trials.append(ref)
            got = oracle_loss(U, s, Vh, y, SNR, x, sym, idx, alph, shape, mode, 1)
            d = {k: (float(got[k]), ref[k]) for k in COUNT_KEYS if float(got[k]) != ref[k]}
            if d:
                bad[j] = d
            tdiff += int(got['T']) != int(ref['T'])
        if bad:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} {EbN0} dB: {bad}')
        Ts = sorted(set(int(t['T']) for t in trials))
        name = f'trials_{alph}_Nt{shape[0]}'
        assert name not in out, name
        out[name] = {'kind': 'trials', 'alphabet': alph, 'Nt': shape[0], 'Na': shape[1], 'Nr': shape[2],
                     'Lin': shape[3], 'Lh': shape[4], 'mode': mode, 'EbN0': EbN0, 'seed': TRIAL_SEED, 'B': 1,
                     'iterations': ITER, 'oracle_T_differs': tdiff, 'trials': trials}
        print(name, 'distinct T', len(Ts), Ts, 'fer', sum(t['fer'] for t in trials), 'oracle T differs', tdiff,
              flush=True)
    for alph, shape, seed, EbN0 in BATCH_POINTS:
        cfg = config(alph, shape, 'sparc', BATCH)
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(seed)
        torch.manual_seed(seed)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        x, sym, idx = da.generate_message()
        y = A @ x + ch.awgn(SNR)
        ref = loss_to_json(ref_vamp.VAMP(cfg)(U, s, Vh, y, SNR, x, sym, idx).loss)
        got = oracle_loss(U, s, Vh, y, SNR, x, sym, idx, alph, shape, 'sparc', BATCH)
        if float(got['ver']) != ref['ver'] or float(got['ser']) != ref['ser']:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} seed {seed} {EbN0} dB: '
                             f"VER {float(got['ver'])} / {ref['ver']} SER {float(got['ser'])} / {ref['ser']}")
        name = f'batch_{alph}_Nt{shape[0]}'
        assert name not in out, name
        out[name] = {'kind': 'batch', 'alphabet': alph, 'Nt': shape[0], 'Na': shape[1], 'Nr': shape[2],
                     'Lin': shape[3], 'Lh': shape[4], 'mode': 'sparc', 'EbN0': EbN0, 'seed': seed, 'B': BATCH,
                     'iterations': ITER, 'loss': ref}
        print(name, 'T', ref['T'], 'ver', ref['ver'], 'ser', ref['ser'], flush=True)
    with open(os.path.join(HERE, 'g17_vamp_wide.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(',', ':'))


if __name__ == '__main__':
    main()
