#!/usr/bin/env python3
"""Generate g16_bamp_wide.json by RUNNING THE REFERENCE (build container only, on the CPU), like
make_g15_scamp_wide.py: the reference is imported flat from AMP_REFERENCE with bytecode writing
disabled, and only the Loss dicts it produces are committed.

g16: BAMP at odd n = Nr * Lout, at N % 4 == 2 and at a partial last column tile (2N no multiple of
the 128-wide tile), the shapes amp_bamp_run refused: the Nt / Na / Nr of the reference's published
BAMP curves (bamp_model.py: Nt=1344, Na=84, Nr=73) at small Lin.  All points: iterations=20, uniform
profile, tail truncation.

* trial points: batch = 1, seed 3, ONE Channel.generate_as_sparc, then E = 40 times
  (Data.generate_message, A @ x + Channel.awgn(SNR), BAMP.forward) on one detector object; each
  trial's Loss dict (T included) is stored;
* batch points: B = 48, generator_mode='sparc', one forward, its Loss dict.

Tests regenerate the inputs with the build's RNG replica (tests/bamp_wide_inputs.py).

The file is written only if the numpy oracle (oracle.bamp_detect + loss_dict), run on the same
inputs, equals the reference on every counting metric of every trial, and equals it in VER and SER
at every batch point: the reference alone then meets every bound the tests set.  (QPSK (12,3,5,2,2)
and BPSK (16,4,6,2,2) are trial points only, and QPSK (24,6,7,2,2) is no point at all: there the
oracle's summation order alone moves decisions away from the reference's.)  Every listed point
passed the guard at the EbN0 and seed given here; none had to be moved.

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g16_bamp_wide.py
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
import bamp as ref_bamp      # noqa: E402

from oracle import OracleConfig, bamp_detect, loss_dict   # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

COUNT_KEYS = ['fer', 'ver', 'verf', 'verm', 'verL', 'ber', 'iber', 'sber', 'ier', 'ser']   # golden_io.COUNT_KEYS
ITER, E, TRIAL_SEED, BATCH = 20, 40, 3, 48
# (alphabet, (Nt, Na, Nr, Lin, Lh), generator_mode, EbN0 dB)
TRIAL_POINTS = [('OOK', (6, 3, 5, 3, 1), 'segmented', 8.0),        # N = 18 (N % 4 = 2), n = 15
                ('QPSK', (12, 3, 5, 2, 2), 'sparc', 10.0),         # n = 15, K = 4
                ('QPSK', (16, 4, 3, 2, 2), 'sparc', 10.0),         # n = 9 (n % 4 = 1)
                ('BPSK', (16, 4, 6, 2, 2), 'sparc', 8.0),          # n = 18 (n % 4 = 2)
                ('OOK', (48, 6, 12, 2, 2), 'segmented', 7.0),      # N = 96: column tiles 128 + 64
                ('8PSK', (168, 84, 73, 3, 2), 'sparc', 9.0),       # M = 2, 2N = 1008: partial last tile of eight
                ('QPSK', (480, 30, 57, 2, 2), 'sparc', 5.0),       # n = 171, a published Nt / Na / Nr family
                ('OOK', (1344, 84, 73, 2, 2), 'segmented', 9.0)]   # the published Nt / Na / Nr, n = 219, 42 tiles
# (alphabet, (Nt, Na, Nr, Lin, Lh), seed, EbN0 dB), generator_mode='sparc', B = 48
BATCH_POINTS = [('OOK', (6, 3, 5, 3, 1), 0, 8.0),
                ('OOK', (48, 6, 12, 2, 2), 1, 8.0),
                ('8PSK', (168, 84, 73, 3, 2), 1, 11.0),
                ('QPSK', (480, 30, 57, 2, 2), 0, 5.0),
                ('OOK', (1344, 84, 73, 2, 2), 0, 11.0)]


def loss_to_json(loss):
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
    return out


def config(alph, shape, mode, batch):
    Nt, Na, Nr, Lin, Lh = shape
    return Config(Nt, Na, Nr, Lin, Lh, batch=batch, generator_mode=mode, iterations=ITER, alphabet=alph,
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


def oracle_loss(A, y, SNR, x, sym, idx, alph, shape, mode, batch):
    Nt, Na, Nr, Lin, Lh = shape
    oc = OracleConfig(Nt, Na, Nr, Lin=Lin, Lh=Lh, B=batch, alphabet=alph, mode=mode, iterations=ITER)
    c = lambda t: t.numpy().reshape(batch, -1)   # noqa: E731
    o = bamp_detect(A.numpy(), c(y), SNR, oc)
    return loss_dict(o['xmap'], o['xmmse'], c(x), sym, idx, o['T'], oc)


def main():
    out = {}
    for alph, shape, mode, EbN0 in TRIAL_POINTS:
        cfg = config(alph, shape, mode, 1)
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(TRIAL_SEED)
        torch.manual_seed(TRIAL_SEED)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        det = ref_bamp.BAMP(cfg)
        trials, bad, tdiff = [], {}, 0
        for j in range(E):
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            ref = loss_to_json(det(A, y, SNR, x, sym, idx).loss)
            trials.append(ref)
            got = oracle_loss(A, y, SNR, x, sym, idx, alph, shape, mode, 1)
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
        print(name, 'distinct T', len(Ts), Ts, 'fer', sum(t['fer'] for t in trials), 'oracle T differs', tdiff)
    for alph, shape, seed, EbN0 in BATCH_POINTS:
        cfg = config(alph, shape, 'sparc', BATCH)
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(seed)
        torch.manual_seed(seed)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        x, sym, idx = da.generate_message()
        y = A @ x + ch.awgn(SNR)
        ref = loss_to_json(ref_bamp.BAMP(cfg)(A, y, SNR, x, sym, idx).loss)
        got = oracle_loss(A, y, SNR, x, sym, idx, alph, shape, 'sparc', BATCH)
        if float(got['ver']) != ref['ver'] or float(got['ser']) != ref['ser']:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} seed {seed} {EbN0} dB: '
                             f"VER {float(got['ver'])} / {ref['ver']} SER {float(got['ser'])} / {ref['ser']}")
        name = f'batch_{alph}_Nt{shape[0]}'
        assert name not in out, name
        out[name] = {'kind': 'batch', 'alphabet': alph, 'Nt': shape[0], 'Na': shape[1], 'Nr': shape[2],
                     'Lin': shape[3], 'Lh': shape[4], 'mode': 'sparc', 'EbN0': EbN0, 'seed': seed, 'B': BATCH,
                     'iterations': ITER, 'loss': ref}
        print(name, 'T', ref['T'], 'ver', ref['ver'], 'ser', ref['ser'])
    with open(os.path.join(HERE, 'g16_bamp_wide.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
