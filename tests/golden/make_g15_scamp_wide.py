#!/usr/bin/env python3
"""Generate g15_scamp_wide.json by RUNNING THE REFERENCE (build container only, on the CPU), like
make_g14_scamp_trials.py: the reference is imported flat from AMP_REFERENCE with bytecode writing
disabled, and only the Loss dicts it produces are committed.

g15: SCAMP at coupling blocks wider than 128 and at Nt that is no power of two (M = Nt/Na is), the
shapes of the reference's driver and published curves (scamp_model.py: Nt=1344, Na=84, Nr=73) at
small Lin.  All points: iterations=20, uniform profile, tail truncation.

* trial points: batch = 1, seed 3, ONE Channel.generate_as_sparc, then E = 40 times
  (Data.generate_message, A @ x + Channel.awgn(SNR), SCAMP.forward) on one detector object; each
  trial's Loss dict (T included) is stored;
* batch points: B = 48, generator_mode='sparc', one forward, its Loss dict.

Tests regenerate the inputs with the build's RNG replica (tests/scamp_wide_inputs.py).

The file is written only if the numpy oracle (oracle.scamp_detect + loss_dict), run on the same
inputs, equals the reference on every counting metric of every trial, and is within 5e-4 of it in
VER and SER at every batch point: the reference alone then meets every bound the tests set.

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g15_scamp_wide.py
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
import scamp as ref_scamp    # noqa: E402

from oracle import OracleConfig, loss_dict, scamp_detect   # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

COUNT_KEYS = ['fer', 'ver', 'verf', 'verm', 'verL', 'ber', 'iber', 'sber', 'ier', 'ser']   # golden_io.COUNT_KEYS
ITER, E, TRIAL_SEED, BATCH = 20, 40, 3, 48
# (alphabet, (Nt, Na, Nr, Lin, Lh), generator_mode, EbN0 dB)
TRIAL_POINTS = [('OOK', (96, 6, 12, 4, 2), 'segmented', 7.0),      # < 128, no power of two, straddles the 64-column tile
                ('8PSK', (168, 84, 73, 3, 2), 'sparc', 9.0),       # M = 2, Nt % 64 != 0, K = 8
                ('QPSK', (192, 12, 24, 3, 2), 'sparc', 5.0),       # a multiple of 64 above 128
                ('QPSK', (480, 30, 57, 2, 2), 'sparc', 5.0),       # a published Nt / Na / Nr family
                ('OOK', (1344, 84, 73, 2, 2), 'segmented', 9.0)]   # the driver's Nt, Na, Nr
# (alphabet, (Nt, Na, Nr, Lin, Lh), seed, EbN0 dB), generator_mode='sparc', B = 48
BATCH_POINTS = [('QPSK', (192, 12, 24, 3, 2), 0, 6.0),
                ('8PSK', (168, 84, 73, 3, 2), 1, 11.0),
                ('OOK', (1344, 84, 73, 2, 2), 0, 11.0)]
BATCH_GUARD = 5e-4


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


def oracle_loss(W, A, y, SNR, x, sym, idx, alph, shape, mode, batch):
    Nt, Na, Nr, Lin, Lh = shape
    oc = OracleConfig(Nt, Na, Nr, Lin=Lin, Lh=Lh, B=batch, alphabet=alph, mode=mode, iterations=ITER)
    c = lambda t: t.numpy().reshape(batch, -1)   # noqa: E731
    o = scamp_detect(W.numpy().reshape(oc.Lout, oc.Lin), A.numpy(), c(y), SNR, oc)
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
        det = ref_scamp.SCAMP(cfg)
        trials, bad, tdiff = [], {}, 0
        for j in range(E):
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            ref = loss_to_json(det(W, A, y, SNR, x, sym, idx).loss)
            trials.append(ref)
            got = oracle_loss(W, A, y, SNR, x, sym, idx, alph, shape, mode, 1)
            d = {k: (float(got[k]), ref[k]) for k in COUNT_KEYS if float(got[k]) != ref[k]}
            if d:
                bad[j] = d
            tdiff += int(got['T']) != int(ref['T'])
        if bad:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} {EbN0} dB: {bad}')
        Ts = sorted(set(int(t['T']) for t in trials))
        name = f'trials_{alph}_Nt{shape[0]}'
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
        ref = loss_to_json(ref_scamp.SCAMP(cfg)(W, A, y, SNR, x, sym, idx).loss)
        got = oracle_loss(W, A, y, SNR, x, sym, idx, alph, shape, 'sparc', BATCH)
        dv, ds = abs(float(got['ver']) - ref['ver']), abs(float(got['ser']) - ref['ser'])
        if dv > BATCH_GUARD or ds > BATCH_GUARD:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} seed {seed} {EbN0} dB: '
                             f'|dVER| {dv} |dSER| {ds}')
        name = f'batch_{alph}_Nt{shape[0]}'
        out[name] = {'kind': 'batch', 'alphabet': alph, 'Nt': shape[0], 'Na': shape[1], 'Nr': shape[2],
                     'Lin': shape[3], 'Lh': shape[4], 'mode': 'sparc', 'EbN0': EbN0, 'seed': seed, 'B': BATCH,
                     'iterations': ITER, 'loss': ref}
        print(name, 'T', ref['T'], 'ver', ref['ver'], 'ser', ref['ser'], '|dVER|', dv, '|dSER|', ds)
    with open(os.path.join(HERE, 'g15_scamp_wide.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
