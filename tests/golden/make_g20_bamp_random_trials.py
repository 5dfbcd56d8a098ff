#!/usr/bin/env python3
"""Generate g20_bamp_random_trials.json by RUNNING THE REFERENCE (build container only), like
make_g13_trials.py: the reference is imported flat from AMP_REFERENCE with bytecode writing disabled,
and only the data it produces is committed.

g20: generator_mode='random' the way the reference can run it, batch = 1 (loss.py:262 reshapes to
(Lin, Nt)), many epochs per channel (bamp_model.py:89, 96).  Per point: np.random.seed(3);
torch.manual_seed(3); ONE Channel.generate_as_sparc, then E = 40 times (Data.generate_message =
Data.random, A @ x + Channel.awgn(SNR), BAMP forward) on one detector object.  Only each trial's Loss
dict (T included) is stored; tests regenerate the inputs with the build's RNG replica
(tests/bamp_random_trials_inputs.py).

Each shape is stored at one low and one high EbN0, the first of LOW / HIGH at which the float64
oracle (oracle/, fed the reference's own inputs) differs from the reference in `ver` / `ser` on 0 of
the 40 trials: at B = 1 the allclose exit is decided by rounding, and a point where the oracle's
summation order already flips a trial would not separate the GPU's roundings from the oracle's.
The count is stored beside the trials ('oracle_differs', always 0 for a stored point; the counts of
every candidate tried are printed).

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g20_bamp_random_trials.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('AMP_REFERENCE')
if not REF:
    raise SystemExit('set AMP_REFERENCE to a checkout of AhmedKishki/AMP-SPARC-SpatialModulation')
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # the numpy oracle (package `oracle`)
sys.path.insert(0, REF)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from config import Config    # noqa: E402  (reference module)
from channel import Channel  # noqa: E402
from data import Data        # noqa: E402
import bamp as ref_bamp      # noqa: E402
from oracle import OracleConfig, bamp_detect, loss_dict   # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

SEED, E = 3, 40
# (Nt, Na, Nr, Lin, Lh, alphabet); the last has N = 18 (N % 4 == 2) and n = 15 (odd)
SHAPES = [(16, 2, 7, 2, 3, 'QPSK'), (32, 4, 12, 3, 2, '16QAM'), (6, 3, 5, 3, 1, 'QPSK')]
LOW = [4.0, 2.0, 6.0, 0.0, 3.0, 5.0]
HIGH = [12.0, 14.0, 10.0, 16.0, 18.0, 20.0]


def loss_to_json(loss):
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
    return out


def run_point(shape, EbN0):
    Nt, Na, Nr, Lin, Lh, alph = shape
    cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='random', iterations=20, alphabet=alph,
                 channel_profile='uniform', channel_truncation='tail', device='cpu')
    ocfg = OracleConfig(Nt, Na, Nr, Lin=Lin, Lh=Lh, B=1, alphabet=alph, mode='random', iterations=20)
    SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    det = ref_bamp.BAMP(cfg)
    trials, differs = [], 0
    for _ in range(E):
        x, sym, idx = da.generate_message()
        y = A @ x + ch.awgn(SNR)
        L = det(A, y, SNR, x, sym, idx)
        ref = loss_to_json(L.loss)
        trials.append(ref)
        o = bamp_detect(A.numpy(), y.numpy().reshape(1, -1), SNR, ocfg)
        got = loss_dict(o['xmap'], o['xmmse'], x.numpy().reshape(1, -1), sym, idx, o['T'], ocfg)
        differs += int(float(got['ver']) != ref['ver'] or float(got['ser']) != ref['ser'])
    return trials, differs


def main():
    out = {}
    for shape in SHAPES:
        Nt, Na, Nr, Lin, Lh, alph = shape
        for level, cands in (('low', LOW), ('high', HIGH)):
            for EbN0 in cands:
                trials, differs = run_point(shape, EbN0)
                Ts = sorted(set(int(t['T']) for t in trials))
                print(f'{alph} Nt={Nt} Na={Na} EbN0={EbN0}: oracle differs on {differs} of {E} trials; distinct T {Ts}; '
                      f"fer {sum(t['fer'] for t in trials)}")
                if differs == 0:
                    break
            else:
                raise SystemExit(f'no {level} EbN0 of {cands} at which the oracle agrees on all trials: {shape}')
            name = f'{alph}_Nt{Nt}_Na{Na}_{level}'
            out[name] = {'algo': 'bamp', 'mode': 'random', 'alphabet': alph, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'Lin': Lin,
                         'Lh': Lh, 'EbN0': EbN0, 'seed': SEED, 'iterations': 20, 'oracle_differs': differs,
                         'trials': trials}
    with open(os.path.join(HERE, 'g20_bamp_random_trials.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
