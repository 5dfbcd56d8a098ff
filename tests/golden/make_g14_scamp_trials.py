#!/usr/bin/env python3
"""Generate g14_scamp_trials.json by RUNNING THE REFERENCE (build container only), like make_goldens.py:
the reference is imported flat from AMP_REFERENCE with bytecode writing disabled, and only the
data it produces is committed.

g14: SCAMP the way the reference's driver runs it — batch = 1, many epochs per channel
(scamp_model.py:53-58, 88, 95) in generator_mode='segmented'.  Per point: np.random.seed(3);
torch.manual_seed(3); ONE Channel.generate_as_sparc, then E = 40 times (Data.generate_message,
A @ x + Channel.awgn(SNR), SCAMP.forward) on one detector object.  Only each trial's Loss dict
(T included) is stored; tests regenerate the inputs with the build's RNG replica
(tests/scamp_trials_inputs.py).  A file of its own: trials_inputs.POINTS is every g13 point.

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g14_scamp_trials.py
"""
import json
import os
import sys

sys.dont_write_bytecode = True
REF = os.environ.get('AMP_REFERENCE')
if not REF:
    raise SystemExit('set AMP_REFERENCE to a checkout of AhmedKishki/AMP-SPARC-SpatialModulation')
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from config import Config    # noqa: E402  (reference module)
from channel import Channel  # noqa: E402
from data import Data        # noqa: E402
import scamp as ref_scamp    # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

SEED, E = 3, 40
# (detector, alphabet, (Nt, Na, Nr, Lin, Lh), EbN0 dB); at Nt = 128 a coupling block (2 Nt columns)
# is wider than the A^H column tile: the split-psi path and the block-banded GEMMs
POINTS = [('scamp', 'QPSK', (32, 4, 64, 1, 1), 4.0),
          ('scamp', 'OOK', (16, 2, 12, 4, 2), 4.0),
          ('scamp', 'OOK', (128, 8, 24, 4, 3), 6.0)]


def loss_to_json(loss):
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
    return out


def main():
    out = {}
    for algo, alph, (Nt, Na, Nr, Lin, Lh), EbN0 in POINTS:
        cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='segmented', iterations=20, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        det = ref_scamp.SCAMP(cfg)
        trials = []
        for _ in range(E):
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            L = det(W, A, y, SNR, x, sym, idx)
            trials.append(loss_to_json(L.loss))
        Ts = sorted(set(int(t['T']) for t in trials))
        assert len(Ts) >= 5, (algo, alph, Ts)      # ragged exits: what the per-trial records are for
        name = f'{algo}_{alph}_Nt{Nt}'
        out[name] = {'algo': algo, 'alphabet': alph, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'Lin': Lin, 'Lh': Lh,
                     'EbN0': EbN0, 'seed': SEED, 'iterations': 20, 'trials': trials}
        print(name, 'distinct T', len(Ts), Ts, 'fer', sum(t['fer'] for t in trials))
    with open(os.path.join(HERE, 'g14_scamp_trials.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
