#!/usr/bin/env python3
"""Generate g18_trials_channels.json by RUNNING THE REFERENCE (build container only), like
make_goldens.py: the reference is imported flat from AMP_REFERENCE with bytecode writing disabled,
and only the data it produces is committed.

g18: BAMP and SCAMP the way the reference's drivers run them — batch = 1 and the channel redrawn
every `res` epochs (bamp_model.py:44-67, scamp_model.py:43-66) — with res = 5 over 40 epochs, in
generator_mode='segmented', at the g13 `bamp_OOK_Nt16` shape and the g14 `scamp_OOK_Nt16` shape.
Per point: np.random.seed / torch.manual_seed, then for epoch i = 0 .. 39: Channel.generate_as_sparc
when i % 5 == 0, Data.generate_message, A @ x + Channel.awgn(SNR), the detector's forward on one
detector object.  Only each trial's Loss dict (T included) is stored; tests regenerate the inputs
with the build's RNG replica in the same order (tests/trials_channels_inputs.py).

Seed and EbN0 are chosen so that the numpy oracle, fed by that replica, reproduces every counting
metric of all 40 trials of each point (tests/test_trials_channels_cpu.py).

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g18_trials_channels.py
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
import bamp as ref_bamp      # noqa: E402
import scamp as ref_scamp    # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))

E, RES = 40, 5
# (detector, alphabet, (Nt, Na, Nr, Lin, Lh), EbN0 dB, seed)
POINTS = [('bamp', 'OOK', (16, 2, 12, 4, 2), 6.0, int(os.environ.get('G18_SEED_BAMP', '3'))),
          ('scamp', 'OOK', (16, 2, 12, 4, 2), 4.0, int(os.environ.get('G18_SEED_SCAMP', '3')))]


def loss_to_json(loss):
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
    return out


def main():
    out = {}
    for algo, alph, (Nt, Na, Nr, Lin, Lh), EbN0, seed in POINTS:
        cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='segmented', iterations=20, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(seed)
        torch.manual_seed(seed)
        ch, da = Channel(cfg), Data(cfg)
        det = ref_bamp.BAMP(cfg) if algo == 'bamp' else ref_scamp.SCAMP(cfg)
        trials = []
        for i in range(E):
            if i % RES == 0:
                W, A = ch.generate_as_sparc()
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            L = det(A, y, SNR, x, sym, idx) if algo == 'bamp' else det(W, A, y, SNR, x, sym, idx)
            trials.append(loss_to_json(L.loss))
        Ts = sorted(set(int(t['T']) for t in trials))
        name = f'{algo}_{alph}_Nt{Nt}'
        out[name] = {'algo': algo, 'alphabet': alph, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'Lin': Lin, 'Lh': Lh,
                     'EbN0': EbN0, 'seed': seed, 'iterations': 20, 'res': RES, 'trials': trials}
        print(name, 'distinct T', len(Ts), Ts, 'fer', sum(t['fer'] for t in trials))
    with open(os.path.join(HERE, 'g18_trials_channels.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == '__main__':
    main()
