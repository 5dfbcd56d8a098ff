#!/usr/bin/env python3
"""Generate g19_vamp_trials_channels.json by RUNNING THE REFERENCE (build container only, on the
CPU), like make_g18_trials_channels.py and make_g17_vamp_wide.py: the reference is imported flat from
AMP_REFERENCE with bytecode writing disabled, and only the Loss dicts it produces are committed.

g19: VAMP the way the reference's driver runs it — batch = 1 and the channel with its SVD redrawn
every `res` epochs (vamp_model.py:45-61) — with res = 5 over 40 epochs, generator_mode='segmented',
iterations=20, uniform profile, tail truncation.  Per point: np.random.seed(3); torch.manual_seed(3),
then for epoch i = 0 .. 39: Channel.generate_as_sparc + torch.linalg.svd when i % 5 == 0,
Data.generate_message, A @ x + Channel.awgn(SNR), VAMP.forward on one detector object.  Each trial's
Loss dict (T included) is stored, the nMSE values at 7 significant digits as in g17; tests regenerate
the inputs with the build's RNG replica in the same order (tests/vamp_trials_channels_inputs.py).

The file is written only if the numpy oracle (oracle.vamp_detect + loss_dict), run on the same
inputs, equals the reference on every counting metric of all 40 trials of each point: the reference
alone then meets the bound the tests set.  `oracle_T_differs` records on how many trials the
oracle's T differs (the reference's T is ragged inside the blocks).  Every listed point passed the
guard at the EbN0 and seed given here; none had to be moved.

Usage: AMP_REFERENCE=/path/to/reference python tests/golden/make_g19_vamp_trials_channels.py
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
ITER, E, RES, SEED = 20, 40, 5, 3
# (alphabet, (Nt, Na, Nr, Lin, Lh), generator_mode, EbN0 dB)                N / n / k
POINTS = [('OOK', (16, 2, 12, 4, 2), 'segmented', 2.0),       # 64 / 60 / 60: the g13 vamp_OOK_Nt16 shape
          ('OOK', (6, 3, 5, 3, 1), 'segmented', 8.0),         # 18 / 15 / 15: odd k, N % 4 == 2
          ('QPSK', (32, 4, 64, 1, 1), 'segmented', 6.0)]      # 32 / 64 / 32: n > N


def loss_to_json(loss):
    """The Loss dict; the four nMSE values (float32 in the reference, compared by no test) at 7
    significant digits."""
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
        if k.startswith('nMSE'):
            out[k] = float('%.7g' % out[k])
    return out


def oracle_loss(U, s, Vh, y, SNR, x, sym, idx, alph, shape, mode):
    Nt, Na, Nr, Lin, Lh = shape
    oc = OracleConfig(Nt, Na, Nr, Lin=Lin, Lh=Lh, B=1, alphabet=alph, mode=mode, iterations=ITER)
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    o = vamp_detect(U.numpy(), s.numpy(), Vh.numpy(), c(y), SNR, oc)
    return loss_dict(o['r'], o['xmmse'], c(x), sym, idx, o['T'], oc)


def main():
    out = {}
    for alph, shape, mode, EbN0 in POINTS:
        Nt, Na, Nr, Lin, Lh = shape
        cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode=mode, iterations=ITER, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        SNR = 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        ch, da = Channel(cfg), Data(cfg)
        det = ref_vamp.VAMP(cfg)
        trials, bad, tdiff = [], {}, 0
        for i in range(E):
            if i % RES == 0:
                W, A = ch.generate_as_sparc()
                U, s, Vh = torch.linalg.svd(A, full_matrices=False)
            x, sym, idx = da.generate_message()
            y = A @ x + ch.awgn(SNR)
            ref = loss_to_json(det(U, s, Vh, y, SNR, x, sym, idx).loss)
            trials.append(ref)
            got = oracle_loss(U, s, Vh, y, SNR, x, sym, idx, alph, shape, mode)
            d = {k: (float(got[k]), ref[k]) for k in COUNT_KEYS if float(got[k]) != ref[k]}
            if d:
                bad[i] = d
            tdiff += int(got['T']) != int(ref['T'])
        if bad:
            raise SystemExit(f'oracle differs from the reference at {alph} {shape} {EbN0} dB: {bad}')
        Ts = sorted(set(int(t['T']) for t in trials))
        name = f'vamp_{alph}_Nt{Nt}'
        assert name not in out, name
        out[name] = {'algo': 'vamp', 'alphabet': alph, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'Lin': Lin, 'Lh': Lh, 'mode': mode,
                     'EbN0': EbN0, 'seed': SEED, 'iterations': ITER, 'res': RES, 'oracle_T_differs': tdiff,
                     'trials': trials}
        print(name, 'distinct T', len(Ts), Ts, 'fer', sum(t['fer'] for t in trials), 'oracle T differs', tdiff,
              flush=True)
    with open(os.path.join(HERE, 'g19_vamp_trials_channels.json'), 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True, separators=(',', ':'))


if __name__ == '__main__':
    main()
