#!/usr/bin/env python3
"""BAMP / SCAMP trial batches over several channels at the reference's published long-sequence
shape (Nt=128 Na=8 Nr=24 Lh=3 Lin=20, OOK, generator_mode='segmented': N = 2560, n = 528), the way
its drivers run it: batch = 1, the channel redrawn every `res` epochs (bamp_model.py:44-67,
scamp_model.py:43-66; res defaults to 1).

Per detector and per R in {1, 10, 100} (trials per channel): the same E = 100 trials, trial e on
channel e // R, once as 100 sequential B = 1 forwards (launch engine, each with its own channel)
and once as ONE forward_trials(..., per_channel=R) call, in the same process, alternating, after a
warm-up of both; `reps` timed windows per path, each a whole pass over the 100 trials that ends in
a device synchronise with the Losses resolved inside the window.  At R = 100 the existing
single-channel call is timed as well (same windows).  The results are compared first (T and every
counter per trial).  Writes one JSON line per (detector, R) to
profiles/trials_channels_bench.jsonl and prints it.
  python tools/trials_channels_bench.py [E] [reps] [EbN0dB] [bamp,scamp] [1,10,100]"""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import amp_native as nat  # noqa: E402
from bamp import BAMP  # noqa: E402
from channel import Channel  # noqa: E402
from config import Config  # noqa: E402
from data import Data  # noqa: E402
from loss import counts_to_vector  # noqa: E402
from scamp import SCAMP  # noqa: E402

SHAPE = dict(Nt=128, Na=8, Nr=24, Lin=20, Lh=3)
DETECTORS = ('bamp', 'scamp')


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 6.0
    legs = sys.argv[4].split(',') if len(sys.argv) > 4 else list(DETECTORS)
    Rs = [int(r) for r in sys.argv[5].split(',')] if len(sys.argv) > 5 else [1, 10, 100]
    if not legs or any(a not in DETECTORS for a in legs):
        raise SystemExit(f'trials_channels_bench: detectors are {DETECTORS}')
    if not torch.cuda.is_available():
        raise SystemExit('trials_channels_bench: no ROCm device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out_path = os.path.join(REPO, 'profiles', 'trials_channels_bench.jsonl')
    lines = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            for ln in f:
                if ln.strip():
                    r = json.loads(ln)
                    lines[(r['detector'], r['per_channel'])] = ln.strip()
    np.random.seed(0)
    torch.manual_seed(0)
    cfg = Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=1,
                 generator_mode='segmented', iterations=20, alphabet='OOK', channel_profile='uniform',
                 channel_truncation='tail', device='cpu')
    ch, da = Channel(cfg), Data(cfg)
    SNR = cfg.snr(EbN0)
    As, xs, syms, idxs, noise = [], [], [], [], []
    for _ in range(E):                                   # a channel, a message and a noise vector per trial
        W, A = ch.generate_as_sparc()
        As.append(A.to(dev))
        x, s, i = da.generate_message()
        xs.append(x.to(dev)); syms.append(torch.as_tensor(np.asarray(s, dtype=np.int64)).to(dev))
        idxs.append(torch.as_tensor(np.asarray(i, dtype=np.int64)).to(dev))
        noise.append(ch.awgn(SNR).to(dev))
    W = W.to(dev)
    cfg.device = 'cuda'
    for algo in [a for a in DETECTORS if a in legs]:
        det = BAMP(cfg) if algo == 'bamp' else SCAMP(cfg, engine=nat.ENGINE_LAUNCHES)
        head = () if algo == 'bamp' else (W,)
        for R in Rs:
            G = -(-E // R)
            chans = torch.stack(As[:G]).contiguous()     # [G, n, N], as a driver would keep them
            ys = [As[e // R] @ xs[e] + noise[e] for e in range(E)]
            rec_of = lambda L: (int(L.loss['T']), counts_to_vector(L.last_counts))   # noqa: E731

            def seq():
                recs = [rec_of(det(*head, As[j // R], ys[j], SNR, xs[j], syms[j], idxs[j])) for j in range(E)]
                torch.cuda.synchronize()
                return recs

            def grouped():
                recs = [rec_of(L) for L in det.forward_trials(*head, chans, ys, SNR, xs, syms, idxs, per_channel=R)]
                torch.cuda.synchronize()
                return recs

            def single():                                # the existing one-channel call (R >= E only)
                recs = [rec_of(L) for L in det.forward_trials(*head, As[0], ys, SNR, xs, syms, idxs)]
                torch.cuda.synchronize()
                return recs

            paths = [('sequential', seq), ('grouped', grouped)] + ([('single_channel', single)] if G == 1 else [])
            first = {k: f() for k, f in paths}           # warm-up of every path, and the comparison
            differ = {k: [j for j in range(E) if first[k][j][0] != first['sequential'][j][0] or
                          not np.array_equal(first[k][j][1], first['sequential'][j][1], equal_nan=True)]
                      for k, _ in paths[1:]}
            for _, f in paths:
                f()
            # windows of comparable length: a grouped pass is repeated until it fills about half a
            # sequential pass (a few-millisecond window would measure the clock and the scheduler)
            t0 = time.perf_counter(); grouped(); one = time.perf_counter() - t0
            t0 = time.perf_counter(); seq(); inner = max(1, int((time.perf_counter() - t0) / one / 2))
            win = {k: [] for k, _ in paths}
            for _ in range(reps):                        # alternated
                for k, f in paths:
                    n_in = 1 if k == 'sequential' else inner
                    t0 = time.perf_counter()
                    for _ in range(n_in):
                        f()
                    win[k].append((time.perf_counter() - t0) / n_in)
            Ts = [r[0] for r in first['grouped']]
            med = {k: statistics.median(v) for k, v in win.items()}
            rec = dict(tool='trials_channels_bench', detector=algo, per_channel=R, channels=G, shape=SHAPE,
                       alphabet='OOK', mode='segmented', E=E, EbN0dB=EbN0, reps=reps, grouped_calls_per_window=inner,
                       T_mean=float(np.mean(Ts)), T_max=int(max(Ts)),
                       trials_differing_from_sequential={k: len(v) for k, v in differ.items()},
                       workspace_bytes=det.trials_workspace_bytes(E, R),
                       ms_per_trial={k: 1e3 * v / E for k, v in med.items()},
                       ms_windows={k: [1e3 * t for t in v] for k, v in win.items()},
                       ratio_sequential_over_grouped=med['sequential'] / med['grouped'],
                       device=torch.cuda.get_device_name(0))
            print(json.dumps(rec), flush=True)
            lines[(algo, R)] = json.dumps(rec)
            del chans, ys
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines[k] for k in sorted(lines)) + '\n')


if __name__ == '__main__':
    main()
