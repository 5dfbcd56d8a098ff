#!/usr/bin/env python3
"""Independent-trial batches at the reference's published long-sequence shape
(Nt=128 Na=8 Nr=24 Lh=3 Lin=20, OOK, generator_mode='segmented': N = 2560, n = 528), the way its
drivers run it: batch = 1, E = 100 epochs per channel (vamp_model.py:91, 98; bamp_model.py:89, 96;
scamp_model.py:88, 95).

Per detector (VAMP, BAMP, SCAMP): the same 100 trials, one channel, once as 100 sequential B = 1
forwards (launch engine) and once as ONE forward_trials call, on the same build and device,
alternating, after a warm-up of both; there are `reps` timed windows per path, each a whole pass
over the 100 trials (the grouped path: as many calls as fill half a sequential pass) that ends in
a device synchronise (the Losses are resolved inside the window: the host
needs them per epoch).  The results are compared first (T and every counter per trial).
Writes one JSON line per detector to profiles/trials_bench.jsonl and prints it; with a list of
detectors (e.g. `scamp`) only those legs run and the other detectors' recorded lines are kept.
  python tools/trials_bench.py [E] [reps] [EbN0dB] [vamp,bamp,scamp]"""
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
from vamp import VAMP  # noqa: E402

SHAPE = dict(Nt=128, Na=8, Nr=24, Lin=20, Lh=3)
DETECTORS = ('vamp', 'bamp', 'scamp')


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 6.0
    legs = sys.argv[4].split(',') if len(sys.argv) > 4 else list(DETECTORS)
    if not legs or any(a not in DETECTORS for a in legs):
        raise SystemExit(f'trials_bench: detectors are {DETECTORS}')
    if not torch.cuda.is_available():
        raise SystemExit('trials_bench: no ROCm device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    out_path = os.path.join(REPO, 'profiles', 'trials_bench.jsonl')
    lines = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            lines = {json.loads(ln)['detector']: ln.strip() for ln in f if ln.strip()}
    for algo in [a for a in DETECTORS if a in legs]:
        np.random.seed(0)
        torch.manual_seed(0)
        cfg = Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=1,
                     generator_mode='segmented', iterations=20, alphabet='OOK', channel_profile='uniform',
                     channel_truncation='tail', device='cpu')
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        SNR = cfg.snr(EbN0)
        xs, syms, idxs, ys = [], [], [], []
        for _ in range(E):
            x, s, i = da.generate_message()
            xs.append(x.to(dev)); syms.append(torch.as_tensor(np.asarray(s, dtype=np.int64)).to(dev))
            idxs.append(torch.as_tensor(np.asarray(i, dtype=np.int64)).to(dev))
            ys.append((A @ x + ch.awgn(SNR)).to(dev))
        cfg.device = 'cuda'
        if algo == 'vamp':
            U, sv, Vh = torch.linalg.svd(A, full_matrices=False)
            chan = (U.to(dev), sv.to(dev), Vh.to(dev))
            det = VAMP(cfg, engine=nat.ENGINE_LAUNCHES)
        elif algo == 'bamp':
            chan = (A.to(dev),)
            det = BAMP(cfg)
        else:
            chan = (W.to(dev), A.to(dev))
            det = SCAMP(cfg, engine=nat.ENGINE_LAUNCHES)

        def seq():
            recs = []
            for j in range(E):
                L = det(*chan, ys[j], SNR, xs[j], syms[j], idxs[j])
                recs.append((int(L.loss['T']), counts_to_vector(L.last_counts)))
            torch.cuda.synchronize()
            return recs

        def grouped():
            Ls = det.forward_trials(*chan, ys, SNR, xs, syms, idxs)
            recs = [(int(L.loss['T']), counts_to_vector(L.last_counts)) for L in Ls]
            torch.cuda.synchronize()
            return recs

        a, b = seq(), grouped()          # warm-up of both paths, and the comparison
        differ = [j for j in range(E) if a[j][0] != b[j][0] or not np.array_equal(a[j][1], b[j][1], equal_nan=True)]
        seq(); grouped()
        ts, tg = [], []
        # alternating windows of comparable length: one sequential pass over the E trials, and as
        # many grouped calls as fill about the same time (a few-millisecond window would measure
        # the clock and the scheduler)
        t0 = time.perf_counter(); grouped(); one = time.perf_counter() - t0
        t0 = time.perf_counter(); seq(); inner = max(1, int((time.perf_counter() - t0) / one / 2))
        for _ in range(reps):
            t0 = time.perf_counter(); seq(); ts.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            for _ in range(inner):
                grouped()
            tg.append((time.perf_counter() - t0) / inner)
        Ts = [r[0] for r in b]
        ms, mg = statistics.median(ts), statistics.median(tg)
        rec = dict(tool='trials_bench', detector=algo, shape=SHAPE, alphabet='OOK', mode='segmented', E=E,
                   EbN0dB=EbN0, reps=reps, grouped_calls_per_window=inner, T_mean=float(np.mean(Ts)),
                   T_max=int(max(Ts)), T_distinct=len(set(Ts)),
                   trials_differing_from_sequential=len(differ),
                   sequential_ms_per_trial=1e3 * ms / E, grouped_ms_per_trial=1e3 * mg / E,
                   sequential_ms_windows=[1e3 * t for t in ts], grouped_ms_windows=[1e3 * t for t in tg],
                   ratio=ms / mg, ideal_ratio=E * float(np.mean(Ts)) / max(Ts),
                   device=torch.cuda.get_device_name(0))
        print(json.dumps(rec))
        lines[algo] = json.dumps(rec)
    with open(out_path, 'w') as f:
        f.write('\n'.join(lines[a] for a in DETECTORS if a in lines) + '\n')


if __name__ == '__main__':
    main()
