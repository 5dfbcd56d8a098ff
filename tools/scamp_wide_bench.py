#!/usr/bin/env python3
"""SCAMP at the shape the reference's own driver names (scamp_model.py: Nt=1344 Na=84 Nr=73 Lh=6
Lin=32, OOK, batch = 1, 100 iterations: N = 43008, n = 2701), the way it runs it: one channel,
E = 100 epochs at one EbN0.

* ms per trial of ONE forward_trials call against E sequential B = 1 forwards (launch engine), under
  tools/trials_bench.py's protocol: the results compared first (T and every counter per trial), a
  warm-up of both paths, `reps` alternating windows that end in a device synchronise, medians;
* the cost of a forward's prepare (build_cweight + weight_kband: both operators are packed and
  scanned on every forward) against its per-iteration kernels, from a rocprofv3 --kernel-trace
  --stats run of its own over `prof_trials` sequential forwards (a child process; skipped with
  prof_trials = 0 or where rocprofv3 is missing);
* workspace bytes of both entry points; mean / max T and FER.

Writes one JSON line to profiles/scamp_wide_bench.jsonl (or `out`) and prints it.
  python tools/scamp_wide_bench.py [E] [reps] [EbN0dB] [prof_trials] [out]"""
import csv
import ctypes as C
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import amp_native as nat  # noqa: E402
from channel import Channel  # noqa: E402
from config import Config  # noqa: E402
from data import Data  # noqa: E402
from loss import counts_to_vector  # noqa: E402
from scamp import SCAMP  # noqa: E402

SHAPE = dict(Nt=1344, Na=84, Nr=73, Lin=32, Lh=6)
ITERATIONS = 100
PREPARE = ('build_cweight', 'weight_kband', 'scamp_init')        # kernels of one forward's prepare


def note(*a):
    """Progress on stderr (the result line alone goes to stdout)."""
    print('[scamp_wide_bench]', *a, file=sys.stderr, flush=True)


def setup(E, EbN0, dev):
    np.random.seed(0)
    torch.manual_seed(0)
    cfg = Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=1, generator_mode='sparc',
                 iterations=ITERATIONS, alphabet='OOK', channel_profile='uniform', channel_truncation='tail',
                 device='cpu')
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    note('channel', tuple(A.shape))
    SNR = cfg.snr(EbN0)
    xs, syms, idxs, ys = [], [], [], []
    for _ in range(E):
        x, s, i = da.generate_message()
        xs.append(x.to(dev)); syms.append(torch.as_tensor(np.asarray(s, dtype=np.int64)).to(dev))
        idxs.append(torch.as_tensor(np.asarray(i, dtype=np.int64)).to(dev))
        ys.append((A @ x + ch.awgn(SNR)).to(dev))
    note(E, 'trials drawn')
    cfg.device = 'cuda'
    det = SCAMP(cfg, engine=nat.ENGINE_LAUNCHES)
    return cfg, det, (W.to(dev), A.to(dev)), SNR, xs, syms, idxs, ys


def profile_child(trials, EbN0):
    """`trials` sequential forwards and nothing else (the profiled process)."""
    dev = torch.device('cuda:0')
    _, det, chan, SNR, xs, syms, idxs, ys = setup(trials, EbN0, dev)
    for j in range(trials):
        L = det(*chan, ys[j], SNR, xs[j], syms[j], idxs[j])
        int(L.loss['T'])
    torch.cuda.synchronize()


def profile(trials, EbN0):
    """Per forward: microseconds in the prepare kernels and in everything else, from the stats of
    a kernel trace of `trials` sequential forwards; None without rocprofv3."""
    exe = shutil.which('rocprofv3')
    if not exe or trials <= 0:
        return None
    with tempfile.TemporaryDirectory() as d:
        cmd = [exe, '--kernel-trace', '--stats', '-d', d, '-o', 'wide', '--output-format', 'csv', '--',
               sys.executable, os.path.abspath(__file__), '--profile-child', str(trials), str(EbN0)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        files = glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True)
        if r.returncode != 0 or not files:
            return dict(error=(r.stderr or r.stdout)[-400:])
        rows = list(csv.DictReader(open(files[0])))
    kern = {}
    for row in rows:
        name = row['Name'].split('(')[0].replace('void ', '').replace('amp::', '')
        kern[name] = kern.get(name, 0.0) + float(row['TotalDurationNs']) / 1e3 / trials
    prep = sum(v for k, v in kern.items() if k.startswith(PREPARE))
    ours = sum(v for k, v in kern.items() if k.startswith(('scamp_', 'build_cweight', 'weight_kband')))
    top = dict(sorted(kern.items(), key=lambda kv: -kv[1])[:8])
    return dict(trials=trials, prepare_us_per_forward=prep, iteration_us_per_forward=ours - prep,
                all_kernels_us_per_forward=sum(kern.values()), top_kernels_us_per_forward=top)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--profile-child':
        return profile_child(int(sys.argv[2]), float(sys.argv[3]))
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 8.0
    prof_trials = int(sys.argv[4]) if len(sys.argv) > 4 else 5
    out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(REPO, 'profiles', 'scamp_wide_bench.jsonl')
    if not torch.cuda.is_available():
        raise SystemExit('scamp_wide_bench: no ROCm device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    cfg, det, chan, SNR, xs, syms, idxs, ys = setup(E, EbN0, dev)
    d = cfg.dims()
    ws_run = nat.lib().amp_scamp_workspace_bytes(C.byref(d), ITERATIONS)
    ws_trials = nat.lib().amp_scamp_trials_workspace_bytes(C.byref(d), ITERATIONS, E)

    def seq():
        recs = []
        for j in range(E):
            L = det(*chan, ys[j], SNR, xs[j], syms[j], idxs[j])
            recs.append((int(L.loss['T']), counts_to_vector(L.last_counts), float(L.loss['fer'])))
        torch.cuda.synchronize()
        return recs

    def grouped():
        Ls = det.forward_trials(*chan, ys, SNR, xs, syms, idxs)
        recs = [(int(L.loss['T']), counts_to_vector(L.last_counts), float(L.loss['fer'])) for L in Ls]
        torch.cuda.synchronize()
        return recs

    t0 = time.perf_counter(); a = seq(); note('first sequential pass', round(time.perf_counter() - t0, 2), 's')
    t0 = time.perf_counter(); b = grouped(); note('first grouped call', round(time.perf_counter() - t0, 2), 's')
    # those were the warm-up of both paths; now the comparison
    differ = [j for j in range(E) if a[j][0] != b[j][0] or not np.array_equal(a[j][1], b[j][1], equal_nan=True)]
    seq(); grouped()
    ts, tg = [], []
    t0 = time.perf_counter(); grouped(); one = time.perf_counter() - t0
    t0 = time.perf_counter(); seq(); inner = max(1, int((time.perf_counter() - t0) / one / 2))
    for _ in range(reps):
        t0 = time.perf_counter(); seq(); ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        for _ in range(inner):
            grouped()
        tg.append((time.perf_counter() - t0) / inner)
        note('window', len(ts), 'of', reps)
    Ts = [r[0] for r in b]
    ms, mg = statistics.median(ts), statistics.median(tg)
    del det, chan, xs, ys
    torch.cuda.empty_cache()         # the profiled child allocates the same operators
    rec = dict(tool='scamp_wide_bench', shape=SHAPE, alphabet='OOK', mode='sparc', iterations=ITERATIONS, E=E,
               EbN0dB=EbN0, reps=reps, grouped_calls_per_window=inner, T_mean=float(np.mean(Ts)), T_max=int(max(Ts)),
               T_distinct=len(set(Ts)), FER=float(np.mean([r[2] for r in b])),
               trials_differing_from_sequential=len(differ),
               sequential_ms_per_trial=1e3 * ms / E, grouped_ms_per_trial=1e3 * mg / E,
               sequential_ms_windows=[1e3 * t for t in ts], grouped_ms_windows=[1e3 * t for t in tg], ratio=ms / mg,
               workspace_bytes=ws_run, trials_workspace_bytes=ws_trials, profile=profile(prof_trials, EbN0),
               device=torch.cuda.get_device_name(0))
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
