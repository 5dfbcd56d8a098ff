#!/usr/bin/env python3
"""BAMP at the shape of the reference's published BAMP curves (bamp_model.py: Nt=1344 Na=84 Nr=73
Lh=6 Lin=32, OOK, 'segmented', batch = 1, 100 iterations: N = 43008, n = 2701), the way its driver
runs it: one channel, E = 100 epochs at one EbN0.  Modelled on tools/scamp_wide_bench.py.

* ms per trial of ONE forward_trials call against E sequential B = 1 forwards, under
  tools/trials_bench.py's protocol: the results compared first (T and every counter per trial), a
  warm-up of both paths, `reps` alternating windows that end in a device synchronise, medians;
* the prepare's share of a forward: amp_bamp_prepare alone (the four operators packed, their band
  ranges scanned, the state initialised: all of it once per forward) timed against whole forwards,
  both between device synchronises, medians of `reps`;
* Model(config, 'bamp', group_trials=E) over the same E epochs of one channel, end to end (host
  random streams, the per-epoch A @ x on the host): seconds, FER, mean T;
* workspace bytes of both entry points; mean / max T and FER.

Every GPU step is a child process of its own under a time limit; a step that fails ends the run
(nothing further is started on the device).  At most 16 CPU threads.

Writes one JSON line to profiles/bamp_wide_bench.jsonl (or `out`) and prints it.
  python tools/bamp_wide_bench.py [E] [reps] [EbN0dB] [out]"""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

MAX_CPUS = 16
for _v in ('OMP_NUM_THREADS', 'MKL_NUM_THREADS', 'OPENBLAS_NUM_THREADS'):
    try:
        os.environ[_v] = str(max(1, min(MAX_CPUS, int(os.environ.get(_v, MAX_CPUS)))))
    except ValueError:
        os.environ[_v] = str(MAX_CPUS)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(MAX_CPUS, torch.get_num_threads()))

import amp_native as nat  # noqa: E402
from bamp import BAMP, Tracker  # noqa: E402
from channel import Channel  # noqa: E402
from config import Config  # noqa: E402
from data import Data  # noqa: E402
from loss import counts_to_vector  # noqa: E402

SHAPE = dict(Nt=1344, Na=84, Nr=73, Lin=32, Lh=6)
ITERATIONS = 100                 # bamp_model.py:72
MEASURE_LIMIT_S, MODEL_LIMIT_S = 900, 600


def note(*a):
    """Progress on stderr (the result line alone goes to stdout)."""
    print('[bamp_wide_bench]', *a, file=sys.stderr, flush=True)


def config(device='cpu'):
    return Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=1, generator_mode='segmented',
                  iterations=ITERATIONS, alphabet='OOK', channel_profile='uniform', channel_truncation='tail',
                  device=device)


def setup(E, EbN0, dev):
    np.random.seed(0)
    torch.manual_seed(0)
    cfg = config()
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
    return cfg, BAMP(cfg), A.to(dev), SNR, xs, syms, idxs, ys


def measure_child(E, reps, EbN0, out):
    if not torch.cuda.is_available():
        raise SystemExit('bamp_wide_bench: no ROCm device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    cfg, det, A, SNR, xs, syms, idxs, ys = setup(E, EbN0, dev)

    def seq():
        recs = []
        for j in range(E):
            L = det(A, ys[j], SNR, xs[j], syms[j], idxs[j])
            recs.append((int(L.loss['T']), counts_to_vector(L.last_counts), float(L.loss['fer'])))
        torch.cuda.synchronize()
        return recs

    def grouped():
        Ls = det.forward_trials(A, ys, SNR, xs, syms, idxs)
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
    # the prepare alone against whole forwards (trial 0), each between device synchronises
    tp, tf = [], []
    with torch.cuda.device(dev):
        trk = Tracker(A, ys[0], det.E / SNR, cfg, det._bufs, det.gemm)
        for _ in range(reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            trk.prepare()
            torch.cuda.synchronize(); tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            trk._call('amp_bamp_run')
            torch.cuda.synchronize(); tf.append(time.perf_counter() - t0)
    tp, tf = tp[1:], tf[1:]
    Ts = [r[0] for r in b]
    ms, mg = statistics.median(ts), statistics.median(tg)
    mp, mf = statistics.median(tp), statistics.median(tf)
    rec = dict(E=E, EbN0dB=EbN0, reps=reps, grouped_calls_per_window=inner, T_mean=float(np.mean(Ts)), T_max=int(max(Ts)),
               T_distinct=len(set(Ts)), FER=float(np.mean([r[2] for r in b])), trials_differing_from_sequential=len(differ),
               sequential_ms_per_trial=1e3 * ms / E, grouped_ms_per_trial=1e3 * mg / E,
               sequential_ms_windows=[1e3 * t for t in ts], grouped_ms_windows=[1e3 * t for t in tg], ratio=ms / mg,
               prepare_ms=1e3 * mp, forward_ms=1e3 * mf, prepare_share_of_forward=mp / mf,
               device=torch.cuda.get_device_name(0))
    with open(out, 'w') as f:
        json.dump(rec, f)


def model_child(E, EbN0, out):
    """Model(config, 'bamp', group_trials=E): one SNR point of E epochs that share one channel."""
    from model import Model
    if not torch.cuda.is_available():
        raise SystemExit('bamp_wide_bench: no ROCm device')
    with tempfile.TemporaryDirectory() as d:
        m = Model(config('cuda'), 'bamp', path=d, seed=0, group_trials=E)
        t0 = time.perf_counter()
        res = m.simulate(E, start=EbN0, final=EbN0, res=E)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
    with open(out, 'w') as f:
        json.dump(dict(seconds=dt, epochs=E, FER=float(res[0]['fer']), T_mean=float(res[0]['T'])), f)


def step(args, limit):
    """One GPU step: a child process under its own time limit; its JSON result, or a dict(error)."""
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'out.json')
        cmd = ['timeout', '-k', '10', str(limit), sys.executable, os.path.abspath(__file__)] + args + [out]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0 or not os.path.exists(out):
            return dict(error=f'exit {r.returncode}', tail=(r.stdout or '')[-400:])
        with open(out) as f:
            return json.load(f)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--measure-child':
        return measure_child(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), sys.argv[5])
    if len(sys.argv) > 1 and sys.argv[1] == '--model-child':
        return model_child(int(sys.argv[2]), float(sys.argv[3]), sys.argv[4])
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 8.0
    out_path = sys.argv[4] if len(sys.argv) > 4 else os.path.join(REPO, 'profiles', 'bamp_wide_bench.jsonl')
    d = config().dims()
    rec = dict(tool='bamp_wide_bench', shape=SHAPE, alphabet='OOK', mode='segmented', iterations=ITERATIONS,
               workspace_bytes=nat.lib().amp_bamp_workspace_bytes(C.byref(d), ITERATIONS),
               trials_workspace_bytes=nat.lib().amp_bamp_trials_workspace_bytes(C.byref(d), ITERATIONS, E))
    m = step(['--measure-child', str(E), str(reps), str(EbN0)], MEASURE_LIMIT_S)
    if 'error' in m:
        raise SystemExit(f'bamp_wide_bench: the measurement step failed, nothing written: {m}')
    rec.update(m)
    rec['model_group_trials'] = step(['--model-child', str(E), str(EbN0)], MODEL_LIMIT_S)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
