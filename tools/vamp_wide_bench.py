#!/usr/bin/env python3
"""VAMP at the shape of the reference's published VAMP curve (Simulations/VAMP/OOK,segmented/
uniform,tail/Nt=1344,Na=84,Nr=73,Lh=6,Lin=32; vamp_model.py: batch = 1, 100 iterations: N = 43008,
n = k = 2701), the way its driver runs it: one channel, E = 100 epochs at one EbN0 (the curve's
8 dB).  Modelled on tools/bamp_wide_bench.py.

* ms per trial of ONE forward_trials call of E trials against sequential B = 1 forwards.  A
  sequential forward packs both 1.9 GB operators again, so the sequential side is measured on the
  first `S` trials only (ms per trial is what is compared).  The results are compared first (T and
  every counter of those S trials), both paths are warmed up, then `reps` alternating windows that
  end in a device synchronise; medians;
* the prepare's share of a forward: amp_vamp_prepare alone (the three operators packed, the state
  initialised, y~) timed against whole amp_vamp_run forwards of trial 0, medians of `reps`;
* the per-iteration split between GEMM1 (vamp_k1: 43 column tiles over a reduction of 86016),
  GEMM2 + denoiser (vamp_k2: 672 column tiles over 5402) and the reduction launch, from
  amp_vamp_profile (HIP events around every launch) at B = 1 and at one batch of B = E rows, which
  launches the row and column tiles of the E-trial call;
* workspace bytes of both entry points, and what amp_vamp_workspace_bytes reported while every
  shape also held the persistent engines' operator buffers; mean / max T and FER.

Every GPU step is a child process of its own under a time limit; a step that fails ends the run
(nothing further is started on the device).  At most 16 CPU threads.

Writes one JSON line to profiles/vamp_wide_bench.jsonl (or `out`) and prints it.
  python tools/vamp_wide_bench.py [E] [reps] [EbN0dB] [S] [out]"""
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
from channel import Channel  # noqa: E402
from config import Config  # noqa: E402
from data import Data  # noqa: E402
from loss import counts_to_vector  # noqa: E402
from vamp import VAMP, Tracker  # noqa: E402

SHAPE = dict(Nt=1344, Na=84, Nr=73, Lin=32, Lh=6)
ITERATIONS = 100                 # vamp_model.py
MEASURE_LIMIT_S = 900


def note(*a):
    """Progress on stderr (the result line alone goes to stdout)."""
    print('[vamp_wide_bench]', *a, file=sys.stderr, flush=True)


def config(device='cpu', batch=1, mode='segmented'):
    return Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=batch, generator_mode=mode,
                  iterations=ITERATIONS, alphabet='OOK', channel_profile='uniform', channel_truncation='tail',
                  device=device)


def setup(E, EbN0, dev):
    from model import svd_gram
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
    U, s, Vh = svd_gram(A.to(dev).reshape(A.shape[-2], A.shape[-1]))   # on the device, as Model(rng='device')
    U, s, Vh = U.contiguous(), s.contiguous(), Vh.resolve_conj().contiguous()
    torch.cuda.synchronize()
    note('factors', tuple(U.shape), tuple(Vh.shape))
    return VAMP(config('cuda')), U, s, Vh, SNR, xs, syms, idxs, ys


def profile(det, U, s, Vh, y, SNR, cfg):
    """amp_vamp_profile: ms per executed iteration of vamp_k1, vamp_k2, vamp_r, and the forward."""
    with torch.cuda.device(y.device):
        T = Tracker(U, s, Vh, y, None, det.E / SNR, det.sparsity, cfg)
        T.args.engine, T.args.gemm = nat.ENGINE_LAUNCHES, nat.GEMM_AUTO
        ms = (C.c_float * 4)()
        for _ in range(2):                           # the second call is the measurement
            nat.check(nat.lib().amp_vamp_profile(C.byref(T.dims), C.byref(T.const), C.byref(T.args), ms, T.stream),
                      'amp_vamp_profile')
        st = T.status()
    return dict(gemm1_ms=ms[0], gemm2_denoise_ms=ms[1], reduce_ms=ms[2], forward_ms=ms[3], T=int(st.T))


def measure_child(E, reps, EbN0, S, out):
    if not torch.cuda.is_available():
        raise SystemExit('vamp_wide_bench: no ROCm device (a time is measured on the GPU or not at all)')
    dev = torch.device('cuda:0')
    det, U, s, Vh, SNR, xs, syms, idxs, ys = setup(E, EbN0, dev)
    S = min(S, E)

    def seq():
        recs = []
        for j in range(S):
            L = det(U, s, Vh, ys[j], SNR, xs[j], syms[j], idxs[j])
            recs.append((int(L.loss['T']), counts_to_vector(L.last_counts), float(L.loss['fer'])))
        torch.cuda.synchronize()
        return recs

    def grouped():
        Ls = det.forward_trials(U, s, Vh, ys, SNR, xs, syms, idxs)
        recs = [(int(L.loss['T']), counts_to_vector(L.last_counts), float(L.loss['fer'])) for L in Ls]
        torch.cuda.synchronize()
        return recs

    t0 = time.perf_counter(); a = seq(); note('first sequential pass', round(time.perf_counter() - t0, 2), 's')
    t0 = time.perf_counter(); b = grouped(); note('first grouped call', round(time.perf_counter() - t0, 2), 's')
    # those were the warm-up of both paths; now the comparison
    differ = [j for j in range(S) if a[j][0] != b[j][0] or not np.array_equal(a[j][1], b[j][1], equal_nan=True)]
    ts, tg = [], []
    for _ in range(reps):
        t0 = time.perf_counter(); seq(); ts.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); grouped(); tg.append(time.perf_counter() - t0)
        note('window', len(ts), 'of', reps)
    # the prepare alone against whole forwards (trial 0), each between device synchronises
    tp, tf = [], []
    cfg1 = config('cuda')
    with torch.cuda.device(dev):
        trk = Tracker(U, s, Vh, ys[0], None, det.E / SNR, det.sparsity, cfg1)
        trk.args.engine, trk.args.gemm = nat.ENGINE_LAUNCHES, nat.GEMM_AUTO
        for _ in range(reps + 1):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            trk.prepare()
            torch.cuda.synchronize(); tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            nat.check(nat.lib().amp_vamp_run(C.byref(trk.dims), C.byref(trk.const), C.byref(trk.args), trk.stream),
                      'amp_vamp_run')
            torch.cuda.synchronize(); tf.append(time.perf_counter() - t0)
    tp, tf = tp[1:], tf[1:]
    p1 = profile(det, U, s, Vh, ys[0], SNR, cfg1)
    note('profile B = 1', p1)
    pE = profile(det, U, s, Vh, torch.cat(ys, 0), SNR, config('cuda', batch=E, mode='sparc'))
    note('profile B = E', pE)
    Ts = [r[0] for r in b]
    ms, mg = statistics.median(ts), statistics.median(tg)
    mp, mf = statistics.median(tp), statistics.median(tf)
    rec = dict(E=E, EbN0dB=EbN0, reps=reps, sequential_trials_per_window=S, T_mean=float(np.mean(Ts)), T_max=int(max(Ts)),
               T_distinct=len(set(Ts)), FER=float(np.mean([r[2] for r in b])), trials_differing_from_sequential=len(differ),
               sequential_ms_per_trial=1e3 * ms / S, grouped_ms_per_trial=1e3 * mg / E,
               sequential_ms_windows=[1e3 * t for t in ts], grouped_ms_windows=[1e3 * t for t in tg],
               ratio=(ms / S) / (mg / E), prepare_ms=1e3 * mp, forward_ms=1e3 * mf, prepare_share_of_forward=mp / mf,
               per_iteration_B1=p1, per_iteration_BE=pE, device=torch.cuda.get_device_name(0))
    with open(out, 'w') as f:
        json.dump(rec, f)


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


def persistent_operator_bytes(d, k):
    """Wq0, Wq1, Wq2, Wx1, Wx2 (csrc/amp_vamp.h vamp_carve), each rounded up to the carve's 256 bytes:
    what every shape's workspace also held before they were carved for persistent-eligible shapes only."""
    up = lambda v: (v + 255) // 256 * 256   # noqa: E731
    return sum(up(4 * c) for c in (2 * k * 2 * d.n, 2 * k * 2 * d.N, 2 * d.N * 2 * k, 3 * k * d.N, 3 * k * d.N))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == '--measure-child':
        return measure_child(int(sys.argv[2]), int(sys.argv[3]), float(sys.argv[4]), int(sys.argv[5]), sys.argv[6])
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 8.0
    S = int(sys.argv[4]) if len(sys.argv) > 4 else 4
    out_path = sys.argv[5] if len(sys.argv) > 5 else os.path.join(REPO, 'profiles', 'vamp_wide_bench.jsonl')
    d = config().dims()
    k = min(d.N, d.n)
    wsb = nat.lib().amp_vamp_workspace_bytes(C.byref(d), k, ITERATIONS)
    rec = dict(tool='vamp_wide_bench', shape=SHAPE, alphabet='OOK', mode='segmented', iterations=ITERATIONS,
               workspace_bytes=wsb, workspace_bytes_with_persistent_operators=wsb + persistent_operator_bytes(d, k),
               trials_workspace_bytes=nat.lib().amp_vamp_trials_workspace_bytes(C.byref(d), k, ITERATIONS, E))
    m = step(['--measure-child', str(E), str(reps), str(EbN0), str(S)], MEASURE_LIMIT_S)
    if 'error' in m:
        raise SystemExit(f'vamp_wide_bench: the measurement step failed, nothing written: {m}')
    rec.update(m)
    print(json.dumps(rec))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, 'w') as f:
        f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
