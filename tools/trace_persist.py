#!/usr/bin/env python3
"""Phase timing of the persistent engines (amp_vamp_persist_trace / amp_scamp_persist_trace): per
iteration and workgroup s_memtime stamps -> median cycles per phase, barrier skew across workgroups.

  python tools/trace_persist.py [--config cfg4] [--ebn0 8] [--gemm auto|x3|f32|h2|i8] [--reuse]
--reuse traces a reuse forward (amp_vamp_persist_trace_reuse: the operators and q0 of the forwards
before it stand); iteration 0's phases are printed on their own either way.
  python tools/trace_persist.py --config cfg3        (SCAMP, tools/configs_bench.py's cfg3 inputs)
"""
import argparse
import ctypes as C
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd'))
sys.path.insert(0, REPO)

import numpy as np  # noqa: E402
import torch        # noqa: E402

PHASES = ['r~ build', 'GEMM1', 'w store', 'GEMM2 + r', 'denoiser', 'partial publish', 'partial gather', 'scalars']
STRIDE = 10   # stamps per (workgroup, iteration): amp_vamp_persist.hip AMP_TRACE_STRIDE
SEAM = 24     # AMP_TRACE_SEAM: per (workgroup, iteration) eight arrivals at GEMM1's closing barrier, eight at
              # GEMM2's, eight pack-ahead fallback words (libraries built with AMP_WAVE_TAIL_ARRIVAL=9 only)
DEN = 16      # AMP_TRACE_DEN: behind them, per (workgroup, iteration), every wave's end of the denoiser and the ends of
              # the first four full rounds of waves 0 and 4 (libraries built with AMP_DEN_TRACE=1 only)
# stamp slots in time order.  The exchange's three phases: slot 8 (this wave's denoiser done) -> 5 is the
# partial publish (wave tree, both barriers, thread 0's fold and granule stores: it waits for the SIMD's
# partner wave), 5 -> 6 the gather (sweep, lane fold, tree, LDS broadcast), 6 -> 7 the scalars (the all-NaN
# and danger tests, then vamp_advance or its head)
ORDER = [0, 1, 2, 3, 4, 8, 5, 6, 7]
SPHASES = ['scalars + x planes', 'GEMM1', 's store', 'GEMM2 + xmap', 'denoiser', 'psi + publish',
           'partial gather', 'danger / exit']
SORDER = [0, 1, 2, 3, 4, 5, 6, 7, 8]


def scamp_trace(cfgname, ebn0):
    """cfg3-like SCAMP inputs (tools/configs_bench.py), one traced persistent forward."""
    import amp_native as nat
    from channel import Channel
    from config import Config
    from data import Data
    from scamp import SCAMP
    sys.path.insert(0, os.path.join(REPO, 'tools'))
    import configs_bench
    algo, Nt, Na, Nr, B, alph, iters, e0 = configs_bench.CFGS[cfgname]
    assert algo == 'scamp', cfgname
    cfg = Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=iters, alphabet=alph,
                 channel_profile='uniform', channel_truncation='tail', device='cpu')
    np.random.seed(0)
    torch.manual_seed(0)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    x, _, _ = da.generate_message()
    SNR = cfg.snr(ebn0 if ebn0 is not None else e0)
    y = A @ x + ch.awgn(SNR)
    cfg.device = 'cuda'
    dev = torch.device('cuda', 0)
    W, A, y = (t.to(dev).contiguous() for t in (W, A, y))
    det = SCAMP(cfg, engine=nat.ENGINE_PERSISTENT)
    for _ in range(3):
        det.detect(W, A, y, SNR)
    T = det.detect(W, A, y, SNR)
    nwg = (B + 15) // 16
    tr = torch.zeros(nwg * iters * STRIDE + 2 * nwg, dtype=torch.int64, device=dev)
    nat.check(nat.lib().amp_scamp_persist_trace(C.byref(T.dims), C.byref(T.const), C.byref(T.args), nat.dptr(tr),
                                                T.stream), 'trace')
    torch.cuda.synchronize()
    Tn = int(T.status().T)
    st = tr.cpu().numpy()[:nwg * iters * STRIDE].reshape(nwg, iters, STRIDE).astype(np.int64)[:, :Tn, SORDER]
    d = np.diff(st, axis=2)
    per_it = np.median(st[:, 1:, 0] - st[:, :-1, 0]) if Tn > 1 else 0
    print(f'SCAMP {cfgname}: T={Tn}  nwg={nwg}  median cycles per iteration {per_it:.0f}')
    for i, name in enumerate(SPHASES):
        v = d[:, 1:, i] if Tn > 1 else d[:, :, i]
        print(f'  {name:22s} median {np.median(v):9.0f}  p10 {np.percentile(v, 10):9.0f}  p90 {np.percentile(v, 90):9.0f}'
              f'  ({100 * np.median(v) / per_it:5.1f} %)' if per_it else '')


def main():
    import bench
    import amp_native as nat
    from config import Config
    from vamp import VAMP
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='cfg4')
    ap.add_argument('--ebn0', type=float, default=None)
    ap.add_argument('--gemm', default='auto', choices=['auto', 'x3', 'f32', 'h2', 'i8'])
    ap.add_argument('--reuse', action='store_true',
                    help='trace a reuse forward (the detect calls before it leave the operators and q0)')
    args = ap.parse_args()
    if args.config.startswith('cfg3'):
        return scamp_trace(args.config, args.ebn0)
    if args.ebn0 is None:
        args.ebn0 = 8.0
    Nt, Na, Nr, B, alph, iters = bench.CONFIGS[args.config]
    cfg = Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=iters, alphabet=alph,
                 channel_profile='uniform', channel_truncation='tail', device='cuda')
    dev = torch.device('cuda', 0)
    inp = bench.make_inputs(cfg, 0, args.ebn0, dev)
    gemm = {'auto': nat.GEMM_AUTO, 'x3': nat.GEMM_X3, 'f32': nat.GEMM_F32, 'h2': nat.GEMM_H2,
            'i8': nat.GEMM_I8}[args.gemm]
    det = VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=gemm)
    for _ in range(3):
        det.detect(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'])
    T = det.detect(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'])
    nwg = (B + 15) // 16
    # ten stamps per (workgroup, iteration), 4 nwg start / end clock words, then the gathers' sweep counts
    # (and the seam words of an AMP_WAVE_TAIL_ARRIVAL=9 library, the denoiser words of an AMP_DEN_TRACE=1 one)
    tr = torch.zeros(nwg * iters * STRIDE + 4 * nwg + nwg * iters + nwg * iters * (SEAM + DEN), dtype=torch.int64, device=dev)
    s0, e0 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    b0 = nat.prepare_counts()
    nat.check(nat.lib().amp_vamp_persist_trace_reuse(C.byref(T.dims), C.byref(T.const), C.byref(T.args), nat.dptr(tr),
                                                     1 if args.reuse else 0, T.stream), 'trace')
    b1 = nat.prepare_counts()
    e0.record()
    torch.cuda.synchronize()
    ms = s0.elapsed_time(e0)
    a = tr.cpu().numpy()
    st = a[:nwg * iters * STRIDE].reshape(nwg, iters, STRIDE).astype(np.int64)[:, :, ORDER]
    Tn = int(T.status().T)
    st = st[:, :Tn]
    d = np.diff(st, axis=2)                       # [nwg, T, 8]
    total_cyc = np.median(st[:, -1, -1] - st[:, 0, 0])
    print(f'T={Tn}  nwg={nwg}  kernel+prepare {ms:.3f} ms (events)  median loop cycles {total_cyc:.0f}  '
          f'prepare: {"reuse" if b1[1] > b0[1] else "building"}')
    per_it = np.median(st[:, 1:, 0] - st[:, :-1, 0]) if Tn > 1 else 0
    print(f'median cycles per iteration {per_it:.0f}')
    for i, name in enumerate(PHASES):
        v = d[:, 1:, i] if Tn > 1 else d[:, :, i]
        print(f'  {name:22s} median {np.median(v):9.0f}  p10 {np.percentile(v, 10):9.0f}  p90 {np.percentile(v, 90):9.0f}'
              f'  ({100 * np.median(v) / per_it:5.1f} %)' if per_it else '')
    print('iteration 0 (median cycles): ' + '  '.join(f'{name} {np.median(d[:, 0, i]):.0f}'
                                                       for i, name in enumerate(PHASES[:5])))
    raw = a[:nwg * iters * STRIDE].reshape(nwg, iters, STRIDE).astype(np.int64)[:, 1:Tn]
    if Tn > 1 and np.all(raw[:, :, 9] > 0) and np.all(raw[:, :, 9] < raw[:, :, 6]):
        # vamp_advance in two parts (bf16x3, one workgroup per CU): slot 9 is the end of the tail, inside
        # this iteration's GEMM1 (slot 1 -> slot 2); the scalars phase is the head alone
        print(f'  scalars: head (gather end -> record) median {np.median(raw[:, :, 7] - raw[:, :, 6]):.0f} cycles; '
              f'tail done median {np.median(raw[:, :, 9] - raw[:, :, 1]):.0f} cycles into GEMM1 '
              f'(of {np.median(raw[:, :, 2] - raw[:, :, 1]):.0f})')
    elif Tn > 1 and np.all(raw[:, :, 9] > 0):   # slot 9: the start of vamp_advance (the scalars' own work)
        print(f'  scalars: gather end -> advance start median {np.median(raw[:, :, 9] - raw[:, :, 6]):.0f}, '
              f'vamp_advance median {np.median(raw[:, :, 7] - raw[:, :, 9]):.0f} cycles')
    sweep_counts(a, nwg, iters, Tn)
    seam_arrivals(a, nwg, iters, Tn)
    denoiser_ends(a, nwg, iters, Tn)
    arrival_spread(a, st, nwg, iters, Tn)


def seam_arrivals(a, nwg, iters, Tn):
    """Each wave's arrival at the barrier that closes GEMM1 (cycles behind stamp 1) and at the one that
    closes GEMM2 + r (behind stamp 3), and the waves that did not pack their w ahead of the barrier
    (the flag did not show the iteration yet).  Written by an AMP_WAVE_TAIL_ARRIVAL=9 library only."""
    base = nwg * iters * STRIDE + 4 * nwg + nwg * iters
    sm = a[base:base + nwg * iters * SEAM].reshape(nwg, iters, SEAM).astype(np.int64)[:, 1:Tn]
    raw = a[:nwg * iters * STRIDE].reshape(nwg, iters, STRIDE).astype(np.int64)[:, 1:Tn]
    if sm.size == 0 or not np.all(sm[:, :, :16] > 0):
        print('  seam arrivals: not recorded by this library')
        return
    for name, lo, s0, s1 in (('GEMM1', 0, 1, 2), ('GEMM2 + r', 8, 3, 4)):
        arr = np.median(sm[:, :, lo:lo + 8] - raw[:, :, s0, None], axis=(0, 1))
        # stamp s1 is thread 0's, behind the barrier (GEMM2 + r: behind the argument reload as well)
        print(f'  arrival at the barrier closing {name} (median cycles into the phase, waves 0-7): '
              + ' '.join(f'{v:.0f}' for v in arr) + f'  of {np.median(raw[:, :, s1] - raw[:, :, s0]):.0f}')
    fb = a[base:base + nwg * iters * SEAM].reshape(nwg, iters, SEAM)[:, :Tn, 16:24]
    print(f'  pack-ahead fallbacks: {int(fb.sum())} of {fb.size} (wave, workgroup, iteration); iteration 0: {int(fb[:, 0].sum())}; '
          f'per wave: {[int(v) for v in fb.sum(axis=(0, 1))]}')


def denoiser_ends(a, nwg, iters, Tn):
    """Each wave's end of the denoiser (cycles behind stamp 4), the round times of waves 0 and 4 (the SIMD 0
    pair: the older and the younger wave) and the publish chain alone, from the last wave's end to stamp 5.
    Written by an AMP_DEN_TRACE=1 library only (the kernels with the full-round denoiser step)."""
    base = nwg * iters * STRIDE + 4 * nwg + nwg * iters + nwg * iters * SEAM
    dn = a[base:base + nwg * iters * DEN].reshape(nwg, iters, DEN).astype(np.int64)[:, 1:Tn]
    raw = a[:nwg * iters * STRIDE].reshape(nwg, iters, STRIDE).astype(np.int64)[:, 1:Tn]
    if dn.size == 0 or not np.all(dn[:, :, :8] > 0):
        print('  denoiser ends: not recorded by this library')
        return
    ends = dn[:, :, :8] - raw[:, :, 4, None]
    med = np.median(ends, axis=(0, 1))
    print('  end of the denoiser (median cycles behind stamp 4, waves 0-7): ' + ' '.join(f'{v:.0f}' for v in med)
          + f'  halves: {np.median(ends[:, :, :4]):.0f} | {np.median(ends[:, :, 4:]):.0f}'
          + f'  younger - older per SIMD: {np.median(ends[:, :, 4:] - ends[:, :, :4]):.0f}')
    for w, lo in ((0, 8), (4, 12)):
        full = np.all(dn[:, :, lo:lo + 4] > 0, axis=2)   # workgroups with four full rounds in this wave
        if not full.any():
            continue
        st = np.concatenate([raw[:, :, 4, None], dn[:, :, lo:lo + 4]], axis=2)[full]
        print(f'  wave {w}: rounds (median cycles each) ' + ' '.join(f'{v:.0f}' for v in np.median(np.diff(st, axis=1), axis=0))
              + f'  last round\'s end {np.median(st[:, 4] - st[:, 0]):.0f}')
    last = dn[:, :, :8].max(axis=2)
    print(f'  publish chain alone (last wave\'s end -> stamp 5): median {np.median(raw[:, :, 5] - last):.0f}  '
          f'p10 {np.percentile(raw[:, :, 5] - last, 10):.0f}  p90 {np.percentile(raw[:, :, 5] - last, 90):.0f};  '
          f'last end: median {np.median(last - raw[:, :, 4]):.0f};  denoiser + publish (4 -> 5): median '
          f'{np.median(raw[:, :, 5] - raw[:, :, 4]):.0f}')


def sweep_counts(a, nwg, iters, Tn):
    """Sweeps per gather (the words behind the clock pairs, [wg, t]): written by the eight-wave bf16x3
    kernels only, so all zero from another kernel or an older library."""
    base = nwg * iters * STRIDE + 4 * nwg
    sw = a[base:base + nwg * iters].reshape(nwg, iters)[:, 1:Tn]
    if sw.size == 0 or not np.all(sw > 0):
        print('  gather sweeps: not recorded by this kernel')
        return
    print(f'  gather sweeps (iterations 1 ...): median {np.median(sw):.0f}  p90 {np.percentile(sw, 90):.0f}  '
          f'max {sw.max()}  mean {sw.mean():.2f}')


def arrival_spread(a, st, nwg, iters, Tn):
    """Spread of the workgroups' arrival at the batch exchange (the stamp after the partial publish)
    per iteration, in cycles.  s_memtime counts each XCD's own clock (its own origin), so stamps
    are put on one time base with the per-workgroup (s_memtime, s_memrealtime) pairs taken at
    kernel start and end: rate = d memtime / d realtime (cycles per 10 ns tick), and
    t = realtime_start + (memtime - memtime_start) / rate.  (Raw s_memtime values are never compared
    across workgroups: their origins differ, even within one XCD.)"""
    base = nwg * iters * STRIDE
    m0, r0 = a[base:base + 2 * nwg:2].astype(np.float64), a[base + 1:base + 2 * nwg:2].astype(np.float64)
    m1, r1 = a[base + 2 * nwg:base + 4 * nwg:2].astype(np.float64), a[base + 2 * nwg + 1:base + 4 * nwg:2].astype(np.float64)
    if Tn < 2 or not (np.all(r1 > r0) and np.all(m1 > m0)):
        print('  barrier arrival spread: no valid end stamps (old library?) '
              f'm0 {m0[:3]} m1 {m1[:3]} r0 {r0[:3]} r1 {r1[:3]}')
        return
    rate = (m1 - m0) / (r1 - r0)                          # cycles per realtime tick, per workgroup
    arr = st[:, 1:, 6].astype(np.float64)                 # [nwg, T-1]: publish done
    g = r0[:, None] + (arr - m0[:, None]) / rate[:, None]  # realtime ticks
    cyc = np.median(rate)
    spread = (g.max(0) - g.min(0)) * cyc
    lag = (g - g.min(0)) * cyc                            # [nwg, T-1] cycles behind the first arrival
    late = np.argsort(-lag.mean(1))[:4]
    # per XCD (workgroup wg runs on XCD wg % 8: round-robin dispatch): mean lag and clock
    xl = [float(lag[x::8].mean()) for x in range(8)]
    xc = [float(np.median(rate[x::8]) * 100) for x in range(8)]
    print(f'  clock: {cyc * 100:.0f} MHz median (min {rate.min() * 100:.0f}, max {rate.max() * 100:.0f})')
    print(f'  barrier arrival spread, all workgroups (realtime-aligned, cycles): median {np.median(spread):.0f} '
          f'p10 {np.percentile(spread, 10):.0f} p90 {np.percentile(spread, 90):.0f}')
    print('  mean arrival lag per XCD (cycles): ' + ' '.join(f'{v:.0f}' for v in xl))
    print('  clock per XCD (MHz, median of its workgroups): ' + ' '.join(f'{v:.0f}' for v in xc))
    print(f'  latest workgroups on average: {list(map(int, late))} '
          f'(mean lag {[round(float((g[w] - g.min(0)).mean() * cyc)) for w in late]} cycles)')

if __name__ == '__main__':
    main()
