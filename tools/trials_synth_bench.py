#!/usr/bin/env python3
"""Input generation of the trial batches at the reference's published long-sequence shape
(Nt=128 Na=8 Nr=24 Lh=3 Lin=20, OOK, generator_mode='segmented': N = 2560, n = 528), batch = 1,
E = 100 epochs, res in {1, 10, 100} epochs per channel, throughput mode (rng='device').

Two paths on the same build and device, through Model's own generators:
  parent  Model(rng='device', group_trials=E, trial_channels=E): one Channel.generate_as_sparc per
          channel and one Data.generate_message + Channel.awgn + dense A x per trial (Model._inputs);
  synth   the same with synth_trials=True: one amp_synth_channels launch per call's channels and one
          amp_synth_trials launch per call's trials (synth.TrialSynth).
Per res: input generation alone (no detector, no SVD) and VAMP's SVDs alone (svd_gram per channel
against svd_gram on the call's stack); per detector (BAMP, SCAMP, VAMP) and res: end to end (inputs,
SVD for VAMP, forward_trials, Losses resolved) for both paths, and the synth path's detection alone
(its inputs and SVDs drawn beforehand).  Alternating windows after a warm-up of both paths, each
window at least ~50 ms and ended by a device synchronise; medians, every window recorded.
Writes one JSON line per (detector, res) to profiles/trials_synth_bench.jsonl and prints it.
  python tools/trials_synth_bench.py [E] [reps] [EbN0dB] [vamp,bamp,scamp] [res,res,...]"""
import json
import os
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, 'amp-sparc-spatialmodulation_amd')]
import torch  # noqa: E402

import model as model_mod  # noqa: E402
from config import Config  # noqa: E402
from model import Model, svd_gram  # noqa: E402

SHAPE = dict(Nt=128, Na=8, Nr=24, Lin=20, Lh=3)
DETECTORS = ('bamp', 'scamp', 'vamp')


def config():
    return Config(SHAPE['Nt'], SHAPE['Na'], SHAPE['Nr'], SHAPE['Lin'], SHAPE['Lh'], batch=1,
                  generator_mode='segmented', iterations=20, alphabet='OOK', channel_profile='uniform',
                  channel_truncation='tail', device='cuda')


def window(fn, inner):
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / inner


def alternate(fa, fb, reps):
    """Medians and windows (seconds per pass) of two paths measured in alternating windows."""
    inner = []
    for f in (fa, fb):
        f(); f()
        torch.cuda.synchronize()
        inner.append(max(1, int(0.05 / max(window(f, 1), 1e-6))))
    ta, tb = [], []
    for _ in range(reps):
        ta.append(window(fa, inner[0]))
        tb.append(window(fb, inner[1]))
    return statistics.median(ta), statistics.median(tb), ta, tb


def single(f, reps):
    f(); f()
    torch.cuda.synchronize()
    inner = max(1, int(0.05 / max(window(f, 1), 1e-6)))
    t = [window(f, inner) for _ in range(reps)]
    return statistics.median(t), t


class Drawn:
    """TrialSynth's outputs drawn once and handed out again: the synth path's detection alone."""

    def __init__(self, synth):
        self.synth, self.memo = synth, {}

    def channels(self, G, channel0):
        key = ('c', G, channel0)
        if key not in self.memo:
            self.memo[key] = self.synth.channels(G, channel0)
        return self.memo[key]

    def trials(self, At, E, per_channel, SNR, trial0):
        key = ('t', E, per_channel, trial0)
        if key not in self.memo:
            self.memo[key] = self.synth.trials(At, E, per_channel, SNR, trial0)
        return self.memo[key]


def main():
    E = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    EbN0 = float(sys.argv[3]) if len(sys.argv) > 3 else 6.0
    legs = sys.argv[4].split(',') if len(sys.argv) > 4 else list(DETECTORS)
    ress = [int(r) for r in sys.argv[5].split(',')] if len(sys.argv) > 5 else [1, 10, 100]
    if not legs or any(a not in DETECTORS for a in legs):
        raise SystemExit(f'trials_synth_bench: detectors are {DETECTORS}')
    if not torch.cuda.is_available():
        raise SystemExit('trials_synth_bench: no ROCm device (a time is measured on the GPU or not at all)')
    out_path = os.path.join(REPO, 'profiles', 'trials_synth_bench.jsonl')
    lines = {}
    if os.path.exists(out_path):
        with open(out_path) as f:
            for ln in f:
                if ln.strip():
                    r = json.loads(ln)
                    lines[r['detector'], r['res']] = ln.strip()
    tmp = tempfile.mkdtemp()
    ids = list(range(E))
    ms = lambda t: 1e3 * t / E   # noqa: E731
    SNR = config().snr(EbN0)

    def models(algo):
        kw = dict(path=os.path.join(tmp, algo), seed=0, rng='device', group_trials=E, trial_channels=E)
        return Model(config(), algo, **kw), Model(config(), algo, synth_trials=True, **kw)

    for res in ress:
        # input generation alone and the SVDs alone do not depend on the detector
        par, syn = models('bamp')
        G = -(-E // res)

        def gen_parent():
            for i in ids:
                par._inputs(SNR, i % res == 0)

        def gen_synth():
            for e0, n, b0, g in syn._synth_calls(ids, res):
                _, _, At = syn.synth.channels(g, b0)
                syn.synth.trials(At, n, res if g > 1 else n, SNR, e0)

        gp, gs, gpw, gsw = alternate(gen_parent, gen_synth, reps)
        calls = syn._synth_calls(ids, res)
        sp = ss = 0.0
        if 'vamp' in legs:
            stack = syn.synth.channels(G, 0)[1]
            sp, ss, spw, ssw = alternate(lambda: [svd_gram(stack[g]) for g in range(G)],
                                         lambda: svd_gram(stack), reps)
            del stack
        common = dict(tool='trials_synth_bench', shape=SHAPE, alphabet='OOK', mode='segmented', E=E, res=res,
                      channels=G, EbN0dB=EbN0, reps=reps, synth_calls=len(calls),
                      gen_parent_ms_per_trial=ms(gp), gen_synth_ms_per_trial=ms(gs), gen_ratio=gp / gs,
                      gen_parent_ms_windows=[ms(t) for t in gpw], gen_synth_ms_windows=[ms(t) for t in gsw],
                      device=torch.cuda.get_device_name(0))
        for algo in [a for a in DETECTORS if a in legs]:
            par, syn = models(algo)

            def e2e(m, gen):
                for L in gen(SNR, ids, res):
                    L.loss['T']

            ep, es, epw, esw = alternate(lambda: e2e(par, par._group_trial_channels),
                                         lambda: e2e(syn, syn._group_synth), reps)
            # detection alone: the synth path with its inputs (and VAMP's SVDs) drawn beforehand
            real, memo = syn.synth, {}
            syn.synth = Drawn(real)
            keep = model_mod.svd_gram
            model_mod.svd_gram = lambda A: memo[A.data_ptr()] if A.data_ptr() in memo else \
                memo.setdefault(A.data_ptr(), keep(A))
            try:
                det, detw = single(lambda: e2e(syn, syn._group_synth), reps)
            finally:
                model_mod.svd_gram = keep
                syn.synth = real
            own = gs + (ss if algo == 'vamp' else 0.0)
            rec = dict(common, detector=algo,
                       e2e_parent_ms_per_trial=ms(ep), e2e_synth_ms_per_trial=ms(es), e2e_ratio=ep / es,
                       detect_ms_per_trial=ms(det), gen_synth_below_detect=bool(gs < det),
                       gen_share_of_call_parent=(gp + (sp if algo == 'vamp' else 0.0)) / ep,
                       gen_share_of_call_synth=own / es,
                       e2e_parent_ms_windows=[ms(t) for t in epw], e2e_synth_ms_windows=[ms(t) for t in esw],
                       detect_ms_windows=[ms(t) for t in detw])
            if algo == 'vamp':
                rec.update(svd_parent_ms_per_trial=ms(sp), svd_stack_ms_per_trial=ms(ss),
                           svd_parent_ms_windows=[ms(t) for t in spw], svd_stack_ms_windows=[ms(t) for t in ssw])
            print(json.dumps(rec), flush=True)
            lines[algo, res] = json.dumps(rec)
            with open(out_path, 'w') as f:
                f.write('\n'.join(lines[k] for k in sorted(lines)) + '\n')


if __name__ == '__main__':
    main()
