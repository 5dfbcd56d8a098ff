#!/usr/bin/env python3
"""Generate golden vectors by RUNNING THE REFERENCE (build container only).

The reference (AhmedKishki/AMP-SPARC-SpatialModulation, mounted read-only at
/root/reference) is imported flat, exactly as its own drivers import it, with
bytecode writing disabled so nothing is written under /root/reference.  Only
the data it produces is committed (``*.npz`` / ``*.json`` next to this file);
no reference source travels.

Seeding protocol (the reference never seeds): for every
(config, seed S, EbN0) point, ``np.random.seed(S); torch.manual_seed(S)`` and
then the reference's own per-epoch call order (vamp_model.py:55-61):
``Channel.generate_as_sparc`` -> ``torch.linalg.svd`` (VAMP only) ->
``Data.generate_message`` -> ``A @ x + Channel.awgn(SNR)`` -> detector.

Groups:
  g1  per-iteration traces at small shapes, inputs stored (VAMP, BAMP, SCAMP)
  g2  denoiser unit vectors (scalar tau, per-element tau, SCAMP mean-only, NaN onset)
  g3  MAP decision + all 14 metrics on crafted inputs (ties, 16QAM duplicate, NaN rows)
  g5  Shrink element-wise denoisers (bayes, shrinkOOK, sw_shrinkOOK) on random inputs,
      scalar and per-element cov, real and complex configs, overflow / NaN regimes
  g6  BASELINE cfg5 shape (BAMP Nt=512 Nr=1024 Na=16) on the build-defined Kronecker
      exponentially-correlated channel (rho = 0.5, injected into the reference's BAMP, which
      takes any H), 16-QAM and QPSK twins of cfg5's 64-QAM (which Config rejects), B = 1024
  g7  generator_mode='segmented' (B = 1): Loss.segmented_decision on crafted inputs (ties,
      zero rows, the 16-QAM duplicate point) and VAMP / BAMP Loss dicts along EbN0
  g8  generator_mode='random' (B = 1): Loss.random_decision on crafted inputs and BAMP Loss
      dicts along EbN0 (the reference's random-mode VAMP raises; recorded)
  g9  BAMPLayer.random_denoiser (bamp.py:79-88) unit vectors (per-element cov, underflow regimes)
  g4  Loss dicts along EbN0 for the BASELINE configs + QPSK twins (inputs regenerated
      by the build's RNG replica; SHA-256 of the first (A, x) pins the replica)
  g10 the reference's own Model.simulate drivers (vamp/bamp/scamp_model.py) end to end: every
      {EbN0}.json they write, seeded once before the Model is built
  g11 ISI / spatial coupling (Lin > 1, Lh > 1, tail) Loss dicts for VAMP, BAMP and SCAMP
  g12 vamp2.py damped VAMP: per-iteration traces and Loss dicts (sparc mode)

Usage: python tests/golden/make_goldens.py [g1 g2 g3 g4 g4p g4pp ...]
"""
import hashlib
import json
import os
import sys
import time

sys.dont_write_bytecode = True
REF = os.environ.get('AMP_REFERENCE', '/root/reference')
sys.path.insert(0, REF)
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from config import Config    # noqa: E402  (reference module)
from channel import Channel  # noqa: E402
from data import Data        # noqa: E402
from loss import Loss        # noqa: E402
import vamp as ref_vamp      # noqa: E402
import bamp as ref_bamp      # noqa: E402
import scamp as ref_scamp    # noqa: E402
import shrink as ref_shrink  # noqa: E402

sys.path.append(os.path.dirname(HERE))      # tests/, after everything else: the fixture readers
from golden_io import save_parts            # noqa: E402

torch.set_num_threads(int(os.environ.get('GOLDEN_THREADS', '8')))


def cfg_of(Nt, Na, Nr, B, alphabet, iterations=20, Lin=1, Lh=1):
    return Config(Nt, Na, Nr, Lin, Lh, batch=B, generator_mode='sparc', iterations=iterations,
                  alphabet=alphabet, channel_profile='uniform', channel_truncation='tail', device='cpu')


def snr_of(cfg, EbN0):
    return 10 ** ((EbN0 + 10 * np.log10(cfg.code_rate)) / 10)


def gen_inputs(cfg, seed, EbN0, svd=True):
    np.random.seed(seed)
    torch.manual_seed(seed)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    U = s = Vh = None
    if svd:
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
    x, sym, idx = da.generate_message()
    SNR = snr_of(cfg, EbN0)
    y = A @ x + ch.awgn(SNR)
    return dict(W=W, A=A, U=U, s=s, Vh=Vh, x=x, sym=sym, idx=idx, y=y, SNR=SNR)


def perturbed_rerun(algo, cfg, inp):
    """The reference once more on the same inputs with y scaled by (1 + 2^-23) — a one-ulp
    perturbation, the size of a BLAS summation-order change.  Where the detector is well
    conditioned nothing moves; near a slow fixed point or in a diverging regime T / ier move
    (the reference is not reproducible there under reordering); the GPU tests accept the
    spread of the two runs (SURVEY.md §7 hard part 3)."""
    y = inp['y'] * np.float32(1.0 + 2.0 ** -23)
    if algo == 'vamp':
        L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    elif algo == 'bamp':
        L = ref_bamp.BAMP(cfg)(inp['A'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    else:
        L = ref_scamp.SCAMP(cfg)(inp['W'], inp['A'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    return {f'{k}_pert': float(np.asarray(L.loss[k])) for k in ('T', 'ver', 'ser', 'ier', 'fer')}


def loss_to_json(loss):
    out = {}
    for k, v in loss.items():
        v = np.asarray(v)
        out[k] = float(v) if v.ndim == 0 else [float(t) for t in v.ravel()]
    return out


def sha(t):
    a = t.numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def c(t):
    """torch [B,N,1] / [n,N] -> numpy without the trailing singleton."""
    a = t.detach().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.ndim == 3 and a.shape[-1] == 1:
        a = a[..., 0]
    return a.copy()


# ---------------------------------------------------------------------------
def g1():
    """Per-iteration traces with stored inputs."""
    out = {}
    cases = []
    for alph in ['QPSK', '16QAM']:
        for EbN0 in [0.0, 6.0, 20.0, 30.0]:
            for seed in [0, 1]:
                cases.append(('vamp', alph, EbN0, seed))
    for alph in ['QPSK']:
        for EbN0 in [0.0, 6.0, 12.0]:
            cases.append(('bamp', alph, EbN0, 0))
    for alph in ['QPSK', '16QAM']:
        for EbN0 in [2.0, 8.0]:
            cases.append(('scamp', alph, EbN0, 0))
    for algo, alph, EbN0, seed in cases:
        if algo == 'vamp':
            cfg = cfg_of(16, 2, 32, 8, alph)
        elif algo == 'bamp':
            cfg = cfg_of(4, 1, 8, 100, alph, iterations=10)
        else:
            cfg = cfg_of(32, 4, 64, 16, alph)
        inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
        trace = []
        if algo == 'vamp':
            orig = ref_vamp.VAMPLayer.forward

            def hook(self, T, _o=orig):
                _o(self, T)
                trace.append(dict(r=c(T.r), xmmse=c(T.xmmse), var=c(T.var), r_tilde=c(T.r_tilde),
                                  sigma2_tilde=float(T.sigma2_tilde)))
            ref_vamp.VAMPLayer.forward = hook
            try:
                L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'],
                                       inp['sym'], inp['idx'])
            finally:
                ref_vamp.VAMPLayer.forward = orig
        elif algo == 'bamp':
            orig = ref_bamp.BAMPLayer.forward

            def hook(self, T, _o=orig):
                _o(self, T)
                trace.append(dict(xmap=c(T.xmap), xmmse=c(T.xmmse), var=c(T.var), z=c(T.z), u=c(T.u)))
            ref_bamp.BAMPLayer.forward = hook
            try:
                L = ref_bamp.BAMP(cfg)(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
            finally:
                ref_bamp.BAMPLayer.forward = orig
        else:
            orig = ref_scamp.SCAMPLayer.forward

            def hook(self, T, _o=orig):
                _o(self, T)
                trace.append(dict(xmap=c(T.xmap), xmmse=c(T.xmmse), psi=c(T.psi), z=c(T.z)))
            ref_scamp.SCAMPLayer.forward = hook
            try:
                L = ref_scamp.SCAMP(cfg)(inp['W'], inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'],
                                         inp['idx'])
            finally:
                ref_scamp.SCAMPLayer.forward = orig
        key = f'{algo}_{alph}_{EbN0:g}_{seed}'
        rec = dict(Nt=cfg.Nt, Na=cfg.Na, Nr=cfg.Nr, B=cfg.B, iters=cfg.N_Layers, SNR=inp['SNR'],
                   A=c(inp['A']), W=c(inp['W']), y=c(inp['y']), x=c(inp['x']), sym=inp['sym'],
                   idx=inp['idx'], T=len(trace), loss=json.dumps(loss_to_json(L.loss)))
        if algo == 'vamp':
            rec.update(U=c(inp['U']), s=c(inp['s']), Vh=c(inp['Vh']))
        for t, tr in enumerate(trace):
            for k, v in tr.items():
                rec[f'it{t}_{k}'] = v
        out[key] = rec
        print(key, 'T=', len(trace), flush=True)
    flat = {}
    for key, rec in out.items():
        for k, v in rec.items():
            flat[f'{key}/{k}'] = np.asarray(v)
    save_parts('g1_traces', flat)       # larger than 1 MiB in one file: g1_traces.part<k>.npz


# ---------------------------------------------------------------------------
def g2():
    """Denoiser unit vectors straight from the reference denoiser methods."""
    rng = np.random.default_rng(1234)
    flat = {}
    n = 0
    for alph in ['QPSK', '16QAM', 'BPSK', 'OOK', '8PSK']:
        for (Nt, Na, B) in [(16, 2, 8), (64, 4, 4)]:
            cfg = cfg_of(Nt, Na, 2 * Nt, B, alph)
            lay_v = ref_vamp.VAMPLayer(cfg)
            lay_b = ref_bamp.BAMPLayer(cfg)
            lay_s = ref_scamp.SCAMPLayer(cfg)
            for tau in [1e-9, 1e-4, 1e-2, 0.1, 0.5, 2.0, 1e2]:
                r = (rng.standard_normal((B, Nt)) + 1j * rng.standard_normal((B, Nt))).astype(np.complex64) * 0.7
                # plant one strong entry per section so the posterior is peaked
                sec = r.reshape(B, Na, Nt // Na)
                pos = rng.integers(0, Nt // Na, size=(B, Na))
                kk = rng.integers(0, cfg.K, size=(B, Na))
                for b in range(B):
                    for l in range(Na):
                        sec[b, l, pos[b, l]] += cfg.symbols[kk[b, l]]
                r = sec.reshape(B, Nt)
                rt = torch.from_numpy(r).view(B, Nt, 1)
                xm_v, var_v = lay_v.segmented_denoiser(rt, torch.tensor(np.float32(tau)))
                cov = (np.abs(rng.standard_normal((B, Nt))) * 0.5 + 0.5).astype(np.float32) * np.float32(tau)
                xm_b, var_b = lay_b.segmented_denoiser(rt, torch.from_numpy(cov).view(B, Nt, 1))
                tau_use = np.repeat((np.abs(rng.standard_normal((B, 1))) + 0.5).astype(np.float32) * np.float32(tau),
                                    Nt, axis=1)
                xm_s = lay_s.denoiser(rt, torch.from_numpy(tau_use).view(B, Nt, 1))
                key = f'case{n}'
                flat.update({f'{key}/alphabet': np.array(alph), f'{key}/Nt': np.array(Nt),
                             f'{key}/Na': np.array(Na), f'{key}/B': np.array(B),
                             f'{key}/r': r, f'{key}/tau': np.array(np.float32(tau)), f'{key}/cov': cov,
                             f'{key}/tau_use': tau_use,
                             f'{key}/v_xmmse': c(xm_v), f'{key}/v_var': c(var_v),
                             f'{key}/b_xmmse': c(xm_b), f'{key}/b_var': c(var_b),
                             f'{key}/s_xmmse': c(xm_s)})
                n += 1
    # NaN onset: one section far above the rest at a tiny tau (float64 underflow -> 0/0).
    for alph in ['QPSK', '16QAM']:
        cfg = cfg_of(16, 2, 32, 4, alph)
        lay_v = ref_vamp.VAMPLayer(cfg)
        r = (rng.standard_normal((4, 16)) * 0.01 + 1j * rng.standard_normal((4, 16)) * 0.01).astype(np.complex64)
        r[0, 3] = 1.0 + 1.0j
        for tau in [1e-3, 5e-4, 1e-4]:
            xm_v, var_v = lay_v.segmented_denoiser(torch.from_numpy(r).view(4, 16, 1), torch.tensor(np.float32(tau)))
            key = f'case{n}'
            flat.update({f'{key}/alphabet': np.array(alph), f'{key}/Nt': np.array(16), f'{key}/Na': np.array(2),
                         f'{key}/B': np.array(4), f'{key}/r': r, f'{key}/tau': np.array(np.float32(tau)),
                         f'{key}/v_xmmse': c(xm_v), f'{key}/v_var': c(var_v), f'{key}/nan_case': np.array(1)})
            n += 1
    flat['ncases'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'g2_denoiser.npz'), **flat)
    print('g2 cases', n)


# ---------------------------------------------------------------------------
def g3():
    """MAP decision + metrics on crafted inputs."""
    rng = np.random.default_rng(99)
    flat = {}
    n = 0
    for alph in ['QPSK', '16QAM', 'BPSK', '8PSK', 'OOK']:
        for (Nt, Na, Nr, B, Lin, Lh) in [(16, 2, 32, 8, 1, 1), (32, 4, 16, 6, 3, 2)]:
            cfg = Config(Nt, Na, Nr, Lin, Lh, batch=B, generator_mode='sparc', iterations=5, alphabet=alph,
                         channel_profile='uniform', channel_truncation='tail', device='cpu')
            np.random.seed(n)
            x, sym, idx = Data(cfg).generate_message()
            for variant in ['noisy', 'ties', 'nanrows', 'exact']:
                xv = c(x).reshape(B, -1)
                if variant == 'noisy':
                    xmap = xv + (rng.standard_normal(xv.shape) + 1j * rng.standard_normal(xv.shape)).astype(np.complex64) * 0.4
                elif variant == 'ties':
                    xmap = np.zeros_like(xv)          # every logit equal -> first index
                    xmap[::2] = xv[::2]
                elif variant == 'nanrows':
                    xmap = xv + (rng.standard_normal(xv.shape)).astype(np.complex64) * 0.2
                    xmap[0, :] = np.nan
                    if B > 2:
                        xmap[2, 1] = np.nan + 0j
                else:
                    xmap = xv.copy()
                xmap = xmap.astype(np.complex64)
                xmmse = (xv + rng.standard_normal(xv.shape).astype(np.float32) * 0.1).astype(np.complex64)
                L = Loss(cfg)
                L(torch.from_numpy(xmap).view(B, -1, 1), torch.from_numpy(xmmse).view(B, -1, 1), x, sym, idx, 3)
                dec = L.decision(xmap.reshape(-1, cfg.Lin, cfg.Nt))
                key = f'case{n}'
                flat.update({f'{key}/alphabet': np.array(alph), f'{key}/dims': np.array([Nt, Na, Nr, B, Lin, Lh]),
                             f'{key}/xmap': xmap, f'{key}/xmmse': xmmse, f'{key}/x': c(x).reshape(B, -1),
                             f'{key}/sym': sym, f'{key}/idx': idx,
                             f'{key}/xhat': dec[0], f'{key}/shat': dec[1], f'{key}/ihat': dec[2],
                             f'{key}/loss': np.array(json.dumps(loss_to_json(L.loss)))})
                n += 1
    flat['ncases'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'g3_decision.npz'), **flat)
    print('g3 cases', n)


# ---------------------------------------------------------------------------
def g5():
    """Shrink (shrink.py:8-166) outputs straight from the reference class."""
    rng = np.random.default_rng(555)
    flat = {}
    n = 0
    shapes = [(16, 2, 4), (64, 4, 8), (24, 2, 3), (256, 2, 2)]     # (Nt, Na, B): M = 8, 16, 12, 128
    combos = [(a, True) for a in ['OOK', 'BPSK', '4ASK', 'QPSK', '8PSK', '16PSK', '16QAM']] + \
             [(a, False) for a in ['OOK', 'BPSK', '4ASK']]
    for alph, is_complex in combos:
        for si, (Nt, Na, B) in enumerate(shapes):
            cfg = Config(Nt, Na, 2 * Nt, 1, 1, batch=B, generator_mode='sparc', iterations=5, alphabet=alph,
                         channel_profile='uniform', channel_truncation='tail', is_complex=is_complex, device='cpu')
            covs = [1e-3, 0.05, 0.5, 3.0, 'vec'] if si < 2 else [0.2, 'vec']
            for cv in covs:
                # sparse truth (one active point per section) + noise
                x = np.zeros((B, Nt), dtype=np.complex128)
                M = Nt // Na
                for b in range(B):
                    for l in range(Na):
                        x[b, l * M + rng.integers(M)] = cfg.symbols[rng.integers(cfg.K)]
                sd = 0.3 if cv == 'vec' else float(np.sqrt(max(cv, 1e-2)))
                noise = rng.standard_normal((B, Nt)) + (1j * rng.standard_normal((B, Nt)) if is_complex else 0)
                r = (x + sd * noise)
                r = r.astype(np.complex64) if is_complex else r.real.astype(np.float32)
                if cv == 'vec':
                    cov = ((np.abs(rng.standard_normal((B, Nt))) + 0.05) * 0.3).astype(np.float32)
                    cov_t = torch.from_numpy(cov).view(B, Nt, 1)
                else:
                    cov = np.array(np.float32(cv))
                    cov_t = torch.tensor(np.float32(cv))
                rt = torch.from_numpy(r).view(B, Nt, 1)
                S = ref_shrink.Shrink(cfg, 'bayes')
                xb = S(rt.clone(), cov_t.clone())
                So = ref_shrink.Shrink(cfg, 'shrinkOOK')
                xo, do = So(rt.clone(), cov_t.clone())
                xs, vs = So.sw_shrinkOOK(rt.clone(), cov_t.clone())
                key = f'case{n}'
                flat.update({f'{key}/alphabet': np.array(alph), f'{key}/is_complex': np.array(int(is_complex)),
                             f'{key}/dims': np.array([Nt, Na, B]), f'{key}/r': r, f'{key}/cov': cov,
                             f'{key}/bayes': c(xb), f'{key}/ook_x': c(xo), f'{key}/ook_dxdr': c(do),
                             f'{key}/sw_x': c(xs), f'{key}/sw_var': c(vs)})
                n += 1
    # overflow regimes: logits at / above log(FLT_MAX) (regularize_exp), leave-one-out sums
    # that overflow to inf (sw: inf - inf = NaN) and a section whose only large logit wins
    for alph in ['OOK', 'QPSK']:
        Nt, Na, B = 16, 2, 2
        cfg = Config(Nt, Na, 2 * Nt, 1, 1, batch=B, generator_mode='sparc', iterations=5, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        for cv in [1e-2, 5e-3, 1e-4]:
            r = (0.5 + 0.1 * rng.standard_normal((B, Nt))).astype(np.complex64)
            r[0, 2] = 1.0
            r[0, 9] = 1.5
            r[0, 10] = 1.5
            r[1, :8] = 2.0
            rt = torch.from_numpy(r).view(B, Nt, 1)
            cov_t = torch.tensor(np.float32(cv))
            xb = ref_shrink.Shrink(cfg, 'bayes')(rt.clone(), cov_t.clone())
            So = ref_shrink.Shrink(cfg, 'shrinkOOK')
            xo, do = So(rt.clone(), cov_t.clone())
            xs, vs = So.sw_shrinkOOK(rt.clone(), cov_t.clone())
            key = f'case{n}'
            flat.update({f'{key}/alphabet': np.array(alph), f'{key}/is_complex': np.array(1),
                         f'{key}/dims': np.array([Nt, Na, B]), f'{key}/r': r, f'{key}/cov': np.array(np.float32(cv)),
                         f'{key}/bayes': c(xb), f'{key}/ook_x': c(xo), f'{key}/ook_dxdr': c(do),
                         f'{key}/sw_x': c(xs), f'{key}/sw_var': c(vs), f'{key}/overflow': np.array(1)})
            n += 1
    flat['ncases'] = np.array(n)
    save_parts('g5_shrink', flat)       # larger than 1 MiB in one file: g5_shrink.part<k>.npz
    print('g5 cases', n)


# ---------------------------------------------------------------------------
def correlated_channel(Nr, Nt, rho):
    """Same recursion as the build's Channel.generate_correlated (its SHA is checked by the
    tests): G ~ CN(0, 1/Nr), AR(1) filter over rows then columns, float64, then complex64."""
    gr = np.random.normal(size=(Nr, Nt))
    gi = np.random.normal(size=(Nr, Nt))
    A = (gr + 1j * gi) / np.sqrt(2 * Nr)
    c = np.sqrt(1.0 - rho * rho)
    for i in range(1, Nr):
        A[i] = rho * A[i - 1] + c * A[i]
    for j in range(1, Nt):
        A[:, j] = rho * A[:, j - 1] + c * A[:, j]
    return torch.tensor(A.astype(np.complex64))


def inject_square_qam(cfg, K=64):
    """Square K-QAM (unit mean power, per-axis binary-reflected gray code) injected into a
    reference Config after construction, as SURVEY.md §8(c) verified the reference's BAMP takes
    it: the reference's Config rejects 64QAM (config.py:44).  Every Config attribute the
    constellation feeds is set the way config.py:117-157 would derive it."""
    m = int(round(np.sqrt(K)))
    b = int(np.log2(m))
    levels = np.arange(-(m - 1), m, 2)
    g1 = [i ^ (i >> 1) for i in range(m)]
    pts = [complex(levels[i], levels[q]) for i in range(m) for q in range(m)]
    cfg.symbols = np.array(pts) / np.sqrt(np.mean(np.abs(pts) ** 2))
    cfg.gray = [(g1[i] << b) | g1[q] for i in range(m) for q in range(m)]
    cfg.alphabet = f'{K}QAM'
    cfg.K = K
    cfg.symbol_bits = int(np.log2(K))
    cfg.Ps = cfg.sparsity / K
    cfg.is_complex = True
    cfg.inner_code_rate = cfg.Na * np.log2(cfg.M * cfg.K) / cfg.Mr
    cfg.code_rate = cfg.Lc * cfg.inner_code_rate / cfg.Lr
    cfg.min_amp_snr = 1 / (cfg.kappa * (1 / (np.exp(2 * cfg.code_rate) - 1) - 1 / cfg.Lh))
    cfg.min_snr = 2 ** cfg.code_rate - 1
    cfg.min_snr_dB = 10 * np.log10(cfg.min_snr)
    cfg.shannon_limit_dB = cfg.min_snr_dB - 10 * np.log10(cfg.code_rate)
    cfg.name = (f'{cfg.alphabet},{cfg.mode}/{cfg.profile},{cfg.trunc}/'
                f'Nt={cfg.Nt},Na={cfg.Na},Nr={cfg.Nr},Lh={cfg.Lh},Lin={cfg.Lin}')
    return cfg


G6_CONFIGS = {
    'cfg5_bamp_corr_16qam': (512, 16, 1024, 1024, '16QAM', 20, [6, 10, 14, 18], [0]),
    'cfg5_bamp_corr_qpsk': (512, 16, 1024, 1024, 'QPSK', 20, [2, 6, 10, 14], [0]),
    # BASELINE cfg5's own alphabet (round 2): 64-QAM injected into the reference's Config
    'cfg5_bamp_corr_64qam': (512, 16, 1024, 1024, '64QAM', 20, [0, 2, 4, 6, 7, 8, 9, 10, 14, 18, 22, 26], [0]),
    'cfg5_bamp_corr_64qam_b8192': (512, 16, 1024, 8192, '64QAM', 20, [6], [0]),
}


def g6(names=None):
    path = os.path.join(HERE, 'g6_cfg5_corr.json')
    db = json.load(open(path)) if os.path.exists(path) else {}
    rho = 0.5
    for name, (Nt, Na, Nr, B, alph, iters, grid, seeds) in G6_CONFIGS.items():
        if names and name not in names:
            continue
        if alph == '64QAM':
            cfg = inject_square_qam(cfg_of(Nt, Na, Nr, B, '16QAM', iterations=iters), 64)
        else:
            cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db.get(name, {'algo': 'bamp', 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'B': B, 'alphabet': alph,
                            'iterations': iters, 'rho': rho, 'points': {}})
        if alph == '64QAM':
            ent['symbols_re'] = [float(v) for v in np.real(cfg.symbols)]
            ent['symbols_im'] = [float(v) for v in np.imag(cfg.symbols)]
            ent['gray'] = [int(v) for v in cfg.gray]
            ent['code_rate'] = float(cfg.code_rate)
        for seed in seeds:
            for EbN0 in grid:
                if f'{seed}/{EbN0}' in ent['points']:
                    continue
                t0 = time.time()
                np.random.seed(seed)
                torch.manual_seed(seed)
                ch, da = Channel(cfg), Data(cfg)
                A = correlated_channel(Nr, Nt, rho)
                x, sym, idx = da.generate_message()
                SNR = snr_of(cfg, float(EbN0))
                y = A @ x + ch.awgn(SNR)
                L = ref_bamp.BAMP(cfg)(A, y, SNR, x, sym, idx)
                rec = loss_to_json(L.loss)
                rec['sha_A'] = sha(A)
                rec['sha_x'] = sha(x)
                rec['y_abs2_sum'] = float(np.sum(np.abs(y.numpy().astype(np.complex128)) ** 2))
                rec['SNR'] = float(SNR)
                ent['points'][f'{seed}/{EbN0}'] = rec
                print(name, seed, EbN0, 'T=', rec['T'], 'ver=', rec['ver'], 'ser=', rec['ser'],
                      f'{time.time() - t0:.1f}s', flush=True)
                db[name] = ent
                with open(path, 'w') as f:
                    json.dump(db, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------
def g7():
    """generator_mode='segmented' at B = 1 (the only batch its decision reshape accepts)."""
    rng = np.random.default_rng(77)
    flat = {}
    n = 0
    for alph in ['QPSK', '16QAM', 'BPSK', '8PSK', 'OOK']:
        for (Nt, Na, Nr, Lin, Lh) in [(16, 2, 32, 1, 1), (64, 4, 32, 3, 2), (128, 2, 64, 1, 1)]:
            cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='segmented', iterations=5, alphabet=alph,
                         channel_profile='uniform', channel_truncation='tail', device='cpu')
            np.random.seed(n)
            x, sym, idx = Data(cfg).generate_message()
            xv = c(x).reshape(1, -1)
            for variant in ['noisy', 'ties', 'zeros', 'exact']:
                if variant == 'noisy':
                    xmap = xv + (rng.standard_normal(xv.shape) + 1j * rng.standard_normal(xv.shape)).astype(np.complex64) * 0.4
                elif variant == 'ties':
                    xmap = xv.copy()
                    xmap[0, 1::3] = xmap[0, 1::3] + np.complex64(1.0)    # repeated magnitudes inside sections
                    xmap[0, ::5] = np.complex64(1.0 + 0j)
                elif variant == 'zeros':
                    xmap = np.zeros_like(xv)                              # every |x| equal -> last position
                    xmap[0, :Nt // Na] = xv[0, :Nt // Na]
                else:
                    xmap = xv.copy()
                xmap = xmap.astype(np.complex64)
                xmmse = (xv + rng.standard_normal(xv.shape).astype(np.float32) * 0.1).astype(np.complex64)
                L = Loss(cfg)
                L(torch.from_numpy(xmap).view(1, -1, 1), torch.from_numpy(xmmse).view(1, -1, 1), x, sym, idx, 3)
                dec = L.decision(xmap.reshape(-1, cfg.Lin, cfg.Nt))
                key = f'case{n}'
                flat.update({f'{key}/alphabet': np.array(alph), f'{key}/dims': np.array([Nt, Na, Nr, 1, Lin, Lh]),
                             f'{key}/xmap': xmap, f'{key}/xmmse': xmmse, f'{key}/x': xv,
                             f'{key}/sym': sym, f'{key}/idx': idx,
                             f'{key}/xhat': dec[0], f'{key}/shat': dec[1], f'{key}/ihat': dec[2],
                             f'{key}/loss': np.array(json.dumps(loss_to_json(L.loss)))})
                n += 1
    flat['ncases'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'g7_segmented.npz'), **flat)
    print('g7 decision cases', n)
    # detectors end to end (B = 1, one epoch per seed, the reference's call order)
    curves = {}
    for algo in ['vamp', 'bamp']:
        for alph in ['QPSK', '16QAM']:
            Nt, Na, Nr = 32, 4, 64
            cfg = Config(Nt, Na, Nr, 1, 1, batch=1, generator_mode='segmented', iterations=20, alphabet=alph,
                         channel_profile='uniform', channel_truncation='tail', device='cpu')
            pts = {}
            for EbN0 in [0, 4, 8, 12, 16]:
                for seed in range(6):
                    inp = gen_inputs(cfg, seed, float(EbN0), svd=(algo == 'vamp'))
                    if algo == 'vamp':
                        L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'],
                                               inp['sym'], inp['idx'])
                    else:
                        L = ref_bamp.BAMP(cfg)(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                    rec = loss_to_json(L.loss)
                    rec['sha_A'] = sha(inp['A'])
                    rec['sha_x'] = sha(inp['x'])
                    pts[f'{seed}/{EbN0}'] = rec
            curves[f'seg_{algo}_{alph}'] = {'algo': algo, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'B': 1, 'alphabet': alph,
                                            'iterations': 20, 'points': pts}
            print('g7', algo, alph, 'ver', [round(p['ver'], 2) for p in pts.values()][:10])
    with open(os.path.join(HERE, 'g7_segmented_curves.json'), 'w') as f:
        json.dump(curves, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------
def g8():
    """generator_mode='random' at B = 1."""
    rng = np.random.default_rng(88)
    flat = {}
    n = 0
    for alph in ['QPSK', '16QAM', 'BPSK', '8PSK']:
        for (Nt, Na, Nr, Lin, Lh) in [(16, 2, 32, 1, 1), (24, 3, 32, 3, 2), (64, 8, 64, 2, 1)]:
            cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='random', iterations=5, alphabet=alph,
                         channel_profile='uniform', channel_truncation='tail', device='cpu')
            np.random.seed(n)
            x, sym, idx = Data(cfg).generate_message()
            xv = c(x).reshape(1, -1)
            for variant in ['noisy', 'weak', 'exact']:
                if variant == 'noisy':
                    xmap = xv + (rng.standard_normal(xv.shape) + 1j * rng.standard_normal(xv.shape)).astype(np.complex64) * 0.4
                elif variant == 'weak':
                    xmap = 0.3 * xv + (rng.standard_normal(xv.shape) + 1j * rng.standard_normal(xv.shape)).astype(np.complex64) * 0.3
                else:
                    xmap = xv.copy()
                xmap = xmap.astype(np.complex64)
                xmmse = (xv + rng.standard_normal(xv.shape).astype(np.float32) * 0.1).astype(np.complex64)
                L = Loss(cfg)
                L(torch.from_numpy(xmap).view(1, -1, 1), torch.from_numpy(xmmse).view(1, -1, 1), x, sym, idx, 3)
                dec = L.decision(xmap.reshape(-1, cfg.Lin, cfg.Nt))
                key = f'case{n}'
                flat.update({f'{key}/alphabet': np.array(alph), f'{key}/dims': np.array([Nt, Na, Nr, 1, Lin, Lh]),
                             f'{key}/xmap': xmap, f'{key}/xmmse': xmmse, f'{key}/x': xv,
                             f'{key}/sym': sym, f'{key}/idx': idx,
                             f'{key}/xhat': dec[0], f'{key}/shat': dec[1], f'{key}/ihat': dec[2],
                             f'{key}/loss': np.array(json.dumps(loss_to_json(L.loss)))})
                n += 1
    flat['ncases'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'g8_random.npz'), **flat)
    print('g8 decision cases', n)
    curves = {}
    for alph in ['QPSK', '16QAM']:
        Nt, Na, Nr = 32, 4, 64
        cfg = Config(Nt, Na, Nr, 1, 1, batch=1, generator_mode='random', iterations=20, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        pts = {}
        for EbN0 in [0, 4, 8, 12, 16]:
            for seed in range(6):
                inp = gen_inputs(cfg, seed, float(EbN0), svd=False)
                L = ref_bamp.BAMP(cfg)(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                rec = loss_to_json(L.loss)
                rec['sha_A'] = sha(inp['A'])
                rec['sha_x'] = sha(inp['x'])
                pts[f'{seed}/{EbN0}'] = rec
        curves[f'rand_bamp_{alph}'] = {'algo': 'bamp', 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'B': 1, 'alphabet': alph,
                                       'iterations': 20, 'points': pts}
        print('g8 bamp', alph, 'ver', [round(p['ver'], 2) for p in pts.values()][:10])
    cfg = Config(32, 4, 64, 1, 1, batch=1, generator_mode='random', iterations=20, alphabet='QPSK',
                 channel_profile='uniform', channel_truncation='tail', device='cpu')
    inp = gen_inputs(cfg, 0, 8.0, svd=True)
    try:
        ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
        curves['vamp_random_error'] = None
    except Exception as e:  # noqa: BLE001  (recorded, not raised)
        curves['vamp_random_error'] = [type(e).__name__, str(e)]
    with open(os.path.join(HERE, 'g8_random_curves.json'), 'w') as f:
        json.dump(curves, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------
def g9():
    """BAMPLayer.random_denoiser straight from the reference layer ('random' mode)."""
    rng = np.random.default_rng(99)
    flat = {}
    n = 0
    for alph in ['QPSK', '16QAM', 'BPSK', '8PSK', 'OOK']:
        cfg = Config(32, 4, 64, 1, 1, batch=4, generator_mode='random', iterations=5, alphabet=alph,
                     channel_profile='uniform', channel_truncation='tail', device='cpu')
        lay = ref_bamp.BAMPLayer(cfg)
        for scale in [1e-4, 1e-2, 0.1, 1.0, 10.0]:
            r = ((rng.standard_normal((4, 32)) + 1j * rng.standard_normal((4, 32))) * 0.7).astype(np.complex64)
            cov = ((np.abs(rng.standard_normal((4, 32))) + 0.2) * scale).astype(np.float32)
            xm, var = lay.random_denoiser(torch.from_numpy(r).view(4, 32, 1), torch.from_numpy(cov).view(4, 32, 1))
            key = f'case{n}'
            flat.update({f'{key}/alphabet': np.array(alph), f'{key}/r': r, f'{key}/cov': cov,
                         f'{key}/xmmse': c(xm), f'{key}/var': c(var)})
            n += 1
    flat['ncases'] = np.array(n)
    np.savez_compressed(os.path.join(HERE, 'g9_bamp_random_denoise.npz'), **flat)
    print('g9 cases', n)


# ---------------------------------------------------------------------------
G10_RUNS = {
    # name: (driver module, Nt, Na, Nr, B, alphabet, iterations, seed, simulate kwargs)
    'vamp_cfg2_qpsk': ('vamp_model', 64, 4, 128, 1024, 'QPSK', 20, 3, dict(epochs=4, start=2.0, final=6.0, step=2.0,
                                                                           res=2)),
    'bamp_cfg1_qpsk': ('bamp_model', 4, 1, 8, 100, 'QPSK', 10, 5, dict(epochs=6, start=0.0, final=20.0, step=4.0,
                                                                       res=3)),
    'scamp_qpsk': ('scamp_model', 128, 8, 256, 512, 'QPSK', 20, 7, dict(epochs=4, start=0.0, final=8.0, step=4.0,
                                                                        res=2)),
}


def g10():
    """The reference's own Monte-Carlo drivers (vamp_model.py:45-69, bamp_model.py:44-67,
    scamp_model.py:43-66) run end to end in a scratch directory, seeded once before the Model is
    built; every {EbN0}.json they write is recorded verbatim (keys, values, file names), with
    the epoch / res channel reuse and the FER < 1e-3 early stop as the drivers do them."""
    import importlib
    import shutil
    import tempfile
    import types
    import loss as ref_loss
    # Loss.export (loss.py:319-320) json.dumps the averaged dict, whose nMSE* entries are numpy
    # float32 scalars (complex64 inputs, loss.py:116-119): json raises "TypeError: Object of type
    # float32 is not JSON serializable" at the first SNR point, so the reference driver cannot
    # finish as written.  The golden serialises numpy scalars by value (float(v), exact for
    # float32) — the file the driver means to write; the build's Loss.export does the same.
    ref_loss.json = types.SimpleNamespace(
        dump=lambda obj, f, **kw: json.dump(obj, f, default=lambda o: o.item() if hasattr(o, 'item') else str(o), **kw))
    out = {'_reference_export_error': 'TypeError: Object of type float32 is not JSON serializable '
                                      '(loss.py:320, unpatched)'}
    for name, (mod, Nt, Na, Nr, B, alph, iters, seed, kw) in G10_RUNS.items():
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        drv = importlib.import_module(mod)
        cwd = os.getcwd()
        tmp = tempfile.mkdtemp(prefix='g10_')
        try:
            os.chdir(tmp)
            np.random.seed(seed)
            torch.manual_seed(seed)
            t0 = time.time()
            m = drv.Model(cfg)
            m.simulate(**kw)
            files = {}
            for f in sorted(os.listdir(m.path)):
                if f.endswith('.json'):
                    with open(os.path.join(m.path, f)) as fh:
                        files[f] = json.load(fh)
            out[name] = {'driver': mod, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'B': B, 'alphabet': alph, 'iterations': iters,
                         'seed': seed, 'simulate': kw, 'path': m.path, 'files': files}
            print(name, sorted(files), f'{time.time() - t0:.1f}s', flush=True)
        finally:
            os.chdir(cwd)
            shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(HERE, 'g10_simulate.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------
G11_CONFIGS = {
    # ISI / spatial coupling (Lin > 1, Lh > 1, tail): the reference's published curves all live
    # at Lin = 10-55, Lh = 3-12 (Simulations/); small enough for the CPU reference
    # name: (algo, Nt, Na, Nr, Lin, Lh, B, alphabet, iterations, EbN0 grid, seeds)
    'isi_vamp_qpsk': ('vamp', 32, 4, 32, 4, 2, 64, 'QPSK', 20, [0, 4, 8, 12], [0, 1]),
    'isi_vamp_16qam': ('vamp', 32, 4, 32, 4, 2, 64, '16QAM', 20, [0, 6, 12], [0]),
    'isi_bamp_qpsk': ('bamp', 32, 4, 32, 4, 2, 64, 'QPSK', 20, [0, 4, 8, 12], [0, 1]),
    'isi_bamp_16qam': ('bamp', 32, 4, 32, 4, 2, 64, '16QAM', 20, [0, 6, 12], [0]),
    'isi_scamp_qpsk': ('scamp', 32, 4, 32, 4, 2, 64, 'QPSK', 20, [0, 4, 8, 12], [0, 1]),
    'isi_scamp_16qam': ('scamp', 32, 4, 32, 4, 2, 64, '16QAM', 20, [0, 6, 12], [0]),
    'isi3_scamp_qpsk': ('scamp', 64, 4, 32, 8, 3, 32, 'QPSK', 20, [2, 6, 10], [0]),
    'isi3_bamp_qpsk': ('bamp', 64, 4, 32, 8, 3, 32, 'QPSK', 20, [2, 6, 10], [0]),
}


def g11():
    path = os.path.join(HERE, 'g11_isi.json')
    db = json.load(open(path)) if os.path.exists(path) else {}
    for name, (algo, Nt, Na, Nr, Lin, Lh, B, alph, iters, grid, seeds) in G11_CONFIGS.items():
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters, Lin=Lin, Lh=Lh)
        ent = db.get(name, {'algo': algo, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'Lin': Lin, 'Lh': Lh, 'B': B,
                            'alphabet': alph, 'iterations': iters, 'points': {}})
        for seed in seeds:
            for EbN0 in grid:
                key = f'{seed}/{EbN0}'
                if key in ent['points']:
                    continue
                inp = gen_inputs(cfg, seed, float(EbN0), svd=(algo == 'vamp'))
                if algo == 'vamp':
                    L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'],
                                           inp['sym'], inp['idx'])
                elif algo == 'bamp':
                    L = ref_bamp.BAMP(cfg)(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                else:
                    L = ref_scamp.SCAMP(cfg)(inp['W'], inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'],
                                             inp['idx'])
                rec = loss_to_json(L.loss)
                rec.update(perturbed_rerun(algo, cfg, inp))
                rec['sha_A'] = sha(inp['A'])
                rec['sha_W'] = sha(inp['W'])
                rec['sha_x'] = sha(inp['x'])
                rec['y_abs2_sum'] = float(np.sum(np.abs(inp['y'].numpy().astype(np.complex128)) ** 2))
                ent['points'][key] = rec
                print(name, key, 'T=', rec['T'], 'ver=', rec['ver'], 'ser=', rec['ser'], flush=True)
        db[name] = ent
        with open(path, 'w') as f:
            json.dump(db, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------------------
G12_CASES = [
    # (alphabet, EbN0, seed, damping, Nt, Na, Nr, B): vamp2's VAMP takes damping = 1.0 by default
    # (vamp2.py:96); 0.97 is VAMPLayer's own default (vamp2.py:29)
    ('QPSK', 0.0, 0, 1.0, 16, 2, 32, 8), ('QPSK', 6.0, 0, 1.0, 16, 2, 32, 8), ('QPSK', 20.0, 1, 1.0, 16, 2, 32, 8),
    ('16QAM', 6.0, 0, 1.0, 16, 2, 32, 8), ('16QAM', 20.0, 1, 1.0, 16, 2, 32, 8),
    ('QPSK', 6.0, 0, 0.97, 16, 2, 32, 8), ('16QAM', 12.0, 2, 0.97, 16, 2, 32, 8),
    ('QPSK', 8.0, 0, 1.0, 64, 4, 128, 64), ('16QAM', 8.0, 0, 1.0, 64, 4, 128, 64),
]


def g12():
    """vamp2.py (damped "Rangan" VAMP, vamp2.py:12-131): per-iteration traces (r, xmmse, var,
    gamma after every layer) and the Loss dict, inputs stored.  Sparc mode only: the reference
    crashes in 'random' / 'segmented' mode."""
    import vamp2 as ref_vamp2
    out = {}
    for alph, EbN0, seed, damp, Nt, Na, Nr, B in G12_CASES:
        cfg = cfg_of(Nt, Na, Nr, B, alph)
        inp = gen_inputs(cfg, seed, EbN0)
        trace = []
        orig = ref_vamp2.VAMPLayer.forward

        def hook(self, T, _o=orig):
            _o(self, T)
            trace.append(dict(r=c(T.r), xmmse=c(T.xmmse), var=c(T.var), gamma=float(T.gamma)))
        ref_vamp2.VAMPLayer.forward = hook
        try:
            L = ref_vamp2.VAMP(cfg, damping=damp)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'],
                                                  inp['sym'], inp['idx'])
        finally:
            ref_vamp2.VAMPLayer.forward = orig
        key = f'vamp2_{alph}_{Nt}_{EbN0:g}_{seed}_{damp:g}'
        rec = dict(Nt=Nt, Na=Na, Nr=Nr, B=B, iters=cfg.N_Layers, SNR=inp['SNR'], damping=damp,
                   U=c(inp['U']), s=c(inp['s']), Vh=c(inp['Vh']), y=c(inp['y']), x=c(inp['x']), sym=inp['sym'],
                   idx=inp['idx'], T=len(trace), loss=json.dumps(loss_to_json(L.loss)))
        keep = range(len(trace)) if Nt <= 16 else [0, len(trace) - 1]
        for t in keep:
            for k, v in trace[t].items():
                rec[f'it{t}_{k}'] = v
        out[key] = rec
        print(key, 'T=', len(trace), 'ver', float(L.loss['ver']), 'gamma', [round(t['gamma'], 4) for t in trace][:6],
              flush=True)
    flat = {}
    for key, rec in out.items():
        for k, v in rec.items():
            flat[f'{key}/{k}'] = np.asarray(v)
    np.savez_compressed(os.path.join(HERE, 'g12_vamp2.npz'), **flat)


# ---------------------------------------------------------------------------
G4_CONFIGS = {
    # name: (algo, Nt, Na, Nr, B, alphabet, iterations, EbN0 grid, seeds)
    # (round 2: seeds {0, 1, 2} over EbN0 0-20 step 1 for cfg2-cfg4)
    'cfg1_bamp_qpsk': ('bamp', 4, 1, 8, 100, 'QPSK', 10, list(range(0, 21, 2)), [0, 1]),
    'cfg2_vamp_16qam': ('vamp', 64, 4, 128, 1024, '16QAM', 20, list(range(0, 21)), [0, 1, 2]),
    'cfg2_vamp_qpsk': ('vamp', 64, 4, 128, 1024, 'QPSK', 20, list(range(0, 21)), [0, 1, 2]),
    'cfg3_scamp_16qam': ('scamp', 128, 8, 256, 4096, '16QAM', 20, list(range(0, 21)), [0, 1, 2]),
    'cfg3_scamp_qpsk': ('scamp', 128, 8, 256, 4096, 'QPSK', 20, list(range(0, 21)), [0, 1, 2]),
    'cfg4_vamp_16qam': ('vamp', 256, 8, 512, 4096, '16QAM', 20, list(range(0, 21)), [0, 1, 2]),
    'cfg4_vamp_qpsk': ('vamp', 256, 8, 512, 4096, 'QPSK', 20, list(range(0, 21)), [0, 1, 2]),
}


def g4p(names=None):
    """Add the one-ulp perturbed rerun (perturbed_rerun) to every g4 point that lacks it."""
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path))
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db[name]
        for key in sorted(ent['points'], key=lambda k: (int(k.split('/')[0]), float(k.split('/')[1]))):
            rec = ent['points'][key]
            if 'T_pert' in rec:
                continue
            seed, EbN0 = int(key.split('/')[0]), float(key.split('/')[1])
            inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
            assert sha(inp['x']) == rec['sha_x']
            rec.update(perturbed_rerun(algo, cfg, inp))
            print(name, key, 'T', rec['T'], rec['T_pert'], 'ver', rec['ver'], rec['ver_pert'], flush=True)
            with open(path, 'w') as f:
                json.dump(db, f, indent=1, sort_keys=True)


PERTURBATIONS = (1.0 - 2.0 ** -23, 1.0 + 2.0 ** -22, 1.0 - 2.0 ** -22)


def g4pp(names=None):
    """Where the reference's own early exit moved under the one-ulp rerun (T != T_pert), three more
    reruns with y scaled by PERTURBATIONS: `T_span` = [min, max] of T over all five runs, the bar
    the GPU tests hold T to there (tests/test_gpu_vamp.py _check_T; round-3 review item 7)."""
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path))
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db[name]
        for key in sorted(ent['points'], key=lambda k: (int(k.split('/')[0]), float(k.split('/')[1]))):
            rec = ent['points'][key]
            if 'T_pert' not in rec or rec['T'] == rec['T_pert'] or 'T_span' in rec:
                continue
            seed, EbN0 = int(key.split('/')[0]), float(key.split('/')[1])
            inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
            assert sha(inp['x']) == rec['sha_x']
            Ts = [rec['T'], rec['T_pert']]
            for f in PERTURBATIONS:
                y = inp['y'] * np.float32(f)
                if algo == 'vamp':
                    L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], y, inp['SNR'], inp['x'], inp['sym'],
                                           inp['idx'])
                elif algo == 'bamp':
                    L = ref_bamp.BAMP(cfg)(inp['A'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                else:
                    L = ref_scamp.SCAMP(cfg)(inp['W'], inp['A'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                Ts.append(float(np.asarray(L.loss['T'])))
            rec['T_runs'] = Ts
            rec['T_span'] = [min(Ts), max(Ts)]
            print(name, key, 'T runs', Ts, flush=True)
            with open(path, 'w') as f:
                json.dump(db, f, indent=1, sort_keys=True)


PERT_SEEDS = tuple(range(8))


def g4pp_elem(names=None):
    """More evidence where the reference's exit moved: eight reruns with every element of y moved
    independently by -1, 0 or +1 float32 ulp (seeded), the closest model of a summation-order
    change in the GEMMs.  Appended to `T_runs`; `T_span` widened to their [min, max]."""
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path))
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db[name]
        for key in sorted(ent['points'], key=lambda k: (int(k.split('/')[0]), float(k.split('/')[1]))):
            rec = ent['points'][key]
            if 'T_runs' not in rec or len(rec['T_runs']) > 5:
                continue
            seed, EbN0 = int(key.split('/')[0]), float(key.split('/')[1])
            inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
            assert sha(inp['x']) == rec['sha_x']
            Ts = list(rec['T_runs'])
            for ps in PERT_SEEDS:
                g = torch.Generator().manual_seed(1000 + ps)
                y0 = torch.as_tensor(inp['y'])
                u = torch.randint(-1, 2, y0.shape, generator=g).to(torch.float32) * 2.0 ** -23
                y = y0 * (1.0 + u).to(y0.dtype)
                assert algo == 'vamp'
                L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], y, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                Ts.append(float(np.asarray(L.loss['T'])))
            rec['T_runs'] = Ts
            rec['T_span'] = [min(Ts), max(Ts)]
            print(name, key, 'T runs', Ts, flush=True)
            with open(path, 'w') as f:
                json.dump(db, f, indent=1, sort_keys=True)


def g4pp_den(names=None):
    """Where the reference's exit moved: eight reruns on the UNPERTURBED inputs with every value of
    the denoiser's exponential (vamp.py:110, torch.exp, float64 in the reference) moved by a random
    relative amount within +-2^-22 (seeded) — the size of a float32 evaluation of that denoiser,
    which is what every GPU engine runs (amp_denoise.h).  Appended to `T_runs`, `T_span` widened."""
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path))
    exp0 = torch.exp
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db[name]
        for key in sorted(ent['points'], key=lambda k: (int(k.split('/')[0]), float(k.split('/')[1]))):
            rec = ent['points'][key]
            if 'T_runs' not in rec or 'T_runs_den' in rec:
                continue
            seed, EbN0 = int(key.split('/')[0]), float(key.split('/')[1])
            inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
            assert sha(inp['x']) == rec['sha_x'] and algo == 'vamp'
            Td = []
            for ps in PERT_SEEDS:
                g = torch.Generator().manual_seed(2000 + ps)

                def exp_f32(x, g=g):
                    e = exp0(x)
                    u = (torch.rand(e.shape, generator=g, dtype=torch.float64) * 2 - 1) * 2.0 ** -22
                    return e * (1 + u).to(e.dtype)
                torch.exp = exp_f32
                try:
                    L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'], inp['sym'],
                                           inp['idx'])
                finally:
                    torch.exp = exp0
                Td.append(float(np.asarray(L.loss['T'])))
            rec['T_runs_den'] = Td
            Ts = rec['T_runs'] + Td
            rec['T_span'] = [min(Ts), max(Ts)]
            print(name, key, 'T runs (denoiser exp +-2^-22)', Td, flush=True)
            with open(path, 'w') as f:
                json.dump(db, f, indent=1, sort_keys=True)


def relabel_within_sections(inp, cfg, g):
    """The same problem with the positions of every section permuted (seeded): Vh's columns and x's
    rows move together, so A[:, p] x[p] = A x = y unchanged and U, s, Vh[:, p] are exactly the
    SVD factors of A[:, p].  Only the order of the reference's sums over the positions changes:
    q = Vh r~ (vamp.py:67) reduces over them, and var.mean() (vamp.py:85) sums them in another
    order.  Returns (Vh', x')."""
    M = cfg.Nt // cfg.Na
    nsec = cfg.Nt * cfg.Lin // M
    perm = torch.cat([l * M + torch.randperm(M, generator=g) for l in range(nsec)])
    return inp['Vh'][:, perm].contiguous(), inp['x'][:, perm].contiguous()


# points whose one-ulp rerun did not move the reference's exit but where an engine's exit differs
# (the int8x4 engine, more accurate than BLAS, exits at 14-16 where the reference ran to 20):
# relabelled reruns there too
G4PR_EXTRA = ('cfg4_vamp_qpsk:0/1', 'cfg4_vamp_qpsk:1/1', 'cfg4_vamp_qpsk:2/1')


def g4pr(names=None):
    """Where the reference's exit moved: eight reruns OF THE REFERENCE on the unperturbed inputs
    with the positions relabelled within every section (relabel_within_sections; seeded) — the
    identical problem with the reference's GEMM and var.mean() summation orders changed, which is
    what any other implementation of the same arithmetic (another BLAS, thread count or a GPU)
    changes.  T recorded as `T_runs_perm` (the losses of a relabelled run compare positions, so
    only T is kept); `T_span` = the span of every reference run (T_runs, T_runs_den,
    T_runs_perm)."""
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path))
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db[name]
        for key in sorted(ent['points'], key=lambda k: (int(k.split('/')[0]), float(k.split('/')[1]))):
            rec = ent['points'][key]
            extra = f'{name}:{key}' in G4PR_EXTRA
            if ('T_runs' not in rec and not extra) or 'T_runs_perm' in rec:
                continue
            seed, EbN0 = int(key.split('/')[0]), float(key.split('/')[1])
            inp = gen_inputs(cfg, seed, EbN0, svd=(algo == 'vamp'))
            assert sha(inp['x']) == rec['sha_x'] and algo == 'vamp'
            Tp = []
            for ps in PERT_SEEDS:
                Vh, x = relabel_within_sections(inp, cfg, torch.Generator().manual_seed(3000 + ps))
                L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], Vh, inp['y'], inp['SNR'], x, inp['sym'], inp['idx'])
                Tp.append(float(np.asarray(L.loss['T'])))
            rec['T_runs_perm'] = Tp
            Ts = rec.get('T_runs', [rec['T'], rec['T_pert']]) + rec.get('T_runs_den', []) + Tp
            rec['T_span'] = [min(Ts), max(Ts)]
            print(name, key, 'T runs (relabelled)', Tp, 'span', rec['T_span'], flush=True)
            with open(path, 'w') as f:
                json.dump(db, f, indent=1, sort_keys=True)


def g4(names=None):
    path = os.path.join(HERE, 'g4_curves.json')
    db = json.load(open(path)) if os.path.exists(path) else {}
    for name, (algo, Nt, Na, Nr, B, alph, iters, grid, seeds) in G4_CONFIGS.items():
        if names and name not in names:
            continue
        cfg = cfg_of(Nt, Na, Nr, B, alph, iterations=iters)
        ent = db.get(name, {'algo': algo, 'Nt': Nt, 'Na': Na, 'Nr': Nr, 'B': B, 'alphabet': alph,
                            'iterations': iters, 'points': {}})
        for seed in seeds:
            for EbN0 in grid:
                key = f'{seed}/{EbN0}'
                if key in ent['points']:
                    continue
                t0 = time.time()
                inp = gen_inputs(cfg, seed, float(EbN0), svd=(algo == 'vamp'))
                if algo == 'vamp':
                    L = ref_vamp.VAMP(cfg)(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'],
                                           inp['sym'], inp['idx'])
                elif algo == 'bamp':
                    L = ref_bamp.BAMP(cfg)(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                else:
                    L = ref_scamp.SCAMP(cfg)(inp['W'], inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'],
                                             inp['idx'])
                rec = loss_to_json(L.loss)
                rec['sha_A'] = sha(inp['A'])
                rec['sha_x'] = sha(inp['x'])
                rec['sha_sym'] = sha(np.asarray(inp['sym'], dtype=np.int64))
                rec['y_abs2_sum'] = float(np.sum(np.abs(inp['y'].numpy().astype(np.complex128)) ** 2))
                ent['points'][key] = rec
                print(name, key, 'T=', rec['T'], 'ver=', rec['ver'], 'ser=', rec['ser'],
                      f'{time.time() - t0:.1f}s', flush=True)
                db[name] = ent
                with open(path, 'w') as f:
                    json.dump(db, f, indent=1, sort_keys=True)


if __name__ == '__main__':
    which = sys.argv[1:] or ['g1', 'g2', 'g3', 'g4', 'g5', 'g6', 'g7', 'g8', 'g9']
    names = [w for w in which if w.startswith('cfg')]
    for w in which:
        if w == 'g1':
            g1()
        elif w == 'g2':
            g2()
        elif w == 'g3':
            g3()
        elif w == 'g9':
            g9()
        elif w == 'g8':
            g8()
        elif w == 'g7':
            g7()
        elif w == 'g6':
            g6(names or None)
        elif w == 'g5':
            g5()
        elif w == 'g4':
            g4(names or None)
        elif w == 'g10':
            g10()
        elif w == 'g4p':
            g4p(names or None)
        elif w == 'g4pp':
            g4pp(names or None)
        elif w == 'g4pe':
            g4pp_elem(names or None)
        elif w == 'g4pd':
            g4pp_den(names or None)
        elif w == 'g4pr':
            g4pr(names or None)
        elif w == 'g11':
            g11()
        elif w == 'g12':
            g12()
