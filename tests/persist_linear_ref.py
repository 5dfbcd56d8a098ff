"""Float64 reference, numpy yardstick and cases of the persistent VAMP engine's linear-half tests
(test_persist_linear_cpu.py, test_gpu_persist_linear.py, tools/persist_linear_err.py).  No GPU here.

One VAMP iteration's linear half (vamp.py:66-94 without the denoiser) as explicit steps, each taking
its inputs as arguments so that a phase of the kernel is judged on the kernel's own input:

  y~  = (s U^H) y                                   vamp.py:22      ytil_*
  r~  = (xmmse - dxdr r) / (1 - dxdr)               vamp.py:91      rt_*
  w   = scale (y~ + vr q) - q,  q = Vh r~           vamp.py:67-70   w_*     (GEMM1 and its epilogue)
  r   = (V w + r~ - alpha r~) / (1 - alpha)         vamp.py:72, 79  r_*     (GEMM2 and its epilogue)

`*_f64` evaluates a step in float64 / complex128 throughout (the scalars are the float32 values of
the chain, widened).  `*_c64` is the same step in the oracle's arithmetic: numpy complex64 products
and float32 elementwise operations, the lines of oracle.amp_oracle.vamp_detect with its helpers.
The c64 restatement's error against float64 on identical inputs is the yardstick of the GPU test:
no engine's deviation is ever another engine's bar.

`lmmse_scalars` / `next_scalars` are vamp_detect's float32 scalar chain (vamp.py:66, 68, 71, 73-82
and 85-94), lifted unchanged, so a chain run on the kernel's dumped var means rounds where the
reference rounds.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from oracle.amp_oracle import (C64, F32, VAR_MAX, VAR_MIN, VAR_RATIO_MAX, VAR_RATIO_MIN, _clamp, _div_real, _recip)

# amp_native.GEMM_* / ENGINE_* (restated: this module imports without the built library)
GEMM_F32, GEMM_X3, GEMM_H2, GEMM_I8 = 1, 2, 3, 4
ENGINE_PERSISTENT = 2
ARITHMETICS = {'f32': GEMM_F32, 'bf16x3': GEMM_X3, 'fp16x2': GEMM_H2, 'int8x4': GEMM_I8}

SEED, EBN0, B, ITERS = 0, 2.0, 35, 3     # workgroups of 16, 16 and 3 trials
PBM = 16                                  # trials per workgroup (amp_vamp.h)

# (Nt, Na, Nr, alphabet): every kernel instantiation and y~ path of the persistent engine
#   64, 8, 128    two-wave-group ring, the two-per-CU build; n = 2N: the y~ launch of the split forms
#   64, 8, 64     n = N: y~ by the launch GEMM, small singular values
#   64, 8, 66     n != 2N, n % 4 == 2
#   128, 4 / 16   four-wave forms at M = 32 and M = 8
#   256, 8, 512   eight-wave bf16x3 / int8x4 (A-operand and key-exchange forms), four-wave fp16x2
#   256, 8, 256   N = 256 with the launch GEMM's y~
CASES = [(64, 8, 128, '16QAM'), (64, 8, 128, 'QPSK'), (64, 8, 64, '16QAM'), (64, 8, 66, 'QPSK'),
         (128, 4, 256, '16QAM'), (128, 4, 256, 'QPSK'), (128, 16, 256, '16QAM'), (128, 16, 256, 'QPSK'),
         (256, 8, 512, '16QAM'), (256, 8, 512, 'QPSK'), (256, 8, 256, 'QPSK')]

# one B = 1 forward at the smallest and the largest N: a single valid row
B1_CASES = [(64, 8, 128, '16QAM'), (256, 8, 512, '16QAM')]

# The bars of the GPU test: an engine's error statistic over the c64 restatement's on identical
# inputs.  K_RMS: DESIGN §4 measured the worst healthy arithmetic (f32 MFMA) at 2.2x numpy's rms;
# test_persist_linear_cpu.py holds every mutant of every case at >= 2 K_RMS (the smallest ratio of
# the table is 7.6: K_RMS <= 3.8).  K_MAX is a gross-error guard only.
K_RMS, K_MAX = 3.0, 6.0


def case_id(case) -> str:
    nt, na, nr, alphabet = case
    return f'Nt{nt}-Na{na}-Nr{nr}-{alphabet}'


# ----------------------------------------------------------------------------- float64 steps
def ytil_f64(U, s, y):
    """y~ = (s U^H) y, vamp.py:22: y [B, n], U [n, k], s [k] -> [B, k] complex128."""
    U = np.asarray(U, np.complex128)
    s = np.asarray(s, np.float64)
    return np.asarray(y, np.complex128) @ (s[:, None] * np.conj(U).T).T


def rt_f64(x, r, dxdr, ns):
    """r~ = (xmmse - dxdr r) normScalar, vamp.py:91."""
    return (np.asarray(x, np.complex128) - np.float64(dxdr) * np.asarray(r, np.complex128)) * np.float64(ns)


def w_f64(rt, Vh, ytil, s2, vr, mm=None):
    """GEMM1 and its epilogue, vamp.py:67-70 and the operand of vamp.py:72: q = Vh r~,
    w = (y~ + vr q) / (s^2 + vr) - q.  rt [B, N], Vh [k, N], ytil [B, k], s2 [k] -> [B, k].
    mm(A, Bm) -> A @ Bm.T replaces the product (the mutants of the sensitivity test)."""
    rt, Vh = np.asarray(rt, np.complex128), np.asarray(Vh, np.complex128)
    q = mm(rt, Vh) if mm else rt @ Vh.T
    scale = 1.0 / (np.asarray(s2, np.float64) + np.float64(vr))
    return scale * (np.asarray(ytil, np.complex128) + np.float64(vr) * q) - q


def r_f64(w, Vh, rt, alpha, mm=None):
    """GEMM2 and its epilogue, vamp.py:72, 79: x~ = V w + r~, r = (x~ - alpha r~) / (1 - alpha).
    mm as in w_f64 (its operand is V = Vh^H, [N, k])."""
    rt, w, V = np.asarray(rt, np.complex128), np.asarray(w, np.complex128), np.conj(np.asarray(Vh, np.complex128)).T
    xt = (mm(w, V) if mm else w @ V.T) + rt
    a = np.float64(alpha)
    return (xt - a * rt) / (1.0 - a)


# ----------------------------------------------------------------------------- the oracle's arithmetic
def _mm_c64(a, bT, pad: int = 0):
    """a @ bT in complex64.  pad: `a` is zero-padded to at least `pad` rows first (the result's
    first rows are returned): numpy hands a one-row product to another BLAS routine than a matrix
    product, and that routine is no yardstick for a GEMM.  Measured at Nt = 64, B = 1 (y~): e_rms
    2.9e-8 through the row routine, 6.4e-8 for the same row inside a batch (every B > 1 forward of
    the oracle); a plain sequential float32 sum of the same row errs by 1.2e-7.  The GPU test pads a
    B = 1 batch to the kernel's own 16-row tile (its MFMA tile holds 15 zero rows beside the trial)."""
    rows = a.shape[0]
    if rows >= pad:
        return a @ bT
    ap = np.zeros((pad, a.shape[1]), dtype=a.dtype)
    ap[:rows] = a
    return (ap @ bT)[:rows]


def ytil_c64(U, s, y, pad: int = 0):
    U = np.asarray(U, C64)
    s = np.asarray(s, F32)
    Uh = np.conj(U).T
    return _mm_c64(np.asarray(y, C64), ((s[:, None] * Uh).astype(C64)).T, pad).astype(C64)   # vamp.py:22


def rt_c64(x, r, dxdr, ns):
    return ((np.asarray(x, C64) - F32(dxdr) * np.asarray(r, C64)) * F32(ns)).astype(C64)   # vamp.py:91


def w_c64(rt, Vh, ytil, s2, vr, pad: int = 0):
    """vamp_detect's lines for vamp.py:67-70 and the GEMM2 operand (xt - q) of vamp.py:72."""
    vr = F32(vr)
    s2 = np.asarray(s2, F32)
    q = _mm_c64(np.asarray(rt, C64), np.asarray(Vh, C64).T, pad).astype(C64)              # vamp.py:67
    scale = _recip(s2 + vr)                                                               # vamp.py:68
    xt = (scale * (np.asarray(ytil, C64) + vr * q)).astype(C64)                           # vamp.py:70
    return (xt - q).astype(C64)


def r_c64(w, Vh, rt, alpha, pad: int = 0):
    """vamp_detect's lines for vamp.py:72, 79."""
    rt = np.asarray(rt, C64)
    alpha = F32(alpha)
    xt = (_mm_c64(np.asarray(w, C64), np.conj(np.asarray(Vh, C64)), pad) + rt).astype(C64)   # vamp.py:72
    return _div_real(xt - alpha * rt, F32(1) - alpha)                                     # vamp.py:79


# ----------------------------------------------------------------------------- float32 scalar chain
def initial_s2t(p: float) -> float:
    """The Tracker's sigma2_tilde, a Python float (vamp.py:26)."""
    return p ** 2 * (1 - p) + (1 - p) ** 2 * p


def lmmse_scalars(s2, noise_var: float, s2t, eta: float):
    """vamp.py:66, 68, 71, 73-82 as vamp_detect evaluates them.  s2 = float32 s * s; s2t: the Python
    float of vamp.py:26 at t = 0, a float32 afterwards.  Returns vr, alpha, sigma2 and s2t32 (the
    float32 sigma2_tilde that drove the iteration: amp_status.last_scalar[0])."""
    first = isinstance(s2t, float)
    vr = F32(noise_var / s2t) if first else F32(_recip(s2t) * F32(noise_var))
    scale = _recip(s2 + vr)                                   # vamp.py:68
    varL = F32(F32(np.sum(scale, dtype=np.float64) / scale.size) * F32(noise_var))   # vamp.py:71
    if first:                                                 # vamp.py:73
        xtv = F32(F32(eta) * varL + F32((1 - eta) * s2t))
        alpha = F32(xtv / F32(s2t))                           # vamp.py:75
        s2t32 = F32(s2t)
    else:
        xtv = F32(F32(eta) * varL + F32(F32(1 - eta) * s2t))
        alpha = F32(xtv / s2t)
        s2t32 = s2t
    alpha_raw = alpha
    alpha = _clamp(alpha, VAR_RATIO_MIN, VAR_RATIO_MAX)       # vamp.py:76-77
    sigma2_raw = F32(F32(alpha / (F32(1) - alpha)) * s2t32)   # vamp.py:80
    sigma2 = _clamp(sigma2_raw, VAR_MIN, VAR_MAX)             # vamp.py:81-82
    return SimpleNamespace(vr=vr, alpha=alpha, sigma2=sigma2, s2t32=s2t32, alpha_raw=alpha_raw, sigma2_raw=sigma2_raw)


def next_scalars(mean_var, sigma2):
    """vamp.py:85-94 from var.mean() (a float32): dxdr, normScalar and the next sigma2_tilde."""
    dxdr_raw = F32(F32(mean_var) / sigma2)
    dxdr = _clamp(dxdr_raw, VAR_RATIO_MIN, VAR_RATIO_MAX)     # vamp.py:85-87
    ns = _recip(F32(1) - dxdr)                                # vamp.py:89
    s2t = _clamp(F32(F32(sigma2 * dxdr) * ns), VAR_MIN, VAR_MAX)   # vamp.py:92-94
    return SimpleNamespace(dxdr=dxdr, ns=ns, s2t=s2t, dxdr_raw=dxdr_raw)


def mean_var_f32(var) -> np.float32:
    """var.mean() as vamp_detect forms it: a float64 sum of the float32 values, then float32."""
    var = np.asarray(var, F32)
    return F32(np.sum(var, dtype=np.float64) / var.size)


def scalar_chain(s2, noise_var: float, p: float, eta: float, var_means):
    """The chain from t = 0 over the given var means (one per finished iteration): a list with one
    record per iteration t = 0 .. len(var_means), record t holding the scalars that DRIVE iteration
    t (vr, alpha, sigma2, s2t32; dxdr_prev / ns_prev of vamp.py:91, 0 and 1 at t = 0) and, where
    var_means[t] is given, the dxdr / ns / s2t it leaves."""
    out = []
    s2t = initial_s2t(p)
    dxdr_prev, ns_prev = F32(0), F32(1)
    for t in range(len(var_means) + 1):
        it = lmmse_scalars(s2, noise_var, s2t, eta)
        it.dxdr_prev, it.ns_prev = dxdr_prev, ns_prev
        it.inv_sigma2 = F32(1) / it.sigma2
        out.append(it)
        if t == len(var_means):
            break
        nx = next_scalars(var_means[t], it.sigma2)
        it.dxdr, it.ns, it.s2t_next, it.dxdr_raw = nx.dxdr, nx.ns, nx.s2t, nx.dxdr_raw
        s2t, dxdr_prev, ns_prev = nx.s2t, nx.dxdr, nx.ns
    return out


def scalar_chain_f64(s2, noise_var: float, p: float, eta: float, var_means):
    """The same chain in float64 on the same (float32) var means: the measure of how far a float32
    chain may legitimately sit from the exact one.  Returns per iteration (vr, alpha, sigma2, s2t,
    inv_sigma2) as float64."""
    s2 = np.asarray(s2, np.float64)
    out = []
    s2t = initial_s2t(p)
    for t in range(len(var_means) + 1):
        vr = noise_var / s2t
        varL = np.mean(1.0 / (s2 + vr)) * noise_var
        alpha = min(max((eta * varL + (1 - eta) * s2t) / s2t, float(VAR_RATIO_MIN)), float(VAR_RATIO_MAX))
        sigma2 = min(max(alpha / (1 - alpha) * s2t, float(VAR_MIN)), float(VAR_MAX))
        out.append(SimpleNamespace(vr=vr, alpha=alpha, sigma2=sigma2, s2t32=s2t, inv_sigma2=1.0 / sigma2))
        if t == len(var_means):
            break
        dxdr = min(max(float(var_means[t]) / sigma2, float(VAR_RATIO_MIN)), float(VAR_RATIO_MAX))
        out[-1].dxdr = dxdr
        s2t = min(max(sigma2 * dxdr / (1 - dxdr), float(VAR_MIN)), float(VAR_MAX))
    return out


# ----------------------------------------------------------------------------- statistics
def stats(z, z64):
    """DESIGN §4's metric over the given (valid) rows: (e_max, e_rms) =
    (max, rms)|z - z64| / max|z64|."""
    z64 = np.asarray(z64, np.complex128)
    d = np.abs(np.asarray(z, np.complex128) - z64) / np.abs(z64).max()
    return float(d.max()), float(np.sqrt((d ** 2).mean()))


def ratios(got, yard, ref):
    """(e_max ratio, e_rms ratio, got's (e_max, e_rms), yardstick's) of `got` against the c64
    restatement `yard`, both measured against the float64 value `ref`."""
    g, y = stats(got, ref), stats(yard, ref)
    return g[0] / y[0], g[1] / y[1], g, y


# ----------------------------------------------------------------------------- mutants (sensitivity)
def round_sig(a, bits: int):
    """Complex / real array with every component rounded to `bits` significand bits (the implicit
    one counted): bits = 16 is an operand that lost the third bf16 plane of a bf16x3 split."""
    def rnd(v):
        v = np.asarray(v, np.float64)
        m, e = np.frexp(v)
        return np.ldexp(np.round(np.ldexp(m, bits)), e - bits)
    a = np.asarray(a)
    return rnd(a.real) + 1j * rnd(a.imag) if np.iscomplexobj(a) else rnd(a)


def x3_planes(a):
    """The three bf16 pieces (b0, b1, b2) of a float32 array (tests/x3_split_ref.split_raw), float64."""
    import torch
    import x3_split_ref as xs
    b = xs.split_raw(torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)))
    return [p.numpy().astype(np.float64) for p in b[:3]]


def cross_sign_product(A, Bm):
    """A @ Bm.T for complex A [B, K], Bm [O, K] with the operand Bm held as bf16x3 planes and ONE
    imaginary cross term of the low plane mis-signed: Im(out) takes - A.re * Bm.im(low) where the
    product has + (a complex product's Im is a.re b.im + a.im b.re; this term also acts at t = 0,
    where r~ is real).  Everything else exact."""
    A = np.asarray(A, np.complex128)
    re, im = x3_planes(np.asarray(Bm).real), x3_planes(np.asarray(Bm).imag)
    exact = A @ ((re[0] + re[1] + re[2]) + 1j * (im[0] + im[1] + im[2])).T
    return exact - 2.0j * (A.real @ im[2].T)


# ----------------------------------------------------------------------------- inputs and the oracle's trace
def make_config(case, batch: int = B, iterations: int = ITERS, device: str = 'cuda'):
    from config import Config
    nt, na, nr, alphabet = case
    return Config(nt, na, nr, 1, 1, batch=batch, generator_mode='sparc', iterations=iterations, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', device=device)


_INPUTS = {}


def inputs(case, batch: int = B):
    """Host tensors and numpy arrays of the case's operating point (seed 0, EbN0 = 2 dB) from the
    repository's generators in the reference's call order; built once per case, left unchanged."""
    key = (case, batch)
    if key not in _INPUTS:
        from test_gpu_vamp import _regen_inputs
        inp = _regen_inputs(make_config(case, batch, device='cpu'), SEED, EBN0)
        c = lambda t: t.numpy()[..., 0] if t.dim() == 3 else t.numpy()   # noqa: E731
        _INPUTS[key] = SimpleNamespace(t={k: inp[k] for k in ('U', 's', 'Vh', 'y')}, SNR=float(inp['SNR']),
                                       U=c(inp['U']), s=c(inp['s']), Vh=c(inp['Vh']), y=c(inp['y']))
    return _INPUTS[key]


def problem(case, inp):
    """The constants of a case's forward: p, eta, noise_var and s^2 (float32 and exact)."""
    nt, na, nr, _ = case
    s = np.asarray(inp.s, F32)
    return SimpleNamespace(p=na / nt, eta=s.shape[0] / inp.Vh.shape[1], noise_var=(na / nr) / inp.SNR,
                           s2=(s * s).astype(F32), s2_64=s.astype(np.float64) ** 2)


_TRACES = {}


def oracle_trace(case, batch: int = B):
    """vamp_detect's trace of the case (ITERS iterations), computed once."""
    key = (case, batch)
    if key not in _TRACES:
        import oracle.amp_oracle as O
        nt, na, nr, alphabet = case
        inp = inputs(case, batch)
        ocfg = O.OracleConfig(nt, na, nr, B=batch, alphabet=alphabet, iterations=ITERS)
        tr = []
        out = O.vamp_detect(inp.U, inp.s, inp.Vh, inp.y, inp.SNR, ocfg, trace=tr)
        _TRACES[key] = (out, tr)
    return _TRACES[key]
