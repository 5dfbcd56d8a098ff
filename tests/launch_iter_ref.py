"""Float64 reference, numpy yardstick, cases and statistics of the per-iteration BAMP / SCAMP tests
(test_launch_iter_cpu.py, test_gpu_bamp_iter.py, test_gpu_scamp_iter.py,
test_gpu_scamp_persist_iter.py, tools/launch_iter_err.py).  numpy only, no GPU here.

The engines expose xmap, xmmse and var (BAMP) or psi (SCAMP), not z.  A float64 trajectory beside the
kernel's would part from it through the denoiser, so every nonlinear quantity is fed back from the
engine and only the linear residual recursion is carried here.  The state after iteration t is the
output of a forward with `iterations = t` (t = 1 .. T on the same inputs); step t then is

  BAMP (bamp.py:59-64, oracle.bamp_detect)          SCAMP (scamp.py:45-57, oracle.scamp_detect)
    v     = var_{t-1} |H|^2^T                         gma   = psi_{t-1} W^T / Lin
    z_t   = xm_{t-1} H^T - v (y - z_{t-1}) / u_{t-1}  b     = gma / phi_{t-1}
    u_t   = v + sigma2                                z_t   = y - xm_{t-1} A^T + b z_{t-1}
    cov   = 1 / ((1 / u_t) |H|^2)                     phi_t = sigma2 + gma
    xmap  = xm_{t-1} + cov (((y - z_t) / u_t) H^*)    tau   = L / (Mr ((1 / phi_t) W))
                                                      xmap  = xm_{t-1} + tau ((z_t / phi_t) A^*)

with xm_{t-1}, var_{t-1} / psi_{t-1} the ENGINE's outputs, z the step's own (z_0 = y) and u / phi the
step's own too (they are functions of the engine's var_{t-2} / psi_{t-2}).  `*_step_f64` evaluates this in
float64 / complex128; `*_step_c64` is the same step in the oracle's arithmetic (its lines, lifted),
carrying its own complex64 z.  The c64 step's error against float64 on identical inputs is the
yardstick of the GPU tests: an engine's statistic may be K_RMS / K_MAX (persist_linear_ref.py) times
the yardstick's, no more.  The denoiser half (xmmse, var from the engine's own xmap with the float64
cov / 2 or tau / 2) is held to persist_denoiser_cases.xtol / VAR_RTOL.
"""
from __future__ import annotations

from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from oracle.amp_oracle import C64, F32, _div_real, _logits, _recip, _torch_abs, allclose_f32
from persist_denoiser_cases import VAR_RTOL, denoise_f64, xtol
from persist_linear_ref import K_MAX, K_RMS, _mm_c64, round_sig  # noqa: F401  (the project's bars, by import)

# amp_native.GEMM_* / ENGINE_* (restated: this module imports without the built library)
GEMM_F32, GEMM_X3, GEMM_H2 = 1, 2, 3
ENGINE_LAUNCHES, ENGINE_PERSISTENT = 1, 2
ARITH_NAMES = {GEMM_F32: 'f32', GEMM_X3: 'bf16x3', GEMM_H2: 'fp16x2'}

SEED, T = 0, 4
PAD = 16            # rows of the yardstick's products at B = 1 (persist_linear_ref._mm_c64)
BLOCK = (32, 64)    # rows x complex columns of the block statistic: a row tile x a 128-float column tile

Case = namedtuple('Case', 'Nt Na Nr Lin Lh B alphabet ebn0 band', defaults=(False,))

# BAMP, launch engine
#   6,3,5,3,1      N = 18: N % 4 == 2 through the pair loader; n = 15 odd (padded s / invu strides)
#   48,6,12,2,2    N = 96: column tiles of 128 + 64 floats, the last partial; B = 1: one valid row
#   32,4,32,4,2    banded ISI, two and three column tiles; 16QAM: the product-grid denoiser
#   64,4,32,8,3    N = 512, n = 320: several reduction chunks, banded, B = 35 a partial 32-row tile;
#                  both multiples of 64: the bf16x3 and fp16x2 tiles run here
#   168,84,73,3,2  M = 2, 2N = 1008
#   band=True      the (32,4,32,4,2) channel with ONE nonzero entry far outside the band (f32 tiles:
#                  n = 160 is no multiple of 64), and the same on the (64,4,32,8,3) channel, where the
#                  bf16x3 / fp16x2 tiles form their band ranges too
BAMP_CASES = [Case(6, 3, 5, 3, 1, 48, 'OOK', 8.0), Case(48, 6, 12, 2, 2, 48, 'OOK', 8.0),
              Case(32, 4, 32, 4, 2, 64, 'QPSK', 4.0), Case(32, 4, 32, 4, 2, 64, '16QAM', 6.0),
              Case(64, 4, 32, 8, 3, 35, 'QPSK', 6.0), Case(168, 84, 73, 3, 2, 48, '8PSK', 11.0),
              Case(48, 6, 12, 2, 2, 1, 'OOK', 8.0), Case(32, 4, 32, 4, 2, 64, 'QPSK', 4.0, True),
              Case(64, 4, 32, 8, 3, 35, 'QPSK', 6.0, True)]
# SCAMP, launch engine: the same ISI, odd and partial-tile shapes, and a coupling block wider than
# a column tile (Nt = 192 > 128)
SCAMP_CASES = [Case(6, 3, 5, 3, 1, 48, 'OOK', 8.0), Case(48, 6, 12, 2, 2, 48, 'OOK', 8.0),
               Case(32, 4, 32, 4, 2, 64, 'QPSK', 4.0), Case(32, 4, 32, 4, 2, 64, '16QAM', 0.0),
               Case(64, 4, 32, 8, 3, 35, 'QPSK', 6.0), Case(192, 12, 24, 3, 2, 48, 'QPSK', 6.0),
               Case(48, 6, 12, 2, 2, 1, 'OOK', 8.0)]
# SCAMP, persistent engine: its three shapes (2N, 2n) = (128, 256), (256, 512), (256, 256); B = 35
# (workgroups of 16, 16 and 3 trials) and B = 1
PERSIST_SHAPES = [(64, 8, 128), (128, 8, 256), (128, 8, 128)]
PERSIST_EBN0 = {'QPSK': 2.0, '16QAM': 0.0}
PERSIST_CASES = [Case(nt, na, nr, 1, 1, b, alph, PERSIST_EBN0[alph]) for nt, na, nr in PERSIST_SHAPES
                 for alph in ('QPSK', '16QAM') for b in (35, 1)]
# early exit: the g11 isi3 shape at 10 dB (the launch engines) and the persistent engine's cfg3 shape
EXIT_CASE = Case(64, 4, 32, 8, 3, 32, 'QPSK', 10.0)
EXIT_CASE_PERSIST = Case(128, 8, 256, 1, 1, 35, 'QPSK', 8.0)
EXIT_ITERS = 20


def split_shape(case) -> bool:
    """amp_bamp.h bamp_h2_shape / amp_scamp.h scamp_lx3_shape: the launch engines' split tiles."""
    return (case.Nt * case.Lin) % 64 == 0 and (case.Nr * (case.Lin + case.Lh - 1)) % 64 == 0


def bamp_arithmetics(case):
    return (GEMM_F32, GEMM_X3, GEMM_H2) if split_shape(case) else (GEMM_F32,)


def scamp_arithmetics(case):
    return (GEMM_F32, GEMM_X3) if split_shape(case) else (GEMM_F32,)


def case_id(case) -> str:
    return (f'Nt{case.Nt}-Na{case.Na}-Nr{case.Nr}-Lin{case.Lin}-Lh{case.Lh}-B{case.B}-{case.alphabet}-'
            f'{case.ebn0:g}dB' + ('-offband' if case.band else ''))


# ----------------------------------------------------------------------------- inputs
def make_config(case, iterations: int = T, device: str = 'cuda'):
    from config import Config
    return Config(case.Nt, case.Na, case.Nr, case.Lin, case.Lh, batch=case.B, generator_mode='sparc',
                  iterations=iterations, alphabet=case.alphabet, channel_profile='uniform', channel_truncation='tail',
                  device=device)


def oracle_config(case, iterations: int = T):
    from oracle import OracleConfig
    return OracleConfig(case.Nt, case.Na, case.Nr, Lin=case.Lin, Lh=case.Lh, B=case.B, alphabet=case.alphabet,
                        iterations=iterations)


def off_band_entry(case):
    """(row, column, value) of the band case's extra entry: the last output row (lo = Lout - 1) in
    the first input column (li = 0), Lout - 1 >= Lh blocks below the band."""
    assert case.Lin + case.Lh - 2 >= case.Lh
    return case.Nr * (case.Lin + case.Lh - 1) - 1, 0, np.complex64(0.25 - 0.125j)


_INPUTS = {}


def inputs(case):
    """W, A, y and the noise variance of the case (seed 0) from the repository's generators in the
    reference's call order (isi_inputs.isi_inputs); built once per case, left unchanged.  The band
    case adds its entry to A and the entry's contribution to y."""
    if case not in _INPUTS:
        import torch
        from channel import Channel
        from data import Data
        cfg = make_config(case, device='cpu')
        np.random.seed(SEED)
        torch.manual_seed(SEED)
        ch, da = Channel(cfg), Data(cfg)
        W, A = ch.generate_as_sparc()
        x, _, _ = da.generate_message()
        SNR = cfg.snr(case.ebn0)
        y = A @ x + ch.awgn(SNR)
        if case.band:
            i, j, val = off_band_entry(case)
            assert A[i, j] == 0
            A = A.clone()
            A[i, j] = complex(val)
            y = y.clone()
            y[:, i] += complex(val) * x[:, j]
        An, yn = A.numpy().astype(C64), y.numpy()[..., 0].astype(C64)
        _INPUTS[case] = SimpleNamespace(t=dict(W=W, A=A, y=y), SNR=float(SNR), W=W.numpy().astype(F32), A=An, y=yn,
                                        noise_var=(case.Na / case.Nr) / float(SNR))
    return _INPUTS[case]


# ----------------------------------------------------------------------------- mutants' operands
def drop_band_granule(H, cols: int = 64, gran: int = 32):
    """H with the last `gran` rows of the first `cols` columns' nonzero row range zeroed: the A^H
    product's first column tile with a band end one granule of 64 reduction floats short."""
    H = np.array(H, copy=True)
    rows = np.nonzero(np.abs(H[:, :cols]).sum(axis=1))[0]
    ke = int(rows.max()) + 1
    assert ke - gran >= int(rows.min())
    H[ke - gran:ke, :cols] = 0
    return H


def _rep(a, k):
    return np.repeat(a, k, axis=1)


# ----------------------------------------------------------------------------- BAMP
BAMP_MUTANTS = ('h16', 'onsager', 'lastcol', 'granule', 'offband')


def bamp_state(y, dtype):
    """The Tracker's z = y; u = None stands for the scalar sigma2 of bamp.py:25."""
    return SimpleNamespace(z=np.asarray(y, dtype), u=None)


def bamp_step_f64(H, y, sigma2, xm, var, st, mut=None, case=None):
    """One BAMPLayer.forward without the denoiser, float64.  xm [B, N], var [B, N]: the engine's
    outputs of the iteration before (0 and 1 at the first); st: bamp_state / the last step's
    result.  sigma2 is the float32 value every implementation rounds to, widened.  mut: a defect
    (the sensitivity test): 'h16' H rounded to 16 significand bits, 'onsager' the Onsager term
    divided by the new u, 'lastcol' the last column of |H|^2 missing from the v product, 'granule'
    drop_band_granule in the H^H product, 'offband' the band case's extra entry ignored."""
    H = np.asarray(H, np.complex128)
    y = np.asarray(y, np.complex128)
    s2 = np.float64(F32(sigma2))
    if mut == 'h16':
        H = round_sig(H, 16)
    if mut == 'offband':
        i, j, _ = off_band_entry(case)
        H = H.copy()
        H[i, j] = 0
    abs2 = np.abs(H) ** 2
    abs2v = abs2
    if mut == 'lastcol':
        abs2v = abs2.copy()
        abs2v[:, -1] = 0
    Hg = drop_band_granule(H) if mut == 'granule' else H
    xm, var = np.asarray(xm, np.complex128), np.asarray(var, np.float64)
    v = var @ abs2v.T                                             # bamp.py:59
    u = v + s2                                                    # bamp.py:61
    ud = u if mut == 'onsager' else (s2 if st.u is None else st.u)
    z = xm @ H.T - v * (y - st.z) / ud                            # bamp.py:60
    cov = 1.0 / ((1.0 / u) @ abs2)                                # bamp.py:62
    xmap = xm + cov * (((y - z) / u) @ np.conj(Hg))               # bamp.py:63
    return SimpleNamespace(xmap=xmap, cov=cov, z=z, u=u)


def bamp_step_c64(H, y, sigma2, xm, var, st, pad: int = 0):
    """The same step as oracle.bamp_detect writes it (complex64 / float32 products)."""
    H, y = np.asarray(H, C64), np.asarray(y, C64)
    xm, var = np.asarray(xm, C64), np.asarray(var, F32)
    Hc = np.conj(H)
    abs2 = (_torch_abs(H) ** 2).astype(F32)                        # bamp.py:18
    v = _mm_c64(var, abs2.T, pad).astype(F32)                      # bamp.py:59
    res = (y - st.z).astype(C64)
    ud = F32(sigma2) if st.u is None else st.u
    z = (_mm_c64(xm, H.T, pad) - _div_real((v * res).astype(C64), ud)).astype(C64)     # bamp.py:60
    u = (v + F32(sigma2)).astype(F32)                              # bamp.py:61
    cov = _recip(_mm_c64(_recip(u), abs2, pad).astype(F32))        # bamp.py:62
    g = _mm_c64(_div_real((y - z).astype(C64), u), Hc, pad).astype(C64)   # bamp.py:63
    xmap = (xm + cov * g).astype(C64)
    return SimpleNamespace(xmap=xmap, cov=cov, z=z, u=u)


# ----------------------------------------------------------------------------- SCAMP
SCAMP_MUTANTS = ('h16', 'onsager', 'granule', 'tau1e5')


def scamp_state(y, dtype):
    """The Tracker's z = y; phi = None stands for the +inf of scamp.py:22 (b = 0)."""
    return SimpleNamespace(z=np.asarray(y, dtype), phi=None)


def scamp_step_f64(W, A, y, sigma2, case, xm, psi, st, mut=None):
    """One SCAMPLayer.forward without the denoiser, float64.  xm [B, N], psi [B, Lin]: the engine's
    outputs of the iteration before (0 and 1 at the first).  mut: 'h16' A rounded to 16 bits,
    'onsager' b = gma / phi with the new phi, 'granule' drop_band_granule in the A^H product,
    'tau1e5' the first coupling block's tau off by 1e-5."""
    A = np.asarray(A, np.complex128)
    W = np.asarray(W, np.float64)
    y = np.asarray(y, np.complex128)
    s2 = np.float64(F32(sigma2))
    Mr, Mc, Lc, L = case.Nr, case.Nt, case.Lin, case.Na * case.Lin
    if mut == 'h16':
        A = round_sig(A, 16)
    Ag = drop_band_granule(A) if mut == 'granule' else A
    xm, psi = np.asarray(xm, np.complex128), np.asarray(psi, np.float64)
    gma = psi @ W.T / Lc                                          # scamp.py:45
    phi = s2 + gma                                                # scamp.py:51
    pd = phi if mut == 'onsager' else st.phi
    b = np.zeros_like(gma) if pd is None else gma / pd            # scamp.py:47
    z = y - xm @ A.T + _rep(b, Mr) * st.z                         # scamp.py:49
    tau = L / (Mr * ((1.0 / phi) @ W))                            # scamp.py:53
    if mut == 'tau1e5':
        tau = tau.copy()
        tau[:, 0] *= 1.0 + 1e-5
    xmap = xm + _rep(tau, Mc) * ((z / _rep(phi, Mr)) @ np.conj(Ag))   # scamp.py:57
    return SimpleNamespace(xmap=xmap, tau=_rep(tau, Mc), z=z, phi=phi)


def scamp_step_c64(W, A, y, sigma2, case, xm, psi, st, pad: int = 0):
    """The same step as oracle.scamp_detect writes it."""
    W, A, y = np.asarray(W, F32), np.asarray(A, C64), np.asarray(y, C64)
    xm, psi = np.asarray(xm, C64), np.asarray(psi, F32)
    Mr, Mc, Lc, L = case.Nr, case.Nt, case.Lin, case.Na * case.Lin
    Ac = np.conj(A)
    phi0 = np.full((y.shape[0], W.shape[0]), np.inf, F32) if st.phi is None else st.phi
    gma = ((psi @ W.T).astype(F32) / F32(Lc)).astype(F32)         # scamp.py:45
    b = (gma / phi0).astype(F32)                                  # scamp.py:47
    z = (y - _mm_c64(xm, A.T, pad).astype(C64) + _rep(b, Mr) * st.z).astype(C64)   # scamp.py:49
    phi = (F32(sigma2) + gma).astype(F32)                         # scamp.py:51
    tau = ((_recip((_recip(phi) @ W).astype(F32)) * F32(L)) / F32(Mr)).astype(F32)   # scamp.py:53
    tau_use = _rep(tau, Mc)                                       # scamp.py:54
    g = _mm_c64(_div_real(z, _rep(phi, Mr)), Ac, pad).astype(C64)
    xmap = (xm + tau_use * g).astype(C64)                         # scamp.py:57
    return SimpleNamespace(xmap=xmap, tau=tau_use, z=z, phi=phi)


def psi_f64(xm, case):
    """scamp.py:59 in float64: (psi, the subtracted sum sum |xm|^2 / Na), both [B, Lin]."""
    xm = np.asarray(xm, np.complex128)
    s = (np.abs(xm) ** 2).reshape(xm.shape[0], case.Lin, case.Nt).sum(axis=-1) / case.Na
    return 1.0 - s, s


def psi_c64(xm, case):
    """scamp.py:59 as oracle.scamp_detect writes it."""
    xm = np.asarray(xm, C64)
    return (F32(1) - (_torch_abs(xm) ** 2).reshape(xm.shape[0], case.Lin, case.Nt).sum(axis=-1) / F32(case.Na)).astype(F32)


# ----------------------------------------------------------------------------- statistics
def psi_yardstick(xm, case, pad: int = 0):
    """The normalised errors (psi_errors) of the oracle's float32 psi line on xm.  A batch of fewer
    than `pad` rows is filled up to it with seeded permutations of the rows' positions inside every
    coupling block: the same sums in other float32 summation orders."""
    xm = np.asarray(xm, C64)
    rows = xm.shape[0]
    if rows < pad:
        rng = np.random.default_rng(SEED)
        x = xm.reshape(rows, case.Lin, case.Nt)
        reps = [x] + [x[:, :, rng.permutation(case.Nt)] for _ in range(-(-pad // rows) - 1)]
        xm = np.concatenate(reps).reshape(-1, case.Lin * case.Nt)
    p64, sub = psi_f64(xm, case)
    return psi_errors(psi_c64(xm, case), p64, sub)


def _rms(a):
    return float(np.sqrt(np.mean(np.abs(a) ** 2)))


def xstats(z, ref):
    """(rms, max, blk) of |z - ref| over the rms of ref; blk: the worst rms over BLOCK-sized blocks
    of rows x complex columns, so that a defect confined to an edge tile is not averaged away."""
    ref = np.asarray(ref, np.complex128)
    d = np.abs(np.asarray(z, np.complex128) - ref)
    s = _rms(ref)
    blk = max(_rms(d[i:i + BLOCK[0], j:j + BLOCK[1]]) for i in range(0, d.shape[0], BLOCK[0])
              for j in range(0, d.shape[1], BLOCK[1]))
    return SimpleNamespace(rms=_rms(d) / s, max=float(d.max()) / s, blk=blk / s)


def psi_errors(psi, ref, sub):
    """|psi - ref| over the rms of the subtracted sum (psi itself goes to 0), per value."""
    return (np.abs(np.asarray(psi, np.float64) - ref) / _rms(sub)).ravel()


def psi_stats(errs):
    """(rms, max) of psi_errors; one value per trial and coupling block: there are no blocks."""
    return SimpleNamespace(rms=_rms(errs), max=float(np.max(errs)), blk=_rms(errs))


def _ratio(g, y):
    return g / y if y > 0 else (0.0 if g == 0 else float('inf'))


def record(what, t, got, yard):
    """An engine's statistics, the yardstick's, and their ratios."""
    return SimpleNamespace(what=what, t=t, got=got, yard=yard, rms=_ratio(got.rms, yard.rms),
                           max=_ratio(got.max, yard.max), blk=_ratio(got.blk, yard.blk))


def linear_ok(r) -> bool:
    return r.rms <= K_RMS and r.blk <= K_RMS and r.max <= K_MAX


def denoiser_record(what, t, x, var, ref):
    """The float32-logit denoiser's bars (persist_denoiser_cases): |x - ref| <= xtol(max |xi|),
    |var - ref| <= VAR_RTOL |ref| + the same term; x / var as fractions of their bars."""
    tol = xtol(ref.max_abs_xi)
    fx = float(np.abs(np.asarray(x, np.complex128) - ref.x).max()) / tol
    fv = None
    if var is not None:
        fv = float((np.abs(np.asarray(var, np.float64) - ref.var) / (VAR_RTOL * np.abs(ref.var) + tol)).max())
    return SimpleNamespace(what=what, t=t, x=fx, var=fv, tol=tol, max_abs_xi=ref.max_abs_xi)


def denoiser_ok(r) -> bool:
    return r.x <= 1.0 and (r.var is None or r.var <= 1.0)


# ----------------------------------------------------------------------------- a forward's records
def bamp_records(case, outs, pad: int = PAD):
    """outs[t - 1] = (xmap, xmmse, var) after iteration t (the outputs of a forward of t iterations),
    t = 1 .. len(outs).  Returns (linear records, denoiser records)."""
    inp = inputs(case)
    sym = oracle_config(case).symbols
    L, M = case.Na * case.Lin, case.Nt // case.Na
    B, N = inp.y.shape[0], inp.A.shape[1]
    xm, var = np.zeros((B, N), C64), np.ones((B, N), F32)
    s64, s32 = bamp_state(inp.y, np.complex128), bamp_state(inp.y, C64)
    lin, den = [], []
    for t, (xmap, xmmse, var_t) in enumerate(outs, 1):
        s64 = bamp_step_f64(inp.A, inp.y, inp.noise_var, xm, var, s64)
        s32 = bamp_step_c64(inp.A, inp.y, inp.noise_var, xm, var, s32, pad)
        lin.append(record('xmap', t, xstats(xmap, s64.xmap), xstats(s32.xmap, s64.xmap)))
        ref = denoise_f64(xmap, s64.cov / 2.0, sym, L, M)         # the engine's own xmap
        den.append(denoiser_record('xmmse/var', t, xmmse, var_t, ref))
        xm, var = xmmse, var_t
    return lin, den


def scamp_records(case, outs, pad: int = PAD):
    """outs[t - 1] = (xmap, xmmse, psi) after iteration t.  Returns (linear records: xmap and psi
    from the engine's own xmmse, denoiser records).

    psi holds B Lin values per iteration.  Below `pad` of them an iteration's rms is no rms: at
    B = 1, Lin = 1 psi is ONE float32 value, and the ratio of two single rounding errors says
    nothing (persistent engine, fp16x2, Nt 128 / Nr 256, 16QAM, iteration 2: the engine's psi is
    6.5e-8 off, one ulp of the sum, where numpy's single value happened to land 4.9e-9 from the
    exact one: 13.3x).  Such a forward gets ONE psi record (t = 0) over all its iterations, against
    the oracle's line on the same rows in `pad` summation orders (psi_yardstick); measured that way
    the same forward reads 1.17x."""
    inp = inputs(case)
    sym = oracle_config(case).symbols
    L, M = case.Na * case.Lin, case.Nt // case.Na
    B, N = inp.y.shape[0], inp.A.shape[1]
    xm, psi = np.zeros((B, N), C64), np.ones((B, case.Lin), F32)
    s64, s32 = scamp_state(inp.y, np.complex128), scamp_state(inp.y, C64)
    lin, den = [], []
    pooled = B * case.Lin < pad
    eg, ey = [], []
    for t, (xmap, xmmse, psi_t) in enumerate(outs, 1):
        s64 = scamp_step_f64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, psi, s64)
        s32 = scamp_step_c64(inp.W, inp.A, inp.y, inp.noise_var, case, xm, psi, s32, pad)
        lin.append(record('xmap', t, xstats(xmap, s64.xmap), xstats(s32.xmap, s64.xmap)))
        ref = denoise_f64(xmap, s64.tau / 2.0, sym, L, M)
        den.append(denoiser_record('xmmse', t, xmmse, None, ref))
        p64, sub = psi_f64(xmmse, case)
        eg.append(psi_errors(psi_t, p64, sub))
        ey.append(psi_yardstick(xmmse, case, pad))
        if not pooled:
            lin.append(record('psi', t, psi_stats(eg[-1]), psi_stats(ey[-1])))
        xm, psi = xmmse, psi_t
    if pooled:
        lin.append(record('psi', 0, psi_stats(np.concatenate(eg)), psi_stats(np.concatenate(ey))))
    return lin, den


def show(who, lin, den):
    for r in lin:
        print(f'{who} {r.what:5s} t={r.t}: rms {r.got.rms:.3e} (numpy {r.yard.rms:.3e}, x{r.rms:.2f})  '
              f'max {r.got.max:.3e} (numpy {r.yard.max:.3e}, x{r.max:.2f})  block x{r.blk:.2f}')
    for r in den:
        v = '' if r.var is None else f'  var {r.var:.3f}'
        print(f'{who} {r.what:5s} t={r.t}: fraction of the bar: x {r.x:.3f}{v}  (max|xi| {r.max_abs_xi:.1f})')


def assert_bars(who, lin, den):
    bad = [f'{r.what} t={r.t} rms x{r.rms:.2f} block x{r.blk:.2f} max x{r.max:.2f}' for r in lin if not linear_ok(r)]
    bad += [f'{r.what} t={r.t} x {r.x:.2f} var {r.var}' for r in den if not denoiser_ok(r)]
    assert not bad, f'{who}: ' + '; '.join(bad)


# ----------------------------------------------------------------------------- the oracle standing in
_TRACES = {}


def oracle_trace(case, algo: str, iterations: int = T):
    """(result, trace) of oracle.bamp_detect / scamp_detect on the case, computed once."""
    key = (case, algo, iterations)
    if key not in _TRACES:
        import oracle.amp_oracle as O
        inp = inputs(case)
        tr = []
        if algo == 'bamp':
            out = O.bamp_detect(inp.A, inp.y, inp.SNR, oracle_config(case, iterations), trace=tr)
        else:
            out = O.scamp_detect(inp.W, inp.A, inp.y, inp.SNR, oracle_config(case, iterations), trace=tr)
        _TRACES[key] = (out, tr)
    return _TRACES[key]


def normalisers_ok(xmap, tau, case) -> bool:
    """Every section's normaliser of the oracle's float64 denoiser (the batch-global max |xi| shift,
    vamp.py:112) is finite and positive: the engines' exact-float64 section path is not entered."""
    cfg = oracle_config(case)
    xi = _logits(np.asarray(xmap, C64), np.asarray(tau, F32), cfg, xmap.shape[0])
    with np.errstate(under='ignore'):
        z = np.exp(xi - np.abs(xi).max()).sum(axis=-1).sum(axis=2)
    return bool(np.all(np.isfinite(z) & (z > 0)))


def first_close(seq, start):
    """The first t (from 1) at which allclose_f32(seq[t - 1], its predecessor) holds, or None."""
    prev = start
    for t, cur in enumerate(seq, 1):
        if allclose_f32(np.asarray(cur, F32), np.asarray(prev, F32)):
            return t
        prev = cur
    return None
