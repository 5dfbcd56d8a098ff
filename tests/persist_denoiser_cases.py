"""Cases and the float64 reference of the persistent VAMP engine's denoiser tests
(test_persist_denoiser_cpu.py, test_gpu_persist_denoiser.py).  No GPU needed here.

The section denoiser of csrc/amp_denoise.h has about twenty code paths, selected by the
constellation size KK, the section size M (lane group G), the sections in flight U, the packing
policy PK_ALL / PK_GRID / PK_NONE, the product-grid pattern GRID_FULL / GRID_REF16 and FAST.
`expected_form` restates that dispatch (denoise_sections_u -> _sel -> _grid / _gp / _g, and
vamp_persist's PKDEN / DENFAST / persist_launch_nt's DU) so that every test names the path it runs.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

# amp_native.GEMM_* / ENGINE_* (restated: this module imports without the built library)
GEMM_F32, GEMM_X3 = 1, 2
ENGINE_PERSISTENT = 2
AMP_E_ARG = -1

PK_NONE, PK_ALL, PK_GRID = 'PK_NONE', 'PK_ALL', 'PK_GRID'

# class -> (gemm, Nt, waves per workgroup, workgroups per CU the build is bounded for)
#   x3_n64    bf16x3, four waves, the two-per-CU build (OCC = 2: two waves per SIMD)  -> PK_NONE
#   x3_n128   bf16x3, four waves, one per CU                                          -> PK_ALL
#   x3_n256   bf16x3, eight waves (two per SIMD) -> PK_GRID + FAST for KK = 16, else PK_NONE
#   f32_n64 / f32_n256   f32 MFMA, four waves, one per CU -> PK_ALL, other column tilings (NT)
CLASSES = {
    'x3_n64': (GEMM_X3, 64, 4, 2),
    'x3_n128': (GEMM_X3, 128, 4, 1),
    'x3_n256': (GEMM_X3, 256, 8, 1),
    'f32_n64': (GEMM_F32, 64, 4, 1),
    'f32_n256': (GEMM_F32, 256, 4, 1),
}
ALPHABETS = ('OOK', 'BPSK', '4ASK', 'QPSK', 'sq4', '8PSK', '16PSK', '16QAM', 'sq16', 'sq64')
SECTION_SIZES = (2, 4, 8, 16, 32, 64)
B = 35            # workgroups of 16, 16 and 3 trials
SEED, EBN0, ITERS = 0, 8.0, 3
PBM = 16          # trials per workgroup (amp_vamp.h)

AMP_DANGER = -700.0   # amp_common.h


def logit_slack(G: float) -> float:
    """amp_common.h logit_slack."""
    return 1e-5 * abs(G) + 2.0


def alphabet_size(alphabet: str) -> int:
    return {'OOK': 1, 'BPSK': 2, '4ASK': 4, 'QPSK': 4, 'sq4': 4, '8PSK': 8, '16PSK': 16, '16QAM': 16, 'sq16': 16,
            'sq64': 64}[alphabet]


def grid_of(alphabet: str):
    """(R, pattern) of amp_host.h grid_decompose, or None: the alphabets whose float32 points fill
    an R x R grid with K = R^2 (QPSK {1, j, -1, -j} has three values per axis; the PSKs and the
    real alphabets are no grids)."""
    return {'sq4': (2, 'FULL'), '16QAM': (4, 'REF16'), 'sq16': (4, 'FULL'), 'sq64': (8, 'FULL')}.get(alphabet)


def packing(cls: str, alphabet: str) -> str:
    """vamp_persist's PKDEN."""
    _, _, nwv, occ = CLASSES[cls]
    if occ * nwv // 4 == 1:
        return PK_ALL
    return PK_GRID if (nwv == 8 and alphabet_size(alphabet) == 16) else PK_NONE


def sections_in_flight(alphabet: str) -> int:
    """persist_launch_nt's DU (AMP_KK4_DU = 4, AMP_X3_DU = 2)."""
    return {1: 4, 2: 4, 4: 4, 8: 2, 16: 2, 64: 1}[alphabet_size(alphabet)]


def expected_form(cls: str, alphabet: str) -> str:
    """The amp_denoise.h path vamp_persist's denoiser call takes for this kernel class and alphabet
    (the same for every M: M only picks the lane group size G)."""
    kk, u, pk, grid = alphabet_size(alphabet), sections_in_flight(alphabet), packing(cls, alphabet), grid_of(alphabet)
    if kk > 16:     # denoise_sections_wide_m: the grid loop at U = 1, else the streamed per-point form
        return f'wide/grid/R{grid[0]}' if grid else 'wide'
    if grid:        # denoise_sections_grid
        r, pat = grid
        packed = pk in (PK_ALL, PK_GRID) and u == 2           # PKG && U == 2
        if packed and pat == 'REF16' and pk == PK_GRID:       # FAST: every round at N = 256 is full
            return 'grid2_full/REF16'
        if packed:
            return f'grid2/{pat}'
        return f'grid/R{r}/{pat}/U{u}'
    if pk == PK_ALL and kk % 2 == 0:
        return f'gp/U{u}'
    return f'g/U{u}'


def case_id(cls: str, alphabet: str) -> str:
    return f'{cls}-{alphabet}-K{alphabet_size(alphabet)}-{packing(cls, alphabet)}-{expected_form(cls, alphabet)}'


def partial_round(cls: str, alphabet: str, M: int) -> bool:
    """Whether the last workgroup (3 of 16 trials) runs a masked partial step: its 3 Nt / M sections
    are no multiple of the U * 64 / M sections one wave takes per step."""
    nt = CLASSES[cls][1]
    return (3 * nt // M) % (sections_in_flight(alphabet) * 64 // M) != 0


def x3_fits(nt: int, M: int, K: int = 0) -> bool:
    """vamp_persist_x3_fits at k = N = Nt, Lin = 1: the split-precision layout (six bf16 planes,
    r and x~ with stride 2N + 8, two var buffers, 2 x 16 L section words, 1024 words of scratch)
    plus the kernel's static LDS (2 KB allowed; 5 KB with a 64-point table) within 160 KB.  At
    Nt = 256 that holds for L = Nt / M <= 72, i.e. M >= 4, and for K = 64 up to L = 48: M >= 8."""
    L = nt // M
    plane = max(6 * 16 * nt // 2, PBM * (2 * nt + 4))
    total = plane + 2 * PBM * (2 * nt + 8) + 2 * PBM * nt + 2 * PBM * L
    total = (total + 3) // 4 * 4 + 1024
    return total * 4 + (5120 if K > 16 else 2048) <= 160 * 1024


def section_sizes(cls: str, alphabet: str):
    """The section sizes of a case: all six, except where the split-precision engine's LDS does not
    hold the shape and the library refuses it (amp_vamp_select_gemm_k answers AMP_E_ARG): M = 2 at
    x3_n256 (L = 128 sections per trial), and M = 4 too for the 64-point alphabet, whose kernels
    hold 3.5 KB more static LDS.  The f32 class runs those shapes."""
    gemm, nt, _, _ = CLASSES[cls]
    return tuple(M for M in SECTION_SIZES if gemm != GEMM_X3 or x3_fits(nt, M, alphabet_size(alphabet)))


# ----------------------------------------------------------------------------- configs
def make_config(alphabet: str, nt: int, M: int, batch: int = B, iterations: int = ITERS, device: str = 'cuda'):
    """Config at Nr = 2 Nt, Lin = Lh = 1, 'sparc'; 'sqK' is Config.inject_square_qam(K), applied
    before Channel / Data / VAMP are built."""
    from config import Config
    sq = alphabet.startswith('sq')
    cfg = Config(nt, nt // M, 2 * nt, 1, 1, batch=batch, generator_mode='sparc', iterations=iterations,
                 alphabet='QPSK' if sq else alphabet, channel_profile='uniform', channel_truncation='tail',
                 device=device)
    if sq:
        cfg.inject_square_qam(int(alphabet[2:]))
    assert cfg.K == alphabet_size(alphabet)
    return cfg


def oracle_config(cfg):
    """The oracle's config of `cfg`, with the (possibly injected) constellation."""
    from oracle import OracleConfig
    base = cfg.alphabet if not cfg.alphabet.endswith('QAM') or cfg.alphabet == '16QAM' else 'QPSK'
    o = OracleConfig(cfg.Nt, cfg.Na, cfg.Nr, B=cfg.B, alphabet=base, iterations=cfg.N_Layers)
    o.symbols = cfg.symbols
    o.K = cfg.K
    return o


# ----------------------------------------------------------------------------- float64 reference
def denoise_f64(r, tau, symbols, L: int, M: int):
    """The block-sparse denoiser (oracle.amp_oracle.block_denoise, vamp.py:96-119) in float64
    throughout, the division r / tau included; nothing is cast down.

    r [B, L * M] complex, tau a scalar or [B, L * M]; returns x (complex128 [B, L * M]), var
    (float64 [B, L * M]), secmax (float64 [B, L]: each section's max logit) and max_abs_xi (the
    batch's max |xi|).  The softmax runs over a whole section (M positions x K points); it is
    shifted by the section's own max (the softmax is shift-invariant; the oracle's batch-global
    max|xi| shift only matters once exp leaves the float64 range, which no case here reaches)."""
    r = np.asarray(r, np.complex128)
    nb = r.shape[0]
    a = np.asarray(symbols).astype(np.complex128)
    t = np.asarray(tau, np.float64)
    u = (r / (t if t.ndim == 0 else t.reshape(nb, L * M))).reshape(nb, L, M)
    xi = (u[..., None] * np.conj(a)).real                              # [B, L, M, K]
    secmax = xi.max(axis=(2, 3))
    eta = np.exp(xi - secmax[:, :, None, None])
    zm = eta.sum(axis=-1)                                              # [B, L, M]
    z = zm.sum(axis=2, keepdims=True)                                  # [B, L, 1]
    x = (a * eta).sum(axis=-1) / z
    var = np.abs(x) ** 2 * (1 - zm / z) + (np.abs(x[..., None] - a) ** 2 * eta).sum(axis=-1) / z
    return SimpleNamespace(x=x.reshape(nb, -1), var=var.reshape(nb, -1), secmax=secmax,
                           max_abs_xi=float(np.abs(xi).max()))


def xtol(max_abs_xi: float) -> float:
    """The project's bar for the float32-logit denoiser against the float64 one
    (test_gpu_vamp._xtol), with the exact max |xi| in place of its 1.35 max|r| / tau estimate."""
    return 3e-6 + 4e-7 * max_abs_xi


VAR_RTOL = 1e-4    # test_g2_denoiser's relative bar on var


def torch_close_f32(a, b):
    """torch.allclose's element test in float32, operation for operation as amp_common.h
    torch_close evaluates it (rtol 1e-5, atol 1e-8)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        actual = np.abs(a - b)
        allowed = np.float32(1.0e-8) + np.abs(np.float32(1.0e-5) * b)
        return (a == b) | (np.isfinite(actual) & (actual <= allowed))
