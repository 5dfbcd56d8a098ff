"""CPU: the helper of the persistent-engine denoiser tests (persist_denoiser_cases.py).

* its float64 denoiser against the oracle's block_denoise for every alphabet of the case table;
* the case table reaches every amp_denoise.h form the GPU test claims, a masked partial round for
  U = 2 and for U = 4, and its LDS rule for the split-precision engine is the library's own;
* at the table's operating point (seed 0, EbN0 = 8 dB, 3 iterations, B = 35) the oracle runs all
  three iterations and no section comes near the rare exact-float64 path, so what the GPU test
  reads from the persistent kernel is the fast path's output.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import persist_denoiser_cases as pdc
from oracle import block_denoise, vamp_detect
from oracle.amp_oracle import _logits


@pytest.mark.parametrize('M', [2, 64])
@pytest.mark.parametrize('alphabet', pdc.ALPHABETS)
def test_denoise_f64_matches_oracle(alphabet, M):
    """tau is a power of two and r holds float32 values, so the oracle's complex64 r * (1 / tau)
    is exact and both form the same float64 logits: the oracle's complex64 / float32 outputs are
    then denoise_f64's values rounded once (half a float32 ulp; the float64 sums differ in order
    and shift by ~1e-15 relative)."""
    nt, nb = 128, 9
    cfg = pdc.make_config(alphabet, nt, M, batch=nb, device='cpu')
    ocfg = pdc.oracle_config(cfg)
    rng = np.random.default_rng(1000 + M)
    r = (0.7 * (rng.standard_normal((nb, nt)) + 1j * rng.standard_normal((nb, nt)))).astype(np.complex64)
    tau = np.float32(0.125)
    xo, vo = block_denoise(r, tau, ocfg)
    ref = pdc.denoise_f64(r, tau, cfg.symbols, ocfg.L, M)
    assert 10 < ref.max_abs_xi < 60                        # weights from 1 down to e^-100: a real softmax
    assert ref.x.dtype == np.complex128 and ref.var.dtype == np.float64
    ulp = 2.0 ** -24
    for got, want in ((xo.real, ref.x.real), (xo.imag, ref.x.imag), (vo, ref.var)):
        err = np.abs(got.astype(np.float64) - want)
        assert np.all(err <= ulp * np.abs(want) + 1e-45 + 1e-13 * np.abs(want).max()), float(err.max())
    xi = _logits(r, tau, ocfg, nb)
    assert ref.max_abs_xi == float(np.abs(xi).max())
    assert np.array_equal(ref.secmax, xi.max(axis=(2, 3)))


def test_section_size_one_is_out():
    """M = 1 (p = 1): the oracle's initial sigma2~ = p^2 (1 - p) + (1 - p)^2 p is zero, so its first
    noise_var / sigma2~ (a Python float division, vamp.py:66) raises: no reference to compare with."""
    cfg = pdc.make_config('QPSK', 64, 1, batch=2, device='cpu')
    ocfg = pdc.oracle_config(cfg)
    with pytest.raises(ZeroDivisionError):
        vamp_detect(np.eye(128, 64, dtype=np.complex64), np.ones(64, np.float32), np.eye(64, dtype=np.complex64),
                    np.zeros((2, 128), np.complex64), 1.0, ocfg)


def test_form_coverage():
    """The persistent cases reach every path the denoiser's dispatch has for them."""
    seen = {(pdc.alphabet_size(a), pdc.packing(c, a), pdc.expected_form(c, a), pdc.CLASSES[c][3])
            for c in pdc.CLASSES for a in pdc.ALPHABETS}
    forms = {(kk, pk, f) for kk, pk, f, _ in seen}
    assert (1, pdc.PK_ALL, 'g/U4') in forms and (1, pdc.PK_NONE, 'g/U4') in forms
    for kk, u in ((2, 4), (4, 4), (8, 2)):
        assert (kk, pdc.PK_NONE, f'g/U{u}') in forms and (kk, pdc.PK_ALL, f'gp/U{u}') in forms
    # 16PSK: the scalar per-point form at two waves per SIMD (both policies), the packed one at one
    assert {(16, pdc.PK_NONE, 'g/U2'), (16, pdc.PK_GRID, 'g/U2'), (16, pdc.PK_ALL, 'gp/U2')} <= forms
    assert (4, pdc.PK_NONE, 'grid/R2/FULL/U4') in forms and (4, pdc.PK_ALL, 'grid/R2/FULL/U4') in forms
    # the scalar R = 4 grids at U = 2 run in the two-per-CU build
    assert {(16, pdc.PK_NONE, 'grid/R4/REF16/U2', 2), (16, pdc.PK_NONE, 'grid/R4/FULL/U2', 2)} <= seen
    assert {(16, pdc.PK_ALL, 'grid2/REF16'), (16, pdc.PK_ALL, 'grid2/FULL')} <= forms
    assert {(16, pdc.PK_GRID, 'grid2_full/REF16'), (16, pdc.PK_GRID, 'grid2/FULL')} <= forms
    assert {(64, pdc.PK_NONE, 'wide/grid/R8'), (64, pdc.PK_ALL, 'wide/grid/R8')} <= forms
    # a masked partial round (the 3-trial workgroup) with two and with four sections in flight, and
    # none at Nt = 256, where the FAST loop must take every round
    part = {pdc.sections_in_flight(a) for c in pdc.CLASSES for a in pdc.ALPHABETS for M in pdc.section_sizes(c, a)
            if pdc.partial_round(c, a, M)}
    assert {2, 4} <= part
    assert not any(pdc.partial_round(c, a, M) for c in ('x3_n256', 'f32_n256') for a in pdc.ALPHABETS
                   for M in pdc.section_sizes(c, a))
    ids = [pdc.case_id(c, a) for c in pdc.CLASSES for a in pdc.ALPHABETS]
    assert len(set(ids)) == len(ids) == 50


def test_split_precision_lds_rule_is_the_librarys():
    """section_sizes drops exactly the shapes amp_vamp_select_gemm_k refuses: on the bf16x3 engine
    at Nt = 256, M = 2 (L = 128 sections per trial) and, for the 64-point alphabet, M = 4 as well;
    every other (class, alphabet, M) keeps the arithmetic the case asks for."""
    import amp_native as nat
    assert (pdc.GEMM_F32, pdc.GEMM_X3, pdc.ENGINE_PERSISTENT) == (nat.GEMM_F32, nat.GEMM_X3, nat.ENGINE_PERSISTENT)
    dropped = set()
    for cls, (gemm, nt, _, _) in pdc.CLASSES.items():
        for alphabet in pdc.ALPHABETS:
            K = pdc.alphabet_size(alphabet)
            for M in pdc.SECTION_SIZES:
                d = pdc.make_config('QPSK', nt, M, device='cpu').dims()
                got = nat.lib().amp_vamp_select_gemm_k(C.byref(d), nt, gemm, K)
                if M in pdc.section_sizes(cls, alphabet):
                    assert got == gemm, (cls, alphabet, M, got)
                else:
                    assert got == pdc.AMP_E_ARG, (cls, alphabet, M, got)
                    dropped.add((cls, K, M))
                if K <= 16:
                    assert nat.lib().amp_vamp_select_gemm(C.byref(d), nt, gemm) == got
    assert dropped == {('x3_n256', K, 2) for K in (1, 2, 4, 8, 16, 64)} | {('x3_n256', 64, 4)}


OBJ_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'amp-sparc-spatialmodulation_amd',
                       'build')
LLVM = '/opt/rocm/llvm/bin'
UNITS = ('amp_vamp_persist', 'amp_vamp_persist_x3', 'amp_vamp_persist_h2', 'amp_vamp_persist_i8')


def _static_lds(obj, td):
    """{kernel name: static LDS bytes (.group_segment_fixed_size)} of the gfx950 code object in obj."""
    fb, dev = os.path.join(td, 'fb.bin'), os.path.join(td, 'dev.o')
    subprocess.run([f'{LLVM}/llvm-objcopy', '--dump-section=.hip_fatbin=' + fb, obj, os.path.join(td, 'h.o')],
                   check=True, capture_output=True)
    subprocess.run([f'{LLVM}/clang-offload-bundler', '--type=o', '--unbundle', '--input=' + fb,
                    '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', '--output=' + dev], check=True, capture_output=True)
    notes = subprocess.run([f'{LLVM}/llvm-readelf', '--notes', dev], check=True, capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r'\n\s*- \.agpr_count:', notes)[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk)
        lds = re.search(r'\.group_segment_fixed_size:\s+(\d+)', blk)
        if name and lds:
            out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-readelf')), reason='llvm-readelf not installed')
def test_static_lds_within_the_eligibility_allowance(tmp_path):
    """The eligibility rules (vamp_persist_x3_fits, vamp_persist_eligible) allow a constant for the
    static LDS vamp_persist holds beside its dynamic carve: 2 KB, and 5 KB on the split-precision
    engines with a 64-point table.  Every instantiation's code object stays within it (the f32
    form's 2 KB for K = 64 is short of its 3.7 KB, but its largest carve, N = 256 at L = 128,
    leaves 11 KB)."""
    objs = [os.path.join(OBJ_DIR, u + '.o') for u in UNITS]
    if not all(os.path.exists(o) for o in objs):
        pytest.skip('the build objects are not here (build() / make -C amp-sparc-spatialmodulation_amd/csrc)')
    seen = 0
    for i, obj in enumerate(objs):
        td = tmp_path / str(i)
        td.mkdir()
        for name, lds in _static_lds(obj, str(td)).items():
            m = re.match(r'_ZN3amp12vamp_persistILi(\d+)ELi(\d+)ELi(\d+)ELi\d+ELb([01])E', name)
            if not m:
                continue
            nt, kk, nwv, x3 = (int(v) for v in m.groups())
            seen += 1
            if x3:
                assert lds <= (5120 if kk > 16 else 2048), (name, lds)
            else:
                # f32 carve (floats): A, r, x~ at 16 (2N + 4), two var buffers, 32 L at L = N / 2, scratch;
                # a wave owns 16 NT of the 2N real columns
                n = 8 * nt * nwv
                carve = 4 * (3 * 16 * (2 * n + 4) + 2 * 16 * n + 32 * (n // 2) + 1024)
                assert carve + lds <= 160 * 1024, (name, lds, carve)
    assert seen >= 40, seen


@pytest.mark.parametrize('nt', [64, 256])
@pytest.mark.parametrize('alphabet', pdc.ALPHABETS)
def test_operating_point_stays_on_the_fast_path(alphabet, nt):
    """The oracle at the table's operating point: T == 3 (no early exit: every dumped iteration
    exists) and min(section max) - max|xi| > -600 at every iteration, far from AMP_DANGER = -700
    (less the slack), where the kernels hand a section to exact_section_f64."""
    from test_gpu_vamp import _regen_inputs
    for M in (2, 64):
        cfg = pdc.make_config(alphabet, nt, M, device='cpu')
        inp = _regen_inputs(cfg, pdc.SEED, pdc.EBN0)
        ocfg = pdc.oracle_config(cfg)
        c = lambda t: t.numpy()[..., 0] if t.dim() == 3 else t.numpy()   # noqa: E731
        trace = []
        out = vamp_detect(c(inp['U']), c(inp['s']), c(inp['Vh']), c(inp['y']), float(inp['SNR']), ocfg, trace=trace)
        assert out['T'] == pdc.ITERS == len(trace), (M, out['T'])
        for t, it in enumerate(trace):
            ref = pdc.denoise_f64(it['r'], np.float64(it['sigma2']), cfg.symbols, ocfg.L, M)
            spread = float(ref.secmax.min()) - ref.max_abs_xi
            print(f'{alphabet} Nt={nt} M={M} t={t}: max|xi| {ref.max_abs_xi:.1f} spread {spread:.1f}')
            assert spread > -600, (M, t, spread)
            assert np.isfinite(it['xmmse']).all() and np.isfinite(it['var']).all()
