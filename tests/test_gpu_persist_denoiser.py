"""GPU: the denoiser forms of the persistent VAMP engine against a float64 denoiser ON THE KERNEL'S
OWN INPUT, per (kernel class, alphabet) of tests/persist_denoiser_cases.py and every section size.

The end-to-end tests of the persistent engines (VER / SER within 1e-3, engine against engine, bit
fixtures recorded through an earlier build) cannot see a denoiser that is off in the fifth digit at
a shape nobody ran; amp_block_denoise (the g2 goldens) runs the U = 1 / PK_ALL forms only.  Here:

a. bf16x3 classes: one 3-iteration forward with the state dump on (amp_vamp_debug_dump); per
   iteration r, xmmse, var, 1 / sigma2 and the waves' float64 variance sums are read back and
   1. xmmse / var are compared with persist_denoiser_cases.denoise_f64(r, 1 / inv_sigma2) at the
      project's bars for the float32-logit denoiser (test_gpu_vamp._xtol / test_g2_denoiser, with the
      exact max |xi|):  |x - ref| <= 3e-6 + 4e-7 max|xi|,  |var - ref| <= 1e-4 |ref| + the same;
   2. the waves' float64 sums add up to the float64 sum of the stored float32 var (1e-12 relative:
      reassociation only), per workgroup — a masked lane that stores but is not counted, or the
      reverse, fails here;
   3. the published exchange record of every workgroup: the not-close count equals the count from
      the dumped var (exact), max|xi| / min section max agree with the float64 reference's, and the
      batch stays clear of the rare exact-float64 path (so the dump IS the fast path's output);
   4. the outputs r / xmmse / var equal the last iteration's dump bit for bit (the 3-row workgroup).
b. f32 classes (no r plane in the dump): the final outputs after 1 and 3 iterations with
   tau = status.last_scalar[2].
c. amp_block_denoise on the square alphabets (GRID_FULL at R = 2, 4, 8: no other test reaches
   them), M in {1, 2, 8, 64, 128}, modes 0 / 1 / 2, a section count that ends inside a workgroup pass.

Measured margins per form: profiles/persist_denoiser_err.txt (tools/persist_denoiser_err.py).
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import persist_denoiser_cases as pdc

pytestmark = pytest.mark.gpu

# alphabet-major: the classes that share Nt reuse one set of inputs (the cache below)
CASES = [(c, a) for a in pdc.ALPHABETS for c in pdc.CLASSES]
IDS = [pdc.case_id(c, a) for c, a in CASES]


@functools.lru_cache(maxsize=18)
def _inputs(alphabet, nt, M):
    """Host tensors of the case's operating point (seed 0, EbN0 = 8 dB), built once per shape."""
    from test_gpu_vamp import _regen_inputs
    inp = _regen_inputs(pdc.make_config(alphabet, nt, M, device='cpu'), pdc.SEED, pdc.EBN0)
    return {k: inp[k] for k in ('U', 's', 'Vh', 'y', 'SNR')}


def _on(device, inp):
    return [inp[k].to(device) for k in ('U', 's', 'Vh', 'y')] + [inp['SNR']]


def _assert_route(cfg, nt, gemm):
    import amp_native as nat
    d = cfg.dims()
    assert nat.lib().amp_vamp_select_engine(C.byref(d), nt, nat.ENGINE_PERSISTENT) == nat.ENGINE_PERSISTENT
    assert nat.lib().amp_vamp_select_gemm_k(C.byref(d), nt, gemm, cfg.K) == gemm


def _f32(t, cols):
    return t.detach().cpu().contiguous().view(torch.float32).numpy().reshape(-1, cols)


def _cplx(a):
    """[rows, 2N] float32 (re, im interleaved) -> [rows, N] complex128."""
    a = a.astype(np.float64)
    return a[:, 0::2] + 1j * a[:, 1::2]


def errors(x, var, ref):
    """(max |x - ref| / tol, max var error / its bar) at the bars of assertion 1; var None: mean only."""
    tol = pdc.xtol(ref.max_abs_xi)
    ex = float(np.abs(x - ref.x).max() / tol)
    ev = 0.0 if var is None else float((np.abs(var - ref.var) / (pdc.VAR_RTOL * np.abs(ref.var) + tol)).max())
    return ex, ev


def capture_x3(device, cls, alphabet, M):
    """One forward of a bf16x3 class with the state dump on: per-iteration r / xmmse / var of the
    valid trials, 1 / sigma2, the waves' float64 var sums and the exchange records, plus the outputs."""
    import amp_native as nat
    from vamp import VAMP
    gemm, nt, nwv, _ = pdc.CLASSES[cls]
    cfg = pdc.make_config(alphabet, nt, M)
    _assert_route(cfg, nt, gemm)
    U, s, Vh, y, snr = _on(device, _inputs(alphabet, nt, M))
    nwg = (pdc.B + pdc.PBM - 1) // pdc.PBM
    dump = torch.zeros(pdc.ITERS, nwg, 5, pdc.PBM, 2 * nt, dtype=torch.float32, device=device)
    det = VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=gemm)
    nat.check(nat.lib().amp_vamp_debug_dump(C.c_void_p(dump.data_ptr())), 'amp_vamp_debug_dump')
    try:
        T = det.detect(U, s, Vh, y, snr)
        torch.cuda.synchronize()
    finally:
        nat.lib().amp_vamp_debug_dump(None)
    st = T.status()
    d = dump.cpu().numpy()
    off = (C.c_uint64 * 5)()
    dims = cfg.dims()
    nat.check(nat.lib().amp_vamp_debug_offsets(C.byref(dims), nt, pdc.ITERS, 1, off), 'amp_vamp_debug_offsets')
    gran = T.buf.ws[int(off[0]):int(off[0]) + pdc.ITERS * nwg * 32].cpu().numpy().view(np.uint32)
    gran = gran.reshape(pdc.ITERS, nwg, 8).copy()
    rows = [min(pdc.PBM, pdc.B - w * pdc.PBM) for w in range(nwg)]
    valid = lambda p: np.concatenate([d[:, w, p, :rows[w]] for w in range(nwg)], axis=1)   # noqa: E731
    wsum = np.ascontiguousarray(d[:, :, 3, 0, nt:nt + 2 * nwv]).view(np.float64)           # [ITERS, nwg, nwv]
    return SimpleNamespace(cfg=cfg, nt=nt, nwg=nwg, rows=rows, status=st, r=valid(1), x=valid(2),
                           var=valid(3)[:, :, :nt], inv=d[:, 0, 3, 1, nt], inv_all=d[:, :, 3, 1, nt], wsum=wsum,
                           gran=gran, out_r=_f32(T.buf.r, 2 * nt), out_x=_f32(T.buf.xmmse, 2 * nt),
                           out_var=_f32(T.buf.var, nt))


def check_x3(cap, M):
    """Assertions 1-4 on a captured forward; returns the error ratios of assertion 1 per iteration."""
    cfg, nt = cap.cfg, cap.nt
    L = nt // M
    assert cap.status.T == pdc.ITERS and cap.status.nan_state == 0 and cap.status.gemm == 2, \
        (cap.status.T, cap.status.nan_state, cap.status.gemm)
    for name in ('r', 'x', 'var'):
        assert not np.isnan(getattr(cap, name)).any(), name
    ratios = []
    prev = np.ones_like(cap.var[0])
    for t in range(pdc.ITERS):
        inv = cap.inv[t]
        assert inv > 0 and np.all(cap.inv_all[t] == inv)           # one batch scalar in every workgroup
        tau = 1.0 / np.float64(inv)
        r = _cplx(cap.r[t])
        ref = pdc.denoise_f64(r, tau, cfg.symbols, L, M)
        x, var = _cplx(cap.x[t]), cap.var[t].astype(np.float64)
        ex, ev = errors(x, var, ref)
        print(f'M={M} t={t}: max|xi| {ref.max_abs_xi:.1f}  x err/tol {ex:.3f}  var err/tol {ev:.3f}')
        ratios.append((ex, ev))
        tol = pdc.xtol(ref.max_abs_xi)
        # 1. mean and variance against float64 on the kernel's own input
        assert np.all(np.abs(x - ref.x) <= tol), (M, t, ex)
        assert np.all(np.abs(var - ref.var) <= pdc.VAR_RTOL * np.abs(ref.var) + tol), (M, t, ev)
        notclose = ~pdc.torch_close_f32(cap.var[t], prev)
        gmax, gmin = 0.0, np.inf
        row0 = 0
        for w, n in enumerate(cap.rows):
            sl = slice(row0, row0 + n)
            row0 += n
            # 2. accounting: the waves' float64 sums of the float32 var they stored
            want = cap.var[t][sl].astype(np.float64).sum()
            got = cap.wsum[t, w].sum()
            assert abs(got - want) <= 1e-12 * abs(want), (M, t, w, got, want)
            # 3. the exchange record the workgroup published
            g = cap.gran[t, w]
            assert g[3] == g[7] and g[3] != 0, (M, t, w, g)
            sumvar = g[:2].copy().view(np.float64)[0]
            assert abs(sumvar - want) <= 1e-12 * abs(want), (M, t, w, sumvar, want)
            assert int(g[2]) == int(notclose[sl].sum()), (M, t, w, int(g[2]), int(notclose[sl].sum()))
            mx, mn = (float(v) for v in g[4:6].copy().view(np.float32))
            rw = pdc.denoise_f64(r[sl], tau, cfg.symbols, L, M)
            tw = pdc.xtol(rw.max_abs_xi)
            assert abs(mx - rw.max_abs_xi) <= tw, (M, t, w, mx, rw.max_abs_xi)
            assert abs(mn - float(rw.secmax.min())) <= tw, (M, t, w, mn, float(rw.secmax.min()))
            gmax, gmin = max(gmax, mx), min(gmin, mn)
        # the batch never came near the rare exact-float64 path (amp_common.h part_danger)
        assert gmin - gmax > pdc.AMP_DANGER + pdc.logit_slack(gmax), (M, t, gmin, gmax)
        prev = cap.var[t]
    # 4. the outputs are the last iteration's state, bit for bit
    last = pdc.ITERS - 1
    for name, out, dumped in (('r', cap.out_r, cap.r[last]), ('xmmse', cap.out_x, cap.x[last]),
                              ('var', cap.out_var, cap.var[last])):
        assert np.array_equal(out.view(np.uint32), np.ascontiguousarray(dumped).view(np.uint32)), (M, name)
    return ratios


def capture_f32(device, cls, alphabet, M, iters):
    """One forward of an f32 class: the final r / xmmse / var and sigma2 of the last iteration."""
    import amp_native as nat
    from vamp import VAMP
    gemm, nt, _, _ = pdc.CLASSES[cls]
    cfg = pdc.make_config(alphabet, nt, M, iterations=iters)
    _assert_route(cfg, nt, gemm)
    U, s, Vh, y, snr = _on(device, _inputs(alphabet, nt, M))
    T = VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=gemm).detect(U, s, Vh, y, snr)
    torch.cuda.synchronize()
    return SimpleNamespace(cfg=cfg, nt=nt, status=T.status(), r=_f32(T.buf.r, 2 * nt), x=_f32(T.buf.xmmse, 2 * nt),
                           var=_f32(T.buf.var, nt))


def check_f32(cap, M, iters):
    st = cap.status
    assert st.T == iters and st.nan_state == 0 and st.gemm == 1, (st.T, st.nan_state, st.gemm)
    for name in ('r', 'x', 'var'):
        assert not np.isnan(getattr(cap, name)).any(), name
    sigma2 = np.float32(st.last_scalar[2])
    assert sigma2 > 0
    ref = pdc.denoise_f64(_cplx(cap.r), np.float64(sigma2), cap.cfg.symbols, cap.nt // M, M)
    x, var = _cplx(cap.x), cap.var.astype(np.float64)
    ex, ev = errors(x, var, ref)
    print(f'M={M} iterations={iters}: max|xi| {ref.max_abs_xi:.1f}  x err/tol {ex:.3f}  var err/tol {ev:.3f}')
    tol = pdc.xtol(ref.max_abs_xi)
    assert np.all(np.abs(x - ref.x) <= tol), (M, iters, ex)
    assert np.all(np.abs(var - ref.var) <= pdc.VAR_RTOL * np.abs(ref.var) + tol), (M, iters, ev)
    return ex, ev


@pytest.mark.parametrize('cls,alphabet', CASES, ids=IDS)
def test_persistent_denoiser_form(device, cls, alphabet):
    x3 = pdc.CLASSES[cls][0] == pdc.GEMM_X3
    for M in pdc.section_sizes(cls, alphabet):
        if x3:
            check_x3(capture_x3(device, cls, alphabet, M), M)
        else:
            for iters in (1, pdc.ITERS):
                check_f32(capture_f32(device, cls, alphabet, M, iters), M, iters)


@pytest.mark.parametrize('alphabet,M', [('QPSK', 2), ('sq64', 2), ('sq64', 4)])
def test_split_precision_refuses_the_shapes_its_lds_cannot_hold(device, alphabet, M):
    """Nt = 256 at M = 2 (L = 128), and at M = 4 (L = 64) with the 64-point alphabet, are the shapes
    of the table the bf16x3 engine does not take.  The library says so (AMP_E_ARG) and an explicit
    GEMM_X3 forward raises before any launch; GEMM_AUTO runs the f32 form, checked like an f32
    class.  (Square 64-QAM at M = 4 used to be accepted and then failed inside the launch, in
    hipFuncSetAttribute, leaving its error for the caller's next HIP call.)"""
    import amp_native as nat
    from vamp import VAMP
    cfg = pdc.make_config(alphabet, 256, M)
    d = cfg.dims()
    assert nat.lib().amp_vamp_select_gemm_k(C.byref(d), 256, nat.GEMM_X3, cfg.K) == pdc.AMP_E_ARG
    assert nat.lib().amp_vamp_select_gemm_k(C.byref(d), 256, nat.GEMM_AUTO, cfg.K) == nat.GEMM_F32
    U, s, Vh, y, snr = _on(device, _inputs(alphabet, 256, M))
    with pytest.raises(nat.AmpError):
        VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=nat.GEMM_X3).detect(U, s, Vh, y, snr)
    torch.cuda.synchronize()                       # no error left behind in the runtime
    T = VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=nat.GEMM_AUTO).detect(U, s, Vh, y, snr)
    torch.cuda.synchronize()
    cap = SimpleNamespace(cfg=cfg, nt=256, status=T.status(), r=_f32(T.buf.r, 512), x=_f32(T.buf.xmmse, 512),
                          var=_f32(T.buf.var, 256))
    check_f32(cap, M, pdc.ITERS)


# ----------------------------------------------------------------------------- standalone op
ST_B, ST_NA = 45, 7      # 315 sections: no multiple of the 256 / 128 / 32 / 4 sections of a workgroup pass
ST_CASES = [(a, M) for a in ('sq4', 'sq16', 'sq64') for M in (1, 2, 8, 64)] + [('sq4', 128), ('sq16', 128)]


def standalone_errors(device, alphabet, M):
    """amp_block_denoise modes 0 / 1 / 2 on seeded r with max |xi| ~ 100 against denoise_f64;
    returns {mode: (x err/tol, var err/tol)} after asserting the bars."""
    from config import Config
    from vamp import block_denoise
    nt = ST_NA * M
    cfg = Config(nt, ST_NA, 2 * nt, 1, 1, batch=ST_B, generator_mode='sparc', alphabet='QPSK',
                 channel_profile='uniform', channel_truncation='tail', device='cuda')
    cfg.inject_square_qam(int(alphabet[2:]))
    per = 4 * (64 // min(M, 64))
    assert ST_B * ST_NA > per and (ST_B * ST_NA) % per != 0     # full passes, then one that ends early
    rng = np.random.default_rng(4000 + 8 * M + cfg.K)
    tau = np.float32(0.05)
    g = rng.standard_normal((ST_B, nt)) + 1j * rng.standard_normal((ST_B, nt))
    peak = float(np.abs((g[..., None] * np.conj(cfg.symbols)).real).max())      # max |Re(g a*)|
    r = (g * (100.0 * float(tau) / peak)).astype(np.complex64)                   # max |xi| = 100 at tau
    spread = (1.0 + 0.5 * rng.random((ST_B, nt))).astype(np.float32)
    cov = (np.float32(2.0) * tau * spread).astype(np.float32)       # modes 1 / 2: tau = cov / 2 in [tau, 1.5 tau]
    rd = torch.from_numpy(r).to(device)
    cd = torch.from_numpy(cov).to(device)
    out = {}
    for mode, tv, tref in ((0, float(tau), np.float64(tau)), (1, cd, cov.astype(np.float64) / 2),
                           (2, cd, cov.astype(np.float64) / 2)):
        ref = pdc.denoise_f64(r, tref, cfg.symbols, ST_NA, M)
        if mode == 0:
            assert 99.9 < ref.max_abs_xi < 100.1, ref.max_abs_xi
        got = block_denoise(cfg, rd, tv, mode=mode)
        xm, var = (got, None) if mode == 2 else got
        x = xm.cpu().numpy()[..., 0].astype(np.complex128)
        v = None if var is None else var.cpu().numpy()[..., 0].astype(np.float64)
        assert not np.isnan(x).any() and (v is None or not np.isnan(v).any())
        ex, ev = errors(x, v, ref)
        print(f'{alphabet} M={M} mode {mode}: max|xi| {ref.max_abs_xi:.1f}  x err/tol {ex:.3f}  var err/tol {ev:.3f}')
        tol = pdc.xtol(ref.max_abs_xi)
        assert np.all(np.abs(x - ref.x) <= tol), (mode, ex)
        if v is not None:
            assert np.all(np.abs(v - ref.var) <= pdc.VAR_RTOL * np.abs(ref.var) + tol), (mode, ev)
        out[mode] = (ex, ev)
    return out


@pytest.mark.parametrize('alphabet,M', ST_CASES, ids=[f'{a}-M{m}' for a, m in ST_CASES])
def test_block_denoise_square_alphabets(device, alphabet, M):
    """The U = 1 forms no persistent case reaches: denoise_step_grid<GRID_FULL> at R = 2 / 4 / 8
    through denoise_sections, and the M > 64 per-point form on square alphabets (not a grid form)."""
    standalone_errors(device, alphabet, M)
