"""GPU: the linear half of every iteration of the persistent VAMP engine (the y~ product, GEMM1 with
the w = scale (y~ + vr q) - q epilogue, GEMM2 with the r epilogue, the LMMSE scalar chain) against a
float64 evaluation ON THE KERNEL'S OWN INPUT, for every arithmetic (f32 MFMA, bf16x3, fp16x2,
int8x4) at every instantiation of tests/persist_linear_ref.CASES.

The bit fixtures of the engine prove that a rewrite changed nothing, not that the chain's root is
right, and only at the shapes recorded; test_vamp_x3_gemm_matches_f32 bounds the split engines by
the f32 engine's own deviation.  Neither would see a bf16x3 low plane that is dropped, mis-signed or
mis-indexed (a 2^-16-level operand error), a wrong q0 on the reuse path, or a y~ that is off in the
sixth digit at a shape nobody recorded.  Here, per forward (seed 0, EbN0 = 2 dB, B = 35: workgroups
of 16, 16 and 3 rows, 3 iterations; the state dump amp_vamp_debug_dump on, y~ read from the
workspace at amp_vamp_debug_offsets[4]):

1. the route (amp_vamp_select_engine, amp_vamp_select_gemm_k, status.gemm), T == 3, no NaN state,
   no NaN in any plane; rows past the valid ones are never compared;
2. scalars: persist_linear_ref.scalar_chain (vamp_detect's float32 lines) run from t = 0 on the
   dumped var means gives the dumped 1 / sigma2 of every iteration and workgroup and the status
   record's four last scalars BIT FOR BIT;
3. y~ against ytil_f64;
4. w_t against w_f64 on the kernel's own r~ (dump t - 1 and the scalars of 2; the Tracker's at
   t = 0) and its own y~;
5. r_t against r_f64 on the kernel's own dumped w_t: GEMM2 is judged alone;
6. the f32 class (no w / r planes in the dump): forwards of 1, 2 and 3 iterations, asserted
   prefix-consistent (the 3-iteration forward's dumped xmmse / var / 1 / sigma2 of iteration t are
   the (t + 1)-iteration forward's outputs, bit for bit, and y~ is the same); r of the
   (t + 1)-iteration forward against r_f64(w_f64(...)) on the t-iteration forward's outputs.

Bars of 3-6: e_rms <= K_RMS and e_max <= K_MAX times the same statistic of the numpy c64
restatement on the identical inputs, computed here on the host (K_RMS = 3, K_MAX = 6, no absolute
floor; tests/test_persist_linear_cpu.py holds a 16-bit operand at >= 2 K_RMS for every case).
The fp16x2 engine at n = 2N forms y~ inside vamp_persist and stores none: its w is judged against
w_f64 on ytil_f64, the yardstick taking its own c64 y~ (y~ and GEMM1 together).

Also: a B = 1 forward at Nt = 64 and at Nt = 256 (a single valid row), and for bf16x3 at Nt = 64 and
256 a building forward and the reuse forward after it with a new y (the q0_load branch).
The yardstick's products are matrix products at every batch size: a batch below the kernel's
16-row tile is zero-padded to it (persist_linear_ref._mm_c64).  numpy hands a one-row product to
another BLAS routine, which errs 2.2x less than its matrix product on the same row (y~ at Nt = 64,
B = 1: e_rms 2.9e-8 against 6.4e-8; a sequential float32 sum: 1.2e-7); against that routine the
f32 launch GEMM's y~ (1.0e-7 on that row, 1.5x numpy's at B = 35) measured 3.5x in rms and 6.4x in
max, every other phase and arithmetic of the two B = 1 cases staying inside the bars.

Measured ratios per case, phase and arithmetic: profiles/persist_linear_err.txt
(tools/persist_linear_err.py).
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import persist_linear_ref as plr

pytestmark = pytest.mark.gpu

F32 = np.float32
CASES = [(c, a) for c in plr.CASES for a in plr.ARITHMETICS]
IDS = [f'{plr.case_id(c)}-{a}' for c, a in CASES]
B1 = [(c, a) for c in plr.B1_CASES for a in plr.ARITHMETICS]
B1_IDS = [f'{plr.case_id(c)}-B1-{a}' for c, a in B1]
REUSE = [(64, 8, 128, '16QAM'), (256, 8, 512, 'QPSK')]


def _cplx(a):
    """[rows, 2N] float32 (re, im interleaved) -> [rows, N] complex64 (the same bits)."""
    return np.ascontiguousarray(a, dtype=F32).view(np.complex64)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_route(cfg, gemm):
    import amp_native as nat
    d = cfg.dims()
    k = min(d.n, d.N)
    assert nat.lib().amp_vamp_select_engine(C.byref(d), k, nat.ENGINE_PERSISTENT) == nat.ENGINE_PERSISTENT
    assert nat.lib().amp_vamp_select_gemm_k(C.byref(d), k, gemm, cfg.K) == gemm
    return k


def ytil_stored(gemm, cfg) -> bool:
    """Whether the forward leaves y~ in the workspace: every path but the fp16x2 engine's in-kernel
    prologue at n = 2N (amp_vamp.hip vamp_persist_prepare)."""
    return not (gemm == plr.GEMM_H2 and cfg.Nr * cfg.Lout == 2 * cfg.Nt * cfg.Lin)


def capture(device, case, gemm, batch=plr.B, iters=plr.ITERS, det=None, y=None, chan=None):
    """One forward with the state dump on.  Returns the valid rows of the dumped planes per
    iteration (w, r: split-precision arithmetics only; xmmse, var), the dumped 1 / sigma2 of every
    workgroup, y~ where the forward stored it, the outputs and the status record."""
    import amp_native as nat
    from vamp import VAMP
    cfg = plr.make_config(case, batch, iters)
    k = _assert_route(cfg, gemm)
    nt = cfg.Nt * cfg.Lin
    inp = plr.inputs(case, batch)
    if chan is None:
        chan = tuple(inp.t[n].to(device) for n in ('U', 's', 'Vh'))
    y = inp.t['y'].to(device) if y is None else y
    nwg = (batch + plr.PBM - 1) // plr.PBM
    dump = torch.zeros(iters, nwg, 5, plr.PBM, 2 * nt, dtype=torch.float32, device=device)
    det = det or VAMP(cfg, engine=nat.ENGINE_PERSISTENT, gemm=gemm)
    nat.check(nat.lib().amp_vamp_debug_dump(C.c_void_p(dump.data_ptr())), 'amp_vamp_debug_dump')
    try:
        T = det.detect(chan[0], chan[1], chan[2], y, inp.SNR)
        torch.cuda.synchronize()
    finally:
        nat.lib().amp_vamp_debug_dump(None)
    d = dump.cpu().numpy()
    off = (C.c_uint64 * 5)()
    dims = cfg.dims()
    nat.check(nat.lib().amp_vamp_debug_offsets(C.byref(dims), k, iters, 1, off), 'amp_vamp_debug_offsets')
    ytil = None
    if ytil_stored(gemm, cfg):
        raw = T.buf.ws[int(off[4]):int(off[4]) + batch * 2 * k * 4].cpu().numpy().view(F32).reshape(batch, 2 * k)
        ytil = _cplx(raw.copy())
    rows = [min(plr.PBM, batch - w * plr.PBM) for w in range(nwg)]
    valid = lambda p: np.concatenate([d[:, w, p, :rows[w]] for w in range(nwg)], axis=1)   # noqa: E731
    out = lambda t, cols: t.detach().cpu().contiguous().view(torch.float32).numpy().reshape(-1, cols).copy()   # noqa: E731
    return SimpleNamespace(cfg=cfg, case=case, gemm=gemm, batch=batch, iters=iters, nt=nt, k=k, status=T.status(),
                           w=valid(0), r=valid(1), x=valid(2), var=valid(3)[:, :, :nt], inv=d[:, :, 3, 1, nt],
                           ytil=ytil, out_r=out(T.buf.r, 2 * nt), out_x=out(T.buf.xmmse, 2 * nt),
                           out_var=out(T.buf.var, nt), y=y.cpu().numpy()[..., 0], det=det, chan=chan)


def check_scalars(cap):
    """Assertions 1 (status) and 2; returns the chain (record t drives iteration t)."""
    st, iters = cap.status, cap.iters
    assert st.T == iters and st.nan_state == 0 and st.gemm == cap.gemm, (st.T, st.nan_state, st.gemm, cap.gemm)
    for name in ('x', 'var'):
        assert not np.isnan(getattr(cap, name)).any(), name
    inp = plr.inputs(cap.case, cap.batch)
    pb = plr.problem(cap.case, inp)
    means = [plr.mean_var_f32(cap.var[t]) for t in range(iters)]
    chain = plr.scalar_chain(pb.s2, pb.noise_var, pb.p, pb.eta, means)
    for t in range(iters):
        want = F32(chain[t].inv_sigma2)
        assert np.all(_bits(cap.inv[t]) == _bits(want)), (t, cap.inv[t], want)
    last = chain[iters - 1]
    # the record of a forward that ran to the cap: sigma2_tilde, alpha, sigma2 that drove the last
    # iteration and the dxdr it left (on an allclose stop at the cap: the one it was driven by)
    dx = last.dxdr_prev if st.stopped else last.dxdr
    want = np.array([last.s2t32, last.alpha, last.sigma2, dx], dtype=F32)
    got = np.array(list(st.last_scalar), dtype=F32)
    assert np.array_equal(_bits(got), _bits(want)), (got, want)
    return pb, chain


def _tracker_state(pb, shape):
    return np.full(shape, F32(pb.p), dtype=np.complex64), np.zeros(shape, dtype=np.complex64)


def _bar(recs, who):
    bad = [r for r in recs if not (r.rms <= plr.K_RMS and r.max <= plr.K_MAX)]
    assert not bad, f'{who}: ' + '; '.join(f'{r.phase} t={r.t} e_rms x{r.rms:.2f} e_max x{r.max:.2f}' for r in bad)


def _rec(phase, t, got, yard, ref):
    mx, rms, g, y = plr.ratios(got, yard, ref)
    return SimpleNamespace(phase=phase, t=t, max=mx, rms=rms, got=g, yard=y)


def _show(who, recs):
    for r in recs:
        print(f'{who} {r.phase:4s} t={r.t}: e_rms {r.got[1]:.3e} (numpy {r.yard[1]:.3e}, x{r.rms:.2f})  '
              f'e_max {r.got[0]:.3e} (numpy {r.yard[0]:.3e}, x{r.max:.2f})')


def measure_split(cap, who=''):
    """Assertions 1-5 of a split-precision forward; returns the records of 3-5 (asserted by _bar)."""
    pb, chain = check_scalars(cap)
    for name in ('w', 'r'):
        assert not np.isnan(getattr(cap, name)).any(), name
    inp = plr.inputs(cap.case, cap.batch)
    recs = []
    y64 = plr.ytil_f64(inp.U, inp.s, cap.y)
    pad = plr.PBM                                          # a B = 1 batch: the yardstick's products stay GEMMs
    yc = plr.ytil_c64(inp.U, inp.s, cap.y, pad)
    if cap.ytil is not None:
        assert not np.isnan(cap.ytil).any()
        recs.append(_rec('y~', 0, cap.ytil, yc, y64))
    yk = cap.ytil if cap.ytil is not None else y64        # GEMM1's y~ input (float64 where none is stored)
    for t in range(cap.iters):
        it = chain[t]
        x, r = (_cplx(cap.x[t - 1]), _cplx(cap.r[t - 1])) if t else _tracker_state(pb, (cap.batch, cap.nt))
        rt64 = plr.rt_f64(x, r, it.dxdr_prev, it.ns_prev)
        rtc = plr.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        w = _cplx(cap.w[t])
        w64 = plr.w_f64(rt64, inp.Vh, yk, pb.s2_64, it.vr)
        wc = plr.w_c64(rtc, inp.Vh, cap.ytil if cap.ytil is not None else yc, pb.s2, it.vr, pad)
        recs.append(_rec('w', t, w, wc, w64))
        r64 = plr.r_f64(w, inp.Vh, rt64, it.alpha)         # the kernel's own w
        rc = plr.r_c64(w, inp.Vh, rtc, it.alpha, pad)
        recs.append(_rec('r', t, _cplx(cap.r[t]), rc, r64))
    # the outputs are the last iteration's state
    assert np.array_equal(_bits(cap.out_r), _bits(cap.r[-1]))
    assert np.array_equal(_bits(cap.out_x), _bits(cap.x[-1])) and np.array_equal(_bits(cap.out_var), _bits(cap.var[-1]))
    _show(who, recs)
    return recs


def measure_f32(device, case, batch=plr.B, who=''):
    """Assertion 6: forwards of 1 .. ITERS iterations of the f32 class."""
    caps = [capture(device, case, plr.GEMM_F32, batch, iters) for iters in range(1, plr.ITERS + 1)]
    full = caps[-1]
    inp = plr.inputs(case, batch)
    recs = []
    for cap in caps:
        pb, chain = check_scalars(cap)
        assert not np.isnan(cap.out_r).any()
        # prefix consistency: this forward is the first cap.iters iterations of the longest one
        t = cap.iters - 1
        assert np.array_equal(_bits(cap.ytil), _bits(full.ytil)), cap.iters
        assert np.array_equal(_bits(cap.out_x), _bits(full.x[t])), cap.iters
        assert np.array_equal(_bits(cap.out_var), _bits(full.var[t])), cap.iters
        assert np.array_equal(_bits(cap.inv[:, 0]), _bits(full.inv[:cap.iters, 0])), cap.iters
    y64 = plr.ytil_f64(inp.U, inp.s, full.y)
    recs.append(_rec('y~', 0, full.ytil, plr.ytil_c64(inp.U, inp.s, full.y, plr.PBM), y64))
    for t in range(plr.ITERS):
        it = chain[t]
        if t:
            x, r = _cplx(caps[t - 1].out_x), _cplx(caps[t - 1].out_r)
        else:
            x, r = _tracker_state(pb, (batch, full.nt))
        rt64 = plr.rt_f64(x, r, it.dxdr_prev, it.ns_prev)
        rtc = plr.rt_c64(x, r, it.dxdr_prev, it.ns_prev)
        r64 = plr.r_f64(plr.w_f64(rt64, inp.Vh, full.ytil, pb.s2_64, it.vr), inp.Vh, rt64, it.alpha)
        rc = plr.r_c64(plr.w_c64(rtc, inp.Vh, full.ytil, pb.s2, it.vr, plr.PBM), inp.Vh, rtc, it.alpha, plr.PBM)
        recs.append(_rec('w+r', t, _cplx(caps[t].out_r), rc, r64))
    _show(who, recs)
    return recs


def measure(device, case, arith, batch=plr.B):
    who = f'{plr.case_id(case)} B={batch} {arith}'
    gemm = plr.ARITHMETICS[arith]
    if gemm == plr.GEMM_F32:
        return measure_f32(device, case, batch, who)
    return measure_split(capture(device, case, gemm, batch), who)


@pytest.mark.parametrize('case,arith', CASES, ids=IDS)
def test_linear_half_against_float64(device, case, arith):
    _bar(measure(device, case, arith), f'{plr.case_id(case)} {arith}')


@pytest.mark.parametrize('case,arith', B1, ids=B1_IDS)
def test_single_valid_row(device, case, arith):
    """B = 1: one workgroup with one valid row (15 padded rows beside it in every MFMA tile)."""
    _bar(measure(device, case, arith, batch=1), f'{plr.case_id(case)} B=1 {arith}')


def measure_reuse(device, case):
    """bf16x3: a building forward and the reuse forward after it on the same channel objects with a
    new y (iteration 0 takes q = Vh r~ from the stored q0: no GEMM1); both checked like any forward."""
    import amp_native as nat
    who = f'{plr.case_id(case)} bf16x3'
    c0 = nat.prepare_counts()
    built = capture(device, case, plr.GEMM_X3)
    c1 = nat.prepare_counts()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (1, 0), (c0, c1)
    recs = measure_split(built, who + ' building')
    y2 = torch.roll(plr.inputs(case).t['y'], 1, 0).contiguous().to(device)      # the rows' trials, shifted by one
    reused = capture(device, case, plr.GEMM_X3, det=built.det, y=y2, chan=built.chan)
    c2 = nat.prepare_counts()
    assert (c2[0] - c1[0], c2[1] - c1[1]) == (0, 1), (c1, c2)
    assert not np.array_equal(_bits(reused.w[0]), _bits(built.w[0]))              # a new y reached iteration 0
    return recs, measure_split(reused, who + ' reuse')


@pytest.mark.parametrize('case', REUSE, ids=[plr.case_id(c) for c in REUSE])
def test_reuse_forward_against_float64(device, case):
    built, reused = measure_reuse(device, case)
    _bar(built, f'{plr.case_id(case)} building')
    _bar(reused, f'{plr.case_id(case)} reuse')
