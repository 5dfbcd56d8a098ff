"""The forwards of the per-iteration BAMP / SCAMP GPU tests (test_gpu_bamp_iter.py,
test_gpu_scamp_iter.py, test_gpu_scamp_persist_iter.py, tools/launch_iter_err.py): the state after
iteration t is the output of a forward of t iterations through the detectors' public contract."""
import ctypes as C

import numpy as np
import torch

import launch_iter_ref as lir

ENGINE_NAMES = {lir.ENGINE_LAUNCHES: 'launches', lir.ENGINE_PERSISTENT: 'persistent'}


def _np(t):
    return t.detach().cpu().numpy().copy()


def bamp_forward(device, case, gemm, iterations):
    """One BAMP forward of `iterations` iterations: ((xmap, xmmse, var), status)."""
    from bamp import BAMP
    inp = lir.inputs(case)
    det = BAMP(lir.make_config(case, iterations), gemm=gemm)
    T = det.detect(inp.t['A'].to(device), inp.t['y'].to(device), inp.SNR)
    torch.cuda.synchronize()
    return (_np(T.buf.xmap), _np(T.buf.xmmse), _np(T.buf.var)), T.status()


def scamp_forward(device, case, gemm, iterations, engine):
    """One SCAMP forward of `iterations` iterations on `engine`: ((xmap, xmmse, psi), status)."""
    import amp_native as nat
    from scamp import SCAMP
    inp = lir.inputs(case)
    cfg = lir.make_config(case, iterations)
    d = cfg.dims()
    assert nat.lib().amp_scamp_select_engine(C.byref(d), engine) == engine
    det = SCAMP(cfg, engine=engine, gemm=gemm)
    T = det.detect(inp.t['W'].to(device), inp.t['A'].to(device), inp.t['y'].to(device), inp.SNR)
    torch.cuda.synchronize()
    return (_np(T.buf.xmap), _np(T.buf.xmmse), _np(T.buf.psi)), T.status()


def sweep(forward, gemm, last=lir.T):
    """The state after iterations 1 .. last; every forward ran to its cap on the arithmetic asked
    for, without an exit, a NaN state or a NaN."""
    outs = []
    for t in range(1, last + 1):
        out, st = forward(t)
        assert (st.T, st.stopped, st.nan_state, st.gemm) == (t, 0, 0, gemm), (t, st.T, st.stopped, st.nan_state, st.gemm)
        assert not any(np.isnan(a).any() for a in out), t
        outs.append(out)
    return outs


def measure_bamp(device, case, gemm):
    who = f'bamp launches {lir.case_id(case)} {lir.ARITH_NAMES[gemm]}'
    lin, den = lir.bamp_records(case, sweep(lambda t: bamp_forward(device, case, gemm, t), gemm))
    lir.show(who, lin, den)
    return who, lin, den


def measure_scamp(device, case, gemm, engine):
    who = f'scamp {ENGINE_NAMES[engine]} {lir.case_id(case)} {lir.ARITH_NAMES[gemm]}'
    lin, den = lir.scamp_records(case, sweep(lambda t: scamp_forward(device, case, gemm, t, engine), gemm))
    lir.show(who, lin, den)
    return who, lin, den


def check_exit(forward, bitwise: bool):
    """forward(iterations) -> ((xmap, xmmse, var | psi), status).  The EXIT_ITERS-iteration forward
    stops by allclose at the first t at which oracle.allclose_f32 holds between the outputs of the
    forwards of t and t - 1 iterations (ones before the first); bitwise: the forward of T iterations
    equals it bit for bit."""
    full, st = forward(lir.EXIT_ITERS)
    assert st.stopped == 1 and st.nan_state == 0 and 1 < st.T < lir.EXIT_ITERS, (st.T, st.stopped, st.nan_state)
    outs = []
    for t in range(1, st.T + 1):
        out, s = forward(t)
        assert s.T == t and s.nan_state == 0, (t, s.T)
        outs.append(out)
    assert lir.first_close([o[2] for o in outs], np.ones_like(outs[0][2])) == st.T
    if bitwise:
        for a, b in zip(outs[-1], full):
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    return st.T
