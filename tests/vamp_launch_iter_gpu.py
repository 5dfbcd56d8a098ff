"""The forwards of the per-iteration VAMP launch-engine GPU test (test_gpu_vamp_launch_iter.py,
tools/vamp_launch_iter_err.py): the state after iteration t is a forward of t + 1 iterations through
VAMP(cfg, engine=ENGINE_LAUNCHES) with its workspace's y~ and w read back."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

import vamp_launch_iter_ref as vir

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cplx(t, cols):
    """A device tensor -> [rows, cols] complex64 on the host (the same bits)."""
    return t.detach().cpu().contiguous().view(torch.float32).numpy().reshape(-1, 2 * cols).copy().view(np.complex64)


def _f32(t, cols):
    return t.detach().cpu().contiguous().view(torch.float32).numpy().reshape(-1, cols).copy()


def workspace_planes(ws, dims, k, iterations, rows, with_ytil=True):
    """(y~ [rows, k] complex64 or None, w [rows, k] complex64, w's pad floats [rows, wld - 2k]) of a
    launch-engine workspace (amp_vamp_debug_offsets[4], amp_vamp_debug_launch_offsets)."""
    import amp_native as nat
    off = (C.c_uint64 * 5)()
    nat.check(nat.lib().amp_vamp_debug_offsets(C.byref(dims), k, iterations, 1, off), 'amp_vamp_debug_offsets')
    lo = (C.c_uint64 * 3)()
    nat.check(nat.lib().amp_vamp_debug_launch_offsets(C.byref(dims), k, iterations, lo), 'amp_vamp_debug_launch_offsets')
    wld = int(lo[1])
    assert wld == (2 * k + 3) // 4 * 4 and int(lo[0]) % 16 == 0
    host = lambda o, n: ws[int(o):int(o) + 4 * n].cpu().numpy().view(F32).copy()   # noqa: E731
    ytil = host(off[4], rows * 2 * k).reshape(rows, 2 * k).view(np.complex64) if with_ytil else None
    wraw = host(lo[0], rows * wld).reshape(rows, wld)
    return ytil, np.ascontiguousarray(wraw[:, :2 * k]).view(np.complex64), wraw[:, 2 * k:]


def forward(device, case, iterations):
    """One forward of `iterations` iterations on the launch engine (gemm AUTO): r, x, var, w, w's pad,
    y~ and the status record."""
    import amp_native as nat
    from vamp import VAMP
    g = vir.geometry(case)
    cfg = vir.make_config(case, iterations)
    d = cfg.dims()
    assert (d.N, d.n) == (g.N, g.n)
    assert nat.lib().amp_vamp_select_engine(C.byref(d), g.k, nat.ENGINE_LAUNCHES) == nat.ENGINE_LAUNCHES
    inp = vir.inputs(case)
    U, s, Vh, y = (inp.t[n].to(device) for n in ('U', 's', 'Vh', 'y'))
    T = VAMP(cfg, engine=nat.ENGINE_LAUNCHES, gemm=nat.GEMM_AUTO).detect(U, s, Vh, y, inp.SNR)
    torch.cuda.synchronize()
    ytil, w, pad = workspace_planes(T.buf.ws, d, g.k, iterations, case.B)
    return SimpleNamespace(r=_cplx(T.buf.r, g.N), x=_cplx(T.buf.xmmse, g.N), var=_f32(T.buf.var, g.N), w=w, pad=pad,
                           ytil=ytil, status=T.status())


def check_forward(fw, iterations, stopped=0):
    """Assertion 1 of one forward: it ran `iterations` iterations on f32 tiles, no NaN state, no NaN
    anywhere, and w's pad floats are exactly 0."""
    st = fw.status
    assert (st.T, st.stopped, st.nan_state, st.gemm) == (iterations, stopped, 0, vir.GEMM_F32), \
        (iterations, st.T, st.stopped, st.nan_state, st.gemm)
    for name in ('r', 'x', 'var', 'w') + (('ytil',) if fw.ytil is not None else ()):
        assert not np.isnan(getattr(fw, name)).any(), (iterations, name)
    assert np.all(_bits(fw.pad) == 0), (iterations, fw.pad)


def check_scalars(case, fws, var_means=None):
    """Assertion 2: the float32 chain on the engine's own var means gives every prefix forward's
    status.last_scalar bit for bit.  Returns the chain."""
    means = var_means if var_means is not None else [vir.mean_var_f32(fw.var) for fw in fws]
    chain = vir.chain_of(case, means)
    for T, fw in enumerate(fws, 1):
        want = vir.last_scalars(chain, T, fw.status.stopped)
        got = np.array(list(fw.status.last_scalar), dtype=F32)
        assert np.array_equal(_bits(got), _bits(want)), (T, got, want)
    return chain


def sweep(device, case, last=vir.ITERS):
    """The prefix forwards 1 .. last with assertion 1; y~ is the same bits in all of them."""
    fws = [forward(device, case, t) for t in range(1, last + 1)]
    for t, fw in enumerate(fws, 1):
        check_forward(fw, t)
        assert np.array_equal(_bits(fw.ytil), _bits(fws[0].ytil)), t
    return fws


def measure(device, case):
    """Assertions 1 and 2 and the records of 3 - 6 (asserted by vir.assert_bars)."""
    who = f'vamp launches {vir.case_id(case)}'
    fws = sweep(device, case)
    chain = check_scalars(case, fws)
    lin, den = vir.records(case, fws, chain)
    vir.show(who, lin, den)
    return who, lin, den


def sharded_sweep(device, monkeypatch, case=vir.SHARD_CASE, rows=vir.SHARD_ROWS, last=vir.ITERS):
    """The case as two slices of `rows` trials through ShardedVAMP (vamp_xr1 .. vamp_xr4), prefix
    forwards 1 .. last: per rank the list of the slice's states, each checked by assertion 1."""
    import shard_threads
    g = vir.geometry(case)
    inp = vir.inputs(case)
    dev_inp = dict(SNR=inp.SNR, sym=inp.sym, idx=inp.idx, **{n: inp.t[n].to(device) for n in ('U', 's', 'Vh', 'y', 'x')})
    world = case.B // rows
    assert world * rows == case.B
    per_rank = [[] for _ in range(world)]
    for t in range(1, last + 1):
        cfg = vir.make_config(case, t)

        def collect(det, L, cfg=cfg, t=t):
            torch.cuda.synchronize()
            r, xm, var = det.last_shard
            _, w, pad = workspace_planes(det._ws, cfg.dims(batch=rows), g.k, t, rows, with_ytil=False)
            return SimpleNamespace(r=_cplx(r, g.N), x=_cplx(xm, g.N), var=_f32(var, g.N), w=w, pad=pad, ytil=None,
                                   status=L.last_status)

        for rank, fw in enumerate(shard_threads.run_slices(monkeypatch, lambda t=t: vir.make_config(case, t), dev_inp,
                                                           collect, rows=rows, world=world)):
            check_forward(fw, t)
            per_rank[rank].append(fw)
    return per_rank


def measure_sharded(device, monkeypatch, case=vir.SHARD_CASE, rows=vir.SHARD_ROWS):
    """Assertions 2, 5 and 6 per slice, the var mean taken over the whole batch."""
    per_rank = sharded_sweep(device, monkeypatch, case, rows)
    means = [vir.mean_var_f32(np.concatenate([fws[t].var for fws in per_rank])) for t in range(vir.ITERS)]
    out = []
    for rank, fws in enumerate(per_rank):
        chain = check_scalars(case, fws, means)
        who = f'vamp sharded {vir.case_id(case)} rows {rank * rows}..{rank * rows + rows - 1}'
        lin, den = vir.records(case, fws, chain, rows=slice(rank * rows, rank * rows + rows), linear_half=False)
        vir.show(who, lin, den)
        out.append((who, lin, den))
    return out


def check_exit(device, case):
    """Assertion 7: the EXIT_ITERS forward stops by allclose at the first t at which
    torch_close_f32(var_t, var_{t-1}) holds everywhere on the engine's own prefix-forward outputs.
    Returns (the engine's T, the oracle's)."""
    full = forward(device, case, vir.EXIT_ITERS)
    st = full.status
    assert st.stopped == 1 and st.nan_state == 0 and 1 < st.T < vir.EXIT_ITERS, (st.T, st.stopped, st.nan_state)
    fws = [forward(device, case, t) for t in range(1, st.T + 1)]
    for t, fw in enumerate(fws, 1):
        check_forward(fw, t, stopped=1 if t == st.T else 0)
    assert vir.first_close([fw.var for fw in fws]) == st.T, (vir.first_close([fw.var for fw in fws]), st.T)
    for name in ('r', 'x', 'var'):
        assert np.array_equal(_bits(getattr(fws[-1], name)), _bits(getattr(full, name))), name
    check_scalars(case, fws)
    return int(st.T), int(vir.oracle_trace(case, vir.EXIT_ITERS)[0]['T'])
