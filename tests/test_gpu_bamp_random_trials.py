"""generator_mode='random' trial batches on the GPU: BAMP(config, random_trials=True).forward_trials
(amp_bamp_random_trials_run) against sequential BAMP(config).forward calls (amp_bamp_run with the
element-wise denoiser + amp_random_decide_count), at the shapes of tests/bamp_random_trials_inputs.py:
(32, 4, 12, 3, 2) 16-QAM (N = 96, n = 48, a partial last column tile), (64, 4, 16, 5, 2) QPSK
(2N = 640: several column tiles, so several partial slots per row) and (6, 3, 5, 3, 1) QPSK
(N % 4 == 2, odd n).  Per shape 33 channels, messages and noise vectors drawn once.

1. bit-equality: E = 33 trials on one channel, then per_channel R in {1, 5, 33} with ceil(33 / R)
   channels: every trial's xmap, xmmse and var are BIT-equal to the forward of that trial alone with
   its channel; T, nan_state, every counter and every key of Loss.loss are equal;
2. isolation: one trial's y scaled by 1e20, another given y = A x exactly (no noise: its exit does
   not depend on the SNR), a third all NaN: every other trial keeps the bits of the clean call, the
   three equal their own sequential forwards (a stopped trial's outputs are those of its iteration
   T_e), the NaN trial runs to the last iteration.  (With the element-wise denoiser a 1e20 input need
   not turn NaN: every G(a_k) underflows, regularize_zero sets the normaliser to 1e-9 (bamp.py:90-92)
   and xmmse and var become 0; what it did is printed, the NaN trial is there for the non-finite case.)
3. max_iter = 1 and 2 return the first iterations' values: equal to sequential forwards of 1 and 2
   iterations;
4. every Loss reports arithmetic 'f32' (amp_status[e].gemm == AMP_ARITH_F32);
5. g20: forward_trials over each point's 40 trials equals the sequential GPU forwards exactly, and
   at most 1 of the 40 trials differs from the reference's stored ver / ser (the allowance
   test_gpu_random.py gives this mode: at B = 1 the exit is decided by GEMM rounding; the oracle
   alone differs in 0).
"""
import functools

import numpy as np
import pytest
import torch

import bamp_random_trials_inputs as ri
import golden_io as gio

pytestmark = pytest.mark.gpu

E = ri.E


def _det(name, iterations=20, trials=True):
    from bamp import BAMP
    cfg = ri.shape_config(name, device='cuda', iterations=iterations)
    return BAMP(cfg, random_trials=True) if trials else BAMP(cfg)


def _record(L):
    from loss import counts_to_vector
    assert L.arithmetic == 'f32'                                                    # 4.
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _forward(det, inp, e, A, y):
    """One sequential B = 1 forward of trial e with channel A: (T, counters, metrics, nan_state, xmap, xmmse, var)."""
    L = det(A, y, inp['SNR'], inp['x'][e], inp['sym'][e], inp['idx'][e])
    rec = _record(L)
    b = det.last.buf
    return rec + (b.xmap.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.var.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def _seq_detector(name, iterations=20):
    return _det(name, iterations, trials=False)


@functools.lru_cache(maxsize=None)
def sequential(name, e, g, iterations=20):
    """Trial e through channel g as a sequential forward.  Computed once, shared, never modified."""
    inp = ri.shape_point(name)
    return _forward(_seq_detector(name, iterations), inp, e, inp['A'][g], ri.received(inp, e, g))


def _grouped(det, inp, chans, ys, R):
    kw = {} if R is None else dict(per_channel=R)
    Ls = det.forward_trials(chans, ys, inp['SNR'], inp['x'], inp['sym'], inp['idx'], **kw)
    recs = [_record(L) for L in Ls]
    xmap, xm, var = (t.reshape(len(ys), -1) for t in det.last_trials)
    return recs, xmap, xm, var


@functools.lru_cache(maxsize=None)
def grouped(name, R, iterations=20):
    """Trials 0 .. 32 in one call: R None, one channel (channel 0, a single matrix); else trial e through
    channel e // R."""
    inp = ri.shape_point(name)
    if R is None:
        return _grouped(_det(name, iterations), inp, inp['A'][0], [ri.received(inp, e, 0) for e in range(E)], None)
    G = -(-E // R)
    return _grouped(_det(name, iterations), inp, inp['A'][:G], [ri.received(inp, e, e // R) for e in range(E)], R)


def _differences(rec, bufs, ref):
    from loss import COUNT_FIELDS
    d = {}
    if rec[0] != ref[0]:
        d['T'] = (rec[0], ref[0])
    for f, a, b in zip(COUNT_FIELDS, rec[1], ref[1]):
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d[f] = (a, b)
    for k in gio.LOSS_KEYS:
        a, b = rec[2][k], ref[2][k]
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d['loss.' + k] = (a, b)
    if rec[3] != ref[3]:
        d['nan_state'] = (rec[3], ref[3])
    for key, got, want in zip(('xmap', 'xmmse', 'var'), bufs, ref[4:7]):
        if not gio.bits_equal(got, want):
            d[key] = 'bits differ'
    return d


@pytest.mark.parametrize('R', [None, 1, 5, 33])
@pytest.mark.parametrize('name', sorted(ri.SHAPES))
def test_random_trials_equal_sequential_forwards(device, name, R):                  # 1.
    recs, xmap, xm, var = grouped(name, R)
    bad = {}
    for e in range(E):
        d = _differences(recs[e], (xmap[e], xm[e], var[e]), sequential(name, e, 0 if R is None else e // R))
        if d:
            bad[e] = d
    print(name, R, 'T', [r[0] for r in recs])
    assert not bad, bad


@pytest.mark.parametrize('name', sorted(ri.SHAPES))
def test_random_trials_are_isolated(device, name):                                   # 2.
    R, huge, exact, nan = 5, 7, 12, 21                       # rows of different channels of the first tile
    base_recs, bxmap, bxm, bvar = grouped(name, R)
    inp = ri.shape_point(name)
    ys = [ri.received(inp, e, e // R) for e in range(E)]
    ys[huge] = ys[huge] * 1e20
    ys[exact] = inp['A'][exact // R] @ inp['x'][exact]
    ys[nan] = ys[nan] * float('nan')
    recs, xmap, xm, var = _grouped(_det(name), inp, inp['A'][:-(-E // R)], ys, R)
    det = _det(name, trials=False)
    bad = {}
    for e in range(E):
        if e in (huge, exact, nan):
            ref = _forward(det, inp, e, inp['A'][e // R], ys[e])
        else:
            ref = base_recs[e] + (bxmap[e], bxm[e], bvar[e])
        d = _differences(recs[e], (xmap[e], xm[e], var[e]), ref)
        if d:
            bad[e] = d
    print(name, 'huge: T', recs[huge][0], 'var finite', bool(torch.isfinite(var[huge]).all()), 'xmap finite',
          bool(torch.isfinite(torch.view_as_real(xmap[huge])).all()), '| exact: T', recs[exact][0], '| nan: T', recs[nan][0])
    assert not bad, bad
    assert torch.isnan(var[nan]).all() and recs[nan][0] == 20      # never allclose: it runs to the last iteration
    assert min(r[0] for r in recs) < 20                             # some trial left early, frozen at its T_e


@pytest.mark.parametrize('iterations', [1, 2])
@pytest.mark.parametrize('name', sorted(ri.SHAPES))
def test_random_trials_first_iterations(device, name, iterations):                  # 3.
    R = 5
    recs, xmap, xm, var = grouped(name, R, iterations)
    bad = {}
    for e in range(E):
        assert recs[e][0] == iterations
        d = _differences(recs[e], (xmap[e], xm[e], var[e]), sequential(name, e, e // R, iterations))
        if d:
            bad[e] = d
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def _golden(name):
    """(grouped records, sequential records) of a g20 point's 40 trials on its one channel."""
    from bamp import BAMP
    h = ri.golden_inputs(name)
    inp = dict(h)
    inp['x'] = [t.cuda() for t in h['x']]
    A = h['A'].cuda()
    ys = [t.cuda() for t in h['y']]
    cfg = ri.golden_config(name, device='cuda')
    recs, xmap, xm, var = _grouped(BAMP(cfg, random_trials=True), inp, A, ys, None)
    det = BAMP(cfg)
    seq = [_forward(det, inp, e, A, ys[e]) for e in range(ri.E_G20)]
    return recs, (xmap, xm, var), seq


@pytest.mark.parametrize('name', ri.POINTS)
def test_random_trials_g20(device, name):                                            # 5.
    recs, (xmap, xm, var), seq = _golden(name)
    bad = {}
    for e in range(ri.E_G20):
        d = _differences(recs[e], (xmap[e], xm[e], var[e]), seq[e])
        if d:
            bad[e] = d
    assert not bad, bad
    ref = ri.G20[name]['trials']
    differs = [e for e in range(ri.E_G20)
               if recs[e][2]['ver'] != ref[e]['ver'] or recs[e][2]['ser'] != ref[e]['ser']]
    tdiff = [e for e in range(ri.E_G20) if recs[e][0] != int(ref[e]['T'])]
    print(name, 'trials whose ver / ser differ from the reference:', differs, '| whose T differs:', tdiff)
    assert len(differs) <= 1, differs
