"""SCAMP independent-trial batches on the GPU: SCAMP.forward_trials (amp_scamp_trials_run) at the
three g14 points (tests/golden/make_g14_scamp_trials.py).  scamp_OOK_Nt128 has 2 Nt > the A^H
column tile: the split-psi kernel and the block-banded GEMMs.

1. against sequential B = 1 forwards of the launch engine on the same inputs (E = 40: a ragged
   second row tile; also E = 33 and E = 1): T_e, every counter and nan_state equal for every trial,
   xmap / xmmse / psi BIT-equal (an MFMA output row reduces its own A row only, every epilogue
   value is formed per row in the sequential kernels' order);
2. against g14 (the reference at batch = 1): counting metrics per trial, at most 1 of 40 trials
   may differ per point (the convention of test_gpu_segmented.py::test_segmented_detectors_b1);
3. isolation: trial 5's y scaled by 1e6, or set to NaN, leaves every other trial's T, counters and
   xmap / xmmse / psi bit-equal, and the victim equal to its own sequential forward;
4. frozen psi: trials exit at odd and at even T, every psi bit-equal to the sequential forward's;
5. the 'sparc' rule at scamp_QPSK_Nt32;
6. every Loss reports arithmetic 'f32';
7. the exact float64 fix-up: a victim scaled so that its LAST iteration leaves some, not all, of
   its sections NaN (sections beyond the float64 range of the trial's own max|xi| shift; the
   scale and iteration count per point were found by a sweep) is bit-equal to its own sequential
   forward, as are its seven neighbours.
"""
import functools

import numpy as np
import pytest
import torch

import golden_io as gio
import scamp_trials_inputs as si

pytestmark = pytest.mark.gpu

E = si.E_G14
VICTIM = 5                                     # a row inside the first tile, among live neighbours


def _detector(name, mode='segmented', iterations=None):
    import amp_native as nat
    from scamp import SCAMP
    return SCAMP(si.config_of(name, device='cuda', mode=mode, iterations=iterations), engine=nat.ENGINE_LAUNCHES)


def _record(L):
    from loss import counts_to_vector
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _forward(det, inp, j, y):
    """One sequential B = 1 forward: (T, counters, metrics, nan_state, xmap, xmmse, psi)."""
    L = det(inp['W'], inp['A'], y, inp['SNR'], inp['x'][j], inp['sym'][j], inp['idx'][j])
    rec = _record(L)
    b = det.last.buf
    return rec + (b.xmap.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.psi.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def sequential(name, mode='segmented'):
    """The 40 trials as sequential B = 1 forwards of the launch engine.  Computed once, shared,
    never modified."""
    det = _detector(name, mode)
    inp = si.device_inputs(name)
    return [_forward(det, inp, j, inp['y'][j]) for j in range(E)]


def _trials(name, ids, ys=None, mode='segmented', iterations=None):
    det = _detector(name, mode, iterations)
    inp = si.device_inputs(name)
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(inp['W'], inp['A'], ys if ys is not None else pick(inp['y']), inp['SNR'], pick(inp['x']),
                            pick(inp['sym']), pick(inp['idx']))
    recs = [_record(L) for L in Ls]
    assert all(L.arithmetic == 'f32' for L in Ls)                           # 6.
    xmap, xm, psi = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, xmap, xm, psi


@functools.lru_cache(maxsize=None)
def grouped40(name):
    return _trials(name, tuple(range(E)))


def _count_fields():
    from loss import COUNT_FIELDS
    return COUNT_FIELDS


def _differences(rec, bufs, ref):
    """Keys on which one trial (record, (xmap, xmmse, psi) rows) differs from a sequential forward."""
    d = {}
    if rec[0] != ref[0]:
        d['T'] = (rec[0], ref[0])
    for f, a, b in zip(_count_fields(), rec[1], ref[1]):
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d[f] = (a, b)
    if rec[3] != ref[3]:
        d['nan_state'] = (rec[3], ref[3])
    if bufs is not None:
        for key, got, want in zip(('xmap', 'xmmse', 'psi'), bufs, ref[4:7]):
            if not gio.bits_equal(got, want):
                d[key] = 'bits differ'
    return d


@pytest.mark.parametrize('nE', [40, 33, 1])
@pytest.mark.parametrize('name', si.POINTS)
def test_scamp_trials_equal_sequential_forwards(device, name, nE):
    seq = sequential(name)
    recs, xmap, xm, psi = grouped40(name) if nE == 40 else _trials(name, tuple(range(nE)))
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (xmap[j], xm[j], psi[j]), seq[j])
        if d:
            bad[j] = d
    print(name, nE, 'T', [r[0] for r in recs])
    assert not bad, bad


@pytest.mark.parametrize('name', si.POINTS)
def test_scamp_trials_match_reference_g14(device, name):
    recs = grouped40(name)[0]
    ref = si.G14[name]['trials']
    diff = {}
    for j in range(E):
        d = {k: (recs[j][2][k], ref[j][k]) for k in gio.COUNT_KEYS if recs[j][2][k] != ref[j][k]}
        if d:
            diff[j] = d
    tdiff = [(j, recs[j][0], int(ref[j]['T'])) for j in range(E) if recs[j][0] != int(ref[j]['T'])]
    print(name, 'trials whose counting metrics differ from the reference:', len(diff))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert len(diff) <= 1, diff


@pytest.mark.parametrize('kind', ['huge', 'nan'])
@pytest.mark.parametrize('name', si.POINTS)
def test_scamp_trials_isolated_from_a_bad_trial(device, name, kind):
    base_recs, bxmap, bxm, bpsi = grouped40(name)
    inp = si.device_inputs(name)
    ys = list(inp['y'])
    ys[VICTIM] = ys[VICTIM] * 1e6 if kind == 'huge' else torch.full_like(ys[VICTIM], float('nan'))
    recs, xmap, xm, psi = _trials(name, tuple(range(E)), ys=ys)
    bad = {}
    for j in range(E):
        if j == VICTIM:
            continue
        d = []
        if recs[j][0] != base_recs[j][0]:
            d.append(('T', recs[j][0], base_recs[j][0]))
        if not np.array_equal(recs[j][1], base_recs[j][1], equal_nan=True):
            d.append('counters')
        for key, a, b in (('xmap', xmap[j], bxmap[j]), ('xmmse', xm[j], bxm[j]), ('psi', psi[j], bpsi[j])):
            if not gio.bits_equal(a, b):
                d.append(key)
        if d:
            bad[j] = d
    assert not bad, bad
    # the victim is its own sequential forward on the same modified y
    own = _forward(_detector(name), inp, VICTIM, ys[VICTIM])
    d = _differences(recs[VICTIM], None, own)
    print(name, kind, 'victim T', recs[VICTIM][0], 'nan_state', recs[VICTIM][3])
    assert not d, d
    if kind == 'nan':
        assert bool(torch.isnan(psi[VICTIM]).all()) and recs[VICTIM][0] == si.G14[name]['iterations']


@pytest.mark.parametrize('name', si.POINTS)
def test_scamp_trials_frozen_psi_at_odd_and_even_exits(device, name):
    seq = sequential(name)
    recs, _, _, psi = grouped40(name)
    Ts = [r[0] for r in recs]
    assert any(t % 2 for t in Ts) and any(t % 2 == 0 for t in Ts), Ts      # both ping-pong buffers
    bad = [(j, Ts[j]) for j in range(E) if not gio.bits_equal(psi[j], seq[j][6])]
    assert not bad, bad


def test_scamp_trials_sparc_rule(device):
    """generator_mode='sparc' (the MAP rule, loss.py:282-302) per trial."""
    name = 'scamp_QPSK_Nt32'
    seq = sequential(name, 'sparc')
    recs = _trials(name, tuple(range(E)), mode='sparc')[0]
    bad = {j: (recs[j][0], seq[j][0]) for j in range(E)
           if recs[j][0] != seq[j][0] or not np.array_equal(recs[j][1], seq[j][1], equal_nan=True)}
    assert not bad, bad


@pytest.mark.parametrize('name,iterations,scale', [('scamp_OOK_Nt128', 3, 14.0), ('scamp_OOK_Nt16', 2, 30.0),
                                                   ('scamp_QPSK_Nt32', 1, 300.0)])
def test_scamp_trials_exact_fixup_of_one_trial(device, name, iterations, scale):
    nE = 8
    inp = si.device_inputs(name)
    ys = list(inp['y'][:nE])
    ys[VICTIM] = ys[VICTIM] * scale
    recs, xmap, xm, psi = _trials(name, tuple(range(nE)), ys=ys, iterations=iterations)
    nan = int(torch.isnan(xm[VICTIM].real).sum())
    print(name, 'victim T', recs[VICTIM][0], 'nan_state', recs[VICTIM][3], 'NaN entries', nan, 'of', xm.shape[1])
    assert recs[VICTIM][3] == 1 and 0 < nan < xm.shape[1]          # the fix-up ran, not the all-NaN rule
    det = _detector(name, iterations=iterations)
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (xmap[j], xm[j], psi[j]), _forward(det, inp, j, ys[j]))
        if d:
            bad[j] = d
    assert not bad, bad
