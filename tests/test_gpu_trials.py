"""Independent-trial batches on the GPU: VAMP.forward_trials / BAMP.forward_trials
(amp_vamp_trials_run / amp_bamp_trials_run) at the four g13 points (tests/golden/make_g13_trials.py).

1. against sequential B = 1 forwards of the launch engine on the same inputs (E = 40: a ragged
   second row tile; also E = 1 and E = 33): T_e and every counter equal for every trial; with
   iterations = 1, r / xmmse / var within 2e-6 max|r| (the engine-agreement bar of
   test_gpu_vamp.py::test_vamp_engines_agree);
2. against g13 (the reference at batch = 1): counting metrics per trial, at most 1 of 40 trials
   may differ per point (the convention of test_gpu_segmented.py::test_segmented_detectors_b1);
3. isolation: one trial's y scaled by 1e6, or set to NaN, leaves every other trial's T, counters
   and r / xmmse / var bit-equal;
4. frozen outputs: trials that exit at odd and at even T return the sequential forward's var;
5. Model.simulate(group_trials=8) writes the per-epoch loop's JSON points.
"""
import functools
import json

import numpy as np
import pytest
import torch

import golden_io as gio
import trials_inputs as ti

pytestmark = pytest.mark.gpu

E = ti.E_G13


def _detector(name, iterations=None, mode='segmented'):
    import amp_native as nat
    from bamp import BAMP
    from vamp import VAMP
    cfg = ti.config_of(name, device='cuda', iterations=iterations, mode=mode)
    return VAMP(cfg, engine=nat.ENGINE_LAUNCHES) if ti.G13[name]['algo'] == 'vamp' else BAMP(cfg)


def _channel(name, inp):
    return (inp['U'], inp['s'], inp['Vh']) if ti.G13[name]['algo'] == 'vamp' else (inp['A'],)


def _record(L):
    from loss import counts_to_vector
    return int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS}


@functools.lru_cache(maxsize=None)
def sequential(name, iterations, mode='segmented'):
    """The 40 trials as sequential B = 1 forwards of the launch engine: per trial (T, counters,
    metrics, r / xmap, xmmse, var).  Computed once, shared, never modified."""
    det = _detector(name, iterations, mode)
    inp = ti.device_inputs(name)
    out = []
    for j in range(E):
        L = det(*_channel(name, inp), inp['y'][j], inp['SNR'], inp['x'][j], inp['sym'][j], inp['idx'][j])
        T, cnt, met = _record(L)
        b = det.last.buf
        dec = b.r if ti.G13[name]['algo'] == 'vamp' else b.xmap
        out.append((T, cnt, met, dec.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.var.clone().reshape(-1)))
    return out


def _trials(name, iterations, ids, ys=None, mode='segmented'):
    det = _detector(name, iterations, mode)
    inp = ti.device_inputs(name)
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(*_channel(name, inp), ys if ys is not None else pick(inp['y']), inp['SNR'], pick(inp['x']),
                            pick(inp['sym']), pick(inp['idx']))
    recs = [_record(L) for L in Ls]
    assert all(L.arithmetic == 'f32' for L in Ls)
    dec, xm, var = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, dec, xm, var


@functools.lru_cache(maxsize=None)
def grouped40(name):
    return _trials(name, None, tuple(range(E)))


@pytest.mark.parametrize('nE', [40, 1, 33])
@pytest.mark.parametrize('name', ti.POINTS)
def test_trials_equal_sequential_forwards(device, name, nE):
    seq = sequential(name, None)
    recs = grouped40(name)[0] if nE == 40 else _trials(name, None, tuple(range(nE)))[0]
    bad = {}
    for j in range(nE):
        d = {}
        if recs[j][0] != seq[j][0]:
            d['T'] = (recs[j][0], seq[j][0])
        for f, a, b in zip(_count_fields(), recs[j][1], seq[j][1]):
            if not (a == b or (np.isnan(a) and np.isnan(b))):
                d[f] = (a, b)
        if d:
            bad[j] = d
    print(name, nE, 'T', [r[0] for r in recs])
    assert not bad, bad


def _count_fields():
    from loss import COUNT_FIELDS
    return COUNT_FIELDS


@pytest.mark.parametrize('name', ti.POINTS)
def test_trials_first_iteration_state_agrees(device, name):
    seq = sequential(name, 1)
    recs, dec, xm, var = _trials(name, 1, tuple(range(E)))
    bad = {}
    for j in range(E):
        scale = float(seq[j][3].abs().max())
        for key, got, ref in (('r', dec[j], seq[j][3]), ('xmmse', xm[j], seq[j][4]), ('var', var[j], seq[j][5])):
            err = float((got - ref).abs().max())
            if not err <= 2e-6 * scale:
                bad[(j, key)] = (err, scale)
        if recs[j][0] != 1:
            bad[(j, 'T')] = recs[j][0]
    assert not bad, bad


@pytest.mark.parametrize('name', ti.POINTS)
def test_trials_match_reference_g13(device, name):
    recs = grouped40(name)[0]
    ref = ti.G13[name]['trials']
    diff = {}
    for j in range(E):
        d = {k: (recs[j][2][k], ref[j][k]) for k in gio.COUNT_KEYS if recs[j][2][k] != ref[j][k]}
        if d:
            diff[j] = d
    tdiff = [(j, recs[j][0], int(ref[j]['T'])) for j in range(E) if recs[j][0] != int(ref[j]['T'])]
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert len(diff) <= 1, diff


@pytest.mark.parametrize('kind', ['huge', 'nan'])
@pytest.mark.parametrize('name', ti.POINTS)
def test_trials_isolated_from_a_bad_trial(device, name, kind):
    base_recs, bdec, bxm, bvar = grouped40(name)
    inp = ti.device_inputs(name)
    victim = 5                                     # a row inside the first tile, among live neighbours
    ys = list(inp['y'])
    ys[victim] = ys[victim] * 1e6 if kind == 'huge' else torch.full_like(ys[victim], float('nan'))
    recs, dec, xm, var = _trials(name, None, tuple(range(E)), ys=ys)
    bad = {}
    for j in range(E):
        if j == victim:
            continue
        d = []
        if recs[j][0] != base_recs[j][0]:
            d.append(('T', recs[j][0], base_recs[j][0]))
        if not np.array_equal(recs[j][1], base_recs[j][1], equal_nan=True):
            d.append('counters')
        for key, a, b in (('r', dec[j], bdec[j]), ('xmmse', xm[j], bxm[j]), ('var', var[j], bvar[j])):
            if not gio.bits_equal(a, b):
                d.append(key)
        if d:
            bad[j] = d
    assert not bad, bad
    if kind == 'nan':
        assert bool(torch.isnan(var[victim]).all()) and recs[victim][0] == ti.G13[name]['iterations']


@pytest.mark.parametrize('name', ti.POINTS)
def test_trials_frozen_var_at_odd_and_even_exits(device, name):
    seq = sequential(name, None)
    recs, _, _, var = grouped40(name)
    Ts = [r[0] for r in recs]
    assert any(t % 2 for t in Ts) and any(t % 2 == 0 for t in Ts), Ts      # both ping-pong buffers
    bad = [(j, Ts[j]) for j in range(E) if not gio.bits_equal(var[j], seq[j][5])]
    assert not bad, bad


@pytest.mark.parametrize('name', [p for p in ti.POINTS if 'Nt32' in p])
def test_trials_sparc_rule(device, name):
    """generator_mode='sparc' (the MAP rule, loss.py:282-302) per trial."""
    seq = sequential(name, None, 'sparc')
    recs = _trials(name, None, tuple(range(E)), mode='sparc')[0]
    bad = {j: (recs[j][0], seq[j][0]) for j in range(E)
           if recs[j][0] != seq[j][0] or not np.array_equal(recs[j][1], seq[j][1], equal_nan=True)}
    assert not bad, bad


@pytest.mark.parametrize('det', ['vamp', 'bamp'])
def test_model_simulate_group_trials(device, tmp_path, det):
    from model import Model
    name = f'{det}_QPSK_Nt32'
    out = {}
    for gt in (0, 8):
        cfg = ti.config_of(name, device='cuda')
        m = Model(cfg, det, path=str(tmp_path / f'g{gt}'), seed=5, group_trials=gt)
        out[gt] = m.simulate(epochs=8, start=6, final=7.0, step=1, res=4)
    assert len(out[0]) >= 1
    assert json.dumps(out[0], sort_keys=True) == json.dumps(out[8], sort_keys=True)
    for p in out[0]:
        f = f"{p['EbN0dB']}.json"
        assert open(tmp_path / 'g0' / f).read() == open(tmp_path / 'g8' / f).read()
