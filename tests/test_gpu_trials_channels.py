"""BAMP / SCAMP trial batches over several channels on the GPU: forward_trials(..., per_channel=R)
(amp_bamp_trials_ch_run / amp_scamp_trials_ch_run).  Per point (tests/trials_channels_inputs.py): 40
channels, 40 messages and 40 noise vectors drawn once from a seed; for a given R, trial e uses
channel e // R.  scamp_OOK_Nt128 reaches the split-psi kernel and the block-banded GEMMs;
trials_OOK_Nt6 has N % 4 == 2 and odd n (ALoadPair from an odd first row).

1. grouped equals sequential: E = 40 with R in {1, 5, 32, 33} (one-row tiles; several channels per 32
   rows; a full tile followed by a ragged tile; two tiles per channel, the second holding one row,
   the next channel starting at odd row 33) and E = 1, R = 1: every trial equals the sequential
   launch-engine B = 1 forward with its own channel: T, all counters, nan_state, xmap / xmmse and
   var (BAMP) / psi (SCAMP) BIT-equal; all differing trials and keys in one assertion;
2. one channel given G times with R = 5 is bit-equal to the single-channel forward_trials;
3. isolation: with R = 5 and channel 2 set to NaN the other 35 trials are bit-equal to the clean
   grouped run and the five victims equal their own sequential forwards;
4. the exact float64 fix-up across a channel boundary: a victim case of test_gpu_scamp_trials.py
   (its scale and iteration count, its g14 channel and inputs) with R = 3, its tile neighbours on
   other channels: the victim and the seven others equal their sequential forwards;
5. against g18 (the reference at res = 5): the grouped run (R = 5) differs from the reference's
   counting metrics on exactly the trials where the sequential forwards differ (count printed);
6. every Loss reports arithmetic 'f32'.
"""
import functools

import numpy as np
import pytest
import torch

import golden_io as gio
import scamp_trials_inputs as si
import trials_channels_inputs as tc

pytestmark = pytest.mark.gpu

E = tc.E


def _detector(name, iterations=None, golden=False):
    import amp_native as nat
    from bamp import BAMP
    from scamp import SCAMP
    cfg = tc.config_of(name, device='cuda', iterations=iterations, golden=golden)
    return SCAMP(cfg, engine=nat.ENGINE_LAUNCHES) if tc.algo_of(name) == 'scamp' else BAMP(cfg)


def _record(L):
    from loss import counts_to_vector
    assert L.arithmetic == 'f32'                                                # 6.
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _head(det, inp):
    return (inp['W'],) if type(det).__name__ == 'SCAMP' else ()


def _forward(det, inp, e, A, y):
    """One sequential B = 1 forward of trial e with channel A:
    (T, counters, metrics, nan_state, xmap, xmmse, var | psi)."""
    L = det(*_head(det, inp), A, y, inp['SNR'], inp['x'][e], inp['sym'][e], inp['idx'][e])
    rec = _record(L)
    b = det.last.buf
    state = b.psi if type(det).__name__ == 'SCAMP' else b.var
    return rec + (b.xmap.clone().reshape(-1), b.xmmse.clone().reshape(-1), state.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def _seq_detector(name):
    return _detector(name)


@functools.lru_cache(maxsize=None)
def sequential(name, e, g):
    """Trial e through channel g as a sequential B = 1 forward of the launch engine.  Computed once,
    shared, never modified."""
    inp = tc.device_point(name)
    return _forward(_seq_detector(name), inp, e, inp['A'][g], tc.received(inp, e, g))


def _grouped(det, inp, ids, chans, ys, R):
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(*_head(det, inp), chans, ys, inp['SNR'], pick(inp['x']), pick(inp['sym']),
                            pick(inp['idx']), per_channel=R)
    recs = [_record(L) for L in Ls]
    xmap, xm, state = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, xmap, xm, state


@functools.lru_cache(maxsize=None)
def grouped(name, nE, R):
    """Trials 0 .. nE - 1, trial e through channel e // R, in one call."""
    inp = tc.device_point(name)
    G = -(-nE // R)
    ys = [tc.received(inp, e, e // R) for e in range(nE)]
    return _grouped(_detector(name), inp, tuple(range(nE)), inp['A'][:G], ys, R)


def _count_fields():
    from loss import COUNT_FIELDS
    return COUNT_FIELDS


def _differences(rec, bufs, ref, state='state'):
    """Keys on which one trial (record, (xmap, xmmse, var | psi) rows) differs from a sequential forward."""
    d = {}
    if rec[0] != ref[0]:
        d['T'] = (rec[0], ref[0])
    for f, a, b in zip(_count_fields(), rec[1], ref[1]):
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d[f] = (a, b)
    if rec[3] != ref[3]:
        d['nan_state'] = (rec[3], ref[3])
    for key, got, want in zip(('xmap', 'xmmse', state), bufs, ref[4:7]):
        if not gio.bits_equal(got, want):
            d[key] = 'bits differ'
    return d


def _state(name):
    return 'psi' if tc.algo_of(name) == 'scamp' else 'var'


@pytest.mark.parametrize('nE,R', [(40, 1), (40, 5), (40, 32), (40, 33), (40, 40), (1, 1)])
@pytest.mark.parametrize('name', tc.POINT_IDS)
def test_trials_channels_equal_sequential_forwards(device, name, nE, R):
    recs, xmap, xm, st = grouped(name, nE, R)
    bad = {}
    for e in range(nE):
        d = _differences(recs[e], (xmap[e], xm[e], st[e]), sequential(name, e, e // R), _state(name))
        if d:
            bad[e] = d
    print(name, nE, R, 'T', [r[0] for r in recs])
    assert not bad, bad


@pytest.mark.parametrize('name', tc.POINT_IDS)
def test_one_channel_given_several_times_equals_the_single_channel_call(device, name):
    inp = tc.device_point(name)
    A = inp['A'][0]
    ys = [tc.received(inp, e, 0) for e in range(E)]
    ids = tuple(range(E))
    recs, xmap, xm, st = _grouped(_detector(name), inp, ids, [A] * 8, ys, 5)
    det = _detector(name)
    Ls = det.forward_trials(*_head(det, inp), A, ys, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    ref = [_record(L) for L in Ls]
    rx, rm, rs = (t.reshape(E, -1) for t in det.last_trials)
    bad = {}
    for e in range(E):
        d = _differences(recs[e], (xmap[e], xm[e], st[e]), ref[e] + (rx[e], rm[e], rs[e]), _state(name))
        if d:
            bad[e] = d
    assert not bad, bad


@pytest.mark.parametrize('name', tc.POINT_IDS)
def test_trials_isolated_from_a_nan_channel(device, name):
    R, bad_g = 5, 2
    base_recs, bxmap, bxm, bst = grouped(name, E, R)
    inp = tc.device_point(name)
    chans = list(inp['A'][:E // R])
    chans[bad_g] = torch.full_like(chans[bad_g], float('nan'))
    ys = [tc.received(inp, e, e // R) for e in range(E)]                     # the clean run's y
    recs, xmap, xm, st = _grouped(_detector(name), inp, tuple(range(E)), chans, ys, R)
    victims = range(bad_g * R, (bad_g + 1) * R)
    det = _detector(name)
    bad = {}
    for e in range(E):
        if e in victims:      # its own sequential forward with the NaN channel
            ref = _forward(det, inp, e, chans[bad_g], ys[e])
        else:                 # the clean grouped run, bit for bit
            ref = base_recs[e] + (bxmap[e], bxm[e], bst[e])
        d = _differences(recs[e], (xmap[e], xm[e], st[e]), ref, _state(name))
        if d:
            bad[e] = d
    print(name, 'victims T', [recs[e][0] for e in victims], 'nan_state', [recs[e][3] for e in victims])
    assert not bad, bad


def test_scamp_exact_fixup_across_a_channel_boundary(device):
    """('scamp_OOK_Nt16', 2 iterations, y x 30) of test_gpu_scamp_trials.py: the victim (trial 5) keeps
    its g14 channel and inputs, with R = 3 it shares that channel with trials 3 and 4 only; trials
    0-2 and 6-7, its tile neighbours, run on other channels."""
    name, iterations, scale, nE, R, victim = 'scamp_OOK_Nt16', 2, 30.0, 8, 3, 5
    g14 = si.device_inputs(name)
    other = tc.device_point(name)
    chans = [other['A'][0], g14['A'], other['A'][1]]
    inp = dict(g14)
    ys = [g14['y'][e] if e // R == 1 else chans[e // R] @ g14['x'][e] + other['noise'][e] for e in range(nE)]
    ys[victim] = ys[victim] * scale
    recs, xmap, xm, psi = _grouped(_detector(name, iterations), inp, tuple(range(nE)), chans, ys, R)
    nan = int(torch.isnan(xm[victim].real).sum())
    print(name, 'victim T', recs[victim][0], 'nan_state', recs[victim][3], 'NaN entries', nan, 'of', xm.shape[1])
    assert recs[victim][3] == 1 and 0 < nan < xm.shape[1]          # the fix-up ran, not the all-NaN rule
    det = _detector(name, iterations)
    bad = {}
    for e in range(nE):
        d = _differences(recs[e], (xmap[e], xm[e], psi[e]), _forward(det, inp, e, chans[e // R], ys[e]), 'psi')
        if d:
            bad[e] = d
    assert not bad, bad


@pytest.mark.parametrize('name', tc.GOLDEN_POINTS)
def test_trials_channels_against_the_reference_g18(device, name):
    h = tc.golden_inputs(name)
    R = h['res']
    inp = dict(h)
    inp['W'] = h['W'].cuda()
    inp['x'] = [t.cuda() for t in h['x']]
    As = [h['A'][g * R].cuda() for g in range(E // R)]
    ys = [t.cuda() for t in h['y']]
    recs = _grouped(_detector(name, golden=True), inp, tuple(range(E)), As, ys, R)[0]
    det = _detector(name, golden=True)
    seq = [_forward(det, inp, e, As[e // R], ys[e]) for e in range(E)]
    ref = tc.G18[name]['trials']
    differs = lambda rec: {j for j in range(E)   # noqa: E731
                           if any(rec[j][2][k] != ref[j][k] for k in gio.COUNT_KEYS)}
    dg, ds = differs(recs), differs(seq)
    print(name, 'trials whose counting metrics differ from the reference: grouped', sorted(dg), 'sequential',
          sorted(ds), 'count', len(dg))
    assert dg == ds, (sorted(dg), sorted(ds))


@pytest.mark.parametrize('res', [1, 3])
@pytest.mark.parametrize('det', ['bamp', 'scamp'])
def test_model_simulate_trial_channels(device, tmp_path, det, res):
    """Model(group_trials=8, trial_channels=8) with the real detectors: the points and the exported
    files of the per-epoch loop (res = 3 over 8 epochs: blocks of 3, 3, 2, so a short last block)."""
    import json
    from model import Model
    name = f'{det}_QPSK_Nt32'
    out = {}
    for key, kw in (('loop', {}), ('grouped', dict(group_trials=8, trial_channels=8))):
        cfg = tc.config_of(name, device='cuda')
        m = Model(cfg, det, path=str(tmp_path / key), seed=5, **kw)
        out[key] = m.simulate(epochs=8, start=6, final=7.0, step=1, res=res)
    assert len(out['loop']) >= 1
    assert json.dumps(out['loop'], sort_keys=True) == json.dumps(out['grouped'], sort_keys=True)
    for p in out['loop']:
        f = f"{p['EbN0dB']}.json"
        assert open(tmp_path / 'loop' / f).read() == open(tmp_path / 'grouped' / f).read()
