"""VAMP trial batches over several channels on the GPU: VAMP.forward_trials(..., per_channel=R)
(amp_vamp_trials_ch_run).  Per point (tests/vamp_trials_channels_inputs.py, which says which point
covers which tile case): 40 channels with their SVD, 40 messages and 40 noise vectors drawn once from
a seed; for a given R, trial e uses channel e // R.

1. grouped equals sequential: E = 40 with R in {1, 5, 32, 33} (one-row tiles; several channels per 32
   rows; a full tile followed by a ragged tile; two tiles per channel, the second holding one row,
   the next channel starting at odd row 33) and E = 1, R = 1: every trial equals the sequential
   launch-engine B = 1 forward with its own (U, s, Vh): T, all counters, nan_state, r / xmmse / var
   BIT-equal; all differing trials and keys in one assertion;
2. iteration 0 alone: the same with iterations = 1 at R = 5 (the per-channel iteration-0 record and y~);
3. one channel given 8 times with R = 5 is bit-equal to the single-channel forward_trials;
4. isolation: with R = 5 and channel 2's U, s, Vh set to NaN the other 35 trials are bit-equal to the
   clean grouped run and the five victims equal their own sequential forwards;
5. rare paths across a channel boundary: the 'huge' construction of
   test_gpu_trials.py::test_trials_isolated_from_a_bad_trial (one trial's y x 1e6) at R = 3, the
   victim's tile neighbours on other channels: the victim and the seven others equal their
   sequential forwards, and the victim's nan_state says the fix-up or the all-NaN rule ran (y x 1e6
   turns every section NaN; y x 100 over two iterations leaves some finite at three points: the
   exact float64 fix-up);
6. against g19 (the reference at res = 5): the grouped run (R = 5) differs from the reference's
   counting metrics on exactly the trials where the sequential forwards differ (set and count printed);
7. every Loss reports arithmetic 'f32';
8. Model(group_trials=8, trial_channels=8) equals the per-epoch loop: result list and exported files.
"""
import functools
import json

import numpy as np
import pytest
import torch

import golden_io as gio
import vamp_trials_channels_inputs as vc

pytestmark = pytest.mark.gpu

E = vc.E


def _detector(name, iterations=None, golden=False):
    import amp_native as nat
    from vamp import VAMP
    return VAMP(vc.config_of(name, device='cuda', iterations=iterations, golden=golden), engine=nat.ENGINE_LAUNCHES)


def _record(L):
    from loss import counts_to_vector
    assert L.arithmetic == 'f32'                                                # 7.
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _forward(det, inp, e, ch, y):
    """One sequential B = 1 forward of trial e with the channel factors ch = (U, s, Vh):
    (T, counters, metrics, nan_state, r, xmmse, var)."""
    rec = _record(det(*ch, y, inp['SNR'], inp['x'][e], inp['sym'][e], inp['idx'][e]))
    b = det.last.buf
    return rec + (b.r.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.var.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def _seq_detector(name, iterations):
    return _detector(name, iterations)


@functools.lru_cache(maxsize=None)
def sequential(name, e, g, iterations=None):
    """Trial e through channel g as a sequential B = 1 forward of the launch engine.  Computed once,
    shared, never modified."""
    inp = vc.device_point(name)
    ch = (inp['U'][g], inp['s'][g], inp['Vh'][g])
    return _forward(_seq_detector(name, iterations), inp, e, ch, vc.received(inp, e, g))


def _grouped(det, inp, ids, chans, ys, R):
    """chans = (Us, ss, Vhs)."""
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(*chans, ys, inp['SNR'], pick(inp['x']), pick(inp['sym']), pick(inp['idx']), per_channel=R)
    recs = [_record(L) for L in Ls]
    r, xm, var = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, r, xm, var


@functools.lru_cache(maxsize=None)
def grouped(name, nE, R, iterations=None):
    """Trials 0 .. nE - 1, trial e through channel e // R, in one call."""
    inp = vc.device_point(name)
    G = -(-nE // R)
    ys = [vc.received(inp, e, e // R) for e in range(nE)]
    return _grouped(_detector(name, iterations), inp, tuple(range(nE)), vc.factors(inp, range(G)), ys, R)


def _count_fields():
    from loss import COUNT_FIELDS
    return COUNT_FIELDS


def _differences(rec, bufs, ref):
    """Keys on which one trial (record, (r, xmmse, var) rows) differs from a sequential forward."""
    d = {}
    if rec[0] != ref[0]:
        d['T'] = (rec[0], ref[0])
    for f, a, b in zip(_count_fields(), rec[1], ref[1]):
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d[f] = (a, b)
    if rec[3] != ref[3]:
        d['nan_state'] = (rec[3], ref[3])
    for key, got, want in zip(('r', 'xmmse', 'var'), bufs, ref[4:7]):
        if not gio.bits_equal(got, want):
            d[key] = 'bits differ'
    return d


@pytest.mark.parametrize('nE,R', [(40, 1), (40, 5), (40, 32), (40, 33), (40, 40), (1, 1)])
@pytest.mark.parametrize('name', vc.POINT_IDS)
def test_vamp_trials_channels_equal_sequential_forwards(device, name, nE, R):
    recs, r, xm, var = grouped(name, nE, R)
    bad = {}
    for e in range(nE):
        d = _differences(recs[e], (r[e], xm[e], var[e]), sequential(name, e, e // R))
        if d:
            bad[e] = d
    print(name, nE, R, 'T', [rec[0] for rec in recs])
    assert not bad, bad


@pytest.mark.parametrize('name', vc.POINT_IDS)
def test_vamp_trials_channels_iteration_0_alone(device, name):
    R = 5
    recs, r, xm, var = grouped(name, E, R, 1)
    bad = {}
    for e in range(E):
        d = _differences(recs[e], (r[e], xm[e], var[e]), sequential(name, e, e // R, 1))
        if d:
            bad[e] = d
    assert not bad, bad


@pytest.mark.parametrize('name', vc.POINT_IDS)
def test_one_channel_given_several_times_equals_the_single_channel_call(device, name):
    inp = vc.device_point(name)
    ch = (inp['U'][0], inp['s'][0], inp['Vh'][0])
    ys = [vc.received(inp, e, 0) for e in range(E)]
    recs, r, xm, var = _grouped(_detector(name), inp, tuple(range(E)), vc.factors(inp, [0] * 8), ys, 5)
    det = _detector(name)
    Ls = det.forward_trials(*ch, ys, inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    ref = [_record(L) for L in Ls]
    rr, rm, rv = (t.reshape(E, -1) for t in det.last_trials)
    bad = {}
    for e in range(E):
        d = _differences(recs[e], (r[e], xm[e], var[e]), ref[e] + (rr[e], rm[e], rv[e]))
        if d:
            bad[e] = d
    assert not bad, bad


@pytest.mark.parametrize('name', vc.POINT_IDS)
def test_trials_isolated_from_a_nan_channel(device, name):
    R, bad_g = 5, 2
    base_recs, br, bxm, bvar = grouped(name, E, R)
    inp = vc.device_point(name)
    Us, ss, Vhs = vc.factors(inp, range(E // R))
    nan = lambda t: torch.full_like(t, float('nan'))   # noqa: E731
    Us[bad_g], ss[bad_g], Vhs[bad_g] = nan(Us[bad_g]), nan(ss[bad_g]), nan(Vhs[bad_g])
    ys = [vc.received(inp, e, e // R) for e in range(E)]                     # the clean run's y
    recs, r, xm, var = _grouped(_detector(name), inp, tuple(range(E)), (Us, ss, Vhs), ys, R)
    victims = range(bad_g * R, (bad_g + 1) * R)
    det = _detector(name)
    bad = {}
    for e in range(E):
        if e in victims:      # its own sequential forward with the NaN channel
            ref = _forward(det, inp, e, (Us[bad_g], ss[bad_g], Vhs[bad_g]), ys[e])
        else:                 # the clean grouped run, bit for bit
            ref = base_recs[e] + (br[e], bxm[e], bvar[e])
        d = _differences(recs[e], (r[e], xm[e], var[e]), ref)
        if d:
            bad[e] = d
    print(name, 'victims T', [recs[e][0] for e in victims], 'nan_state', [recs[e][3] for e in victims])
    assert not bad, bad


# y x 1e6 at every point (the all-NaN rule fires at each); y x 100 over 2 iterations where that leaves
# some sections finite, i.e. the exact float64 fix-up ran and not the all-NaN rule
RARE = [(name, None, 1e6, False) for name in vc.POINT_IDS] + \
       [(name, 2, 100.0, True) for name in ('vamp_QPSK_Nt32', 'trials_OOK_Nt48', 'wide_OOK_Nt256')]


@pytest.mark.parametrize('name,iterations,scale,partial', RARE)
def test_rare_paths_across_a_channel_boundary(device, name, iterations, scale, partial):
    """Trial 5's y scaled: with R = 3 it shares its channel with trials 3 and 4 only; trials 0-2 and
    6-7, its tile neighbours, run on other channels."""
    nE, R, victim = 8, 3, 5
    inp = vc.device_point(name)
    ys = [vc.received(inp, e, e // R) for e in range(nE)]
    ys[victim] = ys[victim] * scale
    recs, r, xm, var = _grouped(_detector(name, iterations), inp, tuple(range(nE)), vc.factors(inp, range(3)), ys, R)
    nan = int(torch.isnan(xm[victim].real).sum())
    print(name, 'victim T', recs[victim][0], 'nan_state', recs[victim][3], 'NaN entries', nan, 'of', xm.shape[1])
    assert recs[victim][3] != 0                                    # the fix-up or the all-NaN rule ran
    if partial:
        assert 0 < nan < xm.shape[1]                               # the fix-up, not the all-NaN rule
    det = _detector(name, iterations)
    bad = {}
    for e in range(nE):
        g = e // R
        d = _differences(recs[e], (r[e], xm[e], var[e]), _forward(det, inp, e, (inp['U'][g], inp['s'][g], inp['Vh'][g]), ys[e]))
        if d:
            bad[e] = d
    assert not bad, bad


@pytest.mark.parametrize('name', vc.GOLDEN_POINTS)
def test_vamp_trials_channels_against_the_reference_g19(device, name):
    h = vc.golden_inputs(name)
    R = h['res']
    inp = dict(h)
    inp['x'] = [t.cuda() for t in h['x']]
    chans = tuple([h[k][g * R].cuda() for g in range(E // R)] for k in ('U', 's', 'Vh'))
    ys = [t.cuda() for t in h['y']]
    recs = _grouped(_detector(name, golden=True), inp, tuple(range(E)), chans, ys, R)[0]
    det = _detector(name, golden=True)
    seq = [_forward(det, inp, e, tuple(c[e // R] for c in chans), ys[e]) for e in range(E)]
    ref = vc.G19[name]['trials']
    differs = lambda rec: {j for j in range(E)   # noqa: E731
                           if any(rec[j][2][k] != ref[j][k] for k in gio.COUNT_KEYS)}
    dg, ds = differs(recs), differs(seq)
    print(name, 'trials whose counting metrics differ from the reference: grouped', sorted(dg), 'sequential',
          sorted(ds), 'count', len(dg))
    assert dg == ds, (sorted(dg), sorted(ds))


@pytest.mark.parametrize('res', [1, 3])
def test_model_simulate_vamp_trial_channels(device, tmp_path, res):
    """Model(group_trials=8, trial_channels=8) with the real detector: the points and the exported
    files of the per-epoch loop (res = 3 over 8 epochs: blocks of 3, 3, 2, so a short last block)."""
    from model import Model
    out = {}
    for key, kw in (('loop', {}), ('grouped', dict(group_trials=8, trial_channels=8))):
        cfg = vc.config_of('vamp_QPSK_Nt32', device='cuda')
        m = Model(cfg, 'vamp', path=str(tmp_path / key), seed=5, **kw)
        out[key] = m.simulate(epochs=8, start=6, final=7.0, step=1, res=res)
    assert len(out['loop']) >= 1
    assert json.dumps(out['loop'], sort_keys=True) == json.dumps(out['grouped'], sort_keys=True)
    for p in out['loop']:
        f = f"{p['EbN0dB']}.json"
        assert open(tmp_path / 'loop' / f).read() == open(tmp_path / 'grouped' / f).read()
