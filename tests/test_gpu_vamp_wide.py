"""VAMP at odd n, odd k and a partial last column tile on the GPU (launch engines, f32 tiles): the
g17 points (tests/golden/make_g17_vamp_wide.py).  w, the A operand of GEMM2, has a padded row stride
there (vamp_wld), y is staged through the pair loader where n is odd, and the column tiles end in a
partial one at N = 96 (128 + 64 columns) and 2N = 1008.  Every test here raised AMP_E_ARG before
these shapes were taken.

1. sequential B = 1 forwards against g17 (the reference at batch = 1): every counting metric; at
   most 1 of 40 trials per point and 2 over all points may differ (the CPU oracle differs on none:
   test_vamp_wide_cpu.py; the cap leaves room for f32 summation order at B = 1, as g16's does).  T is
   printed, not asserted.  nan_state is 0 everywhere and the arithmetic is f32.
2. VAMP.forward_trials (E = 40, 33, 1) against those sequential forwards: T_e, every counter and
   nan_state equal, r / xmmse / var BIT-equal; exits at odd and at even T_e (QPSK Nt = 12 has both).
3. isolation: trial 5's y scaled by 1e6, or set to NaN, leaves every other trial bit-equal, and the
   victim equal to its own sequential forward.
4. B = 48 (a full 32-row tile and a partial one) against the reference: VER and SER within 1e-3 (the
   project's parity bar), T equal to g17's, and two further forwards on the same inputs return the
   same bits.
5. ShardedVAMP over two slices of 24 trials in one process (two threads whose all-reduce hook meets
   on a barrier) against the whole-batch forward: T and every counter, at an odd-k point and at the
   partial-tile point.
6. the layer-level path (amp_vamp_prepare / amp_vamp_iterate x T / amp_vamp_finalize) against
   amp_vamp_run, bit for bit, at an odd-k point.
7. pad hygiene at an odd-k point: a forward on a workspace filled with NaN bytes equals the forward
   on a zero-filled one bit for bit (an unzeroed pad of w, or a read past a partial tile, would not).
8. the published shape (Nt=1344 Na=84 Nr=73 Lh=6 Lin=32: N = 43008, n = k = 2701) once:
   forward_trials of four trials against four sequential forwards.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import golden_io as gio
import vamp_wide_inputs as wi

pytestmark = pytest.mark.gpu

E = wi.E_G17
VICTIM = 5                                     # a row inside the first tile, among live neighbours


def _detector(name):
    from vamp import VAMP
    return VAMP(wi.config_of(name, device='cuda'))


def _record(L):
    from loss import counts_to_vector
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _forward(det, inp, j, y):
    """One sequential B = 1 forward: (T, counters, metrics, nan_state, r, xmmse, var)."""
    L = det(inp['U'], inp['s'], inp['Vh'], y, inp['SNR'], inp['x'][j], inp['sym'][j], inp['idx'][j])
    rec = _record(L)
    assert L.arithmetic == 'f32'
    b = det.last.buf
    return rec + (b.r.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.var.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def sequential(name):
    """The 40 trials as sequential B = 1 forwards.  Computed once, shared, never modified."""
    det = _detector(name)
    inp = wi.device_inputs(name)
    return [_forward(det, inp, j, inp['y'][j]) for j in range(E)]


def _trials(det, inp, ids, ys=None):
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(inp['U'], inp['s'], inp['Vh'], ys if ys is not None else pick(inp['y']), inp['SNR'],
                            pick(inp['x']), pick(inp['sym']), pick(inp['idx']))
    recs = [_record(L) for L in Ls]
    assert all(L.arithmetic == 'f32' for L in Ls)
    r, xm, var = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, r, xm, var


@functools.lru_cache(maxsize=None)
def grouped40(name):
    return _trials(_detector(name), wi.device_inputs(name), tuple(range(E)))


def _differences(rec, bufs, ref):
    """Keys on which one trial (record, (r, xmmse, var) rows) differs from a sequential forward."""
    from loss import COUNT_FIELDS
    d = {}
    if rec[0] != ref[0]:
        d['T'] = (rec[0], ref[0])
    for f, a, b in zip(COUNT_FIELDS, rec[1], ref[1]):
        if not (a == b or (np.isnan(a) and np.isnan(b))):
            d[f] = (a, b)
    if rec[3] != ref[3]:
        d['nan_state'] = (rec[3], ref[3])
    if bufs is not None:
        for key, got, want in zip(('r', 'xmmse', 'var'), bufs, ref[4:7]):
            if not gio.bits_equal(got, want):
                d[key] = 'bits differ'
    return d


def _reference_differences(name):
    """Trials of a point whose counting metrics differ from the reference's: {trial: {key: (got, ref)}}."""
    seq = sequential(name)
    ref = wi.G17[name]['trials']
    diff = {}
    for j in range(E):
        d = {k: (seq[j][2][k], ref[j][k]) for k in gio.COUNT_KEYS if seq[j][2][k] != ref[j][k]}
        if d:
            diff[j] = d
    return diff


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_sequential_forwards_match_reference_g17(device, name):
    seq = sequential(name)
    ref = wi.G17[name]['trials']
    diff = _reference_differences(name)
    tdiff = [(j, seq[j][0], int(ref[j]['T'])) for j in range(E) if seq[j][0] != int(ref[j]['T'])]
    print(name, 'trials whose T differs from the reference:', len(tdiff), '(the CPU oracle:',
          wi.G17[name]['oracle_T_differs'], ')', tdiff)
    print(name, 'trials whose counting metrics differ from the reference:', diff)
    assert all(r[3] == 0 for r in seq), [r[3] for r in seq]
    assert len(diff) <= 1, diff


def test_sequential_forwards_match_reference_over_all_points(device):
    diff = {name: _reference_differences(name) for name in wi.TRIAL_POINTS}
    diff = {name: d for name, d in diff.items() if d}
    print('trials whose counting metrics differ from the reference, all points:', diff)
    assert sum(len(d) for d in diff.values()) <= 2, diff


@pytest.mark.parametrize('nE', [40, 33, 1])
@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_wide_trials_equal_sequential_forwards(device, name, nE):
    seq = sequential(name)
    recs, r, xm, var = (grouped40(name) if nE == 40 else
                        _trials(_detector(name), wi.device_inputs(name), tuple(range(nE))))
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (r[j], xm[j], var[j]), seq[j])
        if d:
            bad[j] = d
    print(name, nE, 'T', [rec[0] for rec in recs])
    assert not bad, bad


def test_wide_trials_exit_at_odd_and_even_T(device):
    """var is frozen in either ping-pong buffer (the caller's, or the workspace's copied out)."""
    name = 'trials_QPSK_Nt12'
    early = [rec[0] for rec in grouped40(name)[0] if rec[0] < wi.G17[name]['iterations']]
    print('early exits', early)
    assert {t % 2 for t in early} == {0, 1}, early


@pytest.mark.parametrize('kind', ['huge', 'nan'])
@pytest.mark.parametrize('name', ['trials_OOK_Nt6', 'trials_QPSK_Nt12', 'trials_OOK_Nt1344'])
def test_wide_trials_isolated_from_a_bad_trial(device, name, kind):
    base_recs, br, bxm, bvar = grouped40(name)
    inp = wi.device_inputs(name)
    ys = list(inp['y'])
    ys[VICTIM] = ys[VICTIM] * 1e6 if kind == 'huge' else torch.full_like(ys[VICTIM], float('nan'))
    recs, r, xm, var = _trials(_detector(name), inp, tuple(range(E)), ys=ys)
    bad = {}
    for j in range(E):
        if j == VICTIM:
            continue
        d = []
        if recs[j][0] != base_recs[j][0]:
            d.append(('T', recs[j][0], base_recs[j][0]))
        if not np.array_equal(recs[j][1], base_recs[j][1], equal_nan=True):
            d.append('counters')
        for key, a, b in (('r', r[j], br[j]), ('xmmse', xm[j], bxm[j]), ('var', var[j], bvar[j])):
            if not gio.bits_equal(a, b):
                d.append(key)
        if d:
            bad[j] = d
    assert not bad, bad
    # the victim is its own sequential forward on the same modified y (its float64 fix-up included)
    own = _forward(_detector(name), inp, VICTIM, ys[VICTIM])
    d = _differences(recs[VICTIM], (r[VICTIM], xm[VICTIM], var[VICTIM]), own)
    print(name, kind, 'victim T', recs[VICTIM][0], 'nan_state', recs[VICTIM][3])
    assert not d, d


def _batch_forward(det, inp):
    L = det(inp['U'], inp['s'], inp['Vh'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    rec = _record(L)
    assert L.arithmetic == 'f32'
    b = det.last.buf
    return rec, (b.r.clone(), b.xmmse.clone(), b.var.clone())


@functools.lru_cache(maxsize=None)
def whole_batch(name):
    """The B = 48 forward: (record, (r, xmmse, var)).  Shared, never modified."""
    return _batch_forward(_detector(name), wi.device_inputs(name))


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_wide_batch_point(device, name):
    ref = wi.G17[name]['loss']
    rec, bufs = whole_batch(name)
    for k in ('ver', 'ser'):
        print(name, k, rec[2][k], ref[k])
    for k in ('ver', 'ser'):                       # the project's parity bar
        assert abs(rec[2][k] - ref[k]) <= 1e-3, (k, rec[2][k], ref[k])
    assert rec[0] == int(ref['T']), (rec[0], ref['T'])
    assert rec[3] == 0
    det = _detector(name)
    for _ in range(2):
        rec2, bufs2 = _batch_forward(det, wi.device_inputs(name))
        assert rec2[0] == rec[0] and np.array_equal(rec2[1], rec[1], equal_nan=True)
        for key, a, b in zip(('r', 'xmmse', 'var'), bufs2, bufs):
            assert gio.bits_equal(a, b), key


@pytest.mark.parametrize('name', ['batch_OOK_Nt16', 'batch_8PSK_Nt168'])
def test_wide_sharded_slices_equal_whole_batch(device, monkeypatch, name):
    """batch_OOK_Nt16: k = 35 (w's rows padded); batch_8PSK_Nt168: k = 292, 2N = 1008 (partial last tile)."""
    import shard_threads
    from loss import counts_to_vector
    whole, _ = whole_batch(name)
    out = shard_threads.run_slices(monkeypatch, lambda: wi.config_of(name, device='cuda'), wi.device_inputs(name),
                                   lambda det, L: (int(L.last_status.T), counts_to_vector(L.last_counts)))
    assert out[0][0] == out[1][0] == whole[0], (out[0][0], out[1][0], whole[0])
    both = out[0][1] + out[1][1]
    # the nine integer counters exactly; the four float64 error sums up to their summation order
    assert np.array_equal(both[:9], whole[1][:9]), (out[0][1], out[1][1], whole[1])
    assert np.allclose(both[9:], whole[1][9:], rtol=1e-12, atol=0.0), (both[9:], whole[1][9:])


def _tracker(name, inp, j=0):
    from vamp import Tracker
    cfg = wi.config_of(name, device='cuda')
    return Tracker(inp['U'], inp['s'], inp['Vh'], inp['y'][j], None, (cfg.Na / cfg.Nr) / inp['SNR'], cfg.Na / cfg.Nt,
                   cfg)


def _state(T):
    torch.cuda.synchronize()
    s = T.status()
    return (int(s.T), int(s.nan_state), int(s.stopped)), (T.buf.r.clone(), T.buf.xmmse.clone(), T.buf.var.clone())


@pytest.mark.parametrize('name', ['trials_OOK_Nt16', 'trials_QPSK_Nt12'])
def test_layer_level_path_equals_run(device, name):
    """prepare / iterate x T / finalize (Tracker + VAMPLayer) against amp_vamp_run, k = 35 and 15."""
    import amp_native as nat
    from vamp import VAMPLayer
    inp = wi.device_inputs(name)
    cfg = wi.config_of(name, device='cuda')
    with torch.cuda.device(inp['y'][0].device):
        Ta = _tracker(name, inp)
        Ta.args.engine, Ta.args.gemm = nat.ENGINE_LAUNCHES, nat.GEMM_AUTO
        nat.check(nat.lib().amp_vamp_run(C.byref(Ta.dims), C.byref(Ta.const), C.byref(Ta.args), Ta.stream),
                  'amp_vamp_run')
        sa, ba = _state(Ta)
        Tb = _tracker(name, inp)
        Tb.prepare()
        for i in range(cfg.N_Layers):
            VAMPLayer(cfg, i)(Tb)
        Tb.finalize()
        sb, bb = _state(Tb)
    print(name, 'run', sa, 'layers', sb)
    assert sa == sb and sa[1] == 0
    for key, a, b in zip(('r', 'xmmse', 'var'), ba, bb):
        assert gio.bits_equal(a, b), key


@pytest.mark.parametrize('name', ['trials_OOK_Nt16', 'batch_8PSK_Nt168'])
def test_workspace_contents_do_not_reach_the_result(device, name):
    """NaN bytes against zero bytes in the whole workspace before the forward: k = 35 at B = 1 (two
    pad floats per row of w) and k = 292, 2N = 1008 at B = 48 (a partial last column tile)."""
    inp = wi.device_inputs(name)
    det = _detector(name)
    trial = wi.G17[name]['kind'] == 'trials'

    def run():
        if trial:
            return _forward(det, inp, 0, inp['y'][0])
        rec, bufs = _batch_forward(det, inp)
        return rec + bufs

    run()                                          # sizes det's buffers
    ws = det.last.buf.ws
    out = []
    for byte in (0xFF, 0x00):
        torch.cuda.synchronize()
        ws.fill_(byte)
        det._ops.clear()                           # (no operator reuse on the launch engine: stated, not assumed)
        out.append(run())
        assert det.last.buf.ws.data_ptr() == ws.data_ptr()
    a, b = out
    assert a[0] == b[0] and a[3] == b[3] == 0 and np.array_equal(a[1], b[1], equal_nan=True), (a[:4], b[:4])
    for key, x, y in zip(('r', 'xmmse', 'var'), a[4:7], b[4:7]):
        assert gio.bits_equal(x, y), key
        assert bool(torch.isfinite(torch.view_as_real(x) if x.is_complex() else x).all()), key


def test_published_shape_trials_equal_sequential_forwards(device):
    """Nt=1344 Na=84 Nr=73 Lh=6 Lin=32, OOK, segmented (vamp_model.py), 20 iterations: N = 43008,
    n = k = 2701 (odd: w's padded stride, the pair loader on y), 672 column tiles per trial in GEMM2
    and 43 in GEMM1.  U, s, Vh from model.svd_gram on the device: both sides get the same factors."""
    from channel import Channel
    from data import Data
    from model import svd_gram
    from vamp import VAMP
    nE = 4
    cfg = wi.published_config(iterations=20)
    np.random.seed(3)
    torch.manual_seed(3)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    assert tuple(A.shape[-2:]) == (2701, 43008)
    SNR = cfg.snr(8.0)
    Ad = A.to(device).reshape(2701, 43008)
    U, s, Vh = svd_gram(Ad)
    assert tuple(U.shape) == (2701, 2701) and tuple(Vh.shape) == (2701, 43008)
    inp = dict(U=U, s=s, Vh=Vh, SNR=SNR, x=[], sym=[], idx=[], y=[])
    for _ in range(nE):
        x, sym, idx = da.generate_message()
        inp['x'].append(x.to(device)); inp['sym'].append(sym); inp['idx'].append(idx)
        inp['y'].append((A @ x + ch.awgn(SNR)).to(device))
    del Ad
    det = VAMP(wi.published_config(device='cuda', iterations=20))
    seq = [_forward(det, inp, j, inp['y'][j]) for j in range(nE)]
    recs, r, xm, var = _trials(det, inp, tuple(range(nE)))
    print('published shape: T', [rec[0] for rec in recs], 'fer', [rec[2]['fer'] for rec in recs])
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (r[j], xm[j], var[j]), seq[j])
        if d:
            bad[j] = d
    assert not bad, bad
    assert all(rec[3] == 0 for rec in recs)
