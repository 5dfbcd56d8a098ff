"""BAMP at odd n, N % 4 == 2 and a partial last column tile on the GPU (launch engine, f32 tiles):
the g16 points (tests/golden/make_g16_bamp_wide.py).  invu and s, the A operands of two of the four
GEMMs, have padded row strides there (bamp_ild / bamp_sld), var is staged through the pair loader
at N = 18, and the column tiles end in a partial one at N = 96 (128 + 64 columns) and 2N = 1008.
Every test here raised AMP_E_ARG before these shapes were taken.

1. sequential B = 1 forwards against g16 (the reference at batch = 1): every counting metric; at
   most 1 of 40 trials per point and 2 over all points may differ (the CPU oracle differs on none:
   test_bamp_wide_cpu.py; the cap leaves room for the reference's own rounding sensitivity at
   B = 1).  T is printed, not asserted.  nan_state is 0 everywhere.
2. BAMP.forward_trials (E = 40, 33, 1) against those sequential forwards: T_e, every counter and
   nan_state equal, xmap / xmmse / var BIT-equal; exits at odd and at even T_e among the points.
3. isolation: trial 5's y scaled by 1e6, or set to NaN, leaves every other trial bit-equal, and the
   victim equal to its own sequential forward.
4. B = 48 (a full 32-row tile and a partial one) against the reference: VER and SER within 1e-3 (the
   project's parity bar; VER has a granularity of 1/96 there), T = 20, and two further forwards on
   the same inputs return the same bits.
5. ShardedBAMP over two slices of 24 trials in one process (two threads whose all-reduce hook meets
   on a barrier) against the whole-batch forward: T and every counter.
6. 'random' mode (the element-wise denoiser) at n = 7 against the numpy oracle.
7. the published shape (Nt=1344 Na=84 Nr=73 Lh=6 Lin=32: N = 43008, n = 2701) once: forward_trials
   of four trials against four sequential forwards.
"""
import functools
import threading

import numpy as np
import pytest
import torch

import bamp_wide_inputs as wi
import golden_io as gio

pytestmark = pytest.mark.gpu

E = wi.E_G16
VICTIM = 5                                     # a row inside the first tile, among live neighbours


def _detector(name):
    from bamp import BAMP
    return BAMP(wi.config_of(name, device='cuda'))


def _record(L):
    from loss import counts_to_vector
    return (int(L.loss['T']), counts_to_vector(L.last_counts), {k: float(np.asarray(L.loss[k])) for k in gio.LOSS_KEYS},
            int(L.last_status.nan_state))


def _forward(det, inp, j, y):
    """One sequential B = 1 forward: (T, counters, metrics, nan_state, xmap, xmmse, var)."""
    L = det(inp['A'], y, inp['SNR'], inp['x'][j], inp['sym'][j], inp['idx'][j])
    rec = _record(L)
    assert L.arithmetic == 'f32'
    b = det.last.buf
    return rec + (b.xmap.clone().reshape(-1), b.xmmse.clone().reshape(-1), b.var.clone().reshape(-1))


@functools.lru_cache(maxsize=None)
def sequential(name):
    """The 40 trials as sequential B = 1 forwards.  Computed once, shared, never modified."""
    det = _detector(name)
    inp = wi.device_inputs(name)
    return [_forward(det, inp, j, inp['y'][j]) for j in range(E)]


def _trials(det, inp, ids, ys=None):
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(inp['A'], ys if ys is not None else pick(inp['y']), inp['SNR'], pick(inp['x']),
                            pick(inp['sym']), pick(inp['idx']))
    recs = [_record(L) for L in Ls]
    assert all(L.arithmetic == 'f32' for L in Ls)
    xmap, xm, var = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, xmap, xm, var


@functools.lru_cache(maxsize=None)
def grouped40(name):
    return _trials(_detector(name), wi.device_inputs(name), tuple(range(E)))


def _differences(rec, bufs, ref):
    """Keys on which one trial (record, (xmap, xmmse, var) rows) differs from a sequential forward."""
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
        for key, got, want in zip(('xmap', 'xmmse', 'var'), bufs, ref[4:7]):
            if not gio.bits_equal(got, want):
                d[key] = 'bits differ'
    return d


def _reference_differences(name):
    """Trials of a point whose counting metrics differ from the reference's: {trial: {key: (got, ref)}}."""
    seq = sequential(name)
    ref = wi.G16[name]['trials']
    diff = {}
    for j in range(E):
        d = {k: (seq[j][2][k], ref[j][k]) for k in gio.COUNT_KEYS if seq[j][2][k] != ref[j][k]}
        if d:
            diff[j] = d
    return diff


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_sequential_forwards_match_reference_g16(device, name):
    seq = sequential(name)
    ref = wi.G16[name]['trials']
    diff = _reference_differences(name)
    tdiff = [(j, seq[j][0], int(ref[j]['T'])) for j in range(E) if seq[j][0] != int(ref[j]['T'])]
    print(name, 'trials whose T differs from the reference:', len(tdiff), '(the CPU oracle:',
          wi.G16[name]['oracle_T_differs'], ')', tdiff)
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
    recs, xmap, xm, var = (grouped40(name) if nE == 40 else
                           _trials(_detector(name), wi.device_inputs(name), tuple(range(nE))))
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (xmap[j], xm[j], var[j]), seq[j])
        if d:
            bad[j] = d
    print(name, nE, 'T', [r[0] for r in recs])
    assert not bad, bad


def test_wide_trials_exit_at_odd_and_even_T(device):
    """var is frozen in either ping-pong buffer (the caller's, or the workspace's copied out)."""
    early = {name: [r[0] for r in grouped40(name)[0] if r[0] < wi.G16[name]['iterations']] for name in wi.TRIAL_POINTS}
    print('early exits', early)
    assert {t % 2 for ts in early.values() for t in ts} == {0, 1}, early


@pytest.mark.parametrize('kind', ['huge', 'nan'])
@pytest.mark.parametrize('name', ['trials_OOK_Nt6', 'trials_OOK_Nt1344'])
def test_wide_trials_isolated_from_a_bad_trial(device, name, kind):
    base_recs, bxmap, bxm, bvar = grouped40(name)
    inp = wi.device_inputs(name)
    ys = list(inp['y'])
    ys[VICTIM] = ys[VICTIM] * 1e6 if kind == 'huge' else torch.full_like(ys[VICTIM], float('nan'))
    recs, xmap, xm, var = _trials(_detector(name), inp, tuple(range(E)), ys=ys)
    bad = {}
    for j in range(E):
        if j == VICTIM:
            continue
        d = []
        if recs[j][0] != base_recs[j][0]:
            d.append(('T', recs[j][0], base_recs[j][0]))
        if not np.array_equal(recs[j][1], base_recs[j][1], equal_nan=True):
            d.append('counters')
        for key, a, b in (('xmap', xmap[j], bxmap[j]), ('xmmse', xm[j], bxm[j]), ('var', var[j], bvar[j])):
            if not gio.bits_equal(a, b):
                d.append(key)
        if d:
            bad[j] = d
    assert not bad, bad
    # the victim is its own sequential forward on the same modified y (its float64 fix-up included)
    own = _forward(_detector(name), inp, VICTIM, ys[VICTIM])
    d = _differences(recs[VICTIM], (xmap[VICTIM], xm[VICTIM], var[VICTIM]), own)
    print(name, kind, 'victim T', recs[VICTIM][0], 'nan_state', recs[VICTIM][3])
    assert not d, d


def _batch_forward(det, inp):
    L = det(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    rec = _record(L)
    b = det.last.buf
    return rec, (b.xmap.clone(), b.xmmse.clone(), b.var.clone())


@functools.lru_cache(maxsize=None)
def whole_batch(name):
    """The B = 48 forward: (record, (xmap, xmmse, var)).  Shared, never modified."""
    return _batch_forward(_detector(name), wi.device_inputs(name))


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_wide_batch_point(device, name):
    ref = wi.G16[name]['loss']
    rec, bufs = whole_batch(name)
    for k in ('ver', 'ser'):
        print(name, k, rec[2][k], ref[k])
    for k in ('ver', 'ser'):                       # the project's parity bar
        assert abs(rec[2][k] - ref[k]) <= 1e-3, (k, rec[2][k], ref[k])
    assert rec[0] == 20 == int(ref['T']), rec[0]
    assert rec[3] == 0
    det = _detector(name)
    for _ in range(2):
        rec2, bufs2 = _batch_forward(det, wi.device_inputs(name))
        assert rec2[0] == rec[0] and np.array_equal(rec2[1], rec[1], equal_nan=True)
        for key, a, b in zip(('xmap', 'xmmse', 'var'), bufs2, bufs):
            assert gio.bits_equal(a, b), key


class _Exchange:
    """The all-reduce of two slices detected by two threads of one process: each thread's hook puts
    its float64 words on the host, the threads meet, each takes the reduction of both."""

    def __init__(self, world):
        self.local = threading.local()
        self.barrier = threading.Barrier(world, timeout=60)
        self.slots = [None] * world

    def allreduce(self, buf, count, op):
        import amp_native as nat
        ws = self.local.det._ws
        off = int(buf) - ws.data_ptr()
        assert 0 <= off and off + 8 * count <= ws.numel()
        view = ws[off:off + 8 * count].view(torch.float64)
        self.slots[self.local.rank] = view.cpu()           # after the slice's launches on its stream
        self.barrier.wait()
        both = torch.stack(self.slots)
        tot = both.sum(0) if op == nat.ALLREDUCE_SUM else torch.where(torch.isnan(both).any(0), both.sum(0),
                                                                      both.max(0).values)
        self.barrier.wait()                                # both have read the slots
        view.copy_(tot)


@pytest.mark.parametrize('name', ['batch_OOK_Nt48', 'batch_OOK_Nt1344'])
def test_wide_sharded_slices_equal_whole_batch(device, monkeypatch, name):
    import amp_native as nat
    from bamp import ShardedBAMP
    from loss import counts_to_vector
    whole, _ = whole_batch(name)
    inp = wi.device_inputs(name)
    xch = _Exchange(2)
    workspace_type = type(nat.WORKSPACE)

    class PerThreadWorkspace:                              # one workspace cache per slice
        def get(self, dev, key, nbytes):
            if not hasattr(xch.local, 'ws'):
                xch.local.ws = workspace_type()
            return xch.local.ws.get(dev, key, nbytes)

    monkeypatch.setattr(nat, 'WORKSPACE', PerThreadWorkspace())

    class Slice(ShardedBAMP):
        bounds = (0, 0)

        def shard(self):
            return self.bounds

        def _allreduce(self, buf, count, op, stream, ctx):
            try:
                xch.allreduce(buf, count, op)
                return 0
            except Exception as e:   # noqa: BLE001 — reported by _run_hooked
                self._hook_error = self._hook_error or e
                return 1

    out, errs = [None, None], []

    def run(rank):
        try:
            with torch.cuda.device(inp['y'].device):
                det = Slice(wi.config_of(name, device='cuda'))
                det.bounds = (24 * rank, 24 * rank + 24)
                xch.local.rank, xch.local.det = rank, det
                L = det(inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
                out[rank] = (int(L.last_status.T), counts_to_vector(L.last_counts))
        except Exception as e:   # noqa: BLE001
            errs.append((rank, repr(e)))
            xch.barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errs, errs
    assert out[0][0] == out[1][0] == whole[0], (out[0][0], out[1][0], whole[0])
    both = out[0][1] + out[1][1]
    # the nine integer counters exactly; the four float64 error sums up to their summation order
    assert np.array_equal(both[:9], whole[1][:9]), (out[0][1], out[1][1], whole[1])
    assert np.allclose(both[9:], whole[1][9:], rtol=1e-12, atol=0.0), (both[9:], whole[1][9:])


# The larger of max |xmap - oracle| = 2.70e-7 and max |xmmse - oracle| = 2.09e-7 after three iterations
# of 'random' mode at (16, 2, 8, 1, 1), seed 0, QPSK, 8 dB, measured on an MI355X with the build that
# still required n % 4 == 0 (this build returns the same bits at that shape)
RANDOM_PARENT_ERR = 2.6997435043085716e-07


def random_mode_errors(Nr, device='cuda'):
    """(max |xmap - oracle|, max |xmmse - oracle|, T, oracle T) of BAMP in 'random' mode, B = 1,
    (16, 2, Nr, 1, 1), QPSK, seed 0, 8 dB, three iterations."""
    from bamp import BAMP
    from channel import Channel
    from config import Config
    from data import Data
    from oracle import OracleConfig, bamp_detect
    cfg = Config(16, 2, Nr, 1, 1, batch=1, generator_mode='random', iterations=3, alphabet='QPSK',
                 channel_profile='uniform', channel_truncation='tail', device='cpu')
    np.random.seed(0)
    torch.manual_seed(0)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    x, sym, idx = da.generate_message()
    SNR = cfg.snr(8.0)
    y = A @ x + ch.awgn(SNR)
    oc = OracleConfig(16, 2, Nr, Lin=1, Lh=1, B=1, alphabet='QPSK', mode='random', iterations=3)
    o = bamp_detect(A.numpy(), y.numpy().reshape(1, -1), SNR, oc)
    cfg.device = 'cuda'
    det = BAMP(cfg)
    L = det(A.to(device), y.to(device), SNR, x.to(device), sym, idx)
    T = int(L.loss['T'])
    b = det.last.buf
    dmap = float(np.max(np.abs(b.xmap.cpu().numpy().reshape(1, -1) - o['xmap'])))
    dmm = float(np.max(np.abs(b.xmmse.cpu().numpy().reshape(1, -1) - o['xmmse'])))
    return dmap, dmm, T, int(o['T'])


def test_random_mode_at_odd_n_against_the_oracle(device):
    """The element-wise denoiser at n = 7 (invu one pad float per row, s two), B = 1, three iterations.
    Bound: 4 x the larger of the two errors the build that required n % 4 == 0 shows against the
    oracle at (16, 2, 8, 1, 1), same seed and iterations (the factor covers the different reduction
    length and tile edge).  Measured on an MI355X: n = 8 before this change 2.70e-7 (xmap) and 2.09e-7
    (xmmse), so the bound is 1.08e-6; n = 7 here 1.74e-7 (xmap) and 4.47e-8 (xmmse)."""
    dmap, dmm, T, To = random_mode_errors(7)
    print("'random' n = 7: max |xmap - oracle|", dmap, 'max |xmmse - oracle|', dmm, 'T', T, 'oracle T', To,
          'bound', 4 * RANDOM_PARENT_ERR)
    assert T == To
    assert max(dmap, dmm) <= 4 * RANDOM_PARENT_ERR, (dmap, dmm, RANDOM_PARENT_ERR)


def test_published_shape_trials_equal_sequential_forwards(device):
    """Nt=1344 Na=84 Nr=73 Lh=6 Lin=32, OOK, segmented (bamp_model.py), 20 iterations: N = 43008,
    n = 2701 (odd: both padded strides), 672 column tiles per trial, block-banded H."""
    from bamp import BAMP
    from channel import Channel
    from data import Data
    nE = 4
    cfg = wi.published_config(iterations=20)
    np.random.seed(3)
    torch.manual_seed(3)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    assert tuple(A.shape[-2:]) == (2701, 43008)
    SNR = cfg.snr(9.0)
    inp = dict(A=A.to(device), SNR=SNR, x=[], sym=[], idx=[], y=[])
    for _ in range(nE):
        x, sym, idx = da.generate_message()
        inp['x'].append(x.to(device)); inp['sym'].append(sym); inp['idx'].append(idx)
        inp['y'].append((A @ x + ch.awgn(SNR)).to(device))
    det = BAMP(wi.published_config(device='cuda', iterations=20))
    seq = [_forward(det, inp, j, inp['y'][j]) for j in range(nE)]
    recs, xmap, xm, var = _trials(det, inp, tuple(range(nE)))
    print('published shape: T', [r[0] for r in recs], 'fer', [r[2]['fer'] for r in recs])
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (xmap[j], xm[j], var[j]), seq[j])
        if d:
            bad[j] = d
    assert not bad, bad
    assert all(r[3] == 0 for r in recs)
