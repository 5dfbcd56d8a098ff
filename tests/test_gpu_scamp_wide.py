"""SCAMP at any Nt on the GPU (launch engine): the g15 points (tests/golden/make_g15_scamp_wide.py),
coupling blocks wider than 128 columns and Nt that is no power of two (M = Nt/Na is): blocks that
straddle the A^H column tiles, a partial last column tile (Nt = 168, Lin = 3: 2N = 1008), M = 2,
42 column tiles per trial (Nt = 1344).

1. sequential B = 1 forwards against g15 (the reference at batch = 1): every counting metric of all
   40 trials, no trial exempt (the CPU oracle meets the same bar: test_scamp_wide_cpu.py).  T is
   printed, not asserted: at B = 1 the allclose(psi) exit is decided by rounding.
2. SCAMP.forward_trials (E = 40, 33, 1) against those sequential forwards: T_e, every counter and
   nan_state equal, xmap / xmmse / psi BIT-equal; psi frozen at odd and at even T_e.
3. isolation: trial 5's y scaled by 1e6, or set to NaN, leaves every other trial bit-equal, and the
   victim equal to its own sequential forward.
4. B = 48 (a full 32-row tile and a partial one) against the reference: VER and SER within 1e-3 (the
   project's parity bar), T = 20, and two further forwards on the same inputs return the same bits.
5. ShardedSCAMP over two slices of 24 trials in one process (two threads whose all-reduce hook
   meets on a barrier) against the whole-batch forward: T and every counter.
6. Nt = 48 (coupling-block boundaries inside a column tile, which no g15 point has) against the
   numpy oracle after four iterations.
"""
import functools
import threading

import numpy as np
import pytest
import torch

import golden_io as gio
import scamp_wide_inputs as wi

pytestmark = pytest.mark.gpu

E = wi.E_G15
VICTIM = 5                                     # a row inside the first tile, among live neighbours


def _detector(name):
    import amp_native as nat
    from scamp import SCAMP
    return SCAMP(wi.config_of(name, device='cuda'), engine=nat.ENGINE_LAUNCHES)


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
def sequential(name):
    """The 40 trials as sequential B = 1 forwards of the launch engine.  Computed once, shared,
    never modified."""
    det = _detector(name)
    inp = wi.device_inputs(name)
    return [_forward(det, inp, j, inp['y'][j]) for j in range(E)]


def _trials(name, ids, ys=None):
    det = _detector(name)
    inp = wi.device_inputs(name)
    pick = lambda v: [v[j] for j in ids]   # noqa: E731
    Ls = det.forward_trials(inp['W'], inp['A'], ys if ys is not None else pick(inp['y']), inp['SNR'], pick(inp['x']),
                            pick(inp['sym']), pick(inp['idx']))
    recs = [_record(L) for L in Ls]
    assert all(L.arithmetic == 'f32' for L in Ls)
    xmap, xm, psi = (t.reshape(len(ids), -1) for t in det.last_trials)
    return recs, xmap, xm, psi


@functools.lru_cache(maxsize=None)
def grouped40(name):
    return _trials(name, tuple(range(E)))


def _differences(rec, bufs, ref):
    """Keys on which one trial (record, (xmap, xmmse, psi) rows) differs from a sequential forward."""
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
        for key, got, want in zip(('xmap', 'xmmse', 'psi'), bufs, ref[4:7]):
            if not gio.bits_equal(got, want):
                d[key] = 'bits differ'
    return d


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_sequential_forwards_match_reference_g15(device, name):
    seq = sequential(name)
    ref = wi.G15[name]['trials']
    diff = {}
    for j in range(E):
        d = {k: (seq[j][2][k], ref[j][k]) for k in gio.COUNT_KEYS if seq[j][2][k] != ref[j][k]}
        if d:
            diff[j] = d
    tdiff = [(j, seq[j][0], int(ref[j]['T'])) for j in range(E) if seq[j][0] != int(ref[j]['T'])]
    print(name, 'trials whose T differs from the reference:', len(tdiff), '(the CPU oracle:',
          wi.G15[name]['oracle_T_differs'], ')', tdiff)
    assert all(r[3] == 0 for r in seq), [r[3] for r in seq]
    assert not diff, diff


@pytest.mark.parametrize('nE', [40, 33, 1])
@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_wide_trials_equal_sequential_forwards(device, name, nE):
    seq = sequential(name)
    recs, xmap, xm, psi = grouped40(name) if nE == 40 else _trials(name, tuple(range(nE)))
    bad = {}
    for j in range(nE):
        d = _differences(recs[j], (xmap[j], xm[j], psi[j]), seq[j])
        if d:
            bad[j] = d
    Ts = [r[0] for r in recs]
    print(name, nE, 'T', Ts)
    assert not bad, bad
    if nE == 40:
        # psi is frozen in either ping-pong buffer: both parities, where the reference's exits have both
        for par in {int(t['T']) % 2 for t in wi.G15[name]['trials']}:
            assert any(t % 2 == par for t in Ts), (par, Ts)


@pytest.mark.parametrize('kind', ['huge', 'nan'])
@pytest.mark.parametrize('name', ['trials_OOK_Nt96', 'trials_OOK_Nt1344'])
def test_wide_trials_isolated_from_a_bad_trial(device, name, kind):
    base_recs, bxmap, bxm, bpsi = grouped40(name)
    inp = wi.device_inputs(name)
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
    # the victim is its own sequential forward on the same modified y (its float64 fix-up included)
    own = _forward(_detector(name), inp, VICTIM, ys[VICTIM])
    d = _differences(recs[VICTIM], (xmap[VICTIM], xm[VICTIM], psi[VICTIM]), own)
    print(name, kind, 'victim T', recs[VICTIM][0], 'nan_state', recs[VICTIM][3])
    assert not d, d
    if kind == 'nan':
        assert bool(torch.isnan(psi[VICTIM]).all()) and recs[VICTIM][0] == wi.G15[name]['iterations']


def _batch_forward(det, inp):
    L = det(inp['W'], inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
    rec = _record(L)
    b = det.last.buf
    return rec, (b.xmap.clone(), b.xmmse.clone(), b.psi.clone())


@functools.lru_cache(maxsize=None)
def whole_batch(name):
    """The B = 48 forward of the launch engine: (record, (xmap, xmmse, psi)).  Shared, never modified."""
    return _batch_forward(_detector(name), wi.device_inputs(name))


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_wide_batch_point(device, name):
    ref = wi.G15[name]['loss']
    rec, bufs = whole_batch(name)
    for k in ('ver', 'ser'):
        print(name, k, rec[2][k], ref[k])
    for k in ('ver', 'ser'):                       # the project's parity bar
        assert abs(rec[2][k] - ref[k]) <= 1e-3, (k, rec[2][k], ref[k])
    assert rec[0] == 20 == int(ref['T']), rec[0]
    det = _detector(name)
    for _ in range(2):
        rec2, bufs2 = _batch_forward(det, wi.device_inputs(name))
        assert rec2[0] == rec[0] and np.array_equal(rec2[1], rec[1], equal_nan=True)
        for key, a, b in zip(('xmap', 'xmmse', 'psi'), bufs2, bufs):
            assert gio.bits_equal(a, b), key


def test_block_boundaries_inside_a_tile_against_the_oracle(device):
    """Nt = 48 (M = 8): coupling blocks narrower than the 64-column A^H tile whose boundaries fall
    inside tiles, so psi cannot be formed in a tile's epilogue.  No g15 point has such a shape; the
    numpy oracle is the reference here.  Four iterations at B = 32, before rounding can move the
    two float32 computations apart: psi (a mean of 48 squares of O(1) values per block) within 1e-3
    and xmap within 5e-3 (smoke()'s bar for a float32 detector state) of the oracle's, where a psi
    formed from a partly written block is off by O(0.1)."""
    import amp_native as nat
    from channel import Channel
    from config import Config
    from data import Data
    from oracle import OracleConfig, scamp_detect
    from scamp import SCAMP
    shape = (48, 6, 12, 4, 2)
    cfg = Config(*shape, batch=32, generator_mode='sparc', iterations=4, alphabet='QPSK', channel_profile='uniform',
                 channel_truncation='tail', device='cpu')
    np.random.seed(0)
    torch.manual_seed(0)
    ch, da = Channel(cfg), Data(cfg)
    W, A = ch.generate_as_sparc()
    x, sym, idx = da.generate_message()
    SNR = cfg.snr(6.0)
    y = A @ x + ch.awgn(SNR)
    oc = OracleConfig(shape[0], shape[1], shape[2], Lin=shape[3], Lh=shape[4], B=32, alphabet='QPSK', mode='sparc',
                      iterations=4)
    o = scamp_detect(W.numpy().reshape(oc.Lout, oc.Lin), A.numpy(), y.numpy().reshape(32, -1), SNR, oc)
    cfg.device = 'cuda'
    det = SCAMP(cfg, engine=nat.ENGINE_LAUNCHES)
    L = det(W.to(device), A.to(device), y.to(device), SNR, x.to(device), sym, idx)
    assert int(L.loss['T']) == int(o['T']) == 4
    b = det.last.buf
    dpsi = float(np.max(np.abs(b.psi.cpu().numpy() - o['psi'])))
    dx = float(np.max(np.abs(b.xmap.cpu().numpy() - o['xmap'])))
    print('Nt=48: max |psi - oracle|', dpsi, 'max |xmap - oracle|', dx)
    assert dpsi <= 1e-3 and dx <= 5e-3, (dpsi, dx)


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


def test_wide_sharded_slices_equal_whole_batch(device, monkeypatch):
    import amp_native as nat
    from loss import counts_to_vector
    from scamp import ShardedSCAMP
    name = 'batch_QPSK_Nt192'
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

    class Slice(ShardedSCAMP):
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
                L = det(inp['W'], inp['A'], inp['y'], inp['SNR'], inp['x'], inp['sym'], inp['idx'])
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
