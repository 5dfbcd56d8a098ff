"""VAMP trial batches over several channels, on the CPU (no GPU needed).

* g19 (tests/golden/make_g19_vamp_trials_channels.py: the reference's VAMP at batch = 1, the channel
  and its SVD redrawn every res = 5 epochs, 40 epochs, three shapes) is reproduced by the numpy
  oracle fed by the build's RNG replica in that redraw order: every counting metric of all 40 trials
  of every point.  T is not compared per trial (at B = 1 the allclose exit is decided by rounding;
  the count of differing trials is printed and equals the file's oracle_T_differs).
* amp_vamp_trials_ch_run / _ch_workspace_bytes are declared in include/amp_sparc.h, bound and
  exported; the byte query equals the single-channel query at per_channel >= trials, grows by exactly
  (G - 1) x (the three packed operators + s2 of one channel) otherwise, and is 0 for per_channel < 1,
  a batch or refused shapes.
* the run answers AMP_E_ARG for per_channel = 0, B != 1, the persistent engine, split-precision
  GEMMs and more channels than a grid axis before it reads a buffer.
* forward_trials raises ValueError on a channel count that is not ceil(E / per_channel), on factors
  that disagree in their channel count or shapes, and without a valid per_channel.
* Model(config, 'vamp', group_trials=n, trial_channels=c) with a stand-in detector that has
  trials_per_channel = True: whole blocks per call, the reference's draw order (channel, SVD, message,
  noise), results and exported files equal to the per-epoch loop, a short last block, and a block
  longer than group_trials through single-channel chunks.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import golden_io as gio
import vamp_trials_channels_inputs as vc
from oracle import OracleConfig, loss_dict, vamp_detect

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('amp_vamp_trials_ch_workspace_bytes', 'amp_vamp_trials_ch_run')


def test_g19_is_the_reference_at_res_5():
    assert vc.GOLDEN_POINTS == ['vamp_OOK_Nt16', 'vamp_OOK_Nt6', 'vamp_QPSK_Nt32']
    for name in vc.GOLDEN_POINTS:
        e = vc.G19[name]
        assert e['res'] == 5 and e['seed'] == 3 and e['iterations'] == 20 and len(e['trials']) == vc.E == 40
        assert len({int(t['T']) for t in e['trials']}) >= 5, name        # ragged exits inside the blocks


@pytest.mark.parametrize('name', vc.GOLDEN_POINTS)
def test_oracle_in_redraw_order_matches_g19(name):
    e = vc.G19[name]
    inp = vc.golden_inputs(name)
    cfg = OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=1, alphabet=e['alphabet'],
                       mode=e['mode'], iterations=e['iterations'])
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    bad, tdiff = {}, []
    for j, ref in enumerate(e['trials']):
        o = vamp_detect(inp['U'][j].numpy(), inp['s'][j].numpy(), inp['Vh'][j].numpy(), c(inp['y'][j]), inp['SNR'], cfg)
        got = loss_dict(o['r'], o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
        if int(o['T']) != int(ref['T']):
            tdiff.append((j, int(o['T']), int(ref['T'])))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert not bad, bad
    assert len(tdiff) == e['oracle_T_differs']
    # the channel and its factors really change every res epochs, and only then
    for key in ('A', 'U', 's', 'Vh'):
        same = [inp[key][j] is inp[key][j - 1] for j in range(1, vc.E)]
        assert same == [j % 5 != 0 for j in range(1, vc.E)], key


def _ru(v, m):
    return (v + m - 1) // m * m


def _channel_bytes(d, k):
    """Bytes of ONE channel's three packed f32 operators (s U^H [2k x 2n], Vh [2k x 2N], V [2N x 2k]:
    columns padded to the column tile, the reduction to 64) plus its s2 (a whole 256-byte granule)."""
    N, n, bn = d.N, d.n, (128 if 2 * d.M <= 128 else 256)
    ops = [(_ru(2 * k, 128), _ru(2 * n, 64)), (_ru(2 * k, 128), _ru(2 * N, 64)), (_ru(2 * N, bn), _ru(2 * k, 64))]
    return sum(4 * ncp * kap for ncp, kap in ops) + _ru(4 * k, 256)


def test_vamp_trials_ch_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    assert 'vamp_model.py:45-61' in header


@pytest.mark.parametrize('name', vc.POINT_IDS)
def test_vamp_trials_ch_workspace_bytes(name):
    import amp_native as nat
    lib = nat.lib()
    one, ch = lib.amp_vamp_trials_workspace_bytes, lib.amp_vamp_trials_ch_workspace_bytes
    d = vc.config_of(name).dims()
    k = min(d.n, d.N)
    for E in (1, 33, 40):
        single = one(C.byref(d), k, 20, E)
        assert single > 0
        for R in (E, E + 1, 1000):                             # one channel: the single-channel bytes
            assert ch(C.byref(d), k, 20, E, R) == single, (E, R)
        for R in (1, 5, 32, 33):
            if R >= E:
                continue
            G = -(-E // R)
            assert ch(C.byref(d), k, 20, E, R) == single + (G - 1) * _channel_bytes(d, k), (E, R, G)
    assert ch(C.byref(d), k, 20, 40, 0) == 0 and ch(C.byref(d), k, 20, 40, -3) == 0
    assert ch(C.byref(d), k, 20, 0, 1) == 0 and ch(C.byref(d), k, 0, 40, 5) == 0
    assert ch(C.byref(d), 0, 20, 40, 5) == 0 and ch(C.byref(d), k + 1, 20, 40, 5) == 0
    d2 = vc.config_of(name, batch=2).dims()                    # dims describe ONE trial
    assert ch(C.byref(d2), k, 20, 40, 5) == 0
    assert ch(C.byref(d), k, 20, 2 ** 31 - 1, 5) == 0          # trials x columns beyond 32-bit offsets
    assert ch(C.byref(d), k, 20, 70000, 1) == 0                # more channels than a grid axis holds
    odd = vc.config_of(name).dims()
    odd.N += 1                                                 # odd N: refused by amp_vamp_run
    assert ch(C.byref(odd), k, 20, 40, 5) == 0


def test_vamp_trials_workspace_bytes_method():
    import amp_native as nat
    from vamp import VAMP
    cfg = vc.config_of('vamp_OOK_Nt16')
    det = VAMP(cfg)
    d = cfg.dims()
    assert VAMP.trials_per_channel is True
    assert det.trials_workspace_bytes(40, 5) == nat.lib().amp_vamp_trials_ch_workspace_bytes(C.byref(d), 60, 20, 40, 5) > 0
    assert det.trials_workspace_bytes(40, 40) == nat.lib().amp_vamp_trials_workspace_bytes(C.byref(d), 60, 20, 40)


def test_vamp_trials_ch_run_refuses_before_touching_the_device():
    import amp_native as nat
    lib = nat.lib()
    cfg = vc.config_of('vamp_OOK_Nt16')
    cst = cfg.constellation()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def run(d, trials=8, per=2, engine=nat.ENGINE_LAUNCHES, gemm=nat.GEMM_AUTO, null=None):
        a = nat.AmpVampArgs()
        a.U = a.s = a.Vh = a.y = a.r = a.xmmse = a.var = a.status = a.ws = ptr
        if null:
            setattr(a, null, None)
        a.ws_bytes = 0                                   # a valid call would stop here, before any launch
        a.k, a.max_iter, a.engine, a.gemm, a.noise_var, a.sparsity = 60, 20, engine, gemm, 0.1, 0.125
        return lib.amp_vamp_trials_ch_run(C.byref(d), C.byref(cst), C.byref(a), None, trials, per, None)

    d = cfg.dims()
    err = lambda: lib.amp_last_error().decode()   # noqa: E731
    assert run(d, per=0) == -1 and 'per_channel = 0' in err()
    assert run(d, per=-2) == -1 and 'per_channel = -2' in err()
    assert run(vc.config_of('vamp_OOK_Nt16', batch=2).dims()) == -1 and 'ONE trial' in err()
    assert run(d, trials=0) == -1 and 'trials = 0' in err()
    assert run(d, engine=nat.ENGINE_PERSISTENT) == -1 and 'persistent engine' in err()
    for g in (nat.GEMM_X3, nat.GEMM_H2):
        assert run(d, gemm=g) == -1 and 'f32 GEMMs only' in err()
    assert run(d, trials=70000, per=1) == -1 and 'channels' in err()
    for field in ('U', 's', 'Vh', 'y', 'ws'):
        assert run(d, null=field) == -1 and 'null pointer' in err()
    assert run(d) == -1 and 'workspace' in err()


def test_vamp_forward_trials_rejects_wrong_channels():
    from vamp import VAMP
    cfg = vc.config_of('vamp_OOK_Nt16')
    n, N = cfg.Nr * cfg.Lout, cfg.Nt * cfg.Lin
    k = min(n, N)
    E = 7
    ys = [torch.zeros(1, n, 1, dtype=torch.complex64)] * E
    xs = [torch.zeros(1, N, 1, dtype=torch.complex64)] * E
    lab = [np.zeros(cfg.Na * cfg.Lin, np.int64)] * E
    U, s, Vh = torch.zeros(n, k, dtype=torch.complex64), torch.ones(k), torch.zeros(k, N, dtype=torch.complex64)
    det = VAMP(cfg)
    ft = lambda Us, ss, Vhs, R: det.forward_trials(Us, ss, Vhs, ys, 10.0, xs, lab, lab, per_channel=R)   # noqa: E731
    # a wrong channel count: ceil(7 / 2) = 4, ceil(7 / 3) = 3
    for G, R in ((3, 2), (5, 2), (7, 2), (2, 3)):
        with pytest.raises(ValueError, match='channels for 7 trials'):
            ft([U] * G, [s] * G, [Vh] * G, R)
    with pytest.raises(ValueError, match='channels for 7 trials'):
        ft(torch.zeros(2, n, k, dtype=torch.complex64), torch.ones(2, k), torch.zeros(2, k, N, dtype=torch.complex64), 3)
    with pytest.raises(ValueError, match='channels for 7 trials'):
        ft(U, s, Vh, 3)                                                       # one channel for three
    # the three disagree on G
    for Gs in ((4, 3, 4), (4, 4, 5), (3, 4, 4)):
        with pytest.raises(ValueError, match='channels for 7 trials'):
            ft([U] * Gs[0], [s] * Gs[1], [Vh] * Gs[2], 2)
    with pytest.raises(ValueError, match='channels for 7 trials'):
        ft([U] * 4, torch.ones(3, k), [Vh] * 4, 2)
    # or on shapes
    with pytest.raises(ValueError, match='disagree in shape'):
        ft([U] * 4, [s] * 3 + [torch.ones(k - 1)], [Vh] * 4, 2)
    with pytest.raises(ValueError, match='disagree in shape'):
        ft([U] * 3 + [U[:, :k - 1]], [s] * 4, [Vh] * 4, 2)
    with pytest.raises(ValueError, match='disagree in shape'):
        ft([U] * 4, [s] * 4, torch.zeros(4, k - 1, N, dtype=torch.complex64), 2)
    for R in (None, 0):
        with pytest.raises(ValueError, match='per_channel'):
            ft([U] * 4, [s] * 4, [Vh] * 4, R)


def test_svd_channel_stack_does_not_copy_stacked_factors():
    from vamp import _svd_channel_stack
    G, n, k, N = 3, 6, 4, 4
    U, s, Vh = torch.zeros(G, n, k, dtype=torch.complex64), torch.ones(G, k), torch.zeros(G, k, N, dtype=torch.complex64)
    Uc, sc, Vhc, R, *dims = _svd_channel_stack(U, s, Vh, 6, 2)
    assert (R, dims) == (2, [n, k, N])
    assert Uc.data_ptr() == U.data_ptr() and sc.data_ptr() == s.data_ptr() and Vhc.data_ptr() == Vh.data_ptr()
    Ul, sl, Vl, *_ = _svd_channel_stack(list(U), [v.double() for v in s], list(Vh), 6, 2)
    assert Ul.shape == U.shape and sl.dtype == torch.float32 and sl.shape == (G, k) and Vl.is_contiguous()


class FakeVampChannelsAmp:
    """Stands in for VAMP: forward and forward_trials (one (U, s, Vh), or three lists with per_channel)
    with their signatures.  Every trial's Loss carries values derived from its own y and its own
    factors, so the totals depend on which trial was detected with which channel."""
    trials_per_channel = True

    def __init__(self, config):
        from loss import Loss
        self.Loss, self.config = Loss, config
        self.L = Loss(config)
        self.log = []          # ('single' | 'trials' | 'channels', number of trials, trials per channel)
        self.seen = []         # every detected (y, U, s, Vh), in order

    def _rates(self, y, ch):
        v = float(y.abs().sum()) + sum(float(t.abs().sum()) for t in ch)
        return [v % 1.0] + [v] * 13

    def __call__(self, U, s, Vh, y, SNR, x, sym, idx):
        self.log.append(('single', 1, None))
        self.seen.append((y.clone(), U.clone(), s.clone(), Vh.clone()))
        self.L.dump()
        self.L.loss = {'T': 0}
        self.L.record(self._rates(y, (U, s, Vh)), 3)
        return self.L

    def forward_trials(self, U, s, Vh, ys, SNR, xs, syms, idxs, per_channel=None):
        assert len(ys) == len(xs) == len(syms) == len(idxs)
        if per_channel is None:
            assert all(isinstance(t, torch.Tensor) for t in (U, s, Vh))
            chans = [(U, s, Vh)] * len(ys)
            self.log.append(('trials', len(ys), None))
        else:
            G = -(-len(ys) // per_channel)
            assert all(isinstance(t, list) and len(t) == G for t in (U, s, Vh)) and G > 1
            chans = [(U[e // per_channel], s[e // per_channel], Vh[e // per_channel]) for e in range(len(ys))]
            self.log.append(('channels', len(ys), per_channel))
        out = []
        for y, ch in zip(ys, chans):
            self.seen.append((y.clone(),) + tuple(t.clone() for t in ch))
            L = self.Loss(self.config)
            L.record(self._rates(y, ch), 3)
            out.append(L)
        return out


def _cfg(B=1, mode='segmented'):
    from config import Config
    return Config(16, 2, 32, 1, 1, batch=B, generator_mode=mode, iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


# (res, group_trials, trial_channels) -> the calls of one SNR point over 10 epochs
CASES = {(4, 8, 2): [('channels', 8, 4), ('trials', 2, None)],           # 4 + 4, then 2
         (1, 8, 8): [('channels', 8, 1), ('channels', 2, 1)],            # eight, then two
         (1, 8, 3): [('channels', 3, 1)] * 3 + [('single', 1, None)],    # at most 3 blocks per call
         (4, 9, 8): [('channels', 8, 4), ('trials', 2, None)],           # at most 9 trials: two whole blocks
         (3, 7, 4): [('channels', 6, 3), ('channels', 4, 3)],            # a short last block closes its call
         (4, 3, 2): [('trials', 3, None), ('single', 1, None)] * 2 + [('trials', 2, None)]}   # blocks longer than n


@pytest.mark.parametrize('case', sorted(CASES))
def test_model_vamp_trial_channels_blocks_order_and_totals(tmp_path, case):
    from model import Model
    res, gt, tcap = case
    cfg = _cfg()
    runs = {}
    for key, kw in (('base', {}), ('grouped', dict(group_trials=gt, trial_channels=tcap))):
        amp = FakeVampChannelsAmp(cfg)
        m = Model(cfg, 'vamp', path=str(tmp_path / key), amp=amp, seed=11, **kw)
        runs[key] = (amp, m.simulate(epochs=10, start=0, final=1.0, step=1, res=res))
    base, grouped = runs['base'][0], runs['grouped'][0]
    assert grouped.log == CASES[case] * 2                                   # two SNR points
    assert base.log == [('single', 1, None)] * 20
    # the reference's draw order (channel, SVD, message, noise): the same y with the same factors, in the
    # same order, as the per-epoch loop
    assert len(base.seen) == len(grouped.seen) == 20
    for a, b in zip(base.seen, grouped.seen):
        assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert json.dumps(runs['base'][1], sort_keys=True) == json.dumps(runs['grouped'][1], sort_keys=True)
    for p in ('0.0.json', '1.0.json'):
        assert open(tmp_path / 'base' / p, 'rb').read() == open(tmp_path / 'grouped' / p, 'rb').read()


def test_model_vamp_trial_channels_workspace_cap(tmp_path):
    """The channels per call are capped by the detector's workspace query against trials_ws_limit."""
    from model import Model
    cfg = _cfg()
    amp = FakeVampChannelsAmp(cfg)
    amp.trials_workspace_bytes = lambda trials, per: 1000 * (-(-trials // per))     # 1000 bytes per channel
    m = Model(cfg, 'vamp', path=str(tmp_path), amp=amp, seed=2, group_trials=8, trial_channels=8,
              trials_ws_limit=3500)
    m.simulate(epochs=10, start=0, final=0.0, step=1, res=1)
    assert amp.log == [('channels', 3, 1)] * 3 + [('single', 1, None)]


def test_model_vamp_without_the_attribute_still_raises(tmp_path):
    from model import Model
    cfg = _cfg()
    amp = FakeVampChannelsAmp(cfg)
    amp.trials_per_channel = False
    with pytest.raises(ValueError, match='trial_channels'):
        Model(cfg, 'vamp', path=str(tmp_path), amp=amp, group_trials=8, trial_channels=2)
    with pytest.raises(ValueError, match='trial_channels'):
        Model(cfg, 'vamp', path=str(tmp_path), amp=FakeVampChannelsAmp(cfg), trial_channels=2)    # no group_trials
