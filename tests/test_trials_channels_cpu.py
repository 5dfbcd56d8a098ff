"""BAMP / SCAMP trial batches over several channels, on the CPU (no GPU needed).

* g18 (tests/golden/make_g18_trials_channels.py: the reference at batch = 1, the channel redrawn
  every res = 5 epochs, 40 epochs, at the g13 bamp_OOK_Nt16 and the g14 scamp_OOK_Nt16 shapes) is
  reproduced by the numpy oracle fed by the build's RNG replica in that redraw order: every counting
  metric of all 40 trials of both points.  T is not compared per trial (at B = 1 the allclose exit is
  decided by rounding; test_trials_cpu.py).
* amp_{bamp,scamp}_trials_ch_run / _ch_workspace_bytes are declared in include/amp_sparc.h, bound
  and exported; the byte query equals the single-channel query at per_channel >= trials, grows by
  exactly (G - 1) x (packed operators + band ranges of one channel) otherwise, and is 0 for
  per_channel < 1, a batch or refused shapes.
* the run answers AMP_E_ARG for per_channel = 0, B != 1, the persistent engine and split-precision
  GEMMs before it reads a buffer.
* forward_trials raises ValueError on a channel count that is not ceil(E / per_channel).
* Model(group_trials=n, trial_channels=c) with a stand-in detector: whole blocks per call, the
  reference's draw order, results and exported files equal to the per-epoch loop; 'vamp' raises.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import golden_io as gio
import trials_channels_inputs as tc
from oracle import OracleConfig, bamp_detect, loss_dict, scamp_detect

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('amp_bamp_trials_ch_workspace_bytes', 'amp_bamp_trials_ch_run',
               'amp_scamp_trials_ch_workspace_bytes', 'amp_scamp_trials_ch_run')


def test_g18_is_the_reference_at_res_5():
    assert tc.GOLDEN_POINTS == ['bamp_OOK_Nt16', 'scamp_OOK_Nt16']
    for name in tc.GOLDEN_POINTS:
        e = tc.G18[name]
        assert e['res'] == 5 and len(e['trials']) == tc.E == 40
        assert len({int(t['T']) for t in e['trials']}) >= 5, name        # ragged exits


@pytest.mark.parametrize('name', tc.GOLDEN_POINTS)
def test_oracle_in_redraw_order_matches_g18(name):
    e = tc.G18[name]
    inp = tc.golden_inputs(name)
    cfg = OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=1, alphabet=e['alphabet'],
                       mode='segmented', iterations=e['iterations'])
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    bad, tdiff = {}, []
    for j, ref in enumerate(e['trials']):
        A = inp['A'][j].numpy()
        if e['algo'] == 'bamp':
            o = bamp_detect(A, c(inp['y'][j]), inp['SNR'], cfg)
        else:
            o = scamp_detect(inp['W'].numpy().reshape(cfg.Lout, cfg.Lin), A, c(inp['y'][j]), inp['SNR'], cfg)
        got = loss_dict(o['xmap'], o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
        if int(o['T']) != int(ref['T']):
            tdiff.append((j, int(o['T']), int(ref['T'])))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert not bad, bad
    # the channel really changes every res epochs, and only then
    same = [inp['A'][j] is inp['A'][j - 1] for j in range(1, tc.E)]
    assert same == [j % 5 != 0 for j in range(1, tc.E)]


def _ru(v, m):
    return (v + m - 1) // m * m


def _channel_bytes(algo, d):
    """Bytes of ONE channel's packed f32 operators plus its band ranges (whole 256-byte granules)."""
    N, n, bn = d.N, d.n, (128 if 2 * d.M <= 128 else 256)
    if algo == 'bamp':
        ops = [(_ru(n, 128), _ru(N, 64), 128), (_ru(2 * n, 128), _ru(2 * N, 64), 128),
               (_ru(N, 128), _ru(n, 64), 128), (_ru(2 * N, bn), _ru(2 * n, 64), bn)]
    else:
        ops = [(_ru(2 * n, 128), _ru(2 * N, 64), 128), (_ru(2 * N, bn), _ru(2 * n, 64), bn)]
    return sum(4 * ncp * kap + _ru(8 * (ncp // tile), 256) for ncp, kap, tile in ops)


def test_trials_ch_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name


@pytest.mark.parametrize('name', tc.POINT_IDS)
def test_trials_ch_workspace_bytes(name):
    import amp_native as nat
    lib = nat.lib()
    algo = tc.algo_of(name)
    one = getattr(lib, f'amp_{algo}_trials_workspace_bytes')
    ch = getattr(lib, f'amp_{algo}_trials_ch_workspace_bytes')
    d = tc.config_of(name).dims()
    for E in (1, 33, 40):
        single = one(C.byref(d), 20, E)
        assert single > 0
        for R in (E, E + 1, 1000):                             # one channel: the single-channel bytes
            assert ch(C.byref(d), 20, E, R) == single, (E, R)
        for R in (1, 5, 32, 33):
            if R >= E:
                continue
            G = -(-E // R)
            assert ch(C.byref(d), 20, E, R) == single + (G - 1) * _channel_bytes(algo, d), (E, R, G)
    assert ch(C.byref(d), 20, 40, 0) == 0 and ch(C.byref(d), 20, 40, -3) == 0
    assert ch(C.byref(d), 20, 0, 1) == 0 and ch(C.byref(d), 0, 40, 5) == 0
    d2 = tc.config_of(name, batch=2).dims()                    # dims describe ONE trial
    assert ch(C.byref(d2), 20, 40, 5) == 0
    big = tc.config_of(name).dims()                            # trials x columns beyond 32-bit offsets
    assert ch(C.byref(big), 20, 2 ** 31 - 1, 5) == 0
    assert ch(C.byref(d), 20, 70000, 1) == 0                   # more channels than a grid axis holds
    if algo == 'scamp':
        wide = tc.config_of(name).dims()
        wide.Lin = 65                                          # more coupling blocks than amp_scamp_run takes
        assert ch(C.byref(wide), 20, 40, 5) == 0
    else:
        odd = tc.config_of(name).dims()
        odd.N += 1                                             # odd N: refused by amp_bamp_run
        assert ch(C.byref(odd), 20, 40, 5) == 0


def test_bamp_trials_ch_run_refuses_before_touching_the_device():
    import amp_native as nat
    lib = nat.lib()
    cfg = tc.config_of('bamp_OOK_Nt16')
    cst = cfg.constellation()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def run(d, trials=8, per=2, gemm=nat.GEMM_AUTO, denoiser=0):
        a = nat.AmpBampArgs()
        a.H = a.y = a.xmap = a.xmmse = a.var = a.status = a.ws = ptr
        a.ws_bytes = 0                                   # a valid call would stop here, before any launch
        a.max_iter, a.denoiser, a.gemm, a.noise_var = 20, denoiser, gemm, 0.1
        return lib.amp_bamp_trials_ch_run(C.byref(d), C.byref(cst), C.byref(a), None, trials, per, None)

    d = cfg.dims()
    err = lambda: lib.amp_last_error().decode()   # noqa: E731
    assert run(d, per=0) == -1 and 'per_channel = 0' in err()
    assert run(tc.config_of('bamp_OOK_Nt16', batch=2).dims()) == -1 and 'ONE trial' in err()
    assert run(d, trials=0) == -1 and 'trials = 0' in err()
    for g in (nat.GEMM_X3, nat.GEMM_H2):
        assert run(d, gemm=g) == -1 and 'f32 GEMMs only' in err()
    assert run(d, denoiser=1) == -1 and 'element-wise' in err()
    assert run(d, trials=70000, per=1) == -1 and 'channels' in err()
    assert run(d) == -1 and 'workspace' in err()


def test_scamp_trials_ch_run_refuses_before_touching_the_device():
    import amp_native as nat
    lib = nat.lib()
    cfg = tc.config_of('scamp_OOK_Nt16')
    cst = cfg.constellation()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def run(d, trials=8, per=2, engine=nat.ENGINE_LAUNCHES, gemm=nat.GEMM_AUTO):
        a = nat.AmpScampArgs()
        a.W = a.A = a.y = a.xmap = a.xmmse = a.psi = a.status = a.ws = ptr
        a.ws_bytes = 0                                   # a valid call would stop here, before any launch
        a.max_iter, a.engine, a.gemm, a.noise_var = 20, engine, gemm, 0.1
        return lib.amp_scamp_trials_ch_run(C.byref(d), C.byref(cst), C.byref(a), None, trials, per, None)

    d = cfg.dims()
    err = lambda: lib.amp_last_error().decode()   # noqa: E731
    assert run(d, per=0) == -1 and 'per_channel = 0' in err()
    assert run(tc.config_of('scamp_OOK_Nt16', batch=2).dims()) == -1 and 'ONE trial' in err()
    assert run(d, trials=0) == -1 and 'trials = 0' in err()
    assert run(d, engine=nat.ENGINE_PERSISTENT) == -1 and 'launch engine only' in err()
    for g in (nat.GEMM_X3, nat.GEMM_H2):
        assert run(d, gemm=g) == -1 and 'f32 GEMMs only' in err()
    assert run(d, trials=70000, per=1) == -1 and 'channels' in err()
    assert run(d) == -1 and 'workspace' in err()


@pytest.mark.parametrize('algo', ['bamp', 'scamp'])
def test_forward_trials_rejects_a_wrong_channel_count(algo):
    from bamp import BAMP
    from scamp import SCAMP
    name = f'{algo}_OOK_Nt16'
    cfg = tc.config_of(name)
    n, N = cfg.Nr * cfg.Lout, cfg.Nt * cfg.Lin
    E = 7
    ys = [torch.zeros(1, n, 1, dtype=torch.complex64)] * E
    xs = [torch.zeros(1, N, 1, dtype=torch.complex64)] * E
    lab = [np.zeros(cfg.Na * cfg.Lin, np.int64)] * E
    H = torch.zeros(n, N, dtype=torch.complex64)
    det = BAMP(cfg) if algo == 'bamp' else SCAMP(cfg)
    head = () if algo == 'bamp' else (torch.ones(cfg.Lout, cfg.Lin),)
    for chans, R in (([H] * 3, 2), ([H] * 5, 2), (torch.zeros(2, n, N, dtype=torch.complex64), 3), ([H] * 7, 2),
                     (H, 3)):
        with pytest.raises(ValueError, match='channels for 7 trials'):      # ceil(7 / 2) = 4, ceil(7 / 3) = 3
            det.forward_trials(*head, chans, ys, 10.0, xs, lab, lab, per_channel=R)
    for R in (None, 0):
        with pytest.raises(ValueError, match='per_channel'):
            det.forward_trials(*head, [H] * 4, ys, 10.0, xs, lab, lab, per_channel=R)


class FakeChannelsAmp:
    """Stands in for BAMP / SCAMP: forward and forward_trials (one channel, or a list with
    per_channel) with their signatures.  Every trial's Loss carries values derived from its own y
    and its own channel, so the totals depend on which trial was detected with which channel."""

    def __init__(self, config, scamp=False):
        from loss import Loss
        self.Loss, self.config, self.skip = Loss, config, (1 if scamp else 0)
        self.L = Loss(config)
        self.log = []          # ('single' | 'trials' | 'channels', number of trials, trials per channel)
        self.seen = []         # every detected (y, channel), in order

    def _rates(self, y, A):
        v = float(y.abs().sum()) + float(A.abs().sum())
        return [v % 1.0] + [v] * 13

    def __call__(self, *a):
        A, y = a[self.skip], a[self.skip + 1]
        self.log.append(('single', 1, None))
        self.seen.append((y.clone(), A.clone()))
        self.L.dump()
        self.L.loss = {'T': 0}
        self.L.record(self._rates(y, A), 3)
        return self.L

    def forward_trials(self, *a, per_channel=None):
        A, ys = a[self.skip], a[self.skip + 1]
        assert len(ys) == len(a[-1]) == len(a[-2]) == len(a[-3])
        if per_channel is None:
            assert isinstance(A, torch.Tensor)
            chans = [A] * len(ys)
            self.log.append(('trials', len(ys), None))
        else:
            assert isinstance(A, list) and len(A) == -(-len(ys) // per_channel) and len(A) > 1
            chans = [A[e // per_channel] for e in range(len(ys))]
            self.log.append(('channels', len(ys), per_channel))
        out = []
        for y, Ae in zip(ys, chans):
            self.seen.append((y.clone(), Ae.clone()))
            L = self.Loss(self.config)
            L.record(self._rates(y, Ae), 3)
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


@pytest.mark.parametrize('det', ['bamp', 'scamp'])
@pytest.mark.parametrize('case', sorted(CASES))
def test_model_trial_channels_blocks_order_and_totals(tmp_path, det, case):
    from model import Model
    res, gt, tcap = case
    cfg = _cfg()
    runs = {}
    for key, kw in (('base', {}), ('grouped', dict(group_trials=gt, trial_channels=tcap))):
        amp = FakeChannelsAmp(cfg, scamp=(det == 'scamp'))
        m = Model(cfg, det, path=str(tmp_path / key), amp=amp, seed=11, **kw)
        runs[key] = (amp, m.simulate(epochs=10, start=0, final=1.0, step=1, res=res))
    base, grouped = runs['base'][0], runs['grouped'][0]
    assert grouped.log == CASES[case] * 2                                   # two SNR points
    assert base.log == [('single', 1, None)] * 20
    # the reference's draw order: the same y with the same channel, in the same order, as the per-epoch loop
    assert len(base.seen) == len(grouped.seen) == 20
    for (ya, Aa), (yb, Ab) in zip(base.seen, grouped.seen):
        assert torch.equal(ya, yb) and torch.equal(Aa, Ab)
    assert json.dumps(runs['base'][1], sort_keys=True) == json.dumps(runs['grouped'][1], sort_keys=True)
    for p in ('0.0.json', '1.0.json'):
        assert open(tmp_path / 'base' / p, 'rb').read() == open(tmp_path / 'grouped' / p, 'rb').read()


def test_model_trial_channels_workspace_cap(tmp_path):
    """The channels per call are capped by the detector's workspace query against trials_ws_limit."""
    from model import Model
    cfg = _cfg()
    amp = FakeChannelsAmp(cfg)
    amp.trials_workspace_bytes = lambda trials, per: 1000 * (-(-trials // per))     # 1000 bytes per channel
    m = Model(cfg, 'bamp', path=str(tmp_path), amp=amp, seed=2, group_trials=8, trial_channels=8,
              trials_ws_limit=3500)
    m.simulate(epochs=10, start=0, final=0.0, step=1, res=1)
    assert amp.log == [('channels', 3, 1)] * 3 + [('single', 1, None)]


def test_model_trial_channels_rejections(tmp_path):
    from model import Model
    cfg = _cfg()
    with pytest.raises(ValueError, match='trial_channels'):
        Model(cfg, 'vamp', path=str(tmp_path), amp=FakeChannelsAmp(cfg), group_trials=8, trial_channels=2)
    with pytest.raises(ValueError, match='trial_channels'):
        Model(cfg, 'bamp', path=str(tmp_path), amp=FakeChannelsAmp(cfg), trial_channels=2)       # no group_trials
    with pytest.raises(ValueError, match='trial_channels'):
        Model(cfg, 'bamp', path=str(tmp_path), amp=FakeChannelsAmp(cfg), group_trials=8, trial_channels=-1)
    with pytest.raises(ValueError, match='group_trials'):
        Model(_cfg(B=2, mode='sparc'), 'scamp', path=str(tmp_path), amp=FakeChannelsAmp(_cfg(B=2, mode='sparc')),
              group_trials=8, trial_channels=2)
    with pytest.raises(ValueError, match='group_trials'):                    # as before without trial_channels
        Model(cfg, 'scamp', path=str(tmp_path), amp=FakeChannelsAmp(cfg), group_trials=8)
