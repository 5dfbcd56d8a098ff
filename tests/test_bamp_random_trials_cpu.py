"""generator_mode='random' trial batches (amp_bamp_random_trials_run, BAMP(config, random_trials=True)) on
the CPU (no GPU needed).

* the two new entry points and AMP_RULE_RANDOM are declared in include/amp_sparc.h, bound in
  amp_native.py and exported by the library;
* the workspace query grows with `trials`, equals amp_bamp_trials_ch_workspace_bytes at the same
  arguments (the carve is shared: the decision's workspace holds either rule's partials) and is 0 for
  a batch, for no trials, for per_channel < 1 and for more channels than a grid axis;
* amp_bamp_random_trials_run answers AMP_E_ARG with a message, before a buffer is read, for B != 1,
  trials / per_channel < 1, more than 65535 channels, a split-precision gemm, another denoiser, null
  pointers, a short workspace, Na > 64 or another rule with a decision, and the shapes amp_bamp_run
  refuses (odd N, M no power of two);
* the other trial entries keep refusing the element-wise denoiser and the 'random' rule;
* BAMP(cfg) still raises for 'random'; BAMP(cfg, random_trials=True) raises ValueError for B != 1
  and for 'sparc' / 'segmented' configs;
* Model in 'random' mode with a stand-in detector: group_trials / trial_channels issue the
  reference's random-call order (Data.random) and their totals equal the per-epoch loop; without a
  detector passed in it builds BAMP(config, random_trials=True);
* g20 (tests/golden/make_g20_bamp_random_trials.py: the reference at batch = 1, 'random', 40 trials
  per channel, three shapes at a low and a high EbN0): the float64 oracle, fed by the build's RNG
  replica, reproduces every counting metric of every stored trial (the points were chosen so).  T is
  not compared per trial (at B = 1 the allclose exit is decided by rounding; test_trials_cpu.py).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import bamp_random_trials_inputs as ri
import golden_io as gio
from oracle import OracleConfig, bamp_detect, loss_dict

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('amp_bamp_random_trials_workspace_bytes', 'amp_bamp_random_trials_run')


def test_random_trials_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    assert '#define AMP_RULE_RANDOM 2' in header
    assert (nat.RULE_SPARC, nat.RULE_SEGMENTED, nat.RULE_RANDOM) == (0, 1, 2)
    assert nat.AmpTrialsDecideArgs.counts.offset == 32 and C.sizeof(nat.AmpTrialsDecideArgs) == 40


@pytest.mark.parametrize('name', sorted(ri.SHAPES))
def test_random_trials_workspace_bytes(name):
    import amp_native as nat
    lib = nat.lib()
    q, ch = lib.amp_bamp_random_trials_workspace_bytes, lib.amp_bamp_trials_ch_workspace_bytes
    cfg = ri.shape_config(name)
    d = cfg.dims()
    last = 0
    for E in (1, 2, 33, 40, 100):
        b = q(C.byref(d), 20, E, E)
        assert b > last, (E, b, last)                            # grows with the trials
        last = b
        for R in (1, 5, 32, 33, E, E + 7):
            assert q(C.byref(d), 20, E, R) == ch(C.byref(d), 20, E, R) > 0, (E, R)
        assert q(C.byref(d), 20, E, E) == lib.amp_bamp_trials_workspace_bytes(C.byref(d), 20, E)
    assert q(C.byref(d), 20, 33, 5) > q(C.byref(d), 20, 33, 33)          # seven channels' operators
    assert q(C.byref(d), 20, 0, 1) == 0 and q(C.byref(d), 20, -2, 1) == 0
    assert q(C.byref(d), 20, 40, 0) == 0 and q(C.byref(d), 20, 40, -3) == 0
    assert q(C.byref(d), 0, 40, 5) == 0
    assert q(C.byref(ri.make_config(*ri.SHAPES[name][:6], batch=2).dims()), 20, 40, 5) == 0     # a batch
    assert q(C.byref(d), 20, 70000, 1) == 0                             # more channels than a grid axis
    odd = cfg.dims()
    odd.N += 1
    assert q(C.byref(odd), 20, 40, 5) == 0


def _dummy():
    buf = (C.c_char * 64)()
    return buf, C.cast(buf, C.c_void_p).value


def test_random_trials_run_refuses_before_touching_the_device():
    import amp_native as nat
    lib = nat.lib()
    cfg = ri.shape_config('16QAM_Nt32')
    cst = cfg.constellation()
    keep, ptr = _dummy()

    def args(gemm=nat.GEMM_AUTO, denoiser=1, ws_bytes=0, **null):
        a = nat.AmpBampArgs()
        a.H = a.y = a.xmap = a.xmmse = a.var = a.status = a.ws = ptr
        for k in null:
            setattr(a, k, None)
        a.ws_bytes = ws_bytes                                # 0: a valid call would stop here, before any launch
        a.max_iter, a.denoiser, a.gemm, a.noise_var = 20, denoiser, gemm, 0.1
        a.P0, a.Ps = 0.9, 0.025
        return a

    def decide(rule=nat.RULE_RANDOM):
        dec = nat.AmpTrialsDecideArgs()
        dec.x = dec.sym = dec.idx = dec.counts = ptr
        dec.ibits_trunc, dec.rule = 4, rule
        return dec

    def run(d, trials=8, per=2, dec=None, **kw):
        a = args(**kw)
        rc = lib.amp_bamp_random_trials_run(C.byref(d), C.byref(cst), C.byref(a), C.byref(dec) if dec else None, trials,
                                            per, None)
        return rc, lib.amp_last_error().decode()

    d = cfg.dims()
    odd = cfg.dims()
    odd.N += 1
    m3 = ri.make_config(12, 4, 5, 2, 1, 'QPSK').dims()               # M = 3
    na65 = ri.make_config(130, 65, 8, 2, 1, 'QPSK').dims()           # M = 2, Na = 65
    cases = [(run(ri.make_config(*ri.SHAPES['16QAM_Nt32'][:6], batch=2).dims()), 'ONE trial'),
             (run(d, trials=0), 'trials = 0'),
             (run(d, trials=-1), 'trials = -1'),
             (run(d, per=0), 'per_channel = 0'),
             (run(d, trials=70000, per=1), 'channels'),
             (run(d, gemm=nat.GEMM_X3), 'f32 GEMMs only'),
             (run(d, gemm=nat.GEMM_H2), 'f32 GEMMs only'),
             (run(d, denoiser=0), 'denoiser 0'),
             (run(d, y=None), 'null pointer'),
             (run(d, ws=None), 'null pointer'),
             (run(d, status=None), 'null pointer'),
             (run(d), 'workspace'),
             (run(d, ws_bytes=4096), 'workspace'),
             (run(d, dec=decide()), 'workspace'),                    # a decision it takes: refused for the bytes only
             (run(na65, dec=decide()), 'Na <= 64'),
             (run(na65), 'workspace'),                               # forward only: Na is not limited
             (run(d, dec=decide(nat.RULE_SPARC)), 'rule 0'),
             (run(d, dec=decide(nat.RULE_SEGMENTED)), 'rule 1'),
             (run(odd), 'inconsistent'),
             (run(m3), 'power of two')]
    for (rc, msg), word in cases:
        assert rc == -1 and word in msg, (rc, msg, word)
    assert 'amp_bamp_random_trials_run' in run(d)[1]
    del keep


def test_the_other_trial_entries_still_refuse_random_mode():
    import amp_native as nat
    lib = nat.lib()
    cfg = ri.shape_config('16QAM_Nt32')
    cst, d = cfg.constellation(), cfg.dims()
    keep, ptr = _dummy()
    a = nat.AmpBampArgs()
    a.H = a.y = a.xmap = a.xmmse = a.var = a.status = a.ws = ptr
    a.max_iter, a.noise_var, a.ws_bytes = 20, 0.1, 1 << 40          # a workspace size that passes (never read)
    dec = nat.AmpTrialsDecideArgs()
    dec.x = dec.sym = dec.idx = dec.counts = ptr
    dec.ibits_trunc, dec.rule = 4, nat.RULE_RANDOM
    err = lambda: lib.amp_last_error().decode()   # noqa: E731
    a.denoiser = 1
    assert lib.amp_bamp_trials_run(C.byref(d), C.byref(cst), C.byref(a), None, 8, None) == -1 and 'element-wise' in err()
    assert lib.amp_bamp_trials_ch_run(C.byref(d), C.byref(cst), C.byref(a), None, 8, 2, None) == -1
    assert 'element-wise' in err()
    a.denoiser = 0                                                   # the block denoiser with the 'random' rule
    assert lib.amp_bamp_trials_run(C.byref(d), C.byref(cst), C.byref(a), C.byref(dec), 8, None) == -1
    assert "'random' rule has no independent-trial form" in err()
    assert lib.amp_bamp_trials_ch_run(C.byref(d), C.byref(cst), C.byref(a), C.byref(dec), 8, 2, None) == -1
    assert "'random' rule has no independent-trial form" in err()
    del keep


def _cfg(B=1, mode='random'):
    from config import Config
    return Config(16, 2, 32, 1, 1, batch=B, generator_mode=mode, iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


def test_bamp_keyword():
    from bamp import BAMP
    z = [torch.zeros(1, 32, 1, dtype=torch.complex64)] * 3
    x = [torch.zeros(1, 16, 1, dtype=torch.complex64)] * 3
    lab = [np.zeros(2, np.int64)] * 3
    H = torch.zeros(32, 16, dtype=torch.complex64)
    with pytest.raises(ValueError, match='forward_trials'):         # without the keyword: as before
        BAMP(_cfg()).forward_trials(H, z, 10.0, x, lab, lab)
    with pytest.raises(ValueError, match='forward_trials'):
        BAMP(_cfg(), random_trials=False).forward_trials(H, z, 10.0, x, lab, lab)
    with pytest.raises(ValueError, match='random_trials'):          # a batch shares its exit
        BAMP(_cfg(B=2), random_trials=True)
    for mode in ('sparc', 'segmented'):                             # nothing new to combine with
        with pytest.raises(ValueError, match='random_trials'):
            BAMP(_cfg(mode=mode), random_trials=True)
    det = BAMP(_cfg(), random_trials=True)
    assert det.random_trials is True and BAMP(_cfg()).random_trials is False
    d = _cfg().dims()
    lib = __import__('amp_native').lib()
    assert det.trials_workspace_bytes(33, 5) == lib.amp_bamp_random_trials_workspace_bytes(C.byref(d), 5, 33, 5) > 0
    with pytest.raises(ValueError, match='same number'):            # the list checks still come first
        det.forward_trials(H, z, 10.0, x[:2], lab, lab)
    with pytest.raises(ValueError, match='channels for 3 trials'):
        det.forward_trials([H] * 3, z, 10.0, x, lab, lab, per_channel=2)


class FakeRandomAmp:
    """Stands in for BAMP(config, random_trials=True): forward and forward_trials (one channel, or a
    list with per_channel).  Every trial's Loss carries values derived from its own y, x, labels and
    channel, so the totals depend on which message was detected with which channel."""

    def __init__(self, config):
        from loss import Loss
        self.Loss, self.config = Loss, config
        self.L = Loss(config)
        self.log, self.seen = [], []

    def _rates(self, A, y, x, sym, idx):
        v = float(y.abs().sum()) + float(A.abs().sum()) + float(np.sum(idx)) + 0.5 * float(np.sum(sym))
        self.seen.append((y.clone(), x.clone(), np.array(sym), np.array(idx), A.clone()))
        return [v % 1.0] + [v] * 13

    def __call__(self, A, y, SNR, x, sym, idx):
        self.log.append(('single', 1, None))
        self.L.dump()
        self.L.loss = {'T': 0}
        self.L.record(self._rates(A, y, x, sym, idx), 3)
        return self.L

    def forward_trials(self, A, ys, SNR, xs, syms, idxs, per_channel=None):
        E = len(ys)
        assert E == len(xs) == len(syms) == len(idxs)
        if per_channel is None:
            chans = [A] * E
            self.log.append(('trials', E, None))
        else:
            assert isinstance(A, list) and len(A) == -(-E // per_channel)
            chans = [A[e // per_channel] for e in range(E)]
            self.log.append(('channels', E, per_channel))
        out = []
        for e in range(E):
            L = self.Loss(self.config)
            L.record(self._rates(chans[e], ys[e], xs[e], syms[e], idxs[e]), 3)
            out.append(L)
        return out


def _model_cfg():
    from config import Config
    return Config(16, 3, 8, 2, 2, batch=1, generator_mode='random', iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


@pytest.mark.parametrize('res,kw,calls', [
    (4, dict(group_trials=3), [('trials', 3, None), ('single', 1, None)] * 2 + [('trials', 2, None)]),
    (4, dict(group_trials=8, trial_channels=2), [('channels', 8, 4), ('trials', 2, None)]),
    (1, dict(group_trials=8, trial_channels=8), [('channels', 8, 1), ('channels', 2, 1)])])
def test_model_random_mode_order_and_totals(tmp_path, res, kw, calls):
    from model import Model
    cfg = _model_cfg()
    runs = {}
    for key, k in (('base', {}), ('grouped', kw)):
        amp = FakeRandomAmp(cfg)
        m = Model(cfg, 'bamp', path=str(tmp_path / key), amp=amp, seed=11, **k)
        runs[key] = (amp, m.simulate(epochs=10, start=0, final=1.0, step=1, res=res))
    base, grouped = runs['base'][0], runs['grouped'][0]
    assert grouped.log == calls * 2 and base.log == [('single', 1, None)] * 20
    # the reference's random-call order (channel, Data.random, awgn): the same draws, in the same order
    assert len(base.seen) == len(grouped.seen) == 20
    for a, b in zip(base.seen, grouped.seen):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4], b[4])
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
    x0 = base.seen[0][1].reshape(cfg.Lin, cfg.Nt)
    assert ((x0 != 0).sum(dim=1) == cfg.Na).all()                    # Data.random: Na antennas per channel use
    assert json.dumps(runs['base'][1], sort_keys=True) == json.dumps(runs['grouped'][1], sort_keys=True)
    for p in ('0.0.json', '1.0.json'):
        assert open(tmp_path / 'base' / p, 'rb').read() == open(tmp_path / 'grouped' / p, 'rb').read()


def test_model_builds_the_random_trials_detector(tmp_path):
    from bamp import BAMP
    from model import Model
    cfg = _model_cfg()
    m = Model(cfg, 'bamp', path=str(tmp_path), seed=1, group_trials=8, trial_channels=2)
    assert isinstance(m.amp, BAMP) and m.amp.random_trials is True
    assert Model(cfg, 'bamp', path=str(tmp_path), seed=1).amp.random_trials is False       # no grouping asked for
    seg = ri.make_config(16, 2, 8, 2, 2, 'QPSK', mode='segmented')
    assert Model(seg, 'bamp', path=str(tmp_path), seed=1, group_trials=8).amp.random_trials is False
    given = BAMP(cfg)
    assert Model(cfg, 'bamp', path=str(tmp_path), seed=1, amp=given, group_trials=8).amp is given   # used as given
    with pytest.raises(NotImplementedError):                         # Data has no device generator for the mode;
        Model(cfg, 'bamp', path=str(tmp_path), seed=1, rng='device', group_trials=8).data.generate_message()


def test_g20_is_the_reference_in_random_mode():
    assert len(ri.POINTS) == 6
    shapes = {(e['Nt'], e['Na'], e['Nr'], e['Lin'], e['Lh'], e['alphabet']) for e in ri.G20.values()}
    assert shapes == {(16, 2, 7, 2, 3, 'QPSK'), (32, 4, 12, 3, 2, '16QAM'), (6, 3, 5, 3, 1, 'QPSK')}
    for name in ri.POINTS:
        e = ri.G20[name]
        assert e['mode'] == 'random' and e['seed'] == 3 and len(e['trials']) == ri.E_G20 == 40
        assert e['oracle_differs'] == 0
        assert all(set(gio.COUNT_KEYS) <= set(t) and 'T' in t for t in e['trials'])
    for s in shapes:
        lo, hi = (ri.G20[f'{s[5]}_Nt{s[0]}_Na{s[1]}_{lv}'] for lv in ('low', 'high'))
        assert lo['EbN0'] < hi['EbN0']
        assert sum(t['fer'] for t in lo['trials']) > sum(t['fer'] for t in hi['trials'])


@pytest.mark.parametrize('name', ri.POINTS)
def test_oracle_trial_by_trial_matches_g20(name):
    e = ri.G20[name]
    inp = ri.golden_inputs(name)
    cfg = OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=1, alphabet=e['alphabet'],
                       mode='random', iterations=e['iterations'])
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    bad, tdiff = {}, []
    for j, ref in enumerate(e['trials']):
        o = bamp_detect(inp['A'].numpy(), c(inp['y'][j]), inp['SNR'], cfg)
        got = loss_dict(o['xmap'], o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
        if int(o['T']) != int(ref['T']):
            tdiff.append((j, int(o['T']), int(ref['T'])))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert not bad, bad
