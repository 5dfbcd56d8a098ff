"""Independent-trial batches on the CPU (no GPU needed).

* g13 (tests/golden/make_g13_trials.py: the reference at batch = 1, 40 trials per channel,
  generator_mode='segmented') is reproduced by the oracle run trial by trial (OracleConfig(B=1)):
  every counting metric of every trial.  T is not compared per trial: at B = 1 the allclose exit
  (vamp.py:185, bamp.py:140) is decided by rounding, and the oracle's BLAS summation order already
  moves it against the reference's.
* the new entry points are declared in include/amp_sparc.h, bound and exported by the library;
* forward_trials rejects B != 1 and generator_mode='random' before touching the device;
* Model(group_trials=...) with a stand-in detector: the reference's call order, chunking by the cap
  and by channel run, totals equal to the per-epoch loop.
"""
import json
import os

import numpy as np
import pytest
import torch

import golden_io as gio
import trials_inputs as ti
from oracle import OracleConfig, bamp_detect, loss_dict, vamp_detect

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('amp_vamp_trials_run', 'amp_vamp_trials_workspace_bytes', 'amp_bamp_trials_run',
               'amp_bamp_trials_workspace_bytes')


@pytest.mark.parametrize('name', ti.POINTS)
def test_oracle_trial_by_trial_matches_g13(name):
    e = ti.G13[name]
    inp = ti.host_inputs(name)
    cfg = OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=1, alphabet=e['alphabet'],
                       mode='segmented', iterations=e['iterations'])
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    bad = {}
    for j, ref in enumerate(e['trials']):
        if e['algo'] == 'vamp':
            o = vamp_detect(inp['U'].numpy(), inp['s'].numpy(), inp['Vh'].numpy(), c(inp['y'][j]), inp['SNR'], cfg)
            xmap = o['r']
        else:
            o = bamp_detect(inp['A'].numpy(), c(inp['y'][j]), inp['SNR'], cfg)
            xmap = o['xmap']
        got = loss_dict(xmap, o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
    assert not bad, bad


def test_trials_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    import ctypes as C
    # x, sym, idx, (ibits_trunc, rule), counts
    assert nat.AmpTrialsDecideArgs.counts.offset == 32 and C.sizeof(nat.AmpTrialsDecideArgs) == 40
    cfg = ti.config_of(ti.POINTS[0])
    d = cfg.dims()
    one = lib.amp_vamp_trials_workspace_bytes(C.byref(d), 32, 20, 1)
    many = lib.amp_vamp_trials_workspace_bytes(C.byref(d), 32, 20, 40)
    assert 0 < one < many
    assert 0 < lib.amp_bamp_trials_workspace_bytes(C.byref(d), 20, 1) < lib.amp_bamp_trials_workspace_bytes(C.byref(d), 20, 40)
    assert lib.amp_vamp_trials_workspace_bytes(C.byref(d), 32, 20, 0) == 0
    d2 = ti.config_of(ti.POINTS[0]).dims(batch=2)       # dims describe ONE trial
    assert lib.amp_vamp_trials_workspace_bytes(C.byref(d2), 32, 20, 4) == 0
    assert lib.amp_bamp_trials_workspace_bytes(C.byref(d2), 20, 4) == 0


def _cfg(B, mode):
    from config import Config
    return Config(16, 2, 32, 1, 1, batch=B, generator_mode=mode, iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


@pytest.mark.parametrize('B,mode', [(2, 'sparc'), (4, 'segmented'), (1, 'random')])
def test_forward_trials_rejects_batches_and_random(B, mode):
    from bamp import BAMP
    from vamp import VAMP
    cfg = _cfg(B, mode)
    z = [torch.zeros(B, 32, 1, dtype=torch.complex64)] * 3
    x = [torch.zeros(B, 16, 1, dtype=torch.complex64)] * 3
    lab = [np.zeros(2 * B, np.int64)] * 3
    U, s, Vh = torch.zeros(32, 16, dtype=torch.complex64), torch.ones(16), torch.zeros(16, 16, dtype=torch.complex64)
    with pytest.raises(ValueError, match='forward_trials'):
        VAMP(cfg).forward_trials(U, s, Vh, z, 10.0, x, lab, lab)
    with pytest.raises(ValueError, match='forward_trials'):
        BAMP(cfg).forward_trials(torch.zeros(32, 16, dtype=torch.complex64), z, 10.0, x, lab, lab)


def test_forward_trials_rejects_mismatched_lists():
    from vamp import VAMP
    cfg = _cfg(1, 'segmented')
    z = [torch.zeros(1, 32, 1, dtype=torch.complex64)] * 3
    with pytest.raises(ValueError, match='same number'):
        VAMP(cfg).forward_trials(None, None, None, z, 10.0, z[:2], z, z)


class FakeTrialsAmp:
    """Stands in for VAMP / BAMP: forward and forward_trials with their signatures; every trial's
    Loss carries values derived from its own y, so totals depend on which trials were detected."""

    def __init__(self, config, vamp=True):
        from loss import Loss
        self.Loss, self.config, self.vamp = Loss, config, vamp
        self.L = Loss(config)
        self.log = []          # ('single' | 'trials', channel id, number of trials)
        self.seen = []         # every detected y, in order

    def _rates(self, y):
        v = float(y.abs().sum())
        return [v % 1.0] + [v] * 13

    def __call__(self, *a):
        ch, y = (a[2], a[3]) if self.vamp else (a[0], a[1])
        self.log.append(('single', id(ch), 1))
        self.seen.append(y.clone())
        self.L.dump()
        self.L.loss = {'T': 0}
        self.L.record(self._rates(y), 3)
        return self.L

    def forward_trials(self, *a):
        ch, ys = (a[2], a[3]) if self.vamp else (a[0], a[1])
        assert len(ys) == len(a[-1]) == len(a[-2]) == len(a[-3])
        self.log.append(('trials', id(ch), len(ys)))
        out = []
        for y in ys:
            self.seen.append(y.clone())
            L = self.Loss(self.config)
            L.record(self._rates(y), 3)
            out.append(L)
        return out


@pytest.mark.parametrize('det', ['vamp', 'bamp'])
def test_model_group_trials_order_chunks_and_totals(tmp_path, det):
    from model import Model
    cfg = _cfg(1, 'segmented')
    runs = {}
    for gt in (0, 3):
        amp = FakeTrialsAmp(cfg, vamp=(det == 'vamp'))
        m = Model(cfg, det, path=str(tmp_path / f'g{gt}'), amp=amp, seed=11, group_trials=gt)
        res = m.simulate(epochs=10, start=0, final=1.0, step=1, res=4)
        runs[gt] = (amp, res)
    base, grouped = runs[0][0], runs[3][0]
    # per SNR point, epochs 0-3 | 4-7 | 8-9 share a channel: runs of 4, 4, 2 in chunks of at most 3
    per_point = [('trials', 3), ('single', 1), ('trials', 3), ('single', 1), ('trials', 2)]
    assert [(k, n) for k, _, n in grouped.log] == per_point * 2
    ids = [c for _, c, _ in grouped.log]
    assert ids[0] == ids[1] and ids[2] == ids[3] and len({ids[0], ids[2], ids[4]}) == 3    # chunk by channel run
    assert [k for k, _, _ in base.log] == ['single'] * 20
    # the reference's call order: the same inputs, in the same order, as the per-epoch loop
    assert len(base.seen) == len(grouped.seen) == 20
    for a, b in zip(base.seen, grouped.seen):
        assert torch.equal(a, b)
    assert json.dumps(runs[0][1], sort_keys=True) == json.dumps(runs[3][1], sort_keys=True)
    for p in ('0.0.json', '1.0.json'):
        assert open(tmp_path / 'g0' / p).read() == open(tmp_path / 'g3' / p).read()


def test_model_group_trials_rejects_batches_and_scamp(tmp_path):
    from model import Model
    cfg = _cfg(1, 'segmented')
    with pytest.raises(ValueError, match='group_trials'):
        Model(_cfg(2, 'sparc'), 'vamp', path=str(tmp_path), amp=FakeTrialsAmp(_cfg(2, 'sparc')), group_trials=4)
    with pytest.raises(ValueError, match='group_trials'):
        Model(cfg, 'scamp', path=str(tmp_path), amp=FakeTrialsAmp(cfg), group_trials=4)


def test_model_group_trials_res1_single_calls(tmp_path):
    from model import Model
    cfg = _cfg(1, 'segmented')
    amp = FakeTrialsAmp(cfg)
    Model(cfg, 'vamp', path=str(tmp_path), amp=amp, seed=1, group_trials=8).simulate(epochs=3, start=0, final=0.0,
                                                                                     step=1, res=1)
    assert [k for k, _, _ in amp.log] == ['single'] * 3
