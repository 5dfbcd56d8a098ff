"""SCAMP independent-trial batches on the CPU (no GPU needed).

* g14 (tests/golden/make_g14_scamp_trials.py: the reference's SCAMP at batch = 1, 40 trials per
  channel, generator_mode='segmented') is reproduced by the oracle's scamp_detect run trial by
  trial (OracleConfig(B=1)): every counting metric of every trial, at all three points.  T is not
  compared per trial: at B = 1 the allclose(psi) exit (scamp.py:105) is decided by rounding, and the
  oracle's BLAS summation order already moves it against the reference's.
* amp_scamp_trials_run / amp_scamp_trials_workspace_bytes are declared in include/amp_sparc.h,
  bound and exported by the library; the workspace grows with the trials and is 0 for no trials or
  dims that describe a batch;
* amp_scamp_trials_run answers AMP_E_ARG for a batch, no trials, the persistent engine, split
  precision GEMMs and a short workspace before it reads a buffer;
* SCAMP.forward_trials rejects B != 1 and generator_mode='random' before touching the device.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_io as gio
import scamp_trials_inputs as si
from oracle import OracleConfig, loss_dict, scamp_detect

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ('amp_scamp_trials_run', 'amp_scamp_trials_workspace_bytes')


def test_g14_points_have_ragged_exits_of_both_parities():
    assert si.POINTS == ['scamp_OOK_Nt128', 'scamp_OOK_Nt16', 'scamp_QPSK_Nt32']
    for name in si.POINTS:
        Ts = [int(t['T']) for t in si.G14[name]['trials']]
        assert len(Ts) == si.E_G14 and len(set(Ts)) >= 5, (name, Ts)
        assert any(t % 2 for t in Ts) and any(t % 2 == 0 for t in Ts), (name, Ts)


@pytest.mark.parametrize('name', si.POINTS)
def test_oracle_trial_by_trial_matches_g14(name):
    e = si.G14[name]
    inp = si.host_inputs(name)
    cfg = OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=1, alphabet=e['alphabet'],
                       mode='segmented', iterations=e['iterations'])
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    W = inp['W'].numpy().reshape(cfg.Lout, cfg.Lin)
    bad, tdiff = {}, []
    for j, ref in enumerate(e['trials']):
        o = scamp_detect(W, inp['A'].numpy(), c(inp['y'][j]), inp['SNR'], cfg)
        got = loss_dict(o['xmap'], o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
        if int(o['T']) != int(ref['T']):
            tdiff.append((j, int(o['T']), int(ref['T'])))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert not bad, bad


def test_scamp_trials_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in NEW_SYMBOLS:
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    for name in si.POINTS:
        d = si.config_of(name).dims()
        one = lib.amp_scamp_trials_workspace_bytes(C.byref(d), 20, 1)
        many = lib.amp_scamp_trials_workspace_bytes(C.byref(d), 20, 40)
        assert 0 < one < many, (name, one, many)
        assert lib.amp_scamp_trials_workspace_bytes(C.byref(d), 20, 0) == 0
        d2 = si.config_of(name).dims(batch=2)              # dims describe ONE trial
        assert lib.amp_scamp_trials_workspace_bytes(C.byref(d2), 20, 4) == 0


def _cfg(B, mode):
    from config import Config
    return Config(16, 2, 32, 1, 1, batch=B, generator_mode=mode, iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


@pytest.mark.parametrize('B,mode', [(2, 'sparc'), (2, 'segmented'), (1, 'random')])
def test_scamp_forward_trials_rejects_batches_and_random(B, mode):
    from scamp import SCAMP
    cfg = _cfg(B, mode)
    z = [torch.zeros(B, 32, 1, dtype=torch.complex64)] * 3
    x = [torch.zeros(B, 16, 1, dtype=torch.complex64)] * 3
    lab = [np.zeros(2 * B, np.int64)] * 3
    with pytest.raises(ValueError, match='forward_trials'):
        SCAMP(cfg).forward_trials(torch.ones(1, 1), torch.zeros(32, 16, dtype=torch.complex64), z, 10.0, x, lab, lab)


def test_scamp_trials_run_refuses_before_touching_the_device():
    """AMP_E_ARG (-1) for dims that describe a batch, no trials, the persistent engine, split
    precision GEMMs and the shapes amp_scamp_run refuses: every check precedes the first use of a
    pointer, so the buffers here are never read."""
    import amp_native as nat
    lib = nat.lib()
    name = 'scamp_OOK_Nt16'
    cfg = si.config_of(name)
    cst = cfg.constellation()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value

    def run(d, trials=4, engine=nat.ENGINE_LAUNCHES, gemm=nat.GEMM_AUTO):
        a = nat.AmpScampArgs()
        a.W = a.A = a.y = a.xmap = a.xmmse = a.psi = a.status = a.ws = ptr
        a.ws_bytes = 0                                   # a valid call would stop here, before any launch
        a.max_iter, a.engine, a.gemm, a.noise_var = 20, engine, gemm, 0.1
        return lib.amp_scamp_trials_run(C.byref(d), C.byref(cst), C.byref(a), None, trials, None)

    d = cfg.dims()
    assert run(cfg.dims(batch=2)) == -1 and 'ONE trial' in lib.amp_last_error().decode()
    assert run(d, trials=0) == -1 and 'trials = 0' in lib.amp_last_error().decode()
    assert run(d, engine=nat.ENGINE_PERSISTENT) == -1 and 'launch engine only' in lib.amp_last_error().decode()
    for g in (nat.GEMM_X3, nat.GEMM_H2):
        assert run(d, gemm=g) == -1 and 'f32 GEMMs only' in lib.amp_last_error().decode()
    assert run(d) == -1 and 'workspace' in lib.amp_last_error().decode()
    wide = si.config_of(name).dims()
    wide.Lin = 65                                        # more coupling blocks than amp_scamp_run takes
    assert lib.amp_scamp_trials_workspace_bytes(C.byref(wide), 20, 4) == 0
