"""The batched Jacobi eigensolver (csrc/amp_eigh.hip, svd_gram(method='jacobi'),
Model(device_svd='jacobi')), the parts that need no GPU.

* tests/eigh_ref.py's restatement against numpy.linalg.eigh on every matrix the GPU tests use: it
  converges within 24 sweeps, max|E^H E - I| <= tol + 16 k 2^-53, |w - w_ref| <= 64 k 2^-53 w_max.
* The library exports, and the binding declares, amp_eigh_workspace_bytes / amp_eigh_run; every
  refusal answers AMP_E_ARG with a message before anything is launched, and the workspace query
  returns 0 for refused sizes.
* svd_gram raises on an unknown method and on 'jacobi' with a CPU tensor (there is no CPU fallback).
* Model(device_svd='jacobi') raises with rng='host' and with a BAMP detector; with a stand-in
  svd_gram and detector it passes method='jacobi' from _group_synth, and with the default
  device_svd it passes no keyword.
"""
import os

import numpy as np
import pytest
import torch

import eigh_ref as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -53


@pytest.mark.parametrize('name', sorted(er.matrices()))
def test_restatement_against_lapack(name):
    G = er.matrices()[name]
    k = G.shape[0]
    w, E, sweeps, conv, orth, resid = er.restated(name)
    w_ref = np.linalg.eigvalsh(G)[::-1]
    dw = float(np.abs(w - w_ref).max())
    print(f'{name}: k = {k}, sweeps = {sweeps}, max|E^H E - I| = {orth:.3e}, max|G E - E w| / w_max = {resid:.3e}, '
          f'max|w - w_ref| / w_max = {dw / w_ref.max():.3e}')
    assert conv
    assert sweeps <= er.MAX_SWEEPS
    assert (w[:-1] >= w[1:]).all()
    assert orth <= er.TOL + 16 * k * EPS
    assert dw <= 64 * k * EPS * w_ref.max()


def test_restatement_exact_on_diagonal_input():
    for name, want in (('identity32', np.ones(32)), ('diag32', er.DIAG)):
        w, E, sweeps, conv = er.restated(name)[:4]
        assert sweeps == 1 and conv
        assert np.array_equal(w, want)


def test_restatement_sweep_covers_every_pair_once():
    for k in (2, 3, 17, 33, 64, 130, 257, 528):
        seen = set()
        for pairs in er.sweep_pairs(k):
            cols = [c for pq in pairs for c in pq]
            assert len(cols) == len(set(cols))              # the pairs of an inner round are disjoint
            for p, q in pairs:
                assert p < q < k and (p, q) not in seen
                seen.add((p, q))
        assert len(seen) == k * (k - 1) // 2


def test_restatement_reports_non_convergence():
    w, E, sweeps, conv = er.jacobi_eigh(er.matrices()['gauss64x64'], max_sweeps=2)
    assert sweeps == 2 and not conv and np.isfinite(w).all() and np.isfinite(E).all()


def test_eigh_abi_declared_bound_and_exported():
    import amp_native as nat
    header = open(os.path.join(REPO, 'include', 'amp_sparc.h')).read()
    lib = nat.lib()
    for name in ('amp_eigh_workspace_bytes', 'amp_eigh_run'):
        assert f' {name}(' in header, name
        assert name in nat.SIGNATURES, name
        assert hasattr(lib, name), name
    assert 'typedef struct amp_eigh_args' in header
    assert f'#define AMP_EIGH_MAX_K {nat.EIGH_MAX_K}' in header and nat.EIGH_MAX_K >= 640
    assert f'#define AMP_EIGH_MAX_SWEEPS {nat.EIGH_MAX_SWEEPS}' in header and nat.EIGH_MAX_SWEEPS == 24


def test_eigh_refuses_bad_arguments():
    """AMP_E_ARG with a message, before anything is launched (no device is touched here: the pointers
    below are never read)."""
    import ctypes as C
    import amp_native as nat
    lib = nat.lib()

    def args(**kw):
        a = nat.AmpEighArgs()
        for f in ('G', 'E', 'w', 'info', 'workspace'):
            setattr(a, f, 256)
        a.workspace_bytes = 1 << 40
        for f, v in kw.items():
            setattr(a, f, v)
        return a

    def run(a, k, batch):
        rc = lib.amp_eigh_run(C.byref(a) if a is not None else None, k, batch, None)
        return rc, lib.amp_last_error().decode()

    need = lib.amp_eigh_workspace_bytes(48, 3)
    assert need >= 3 * 48 * 48 * 16
    for (rc, msg), word in [(run(args(), 0, 1), 'k ='),
                            (run(args(), nat.EIGH_MAX_K + 1, 1), 'k ='),
                            (run(args(), 48, 0), 'batch'),
                            (run(args(), 48, 65536), 'batch'),
                            (run(None, 48, 1), 'null'),
                            (run(args(G=None), 48, 1), 'null pointer'),
                            (run(args(E=None), 48, 1), 'null pointer'),
                            (run(args(w=None), 48, 1), 'null pointer'),
                            (run(args(info=None), 48, 1), 'null pointer'),
                            (run(args(workspace=None), 48, 1), 'null pointer'),
                            (run(args(workspace_bytes=need - 1), 48, 3), 'workspace'),
                            (run(args(tol=-1e-9), 48, 1), 'tol'),
                            (run(args(max_sweeps=-1), 48, 1), 'max_sweeps')]:
        assert rc == -1 and word in msg, (rc, msg, word)
    for k, batch in ((0, 1), (-3, 1), (nat.EIGH_MAX_K + 1, 1), (48, 0), (48, 65536)):
        assert lib.amp_eigh_workspace_bytes(k, batch) == 0
    assert lib.amp_eigh_workspace_bytes(nat.EIGH_MAX_K, 65535) > 0


def test_svd_gram_method_refusals():
    from model import svd_gram
    A = torch.tensor(er.gaussian(20, 48, 1))
    with pytest.raises(ValueError, match='method'):
        svd_gram(A, method='qr')
    with pytest.raises(ValueError, match='no CPU fallback'):
        svd_gram(A, method='jacobi')
    U, s, Vh = svd_gram(A)                                      # the default is today's path
    U2, s2, Vh2 = svd_gram(A, method='eigh')
    assert torch.equal(U, U2) and torch.equal(s, s2) and torch.equal(Vh, Vh2)


# ---- Model(device_svd=...) with stand-ins ----

def _cfg():
    from config import Config
    return Config(16, 2, 7, 4, 3, batch=1, generator_mode='segmented', iterations=5, alphabet='QPSK',
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


class FakeVamp:
    trials_per_channel = True

    def __init__(self, cfg):
        from loss import Loss
        self.Loss, self.config = Loss, cfg

    def forward_trials(self, U, s, Vh, ys, SNR, xs, syms, idxs, per_channel=None):
        out = []
        for _ in range(len(ys)):
            L = self.Loss(self.config)
            L.record([0.5] + [0.0] * 13, 3)
            out.append(L)
        return out


class FakeSynth:
    """TrialSynth's two calls on the host."""

    def __init__(self, cfg):
        self.d = cfg.dims(batch=1)

    def channels(self, G, channel0):
        d = self.d
        A = torch.ones(G, d.n, d.N, dtype=torch.complex64)
        return torch.ones(d.Lout, d.Lin), A, A.transpose(1, 2).contiguous()

    def trials(self, At, E, per_channel, SNR, trial0, band=True, want_noise=False):
        d = self.d
        return (torch.zeros(E, d.N, dtype=torch.complex64), torch.zeros(E, d.L, dtype=torch.int64),
                torch.zeros(E, d.L, dtype=torch.int64), torch.zeros(E, d.n, dtype=torch.complex64))


def test_model_device_svd_refusals(tmp_path):
    from model import Model
    cfg = _cfg()
    with pytest.raises(ValueError, match='device_svd'):
        Model(cfg, 'vamp', path=str(tmp_path), amp=FakeVamp(cfg), seed=3, rng='host', device_svd='jacobi')
    with pytest.raises(ValueError, match='device_svd'):
        Model(cfg, 'bamp', path=str(tmp_path), amp=FakeVamp(cfg), seed=3, rng='device', device_svd='jacobi')
    with pytest.raises(ValueError, match='device_svd'):
        Model(cfg, 'vamp', path=str(tmp_path), amp=FakeVamp(cfg), seed=3, rng='device', device_svd='qr')
    assert Model(cfg, 'vamp', path=str(tmp_path), amp=FakeVamp(cfg), seed=3, rng='device').device_svd == 'eigh'


@pytest.mark.parametrize('setting', ['eigh', 'jacobi'])
def test_model_passes_the_method_from_group_synth(tmp_path, monkeypatch, setting):
    import model
    cfg = _cfg()
    calls = []

    def fake_svd(A, *args, **kw):
        calls.append((tuple(A.shape), args, dict(kw)))
        G, n, N = A.shape
        k = min(n, N)
        return (torch.zeros(G, n, k, dtype=A.dtype), torch.ones(G, k), torch.zeros(G, k, N, dtype=A.dtype))

    monkeypatch.setattr(model, 'svd_gram', fake_svd)
    kw = {} if setting == 'eigh' else {'device_svd': setting}
    m = model.Model(cfg, 'vamp', path=str(tmp_path), amp=FakeVamp(cfg), seed=3, rng='device', group_trials=8,
                    trial_channels=4, synth_trials=True, **kw)
    m.synth = FakeSynth(cfg)
    m.simulate(epochs=8, start=0, final=0.0, step=1, res=2)
    assert calls and all(c[0][1:] == (cfg.Nr * cfg.Lout, cfg.Nt * cfg.Lin) for c in calls)
    want = {} if setting == 'eigh' else {'method': 'jacobi'}
    assert all(c[1] == () and c[2] == want for c in calls), calls
