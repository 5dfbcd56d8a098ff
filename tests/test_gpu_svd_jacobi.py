"""svd_gram(A, method='jacobi') on the GPU (model.py over amp_eigh_run).

Inputs: stacks 5 x (20 x 48) and 3 x (48 x 128) SPARC channels, 2 x (128 x 64) and 1 x (33 x 80)
Gaussian, a 2-D 64 x 128 input, and 2 x (528 x 2560), the published shape, from
Channel.generate_as_sparc on the host with a fixed numpy seed.

* Shapes, dtypes, descending s; channel g of a stack equals the 2-D call on A[g] bit for bit.
* max|U S Vh - A| / max|A|, max|U^H U - I| and max|Vh Vh^H - I| are each at most max(the eigh path's
  figure on the same input, 2e-6): 2e-6 is a few float32 roundings of a k-term product (the factors
  are rounded to complex64; the float64 restatement gives 6.6e-7 at most).
  max|s - svdvals_float64(A)| <= 4 x 2^-24 s_max.
* A 64 x 64 square channel (cond near 80) with max_cond=1e3 meets the same bars without falling
  back; a matrix with cond 1e6 falls back and reconstructs to 1e-5.
* End to end: Model('vamp', rng='device', synth_trials=True, device_svd=...) at Nt=32 Na=4 Nr=8 Lin=4
  Lh=3, QPSK, segmented, 200 epochs at res = 4 near 8 dB: VER and SER of the two settings differ by at
  most 1e-3 absolute (one flipped section of 3200 is 3e-4), mean T by at most 1.

The measured figures are printed; with AMP_EIGH_ERR_FILE set they are appended to that file.
"""
import functools
import os

import numpy as np
import pytest
import torch

import eigh_ref as er

pytestmark = pytest.mark.gpu
BAR = 2e-6


def _record(line):
    print(line)
    path = os.environ.get('AMP_EIGH_ERR_FILE')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


@functools.lru_cache(maxsize=None)
def stack(name):
    """The named input on the host (complex64 numpy), computed once and never modified."""
    if name == 'sparc20x48':
        A = np.stack([er.sparc_channel(16, 4, 5, 3, 2, 20 + g) for g in range(5)])
    elif name == 'sparc48x128':
        A = np.stack([er.sparc_channel(32, 4, 8, 4, 3, 30 + g, profile='exponential') for g in range(3)])
    elif name == 'gauss128x64':
        A = np.stack([er.gaussian(128, 64, 40 + g) for g in range(2)])
    elif name == 'gauss33x80':
        A = er.gaussian(33, 80, 50)[None]
    elif name == 'gauss64x128_2d':
        A = er.gaussian(64, 128, 60)
    elif name == 'published528x2560':
        A = np.stack([er.sparc_channel(128, 8, 24, 20, 3, 70 + g) for g in range(2)])
    else:
        raise KeyError(name)
    A.setflags(write=False)
    return A


STACKS = ['sparc20x48', 'sparc48x128', 'gauss128x64', 'gauss33x80', 'gauss64x128_2d', 'published528x2560']


@functools.lru_cache(maxsize=None)
def factors(name, method):
    from model import svd_gram
    A = torch.tensor(stack(name), device='cuda:0')
    U, s, Vh = svd_gram(A) if method == 'eigh' else svd_gram(A, method=method)
    torch.cuda.synchronize()
    return A, U, s, Vh


def _np(t):
    return t.detach().cpu().numpy()


def _bars(tag, A, U, s, Vh, Ue, se, Vhe):
    """The accuracy checks of one matrix: jacobi factors against the eigh path's on the same input."""
    fj = er.svd_figures(A, U, s, Vh)
    fe = er.svd_figures(A, Ue, se, Vhe)
    _record(f'svd {tag}: jacobi |USVh-A|/|A| {fj[0]:.3e} |UhU-I| {fj[1]:.3e} |VhVhH-I| {fj[2]:.3e} |s-s64|/s_max '
            f'{fj[3]:.3e}; eigh {fe[0]:.3e} {fe[1]:.3e} {fe[2]:.3e} {fe[3]:.3e}')
    for i, what in enumerate(('reconstruction', 'U orthogonality', 'Vh orthogonality')):
        assert fj[i] <= max(fe[i], BAR), (tag, what, fj[i], fe[i])
    assert fj[3] <= 4 * 2.0 ** -24, (tag, fj[3])


@pytest.mark.parametrize('name', STACKS)
def test_structure_and_accuracy(name):
    A, U, s, Vh = factors(name, 'jacobi')
    _, Ue, se, Vhe = factors(name, 'eigh')
    n, N = A.shape[-2:]
    k = min(n, N)
    lead = tuple(A.shape[:-2])
    assert U.shape == lead + (n, k) and s.shape == lead + (k,) and Vh.shape == lead + (k, N)
    assert U.dtype == torch.complex64 and s.dtype == torch.float32 and Vh.dtype == torch.complex64
    assert U.device == A.device and s.device == A.device and Vh.device == A.device
    assert bool((s[..., :-1] >= s[..., 1:]).all())
    if A.dim() == 2:
        _bars(name, _np(A), _np(U), _np(s), _np(Vh), _np(Ue), _np(se), _np(Vhe))
    else:
        for g in range(A.shape[0]):
            _bars(f'{name}[{g}]', _np(A[g]), _np(U[g]), _np(s[g]), _np(Vh[g]), _np(Ue[g]), _np(se[g]), _np(Vhe[g]))


@pytest.mark.parametrize('name', [n for n in STACKS if not n.endswith('_2d')])
def test_a_stack_equals_its_channels_alone(name):
    from model import svd_gram
    A, U, s, Vh = factors(name, 'jacobi')
    for g in range(A.shape[0]):
        U1, s1, Vh1 = svd_gram(A[g], method='jacobi')
        assert U1.shape == U[g].shape and s1.shape == s[g].shape and Vh1.shape == Vh[g].shape
        assert torch.equal(U1, U[g]) and torch.equal(s1, s[g]) and torch.equal(Vh1, Vh[g]), (name, g)


def test_square_channel_with_a_larger_max_cond(monkeypatch):
    from model import svd_gram
    An = er.gaussian(64, 64, 121)
    sv = np.linalg.svd(An.astype(np.complex128), compute_uv=False)
    cond = sv[0] / sv[-1]
    print('condition number', cond)
    assert 20 < cond < 1e3
    A = torch.tensor(An, device='cuda:0')
    Ue, se, Vhe = torch.linalg.svd(A, full_matrices=False)

    def no_fallback(*a, **kw):
        raise AssertionError('svd_gram fell back to torch.linalg.svd')

    monkeypatch.setattr(torch.linalg, 'svd', no_fallback)
    U, s, Vh = svd_gram(A, max_cond=1e3, method='jacobi')
    monkeypatch.undo()
    # the "eigh path's figure" at this condition number is its fallback's (torch.linalg.svd)
    _bars('square64 cond %.0f' % cond, An, _np(U), _np(s), _np(Vh), _np(Ue), _np(se), _np(Vhe))


def test_ill_conditioned_input_falls_back(monkeypatch):
    from model import svd_gram
    g = torch.Generator().manual_seed(5)
    A = torch.complex(torch.randn(64, 32, generator=g), torch.randn(64, 32, generator=g)) / 128 ** 0.5
    U, s, Vh = torch.linalg.svd(A, full_matrices=False)
    s = s.clone()
    s[-1] = s[0] * 1e-6                               # condition number 1e6
    B = ((U * s.to(U.dtype)) @ Vh).to('cuda:0')
    calls, real = [], torch.linalg.svd

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(torch.linalg, 'svd', spy)
    U2, s2, Vh2 = svd_gram(B, method='jacobi')
    monkeypatch.undo()
    assert len(calls) == 1                            # the max_cond rule sent it to torch.linalg.svd
    R = (U2 * s2.to(U2.dtype)) @ Vh2
    assert float((R - B).abs().max() / B.abs().max()) < 1e-5
    assert float(s2[-1] / s2[0]) < 1e-5


def test_model_sweeps_agree(tmp_path):
    from config import Config
    from model import Model
    out = {}
    for setting in ('eigh', 'jacobi'):
        cfg = Config(32, 4, 8, 4, 3, batch=1, generator_mode='segmented', iterations=20, alphabet='QPSK',
                     channel_profile='uniform', channel_truncation='tail', device='cuda')
        m = Model(cfg, 'vamp', path=str(tmp_path / setting), rng='device', seed=3, group_trials=40, trial_channels=10,
                  synth_trials=True, device_svd=setting)
        out[setting] = m.simulate(epochs=200, start=8.0, final=8.0, step=1, res=4)[0]
    e, j = out['eigh'], out['jacobi']
    _record(f"model 8 dB: eigh VER {e['ver']:.5f} SER {e['ser']:.5f} T {e['T']:.3f}; jacobi VER {j['ver']:.5f} "
            f"SER {j['ser']:.5f} T {j['T']:.3f}")
    assert abs(e['ver'] - j['ver']) <= 1e-3 and abs(e['ser'] - j['ser']) <= 1e-3
    assert abs(e['T'] - j['T']) <= 1
