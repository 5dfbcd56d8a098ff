"""amp_eigh_run (csrc/amp_eigh.hip) through ctypes against numpy.linalg.eigh in float64 and against
the restatement tests/eigh_ref.py, on the matrices of eigh_ref.matrices():

* Gram matrices of complex Gaussian A of shapes 2 x 2, 3 x 5, 17 x 40, 33 x 80, 64 x 64, 130 x 200,
  257 x 300 (k below one block pair, odd k, k no multiple of a block width, a wide spectrum);
* the 20 x 48 and 48 x 128 SPARC channels' Grams (block-banded: whole rounds rotate nothing);
* the identity at k = 32 and diag{4, 2, 1, 0.5} x 8: sweeps == 1, the input's eigenvalues exactly;
* that diagonal matrix conjugated by a random unitary (degenerate eigenvalues).

Batches of 1, 3 and 7; one batch mixes the identity with a dense matrix, and the identity's outputs
and info must not depend on its neighbour.  Per matrix: w descending, |w - w_ref| <= 64 k 2^-53
w_max, max|E^H E - I| <= tol + 16 k 2^-53, max|G E - E diag(w)| / w_max <= 4 x the restatement's
figure + k 2^-50 (rotation order within a round and summation order differ from the restatement),
converged, sweeps within 2 of the restatement's, G unchanged.  max_sweeps = 2 on {identity, 64 x 64
Gram} reports converged {1, 0}, sweeps {1, 2} and no NaN.

The measured figures are printed; with AMP_EIGH_ERR_FILE set they are appended to that file
(profiles/eigh_err.txt is such a run's record).
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import eigh_ref as er

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53


def _record(line):
    print(line)
    path = os.environ.get('AMP_EIGH_ERR_FILE')
    if path:
        with open(path, 'a') as f:
            f.write(line + '\n')


def run(mats, tol=0.0, max_sweeps=0):
    """amp_eigh_run on a batch of equal-size matrices: (w [b, k], E [b, k, k], info [b, 2], G after)."""
    import amp_native as nat
    lib = nat.lib()
    dev = torch.device('cuda:0')
    G = torch.tensor(np.stack(mats), dtype=torch.complex128, device=dev)
    b, k = G.shape[0], G.shape[1]
    E = torch.full((b, k, k), float('nan'), dtype=torch.complex128, device=dev)
    w = torch.full((b, k), float('nan'), dtype=torch.float64, device=dev)
    info = torch.full((b, 2), -1, dtype=torch.int32, device=dev)
    need = lib.amp_eigh_workspace_bytes(k, b)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    a = nat.AmpEighArgs()
    a.G, a.E, a.w, a.info = G.data_ptr(), E.data_ptr(), w.data_ptr(), info.data_ptr()
    a.workspace, a.workspace_bytes = ws.data_ptr(), need
    a.tol, a.max_sweeps = tol, max_sweeps
    nat.check(lib.amp_eigh_run(C.byref(a), k, b, nat.stream_ptr(dev)), 'amp_eigh_run')
    torch.cuda.synchronize()
    return w.cpu().numpy(), E.cpu().numpy(), info.cpu().numpy(), G.cpu().numpy()


@functools.lru_cache(maxsize=None)
def solved(name, batch):
    """The batch of `batch` copies-in-place of the named matrix (position i holds it scaled by
    2^i, an exact scaling), solved once and shared."""
    G = er.matrices()[name]
    mats = [G * 2.0 ** i for i in range(batch)]
    return mats, run(mats)


def check(name, G, w, E, info, tag):
    k = G.shape[0]
    w_ref = np.linalg.eigvalsh(G)[::-1]
    rw, rE, rsweeps, rconv, rorth, rres = er.restated(name)
    orth, res = er.eigh_figures(G, w, E)
    dw = float(np.abs(w - w_ref).max() / w_ref.max())
    ratio = res / rres if rres > 0 else 0.0
    # positions 1 .. of a batch hold exact scalings of position 0 and are asserted equal to it: one line per batch
    (_record if tag.endswith('[0]') else print)(f'eigh {name} {tag}: k = {k}, sweeps = {int(info[0])} (restatement {rsweeps}), max|w - w_ref| / w_max = '
            f'{dw:.3e}, max|E^H E - I| = {orth:.3e} (restatement {rorth:.3e}), max|G E - E w| / w_max = {res:.3e} '
            f'(restatement {rres:.3e}, ratio {ratio:.2f})')
    assert np.isfinite(w).all() and np.isfinite(E).all()
    assert (w[:-1] >= w[1:]).all()
    assert dw <= 64 * k * EPS
    assert orth <= er.TOL + 16 * k * EPS
    assert res <= 4 * rres + k * 2.0 ** -50
    assert int(info[1]) == 1 and rconv
    assert abs(int(info[0]) - rsweeps) <= 2


@pytest.mark.parametrize('name', sorted(er.matrices()))
@pytest.mark.parametrize('batch', [1, 3, 7])
def test_eigh_against_lapack_and_restatement(name, batch):
    mats, (w, E, info, G_after) = solved(name, batch)
    for i in range(batch):
        assert np.array_equal(G_after[i], mats[i])                           # G is not written
        check(name, mats[i], w[i], E[i], info[i], f'batch {batch}[{i}]')
    # an exact scaling of the input scales w exactly and leaves E and the sweeps alone
    for i in range(1, batch):
        assert np.array_equal(w[i], w[0] * 2.0 ** i) and np.array_equal(E[i], E[0]) and np.array_equal(info[i], info[0])


@pytest.mark.parametrize('name, want', [('identity32', np.ones(32)), ('diag32', er.DIAG)])
def test_diagonal_input_is_returned_exactly(name, want):
    w, E, info, _ = solved(name, 1)[1]
    assert info.tolist() == [[1, 1]]
    assert np.array_equal(w[0], want)
    assert np.array_equal(np.abs(E[0]) != 0, np.abs(E[0]) == 1) and (np.abs(E[0]).sum(0) == 1).all()


def test_a_finished_matrix_does_not_depend_on_its_neighbour():
    eye, dense = er.matrices()['identity32'], er.matrices()['gauss33x80'][:32, :32]
    alone = run([eye])
    w, E, info, _ = run([eye, dense, eye])
    for i in (0, 2):
        assert np.array_equal(w[i], alone[0][0]) and np.array_equal(E[i], alone[1][0])
        assert info[i].tolist() == [1, 1]
    assert info[1, 1] == 1 and info[1, 0] > 1
    # and the dense one equals its own batch of one
    w1, E1, info1, _ = run([dense])
    assert np.array_equal(w[1], w1[0]) and np.array_equal(E[1], E1[0]) and np.array_equal(info[1], info1[0])


def test_non_convergence_is_reported():
    eye64, dense = np.eye(64, dtype=np.complex128), er.matrices()['gauss64x64']
    w, E, info, _ = run([eye64, dense], max_sweeps=2)
    assert info.tolist() == [[1, 1], [2, 0]]
    assert np.isfinite(w).all() and np.isfinite(E).all()
    assert np.array_equal(w[0], np.ones(64))


def test_looser_tolerance_and_sweep_cap_arguments():
    G = er.matrices()['gauss17x40']
    w, E, info, _ = run([G], tol=1e-6)
    w9 = solved('gauss17x40', 1)[1]
    assert info[0, 1] == 1 and info[0, 0] <= w9[2][0, 0]
    orth, _ = er.eigh_figures(G, w[0], E[0])
    assert orth <= 1e-6 + 16 * 17 * EPS
