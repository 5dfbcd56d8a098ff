"""Float64 numpy restatement of csrc/amp_eigh.hip (amp_eigh_run): the cyclic one-sided (Hestenes)
Jacobi iteration on the columns of a Hermitian positive semidefinite matrix, with the kernel's pair
criterion, tolerance, padding (columns that do not exist are never rotated), norms and ordering, in
the kernel's own cyclic order (block round-robin; the disjoint pairs of one inner round are rotated
at once here, which is what the workgroups do side by side).  Rotation order inside an inner round
and summation order differ from the kernel's; nothing else does.

Also the matrices the eigensolver's tests share, and the error figures of a thin SVD.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'amp-sparc-spatialmodulation_amd'))

TOL = 1e-9
MAX_SWEEPS = 24
RANGE = 2.0 ** -40          # eigenvectors are defined above this share of the largest eigenvalue


def block_width(k):
    """amp_eigh.hip eigh_block_width: 8 columns per block at every k."""
    return 8


def _circle(g, r, m):
    """Pair g of round r of the round-robin over m + 1 items (m odd): item m is fixed."""
    if g == 0:
        return (r, m)
    a, b = (r + g) % m, (r - g + m) % m
    return (a, b) if a < b else (b, a)


def sweep_pairs(k, bw=None):
    """The inner rounds of one sweep: lists of disjoint column pairs (p, q), in launch order."""
    bw = bw or block_width(k)
    nb = -(-k // bw)
    nbe = nb + (nb & 1)
    rounds = []
    for t in range(bw - 1):                          # round W: every pair inside a block
        pairs = []
        for blk in range(nb):
            c0 = blk * bw
            for w in range(bw // 2):
                p, q = _circle(w, t, bw - 1)
                if c0 + q < k:
                    pairs.append((c0 + p, c0 + q))
        if pairs:
            rounds.append(pairs)
    if nb > 1:
        for r in range(nbe - 1):                     # block pairs (I, J) of the round-robin
            bp = [_circle(g, r, nbe - 1) for g in range(nbe // 2)]
            bp = [(i, j) for i, j in bp if j < nb]
            for t in range(bw):
                pairs = [(i * bw + w, j * bw + (w + t) % bw) for i, j in bp for w in range(bw)
                         if j * bw + (w + t) % bw < k]
                if pairs:
                    rounds.append(pairs)
    return rounds


def jacobi_eigh(G, tol=TOL, max_sweeps=MAX_SWEEPS, bw=None):
    """(w descending, E with unit eigenvector columns, sweeps run, converged) of Hermitian PSD G."""
    G = np.asarray(G, dtype=np.complex128)
    k = G.shape[0]
    X = G.conj().copy()                              # row c = column c of G
    rounds = [(np.array([p for p, _ in pr]), np.array([q for _, q in pr])) for pr in sweep_pairs(k, bw)]
    sweeps, converged = max_sweeps, False
    for s in range(max_sweeps):
        rotated = 0
        for P, Q in rounds:
            xp, xq = X[P], X[Q]
            a = (xp.real ** 2 + xp.imag ** 2).sum(1)
            b = (xq.real ** 2 + xq.imag ** 2).sum(1)
            c = (xp.conj() * xq).sum(1)
            cabs = np.abs(c)
            go = cabs > tol * np.sqrt(a * b)
            if not go.any():
                continue
            rotated += int(go.sum())
            P, Q, xp, xq, a, b, c, cabs = P[go], Q[go], xp[go], xq[go], a[go], b[go], c[go], cabs[go]
            zeta = (b - a) / (2.0 * cabs)
            t = np.copysign(1.0, zeta) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            cs = 1.0 / np.sqrt(1.0 + t * t)
            sp = (cs * t * (c / cabs))[:, None]
            cs = cs[:, None]
            X[P] = cs * xp - sp.conj() * xq
            X[Q] = sp * xp + cs * xq
        if rotated == 0:
            sweeps, converged = s + 1, True
            break
    nrm = np.sqrt((X.real ** 2 + X.imag ** 2).sum(1))
    order = np.lexsort((np.arange(k), -nrm))         # descending, ties by column index
    w = nrm[order]
    inv = np.where(w > 0, 1.0 / np.where(w > 0, w, 1.0), 0.0)
    E = (X[order] * inv[:, None]).T.copy()
    if not (w[-1] > w[0] * RANGE):
        converged = False
    return w, E, sweeps, converged


# ---- error figures ----

def eigh_figures(G, w, E):
    """(max|E^H E - I|, max|G E - E diag(w)| / w_max) in float64."""
    G, E, w = np.asarray(G, np.complex128), np.asarray(E, np.complex128), np.asarray(w, np.float64)
    k = G.shape[0]
    return (float(np.abs(E.conj().T @ E - np.eye(k)).max()),
            float(np.abs(G @ E - E * w[None, :]).max() / w.max()))


def svd_figures(A, U, s, Vh):
    """(max|U S Vh - A| / max|A|, max|U^H U - I|, max|Vh Vh^H - I|, max|s - s64| / s_max): the
    factors as given (complex64 / float32 from svd_gram), the arithmetic here in float64."""
    A, U, Vh = np.asarray(A, np.complex128), np.asarray(U, np.complex128), np.asarray(Vh, np.complex128)
    s = np.asarray(s, np.float64)
    k = s.shape[0]
    s64 = np.linalg.svd(A, compute_uv=False)
    return (float(np.abs((U * s[None, :]) @ Vh - A).max() / np.abs(A).max()),
            float(np.abs(U.conj().T @ U - np.eye(k)).max()),
            float(np.abs(Vh @ Vh.conj().T - np.eye(k)).max()),
            float(np.abs(s - s64).max() / s64.max()))


# ---- the matrices the tests share ----

def gaussian(n, N, seed):
    r = np.random.RandomState(seed)
    return ((r.normal(size=(n, N)) + 1j * r.normal(size=(n, N))) / np.sqrt(2 * max(n, N))).astype(np.complex64)


def gram(A):
    """The smaller Gram matrix of A in complex128, made exactly Hermitian."""
    A = np.asarray(A, np.complex128)
    G = A.conj().T @ A if A.shape[0] >= A.shape[1] else A @ A.conj().T
    return (G + G.conj().T) / 2


def sparc_channel(Nt, Na, Nr, Lin, Lh, seed, profile='uniform', truncation='tail'):
    """Channel.generate_as_sparc on the host with a fixed numpy seed: complex64 [Nr Lout, Nt Lin]."""
    from channel import Channel
    from config import Config
    cfg = Config(Nt, Na, Nr, Lin, Lh, batch=1, generator_mode='segmented', alphabet='QPSK', channel_profile=profile,
                 channel_truncation=truncation, device='cpu')
    state = np.random.get_state()
    np.random.seed(seed)
    try:
        _, A = Channel(cfg).generate_as_sparc()
    finally:
        np.random.set_state(state)
    return A.numpy().astype(np.complex64)


GAUSS_SHAPES = [(2, 2), (3, 5), (17, 40), (33, 80), (64, 64), (130, 200), (257, 300)]
DIAG = np.repeat([4.0, 2.0, 1.0, 0.5], 8)


def unitary(k, seed):
    r = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(r.normal(size=(k, k)) + 1j * r.normal(size=(k, k)))
    return Q


_CACHE = {}


def matrices():
    """name -> Hermitian PSD complex128 matrix, computed once and shared (do not write to them)."""
    if not _CACHE:
        for i, (n, N) in enumerate(GAUSS_SHAPES):
            _CACHE[f'gauss{n}x{N}'] = gram(gaussian(n, N, 100 + i))
        _CACHE['sparc20x48'] = gram(sparc_channel(16, 4, 5, 3, 2, 7))
        _CACHE['sparc48x128'] = gram(sparc_channel(32, 4, 8, 4, 3, 8, profile='exponential'))
        _CACHE['identity32'] = np.eye(32, dtype=np.complex128)
        _CACHE['diag32'] = np.diag(DIAG).astype(np.complex128)
        Q = unitary(32, 9)
        D = (Q * DIAG[None, :]) @ Q.conj().T
        _CACHE['degenerate32'] = (D + D.conj().T) / 2
        for v in _CACHE.values():
            v.setflags(write=False)
    return _CACHE


_REF = {}


def restated(name):
    """(w, E, sweeps, converged, orthogonality, residual) of the restatement on matrices()[name], once."""
    if name not in _REF:
        G = matrices()[name]
        w, E, sweeps, conv = jacobi_eigh(G)
        _REF[name] = (w, E, sweeps, conv) + eigh_figures(G, w, E)
    return _REF[name]
