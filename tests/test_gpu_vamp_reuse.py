"""GPU: operator reuse across forwards on one channel (amp_vamp_detect_count_reuse / amp_vamp_run_reuse).

A `VAMP` that is handed the same U, s, Vh tensor objects again (one `res` block of Model.simulate,
vamp_model.py:55-61) tells the library that its workspace still holds the packed operators and
q0 = Vh r~ of iteration 0: the forward then runs y~ and vamp_persist alone.  The bar is bit
identity with a fresh detector (which always builds) on the same inputs: r, xmmse and var bits, T
and all 13 counters.  An in-place edit, new tensor objects, another gemm or engine make the next
forward build again.

Shapes: Nt=64 Na=4 Nr=128 with B = 48 (three workgroups, the last full) and B = 40 (the last with 8
valid rows: the padded-row fill), Nt=256 Na=8 Nr=512 with B = 32 (two workgroups of the eight-wave
cfg4 instantiation).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [(64, 4, 128, 48), (64, 4, 128, 40), (256, 8, 512, 32)]
CASES = [(s, a) for s in SHAPES for a in ('16QAM', 'QPSK')]
EBN0 = {'16QAM': 10.0, 'QPSK': 6.0}


def _cfg(Nt, Na, Nr, B, alphabet, device='cuda'):
    from config import Config
    return Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=20, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', device=device)


_INPUTS = {}


def _inputs(shape, alphabet, E=4, seed=11):
    """One channel and E epochs of messages + noise from the repository's generators, in the
    reference's call order, at a fixed seed (host tensors; computed once per case and left unchanged)."""
    key = (shape, alphabet, E, seed)
    if key not in _INPUTS:
        from channel import Channel
        from data import Data
        np.random.seed(seed)
        torch.manual_seed(seed)
        c = _cfg(*shape, alphabet, device='cpu')
        ch, da = Channel(c), Data(c)
        _, A = ch.generate_as_sparc()
        U, s, Vh = torch.linalg.svd(A, full_matrices=False)
        SNR = c.snr(EBN0[alphabet])
        eps = []
        for _ in range(E):
            x, sym, idx = da.generate_message()
            eps.append((x, sym, idx, A @ x + ch.awgn(SNR)))
        _INPUTS[key] = ((U, s, Vh), SNR, eps)
    return _INPUTS[key]


def _forward(det, chan, SNR, ep, device):
    """One forward; returns (building prepares, reuse prepares) it made and its results."""
    import amp_native as nat
    from loss import counts_to_vector
    x, sym, idx, y = ep
    b0, r0 = nat.prepare_counts()
    L = det(chan[0], chan[1], chan[2], y.to(device).contiguous(), SNR, x.to(device).contiguous(), sym, idx)
    L.resolve()
    b1, r1 = nat.prepare_counts()
    out = dict(r=torch.view_as_real(det.last.r.squeeze(-1).contiguous()).cpu().numpy().copy(),
               xmmse=torch.view_as_real(det.last.xmmse.squeeze(-1).contiguous()).cpu().numpy().copy(),
               var=det.last.var.squeeze(-1).cpu().numpy().copy(),
               T=np.array([int(L.last_status.T)]), counts=counts_to_vector(L.last_counts))
    return (b1 - b0, r1 - r0), out


def _fresh(cfg, chan, SNR, ep, device, **kw):
    """A new detector's (always building) forward on the same inputs."""
    from vamp import VAMP
    made, out = _forward(VAMP(cfg, **kw), chan, SNR, ep, device)
    assert made == (1, 0), made
    return out


def _diff(got, want):
    """Every differing array and its first differing index (bitwise), r / xmmse / var first."""
    bad = []
    for name in ('r', 'xmmse', 'var', 'T', 'counts'):
        a, b = got[name], want[name]
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1) if a.shape == b.shape else None
        if ne is None:
            bad.append(f'{name}: shape {a.shape} != {b.shape}')
        elif ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            bad.append(f'{name}: first difference at flat index {i} of {a.size} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r})')
    return bad


def _dev(chan, device):
    return tuple(t.to(device).contiguous() for t in chan)


@pytest.mark.parametrize('shape,alphabet', CASES)
def test_same_channel_objects_new_y(device, shape, alphabet):
    """Three forwards of one VAMP on the same channel objects with a new y each: the first builds,
    the next two reuse, and each equals a fresh detector's forward bit for bit."""
    from vamp import VAMP
    chan, SNR, eps = _inputs(shape, alphabet)
    cfg = _cfg(*shape, alphabet)
    dchan = _dev(chan, device)
    det = VAMP(cfg)
    bad = []
    for i, want_made in enumerate([(1, 0), (0, 1), (0, 1)]):
        made, got = _forward(det, dchan, SNR, eps[i], device)
        assert made == want_made, (i, made)
        bad += [f'forward {i}: {m}' for m in _diff(got, _fresh(cfg, dchan, SNR, eps[i], device))]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape,alphabet', [(SHAPES[1], '16QAM'), (SHAPES[2], 'QPSK')])
def test_in_place_edit_rebuilds(device, shape, alphabet):
    """Vh.mul_(-1) bumps Vh's version (and legitimately changes the result): the next forward
    builds and equals a fresh detector's on the edited channel; reuse then resumes."""
    from vamp import VAMP
    chan, SNR, eps = _inputs(shape, alphabet)
    cfg = _cfg(*shape, alphabet)
    U, s, Vh = _dev(chan, device)
    det = VAMP(cfg)
    assert _forward(det, (U, s, Vh), SNR, eps[0], device)[0] == (1, 0)
    assert _forward(det, (U, s, Vh), SNR, eps[1], device)[0] == (0, 1)
    Vh.mul_(-1)
    bad = []
    for i, want_made in ((2, (1, 0)), (3, (0, 1))):
        made, got = _forward(det, (U, s, Vh), SNR, eps[i], device)
        assert made == want_made, (i, made)
        bad += [f'forward {i}: {m}' for m in _diff(got, _fresh(cfg, (U, s, Vh), SNR, eps[i], device))]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape,alphabet', [(SHAPES[0], 'QPSK'), (SHAPES[2], '16QAM')])
def test_new_objects_equal_contents_rebuild(device, shape, alphabet):
    """New tensor objects with the same contents: the forward builds, and the results are equal."""
    from vamp import VAMP
    chan, SNR, eps = _inputs(shape, alphabet)
    cfg = _cfg(*shape, alphabet)
    dchan = _dev(chan, device)
    det = VAMP(cfg)
    assert _forward(det, dchan, SNR, eps[0], device)[0] == (1, 0)
    made, reused = _forward(det, dchan, SNR, eps[1], device)
    assert made == (0, 1)
    made, rebuilt = _forward(det, tuple(t.clone() for t in dchan), SNR, eps[1], device)
    assert made == (1, 0), made
    bad = _diff(rebuilt, reused)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('shape,alphabet', [(SHAPES[1], 'QPSK')])
def test_changed_gemm_or_engine_rebuilds(device, shape, alphabet):
    """Another gemm or engine between forwards: the next forward builds (its operators have
    another packing, or it runs the launch engine, which never reuses)."""
    import amp_native as nat
    from vamp import VAMP
    chan, SNR, eps = _inputs(shape, alphabet)
    cfg = _cfg(*shape, alphabet)
    dchan = _dev(chan, device)
    det = VAMP(cfg)
    assert _forward(det, dchan, SNR, eps[0], device)[0] == (1, 0)
    assert _forward(det, dchan, SNR, eps[1], device)[0] == (0, 1)
    det.gemm = nat.GEMM_F32
    made, got = _forward(det, dchan, SNR, eps[2], device)
    assert made == (1, 0), made
    bad = [f'f32: {m}' for m in _diff(got, _fresh(cfg, dchan, SNR, eps[2], device, gemm=nat.GEMM_F32))]
    det.gemm = nat.GEMM_AUTO
    made, got = _forward(det, dchan, SNR, eps[3], device)
    assert made == (1, 0), made
    bad += [f'back to auto: {m}' for m in _diff(got, _fresh(cfg, dchan, SNR, eps[3], device))]
    assert _forward(det, dchan, SNR, eps[0], device)[0] == (0, 1)
    det.engine = nat.ENGINE_LAUNCHES
    assert _forward(det, dchan, SNR, eps[1], device)[0] == (0, 0)     # no persistent prepare at all
    det.engine = nat.ENGINE_AUTO
    made, got = _forward(det, dchan, SNR, eps[2], device)
    assert made == (1, 0), made
    bad += [f'back from the launch engine: {m}' for m in _diff(got, _fresh(cfg, dchan, SNR, eps[2], device))]
    assert not bad, '\n'.join(bad)


def test_flag_reaches_the_library(device):
    """amp_vamp_run_reuse called directly: reuse = 0 tallies a building prepare, reuse = 1 a reuse
    prepare whose outputs equal the building forward's; on the f32 arithmetic the flag is ignored."""
    import ctypes as C
    import amp_native as nat
    from vamp import VAMP
    shape, alphabet = SHAPES[1], '16QAM'
    chan, SNR, eps = _inputs(shape, alphabet)
    cfg = _cfg(*shape, alphabet)
    U, s, Vh = _dev(chan, device)
    y = eps[0][3].to(device).contiguous()
    lib = nat.lib()
    for gemm, want in ((nat.GEMM_AUTO, (0, 1)), (nat.GEMM_F32, (1, 0))):
        det = VAMP(cfg, gemm=gemm)
        T = det.detect(U, s, Vh, y, SNR)                       # builds
        torch.cuda.synchronize()
        built = (T.buf.r.clone(), T.buf.xmmse.clone(), T.buf.var.clone())
        for t in (T.buf.r, T.buf.xmmse, T.buf.var):
            t.zero_()
        c0 = nat.prepare_counts()
        nat.check(lib.amp_vamp_run_reuse(C.byref(T.dims), C.byref(T.const), C.byref(T.args), 1, T.stream), 'reuse')
        torch.cuda.synchronize()
        c1 = nat.prepare_counts()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == want, (gemm, c0, c1)
        for a, b in zip(built, (T.buf.r, T.buf.xmmse, T.buf.var)):
            assert torch.equal(torch.view_as_real(a) if a.is_complex() else a,
                               torch.view_as_real(b) if b.is_complex() else b), gemm
