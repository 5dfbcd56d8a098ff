"""GPU: the narrowed candidate scan of the fused epilogue's section decision (amp_decide.h
decide_section NARROW, used by vamp_persist at one workgroup per CU) decides what the scan over
every position decides, and both decide what numpy decides.

amp_decide_debug_sections runs the epilogue's decision (four lanes per section, rows in LDS, 16
sections per wave step, eight waves and 16 rows per workgroup) on rows built here, so a wave can be
handed ties, near-ties and non-finite sections a forward would never produce on demand.

For every section:
* the expected decision is np.argmax over the float64 values Re(x_m conj(a_k)) formed by numpy's
  complex multiply (the oracle's rule, oracle/amp_oracle.py map_decision), computed here;
* amp_map_decide_count's `decisions` (every (m, k) in float64, no prefilter) equals it;
* the narrowed and the full scan both equal it, and return the same mismatch flag and the same bits
  of the squared-error sum.

Each built property (which sections have one candidate position per lane, which force the wave
back to the full scan) is checked on the CPU with a float32 restatement of the prefilter before
anything runs.  A wave decides sections [16 w, 16 w + 16) of its workgroup's 16 rows: with L = 8
sections per row that is rows 2 w and 2 w + 1.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

F32 = np.float32

# (alphabet, Nt, Na, B): M = 32 with the reference's 16-QAM table (two workgroups, the second with
# 8 rows), M = 32 QPSK, M = 64 16-QAM
SHAPES = [('16QAM', 256, 8, 24), ('QPSK', 256, 8, 16), ('16QAM', 256, 4, 16)]
IDS = ['16QAM-M32', 'QPSK-M32', '16QAM-M64']


def _config(alphabet, Nt, Na, B):
    from config import Config
    return Config(Nt, Na, 2 * Nt, 1, 1, batch=B, generator_mode='sparc', iterations=1, alphabet=alphabet,
                  channel_profile='uniform', channel_truncation='tail', device='cuda')


def _prefilter(xs, sym):
    """The float32 prefilter of one section xs [M] c64 (amp_decide.h): (v32 [M, K], thr)."""
    re32, im32 = sym.real.astype(F32), sym.imag.astype(F32)
    xr, xi = xs.real.astype(F32), xs.imag.astype(F32)
    with np.errstate(all='ignore'):
        p = (xi[:, None].astype(np.float64) * im32[None, :]).astype(F32)           # xv.y * im32[k]
        v = (xr[:, None].astype(np.float64) * re32[None, :] + p).astype(F32)       # fmaf(xv.x, re32[k], p)
        amax = F32(max(np.abs(sym.real).max(), np.abs(sym.imag).max()) * (1.0 + 1e-6))
        s = (np.abs(xr) + np.abs(xi)).max().astype(F32)
        thr = F32(np.nanmax(v)) - F32(2) * (F32(F32(s * amax) * F32(2.0 ** -20)) + F32(2.0 ** -126))
    return v, F32(thr)


def _section_narrow(xs, sym, margin=4.0):
    """True: every lane (positions g, g + 4, ...) has at most one position whose maximum over k
    reaches thr, with `margin` float32 ulps of thr to spare (the restatement above rounds the fused
    multiply-add twice); False: some lane has two such positions, or the section is non-finite."""
    if not np.isfinite(xs.view(F32)).all():
        return False
    v, thr = _prefilter(xs, sym)
    pm = v.max(axis=1)
    tol = margin * np.spacing(np.abs(thr))
    narrow = True
    for g in range(4):
        second = np.sort(pm[g::4])[-2]
        assert abs(float(second) - float(thr)) > tol, 'a built section sits on the threshold'
        narrow &= bool(second < thr)
    return narrow


def _build(alphabet, Nt, Na, B, seed):
    """Rows (xmap, xmmse, x) [B, N] c64, the constellation, and {name: (row, section)} of the built
    sections."""
    cfg = _config(alphabet, Nt, Na, B)
    sym = np.asarray(cfg.symbols, np.complex128)
    sym32 = sym.astype(np.complex64)
    K, M, L, N = len(sym), Nt // Na, Na, Nt
    rng = np.random.default_rng(seed)
    noise = lambda *s: (0.05 * (rng.standard_normal(s) + 1j * rng.standard_normal(s))).astype(np.complex64)  # noqa: E731
    xmap = noise(B, L, M)
    x = np.zeros((B, L, M), np.complex64)
    pos = rng.integers(0, M, (B, L))
    kk = rng.integers(0, K, (B, L))
    bb, ll = np.meshgrid(np.arange(B), np.arange(L), indexing='ij')
    x[bb, ll, pos] = sym32[kk]
    xmap += x                                     # ordinary rows: the sent point plus noise
    xmap[B - 2:] = (rng.standard_normal((2, L, M)) + 1j * rng.standard_normal((2, L, M))).astype(np.complex64)  # dense rows
    xmmse = (x + noise(B, L, M)).astype(np.complex64)
    kmax = int(np.argmax(sym.real))               # a point of largest real part
    special = {}

    def put(name, row, sec, entries):
        xmap[row, sec] = noise(M)
        for m, val in entries.items():
            xmap[row, sec, m] = val
        special[name] = (row, sec)

    # two equal maxima at positions 5 and 9 (one lane): the full scan, the lower m wins
    put('tie_same_lane', 2, 0, {5: sym32[kmax], 9: sym32[kmax]})
    # two equal maxima at positions 6 and 7 (two lanes): one candidate position per lane
    put('tie_two_lanes', 4, 1, {7: sym32[kmax], 6: sym32[kmax]})
    xmap[6, 3] = 0                                # everything ties: index 0
    special['all_zero'] = (6, 3)
    # two positions of one lane whose float32 maxima differ by one ulp (real inputs: the value
    # a * re is rounded once, so the restatement is exact)
    c = sym.real.astype(F32).max()
    a = F32(1.0)
    while True:
        a2 = np.nextafter(a, F32(2))
        lo, hi = F32(np.float64(a) * c), F32(np.float64(a2) * c)
        if hi == np.nextafter(lo, F32(2)):
            break
        a = a2
    put('one_ulp', 8, 2, {3: np.complex64(a), 11: np.complex64(a2)})
    special['one_ulp_values'] = (float(lo), float(hi))
    xmap[10, L - 3, 17] = np.complex64(complex(np.nan, 0.25))
    special['nan'] = (10, L - 3)
    if alphabet == '16QAM':
        xmap[12, L - 1, 20] = np.complex64(complex(np.inf, 0.5))   # re_k != 0 for every point: +-inf, no NaN
        special['inf'] = (12, L - 1)
        # the maximum on the table's duplicated point -1+3j (k = 13 and 14).  That point lies on the
        # top edge of the constellation's hull, between -3+3j and 3+3j, so Re(x conj(a)) is never
        # largest there alone: the input that puts the maximum on it is purely imaginary, and the
        # maximum is then shared by all five points of imaginary part 3 (k = 8, 10, 12, 13, 14), both
        # copies among them; the lowest k is taken
        dup = [k for k in range(K) if sym[k] == sym[13]]
        assert dup == [13, 14], dup
        put('dup_point', 0, 1, {9: np.complex64(1.25j)})
    return cfg, sym, xmap.reshape(B, N), xmmse.reshape(B, N), x.reshape(B, N), special


def _expected(xmap, x, xmmse, sym, M):
    """numpy's decision (the oracle's rule), the mismatch flag and the squared-error sum per section."""
    xa = xmap.reshape(-1, M)
    with np.errstate(all='ignore'):
        tmp = (xa.astype(np.complex128)[:, :, None] * np.conj(sym)[None, None, :]).real
    flat = tmp.reshape(xa.shape[0], -1).argmax(axis=1)
    mh, kh = np.divmod(flat, len(sym))
    xhat = np.zeros_like(xa)
    xhat[np.arange(xa.shape[0]), mh] = sym.astype(np.complex64)[kh]
    mm = (xhat != x.reshape(-1, M)).any(axis=1).astype(np.int32)
    d = (xmmse.reshape(-1, M) - x.reshape(-1, M))
    se = (d.real.astype(np.float64) ** 2 + d.imag.astype(np.float64) ** 2).sum(axis=1)
    return flat.astype(np.int32), mm, se


def _run_debug(cfg, dev, xmap, xmmse, x, narrow):
    import amp_native as nat
    d, c = cfg.dims(), cfg.constellation()
    S = cfg.B * cfg.L
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    a, b, e = t(xmap), t(xmmse), t(x)
    bi = torch.full((S,), -1, dtype=torch.int32, device=dev)
    mm = torch.full((S,), -1, dtype=torch.int32, device=dev)
    se = torch.full((S,), -1.0, dtype=torch.float64, device=dev)
    nat.check(nat.lib().amp_decide_debug_sections(C.byref(d), C.byref(c), nat.dptr(a), nat.dptr(b), nat.dptr(e),
                                                  int(narrow), nat.dptr(bi), nat.dptr(mm), nat.dptr(se),
                                                  nat.stream_ptr(dev)), 'amp_decide_debug_sections')
    torch.cuda.synchronize()
    return bi.cpu().numpy(), mm.cpu().numpy(), se.cpu().numpy()


def _run_map_decide(cfg, dev, xmap, xmmse, x):
    import amp_native as nat
    d, c = cfg.dims(), cfg.constellation()
    S = cfg.B * cfg.L
    lib = nat.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    a, b, e = t(xmap), t(xmmse), t(x)
    lab = torch.zeros(S, dtype=torch.int64, device=dev)
    wsb = lib.amp_map_decide_workspace_bytes(C.byref(d))
    ws = torch.zeros(max(wsb, 16), dtype=torch.uint8, device=dev)
    counts = torch.zeros(256, dtype=torch.uint8, device=dev)
    dec = torch.full((S,), -1, dtype=torch.int32, device=dev)
    nat.check(lib.amp_map_decide_count(C.byref(d), C.byref(c), nat.dptr(a), nat.dptr(b), nat.dptr(e), nat.dptr(lab),
                                       nat.dptr(lab), 8, nat.dptr(counts), nat.dptr(dec), nat.dptr(ws), wsb,
                                       nat.stream_ptr(dev)), 'amp_map_decide_count')
    torch.cuda.synchronize()
    return dec.cpu().numpy()


@pytest.mark.parametrize('shape', SHAPES, ids=IDS)
def test_narrow_scan_decides_what_the_full_scan_and_numpy_decide(device, shape):
    alphabet, Nt, Na, B = shape
    cfg, sym, xmap, xmmse, x, special = _build(alphabet, Nt, Na, B, seed=20 + Na)
    K, M, L = len(sym), Nt // Na, Na
    sec = lambda name: xmap.reshape(B, L, M)[special[name]]  # noqa: E731
    sid = lambda name: special[name][0] * L + special[name][1]  # noqa: E731
    want, want_mm, want_se = _expected(xmap, x, xmmse, sym, M)

    # ---- the built properties, on the CPU ----
    narrow = np.array([_section_narrow(s, sym) for s in xmap.reshape(-1, M)])
    assert narrow[:(B - 2) * L].sum() >= (B - 2) * L - 8, 'ordinary rows: one candidate position per lane'
    for name in ('tie_same_lane', 'all_zero', 'one_ulp', 'nan') + (('inf',) if 'inf' in special else ()):
        assert not narrow[sid(name)], name
    for name in ('tie_two_lanes',) + (('dup_point',) if 'dup_point' in special else ()):
        assert narrow[sid(name)], name
    v, thr = _prefilter(sec('tie_same_lane'), sym)
    assert v[5].max() == v[9].max() == v.max() and want[sid('tie_same_lane')] // K == 5
    v, thr = _prefilter(sec('tie_two_lanes'), sym)
    assert v[6].max() == v[7].max() == v.max() and want[sid('tie_two_lanes')] // K == 6
    assert want[sid('all_zero')] == 0
    v, thr = _prefilter(sec('one_ulp'), sym)
    lo, hi = special['one_ulp_values']
    assert float(v[3].max()) == lo and float(v[11].max()) == hi and hi == float(np.nextafter(F32(lo), F32(2))) and lo >= thr
    assert want[sid('one_ulp')] // K == 11
    assert want[sid('nan')] == 17 * K                       # np.argmax: the first NaN
    if 'inf' in special:
        assert want[sid('inf')] // K == 20
    if 'dup_point' in special:
        v, thr = _prefilter(sec('dup_point'), sym)
        top = [k for k in range(K) if sym[k].imag == sym[13].imag]
        assert top == [8, 10, 12, 13, 14] and (v >= thr).sum() == 5
        assert (v[9, top] == v.max()).all() and v[9, 13] == v[9, 14] >= thr
        assert want[sid('dup_point')] == 9 * K + 8
    if L == 8:
        # a wave decides rows 2 w and 2 w + 1 of a workgroup: each built fallback section stands
        # alone among fifteen sections with one candidate position per lane (the NaN and the inf
        # section beside ordinary ones), and the ties across lanes sit in waves that stay narrow
        for name in ('tie_same_lane', 'all_zero', 'one_ulp', 'nan') + (('inf',) if 'inf' in special else ()):
            r0 = special[name][0] & ~1
            assert (~narrow[r0 * L:(r0 + 2) * L]).sum() == 1, name
        for name in ('tie_two_lanes',) + (('dup_point',) if 'dup_point' in special else ()):
            r0 = special[name][0] & ~1
            assert narrow[r0 * L:(r0 + 2) * L].all(), name

    # ---- the GPU ----
    dec = _run_map_decide(cfg, device, xmap, xmmse, x)
    assert np.array_equal(dec, want), np.flatnonzero(dec != want)[:8]
    bi_n, mm_n, se_n = _run_debug(cfg, device, xmap, xmmse, x, narrow=True)
    bi_o, mm_o, se_o = _run_debug(cfg, device, xmap, xmmse, x, narrow=False)
    assert np.array_equal(bi_o, want), np.flatnonzero(bi_o != want)[:8]
    assert np.array_equal(bi_n, want), np.flatnonzero(bi_n != want)[:8]
    assert np.array_equal(mm_n, mm_o) and np.array_equal(mm_o, want_mm)
    assert np.array_equal(se_n.view(np.uint64), se_o.view(np.uint64))
    assert np.allclose(se_o, want_se, rtol=1e-12, atol=0)
