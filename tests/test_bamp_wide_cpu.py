"""BAMP at odd n, N % 4 == 2 and a partial last column tile, on the CPU (no GPU needed).

* g16 (tests/golden/make_g16_bamp_wide.py: the reference's BAMP at eight batch = 1 points of 40
  trials and five B = 48 points) is reproduced by the oracle's bamp_detect: every counting metric of
  every trial; VER and SER equal at the batch points.  T is not compared per trial (at B = 1 the
  allclose exit is decided by rounding).
* the shape gate through the ABI: with null buffers amp_bamp_run and amp_bamp_trials_run get as far
  as the null-pointer check at (N = 18, n = 15), (N = 96, n = 36) and the published N = 43008,
  n = 2701 (every check of a dimension precedes it; before, the text named the dimensions).  The
  split-precision tiles keep their N % 64 rule, an odd N its even-N message, and a shape beyond
  32-bit indexing is refused with a message of its own.
* the workspace: positive and growing with E at the odd shapes; at cfg1, cfg5 and the g13 shapes the
  bytes of the dense layout (the carve's formula, written out below).
"""
import ctypes as C

import pytest

import bamp_wide_inputs as wi
import golden_io as gio
from oracle import OracleConfig, bamp_detect, loss_dict


def _oracle_cfg(e):
    return OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=e['B'], alphabet=e['alphabet'],
                        mode=e['mode'], iterations=e['iterations'])


def test_g16_points():
    assert wi.TRIAL_POINTS == ['trials_8PSK_Nt168', 'trials_BPSK_Nt16', 'trials_OOK_Nt1344', 'trials_OOK_Nt48',
                               'trials_OOK_Nt6', 'trials_QPSK_Nt12', 'trials_QPSK_Nt16', 'trials_QPSK_Nt480']
    assert wi.BATCH_POINTS == ['batch_8PSK_Nt168', 'batch_OOK_Nt1344', 'batch_OOK_Nt48', 'batch_OOK_Nt6',
                               'batch_QPSK_Nt480']
    for name in wi.TRIAL_POINTS:
        e = wi.G16[name]
        assert len(e['trials']) == wi.E_G16 and e['B'] == 1 and e['iterations'] == 20, name
        M = e['Nt'] // e['Na']
        N, n = e['Nt'] * e['Lin'], e['Nr'] * (e['Lin'] + e['Lh'] - 1)
        # what amp_bamp_run refused: N or n no multiple of 4, or a partial last column tile
        assert M & (M - 1) == 0 and (N % 4 or n % 4 or (2 * N > 128 and 2 * N % 128)), name
    for name in wi.BATCH_POINTS:
        assert wi.G16[name]['B'] == 48 and int(wi.G16[name]['loss']['T']) == 20, name
    # exits at odd and at even T (var frozen in either ping-pong buffer) among the points
    Ts = {int(t['T']) % 2 for name in wi.TRIAL_POINTS for t in wi.G16[name]['trials'] if int(t['T']) < 20}
    assert Ts == {0, 1}


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_oracle_trial_by_trial_matches_g16(name):
    e = wi.G16[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
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


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_oracle_matches_g16_batch_points(name):
    e = wi.G16[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
    c = lambda t: t.numpy().reshape(e['B'], -1)   # noqa: E731
    o = bamp_detect(inp['A'].numpy(), c(inp['y']), inp['SNR'], cfg)
    got = loss_dict(o['xmap'], o['xmmse'], c(inp['x']), inp['sym'], inp['idx'], o['T'], cfg)
    for k in ('ver', 'ser'):
        print(name, k, float(got[k]), e['loss'][k])
        assert float(got[k]) == e['loss'][k], (k, float(got[k]), e['loss'][k])


def _config(shape, alph='OOK', batch=1, iterations=20):
    from config import Config
    Nt, Na, Nr, Lin, Lh = shape
    return Config(Nt, Na, Nr, Lin, Lh, batch=batch, generator_mode='sparc', iterations=iterations, alphabet=alph,
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


def _args(nat, ptr, gemm=0):
    a = nat.AmpBampArgs()
    a.H = a.y = a.xmap = a.xmmse = a.var = a.status = a.ws = ptr
    a.ws_bytes = 0                                   # with real pointers a valid call stops here, before any launch
    a.max_iter, a.denoiser, a.gemm, a.noise_var = 20, 0, gemm, 0.1
    return a


def _run(lib, nat, cfg, a, trials=None):
    d, cst = cfg.dims(), cfg.constellation()
    if trials is None:
        rc = lib.amp_bamp_run(C.byref(d), C.byref(cst), C.byref(a), None)
    else:
        rc = lib.amp_bamp_trials_run(C.byref(d), C.byref(cst), C.byref(a), None, trials, None)
    return rc, lib.amp_last_error().decode()


# (Nt, Na, Nr, Lin, Lh): (N, n) = (18, 15), (96, 36), (43008, 2701)
GATE_SHAPES = [(6, 3, 5, 3, 1), (48, 6, 12, 2, 2), (1344, 84, 73, 32, 6)]


@pytest.mark.parametrize('shape', GATE_SHAPES)
def test_bamp_entries_take_the_shapes_up_to_the_null_pointer_check(shape):
    import amp_native as nat
    lib = nat.lib()
    cfg = _config(shape)
    d = cfg.dims()
    assert (d.N, d.n) in ((18, 15), (96, 36), (43008, 2701))
    for trials in (None, 4):
        rc, msg = _run(lib, nat, cfg, _args(nat, None), trials)
        assert rc == -1 and 'null pointer' in msg, (trials, rc, msg)
        for word in ('multiple', 'even', '2N'):      # no dimension is named
            assert word not in msg, msg


@pytest.mark.parametrize('shape', GATE_SHAPES)
def test_split_precision_tiles_keep_their_shape_rule(shape):
    import amp_native as nat
    lib = nat.lib()
    cfg = _config(shape)
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value              # never read: the check precedes every use
    for gemm in (nat.GEMM_X3, nat.GEMM_H2):
        rc, msg = _run(lib, nat, cfg, _args(nat, ptr, gemm))
        assert rc == -1 and 'N % 64 == 0 and n % 64 == 0' in msg, (gemm, rc, msg)
        rc, msg = _run(lib, nat, cfg, _args(nat, ptr, gemm), trials=4)
        assert rc == -1 and 'f32 GEMMs only' in msg, (gemm, rc, msg)
    # AUTO and F32 pass every check of an argument: they stop at the workspace size
    for gemm in (nat.GEMM_AUTO, nat.GEMM_F32):
        for trials in (None, 4):
            rc, msg = _run(lib, nat, cfg, _args(nat, ptr, gemm), trials)
            assert rc == -1 and 'workspace' in msg, (gemm, trials, rc, msg)


def test_odd_N_and_shapes_beyond_32_bit_indexing_are_refused():
    import amp_native as nat
    lib = nat.lib()
    odd = _config((3, 3, 5, 3, 1), 'QPSK')           # M = 1, N = 9
    for trials in (None, 4):
        rc, msg = _run(lib, nat, odd, _args(nat, None), trials)
        assert rc == -1 and 'must be even' in msg, (trials, rc, msg)
    # 30000 rows of 2N = 86016 columns: 2.58e9 > 2^31 - 1
    rc, msg = _run(lib, nat, _config(GATE_SHAPES[2], batch=30000), _args(nat, None))
    assert rc == -1 and '32-bit offsets' in msg and 'amp_bamp_run' in msg, (rc, msg)
    rc, msg = _run(lib, nat, _config(GATE_SHAPES[2]), _args(nat, None), trials=30000)
    assert rc == -1 and '32-bit offsets' in msg and 'amp_bamp_trials_run' in msg, (rc, msg)
    # one row fewer than the limit passes the gate
    rc, msg = _run(lib, nat, _config(GATE_SHAPES[2]), _args(nat, None), trials=24000)
    assert rc == -1 and 'null pointer' in msg, (rc, msg)


# ---- the workspace: the carve of csrc/amp_bamp.hip and amp_bamp_trials.hip for the dense layout ----

def _up(v, a):
    return (v + a - 1) // a * a


class _Carve:
    def __init__(self):
        self.off = 0

    def take(self, count, size):
        self.off = _up(self.off, 256) + count * size


def _geometry(d):
    bn = 128 if 2 * d.M <= 128 else 256
    return dict(bn=bn, kapA1=_up(d.N, 64), ncpA1=_up(d.n, 128), kapA2=_up(2 * d.N, 64), ncpA2=_up(2 * d.n, 128),
                kapB1=_up(d.n, 64), ncpB1=_up(d.N, 128), kapB2=_up(2 * d.n, 64), ncpB2=_up(2 * d.N, bn))


def dense_bamp_bytes(d, max_iter):
    """bamp_carve with invu [B][n] and s [B][2n]: the layout every shape had when N % 4 == n % 4 == 0
    was required."""
    g = _geometry(d)
    B, split = d.B, d.N % 64 == 0 and d.n % 64 == 0
    cv = _Carve()
    cv.take(g['ncpA1'] * g['kapA1'] * (3 if split else 2) // 2, 4)
    cv.take(g['ncpA2'] * g['kapA2'], 4)
    cv.take(g['ncpB1'] * g['kapB1'] * (3 if split else 2) // 2, 4)
    cv.take(g['ncpB2'] * g['kapB2'], 4)
    for count in (B * d.n, B * 2 * d.n, B * d.n, B * 2 * d.n, B * d.N, B * d.N, B * d.L, B * d.L):
        cv.take(count, 4)                            # v z invu s cov var1 secmax secabs
    nblk = -(-B // 32) * (g['ncpB2'] // g['bn'])
    cv.take(max_iter * nblk, 32)                     # Partial
    cv.take(max_iter + 1, 48)                        # BampIter
    for nt in (g['ncpA1'] // 128, g['ncpA2'] // 128, g['ncpB1'] // 128, g['ncpB2'] // g['bn']):
        cv.take(2 * nt, 4)
    cv.take(1, 96)                                   # XState
    cv.take(16, 4)
    if split:
        rp = _up(B, 32)
        cv.take(6 * rp * max(d.N, d.n), 2)
        cv.take(rp, 4)
    return cv.off


def dense_trials_bytes(d, E):
    """tbamp_carve with invu [E][n] and s [E][2n], and the decision's tail (trials_decide_ws_bytes)."""
    g = _geometry(d)
    cv = _Carve()
    for a, b in (('ncpA1', 'kapA1'), ('ncpA2', 'kapA2'), ('ncpB1', 'kapB1'), ('ncpB2', 'kapB2')):
        cv.take(g[a] * g[b], 4)
    for count in (E * d.n, E * 2 * d.n, E * d.n, E * 2 * d.n, E * d.N, E * d.N, E * d.L, E * d.L):
        cv.take(count, 4)
    cv.take(E * (g['ncpB2'] // g['bn']), 32)
    cv.take(E, 16)                                   # TBampIter
    for nt in (g['ncpA1'] // 128, g['ncpA2'] // 128, g['ncpB1'] // 128, g['ncpB2'] // g['bn']):
        cv.take(2 * nt, 4)
    cv.take(16, 4)
    per = 4 * (64 // min(d.M, 64))                   # trials_decide_nblk: sections per workgroup
    dec = _Carve()
    dec.take(E * d.L, 1)
    dec.take(E * max(1, min(-(-d.L // per), 2048)), 64)
    cv.take(dec.off, 1)
    return cv.off


# (Nt, Na, Nr, Lin, Lh), B, alphabet, iterations: cfg1, cfg5 (tools/configs_bench.py, cfg5_bench.py)
# and the two BAMP shapes of g13 (make_g13_trials.py)
DENSE_SHAPES = [((4, 1, 8, 1, 1), 100, 'QPSK', 10),
                ((512, 16, 1024, 1, 1), 8192, 'QPSK', 20),
                ((32, 4, 64, 1, 1), 1, 'QPSK', 20),
                ((16, 2, 12, 4, 2), 1, 'OOK', 20)]


@pytest.mark.parametrize('shape,B,alph,it', DENSE_SHAPES)
def test_workspace_bytes_unchanged_where_nothing_is_padded(shape, B, alph, it):
    import amp_native as nat
    lib = nat.lib()
    d = _config(shape, alph, batch=B, iterations=it).dims()
    assert d.N % 4 == 0 and d.n % 4 == 0
    got, want = lib.amp_bamp_workspace_bytes(C.byref(d), it), dense_bamp_bytes(d, it)
    print(shape, B, 'amp_bamp_workspace_bytes', got, 'dense layout', want)
    assert got == want
    d1 = _config(shape, alph, batch=1, iterations=it).dims()
    for E in (1, 40, 100):
        got, want = lib.amp_bamp_trials_workspace_bytes(C.byref(d1), it, E), dense_trials_bytes(d1, E)
        assert got == want, (shape, E, got, want)


@pytest.mark.parametrize('shape', GATE_SHAPES + [(16, 4, 3, 2, 2), (168, 84, 73, 3, 2)])
def test_workspace_bytes_at_the_odd_shapes(shape):
    import amp_native as nat
    lib = nat.lib()
    d1 = _config(shape).dims()
    one = lib.amp_bamp_trials_workspace_bytes(C.byref(d1), 20, 1)
    many = lib.amp_bamp_trials_workspace_bytes(C.byref(d1), 20, 40)
    more = lib.amp_bamp_trials_workspace_bytes(C.byref(d1), 20, 100)
    assert 0 < one < many < more, (shape, one, many, more)
    # the padded rows: at most three floats per row of invu and of s beyond the dense layout
    for E in (40, 100):
        got, dense = lib.amp_bamp_trials_workspace_bytes(C.byref(d1), 20, E), dense_trials_bytes(d1, E)
        assert dense <= got <= dense + 4 * 6 * E + 2 * 256, (shape, E, got, dense)
    d48 = _config(shape, batch=48).dims()
    got, dense = lib.amp_bamp_workspace_bytes(C.byref(d48), 20), dense_bamp_bytes(d48, 20)
    assert 0 < dense <= got <= dense + 4 * 6 * 48 + 2 * 256, (shape, got, dense)
