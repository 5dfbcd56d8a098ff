"""VAMP at odd n, odd k and a partial last column tile, on the CPU (no GPU needed).

* g17 (tests/golden/make_g17_vamp_wide.py: the reference's VAMP at nine batch = 1 points of 40
  trials and eight B = 48 points) is reproduced by the oracle's vamp_detect: every counting metric
  of every trial; VER and SER equal at the batch points.  T is not compared per trial (at B = 1 the
  allclose exit is decided by rounding).
* the shape gate through the ABI: amp_vamp_run, the layer-level entry points, amp_vamp_run_sharded
  and amp_vamp_trials_run pass every check of an argument at (N, n, k) = (18, 15, 15), (8, 11, 8),
  (96, 36, 36) and the published (43008, 2701, 2701): with null buffers they stop at the null-pointer
  check, with a dummy pointer at the workspace size (before, the text named n or k).  An odd N keeps
  its even-N message, the split-precision arithmetics and amp_vamp2_run keep their rules, and a shape
  beyond 32-bit indexing is refused with a message of its own.
* the workspace: at persistent-eligible shapes (cfg2, cfg4, N = 128) exactly the bytes of the carve
  that holds every engine's buffers (written out below); strictly fewer at the odd and published
  shapes, where no persistent engine can run; the trials workspace grows with E.
"""
import ctypes as C

import pytest

import golden_io as gio
import vamp_wide_inputs as wi
from oracle import OracleConfig, loss_dict, vamp_detect


def _oracle_cfg(e):
    return OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=e['B'], alphabet=e['alphabet'],
                        mode=e['mode'], iterations=e['iterations'])


def test_g17_points():
    assert wi.TRIAL_POINTS == ['trials_8PSK_Nt168', 'trials_BPSK_Nt8', 'trials_OOK_Nt1344', 'trials_OOK_Nt16',
                               'trials_OOK_Nt48', 'trials_OOK_Nt6', 'trials_QPSK_Nt12', 'trials_QPSK_Nt16',
                               'trials_QPSK_Nt480']
    assert wi.BATCH_POINTS == ['batch_8PSK_Nt168', 'batch_BPSK_Nt8', 'batch_OOK_Nt1344', 'batch_OOK_Nt16',
                               'batch_OOK_Nt48', 'batch_OOK_Nt6', 'batch_QPSK_Nt16', 'batch_QPSK_Nt480']
    for name in wi.TRIAL_POINTS:
        e = wi.G17[name]
        assert len(e['trials']) == wi.E_G17 and e['B'] == 1 and e['iterations'] == 20, name
        M = e['Nt'] // e['Na']
        N, n = e['Nt'] * e['Lin'], e['Nr'] * (e['Lin'] + e['Lh'] - 1)
        # what the VAMP launch engines refused: an odd n (so an odd k where n < N) or a partial last tile
        assert M & (M - 1) == 0 and N % 2 == 0 and (n % 2 or (2 * N > 128 and 2 * N % 128)), name
    for name in wi.BATCH_POINTS:
        assert wi.G17[name]['B'] == 48 and int(wi.G17[name]['loss']['T']) == 20, name
    # exits at odd and at even T (var frozen in either ping-pong buffer) within one point
    Ts = {int(t['T']) % 2 for t in wi.G17['trials_QPSK_Nt12']['trials'] if int(t['T']) < 20}
    assert Ts == {0, 1}


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_oracle_trial_by_trial_matches_g17(name):
    e = wi.G17[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
    c = lambda t: t.numpy().reshape(1, -1)   # noqa: E731
    U, s, Vh = inp['U'].numpy(), inp['s'].numpy(), inp['Vh'].numpy()
    bad, tdiff = {}, []
    for j, ref in enumerate(e['trials']):
        o = vamp_detect(U, s, Vh, c(inp['y'][j]), inp['SNR'], cfg)
        got = loss_dict(o['r'], o['xmmse'], c(inp['x'][j]), inp['sym'][j], inp['idx'][j], o['T'], cfg)
        d = {k: (float(got[k]), ref[k]) for k in gio.COUNT_KEYS if float(got[k]) != ref[k]}
        if d:
            bad[j] = d
        if int(o['T']) != int(ref['T']):
            tdiff.append((j, int(o['T']), int(ref['T'])))
    print(name, 'trials whose T differs from the reference:', len(tdiff), tdiff)
    assert not bad, bad


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_oracle_matches_g17_batch_points(name):
    e = wi.G17[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
    c = lambda t: t.numpy().reshape(e['B'], -1)   # noqa: E731
    o = vamp_detect(inp['U'].numpy(), inp['s'].numpy(), inp['Vh'].numpy(), c(inp['y']), inp['SNR'], cfg)
    got = loss_dict(o['r'], o['xmmse'], c(inp['x']), inp['sym'], inp['idx'], o['T'], cfg)
    for k in ('ver', 'ser'):
        print(name, k, float(got[k]), e['loss'][k])
        assert float(got[k]) == e['loss'][k], (k, float(got[k]), e['loss'][k])


def _config(shape, alph='OOK', batch=1, iterations=20):
    from config import Config
    Nt, Na, Nr, Lin, Lh = shape
    return Config(Nt, Na, Nr, Lin, Lh, batch=batch, generator_mode='sparc', iterations=iterations, alphabet=alph,
                  channel_profile='uniform', channel_truncation='tail', device='cpu')


def _args(nat, ptr, k, gemm=0, engine=0):
    a = nat.AmpVampArgs()
    a.U = a.s = a.Vh = a.y = a.r = a.xmmse = a.var = a.status = a.ws = ptr
    a.ws_bytes = 0                                   # with real pointers a valid call stops here, before any launch
    a.k, a.max_iter, a.engine, a.gemm = k, 20, engine, gemm
    a.noise_var, a.sparsity = 0.1, 0.5
    return a


def _dummy():
    buf = (C.c_char * 64)()
    return buf, C.cast(buf, C.c_void_p).value        # never read: the checks precede every use


ENTRIES = ('run', 'prepare', 'iterate', 'finalize', 'sharded', 'trials')


def _call(lib, cfg, a, entry, trials=4):
    d, cst = cfg.dims(), cfg.constellation()
    r = C.byref
    if entry == 'run':
        rc = lib.amp_vamp_run(r(d), r(cst), r(a), None)
    elif entry == 'prepare':
        rc = lib.amp_vamp_prepare(r(d), r(cst), r(a), None)
    elif entry == 'iterate':
        rc = lib.amp_vamp_iterate(r(d), r(cst), r(a), 0, None)
    elif entry == 'finalize':
        rc = lib.amp_vamp_finalize(r(d), r(cst), r(a), None)
    elif entry == 'sharded':
        rc = lib.amp_vamp_run_sharded(r(d), r(cst), r(a), d.B, None)
    else:
        rc = lib.amp_vamp_trials_run(r(d), r(cst), r(a), None, trials, None)
    return rc, lib.amp_last_error().decode()


# (Nt, Na, Nr, Lin, Lh): (N, n, k) = (18, 15, 15), (8, 11, 8), (96, 36, 36), (43008, 2701, 2701)
GATE_SHAPES = [(6, 3, 5, 3, 1), (8, 2, 11, 1, 1), (48, 6, 12, 2, 2), (1344, 84, 73, 32, 6)]
GATE_DIMS = ((18, 15), (8, 11), (96, 36), (43008, 2701))


@pytest.mark.parametrize('shape', GATE_SHAPES)
def test_vamp_entries_pass_every_argument_check_at_the_shapes(shape):
    import amp_native as nat
    lib = nat.lib()
    cfg = _config(shape)
    d = cfg.dims()
    assert (d.N, d.n) in GATE_DIMS
    k = min(d.N, d.n)
    keep, ptr = _dummy()
    for entry in ENTRIES:
        rc, msg = _call(lib, cfg, _args(nat, None, k), entry)
        assert rc == -1 and 'null pointer' in msg, (entry, rc, msg)
        for gemm in (nat.GEMM_AUTO, nat.GEMM_F32):
            rc, msg = _call(lib, cfg, _args(nat, ptr, k, gemm), entry)
            assert rc == -1 and 'workspace' in msg, (entry, gemm, rc, msg)
            for word in ('multiple', 'even', '2N'):      # no dimension is named
                assert word not in msg, msg
    # k beyond min(n, N) is still refused
    rc, msg = _call(lib, cfg, _args(nat, ptr, k + 1), 'run')
    assert rc == -1 and 'must be min(n, N)' in msg, (rc, msg)


@pytest.mark.parametrize('shape', GATE_SHAPES)
def test_split_precision_arithmetics_and_vamp2_keep_their_rules(shape):
    import amp_native as nat
    lib = nat.lib()
    cfg = _config(shape)
    d, cst = cfg.dims(), cfg.constellation()
    k = min(d.N, d.n)
    keep, ptr = _dummy()
    for gemm in (nat.GEMM_X3, nat.GEMM_H2, nat.GEMM_I8):
        for entry in ENTRIES[:-1]:
            rc, msg = _call(lib, cfg, _args(nat, ptr, k, gemm), entry)
            assert rc == -1 and 'the split-precision engines need k == N, N % 64 == 0' in msg, (entry, gemm, rc, msg)
        rc, msg = _call(lib, cfg, _args(nat, ptr, k, gemm), 'trials')
        assert rc == -1 and 'f32 GEMMs only' in msg, (gemm, rc, msg)
    # the persistent engine is never eligible here
    assert lib.amp_vamp_select_engine(C.byref(d), k, nat.ENGINE_AUTO) == nat.ENGINE_LAUNCHES
    rc, msg = _call(lib, cfg, _args(nat, ptr, k, engine=nat.ENGINE_PERSISTENT), 'trials')
    assert rc == -1 and 'persistent engine has no independent-trial form' in msg, (rc, msg)
    # damped VAMP (amp_vamp2_run): an even n, and 2N within one column tile or a multiple of it
    a2 = nat.AmpVamp2Args()
    a2.U = a2.s = a2.Vh = a2.y = a2.r = a2.xmmse = a2.var = a2.status = a2.ws = ptr
    a2.k, a2.max_iter, a2.sigma2, a2.damping, a2.ws_bytes = k, 20, 0.1, 0.5, 0
    rc = lib.amp_vamp2_run(C.byref(d), C.byref(cst), C.byref(a2), None)
    msg = lib.amp_last_error().decode()
    want = 'must be even' if d.n % 2 else 'or a multiple of it'
    assert rc == -1 and want in msg, (rc, msg)


def test_odd_N_and_shapes_beyond_32_bit_indexing_are_refused():
    import amp_native as nat
    lib = nat.lib()
    odd = _config((3, 3, 5, 3, 1), 'QPSK')           # M = 1, N = 9
    for entry in ENTRIES:
        rc, msg = _call(lib, odd, _args(nat, None, 9), entry)
        assert rc == -1 and 'must be even' in msg, (entry, rc, msg)
    pub = GATE_SHAPES[3]
    # rows x (2N + 4) = rows x 86020 within 2^31 - 1: 24964 rows pass, 24965 do not
    assert 24964 * 86020 <= 2**31 - 1 < 24965 * 86020
    for entry in ENTRIES[:-1]:
        rc, msg = _call(lib, _config(pub, batch=24965), _args(nat, None, 2701), entry)
        assert rc == -1 and '32-bit offsets' in msg and 'amp_vamp' in msg, (entry, rc, msg)
    rc, msg = _call(lib, _config(pub, batch=24964), _args(nat, None, 2701), 'run')
    assert rc == -1 and 'null pointer' in msg, (rc, msg)
    rc, msg = _call(lib, _config(pub), _args(nat, None, 2701), 'trials', trials=24965)
    assert rc == -1 and '32-bit offsets' in msg and 'amp_vamp_trials_run' in msg, (rc, msg)
    rc, msg = _call(lib, _config(pub), _args(nat, None, 2701), 'trials', trials=24964)
    assert rc == -1 and 'null pointer' in msg, (rc, msg)


# ---- the workspace: vamp_carve (csrc/amp_vamp.h) with every engine's buffers, dense w ----

def _up(v, a):
    return (v + a - 1) // a * a


class _Carve:
    def __init__(self):
        self.off = 0

    def take(self, count, size):
        self.off = _up(self.off, 256) + count * size


def _geometry(d, k):
    bn = 128 if 2 * d.M <= 128 else 256
    return dict(bn=bn, kap0=_up(2 * d.n, 64), ncp0=_up(2 * k, 128), kap1=_up(2 * d.N, 64), ncp1=_up(2 * k, 128),
                kap2=_up(2 * k, 64), ncp2=_up(2 * d.N, bn))


def full_vamp_bytes(d, k, max_iter, persistent=True):
    """vamp_carve as it stood while every shape held the persistent engines' operators (Wq0, Wq1,
    Wq2, Wx1, Wx2) and w was [B][2k]; persistent=False leaves those five out."""
    g = _geometry(d, k)
    B, N, n = d.B, d.N, d.n
    cv = _Carve()
    for a, b in (('ncp0', 'kap0'), ('ncp1', 'kap1'), ('ncp2', 'kap2')):
        cv.take(g[a] * g[b], 4)
    for count in (k, B * 2 * k, B * 2 * k, B * N, B * d.L, B * d.L):
        cv.take(count, 4)                            # s2 ytil w var1 secmax secabs
    cv.take(max_iter * (-(-B // 32) * (g['ncp2'] // g['bn'])), 32)   # Partial
    cv.take(max_iter + 1, 80)                        # VampIter
    nwg = -(-B // 16)
    if persistent:
        for count in (2 * k * 2 * n, 2 * k * 2 * N, 2 * N * 2 * k, 3 * k * N, 3 * k * N):
            cv.take(count, 4)                        # Wq0 Wq1 Wq2 Wx1 Wx2
    cv.take(max_iter * nwg * 4, 8)                   # pxch
    cv.take(64 + 256, 4)                             # pbar
    cv.take(max_iter * nwg, 32)                      # pparts
    cv.take(2 * nwg, 128)                            # DecWG
    cv.take(1, 96)                                   # XState
    cv.take(2 * k, 4)                                # q0
    return cv.off


def dense_trials_bytes(d, k, E):
    """tvamp_carve with w [E][2k], and the decision's tail (trials_decide_ws_bytes)."""
    g = _geometry(d, k)
    cv = _Carve()
    for a, b in (('ncp0', 'kap0'), ('ncp1', 'kap1'), ('ncp2', 'kap2')):
        cv.take(g[a] * g[b], 4)
    for count in (k, E * 2 * k, E * 2 * k, E * d.N, E * d.L, E * d.L):
        cv.take(count, 4)
    cv.take(E * (g['ncp2'] // g['bn']), 32)
    cv.take(E, 80)                                   # VampIter
    cv.take(16, 4)
    per = 4 * (64 // min(d.M, 64))                   # trials_decide_nblk: sections per workgroup
    dec = _Carve()
    dec.take(E * d.L, 1)
    dec.take(E * max(1, min(-(-d.L // per), 2048)), 64)
    cv.take(dec.off, 1)
    return cv.off


# (Nt, Na, Nr, Lin, Lh), B, alphabet: cfg2, cfg4 (tools/configs_bench.py), N = 128, and cfg2's shape
# at B = 1 and B = 100 (no multiple of the 16 trials of a persistent workgroup)
PERSIST_SHAPES = [((64, 4, 128, 1, 1), 1024, '16QAM'),
                  ((256, 8, 512, 1, 1), 4096, '16QAM'),
                  ((128, 8, 256, 1, 1), 512, 'QPSK'),
                  ((64, 4, 128, 1, 1), 1, 'QPSK'),
                  ((64, 4, 64, 1, 1), 100, 'QPSK')]


@pytest.mark.parametrize('shape,B,alph', PERSIST_SHAPES)
def test_workspace_bytes_unchanged_at_persistent_eligible_shapes(shape, B, alph):
    import amp_native as nat
    lib = nat.lib()
    d = _config(shape, alph, batch=B).dims()
    k = min(d.N, d.n)
    assert k == d.N and d.N in (64, 128, 256)
    for it in (10, 20):
        got, want = lib.amp_vamp_workspace_bytes(C.byref(d), k, it), full_vamp_bytes(d, k, it)
        print(shape, B, it, 'amp_vamp_workspace_bytes', got, 'full carve', want)
        assert got == want
    d1 = _config(shape, alph, batch=1).dims()
    for E in (1, 40, 100):
        got, want = lib.amp_vamp_trials_workspace_bytes(C.byref(d1), k, 20, E), dense_trials_bytes(d1, k, E)
        assert got == want, (shape, E, got, want)


@pytest.mark.parametrize('shape', GATE_SHAPES + [(16, 4, 3, 2, 2), (168, 84, 73, 3, 2), (16, 2, 12, 4, 2)])
def test_workspace_bytes_smaller_where_no_persistent_engine_can_run(shape):
    import amp_native as nat
    lib = nat.lib()
    for B in (1, 48):
        d = _config(shape, batch=B).dims()
        k = min(d.N, d.n)
        got = lib.amp_vamp_workspace_bytes(C.byref(d), k, 20)
        full, lean = full_vamp_bytes(d, k, 20), full_vamp_bytes(d, k, 20, persistent=False)
        print(shape, B, 'amp_vamp_workspace_bytes', got, 'with the persistent operators', full)
        assert 0 < got < full, (shape, B, got, full)
        # the launch engine's own buffers, w's rows padded by at most two floats
        assert lean <= got <= lean + 4 * 2 * B + 256, (shape, B, got, lean)
    d1 = _config(shape).dims()
    k = min(d1.N, d1.n)
    one, many, more = (lib.amp_vamp_trials_workspace_bytes(C.byref(d1), k, 20, E) for E in (1, 40, 100))
    assert 0 < one < many < more, (shape, one, many, more)
    for E in (40, 100):
        got, dense = lib.amp_vamp_trials_workspace_bytes(C.byref(d1), k, 20, E), dense_trials_bytes(d1, k, E)
        assert dense <= got <= dense + 4 * 2 * E + 256, (shape, E, got, dense)


def test_published_shape_workspace_is_the_launch_engines():
    """Nt=1344 Na=84 Nr=73 Lh=6 Lin=32: 10.5 GB with the persistent operators (6.6 GB that nothing
    reads), 3.9 GB without; Wt1 + Wt2 are 3.8 GB of it."""
    import amp_native as nat
    lib = nat.lib()
    d = _config(GATE_SHAPES[3], iterations=100).dims()
    got = lib.amp_vamp_workspace_bytes(C.byref(d), 2701, 100)
    full = full_vamp_bytes(d, 2701, 100)
    print('published shape: workspace', got, 'bytes; with the persistent operators', full)
    assert 3.8e9 < got < 3.9e9 and 6.6e9 < full - got < 6.7e9
