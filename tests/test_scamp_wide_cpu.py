"""SCAMP at any Nt (coupling blocks wider than 128, Nt no power of two) on the CPU (no GPU needed).

* g15 (tests/golden/make_g15_scamp_wide.py: the reference's SCAMP at five batch = 1 points of 40
  trials and three B = 48 points) is reproduced by the oracle's scamp_detect: every counting metric
  of every trial; VER and SER within 1e-3 (the project's parity bar) at the batch points.  T is not
  compared per trial (test_scamp_trials_cpu.py: at B = 1 the allclose exit is decided by rounding).
* amp_scamp_run and amp_scamp_trials_run take the five shapes: with dummy pointers and ws_bytes = 0
  they get as far as the workspace check (every check precedes the first use of a pointer), and
  amp_scamp_trials_workspace_bytes answers for them; Lin = 65 is still refused.
* the workspace of the reference driver's shape holds the launch engine's two operators and little
  else (the persistent engines' operators are carved only where a persistent engine can run), and
  the shapes a persistent engine takes report the bytes they reported before.
"""
import ctypes as C

import pytest

import golden_io as gio
import scamp_wide_inputs as wi
from oracle import OracleConfig, loss_dict, scamp_detect


def _oracle_cfg(e):
    return OracleConfig(e['Nt'], e['Na'], e['Nr'], Lin=e['Lin'], Lh=e['Lh'], B=e['B'], alphabet=e['alphabet'],
                        mode=e['mode'], iterations=e['iterations'])


def test_g15_points():
    assert wi.TRIAL_POINTS == ['trials_8PSK_Nt168', 'trials_OOK_Nt1344', 'trials_OOK_Nt96', 'trials_QPSK_Nt192',
                               'trials_QPSK_Nt480']
    assert wi.BATCH_POINTS == ['batch_8PSK_Nt168', 'batch_OOK_Nt1344', 'batch_QPSK_Nt192']
    for name in wi.TRIAL_POINTS:
        e = wi.G15[name]
        assert len(e['trials']) == wi.E_G15 and e['B'] == 1 and e['iterations'] == 20, name
        M = e['Nt'] // e['Na']
        assert M & (M - 1) == 0 and (e['Nt'] > 128 or e['Nt'] & (e['Nt'] - 1)), name   # what amp_scamp_run refused
    for name in wi.BATCH_POINTS:
        assert wi.G15[name]['B'] == 48 and int(wi.G15[name]['loss']['T']) == 20, name


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_oracle_trial_by_trial_matches_g15(name):
    e = wi.G15[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
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


@pytest.mark.parametrize('name', wi.BATCH_POINTS)
def test_oracle_matches_g15_batch_points(name):
    e = wi.G15[name]
    inp = wi.host_inputs(name)
    cfg = _oracle_cfg(e)
    c = lambda t: t.numpy().reshape(e['B'], -1)   # noqa: E731
    o = scamp_detect(inp['W'].numpy().reshape(cfg.Lout, cfg.Lin), inp['A'].numpy(), c(inp['y']), inp['SNR'], cfg)
    got = loss_dict(o['xmap'], o['xmmse'], c(inp['x']), inp['sym'], inp['idx'], o['T'], cfg)
    for k in ('ver', 'ser'):
        print(name, k, float(got[k]), e['loss'][k])
        assert abs(float(got[k]) - e['loss'][k]) <= 1e-3, (k, float(got[k]), e['loss'][k])


def _dummy_args(nat, ptr):
    a = nat.AmpScampArgs()
    a.W = a.A = a.y = a.xmap = a.xmmse = a.psi = a.status = a.ws = ptr
    a.ws_bytes = 0                                   # a valid call stops here, before any launch
    a.max_iter, a.engine, a.gemm, a.noise_var = 20, nat.ENGINE_LAUNCHES, nat.GEMM_AUTO, 0.1
    return a


@pytest.mark.parametrize('name', wi.TRIAL_POINTS)
def test_scamp_entries_take_the_wide_shapes_up_to_the_workspace_check(name):
    import amp_native as nat
    lib = nat.lib()
    cfg = wi.config_of(name)
    d, cst = cfg.dims(), cfg.constellation()
    buf = (C.c_char * 64)()
    ptr = C.cast(buf, C.c_void_p).value
    a = _dummy_args(nat, ptr)
    assert lib.amp_scamp_run(C.byref(d), C.byref(cst), C.byref(a), None) == -1
    assert 'workspace' in lib.amp_last_error().decode(), lib.amp_last_error().decode()
    assert lib.amp_scamp_trials_run(C.byref(d), C.byref(cst), C.byref(a), None, 4, None) == -1
    assert 'workspace' in lib.amp_last_error().decode(), lib.amp_last_error().decode()
    one = lib.amp_scamp_trials_workspace_bytes(C.byref(d), 20, 1)
    many = lib.amp_scamp_trials_workspace_bytes(C.byref(d), 20, 40)
    assert 0 < one < many, (name, one, many)
    wide = cfg.dims()
    wide.Lin = 65                                    # more coupling blocks than amp_scamp_run takes
    assert lib.amp_scamp_trials_workspace_bytes(C.byref(wide), 20, 4) == 0


def _geometry(d):
    """scamp_geometry (csrc/amp_scamp.h): the launch engine's packed operators [ncpA][kapA], [ncpB][kapB]."""
    up = lambda v, a: (v + a - 1) // a * a   # noqa: E731
    bn = 128 if 2 * d.M <= 128 else 256
    return up(2 * d.n, 128), up(2 * d.N, 64), up(2 * d.N, bn), up(2 * d.n, 64)


def test_driver_shape_workspace_holds_the_launch_operators_only():
    import amp_native as nat
    lib = nat.lib()
    cfg = wi.driver_config()
    d = cfg.dims()
    assert (d.N, d.n, d.L, d.M) == (1344 * 32, 73 * 37, 84 * 32, 16)
    ncpA, kapA, ncpB, kapB = _geometry(d)
    got = lib.amp_scamp_workspace_bytes(C.byref(d), 100)
    bound = 4 * (ncpA * kapA + ncpB * kapB) + (64 << 20)
    print('driver shape workspace', got, 'bound', bound)
    assert 0 < got <= bound, (got, bound)
    assert lib.amp_scamp_trials_workspace_bytes(C.byref(d), 100, 100) > 4 * (ncpA * kapA + ncpB * kapB)


# (Nt, Na, Nr, B, alphabet): cfg3 (tools/configs_bench.py) and one shape of each (2N, 2n) the
# persistent engine takes; the bytes are those of the build before the carve became conditional
PERSIST_BYTES = [((128, 8, 256, 4096, '16QAM'), 33212416),    # cfg3: (256, 512)
                 ((64, 4, 128, 64, 'QPSK'), 964096),          # (128, 256)
                 ((128, 8, 128, 48, 'QPSK'), 1652992),        # (256, 256)
                 ((128, 8, 256, 1, 'QPSK'), 2992640)]         # (256, 512) at B = 1


@pytest.mark.parametrize('shape,want', PERSIST_BYTES)
def test_persistent_shapes_keep_their_workspace_bytes(shape, want):
    import amp_native as nat
    from config import Config
    Nt, Na, Nr, B, alph = shape
    cfg = Config(Nt, Na, Nr, 1, 1, batch=B, generator_mode='sparc', iterations=20, alphabet=alph,
                 channel_profile='uniform', channel_truncation='tail', device='cpu')
    d = cfg.dims()
    assert nat.lib().amp_scamp_workspace_bytes(C.byref(d), 20) == want
