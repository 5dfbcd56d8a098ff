"""GPU: the eight-wave bf16x3 VAMP engine at one workgroup per CU with the w epilogue split around
GEMM1's closing barrier (AMP_W_PACK_AHEAD: each wave forms w = sc (y~ + vr q) - q and packs its 24
plane words right behind its own GEMM1, ahead of the barrier, and only stores behind it; the record
and the reciprocal table are handed over ahead of the barrier through a flag word the tail wave
raises, with the order before as the fallback) computes the bits it computed before.

Only the time at which instructions issue changes, so every forward must equal, bit for bit, what
the commit before the change computed on an MI355X: r, xmmse and var bits, T, all 13 counters and
status.last_scalar, and from the state dump (amp_vamp_debug_dump), per iteration, every trial row of
w (one CRC-32 per row) and every workgroup's 1 / sigma2 as its denoiser took it.  Against
tests/golden/gemm_seam_bits.part*.npz, recorded on that commit, through its library, with

  python tools/record_forward_bits.py --stem gemm_seam_bits --share-channel --tail --forwards 3 \\
      --cases "256,8,512,35,16QAM;256,8,512,35,QPSK;256,8,512,35,16QAM" --ebn0 "8;0;8" --iters "4;20;4" \\
      --tags ";;naninf" --nan-row ";;33" --inf-entry ";;2,7"

All at N = k = 256, n = 512 (the only geometry these kernels take) and B = 35: the workgroups hold
16, 16 and 3 trials, so the last one packs 13 masked (zero) rows.
  16QAM_256_8_512_35          8 dB, 4 iterations, three forwards on one channel: the first builds, the
                              next two reuse, so their iteration 0 takes q from q0 into the packed store;
  QPSK_256_8_512_35           0 dB, 20 iterations allowed: the forwards stop before the cap (asserted), so
                              the flag and the record of the last executed iteration stand in LDS when the
                              next forward starts and must not be taken for its own;
  16QAM_256_8_512_35#naninf   row 33 of y is NaN and y[2, 7] is +inf: the items that hold them take the
                              masked split (x3_item_masked) inside the pack half; nan_state is the parent's;
  test_a_forward_is_not_marked_by_the_one_before_it: forward A (the first case's building forward), then
                              another channel at another SNR, then A again: A's second result is its first
                              and the fixture's, so no flag or record carries over between launches.

  test_pack_and_store_halves_write_the_whole_items_planes: the two halves alone, around a barrier, through
                              amp_x3_pack_store_debug against the unsplit x3_store_acc_item (form 3 of
                              amp_x3_planes_debug) on rows that hold +-inf, NaN and values that overflow bf16,
                              with 16 and with 3 valid rows.  Both sides run the same pack code (form 3 is the
                              same body, both halves back to back), so this pins the hand-over of the words and
                              the store half; that the shared pack code itself is right is what
                              tests/test_gpu_x3_planes.py holds, which compares form 3 with forms 0-2 and numpy.
  test_a_reuse_forward_behind_a_forward_with_another_iteration_cap: the first case's three forwards, each behind
                              a forward of another detector (iteration cap 1 or 20, another channel and SNR).

Mutations tried once (profiles/r16_gemm_seam_ab.txt has the outcome).  A store half that writes rows row0 + h
with h swapped fails the first case (and the QPSK, the carry-over and the halves' cases).  A pack half that
drops the masked fallback (placed in the pack half alone, not in the shared body) fails the halves' case; it does NOT fail the #naninf case, and no forward can show
it: the inf and the NaN of y spread over the whole row of y~ = (s Uh) y and of w, GEMM2 sums a row's +inf and
-inf products to NaN with or without the mask, and the recorded bits are the same NaNs.  The planes differ
(a masked inf's lower pieces are 0, not NaN), which is what the halves' case compares.
"""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
import record_forward_bits as rec  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
STEM = 'gemm_seam_bits'
QAM = (256, 8, 512, 35, '16QAM')
QPSK = (256, 8, 512, 35, 'QPSK')
# (case, tag, iteration cap)
CASES = [(QAM, '', 4), (QPSK, '', 20), (QAM, 'naninf', 4)]
FORWARDS = 3
FIELDS = ('r', 'xmmse', 'var', 'T', 'nan_state', 'counts', 'last_scalar', 'it_wcrc', 'it_wfin', 'it_inv')

_FIX = {}


def _name(case, tag):
    return rec.case_name(*case) + (f'#{tag}' if tag else '')


def _fixture():
    """{case or 'shared': {field: array}} of the parts, row blocks ('field@i') joined (read once)."""
    if not _FIX:
        raw, k = {}, 0
        while os.path.exists(os.path.join(GOLDEN, f'{STEM}.part{k}.npz')):
            z = np.load(os.path.join(GOLDEN, f'{STEM}.part{k}.npz'))
            raw.update({n: z[n] for n in z.files})
            k += 1
        assert k, 'no fixture parts'
        blocks = {}
        for n, a in raw.items():
            base, _, i = n.partition('@')
            blocks.setdefault(base, []).append((int(i or 0), a))
        for base, bl in blocks.items():
            case, field = base.split('/', 1)
            bl.sort(key=lambda p: p[0])
            _FIX.setdefault(case, {})[field] = bl[0][1] if len(bl) == 1 else np.concatenate([a for _, a in bl], axis=0)
    return _FIX


def _diff(got, want, fields=FIELDS):
    """Every differing array and its first differing index (bitwise)."""
    bad = []
    for name in fields:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append(f'{name}: {a.dtype}{a.shape} != {b.dtype}{b.shape}')
            continue
        ne = a.view(np.uint8).reshape(-1) != b.view(np.uint8).reshape(-1)
        if ne.any():
            i = int(np.flatnonzero(ne)[0]) // a.dtype.itemsize
            where = f' = [iteration, row or workgroup] {np.unravel_index(i, a.shape)}' if name.startswith('it_') else ''
            bad.append(f'{name}: first difference at flat index {i} of {a.size}{where} '
                       f'({a.reshape(-1)[i]!r} != {b.reshape(-1)[i]!r})')
    return bad


def _inputs(fix, case, tag):
    fx = fix[_name(case, tag)]
    ch = fx if 'U' in fx else fix['shared']             # its own channel, or the shared one
    snr = fx['SNR'] if 'SNR' in fx else ch['SNR']       # its own Eb/N0, or the channel's
    return fx, dict(U=torch.from_numpy(ch['U']), s=torch.from_numpy(ch['s']), Vh=torch.from_numpy(ch['Vh']),
                    SNR=float(snr[0]),
                    eps=[dict(x=torch.from_numpy(fx[f'f{i}_x']), sym=fx[f'f{i}_sym'], idx=fx[f'f{i}_idx'],
                              y=torch.from_numpy(fx[f'f{i}_y'])) for i in range(FORWARDS)])


def test_the_fixture_holds_the_cases_it_is_for():
    fix = _fixture()
    T = {_name(c, tag): [int(fix[_name(c, tag)][f'f{i}_T'][0]) for i in range(FORWARDS)] for c, tag, _ in CASES}
    print(T)
    assert T[_name(QAM, '')] == [4] * FORWARDS
    assert all(1 < t < 20 for t in T[_name(QPSK, '')]), 'the QPSK forwards stop before the cap'
    bad = fix[_name(QAM, 'naninf')]
    for i in range(FORWARDS):
        y = bad[f'f{i}_y'].reshape(QAM[3], -1)
        assert np.isnan(y[33]).all() and np.isinf(y[2, 7]) and np.isfinite(np.delete(y, [2, 33], axis=0)).all()
        assert not bad[f'f{i}_it_wfin'].all()
    for c, tag, _ in CASES:   # one record per (iteration, trial) and per (iteration, workgroup)
        fx = fix[_name(c, tag)]
        for i in range(FORWARDS):
            t = int(fx[f'f{i}_T'][0])
            assert fx[f'f{i}_it_wcrc'].shape == (t, c[3]) and fx[f'f{i}_it_inv'].shape == (t, 3)
            assert tuple(int(v) for v in fx[f'f{i}_made']) == ((1, 0), (0, 1), (0, 1))[i]


@pytest.mark.parametrize('case,tag,iters', CASES, ids=[_name(c, tag) for c, tag, _ in CASES])
def test_forward_and_dump_bits_equal_the_parent_commits(device, case, tag, iters):
    fx, inp = _inputs(_fixture(), case, tag)
    res = rec.run_case(case, inp, device, tail=True, iters=iters)
    bad = []
    for i, (made, got) in enumerate(res):
        assert made == ((1, 0), (0, 1), (0, 1))[i], (i, made)
        want = {k: fx[f'f{i}_{k}'] for k in FIELDS}
        print(f'forward {i}: T {int(got["T"][0])} (fixture {int(want["T"][0])}) nan_state {int(got["nan_state"][0])} '
              f'(fixture {int(want["nan_state"][0])})')
        bad += [f'forward {i} ({"building" if i == 0 else "reuse"}): {m}' for m in _diff(got, want)]
    assert not bad, '\n'.join(bad)


def test_a_forward_is_not_marked_by_the_one_before_it(device, monkeypatch):
    from vamp import VAMP
    fx, inp = _inputs(_fixture(), QAM, '')
    # forward B: another channel (another seed) at another SNR, on the same detector
    monkeypatch.setattr(rec, 'SEED', rec.SEED + 1)
    other = rec.make_inputs(QAM, ebn0=14.0, forwards=1)
    assert not np.array_equal(other['s'].numpy(), inp['s'].numpy())
    cfg = rec.config(*QAM, device='cuda', iterations=4)
    det = VAMP(cfg)
    chan_a = tuple(inp[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    chan_b = tuple(other[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    _, a0 = rec.dumped_forward(det, cfg, chan_a, inp['SNR'], inp['eps'][0], device, tail=True)
    _, b = rec.dumped_forward(det, cfg, chan_b, other['SNR'], other['eps'][0], device, tail=True)
    _, a1 = rec.dumped_forward(det, cfg, chan_a, inp['SNR'], inp['eps'][0], device, tail=True)
    assert _diff(b, a0, ('r', 'it_wcrc')), 'forward B is another forward'
    bad = [f'A again against A: {m}' for m in _diff(a1, a0)]
    bad += [f'A again against the fixture: {m}' for m in _diff(a1, {k: fx[f'f0_{k}'] for k in FIELDS})]
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('cap', [1, 20])
def test_a_reuse_forward_behind_a_forward_with_another_iteration_cap(device, monkeypatch, cap):
    """A reuse forward reads iteration 0's table, record and flag with no barrier of the loop ahead of the read
    (it has no r~ build at t = 0); the forward before it, from another detector with another iteration cap, on
    another channel at another SNR, leaves its own in the same LDS.  cap = 1 leaves iteration 0's flag value."""
    from vamp import VAMP
    fx, inp = _inputs(_fixture(), QAM, '')
    monkeypatch.setattr(rec, 'SEED', rec.SEED + 2)
    other = rec.make_inputs(QAM, ebn0=14.0, forwards=1)
    cfg = rec.config(*QAM, device='cuda', iterations=4)
    ocfg = rec.config(*QAM, device='cuda', iterations=cap)
    det, odet = VAMP(cfg), VAMP(ocfg)
    chan = tuple(inp[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    ochan = tuple(other[k].to(device).contiguous() for k in ('U', 's', 'Vh'))
    bad = []
    for i in range(FORWARDS):   # building, reuse, reuse: the other detector's forward ahead of each
        rec.forward(odet, ochan, other['SNR'], other['eps'][0], device)
        made, got = rec.dumped_forward(det, cfg, chan, inp['SNR'], inp['eps'][i], device, tail=True)
        assert made == ((1, 0), (0, 1), (0, 1))[i], (i, made)
        bad += [f'forward {i}: {m}' for m in _diff(got, {k: fx[f'f{i}_{k}'] for k in FIELDS})]
    assert not bad, '\n'.join(bad)


def _bad_rows():
    """float32 [16, 256, 2]: finite rows with +-inf, NaN and bf16-overflowing values: one lane's item alone (row 3),
    every lane of rows 1, 5, 9, 13, a NaN row (6), +inf and -inf residuals in one item (row 11), a bad row 0."""
    N, inf, nan, over = 256, np.float32(np.inf), np.float32(np.nan), np.float32(3.39e38)
    rng = np.random.default_rng(16)
    x = rng.standard_normal((rec.PBM, N, 2)).astype(np.float32)
    x[3, 72, 0], x[3, 73, 1], x[3, 75, 0], x[3, 74, 1] = inf, over, nan, -inf
    bad = np.array([inf, -inf, nan, over, -over], dtype=np.float32)
    for r in (0, 1, 5, 9, 13):
        x[r, :, 0] = bad[(np.arange(N) + r) % 5]
        x[r, ::3, 1] = bad[(np.arange(0, N, 3) + 2) % 5]
    x[6] = nan
    x[11, 16, 0], x[11, 17, 0], x[11, 18, 1] = over, -over, -over
    return x


@pytest.mark.parametrize('nrows', [16, 3])
def test_pack_and_store_halves_write_the_whole_items_planes(device, nrows):
    import ctypes as C
    import amp_native as nat
    x = torch.from_numpy(_bad_rows()[:nrows].copy()).to(device)
    whole = torch.zeros(4, 6, rec.PBM, 256, dtype=torch.int16, device=device)
    halves = torch.full((6, rec.PBM, 256), -1, dtype=torch.int16, device=device)
    st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    nat.check(nat.lib().amp_x3_planes_debug(C.c_void_p(x.data_ptr()), nrows, C.c_void_p(whole.data_ptr()), st), 'amp_x3_planes_debug')
    nat.check(nat.lib().amp_x3_pack_store_debug(C.c_void_p(x.data_ptr()), nrows, C.c_void_p(halves.data_ptr()), st),
              'amp_x3_pack_store_debug')
    torch.cuda.synchronize()
    want, got = whole[3].cpu().numpy().view(np.uint16), halves.cpu().numpy().view(np.uint16)
    assert (want[:, :nrows] != 0).any() and not want[:, nrows:].any(), 'form 3 wrote the valid rows, and zeros past them'
    ne = np.argwhere(got != want)
    assert ne.size == 0, f'{len(ne)} plane words differ; the first at [plane, row, column] {ne[0]}: {got[tuple(ne[0])]:#06x} != {want[tuple(ne[0])]:#06x}'
    for bad_nrows in (0, 17):
        assert nat.lib().amp_x3_pack_store_debug(C.c_void_p(x.data_ptr()), bad_nrows, C.c_void_p(halves.data_ptr()), None) != 0
