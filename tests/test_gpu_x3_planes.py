"""The A-operand plane writers of the persistent VAMP engine through amp_x3_planes_debug (one
workgroup of eight waves, N = 256): the item forms of the eight-wave bf16x3 kernel
(x3_store8_item, x3_store_acc_item: no per-value finite test, one wave-uniform branch per item)
write the same bits as the shared writers (x3_store8, x3_store_acc), and all four equal the host
restatement of split3x2 in the planes' LDS order (tests/x3_split_ref.py).  A piece that is NaN is
compared as NaN: the sign and payload of a generated NaN are not part of the restatement.
"""
import ctypes as C

import numpy as np
import pytest

import x3_split_ref as ref

pytestmark = pytest.mark.gpu

N, PBM = 256, 16
INF, NAN = np.float32(np.inf), np.float32(np.nan)
OVER = np.float32(3.3961775292304601e38)   # finite, rounds to bf16 inf


def finite_rows(seed=3):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((PBM, N, 2)) * np.exp2(rng.integers(-12, 12, (PBM, N, 1)))).astype(np.float32)
    x[2, 5] = (0.0, -0.0)
    x[7, 100] = (1e-40, -1.4e-45)          # denormals
    x[9, 255] = (3.38e38, -3.39e38)        # the largest binade, finite in bf16
    return x


def one_lane():
    # one 8-column item of row 3 (one lane of wave 2 in the row-item map; columns 72-75 belong to
    # lanes of wave 2 alone in the accumulator map): every other wave stays on the fast path
    x = finite_rows()
    x[3, 72, 0] = INF
    x[3, 73, 1] = OVER
    x[3, 75, 0] = NAN
    x[3, 74, 1] = -INF
    return x


def every_lane():
    # rows 1, 5, 9, 13: every item of the row-item map's rows and every lane of the accumulator map
    # (rows 4 q ... 4 q + 3 per lane) holds a value that needs the mask or overflows
    x = finite_rows()
    bad = np.array([INF, -INF, NAN, OVER, -OVER], dtype=np.float32)
    for r in (1, 5, 9, 13):
        x[r, :, 0] = bad[(np.arange(N) + r) % 5]
        x[r, ::3, 1] = bad[(np.arange(0, N, 3) + 2) % 5]
    return x


def nan_row():
    x = finite_rows()
    x[6] = NAN
    return x


def opposite_overflows():
    # +inf and -inf residuals in one item: the item test's false positive (the masked form runs)
    x = finite_rows()
    x[11, 16, 0] = OVER
    x[11, 17, 0] = -OVER
    x[11, 18, 1] = -OVER
    return x


CASES = {
    'finite_16': (finite_rows, 16),
    'finite_1': (finite_rows, 1),
    'one_lane_16': (one_lane, 16),
    'every_lane_16': (every_lane, 16),
    'every_lane_1': (lambda: np.roll(every_lane(), -1, axis=0), 1),   # row 0 is a bad row
    'nan_row_16': (nan_row, 16),
    'opposite_overflows_16': (opposite_overflows, 16),
}


def run(device, rows, nrows):
    import torch
    import amp_native as nat
    x = torch.from_numpy(np.ascontiguousarray(rows[:nrows])).to(device)
    out = torch.zeros(4, 6, PBM, N, dtype=torch.int16, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    nat.check(nat.lib().amp_x3_planes_debug(C.c_void_p(x.data_ptr()), nrows, C.c_void_p(out.data_ptr()), C.c_void_p(st)),
              'amp_x3_planes_debug')
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint16)


@pytest.mark.parametrize('name', sorted(CASES))
def test_item_forms_write_the_shared_writers_bits(device, name):
    make, nrows = CASES[name]
    rows = make()
    got = run(device, rows, nrows)
    assert np.array_equal(got[0], got[1]), 'x3_store8_item != x3_store8'
    assert np.array_equal(got[2], got[3]), 'x3_store_acc_item != x3_store_acc'
    padded = rows.copy()
    padded[nrows:] = 0.0
    want = ref.canon(ref.planes_lds(padded))
    for form in range(4):
        assert np.array_equal(ref.canon(got[form]), want), form
    if name.startswith('finite'):
        assert np.array_equal(got[0], want) and np.array_equal(got[2], want)


def test_arguments_are_checked(device):
    import torch
    import amp_native as nat
    x = torch.zeros(PBM, N, 2, device=device)
    out = torch.zeros(4, 6, PBM, N, dtype=torch.int16, device=device)
    for nrows in (0, 17):
        assert nat.lib().amp_x3_planes_debug(C.c_void_p(x.data_ptr()), nrows, C.c_void_p(out.data_ptr()), None) != 0
    assert nat.lib().amp_x3_planes_debug(None, 1, C.c_void_p(out.data_ptr()), None) != 0
