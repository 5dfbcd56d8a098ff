"""The bf16x3 split without per-value selects (csrc/amp_persist.h split3x2_raw, x3_item_masked),
restated on the host (tests/x3_split_ref.py):
  * the unmasked first residual x - bf16(x) is NaN exactly when x is non-finite;
  * the item test (the NaN-ness of the packed sum of an item's residuals) fires whenever a value
    of the item needs split3x2's mask;
  * the item form (raw pieces, or the masked ones for the whole item when the test fires) and
    split3x2 agree bit for bit, wherever the non-finite value stands in the item.
"""
import numpy as np
import torch

import x3_split_ref as ref

F32_MAX = float(np.finfo(np.float32).max)
BF16_MAX = 3.3895313892515355e38          # 0x7f7f
# finite float32 values that round to bf16 inf: from the midpoint of bf16 max and 2^128 up
OVERFLOW = [3.3961775292304601e38, 3.4e38, F32_MAX]
NONFINITE = [float('inf'), float('-inf'), float('nan')]


def finite_values():
    rng = np.random.default_rng(5)
    v = []
    for e in list(range(-20, 21)) + [-126, -100, -60, 60, 100, 126]:   # well over 30 binades
        v += list(np.ldexp(rng.uniform(1.0, 2.0, 24) * rng.choice([-1.0, 1.0], 24), e))
    v += [0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.17549435e-38, 1.0, -1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -9,
          1.0 + 2.0 ** -16, 1.0 + 2.0 ** -23, BF16_MAX, -BF16_MAX, 3.39e38, -3.39e38]
    v += OVERFLOW + [-x for x in OVERFLOW]
    return torch.tensor(v, dtype=torch.float32)


def same_bits(a, b):
    return np.array_equal(ref.bits16(a), ref.bits16(b))


def test_overflow_values_round_to_bf16_inf():
    x = torch.tensor(OVERFLOW + [-v for v in OVERFLOW], dtype=torch.float32)
    assert torch.isfinite(x).all() and torch.isinf(ref.bf16(x)).all()
    assert torch.isfinite(ref.bf16(torch.tensor([BF16_MAX, 3.39e38], dtype=torch.float32))).all()


def test_unmasked_residual_is_nan_exactly_for_nonfinite():
    x = torch.cat([finite_values(), torch.tensor(NONFINITE, dtype=torch.float32)])
    r1 = ref.split_raw(x)[3]
    assert torch.equal(torch.isnan(r1), ~torch.isfinite(x))
    # the overflow case: the residual is -+inf, which the masked form keeps too
    ov = torch.tensor(OVERFLOW, dtype=torch.float32)
    assert torch.equal(ref.split_raw(ov)[3], torch.full_like(ov, float('-inf')))
    assert torch.equal(ref.split_masked(ov)[3], torch.full_like(ov, float('-inf')))


def test_raw_pieces_of_finite_values_are_the_masked_ones():
    x = finite_values()
    raw, msk = ref.split_raw(x), ref.split_masked(x)
    for i in range(3):
        assert same_bits(raw[i], msk[i]), i
    # three pieces carry 24 bits: the split is exact away from the denormal and overflow ends
    ok = (x.abs() > 1e-30) & (x.abs() < 1e38)
    assert torch.equal((raw[0] + raw[1] + raw[2])[ok], x[ok])


def items(pairs):
    """Items of `pairs` packed registers of finite values drawn from finite_values() (overflow values among them)."""
    v = finite_values()
    g = torch.Generator().manual_seed(11)
    n = 64
    return v[torch.randint(0, v.numel(), (n, pairs, 2), generator=g)]


def test_item_test_fires_whenever_a_value_needs_the_mask():
    for pairs in (4, 8):            # x3_store_acc_item: 4 registers per item, x3_store8_item: 8
        base = items(pairs)
        assert not ref.item_fires(ref.split_raw(base[:, :, :])[3])[
            ~torch.isinf(ref.bf16(base)).flatten(1).any(1)].any()   # no overflow value: never fires
        for bad in NONFINITE:
            for p in range(pairs):
                for h in range(2):
                    x = base.clone()
                    x[:, p, h] = bad
                    assert ref.item_fires(ref.split_raw(x)[3]).all(), (bad, p, h)


def test_item_form_equals_split3x2_bit_for_bit():
    for pairs in (4, 8):
        base = items(pairs)
        cases = [base]
        for bad in NONFINITE + OVERFLOW[:1]:
            for p in range(pairs):
                for h in range(2):
                    x = base.clone()
                    x[:, p, h] = bad
                    cases.append(x)
        # opposite overflows in one item: +inf and -inf residuals meet, a false positive of the test
        x = base.clone()
        x[:, 0, 0] = OVERFLOW[0]
        x[:, pairs - 1, 0] = -OVERFLOW[0]
        cases.append(x)
        assert ref.item_fires(ref.split_raw(x)[3]).all()
        for x in cases:
            got, _ = ref.split_item(x)
            want = ref.split_masked(x)
            for i in range(3):
                assert same_bits(got[i], want[i]), i
