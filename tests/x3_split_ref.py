"""Host restatement of the bf16x3 A-operand split (csrc/amp_persist.h): split3x2 (per-value finite
test), split3x2_raw (none), the item test x3_item_masked and the plane layout of x3_store8 /
x3_store_acc.  float32 arithmetic with torch.bfloat16's round-to-nearest-even conversion, which
is v_cvt_pk_bf16_f32's; shared by tests/test_x3_split_cpu.py and tests/test_gpu_x3_planes.py.
"""
import numpy as np
import torch


def bf16(x):
    """float32 -> bf16 (RNE) -> float32."""
    return x.to(torch.bfloat16).to(torch.float32)


def bits16(x):
    """The bf16 piece of a float32 tensor that holds a bf16 value, as uint16 (numpy)."""
    return (x.contiguous().view(torch.int32).numpy().view(np.uint32) >> 16).astype(np.uint16)


def split_masked(x):
    """split3x2: (b0, b1, b2, r1); a non-finite x keeps b0 = x and zero residuals."""
    b0 = bf16(x)
    r1 = torch.where(torch.isfinite(x), x - b0, torch.zeros_like(x))
    b1 = bf16(r1)
    r2 = r1 - b1
    return b0, b1, bf16(r2), r1


def split_raw(x):
    """split3x2_raw: the same pieces with no finite test; r1 is the unmasked first residual."""
    b0 = bf16(x)
    r1 = x - b0
    b1 = bf16(r1)
    r2 = r1 - b1
    return b0, b1, bf16(r2), r1


def item_fires(r1_items):
    """x3_item_masked per item: r1_items [..., pairs, 2] unmasked residuals in the kernel's order
    (pair p = one packed register, summed pair by pair, then low + high); True where the sum is NaN."""
    s = r1_items[..., 0, :].clone()
    for p in range(1, r1_items.shape[-2]):
        s = s + r1_items[..., p, :]
    t = s[..., 0] + s[..., 1]
    return t != t


def split_item(x_items):
    """The item form: x_items [..., pairs, 2]; raw pieces unless the item's test fires, then masked."""
    raw, msk = split_raw(x_items), split_masked(x_items)
    fire = item_fires(raw[3])[..., None, None]
    return tuple(torch.where(fire, m, r) for r, m in zip(raw[:3], msk[:3])), fire[..., 0, 0]


def canon(p):
    """uint16 bf16 pieces with every NaN mapped to 0x7fc0: the sign and payload of a generated NaN
    (inf - inf) are the processor's default NaN, not part of the restatement."""
    p = np.array(p, dtype=np.uint16, copy=True)
    p[((p & 0x7f80) == 0x7f80) & ((p & 0x7f) != 0)] = 0x7fc0
    return p


def planes_lds(rows):
    """rows: float32 [16, N, 2] -> the six planes uint16 [6, 16, N] in LDS order (Re x0 x1 x2,
    Im x0 x1 x2; element j of row r at column j ^ 8 (r & m), csrc/amp_persist.h pl_col)."""
    x = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32))
    N = x.shape[1]
    n = N >> 3
    m = min(n & -n, 16) - 1
    out = np.zeros((6, 16, N), dtype=np.uint16)
    j = np.arange(N)
    for c in range(2):
        b = split_masked(x[..., c].contiguous())
        for i in range(3):
            p = bits16(b[i])
            for r in range(16):
                out[3 * c + i, r, j ^ (8 * (r & m))] = p[r]
    return out
