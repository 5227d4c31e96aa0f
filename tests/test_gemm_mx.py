"""gemmcheck's MX stages in numpy alone (no GPU): the expected folds against
a product computed from an independent decode, and the exactness bounds."""

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import gemmcheck as gc

# OCP e2m1 magnitudes, codes 0..7; bit 3 is the sign
E2M1_MAG = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def decode(dtype, codes, scales):
    """float64 values of element codes [rows, k] and E8M0 scales [rows, k / 32]."""
    if dtype == "mxfp8":
        vals = torch.from_numpy(codes.copy()).view(torch.float8_e4m3fn).double().numpy()
    else:
        vals = np.array(E2M1_MAG)[codes & 7] * np.where(codes & 8, -1.0, 1.0)
    out = np.empty_like(vals)
    for b in range(scales.shape[1]):
        out[:, 32 * b:32 * b + 32] = vals[:, 32 * b:32 * b + 32] * 2.0 ** (
            scales[:, b:b + 1].astype(np.int64) - 127)
    return out


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("dtype", gc.MX_DTYPES)
def test_reference_expected_equals_a_fold_of_an_independent_decode(dtype, seed):
    k = 2 * gc.SLAB[dtype]
    a, sa, bt, sb = gc.mx_operand_block(seed, dtype, k)
    assert a.shape == bt.shape == (256, k) and sa.shape == sb.shape == (256, k // 32)
    assert all(x.dtype == np.uint8 for x in (a, sa, bt, sb))
    if dtype == "mxfp8":  # the integers -16..15, no NaN code
        va = decode(dtype, a, np.full_like(sa, 127))
        assert va.min() == -16 and va.max() == 15 and np.array_equal(va, np.rint(va))
    else:  # every nibble
        assert set(np.unique(a)) == set(np.unique(bt)) == set(range(16))
    # SA + SB = 254 + ra + cb in every block, ra and cb in -8..7, t in -8..8, no 0xFF
    both = sa.astype(int)[:, None, :] + sb.astype(int)[None, :, :]
    assert (both == both[:, :, :1]).all() and both.min() >= 254 - 16 and both.max() <= 254 + 14
    assert 127 - 16 <= min(sa.min(), sb.min()) and max(sa.max(), sb.max()) <= 127 + 16
    assert len(np.unique(sa[0])) > 1 and len(np.unique(sa[:, 0])) > 1
    c = decode(dtype, a, sa) @ decode(dtype, bt, sb).T
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    want = gc.fold_tiles(gc.split_tiles(gc.tile_bits(dtype, c))).reshape(4, 4)
    got = gc.reference_expected(seed, dtype, k)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert len({tuple(row) for row in got.tolist()}) == 4
    # the packing gemm_mx_nt reads: element 2b is the low nibble of byte b
    packed = gc.mx_pack(dtype, a)
    if dtype == "mxfp4":
        assert np.array_equal(packed & 15, a[:, 0::2]) and np.array_equal(packed >> 4, a[:, 1::2])
    else:
        assert np.array_equal(packed, a)


def test_mx_partial_sums_stay_exact_at_the_k_limits():
    # in units of the product scale: |a b| <= 16 . 16, and 6 . 6 = 144 quarters
    assert 16 * 16 * gc.MAX_K["mxfp8"] <= 2 ** 23 < 2 ** 24
    assert int(4 * max(E2M1_MAG) ** 2) == 144 and 144 * gc.MAX_K["mxfp4"] < 2 ** 24
    for dtype in gc.MX_DTYPES:
        assert gc.MAX_K[dtype] % gc.SLAB[dtype] == 0 and gc.SLAB[dtype] % 32 == 0
        with pytest.raises(ValueError):
            gc.mx_operand_block(0, dtype, gc.MAX_K[dtype] + gc.SLAB[dtype])
    assert gc.DTYPES == ("bf16", "i8") and not set(gc.DTYPES) & set(gc.MX_DTYPES)
