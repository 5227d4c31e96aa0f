"""gemmcheck's further MX stages (e5m2, fp6, mixed formats) in numpy alone
(no GPU): the expected folds against a product computed from an independent
decode, the fp6 packing, the codes that occur and the exactness bounds."""

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import gemmcheck as gc


def fp6(code, ebits, bias):
    """OCP fp6 value of one code: sign, ebits of exponent, the rest mantissa."""
    mbits = 5 - ebits
    e, m = (code >> mbits) & ((1 << ebits) - 1), code & ((1 << mbits) - 1)
    mag = m * 2.0 ** (1 - bias - mbits) if e == 0 else (1 + m / 2.0 ** mbits) * 2.0 ** (e - bias)
    return -mag if code & 32 else mag


TABLES = {"e2m3": np.array([fp6(c, 2, 1) for c in range(64)]),
          "e3m2": np.array([fp6(c, 3, 3) for c in range(64)])}
FP8 = {"e4m3": torch.float8_e4m3fn, "e5m2": torch.float8_e5m2}
# (largest |a b| in units of `unit`, unit) per stage, the issue's bounds
BOUNDS = {"mxfp8_e5m2": (784, 16), "mxfp6_e2m3": (900, 64), "mxfp6_e3m2": (784, 16),
          "mxfp8_e5m2:mxfp8": (448, 4)}


def allowed_codes(fmt):
    """Every code the rule of the module docstring can make."""
    w = np.arange(256)
    if fmt == "e4m3":
        return set(gc.e4m3_of_int(np.arange(-16, 16)).tolist())
    if fmt == "e2m3":
        return set(np.where((w >> 3) & 3 == 3, w & 0x27, w & 0x3F).tolist())
    sign, keep, bias = (0x80, 0x83, 15) if fmt == "e5m2" else (0x20, 0x23, 3)
    f = (w >> 2) & 3
    return set(np.where(f == 3, w & sign, (w & keep) | ((bias + f) << 2)).tolist())


def decode(fmt, codes, scales):
    """float64 values of element codes [rows, k] and E8M0 scales [rows, k / 32]."""
    if fmt in FP8:
        vals = torch.from_numpy(codes.copy()).view(FP8[fmt]).double().numpy()
    else:
        vals = TABLES[fmt][codes]
    return vals * 2.0 ** (np.repeat(scales.astype(np.int64), 32, axis=1) - 127)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("dtype", gc.MX_EXT_DTYPES)
def test_reference_expected_equals_a_fold_of_an_independent_decode(dtype, seed):
    k = 2 * gc.SLAB[dtype]
    fa, fb = gc.mx_formats(dtype)
    a, sa, bt, sb = gc.mx_operand_block(seed, dtype, k)
    assert a.shape == bt.shape == (256, k) and sa.shape == sb.shape == (256, k // 32)
    assert all(x.dtype == np.uint8 for x in (a, sa, bt, sb))
    assert set(np.unique(a)) == allowed_codes(fa) and set(np.unique(bt)) == allowed_codes(fb)
    both = sa.astype(int)[:, None, :] + sb.astype(int)[None, :, :]
    assert (both == both[:, :, :1]).all() and max(sa.max(), sb.max()) <= 127 + 16
    va, vb = decode(fa, a, np.full_like(sa, 127)), decode(fb, bt, np.full_like(sb, 127))
    most, unit = BOUNDS[dtype]
    assert np.abs(va).max() * np.abs(vb).max() * unit == most
    assert np.array_equal(np.rint(va * vb * unit), va * vb * unit)
    c = decode(fa, a, sa) @ decode(fb, bt, sb).T
    assert np.array_equal(c.astype(np.float32).astype(np.float64), c)
    want = gc.fold_tiles(gc.split_tiles(gc.tile_bits(dtype, c))).reshape(4, 4)
    got = gc.reference_expected(seed, dtype, k)
    assert got.dtype == np.uint32 and got.tolist() == want.tolist()
    assert len({tuple(row) for row in got.tolist()}) == 4
    for fmt, codes in ((fa, a), (fb, bt)):
        packed = gc.mx_pack(fmt, codes)
        if fmt in TABLES:  # element e: bits 6e..6e+5 of each 24-byte block
            assert packed.shape == (256, 3 * k // 4) and packed.dtype == np.uint8
            for row in (0, 255):
                for blk in (0, k // 32 - 1):
                    word = int.from_bytes(packed[row, 24 * blk:24 * blk + 24].tobytes(), "little")
                    assert [(word >> (6 * e)) & 63 for e in range(32)] == \
                        codes[row, 32 * blk:32 * blk + 32].tolist()
        else:
            assert np.array_equal(packed, codes)


def test_partial_sums_stay_exact_at_the_k_limits():
    for dtype in gc.MX_EXT_DTYPES:
        assert BOUNDS[dtype][0] * gc.MAX_K[dtype] < 2 ** 24
        assert gc.MAX_K[dtype] == (16384 if BOUNDS[dtype][1] >= 16 else 32768)
        assert gc.SLAB[dtype] == 128 and gc.MAX_K[dtype] % 128 == 0
        with pytest.raises(ValueError):
            gc.mx_operand_block(0, dtype, gc.MAX_K[dtype] + gc.SLAB[dtype])
    assert gc.DTYPES == ("bf16", "i8") and gc.MX_DTYPES == ("mxfp8", "mxfp4")
    assert gc._STAGES == gc.DTYPES + gc.MX_DTYPES + gc.MX_EXT_DTYPES and len(gc._STAGES) == 8
