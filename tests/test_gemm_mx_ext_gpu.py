"""The e5m2, fp6 and mixed-format block-scaled GEMMs on a real MI355X:
gemm_mx_nt element by element against the float64 product of the dequantised
operands, the store sink against the numpy reference, a clean gemmcheck run,
exact attribution of an injected fault and the operand checks."""

import functools

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import gemm_mx_nt
from kubegpu_amd.probe import gemmcheck as gc

pytestmark = pytest.mark.gpu

# (M, N, K in slabs), test_gemm_mx_gpu.py's: no pipeline; an odd slab count
# (both LDS stages and the drain); non-square, the walk on 2 workgroups; the
# super-block tile order
SHAPES = [(128, 128, 1), (128, 256, 3), (384, 256, 2), (1024, 8192, 1)]


def codes(rng, fmt, shape):
    """Non-periodic random codes, exact at K <= 384: all 64 of e2m3 (3600
    sixty-fourths . 768 < 2**24), the probe's three-exponent window and zeros
    for e5m2 / e3m2, the e4m3 integers."""
    if fmt == "e4m3":
        return gc.e4m3_of_int(rng.integers(-16, 16, size=shape))
    if fmt in ("e5m2", "e3m2"):
        w = rng.integers(0, 256, size=shape)
        sign, keep, bias = (0x80, 0x83, 15) if fmt == "e5m2" else (0x20, 0x23, 3)
        f = (w >> 2) & 3
        return np.where(f == 3, w & sign, (w & keep) | ((bias + f) << 2)).astype(np.uint8)
    return rng.integers(0, 64, size=shape, dtype=np.uint8)  # e2m3


@functools.lru_cache(maxsize=None)
def case(dtype, m, n, slabs):
    """Shared, read-only: operands with scales in the probe's ranges (ra per
    row, cb per column, t per block) and their exact product."""
    k = slabs * gc.SLAB[dtype]
    fa, fb = gc.mx_formats(dtype)
    rng = np.random.default_rng(1000 * m + n + slabs)
    a, bt = codes(rng, fa, (m, k)), codes(rng, fb, (n, k))
    t = rng.integers(-8, 9, size=(1, k // 32))
    sa = (127 + rng.integers(-8, 8, size=(m, 1)) + t).astype(np.uint8)
    sb = (127 + rng.integers(-8, 8, size=(n, 1)) - t).astype(np.uint8)
    want = torch.from_numpy(gc.mx_dequantise(fa, a, sa)) @ \
        torch.from_numpy(gc.mx_dequantise(fb, bt, sb)).T
    return gc.mx_pack(fa, a), sa, gc.mx_pack(fb, bt), sb, want.numpy()


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("m,n,slabs", SHAPES)
@pytest.mark.parametrize("dtype", gc.MX_EXT_DTYPES)
def test_gemm_mx_nt_is_exact(dtype, m, n, slabs, blocks):
    *ops, want = case(dtype, m, n, slabs)
    c = gemm_mx_nt(*(torch.from_numpy(x).cuda() for x in ops), dtype, blocks)
    assert c.shape == (m, n) and c.dtype == torch.float32
    got = c.cpu().numpy().astype(np.float64)
    bad = got != want
    if bad.any():
        i, j = (int(x) for x in np.argwhere(bad)[0])
        rows, cols = bad.sum(axis=1), bad.sum(axis=0)
        pytest.fail(
            f"first wrong element at (row {i}, col {j}): got {got[i, j]}, want {want[i, j]}; "
            f"{int(bad.sum())} of {bad.size} differ; wrong rows {np.flatnonzero(rows)[:40].tolist()} "
            f"(counts {rows[rows > 0][:40].tolist()}), wrong cols "
            f"{np.flatnonzero(cols)[:40].tolist()} (counts {cols[cols > 0][:40].tolist()})")


@pytest.mark.parametrize("dtype", gc.MX_EXT_DTYPES)
def test_store_sink_folds_to_the_reference(dtype):
    m, n, k = 512, 256, 3 * gc.SLAB[dtype]
    c = gemm_mx_nt(*gc.mx_operands(5, dtype, m, n, k), dtype).cpu().numpy()
    folds = gc.fold_tiles(gc.split_tiles(gc.tile_bits(dtype, c)))  # [4, 2, 4]
    want = gc.reference_expected(5, dtype, k)
    for bi in range(m // 128):
        for bj in range(n // 128):
            assert folds[bi, bj].tolist() == want[2 * (bi % 2) + bj % 2].tolist(), (bi, bj)


@pytest.mark.parametrize("dtype", gc.MX_EXT_DTYPES)
def test_clean_run_and_injected_fault(dtype):
    shape = dict(m=512, n=256, k=3 * gc.SLAB[dtype], rounds=3, blocks=3, dtypes=(dtype,))
    res = gc.gemmcheck(seed=0, **shape)
    assert res.ok and res.mismatches == 0 and res.records == [] and res.bad_stages == []
    assert sum(res.waves_on) == res.waves == 3 * 4
    assert set(res.elapsed_s) == set(res.tflops) == {dtype} and res.tflops[dtype] > 0

    # wave 6 = workgroup 1, quadrant 2; its first step of round 1 (8 tiles
    # a round, 3 workgroups) is t = 10: tile (1, 0) = 2, of class 2
    mask = 0x00100004
    res = gc.gemmcheck(seed=0, _inject=(dtype, 6, 1, mask), **shape)
    assert not res.ok and res.mismatches == 1 and res.records_dropped == 0
    assert res.first_bad_round == 1 and res.bad_stages == [dtype] and len(res.records) == 1
    rec = res.records[0]
    want = int(gc.reference_expected(0, dtype, shape["k"])[2, 2])
    assert (rec["tile"], rec["quadrant"], rec["round"], rec["dtype"]) == (2, 2, 1, dtype)
    assert rec["expected"] == want and rec["got"] == want ^ mask


@pytest.mark.parametrize("dtype", gc.MX_EXT_DTYPES)
def test_operand_checks(dtype):
    fa, fb = gc.mx_formats(dtype)
    a, sa, bt, sb = gc.mx_operands(0, dtype, 128, 128, 2 * gc.SLAB[dtype])
    with pytest.raises(RuntimeError, match="a_scale must be"):
        gemm_mx_nt(a, sa[:, :-1].contiguous(), bt, sb, dtype)
    with pytest.raises(RuntimeError, match="bt_scale must be"):
        gemm_mx_nt(a, sa, bt, sb[:64].contiguous(), dtype)

    def cut(x):  # 1.5 slabs
        return x[:, :x.shape[1] * 3 // 4].contiguous()
    with pytest.raises(RuntimeError, match="K must be a positive multiple"):
        gemm_mx_nt(cut(a), cut(sa), cut(bt), cut(sb), dtype)
    if fb in ("e2m3", "e3m2"):
        # bt as wide as K elements of one byte each: not [N, 3K/4]
        wide = torch.zeros(128, 2 * gc.SLAB[dtype], dtype=torch.uint8, device=a.device)
        with pytest.raises(RuntimeError, match="but bt is"):
            gemm_mx_nt(a, sa, wide, sb, dtype)
    for fmt, x in ((fa, a), (fb, bt)):
        if fmt == "e5m2":  # float8_e5m2 tensors are accepted and mean the same
            y = x.view(torch.float8_e5m2)
            ops = (y, sa, bt, sb) if x is a else (a, sa, y, sb)
            assert torch.equal(gemm_mx_nt(*ops, dtype), gemm_mx_nt(a, sa, bt, sb, dtype))
    for name in ("mxfp6", "mxfp4:mxfp8", "mxfp8:mxfp4", dtype + ":"):
        with pytest.raises(RuntimeError, match="format must be"):
            gemm_mx_nt(a, sa, bt, sb, name)
