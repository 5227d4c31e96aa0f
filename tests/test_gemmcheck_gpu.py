"""gemmcheck on a real MI355X: the tile kernel's C element by element
against the exact product, the fold sink against the numpy reference and
against the store sink, clean-run accounting, exact attribution of an
injected fault, the child process and the CLI."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import gemm_nt
from kubegpu_amd.probe import gemmcheck as gc
from kubegpu_amd.probe.cucheck import cu_key

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (M, N, K in slabs): one tile and one slab (no pipeline); an odd slab count
# (both LDS stages and the drain); non-square, 6 tiles on 2 workgroups (a
# swapped bi / bj or pitch, the walk); 8 x 64 tiles (the super-block tile
# order instead of the row-major one)
SHAPES = [(128, 128, 1), (128, 256, 3), (384, 256, 2), (1024, 8192, 1)]


@functools.lru_cache(maxsize=None)
def case(dtype, m, n, slabs):
    """Shared, read-only: non-periodic operands in the probe's value ranges
    and their exact product."""
    k = slabs * gc.SLAB[dtype]
    rng = np.random.default_rng(1000 * m + n + slabs)
    lo, hi = (-16, 16) if dtype == "bf16" else (-128, 128)
    a = rng.integers(lo, hi, size=(m, k), dtype=np.int8)
    bt = rng.integers(lo, hi, size=(n, k), dtype=np.int8)
    want = torch.from_numpy(a).double() @ torch.from_numpy(bt).double().T
    return a, bt, want.numpy()


@pytest.mark.parametrize("blocks", [0, 2])
@pytest.mark.parametrize("m,n,slabs", SHAPES)
@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_gemm_nt_is_exact(dtype, m, n, slabs, blocks):
    a, bt, want = case(dtype, m, n, slabs)
    kind = torch.bfloat16 if dtype == "bf16" else torch.int8
    c = gemm_nt(torch.from_numpy(a).cuda().to(kind), torch.from_numpy(bt).cuda().to(kind), blocks)
    assert c.shape == (m, n) and c.dtype == (torch.float32 if dtype == "bf16" else torch.int32)
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


@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_store_sink_and_fold_sink_agree(dtype):
    m, n, k = 512, 256, 3 * gc.SLAB[dtype]
    c = gemm_nt(*gc.operands(5, dtype, m, n, k)).cpu().numpy()
    folds = gc.fold_tiles(gc.split_tiles(gc.tile_bits(dtype, c)))  # [4, 2, 4]
    want = gc.reference_expected(5, dtype, k)
    for bi in range(m // 128):
        for bj in range(n // 128):
            assert folds[bi, bj].tolist() == want[2 * (bi % 2) + bj % 2].tolist(), (bi, bj)


@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_clean_run_and_injected_fault(dtype):
    shape = dict(m=512, n=256, k=3 * gc.SLAB[dtype], rounds=3, blocks=3, dtypes=(dtype,))
    res = gc.gemmcheck(seed=0, **shape)
    assert res.ok and res.mismatches == 0 and res.records == [] and res.bad_cus == []
    assert res.first_bad_round is None and res.bad_stages == [] and res.records_dropped == 0
    assert len(res.waves_on) == 1024 and sum(res.waves_on) == res.waves == 3 * 4
    assert res.cu_count == torch.cuda.get_device_properties(0).multi_processor_count
    assert 1 <= res.cus_covered <= min(res.cu_count, res.waves)
    assert set(res.elapsed_s) == set(res.tflops) == {dtype}
    assert res.elapsed_s[dtype] > 0 and res.tflops[dtype] > 0

    # wave 6 = workgroup 1, quadrant 2; its first step of round 1 (8 tiles
    # a round, 3 workgroups) is t = 10: tile (1, 0) = 2, of class 2
    mask = 0x00100004
    res = gc.gemmcheck(seed=0, _inject=(dtype, 6, 1, mask), **shape)
    assert not res.ok and res.mismatches == 1 and res.records_dropped == 0
    assert res.first_bad_round == 1 and res.bad_stages == [dtype] and len(res.records) == 1
    rec = res.records[0]
    want = int(gc.reference_expected(0, dtype, shape["k"])[2, 2])
    assert gc.step_tile(10 % 8, 4, 2) == (1, 0)
    assert (rec["tile"], rec["quadrant"], rec["round"], rec["dtype"]) == (2, 2, 1, dtype)
    assert rec["expected"] == want and rec["got"] == want ^ mask
    assert res.waves_on[cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert res.bad_cus == [f"{rec['xcc']}/{rec['se']}/{rec['sh']}/{rec['cu']}"]
    assert sum(res.waves_on) == 12


def test_child_process_and_cli():
    rec = gc.run_gemmcheck_subprocess(0, rounds=2)
    assert rec["exit_code"] == 0 and rec["device"] == 0, rec
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--gemmcheck", "--rounds", "2"],
        capture_output=True, timeout=240, cwd=REPO, text=True)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    for rec in [rec] + list(json.loads(res.stdout).values()):
        assert rec["ok"] is True and rec["rounds"] == 2 and rec["mismatches"] == 0
        assert 1 <= rec["cus_covered"] <= rec["cu_count"]
        assert rec["tflops"]["bf16"] > 0 and rec["tflops"]["i8"] > 0
