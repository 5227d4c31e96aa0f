"""gemmcheck's numpy reference on its own (no GPU): the expected folds
against a plain integer loop, the four tile classes, the exactness bound
of the operands and the verdict plumbing."""

import struct

import numpy as np
import pytest

from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.metrics import Metrics
from kubegpu_amd.probe import _active
from kubegpu_amd.probe import gemmcheck as gc

M32 = 0xFFFFFFFF


def fmix32(h):
    h ^= h >> 16
    h = h * 0x85EBCA6B & M32
    h ^= h >> 13
    h = h * 0xC2B2AE35 & M32
    return h ^ h >> 16


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("dtype", gc.DTYPES)
def test_reference_expected_equals_a_plain_integer_fold(dtype, seed):
    k = gc.SLAB[dtype]
    a, bt = gc.operand_block(seed, dtype, k)
    lo, hi = (-16, 15) if dtype == "bf16" else (-128, 127)
    assert a.shape == bt.shape == (256, k) and not np.array_equal(a[:128], a[128:])
    assert min(a.min(), bt.min()) == lo and max(a.max(), bt.max()) == hi
    c = a.astype(np.int64) @ bt.astype(np.int64).T
    want = [[0] * 4 for _ in range(4)]
    for i in range(256):
        for j in range(256):
            v = int(c[i, j])
            bits = v & M32 if dtype == "i8" else \
                struct.unpack("<I", struct.pack("<f", float(v)))[0] if v else 0
            ti, tj = i % 128, j % 128
            q = 2 * (ti // 64) + tj // 64
            salt = (128 * ti + tj + 1) * 0x9E3779B9 & M32
            cls = 2 * (i // 128) + j // 128
            want[cls][q] = (want[cls][q] + fmix32(bits + salt & M32)) & M32
    got = gc.reference_expected(seed, dtype, k)
    assert got.dtype == np.uint32 and got.tolist() == want
    # a workgroup that reads the wrong row or column block is seen
    assert len({tuple(row) for row in want}) == 4


def test_partial_sums_stay_exact_at_the_k_limits():
    # from the value ranges: |a b| <= 16 . 16 and 128 . 128
    assert 16 * 16 * gc.MAX_K["bf16"] <= 2 ** 23 < 2 ** 24
    assert 128 * 128 * gc.MAX_K["i8"] < 2 ** 31
    for dtype in gc.DTYPES:
        assert gc.MAX_K[dtype] % gc.SLAB[dtype] in (0, gc.SLAB[dtype] - 1)
        with pytest.raises(ValueError):
            gc.operand_block(0, dtype, gc.MAX_K[dtype] + gc.SLAB[dtype])


@pytest.mark.parametrize("tm,tn", [(1, 1), (3, 2), (8, 8), (8, 64), (16, 32)])
def test_step_tile_is_a_bijection(tm, tn):
    tiles = [gc.step_tile(u, tm, tn) for u in range(tm * tn)]
    assert sorted(tiles) == [(i, j) for i in range(tm) for j in range(tn)]
    if (tm, tn) == (8, 64):  # 64 consecutive steps of one XCD share 8 + 8 panels
        mine = [tiles[8 * v + 5] for v in range(64)]
        assert len({i for i, _ in mine}) == 8 and len({j for _, j in mine}) == 8


def test_verdict_plumbing():
    assert _active.LOAD_PROBES[-1] == "gemmcheck"
    assert _active.LOAD_PROBES[:-1] == _active.CHECK_PROBES
    assert _active.CHECK_PROBES[-1] == "matcheck" and len(_active.CHECK_PROBES) == 12
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    uuid = sorted(mgr.gpus)[0]
    assert mgr.gemmcheck_status(uuid) is None and mgr.device_health()[uuid]
    good = gc.GemmcheckResult(m=256, n=256, k=128, rounds=4).to_dict()
    mgr.record_gemmcheck(uuid, good)
    assert mgr.gemmcheck_status(uuid)["ok"] and mgr.device_health()[uuid]
    mgr.record_gemmcheck(uuid, dict(good, ok=False, mismatches=3, first_bad_round=1,
                                    bad_stages=["i8"]))
    assert not mgr.device_health()[uuid]
    assert mgr.clear_gemmcheck(uuid) and mgr.device_health()[uuid]
    metrics = Metrics()
    metrics.set_gpu_gemmcheck(uuid, 3, 256, 1.0)
    metrics.inc_gemmcheck_error(uuid)
    assert metrics.gpu_gemmcheck[uuid]["mismatches"] == 3
    assert metrics.gpu_gemmcheck_errors[uuid] == 1
