"""matcheck's numpy reference on its own (no GPU): every tile is exact in
float32, the operand recipes reach the codes, scales, op_sel bytes and
index pairs they promise, and the verdict plumbing."""

import numpy as np
import pytest

from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.probe import _active
from kubegpu_amd.probe import matcheck as mc

FORMS = [(s, f) for s in range(4) for f in range(len(mc.FORMS[s]))]


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("stage,form", FORMS)
def test_tiles_are_exact(stage, form, seed):
    for r in range(32):
        tile = mc.matmul_tile(seed, stage, form, r)
        n = mc.tile_dim(stage, r)
        assert tile.dtype == np.float64 and tile.shape == (n, n)
        fin = np.isfinite(tile)
        assert fin.all() or (stage == 1 and r % 8 == 7), (r, int((~fin).sum()))
        if stage == 1 and r % 8 == 7:
            assert np.isnan(tile).any() and np.isinf(tile).any(), r
        with np.errstate(over="ignore"):
            back = tile[fin].astype(np.float32).astype(np.float64)
        assert np.array_equal(back, tile[fin]), r
        q = tile[fin] / mc.tile_unit(seed, stage, form, r)[fin]
        assert np.array_equal(q, np.rint(q)) and np.abs(q).max() < 2 ** 24, r


def test_coverage_over_364_rounds():
    fed = {f: set() for f in range(5)}
    scales, pairs = set(), set()
    for k in range(4):  # rounds that share r & 3 go through numpy together
        r = np.arange(k, 364, 4, dtype=np.uint32)
        for stage, form in FORMS:
            if stage in (1, 2):
                fa, fb, ca, cb, sa, sb = mc.codes(0, stage, form, r)
                fed[fa] |= set(np.unique(ca).tolist())
                fed[fb] |= set(np.unique(cb).tolist())
                if stage == 1:
                    scales |= set(np.unique(sa).tolist()) | set(np.unique(sb).tolist())
    for form in range(4):
        pairs |= set(np.unique(mc.sparse_pairs(0, form, np.arange(8, dtype=np.uint32))).tolist())
    finite = {f: {c for c in range(256) if np.isfinite(t[c])}
              for f, t in ((mc.FMT_E4M3, mc.E4M3), (mc.FMT_E5M2, mc.E5M2))}
    assert fed[mc.FMT_E4M3] >= finite[mc.FMT_E4M3] and fed[mc.FMT_E5M2] >= finite[mc.FMT_E5M2]
    assert fed[mc.FMT_E2M3] == fed[mc.FMT_E3M2] == set(range(64))
    assert min(scales) <= 40 and max(scales - {255}) >= 214 and 255 in scales
    assert {mc.op_sel(r) for r in range(364)} == {0, 1, 2, 3}
    assert pairs == set(range(6)) and len(set(mc.PAIRS)) == 6
    assert all(0 <= i0 < i1 <= 3 for i0, i1 in mc.PAIRS)


def test_verdict_plumbing():
    assert _active.CHECK_PROBES[-1] == "matcheck"
    assert _active.CHECK_PROBES[:-1] == _active.VERDICT_PROBES
    assert len(set(_active.CHECK_PROBES)) == len(_active.CHECK_PROBES)
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    uuid = sorted(mgr.gpus)[0]
    assert mgr.matcheck_status(uuid) is None and mgr.device_health()[uuid]
    good = mc.MatcheckResult(rounds=4).to_dict()
    mgr.record_matcheck(uuid, good)
    assert mgr.matcheck_status(uuid)["ok"] and mgr.device_health()[uuid]
    mgr.record_matcheck(uuid, dict(good, ok=False, mismatches=3, first_bad_round=1,
                                   bad_stages=["sparse"]))
    assert not mgr.device_health()[uuid]
    assert mgr.clear_matcheck(uuid) and mgr.device_health()[uuid]
