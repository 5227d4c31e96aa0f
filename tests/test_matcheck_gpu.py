"""matcheck on a real MI355X: the accumulator tile of every form element
by element against the exact product (which proves the operand, scale,
index and C/D lane maps), every wave's digests against the numpy
reference, clean-run accounting, exact attribution of an injected fault,
the child process and the CLI."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import matcheck as mc
from kubegpu_amd.probe.cucheck import cu_key

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = [(s, f) for s in range(4) for f in range(len(mc.FORMS[s]))]


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = mc.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# both shapes, both format orders, op_sel 0, 1 and 3, one special round
@pytest.mark.parametrize("seed,r", [(0, 0), (0xDEADBEEF, 1), (0, 7)])
@pytest.mark.parametrize("stage,form", FORMS)
def test_wave_tile_equals_the_exact_product(stage, form, seed, r):
    got = mc.wave_tile(seed, stage, form, r)
    want = mc.tile_bits(stage, form, mc.matmul_tile(seed, stage, form, r))
    n = mc.tile_dim(stage, r)
    assert got.dtype == np.uint32 and got.shape == want.shape == (n, n)
    bad = got != want
    if bad.any():
        i, j = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(
            f"{mc.STAGES[stage]} / {mc.FORMS[stage][form]}: first wrong element at "
            f"(row {i}, col {j}): got {int(got[i, j]):08x}, want {int(want[i, j]):08x}; "
            f"{int(bad.sum())} of {bad.size} differ, wrong per row "
            f"{bad.sum(axis=1).tolist()}, per col {bad.sum(axis=0).tolist()}; "
            f"transposed tile matches: {bool(np.array_equal(got.T, want))}")


@pytest.mark.parametrize("blocks,rounds", [(1, 1), (3, 9), (0, 2)])
@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
def test_wave_digests_match_reference(seed, blocks, rounds):
    got = mc.wave_digests(seed, rounds, blocks)
    waves = (blocks or cu_count()) * 16
    assert got.dtype == np.uint32 and got.shape == (waves, rounds, 4)
    want = ref(seed, rounds)
    bad = got != want[None, :, :]
    if bad.any():
        w, r, s = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(
            f"first difference at wave {w}, round {r}, stage {mc.STAGES[s]}: "
            f"got {int(got[w, r, s]):08x}, want {int(want[r, s]):08x}; "
            f"{int(bad.sum())} of {bad.size} digests differ, per stage "
            f"{bad.sum(axis=(0, 1)).tolist()}")
    # the tile dump and the production kernel are the same stage code
    r = rounds - 1
    for stage in range(4):
        folded = sum(int(mc.fold_bits(mc.wave_tile(seed, stage, f, r)))
                     for f in range(len(mc.FORMS[stage]))) & 0xFFFFFFFF
        assert got[:, r, stage].tolist() == [folded] * waves, mc.STAGES[stage]


def test_clean_run_and_injected_fault():
    res = mc.matcheck(seed=0, rounds=3, blocks=3)
    assert res.ok and res.mismatches == 0 and res.records == []
    assert res.first_bad_round is None and res.bad_stages == [] and res.bad_cus == []
    assert res.records_dropped == 0 and len(res.waves_on) == 1024
    assert sum(res.waves_on) == res.waves == 48 and res.cu_count == cu_count()
    assert 1 <= res.cus_covered <= min(res.cu_count, res.waves)
    assert res.rounds == 3 and res.elapsed_s > 0

    mask = 0x00100004
    res = mc.matcheck(seed=0, rounds=3, blocks=3, _inject=(37, 1, 2, mask))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["mxfp6"]
    assert len(res.records) == 1 and res.records_dropped == 0
    rec = res.records[0]
    want = int(ref(0, 3)[1, 2])
    assert rec["wave"] == 37 and rec["block"] == 2
    assert rec["round"] == 1 and rec["stage"] == "mxfp6"
    assert rec["expected"] == want and rec["got"] == want ^ mask
    assert res.waves_on[cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert res.bad_cus == [f"{rec['xcc']}/{rec['se']}/{rec['sh']}/{rec['cu']}"]
    assert sum(res.waves_on) == 48


def test_child_process_and_cli():
    rec = mc.run_matcheck_subprocess(0, rounds=8)
    assert rec["exit_code"] == 0 and rec["device"] == 0, rec
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--matcheck", "--rounds", "8"],
        capture_output=True, timeout=240, cwd=REPO, text=True)
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    for rec in [rec] + list(json.loads(res.stdout).values()):
        assert rec["ok"] is True and rec["rounds"] == 8 and rec["mismatches"] == 0
        assert rec["waves"] == rec["cu_count"] * 16
        assert 1 <= rec["cus_covered"] <= rec["cu_count"]
