"""Vector-memory kernel on a real MI355X: every wave's digests against the
numpy reference (period wrap included), every value of the lowest and the
highest wave of a workgroup against it element for element (which names
the access that disagrees), the default grid, repeatability, exact
attribution of an injected fault, a tampered table, argument checks, the
tables of both sides, the CLI child, and a guard round the arena that
shows that dropped stores were dropped and nothing strayed."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import vmemcheck as vm

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = vm.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def table(seed=0):
    return torch.from_numpy(vm.source_table(seed).view(np.int32).copy()).cuda()


def arena(blocks):
    return torch.zeros(blocks * 16 * vm.SPAN_DWORDS, dtype=torch.int32, device="cuda")


# 1. digests ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_equal_the_reference(seed):
    got = vm.wave_digests(seed, rounds=3, blocks=2)
    assert got.shape == (32, 3, 4) and got.dtype == np.uint32
    bad = np.argwhere(got != ref(seed, 3)[None])
    assert len(bad) == 0, [(int(w), int(r), vm.STAGES[s]) for w, r, s in bad[:8]]


def test_wave_digests_across_the_period_wrap():
    rounds = vm.PERIOD + 1
    got = vm.wave_digests(0, rounds, blocks=1)
    assert np.array_equal(got, np.broadcast_to(ref(0, rounds), (16, rounds, 4)))
    assert np.array_equal(got[:, vm.PERIOD], got[:, 0])


# 2. every value ----------------------------------------------------------------------------

@pytest.mark.parametrize("wave", (0, 15))
@pytest.mark.parametrize("r", (0, 1))
@pytest.mark.parametrize("stage", range(4))
def test_wave_values_equal_the_reference(stage, r, wave):
    got = vm.wave_values(0, stage, r, wave=wave)
    want = vm.reference_values(0, stage, r)
    assert list(got) == list(want) == vm.slot_table(stage)
    failures = []
    for n, name in enumerate(want):
        g, w = got[name], want[name]
        if not np.array_equal(g, w):
            lanes = np.flatnonzero(g != w)
            failures.append((n, name, [(int(i), hex(int(g[i])), hex(int(w[i])))
                                       for i in lanes[:4]]))
    assert not failures, failures[:4]


# 3. whole-GPU run ------------------------------------------------------------------------------

def test_default_grid_is_clean_and_repeatable():
    for _ in range(2):
        res = vm.vmemcheck(rounds=2)
        assert res.ok and res.mismatches == 0, res.to_dict()
        assert res.waves == 16 * cu_count() == 16 * res.cu_count
        assert 1 <= res.cus_covered <= res.cu_count
        assert res.records == [] and res.bad_cus == [] and res.bad_stages == []
        assert res.first_bad_round is None and res.rounds == 2
        assert res.elapsed_s > 0
        assert min(res.width_gbps, res.gather_gbps, res.partial_gbps, res.buffer_gbps) > 0
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d


# 4. test hooks ---------------------------------------------------------------------------------

def test_injected_digest_fault_is_attributed_exactly():
    res = vm.vmemcheck(seed=0, rounds=3, blocks=2, _inject=(17, 1, 2, 0x10))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["partial"]
    (rec,) = res.records
    assert rec["wave"] == 17 and rec["block"] == 1
    assert rec["round"] == 1 and rec["stage"] == "partial"
    assert rec["expected"] ^ rec["got"] == 0x10
    assert rec["expected"] == int(ref(0, 3)[1, 2])


def test_a_tampered_table_fails_every_wave_in_that_round():
    want = ref(0, 3).copy()
    want[1, 3] ^= 1
    res = vm.vmemcheck(seed=0, rounds=3, blocks=2, max_records=64, _expected=want)
    assert not res.ok and res.mismatches == 32
    assert res.first_bad_round == 1 and res.bad_stages == ["buffer"]
    assert sorted(r["wave"] for r in res.records) == list(range(32))
    assert all(r["round"] == 1 and r["stage"] == "buffer" for r in res.records)


# 5. arguments ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs", [
    dict(rounds=0), dict(rounds=65537), dict(blocks=4097), dict(seed=1 << 32),
    dict(rounds=2, blocks=2, _inject=(32, 0, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 2, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 0, 4, 1)),
    dict(rounds=2, blocks=2, _expected=np.zeros((3, 4), dtype=np.uint32)),
])
def test_bad_arguments_raise_before_any_launch(kwargs):
    with pytest.raises((ValueError, RuntimeError), match="vmemcheck"):
        vm.vmemcheck(**kwargs)


def test_the_extension_checks_its_own_arguments_and_holds_the_same_tables():
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    expected = torch.from_numpy(ref(0, 2).view(np.int32).copy()).cuda()
    x, a2, a1 = table(), arena(2), arena(1)
    with pytest.raises(RuntimeError, match="vmemcheck: rounds"):
        ext.vmemcheck_run(expected, 0, 0, 2, a2, x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: expected must hold"):
        ext.vmemcheck_run(expected, 0, 3, 2, a2, x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: inject"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2, x, 0, None, (0, 0, 4, 1))
    # an arena or a table of the wrong size, dtype or device
    with pytest.raises(RuntimeError, match="vmemcheck: arena must hold"):
        ext.vmemcheck_run(expected, 0, 2, 2, a1, x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: arena must hold"):
        ext.vmemcheck_run(expected, 0, 2, 2, arena(3), x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: arena must be a contiguous int32"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2.to(torch.int64), x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: arena must be a contiguous int32"):
        ext.vmemcheck_run(expected, 0, 2, 2, arena(4)[::2], x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: arena must be on the GPU"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2.cpu(), x, 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: table must hold"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2, x[:-1].contiguous(), 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: table must be a contiguous int32"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2, x.to(torch.int64), 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: table must be on the GPU"):
        ext.vmemcheck_run(expected, 0, 2, 2, a2, x.cpu(), 0, None, None)
    with pytest.raises(RuntimeError, match="vmemcheck: arena must hold"):
        ext.vmemcheck_values(0, 0, 0, a2, x, 0)
    with pytest.raises(RuntimeError, match="vmemcheck: table must hold"):
        ext.vmemcheck_values(0, 0, 0, a1, x[:-1].contiguous(), 0)
    with pytest.raises(RuntimeError, match="vmemcheck: table must be on the GPU"):
        ext.vmemcheck_values(0, 0, 0, a1, x.cpu(), 0)
    with pytest.raises(RuntimeError, match="vmemcheck: stage"):
        ext.vmemcheck_values(0, 4, 0, a1, x, 0)
    with pytest.raises(RuntimeError, match="vmemcheck: seed"):
        ext.vmemcheck_values(1 << 32, 0, 0, a1, x, 0)
    with pytest.raises(RuntimeError, match="vmemcheck: wave"):
        ext.vmemcheck_values(0, 0, 0, a1, x, 16)
    period, rows, sizes, gather, buffer = ext.vmemcheck_layout()
    assert (period, rows) == (vm.PERIOD, vm._VALUE_ROWS)
    assert tuple(sizes) == (vm.SPAN_DWORDS, *vm.REGIONS["width"], *vm.REGIONS["partial"],
                            *vm.REGIONS["buffer"], vm.X_DWORDS, vm.BUFFER_CELLS, vm.BUFFER_IMM)
    assert tuple(gather) == vm.GATHER_STRIDES and tuple(buffer) == vm.BUFFER_STRIDES


# 6. nothing strays -------------------------------------------------------------------------------

def test_no_store_leaves_the_regions_and_dropped_stores_are_dropped():
    sentinel = 0x5EA7BEEF
    blocks, guard = 2, 4096
    n = blocks * 16 * vm.SPAN_DWORDS
    whole = torch.full((guard + n + guard,), sentinel, dtype=torch.int32, device="cuda")
    middle = whole[guard:guard + n]
    assert middle.is_contiguous()
    res = vm.vmemcheck(seed=0, rounds=3, blocks=blocks, _arena_tensor=middle)
    assert res.ok and res.mismatches == 0 and res.waves == 32, res.to_dict()
    host = whole.cpu().numpy()
    assert (host[:guard] == sentinel).all() and (host[guard + n:] == sentinel).all()
    spans = host[guard:guard + n].reshape(blocks * 16, vm.SPAN_DWORDS)
    used = np.zeros(vm.SPAN_DWORDS, dtype=bool)
    for first, dwords in vm.REGIONS.values():
        used[first:first + dwords] = True
    assert used.sum() == 2560
    assert (spans[:, ~used] == sentinel).all()
    # the regions were written: not one sentinel word is left in them
    assert not (spans[:, used] == sentinel).any()
    # in the buffer region, above num_records of the last round, the image
    # stands as it was filled: every store there was dropped
    first = vm.REGIONS["buffer"][0]
    r = np.array([2], dtype=np.uint32)
    top = int(vm.buffer_plan(0, r)["num_records"][0]) // 4
    img = vm._Words(0, 3, r).img()[0]
    for g in (0, 31):
        tags = vm.tag(np.arange(vm.SPAN_DWORDS * g + first, vm.SPAN_DWORDS * g + first + 1024,
                                dtype=np.uint32))
        got = spans[g, first:first + 1024].view(np.uint32) ^ tags
        assert np.array_equal(got[top:], img[top:])
        assert not np.array_equal(got[:top], img[:top])


# 7. child process --------------------------------------------------------------------------------

def test_vmemcheck_child_process():
    env = dict(os.environ)
    # --device takes effect through this variable: main() overwrites a
    # value that would leave the child without a GPU
    env["ROCR_VISIBLE_DEVICES"] = "63"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.vmemcheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True, env=env,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["device"] == 0 and rec["rounds"] == 8
    assert rec["mismatches"] == 0 and rec["waves"] == 16 * cu_count()
