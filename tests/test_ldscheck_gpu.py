"""LDS kernel on a real MI355X: every wave's digests against the numpy
reference (period wrap included), every value of the lowest and the
highest wave of a workgroup against it element for element (which names
the access that disagrees), the default grid, repeatability, exact
attribution of an injected fault, a tampered table, argument checks, the
tables of both sides and the CLI child."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import ldscheck as ld

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = ld.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def tables(seed=0):
    return torch.from_numpy(ld.source_tables(seed).view(np.int32).copy()).cuda()


# 1. digests ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_equal_the_reference(seed):
    got = ld.wave_digests(seed, rounds=3, blocks=2)
    assert got.shape == (32, 3, 4) and got.dtype == np.uint32
    bad = np.argwhere(got != ref(seed, 3)[None])
    assert len(bad) == 0, [(int(w), int(r), ld.STAGES[s]) for w, r, s in bad[:8]]


def test_wave_digests_across_the_period_wrap():
    rounds = ld.PERIOD + 1
    got = ld.wave_digests(0, rounds, blocks=1)
    assert np.array_equal(got, np.broadcast_to(ref(0, rounds), (16, rounds, 4)))
    assert np.array_equal(got[:, ld.PERIOD], got[:, 0])


# 2. every value ----------------------------------------------------------------------------

@pytest.mark.parametrize("wave", (0, 15))  # wave 15's slice ends at the top of the 160 KiB
@pytest.mark.parametrize("r", (0, 1))
@pytest.mark.parametrize("stage", range(4))
def test_wave_values_equal_the_reference(stage, r, wave):
    got = ld.wave_values(0, stage, r, wave=wave)
    want = ld.reference_values(0, stage, r)
    assert list(got) == list(want) == ld.slot_table(stage)
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
        res = ld.ldscheck(rounds=2)
        assert res.ok and res.mismatches == 0, res.to_dict()
        assert res.waves == 16 * cu_count() == 16 * res.cu_count
        assert 1 <= res.cus_covered <= res.cu_count
        assert res.records == [] and res.bad_cus == [] and res.bad_stages == []
        assert res.first_bad_round is None and res.rounds == 2
        assert res.elapsed_s > 0
        assert min(res.width_gbps, res.bank_gbps, res.dma_gbps, res.xwave_gbps) > 0
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d


# 4. test hooks ---------------------------------------------------------------------------------

def test_injected_digest_fault_is_attributed_exactly():
    res = ld.ldscheck(seed=0, rounds=3, blocks=2, _inject=(17, 1, 2, 0x10))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["dma"]
    (rec,) = res.records
    assert rec["wave"] == 17 and rec["block"] == 1
    assert rec["round"] == 1 and rec["stage"] == "dma"
    assert rec["expected"] ^ rec["got"] == 0x10
    assert rec["expected"] == int(ref(0, 3)[1, 2])


def test_a_tampered_table_fails_every_wave_in_that_round():
    table = ref(0, 3).copy()
    table[1, 3] ^= 1
    res = ld.ldscheck(seed=0, rounds=3, blocks=2, max_records=64, _expected=table)
    assert not res.ok and res.mismatches == 32
    assert res.first_bad_round == 1 and res.bad_stages == ["xwave"]
    assert sorted(r["wave"] for r in res.records) == list(range(32))
    assert all(r["round"] == 1 and r["stage"] == "xwave" for r in res.records)


# 5. arguments ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs", [
    dict(rounds=0), dict(rounds=65537), dict(blocks=4097), dict(seed=1 << 32),
    dict(rounds=2, blocks=2, _inject=(32, 0, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 2, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 0, 4, 1)),
    dict(rounds=2, blocks=2, _expected=np.zeros((3, 4), dtype=np.uint32)),
])
def test_bad_arguments_raise_before_any_launch(kwargs):
    with pytest.raises((ValueError, RuntimeError), match="ldscheck"):
        ld.ldscheck(**kwargs)


def test_the_extension_checks_its_own_arguments_and_holds_the_same_tables():
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    expected = torch.from_numpy(ref(0, 2).view(np.int32).copy()).cuda()
    good = tables()
    with pytest.raises(RuntimeError, match="ldscheck: rounds"):
        ext.ldscheck_run(expected, 0, 0, 2, good, 0, None, None)
    with pytest.raises(RuntimeError, match="ldscheck: expected must hold"):
        ext.ldscheck_run(expected, 0, 3, 2, good, 0, None, None)
    with pytest.raises(RuntimeError, match="ldscheck: inject"):
        ext.ldscheck_run(expected, 0, 2, 2, good, 0, None, (0, 0, 4, 1))
    # a tables tensor of the wrong size, dtype or device
    with pytest.raises(RuntimeError, match="ldscheck: tables must hold"):
        ext.ldscheck_run(expected, 0, 2, 2, good[:-1].contiguous(), 0, None, None)
    with pytest.raises(RuntimeError, match="ldscheck: tables must be a contiguous int32"):
        ext.ldscheck_run(expected, 0, 2, 2, good.to(torch.int64), 0, None, None)
    with pytest.raises(RuntimeError, match="ldscheck: tables must be on the GPU"):
        ext.ldscheck_run(expected, 0, 2, 2, good.cpu(), 0, None, None)
    with pytest.raises(RuntimeError, match="ldscheck: tables must hold"):
        ext.ldscheck_values(0, 0, 0, good[:-1].contiguous(), 0)
    with pytest.raises(RuntimeError, match="ldscheck: tables must be on the GPU"):
        ext.ldscheck_values(0, 0, 0, good.cpu(), 0)
    with pytest.raises(RuntimeError, match="ldscheck: stage"):
        ext.ldscheck_values(0, 4, 0, good, 0)
    with pytest.raises(RuntimeError, match="ldscheck: seed"):
        ext.ldscheck_values(1 << 32, 0, 0, good, 0)
    with pytest.raises(RuntimeError, match="ldscheck: wave"):
        ext.ldscheck_values(0, 0, 0, good, 16)
    period, rows, sizes, b32, wide, scatters, placed_x4, placed_dword = ext.ldscheck_layout()
    assert (period, rows) == (ld.PERIOD, ld._VALUE_ROWS)
    assert tuple(sizes) == (ld.SLICE_DWORDS, ld.BANK_DWORDS, ld.ST64_K, ld.CHUNK_DWORDS,
                            ld.UNIT_DWORDS, ld.X_DWORDS, ld.TABLE_DWORDS)
    assert tuple(b32) == ld.B32_STRIDES and tuple(wide) == ld.WIDE_STRIDES
    assert tuple(tuple(e) for e in scatters) == ld.SCATTERS
    assert tuple(tuple(e) for e in placed_x4) == ld.PLACED_X4
    assert tuple(tuple(e) for e in placed_dword) == ld.PLACED_DWORD


# 6. child process --------------------------------------------------------------------------------

def test_ldscheck_child_process():
    env = dict(os.environ)
    # --device takes effect through this variable: main() overwrites a
    # value that would leave the child without a GPU
    env["ROCR_VISIBLE_DEVICES"] = "63"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.ldscheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True, env=env,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["device"] == 0 and rec["rounds"] == 8
    assert rec["mismatches"] == 0 and rec["waves"] == 16 * cu_count()
