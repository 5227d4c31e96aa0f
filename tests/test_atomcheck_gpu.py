"""Atomic-unit kernel on a real MI355X: every wave's digests against the
numpy reference (period wrap included), every returned value and final
of wave 0 against it (which names the op that disagrees), the default
grid with its cross-XCD shared region, repeatability, exact attribution
of an injected fault, a really lost update, a tampered table, argument
checks and the CLI child."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import atomcheck as at

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = at.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# 1. digests ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_equal_the_reference(seed):
    got = at.wave_digests(seed, rounds=3, blocks=2)
    assert got.shape == (32, 3, 4) and got.dtype == np.uint32
    bad = np.argwhere(got != ref(seed, 3)[None])
    assert len(bad) == 0, [(int(w), int(r), at.STAGES[s]) for w, r, s in bad[:8]]


def test_wave_digests_across_the_period_wrap():
    rounds = at.PERIOD + 1
    got = at.wave_digests(0, rounds, blocks=1)
    assert np.array_equal(got, np.broadcast_to(ref(0, rounds), (16, rounds, 4)))
    assert np.array_equal(got[:, at.PERIOD], got[:, 0])


# 2. every value ----------------------------------------------------------------------------

def _by_cell(v):
    """[64 lanes] -> sorted arrivals per cell, [8, 8]."""
    return np.sort(v.reshape(8, 8), axis=0)


@pytest.mark.parametrize("r", (0, 1))
@pytest.mark.parametrize("stage", range(4))
def test_wave_values_equal_the_reference(stage, r):
    got = at.wave_values(0, stage, r)
    want = at.reference_values(0, stage, r)
    table = at.slot_table(stage)
    assert list(got) == list(want) == [n for n, _ in table]
    failures = []
    for n, (name, kind) in enumerate(table):
        g, w = got[name], want[name]
        if kind in ("owned", "cross"):  # element for element
            ok = np.array_equal(g, w)
        elif kind == "returns" and name.endswith(".xchg"):
            # an exchanged cell's returns and its final: one multiset
            final = table[n + 1][0]
            assert final == name + ".final"
            ok = np.array_equal(
                np.sort(np.vstack([g.reshape(8, 8), got[final][None, :8]]), axis=0),
                np.sort(np.vstack([w.reshape(8, 8), want[final][None, :8]]), axis=0))
        elif kind == "returns":  # sorted multisets per cell
            ok = np.array_equal(_by_cell(g), _by_cell(w))
        elif name.endswith(".xchg.final"):
            # which lane came last is not defined, only that it was one of them
            cells = want[name[:-6]].reshape(8, 8)
            ok = all(g[c] in cells[:, c] or g[c] == w[c] for c in range(8)) \
                and not g[8:].any()
        else:  # finals exactly
            ok = np.array_equal(g, w)
        if not ok:
            failures.append((name, kind, [hex(int(x)) for x in g[:8]],
                             [hex(int(x)) for x in w[:8]]))
    assert not failures, failures[:4]


# 3. whole-GPU run ------------------------------------------------------------------------------

def test_default_grid_is_clean_and_repeatable():
    for _ in range(2):  # the arena is initialised anew for every run
        res = at.atomcheck(rounds=2)
        assert res.ok and res.mismatches == 0 and res.shared_mismatches == 0, res.to_dict()
        assert res.waves == 16 * cu_count() == 16 * res.cu_count
        assert 1 <= res.cus_covered <= res.cu_count
        assert res.records == [] and res.shared_records == [] and res.bad_cus == []
        assert res.first_bad_round is None and res.rounds == 2
        assert res.elapsed_s > 0 and res.gfp_gops > 0
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d


# 4. test hooks ---------------------------------------------------------------------------------

def test_injected_digest_fault_is_attributed_exactly():
    res = at.atomcheck(seed=0, rounds=3, blocks=2, _inject=(17, 1, 2, 0x10))
    assert not res.ok and res.mismatches == 1 and res.shared_mismatches == 0
    assert res.first_bad_round == 1 and res.bad_stages == ["g64"]
    (rec,) = res.records
    assert rec["wave"] == 17 and rec["block"] == 1
    assert rec["round"] == 1 and rec["stage"] == "g64"
    assert rec["expected"] ^ rec["got"] == 0x10
    assert rec["expected"] == int(ref(0, 3)[1, 2])


def test_a_lost_update_shows_in_the_shared_region_only():
    rounds, blocks = 2, 2
    want = at.reference_shared(0, rounds, 32)
    dropped = at.reference_shared(0, rounds, 32, drop=(5, 0))
    changed = np.argwhere(want != dropped)
    assert len(changed) >= 3 * 64  # the three adds move in every cell
    res = at.atomcheck(seed=0, rounds=rounds, blocks=blocks, max_records=512, _drop=(5, 0))
    assert res.mismatches == 0 and res.records == []
    assert res.shared_mismatches == len(changed)
    assert not res.ok
    assert [(at.SHARED_OPS.index(r["op"]), r["cell"]) for r in res.shared_records] == \
        [(int(op), int(cell)) for op, cell in changed]
    for r in res.shared_records:
        op = at.SHARED_OPS.index(r["op"])
        assert r["expected"] == int(want[op, r["cell"]])
        assert r["got"] == int(dropped[op, r["cell"]])


def test_a_tampered_table_fails_every_wave_in_that_round():
    table = ref(0, 3).copy()
    table[1, 3] ^= 1
    res = at.atomcheck(seed=0, rounds=3, blocks=2, max_records=64, _expected=table)
    assert not res.ok and res.mismatches == 32 and res.shared_mismatches == 0
    assert res.first_bad_round == 1 and res.bad_stages == ["gfp"]
    assert sorted(r["wave"] for r in res.records) == list(range(32))
    assert all(r["round"] == 1 and r["stage"] == "gfp" for r in res.records)


# 5. arguments ----------------------------------------------------------------------------------

@pytest.mark.parametrize("kwargs", [
    dict(rounds=0), dict(rounds=65537), dict(blocks=4097),
    dict(rounds=2, blocks=2, _inject=(32, 0, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 2, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 0, 4, 1)),
    dict(rounds=2, blocks=2, _drop=(32, 0)),
    dict(rounds=2, blocks=2, _drop=(0, 2)),
])
def test_bad_arguments_raise_before_any_launch(kwargs):
    with pytest.raises((ValueError, RuntimeError), match="atomcheck"):
        at.atomcheck(**kwargs)


def test_the_extension_checks_its_own_arguments():
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    expected = torch.from_numpy(ref(0, 2).view(np.int32).copy()).cuda()
    small = torch.zeros(8, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="atomcheck: arena must hold"):
        ext.atomcheck_run(expected, 0, 2, 2, small, 1, 0, None, None, None)
    arena = at._arena(2, torch.device("cuda", 0))
    with pytest.raises(RuntimeError, match="atomcheck: drop"):
        ext.atomcheck_run(expected, 0, 2, 2, arena, 1, 0, None, None, (32, 0))
    with pytest.raises(RuntimeError, match="atomcheck: inject"):
        ext.atomcheck_run(expected, 0, 2, 2, arena, 1, 0, None, (0, 0, 4, 1), None)
    with pytest.raises(RuntimeError, match="atomcheck: stage"):
        ext.atomcheck_values(0, 4, 0)
    assert ext.atomcheck_layout() == (at.WAVE_CELLS, at.SHARED_CELLS, at._VALUE_ROWS,
                                      at.PERIOD)


# 6. child process --------------------------------------------------------------------------------

def test_atomcheck_child_process():
    env = dict(os.environ)
    # --device takes effect through this variable: main() overwrites a
    # value that would leave the child without a GPU
    env["ROCR_VISIBLE_DEVICES"] = "63"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.atomcheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True, env=env,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["device"] == 0 and rec["rounds"] == 8
    assert rec["mismatches"] == 0 and rec["shared_mismatches"] == 0
    assert rec["waves"] == 16 * cu_count()
