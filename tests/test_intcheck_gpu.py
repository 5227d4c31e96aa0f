"""Integer-ALU kernel on a real MI355X: every wave's digests against the
numpy reference (period wrap included), every value of one wave against
it element for element (which names the op that disagrees), the default
grid, exact attribution of an injected fault, a tampered table, argument
checks and the CLI child."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import intcheck as ic

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = ic.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_equal_the_reference(seed):
    got = ic.wave_digests(seed, rounds=3, blocks=2)
    assert got.shape == (32, 3, 4) and got.dtype == np.uint32
    bad = np.argwhere(got != ref(seed, 3)[None])
    assert len(bad) == 0, [(int(w), int(r), ic.STAGES[s]) for w, r, s in bad[:8]]


def test_wave_digests_across_the_period_wrap():
    rounds = ic.PERIOD + 1
    got = ic.wave_digests(0, rounds, blocks=1)
    assert np.array_equal(got, np.broadcast_to(ref(0, rounds), (16, rounds, 4)))
    assert np.array_equal(got[:, ic.PERIOD], got[:, 0])


# rounds 0, 1 and 7 with the lane and group offsets put every recipe in
# every lane
@pytest.mark.parametrize("r", (0, 1, 7))
@pytest.mark.parametrize("stage", range(4))
def test_wave_values_equal_the_reference(stage, r):
    got = ic.wave_values(0, stage, r)
    want = ic.reference_values(0, stage, r)
    assert list(got) == list(want) == ic.slot_table(stage)
    failures = []
    for n, name in enumerate(want):
        g, w = got[name], want[name]
        if not np.array_equal(g, w):
            lanes = np.flatnonzero(g != w)
            failures.append((n, name, len(lanes), [(int(i), hex(int(g[i])), hex(int(w[i])))
                                                   for i in lanes[:4]]))
    assert not failures, failures[:6]


def test_default_grid_is_clean():
    res = ic.intcheck(rounds=2)
    assert res.ok and res.mismatches == 0, res.to_dict()
    assert res.waves == 16 * cu_count() == 16 * res.cu_count
    assert 1 <= res.cus_covered <= res.cu_count
    assert res.records == [] and res.bad_cus == [] and res.bad_stages == []
    assert res.first_bad_round is None and res.rounds == 2
    assert res.elapsed_s > 0 and res.scalar_gops > 0
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d


def test_injected_digest_fault_is_attributed_exactly():
    res = ic.intcheck(seed=0, rounds=3, blocks=2, _inject=(17, 1, 2, 0x10))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["packed"]
    (rec,) = res.records
    assert rec["wave"] == 17 and rec["block"] == 1
    assert rec["round"] == 1 and rec["stage"] == "packed"
    assert rec["expected"] ^ rec["got"] == 0x10
    assert rec["expected"] == int(ref(0, 3)[1, 2])


def test_a_tampered_table_fails_every_wave_in_that_round():
    table = ref(0, 3).copy()
    table[1, 3] ^= 1
    res = ic.intcheck(seed=0, rounds=3, blocks=2, max_records=64, _expected=table)
    assert not res.ok and res.mismatches == 32
    assert res.first_bad_round == 1 and res.bad_stages == ["scalar"]
    assert sorted(r["wave"] for r in res.records) == list(range(32))
    assert all(r["round"] == 1 and r["stage"] == "scalar" for r in res.records)


@pytest.mark.parametrize("kwargs", [
    dict(rounds=0), dict(rounds=65537), dict(blocks=4097),
    dict(rounds=2, blocks=2, _inject=(32, 0, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 2, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 0, 4, 1)),
    dict(rounds=2, blocks=2, _expected=np.zeros((3, 4), dtype=np.uint32)),
])
def test_bad_arguments_raise_before_any_launch(kwargs):
    with pytest.raises((ValueError, RuntimeError), match="intcheck"):
        ic.intcheck(**kwargs)


def test_the_extension_checks_its_own_arguments():
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    expected = torch.from_numpy(ref(0, 2).view(np.int32).copy()).cuda()
    with pytest.raises(RuntimeError, match="intcheck: rounds"):
        ext.intcheck_run(expected, 0, 0, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="intcheck: expected must hold"):
        ext.intcheck_run(expected, 0, 3, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="intcheck: inject"):
        ext.intcheck_run(expected, 0, 2, 2, 0, None, (0, 0, 4, 1))
    with pytest.raises(RuntimeError, match="intcheck: stage"):
        ext.intcheck_values(0, 4, 0)
    with pytest.raises(RuntimeError, match="intcheck: seed"):
        ext.intcheck_values(1 << 32, 0, 0)


def test_intcheck_child_process():
    env = dict(os.environ)
    # --device takes effect through this variable: main() overwrites a
    # value that would leave the child without a GPU
    env["ROCR_VISIBLE_DEVICES"] = "63"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.intcheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True, env=env,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["device"] == 0 and rec["rounds"] == 8
    assert rec["mismatches"] == 0 and rec["waves"] == 16 * cu_count()
