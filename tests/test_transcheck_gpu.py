"""Transcendental-unit kernel on a real MI355X: one wave's values against
the high-precision reference under BOUNDS and the class rules (a failure
names operation, operand bits, got, reference and error), the prng chain
exactly, every f16 input of one period, every wave's digests against the
fold of the golden values, the period wrap, the default grid, exact
attribution of an injected fault, a damaged golden value, argument checks
and the CLI children."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import transcheck as tc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUNDS = np.arange(tc.PERIOD)


@functools.lru_cache(maxsize=None)
def golden(seed=0):
    """Shared, read-only: (values per stage, hardware id, digest table)."""
    values, hw = tc.golden_values(seed)
    table = np.stack([tc.fold_values(s, v) for s, v in enumerate(values)], axis=1)
    for a in values + [table]:
        a.setflags(write=False)
    return values, hw, table


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# rounds 0, 1 and 7 with the lane and slot offsets put every recipe in
# every lane
@pytest.mark.parametrize("seed,r", [(0, 0), (0xDEADBEEF, 1), (0, 7)])
@pytest.mark.parametrize("stage", range(4))
def test_wave_values_are_within_the_bounds_and_class_rules(stage, seed, r):
    got = tc.wave_values(seed, stage, r)
    assert list(got) == tc.slot_table(stage)
    worst = tc.max_errors(stage, r, got, seed)
    print(tc.STAGES[stage], hex(seed), r, json.dumps(worst))
    bad = tc.check_values(stage, r, got, seed)
    assert not bad, (len(bad), bad[:6])


def test_the_prng_chain_is_exact():
    got = tc.wave_values(0xDEADBEEF, 3, 5)
    p = tc.operands(0xDEADBEEF, 3, 5)["p"][0]
    for j in range(2):
        s = p[j]
        for i in range(8):
            s = tc.prng_step(s)
            assert np.array_equal(got[f"{j}.prng.{i}"], s.astype(np.uint32)), (j, i)


def test_every_f16_input_of_every_operation_is_bounded():
    values = golden()[0][1]
    worst = tc.max_errors(1, ROUNDS, values, 0)
    print(json.dumps(worst))
    bad = tc.check_values(1, ROUNDS, values, 0)
    assert not bad, (len(bad), bad[:6])


@pytest.mark.parametrize("blocks", (1, 3, 0))
def test_every_wave_equals_the_fold_of_one_waves_values(blocks):
    table = golden()[2]
    for s in range(4):
        assert tc.fold_values(s, tc.wave_values(0, s, 1))[0] == table[1, s]
    got = tc.wave_digests(0, 2, blocks)
    assert got.shape == (16 * (blocks or cu_count()), 2, 4) and got.dtype == np.uint32
    bad = np.argwhere(got != table[None, :2])
    assert len(bad) == 0, [(int(w), int(r), tc.STAGES[s]) for w, r, s in bad[:8]]


def test_digests_repeat_at_the_period():
    rounds = tc.PERIOD + 1
    got = tc.wave_digests(0, rounds, blocks=1)
    table = np.vstack([golden()[2], golden()[2][:1]])
    assert np.array_equal(got, np.broadcast_to(table, (16, rounds, 4)))


def test_default_grid_is_clean():
    res = tc.transcheck(rounds=2)
    assert res.ok and res.mismatches == 0, res.to_dict()
    assert res.golden_errors == 0 and res.digest_mismatches == 0 and res.golden_records == []
    assert res.waves == 16 * cu_count() == 16 * res.cu_count
    assert 1 <= res.cus_covered <= res.cu_count
    assert res.records == [] and res.bad_cus == [] and res.bad_stages == []
    assert res.first_bad_round is None and res.rounds == 2 and not res.golden_suspect
    assert res.elapsed_s > 0 and res.chain_gops > 0 and res.golden_s > 0
    assert set(res.golden_wave) == {"xcc", "se", "sh", "cu", "simd"}
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d


def test_injected_digest_fault_is_attributed_exactly():
    res = tc.transcheck(seed=0, rounds=3, blocks=2, _inject=(17, 1, 2, 0x10))
    assert not res.ok and res.mismatches == res.digest_mismatches == 1
    assert res.golden_errors == 0
    assert res.first_bad_round == 1 and res.bad_stages == ["f64"]
    (rec,) = res.records
    assert rec["wave"] == 17 and rec["block"] == 1
    assert rec["round"] == 1 and rec["stage"] == "f64"
    assert rec["expected"] ^ rec["got"] == 0x10
    assert rec["expected"] == int(golden()[2][1, 2])
    # the hook flips the digest before the compare only: no wave differs
    assert res.waves_disagreeing == 0 and not res.golden_suspect


def test_a_damaged_golden_value_fails_the_bound_and_every_wave():
    values, hw, _ = golden()
    err = tc._compare(0, ROUNDS, values[0], 0)[4]
    k = tc.OPS[0].index("exp2")
    r, j, lane = (int(x) for x in np.argwhere(~np.isnan(err[:2, :, k]))[-1])
    damaged = [v.copy() for v in values]
    damaged[0][r, 7 * j + k, lane] ^= 1 << 22  # the top stored significand bit
    res = tc.transcheck(seed=0, rounds=2, blocks=2, max_records=64,
                        _golden_values=(damaged, hw))
    assert not res.ok and res.golden_errors == 1 and res.digest_mismatches == 32
    assert res.mismatches == 33
    (rec,) = res.golden_records
    assert (rec["stage"], rec["op"], rec["round"], rec["slot"], rec["lane"]) == (
        "f32", "exp2", r, j, lane)
    assert rec["error"] > tc.BOUNDS["f32"]["exp2"]
    assert sorted(x["wave"] for x in res.records) == list(range(32))
    assert all(x["round"] == r and x["stage"] == "f32" for x in res.records)
    assert res.waves_disagreeing == 32 and res.golden_suspect


def test_a_late_mismatch_is_recounted_within_one_period():
    rounds, bad = 2 * tc.PERIOD + 8, 2 * tc.PERIOD + 5
    table = np.tile(golden()[2], (3, 1))[:rounds].copy()
    table[bad, 3] ^= 1
    res = tc.transcheck(seed=0, rounds=rounds, blocks=1, _expected=table)
    assert res.digest_mismatches == 16 and res.first_bad_round == bad
    assert res.bad_stages == ["chain"] and res.golden_errors == 0
    assert res.waves_disagreeing == 16 and res.golden_suspect


@pytest.mark.parametrize("kwargs", [
    dict(rounds=0), dict(rounds=65537), dict(blocks=4097),
    dict(rounds=2, blocks=2, _inject=(32, 0, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 2, 0, 1)),
    dict(rounds=2, blocks=2, _inject=(0, 0, 4, 1)),
    dict(rounds=2, blocks=2, _expected=np.zeros((3, 4), dtype=np.uint32)),
])
def test_bad_arguments_raise_before_any_launch(kwargs):
    with pytest.raises(ValueError, match="transcheck"):
        tc.transcheck(**kwargs)


def test_the_extension_checks_its_own_arguments():
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    expected = torch.from_numpy(golden()[2][:2].view(np.int32).copy()).cuda()
    with pytest.raises(RuntimeError, match="transcheck: rounds"):
        ext.transcheck_run(expected, 0, 0, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="transcheck: expected must hold"):
        ext.transcheck_run(expected, 0, 3, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="transcheck: expected must be a contiguous int32"):
        ext.transcheck_run(expected.float(), 0, 2, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="transcheck: expected must be on GPU"):
        ext.transcheck_run(expected.cpu(), 0, 2, 2, 0, None, None)
    with pytest.raises(RuntimeError, match="transcheck: inject"):
        ext.transcheck_run(expected, 0, 2, 2, 0, None, (0, 0, 4, 1))
    with pytest.raises(RuntimeError, match="transcheck: stage"):
        ext.transcheck_values(0, 4, 0, 1)
    with pytest.raises(RuntimeError, match="transcheck: seed"):
        ext.transcheck_values(1 << 32, 0, 0, 1)
    for n_rounds in (0, tc.PERIOD + 1):
        with pytest.raises(RuntimeError, match="transcheck: n_rounds"):
            ext.transcheck_values(0, 0, 0, n_rounds)


def test_transcheck_child_process():
    env = dict(os.environ)
    # --device takes effect through this variable: main() overwrites a
    # value that would leave the child without a GPU
    env["ROCR_VISIBLE_DEVICES"] = "63"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.transcheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True, env=env,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["device"] == 0 and rec["rounds"] == 8
    assert rec["mismatches"] == 0 and rec["golden_errors"] == 0
    assert rec["waves"] == 16 * cu_count()


def test_amddevs_transcheck_cli():
    from kubegpu_amd.discovery import default_backend

    n_gpus = len(default_backend().get_devices().devices)
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--transcheck", "--rounds", "8"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    results = json.loads(res.stdout)
    assert len(results) == n_gpus >= 1
    for rec in results.values():
        assert rec["ok"] is True and rec["mismatches"] == 0 and rec["rounds"] == 8


def test_default_size_run():
    res = tc.transcheck()
    d = res.to_dict()
    print(json.dumps(d))
    assert res.ok and res.rounds == tc.DEFAULT_ROUNDS and res.rounds % tc.PERIOD == 0
    assert res.waves == 16 * cu_count() and res.cus_covered >= 1
