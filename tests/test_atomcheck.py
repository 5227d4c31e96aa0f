"""atomcheck without a GPU: the numpy reference, the claim that every
digest and final is independent of arrival order (replayed op by op in
plain Python, in random orders), the coverage the operand recipes
promise, the closed form of the shared region, and the plumbing from
verdict to health, metrics, agent and CLI with fake runners."""

import json
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import _active
from kubegpu_amd.probe import atomcheck as at

M32 = 0xFFFFFFFF
SEEDS = (0, 0xC0FFEE)
PERMUTATIONS = 5


# -- reference basics ----------------------------------------------------------------------

def test_reference_digests_shape_determinism_seeds_and_period():
    a = at.reference_digests(0, at.PERIOD + 3)
    assert a.shape == (at.PERIOD + 3, 4) and a.dtype == np.uint32
    assert np.array_equal(a, at.reference_digests(0, at.PERIOD + 3))
    assert np.array_equal(a[at.PERIOD:], a[:3])  # period tiling
    assert len({tuple(row) for row in a[:at.PERIOD].tolist()}) == at.PERIOD
    assert np.array_equal(at.reference_digests(0, 5), a[:5])  # prefix property
    b = at.reference_digests(1, 4)
    assert not (a[:4] == b).any()  # every row depends on the seed
    assert np.array_equal(at.reference_digests(1 << 32, 2), a[:2])  # seed is a u32
    assert at.reference_digests(0, 0).shape == (0, 4)


def test_argument_errors():
    with pytest.raises(ValueError):
        at.reference_digests(0, -1)
    with pytest.raises(ValueError):
        at.reference_values(0, 4, 0)
    with pytest.raises(ValueError):
        at.reference_values(0, 0, 65536)
    with pytest.raises(ValueError):
        at.reference_shared(0, -1, 16)
    with pytest.raises(ValueError):
        at.reference_shared(0, 2, 16, drop=(16, 0))
    with pytest.raises(ValueError):
        at.reference_shared(0, 2, 16, drop=(0, 2))
    with pytest.raises(ValueError):
        at.apply_int("nand", 0, 0, 32)


def test_slot_tables_and_values_agree():
    assert at.STAGES == ("lds", "g32", "g64", "gfp")
    assert [len(at.slot_table(s)) for s in range(4)] == [50, 26, 20, 19]
    for s in range(4):
        table = at.slot_table(s)
        vals = at.reference_values(0, s, 3)
        assert list(vals) == [n for n, _ in table]
        assert all(v.shape == (64,) and v.dtype == np.uint64 for v in vals.values())
        for name, kind in table:
            if kind == "final":
                assert not vals[name][8:].any()
    # rounds PERIOD apart share their inputs
    for s in range(4):
        a, b = at.reference_values(5, s, 1), at.reference_values(5, s, 1 + at.PERIOD)
        assert all(np.array_equal(a[k], b[k]) for k in a)


def _fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _salt(n):
    return ((n + 1) * 0x9E3779B9) & M32


def _fold(v, key):
    return _fmix((v & M32) ^ _fmix((v >> 32) + _salt(key)))


def _digest_of_values(stage, vals):
    """The docstring's digest, in plain Python, from reference_values."""
    table = at.slot_table(stage)
    total, key_slot = 0, {}
    for n, (name, kind) in enumerate(table):
        key_slot[name] = n
        if kind == "final" and n and table[n - 1][1] == "returns" \
                and table[n - 1][0].endswith(".xchg"):
            key_slot[name] = n - 1
    for name, kind in table:
        v, k = [int(x) for x in vals[name]], key_slot[name]
        if kind in ("owned", "cross"):
            total += sum(_fold(v[lane], 64 * k + lane) for lane in range(64))
        elif kind == "returns":
            total += sum(_fold(v[lane], 64 * k + (lane & 7)) for lane in range(64))
        else:
            total += sum(_fold(v[c], 64 * k + c) for c in range(8))
    return total & M32


def test_reference_digests_fold_the_values():
    ref = at.reference_digests(7, 3)
    for r in (0, 2):
        for s in range(4):
            assert _digest_of_values(s, at.reference_values(7, s, r)) == int(ref[r, s])


# -- order independence ----------------------------------------------------------------------

def _bf16_round(x):
    """Nearest-even rounding of an integer to 8 significant bits: what a
    bf16 running sum keeps."""
    if x == 0:
        return 0
    sign, m = (-1 if x < 0 else 1), abs(x)
    shift = max(0, m.bit_length() - 8)
    q, rem = m >> shift, m & ((1 << shift) - 1)
    half = (1 << shift) >> 1
    if shift and (rem > half or (rem == half and (q & 1))):
        q += 1
    return sign * (q << shift)


def _float_add(fmt, acc, x):
    """acc + x in the actual narrow type; asserts that it is exact."""
    exact = acc + x
    if fmt == "f16":
        got = int(np.float16(acc) + np.float16(x))
    elif fmt == "bf16":
        got = _bf16_round(exact)
    elif fmt == "f32":
        got = int(np.float32(acc) + np.float32(x))
    else:
        got = int(np.float64(acc) + np.float64(x))
    assert got == exact and abs(exact) <= at.FLOAT_EXACT[fmt], (fmt, acc, x)
    return got


def _bits(fmt, v):
    if fmt == "f16":
        return int(np.float16(v).view(np.uint16))
    if fmt == "bf16":
        return int(np.float32(v).view(np.uint32)) >> 16
    if fmt == "f32":
        return int(np.float32(v).view(np.uint32))
    return int(np.float64(v).view(np.uint64))


def _replay_contended(entry, order):
    """Apply one contended op lane by lane in ``order``: (finals [8],
    returned value per lane [64])."""
    name, op, typ, init, x = entry
    returns = [None] * 64
    if typ.startswith("u"):
        width = int(typ[1:])
        cells = [int(v) for v in init]
        for lane in order:
            c = lane & 7
            returns[lane] = cells[c]
            cells[c] = at.apply_int(op, cells[c], int(x[lane]), width)
        return cells, returns
    if op == "add":
        cells = [0] * 8
        for lane in order:
            cells[lane & 7] = _float_add(typ, cells[lane & 7], int(x[lane]))
        return cells, returns
    cells = [float("inf") if op == "min" else float("-inf")] * 8
    for lane in order:
        c = lane & 7
        cells[c] = min(cells[c], int(x[lane])) if op == "min" else max(cells[c], int(x[lane]))
    return [int(v) for v in cells], returns


@pytest.mark.parametrize("seed", SEEDS)
def test_contended_phase_is_independent_of_arrival_order(seed):
    rng = random.Random(1234 + seed)
    for stage in range(4):
        r = stage  # a different round per stage
        ref = at.reference_values(seed, stage, r)
        want_digest = int(at.reference_digests(seed, r + 1)[r, stage])
        entries = at.reference_contended(seed, stage, r)
        assert entries
        for _ in range(PERMUTATIONS):
            vals = {k: v.copy() for k, v in ref.items()}
            packed = {}
            for entry in entries:
                order = list(range(64))
                rng.shuffle(order)
                name, op, typ = entry[:3]
                finals, returns = _replay_contended(entry, order)
                if typ.startswith("u"):
                    if op in ("ticket", "xchg"):
                        vals[name] = np.array(returns, dtype=np.uint64)
                    assert [int(v) for v in ref[name + ".final"][:8]] == finals \
                        or op == "xchg"
                    vals[name + ".final"][:8] = np.array(finals, dtype=np.uint64)
                    if op == "xchg":  # the multiset is what is defined
                        got = sorted(zip([l & 7 for l in range(64)], returns)) \
                            + sorted(enumerate(finals))
                        want = sorted(zip([l & 7 for l in range(64)],
                                          (int(v) for v in ref[name]))) \
                            + sorted(enumerate(int(v) for v in ref[name + ".final"][:8]))
                        assert sorted(got) == sorted(want)
                elif name.endswith((".lo", ".hi")):
                    packed[name] = [_bits(typ, v) for v in finals]
                else:
                    assert [_bits(typ, v) for v in finals] == \
                        [int(v) for v in ref[name + ".final"][:8]]
            for name in {n[:-3] for n in packed}:
                both = [lo | (hi << 16) for lo, hi in zip(packed[name + ".lo"],
                                                           packed[name + ".hi"])]
                assert both == [int(v) for v in ref[name + ".final"][:8]]
            # what the kernel would fold after this arrival order
            assert _digest_of_values(stage, vals) == want_digest


@pytest.mark.parametrize("seed", SEEDS)
def test_cross_wave_phase_is_independent_of_arrival_order(seed):
    rng = random.Random(99 + seed)
    init, contributions = at.reference_cross(seed, 2)
    assert len(contributions) == 16 * 64 * 8
    want = [int(v) for v in at.reference_values(seed, 0, 2)["cross.final"]]
    per_cell = [0] * 64
    for cell, op, _ in contributions:
        assert at.CROSS_OPS[cell & 7] == op
        per_cell[cell] += 1
    assert per_cell == [128] * 64
    for _ in range(PERMUTATIONS):
        rng.shuffle(contributions)
        cells = [int(v) for v in init]
        for cell, op, x in contributions:
            cells[cell] = at.apply_int(op, cells[cell], x, 32)
        assert cells == want
    # or / and / umin / umax finals are not trivial
    ops = [at.CROSS_OPS[c & 7] for c in range(64)]
    assert all(0 < want[c] < M32 for c in range(64) if ops[c] in ("or", "and"))


def _replay_shared(seed, rounds, waves, order, skip=None):
    cells = [[int(v) for v in row] for row in at.shared_initial()]
    fsum = [0] * 64
    ops = {(r, w): at.shared_operands(seed, r, w)
           for r in range(0, rounds, at.SHARED_EVERY) for w in range(waves)}
    for key in order:
        if key == skip:
            continue
        x = ops[key]
        for lane in range(64):
            cells[0][lane] = at.apply_int("add", cells[0][lane], int(x[0, lane]), 32)
            cells[1][lane] = at.apply_int("add", cells[1][lane], int(x[1, lane]), 64)
            cells[2][lane] = at.apply_int("xor", cells[2][lane], int(x[2, lane]), 32)
            cells[3][lane] = at.apply_int("umax", cells[3][lane], int(x[3, lane]), 32)
            cells[4][lane] = at.apply_int("umin", cells[4][lane], int(x[4, lane]), 32)
            v = float(np.uint64(x[5, lane]).view(np.float64))
            assert v == int(v) and v != 0 and abs(v) < 1 << 20
            fsum[lane] = _float_add("f64", fsum[lane], int(v))
    cells[5] = [_bits("f64", v) for v in fsum]
    return np.array(cells, dtype=np.uint64)


@pytest.mark.parametrize("seed", SEEDS)
def test_reference_shared_closed_form_equals_brute_force_in_any_order(seed):
    rounds, waves = 5, 32
    keys = [(r, w) for r in range(0, rounds, at.SHARED_EVERY) for w in range(waves)]
    want = at.reference_shared(seed, rounds, waves)
    assert want.shape == (6, 64) and want.dtype == np.uint64
    rng = random.Random(7 + seed)
    for _ in range(PERMUTATIONS):
        rng.shuffle(keys)
        assert np.array_equal(_replay_shared(seed, rounds, waves, keys), want)
    # rounds the shared region is not hit on change nothing
    if at.SHARED_EVERY > 1:
        assert np.array_equal(at.reference_shared(seed, 1, waves),
                              at.reference_shared(seed, at.SHARED_EVERY, waves))
    assert np.array_equal(at.reference_shared(seed, 0, waves), at.shared_initial())


def test_every_single_contribution_changes_the_three_add_finals():
    rounds, waves = 5, 32
    want = at.reference_shared(0, rounds, waves)
    for r in range(0, rounds, at.SHARED_EVERY):
        for w in range(waves):
            got = at.reference_shared(0, rounds, waves, drop=(w, r))
            for row in (0, 1, 5):
                assert (got[row] != want[row]).all(), (r, w, row)
    # the closed form with a contribution left out equals the replay without it
    keys = [(r, w) for r in range(0, rounds, at.SHARED_EVERY) for w in range(waves)]
    for skip in ((0, 0), (at.SHARED_EVERY * 2, 31), (0, 17)):
        got = at.reference_shared(0, rounds, waves, drop=(skip[1], skip[0]))
        assert np.array_equal(_replay_shared(0, rounds, waves, keys, skip=skip), got)
    # a round the region is not hit on has nothing to drop
    if at.SHARED_EVERY > 1:
        assert np.array_equal(at.reference_shared(0, rounds, waves, drop=(3, 1)), want)
    # a round that repeats PERIOD later: one of two equal contributions
    # leaves max and min alone, the adds still move
    long = at.PERIOD + 1
    a = at.reference_shared(0, long, 2)
    b = at.reference_shared(0, long, 2, drop=(1, 0))
    assert (a[0] != b[0]).all() and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4])


# -- coverage conditions ---------------------------------------------------------------------

def _owned_columns(stage, tag):
    """{slot name: uint64 [PERIOD * 64]} of one owned chain over a period."""
    cols = {}
    for r in range(at.PERIOD):
        for k, v in at.reference_values(0, stage, r).items():
            if k.startswith(tag + "."):
                cols.setdefault(k, []).append(v)
    return {k: np.concatenate(v) for k, v in cols.items()}


def _next_value(cols, names, name):
    """The cell after op ``name``: what the next op in the chain returned."""
    return cols[names[names.index(name) + 1]]


def _signed(v, width):
    return v.astype(np.int64) if width == 64 else v.astype(np.uint32).view(np.int32)


@pytest.mark.parametrize("stage,tag,width", [(0, "u32", 32), (1, "u32", 32),
                                             (0, "u64", 64), (2, "u64", 64)])
def test_owned_integer_chains_reach_both_outcomes(stage, tag, width):
    cols = _owned_columns(stage, tag)
    names = [n for n, _ in at.slot_table(stage) if n.startswith(tag + ".")]
    n = len(cols[names[0]])
    lo, hi = n / 8, 7 * n / 8

    def changed(op):
        return int((_next_value(cols, names, f"{tag}.{op}") != cols[f"{tag}.{op}"]).sum())

    for op in ("umin", "umax", "smin", "smax"):
        if f"{tag}.{op}" in cols:
            assert lo <= changed(op) <= hi, op
    if f"{tag}.cas" in cols:
        before, after = cols[f"{tag}.cas"], _next_value(cols, names, f"{tag}.cas")
        # the cell held what the exchange put there; a hit replaces it
        hits = int((after != before).sum())
        assert lo <= hits <= hi
    if f"{tag}.inc" in cols:
        before, after = cols[f"{tag}.inc"], _next_value(cols, names, f"{tag}.inc")
        wraps = int(((after == 0) & (before != M32)).sum())
        assert lo <= wraps <= hi and int((after == before + 1).sum()) >= lo
        before, after = cols[f"{tag}.dec"], _next_value(cols, names, f"{tag}.dec")
        steps = int(((before != 0) & (after == before - 1)).sum())
        assert lo <= steps <= hi and n - steps >= lo


def test_owned_f64_min_and_max_reach_both_outcomes():
    cols = _owned_columns(3, "f64")
    n = len(cols["f64.min"])
    as_f = lambda v: v.view(np.float64)  # noqa: E731
    for op, nxt in (("min", "f64.max"), ("max", "f64.final")):
        moved = int((as_f(cols[nxt]) != as_f(cols[f"f64.{op}"])).sum())
        assert n / 8 <= moved <= 7 * n / 8, op


def test_contended_min_max_change_and_keep():
    """Each contended min / max sees operands that lower (raise) the
    cell and operands that leave it alone."""
    for stage in range(4):
        for r in range(8):
            for name, op, typ, init, x in at.reference_contended(0, stage, r):
                if op not in ("umin", "umax", "smin", "smax"):
                    continue
                width = int(typ[1:])
                moved = kept = 0
                cells = [int(v) for v in init]
                for lane in range(64):
                    new = at.apply_int(op, cells[lane & 7], int(x[lane]), width)
                    moved += new != cells[lane & 7]
                    kept += new == cells[lane & 7]
                    cells[lane & 7] = new
                assert moved >= 8 and kept >= 8, (stage, r, name)


def test_float_operands_are_nonzero_and_within_their_bounds():
    limits = {"f32": 1 << 12, "f64": 1 << 20, "f16": 1 << 7, "bf16": 1 << 5}
    assert {k: 1 << v for k, v in at.FLOAT_BITS.items()} == limits
    for stage in (0, 3):
        for r in range(at.PERIOD):
            for name, op, typ, init, x in at.reference_contended(0, stage, r):
                if typ.startswith("u"):
                    continue
                x = np.asarray(x)
                assert (x != 0).all() and (np.abs(x) <= limits[typ]).all(), name
                # eight terms from zero stay exact whatever the order
                assert 8 * limits[typ] <= at.FLOAT_EXACT[typ]
    # the owned chains: three terms (four for f64 in gfp), all in range
    for stage in (0, 3):
        for fmt, width in (("f32", 32), ("f64", 64), ("f16x2", 16), ("bf16x2", 16)):
            base = fmt.split("x")[0]
            assert 4 * limits[base] <= at.FLOAT_EXACT[base]
            cols = _owned_columns(stage, fmt)
            for name, v in cols.items():
                if base in ("f16", "bf16"):
                    halves = np.concatenate([v & np.uint64(0xFFFF), v >> np.uint64(16)])
                    if base == "f16":
                        f = halves.astype(np.uint16).view(np.float16).astype(np.float64)
                    else:
                        f = (halves.astype(np.uint32) << np.uint32(16)).view(np.float32)
                elif base == "f32":
                    f = v.astype(np.uint32).view(np.float32)
                else:
                    f = v.view(np.float64)
                assert np.isfinite(f).all() and (f == np.rint(f)).all()
                assert (np.abs(f) <= 4 * limits[base]).all(), name
                if name.endswith("add0") or name == "f64.add":  # the stored operand
                    assert (f != 0).all()


def test_inputs_do_not_depend_on_the_wave_but_on_stage_and_seed():
    a = at.reference_values(0, 1, 0)
    b = at.reference_values(0, 0, 0)
    assert not np.array_equal(a["u32.add"], b["u32.add"])  # stage enters the base
    from kubegpu_amd.probe import fpcheck as fp

    w = at._Words(0, 0, np.array([0], dtype=np.uint32)).w(np.arange(64))
    assert not np.array_equal(w[0], fp._slot_words(0, 0, np.array([0], dtype=np.uint32))
                              .reshape(-1)[:64])


# -- result type and exports ---------------------------------------------------------------------

def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = at.AtomcheckResult(ok=False, rounds=3, waves=48, mismatches=0, shared_mismatches=2,
                             shared_records=[{"op": "u32_add", "cell": 3, "expected": 1,
                                              "got": 2}],
                             cus_covered=3, cu_count=256, elapsed_s=0.5, g32_gops=1.5,
                             waves_on=[0] * 1024)
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"lds_gops", "g32_gops", "g64_gops", "gfp_gops", "shared_mismatches",
            "shared_records", "mismatches", "cus_covered"} <= set(d)
    assert d["shared_mismatches"] == 2 and d["g32_gops"] == 1.5
    assert at.metric_args(d) == (0, 2, 3)
    assert at.DEFAULT_ROUNDS % at.PERIOD == 0 and at.PERIOD <= at.DEFAULT_ROUNDS <= 65536
    assert at.SHARED_EVERY >= 1
    assert probe.AtomcheckResult is at.AtomcheckResult
    assert probe.atomcheck_round is at.atomcheck_round
    assert probe.run_atomcheck_subprocess is at.run_atomcheck_subprocess
    assert probe.reference_shared is at.reference_shared


def test_registry():
    assert _active.ACTIVE_PROBES == ("memcheck", "cucheck", "mxcheck", "fpcheck", "hostlink")
    assert _active.HEALTH_PROBES[:-1] == _active.ACTIVE_PROBES
    assert _active.HEALTH_PROBES[-1] == "atomcheck"
    assert at._child_lock is _active._child_lock


def test_run_atomcheck_subprocess_passes_rounds(monkeypatch):
    calls = []

    def fake(cmd, **kw):
        calls.append((list(cmd), kw, _active._child_lock.locked()))
        return subprocess.CompletedProcess(cmd, 1, 'noise\n{"ok": false, "mismatches": 1}\n', "")

    monkeypatch.setattr(_active.subprocess, "run", fake)
    rec = at.run_atomcheck_subprocess(3, 128, timeout_s=9.0)
    assert rec == {"ok": False, "mismatches": 1, "exit_code": 1}
    cmd, kw, locked = calls[0]
    assert cmd == [sys.executable, "-m", "kubegpu_amd.probe.atomcheck",
                   "--device", "3", "--rounds", "128"]
    assert locked and kw["timeout"] == 9.0


# -- manager verdicts ------------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


PASS = {"ok": True, "mismatches": 0, "shared_mismatches": 0, "first_bad_round": None,
        "bad_stages": [], "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}
FAIL = dict(PASS, ok=False, mismatches=4, first_bad_round=1, bad_stages=["gfp"],
            bad_cus=["3/1/0/7"])
# wrong cells of the shared region only; ok left for the manager to work out
SHARED_FAIL = {k: v for k, v in dict(PASS, shared_mismatches=3).items() if k != "ok"}


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.atomcheck_status(uuid) is None

    assert mgr.record_atomcheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.atomcheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.fpcheck_status(uuid) is None and mgr.cucheck_status(uuid) is None
    assert len(lines) == 1 and "atomcheck" in lines[0] and uuid in lines[0]
    assert "3/1/0/7" in lines[0] and "gfp" in lines[0]

    assert mgr.record_atomcheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    assert _node_info(mgr).allocatable == base.allocatable

    # shared_mismatches alone turns the GPU unhealthy, even where the
    # result calls itself ok
    assert mgr.record_atomcheck(uuid, SHARED_FAIL) is False
    assert mgr.device_health()[uuid] is False
    assert mgr.atomcheck_status(uuid)["shared_mismatches"] == 3
    assert "3 wrong shared cell" in lines[-1]
    assert mgr.record_atomcheck(uuid, dict(PASS, shared_mismatches=1)) is False
    assert mgr.clear_atomcheck(uuid) is True
    assert mgr.clear_atomcheck(uuid) is False
    assert mgr.atomcheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough, and the five older probes still count
    mgr.record_atomcheck(uuid, PASS)
    mgr.record_fpcheck(uuid, {"ok": False, "mismatches": 1})
    assert mgr.device_health()[uuid] is False
    mgr.clear_fpcheck(uuid)
    assert mgr.device_health()[uuid] is True

    with pytest.raises(KeyError):
        mgr.record_atomcheck("GPU-does-not-exist", FAIL)
    assert set(mgr.atomcheck) == {uuid}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_atomcheck(uuid, SHARED_FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.atomcheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.atomcheck_status(uuid) is None


# -- atomcheck_round ---------------------------------------------------------------------

def test_round_records_verdicts_and_selects_idle_gpus():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    calls = []

    def runner(index, rounds):
        calls.append((index, rounds))
        rec = dict(FAIL if index == 5 else SHARED_FAIL if index == 6 else PASS)
        rec["exit_code"] = 1 if index in (5, 6) else 0
        return rec

    metrics = Metrics()
    out = at.atomcheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False and health[by_index[6]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 7))
    assert mgr.atomcheck_status(by_index[1]) is None
    assert mgr.fpcheck == {} and mgr.cucheck == {}
    assert metrics.gpu_atomcheck[by_index[5]]["mismatches"] == 4
    assert metrics.gpu_atomcheck[by_index[6]] == {
        "mismatches": 0, "shared_mismatches": 3, "cus_covered": 256,
        "timestamp": metrics.gpu_atomcheck[by_index[6]]["timestamp"]}
    assert metrics.gpu_atomcheck[by_index[0]]["shared_mismatches"] == 0
    assert metrics.gpu_atomcheck_errors == {} and metrics.gpu_fpcheck == {}

    calls.clear()
    at.atomcheck_round(mgr, runner, None, rounds=8, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_runner_errors_leave_health_untouched_and_count():
    from kubegpu_amd.metrics import Metrics

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_atomcheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, rounds):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("atomcheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        if index == 4:
            return "not a dict"
        if index == 7:  # gone while its child ran
            with mgr._lock:
                del mgr.gpus[by_index[7]]
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = at.atomcheck_round(mgr, runner, metrics, rounds=8)
    after = mgr.device_health()
    assert by_index[7] not in after
    assert after == {u: h for u, h in before.items() if u != by_index[7]}
    assert mgr.atomcheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2, 4):
        assert mgr.atomcheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_atomcheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3, 4)}
    assert set(metrics.gpu_atomcheck) == {by_index[i] for i in (5, 6)}
    assert by_index[7] not in out and by_index[7] not in mgr.atomcheck


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_atomcheck("GPU-a", 2, 5, 255, 1700000000.0)
        m.inc_atomcheck_error("GPU-a")
        m.inc_atomcheck_error("GPU-a")
        assert m.gpu_atomcheck["GPU-a"] == {
            "mismatches": 2, "shared_mismatches": 5, "cus_covered": 255,
            "timestamp": 1700000000.0}
        assert m.gpu_atomcheck_errors["GPU-a"] == 2
        assert m.gpu_fpcheck == {} and m.gpu_hostlink_errors == {}
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_atomcheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_atomcheck_shared_mismatches", lab) == 5.0
        assert reg.get_sample_value("kubegpu_amd_gpu_atomcheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_atomcheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_atomcheck_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert generate_latest(reg).count(b"/mxcheck)/atomcheck\n") == 1  # the health gauge's help text
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_atomcheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--atomcheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--atomcheck needs real GPUs" in cap.err and "atomic units" in cap.err
    assert cap.out == ""
    assert amddevs._PROBE_RUNS["atomcheck"][3] == ("mismatches", "shared_mismatches")


def test_amddevs_exit_code_counts_shared_mismatches(monkeypatch, capsys):
    """A result whose only wrong data is in the shared region exits 1."""
    from kubegpu_amd.cli import amddevs

    results = {}
    monkeypatch.setattr(at, "atomcheck_round",
                        lambda mgr, runner, metrics, rounds, max_process_count: results)
    backend = FakeBackend(fixtures.fixture_8x_mi355x())
    args = amddevs.argparse.Namespace(fake=False, rounds=8, memcheck_idle_only=False)
    results["GPU-a"] = dict(PASS)
    assert amddevs._run_probe("atomcheck", args, backend) == 0
    results["GPU-b"] = dict(SHARED_FAIL)
    assert amddevs._run_probe("atomcheck", args, backend) == 1
    results.clear()
    results["GPU-a"] = {"error": "x", "exit_code": 2}
    assert amddevs._run_probe("atomcheck", args, backend) == 2
    capsys.readouterr()


def test_amddevs_health_shows_the_row(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["atomcheck"] is None for r in rows.values())
    assert all("fpcheck" in r and "mxcheck" in r for r in rows.values())


def test_agent_oneshot_accepts_atomcheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--atomcheck-interval", "600", "--atomcheck-rounds", "64",
                              "--atomcheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_atomcheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert at.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
