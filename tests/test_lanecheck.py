"""lanecheck without a GPU: the numpy reference against a second, scalar
implementation written here lane by lane from the documented semantics,
the coverage the operand recipes promise, the digest's dependence on
every slot, and the plumbing from verdict to health, metrics, agent and
CLI with fake runners."""

import functools
import json
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
from kubegpu_amd.probe import lanecheck as lc

M32 = 0xFFFFFFFF
SEEDS = (0, 0xC0FFEE)


# -- a second implementation: plain Python, one lane at a time -----------------------------

def _fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def _salt(n):
    return ((n + 1) * 0x9E3779B9) & M32


def _base(seed, stage, r):
    return _fmix(seed ^ (((24 + stage + 1) * 0x9E3779B9) & M32)
                 ^ (((r % lc.PERIOD) * 0x7F4A7C15) & M32))


class Words:
    def __init__(self, seed, stage, r):
        self.base = _base(seed, stage, r)

    def v(self, k):
        return [_fmix(self.base + 64 * k + lane) for lane in range(64)]

    def u(self, k):
        return _fmix(self.base + 64 * k)


def scalar_dpp_source(ctrl, i):
    """Source lane of lane i, or None, from the issue's wording."""
    row, pos = i // 16, i % 16
    if ctrl < 0x100:  # quad_perm
        return 4 * (i // 4) + ((ctrl >> (2 * (i % 4))) & 3)
    fam, n = ctrl & 0x1F0, ctrl & 0xF
    if fam == 0x100:  # row_shl
        return i + n if pos + n < 16 else None
    if fam == 0x110:  # row_shr
        return i - n if pos - n >= 0 else None
    if fam == 0x120:  # row_ror
        return 16 * row + (pos - n) % 16
    if ctrl == 0x130:  # wave_shl:1
        return i + 1 if i + 1 < 64 else None
    if ctrl == 0x134:  # wave_rol:1
        return (i + 1) % 64
    if ctrl == 0x138:  # wave_shr:1
        return i - 1 if i >= 1 else None
    if ctrl == 0x13C:  # wave_ror:1
        return (i - 1) % 64
    if ctrl == 0x140:  # row_mirror
        return 16 * row + 15 - pos
    if ctrl == 0x141:  # row_half_mirror
        return 8 * (i // 8) + 7 - i % 8
    if ctrl == 0x142:  # row_bcast:15
        return 16 * (row - 1) + 15 if row >= 1 else None
    if ctrl == 0x143:  # row_bcast:31
        return 31 if row >= 2 else None
    if fam == 0x150:  # row_newbcast
        return 16 * row + n
    raise AssertionError(hex(ctrl))


def scalar_dpp(entry, old, src):
    ctrl, row_mask, bank_mask, bound_ctrl = entry
    out = []
    for i in range(64):
        row, bank = i // 16, (i % 16) // 4
        if not (row_mask >> row) & 1 or not (bank_mask >> bank) & 1:
            out.append(old[i])
            continue
        s = scalar_dpp_source(ctrl, i)
        if s is None:
            out.append(0 if bound_ctrl else old[i])
        else:
            out.append(src[s])
    return out


def scalar_swizzle(offset, src):
    out = []
    for i in range(64):
        if offset & 0x8000:
            j = 4 * (i // 4) + ((offset >> (2 * (i % 4))) & 3)
        else:
            and_m, or_m, xor_m = offset & 31, (offset >> 5) & 31, (offset >> 10) & 31
            j = 32 * (i // 32) + ((((i % 32) & and_m) | or_m) ^ xor_m)
        out.append(src[j])
    return out


def scalar_stage(seed, stage, r):
    """Every slot of a stage, in order, as lists of 64 ints."""
    W = Words(seed, stage, r)
    rows = []
    if stage == 0:
        for j, entry in enumerate(lc.DPP_TABLE):
            rows.append(scalar_dpp(entry, W.v(2 * j), W.v(2 * j + 1)))
    elif stage == 1:
        for g in range(4):
            data, idx = W.v(2 * g), W.v(2 * g + 1)
            mask = 0x3FFF if g == 3 else 63
            # the byte address is 4 * (w & mask); the hardware keeps (address / 4) mod 64
            rows.append([data[((4 * (idx[i] & mask)) // 4) % 64] for i in range(64)])
        for p in range(3):
            data, u = W.v(8 + 2 * p), W.u(9 + 2 * p)
            a, b = u | 1, u >> 8
            res = [None] * 64
            for lane in range(64):
                res[(a * lane + b) & 63] = data[lane]
            rows.append(res)
        for s, offset in enumerate(lc.SWIZZLES):
            rows.append(scalar_swizzle(offset, W.v(14 + s)))
    elif stage == 2:
        for i, idx in enumerate(lc.READLANES):
            rows.append([W.v(i)[idx]] * 64)
        for i in range(4):
            if i < 3:
                idx = W.u(3 + 2 * i) & 63
            else:
                idx = (Words(seed, 2, 0).u(9) + r % lc.PERIOD) & 63
            rows.append([W.v(2 + 2 * i)[idx]] * 64)
        t = 1 + W.u(11) % 62
        a, other = W.v(10), W.v(12)
        rows.append([a[t] if lane >= t else other[lane] for lane in range(64)])
        bits0 = [x & 1 for x in W.v(13)]
        bits1 = [x >> 31 for x in W.v(14)]
        for bits in (bits0, bits1):
            word = sum(b << lane for lane, b in enumerate(bits))
            rows.append([word & M32] * 64)
            rows.append([word >> 32] * 64)
        rows.append([sum(bits1[:lane]) for lane in range(64)])
        a, b = W.v(15), W.v(16)
        na, nb = list(a), list(b)
        for arow, brow in ((1, 0), (3, 2)):
            for k in range(16):
                na[16 * arow + k], nb[16 * brow + k] = b[16 * brow + k], a[16 * arow + k]
        rows += [na, nb]
        a, b = W.v(17), W.v(18)
        rows += [a[:32] + b[:32], a[32:] + b[32:]]
    else:
        x = W.v(0)
        incl = [sum(x[:lane + 1]) & M32 for lane in range(64)]
        rows.append(incl)
        rows.append([0] + incl[:63])
        rows.append([sum(W.v(1)) & M32] * 64)
        rows.append([min(W.v(2))] * 64)
        rows.append([max(W.v(3))] * 64)
        rows.append([functools.reduce(lambda p, q: p ^ q, W.v(4))] * 64)
        y = W.v(5)
        rows.append([sum(y[16 * (lane // 16):16 * (lane // 16) + 16]) & M32
                     for lane in range(64)])
    return rows


def scalar_digest(rows):
    total = 0
    for n, row in enumerate(rows):
        for lane, v in enumerate(row):
            total += _fmix(v + _salt(64 * n + lane))
    return total & M32


@functools.lru_cache(maxsize=None)
def ref_period(seed, stage):
    """[(name, uint32 [PERIOD, 64])] of a stage over one period; shared,
    read-only."""
    slots = lc._stage(seed, stage, np.arange(lc.PERIOD, dtype=np.uint32))
    for _, v in slots:
        v.setflags(write=False)
    return slots


# -- the reference against the scalar implementation ----------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("stage", range(4))
def test_reference_values_equal_the_scalar_implementation(seed, stage):
    slots = ref_period(seed, stage)
    digests = lc.reference_digests(seed, lc.PERIOD)
    for r in range(lc.PERIOD):
        rows = scalar_stage(seed, stage, r)
        assert len(rows) == len(slots)
        for n, (name, v) in enumerate(slots):
            assert rows[n] == [int(x) for x in v[r]], (stage, r, n, name)
        assert scalar_digest(rows) == int(digests[r, stage]), (stage, r)


def test_reference_values_shape_and_names():
    assert lc.STAGES == ("dpp", "xbar", "sgpr", "scan")
    assert [len(lc.slot_table(s)) for s in range(4)] == [len(lc.DPP_TABLE), 16, 16, 7]
    assert max(len(lc.slot_table(s)) for s in range(4)) <= lc._VALUE_ROWS
    for s in range(4):
        vals = lc.reference_values(5, s, 3)
        assert list(vals) == lc.slot_table(s) and len(set(vals)) == len(vals)
        assert all(v.shape == (64,) and v.dtype == np.uint32 for v in vals.values())
        for n, (name, v) in enumerate(ref_period(5, s)):
            assert np.array_equal(vals[name], v[3])
        again = lc.reference_values(5, s, 3 + lc.PERIOD)
        assert all(np.array_equal(vals[k], again[k]) for k in vals)
        assert lc.digest_of(vals) == int(lc.reference_digests(5, 4)[3, s])


def test_argument_errors():
    with pytest.raises(ValueError):
        lc.reference_digests(0, -1)
    with pytest.raises(ValueError):
        lc.reference_values(0, 4, 0)
    with pytest.raises(ValueError):
        lc.reference_values(0, 0, 65536)
    with pytest.raises(ValueError):
        lc.dpp_source(0x1FF, 0)
    with pytest.raises(ValueError):
        lc.dpp_source(0, 64)


# -- the tables --------------------------------------------------------------------------------

def test_dpp_source_by_hand():
    qp = lc.quad_perm
    assert [lc.dpp_source(qp(3, 2, 1, 0), i) for i in (0, 1, 2, 3, 62)] == [3, 2, 1, 0, 61]
    assert [lc.dpp_source(qp(0, 0, 2, 2), i) for i in (4, 5, 6, 7)] == [4, 4, 6, 6]
    assert [lc.dpp_source(lc.row_shl(3), i) for i in (0, 12, 13, 15, 16, 63)] == \
        [3, 15, None, None, 19, None]
    assert [lc.dpp_source(lc.row_shr(4), i) for i in (0, 3, 4, 15, 16, 20, 63)] == \
        [None, None, 0, 11, None, 16, 59]
    assert [lc.dpp_source(lc.row_ror(5), i) for i in (0, 4, 5, 15, 16, 37)] == \
        [11, 15, 0, 10, 27, 32]
    assert [lc.dpp_source(lc.WAVE_SHL1, i) for i in (0, 15, 62, 63)] == [1, 16, 63, None]
    assert [lc.dpp_source(lc.WAVE_ROL1, i) for i in (0, 15, 63)] == [1, 16, 0]
    assert [lc.dpp_source(lc.WAVE_SHR1, i) for i in (0, 1, 16, 63)] == [None, 0, 15, 62]
    assert [lc.dpp_source(lc.WAVE_ROR1, i) for i in (0, 1, 16)] == [63, 0, 15]
    assert [lc.dpp_source(lc.ROW_MIRROR, i) for i in (0, 15, 17, 40)] == [15, 0, 30, 39]
    assert [lc.dpp_source(lc.ROW_HALF_MIRROR, i) for i in (0, 7, 8, 61)] == [7, 0, 15, 58]
    assert [lc.dpp_source(lc.ROW_BCAST15, i) for i in (0, 15, 16, 31, 32, 63)] == \
        [None, None, 15, 15, 31, 47]
    assert [lc.dpp_source(lc.ROW_BCAST31, i) for i in (0, 31, 32, 48, 63)] == \
        [None, None, 31, 31, 31]
    assert [lc.dpp_source(lc.row_newbcast(5), i) for i in (0, 5, 15, 16, 63)] == \
        [5, 5, 5, 21, 53]
    for ctrl, *_ in lc.DPP_TABLE:
        assert [lc.dpp_source(ctrl, i) for i in range(64)] == \
            [scalar_dpp_source(ctrl, i) for i in range(64)]


def test_dpp_table_holds_what_it_must():
    qp = lc.quad_perm
    assert len(lc.DPP_TABLE) >= 24
    ctrls = [e[0] for e in lc.DPP_TABLE]
    must = [qp(3, 2, 1, 0), qp(1, 0, 3, 2)] \
        + [lc.row_shl(n) for n in (1, 3, 15)] + [lc.row_shr(n) for n in (1, 2, 4, 8)] \
        + [lc.row_ror(n) for n in (1, 5, 12)] \
        + [lc.WAVE_SHL1, lc.WAVE_ROL1, lc.WAVE_SHR1, lc.WAVE_ROR1, lc.ROW_MIRROR,
           lc.ROW_HALF_MIRROR] + [lc.row_newbcast(n) for n in (0, 5, 15)]
    assert all(c in ctrls for c in must)
    # a quad_perm with repeated selects
    assert any(c < 0x100 and len({(c >> s) & 3 for s in (0, 2, 4, 6)}) < 4 for c in ctrls)
    assert (lc.ROW_BCAST15, 0xA, 0xF, 0) in lc.DPP_TABLE
    assert (lc.ROW_BCAST31, 0xC, 0xF, 0) in lc.DPP_TABLE
    # the broadcasts of the older encoding only under the scans' row masks
    assert all(e[1] == 0xA for e in lc.DPP_TABLE if e[0] == lc.ROW_BCAST15)
    assert all(e[1] == 0xC for e in lc.DPP_TABLE if e[0] == lc.ROW_BCAST31)
    # the shifts with both bound_ctrl settings
    for lo in (0x100, 0x110):
        assert {e[3] for e in lc.DPP_TABLE if lo < e[0] <= lo + 15} == {0, 1}
    for c in (lc.WAVE_SHL1, lc.WAVE_SHR1):
        assert {e[3] for e in lc.DPP_TABLE if e[0] == c} == {0, 1}
    partial = [e for e in lc.DPP_TABLE if e[1] != 0xF or e[2] != 0xF]
    assert len(partial) >= 4
    assert {0x5, 0xA, 0xC} <= {e[1] for e in partial}
    assert {0x3, 0x5, 0xE} <= {e[2] for e in partial}
    assert all(0 <= e[1] <= 0xF and 0 <= e[2] <= 0xF and e[3] in (0, 1) for e in lc.DPP_TABLE)


def test_masked_dpp_entries_keep_some_lanes_and_move_others():
    slots = ref_period(0, 0)
    W = lc._Words(0, 0, np.arange(lc.PERIOD, dtype=np.uint32))
    for j, entry in enumerate(lc.DPP_TABLE):
        if entry[1] == 0xF and entry[2] == 0xF:
            continue
        old, got = W.v(2 * j), slots[j][1]
        kept = (got == old).all(axis=0)  # over the whole period
        assert kept.any() and not kept.all(), (j, entry)
        _, valid, enabled = lc._dpp_maps(entry)
        assert kept[~enabled].all() and not kept[enabled & valid].any()


def test_swizzle_table():
    assert len(lc.SWIZZLES) >= 8
    swap = [lc.swizzle_bits(0x1F, 0, x) for x in (1, 2, 4, 8, 16)]
    assert list(lc.SWIZZLES[:5]) == swap
    for x, off in zip((1, 2, 4, 8, 16), swap):
        assert [lc.swizzle_source(off, i) for i in range(64)] == [i ^ x for i in range(64)]
    rev = lc.swizzle_bits(0x1F, 0, 0x1F)
    assert rev in lc.SWIZZLES
    assert [lc.swizzle_source(rev, i) for i in (0, 31, 32, 40)] == [31, 0, 63, 55]
    bc = lc.swizzle_bits(0x18, 3, 0)
    assert bc in lc.SWIZZLES
    assert [lc.swizzle_source(bc, i) for i in (0, 7, 8, 31, 32, 63)] == [3, 3, 11, 27, 35, 59]
    quads = [o for o in lc.SWIZZLES if o & 0x8000]
    assert lc.swizzle_quad(3, 2, 1, 0) in quads
    assert any(len({(o >> s) & 3 for s in (0, 2, 4, 6)}) < 4 for o in quads)
    assert [lc.swizzle_source(lc.swizzle_quad(1, 1, 3, 0), i) for i in (4, 5, 6, 7)] == \
        [5, 5, 7, 4]
    assert len(lc.READLANES) == 2 and all(0 <= i < 64 for i in lc.READLANES)


# -- coverage conditions ---------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_permute_destinations_are_bijections_in_every_round(seed):
    r = np.arange(lc.PERIOD, dtype=np.uint32)
    maps = set()
    for p in range(3):
        dst = lc.permute_destinations(seed, p, r)
        assert dst.shape == (lc.PERIOD, 64)
        assert (np.sort(dst, axis=1) == np.arange(64)[None, :]).all()
        maps |= {tuple(row) for row in dst.tolist()}
    assert len(maps) > lc.PERIOD  # not one map over and over


@pytest.mark.parametrize("seed", SEEDS)
def test_every_lane_is_a_source_within_one_period(seed):
    r = np.arange(lc.PERIOD, dtype=np.uint32)
    for g in range(4):
        assert set(lc.bpermute_sources(seed, g, r).reshape(-1).tolist()) == set(range(64))
    idx = lc.readlane_indices(seed, r)
    assert idx.shape == (lc.PERIOD, 4)
    assert set(idx.reshape(-1).tolist()) == set(range(64))
    assert sorted(idx[:, 3].tolist()) == list(range(64))  # by construction
    assert len(set(idx[:, 0].tolist())) > 16  # the data-driven ones move too
    # the gather that leaves 14 index bits really has indices past 63
    W = lc._Words(seed, 1, r)
    assert ((W.v(7) & np.uint32(0x3FFF)) > 63).any()


@pytest.mark.parametrize("seed", SEEDS)
def test_ballots_and_readfirstlane_have_both_sides_in_every_round(seed):
    slots = dict(ref_period(seed, 2))
    for name in ("ballot0", "ballot1"):
        word = slots[name + ".lo"][:, 0].astype(np.uint64) \
            | (slots[name + ".hi"][:, 0].astype(np.uint64) << np.uint64(32))
        assert ((word != 0) & (word != np.uint64(0xFFFFFFFFFFFFFFFF))).all()
    t = lc.readfirstlane_threshold(seed, np.arange(lc.PERIOD, dtype=np.uint32))
    assert ((t >= 1) & (t <= 62)).all() and len(set(t.tolist())) > 16
    assert (slots["mbcnt"][:, 0] == 0).all() and (slots["mbcnt"] <= 63).all()


# -- the digest ---------------------------------------------------------------------------------

def test_digest_depends_on_every_slot_and_only_on_its_stage():
    rng = np.random.default_rng(11)
    want = lc.reference_digests(3, 2)[1]
    for stage in range(4):
        vals = lc.reference_values(3, stage, 1)
        assert lc.digest_of(vals) == int(want[stage])
        for name in vals:
            flipped = {k: v.copy() for k, v in vals.items()}
            flipped[name][rng.integers(64)] ^= np.uint32(1 << int(rng.integers(32)))
            got = [lc.digest_of(flipped if s == stage else lc.reference_values(3, s, 1))
                   for s in range(4)]
            assert got[stage] != int(want[stage]), (stage, name)
            assert [g for s, g in enumerate(got) if s != stage] == \
                [int(w) for s, w in enumerate(want) if s != stage]


def test_reference_digests_shape_determinism_seeds_and_period():
    a = lc.reference_digests(0, lc.PERIOD + 3)
    assert a.shape == (lc.PERIOD + 3, 4) and a.dtype == np.uint32
    assert np.array_equal(a, lc.reference_digests(0, lc.PERIOD + 3))
    assert np.array_equal(a[lc.PERIOD:], a[:3])  # rounds r and r + PERIOD
    assert len({tuple(row) for row in a[:lc.PERIOD].tolist()}) == lc.PERIOD
    assert len(set(a[:lc.PERIOD].reshape(-1).tolist())) == 4 * lc.PERIOD  # stage and round
    assert np.array_equal(lc.reference_digests(0, 5), a[:5])
    b = lc.reference_digests(1, 4)
    assert not (a[:4] == b).any()  # every digest depends on the seed
    assert np.array_equal(lc.reference_digests(1 << 32, 2), a[:2])  # seed is a u32
    assert lc.reference_digests(0, 0).shape == (0, 4)


def test_inputs_differ_from_the_other_probes():
    from kubegpu_amd.probe import atomcheck as at

    r0 = np.array([0], dtype=np.uint32)
    mine = {tuple(lc._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    assert len(mine) == 4
    theirs = {tuple(at._Words(0, s, r0).w(np.arange(64))[0].tolist()) for s in range(4)}
    assert not mine & theirs


@pytest.mark.parametrize("seed", SEEDS)
def test_inclusive_scan_is_cumsum(seed):
    r = np.arange(lc.PERIOD, dtype=np.uint32)
    slots = dict(ref_period(seed, 3))
    x = lc._Words(seed, 3, r).v(0).astype(np.uint64)
    want = (np.cumsum(x, axis=1) & np.uint64(M32)).astype(np.uint32)
    assert np.array_equal(slots["scan.inclusive"], want)
    assert np.array_equal(slots["scan.exclusive"][:, 1:], want[:, :-1])
    assert not slots["scan.exclusive"][:, 0].any()
    assert np.array_equal(slots["reduce.sum"][:, 0],
                          (lc._Words(seed, 3, r).v(1).astype(np.uint64).sum(axis=1)
                           & np.uint64(M32)).astype(np.uint32))


# -- result type and exports ---------------------------------------------------------------------

def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = lc.LanecheckResult(ok=False, rounds=3, waves=48, mismatches=2, first_bad_round=1,
                             bad_stages=["xbar"], cus_covered=3, cu_count=256,
                             elapsed_s=0.5, xbar_gops=1.5, waves_on=[0] * 1024)
    assert res.rate_fields() == ["dpp_gops", "xbar_gops", "sgpr_gops", "scan_gops"]
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"dpp_gops", "xbar_gops", "sgpr_gops", "scan_gops", "mismatches",
            "cus_covered"} <= set(d)
    assert d["xbar_gops"] == 1.5 and d["bad_stages"] == ["xbar"]
    assert lc.metric_args(d) == (2, 3)
    assert lc.DEFAULT_ROUNDS % lc.PERIOD == 0 and lc.PERIOD <= lc.DEFAULT_ROUNDS <= 65536
    assert len(lc._OPS_PER_WAVE_ROUND) == 4 and all(x > 0 for x in lc._OPS_PER_WAVE_ROUND)
    assert probe.LanecheckResult is lc.LanecheckResult
    assert probe.lanecheck_round is lc.lanecheck_round
    assert probe.run_lanecheck_subprocess is lc.run_lanecheck_subprocess
    assert probe.dpp_source is lc.dpp_source


def test_registry():
    assert _active.ALL_PROBES == _active.HEALTH_PROBES + ("lanecheck",)
    assert _active.HEALTH_PROBES == _active.ACTIVE_PROBES + ("atomcheck",)
    assert lc._child_lock is _active._child_lock


def test_run_lanecheck_subprocess_passes_rounds(monkeypatch):
    calls = []

    def fake(cmd, **kw):
        calls.append((list(cmd), kw, _active._child_lock.locked()))
        return subprocess.CompletedProcess(cmd, 1, 'noise\n{"ok": false, "mismatches": 1}\n', "")

    monkeypatch.setattr(_active.subprocess, "run", fake)
    rec = lc.run_lanecheck_subprocess(3, 128, timeout_s=9.0)
    assert rec == {"ok": False, "mismatches": 1, "exit_code": 1}
    cmd, kw, locked = calls[0]
    assert cmd == [sys.executable, "-m", "kubegpu_amd.probe.lanecheck",
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


PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}
FAIL = dict(PASS, ok=False, mismatches=4, first_bad_round=1, bad_stages=["sgpr"],
            bad_cus=["3/1/0/7"])


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.lanecheck_status(uuid) is None

    assert mgr.record_lanecheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.lanecheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.atomcheck_status(uuid) is None and mgr.cucheck_status(uuid) is None
    assert len(lines) == 1 and "lanecheck" in lines[0] and uuid in lines[0]
    assert "3/1/0/7" in lines[0] and "sgpr" in lines[0]

    assert mgr.record_lanecheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    assert _node_info(mgr).allocatable == base.allocatable

    # mismatches alone fail the verdict, even where the result calls itself ok
    assert mgr.record_lanecheck(uuid, dict(PASS, mismatches=1)) is False
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_lanecheck(uuid) is True
    assert mgr.clear_lanecheck(uuid) is False
    assert mgr.lanecheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough, and the six older probes still count
    mgr.record_lanecheck(uuid, PASS)
    mgr.record_atomcheck(uuid, {"ok": False, "mismatches": 1})
    assert mgr.device_health()[uuid] is False
    mgr.clear_atomcheck(uuid)
    assert mgr.device_health()[uuid] is True

    with pytest.raises(KeyError):
        mgr.record_lanecheck("GPU-does-not-exist", FAIL)
    assert set(mgr.lanecheck) == {uuid}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_lanecheck(uuid, FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.lanecheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.lanecheck_status(uuid) is None


# -- lanecheck_round ---------------------------------------------------------------------

def test_round_records_verdicts_and_selects_idle_gpus():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    calls = []

    def runner(index, rounds):
        calls.append((index, rounds))
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = lc.lanecheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.lanecheck_status(by_index[1]) is None
    assert mgr.atomcheck == {} and mgr.cucheck == {}
    assert metrics.gpu_lanecheck[by_index[5]] == {
        "mismatches": 4, "cus_covered": 256,
        "timestamp": metrics.gpu_lanecheck[by_index[5]]["timestamp"]}
    assert metrics.gpu_lanecheck[by_index[0]]["mismatches"] == 0
    assert metrics.gpu_lanecheck_errors == {} and metrics.gpu_atomcheck == {}

    calls.clear()
    lc.lanecheck_round(mgr, runner, None, rounds=8, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_runner_errors_leave_health_untouched_and_count():
    from kubegpu_amd.metrics import Metrics

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_lanecheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, rounds):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("lanecheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        if index == 4:
            return "not a dict"
        if index == 7:  # gone while its child ran
            with mgr._lock:
                del mgr.gpus[by_index[7]]
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = lc.lanecheck_round(mgr, runner, metrics, rounds=8)
    after = mgr.device_health()
    assert by_index[7] not in after
    assert after == {u: h for u, h in before.items() if u != by_index[7]}
    assert mgr.lanecheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2, 4):
        assert mgr.lanecheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_lanecheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3, 4)}
    assert set(metrics.gpu_lanecheck) == {by_index[i] for i in (5, 6)}
    assert by_index[7] not in out and by_index[7] not in mgr.lanecheck


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_lanecheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_lanecheck_error("GPU-a")
        m.inc_lanecheck_error("GPU-a")
        assert m.gpu_lanecheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_lanecheck_errors["GPU-a"] == 2
        assert m.gpu_atomcheck == {} and m.gpu_hostlink_errors == {}
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_lanecheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_lanecheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_lanecheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_lanecheck_errors_total", lab) == 2.0
    assert [row[2] for row in metrics_mod._PROBE_METRICS["lanecheck"]] == [
        "mismatches", "cus_covered", "last_run_timestamp_seconds", "errors_total"]
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_lanecheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--lanecheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--lanecheck needs real GPUs" in cap.err and "cross-lane" in cap.err
    assert cap.out == ""
    assert amddevs._PROBE_RUNS["lanecheck"][3] == ("mismatches",)


def test_amddevs_lanecheck_exit_codes_with_a_fake_backend(monkeypatch, capsys):
    from kubegpu_amd.cli import amddevs

    results = {}
    seen = []

    def fake_round(mgr, runner, metrics, rounds, max_process_count):
        seen.append((runner, metrics, rounds, max_process_count, len(mgr.gpus)))
        return results

    monkeypatch.setattr(lc, "lanecheck_round", fake_round)
    backend = FakeBackend(fixtures.fixture_8x_mi355x())
    args = amddevs.argparse.Namespace(fake=False, rounds=8, memcheck_idle_only=False)
    results["GPU-a"] = dict(PASS)
    assert amddevs._run_probe("lanecheck", args, backend) == 0
    assert seen[0] == (lc.run_lanecheck_subprocess, None, 8, None, 8)
    assert json.loads(capsys.readouterr().out) == results
    results["GPU-b"] = dict(FAIL)
    assert amddevs._run_probe("lanecheck", args, backend) == 1
    results.clear()
    results["GPU-a"] = {"error": "x", "exit_code": 2}
    assert amddevs._run_probe("lanecheck", args, backend) == 2
    args.rounds = None  # the probe's own default
    amddevs._run_probe("lanecheck", args, backend)
    assert seen[-1][2] == lc.DEFAULT_ROUNDS
    capsys.readouterr()


def test_amddevs_health_shows_the_row(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["lanecheck"] is None for r in rows.values())
    assert all("atomcheck" in r and "fpcheck" in r for r in rows.values())


def test_agent_oneshot_accepts_lanecheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--lanecheck-interval", "600", "--lanecheck-rounds", "64",
                              "--lanecheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_lanecheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert lc.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
