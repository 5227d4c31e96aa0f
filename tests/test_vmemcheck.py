"""vmemcheck without a GPU: the numpy reference's shape, period and digest,
the address tag, what the address tables promise (checked on the
reference alone over one period and two seeds: every address inside its
region, every partially stored byte stored once, every byte lane with
both signs, every buffer access wholly on one side of num_records), and
the plumbing from verdict to health, metrics, agent and CLI with fake
runners."""

import functools
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.probe import _active
from kubegpu_amd.probe import vmemcheck as vm

M32 = 0xFFFFFFFF
ROUNDS = np.arange(vm.PERIOD, dtype=np.uint32)
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref_period(seed, stage):
    """Every slot of a stage over one period: ((name, uint32 [64, 64]), ...)."""
    return tuple(vm._stage(seed, stage, ROUNDS))


@functools.lru_cache(maxsize=None)
def table(seed, rounds):
    a = vm.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


# -- reference digests ----------------------------------------------------------------------

def test_reference_digests_shape_period_and_seed():
    a = table(0, 2 * vm.PERIOD + 3)
    assert a.shape == (2 * vm.PERIOD + 3, 4) and a.dtype == np.uint32
    assert np.array_equal(a, vm.reference_digests(0, 2 * vm.PERIOD + 3))  # deterministic
    assert np.array_equal(a[vm.PERIOD:2 * vm.PERIOD], a[:vm.PERIOD])  # wraps at PERIOD
    assert np.array_equal(a[2 * vm.PERIOD:], a[:3])
    assert len(set(a[:vm.PERIOD].reshape(-1).tolist())) == 4 * vm.PERIOD  # stage and round
    assert np.array_equal(vm.reference_digests(0, 5), a[:5])
    assert not (a[:4] == vm.reference_digests(1, 4)).any()  # every digest depends on the seed
    assert np.array_equal(vm.reference_digests(1 << 32, 2), a[:2])  # seed is a u32
    assert vm.reference_digests(0, 0).shape == (0, 4)
    with pytest.raises(ValueError):
        vm.reference_digests(0, -1)


@pytest.mark.parametrize("stage", range(4))
def test_digest_of_the_values_is_the_table_and_sees_every_slot(stage):
    for r in (0, 1, vm.PERIOD - 1):
        values = vm.reference_values(0, stage, r)
        assert list(values) == vm.slot_table(stage)
        assert all(v.shape == (64,) and v.dtype == np.uint32 for v in values.values())
        assert vm.digest_of(values) == int(table(0, vm.PERIOD)[r, stage])
    assert len(values) <= vm._VALUE_ROWS
    # the period wrap of the values themselves
    again = vm.reference_values(0, stage, r + vm.PERIOD)
    assert all(np.array_equal(again[k], values[k]) for k in values)
    # one flipped bit of one slot changes this stage's digest, whichever slot
    want = vm.digest_of(values)
    for n, name in enumerate(values):
        rows = [v.copy() for v in values.values()]
        rows[n][(7 * n) % 64] ^= np.uint32(1 << (n % 32))
        assert vm.digest_of(rows) != want, name
    # and no other stage's: the stages share nothing but the seed
    others = [int(table(0, vm.PERIOD)[r, s]) for s in range(4) if s != stage]
    assert [vm.digest_of(vm.reference_values(0, s, r)) for s in range(4) if s != stage] == others


def test_reference_values_reject_bad_arguments():
    with pytest.raises(ValueError, match="vmemcheck: stage"):
        vm.reference_values(0, 4, 0)
    with pytest.raises(ValueError, match="vmemcheck: round"):
        vm.reference_values(0, 0, 65536)


def test_a_flipped_byte_or_two_swapped_addresses_change_the_digest(monkeypatch):
    """The digest sees the modelled memory: flip one byte of what the
    partial stage left behind, or let two dwords answer for each other."""
    want = int(table(0, 1)[0, 2])
    load = vm._Bytes.load_dwords

    def flipped(self, byte, n):
        if self.what == "the partial region" and not getattr(self, "_done", False):
            self.mem[:, 777] ^= 0x10
            self._done = True
        return load(self, byte, n)

    monkeypatch.setattr(vm._Bytes, "load_dwords", flipped)
    assert vm.digest_of(vm.reference_values(0, 2, 0)) != want
    assert int(vm.reference_digests(0, 1)[0, 2]) != want

    def swapped(self, byte, n):
        if self.what == "the partial region" and not getattr(self, "_done", False):
            a, b = self.mem[:, 400:404].copy(), self.mem[:, 1200:1204].copy()
            self.mem[:, 400:404], self.mem[:, 1200:1204] = b, a
            self._done = True
        return load(self, byte, n)

    monkeypatch.setattr(vm._Bytes, "load_dwords", swapped)
    assert vm.digest_of(vm.reference_values(0, 2, 0)) != want
    monkeypatch.setattr(vm._Bytes, "load_dwords", load)
    assert vm.digest_of(vm.reference_values(0, 2, 0)) == want


# -- the address tag and the table -------------------------------------------------------------

def _fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def test_tag_is_injective_and_sees_every_address_bit():
    a = np.arange(1 << 18, dtype=np.uint32)  # the default grid's arena is 2**24 dwords
    t = vm.tag(a)
    assert t.dtype == np.uint32 and len(np.unique(t)) == len(a)
    for x in (0, 1, 4095, 4096, (1 << 28) - 1):  # the last dword of the largest arena
        assert vm.tag(x) == _fmix(0xA5A5A5A5 ^ ((x * 0x9E3779B9) & M32))
    for k in range(28):  # every bit of an arena dword index
        assert (t ^ vm.tag(a ^ np.uint32(1 << k))).all(), k
    # a narrow store takes the matching bytes, and none of them is always 0
    for shift in (0, 8, 16, 24):
        assert len(np.unique((t >> np.uint32(shift)) & np.uint32(0xFF))) == 256


def test_source_table_and_layout():
    x = vm.source_table(0)
    assert x.shape == (vm.X_DWORDS,) == (65536,) and x.dtype == np.uint32
    assert len(np.unique(x)) > 65000
    assert not np.array_equal(x, vm.source_table(1))
    assert np.array_equal(x, vm.source_table(1 << 32))
    assert vm.SPAN_DWORDS == 4096 and vm.PERIOD == 64 and vm._STAGE0 == 40 and vm._STAGE_X == 44
    assert vm.REGIONS == {"width": (0, 1024), "partial": (1024, 512), "buffer": (2048, 1024)}
    assert vm.GATHER_STRIDES == (0, 1, 2, 3, 8, 16, 33)
    assert vm.POLICIES == ("plain", "sc1", "nt")


def test_inputs_differ_from_the_other_probes():
    from kubegpu_amd.probe import atomcheck as at
    from kubegpu_amd.probe import lanecheck as lc
    from kubegpu_amd.probe import ldscheck as ld

    r0 = np.array([0], dtype=np.uint32)
    mine = {tuple(vm._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    assert len(mine) == 4
    theirs = {tuple(ld._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    theirs |= {tuple(lc._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    assert not mine & theirs
    stages = set(range(vm._STAGE0, vm._STAGE0 + 4)) | {vm._STAGE_X}
    assert len(stages) == 5
    assert not stages & (set(range(ld._STAGE0, ld._STAGE0 + 4)) | {ld._STAGE_G, ld._STAGE_X})
    assert not stages & set(range(lc._STAGE0, lc._STAGE0 + 4))
    assert not stages & set(range(at._STAGE0, at._STAGE0 + 6))


# -- addresses ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_every_address_lies_inside_its_region_or_inside_x(seed, monkeypatch):
    """The reference raises where an address leaves its array; here every
    address it forms over one period is also recorded and checked."""
    seen = {}
    check = vm._Bytes._addr

    def recording(self, addr, nbytes):
        out = check(self, addr, nbytes)
        lo, hi = seen.get(self.what, (1 << 62, -1))
        seen[self.what] = (min(lo, int(out.min())), max(hi, int(out.max()) + nbytes))
        return out

    monkeypatch.setattr(vm._Bytes, "_addr", recording)
    for stage in range(4):
        vm._stage(seed, stage, ROUNDS)
    assert set(seen) == {"the width region", "the table X", "the partial region",
                         "the buffer region"}
    for what, size in (("the width region", 4096), ("the partial region", 2048),
                       ("the buffer region", 4096), ("the table X", vm.X_BYTES)):
        lo, hi = seen[what]
        assert 0 <= lo and hi <= size, (what, lo, hi)
    assert seen["the buffer region"] == (0, 4096) and seen["the partial region"] == (0, 2048)
    assert seen["the table X"][1] > vm.X_BYTES - 4096  # the gathers reach the table's end
    # the regions lie inside the span, one behind the other, and the rest is unused
    spans = sorted(vm.REGIONS.values())
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))
    assert spans[-1][0] + spans[-1][1] <= vm.SPAN_DWORDS


def test_the_reference_raises_outside_a_region():
    mem = vm._region("partial", 1)
    with pytest.raises(ValueError, match="outside the partial region"):
        mem.load(np.full(64, 2048 - 3), 4)
    with pytest.raises(ValueError, match="outside the partial region"):
        mem.store(np.full(64, -1), np.zeros((1, 64), dtype=np.uint32), 1)
    mem.load(np.full(64, 2048 - 4), 4)


# -- stage width --------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_narrow_accesses_reach_every_byte_lane_and_both_signs_in_every_round(seed):
    b8, b16 = vm.subdword_offsets(seed, ROUNDS)
    assert b8.shape == b16.shape == (vm.PERIOD, 2, 64)
    slots = dict(ref_period(seed, 0))
    lane = np.arange(64)
    for j in range(2):
        for r in range(vm.PERIOD):
            # byte lane x top bit of the stored byte: all eight combinations
            assert len(set(zip(b8[r, j].tolist(), ((lane >> 2) & 1).tolist()))) == 8
            assert len(set(zip(b16[r, j].tolist(), ((lane >> 1) & 1).tolist()))) == 4
        u8, i8 = slots[f"b8.{j}.u8"], slots[f"b8.{j}.i8"]
        assert (u8 < 256).all() and ((u8 >= 128).any(axis=1) & (u8 < 128).any(axis=1)).all()
        top = i8 >> np.uint32(8)
        assert set(np.unique(top).tolist()) == {0, 0xFFFFFF}
        assert ((top == 0).any(axis=1) & (top != 0).any(axis=1)).all()
        assert np.array_equal(top != 0, (i8 & np.uint32(0x80)) != 0)  # the sign, extended
        u16, i16 = slots[f"b16.{j}.u16"], slots[f"b16.{j}.i16"]
        assert (u16 < 65536).all()
        assert ((u16 >= 32768).any(axis=1) & (u16 < 32768).any(axis=1)).all()
        top = i16 >> np.uint32(16)
        assert set(np.unique(top).tolist()) == {0, 0xFFFF}
        assert ((top == 0).any(axis=1) & (top != 0).any(axis=1)).all()
        assert np.array_equal(top != 0, (i16 & np.uint32(0x8000)) != 0)


def test_a_narrow_store_changes_its_bytes_and_nothing_else():
    W = vm._Words(0, 0, ROUNDS)
    img = W.img()
    slots = dict(ref_period(0, 0))
    b8, b16 = vm.subdword_offsets(0, ROUNDS)
    lane = np.arange(64)
    first = slots["b8.0.dword"] ^ img[:, 2 * lane]
    mask = np.uint32(0xFF) << (8 * b8[:, 0]).astype(np.uint32)
    assert not (first & ~mask).any() and first.any()
    assert np.array_equal(slots["b8.0.next"], img[:, 2 * lane + 1])  # its neighbour: intact
    assert np.array_equal(slots["b8.1.dword"], slots["b8.0.dword"])
    second = slots["b8.1.next"] ^ img[:, 2 * lane + 1]
    mask = np.uint32(0xFF) << (8 * b8[:, 1]).astype(np.uint32)
    assert not (second & ~mask).any() and second.any()
    first = slots["b16.0.dword"] ^ img[:, 128 + 2 * lane]
    mask = np.uint32(0xFFFF) << (16 * b16[:, 0]).astype(np.uint32)
    assert not (first & ~mask).any() and first.any()
    assert np.array_equal(slots["b16.0.next"], img[:, 129 + 2 * lane])
    # the 16-byte load over the 12-byte store: three stored dwords, then the fill
    assert np.array_equal(slots["b96.b128.3"],
                          np.take_along_axis(img, 384 + 4 * W.rot(13) + 3, axis=1))
    assert np.array_equal(slots["b96.b128.0"], np.take_along_axis(W.v(9), W.rot(13), axis=1))
    assert np.array_equal(slots["b96.2"], np.take_along_axis(W.v(11), W.rot(12), axis=1))
    assert np.array_equal(slots["b128.3"], np.take_along_axis(W.v(17), W.rot(18), axis=1))
    assert np.array_equal(slots["b64.1"], np.take_along_axis(W.v(8), W.rot(6), axis=1))


# -- stage gather -------------------------------------------------------------------------------

def test_gathers_cover_strides_widths_policies_and_the_scalar_path():
    names = vm.slot_table(1)
    plan = vm.gather_plan(0, ROUNDS)
    assert len(plan) == 24 and len(names) == 66
    assert [(w, p) for _, w, p, _ in plan[:7]] == [
        (4, p) for p in ("plain", "sc1", "nt", "plain", "sc1", "nt", "plain")]
    X = vm.source_table(0)
    slots = dict(ref_period(0, 1))
    n = 0
    for name, width, policy, unit in plan:
        assert policy == vm.POLICIES[n % 3] and unit.shape == (vm.PERIOD, 64)
        assert unit.min() >= 0 and unit.max() < vm.X_BYTES // width
        for c in range(width // 4):
            key = f"{name}.{policy}.{c}" if width > 4 else f"{name}.{policy}"
            assert names[n] == key
            assert np.array_equal(slots[key], X[(width // 4) * unit + c])
            n += 1
    assert n == 56
    for width in vm.GATHER_WIDTHS:  # every width is read under every policy
        assert {p for _, w, p, _ in plan if w == width} == set(vm.POLICIES)
    lane = np.arange(64)
    by_name = {name: unit for name, _, _, unit in plan}
    assert (by_name["b32.s0"] == by_name["b32.s0"][:, :1]).all()  # all lanes on one address
    assert ((by_name["b128.s1"] - by_name["b128.s1"][:, :1]) % (vm.X_BYTES // 16)
            == lane[None, :]).all()  # lane-linear
    s8 = (by_name["b128.s8"] * 16) // 128  # one 128-byte line per lane
    assert all(len(np.unique(row)) == 64 for row in s8)
    assert any(len(np.unique(row)) < 64 for row in by_name["b32.free"] // 32)  # lines collide
    # narrow gathers: both signs in every round, extended from the right bit
    u8, i8, u16, i16 = (slots[k] for k in ("u8", "i8", "u16", "i16"))
    assert (u8 < 256).all() and (u16 < 65536).all()
    assert ((i8 >> np.uint32(8) == 0xFFFFFF) == ((i8 & np.uint32(0x80)) != 0)).all()
    assert ((i16 >> np.uint32(16) == 0xFFFF) == ((i16 & np.uint32(0x8000)) != 0)).all()
    for a in (i8, i16):
        neg = a >= np.uint32(1 << 31)
        assert (neg.any(axis=1) & (~neg).any(axis=1)).all()
    # uniform loads: lane l holds dword l mod n of a naturally aligned block
    W = vm._Words(0, 1, ROUNDS)
    for j, nd in enumerate(vm.UNIFORM_DWORDS[:-1]):
        index = (W.u(28 + j) % np.uint32(vm.X_DWORDS // nd)).astype(np.int64)
        assert np.array_equal(slots[f"uniform.x{nd}"], X[nd * index[:, None] + lane % nd])
    first = (W.u(28) % np.uint32(vm.X_DWORDS)).astype(np.int64)
    assert np.array_equal(slots["uniform.x16"], X[16 * (first // 16)[:, None] + lane % 16])
    # the block of the last holds the dword of the first; scalar and vector agree
    assert (slots["uniform.x16"][np.arange(vm.PERIOD), first % 16]
            == slots["uniform.x1"][:, 0]).all()
    assert np.array_equal(slots["uniform.x16.vector"], slots["uniform.x16"])
    assert names[-6:] == ["uniform.x1", "uniform.x2", "uniform.x4", "uniform.x8", "uniform.x16",
                          "uniform.x16.vector"]


# -- stage partial ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_partial_stores_are_bijections_and_no_byte_is_stored_twice(seed):
    rows = vm.partial_rows(seed, ROUNDS)
    ident = np.arange(64)[None, :]
    for j in range(4):
        assert (np.sort(rows["byte"][:, j], axis=1) == ident).all()
        assert (np.sort(rows["dword"][:, j], axis=1) == 128 + 64 * j + ident).all()
    for j in range(2):
        assert (np.sort(rows["half"][:, j], axis=1) == 64 + ident).all()
    assert (np.sort(rows["b64"], axis=1) == 384 + 2 * ident).all()
    # every byte of the 512 dwords, counted over all stores between the fences
    count = np.zeros((vm.PERIOD, 2048), dtype=np.int64)
    r = np.arange(vm.PERIOD)[:, None]
    for j in range(4):
        np.add.at(count, (r, 4 * rows["byte"][:, j] + rows["byte_lane"][:, j]), 1)
    for j in range(2):
        for b in range(2):
            np.add.at(count, (r, 4 * rows["half"][:, j] + 2 * rows["half_lane"][:, j] + b), 1)
    for j in range(4):
        for b in range(4):
            np.add.at(count, (r, 4 * rows["dword"][:, j] + b), 1)
    for b in range(8):
        np.add.at(count, (r, 4 * rows["b64"] + b), 1)
    assert (count == 1).all()  # each byte once: never twice, and none left to the fill
    # dwords 0 .. 63 are assembled from four different lanes in most dwords
    lanes = np.empty((vm.PERIOD, 4, 64), dtype=np.int64)
    for j in range(4):
        np.put_along_axis(lanes[:, j], rows["byte"][:, j], np.broadcast_to(ident, (64, 64)), axis=1)
    distinct = np.array([[len(set(lanes[q, :, d])) for d in range(64)] for q in range(vm.PERIOD)])
    assert (distinct >= 2).all() and (distinct == 4).mean() > 0.8
    assert vm.PARTIAL_POLICIES == ("plain", "sc1", "nt", "plain")


def test_partial_readbacks_find_what_the_lanes_stored():
    slots = dict(ref_period(0, 2))
    rows = vm.partial_rows(0, ROUNDS)
    W = vm._Words(0, 2, ROUNDS)
    names = vm.slot_table(2)
    assert names == [f"{p}.t{t}.{c}" for p in ("plain", "sc1") for t in (0, 1) for c in range(4)]
    # lane-linear images: dword 4 (64 t + l) + c
    image = np.empty((vm.PERIOD, 512), dtype=np.uint32)
    for t in range(2):
        for c in range(4):
            image[:, 256 * t + c:256 * (t + 1):4] = slots[f"plain.t{t}.{c}"]
            assert np.array_equal(slots[f"sc1.t{t}.{c}"], slots[f"plain.t{t}.{c}"])
    r = np.arange(vm.PERIOD)[:, None]
    for j in range(4):
        assert np.array_equal(image[r, rows["dword"][:, j]], W.v(16 + j))
        got = (image[r, rows["byte"][:, j]] >> (8 * rows["byte_lane"][:, j]).astype(np.uint32))
        assert np.array_equal(got & np.uint32(0xFF), W.v(4 + j) & np.uint32(0xFF))
    for j in range(2):
        got = image[r, rows["half"][:, j]] >> (16 * rows["half_lane"][:, j]).astype(np.uint32)
        assert np.array_equal(got & np.uint32(0xFFFF), W.v(10 + j) & np.uint32(0xFFFF))
    assert np.array_equal(image[r, rows["b64"] + 1], W.v(22))
    assert not np.array_equal(image, W.img(512))


# -- stage buffer -------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_buffer_accesses_lie_wholly_on_one_side_of_num_records(seed):
    plan = vm.buffer_plan(seed, ROUNDS)
    N = plan["num_records"]
    assert N.shape == (vm.PERIOD,) and not (N % 16).any()
    assert N.min() >= 1536 and N.max() <= 3056 and len(np.unique(N)) > 20
    assert [w for _, w in plan["loads"].values()] == list(vm.BUFFER_WIDTHS)
    assert list(plan["loads"]) == ["load.b8", "load.b16", "load.b32", "load.b64", "load.b96",
                                   "load.b128"]
    for name, (at, w) in list(plan["loads"].items()) + list(plan["stores"].items()):
        assert at.shape == (vm.PERIOD, 64) and at.min() >= 0 and at.max() + w <= 4096, name
        assert not (at % (4 if w == 12 else w)).any(), name  # naturally aligned, b96 to 4
        assert (at // 16 == (at + w - 1) // 16).all(), name  # inside one 16-byte cell
        below, above = at + w <= N[:, None], at >= N[:, None]
        assert (below | above).all(), name
        # lanes on both sides in every round
        assert (below.any(axis=1) & above.any(axis=1)).all(), name
    assert all(s >= 4 for s in vm.BUFFER_STRIDES) and len(vm.BUFFER_STRIDES) == 6
    # the variants with an soffset or an immediate offset: in range whatever counts
    assert set(plan["offset_loads"]) == {"load.b32.soffset", "load.b128.imm"}
    for name, (at, w) in plan["offset_loads"].items():
        assert at.min() >= 0 and at.max() + w <= 1536 <= N.min(), name
    # the stores: bijective cells over the whole region, no byte twice
    count = np.zeros((vm.PERIOD, 4096), dtype=np.int64)
    r = np.arange(vm.PERIOD)[:, None]
    for name, (at, w) in plan["stores"].items():
        for b in range(w):
            np.add.at(count, (r, at + b), 1)
        cells = at // 16
        assert all(len(np.unique(row)) == 64 for row in cells), name
        assert cells.min() < 4 and cells.max() >= 252, name
    assert count.max() == 1


def test_buffer_reference_returns_zero_beyond_num_records_and_drops_stores():
    slots = dict(ref_period(0, 3))
    plan = vm.buffer_plan(0, ROUNDS)
    N = plan["num_records"][:, None]
    W = vm._Words(0, 3, ROUNDS)
    img = W.img()
    r = np.arange(vm.PERIOD)[:, None]
    at, _ = plan["loads"]["load.b32"]
    assert np.array_equal(slots["load.b32"], np.where(at < N, img[r, at // 4], 0))
    at, _ = plan["loads"]["load.b128"]
    for c in range(4):
        assert np.array_equal(slots[f"load.b128.{c}"], np.where(at < N, img[r, at // 4 + c], 0))
    at, _ = plan["loads"]["load.b8"]
    want = (img[r, at // 4] >> (8 * (at % 4)).astype(np.uint32)) & np.uint32(0xFF)
    assert np.array_equal(slots["load.b8"], np.where(at < N, want, 0))
    at, _ = plan["offset_loads"]["load.b32.soffset"]
    assert np.array_equal(slots["load.b32.soffset"], img[r, at // 4])
    # the read-back: new values below num_records, the image above
    image = np.empty((vm.PERIOD, 1024), dtype=np.uint32)
    for t in range(4):
        for c in range(4):
            image[:, 256 * t + c:256 * (t + 1):4] = slots[f"readback.t{t}.{c}"]
    above = np.arange(1024)[None, :] >= N // 4
    assert np.array_equal(image[above], img[above])
    at, _ = plan["stores"]["store.b32"]
    kept = at < N
    assert np.array_equal(image[r, at // 4][kept], W.v(25)[kept])
    assert kept.any() and (~kept).any()
    assert (image != img).sum(axis=1).min() >= 24 * 5  # b128 and b32 landed below N
    assert len(vm.slot_table(3)) == 33


# -- result type and exports ---------------------------------------------------------------------

def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = vm.VmemcheckResult(ok=False, rounds=3, waves=48, mismatches=2, first_bad_round=1,
                             bad_stages=["gather"], cus_covered=3, cu_count=256,
                             elapsed_s=0.5, gather_gbps=1.5, waves_on=[0] * 1024)
    assert res.rate_fields() == ["width_gbps", "gather_gbps", "partial_gbps", "buffer_gbps"]
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"width_gbps", "gather_gbps", "partial_gbps", "buffer_gbps", "mismatches",
            "cus_covered"} <= set(d)
    assert d["gather_gbps"] == 1.5 and d["bad_stages"] == ["gather"]
    assert vm.metric_args(d) == (2, 3)
    assert vm.DEFAULT_ROUNDS % vm.PERIOD == 0 and vm.PERIOD <= vm.DEFAULT_ROUNDS <= 65536
    assert len(vm._BYTES_PER_WAVE_ROUND) == 4 and all(x > 0 for x in vm._BYTES_PER_WAVE_ROUND)
    assert vm.STAGES == ("width", "gather", "partial", "buffer")
    assert probe.VmemcheckResult is vm.VmemcheckResult
    assert probe.vmemcheck_round is vm.vmemcheck_round
    assert probe.run_vmemcheck_subprocess is vm.run_vmemcheck_subprocess
    assert probe.source_table is vm.source_table


def test_registry():
    assert _active.PROBE_NAMES[:len(_active.PROBES)] == _active.PROBES
    assert "vmemcheck" in _active.PROBE_NAMES
    assert len(set(_active.PROBE_NAMES)) == len(_active.PROBE_NAMES)
    assert vm._child_lock is _active._child_lock


def test_run_vmemcheck_subprocess_passes_rounds(monkeypatch):
    calls = []

    def fake(cmd, **kw):
        calls.append((list(cmd), kw, _active._child_lock.locked()))
        return subprocess.CompletedProcess(cmd, 1, 'noise\n{"ok": false, "mismatches": 1}\n', "")

    monkeypatch.setattr(_active.subprocess, "run", fake)
    rec = vm.run_vmemcheck_subprocess(3, 128, timeout_s=9.0)
    assert rec == {"ok": False, "mismatches": 1, "exit_code": 1}
    cmd, kw, locked = calls[0]
    assert cmd == [sys.executable, "-m", "kubegpu_amd.probe.vmemcheck",
                   "--device", "3", "--rounds", "128"]
    assert locked and kw["timeout"] == 9.0


def test_bad_arguments_raise_before_the_extension_is_loaded(monkeypatch):
    monkeypatch.setattr(vm, "_ext", lambda: pytest.fail("loaded the extension"))
    for kwargs in (dict(rounds=0), dict(rounds=65537), dict(blocks=-1), dict(blocks=4097),
                   dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError, match="vmemcheck"):
            vm.vmemcheck(**kwargs)


# -- manager verdicts ------------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}
FAIL = dict(PASS, ok=False, mismatches=4, first_bad_round=1, bad_stages=["buffer"],
            bad_cus=["3/1/0/7"])


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[2]
    assert mgr.vmemcheck_status(uuid) is None

    assert mgr.record_vmemcheck(uuid, PASS) is True  # clean
    assert mgr.device_health()[uuid] is True and lines == []

    assert mgr.record_vmemcheck(uuid, FAIL) is False  # a mismatch: Unhealthy
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    st = mgr.vmemcheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.ldscheck_status(uuid) is None and mgr.cucheck_status(uuid) is None
    assert len(lines) == 1 and "vmemcheck" in lines[0] and uuid in lines[0]
    assert "3/1/0/7" in lines[0] and "buffer" in lines[0]

    assert mgr.record_vmemcheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    # mismatches alone fail the verdict, even where the result calls itself ok
    assert mgr.record_vmemcheck(uuid, dict(PASS, mismatches=1)) is False
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_vmemcheck(uuid) is True
    assert mgr.clear_vmemcheck(uuid) is False
    assert mgr.vmemcheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough, and the eight older probes still count
    mgr.record_vmemcheck(uuid, PASS)
    mgr.record_ldscheck(uuid, {"ok": False, "mismatches": 1})
    assert mgr.device_health()[uuid] is False
    mgr.clear_ldscheck(uuid)
    assert mgr.device_health()[uuid] is True
    with pytest.raises(KeyError):
        mgr.record_vmemcheck("GPU-does-not-exist", FAIL)
    assert set(mgr.vmemcheck) == {uuid}


def test_verdict_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_vmemcheck(uuid, FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False
    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.vmemcheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished and mgr.vmemcheck_status(uuid) is None


def test_round_records_verdicts_and_exit_code_2_leaves_health_alone():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    mgr.record_vmemcheck(by_index[3], FAIL)  # an earlier verdict must stay
    calls = []

    def runner(index, rounds):
        calls.append((index, rounds))
        if index == 0:
            raise RuntimeError("boom")
        if index in (3, 4):
            return {"error": "no GPU visible", "exit_code": 2}
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = vm.vmemcheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    health = mgr.device_health()
    assert health[by_index[5]] is False and health[by_index[3]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 4, 6, 7))
    for i in (0, 4):
        assert mgr.vmemcheck_status(by_index[i]) is None and out[by_index[i]]["exit_code"] == 2
    assert mgr.vmemcheck_status(by_index[3])["mismatches"] == 4
    assert mgr.ldscheck == {} and mgr.cucheck == {}
    assert metrics.gpu_vmemcheck[by_index[5]] == {
        "mismatches": 4, "cus_covered": 256,
        "timestamp": metrics.gpu_vmemcheck[by_index[5]]["timestamp"]}
    assert set(metrics.gpu_vmemcheck) == {by_index[i] for i in (5, 6, 7)}
    assert metrics.gpu_vmemcheck_errors == {by_index[i]: 1 for i in (0, 3, 4)}
    assert metrics.gpu_ldscheck == {}


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_vmemcheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_vmemcheck_error("GPU-a")
        m.inc_vmemcheck_error("GPU-a")
        assert m.gpu_vmemcheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_vmemcheck_errors["GPU-a"] == 2
        assert m.gpu_ldscheck == {} and m.gpu_hostlink_errors == {}
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        from prometheus_client import generate_latest

        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_vmemcheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_vmemcheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_vmemcheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_vmemcheck_errors_total", lab) == 2.0
        text = generate_latest(reg).decode()
        assert 'kubegpu_amd_gpu_vmemcheck_mismatches{uuid="GPU-a"} 2.0' in text
        assert "# HELP kubegpu_amd_gpu_vmemcheck_cus_covered" in text
    assert [row[2] for row in metrics_mod._PROBE_METRICS["vmemcheck"]] == [
        "mismatches", "cus_covered", "last_run_timestamp_seconds", "errors_total"]
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_vmemcheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--vmemcheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--vmemcheck needs real GPUs" in cap.err and "vector-memory" in cap.err
    assert cap.out == ""
    assert amddevs._PROBE_RUNS["vmemcheck"][3] == ("mismatches",)


def test_amddevs_help_names_the_probe(capsys):
    from kubegpu_amd.cli import amddevs

    with pytest.raises(SystemExit) as e:
        amddevs.main(["--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--vmemcheck" in out and "buffer range check" in " ".join(out.split())


def test_amddevs_vmemcheck_exit_codes_with_a_fake_backend(monkeypatch, capsys):
    from kubegpu_amd.cli import amddevs

    results = {}
    seen = []

    def fake_round(mgr, runner, metrics, rounds, max_process_count):
        seen.append((runner, metrics, rounds, max_process_count, len(mgr.gpus)))
        return results

    monkeypatch.setattr(vm, "vmemcheck_round", fake_round)
    backend = FakeBackend(fixtures.fixture_8x_mi355x())
    args = amddevs.argparse.Namespace(fake=False, rounds=8, memcheck_idle_only=False)
    results["GPU-a"] = dict(PASS)
    assert amddevs._run_probe("vmemcheck", args, backend) == 0
    assert seen[0] == (vm.run_vmemcheck_subprocess, None, 8, None, 8)
    assert json.loads(capsys.readouterr().out) == results
    results["GPU-b"] = dict(FAIL)
    assert amddevs._run_probe("vmemcheck", args, backend) == 1
    results.clear()
    results["GPU-a"] = {"error": "x", "exit_code": 2}
    assert amddevs._run_probe("vmemcheck", args, backend) == 2
    args.rounds = None  # the probe's own default
    amddevs._run_probe("vmemcheck", args, backend)
    assert seen[-1][2] == vm.DEFAULT_ROUNDS
    capsys.readouterr()


def test_amddevs_health_shows_the_row(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["vmemcheck"] is None for r in rows.values())
    assert all("ldscheck" in r and "atomcheck" in r for r in rows.values())


def test_agent_oneshot_accepts_vmemcheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--vmemcheck-interval", "600", "--vmemcheck-rounds", "64",
                              "--vmemcheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_vmemcheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert vm.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
