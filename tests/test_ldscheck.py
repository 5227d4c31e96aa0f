"""ldscheck without a GPU: the numpy reference's shape, period and digest,
the address tag, the coverage the address tables promise (checked on the
reference alone over one period), the transposed read on a hand-written
block, and the plumbing from verdict to health, metrics, agent and CLI
with fake runners."""

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
from kubegpu_amd.probe import ldscheck as ld

M32 = 0xFFFFFFFF
ROUNDS = np.arange(ld.PERIOD, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def ref_period(seed, stage):
    """Every slot of a stage over one period: ((name, uint32 [64, 64]), ...)."""
    return tuple(ld._stage(seed, stage, ROUNDS))


@functools.lru_cache(maxsize=None)
def table(seed, rounds):
    a = ld.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


# -- reference digests ----------------------------------------------------------------------

def test_reference_digests_shape_period_and_seed():
    a = table(0, 2 * ld.PERIOD + 3)
    assert a.shape == (2 * ld.PERIOD + 3, 4) and a.dtype == np.uint32
    assert np.array_equal(a, ld.reference_digests(0, 2 * ld.PERIOD + 3))  # deterministic
    assert np.array_equal(a[ld.PERIOD:2 * ld.PERIOD], a[:ld.PERIOD])  # wraps at PERIOD
    assert np.array_equal(a[2 * ld.PERIOD:], a[:3])
    assert len(set(a[:ld.PERIOD].reshape(-1).tolist())) == 4 * ld.PERIOD  # stage and round
    assert np.array_equal(ld.reference_digests(0, 5), a[:5])
    assert not (a[:4] == ld.reference_digests(1, 4)).any()  # every digest depends on the seed
    assert np.array_equal(ld.reference_digests(1 << 32, 2), a[:2])  # seed is a u32
    assert ld.reference_digests(0, 0).shape == (0, 4)
    with pytest.raises(ValueError):
        ld.reference_digests(0, -1)


@pytest.mark.parametrize("stage", range(4))
def test_digest_of_the_values_is_the_table_and_sees_every_slot(stage):
    for r in (0, 1, ld.PERIOD - 1):
        values = ld.reference_values(0, stage, r)
        assert list(values) == ld.slot_table(stage)
        assert all(v.shape == (64,) and v.dtype == np.uint32 for v in values.values())
        assert ld.digest_of(values) == int(table(0, ld.PERIOD)[r, stage])
    assert len(values) <= ld._VALUE_ROWS
    # one flipped bit of one slot changes this stage's digest, whichever slot
    want = ld.digest_of(values)
    for n, name in enumerate(values):
        rows = [v.copy() for v in values.values()]
        rows[n][(7 * n) % 64] ^= np.uint32(1 << (n % 32))
        assert ld.digest_of(rows) != want, name
    # and no other stage's: the stages share nothing but the seed
    others = [int(table(0, ld.PERIOD)[r, s]) for s in range(4) if s != stage]
    assert [ld.digest_of(ld.reference_values(0, s, r)) for s in range(4) if s != stage] == others


def test_reference_values_reject_bad_arguments():
    with pytest.raises(ValueError, match="ldscheck: stage"):
        ld.reference_values(0, 4, 0)
    with pytest.raises(ValueError, match="ldscheck: round"):
        ld.reference_values(0, 0, 65536)


# -- the address tag -------------------------------------------------------------------------

def _fmix(h):
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    return h ^ (h >> 16)


def test_tag_is_injective_and_sees_every_address_bit():
    a = np.arange(ld.LDS_DWORDS, dtype=np.uint32)
    assert ld.LDS_DWORDS == 40960 == 16 * ld.SLICE_DWORDS
    t = ld.tag(a)
    assert t.dtype == np.uint32 and len(np.unique(t)) == ld.LDS_DWORDS
    for x in (0, 1, 2559, 2560, 40959):
        assert ld.tag(x) == int(t[x]) == _fmix(0xA5A5A5A5 ^ ((x * 0x9E3779B9) & M32))
    for k in range(16):  # 2**16 > 40960: every bit of a dword address
        assert (t ^ ld.tag(a ^ np.uint32(1 << k))).all(), k
    # a narrow store takes the matching bytes, and none of them is always 0
    for shift in (0, 8, 16, 24):
        assert len(np.unique((t >> np.uint32(shift)) & np.uint32(0xFF))) == 256


def test_source_tables_carry_the_tag_of_the_slice_they_go_to():
    t = ld.source_tables(0)
    assert t.shape == (ld.TABLE_DWORDS,) and t.dtype == np.uint32
    assert ld.TABLE_DWORDS == 16 * 2560 + 4096
    g = t[:ld.G_DWORDS].reshape(16, ld.SLICE_DWORDS)
    plain = g ^ ld.tag(np.arange(ld.G_DWORDS, dtype=np.uint32)).reshape(16, -1)
    assert (plain == plain[0]).all() and len(np.unique(plain[0])) > 2500
    assert not np.array_equal(g[0], g[1])
    assert not np.array_equal(t, ld.source_tables(1))
    assert np.array_equal(t, ld.source_tables(1 << 32))


def test_inputs_differ_from_the_other_probes():
    from kubegpu_amd.probe import atomcheck as at
    from kubegpu_amd.probe import lanecheck as lc

    r0 = np.array([0], dtype=np.uint32)
    mine = {tuple(ld._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    assert len(mine) == 4
    lanes = {tuple(lc._Words(0, s, r0).v(0)[0].tolist()) for s in range(4)}
    atoms = {tuple(at._Words(0, s, r0).w(np.arange(64))[0].tolist()) for s in range(6)}
    assert not mine & lanes and not mine & atoms
    stages = set(range(ld._STAGE0, ld._STAGE0 + 4)) | {ld._STAGE_G, ld._STAGE_X}
    assert len(stages) == 6
    assert not stages & set(range(lc._STAGE0, lc._STAGE0 + 4))
    assert not stages & set(range(at._STAGE0, at._STAGE0 + 6))


# -- coverage of the chosen tables, on the reference alone -----------------------------------

def test_narrow_accesses_reach_every_byte_lane_and_both_signs_in_every_round():
    b8, b16 = ld.subdword_offsets(0, ROUNDS)
    assert b8.shape == b16.shape == (ld.PERIOD, 2, 64)
    slots = dict(ref_period(0, 0))
    lane = np.arange(64)
    for j in range(2):
        for r in range(ld.PERIOD):
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
    W = ld._Words(0, 0, ROUNDS)
    img = W.img()
    slots = dict(ref_period(0, 0))
    b8, b16 = ld.subdword_offsets(0, ROUNDS)
    lane = np.arange(64)
    # after the first b8 store: dword 2l differs from the fill in one byte at most
    first = slots["b8.0.dword"] ^ img[:, 2 * lane]
    mask = np.uint32(0xFF) << (8 * b8[:, 0]).astype(np.uint32)
    assert not (first & ~mask).any() and first.any()
    assert np.array_equal(slots["b8.0.next"], img[:, 2 * lane + 1])  # its neighbour: intact
    assert np.array_equal(slots["b8.1.dword"], slots["b8.0.dword"])  # the second store's
    second = slots["b8.1.next"] ^ img[:, 2 * lane + 1]
    mask = np.uint32(0xFF) << (8 * b8[:, 1]).astype(np.uint32)
    assert not (second & ~mask).any() and second.any()
    first = slots["b16.0.dword"] ^ img[:, 128 + 2 * lane]
    mask = np.uint32(0xFFFF) << (16 * b16[:, 0]).astype(np.uint32)
    assert not (first & ~mask).any() and first.any()
    assert np.array_equal(slots["b16.0.next"], img[:, 129 + 2 * lane])
    # the 96-bit store leaves the fourth dword of its 16 bytes as filled
    assert np.array_equal(slots["b96.b128.3"], img[:, 384 + 4 * W.rot(13) + 3][
        np.arange(ld.PERIOD)[:, None], np.arange(ld.PERIOD)[:, None] * 0 + lane[None, :]]
        if False else np.take_along_axis(img, 384 + 4 * W.rot(13) + 3, axis=1))
    assert np.array_equal(slots["b96.b128.0"], np.take_along_axis(W.v(9), W.rot(13), axis=1))


def test_bank_strides_scatters_and_gathers():
    for need, have in (((1, 2, 3, 4, 8, 16, 32, 33, 64, 65), ld.B32_STRIDES),
                       ((1, 2, 4, 8, 16, 17), ld.WIDE_STRIDES)):
        assert set(need) <= set(have)
    names = ld.slot_table(1)
    for s in ld.B32_STRIDES:
        assert f"b32.s{s}" in names
    for s in ld.WIDE_STRIDES:
        assert f"b64.s{s}.1" in names and f"b128.s{s}.3" in names
    assert {"broadcast", "two", "gather"} <= set(names)
    # every scatter map is a bijection of the 64 rows, and stays inside the region
    for p, (stride, offset) in enumerate(ld.SCATTERS):
        rows = ld.scatter_rows(0, p, ROUNDS)
        assert rows.shape == (ld.PERIOD, 64)
        assert (np.sort(rows, axis=1) == np.arange(64)[None, :]).all()
        assert 0 <= offset and 63 * stride + offset < ld.BANK_DWORDS
    # one scatter's 64 targets share a bank of a dword store (dword address mod 32)
    assert any(stride % 32 == 0 for stride, _ in ld.SCATTERS)
    # what was scattered is what the linear read finds
    slots = dict(ref_period(0, 1))
    W = ld._Words(0, 1, ROUNDS)
    for p, (stride, _) in enumerate(ld.SCATTERS):
        want = np.empty((ld.PERIOD, 64), dtype=np.uint32)
        np.put_along_axis(want, ld.scatter_rows(0, p, ROUNDS), W.v(27 + 2 * p), axis=1)
        if p == 0 or stride != 1:  # a later scatter may overwrite cells of an earlier one
            got = slots[f"scatter{p}.s{stride}"]
            assert got.shape == want.shape
        if p == len(ld.SCATTERS) - 1:
            assert np.array_equal(slots[f"scatter{p}.s{stride}"], want)
    idx = ld.gather_indices(0, ROUNDS)
    assert idx.min() >= 0 and idx.max() < ld.BANK_DWORDS
    assert (np.array([len(np.unique(row)) for row in idx]) < 64).any()  # collisions occur
    # the broadcast row is one value, the two-address row two
    assert (slots["broadcast"] == slots["broadcast"][:, :1]).all()
    assert (slots["two"][:, 0::2] == slots["two"][:, :1]).all()
    assert (slots["two"][:, 1::2] == slots["two"][:, 1:2]).all()


def test_dma_indices_stay_inside_their_tables():
    plan = ld.dma_plan(0, ROUNDS)
    chunks = ld.SLICE_DWORDS // ld.CHUNK_DWORDS
    units = ld.SLICE_DWORDS // ld.UNIT_DWORDS
    for key, top in (("placed_x4", chunks), ("gather_x4_dst", chunks),
                     ("placed_dword", units), ("gather_dword_dst", units)):
        assert plan[key].min() >= 0 and plan[key].max() < top, key
    # whatever the word, by construction
    for m, add in ld.PLACED_X4:
        assert (m - 1 + add + 1) * ld.CHUNK_DWORDS <= ld.SLICE_DWORDS
    for m, add in ld.PLACED_DWORD:
        assert (m - 1 + add + 1) * ld.UNIT_DWORDS <= ld.SLICE_DWORDS
    assert 16 * ld.SLICE_DWORDS == ld.G_DWORDS  # wave 15's part ends where G ends
    src = plan["gather_x4_src"]
    assert src.min() >= 0 and src.max() + 3 < ld.X_DWORDS and not (src & 3).any()
    src = plan["gather_dword_src"]
    assert src.min() >= 0 and src.max() < ld.X_DWORDS
    # the choices move: every chunk is placed in some round, sources collide and spread
    assert set(np.unique(plan["placed_x4"]).tolist()) == set(range(chunks))
    assert len(np.unique(plan["gather_dword_src"])) > 2000
    # the gathers find X at the per-lane index
    _, X = ld._plain_tables(0)
    slots = dict(ref_period(0, 2))
    last = plan["gather_dword_src"][:, 1]
    assert np.array_equal(slots["gather.dword.1"], X[last])
    for c in range(4):
        assert np.array_equal(slots[f"gather.x4.1.{c}"], X[plan["gather_x4_src"][:, 1] + c])


def test_placed_dma_uses_bases_above_64_kib():
    top = 0
    for wave in range(16):
        bases = ld.placed_m0_bases(0, ROUNDS, wave)
        assert bases.shape == (ld.PERIOD, 5) and bases.min() >= 4 * ld.SLICE_DWORDS * wave
        assert bases.max() < 4 * ld.SLICE_DWORDS * (wave + 1)
        top = max(top, int(bases.max()))
    assert top > 65536
    assert ld.placed_m0_bases(0, ROUNDS, 7).min() > 65536  # every copy of waves 7 .. 15
    assert ld.placed_m0_bases(0, ROUNDS, 6).max() > 65536 > ld.placed_m0_bases(0, ROUNDS, 6).min()


def test_xwave_partners_cover_the_other_fifteen_in_five_rounds():
    for wave in range(16):
        for r0 in (0, 1, 59):
            seen = set()
            for r in range(r0, r0 + 5):
                p = ld.xwave_partners(wave, r)
                assert len(set(p)) == 3 and wave not in p
                seen |= set(p)
            assert seen == set(range(16)) - {wave}
    assert ld.xwave_partners(3, ld.PERIOD + 2) == ld.xwave_partners(3, 2)
    # the folded values are the image and its complement, whoever the partner
    slots = ref_period(0, 3)
    assert len(slots) == 2 * 3 * ld.SLICE_DWORDS // 64 == 240
    img = ld._Words(0, 3, ROUNDS).img()
    half = len(slots) // 2
    for j in range(3):
        got = np.stack([v for _, v in slots[j * 40:(j + 1) * 40]], axis=1)  # [r, t*4+c, l]
        got = got.reshape(ld.PERIOD, 10, 4, 64).transpose(0, 1, 3, 2).reshape(ld.PERIOD, -1)
        assert np.array_equal(got, img)
    assert np.array_equal(slots[half][1], ~slots[0][1])


# -- the transposed read ----------------------------------------------------------------------

def test_transposed_read_on_a_hand_written_block():
    # four 4 x 16 blocks of 16-bit elements, one per group of 16 lanes, rows
    # 32 bytes long and stored one after another: element (g, q, c) = g q c
    mem = np.zeros(4 * 4 * 32, dtype=np.uint8)
    elem = lambda g, q, c: (g << 12) | (q << 8) | c  # noqa: E731
    for g in range(4):
        for q in range(4):
            for c in range(16):
                at = 128 * g + 32 * q + 2 * c
                mem[at] = elem(g, q, c) & 0xFF
                mem[at + 1] = elem(g, q, c) >> 8
    # lane 4q + p of a group supplies row q, columns 4p .. 4p + 3
    addr = np.array([128 * (l // 16) + 32 * ((l % 16) // 4) + 8 * (l % 4) for l in range(64)])
    lo, hi = ld.transposed_read(mem, addr)
    assert lo.shape == hi.shape == (64,) and lo.dtype == np.uint32
    for l in range(64):
        g, i = l // 16, l % 16  # lane i receives column i, row q in element q
        assert int(lo[l]) == elem(g, 0, i) | (elem(g, 1, i) << 16)
        assert int(hi[l]) == elem(g, 2, i) | (elem(g, 3, i) << 16)
    # the rows may lie anywhere: swap the addresses of rows 0 and 3 of group 1
    moved = addr.copy()
    moved[16:20], moved[28:32] = addr[28:32], addr[16:20]
    lo2, hi2 = ld.transposed_read(mem, moved)
    assert int(lo2[16 + 5]) == elem(1, 3, 5) | (elem(1, 1, 5) << 16)
    assert int(hi2[16 + 5]) == elem(1, 2, 5) | (elem(1, 0, 5) << 16)
    assert np.array_equal(lo2[:16], lo[:16]) and np.array_equal(hi2[32:], hi[32:])
    with pytest.raises(ValueError, match="8-byte aligned"):
        ld.transposed_read(mem, addr + 4)


def test_transposed_read_addresses_of_the_stage_are_aligned_and_inside():
    W = ld._Words(0, 0, ROUNDS)
    for t in range(2):
        addr = 8 * (W.v(25 + t) % np.uint32(ld.SLICE_BYTES // 8)).astype(np.int64)
        assert addr.min() >= 0 and addr.max() + 8 <= ld.SLICE_BYTES and not (addr & 7).any()


# -- result type and exports ---------------------------------------------------------------------

def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = ld.LdscheckResult(ok=False, rounds=3, waves=48, mismatches=2, first_bad_round=1,
                            bad_stages=["bank"], cus_covered=3, cu_count=256,
                            elapsed_s=0.5, bank_gbps=1.5, waves_on=[0] * 1024)
    assert res.rate_fields() == ["width_gbps", "bank_gbps", "dma_gbps", "xwave_gbps"]
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"width_gbps", "bank_gbps", "dma_gbps", "xwave_gbps", "mismatches",
            "cus_covered"} <= set(d)
    assert d["bank_gbps"] == 1.5 and d["bad_stages"] == ["bank"]
    assert ld.metric_args(d) == (2, 3)
    assert ld.DEFAULT_ROUNDS % ld.PERIOD == 0 and ld.PERIOD <= ld.DEFAULT_ROUNDS <= 65536
    assert len(ld._BYTES_PER_WAVE_ROUND) == 4 and all(x > 0 for x in ld._BYTES_PER_WAVE_ROUND)
    assert ld.STAGES == ("width", "bank", "dma", "xwave")
    assert probe.LdscheckResult is ld.LdscheckResult
    assert probe.ldscheck_round is ld.ldscheck_round
    assert probe.run_ldscheck_subprocess is ld.run_ldscheck_subprocess
    assert probe.source_tables is ld.source_tables
    assert probe.transposed_read is ld.transposed_read


def test_registry():
    assert _active.PROBES == _active.ALL_PROBES + ("ldscheck",)
    assert _active.ALL_PROBES == _active.HEALTH_PROBES + ("lanecheck",)
    assert _active.HEALTH_PROBES == _active.ACTIVE_PROBES + ("atomcheck",)
    assert _active.ACTIVE_PROBES == ("memcheck", "cucheck", "mxcheck", "fpcheck", "hostlink")
    assert ld._child_lock is _active._child_lock


def test_run_ldscheck_subprocess_passes_rounds(monkeypatch):
    calls = []

    def fake(cmd, **kw):
        calls.append((list(cmd), kw, _active._child_lock.locked()))
        return subprocess.CompletedProcess(cmd, 1, 'noise\n{"ok": false, "mismatches": 1}\n', "")

    monkeypatch.setattr(_active.subprocess, "run", fake)
    rec = ld.run_ldscheck_subprocess(3, 128, timeout_s=9.0)
    assert rec == {"ok": False, "mismatches": 1, "exit_code": 1}
    cmd, kw, locked = calls[0]
    assert cmd == [sys.executable, "-m", "kubegpu_amd.probe.ldscheck",
                   "--device", "3", "--rounds", "128"]
    assert locked and kw["timeout"] == 9.0


def test_bad_arguments_raise_before_the_extension_is_loaded(monkeypatch):
    monkeypatch.setattr(ld, "_ext", lambda: pytest.fail("loaded the extension"))
    for kwargs in (dict(rounds=0), dict(rounds=65537), dict(blocks=-1), dict(blocks=4097),
                   dict(seed=-1), dict(seed=1 << 32)):
        with pytest.raises(ValueError, match="ldscheck"):
            ld.ldscheck(**kwargs)


# -- manager verdicts ------------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}
FAIL = dict(PASS, ok=False, mismatches=4, first_bad_round=1, bad_stages=["dma"],
            bad_cus=["3/1/0/7"])


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[2]
    assert mgr.ldscheck_status(uuid) is None

    assert mgr.record_ldscheck(uuid, PASS) is True  # clean
    assert mgr.device_health()[uuid] is True and lines == []

    assert mgr.record_ldscheck(uuid, FAIL) is False  # a mismatch: Unhealthy
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    st = mgr.ldscheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.lanecheck_status(uuid) is None and mgr.cucheck_status(uuid) is None
    assert len(lines) == 1 and "ldscheck" in lines[0] and uuid in lines[0]
    assert "3/1/0/7" in lines[0] and "dma" in lines[0]

    assert mgr.record_ldscheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    # mismatches alone fail the verdict, even where the result calls itself ok
    assert mgr.record_ldscheck(uuid, dict(PASS, mismatches=1)) is False
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_ldscheck(uuid) is True
    assert mgr.clear_ldscheck(uuid) is False
    assert mgr.ldscheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough, and the seven older probes still count
    mgr.record_ldscheck(uuid, PASS)
    mgr.record_lanecheck(uuid, {"ok": False, "mismatches": 1})
    assert mgr.device_health()[uuid] is False
    mgr.clear_lanecheck(uuid)
    assert mgr.device_health()[uuid] is True
    with pytest.raises(KeyError):
        mgr.record_ldscheck("GPU-does-not-exist", FAIL)
    assert set(mgr.ldscheck) == {uuid}


def test_verdict_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_ldscheck(uuid, FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False
    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.ldscheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished and mgr.ldscheck_status(uuid) is None


def test_round_records_verdicts_and_exit_code_2_leaves_health_alone():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    mgr.record_ldscheck(by_index[3], FAIL)  # an earlier verdict must stay
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
    out = ld.ldscheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    health = mgr.device_health()
    assert health[by_index[5]] is False and health[by_index[3]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 4, 6, 7))
    for i in (0, 4):
        assert mgr.ldscheck_status(by_index[i]) is None and out[by_index[i]]["exit_code"] == 2
    assert mgr.ldscheck_status(by_index[3])["mismatches"] == 4
    assert mgr.lanecheck == {} and mgr.cucheck == {}
    assert metrics.gpu_ldscheck[by_index[5]] == {
        "mismatches": 4, "cus_covered": 256,
        "timestamp": metrics.gpu_ldscheck[by_index[5]]["timestamp"]}
    assert set(metrics.gpu_ldscheck) == {by_index[i] for i in (5, 6, 7)}
    assert metrics.gpu_ldscheck_errors == {by_index[i]: 1 for i in (0, 3, 4)}
    assert metrics.gpu_lanecheck == {}


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_ldscheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_ldscheck_error("GPU-a")
        m.inc_ldscheck_error("GPU-a")
        assert m.gpu_ldscheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_ldscheck_errors["GPU-a"] == 2
        assert m.gpu_lanecheck == {} and m.gpu_hostlink_errors == {}
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        from prometheus_client import generate_latest

        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_ldscheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_ldscheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_ldscheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_ldscheck_errors_total", lab) == 2.0
        text = generate_latest(reg).decode()
        assert 'kubegpu_amd_gpu_ldscheck_mismatches{uuid="GPU-a"} 2.0' in text
        assert "# HELP kubegpu_amd_gpu_ldscheck_cus_covered" in text
    assert [row[2] for row in metrics_mod._PROBE_METRICS["ldscheck"]] == [
        "mismatches", "cus_covered", "last_run_timestamp_seconds", "errors_total"]
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_ldscheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--ldscheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--ldscheck needs real GPUs" in cap.err and "LDS" in cap.err
    assert cap.out == ""
    assert amddevs._PROBE_RUNS["ldscheck"][3] == ("mismatches",)


def test_amddevs_ldscheck_exit_codes_with_a_fake_backend(monkeypatch, capsys):
    from kubegpu_amd.cli import amddevs

    results = {}
    seen = []

    def fake_round(mgr, runner, metrics, rounds, max_process_count):
        seen.append((runner, metrics, rounds, max_process_count, len(mgr.gpus)))
        return results

    monkeypatch.setattr(ld, "ldscheck_round", fake_round)
    backend = FakeBackend(fixtures.fixture_8x_mi355x())
    args = amddevs.argparse.Namespace(fake=False, rounds=8, memcheck_idle_only=False)
    results["GPU-a"] = dict(PASS)
    assert amddevs._run_probe("ldscheck", args, backend) == 0
    assert seen[0] == (ld.run_ldscheck_subprocess, None, 8, None, 8)
    assert json.loads(capsys.readouterr().out) == results
    results["GPU-b"] = dict(FAIL)
    assert amddevs._run_probe("ldscheck", args, backend) == 1
    results.clear()
    results["GPU-a"] = {"error": "x", "exit_code": 2}
    assert amddevs._run_probe("ldscheck", args, backend) == 2
    args.rounds = None  # the probe's own default
    amddevs._run_probe("ldscheck", args, backend)
    assert seen[-1][2] == ld.DEFAULT_ROUNDS
    capsys.readouterr()


def test_amddevs_health_shows_the_row(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["ldscheck"] is None for r in rows.values())
    assert all("lanecheck" in r and "atomcheck" in r for r in rows.values())


def test_agent_oneshot_accepts_ldscheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--ldscheck-interval", "600", "--ldscheck-rounds", "64",
                              "--ldscheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_ldscheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert ld.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
