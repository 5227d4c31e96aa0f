"""Compute-unit integrity kernel on a real MI355X: the values of every
stage element by element against the exact numpy reference (the tile test
proves the MFMA operand and C/D lane maps, the LDS test that every wave
reads its own dwords at its own offsets), those values tied to the
digests the production kernel compares, every wave's digests against the
numpy reference, clean-run accounting, exact attribution of an injected
fault, a tampered table, argument checks, the child process and CLI."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import cucheck as cc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)
FULL_LDS = 163840


@functools.lru_cache(maxsize=None)
def ref(seed, rounds, lds_bytes):
    """Shared, read-only reference digests."""
    a = cc.reference_digests(seed, rounds, lds_bytes // 64)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ext():
    from kubegpu_amd.probe.bandwidth import load_ext

    return load_ext(required=True)


def expected_on_gpu(seed, rounds, lds_bytes=FULL_LDS):
    return torch.from_numpy(ref(seed, rounds, lds_bytes).view(np.int32).copy()).cuda()


# 0. one wave's values, element by element ------------------------------------------

# the last case is the top of both u32 ranges, where r * 0x7F4A7C15 wraps
CASES = [(0, 0), (0xDEADBEEF, 1), (0xFFFFFFFF, 65535)]


@pytest.mark.parametrize("seed,r", CASES)
@pytest.mark.parametrize("stage", [0, 1])
def test_wave_tile_equals_the_exact_product(stage, seed, r):
    got = cc.wave_values(seed, stage, r)
    want = cc.matmul_tile(seed, stage, r)
    assert got.dtype == np.int64 and got.shape == want.shape == (32, 32)
    bad = got != want
    if bad.any():
        i, j = (int(x) for x in np.argwhere(bad)[0])
        halves_swapped = got.reshape(4, 2, 4, 32)[:, ::-1].reshape(32, 32)
        pytest.fail(
            f"stage {cc.STAGES[stage]}: first wrong element at (row {i}, col {j}): "
            f"got {int(got[i, j])}, want {int(want[i, j])}; "
            f"{int(bad.sum())} of {bad.size} differ, wrong per row "
            f"{bad.sum(axis=1).tolist()}, per col {bad.sum(axis=0).tolist()}; "
            f"transposed tile matches: {bool(np.array_equal(got.T, want))}; "
            f"with the two half-waves' row blocks swapped it matches: "
            f"{bool(np.array_equal(halves_swapped, want))}")


@pytest.mark.parametrize("seed,r", CASES)
def test_wave_valu_trace_equals_the_reference(seed, r):
    got = cc.wave_values(seed, 2, r)
    want = cc.reference_values(seed, 2, r)
    assert got.dtype == np.uint32 and got.shape == want.shape == (32, 64)
    bad = got != want
    if bad.any():
        it, lane = (int(x) for x in np.argwhere(bad)[0])
        if it:
            before = f"{int(got[it - 1, lane]):08x}"
        else:  # the dump begins after iteration 0
            start = cc._words(seed, 2, np.array([r], dtype=np.uint32), lane, 1)
            before = f"the start word, not dumped (reference {int(start[0, 0]):08x})"
        pytest.fail(
            f"first wrong x after iteration {it} in lane {lane}: the GPU's x before "
            f"that iteration was {before}; got {int(got[it, lane]):08x}, want "
            f"{int(want[it, lane]):08x}; {int(bad.sum())} of {bad.size} differ, "
            f"lanes wrong after the last iteration: {np.flatnonzero(bad[-1]).tolist()}")


@pytest.mark.parametrize("lds_bytes,wave", [
    (4096, 0), (4096, 7), (4096, 15), (FULL_LDS, 0),
    (FULL_LDS, 15),  # this slice ends at the last byte of the CU's LDS
])
def test_wave_lds_readback_equals_the_reference(lds_bytes, wave):
    n = lds_bytes // 64
    for seed, r in CASES:
        got = cc.wave_values(seed, 3, r, lds_bytes, wave)
        want = cc.reference_values(seed, 3, r, n)
        assert got.dtype == np.uint32 and got.shape == want.shape == (2, n)
        bad = got != want
        if bad.any():
            p, d = (int(x) for x in np.argwhere(bad)[0])
            pytest.fail(
                f"seed {seed:#x} round {r}, wave {wave} of a {lds_bytes}-byte workgroup: "
                f"first wrong word in pass {p} at dword {d} of the slice: got "
                f"{int(got[p, d]):08x}, want {int(want[p, d]):08x}, xor "
                f"{int(got[p, d] ^ want[p, d]):08x}; wrong per pass "
                f"{bad.sum(axis=1).tolist()} of {n}")


@pytest.mark.parametrize("seed,r", CASES[:2])
def test_dumped_values_fold_to_the_production_digests(seed, r):
    """The dump and the kernel that runs in production are the same stage
    code: folding what one prints gives what every wave of the other
    compares."""
    for lds_bytes in (4096, FULL_LDS):
        prod = cc.wave_digests(seed, r + 1, blocks=1, lds_bytes=lds_bytes)[:, r, :]
        assert prod.shape == (16, 4)
        for stage in range(3):
            folded = cc.fold_values(stage, cc.wave_values(seed, stage, r, lds_bytes))
            assert prod[:, stage].tolist() == [int(folded)] * 16, (stage, lds_bytes)
        waves = range(16) if lds_bytes == 4096 else (0, 15)
        for wave in waves:
            folded = cc.fold_values(3, cc.wave_values(seed, 3, r, lds_bytes, wave))
            assert int(prod[wave, 3]) == int(folded), (wave, lds_bytes)


# 1. every wave against the reference --------------------------------------------

@pytest.mark.parametrize("blocks,lds_bytes,rounds", [
    (1, 4096, 1), (3, 4096, 3), (1, FULL_LDS, 2), (0, FULL_LDS, 2),
])
@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_match_reference(seed, blocks, lds_bytes, rounds):
    got = cc.wave_digests(seed, rounds, blocks, lds_bytes)
    waves = (blocks or cu_count()) * 16
    assert got.dtype == np.uint32 and got.shape == (waves, rounds, 4)
    want = ref(seed, rounds, lds_bytes)
    bad = got != want[None, :, :]
    if bad.any():
        w, r, s = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(
            f"first difference at wave {w}, round {r}, stage {cc.STAGES[s]}: "
            f"got {int(got[w, r, s]):08x}, want {int(want[r, s]):08x}; "
            f"{int(bad.sum())} of {bad.size} digests differ, per stage "
            f"{bad.sum(axis=(0, 1)).tolist()}")


# 2. clean run ---------------------------------------------------------------------

@pytest.mark.parametrize("blocks", [3, 0])
def test_clean_run(blocks):
    res = cc.cucheck(seed=5, rounds=3, blocks=blocks)
    n_blocks = blocks or cu_count()
    assert res.ok and res.mismatches == 0 and res.records == []
    assert res.first_bad_round is None and res.bad_stages == [] and res.bad_cus == []
    assert res.records_dropped == 0
    assert len(res.waves_on) == 1024
    assert sum(res.waves_on) == res.waves == n_blocks * 16
    assert res.cu_count == cu_count()
    print(f"blocks={n_blocks}: cus_covered/cu_count = {res.cus_covered}/{res.cu_count}")
    # a decode that mixed in SIMD or wave-slot bits would exceed cu_count
    assert 1 <= res.cus_covered <= min(res.cu_count, res.waves)
    assert res.rounds == 3 and res.elapsed_s > 0


# 3. exact attribution ---------------------------------------------------------------

def test_injected_fault_is_attributed_to_its_wave():
    mask = 0x00100004
    res = cc.cucheck(seed=0, rounds=3, blocks=3, _inject=(37, 1, 2, mask))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["valu"]
    assert len(res.records) == 1 and res.records_dropped == 0
    rec = res.records[0]
    want = int(ref(0, 3, FULL_LDS)[1, 2])
    assert rec["wave"] == 37 and rec["block"] == 2
    assert rec["round"] == 1 and rec["stage"] == "valu"
    assert rec["expected"] == want and rec["got"] == want ^ mask
    # every field in range, and the CU it names ran at least one wave
    assert 0 <= rec["xcc"] < 8 and 0 <= rec["se"] < 4 and 0 <= rec["sh"] < 2
    assert 0 <= rec["cu"] < 16 and 0 <= rec["simd"] < 4
    assert res.waves_on[cc.cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert res.bad_cus == [f"{rec['xcc']}/{rec['se']}/{rec['sh']}/{rec['cu']}"]
    assert sum(res.waves_on) == 48


# 4. tampered table -------------------------------------------------------------------

@pytest.mark.parametrize("max_records", [16, 0])
def test_tampered_table_is_reported_by_every_wave(max_records):
    table = ref(0, 4, FULL_LDS).copy()
    true = int(table[2, 0])
    table[2, 0] ^= np.uint32(1 << 9)
    res = cc.cucheck(seed=0, rounds=4, blocks=3, max_records=max_records, _expected=table)
    assert not res.ok and res.waves == 48
    assert res.mismatches == res.waves
    assert res.first_bad_round == 2 and res.bad_stages == ["mfma_i8"]
    assert len(res.records) == max_records
    assert res.records_dropped == res.mismatches - max_records
    for rec in res.records:
        assert rec["round"] == 2 and rec["stage"] == "mfma_i8"
        assert rec["got"] == true and rec["expected"] == true ^ (1 << 9)
        assert 0 <= rec["wave"] < 48 and rec["block"] == rec["wave"] // 16
        assert res.waves_on[cc.cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert len({rec["wave"] for rec in res.records}) == max_records


# 5. argument checks --------------------------------------------------------------------

def test_argument_checks():
    e = ext()
    exp2 = expected_on_gpu(0, 2, 4096)
    sentinel = 0x5A5A5A5A
    dump = torch.full((1 * 16 * 2 * 4,), sentinel, dtype=torch.int32, device="cuda")

    def run(expected=exp2, rounds=2, blocks=1, lds_bytes=4096, max_records=4, d=dump):
        return e.cucheck_run(expected, 0, rounds, blocks, lds_bytes, max_records, d, None)

    for rounds in (0, -1, 65537):
        with pytest.raises(RuntimeError, match="rounds"):
            run(rounds=rounds)
    for blocks in (-1, 4097):
        with pytest.raises(RuntimeError, match="blocks"):
            run(blocks=blocks)
    for lds_bytes in (0, 2048, 4100, 6144, FULL_LDS + 4096):
        with pytest.raises(RuntimeError, match="lds_bytes"):
            run(lds_bytes=lds_bytes)
    with pytest.raises(RuntimeError, match="max_records"):
        run(max_records=4097)
    with pytest.raises(RuntimeError, match="on GPU"):
        run(expected=exp2.cpu())
    with pytest.raises(RuntimeError, match="expected must hold"):
        run(expected=expected_on_gpu(0, 3))
    with pytest.raises(RuntimeError, match="int32"):
        run(expected=exp2.to(torch.int64))
    for numel in (16 * 2 * 4 - 1, 16 * 2 * 4 + 1, 2 * 16 * 2 * 4):
        with pytest.raises(RuntimeError, match="dump must hold"):
            run(d=torch.zeros(numel, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="inject"):
        e.cucheck_run(exp2, 0, 2, 1, 4096, 4, None, (16, 0, 0, 1))  # wave past the grid
    # cucheck_values(seed, stage, round, lds_bytes, wave)
    for args in ((0, 4, 0), (0, -1, 0), (0, 0, 65536), (0, 0, -1), (1 << 32, 0, 0),
                 (0, 3, 0, 4096, 16), (0, 3, 0, 4096, -1)):
        with pytest.raises(RuntimeError, match="cucheck"):
            e.cucheck_values(*args)
    for what, args in (("stage", (0, 4, 0)), ("round", (0, 0, 65536)), ("seed", (1 << 32, 0, 0)),
                       ("wave", (0, 3, 0, 4096, 16))):
        with pytest.raises(RuntimeError, match=what):
            e.cucheck_values(*args)
    for lds_bytes in (0, 2048, 6144, FULL_LDS + 4096):
        with pytest.raises(RuntimeError, match="cucheck: lds_bytes"):
            e.cucheck_values(0, 3, 0, lds_bytes, 0)
    with pytest.raises(ValueError):
        cc.wave_values(0, 4, 0)
    with pytest.raises(ValueError):
        cc.cucheck(rounds=0)
    with pytest.raises(ValueError):
        cc.cucheck(rounds=2, lds_bytes=6144)
    with pytest.raises(ValueError):
        cc.cucheck(rounds=2, _expected=ref(0, 3, FULL_LDS))
    torch.cuda.synchronize()
    # none of the refused calls launched anything
    assert bool((dump == sentinel).all())
    # and the accepted one fills the whole dump
    count, first, mask, records, waves_on, elapsed = run()
    torch.cuda.synchronize()
    assert (count, first, mask, records) == (0, -1, 0, [])
    assert len(waves_on) == 1024 and sum(waves_on) == 16 and elapsed > 0
    got = dump.cpu().numpy().view(np.uint32).reshape(16, 2, 4)
    assert np.array_equal(got, np.broadcast_to(ref(0, 2, 4096), (16, 2, 4)))


def test_lds_size_mismatch_shows_only_in_the_lds_stage():
    """The table was made for the full LDS; a 4 KiB run must disagree in
    stage 3 alone, in every wave and round."""
    res = cc.cucheck(seed=0, rounds=2, blocks=1, lds_bytes=4096, max_records=64,
                     _expected=ref(0, 2, FULL_LDS))
    assert res.mismatches == 32 and res.bad_stages == ["lds"] and res.first_bad_round == 0
    small = ref(0, 2, 4096)
    assert sorted((r["wave"], r["round"]) for r in res.records) == [
        (w, r) for w in range(16) for r in range(2)]
    assert all(r["got"] == int(small[r["round"], 3]) for r in res.records)


# 6. child process and CLI ---------------------------------------------------------------

def test_cucheck_child_process():
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.cucheck",
         "--device", "0", "--rounds", "8", "--seed", "3"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["rounds"] == 8 and rec["mismatches"] == 0
    assert rec["device"] == 0 and rec["waves"] == rec["cu_count"] * 16
    assert 1 <= rec["cus_covered"] <= rec["cu_count"]


def test_amddevs_cucheck_cli():
    from kubegpu_amd.discovery import default_backend

    n_gpus = len(default_backend().get_devices().devices)
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--cucheck", "--rounds", "8"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    results = json.loads(res.stdout)
    assert len(results) == n_gpus >= 1
    for rec in results.values():
        assert rec["ok"] is True and rec["mismatches"] == 0 and rec["rounds"] == 8


# 7. one default-size run -----------------------------------------------------------------

def test_default_size_run():
    res = cc.cucheck()
    d = res.to_dict()
    print(json.dumps(d))
    assert res.ok and res.rounds == cc.DEFAULT_ROUNDS
    assert res.elapsed_s > 0 and res.mfma_i8_tops > 0 and res.mfma_bf16_tflops > 0
    assert res.waves == res.cu_count * 16
    assert json.loads(json.dumps(d)) == d
