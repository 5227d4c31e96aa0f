"""Matrix-core format kernel on a real MI355X: the accumulator tile of
every stage element by element against the exact product (which proves
the operand, block-scale and C/D lane maps), every wave's digests against
the numpy reference, clean-run accounting, exact attribution of an
injected fault, a tampered table, argument checks, the child process and
CLI."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import mxcheck as mx
from kubegpu_amd.probe.cucheck import cu_key

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(seed, rounds):
    """Shared, read-only reference digests."""
    a = mx.reference_digests(seed, rounds)
    a.setflags(write=False)
    return a


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ext():
    from kubegpu_amd.probe.bandwidth import load_ext

    return load_ext(required=True)


def expected_on_gpu(seed, rounds):
    return torch.from_numpy(ref(seed, rounds).view(np.int32).copy()).cuda()


# 1. the tile, element by element ---------------------------------------------------

@pytest.mark.parametrize("seed,r", [(0, 0), (0xDEADBEEF, 1)])
@pytest.mark.parametrize("stage", range(4))
def test_wave_tile_equals_the_exact_product(stage, seed, r):
    got = mx.wave_tile(seed, stage, r)
    want = mx.matmul_tile(seed, stage, r)
    n = mx.TILE_DIMS[stage]
    assert got.dtype == np.int64 and got.shape == want.shape == (n, n)
    bad = got != want
    if bad.any():
        i, j = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(
            f"stage {mx.STAGES[stage]}: first wrong element at (row {i}, col {j}): "
            f"got {int(got[i, j])}, want {int(want[i, j])} (units of 1/{mx.UNITS[stage]}); "
            f"{int(bad.sum())} of {bad.size} differ, wrong per row "
            f"{bad.sum(axis=1).tolist()}, per col {bad.sum(axis=0).tolist()}; "
            f"transposed tile matches: {bool(np.array_equal(got.T, want))}")


@pytest.mark.parametrize("seed,r", [(0, 0), (0xDEADBEEF, 1)])
def test_dumped_tiles_fold_to_the_production_digests(seed, r):
    """The tile dump and the kernel that runs in production are the same
    stage code and the same two C/D maps: folding what one stores gives
    what every wave of the other compares."""
    got = mx.wave_digests(seed, rounds=2, blocks=1)
    assert got.shape == (16, 2, 4)
    for stage in range(4):
        folded = int(mx.fold_tile(stage, mx.wave_tile(seed, stage, r)))
        assert got[:, r, stage].tolist() == [folded] * 16, mx.STAGES[stage]


# 2. every wave against the reference --------------------------------------------------

@pytest.mark.parametrize("blocks,rounds", [(1, 1), (3, 3), (0, 2)])
@pytest.mark.parametrize("seed", SEEDS)
def test_wave_digests_match_reference(seed, blocks, rounds):
    got = mx.wave_digests(seed, rounds, blocks)
    waves = (blocks or cu_count()) * 16
    assert got.dtype == np.uint32 and got.shape == (waves, rounds, 4)
    want = ref(seed, rounds)
    bad = got != want[None, :, :]
    if bad.any():
        w, r, s = (int(x) for x in np.argwhere(bad)[0])
        pytest.fail(
            f"first difference at wave {w}, round {r}, stage {mx.STAGES[s]}: "
            f"got {int(got[w, r, s]):08x}, want {int(want[r, s]):08x}; "
            f"{int(bad.sum())} of {bad.size} digests differ, per stage "
            f"{bad.sum(axis=(0, 1)).tolist()}")


# 3. clean run ----------------------------------------------------------------------------

@pytest.mark.parametrize("blocks", [3, 0])
def test_clean_run(blocks):
    res = mx.mxcheck(seed=5, rounds=3, blocks=blocks)
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


# 4. exact attribution ----------------------------------------------------------------------

def test_injected_fault_is_attributed_to_its_wave():
    mask = 0x00100004
    res = mx.mxcheck(seed=0, rounds=3, blocks=3, _inject=(37, 1, 2, mask))
    assert not res.ok and res.mismatches == 1
    assert res.first_bad_round == 1 and res.bad_stages == ["mfma_mxfp4"]
    assert len(res.records) == 1 and res.records_dropped == 0
    rec = res.records[0]
    want = int(ref(0, 3)[1, 2])
    assert rec["wave"] == 37 and rec["block"] == 2
    assert rec["round"] == 1 and rec["stage"] == "mfma_mxfp4"
    assert rec["expected"] == want and rec["got"] == want ^ mask
    # every field in range, and the CU it names ran at least one wave
    assert 0 <= rec["xcc"] < 8 and 0 <= rec["se"] < 4 and 0 <= rec["sh"] < 2
    assert 0 <= rec["cu"] < 16 and 0 <= rec["simd"] < 4
    assert res.waves_on[cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert res.bad_cus == [f"{rec['xcc']}/{rec['se']}/{rec['sh']}/{rec['cu']}"]
    assert sum(res.waves_on) == 48


# 5. tampered table ---------------------------------------------------------------------------

@pytest.mark.parametrize("max_records", [16, 0])
def test_tampered_table_is_reported_by_every_wave(max_records):
    table = ref(0, 4).copy()
    true = int(table[2, 3])
    table[2, 3] ^= np.uint32(1 << 9)
    res = mx.mxcheck(seed=0, rounds=4, blocks=3, max_records=max_records, _expected=table)
    assert not res.ok and res.waves == 48
    assert res.mismatches == res.waves
    assert res.first_bad_round == 2 and res.bad_stages == ["mfma_f64"]
    assert len(res.records) == max_records
    assert res.records_dropped == res.mismatches - max_records
    for rec in res.records:
        assert rec["round"] == 2 and rec["stage"] == "mfma_f64"
        assert rec["got"] == true and rec["expected"] == true ^ (1 << 9)
        assert 0 <= rec["wave"] < 48 and rec["block"] == rec["wave"] // 16
        assert res.waves_on[cu_key(rec["xcc"], rec["se"], rec["sh"], rec["cu"])] > 0
    assert len({rec["wave"] for rec in res.records}) == max_records


# 6. argument checks ------------------------------------------------------------------------------

def test_argument_checks():
    e = ext()
    exp2 = expected_on_gpu(0, 2)
    sentinel = 0x5A5A5A5A
    dump = torch.full((1 * 16 * 2 * 4,), sentinel, dtype=torch.int32, device="cuda")

    def run(expected=exp2, rounds=2, blocks=1, max_records=4, d=dump):
        return e.mxcheck_run(expected, 0, rounds, blocks, max_records, d, None)

    for rounds in (0, -1, 65537):
        with pytest.raises(RuntimeError, match="rounds"):
            run(rounds=rounds)
    for blocks in (-1, 4097):
        with pytest.raises(RuntimeError, match="blocks"):
            run(blocks=blocks)
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
        e.mxcheck_run(exp2, 0, 2, 1, 4, None, (16, 0, 0, 1))  # wave past the grid
    with pytest.raises(RuntimeError, match="seed"):
        e.mxcheck_run(exp2, 1 << 32, 2, 1, 4, None, None)
    for args in ((-1, 0, 0), (1 << 32, 0, 0), (0, 4, 0), (0, -1, 0), (0, 0, -1), (0, 0, 65536)):
        with pytest.raises(RuntimeError, match="mxcheck"):
            e.mxcheck_tile(*args)
    with pytest.raises(ValueError):
        mx.mxcheck(rounds=0)
    with pytest.raises(ValueError):
        mx.mxcheck(rounds=2, _expected=ref(0, 3))
    torch.cuda.synchronize()
    # none of the refused calls launched anything
    assert bool((dump == sentinel).all())
    # and the accepted one fills the whole dump
    count, first, mask, records, waves_on, elapsed = run()
    torch.cuda.synchronize()
    assert (count, first, mask, records) == (0, -1, 0, [])
    assert len(waves_on) == 1024 and sum(waves_on) == 16 and elapsed > 0
    got = dump.cpu().numpy().view(np.uint32).reshape(16, 2, 4)
    assert np.array_equal(got, np.broadcast_to(ref(0, 2), (16, 2, 4)))


# 7. child process and CLI ----------------------------------------------------------------------------

def test_mxcheck_child_process():
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.mxcheck",
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


def test_amddevs_mxcheck_cli():
    from kubegpu_amd.discovery import default_backend

    n_gpus = len(default_backend().get_devices().devices)
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--mxcheck", "--rounds", "8"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    results = json.loads(res.stdout)
    assert len(results) == n_gpus >= 1
    for rec in results.values():
        assert rec["ok"] is True and rec["mismatches"] == 0 and rec["rounds"] == 8


# 8. one default-size run --------------------------------------------------------------------------------

def test_default_size_run():
    res = mx.mxcheck()
    d = res.to_dict()
    print(json.dumps(d))
    assert res.ok and res.rounds == mx.DEFAULT_ROUNDS
    assert res.elapsed_s > 0
    assert min(res.mfma_f16_tflops, res.mfma_fp8_tflops, res.mfma_mxfp4_tflops,
               res.mfma_f64_tflops) > 0
    assert res.waves == res.cu_count * 16
    assert json.loads(json.dumps(d)) == d
