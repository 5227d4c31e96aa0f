"""rcclprobe on a real GPU: the fill, reduce and verify kernels against
the numpy definition in probe/rccl_probe.py, exactly.

Most cases use --loopback (no communicator, N ranks on one device): it is
the only way the rank-r fill and the n-rank expected sum run on a
one-GPU machine.  Both loopback results are needed together: a verify
kernel with a wrong n-rank sum fails on the correct buffer, and a reduce
kernel and a verify kernel that dropped the same rank leave a dump that
disagrees with numpy.

Sweep boundaries come from the grid sizes the binary reports
(F = fill_blocks * block_threads, V = verify_blocks * block_threads).
"""

import json
import os
import subprocess

import numpy as np
import pytest

from kubegpu_amd.probe.rccl_probe import (
    _default_binary,
    reference_send,
    reference_sum,
)

pytestmark = pytest.mark.gpu

TIMEOUT_S = 120


def run_probe(args, dump_dir=None):
    """Run the binary; returns (exit code, record or None, stderr)."""
    cmd = [_default_binary()] + [str(a) for a in args]
    if dump_dir is not None:
        cmd += ["--dump-dir", str(dump_dir)]
    out = subprocess.run(cmd, capture_output=True, timeout=TIMEOUT_S)
    # librccl may print a version banner to stdout before the record, so
    # the record is the last line, as run_rccl_probe reads it
    lines = out.stdout.decode().strip().splitlines()
    rec = json.loads(lines[-1]) if lines and lines[-1].startswith("{") else None
    assert sum(ln.startswith("{") for ln in lines) <= 1, lines
    return out.returncode, rec, out.stderr.decode()


def loopback_args(n, count, seed, corrupt=()):
    args = ["--loopback", n, "--bytes", 2 * count, "--iters", 1, "--warmup", 0,
            "--seed", seed]
    for index, mask in corrupt:
        args += ["--corrupt", f"0:{index}:{mask}"]
    return args


def rccl_args(count, seed, corrupt=()):
    args = ["--ndev", 1, "--bytes", 2 * count, "--iters", 2, "--warmup", 1,
            "--seed", seed]
    for index, mask in corrupt:
        args += ["--corrupt", f"0:{index}:{mask}"]
    return args


def load(dump_dir, name, rank):
    return np.fromfile(os.path.join(str(dump_dir), f"{name}_{rank}.bin"),
                       dtype=np.uint16)


def record_set(rec):
    return {(r["rank"], r["buffer"], r["index"], r["expected"], r["got"])
            for r in rec["records"]}


def expected_records(ref, corrupt):
    return {(0, "recv", i, int(ref[i]), int(ref[i]) ^ m) for i, m in corrupt}


@pytest.fixture(scope="module")
def grid(tmp_path_factory):
    """Grid sizes from a first record (one element, one rank)."""
    d = tmp_path_factory.mktemp("grid")
    rc, rec, err = run_probe(loopback_args(1, 1, 0), d)
    assert rc == 0, err
    b = rec["block_threads"]
    f, v = rec["fill_blocks"] * b, rec["verify_blocks"] * b
    assert b >= 64 and b % 64 == 0 and f >= b and v >= b
    return {"B": b, "F": f, "V": v, "1": 1, "3": 3, "255": 255, "257": 257,
            "F+1": f + 1, "2M+1": 2 * max(f, v) + 1}


# every N of {1, 2, 3, 8, 64}, every count and both seeds appear
CLEAN_CASES = [
    (1, "1", 0xDEADBEEF),
    (2, "3", 0),
    (3, "255", 0xDEADBEEF),
    (8, "257", 0),
    (64, "F+1", 0xDEADBEEF),
    (3, "2M+1", 0),
    (64, "3", 0),
    (2, "2M+1", 0xDEADBEEF),
    (8, "F+1", 0),
]


@pytest.mark.parametrize("n,count_key,seed", CLEAN_CASES)
def test_loopback_clean(grid, tmp_path, n, count_key, seed):
    count = grid[count_key]
    rc, rec, err = run_probe(loopback_args(n, count, seed), tmp_path)
    assert rc == 0, err
    assert rec["mode"] == "loopback" and rec["ndev"] == n
    assert rec["seed"] == seed and rec["bytes"] == 2 * count
    assert rec["check"] == "pass"
    assert rec["mismatches"] == 0
    assert rec["first_bad"] is None and rec["records"] == []
    # one recv and n sends, every element of each
    assert rec["checked_elements"] == count * (n + 1)
    assert np.array_equal(load(tmp_path, "recv", 0), reference_sum(n, count, seed))
    for r in range(n):
        assert np.array_equal(load(tmp_path, "send", r),
                              reference_send(r, count, seed)), f"send_{r}"
    assert sorted(os.listdir(tmp_path)) == sorted(
        ["recv_0.bin"] + [f"send_{r}.bin" for r in range(n)])


def test_loopback_wrong_seed_disagrees(grid, tmp_path):
    """Guards against a comparison that compares nothing."""
    count = grid["257"]
    rc, rec, err = run_probe(loopback_args(3, count, 5), tmp_path)
    assert rc == 0, err
    recv = load(tmp_path, "recv", 0)
    assert recv.shape == (count,)
    assert np.array_equal(recv, reference_sum(3, count, 5))
    assert not np.array_equal(recv, reference_sum(3, count, 6))
    assert not np.array_equal(recv, reference_sum(2, count, 5))
    assert not np.array_equal(load(tmp_path, "send", 1), reference_send(1, count, 6))
    assert not np.array_equal(load(tmp_path, "send", 1), reference_send(2, count, 5))


def test_loopback_exact_detection(grid, tmp_path):
    n, seed = 3, 0xDEADBEEF
    b, v = grid["B"], grid["V"]
    count = 2 * v + 1
    ref = reference_sum(n, count, seed)
    # workgroup edge, sweep edge, both ends; distinct masks, one of two bits
    corrupt = [(0, 0x0001), (b - 1, 0x0002), (b, 0x8004), (v - 1, 0x0008),
               (v, 0x0010), (count - 1, 0x4020)]
    assert len({i for i, _ in corrupt}) == len(corrupt)

    rc, rec, err = run_probe(loopback_args(n, count, seed, corrupt), tmp_path)
    assert rc == 3, err
    assert "NUMERICS CHECK FAILED" in err
    assert rec["check"] == "fail"
    assert rec["mismatches"] == len(corrupt)
    assert rec["checked_elements"] == count * (n + 1)
    assert rec["first_bad"] == {"rank": 0, "buffer": "recv", "index": 0,
                                "expected": int(ref[0]), "got": int(ref[0]) ^ 1}
    assert len(rec["records"]) == len(corrupt)
    assert record_set(rec) == expected_records(ref, corrupt)
    # the dump shows the corrupted buffer, the sends are untouched
    want = ref.copy()
    for i, m in corrupt:
        want[i] ^= m
    assert np.array_equal(load(tmp_path, "recv", 0), want)
    for r in range(n):
        assert np.array_equal(load(tmp_path, "send", r), reference_send(r, count, seed))

    # without index 0 the next lowest is first
    rc, rec, err = run_probe(loopback_args(n, count, seed, corrupt[1:]))
    assert rc == 3, err
    assert rec["mismatches"] == len(corrupt) - 1
    i, m = corrupt[1]
    assert rec["first_bad"] == {"rank": 0, "buffer": "recv", "index": i,
                                "expected": int(ref[i]), "got": int(ref[i]) ^ m}
    assert record_set(rec) == expected_records(ref, corrupt[1:])


def test_loopback_corrupting_twice_restores(grid):
    rc, rec, err = run_probe(
        loopback_args(2, grid["257"], 0, [(256, 0x00F0), (256, 0x00F0)]))
    assert rc == 0, err
    assert rec["check"] == "pass" and rec["mismatches"] == 0


def test_loopback_record_cap(grid):
    n, seed = 3, 0
    v = grid["V"]
    count = 2 * v + 1
    ref = reference_sum(n, count, seed)
    # 20 bad elements over all three sweeps, several in one wave
    idx = list(range(0, 8)) + [63, 64, 65, 777, 1000, v - 2, v - 1, v, v + 1,
                               2 * v - 2, 2 * v - 1, 2 * v]
    assert len(set(idx)) == 20 and max(idx) == count - 1
    corrupt = [(i, 0x0100 + k) for k, i in enumerate(idx)]
    rc, rec, err = run_probe(loopback_args(n, count, seed, corrupt))
    assert rc == 3, err
    assert rec["mismatches"] == 20
    assert rec["first_bad"]["index"] == 0
    got = record_set(rec)
    assert len(rec["records"]) == 16 and len(got) == 16
    assert got <= expected_records(ref, corrupt)


# -- the RCCL path, one device -------------------------------------------------

@pytest.mark.parametrize("count_key,seed", [("1", 0), ("257", 0xDEADBEEF),
                                            ("2M+1", 0)])
def test_rccl_one_device_clean(grid, tmp_path, count_key, seed):
    count = grid[count_key]
    rc, rec, err = run_probe(rccl_args(count, seed), tmp_path)
    assert rc == 0, err
    assert rec["mode"] == "rccl" and rec["ndev"] == 1
    assert rec["iters"] == 2 and rec["warmup"] == 1 and rec["seed"] == seed
    assert rec["check"] == "pass" and rec["mismatches"] == 0
    assert rec["first_bad"] is None and rec["records"] == []
    assert rec["checked_elements"] == 2 * count  # recv and send
    assert rec["dtype"] == "bf16"
    # two decimals: a buffer of a few bytes rounds to 0.00 GB/s
    assert rec["busbw_gbps"] >= 0 and rec["algbw_gbps"] >= 0
    assert (rec["busbw_gbps"] > 0) or count < (1 << 20)
    assert np.array_equal(load(tmp_path, "recv", 0), reference_sum(1, count, seed))
    assert np.array_equal(load(tmp_path, "send", 0), reference_send(0, count, seed))


def test_rccl_one_device_detects_last_element(grid):
    count, seed = grid["2M+1"], 0xDEADBEEF
    ref = reference_sum(1, count, seed)
    corrupt = [(count - 1, 0x0081)]
    rc, rec, err = run_probe(rccl_args(count, seed, corrupt))
    assert rc == 3, err
    assert rec["check"] == "fail" and rec["mismatches"] == 1
    assert rec["busbw_gbps"] > 0  # the record is complete on failure too
    want = {"rank": 0, "buffer": "recv", "index": count - 1,
            "expected": int(ref[-1]), "got": int(ref[-1]) ^ 0x0081}
    assert rec["first_bad"] == want
    assert rec["records"] == [want]


def test_rccl_one_device_no_check(grid):
    rc, rec, err = run_probe(rccl_args(grid["257"], 0) + ["--no-check"])
    assert rc == 0, err
    assert rec["check"] == "skipped"
    for key in ("mismatches", "checked_elements", "first_bad", "records"):
        assert key not in rec
    assert rec["busbw_gbps"] >= 0 and rec["mode"] == "rccl"


@pytest.mark.parametrize("args", [
    ["--devices", "99"],
    ["--devices", "0,99"],
    ["--ndev", "65"],
    ["--loopback", "2", "--devices", "99"],
])
def test_device_arguments_exit_1(args):
    rc, rec, err = run_probe(args + ["--bytes", "512", "--iters", "1"])
    assert rc == 1, err
    assert rec is None
    assert err.startswith("rcclprobe: ") and "available" in err
