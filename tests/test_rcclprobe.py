"""rcclprobe's check pattern and argument handling — everything that
needs no GPU: the numpy definition against a scalar one, the binary's
argument validation (decided before it touches HIP), and the failure
path of run_rccl_probe with a stub binary."""

import json
import os
import stat
import subprocess

import numpy as np
import pytest

from kubegpu_amd.probe import rccl_probe as rp
from kubegpu_amd.probe.rccl_probe import reference_send, reference_sum

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BINARY = os.path.join(REPO, "kubegpu_amd", "csrc", "bin", "rcclprobe")

needs_binary = pytest.mark.skipif(
    not os.path.exists(BINARY), reason="rcclprobe binary not built"
)

# bf16 bits of 0.0, 1.0, 2.0, 3.0
BITS = [0x0000, 0x3F80, 0x4000, 0x4040]


# -- the numpy definition ------------------------------------------------------

def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _scalar_value(seed, r, i):
    """The issue's definition in plain Python integers."""
    base = _fmix(seed ^ (((r + 1) * 0x9E3779B9) & 0xFFFFFFFF))
    return _fmix(base ^ i) & 3


def _scalar_bf16(v):
    """bf16 bits of a small non-negative integer, from its binary digits."""
    if v == 0:
        return 0
    e = v.bit_length() - 1
    frac = v - (1 << e)  # below 2**e
    assert e <= 7 or frac == 0, "needs more than 8 significant bits"
    mant = (frac << 7) >> e if e <= 7 else 0
    assert (mant << e) >> 7 == frac
    return ((127 + e) << 7) | mant


def test_fmix_pin():
    # murmur3's finaliser: fmix32(1) is a published value
    assert _fmix(1) == 0x514E28B7
    assert int(rp._fmix32(np.array([1], dtype=np.uint32))[0]) == 0x514E28B7


def test_known_bit_patterns():
    assert [_scalar_bf16(v) for v in range(4)] == BITS
    got = rp._bf16_bits(np.arange(4, dtype=np.uint32))
    assert got.dtype == np.uint16 and got.tolist() == BITS
    for seed in (0, 7, 0xDEADBEEF):
        s = reference_send(3, 4096, seed)
        assert s.dtype == np.uint16 and s.shape == (4096,)
        # all four values occur, and nothing else
        assert sorted(set(s.tolist())) == BITS


def test_small_integers_round_trip_through_bf16():
    v = np.arange(257, dtype=np.uint32)
    bits = rp._bf16_bits(v)
    back = (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert np.array_equal(back, v.astype(np.float32))
    assert bits.tolist() == [_scalar_bf16(int(x)) for x in v]


@pytest.mark.parametrize("seed", [0, 7, 0xDEADBEEF, 0xFFFFFFFF])
def test_send_matches_scalar_definition(seed):
    for rank in (0, 1, 5, 63):
        got = reference_send(rank, 300, seed)
        want = [BITS[_scalar_value(seed, rank, i)] for i in range(300)]
        assert got.tolist() == want


def test_ranks_seeds_and_positions_differ():
    a = reference_send(0, 4096, 0)
    assert not np.array_equal(a, reference_send(1, 4096, 0))
    assert not np.array_equal(a, reference_send(0, 4096, 1))
    # no short period: a shifted copy disagrees
    assert not np.array_equal(a[:-256], a[256:])
    # a prefix of a longer buffer is the shorter buffer
    assert np.array_equal(a[:257], reference_send(0, 257, 0))


def test_one_rank_sum_is_its_send():
    for seed in (0, 0xDEADBEEF):
        assert np.array_equal(reference_sum(1, 1000, seed),
                              reference_send(0, 1000, seed))


@pytest.mark.parametrize("ndev", [2, 3, 8, 64])
def test_sum_is_integer_sum_of_ranks(ndev):
    seed, count = 0xDEADBEEF, 513
    total = [sum(_scalar_value(seed, r, i) for r in range(ndev))
             for i in range(count)]
    assert reference_sum(ndev, count, seed).tolist() == [_scalar_bf16(t) for t in total]


def test_sum_stays_exact_for_64_ranks():
    s = reference_sum(64, 1 << 20, 7)
    vals = (s.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert vals.max() <= 192  # 3 * 64, below bf16's last exact integer 256
    assert np.array_equal(vals, np.floor(vals))
    assert vals.max() == 138  # the issue's figure for seed 7


def test_index_is_u32_at_the_top():
    # element 2**32 - 1 is the last one the binary accepts (8 GiB)
    i = (1 << 32) - 1
    assert _scalar_value(5, 2, i) in range(4)
    with pytest.raises(ValueError):
        reference_send(0, (1 << 32) + 1, 0)


def test_reference_argument_errors():
    with pytest.raises(ValueError):
        reference_sum(0, 4, 0)
    with pytest.raises(ValueError):
        reference_sum(65, 4, 0)
    with pytest.raises(ValueError):
        reference_send(64, 4, 0)
    with pytest.raises(ValueError):
        reference_send(0, 4, 1 << 32)
    with pytest.raises(ValueError):
        reference_send(0, 4, -1)
    assert reference_send(0, 0, 0).shape == (0,)


# -- argument validation in the binary -----------------------------------------

BAD_ARGS = [
    ["--bytes", "0"],
    ["--bytes", "-2"],
    ["--bytes", "3"],                       # odd
    ["--bytes", str((8 << 30) + 2)],        # above 8 GiB
    ["--bytes", "x"],
    ["--bytes", "1.5"],
    ["--bytes", "64k"],
    ["--bytes", ""],
    ["--bytes", "99999999999999999999"],    # overflows a long long
    ["--bytes"],                            # no value
    ["--iters", "0"],
    ["--iters", "-1"],
    ["--iters", "x"],
    ["--iters"],
    ["--warmup", "-1"],
    ["--warmup", "x"],
    ["--warmup"],
    ["--ndev", "0"],
    ["--ndev", "-1"],
    ["--ndev", "x"],
    ["--ndev"],
    ["--devices", "0,0"],
    ["--devices", "-1"],
    ["--devices", "0,-1"],
    ["--devices", "x"],
    ["--devices", "0,,1"],
    ["--devices", "0,"],
    ["--devices", ""],
    ["--devices"],
    ["--seed", "-1"],
    ["--seed", str(1 << 32)],
    ["--seed", "x"],
    ["--seed"],
    ["--loopback", "0"],
    ["--loopback", "65"],
    ["--loopback", "x"],
    ["--loopback"],
    ["--loopback", "2", "--ndev", "2"],
    ["--corrupt", "0:0"],
    ["--corrupt", "0:0:0"],                 # empty mask
    ["--corrupt", "0:0:0x10000"],           # mask wider than 16 bits
    ["--corrupt", "0:x:1"],
    ["--corrupt", "-1:0:1"],
    ["--corrupt", "64:0:1"],
    ["--bytes", "10", "--corrupt", "0:5:1"],        # index == count
    ["--loopback", "2", "--corrupt", "1:0:1"],      # loopback has one recv
    ["--ndev", "1", "--corrupt", "1:0:1"],
    ["--corrupt"],
    ["--no-check", "--corrupt", "0:0:1"],
    ["--no-check", "--dump-dir", "d"],
    ["--dump-dir", "d", "--bytes", str((64 << 20) + 2)],
    ["--dump-dir"],
    ["--frobnicate"],
]


@needs_binary
@pytest.mark.parametrize("args", BAD_ARGS, ids=lambda a: " ".join(a) or "-")
def test_bad_arguments_exit_2_before_hip(args, tmp_path):
    out = subprocess.run([BINARY] + args, capture_output=True, timeout=60,
                         cwd=tmp_path)
    assert out.returncode == 2, (out.returncode, out.stderr)
    assert out.stdout == b""
    lines = out.stderr.decode().strip().splitlines()
    if args == ["--frobnicate"]:
        assert lines[0].startswith("usage: rcclprobe")
        assert "test hooks" in out.stderr.decode()
    else:
        assert len(lines) == 1 and lines[0].startswith("rcclprobe: ")
    assert not os.listdir(tmp_path)  # no dump directory was created


# -- run_rccl_probe ------------------------------------------------------------

FAIL_RECORD = {
    "ndev": 2, "bytes": 514, "iters": 2, "warmup": 1, "time_ms_per_iter": 0.1,
    "algbw_gbps": 1.0, "busbw_gbps": 1.0, "dtype": "bf16", "check": "fail",
    "mode": "rccl", "seed": 5, "checked_elements": 1028, "mismatches": 1,
    "first_bad": {"rank": 1, "buffer": "recv", "index": 256,
                  "expected": 0x4000, "got": 0x4001},
    "records": [{"rank": 1, "buffer": "recv", "index": 256,
                 "expected": 0x4000, "got": 0x4001}],
    "fill_blocks": 1024, "verify_blocks": 2048, "block_threads": 256,
}


def _stub(tmp_path, body):
    stub = tmp_path / "rcclprobe"
    stub.write_text("#!/bin/sh\n" + body)
    stub.chmod(stub.stat().st_mode | stat.S_IEXEC)
    return str(stub)


def test_run_rccl_probe_surfaces_the_fail_record(tmp_path):
    stub = _stub(
        tmp_path,
        "echo \"$@\" > " + str(tmp_path / "argv") + "\n"
        "echo 'rcclprobe: NUMERICS CHECK FAILED (1 bad elements)' >&2\n"
        "echo '" + json.dumps(FAIL_RECORD) + "'\n"
        "exit 3\n",
    )
    with pytest.raises(rp.RcclProbeCheckFailed) as ei:
        rp.run_rccl_probe(ndev=2, nbytes=514, iters=2, warmup=1, seed=5,
                          binary=stub)
    e = ei.value
    assert isinstance(e, subprocess.CalledProcessError)
    assert e.returncode == 3
    assert e.record == FAIL_RECORD
    assert "NUMERICS CHECK FAILED" in e.stderr
    assert "256" in str(e)  # the message names the first bad element
    argv = (tmp_path / "argv").read_text().split()
    assert argv[argv.index("--seed") + 1] == "5"
    assert argv[argv.index("--bytes") + 1] == "514"
    # callers that catch Exception / CalledProcessError keep working
    try:
        rp.run_rccl_probe(ndev=2, binary=stub)
    except subprocess.CalledProcessError as again:
        assert again.record["first_bad"]["index"] == 256


def test_run_rccl_probe_exit_3_without_a_record(tmp_path):
    stub = _stub(tmp_path, "echo garbage\nexit 3\n")
    with pytest.raises(rp.RcclProbeCheckFailed) as ei:
        rp.run_rccl_probe(ndev=1, binary=stub)
    assert ei.value.record is None


def test_run_rccl_probe_other_failures_stay_plain(tmp_path):
    stub = _stub(tmp_path, "echo 'rcclprobe: HIP error' >&2\nexit 1\n")
    with pytest.raises(subprocess.CalledProcessError) as ei:
        rp.run_rccl_probe(ndev=1, binary=stub)
    assert not isinstance(ei.value, rp.RcclProbeCheckFailed)
    assert ei.value.returncode == 1


def test_run_rccl_probe_pass_record_and_default_seed(tmp_path):
    rec = dict(FAIL_RECORD, check="pass", mismatches=0, first_bad=None,
               records=[], seed=0)
    stub = _stub(
        tmp_path,
        "echo \"$@\" > " + str(tmp_path / "argv") + "\n"
        "echo '" + json.dumps(rec) + "'\n",
    )
    assert rp.run_rccl_probe(devices=[0, 1], binary=stub) == rec
    argv = (tmp_path / "argv").read_text().split()
    assert "--seed" not in argv and argv[argv.index("--devices") + 1] == "0,1"
