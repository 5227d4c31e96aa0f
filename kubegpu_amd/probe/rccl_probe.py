"""RCCL all-reduce probe wrappers.

Two paths to the same measurement:

* ``run_rccl_probe`` — exec the native single-process ``rcclprobe``
  binary (csrc/rcclprobe.cpp, librccl over xGMI) inside the pod's GPU
  set.  This is the in-pod verification probe named by BASELINE.json.
* ``torch_allreduce_busbw`` — in-process bucketed all-reduce through an
  already-initialized torch.distributed process group (backend "nccl"
  IS RCCL on ROCm); used by bench.py's one-rank-per-GPU mode.

The binary checks its own result: after the timed loop it all-reduces a
rank- and position-dependent pattern once more and compares every
element of every buffer on the GPU, bitwise.  ``reference_send`` and
``reference_sum`` are the numpy definition of that pattern (what the
tests compare the binary's dumps and mismatch records against).
Arithmetic is mod 2**32, ``fmix32`` is memcheck's and cucheck's:

  base(seed, r)  = fmix32(seed ^ (r + 1) * 0x9E3779B9)
  v(seed, r, i)  = fmix32(base(seed, r) ^ i) & 3       r = rank, i = element
  send_r[i]      = bf16(v)          bits 0x0000, 0x3F80, 0x4000, 0x4040
  expected[i]    = bf16(sum over r < n of v(seed, r, i))

Every partial sum is an integer <= 3n, bf16 holds integers up to 256
exactly, so for n <= 64 the sum is exact in whatever order RCCL adds.
"""

from __future__ import annotations

import json
import os
import subprocess
import time
from typing import Dict, List, Optional


def _default_binary() -> str:
    env = os.environ.get("KUBEGPU_RCCLPROBE")
    if env:
        return env
    here = os.path.dirname(os.path.abspath(__file__))
    return os.path.normpath(os.path.join(here, "..", "csrc", "bin", "rcclprobe"))


MAX_RANKS = 64
MAX_ELEMENTS = 1 << 32  # the element index is a u32 (8 GiB of bf16)


def _fmix32(h):
    import numpy as np

    h = h.astype(np.uint32, copy=True)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _check_pattern_args(count: int, seed: int) -> None:
    if not 0 <= count <= MAX_ELEMENTS:
        raise ValueError(f"count {count} outside 0..2**32")
    if not 0 <= seed <= 0xFFFFFFFF:
        raise ValueError(f"seed {seed} is not a u32")


def reference_values(rank: int, count: int, seed: int = 0):
    """v(seed, rank, i) for i < count: uint32 array of values 0..3."""
    import numpy as np

    _check_pattern_args(count, seed)
    if not 0 <= rank < MAX_RANKS:
        raise ValueError(f"rank {rank} outside 0..{MAX_RANKS - 1}")
    mult = ((rank + 1) * 0x9E3779B9) & 0xFFFFFFFF
    base = _fmix32(np.array([seed ^ mult], dtype=np.uint32))[0]
    idx = np.arange(count, dtype=np.uint64).astype(np.uint32)
    return _fmix32(idx ^ base) & np.uint32(3)


def _bf16_bits(values):
    """bf16 bits of integers 0..256: the top half of the f32 encoding
    (exact: such an integer needs at most 8 significant bits)."""
    import numpy as np

    return (values.astype(np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def reference_send(rank: int, count: int, seed: int = 0):
    """bf16 bits (uint16) of rank ``rank``'s send buffer."""
    return _bf16_bits(reference_values(rank, count, seed))


def reference_sum(ndev: int, count: int, seed: int = 0):
    """bf16 bits (uint16) of the all-reduced buffer of ``ndev`` ranks."""
    import numpy as np

    if not 1 <= ndev <= MAX_RANKS:
        raise ValueError(f"ndev {ndev} outside 1..{MAX_RANKS}")
    _check_pattern_args(count, seed)
    total = np.zeros(count, dtype=np.uint32)
    for r in range(ndev):
        total += reference_values(r, count, seed)
    return _bf16_bits(total)


class RcclProbeCheckFailed(subprocess.CalledProcessError):
    """The binary ran and its numerics check failed (exit code 3).

    ``record`` is the parsed JSON line (``mismatches``, ``first_bad``,
    ``records``, ...; None if stdout held none), ``stderr`` the text.
    """

    def __init__(self, returncode, cmd, output=None, stderr=None, record=None):
        super().__init__(returncode, cmd, output=output, stderr=stderr)
        self.record = record

    def __str__(self):
        rec = self.record or {}
        return (
            f"rcclprobe numerics check failed: {rec.get('mismatches')} bad "
            f"elements, first {rec.get('first_bad')} ({super().__str__()})"
        )


def _last_json_line(stdout: bytes) -> Optional[Dict]:
    lines = stdout.decode(errors="replace").strip().splitlines()
    if not lines:
        return None
    try:
        rec = json.loads(lines[-1])
    except ValueError:
        return None
    return rec if isinstance(rec, dict) else None


def run_rccl_probe(
    ndev: Optional[int] = None,
    devices: Optional[List[int]] = None,
    nbytes: int = 256 << 20,
    iters: int = 20,
    warmup: int = 5,
    binary: Optional[str] = None,
    timeout_s: float = 300.0,
    seed: int = 0,
) -> Dict:
    """Run the native probe; returns its JSON record (busbw_gbps etc.).

    Raises RcclProbeCheckFailed (a CalledProcessError carrying the
    parsed record and stderr) when the probe's own check fails, a plain
    CalledProcessError for every other non-zero exit.
    """
    binary = binary or _default_binary()
    if not os.path.exists(binary):
        raise FileNotFoundError(
            f"rcclprobe binary not built at {binary}; run python -m kubegpu_amd.build_native"
        )
    cmd = [binary, "--bytes", str(nbytes), "--iters", str(iters), "--warmup", str(warmup)]
    if seed:
        cmd += ["--seed", str(seed)]
    if devices is not None:
        cmd += ["--devices", ",".join(str(d) for d in devices)]
    elif ndev is not None:
        cmd += ["--ndev", str(ndev)]
    out = subprocess.run(cmd, capture_output=True, timeout=timeout_s)
    if out.returncode == 3:
        raise RcclProbeCheckFailed(
            out.returncode, cmd, output=out.stdout,
            stderr=out.stderr.decode(errors="replace"),
            record=_last_json_line(out.stdout),
        )
    out.check_returncode()
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def torch_allreduce_busbw(
    nbytes: int = 256 << 20,
    iters: int = 20,
    warmup: int = 5,
    device=None,
) -> Dict:
    """Bucketed all-reduce bandwidth through torch.distributed.

    Requires an initialized process group; each rank calls this
    collectively.  Returns {'busbw_gbps', 'algbw_gbps',
    'time_ms_per_iter'} computed from the MAX per-iteration time across
    ranks (the job is as slow as its slowest rank).
    """
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    on_gpu = torch.cuda.is_available()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device()) if on_gpu else torch.device("cpu")
    count = nbytes // 2
    buf = torch.ones(count, dtype=torch.bfloat16, device=device)

    def _sync():
        if on_gpu:
            torch.cuda.synchronize(device)

    for _ in range(warmup):
        dist.all_reduce(buf)
    dist.barrier()
    _sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        dist.all_reduce(buf)
    _sync()
    dist.barrier()
    _sync()  # the barrier itself is a device op under NCCL
    t1 = time.perf_counter()

    elapsed = torch.tensor([t1 - t0], dtype=torch.float64)
    if on_gpu:
        elapsed = elapsed.to(device)
    dist.all_reduce(elapsed, op=dist.ReduceOp.MAX)
    sec = float(elapsed.item()) / iters
    algbw = nbytes / sec / 1e9
    factor = 2.0 * (world - 1) / world if world > 1 else 1.0
    return {
        "busbw_gbps": algbw * factor,
        "algbw_gbps": algbw,
        "time_ms_per_iter": sec * 1e3,
        "world": world,
        "bytes": nbytes,
    }
