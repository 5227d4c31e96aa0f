"""Active compute-unit integrity probe — wrapper over the cucheck HIP kernel.

``memcheck`` asks whether HBM returns what was written; this asks
whether the part of the GPU that computes returns right answers.  A
matrix core that drops a partial product, a vector ALU with a stuck bit
or an LDS bank that flips one moves no ECC counter and passes memcheck.
``cucheck()`` launches one 16-wave workgroup per compute unit; every
wave runs the same deterministic workload and compares four 32-bit
digests per round with ``reference_digests``, computed here in numpy.
A wave that disagrees logs where the hardware says it ran (XCD, shader
engine, shader array, CU, SIMD), so a wrong answer points at a
physical CU.

The workload (csrc/cucheck.hip; ``reference_digests`` is the
definition).  Arithmetic is mod 2**32, ``fmix32`` / ``rotl32`` are
memcheck's:

  base(seed, stage, r)      = fmix32(seed ^ (stage+1)*0x9E3779B9 ^ r*0x7F4A7C15)
  word(seed, stage, r, idx) = fmix32(base(seed, stage, r) + idx)
  i8(w, b)                  = byte b of w (little endian), signed
  salt(n)                   = (n+1) * 0x9E3779B9

  0 mfma_i8    A[i][k] = i8(word(0, r, 64i + k/4), k%4), 32 x 256
               B[k][j] = i8(word(0, r, 2048 + 64j + k/4), k%4), 256 x 32
               C = A.B in int32; digest = sum fmix32(u32(C[i][j]) + salt(32i + j))
  1 mfma_bf16  the same with K = 128, 32 words per row (A 32i + k/4,
               B 1024 + 32j + k/4), values converted to bf16, f32 accumulate
  2 valu       per lane l: x = word(2, r, l); 32 times
                   x = x*0x9E3779B1 + rotl32(x, 13)
                   x ^= mulhi_u32(x, 0x85EBCA6B)
                   x += u32(fmaf(f32(x & 0xFFF), f32((x>>12) & 0xFFF), f32(x>>24)))
               digest = sum over 64 lanes of fmix32(x_l + l)
  3 lds        v[d] = word(3, r, d) written to dword d of the wave's LDS
               slice (lds_bytes/64 dwords), read back by another lane,
               then ~v[d] the same way;
               digest = sum fmix32(v[d] + salt(d)) + sum fmix32(~v[d] + salt(d))

Floating-point stages use only data for which every intermediate is an
exactly representable integer (bytes in bf16, sums below 2**24 in f32),
so the reference is integer arithmetic — and rounding logic is therefore
not covered: it is ``probe/fpcheck.py``'s ground.  The f16, fp8, MXFP4
and f64 matrix paths are
``probe/mxcheck.py``'s ground; transcendental units are not covered,
nor is the path to HBM (memcheck's ground).

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.cucheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

from .memcheck import (
    EXIT_CANNOT_RUN,
    EXIT_MISMATCH,
    EXIT_PASS,
    _REPO_ROOT,
    _child_lock,
    idle_gpus,
)

STAGES: Tuple[str, ...] = ("mfma_i8", "mfma_bf16", "valu", "lds")
WAVES_PER_BLOCK = 16
DEFAULT_LDS_BYTES = 163840
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/cucheck_mi355x.json): 22.6 us per round
# with the default grid (256 workgroups, 4096 waves, 160 KiB LDS each),
# flat from 1024 to 22528 rounds, so 22 x 1024 rounds take 0.51 s.  The
# whole-run lower bounds at that size are 95 TOPS int8 and 48 TFLOPS
# bf16: operand generation and the VALU / LDS stages set the time, not
# the matrix cores.  The numpy table for it cost 0.7 s of host time.
DEFAULT_ROUNDS = 22528

# integer ops / flops one wave spends in the matrix cores per round
_I8_OPS_PER_WAVE_ROUND = 2 * 32 * 32 * 256
_BF16_FLOPS_PER_WAVE_ROUND = 2 * 32 * 32 * 128
_REF_CHUNK = 128  # rounds per numpy batch


# -- numpy definition ----------------------------------------------------------

def _fmix32(h):
    import numpy as np

    h = h.astype(np.uint32, copy=True)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _base(seed: int, stage: int, r):
    import numpy as np

    c = np.uint32(((stage + 1) * 0x9E3779B9) & 0xFFFFFFFF)
    return _fmix32(np.uint32(seed) ^ c ^ (r * np.uint32(0x7F4A7C15)))


def _words(seed: int, stage: int, r, first: int, count: int):
    """word(seed, stage, r, first .. first+count-1) as uint32[len(r), count]."""
    import numpy as np

    idx = np.arange(first, first + count, dtype=np.uint32)
    return _fmix32(_base(seed, stage, r)[:, None] + idx[None, :])


def _salt(n):
    import numpy as np

    return (n.astype(np.uint32) + np.uint32(1)) * np.uint32(0x9E3779B9)


def _signed_bytes(words):
    """uint32[..., n] -> int8[..., 4n], little-endian byte order."""
    import numpy as np

    return np.ascontiguousarray(words).astype("<u4").view(np.int8)


def matmul_tile(seed: int, stage: int, r: int):
    """The 32x32 int64 product C = A.B of a matrix stage (0 or 1) for
    one round — what the digest is folded from."""
    import numpy as np

    if stage not in (0, 1):
        raise ValueError(f"stage {stage} is not a matrix stage")
    wpr = 64 if stage == 0 else 32  # words per row
    rr = np.array([r], dtype=np.uint32)
    a = _signed_bytes(_words(seed, stage, rr, 0, 32 * wpr)).reshape(32, 4 * wpr)
    bt = _signed_bytes(_words(seed, stage, rr, 32 * wpr, 32 * wpr)).reshape(32, 4 * wpr)
    return a.astype(np.int64) @ bt.astype(np.int64).T


def _matmul_digests(seed: int, stage: int, r):
    import numpy as np

    wpr = 64 if stage == 0 else 32
    n = len(r)
    a = _signed_bytes(_words(seed, stage, r, 0, 32 * wpr)).reshape(n, 32, 4 * wpr)
    bt = _signed_bytes(_words(seed, stage, r, 32 * wpr, 32 * wpr)).reshape(n, 32, 4 * wpr)
    # |C| <= 2**22: float64 products and sums are exact, and BLAS is fast
    c = np.matmul(a.astype(np.float64), bt.astype(np.float64).transpose(0, 2, 1))
    cu = (c.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).reshape(n, 1024)
    salt = _salt(np.arange(1024, dtype=np.uint32))  # 32*i + j, row-major
    return _fmix32(cu + salt[None, :]).sum(axis=1, dtype=np.uint32)


def _valu_digests(seed: int, r):
    import numpy as np

    x = _words(seed, 2, r, 0, 64)
    for _ in range(32):
        x = x * np.uint32(0x9E3779B1) + ((x << np.uint32(13)) | (x >> np.uint32(19)))
        x ^= ((x.astype(np.uint64) * np.uint64(0x85EBCA6B)) >> np.uint64(32)).astype(np.uint32)
        # a*b + c < 2**24: the f32 FMA is exact, so integers define it
        x += (x & np.uint32(0xFFF)) * ((x >> np.uint32(12)) & np.uint32(0xFFF)) \
            + (x >> np.uint32(24))
    lanes = np.arange(64, dtype=np.uint32)
    return _fmix32(x + lanes[None, :]).sum(axis=1, dtype=np.uint32)


def _lds_digests(seed: int, r, lds_dwords: int):
    import numpy as np

    v = _words(seed, 3, r, 0, lds_dwords)
    salt = _salt(np.arange(lds_dwords, dtype=np.uint32))[None, :]
    return (_fmix32(v + salt).sum(axis=1, dtype=np.uint32)
            + _fmix32(~v + salt).sum(axis=1, dtype=np.uint32))


def reference_digests(seed: int, rounds: int, lds_dwords: int = 2560):
    """Expected digests as uint32[rounds, 4], columns in STAGES order.

    Pure numpy: needs neither torch nor a GPU.  ``lds_dwords`` is the
    per-wave LDS slice, lds_bytes / 64.  This is the definition the GPU
    kernel is tested against."""
    import numpy as np

    seed = int(seed) & 0xFFFFFFFF
    rounds = int(rounds)
    lds_dwords = int(lds_dwords)
    if rounds < 0 or lds_dwords <= 0:
        raise ValueError("reference_digests: rounds >= 0 and lds_dwords > 0 required")
    out = np.empty((rounds, len(STAGES)), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rounds, _REF_CHUNK):
            r = np.arange(lo, min(lo + _REF_CHUNK, rounds), dtype=np.uint32)
            out[lo:lo + len(r), 0] = _matmul_digests(seed, 0, r)
            out[lo:lo + len(r), 1] = _matmul_digests(seed, 1, r)
            out[lo:lo + len(r), 2] = _valu_digests(seed, r)
            out[lo:lo + len(r), 3] = _lds_digests(seed, r, lds_dwords)
    return out


# -- GPU run ---------------------------------------------------------------------

@dataclass
class CucheckResult:
    ok: bool = True
    rounds: int = 0
    waves: int = 0
    mismatches: int = 0
    first_bad_round: Optional[int] = None
    bad_stages: List[str] = field(default_factory=list)
    # {"wave", "block", "xcc", "se", "sh", "cu", "simd", "round", "stage",
    #  "expected", "got"} per logged digest
    records: List[Dict] = field(default_factory=list)
    records_dropped: int = 0
    cus_covered: int = 0  # distinct CUs that ran at least one wave
    cu_count: int = 0  # multiProcessorCount
    bad_cus: List[str] = field(default_factory=list)  # "xcc/se/sh/cu"
    elapsed_s: float = 0.0
    # Whole-run lower bounds (the kernel's time also holds operand
    # generation, the VALU and LDS stages and the digests): informative.
    mfma_i8_tops: float = 0.0
    mfma_bf16_tflops: float = 0.0
    waves_on: List[int] = field(default_factory=list, repr=False)

    def to_dict(self) -> dict:
        return {
            "ok": bool(self.ok),
            "rounds": int(self.rounds),
            "waves": int(self.waves),
            "mismatches": int(self.mismatches),
            "first_bad_round": self.first_bad_round,
            "bad_stages": list(self.bad_stages),
            "records": [dict(r) for r in self.records],
            "records_dropped": int(self.records_dropped),
            "cus_covered": int(self.cus_covered),
            "cu_count": int(self.cu_count),
            "bad_cus": list(self.bad_cus),
            "elapsed_s": float(self.elapsed_s),
            "mfma_i8_tops": float(self.mfma_i8_tops),
            "mfma_bf16_tflops": float(self.mfma_bf16_tflops),
        }


def _ext():
    from .bandwidth import load_ext

    return load_ext(required=True)


def cu_key(xcc: int, se: int, sh: int, cu: int) -> int:
    """Index of a CU in the kernel's waves_on table."""
    return (xcc << 7) | (se << 5) | (sh << 4) | cu


def _decode_record(raw) -> dict:
    wave, hw, rnd, stage, expected, got = (int(x) for x in raw)
    # hw = XCC_ID << 16 | HW_ID[15:0]; HW_ID: SIMD 5:4, CU 11:8, SH 12, SE 14:13
    return {
        "wave": wave,
        "block": wave // WAVES_PER_BLOCK,
        "xcc": (hw >> 16) & 0xF,
        "se": (hw >> 13) & 0x3,
        "sh": (hw >> 12) & 0x1,
        "cu": (hw >> 8) & 0xF,
        "simd": (hw >> 4) & 0x3,
        "round": rnd,
        "stage": STAGES[stage] if 0 <= stage < len(STAGES) else stage,
        "expected": expected,
        "got": got,
    }


def _device(device):
    import torch

    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def _expected_tensor(table, rounds: int, device):
    import numpy as np
    import torch

    table = np.array(table, dtype=np.uint32)  # own, writable copy for torch
    if table.shape != (rounds, len(STAGES)):
        raise ValueError(
            f"cucheck: expected table must be [{rounds}, {len(STAGES)}], got {table.shape}")
    return torch.from_numpy(table.view(np.int32)).to(device)


def cucheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    lds_bytes: int = DEFAULT_LDS_BYTES,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> CucheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    With the default ``lds_bytes`` a workgroup takes a CU's whole LDS,
    so on an idle GPU the default grid lands one workgroup on every CU;
    ``cus_covered`` reports how many distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot corrupt a
    CU."""
    import torch

    rounds, blocks, lds_bytes = int(rounds), int(blocks), int(lds_bytes)
    seed = int(seed)
    ext = _ext()
    device = _device(device)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"cucheck: rounds must be in 1..65536, got {rounds}")
    if lds_bytes < 4096 or lds_bytes > DEFAULT_LDS_BYTES or lds_bytes % 4096:
        raise ValueError(
            f"cucheck: lds_bytes must be a multiple of 4096 in 4096..163840, got {lds_bytes}")
    table = _expected if _expected is not None else reference_digests(
        seed, rounds, lds_bytes // 64)
    expected = _expected_tensor(table, rounds, device)
    inject = None if _inject is None else tuple(int(x) for x in _inject)
    count, first, mask, records, waves_on, elapsed = ext.cucheck_run(
        expected, seed, rounds, blocks, lds_bytes, int(max_records), None, inject)

    res = CucheckResult(rounds=rounds)
    res.waves_on = [int(x) for x in waves_on]
    res.waves = sum(res.waves_on)
    res.mismatches = int(count)
    res.ok = res.mismatches == 0
    res.first_bad_round = int(first) if res.mismatches else None
    res.bad_stages = [s for i, s in enumerate(STAGES) if (int(mask) >> i) & 1]
    res.records = [_decode_record(r) for r in records]
    res.records_dropped = res.mismatches - len(res.records)
    res.cus_covered = sum(1 for x in res.waves_on if x)
    res.cu_count = int(torch.cuda.get_device_properties(device).multi_processor_count)
    res.bad_cus = sorted({f"{r['xcc']}/{r['se']}/{r['sh']}/{r['cu']}" for r in res.records})
    res.elapsed_s = float(elapsed)
    if res.elapsed_s > 0:
        work = res.waves * rounds / res.elapsed_s / 1e12
        res.mfma_i8_tops = work * _I8_OPS_PER_WAVE_ROUND
        res.mfma_bf16_tflops = work * _BF16_FLOPS_PER_WAVE_ROUND
    return res


def wave_digests(seed: int, rounds: int, blocks: int = 0,
                 lds_bytes: int = DEFAULT_LDS_BYTES, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``cucheck`` with its dump pointer set."""
    import numpy as np
    import torch

    rounds, blocks, lds_bytes = int(rounds), int(blocks), int(lds_bytes)
    device = _device(device)
    if blocks == 0:
        blocks = int(torch.cuda.get_device_properties(device).multi_processor_count)
    waves = blocks * WAVES_PER_BLOCK
    expected = _expected_tensor(
        reference_digests(seed, rounds, lds_bytes // 64), rounds, device)
    dump = torch.zeros(waves * rounds * len(STAGES), dtype=torch.int32, device=device)
    _ext().cucheck_run(expected, int(seed), rounds, blocks, lds_bytes, 0, dump, None)
    return dump.cpu().numpy().view(np.uint32).reshape(waves, rounds, len(STAGES))


# -- child process -----------------------------------------------------------

def run_cucheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                           timeout_s: float = 120.0) -> dict:
    """Run the cucheck CLI for GPU ``index`` in a fresh child process
    (never exec: the parent may hold the GPU open) and return its JSON
    record with ``exit_code`` added.  Serialised on memcheck's child
    lock, so the two probes never overlap on a GPU.  Raises
    subprocess.TimeoutExpired when the child overruns (it is killed
    first)."""
    cmd = [sys.executable, "-m", "kubegpu_amd.probe.cucheck",
           "--device", str(int(index)), "--rounds", str(int(rounds))]
    env = dict(os.environ)
    env["PYTHONPATH"] = _REPO_ROOT + os.pathsep + env["PYTHONPATH"] \
        if env.get("PYTHONPATH") else _REPO_ROOT
    with _child_lock:
        out = subprocess.run(cmd, capture_output=True, timeout=timeout_s,
                             env=env, text=True)
    lines = out.stdout.strip().splitlines()
    try:
        rec = json.loads(lines[-1])
    except (IndexError, ValueError):
        rec = {"error": f"no JSON from cucheck child: {out.stderr[-500:]}"}
        out.returncode = EXIT_CANNOT_RUN
    rec["exit_code"] = out.returncode
    return rec


def cucheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                  rounds: int = DEFAULT_ROUNDS,
                  max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """Check every idle GPU once and record the verdicts.

    Same selection as ``memcheck_round`` (no allocation, process_count
    at most ``max_process_count``, None ignores it), in index order;
    ``runner(index, rounds)`` is called and its result dict recorded on
    the manager.  A runner that raises, times out or reports exit code
    2 says nothing about the hardware: it is logged and counted as an
    error, and the GPU's health is left as it was.  Returns
    {uuid: result}."""
    from ..api import utils

    out: Dict[str, dict] = {}
    for index, uuid in idle_gpus(manager, max_process_count):
        try:
            rec = runner(index, rounds)
            if not isinstance(rec, dict):
                raise TypeError(f"cucheck runner returned {type(rec).__name__}")
            if rec.get("exit_code") == EXIT_CANNOT_RUN or "mismatches" not in rec:
                raise RuntimeError(rec.get("error") or "cucheck could not run")
        except Exception as e:  # not a compute fault: health unchanged
            utils.errorf("cucheck on GPU %s (index %d) did not run: %s", uuid, index, e)
            if metrics is not None:
                metrics.inc_cucheck_error(uuid)
            out[uuid] = {"error": str(e), "exit_code": EXIT_CANNOT_RUN}
            continue
        try:
            manager.record_cucheck(uuid, rec)
        except KeyError:  # vanished mid-round
            continue
        if metrics is not None:
            metrics.set_gpu_cucheck(
                uuid, int(rec["mismatches"]), int(rec.get("cus_covered", 0)),
                time.time(),
            )
        out[uuid] = rec
    return out


def main(argv=None) -> int:
    import argparse

    ap = argparse.ArgumentParser(prog="kubegpu-amd-cucheck")
    ap.add_argument("--device", type=int, required=True, metavar="INDEX")
    ap.add_argument("--rounds", type=int, default=DEFAULT_ROUNDS, metavar="N")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)

    # pin before torch / HIP initialise (same as memcheck)
    os.environ["ROCR_VISIBLE_DEVICES"] = str(args.device)
    rec: dict
    try:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible")
        torch.cuda.set_device(0)
        result = cucheck(seed=args.seed, rounds=args.rounds)
        rec = result.to_dict()
        code = EXIT_PASS if result.ok else EXIT_MISMATCH
    except Exception as e:  # no GPU, extension missing, bad argument
        rec = {"error": f"{type(e).__name__}: {e}"}
        code = EXIT_CANNOT_RUN
    rec["device"] = args.device
    print(json.dumps(rec), flush=True)
    return code


if __name__ == "__main__":
    sys.exit(main())
