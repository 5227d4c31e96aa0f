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
nor is the path to HBM (memcheck's ground).  The LDS stage uses plain
reads and writes only: LDS, L2 and memory-side atomics are
``probe/atomcheck.py``'s ground.

A digest says that something in a stage is wrong, not what.  Three
functions give the values the digests are folded from, for one wave,
stage and round:

  wave_values(seed, stage, r, lds_bytes, wave)   what the GPU computed: the
                    kernel's own stage code with a sink that stores
                    instead of folding, run by one wave of one workgroup
  reference_values(seed, stage, r, lds_dwords)   the same in numpy
  fold_values(stage, values)                     the digest of either

Value layouts, the same for both:

  0, 1  int64[32, 32]          C[i][j] as above, read out of the
                               accumulator registers through the C/D map
                               the fold uses
  2     uint32[32, 64]         [it, l] = x of lane l after iteration it;
                               the digest folds the last row only
  3     uint32[2, lds_dwords]  [p, d] = the word read back from dword d
                               of the wave's slice in pass p: v[d], ~v[d]

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.cucheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

from . import _active, _digest
from ._active import (  # noqa: F401
    EXIT_CANNOT_RUN,
    EXIT_MISMATCH,
    EXIT_PASS,
    _REPO_ROOT,
    _child_lock,
    _ext,
    idle_gpus,
)
from ._digest import (  # noqa: F401
    WAVES_PER_BLOCK,
    DigestResult,
    _base,
    _device,
    _fmix32,
    _salt,
    cu_key,
)

STAGES: Tuple[str, ...] = ("mfma_i8", "mfma_bf16", "valu", "lds")
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
# (rows, cols) of a stage's values; 0 stands for lds_dwords
_VALUE_SHAPES = ((32, 32), (32, 32), (32, 64), (2, 0))


# -- numpy definition ----------------------------------------------------------

def _words(seed: int, stage: int, r, first: int, count: int):
    """word(seed, stage, r, first .. first+count-1) as uint32[len(r), count]."""
    import numpy as np

    idx = np.arange(first, first + count, dtype=np.uint32)
    return _fmix32(_base(seed, stage, r)[:, None] + idx[None, :])


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
    return fold_values(stage, c)


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


def _check_stage(who: str, stage: int) -> int:
    stage = int(stage)
    if stage not in range(len(STAGES)):
        raise ValueError(f"{who}: stage must be in 0..3, got {stage}")
    return stage


def reference_values(seed: int, stage: int, r: int, lds_dwords: int = 2560):
    """The values one wave's digest of ``stage`` in round ``r`` is folded
    from, in the layouts of the module docstring.  Pure numpy."""
    import numpy as np

    stage = _check_stage("reference_values", stage)
    seed, r, lds_dwords = int(seed) & 0xFFFFFFFF, int(r), int(lds_dwords)
    if not 0 <= r < 65536 or lds_dwords <= 0:
        raise ValueError("reference_values: r in 0..65535 and lds_dwords > 0 required")
    if stage in (0, 1):
        return matmul_tile(seed, stage, r)
    rr = np.array([r], dtype=np.uint32)
    with np.errstate(over="ignore"):
        if stage == 3:
            v = _words(seed, 3, rr, 0, lds_dwords)[0]
            return np.stack([v, ~v])
        x = _words(seed, 2, rr, 0, 64)[0]
        trace = np.empty((32, 64), dtype=np.uint32)
        for it in range(32):
            x = x * np.uint32(0x9E3779B1) + ((x << np.uint32(13)) | (x >> np.uint32(19)))
            x = x ^ ((x.astype(np.uint64) * np.uint64(0x85EBCA6B))
                     >> np.uint64(32)).astype(np.uint32)
            # a*b + c < 2**24: the f32 FMA is exact, so integers define it
            x = x + (x & np.uint32(0xFFF)) * ((x >> np.uint32(12)) & np.uint32(0xFFF)) \
                + (x >> np.uint32(24))
            trace[it] = x
    return trace


def fold_values(stage: int, values):
    """The uint32 digest of one wave's values (``wave_values`` or
    ``reference_values``), by the module docstring's definition.  Leading
    axes are kept: values[..., rows, cols] gives digests[...]."""
    import numpy as np

    stage = _check_stage("fold_values", stage)
    values = np.asarray(values)
    rows, cols = _VALUE_SHAPES[stage]
    if values.ndim >= 2 and cols == 0:
        cols = values.shape[-1]  # lds_dwords
    if values.ndim < 2 or values.shape[-2:] != (rows, cols) or cols == 0:
        raise ValueError(f"fold_values: stage {stage} takes [..., {rows}, "
                         f"{cols or 'lds_dwords'}], got {values.shape}")
    lead = values.shape[:-2]
    with np.errstate(over="ignore"):
        if stage in (0, 1):
            cu = (values.astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)
            salt = _salt(np.arange(1024, dtype=np.uint32))  # 32*i + j, row-major
            h = _fmix32(cu.reshape(lead + (1024,)) + salt)
        elif stage == 2:
            h = _fmix32(values[..., -1, :].astype(np.uint32)
                        + np.arange(64, dtype=np.uint32))
        else:
            salt = _salt(np.arange(cols, dtype=np.uint32))
            h = _fmix32(values.astype(np.uint32) + salt).reshape(lead + (2 * cols,))
        return h.sum(axis=-1, dtype=np.uint32)


# -- GPU run ---------------------------------------------------------------------

@dataclass
class CucheckResult(DigestResult):
    # Whole-run lower bounds (the kernel's time also holds operand
    # generation, the VALU and LDS stages and the digests): informative.
    mfma_i8_tops: float = 0.0
    mfma_bf16_tflops: float = 0.0


def _decode_record(raw) -> dict:
    return _digest.decode_record(raw, STAGES)


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
    rounds, blocks, lds_bytes = int(rounds), int(blocks), int(lds_bytes)
    seed = int(seed)
    if lds_bytes < 4096 or lds_bytes > DEFAULT_LDS_BYTES or lds_bytes % 4096:
        raise ValueError(
            f"cucheck: lds_bytes must be a multiple of 4096 in 4096..163840, got {lds_bytes}")
    return _digest.run_probe(
        "cucheck", CucheckResult(rounds=rounds), STAGES,
        (_I8_OPS_PER_WAVE_ROUND, _BF16_FLOPS_PER_WAVE_ROUND), 1e12,
        lambda: reference_digests(seed, rounds, lds_bytes // 64),
        seed, blocks, max_records, device, _inject, _expected, lds_bytes)


def wave_digests(seed: int, rounds: int, blocks: int = 0,
                 lds_bytes: int = DEFAULT_LDS_BYTES, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``cucheck`` with its dump pointer set."""
    lds_bytes = int(lds_bytes)
    return _digest.wave_digests(
        "cucheck", _ext().cucheck_run, reference_digests(seed, rounds, lds_bytes // 64),
        STAGES, seed, rounds, blocks, device, lds_bytes)


def wave_values(seed: int, stage: int, r: int, lds_bytes: int = DEFAULT_LDS_BYTES,
                wave: int = 0, device=None):
    """What wave ``wave`` (0..15) of one workgroup with ``lds_bytes`` of
    LDS computed for a stage and round, shaped like ``reference_values``:
    the production kernel's stage code storing every value instead of
    folding it.  A digest cannot say which element is wrong; this can."""
    import numpy as np
    import torch

    stage = _check_stage("wave_values", stage)
    with torch.cuda.device(_device(device)):
        raw = _ext().cucheck_values(
            int(seed), stage, int(r), int(lds_bytes), int(wave)).cpu().numpy()
    if stage in (0, 1):
        return raw
    if (raw >> 32).any():
        raise RuntimeError(f"cucheck: stage {stage} dump holds more than 32 bits")
    return raw.astype(np.uint32)


# -- child process -----------------------------------------------------------

def run_cucheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                           timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the cucheck CLI."""
    return _active.run_probe_subprocess("cucheck", index, "--rounds", rounds, timeout_s)


def cucheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                  rounds: int = DEFAULT_ROUNDS,
                  max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("cucheck", "mismatches", _digest.metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "cucheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: cucheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
