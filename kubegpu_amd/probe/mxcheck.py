"""Active matrix-core format probe — wrapper over the mxcheck HIP kernel.

``cucheck`` reaches the matrix cores only through their int8 and bf16
instructions.  This probe is its twin for the formats an MI355X is
mostly picked for: f16, OCP fp8 (e4m3fn x e5m2), the block-scaled MX
path with e2m1 (MXFP4) operands and E8M0 scales, and the f64 matrix
core.  A matrix core that decodes e2m1 wrongly, applies the wrong block
scale or drops an f64 partial product moves no ECC counter and passes
memcheck, cucheck and hostlink.  ``mxcheck()`` launches one 16-wave
workgroup per compute unit; every wave runs the same deterministic
workload and compares four 32-bit digests per round with
``reference_digests``, computed here in numpy.  Launch shape, accounting
and the mismatch log (XCD, shader engine, shader array, CU, SIMD of the
wave that disagreed) are cucheck's.

The workload (csrc/mxcheck.hip; ``reference_digests`` is the
definition).  Arithmetic is mod 2**32; ``fmix32``, ``base``, ``salt``
are cucheck's and the stage number fed to ``base`` is 4 + s, so the
inputs differ from cucheck's:

  word(s, r, idx) = fmix32(base(seed, 4 + s, r) + idx)
  sext(x, n)      = the low n bits of x as a two's-complement integer
  fold32(C)       = sum over i, j of fmix32(u32(C[i][j]) + salt(32i + j))

  0 mfma_f16    32 x 128 by 128 x 32, two 16-bit halves per word:
                A[i][k] = sext(word(0, r, 64i + k/2) >> 16(k%2), 11)
                B[k][j] = sext(word(0, r, 2048 + 64j + k/2) >> 16(k%2), 5)
                f16 operands, f32 accumulate; |C| <= 2**21;
                digest = fold32(C)
  1 mfma_fp8    32 x 128 by 128 x 32, one byte x per element:
                A[i][k] = E4M3[(x & 0x87) | (7 + ((x>>3) & 3)) << 3],
                          x = byte k%4 of word(1, r, 32i + k/4)
                B[k][j] = E5M2[(x & 0x83) | (15 + ((x>>2) & 3)) << 2],
                          x = byte k%4 of word(1, r, 1024 + 32j + k/4)
                so A = +-(8+m) * 2**(0..3) / 8 and B = +-(4+m) * 2**(0..3) / 4:
                every sign and mantissa, four exponents.  Zero,
                subnormals, Inf and NaN are not covered.
                |32 C| < 2**20; digest = fold32(32 C)
  2 mfma_mxfp4  32 x 256 by 256 x 32, eight e2m1 nibbles per word, one
                E8M0 scale per 32 elements of k:
                A[i][k]  = E2M1[nibble k%8 of word(2, r, 32i + k/8)]
                B[k][j]  = E2M1[nibble k%8 of word(2, r, 1024 + 32j + k/8)]
                SA[i][b] = 127 + ((word(2, r, 2048 + i) >> 2b) & 3), b = 0..7
                SB[j][b] = 127 + ((word(2, r, 2080 + j) >> 2b) & 3)
                C[i][j]  = sum over k of A[i][k] 2**(SA[i][k/32] - 127)
                                         * B[k][j] 2**(SB[j][k/32] - 127)
                all sixteen e2m1 codes, scales 2**0 .. 2**3;
                |4 C| <= 256 * 144 * 64 < 2**22; digest = fold32(4 C)
  3 mfma_f64    16 x 32 by 32 x 16:
                A[i][k] = sext(word(3, r, 32i + k), 24)
                B[k][j] = sext(word(3, r, 512 + 32j + k), 24)
                |C| < 2**51; with C as a two's-complement int64,
                digest = sum over i, j of fmix32(lo32(C) + salt(16i + j))
                                        + fmix32(hi32(C) + salt(256 + 16i + j))

Every stage uses only operands for which all partial sums are exactly
representable in the accumulator type, so the reference is integer
arithmetic, the result does not depend on the order the hardware sums
in — and rounding logic is not covered (``probe/fpcheck.py``'s ground).

How the kernel feeds the instructions (proved element by element by the
GPU test of ``wave_tile`` against ``matmul_tile``): in the 32x32 stages
lane l holds row l&31 of A and column l&31 of B, and in step s the lane
half h = l>>5 holds the h-th half of the step's k range.  C = A.B does
not change under a permutation of k applied to A and B alike, so the k
order inside a fragment does not matter; for the scaled instruction
only the lane-to-block assignment does: step s, half h holds 32-element
block 2s + h in the first four operand registers, format field 4
(e2m1) for A and B, and byte 0 of the lane's own scale register
(op_sel 0) scales exactly those 32 elements.  The f64 instruction takes
A[l&15][4s + (l>>4)] and B[4s + (l>>4)][l&15] from lane l and returns
row (l>>4) + 4g, column l&15 in result register g.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.mxcheck --device INDEX [--rounds N] [--seed S]
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
)

STAGES: Tuple[str, ...] = ("mfma_f16", "mfma_fp8", "mfma_mxfp4", "mfma_f64")
# what one unit of a stage's integer tile stands for: C = tile / UNIT
UNITS: Tuple[int, ...] = (1, 32, 4, 1)
TILE_DIMS: Tuple[int, ...] = (32, 32, 32, 16)
_STAGE0 = 4  # stage number fed to base() is _STAGE0 + s
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/mxcheck_mi355x.json): 16.9 us per round
# with the default grid (256 workgroups, 4096 waves), flat from 1024 to
# 29696 rounds, so 0.5 s are 29.6 x 1024 rounds; 29 x 1024 take 0.50 s.
# Operand generation sets the time, not the matrix cores.  The numpy
# table for it cost 1.6 s of host time there.
DEFAULT_ROUNDS = 29696

# flops one wave spends in the matrix cores per round, per stage
_FLOPS_PER_WAVE_ROUND = (2 * 32 * 32 * 128, 2 * 32 * 32 * 128,
                         2 * 32 * 32 * 256, 2 * 16 * 16 * 32)
_REF_CHUNK = 128  # rounds per numpy batch


# -- decode tables ---------------------------------------------------------------

def _fp8_table(exp_bits: int, man_bits: int, bias: int, fn: bool) -> Tuple[float, ...]:
    """All 256 codes of an OCP 8-bit float; ``fn`` = the finite-only
    flavour (no Inf, NaN only at S.1111.111)."""
    out = []
    top = (1 << exp_bits) - 1
    for code in range(256):
        sign = -1.0 if code & 0x80 else 1.0
        e = (code >> man_bits) & top
        m = code & ((1 << man_bits) - 1)
        if e == 0:
            v = m * 2.0 ** (1 - bias - man_bits)
        elif e == top and not fn:
            v = float("inf") if m == 0 else float("nan")
        elif e == top and m == (1 << man_bits) - 1:
            v = float("nan")
        else:
            v = ((1 << man_bits) + m) * 2.0 ** (e - bias - man_bits)
        out.append(sign * v)
    return tuple(out)


E4M3: Tuple[float, ...] = _fp8_table(4, 3, 7, True)  # OCP e4m3fn: code -> value
E5M2: Tuple[float, ...] = _fp8_table(5, 2, 15, False)  # OCP e5m2
# OCP e2m1, the MXFP4 element
E2M1: Tuple[float, ...] = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0,
                           -0.0, -0.5, -1.0, -1.5, -2.0, -3.0, -4.0, -6.0)


def e8m0(byte: int) -> float:
    """Value of an E8M0 block scale: 2**(byte - 127); 255 is NaN."""
    byte = int(byte)
    if not 0 <= byte <= 255:
        raise ValueError(f"e8m0: byte out of range: {byte}")
    return float("nan") if byte == 255 else 2.0 ** (byte - 127)


def e4m3_code(x):
    """The e4m3 code stage 1 makes of a raw byte: sign and mantissa
    kept, exponent field 7 + two bits."""
    return (x & 0x87) | ((7 + ((x >> 3) & 3)) << 3)


def e5m2_code(x):
    """The e5m2 code stage 1 makes of a raw byte."""
    return (x & 0x83) | ((15 + ((x >> 2) & 3)) << 2)


# -- numpy definition ----------------------------------------------------------

def _words(seed: int, stage: int, r, first: int, count: int):
    """word(stage, r, first .. first+count-1) as uint32[len(r), count]."""
    import numpy as np

    idx = np.arange(first, first + count, dtype=np.uint32)
    return _fmix32(_base(seed, _STAGE0 + stage, r)[:, None] + idx[None, :])


def _fields(words, dtype):
    """uint32[n, m] -> dtype[n, m * 4/itemsize]: the words cut into
    little-endian fields, lowest first."""
    import numpy as np

    return np.ascontiguousarray(words).astype("<u4").view(dtype)


def _nibbles(words):
    """uint32[n, m] -> uint8[n, 8m], lowest nibble first."""
    import numpy as np

    b = _fields(words, np.uint8)
    out = np.empty(b.shape + (2,), dtype=np.uint8)
    out[..., 0] = b & 15
    out[..., 1] = b >> 4
    return out.reshape(b.shape[0], -1)


def _scale_bits(words):
    """uint32[n, 32] -> uint8[n, 32, 8]: two bits per k-block, lowest first."""
    import numpy as np

    shifts = np.arange(0, 16, 2, dtype=np.uint32)
    return ((words[:, :, None] >> shifts[None, None, :]) & np.uint32(3)).astype(np.uint8)


def operands(seed: int, stage: int, r):
    """(A, Bt) of a stage for rounds ``r`` (uint32 array) as float arrays
    [len(r), n, K] holding exact integers (float32 in stages 0-2, float64
    in stage 3: the accumulator's type), in units whose product is the
    stage's unit; Bt[j][k] = B[k][j].  Stage 1: A in 1/8, B in 1/4.
    Stage 2: both in 1/2, the block scales multiplied in."""
    import numpy as np

    n = len(r)
    if stage == 0:
        # sign extension of the low 11 / 5 bits by two int16 shifts
        a = (_fields(_words(seed, 0, r, 0, 2048), "<i2") << 5) >> 5
        b = (_fields(_words(seed, 0, r, 2048, 2048), "<i2") << 11) >> 11
        return (a.astype(np.float32).reshape(n, 32, 128),
                b.astype(np.float32).reshape(n, 32, 128))
    if stage == 1:
        # byte -> value of its masked code, in 1/8 and 1/4 (never NaN or Inf)
        e4 = (np.array(E4M3)[e4m3_code(np.arange(256))] * 8).astype(np.float32)
        e5 = (np.array(E5M2)[e5m2_code(np.arange(256))] * 4).astype(np.float32)
        a = np.take(e4, _fields(_words(seed, 1, r, 0, 1024), np.uint8))
        b = np.take(e5, _fields(_words(seed, 1, r, 1024, 1024), np.uint8))
        return a.reshape(n, 32, 128), b.reshape(n, 32, 128)
    if stage == 2:
        # one 64-entry table: value of nibble | scale bits << 4, in 1/2
        # (E8M0 byte 127 + s: times 2**s)
        e2 = (np.array(E2M1)[None, :] * np.array([2.0, 4.0, 8.0, 16.0])[:, None])
        e2 = e2.reshape(64).astype(np.float32)
        a = _nibbles(_words(seed, 2, r, 0, 1024)).reshape(n, 32, 8, 32)
        b = _nibbles(_words(seed, 2, r, 1024, 1024)).reshape(n, 32, 8, 32)
        a |= (_scale_bits(_words(seed, 2, r, 2048, 32)) << 4)[:, :, :, None]
        b |= (_scale_bits(_words(seed, 2, r, 2080, 32)) << 4)[:, :, :, None]
        return np.take(e2, a).reshape(n, 32, 256), np.take(e2, b).reshape(n, 32, 256)
    if stage == 3:
        # sign extension of the low 24 bits by two int32 shifts
        a = (_words(seed, 3, r, 0, 512).view(np.int32) << 8) >> 8
        b = (_words(seed, 3, r, 512, 512).view(np.int32) << 8) >> 8
        return (a.astype(np.float64).reshape(n, 16, 32),
                b.astype(np.float64).reshape(n, 16, 32))
    raise ValueError(f"stage {stage} out of range 0..3")


def block_scales(seed: int, r: int):
    """(SA, SB) of stage 2 for one round: the E8M0 bytes, uint8[32, 8]."""
    import numpy as np

    rr = np.array([r], dtype=np.uint32)
    seed = int(seed) & 0xFFFFFFFF
    return (127 + _scale_bits(_words(seed, 2, rr, 2048, 32))[0],
            127 + _scale_bits(_words(seed, 2, rr, 2080, 32))[0])


def matmul_tile(seed: int, stage: int, r: int):
    """The exact product of a stage for one round as int64 in the stage's
    unit (C, 32 C, 4 C, C): [32, 32], or [16, 16] for stage 3 — what the
    digest is folded from."""
    import numpy as np

    a, bt = operands(int(seed) & 0xFFFFFFFF, stage, np.array([r], dtype=np.uint32))
    return a[0].astype(np.int64) @ bt[0].astype(np.int64).T


def fold_tile(stage: int, tile):
    """The uint32 digest of a stage's tile in the stage's unit
    (``wave_tile`` or ``matmul_tile``), by the module docstring's
    definition.  Leading axes are kept: tile[..., n, n] gives
    digests[...]."""
    import numpy as np

    stage = int(stage)
    if stage not in range(len(STAGES)):
        raise ValueError(f"fold_tile: stage must be in 0..3, got {stage}")
    tile, n = np.asarray(tile), TILE_DIMS[stage]
    if tile.shape[-2:] != (n, n):
        raise ValueError(f"fold_tile: stage {stage} takes [..., {n}, {n}], got {tile.shape}")
    c = tile.astype(np.int64).reshape(tile.shape[:-2] + (n * n,))
    idx = np.arange(n * n, dtype=np.uint32)  # n*i + j, row-major
    with np.errstate(over="ignore"):
        h = _fmix32((c & 0xFFFFFFFF).astype(np.uint32) + _salt(idx))
        if stage == 3:
            hi = ((c >> 32) & 0xFFFFFFFF).astype(np.uint32)
            return (h.sum(axis=-1, dtype=np.uint32)
                    + _fmix32(hi + _salt(idx + np.uint32(256))).sum(axis=-1, dtype=np.uint32))
        return h.sum(axis=-1, dtype=np.uint32)


def _digests(seed: int, stage: int, r):
    import numpy as np

    a, bt = operands(seed, stage, r)
    # every partial sum is an integer below 2**24 in stages 0-2 (float32)
    # and below 2**53 in stage 3 (float64): products and sums are exact
    # in any order, and BLAS is fast
    return fold_tile(stage, np.matmul(a, bt.transpose(0, 2, 1)))


def reference_digests(seed: int, rounds: int):
    """Expected digests as uint32[rounds, 4], columns in STAGES order.

    Pure numpy: needs neither torch nor a GPU.  This is the definition
    the GPU kernel is tested against."""
    import numpy as np

    seed = int(seed) & 0xFFFFFFFF
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("reference_digests: rounds >= 0 required")
    out = np.empty((rounds, len(STAGES)), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rounds, _REF_CHUNK):
            r = np.arange(lo, min(lo + _REF_CHUNK, rounds), dtype=np.uint32)
            for s in range(len(STAGES)):
                out[lo:lo + len(r), s] = _digests(seed, s, r)
    return out


# -- GPU run ---------------------------------------------------------------------

@dataclass
class MxcheckResult(DigestResult):
    # Whole-run lower bounds per stage (the kernel's time also holds
    # operand generation, the other stages and the digests): informative.
    mfma_f16_tflops: float = 0.0
    mfma_fp8_tflops: float = 0.0
    mfma_mxfp4_tflops: float = 0.0
    mfma_f64_tflops: float = 0.0


def mxcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> MxcheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup asks for a CU's whole LDS without touching it, so on an
    idle GPU the default grid lands one workgroup on every CU;
    ``cus_covered`` reports how many distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot corrupt a
    matrix core."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    return _digest.run_probe(
        "mxcheck", MxcheckResult(rounds=rounds), STAGES, _FLOPS_PER_WAVE_ROUND, 1e12,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected)


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``mxcheck`` with its dump pointer set."""
    return _digest.wave_digests(
        "mxcheck", _ext().mxcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device)


def wave_tile(seed: int, stage: int, r: int, device=None):
    """The accumulator tile wave 0 of one workgroup computed for a stage
    and round, as int64 in the stage's unit like ``matmul_tile``: [32, 32],
    or [16, 16] for stage 3.  A digest cannot say which element is wrong;
    this can.  Raises if an element is no integer in that unit."""
    import numpy as np
    import torch

    with torch.cuda.device(_device(device)):
        tile = _ext().mxcheck_tile(int(seed), int(stage), int(r)).cpu().numpy()
    out = tile.astype(np.int64)
    if not np.array_equal(out.astype(np.float64), tile):
        raise ValueError(f"mxcheck: stage {stage} tile holds non-integers")
    return out


# -- child process -----------------------------------------------------------

def run_mxcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                           timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the mxcheck CLI."""
    return _active.run_probe_subprocess("mxcheck", index, "--rounds", rounds, timeout_s)


def mxcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                  rounds: int = DEFAULT_ROUNDS,
                  max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("mxcheck", "mismatches", _digest.metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "mxcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: mxcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
