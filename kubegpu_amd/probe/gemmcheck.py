"""Active full-chip load probe: a tiled GEMM over the whole GPU, compared
digest by digest — wrapper over the gemmcheck HIP kernel.

The other active probes isolate one unit each with a short workload made
in registers.  This one checks the GPU while it does the job it is
scheduled for: ``C[M,N] = A[M,K] . Bt[N,K]^T`` with HBM, L2, LDS and the
matrix cores busy on every CU at once, many GEMMs in one launch, in bf16
(``v_mfma_f32_32x32x16_bf16``, f32 accumulators) and in i8
(``v_mfma_i32_32x32x32_i8``, i32 accumulators).  Marginal parts fail under
combined load first; ECC does not see a wrong product.  ``gemm_nt`` is the
same kernel with a store sink: the public NT GEMM.

The workload (csrc/gemmcheck.hip; this module is the definition).
Arithmetic is mod 2**32; ``fmix32``, ``base``, ``salt`` are cucheck's:

  word(s, r, idx) = fmix32(base(seed, s, r) + idx)
  A[i][k]  = val(word(70, i % 256, k)),   Bt[j][k] = val(word(71, j % 256, k))
  val(w)   = the low 5 bits of w as a two's-complement integer (-16..15)
             for bf16, the low byte as a signed byte for i8
  bits(c)  = the i32 value, or the f32 bit pattern with any zero as 0
  fold(T, q) = sum over the 64 x 64 quadrant q = 2 (i // 64) + (j // 64) of
               a 128 x 128 tile T of fmix32(bits(T[i][j]) + salt(128 i + j))

The content repeats every 256 rows, so a tile (bi, bj) of C is one of four
classes 2 (bi % 2) + (bj % 2), and a workgroup that reads the neighbouring
row block folds to another value.  The 256 x K blocks are uploaded once
and repeated on the device: the HBM and L2 traffic is real, only the
content repeats.  For bf16 every product is at most 256 in magnitude, so
every partial sum in any order stays at or below 2**23 for K <= 32768 and
is exact in f32; for i8 products are at most 2**14 and the sums stay below
2**31 for K < 131072.  ``reference_expected`` is therefore the float64
product of the two blocks (exact), folded per class and quadrant, and the
GPU's folds are compared bit for bit: ``expected[class][quadrant]``.

A workgroup of four waves owns a tile and wave q its quadrant q; the
kernel walks ``t = block; t < rounds * tiles; t += blocks`` with the round
as the slow index, and ``step_tile`` is its map from ``t % tiles`` to
(bi, bj).  A wrong fold is logged with tile ``bi * (N // 128) + bj``,
quadrant, round, dtype and the place the hardware says the wave ran.

``ok`` is about folds only.  ``tflops`` (2 M N K rounds / elapsed, from
shapes) is reported and never changes health, like hostlink's bandwidth.
Measured on MI355X at 8192 x 8192 x 8192: 530 TFLOP/s in bf16 and 1252
TOP/s in i8 sustained, 29 % of torch.matmul's bf16 rate on the same
operands (DEFAULT_ROUNDS below, profiles/gemmcheck_mi355x.json).

Not covered: power, clock and temperature under load; shapes that are no
multiple of the tile; fp8 and MX operands; address tagging finer than the
four classes (memcheck's and vmemcheck's ground).

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.gemmcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from . import _active, _digest
from ._digest import _base, _device, _fmix32, _salt

DTYPES: Tuple[str, ...] = ("bf16", "i8")  # the kernel's stage 0 and 1
TILE = 128
PERIOD = 256  # rows after which the operands' content repeats
SLAB = {"bf16": 64, "i8": 128}  # elements of K per 128-byte slab
MAX_K = {"bf16": 32768, "i8": 131071}
_STAGE_A, _STAGE_BT = 70, 71
# One default run of both dtypes should hold the GPU for about a second.
# Measured on MI355X at 8192 x 8192 x 8192 on the default grid (512
# workgroups) in windows of 1.7 to 2.2 s (profiles/gemmcheck_mi355x.json):
# 2.078 ms per round in bf16 (530 TFLOP/s) and 0.879 ms in i8 (1252 TOP/s),
# 2.957 ms for both, so 1 s is 338 rounds; 340 take 1.005 s.  (Windows of
# 16 rounds run at 911 TFLOP/s and 1689 TOP/s: the rate falls under
# sustained load.  torch.matmul takes 0.607 ms on the bf16 operands.)
DEFAULT_ROUNDS = 340


# -- numpy definition ----------------------------------------------------------

def _check_dtype(dtype: str) -> str:
    if dtype not in DTYPES:
        raise ValueError(f"gemmcheck: dtype must be one of {DTYPES}, got {dtype!r}")
    return dtype


def operand_block(seed: int, dtype: str, k: int):
    """The 256 x k blocks (A, Bt) the operands repeat, as int8 values."""
    import numpy as np

    _check_dtype(dtype)
    seed, k = int(seed) & 0xFFFFFFFF, int(k)
    if k < 1 or k % SLAB[dtype] or k > MAX_K[dtype]:
        raise ValueError(f"gemmcheck: K must be a multiple of {SLAB[dtype]} in "
                         f"{SLAB[dtype]}..{MAX_K[dtype]} for {dtype}, got {k}")
    rows = np.arange(PERIOD, dtype=np.uint32)
    idx = np.arange(k, dtype=np.uint32)
    out = []
    with np.errstate(over="ignore"):
        for stage in (_STAGE_A, _STAGE_BT):
            w = _fmix32(_base(seed, stage, rows)[:, None] + idx[None, :])
            if dtype == "bf16":
                out.append((((w & np.uint32(31)) ^ np.uint32(16)).astype(np.int8) - np.int8(16)))
            else:
                out.append((w & np.uint32(0xFF)).astype(np.uint8).view(np.int8))
    return out[0], out[1]


def operands(seed: int, dtype: str, m: int, n: int, k: int, device=None):
    """(A [m, k], Bt [n, k]) on the GPU as bfloat16 or int8: the blocks of
    ``operand_block`` uploaded once and repeated on the device."""
    import torch

    m, n = int(m), int(n)
    if m < TILE or n < TILE or m % TILE or n % TILE:
        raise ValueError(f"gemmcheck: M and N must be multiples of {TILE}, got {m} and {n}")
    device = _device(device)
    kind = torch.bfloat16 if dtype == "bf16" else torch.int8
    out = []
    for block, rows in zip(operand_block(seed, dtype, k), (m, n)):
        t = torch.from_numpy(block).to(device).to(kind)
        out.append(t.repeat(-(-rows // PERIOD), 1)[:rows].contiguous())
    return out[0], out[1]


def tile_bits(dtype: str, c):
    """bits() of exact values c[...] as uint32."""
    import numpy as np

    c = np.asarray(c)
    if _check_dtype(dtype) == "i8":
        return c.astype(np.int64).astype(np.uint32)
    b = c.astype(np.float32).view(np.uint32).copy()
    b[c == 0] = 0
    return b


def fold_tiles(bits):
    """fold() of uint32 bit patterns [..., 128, 128] -> uint32[..., 4], one
    per quadrant."""
    import numpy as np

    bits = np.asarray(bits, dtype=np.uint32)
    i = np.arange(TILE, dtype=np.uint32)
    with np.errstate(over="ignore"):
        mixed = _fmix32(bits + _salt(np.uint32(TILE) * i[:, None] + i[None, :]))
    quads = mixed.reshape(bits.shape[:-2] + (2, TILE // 2, 2, TILE // 2))
    return quads.sum(axis=(-3, -1), dtype=np.uint32).reshape(bits.shape[:-2] + (4,))


def split_tiles(c):
    """[M, N] -> [M // 128, N // 128, 128, 128]."""
    m, n = c.shape
    return c.reshape(m // TILE, TILE, n // TILE, TILE).transpose(0, 2, 1, 3)


def reference_expected(seed: int, dtype: str, k: int):
    """Expected folds as uint32[4, 4]: [class 2 (bi % 2) + (bj % 2)][quadrant].

    Pure numpy: needs neither torch nor a GPU.  This is the definition the
    GPU kernel is tested against."""
    import numpy as np

    a, bt = operand_block(seed, dtype, k)
    c = a.astype(np.float64) @ bt.astype(np.float64).T  # exact: see the module docstring
    return fold_tiles(split_tiles(tile_bits(dtype, c))).reshape(4, 4)


def step_tile(u: int, tm: int, tn: int) -> Tuple[int, int]:
    """The kernel's map from step u of a round to the tile (bi, bj) of a
    tm x tn grid: the steps that land on one XCD (u % 8) run through 8 x 8
    super-blocks of tiles where the grid allows it, else row-major."""
    if tm % 8 == 0 and tn % 8 == 0 and ((tm // 8) * (tn // 8)) % 8 == 0:
        v = u >> 3
        sb, sn = ((v >> 6) << 3) | (u & 7), tn // 8
        return 8 * (sb // sn) + ((v >> 3) & 7), 8 * (sb % sn) + (v & 7)
    return u // tn, u % tn


# -- GPU run ---------------------------------------------------------------------

@dataclass
class GemmcheckResult:
    ok: bool = True
    m: int = 0
    n: int = 0
    k: int = 0
    rounds: int = 0
    waves: int = 0
    mismatches: int = 0
    first_bad_round: Optional[int] = None
    bad_stages: List[str] = field(default_factory=list)  # dtypes with a wrong fold
    # {"tile", "quadrant", "round", "dtype", "xcc", "se", "sh", "cu", "simd",
    #  "expected", "got"} per logged fold
    records: List[Dict] = field(default_factory=list)
    records_dropped: int = 0
    cus_covered: int = 0  # distinct CUs that ran at least one wave
    cu_count: int = 0  # multiProcessorCount
    bad_cus: List[str] = field(default_factory=list)  # "xcc/se/sh/cu"
    elapsed_s: Dict[str, float] = field(default_factory=dict)  # per dtype
    tflops: Dict[str, float] = field(default_factory=dict)  # per dtype, from shapes
    waves_on: List[int] = field(default_factory=list, repr=False)

    def to_dict(self) -> dict:
        out = {f: getattr(self, f) for f in (
            "ok", "m", "n", "k", "rounds", "waves", "mismatches", "first_bad_round",
            "records_dropped", "cus_covered", "cu_count")}
        out.update(bad_stages=list(self.bad_stages), records=[dict(r) for r in self.records],
                   bad_cus=list(self.bad_cus), elapsed_s=dict(self.elapsed_s),
                   tflops=dict(self.tflops))
        return out


def _decode(raw) -> dict:
    rec = _digest.decode_record(raw, DTYPES)
    where = rec.pop("wave")
    del rec["block"]
    return dict(rec, tile=where >> 2, quadrant=where & 3, dtype=rec.pop("stage"))


def gemmcheck(
    seed: int = 0,
    m: int = 8192,
    n: int = 8192,
    k: int = 8192,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    dtypes: Sequence[str] = DTYPES,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[str, int, int, int]] = None,
) -> GemmcheckResult:
    """Run ``rounds`` GEMMs of [m, k] by [n, k] per dtype in one launch each
    on ``blocks`` workgroups of four waves (0 = two per CU, or one per tile
    step if that is fewer) and compare every wave's fold with
    ``reference_expected``.

    The operands are taken from free VRAM: 2 (m + n) k bytes at most; where
    they do not fit the probe raises, which says nothing about the hardware.

    ``_inject=(dtype, wave of the grid, round, xor_mask)`` flips bits of
    the fold that wave computes for the first tile of its workgroup in that
    round; a test hook, since a test cannot corrupt a matrix core."""
    import torch

    seed, m, n, k, rounds, blocks = (int(x) for x in (seed, m, n, k, rounds, blocks))
    if not 1 <= rounds <= 65536:
        raise ValueError(f"gemmcheck: rounds must be in 1..65536, got {rounds}")
    ext = _active._ext()
    device = _device(device)
    res = GemmcheckResult(m=m, n=n, k=k, rounds=rounds)
    res.cu_count = int(torch.cuda.get_device_properties(device).multi_processor_count)
    res.waves_on = [0] * 1024
    need = 2 * (m + n) * k
    free = torch.cuda.mem_get_info(device)[0]
    if need > free:
        raise RuntimeError(f"gemmcheck: operands need {need} bytes, {free} are free")
    with torch.cuda.device(device):
        for dtype in dtypes:
            stage = DTYPES.index(_check_dtype(dtype))
            a, bt = operands(seed, dtype, m, n, k, device)
            table = reference_expected(seed, dtype, k)
            expected = _digest.expected_tensor("gemmcheck", table, 4, range(4), device)
            inject = None
            if _inject is not None and _inject[0] == dtype:
                inject = (int(_inject[1]), int(_inject[2]), stage, int(_inject[3]))
            count, first, _mask, records, waves_on, elapsed = ext.gemmcheck_run(
                a, bt, expected, rounds, blocks, int(max_records), inject)
            del a, bt
            res.waves_on = [x + int(y) for x, y in zip(res.waves_on, waves_on)]
            if count:
                res.mismatches += int(count)
                res.bad_stages.append(dtype)
                res.first_bad_round = int(first) if res.first_bad_round is None \
                    else min(res.first_bad_round, int(first))
            res.records += [_decode(r) for r in records]
            res.elapsed_s[dtype] = float(elapsed)
            res.tflops[dtype] = 2.0 * m * n * k * rounds / elapsed / 1e12 if elapsed > 0 else 0.0
    res.ok = res.mismatches == 0
    res.waves = sum(res.waves_on)
    res.records_dropped = res.mismatches - len(res.records)
    res.cus_covered = sum(1 for x in res.waves_on if x)
    res.bad_cus = sorted({f"{r['xcc']}/{r['se']}/{r['sh']}/{r['cu']}" for r in res.records})
    return res


def gemm_nt(a, bt, blocks: int = 0):
    """``a [M, K] . bt [N, K]^T`` on the GPU of the operands by the gemmcheck
    tile kernel: float32 for bfloat16 operands, int32 for int8.  M and N
    multiples of 128, K a multiple of 64 (bfloat16) or 128 (int8); exact
    whenever every partial sum is representable in the accumulator.
    ``blocks`` workgroups walk the tiles (0 = two per CU)."""
    import torch

    with torch.cuda.device(a.device):
        return _active._ext().gemm_nt(a, bt, int(blocks))


# -- child process -----------------------------------------------------------

def run_gemmcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                             timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the gemmcheck CLI."""
    return _active.run_probe_subprocess("gemmcheck", index, "--rounds", rounds, timeout_s)


def gemmcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                    rounds: int = DEFAULT_ROUNDS,
                    max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("gemmcheck", "mismatches", _digest.metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "gemmcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: gemmcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
