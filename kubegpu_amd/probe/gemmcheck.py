"""Active full-chip load probe: a tiled GEMM over the whole GPU, compared
digest by digest — wrapper over the gemmcheck HIP kernel.

The other active probes isolate one unit each with a short workload made
in registers.  This one checks the GPU while it does the job it is
scheduled for: ``C[M,N] = A[M,K] . Bt[N,K]^T`` with HBM, L2, LDS and the
matrix cores busy on every CU at once, many GEMMs in one launch, in bf16
(``v_mfma_f32_32x32x16_bf16``, f32 accumulators) and in i8
(``v_mfma_i32_32x32x32_i8``, i32 accumulators) by default, and on request
(``dtypes=``) in the block-scaled OCP MX formats mxfp8 (e4m3 elements) and
mxfp4 (e2m1 elements, two per byte), and in the rest of the family
(``MX_EXT_DTYPES``: e5m2, the two packed fp6 formats and e5m2 x e4m3), all on ``v_mfma_scale_f32_32x32x64_f8f6f4`` with one E8M0 scale
byte per row and 32 elements of K.  Marginal parts fail under combined load
first; ECC does not see a wrong product.  ``gemm_nt`` and ``gemm_mx_nt``
are the same kernels with a store sink: the public NT GEMMs.

The workload (csrc/gemmcheck.hip, csrc/gemmcheck_mx.hip,
csrc/gemmcheck_mx6.hip; this module is the definition).
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

The MX stages (``MX_DTYPES``, stages 2 and 3 of the records), with
``sext`` as above and the same fold over f32 bit patterns:

  C[i][j]  = sum over k of A[i][k] 2**(SA[i][k // 32] - 127)
                         * Bt[j][k] 2**(SB[j][k // 32] - 127)
  mxfp8    A[i][k] = e4m3(sext(word(72, i % 256, k), 5)), Bt from word(73, ..):
           the bf16 stage's integers -16..15, all exact in e4m3
  mxfp4    A[i][k] = E2M1[word(72, i % 256, k) & 15], Bt from word(73, ..):
           all sixteen codes; element 2b is the low nibble of byte b
  SA[i][b] = 127 + ra(i % 256) + t(b),  SB[j][b] = 127 + cb(j % 256) - t(b)
  ra(i) = sext(word(74, 0, i), 4), cb(j) = sext(word(75, 0, j), 4): -8..7
  t(b)  = word(76, 0, b) % 17 - 8: -8..8

matcheck's rule: every block of a dot product carries the product scale
2**(ra + cb), so C[i][j] is an integer (mxfp4: a multiple of 1/4) times a
power of two, every partial sum in any order is exact in f32 for K <= 32768
(16 . 16 . K <= 2**23) and K <= 65536 (144 K < 2**24), and a wrong row's
scale, a wrong block's scale or a wrong byte select changes the fold.  No
NaN code and no 0xFF scale appears.

The further MX stages (``MX_EXT_DTYPES``, stages 4..7; a name "FA:FB" gives
A's and Bt's formats, a single name both) take the same words, scales and
product, and only val() is new, on the low byte w of the word:

  e5m2  f = (w >> 2) & 3; code = w & 0x80 if f == 3 else
        (w & 0x83) | ((15 + f) << 2): +-0 and +-(1 + m/4) 2**f, at most 7
  e3m2  the same f; code = w & 0x20 if f == 3 else (w & 0x23) | ((3 + f) << 2):
        the same values
  e2m3  f = (w >> 3) & 3; code = w & 0x27 if f == 3 else w & 0x3F: exponent
        field 3 folds to 0, the subnormals; at most 3.75, multiples of 1/8
  mxfp8_e5m2 e5m2 x e5m2, mxfp6_e2m3 and mxfp6_e3m2 both operands alike,
  mxfp8_e5m2:mxfp8 e5m2 x the e4m3 integers of mxfp8
  fp6 in memory: 24 bytes per 32 elements, element e of the block bits
  6e..6e+5 of that 192-bit little-endian integer; K per slab is 128 for all

Bounds, in units of the product scale: products are at most 784 sixteenths
(e5m2, e3m2) or 900 sixty-fourths (e2m3), exact up to K = 16384 (900 . 16384
< 2**24); 448 quarters (mxfp8_e5m2:mxfp8), exact up to K = 32768 (448 . 32768
< 2**24): ``MAX_K``.

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

The MX stages, measured on MI355X at 8192 x 8192 x 8192 in windows of 2.0
to 2.1 s alternating with the bf16 stage (profiles/gemmcheck_mx_mi355x.json):
1229 TFLOP/s in mxfp8 (0.895 ms per round) and 2598 TFLOP/s in mxfp4
(0.423 ms), with bf16 at 519 TFLOP/s (2.12 ms) in the same session.
``MX_EXT_DTYPES``, six kinds alternating in windows of 2.0 to 2.7 s
(profiles/gemmcheck_mx6_mi355x.json): 1664 TFLOP/s in mxfp8_e5m2 (0.661 ms),
1683 in mxfp8_e5m2:mxfp8 (0.653 ms), 1080 in mxfp6_e2m3 (1.018 ms) and 1078
in mxfp6_e3m2 (1.020 ms), with mxfp8 at 1216 and mxfp4 at 2641 in that
session: fp6 runs below mxfp8, for a reason not yet measured.

Not covered: power, clock and temperature under load; shapes that are no
multiple of the tile; unscaled fp8 and every format pair but e5m2 x e4m3
under load (mxcheck and matcheck probe those instructions in isolation;
e4m3 x e2m1, "mxfp8:mxfp4", was built with an LDS map of its own and gave a
wrong product in every element on an MI355X, the way matcheck's e2m1 x e4m3
form does: no register map is known for fp8 meeting fp4, so it is left out
rather than compared loosely); NaN, Inf (e5m2's too) and scale-NaN under load;
address tagging finer than the four classes (memcheck's and vmemcheck's
ground).

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.gemmcheck --device INDEX [--rounds N] [--seed S]
                                          [--dtypes bf16,i8,mxfp8,mxfp4,mxfp6_e2m3,...]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

from . import _active, _digest
from ._digest import _base, _device, _fmix32, _salt

DTYPES: Tuple[str, ...] = ("bf16", "i8")  # the kernel's stage 0 and 1
MX_DTYPES: Tuple[str, ...] = ("mxfp8", "mxfp4")  # stage 2 and 3, on request only
# stages 4..7, on request only; "FA:FB" names A's and Bt's formats
MX_EXT_DTYPES: Tuple[str, ...] = ("mxfp8_e5m2", "mxfp6_e2m3", "mxfp6_e3m2", "mxfp8_e5m2:mxfp8")
_STAGES = DTYPES + MX_DTYPES + MX_EXT_DTYPES
_MX_STAGES = MX_DTYPES + MX_EXT_DTYPES
# a one-format stage's element format; mx_formats() splits the pairs
_ELEMENT = {"mxfp8": "e4m3", "mxfp4": "e2m1", "mxfp8_e5m2": "e5m2", "mxfp6_e2m3": "e2m3",
            "mxfp6_e3m2": "e3m2"}
_ELEMENT_BITS = {"e4m3": 8, "e5m2": 8, "e2m3": 6, "e3m2": 6, "e2m1": 4}
TILE = 128
PERIOD = 256  # rows after which the operands' content repeats
# elements of K per slab: 128 bytes of a row, and for MX_EXT_DTYPES 128
# elements whatever their width
SLAB = {"bf16": 64, "i8": 128, "mxfp8": 128, "mxfp4": 256, **{d: 128 for d in MX_EXT_DTYPES}}
MAX_K = {"bf16": 32768, "i8": 131071, "mxfp8": 32768, "mxfp4": 65536,
         "mxfp8_e5m2": 16384, "mxfp6_e2m3": 16384, "mxfp6_e3m2": 16384,
         "mxfp8_e5m2:mxfp8": 32768}
MX_BLOCK = 32  # elements of K per E8M0 scale
_STAGE_A, _STAGE_BT = 70, 71
_STAGE_MX_A, _STAGE_MX_BT, _STAGE_RA, _STAGE_CB, _STAGE_T = 72, 73, 74, 75, 76
# One default run of both dtypes should hold the GPU for about a second.
# Measured on MI355X at 8192 x 8192 x 8192 on the default grid (512
# workgroups) in windows of 1.7 to 2.2 s (profiles/gemmcheck_mi355x.json):
# 2.078 ms per round in bf16 (530 TFLOP/s) and 0.879 ms in i8 (1252 TOP/s),
# 2.957 ms for both, so 1 s is 338 rounds; 340 take 1.005 s.  (Windows of
# 16 rounds run at 911 TFLOP/s and 1689 TOP/s: the rate falls under
# sustained load.  torch.matmul takes 0.607 ms on the bf16 operands.)
DEFAULT_ROUNDS = 340


# -- numpy definition ----------------------------------------------------------

def _check_dtype(dtype: str, allowed: Tuple[str, ...] = DTYPES) -> str:
    if dtype not in allowed:
        raise ValueError(f"gemmcheck: dtype must be one of {allowed}, got {dtype!r}")
    return dtype


def _check_k(dtype: str, k: int) -> int:
    k = int(k)
    if k < 1 or k % SLAB[dtype] or k > MAX_K[dtype]:
        raise ValueError(f"gemmcheck: K must be a multiple of {SLAB[dtype]} in "
                         f"{SLAB[dtype]}..{MAX_K[dtype]} for {dtype}, got {k}")
    return k


def operand_block(seed: int, dtype: str, k: int):
    """The 256 x k blocks (A, Bt) the operands repeat, as int8 values."""
    import numpy as np

    _check_dtype(dtype)
    seed, k = int(seed) & 0xFFFFFFFF, _check_k(dtype, k)
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


def e4m3_of_int(v):
    """The e4m3 codes (uint8) of integers -16..16, all exactly representable."""
    import numpy as np

    mag = np.abs(np.asarray(v, dtype=np.int64))
    e = np.floor(np.log2(np.maximum(mag, 1))).astype(np.int64)
    code = ((e + 7) << 3) | ((mag << 3 >> e) & 7)  # mag >= 1 is normal in e4m3
    return (np.where(mag == 0, 0, code) | np.where(np.asarray(v) < 0, 0x80, 0)).astype(np.uint8)


def mx_formats(dtype: str) -> Tuple[str, str]:
    """An MX stage's element formats (A's, Bt's), of e4m3, e5m2, e2m3, e3m2
    and e2m1: "mxfp8:mxfp4" -> ("e4m3", "e2m1")."""
    names = _check_dtype(dtype, _MX_STAGES).split(":")
    return _ELEMENT[names[0]], _ELEMENT[names[-1]]


def _element(fmt: str) -> str:
    """An element format's name, given as such or as a one-format stage."""
    fmt = _ELEMENT.get(fmt, fmt)
    if fmt not in _ELEMENT_BITS:
        raise ValueError(f"gemmcheck: no element format {fmt!r}")
    return fmt


def _val(fmt: str, w):
    """val(): the element codes (uint8) made of words w; module docstring."""
    import numpy as np

    w = w & np.uint32(0xFF)
    if fmt == "e4m3":
        return e4m3_of_int(((w & 31) ^ 16).astype(np.int64) - 16)
    if fmt == "e2m1":
        return (w & 15).astype(np.uint8)
    if fmt == "e2m3":
        return np.where((w >> 3) & 3 == 3, w & 0x27, w & 0x3F).astype(np.uint8)
    f = (w >> 2) & 3
    sign, keep, bias = (0x80, 0x83, 15) if fmt == "e5m2" else (0x20, 0x23, 3)
    return np.where(f == 3, w & sign, (w & keep) | ((bias + f) << 2)).astype(np.uint8)


def mx_operand_block(seed: int, dtype: str, k: int):
    """The 256-row blocks the MX operands repeat, as uint8: (A codes [256, k],
    SA [256, k // 32], Bt codes [256, k], SB [256, k // 32]); one element
    code per entry, fp8 bytes, fp6 codes or e2m1 nibbles (``mx_pack`` packs
    them)."""
    import numpy as np

    formats = mx_formats(dtype)
    seed, k = int(seed) & 0xFFFFFFFF, _check_k(dtype, k)
    rows = np.arange(PERIOD, dtype=np.uint32)
    idx = np.arange(k, dtype=np.uint32)
    blocks = np.arange(k // MX_BLOCK, dtype=np.uint32)
    zero = np.zeros(1, dtype=np.uint32)
    with np.errstate(over="ignore"):
        codes = []
        for stage, fmt in zip((_STAGE_MX_A, _STAGE_MX_BT), formats):
            codes.append(_val(fmt, _fmix32(_base(seed, stage, rows)[:, None] + idx[None, :])))
        ra, cb = ((((_fmix32(_base(seed, stage, zero) + rows) & np.uint32(15)) ^ np.uint32(8))
                   .astype(np.int64) - 8) for stage in (_STAGE_RA, _STAGE_CB))
        t = (_fmix32(_base(seed, _STAGE_T, zero) + blocks) % np.uint32(17)).astype(np.int64) - 8
    sa = (127 + ra[:, None] + t[None, :]).astype(np.uint8)
    sb = (127 + cb[:, None] - t[None, :]).astype(np.uint8)
    return codes[0], sa, codes[1], sb


def mx_pack(fmt: str, codes):
    """Element codes [rows, k] of one operand as the kernel reads them.
    ``fmt`` is its element format (or a one-format stage): fp8 bytes as they
    are; e2m1 nibbles two per byte with element 2b the low nibble of byte b;
    fp6 codes 24 bytes per 32 elements, element e of a block bits 6e..6e+5
    of that 192-bit little-endian integer."""
    import numpy as np

    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    bits = _ELEMENT_BITS[_element(fmt)]
    if bits == 8:
        return codes
    if bits == 4:
        return codes[:, 0::2] | (codes[:, 1::2] << 4)
    each = np.unpackbits(codes[:, :, None], axis=2, bitorder="little")[:, :, :6]
    return np.packbits(each.reshape(codes.shape[0], -1), axis=1, bitorder="little")


def mx_dequantise(fmt: str, codes, scales):
    """The float64 values codes [rows, k] of element format ``fmt`` (or a
    one-format stage) and E8M0 scales [rows, k // 32] stand for (exact)."""
    import numpy as np

    from .matcheck import E2M3, E3M2
    from .mxcheck import E2M1, E4M3, E5M2

    table = np.array({"e4m3": E4M3, "e5m2": E5M2, "e2m3": E2M3, "e3m2": E3M2,
                      "e2m1": E2M1}[_element(fmt)])
    exp = np.repeat(np.asarray(scales).astype(np.int64), MX_BLOCK, axis=1) - 127
    return np.ldexp(table[np.asarray(codes)], exp)


def mx_operands(seed: int, dtype: str, m: int, n: int, k: int, device=None):
    """(A, SA, Bt, SB) on the GPU as uint8, packed for ``gemm_mx_nt``: the
    blocks of ``mx_operand_block`` uploaded once and repeated on the device."""
    import torch

    m, n = int(m), int(n)
    if m < TILE or n < TILE or m % TILE or n % TILE:
        raise ValueError(f"gemmcheck: M and N must be multiples of {TILE}, got {m} and {n}")
    device = _device(device)
    a, sa, bt, sb = mx_operand_block(seed, dtype, k)
    fa, fb = mx_formats(dtype)
    out = []
    for block, rows in ((mx_pack(fa, a), m), (sa, m), (mx_pack(fb, bt), n), (sb, n)):
        t = torch.from_numpy(block).to(device)
        out.append(t.repeat(-(-rows // PERIOD), 1)[:rows].contiguous())
    return tuple(out)


def tile_bits(dtype: str, c):
    """bits() of exact values c[...] as uint32."""
    import numpy as np

    c = np.asarray(c)
    if _check_dtype(dtype, _STAGES) == "i8":
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

    if dtype in _MX_STAGES:
        a, sa, bt, sb = mx_operand_block(seed, dtype, k)
        fa, fb = mx_formats(dtype)
        a, bt = mx_dequantise(fa, a, sa), mx_dequantise(fb, bt, sb)
    else:
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
    rec = _digest.decode_record(raw, _STAGES)
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
    ``reference_expected``.  ``dtypes`` may name any of ``DTYPES``,
    ``MX_DTYPES`` and ``MX_EXT_DTYPES``; the default is ``DTYPES``.

    The operands are taken from free VRAM: 2 (m + n) k bytes at most (bf16;
    every MX stage is at most a byte per element and one per 32 of scale); where
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
            stage = _STAGES.index(_check_dtype(dtype, _STAGES))
            table = reference_expected(seed, dtype, k)
            expected = _digest.expected_tensor("gemmcheck", table, 4, range(4), device)
            inject = None
            if _inject is not None and _inject[0] == dtype:
                inject = (int(_inject[1]), int(_inject[2]), stage, int(_inject[3]))
            if dtype in _MX_STAGES:
                ops = mx_operands(seed, dtype, m, n, k, device)
                raw = ext.gemmcheck_mx_run(*ops, dtype, expected, rounds, blocks,
                                           int(max_records), inject)
            else:
                ops = operands(seed, dtype, m, n, k, device)
                raw = ext.gemmcheck_run(*ops, expected, rounds, blocks, int(max_records), inject)
            del ops
            count, first, _mask, records, waves_on, elapsed = raw
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


def gemm_mx_nt(a, a_scale, bt, bt_scale, format: str, blocks: int = 0):
    """The block-scaled NT GEMM on the GPU of the operands, float32 [M, N]:
    ``sum_k a[i][k] 2**(a_scale[i][k // 32] - 127) bt[j][k] 2**(bt_scale[j][k // 32] - 127)``.
    ``format`` "mxfp8": ``a [M, K]``, ``bt [N, K]`` hold e4m3 codes (uint8 or
    float8_e4m3fn), K a multiple of 128, at most 32768.  "mxfp4": ``a [M, K / 2]``,
    ``bt [N, K / 2]`` uint8 hold two e2m1 codes per byte, the low nibble
    first, K a multiple of 256, at most 65536.  "mxfp8_e5m2": e5m2 codes
    (uint8 or float8_e5m2) ``[M, K]``, ``[N, K]``; "mxfp6_e2m3" and
    "mxfp6_e3m2": ``a [M, 3 K / 4]``, ``bt [N, 3 K / 4]`` uint8, 24 bytes per
    32 elements, element e of a block bits 6e..6e+5 of that little-endian
    integer; "mxfp8_e5m2:mxfp8": e5m2 ``a`` and e4m3 ``bt``, both ``[.., K]``;
    for these four K is a multiple of 128 (MAX_K at most).  The scales are uint8 E8M0,
    ``[M, K / 32]`` and ``[N, K / 32]``; M and N multiples of 128.  Exact
    whenever every partial sum is representable in float32.  ``blocks``
    workgroups walk the tiles (0 = two per CU)."""
    import torch

    with torch.cuda.device(a.device):
        return _active._ext().gemm_mx_nt(a, a_scale, bt, bt_scale, str(format), int(blocks))


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
    def add_arguments(ap):
        ap.add_argument("--dtypes", default=",".join(DTYPES), metavar="NAMES",
                        help="comma-separated stages to run, of " + ", ".join(_STAGES))

    return _active.probe_main(
        "gemmcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: gemmcheck(seed=args.seed, rounds=args.rounds,
                               dtypes=tuple(args.dtypes.split(","))), argv, add_arguments)


if __name__ == "__main__":
    sys.exit(main())
