"""Active matrix-core probe for the 16x16 shapes, the MXFP8 / MXFP6 /
mixed-width formats and 2:4 structured sparsity — wrapper over the
matcheck HIP kernel.

``cucheck`` and ``mxcheck`` reach the matrix cores through six
instructions, all but one of them 32x32, with fp8 operands of four
exponents and E8M0 scales 2**0 .. 2**3 in byte 0 of the scale register.
This probe is their twin for the rest: the 16x16 shapes with their own
operand routing and C/D register map, format fields 0..3 of the scaled
instruction (e4m3, e5m2, e2m3, e3m2, the 192-bit packing of 32 six-bit
codes, mixed products), zero / subnormal / Inf / NaN elements, scales
over 23..230 read from every byte of the scale register, and the
``v_smfmac_*`` instructions with their index path.  ``matcheck()``
launches one 16-wave workgroup per compute unit; every wave runs the same
deterministic workload and compares four 32-bit digests per round with
``reference_digests``, computed here in numpy.  Launch shape, accounting
and the mismatch log are cucheck's.

The workload (csrc/matcheck.hip; ``reference_digests`` is the
definition).  Arithmetic is mod 2**32; ``fmix32``, ``base``, ``salt`` are
cucheck's; form f of stage s draws

  word(s, f, r, idx) = fmix32(base(seed, 60 + s, r) + 4096 f + idx)
  sext(x, n)         = the low n bits of x as a two's-complement integer
  bits(c)            = the f32 bit pattern of c; any zero as 0, any NaN as
                       0x7FC00000; an i32 tile's values as they are
  fold(C)            = sum over i, j of fmix32(bits(C[i][j]) + salt(n i + j))
                       for an n x n tile

and a stage's digest is the wrapping sum of fold over its forms.  Every
operand is chosen so that all partial sums of every dot product are
exactly representable in the accumulator: an element of C is 2**e(i, j)
(``tile_unit``) times an integer below 2**24 whatever order the hardware
sums in, so the reference multiplies decode tables in float64 and
converts to float32 without rounding.  K = 128 everywhere.

  0 shape16  16x16 tiles, C = C0 + A.B, C0[i][j] = sext(word(2048 + 16i + j), 16)
       i8    A[i][k] = signed byte k%4 of word(32i + k/4), B[k][j] the same
             of word(1024 + 32j + k/4); mfma_i32_16x16x64_i8, two issues
       bf16  the same bytes as bf16; mfma_f32_16x16x32_bf16, four issues
       f16   A[i][k] = sext(word(64i + k/2) >> 16(k%2), 11), B[k][j] =
             sext(word(1024 + 64j + k/2) >> 16(k%2), 5);
             mfma_f32_16x16x32_f16, four issues
  1 mxfp8    one scaled form per round: mfma_scale_f32_16x16x128_f8f6f4
             (16x16 tile, one issue) in even rounds, ..._32x32x64_f8f6f4
             (32x32 tile, two issues) in odd ones; (A, B) = (e4m3, e5m2)
             where (r >> 1) & 1 is 0, else (e5m2, e4m3).  Element k of row
             i of A is byte k%4 x of word(32i + k/4), of column j of B of
             word(1024 + 32j + k/4), sign and mantissa kept and the
             exponent field forced:
               e4m3: r % 13 + ((x >> 3) & 3), S.1111.111 (NaN) -> mantissa 6
               e5m2: r % 28 + ((x >> 2) & 3)
             so zero, every subnormal and, across rounds, every finite
             code is fed.  Block b = k/32 is scaled by the E8M0 bytes
               SA[i][b] = 127 + ra[i] + t[b],  SB[j][b] = 127 + cb[j] - t[b]
               ra[i] = sext(word(2048 + i), 4), cb[j] = sext(word(2080 + j), 4)
               t[b]  = word(2112 + b) % 193 - 96
             each in 23..230, while every block of a dot product carries
             2**(ra[i] + cb[j]).  The lane's scale register holds that
             byte in byte r & 3 (op_sel) and three different decoys
             elsewhere.  Rounds with r % 8 == 7 are special, placed by
             sp = word(2120) and n = the tile's side: row nl = sp % n of A
             gets the NaN code 0x7F at k = (sp >> 8) % 128; line il =
             (nl + 5) % n of the e5m2 operand gets +-Inf (sign sp >> 31) at
             k = (sp >> 16) % 128; SA[(nl + 10) % n][(sp >> 24) % 4] = 0xFF,
             the E8M0 NaN.  r % 8 == 7 implies that A is the e5m2 operand,
             so the Inf sits in a row of A, and that row of C is +-Inf, or
             NaN where it meets a zero of B.  The reference follows IEEE.
  2 mxfp6    three scaled forms per round, shapes, scales (t = word % 129 -
             64) and op_sel as in stage 1:
               e2m3_e3m2, e3m2_e2m3  32 six-bit codes little-endian in the
                         first six of a block's eight words: all 64 codes
                         of both formats, straight from random bits
               e3m2_e2m1  mixed register counts: e2m1 from the nibbles of
                         the first four words of a block
  3 sparse   16x16 tiles, 2:4 sparse A by dense B.  Group g = k/4 of row i
             keeps two elements, from bits 0 and 16 on of word(32i + g), at
             positions PAIRS[word(512 + 32i + g) % 6] of the group; the
             rest of the dense A is zero.
               f16      kept sext(.., 11); B[k][j] = sext(word(1024 + 64j +
                        k/2) >> 16(k%2), 5); smfmac_f32_16x16x64_f16, two
                        issues
               bf16     kept signed bytes; B[k][j] = signed byte 2(k%2) of
                        word(1024 + 64j + k/2); smfmac_f32_16x16x64_bf16
               i8       kept signed bytes; B[k][j] = signed byte k%4 of
                        word(1024 + 32j + k/4); smfmac_i32_16x16x128_i8
               fp8_bf8  the same bytes as mxcheck's four-exponent e4m3
                        (fields 7..10) and e5m2 (fields 15..18);
                        smfmac_f32_16x16x128_fp8_bf8
             The 16-bit forms read their 16 index bits from half r & 1 of
             the index register (abid); the other half holds decoys.

How the kernel feeds the instructions (proved element by element by the
GPU test of ``wave_tile`` against ``matmul_tile``):
f32 / i32 16x16 C/D: lane l, register g holds row 4(l>>4) + g, column
l&15.  Dense 16x16 A and B: lane l holds row / column l&15 and the
(l>>4)-th quarter of the issue's k range; C = A.B does not change under a
permutation of k applied to both.  16x16x128 scaled: that quarter is one
32-element block and the lane's selected scale byte scales it; 32x32x64
scaled as in mxcheck.  Sparse: A's lane holds the (l>>4)-th quarter of
the issue's k, groups of four k in register order, and the index is two
bits per kept element, low group first; B's eight registers are two
halves of four, the first holding the (l>>4)-th quarter of the first half
of the issue's k range and the second that of the second half (observed
on an MI355X: with B contiguous like A every element of all four forms
was wrong, with this map every element agrees).  All special classes of
stage 1 (NaN element, +-Inf, Inf x 0, E8M0 NaN) follow IEEE on the
hardware, and scales 23..230 stay exact: nothing was narrowed.

Not covered: the e2m1 x e4m3 form of stage 2 (A in four registers, B
in eight).  On an MI355X its tile disagreed with the exact product in
every element in every round tried, by about a tenth of the sum of
|a b| with the lane map above and by more with B's or A's registers
taken as two halves of the k range; no map was found, so the form is
left out rather than compared loosely.  e3m2 x e2m1 keeps a mixed
register count in the stage.  Also not covered: rounding
(``probe/fpcheck.py``), the 32x32 dense forms (``cucheck``,
``mxcheck``), e2m1 x e2m1 (``mxcheck``), the 4x4 and xf32 forms, the
32x32 sparse shapes, cbsz / blgp broadcasts.  The 16x16 scaled
shape only sees op_sel 0 and 2 and the 32x32 one 1 and 3, special rounds
are always 32x32 with op_sel 3: all three follow the parity of r.
30.1 us per round on the default grid (see DEFAULT_ROUNDS below).

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.matcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

from . import _active, _digest
from ._digest import _base, _device, _fmix32, _salt
from .mxcheck import E2M1, E4M3, E5M2, _fields, _nibbles

STAGES: Tuple[str, ...] = ("shape16", "mxfp8", "mxfp6", "sparse")
FORMS: Tuple[Tuple[str, ...], ...] = (
    ("i8", "bf16", "f16"),
    ("fp8",),
    ("e2m3_e3m2", "e3m2_e2m3", "e3m2_e2m1"),
    ("f16", "bf16", "i8", "fp8_bf8"),
)
_STAGE0 = 60  # stage number fed to base() is _STAGE0 + s
_FORM_WORDS = 4096
# positions (i0, i1) of the two kept elements of a group of four k
PAIRS: Tuple[Tuple[int, int], ...] = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# format fields of the scaled instruction
FMT_E4M3, FMT_E5M2, FMT_E2M3, FMT_E3M2, FMT_E2M1 = range(5)
# (A, B) formats of stage 2's forms
_MXFP6_FORMATS = ((FMT_E2M3, FMT_E3M2), (FMT_E3M2, FMT_E2M3), (FMT_E3M2, FMT_E2M1))
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/matcheck_mi355x.json): 30.81, 30.30 and
# 30.08 us per round at 1024, 2048 and 4096 rounds with the default grid
# (256 workgroups, 4096 waves), so 0.5 s are 16.2 x 1024 rounds; 16 x 1024
# take 0.49 s.  Operand generation sets the time, not the matrix cores.
# The numpy table costs 0.38 ms of host time per round, 6.2 s for these.
DEFAULT_ROUNDS = 16384

# dense-equivalent flops one wave spends in the matrix cores per round, per
# stage (the scaled stages alternate between a 16x16 and a 32x32 tile)
_TILE_FLOPS = 2 * 16 * 16 * 128
_FLOPS_PER_WAVE_ROUND = (3 * _TILE_FLOPS, 5 * _TILE_FLOPS // 2,
                         3 * 5 * _TILE_FLOPS // 2, 4 * _TILE_FLOPS)
_REF_CHUNK = 128  # rounds per numpy batch


# -- decode tables ---------------------------------------------------------------

def _fp6_table(exp_bits: int, man_bits: int, bias: int) -> Tuple[float, ...]:
    """All 64 codes of an OCP six-bit float (no Inf, no NaN), built the
    way ``mxcheck._fp8_table`` builds its tables."""
    out = []
    for code in range(64):
        sign = -1.0 if code & 0x20 else 1.0
        e = (code >> man_bits) & ((1 << exp_bits) - 1)
        m = code & ((1 << man_bits) - 1)
        if e == 0:
            v = m * 2.0 ** (1 - bias - man_bits)
        else:
            v = ((1 << man_bits) + m) * 2.0 ** (e - bias - man_bits)
        out.append(sign * v)
    return tuple(out)


E2M3: Tuple[float, ...] = _fp6_table(2, 3, 1)  # OCP e2m3: code -> value, up to 7.5
E3M2: Tuple[float, ...] = _fp6_table(3, 2, 3)  # OCP e3m2, up to 28
_TABLES = (E4M3, E5M2, E2M3, E3M2, E2M1)


def e4m3_code(x, f0):
    """The e4m3 code made of a raw byte: sign and mantissa kept, exponent
    field f0 + two bits; the NaN code S.1111.111 gets mantissa 6."""
    c = (x & 0x87) | ((f0 + ((x >> 3) & 3)) << 3)
    return c & ~((c & 0x7F) == 0x7F).astype(c.dtype)


def e5m2_code(x, f0):
    """The e5m2 code made of a raw byte."""
    return (x & 0x83) | ((f0 + ((x >> 2) & 3)) << 2)


def op_sel(r: int) -> int:
    """The byte of the scale register that holds the real scale."""
    return int(r) & 3


def tile_dim(stage: int, r: int) -> int:
    """Side of the tile a form of ``stage`` computes in round ``r``."""
    return 32 if stage in (1, 2) and int(r) & 1 else 16


# -- numpy definition ----------------------------------------------------------

def _words(seed: int, stage: int, form: int, r, first: int, count: int):
    """word(stage, form, r, first .. first+count-1) as uint32[len(r), count]."""
    import numpy as np

    idx = np.arange(first, first + count, dtype=np.uint32) + np.uint32(_FORM_WORDS * form)
    with np.errstate(over="ignore"):
        return _fmix32(_base(seed, _STAGE0 + stage, r)[:, None] + idx[None, :])


def _sext(x, bits: int):
    import numpy as np

    x = x.astype(np.int64) & ((1 << bits) - 1)
    return (x ^ (1 << (bits - 1))) - (1 << (bits - 1))


def _halves(words, bits: int):
    """uint32[n, m] -> int64[n, 2m]: sext of both 16-bit halves, low first."""
    return _sext(_fields(words, "<u2"), bits)


def _block_codes(fmt: int, words, r):
    """uint32[n, rows, 4, 8] (a block's eight words) -> the 32 element
    codes of every block, int64[n, rows, 4, 32]."""
    import numpy as np

    n, rows = words.shape[:2]
    if fmt in (FMT_E4M3, FMT_E5M2):
        x = _fields(words.reshape(n, -1), np.uint8).astype(np.int64).reshape(n, rows, 4, 32)
        if fmt == FMT_E4M3:
            return e4m3_code(x, (r.astype(np.int64) % 13)[:, None, None, None])
        return e5m2_code(x, (r.astype(np.int64) % 28)[:, None, None, None])
    if fmt == FMT_E2M1:
        w = np.ascontiguousarray(words[..., :4]).reshape(n, -1)
        return _nibbles(w).astype(np.int64).reshape(n, rows, 4, 32)
    # 32 six-bit codes, little-endian, in the first six words
    b = _fields(np.ascontiguousarray(words[..., :6]).reshape(n, -1), np.uint8)
    bits = np.unpackbits(b, axis=-1, bitorder="little").reshape(n, rows, 4, 32, 6)
    return (bits.astype(np.int64) << np.arange(6)).sum(axis=-1)


def _scaled_formats(stage: int, form: int, r) -> Tuple[int, int]:
    if stage == 2:
        return _MXFP6_FORMATS[form]
    return (FMT_E5M2, FMT_E4M3) if (int(r[0]) >> 1) & 1 else (FMT_E4M3, FMT_E5M2)


def codes(seed: int, stage: int, form: int, r):
    """What a scaled form (stages 1, 2) feeds in rounds ``r`` (uint32
    array, all with the same r & 3, which fixes shape and formats):
    (fmt_a, fmt_b, A codes, B codes, SA, SB) with codes as int64[len(r), n,
    4, 32] (row / column, block, element) and the E8M0 bytes as
    int64[len(r), n, 4].  Special rounds of stage 1 are patched in."""
    import numpy as np

    if stage not in (1, 2) or not 0 <= form < len(FORMS[stage]):
        raise ValueError(f"codes: no scaled form {form} in stage {stage}")
    r = np.asarray(r, dtype=np.uint32)
    if len(set((r & 3).tolist())) != 1:
        raise ValueError("codes: rounds must share r & 3")
    seed = int(seed) & 0xFFFFFFFF
    m, n = len(r), tile_dim(stage, r[0])
    fa, fb = _scaled_formats(stage, form, r)
    ca = _block_codes(fa, _words(seed, stage, form, r, 0, 32 * n).reshape(m, n, 4, 8), r)
    cb = _block_codes(fb, _words(seed, stage, form, r, 1024, 32 * n).reshape(m, n, 4, 8), r)
    trange = 96 if stage == 1 else 64
    ra = _sext(_words(seed, stage, form, r, 2048, n), 4)
    cbs = _sext(_words(seed, stage, form, r, 2080, n), 4)
    t = (_words(seed, stage, form, r, 2112, 4) % np.uint32(2 * trange + 1)).astype(np.int64) - trange
    sa = 127 + ra[:, :, None] + t[:, None, :]
    sb = 127 + cbs[:, :, None] - t[:, None, :]
    if stage == 1:
        sp = _words(seed, stage, form, r, 2120, 1)[:, 0].astype(np.int64)
        for q in np.flatnonzero((r & 7) == 7):
            w = int(sp[q])
            nl, nk, ik = w % n, (w >> 8) % 128, (w >> 16) % 128
            ca[q, nl, nk // 32, nk % 32] = 0x7F
            inf_op = ca if fa == FMT_E5M2 else cb
            inf_op[q, (nl + 5) % n, ik // 32, ik % 32] = 0x7C | ((w >> 31) << 7)
            sa[q, (nl + 10) % n, (w >> 24) % 4] = 0xFF
    return fa, fb, ca, cb, sa, sb


def sparse_pairs(seed: int, form: int, r):
    """Index p into PAIRS of every group of stage 3: int64[len(r), 16, 32]."""
    import numpy as np

    r = np.asarray(r, dtype=np.uint32)
    w = _words(int(seed) & 0xFFFFFFFF, 3, form, r, 512, 512)
    return (w % np.uint32(6)).astype(np.int64).reshape(len(r), 16, 32)


def _fp8_values(fmt: int, code_fn, f0: int, x):
    import numpy as np

    return np.array(_TABLES[fmt])[code_fn(x.astype(np.int64), f0)]


def operands(seed: int, stage: int, form: int, r):
    """(A, Bt, C0) of a form for rounds ``r`` (uint32 array; for stages 1
    and 2 all with the same r & 3) as float64 [len(r), n, 128], block
    scales multiplied in, sparse A expanded to dense; Bt[j][k] = B[k][j];
    C0 is the accumulator-in [len(r), n, n], or None."""
    import numpy as np

    r = np.asarray(r, dtype=np.uint32)
    seed = int(seed) & 0xFFFFFFFF
    m = len(r)
    if stage not in range(len(STAGES)) or not 0 <= form < len(FORMS[stage]):
        raise ValueError(f"operands: no form {form} in stage {stage}")

    def words(first, count):
        return _words(seed, stage, form, r, first, count)

    if stage == 0:
        c0 = _sext(words(2048, 256), 16).astype(np.float64).reshape(m, 16, 16)
        if form == 2:
            a, b = _halves(words(0, 1024), 11), _halves(words(1024, 1024), 5)
        else:
            a, b = _fields(words(0, 512), np.int8), _fields(words(1024, 512), np.int8)
        return (a.astype(np.float64).reshape(m, 16, 128),
                b.astype(np.float64).reshape(m, 16, 128), c0)
    if stage in (1, 2):
        fa, fb, ca, cb, sa, sb = codes(seed, stage, form, r)
        with np.errstate(invalid="ignore"):
            a = np.array(_TABLES[fa])[ca] * np.where(sa == 255, np.nan, 2.0 ** (sa - 127.0))[..., None]
            b = np.array(_TABLES[fb])[cb] * np.where(sb == 255, np.nan, 2.0 ** (sb - 127.0))[..., None]
        return a.reshape(m, -1, 128), b.reshape(m, -1, 128), None
    # stage 3: kept pairs [m, 16, 32, 2] scattered into the dense A
    aw = words(0, 512)
    if form == 0:
        kept = _halves(aw, 11).astype(np.float64)
        b = _halves(words(1024, 1024), 5).astype(np.float64)
    else:
        ab = _fields(aw, np.uint8)[:, 0::2]  # bytes 0 and 2 of every word
        if form == 1:
            kept = ab.view(np.int8).astype(np.float64)
            b = _fields(words(1024, 1024), np.int8)[:, 0::2].astype(np.float64)
        elif form == 2:
            kept = ab.view(np.int8).astype(np.float64)
            b = _fields(words(1024, 512), np.int8).astype(np.float64)
        else:
            kept = _fp8_values(FMT_E4M3, e4m3_code, 7, ab)
            b = _fp8_values(FMT_E5M2, e5m2_code, 15, _fields(words(1024, 512), np.uint8))
    kept = kept.reshape(m, 16, 32, 2)
    pos = np.array(PAIRS)[sparse_pairs(seed, form, r)]  # [m, 16, 32, 2]
    a = np.zeros((m, 16, 32, 4))
    np.put_along_axis(a, pos, kept, axis=-1)
    return a.reshape(m, 16, 128), b.reshape(m, 16, 128), None


def _is_int(stage: int, form: int) -> bool:
    return FORMS[stage][form] == "i8"


def _matmul(seed: int, stage: int, form: int, r):
    """Exact tiles float64[len(r), n, n].  Rounds that hold NaN or Inf
    go through einsum, which follows IEEE term by term."""
    import numpy as np

    a, bt, c0 = operands(seed, stage, form, r)
    with np.errstate(invalid="ignore"):
        c = np.matmul(a, bt.transpose(0, 2, 1))
    bad = ~(np.isfinite(a).all(axis=(1, 2)) & np.isfinite(bt).all(axis=(1, 2)))
    if bad.any():
        with np.errstate(invalid="ignore"):
            c[bad] = np.einsum("rik,rjk->rij", a[bad], bt[bad])
    return c if c0 is None else c + c0


def matmul_tile(seed: int, stage: int, form: int, r: int):
    """The exact product of one form for one round as float64 [n, n]
    (n = ``tile_dim``) — what the digest is folded from."""
    return _matmul(seed, stage, form, _digest.one_round("matcheck", r))[0]


def tile_unit(seed: int, stage: int, form: int, r: int):
    """2**e(i, j) as float64 [n, n]: every finite element of
    ``matmul_tile`` is this times an integer below 2**24."""
    import numpy as np

    n = tile_dim(stage, r)
    if stage in (0, 3):
        return np.full((n, n), 1 / 32 if FORMS[stage][form] == "fp8_bf8" else 1.0)
    rr = _digest.one_round("matcheck", r)
    fa, fb = _scaled_formats(stage, form, rr)
    units = (2.0 ** (max(int(r) % 13, 1) - 10), 2.0 ** (max(int(r) % 28, 1) - 17),
             1 / 8, 1 / 16, 1 / 2)
    seed = int(seed) & 0xFFFFFFFF
    ra = _sext(_words(seed, stage, form, rr, 2048, n), 4)[0]
    cb = _sext(_words(seed, stage, form, rr, 2080, n), 4)[0]
    return units[fa] * units[fb] * 2.0 ** (ra[:, None] + cb[None, :]).astype(np.float64)


def tile_bits(stage: int, form: int, tile):
    """bits() of a tile[..., n, n] of exact values, as uint32."""
    import numpy as np

    tile = np.asarray(tile, dtype=np.float64)
    if _is_int(stage, form):
        return tile.astype(np.int64).astype(np.uint32)
    with np.errstate(over="ignore", invalid="ignore"):
        b = tile.astype(np.float32).view(np.uint32).copy()
    b[tile == 0] = 0
    b[np.isnan(tile)] = 0x7FC00000
    return b


def fold_bits(bits):
    """fold() of uint32 bit patterns [..., n, n] (``tile_bits`` or
    ``wave_tile``) -> uint32[...]."""
    import numpy as np

    bits = np.asarray(bits, dtype=np.uint32)
    n = bits.shape[-1]
    flat = bits.reshape(bits.shape[:-2] + (n * n,))
    with np.errstate(over="ignore"):
        return _fmix32(flat + _salt(np.arange(n * n, dtype=np.uint32))).sum(
            axis=-1, dtype=np.uint32)


def fold_tile(stage: int, form: int, tile):
    """The uint32 digest share of a form's exact tile[..., n, n]."""
    return fold_bits(tile_bits(stage, form, tile))


def reference_digests(seed: int, rounds: int):
    """Expected digests as uint32[rounds, 4], columns in STAGES order.

    Pure numpy: needs neither torch nor a GPU.  This is the definition
    the GPU kernel is tested against."""
    import numpy as np

    seed = int(seed) & 0xFFFFFFFF
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("reference_digests: rounds >= 0 required")
    out = np.zeros((rounds, len(STAGES)), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, rounds, _REF_CHUNK):
            hi = min(lo + _REF_CHUNK, rounds)
            for s in range(len(STAGES)):
                # the scaled stages' shape and formats follow r & 3
                step = 4 if s in (1, 2) else 1
                for first in range(lo, min(lo + step, hi)):
                    r = np.arange(first, hi, step, dtype=np.uint32)
                    for f in range(len(FORMS[s])):
                        out[first:hi:step, s] += fold_tile(s, f, _matmul(seed, s, f, r))
    return out


# -- GPU run ---------------------------------------------------------------------

@dataclass
class MatcheckResult(_digest.DigestResult):
    # Whole-run lower bounds per stage in dense-equivalent flops (the
    # kernel's time also holds operand generation, the other stages and
    # the digests): informative.
    shape16_tflops: float = 0.0
    mxfp8_tflops: float = 0.0
    mxfp6_tflops: float = 0.0
    sparse_tflops: float = 0.0


def matcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> MatcheckResult:
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
        "matcheck", MatcheckResult(rounds=rounds), STAGES, _FLOPS_PER_WAVE_ROUND, 1e12,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected)


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``matcheck`` with its dump pointer set."""
    return _digest.wave_digests(
        "matcheck", _active._ext().matcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device)


def wave_tile(seed: int, stage: int, form: int, r: int, device=None):
    """bits() of the accumulator tile wave 0 of one workgroup computed for
    one form and round, as uint32 [n, n] like ``tile_bits`` of
    ``matmul_tile``.  A digest cannot say which element is wrong; this
    can."""
    import numpy as np
    import torch

    with torch.cuda.device(_device(device)):
        tile = _active._ext().matcheck_tile(int(seed), int(stage), int(form), int(r))
    return tile.cpu().numpy().view(np.uint32)


# -- child process -----------------------------------------------------------

def run_matcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                            timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the matcheck CLI."""
    return _active.run_probe_subprocess("matcheck", index, "--rounds", rounds, timeout_s)


def matcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                   rounds: int = DEFAULT_ROUNDS,
                   max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("matcheck", "mismatches", _digest.metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "matcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: matcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
