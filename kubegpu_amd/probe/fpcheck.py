"""Active IEEE-rounding probe for the vector FP units — wrapper over the
fpcheck HIP kernel.

``cucheck`` and ``mxcheck`` feed the floating-point hardware only
operands whose every intermediate is an exactly representable integer,
so neither the alignment shifter, the normaliser, the round-to-nearest-
even increment and sticky bit, subnormal handling, overflow and
underflow, the division and square-root sequences, ``v_fma_f64``, the
packed f16 / f32 pipes nor any conversion instruction is checked by
them.  This probe is their twin for exactly that logic.  IEEE 754
defines add, mul, fma, div, sqrt, round-to-integral and the conversions
bit for bit, so numpy is the exact reference here too and every compare
is bit-exact.  ``fpcheck()`` launches one 16-wave workgroup per compute
unit; every wave runs the same deterministic workload and compares four
32-bit digests per round with ``reference_digests``.  Launch shape,
accounting and the mismatch log (XCD, shader engine, shader array, CU,
SIMD of the wave that disagreed) are cucheck's.

The workload (csrc/fpcheck.hip; ``reference_values`` and
``reference_digests`` are the definition).  Integer arithmetic is mod
2**32 (2**64 where a 64-bit pattern is built); ``fmix32``, ``base``,
``salt`` are cucheck's and the stage number fed to ``base`` is 8 + s,
so the inputs differ from cucheck's and mxcheck's.  Inputs repeat with
PERIOD = 256 rounds:

  word(s, r, idx) = fmix32(base(seed, 8 + s, r % PERIOD) + idx)

A *slot* is q = 64 j + lane, j = 0 .. slots-per-lane - 1; slot q owns
words 16 q .. 16 q + 15.  An operand triple (a, b, c) of element e
(0, or 1 for the second half of a packed pair) is made from

  ra = word 8e + 0 (| word 8e + 1 << 32 for f64), rb = words 8e + 2, 3,
  rc = words 8e + 4, 5, sel = word 8e + 6; f16 takes the low 16 bits

by recipe (lane + j + r + 3 e) mod 8, with integer operations only.
pack(s, e, m) is sign, biased exponent field, mantissa field; S, E, M
take them apart; B is the bias, Mb the mantissa width, X the all-ones
exponent field; v = sel & 3, t = ((sel >> 2) & 255) % 3,
p = (sel >> 10) & 7, cm = (sel >> 13) & 3, and mid(x) =
pack(S x, B - 8 + (E x & 15), M x):

  0 raw      a, b, c = ra, rb, rc
  1 mid      a, b, c = mid(ra), mid(rb), mid(rc): plain inexact rounding
  2 ties     half(s, e, t) = pack(s, e - Mb - 1, 0), pack(s, e - Mb - 1, 1)
             or pack(s, e - Mb - 2, all ones) for t = 0, 1, 2: half an ulp
             of a number with exponent field e, and one step either side
             v = 0, 3: a = pack(S ra, B + (E ra & 7), M ra),
                       b = half(S rb, E a, t), c = mid(rc)       (add)
             v = 1:    a, b keep only their top h = (Mb - 1) // 2 mantissa
                       bits at exponents B + (E & 7), so a * b is exact;
                       c = half(S rc, exponent field of a * b, t)  (fma)
             v = 2:    a, b have odd significands of (Mb + 2) // 2 and
                       Mb + 2 - that many bits (b one more for t != 0) at
                       exponents B - 4 + (E & 7): the product has Mb + 1
                       or Mb + 2 bits and is odd, so about half are exact
                       ties; c = mid(rc)                           (mul)
  3 cancel   v even:   a = mid(ra), b = a ^ sign ^ p, c = mid(rc)  (add)
             v odd:    a = pack(S ra, B - 4 + (E ra & 7), M ra), b the same
                       with only its top 10 mantissa bits (the product
                       fits 64 bits in every format), c = minus the top
                       Mb + 1 bits of the exact product (truncated),
                       ^ (p & 3): the fma returns the bits the multiply
                       alone would round away                      (fma)
  4 subnorm  a = pack(S ra, 0 if v & 1 else 1 + (E ra & 3), M ra)
             b = pack(S rb, 0 if v & 2 else B - 2 + (E rb & 3), M rb)
             c = pack(S rc, 0 if cm & 1 else 1 + (E rc & 3), M rc)
  5 overflow a, c at exponent X - 1 - (E & 1); b at that too (v = 0, 3),
             at B + (E rb & 3) (v = 1) or at B - 1 - (E rb & 3) (v = 2)
  6 underfl. a at exponent 1 + (E ra & 7); b at B - Mb - 4 + (E rb & 7),
             B - (E rb & 7), B + 1 + (E rb & 7), B + Mb - 2 + (E rb & 7)
             for v = 0 .. 3 (products, then quotients, in the upper and
             the lowest part of the subnormal range and below it);
             c = +-0, a subnormal, or exponent 1 + (E rc & 3) for
             cm = 0, 1, 2-3
  7 special  each of a, b, c by its own 3-bit code from sel >> 16, 19, 22:
             0, 5 zero; 1, 6 Inf; 2 NaN; 3 one; 4, 7 mid(x); sign kept

  0 f32     8 slots per lane; add a + b, mul a * b, fma(a, b, c),
            div a / b, sqrt |a|
  1 f64     4 slots per lane, the same five.  The fma alone takes
            operands whose exponent is more than 200 from B remapped to
            B - 64 + (E & 127), so the reference's splitting neither
            overflows nor underflows; the f64 special classes go through
            add, mul, div and sqrt.
  2 packed  8 slots per lane, two triples each (e = 0, 1): pk_fma_f16,
            pk_mul_f16, pk_add_f16 on 2-element f16 vectors (result word =
            lo | hi << 16), pk_fma_f32, pk_mul_f32, pk_add_f32 on
            2-element f32 vectors (.x and .y are separate results)
  3 cvt     8 slots per lane; x (f32) from word 0, d (f64) from words
            2, 3, u (u32) from word 4, sel word 6, by the same recipe
            number (``_cvt_operands`` is the definition: operands at the
            edges of the target format, exact halves in the bits that the
            conversion drops, x.5 values, subnormals, values about the
            largest finite f16 / bf16 / f32, specials).  f32_f16 (RNE),
            f32_bf16 (RNE), f64_f32 (RNE), u32_f32, i32_f32 (RNE), f32_i32
            (truncating; an x with |x| >= 2**31, Inf or NaN is first
            remapped to exponent 23 + (E & 7), the C cast is undefined
            there), rint, floor, ceil, trunc on f32.

Digest of a stage: with results numbered n = 64 * slots-per-lane * k + q
for operation k in OPS order, sum of fmix32(bits + salt(n)), and for
f64 results sum of fmix32(lo ^ fmix32(hi + salt(n))).  Any NaN is first
replaced by the canonical quiet NaN (0x7FC00000, 0x7E00, 0x7FC0,
0x7FF8000000000000); signed zeros are kept.

Ties: a quotient can be an exact tie only in the subnormal range and a
square root never, so recipe 2 builds none for them; f16 addends carry
11 significant bits, so the sum of two cannot cancel by 20 binary
orders unless it is zero (the f16 fma can: its product has 22 bits).

Not covered: standalone v_exp, v_log, v_sin and v_cos — IEEE does not
define their results, so no independent exact reference exists; their
unit is reached only through the v_rcp, v_rsq and v_sqrt seeds inside
division and square root.  fp8 conversions.  Rounding modes other than
nearest-even.  Atomic operations, float ones included: they execute in
units of their own, which are ``probe/atomcheck.py``'s ground.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.fpcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

from . import _active
from . import _digest as _shared  # _digest is this module's own fold
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

STAGES: Tuple[str, ...] = ("f32", "f64", "packed", "cvt")
PERIOD = 256  # inputs of round r are those of round r % PERIOD
SLOTS_PER_LANE: Tuple[int, ...] = (8, 4, 8, 8)
WORDS_PER_SLOT = 16
_STAGE0 = 8  # stage number fed to base() is _STAGE0 + s
OPS: Tuple[Tuple[str, ...], ...] = (
    ("add", "mul", "fma", "div", "sqrt"),
    ("add", "mul", "fma", "div", "sqrt"),
    ("pk_fma_f16", "pk_mul_f16", "pk_add_f16", "pk_fma_f32.x", "pk_fma_f32.y",
     "pk_mul_f32.x", "pk_mul_f32.y", "pk_add_f32.x", "pk_add_f32.y"),
    ("f32_f16", "f32_bf16", "f64_f32", "u32_f32", "i32_f32", "f32_i32",
     "rint", "floor", "ceil", "trunc"),
)
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/fpcheck_mi355x.json): 155.5 us per round
# with the default grid (256 workgroups, 4096 waves), flat from 256 to
# 8192 rounds (155.3 .. 156.0), so 0.5 s are 3215 rounds; 3 x 1024 = 12
# periods take 0.48 s.  The numpy table costs 0.21 s of host time
# whatever the rounds, since only PERIOD rows are computed.
DEFAULT_ROUNDS = 3072

# floating-point results one wave produces per round, per stage
_OPS_PER_WAVE_ROUND = (64 * 8 * 5, 64 * 4 * 5, 64 * 8 * 12, 64 * 8 * 10)


# -- formats ---------------------------------------------------------------------

@dataclass(frozen=True)
class _Fmt:
    name: str
    ebits: int
    mbits: int

    @property
    def width(self) -> int:
        return 1 + self.ebits + self.mbits

    @property
    def bias(self) -> int:
        return (1 << (self.ebits - 1)) - 1

    @property
    def emask(self) -> int:
        return (1 << self.ebits) - 1

    @property
    def mmask(self) -> int:
        return (1 << self.mbits) - 1

    @property
    def canonical_nan(self) -> int:
        return (self.emask << self.mbits) | (1 << (self.mbits - 1))


F16 = _Fmt("f16", 5, 10)
F32 = _Fmt("f32", 8, 23)
F64 = _Fmt("f64", 11, 52)
BF16_CANONICAL_NAN = 0x7FC0


def _np_types(fmt: _Fmt):
    import numpy as np

    return {"f16": (np.uint16, np.float16), "f32": (np.uint32, np.float32),
            "f64": (np.uint64, np.float64)}[fmt.name]


def _as_float(bits, fmt: _Fmt):
    """uint64 bit patterns -> float array of the format."""
    it, ft = _np_types(fmt)
    return bits.astype(it).view(ft)


def _as_bits(x, fmt: _Fmt):
    """float array -> uint64 bit patterns, NaN canonical."""
    import numpy as np

    it, _ = _np_types(fmt)
    bits = np.ascontiguousarray(x).view(it).astype(np.uint64)
    return np.where(np.isnan(x), np.uint64(fmt.canonical_nan), bits)


# -- operand recipes (integer operations only) ---------------------------------------

def _u(x):
    import numpy as np

    return np.uint64(x)


class _Fields:
    """pack / S / E / M of a format on uint64 arrays."""

    def __init__(self, fmt: _Fmt):
        self.f = fmt
        self.Mb, self.B, self.X = fmt.mbits, fmt.bias, fmt.emask
        self.mm = fmt.mmask
        self.wmask = (1 << fmt.width) - 1

    def S(self, x):
        return (x >> _u(self.f.width - 1)) & _u(1)

    def E(self, x):
        return (x >> _u(self.Mb)) & _u(self.X)

    def M(self, x):
        return x & _u(self.mm)

    def pack(self, s, e, m):
        return ((s << _u(self.f.width - 1)) | (e << _u(self.Mb)) | m) & _u(self.wmask)

    def mid(self, x):
        return self.pack(self.S(x), _u(self.B - 8) + (self.E(x) & _u(15)), self.M(x))

    def at(self, x, lo: int, mask: int):
        """x moved to exponent field lo + (E x & mask)."""
        return self.pack(self.S(x), _u(lo) + (self.E(x) & _u(mask)), self.M(x))

    def half(self, s, e, t):
        import numpy as np

        return np.where(
            t == 0, self.pack(s, e - _u(self.Mb + 1), _u(0)),
            np.where(t == 1, self.pack(s, e - _u(self.Mb + 1), _u(1)),
                     self.pack(s, e - _u(self.Mb + 2), _u(self.mm))))

    def special(self, x, code):
        import numpy as np

        s = self.S(x)
        zero = self.pack(s, _u(0), _u(0))
        inf = self.pack(s, _u(self.X), _u(0))
        nan = self.pack(s, _u(self.X), self.M(x) | _u(1))
        one = self.pack(s, _u(self.B), _u(0))
        return np.select([(code == 0) | (code == 5), (code == 1) | (code == 6),
                          code == 2, code == 3], [zero, inf, nan, one], self.mid(x))


def _sel_fields(sel):
    v = sel & _u(3)
    t = ((sel >> _u(2)) & _u(255)) % _u(3)
    p = (sel >> _u(10)) & _u(7)
    cm = (sel >> _u(13)) & _u(3)
    return v, t, p, cm


def _triple(fmt: _Fmt, recipe, ra, rb, rc, sel):
    """(a, b, c) bit patterns (uint64 arrays) by the module docstring's
    recipes; ``recipe`` is an integer array 0..7 of the same shape."""
    import numpy as np

    F = _Fields(fmt)
    Mb, B, X = F.Mb, F.B, F.X
    S, E, M, pack = F.S, F.E, F.M, F.pack
    v, t, p, cm = _sel_fields(sel)
    sign = _u(1 << (fmt.width - 1))
    out = []

    # 0 raw
    out.append((ra, rb, rc))
    # 1 mid
    out.append((F.mid(ra), F.mid(rb), F.mid(rc)))

    # 2 ties
    a0 = F.at(ra, B, 7)
    b0 = F.half(S(rb), E(a0), t)
    c0 = F.mid(rc)
    h = (Mb - 1) // 2
    sh = _u(Mb - h)
    ha, hb = (M(ra) >> sh) << sh, (M(rb) >> sh) << sh
    a1 = pack(S(ra), _u(B) + (E(ra) & _u(7)), ha)
    b1 = pack(S(rb), _u(B) + (E(rb) & _u(7)), hb)
    prod = (_u(1 << h) | (ha >> sh)) * (_u(1 << h) | (hb >> sh))
    carry = (prod >> _u(2 * h + 1)) & _u(1)
    c1 = F.half(S(rc), E(a1) + E(b1) - _u(B) + carry, t)
    ka = (Mb + 2) // 2
    kb = Mb + 2 - ka
    sa_ = _u(Mb + 1 - ka)
    sb_ = _u(Mb + 1 - kb) - (t != 0).astype(np.uint64)
    a2 = pack(S(ra), _u(B - 4) + (E(ra) & _u(7)), ((M(ra) >> sa_) | _u(1)) << sa_)
    b2 = pack(S(rb), _u(B - 4) + (E(rb) & _u(7)), ((M(rb) >> sb_) | _u(1)) << sb_)
    is1, is2 = v == 1, v == 2
    out.append((np.where(is1, a1, np.where(is2, a2, a0)),
                np.where(is1, b1, np.where(is2, b2, b0)),
                np.where(is1, c1, c0)))

    # 3 cancel
    a0 = F.mid(ra)
    b0 = a0 ^ sign ^ p
    a1 = F.at(ra, B - 4, 7)
    mb10 = (M(rb) >> _u(Mb - 10)) << _u(Mb - 10)
    b1 = pack(S(rb), _u(B - 4) + (E(rb) & _u(7)), mb10)
    prod = (_u(1 << Mb) | M(a1)) * (_u(1 << 10) | (mb10 >> _u(Mb - 10)))
    carry = (prod >> _u(Mb + 11)) & _u(1)
    top = prod >> (_u(10) + carry)
    c1 = pack(_u(1) ^ S(ra) ^ S(rb), E(a1) + E(b1) - _u(B) + carry,
              top & _u(F.mm)) ^ (p & _u(3))
    odd = (v & _u(1)) == 1
    out.append((np.where(odd, a1, a0), np.where(odd, b1, b0),
                np.where(odd, c1, F.mid(rc))))

    # 4 subnormal operands
    out.append((
        np.where((v & _u(1)) != 0, pack(S(ra), _u(0), M(ra)), F.at(ra, 1, 3)),
        np.where((v & _u(2)) != 0, pack(S(rb), _u(0), M(rb)), F.at(rb, B - 2, 3)),
        np.where((cm & _u(1)) != 0, pack(S(rc), _u(0), M(rc)), F.at(rc, 1, 3))))

    # 5 overflow
    big = lambda x: pack(S(x), _u(X - 1) - (E(x) & _u(1)), M(x))  # noqa: E731
    out.append((big(ra),
                np.where(v == 1, F.at(rb, B, 3),
                         np.where(v == 2, pack(S(rb), _u(B - 1) - (E(rb) & _u(3)), M(rb)),
                                  big(rb))),
                big(rc)))

    # 6 underflow
    out.append((
        F.at(ra, 1, 7),
        np.select([v == 0, v == 1, v == 2],
                  [F.at(rb, B - Mb - 4, 7),
                   pack(S(rb), _u(B) - (E(rb) & _u(7)), M(rb)),
                   F.at(rb, B + 1, 7)], F.at(rb, B + Mb - 2, 7)),
        np.select([cm == 0, cm == 1],
                  [pack(S(rc), _u(0), _u(0)), pack(S(rc), _u(0), M(rc))], F.at(rc, 1, 3))))

    # 7 specials
    out.append((F.special(ra, (sel >> _u(16)) & _u(7)),
                F.special(rb, (sel >> _u(19)) & _u(7)),
                F.special(rc, (sel >> _u(22)) & _u(7))))

    conds = [recipe == k for k in range(7)]
    return tuple(np.select(conds, [o[i] for o in out[:7]], out[7][i]) for i in range(3))


def _fma64_operand(x):
    """Stage 1's fma operand: exponents more than 200 from the bias are
    remapped to B - 64 + (E & 127)."""
    import numpy as np

    F = _Fields(F64)
    e = F.E(x)
    far = (e + _u(200) < _u(F.B)) | (e > _u(F.B + 200))
    return np.where(far, F.at(x, F.B - 64, 127), x)


def _cvt_operands(recipe, rx, rd, ru, sel):
    """(x, xi, d, u) of the cvt stage: f32 pattern, the pattern f32_i32
    takes, f64 pattern, u32 — all uint64 arrays."""
    import numpy as np

    v, t, _, _ = _sel_fields(sel)
    F, D = _Fields(F32), _Fields(F64)
    s, e, m = F.S(rx), F.E(rx), F.M(rx)

    def low(base, bits: int):
        """base with its low ``bits`` bits set to half, half + 1, half - 1."""
        h = 1 << (bits - 1)
        return (base & ~_u((1 << bits) - 1)) \
            + np.select([t == 0, t == 1], [_u(h), _u(h + 1)], _u(h - 1))

    x1 = F.pack(s, _u(99) + (e & _u(63)), m)
    x2 = np.where((v & _u(1)) != 0, low(x1, 13), low(x1, 16))
    ee = e & _u(31)  # unbiased exponent ee - 2
    hb = (_u(24) - ee) & _u(31)  # mantissa bit worth 0.5, for ee in 2..24
    keep = ~((_u(2) << hb) - _u(1)) & _u(F.mm)
    m3 = np.where((ee >= 2) & (ee <= 24) & (t != 1),
                  (m & keep) | np.where(t == 0, _u(1) << hb, _u(0)), m)
    x3 = F.pack(s, _u(125) + ee, m3)
    x4 = F.pack(s, _u(0), m)
    x5 = np.where(
        v == 2,
        # the top 2**-8 of the largest binade: about the largest finite bf16
        F.pack(s, _u(254), _u(0x7F0000) | (m & _u(0xFFFF))),
        F.pack(s, _u(141) + (e & _u(3)),
               np.where((v & _u(1)) != 0, _u(0x7FE000) | (m & _u(0x1FFF)), m)))
    x6 = F.pack(s, _u(151) + (e & _u(7)), m)
    x7 = F.special(rx, (sel >> _u(16)) & _u(7))
    x = np.select([recipe == k for k in range(7)], [rx, x1, x2, x3, x4, x5, x6], x7)
    xi = np.where(F.E(x) >= _u(158), F.at(x, 150, 7), x)

    ds, de, dm = D.S(rd), D.E(rd), D.M(rd)
    d1 = D.pack(ds, _u(1023 - 128) + (de & _u(255)), dm)
    d2 = low(d1, 29)
    d4 = D.pack(ds, _u(1023 - 152) + (de & _u(31)), dm)
    d5 = D.pack(ds, _u(1023 + 127) + (de & _u(1)),
                np.where((v & _u(1)) != 0,
                         _u(0xFFFFFE0000000) | (dm & _u(0x1FFFFFFF)), dm))
    d6 = D.pack(ds, de & _u(15), dm)
    d7 = D.special(rd, (sel >> _u(19)) & _u(7))
    d = np.select([recipe == k for k in range(7)], [rd, d1, d2, d1, d4, d5, d6], d7)

    pbit = _u(24) + ((sel >> _u(8)) & _u(7))
    top = (ru | _u(0x80000000)) >> (_u(31) - pbit)
    ub = pbit - _u(24)
    u2 = ((top & ~((_u(2) << ub) - _u(1)))
          + np.select([t == 0, t == 1], [_u(1) << ub, (_u(1) << ub) + _u(1)],
                      (_u(1) << ub) - _u(1))) & _u(0xFFFFFFFF)
    u = np.where(recipe == 2, u2,
                 np.where((recipe & 1) != 0, ru >> ((sel >> _u(8)) & _u(31)), ru))
    return x, xi, d, u


# -- reference arithmetic --------------------------------------------------------------

def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _round_to_odd_sum(a, b):
    """a + b in float64 rounded to odd: where the sum is inexact and its
    last bit even, one ulp toward the error."""
    import numpy as np

    s, e = _two_sum(a, b)
    bits = s.view(np.int64).copy()
    fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((bits & 1) == 0)
    step = np.where((e > 0) == (s > 0), 1, -1)
    return np.where(fix, bits + step, bits).view(np.float64)


def fma_narrow(a, b, c):
    """Correctly rounded fma of float16 or float32 arrays: the product is
    exact in float64, the sum with c is rounded to odd there, and the
    cast does the one real rounding."""
    import numpy as np

    with np.errstate(all="ignore"):
        p = a.astype(np.float64) * b.astype(np.float64)
        return _round_to_odd_sum(p, c.astype(np.float64)).astype(a.dtype)


def _split(a):
    c = 134217729.0 * a  # 2**27 + 1
    h = c - (c - a)
    return h, a - h


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def fma_f64(a, b, c):
    """Correctly rounded float64 fma (Boldo-Melquiond) for operands whose
    exponents are within 200 of the bias: exact product as a pair, exact
    sum of its high part with c, the two low parts summed to odd, one
    final rounding."""
    import numpy as np

    with np.errstate(all="ignore"):
        ph, pl = _two_prod(a, b)
        sh, sl = _two_sum(ph, c)
        return sh + _round_to_odd_sum(pl, sl)


def f32_to_bf16_bits(bits):
    """Round-to-nearest-even on the f32 bit pattern (uint64 array) ->
    bf16 pattern, NaN canonical."""
    import numpy as np

    bits = bits.astype(np.uint64)
    nan = (bits & _u(0x7FFFFFFF)) > _u(0x7F800000)
    r = (bits + _u(0x7FFF) + ((bits >> _u(16)) & _u(1))) >> _u(16)
    return np.where(nan, _u(BF16_CANONICAL_NAN), r & _u(0xFFFF))


def _check_subnormals():
    import numpy as np

    with np.errstate(all="ignore"):
        if (np.float32(1e-40) * np.float32(0.5) == 0
                or np.float64(1e-310) * np.float64(0.5) == 0
                or np.float16(6e-8) + np.float16(0) == 0):
            raise RuntimeError(
                "fpcheck: this host flushes subnormals to zero; numpy cannot "
                "serve as the IEEE reference")


def _five(fmt: _Fmt, a, b, c, fa=None, fb=None, fc=None):
    """add, mul, fma, div, sqrt|a| of bit patterns -> list of uint64 bits."""
    import numpy as np

    x, y, z = (_as_float(q, fmt) for q in (a, b, c))
    with np.errstate(all="ignore"):
        if fmt is F64:
            fma = fma_f64(*(_as_float(q, fmt) for q in (fa, fb, fc)))
        else:
            fma = fma_narrow(x, y, z)
        res = [x + y, x * y, fma, x / y, np.sqrt(np.abs(x))]
    return [_as_bits(q, fmt) for q in res]


# -- numpy definition ------------------------------------------------------------------

def _slot_words(seed: int, stage: int, r):
    """uint64[len(r), slots, 16]: the words of every slot, zero-extended."""
    import numpy as np

    n = 64 * SLOTS_PER_LANE[stage] * WORDS_PER_SLOT
    idx = np.arange(n, dtype=np.uint32)
    rp = (r % np.uint32(PERIOD)).astype(np.uint32)
    w = _fmix32(_base(seed, _STAGE0 + stage, rp)[:, None] + idx[None, :])
    return w.astype(np.uint64).reshape(len(r), -1, WORDS_PER_SLOT)


def _recipes(stage: int, r, e: int = 0):
    """int64[len(r), slots]: recipe of element e of every slot."""
    import numpy as np

    q = np.arange(64 * SLOTS_PER_LANE[stage], dtype=np.int64)
    rp = (r % np.uint32(PERIOD)).astype(np.int64)
    return ((q & 63)[None, :] + (q >> 6)[None, :] + rp[:, None] + 3 * e) & 7


def _raw(w, e: int, fmt: _Fmt):
    lo = 8 * e
    if fmt is F64:
        ra, rb, rc = (w[..., lo + k] | (w[..., lo + k + 1] << _u(32)) for k in (0, 2, 4))
    else:
        mask = _u((1 << fmt.width) - 1)
        ra, rb, rc = (w[..., lo + k] & mask for k in (0, 2, 4))
    return ra, rb, rc, w[..., lo + 6]


def _stage(seed: int, stage: int, r):
    """(operands, results) of a stage for rounds ``r`` (uint32 array):
    dicts name -> uint64[len(r), slots]; results in OPS order."""
    import numpy as np

    if stage not in range(len(STAGES)):
        raise ValueError(f"stage {stage} out of range 0..3")
    _check_subnormals()
    w = _slot_words(seed, stage, r)
    ops: Dict[str, object] = {}
    if stage in (0, 1):
        fmt = F32 if stage == 0 else F64
        a, b, c = _triple(fmt, _recipes(stage, r), *_raw(w, 0, fmt))
        ops.update(a=a, b=b, c=c)
        if stage == 1:
            fa, fb, fc = (_fma64_operand(q) for q in (a, b, c))
            ops.update(fma_a=fa, fma_b=fb, fma_c=fc)
            res = _five(fmt, a, b, c, fa, fb, fc)
        else:
            res = _five(fmt, a, b, c)
    elif stage == 2:
        res_h, res_f = [], []
        for e in (0, 1):
            rec = _recipes(stage, r, e)
            for fmt, acc, tag in ((F16, res_h, "h"), (F32, res_f, "f")):
                a, b, c = _triple(fmt, rec, *_raw(w, e, fmt))
                ops.update({f"{tag}{e}.a": a, f"{tag}{e}.b": b, f"{tag}{e}.c": c})
                add, mul, fma, _, _ = _five(fmt, a, b, c)
                acc.append((fma, mul, add))
        res = [res_h[0][k] | (res_h[1][k] << _u(16)) for k in range(3)]
        for k in range(3):
            res += [res_f[0][k], res_f[1][k]]
    else:
        x, xi, d, u = _cvt_operands(_recipes(stage, r), w[..., 0],
                                    w[..., 2] | (w[..., 3] << _u(32)), w[..., 4], w[..., 6])
        ops.update(x=x, xi=xi, d=d, u=u)
        xf, xif, df = _as_float(x, F32), _as_float(xi, F32), _as_float(d, F64)
        u32 = u.astype(np.uint32)
        with np.errstate(all="ignore"):
            res = [
                _as_bits(xf.astype(np.float16), F16),
                f32_to_bf16_bits(x),
                _as_bits(df.astype(np.float32), F32),
                _as_bits(u32.astype(np.float32), F32),
                _as_bits(u32.view(np.int32).astype(np.float32), F32),
                # |xi| < 2**31 and finite by construction; int64 first so
                # that the cast is defined whatever the platform
                np.trunc(xif).astype(np.int64).astype(np.uint64) & _u(0xFFFFFFFF),
                _as_bits(np.rint(xf), F32), _as_bits(np.floor(xf), F32),
                _as_bits(np.ceil(xf), F32), _as_bits(np.trunc(xf), F32),
            ]
    return ops, dict(zip(OPS[stage], res))


def reference_values(seed: int, stage: int, r: int):
    """Raw result bits of one stage and round: {operation: uint64[slots]}
    in OPS[stage] order, slot q = 64 j + lane.  NaN results are canonical.
    Raises RuntimeError if this host flushes subnormals."""
    _, res = _stage(int(seed) & 0xFFFFFFFF, int(stage),
                      _shared.one_round("fpcheck", r))
    return {k: v[0] for k, v in res.items()}


def reference_operands(seed: int, stage: int, r: int):
    """The operand bit patterns behind ``reference_values``:
    {name: uint64[slots]}."""
    ops, _ = _stage(int(seed) & 0xFFFFFFFF, int(stage),
                      _shared.one_round("fpcheck", r))
    return {k: v[0] for k, v in ops.items()}


def operands_of(stage: int, op: str) -> Tuple[str, ...]:
    """Names in ``reference_operands`` that feed operation ``op``."""
    if stage == 0:
        return ("a", "b", "c")
    if stage == 1:
        return ("fma_a", "fma_b", "fma_c") if op == "fma" else ("a", "b", "c")
    if stage == 2:
        tag = "h" if op.endswith("f16") else "f"
        es = (0, 1) if tag == "h" else ((0,) if op.endswith(".x") else (1,))
        return tuple(f"{tag}{e}.{n}" for e in es for n in "abc")
    return {"f32_f16": ("x",), "f32_bf16": ("x",), "f64_f32": ("d",), "u32_f32": ("u",),
            "i32_f32": ("u",), "f32_i32": ("xi",)}.get(op, ("x",))


def _digest(stage: int, res: Dict[str, object]):
    """uint32[rounds] from {op: uint64[rounds, slots]}."""
    import numpy as np

    slots = 64 * SLOTS_PER_LANE[stage]
    q = np.arange(slots, dtype=np.uint32)
    total = 0
    for k, name in enumerate(OPS[stage]):
        bits = res[name]
        salt = _salt(q + np.uint32(slots * k))[None, :]
        lo = (bits & _u(0xFFFFFFFF)).astype(np.uint32)
        if stage == 1:
            hi = (bits >> _u(32)).astype(np.uint32)
            h = _fmix32(lo ^ _fmix32(hi + salt))
        else:
            h = _fmix32(lo + salt)
        total = total + h.sum(axis=1, dtype=np.uint32)
    return total


def reference_digests(seed: int, rounds: int):
    """Expected digests as uint32[rounds, 4], columns in STAGES order:
    min(rounds, PERIOD) rows are computed and tiled.

    Pure numpy: needs neither torch nor a GPU.  This is the definition
    the GPU kernel is tested against."""
    import numpy as np

    seed = int(seed) & 0xFFFFFFFF
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("reference_digests: rounds >= 0 required")
    n = min(rounds, PERIOD)
    rows = np.empty((n, len(STAGES)), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for lo in range(0, n, 32):
            r = np.arange(lo, min(lo + 32, n), dtype=np.uint32)
            for s in range(len(STAGES)):
                rows[lo:lo + len(r), s] = _digest(s, _stage(seed, s, r)[1])
    return _shared.tile_period(rows, rounds, PERIOD)


# -- GPU run ---------------------------------------------------------------------

@dataclass
class FpcheckResult(DigestResult):
    # Whole-run lower bounds per stage in 1e9 results per second (the
    # kernel's time also holds operand generation, the other stages and
    # the digests): informative.
    f32_gops: float = 0.0
    f64_gops: float = 0.0
    packed_gops: float = 0.0
    cvt_gops: float = 0.0


def fpcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> FpcheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup asks for a CU's whole LDS without touching it, so on an
    idle GPU the default grid lands one workgroup on every CU;
    ``cus_covered`` reports how many distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot corrupt a
    rounding unit."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    return _shared.run_probe(
        "fpcheck", FpcheckResult(rounds=rounds), STAGES, _OPS_PER_WAVE_ROUND, 1e9,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected)


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``fpcheck`` with its dump pointer set."""
    return _shared.wave_digests(
        "fpcheck", _ext().fpcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device)


def wave_values(seed: int, stage: int, r: int, device=None):
    """The raw result bits wave 0 of one workgroup computed for a stage
    and round, shaped like ``reference_values``: {operation:
    uint64[slots]}, NaN canonical.  A digest cannot say which operation
    on which operands is wrong; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    with torch.cuda.device(_device(device)):
        raw = _ext().fpcheck_values(int(seed), stage, int(r)).cpu().numpy()
    raw = raw.view(np.uint64).reshape(len(OPS[stage]), 64 * SLOTS_PER_LANE[stage])
    return {name: raw[k] for k, name in enumerate(OPS[stage])}


# -- child process -----------------------------------------------------------

def run_fpcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                           timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the fpcheck CLI."""
    return _active.run_probe_subprocess("fpcheck", index, "--rounds", rounds, timeout_s)


def fpcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                  rounds: int = DEFAULT_ROUNDS,
                  max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("fpcheck", "mismatches", _shared.metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "fpcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: fpcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
