"""Active probe for the integer vector and scalar ALUs — wrapper over the
intcheck HIP kernel.

Address arithmetic, loop control, masks, quantised dot products and packed
16-bit math all run on the integer datapath, and no other probe issues an
integer operation as workload (cucheck's ``valu`` stage runs four on raw
random words).  A carry chain that breaks at one bit, a shifter that
fails at amount 0 or 31, a saturating pipe that wraps, a scalar ALU with a
stuck bit (which corrupts addresses for a whole wave) move no ECC counter.
Every operation here is exact in C and in Python integers, so numpy is an
exact reference.  ``intcheck()`` launches one 16-wave workgroup per
compute unit; every wave runs the same deterministic sequence of integer
operations and compares four 32-bit digests per round with
``reference_digests``.  Launch shape, accounting and the mismatch log are
cucheck's.

The workload (csrc/intcheck.hip; ``reference_values`` and
``reference_digests`` are the definition).  Arithmetic is mod 2**32 unless
said otherwise; ``fmix32``, ``base``, ``salt`` are cucheck's and the stage
number fed to ``base`` is 48 + s.  Inputs repeat with PERIOD = 64 rounds:

  word(s, r, idx) = fmix32(base(seed, 48 + s, r % PERIOD) + idx)

Nothing depends on the wave number.  sext(x, n) sign-extends the low n
bits; (h:l) is the 64-bit value with high word h and low word l; a 64-bit
result takes two slots, ``.lo`` then ``.hi``.  Every result is a *result
slot*, a row of 64 u32, numbered in the order below (``slot_table``).

Operands of the vector stages (``operands``).  A stage applies its whole
list of ops to GROUPS = 2 operand groups j; group j's slots follow group
j - 1's and are named ``j.op``.  Operand slot q = 64 j + lane; words 8 q
.. 8 q + 3 are ra, rb, rc, sel.  Raw random words almost never hit an
integer edge, so a, b, c come from recipe (lane + j + r) mod 8:

  0 raw    a, b, c = ra, rb, rc
  1 small  sext(ra, 9), sext(rb, 17), sext(rc, 5)
  2 edge   EDGE[sel & 15], EDGE[(sel >> 4) & 15], EDGE[(sel >> 8) & 15]
  3 bit    1 << (ra & 31), ~(1 << (rb & 31)), 1 << (rc & 31)
  4 run    run(ra), run(rb), rc with run(x) = rotl((1 << ((x >> 8) & 31))
           - 1, x & 31)
  5 carry  ra, ~ra + sext(sel, 3), rc & 1: a + b lies within 4 of 2**32 -
           1, so the carry runs across every bit
  6 equal  a = ra; b = a, or a ^ (1 << (sel & 31)) where sel bit 5 is set;
           c = a ^ INT_MIN: compares at equality and at the sign boundary
  7 bytes  byte i of a, b, c = BYTES[(sel >> (3 i + o)) & 7] with o = 0, 12,
           20; codes 6 and 7 keep the raw byte of ra, rb, rc

X = (c:a) and Y = (a ^ INT_MIN : b) are the 64-bit operands.

Stages (STAGES) and their ops, in slot order:

  bits    n = b & 31, n6 = b & 63.  shl, shr, sar of a by n; shl64, shr64,
          sar64 of X by n6; alignbit = low 32 of ((a:c) >> n); rotr =
          alignbit(a, a, n); alignbyte = low 32 of ((a:c) >> 8 (b & 3));
          ubfe, sbfe(a, off, w) with off = n and w = (b >> 8) mod (min(31,
          32 - off) + 1), width 0 giving 0; bfi = (a & b) | (~a & c);
          perm(a, c, S): byte i of S is code (sel >> 4 i & 15) mod 9, codes
          0..3 picking that byte of c, 4..7 of a, 8 standing for selector
          0x0C = 0x00; brev; popc_add = popcount(a) + c; clz, ctz (32 for
          0), clrsb (redundant sign bits, 31 for 0 and -1); popc64, clz64
          of X (64 for 0); shl1_add .. shl4_add = (a << k) + b; add_shl =
          (a + b) << 3; shl_or = (a << 2) | b; and_or = (a & b) | c; or3;
          add3; xad = (a ^ b) + c.
  arith   add3l.0 .. 2 and add3l.carry: the limbs of (a, b, c) + (b, c, a)
          and the final carry; sub3l.0 .. 2, sub3l.borrow of (a, b, c) -
          (b, c, a); add64 = X + Y, sub64 = X - Y; mul_lo, mulhi_u,
          mulhi_i; mul_i24, mulhi_i24, mul_u24, mulhi_u24 on sext(., 24) /
          the low 24 bits of a, b; mad_u64 = (u64) a * b + X, mad_i64 =
          (i64) a * b + X, mul64 = low 64 of X * Y; udiv, urem, sdiv, srem
          of a by b, C semantics, with the denominator 0 remapped to 1 and
          INT_MIN / -1 to INT_MIN / 1 (C leaves both undefined); udiv64,
          urem64 of X by Y >> (sel >> 26), 0 remapped to 1; min_i, max_i,
          min_u, max_u; med3_i, med3_u, min3_i, min3_u, max3_i, max3_u of
          a, b, c; absdiff = |a - b| unsigned; the ballots of a < b signed
          (lt_i), unsigned (lt_u), a == b (eq), X < Y unsigned (lt_u64)
          and signed (lt_i64), each as two slots holding the mask's low
          and high word in every lane; select4: s = a & 1 ? b : c; s = s <
          a ? s + 1 : a; s = s < b signed ? s ^ c : s - b; s = s == c ? a
          : s.
  packed  on the two 16-bit halves: add16, sub16 (wrapping), add_sat_i16,
          sub_sat_i16, add_sat_u16, sub_sat_u16, mul16, mad_i16 = a * c +
          b, mad_u16 = a * b + c (wrapping, so the same bits signed or
          unsigned), min_i16, max_i16,
          min_u16, max_u16, shl16, lshr16, ashr16 by b's half & 15;
          sad_u8 = c + sum |a.byte - b.byte|; sad_hi_u8 = c + (sum << 16);
          sad_u16 = c + sum |a.half - b.half|; lerp: byte i = (a.byte[i] +
          b.byte[i] + (c.byte[i] & 1)) >> 1; sdot4, udot4 (bytes), sdot8,
          udot8 (nibbles), sdot2, udot2 (halves): c + sum of products mod
          2**32, and each again as ``.clamp``: the exact sum saturated to
          i32 / u32, with c replaced by ANCHOR[sel >> 30] + sext(c, w) mod
          2**32, w = CLAMP_BITS = 15, 8, 18 for the dot4, dot8 and dot2
          pairs (the size of their sums of products), ANCHOR = INT_MAX,
          INT_MIN, 0, UINT_MAX, so that saturation happens in both
          directions, and not at all, many times in every period.
  scalar  v(k)[l] = word(64 k + l), u(k) = word(64 k) through
          v_readfirstlane.  Two groups j of wave-uniform operands x, y, z
          = recipe (j + r) mod 8 of ra, rb, rc, sel = u(4 + 4 j) .. u(7 +
          4 j); Z = (z:x), W = (x ^ INT_MIN : y).  Every result is the same
          in all lanes.  popc, ctz, clz, brev, clrsb of x; popc64, ctz64
          of Z; mul_lo, mulhi_u, mulhi_i of x, y; shl, shr, sar of x by y
          & 31; shl64, shr64, sar64 of Z by y & 63; field_u = (x >> (y &
          31)) & ((1 << (y >> 8 & 15)) - 1), field_i = (i32)(x << (31 - (y
          & 31))) >> (y >> 16 & 31); min_i, max_i, min_u, max_u, absdiff;
          andn2 = x & ~y, orn2 = x | ~y, nand, nor, xnor; sext8, sext16;
          add64 = Z + W, sub64 = Z - W; shl1_add .. shl4_add; switch on
          sel & 3: x + y, x ^ (y >> 3), (x & y) * 3, x - z; loop(t): h =
          0; while t: h = h * 33 + ctz(t); t &= t - 1 — the one bounded
          data-dependent loop, 0..32 trips — as loop = loop(x) and loop2
          = loop(x & (x - 1)).  Then once the wave-mask block: m1 =
          ballot(v(0) < v(1)), m2 = ballot(v(2) & 1), andn = m1 & ~m2, xor
          = m1 ^ m2, each as .lo / .hi; popc, ctz, clz (64 for 0) of the
          four; m1.shl = m1 << (u(3) & 63), m1.sar = (i64) m1 >> (u(3) &
          63).

Digest of a stage: sum over slots n and lanes l of fmix32(value_n[l] +
salt(64 n + l)), mod 2**32.

Not covered: v_msad_u8, v_qsad_*, v_mqsad_* (video ops whose masking rule
no document at hand fixes), v_perm selectors 8..0xB and >= 0xD, bfe fields
that run past bit 31, SDWA, integer atomics (atomcheck), the integer
matrix cores (cucheck).

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.intcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

from . import _active
from . import _digest as _shared
from ._active import (  # noqa: F401
    EXIT_CANNOT_RUN,
    EXIT_MISMATCH,
    EXIT_PASS,
    _ext,
    idle_gpus,
)
from ._digest import (  # noqa: F401
    WAVES_PER_BLOCK,
    DigestResult,
    _base,
    _device,
    _fmix32,
    metric_args,
)
from .lanecheck import _ballot, _digest, _rows, digest_of  # noqa: F401

STAGES: Tuple[str, ...] = ("bits", "arith", "packed", "scalar")
PERIOD = 64  # inputs of round r are those of round r % PERIOD
_STAGE0 = 48  # stage number fed to base() is _STAGE0 + s
GROUPS = 2  # operand groups per stage
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/intcheck_mi355x.json), default grid (256
# workgroups, 4096 waves): 37.08, 35.31 and 34.71 us per round at 256,
# 1024 and 4096 rounds (the fixed cost of a launch fades), so 0.5 s are
# 14405 rounds; the nearest multiple of PERIOD, 225 x 64 = 14400 rounds,
# took 0.497 s.  The numpy table costs about 0.1 s of host time whatever
# the rounds, since only PERIOD rows are computed.
DEFAULT_ROUNDS = 14400
_VALUE_ROWS = 128

_M32 = 0xFFFFFFFF
INT_MIN, INT_MAX = 0x80000000, 0x7FFFFFFF
EDGE: Tuple[int, ...] = (0, 1, 2, 0xFFFFFFFF, 0xFFFFFFFE, INT_MAX, INT_MIN, INT_MIN + 1,
                         0xFFFF, 0x10000, 0xFF, 0x100, 0x7FFFFF, 0x800000, 0xFFFFFF,
                         0xFF800000)
BYTES: Tuple[int, ...] = (0x00, 0x01, 0x7F, 0x80, 0xFF, 0xFE)  # codes 6, 7: the raw byte
ANCHOR: Tuple[int, ...] = (INT_MAX, INT_MIN, 0, 0xFFFFFFFF)
CLAMP_BITS = {8: 15, 4: 8, 16: 18}  # field width of a dot -> bits of the offset to ANCHOR

# integer operations one wave issues per round, per stage (a wave
# instruction counts 64, a 64-bit result as one)
_OPS_PER_WAVE_ROUND = (64 * GROUPS * 30, 64 * GROUPS * 44, 64 * GROUPS * 32,
                       GROUPS * 40 + 20)


# -- numpy helpers: u32 values live in uint64 arrays, masked ------------------------------

def _u(x):
    import numpy as np

    return np.asarray(x).astype(np.uint64) & np.uint64(_M32)


def _i(x, bits: int = 32):
    """The low ``bits`` bits of x, sign-extended, as int64."""
    import numpy as np

    m = np.uint64((1 << bits) - 1)
    x = np.asarray(x).astype(np.uint64) & m
    return x.astype(np.int64) - ((x >> np.uint64(bits - 1)) << np.uint64(bits)).astype(np.int64)


def _sext(x, bits: int):
    return _u(_i(x, bits))


def _cat(hi, lo):
    import numpy as np

    return (_u(hi) << np.uint64(32)) | _u(lo)


def _popc(x):
    import numpy as np

    x = np.asarray(x, dtype=np.uint64)
    return sum((x >> np.uint64(k)) & np.uint64(1) for k in range(64))


def _clz(x, bits: int):
    """Leading zeros of the ``bits``-bit x; ``bits`` for 0."""
    import numpy as np

    x = np.asarray(x, dtype=np.uint64).copy()
    for k in (1, 2, 4, 8, 16, 32):
        x |= x >> np.uint64(k)
    return np.uint64(bits) - _popc(x)


def _ctz(x, bits: int):
    import numpy as np

    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        low = (x & (~x + np.uint64(1))) - np.uint64(1)  # ones below the lowest set bit
    return _popc(low & np.uint64((1 << bits) - 1))


def _brev(x):
    import numpy as np

    x = _u(x)
    return sum(((x >> np.uint64(k)) & np.uint64(1)) << np.uint64(31 - k) for k in range(32))


def _clrsb(x):
    import numpy as np

    x = _u(x)
    return _clz(x ^ _u(_i(x) >> np.int64(31)), 32) - np.uint64(1)


def _shl(x, n):
    return _u(_u(x) << n)


def _sar64(x, n):
    import numpy as np

    return (np.asarray(x, dtype=np.uint64).astype(np.int64) >> n.astype(np.int64)).astype(
        np.uint64)


def _parts(x, bits: int, signed: bool = False):
    """The 32 // bits fields of a u32, lowest first, as int64."""
    import numpy as np

    out = [(_u(x) >> np.uint64(k)) & np.uint64((1 << bits) - 1) for k in range(0, 32, bits)]
    return [_i(p, bits) if signed else p.astype(np.int64) for p in out]


def _join(parts, bits: int):
    import numpy as np

    m = np.uint64((1 << bits) - 1)
    return sum((np.asarray(p).astype(np.uint64) & m) << np.uint64(bits * k)
               for k, p in enumerate(parts))


def _pk(f, bits: int, signed: bool, *xs):
    """f on the fields of the operands, joined."""
    cols = zip(*(_parts(x, bits, signed) for x in xs))
    return _join([f(*c) for c in cols], bits)


def _w64(name: str, x) -> List[tuple]:
    import numpy as np

    x = np.asarray(x).astype(np.uint64)
    return [(name + ".lo", x & np.uint64(_M32)), (name + ".hi", x >> np.uint64(32))]


def _where(cond, a, b):
    import numpy as np

    return np.where(cond, a, b)


# -- operands ----------------------------------------------------------------------

def _recipe(k, ra, rb, rc, sel):
    """a, b, c of recipe ``k`` (an array like the words) from the raw
    words, as uint64 arrays holding u32."""
    import numpy as np

    ra, rb, rc, sel = _u(ra), _u(rb), _u(rc), _u(sel)
    one, m5 = np.uint64(1), np.uint64(31)
    edge = np.array(EDGE, dtype=np.uint64)
    byte = np.array(BYTES + (0, 0), dtype=np.uint64)

    def rotl(x, n):
        return _u((x << n) | (x >> ((np.uint64(32) - n) & m5)))

    def run(x):
        return rotl((one << ((x >> np.uint64(8)) & m5)) - one, x & m5)

    def bytes_of(raw, o):
        out = []
        for i in range(4):
            code = (sel >> np.uint64(3 * i + o)) & np.uint64(7)
            out.append(_where(code >= 6, (raw >> np.uint64(8 * i)) & np.uint64(0xFF),
                              byte[code.astype(np.int64)]))
        return _join(out, 8)

    bit6 = ra ^ (one << (sel & m5))
    recipes = (
        (ra, rb, rc),
        (_sext(ra, 9), _sext(rb, 17), _sext(rc, 5)),
        tuple(edge[((sel >> np.uint64(s)) & np.uint64(15)).astype(np.int64)] for s in (0, 4, 8)),
        (one << (ra & m5), _u(~(one << (rb & m5))), one << (rc & m5)),
        (run(ra), run(rb), rc),
        (ra, _u(_u(~ra) + _sext(sel, 3)), rc & one),
        (ra, _where((sel >> np.uint64(5)) & one != 0, bit6, ra), ra ^ np.uint64(INT_MIN)),
        (bytes_of(ra, 0), bytes_of(rb, 12), bytes_of(rc, 20)),
    )
    k = np.asarray(k).astype(np.int64)
    return tuple(np.choose(k, [rec[i] for rec in recipes]) for i in range(3))


def _base_of(seed: int, stage: int, r):
    import numpy as np

    rp = (np.asarray(r, dtype=np.uint32) % np.uint32(PERIOD)).astype(np.uint32)
    return rp, _base(seed, _STAGE0 + stage, rp)


def _word(base, idx):
    import numpy as np

    with np.errstate(over="ignore"):
        return _fmix32(base + np.asarray(idx, dtype=np.uint32))


def operands(seed: int, stage: int, r, j: int):
    """(a, b, c, sel) of operand group ``j`` of vector stage ``stage`` in
    rounds ``r`` (an array): uint64 [rounds, 64] holding u32."""
    import numpy as np

    rp, base = _base_of(int(seed) & _M32, stage, r)
    lane = np.arange(64, dtype=np.uint32)
    q = np.uint32(8) * (np.uint32(64 * j) + lane)[None, :]
    ra, rb, rc, sel = (_word(base[:, None], q + np.uint32(i)) for i in range(4))
    k = (lane[None, :] + np.uint32(j) + rp[:, None]) % np.uint32(8)
    return _recipe(k, ra, rb, rc, sel) + (_u(sel),)


def scalar_operands(seed: int, r, j: int):
    """(x, y, z, sel) of group ``j`` of the scalar stage in rounds ``r``:
    uint64 [rounds]."""
    import numpy as np

    rp, base = _base_of(int(seed) & _M32, 3, r)
    ra, rb, rc, sel = (_word(base, 64 * (4 + 4 * j + i)) for i in range(4))
    return _recipe((rp + np.uint32(j)) % np.uint32(8), ra, rb, rc, sel) + (_u(sel),)


# -- the stages: [(name, values)] of one operand group --------------------------------------

def _ops_bits(a, b, c, sel) -> List[tuple]:
    import numpy as np

    u64 = np.uint64
    n, n6, X = b & u64(31), b & u64(63), _cat(c, a)
    out = [("shl", _shl(a, n)), ("shr", a >> n), ("sar", _u(_i(a) >> n.astype(np.int64)))]
    out += _w64("shl64", X << n6) + _w64("shr64", X >> n6) + _w64("sar64", _sar64(X, n6))
    out.append(("alignbit", _u(_cat(a, c) >> n)))
    out.append(("rotr", _u(_cat(a, a) >> n)))
    out.append(("alignbyte", _u(_cat(a, c) >> (u64(8) * (b & u64(3))))))
    w = (b >> u64(8)) % (np.minimum(u64(31), u64(32) - n) + u64(1))
    field = (a >> n) & ((u64(1) << w) - u64(1))
    out.append(("ubfe", field))
    sign = _where(w == 0, u64(0), (field >> (np.maximum(w, u64(1)) - u64(1))) & u64(1))
    out.append(("sbfe", _u(field | _u(u64(0) - (sign << w)))))
    out.append(("bfi", (a & b) | (_u(~a) & c)))
    both = _parts(c, 8) + _parts(a, 8) + [np.zeros_like(a, dtype=np.int64)]
    picked = []
    for i in range(4):
        code = ((sel >> u64(4 * i)) & u64(15)) % u64(9)
        picked.append(np.choose(code.astype(np.int64), both))
    out.append(("perm", _join(picked, 8)))
    out.append(("brev", _brev(a)))
    out.append(("popc_add", _u(_popc(a) + c)))
    out += [("clz", _clz(a, 32)), ("ctz", _ctz(a, 32)), ("clrsb", _clrsb(a))]
    out += [("popc64", _popc(X)), ("clz64", _clz(X, 64))]
    out += [(f"shl{k}_add", _u(_shl(a, u64(k)) + b)) for k in (1, 2, 3, 4)]
    out.append(("add_shl", _shl(a + b, u64(3))))
    out.append(("shl_or", _shl(a, u64(2)) | b))
    out += [("and_or", (a & b) | c), ("or3", a | b | c), ("add3", _u(a + b + c)),
            ("xad", _u((a ^ b) + c))]
    return out


def _divmod_c(a, b):
    """C's truncating / and % on int64 arrays, b != 0."""
    import numpy as np

    q = np.abs(a) // np.abs(b) * np.sign(a) * np.sign(b)
    return q, a - q * b


def _ops_arith(a, b, c, sel) -> List[tuple]:
    import numpy as np

    u64, one = np.uint64, np.uint64(1)
    X, Y = _cat(c, a), _cat(a ^ u64(INT_MIN), b)
    ia, ib, ic = _i(a), _i(b), _i(c)
    out = []
    carry = u64(0)
    for i, (p, q) in enumerate(((a, b), (b, c), (c, a))):
        s = p + q + carry
        out.append((f"add3l.{i}", _u(s)))
        carry = s >> u64(32)
    out.append(("add3l.carry", carry))
    borrow = np.int64(0)
    for i, (p, q) in enumerate(((a, b), (b, c), (c, a))):
        d = p.astype(np.int64) - q.astype(np.int64) - borrow
        out.append((f"sub3l.{i}", _u(d)))
        borrow = (d < 0).astype(np.int64)
    out.append(("sub3l.borrow", _u(borrow)))
    with np.errstate(over="ignore"):
        out += _w64("add64", X + Y) + _w64("sub64", X - Y)
        out += [("mul_lo", _u(a * b)), ("mulhi_u", (a * b) >> u64(32)),
                ("mulhi_i", _u((ia * ib) >> np.int64(32)))]
        s24 = _i(a, 24) * _i(b, 24)
        u24 = (a & u64(0xFFFFFF)) * (b & u64(0xFFFFFF))
        out += [("mul_i24", _u(s24)), ("mulhi_i24", _u(s24 >> np.int64(32))),
                ("mul_u24", _u(u24)), ("mulhi_u24", u24 >> u64(32))]
        out += _w64("mad_u64", a * b + X) + _w64("mad_i64", (ia * ib).astype(u64) + X)
        out += _w64("mul64", X * Y)
    den = _where(b == 0, one, b)
    out += [("udiv", a // den), ("urem", a % den)]
    iden = _where((ib == 0) | ((a == INT_MIN) & (ib == -1)), np.int64(1), ib)
    q, rem = _divmod_c(ia, iden)
    out += [("sdiv", _u(q)), ("srem", _u(rem))]
    den64 = Y >> (sel >> u64(26))
    den64 = _where(den64 == 0, one, den64)
    out += _w64("udiv64", X // den64) + _w64("urem64", X % den64)
    out += [("min_i", _u(np.minimum(ia, ib))), ("max_i", _u(np.maximum(ia, ib))),
            ("min_u", np.minimum(a, b)), ("max_u", np.maximum(a, b))]
    si, su = np.sort(np.stack([ia, ib, ic]), axis=0), np.sort(np.stack([a, b, c]), axis=0)
    out += [("med3_i", _u(si[1])), ("med3_u", su[1]), ("min3_i", _u(si[0])),
            ("min3_u", su[0]), ("max3_i", _u(si[2])), ("max3_u", su[2])]
    out.append(("absdiff", np.maximum(a, b) - np.minimum(a, b)))
    for name, bits in (("lt_i", ia < ib), ("lt_u", a < b), ("eq", a == b), ("lt_u64", X < Y),
                       ("lt_i64", X.astype(np.int64) < Y.astype(np.int64))):
        lo, hi = _ballot(bits)
        out += [(name + ".lo", _rows(lo)), (name + ".hi", _rows(hi))]
    s = _where(a & one != 0, b, c)
    s = _where(s < a, _u(s + one), a)
    s = _where(_i(s) < ib, s ^ c, _u(s - b))
    out.append(("select4", _where(s == c, a, s)))
    return out


def _ops_packed(a, b, c, sel) -> List[tuple]:
    import numpy as np

    def sat(lo, hi):
        return lambda f: (lambda *x: np.clip(f(*x), lo, hi))

    def add(x, y):
        return x + y

    def sub(x, y):
        return x - y

    i16, u16 = sat(-0x8000, 0x7FFF), sat(0, 0xFFFF)
    out = [("add16", _pk(add, 16, False, a, b)), ("sub16", _pk(sub, 16, False, a, b)),
           ("add_sat_i16", _pk(i16(add), 16, True, a, b)),
           ("sub_sat_i16", _pk(i16(sub), 16, True, a, b)),
           ("add_sat_u16", _pk(u16(add), 16, False, a, b)),
           ("sub_sat_u16", _pk(u16(sub), 16, False, a, b)),
           ("mul16", _pk(lambda x, y: x * y, 16, False, a, b)),
           ("mad_i16", _pk(lambda x, y, z: x * y + z, 16, True, a, c, b)),
           ("mad_u16", _pk(lambda x, y, z: x * y + z, 16, False, a, b, c)),
           ("min_i16", _pk(np.minimum, 16, True, a, b)),
           ("max_i16", _pk(np.maximum, 16, True, a, b)),
           ("min_u16", _pk(np.minimum, 16, False, a, b)),
           ("max_u16", _pk(np.maximum, 16, False, a, b)),
           ("shl16", _pk(lambda x, y: x << (y & 15), 16, False, a, b)),
           ("lshr16", _pk(lambda x, y: x >> (y & 15), 16, False, a, b)),
           ("ashr16", _pk(lambda x, y: x >> (y & 15), 16, True, a, b))]
    sad8 = sum(np.abs(x - y) for x, y in zip(_parts(a, 8), _parts(b, 8))).astype(np.uint64)
    sad16 = sum(np.abs(x - y) for x, y in zip(_parts(a, 16), _parts(b, 16))).astype(np.uint64)
    out += [("sad_u8", _u(c + sad8)), ("sad_hi_u8", _u(c + (sad8 << np.uint64(16)))),
            ("sad_u16", _u(c + sad16)),
            ("lerp", _pk(lambda x, y, z: (x + y + (z & 1)) >> 1, 8, False, a, b, c))]
    anchor = np.array(ANCHOR, dtype=np.uint64)[(sel >> np.uint64(30)).astype(np.int64)]
    for name, bits, signed in (("sdot4", 8, True), ("udot4", 8, False), ("sdot8", 4, True),
                               ("udot8", 4, False), ("sdot2", 16, True), ("udot2", 16, False)):
        dot = sum(x * y for x, y in zip(_parts(a, bits, signed), _parts(b, bits, signed)))
        out.append((name, _u(dot + c.astype(np.int64))))
        cc = _u(anchor + _sext(c, CLAMP_BITS[bits]))
        lo, hi = (-(1 << 31), INT_MAX) if signed else (0, _M32)
        out.append((name + ".clamp",
                    _u(np.clip(dot + (_i(cc) if signed else cc.astype(np.int64)), lo, hi))))
    return out


def _loop_hash(t):
    import numpy as np

    t = np.asarray(t, dtype=np.uint64).copy()
    h = np.zeros_like(t)
    for _ in range(32):
        live = t != 0
        h = _where(live, _u(h * np.uint64(33) + _ctz(t, 32)), h)
        t &= _u(t - np.uint64(1))
    return h


def _ops_scalar(x, y, z, sel) -> List[tuple]:
    import numpy as np

    u64, one = np.uint64, np.uint64(1)
    Z, W = _cat(z, x), _cat(x ^ u64(INT_MIN), y)
    ix, iy = _i(x), _i(y)
    n, n6 = y & u64(31), y & u64(63)
    out = [("popc", _popc(x)), ("ctz", _ctz(x, 32)), ("clz", _clz(x, 32)), ("brev", _brev(x)),
           ("clrsb", _clrsb(x)), ("popc64", _popc(Z)), ("ctz64", _ctz(Z, 64))]
    with np.errstate(over="ignore"):
        out += [("mul_lo", _u(x * y)), ("mulhi_u", (x * y) >> u64(32)),
                ("mulhi_i", _u((ix * iy) >> np.int64(32)))]
        out += [("shl", _shl(x, n)), ("shr", x >> n), ("sar", _u(ix >> n.astype(np.int64)))]
        out += _w64("shl64", Z << n6) + _w64("shr64", Z >> n6) + _w64("sar64", _sar64(Z, n6))
        out.append(("field_u", (x >> n) & ((one << ((y >> u64(8)) & u64(15))) - one)))
        out.append(("field_i", _u(_i(_shl(x, u64(31) - n))
                                  >> ((y >> u64(16)) & u64(31)).astype(np.int64))))
        out += [("min_i", _u(np.minimum(ix, iy))), ("max_i", _u(np.maximum(ix, iy))),
                ("min_u", np.minimum(x, y)), ("max_u", np.maximum(x, y)),
                ("absdiff", np.maximum(x, y) - np.minimum(x, y))]
        out += [("andn2", x & _u(~y)), ("orn2", x | _u(~y)), ("nand", _u(~(x & y))),
                ("nor", _u(~(x | y))), ("xnor", _u(~(x ^ y)))]
        out += [("sext8", _sext(x, 8)), ("sext16", _sext(x, 16))]
        out += _w64("add64", Z + W) + _w64("sub64", Z - W)
        out += [(f"shl{k}_add", _u(_shl(x, u64(k)) + y)) for k in (1, 2, 3, 4)]
        arms = [_u(x + y), x ^ (y >> u64(3)), _u((x & y) * u64(3)), _u(x - z)]
        out.append(("switch", np.choose((sel & u64(3)).astype(np.int64), arms)))
        out += [("loop", _loop_hash(x)), ("loop2", _loop_hash(x & _u(x - one)))]
    return out


def wave_masks(seed: int, r):
    """(m1, m2, u(3) & 63) of the scalar stage's wave-mask block in rounds
    ``r``: uint64 [rounds]."""
    import numpy as np

    _, base = _base_of(int(seed) & _M32, 3, r)
    lane = np.arange(64, dtype=np.uint32)[None, :]
    v = [_word(base[:, None], np.uint32(64 * k) + lane) for k in range(3)]
    m = []
    for bits in (v[0] < v[1], (v[2] & np.uint32(1)) != 0):
        lo, hi = _ballot(bits)
        m.append(_cat(hi, lo))
    return m[0], m[1], _u(_word(base, 64 * 3)) & np.uint64(63)


def _mask_block(seed: int, r) -> List[tuple]:
    import numpy as np

    m1, m2, n = wave_masks(seed, r)
    masks = (("m1", m1), ("m2", m2), ("andn", m1 & ~m2), ("xor", m1 ^ m2))
    out = [row for name, m in masks for row in _w64(name, m)]
    for name, m in masks:
        out += [(name + ".popc", _popc(m)), (name + ".ctz", _ctz(m, 64)),
                (name + ".clz", _clz(m, 64))]
    return out + _w64("m1.shl", m1 << n) + _w64("m1.sar", _sar64(m1, n))


_VECTOR_OPS = (_ops_bits, _ops_arith, _ops_packed)


def _stage(seed: int, stage: int, r) -> List[tuple]:
    """[(slot name, uint32 [rounds, 64])] of a stage for rounds ``r``
    (uint32 array), in slot order."""
    import numpy as np

    if stage not in range(len(STAGES)):
        raise ValueError(f"intcheck: stage {stage} out of range 0..3")
    out = []
    for j in range(GROUPS):
        if stage < 3:
            rows = _VECTOR_OPS[stage](*operands(seed, stage, r, j))
        else:
            rows = [(name, _rows(v)) for name, v in _ops_scalar(*scalar_operands(seed, r, j))]
        out += [(f"{j}.{name}", v) for name, v in rows]
    if stage == 3:
        out += [(name, _rows(v)) for name, v in _mask_block(seed, r)]
    return [(name, np.asarray(v).astype(np.uint32)) for name, v in out]


def slot_table(stage: int) -> List[str]:
    """The name of every result slot of a stage, in slot order."""
    return [name for name, _ in _stage(0, int(stage), _shared.one_round("intcheck", 0))]


def reference_values(seed: int, stage: int, r: int):
    """What a wave folds in one stage and round: {slot name: uint32[64]},
    in slot order, exact per lane."""
    slots = _stage(int(seed) & _M32, int(stage), _shared.one_round("intcheck", r))
    return {name: v[0] for name, v in slots}


def reference_digests(seed: int, rounds: int):
    """Expected digests as uint32[rounds, 4], columns in STAGES order:
    min(rounds, PERIOD) rows are computed and tiled.

    Pure numpy: needs neither torch nor a GPU.  This is the definition
    the GPU kernel is tested against."""
    import numpy as np

    seed = int(seed) & _M32
    rounds = int(rounds)
    if rounds < 0:
        raise ValueError("reference_digests: rounds >= 0 required")
    n = min(rounds, PERIOD)
    rows = np.empty((n, len(STAGES)), dtype=np.uint32)
    r = np.arange(n, dtype=np.uint32)
    if n:
        for s in range(len(STAGES)):
            rows[:, s] = _digest(_stage(seed, s, r))
    return _shared.tile_period(rows, rounds, PERIOD)


# -- GPU run ---------------------------------------------------------------------

@dataclass
class IntcheckResult(DigestResult):
    # Whole-run lower bounds per stage in 1e9 lane-level integer
    # operations per second (the kernel's time also holds operand
    # generation, the other stages and the digests): informative.
    bits_gops: float = 0.0
    arith_gops: float = 0.0
    packed_gops: float = 0.0
    scalar_gops: float = 0.0


def intcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> IntcheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup asks for a CU's whole LDS without touching it, so on an
    idle GPU the default grid lands one workgroup on every CU;
    ``cus_covered`` reports how many distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot break an
    adder."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"intcheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"intcheck: blocks must be in 0..4096, got {blocks}")
    return _shared.run_probe(
        "intcheck", IntcheckResult(rounds=rounds), STAGES, _OPS_PER_WAVE_ROUND, 1e9,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected)


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``intcheck`` with its dump pointer set."""
    return _shared.wave_digests(
        "intcheck", _ext().intcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device)


def wave_values(seed: int, stage: int, r: int, device=None):
    """What one wave folded for a stage and round, shaped like
    ``reference_values``: {slot name: uint32[64]}.  A digest cannot say
    which op went wrong; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    names = slot_table(stage)
    with torch.cuda.device(_device(device)):
        raw = _ext().intcheck_values(int(seed), stage, int(r)).cpu().numpy()
    return _shared.value_rows("intcheck", raw.view(np.uint32), names, _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def run_intcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                            timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the intcheck CLI."""
    return _active.run_probe_subprocess("intcheck", index, "--rounds", rounds, timeout_s)


def intcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                   rounds: int = DEFAULT_ROUNDS,
                   max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("intcheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "intcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: intcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
