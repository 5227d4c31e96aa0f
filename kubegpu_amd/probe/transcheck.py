"""Active probe for the transcendental units — wrapper over the transcheck
HIP kernel.

Every SIMD has one quarter-rate transcendental pipe: v_exp, v_log, v_rcp,
v_rsq, v_sqrt, v_sin, v_cos.  Softmax, SiLU / GELU, RMSNorm and rotary
embeddings all pass through it.  ``fpcheck`` reaches it only through the
seeds of its division and square-root sequences, whose correction steps
absorb exactly the low-order errors a damaged table entry or a stuck
significand bit would make; no other probe issues these instructions, and
no ECC counter moves when they go wrong.

IEEE 754 does not define their results, so numpy cannot say what v_exp_f32
must return bit for bit.  The results are deterministic though: every SIMD
of a healthy chip returns the same bits for the same input.  ``transcheck()``
therefore works in two steps per call:

  1 golden     one workgroup (``golden_values``) runs the workload of all
               PERIOD rounds and stores every raw result.  ``check_values``
               compares each with a high-precision reference (numpy float64
               for f32 and f16 results, ``numpy.longdouble`` for f64) under
               the bound of its operation (BOUNDS), or with the class of
               the mathematical result on special inputs.  This catches a
               unit that is wrong everywhere and a golden wave that is bad.
  2 consensus  ``fold_values`` folds the golden values into the [PERIOD, 4]
               digest table, which goes to the digest kernel as its
               expected table: one 16-wave workgroup per compute unit, every
               wave recomputes every round and compares four digests bit
               for bit.  A SIMD that differs in the last bit is named by
               XCD / SE / SH / CU / SIMD in ``records``, as in the siblings.

``ok`` needs zero golden violations and zero digest mismatches;
``mismatches`` is their sum, ``golden_errors`` and ``digest_mismatches`` the
parts.  The consensus pass runs whatever the golden pass found.  Where
digests differ, the rounds of one period up to the first bad one are run
once more with the digest dump set (at most 8 MiB at the default grid) and
``waves_disagreeing`` counts the waves that differ from the table in that
round; more than half of all waves sets ``golden_suspect``: the
golden wave, not the others, is then the one to distrust.

The workload (csrc/transcheck.hip; ``operands``, ``reference_values`` and
``fold_values`` are the definition).  ``fmix32``, ``base``, ``salt`` are
cucheck's, the stage number fed to ``base`` is 56 + s, and inputs repeat
with PERIOD = 128 rounds:

  word(s, r, idx) = fmix32(base(seed, 56 + s, r % PERIOD) + idx)

pack(s, e, m) is sign, biased exponent field, mantissa field; S, E, M take
a raw word apart the same way.  Operands are put together from those fields
with integer operations only.  A *slot* is q = 64 j + lane.

Stage 0, ``f32``: 8 slots per lane; exp2, log2, rcp, rsq, sqrt, sin, cos
(sin and cos take revolutions) on the slot's operand, made from ra = word
2 q and sel = word 2 q + 1 by recipe (lane + j + r) mod 8:

  0 normal    pack(S, 1 + E mod 254, M): the whole normal range
  1 exp-arg   sel & 1: an exact integer, pack(S, 127 + n, M with its low
              23 - n bits cleared), n = E mod 7; else pack(S, 117 + E mod
              17, M), |x| in [2**-10, 128): arguments of exp2 from -128 to
              128 with random fraction bits
  2 near-one  1.0 + d or 1.0 - d (sel bit 5) in the bit pattern, d = (2**23
              | M) >> k, k = 1 + (sel & 31) mod 20: within 2**-1 .. 2**-20
              of 1.0 on either side, where log cancels
  3 revs      sel & 3 = 0: pack(S, 114 + E mod 21, M), |x| in [2**-13, 256);
              else n / 8 for n = 1 + (ra & 2047), that is every multiple of
              1/8 and 1/4 up to 256.0, exactly (1), one step above (2) and
              one below (3)
  4 pow2      pack(S, e, 0), e = 1 + E mod 253, forced odd where sel & 1
              (the powers of four)
  5 subnormal pack(S, 0, (M >> (sel & 15)) | 1)
  6 large     pack(S, 136 + E mod 118, M), |x| >= 512: outside the domain
              of sin and cos, exp2 overflows or underflows
  7 special   by code (sel >> 16) & 7: 0, 5 zero; 1, 6 Inf; 2 NaN; 3 one;
              4, 7 pack(S, 119 + (E & 15), M); sign kept, so negative
              inputs reach log, sqrt and rsq here and in every recipe but 2

Stage 1, ``f16``, exhaustive: 8 slots per lane and the same seven
operations; the slot's operand is f16 code perm(512 (r mod 128) + 64 j +
lane), perm(i) = ((40503 i) mod 2**16) ^ 0xA5C3, a bijection of 0..65535
that does not depend on the seed.  One period feeds every f16 bit pattern
to every f16 operation exactly once; that fixes PERIOD.

Stage 2, ``f64``: 4 slots per lane; rcp, rsq, sqrt — the approximation
instructions, not the correctly rounded results fpcheck checks — on ra =
words 4 q, 4 q + 1 (low, high) and sel = word 4 q + 2, the same families:
0 pack(S, 1 + E mod 2046, M); 1 pack(S, 1015 + (E & 15), M); 2 1.0 +- ((2**52
| M) >> k), k = 1 + (sel & 63) mod 40, minus where sel bit 6; 3 pack(S, 1023
+ (E & 7), M with its low 40 bits cleared); 4 pack(S, e, 0), e = 1 + E mod
2045, odd where sel & 1; 5 pack(S, 0, (M >> (sel & 31)) | 1); 6 pack(S, 1 +
(E & 7), M) where sel & 1, else pack(S, 2046 - (E & 7), M); 7 the special
codes with pack(S, 1015 + (E & 15), M).  A result takes two rows, ``.lo``
then ``.hi``.

Stage 3, ``chain``: 2 groups j per lane of dependent sequences as
workloads issue them, per lane, in f32 unless said; contraction is off, so
every product and sum rounds on its own.  w_i = word 8 q + i, at(w, lo, n) =
pack(S w, lo + E w mod n, M w); L, K, C, EPS are the f32 nearest log2 e,
2 sqrt(2 / pi), 0.044715 and 1e-6 (CONST holds their bits):

  x = at(w_0, 124, 6), 1/8 <= |x| < 8
  sigmoid.exp = exp2(-x L); sigmoid = rcp(1 + sigmoid.exp)
  gelu.exp = exp2(-u L), u = K (x + C x x x); gelu.rcp = rcp(1 + gelu.exp);
      gelu = x gelu.rcp: the tanh form, written as x sigmoid(2 t) so that
      nothing cancels
  rms.rsq = rsq(x x + EPS); rms = x rms.rsq
  a, b = at(w_1, 125, 6), at(w_2, 125, 6); m = max(a, b); lse.exp_a =
      exp2(a - m), lse.exp_b = exp2(b - m); lse.log = log2(lse.exp_a +
      lse.exp_b); lse = m + lse.log
  t = at(w_3, 117, 10) revolutions, rx, ry = at(w_4, 125, 4), at(w_5, 125,
      4); rot.cos = cos t, rot.sin = sin t; rot.x = rx cos - ry sin, rot.y =
      rx sin + ry cos
  softmax16 = exp2((h0 - max(h0, h1)) L16) in f16, h0, h1 from the low and
      high half of w_6 as pack16(S, 12 + E mod 6, M), L16 = 0x3DC5
  prng.0 .. 7: eight dependent steps of v_prng_b32 from w_7, D = (S << 1)
      ^ (0xC5 where S bit 31 is set) mod 2**32; exact, compared as such

Error measure of the golden compare (BOUNDS, in units of it):

  exp2, rcp, rsq, sqrt and the chains built only from them: |got - ref| in
      ulps of the format at ref
  log2, sin, cos and the chains that hold one (lse.log, lse, rot.*): |got -
      ref| in ulps of the format at max(|ref|, 1), since these results cross
      zero, where a relative measure means nothing

The bound applies where input and reference are finite and normal, the
reference lies at least four binades inside the format's range and, for sin
and cos, |x| <= 256; in the second measure a reference of exactly 0 (sin at
whole revolutions, log2(1)) is bounded too.  On special inputs (zero, Inf, NaN of either sign,
negative inputs to log2, rsq and sqrt) the class of the result — +0, -0,
+Inf, -Inf, NaN, finite of either sign; NaN without sign — must equal that
of the mathematical function: exp2(-Inf) = +0, log2(+-0) = -Inf, log2(x < 0)
= NaN, rcp(+-0) = +-Inf, rsq(+0) = +Inf, rsq(-0) = -Inf, sqrt(-0) = -0,
sin(+-0) = +-0, sin(Inf) = NaN.  Everything else — subnormal inputs and
results, results in the outermost binades, NaN payloads, sin and cos out of
their domain — is consensus-only: the golden wave defines it and every wave
must agree.

BOUNDS were measured on an MI355X (profiles/transcheck_mi355x.json): the
largest error of each operation over all PERIOD rounds of seeds 0 and
0xDEADBEEF against ``reference_values``, doubled and rounded up to a power
of two, at least 1.  The bound only has to catch gross damage on the golden
wave — consensus catches everything finer — and the factor keeps a part
whose microcode differs in the last place from raising an alarm.  A bound
of 2**b in a format with p significand bits still protects the leading p -
b, the hidden one included; ``protected_bits`` counts the stored ones a flip
of which the bound always catches, p - b - 2, one fewer for sin and cos,
whose results lie below 1 where the measure's ulp is that of 1.  Largest
measured error -> bound (significand bits still protected, of 24, 11, 53):

  f32    exp2 0.76, log2 1.00, rcp 0.85, rsq 0.80, sqrt 0.88, sin 0.97 -> 2
         (23); cos 1.02 -> 4 (22)
  f16    every operation at most 0.4999: correctly rounded on all 65,536
         inputs -> 1 (11)
  f64    rcp 2.42e8, rsq 2.35e8, sqrt 1.64e8 -> 2**29 (24)
  chain  sigmoid.exp 5.6, sigmoid 6.1 -> 16 (20); gelu.exp 110, gelu.rcp 90,
         gelu 107 -> 256 (16); rms.rsq 1.4 -> 4 (22); rms 2.2 -> 8 (21);
         lse.exp_a, _b 11.4 -> 32 (19); lse.log 1.1, lse 1.5, rot.cos 1.02 ->
         4 (22); rot.sin 0.95 -> 2 (23); rot.x, rot.y 4.3 -> 16 (20); softmax16
         7.9 -> 16 (7); prng exact
  (the chains' errors include the rounding of the exp2 argument, which the
  reference, a function of the inputs alone, does not make)

No class rule had to be bent: the hardware returned the class of the
mathematical result on every special input of both seeds, and v_prng_b32
matched the formula above on every element.

Not covered: rounding modes other than nearest-even, the library functions
the compiler builds around these instructions, fp8 and bf16 conversions,
cross-lane softmax reductions, v_exp_legacy / v_log_legacy, v_frexp / v_ldexp.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.transcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
import time
from dataclasses import dataclass, field
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
    _salt,
    metric_args,
)

STAGES: Tuple[str, ...] = ("f32", "f16", "f64", "chain")
PERIOD = 128  # inputs of round r are those of round r % PERIOD
_STAGE0 = 56  # stage number fed to base() is _STAGE0 + s
SLOTS_PER_LANE: Tuple[int, ...] = (8, 8, 4, 2)
_UNARY = ("exp2", "log2", "rcp", "rsq", "sqrt", "sin", "cos")
OPS: Tuple[Tuple[str, ...], ...] = (
    _UNARY, _UNARY, ("rcp", "rsq", "sqrt"),
    ("sigmoid.exp", "sigmoid", "gelu.exp", "gelu.rcp", "gelu", "rms.rsq", "rms",
     "lse.exp_a", "lse.exp_b", "lse.log", "lse", "rot.cos", "rot.sin", "rot.x", "rot.y",
     "softmax16") + tuple(f"prng.{i}" for i in range(8)),
)
CONST = {"log2e": 0x3FB8AA3B, "gelu_2k": 0x3FCC422A, "gelu_c3": 0x3D372713,
         "eps": 0x358637BD, "log2e_f16": 0x3DC5}
_VALUE_ROWS = 64
_ROUND_WORDS = 64 * _VALUE_ROWS + 1

# format -> (exponent bits, mantissa bits)
_FORMATS = {"f16": (5, 10), "f32": (8, 23), "f64": (11, 52)}
# operations measured at max(|ref|, 1)
_ABSOLUTE = {"log2", "sin", "cos", "lse.log", "lse", "rot.cos", "rot.sin", "rot.x", "rot.y"}
SIN_COS_DOMAIN = 256.0  # revolutions

# Largest |got - ref| the golden wave may show, per stage and operation, in
# the module docstring's measure.  Measured maxima and these values:
# profiles/transcheck_mi355x.json.
BOUNDS: Dict[str, Dict[str, float]] = {
    "f32": {"exp2": 2, "log2": 2, "rcp": 2, "rsq": 2, "sqrt": 2, "sin": 2, "cos": 4},
    "f16": {"exp2": 1, "log2": 1, "rcp": 1, "rsq": 1, "sqrt": 1, "sin": 1, "cos": 1},
    "f64": {"rcp": 2 ** 29, "rsq": 2 ** 29, "sqrt": 2 ** 29},
    "chain": {"sigmoid.exp": 16, "sigmoid": 16, "gelu.exp": 256, "gelu.rcp": 256, "gelu": 256,
              "rms.rsq": 4, "rms": 8, "lse.exp_a": 32, "lse.exp_b": 32, "lse.log": 4, "lse": 4,
              "rot.cos": 4, "rot.sin": 2, "rot.x": 16, "rot.y": 16, "softmax16": 16,
              **{f"prng.{i}": 0 for i in range(8)}},  # exact
}
# operations whose results lie below 1 while their measure's ulp is that of 1
_BELOW_ONE = {"sin", "cos", "rot.cos", "rot.sin", "lse.log"}

# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/transcheck_mi355x.json), default grid (256
# workgroups, 4096 waves): 29.23, 28.10 and 27.81 us per round at 256, 1024
# and 4096 rounds (the fixed cost of a launch fades), so 0.5 s are about
# 17,980 rounds; 138 x 128 = 17664 rounds took 0.489 s.  The golden
# pass (four one-workgroup launches, the compare and the fold of one
# period) adds 0.05 s whatever the rounds.
DEFAULT_ROUNDS = 17664

# transcendental instructions one wave issues per round, per stage, lane-level
_OPS_PER_WAVE_ROUND = (64 * 8 * 7, 64 * 8 * 7, 64 * 4 * 3, 64 * 2 * 19)

_M32 = 0xFFFFFFFF


def _format_of(stage: int, op: str) -> str:
    if stage == 3:
        return "f16" if op == "softmax16" else "f32"
    return ("f32", "f16", "f64")[stage]


def protected_bits(stage: int, op: str) -> int:
    """Leading stored significand bits of a result of ``op`` a flip of
    which ``check_values`` always rejects (module docstring)."""
    import math

    bound = BOUNDS[STAGES[stage]][op]
    mbits = _FORMATS[_format_of(stage, op)][1]
    return mbits - int(math.log2(bound)) - (2 if op in _BELOW_ONE else 1)


# -- operands (integer operations only) ------------------------------------------------

def _u(x):
    import numpy as np

    return np.uint64(x)


def _pack(fmt: str, s, e, m):
    eb, mb = _FORMATS[fmt]
    return (s << _u(eb + mb)) | (e << _u(mb)) | m


def _split(fmt: str, x):
    eb, mb = _FORMATS[fmt]
    return (x >> _u(eb + mb)) & _u(1), (x >> _u(mb)) & _u((1 << eb) - 1), x & _u((1 << mb) - 1)


def _special(fmt: str, s, e, m, code):
    import numpy as np

    eb, _ = _FORMATS[fmt]
    X, B = (1 << eb) - 1, (1 << (eb - 1)) - 1
    zero = _u(0)
    return np.select(
        [(code == 0) | (code == 5), (code == 1) | (code == 6), code == 2, code == 3],
        [_pack(fmt, s, zero, zero), _pack(fmt, s, _u(X), zero), _pack(fmt, s, _u(X), m | _u(1)),
         _pack(fmt, s, _u(B), zero)],
        _pack(fmt, s, _u(B - 8) + (e & _u(15)), m))


def _operand32(k, ra, sel):
    """The f32 operand of recipe ``k`` (an array like the words) as uint64
    bit patterns."""
    import numpy as np

    s, e, m = _split("f32", ra)
    zero, one = _u(0), _u(1)
    n7 = e % _u(7)
    r1 = np.where(sel & one != 0,
                  _pack("f32", s, _u(127) + n7, m & ~((one << (_u(23) - n7)) - one)),
                  _pack("f32", s, _u(117) + e % _u(17), m))
    step = ((one << _u(23)) | m) >> (one + (sel & _u(31)) % _u(20))
    r2 = np.where((sel >> _u(5)) & one != 0, _u(0x3F800000) - step, _u(0x3F800000) + step)
    n = one + (ra & _u(2047))
    top = sum((n >> _u(i) != 0).astype(np.uint64) for i in range(1, 12))
    x8 = _pack("f32", s, _u(124) + top, (n << (_u(23) - top)) & _u(0x7FFFFF))
    v = sel & _u(3)
    r3 = np.select([v == 0, v == 1, v == 2],
                   [_pack("f32", s, _u(114) + e % _u(21), m), x8, x8 + one], x8 - one)
    ex = one + e % _u(253)
    return np.choose(np.asarray(k).astype(np.int64), [
        _pack("f32", s, one + e % _u(254), m), r1, r2, r3,
        _pack("f32", s, np.where(sel & one != 0, ex | one, ex), zero),
        _pack("f32", s, zero, (m >> (sel & _u(15))) | one),
        _pack("f32", s, _u(136) + e % _u(118), m),
        _special("f32", s, e, m, (sel >> _u(16)) & _u(7))])


def _operand64(k, ra, sel):
    import numpy as np

    s, e, m = _split("f64", ra)
    zero, one, unit = _u(0), _u(1), _u(0x3FF0000000000000)
    step = ((one << _u(52)) | m) >> (one + (sel & _u(63)) % _u(40))
    ex = one + e % _u(2045)
    return np.choose(np.asarray(k).astype(np.int64), [
        _pack("f64", s, one + e % _u(2046), m),
        _pack("f64", s, _u(1015) + (e & _u(15)), m),
        np.where((sel >> _u(6)) & one != 0, unit - step, unit + step),
        _pack("f64", s, _u(1023) + (e & _u(7)), m & ~((one << _u(40)) - one)),
        _pack("f64", s, np.where(sel & one != 0, ex | one, ex), zero),
        _pack("f64", s, zero, (m >> (sel & _u(31))) | one),
        np.where(sel & one != 0, _pack("f64", s, one + (e & _u(7)), m),
                 _pack("f64", s, _u(2046) - (e & _u(7)), m)),
        _special("f64", s, e, m, (sel >> _u(16)) & _u(7))])


def _rounds(r):
    import numpy as np

    r = np.atleast_1d(np.asarray(r, dtype=np.int64))
    if r.ndim != 1 or (r < 0).any() or (r >= 65536).any():
        raise ValueError("transcheck: rounds must be in 0..65535")
    return (r % PERIOD).astype(np.uint32)


def f16_codes(r):
    """The f16 bit patterns stage 1 feeds its operations in rounds ``r`` (an
    int or an array): uint64 [rounds, 8, 64]."""
    import numpy as np

    rp = _rounds(r).astype(np.uint64)
    i = (_u(512) * rp[:, None, None] + _u(64) * np.arange(8, dtype=np.uint64)[None, :, None]
         + np.arange(64, dtype=np.uint64)[None, None, :])
    return ((i * _u(40503)) & _u(0xFFFF)) ^ _u(0xA5C3)


def _words(seed: int, stage: int, rp, per_slot: int, count: int):
    """word(stage, r, per_slot * q + i) for i < count as uint64 arrays
    [rounds, slots, 64]."""
    import numpy as np

    base = _base(int(seed) & _M32, _STAGE0 + stage, rp)[:, None, None]
    q = (np.uint32(64) * np.arange(SLOTS_PER_LANE[stage], dtype=np.uint32)[None, :, None]
         + np.arange(64, dtype=np.uint32)[None, None, :])
    with np.errstate(over="ignore"):
        return [_fmix32(base + np.uint32(per_slot) * q + np.uint32(i)).astype(np.uint64)
                for i in range(count)]


def _recipe(stage: int, rp):
    import numpy as np

    j = np.arange(SLOTS_PER_LANE[stage], dtype=np.uint32)[None, :, None]
    return (np.arange(64, dtype=np.uint32)[None, None, :] + j + rp[:, None, None]) % np.uint32(8)


def operands(seed: int, stage: int, r):
    """The operand bit patterns of ``stage`` in rounds ``r`` (an int or an
    array), uint64 [rounds, slots per lane, 64]; for the chain stage a dict
    of such arrays by input name (x, a, b, t, rx, ry, h0, h1, p)."""
    stage, rp = int(stage), _rounds(r)
    if stage == 0:
        ra, sel = _words(seed, 0, rp, 2, 2)
        return _operand32(_recipe(0, rp), ra, sel)
    if stage == 1:
        return f16_codes(rp)
    if stage == 2:
        lo, hi, sel = _words(seed, 2, rp, 4, 3)
        return _operand64(_recipe(2, rp), lo | (hi << _u(32)), sel)
    if stage != 3:
        raise ValueError(f"transcheck: stage {stage} out of range 0..3")
    w = _words(seed, 3, rp, 8, 8)

    def at(x, lo, n):
        s, e, m = _split("f32", x)
        return _pack("f32", s, _u(lo) + e % _u(n), m)

    def at16(h):
        s, e, m = _split("f16", h & _u(0xFFFF))
        return _pack("f16", s, _u(12) + e % _u(6), m)

    return {"x": at(w[0], 124, 6), "a": at(w[1], 125, 6), "b": at(w[2], 125, 6),
            "t": at(w[3], 117, 10), "rx": at(w[4], 125, 4), "ry": at(w[5], 125, 4),
            "h0": at16(w[6]), "h1": at16(w[6] >> _u(16)), "p": w[7]}


# -- the reference -----------------------------------------------------------------

def _floats(fmt: str, bits):
    """Bit patterns (uint64) as floats of the format."""
    import numpy as np

    it, ft = {"f16": (np.uint16, np.float16), "f32": (np.uint32, np.float32),
              "f64": (np.uint64, np.float64)}[fmt]
    return np.ascontiguousarray(np.asarray(bits).astype(it)).view(ft)


def _turns(x, f):
    """sin or cos of x revolutions: the whole turns leave x exactly."""
    import numpy as np

    y = f(2.0 * np.pi * (x - np.rint(x)))
    return np.where(x == 0, x, y) if f is np.sin else y


def _unary(x, ops):
    """[rounds, slots, ops, 64]: the mathematical results on x (float64 or
    longdouble), not rounded to any format."""
    import numpy as np

    with np.errstate(all="ignore"):
        f = {"exp2": np.exp2, "log2": np.log2, "rcp": lambda v: 1 / v,
             "rsq": lambda v: 1 / np.sqrt(v), "sqrt": np.sqrt,
             "sin": lambda v: _turns(v, np.sin), "cos": lambda v: _turns(v, np.cos)}
        return np.stack([f[op](x) for op in ops], axis=2)


def prng_step(s):
    """v_prng_b32 on uint64 arrays holding u32."""
    return ((s << _u(1)) & _u(_M32)) ^ (((s >> _u(31)) & _u(1)) * _u(0xC5))


def _chain(o):
    import numpy as np

    f32 = {k: float(_floats("f32", np.array([v]))[0]) for k, v in CONST.items() if k != "log2e_f16"}
    L, L16 = f32["log2e"], float(_floats("f16", np.array([CONST["log2e_f16"]]))[0])
    x, a, b, t, rx, ry = (_floats("f32", o[k]).astype(np.float64)
                          for k in ("x", "a", "b", "t", "rx", "ry"))
    h0, h1 = (_floats("f16", o[k]).astype(np.float64) for k in ("h0", "h1"))
    out = {}
    out["sigmoid.exp"] = np.exp2(-x * L)
    out["sigmoid"] = 1 / (1 + out["sigmoid.exp"])
    out["gelu.exp"] = np.exp2(-f32["gelu_2k"] * (x + f32["gelu_c3"] * x * x * x) * L)
    out["gelu.rcp"] = 1 / (1 + out["gelu.exp"])
    out["gelu"] = x * out["gelu.rcp"]
    out["rms.rsq"] = 1 / np.sqrt(x * x + f32["eps"])
    out["rms"] = x * out["rms.rsq"]
    m = np.maximum(a, b)
    out["lse.exp_a"], out["lse.exp_b"] = np.exp2(a - m), np.exp2(b - m)
    out["lse.log"] = np.log2(out["lse.exp_a"] + out["lse.exp_b"])
    out["lse"] = m + out["lse.log"]
    c, s = _turns(t, np.cos), _turns(t, np.sin)
    out["rot.cos"], out["rot.sin"] = c, s
    out["rot.x"], out["rot.y"] = rx * c - ry * s, rx * s + ry * c
    out["softmax16"] = np.exp2((h0 - np.maximum(h0, h1)) * L16)
    p = o["p"]
    for i in range(8):
        p = prng_step(p)
        out[f"prng.{i}"] = p.astype(np.float64)
    return np.stack([out[op] for op in OPS[3]], axis=2)


def reference_values(seed: int, stage: int, r):
    """The mathematical results of ``stage`` in rounds ``r`` (an int or an
    array), [rounds, slots per lane, operations, 64] in OPS order: float64,
    longdouble for the f64 stage; never rounded to the format."""
    import numpy as np

    stage = int(stage)
    o = operands(seed, stage, r)
    if stage == 3:
        return _chain(o)
    with np.errstate(invalid="ignore"):  # NaN operands
        x = _floats(("f32", "f16", "f64")[stage], o).astype(
            np.longdouble if stage == 2 else np.float64)
    return _unary(x, OPS[stage])


# -- rows, typed values, the fold --------------------------------------------------------

def slot_table(stage: int) -> List[str]:
    """The name of every row of a stage, in the kernel's order."""
    names = [f"{j}.{op}" for j in range(SLOTS_PER_LANE[stage]) for op in OPS[stage]]
    return [n + h for n in names for h in (".lo", ".hi")] if stage == 2 else names


def _raw(stage: int, values):
    """uint32 [rounds, rows, 64] from that, from [rows, 64] or from what
    ``wave_values`` returns."""
    import numpy as np

    if isinstance(values, dict):
        values = np.stack([values[n] for n in slot_table(stage)])
    values = np.asarray(values, dtype=np.uint32)
    values = values[None] if values.ndim == 2 else values
    if values.shape[1:] != (len(slot_table(stage)), 64):
        raise ValueError(f"transcheck: stage {stage} has {len(slot_table(stage))} rows of 64, "
                         f"got {values.shape}")
    return values


def _typed(stage: int, raw):
    """Result bit patterns, uint64 [rounds, slots, operations, 64]."""
    import numpy as np

    raw = raw.astype(np.uint64)
    if stage == 2:
        raw = raw[:, 0::2] | (raw[:, 1::2] << _u(32))
    return raw.reshape(raw.shape[0], SLOTS_PER_LANE[stage], len(OPS[stage]), 64)


def fold_values(stage: int, values):
    """The digests of a stage from its values (``_raw`` says in which
    shapes), uint32 [rounds]: sum over rows n and lanes l of fmix32(value
    + salt(64 n + l)), the kernel's fold."""
    import numpy as np

    raw = _raw(int(stage), values)
    n = np.arange(raw.shape[1] * 64, dtype=np.uint32).reshape(1, raw.shape[1], 64)
    with np.errstate(over="ignore"):
        return _fmix32(raw + _salt(n)).sum(axis=(1, 2), dtype=np.uint32)


# -- the golden compare ----------------------------------------------------------------

def _classes(x):
    """0 +0, 1 -0, 2 +Inf, 3 -Inf, 4 NaN, 5 / 6 finite positive / negative."""
    import numpy as np

    kind = np.select([np.isnan(x), x == 0, np.isinf(x)], [4, 0, 2], 5)
    return np.where(kind == 4, 4, kind + np.signbit(x))


def _compare(stage: int, r, got, seed: int):
    """(rounds, operands, result bits, reference, error where a bound
    applies and NaN elsewhere, class violations) of ``got``; the arrays are
    [rounds, slots, operations, 64]."""
    import numpy as np

    rp = _rounds(r)
    bits = _typed(stage, _raw(stage, got))
    if bits.shape[0] != len(rp):
        raise ValueError(f"transcheck: {len(rp)} rounds, values of {bits.shape[0]}")
    ref = reference_values(seed, stage, rp)
    o = operands(seed, stage, rp)
    wrong_class = np.zeros(bits.shape, dtype=bool)
    err = np.full(bits.shape, np.nan)
    with np.errstate(all="ignore"):
        for k, op in enumerate(OPS[stage]):
            g_bits, want = bits[:, :, k], ref[:, :, k]
            if op.startswith("prng"):
                err[:, :, k] = np.abs(g_bits.astype(np.float64) - want)
                continue
            fmt = _format_of(stage, op)
            eb, mb = _FORMATS[fmt]
            bias = (1 << (eb - 1)) - 1
            g = _floats(fmt, g_bits).astype(want.dtype)
            _, ex = np.frexp(np.abs(want))  # |want| = m 2**ex, 0.5 <= m < 1
            inside = (ex - 1 >= 5 - bias) & (want != 0)
            if op in _ABSOLUTE:  # measured at max(|ref|, 1): a reference of 0 is as good
                inside |= want == 0
            bounded = np.isfinite(want) & inside & (ex - 1 <= bias - 4)
            if stage != 3:  # the chains' inputs are all normal
                _, e_, m_ = _split(fmt, o)
                special = ((e_ == 0) & (m_ == 0)) | (e_ == (1 << eb) - 1) | np.isnan(want)
                special &= (e_ != 0) | (m_ == 0)  # subnormal inputs are consensus-only
                bounded &= ~special & (e_ != 0)
                if op in ("sin", "cos"):
                    bounded &= np.abs(_floats(fmt, o).astype(want.dtype)) <= SIN_COS_DOMAIN
                wrong_class[:, :, k] = special & (_classes(g) != _classes(want))
            scale = np.maximum(ex - 1, 0) if op in _ABSOLUTE else ex - 1
            e_k = np.abs(g - want) / np.ldexp(np.ones_like(want), scale - mb)
            e_k = np.where(np.isfinite(g), e_k, np.inf).astype(np.float64)
            err[:, :, k] = np.where(bounded, e_k, np.nan)
    return rp, o, bits, ref, err, wrong_class


def _violations(stage: int, r, got, seed: int, limit: Optional[int]):
    """(number of violations, records of the first ``limit``) of
    ``check_values``: a unit that is wrong everywhere gives more than a
    million, which are counted, not listed."""
    import numpy as np

    rp, o, bits, ref, err, wrong_class = _compare(stage, r, got, seed)
    bound = np.array([BOUNDS[STAGES[stage]][op] for op in OPS[stage]], dtype=np.float64)
    with np.errstate(invalid="ignore"):
        bad = wrong_class | (err > bound[None, None, :, None])
    out = []
    for i, j, k, lane in np.argwhere(bad)[:limit]:
        operand = ({n: hex(int(v[i, j, lane])) for n, v in o.items()} if stage == 3
                   else hex(int(o[i, j, lane])))
        e = err[i, j, k, lane]
        out.append({"stage": STAGES[stage], "op": OPS[stage][k], "round": int(rp[i]),
                    "slot": int(j), "lane": int(lane), "operand": operand,
                    "got": hex(int(bits[i, j, k, lane])),
                    "reference": repr(float(ref[i, j, k, lane])),
                    "error": "class" if np.isnan(e) else float(e)})
    return int(bad.sum()), out


def check_values(stage: int, r, got, seed: int = 0, limit: Optional[int] = None) -> List[dict]:
    """The violations of the module docstring's bounds and class rules in
    ``got``, the values of ``stage`` in rounds ``r`` (an int or an array;
    ``got`` in the shapes ``_raw`` takes), at most ``limit`` of them.  Each
    names stage, operation, round, slot, lane, operand bits, got bits, the
    reference and the error (in the operation's measure, or "class")."""
    return _violations(int(stage), r, got, seed, limit)[1]


def max_errors(stage: int, r, got, seed: int = 0) -> Dict[str, float]:
    """The largest error per operation of ``got`` where a bound applies, in
    the operation's measure: what BOUNDS was set from."""
    import numpy as np

    err = _compare(int(stage), r, got, seed)[4]
    worst = np.nanmax(np.where(np.isnan(err), 0.0, err), axis=(0, 1, 3))
    return {op: float(w) for op, w in zip(OPS[stage], worst)}


# -- GPU run ---------------------------------------------------------------------

def decode_hw(hw: int) -> dict:
    """Where a wave ran, from xcc << 16 | HW_ID[15:0]."""
    rec = _shared.decode_record((0, hw, 0, 0, 0, 0), STAGES)
    return {k: rec[k] for k in ("xcc", "se", "sh", "cu", "simd")}


def golden_values(seed: int, device=None):
    """The golden pass on the GPU: ([uint32 [PERIOD, rows, 64] per stage],
    packed hardware id of the wave that ran round 0)."""
    import numpy as np
    import torch

    values, hw = [], 0
    with torch.cuda.device(_device(device)):
        for stage in range(len(STAGES)):
            raw = _ext().transcheck_values(int(seed), stage, 0, PERIOD).cpu().numpy()
            raw = raw.view(np.uint32)
            hw = int(raw[-1])
            raw = raw[:-1].reshape(PERIOD, _ROUND_WORDS)
            rows = len(slot_table(stage))
            if (raw[:, -1] != rows).any():
                raise RuntimeError(f"transcheck: the kernel filled {int(raw[0, -1])} rows of "
                                   f"stage {stage}, the reference has {rows}")
            values.append(raw[:, :-1].reshape(PERIOD, _VALUE_ROWS, 64)[:, :rows].copy())
    return values, hw


def _golden(seed: int, device, values, limit: Optional[int]):
    """(digest table, number of violations, records of the first ``limit``
    per stage, packed hardware id) of ``golden``."""
    import numpy as np

    values, hw = values if values is not None else golden_values(seed, device)
    r = np.arange(PERIOD)
    table = np.stack([fold_values(s, v) for s, v in enumerate(values)], axis=1)
    found = [_violations(s, r, v, seed, limit) for s, v in enumerate(values)]
    return table, sum(n for n, _ in found), [rec for _, recs in found for rec in recs], hw


def golden(seed: int, device=None, _values=None):
    """(digest table uint32 [PERIOD, 4], violations, packed hardware id):
    ``golden_values`` (or ``_values``, what it would have returned) checked
    with ``check_values`` and folded with ``fold_values``."""
    table, _, violations, hw = _golden(seed, device, _values, None)
    return table, violations, hw


@dataclass
class TranscheckResult(DigestResult):
    # Whole-run lower bounds per stage in 1e9 lane-level transcendental
    # operations per second (the kernel's time also holds operand
    # generation, the other stages and the digests): informative.
    f32_gops: float = 0.0
    f16_gops: float = 0.0
    f64_gops: float = 0.0
    chain_gops: float = 0.0
    # mismatches = golden_errors + digest_mismatches
    golden_errors: int = 0
    digest_mismatches: int = 0
    golden_records: List[Dict] = field(default_factory=list)
    golden_wave: Dict = field(default_factory=dict)  # xcc, se, sh, cu, simd
    golden_s: float = 0.0  # host and GPU time of the golden pass
    waves_disagreeing: int = 0  # counted only where digests differed
    golden_suspect: bool = False

    def rate_fields(self) -> List[str]:
        return ["f32_gops", "f16_gops", "f64_gops", "chain_gops"]

    def to_dict(self) -> dict:
        out = super().to_dict()
        out.update(golden_errors=int(self.golden_errors),
                   digest_mismatches=int(self.digest_mismatches),
                   golden_records=[dict(r) for r in self.golden_records],
                   golden_wave=dict(self.golden_wave), golden_s=float(self.golden_s),
                   waves_disagreeing=int(self.waves_disagreeing),
                   golden_suspect=bool(self.golden_suspect))
        return out


def transcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
    _golden_values=None,
) -> TranscheckResult:
    """The golden pass, then ``rounds`` rounds of the workload on ``blocks``
    workgroups of 16 waves (0 = one per CU), every wave's digests compared
    with the golden table (module docstring).

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that one
    digest before the compare, ``_expected`` replaces the digest table and
    ``_golden_values`` what ``golden_values`` returns; all three are test
    hooks, since a test cannot damage a transcendental unit."""
    import numpy as np

    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"transcheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"transcheck: blocks must be in 0..4096, got {blocks}")
    if _expected is not None and np.shape(_expected) != (rounds, len(STAGES)):
        raise ValueError(f"transcheck: expected table must be [{rounds}, {len(STAGES)}], "
                         f"got {np.shape(_expected)}")
    if _inject is not None:  # checked here too: the golden pass launches first
        import torch

        waves = WAVES_PER_BLOCK * (blocks or torch.cuda.get_device_properties(
            _device(device)).multi_processor_count)
        limits = (waves, rounds, len(STAGES), 1 << 32)
        if len(_inject) != 4 or not all(0 <= int(v) < n for v, n in zip(_inject, limits)):
            raise ValueError(f"transcheck: inject (wave, round, stage, mask) {_inject} out of "
                             f"range {limits}")
    t0 = time.perf_counter()
    table, golden_errors, violations, hw = _golden(seed, device, _golden_values,
                                                   int(max_records))
    golden_s = time.perf_counter() - t0
    if _expected is None:
        _expected = _shared.tile_period(table[:min(rounds, PERIOD)], rounds, PERIOD)
    res = _shared.run_probe(
        "transcheck", TranscheckResult(rounds=rounds), STAGES, _OPS_PER_WAVE_ROUND, 1e9,
        None, seed, blocks, max_records, device, _inject, _expected)
    res.golden_s = golden_s
    res.golden_errors, res.digest_mismatches = golden_errors, res.mismatches
    res.golden_records = violations[:int(max_records)]
    res.golden_wave = decode_hw(hw)
    res.mismatches += res.golden_errors
    res.ok = res.mismatches == 0
    if res.digest_mismatches:
        # Inputs repeat with PERIOD, so the period's rounds up to the first
        # bad one show the same digests: at most waves x PERIOD x 16 bytes
        # of dump (8 MiB at the default grid).  Diagnostic only: whatever
        # goes wrong here, the verdict in res stands.
        try:
            n = res.first_bad_round % PERIOD + 1
            want = np.asarray(_expected)[res.first_bad_round]
            seen = _shared.wave_digests(
                "transcheck", _ext().transcheck_run,
                np.asarray(_expected)[res.first_bad_round + 1 - n:res.first_bad_round + 1],
                STAGES, seed, n, blocks, device)
            res.waves_disagreeing = int((seen[:, n - 1] != want[None]).any(axis=1).sum())
            res.golden_suspect = 2 * res.waves_disagreeing > len(seen)
        except Exception as e:
            from ..api import utils

            utils.errorf("transcheck: could not count the disagreeing waves: %s", e)
    return res


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None, table=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the same
    kernel as ``transcheck`` with its dump pointer set."""
    import numpy as np

    if table is None:
        table = np.zeros((int(rounds), len(STAGES)), dtype=np.uint32)
    return _shared.wave_digests("transcheck", _ext().transcheck_run, table, STAGES,
                                seed, rounds, blocks, device)


def wave_values(seed: int, stage: int, r: int, device=None):
    """What one wave folds for a stage and round: {row name: uint32[64]} in
    ``slot_table`` order, raw result bits.  A digest cannot say which
    operation went wrong; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    with torch.cuda.device(_device(device)):
        raw = _ext().transcheck_values(int(seed), stage, int(r), 1).cpu().numpy()
    return _shared.value_rows("transcheck", raw.view(np.uint32)[:-1], slot_table(stage),
                              _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def run_transcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                              timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the transcheck CLI."""
    return _active.run_probe_subprocess("transcheck", index, "--rounds", rounds, timeout_s)


def transcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                     rounds: int = DEFAULT_ROUNDS,
                     max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("transcheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "transcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: transcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
