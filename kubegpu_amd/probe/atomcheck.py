"""Active probe for the read-modify-write units — wrapper over the
atomcheck HIP kernel.

``cucheck``, ``mxcheck`` and ``fpcheck`` never issue an atomic as
workload, and the units that execute atomics are hardware of their own:
the LDS atomic ALUs of every CU, the integer atomic units in every XCD's
L2 and, for global float atomics, units on the memory side.  Scatter-add
and embedding backward, split-K reductions, attention-backward dQ sums
and every work queue go through them; a unit that loses, doubles or
mis-computes an update corrupts results silently and ECC does not see
it.  ``atomcheck()`` launches one 16-wave workgroup per compute unit;
every wave runs the same deterministic sequence of atomics and compares
four 32-bit digests per round with ``reference_digests``, and the host
then checks one region that every wave of the grid has added into
against ``reference_shared``.  Launch shape, accounting and the mismatch
log are cucheck's.

The workload (csrc/atomcheck.hip; ``reference_values``,
``reference_digests`` and ``reference_shared`` are the definition).
Integer arithmetic is mod 2**32 or 2**64; ``fmix32``, ``base``, ``salt``
are cucheck's and the stage number fed to ``base`` is 16 + s.  Inputs
repeat with PERIOD = 64 rounds:

  word(s, r, idx) = fmix32(base(seed, 16 + s, r % PERIOD) + idx)

*Operand slot* k of a lane is lo = word 128 k + lane and hi = word
128 k + 64 + lane; a 32-bit operand is lo, a 64-bit one lo | hi << 32.
No input depends on the global wave number, so the table is the same
for every wave.  Memory is cut in 8-byte *cells*; a 32-bit op uses the
low half.  A wave has one slice (64 owned cells, then blocks of 8
contended cells) in the LDS and three in the arena, one per global
stage.  Every access is a relaxed atomic store, load or RMW, at agent
scope in the arena and at workgroup scope in the LDS.

Stages (STAGES) and what they run:

  lds   LDS: u32 / i32 all 13 ops; u64 add, umin, umax; f32, f64,
        packed 2 x f16 and packed 2 x bf16 add; the cross-wave phase
  g32   arena: u32 / i32 all 13 ops
  g64   arena: u64 add, sub, umin, umax, and, or, xor, exchange, cas
  gfp   arena: f32 add; f64 add, min, max; packed f16 and bf16 add

Owned phase: lane l alone on cell l.  Integers, operand slots k0 .. k0
+ 14 (k0 = 0 for u32, 35 for u64): store slot k0; then, of OWNED_OPS
those the stage has, in order add, sub, umin, umax, smin, smax, and, or,
xor, inc, dec, xchg, cas, op number i taking slot k0 + 1 + i; then a
load.  inc stores 0 where old >= operand, else old + 1; dec stores the
operand where old == 0 or old > operand, else old - 1: the cell and the
bound are both uniform words, so both outcomes occur.  The cas follows
the exchange: compare = the exchanged-in operand ^ (slot k0 + 14 & 1),
new value = slot k0 + 13, so hit or miss is decided by an input bit.
Every returned (old) value and the final load are results; no operand
derives from a returned value.  Floats, slots 70 .. 82: f32 store, add,
add, load; f64 store, add, then add (lds) or min, max (gfp), load;
packed f16 and packed bf16 store, add, add, load (halves from lo and hi
of the same slot).

Contended phase: one block of 8 cells per op, lane l on cell l & 7, so
eight lanes share a cell.  Lanes 0..7 store the initial values; all
lanes issue the op; lanes 0..7 load the finals; each step is complete
before the next starts.  Integer op j of CONTENDED_OPS has slots c0 + 2 j
(per cell) and c0 + 2 j + 1 (per lane), c0 = 15 for u32, 50 for u64:
add, xor (initial value a word), and (operand = all ones but two bits,
initial all ones), or (two bits, initial 0), umin, umax, smin, smax
(initial value the op's identity) are non-returning and only the finals
are results; ``ticket`` is a returning add of the per-cell constant
(slot | 1), ``xchg`` a returning exchange.  Float op j takes slot 83 + j
from 0: f32 add, f64 add, f64 min, f64 max, packed f16 add, packed bf16
add, initial value 0 (plus / minus infinity for min / max).

Cross-wave phase (stage lds): 64 u32 cells shared by the workgroup; cell
c takes op c & 7 of (add, xor, or, and, umin, umax, add, xor).  Wave w
stores the initial values of cells 4 w .. 4 w + 3 (a word at 128 * 96 +
8192 + c for add and xor, else the identity); barrier; lane l of wave w
applies op j = 0 .. 7 to cell 8 ((l + w + j) & 7) + j with the word at
128 * 96 + 1024 j + 64 w + l (or: that word's bit (w & 31) if bits 5..7
are zero, else nothing; and: the complement); barrier; every wave loads
all 64 cells; barrier.  The only dependence on the wave's index in the
workgroup is here, and the 64 finals are the same for all 16 waves.

Float operands are fop(word, bits) = +-(1 + (word & (2**bits - 1))),
sign from bit 31: nonzero integers.  Bounds, so that every partial sum
in every order is an exactly representable integer:
  f32   bits 12: |x| <= 4096, at most 9 terms: < 2**16 <= 2**24
  f64   bits 20: |x| <= 2**20, at most 9 terms: < 2**24 <= 2**53
  f16   bits 7:  |x| <= 128, owned 3 terms <= 384, contended 8 terms
        from 0 <= 1024 <= 2048 = 2**11
  bf16  bits 5:  |x| <= 32, owned 3 terms <= 96, contended 8 terms from
        0 <= 256 = 2**8
so rounding inside the float atomics is deliberately not covered.

Digest of a stage: results are numbered by *slot* n in the order above
(``slot_table``); value v of slot n contributes fmix32(lo(v) ^
fmix32(hi(v) + salt(key))), summed mod 2**32, with key = 64 n + lane
for owned results and the cross-wave finals, 64 n + cell for contended
finals and ticket returns; the returns of ``xchg`` and its finals share
the key 64 n + cell of the returns' slot.  What eight lanes get back
from a ticket add or an exchange depends on arrival order only as a
permutation within a cell, and the final of an exchanged cell is the one
value missing from its returns, so every digest is independent of
arrival order.

Shared region: 6 rows of 64 cells at the end of the arena, the only
place where contention crosses workgroups and XCDs.  On rounds with r %
SHARED_EVERY == 0, lane l of every wave g of the grid applies to cell l
of each row one non-returning op whose operand combines A_i = fmix32(
base(seed, 20, r % PERIOD) + 64 i + l) and B_i = fmix32(base(seed, 21, g)
+ 64 i + l):
  0 u32 add   (A_0 | 1) + (B_0 & ~1): odd, so never zero
  1 u64 add   ((A_1 | A_6 << 32) | 1) + ((B_1 | B_6 << 32) & ~1)
  2 u32 xor   A_2 ^ B_2
  3 u32 umax  (A_3 >> 1) + (B_3 >> 1): no overflow, so max separates
  4 u32 umin  the same with A_4, B_4
  5 f64 add   +-((A_5 & 0x3FFFE) | 1) +- (B_5 & 0x3FFFE), signs from bit
              31: odd, |x| < 2**19, so 65536 rounds x 65536 waves stay
              below 2**53 and exact
``reference_shared`` has the finals in closed form, O(PERIOD * 64 +
waves * 64).

Not covered: rounding inside float atomics (operands are exact by
construction), f32 min and max, fine-grained and host memory, system
scope, peer GPUs.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.atomcheck --device INDEX [--rounds N] [--seed S]
"""

from __future__ import annotations

import sys
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple

from . import _active
from . import _digest as _shared
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

STAGES: Tuple[str, ...] = ("lds", "g32", "g64", "gfp")
PERIOD = 64  # inputs of round r are those of round r % PERIOD
_STAGE0 = 16  # stage number fed to base() is _STAGE0 + s
# The shared region is hit on rounds r % SHARED_EVERY == 0.  Measured on
# MI355X (profiles/atomcheck_mi355x.json), default grid (256 workgroups,
# 4096 waves all adding into the same 6 x 64 cells): 191.7 us per round
# with the shared ops every round, 124.6 us with none, so they cost
# 67.1 us, 35 % of a round.  That is not under a third, so they run
# every second round: 152.0 us per round on average, 18 % of it theirs.
SHARED_EVERY = 2
# One default launch should hold the GPU for roughly half a second.
# Measured with SHARED_EVERY = 2: 152.7, 152.0 and 152.0 us per round at
# 512, 3200 and 12800 rounds, so 0.5 s are 3289 rounds; 51 x 64 = 3264
# rounds (51 periods) take 0.50 s (0.500 measured).  The numpy table
# costs about 0.05 s of host time whatever the rounds, since only PERIOD
# rows are computed.
DEFAULT_ROUNDS = 3264

OWNED_OPS = ("add", "sub", "umin", "umax", "smin", "smax", "and", "or", "xor",
             "inc", "dec", "xchg", "cas")
CONTENDED_OPS = ("add", "and", "or", "xor", "umin", "umax", "smin", "smax",
                 "ticket", "xchg")
FLOAT_OPS = ("f32_add", "f64_add", "f64_min", "f64_max", "f16x2_add", "bf16x2_add")
CROSS_OPS = ("add", "xor", "or", "and", "umin", "umax", "add", "xor")
SHARED_OPS = ("u32_add", "u64_add", "u32_xor", "u32_umax", "u32_umin", "f64_add")
_OWNED_L64 = ("add", "umin", "umax")
_OWNED_G64 = ("add", "sub", "umin", "umax", "and", "or", "xor", "xchg", "cas")
_CONT_L64 = ("add", "umin", "umax")
_CONT_G64 = ("add", "and", "or", "xor", "umin", "umax", "ticket", "xchg")
_FLOAT_LDS = ("f32_add", "f64_add", "f16x2_add", "bf16x2_add")
FLOAT_BITS = {"f32": 12, "f64": 20, "f16": 7, "bf16": 5}
# largest integer below which every integer is representable
FLOAT_EXACT = {"f32": 1 << 24, "f64": 1 << 53, "f16": 1 << 11, "bf16": 1 << 8}
_K_O32, _K_C32, _K_O64, _K_C64, _K_F, _K_CF, _K_XW = 0, 15, 35, 50, 70, 83, 96

WAVE_CELLS = 3 * (64 + 8 * 17)  # arena cells of one wave
SHARED_CELLS = 64 * len(SHARED_OPS)
_VALUE_ROWS = 64

# atomic RMW operations one wave issues per round, per stage
_OPS_PER_WAVE_ROUND = (64 * (13 + 3 + 8 + 10 + 3 + 4 + 8), 64 * (13 + 10),
                       64 * (9 + 8), 64 * (9 + 6))

_M32 = 0xFFFFFFFF
_M64 = 0xFFFFFFFFFFFFFFFF


def _u(x):
    import numpy as np

    return np.uint64(x)


# -- operands ------------------------------------------------------------------------

class _Words:
    """word(s, r, idx) for an array of rounds: ``w(idx)`` is uint64
    [rounds, len(idx)], zero-extended."""

    def __init__(self, seed: int, stage: int, r):
        import numpy as np

        rp = (np.asarray(r, dtype=np.uint32) % np.uint32(PERIOD)).astype(np.uint32)
        self.base = _base(seed, _STAGE0 + stage, rp)
        self.lane = np.arange(64, dtype=np.uint32)

    def w(self, idx):
        import numpy as np

        idx = np.asarray(idx, dtype=np.uint32)
        with np.errstate(over="ignore"):
            return _fmix32(self.base[:, None] + idx[None, :]).astype(np.uint64)

    def lo(self, k: int):
        return self.w(128 * k + self.lane)

    def hi(self, k: int):
        return self.w(128 * k + 64 + self.lane)

    def opnd(self, k: int, wide: bool):
        return self.lo(k) | (self.hi(k) << _u(32)) if wide else self.lo(k)


def _fop(w, bits: int):
    """int64: +-(1 + (w & (2**bits - 1))), sign from bit 31."""
    import numpy as np

    m = (w & _u((1 << bits) - 1)).astype(np.int64) + 1
    return np.where((w >> _u(31)) != 0, -m, m)


def _two_bits(w, width: int):
    m = _u(width - 1)
    return (_u(1) << (w & m)) | (_u(1) << ((w >> _u(8)) & m))


def _sparse_bit(w):
    import numpy as np

    return np.where(((w >> _u(5)) & _u(7)) == 0, _u(1) << (w & _u(31)), _u(0))


def _f32_bits(i):
    import numpy as np

    return np.asarray(i).astype(np.float32).view(np.uint32).astype(np.uint64)


def _f64_bits(i):
    import numpy as np

    return np.asarray(i).astype(np.float64).view(np.uint64)


def _f16_bits(i):
    import numpy as np

    return np.asarray(i).astype(np.float16).view(np.uint16).astype(np.uint64)


def _bf16_bits(i):
    """bf16 pattern of integers with at most 8 significant bits."""
    return _f32_bits(i) >> _u(16)


_NARROW_BITS = {"f16": _f16_bits, "bf16": _bf16_bits}


# -- sequential semantics of every op (plain Python integers) ------------------------------

def _signed(x: int, width: int) -> int:
    return x - (1 << width) if x >> (width - 1) else x


def apply_int(op: str, old: int, x: int, width: int, cmp: Optional[int] = None) -> int:
    """New cell value after integer atomic ``op`` with operand ``x`` on a
    cell holding ``old``: the definition of each op, one at a time."""
    m = (1 << width) - 1
    if op in ("add", "ticket"):
        return (old + x) & m
    if op == "sub":
        return (old - x) & m
    if op == "umin":
        return min(old, x)
    if op == "umax":
        return max(old, x)
    if op == "smin":
        return old if _signed(old, width) <= _signed(x, width) else x
    if op == "smax":
        return old if _signed(old, width) >= _signed(x, width) else x
    if op == "and":
        return old & x
    if op == "or":
        return old | x
    if op == "xor":
        return old ^ x
    if op == "inc":
        return 0 if old >= x else old + 1
    if op == "dec":
        return x if old == 0 or old > x else old - 1
    if op == "xchg":
        return x
    if op == "cas":
        return x if old == cmp else old
    raise ValueError(f"atomcheck: no integer op {op!r}")


# -- numpy definition: one stage, many rounds ---------------------------------------------

@dataclass
class Slot:
    """One row of results: ``kind`` is "owned" (64 lanes, exact),
    "returns" (64 lanes, a multiset per cell l & 7), "final" (cells 0..7)
    or "cross" (64 cells); ``key_slot`` is the slot whose number salts
    the digest (an exchange's finals use its returns' slot)."""

    name: str
    kind: str
    values: object  # uint64 [rounds, 64]; finals in columns 0..7, rest 0
    key_slot: int


def _pad8(v):
    import numpy as np

    out = np.zeros((v.shape[0], 64), dtype=np.uint64)
    out[:, :8] = v
    return out


def _by_cell(x):
    """[rounds, 64 lanes] -> [rounds, 8 arrivals, 8 cells]: lane l is on
    cell l & 7."""
    return x.reshape(x.shape[0], 8, 8)


def _sflip(x, width: int):
    return x ^ _u(1 << (width - 1))


class _Stage:
    def __init__(self, seed: int, stage: int, r):
        self.W = _Words(seed, stage, r)
        self.slots: List[Slot] = []
        # what the order-independence test replays: (name, op, type,
        # initial value per cell [rounds, 8], operand per lane [rounds, 64])
        self.contended: List[tuple] = []
        self.cross = None

    def emit(self, name, kind, values, key_slot=None):
        n = len(self.slots)
        self.slots.append(Slot(name, kind, values, n if key_slot is None else key_slot))

    # owned integers
    def owned_int(self, tag: str, width: int, k0: int, ops):
        import numpy as np

        wide, W = width == 64, self.W
        m = _u(_M64 if wide else _M32)
        cell = W.opnd(k0, wide)
        for i, op in enumerate(OWNED_OPS):
            if op not in ops:
                continue
            x, old = W.opnd(k0 + 1 + i, wide), cell
            with np.errstate(over="ignore"):
                if op == "add":
                    cell = (old + x) & m
                elif op == "sub":
                    cell = (old - x) & m
                elif op == "umin":
                    cell = np.minimum(old, x)
                elif op == "umax":
                    cell = np.maximum(old, x)
                elif op == "smin":
                    cell = np.where(_sflip(old, width) <= _sflip(x, width), old, x)
                elif op == "smax":
                    cell = np.where(_sflip(old, width) >= _sflip(x, width), old, x)
                elif op == "and":
                    cell = old & x
                elif op == "or":
                    cell = old | x
                elif op == "xor":
                    cell = old ^ x
                elif op == "inc":
                    cell = np.where(old >= x, _u(0), (old + _u(1)) & m)
                elif op == "dec":
                    cell = np.where((old == 0) | (old > x), x, (old - _u(1)) & m)
                elif op == "xchg":
                    cell = x
                else:  # cas, right after the exchange
                    cmp = W.opnd(k0 + 12, wide) ^ (W.lo(k0 + 14) & _u(1))
                    cell = np.where(old == cmp, x, old)
            self.emit(f"{tag}.{op}", "owned", old)
        self.emit(f"{tag}.final", "owned", cell)

    # contended integers
    def contended_int(self, tag: str, width: int, c0: int, ops):
        import numpy as np

        wide, W = width == 64, self.W
        full = _M64 if wide else _M32
        m = _u(full)
        n_rounds = len(W.base)
        const = lambda v: np.full((n_rounds, 8), v, dtype=np.uint64)  # noqa: E731
        for j, op in enumerate(CONTENDED_OPS):
            if op not in ops:
                continue
            per_cell = W.opnd(c0 + 2 * j, wide)[:, :8]
            x = W.opnd(c0 + 2 * j + 1, wide)
            name = f"{tag}.{op}"
            if op == "and":
                init, x = const(full), ~_two_bits(x & _u(_M32), width) & m
            elif op == "or":
                init, x = const(0), _two_bits(x & _u(_M32), width)
            elif op == "umin":
                init = const(full)
            elif op == "umax":
                init = const(0)
            elif op == "smin":
                init = const(full >> 1)
            elif op == "smax":
                init = const((full >> 1) + 1)
            else:
                init = per_cell
            if op == "ticket":
                step = W.opnd(c0 + 2 * j + 1, wide)[:, :8] | _u(1)
                x = np.tile(step, (1, 8))
            self.contended.append((name, op, f"u{width}", init, x))
            g = _by_cell(x)
            with np.errstate(over="ignore"):
                if op == "add":
                    final = (init + g.sum(axis=1, dtype=np.uint64)) & m
                elif op == "and":
                    final = init & np.bitwise_and.reduce(g, axis=1)
                elif op == "or":
                    final = init | np.bitwise_or.reduce(g, axis=1)
                elif op == "xor":
                    final = init ^ np.bitwise_xor.reduce(g, axis=1)
                elif op == "umin":
                    final = np.minimum(init, g.min(axis=1))
                elif op == "umax":
                    final = np.maximum(init, g.max(axis=1))
                elif op == "smin":
                    final = _sflip(np.minimum(_sflip(init, width),
                                              _sflip(g, width).min(axis=1)), width)
                elif op == "smax":
                    final = _sflip(np.maximum(_sflip(init, width),
                                              _sflip(g, width).max(axis=1)), width)
                elif op == "ticket":
                    # arrivals in lane order: the multiset is what counts
                    olds = (init[:, None, :] + np.arange(8, dtype=np.uint64)[None, :, None]
                            * g) & m
                    final = (init + _u(8) * g[:, 0, :]) & m
                    self.emit(name, "returns", olds.reshape(n_rounds, 64))
                else:  # xchg, arrivals in lane order
                    olds = np.concatenate([init[:, None, :], g[:, :7, :]], axis=1)
                    final = g[:, 7, :]
                    self.emit(name, "returns", olds.reshape(n_rounds, 64))
                    self.emit(name + ".final", "final", _pad8(final),
                              key_slot=len(self.slots) - 1)
                    continue
            self.emit(name + ".final", "final", _pad8(final))

    # floats
    def _packed(self, k: int, fmt: str):
        bits = FLOAT_BITS[fmt]
        return _fop(self.W.lo(k), bits), _fop(self.W.hi(k), bits)

    def owned_float(self, minmax: bool):
        import numpy as np

        W = self.W
        f = lambda k: _fop(W.lo(_K_F + k), FLOAT_BITS["f32"]).astype(np.float32)  # noqa: E731
        d = lambda k: _fop(W.lo(_K_F + k), FLOAT_BITS["f64"]).astype(np.float64)  # noqa: E731
        a, b, c = f(0), f(1), f(2)
        self.emit("f32.add0", "owned", _f32_bits(a))
        self.emit("f32.add1", "owned", _f32_bits(a + b))
        self.emit("f32.final", "owned", _f32_bits((a + b) + c))
        a, b, c = d(3), d(4), d(5)
        self.emit("f64.add", "owned", _f64_bits(a))
        if minmax:
            e = d(6)
            lo = np.minimum(a + b, c)
            self.emit("f64.min", "owned", _f64_bits(a + b))
            self.emit("f64.max", "owned", _f64_bits(lo))
            self.emit("f64.final", "owned", _f64_bits(np.maximum(lo, e)))
        else:
            self.emit("f64.add1", "owned", _f64_bits(a + b))
            self.emit("f64.final", "owned", _f64_bits((a + b) + c))
        for fmt, k in (("f16", 7), ("bf16", 10)):
            to_bits = _NARROW_BITS[fmt]
            lo = [self._packed(_K_F + k + i, fmt)[0] for i in range(3)]
            hi = [self._packed(_K_F + k + i, fmt)[1] for i in range(3)]
            pk = lambda x, y: to_bits(x) | (to_bits(y) << _u(16))  # noqa: E731
            self.emit(f"{fmt}x2.add0", "owned", pk(lo[0], hi[0]))
            self.emit(f"{fmt}x2.add1", "owned", pk(lo[0] + lo[1], hi[0] + hi[1]))
            self.emit(f"{fmt}x2.final", "owned",
                      pk(lo[0] + lo[1] + lo[2], hi[0] + hi[1] + hi[2]))

    def contended_float(self, ops):
        import numpy as np

        W = self.W
        n_rounds = len(W.base)
        zero = np.zeros((n_rounds, 8), dtype=np.int64)
        for j, op in enumerate(FLOAT_OPS):
            if op not in ops:
                continue
            k = _K_CF + j
            if op in ("f32_add", "f64_add"):
                fmt = op[:3]
                x = _fop(W.lo(k), FLOAT_BITS[fmt])
                self.contended.append((op, "add", fmt, zero, x))
                total = _by_cell(x).sum(axis=1)
                final = _f32_bits(total) if fmt == "f32" else _f64_bits(total)
            elif op in ("f64_min", "f64_max"):
                x = _fop(W.lo(k), FLOAT_BITS["f64"])
                self.contended.append((op, op[4:], "f64", None, x))
                g = _by_cell(x)
                final = _f64_bits(g.min(axis=1) if op == "f64_min" else g.max(axis=1))
            else:
                fmt = op.split("x")[0]
                lo, hi = self._packed(k, fmt)
                self.contended.append((op + ".lo", "add", fmt, zero, lo))
                self.contended.append((op + ".hi", "add", fmt, zero, hi))
                to_bits = _NARROW_BITS[fmt]
                final = to_bits(_by_cell(lo).sum(axis=1)) \
                    | (to_bits(_by_cell(hi).sum(axis=1)) << _u(16))
            self.emit(op + ".final", "final", _pad8(final))

    # stage lds's cross-wave phase
    def cross_wave(self):
        import numpy as np

        W = self.W
        n_rounds = len(W.base)
        lane = np.arange(64, dtype=np.uint32)
        wave = np.arange(16, dtype=np.uint32)
        c = np.arange(64, dtype=np.uint32)
        word = W.w(128 * _K_XW + 8192 + c)
        ident = {"add": None, "xor": None, "or": 0, "and": _M32, "umin": _M32, "umax": 0}
        init = np.empty((n_rounds, 64), dtype=np.uint64)
        for cell in range(64):
            v = ident[CROSS_OPS[cell & 7]]
            init[:, cell] = word[:, cell] if v is None else _u(v)
        contributions = []  # (cell index [16, 64], op, operands [rounds, 16, 64]) per j
        final = init.copy()
        for j, op in enumerate(CROSS_OPS):
            idx = 128 * _K_XW + 1024 * j + 64 * wave[:, None] + lane[None, :]
            x = W.w(idx.reshape(-1)).reshape(n_rounds, 16, 64)
            if op == "or":
                x = _sparse_bit(x)
            elif op == "and":
                x = ~_sparse_bit(x) & _u(_M32)
            target = 8 * ((lane[None, :] + wave[:, None] + j) & 7) + j
            contributions.append((target, op, x))
            for t in range(8):
                cell = 8 * t + j
                sel = x[:, target == cell]
                with np.errstate(over="ignore"):
                    if op == "add":
                        final[:, cell] = (init[:, cell]
                                          + sel.sum(axis=1, dtype=np.uint64)) & _u(_M32)
                    elif op == "xor":
                        final[:, cell] = init[:, cell] ^ np.bitwise_xor.reduce(sel, axis=1)
                    elif op == "or":
                        final[:, cell] = init[:, cell] | np.bitwise_or.reduce(sel, axis=1)
                    elif op == "and":
                        final[:, cell] = init[:, cell] & np.bitwise_and.reduce(sel, axis=1)
                    elif op == "umin":
                        final[:, cell] = np.minimum(init[:, cell], sel.min(axis=1))
                    else:
                        final[:, cell] = np.maximum(init[:, cell], sel.max(axis=1))
        self.cross = (init, contributions)
        self.emit("cross.final", "cross", final)


def _stage(seed: int, stage: int, r) -> _Stage:
    """Every slot of a stage for rounds ``r`` (uint32 array), in the
    kernel's order."""
    if stage not in range(len(STAGES)):
        raise ValueError(f"atomcheck: stage {stage} out of range 0..3")
    st = _Stage(seed, stage, r)
    if stage == 0:
        st.owned_int("u32", 32, _K_O32, OWNED_OPS)
        st.contended_int("c32", 32, _K_C32, CONTENDED_OPS)
        st.owned_int("u64", 64, _K_O64, _OWNED_L64)
        st.contended_int("c64", 64, _K_C64, _CONT_L64)
        st.owned_float(minmax=False)
        st.contended_float(_FLOAT_LDS)
        st.cross_wave()
    elif stage == 1:
        st.owned_int("u32", 32, _K_O32, OWNED_OPS)
        st.contended_int("c32", 32, _K_C32, CONTENDED_OPS)
    elif stage == 2:
        st.owned_int("u64", 64, _K_O64, _OWNED_G64)
        st.contended_int("c64", 64, _K_C64, _CONT_G64)
    else:
        st.owned_float(minmax=True)
        st.contended_float(FLOAT_OPS)
    return st


def _round_stage(seed: int, stage: int, r: int) -> _Stage:
    return _stage(int(seed) & _M32, int(stage), _shared.one_round("atomcheck", r))


def slot_table(stage: int) -> List[Tuple[str, str]]:
    """(name, kind) of every result slot of a stage, in slot order."""
    return [(s.name, s.kind) for s in _round_stage(0, stage, 0).slots]


def reference_values(seed: int, stage: int, r: int):
    """What wave 0 folds in one stage and round: {slot name: uint64[64]},
    in slot order (``slot_table`` gives each slot's kind).  "owned" and
    "cross" rows are exact per lane; a "returns" row is given for
    arrivals in lane order and is defined only as a multiset per cell
    l & 7 (for ``xchg`` together with the cell's final); "final" rows
    hold cells 0..7, the rest is zero."""
    st = _round_stage(seed, stage, r)
    return {s.name: s.values[0] for s in st.slots}


def reference_contended(seed: int, stage: int, r: int):
    """The contended phase's inputs for one stage and round, for replay
    in any order: a list of (name, op, type, initial value per cell
    [8] or None for the op's identity, operand per lane [64]); lane l
    acts on cell l & 7.  Integer types carry uint64 patterns, float
    types signed integers."""
    st = _round_stage(seed, stage, r)
    return [(n, op, t, None if init is None else init[0], x[0])
            for n, op, t, init, x in st.contended]


def reference_cross(seed: int, r: int):
    """The cross-wave phase's inputs for one round: (initial values
    uint64[64], [(cell, op, operand) for every lane of every wave])."""
    st = _round_stage(seed, 0, r)
    init, contributions = st.cross
    flat = []
    for target, op, x in contributions:
        for w in range(16):
            for lane in range(64):
                flat.append((int(target[w, lane]), op, int(x[0, w, lane])))
    return init[0], flat


def _digest(st: _Stage):
    """uint32[rounds] of a stage."""
    import numpy as np

    lane = np.arange(64, dtype=np.uint32)
    total = np.zeros(len(st.W.base), dtype=np.uint32)
    with np.errstate(over="ignore"):
        for s in st.slots:
            if s.kind in ("owned", "cross"):
                key, v = 64 * s.key_slot + lane, s.values
            elif s.kind == "returns":
                key, v = 64 * s.key_slot + (lane & 7), s.values
            else:
                key, v = 64 * s.key_slot + lane[:8], s.values[:, :8]
            lo = (v & _u(_M32)).astype(np.uint32)
            hi = (v >> _u(32)).astype(np.uint32)
            h = _fmix32(lo ^ _fmix32(hi + _salt(key.astype(np.uint32))[None, :]))
            total = total + h.sum(axis=1, dtype=np.uint32)
    return total


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


# -- the shared region ------------------------------------------------------------------

def _shared_terms(seed: int, which: int, n: int):
    """A (which = 4, n = PERIOD) or B (which = 5, n = waves) as uint64
    [7, n, 64]."""
    import numpy as np

    base = _base(seed, _STAGE0 + which, np.arange(n, dtype=np.uint32))
    idx = np.arange(7 * 64, dtype=np.uint32)
    with np.errstate(over="ignore"):
        w = _fmix32(base[:, None] + idx[None, :]).astype(np.uint64)
    return w.reshape(n, 7, 64).transpose(1, 0, 2)


def shared_operands(seed: int, r: int, wave: int):
    """The six operands lane l of global wave ``wave`` applies in round
    ``r``: uint64 [6, 64] (the f64 row holds the value's bit pattern)."""
    import numpy as np

    seed = int(seed) & _M32
    A = _shared_terms(seed, 4, PERIOD)[:, int(r) % PERIOD]
    B = _shared_terms(seed, 5, int(wave) + 1)[:, int(wave)]
    out = np.empty((6, 64), dtype=np.uint64)
    with np.errstate(over="ignore"):
        out[0] = ((A[0] | _u(1)) + (B[0] & _u(_M32 - 1))) & _u(_M32)
        out[1] = ((A[1] | (A[6] << _u(32))) | _u(1)) \
            + ((B[1] | (B[6] << _u(32))) & _u(_M64 - 1))
        out[2] = A[2] ^ B[2]
        out[3] = (A[3] >> _u(1)) + (B[3] >> _u(1))
        out[4] = (A[4] >> _u(1)) + (B[4] >> _u(1))
    out[5] = _f64_bits(_shared_fa(A[5]) + _shared_fb(B[5]))
    return out


def _shared_fa(a):
    import numpy as np

    m = ((a & _u(0x3FFFE)) | _u(1)).astype(np.int64)
    return np.where((a >> _u(31)) != 0, -m, m)


def _shared_fb(b):
    import numpy as np

    m = (b & _u(0x3FFFE)).astype(np.int64)
    return np.where((b >> _u(31)) != 0, -m, m)


def shared_initial():
    """The shared region before a launch, uint64 [6, 64]: zero, and all
    ones in the low word of the umin row."""
    import numpy as np

    init = np.zeros((len(SHARED_OPS), 64), dtype=np.uint64)
    init[4] = _u(_M32)
    return init


def reference_shared(seed: int, rounds: int, waves: int,
                     drop: Optional[Tuple[int, int]] = None,
                     shared_every: Optional[int] = None):
    """Finals of the shared region after ``rounds`` rounds of ``waves``
    waves as uint64 [6, 64] bit patterns, rows in SHARED_OPS order, in
    closed form: O(PERIOD * 64 + waves * 64).  ``drop=(wave, round)``
    leaves that one wave's contribution of that one round out."""
    import numpy as np

    seed, rounds, waves = int(seed) & _M32, int(rounds), int(waves)
    every = SHARED_EVERY if shared_every is None else int(shared_every)
    if rounds < 0 or waves < 0:
        raise ValueError("reference_shared: rounds >= 0 and waves >= 0 required")
    out = shared_initial()
    active = list(range(0, rounds, every)) if every > 0 else []
    if drop is not None:
        dw, dr = int(drop[0]), int(drop[1])
        if not (0 <= dw < waves and 0 <= dr < rounds):
            raise ValueError("reference_shared: drop (wave, round) out of range")
        if dr not in active:
            drop = None
    if not active or waves == 0:
        return out
    count = np.bincount(np.array(active) % PERIOD, minlength=PERIOD).astype(np.uint64)
    used = count > 0
    A = _shared_terms(seed, 4, PERIOD)
    B = _shared_terms(seed, 5, waves)
    nr, nw = _u(len(active)), _u(waves)
    cnt = count[:, None]
    with np.errstate(over="ignore"):
        a0, b0 = A[0] | _u(1), B[0] & _u(_M32 - 1)
        out[0] = (nw * (cnt * a0).sum(axis=0, dtype=np.uint64)
                  + nr * b0.sum(axis=0, dtype=np.uint64)) & _u(_M32)
        a1 = (A[1] | (A[6] << _u(32))) | _u(1)
        b1 = (B[1] | (B[6] << _u(32))) & _u(_M64 - 1)
        out[1] = nw * (cnt * a1).sum(axis=0, dtype=np.uint64) \
            + nr * b1.sum(axis=0, dtype=np.uint64)
        # a term repeated an even number of times cancels
        xa = np.bitwise_xor.reduce(np.where((cnt * nw) % _u(2) == 1, A[2], _u(0)), axis=0)
        xb = np.bitwise_xor.reduce(B[2], axis=0) if len(active) % 2 else _u(0)
        out[2] = xa ^ xb
        a3, b3 = A[3] >> _u(1), B[3] >> _u(1)
        a4, b4 = A[4] >> _u(1), B[4] >> _u(1)
        out[3] = a3[used].max(axis=0) + b3.max(axis=0)
        out[4] = np.minimum(out[4], a4[used].min(axis=0) + b4.min(axis=0))
        fa, fb = _shared_fa(A[5]), _shared_fb(B[5])
        total = waves * (count.astype(np.int64)[:, None] * fa).sum(axis=0) \
            + len(active) * fb.sum(axis=0)
        if drop is not None:
            rp = dr % PERIOD
            out[0] = (out[0] - (a0[rp] + b0[dw])) & _u(_M32)
            out[1] = out[1] - (a1[rp] + b1[dw])
            out[2] = out[2] ^ A[2][rp] ^ B[2][dw]
            total = total - (fa[rp] + fb[dw])
            # max / min over every (round, wave) pair but the dropped one:
            # the other rounds with any wave, or that round with another wave
            others = count.copy()
            others[rp] -= _u(1)
            rest = others > 0
            for row, a, b, pick, ident in ((3, a3, b3, np.maximum, 0),
                                           (4, a4, b4, np.minimum, _M32)):
                red = np.max if row == 3 else np.min
                best = np.full(64, ident, dtype=np.uint64)
                if rest.any():
                    best = pick(best, red(a[rest], axis=0) + red(b, axis=0))
                if waves > 1:
                    best = pick(best, a[rp] + red(np.delete(b, dw, axis=0), axis=0))
                out[row] = best
    out[5] = _f64_bits(total)
    return out


# -- GPU run ---------------------------------------------------------------------

@dataclass
class AtomcheckResult(DigestResult):
    # cells of the shared region that differ from reference_shared, and up
    # to max_records of them as {"op", "cell", "expected", "got"}
    shared_mismatches: int = 0
    shared_records: List[Dict] = field(default_factory=list)
    # Whole-run lower bounds per stage in 1e9 lane-level atomic RMW
    # operations per second (the kernel's time also holds operand
    # generation, the other stages and the digests): informative.
    lds_gops: float = 0.0
    g32_gops: float = 0.0
    g64_gops: float = 0.0
    gfp_gops: float = 0.0

    def rate_fields(self) -> List[str]:
        return ["lds_gops", "g32_gops", "g64_gops", "gfp_gops"]

    def to_dict(self) -> dict:
        out = super().to_dict()
        out["shared_mismatches"] = int(self.shared_mismatches)
        out["shared_records"] = [dict(r) for r in self.shared_records]
        return out


def _check_args(rounds: int, blocks: int) -> None:
    if not 1 <= rounds <= 65536:
        raise ValueError(f"atomcheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"atomcheck: blocks must be in 0..4096, got {blocks}")


def _grid(blocks: int, device) -> int:
    import torch

    return blocks or int(torch.cuda.get_device_properties(device).multi_processor_count)


def _arena(blocks: int, device):
    """A fresh arena for ``blocks`` workgroups: the waves' slices zeroed
    (the kernel stores every cell before it uses it), the shared region
    at the end set to ``shared_initial()``."""
    import numpy as np
    import torch

    arena = torch.zeros(blocks * WAVES_PER_BLOCK * WAVE_CELLS + SHARED_CELLS,
                        dtype=torch.int64, device=device)
    init = shared_initial().reshape(-1).view(np.int64)
    arena[-SHARED_CELLS:] = torch.from_numpy(init.copy()).to(device)
    return arena


def atomcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _drop: Optional[Tuple[int, int]] = None,
    _expected=None,
) -> AtomcheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU), compare every wave's digests with
    ``reference_digests`` and the shared region with
    ``reference_shared``.

    A workgroup asks for a CU's whole LDS, so on an idle GPU the default
    grid lands one workgroup on every CU; ``cus_covered`` reports how
    many distinct CUs actually ran a wave.  The arena is allocated and
    initialised anew for every call.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare, ``_drop=(global_wave, round)`` makes
    that wave skip its shared-region ops in that round (a real lost
    update) and ``_expected`` replaces the digest table; all three are
    test hooks, since a test cannot break an atomic unit."""
    import numpy as np

    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    _check_args(rounds, blocks)
    ext = _ext()
    device = _device(device)
    blocks = _grid(blocks, device)
    waves = blocks * WAVES_PER_BLOCK
    inject = None if _inject is None else tuple(int(x) for x in _inject)
    drop = None if _drop is None else tuple(int(x) for x in _drop)
    if inject is not None and not (0 <= inject[0] < waves and 0 <= inject[1] < rounds
                                   and 0 <= inject[2] < len(STAGES)
                                   and 0 <= inject[3] <= _M32):
        raise ValueError("atomcheck: inject (wave, round, stage, mask) out of range")
    if drop is not None and not (0 <= drop[0] < waves and 0 <= drop[1] < rounds):
        raise ValueError("atomcheck: drop (wave, round) out of range")
    table = _expected if _expected is not None else reference_digests(seed, rounds)
    expected = _shared.expected_tensor("atomcheck", table, rounds, STAGES, device)
    arena = _arena(blocks, device)
    raw = ext.atomcheck_run(expected, seed, rounds, blocks, arena, SHARED_EVERY,
                            int(max_records), None, inject, drop)
    res = _shared.fill_result(
        AtomcheckResult(rounds=rounds), raw, STAGES, device, _OPS_PER_WAVE_ROUND, 1e9)
    got = arena[-SHARED_CELLS:].cpu().numpy().view(np.uint64).reshape(len(SHARED_OPS), 64)
    want = reference_shared(seed, rounds, waves)
    bad = np.argwhere(got != want)
    res.shared_mismatches = int(len(bad))
    res.shared_records = [
        {"op": SHARED_OPS[op], "cell": int(cell), "expected": int(want[op, cell]),
         "got": int(got[op, cell])} for op, cell in bad[:int(max_records)]]
    res.ok = res.mismatches == 0 and res.shared_mismatches == 0
    return res


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``atomcheck`` with its dump pointer set."""
    rounds, blocks = int(rounds), int(blocks)
    _check_args(rounds, blocks)
    device = _device(device)
    blocks = _grid(blocks, device)
    return _shared.wave_digests(
        "atomcheck", _ext().atomcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device, _arena(blocks, device), SHARED_EVERY)


def wave_values(seed: int, stage: int, r: int, device=None):
    """What wave 0 of one workgroup folded for a stage and round, shaped
    like ``reference_values``: {slot name: uint64[64]}.  A digest cannot
    say which op returned what; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    names = [n for n, _ in slot_table(stage)]
    with torch.cuda.device(_device(device)):
        raw = _ext().atomcheck_values(int(seed), stage, int(r)).cpu().numpy()
    return _shared.value_rows("atomcheck", raw.view(np.uint64), names, _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def metric_args(rec: dict) -> tuple:
    """What ``set_gpu_atomcheck`` takes of a result dict, before the
    timestamp."""
    return (int(rec["mismatches"]), int(rec.get("shared_mismatches", 0)),
            int(rec.get("cus_covered", 0)))


def run_atomcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                             timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the atomcheck CLI."""
    return _active.run_probe_subprocess("atomcheck", index, "--rounds", rounds, timeout_s)


def atomcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                    rounds: int = DEFAULT_ROUNDS,
                    max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("atomcheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "atomcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: atomcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
