"""Active probe for the vector-memory and cache paths — wrapper over the
vmemcheck HIP kernel.

The path between a wave's registers and the L2 is the block every kernel
depends on and no other probe exercises on purpose: the address coalescer
and the data-return formatter of the texture path, the per-CU vector L1,
the scalar data cache, the L2's byte-masked partial-line writes, the
cache-policy bits and the buffer-resource range check that CK-style
kernels use for their masking.  ``memcheck`` reaches global memory only
with lane-linear, 16-byte, nontemporal streaming accesses, and its data
does not depend on how it was accessed.  A byte enable dropped when four
lanes assemble one dword, a sign extension taken from the wrong byte, an
L1 hit that returns the neighbouring line, a scalar-cache line that
answers for another address or a range check that lets an out-of-range
lane through moves no ECC counter and passes the other eight probes.
This is ``ldscheck``'s twin for global memory.  Every op is a move, so
numpy is an exact reference.  ``vmemcheck()`` launches one 16-wave
workgroup per compute unit (it asks for the whole LDS only to keep a
second workgroup off the CU); every wave runs the same deterministic
workload and compares four 32-bit digests per round with
``reference_digests``.  Launch shape, accounting and the mismatch log are
cucheck's.

The workload (csrc/vmemcheck.hip; ``reference_values`` and
``reference_digests`` are the definition).  Integer arithmetic is mod
2**32; ``fmix32``, ``base``, ``salt`` are cucheck's and the stage number
fed to ``base`` is 40 + s.  Inputs repeat with PERIOD = 64 rounds:

  word(s, r, idx) = fmix32(base(seed, 40 + s, r % PERIOD) + idx)

Operand slot k is the per-lane value v(k)[l] = word(64 k + l), u(k) =
word(64 k) a wave-uniform word, and img(i) = word(4096 + i), i < 1024,
the stage's *image* of its region.  "rot k" is the lane (l + u(k)) mod 64,
so a lane reads what another lane stored, and perm(k)[l] = ((u(k) | 1) l +
(u(k) >> 8)) mod 64 is a bijection of the lanes.

Memory.  The *arena* is an int32 tensor the host allocates per call;
global wave g owns the *span* of SPAN_DWORDS = 4096 dwords at dword
4096 g and never touches another wave's.  Span dwords 0 .. 1023 are the
region of stage width, 1024 .. 1535 that of partial, 2048 .. 3071 that of
buffer; the rest is never touched.  Dword numbers d below are relative to
the stage's region.  *Address in data*: with tag(a) = fmix32(0xA5A5A5A5 ^
(a * 0x9E3779B9)) for the absolute arena dword index a, whatever a lane
stores to a is value ^ tag(a) (the matching bytes of the tag for a narrow
store) and whatever it loads from the address it meant to read is XORed
with that address's tag (sign-extended like the load for the signed
narrow loads) before it is folded.  On healthy hardware the tags cancel
and the table is the same for every wave; a line that answers for the
wrong address leaves tag(a) ^ tag(a') in the digest.  The reference never
sees a tag: it models a region as a little-endian byte array, applies the
stores in program order and takes views for the loads, and raises if an
address leaves the region.  The table X[65536], X[i] = fmix32(base(seed,
44, 0) + i), is read-only and untagged, written by the host before the
launch, and the only memory more than one wave reads.

Ordering.  A *fence* below is a workgroup-scope release and acquire fence
pair: it stands between a store and a load (or a second store) of the
same bytes by another lane.  On gfx950 the compiler emits no cache
maintenance for it, so the data stays where the access left it.  There
are no agent-scope fences inside the round loop, the scalar unit only
loads, and every store is a vector store written in plain C++ or a
builtin.  Cache policies (POLICIES): *plain*; *sc1*, a relaxed
agent-scope atomic load or store of 4 or 8 bytes (a 16-byte sc1 load is
two of 8: the compiler has no wider atomic); *nt*,
``__builtin_nontemporal_load`` / ``_store``.  By the microarchitecture
guide plain loads may hit the L1 while sc1 and nt loads are served by the
L2; that is not measured here.

Every op's result is a *result slot* n, a row of 64 u32, numbered in the
order below (``slot_table``).

Stages (STAGES) and what they run:

  width   global_store_dwordx4 fill of the region with img; fence.  For
          j = 0, 1: global_store_byte of (v(1 + j) & 0x7F) | ((l >> 2) & 1)
          << 7 to byte (l + u(0) + j) & 3 of dword 2 l + j; fence;
          global_load_dword of dwords 2 l and 2 l + 1 (the compiler
          fetches the pair as one global_load_dwordx2), global_load_ubyte of
          the byte lane rot 27 stored and global_load_sbyte of the byte
          lane rot 28 stored.  For j = 0, 1: global_store_short of (v(4 +
          j) & 0x7FFF) | ((l >> 1) & 1) << 15 to half (l + u(3) + j) & 1 of
          dword 128 + 2 l + j; fence; dwords 128 + 2 l and + 1,
          global_load_ushort and global_load_sshort of the halves lanes
          rot 29 and rot 30 stored.  So every byte lane and half, each
          with the top bit set and clear, occurs in every round.  Then
          global_store_dwordx2 of v(7), v(8) at dword 256 + 2 l,
          global_store_dwordx3 of v(9..11) at 384 + 4 l (aligned to 4 by
          its type), global_store_dwordx4 of v(14..17) at 640 + 4 l;
          fence; global_load_dwordx2 at rot 6, global_load_dwordx3 at rot
          12, global_load_dwordx4 over the 12-byte store at rot 13 (its
          fourth dword is the fill), global_load_dwordx4 at rot 18.  One
          slot per dword: 29 slots.
  gather  Reads X only.  For the widths 4, 8, 16 bytes (wi = 0, 1, 2) and
          the strides S = GATHER_STRIDES[si]: lane l loads the unit (l S +
          u(7 wi + si)) mod units, units = 262144 / width: all lanes on one
          address, on one line, on several lines, one line per lane.
          Then a free gather per width at unit v(21 + wi)[l] mod units.
          Each of these 24 loads uses POLICIES[n mod 3], n the number of
          its first slot, so L1-served and L2-served reads of the same
          table alternate.  Slots 0 .. 55.  Narrow gathers, plain:
          global_load_ubyte / sbyte at byte v(24) / v(25) mod 262144,
          global_load_ushort / sshort at half v(26) / v(27) mod 131072.
          Uniform loads j = 0 .. 4 of n = 1, 2, 4, 8, 16 dwords at the
          naturally aligned index readfirstlane(u(28 + j)) mod (65536 / n)
          (s_load_dword .. s_load_dwordx16), lane l folding dword l mod n;
          the last takes the 64-byte block that holds the first's dword
          (index (u(28) mod 65536) / 16) and one more slot reads that
          block by global_load_dword, lane l its dword l mod 16: the
          scalar cache and the vector L1 must agree.  66 slots.
  partial global_store_dwordx4 fill of the region's 512 dwords (16 lines
          of 128 bytes) with img and, with *no* fence in between: for j =
          0 .. 3 global_store_byte of v(4 + j) & 0xFF to byte (d + j) & 3
          of dword d = perm(j)[l], so every one of dwords 0 .. 63 is
          assembled from four lanes' bytes; for j = 0, 1
          global_store_short of v(10 + j) & 0xFFFF to half (d + j) & 1 of
          dword 64 + d, d = perm(8 + j)[l]; for j = 0 .. 3
          global_store_dword of v(16 + j) to dword 128 + 64 j + perm(12 +
          j)[l] with PARTIAL_POLICIES[j] = plain, sc1, nt, plain;
          global_store_dwordx2 of v(21), v(22) to dwords 384 + 2 perm(20)[l]
          and + 1.  No byte is stored twice after the fill.  Fence.  The
          512 dwords are read lane-linear (dwords 4 (64 t + l) .. + 3, t =
          0, 1), once plain and once sc1: 16 slots.
  buffer  The region's 4096 bytes are filled with img by
          global_store_dwordx4; fence.  A raw buffer resource
          (``__builtin_amdgcn_make_buffer_rsrc``, stride 0, flags word
          0x00020000) covers the region with num_records = N = 16 (96 +
          u(0) mod 96) bytes.  ``raw_buffer_load_b8 / b16 / b32 / b64 / b96
          / b128`` (wi = 0 .. 5, width w) at voffset = 16 ((l
          BUFFER_STRIDES[wi] + u(1 + wi)) mod 256) + w (v(8 + wi)[l] mod
          (16 / w)) (for b96 + 4 (v & 1), for b128 + 0): every access lies
          inside one 16-byte cell, hence wholly below N or wholly at or
          above it.  The reference returns the bytes where voffset < N,
          else 0; the kernel removes the tag only for the lanes it expects
          in range.  Two variants that stay below 1536 <= N under every
          reading of the range rule (no document at hand fixes whether
          soffset takes part in the check): b32 at voffset 4 ((5 l + u(14))
          mod 256) with the uniform soffset 16 (u(15) mod 16), and b128 at
          voffset 16 ((l + u(16)) mod 64) with the immediate offset 256.
          Fence.  ``raw_buffer_store_b128`` of v(20..23) to cell 4
          perm(19)[l], ``_b32`` of v(25) to dword v(28)[l] & 3 of cell 4
          perm(24)[l] + 1, ``_b8`` of v(27) & 0xFF to byte v(29)[l] & 15 of
          cell 4 perm(26)[l] + 2: those at or above N must be dropped.
          Fence.  Last, global_load_dwordx4 of all 4096 bytes, lane-linear:
          new values below N, img above.  A range check that fails still
          lands inside the wave's own span, so a broken GPU shows as a
          mismatch, never as a fault.  33 slots.

Digest of a stage: sum over slots n and lanes l of fmix32(value_n[l] +
salt(64 n + l)), mod 2**32.

Not covered: flat_ and scratch accesses, structured / swizzled buffers,
the _d16 / _d16_hi forms, misaligned accesses, soffset in the range
check, the Infinity Cache and HBM (memcheck's ground), cross-CU
visibility.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.vmemcheck --device INDEX [--rounds N] [--seed S]
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
    metric_args,
)

STAGES: Tuple[str, ...] = ("width", "gather", "partial", "buffer")
PERIOD = 64  # inputs of round r are those of round r % PERIOD
_STAGE0 = 40  # stage number fed to base() is _STAGE0 + s
_STAGE_X = 44  # base() stage number of the table X
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/vmemcheck_mi355x.json), default grid (256
# workgroups, 4096 waves, 256/256 CUs covered): 41.11, 36.57 and 34.49 us
# per round at 256, 1024 and 4096 rounds (the fixed cost of a launch
# fades), so 0.5 s are 14,497 rounds; the nearest multiple of PERIOD, 227 x
# 64 = 14528 rounds, takes 0.494 s measured.  The numpy table costs well
# under 0.1 s of host time whatever the rounds, since only PERIOD rows are
# computed.
DEFAULT_ROUNDS = 14528
_VALUE_ROWS = 128

_M32 = 0xFFFFFFFF

# -- layout and access tables (csrc/vmemcheck.hip holds the same) ------------------------

SPAN_DWORDS = 4096  # arena dwords of one wave
SPAN_BYTES = 4 * SPAN_DWORDS
_IMG0 = 4096  # word index of img(0)
IMG_DWORDS = 1024
# (first span dword, dwords) of each stage's region; gather has none
REGIONS: Dict[str, Tuple[int, int]] = {
    "width": (0, 1024), "partial": (1024, 512), "buffer": (2048, 1024)}
X_DWORDS = 65536
X_BYTES = 4 * X_DWORDS
GATHER_STRIDES: Tuple[int, ...] = (0, 1, 2, 3, 8, 16, 33)  # in units of the access
GATHER_WIDTHS: Tuple[int, ...] = (4, 8, 16)  # bytes
POLICIES: Tuple[str, ...] = ("plain", "sc1", "nt")
UNIFORM_DWORDS: Tuple[int, ...] = (1, 2, 4, 8, 16)
PARTIAL_POLICIES: Tuple[str, ...] = ("plain", "sc1", "nt", "plain")
BUFFER_WIDTHS: Tuple[int, ...] = (1, 2, 4, 8, 12, 16)  # bytes: b8 .. b128
# cells between neighbouring lanes: at least 4, so that the 64 lanes lie
# round the whole region at a distance below its shortest part, and every
# width has lanes below N and lanes at or above it
BUFFER_STRIDES: Tuple[int, ...] = (4, 5, 7, 8, 11, 16)
BUFFER_CELLS = 256  # 16-byte cells of the buffer region
BUFFER_IMM = 256  # immediate offset of the last load variant

# bytes one wave moves per round, per stage (stores and loads alike)
_BYTES_PER_WAVE_ROUND = (
    4096 + 64 * (2 * (1 + 4 + 4 + 1 + 1) + 2 * (2 + 4 + 4 + 2 + 2) + 2 * (8 + 12 + 16) + 16),
    64 * (8 * (4 + 8 + 16) + 1 + 1 + 2 + 2 + 4) + 4 * (1 + 2 + 4 + 8 + 16),
    2048 + 64 * (4 * 1 + 2 * 2 + 4 * 4 + 8) + 2 * 2048,
    4096 + 64 * (1 + 2 + 4 + 8 + 12 + 16 + 4 + 16) + 64 * (16 + 4 + 1) + 4096,
)


def tag(a):
    """The tag of absolute arena dword index ``a`` (an int or an array):
    what is XORed into every value stored there."""
    import numpy as np

    a = np.asarray(a, dtype=np.uint32)
    with np.errstate(over="ignore"):
        t = _fmix32(np.atleast_1d(np.uint32(0xA5A5A5A5) ^ (a * np.uint32(0x9E3779B9))))
    return t.reshape(a.shape) if a.shape else int(t[0])


def source_table(seed: int):
    """The read-only table X as uint32[X_DWORDS] (untagged)."""
    import numpy as np

    seed = int(seed) & _M32
    with np.errstate(over="ignore"):
        return _fmix32(_base(seed, _STAGE_X, np.uint32(0))
                       + np.arange(X_DWORDS, dtype=np.uint32))


# -- numpy definition: one stage, many rounds ---------------------------------------------

class _Words:
    """word(s, r, idx) for an array of rounds."""

    def __init__(self, seed: int, stage: int, r):
        import numpy as np

        rp = (np.asarray(r, dtype=np.uint32) % np.uint32(PERIOD)).astype(np.uint32)
        self.rp = rp
        self.base = _base(seed, _STAGE0 + stage, rp)
        self.lane = np.arange(64, dtype=np.uint32)

    def v(self, k: int):
        """uint32 [rounds, 64]"""
        import numpy as np

        with np.errstate(over="ignore"):
            return _fmix32(self.base[:, None] + (np.uint32(64 * k) + self.lane)[None, :])

    def u(self, k: int):
        """uint32 [rounds]"""
        import numpy as np

        with np.errstate(over="ignore"):
            return _fmix32(self.base + np.uint32(64 * k))

    def img(self, n: int = IMG_DWORDS):
        """uint32 [rounds, n]"""
        import numpy as np

        idx = np.uint32(_IMG0) + np.arange(n, dtype=np.uint32)
        with np.errstate(over="ignore"):
            return _fmix32(self.base[:, None] + idx[None, :])

    def rot(self, k: int):
        """int64 [rounds, 64]: lane (l + u(k)) mod 64"""
        import numpy as np

        return ((self.lane[None, :] + self.u(k)[:, None]) & np.uint32(63)).astype(np.int64)

    def perm(self, k: int):
        """int64 [rounds, 64]: ((u(k) | 1) l + (u(k) >> 8)) mod 64, a
        bijection of the lanes"""
        import numpy as np

        u = self.u(k)
        with np.errstate(over="ignore"):
            row = (u | np.uint32(1))[:, None] * self.lane[None, :] + (u >> np.uint32(8))[:, None]
        return (row & np.uint32(63)).astype(np.int64)

    def strided(self, k: int, stride: int, units: int):
        """int64 [rounds, 64]: (l stride + u(k)) mod units, units a power of two"""
        import numpy as np

        with np.errstate(over="ignore"):
            x = self.lane[None, :] * np.uint32(stride) + self.u(k)[:, None]
        return (x & np.uint32(units - 1)).astype(np.int64)


class _Bytes:
    """A little-endian byte array per round, uint8 [rounds, n]: a stage's
    region, or X.  Addresses are byte offsets into it, int64 [rounds, 64]
    or [64]; one that leaves the array raises."""

    def __init__(self, rounds: int, nbytes: int, what: str, mem=None):
        import numpy as np

        self.what = what
        self.mem = np.zeros((rounds, nbytes), dtype=np.uint8) if mem is None else mem

    def _addr(self, addr, nbytes: int):
        import numpy as np

        addr = np.broadcast_to(np.asarray(addr, dtype=np.int64), (len(self.mem), 64))
        if addr.min() < 0 or addr.max() + nbytes > self.mem.shape[1]:
            raise ValueError(f"vmemcheck: address outside {self.what}")
        return addr

    def fill(self, words):
        """the first dwords of every round from uint32 [rounds, n]"""
        import numpy as np

        raw = np.ascontiguousarray(words.astype("<u4")).view(np.uint8)
        self.mem[:, :raw.shape[1]] = raw

    def store(self, addr, value, nbytes: int, mask=None):
        """the low ``nbytes`` (1 .. 4) bytes of uint32 [rounds, 64] at byte
        ``addr``, of the lanes in ``mask`` (all if None)"""
        import numpy as np

        addr = self._addr(addr, nbytes)
        for b in range(nbytes):
            byte = ((value >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8)
            if mask is not None:
                byte = np.where(mask, byte, np.take_along_axis(self.mem, addr + b, axis=1))
            np.put_along_axis(self.mem, addr + b, byte, axis=1)

    def load(self, addr, nbytes: int):
        """uint32 [rounds, 64]: ``nbytes`` (1 .. 4) bytes at byte ``addr``,
        zero-extended"""
        import numpy as np

        addr = self._addr(addr, nbytes)
        out = np.zeros(addr.shape, dtype=np.uint32)
        for b in range(nbytes):
            out |= np.take_along_axis(self.mem, addr + b, axis=1).astype(np.uint32) \
                << np.uint32(8 * b)
        return out

    def store_dwords(self, byte, values, mask=None):
        for c, v in enumerate(values):
            self.store(byte + 4 * c, v, 4, mask)

    def load_dwords(self, byte, n: int):
        return [self.load(byte + 4 * c, 4) for c in range(n)]


def _region(stage: str, rounds: int) -> _Bytes:
    return _Bytes(rounds, 4 * REGIONS[stage][1], f"the {stage} region")


def _sext(x, bits: int):
    """Sign-extend the low ``bits`` of uint32 values."""
    import numpy as np

    m = np.uint32(1 << (bits - 1))
    with np.errstate(over="ignore"):
        return ((x & np.uint32((1 << bits) - 1)) ^ m) - m


def subdword_offsets(seed: int, r):
    """Where the narrow stores of stage width go in rounds ``r``: (byte
    within the dword [rounds, 2, 64], half within the dword [rounds, 2,
    64]) for the two byte and the two 16-bit stores."""
    import numpy as np

    W = _Words(int(seed) & _M32, 0, r)
    j = np.arange(2, dtype=np.uint32)[None, :, None]
    lane = W.lane[None, None, :]
    b8 = (lane + W.u(0)[:, None, None] + j) & np.uint32(3)
    b16 = (lane + W.u(3)[:, None, None] + j) & np.uint32(1)
    return b8.astype(np.int64), b16.astype(np.int64)


def _stage_width(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 0, r)
    S = _region("width", len(W.base))
    lane = np.arange(64, dtype=np.int64)
    l32 = W.lane
    S.fill(W.img())
    b8, b16 = subdword_offsets(seed, r)
    out = []
    for j in range(2):
        addr = 4 * (2 * lane + j)[None, :] + b8[:, j]
        val = (W.v(1 + j) & np.uint32(0x7F)) | (((l32 >> np.uint32(2)) & np.uint32(1))
                                                << np.uint32(7))[None, :]
        S.store(addr, val, 1)
        out.append((f"b8.{j}.dword", S.load(8 * lane, 4)))
        out.append((f"b8.{j}.next", S.load(8 * lane + 4, 4)))
        for name, k in (("u8", 27), ("i8", 28)):
            got = S.load(np.take_along_axis(addr, W.rot(k), axis=1), 1)
            out.append((f"b8.{j}.{name}", got if name == "u8" else _sext(got, 8)))
    for j in range(2):
        addr = 4 * (128 + 2 * lane + j)[None, :] + 2 * b16[:, j]
        val = (W.v(4 + j) & np.uint32(0x7FFF)) | (((l32 >> np.uint32(1)) & np.uint32(1))
                                                  << np.uint32(15))[None, :]
        S.store(addr, val, 2)
        out.append((f"b16.{j}.dword", S.load(4 * (128 + 2 * lane), 4)))
        out.append((f"b16.{j}.next", S.load(4 * (129 + 2 * lane), 4)))
        for name, k in (("u16", 29), ("i16", 30)):
            got = S.load(np.take_along_axis(addr, W.rot(k), axis=1), 2)
            out.append((f"b16.{j}.{name}", got if name == "u16" else _sext(got, 16)))
    S.store_dwords(4 * (256 + 2 * lane), [W.v(7), W.v(8)])
    S.store_dwords(4 * (384 + 4 * lane), [W.v(9 + c) for c in range(3)])
    S.store_dwords(4 * (640 + 4 * lane), [W.v(14 + c) for c in range(4)])
    for name, d0, step, k, n in (("b64", 256, 2, 6, 2), ("b96", 384, 4, 12, 3),
                                 ("b96.b128", 384, 4, 13, 4), ("b128", 640, 4, 18, 4)):
        for c, v in enumerate(S.load_dwords(4 * (d0 + step * W.rot(k)), n)):
            out.append((f"{name}.{c}", v))
    return out


def gather_plan(seed: int, r):
    """The 24 wide gathers of stage gather in rounds ``r``, in slot
    order: [(slot name, width in bytes, policy, unit index int64 [rounds,
    64])]."""
    import numpy as np

    W = _Words(int(seed) & _M32, 1, r)
    plan, n = [], 0
    for wi, width in enumerate(GATHER_WIDTHS):
        for si, s in enumerate(GATHER_STRIDES):
            plan.append((f"b{8 * width}.s{s}", width, POLICIES[n % 3],
                         W.strided(7 * wi + si, s, X_BYTES // width)))
            n += width // 4
    for wi, width in enumerate(GATHER_WIDTHS):
        unit = (W.v(21 + wi) & np.uint32(X_BYTES // width - 1)).astype(np.int64)
        plan.append((f"b{8 * width}.free", width, POLICIES[n % 3], unit))
        n += width // 4
    return plan


def _stage_gather(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 1, r)
    n = len(W.base)
    table = np.ascontiguousarray(source_table(seed).astype("<u4")).view(np.uint8)
    X = _Bytes(n, X_BYTES, "the table X", np.broadcast_to(table, (n, X_BYTES)))
    out = []
    for name, width, policy, unit in gather_plan(seed, r):
        for c, v in enumerate(X.load_dwords(width * unit, width // 4)):
            out.append((f"{name}.{policy}.{c}" if width > 4 else f"{name}.{policy}", v))
    byte = lambda k: (W.v(k) & np.uint32(X_BYTES - 1)).astype(np.int64)  # noqa: E731
    half = lambda k: 2 * (W.v(k) & np.uint32(X_BYTES // 2 - 1)).astype(np.int64)  # noqa: E731
    out.append(("u8", X.load(byte(24), 1)))
    out.append(("i8", _sext(X.load(byte(25), 1), 8)))
    out.append(("u16", X.load(half(26), 2)))
    out.append(("i16", _sext(X.load(half(27), 2), 16)))
    lane = np.arange(64, dtype=np.int64)
    for j, nd in enumerate(UNIFORM_DWORDS):
        index = (W.u(28 + j) % np.uint32(X_DWORDS // nd)).astype(np.int64)
        if nd == 16:  # the block that holds the first uniform load's dword
            index = (W.u(28) % np.uint32(X_DWORDS)).astype(np.int64) // 16
        at = 4 * (nd * index[:, None] + (lane % nd)[None, :])
        out.append((f"uniform.x{nd}", X.load(at, 4)))
    out.append(("uniform.x16.vector", X.load(at, 4)))
    return out


def partial_rows(seed: int, r):
    """Where the scattered stores of stage partial go in rounds ``r``, as
    int64 arrays of region dwords: "byte" [rounds, 4, 64] with
    "byte_lane" the byte within the dword, "half" [rounds, 2, 64] with
    "half_lane", "dword" [rounds, 4, 64], and "b64" [rounds, 64], the first
    dword of each 8-byte store."""
    import numpy as np

    W = _Words(int(seed) & _M32, 2, r)
    byte = np.stack([W.perm(j) for j in range(4)], axis=1)
    half = np.stack([64 + W.perm(8 + j) for j in range(2)], axis=1)
    return {
        "byte": byte,
        "byte_lane": (byte + np.arange(4)[None, :, None]) & 3,
        "half": half,
        "half_lane": (half + np.arange(2)[None, :, None]) & 1,
        "dword": np.stack([128 + 64 * j + W.perm(12 + j) for j in range(4)], axis=1),
        "b64": 384 + 2 * W.perm(20),
    }


def _stage_partial(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 2, r)
    S = _region("partial", len(W.base))
    lane = np.arange(64, dtype=np.int64)
    S.fill(W.img(512))
    rows = partial_rows(seed, r)
    for j in range(4):
        S.store(4 * rows["byte"][:, j] + rows["byte_lane"][:, j], W.v(4 + j), 1)
    for j in range(2):
        S.store(4 * rows["half"][:, j] + 2 * rows["half_lane"][:, j], W.v(10 + j), 2)
    for j in range(4):
        S.store(4 * rows["dword"][:, j], W.v(16 + j), 4)
    S.store_dwords(4 * rows["b64"], [W.v(21), W.v(22)])
    out = []
    for policy in ("plain", "sc1"):
        for t in range(2):
            for c, v in enumerate(S.load_dwords(16 * (64 * t + lane), 4)):
                out.append((f"{policy}.t{t}.{c}", v))
    return out


def buffer_plan(seed: int, r):
    """The data-driven choices of stage buffer in rounds ``r``:
    "num_records" int64 [rounds]; "loads" and "stores", {name: (byte
    offset into the region int64 [rounds, 64], bytes per lane)} of the
    accesses the range check decides; "offset_loads", the same for the two
    variants with an soffset and an immediate offset, the offset being
    the sum of all its parts."""
    import numpy as np

    W = _Words(int(seed) & _M32, 3, r)
    i64 = lambda x: x.astype(np.int64)  # noqa: E731
    loads = {}
    for wi, (w, s) in enumerate(zip(BUFFER_WIDTHS, BUFFER_STRIDES)):
        cell = W.strided(1 + wi, s, BUFFER_CELLS)
        if w == 12:
            sub = 4 * i64(W.v(8 + wi) & np.uint32(1))
        else:
            sub = w * i64(W.v(8 + wi) & np.uint32(16 // w - 1))
        loads[f"load.b{8 * w}"] = (16 * cell + sub, w)
    soff = 16 * i64(W.u(15) & np.uint32(15))
    return {
        "num_records": 16 * (96 + i64(W.u(0) % np.uint32(96))),
        "loads": loads,
        "offset_loads": {
            "load.b32.soffset": (4 * W.strided(14, 5, 256) + soff[:, None], 4),
            "load.b128.imm": (16 * W.strided(16, 1, 64) + BUFFER_IMM, 16),
        },
        "stores": {
            "store.b128": (16 * (4 * W.perm(19)), 16),
            "store.b32": (16 * (4 * W.perm(24) + 1) + 4 * i64(W.v(28) & np.uint32(3)), 4),
            "store.b8": (16 * (4 * W.perm(26) + 2) + i64(W.v(29) & np.uint32(15)), 1),
        },
    }


def _stage_buffer(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 3, r)
    S = _region("buffer", len(W.base))
    lane = np.arange(64, dtype=np.int64)
    S.fill(W.img())
    plan = buffer_plan(seed, r)
    N = plan["num_records"][:, None]
    out = []

    def load(name, at, w):
        # the range check: whole accesses below num_records, else zeros
        ok = at < N
        if w < 4:
            out.append((name, np.where(ok, S.load(at, w), np.uint32(0))))
            return
        for c, v in enumerate(S.load_dwords(at, w // 4)):
            out.append((f"{name}.{c}" if w > 4 else name, np.where(ok, v, np.uint32(0))))

    for name, (at, w) in plan["loads"].items():
        load(name, at, w)
    for name, (at, w) in plan["offset_loads"].items():
        load(name, at, w)
    at, _ = plan["stores"]["store.b128"]
    S.store_dwords(at, [W.v(20 + c) for c in range(4)], at < N)
    at, _ = plan["stores"]["store.b32"]
    S.store(at, W.v(25), 4, at < N)
    at, _ = plan["stores"]["store.b8"]
    S.store(at, W.v(27), 1, at < N)
    for t in range(4):
        for c, v in enumerate(S.load_dwords(16 * (64 * t + lane), 4)):
            out.append((f"readback.t{t}.{c}", v))
    return out


_STAGE_FUNCS = (_stage_width, _stage_gather, _stage_partial, _stage_buffer)


def _stage(seed: int, stage: int, r) -> List[tuple]:
    """[(slot name, uint32 [rounds, 64])] of a stage for rounds ``r``
    (uint32 array), in slot order."""
    if stage not in range(len(STAGES)):
        raise ValueError(f"vmemcheck: stage {stage} out of range 0..3")
    return _STAGE_FUNCS[stage](seed, r)


def slot_table(stage: int) -> List[str]:
    """The name of every result slot of a stage, in slot order."""
    return [name for name, _ in _stage(0, int(stage), _shared.one_round("vmemcheck", 0))]


def reference_values(seed: int, stage: int, r: int):
    """What a wave folds in one stage and round: {slot name: uint32[64]},
    in slot order, exact per lane and the same for every wave."""
    slots = _stage(int(seed) & _M32, int(stage), _shared.one_round("vmemcheck", r))
    return {name: v[0] for name, v in slots}


def digest_of(values) -> int:
    """The stage digest of rows of 64 u32 in slot order (a sequence of
    arrays, or what ``reference_values`` returns)."""
    import numpy as np

    rows = list(values.values()) if isinstance(values, dict) else list(values)
    lane = np.arange(64, dtype=np.uint32)
    total = np.uint32(0)
    with np.errstate(over="ignore"):
        for n, v in enumerate(rows):
            h = _fmix32(np.asarray(v, dtype=np.uint32) + _salt(np.uint32(64 * n) + lane))
            total = total + h.sum(dtype=np.uint32)
    return int(total)


def _digest(slots: List[tuple]):
    """uint32[rounds] of a stage."""
    import numpy as np

    lane = np.arange(64, dtype=np.uint32)
    total = 0
    with np.errstate(over="ignore"):
        for n, (_, v) in enumerate(slots):
            h = _fmix32(v + _salt(np.uint32(64 * n) + lane)[None, :])
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


# -- GPU run ---------------------------------------------------------------------

@dataclass
class VmemcheckResult(DigestResult):
    # Whole-run lower bounds per stage in GB/s of bytes loaded and stored
    # (the kernel's time also holds operand generation, the address tags,
    # the other stages and the digests): informative.
    width_gbps: float = 0.0
    gather_gbps: float = 0.0
    partial_gbps: float = 0.0
    buffer_gbps: float = 0.0


def _table(seed: int, device):
    import numpy as np
    import torch

    return torch.from_numpy(source_table(seed).view(np.int32).copy()).to(device)


def _arena(blocks: int, device):
    """A fresh, zeroed arena for ``blocks`` workgroups (0 = one per CU)."""
    import torch

    if blocks == 0:
        blocks = int(torch.cuda.get_device_properties(device).multi_processor_count)
    return torch.zeros(blocks * WAVES_PER_BLOCK * SPAN_DWORDS, dtype=torch.int32,
                       device=device)


def vmemcheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
    _arena_tensor=None,
) -> VmemcheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup asks for a CU's whole LDS, so on an idle GPU the default
    grid lands one workgroup on every CU; ``cus_covered`` reports how
    many distinct CUs actually ran a wave.  The arena (64 KiB per wave)
    and the table X are allocated per call.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare, ``_expected`` replaces the reference
    table and ``_arena_tensor`` the arena (int32, blocks x 16 x
    SPAN_DWORDS, contiguous, on the GPU); all three are test hooks."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"vmemcheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"vmemcheck: blocks must be in 0..4096, got {blocks}")
    if not 0 <= seed <= _M32:
        raise ValueError("vmemcheck: seed must be a u32")
    dev = _device(device)
    arena = _arena_tensor if _arena_tensor is not None else _arena(blocks, dev)
    return _shared.run_probe(
        "vmemcheck", VmemcheckResult(rounds=rounds), STAGES, _BYTES_PER_WAVE_ROUND, 1e9,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected, arena, _table(seed, dev))


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``vmemcheck`` with its dump pointer set."""
    dev = _device(device)
    return _shared.wave_digests(
        "vmemcheck", _ext().vmemcheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device, _arena(int(blocks), dev), _table(seed, dev))


def wave_values(seed: int, stage: int, r: int, wave: int = 0, device=None):
    """What wave ``wave`` of one workgroup folded for a stage and round,
    shaped like ``reference_values``: {slot name: uint32[64]}.  A digest
    cannot say which access moved what; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    names = slot_table(stage)
    device = _device(device)
    with torch.cuda.device(device):
        raw = _ext().vmemcheck_values(int(seed), stage, int(r), _arena(1, device),
                                      _table(seed, device), int(wave)).cpu().numpy()
    return _shared.value_rows("vmemcheck", raw.view(np.uint32), names, _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def run_vmemcheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                             timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the vmemcheck CLI."""
    return _active.run_probe_subprocess("vmemcheck", index, "--rounds", rounds, timeout_s)


def vmemcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                    rounds: int = DEFAULT_ROUNDS,
                    max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("vmemcheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "vmemcheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: vmemcheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
