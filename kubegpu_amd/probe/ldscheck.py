"""Active probe for the LDS array and its access paths — wrapper over the
ldscheck HIP kernel.

The 160 KiB LDS of a compute unit is the largest block the other probes
leave almost untouched: ``mxcheck``, ``fpcheck`` and ``lanecheck`` ask for
it only to keep a second workgroup off the CU, ``atomcheck`` issues
atomics on a few cells, and ``cucheck``'s ``lds`` stage stores and loads
dwords at lane-linear, conflict-free addresses inside each wave's own
slice, with data that does not depend on the address.  The byte-enable,
sign-extension and multi-cycle paths of the narrow and wide accesses, the
bank-conflict replay and broadcast logic, gfx950's transposed read, the
LDS-DMA write port and the address decode above a wave's slice are
hardware of their own.  A GEMM tile that lands 1 KiB off, or a conflict
replay that drops a lane, corrupts results silently and ECC does not see
it: the cells hold what was stored.  Every op here is a move, so numpy is
an exact reference.  ``ldscheck()`` launches one 16-wave workgroup per
compute unit; every wave runs the same deterministic workload and compares
four 32-bit digests per round with ``reference_digests``.  Launch shape,
accounting and the mismatch log are cucheck's.

The workload (csrc/ldscheck.hip; ``reference_values`` and
``reference_digests`` are the definition).  Integer arithmetic is mod
2**32; ``fmix32``, ``base``, ``salt`` are cucheck's and the stage number
fed to ``base`` is 32 + s.  Inputs repeat with PERIOD = 64 rounds:

  word(s, r, idx) = fmix32(base(seed, 32 + s, r % PERIOD) + idx)

Operand slot k is the per-lane value v(k)[l] = word(64 k + l), u(k) =
word(64 k) a wave-uniform word, and img(i) = word(4096 + i), i < 2560,
the stage's *image* of a slice.

The workgroup uses all 163,840 bytes: wave w of the block owns the
*slice* of SLICE_DWORDS = 2,560 dwords at absolute dword address 2560 w,
and all dword numbers d below are relative to the slice.  *Address in
data*: with tag(a) = fmix32(0xA5A5A5A5 ^ (a * 0x9E3779B9)) for the
absolute dword address a, whatever a lane stores to a is value ^ tag(a)
(the matching bytes of the tag for a narrow store) and whatever it loads
from the address it meant to read is XORed with that address's tag
(sign-extended like the load for the signed narrow loads) before it is
folded.  On healthy hardware the tags cancel and the table is the same
for every wave; a cell that answers for the wrong address leaves tag(a) ^
tag(a') in the digest.  The reference never sees a tag: it models one
slice as a little-endian byte array, applies the stores in program order
and takes views for the loads.  Every op's result is a *result slot* n, a
row of 64 u32, numbered in the order below (``slot_table``).  "rot" is a
lane rotation (l + u) mod 64 by a uniform word, so a lane reads what
another lane stored.

Stages (STAGES) and what they run:

  width  ds_write_b32 fill of the slice with img.  For j = 0, 1:
         ds_write_b8 of (v(1 + j) & 0x7F) | ((l >> 2) & 1) << 7 to byte
         (l + u(0) + j) & 3 of dword 2 l + j, then ds_read_b32 of dwords
         2 l and 2 l + 1, ds_read_u8 of the byte lane rot u(27) stored and
         ds_read_i8 of the byte lane rot u(28) stored (a lane's own byte
         would be forwarded in registers).  For j = 0, 1: ds_write_b16 of
         (v(4 + j) & 0x7FFF) | ((l >> 1) & 1) << 15 to half (l + u(3) + j)
         & 1 of dword 128 + 2 l + j, then dwords 128 + 2 l and + 1,
         ds_read_u16 and ds_read_i16 of the halves lanes rot u(29) and rot
         u(30) stored.  So every byte lane and half, each with the top
         bit set and clear, occurs in every round, and every narrow store
         is followed by its whole dword and the next one.
         ds_write_b64 of v(7), v(8) at dword 256 + 2 l, ds_read_b64 at rot
         u(6); ds_write_b96 of v(9..11) at 384 + 4 l, ds_read_b96 at rot
         u(12), ds_read_b128 at rot u(13) (its fourth dword is the fill);
         ds_write_b128 of v(14..17) at 640 + 4 l, ds_read_b128 at rot
         u(18); an 8-byte access aligned to 4 (ds_write2_b32 /
         ds_read2_b32) of v(19), v(20) at 897 + 2 l, read at rot u(21);
         dwords 1088 + l and 1088 + l + 64 * ST64_K (ds_write2st64_b32 /
         ds_read2st64_b32) of v(22), v(23), read at rot u(24).  One slot
         per dword.
         Two ds_read_b64_tr_b16, t = 0, 1: lane l gives byte address 8 *
         (v(25 + t)[l] mod 1280).  Within each group of 16 lanes, lane
         4 q + p supplies row q, columns 4 p .. 4 p + 3 of a 4 x 16 block
         of 16-bit elements; lane i receives column i, row q in its
         element q (``transposed_read``).  Slots: elements 0, 1 and
         elements 2, 3, packed little-endian.
  bank   ds_write_b128 fill of dwords 0 .. 2047 with img.  ds_read_b32 at
         dword (l S + u(j)) mod 2048 for S = B32_STRIDES[j]; ds_read_b64
         at 8-byte unit (l S + u(10 + j)) mod 1024 for S = WIDE_STRIDES[j];
         ds_read_b128 at 16-byte unit (l S + u(16 + j)) mod 512 likewise;
         all lanes at dword u(22) mod 2048; lanes at u(23 + (l & 1)) mod
         2048; a free gather at v(25)[l] mod 2048.  Scatter p of SCATTERS
         = (stride, offset): lane l stores v(27 + 2 p) to dword stride *
         row + offset, row = ((u(26 + 2 p) | 1) l + (u(26 + 2 p) >> 8))
         mod 64, a bijection; then lane l reads dword stride * l + offset.
         Stride 32 puts all 64 targets on one bank.
  dma    Two read-only global tables (``source_tables``): G[16][2560] with
         G[w][i] = g(i) ^ tag(2560 w + i), g(i) = fmix32(base(seed, 36, 0)
         + i), and X[4096] with X[i] = fmix32(base(seed, 37, 0) + i).
         *placed*: wave w copies chunks of G[w] to the same dwords of its
         slice: global_load_lds_dwordx4 (1 KiB) of chunk u(0) mod 10, and
         from the base of chunk u(1) mod 8 with instruction offsets 1024
         and 2048; global_load_lds_dword (256 B) of unit u(2) mod 37 and,
         by instruction offset 768, the unit three further.  After
         vmcnt(0) the three chunks are read with ds_read_b128 (dwords 256 c
         + 4 l ..) and the two units with ds_read_b32, tags removed.  The
         M0 base of wave w is 4 (2560 w + ..) bytes: above 64 KiB from
         wave 7 on.
         *gather*: every wave reads X; x4 gather g = 0, 1: lane l loads
         the 16 bytes at dword v(3 + g)[l] & 0xFFC into chunk u(5 + g) mod
         10, lane-linear; dword gather g = 0, 1: dword v(7 + g)[l] & 0xFFF
         into unit u(9 + g) mod 40; each read back, untagged.
  xwave  Each wave fills its slice with img by ds_write_b128, barrier,
         reads the whole slice of the waves (w + 1 + (3 r + j) mod 15) mod
         16, j = 0, 1, 2, (r taken mod PERIOD) by ds_read_b128, removes
         the tag of the address it meant and folds every dword; barrier;
         the same with ~img; barrier.  Over five rounds every wave has
         read every other wave's cells.  The values are the image,
         whoever the partner is.

Digest of a stage: sum over slots n and lanes l of fmix32(value_n[l] +
salt(64 n + l)), mod 2**32.

Not covered: global_load_lds of 1, 2 and 12 bytes and the _tr_b4 / _tr_b6
/ _tr_b8 reads (their layouts are not documented where this was written),
ds_read_addtid / ds_write_addtid, LDS atomics (atomcheck's ground), GDS,
misaligned wide accesses, retention over time.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.ldscheck --device INDEX [--rounds N] [--seed S]
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

STAGES: Tuple[str, ...] = ("width", "bank", "dma", "xwave")
PERIOD = 64  # inputs of round r are those of round r % PERIOD
_STAGE0 = 32  # stage number fed to base() is _STAGE0 + s
_STAGE_G, _STAGE_X = 36, 37  # base() stage numbers of the DMA tables
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/ldscheck_mi355x.json), default grid (256
# workgroups, 4096 waves, 256/256 CUs covered): 69.00, 65.75 and 64.94 us
# per round at 256, 1024 and 4096 rounds (the fixed cost of a launch
# fades), so 0.5 s are 7700 rounds; the nearest multiple of PERIOD, 120 x
# 64 = 7680 rounds, takes 0.496 s measured.  The numpy table costs about
# 0.1 s of host time whatever the rounds, since only PERIOD rows are
# computed.
DEFAULT_ROUNDS = 7680
_VALUE_ROWS = 256

_M32 = 0xFFFFFFFF

# -- layout and access tables (csrc/ldscheck.hip holds the same) -------------------------

SLICE_DWORDS = 2560  # 160 KiB / 16 waves / 4
SLICE_BYTES = 4 * SLICE_DWORDS
LDS_DWORDS = WAVES_PER_BLOCK * SLICE_DWORDS
_IMG0 = 4096  # word index of img(0)
BANK_DWORDS = 2048  # stage bank's region: 8 KiB
ST64_K = 3  # the st64 pair is 64 * ST64_K dwords apart
B32_STRIDES: Tuple[int, ...] = (1, 2, 3, 4, 8, 16, 32, 33, 64, 65)
WIDE_STRIDES: Tuple[int, ...] = (1, 2, 4, 8, 16, 17)  # in units of the access
# (stride, offset) of the scatters' 64 rows, in dwords
SCATTERS: Tuple[Tuple[int, int], ...] = ((1, 0), (32, 7), (17, 3))
CHUNK_DWORDS = 256  # one global_load_lds_dwordx4
UNIT_DWORDS = 64  # one global_load_lds_dword
X_DWORDS = 4096
G_DWORDS = WAVES_PER_BLOCK * SLICE_DWORDS
TABLE_DWORDS = G_DWORDS + X_DWORDS
# chunk choices of the placed phase: (modulus of the base chunk, chunks
# added by the instruction offset), and the same for the dword units
PLACED_X4: Tuple[Tuple[int, int], ...] = ((10, 0), (8, 1), (8, 2))
PLACED_DWORD: Tuple[Tuple[int, int], ...] = ((37, 0), (37, 3))

# bytes one wave moves through the LDS per round, per stage (stores,
# loads and DMA alike)
_BYTES_PER_WAVE_ROUND = (
    SLICE_BYTES + 64 * (2 * (1 + 8 + 2) + 2 * (2 + 8 + 4) + 16 + 12 + 12 + 16 + 32 + 16 + 16
                        + 16),
    4 * BANK_DWORDS + 64 * (4 * 10 + 8 * 6 + 16 * 6 + 12 + 3 * 8),
    2 * (3 * 1024 + 2 * 256) + 2 * (2 * 1024 + 2 * 256),
    2 * SLICE_BYTES * 4,
)


def tag(a):
    """The tag of absolute dword address ``a`` (an int or an array):
    what is XORed into every value stored there."""
    import numpy as np

    a = np.asarray(a, dtype=np.uint32)
    with np.errstate(over="ignore"):
        t = _fmix32(np.atleast_1d(np.uint32(0xA5A5A5A5) ^ (a * np.uint32(0x9E3779B9))))
    return t.reshape(a.shape) if a.shape else int(t[0])


def source_tables(seed: int):
    """The two read-only tables of stage dma as one uint32 array of
    TABLE_DWORDS: G[16][2560] (tagged, one part per wave slot), then
    X[4096] (untagged)."""
    import numpy as np

    seed = int(seed) & _M32
    zero = np.uint32(0)
    with np.errstate(over="ignore"):
        g = _fmix32(_base(seed, _STAGE_G, zero) + np.arange(SLICE_DWORDS, dtype=np.uint32))
        x = _fmix32(_base(seed, _STAGE_X, zero) + np.arange(X_DWORDS, dtype=np.uint32))
    tags = tag(np.arange(G_DWORDS, dtype=np.uint32))
    return np.concatenate([np.tile(g, WAVES_PER_BLOCK) ^ tags, x])


def _plain_tables(seed: int):
    """(g [2560], X [4096]) without tags."""
    import numpy as np

    t = source_tables(seed)
    return t[:SLICE_DWORDS] ^ tag(np.arange(SLICE_DWORDS, dtype=np.uint32)), t[G_DWORDS:]


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

    def img(self):
        """uint32 [rounds, SLICE_DWORDS]"""
        import numpy as np

        idx = np.uint32(_IMG0) + np.arange(SLICE_DWORDS, dtype=np.uint32)
        with np.errstate(over="ignore"):
            return _fmix32(self.base[:, None] + idx[None, :])

    def rot(self, k: int):
        """int64 [rounds, 64]: lane (l + u(k)) mod 64"""
        import numpy as np

        return ((self.lane[None, :] + self.u(k)[:, None]) & np.uint32(63)).astype(np.int64)


class _Slice:
    """One slice as a little-endian byte array per round: uint8 [rounds,
    SLICE_BYTES].  Addresses are int64 [rounds, 64] or [64]."""

    def __init__(self, rounds: int):
        import numpy as np

        self.mem = np.zeros((rounds, SLICE_BYTES), dtype=np.uint8)

    def _addr(self, addr):
        import numpy as np

        addr = np.broadcast_to(np.asarray(addr, dtype=np.int64), (len(self.mem), 64))
        if addr.min() < 0 or addr.max() >= SLICE_BYTES:
            raise ValueError("ldscheck: address outside the slice")
        return addr

    def fill(self, d0: int, words):
        """dwords d0 .. of every round from uint32 [rounds, n]"""
        import numpy as np

        raw = np.ascontiguousarray(words.astype("<u4")).view(np.uint8)
        self.mem[:, 4 * d0:4 * d0 + raw.shape[1]] = raw

    def store(self, addr, value, nbytes: int):
        """the low ``nbytes`` bytes of uint32 [rounds, 64] at byte ``addr``"""
        import numpy as np

        addr = self._addr(addr)
        for b in range(nbytes):
            byte = ((value >> np.uint32(8 * b)) & np.uint32(0xFF)).astype(np.uint8)
            np.put_along_axis(self.mem, addr + b, byte, axis=1)

    def load(self, addr, nbytes: int):
        """uint32 [rounds, 64]: ``nbytes`` bytes at byte ``addr``, zero-extended"""
        import numpy as np

        addr = self._addr(addr)
        out = np.zeros(addr.shape, dtype=np.uint32)
        for b in range(nbytes):
            out |= np.take_along_axis(self.mem, addr + b, axis=1).astype(np.uint32) \
                << np.uint32(8 * b)
        return out

    def store_dwords(self, d, values):
        for c, v in enumerate(values):
            self.store(4 * (d + c), v, 4)

    def load_dwords(self, d, n: int):
        return [self.load(4 * (d + c), 4) for c in range(n)]


def _sext(x, bits: int):
    """Sign-extend the low ``bits`` of uint32 values."""
    import numpy as np

    m = np.uint32(1 << (bits - 1))
    with np.errstate(over="ignore"):
        return ((x & np.uint32((1 << bits) - 1)) ^ m) - m


def transposed_read(mem, addr):
    """ds_read_b64_tr_b16 on a little-endian byte array: ``mem`` uint8
    [rounds, bytes] or [bytes], ``addr`` the 64 lanes' byte addresses
    (8-byte aligned), [rounds, 64] or [64].  Within each group of 16
    lanes, lane 4 q + p supplies row q, columns 4 p .. 4 p + 3 of a 4 x 16
    block of 16-bit elements, and lane i receives column i with row q in
    its element q.  Returns (elements 0 and 1, elements 2 and 3) packed
    little-endian into uint32, shaped like ``addr``."""
    import numpy as np

    mem = np.asarray(mem, dtype=np.uint8)
    addr = np.asarray(addr, dtype=np.int64)
    flat = mem.ndim == 1
    mem2 = np.atleast_2d(mem)
    addr2 = np.broadcast_to(np.atleast_2d(addr), (len(mem2), 64))
    if (addr2 & 7).any():
        raise ValueError("ldscheck: transposed read needs 8-byte aligned addresses")
    lane = np.arange(64)
    group, i = lane & ~15, lane & 15
    elems = []
    for q in range(4):
        src = group + 4 * q + (i >> 2)  # the lane that supplied this element's row piece
        byte = addr2[:, src] + 2 * (i & 3)[None, :]
        lo = np.take_along_axis(mem2, byte, axis=1).astype(np.uint32)
        hi = np.take_along_axis(mem2, byte + 1, axis=1).astype(np.uint32)
        elems.append(lo | (hi << np.uint32(8)))
    a = elems[0] | (elems[1] << np.uint32(16))
    b = elems[2] | (elems[3] << np.uint32(16))
    return (a[0], b[0]) if flat and addr.ndim == 1 else (a, b)


def subdword_offsets(seed: int, r):
    """Where the narrow stores of stage width go in rounds ``r``: (byte
    within the dword [rounds, 2, 64], half within the dword [rounds, 2,
    64]) for the two ds_write_b8 and the two ds_write_b16."""
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
    S = _Slice(len(W.base))
    lane = np.arange(64, dtype=np.int64)
    l32 = W.lane
    S.fill(0, W.img())
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

    def wide(name, d0, step, first, n_store, rots):
        S.store_dwords(d0 + step * lane, [W.v(first + c) for c in range(n_store)])
        for tagname, k, n in rots:
            for c, v in enumerate(S.load_dwords(d0 + step * W.rot(k), n)):
                out.append((f"{name}{tagname}.{c}", v))

    wide("b64", 256, 2, 7, 2, (("", 6, 2),))
    wide("b96", 384, 4, 9, 3, (("", 12, 3), (".b128", 13, 4)))
    wide("b128", 640, 4, 14, 4, (("", 18, 4),))
    wide("rw2", 897, 2, 19, 2, (("", 21, 2),))
    S.store(4 * (1088 + lane), W.v(22), 4)
    S.store(4 * (1088 + 64 * ST64_K + lane), W.v(23), 4)
    out.append(("st64.0", S.load(4 * (1088 + W.rot(24)), 4)))
    out.append(("st64.1", S.load(4 * (1088 + 64 * ST64_K + W.rot(24)), 4)))
    for t in range(2):
        addr = 8 * (W.v(25 + t) % np.uint32(SLICE_BYTES // 8)).astype(np.int64)
        a, b = transposed_read(S.mem, addr)
        out.append((f"tr16.{t}.lo", a))
        out.append((f"tr16.{t}.hi", b))
    return out


def scatter_rows(seed: int, p: int, r):
    """The row lane l of scatter ``p`` writes in rounds ``r``: int64
    [rounds, 64], a bijection of 0..63."""
    import numpy as np

    W = _Words(int(seed) & _M32, 1, r)
    u = W.u(26 + 2 * p)
    with np.errstate(over="ignore"):
        row = ((u | np.uint32(1))[:, None] * W.lane[None, :] + (u >> np.uint32(8))[:, None])
    return (row & np.uint32(63)).astype(np.int64)


def gather_indices(seed: int, r):
    """The dwords the free gather of stage bank reads: int64 [rounds, 64]."""
    import numpy as np

    W = _Words(int(seed) & _M32, 1, r)
    return (W.v(25) & np.uint32(BANK_DWORDS - 1)).astype(np.int64)


def _stage_bank(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 1, r)
    S = _Slice(len(W.base))
    lane = np.arange(64, dtype=np.int64)
    S.fill(0, W.img()[:, :BANK_DWORDS])
    out = []

    def strided(j, stride, units):
        with np.errstate(over="ignore"):
            x = W.lane[None, :] * np.uint32(stride) + W.u(j)[:, None]
        return (x & np.uint32(units - 1)).astype(np.int64)

    for j, s in enumerate(B32_STRIDES):
        out.append((f"b32.s{s}", S.load(4 * strided(j, s, BANK_DWORDS), 4)))
    for j, s in enumerate(WIDE_STRIDES):
        for c, v in enumerate(S.load_dwords(2 * strided(10 + j, s, BANK_DWORDS // 2), 2)):
            out.append((f"b64.s{s}.{c}", v))
    for j, s in enumerate(WIDE_STRIDES):
        for c, v in enumerate(S.load_dwords(4 * strided(16 + j, s, BANK_DWORDS // 4), 4)):
            out.append((f"b128.s{s}.{c}", v))
    same = (W.u(22) & np.uint32(BANK_DWORDS - 1)).astype(np.int64)
    out.append(("broadcast", S.load(4 * np.repeat(same[:, None], 64, axis=1), 4)))
    two = np.where((lane & 1)[None, :] == 0, W.u(23)[:, None], W.u(24)[:, None])
    out.append(("two", S.load(4 * (two & np.uint32(BANK_DWORDS - 1)).astype(np.int64), 4)))
    out.append(("gather", S.load(4 * gather_indices(seed, r), 4)))
    for p, (stride, offset) in enumerate(SCATTERS):
        S.store(4 * (stride * scatter_rows(seed, p, r) + offset), W.v(27 + 2 * p), 4)
        out.append((f"scatter{p}.s{stride}", S.load(4 * (stride * lane + offset), 4)))
    return out


def dma_plan(seed: int, r):
    """The data-driven choices of stage dma in rounds ``r``, as int64
    arrays: placed_x4 [rounds, 3] and gather_x4_dst [rounds, 2] in chunks
    of CHUNK_DWORDS, placed_dword [rounds, 2] and gather_dword_dst
    [rounds, 2] in units of UNIT_DWORDS, gather_x4_src and
    gather_dword_src [rounds, 2, 64] as dword indices into X."""
    import numpy as np

    W = _Words(int(seed) & _M32, 2, r)
    i64 = lambda x: x.astype(np.int64)  # noqa: E731
    px4 = [i64(W.u(k) % np.uint32(m)) + add
           for k, (m, add) in zip((0, 1, 1), PLACED_X4)]
    pdw = [i64(W.u(2) % np.uint32(m)) + add for m, add in PLACED_DWORD]
    return {
        "placed_x4": np.stack(px4, axis=1),
        "placed_dword": np.stack(pdw, axis=1),
        "gather_x4_src": np.stack([i64(W.v(3 + g) & np.uint32(X_DWORDS - 4))
                                   for g in range(2)], axis=1),
        "gather_x4_dst": np.stack([i64(W.u(5 + g) % np.uint32(10)) for g in range(2)], axis=1),
        "gather_dword_src": np.stack([i64(W.v(7 + g) & np.uint32(X_DWORDS - 1))
                                      for g in range(2)], axis=1),
        "gather_dword_dst": np.stack([i64(W.u(9 + g) % np.uint32(40)) for g in range(2)],
                                     axis=1),
    }


def placed_m0_bases(seed: int, r, wave: int):
    """The byte addresses in M0 for the five placed copies of wave slot
    ``wave`` in rounds ``r``: int64 [rounds, 5]."""
    import numpy as np

    plan = dma_plan(seed, r)
    x4 = plan["placed_x4"] - np.array([add for _, add in PLACED_X4])
    dw = plan["placed_dword"] - np.array([add for _, add in PLACED_DWORD])
    return 4 * (SLICE_DWORDS * int(wave)
                + np.concatenate([CHUNK_DWORDS * x4, UNIT_DWORDS * dw], axis=1))


def _stage_dma(seed: int, r) -> List[tuple]:
    import numpy as np

    g, X = _plain_tables(seed)
    plan = dma_plan(seed, r)
    n = len(plan["placed_x4"])
    S = _Slice(n)
    lane = np.arange(64, dtype=np.int64)
    out = []
    # placed: the copied chunks hold g at the same dwords
    S.fill(0, np.repeat(g[None, :], n, axis=0))
    for j in range(3):
        d = CHUNK_DWORDS * plan["placed_x4"][:, j, None] + 4 * lane[None, :]
        for c, v in enumerate(S.load_dwords(d, 4)):
            out.append((f"placed.x4.{j}.{c}", v))
    for j in range(2):
        d = UNIT_DWORDS * plan["placed_dword"][:, j, None] + lane[None, :]
        out.append((f"placed.dword.{j}", S.load(4 * d, 4)))
    for gi in range(2):
        src = plan["gather_x4_src"][:, gi]
        d = CHUNK_DWORDS * plan["gather_x4_dst"][:, gi, None] + 4 * lane[None, :]
        S.store_dwords(d, [X[src + c] for c in range(4)])
        for c, v in enumerate(S.load_dwords(d, 4)):
            out.append((f"gather.x4.{gi}.{c}", v))
    for gi in range(2):
        d = UNIT_DWORDS * plan["gather_dword_dst"][:, gi, None] + lane[None, :]
        S.store(4 * d, X[plan["gather_dword_src"][:, gi]], 4)
        out.append((f"gather.dword.{gi}", S.load(4 * d, 4)))
    return out


def xwave_partners(wave: int, r: int) -> Tuple[int, int, int]:
    """The three waves whose slices wave ``wave`` reads in round ``r``."""
    rp = int(r) % PERIOD
    return tuple((int(wave) + 1 + (3 * rp + j) % 15) % 16 for j in range(3))


def _stage_xwave(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 3, r)
    img = W.img()
    out = []
    for phase, image in enumerate((img, ~img)):
        for j in range(3):
            for t in range(SLICE_DWORDS // 256):
                for c in range(4):
                    out.append((f"p{phase}.j{j}.t{t}.{c}",
                                image[:, 256 * t + c:256 * (t + 1):4]))
    return out


_STAGE_FUNCS = (_stage_width, _stage_bank, _stage_dma, _stage_xwave)


def _stage(seed: int, stage: int, r) -> List[tuple]:
    """[(slot name, uint32 [rounds, 64])] of a stage for rounds ``r``
    (uint32 array), in slot order."""
    if stage not in range(len(STAGES)):
        raise ValueError(f"ldscheck: stage {stage} out of range 0..3")
    return _STAGE_FUNCS[stage](seed, r)


def slot_table(stage: int) -> List[str]:
    """The name of every result slot of a stage, in slot order."""
    return [name for name, _ in _stage(0, int(stage), _shared.one_round("ldscheck", 0))]


def reference_values(seed: int, stage: int, r: int):
    """What a wave folds in one stage and round: {slot name: uint32[64]},
    in slot order, exact per lane and the same for every wave."""
    slots = _stage(int(seed) & _M32, int(stage), _shared.one_round("ldscheck", r))
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
class LdscheckResult(DigestResult):
    # Whole-run lower bounds per stage in GB/s of LDS traffic (stores,
    # loads and DMA; the kernel's time also holds operand generation, the
    # other stages and the digests): informative.
    width_gbps: float = 0.0
    bank_gbps: float = 0.0
    dma_gbps: float = 0.0
    xwave_gbps: float = 0.0


def _tables(seed: int, device):
    import numpy as np
    import torch

    return torch.from_numpy(source_tables(seed).view(np.int32).copy()).to(device)


def ldscheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> LdscheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup uses a CU's whole LDS, so on an idle GPU the default grid
    lands one workgroup on every CU; ``cus_covered`` reports how many
    distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot break an
    LDS bank."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"ldscheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"ldscheck: blocks must be in 0..4096, got {blocks}")
    if not 0 <= seed <= _M32:
        raise ValueError("ldscheck: seed must be a u32")
    return _shared.run_probe(
        "ldscheck", LdscheckResult(rounds=rounds), STAGES, _BYTES_PER_WAVE_ROUND, 1e9,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected, _tables(seed, _device(device)))


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``ldscheck`` with its dump pointer set."""
    return _shared.wave_digests(
        "ldscheck", _ext().ldscheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device, _tables(seed, _device(device)))


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
        raw = _ext().ldscheck_values(int(seed), stage, int(r), _tables(seed, device),
                                     int(wave)).cpu().numpy()
    return _shared.value_rows("ldscheck", raw.view(np.uint32), names, _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def run_ldscheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                            timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the ldscheck CLI."""
    return _active.run_probe_subprocess("ldscheck", index, "--rounds", rounds, timeout_s)


def ldscheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                   rounds: int = DEFAULT_ROUNDS,
                   max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("ldscheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "ldscheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: ldscheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
