"""Active probe for the cross-lane data paths — wrapper over the
lanecheck HIP kernel.

``cucheck``, ``mxcheck``, ``fpcheck`` and ``atomcheck`` never move a
value from one lane of a wave to another as workload (their only
cross-lane traffic is the butterfly that adds up a digest), and the
hardware that does so is a block of its own: the DPP network in front of
the vector ALUs, the LDS crossbar used without memory, the path from a
vector register through a scalar register and back, and gfx950's
permlane swaps.  Every softmax, layer norm, top-k, wave-level reduction
and scan, every MFMA layout transpose and every wave-aggregated atomic
goes through them; a bad select line in one SIMD's DPP mux, or a crossbar
port that returns the neighbour's dword, corrupts such results silently
and ECC does not see it.  Every op here is a permutation or a select, so
numpy is an exact reference.  ``lanecheck()`` launches one 16-wave
workgroup per compute unit; every wave runs the same deterministic
sequence of cross-lane operations and compares four 32-bit digests per
round with ``reference_digests``.  Launch shape, accounting and the
mismatch log (XCD, shader engine, shader array, CU, SIMD of the wave that
disagreed) are cucheck's.

The workload (csrc/lanecheck.hip; ``reference_values`` and
``reference_digests`` are the definition).  Integer arithmetic is mod
2**32; ``fmix32``, ``base``, ``salt`` are cucheck's and the stage number
fed to ``base`` is 24 + s.  Inputs repeat with PERIOD = 64 rounds:

  word(s, r, idx) = fmix32(base(seed, 24 + s, r % PERIOD) + idx)

*Operand slot* k is the per-lane value v(k)[l] = word(64 k + l); u(k) =
word(64 k) is a wave-uniform word (it equals v(k)[0]).  No input depends
on the wave number, so the table is the same for every wave.  A wave has
64 lanes, in four *rows* of 16; the *bank* of lane i is (i & 15) >> 2.
Every op's result is a *result slot* n, a row of 64 u32, numbered in the
order below (``slot_table``).

Stages (STAGES) and what they run:

  dpp   entry j of DPP_TABLE = (ctrl, row_mask, bank_mask, bound_ctrl) is
        v_mov_b32_dpp with old = v(2 j), src = v(2 j + 1); result slot j.
        ``dpp_source(ctrl, i)`` is the lane that lane i reads, or None:
          quad_perm [a, b, c, d]  lane 4 q + k reads lane 4 q + [a, b, c, d][k]
          row_shl:n   i + n, row_shr:n  i - n, within the row, else None
          row_ror:n   the row rotated right: (i - n) mod 16 of the row
          wave_shl:1  i + 1, wave_shr:1  i - 1 across the wave, else None
          wave_rol:1  (i + 1) mod 64, wave_ror:1  (i - 1) mod 64
          row_mirror  15 - i within the row, row_half_mirror  7 - i
                      within the half row
          row_bcast:15  lane 15 of row k for every lane of row k + 1; row
                      0 has None
          row_bcast:31  lane 31 for rows 2 and 3; rows 0 and 1 have None
          row_newbcast:n  lane n of the lane's own row
        A lane whose row bit (row_mask >> row) or bank bit (bank_mask >>
        bank) is clear keeps old.  An enabled lane with a source gets
        src[source]; with None it gets 0 if bound_ctrl, else it keeps
        old.  The table holds every control family, the shifts with both
        bound_ctrl settings, row_bcast:15 / 31 only with the row masks
        0xA / 0xC that scans use, and seven entries with partial masks.
  xbar  operand slots: gather g takes 2 g (data) and 2 g + 1 (indices),
        scatter p takes 8 + 2 p (data) and u(9 + 2 p), swizzle s takes
        14 + s.
        Four ds_bpermute gathers: lane i gets data[idx[i] mod 64], the
        byte address being 4 * (idx & 63) for g = 0 .. 2 and 4 * (idx &
        0x3FFF) for g = 3, since the hardware takes the index mod 64;
        sources may collide or go unused.
        Three ds_permute scatters: lane l sends data[l] to lane (a l + b)
        mod 64 with a = u | 1, b = u >> 8: a bijection.
        The ds_swizzle patterns of SWIZZLES (the instruction's 16-bit
        offset): bit mode, bit 15 clear, within each group of 32 lanes
        lane i reads lane ((i & and) | or) ^ xor with and = bits 4..0, or
        = bits 9..5, xor = bits 14..10 — SWAP 1, 2, 4, 8, 16, REVERSE
        within 32, and lane 3 of every group of 8 broadcast; quad-perm
        mode, bit 15 set, selects in bits 7..0 as in DPP — [3, 2, 1, 0]
        and [1, 1, 3, 0].
  sgpr  v_readlane of v(0), v(1) at the constant lanes READLANES; four
        v_readlane of v(2 + 2 i) at a uniform run-time index: u(3 + 2 i)
        & 63 for i = 0 .. 2, and for i = 3 (round 0's u(9) + r % PERIOD)
        & 63, which walks through all 64 lanes in a period;
        v_readfirstlane of v(10) inside ``if (lane >= t)``, t = 1 + u(11)
        % 62 (so 1 <= t <= 62: both sides of the branch have lanes):
        lanes t .. 63 get v(10)[t], the others v(12)[l];
        the ballots of v(13)[l] & 1 and of v(14)[l] >> 31, each as a slot
        of its low and a slot of its high 32 bits, the same in every lane;
        v_mbcnt_lo / hi of the second ballot: the number of its set bits
        in lanes below l;
        v_permlane16_swap(A = v(15), B = v(16)): rows 1 and 3 of A swap
        with rows 0 and 2 of B, both results are slots;
        v_permlane32_swap(A = v(17), B = v(18)): lanes 32..63 of A swap
        with lanes 0..31 of B, both results are slots.  fi and bound_ctrl
        are false.
  scan  the dependent chains workloads run.  Inclusive prefix sum of v(0)
        over the 64 lanes: x += dpp(old 0, x) for row_shr 1, 2, 4, 8,
        then row_bcast:15 (row mask 0xA) and row_bcast:31 (row mask 0xC),
        as rocPRIM and LLVM's atomic optimiser do; its exclusive form
        through wave_shr:1 with old 0; all-reduce sum of v(1), umin of
        v(2), umax of v(3), xor of v(4) by an xor butterfly over lane
        distances 1, 2 (DPP quad_perm), 4, 8, 16 (ds_swizzle), 32
        (ds_bpermute), the result in every lane; per-row sum of v(5) by
        row_ror 8, 4, 2, 1, the result in every lane of the row.

Digest of a stage: sum over slots n and lanes l of fmix32(value_n[l] +
salt(64 n + l)), mod 2**32.

Not covered: v_writelane (no builtin in this compiler, and no inline
assembly here), ds_bpermute from EXEC-disabled lanes, ds_permute scatter
collisions (which lane wins is not defined), fi / bound_ctrl on the
permlane swaps, SDWA, 64-bit DPP, row_bcast without the scans' row masks.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.lanecheck --device INDEX [--rounds N] [--seed S]
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

STAGES: Tuple[str, ...] = ("dpp", "xbar", "sgpr", "scan")
PERIOD = 64  # inputs of round r are those of round r % PERIOD
_STAGE0 = 24  # stage number fed to base() is _STAGE0 + s
# One default launch should hold the GPU for roughly half a second.
# Measured on MI355X (profiles/lanecheck_mi355x.json), default grid (256
# workgroups, 4096 waves): 10.94, 10.37 and 10.13 us per round at 1024,
# 4096 and 16384 rounds (the fixed cost of a launch fades), so 0.5 s are
# 49345 rounds; the nearest multiple of PERIOD, 771 x 64 = 49344 rounds,
# takes 0.500 s (0.4996 measured).  The numpy table costs about 0.01 s
# of host time whatever the rounds, since only PERIOD rows are computed.
DEFAULT_ROUNDS = 49344
_VALUE_ROWS = 48

_M32 = 0xFFFFFFFF


# -- control tables (csrc/lanecheck.hip holds the same) --------------------------------

def quad_perm(a: int, b: int, c: int, d: int) -> int:
    return a | (b << 2) | (c << 4) | (d << 6)


def row_shl(n: int) -> int:
    return 0x100 + n


def row_shr(n: int) -> int:
    return 0x110 + n


def row_ror(n: int) -> int:
    return 0x120 + n


def row_newbcast(n: int) -> int:
    return 0x150 + n


WAVE_SHL1, WAVE_ROL1, WAVE_SHR1, WAVE_ROR1 = 0x130, 0x134, 0x138, 0x13C
ROW_MIRROR, ROW_HALF_MIRROR, ROW_BCAST15, ROW_BCAST31 = 0x140, 0x141, 0x142, 0x143

# (ctrl as the instruction encodes it, row_mask, bank_mask, bound_ctrl)
DPP_TABLE: Tuple[Tuple[int, int, int, int], ...] = (
    (quad_perm(3, 2, 1, 0), 0xF, 0xF, 0),
    (quad_perm(1, 0, 3, 2), 0xF, 0xF, 0),
    (quad_perm(0, 0, 2, 2), 0xF, 0xF, 0),
    (row_shl(1), 0xF, 0xF, 0),
    (row_shl(1), 0xF, 0xF, 1),
    (row_shl(3), 0xF, 0xF, 1),
    (row_shl(15), 0xF, 0xF, 0),
    (row_shr(1), 0xF, 0xF, 1),
    (row_shr(1), 0xF, 0xF, 0),
    (row_shr(2), 0xF, 0xF, 0),
    (row_shr(4), 0xF, 0xF, 1),
    (row_shr(8), 0xF, 0xF, 0),
    (row_ror(1), 0xF, 0xF, 0),
    (row_ror(5), 0xF, 0xF, 0),
    (row_ror(12), 0xF, 0xF, 0),
    (WAVE_SHL1, 0xF, 0xF, 0),
    (WAVE_SHL1, 0xF, 0xF, 1),
    (WAVE_ROL1, 0xF, 0xF, 0),
    (WAVE_SHR1, 0xF, 0xF, 1),
    (WAVE_SHR1, 0xF, 0xF, 0),
    (WAVE_ROR1, 0xF, 0xF, 0),
    (ROW_MIRROR, 0xF, 0xF, 0),
    (ROW_HALF_MIRROR, 0xF, 0xF, 0),
    (ROW_BCAST15, 0xA, 0xF, 0),
    (ROW_BCAST31, 0xC, 0xF, 0),
    (row_newbcast(0), 0xF, 0xF, 0),
    (row_newbcast(5), 0xF, 0xF, 0),
    (row_newbcast(15), 0xF, 0xF, 0),
    # partial masks
    (row_shl(1), 0x5, 0xF, 1),
    (row_shr(1), 0xF, 0x3, 0),
    (quad_perm(2, 3, 0, 1), 0xA, 0x5, 0),
    (row_ror(5), 0xC, 0xE, 0),
    (ROW_MIRROR, 0x5, 0xE, 0),
    (WAVE_SHR1, 0xA, 0x3, 1),
    (row_newbcast(9), 0xC, 0x5, 0),
)


def swizzle_bits(and_mask: int, or_mask: int, xor_mask: int) -> int:
    return and_mask | (or_mask << 5) | (xor_mask << 10)


def swizzle_quad(a: int, b: int, c: int, d: int) -> int:
    return 0x8000 | quad_perm(a, b, c, d)


# ds_swizzle offsets, in slot order
SWIZZLES: Tuple[int, ...] = (
    swizzle_bits(0x1F, 0, 1), swizzle_bits(0x1F, 0, 2), swizzle_bits(0x1F, 0, 4),
    swizzle_bits(0x1F, 0, 8), swizzle_bits(0x1F, 0, 16),
    swizzle_bits(0x1F, 0, 0x1F),  # reverse within 32
    swizzle_bits(0x18, 3, 0),  # lane 3 of every group of 8, broadcast
    swizzle_quad(3, 2, 1, 0),
    swizzle_quad(1, 1, 3, 0),
)

# constant v_readlane indices
READLANES: Tuple[int, ...] = (17, 63)

_N_BPERMUTE, _N_PERMUTE, _N_READLANE_DYN = 4, 3, 4

# lane-level cross-lane operations one wave issues per round, per stage
# (a wave instruction counts 64): the butterflies of scan have 6 steps
_OPS_PER_WAVE_ROUND = (
    64 * len(DPP_TABLE),
    64 * (_N_BPERMUTE + _N_PERMUTE + len(SWIZZLES)),
    64 * (len(READLANES) + _N_READLANE_DYN + 1 + 2 + 2 + 2 + 2),
    64 * (6 + 1 + 4 * 6 + 4),
)


def dpp_source(ctrl: int, lane: int) -> Optional[int]:
    """The lane that lane ``lane`` reads under DPP control ``ctrl`` (the
    instruction's encoding), or None where it has no source."""
    ctrl, i = int(ctrl), int(lane)
    if not 0 <= i < 64:
        raise ValueError(f"lanecheck: lane {lane} out of range 0..63")
    row, pos = i & ~15, i & 15
    if 0 <= ctrl <= 0xFF:
        return (i & ~3) | ((ctrl >> (2 * (i & 3))) & 3)
    if 0x101 <= ctrl <= 0x10F:
        n = ctrl - 0x100
        return row + pos + n if pos + n <= 15 else None
    if 0x111 <= ctrl <= 0x11F:
        n = ctrl - 0x110
        return row + pos - n if pos >= n else None
    if 0x121 <= ctrl <= 0x12F:
        return row + ((pos - (ctrl - 0x120)) & 15)
    if ctrl == WAVE_SHL1:
        return i + 1 if i < 63 else None
    if ctrl == WAVE_ROL1:
        return (i + 1) & 63
    if ctrl == WAVE_SHR1:
        return i - 1 if i > 0 else None
    if ctrl == WAVE_ROR1:
        return (i - 1) & 63
    if ctrl == ROW_MIRROR:
        return row + 15 - pos
    if ctrl == ROW_HALF_MIRROR:
        return (i & ~7) + 7 - (i & 7)
    if ctrl == ROW_BCAST15:
        return row - 1 if row else None
    if ctrl == ROW_BCAST31:
        return 31 if i >= 32 else None
    if 0x150 <= ctrl <= 0x15F:
        return row + (ctrl - 0x150)
    raise ValueError(f"lanecheck: no DPP control 0x{ctrl:x}")


def swizzle_source(offset: int, lane: int) -> int:
    """The lane that lane ``lane`` reads under ds_swizzle offset
    ``offset``."""
    offset, i = int(offset), int(lane)
    if offset & 0x8000:
        return (i & ~3) | ((offset >> (2 * (i & 3))) & 3)
    and_mask, or_mask, xor_mask = offset & 31, (offset >> 5) & 31, (offset >> 10) & 31
    return (i & 32) | ((((i & 31) & and_mask) | or_mask) ^ xor_mask)


def _dpp_maps(entry):
    """(source lane or 0 [64], has a source [64], write-enabled [64]) of
    a DPP_TABLE entry, as numpy arrays."""
    import numpy as np

    ctrl, row_mask, bank_mask, _ = entry
    src = [dpp_source(ctrl, i) for i in range(64)]
    valid = np.array([s is not None for s in src])
    idx = np.array([s or 0 for s in src], dtype=np.int64)
    lane = np.arange(64)
    enabled = (((row_mask >> (lane >> 4)) & 1) != 0) & (((bank_mask >> ((lane & 15) >> 2)) & 1) != 0)
    return idx, valid, enabled


def _dpp(entry, old, src):
    """update_dpp on uint32 [rounds, 64] arrays."""
    import numpy as np

    idx, valid, enabled = _dpp_maps(entry)
    moved = src[:, idx]
    if entry[3]:
        moved = np.where(valid[None, :], moved, np.uint32(0))
        write = enabled
    else:
        write = enabled & valid
    return np.where(write[None, :], moved, old)


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


def _ctrl_name(ctrl: int) -> str:
    if ctrl <= 0xFF:
        return "quad_perm[%d,%d,%d,%d]" % tuple((ctrl >> s) & 3 for s in (0, 2, 4, 6))
    for lo, name in ((0x100, "row_shl"), (0x110, "row_shr"), (0x120, "row_ror"),
                     (0x150, "row_newbcast")):
        if lo <= ctrl <= lo + 15 and (ctrl > lo or lo == 0x150):
            return f"{name}:{ctrl - lo}"
    return {WAVE_SHL1: "wave_shl:1", WAVE_ROL1: "wave_rol:1", WAVE_SHR1: "wave_shr:1",
            WAVE_ROR1: "wave_ror:1", ROW_MIRROR: "row_mirror",
            ROW_HALF_MIRROR: "row_half_mirror", ROW_BCAST15: "row_bcast:15",
            ROW_BCAST31: "row_bcast:31"}[ctrl]


def _swizzle_name(offset: int) -> str:
    if offset & 0x8000:
        return "swizzle.quad[%d,%d,%d,%d]" % tuple((offset >> s) & 3 for s in (0, 2, 4, 6))
    return "swizzle.and%02x.or%02x.xor%02x" % (offset & 31, (offset >> 5) & 31,
                                               (offset >> 10) & 31)


def _rows(x):
    """A per-round uniform uint32 [rounds] in every lane."""
    import numpy as np

    return np.repeat(x[:, None], 64, axis=1)


def _stage_dpp(seed: int, r) -> List[tuple]:
    W = _Words(seed, 0, r)
    return [(f"{j}.{_ctrl_name(e[0])}.r{e[1]:x}.b{e[2]:x}.bc{e[3]}",
             _dpp(e, W.v(2 * j), W.v(2 * j + 1))) for j, e in enumerate(DPP_TABLE)]


def permute_destinations(seed: int, p: int, r):
    """Where lane l of scatter ``p`` sends its value in rounds ``r``:
    int64 [rounds, 64]."""
    import numpy as np

    W = _Words(seed, 1, r)
    u = W.u(9 + 2 * p).astype(np.uint64)
    lane = np.arange(64, dtype=np.uint64)
    return (((u | np.uint64(1))[:, None] * lane[None, :] + (u >> np.uint64(8))[:, None])
            & np.uint64(63)).astype(np.int64)


def bpermute_sources(seed: int, g: int, r):
    """The lane that lane l of gather ``g`` reads in rounds ``r``: int64
    [rounds, 64]."""
    import numpy as np

    W = _Words(seed, 1, r)
    mask = 0x3FFF if g == _N_BPERMUTE - 1 else 63
    return ((W.v(2 * g + 1) & np.uint32(mask)) & np.uint32(63)).astype(np.int64)


def _stage_xbar(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 1, r)
    out = []
    for g in range(_N_BPERMUTE):
        out.append((f"bpermute{g}",
                    np.take_along_axis(W.v(2 * g), bpermute_sources(seed, g, r), axis=1)))
    for p in range(_N_PERMUTE):
        data, res = W.v(8 + 2 * p), np.zeros((len(W.base), 64), dtype=np.uint32)
        np.put_along_axis(res, permute_destinations(seed, p, r), data, axis=1)
        out.append((f"permute{p}", res))
    for s, offset in enumerate(SWIZZLES):
        idx = np.array([swizzle_source(offset, i) for i in range(64)])
        out.append((f"{_swizzle_name(offset)}", W.v(14 + s)[:, idx]))
    return out


def readlane_indices(seed: int, r):
    """The four run-time v_readlane indices of rounds ``r``: int64
    [rounds, 4]."""
    import numpy as np

    W = _Words(seed, 2, r)
    cols = [W.u(3 + 2 * i) & np.uint32(63) for i in range(_N_READLANE_DYN - 1)]
    u0 = _Words(seed, 2, np.zeros(1, dtype=np.uint32)).u(3 + 2 * (_N_READLANE_DYN - 1))
    cols.append((u0 + W.rp) & np.uint32(63))
    return np.stack(cols, axis=1).astype(np.int64)


def readfirstlane_threshold(seed: int, r):
    """t of rounds ``r``: int64 [rounds], 1 <= t <= 62."""
    import numpy as np

    return (1 + _Words(seed, 2, r).u(11) % np.uint32(62)).astype(np.int64)


def _ballot(bits):
    """bool [rounds, 64] -> (lo, hi) uint32 [rounds]."""
    import numpy as np

    w = (bits.astype(np.uint64) << np.arange(64, dtype=np.uint64)[None, :]).sum(
        axis=1, dtype=np.uint64)
    return (w & np.uint64(_M32)).astype(np.uint32), (w >> np.uint64(32)).astype(np.uint32)


def _stage_sgpr(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 2, r)
    n = len(W.base)
    rounds = np.arange(n)
    out = []
    for i, idx in enumerate(READLANES):
        out.append((f"readlane.{idx}", _rows(W.v(i)[:, idx])))
    dyn = readlane_indices(seed, r)
    for i in range(_N_READLANE_DYN):
        out.append((f"readlane.u{i}", _rows(W.v(2 + 2 * i)[rounds, dyn[:, i]])))
    t = readfirstlane_threshold(seed, r)
    first = W.v(10)[rounds, t]
    out.append(("readfirstlane",
                np.where(np.arange(64)[None, :] >= t[:, None], first[:, None], W.v(12))))
    b0 = (W.v(13) & np.uint32(1)) != 0
    b1 = (W.v(14) >> np.uint32(31)) != 0
    for name, b in (("ballot0", b0), ("ballot1", b1)):
        lo, hi = _ballot(b)
        out.append((name + ".lo", _rows(lo)))
        out.append((name + ".hi", _rows(hi)))
    below = np.cumsum(b1, axis=1) - b1  # set bits in the lanes below
    out.append(("mbcnt", below.astype(np.uint32)))
    a, b = W.v(15), W.v(16)
    lane = np.arange(64)
    odd_row = ((lane >> 4) & 1) == 1
    # rows 1, 3 of A <-> rows 0, 2 of B
    out.append(("permlane16_swap.a", np.where(odd_row[None, :], b[:, (lane - 16) & 63], a)))
    out.append(("permlane16_swap.b", np.where(odd_row[None, :], b, a[:, (lane + 16) & 63])))
    a, b = W.v(17), W.v(18)
    upper = lane >= 32
    out.append(("permlane32_swap.a", np.where(upper[None, :], b[:, (lane - 32) & 63], a)))
    out.append(("permlane32_swap.b", np.where(upper[None, :], b, a[:, (lane + 32) & 63])))
    return out


def _stage_scan(seed: int, r) -> List[tuple]:
    import numpy as np

    W = _Words(seed, 3, r)
    zero = np.zeros((len(W.base), 64), dtype=np.uint32)
    x = W.v(0)
    with np.errstate(over="ignore"):
        for ctrl, row_mask in ((row_shr(1), 0xF), (row_shr(2), 0xF), (row_shr(4), 0xF),
                               (row_shr(8), 0xF), (ROW_BCAST15, 0xA), (ROW_BCAST31, 0xC)):
            x = x + _dpp((ctrl, row_mask, 0xF, 0), zero, x)
        out = [("scan.inclusive", x),
               ("scan.exclusive", _dpp((WAVE_SHR1, 0xF, 0xF, 0), zero, x))]
        out.append(("reduce.sum", _rows(W.v(1).sum(axis=1, dtype=np.uint32))))
        out.append(("reduce.umin", _rows(W.v(2).min(axis=1))))
        out.append(("reduce.umax", _rows(W.v(3).max(axis=1))))
        out.append(("reduce.xor", _rows(np.bitwise_xor.reduce(W.v(4), axis=1))))
        y = W.v(5).reshape(-1, 4, 16).sum(axis=2, dtype=np.uint32)
    out.append(("rowsum", np.repeat(y, 16, axis=1)))
    return out


_STAGE_FUNCS = (_stage_dpp, _stage_xbar, _stage_sgpr, _stage_scan)


def _stage(seed: int, stage: int, r) -> List[tuple]:
    """[(slot name, uint32 [rounds, 64])] of a stage for rounds ``r``
    (uint32 array), in slot order."""
    if stage not in range(len(STAGES)):
        raise ValueError(f"lanecheck: stage {stage} out of range 0..3")
    return _STAGE_FUNCS[stage](seed, r)


def slot_table(stage: int) -> List[str]:
    """The name of every result slot of a stage, in slot order."""
    return [name for name, _ in _stage(0, int(stage), _shared.one_round("lanecheck", 0))]


def reference_values(seed: int, stage: int, r: int):
    """What a wave folds in one stage and round: {slot name: uint32[64]},
    in slot order, exact per lane."""
    slots = _stage(int(seed) & _M32, int(stage), _shared.one_round("lanecheck", r))
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
class LanecheckResult(DigestResult):
    # Whole-run lower bounds per stage in 1e9 lane-level cross-lane
    # operations per second (the kernel's time also holds operand
    # generation, the other stages and the digests): informative.
    dpp_gops: float = 0.0
    xbar_gops: float = 0.0
    sgpr_gops: float = 0.0
    scan_gops: float = 0.0


def lanecheck(
    seed: int = 0,
    rounds: int = DEFAULT_ROUNDS,
    blocks: int = 0,
    max_records: int = 16,
    device=None,
    _inject: Optional[Tuple[int, int, int, int]] = None,
    _expected=None,
) -> LanecheckResult:
    """Run ``rounds`` rounds of the workload on ``blocks`` workgroups of
    16 waves (0 = one per CU) and compare every wave's digests with
    ``reference_digests``.

    A workgroup asks for a CU's whole LDS without touching it, so on an
    idle GPU the default grid lands one workgroup on every CU;
    ``cus_covered`` reports how many distinct CUs actually ran a wave.

    ``_inject=(global_wave, round, stage, xor_mask)`` flips bits of that
    one digest before the compare and ``_expected`` replaces the
    reference table; both are test hooks, since a test cannot break a
    lane mux."""
    rounds, blocks, seed = int(rounds), int(blocks), int(seed)
    if not 1 <= rounds <= 65536:
        raise ValueError(f"lanecheck: rounds must be in 1..65536, got {rounds}")
    if not 0 <= blocks <= 4096:
        raise ValueError(f"lanecheck: blocks must be in 0..4096, got {blocks}")
    return _shared.run_probe(
        "lanecheck", LanecheckResult(rounds=rounds), STAGES, _OPS_PER_WAVE_ROUND, 1e9,
        lambda: reference_digests(seed, rounds), seed, blocks, max_records, device,
        _inject, _expected)


def wave_digests(seed: int, rounds: int, blocks: int = 0, device=None):
    """What every wave computed, as uint32[blocks*16, rounds, 4] — the
    same kernel as ``lanecheck`` with its dump pointer set."""
    return _shared.wave_digests(
        "lanecheck", _ext().lanecheck_run, reference_digests(seed, rounds), STAGES,
        seed, rounds, blocks, device)


def wave_values(seed: int, stage: int, r: int, device=None):
    """What one wave folded for a stage and round, shaped like
    ``reference_values``: {slot name: uint32[64]}.  A digest cannot say
    which op moved what; this can."""
    import numpy as np
    import torch

    stage = int(stage)
    names = slot_table(stage)
    with torch.cuda.device(_device(device)):
        raw = _ext().lanecheck_values(int(seed), stage, int(r)).cpu().numpy()
    return _shared.value_rows("lanecheck", raw.view(np.uint32), names, _VALUE_ROWS, stage)


# -- child process -----------------------------------------------------------

def run_lanecheck_subprocess(index: int, rounds: int = DEFAULT_ROUNDS,
                             timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the lanecheck CLI."""
    return _active.run_probe_subprocess("lanecheck", index, "--rounds", rounds, timeout_s)


def lanecheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                    rounds: int = DEFAULT_ROUNDS,
                    max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, rounds)``."""
    return _active.probe_round("lanecheck", "mismatches", metric_args, manager,
                               runner, metrics, rounds, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "lanecheck", "--rounds", DEFAULT_ROUNDS,
        lambda args: lanecheck(seed=args.seed, rounds=args.rounds), argv)


if __name__ == "__main__":
    sys.exit(main())
