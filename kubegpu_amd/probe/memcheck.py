"""Active HBM integrity probe — wrapper over the memcheck HIP kernels.

The bandwidth probes verify that a placement delivers the bandwidth the
model promised; this is the same promise for memory correctness.  A GPU
whose HBM returns wrong data without moving the ECC counters (stuck
bits, address-line faults, pages not yet retired) still looks healthy
to passive monitoring.  ``memcheck()`` runs a moving-inversions pass
sequence over one buffer taken from free VRAM and reports every 32-bit
word that read back wrong.

Patterns (csrc/memcheck.hip; ``reference_words`` is the numpy
definition): ``v`` is the 64-bit index of a 16-byte vector, counted
from the buffer's first byte plus the caller's ``first_vector`` (0 by
default and in ``memcheck()``), ``j = 0..3`` the 32-bit word inside it.

  0 addr / 1 addr_inv      h = fmix32(lo32(v) ^ hi32(v)*0x9E3779B9 ^ seed)
                           word[j] = rotl32(h, 8j) ^ K[j]
  2 checker / 3 checker_inv  c = 0xAAAAAAAA (v even) / 0x55555555 (v odd)
                           word[j] = c (j even) / ~c (j odd); seed ignored
  4 walk1 / 5 walk0        word[j] = 1 << ((4v + j + seed) mod 32)

Odd ids are the bitwise complement of the even id below them.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.memcheck --device INDEX --bytes N [--seed S]
"""

from __future__ import annotations

import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional, Tuple, Union

from . import _active
from ._active import (  # noqa: F401
    EXIT_CANNOT_RUN,
    EXIT_MISMATCH,
    EXIT_PASS,
    _REPO_ROOT,
    _child_lock,
    _ext,
    idle_gpus,
)

PATTERNS: Tuple[str, ...] = (
    "addr", "addr_inv", "checker", "checker_inv", "walk1", "walk0",
)
_ADDR_K = (0x00000000, 0x9E3779B9, 0x7F4A7C15, 0xF39CC060)
# Infinity Cache size: a smaller buffer may be verified out of cache.
LLC_BYTES = 256 << 20
DEFAULT_BYTES = 1 << 30

Pattern = Union[int, str]


def pattern_id(pattern: Pattern) -> int:
    """Pattern name or id -> id (0..5)."""
    if isinstance(pattern, str):
        if pattern not in PATTERNS:
            raise ValueError(f"unknown memcheck pattern {pattern!r}; one of {PATTERNS}")
        return PATTERNS.index(pattern)
    pid = int(pattern)
    if not 0 <= pid < len(PATTERNS):
        raise ValueError(f"memcheck pattern id {pid} out of range 0..{len(PATTERNS) - 1}")
    return pid


def reference_words(first_vector: int, n_vectors: int, pattern: Pattern, seed: int):
    """Expected buffer contents as a flat uint32 array of 4*n_vectors
    words, for vectors first_vector .. first_vector+n_vectors-1.

    Pure numpy: needs neither torch nor a GPU.  This is the definition
    the GPU kernels are tested against."""
    import numpy as np

    pid = pattern_id(pattern)
    seed = int(seed) & 0xFFFFFFFF
    v = np.uint64(first_vector) + np.arange(n_vectors, dtype=np.uint64)
    out = np.empty((n_vectors, 4), dtype=np.uint32)
    family = pid >> 1
    if family == 0:
        lo = (v & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        hi = (v >> np.uint64(32)).astype(np.uint32)
        h = lo ^ (hi * np.uint32(0x9E3779B9)) ^ np.uint32(seed)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
        for j in range(4):
            r = h if j == 0 else (h << np.uint32(8 * j)) | (h >> np.uint32(32 - 8 * j))
            out[:, j] = r ^ np.uint32(_ADDR_K[j])
    elif family == 1:
        c = np.where((v & np.uint64(1)) == 0, np.uint32(0xAAAAAAAA), np.uint32(0x55555555))
        c = c.astype(np.uint32)
        out[:, 0] = c
        out[:, 1] = ~c
        out[:, 2] = c
        out[:, 3] = ~c
    else:
        for j in range(4):
            shift = (np.uint64(4) * v + np.uint64(j) + np.uint64(seed)) % np.uint64(32)
            out[:, j] = np.uint32(1) << shift.astype(np.uint32)
    if pid & 1:
        out = ~out
    return out.reshape(-1)


@dataclass
class VerifyResult:
    """Outcome of one verify pass over a buffer."""

    mismatched_words: int = 0
    first_bad_offset: Optional[int] = None  # bytes from the buffer start
    bad_bits_mask: int = 0  # OR of got ^ expected over all bad words
    # up to max_records (word_index, expected, got) tuples
    records: List[Tuple[int, int, int]] = field(default_factory=list)

    @property
    def ok(self) -> bool:
        return self.mismatched_words == 0


def _to_result(raw) -> VerifyResult:
    count, first_word, mask, records = raw
    return VerifyResult(
        mismatched_words=int(count),
        first_bad_offset=None if first_word < 0 else int(first_word) * 4,
        bad_bits_mask=int(mask),
        records=[(int(w), int(e), int(g)) for (w, e, g) in records],
    )


def first_vector_arg(first_vector: int, name: str = "first_vector") -> int:
    """A caller's first_vector as an int; negative raises ValueError
    before the extension is loaded."""
    first_vector = int(first_vector)
    if first_vector < 0:
        raise ValueError(f"{name} must not be negative, got {first_vector}")
    return first_vector


def fill_pattern(buf, pattern: Pattern, seed: int = 0, blocks: int = 0,
                 first_vector: int = 0) -> None:
    """Fill a contiguous GPU tensor (nbytes a positive multiple of 16)
    with a pattern.  The tensor's own first byte is vector
    ``first_vector`` of the pattern (``reference_words(first_vector,
    ...)``); first_vector + nbytes/16 may be at most 2**63."""
    pid, first = pattern_id(pattern), first_vector_arg(first_vector)
    _ext().fill_pattern(buf, pid, int(seed), int(blocks), first)


def verify_pattern(
    buf, pattern: Pattern, seed: int = 0, max_records: int = 16, blocks: int = 0,
    first_vector: int = 0,
) -> VerifyResult:
    """Read the buffer back and compare every word with the pattern
    counted from ``first_vector``.  Reported word indices and offsets
    are from the buffer start whatever first_vector is."""
    pid, first = pattern_id(pattern), first_vector_arg(first_vector)
    return _to_result(
        _ext().verify_pattern(buf, pid, int(seed), int(max_records), int(blocks), first)
    )


def verify_then_fill(
    buf,
    expect_pattern: Pattern,
    next_pattern: Pattern,
    seed: int = 0,
    max_records: int = 16,
    blocks: int = 0,
    first_vector: int = 0,
) -> VerifyResult:
    """One fused read-check-write pass: verify expect_pattern, leave
    next_pattern in every word whether or not it matched.  Both
    patterns count from ``first_vector``."""
    epid, npid = pattern_id(expect_pattern), pattern_id(next_pattern)
    first = first_vector_arg(first_vector)
    return _to_result(
        _ext().verify_then_fill(
            buf, epid, npid, int(seed), int(max_records), int(blocks), first,
        )
    )


@dataclass
class MemcheckResult:
    ok: bool = True
    bytes_tested: int = 0
    passes: int = 0
    mismatched_words: int = 0
    first_bad_offset: Optional[int] = None
    bad_bits_mask: int = 0
    # {"pass", "offset", "word_index", "expected", "got"} per logged word
    records: List[Dict[str, int]] = field(default_factory=list)
    records_dropped: int = 0
    elapsed_s: float = 0.0
    gbps: float = 0.0
    exceeds_llc: bool = False

    def to_dict(self) -> dict:
        return {
            "ok": bool(self.ok),
            "bytes_tested": int(self.bytes_tested),
            "passes": int(self.passes),
            "mismatched_words": int(self.mismatched_words),
            "first_bad_offset": self.first_bad_offset,
            "bad_bits_mask": int(self.bad_bits_mask),
            "records": [dict(r) for r in self.records],
            "records_dropped": int(self.records_dropped),
            "elapsed_s": float(self.elapsed_s),
            "gbps": float(self.gbps),
            "exceeds_llc": bool(self.exceeds_llc),
        }


# (expected pattern or None, next pattern or None): fill, five fused
# moving-inversions steps, final verify.
_PASS_SEQUENCE: Tuple[Tuple[Optional[str], Optional[str]], ...] = (
    (None, "addr"),
    ("addr", "addr_inv"),
    ("addr_inv", "checker"),
    ("checker", "checker_inv"),
    ("checker_inv", "walk1"),
    ("walk1", "walk0"),
    ("walk0", None),
)


def memcheck(
    nbytes: int = DEFAULT_BYTES,
    seed: int = 0,
    max_records: int = 16,
    device=None,
    _after_pass: Optional[Callable] = None,
) -> MemcheckResult:
    """Allocate one buffer from free VRAM and run the pass sequence
    fill(addr), verify_then_fill(addr->addr_inv), (addr_inv->checker),
    (checker->checker_inv), (checker_inv->walk1), (walk1->walk0),
    verify(walk0), accumulating the per-pass results.

    All accesses are nontemporal, but a buffer of at most 256 MiB can
    still be served from the Infinity Cache between passes, so such a
    run may verify the cache rather than HBM; ``exceeds_llc`` says which
    side of that line the run was on.  ``gbps`` is synchronised wall
    time over the bytes actually moved (12 x nbytes).  Records are
    capped at ``max_records`` per pass and overall.

    ``_after_pass(pass_index, buf)`` is a test hook called after every
    pass; it exists so a test can corrupt the buffer between passes.
    """
    import torch

    nbytes = int(nbytes)
    if nbytes <= 0 or nbytes % 16:
        raise ValueError(f"memcheck: nbytes must be a positive multiple of 16, got {nbytes}")
    ext = _ext()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    torch.cuda.synchronize(device)

    res = MemcheckResult(bytes_tested=nbytes, exceeds_llc=nbytes > LLC_BYTES)
    moved = 0
    for idx, (expect, nxt) in enumerate(_PASS_SEQUENCE):
        t0 = time.perf_counter()
        if expect is None:
            ext.fill_pattern(buf, pattern_id(nxt), seed, 0)
            torch.cuda.synchronize(device)
            vr = None
            moved += nbytes
        elif nxt is None:
            vr = _to_result(ext.verify_pattern(buf, pattern_id(expect), seed, max_records, 0))
            moved += nbytes
        else:
            vr = _to_result(
                ext.verify_then_fill(
                    buf, pattern_id(expect), pattern_id(nxt), seed, max_records, 0
                )
            )
            moved += 2 * nbytes
        res.elapsed_s += time.perf_counter() - t0
        res.passes += 1
        if vr is not None and vr.mismatched_words:
            res.mismatched_words += vr.mismatched_words
            res.bad_bits_mask |= vr.bad_bits_mask
            if res.first_bad_offset is None or vr.first_bad_offset < res.first_bad_offset:
                res.first_bad_offset = vr.first_bad_offset
            for word, expected, got in vr.records:
                if len(res.records) >= max_records:
                    break
                res.records.append({
                    "pass": idx, "offset": word * 4, "word_index": word,
                    "expected": expected, "got": got,
                })
        if _after_pass is not None:
            _after_pass(idx, buf)
            torch.cuda.synchronize(device)
    res.ok = res.mismatched_words == 0
    res.records_dropped = res.mismatched_words - len(res.records)
    res.gbps = moved / res.elapsed_s / 1e9 if res.elapsed_s > 0 else 0.0
    del buf
    return res


# -- child process -----------------------------------------------------------

def run_memcheck_subprocess(index: int, nbytes: int = DEFAULT_BYTES,
                            timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the memcheck CLI."""
    return _active.run_probe_subprocess("memcheck", index, "--bytes", nbytes, timeout_s)


def _metric_args(rec: dict) -> tuple:
    return int(rec["mismatched_words"]), float(rec.get("gbps", 0.0))


def memcheck_round(manager, runner: Callable[[int, int], dict], metrics=None,
                   nbytes: int = DEFAULT_BYTES,
                   max_process_count: Optional[int] = 0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, nbytes)``."""
    return _active.probe_round("memcheck", "mismatched_words", _metric_args, manager,
                               runner, metrics, nbytes, max_process_count)


def main(argv=None) -> int:
    return _active.probe_main(
        "memcheck", "--bytes", DEFAULT_BYTES,
        lambda args: memcheck(nbytes=args.bytes, seed=args.seed), argv)


if __name__ == "__main__":
    sys.exit(main())
