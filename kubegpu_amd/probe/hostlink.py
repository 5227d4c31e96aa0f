"""Active host-link integrity and bandwidth probe — wrapper over the
hostlink HIP kernels.

``memcheck`` asks whether HBM returns what was written and ``cucheck``
whether the compute units return right answers; this asks the same of
the path between the GPU and host memory: the PCIe endpoint, the root
port or switch above it, the IOMMU mapping, the runtime's copy path and
the host DRAM behind it.  ``hostlink()`` moves the memcheck patterns
over that path in both directions, with kernels that load and store
pinned host memory directly and with the runtime's own copies, and
reports every 32-bit word that arrived wrong together with the
bandwidth each way.

The patterns are memcheck's, unchanged; ``memcheck.reference_words``
is the one numpy definition (csrc/pattern_common.h on the GPU side).

What a verdict means: PCIe protects each link with its own CRC and
replay, so wrong data over a healthy link is rare; a mismatch is a
statement about the whole GPU-to-host path, not about one lane.  The
bandwidth figures describe the link as it was trained and loaded at
that moment — an idle GPU does not mean an idle host — so a figure
under ``min_gbps`` is reported (``below_floor``) and never makes a GPU
unhealthy.

CLI (one JSON line; exit 0 pass, 1 mismatches, 2 could not run):
    python -m kubegpu_amd.probe.hostlink --device INDEX [--bytes N]
        [--seed S] [--min-gbps X]
"""

from __future__ import annotations

import os
import re
import sys
import time
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

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
from .memcheck import (
    Pattern,
    VerifyResult,
    _to_result,
    first_vector_arg,
    pattern_id,
    reference_words,
)

# Pinned memory is a host resource on a node that runs pods: the default
# stays modest.
DEFAULT_BYTES = 256 << 20
# What crosses the link in each pass of hostlink(), in order.
PASS_PATHS = (
    "kernel_write", "kernel_read", "copy_h2d", "copy_d2h",
    "kernel_read", "host_write", "duplex", "kernel_read",
)
_SAMPLE_EDGE_BYTES = 4096  # CPU-checked head and tail of pass 0
_SAMPLE_VECTORS = 64  # plus this many vectors at seeded random positions
_HOST_WRITE_CHUNK_VECTORS = 1 << 16  # 1 MiB of pattern per numpy batch
_COPY_WARMUP_BYTES = 1 << 20  # untimed first copy each way


def _device_index(device) -> int:
    import torch

    if device is None:
        return int(torch.cuda.current_device())
    if isinstance(device, int):
        return device
    d = torch.device(device)
    return int(torch.cuda.current_device()) if d.index is None else int(d.index)


def default_blocks():
    """(DEFAULT_READ_BLOCKS, DEFAULT_WRITE_BLOCKS) of the built kernels:
    the grid per direction when ``blocks`` is 0."""
    ext = _ext()
    return int(ext.HOSTLINK_DEFAULT_READ_BLOCKS), int(ext.HOSTLINK_DEFAULT_WRITE_BLOCKS)


# -- thin wrappers -------------------------------------------------------------

def alloc(nbytes: int, device=None):
    """Pinned, mapped, fine-grained host memory as a CPU uint8 tensor
    (``.numpy()`` views it); freed with the tensor."""
    return _ext().hostlink_alloc(int(nbytes), _device_index(device))


def fill_pattern(host, pattern: Pattern, seed: int = 0, device=None, blocks: int = 0,
                 first_vector: int = 0) -> None:
    """The GPU stores a pattern straight into a pinned CPU tensor
    (contiguous, 16-byte aligned, nbytes a positive multiple of 16).
    The tensor's own first byte is vector ``first_vector`` of the
    pattern; first_vector + nbytes/16 may be at most 2**63.  Returns
    after the kernel has finished.  A pageable tensor raises
    RuntimeError."""
    pid, first = pattern_id(pattern), first_vector_arg(first_vector)
    _ext().hostlink_fill(host, pid, int(seed), _device_index(device), int(blocks), first)


def verify_pattern(host, pattern: Pattern, seed: int = 0, device=None,
                   max_records: int = 16, blocks: int = 0,
                   first_vector: int = 0) -> VerifyResult:
    """The GPU loads a pinned CPU tensor and compares every word with
    the pattern counted from ``first_vector``.  Reported word indices
    and offsets are from the tensor's first byte."""
    pid, first = pattern_id(pattern), first_vector_arg(first_vector)
    return _to_result(_ext().hostlink_verify(
        host, pid, int(seed), _device_index(device), int(max_records), int(blocks), first))


def duplex(read_host, read_pattern: Pattern, write_host, write_pattern: Pattern,
           seed: int = 0, device=None, max_records: int = 16,
           read_blocks: int = 0, write_blocks: int = 0,
           read_first_vector: int = 0, write_first_vector: int = 0) -> VerifyResult:
    """One launch that verifies ``read_host`` while it fills
    ``write_host``, so both directions of the link carry traffic at
    once.  The two tensors must not overlap; each is indexed from its
    own first byte, plus its own ``*_first_vector`` for the pattern.
    Returns the verify result of the read side."""
    rpid, wpid = pattern_id(read_pattern), pattern_id(write_pattern)
    rfirst = first_vector_arg(read_first_vector, "read_first_vector")
    wfirst = first_vector_arg(write_first_vector, "write_first_vector")
    return _to_result(_ext().hostlink_duplex(
        read_host, rpid, write_host, wpid, int(seed), _device_index(device),
        int(max_records), int(read_blocks), int(write_blocks), rfirst, wfirst))


# -- PCIe link state -------------------------------------------------------------

_SPEED_RE = re.compile(r"^\s*([0-9]+(?:\.[0-9]+)?)\s*GT/s")


def read_pcie_link(bdf: str, sysfs_root: str = "/sys") -> Optional[dict]:
    """Trained and maximum speed and width of a PCI device, and its NUMA
    node, read from sysfs; None if anything is missing or unparsable.
    ``downtrained`` says the link runs below its maximum speed or width.
    Informative only."""
    if not bdf:
        return None
    base = os.path.join(sysfs_root, "bus", "pci", "devices", bdf)

    def read(name: str) -> str:
        with open(os.path.join(base, name)) as f:
            return f.read().strip()

    def speed(name: str) -> float:
        m = _SPEED_RE.match(read(name))  # "32.0 GT/s PCIe"
        if m is None:
            raise ValueError(name)
        return float(m.group(1))

    try:
        out = {
            "speed_gts": speed("current_link_speed"),
            "max_speed_gts": speed("max_link_speed"),
            "width": int(read("current_link_width")),
            "max_width": int(read("max_link_width")),
            "numa_node": int(read("numa_node")),
        }
    except (OSError, ValueError):
        return None
    if out["width"] <= 0 or out["max_width"] <= 0:
        return None
    out["downtrained"] = (out["speed_gts"] < out["max_speed_gts"]
                          or out["width"] < out["max_width"])
    return out


def _device_bdf(index: int) -> str:
    import torch

    p = torch.cuda.get_device_properties(index)
    return "%04x:%02x:%02x.0" % (p.pci_domain_id, p.pci_bus_id, p.pci_device_id)


# -- the probe --------------------------------------------------------------------

ONE_WAY_FIGURES = ("kernel_h2d_gbps", "kernel_d2h_gbps", "copy_h2d_gbps", "copy_d2h_gbps")


def _below_floor(rec: dict, min_gbps: float) -> bool:
    """A floor above 0 with any one-way figure of the result dict under
    it; the duplex figure is not a one-way figure."""
    return min_gbps > 0 and any(
        rec.get(k) is not None and float(rec[k]) < min_gbps for k in ONE_WAY_FIGURES)


@dataclass
class HostlinkResult:
    ok: bool = True
    bytes_tested: int = 0
    passes: int = 0
    mismatched_words: int = 0  # found by the GPU, all passes
    first_bad_offset: Optional[int] = None  # bytes from the buffer start
    bad_bits_mask: int = 0
    # {"pass", "path", "offset", "word_index", "expected", "got"} per logged word
    records: List[Dict] = field(default_factory=list)
    records_dropped: int = 0
    cpu_sample_mismatches: int = 0  # found by the CPU in what the GPU wrote (pass 0)
    elapsed_s: float = 0.0  # sum of the timed passes
    kernel_h2d_gbps: float = 0.0  # GPU loads from host memory, best kernel_read pass
    kernel_d2h_gbps: float = 0.0  # GPU stores to host memory
    copy_h2d_gbps: float = 0.0  # the runtime's copy, host to device
    copy_d2h_gbps: float = 0.0
    duplex_gbps: float = 0.0  # read + written bytes over the one kernel's time
    min_gbps: float = 0.0
    below_floor: bool = False
    link: Optional[dict] = None  # read_pcie_link() of the GPU

    def apply_floor(self, min_gbps: float) -> None:
        """Set min_gbps and below_floor.  Never touches ok."""
        self.min_gbps = float(min_gbps)
        self.below_floor = _below_floor(self.to_dict(), self.min_gbps)

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
            "cpu_sample_mismatches": int(self.cpu_sample_mismatches),
            "elapsed_s": float(self.elapsed_s),
            "kernel_h2d_gbps": float(self.kernel_h2d_gbps),
            "kernel_d2h_gbps": float(self.kernel_d2h_gbps),
            "copy_h2d_gbps": float(self.copy_h2d_gbps),
            "copy_d2h_gbps": float(self.copy_d2h_gbps),
            "duplex_gbps": float(self.duplex_gbps),
            "min_gbps": float(self.min_gbps),
            "below_floor": bool(self.below_floor),
            "link": dict(self.link) if self.link is not None else None,
        }


def _sample_vectors(n_vectors: int, seed: int):
    """Sorted vector indices the CPU checks after pass 0: the first and
    the last 4 KiB and 64 seeded random positions."""
    import numpy as np

    edge = min(_SAMPLE_EDGE_BYTES // 16, n_vectors)
    rng = np.random.default_rng(int(seed))
    picks = rng.integers(0, n_vectors, size=_SAMPLE_VECTORS, dtype=np.int64)
    return np.unique(np.concatenate([
        np.arange(edge, dtype=np.int64),
        np.arange(n_vectors - edge, n_vectors, dtype=np.int64),
        picks,
    ]))


def _host_write(words, pattern: Pattern, seed: int) -> None:
    """The CPU writes a pattern into a uint32 numpy view, in batches."""
    n_vectors = len(words) // 4
    for v0 in range(0, n_vectors, _HOST_WRITE_CHUNK_VECTORS):
        n = min(_HOST_WRITE_CHUNK_VECTORS, n_vectors - v0)
        words[4 * v0:4 * (v0 + n)] = reference_words(v0, n, pattern, seed)


def hostlink(
    nbytes: int = DEFAULT_BYTES,
    seed: int = 0,
    max_records: int = 16,
    device=None,
    min_gbps: float = 0.0,
    _after_pass: Optional[Callable] = None,
) -> HostlinkResult:
    """Allocate one pinned host buffer H and one device buffer D of
    ``nbytes`` and run eight passes (``PASS_PATHS``):

      0 kernel_write  the GPU stores addr into H; the CPU checks a sample
      1 kernel_read   the GPU loads H and verifies addr
      2 copy_h2d      D.copy_(H), then memcheck verifies D == addr
      3 copy_d2h      memcheck fills D with addr_inv, then H.copy_(D)
      4 kernel_read   the GPU verifies H == addr_inv
      5 host_write    the CPU writes checker into H, the GPU verifies it
      6 duplex        one kernel verifies the lower half of H (checker)
                      while it fills the upper half with walk1
      7 kernel_read   the GPU verifies the upper half == walk1

    Only the transfer named by a pass is timed (perf_counter around a
    synchronised pass); the checks and fills on D and the CPU's own work
    are not.  Data the CPU wrote and only the GPU read (pass 5), and
    data the GPU wrote and the CPU read (the pass 0 sample), cannot be
    faked by a cache on the GPU side.

    ``ok`` is about data alone.  ``below_floor`` says a one-way figure
    was under ``min_gbps`` (0 = no floor) and never changes ``ok``.
    Records are capped at ``max_records`` per pass and overall; offsets
    are bytes from the start of H.

    ``_after_pass(pass_index, host_numpy_view)`` is a test hook called
    after every pass with the uint8 numpy view of H, so that a test can
    corrupt host memory between passes; the CPU's sample of pass 0 is
    taken after the hook.
    """
    import numpy as np
    import torch

    nbytes = int(nbytes)
    if nbytes <= 0 or nbytes % 32:
        raise ValueError(f"hostlink: nbytes must be a positive multiple of 32, got {nbytes}")
    seed = int(seed)
    max_records = int(max_records)
    ext = _ext()
    index = _device_index(device)
    dev = torch.device("cuda", index)
    H = ext.hostlink_alloc(nbytes, index)
    D = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    # The runtime sets its copy path up on a process's first copy each
    # way, and this probe is a process's whole life: warm both before
    # anything is timed, while neither buffer holds data yet.
    warm = min(nbytes, _COPY_WARMUP_BYTES)
    D[:warm].copy_(H[:warm], non_blocking=True)
    H[:warm].copy_(D[:warm])
    torch.cuda.synchronize(dev)
    view = H.numpy()
    half = nbytes // 2
    lower, upper = H[:half], H[half:]

    res = HostlinkResult(bytes_tested=nbytes)
    try:
        res.link = read_pcie_link(_device_bdf(index))
    except Exception:  # informative only
        res.link = None
    read_gbps: List[float] = []

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        res.elapsed_s += dt
        return out, dt

    def gbps(moved: int, dt: float) -> float:
        return moved / dt / 1e9 if dt > 0 else 0.0

    def record(idx: int, word: int, expected: int, got: int, base: int) -> None:
        if len(res.records) < max_records:
            res.records.append({
                "pass": idx, "path": PASS_PATHS[idx], "offset": base + word * 4,
                "word_index": (base + word * 4) // 4, "expected": expected, "got": got,
            })

    def first_bad(offset: int) -> None:
        if res.first_bad_offset is None or offset < res.first_bad_offset:
            res.first_bad_offset = offset

    def account(idx: int, vr: VerifyResult, base: int = 0) -> None:
        if not vr.mismatched_words:
            return
        res.mismatched_words += vr.mismatched_words
        res.bad_bits_mask |= vr.bad_bits_mask
        first_bad(base + vr.first_bad_offset)
        for word, expected, got in vr.records:
            record(idx, word, expected, got, base)

    def done(idx: int) -> None:
        res.passes += 1
        if _after_pass is not None:
            _after_pass(idx, view)
            torch.cuda.synchronize(dev)

    def kernel_read(idx: int, host, pattern: str, base: int = 0) -> None:
        raw, dt = timed(lambda: ext.hostlink_verify(
            host, pattern_id(pattern), seed, index, max_records, 0))
        read_gbps.append(gbps(host.nbytes, dt))
        account(idx, _to_result(raw), base)
        done(idx)

    # 0: GPU -> host stores, checked by the CPU
    _, dt = timed(lambda: ext.hostlink_fill(H, pattern_id("addr"), seed, index, 0))
    res.kernel_d2h_gbps = gbps(nbytes, dt)
    done(0)
    words = view.view(np.uint32)
    sample = _sample_vectors(nbytes // 16, seed)
    for run in np.split(sample, np.nonzero(np.diff(sample) != 1)[0] + 1):
        v0 = int(run[0])  # a run of consecutive vectors
        want = reference_words(v0, len(run), "addr", seed)
        got = words[4 * v0:4 * (v0 + len(run))]
        for j in np.nonzero(got != want)[0]:
            w = 4 * v0 + int(j)
            res.cpu_sample_mismatches += 1
            res.bad_bits_mask |= int(got[j]) ^ int(want[j])
            first_bad(4 * w)
            record(0, w, int(want[j]), int(got[j]), 0)
    # 1: host -> GPU loads
    kernel_read(1, H, "addr")
    # 2: the runtime's copy, host -> device; D is checked in HBM
    _, dt = timed(lambda: D.copy_(H, non_blocking=True))
    res.copy_h2d_gbps = gbps(nbytes, dt)
    account(2, _to_result(ext.verify_pattern(D, pattern_id("addr"), seed, max_records, 0)))
    done(2)
    # 3: the runtime's copy, device -> host; pass 4 checks it
    ext.fill_pattern(D, pattern_id("addr_inv"), seed, 0)
    _, dt = timed(lambda: H.copy_(D))
    res.copy_d2h_gbps = gbps(nbytes, dt)
    done(3)
    kernel_read(4, H, "addr_inv")
    # 5: CPU-authored data, read by the GPU alone
    _host_write(words, "checker", seed)
    account(5, _to_result(ext.hostlink_verify(
        H, pattern_id("checker"), seed, index, max_records, 0)))
    done(5)
    # 6: both directions in one kernel
    raw, dt = timed(lambda: ext.hostlink_duplex(
        lower, pattern_id("checker"), upper, pattern_id("walk1"), seed, index,
        max_records, 0, 0))
    res.duplex_gbps = gbps(nbytes, dt)
    account(6, _to_result(raw))
    done(6)
    kernel_read(7, upper, "walk1", base=half)

    res.kernel_h2d_gbps = max(read_gbps)
    res.ok = res.mismatched_words == 0 and res.cpu_sample_mismatches == 0
    res.records_dropped = (res.mismatched_words + res.cpu_sample_mismatches
                           - len(res.records))
    res.apply_floor(min_gbps)
    return res


# -- child process -----------------------------------------------------------

def run_hostlink_subprocess(index: int, nbytes: int = DEFAULT_BYTES,
                            timeout_s: float = 120.0) -> dict:
    """``_active.run_probe_subprocess`` for the hostlink CLI."""
    return _active.run_probe_subprocess("hostlink", index, "--bytes", nbytes, timeout_s)


def _attach_link(manager, min_gbps: float, uuid: str, rec: dict) -> None:
    """Between the runner and ``record_hostlink``: attach the GPU's PCIe
    link state (``read_pcie_link`` of its bdf, read here in the parent)
    as ``link`` and apply ``min_gbps``.  A figure below the floor is
    logged and exported and leaves health alone."""
    from ..api import utils

    gpu = manager.gpu_or_tombstone(uuid)
    rec["link"] = read_pcie_link(gpu.bdf) if gpu is not None else None
    rec["min_gbps"] = float(min_gbps)
    rec["below_floor"] = _below_floor(rec, float(min_gbps))
    if rec["below_floor"]:
        utils.errorf(
            "hostlink on GPU %s: below the %.1f GB/s floor (kernel h2d %.1f, "
            "kernel d2h %.1f, copy h2d %.1f, copy d2h %.1f GB/s, link %s) — "
            "health unchanged",
            uuid, float(min_gbps), float(rec.get("kernel_h2d_gbps", 0.0)),
            float(rec.get("kernel_d2h_gbps", 0.0)),
            float(rec.get("copy_h2d_gbps", 0.0)),
            float(rec.get("copy_d2h_gbps", 0.0)), rec["link"],
        )


def _metric_args(rec: dict) -> tuple:
    return (
        int(rec["mismatched_words"]) + int(rec.get("cpu_sample_mismatches", 0)),
        float(rec.get("kernel_h2d_gbps", 0.0)),
        float(rec.get("kernel_d2h_gbps", 0.0)),
        bool(rec["below_floor"]),
    )


def hostlink_round(manager, runner: Callable[[int, int], dict], metrics=None,
                   nbytes: int = DEFAULT_BYTES,
                   max_process_count: Optional[int] = 0,
                   min_gbps: float = 0.0) -> Dict[str, dict]:
    """``_active.probe_round`` with ``runner(index, nbytes)`` and
    ``_attach_link`` before the result is recorded."""
    return _active.probe_round(
        "hostlink", "mismatched_words", _metric_args, manager, runner, metrics, nbytes,
        max_process_count,
        after_run=lambda uuid, rec: _attach_link(manager, min_gbps, uuid, rec))


def main(argv=None) -> int:
    return _active.probe_main(
        "hostlink", "--bytes", DEFAULT_BYTES,
        lambda args: hostlink(nbytes=args.bytes, seed=args.seed, min_gbps=args.min_gbps),
        argv,
        add_arguments=lambda ap: ap.add_argument(
            "--min-gbps", type=float, default=0.0, metavar="X"))


if __name__ == "__main__":
    sys.exit(main())
