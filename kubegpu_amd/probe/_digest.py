"""What the digest probes (cucheck, mxcheck, fpcheck, atomcheck, lanecheck,
ldscheck, vmemcheck) share on the host: the hash that generates their inputs, the one-round and
period helpers of their references, the result type, the run body, the
decoding of the kernel's result block and of its value rows, and the dump
run.  Their kernels share csrc/cucheck_common.h the same way.

Imports neither torch nor numpy at import time.
"""

from __future__ import annotations

from dataclasses import dataclass, field, fields
from typing import Dict, List, Optional, Sequence

WAVES_PER_BLOCK = 16


# -- numpy definition ----------------------------------------------------------

def _fmix32(h):
    import numpy as np

    h = h.astype(np.uint32, copy=True)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x85EBCA6B)
    h ^= h >> np.uint32(13)
    h *= np.uint32(0xC2B2AE35)
    h ^= h >> np.uint32(16)
    return h


def _base(seed: int, stage: int, r):
    import numpy as np

    c = np.uint32(((stage + 1) * 0x9E3779B9) & 0xFFFFFFFF)
    return _fmix32(np.uint32(seed) ^ c ^ (r * np.uint32(0x7F4A7C15)))


def _salt(n):
    import numpy as np

    return (n.astype(np.uint32) + np.uint32(1)) * np.uint32(0x9E3779B9)


def one_round(name: str, r: int):
    """Round ``r`` as the uint32[1] array the stage functions take."""
    import numpy as np

    r = int(r)
    if not 0 <= r < 65536:
        raise ValueError(f"{name}: round must be in 0..65535, got {r}")
    return np.array([r], dtype=np.uint32)


def tile_period(rows, rounds: int, period: int):
    """The table of ``rounds`` rounds of a probe whose inputs repeat with
    ``period``, from its first min(rounds, period) rows."""
    import numpy as np

    if rounds <= period:
        return rows
    return np.tile(rows, (-(-rounds // period), 1))[:rounds].copy()


# -- GPU run ---------------------------------------------------------------------

@dataclass
class DigestResult:
    """The fields every digest probe reports; a probe's own result type
    adds its rate fields (floats), which ``to_dict`` appends in the
    order they are declared."""

    ok: bool = True
    rounds: int = 0
    waves: int = 0
    mismatches: int = 0
    first_bad_round: Optional[int] = None
    bad_stages: List[str] = field(default_factory=list)
    # {"wave", "block", "xcc", "se", "sh", "cu", "simd", "round", "stage",
    #  "expected", "got"} per logged digest
    records: List[Dict] = field(default_factory=list)
    records_dropped: int = 0
    cus_covered: int = 0  # distinct CUs that ran at least one wave
    cu_count: int = 0  # multiProcessorCount
    bad_cus: List[str] = field(default_factory=list)  # "xcc/se/sh/cu"
    elapsed_s: float = 0.0
    waves_on: List[int] = field(default_factory=list, repr=False)

    def rate_fields(self) -> List[str]:
        return [f.name for f in fields(self)[len(fields(DigestResult)):]]

    def to_dict(self) -> dict:
        out = {
            "ok": bool(self.ok),
            "rounds": int(self.rounds),
            "waves": int(self.waves),
            "mismatches": int(self.mismatches),
            "first_bad_round": self.first_bad_round,
            "bad_stages": list(self.bad_stages),
            "records": [dict(r) for r in self.records],
            "records_dropped": int(self.records_dropped),
            "cus_covered": int(self.cus_covered),
            "cu_count": int(self.cu_count),
            "bad_cus": list(self.bad_cus),
            "elapsed_s": float(self.elapsed_s),
        }
        for name in self.rate_fields():
            out[name] = float(getattr(self, name))
        return out


def cu_key(xcc: int, se: int, sh: int, cu: int) -> int:
    """Index of a CU in the kernel's waves_on table."""
    return (xcc << 7) | (se << 5) | (sh << 4) | cu


def decode_record(raw, stages: Sequence[str]) -> dict:
    wave, hw, rnd, stage, expected, got = (int(x) for x in raw)
    # hw = XCC_ID << 16 | HW_ID[15:0]; HW_ID: SIMD 5:4, CU 11:8, SH 12, SE 14:13
    return {
        "wave": wave,
        "block": wave // WAVES_PER_BLOCK,
        "xcc": (hw >> 16) & 0xF,
        "se": (hw >> 13) & 0x3,
        "sh": (hw >> 12) & 0x1,
        "cu": (hw >> 8) & 0xF,
        "simd": (hw >> 4) & 0x3,
        "round": rnd,
        "stage": stages[stage] if 0 <= stage < len(stages) else stage,
        "expected": expected,
        "got": got,
    }


def _device(device):
    import torch

    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device(device)


def expected_tensor(name: str, table, rounds: int, stages: Sequence[str], device):
    import numpy as np
    import torch

    table = np.array(table, dtype=np.uint32)  # own, writable copy for torch
    if table.shape != (rounds, len(stages)):
        raise ValueError(
            f"{name}: expected table must be [{rounds}, {len(stages)}], got {table.shape}")
    return torch.from_numpy(table.view(np.int32)).to(device)


def fill_result(res: DigestResult, raw, stages: Sequence[str], device,
                work_per_wave_round: Sequence[int], unit: float) -> DigestResult:
    """Fill ``res`` (its ``rounds`` set) from what the extension's run
    returned: (mismatches, first_bad_round, stage_mask, records,
    waves_on, elapsed_s).  The rate fields are whole-run lower bounds:
    waves x rounds x ``work_per_wave_round`` of the field, per second,
    in ``unit``."""
    import torch

    count, first, mask, records, waves_on, elapsed = raw
    res.waves_on = [int(x) for x in waves_on]
    res.waves = sum(res.waves_on)
    res.mismatches = int(count)
    res.ok = res.mismatches == 0
    res.first_bad_round = int(first) if res.mismatches else None
    res.bad_stages = [s for i, s in enumerate(stages) if (int(mask) >> i) & 1]
    res.records = [decode_record(r, stages) for r in records]
    res.records_dropped = res.mismatches - len(res.records)
    res.cus_covered = sum(1 for x in res.waves_on if x)
    res.cu_count = int(torch.cuda.get_device_properties(device).multi_processor_count)
    res.bad_cus = sorted({f"{r['xcc']}/{r['se']}/{r['sh']}/{r['cu']}" for r in res.records})
    res.elapsed_s = float(elapsed)
    if res.elapsed_s > 0:
        work = res.waves * res.rounds / res.elapsed_s / unit
        for name, f in zip(res.rate_fields(), work_per_wave_round):
            setattr(res, name, work * f)
    return res


def run_probe(name: str, res: DigestResult, stages: Sequence[str],
              work_per_wave_round: Sequence[int], unit: float, reference, seed: int,
              blocks: int, max_records: int, device, inject, expected, *extra) -> DigestResult:
    """The body of ``cucheck()``, ``mxcheck()``, ``fpcheck()``,
    ``lanecheck()``, ``ldscheck()`` and ``vmemcheck()``: ``res.rounds`` rounds of
    ``<name>_run`` against the table ``expected``, or ``reference()``
    where that is None, into ``res``.  ``extra`` goes between ``blocks``
    and ``max_records``."""
    from ._active import _ext

    ext = _ext()
    device = _device(device)
    rounds = res.rounds
    if not 1 <= rounds <= 65536:
        raise ValueError(f"{name}: rounds must be in 1..65536, got {rounds}")
    table = expected if expected is not None else reference()
    tensor = expected_tensor(name, table, rounds, stages, device)
    inject = None if inject is None else tuple(int(x) for x in inject)
    raw = getattr(ext, name + "_run")(
        tensor, seed, rounds, blocks, *extra, int(max_records), None, inject)
    return fill_result(res, raw, stages, device, work_per_wave_round, unit)


def value_rows(name: str, raw, names: Sequence[str], rows: int, stage: int) -> dict:
    """{slot name: row of 64} from what ``<name>_values`` returned for
    ``stage``, viewed as unsigned: ``rows`` rows of 64 lanes, then the
    number of rows the kernel filled."""
    if int(raw[-1]) != len(names):
        raise RuntimeError(f"{name}: the kernel filled {int(raw[-1])} slots of stage "
                           f"{stage}, the reference has {len(names)}")
    table = raw[:-1].reshape(rows, 64)
    return {n: table[k] for k, n in enumerate(names)}


def wave_digests(name: str, run, table, stages: Sequence[str], seed: int, rounds: int,
                 blocks: int, device, *extra):
    """What every wave computed, as uint32[blocks*16, rounds, 4]: the
    probe's own kernel (``run``, the extension's ``<name>_run``) with
    its dump pointer set.  ``table`` is the reference for those rounds;
    ``extra`` goes between ``blocks`` and ``max_records``."""
    import numpy as np
    import torch

    rounds, blocks = int(rounds), int(blocks)
    device = _device(device)
    if blocks == 0:
        blocks = int(torch.cuda.get_device_properties(device).multi_processor_count)
    waves = blocks * WAVES_PER_BLOCK
    expected = expected_tensor(name, table, rounds, stages, device)
    dump = torch.zeros(waves * rounds * len(stages), dtype=torch.int32, device=device)
    run(expected, int(seed), rounds, blocks, *extra, 0, dump, None)
    return dump.cpu().numpy().view(np.uint32).reshape(waves, rounds, len(stages))


def metric_args(rec: dict) -> tuple:
    """What ``set_gpu_cucheck`` / ``_mxcheck`` / ``_fpcheck`` / ``_lanecheck`` /
    ``_ldscheck`` / ``_vmemcheck`` take of a result dict, before the timestamp."""
    return int(rec["mismatches"]), int(rec.get("cus_covered", 0))
