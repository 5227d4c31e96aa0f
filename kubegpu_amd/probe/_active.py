"""What the active integrity probes (memcheck, cucheck, mxcheck,
fpcheck, hostlink, atomcheck, lanecheck, ldscheck, vmemcheck) share: the exit codes, the one child-process lock,
the child runner, the round over a node's idle GPUs and the CLI body.
Each probe module binds these to its own name, so a probe adds only
what is its own: kernels, reference, result type.

Imports neither torch nor numpy at import time.
"""

from __future__ import annotations

import json
import os
import subprocess
import sys
import threading
import time
from typing import Callable, Dict, List, Optional, Tuple

# In the order the manager, the metrics, the agent and the CLI go
# through them.
ACTIVE_PROBES: Tuple[str, ...] = ("memcheck", "cucheck", "mxcheck", "fpcheck", "hostlink")
# ACTIVE_PROBES stays the first five and HEALTH_PROBES the first six.
HEALTH_PROBES: Tuple[str, ...] = ACTIVE_PROBES + ("atomcheck",)
# The first seven probes whose verdict decides a GPU's health; later
# probes are appended to PROBES below.
ALL_PROBES: Tuple[str, ...] = HEALTH_PROBES + ("lanecheck",)
# ALL_PROBES stays the first seven as well, and PROBES the first eight.
PROBES: Tuple[str, ...] = ALL_PROBES + ("ldscheck",)
# Every probe whose verdict decides a GPU's health: the tuple the manager,
# the metrics, the agent loop and the CLI go through; later probes are
# appended here.
PROBE_NAMES: Tuple[str, ...] = PROBES + ("vmemcheck",)

EXIT_PASS, EXIT_MISMATCH, EXIT_CANNOT_RUN = 0, 1, 2

_REPO_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# One active-probe child at a time, whichever of the probes it
# runs: two probes never overlap on a GPU, nor on the host's memory.
_child_lock = threading.Lock()


def _ext():
    from .bandwidth import load_ext

    return load_ext(required=True)


def run_probe_subprocess(name: str, index: int, size_flag: str, size: int,
                         timeout_s: float) -> dict:
    """Run the CLI of probe ``name`` for GPU ``index`` in a fresh child
    process (never exec: the parent may hold the GPU open) and return
    its JSON record, the last line of its stdout, with ``exit_code``
    added.  ``size_flag`` is ``--bytes`` or ``--rounds``.  Serialised on
    the one child lock.  Raises subprocess.TimeoutExpired when the child
    overruns (it is killed first)."""
    cmd = [sys.executable, "-m", f"kubegpu_amd.probe.{name}",
           "--device", str(int(index)), size_flag, str(int(size))]
    env = dict(os.environ)
    env["PYTHONPATH"] = _REPO_ROOT + os.pathsep + env["PYTHONPATH"] \
        if env.get("PYTHONPATH") else _REPO_ROOT
    with _child_lock:
        out = subprocess.run(cmd, capture_output=True, timeout=timeout_s,
                             env=env, text=True)
    lines = out.stdout.strip().splitlines()
    try:
        rec = json.loads(lines[-1])
    except (IndexError, ValueError):
        rec = {"error": f"no JSON from {name} child: {out.stderr[-500:]}"}
        out.returncode = EXIT_CANNOT_RUN
    rec["exit_code"] = out.returncode
    return rec


def idle_gpus(manager, max_process_count: Optional[int]) -> List[Tuple[int, str]]:
    """(index, uuid) of every present GPU an active probe may take, in
    index order: no allocation, and process_count at most
    max_process_count (None ignores process_count)."""
    with manager._lock:
        return sorted(
            (g.index, u) for u, g in manager.gpus.items()
            if not g.in_use and (
                max_process_count is None or g.process_count <= max_process_count
            )
        )


def probe_round(name: str, count_key: str, metric_args: Callable[[dict], tuple],
                manager, runner: Callable[[int, int], dict], metrics, size: int,
                max_process_count: Optional[int],
                after_run: Optional[Callable[[str, dict], None]] = None) -> Dict[str, dict]:
    """Check every idle GPU once with probe ``name`` and record the
    verdicts.

    For each present GPU with no allocation (``in_use``) and a
    ``process_count`` of at most ``max_process_count``, in index order,
    ``runner(index, size)`` is called, ``after_run(uuid, rec)`` may add
    to its result dict, and the dict is recorded on the manager
    (``record_<name>``) and exported (``set_gpu_<name>(uuid,
    *metric_args(rec), now)``).  ``max_process_count`` is the highest
    process_count still taken as idle: daemons that register on KFD make
    a node with no workload report 1 or 2, so such nodes raise it to
    their resting value; None ignores process_count altogether.  A
    runner that raises, times out, reports exit code 2 or returns no
    ``count_key`` says nothing about the hardware: it is logged and
    counted as an error (``inc_<name>_error``), and the GPU's health is
    left as it was.  Returns {uuid: result}."""
    from ..api import utils

    out: Dict[str, dict] = {}
    for index, uuid in idle_gpus(manager, max_process_count):
        try:
            rec = runner(index, size)
            if not isinstance(rec, dict):
                raise TypeError(f"{name} runner returned {type(rec).__name__}")
            if rec.get("exit_code") == EXIT_CANNOT_RUN or count_key not in rec:
                raise RuntimeError(rec.get("error") or f"{name} could not run")
        except Exception as e:  # not a hardware fault: health unchanged
            utils.errorf(name + " on GPU %s (index %d) did not run: %s", uuid, index, e)
            if metrics is not None:
                getattr(metrics, f"inc_{name}_error")(uuid)
            out[uuid] = {"error": str(e), "exit_code": EXIT_CANNOT_RUN}
            continue
        if after_run is not None:
            after_run(uuid, rec)
        try:
            getattr(manager, f"record_{name}")(uuid, rec)
        except KeyError:  # vanished mid-round
            continue
        if metrics is not None:
            getattr(metrics, f"set_gpu_{name}")(uuid, *metric_args(rec), time.time())
        out[uuid] = rec
    return out


def probe_main(name: str, size_flag: str, default_size: int,
               probe: Callable[..., object], argv=None,
               add_arguments: Optional[Callable] = None) -> int:
    """The CLI of probe ``name``: ``--device INDEX``, ``size_flag``
    (``--bytes`` or ``--rounds``), ``--seed`` and whatever
    ``add_arguments(parser)`` adds.  Pins the process to the device,
    calls ``probe(args)``, prints its ``to_dict()`` as one JSON line with
    ``device`` added and returns EXIT_PASS or EXIT_MISMATCH; anything
    that keeps the probe from running (no GPU, extension missing, out of
    memory, bad argument) prints ``{"error": ...}`` and returns
    EXIT_CANNOT_RUN."""
    import argparse

    ap = argparse.ArgumentParser(prog=f"kubegpu-amd-{name}")
    ap.add_argument("--device", type=int, required=True, metavar="INDEX")
    ap.add_argument(size_flag, type=int, default=default_size, metavar="N")
    ap.add_argument("--seed", type=int, default=0)
    if add_arguments is not None:
        add_arguments(ap)
    args = ap.parse_args(argv)

    # pin before torch / HIP initialise (same as bench.py)
    os.environ["ROCR_VISIBLE_DEVICES"] = str(args.device)
    rec: dict
    try:
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible")
        torch.cuda.set_device(0)
        result = probe(args)
        rec = result.to_dict()
        code = EXIT_PASS if result.ok else EXIT_MISMATCH
    except Exception as e:
        rec = {"error": f"{type(e).__name__}: {e}"}
        code = EXIT_CANNOT_RUN
    rec["device"] = args.device
    print(json.dumps(rec), flush=True)
    return code
