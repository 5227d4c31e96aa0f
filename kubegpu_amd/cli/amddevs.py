"""amddevs — operator CLI (analog of the reference's nvidiadevs,
/root/reference/nvidiagpuplugin/cmd/main.go:13-45).

Modes:
  amddevs                 raw discovery dump (GpusInfo JSON)
  amddevs --plugin        full device-plugin path: New/Start/UpdateNodeInfo,
                          print the advertised NodeInfo
  amddevs --schedule K    schedule a synthetic K-GPU pod against the local
                          node and print the chosen GPU set + allocation
  amddevs --probe K       same, then run the in-pod RCCL probe over the set
  amddevs --health        per-GPU health view (ECC totals, tombstones,
                          the active probes' verdicts)
  amddevs --memcheck      HBM integrity probe over the idle GPUs, one child
                          process per GPU; prints {uuid: result}
                          (exit 1 = mismatches, 2 = nothing could run)
  amddevs --cucheck       compute-unit integrity probe over the idle GPUs,
                          same shape and exit codes ([--rounds N])
  amddevs --mxcheck       matrix-core format (f16, fp8, MXFP4, f64) integrity
                          probe over the idle GPUs, same shape and exit
                          codes ([--rounds N])
  amddevs --fpcheck       IEEE rounding (f32, f64, packed f16 / f32,
                          conversions) integrity probe over the idle GPUs,
                          same shape and exit codes ([--rounds N])
  amddevs --hostlink      host-link (PCIe path) integrity and bandwidth
                          probe over the idle GPUs, same shape and exit
                          codes ([--bytes N])
  amddevs --atomcheck     atomic-unit (LDS, L2 and memory-side atomics)
                          integrity probe over the idle GPUs, same shape and
                          exit codes ([--rounds N])
  amddevs --lanecheck     cross-lane (DPP, LDS crossbar, readlane, permlane
                          swaps) integrity probe over the idle GPUs, same
                          shape and exit codes ([--rounds N])
  amddevs --ldscheck      LDS (narrow and wide accesses, bank conflicts,
                          transposed read, LDS-DMA, cross-wave addressing)
                          integrity probe over the idle GPUs, same shape and
                          exit codes ([--rounds N])
  amddevs --vmemcheck     vector-memory (narrow and wide global accesses,
                          gathers through L1, scalar cache and L2, partial-line
                          writes, buffer range check) integrity probe over the
                          idle GPUs, same shape and exit codes ([--rounds N])
"""

from __future__ import annotations

import argparse
import json
import sys

from ..api.types import ContainerInfo, NodeInfo, PodInfo
from ..core import Cluster
from ..deviceplugin import create_device_plugin
from ..discovery import default_backend
from ..plugintypes import RESOURCE_GPU
from ..probe._active import EXIT_CANNOT_RUN, PROBE_NAMES

# probe -> (what the --fake backend lacks, size argument, name of its
# default in the probe's module, result keys that count wrong data)
_PROBE_RUNS = {
    "memcheck": ("memory", "bytes", "DEFAULT_BYTES", ("mismatched_words",)),
    "cucheck": ("compute units", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
    "mxcheck": ("matrix cores", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
    "fpcheck": ("FP units", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
    "hostlink": ("host link", "bytes", "DEFAULT_BYTES",
                 ("mismatched_words", "cpu_sample_mismatches")),
    "atomcheck": ("atomic units", "rounds", "DEFAULT_ROUNDS",
                  ("mismatches", "shared_mismatches")),
    "lanecheck": ("cross-lane paths", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
    "ldscheck": ("LDS", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
    "vmemcheck": ("vector-memory paths", "rounds", "DEFAULT_ROUNDS", ("mismatches",)),
}


def _run_probe(probe: str, args, backend) -> int:
    """Run an active probe over the idle GPUs, print {uuid: result} and
    turn the results into an exit code: 1 = wrong data on some GPU, 2 =
    nothing could run, 0 otherwise."""
    import importlib

    lacks, size_arg, default_name, fail_keys = _PROBE_RUNS[probe]
    if args.fake:
        print(f"--{probe} needs real GPUs; the --fake fixture backend "
              f"has no {lacks} to test", file=sys.stderr)
        return EXIT_CANNOT_RUN
    mod = importlib.import_module(f"..probe.{probe}", __package__)
    mgr = create_device_plugin(backend)
    mgr.start()
    size = getattr(args, size_arg)
    # An operator asked for this run, and a fresh manager has no
    # allocation view.  Raw process_count is not occupancy (daemons
    # registered on KFD make a resting node report 1-2), so it gates
    # only memcheck and only on request; memcheck takes its buffer from
    # free VRAM and cannot disturb a running job's data.
    idle_only = probe == "memcheck" and args.memcheck_idle_only
    results = getattr(mod, f"{probe}_round")(
        mgr, getattr(mod, f"run_{probe}_subprocess"), None,
        size if size is not None else getattr(mod, default_name),
        max_process_count=0 if idle_only else None,
    )
    print(json.dumps(results, indent=1))
    ran = [r for r in results.values() if fail_keys[0] in r]
    if any(r.get(k) for r in ran for k in fail_keys):
        return 1
    if not ran:
        print(f"{probe}: no idle GPU could be checked", file=sys.stderr)
        return EXIT_CANNOT_RUN
    return 0


def main(argv=None) -> int:
    p = argparse.ArgumentParser(prog="amddevs")
    p.add_argument("--plugin", action="store_true", help="run the device-plugin path")
    p.add_argument("--schedule", type=int, metavar="K", help="schedule a K-GPU pod")
    p.add_argument("--probe", type=int, metavar="K", help="schedule + RCCL probe")
    p.add_argument("--bytes", type=int, default=None,
                   help="probe buffer size (default 256 MiB for --probe, "
                        "1 GiB for --memcheck, 256 MiB for --hostlink)")
    p.add_argument("--memcheck", action="store_true",
                   help="run the HBM integrity probe on every GPU this "
                        "command can see no allocation on")
    p.add_argument("--memcheck-idle-only", action="store_true",
                   help="with --memcheck: also skip GPUs that report any "
                        "compute process (process_count > 0)")
    p.add_argument("--cucheck", action="store_true",
                   help="run the compute-unit integrity probe on every GPU "
                        "this command can see no allocation on")
    p.add_argument("--rounds", type=int, default=None, metavar="N",
                   help="with --cucheck, --mxcheck, --fpcheck, --atomcheck, --lanecheck, "
                        "--ldscheck or --vmemcheck: rounds per GPU "
                        "(default: the probe's own, about 0.5 s)")
    p.add_argument("--mxcheck", action="store_true",
                   help="run the matrix-core format integrity probe (f16, fp8, "
                        "MXFP4, f64) on every GPU this command can see no "
                        "allocation on")
    p.add_argument("--fpcheck", action="store_true",
                   help="run the IEEE rounding integrity probe (f32, f64, "
                        "packed f16 / f32, conversions) on every GPU this "
                        "command can see no allocation on")
    p.add_argument("--hostlink", action="store_true",
                   help="run the host-link integrity and bandwidth probe on "
                        "every GPU this command can see no allocation on")
    p.add_argument("--atomcheck", action="store_true",
                   help="run the atomic-unit integrity probe (LDS, L2 and "
                        "memory-side atomics) on every GPU this command can "
                        "see no allocation on")
    p.add_argument("--lanecheck", action="store_true",
                   help="run the cross-lane integrity probe (DPP, LDS "
                        "crossbar, readlane, permlane swaps) on every GPU this "
                        "command can see no allocation on")
    p.add_argument("--ldscheck", action="store_true",
                   help="run the LDS integrity probe (narrow and wide accesses, "
                        "bank conflicts, transposed read, LDS-DMA, cross-wave "
                        "addressing) on every GPU this command can see no "
                        "allocation on")
    p.add_argument("--vmemcheck", action="store_true",
                   help="run the vector-memory integrity probe (narrow and wide "
                        "global accesses, gathers through L1, scalar cache and "
                        "L2, partial-line writes, buffer range check) on every "
                        "GPU this command can see no allocation on")
    p.add_argument("--health", action="store_true",
                   help="per-GPU health view (ECC totals, tombstones)")
    p.add_argument("--cdi", action="store_true",
                   help="emit a CDI v0.6.0 spec for the node's GPUs "
                        "(write to /etc/cdi/amd.com-gpu.json to activate)")
    p.add_argument("--fake", action="store_true",
                   help="use the 8xMI355X fixture backend (no GPU needed)")
    from .. import __version__

    p.add_argument("--version", action="version",
                   version=f"kubegpu-amd {__version__}")
    args = p.parse_args(argv)

    if args.fake:
        from ..discovery import FakeBackend, fixtures

        backend = FakeBackend(fixtures.fixture_8x_mi355x())
    else:
        backend = default_backend()
    if args.cdi:
        from ..deviceplugin.cdi import cdi_json

        info = None
        mgr = create_device_plugin(backend)
        mgr.start()
        if mgr._last_info is None:
            print("no GPUs discovered", file=sys.stderr)
            return 1
        print(cdi_json(mgr._last_info))
        return 0
    for probe in PROBE_NAMES:
        if getattr(args, probe):
            return _run_probe(probe, args, backend)
    if args.health:
        mgr = create_device_plugin(backend)
        mgr.start()
        health = mgr.device_health()
        rows = {}
        for uuid in sorted(health):
            g = mgr.gpu_or_tombstone(uuid)
            rows[uuid] = {
                "healthy": health[uuid],
                "present": uuid in mgr.gpus,
                "in_use": bool(g.in_use) if g else None,
                "ecc_correctable": g.ecc_correctable if g else None,
                "ecc_uncorrectable": g.ecc_uncorrectable if g else None,
                "process_count": g.process_count if g else None,
                "mxcheck": mgr.mxcheck_status(uuid),
                "fpcheck": mgr.fpcheck_status(uuid),
                "atomcheck": mgr.atomcheck_status(uuid),
                "lanecheck": mgr.lanecheck_status(uuid),
                "ldscheck": mgr.ldscheck_status(uuid),
                "vmemcheck": mgr.vmemcheck_status(uuid),
            }
        print(json.dumps(rows, indent=1))
        return 0
    if not (args.plugin or args.schedule or args.probe):
        print(backend.get_gpu_info().decode())
        return 0

    mgr = create_device_plugin(backend)
    mgr.start()
    ni = NodeInfo(name="local")
    mgr.update_node_info(ni)
    if args.plugin:
        print(json.dumps({
            "capacity": ni.capacity,
            "allocatable": ni.allocatable,
            "kube_cap": ni.kube_cap,
            "kube_alloc": ni.kube_alloc,
        }, indent=1))
        return 0

    k = args.probe or args.schedule
    cluster = Cluster()
    cluster.add_node(ni, mgr._last_info, mgr)
    pod = PodInfo(
        name=f"cli-{k}gpu",
        running_containers={"c": ContainerInfo(kube_requests={RESOURCE_GPU: k})},
    )
    res = cluster.schedule(pod)
    mounts, devices, envs = cluster.container_allocate(pod, "c")
    from ..events import EVENTS

    print(json.dumps({
        "node": res.node_name,
        "gpus": res.uuids,
        "devices": devices,
        "envs": envs,
        "schedule_latency_ms": res.latency_s * 1e3,
        "event": (EVENTS.recent(1) or [None])[-1],
    }, indent=1))

    if args.probe:
        from ..probe import probe_with_link_utilization, run_rccl_probe

        idxs = sorted(mgr.gpus[u].index for u in res.uuids)
        # model prediction for the scheduled subset (the quantity the
        # probe verifies — SURVEY.md hard part (b))
        st = cluster.core.nodes[res.node_name]
        pred = st.scorer.ring_bw(idxs)
        pred = None if pred >= 1e9 else pred
        out, links = probe_with_link_utilization(
            run_rccl_probe, devices=idxs,
            nbytes=args.bytes if args.bytes is not None else 256 << 20,
        )
        measured = out.get("busbw_gbps")
        print(json.dumps({
            "probe": out,
            "predicted_ring_bottleneck_gbps": pred,
            "model_vs_measured_ratio": (
                round(measured / pred, 3) if pred and measured else None
            ),
            "xgmi_link_traffic": links,
        }, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
