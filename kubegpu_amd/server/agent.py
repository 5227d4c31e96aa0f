"""Node agent — the long-running production entry point.

Runs the device-plugin gRPC server, registers with kubelet (with retry —
kubelet restarts wipe the plugin registry, so the agent watches its own
socket and re-registers when the plugin dir is recreated), keeps
discovery fresh, and serves Prometheus metrics.

Usage:
    python -m kubegpu_amd.server.agent [--socket PATH] [--plugin-dir DIR]
        [--kubelet-socket PATH] [--no-register] [--metrics-port 9400]
        [--fake]  (fixture backend, for plumbing tests without a GPU)
"""

from __future__ import annotations

import argparse
import importlib
import json
import os
import signal
import sys
import time

from ..api import utils
from ..deviceplugin import create_device_plugin
from ..discovery import FakeBackend, default_backend, fixtures
from ..metrics import METRICS
from ..probe._active import PROBE_NAMES
from . import dpapi
from .kubelet_plugin import KubeletDevicePlugin


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="kubegpu-amd-agent")
    ap.add_argument("--socket", default=None)
    ap.add_argument("--plugin-dir", default=dpapi.DEVICE_PLUGIN_PATH)
    ap.add_argument("--kubelet-socket", default=dpapi.KUBELET_SOCKET)
    ap.add_argument("--pod-resources-socket", default=None,
                    help="kubelet pod-resources socket for in_use "
                         "reconciliation (default: the standard path "
                         "when it exists)")
    ap.add_argument("--no-register", action="store_true")
    ap.add_argument("--extender-url", default=None,
                    help="scheduler-extender base URL (e.g. "
                         "http://gpu-extender:9109); the agent POSTs its "
                         "inventory to /v1/nodes/<node-name> every health "
                         "tick so the extender scores this node")
    ap.add_argument("--node-name", default=None,
                    help="node name for extender registration "
                         "(default: hostname)")
    ap.add_argument("--metrics-port", type=int, default=9400)
    ap.add_argument("--health-interval", type=float, default=30.0)
    ap.add_argument("--fake", action="store_true",
                    help="use the 8xMI355X fixture backend (no GPU needed)")
    ap.add_argument("--startup-probe", action="store_true",
                    help="run the RCCL all-reduce probe over the node's "
                         "GPUs at start and export the measured busbw "
                         "(the verification loop, BASELINE.json)")
    ap.add_argument("--probe-bytes", type=int, default=256 << 20)
    ap.add_argument("--memcheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the HBM integrity probe over the idle GPUs "
                         "every SECONDS from the health loop; a GPU with "
                         "mismatches turns Unhealthy (0 = off)")
    ap.add_argument("--memcheck-bytes", type=int, default=1 << 30,
                    help="buffer size per GPU for the HBM integrity probe")
    ap.add_argument("--memcheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the HBM integrity probe; set it to the "
                         "node's resting value when daemons hold KFD open")
    ap.add_argument("--cucheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the compute-unit integrity probe over the idle "
                         "GPUs every SECONDS from the health loop; a GPU "
                         "with a wrong digest turns Unhealthy (0 = off)")
    ap.add_argument("--cucheck-rounds", type=int, default=None,
                    help="rounds per GPU for the compute-unit integrity "
                         "probe (default: the probe's own, about 0.5 s)")
    ap.add_argument("--cucheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the compute-unit integrity probe")
    ap.add_argument("--mxcheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the matrix-core format integrity probe (f16, "
                         "fp8, MXFP4, f64) over the idle GPUs every SECONDS "
                         "from the health loop; a GPU with a wrong digest "
                         "turns Unhealthy (0 = off)")
    ap.add_argument("--mxcheck-rounds", type=int, default=None,
                    help="rounds per GPU for the matrix-core format integrity "
                         "probe (default: the probe's own, about 0.5 s)")
    ap.add_argument("--mxcheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the matrix-core format integrity probe")
    ap.add_argument("--fpcheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the IEEE rounding integrity probe (f32, f64, "
                         "packed, conversions) over the idle GPUs every "
                         "SECONDS from the health loop; a GPU with a wrong "
                         "digest turns Unhealthy (0 = off)")
    ap.add_argument("--fpcheck-rounds", type=int, default=None,
                    help="rounds per GPU for the IEEE rounding integrity "
                         "probe (default: the probe's own, about 0.5 s)")
    ap.add_argument("--fpcheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the IEEE rounding integrity probe")
    ap.add_argument("--hostlink-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the host-link integrity probe over the idle "
                         "GPUs every SECONDS from the health loop; a GPU "
                         "with words that crossed the link wrong turns "
                         "Unhealthy (0 = off)")
    ap.add_argument("--hostlink-bytes", type=int, default=256 << 20,
                    help="pinned host buffer (and device buffer) size per "
                         "GPU for the host-link integrity probe")
    ap.add_argument("--hostlink-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the host-link integrity probe")
    ap.add_argument("--hostlink-min-gbps", type=float, default=0.0,
                    help="report (log, metric) a GPU whose one-way host-link "
                         "bandwidth is under this many GB/s; never changes "
                         "health (0 = no floor)")
    ap.add_argument("--atomcheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the atomic-unit integrity probe (LDS, L2 and "
                         "memory-side atomics) over the idle GPUs every "
                         "SECONDS from the health loop; a GPU with a wrong "
                         "digest or a wrong shared cell turns Unhealthy "
                         "(0 = off)")
    ap.add_argument("--atomcheck-rounds", type=int, default=None,
                    help="rounds per GPU for the atomic-unit integrity "
                         "probe (default: the probe's own, about 0.5 s)")
    ap.add_argument("--atomcheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the atomic-unit integrity probe")
    ap.add_argument("--lanecheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the cross-lane integrity probe (DPP, LDS "
                         "crossbar, readlane, permlane swaps) over the idle "
                         "GPUs every SECONDS from the health loop; a GPU "
                         "with a wrong digest turns Unhealthy (0 = off)")
    ap.add_argument("--lanecheck-rounds", type=int, default=None,
                    help="rounds per GPU for the cross-lane integrity "
                         "probe (default: the probe's own, about 0.5 s)")
    ap.add_argument("--lanecheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the cross-lane integrity probe")
    ap.add_argument("--ldscheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the LDS integrity probe (narrow and wide "
                         "accesses, bank conflicts, transposed read, LDS-DMA, "
                         "the whole array across waves) over the idle GPUs "
                         "every SECONDS from the health loop; a GPU with a "
                         "wrong digest turns Unhealthy (0 = off)")
    ap.add_argument("--ldscheck-rounds", type=int, default=None,
                    help="rounds per GPU for the LDS integrity probe "
                         "(default: the probe's own, about 0.5 s)")
    ap.add_argument("--ldscheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the LDS integrity probe")
    ap.add_argument("--vmemcheck-interval", type=float, default=0.0,
                    metavar="SECONDS",
                    help="run the vector-memory integrity probe (narrow and "
                         "wide global accesses, gathers through the L1, the "
                         "scalar cache and the L2, partial-line writes, the "
                         "buffer range check) over the idle GPUs every SECONDS "
                         "from the health loop; a GPU with a wrong digest "
                         "turns Unhealthy (0 = off)")
    ap.add_argument("--vmemcheck-rounds", type=int, default=None,
                    help="rounds per GPU for the vector-memory integrity probe "
                         "(default: the probe's own, about 0.5 s)")
    ap.add_argument("--vmemcheck-max-procs", type=int, default=0,
                    help="highest amdsmi process_count still treated as "
                         "idle by the vector-memory integrity probe")
    ap.add_argument("--oneshot", action="store_true",
                    help="start, print state, exit (plumbing check)")
    args = ap.parse_args(argv)

    backend = (
        FakeBackend(fixtures.fixture_8x_mi355x()) if args.fake else default_backend()
    )
    manager = create_device_plugin(backend)
    manager.start()
    utils.logf(0, "agent: discovered %d GPU(s)", len(manager.gpus))

    if args.startup_probe:
        try:
            from ..probe import run_rccl_probe

            idxs = sorted(g.index for g in manager.gpus.values())
            rec = run_rccl_probe(devices=idxs, nbytes=args.probe_bytes,
                                 iters=10, warmup=3)
            METRICS.set_xgmi_gbps(rec.get("busbw_gbps", 0.0))
            utils.logf(
                0, "startup probe: %d GPU(s) busbw %.1f GB/s (check=%s)",
                len(idxs), rec.get("busbw_gbps", 0.0), rec.get("check"),
            )
        except Exception as e:
            utils.errorf("startup probe failed (agent continues): %s", e)

    plugin = KubeletDevicePlugin(
        manager,
        socket_path=args.socket,
        plugin_dir=args.plugin_dir,
    )
    plugin.servicer.health_interval_s = args.health_interval
    plugin.start()

    if args.metrics_port:
        if METRICS.serve(args.metrics_port):
            utils.logf(1, "agent: metrics on :%d", args.metrics_port)

    stop = {"flag": False}

    def _sig(_signo, _frame):
        stop["flag"] = True

    signal.signal(signal.SIGTERM, _sig)
    signal.signal(signal.SIGINT, _sig)

    registered = False
    if args.oneshot:
        print(f"agent ok: {len(manager.gpus)} GPUs, socket {plugin.socket_path}")
        plugin.stop()
        return 0

    watcher_started = False
    # first round of every enabled probe on the first tick
    next_due = {probe: time.monotonic() for probe in PROBE_NAMES}
    while not stop["flag"]:
        if not args.no_register and not registered:
            try:
                plugin.register_with_kubelet(args.kubelet_socket)
                registered = True
                if not watcher_started:
                    # kubelet-side restart detection: its socket is
                    # recreated on restart; the watcher re-registers
                    plugin.watch_kubelet(args.kubelet_socket)
                    watcher_started = True
            except Exception as e:
                utils.logf(2, "agent: kubelet registration pending: %s", e)
        # kubelet restart detection: our socket vanishes when the plugin
        # dir is recreated -> re-serve + re-register
        if not os.path.exists(plugin.socket_path):
            utils.logf(0, "agent: socket vanished (kubelet restart?); re-serving")
            plugin.stop()
            plugin.start()
            registered = False
        plugin.servicer.notify()  # wake ListAndWatch to refresh health
        if args.extender_url and manager._last_info is not None:
            try:
                import socket as _socket
                import urllib.request as _ur

                node = args.node_name or _socket.gethostname()
                payload = json.loads(manager._last_info.to_json())
                payload["in_use"] = manager.in_use_uuids()
                req = _ur.Request(
                    f"{args.extender_url.rstrip('/')}/v1/nodes/{node}",
                    data=json.dumps(payload).encode(),
                    headers={"Content-Type": "application/json"},
                    method="POST",
                )
                _ur.urlopen(req, timeout=10).read()
            except Exception as e:
                utils.logf(2, "agent: extender registration failed: %s", e)
        # kubelet is the allocation source of truth on the stock path:
        # reconcile in_use from its pod-resources API when available
        try:
            from .podresources import PodResourcesClient, reconcile_in_use

            client = (PodResourcesClient(args.pod_resources_socket)
                      if args.pod_resources_socket else PodResourcesClient())
            reconcile_in_use(manager, client)
        except Exception as e:  # never let reconcile kill the agent
            utils.logf(2, "agent: pod-resources reconcile error: %s", e)
        # active integrity probes: one child process per idle GPU,
        # after reconcile so in_use is current; a failed verdict flips
        # device_health(), so wake ListAndWatch again afterwards.  Their
        # children share one lock, so no two overlap on a GPU.
        for probe in PROBE_NAMES:
            interval = getattr(args, f"{probe}_interval")
            if not (interval > 0 and time.monotonic() >= next_due[probe]):
                continue
            next_due[probe] = time.monotonic() + interval
            try:
                mod = importlib.import_module(f"..probe.{probe}", __package__)
                if probe in ("memcheck", "hostlink"):
                    size = getattr(args, f"{probe}_bytes")
                else:
                    size = getattr(args, f"{probe}_rounds") or mod.DEFAULT_ROUNDS
                extra = {"min_gbps": args.hostlink_min_gbps} if probe == "hostlink" else {}
                getattr(mod, f"{probe}_round")(
                    manager, getattr(mod, f"run_{probe}_subprocess"), METRICS, size,
                    max_process_count=getattr(args, f"{probe}_max_procs"), **extra)
            except Exception as e:  # never let the probe kill the agent
                utils.errorf("agent: " + probe + " round failed: %s", e)
            plugin.servicer.notify()
        for uuid, ok in manager.device_health().items():
            g = manager.gpu_or_tombstone(uuid)
            METRICS.set_gpu_health(
                uuid, ok, g.ecc_uncorrectable if g is not None else 0
            )
            METRICS.set_gpu_in_use(
                uuid, bool(g.in_use) if g is not None else False
            )
        time.sleep(args.health_interval if registered else 5.0)

    plugin.stop()
    return 0


if __name__ == "__main__":
    sys.exit(main())
