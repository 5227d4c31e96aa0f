"""Prometheus metrics (the reference has none; the build
adds pod-schedule latency and xGMI utilization per BASELINE.json).

Soft dependency: when prometheus_client is unavailable everything
degrades to in-memory counters so the control plane never hard-requires
a metrics stack.
"""

from __future__ import annotations

import threading
from typing import Dict, List, Optional

from .probe._active import PROBE_NAMES

try:
    from prometheus_client import (
        CollectorRegistry,
        Counter,
        Gauge,
        Histogram,
        start_http_server,
    )

    _HAVE_PROM = True
except ImportError:  # pragma: no cover
    _HAVE_PROM = False


# Per-GPU metrics of the active probes: probe -> rows of (attribute
# suffix, "gauge" or "counter", metric suffix, help).  The attribute is
# _<probe>_<suffix>, the metric kubegpu_amd_gpu_<probe>_<suffix>; all
# are labelled by uuid and declared in this order.
_PROBE_METRICS = {
    "memcheck": (
        ("words", "gauge", "mismatched_words",
         "32-bit words that read back wrong in the last HBM memcheck"),
        ("gbps", "gauge", "gbps", "throughput of the last HBM memcheck, GB/s"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed HBM memcheck"),
        ("err", "counter", "errors_total",
         "HBM memcheck runs that could not complete (not a memory fault)"),
    ),
    "cucheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last compute-unit cucheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last cucheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed compute-unit cucheck"),
        ("err", "counter", "errors_total",
         "cucheck runs that could not complete (not a compute fault)"),
    ),
    "mxcheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last matrix-core format mxcheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last mxcheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed matrix-core format mxcheck"),
        ("err", "counter", "errors_total",
         "mxcheck runs that could not complete (not a matrix-core fault)"),
    ),
    "fpcheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last IEEE rounding fpcheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last fpcheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed IEEE rounding fpcheck"),
        ("err", "counter", "errors_total",
         "fpcheck runs that could not complete (not a rounding fault)"),
    ),
    "hostlink": (
        ("words", "gauge", "mismatches",
         "32-bit words that crossed the host link wrong in the last hostlink"),
        ("h2d", "gauge", "h2d_gbps",
         "host-to-device bandwidth of GPU loads from pinned host memory "
         "in the last hostlink, GB/s"),
        ("d2h", "gauge", "d2h_gbps",
         "device-to-host bandwidth of GPU stores to pinned host memory "
         "in the last hostlink, GB/s"),
        ("floor", "gauge", "below_floor",
         "1 = a one-way figure of the last hostlink was under the "
         "configured floor (health unaffected)"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed hostlink"),
        ("err", "counter", "errors_total",
         "hostlink runs that could not complete (not a link fault)"),
    ),
    "atomcheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last atomic-unit atomcheck"),
        ("shared", "gauge", "shared_mismatches",
         "cells of the cross-workgroup region that came out wrong in the last atomcheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last atomcheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed atomic-unit atomcheck"),
        ("err", "counter", "errors_total",
         "atomcheck runs that could not complete (not an atomic-unit fault)"),
    ),
    "lanecheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last cross-lane lanecheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last lanecheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed cross-lane lanecheck"),
        ("err", "counter", "errors_total",
         "lanecheck runs that could not complete (not a cross-lane fault)"),
    ),
    "ldscheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last LDS ldscheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last ldscheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed LDS ldscheck"),
        ("err", "counter", "errors_total",
         "ldscheck runs that could not complete (not an LDS fault)"),
    ),
    "vmemcheck": (
        ("mismatches", "gauge", "mismatches",
         "wave digests that came out wrong in the last vector-memory vmemcheck"),
        ("cus", "gauge", "cus_covered",
         "distinct compute units that ran a wave of the last vmemcheck"),
        ("ts", "gauge", "last_run_timestamp_seconds",
         "unix time of the last completed vector-memory vmemcheck"),
        ("err", "counter", "errors_total",
         "vmemcheck runs that could not complete (not a memory-path fault)"),
    ),
}


class Metrics:
    def __init__(self, registry=None) -> None:
        self._lock = threading.Lock()
        self.schedule_latencies: List[float] = []
        self.allocations = 0
        self.failures = 0
        self.gpu_health: Dict[str, bool] = {}
        self.gpu_in_use: Dict[str, bool] = {}
        # gpu_<probe>: uuid -> what the last run's setter was given;
        # gpu_<probe>_errors: uuid -> runs that could not complete
        for probe in PROBE_NAMES:
            setattr(self, f"gpu_{probe}", {})
            setattr(self, f"gpu_{probe}_errors", {})
        if _HAVE_PROM:
            # per-instance registry: multiple Metrics objects (tests,
            # embedded schedulers) must not collide in the global one
            self.registry = registry if registry is not None else CollectorRegistry()
            self._h = Histogram(
                "kubegpu_amd_schedule_latency_seconds",
                "pod schedule latency",
                buckets=(1e-5, 1e-4, 5e-4, 1e-3, 5e-3, 1e-2, 0.1, 1.0),
                registry=self.registry,
            )
            self._alloc = Counter(
                "kubegpu_amd_allocations_total", "pod GPU allocations",
                registry=self.registry,
            )
            self._fail = Counter(
                "kubegpu_amd_schedule_failures_total", "schedule failures",
                registry=self.registry,
            )
            self._xgmi = Gauge(
                "kubegpu_amd_xgmi_link_gbps", "last probed xGMI ring bandwidth GB/s",
                registry=self.registry,
            )
            self._gpu_health = Gauge(
                "kubegpu_amd_gpu_healthy",
                "1 = GPU healthy, 0 = unhealthy (ECC/vanished/memcheck/cucheck/hostlink/fpcheck/mxcheck)/atomcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._gpu_ecc = Gauge(
                "kubegpu_amd_gpu_ecc_uncorrectable",
                "accumulated uncorrectable ECC errors",
                ["uuid"],
                registry=self.registry,
            )
            self._gpu_in_use = Gauge(
                "kubegpu_amd_gpu_in_use",
                "1 = GPU held by a live allocation (manager path)",
                ["uuid"],
                registry=self.registry,
            )
            for probe in PROBE_NAMES:
                for attr, kind, name, help_text in _PROBE_METRICS[probe]:
                    setattr(self, f"_{probe}_{attr}",
                            (Gauge if kind == "gauge" else Counter)(
                                f"kubegpu_amd_gpu_{probe}_{name}", help_text,
                                ["uuid"], registry=self.registry))

    def observe_schedule(self, seconds: float) -> None:
        with self._lock:
            self.schedule_latencies.append(seconds)
        if _HAVE_PROM:
            self._h.observe(seconds)

    def inc_allocation(self) -> None:
        with self._lock:
            self.allocations += 1
        if _HAVE_PROM:
            self._alloc.inc()

    def inc_failure(self) -> None:
        with self._lock:
            self.failures += 1
        if _HAVE_PROM:
            self._fail.inc()

    def set_xgmi_gbps(self, gbps: float) -> None:
        if _HAVE_PROM:
            self._xgmi.set(gbps)

    def set_gpu_health(self, uuid: str, healthy: bool, ecc_uncorrectable: int = 0) -> None:
        with self._lock:
            self.gpu_health[uuid] = healthy
        if _HAVE_PROM:
            self._gpu_health.labels(uuid=uuid).set(1.0 if healthy else 0.0)
            self._gpu_ecc.labels(uuid=uuid).set(float(ecc_uncorrectable))

    def set_gpu_in_use(self, uuid: str, in_use: bool) -> None:
        with self._lock:
            self.gpu_in_use[uuid] = in_use
        if _HAVE_PROM:
            self._gpu_in_use.labels(uuid=uuid).set(1.0 if in_use else 0.0)

    def _set_gpu_probe(self, probe: str, uuid: str, values: dict, timestamp: float) -> None:
        """Export a completed run: ``values`` maps the key kept in
        ``gpu_<probe>[uuid]`` to (value, attribute suffix of its gauge)."""
        record = {key: v for key, (v, _) in values.items()}
        record["timestamp"] = float(timestamp)
        with self._lock:
            getattr(self, f"gpu_{probe}")[uuid] = record
        if _HAVE_PROM:
            for v, attr in values.values():
                getattr(self, f"_{probe}_{attr}").labels(uuid=uuid).set(float(v))
            getattr(self, f"_{probe}_ts").labels(uuid=uuid).set(float(timestamp))

    def _inc_probe_error(self, probe: str, uuid: str) -> None:
        with self._lock:
            errors = getattr(self, f"gpu_{probe}_errors")
            errors[uuid] = errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            getattr(self, f"_{probe}_err").labels(uuid=uuid).inc()

    def _set_gpu_digests(self, probe: str, uuid: str, mismatches: int, cus_covered: int,
                         timestamp: float) -> None:
        self._set_gpu_probe(probe, uuid, {
            "mismatches": (int(mismatches), "mismatches"),
            "cus_covered": (int(cus_covered), "cus"),
        }, timestamp)

    def set_gpu_memcheck(self, uuid: str, mismatched_words: int, gbps: float,
                         timestamp: float) -> None:
        self._set_gpu_probe("memcheck", uuid, {
            "mismatched_words": (int(mismatched_words), "words"),
            "gbps": (float(gbps), "gbps"),
        }, timestamp)

    def inc_memcheck_error(self, uuid: str) -> None:
        self._inc_probe_error("memcheck", uuid)

    def set_gpu_cucheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        self._set_gpu_digests("cucheck", uuid, mismatches, cus_covered, timestamp)

    def inc_cucheck_error(self, uuid: str) -> None:
        self._inc_probe_error("cucheck", uuid)

    def set_gpu_mxcheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        self._set_gpu_digests("mxcheck", uuid, mismatches, cus_covered, timestamp)

    def inc_mxcheck_error(self, uuid: str) -> None:
        self._inc_probe_error("mxcheck", uuid)

    def set_gpu_fpcheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        self._set_gpu_digests("fpcheck", uuid, mismatches, cus_covered, timestamp)

    def inc_fpcheck_error(self, uuid: str) -> None:
        self._inc_probe_error("fpcheck", uuid)

    def set_gpu_hostlink(self, uuid: str, mismatches: int, h2d_gbps: float,
                         d2h_gbps: float, below_floor: bool, timestamp: float) -> None:
        self._set_gpu_probe("hostlink", uuid, {
            "mismatches": (int(mismatches), "words"),
            "h2d_gbps": (float(h2d_gbps), "h2d"),
            "d2h_gbps": (float(d2h_gbps), "d2h"),
            "below_floor": (bool(below_floor), "floor"),
        }, timestamp)

    def inc_hostlink_error(self, uuid: str) -> None:
        self._inc_probe_error("hostlink", uuid)

    def set_gpu_atomcheck(self, uuid: str, mismatches: int, shared_mismatches: int,
                          cus_covered: int, timestamp: float) -> None:
        self._set_gpu_probe("atomcheck", uuid, {
            "mismatches": (int(mismatches), "mismatches"),
            "shared_mismatches": (int(shared_mismatches), "shared"),
            "cus_covered": (int(cus_covered), "cus"),
        }, timestamp)

    def inc_atomcheck_error(self, uuid: str) -> None:
        self._inc_probe_error("atomcheck", uuid)

    def set_gpu_lanecheck(self, uuid: str, mismatches: int, cus_covered: int,
                          timestamp: float) -> None:
        self._set_gpu_digests("lanecheck", uuid, mismatches, cus_covered, timestamp)

    def inc_lanecheck_error(self, uuid: str) -> None:
        self._inc_probe_error("lanecheck", uuid)

    def set_gpu_ldscheck(self, uuid: str, mismatches: int, cus_covered: int,
                         timestamp: float) -> None:
        self._set_gpu_digests("ldscheck", uuid, mismatches, cus_covered, timestamp)

    def inc_ldscheck_error(self, uuid: str) -> None:
        self._inc_probe_error("ldscheck", uuid)

    def set_gpu_vmemcheck(self, uuid: str, mismatches: int, cus_covered: int,
                          timestamp: float) -> None:
        self._set_gpu_digests("vmemcheck", uuid, mismatches, cus_covered, timestamp)

    def inc_vmemcheck_error(self, uuid: str) -> None:
        self._inc_probe_error("vmemcheck", uuid)

    def percentile(self, q: float) -> Optional[float]:
        with self._lock:
            if not self.schedule_latencies:
                return None
            data = sorted(self.schedule_latencies)
            idx = min(len(data) - 1, int(q * len(data)))
            return data[idx]

    def serve(self, port: int = 9400) -> bool:
        if _HAVE_PROM:
            start_http_server(port, registry=self.registry)
            return True
        return False


METRICS = Metrics()
