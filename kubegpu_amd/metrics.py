"""Prometheus metrics (the reference has none; the build
adds pod-schedule latency and xGMI utilization per BASELINE.json).

Soft dependency: when prometheus_client is unavailable everything
degrades to in-memory counters so the control plane never hard-requires
a metrics stack.
"""

from __future__ import annotations

import threading
from typing import Dict, List, Optional

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


class Metrics:
    def __init__(self, registry=None) -> None:
        self._lock = threading.Lock()
        self.schedule_latencies: List[float] = []
        self.allocations = 0
        self.failures = 0
        self.gpu_health: Dict[str, bool] = {}
        self.gpu_in_use: Dict[str, bool] = {}
        self.gpu_memcheck: Dict[str, dict] = {}
        self.gpu_memcheck_errors: Dict[str, int] = {}
        self.gpu_cucheck: Dict[str, dict] = {}
        self.gpu_cucheck_errors: Dict[str, int] = {}
        self.gpu_mxcheck: Dict[str, dict] = {}
        self.gpu_mxcheck_errors: Dict[str, int] = {}
        self.gpu_fpcheck: Dict[str, dict] = {}
        self.gpu_fpcheck_errors: Dict[str, int] = {}
        self.gpu_hostlink: Dict[str, dict] = {}
        self.gpu_hostlink_errors: Dict[str, int] = {}
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
                "1 = GPU healthy, 0 = unhealthy (ECC/vanished/memcheck/cucheck/hostlink/fpcheck/mxcheck)",
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
            self._memcheck_words = Gauge(
                "kubegpu_amd_gpu_memcheck_mismatched_words",
                "32-bit words that read back wrong in the last HBM memcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._memcheck_gbps = Gauge(
                "kubegpu_amd_gpu_memcheck_gbps",
                "throughput of the last HBM memcheck, GB/s",
                ["uuid"],
                registry=self.registry,
            )
            self._memcheck_ts = Gauge(
                "kubegpu_amd_gpu_memcheck_last_run_timestamp_seconds",
                "unix time of the last completed HBM memcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._memcheck_err = Counter(
                "kubegpu_amd_gpu_memcheck_errors_total",
                "HBM memcheck runs that could not complete (not a memory fault)",
                ["uuid"],
                registry=self.registry,
            )
            self._cucheck_mismatches = Gauge(
                "kubegpu_amd_gpu_cucheck_mismatches",
                "wave digests that came out wrong in the last compute-unit cucheck",
                ["uuid"],
                registry=self.registry,
            )
            self._cucheck_cus = Gauge(
                "kubegpu_amd_gpu_cucheck_cus_covered",
                "distinct compute units that ran a wave of the last cucheck",
                ["uuid"],
                registry=self.registry,
            )
            self._cucheck_ts = Gauge(
                "kubegpu_amd_gpu_cucheck_last_run_timestamp_seconds",
                "unix time of the last completed compute-unit cucheck",
                ["uuid"],
                registry=self.registry,
            )
            self._cucheck_err = Counter(
                "kubegpu_amd_gpu_cucheck_errors_total",
                "cucheck runs that could not complete (not a compute fault)",
                ["uuid"],
                registry=self.registry,
            )
            self._mxcheck_mismatches = Gauge(
                "kubegpu_amd_gpu_mxcheck_mismatches",
                "wave digests that came out wrong in the last matrix-core format mxcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._mxcheck_cus = Gauge(
                "kubegpu_amd_gpu_mxcheck_cus_covered",
                "distinct compute units that ran a wave of the last mxcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._mxcheck_ts = Gauge(
                "kubegpu_amd_gpu_mxcheck_last_run_timestamp_seconds",
                "unix time of the last completed matrix-core format mxcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._mxcheck_err = Counter(
                "kubegpu_amd_gpu_mxcheck_errors_total",
                "mxcheck runs that could not complete (not a matrix-core fault)",
                ["uuid"],
                registry=self.registry,
            )
            self._fpcheck_mismatches = Gauge(
                "kubegpu_amd_gpu_fpcheck_mismatches",
                "wave digests that came out wrong in the last IEEE rounding fpcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._fpcheck_cus = Gauge(
                "kubegpu_amd_gpu_fpcheck_cus_covered",
                "distinct compute units that ran a wave of the last fpcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._fpcheck_ts = Gauge(
                "kubegpu_amd_gpu_fpcheck_last_run_timestamp_seconds",
                "unix time of the last completed IEEE rounding fpcheck",
                ["uuid"],
                registry=self.registry,
            )
            self._fpcheck_err = Counter(
                "kubegpu_amd_gpu_fpcheck_errors_total",
                "fpcheck runs that could not complete (not a rounding fault)",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_words = Gauge(
                "kubegpu_amd_gpu_hostlink_mismatches",
                "32-bit words that crossed the host link wrong in the last hostlink",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_h2d = Gauge(
                "kubegpu_amd_gpu_hostlink_h2d_gbps",
                "host-to-device bandwidth of GPU loads from pinned host memory "
                "in the last hostlink, GB/s",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_d2h = Gauge(
                "kubegpu_amd_gpu_hostlink_d2h_gbps",
                "device-to-host bandwidth of GPU stores to pinned host memory "
                "in the last hostlink, GB/s",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_floor = Gauge(
                "kubegpu_amd_gpu_hostlink_below_floor",
                "1 = a one-way figure of the last hostlink was under the "
                "configured floor (health unaffected)",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_ts = Gauge(
                "kubegpu_amd_gpu_hostlink_last_run_timestamp_seconds",
                "unix time of the last completed hostlink",
                ["uuid"],
                registry=self.registry,
            )
            self._hostlink_err = Counter(
                "kubegpu_amd_gpu_hostlink_errors_total",
                "hostlink runs that could not complete (not a link fault)",
                ["uuid"],
                registry=self.registry,
            )

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

    def set_gpu_memcheck(self, uuid: str, mismatched_words: int, gbps: float,
                         timestamp: float) -> None:
        with self._lock:
            self.gpu_memcheck[uuid] = {
                "mismatched_words": int(mismatched_words),
                "gbps": float(gbps),
                "timestamp": float(timestamp),
            }
        if _HAVE_PROM:
            self._memcheck_words.labels(uuid=uuid).set(float(mismatched_words))
            self._memcheck_gbps.labels(uuid=uuid).set(float(gbps))
            self._memcheck_ts.labels(uuid=uuid).set(float(timestamp))

    def inc_memcheck_error(self, uuid: str) -> None:
        with self._lock:
            self.gpu_memcheck_errors[uuid] = self.gpu_memcheck_errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            self._memcheck_err.labels(uuid=uuid).inc()

    def set_gpu_cucheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        with self._lock:
            self.gpu_cucheck[uuid] = {
                "mismatches": int(mismatches),
                "cus_covered": int(cus_covered),
                "timestamp": float(timestamp),
            }
        if _HAVE_PROM:
            self._cucheck_mismatches.labels(uuid=uuid).set(float(mismatches))
            self._cucheck_cus.labels(uuid=uuid).set(float(cus_covered))
            self._cucheck_ts.labels(uuid=uuid).set(float(timestamp))

    def inc_cucheck_error(self, uuid: str) -> None:
        with self._lock:
            self.gpu_cucheck_errors[uuid] = self.gpu_cucheck_errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            self._cucheck_err.labels(uuid=uuid).inc()

    def set_gpu_mxcheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        with self._lock:
            self.gpu_mxcheck[uuid] = {
                "mismatches": int(mismatches),
                "cus_covered": int(cus_covered),
                "timestamp": float(timestamp),
            }
        if _HAVE_PROM:
            self._mxcheck_mismatches.labels(uuid=uuid).set(float(mismatches))
            self._mxcheck_cus.labels(uuid=uuid).set(float(cus_covered))
            self._mxcheck_ts.labels(uuid=uuid).set(float(timestamp))

    def inc_mxcheck_error(self, uuid: str) -> None:
        with self._lock:
            self.gpu_mxcheck_errors[uuid] = self.gpu_mxcheck_errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            self._mxcheck_err.labels(uuid=uuid).inc()

    def set_gpu_fpcheck(self, uuid: str, mismatches: int, cus_covered: int,
                        timestamp: float) -> None:
        with self._lock:
            self.gpu_fpcheck[uuid] = {
                "mismatches": int(mismatches),
                "cus_covered": int(cus_covered),
                "timestamp": float(timestamp),
            }
        if _HAVE_PROM:
            self._fpcheck_mismatches.labels(uuid=uuid).set(float(mismatches))
            self._fpcheck_cus.labels(uuid=uuid).set(float(cus_covered))
            self._fpcheck_ts.labels(uuid=uuid).set(float(timestamp))

    def inc_fpcheck_error(self, uuid: str) -> None:
        with self._lock:
            self.gpu_fpcheck_errors[uuid] = self.gpu_fpcheck_errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            self._fpcheck_err.labels(uuid=uuid).inc()

    def set_gpu_hostlink(self, uuid: str, mismatches: int, h2d_gbps: float,
                         d2h_gbps: float, below_floor: bool, timestamp: float) -> None:
        with self._lock:
            self.gpu_hostlink[uuid] = {
                "mismatches": int(mismatches),
                "h2d_gbps": float(h2d_gbps),
                "d2h_gbps": float(d2h_gbps),
                "below_floor": bool(below_floor),
                "timestamp": float(timestamp),
            }
        if _HAVE_PROM:
            self._hostlink_words.labels(uuid=uuid).set(float(mismatches))
            self._hostlink_h2d.labels(uuid=uuid).set(float(h2d_gbps))
            self._hostlink_d2h.labels(uuid=uuid).set(float(d2h_gbps))
            self._hostlink_floor.labels(uuid=uuid).set(1.0 if below_floor else 0.0)
            self._hostlink_ts.labels(uuid=uuid).set(float(timestamp))

    def inc_hostlink_error(self, uuid: str) -> None:
        with self._lock:
            self.gpu_hostlink_errors[uuid] = self.gpu_hostlink_errors.get(uuid, 0) + 1
        if _HAVE_PROM:
            self._hostlink_err.labels(uuid=uuid).inc()

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
