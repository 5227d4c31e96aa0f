"""Host-link integrity probe — everything that needs no GPU: the result
type, the floor logic, the manager's verdict handling, the round driver
with fake runners, metrics, the sysfs link reader, CLI and agent flags."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import hostlink as hl
from kubegpu_amd.probe import memcheck as mc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIELDS = {
    "ok", "bytes_tested", "passes", "mismatched_words", "first_bad_offset",
    "bad_bits_mask", "records", "records_dropped", "cpu_sample_mismatches",
    "elapsed_s", "kernel_h2d_gbps", "kernel_d2h_gbps", "copy_h2d_gbps",
    "copy_d2h_gbps", "duplex_gbps", "min_gbps", "below_floor", "link",
}
LINK = {"speed_gts": 32.0, "max_speed_gts": 32.0, "width": 16, "max_width": 16,
        "numa_node": 1, "downtrained": False}
RECORD = {"pass": 4, "path": "kernel_read", "offset": 4096, "word_index": 1024,
          "expected": 0x1234, "got": 0x1235}
PASS = {"ok": True, "bytes_tested": 1 << 20, "passes": 8, "mismatched_words": 0,
        "first_bad_offset": None, "bad_bits_mask": 0, "records": [],
        "cpu_sample_mismatches": 0, "kernel_h2d_gbps": 50.0, "kernel_d2h_gbps": 48.0,
        "copy_h2d_gbps": 55.0, "copy_d2h_gbps": 54.0, "duplex_gbps": 90.0}
FAIL = dict(PASS, ok=False, mismatched_words=1, first_bad_offset=4096, bad_bits_mask=1,
            records=[RECORD])
MEM_FAIL = {"ok": False, "mismatched_words": 3, "first_bad_offset": 64, "bad_bits_mask": 0x10}
CU_FAIL = {"ok": False, "mismatches": 4, "first_bad_round": 1, "bad_stages": ["valu"],
           "bad_cus": ["3/1/0/7"]}


# -- result type -------------------------------------------------------------------

def test_result_to_dict_round_trips_json():
    res = hl.HostlinkResult(
        ok=False, bytes_tested=64, passes=8, mismatched_words=2, first_bad_offset=4096,
        bad_bits_mask=0x80000001, records=[dict(RECORD)], records_dropped=1,
        cpu_sample_mismatches=0, elapsed_s=0.25, kernel_h2d_gbps=51.5,
        kernel_d2h_gbps=49.0, copy_h2d_gbps=56.0, copy_d2h_gbps=55.0, duplex_gbps=92.0,
        link=dict(LINK))
    d = json.loads(json.dumps(res.to_dict()))
    assert set(d) == FIELDS
    assert d == res.to_dict()
    assert d["records"] == [RECORD] and d["link"] == LINK
    assert d["ok"] is False and d["below_floor"] is False and d["min_gbps"] == 0.0
    # defaults: a fresh result is a clean one, and link may be absent
    fresh = json.loads(json.dumps(hl.HostlinkResult().to_dict()))
    assert set(fresh) == FIELDS
    assert fresh["ok"] is True and fresh["link"] is None and fresh["records"] == []
    assert fresh["first_bad_offset"] is None


def test_pass_table():
    assert hl.PASS_PATHS == ("kernel_write", "kernel_read", "copy_h2d", "copy_d2h",
                             "kernel_read", "host_write", "duplex", "kernel_read")
    assert hl.DEFAULT_BYTES == 256 << 20


def test_below_floor_logic():
    res = hl.HostlinkResult(kernel_h2d_gbps=50.0, kernel_d2h_gbps=48.0,
                            copy_h2d_gbps=55.0, copy_d2h_gbps=54.0, duplex_gbps=10.0)
    res.apply_floor(0.0)  # off: nothing is below
    assert res.below_floor is False and res.min_gbps == 0.0
    res.apply_floor(48.0)  # at the floor is not under it
    assert res.below_floor is False and res.min_gbps == 48.0
    res.apply_floor(48.5)  # one figure under
    assert res.below_floor is True
    for name in ("kernel_h2d_gbps", "kernel_d2h_gbps", "copy_h2d_gbps", "copy_d2h_gbps"):
        r = hl.HostlinkResult(kernel_h2d_gbps=50.0, kernel_d2h_gbps=50.0,
                              copy_h2d_gbps=50.0, copy_d2h_gbps=50.0)
        setattr(r, name, 39.9)
        r.apply_floor(40.0)
        assert r.below_floor is True, name
    # the duplex figure is not a one-way figure, and ok is never touched
    res.duplex_gbps = 1.0
    res.apply_floor(40.0)
    assert res.below_floor is False and res.ok is True
    res.apply_floor(1e9)
    assert res.below_floor is True and res.ok is True


def test_sample_vectors():
    v = hl._sample_vectors(1 << 20, 7)
    assert v.dtype == np.int64 and np.array_equal(v, np.unique(v))
    assert set(range(256)) <= set(v.tolist())  # first 4 KiB
    assert set(range((1 << 20) - 256, 1 << 20)) <= set(v.tolist())  # last 4 KiB
    picks = np.random.default_rng(7).integers(0, 1 << 20, size=64, dtype=np.int64)
    assert set(picks.tolist()) <= set(v.tolist())
    assert len(v) <= 256 + 256 + 64 and v.min() == 0 and v.max() == (1 << 20) - 1
    # a buffer smaller than the edges is covered whole, once
    assert hl._sample_vectors(2, 0).tolist() == [0, 1]


def test_host_write_matches_reference():
    n_vectors = hl._HOST_WRITE_CHUNK_VECTORS + 5  # crosses a batch boundary
    for pattern in ("checker", "addr", "walk1"):
        words = np.zeros(4 * n_vectors, dtype=np.uint32)
        hl._host_write(words, pattern, 3)
        assert np.array_equal(words, mc.reference_words(0, n_vectors, pattern, 3)), pattern


def test_hostlink_rejects_bad_size_before_touching_a_gpu():
    for nbytes in (0, -32, 16, 48, (1 << 20) + 16):
        with pytest.raises(ValueError):
            hl.hostlink(nbytes=nbytes)


def test_lazy_reexports():
    from kubegpu_amd import probe

    for name in ("HostlinkResult", "hostlink_round", "read_pcie_link",
                 "run_hostlink_subprocess"):
        assert getattr(probe, name) is getattr(hl, name)
    # the three probes' children share one lock, and one pattern definition
    assert hl._child_lock is mc._child_lock
    assert hl.reference_words is mc.reference_words
    assert probe.fill_pattern is mc.fill_pattern  # package-level names stay memcheck's


def test_shared_header_is_part_of_the_staleness_check(monkeypatch):
    from kubegpu_amd import build_native

    seen = []

    def needs_build(target, *sources):
        seen.append(sources)
        return False  # up to date: build_gpuprobe returns without compiling

    monkeypatch.setattr(build_native, "_needs_build", needs_build)
    build_native.build_gpuprobe(verbose=False)
    assert seen
    for sources in seen:
        names = {os.path.basename(s) for s in sources}
        assert {"hostlink.hip", "memcheck.hip", "pattern_common.h"} <= names
        assert all(os.path.exists(s) for s in sources)


# -- manager verdicts ------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


def test_failed_verdict_drops_health_and_allocatable():
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.hostlink == {} and mgr.hostlink_status(uuid) is None

    assert mgr.record_hostlink(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.hostlink_status(uuid)
    assert st["ok"] is False and st["mismatched_words"] == 1 and "timestamp" in st
    assert mgr.memcheck_status(uuid) is None and mgr.cucheck_status(uuid) is None

    # a later passing verdict restores the GPU, and so does clear_hostlink
    assert mgr.record_hostlink(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True
    assert _node_info(mgr).allocatable == base.allocatable
    mgr.record_hostlink(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_hostlink(uuid) is True
    assert mgr.clear_hostlink(uuid) is False
    assert mgr.hostlink_status(uuid) is None
    assert mgr.device_health()[uuid] is True


def test_cpu_sample_mismatch_alone_fails_the_verdict():
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[0]
    assert mgr.record_hostlink(uuid, dict(PASS, cpu_sample_mismatches=2)) is False
    assert mgr.device_health()[uuid] is False


def test_below_floor_alone_leaves_the_gpu_healthy():
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[0]
    assert mgr.record_hostlink(uuid, dict(PASS, below_floor=True, min_gbps=60.0)) is True
    assert mgr.device_health()[uuid] is True
    assert mgr.hostlink_status(uuid)["below_floor"] is True


def test_failure_log_names_pass_path_and_offset(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[0]
    mgr.record_hostlink(uuid, PASS)
    assert lines == []
    mgr.record_hostlink(uuid, FAIL)
    assert len(lines) == 1
    assert uuid in lines[0] and "pass 4" in lines[0] and "kernel_read" in lines[0]
    assert "offset 4096" in lines[0]


def test_verdict_is_independent_of_memcheck_and_cucheck():
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[1]
    mgr.record_memcheck(uuid, {"ok": True, "mismatched_words": 0})
    mgr.record_cucheck(uuid, {"ok": True, "mismatches": 0})
    mgr.record_hostlink(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.memcheck_status(uuid)["ok"] and mgr.cucheck_status(uuid)["ok"]
    mgr.clear_memcheck(uuid)
    mgr.clear_cucheck(uuid)
    assert mgr.device_health()[uuid] is False  # clearing the others does not help
    mgr.clear_hostlink(uuid)
    assert mgr.device_health()[uuid] is True
    # and the other way round: a passing hostlink does not hide the others
    mgr.record_hostlink(uuid, PASS)
    mgr.record_memcheck(uuid, MEM_FAIL)
    assert mgr.device_health()[uuid] is False
    mgr.clear_memcheck(uuid)
    mgr.record_cucheck(uuid, CU_FAIL)
    assert mgr.device_health()[uuid] is False
    mgr.clear_cucheck(uuid)
    assert mgr.device_health()[uuid] is True


def test_unknown_uuid_is_rejected():
    mgr = _mgr()
    with pytest.raises(KeyError):
        mgr.record_hostlink("GPU-does-not-exist", FAIL)
    assert mgr.hostlink == {}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_hostlink(uuid, FAIL)
    before = mgr.gpus[uuid]
    mgr.update_gpu_info(force=True)
    assert mgr.gpus[uuid] is not before  # GpuInfo was replaced...
    assert mgr.device_health()[uuid] is False  # ...the verdict was not

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.hostlink_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.hostlink_status(uuid) is None


# -- hostlink_round ----------------------------------------------------------------

def _fake_sysfs(root, bdf, speed="32.0 GT/s PCIe", max_speed="32.0 GT/s PCIe",
                width="16", max_width="16", numa="1", skip=()):
    d = root / "bus" / "pci" / "devices" / bdf
    d.mkdir(parents=True)
    for name, text in (("current_link_speed", speed), ("max_link_speed", max_speed),
                       ("current_link_width", width), ("max_link_width", max_width),
                       ("numa_node", numa)):
        if name not in skip:
            (d / name).write_text(text + "\n")
    return str(root)


def test_round_skips_busy_gpus_records_failures_and_attaches_link(tmp_path, monkeypatch):
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    # only GPU 0's device has link files; read through the real reader
    root = _fake_sysfs(tmp_path, mgr.gpus[by_index[0]].bdf, width="8")
    real = hl.read_pcie_link
    monkeypatch.setattr(hl, "read_pcie_link", lambda bdf: real(bdf, sysfs_root=root))
    calls = []

    def runner(index, nbytes):
        calls.append((index, nbytes))
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = hl.hostlink_round(mgr, runner, metrics, nbytes=1 << 20)
    assert calls == [(i, 1 << 20) for i in (0, 3, 4, 5, 6, 7)]  # index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.hostlink_status(by_index[1]) is None
    assert out[by_index[0]]["link"] == dict(LINK, width=8, downtrained=True)
    assert mgr.hostlink_status(by_index[0])["link"]["downtrained"] is True
    assert out[by_index[3]]["link"] is None  # no sysfs entry: informative only
    assert health[by_index[0]] is True  # a downtrained link is not a verdict
    assert metrics.gpu_hostlink[by_index[5]]["mismatches"] == 1
    assert metrics.gpu_hostlink[by_index[0]] == {
        "mismatches": 0, "h2d_gbps": 50.0, "d2h_gbps": 48.0, "below_floor": False,
        "timestamp": metrics.gpu_hostlink[by_index[0]]["timestamp"]}
    assert metrics.gpu_hostlink_errors == {}
    assert all(r["below_floor"] is False and r["min_gbps"] == 0.0 for r in out.values())

    # the ceiling moves with max_process_count; None ignores the field
    calls.clear()
    hl.hostlink_round(mgr, runner, None, nbytes=64, max_process_count=4)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]
    calls.clear()
    hl.hostlink_round(mgr, runner, None, nbytes=64, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_below_floor_is_reported_and_leaves_health_alone(monkeypatch):
    from kubegpu_amd.api import utils
    from kubegpu_amd.metrics import Metrics

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    before = mgr.device_health()

    def runner(index, nbytes):
        return dict(PASS, exit_code=0, kernel_d2h_gbps=12.0 if index == 2 else 48.0)

    metrics = Metrics()
    out = hl.hostlink_round(mgr, runner, metrics, nbytes=64, min_gbps=40.0)
    assert mgr.device_health() == before and all(before.values())
    assert [u for u, r in out.items() if r["below_floor"]] == [by_index[2]]
    assert all(r["min_gbps"] == 40.0 and r["ok"] for r in out.values())
    assert metrics.gpu_hostlink[by_index[2]]["below_floor"] is True
    assert metrics.gpu_hostlink[by_index[3]]["below_floor"] is False
    assert len(lines) == 1 and by_index[2] in lines[0] and "floor" in lines[0]


def test_round_runner_errors_leave_health_unchanged():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_hostlink(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, nbytes):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("hostlink", 1.0)
        if index in (2, 3):
            return {"error": "hipHostMalloc failed", "exit_code": 2}
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = hl.hostlink_round(mgr, runner, metrics, nbytes=64)
    assert mgr.device_health() == before
    assert mgr.hostlink_status(by_index[3])["ok"] is False
    for i in (0, 1, 2):
        assert mgr.hostlink_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_hostlink_errors == {by_index[i]: 1 for i in (0, 1, 2, 3)}
    assert set(metrics.gpu_hostlink) == {by_index[i] for i in (4, 5, 6, 7)}


# -- metrics -------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_hostlink("GPU-a", 2, 51.5, 49.25, True, 1700000000.0)
        m.inc_hostlink_error("GPU-a")
        m.inc_hostlink_error("GPU-a")
        assert m.gpu_hostlink["GPU-a"] == {
            "mismatches": 2, "h2d_gbps": 51.5, "d2h_gbps": 49.25, "below_floor": True,
            "timestamp": 1700000000.0}
        assert m.gpu_hostlink_errors["GPU-a"] == 2
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_hostlink_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_hostlink_h2d_gbps", lab) == 51.5
        assert reg.get_sample_value("kubegpu_amd_gpu_hostlink_d2h_gbps", lab) == 49.25
        assert reg.get_sample_value("kubegpu_amd_gpu_hostlink_below_floor", lab) == 1.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_hostlink_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_hostlink_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert b"ECC/vanished/memcheck/cucheck/hostlink" in generate_latest(reg)
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- read_pcie_link --------------------------------------------------------------------

BDF = "0000:c1:00.0"


def test_read_pcie_link_healthy(tmp_path):
    root = _fake_sysfs(tmp_path, BDF)
    assert hl.read_pcie_link(BDF, sysfs_root=root) == LINK


def test_read_pcie_link_downtrained(tmp_path):
    root = _fake_sysfs(tmp_path / "w", BDF, width="8")
    got = hl.read_pcie_link(BDF, sysfs_root=root)
    assert got["width"] == 8 and got["max_width"] == 16 and got["downtrained"] is True
    root = _fake_sysfs(tmp_path / "s", BDF, speed="8.0 GT/s PCIe", numa="-1")
    got = hl.read_pcie_link(BDF, sysfs_root=root)
    assert got["speed_gts"] == 8.0 and got["max_speed_gts"] == 32.0
    assert got["downtrained"] is True and got["numa_node"] == -1
    root = _fake_sysfs(tmp_path / "i", BDF, speed="2.5 GT/s", max_speed="2.5 GT/s")
    assert hl.read_pcie_link(BDF, sysfs_root=root)["downtrained"] is False


def test_read_pcie_link_missing(tmp_path):
    assert hl.read_pcie_link(BDF, sysfs_root=str(tmp_path)) is None  # no device
    assert hl.read_pcie_link("", sysfs_root=str(tmp_path)) is None
    for name in ("current_link_speed", "max_link_speed", "current_link_width",
                 "max_link_width", "numa_node"):
        root = _fake_sysfs(tmp_path / name, BDF, skip=(name,))
        assert hl.read_pcie_link(BDF, sysfs_root=root) is None, name


def test_read_pcie_link_garbled(tmp_path):
    cases = (dict(speed="Unknown"), dict(max_speed="fast"), dict(width="x16"),
             dict(max_width=""), dict(numa="none"), dict(width="0"))
    for k, kw in enumerate(cases):
        root = _fake_sysfs(tmp_path / str(k), BDF, **kw)
        assert hl.read_pcie_link(BDF, sysfs_root=root) is None, kw


# -- CLI and agent ---------------------------------------------------------------------

def test_amddevs_fake_hostlink_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--hostlink", "--bytes", "1048576"]) == 2
    cap = capsys.readouterr()
    assert "--hostlink needs real GPUs" in cap.err
    assert cap.out == ""


def test_agent_oneshot_accepts_hostlink_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "h.sock"),
                              "--hostlink-interval", "600", "--hostlink-bytes", "1048576",
                              "--hostlink-max-procs", "2",
                              "--hostlink-min-gbps", "40"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1
    # off by default
    assert agent.main(base + ["--socket", str(sock_dir / "d.sock")]) == 0


def test_hostlink_cli_child_without_gpu_exits_2():
    """Started as a child where no GPU can be seen: exactly one JSON line
    with an error field, exit 2."""
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env["PYTHONPATH"] \
        if env.get("PYTHONPATH") else REPO
    env["HIP_VISIBLE_DEVICES"] = "-1"  # no GPU for the child, wherever this runs
    env["CUDA_VISIBLE_DEVICES"] = "-1"
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.hostlink",
         "--device", "0", "--bytes", "1048576", "--min-gbps", "1"],
        capture_output=True, timeout=120, cwd=REPO, env=env, text=True,
    )
    assert res.returncode == 2, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
    assert "mismatched_words" not in rec
