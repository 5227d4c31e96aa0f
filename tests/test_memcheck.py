"""HBM integrity probe — everything that needs no GPU: the numpy pattern
definition, the manager's verdict handling, the round driver with a fake
runner, metrics, CLI and agent flags."""

import numpy as np
import pytest

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import memcheck as mc
from kubegpu_amd.probe import reference_words


# -- reference_words -----------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
def test_odd_ids_are_complements(seed):
    for even in (0, 2, 4):
        a = reference_words(5, 300, even, seed)
        b = reference_words(5, 300, even + 1, seed)
        assert a.dtype == np.uint32 and a.shape == (1200,)
        assert np.array_equal(a ^ b, np.full(1200, 0xFFFFFFFF, dtype=np.uint32))


def test_pattern_names_and_ids_agree():
    for pid, name in enumerate(mc.PATTERNS):
        assert np.array_equal(reference_words(0, 64, pid, 3), reference_words(0, 64, name, 3))
    with pytest.raises(ValueError):
        reference_words(0, 4, 6, 0)
    with pytest.raises(ValueError):
        reference_words(0, 4, "nope", 0)


def test_walk1_is_a_single_walking_bit():
    w = reference_words(0, 64, "walk1", 0)
    # word k of the buffer (k = 4v + j) holds bit k mod 32
    assert [int(x) for x in w] == [1 << (k % 32) for k in range(256)]
    # the seed rotates the start
    ws = reference_words(0, 64, "walk1", 5)
    assert [int(x) for x in ws] == [1 << ((k + 5) % 32) for k in range(256)]
    # a window elsewhere continues the same walk
    assert np.array_equal(reference_words(3, 8, "walk1", 0), w[12:44])
    w0 = reference_words(0, 64, "walk0", 0)
    assert all(bin(int(x)).count("1") == 31 for x in w0)


def test_checker_alternates_and_ignores_seed():
    c = reference_words(0, 4, "checker", 0).reshape(4, 4)
    A, B = 0xAAAAAAAA, 0x55555555
    assert c.tolist() == [[A, B, A, B], [B, A, B, A], [A, B, A, B], [B, A, B, A]]
    assert np.array_equal(reference_words(0, 64, "checker", 0),
                          reference_words(0, 64, "checker", 12345))
    # odd starting vector starts on the other phase
    assert reference_words(1, 1, "checker", 0).tolist() == [B, A, B, A]


def test_addr_definition_and_seed_dependence():
    # hand-rolled scalar version of the definition for a few vectors
    def fmix(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & 0xFFFFFFFF
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & 0xFFFFFFFF
        h ^= h >> 16
        return h

    def rotl(x, r):
        return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF if r else x

    K = [0, 0x9E3779B9, 0x7F4A7C15, 0xF39CC060]
    for seed in (0, 7, 0xDEADBEEF):
        for v in (0, 1, 255, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (5 << 32) + 9):
            lo, hi = v & 0xFFFFFFFF, v >> 32
            h = fmix(lo ^ ((hi * 0x9E3779B9) & 0xFFFFFFFF) ^ seed)
            want = [rotl(h, 8 * j) ^ K[j] for j in range(4)]
            assert reference_words(v, 1, "addr", seed).tolist() == want
    a = reference_words(0, 4096, "addr", 0)
    b = reference_words(0, 4096, "addr", 1)
    assert (a != b).mean() > 0.99
    # nearly all words distinct (the issue measured 99.98% over 8 MiB)
    big = reference_words(0, (8 << 20) // 16, "addr", 0)
    assert len(np.unique(big)) / big.size > 0.999


def test_addr_is_continuous_across_2_pow_32_vectors():
    """v = 2^32 - 1 -> 2^32: the high half of the index enters the hash,
    so the window straddling the boundary is well defined and the
    pattern does not simply wrap around to v = 0."""
    edge = (1 << 32) - 2
    w = reference_words(edge, 4, "addr", 9).reshape(4, 4)
    for k in range(4):
        assert np.array_equal(w[k], reference_words(edge + k, 1, "addr", 9))
    assert not np.array_equal(w[2], reference_words(0, 1, "addr", 9))
    assert not np.array_equal(w[3], reference_words(1, 1, "addr", 9))


# -- the 64-bit vector index ------------------------------------------------------

M32 = 0xFFFFFFFF
# where the index arithmetic changes: the walk family's u32 `v << 2` wraps;
# lo32 wraps and hi32 becomes 1; hi32 * golden wraps; 4v wraps u64; the
# largest hi32 an int64 first_vector reaches
BOUNDARIES = (1 << 30, 1 << 32, 1 << 33, 1 << 62, 0x7FFFFFFF << 32)


def scalar_words(v, pid, seed):
    """The four words of vector v straight from the module docstring's
    formulas, in Python ints masked to 32 bits."""
    def fmix32(h):
        h ^= h >> 16
        h = (h * 0x85EBCA6B) & M32
        h ^= h >> 13
        h = (h * 0xC2B2AE35) & M32
        h ^= h >> 16
        return h

    def rotl32(x, r):
        return ((x << r) | (x >> (32 - r))) & M32

    family = pid >> 1
    if family == 0:
        lo, hi = v & M32, (v >> 32) & M32
        h = fmix32(lo ^ ((hi * 0x9E3779B9) & M32) ^ seed)
        k = (0x00000000, 0x9E3779B9, 0x7F4A7C15, 0xF39CC060)
        w = [rotl32(h, 8 * j) ^ k[j] for j in range(4)]
    elif family == 1:
        c = 0xAAAAAAAA if v % 2 == 0 else 0x55555555
        w = [c if j % 2 == 0 else c ^ M32 for j in range(4)]
    else:
        w = [1 << ((4 * v + j + seed) % 32) for j in range(4)]
    return [x ^ M32 for x in w] if pid & 1 else w


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("pid", range(6))
def test_reference_matches_scalar_definition_across_index_boundaries(pid, seed):
    """Pins reference_words independently of numpy's integer promotion."""
    for first in (0,) + tuple(b - 4 for b in BOUNDARIES):
        got = reference_words(first, 8, pid, seed)
        assert got.dtype == np.uint32 and got.shape == (32,)
        want = [w for v in range(first, first + 8) for w in scalar_words(v, pid, seed)]
        assert [int(x) for x in got] == want, (hex(first), pid, seed)


@pytest.mark.parametrize("seed", [0, 0xDEADBEEF])
@pytest.mark.parametrize("v", [5, (1 << 32) - 3])
def test_addr_tells_v_from_v_plus_2_pow_32(v, seed):
    n = 64
    a = reference_words(v, n, "addr", seed).reshape(n, 4)
    b = reference_words(v + (1 << 32), n, "addr", seed).reshape(n, 4)
    assert (a[:, 0] != b[:, 0]).all()


def test_negative_first_vector_is_rejected_before_the_extension_loads(monkeypatch):
    from kubegpu_amd.probe import hostlink as hl

    def no_ext():
        raise AssertionError("the extension must not be loaded for a bad first_vector")

    monkeypatch.setattr(mc, "_ext", no_ext)
    monkeypatch.setattr(hl, "_ext", no_ext)
    calls = [
        lambda: mc.fill_pattern(None, "addr", 0, first_vector=-1),
        lambda: mc.verify_pattern(None, "addr", 0, first_vector=-1),
        lambda: mc.verify_then_fill(None, "addr", "walk1", 0, first_vector=-1),
        lambda: hl.fill_pattern(None, "addr", 0, first_vector=-1),
        lambda: hl.verify_pattern(None, "addr", 0, first_vector=-1),
        lambda: hl.duplex(None, "addr", None, "addr", 0, read_first_vector=-1),
        lambda: hl.duplex(None, "addr", None, "addr", 0, write_first_vector=-1),
    ]
    for call in calls:
        with pytest.raises(ValueError, match="first_vector"):
            call()
    # a good value gets as far as the extension
    with pytest.raises(AssertionError):
        mc.fill_pattern(None, "addr", 0, first_vector=1 << 62)


# -- manager verdicts ------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


FAIL = {"ok": False, "mismatched_words": 3, "first_bad_offset": 64,
        "bad_bits_mask": 0x10, "gbps": 4000.0, "bytes_tested": 1 << 30}
PASS = {"ok": True, "mismatched_words": 0, "first_bad_offset": None,
        "bad_bits_mask": 0, "gbps": 4000.0, "bytes_tested": 1 << 30}


def test_failed_verdict_drops_health_and_allocatable():
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    name = mgr.gpus[uuid].name
    assert mgr.memcheck_status(uuid) is None

    assert mgr.record_memcheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False
    assert sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only

    ni = _node_info(mgr)
    assert ni.capacity == base.capacity and ni.kube_cap == base.kube_cap
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    assert ni.kube_alloc[RESOURCE_GPU] == base.kube_alloc[RESOURCE_GPU] - 1 == 7
    gone = set(base.allocatable) - set(ni.allocatable)
    assert any(k.endswith(f"{name}/cards") for k in gone)
    assert any(k.endswith(f"{name}/memory") for k in gone)
    assert len(gone) == 2
    st = mgr.memcheck_status(uuid)
    assert st["ok"] is False and st["mismatched_words"] == 3 and "timestamp" in st


def test_verdict_survives_forced_rediscovery_and_is_restored():
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[0]
    mgr.record_memcheck(uuid, FAIL)
    before = mgr.gpus[uuid]
    mgr.update_gpu_info(force=True)
    assert mgr.gpus[uuid] is not before  # GpuInfo was replaced...
    assert mgr.device_health()[uuid] is False  # ...the verdict was not

    # a later passing verdict restores the GPU
    assert mgr.record_memcheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True
    ni = _node_info(mgr)
    assert ni.allocatable == base.allocatable and ni.kube_alloc == base.kube_alloc

    # and so does clear_memcheck
    mgr.record_memcheck(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_memcheck(uuid) is True
    assert mgr.clear_memcheck(uuid) is False
    assert mgr.memcheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True


def test_unknown_uuid_is_rejected():
    mgr = _mgr()
    with pytest.raises(KeyError):
        mgr.record_memcheck("GPU-does-not-exist", FAIL)
    assert mgr.memcheck == {}


def test_no_verdicts_means_identical_node_info():
    a, b = _mgr(), _mgr()
    uuid = sorted(b.gpus)[1]
    b.record_memcheck(uuid, FAIL)
    b.clear_memcheck(uuid)
    na, nb = _node_info(a), _node_info(b)
    assert na == nb
    assert a.device_health() == b.device_health()


def test_verdict_dropped_when_tombstone_expires(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    backend = FakeBackend(fix)
    mgr = create_device_plugin(backend)
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_memcheck(uuid, FAIL)
    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.memcheck_status(uuid) is not None
    assert mgr.device_health()[uuid] is False
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.memcheck_status(uuid) is None


def test_device_plugin_reports_unhealthy():
    from kubegpu_amd.server import dpapi
    from kubegpu_amd.server.kubelet_plugin import DevicePluginServicer

    mgr = _mgr()
    uuid = sorted(mgr.gpus)[5]
    servicer = DevicePluginServicer(mgr)
    assert all(d.health == dpapi.HEALTHY for d in servicer._device_list())
    mgr.record_memcheck(uuid, FAIL)
    by_id = {d.ID: d.health for d in servicer._device_list()}
    assert by_id[uuid] == dpapi.UNHEALTHY
    assert sum(1 for h in by_id.values() if h == dpapi.HEALTHY) == 7


# -- memcheck_round ----------------------------------------------------------------

def test_round_skips_busy_gpus_and_records_failures():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    calls = []

    def runner(index, nbytes):
        calls.append((index, nbytes))
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = mc.memcheck_round(mgr, runner, metrics, 1 << 20)
    assert calls == [(i, 1 << 20) for i in (0, 3, 4, 5, 6, 7)]  # index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.memcheck_status(by_index[1]) is None
    assert metrics.gpu_memcheck[by_index[5]]["mismatched_words"] == 3
    assert metrics.gpu_memcheck[by_index[0]]["mismatched_words"] == 0
    assert metrics.gpu_memcheck_errors == {}


def test_round_process_count_ceiling():
    """Nodes whose daemons keep KFD open rest at process_count 1-2: the
    ceiling moves with max_process_count, None ignores the field, and
    in_use always skips."""
    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    for i in range(8):
        mgr.gpus[by_index[i]].process_count = 2
    mgr.gpus[by_index[4]].process_count = 3
    mgr.gpus[by_index[6]].in_use = True

    def ran(**kw):
        calls = []
        mc.memcheck_round(mgr, lambda i, n: calls.append(i) or dict(PASS, exit_code=0),
                          None, 1 << 20, **kw)
        return calls

    assert ran() == []
    assert ran(max_process_count=2) == [0, 1, 2, 3, 5, 7]
    assert ran(max_process_count=None) == [0, 1, 2, 3, 4, 5, 7]


def test_round_runner_errors_leave_health_unchanged():
    import subprocess

    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_memcheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, nbytes):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("memcheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = mc.memcheck_round(mgr, runner, metrics, 1 << 20)
    assert mgr.device_health() == before
    assert mgr.memcheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2):
        assert mgr.memcheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_memcheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3)}
    assert set(metrics.gpu_memcheck) == {by_index[i] for i in (4, 5, 6, 7)}


# -- metrics -------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_memcheck("GPU-a", 2, 5123.5, 1700000000.0)
        m.inc_memcheck_error("GPU-a")
        m.inc_memcheck_error("GPU-a")
        assert m.gpu_memcheck["GPU-a"] == {
            "mismatched_words": 2, "gbps": 5123.5, "timestamp": 1700000000.0}
        assert m.gpu_memcheck_errors["GPU-a"] == 2
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_memcheck_mismatched_words", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_memcheck_gbps", lab) == 5123.5
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_memcheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_memcheck_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert b"ECC/vanished/memcheck" in generate_latest(reg)
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ---------------------------------------------------------------------

def test_amddevs_fake_memcheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--memcheck"]) == 2
    cap = capsys.readouterr()
    assert "--memcheck needs real GPUs" in cap.err
    assert cap.out == ""


def test_agent_oneshot_accepts_memcheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "a.sock")]) == 0
    assert agent.main(base + ["--socket", str(sock_dir / "b.sock"),
                              "--memcheck-interval", "600",
                              "--memcheck-bytes", str(64 << 20)]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 2


def test_memcheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    import json

    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert mc.main(["--device", "0", "--bytes", "1048576"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
