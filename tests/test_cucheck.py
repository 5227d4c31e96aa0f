"""Compute-unit integrity probe — everything that needs no GPU: the
numpy workload definition, the manager's verdict handling, the round
driver with fake runners, metrics, CLI and agent flags."""

import numpy as np
import pytest

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import cucheck as cc
from kubegpu_amd.probe import reference_digests

# reference_digests(seed, rounds=2, lds_dwords=2560), from a numpy
# prototype cross-checked against a scalar Python version
PINS = {
    0: [[0xD5CD4F24, 0x27F48458, 0x3B6D9D95, 0xDAC55885],
        [0xDEE1CB01, 0xAE68D96C, 0xB9CAB613, 0xA08D1C32]],
    0xDEADBEEF: [[0xA058AEED, 0x2DEFC3CC, 0x595B8FB3, 0x15E5DAD9],
                 [0xD5DC2A24, 0x064B40BC, 0xA3912499, 0xDE806ADD]],
}


# -- reference_digests ---------------------------------------------------------

@pytest.mark.parametrize("seed", sorted(PINS))
def test_reference_pins(seed):
    d = reference_digests(seed, 2, lds_dwords=2560)
    assert d.dtype == np.uint32 and d.shape == (2, 4)
    assert d.tolist() == PINS[seed]
    assert np.array_equal(d, reference_digests(seed, 2))  # 2560 is the default


def test_stage_names_and_tile_pin():
    assert cc.STAGES == ("mfma_i8", "mfma_bf16", "valu", "lds")
    c = cc.matmul_tile(0, 0, 1)
    assert c.shape == (32, 32) and int(c[3][5]) == 58999
    assert np.abs(c).max() <= 1 << 22
    assert np.abs(cc.matmul_tile(0, 1, 1)).max() < 1 << 24  # exact in f32
    with pytest.raises(ValueError):
        cc.matmul_tile(0, 2, 0)


def _fmix(h):
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _scalar_digests(seed, r, lds_dwords):
    """The issue's definition in plain Python integers, one round."""
    M = 0xFFFFFFFF

    def base(stage):
        return _fmix(seed ^ (((stage + 1) * 0x9E3779B9) & M) ^ ((r * 0x7F4A7C15) & M))

    def word(stage, idx):
        return _fmix((base(stage) + idx) & M)

    def i8(w, b):
        v = (w >> (8 * b)) & 0xFF
        return v - 256 if v >= 128 else v

    def salt(n):
        return ((n + 1) * 0x9E3779B9) & M

    out = []
    for stage, wpr in ((0, 64), (1, 32)):
        k_n = 4 * wpr
        a = [[i8(word(stage, wpr * i + k // 4), k % 4) for k in range(k_n)] for i in range(32)]
        b = [[i8(word(stage, 32 * wpr + wpr * j + k // 4), k % 4) for k in range(k_n)]
             for j in range(32)]
        d = 0
        for i in range(32):
            for j in range(32):
                c = sum(x * y for x, y in zip(a[i], b[j]))
                d += _fmix(((c & M) + salt(32 * i + j)) & M)
        out.append(d & M)
    d = 0
    for lane in range(64):
        x = word(2, lane)
        for _ in range(32):
            x = (x * 0x9E3779B1 + (((x << 13) | (x >> 19)) & M)) & M
            x ^= (x * 0x85EBCA6B) >> 32
            x = (x + (x & 0xFFF) * ((x >> 12) & 0xFFF) + (x >> 24)) & M
        d += _fmix((x + lane) & M)
    out.append(d & M)
    d = 0
    for i in range(lds_dwords):
        v = word(3, i)
        d += _fmix((v + salt(i)) & M) + _fmix(((v ^ M) + salt(i)) & M)
    out.append(d & M)
    return out


def test_reference_agrees_with_scalar_definition():
    for seed, r, lds_dwords in ((0, 0, 64), (0xDEADBEEF, 3, 64), (7, 130, 128)):
        want = _scalar_digests(seed, r, lds_dwords)
        got = reference_digests(seed, r + 1, lds_dwords=lds_dwords)[r]
        assert got.tolist() == want, (seed, r)


def test_reference_is_prefix_stable():
    five = reference_digests(9, 5)
    assert np.array_equal(five[:2], reference_digests(9, 2))
    # also across the internal batch boundary
    many = reference_digests(9, cc._REF_CHUNK + 3, lds_dwords=64)
    assert np.array_equal(many[:5], reference_digests(9, 5, lds_dwords=64))
    assert np.array_equal(many[-1], _scalar_digests(9, cc._REF_CHUNK + 2, 64))
    assert reference_digests(9, 0).shape == (0, 4)


def test_every_stage_depends_on_seed_and_round():
    a = reference_digests(0, 3)
    b = reference_digests(1, 3)
    for stage in range(4):
        assert len({int(x) for x in a[:, stage]}) == 3, stage  # rounds differ
        assert all(a[r, stage] != b[r, stage] for r in range(3)), stage  # seeds differ


def test_lds_dwords_changes_only_the_lds_column():
    a = reference_digests(5, 3, lds_dwords=2560)
    b = reference_digests(5, 3, lds_dwords=64)
    assert np.array_equal(a[:, :3], b[:, :3])
    assert all(a[r, 3] != b[r, 3] for r in range(3))


# -- reference_values and fold_values ---------------------------------------------

TRIPLES = ((0, 0, 64), (0xDEADBEEF, 3, 64), (7, 130, 128))


def test_fold_of_reference_values_is_the_reference_digest():
    for seed, r, n in TRIPLES:
        want = reference_digests(seed, r + 1, lds_dwords=n)[r]
        for stage in range(4):
            got = cc.fold_values(stage, cc.reference_values(seed, stage, r, n))
            assert got.dtype == np.uint32 and got.shape == ()
            assert int(got) == int(want[stage]), (seed, r, stage)


def test_valu_trace_agrees_with_plain_integers():
    M = 0xFFFFFFFF
    for seed, r, _ in TRIPLES + ((0xFFFFFFFF, 65535, 64),):
        trace = cc.reference_values(seed, 2, r)
        base = _fmix(seed ^ ((3 * 0x9E3779B9) & M) ^ ((r * 0x7F4A7C15) & M))
        for lane in (0, 63):
            x = _fmix((base + lane) & M)
            for it in range(32):
                x = (x * 0x9E3779B1 + (((x << 13) | (x >> 19)) & M)) & M
                x ^= (x * 0x85EBCA6B) >> 32
                x = (x + (x & 0xFFF) * ((x >> 12) & 0xFFF) + (x >> 24)) & M
                assert int(trace[it, lane]) == x, (seed, r, lane, it)
        # The FMA's operands are those of x before the last line of an
        # iteration, which the trace does not hold; redo the first two lines
        # from the row above (the start words for iteration 0).
        before = np.vstack([cc._words(seed, 2, np.array([r], dtype=np.uint32), 0, 64),
                            trace[:-1]]).astype(np.uint64)
        y = (before * 0x9E3779B1 + (((before << 13) | (before >> 19)) & M)) & M
        y ^= (y * 0x85EBCA6B) >> 32
        fma = (y & 0xFFF) * ((y >> 12) & 0xFFF) + (y >> 24)
        assert int(fma.max()) <= 4095 * 4095 + 255 < 2 ** 24  # exact in f32
        assert np.array_equal((y + fma) & M, trace)


@pytest.mark.parametrize("stage", range(4))
def test_fold_notices_any_single_bit_in_any_element(stage):
    """fmix32 is a bijection, so one flipped bit in one folded element
    changes that element's term and with it the sum — always."""
    ref = cc.reference_values(0xDEADBEEF, stage, 1, 64)
    clean = cc.fold_values(stage, ref)
    rows, cols = ref.shape
    lo = rows - 1 if stage == 2 else 0  # the valu digest folds the last row
    n = (rows - lo) * cols
    i, j = np.divmod(np.arange(n), cols)
    for bit in range(32):
        faulty = np.broadcast_to(ref, (n, rows, cols)).copy()
        faulty[np.arange(n), lo + i, j] ^= ref.dtype.type(1 << bit)
        got = cc.fold_values(stage, faulty)
        assert got.shape == (n,)
        assert (got != clean).all(), (bit, np.argwhere(got == clean)[:4].tolist())
    if stage == 2:  # and only the last row
        ref[:-1] ^= np.uint32(1)
        assert cc.fold_values(2, ref) == clean


def test_value_shapes_dtypes_and_bad_stage():
    for stage, shape, dtype in ((0, (32, 32), np.int64), (1, (32, 32), np.int64),
                                (2, (32, 64), np.uint32), (3, (2, 2560), np.uint32)):
        v = cc.reference_values(5, stage, 2)
        assert v.shape == shape and v.dtype == dtype, stage
    v = cc.reference_values(5, 3, 2, 64)
    assert v.shape == (2, 64) and np.array_equal(v[1], ~v[0])
    assert np.array_equal(cc.reference_values(5, 0, 2), cc.matmul_tile(5, 0, 2))
    for stage in (-1, 4):
        with pytest.raises(ValueError):
            cc.reference_values(0, stage, 0)
        with pytest.raises(ValueError):
            cc.fold_values(stage, np.zeros((32, 32), dtype=np.int64))
        with pytest.raises(ValueError):
            cc.wave_values(0, stage, 0)  # refused before the extension is loaded
    for bad_r in (-1, 65536):
        with pytest.raises(ValueError):
            cc.reference_values(0, 2, bad_r)
    with pytest.raises(ValueError):
        cc.fold_values(2, np.zeros((32, 32), dtype=np.uint32))
    with pytest.raises(ValueError):
        cc.fold_values(3, np.zeros((64,), dtype=np.uint32))


def test_lazy_reexports():
    from kubegpu_amd import probe

    for name in ("CucheckResult", "cucheck_round", "reference_digests",
                 "run_cucheck_subprocess", "wave_digests"):
        assert getattr(probe, name) is getattr(cc, name)
    # the two probes' children share one lock
    from kubegpu_amd.probe import memcheck as mc

    assert cc._child_lock is mc._child_lock


def test_result_to_dict_round_trips_json():
    import json

    res = cc.CucheckResult(ok=False, rounds=3, waves=48, mismatches=1, first_bad_round=1,
                           bad_stages=["valu"], records=[cc._decode_record(
                               (37, (5 << 16) | (2 << 13) | (1 << 12) | (9 << 8) | (3 << 4) | 7,
                                1, 2, 10, 11))],
                           cus_covered=3, cu_count=256, bad_cus=["5/2/1/9"], elapsed_s=0.5)
    d = json.loads(json.dumps(res.to_dict()))
    assert d["records"] == [{"wave": 37, "block": 2, "xcc": 5, "se": 2, "sh": 1, "cu": 9,
                             "simd": 3, "round": 1, "stage": "valu",
                             "expected": 10, "got": 11}]
    assert d["bad_cus"] == ["5/2/1/9"] and d["ok"] is False
    assert set(d) == {"ok", "rounds", "waves", "mismatches", "first_bad_round",
                      "bad_stages", "records", "records_dropped", "cus_covered",
                      "cu_count", "bad_cus", "elapsed_s", "mfma_i8_tops",
                      "mfma_bf16_tflops"}
    assert cc.cu_key(5, 2, 1, 9) == (5 << 7) | (2 << 5) | (1 << 4) | 9 < 1024


# -- manager verdicts ------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


FAIL = {"ok": False, "mismatches": 4, "first_bad_round": 1, "bad_stages": ["mfma_i8"],
        "bad_cus": ["3/1/0/7"], "cus_covered": 256, "cu_count": 256, "rounds": 8}
PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}
MEM_FAIL = {"ok": False, "mismatched_words": 3, "first_bad_offset": 64, "bad_bits_mask": 0x10}


def test_failed_verdict_drops_health_and_allocatable():
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.cucheck_status(uuid) is None

    assert mgr.record_cucheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.cucheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.memcheck_status(uuid) is None  # separate stores

    # a later passing verdict restores the GPU, and so does clear_cucheck
    assert mgr.record_cucheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True
    assert _node_info(mgr).allocatable == base.allocatable
    mgr.record_cucheck(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_cucheck(uuid) is True
    assert mgr.clear_cucheck(uuid) is False
    assert mgr.cucheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True


def test_failure_log_names_cus_and_stages(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[0]
    mgr.record_cucheck(uuid, PASS)
    assert lines == []
    mgr.record_cucheck(uuid, FAIL)
    assert len(lines) == 1
    assert uuid in lines[0] and "3/1/0/7" in lines[0] and "mfma_i8" in lines[0]


def test_failed_memcheck_plus_passing_cucheck_is_unhealthy():
    mgr = _mgr()
    uuid = sorted(mgr.gpus)[1]
    mgr.record_memcheck(uuid, MEM_FAIL)
    mgr.record_cucheck(uuid, PASS)
    assert mgr.device_health()[uuid] is False
    mgr.clear_memcheck(uuid)
    assert mgr.device_health()[uuid] is True
    # and the other way round
    mgr.record_cucheck(uuid, FAIL)
    mgr.record_memcheck(uuid, {"ok": True, "mismatched_words": 0})
    assert mgr.device_health()[uuid] is False


def test_unknown_uuid_is_rejected():
    mgr = _mgr()
    with pytest.raises(KeyError):
        mgr.record_cucheck("GPU-does-not-exist", FAIL)
    assert mgr.cucheck == {}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_cucheck(uuid, FAIL)
    before = mgr.gpus[uuid]
    mgr.update_gpu_info(force=True)
    assert mgr.gpus[uuid] is not before  # GpuInfo was replaced...
    assert mgr.device_health()[uuid] is False  # ...the verdict was not

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.cucheck_status(uuid) is not None
    assert mgr.device_health()[uuid] is False
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.cucheck_status(uuid) is None


# -- cucheck_round -----------------------------------------------------------------

def test_round_skips_busy_gpus_and_records_failures():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    calls = []

    def runner(index, rounds):
        calls.append((index, rounds))
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = cc.cucheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.cucheck_status(by_index[1]) is None
    assert metrics.gpu_cucheck[by_index[5]]["mismatches"] == 4
    assert metrics.gpu_cucheck[by_index[0]]["mismatches"] == 0
    assert metrics.gpu_cucheck[by_index[0]]["cus_covered"] == 256
    assert metrics.gpu_cucheck_errors == {}

    # the ceiling moves with max_process_count; None ignores the field
    calls.clear()
    cc.cucheck_round(mgr, runner, None, rounds=8, max_process_count=4)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]
    calls.clear()
    cc.cucheck_round(mgr, runner, None, rounds=8, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_runner_errors_leave_health_unchanged():
    import subprocess

    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_cucheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, rounds):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("cucheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = cc.cucheck_round(mgr, runner, metrics, rounds=8)
    assert mgr.device_health() == before
    assert mgr.cucheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2):
        assert mgr.cucheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_cucheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3)}
    assert set(metrics.gpu_cucheck) == {by_index[i] for i in (4, 5, 6, 7)}


def test_memcheck_round_selection_unchanged_by_shared_helper():
    from kubegpu_amd.probe import memcheck as mc

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[6]].in_use = True
    mgr.gpus[by_index[4]].process_count = 3
    assert mc.idle_gpus(mgr, 0) == [(i, by_index[i]) for i in (0, 1, 2, 3, 5, 7)]
    assert mc.idle_gpus(mgr, None) == [(i, by_index[i]) for i in (0, 1, 2, 3, 4, 5, 7)]


# -- metrics -------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_cucheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_cucheck_error("GPU-a")
        m.inc_cucheck_error("GPU-a")
        assert m.gpu_cucheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_cucheck_errors["GPU-a"] == 2
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_cucheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_cucheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_cucheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_cucheck_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert b"ECC/vanished/memcheck/cucheck" in generate_latest(reg)
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ---------------------------------------------------------------------

def test_amddevs_fake_cucheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--cucheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--cucheck needs real GPUs" in cap.err
    assert cap.out == ""


def test_agent_oneshot_accepts_cucheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "c.sock"),
                              "--cucheck-interval", "600", "--cucheck-rounds", "64",
                              "--cucheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_cucheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    import json

    import torch

    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert cc.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
