"""mxcheck without a GPU: the decode tables, the exactness condition the
design rests on, the numpy reference, and the plumbing (manager verdicts,
rounds over idle GPUs, metrics, agent and amddevs flags)."""

import json

import numpy as np
import pytest
import torch

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import mxcheck as mx

SEEDS = (0, 0xDEADBEEF)


# -- decode tables ----------------------------------------------------------------

@pytest.mark.parametrize("table,dtype", [
    (mx.E4M3, torch.float8_e4m3fn), (mx.E5M2, torch.float8_e5m2)])
def test_fp8_tables_match_torch(table, dtype):
    want = torch.arange(256, dtype=torch.uint8).view(dtype).float().numpy().astype(np.float64)
    got = np.array(table, dtype=np.float64)
    assert got.shape == (256,)
    finite = np.isfinite(want)
    # the NaN / Inf codes aside, value and sign of zero agree
    assert np.array_equal(got[finite], want[finite])
    assert np.array_equal(np.signbit(got[finite]), np.signbit(want[finite]))
    assert np.array_equal(np.isfinite(got), finite)
    assert int(finite.sum()) == (254 if dtype is torch.float8_e4m3fn else 248)


def test_e2m1_table_and_e8m0():
    assert list(mx.E2M1) == [0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6]
    assert np.signbit(mx.E2M1[8]) and not np.signbit(mx.E2M1[0])
    assert mx.e8m0(127) == 1
    assert [mx.e8m0(b) for b in (126, 128, 129, 130)] == [0.5, 2, 4, 8]
    assert mx.e8m0(0) == 2.0 ** -127 and np.isnan(mx.e8m0(255))
    with pytest.raises(ValueError):
        mx.e8m0(256)


def test_masked_fp8_codes_are_normal_numbers():
    """Every raw byte maps to a normal, finite, non-zero value, and the
    maps reach every sign and mantissa at four exponents."""
    raw = np.arange(256)
    for table, code, man_bits, bias in ((mx.E4M3, mx.e4m3_code, 3, 7),
                                        (mx.E5M2, mx.e5m2_code, 2, 15)):
        codes = code(raw)
        assert codes.min() >= 0 and codes.max() <= 255
        exp = (codes >> man_bits) & ((1 << (7 - man_bits)) - 1)
        assert set(exp.tolist()) == {bias, bias + 1, bias + 2, bias + 3}  # 2^0..2^3
        vals = np.array(table)[codes]
        assert np.isfinite(vals).all() and (vals != 0).all()
        smallest_normal = 2.0 ** (1 - bias)
        assert (np.abs(vals) >= smallest_normal).all()
        assert len(set(codes.tolist())) == 2 * (1 << man_bits) * 4
        assert np.array_equal(codes & 0x80, raw & 0x80)
        assert np.array_equal(codes & ((1 << man_bits) - 1), raw & ((1 << man_bits) - 1))
    a = np.array(mx.E4M3)[mx.e4m3_code(raw)] * 8
    b = np.array(mx.E5M2)[mx.e5m2_code(raw)] * 4
    assert np.array_equal(a, np.round(a)) and np.abs(a).max() == 120
    assert np.array_equal(b, np.round(b)) and np.abs(b).max() == 56


# -- exactness ---------------------------------------------------------------------

@pytest.mark.parametrize("seed", SEEDS)
def test_partial_sums_are_exact_in_the_accumulator(seed):
    """Sum |a||b| per tile element, in the stage's unit, bounds every
    partial sum in any order: below 2**24 it is exact in f32, below 2**53
    in f64.  The whole design rests on this."""
    r = np.arange(64, dtype=np.uint32)
    for stage, limit in ((0, 2 ** 24), (1, 2 ** 24), (2, 2 ** 24), (3, 2 ** 53)):
        a, bt = mx.operands(seed, stage, r)
        a, bt = a.astype(np.int64), bt.astype(np.int64)
        worst = int(np.matmul(np.abs(a), np.abs(bt).transpose(0, 2, 1)).max())
        print(f"seed {seed:#x} stage {mx.STAGES[stage]}: max sum|a||b| = 2**{np.log2(worst):.2f}")
        assert 0 < worst < limit
    # the bounds the stage definitions quote
    assert 128 * 1024 * 16 == 2 ** 21 and 128 * 120 * 56 < 2 ** 20
    assert 256 * 144 * 64 < 2 ** 22 and 32 * 2 ** 23 * 2 ** 23 < 2 ** 52


def test_operands_cover_their_formats():
    r = np.arange(8, dtype=np.uint32)
    a, bt = mx.operands(0, 0, r)
    assert a.min() == -1024 and a.max() == 1023 and bt.min() == -16 and bt.max() == 15
    a, bt = mx.operands(0, 1, r)
    assert len(np.unique(a)) == 64 and len(np.unique(bt)) == 32  # sign x mantissa x 4 exponents
    a, bt = mx.operands(0, 2, r)
    # fifteen distinct e2m1 values (+-0 coincide) at four scales
    assert set(np.unique(np.abs(a))) == {0, 1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 48, 64, 96}
    sa, sb = mx.block_scales(0, 0)
    assert sa.shape == sb.shape == (32, 8) and sa.dtype == np.uint8
    assert set(np.unique(sa)) == set(np.unique(sb)) == {127, 128, 129, 130}
    assert not np.array_equal(sa, sb) and len({tuple(row) for row in sa}) > 16
    a, bt = mx.operands(0, 3, r)
    assert -2 ** 23 <= a.min() < -2 ** 22 and 2 ** 22 < a.max() < 2 ** 23


# -- reference against a plain Python definition ---------------------------------------

def _fmix(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _word(seed, stage, r, idx):
    base = _fmix(seed ^ (((4 + stage + 1) * 0x9E3779B9) & 0xFFFFFFFF)
                 ^ ((r * 0x7F4A7C15) & 0xFFFFFFFF))
    return _fmix(base + idx)


def _sext(x, bits):
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def _element(seed, stage, r, i, j):
    """C[i][j] of a stage by the docstring's formulas, a Python loop over
    k, as an exact int in the stage's unit."""
    from fractions import Fraction

    total = Fraction(0)
    if stage == 0:
        for k in range(128):
            a = _sext(_word(seed, 0, r, 64 * i + k // 2) >> (16 * (k % 2)), 11)
            b = _sext(_word(seed, 0, r, 2048 + 64 * j + k // 2) >> (16 * (k % 2)), 5)
            total += a * b
    elif stage == 1:
        for k in range(128):
            x = (_word(seed, 1, r, 32 * i + k // 4) >> (8 * (k % 4))) & 0xFF
            y = (_word(seed, 1, r, 1024 + 32 * j + k // 4) >> (8 * (k % 4))) & 0xFF
            a = mx.E4M3[(x & 0x87) | ((7 + ((x >> 3) & 3)) << 3)]
            b = mx.E5M2[(y & 0x83) | ((15 + ((y >> 2) & 3)) << 2)]
            total += Fraction(a) * Fraction(b)
    elif stage == 2:
        for k in range(256):
            a = mx.E2M1[(_word(seed, 2, r, 32 * i + k // 8) >> (4 * (k % 8))) & 15]
            b = mx.E2M1[(_word(seed, 2, r, 1024 + 32 * j + k // 8) >> (4 * (k % 8))) & 15]
            sa = 127 + ((_word(seed, 2, r, 2048 + i) >> (2 * (k // 32))) & 3)
            sb = 127 + ((_word(seed, 2, r, 2080 + j) >> (2 * (k // 32))) & 3)
            total += Fraction(a) * Fraction(mx.e8m0(sa)) * Fraction(b) * Fraction(mx.e8m0(sb))
    else:
        for k in range(32):
            total += (_sext(_word(seed, 3, r, 32 * i + k), 24)
                      * _sext(_word(seed, 3, r, 512 + 32 * j + k), 24))
    total *= mx.UNITS[stage]
    assert total.denominator == 1
    return int(total)


@pytest.mark.parametrize("stage,r,i,j", [(0, 1, 5, 30), (1, 2, 31, 0), (2, 3, 17, 9), (3, 1, 15, 2)])
def test_matmul_tile_agrees_with_a_python_loop(stage, r, i, j):
    seed = 0xDEADBEEF
    tile = mx.matmul_tile(seed, stage, r)
    n = mx.TILE_DIMS[stage]
    assert tile.shape == (n, n) and tile.dtype == np.int64
    assert int(tile[i, j]) == _element(seed, stage, r, i, j)
    assert int(tile[j % n, i % n]) == _element(seed, stage, r, j % n, i % n)
    assert tile[i, j] != tile[j % n, i % n]  # the pair tells a transpose apart
    with pytest.raises(ValueError):
        mx.matmul_tile(seed, 4, 0)


def test_block_scales_are_what_operands_applies():
    sa, sb = mx.block_scales(7, 2)
    a, bt = mx.operands(7, 2, np.array([2], dtype=np.uint32))
    for i, blk in ((0, 0), (13, 5), (31, 7)):
        for arr, sc in ((a, sa), (bt, sb)):
            vals = np.abs(arr[0, i, 32 * blk:32 * blk + 32])
            scale = mx.e8m0(int(sc[i, blk]))  # e2m1 0.5 scaled, in units of 1/2
            assert np.array_equal(vals % scale, np.zeros(32))
            assert scale <= vals.max() <= 12 * scale


def _digest_of_tiles(seed, r):
    out = []
    for s in range(4):
        c = mx.matmul_tile(seed, s, r)
        n = mx.TILE_DIMS[s]
        d = 0
        for i in range(n):
            for j in range(n):
                v = int(c[i, j]) & 0xFFFFFFFFFFFFFFFF
                if s == 3:
                    d += _fmix((v & 0xFFFFFFFF) + (16 * i + j + 1) * 0x9E3779B9)
                    d += _fmix((v >> 32) + (256 + 16 * i + j + 1) * 0x9E3779B9)
                else:
                    d += _fmix((v & 0xFFFFFFFF) + (32 * i + j + 1) * 0x9E3779B9)
        out.append(d & 0xFFFFFFFF)
    return out


# -- reference_digests --------------------------------------------------------------------

def test_reference_digests_shape_determinism_seeds_and_zero_rounds():
    a = mx.reference_digests(0, 5)
    assert a.shape == (5, 4) and a.dtype == np.uint32
    assert np.array_equal(a, mx.reference_digests(0, 5))
    b = mx.reference_digests(0xDEADBEEF, 5)
    assert (a != b).all()
    # prefix-stable across the batch size, and rounds differ from each other
    big = mx.reference_digests(0, 131)
    assert np.array_equal(big[:5], a) and len({tuple(x) for x in big}) == 131
    for s in range(4):
        assert len(set(big[:, s].tolist())) == 131
    z = mx.reference_digests(0, 0)
    assert z.shape == (0, 4) and z.dtype == np.uint32
    with pytest.raises(ValueError):
        mx.reference_digests(0, -1)
    assert mx.STAGES == ("mfma_f16", "mfma_fp8", "mfma_mxfp4", "mfma_f64")


def test_reference_digests_fold_the_tiles():
    ref = mx.reference_digests(0xDEADBEEF, 130)
    for r in (0, 129):
        assert ref[r].tolist() == _digest_of_tiles(0xDEADBEEF, r)


@pytest.mark.parametrize("seed,r", [(0, 0), (0xDEADBEEF, 1)])
def test_fold_tile_of_the_exact_product_is_the_reference_digest(seed, r):
    ref = mx.reference_digests(seed, r + 1)
    for stage in range(4):
        tile = mx.matmul_tile(seed, stage, r)
        assert int(mx.fold_tile(stage, tile)) == int(ref[r, stage])
        # leading axes are kept
        assert mx.fold_tile(stage, np.stack([tile, tile])).tolist() == [int(ref[r, stage])] * 2
    with pytest.raises(ValueError):
        mx.fold_tile(4, np.zeros((32, 32), dtype=np.int64))
    with pytest.raises(ValueError):
        mx.fold_tile(3, np.zeros((32, 32), dtype=np.int64))


def test_inputs_differ_from_cuchecks():
    from kubegpu_amd.probe import cucheck as cc

    r = np.array([0], dtype=np.uint32)
    for s in range(4):
        assert not np.array_equal(mx._words(0, s, r, 0, 8), cc._words(0, s, r, 0, 8))
    assert np.array_equal(mx._words(0, 0, r, 0, 8), cc._words(0, 4, r, 0, 8))


def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = mx.MxcheckResult(ok=False, rounds=3, waves=48, mismatches=1, first_bad_round=1,
                           bad_stages=["mfma_mxfp4"], records=[{"wave": 37}],
                           cus_covered=3, cu_count=256, bad_cus=["0/1/0/3"],
                           elapsed_s=0.5, mfma_f64_tflops=1.5, waves_on=[0] * 1024)
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"mfma_f16_tflops", "mfma_fp8_tflops", "mfma_mxfp4_tflops",
            "mfma_f64_tflops"} <= set(d)
    assert "mfma_i8_tops" not in d and "mfma_bf16_tflops" not in d
    assert mx.DEFAULT_ROUNDS % 1024 == 0 and 1024 <= mx.DEFAULT_ROUNDS <= 65536
    assert probe.MxcheckResult is mx.MxcheckResult
    assert probe.mxcheck_round is mx.mxcheck_round
    assert probe.run_mxcheck_subprocess is mx.run_mxcheck_subprocess
    assert probe.wave_tile is mx.wave_tile


# -- manager verdicts ------------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


FAIL = {"ok": False, "mismatches": 4, "first_bad_round": 1, "bad_stages": ["mfma_mxfp4"],
        "bad_cus": ["3/1/0/7"], "cus_covered": 256, "cu_count": 256, "rounds": 8}
PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.mxcheck_status(uuid) is None

    assert mgr.record_mxcheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.mxcheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.cucheck_status(uuid) is None  # separate stores
    assert len(lines) == 1
    assert uuid in lines[0] and "3/1/0/7" in lines[0] and "mfma_mxfp4" in lines[0]

    assert mgr.record_mxcheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    assert _node_info(mgr).allocatable == base.allocatable
    mgr.record_mxcheck(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_mxcheck(uuid) is True
    assert mgr.clear_mxcheck(uuid) is False
    assert mgr.mxcheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough
    mgr.record_mxcheck(uuid, FAIL)
    mgr.record_cucheck(uuid, dict(PASS))
    assert mgr.device_health()[uuid] is False
    mgr.record_mxcheck(uuid, PASS)
    mgr.record_cucheck(uuid, dict(FAIL, bad_stages=["valu"]))
    assert mgr.device_health()[uuid] is False
    mgr.clear_cucheck(uuid)
    assert mgr.device_health()[uuid] is True

    with pytest.raises(KeyError):
        mgr.record_mxcheck("GPU-does-not-exist", FAIL)
    assert set(mgr.mxcheck) == {uuid}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_mxcheck(uuid, FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.mxcheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.mxcheck_status(uuid) is None


# -- mxcheck_round ---------------------------------------------------------------------

def test_round_pass_mismatch_and_idle_selection():
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
    out = mx.mxcheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.mxcheck_status(by_index[1]) is None
    assert mgr.cucheck == {}
    assert metrics.gpu_mxcheck[by_index[5]]["mismatches"] == 4
    assert metrics.gpu_mxcheck[by_index[0]]["mismatches"] == 0
    assert metrics.gpu_mxcheck[by_index[0]]["cus_covered"] == 256
    assert metrics.gpu_mxcheck_errors == {} and metrics.gpu_cucheck == {}

    calls.clear()
    mx.mxcheck_round(mgr, runner, None, rounds=8, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_runner_errors_and_a_gpu_that_vanishes():
    import subprocess

    from kubegpu_amd.metrics import Metrics

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_mxcheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, rounds):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("mxcheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        if index == 4:
            return "not a dict"
        if index == 7:  # gone while its child ran
            with mgr._lock:
                del mgr.gpus[by_index[7]]
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = mx.mxcheck_round(mgr, runner, metrics, rounds=8)
    after = mgr.device_health()
    assert by_index[7] not in after
    assert after == {u: h for u, h in before.items() if u != by_index[7]}
    assert mgr.mxcheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2, 4):
        assert mgr.mxcheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_mxcheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3, 4)}
    assert set(metrics.gpu_mxcheck) == {by_index[i] for i in (5, 6)}
    assert by_index[7] not in out and by_index[7] not in mgr.mxcheck


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_mxcheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_mxcheck_error("GPU-a")
        m.inc_mxcheck_error("GPU-a")
        assert m.gpu_mxcheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_mxcheck_errors["GPU-a"] == 2
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_mxcheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_mxcheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_mxcheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_mxcheck_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert b"mxcheck)" in generate_latest(reg)  # the health gauge's help text
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_mxcheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--mxcheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--mxcheck needs real GPUs" in cap.err
    assert cap.out == ""


def test_amddevs_health_shows_the_verdict(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["mxcheck"] is None for r in rows.values())


def test_agent_oneshot_accepts_mxcheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--mxcheck-interval", "600", "--mxcheck-rounds", "64",
                              "--mxcheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_mxcheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert mx.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
