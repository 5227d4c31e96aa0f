"""GPU tests — run on a real MI355X via gpurun (`pytest -m gpu`)."""

import json
import os
import subprocess

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(REPO, "kubegpu_amd", "csrc", "bin")


@pytest.fixture(scope="module")
def real_inventory():
    from kubegpu_amd.discovery import default_backend

    return default_backend().get_devices()


def test_cuda_available():
    assert torch.cuda.is_available()


def test_amdsmiinfo_binary_json():
    out = subprocess.run(
        [os.path.join(BIN, "amdsmiinfo"), "json"],
        capture_output=True,
        timeout=60,
        check=True,
    )
    from kubegpu_amd.discovery import GpusInfo

    info = GpusInfo.from_json(out.stdout.decode())
    assert len(info.devices) >= 1
    g = info.devices[0]
    assert g.uuid
    assert g.gfx_target == "gfx950"
    # MI355X: 288 GB HBM3E
    assert g.memory.vram_total_bytes > 200 * 1024**3
    assert g.render_path.startswith("/dev/dri/renderD")
    assert os.path.exists(g.render_path)
    # ECC totals present in the payload (health source); a freshly
    # provisioned box should have no uncorrectable errors
    raw = json.loads(out.stdout.decode())
    assert "ecc_uncorrectable" in raw["devices"][0]
    assert g.ecc_uncorrectable == 0 and g.healthy


def test_amdsmiinfo_human_mode():
    out = subprocess.run(
        [os.path.join(BIN, "amdsmiinfo")], capture_output=True, timeout=60, check=True
    )
    assert b"GPU 0:" in out.stdout


def test_real_discovery_and_manager(real_inventory):
    from kubegpu_amd.api.types import NodeInfo
    from kubegpu_amd.deviceplugin import create_device_plugin
    from kubegpu_amd.discovery import default_backend
    from kubegpu_amd.plugintypes import RESOURCE_GPU

    mgr = create_device_plugin(default_backend())
    mgr.start()
    ni = NodeInfo(name="real")
    mgr.update_node_info(ni)
    n = ni.kube_alloc[RESOURCE_GPU]
    assert n == len(real_inventory.devices) >= 1
    cards = [k for k in ni.allocatable if k.endswith("/cards")]
    assert len(cards) == n
    assert all("/gpugrp1/" in c and "/gpugrp0/" in c for c in cards)


def test_schedule_and_allocate_real():
    """Config 2: 1-GPU pod on the real node, /dev injection correct."""
    from kubegpu_amd.api.types import ContainerInfo, PodInfo
    from kubegpu_amd.core import Cluster
    from kubegpu_amd.deviceplugin import create_device_plugin
    from kubegpu_amd.discovery import default_backend
    from kubegpu_amd.plugintypes import RESOURCE_GPU

    mgr = create_device_plugin(default_backend())
    cluster = Cluster()
    cluster.add_node_from_manager("real", mgr)
    pod = PodInfo(
        name="p1",
        running_containers={"c": ContainerInfo(kube_requests={RESOURCE_GPU: 1})},
    )
    res = cluster.schedule(pod)
    assert len(res.uuids) == 1
    mounts, devices, envs = cluster.container_allocate(pod, "c")
    assert "/dev/kfd" in devices and os.path.exists("/dev/kfd")
    renders = [d for d in devices if "renderD" in d]
    assert len(renders) == 1 and os.path.exists(renders[0])
    assert envs["ROCR_VISIBLE_DEVICES"] == res.uuids[0]


def test_gpuprobe_copy_numerics():
    """HIP copy kernel vs plain PyTorch fp32 reference."""
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    torch.manual_seed(0)
    # (1 << 20) + 3 floats: nbytes % 16 == 12, the byte-kernel path
    for n in (1 << 10, (1 << 20) + 4, (1 << 20) + 3, 1 << 24):
        src = torch.randn(n, dtype=torch.float32, device="cuda")
        dst = torch.full_like(src, -1.0)
        ext.copy(dst, src)
        torch.cuda.synchronize()
        assert torch.equal(dst, src)


def test_gpuprobe_bandwidth_sanity():
    from kubegpu_amd.probe.bandwidth import d2d_copy_bw_gbps

    bw = d2d_copy_bw_gbps(1 << 30, iters=10)
    # MI355X HBM3E: 8 TB/s peak, ~6.3 TB/s achievable; require a
    # conservative floor that still proves we're on HBM, not PCIe.
    assert bw > 2000.0, f"copy bandwidth {bw:.0f} GB/s is far below HBM class"


def test_rcclprobe_binary():
    out = subprocess.run(
        [
            os.path.join(BIN, "rcclprobe"),
            "--ndev", "1", "--bytes", str(64 << 20), "--iters", "5", "--warmup", "2",
        ],
        capture_output=True,
        timeout=300,
        check=True,
    )
    rec = json.loads(out.stdout.decode().strip().splitlines()[-1])
    assert rec["ndev"] == 1
    assert rec["busbw_gbps"] > 0
    # every element of recv and send was verified on the GPU
    assert rec["check"] == "pass"
    assert rec["mismatches"] == 0
    assert rec["checked_elements"] == 2 * (64 << 20) // 2


def test_graft_smoke():
    import __graft_entry__ as g

    g.smoke()


def test_probe_with_link_utilization_real():
    """Counter-bracketed probe on the real box: structure is returned
    even when the 1-GPU probe moves no xGMI traffic."""
    from kubegpu_amd.probe import probe_with_link_utilization, run_rccl_probe

    out, links = probe_with_link_utilization(
        run_rccl_probe, ndev=1, nbytes=64 << 20, iters=3, warmup=1
    )
    assert out["busbw_gbps"] > 0
    assert out.get("check") == "pass"
    if links is not None:  # amdsmi counters available
        assert 0 in links


def test_amddevs_cli_plugin_mode():
    import json as _json
    import subprocess as _sp
    import sys as _sys

    res = _sp.run(
        [_sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--plugin"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, res.stderr[-1000:]
    rec = _json.loads(res.stdout)
    assert rec["kube_alloc"]["amd.com/gpu"] >= 1


def test_amddevs_cli_schedule_mode():
    import json as _json
    import subprocess as _sp
    import sys as _sys

    res = _sp.run(
        [_sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--schedule", "1"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, res.stderr[-1000:]
    rec = _json.loads(res.stdout)
    assert len(rec["gpus"]) == 1
    assert "/dev/kfd" in rec["devices"]


def test_sysfs_backend_enumerates_real_node():
    """The KFD-sysfs fallback backend (second real backend, analog of the
    reference's REST path) discovers the same GPU set as amdsmiinfo."""
    from kubegpu_amd.discovery import SysfsBackend, default_backend

    sysfs = SysfsBackend().get_devices()
    smi = default_backend().get_devices()
    assert len(sysfs.devices) == len(smi.devices) >= 1
    g = sysfs.devices[0]
    assert g.render_path.startswith("/dev/dri/renderD")
    assert g.memory.vram_total_bytes > 200 * 1024**3


def test_amdsmiinfo_process_count_field():
    """process_count present; transiently occupying the GPU from this
    process is visible is not asserted (racy) — only schema + sanity."""
    out = subprocess.run(
        [os.path.join(BIN, "amdsmiinfo"), "json"],
        capture_output=True, timeout=60, check=True,
    )
    raw = json.loads(out.stdout.decode())
    assert all("process_count" in d for d in raw["devices"])
    assert all(d["process_count"] >= 0 for d in raw["devices"])


def test_rw_bandwidth_triple():
    """Read-only / write-only / copy bandwidths are each HBM-class and
    mutually consistent (read and write each beat the copy R+W rate)."""
    from kubegpu_amd.probe.bandwidth import load_ext

    ext = load_ext(required=True)
    copy = ext.copy_bw_gbps(1 << 30, 10)
    read = ext.read_bw_gbps(1 << 30, 10)
    write = ext.write_bw_gbps(1 << 30, 10)
    assert read > 2000 and write > 2000 and copy > 2000
    # one-directional streams should each exceed half the R+W copy rate
    assert read > copy / 2 and write > copy / 2


def test_bench_record_is_pinned_and_self_describing():
    """Round-2 bench contract on hardware: the rank pins itself to the
    scheduled device before HIP init (rank_pinning), the record is
    honest about the k=1 degenerate mode (dtype/curve_point), and the
    pinned device's BDF matches what the scheduler chose."""
    import subprocess as _sp
    import sys as _sys

    res = _sp.run(
        [_sys.executable, os.path.join(REPO, "bench.py"),
         "--steps", "20", "--warmup", "5", "--pods", "50"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, res.stderr[-1500:]
    rec = json.loads(res.stdout.strip().splitlines()[-1])
    cfg = rec["config"]
    assert rec["dtype"] == "uint8"
    assert cfg["curve_point"] == "k1-degenerate-hbm"
    assert cfg["rank_pinning"] == "ROCR_VISIBLE_DEVICES"
    assert cfg["scheduled_devices"] == [cfg["pinned_device"]]
    assert cfg.get("bdf_verified") is True, cfg
    assert rec["value"] > 3000  # HBM copy sanity floor


def test_amddevs_health_shows_in_use():
    """--health surfaces the allocation lifecycle field on a real node."""
    import subprocess as _sp
    import sys as _sys

    res = _sp.run(
        [_sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--health"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, res.stderr[-1000:]
    rows = json.loads(res.stdout)
    assert rows
    for row in rows.values():
        assert row["in_use"] is False  # fresh box: nothing allocated
        assert "process_count" in row


def test_rcclprobe_across_all_gpus_when_multi():
    """Opportunistic xGMI measurement: on a multi-GPU box, bf16 ring
    all-reduce across ALL devices (librccl, xGMI transport) with the
    numerics check, plus the scheduler's prediction for the same set —
    the closed verification loop of SURVEY hard part (b).  Skips on the
    1-GPU leases every gpurun box has offered so far; the driver's
    round-end 8-GPU node turns it into a real k=8 point."""
    n = torch.cuda.device_count()
    if n < 2:
        pytest.skip(f"single-GPU box (device_count={n})")
    from kubegpu_amd.core import Cluster
    from kubegpu_amd.deviceplugin import create_device_plugin
    from kubegpu_amd.discovery import default_backend
    from kubegpu_amd.probe.rccl_probe import run_rccl_probe

    cluster = Cluster()
    mgr = create_device_plugin(default_backend())
    cluster.add_node_from_manager("local", mgr)
    st = cluster.core.nodes["local"]
    idxs = sorted(g.index for g in mgr.gpus.values())[:n]
    pred = st.scorer.ring_bw(idxs)

    rec = run_rccl_probe(devices=idxs, nbytes=256 << 20, iters=10, warmup=3,
                         timeout_s=420)
    assert rec["check"] == "pass"
    assert rec["mismatches"] == 0
    assert rec["checked_elements"] == 2 * n * (256 << 20) // 2
    assert rec["ndev"] == n
    # xGMI ring floor: well below one link (~153 GB/s) means the ring
    # fell back to host paths — the placement model would be wrong
    assert rec["busbw_gbps"] > 60, (rec, {"predicted": pred})


def test_extender_with_real_inventory():
    """Scheduler-extender webhook fed the REAL box inventory over HTTP:
    register via POST /v1/nodes/<n> with live amdsmiinfo json, then
    filter + prioritize a 1-GPU pod."""
    import urllib.request

    from kubegpu_amd.server.extender import serve

    server, core = serve(host="127.0.0.1", port=0)
    port = server.server_address[1]
    base = f"http://127.0.0.1:{port}"

    def post(path, payload):
        req = urllib.request.Request(
            base + path, data=json.dumps(payload).encode(),
            headers={"Content-Type": "application/json"}, method="POST")
        with urllib.request.urlopen(req, timeout=30) as r:
            return json.loads(r.read().decode())

    try:
        out = subprocess.run([os.path.join(BIN, "amdsmiinfo"), "json"],
                             capture_output=True, timeout=120)
        inv = json.loads(out.stdout)
        reg = post("/v1/nodes/realnode", inv)
        assert reg["registered"] == "realnode" and reg["gpus"] >= 1

        pod = {"metadata": {"name": "p"}, "spec": {"containers": [
            {"name": "c", "resources": {"limits": {"amd.com/gpu": "1"}}}]}}
        res = post("/v1/filter", {"Pod": pod, "NodeNames": ["realnode"]})
        assert res["NodeNames"] == ["realnode"], res
        pri = post("/v1/prioritize", {"Pod": pod, "NodeNames": ["realnode"]})
        assert pri[0]["Score"] == 10
    finally:
        server.shutdown()


def test_amddevs_cdi_real_device_nodes():
    """CDI spec from the real inventory: every device node it names
    exists on the box (the spec is directly consumable by containerd)."""
    import subprocess as _sp
    import sys as _sys

    res = _sp.run(
        [_sys.executable, "-m", "kubegpu_amd.cli.amddevs", "--cdi"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, res.stderr[-1000:]
    spec = json.loads(res.stdout)
    assert spec["kind"] == "amd.com/gpu"
    for n in spec["containerEdits"]["deviceNodes"]:
        assert os.path.exists(n["path"]), n
    assert spec["devices"]
    for dev in spec["devices"]:
        for n in dev["containerEdits"]["deviceNodes"]:
            assert os.path.exists(n["path"]), (dev["name"], n)
