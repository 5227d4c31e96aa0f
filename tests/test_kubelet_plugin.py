"""Kubelet device-plugin server tests: real gRPC over a unix socket,
fixture-backed manager (config 1 — the CPU-only 'kind cluster' analog)."""

import os

import grpc
import pytest

from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.server import KubeletDevicePlugin, dpapi


def _serialize(m):
    return m.SerializeToString()


@pytest.fixture
def plugin(sock_dir):
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_2hive_8gpu()))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "amdgpu.sock"))
    p.start()
    yield p
    p.stop()


@pytest.fixture
def channel(plugin):
    ch = grpc.insecure_channel(f"unix://{plugin.socket_path}")
    yield ch
    ch.close()


def _stub(channel, method, req_cls, resp_cls, streaming=False):
    path = f"/{dpapi.DEVICE_PLUGIN_SERVICE}/{method}"
    if streaming:
        return channel.unary_stream(path, request_serializer=_serialize,
                                    response_deserializer=resp_cls.FromString)
    return channel.unary_unary(path, request_serializer=_serialize,
                               response_deserializer=resp_cls.FromString)


def test_options(channel):
    opts = _stub(channel, "GetDevicePluginOptions", dpapi.Empty,
                 dpapi.DevicePluginOptions)(dpapi.Empty(), timeout=10)
    assert opts.get_preferred_allocation_available


def test_list_and_watch_first_frame(channel):
    stream = _stub(channel, "ListAndWatch", dpapi.Empty,
                   dpapi.ListAndWatchResponse, streaming=True)(
        dpapi.Empty(), timeout=10
    )
    frame = next(iter(stream))
    assert len(frame.devices) == 8
    d = frame.devices[0]
    assert d.health == dpapi.HEALTHY
    assert d.ID.startswith("GPU-mi355x-")
    assert len(d.topology.nodes) == 1


def test_preferred_allocation_same_hive(channel):
    """kubelet asks for 4 of 8 on a 2-hive node: must get one intact
    hive, never a straddling set."""
    req = dpapi.PreferredAllocationRequest(
        container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=[f"GPU-mi355x-{i:02d}" for i in range(8)],
                allocation_size=4,
            )
        ]
    )
    resp = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)(req, timeout=10)
    ids = sorted(resp.container_responses[0].deviceIDs)
    idx = [int(u.split("-")[-1]) for u in ids]
    assert idx == [0, 1, 2, 3] or idx == [4, 5, 6, 7]


def test_preferred_allocation_partial_free(channel):
    """2 of {2,3,4,5}: pick the same-hive pair (2,3) or (4,5)."""
    req = dpapi.PreferredAllocationRequest(
        container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=[f"GPU-mi355x-{i:02d}" for i in (2, 3, 4, 5)],
                allocation_size=2,
            )
        ]
    )
    resp = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)(req, timeout=10)
    idx = sorted(int(u.split("-")[-1]) for u in resp.container_responses[0].deviceIDs)
    assert idx in ([2, 3], [4, 5])


def test_allocate_device_specs(channel, plugin):
    req = dpapi.AllocateRequest(
        container_requests=[
            dpapi.ContainerAllocateRequest(
                devicesIDs=["GPU-mi355x-01", "GPU-mi355x-02"]
            )
        ]
    )
    resp = _stub(channel, "Allocate", dpapi.AllocateRequest,
                 dpapi.AllocateResponse)(req, timeout=10)
    cr = resp.container_responses[0]
    paths = [d.host_path for d in cr.devices]
    assert "/dev/kfd" in paths
    assert "/dev/dri/renderD129" in paths and "/dev/dri/renderD130" in paths
    assert cr.envs["ROCR_VISIBLE_DEVICES"] == "GPU-mi355x-01,GPU-mi355x-02"
    # v1beta1 has no deallocate RPC, so the kubelet path must NOT set a
    # flag it could never clear
    assert not plugin.manager.gpus["GPU-mi355x-01"].in_use


def test_allocate_unknown_device_rejected(channel):
    req = dpapi.AllocateRequest(
        container_requests=[
            dpapi.ContainerAllocateRequest(devicesIDs=["GPU-bogus"])
        ]
    )
    with pytest.raises(grpc.RpcError) as err:
        _stub(channel, "Allocate", dpapi.AllocateRequest,
              dpapi.AllocateResponse)(req, timeout=10)
    assert err.value.code() == grpc.StatusCode.INVALID_ARGUMENT


def test_registration_roundtrip(sock_dir):
    """Register against a fake kubelet Registration service."""
    from concurrent import futures

    received = {}

    def register(request, context):
        received["req"] = request
        return dpapi.Empty()

    handler = grpc.method_handlers_generic_handler(
        dpapi.REGISTRATION_SERVICE,
        {
            "Register": grpc.unary_unary_rpc_method_handler(
                register,
                request_deserializer=dpapi.RegisterRequest.FromString,
                response_serializer=_serialize,
            )
        },
    )
    kubelet_sock = str(sock_dir / "kubelet.sock")
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    server.add_generic_rpc_handlers((handler,))
    server.add_insecure_port(f"unix://{kubelet_sock}")
    server.start()

    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "amdgpu.sock"))
    p.start()
    p.register_with_kubelet(kubelet_socket=kubelet_sock)
    assert received["req"].resource_name == "amd.com/gpu"
    assert received["req"].version == "v1beta1"
    assert received["req"].endpoint == "amdgpu.sock"
    p.stop()
    server.stop(grace=0.5)


def test_preferred_allocation_must_include(channel):
    """must_include_deviceIDs are honoured: the chosen set contains every
    must device and completes with that device's hive-mates."""
    req = dpapi.PreferredAllocationRequest(
        container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=[f"GPU-mi355x-{i:02d}" for i in range(8)],
                must_include_deviceIDs=["GPU-mi355x-05"],
                allocation_size=2,
            )
        ]
    )
    resp = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)(req, timeout=10)
    ids = resp.container_responses[0].deviceIDs
    idx = sorted(int(u.split("-")[-1]) for u in ids)
    assert 5 in idx and len(idx) == 2
    # completion stays in hive 1 (4-7): cross-hive would be PCIe-bound
    assert all(i in (4, 5, 6, 7) for i in idx)


def test_preferred_allocation_two_musts_both_kept(channel):
    """Two must devices never collapse into one slot (the old last-slot
    overwrite bug)."""
    req = dpapi.PreferredAllocationRequest(
        container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=[f"GPU-mi355x-{i:02d}" for i in range(8)],
                must_include_deviceIDs=["GPU-mi355x-00", "GPU-mi355x-05"],
                allocation_size=4,
            )
        ]
    )
    resp = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)(req, timeout=10)
    idx = sorted(int(u.split("-")[-1])
                 for u in resp.container_responses[0].deviceIDs)
    assert len(idx) == 4 and 0 in idx and 5 in idx


def test_ecc_unhealthy_device_flagged(sock_dir):
    """A GPU with uncorrectable ECC errors is advertised UNHEALTHY;
    healthy peers stay HEALTHY."""
    from kubegpu_amd.discovery import FakeBackend, fixtures

    fix = fixtures.fixture_8x_mi355x()
    fix.devices[3].ecc_uncorrectable = 2
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "ecc.sock"))
    p.start()
    try:
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        stream = _stub(ch, "ListAndWatch", dpapi.Empty,
                       dpapi.ListAndWatchResponse, streaming=True)(
            dpapi.Empty(), timeout=10
        )
        frame = next(iter(stream))
        by_id = {d.ID: d.health for d in frame.devices}
        assert len(by_id) == 8
        assert by_id["GPU-mi355x-03"] == dpapi.UNHEALTHY
        assert by_id["GPU-mi355x-00"] == dpapi.HEALTHY
        ch.close()
    finally:
        p.stop()


def test_vanished_gpu_tombstoned_unhealthy(sock_dir):
    """A GPU that disappears between discoveries stays advertised as an
    UNHEALTHY device (tombstone) instead of silently shrinking the node."""
    from kubegpu_amd.discovery import FakeBackend, fixtures

    full = fixtures.fixture_8x_mi355x()
    backend = FakeBackend(full)
    mgr = create_device_plugin(backend)
    mgr.start()
    assert len(mgr.gpus) == 8
    shrunk = fixtures.fixture_8x_mi355x()
    gone = shrunk.devices.pop(5)
    backend.set_info(shrunk)
    mgr.update_gpu_info(force=True)
    assert len(mgr.gpus) == 7 and gone.uuid in mgr.vanished
    health = mgr.device_health()
    assert health[gone.uuid] is False
    assert sum(health.values()) == 7

    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "van.sock"))
    p.start()
    try:
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        frame = next(iter(_stub(ch, "ListAndWatch", dpapi.Empty,
                                dpapi.ListAndWatchResponse, streaming=True)(
            dpapi.Empty(), timeout=10)))
        by_id = {d.ID: d.health for d in frame.devices}
        assert len(by_id) == 8  # tombstone still advertised
        assert by_id[gone.uuid] == dpapi.UNHEALTHY
        # ...and it comes back HEALTHY when re-discovered
        backend.set_info(fixtures.fixture_8x_mi355x())
        mgr.update_gpu_info(force=True)
        assert gone.uuid not in mgr.vanished
        assert mgr.device_health()[gone.uuid] is True
        ch.close()
    finally:
        p.stop()


def test_register_with_fake_kubelet(sock_dir):
    """register_with_kubelet posts a well-formed RegisterRequest to the
    kubelet Registration service (verified against a fake kubelet)."""
    import threading
    from concurrent import futures

    got = {}
    done = threading.Event()

    def register_handler(request, context):
        got["version"] = request.version
        got["endpoint"] = request.endpoint
        got["resource_name"] = request.resource_name
        got["preferred"] = request.options.get_preferred_allocation_available
        done.set()
        return dpapi.Empty()

    kubelet_sock = str(sock_dir / "kubelet.sock")
    server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
    handler = grpc.method_handlers_generic_handler(
        dpapi.REGISTRATION_SERVICE,
        {"Register": grpc.unary_unary_rpc_method_handler(
            register_handler,
            request_deserializer=dpapi.RegisterRequest.FromString,
            response_serializer=lambda m: m.SerializeToString(),
        )},
    )
    server.add_generic_rpc_handlers((handler,))
    server.add_insecure_port(f"unix://{kubelet_sock}")
    server.start()
    try:
        mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
        mgr.start()
        p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "amdgpu.sock"))
        p.register_with_kubelet(kubelet_sock)
        assert done.wait(5)
        assert got["version"] == dpapi.VERSION
        assert got["endpoint"] == "amdgpu.sock"
        assert got["resource_name"] == "amd.com/gpu"
        assert got["preferred"] is True
    finally:
        server.stop(grace=0.5)


def test_full_kubelet_protocol_lifecycle(sock_dir):
    """The complete kubelet<->plugin protocol in sequence: Register ->
    GetDevicePluginOptions -> ListAndWatch -> GetPreferredAllocation ->
    Allocate (the CPU-only 'kind cluster' flow, BASELINE.json config 1)."""
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_2hive_8gpu()))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "life.sock"))
    p.start()
    try:
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        opts = _stub(ch, "GetDevicePluginOptions", dpapi.Empty,
                     dpapi.DevicePluginOptions)(dpapi.Empty(), timeout=10)
        assert opts.get_preferred_allocation_available
        frame = next(iter(_stub(ch, "ListAndWatch", dpapi.Empty,
                                dpapi.ListAndWatchResponse, streaming=True)(
            dpapi.Empty(), timeout=10)))
        ids = [d.ID for d in frame.devices if d.health == dpapi.HEALTHY]
        assert len(ids) == 8
        pref = _stub(ch, "GetPreferredAllocation",
                     dpapi.PreferredAllocationRequest,
                     dpapi.PreferredAllocationResponse)(
            dpapi.PreferredAllocationRequest(container_requests=[
                dpapi.ContainerPreferredAllocationRequest(
                    available_deviceIDs=ids, allocation_size=2)
            ]), timeout=10)
        chosen = list(pref.container_responses[0].deviceIDs)
        assert len(chosen) == 2
        alloc = _stub(ch, "Allocate", dpapi.AllocateRequest,
                      dpapi.AllocateResponse)(
            dpapi.AllocateRequest(container_requests=[
                dpapi.ContainerAllocateRequest(devicesIDs=chosen)
            ]), timeout=10)
        cresp = alloc.container_responses[0]
        paths = [d.host_path for d in cresp.devices]
        assert "/dev/kfd" in paths
        assert sum("renderD" in x for x in paths) == 2
        assert cresp.envs["ROCR_VISIBLE_DEVICES"] == ",".join(chosen)
        ch.close()
    finally:
        p.stop()


def test_discovery_failure_flips_unhealthy_and_recovers(sock_dir):
    """Backend failing mid-stream: next frame goes all-Unhealthy; a
    recovered backend flips devices back to Healthy."""
    from kubegpu_amd.discovery import Backend, DiscoveryError

    class Flaky(Backend):
        def __init__(self, inner):
            self.inner = inner
            self.fail = False

        def get_gpu_info(self):
            if self.fail:
                raise DiscoveryError("injected")
            return self.inner.get_gpu_info()

    flaky = Flaky(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr = create_device_plugin(flaky)
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "flaky.sock"))
    # fast re-send cadence: gRPC prefetches the next frame eagerly, so a
    # state change lands 1-2 frames later — poll to the expected state
    p.servicer.health_interval_s = 0.2
    p.start()

    def wait_state(it, want, frames=10):
        last = None
        for _ in range(frames):
            f = next(it)
            last = {d.ID: d.health for d in f.devices}
            if last and all(h == want for h in last.values()):
                return last
        raise AssertionError(f"never reached all-{want}: {last}")

    try:
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        stream = _stub(ch, "ListAndWatch", dpapi.Empty,
                       dpapi.ListAndWatchResponse, streaming=True)(
            dpapi.Empty(), timeout=60)
        it = iter(stream)
        wait_state(it, dpapi.HEALTHY)
        flaky.fail = True
        # expire the 5-min discovery cache (-inf, not 0.0: the monotonic
        # clock itself is below 300 s on a freshly booted machine)
        mgr._last_get_time = float("-inf")
        p.servicer.notify()
        bad = wait_state(it, dpapi.UNHEALTHY)
        assert len(bad) == 8  # devices stay visible
        flaky.fail = False
        mgr._last_get_time = float("-inf")
        p.servicer.notify()
        wait_state(it, dpapi.HEALTHY)
        ch.close()
    finally:
        p.stop()


def test_preferred_allocation_edge_cases(channel):
    """Malformed/degenerate requests never crash the server: empty
    request list, k=0, k > available, unknown must ids."""
    stub = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)
    # empty request
    resp = stub(dpapi.PreferredAllocationRequest(), timeout=10)
    assert len(resp.container_responses) == 0
    ids = [f"GPU-mi355x-{i:02d}" for i in range(8)]
    # k = 0
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=ids, allocation_size=0)]), timeout=10)
    assert list(resp.container_responses[0].deviceIDs) == []
    # k > available: best-effort prefix (kubelet treats as hint)
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=ids[:2], allocation_size=5)]), timeout=10)
    assert len(resp.container_responses[0].deviceIDs) == 2
    # unknown must id: falls back to an unconstrained best subset
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=ids,
            must_include_deviceIDs=["GPU-not-real"],
            allocation_size=2)]), timeout=10)
    assert len(resp.container_responses[0].deviceIDs) == 2


def test_allocate_empty_request(channel):
    resp = _stub(channel, "Allocate", dpapi.AllocateRequest,
                 dpapi.AllocateResponse)(
        dpapi.AllocateRequest(container_requests=[
            dpapi.ContainerAllocateRequest(devicesIDs=[])
        ]), timeout=10)
    cresp = resp.container_responses[0]
    # /dev/kfd is still listed (harmless), but no env without GPUs
    assert "ROCR_VISIBLE_DEVICES" not in cresp.envs


def test_preferred_allocation_avoids_down_links(sock_dir):
    """Degraded mesh through the STOCK path: GetPreferredAllocation
    avoids pairs whose xGMI link is down (p2p=false => host-path)."""
    fix = fixtures.fixture_degraded_mesh(missing=((0, 1), (0, 2), (0, 3), (0, 4)))
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "deg.sock"))
    p.start()
    try:
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        ids = [f"GPU-mi355x-{i:02d}" for i in range(8)]
        # ask for a pair including availability of the degraded GPU 0
        resp = _stub(ch, "GetPreferredAllocation",
                     dpapi.PreferredAllocationRequest,
                     dpapi.PreferredAllocationResponse)(
            dpapi.PreferredAllocationRequest(container_requests=[
                dpapi.ContainerPreferredAllocationRequest(
                    available_deviceIDs=ids, allocation_size=2)
            ]), timeout=10)
        pair = sorted(int(u.split("-")[-1])
                      for u in resp.container_responses[0].deviceIDs)
        # GPU 0 has 4 dead links; a healthy pair exists, so 0 with a dead
        # peer must not be chosen
        assert pair not in ([0, 1], [0, 2], [0, 3], [0, 4])
        ch.close()
    finally:
        p.stop()


def test_preferred_allocation_unsatisfiable_must_preserved(channel):
    """Strict must_include contract: when the
    constraint cannot be satisfied (more musts than allocation_size),
    the musts are preserved in the response — never silently dropped."""
    stub = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)
    ids = [f"GPU-mi355x-{i:02d}" for i in range(8)]
    musts = ["GPU-mi355x-01", "GPU-mi355x-06", "GPU-mi355x-03"]
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=ids,
            must_include_deviceIDs=musts,
            allocation_size=2)]), timeout=10)
    got = list(resp.container_responses[0].deviceIDs)
    assert got == musts  # declined, musts undropped


def test_preferred_allocation_must_not_offered_is_filtered(channel):
    """A must id absent from available_deviceIDs was never offered and
    must not appear in the preference."""
    stub = _stub(channel, "GetPreferredAllocation",
                 dpapi.PreferredAllocationRequest,
                 dpapi.PreferredAllocationResponse)
    avail = [f"GPU-mi355x-{i:02d}" for i in range(4)]  # hive 0 only
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=avail,
            must_include_deviceIDs=["GPU-mi355x-06"],  # offered? no
            allocation_size=2)]), timeout=10)
    got = list(resp.container_responses[0].deviceIDs)
    assert "GPU-mi355x-06" not in got
    assert len(got) == 2 and set(got) <= set(avail)
    # fast path (k >= len(avail)) filters too
    resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
        dpapi.ContainerPreferredAllocationRequest(
            available_deviceIDs=avail,
            must_include_deviceIDs=["GPU-mi355x-06"],
            allocation_size=4)]), timeout=10)
    got = list(resp.container_responses[0].deviceIDs)
    assert "GPU-mi355x-06" not in got and set(got) == set(avail)


def test_preferred_allocation_partial_known_musts_kept(plugin, channel):
    """One of two musts is tombstoned (vanished): the KNOWN must is kept
    in the chosen set instead of both being dropped."""
    mgr = plugin.manager
    # simulate GPU 05 vanishing from the inventory while kubelet still
    # offers it (stale ListAndWatch view)
    g5 = mgr.gpus.pop("GPU-mi355x-05")
    mgr.vanished["GPU-mi355x-05"] = (g5, 0.0)
    try:
        stub = _stub(channel, "GetPreferredAllocation",
                     dpapi.PreferredAllocationRequest,
                     dpapi.PreferredAllocationResponse)
        ids = [f"GPU-mi355x-{i:02d}" for i in range(8)]
        resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=ids,
                must_include_deviceIDs=["GPU-mi355x-05", "GPU-mi355x-04"],
                allocation_size=3)]), timeout=10)
        got = list(resp.container_responses[0].deviceIDs)
        assert "GPU-mi355x-04" in got  # the known must survives
        assert "GPU-mi355x-05" in got  # offered must leads even if unknown
        assert len(got) == 3
    finally:
        mgr.gpus["GPU-mi355x-05"] = g5
        mgr.vanished.pop("GPU-mi355x-05", None)


def test_preferred_allocation_prefers_idle_gpus(plugin, channel):
    """GPUs with live allocations or external compute processes lose to
    idle ones when enough idle devices exist (in_use surface,
    VERDICT round 1 #6)."""
    mgr = plugin.manager
    # hive 0 = {00..03}, hive 1 = {04..07}; mark two hive-1 GPUs busy
    mgr.gpus["GPU-mi355x-04"].in_use = True
    mgr.gpus["GPU-mi355x-05"].process_count = 2
    try:
        stub = _stub(channel, "GetPreferredAllocation",
                     dpapi.PreferredAllocationRequest,
                     dpapi.PreferredAllocationResponse)
        ids = [f"GPU-mi355x-{i:02d}" for i in range(8)]
        resp = stub(dpapi.PreferredAllocationRequest(container_requests=[
            dpapi.ContainerPreferredAllocationRequest(
                available_deviceIDs=ids, allocation_size=4)]), timeout=10)
        got = set(resp.container_responses[0].deviceIDs)
        assert got == {f"GPU-mi355x-{i:02d}" for i in range(4)}  # idle hive
    finally:
        mgr.gpus["GPU-mi355x-04"].in_use = False
        mgr.gpus["GPU-mi355x-05"].process_count = 0


# ---- protocol fidelity: version negotiation + kubelet restart ----------

class _FakeKubelet:
    """Minimal kubelet Registration endpoint whose socket can be torn
    down and recreated (restart simulation)."""

    def __init__(self, sock_path, accept_versions=("v1beta1",)):
        self.sock_path = sock_path
        self.accept_versions = accept_versions
        self.registrations = []
        self.server = None

    def start(self):
        import threading
        from concurrent import futures

        self.event = threading.Event()

        def handler(request, context):
            if request.version not in self.accept_versions:
                context.abort(
                    grpc.StatusCode.INVALID_ARGUMENT,
                    f"unsupported API version: {request.version}",
                )
            self.registrations.append(
                (request.version, request.endpoint, request.resource_name)
            )
            self.event.set()
            return dpapi.Empty()

        if os.path.exists(self.sock_path):
            os.unlink(self.sock_path)
        self.server = grpc.server(futures.ThreadPoolExecutor(max_workers=2))
        self.server.add_generic_rpc_handlers((
            grpc.method_handlers_generic_handler(
                dpapi.REGISTRATION_SERVICE,
                {"Register": grpc.unary_unary_rpc_method_handler(
                    handler,
                    request_deserializer=dpapi.RegisterRequest.FromString,
                    response_serializer=lambda m: m.SerializeToString(),
                )},
            ),
        ))
        self.server.add_insecure_port(f"unix://{self.sock_path}")
        self.server.start()

    def stop(self):
        if self.server is not None:
            self.server.stop(grace=0.2)
            self.server = None
        if os.path.exists(self.sock_path):
            os.unlink(self.sock_path)


def test_version_rejected_surfaces_registration_error(sock_dir):
    """A kubelet that only speaks another version rejects v1beta1; the
    plugin raises RegistrationError carrying kubelet's message instead
    of an anonymous RpcError."""
    from kubegpu_amd.server.kubelet_plugin import RegistrationError

    kubelet = _FakeKubelet(str(sock_dir / "kubelet.sock"),
                           accept_versions=("v1alpha2",))
    kubelet.start()
    try:
        mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
        mgr.start()
        p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "a.sock"))
        with pytest.raises(RegistrationError, match="unsupported API version"):
            p.register_with_kubelet(kubelet.sock_path)
    finally:
        kubelet.stop()


def test_reregister_after_kubelet_restart(sock_dir):
    """Kubelet restart wipes its plugin registry and recreates its
    socket; the watcher notices the new inode and re-registers, and the
    plugin keeps serving Allocate across the restart."""
    import time as _time

    kubelet = _FakeKubelet(str(sock_dir / "kubelet.sock"))
    kubelet.start()
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_2hive_8gpu()))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "amdgpu.sock"))
    p.start()
    try:
        p.register_with_kubelet(kubelet.sock_path)
        assert len(kubelet.registrations) == 1
        p.watch_kubelet(kubelet.sock_path, interval_s=0.1)

        # kubelet "restarts": socket torn down and recreated
        before = len(kubelet.registrations)
        kubelet.stop()
        _time.sleep(0.3)  # watcher sees the gap
        kubelet.start()
        deadline = _time.time() + 10
        while len(kubelet.registrations) <= before and _time.time() < deadline:
            _time.sleep(0.05)
        assert len(kubelet.registrations) > before, "watcher did not re-register"

        # plugin still serves allocations on its own (unchanged) socket
        ch = grpc.insecure_channel(f"unix://{p.socket_path}")
        alloc = _stub(ch, "Allocate", dpapi.AllocateRequest,
                      dpapi.AllocateResponse)(
            dpapi.AllocateRequest(container_requests=[
                dpapi.ContainerAllocateRequest(
                    devicesIDs=["GPU-mi355x-00", "GPU-mi355x-01"])
            ]), timeout=10)
        assert "ROCR_VISIBLE_DEVICES" in alloc.container_responses[0].envs
        ch.close()
    finally:
        p.stop()
        kubelet.stop()


def test_plugin_socket_recreation_race(sock_dir):
    """Restarting the plugin over a stale socket path works, and a new
    client connects to the NEW server instance (stale-socket unlink in
    start()); the old server's socket removal must not kill the new."""
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    path = str(sock_dir / "same.sock")
    p1 = KubeletDevicePlugin(mgr, socket_path=path)
    p1.start()
    # second instance takes over the same path (plugin upgrade pattern)
    p2 = KubeletDevicePlugin(mgr, socket_path=path)
    p2.start()
    try:
        ch = grpc.insecure_channel(f"unix://{path}")
        opts = _stub(ch, "GetDevicePluginOptions", dpapi.Empty,
                     dpapi.DevicePluginOptions)(dpapi.Empty(), timeout=10)
        assert opts.get_preferred_allocation_available
        ch.close()
    finally:
        p2.stop()
        p1.stop()


@pytest.mark.timeout(120)
def test_agent_process_lifecycle_with_fake_kubelet(sock_dir):
    """The production entry point end to end as a real process: starts,
    registers with a (fake) kubelet, survives a kubelet restart via the
    watcher, and exits 0 on SIGTERM."""
    import signal
    import subprocess
    import sys
    import time as _time

    kubelet = _FakeKubelet(str(sock_dir / "kubelet.sock"))
    kubelet.start()
    try:
        proc = subprocess.Popen(
            [sys.executable, "-m", "kubegpu_amd.server.agent",
             "--fake",
             "--socket", str(sock_dir / "agent.sock"),
             "--kubelet-socket", kubelet.sock_path,
             "--metrics-port", "0",
             "--health-interval", "0.2"],
            cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True,
        )
        assert kubelet.event.wait(30), "agent never registered"

        # kubelet restart: agent's watcher must re-register
        before = len(kubelet.registrations)
        kubelet.stop()
        _time.sleep(0.5)
        kubelet.start()
        deadline = _time.time() + 20
        while len(kubelet.registrations) <= before and _time.time() < deadline:
            _time.sleep(0.1)
        assert len(kubelet.registrations) > before, "no re-registration"

        proc.send_signal(signal.SIGTERM)
        out, _ = proc.communicate(timeout=30)
        assert proc.returncode == 0, out[-1500:]
    finally:
        kubelet.stop()
        if proc.poll() is None:
            proc.kill()


@pytest.mark.timeout(120)
def test_watcher_retries_until_kubelet_accepts(sock_dir):
    """A kubelet that comes back up broken (rejecting registrations)
    then recovers: the watcher keeps retrying each tick until accepted
    instead of giving up after the first failure."""
    import time as _time

    kubelet = _FakeKubelet(str(sock_dir / "kubelet.sock"))
    kubelet.start()
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    p = KubeletDevicePlugin(mgr, socket_path=str(sock_dir / "w.sock"))
    p.start()
    try:
        p.register_with_kubelet(kubelet.sock_path)
        p.watch_kubelet(kubelet.sock_path, interval_s=0.1)
        before = len(kubelet.registrations)

        # restart REJECTING v1beta1 (config error), then fix it
        kubelet.stop()
        _time.sleep(0.3)
        kubelet.accept_versions = ("v1alpha2",)
        kubelet.start()
        _time.sleep(0.6)  # several failed watcher attempts
        assert len(kubelet.registrations) == before  # rejected, none landed
        kubelet.accept_versions = ("v1beta1",)  # kubelet fixed (no restart)
        deadline = _time.time() + 10
        while len(kubelet.registrations) <= before and _time.time() < deadline:
            _time.sleep(0.05)
        assert len(kubelet.registrations) > before, "watcher gave up"
    finally:
        p.stop()
        kubelet.stop()
