"""A probe that claims to exercise an instruction must issue it: compile
csrc/vmemcheck.hip device-only to gfx950 assembly and look, in the bodies
of both kernels, for every vector-memory, scalar-load and buffer
instruction the probe's docstring names, with the cache-policy bits and
offset forms it names.  Needs hipcc, no GPU."""

import os
import re
import subprocess
import sysconfig

import pytest

from kubegpu_amd import build_native

pytestmark = pytest.mark.skipif(not os.path.exists(build_native.HIPCC),
                                reason="hipcc not installed")

KERNELS = ("vmemcheck_kernel", "vmemcheck_values_kernel")
INSTRUCTIONS = (
    "global_store_byte", "global_store_short", "global_store_dword", "global_store_dwordx2",
    "global_store_dwordx3", "global_store_dwordx4",
    "global_load_ubyte", "global_load_sbyte", "global_load_ushort", "global_load_sshort",
    "global_load_dword", "global_load_dwordx2", "global_load_dwordx3", "global_load_dwordx4",
)
SCALAR_LOADS = ("s_load_dword", "s_load_dwordx2", "s_load_dwordx4", "s_load_dwordx8",
                "s_load_dwordx16")
BUFFER_LOADS = ("buffer_load_ubyte", "buffer_load_ushort", "buffer_load_dword",
                "buffer_load_dwordx2", "buffer_load_dwordx3", "buffer_load_dwordx4")
BUFFER_STORES = ("buffer_store_byte", "buffer_store_dword", "buffer_store_dwordx4")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from torch.utils.cpp_extension import include_paths

    out = tmp_path_factory.mktemp("vmemcheck_isa") / "vmemcheck.s"
    includes = include_paths() + [os.path.join(build_native.ROCM, "include"),
                                  sysconfig.get_paths()["include"]]
    cmd = [build_native.HIPCC, f"--offload-arch={build_native.GFX_ARCH}",
           "--cuda-device-only", "-S", "-O3", "-std=c++17",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1"]
    cmd += [f"-I{p}" for p in includes]
    cmd += [os.path.join(build_native.CSRC, "vmemcheck.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def _body(asm, kernel):
    """The instructions of a kernel, from its label to the end of the
    function: a list of (mnemonic, whole line)."""
    start = re.search(rf"^_Z\d+{kernel}\w*:", asm, re.M).start()
    text = asm[start:asm.index(".Lfunc_end", start)]
    out = []
    for line in text.splitlines():
        line = line.split(";")[0].strip()
        if line and not line.startswith(".") and not line.endswith(":"):
            out.append((line.split()[0], line))
    return out


def _has(line, bit):
    return bit in line.split()[1:]


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_claimed_global_access_is_issued(asm, kernel):
    body = _body(asm, kernel)
    issued = {m for m, _ in body}
    missing = [name for name in INSTRUCTIONS if name not in issued]
    assert not missing, missing
    # every access to the arena and to X is a global one
    assert not [m for m in issued if m.startswith(("flat_", "scratch_"))]


@pytest.mark.parametrize("kernel", KERNELS)
def test_cache_policy_bits(asm, kernel):
    body = _body(asm, kernel)
    for kind in ("global_load", "global_store"):
        lines = [line for m, line in body if m.startswith(kind)]
        assert any(_has(line, "sc1") for line in lines), kind
        assert any(_has(line, "nt") for line in lines), kind
        assert any(not _has(line, "sc1") and not _has(line, "nt") for line in lines), kind
    # each policy at each gather width, the 16-byte sc1 load being two of 8 bytes
    loads = [(m, line) for m, line in body if m.startswith("global_load_dword")]
    for m, bit in (("global_load_dword", "sc1"), ("global_load_dword", "nt"),
                   ("global_load_dwordx2", "sc1"), ("global_load_dwordx2", "nt"),
                   ("global_load_dwordx4", "nt")):
        assert any(name == m and _has(line, bit) for name, line in loads), (m, bit)
    # the fence pairs cost no cache maintenance
    assert not [m for m, _ in body if m.startswith(("buffer_wbl2", "buffer_inv"))]


@pytest.mark.parametrize("kernel", KERNELS)
def test_uniform_loads_go_through_the_scalar_unit(asm, kernel):
    # a kernel-argument load has an immediate offset only; a load from the
    # table takes its offset from a register
    table = [m for m, line in _body(asm, kernel)
             if m.startswith("s_load_dword") and re.search(r"\], s\d+( offset:\w+)?$", line)]
    missing = [name for name in SCALAR_LOADS if name not in table]
    assert not missing, (missing, table)


@pytest.mark.parametrize("kernel", KERNELS)
def test_buffer_accesses_and_their_offset_forms(asm, kernel):
    body = _body(asm, kernel)
    lines = {name: [line for m, line in body if m == name]
             for name in BUFFER_LOADS + BUFFER_STORES}
    for name in BUFFER_LOADS + BUFFER_STORES:
        assert lines[name], name
        assert all(_has(line, "offen") for line in lines[name]), name
    loads = [line for name in BUFFER_LOADS for line in lines[name]]
    # one load with an SGPR soffset, one with an immediate offset
    assert sum(bool(re.search(r"\], s\d+ offen", line)) for line in loads) == 1
    assert sum("offset:256" in line for line in loads) == 1
    # no waterfall loop round a buffer access: the resource is built once
    # per stage from two readfirstlanes
    assert sum(m == "v_readfirstlane_b32" for m, _ in body) <= 4
