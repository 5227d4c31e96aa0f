"""A probe that claims to exercise an instruction must issue it: compile
csrc/ldscheck.hip device-only to gfx950 assembly and look, in the body of
the kernel the probe runs, for every LDS instruction the probe's docstring
names, and for the wait between each LDS-DMA and the first LDS read after
it.  Needs hipcc, no GPU."""

import os
import re
import subprocess
import sysconfig

import pytest

from kubegpu_amd import build_native

pytestmark = pytest.mark.skipif(not os.path.exists(build_native.HIPCC),
                                reason="hipcc not installed")

INSTRUCTIONS = (
    # width
    "ds_write_b8", "ds_write_b16", "ds_read_u8", "ds_read_i8", "ds_read_u16", "ds_read_i16",
    "ds_write_b64", "ds_read_b64", "ds_write_b96", "ds_read_b96", "ds_write_b128",
    "ds_read_b128", "ds_write2_b32", "ds_read2_b32", "ds_write2st64_b32", "ds_read2st64_b32",
    "ds_read_b64_tr_b16",
    # bank, xwave
    "ds_write_b32", "ds_read_b32", "s_barrier",
    # dma
    "global_load_lds_dwordx4", "global_load_lds_dword",
)


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from torch.utils.cpp_extension import include_paths

    out = tmp_path_factory.mktemp("ldscheck_isa") / "ldscheck.s"
    includes = include_paths() + [os.path.join(build_native.ROCM, "include"),
                                  sysconfig.get_paths()["include"]]
    cmd = [build_native.HIPCC, f"--offload-arch={build_native.GFX_ARCH}",
           "--cuda-device-only", "-S", "-O3", "-std=c++17",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1"]
    cmd += [f"-I{p}" for p in includes]
    cmd += [os.path.join(build_native.CSRC, "ldscheck.hip"), "-o", str(out)]
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


def test_every_claimed_instruction_is_issued_by_the_kernel_the_probe_runs(asm):
    for kernel in ("ldscheck_kernel", "ldscheck_values_kernel"):
        issued = {m for m, _ in _body(asm, kernel)}
        missing = [name for name in INSTRUCTIONS if name not in issued]
        assert not missing, (kernel, missing)


def test_the_dma_forms_the_docstring_names(asm):
    lines = [line for m, line in _body(asm, "ldscheck_kernel") if m.startswith("global_load_lds")]
    x4 = [line for line in lines if line.startswith("global_load_lds_dwordx4")]
    dw = [line for line in lines if line.startswith("global_load_lds_dword ")]
    assert len(x4) == 5 and len(dw) == 4  # three placed and two gathered, two and two
    assert sum("offset:1024" in line for line in x4) == 1
    assert sum("offset:2048" in line for line in x4) == 1
    assert sum("offset:768" in line for line in dw) == 1
    # the st64 pair is 64 * ST64_K dwords apart, the two-address pair adjacent
    from kubegpu_amd.probe import ldscheck as ld

    body = _body(asm, "ldscheck_kernel")
    assert any(m == "ds_read2st64_b32" and f"offset1:{ld.ST64_K}" in line for m, line in body)
    assert any(m == "ds_write2st64_b32" and f"offset1:{ld.ST64_K}" in line for m, line in body)
    assert any(m == "ds_write2_b32" and "offset1:1" in line for m, line in body)


@pytest.mark.parametrize("kernel", ("ldscheck_kernel", "ldscheck_values_kernel"))
def test_a_vmcnt_wait_stands_between_each_dma_and_the_next_lds_read(asm, kernel):
    body = _body(asm, kernel)
    dmas = [i for i, (m, _) in enumerate(body) if m.startswith("global_load_lds")]
    assert dmas
    for i in dmas:
        reads = [k for k in range(i + 1, len(body)) if body[k][0].startswith("ds_read")]
        assert reads, "a DMA with no LDS read behind it"
        between = body[i + 1:reads[0]]
        waits = [k for k, (m, line) in enumerate(between)
                 if m == "s_waitcnt" and "vmcnt(0)" in line]
        assert waits, (body[i][1], body[reads[0]][1])
        # and ahead of any branch, so that no path to the read jumps over it
        jumps = [k for k, (m, _) in enumerate(between)
                 if m.startswith("s_cbranch") or m == "s_branch"]
        assert not jumps or waits[0] < jumps[0], (body[i][1], between[jumps[0]][1])
