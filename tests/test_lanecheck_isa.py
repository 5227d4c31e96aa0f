"""A probe that claims to exercise an instruction must issue it: compile
csrc/lanecheck.hip device-only to gfx950 assembly and look for every
cross-lane instruction and DPP control the probe's docstring names.
Needs hipcc, no GPU."""

import os
import re
import subprocess
import sysconfig

import pytest

from kubegpu_amd import build_native
from kubegpu_amd.probe import lanecheck as lc

pytestmark = pytest.mark.skipif(not os.path.exists(build_native.HIPCC),
                                reason="hipcc not installed")

INSTRUCTIONS = (
    "v_mov_b32_dpp",
    "ds_bpermute_b32", "ds_permute_b32", "ds_swizzle_b32",
    "v_readlane_b32", "v_readfirstlane_b32", "v_mbcnt_lo_u32_b32", "v_mbcnt_hi_u32_b32",
    "v_permlane16_swap", "v_permlane32_swap",
)


def _dpp_text(entry):
    """An entry of DPP_TABLE the way the assembler prints it."""
    ctrl, row_mask, bank_mask, bound_ctrl = entry
    name = lc._ctrl_name(ctrl).replace("quad_perm", "quad_perm:")
    text = f"{name} row_mask:0x{row_mask:x} bank_mask:0x{bank_mask:x}"
    return text + (" bound_ctrl:1" if bound_ctrl else "")


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    from torch.utils.cpp_extension import include_paths

    out = tmp_path_factory.mktemp("lanecheck_isa") / "lanecheck.s"
    includes = include_paths() + [os.path.join(build_native.ROCM, "include"),
                                  sysconfig.get_paths()["include"]]
    cmd = [build_native.HIPCC, f"--offload-arch={build_native.GFX_ARCH}",
           "--cuda-device-only", "-S", "-O3", "-std=c++17",
           "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1"]
    cmd += [f"-I{p}" for p in includes]
    cmd += [os.path.join(build_native.CSRC, "lanecheck.hip"), "-o", str(out)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    return out.read_text()


def _run_kernel(asm):
    """The body of the kernel the probe runs: from its label to its
    s_endpgm."""
    start = re.search(r"^_Z\d+lanecheck_kernel\w*:", asm, re.M).start()
    return asm[start:asm.index("s_endpgm", start)]


def test_every_claimed_instruction_is_issued(asm):
    missing = [name for name in INSTRUCTIONS if name not in asm]
    assert not missing, missing
    # and by the kernel the probe runs, not only by the single-wave launcher
    run = _run_kernel(asm)
    missing = [name for name in INSTRUCTIONS if name not in run]
    assert not missing, missing


def test_every_dpp_control_of_the_table_is_issued(asm):
    for keyword in ("quad_perm:[3,2,1,0]", "quad_perm:[1,0,3,2]", "row_shl:", "row_shr:",
                    "row_ror:", "wave_shl:1", "wave_rol:1", "wave_shr:1", "wave_ror:1",
                    "row_mirror", "row_half_mirror", "row_bcast:15", "row_bcast:31",
                    "row_newbcast:"):
        assert keyword in asm, keyword
    run = _run_kernel(asm)
    missing = [text for text in map(_dpp_text, lc.DPP_TABLE) if text not in run]
    assert not missing, missing


def test_every_swizzle_of_the_table_is_issued(asm):
    run = _run_kernel(asm)
    for text in ("swizzle(SWAP,1)", "swizzle(SWAP,2)", "swizzle(SWAP,4)", "swizzle(SWAP,8)",
                 "swizzle(SWAP,16)", "swizzle(REVERSE,32)", "swizzle(BROADCAST,8,3)",
                 "swizzle(QUAD_PERM,3,2,1,0)", "swizzle(QUAD_PERM,1,1,3,0)"):
        assert text in run, text
    assert run.count("ds_swizzle_b32") >= len(lc.SWIZZLES)
