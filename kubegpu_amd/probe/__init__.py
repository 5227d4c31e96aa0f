"""Bandwidth probes: RCCL-over-xGMI all-reduce + CDNA4 HBM kernels."""

from .bandwidth import (  # noqa: F401
    copy,
    copy_variant,
    d2d_copy_bw_gbps,
    fill_word,
    load_ext,
    read_bw_gbps,
    read_sum,
    write_bw_gbps,
)
from .rccl_probe import (  # noqa: F401
    RcclProbeCheckFailed,
    run_rccl_probe,
    torch_allreduce_busbw,
)
from .xgmi_counters import (  # noqa: F401
    diff_link_metrics,
    probe_with_link_utilization,
    read_link_metrics,
)

# HBM integrity probe (probe/memcheck.py), re-exported lazily so that
# `python -m kubegpu_amd.probe.memcheck` runs the module exactly once.
# The memcheck() function itself shares its name with the submodule, so
# it is reached as `kubegpu_amd.probe.memcheck.memcheck`.
_MEMCHECK_EXPORTS = (
    "MemcheckResult",
    "VerifyResult",
    "fill_pattern",
    "memcheck_round",
    "reference_words",
    "run_memcheck_subprocess",
    "verify_pattern",
    "verify_then_fill",
)


# Compute-unit integrity probe (probe/cucheck.py), the same way; the
# cucheck() function is `kubegpu_amd.probe.cucheck.cucheck`.
_CUCHECK_EXPORTS = (
    "CucheckResult",
    "cucheck_round",
    "reference_digests",
    "run_cucheck_subprocess",
    "wave_digests",
)


# Matrix-core format integrity probe (probe/mxcheck.py), the same way;
# the mxcheck() function is `kubegpu_amd.probe.mxcheck.mxcheck`.  Its
# reference_digests / wave_digests stay in the submodule: the
# package-level names are cucheck's.
_MXCHECK_EXPORTS = (
    "MxcheckResult",
    "mxcheck_round",
    "run_mxcheck_subprocess",
    "wave_tile",
)


# IEEE rounding integrity probe (probe/fpcheck.py), the same way; the
# fpcheck() function is `kubegpu_amd.probe.fpcheck.fpcheck`.  Its
# reference_digests / wave_digests stay in the submodule too.
_FPCHECK_EXPORTS = (
    "FpcheckResult",
    "fpcheck_round",
    "run_fpcheck_subprocess",
    "wave_values",
)


# Host-link integrity and bandwidth probe (probe/hostlink.py), the same
# way; the hostlink() function is `kubegpu_amd.probe.hostlink.hostlink`.
# Its fill_pattern / verify_pattern take host tensors and stay in the
# submodule: the package-level names are memcheck's.
_HOSTLINK_EXPORTS = (
    "HostlinkResult",
    "hostlink_round",
    "read_pcie_link",
    "run_hostlink_subprocess",
)


# Atomic-unit integrity probe (probe/atomcheck.py), the same way; the
# atomcheck() function is `kubegpu_amd.probe.atomcheck.atomcheck`.  Its
# reference_digests / wave_digests / wave_values stay in the submodule
# too.
_ATOMCHECK_EXPORTS = (
    "AtomcheckResult",
    "atomcheck_round",
    "reference_shared",
    "run_atomcheck_subprocess",
)


# Cross-lane integrity probe (probe/lanecheck.py), the same way; the
# lanecheck() function is `kubegpu_amd.probe.lanecheck.lanecheck`.  Its
# reference_digests / wave_digests / wave_values stay in the submodule
# too.
_LANECHECK_EXPORTS = (
    "LanecheckResult",
    "dpp_source",
    "lanecheck_round",
    "run_lanecheck_subprocess",
)


# LDS integrity probe (probe/ldscheck.py), the same way; the ldscheck()
# function is `kubegpu_amd.probe.ldscheck.ldscheck`.  Its
# reference_digests / wave_digests / wave_values stay in the submodule
# too.
_LDSCHECK_EXPORTS = (
    "LdscheckResult",
    "ldscheck_round",
    "run_ldscheck_subprocess",
    "source_tables",
    "transposed_read",
)


# Vector-memory integrity probe (probe/vmemcheck.py), the same way; the
# vmemcheck() function is `kubegpu_amd.probe.vmemcheck.vmemcheck`.  Its
# reference_digests / wave_digests / wave_values stay in the submodule
# too.
_VMEMCHECK_EXPORTS = (
    "VmemcheckResult",
    "vmemcheck_round",
    "run_vmemcheck_subprocess",
    "source_table",
)


_LAZY_EXPORTS = {
    "memcheck": _MEMCHECK_EXPORTS,
    "cucheck": _CUCHECK_EXPORTS,
    "mxcheck": _MXCHECK_EXPORTS,
    "fpcheck": _FPCHECK_EXPORTS,
    "hostlink": _HOSTLINK_EXPORTS,
    "atomcheck": _ATOMCHECK_EXPORTS,
    "lanecheck": _LANECHECK_EXPORTS,
    "ldscheck": _LDSCHECK_EXPORTS,
    "vmemcheck": _VMEMCHECK_EXPORTS,
}


def __getattr__(name):
    for module, names in _LAZY_EXPORTS.items():
        if name in names:
            import importlib

            return getattr(importlib.import_module(f"{__name__}.{module}"), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
