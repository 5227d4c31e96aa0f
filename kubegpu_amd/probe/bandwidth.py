"""HBM bandwidth probe — wrapper over the _gpuprobe HIP extension.

The k=1 degenerate point of the BASELINE.md bandwidth curve: a 1-GPU
"scheduled set" has no interconnect, so the sanity number is HBM3E
streaming bandwidth from the hand-written CDNA4 copy kernel
(csrc/gpuprobe.hip; ≈6.3 TB/s achievable of the 8 TB/s spec).

copy() launches the address-ordered tile kernel with capped residency
per CU; copy_tiles / d2d_copy_tiles_bw_gbps expose that kernel's tile
size and cap, copy_variant / d2d_copy_bw_gbps the grid-stride kernels
it is measured against.

Fails LOUDLY when a GPU is present but the native extension is missing —
GPU tests must never silently fall back to eager PyTorch.
"""

from __future__ import annotations

import importlib
import os
import sys

_EXT_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "_ext")
_ext = None


class NativeExtensionMissing(RuntimeError):
    pass


def load_ext(required: bool = True):
    """Import the _gpuprobe torch extension built by build_native."""
    global _ext
    if _ext is not None:
        return _ext
    import torch  # noqa: F401  (extension needs torch symbols loaded)

    if _EXT_DIR not in sys.path:
        sys.path.insert(0, _EXT_DIR)
    try:
        _ext = importlib.import_module("_gpuprobe")
    except ImportError as e:
        if required or torch.cuda.is_available():
            raise NativeExtensionMissing(
                "_gpuprobe HIP extension is not built; run "
                "`python -m kubegpu_amd.build_native` (gfx950) — refusing "
                f"to fall back to eager PyTorch on a GPU box: {e}"
            ) from e
        return None
    return _ext


def copy(dst, src) -> None:
    """Launch the streaming copy kernel (numerics-testable)."""
    load_ext().copy(dst, src)


def copy_variant(
    dst,
    src,
    variant: int = 0,
    nontemporal: bool = True,
    blocks: int = 0,
    threads: int = 0,
) -> None:
    """One untimed launch of a d2d_copy_bw_gbps kernel on dst/src.

    Same kernel selection and default grid as the timed probe. Both
    tensors must be 16-byte aligned with nbytes a multiple of 16.
    """
    load_ext().copy_variant(dst, src, variant, nontemporal, blocks, threads)


def copy_tiles(dst, src, unroll: int, resident: int, max_blocks: int = 0) -> None:
    """One untimed launch of the address-ordered tile copy kernel.

    Tile t is the 256 * unroll consecutive 16-byte vectors from
    t * 256 * unroll, one workgroup per tile; unroll is 1, 2, 4 or 8.
    resident (1..8) keeps a CU from holding more than that many of the
    workgroups at a time, 0 leaves it uncapped. max_blocks > 0 caps the
    grid, so that workgroups loop over several tiles. Both tensors must
    be 16-byte aligned with nbytes a multiple of 16.
    """
    load_ext().copy_tiles(dst, src, unroll, resident, max_blocks)


def read_sum(src, blocks: int = 0) -> int:
    """Sum of all 32-bit words of src modulo 2**64 (one launch of the
    read_bw_gbps kernel into a zeroed accumulator)."""
    return load_ext().read_sum(src, blocks)


def fill_word(dst, word: int, blocks: int = 0) -> None:
    """Set every 32-bit word of dst to word (one launch of the
    write_bw_gbps kernel)."""
    load_ext().fill_word(dst, word, blocks)


def d2d_copy_bw_gbps(
    nbytes: int = 1 << 30,
    iters: int = 20,
    blocks: int = 0,
    nontemporal: bool = True,
    variant: int = 0,
) -> float:
    """Timed device-to-device streaming-copy bandwidth (GB/s, R+W).

    variant: 0 = grid-stride NT, 1 = 4x-unrolled NT, 2 = contiguous-chunk
    NT, 3 = regular loads + NT stores.
    """
    return load_ext().copy_bw_gbps(nbytes, iters, blocks, nontemporal, variant)


def d2d_copy_tiles_bw_gbps(
    nbytes: int = 1 << 30,
    iters: int = 20,
    unroll: int = 1,
    resident: int = 0,
    max_blocks: int = 0,
) -> float:
    """Timed bandwidth (GB/s, R+W) of the tile copy kernel: the same
    launch as copy_tiles, timed and self-checked like d2d_copy_bw_gbps."""
    return load_ext().copy_tiles_bw_gbps(nbytes, iters, unroll, resident, max_blocks)


def read_bw_gbps(nbytes: int = 1 << 30, iters: int = 20, blocks: int = 0) -> float:
    return load_ext().read_bw_gbps(nbytes, iters, blocks)


def write_bw_gbps(nbytes: int = 1 << 30, iters: int = 20, blocks: int = 0) -> float:
    """Timed write-only (nontemporal fill) bandwidth (GB/s)."""
    return load_ext().write_bw_gbps(nbytes, iters, blocks)
