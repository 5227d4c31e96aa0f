"""The address-ordered tile copy kernel (copy_kernel_tiles in
csrc/gpuprobe.hip) and copy(), which may launch it, on a real MI355X
against exact numpy references.

Every source word is distinct, so a permuted index, a vector copied
twice or a wrong source vector cannot pass. Destinations are views into
a sentinel-filled arena with guard bytes on both sides, so a skipped
tail and a write past the end both show. No tolerances, no bandwidth
assertions.
"""

import functools
import math

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import bandwidth as bw

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A  # byte every destination and guard holds before a launch
GUARD = 256  # bytes on each side of a destination (multiple of 16)
MIB = 1 << 20

UNROLLS = (1, 2, 4, 8)
BIG_BYTES = 4 * MIB + 16
SMALL_BYTES = 16 * (9 * 256 * max(UNROLLS) + 77)

# (max_blocks, resident): one tile per workgroup without an LDS request,
# with the whole CU's LDS (above 64 KiB, which has to be asked for) and
# with a quarter of it; then three workgroups looping over the tiles, so
# that the partial tile falls on a workgroup that has run full ones.
SETTINGS = ((0, 0), (0, 1), (0, 4), (3, 0))


def shapes(T):
    """Vector counts around the tile size T = 256 * unroll: below one
    wave, around one wave and one workgroup, around one tile, a partial
    last tile after one, three and nine full ones."""
    return (1, 63, 64, 255, 256, 257, T - 1, T, T + 1, 2 * T - 1, 3 * T + 5, 9 * T + 77)


@functools.lru_cache(maxsize=None)
def ref_words():
    """Shared, read-only host reference: distinct 32-bit words (an odd
    multiplier is a bijection modulo 2^32)."""
    n = BIG_BYTES // 4
    w = ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) & 0xFFFFFFFF).astype(np.uint32)
    assert len(np.unique(w)) == n
    w.setflags(write=False)
    return w


def ref_bytes(nbytes):
    return ref_words().view(np.uint8)[:nbytes]


@functools.lru_cache(maxsize=None)
def dev_source():
    """The reference words on the device, as bytes. Never written."""
    return torch.from_numpy(ref_words().view(np.uint8).copy()).cuda()


class Arena:
    """One reusable device buffer: destination views with guards."""

    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes + 2 * GUARD, dtype=torch.uint8, device="cuda")

    def view(self, nbytes):
        """Refill the sentinel and return nbytes at GUARD."""
        assert GUARD + nbytes + GUARD <= self.buf.numel()
        self.buf.fill_(SENTINEL)
        return self.buf[GUARD:GUARD + nbytes]

    def check(self, nbytes, want, what=None):
        """Destination equals want and every other byte is the sentinel."""
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        got = host[GUARD:GUARD + nbytes]
        bad = np.flatnonzero(got != want)
        assert np.array_equal(got, want), (what, "first bad byte", int(bad[0]), len(bad))
        assert (host[:GUARD] == SENTINEL).all(), (what, "guard before destination overwritten")
        assert (host[GUARD + nbytes:] == SENTINEL).all(), (
            what, "guard after destination overwritten")

    def untouched(self):
        torch.cuda.synchronize()
        assert (self.buf.cpu().numpy() == SENTINEL).all()


@pytest.fixture(scope="module")
def small():
    return Arena(SMALL_BYTES)


@pytest.fixture(scope="module")
def big():
    return Arena(BIG_BYTES)


def ext():
    return bw.load_ext(required=True)


# 1. copy_tiles ------------------------------------------------------------------

@pytest.mark.parametrize("max_blocks,resident", SETTINGS)
@pytest.mark.parametrize("unroll", UNROLLS)
def test_copy_tiles(small, unroll, max_blocks, resident):
    for n4 in shapes(256 * unroll):
        n = 16 * n4
        dst = small.view(n)
        bw.copy_tiles(dst, dev_source()[:n], unroll, resident, max_blocks)
        small.check(n, ref_bytes(n), what=(unroll, resident, max_blocks, n4))


def test_copy_tiles_same_tensor(small):
    """dst == src is legal: a thread reads a vector before it writes it."""
    n = 16 * (3 * 1024 + 5)
    for unroll in UNROLLS:
        t = dev_source()[:n].clone()
        bw.copy_tiles(t, t, unroll, 0)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), ref_bytes(n)), unroll


def test_copy_tiles_argument_checks(small):
    e = ext()
    dst = small.view(4096)
    src = dev_source()
    bad = [
        lambda: e.copy_tiles(dst, src[:4096], 0, 0),  # unroll
        lambda: e.copy_tiles(dst, src[:4096], 3, 0),
        lambda: e.copy_tiles(dst, src[:4096], 16, 0),
        lambda: e.copy_tiles(dst, src[:4096], 1, -1),  # resident
        lambda: e.copy_tiles(dst, src[:4096], 1, 9),
        lambda: e.copy_tiles(dst, src[:4096], 1, 0, -1),  # max_blocks
        lambda: e.copy_tiles(dst, src[:4096], 1, 0, (1 << 20) + 1),
        lambda: e.copy_tiles(dst, src[4:4100], 1, 0),  # misaligned source
        lambda: e.copy_tiles(dst[8:4088], src[:4080], 1, 0),  # misaligned destination
        lambda: e.copy_tiles(dst[:24], src[:24], 1, 0),  # nbytes % 16
        lambda: e.copy_tiles(dst, src[:4080], 1, 0),  # size mismatch
        lambda: e.copy_tiles(dst[:0], src[:0], 1, 0),  # empty
        lambda: e.copy_tiles(dst, src[:4096].cpu(), 1, 0),
        lambda: e.copy_tiles(dst[16:2064], dst[:2048], 1, 0),  # partial overlap
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    small.untouched()


# 2. copy(), vector path ---------------------------------------------------------

@pytest.mark.parametrize("nbytes", [16, 4080, 4112, BIG_BYTES])
def test_copy_vector_path(small, big, nbytes):
    arena = big if nbytes > SMALL_BYTES else small
    dst = arena.view(nbytes)
    bw.copy(dst, dev_source()[:nbytes])
    arena.check(nbytes, ref_bytes(nbytes), what=nbytes)


def test_copy_same_tensor_is_allowed():
    t = dev_source()[:4112].clone()
    bw.copy(t, t)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), ref_bytes(4112))


# 3. copy_tiles_bw_gbps ----------------------------------------------------------

def finite_positive(x):
    return isinstance(x, float) and math.isfinite(x) and x > 0


@pytest.mark.parametrize("resident", [0, 4])
@pytest.mark.parametrize("unroll", UNROLLS)
def test_copy_tiles_bw_gbps_runs_and_checks_itself(unroll, resident):
    assert finite_positive(ext().copy_tiles_bw_gbps(MIB, 2, unroll, resident))
    assert finite_positive(bw.d2d_copy_tiles_bw_gbps(MIB, 2, unroll, resident))


def test_copy_tiles_bw_gbps_argument_checks():
    e = ext()
    bad = [
        lambda: e.copy_tiles_bw_gbps(24, 2, 1, 0),  # nbytes
        lambda: e.copy_tiles_bw_gbps(MIB, 0, 1, 0),  # iters
        lambda: e.copy_tiles_bw_gbps(MIB, 2, 3, 0),  # unroll
        lambda: e.copy_tiles_bw_gbps(MIB, 2, 1, 9),  # resident
        lambda: e.copy_tiles_bw_gbps(MIB, 2, 1, 0, -1),  # max_blocks
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
