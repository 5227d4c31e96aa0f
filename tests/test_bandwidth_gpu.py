"""Bandwidth kernels (csrc/gpuprobe.hip) on a real MI355X against exact
numpy references: every copy variant, the byte fallback, read_sum,
fill_word, copy()'s dispatch and argument checks, and the timed probes'
self-checks.

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
SLACK = 16  # room for destinations at a small byte offset
WORD = 0xA5C3F00F  # not byte-symmetric: a byte-wise fill cannot produce it

# Explicit (blocks, threads) grids: S = blocks * threads vectors per sweep.
GRIDS = ((3, 64), (3, 256), (2, 1024))
DEFAULT_N4 = 1024 * 256 + 1  # one full default-grid sweep plus one vector


def shapes(S):
    """Vector counts around the sweep size S: fewer vectors than blocks
    (the chunked kernel's begin-past-the-end case), ragged tails, 3S (the
    unrolled kernel's bound == 0), 3S+1 (its main loop entered by one
    thread), 4S+5 (a full main pass plus a five-vector tail), and
    several sweeps."""
    return (1, 2, S - 1, S, S + 1, 3 * S - 1, 3 * S, 3 * S + 1, 4 * S, 4 * S + 5,
            9 * S + 77)


ALL_N4 = tuple(sorted({n for b, t in GRIDS for n in shapes(b * t)}))
SMALL_BYTES = 16 * max(ALL_N4)  # 9 * 2048 + 77 vectors, 289 KiB
BIG_BYTES = 16 * DEFAULT_N4  # 4 MiB + 16 B


@functools.lru_cache(maxsize=None)
def ref_words():
    """Shared, read-only host reference: distinct 32-bit words (an odd
    multiplier is a bijection modulo 2^32)."""
    n = BIG_BYTES // 4
    w = ((np.arange(n, dtype=np.uint64) * 2654435761 + 12345) & 0xFFFFFFFF).astype(np.uint32)
    assert len(np.unique(w)) == n
    w.setflags(write=False)
    return w


def ref_bytes(nbytes, offset=0):
    return ref_words().view(np.uint8)[offset:offset + nbytes]


@functools.lru_cache(maxsize=None)
def dev_source():
    """The reference words on the device, as bytes. Never written."""
    return torch.from_numpy(ref_words().view(np.uint8).copy()).cuda()


class Arena:
    """One reusable device buffer: destination views with guards."""

    def __init__(self, nbytes):
        self.buf = torch.empty(nbytes + 2 * GUARD + SLACK, dtype=torch.uint8, device="cuda")

    def view(self, nbytes, offset=0):
        """Refill the sentinel and return nbytes at GUARD + offset."""
        lo = GUARD + offset
        assert lo + nbytes + GUARD <= self.buf.numel()
        self.buf.fill_(SENTINEL)
        return self.buf[lo:lo + nbytes]

    def check(self, nbytes, want, offset=0, what=None):
        """Destination equals want and every other byte is the sentinel."""
        torch.cuda.synchronize()
        host = self.buf.cpu().numpy()
        lo = GUARD + offset
        got = host[lo:lo + nbytes]
        bad = np.flatnonzero(got != want)
        assert np.array_equal(got, want), (what, "first bad byte", int(bad[0]), len(bad))
        assert (host[:lo] == SENTINEL).all(), (what, "guard before destination overwritten")
        assert (host[lo + nbytes:] == SENTINEL).all(), (what, "guard after destination overwritten")

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


# 1. copy_variant ---------------------------------------------------------------

KERNELS = [(0, True), (0, False), (1, True), (2, True), (3, True)]


def run_copy_variant(arena, n4, variant, nontemporal, blocks, threads):
    n = 16 * n4
    dst = arena.view(n)
    bw.copy_variant(dst, dev_source()[:n], variant, nontemporal, blocks, threads)
    arena.check(n, ref_bytes(n), what=(variant, nontemporal, blocks, threads, n4))


@pytest.mark.parametrize("blocks,threads", GRIDS)
@pytest.mark.parametrize("variant,nontemporal", KERNELS)
def test_copy_variant_explicit_grids(small, variant, nontemporal, blocks, threads):
    for n4 in shapes(blocks * threads):
        run_copy_variant(small, n4, variant, nontemporal, blocks, threads)


@pytest.mark.parametrize("variant,nontemporal", KERNELS)
def test_copy_variant_default_grid(big, variant, nontemporal):
    run_copy_variant(big, DEFAULT_N4, variant, nontemporal, 0, 0)


def test_copy_variant_argument_checks(small):
    e = ext()
    dst = small.view(4096)
    src = dev_source()
    bad = [
        lambda: e.copy_variant(dst, src[:4096], 4),  # variant
        lambda: e.copy_variant(dst, src[:4096], -1),
        lambda: e.copy_variant(dst, src[:4096], 0, True, -1),  # blocks
        lambda: e.copy_variant(dst, src[:4096], 0, True, (1 << 20) + 1),
        lambda: e.copy_variant(dst, src[:4096], 0, True, 0, 96),  # threads
        lambda: e.copy_variant(dst, src[:4096], 0, True, 0, 2048),
        lambda: e.copy_variant(dst[:24], src[:24]),  # nbytes % 16
        lambda: e.copy_variant(dst, src[4:4100]),  # misaligned source
        lambda: e.copy_variant(dst[8:4088], src[:4080]),  # misaligned destination
        lambda: e.copy_variant(dst, src[:4080]),  # size mismatch
        lambda: e.copy_variant(dst[:0], src[:0]),  # empty
        lambda: e.copy_variant(dst, src[:4096].cpu()),
        lambda: e.copy_variant(dst[16:2064], dst[:2048]),  # partial overlap
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    small.untouched()


# 2. copy(), vector path ----------------------------------------------------------

@pytest.mark.parametrize("nbytes", [16, 4080, 4112, BIG_BYTES])
def test_copy_vector_path(small, big, nbytes):
    arena = big if nbytes > SMALL_BYTES else small
    dst = arena.view(nbytes)
    bw.copy(dst, dev_source()[:nbytes])
    arena.check(nbytes, ref_bytes(nbytes), what=nbytes)


# 3. copy(), byte path --------------------------------------------------------------

@pytest.mark.parametrize("nbytes", [1, 15, 17, 4099, 256 * 4096 + 7])
def test_copy_byte_path_odd_sizes(small, big, nbytes):
    # 256 * 4096 + 7: past one full sweep of the byte kernel's 4096-block grid
    arena = big if nbytes > SMALL_BYTES else small
    dst = arena.view(nbytes)
    bw.copy(dst, dev_source()[:nbytes])
    arena.check(nbytes, ref_bytes(nbytes), what=nbytes)


@pytest.mark.parametrize("src_off,dst_off", [(4, 8), (4, 0), (0, 8)])
def test_copy_aligned_size_misaligned_pointers(small, src_off, dst_off):
    """nbytes % 16 == 0 alone must not select 16-byte loads and stores."""
    nbytes = 4112
    dst = small.view(nbytes, offset=dst_off)
    src = dev_source()[src_off:src_off + nbytes]
    assert src.data_ptr() % 16 == src_off and dst.data_ptr() % 16 == dst_off
    bw.copy(dst, src)
    small.check(nbytes, ref_bytes(nbytes, src_off), offset=dst_off, what=(src_off, dst_off))


def test_copy_float_view_at_element_offset(small):
    """x[1:] of a float32 tensor: 4-byte-offset pointer, 16-multiple size."""
    n = 1025
    x = dev_source()[:4 * n].view(torch.float32)
    dst = small.view(4 * (n - 1)).view(torch.float32)
    assert (4 * (n - 1)) % 16 == 0 and x[1:].data_ptr() % 16 == 4
    bw.copy(dst, x[1:])
    small.check(4 * (n - 1), ref_bytes(4 * (n - 1), 4))


# 4. copy(), edge and rejection cases ----------------------------------------------------

def test_copy_empty_is_noop(small):
    dst = small.view(64)
    bw.copy(torch.empty(0, device="cuda"), torch.empty(0, device="cuda"))
    bw.copy(dst[:0], dev_source()[:0])
    bw.copy(dst[32:32], dev_source()[7:7])
    small.untouched()


def test_copy_same_tensor_is_allowed():
    for nbytes in (4112, 4099):  # vector and byte kernels
        t = dev_source()[:nbytes].clone()
        bw.copy(t, t)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), ref_bytes(nbytes))


def test_copy_rejections(small):
    dst = small.view(4096)
    src = dev_source()
    strided = torch.zeros(4096, 2, dtype=torch.uint8, device="cuda")[:, 0]
    bad = [
        lambda: bw.copy(dst[16:2064], dst[:2048]),  # partial overlap, dst after src
        lambda: bw.copy(dst[:2048], dst[16:2064]),  # partial overlap, dst before src
        lambda: bw.copy(dst[1:2048], dst[:2047]),  # the same through the byte path
        lambda: bw.copy(dst, src[:4080]),  # size mismatch
        lambda: bw.copy(dst[:4080], src[:4096]),
        lambda: bw.copy(dst, src[:4096].cpu()),  # CPU source
        lambda: bw.copy(torch.zeros(4096, dtype=torch.uint8), src[:4096]),  # CPU destination
        lambda: bw.copy(dst, strided),  # non-contiguous source
        lambda: bw.copy(strided, src[:4096]),  # non-contiguous destination
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    small.untouched()
    assert (strided.cpu() == 0).all()


def test_copy_cross_device_raises(small):
    if torch.cuda.device_count() < 2:
        pytest.skip(f"single-GPU box (device_count={torch.cuda.device_count()})")
    dst = small.view(4096)
    other = torch.zeros(4096, dtype=torch.uint8, device="cuda:1")
    with pytest.raises(RuntimeError):
        bw.copy(dst, other)
    with pytest.raises(RuntimeError):
        bw.copy_variant(dst, other)
    small.untouched()


# 5. read_sum ------------------------------------------------------------------------------

READ_BLOCKS = (0, 1, 3, 1536)
READ_N4 = shapes(3 * 256) + (DEFAULT_N4,)


def as_i32(x):
    return x - (1 << 32) if x & 0x80000000 else x


def test_read_sum_distinct_words():
    words = ref_words()
    for n4 in READ_N4:
        want = int(words[:4 * n4].astype(np.uint64).sum())
        src = dev_source()[:16 * n4]
        for blocks in READ_BLOCKS:
            got = bw.read_sum(src, blocks)
            assert isinstance(got, int) and 0 <= got < 2**64
            assert got == want, (n4, blocks, got, want)


def test_read_sum_all_ones_words():
    """Catches 32-bit accumulation and sign extension of the words."""
    buf = torch.full((BIG_BYTES,), 0xFF, dtype=torch.uint8, device="cuda")
    for n4 in READ_N4:
        for blocks in READ_BLOCKS:
            assert bw.read_sum(buf[:16 * n4], blocks) == 4 * n4 * (2**32 - 1), (n4, blocks)


@pytest.mark.parametrize("blocks", [3, 0])
def test_read_sum_single_word_positions(blocks):
    """One non-zero word in a zero buffer: a lane, wave or tail that the
    reduction drops returns 0 instead."""
    S = 3 * 256
    n4 = 9 * S + 77
    value = 0x80000001
    buf = torch.zeros(16 * n4, dtype=torch.uint8, device="cuda")
    words = buf.view(torch.int32)
    vectors = {
        "first vector": 0,
        "last vector": n4 - 1,
        "lane 63 of a wave": 63,
        "lane 64": 64,
        "last thread of a block": 255,
        "last thread of the grid": S - 1,
        "first vector of the second sweep": S,
    }
    for name, v in vectors.items():
        for j in range(4):
            words[4 * v + j] = as_i32(value)
            got = bw.read_sum(buf, blocks)
            words[4 * v + j] = 0
            assert got == value, (name, j, got)
    assert bw.read_sum(buf, blocks) == 0


def test_read_sum_resets_its_accumulator():
    src = dev_source()[:16 * 3073]
    want = int(ref_words()[:4 * 3073].astype(np.uint64).sum())
    assert bw.read_sum(src) == want
    assert bw.read_sum(src) == want


def test_read_sum_argument_checks():
    src = dev_source()
    bad = [
        lambda: bw.read_sum(src[:24]),
        lambda: bw.read_sum(src[4:4100]),
        lambda: bw.read_sum(src[:0]),
        lambda: bw.read_sum(src[:4096], -1),
        lambda: bw.read_sum(src[:4096], (1 << 20) + 1),
        lambda: bw.read_sum(src[:4096].cpu()),
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()


# 6. fill_word ---------------------------------------------------------------------------------

def want_fill(n4):
    return np.full(4 * n4, WORD, dtype=np.uint32).view(np.uint8)


@pytest.mark.parametrize("blocks", [0, 3, 640])
def test_fill_word(small, big, blocks):
    for n4 in ALL_N4:
        bw.fill_word(small.view(16 * n4), WORD, blocks)
        small.check(16 * n4, want_fill(n4), what=(blocks, n4))
    bw.fill_word(big.view(BIG_BYTES), WORD, blocks)
    big.check(BIG_BYTES, want_fill(DEFAULT_N4), what=(blocks, DEFAULT_N4))


def test_fill_word_argument_checks(small):
    dst = small.view(4096)
    bad = [
        lambda: bw.fill_word(dst[:24], WORD),
        lambda: bw.fill_word(dst[4:4084], WORD),
        lambda: bw.fill_word(dst[:0], WORD),
        lambda: bw.fill_word(dst, -1),
        lambda: bw.fill_word(dst, 1 << 32),
        lambda: bw.fill_word(dst, WORD, -1),
        lambda: bw.fill_word(dst, WORD, (1 << 20) + 1),
        lambda: bw.fill_word(torch.zeros(4096, dtype=torch.uint8), WORD),
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    small.untouched()


# 7. timed probes --------------------------------------------------------------------------------

MIB = 1 << 20


def finite_positive(x):
    return isinstance(x, float) and math.isfinite(x) and x > 0


@pytest.mark.parametrize("threads", [64, 256, 1024])
@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_copy_bw_gbps_runs_and_checks_itself(variant, threads):
    assert finite_positive(ext().copy_bw_gbps(MIB, 2, 0, True, variant, threads))


def test_copy_bw_gbps_temporal_kernel():
    assert finite_positive(ext().copy_bw_gbps(MIB, 2, 0, False))


def test_read_write_bw_gbps_run_and_check_themselves():
    assert finite_positive(bw.read_bw_gbps(MIB, iters=2))
    assert finite_positive(bw.write_bw_gbps(MIB, iters=2))


def test_timed_probes_back_to_back():
    """write, copy, write, read: each frees a buffer full of 0x01 that
    the caching allocator hands to the next one."""
    assert finite_positive(bw.write_bw_gbps(MIB, iters=2))
    assert finite_positive(bw.d2d_copy_bw_gbps(MIB, iters=2))
    assert finite_positive(bw.write_bw_gbps(MIB, iters=2))
    assert finite_positive(bw.read_bw_gbps(MIB, iters=2))


def test_timed_probes_argument_checks():
    e = ext()
    bad = [
        lambda: e.copy_bw_gbps(MIB, 2, 0, True, 4),  # variant
        lambda: e.copy_bw_gbps(MIB, 2, 0, True, 7),
        lambda: e.copy_bw_gbps(MIB, 2, 0, True, -1),
        lambda: e.copy_bw_gbps(MIB, 0),  # iters
        lambda: e.copy_bw_gbps(MIB, 2, -1),  # blocks
        lambda: e.copy_bw_gbps(MIB, 2, (1 << 20) + 1),
        lambda: e.copy_bw_gbps(24, 2),  # nbytes
        lambda: e.copy_bw_gbps(0, 2),
        lambda: e.copy_bw_gbps(MIB, 2, 0, True, 0, 96),  # threads
        lambda: e.copy_bw_gbps(MIB, 2, 0, True, 0, 2048),
    ]
    for fn in (e.read_bw_gbps, e.write_bw_gbps):
        bad += [
            lambda fn=fn: fn(MIB, 0),
            lambda fn=fn: fn(MIB, -3),
            lambda fn=fn: fn(MIB, 2, -1),
            lambda fn=fn: fn(MIB, 2, (1 << 20) + 1),
            lambda fn=fn: fn(24, 2),
            lambda fn=fn: fn(0, 2),
        ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
