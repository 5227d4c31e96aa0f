"""The integrity patterns' 64-bit vector index on a real MI355X.

Every other GPU test indexes the pattern from the buffer's own first
byte, so v < 2^26 there.  Here the kernels count from a caller-given
``first_vector`` just below each value at which the index arithmetic
changes, and one test uses a buffer large enough for the loop index and
the result accounting to pass 2^32 on their own.  Everything is compared
exactly with ``memcheck.reference_words`` at the same first vector.

Every small buffer a kernel touches is a view at a 16-byte offset into a
larger tensor filled with a sentinel byte; tests that write check the
guard bytes on both sides."""

import functools
import time

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import hostlink as hl
from kubegpu_amd.probe import memcheck as mc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
GUARD = 16  # bytes kept on each side of a buffer
SEEDS = (0, 0xDEADBEEF)
# B: where the arithmetic on the vector index changes
BOUNDARIES = (
    1 << 30,  # the walk family's u32 `v << 2` wraps
    1 << 32,  # lo32(v) wraps, hi32(v) goes 0 -> 1
    1 << 33,  # hi32(v) = 2: hi * golden wraps u32
    1 << 62,  # 4v wraps u64 in the reference
    0x7FFFFFFF << 32,  # the largest hi32 an int64 argument reaches
)
BACK = 700  # first_vector = B - BACK: B falls inside the first sweep,
#             mid-workgroup (700 = 2 * 256 + 188) and not on a wave boundary
# (nbytes, blocks): two full sweeps of a 3-workgroup grid plus one ragged
# vector; more than a MiB, ragged, with the default grid
SHAPES = ((16 * (2 * 768 + 1), 3), ((1 << 20) + 48, 0))
BIG = (8 << 20) + 16  # as tests/test_memcheck_gpu.py: ragged at every default grid
F32 = (1 << 32) - BACK


def id_of(x):
    if isinstance(x, tuple):
        return f"{x[0]}B-{x[1]}wg"
    return hex(x)


@functools.lru_cache(maxsize=None)
def ref(first, n_vectors, pattern, seed):
    """Shared, read-only reference words from vector `first`."""
    a = mc.reference_words(first, n_vectors, pattern, seed)
    a.setflags(write=False)
    return a


def or_all(masks):
    return functools.reduce(lambda a, b: a | b, masks, 0)


def as_i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


class GuardedDev:
    """nbytes of device memory with GUARD sentinel bytes either side."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8,
                                device="cuda")
        self.buf = self.whole[GUARD:GUARD + nbytes]

    def reset(self):
        self.whole.fill_(SENTINEL)

    def host(self):
        torch.cuda.synchronize()
        return self.whole.cpu().numpy()

    def words_and_guards(self):
        h = self.host()
        ok = bool((h[:GUARD] == SENTINEL).all() and (h[GUARD + self.nbytes:] == SENTINEL).all())
        return h[GUARD:GUARD + self.nbytes].view(np.uint32), ok

    def untouched(self):
        return bool((self.host() == SENTINEL).all())

    def write(self, want):
        """Upload reference words made by the CPU."""
        self.buf.copy_(torch.from_numpy(want.view(np.uint8).copy()))
        torch.cuda.synchronize()

    def flip(self, flips):
        w = self.buf.view(torch.int32)
        for idx, mask in flips.items():
            w[idx] ^= as_i32(mask)
        torch.cuda.synchronize()


class GuardedHost:
    """nbytes of pinned host memory with GUARD sentinel bytes either side."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.whole = hl.alloc(nbytes + 2 * GUARD)
        self.whole.fill_(SENTINEL)
        self.buf = self.whole[GUARD:GUARD + nbytes]
        self.bytes = self.whole.numpy()
        self.words = self.bytes[GUARD:GUARD + nbytes].view(np.uint32)

    def reset(self):
        self.whole.fill_(SENTINEL)

    def guards_intact(self):
        return bool((self.bytes[:GUARD] == SENTINEL).all()
                    and (self.bytes[GUARD + self.nbytes:] == SENTINEL).all())

    def untouched(self):
        return bool((self.bytes == SENTINEL).all())

    def write(self, want):
        self.words[:] = want

    def flip(self, flips):
        for idx, mask in flips.items():
            self.words[idx] ^= np.uint32(mask)


def seven_flips(nbytes, sweep_vectors):
    """The flip set of the other GPU test files: vector boundary,
    workgroup boundary, past the last full sweep, last word."""
    n_words = nbytes // 4
    flips = {
        0: 0x1,
        3: 0x80000000, 4: 0x00010000,  # vector boundary
        1023: 0x00000100, 1024: 0x00400000,  # workgroup boundary
        4 * (2 * sweep_vectors) + 1: 0x08000000,  # past the last full sweep
        n_words - 1: 0x00002000,
    }
    assert len(flips) == 7 and max(flips) == n_words - 1
    return flips


def expected_records(flips, first, pattern, seed, nbytes):
    """Buffer-relative word index; expected value from the reference at `first`."""
    r = ref(first, nbytes // 16, pattern, seed)
    return {(i, int(r[i]), int(r[i]) ^ m) for i, m in flips.items()}


CLEAN = (0, None, 0, [])


def as_tuple(r):
    return (r.mismatched_words, r.first_bad_offset, r.bad_bits_mask, r.records)


# 1. fill at a base ----------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=id_of)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=id_of)
def test_fill_at_base(boundary, shape):
    nbytes, blocks = shape
    first = boundary - BACK
    g = GuardedDev(nbytes)
    for pattern in range(6):
        for seed in SEEDS:
            g.reset()
            mc.fill_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            got, guards = g.words_and_guards()
            want = ref(first, nbytes // 16, pattern, seed)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (pattern, seed, int(np.argmax(got != want)))
            assert guards, (pattern, seed)


@pytest.mark.parametrize("shape", SHAPES, ids=id_of)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=id_of)
def test_hostlink_fill_at_base(boundary, shape):
    nbytes, blocks = shape
    first = boundary - BACK
    g = GuardedHost(nbytes)
    for pattern in range(6):
        for seed in SEEDS:
            g.reset()
            hl.fill_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            want = ref(first, nbytes // 16, pattern, seed)
            assert np.array_equal(g.words, want), \
                (pattern, seed, int(np.argmax(g.words != want)))
            assert g.guards_intact(), (pattern, seed)


# 2. verify at the same base ----------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=id_of)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=id_of)
def test_verify_clean_at_base(boundary, shape):
    """GPU-filled buffers verify clean at the base they were filled at."""
    nbytes, blocks = shape
    first = boundary - BACK
    g = GuardedDev(nbytes)
    ext = mc._ext()
    for pattern in range(6):
        for seed in SEEDS:
            mc.fill_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            r = mc.verify_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            assert as_tuple(r) == CLEAN, (pattern, seed)
            raw = ext.verify_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            assert tuple(raw) == (0, -1, 0, []), (pattern, seed)


@pytest.mark.parametrize("shape", SHAPES, ids=id_of)
@pytest.mark.parametrize("boundary", BOUNDARIES, ids=id_of)
def test_hostlink_verify_clean_at_base(boundary, shape):
    """CPU-written pinned buffers verify clean at the base the CPU used."""
    nbytes, blocks = shape
    first = boundary - BACK
    g = GuardedHost(nbytes)
    ext = hl._ext()
    for pattern in range(6):
        for seed in SEEDS:
            g.write(ref(first, nbytes // 16, pattern, seed))
            r = hl.verify_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
            assert as_tuple(r) == CLEAN, (pattern, seed)
            raw = ext.hostlink_verify(g.buf, pattern, seed, 0, blocks=blocks,
                                      first_vector=first)
            assert tuple(raw) == (0, -1, 0, []), (pattern, seed)
    assert g.guards_intact()


# 3. verify at a different base ----------------------------------------------------------
#
# F + 2^32 + n must stay within 2^63, which leaves out the last boundary.

@pytest.mark.parametrize("via", ["memcheck", "hostlink"])
@pytest.mark.parametrize("boundary", BOUNDARIES[:4], ids=id_of)
def test_verify_at_other_base_reports_the_reference_difference(boundary, via):
    nbytes, blocks = SHAPES[0]
    n = nbytes // 16
    first = boundary - BACK
    g = GuardedDev(nbytes) if via == "memcheck" else GuardedHost(nbytes)
    for other in (first + 1, first + (1 << 32)):
        for pattern in mc.PATTERNS:
            for seed in SEEDS:
                diff = ref(first, n, pattern, seed) ^ ref(other, n, pattern, seed)
                bad = np.nonzero(diff)[0]
                if pattern == "addr":  # stated first: the test cannot pass vacuously
                    assert len(bad) >= n
                if via == "memcheck":
                    mc.fill_pattern(g.buf, pattern, seed, blocks=blocks, first_vector=first)
                    r = mc.verify_pattern(g.buf, pattern, seed, max_records=4, blocks=blocks,
                                          first_vector=other)
                else:
                    g.write(ref(first, n, pattern, seed))
                    r = hl.verify_pattern(g.buf, pattern, seed, max_records=4, blocks=blocks,
                                          first_vector=other)
                where = (hex(other - first), pattern, seed)
                assert r.mismatched_words == len(bad), where
                assert r.bad_bits_mask == int(np.bitwise_or.reduce(diff)), where
                assert r.first_bad_offset == (int(bad[0]) * 4 if len(bad) else None), where
                assert len(r.records) == min(4, len(bad)), where
                want = ref(other, n, pattern, seed)
                got = ref(first, n, pattern, seed)
                for w, e, gt in r.records:
                    assert (e, gt) == (int(want[w]), int(got[w])) and e != gt, where


# 4. exact detection at a base ---------------------------------------------------------------

def check_exact_detection(g, verify, sweep_vectors):
    nbytes = g.nbytes
    n_words = nbytes // 4
    flips = seven_flips(nbytes, sweep_vectors)
    g.flip(flips)
    r = verify()
    assert r.mismatched_words == len(flips)
    assert r.first_bad_offset == 0
    assert r.bad_bits_mask == or_all(flips.values())
    assert set(r.records) == expected_records(flips, F32, "addr", 7, nbytes)
    assert len(r.records) == len(flips)

    # without word 0: atomicMin must settle on word 3 whichever block got there first
    g.flip({0: flips[0]})  # undo
    rest = {k: v for k, v in flips.items() if k != 0}
    r = verify()
    assert r.mismatched_words == len(rest)
    assert r.first_bad_offset == 3 * 4
    assert r.bad_bits_mask == or_all(rest.values())
    assert set(r.records) == expected_records(rest, F32, "addr", 7, nbytes)

    # only the tail vector bad: first offset is far from the start
    g.flip({k: v for k, v in rest.items() if k != n_words - 1})
    r = verify()
    assert r.mismatched_words == 1 and r.first_bad_offset == (n_words - 1) * 4
    assert set(r.records) == expected_records(
        {n_words - 1: flips[n_words - 1]}, F32, "addr", 7, nbytes)


def test_exact_detection_at_base():
    g = GuardedDev(BIG)
    mc.fill_pattern(g.buf, "addr", 7, first_vector=F32)
    # 1024 * 256: the verify-then-fill sweep; the verify grid is 1.5x that
    check_exact_detection(
        g, lambda: mc.verify_pattern(g.buf, "addr", 7, first_vector=F32), 1024 * 256)
    _, guards = g.words_and_guards()
    assert guards


def test_hostlink_exact_detection_at_base():
    """The CPU writes the pattern and makes the flips; the GPU only reads."""
    sweep_vectors = max(hl.default_blocks()) * 256
    g = GuardedHost(2 * sweep_vectors * 16 + 16)
    g.write(ref(F32, g.nbytes // 16, "addr", 7))
    check_exact_detection(
        g, lambda: hl.verify_pattern(g.buf, "addr", 7, first_vector=F32), sweep_vectors)
    assert g.guards_intact()


# 5. verify_then_fill at a base -------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=id_of)
@pytest.mark.parametrize("boundary", [1 << 30, 1 << 32], ids=id_of)
def test_verify_then_fill_every_pair_at_base(boundary, shape):
    nbytes, blocks = shape
    first = boundary - BACK
    g = GuardedDev(nbytes)
    for expect in range(6):
        for nxt in range(6):
            mc.fill_pattern(g.buf, expect, 9, blocks=blocks, first_vector=first)
            r = mc.verify_then_fill(g.buf, expect, nxt, 9, blocks=blocks, first_vector=first)
            assert as_tuple(r) == CLEAN, (expect, nxt)
            got, guards = g.words_and_guards()
            assert np.array_equal(got, ref(first, nbytes // 16, nxt, 9)), (expect, nxt)
            assert guards, (expect, nxt)


def test_verify_then_fill_reports_flips_at_base():
    n_words = BIG // 4
    g = GuardedDev(BIG)
    mc.fill_pattern(g.buf, "addr", 21, first_vector=F32)
    flips = {5: 0x40, 262144 * 4 + 2: 0x80000000, n_words - 2: 0x1}
    g.flip(flips)
    r = mc.verify_then_fill(g.buf, "addr", "walk0", 21, first_vector=F32)
    assert r.mismatched_words == 3
    assert r.first_bad_offset == 5 * 4
    assert r.bad_bits_mask == 0x80000041
    assert set(r.records) == expected_records(flips, F32, "addr", 21, BIG)
    got, guards = g.words_and_guards()
    assert np.array_equal(got, ref(F32, BIG // 16, "walk0", 21))
    assert guards
    assert as_tuple(mc.verify_pattern(g.buf, "walk0", 21, first_vector=F32)) == CLEAN


# 6. duplex with two different bases ------------------------------------------------------------

@pytest.mark.parametrize("read_blocks,write_blocks", [(0, 0), (1, 1), (3, 5)])
def test_duplex_with_two_bases(read_blocks, write_blocks):
    sweep_vectors = max(hl.default_blocks()) * 256
    read_n, write_n = 2 * sweep_vectors * 16 + 16, (1 << 20) + 48
    read_first, write_first = F32, (1 << 30) - BACK
    rd, wr = GuardedHost(read_n), GuardedHost(write_n)
    rd.write(ref(read_first, read_n // 16, "addr", 9))
    flips = seven_flips(read_n, sweep_vectors)
    rd.flip(flips)
    before = rd.bytes.copy()
    r = hl.duplex(rd.buf, "addr", wr.buf, "walk1", 9,
                  read_blocks=read_blocks, write_blocks=write_blocks,
                  read_first_vector=read_first, write_first_vector=write_first)
    # the written buffer is the write side's pattern at the write side's base
    assert np.array_equal(wr.words, ref(write_first, write_n // 16, "walk1", 9))
    assert wr.guards_intact()
    assert np.array_equal(rd.bytes, before)  # the read side was only read
    # the read side reports exactly the injected flips, at the read side's base
    assert r.mismatched_words == len(flips)
    assert r.first_bad_offset == 0
    assert r.bad_bits_mask == or_all(flips.values())
    assert set(r.records) == expected_records(flips, read_first, "addr", 9, read_n)
    # the two bases are not interchangeable: addr at the write side's base
    # is another pattern, so a kernel that swapped them could not pass above
    assert not np.array_equal(ref(read_first, 8, "addr", 9), ref(write_first, 8, "addr", 9))
    # clean read side; the write side gets addr at its own base
    rd.flip(flips)  # undo
    r = hl.duplex(rd.buf, "addr", wr.buf, "addr_inv", 9,
                  read_blocks=read_blocks, write_blocks=write_blocks,
                  read_first_vector=read_first, write_first_vector=write_first)
    assert as_tuple(r) == CLEAN
    assert np.array_equal(wr.words, ref(write_first, write_n // 16, "addr_inv", 9))
    assert rd.guards_intact() and wr.guards_intact()


# 7. argument checks --------------------------------------------------------------------------

def test_first_vector_argument_checks():
    nbytes = 4112
    n = nbytes // 16
    top = (1 << 63) - n  # the largest first_vector: first_vector + n == 2^63
    mext, hext = mc._ext(), hl._ext()
    d, h, other = GuardedDev(nbytes), GuardedHost(nbytes), GuardedHost(nbytes)
    # (entry point taking first_vector, wrapper taking first_vector)
    entries = [
        (lambda fv: mext.fill_pattern(d.buf, 0, 3, first_vector=fv),
         lambda fv: mc.fill_pattern(d.buf, 0, 3, first_vector=fv)),
        (lambda fv: mext.verify_pattern(d.buf, 0, 3, first_vector=fv),
         lambda fv: mc.verify_pattern(d.buf, 0, 3, first_vector=fv)),
        (lambda fv: mext.verify_then_fill(d.buf, 0, 4, 3, first_vector=fv),
         lambda fv: mc.verify_then_fill(d.buf, 0, 4, 3, first_vector=fv)),
        (lambda fv: hext.hostlink_fill(h.buf, 0, 3, 0, first_vector=fv),
         lambda fv: hl.fill_pattern(h.buf, 0, 3, first_vector=fv)),
        (lambda fv: hext.hostlink_verify(h.buf, 0, 3, 0, first_vector=fv),
         lambda fv: hl.verify_pattern(h.buf, 0, 3, first_vector=fv)),
        (lambda fv: hext.hostlink_duplex(h.buf, 0, other.buf, 0, 3, 0, read_first_vector=fv),
         lambda fv: hl.duplex(h.buf, 0, other.buf, 0, 3, read_first_vector=fv)),
        (lambda fv: hext.hostlink_duplex(other.buf, 0, h.buf, 0, 3, 0, write_first_vector=fv),
         lambda fv: hl.duplex(other.buf, 0, h.buf, 0, 3, write_first_vector=fv)),
    ]
    for entry, wrapper in entries:
        with pytest.raises(RuntimeError, match="negative"):
            entry(-1)
        with pytest.raises(ValueError, match="first_vector"):
            wrapper(-1)
        for call in (entry, wrapper):
            with pytest.raises(RuntimeError, match="2\\^63"):
                call(top + 1)
    torch.cuda.synchronize()
    # no rejected call touched a buffer
    assert d.untouched() and h.untouched() and other.untouched()

    # the largest base is accepted and matches the reference
    want = {p: ref(top, n, p, 3) for p in (0, 4, 5)}
    mext.fill_pattern(d.buf, 0, 3, first_vector=top)
    got, guards = d.words_and_guards()
    assert np.array_equal(got, want[0]) and guards
    assert tuple(mext.verify_pattern(d.buf, 0, 3, first_vector=top)) == (0, -1, 0, [])
    assert tuple(mext.verify_then_fill(d.buf, 0, 4, 3, first_vector=top)) == (0, -1, 0, [])
    got, guards = d.words_and_guards()
    assert np.array_equal(got, want[4]) and guards
    hext.hostlink_fill(h.buf, 0, 3, 0, first_vector=top)
    assert np.array_equal(h.words, want[0]) and h.guards_intact()
    assert tuple(hext.hostlink_verify(h.buf, 0, 3, 0, first_vector=top)) == (0, -1, 0, [])
    # duplex: both sides at the top; h is read (addr), other is written (walk0)
    raw = hext.hostlink_duplex(h.buf, 0, other.buf, 5, 3, 0, read_first_vector=top,
                               write_first_vector=top)
    assert tuple(raw) == (0, -1, 0, [])
    assert np.array_equal(other.words, want[5]) and other.guards_intact()
    # one vector further down is a different pattern: the base was used
    bad = mc.verify_pattern(d.buf, 4, 3, max_records=0, first_vector=top - 1)
    assert bad.mismatched_words == n * 4


# 8. one real large buffer ------------------------------------------------------------------------

LARGE = (1 << 34) + (1 << 16)  # vector 2^30 and word index 2^32 lie inside
WINDOW = 4096


def test_word_index_past_2_32():
    """The loop index, `base = i * 4`, Tally.first, the u64 atomicMin and
    the record's word index beyond 2^32, with first_vector = 0.

    Measured on an MI355X: 0.50 s for the whole test, 0.48 s of it the
    16 GiB allocation; the four passes over the buffer take milliseconds."""
    free = torch.cuda.mem_get_info()[0]
    if free < LARGE + (2 << 30):
        pytest.skip(f"needs {LARGE + (2 << 30)} bytes of free VRAM, {free} are free")
    t0 = time.perf_counter()
    buf = torch.empty(LARGE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t_alloc = time.perf_counter() - t0
    n_words = LARGE // 4
    assert n_words > (1 << 32) + 1 and LARGE // 16 > 1 << 30
    starts = (0, (1 << 34) - WINDOW // 2, LARGE - WINDOW)

    def check_windows(pattern):
        for a in starts:
            got = buf[a:a + WINDOW].cpu().numpy().view(np.uint32)
            want = mc.reference_words(a // 16, WINDOW // 16, pattern, 0)
            assert np.array_equal(got, want), (pattern, a, int(np.argmax(got != want)))

    try:
        mc.fill_pattern(buf, "walk1", 0)
        check_windows("walk1")
        assert as_tuple(mc.verify_pattern(buf, "walk1", 0)) == CLEAN

        flips = {(1 << 32) + 1: 0x00000400, n_words - 1: 0x20000000}
        for idx, mask in flips.items():
            buf[4 * idx:4 * idx + 4].view(torch.int32)[0] ^= as_i32(mask)
        torch.cuda.synchronize()
        # walk1: word k holds bit k mod 32
        records = {(k, 1 << (k % 32), (1 << (k % 32)) ^ m) for k, m in flips.items()}

        r = mc.verify_pattern(buf, "walk1", 0)
        assert r.mismatched_words == 2
        assert r.first_bad_offset == ((1 << 32) + 1) * 4
        assert r.bad_bits_mask == 0x20000400
        assert set(r.records) == records and len(r.records) == 2

        r = mc.verify_then_fill(buf, "walk1", "addr", 0)
        assert r.mismatched_words == 2
        assert r.first_bad_offset == ((1 << 32) + 1) * 4
        assert r.bad_bits_mask == 0x20000400
        assert set(r.records) == records and len(r.records) == 2
        check_windows("addr")
        torch.cuda.synchronize()
        print(f"16 GiB + 64 KiB: allocation {t_alloc:.3f} s, "
              f"whole test {time.perf_counter() - t0:.3f} s")
    finally:
        del buf
        torch.cuda.empty_cache()
