"""Host-link kernels on a real MI355X: the GPU fills and verifies pinned
host memory against the numpy reference, exact mismatch accounting with
flips made by the CPU, the duplex kernel, the pointer guard, hostlink()
end to end, the child process and CLI.

Every buffer a kernel touches is a view at a 16-byte offset into a larger
pinned tensor filled with a sentinel byte, and every test that writes
checks the guard bytes on both sides."""

import functools
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import hostlink as hl
from kubegpu_amd.probe import memcheck as mc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A
GUARD = 16  # bytes kept on each side of a buffer
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def grids():
    return hl.default_blocks()


@functools.lru_cache(maxsize=None)
def big():
    """Two full sweeps of the larger default grid plus one ragged vector."""
    return 2 * max(grids()) * 256 * 16 + 16


@functools.lru_cache(maxsize=None)
def ref(n_vectors, pattern, seed):
    """Shared, read-only reference words from v = 0."""
    a = mc.reference_words(0, n_vectors, pattern, seed)
    a.setflags(write=False)
    return a


class Guarded:
    """nbytes of pinned host memory with GUARD sentinel bytes either side."""

    def __init__(self, nbytes):
        self.nbytes = nbytes
        self.whole = hl.alloc(nbytes + 2 * GUARD)
        self.whole.fill_(SENTINEL)
        self.buf = self.whole[GUARD:GUARD + nbytes]
        self.bytes = self.whole.numpy()
        self.words = self.bytes[GUARD:GUARD + nbytes].view(np.uint32)

    def guards_intact(self):
        return bool((self.bytes[:GUARD] == SENTINEL).all()
                    and (self.bytes[GUARD + self.nbytes:] == SENTINEL).all())

    def untouched(self):
        return bool((self.bytes == SENTINEL).all())

    def write(self, pattern, seed):
        """The CPU writes the reference into the buffer."""
        self.words[:] = ref(self.nbytes // 16, pattern, seed)

    def flip(self, flips):
        """The CPU XORs words: {word_index: mask}."""
        for idx, mask in flips.items():
            self.words[idx] ^= np.uint32(mask)


def expected_records(flips, pattern, seed, nbytes):
    r = ref(nbytes // 16, pattern, seed)
    return {(i, int(r[i]), int(r[i]) ^ m) for i, m in flips.items()}


def or_all(masks):
    return functools.reduce(lambda a, b: a | b, masks)


def test_alloc_and_default_grids():
    rb, wb = grids()
    assert 1 <= rb <= 1024 and 1 <= wb <= 1024
    assert big() <= (8 << 20) + 16
    h = hl.alloc(4096)
    assert h.device.type == "cpu" and h.dtype == torch.uint8 and h.shape == (4096,)
    assert h.is_contiguous() and h.data_ptr() % 16 == 0
    h.numpy()[:] = 7  # writable from the CPU through the numpy view
    assert int(h.sum()) == 7 * 4096
    with pytest.raises(RuntimeError):
        hl.alloc(0)


# 1. fill: the CPU checks what the GPU wrote ---------------------------------------

@pytest.mark.parametrize("nbytes,blocks", [
    (16, 0), (4080, 0), (4112, 0), ((1 << 20) + 48, 0), ((1 << 20) + 48, 3), (None, 0),
])
def test_fill_matches_reference(nbytes, blocks):
    nbytes = big() if nbytes is None else nbytes
    g = Guarded(nbytes)
    for pattern in range(6):
        for seed in SEEDS:
            g.whole.fill_(SENTINEL)
            hl.fill_pattern(g.buf, pattern, seed, blocks=blocks)
            want = ref(nbytes // 16, pattern, seed)
            assert g.words.shape == want.shape
            assert np.array_equal(g.words, want), \
                (pattern, seed, int(np.argmax(g.words != want)))
            assert g.guards_intact(), (pattern, seed)


# 2. verify: the GPU checks what the CPU wrote --------------------------------------

@pytest.mark.parametrize("nbytes,blocks", [
    (16, 0), (4080, 0), (4112, 0), ((1 << 20) + 48, 0), ((1 << 20) + 48, 3), (None, 0),
])
def test_clean_verify(nbytes, blocks):
    nbytes = big() if nbytes is None else nbytes
    g = Guarded(nbytes)
    for pattern in mc.PATTERNS:
        for seed in SEEDS:
            g.write(pattern, seed)
            r = hl.verify_pattern(g.buf, pattern, seed, blocks=blocks)
            assert (r.mismatched_words, r.first_bad_offset, r.bad_bits_mask, r.records) == \
                (0, None, 0, []), (pattern, seed)
    raw = hl._ext().hostlink_verify(g.buf, mc.pattern_id("walk0"), SEEDS[-1], 0)
    assert tuple(raw) == (0, -1, 0, [])
    # a pattern that was NOT written is seen as wrong in every word
    r = hl.verify_pattern(g.buf, "walk1", SEEDS[-1], max_records=4, blocks=blocks)
    assert r.mismatched_words == nbytes // 4 and r.first_bad_offset == 0
    assert r.bad_bits_mask == 0xFFFFFFFF and len(r.records) == min(4, nbytes // 4)


# 3. exact detection ------------------------------------------------------------------

def flips_for(nbytes):
    n_words = nbytes // 4
    sweep_vectors = max(grids()) * 256
    flips = {
        0: 0x1,
        3: 0x80000000, 4: 0x00010000,  # vector boundary
        1023: 0x00000100, 1024: 0x00400000,  # workgroup boundary
        4 * (2 * sweep_vectors) + 1: 0x08000000,  # past the last full sweep
        n_words - 1: 0x00002000,
    }
    assert len(flips) == 7 and max(flips) == n_words - 1
    return flips


def test_exact_detection():
    nbytes = big()
    n_words = nbytes // 4
    flips = flips_for(nbytes)
    g = Guarded(nbytes)
    g.write("addr", 7)
    g.flip(flips)
    r = hl.verify_pattern(g.buf, "addr", 7)
    assert r.mismatched_words == len(flips)
    assert r.first_bad_offset == 0
    assert r.bad_bits_mask == or_all(flips.values())
    assert set(r.records) == expected_records(flips, "addr", 7, nbytes)
    assert len(r.records) == len(flips)

    # without word 0: atomicMin must settle on word 3 whichever block got there first
    g.flip({0: flips[0]})  # undo
    rest = {k: v for k, v in flips.items() if k != 0}
    r = hl.verify_pattern(g.buf, "addr", 7)
    assert r.mismatched_words == len(rest)
    assert r.first_bad_offset == 3 * 4
    assert r.bad_bits_mask == or_all(rest.values())
    assert set(r.records) == expected_records(rest, "addr", 7, nbytes)

    # only the tail vector bad: first offset is far from the start
    g.flip({k: v for k, v in rest.items() if k != n_words - 1})
    r = hl.verify_pattern(g.buf, "addr", 7)
    assert r.mismatched_words == 1 and r.first_bad_offset == (n_words - 1) * 4
    assert g.guards_intact()


def test_two_bits_in_one_word_count_once():
    nbytes = big()
    g = Guarded(nbytes)
    g.write("addr", 7)
    word = nbytes // 4 // 3
    flips = {word: 0x00100004}
    g.flip(flips)
    r = hl.verify_pattern(g.buf, "addr", 7)
    assert r.mismatched_words == 1
    assert r.first_bad_offset == word * 4
    assert r.bad_bits_mask == 0x00100004
    assert set(r.records) == expected_records(flips, "addr", 7, nbytes)


def test_record_cap():
    nbytes = big()
    g = Guarded(nbytes)
    g.write("walk1", 3)
    rng = np.random.default_rng(4)
    idx = sorted(int(i) for i in rng.choice(nbytes // 4, size=40, replace=False))
    flips = {i: 1 << (k % 32) for k, i in enumerate(idx)}
    g.flip(flips)
    r = hl.verify_pattern(g.buf, "walk1", 3, max_records=16)
    assert r.mismatched_words == 40
    assert r.first_bad_offset == idx[0] * 4
    assert len(r.records) == 16
    assert set(r.records) <= expected_records(flips, "walk1", 3, nbytes)
    assert len({w for w, _, _ in r.records}) == 16
    # max_records=0 keeps the count and drops the log
    r0 = hl.verify_pattern(g.buf, "walk1", 3, max_records=0)
    assert r0.mismatched_words == 40 and r0.records == []
    assert r0.first_bad_offset == idx[0] * 4


# 4. duplex ---------------------------------------------------------------------------

@pytest.mark.parametrize("read_blocks,write_blocks", [(0, 0), (1, 1), (3, 5)])
def test_duplex(read_blocks, write_blocks):
    read_n, write_n = big(), (1 << 20) + 48  # both ragged, different sizes
    rd, wr = Guarded(read_n), Guarded(write_n)
    rd.write("checker", 9)
    flips = flips_for(read_n)
    rd.flip(flips)
    before = rd.bytes.copy()
    r = hl.duplex(rd.buf, "checker", wr.buf, "walk1", 9,
                  read_blocks=read_blocks, write_blocks=write_blocks)
    # the written buffer, checked by the CPU, each side indexed from its own byte 0
    assert np.array_equal(wr.words, ref(write_n // 16, "walk1", 9))
    assert wr.guards_intact()
    assert np.array_equal(rd.bytes, before)  # the read side was only read
    # the read side reports exactly the injected flips
    assert r.mismatched_words == len(flips)
    assert r.first_bad_offset == 0
    assert r.bad_bits_mask == or_all(flips.values())
    assert set(r.records) == expected_records(flips, "checker", 9, read_n)
    # clean read side, the other way round in size, another pattern pair
    rd.flip(flips)  # undo
    wr.write("addr_inv", 9)
    r = hl.duplex(wr.buf, "addr_inv", rd.buf, "walk0", 9,
                  read_blocks=read_blocks, write_blocks=write_blocks)
    assert (r.mismatched_words, r.first_bad_offset, r.bad_bits_mask, r.records) == \
        (0, None, 0, [])
    assert np.array_equal(rd.words, ref(read_n // 16, "walk0", 9))
    assert rd.guards_intact() and wr.guards_intact()


def test_duplex_every_pattern_pair():
    """All 36 (read, write) pattern pairs through the nested family
    dispatch: a wrong family or a swapped pair shows as mismatches on the
    read side or as wrong words on the write side.  One workgroup per
    role, both buffers ragged past one 256-thread stride, sizes differ."""
    read_n, write_n = 4096 + 48, 4096 + 16
    rd, wr = Guarded(read_n), Guarded(write_n)
    for read_pattern in mc.PATTERNS:
        for write_pattern in mc.PATTERNS:
            pair = (read_pattern, write_pattern)
            rd.write(read_pattern, 9)
            wr.whole.fill_(SENTINEL)
            r = hl.duplex(rd.buf, read_pattern, wr.buf, write_pattern, 9,
                          read_blocks=1, write_blocks=1)
            assert (r.mismatched_words, r.first_bad_offset, r.bad_bits_mask, r.records) == \
                (0, None, 0, []), pair
            assert np.array_equal(wr.words, ref(write_n // 16, write_pattern, 9)), pair
            assert rd.guards_intact() and wr.guards_intact(), pair


def test_duplex_rejects_overlap():
    g = Guarded(4096)
    cases = [
        (g.buf, g.buf),  # the same range
        (g.buf[:2048], g.buf[1024:3072]),  # partial overlap
        (g.buf[1024:3072], g.buf[:2048]),
        (g.buf, g.buf[2048:2064]),  # one inside the other
        (g.buf[4080:], g.buf),  # the last vector
    ]
    for rd, wr in cases:
        with pytest.raises(RuntimeError, match="overlap"):
            hl.duplex(rd, "addr", wr, "addr", 0)
    assert g.untouched()
    # two halves that only touch are fine
    hl.fill_pattern(g.buf[:2048], "addr", 0)
    r = hl.duplex(g.buf[:2048], "addr", g.buf[2048:], "checker", 0)
    assert r.ok
    assert np.array_equal(g.words[512:], ref(128, "checker", 0))
    assert g.guards_intact()


# 5. argument checks ----------------------------------------------------------------------
#
# The order of the host-side checks in csrc/hostlink.hip: pattern, seed,
# blocks and max_records first, then check_host (CPU, contiguous, size,
# alignment, hipPointerGetAttributes on the first and last byte,
# hipHostGetDevicePointer), all before the result block is allocated and
# before the one launch at the end of each entry point.

def test_argument_checks():
    ext = hl._ext()
    g = Guarded(4096)
    other = Guarded(64)
    calls = [
        lambda b, p: ext.hostlink_fill(b, p, 0, 0),
        lambda b, p: ext.hostlink_verify(b, p, 0, 0),
        lambda b, p: ext.hostlink_duplex(b, p, other.buf, 0, 0, 0),
        lambda b, p: ext.hostlink_duplex(other.buf, 0, b, p, 0, 0),
    ]
    pageable = torch.full((4096,), SENTINEL, dtype=torch.uint8)
    assert not pageable.is_pinned()
    on_gpu = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    bad_bufs = [
        pageable,
        on_gpu,
        g.whole[8:8 + 64],  # misaligned view of pinned memory
        g.buf[:40],  # nbytes % 16 != 0
        g.whole.view(torch.int32)[::2],  # non-contiguous
    ]
    for call in calls:
        for b in bad_bufs:
            with pytest.raises(RuntimeError):
                call(b, 0)
        for bad_pattern in (6, -1):
            with pytest.raises(RuntimeError):
                call(g.buf, bad_pattern)
    with pytest.raises(RuntimeError):
        ext.hostlink_fill(g.buf, 0, 1 << 32, 0)  # seed
    with pytest.raises(RuntimeError):
        ext.hostlink_fill(g.buf, 0, 0, 99)  # device
    with pytest.raises(RuntimeError):
        ext.hostlink_verify(g.buf, 0, 0, 0, 4097)  # max_records
    with pytest.raises(RuntimeError):
        ext.hostlink_fill(g.buf, 0, 0, 0, -1)  # blocks
    with pytest.raises(ValueError):
        hl.fill_pattern(g.buf, 6)
    torch.cuda.synchronize()
    assert g.untouched() and other.untouched()
    assert (pageable == SENTINEL).all() and (on_gpu.cpu() == SENTINEL).all()


def test_torch_pinned_tensor_is_accepted():
    n = 4112
    whole = torch.empty(n + 2 * GUARD, dtype=torch.uint8, pin_memory=True)
    assert whole.is_pinned()
    whole.fill_(SENTINEL)
    buf = whole[GUARD:GUARD + n]
    hl.fill_pattern(buf, "addr", 5)
    host = whole.numpy()
    assert np.array_equal(host[GUARD:GUARD + n].view(np.uint32), ref(n // 16, "addr", 5))
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all()
    assert hl.verify_pattern(buf, "addr", 5).ok
    host[GUARD:GUARD + n].view(np.uint32)[77] ^= np.uint32(0x10)
    r = hl.verify_pattern(buf, "addr", 5)
    assert r.mismatched_words == 1 and r.first_bad_offset == 77 * 4


# 6. hostlink() -----------------------------------------------------------------------------

FIGURES = ("kernel_h2d_gbps", "kernel_d2h_gbps", "copy_h2d_gbps", "copy_d2h_gbps",
           "duplex_gbps")


def test_hostlink_clean():
    r = hl.hostlink(nbytes=8 << 20)
    assert r.ok is True and r.passes == 8
    assert r.mismatched_words == 0 and r.cpu_sample_mismatches == 0
    assert r.first_bad_offset is None and r.records == [] and r.records_dropped == 0
    assert r.bytes_tested == 8 << 20 and r.elapsed_s > 0
    d = json.loads(json.dumps(r.to_dict()))
    for name in FIGURES:
        print(f"hostlink 8 MiB: {name} = {d[name]:.2f} GB/s")
        assert math.isfinite(d[name]) and d[name] > 0, name
    assert d["below_floor"] is False and d["min_gbps"] == 0.0
    assert d["link"] is None or set(d["link"]) == {
        "speed_gts", "max_speed_gts", "width", "max_width", "numa_node", "downtrained"}


def test_hostlink_reports_a_flip_after_the_d2h_copy():
    word = 123457

    def corrupt(pass_index, view):
        if pass_index == 3:  # pass 4 reads it
            view.view(np.uint32)[word] ^= np.uint32(0x4)

    r = hl.hostlink(nbytes=8 << 20, seed=5, _after_pass=corrupt)
    assert r.ok is False and r.passes == 8
    assert r.mismatched_words == 1 and r.cpu_sample_mismatches == 0
    assert r.first_bad_offset == word * 4 and r.bad_bits_mask == 0x4
    assert r.records_dropped == 0
    (rec,) = r.records
    want = int(mc.reference_words(word // 4, 1, "addr_inv", 5)[word % 4])
    assert rec == {"pass": 4, "path": "kernel_read", "offset": word * 4,
                   "word_index": word, "expected": want, "got": want ^ 0x4}
    json.dumps(r.to_dict())


def test_hostlink_flip_after_pass_0_is_seen_by_cpu_and_gpu():
    word = 517  # inside the first 4 KiB

    def corrupt(pass_index, view):
        if pass_index == 0:
            view.view(np.uint32)[word] ^= np.uint32(0x00020000)

    r = hl.hostlink(nbytes=8 << 20, seed=9, _after_pass=corrupt)
    assert r.ok is False
    assert r.cpu_sample_mismatches == 1
    # the GPU's loads (pass 1) see it, and so does the copy into HBM (pass 2)
    assert r.mismatched_words == 2
    assert r.first_bad_offset == word * 4 and r.bad_bits_mask == 0x00020000
    want = int(mc.reference_words(word // 4, 1, "addr", 9)[word % 4])
    assert [(x["pass"], x["path"]) for x in r.records] == [
        (0, "kernel_write"), (1, "kernel_read"), (2, "copy_h2d")]
    for rec in r.records:
        assert (rec["offset"], rec["word_index"]) == (word * 4, word)
        assert (rec["expected"], rec["got"]) == (want, want ^ 0x00020000)
    assert r.records_dropped == 0


def test_hostlink_upper_half_offsets_are_from_the_buffer_start():
    nbytes = 8 << 20
    word = nbytes // 4 - 3  # in the upper half, which pass 6 fills and pass 7 reads

    def corrupt(pass_index, view):
        if pass_index == 6:
            view.view(np.uint32)[word] ^= np.uint32(0x1)

    r = hl.hostlink(nbytes=nbytes, seed=2, _after_pass=corrupt)
    assert r.mismatched_words == 1 and r.first_bad_offset == word * 4
    (rec,) = r.records
    local = word - nbytes // 8  # word index from the upper half's own first byte
    want = int(mc.reference_words(local // 4, 1, "walk1", 2)[local % 4])
    assert rec == {"pass": 7, "path": "kernel_read", "offset": word * 4,
                   "word_index": word, "expected": want, "got": want ^ 0x1}


def test_hostlink_floor_is_reported_and_leaves_ok_alone():
    r = hl.hostlink(nbytes=8 << 20, min_gbps=1e9)
    assert r.below_floor is True and r.min_gbps == 1e9
    assert r.ok is True and r.mismatched_words == 0


# 7. child process and CLI ---------------------------------------------------------------------

def check_record(rec, nbytes):
    assert rec["ok"] is True and rec["passes"] == 8 and rec["bytes_tested"] == nbytes
    assert rec["mismatched_words"] == 0 and rec["cpu_sample_mismatches"] == 0
    assert rec["records"] == [] and rec["below_floor"] is False
    for name in FIGURES:
        assert math.isfinite(rec[name]) and rec[name] > 0, name
    assert "link" in rec


def test_hostlink_child_process():
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.hostlink",
         "--device", "0", "--bytes", "67108864"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    check_record(rec, 67108864)
    assert rec["device"] == 0


def test_amddevs_hostlink_cli():
    from kubegpu_amd.discovery import default_backend

    n_gpus = len(default_backend().get_devices().devices)
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs",
         "--hostlink", "--bytes", "67108864"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    results = json.loads(res.stdout)
    assert len(results) == n_gpus >= 1
    for rec in results.values():
        check_record(rec, 67108864)
        assert rec["exit_code"] == 0
