"""HBM integrity kernels on a real MI355X: fill / verify /
verify_then_fill against the numpy reference, exact mismatch
accounting, memcheck() end to end, the child process and CLI."""

import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from kubegpu_amd.probe import memcheck as mc

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = 0x5A  # byte the buffers hold before a fill
BIG = (8 << 20) + 16  # full grid sweeps plus one ragged vector at every default grid
SEEDS = (0, 0xDEADBEEF)


@functools.lru_cache(maxsize=None)
def ref(n_vectors, pattern, seed):
    """Shared, read-only reference words from v = 0."""
    a = mc.reference_words(0, n_vectors, pattern, seed)
    a.setflags(write=False)
    return a


def new_buf(nbytes):
    return torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device="cuda")


def words(buf):
    """Device buffer -> host uint32 words."""
    return buf.view(torch.int32).cpu().numpy().view(np.uint32)


def as_i32(x):
    x &= 0xFFFFFFFF
    return x - (1 << 32) if x & 0x80000000 else x


def inject(buf, flips):
    """XOR words of the test's own tensor: {word_index: mask}."""
    w = buf.view(torch.int32)
    for idx, mask in flips.items():
        w[idx] ^= as_i32(mask)
    torch.cuda.synchronize()


def expected_records(flips, pattern, seed, nbytes):
    r = ref(nbytes // 16, pattern, seed)
    return {(i, int(r[i]), int(r[i]) ^ m) for i, m in flips.items()}


# 1. fill against the reference ------------------------------------------------

@pytest.mark.parametrize("nbytes,blocks", [
    (16, 0), (4080, 0), (4112, 0), ((1 << 20) + 48, 0), ((1 << 20) + 48, 3), (BIG, 0),
])
def test_fill_matches_reference(nbytes, blocks):
    buf = new_buf(nbytes)
    for pattern in range(6):
        for seed in SEEDS:
            buf.fill_(SENTINEL)
            mc.fill_pattern(buf, pattern, seed, blocks=blocks)
            torch.cuda.synchronize()
            got = words(buf)
            want = ref(nbytes // 16, pattern, seed)
            assert got.shape == want.shape
            assert np.array_equal(got, want), (pattern, seed, int(np.argmax(got != want)))


def test_fill_view_at_offset_starts_at_vector_zero():
    n = 4112
    big = new_buf(16 + n + 64)
    view = big[16:16 + n]
    for pattern in range(6):
        big.fill_(SENTINEL)
        mc.fill_pattern(view, pattern, 0xDEADBEEF)
        torch.cuda.synchronize()
        host = big.cpu().numpy()
        assert np.array_equal(host[16:16 + n].view(np.uint32), ref(n // 16, pattern, 0xDEADBEEF))
        assert (host[:16] == SENTINEL).all() and (host[16 + n:] == SENTINEL).all()


# 2. clean verify ----------------------------------------------------------------

@pytest.mark.parametrize("nbytes", [4080, BIG])
def test_clean_verify(nbytes):
    buf = new_buf(nbytes)
    for pattern in mc.PATTERNS:
        mc.fill_pattern(buf, pattern, 11)
        r = mc.verify_pattern(buf, pattern, 11)
        assert (r.mismatched_words, r.first_bad_offset, r.bad_bits_mask, r.records) == \
            (0, None, 0, [])
        raw = mc._ext().verify_pattern(buf, mc.pattern_id(pattern), 11)
        assert tuple(raw) == (0, -1, 0, [])
    # a pattern that was NOT written is seen as wrong everywhere
    r = mc.verify_pattern(buf, "checker", 11, max_records=4)
    assert r.mismatched_words == nbytes // 4 and len(r.records) == 4


# 3. exact detection ----------------------------------------------------------------

N_WORDS = BIG // 4  # 2097156
SWEEP_VECTORS = 1024 * 256  # verify-then-fill grid; the verify grid is 1.5x that
FLIPS = {
    0: 0x1,
    3: 0x80000000, 4: 0x00010000,  # vector boundary
    1023: 0x00000100, 1024: 0x00400000,  # block boundary
    4 * (2 * SWEEP_VECTORS) + 1: 0x08000000,  # beyond the last full sweep of either
    N_WORDS - 1: 0x00002000,
}


def test_exact_detection():
    assert N_WORDS == 2097156 and 4 * (2 * SWEEP_VECTORS) + 1 < N_WORDS - 1
    buf = new_buf(BIG)
    mc.fill_pattern(buf, "addr", 7)
    inject(buf, FLIPS)
    r = mc.verify_pattern(buf, "addr", 7)
    assert r.mismatched_words == len(FLIPS)
    assert r.first_bad_offset == 0
    assert r.bad_bits_mask == functools.reduce(lambda a, b: a | b, FLIPS.values())
    assert set(r.records) == expected_records(FLIPS, "addr", 7, BIG)
    assert len(r.records) == len(FLIPS)

    # without word 0: atomicMin must settle on word 3 whichever block got there first
    inject(buf, {0: FLIPS[0]})  # undo
    rest = {k: v for k, v in FLIPS.items() if k != 0}
    r = mc.verify_pattern(buf, "addr", 7)
    assert r.mismatched_words == len(rest)
    assert r.first_bad_offset == 3 * 4
    assert r.bad_bits_mask == functools.reduce(lambda a, b: a | b, rest.values())
    assert set(r.records) == expected_records(rest, "addr", 7, BIG)

    # only the tail vector bad: first offset is far from the start
    inject(buf, {k: v for k, v in rest.items() if k != N_WORDS - 1})
    r = mc.verify_pattern(buf, "addr", 7)
    assert r.mismatched_words == 1 and r.first_bad_offset == (N_WORDS - 1) * 4


def test_two_bits_in_one_word_count_once():
    buf = new_buf(BIG)
    mc.fill_pattern(buf, "addr", 7)
    flips = {777777: 0x00100004}
    inject(buf, flips)
    r = mc.verify_pattern(buf, "addr", 7)
    assert r.mismatched_words == 1
    assert r.first_bad_offset == 777777 * 4
    assert r.bad_bits_mask == 0x00100004
    assert set(r.records) == expected_records(flips, "addr", 7, BIG)


# 4. record cap ------------------------------------------------------------------------

def test_record_cap():
    buf = new_buf(BIG)
    mc.fill_pattern(buf, "walk1", 3)
    rng = np.random.default_rng(4)
    idx = sorted(int(i) for i in rng.choice(N_WORDS, size=40, replace=False))
    flips = {i: 1 << (k % 32) for k, i in enumerate(idx)}
    # every mask must actually change the word (walk1 has one bit set; XOR always does)
    inject(buf, flips)
    r = mc.verify_pattern(buf, "walk1", 3, max_records=16)
    assert r.mismatched_words == 40
    assert r.first_bad_offset == idx[0] * 4
    assert len(r.records) == 16
    assert set(r.records) <= expected_records(flips, "walk1", 3, BIG)
    assert len({w for w, _, _ in r.records}) == 16
    # max_records=0 keeps the count and drops the log
    r0 = mc.verify_pattern(buf, "walk1", 3, max_records=0)
    assert r0.mismatched_words == 40 and r0.records == []


# 5. verify_then_fill ------------------------------------------------------------------

def test_verify_then_fill():
    buf = new_buf(BIG)
    mc.fill_pattern(buf, "addr", 21)
    flips = {5: 0x40, 262144 * 4 + 2: 0x80000000, N_WORDS - 2: 0x1}
    inject(buf, flips)
    r = mc.verify_then_fill(buf, "addr", "addr_inv", 21)
    assert r.mismatched_words == 3
    assert r.first_bad_offset == 5 * 4
    assert r.bad_bits_mask == 0x80000041
    assert set(r.records) == expected_records(flips, "addr", 21, BIG)
    assert np.array_equal(words(buf), ref(BIG // 16, "addr_inv", 21))
    clean = mc.verify_pattern(buf, "addr_inv", 21)
    assert clean.ok and clean.first_bad_offset is None and clean.records == []


def test_verify_then_fill_every_family_pair():
    nbytes = (1 << 20) + 48
    buf = new_buf(nbytes)
    for expect in range(6):
        for nxt in range(6):
            mc.fill_pattern(buf, expect, 9)
            r = mc.verify_then_fill(buf, expect, nxt, 9)
            assert r.ok, (expect, nxt)
            assert np.array_equal(words(buf), ref(nbytes // 16, nxt, 9)), (expect, nxt)


# 6. argument checks -------------------------------------------------------------------

def test_argument_checks():
    ext = mc._ext()
    good = new_buf(64)
    calls = [
        lambda b, p: ext.fill_pattern(b, p, 0),
        lambda b, p: ext.verify_pattern(b, p, 0),
        lambda b, p: ext.verify_then_fill(b, p, 0, 0),
    ]
    bad_bufs = [
        new_buf(40),  # nbytes % 16 != 0
        torch.zeros(64, 2, dtype=torch.int32, device="cuda")[:, 0],  # non-contiguous
        torch.zeros(64, dtype=torch.uint8),  # CPU
    ]
    for call in calls:
        for b in bad_bufs:
            with pytest.raises(RuntimeError):
                call(b, 0)
        with pytest.raises(RuntimeError):
            call(good, 6)
    with pytest.raises(RuntimeError):
        ext.verify_then_fill(good, 0, 6, 0)
    with pytest.raises(ValueError):
        mc.fill_pattern(good, 6)
    torch.cuda.synchronize()
    assert (good.cpu() == SENTINEL).all()  # no rejected call touched the buffer


# 7. memcheck() ------------------------------------------------------------------------

def test_memcheck_clean():
    r = mc.memcheck(nbytes=8 << 20)
    assert r.ok is True
    assert r.passes == 7
    assert r.mismatched_words == 0 and r.first_bad_offset is None and r.records == []
    assert r.bytes_tested == 8 << 20
    assert r.gbps > 0 and r.elapsed_s > 0
    assert r.exceeds_llc is False
    assert json.loads(json.dumps(r.to_dict()))["ok"] is True


def test_memcheck_reports_corruption_between_passes():
    word = 123457

    def corrupt(pass_index, buf):
        if pass_index == 2:
            buf.view(torch.int32)[word] ^= 0x4

    r = mc.memcheck(nbytes=8 << 20, seed=5, _after_pass=corrupt)
    assert r.ok is False
    assert r.passes == 7
    assert r.mismatched_words == 1
    assert r.first_bad_offset == word * 4
    assert r.bad_bits_mask == 0x4
    assert r.records_dropped == 0
    (rec,) = r.records
    assert rec["pass"] == 3 and rec["offset"] == word * 4
    want = int(mc.reference_words(word // 4, 1, "checker", 5)[word % 4])
    assert rec["expected"] == want and rec["got"] == want ^ 0x4
    json.dumps(r.to_dict())


# 8. child process and CLI ---------------------------------------------------------------

def test_memcheck_child_process():
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.probe.memcheck",
         "--device", "0", "--bytes", "67108864"],
        capture_output=True, timeout=120, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    lines = res.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["ok"] is True and rec["passes"] == 7 and rec["bytes_tested"] == 67108864
    assert rec["device"] == 0 and rec["gbps"] > 0


def test_amddevs_memcheck_cli():
    from kubegpu_amd.discovery import default_backend

    n_gpus = len(default_backend().get_devices().devices)
    res = subprocess.run(
        [sys.executable, "-m", "kubegpu_amd.cli.amddevs",
         "--memcheck", "--bytes", "67108864"],
        capture_output=True, timeout=240, cwd=REPO, text=True,
    )
    assert res.returncode == 0, (res.stdout[-500:], res.stderr[-1000:])
    results = json.loads(res.stdout)
    assert len(results) == n_gpus >= 1
    for rec in results.values():
        assert rec["ok"] is True and rec["mismatched_words"] == 0
        assert rec["bytes_tested"] == 67108864


# 9. HBM-class floor -----------------------------------------------------------------------

def _gbps(fn, nbytes, iters=5):
    fn()  # warm-up
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return nbytes * iters / (t0.elapsed_time(t1) / 1e3) / 1e9


def test_hbm_class_floor():
    """Same 2000 GB/s floor as tests/test_gpu.py, at 1 GiB."""
    nbytes = 1 << 30
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    fill = _gbps(lambda: mc.fill_pattern(buf, "addr", 1), nbytes)
    verify = _gbps(lambda: mc.verify_pattern(buf, "addr", 1), nbytes)
    print(f"memcheck 1 GiB: fill {fill:.0f} GB/s, verify {verify:.0f} GB/s")
    assert mc.verify_pattern(buf, "addr", 1).ok
    assert fill > 2000.0, f"fill_pattern {fill:.0f} GB/s is far below HBM class"
    assert verify > 2000.0, f"verify_pattern {verify:.0f} GB/s is far below HBM class"
