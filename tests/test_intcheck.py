"""intcheck on the CPU: the numpy reference against a scalar model in
Python's unbounded integers, the coverage the operand recipes promise over
one period, the table's wrap, the slot names and the wiring into the
probe list and the manager."""

import functools

import numpy as np
import pytest

from kubegpu_amd.probe import _active
from kubegpu_amd.probe import intcheck as ic

M, M64, IMIN, IMAX = 0xFFFFFFFF, (1 << 64) - 1, 0x80000000, 0x7FFFFFFF
SEEDS = (0, 0xDEADBEEF)


def s(x, n=32):
    x &= (1 << n) - 1
    return x - ((x >> (n - 1)) << n)


def tdiv(a, b):
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def parts(x, n, sg=False):
    return [s(x >> k, n) if sg else (x >> k) & ((1 << n) - 1) for k in range(0, 32, n)]


def join(ps, n):
    return sum((p & ((1 << n) - 1)) << (n * k) for k, p in enumerate(ps))


def pk(f, n, sg, *xs):
    return join([f(*col) for col in zip(*(parts(x, n, sg) for x in xs))], n)


def dot(a, b, n, sg):
    return sum(x * y for x, y in zip(parts(a, n, sg), parts(b, n, sg)))


def clamped(a, b, c, sel, n, sg):
    cc = (ic.ANCHOR[sel >> 30] + s(c, ic.CLAMP_BITS[n])) & M
    return clip(dot(a, b, n, sg) + (s(cc) if sg else cc), *((-IMIN, IMAX) if sg else (0, M)))


def loop(t):
    h = 0
    while t:
        h = (h * 33 + ctz(t)) & M
        t &= t - 1
    return h


def select4(a, b, c):
    v = b if a & 1 else c
    v = (v + 1) & M if v < a else a
    v = v ^ c if s(v) < s(b) else (v - b) & M
    return a if v == c else v


clip = lambda v, lo, hi: max(lo, min(hi, v))  # noqa: E731
clz = lambda x, n=32: n - x.bit_length()  # noqa: E731
ctz = lambda x, n=32: (x & -x).bit_length() - 1 if x else n  # noqa: E731
popc = lambda x: bin(x).count("1")  # noqa: E731
X = lambda a, c: (c << 32) | a  # noqa: E731
Y = lambda a, b: ((a ^ IMIN) << 32) | b  # noqa: E731
width = lambda b: (b >> 8) % (min(31, 32 - (b & 31)) + 1)  # noqa: E731
limbs = lambda a, b, c: (a | b << 32 | c << 64, b | c << 32 | a << 64)  # noqa: E731
iden = lambda a, b: 1 if b == 0 or (a == IMIN and b == M) else s(b)  # noqa: E731
den64 = lambda a, b, sel: (Y(a, b) >> (sel >> 26)) or 1  # noqa: E731

# one op each, on Python integers: (a, b, c, sel) -> value, masked by the
# test to 32 or 64 bits; the scalar stage calls them with (x, y, z, sel)
MODEL = {
    "shl": lambda a, b, c, e: a << (b & 31), "shr": lambda a, b, c, e: a >> (b & 31),
    "sar": lambda a, b, c, e: s(a) >> (b & 31),
    "shl64": lambda a, b, c, e: X(a, c) << (b & 63), "shr64": lambda a, b, c, e: X(a, c) >> (b & 63),
    "sar64": lambda a, b, c, e: s(X(a, c), 64) >> (b & 63),
    "alignbit": lambda a, b, c, e: X(c, a) >> (b & 31), "rotr": lambda a, b, c, e: X(a, a) >> (b & 31),
    "alignbyte": lambda a, b, c, e: X(c, a) >> 8 * (b & 3),
    "ubfe": lambda a, b, c, e: (a >> (b & 31)) & ((1 << width(b)) - 1),
    "sbfe": lambda a, b, c, e: s(a >> (b & 31), width(b)) if width(b) else 0,
    "bfi": lambda a, b, c, e: (a & b) | (~a & c),
    "perm": lambda a, b, c, e: join([(parts(c, 8) + parts(a, 8) + [0])[((e >> 4 * i) & 15) % 9]
                                     for i in range(4)], 8),
    "brev": lambda a, b, c, e: int(f"{a:032b}"[::-1], 2),
    "popc_add": lambda a, b, c, e: popc(a) + c,
    "clz": lambda a, b, c, e: clz(a), "ctz": lambda a, b, c, e: ctz(a),
    "clrsb": lambda a, b, c, e: clz((a ^ (s(a) >> 31)) & M) - 1,
    "popc64": lambda a, b, c, e: popc(X(a, c)), "clz64": lambda a, b, c, e: clz(X(a, c), 64),
    "ctz64": lambda a, b, c, e: ctz(X(a, c), 64), "popc": lambda a, b, c, e: popc(a),
    "shl1_add": lambda a, b, c, e: (a << 1) + b, "shl2_add": lambda a, b, c, e: (a << 2) + b,
    "shl3_add": lambda a, b, c, e: (a << 3) + b, "shl4_add": lambda a, b, c, e: (a << 4) + b,
    "add_shl": lambda a, b, c, e: (a + b) << 3, "shl_or": lambda a, b, c, e: (a << 2) | b,
    "and_or": lambda a, b, c, e: (a & b) | c, "or3": lambda a, b, c, e: a | b | c,
    "add3": lambda a, b, c, e: a + b + c, "xad": lambda a, b, c, e: (a ^ b) + c,
    "add3l.0": lambda a, b, c, e: sum(limbs(a, b, c)), "add3l.1": lambda a, b, c, e: sum(limbs(a, b, c)) >> 32,
    "add3l.2": lambda a, b, c, e: sum(limbs(a, b, c)) >> 64,
    "add3l.carry": lambda a, b, c, e: sum(limbs(a, b, c)) >> 96,
    "sub3l.0": lambda a, b, c, e: limbs(a, b, c)[0] - limbs(a, b, c)[1],
    "sub3l.1": lambda a, b, c, e: (limbs(a, b, c)[0] - limbs(a, b, c)[1]) >> 32,
    "sub3l.2": lambda a, b, c, e: ((limbs(a, b, c)[0] - limbs(a, b, c)[1]) >> 64) & M,
    "sub3l.borrow": lambda a, b, c, e: int(limbs(a, b, c)[0] < limbs(a, b, c)[1]),
    "add64": lambda a, b, c, e: X(a, c) + Y(a, b), "sub64": lambda a, b, c, e: X(a, c) - Y(a, b),
    "mul_lo": lambda a, b, c, e: a * b, "mulhi_u": lambda a, b, c, e: (a * b) >> 32,
    "mulhi_i": lambda a, b, c, e: (s(a) * s(b)) >> 32,
    "mul_i24": lambda a, b, c, e: s(a, 24) * s(b, 24),
    "mulhi_i24": lambda a, b, c, e: (s(a, 24) * s(b, 24)) >> 32,
    "mul_u24": lambda a, b, c, e: (a & 0xFFFFFF) * (b & 0xFFFFFF),
    "mulhi_u24": lambda a, b, c, e: ((a & 0xFFFFFF) * (b & 0xFFFFFF)) >> 32,
    "mad_u64": lambda a, b, c, e: a * b + X(a, c), "mad_i64": lambda a, b, c, e: s(a) * s(b) + X(a, c),
    "mul64": lambda a, b, c, e: X(a, c) * Y(a, b),
    "udiv": lambda a, b, c, e: a // (b or 1), "urem": lambda a, b, c, e: a % (b or 1),
    "sdiv": lambda a, b, c, e: tdiv(s(a), iden(a, b)),
    "srem": lambda a, b, c, e: s(a) - tdiv(s(a), iden(a, b)) * iden(a, b),
    "udiv64": lambda a, b, c, e: X(a, c) // den64(a, b, e), "urem64": lambda a, b, c, e: X(a, c) % den64(a, b, e),
    "min_i": lambda a, b, c, e: min(s(a), s(b)), "max_i": lambda a, b, c, e: max(s(a), s(b)),
    "min_u": lambda a, b, c, e: min(a, b), "max_u": lambda a, b, c, e: max(a, b),
    "med3_i": lambda a, b, c, e: sorted((s(a), s(b), s(c)))[1], "med3_u": lambda a, b, c, e: sorted((a, b, c))[1],
    "min3_i": lambda a, b, c, e: min(s(a), s(b), s(c)), "min3_u": lambda a, b, c, e: min(a, b, c),
    "max3_i": lambda a, b, c, e: max(s(a), s(b), s(c)), "max3_u": lambda a, b, c, e: max(a, b, c),
    "absdiff": lambda a, b, c, e: abs(a - b), "select4": lambda a, b, c, e: select4(a, b, c),
    "lt_i": lambda a, b, c, e: s(a) < s(b), "lt_u": lambda a, b, c, e: a < b, "eq": lambda a, b, c, e: a == b,
    "lt_u64": lambda a, b, c, e: X(a, c) < Y(a, b),
    "lt_i64": lambda a, b, c, e: s(X(a, c), 64) < s(Y(a, b), 64),
    "add16": lambda a, b, c, e: pk(lambda x, y: x + y, 16, False, a, b),
    "sub16": lambda a, b, c, e: pk(lambda x, y: x - y, 16, False, a, b),
    "add_sat_i16": lambda a, b, c, e: pk(lambda x, y: clip(x + y, -0x8000, 0x7FFF), 16, True, a, b),
    "sub_sat_i16": lambda a, b, c, e: pk(lambda x, y: clip(x - y, -0x8000, 0x7FFF), 16, True, a, b),
    "add_sat_u16": lambda a, b, c, e: pk(lambda x, y: clip(x + y, 0, 0xFFFF), 16, False, a, b),
    "sub_sat_u16": lambda a, b, c, e: pk(lambda x, y: clip(x - y, 0, 0xFFFF), 16, False, a, b),
    "mul16": lambda a, b, c, e: pk(lambda x, y: x * y, 16, False, a, b),
    "mad_i16": lambda a, b, c, e: pk(lambda x, y, z: x * z + y, 16, True, a, b, c),
    "mad_u16": lambda a, b, c, e: pk(lambda x, y, z: x * y + z, 16, False, a, b, c),
    "min_i16": lambda a, b, c, e: pk(min, 16, True, a, b), "max_i16": lambda a, b, c, e: pk(max, 16, True, a, b),
    "min_u16": lambda a, b, c, e: pk(min, 16, False, a, b), "max_u16": lambda a, b, c, e: pk(max, 16, False, a, b),
    "shl16": lambda a, b, c, e: pk(lambda x, y: x << (y & 15), 16, False, a, b),
    "lshr16": lambda a, b, c, e: pk(lambda x, y: x >> (y & 15), 16, False, a, b),
    "ashr16": lambda a, b, c, e: pk(lambda x, y: x >> (y & 15), 16, True, a, b),
    "sad_u8": lambda a, b, c, e: c + sum(abs(x - y) for x, y in zip(parts(a, 8), parts(b, 8))),
    "sad_hi_u8": lambda a, b, c, e: c + (sum(abs(x - y) for x, y in zip(parts(a, 8), parts(b, 8))) << 16),
    "sad_u16": lambda a, b, c, e: c + sum(abs(x - y) for x, y in zip(parts(a, 16), parts(b, 16))),
    "lerp": lambda a, b, c, e: pk(lambda x, y, z: (x + y + (z & 1)) >> 1, 8, False, a, b, c),
    "sdot4": lambda a, b, c, e: dot(a, b, 8, True) + c, "udot4": lambda a, b, c, e: dot(a, b, 8, False) + c,
    "sdot8": lambda a, b, c, e: dot(a, b, 4, True) + c, "udot8": lambda a, b, c, e: dot(a, b, 4, False) + c,
    "sdot2": lambda a, b, c, e: dot(a, b, 16, True) + c, "udot2": lambda a, b, c, e: dot(a, b, 16, False) + c,
    "sdot4.clamp": lambda a, b, c, e: clamped(a, b, c, e, 8, True),
    "udot4.clamp": lambda a, b, c, e: clamped(a, b, c, e, 8, False),
    "sdot8.clamp": lambda a, b, c, e: clamped(a, b, c, e, 4, True),
    "udot8.clamp": lambda a, b, c, e: clamped(a, b, c, e, 4, False),
    "sdot2.clamp": lambda a, b, c, e: clamped(a, b, c, e, 16, True),
    "udot2.clamp": lambda a, b, c, e: clamped(a, b, c, e, 16, False),
    "field_u": lambda x, y, z, e: (x >> (y & 31)) & ((1 << ((y >> 8) & 15)) - 1),
    "field_i": lambda x, y, z, e: s(x << (31 - (y & 31))) >> ((y >> 16) & 31),
    "andn2": lambda x, y, z, e: x & ~y, "orn2": lambda x, y, z, e: x | ~y, "nand": lambda x, y, z, e: ~(x & y),
    "nor": lambda x, y, z, e: ~(x | y), "xnor": lambda x, y, z, e: ~(x ^ y),
    "sext8": lambda x, y, z, e: s(x, 8), "sext16": lambda x, y, z, e: s(x, 16),
    "switch": lambda x, y, z, e: (x + y, x ^ (y >> 3), (x & y) * 3, x - z)[e & 3],
    "loop": lambda x, y, z, e: loop(x), "loop2": lambda x, y, z, e: loop(x & (x - 1)),
}
BALLOTS = ("lt_i", "lt_u", "eq", "lt_u64", "lt_i64")
MASKS = {"m1": lambda p, q: p, "m2": lambda p, q: q, "andn": lambda p, q: p & ~q & M64,
         "xor": lambda p, q: p ^ q}
MASK_OPS = {"popc": popc, "ctz": lambda m: ctz(m, 64), "clz": lambda m: clz(m, 64)}


def model_slot(name, ops, masks):
    """One row of 64 for slot ``name`` from the scalar model."""
    half = name[-3:] if name[-3:] in (".lo", ".hi") else ""
    key = name[:len(name) - len(half)]
    if key.split(".")[0] in MASKS or key.startswith("m1."):
        m1, m2, n = masks
        if key in ("m1.shl", "m1.sar"):
            v = m1 << n if key == "m1.shl" else s(m1, 64) >> n
        else:
            mask = MASKS[key.split(".")[0]](m1, m2)
            v = mask if "." not in key else MASK_OPS[key.split(".")[1]](mask)
        vals = [v] * 64
    else:
        j, op = key.split(".", 1)
        vals = [MODEL[op](*(int(o[lane]) for o in ops[int(j)])) for lane in range(64)]
        if op in BALLOTS:
            vals = [sum(int(bit) << lane for lane, bit in enumerate(vals))] * 64
    shift = 32 if half == ".hi" else 0
    return [((v & M64) >> shift) & M for v in vals]


@pytest.mark.parametrize("r", (0, 1))
@pytest.mark.parametrize("stage", range(4))
def test_reference_values_equal_the_python_int_model(stage, r):
    seed, rr = 0xDEADBEEF, np.array([r], dtype=np.uint32)
    if stage < 3:
        ops = [[o[0] for o in ic.operands(seed, stage, rr, j)] for j in range(ic.GROUPS)]
    else:
        ops = [[np.repeat(o, 64) for o in ic.scalar_operands(seed, rr, j)] for j in range(ic.GROUPS)]
    masks = tuple(int(m[0]) for m in ic.wave_masks(seed, rr))
    for name, row in ic.reference_values(seed, stage, r).items():
        want = model_slot(name, ops, masks)
        assert [int(v) for v in row] == want, (name, [hex(int(v)) for v in row[:4]], want[:4])


@functools.lru_cache(maxsize=None)
def period(seed, stage):
    """Operands (a, b, c, sel) of both groups side by side and the slots of
    a stage over one period, read-only."""
    r = np.arange(ic.PERIOD, dtype=np.uint32)
    if stage < 3:
        ops = [np.concatenate(o, axis=1) for o in zip(*(ic.operands(seed, stage, r, j) for j in (0, 1)))]
    else:
        ops = [np.concatenate(o) for o in zip(*(ic.scalar_operands(seed, r, j) for j in (0, 1)))]
    return ops, dict(ic._stage(seed, stage, r))


def both(bits):
    return bool(bits.any() and not bits.all())


@pytest.mark.parametrize("seed", SEEDS)
def test_the_recipes_cover_the_edges_over_one_period(seed):
    (a, b, c, sel), _ = period(seed, 0)
    assert set((b & 63).ravel().tolist()) == set(range(64))
    off = b & 31
    w = (b >> 8) % (np.minimum(31, 32 - off.astype(np.int64)).astype(np.uint64) + 1)
    assert (w == 0).any() and (off + w == 32).any()
    for i in range(4):
        assert set((((sel >> (4 * i)) & 15) % 9).ravel().tolist()) == set(range(9))

    (a, b, c, sel), slots = period(seed, 1)
    carry = np.concatenate([slots["0.add3l.carry"], slots["1.add3l.carry"]], axis=1)
    assert both(carry == 1)
    assert ((a + b > M) & (b + c == M)).any()  # a carry through a full middle limb
    x, y = (c << 32) | a, ((a ^ IMIN) << 32) | b
    for bits in (ic._i(a) < ic._i(b), a < b, a == b, x < y, x.astype(np.int64) < y.astype(np.int64)):
        assert both(bits)
    assert (x == y).any()
    assert (b == 0).any() and ((a == IMIN) & (b == M)).any()  # both division remaps
    q = np.concatenate([slots["0.udiv"], slots["1.udiv"]])
    assert (q == 0).any() and (q == 1).any()

    (a, b, c, sel), _ = period(seed, 2)
    for sg, (lo, hi) in ((True, (-0x8000, 0x7FFF)), (False, (0, 0xFFFF))):
        for x, y in zip(ic._parts(a, 16, sg), ic._parts(b, 16, sg)):
            assert (x + y > hi).any() and (x + y <= hi).any() and (x - y < lo).any() and (x - y >= lo).any()
            assert not sg or ((x + y < lo).any() and (x - y > hi).any())
    anchor = np.array(ic.ANCHOR, dtype=np.uint64)[(sel >> 30).astype(np.int64)]
    for bits in (8, 4, 16):
        cc = ic._u(anchor + ic._sext(c, ic.CLAMP_BITS[bits]))
        for sg in (True, False):
            exact = sum(x * y for x, y in zip(ic._parts(a, bits, sg), ic._parts(b, bits, sg)))
            exact = exact + (ic._i(cc) if sg else cc.astype(np.int64))
            lo, hi = (-IMIN, IMAX) if sg else (0, M)
            assert (exact > hi).any() and ((exact <= hi) & (exact >= lo)).any(), (bits, sg)
            assert not sg or (exact < lo).any(), bits

    (x, y, z, sel), _ = period(seed, 3)
    trips = {popc(int(v)) for v in x} | {popc(int(v) & (int(v) - 1)) for v in x}
    assert {0, 1} <= trips and max(trips) >= 16
    assert set((sel & 3).tolist()) == {0, 1, 2, 3}
    m1 = ic.wave_masks(seed, np.arange(ic.PERIOD, dtype=np.uint32))[0]
    assert 2 * int(((m1 != 0) & (m1 != M64)).sum()) >= ic.PERIOD


def test_reference_digests_wrap_at_the_period_and_reject_negative_rounds():
    table = ic.reference_digests(3, ic.PERIOD + 2)
    assert table.shape == (ic.PERIOD + 2, 4) and table.dtype == np.uint32
    assert np.array_equal(table[ic.PERIOD:], table[:2]) and not np.array_equal(table[0], table[1])
    assert ic.reference_digests(3, 0).shape == (0, 4)
    with pytest.raises(ValueError):
        ic.reference_digests(3, -1)


@pytest.mark.parametrize("stage", range(4))
def test_slot_names_are_unique_and_fit_the_value_rows(stage):
    names = ic.slot_table(stage)
    assert len(set(names)) == len(names) <= ic._VALUE_ROWS
    assert names == list(ic.reference_values(5, stage, 9))


def test_intcheck_is_the_last_probe_name():
    assert _active.PROBE_NAMES[-1] == "intcheck"
    assert len(set(_active.PROBE_NAMES)) == len(_active.PROBE_NAMES)


def test_a_failed_verdict_turns_the_gpu_unhealthy_until_cleared():
    from kubegpu_amd.deviceplugin import create_device_plugin
    from kubegpu_amd.discovery import FakeBackend, fixtures

    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    uuid = sorted(mgr.gpus)[0]
    bad = ic.IntcheckResult(ok=False, rounds=2, mismatches=3, first_bad_round=1,
                            bad_stages=["scalar"]).to_dict()
    assert mgr.record_intcheck(uuid, bad) is False and mgr.device_health()[uuid] is False
    assert mgr.intcheck_status(uuid)["ok"] is False
    assert mgr.clear_intcheck(uuid) and mgr.device_health()[uuid] is True
