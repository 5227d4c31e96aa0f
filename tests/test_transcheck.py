"""transcheck on the CPU: the exhaustive f16 walk, the classes the f32
recipes promise, the golden compare on the reference alone (accepts it
rounded to the format, rejects a flipped sign, exponent or protected
significand bit and a wrong class), the fold, and the wiring into the
probe list and the manager."""

import functools

import numpy as np
import pytest

from kubegpu_amd.probe import _active
from kubegpu_amd.probe import transcheck as tc

ROUNDS = np.arange(tc.PERIOD)
TYPES = {"f16": (np.float16, np.uint16), "f32": (np.float32, np.uint32),
         "f64": (np.float64, np.uint64)}
STAGE_OPS = [(s, op) for s in range(4) for op in tc.OPS[s] if not op.startswith("prng")]


@functools.lru_cache(maxsize=None)
def rounded(stage):
    """The reference of one period rounded to the format, as the typed bits
    [rounds, slots, operations, 64] and as the kernel's rows; read-only."""
    ref = tc.reference_values(0, stage, ROUNDS)
    bits = np.empty(ref.shape, dtype=np.uint64)
    with np.errstate(all="ignore"):
        for k, op in enumerate(tc.OPS[stage]):
            if op.startswith("prng"):
                bits[:, :, k] = ref[:, :, k].astype(np.uint64)
            else:
                ft, it = TYPES[tc._format_of(stage, op)]
                bits[:, :, k] = ref[:, :, k].astype(ft).view(it)
    bits.setflags(write=False)
    return bits, rows_of(stage, bits)


def rows_of(stage, bits):
    if stage == 2:
        bits = np.stack([bits & np.uint64(0xFFFFFFFF), bits >> np.uint64(32)], axis=3)
    return bits.reshape(bits.shape[0], -1, 64).astype(np.uint32)


def test_one_period_feeds_every_f16_code_once():
    codes = tc.f16_codes(ROUNDS)
    assert codes.shape == (tc.PERIOD, 8, 64)
    assert np.array_equal(np.sort(codes.ravel()), np.arange(65536))
    assert np.array_equal(tc.f16_codes(tc.PERIOD + 3), tc.f16_codes(3))


@pytest.mark.parametrize("seed", (0, 0xDEADBEEF))
def test_the_f32_recipes_reach_the_classes_they_claim(seed):
    def f32(b):
        with np.errstate(invalid="ignore"):  # NaN operands
            return b.astype(np.uint32).view(np.float32).astype(np.float64)

    bits = tc.operands(seed, 0, ROUNDS)
    x = f32(bits)
    for side in (1, -1):  # as close to 1.0 as 2**-20, on either side
        d = side * (x - 1)
        assert ((d > 0) & (d < 2.0 ** -19)).any() and ((d > 0.25) & (d <= 0.5)).any()
    quarter = (np.abs(x) <= 256) & (x * 4 == np.rint(x * 4)) & (x * 2 != np.rint(x * 2))
    assert quarter.sum() > 100 and (np.abs(x) == 256).any()
    for step in (1, -1):  # and one step either side of such a value
        y = f32(bits.astype(np.int64) + step)
        assert ((y * 8 == np.rint(y * 8)) & (x * 8 != np.rint(x * 8)) & (np.abs(x) < 256)).any()
    e, m = (bits >> np.uint64(23)) & np.uint64(0xFF), bits & np.uint64(0x7FFFFF)
    assert ((e == 0) & (m != 0)).sum() > 1000 and ((e == 0) & (m == 1)).any()
    for special in (0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000, 0xBF800000):
        assert (bits == special).any(), hex(special)
    assert ((e == 255) & (m != 0)).any()
    assert ((e > 0) & (e < 255) & (bits >> np.uint64(31) == 1)).any()
    assert (np.abs(x[np.isfinite(x)]) >= 512).any() and (e == 1).any() and (e == 254).any()


@pytest.mark.parametrize("stage", range(4))
def test_the_reference_rounded_to_the_format_is_within_every_bound(stage):
    rows = rounded(stage)[1]
    assert tc.check_values(stage, ROUNDS, rows, 0) == []
    worst = tc.max_errors(stage, ROUNDS, rows, 0)
    assert all(0 < worst[op] <= 0.5 for _, op in STAGE_OPS if _ == stage), worst


@pytest.mark.parametrize("stage,op", STAGE_OPS)
def test_a_flipped_sign_exponent_or_protected_bit_is_rejected(stage, op):
    bits = rounded(stage)[0].copy()
    k = tc.OPS[stage].index(op)
    ref = np.abs(tc.reference_values(0, stage, ROUNDS)[:, :, k])
    eb, mb = tc._FORMATS[tc._format_of(stage, op)]
    # a bound applies, and the measure's ulp is the result's own (or, below
    # one, twice that)
    ok = ~np.isnan(tc._compare(stage, ROUNDS, rounded(stage)[1], 0)[4][:, :, k])
    if op in tc._ABSOLUTE:
        ok &= (ref >= 0.5) & (ref < 1) if op in tc._BELOW_ONE else ref >= 1
    flips = [eb + mb] + list(range(mb, mb + eb)) + [mb - 1 - i
                                                     for i in range(tc.protected_bits(stage, op))]
    where = np.argwhere(ok)[:len(flips)]
    assert len(where) == len(flips)
    for (i, j, lane), bit in zip(where, flips):
        bits[i, j, k, lane] ^= np.uint64(1 << bit)
    got = tc.check_values(stage, ROUNDS, rows_of(stage, bits), 0)
    assert sorted((v["round"], v["slot"], v["lane"]) for v in got) == sorted(
        (int(i), int(j), int(lane)) for i, j, lane in where)
    assert all(v["op"] == op and v["stage"] == tc.STAGES[stage] and v["error"] != "class"
               for v in got)


@pytest.mark.parametrize("op,operand,wrong", [
    ("rcp", 0x00000000, 0xFF800000),   # rcp(+0) = +Inf, not -Inf
    ("log2", 0xBF800000, 0x3F800000),  # log2(-1) = NaN, not 1
    ("exp2", 0xFF800000, 0x80000000),  # exp2(-Inf) = +0, not -0
    ("sqrt", 0x80000000, 0x00000000),  # sqrt(-0) = -0, not +0
    ("sin", 0x7F800000, 0x00000000),   # sin(Inf) = NaN
])
def test_a_wrong_class_on_a_special_input_is_rejected(op, operand, wrong):
    bits = rounded(0)[0].copy()
    k = tc.OPS[0].index(op)
    i, j, lane = np.argwhere(tc.operands(0, 0, ROUNDS) == operand)[0]
    bits[i, j, k, lane] = wrong
    (v,) = tc.check_values(0, ROUNDS, rows_of(0, bits), 0)
    assert (v["op"], v["error"], v["operand"]) == (op, "class", hex(operand))
    assert (v["round"], v["slot"], v["lane"]) == (i, j, lane)


def test_violations_are_counted_but_listed_only_up_to_the_limit():
    zeros = np.zeros_like(rounded(0)[1])
    count, records = tc._violations(0, ROUNDS, zeros, 0, 3)
    assert count > 100000 and len(records) == 3
    assert tc.check_values(0, ROUNDS, zeros, 0, limit=3) == records


def test_a_reference_of_exactly_zero_is_bounded_in_the_absolute_measure():
    bits, ref = rounded(0)[0].copy(), tc.reference_values(0, 0, ROUNDS)
    for op in ("sin", "log2"):  # whole revolutions, log2(1.0)
        k = tc.OPS[0].index(op)
        err = tc._compare(0, ROUNDS, rounded(0)[1], 0)[4][:, :, k]
        i, j, lane = np.argwhere((ref[:, :, k] == 0) & ~np.isnan(err))[0]
        bits[i, j, k, lane] = 0x38800000  # 2**-14 where 0 is due: 2**9 ulps of 1
        (v,) = [x for x in tc.check_values(0, ROUNDS, rows_of(0, bits), 0) if x["op"] == op]
        assert (v["round"], v["slot"], v["lane"], v["error"]) == (i, j, lane, 512.0)


@pytest.mark.parametrize("stage", range(4))
def test_the_fold_sees_every_bit(stage):
    rows = rounded(stage)[1][:2].copy()
    before = tc.fold_values(stage, rows)
    rows[1, -1, 63] ^= 1
    after = tc.fold_values(stage, rows)
    assert before.dtype == np.uint32 and before[0] == after[0] and before[1] != after[1]
    names = tc.slot_table(stage)
    assert tc.fold_values(stage, dict(zip(names, rows[0])))[0] == before[0]


def test_the_prng_step_is_the_lfsr():
    s = np.array([1, 0x80000000, 0xFFFFFFFF, 0x40000000], dtype=np.uint64)
    assert tc.prng_step(s).tolist() == [2, 0xC5, 0xFFFFFFFE ^ 0xC5, 0x80000000]


def test_a_failed_verdict_turns_the_gpu_unhealthy_until_cleared():
    from kubegpu_amd.deviceplugin import create_device_plugin
    from kubegpu_amd.discovery import FakeBackend, fixtures

    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    uuid = sorted(mgr.gpus)[0]
    bad = tc.TranscheckResult(ok=False, rounds=2, mismatches=1, golden_errors=1,
                              golden_records=[{"op": "exp2"}]).to_dict()
    assert bad["golden_errors"] == 1 and bad["digest_mismatches"] == 0
    assert mgr.record_transcheck(uuid, bad) is False and mgr.device_health()[uuid] is False
    assert mgr.transcheck_status(uuid)["golden_records"] == [{"op": "exp2"}]
    assert mgr.clear_transcheck(uuid) and mgr.device_health()[uuid] is True


def test_the_verdict_probes_extend_the_probe_names():
    assert _active.VERDICT_PROBES == _active.PROBE_NAMES + ("transcheck",)
    assert len(set(_active.VERDICT_PROBES)) == len(_active.VERDICT_PROBES)
