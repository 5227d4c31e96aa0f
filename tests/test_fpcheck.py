"""fpcheck without a GPU: the three fma references and the conversions
against independent arithmetic, what the operand recipes reach, the
digests, and the plumbing (manager verdicts, rounds over idle GPUs,
metrics, agent and amddevs flags)."""

import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from kubegpu_amd.api.types import NodeInfo
from kubegpu_amd.deviceplugin import create_device_plugin
from kubegpu_amd.discovery import FakeBackend, fixtures
from kubegpu_amd.plugintypes import RESOURCE_GPU
from kubegpu_amd.probe import fpcheck as fp

# precision, least normal exponent and numpy types of the three formats
FORMATS = {"f16": (11, -14, np.uint16, np.float16), "f32": (24, -126, np.uint32, np.float32),
           "f64": (53, -1022, np.uint64, np.float64)}


def to_float(bits, fmt):
    """uint64 bit patterns -> array of the format's numpy float type."""
    _, _, it, ft = FORMATS[fmt]
    return bits.astype(it).view(ft)


def round_fraction(f, fmt):
    """A rational correctly rounded (nearest, ties to even) to the format,
    as a Python float (every f16 / f32 value is one) or +-inf."""
    p, emin, _, ft = FORMATS[fmt]
    if f == 0:
        return 0.0
    sign = -1.0 if f < 0 else 1.0
    f = abs(f)
    e = f.numerator.bit_length() - f.denominator.bit_length()
    if Fraction(2) ** e > f:
        e -= 1
    e = max(e, emin)
    q = f / Fraction(2) ** (e - p + 1)  # in units of the last place
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    v = Fraction(n) * Fraction(2) ** (e - p + 1)
    if v > Fraction(float(np.finfo(ft).max)):
        return sign * math.inf
    return sign * float(v)  # exact: at most p <= 53 significant bits


def test_round_fraction_itself():
    assert round_fraction(Fraction(1, 3), "f32") == float(np.float32(1) / np.float32(3))
    assert round_fraction(Fraction(1) + Fraction(1, 2 ** 24), "f32") == 1.0  # tie to even
    assert round_fraction(Fraction(1) + Fraction(3, 2 ** 24), "f32") == 1.0 + 2.0 ** -22
    assert round_fraction(Fraction(65520), "f16") == math.inf
    assert round_fraction(Fraction(65519), "f16") == 65504.0
    assert round_fraction(Fraction(1, 2 ** 25), "f16") == 0.0  # half the least subnormal: to even
    assert round_fraction(Fraction(3, 2 ** 26), "f16") == 2.0 ** -24
    assert round_fraction(Fraction(-1, 3), "f64") == -1 / 3


# -- the fma references against rational arithmetic ------------------------------------

def _fma_triples(stage, names, fmt, rounds):
    """Finite operand triples of a stage over ``rounds`` rounds: every
    recipe, so ties, cancellation, subnormals and overflow are among them."""
    cols = [[], [], []]
    for r in range(rounds):
        ops = fp.reference_operands(0, stage, r)
        for k, n in enumerate(names):
            cols[k].append(to_float(ops[n], fmt))
    a, b, c = (np.concatenate(x) for x in cols)
    fin = np.isfinite(a) & np.isfinite(b) & np.isfinite(c)
    return a[fin], b[fin], c[fin]


def _exact_fma(a, b, c, fmt):
    return np.array([round_fraction(Fraction(x) * Fraction(y) + Fraction(z), fmt)
                     for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])


@pytest.mark.parametrize("fmt,stage,names,rounds", [
    ("f32", 0, ("a", "b", "c"), 6), ("f16", 2, ("h0.a", "h0.b", "h0.c"), 6)])
def test_narrow_fma_reference_is_correctly_rounded(fmt, stage, names, rounds):
    a, b, c = _fma_triples(stage, names, fmt, rounds)
    assert len(a) > 2000
    want = _exact_fma(a, b, c, fmt)
    got = fp.fma_narrow(a, b, c)
    assert got.dtype == a.dtype
    bad = got.astype(np.float64) != want  # as values: a rational has no signed zero
    assert not bad.any(), (int(bad.sum()), a[bad][:3], b[bad][:3], c[bad][:3])
    tiny = float(np.finfo(a.dtype).tiny)
    assert np.isinf(want).sum() > 20 and ((np.abs(want) < tiny) & (want != 0)).sum() > 20
    # the set tells a double rounding apart: product and sum rounded once each
    with np.errstate(all="ignore"):
        twice = (a * b + c).astype(np.float64)
    assert (twice != want).any()


def test_f64_fma_reference_is_correctly_rounded_and_the_naive_one_is_not():
    a, b, c = _fma_triples(1, ("fma_a", "fma_b", "fma_c"), "f64", 12)
    assert len(a) == 12 * 256  # the remap leaves no Inf or NaN
    e = np.abs(np.frexp(np.concatenate([a, b, c]))[1])
    assert e.max() <= 202
    # Python's int / int is correctly rounded
    want = np.array([(lambda f: f.numerator / f.denominator)(
        Fraction(x) * Fraction(y) + Fraction(z)) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())])
    got = fp.fma_f64(a, b, c)
    bad = got != want
    assert not bad.any(), (int(bad.sum()), a[bad][:3], b[bad][:3], c[bad][:3])
    naive = a * b + c
    print(f"naive a*b+c wrong on {int((naive != want).sum())} of {len(a)}")
    assert (naive != want).sum() > 100


# -- conversions against torch's CPU casts ------------------------------------------------

def _cvt_inputs(rounds=8):
    xs = [fp.reference_operands(0, 3, r)["x"] for r in range(rounds)]
    return np.concatenate(xs)


def test_bf16_conversion_matches_torch():
    x = _cvt_inputs()
    xf = to_float(x, "f32")
    t = torch.from_numpy(xf.copy()).to(torch.bfloat16).view(torch.int16).numpy()
    want = t.view(np.uint16).astype(np.uint64)
    want = np.where(np.isnan(xf), np.uint64(fp.BF16_CANONICAL_NAN), want)
    got = fp.f32_to_bf16_bits(x)
    assert np.array_equal(got, want)
    assert np.isnan(xf).sum() > 10 and np.isinf(xf).sum() > 10
    assert ((x & np.uint64(0xFFFF)) == 0x8000).sum() > 10  # exact ties among them
    got_ref = np.concatenate([fp.reference_values(0, 3, r)["f32_bf16"] for r in range(8)])
    assert np.array_equal(got_ref, want)


def test_f16_conversion_matches_torch():
    x = _cvt_inputs()
    xf = to_float(x, "f32")
    t = torch.from_numpy(xf.copy()).to(torch.float16).view(torch.int16).numpy()
    want = t.view(np.uint16).astype(np.uint64)
    want = np.where(np.isnan(xf), np.uint64(fp.F16.canonical_nan), want)
    got = np.concatenate([fp.reference_values(0, 3, r)["f32_f16"] for r in range(8)])
    assert np.array_equal(got, want)


def test_f32_to_i32_is_confined_and_truncates():
    for r in range(8):
        xi = to_float(fp.reference_operands(0, 3, r)["xi"], "f32")
        assert np.isfinite(xi).all() and (np.abs(xi) < 2.0 ** 31).all()
        got = fp.reference_values(0, 3, r)["f32_i32"]
        want = [int(v) & 0xFFFFFFFF for v in xi.tolist()]  # int() truncates
        assert got.tolist() == want
    assert (np.abs(xi) >= 2.0 ** 23).any()


def test_subnormal_guard(monkeypatch):
    fp._check_subnormals()  # this host keeps them
    real = np.float32

    class Flushing(real):
        def __mul__(self, other):
            return real(0)

    monkeypatch.setattr(np, "float32", Flushing)
    with pytest.raises(RuntimeError, match="subnormal"):
        fp._check_subnormals()


# -- what the recipes reach ------------------------------------------------------------------

ALL = {"inexact", "tie_up", "tie_down", "subnormal", "overflow", "underflow_zero", "nan",
       "cancel20"}
# What each operation admits, and why not the rest.  A sum or difference
# that lands in the subnormal range is exact, so add cannot underflow
# inexactly; two 11-bit f16 addends cannot cancel by 20 binary orders
# unless to zero; a product has no cancellation; the f64 fma's operands
# are confined to mid exponents (module docstring); a quotient is an
# exact tie only in the subnormal range and a square root never, so
# neither is asked for ties; sqrt of a finite number neither overflows
# nor leaves the normal range.
ADD = ALL - {"underflow_zero"}
MUL = ALL - {"cancel20"}
DIV = {"inexact", "subnormal", "overflow", "underflow_zero", "nan"}
SQRT = {"inexact", "nan"}
WANTED = {
    (0, "add"): ADD, (0, "mul"): MUL, (0, "fma"): ALL, (0, "div"): DIV, (0, "sqrt"): SQRT,
    (1, "add"): ADD, (1, "mul"): MUL, (1, "fma"): {"inexact", "tie_up", "tie_down", "cancel20"},
    (1, "div"): DIV, (1, "sqrt"): SQRT,
    (2, "pk_fma_f16"): ALL, (2, "pk_mul_f16"): MUL, (2, "pk_add_f16"): ADD - {"cancel20"},
    (2, "pk_fma_f32.x"): ALL, (2, "pk_fma_f32.y"): ALL,
    (2, "pk_mul_f32.x"): MUL, (2, "pk_mul_f32.y"): MUL,
    (2, "pk_add_f32.x"): ADD, (2, "pk_add_f32.y"): ADD,
    # conversions: a value to be rounded into a narrower format
    (3, "f32_f16"): MUL, (3, "f64_f32"): MUL,
    # bf16 has f32's exponent range: it cannot underflow
    (3, "f32_bf16"): {"inexact", "tie_up", "tie_down", "subnormal", "overflow", "nan"},
    (3, "u32_f32"): {"inexact", "tie_up", "tie_down"},
    (3, "i32_f32"): {"inexact", "tie_up", "tie_down"},
    (3, "rint"): {"inexact", "tie_up", "tie_down", "nan"},
    (3, "floor"): {"inexact", "nan"}, (3, "ceil"): {"inexact", "nan"},
    (3, "trunc"): {"inexact", "nan"}, (3, "f32_i32"): {"inexact"},
}


def _classes(exact, res, fmt, larger=None):
    """Classes one finite exact value and its rounded result (a Python
    float of format ``fmt``) fall in."""
    p, emin, _, ft = FORMATS[fmt]
    out = set()
    if math.isinf(res):
        return {"overflow", "inexact"}
    if res != exact:
        out.add("inexact")
        if res == 0:
            out.add("underflow_zero")
        other = float(np.nextafter(ft(res), ft(math.inf if exact > res else -math.inf)))
        if not math.isinf(other) and Fraction(res) + Fraction(other) == 2 * exact:
            out.add("tie_up" if res > exact else "tie_down")
    if res != 0 and abs(res) < 2.0 ** emin:
        out.add("subnormal")
    if larger and res != 0 and math.frexp(res)[1] <= math.frexp(larger)[1] - 20:
        out.add("cancel20")
    return out


def _observe(stage, op, ops, vals, q):
    """Classes of result q of an operation; operands and results as
    Python floats / ints."""
    def get(name, fmt):
        return float(to_float(ops[name][q:q + 1], fmt)[0])

    if stage == 3:
        res_fmt = {"f32_f16": "f16"}.get(op, "f32")
        if op == "f32_bf16":
            x = int(ops["x"][q])
            if (x & 0x7FFFFFFF) > 0x7F800000:
                return {"nan"}
            out = set()
            if x & 0xFFFF:
                out.add("inexact")
                if (x & 0xFFFF) == 0x8000:
                    out.add("tie_up" if int(vals[op][q]) > (x >> 16) else "tie_down")
            if 0 < (int(vals[op][q]) & 0x7FFF) < 0x80:
                out.add("subnormal")
            if (int(vals[op][q]) & 0x7FFF) == 0x7F80 and (x & 0x7FFFFFFF) < 0x7F800000:
                out.add("overflow")
            return out
        if op == "f32_i32":
            x = get("xi", "f32")
            return {"inexact"} if x != int(x) else set()
        if op in ("u32_f32", "i32_f32"):
            u = int(ops["u"][q])
            exact = Fraction(u - (1 << 32) if op == "i32_f32" and u >> 31 else u)
        else:
            x = get("d", "f64") if op == "f64_f32" else get("x", "f32")
            if math.isnan(x):
                return {"nan"}
            if math.isinf(x):
                return set()
            exact = Fraction(x)
        res = float(to_float(vals[op][q:q + 1], res_fmt)[0])
        if op in ("rint", "floor", "ceil", "trunc"):
            out = {"inexact"} if res != exact else set()
            if op == "rint" and exact - math.floor(exact) == Fraction(1, 2):
                out.add("tie_up" if res > exact else "tie_down")
            return out
        return _classes(exact, res, res_fmt)

    if stage == 2:
        fmt = "f16" if op.endswith("f16") else "f32"
        e = 1 if op.endswith(".y") else 0
        tag = "h" if fmt == "f16" else "f"
        raw = int(vals[op][q])
        results = [raw & 0xFFFF, raw >> 16] if fmt == "f16" else [raw]
        elems = (0, 1) if fmt == "f16" else (e,)
        out = set()
        for el, rbits in zip(elems, results):
            a, b, c = (get(f"{tag}{el}.{n}", fmt) for n in "abc")
            kind = op.split("_")[1]
            out |= _arith(kind, a, b, c, np.array([rbits], dtype=np.uint64), fmt)
        return out
    fmt = "f32" if stage == 0 else "f64"
    names = fp.operands_of(stage, op)
    a, b, c = (get(n, fmt) for n in names)
    return _arith(op, a, b, c, vals[op][q:q + 1], fmt)


def _arith(kind, a, b, c, rbits, fmt):
    res = float(to_float(rbits, fmt)[0])
    if math.isnan(res):
        return {"nan"}
    if kind == "sqrt":
        return {"inexact"} if math.isfinite(res) and Fraction(res) ** 2 != abs(Fraction(a)) else set()
    used = (a, b, c) if kind == "fma" else (a, b)
    if not all(math.isfinite(v) for v in used) or (kind == "div" and b == 0):
        return set()
    fa, fb = Fraction(a), Fraction(b)
    fc = Fraction(c) if kind == "fma" else None
    if kind == "add":
        exact, larger = fa + fb, max(abs(a), abs(b))
    elif kind == "mul":
        exact, larger = fa * fb, None
    elif kind == "fma":
        exact, larger = fa * fb + fc, float(max(abs(fa * fb), abs(fc)))
    else:
        exact, larger = fa / fb, None
    return _classes(exact, res, fmt, larger)


def test_operand_recipes_reach_every_class_each_operation_admits():
    assert set(WANTED) == {(s, op) for s in range(4) for op in fp.OPS[s]}
    missing = {k: set(v) for k, v in WANTED.items()}
    for r in range(64):
        for stage in range(4):
            todo = [op for op in fp.OPS[stage] if missing[(stage, op)]]
            if not todo:
                continue
            ops = fp.reference_operands(0, stage, r)
            vals = fp.reference_values(0, stage, r)
            for op in todo:
                need = missing[(stage, op)]
                for q in range(64 * fp.SLOTS_PER_LANE[stage]):
                    need -= _observe(stage, op, ops, vals, q)
                    if not need:
                        break
        if not any(missing.values()):
            print(f"every class reached after {r + 1} round(s)")
            break
    left = {f"{fp.STAGES[s]}.{op}": sorted(v) for (s, op), v in missing.items() if v}
    assert not left, left


def test_recipes_rotate_over_lanes_and_rounds():
    r = np.arange(8, dtype=np.uint32)
    for stage in range(4):
        rec = fp._recipes(stage, r)
        assert rec.shape == (8, 64 * fp.SLOTS_PER_LANE[stage])
        for q in (0, 63, 64, 255):
            assert sorted(rec[:, q].tolist()) == list(range(8))  # a lane meets all eight
        assert (np.bincount(rec[0], minlength=8) == rec.shape[1] // 8).all()
    assert np.array_equal(fp._recipes(2, r, 1), (fp._recipes(2, r, 0) + 3) & 7)


# -- digests -----------------------------------------------------------------------------------

def _fmix(h):
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _digest_of_values(seed, stage, r):
    vals = fp.reference_values(seed, stage, r)
    slots = 64 * fp.SLOTS_PER_LANE[stage]
    d = 0
    for k, op in enumerate(fp.OPS[stage]):
        for q, bits in enumerate(vals[op].tolist()):
            salt = (slots * k + q + 1) * 0x9E3779B9
            if stage == 1:
                d += _fmix((bits & 0xFFFFFFFF) ^ _fmix((bits >> 32) + salt))
            else:
                assert bits < 1 << 32
                d += _fmix(bits + salt)
    return d & 0xFFFFFFFF


def test_reference_digests_fold_the_values():
    ref = fp.reference_digests(0xDEADBEEF, 35)
    for r in (0, 34):
        assert ref[r].tolist() == [_digest_of_values(0xDEADBEEF, s, r) for s in range(4)]


def test_reference_digests_shape_determinism_seeds_and_period():
    a = fp.reference_digests(0, 5)
    assert a.shape == (5, 4) and a.dtype == np.uint32
    assert np.array_equal(a, fp.reference_digests(0, 5))
    b = fp.reference_digests(0xDEADBEEF, 5)
    assert (a != b).all()
    big = fp.reference_digests(0, fp.PERIOD + 40)
    assert big.shape == (fp.PERIOD + 40, 4) and big.flags.writeable
    assert np.array_equal(big[:5], a)
    assert np.array_equal(big[fp.PERIOD:], big[:40])  # inputs repeat
    for s in range(4):  # and not sooner
        assert len(set(big[:fp.PERIOD, s].tolist())) == fp.PERIOD
    z = fp.reference_digests(0, 0)
    assert z.shape == (0, 4) and z.dtype == np.uint32
    with pytest.raises(ValueError):
        fp.reference_digests(0, -1)
    assert fp.STAGES == ("f32", "f64", "packed", "cvt") and fp.PERIOD == 256
    # round r and r + PERIOD have the same values, not only the same digest
    for s in range(4):
        v0, v1 = fp.reference_values(3, s, 7), fp.reference_values(3, s, 7 + fp.PERIOD)
        assert all(np.array_equal(v0[k], v1[k]) for k in v0)
    with pytest.raises(ValueError):
        fp.reference_values(0, 4, 0)
    with pytest.raises(ValueError):
        fp.reference_values(0, 0, 65536)


def test_nan_results_are_canonical_and_zeros_keep_their_sign():
    seen_neg_zero = False
    for stage, fmt in ((0, fp.F32), (1, fp.F64)):
        for r in range(8):
            for op, bits in fp.reference_values(0, stage, r).items():
                mag = bits & np.uint64((1 << (fmt.width - 1)) - 1)
                nan = mag > np.uint64(fmt.emask << fmt.mbits)
                assert (bits[nan] == fmt.canonical_nan).all()
                seen_neg_zero |= bool((bits == np.uint64(1 << (fmt.width - 1))).any())
    assert seen_neg_zero


def test_inputs_differ_from_cuchecks_and_mxchecks():
    from kubegpu_amd.probe import cucheck as cc

    r = np.array([0], dtype=np.uint32)
    for s in range(4):
        mine = fp._slot_words(0, s, r)[0, 0, :8].astype(np.uint32)
        assert np.array_equal(mine, cc._words(0, 8 + s, r, 0, 8)[0])
        for other in range(8):
            assert not np.array_equal(mine, cc._words(0, other, r, 0, 8)[0])


def test_result_to_dict_round_trips_json_and_lazy_exports():
    import kubegpu_amd.probe as probe

    res = fp.FpcheckResult(ok=False, rounds=3, waves=48, mismatches=1, first_bad_round=1,
                           bad_stages=["packed"], records=[{"wave": 37}],
                           cus_covered=3, cu_count=256, bad_cus=["0/1/0/3"],
                           elapsed_s=0.5, f64_gops=1.5, waves_on=[0] * 1024)
    d = res.to_dict()
    assert json.loads(json.dumps(d)) == d and "waves_on" not in d
    assert {"f32_gops", "f64_gops", "packed_gops", "cvt_gops"} <= set(d)
    assert "mfma_f16_tflops" not in d
    assert fp.DEFAULT_ROUNDS % fp.PERIOD == 0 and fp.PERIOD <= fp.DEFAULT_ROUNDS <= 65536
    assert probe.FpcheckResult is fp.FpcheckResult
    assert probe.fpcheck_round is fp.fpcheck_round
    assert probe.run_fpcheck_subprocess is fp.run_fpcheck_subprocess
    assert probe.wave_values is fp.wave_values


# -- manager verdicts ------------------------------------------------------------------

def _mgr():
    mgr = create_device_plugin(FakeBackend(fixtures.fixture_8x_mi355x()))
    mgr.start()
    return mgr


def _node_info(mgr):
    ni = NodeInfo(name="n")
    mgr.update_node_info(ni)
    return ni


FAIL = {"ok": False, "mismatches": 4, "first_bad_round": 1, "bad_stages": ["packed"],
        "bad_cus": ["3/1/0/7"], "cus_covered": 256, "cu_count": 256, "rounds": 8}
PASS = {"ok": True, "mismatches": 0, "first_bad_round": None, "bad_stages": [],
        "bad_cus": [], "cus_covered": 256, "cu_count": 256, "rounds": 8}


def test_record_and_clear_flip_device_health(monkeypatch):
    from kubegpu_amd.api import utils

    lines = []
    monkeypatch.setattr(utils, "errorf", lambda fmt, *a: lines.append(fmt % a))
    mgr = _mgr()
    base = _node_info(mgr)
    uuid = sorted(mgr.gpus)[2]
    assert mgr.fpcheck_status(uuid) is None

    assert mgr.record_fpcheck(uuid, FAIL) is False
    health = mgr.device_health()
    assert health[uuid] is False and sum(health.values()) == 7
    assert mgr.gpus[uuid].healthy  # GpuInfo.healthy stays ECC-only
    ni = _node_info(mgr)
    assert ni.capacity == base.capacity
    assert ni.allocatable[RESOURCE_GPU] == base.allocatable[RESOURCE_GPU] - 1 == 7
    st = mgr.fpcheck_status(uuid)
    assert st["ok"] is False and st["mismatches"] == 4 and "timestamp" in st
    assert mgr.mxcheck_status(uuid) is None and mgr.cucheck_status(uuid) is None  # separate stores
    assert len(lines) == 1
    assert "fpcheck" in lines[0] and uuid in lines[0]
    assert "3/1/0/7" in lines[0] and "packed" in lines[0]

    assert mgr.record_fpcheck(uuid, PASS) is True
    assert mgr.device_health()[uuid] is True and len(lines) == 1
    assert _node_info(mgr).allocatable == base.allocatable
    mgr.record_fpcheck(uuid, FAIL)
    assert mgr.device_health()[uuid] is False
    assert mgr.clear_fpcheck(uuid) is True
    assert mgr.clear_fpcheck(uuid) is False
    assert mgr.fpcheck_status(uuid) is None
    assert mgr.device_health()[uuid] is True

    # any one failed verdict is enough
    mgr.record_fpcheck(uuid, FAIL)
    mgr.record_mxcheck(uuid, dict(PASS))
    assert mgr.device_health()[uuid] is False
    mgr.record_fpcheck(uuid, PASS)
    mgr.record_mxcheck(uuid, dict(FAIL, bad_stages=["mfma_f64"]))
    assert mgr.device_health()[uuid] is False
    mgr.clear_mxcheck(uuid)
    assert mgr.device_health()[uuid] is True

    with pytest.raises(KeyError):
        mgr.record_fpcheck("GPU-does-not-exist", FAIL)
    assert set(mgr.fpcheck) == {uuid}


def test_verdict_survives_rediscovery_and_goes_with_the_tombstone(monkeypatch):
    from kubegpu_amd.deviceplugin import manager as manager_mod

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    uuid = fix.devices[-1].uuid
    mgr.record_fpcheck(uuid, FAIL)
    mgr.update_gpu_info(force=True)
    assert mgr.device_health()[uuid] is False

    fix.devices.pop()  # the GPU vanishes
    mgr.update_gpu_info(force=True)
    assert uuid in mgr.vanished and mgr.fpcheck_status(uuid) is not None
    monkeypatch.setattr(manager_mod, "VANISHED_TTL_S", -1.0)
    mgr.update_gpu_info(force=True)
    assert uuid not in mgr.vanished
    assert mgr.fpcheck_status(uuid) is None


# -- fpcheck_round ---------------------------------------------------------------------

def test_round_pass_mismatch_and_idle_selection():
    from kubegpu_amd.metrics import Metrics

    mgr = _mgr()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.gpus[by_index[1]].in_use = True
    mgr.gpus[by_index[2]].process_count = 4
    calls = []

    def runner(index, rounds):
        calls.append((index, rounds))
        rec = dict(FAIL if index == 5 else PASS)
        rec["exit_code"] = 1 if index == 5 else 0
        return rec

    metrics = Metrics()
    out = fp.fpcheck_round(mgr, runner, metrics, rounds=8)
    assert calls == [(i, 8) for i in (0, 3, 4, 5, 6, 7)]  # idle_gpus, index order
    assert set(out) == {by_index[i] for i in (0, 3, 4, 5, 6, 7)}
    health = mgr.device_health()
    assert health[by_index[5]] is False
    assert all(health[by_index[i]] for i in (0, 1, 2, 3, 4, 6, 7))
    assert mgr.fpcheck_status(by_index[1]) is None
    assert mgr.mxcheck == {} and mgr.cucheck == {}
    assert metrics.gpu_fpcheck[by_index[5]]["mismatches"] == 4
    assert metrics.gpu_fpcheck[by_index[0]]["mismatches"] == 0
    assert metrics.gpu_fpcheck[by_index[0]]["cus_covered"] == 256
    assert metrics.gpu_fpcheck_errors == {} and metrics.gpu_mxcheck == {}

    calls.clear()
    fp.fpcheck_round(mgr, runner, None, rounds=8, max_process_count=None)
    assert [i for i, _ in calls] == [0, 2, 3, 4, 5, 6, 7]


def test_round_runner_errors_and_a_gpu_that_vanishes():
    import subprocess

    from kubegpu_amd.metrics import Metrics

    fix = fixtures.fixture_8x_mi355x()
    mgr = create_device_plugin(FakeBackend(fix))
    mgr.start()
    by_index = {g.index: u for u, g in mgr.gpus.items()}
    mgr.record_fpcheck(by_index[3], FAIL)  # an earlier verdict must stay too
    before = mgr.device_health()

    def runner(index, rounds):
        if index == 0:
            raise RuntimeError("boom")
        if index == 1:
            raise subprocess.TimeoutExpired("fpcheck", 1.0)
        if index in (2, 3):
            return {"error": "no GPU visible", "exit_code": 2}
        if index == 4:
            return "not a dict"
        if index == 7:  # gone while its child ran
            with mgr._lock:
                del mgr.gpus[by_index[7]]
        return dict(PASS, exit_code=0)

    metrics = Metrics()
    out = fp.fpcheck_round(mgr, runner, metrics, rounds=8)
    after = mgr.device_health()
    assert by_index[7] not in after
    assert after == {u: h for u, h in before.items() if u != by_index[7]}
    assert mgr.fpcheck_status(by_index[3])["ok"] is False
    for i in (0, 1, 2, 4):
        assert mgr.fpcheck_status(by_index[i]) is None
        assert out[by_index[i]]["exit_code"] == 2
    assert metrics.gpu_fpcheck_errors == {by_index[i]: 1 for i in (0, 1, 2, 3, 4)}
    assert set(metrics.gpu_fpcheck) == {by_index[i] for i in (5, 6)}
    assert by_index[7] not in out and by_index[7] not in mgr.fpcheck


# -- metrics -------------------------------------------------------------------------------

def test_metrics_setters_with_and_without_prometheus(monkeypatch):
    from kubegpu_amd import metrics as metrics_mod

    def exercise():
        m = metrics_mod.Metrics()
        m.set_gpu_fpcheck("GPU-a", 2, 255, 1700000000.0)
        m.inc_fpcheck_error("GPU-a")
        m.inc_fpcheck_error("GPU-a")
        assert m.gpu_fpcheck["GPU-a"] == {
            "mismatches": 2, "cus_covered": 255, "timestamp": 1700000000.0}
        assert m.gpu_fpcheck_errors["GPU-a"] == 2
        return m

    m = exercise()
    if metrics_mod._HAVE_PROM:
        reg = m.registry
        lab = {"uuid": "GPU-a"}
        assert reg.get_sample_value("kubegpu_amd_gpu_fpcheck_mismatches", lab) == 2.0
        assert reg.get_sample_value("kubegpu_amd_gpu_fpcheck_cus_covered", lab) == 255.0
        assert reg.get_sample_value(
            "kubegpu_amd_gpu_fpcheck_last_run_timestamp_seconds", lab) == 1700000000.0
        assert reg.get_sample_value("kubegpu_amd_gpu_fpcheck_errors_total", lab) == 2.0
        from prometheus_client import generate_latest

        assert b"/fpcheck/" in generate_latest(reg)  # the health gauge's help text
    monkeypatch.setattr(metrics_mod, "_HAVE_PROM", False)
    exercise()


# -- CLI and agent ----------------------------------------------------------------------------

def test_amddevs_fake_fpcheck_exits_2(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--fpcheck", "--rounds", "8"]) == 2
    cap = capsys.readouterr()
    assert "--fpcheck needs real GPUs" in cap.err
    assert cap.out == ""


def test_amddevs_health_shows_the_verdict(capsys):
    from kubegpu_amd.cli import amddevs

    assert amddevs.main(["--fake", "--health"]) == 0
    rows = json.loads(capsys.readouterr().out)
    assert len(rows) == 8 and all(r["fpcheck"] is None for r in rows.values())


def test_agent_oneshot_accepts_fpcheck_flags(sock_dir, capsys):
    from kubegpu_amd.server import agent

    base = ["--fake", "--no-register", "--metrics-port", "0", "--oneshot"]
    assert agent.main(base + ["--socket", str(sock_dir / "x.sock"),
                              "--fpcheck-interval", "600", "--fpcheck-rounds", "64",
                              "--fpcheck-max-procs", "2"]) == 0
    assert capsys.readouterr().out.count("agent ok: 8 GPUs") == 1


def test_fpcheck_cli_without_gpu_exits_2(capsys, monkeypatch):
    """No GPU (or no extension): one JSON line with an error, exit 2."""
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0")  # main() overwrites it
    assert fp.main(["--device", "0", "--rounds", "2"]) == 2
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert "error" in rec and rec["device"] == 0
