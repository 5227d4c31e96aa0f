// transcheck — integrity kernel for the transcendental units (gfx950),
// compiled into _gpuprobe.
//
// The twin of fpcheck.hip for the quarter-rate pipe fpcheck reaches only
// through the seeds of its division and square-root sequences: v_exp,
// v_log, v_rcp, v_rsq, v_sqrt, v_sin and v_cos in f32 and f16, v_rcp /
// v_rsq / v_sqrt in f64, and v_prng_b32.  IEEE 754 does not define these
// results, so the host has no exact table of its own.  They are
// deterministic though: one workgroup (transcheck_values_kernel) dumps
// every raw result of one period, the host bounds each against a
// high-precision reference and folds the dump into the digest table, and
// every wave of transcheck_kernel then has to reproduce that table bit
// for bit (probe/transcheck.py holds the definition of every operand,
// operation, bound and digest):
//   stage 0 f32    8 slots per lane, the seven f32 operations on each
//   stage 1 f16    8 slots per lane, the seven f16 operations on each; one
//                  period feeds every f16 bit pattern to every operation
//   stage 2 f64    4 slots per lane: rcp, rsq, sqrt
//   stage 3 chain  2 groups per lane of dependent sequences as workloads
//                  issue them (sigmoid, GELU, x * rsq, log-sum-exp, a
//                  rotary pair, an f16 softmax numerator, a prng chain),
//                  every intermediate transcendental result kept
// Inputs are word(56 + stage, r % TC_PERIOD, idx) of cucheck_common.h.
// Operands are put together from sign, exponent and mantissa fields with
// integer operations only, so host and device agree on them by
// construction.  Raw builtins give the bare instructions; no inline
// assembly.  Contraction is off and no fast-math flag is given.  Results
// are folded as raw bits, NaN payloads included.  Nothing here touches
// the LDS; the 160 KiB of dynamic LDS are asked for only so that one
// workgroup fills a CU.  Launch shape and accounting are cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

#define TC_DEV __device__ __forceinline__
// The chains' f32 multiplies and adds stay on the plain VALU: packed f32
// is fpcheck's ground, and a chain result must not depend on which pipe
// the compiler happened to pair two of them on.
#define TC_KERNEL \
  __global__ void __launch_bounds__(CU_BLOCK) __attribute__((target("no-packed-fp32-ops")))

typedef unsigned long long u64;

#define TC_STAGE0 56u  // stage number fed to cu_base() is TC_STAGE0 + stage
#define TC_PERIOD 128u
#define TC_ROWS 64u  // rows of 64 lanes per round in transcheck_values' output
#define TC_ROUND_WORDS (64u * TC_ROWS + 1u)  // the rows, then how many were filled
#define TC_SLOTS_F32 8u
#define TC_SLOTS_F16 8u
#define TC_SLOTS_F64 4u
#define TC_GROUPS 2u
#define TC_CHAIN_ROWS 24u  // rows of one group of stage 3
static_assert(7u * TC_SLOTS_F32 <= TC_ROWS && 7u * TC_SLOTS_F16 <= TC_ROWS &&
                  6u * TC_SLOTS_F64 <= TC_ROWS && TC_GROUPS * TC_CHAIN_ROWS <= TC_ROWS,
              "transcheck_values' rows must hold every stage");

// f32 constants of the chains by their bits (probe/transcheck.py: CONST)
#define TC_LOG2E 0x3FB8AA3Bu    // log2(e)
#define TC_GELU_2K 0x3FCC422Au  // 2 sqrt(2 / pi)
#define TC_GELU_C3 0x3D372713u  // 0.044715
#define TC_EPS 0x358637BDu      // 1e-6
#define TC_LOG2E_H 0x3DC5u      // log2(e) in f16

#if __HIP_DEVICE_COMPILE__

// Where a stage's values go: into the digest, or into the element dump
// (row `slot`, column lane).
// (an aggregate: an implicit constructor would not carry the kernels'
// target attribute and would stay a call with the digest in scratch)
struct TcFold {
  u32 d;
  TC_DEV void put(u32 slot, u32 lane, u32 v) { d += cu_fmix32(v + cu_salt(64u * slot + lane)); }
};

struct TcDump {
  u32* out;
  TC_DEV void put(u32 slot, u32 lane, u32 v) { out[64u * slot + lane] = v; }
};

TC_DEV float tc_f32(u32 b) { return __builtin_bit_cast(float, b); }
TC_DEV u32 tc_bits(float x) { return __builtin_bit_cast(u32, x); }
TC_DEV double tc_f64(u64 b) { return __builtin_bit_cast(double, b); }
TC_DEV u64 tc_bits(double x) { return __builtin_bit_cast(u64, x); }
TC_DEV _Float16 tc_f16(u32 b) { return __builtin_bit_cast(_Float16, (unsigned short)b); }
// its own name: the f16 builtins return __fp16, which an overload set
// would widen to float
TC_DEV u32 tc_hbits(_Float16 x) { return (u32)__builtin_bit_cast(unsigned short, x); }

TC_DEV u32 tc_pack32(u32 s, u32 e, u32 m) { return (s << 31) | (e << 23) | m; }
TC_DEV u64 tc_pack64(u64 s, u64 e, u64 m) { return (s << 63) | (e << 52) | m; }
TC_DEV u32 tc_pack16(u32 s, u32 e, u32 m) { return (s << 15) | (e << 10) | m; }

// ±0, ±Inf, NaN, ±1 or a mid-range value by a 3-bit code, sign kept
TC_DEV u32 tc_special32(u32 s, u32 e, u32 m, u32 code) {
  if (code == 0u || code == 5u) return tc_pack32(s, 0u, 0u);
  if (code == 1u || code == 6u) return tc_pack32(s, 255u, 0u);
  if (code == 2u) return tc_pack32(s, 255u, m | 1u);
  if (code == 3u) return tc_pack32(s, 127u, 0u);
  return tc_pack32(s, 119u + (e & 15u), m);
}

TC_DEV u64 tc_special64(u64 s, u64 e, u64 m, u32 code) {
  if (code == 0u || code == 5u) return tc_pack64(s, 0u, 0u);
  if (code == 1u || code == 6u) return tc_pack64(s, 2047u, 0u);
  if (code == 2u) return tc_pack64(s, 2047u, m | 1u);
  if (code == 3u) return tc_pack64(s, 1023u, 0u);
  return tc_pack64(s, 1015u + (e & 15u), m);
}

// The f32 operand of recipe k = 0..7; probe/transcheck.py:_operand32 is
// the definition.
TC_DEV u32 tc_operand32(u32 k, u32 ra, u32 sel) {
  const u32 s = ra >> 31, e = (ra >> 23) & 0xFFu, m = ra & 0x7FFFFFu;
  switch (k) {
    case 0u:
      return tc_pack32(s, 1u + e % 254u, m);
    case 1u: {
      const u32 ee = e % 7u;  // an exact integer of ee + 1 bits
      if (sel & 1u) return tc_pack32(s, 127u + ee, m & ~((1u << (23u - ee)) - 1u));
      return tc_pack32(s, 117u + e % 17u, m);
    }
    case 2u: {
      const u32 step = ((1u << 23) | m) >> (1u + (sel & 31u) % 20u);
      return (sel >> 5) & 1u ? 0x3F800000u - step : 0x3F800000u + step;
    }
    case 3u: {
      const u32 v = sel & 3u;
      if (v == 0u) return tc_pack32(s, 114u + e % 21u, m);
      // n / 8 for n = 1..2048, and one step either side
      const u32 n = 1u + (ra & 2047u), top = 31u - (u32)__builtin_clz(n);
      const u32 x = tc_pack32(s, 124u + top, (n << (23u - top)) & 0x7FFFFFu);
      return v == 1u ? x : v == 2u ? x + 1u : x - 1u;
    }
    case 4u: {
      const u32 ex = 1u + e % 253u;
      return tc_pack32(s, sel & 1u ? ex | 1u : ex, 0u);
    }
    case 5u:
      return tc_pack32(s, 0u, (m >> (sel & 15u)) | 1u);
    case 6u:
      return tc_pack32(s, 136u + e % 118u, m);
    default:
      return tc_special32(s, e, m, (sel >> 16) & 7u);
  }
}

// The f64 operand of recipe k; probe/transcheck.py:_operand64.
TC_DEV u64 tc_operand64(u32 k, u64 ra, u32 sel) {
  const u64 s = ra >> 63, e = (ra >> 52) & 0x7FFull, m = ra & 0xFFFFFFFFFFFFFull;
  const u64 one = 0x3FF0000000000000ull;
  switch (k) {
    case 0u:
      return tc_pack64(s, 1u + e % 2046u, m);
    case 1u:
      return tc_pack64(s, 1015u + (e & 15u), m);
    case 2u: {
      const u64 step = ((1ull << 52) | m) >> (1u + (sel & 63u) % 40u);
      return (sel >> 6) & 1u ? one - step : one + step;
    }
    case 3u:
      return tc_pack64(s, 1023u + (e & 7u), m & ~((1ull << 40) - 1u));
    case 4u: {
      const u64 ex = 1u + e % 2045u;
      return tc_pack64(s, sel & 1u ? ex | 1u : ex, 0u);
    }
    case 5u:
      return tc_pack64(s, 0u, (m >> (sel & 31u)) | 1u);
    case 6u:
      return sel & 1u ? tc_pack64(s, 1u + (e & 7u), m) : tc_pack64(s, 2046u - (e & 7u), m);
    default:
      return tc_special64(s, e, m, (sel >> 16) & 7u);
  }
}

// f16 code i of the exhaustive walk: a bijection of 0..65535
TC_DEV u32 tc_perm16(u32 i) { return ((i * 40503u) & 0xFFFFu) ^ 0xA5C3u; }

TC_DEV u32 tc_word(u32 base, u32 idx) { return cu_fmix32(base + idx); }

// ---- stage 0: the seven f32 operations

template <typename SINK>
TC_DEV u32 tc_stage_f32(u32 base, u32 rp, u32 lane, SINK& sink) {
  u32 n = 0;
#pragma unroll 1
  for (u32 j = 0; j < TC_SLOTS_F32; ++j) {
    const u32 q = 64u * j + lane;
    const float x = tc_f32(tc_operand32((lane + j + rp) & 7u, tc_word(base, 2u * q),
                                        tc_word(base, 2u * q + 1u)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_exp2f(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_logf(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_rcpf(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_rsqf(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_sqrtf(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_sinf(x)));
    sink.put(n++, lane, tc_bits(__builtin_amdgcn_cosf(x)));
  }
  return n;
}

// ---- stage 1: the seven f16 operations, exhaustive over one period

template <typename SINK>
TC_DEV u32 tc_stage_f16(u32 rp, u32 lane, SINK& sink) {
  u32 n = 0;
#pragma unroll 1
  for (u32 j = 0; j < TC_SLOTS_F16; ++j) {
    const _Float16 x = tc_f16(tc_perm16(512u * rp + 64u * j + lane));
    sink.put(n++, lane, tc_hbits(__builtin_exp2f16(x)));
    sink.put(n++, lane, tc_hbits(__builtin_log2f16(x)));
    sink.put(n++, lane, tc_hbits(__builtin_amdgcn_rcph(x)));
    sink.put(n++, lane, tc_hbits(__builtin_amdgcn_rsqh(x)));
    sink.put(n++, lane, tc_hbits(__builtin_amdgcn_sqrth(x)));
    sink.put(n++, lane, tc_hbits(__builtin_amdgcn_sinh(x)));
    sink.put(n++, lane, tc_hbits(__builtin_amdgcn_cosh(x)));
  }
  return n;
}

// ---- stage 2: rcp, rsq, sqrt in f64

template <typename SINK>
TC_DEV void tc_put64(SINK& sink, u32& n, u32 lane, double v) {
  const u64 b = tc_bits(v);
  sink.put(n++, lane, (u32)b);
  sink.put(n++, lane, (u32)(b >> 32));
}

template <typename SINK>
TC_DEV u32 tc_stage_f64(u32 base, u32 rp, u32 lane, SINK& sink) {
  u32 n = 0;
#pragma unroll 1
  for (u32 j = 0; j < TC_SLOTS_F64; ++j) {
    const u32 q = 64u * j + lane;
    const u64 ra = (u64)tc_word(base, 4u * q) | ((u64)tc_word(base, 4u * q + 1u) << 32);
    const double x = tc_f64(tc_operand64((lane + j + rp) & 7u, ra, tc_word(base, 4u * q + 2u)));
    tc_put64(sink, n, lane, __builtin_amdgcn_rcp(x));
    tc_put64(sink, n, lane, __builtin_amdgcn_rsq(x));
    tc_put64(sink, n, lane, __builtin_amdgcn_sqrt(x));
  }
  return n;
}

// ---- stage 3: dependent sequences

// w at exponent field lo + (E w mod span), sign and mantissa kept
TC_DEV float tc_ranged(u32 w, u32 lo, u32 span) {
  return tc_f32(tc_pack32(w >> 31, lo + ((w >> 23) & 0xFFu) % span, w & 0x7FFFFFu));
}

TC_DEV _Float16 tc_ranged16(u32 h) {
  return tc_f16(tc_pack16((h >> 15) & 1u, 12u + ((h >> 10) & 31u) % 6u, h & 0x3FFu));
}

template <typename SINK>
TC_DEV u32 tc_stage_chain(u32 base, u32 lane, SINK& sink) {
#pragma clang fp contract(off)
  const float log2e = tc_f32(TC_LOG2E);
  u32 n = 0;
#pragma unroll 1
  for (u32 j = 0; j < TC_GROUPS; ++j) {
    const u32 w = base + 8u * (64u * j + lane);
    const float x = tc_ranged(cu_fmix32(w), 124u, 6u);  // 1/8 <= |x| < 8
    {  // sigmoid
      const float e = __builtin_amdgcn_exp2f(-x * log2e);
      sink.put(n++, lane, tc_bits(e));
      sink.put(n++, lane, tc_bits(__builtin_amdgcn_rcpf(1.0f + e)));
    }
    {  // tanh-form GELU as x * sigmoid(2 u), the form without cancellation
      const float u2 = tc_f32(TC_GELU_2K) * (x + tc_f32(TC_GELU_C3) * (x * x * x));
      const float e = __builtin_amdgcn_exp2f(-u2 * log2e);
      const float s = __builtin_amdgcn_rcpf(1.0f + e);
      sink.put(n++, lane, tc_bits(e));
      sink.put(n++, lane, tc_bits(s));
      sink.put(n++, lane, tc_bits(x * s));
    }
    {  // x * rsq(x^2 + eps)
      const float q = __builtin_amdgcn_rsqf(x * x + tc_f32(TC_EPS));
      sink.put(n++, lane, tc_bits(q));
      sink.put(n++, lane, tc_bits(x * q));
    }
    {  // two-term log-sum-exp in base 2
      const float a = tc_ranged(cu_fmix32(w + 1u), 125u, 6u);  // 1/4 <= |a|, |b| < 16
      const float b = tc_ranged(cu_fmix32(w + 2u), 125u, 6u);
      const float m = __builtin_fmaxf(a, b);
      const float ea = __builtin_amdgcn_exp2f(a - m), eb = __builtin_amdgcn_exp2f(b - m);
      const float l = __builtin_amdgcn_logf(ea + eb);
      sink.put(n++, lane, tc_bits(ea));
      sink.put(n++, lane, tc_bits(eb));
      sink.put(n++, lane, tc_bits(l));
      sink.put(n++, lane, tc_bits(m + l));
    }
    {  // rotary pair, t in revolutions, 2^-10 <= |t| < 1
      const float t = tc_ranged(cu_fmix32(w + 3u), 117u, 10u);
      const float rx = tc_ranged(cu_fmix32(w + 4u), 125u, 4u);  // 1/4 <= |rx|, |ry| < 4
      const float ry = tc_ranged(cu_fmix32(w + 5u), 125u, 4u);
      const float c = __builtin_amdgcn_cosf(t), s = __builtin_amdgcn_sinf(t);
      sink.put(n++, lane, tc_bits(c));
      sink.put(n++, lane, tc_bits(s));
      sink.put(n++, lane, tc_bits(rx * c - ry * s));
      sink.put(n++, lane, tc_bits(rx * s + ry * c));
    }
    {  // f16 softmax numerator of the first of two logits, 1/8 <= |h| < 8
      const u32 hw = cu_fmix32(w + 6u);
      const _Float16 h0 = tc_ranged16(hw), h1 = tc_ranged16(hw >> 16);
      const _Float16 hm = h0 > h1 ? h0 : h1;
      sink.put(n++, lane, tc_hbits(__builtin_exp2f16((h0 - hm) * tc_f16(TC_LOG2E_H))));
    }
    {  // eight dependent steps of the LFSR instruction
      u32 p = cu_fmix32(w + 7u);
#pragma unroll
      for (u32 i = 0; i < 8u; ++i) {
        p = __builtin_amdgcn_prng_b32(p);
        sink.put(n++, lane, p);
      }
    }
  }
  return n;
}

// One stage for one round; returns the number of rows it filled.
template <u32 STAGE, typename SINK>
TC_DEV u32 tc_stage(u32 seed, u32 rp, u32 lane, SINK& sink) {
  const u32 base = cu_base(seed, TC_STAGE0 + STAGE, rp);
  if constexpr (STAGE == 0u) return tc_stage_f32(base, rp, lane, sink);
  else if constexpr (STAGE == 1u) return tc_stage_f16(rp, lane, sink);
  else if constexpr (STAGE == 2u) return tc_stage_f64(base, rp, lane, sink);
  else return tc_stage_chain(base, lane, sink);
}

#endif  // __HIP_DEVICE_COMPILE__

TC_KERNEL
transcheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % TC_PERIOD;
    TcFold f0 = {0}, f1 = {0}, f2 = {0}, f3 = {0};
    tc_stage<0u>(a.seed, rp, lane, f0);
    tc_stage<1u>(a.seed, rp, lane, f1);
    tc_stage<2u>(a.seed, rp, lane, f2);
    tc_stage<3u>(a.seed, rp, lane, f3);
    u32 dig[N_STAGES] = {wave_sum(f0.d), wave_sum(f1.d), wave_sum(f2.d), wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// The golden pass: one workgroup; wave w writes every value it would fold
// for `stage` in rounds first + w + 16 k < first + n_rounds, round k's
// block at out + k * TC_ROUND_WORDS (row `slot`, column lane, then the
// number of rows filled).  Wave 0 leaves where it ran (xcc << 16 |
// HW_ID[15:0]) behind the last block.
TC_KERNEL
transcheck_values_kernel(u32 seed, u32 stage, u32 first, u32 n_rounds, u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  const u32 lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
  if (threadIdx.x == 0) {
    const u32 hw_id = __builtin_amdgcn_s_getreg(GETREG_IMMED(32 - 1, 0, HW_ID));
    const u32 xcc = __builtin_amdgcn_s_getreg(
        GETREG_IMMED(XCC_ID_XCC_ID_SIZE - 1, XCC_ID_XCC_ID_OFFSET, XCC_ID));
    out[(size_t)n_rounds * TC_ROUND_WORDS] = (xcc << 16) | (hw_id & 0xFFFFu);
  }
  for (u32 k = wave; k < n_rounds; k += CU_WAVES) {
    const u32 rp = (first + k) % TC_PERIOD;
    TcDump sink;
    sink.out = out + (size_t)k * TC_ROUND_WORDS;
    u32 n;
    if (stage == 0u) n = tc_stage<0u>(seed, rp, lane, sink);
    else if (stage == 1u) n = tc_stage<1u>(seed, rp, lane, sink);
    else if (stage == 2u) n = tc_stage<2u>(seed, rp, lane, sink);
    else n = tc_stage<3u>(seed, rp, lane, sink);
    if (lane == 0u) sink.out[64u * TC_ROWS] = n;
  }
#endif
}

// ---------------------------------------------------------------- host

CucheckOut transcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                          int64_t blocks_arg, int64_t max_records,
                          c10::optional<at::Tensor> dump, c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("transcheck", expected, seed_arg, rounds, blocks_arg, max_records,
                          dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(transcheck_kernel, l, MAX_LDS_BYTES);
}

// What one wave folds for one stage in n_rounds rounds from first_round
// on, as an int32 tensor on the current GPU: per round TC_ROWS rows of 64
// lanes and the number of rows the stage filled; then where wave 0 ran.
at::Tensor transcheck_values(int64_t seed_arg, int64_t stage, int64_t first_round,
                             int64_t n_rounds) {
  cu_check_wave_args("transcheck", seed_arg, stage, first_round);
  TORCH_CHECK(n_rounds >= 1 && n_rounds <= TC_PERIOD && first_round + n_rounds <= MAX_ROUNDS,
              "transcheck: n_rounds must be in 1..", TC_PERIOD, " and end by round ",
              MAX_ROUNDS, ", got ", n_rounds);
  at::Tensor out = at::zeros({n_rounds * (int64_t)TC_ROUND_WORDS + 1},
                             at::TensorOptions().dtype(at::kInt).device(at::kCUDA));
  return cu_launch_values(transcheck_values_kernel, CU_BLOCK, 0, out, (u32)seed_arg,
                          (u32)stage, (u32)first_round, (u32)n_rounds, (u32*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/transcheck_mi355x.json).
void bind_transcheck(py::module_& m) {
  m.def("transcheck_run", &transcheck_run,
        "transcendental-unit integrity run -> (mismatches, first_bad_round, stage_mask, "
        "records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("max_records") = 16, py::arg("dump") = py::none(),
        py::arg("inject") = py::none());
  m.def("transcheck_values", &transcheck_values,
        "values one wave folds for one stage, per round int32 [64 rows * 64 lanes + 1], "
        "then the hardware id of wave 0",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("first_round"), py::arg("n_rounds"));
}
