// fpcheck — bit-exact IEEE rounding kernel for the vector FP units
// (gfx950), compiled into _gpuprobe.
//
// The twin of cucheck.hip and mxcheck.hip for the logic those two leave
// out on purpose: they feed the floating-point hardware only operands
// whose every intermediate is an exactly representable integer.  Here
// every wave of the launch runs add, mul, fma, div and sqrt in f32 and
// f64, the packed f16 and f32 operations and the conversion and
// round-to-integral instructions on operands built to round: ties and
// near-ties, massive cancellation, subnormal operands and results,
// overflow, underflow, zeros, Inf and NaN.  IEEE 754 defines every one
// of these results bit for bit, so the host computes them in numpy
// (probe/fpcheck.py:reference_values is the definition, its module
// docstring defines every recipe) and the four 32-bit digests per round
// are compared exactly:
//   stage 0 f32     8 slots per lane: a+b, a*b, fma(a,b,c), a/b, sqrt|a|
//   stage 1 f64     4 slots per lane: the same five
//   stage 2 packed  8 slots per lane, two triples each: packed f16 and
//                   packed f32 fma, mul, add
//   stage 3 cvt     8 slots per lane: f32->f16, f32->bf16, f64->f32,
//                   u32->f32, i32->f32, f32->i32, rint, floor, ceil, trunc
// Inputs are word(8 + stage, r % FP_PERIOD, idx) of cucheck_common.h, so
// they differ from cucheck's and mxcheck's and repeat with FP_PERIOD
// rounds.  Operands are put together from sign, exponent and mantissa
// fields with integer operations only, so host and device agree on them
// by construction.  Contraction is off and no fast-math flag is given:
// a*b and a+b stay apart, fused operations are asked for by builtin.
//
// Launch shape and accounting are cucheck's: 1024-thread workgroups (16
// waves), grid 0 = one workgroup per CU, each wave reads HW_ID / XCC_ID
// once and is counted in waves_on.  Nothing here touches the LDS; the
// 160 KiB of dynamic LDS are asked for only so that one workgroup fills
// a CU and the default grid lands one workgroup on every CU.  No wave
// waits for another.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

typedef unsigned long long u64;
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

#define FP_STAGE0 8u  // stage number fed to cu_base() is FP_STAGE0 + stage
#define FP_PERIOD 256u
#define FP_WORDS 16u  // words per slot

// Bit fields of a binary format held in the low W bits of U.
template <typename UT, int EB, int MB>
struct Fp {
  typedef UT U;
  static constexpr int W = 1 + EB + MB;
  static constexpr int Mb = MB;
  static constexpr U B = (U(1) << (EB - 1)) - 1;
  static constexpr U X = (U(1) << EB) - 1;
  static constexpr U MM = (U(1) << MB) - 1;
  static constexpr U WM = ~U(0) >> (8 * sizeof(U) - W);
  static constexpr U SIGN = U(1) << (W - 1);
  static constexpr U QNAN = (X << MB) | (U(1) << (MB - 1));

  static __device__ __forceinline__ U S(U x) { return (x >> (W - 1)) & 1; }
  static __device__ __forceinline__ U E(U x) { return (x >> MB) & X; }
  static __device__ __forceinline__ U M(U x) { return x & MM; }
  static __device__ __forceinline__ U pack(U s, U e, U m) {
    return ((s << (W - 1)) | (e << MB) | m) & WM;
  }
  static __device__ __forceinline__ U mid(U x) { return at(x, B - 8, 15); }
  // x moved to exponent field lo + (E x & mask)
  static __device__ __forceinline__ U at(U x, U lo, U mask) {
    return pack(S(x), lo + (E(x) & mask), M(x));
  }
  // half an ulp of a number with exponent field e, one step above, one below
  static __device__ __forceinline__ U half(U s, U e, u32 t) {
    if (t == 0) return pack(s, e - (MB + 1), 0);
    if (t == 1) return pack(s, e - (MB + 1), 1);
    return pack(s, e - (MB + 2), MM);
  }
  static __device__ __forceinline__ U special(U x, u32 code) {
    U s = S(x);
    if (code == 0 || code == 5) return pack(s, 0, 0);
    if (code == 1 || code == 6) return pack(s, X, 0);
    if (code == 2) return pack(s, X, M(x) | 1);
    if (code == 3) return pack(s, B, 0);
    return mid(x);
  }
  static __device__ __forceinline__ U canon(U bits) {
    return (bits & (WM >> 1)) > (X << MB) ? QNAN : bits;
  }
};

typedef Fp<u32, 5, 10> FpH;
typedef Fp<u32, 8, 23> FpS;
typedef Fp<u64, 11, 52> FpD;

// (a, b, c) by recipe 0..7; probe/fpcheck.py:_triple is the definition.
template <typename F>
__device__ __forceinline__ void fp_triple(u32 recipe, typename F::U ra, typename F::U rb,
                                          typename F::U rc, u32 sel, typename F::U& a,
                                          typename F::U& b, typename F::U& c) {
  typedef typename F::U U;
  constexpr int Mb = F::Mb;
  const U B = F::B, X = F::X;
  const u32 v = sel & 3u, t = ((sel >> 2) & 255u) % 3u;
  const u32 p = (sel >> 10) & 7u, cm = (sel >> 13) & 3u;
  switch (recipe) {
    case 0:
      a = ra, b = rb, c = rc;
      break;
    case 1:
      a = F::mid(ra), b = F::mid(rb), c = F::mid(rc);
      break;
    case 2:
      if (v == 1) {
        constexpr int h = (Mb - 1) / 2, sh = Mb - h;
        U ha = (F::M(ra) >> sh) << sh, hb = (F::M(rb) >> sh) << sh;
        a = F::pack(F::S(ra), B + (F::E(ra) & 7), ha);
        b = F::pack(F::S(rb), B + (F::E(rb) & 7), hb);
        U prod = ((U(1) << h) | (ha >> sh)) * ((U(1) << h) | (hb >> sh));
        U carry = (prod >> (2 * h + 1)) & 1;
        c = F::half(F::S(rc), F::E(a) + F::E(b) - B + carry, t);
      } else if (v == 2) {
        constexpr int ka = (Mb + 2) / 2, kb = Mb + 2 - ka;
        const int sa = Mb + 1 - ka, sb = Mb + 1 - kb - (t != 0 ? 1 : 0);
        a = F::pack(F::S(ra), B - 4 + (F::E(ra) & 7), ((F::M(ra) >> sa) | 1) << sa);
        b = F::pack(F::S(rb), B - 4 + (F::E(rb) & 7), ((F::M(rb) >> sb) | 1) << sb);
        c = F::mid(rc);
      } else {
        a = F::at(ra, B, 7);
        b = F::half(F::S(rb), F::E(a), t);
        c = F::mid(rc);
      }
      break;
    case 3:
      if (v & 1u) {
        a = F::at(ra, B - 4, 7);
        // b keeps 10 mantissa bits: the product fits 64 bits in every format
        U mb10 = (F::M(rb) >> (Mb - 10)) << (Mb - 10);
        b = F::pack(F::S(rb), B - 4 + (F::E(rb) & 7), mb10);
        u64 prod = (u64)((U(1) << Mb) | F::M(a)) * (u64)((U(1) << 10) | (mb10 >> (Mb - 10)));
        U carry = (U)((prod >> (Mb + 11)) & 1);
        U top = (U)(prod >> (10 + carry));
        c = F::pack(1 ^ F::S(ra) ^ F::S(rb), F::E(a) + F::E(b) - B + carry, top & F::MM) ^
            (U)(p & 3u);
      } else {
        a = F::mid(ra);
        b = a ^ F::SIGN ^ (U)p;
        c = F::mid(rc);
      }
      break;
    case 4:
      a = (v & 1u) ? F::pack(F::S(ra), 0, F::M(ra)) : F::at(ra, 1, 3);
      b = (v & 2u) ? F::pack(F::S(rb), 0, F::M(rb)) : F::at(rb, B - 2, 3);
      c = (cm & 1u) ? F::pack(F::S(rc), 0, F::M(rc)) : F::at(rc, 1, 3);
      break;
    case 5:
      a = F::pack(F::S(ra), X - 1 - (F::E(ra) & 1), F::M(ra));
      if (v == 1)
        b = F::at(rb, B, 3);
      else if (v == 2)
        b = F::pack(F::S(rb), B - 1 - (F::E(rb) & 3), F::M(rb));
      else
        b = F::pack(F::S(rb), X - 1 - (F::E(rb) & 1), F::M(rb));
      c = F::pack(F::S(rc), X - 1 - (F::E(rc) & 1), F::M(rc));
      break;
    case 6:
      a = F::at(ra, 1, 7);
      if (v == 0)
        b = F::at(rb, B - Mb - 4, 7);
      else if (v == 1)
        b = F::pack(F::S(rb), B - (F::E(rb) & 7), F::M(rb));
      else if (v == 2)
        b = F::at(rb, B + 1, 7);
      else
        b = F::at(rb, B + Mb - 2, 7);
      if (cm == 0)
        c = F::pack(F::S(rc), 0, 0);
      else if (cm == 1)
        c = F::pack(F::S(rc), 0, F::M(rc));
      else
        c = F::at(rc, 1, 3);
      break;
    default:
      a = F::special(ra, (sel >> 16) & 7u);
      b = F::special(rb, (sel >> 19) & 7u);
      c = F::special(rc, (sel >> 22) & 7u);
      break;
  }
}

// Stage 1's fma operand: exponents more than 200 from the bias are
// remapped, so that the host's error-free splitting stays in range.
__device__ __forceinline__ u64 fp_fma64_operand(u64 x) {
  u64 e = FpD::E(x);
  return (e + 200 < FpD::B || e > FpD::B + 200) ? FpD::at(x, FpD::B - 64, 127) : x;
}

// Where a stage's results go: into the digest, or into the element dump.
struct FpFold {
  u32 d = 0;
  u32 slots;
  __device__ __forceinline__ void put(u32 op, u32 q, u32 bits) {
    d += cu_fmix32(bits + cu_salt(slots * op + q));
  }
  __device__ __forceinline__ void put64(u32 op, u32 q, u64 bits) {
    d += cu_fmix32((u32)bits ^ cu_fmix32((u32)(bits >> 32) + cu_salt(slots * op + q)));
  }
};

struct FpDump {
  u64* out;
  u32 slots;
  __device__ __forceinline__ void put(u32 op, u32 q, u32 bits) { out[slots * op + q] = bits; }
  __device__ __forceinline__ void put64(u32 op, u32 q, u64 bits) {
    out[slots * op + q] = bits;
  }
};

__device__ __forceinline__ u32 fp_word(u32 base, u32 q, u32 k) {
  return cu_fmix32(base + FP_WORDS * q + k);
}

__device__ __forceinline__ u64 fp_word64(u32 base, u32 q, u32 k) {
  return (u64)fp_word(base, q, k) | ((u64)fp_word(base, q, k + 1) << 32);
}

__device__ __forceinline__ float fp_f32(u32 b) { return __builtin_bit_cast(float, b); }
__device__ __forceinline__ u32 fp_bits(float x) {
  return FpS::canon(__builtin_bit_cast(u32, x));
}
__device__ __forceinline__ double fp_f64(u64 b) { return __builtin_bit_cast(double, b); }
__device__ __forceinline__ u64 fp_bits(double x) {
  return FpD::canon(__builtin_bit_cast(u64, x));
}
__device__ __forceinline__ _Float16 fp_f16(u32 b) {
  return __builtin_bit_cast(_Float16, (unsigned short)b);
}
__device__ __forceinline__ u32 fp_bits(_Float16 x) {
  return FpH::canon((u32)__builtin_bit_cast(unsigned short, x));
}

// stage 0: f32
template <typename SINK>
__device__ __forceinline__ void fp_stage_f32(u32 base, u32 rp, u32 lane, SINK& sink) {
#pragma clang fp contract(off)
  sink.slots = 64 * 8;
#pragma unroll 1
  for (u32 j = 0; j < 8; ++j) {
    const u32 q = 64 * j + lane;
    u32 a, b, c;
    fp_triple<FpS>((lane + j + rp) & 7u, fp_word(base, q, 0), fp_word(base, q, 2),
                   fp_word(base, q, 4), fp_word(base, q, 6), a, b, c);
    const float x = fp_f32(a), y = fp_f32(b), z = fp_f32(c);
    // an opaque copy for the sum: with the same two operands feeding the
    // sum and the product the compiler issues both on the packed pipe
    // (stage 2's ground) and v_add_f32 / v_mul_f32 would not run at all
    float xs = x;
    asm volatile("" : "+v"(xs));
    sink.put(0, q, fp_bits(xs + y));
    sink.put(1, q, fp_bits(x * y));
    sink.put(2, q, fp_bits(__builtin_fmaf(x, y, z)));
    sink.put(3, q, fp_bits(x / y));
    sink.put(4, q, fp_bits(__builtin_sqrtf(__builtin_fabsf(x))));
  }
}

// stage 1: f64
template <typename SINK>
__device__ __forceinline__ void fp_stage_f64(u32 base, u32 rp, u32 lane, SINK& sink) {
#pragma clang fp contract(off)
  sink.slots = 64 * 4;
#pragma unroll 1
  for (u32 j = 0; j < 4; ++j) {
    const u32 q = 64 * j + lane;
    u64 a, b, c;
    fp_triple<FpD>((lane + j + rp) & 7u, fp_word64(base, q, 0), fp_word64(base, q, 2),
                   fp_word64(base, q, 4), fp_word(base, q, 6), a, b, c);
    const double x = fp_f64(a), y = fp_f64(b);
    sink.put64(0, q, fp_bits(x + y));
    sink.put64(1, q, fp_bits(x * y));
    sink.put64(2, q, fp_bits(__builtin_fma(fp_f64(fp_fma64_operand(a)),
                                           fp_f64(fp_fma64_operand(b)),
                                           fp_f64(fp_fma64_operand(c)))));
    sink.put64(3, q, fp_bits(x / y));
    sink.put64(4, q, fp_bits(__builtin_sqrt(__builtin_fabs(x))));
  }
}

// stage 2: packed f16 and packed f32, two triples per slot
template <typename SINK>
__device__ __forceinline__ void fp_stage_packed(u32 base, u32 rp, u32 lane, SINK& sink) {
#pragma clang fp contract(off)
  sink.slots = 64 * 8;
#pragma unroll 1
  for (u32 j = 0; j < 8; ++j) {
    const u32 q = 64 * j + lane;
    f16x2 ha, hb, hc;
    f32x2 fa, fb, fc;
#pragma unroll
    for (u32 e = 0; e < 2; ++e) {
      const u32 recipe = (lane + j + rp + 3 * e) & 7u;
      const u32 ra = fp_word(base, q, 8 * e), rb = fp_word(base, q, 8 * e + 2);
      const u32 rc = fp_word(base, q, 8 * e + 4), sel = fp_word(base, q, 8 * e + 6);
      u32 a, b, c;
      fp_triple<FpH>(recipe, ra & 0xFFFFu, rb & 0xFFFFu, rc & 0xFFFFu, sel, a, b, c);
      ha[e] = fp_f16(a), hb[e] = fp_f16(b), hc[e] = fp_f16(c);
      fp_triple<FpS>(recipe, ra, rb, rc, sel, a, b, c);
      fa[e] = fp_f32(a), fb[e] = fp_f32(b), fc[e] = fp_f32(c);
    }
    const f16x2 hf = __builtin_elementwise_fma(ha, hb, hc), hm = ha * hb, hs = ha + hb;
    sink.put(0, q, fp_bits(hf[0]) | (fp_bits(hf[1]) << 16));
    sink.put(1, q, fp_bits(hm[0]) | (fp_bits(hm[1]) << 16));
    sink.put(2, q, fp_bits(hs[0]) | (fp_bits(hs[1]) << 16));
    const f32x2 ff = __builtin_elementwise_fma(fa, fb, fc), fm = fa * fb, fs = fa + fb;
    sink.put(3, q, fp_bits(ff[0]));
    sink.put(4, q, fp_bits(ff[1]));
    sink.put(5, q, fp_bits(fm[0]));
    sink.put(6, q, fp_bits(fm[1]));
    sink.put(7, q, fp_bits(fs[0]));
    sink.put(8, q, fp_bits(fs[1]));
  }
}

// low `bits` bits of base set to half, half + 1, half - 1 for t = 0, 1, 2
template <typename U>
__device__ __forceinline__ U fp_low(U base, int bits, u32 t) {
  const U h = U(1) << (bits - 1);
  return (base & ~((U(1) << bits) - 1)) + (t == 0 ? h : t == 1 ? h + 1 : h - 1);
}

// stage 3: conversions and round-to-integral;
// probe/fpcheck.py:_cvt_operands is the definition
template <typename SINK>
__device__ __forceinline__ void fp_stage_cvt(u32 base, u32 rp, u32 lane, SINK& sink) {
#pragma clang fp contract(off)
  sink.slots = 64 * 8;
#pragma unroll 1
  for (u32 j = 0; j < 8; ++j) {
    const u32 q = 64 * j + lane;
    const u32 recipe = (lane + j + rp) & 7u;
    const u32 rx = fp_word(base, q, 0), ru = fp_word(base, q, 4), sel = fp_word(base, q, 6);
    const u64 rd = fp_word64(base, q, 2);
    const u32 v = sel & 3u, t = ((sel >> 2) & 255u) % 3u;
    const u32 s = FpS::S(rx), e = FpS::E(rx), m = FpS::M(rx);
    const u64 ds = FpD::S(rd), de = FpD::E(rd), dm = FpD::M(rd);
    const u32 x1 = FpS::pack(s, 99u + (e & 63u), m);
    const u64 d1 = FpD::pack(ds, (1023 - 128) + (de & 255), dm);
    u32 x, u = (recipe & 1u) ? ru >> ((sel >> 8) & 31u) : ru;
    u64 d;
    switch (recipe) {
      case 0:
        x = rx, d = rd;
        break;
      case 1:
        x = x1, d = d1;
        break;
      case 2: {
        x = (v & 1u) ? fp_low<u32>(x1, 13, t) : fp_low<u32>(x1, 16, t);
        d = fp_low<u64>(d1, 29, t);
        const u32 pbit = 24u + ((sel >> 8) & 7u), ub = pbit - 24u;
        const u32 top = (ru | 0x80000000u) >> (31u - pbit);
        u = (top & ~((2u << ub) - 1u)) +
            (t == 0 ? (1u << ub) : t == 1 ? (1u << ub) + 1u : (1u << ub) - 1u);
        break;
      }
      case 3: {
        const u32 ee = e & 31u;  // unbiased exponent ee - 2
        u32 m3 = m;
        if (ee >= 2u && ee <= 24u && t != 1u) {
          const u32 hb = 24u - ee;  // the mantissa bit worth 0.5
          m3 = (m & ~((2u << hb) - 1u) & FpS::MM) | (t == 0 ? (1u << hb) : 0u);
        }
        x = FpS::pack(s, 125u + ee, m3);
        d = d1;
        break;
      }
      case 4:
        x = FpS::pack(s, 0, m);
        d = FpD::pack(ds, (1023 - 152) + (de & 31), dm);
        break;
      case 5:
        // about the largest finite bf16 (v = 2), else about the largest f16
        x = v == 2u ? FpS::pack(s, 254u, 0x7F0000u | (m & 0xFFFFu))
                    : FpS::pack(s, 141u + (e & 3u),
                                (v & 1u) ? (0x7FE000u | (m & 0x1FFFu)) : m);
        d = FpD::pack(ds, (1023 + 127) + (de & 1),
                      (v & 1u) ? (0xFFFFFE0000000ull | (dm & 0x1FFFFFFFull)) : dm);
        break;
      case 6:
        x = FpS::pack(s, 151u + (e & 7u), m);
        d = FpD::pack(ds, de & 15, dm);
        break;
      default:
        x = FpS::special(rx, (sel >> 16) & 7u);
        d = FpD::special(rd, (sel >> 19) & 7u);
        break;
    }
    // the C cast is undefined from 2**31 on, for Inf and for NaN
    const u32 xi = FpS::E(x) >= 158u ? FpS::at(x, 150, 7) : x;
    const float xf = fp_f32(x);
    sink.put(0, q, fp_bits((_Float16)xf));
    const unsigned short bf = __builtin_bit_cast(unsigned short, (__bf16)xf);
    sink.put(1, q, (bf & 0x7FFFu) > 0x7F80u ? 0x7FC0u : (u32)bf);
    sink.put(2, q, fp_bits((float)fp_f64(d)));
    sink.put(3, q, fp_bits((float)u));
    sink.put(4, q, fp_bits((float)(int)u));
    sink.put(5, q, (u32)(int)fp_f32(xi));
    sink.put(6, q, fp_bits(__builtin_rintf(xf)));
    sink.put(7, q, fp_bits(__builtin_floorf(xf)));
    sink.put(8, q, fp_bits(__builtin_ceilf(xf)));
    sink.put(9, q, fp_bits(__builtin_truncf(xf)));
  }
}

__global__ void __launch_bounds__(CU_BLOCK)
fpcheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
#pragma clang fp contract(off)
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % FP_PERIOD;
    FpFold f0, f1, f2, f3;
    fp_stage_f32(cu_base(a.seed, FP_STAGE0 + 0, rp), rp, lane, f0);
    fp_stage_f64(cu_base(a.seed, FP_STAGE0 + 1, rp), rp, lane, f1);
    fp_stage_packed(cu_base(a.seed, FP_STAGE0 + 2, rp), rp, lane, f2);
    fp_stage_cvt(cu_base(a.seed, FP_STAGE0 + 3, rp), rp, lane, f3);
    u32 dig[N_STAGES] = {wave_sum(f0.d), wave_sum(f1.d), wave_sum(f2.d), wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One workgroup; wave 0 writes the raw result bits of one stage and
// round, out[slots * op + q], zero-extended to 64 bits.  A digest cannot
// say which operation on which operands is wrong; this can.
__global__ void __launch_bounds__(CU_BLOCK)
fpcheck_values_kernel(u32 seed, u32 stage, u32 r, u64* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
#pragma clang fp contract(off)
  if (threadIdx.x >= WAVE) return;
  const u32 lane = threadIdx.x, rp = r % FP_PERIOD;
  const u32 base = cu_base(seed, FP_STAGE0 + stage, rp);
  FpDump sink;
  sink.out = out;
  if (stage == 0)
    fp_stage_f32(base, rp, lane, sink);
  else if (stage == 1)
    fp_stage_f64(base, rp, lane, sink);
  else if (stage == 2)
    fp_stage_packed(base, rp, lane, sink);
  else
    fp_stage_cvt(base, rp, lane, sink);
#endif
}

// ---------------------------------------------------------------- host

static const int FP_SLOTS[N_STAGES] = {64 * 8, 64 * 4, 64 * 8, 64 * 8};
static const int FP_OPS[N_STAGES] = {5, 5, 9, 10};

CucheckOut fpcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                       int64_t blocks_arg, int64_t max_records,
                       c10::optional<at::Tensor> dump,
                       c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("fpcheck", expected, seed_arg, rounds, blocks_arg,
                          max_records, dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(fpcheck_kernel, l, MAX_LDS_BYTES);
}

// The raw result bits of one stage and round as an int64 tensor on the
// current GPU, [operations x slots].
at::Tensor fpcheck_values(int64_t seed_arg, int64_t stage, int64_t round) {
  cu_check_wave_args("fpcheck", seed_arg, stage, round);
  at::Tensor out = at::zeros({(int64_t)FP_OPS[stage] * FP_SLOTS[stage]},
                             at::TensorOptions().dtype(at::kLong).device(at::kCUDA));
  return cu_launch_values(fpcheck_values_kernel, CU_BLOCK, 0, out, (u32)seed_arg,
                          (u32)stage, (u32)round, (u64*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/fpcheck_mi355x.json).
void bind_fpcheck(py::module_& m) {
  m.def("fpcheck_run", &fpcheck_run,
        "IEEE rounding integrity run -> (mismatches, first_bad_round, "
        "stage_mask, records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"),
        py::arg("blocks") = 0, py::arg("max_records") = 16,
        py::arg("dump") = py::none(), py::arg("inject") = py::none());
  m.def("fpcheck_values", &fpcheck_values,
        "raw result bits of one stage and round as int64 [operations * slots]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"));
}
