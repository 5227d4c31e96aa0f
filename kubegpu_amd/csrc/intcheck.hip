// intcheck — integrity kernel for the integer vector and scalar ALUs
// (gfx950), compiled into _gpuprobe.
//
// The twin of lanecheck.hip for the datapath every kernel leans on for
// addresses, loop control, masks, quantised dots and packed 16-bit math,
// and which no other probe uses as workload.  Every wave of the launch
// runs the same deterministic sequence of integer operations and compares
// four 32-bit digests per round with a table the host computed in numpy
// (probe/intcheck.py holds the definition of every operand, op and
// digest):
//   stage 0 bits    shifts (32 and 64 bit), alignbit / alignbyte, bfe, bfi,
//                   perm, brev, popcount, clz / ctz / clrsb, the
//                   three-operand adds, shifts and logic ops
//   stage 1 arith   three-limb carry and borrow chains, 64-bit add / sub,
//                   mul_lo / mulhi, the 24-bit multiplies, mad_u64_u32 and
//                   i64, 64 x 64 multiply, u32 / i32 / u64 division,
//                   min / max / med3 / min3 / max3, compares as ballots, a
//                   select chain
//   stage 2 packed  the packed 16-bit pipe (wrapping, saturating, mad,
//                   min / max, shifts), sad_u8 / hi_u8 / u16, lerp_u8, the
//                   dot4 / dot8 / dot2 integer dots without and with clamp
//   stage 3 scalar  the same families on wave-uniform values, which the
//                   compiler keeps on the scalar ALU, a uniform switch, one
//                   bounded data-dependent loop and the 64-bit wave-mask
//                   arithmetic behind every ballot
// Every op is exact in C, so the reference is exact.  No inline assembly:
// builtins and plain C++, with every undefined case of C (shift amounts,
// division by 0, INT_MIN / -1, clz(0), signed overflow) written out of
// the expressions.  The scalar unit only computes and loads; every store
// is a vector store.
//
// Inputs are word(48 + stage, r % IC_PERIOD, idx) of cucheck_common.h.
// The vector stages run their op list on IC_GROUPS operand groups j:
// operand slot q = 64 j + lane, words 8 q .. 8 q + 3 are ra, rb, rc, sel,
// and a, b, c come from recipe (lane + j + r) mod 8 (ic_recipe), which
// puts operands on the integer edges raw words almost never hit.  Nothing
// depends on the wave number, no result is used as an address or a loop
// bound but in the one bounded loop of stage 3, and the kernel touches no
// memory but the shared result block and the optional dump; the dynamic
// LDS is asked for only to keep a second workgroup off the CU.  Launch
// shape and accounting are cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#define IC_DEV __device__ __forceinline__

#define IC_STAGE0 48u  // stage number fed to cu_base() is IC_STAGE0 + stage
#define IC_PERIOD 64u
#define IC_GROUPS 2u
#define IC_VALUE_SLOTS 128u  // rows of intcheck_values' output, >= any stage's
// result slots of one operand group of the stages, and of the mask block
#define IC_SLOTS_BITS 33u
#define IC_SLOTS_ARITH 55u
#define IC_SLOTS_PACKED 32u
#define IC_SLOTS_SCALAR 44u
#define IC_SLOTS_MASKS 24u
static_assert(IC_GROUPS * IC_SLOTS_ARITH <= IC_VALUE_SLOTS &&
                  IC_GROUPS * IC_SLOTS_SCALAR + IC_SLOTS_MASKS <= IC_VALUE_SLOTS,
              "intcheck_values' rows must hold every stage");

typedef unsigned long long u64;
typedef long long i64;
typedef short ic_s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short ic_u16x2 __attribute__((ext_vector_type(2)));

#define IC_INT_MIN 0x80000000u
#define IC_INT_MAX 0x7FFFFFFFu

#if __HIP_DEVICE_COMPILE__

// recipe 7's bytes for codes 0..5 (BYTES there), lowest first
#define IC_BYTES 0x0000FEFF807F0100ull

// Where a stage's values go: into the digest, or into the element dump
// (row `slot`, column lane).
struct IcFold {
  u32 d = 0;
  IC_DEV void put(u32 slot, u32 lane, u32 v) { d += cu_fmix32(v + cu_salt(64u * slot + lane)); }
};

struct IcDump {
  u32* out;
  IC_DEV void put(u32 slot, u32 lane, u32 v) { out[64u * slot + lane] = v; }
};

template <typename SINK>
IC_DEV void ic_put64(SINK& sink, u32& n, u32 lane, u64 v) {
  sink.put(n++, lane, (u32)v);
  sink.put(n++, lane, (u32)(v >> 32));
}

IC_DEV u32 ic_sext(u32 x, u32 bits) { return (u32)((int)(x << (32u - bits)) >> (32u - bits)); }
IC_DEV u32 ic_rotl(u32 x, u32 n) { return (x << n) | (x >> ((32u - n) & 31u)); }
IC_DEV u32 ic_run(u32 x) { return ic_rotl((1u << ((x >> 8) & 31u)) - 1u, x & 31u); }
IC_DEV u64 ic_cat(u32 hi, u32 lo) { return ((u64)hi << 32) | lo; }
IC_DEV u32 ic_clz(u32 x) { return x ? (u32)__builtin_clz(x) : 32u; }
IC_DEV u32 ic_ctz(u32 x) { return x ? (u32)__builtin_ctz(x) : 32u; }
IC_DEV u32 ic_clz64(u64 x) { return x ? (u32)__builtin_clzll(x) : 64u; }
IC_DEV u32 ic_ctz64(u64 x) { return x ? (u32)__builtin_ctzll(x) : 64u; }
IC_DEV u32 ic_min(u32 x, u32 y) { return x < y ? x : y; }
IC_DEV u32 ic_max(u32 x, u32 y) { return x > y ? x : y; }
IC_DEV int ic_min(int x, int y) { return x < y ? x : y; }
IC_DEV int ic_max(int x, int y) { return x > y ? x : y; }

IC_DEV u32 ic_bytes(u32 raw, u32 codes) {
  u32 out = 0;
#pragma unroll
  for (u32 i = 0; i < 4u; ++i) {
    const u32 code = (codes >> (3u * i)) & 7u;
    const u32 byte = code >= 6u ? (raw >> (8u * i)) & 0xFFu : (u32)(IC_BYTES >> (8u * code)) & 0xFFu;
    out |= byte << (8u * i);
  }
  return out;
}

struct IcOperands {
  u32 a, b, c, sel;
};

// a, b, c of recipe k = 0..7 from the raw words
IC_DEV IcOperands ic_recipe(u32 k, u32 ra, u32 rb, u32 rc, u32 sel) {
  // recipe 2's values; probe/intcheck.py holds the same table as EDGE
  static constexpr u32 IC_EDGE[16] = {0u,        1u,        2u,        0xFFFFFFFFu,
                                      0xFFFFFFFEu, IC_INT_MAX, IC_INT_MIN, IC_INT_MIN + 1u,
                                      0xFFFFu,   0x10000u,  0xFFu,     0x100u,
                                      0x7FFFFFu, 0x800000u, 0xFFFFFFu, 0xFF800000u};
  IcOperands o = {ra, rb, rc, sel};
  switch (k) {
    case 1u:
      o.a = ic_sext(ra, 9u), o.b = ic_sext(rb, 17u), o.c = ic_sext(rc, 5u);
      break;
    case 2u:
      o.a = IC_EDGE[sel & 15u], o.b = IC_EDGE[(sel >> 4) & 15u], o.c = IC_EDGE[(sel >> 8) & 15u];
      break;
    case 3u:
      o.a = 1u << (ra & 31u), o.b = ~(1u << (rb & 31u)), o.c = 1u << (rc & 31u);
      break;
    case 4u:
      o.a = ic_run(ra), o.b = ic_run(rb);
      break;
    case 5u:
      o.b = ~ra + ic_sext(sel, 3u), o.c = rc & 1u;
      break;
    case 6u:
      o.b = (sel >> 5) & 1u ? ra ^ (1u << (sel & 31u)) : ra, o.c = ra ^ IC_INT_MIN;
      break;
    case 7u:
      o.a = ic_bytes(ra, sel), o.b = ic_bytes(rb, sel >> 12), o.c = ic_bytes(rc, sel >> 20);
      break;
    default:
      break;
  }
  return o;
}

// operand group j of a vector stage
IC_DEV IcOperands ic_operands(u32 base, u32 rp, u32 j, u32 lane) {
  const u32 w = base + 8u * (64u * j + lane);
  return ic_recipe((lane + j + rp) & 7u, cu_fmix32(w), cu_fmix32(w + 1u), cu_fmix32(w + 2u),
                   cu_fmix32(w + 3u));
}

IC_DEV u32 ic_v(u32 base, u32 k, u32 lane) { return cu_fmix32(base + 64u * k + lane); }
IC_DEV u32 ic_u(u32 base, u32 k) {
  return (u32)__builtin_amdgcn_readfirstlane((int)cu_fmix32(base + 64u * k));
}

// ---- stage 0: bit operations

template <typename SINK>
IC_DEV void ic_ops_bits(const IcOperands& o, u32& n, u32 lane, SINK& sink) {
  const u32 a = o.a, b = o.b, c = o.c;
  const u32 s = b & 31u, s6 = b & 63u;
  const u64 X = ic_cat(c, a);
  sink.put(n++, lane, a << s);
  sink.put(n++, lane, a >> s);
  sink.put(n++, lane, (u32)((int)a >> s));
  ic_put64(sink, n, lane, X << s6);
  ic_put64(sink, n, lane, X >> s6);
  ic_put64(sink, n, lane, (u64)((i64)X >> s6));
  sink.put(n++, lane, __builtin_amdgcn_alignbit(a, c, s));
  sink.put(n++, lane, __builtin_amdgcn_alignbit(a, a, s));
  sink.put(n++, lane, __builtin_amdgcn_alignbyte(a, c, b & 3u));
  // the field never runs past bit 31
  const u32 w = (b >> 8) % (ic_min(31u, 32u - s) + 1u);
  sink.put(n++, lane, __builtin_amdgcn_ubfe(a, s, w));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sbfe((int)a, s, w));
  sink.put(n++, lane, (a & b) | (~a & c));
  u32 selector = 0;
#pragma unroll
  for (u32 i = 0; i < 4u; ++i) {
    const u32 code = ((o.sel >> (4u * i)) & 15u) % 9u;
    selector |= (code == 8u ? 0x0Cu : code) << (8u * i);
  }
  sink.put(n++, lane, __builtin_amdgcn_perm(a, c, selector));
  sink.put(n++, lane, __builtin_bitreverse32(a));
  sink.put(n++, lane, (u32)__builtin_popcount(a) + c);
  sink.put(n++, lane, ic_clz(a));
  sink.put(n++, lane, ic_ctz(a));
  sink.put(n++, lane, (u32)__builtin_clrsb((int)a));
  sink.put(n++, lane, (u32)__builtin_popcountll(X));
  sink.put(n++, lane, ic_clz64(X));
  sink.put(n++, lane, (a << 1) + b);
  sink.put(n++, lane, (a << 2) + b);
  sink.put(n++, lane, (a << 3) + b);
  sink.put(n++, lane, (a << 4) + b);
  sink.put(n++, lane, (a + b) << 3);
  sink.put(n++, lane, (a << 2) | b);
  sink.put(n++, lane, (a & b) | c);
  sink.put(n++, lane, a | b | c);
  sink.put(n++, lane, a + b + c);
  sink.put(n++, lane, (a ^ b) + c);
}

// ---- stage 1: arithmetic

template <typename SINK>
IC_DEV void ic_put_ballot(SINK& sink, u32& n, u32 lane, bool bit) {
  ic_put64(sink, n, lane, __builtin_amdgcn_ballot_w64(bit));
}

template <typename SINK>
IC_DEV void ic_ops_arith(const IcOperands& o, u32& n, u32 lane, SINK& sink) {
  const u32 a = o.a, b = o.b, c = o.c;
  const int ia = (int)a, ib = (int)b, ic = (int)c;
  const u64 X = ic_cat(c, a), Y = ic_cat(a ^ IC_INT_MIN, b);
  {
    u32 cy;
    sink.put(n++, lane, __builtin_addc(a, b, 0u, &cy));
    sink.put(n++, lane, __builtin_addc(b, c, cy, &cy));
    sink.put(n++, lane, __builtin_addc(c, a, cy, &cy));
    sink.put(n++, lane, cy);
    u32 bw;
    sink.put(n++, lane, __builtin_subc(a, b, 0u, &bw));
    sink.put(n++, lane, __builtin_subc(b, c, bw, &bw));
    sink.put(n++, lane, __builtin_subc(c, a, bw, &bw));
    sink.put(n++, lane, bw);
  }
  ic_put64(sink, n, lane, X + Y);
  ic_put64(sink, n, lane, X - Y);
  sink.put(n++, lane, a * b);
  sink.put(n++, lane, (u32)(((u64)a * b) >> 32));
  sink.put(n++, lane, (u32)(((i64)ia * ib) >> 32));
  {
    const i64 s24 = (i64)((int)(a << 8) >> 8) * ((int)(b << 8) >> 8);
    const u64 u24 = (u64)(a & 0xFFFFFFu) * (b & 0xFFFFFFu);
    sink.put(n++, lane, (u32)s24);
    sink.put(n++, lane, (u32)(s24 >> 32));
    sink.put(n++, lane, (u32)u24);
    sink.put(n++, lane, (u32)(u24 >> 32));
  }
  ic_put64(sink, n, lane, (u64)a * b + X);
  ic_put64(sink, n, lane, (u64)((i64)ia * ib) + X);
  ic_put64(sink, n, lane, X * Y);
  {
    // C leaves x / 0 and INT_MIN / -1 undefined: both are remapped
    const u32 den = b == 0u ? 1u : b;
    sink.put(n++, lane, a / den);
    sink.put(n++, lane, a % den);
    const int iden = (ib == 0 || (a == IC_INT_MIN && ib == -1)) ? 1 : ib;
    sink.put(n++, lane, (u32)(ia / iden));
    sink.put(n++, lane, (u32)(ia % iden));
    u64 den64 = Y >> (o.sel >> 26);
    den64 = den64 == 0u ? 1u : den64;
    ic_put64(sink, n, lane, X / den64);
    ic_put64(sink, n, lane, X % den64);
  }
  sink.put(n++, lane, (u32)ic_min(ia, ib));
  sink.put(n++, lane, (u32)ic_max(ia, ib));
  sink.put(n++, lane, ic_min(a, b));
  sink.put(n++, lane, ic_max(a, b));
  sink.put(n++, lane, (u32)ic_max(ic_min(ia, ib), ic_min(ic_max(ia, ib), ic)));
  sink.put(n++, lane, ic_max(ic_min(a, b), ic_min(ic_max(a, b), c)));
  sink.put(n++, lane, (u32)ic_min(ic_min(ia, ib), ic));
  sink.put(n++, lane, ic_min(ic_min(a, b), c));
  sink.put(n++, lane, (u32)ic_max(ic_max(ia, ib), ic));
  sink.put(n++, lane, ic_max(ic_max(a, b), c));
  sink.put(n++, lane, a > b ? a - b : b - a);
  ic_put_ballot(sink, n, lane, ia < ib);
  ic_put_ballot(sink, n, lane, a < b);
  ic_put_ballot(sink, n, lane, a == b);
  ic_put_ballot(sink, n, lane, X < Y);
  ic_put_ballot(sink, n, lane, (i64)X < (i64)Y);
  {
    u32 s = a & 1u ? b : c;
    s = s < a ? s + 1u : a;
    s = (int)s < ib ? s ^ c : s - b;
    s = s == c ? a : s;
    sink.put(n++, lane, s);
  }
}

// ---- stage 2: packed 16-bit math, SADs, dots

template <typename V>
IC_DEV u32 ic_bits(V v) { return __builtin_bit_cast(u32, v); }

template <typename SINK>
IC_DEV void ic_ops_packed(const IcOperands& o, u32& n, u32 lane, SINK& sink) {
  const u32 a = o.a, b = o.b, c = o.c;
  const ic_s16x2 sa = __builtin_bit_cast(ic_s16x2, a), sb = __builtin_bit_cast(ic_s16x2, b);
  const ic_u16x2 ua = __builtin_bit_cast(ic_u16x2, a), ub = __builtin_bit_cast(ic_u16x2, b);
  const ic_u16x2 uc = __builtin_bit_cast(ic_u16x2, c);
  sink.put(n++, lane, ic_bits(ua + ub));
  sink.put(n++, lane, ic_bits(ua - ub));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_add_sat(sa, sb)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_sub_sat(sa, sb)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_add_sat(ua, ub)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_sub_sat(ua, ub)));
  sink.put(n++, lane, ic_bits(ua * ub));
  // wrapping, so the same bits signed or unsigned; two operand orders
  sink.put(n++, lane, ic_bits(ua * uc + ub));
  sink.put(n++, lane, ic_bits(ua * ub + uc));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_min(sa, sb)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_max(sa, sb)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_min(ua, ub)));
  sink.put(n++, lane, ic_bits(__builtin_elementwise_max(ua, ub)));
  const ic_u16x2 sh = ub & (unsigned short)15;
  sink.put(n++, lane, ic_bits(ua << sh));
  sink.put(n++, lane, ic_bits(ua >> sh));
  sink.put(n++, lane, ic_bits(sa >> __builtin_convertvector(sh, ic_s16x2)));
  sink.put(n++, lane, __builtin_amdgcn_sad_u8(a, b, c));
  sink.put(n++, lane, __builtin_amdgcn_sad_hi_u8(a, b, c));
  sink.put(n++, lane, __builtin_amdgcn_sad_u16(a, b, c));
  sink.put(n++, lane, __builtin_amdgcn_lerp(a, b, c));
  // for the clamped runs c sits near a bound of the result type, at a
  // distance of the size of the dot (CLAMP_BITS in probe/intcheck.py)
  const u32 k = o.sel >> 30;
  const u32 anchor = k == 0u ? IC_INT_MAX : k == 1u ? IC_INT_MIN : k == 2u ? 0u : 0xFFFFFFFFu;
  const u32 c15 = anchor + ic_sext(c, 15u), c8 = anchor + ic_sext(c, 8u);
  const u32 c18 = anchor + ic_sext(c, 18u);
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot4((int)a, (int)b, (int)c, false));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot4((int)a, (int)b, (int)c15, true));
  sink.put(n++, lane, __builtin_amdgcn_udot4(a, b, c, false));
  sink.put(n++, lane, __builtin_amdgcn_udot4(a, b, c15, true));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot8((int)a, (int)b, (int)c, false));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot8((int)a, (int)b, (int)c8, true));
  sink.put(n++, lane, __builtin_amdgcn_udot8(a, b, c, false));
  sink.put(n++, lane, __builtin_amdgcn_udot8(a, b, c8, true));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot2(sa, sb, (int)c, false));
  sink.put(n++, lane, (u32)__builtin_amdgcn_sdot2(sa, sb, (int)c18, true));
  sink.put(n++, lane, __builtin_amdgcn_udot2(ua, ub, c, false));
  sink.put(n++, lane, __builtin_amdgcn_udot2(ua, ub, c18, true));
}

// ---- stage 3: the scalar ALU

// the one data-dependent loop: one trip per set bit, 32 at the most
IC_DEV u32 ic_loop_hash(u32 t) {
  u32 h = 0;
  while (t) {
    h = h * 33u + (u32)__builtin_ctz(t);
    t &= t - 1u;
  }
  return h;
}

template <typename SINK>
IC_DEV void ic_ops_scalar(const IcOperands& o, u32& n, u32 lane, SINK& sink) {
  const u32 x = o.a, y = o.b, z = o.c;
  const int ix = (int)x, iy = (int)y;
  const u32 s = y & 31u, s6 = y & 63u;
  const u64 Z = ic_cat(z, x), W = ic_cat(x ^ IC_INT_MIN, y);
  sink.put(n++, lane, (u32)__builtin_popcount(x));
  sink.put(n++, lane, ic_ctz(x));
  sink.put(n++, lane, ic_clz(x));
  sink.put(n++, lane, __builtin_bitreverse32(x));
  sink.put(n++, lane, (u32)__builtin_clrsb(ix));
  sink.put(n++, lane, (u32)__builtin_popcountll(Z));
  sink.put(n++, lane, ic_ctz64(Z));
  sink.put(n++, lane, x * y);
  sink.put(n++, lane, (u32)(((u64)x * y) >> 32));
  sink.put(n++, lane, (u32)(((i64)ix * iy) >> 32));
  sink.put(n++, lane, x << s);
  sink.put(n++, lane, x >> s);
  sink.put(n++, lane, (u32)(ix >> s));
  ic_put64(sink, n, lane, Z << s6);
  ic_put64(sink, n, lane, Z >> s6);
  ic_put64(sink, n, lane, (u64)((i64)Z >> s6));
  sink.put(n++, lane, (x >> s) & ((1u << ((y >> 8) & 15u)) - 1u));
  sink.put(n++, lane, (u32)((int)(x << (31u - s)) >> ((y >> 16) & 31u)));
  sink.put(n++, lane, (u32)ic_min(ix, iy));
  sink.put(n++, lane, (u32)ic_max(ix, iy));
  sink.put(n++, lane, ic_min(x, y));
  sink.put(n++, lane, ic_max(x, y));
  sink.put(n++, lane, x > y ? x - y : y - x);
  sink.put(n++, lane, x & ~y);
  sink.put(n++, lane, x | ~y);
  sink.put(n++, lane, ~(x & y));
  sink.put(n++, lane, ~(x | y));
  sink.put(n++, lane, ~(x ^ y));
  sink.put(n++, lane, (u32)(int)(signed char)x);
  sink.put(n++, lane, (u32)(int)(short)x);
  ic_put64(sink, n, lane, Z + W);
  ic_put64(sink, n, lane, Z - W);
  sink.put(n++, lane, (x << 1) + y);
  sink.put(n++, lane, (x << 2) + y);
  sink.put(n++, lane, (x << 3) + y);
  sink.put(n++, lane, (x << 4) + y);
  u32 arm;
  switch (o.sel & 3u) {
    case 0u: arm = x + y; break;
    case 1u: arm = x ^ (y >> 3); break;
    case 2u: arm = (x & y) * 3u; break;
    default: arm = x - z; break;
  }
  sink.put(n++, lane, arm);
  sink.put(n++, lane, ic_loop_hash(x));
  sink.put(n++, lane, ic_loop_hash(x & (x - 1u)));
}

template <typename SINK>
IC_DEV void ic_ops_masks(u32 base, u32& n, u32 lane, SINK& sink) {
  const u64 m1 = __builtin_amdgcn_ballot_w64(ic_v(base, 0u, lane) < ic_v(base, 1u, lane));
  const u64 m2 = __builtin_amdgcn_ballot_w64((ic_v(base, 2u, lane) & 1u) != 0u);
  const u64 masks[4] = {m1, m2, m1 & ~m2, m1 ^ m2};
#pragma unroll
  for (u32 i = 0; i < 4u; ++i) ic_put64(sink, n, lane, masks[i]);
#pragma unroll
  for (u32 i = 0; i < 4u; ++i) {
    sink.put(n++, lane, (u32)__builtin_popcountll(masks[i]));
    sink.put(n++, lane, ic_ctz64(masks[i]));
    sink.put(n++, lane, ic_clz64(masks[i]));
  }
  const u32 s6 = ic_u(base, 3u) & 63u;
  ic_put64(sink, n, lane, m1 << s6);
  ic_put64(sink, n, lane, (u64)((i64)m1 >> s6));
}

// One stage for one round; returns the number of slots it filled.
template <u32 STAGE, typename SINK>
IC_DEV u32 ic_stage(u32 seed, u32 rp, u32 lane, SINK& sink) {
  const u32 base = cu_base(seed, IC_STAGE0 + STAGE, rp);
  u32 n = 0;
#pragma unroll 1
  for (u32 j = 0; j < IC_GROUPS; ++j) {
    if constexpr (STAGE == 0u) ic_ops_bits(ic_operands(base, rp, j, lane), n, lane, sink);
    else if constexpr (STAGE == 1u) ic_ops_arith(ic_operands(base, rp, j, lane), n, lane, sink);
    else if constexpr (STAGE == 2u) ic_ops_packed(ic_operands(base, rp, j, lane), n, lane, sink);
    else
      ic_ops_scalar(ic_recipe((j + rp) & 7u, ic_u(base, 4u + 4u * j), ic_u(base, 5u + 4u * j),
                              ic_u(base, 6u + 4u * j), ic_u(base, 7u + 4u * j)),
                    n, lane, sink);
  }
  if constexpr (STAGE == 3u) ic_ops_masks(base, n, lane, sink);
  return n;
}

#endif  // __HIP_DEVICE_COMPILE__

__global__ void __launch_bounds__(CU_BLOCK)
intcheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % IC_PERIOD;
    IcFold f0, f1, f2, f3;
    ic_stage<0u>(a.seed, rp, lane, f0);
    ic_stage<1u>(a.seed, rp, lane, f1);
    ic_stage<2u>(a.seed, rp, lane, f2);
    ic_stage<3u>(a.seed, rp, lane, f3);
    u32 dig[N_STAGES] = {wave_sum(f0.d), wave_sum(f1.d), wave_sum(f2.d), wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One wave writes every value it would fold for one stage and round,
// out[64 * slot + lane], and the number of slots behind the last row.  A
// digest cannot say which op went wrong; this can.
__global__ void __launch_bounds__(WAVE)
intcheck_values_kernel(u32 seed, u32 stage, u32 r, u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  const u32 lane = threadIdx.x;
  const u32 rp = r % IC_PERIOD;
  IcDump sink;
  sink.out = out;
  u32 n;
  if (stage == 0u) n = ic_stage<0u>(seed, rp, lane, sink);
  else if (stage == 1u) n = ic_stage<1u>(seed, rp, lane, sink);
  else if (stage == 2u) n = ic_stage<2u>(seed, rp, lane, sink);
  else n = ic_stage<3u>(seed, rp, lane, sink);
  if (lane == 0u) out[64u * IC_VALUE_SLOTS] = n;
#endif
}

// ---------------------------------------------------------------- host

CucheckOut intcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                        int64_t blocks_arg, int64_t max_records,
                        c10::optional<at::Tensor> dump, c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("intcheck", expected, seed_arg, rounds, blocks_arg, max_records,
                          dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(intcheck_kernel, l, MAX_LDS_BYTES);
}

// What one wave folds for one stage and round as an int32 tensor on the
// current GPU: IC_VALUE_SLOTS rows of 64 lanes, then the number of rows
// the stage filled.
at::Tensor intcheck_values(int64_t seed_arg, int64_t stage, int64_t round) {
  cu_check_wave_args("intcheck", seed_arg, stage, round);
  at::Tensor out = at::zeros({(int64_t)(64 * IC_VALUE_SLOTS + 1)},
                             at::TensorOptions().dtype(at::kInt).device(at::kCUDA));
  return cu_launch_values(intcheck_values_kernel, WAVE, 0, out, (u32)seed_arg, (u32)stage,
                          (u32)round, (u32*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/intcheck_mi355x.json).
void bind_intcheck(py::module_& m) {
  m.def("intcheck_run", &intcheck_run,
        "integer-ALU integrity run -> (mismatches, first_bad_round, stage_mask, "
        "records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("max_records") = 16, py::arg("dump") = py::none(),
        py::arg("inject") = py::none());
  m.def("intcheck_values", &intcheck_values,
        "values one wave folds for one stage and round as int32 [128 rows * 64 lanes + 1]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"));
}
