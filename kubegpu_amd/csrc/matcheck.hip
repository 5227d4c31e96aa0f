// matcheck — matrix-core integrity kernel for the 16x16 shapes, the MXFP8,
// MXFP6 and mixed-width formats of the scaled instruction with wide
// scales, and the 2:4 structured-sparse instructions (gfx950), compiled
// into _gpuprobe.
//
// The twin of mxcheck.hip for what that kernel leaves out.  Every wave of
// the launch runs the same deterministic workload and compares four
// 32-bit digests per round with values the host computed independently in
// numpy (probe/matcheck.py:reference_digests is the definition, and
// defines the operands, scales and indices of every form):
//   stage 0 shape16  16x16 tiles, K = 128, accumulator-in from a word:
//                    v_mfma_i32_16x16x64_i8, v_mfma_f32_16x16x32_bf16,
//                    v_mfma_f32_16x16x32_f16
//   stage 1 mxfp8    v_mfma_scale_f32_{16x16x128,32x32x64}_f8f6f4, K = 128,
//                    e4m3 x e5m2 and e5m2 x e4m3 on a sliding window of
//                    exponent fields, E8M0 scales 23..230 in byte r&3 of
//                    the scale register (op_sel), NaN / Inf / scale-NaN
//                    classes in rounds with r % 8 == 7
//   stage 2 mxfp6    the same instruction with e2m3 x e3m2, e3m2 x e2m3
//                    and e3m2 x e2m1 operands
//   stage 3 sparse   v_smfmac_f32_16x16x64_{f16,bf16},
//                    v_smfmac_i32_16x16x128_i8,
//                    v_smfmac_f32_16x16x128_fp8_bf8, K = 128 dense
// Inputs are word(60 + stage, r, 4096 form + idx) of cucheck_common.h.
// Every operand is chosen so that all partial sums are exactly
// representable in the accumulator: a tile element is 2**e times an
// integer below 2**24 whatever order the hardware sums in, and the digest
// folds the bit pattern of the f32 (any zero as +0, any NaN as
// 0x7FC00000).  A stage's digest is the wrapping sum over its forms.
//
// Launch shape and accounting are cucheck's: 1024-thread workgroups (16
// waves), grid 0 = one workgroup per CU.  Nothing here touches the LDS;
// the 160 KiB of dynamic LDS are asked for only so that one workgroup
// fills a CU.  No inline assembly and no memory traffic beyond the result
// block.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

#define MT_STAGE0 60u      // stage number fed to cu_base() is MT_STAGE0 + stage
#define MT_FORM_WORDS 4096u  // form f of a stage draws its words from 4096 f on
// FMT field of the scaled MFMA (cbsz for A, blgp for B)
#define MT_E4M3 0
#define MT_E5M2 1
#define MT_E2M3 2
#define MT_E3M2 3
#define MT_E2M1 4
#define MT_NO_PACKED __attribute__((target("no-packed-fp32-ops")))

// What the digest folds of an f32: its bits, any zero as +0, any NaN as
// the one quiet NaN.
__device__ __forceinline__ u32 mt_canon(float c) {
  u32 b = __float_as_uint(c), mag = b & 0x7FFFFFFFu;
  if (mag == 0u) b = 0u;
  if (mag > 0x7F800000u) b = 0x7FC00000u;
  return b;
}

// C/D map of the f32 / i32 16x16 MFMAs and SMFMACs: lane l, register g
// holds row 4(l>>4) + g, column l&15.  Row-major index of that element.
__device__ __forceinline__ u32 mt_index16(int g, int lane) {
  return 16u * (4u * ((u32)lane >> 4) + (u32)g) + ((u32)lane & 15u);
}

// Where a form's accumulator tile goes: matcheck_kernel adds its fold to
// the lane's share of the stage digest, matcheck_tile_kernel stores the
// folded bit patterns row-major; both run the same stage code and go
// through the same two C/D maps.
struct MtFold {
  u32 part = 0;  // this lane's share; digest() sums the wave once per stage
  __device__ __forceinline__ void put(u32 n, u32 bits) { part += cu_fmix32(bits + cu_salt(n)); }
  __device__ __forceinline__ u32 digest() const { return wave_sum(part); }
};

struct MtDump {
  u32* out;
  __device__ __forceinline__ void put(u32 n, u32 bits) { out[n] = bits; }
};

template <typename SINK>
__device__ __forceinline__ void mt_tile16(SINK& sink, const f32x4& acc, int lane) {
#pragma unroll
  for (int g = 0; g < 4; ++g) sink.put(mt_index16(g, lane), mt_canon(acc[g]));
}

template <typename SINK>
__device__ __forceinline__ void mt_tile16(SINK& sink, const i32x4& acc, int lane) {
#pragma unroll
  for (int g = 0; g < 4; ++g) sink.put(mt_index16(g, lane), (u32)acc[g]);
}

template <typename SINK>
__device__ __forceinline__ void mt_tile32(SINK& sink, const f32x16& acc, int lane) {
#pragma unroll
  for (int g = 0; g < 16; ++g) sink.put(cu_tile_index(g, lane), mt_canon(acc[g]));
}

__device__ __forceinline__ int mt_sext(u32 x, int bits) {
  return (int)(x << (32 - bits)) >> (32 - bits);
}

// bf16 of a signed byte: at most eight significant bits, so the top half
// of its f32 encoding is exact.
__device__ __forceinline__ __bf16 mt_byte_bf16(u32 w, int b) {
  float f = (float)(int)(signed char)(w >> (8 * b));
  return __builtin_bit_cast(__bf16, (unsigned short)(__float_as_uint(f) >> 16));
}

// Four raw bytes -> four fp8 codes: sign and mantissa kept, the exponent
// field forced to f0 + two of the byte's bits.  f0 <= 12, so field 15 can
// occur: there the NaN code S.1111.111 gets mantissa 6.
__device__ __forceinline__ u32 mt_e4m3_codes(u32 w, u32 f0) {
  u32 c = (w & 0x87878787u) | ((f0 * 0x01010101u + ((w >> 3) & 0x03030303u)) << 3);
  u32 nan = (((c & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u) >> 7;
  return c & ~nan;
}

// f0 <= 27, so field 31 (Inf, NaN) never occurs.
__device__ __forceinline__ u32 mt_e5m2_codes(u32 w, u32 f0) {
  return (w & 0x83838383u) | ((f0 * 0x01010101u + ((w >> 2) & 0x03030303u)) << 2);
}

// ---------------------------------------------------------------- stage 0

// Accumulator-in: C0[i][j] is the sign-extended low half of a word.
__device__ __forceinline__ int mt_c0(u32 b0, int g, int lane) {
  return mt_sext(cu_fmix32(b0 + 2048u + mt_index16(g, lane)), 16);
}

// Dense 16x16 shapes.  Lane l owns row rc = l&15 of A and column rc of B;
// quarter q = l>>4 holds the q-th quarter of an issue's k range (C = A.B
// does not change under a permutation of k applied to both).  `only` < 0
// runs every form, else just that one.
template <typename SINK>
__device__ __forceinline__ void mt_stage_shape16(u32 base, int lane, SINK& sink, int only) {
  const u32 rc = lane & 15, q = lane >> 4;
  if (only < 0 || only == 0) {  // i8: 32 words of four bytes per row, two issues
    const u32 b0 = base;
    i32x4 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = mt_c0(b0, g, lane);
#pragma unroll
    for (u32 s = 0; s < 2; ++s) {
      u32 w0 = 32 * rc + 16 * s + 4 * q;
      i32x4 a, b;
#pragma unroll
      for (u32 w = 0; w < 4; ++w) {
        a[w] = (int)cu_fmix32(b0 + w0 + w);
        b[w] = (int)cu_fmix32(b0 + 1024u + w0 + w);
      }
      acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
    }
    mt_tile16(sink, acc, lane);
  }
  if (only < 0 || only == 1) {  // bf16: the same bytes as bf16, four issues
    const u32 b0 = base + MT_FORM_WORDS;
    f32x4 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (float)mt_c0(b0, g, lane);
#pragma unroll
    for (u32 s = 0; s < 4; ++s) {
      u32 w0 = 32 * rc + 8 * s + 2 * q;
      u32 aw0 = cu_fmix32(b0 + w0), aw1 = cu_fmix32(b0 + w0 + 1u);
      u32 bw0 = cu_fmix32(b0 + 1024u + w0), bw1 = cu_fmix32(b0 + 1024u + w0 + 1u);
      bf16x8 a, b;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        a[j] = mt_byte_bf16(aw0, j);
        a[4 + j] = mt_byte_bf16(aw1, j);
        b[j] = mt_byte_bf16(bw0, j);
        b[4 + j] = mt_byte_bf16(bw1, j);
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
    }
    mt_tile16(sink, acc, lane);
  }
  if (only < 0 || only == 2) {  // f16: 64 words of two halves per row, four issues
    const u32 b0 = base + 2 * MT_FORM_WORDS;
    f32x4 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = (float)mt_c0(b0, g, lane);
#pragma unroll
    for (u32 s = 0; s < 4; ++s) {
      u32 w0 = 64 * rc + 16 * s + 4 * q;
      f16x8 a, b;
#pragma unroll
      for (u32 w = 0; w < 4; ++w) {
        u32 aw = cu_fmix32(b0 + w0 + w), bw = cu_fmix32(b0 + 1024u + w0 + w);
        a[2 * w] = (_Float16)(short)mt_sext(aw, 11);
        a[2 * w + 1] = (_Float16)(short)mt_sext(aw >> 16, 11);
        b[2 * w] = (_Float16)(short)mt_sext(bw, 5);
        b[2 * w + 1] = (_Float16)(short)mt_sext(bw >> 16, 5);
      }
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc, 0, 0, 0);
    }
    mt_tile16(sink, acc, lane);
  }
}

// ----------------------------------------------------------- stages 1 and 2

// What a round fixes for the scaled forms.  op_sel and the shape are
// immediates of the instruction, so they are template arguments below.
struct MtRound {
  u32 f4, f5;    // first exponent field of the e4m3 / e5m2 window
  u32 special;   // 0, or 1 in a stage-1 round with r % 8 == 7
  u32 sp;        // the word the special classes are placed by
};

// One 32-element block of row / column rc: eight words at `at`, of which
// the format reads eight (fp8), six (fp6: 32 six-bit codes, little-endian)
// or four (fp4); the rest stay zero.
template <int FMT>
__device__ __forceinline__ i32x8 mt_block(u32 at, const MtRound& rd) {
  constexpr u32 NW = FMT <= MT_E5M2 ? 8 : (FMT == MT_E2M1 ? 4 : 6);
  i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (u32 w = 0; w < NW; ++w) {
    u32 x = cu_fmix32(at + w);
    if (FMT == MT_E4M3) x = mt_e4m3_codes(x, rd.f4);
    if (FMT == MT_E5M2) x = mt_e5m2_codes(x, rd.f5);
    v[w] = (int)x;
  }
  return v;
}

// Byte k (0..31) of an fp8 block := code.
__device__ __forceinline__ void mt_put_byte(i32x8& v, u32 k, u32 code) {
  const u32 sh = 8 * (k & 3);
#pragma unroll
  for (u32 w = 0; w < 8; ++w)
    if (w == (k >> 2)) v[w] = (int)(((u32)v[w] & ~(0xFFu << sh)) | (code << sh));
}

// The lane's scale register: the real E8M0 byte in byte SEL, three
// different decoys in the others.
template <int SEL>
__device__ __forceinline__ int mt_scale_reg(u32 s) {
  u32 v = s | (((s + 37u) & 255u) << 8) | (((s + 74u) & 255u) << 16) | (((s + 111u) & 255u) << 24);
  constexpr int sh = 8 * SEL;
  return (int)((v << sh) | (v >> ((32 - sh) & 31)));  // SEL 0: v | v
}

// One scaled form, K = 128: BIG = two issues of 32x32x64 (lane l: row /
// column l&31, block 2s + (l>>5) of issue s), else one issue of 16x16x128
// (row / column l&15, block l>>4).  The lane's own scale byte scales
// exactly that block.  SA = 127 + ra + t, SB = 127 + cb - t, so every
// block of a dot product carries the product scale 2**(ra + cb).
template <int FA, int FB, int SEL, bool BIG, bool SPECIAL, typename SINK>
__device__ __forceinline__ void mt_scaled(u32 b0, const MtRound& rd, u32 trange, int lane,
                                          SINK& sink) {
  constexpr u32 N = BIG ? 32 : 16;
  const u32 rc = lane & (N - 1), part = BIG ? lane >> 5 : lane >> 4;
  const int ra = mt_sext(cu_fmix32(b0 + 2048u + rc), 4);
  const int cb = mt_sext(cu_fmix32(b0 + 2080u + rc), 4);
  // special classes: a NaN element in row nl of A, +-Inf in line il of the
  // e5m2 operand, an E8M0 NaN in block sblk of row sl of A
  const u32 nl = rd.sp & (N - 1), il = (nl + 5) & (N - 1), sl = (nl + 10) & (N - 1);
  const u32 nk = (rd.sp >> 8) & 127u, ik = (rd.sp >> 16) & 127u, sblk = (rd.sp >> 24) & 3u;
  const u32 inf = 0x7Cu | ((rd.sp >> 31) << 7);
  f32x16 acc32 = {0.f};
  f32x4 acc16 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (u32 s = 0; s < (BIG ? 2u : 1u); ++s) {
    const u32 blk = BIG ? 2 * s + part : part;
    const u32 at = 32 * rc + 8 * blk;
    i32x8 a = mt_block<FA>(b0 + at, rd), b = mt_block<FB>(b0 + 1024u + at, rd);
    const int t = (int)(cu_fmix32(b0 + 2112u + blk) % (2 * trange + 1)) - (int)trange;
    u32 sa = (u32)(127 + ra + t), sb = (u32)(127 + cb - t);
    if (SPECIAL && rd.special) {
      if (rc == nl && blk == (nk >> 5)) mt_put_byte(a, nk & 31, 0x7Fu);  // NaN in both formats
      if (rc == il && blk == (ik >> 5)) {
        if (FA == MT_E5M2) mt_put_byte(a, ik & 31, inf);
        else mt_put_byte(b, ik & 31, inf);
      }
      if (rc == sl && blk == sblk) sa = 0xFFu;
    }
    if (BIG)
      acc32 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          a, b, acc32, FA, FB, SEL, mt_scale_reg<SEL>(sa), SEL, mt_scale_reg<SEL>(sb));
    else
      acc16 = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
          a, b, acc16, FA, FB, SEL, mt_scale_reg<SEL>(sa), SEL, mt_scale_reg<SEL>(sb));
  }
  if (BIG) mt_tile32(sink, acc32, lane);
  else mt_tile16(sink, acc16, lane);
}

__device__ __forceinline__ MtRound mt_round(u32 base, u32 r, bool stage1) {
  return {r % 13u, r % 28u, (stage1 && (r & 7u) == 7u) ? 1u : 0u, cu_fmix32(base + 2120u)};
}

// stage 1: fp8 elements, t in -96..96; A e4m3 and B e5m2 where bit 1 of r
// is clear, the other way round where it is set.
template <int SEL, bool BIG, typename SINK>
__device__ __forceinline__ void mt_stage_mxfp8(u32 base, u32 r, int lane, SINK& sink) {
  const MtRound rd = mt_round(base, r, true);
  if ((r >> 1) & 1u) mt_scaled<MT_E5M2, MT_E4M3, SEL, BIG, true>(base, rd, 96u, lane, sink);
  else mt_scaled<MT_E4M3, MT_E5M2, SEL, BIG, true>(base, rd, 96u, lane, sink);
}

// stage 2: six-bit and mixed-width elements, t in -64..64.  e2m1 x e4m3
// is left out: see probe/matcheck.py, "Not covered".
template <int SEL, bool BIG, typename SINK>
__device__ __forceinline__ void mt_stage_mxfp6(u32 base, u32 r, int lane, SINK& sink, int only) {
  const MtRound rd = mt_round(base, r, false);
  if (only < 0 || only == 0)
    mt_scaled<MT_E2M3, MT_E3M2, SEL, BIG, false>(base, rd, 64u, lane, sink);
  if (only < 0 || only == 1)
    mt_scaled<MT_E3M2, MT_E2M3, SEL, BIG, false>(base + MT_FORM_WORDS, rd, 64u, lane, sink);
  if (only < 0 || only == 2)
    mt_scaled<MT_E3M2, MT_E2M1, SEL, BIG, false>(base + 2 * MT_FORM_WORDS, rd, 64u, lane, sink);
}

// Both scaled stages of round r.  The shape follows the parity of r and
// op_sel is r & 3, so four instantiations serve every round.  `stage` < 0
// runs both (the production kernel), else stage 1 or 2 alone.
template <typename S1, typename S2>
__device__ __forceinline__ void mt_scaled_stages(u32 base1, u32 base2, u32 r, int lane, S1& s1,
                                                 S2& s2, int stage, int only) {
#define MT_CASE(SEL, BIG)                                                             \
  case SEL:                                                                           \
    if (stage != 2) mt_stage_mxfp8<SEL, BIG>(base1, r, lane, s1);                     \
    if (stage != 1) mt_stage_mxfp6<SEL, BIG>(base2, r, lane, s2, only);               \
    break;
  switch (r & 3u) {
    MT_CASE(0, false)
    MT_CASE(1, true)
    MT_CASE(2, false)
    MT_CASE(3, true)
  }
#undef MT_CASE
}

// ---------------------------------------------------------------- stage 3

// The 4-bit index of a group of four k: positions i0 < i1 of its two kept
// elements, i0 | i1 << 2, one of six by word % 6.
__device__ __forceinline__ u32 mt_pair(u32 word) {
  return (0xED9C84u >> (4 * (word % 6u))) & 15u;
}

// 2:4 sparse A (16 x 128 dense, stored 16 x 64) by dense B.  Lane l owns
// row rc = l&15 of A and column rc of B.  Of an issue's k range, quarter
// q = l>>4 of A holds the q-th quarter, groups of four k in register order;
// the eight registers of B are two halves of four, the first holding the
// q-th quarter of the first half of the k range, the second that of the
// second half (found on the GPU: with B contiguous like A every element is
// wrong).  One word per group holds the two kept elements (bits 0
// and 16 on), another draws the index.  The 16-bit forms read 16 index
// bits from half ABID of the index register; the other half holds decoys.
template <int ABID, typename SINK>
__device__ __forceinline__ void mt_stage_sparse(u32 base, int lane, SINK& sink, int only) {
  const u32 rc = lane & 15, q = lane >> 4;
  if (only < 0 || only <= 1) {  // f16 and bf16: two issues of K = 64
#pragma unroll
    for (int form = 0; form < 2; ++form) {
      if (only >= 0 && only != form) continue;
      const u32 b0 = base + form * MT_FORM_WORDS;
      f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (u32 s = 0; s < 2; ++s) {
        u32 aw[4], bw[8], idx = 0;
#pragma unroll
        for (u32 g = 0; g < 4; ++g) {
          u32 grp = 32 * rc + 16 * s + 4 * q + g;
          aw[g] = cu_fmix32(b0 + grp);
          idx |= mt_pair(cu_fmix32(b0 + 512u + grp)) << (4 * g);
        }
#pragma unroll
        for (u32 w = 0; w < 8; ++w)
          bw[w] = cu_fmix32(b0 + 1024u + 64 * rc + 32 * s + 16 * (w >> 2) + 4 * q + (w & 3));
        const u32 decoy = ~idx & 0xFFFFu;
        const int ireg = (int)(ABID ? (idx << 16) | decoy : idx | (decoy << 16));
        if (form == 0) {
          f16x8 a;
          f16x16 b;
#pragma unroll
          for (u32 g = 0; g < 4; ++g) {
            a[2 * g] = (_Float16)(short)mt_sext(aw[g], 11);
            a[2 * g + 1] = (_Float16)(short)mt_sext(aw[g] >> 16, 11);
          }
#pragma unroll
          for (u32 w = 0; w < 8; ++w) {
            b[2 * w] = (_Float16)(short)mt_sext(bw[w], 5);
            b[2 * w + 1] = (_Float16)(short)mt_sext(bw[w] >> 16, 5);
          }
          acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(a, b, acc, ireg, 0, ABID);
        } else {
          bf16x8 a;
          bf16x16 b;
#pragma unroll
          for (u32 g = 0; g < 4; ++g) {
            a[2 * g] = mt_byte_bf16(aw[g], 0);
            a[2 * g + 1] = mt_byte_bf16(aw[g], 2);
          }
#pragma unroll
          for (u32 w = 0; w < 8; ++w) {
            b[2 * w] = mt_byte_bf16(bw[w], 0);
            b[2 * w + 1] = mt_byte_bf16(bw[w], 2);
          }
          acc = __builtin_amdgcn_smfmac_f32_16x16x64_bf16(a, b, acc, ireg, 0, ABID);
        }
      }
      mt_tile16(sink, acc, lane);
    }
  }
  if (only < 0 || only >= 2) {  // i8 and fp8 x bf8: one issue of K = 128
#pragma unroll
    for (int form = 2; form < 4; ++form) {
      if (only >= 0 && only != form) continue;
      const u32 b0 = base + form * MT_FORM_WORDS;
      i32x4 a = {0, 0, 0, 0};
      i32x8 b;
      u32 idx = 0;
#pragma unroll
      for (u32 g = 0; g < 8; ++g) {
        u32 grp = 32 * rc + 8 * q + g;
        u32 w = cu_fmix32(b0 + grp);
        u32 two = (w & 0xFFu) | ((w >> 8) & 0xFF00u);
        a[g >> 1] = (int)((u32)a[g >> 1] | (two << (16 * (g & 1))));
        idx |= mt_pair(cu_fmix32(b0 + 512u + grp)) << (4 * g);
      }
#pragma unroll
      for (u32 w = 0; w < 8; ++w)
        b[w] = (int)cu_fmix32(b0 + 1024u + 32 * rc + 16 * (w >> 2) + 4 * q + (w & 3));
      if (form == 2) {
        i32x4 acc = {0, 0, 0, 0};
        acc = __builtin_amdgcn_smfmac_i32_16x16x128_i8(a, b, acc, (int)idx, 0, 0);
        mt_tile16(sink, acc, lane);
      } else {  // mxcheck's four-exponent fp8 operands
#pragma unroll
        for (u32 w = 0; w < 4; ++w) a[w] = (int)mt_e4m3_codes((u32)a[w], 7u);
#pragma unroll
        for (u32 w = 0; w < 8; ++w) b[w] = (int)mt_e5m2_codes((u32)b[w], 15u);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_smfmac_f32_16x16x128_fp8_bf8(a, b, acc, (int)idx, 0, 0);
        mt_tile16(sink, acc, lane);
      }
    }
  }
}

// ---------------------------------------------------------------- kernels

__global__ void __launch_bounds__(CU_BLOCK) MT_NO_PACKED
matcheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const int lane = w.lane;

  for (u32 r = 0; r < a.rounds; ++r) {
    MtFold f0, f1, f2, f3;
    mt_stage_shape16(cu_base(a.seed, MT_STAGE0 + 0, r), lane, f0, -1);
    mt_scaled_stages(cu_base(a.seed, MT_STAGE0 + 1, r), cu_base(a.seed, MT_STAGE0 + 2, r), r,
                     lane, f1, f2, -1, -1);
    if (r & 1u) mt_stage_sparse<1>(cu_base(a.seed, MT_STAGE0 + 3, r), lane, f3, -1);
    else mt_stage_sparse<0>(cu_base(a.seed, MT_STAGE0 + 3, r), lane, f3, -1);
    u32 dig[N_STAGES] = {f0.digest(), f1.digest(), f2.digest(), f3.digest()};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One workgroup; wave 0 runs one form of one stage and round and stores
// the folded bit patterns of its accumulator tile (MtDump), row-major:
// 32x32 for a scaled form in an odd round, else 16x16.  A digest cannot
// say which element is wrong; this can.
__global__ void __launch_bounds__(CU_BLOCK) MT_NO_PACKED
matcheck_tile_kernel(u32 seed, u32 stage, u32 form, u32 r, u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  if (threadIdx.x >= WAVE) return;
  const int lane = threadIdx.x;
  const u32 base = cu_base(seed, MT_STAGE0 + stage, r);
  MtDump sink{out};
  if (stage == 0)
    mt_stage_shape16(base, lane, sink, (int)form);
  else if (stage == 1 || stage == 2)
    mt_scaled_stages(base, base, r, lane, sink, sink, (int)stage, (int)form);
  else if (r & 1u)
    mt_stage_sparse<1>(base, lane, sink, (int)form);
  else
    mt_stage_sparse<0>(base, lane, sink, (int)form);
#endif
}

// ---------------------------------------------------------------- host

CucheckOut matcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                        int64_t blocks_arg, int64_t max_records,
                        c10::optional<at::Tensor> dump,
                        c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("matcheck", expected, seed_arg, rounds, blocks_arg,
                          max_records, dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(matcheck_kernel, l, MAX_LDS_BYTES);
}

// forms per stage, as probe/matcheck.py:FORMS
static const int64_t MT_FORMS[N_STAGES] = {3, 1, 3, 4};

// The folded bit patterns of one form's accumulator tile as an int32
// tensor on the current GPU: [32, 32] for a scaled form (stages 1, 2) in
// an odd round, else [16, 16].
at::Tensor matcheck_tile(int64_t seed_arg, int64_t stage, int64_t form, int64_t round) {
  cu_check_wave_args("matcheck", seed_arg, stage, round);
  TORCH_CHECK(form >= 0 && form < MT_FORMS[stage], "matcheck: form must be in 0..",
              MT_FORMS[stage] - 1, " for stage ", stage, ", got ", form);
  int64_t n = ((stage == 1 || stage == 2) && (round & 1)) ? 32 : 16;
  at::Tensor out = at::zeros({n, n}, at::TensorOptions().dtype(at::kInt).device(at::kCUDA));
  return cu_launch_values(matcheck_tile_kernel, CU_BLOCK, 0, out, (u32)seed_arg, (u32)stage,
                          (u32)form, (u32)round, (u32*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/matcheck_mi355x.json).
void bind_matcheck(py::module_& m) {
  m.def("matcheck_run", &matcheck_run,
        "16x16 / MXFP8 / MXFP6 / sparse matrix-core integrity run -> (mismatches, "
        "first_bad_round, stage_mask, records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"),
        py::arg("blocks") = 0, py::arg("max_records") = 16,
        py::arg("dump") = py::none(), py::arg("inject") = py::none());
  m.def("matcheck_tile", &matcheck_tile,
        "folded bit patterns of one form's accumulator tile as int32 [n, n]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("form"), py::arg("round"));
}
