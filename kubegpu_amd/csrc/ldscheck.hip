// ldscheck — integrity kernel for the LDS array and its access paths
// (gfx950), compiled into _gpuprobe.
//
// The twin of cucheck.hip, mxcheck.hip, fpcheck.hip, atomcheck.hip and
// lanecheck.hip for the 160 KiB LDS of a compute unit, which they leave
// almost untouched (cucheck's lds stage stores and loads dwords at
// lane-linear addresses inside a wave's own slice).  Every wave of the
// launch runs the same deterministic workload and compares four 32-bit
// digests per round with a table the host computed in numpy
// (probe/ldscheck.py holds the definition of every operand, address table
// and digest):
//   stage 0 width  ds_write_b8 / b16, ds_read_u8 / i8 / u16 / i16, the 64-,
//                  96- and 128-bit accesses, ds_write2 / ds_read2 and
//                  their st64 forms, ds_read_b64_tr_b16
//   stage 1 bank   strided reads of every conflict degree, broadcasts, a
//                  free gather, scatter writes through bijections
//   stage 2 dma    global_load_lds_dwordx4 / _dword: chunks placed through
//                  several M0 bases and instruction offsets, and gathers
//                  with per-lane source addresses
//   stage 3 xwave  every wave reads the slices other waves wrote, across
//                  the whole array, between workgroup barriers
// Every op is a move, so the reference is exact.
//
// Wave w of the block owns the slice of LD_SLICE dwords at absolute dword
// address LD_SLICE * w; the workgroup uses all 163,840 bytes.  Whatever is
// stored to absolute dword address a is value ^ ld_tag(a), and whatever is
// loaded from the address the lane meant is XORed with that address's tag
// before it is folded: the tags cancel on healthy hardware, so the table
// is the same for every wave, and a cell that answers for the wrong
// address leaves a tag difference in the digest.  Inputs are word(32 +
// stage, r % LD_PERIOD, idx) of cucheck_common.h.  No inline assembly:
// builtins and typed address_space(3) accesses only.  Launch shape and
// accounting are cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#define LD_DEV __device__ __forceinline__
#define LD_LDS(T) __attribute__((address_space(3))) T*
#define LD_GLB(T) __attribute__((address_space(1))) T*

#define LD_STAGE0 32u  // stage number fed to cu_base() is LD_STAGE0 + stage
#define LD_PERIOD 64u
#define LD_VALUE_SLOTS 256u  // rows of ldscheck_values' output, >= any stage's
#define LD_SLICE 2560u       // dwords of a wave's slice
#define LD_IMG0 4096u        // word index of img(0)
#define LD_BANK 2048u        // dwords of stage bank's region
#define LD_ST64_K 3u         // the st64 pair is 64 * LD_ST64_K dwords apart
#define LD_CHUNK 256u        // dwords of one global_load_lds_dwordx4
#define LD_UNIT 64u          // dwords of one global_load_lds_dword
#define LD_X_DWORDS 4096u
#define LD_G_DWORDS (CU_WAVES * LD_SLICE)
#define LD_TABLE_DWORDS (LD_G_DWORDS + LD_X_DWORDS)
static_assert(MAX_ROUNDS <= (1 << 17) && CU_WAVES * LD_SLICE * 4u == MAX_LDS_BYTES, "the slices fill the LDS");

// probe/ldscheck.py holds the same tables
constexpr u32 LD_B32_STRIDES[] = {1, 2, 3, 4, 8, 16, 32, 33, 64, 65};
constexpr u32 LD_WIDE_STRIDES[] = {1, 2, 4, 8, 16, 17};  // in units of the access
struct LdPair {
  u32 a, b;
};
// (stride, offset) of the scatters' 64 rows, in dwords
constexpr LdPair LD_SCATTERS[] = {{1, 0}, {32, 7}, {17, 3}};
// placed DMA: (modulus of the base chunk or unit, chunks or units added
// by the instruction offset)
constexpr LdPair LD_PLACED_X4[] = {{10, 0}, {8, 1}, {8, 2}};
constexpr LdPair LD_PLACED_DWORD[] = {{37, 0}, {37, 3}};
#define LD_N_B32 10u
#define LD_N_WIDE 6u
#define LD_N_SCATTER 3u
static_assert(63u * 32u + 7u < LD_BANK && 63u * 17u + 3u < LD_BANK, "scatters stay inside");
// no global source index leaves its table: the last chunk and unit a
// placed copy can reach end at the end of a wave's part of G
static_assert((10u - 1u + 0u + 1u) * LD_CHUNK <= LD_SLICE &&
                  (8u - 1u + 2u + 1u) * LD_CHUNK <= LD_SLICE &&
                  (37u - 1u + 3u + 1u) * LD_UNIT <= LD_SLICE,
              "placed copies stay inside the slice");

// Every LDS access goes through one of these, whole: accesses of
// different widths to the same cells must stay in program order.  The
// attribute has to sit on a struct: on a typedef it is lost where the type
// becomes a template argument, and the compiler then moves a dword load
// ahead of a 16-bit store to the same dword.
typedef u32 ld_v2 __attribute__((ext_vector_type(2)));
typedef u32 ld_v4 __attribute__((ext_vector_type(4)));
struct __attribute__((may_alias)) ld_b {
  unsigned char x;
};
struct __attribute__((may_alias)) ld_sb {
  signed char x;
};
struct __attribute__((may_alias)) ld_h {
  unsigned short x;
};
struct __attribute__((may_alias)) ld_sh {
  short x;
};
struct __attribute__((may_alias)) ld_w {
  u32 x;
};
struct __attribute__((may_alias)) ld_w2 {
  ld_v2 x;
};
struct __attribute__((may_alias, aligned(16))) ld_w3 {  // 12 bytes aligned to 16
  u32 x[3];
};
struct __attribute__((may_alias)) ld_w4 {
  ld_v4 x;
};
typedef short ld_s4 __attribute__((ext_vector_type(4)));

#if __HIP_DEVICE_COMPILE__

extern __shared__ u32 ld_mem[];

// a typed pointer to absolute LDS byte address `byte`
template <typename T>
LD_DEV LD_LDS(T) ld_at(u32 byte) {
  return (LD_LDS(T))((LD_LDS(unsigned char))ld_mem + byte);
}

LD_DEV u32 ld_tag(u32 a) { return cu_fmix32(0xA5A5A5A5u ^ (a * 0x9E3779B9u)); }
LD_DEV u32 ld_v(u32 base, u32 k, u32 lane) { return cu_fmix32(base + 64u * k + lane); }
LD_DEV u32 ld_u(u32 base, u32 k) { return cu_fmix32(base + 64u * k); }
LD_DEV u32 ld_img(u32 base, u32 i) { return cu_fmix32(base + LD_IMG0 + i); }

// Where a stage's values go: into the digest, or into the element dump
// (row `slot`, column lane) of the one wave that is asked for.
struct LdFold {
  u32 d = 0;
  LD_DEV void put(u32 slot, u32 lane, u32 v) { d += cu_fmix32(v + cu_salt(64u * slot + lane)); }
};

struct LdDump {
  u32* out;
  bool on;
  LD_DEV void put(u32 slot, u32 lane, u32 v) {
    if (on) out[64u * slot + lane] = v;
  }
};

// dword c of a value of 1 to 4 dwords
LD_DEV u32 ld_get(const ld_w& v, u32) { return v.x; }
template <typename V>
LD_DEV u32 ld_get(const V& v, u32 c) { return v.x[c]; }
LD_DEV void ld_set(ld_w& v, u32, u32 x) { v.x = x; }
template <typename V>
LD_DEV void ld_set(V& v, u32 c, u32 x) { v.x[c] = x; }

// N dwords of operand slots k0 .. at absolute dword a, tagged
template <typename V, u32 N>
LD_DEV void ld_write_vec(u32 a, u32 base, u32 k0, u32 lane) {
  V x;
#pragma unroll
  for (u32 c = 0; c < N; ++c) ld_set(x, c, ld_v(base, k0 + c, lane) ^ ld_tag(a + c));
  *ld_at<V>(4u * a) = x;
}

// N dwords at absolute dword a into N slots, the tags removed
template <typename V, u32 N, typename SINK>
LD_DEV void ld_read_vec(u32 a, u32& n, u32 lane, SINK& sink, bool tagged = true) {
  const V x = *ld_at<V>(4u * a);
#pragma unroll
  for (u32 c = 0; c < N; ++c)
    sink.put(n++, lane, tagged ? ld_get(x, c) ^ ld_tag(a + c) : ld_get(x, c));
}

// N dwords of the image (complemented by inv) from dword i of the slice
// at absolute dword sl, tagged, as one 16-byte store
LD_DEV void ld_fill4(u32 base, u32 sl, u32 i, u32 inv) {
  ld_w4 x;
#pragma unroll
  for (u32 c = 0; c < 4u; ++c) x.x[c] = ld_img(base, i + c) ^ inv ^ ld_tag(sl + i + c);
  *ld_at<ld_w4>(4u * (sl + i)) = x;
}

// ---- stage 0: every access width, inside the wave's slice at absolute
// dword sl

template <typename SINK>
LD_DEV u32 ld_stage_width(u32 base, u32 sl, u32 lane, SINK& sink) {
  u32 n = 0;
  for (u32 t = 0; t < LD_SLICE / 64u; ++t) {
    const u32 i = 64u * t + lane;
    *ld_at<ld_w>(4u * (sl + i)) = ld_w{ld_img(base, i) ^ ld_tag(sl + i)};
  }
  // narrow stores: each followed by its whole dword and the next one;
  // then a lane reads, zero- and sign-extended, the byte or half that
  // lanes (l + u) mod 64 stored (its own would never leave the registers)
#pragma unroll
  for (u32 j = 0; j < 2u; ++j) {
    const u32 d = sl + 2u * lane + j, b = (lane + ld_u(base, 0u) + j) & 3u;
    const u32 val = (ld_v(base, 1u + j, lane) & 0x7Fu) | (((lane >> 2) & 1u) << 7);
    *ld_at<ld_b>(4u * d + b) = ld_b{(unsigned char)(val ^ (ld_tag(d) >> (8u * b)))};
    ld_read_vec<ld_w, 1u>(sl + 2u * lane, n, lane, sink);
    ld_read_vec<ld_w, 1u>(sl + 2u * lane + 1u, n, lane, sink);
#pragma unroll
    for (u32 sign = 0; sign < 2u; ++sign) {
      const u32 rl = (lane + ld_u(base, 27u + sign)) & 63u;
      const u32 rd = sl + 2u * rl + j, rb = (rl + ld_u(base, 0u) + j) & 3u;
      const u32 tb = (ld_tag(rd) >> (8u * rb)) & 0xFFu;
      if (sign == 0u) {
        const ld_b x = *ld_at<ld_b>(4u * rd + rb);
        sink.put(n++, lane, (u32)x.x ^ tb);
      } else {
        // the tag byte is extended like the load (spelled so that the
        // compiler does not extend after the XOR and load unsigned)
        const ld_sb x = *ld_at<ld_sb>(4u * rd + rb);
        sink.put(n++, lane, (u32)(int)x.x ^ (tb | ((0u - (tb >> 7)) << 8)));
      }
    }
  }
#pragma unroll
  for (u32 j = 0; j < 2u; ++j) {
    const u32 d = sl + 128u + 2u * lane + j, h = (lane + ld_u(base, 3u) + j) & 1u;
    const u32 val = (ld_v(base, 4u + j, lane) & 0x7FFFu) | (((lane >> 1) & 1u) << 15);
    *ld_at<ld_h>(4u * d + 2u * h) = ld_h{(unsigned short)(val ^ (ld_tag(d) >> (16u * h)))};
    ld_read_vec<ld_w, 1u>(sl + 128u + 2u * lane, n, lane, sink);
    ld_read_vec<ld_w, 1u>(sl + 129u + 2u * lane, n, lane, sink);
#pragma unroll
    for (u32 sign = 0; sign < 2u; ++sign) {
      const u32 rl = (lane + ld_u(base, 29u + sign)) & 63u;
      const u32 rd = sl + 128u + 2u * rl + j, rh = (rl + ld_u(base, 3u) + j) & 1u;
      const u32 th = (ld_tag(rd) >> (16u * rh)) & 0xFFFFu;
      if (sign == 0u) {
        const ld_h x = *ld_at<ld_h>(4u * rd + 2u * rh);
        sink.put(n++, lane, (u32)x.x ^ th);
      } else {
        const ld_sh x = *ld_at<ld_sh>(4u * rd + 2u * rh);
        sink.put(n++, lane, (u32)(int)x.x ^ (th | ((0u - (th >> 15)) << 16)));
      }
    }
  }
  // wide accesses: a lane reads what lane (l + u) mod 64 stored
#define LD_ROT(k) ((lane + ld_u(base, (k))) & 63u)
  ld_write_vec<ld_w2, 2u>(sl + 256u + 2u * lane, base, 7u, lane);
  ld_read_vec<ld_w2, 2u>(sl + 256u + 2u * LD_ROT(6u), n, lane, sink);
  ld_write_vec<ld_w3, 3u>(sl + 384u + 4u * lane, base, 9u, lane);
  ld_read_vec<ld_w3, 3u>(sl + 384u + 4u * LD_ROT(12u), n, lane, sink);
  ld_read_vec<ld_w4, 4u>(sl + 384u + 4u * LD_ROT(13u), n, lane, sink);
  ld_write_vec<ld_w4, 4u>(sl + 640u + 4u * lane, base, 14u, lane);
  ld_read_vec<ld_w4, 4u>(sl + 640u + 4u * LD_ROT(18u), n, lane, sink);
  {
    // 8 bytes aligned to 4, as two dwords: the two-address forms
    const u32 a = sl + 897u + 2u * lane, ra = sl + 897u + 2u * LD_ROT(21u);
    LD_LDS(ld_w) p = ld_at<ld_w>(4u * a);
    p[0] = ld_w{ld_v(base, 19u, lane) ^ ld_tag(a)};
    p[1] = ld_w{ld_v(base, 20u, lane) ^ ld_tag(a + 1u)};
    LD_LDS(ld_w) q = ld_at<ld_w>(4u * ra);
    const ld_w x0 = q[0], x1 = q[1];
    sink.put(n++, lane, x0.x ^ ld_tag(ra));
    sink.put(n++, lane, x1.x ^ ld_tag(ra + 1u));
  }
  {
    // two dwords 64 * LD_ST64_K apart: the st64 forms
    const u32 a = sl + 1088u + lane, far = 64u * LD_ST64_K;
    LD_LDS(ld_w) p = ld_at<ld_w>(4u * a);
    p[0] = ld_w{ld_v(base, 22u, lane) ^ ld_tag(a)};
    p[far] = ld_w{ld_v(base, 23u, lane) ^ ld_tag(a + far)};
    const u32 ra = sl + 1088u + LD_ROT(24u);
    LD_LDS(ld_w) q = ld_at<ld_w>(4u * ra);
    const ld_w x0 = q[0], x1 = q[far];
    sink.put(n++, lane, x0.x ^ ld_tag(ra));
    sink.put(n++, lane, x1.x ^ ld_tag(ra + far));
  }
#undef LD_ROT
  // transposed reads: within a group of 16 lanes, lane 4q + p supplies
  // row q, columns 4p .. 4p + 3 of a 4 x 16 block of 16-bit elements and
  // lane i receives column i, row q in element q.  EXEC is all ones.
  // The tag of each element is that of the address its supplier gave.
#pragma unroll
  for (u32 t = 0; t < 2u; ++t) {
    const u32 byte = 8u * (ld_v(base, 25u + t, lane) % (LD_SLICE / 2u));
    const ld_s4 x = __builtin_amdgcn_ds_read_tr16_b64_v4i16(ld_at<ld_s4>(4u * sl + byte));
    const u32 group = lane & ~15u, i = lane & 15u;
    u32 e[4];
#pragma unroll
    for (u32 q = 0; q < 4u; ++q) {
      const u32 src = group + 4u * q + (i >> 2);
      const u32 at = 8u * (ld_v(base, 25u + t, src) % (LD_SLICE / 2u)) + 2u * (i & 3u);
      const u32 tg = (ld_tag(sl + (at >> 2)) >> (16u * ((at >> 1) & 1u))) & 0xFFFFu;
      e[q] = (u32)(unsigned short)x[q] ^ tg;
    }
    sink.put(n++, lane, e[0] | (e[1] << 16));
    sink.put(n++, lane, e[2] | (e[3] << 16));
  }
  return n;
}

// ---- stage 1: bank conflicts, broadcasts, gather and scatter, on the
// first LD_BANK dwords of the slice

template <typename SINK>
LD_DEV u32 ld_stage_bank(u32 base, u32 sl, u32 lane, SINK& sink) {
  u32 n = 0;
  for (u32 t = 0; t < LD_BANK / 256u; ++t) ld_fill4(base, sl, 4u * (64u * t + lane), 0u);
#pragma unroll
  for (u32 j = 0; j < LD_N_B32; ++j)
    ld_read_vec<ld_w, 1u>(sl + ((lane * LD_B32_STRIDES[j] + ld_u(base, j)) & (LD_BANK - 1u)), n,
                          lane, sink);
#pragma unroll
  for (u32 j = 0; j < LD_N_WIDE; ++j)
    ld_read_vec<ld_w2, 2u>(
        sl + 2u * ((lane * LD_WIDE_STRIDES[j] + ld_u(base, 10u + j)) & (LD_BANK / 2u - 1u)), n,
        lane, sink);
#pragma unroll
  for (u32 j = 0; j < LD_N_WIDE; ++j)
    ld_read_vec<ld_w4, 4u>(
        sl + 4u * ((lane * LD_WIDE_STRIDES[j] + ld_u(base, 16u + j)) & (LD_BANK / 4u - 1u)), n,
        lane, sink);
  // every lane on one address; two addresses by l & 1; a free gather
  ld_read_vec<ld_w, 1u>(sl + (ld_u(base, 22u) & (LD_BANK - 1u)), n, lane, sink);
  ld_read_vec<ld_w, 1u>(sl + (ld_u(base, 23u + (lane & 1u)) & (LD_BANK - 1u)), n, lane, sink);
  ld_read_vec<ld_w, 1u>(sl + (ld_v(base, 25u, lane) & (LD_BANK - 1u)), n, lane, sink);
  // scatters: lane l stores to row (a l + b) mod 64 with a odd, a
  // bijection, so no two lanes write one cell; read back in row order
#pragma unroll
  for (u32 p = 0; p < LD_N_SCATTER; ++p) {
    const u32 u = ld_u(base, 26u + 2u * p);
    const u32 row = ((u | 1u) * lane + (u >> 8)) & 63u;
    ld_write_vec<ld_w, 1u>(sl + LD_SCATTERS[p].a * row + LD_SCATTERS[p].b, base, 27u + 2u * p,
                           lane);
    ld_read_vec<ld_w, 1u>(sl + LD_SCATTERS[p].a * lane + LD_SCATTERS[p].b, n, lane, sink);
  }
  return n;
}

// ---- stage 2: LDS-DMA.  tables: G[16][LD_SLICE] tagged, then
// X[LD_X_DWORDS] untagged.

// One global_load_lds of SIZE bytes per lane: lane l's bytes at g + OFF
// go to absolute LDS dword `to` (wave-uniform: the M0 base) + OFF + SIZE l.
// The builtin takes SIZE and OFF only as literals.
#define LD_DMA(SIZE, OFF, g, to) \
  __builtin_amdgcn_global_load_lds((LD_GLB(void))(g), ld_at<void>(4u * (to)), SIZE, OFF, 0)
static_assert(4u * LD_CHUNK * LD_PLACED_X4[1].b == 1024u &&
                  4u * LD_CHUNK * LD_PLACED_X4[2].b == 2048u &&
                  4u * LD_UNIT * LD_PLACED_DWORD[1].b == 768u && LD_PLACED_X4[0].b == 0u &&
                  LD_PLACED_DWORD[0].b == 0u && LD_PLACED_X4[1].a == LD_PLACED_X4[2].a &&
                  LD_PLACED_DWORD[0].a == LD_PLACED_DWORD[1].a,
              "the instruction offsets below are those of the tables");

// s_waitcnt lgkmcnt(0): this wave's LDS loads and stores have finished,
// so a DMA may overwrite their cells
LD_DEV void ld_wait_lds() { __builtin_amdgcn_s_waitcnt(0xC07F); }
// s_waitcnt vmcnt(0): this wave's DMAs have landed in the LDS
LD_DEV void ld_wait_dma() { __builtin_amdgcn_s_waitcnt(0x0F70); }

template <typename SINK>
LD_DEV u32 ld_stage_dma(u32 base, u32 sl, u32 wib, u32 lane, const u32* __restrict__ tables,
                        SINK& sink) {
  u32 n = 0;
  // every index below is reduced into its table before it is used
  const u32* G = tables + (wib % CU_WAVES) * LD_SLICE;
  const u32* X = tables + LD_G_DWORDS;
  const u32 c0 = LD_CHUNK * (ld_u(base, 0u) % LD_PLACED_X4[0].a);
  const u32 c1 = LD_CHUNK * (ld_u(base, 1u) % LD_PLACED_X4[1].a);
  const u32 d0 = LD_UNIT * (ld_u(base, 2u) % LD_PLACED_DWORD[0].a);
  // placed: chunks of the wave's part of G to the same dwords of its slice
  ld_wait_lds();
  LD_DMA(16, 0, G + c0 + 4u * lane, sl + c0);
  LD_DMA(16, 1024, G + c1 + 4u * lane, sl + c1);
  LD_DMA(16, 2048, G + c1 + 4u * lane, sl + c1);
  LD_DMA(4, 0, G + d0 + lane, sl + d0);
  LD_DMA(4, 768, G + d0 + lane, sl + d0);
  ld_wait_dma();
  ld_read_vec<ld_w4, 4u>(sl + c0 + 4u * lane, n, lane, sink);
  ld_read_vec<ld_w4, 4u>(sl + c1 + LD_CHUNK * LD_PLACED_X4[1].b + 4u * lane, n, lane, sink);
  ld_read_vec<ld_w4, 4u>(sl + c1 + LD_CHUNK * LD_PLACED_X4[2].b + 4u * lane, n, lane, sink);
  ld_read_vec<ld_w, 1u>(sl + d0 + lane, n, lane, sink);
  ld_read_vec<ld_w, 1u>(sl + d0 + LD_UNIT * LD_PLACED_DWORD[1].b + lane, n, lane, sink);
  // gather: per-lane source addresses into X, lane-linear destination
#pragma unroll
  for (u32 g = 0; g < 2u; ++g) {
    const u32 src = ld_v(base, 3u + g, lane) & (LD_X_DWORDS - 4u);
    const u32 to = sl + LD_CHUNK * (ld_u(base, 5u + g) % (LD_SLICE / LD_CHUNK));
    ld_wait_lds();
    LD_DMA(16, 0, X + src, to);
    ld_wait_dma();
    ld_read_vec<ld_w4, 4u>(to + 4u * lane, n, lane, sink, false);
  }
#pragma unroll
  for (u32 g = 0; g < 2u; ++g) {
    const u32 src = ld_v(base, 7u + g, lane) & (LD_X_DWORDS - 1u);
    const u32 to = sl + LD_UNIT * (ld_u(base, 9u + g) % (LD_SLICE / LD_UNIT));
    ld_wait_lds();
    LD_DMA(4, 0, X + src, to);
    ld_wait_dma();
    ld_read_vec<ld_w, 1u>(to + lane, n, lane, sink, false);
  }
  return n;
}

// ---- stage 3: the whole array, across waves.  All 16 waves of the
// workgroup run this together.

template <typename SINK>
LD_DEV u32 ld_stage_xwave(u32 base, u32 rp, u32 sl, u32 wib, u32 lane, SINK& sink) {
  u32 n = 0;
#pragma unroll 1
  for (u32 phase = 0; phase < 2u; ++phase) {
    const u32 inv = phase ? 0xFFFFFFFFu : 0u;
    for (u32 t = 0; t < LD_SLICE / 256u; ++t) ld_fill4(base, sl, 4u * (64u * t + lane), inv);
    __syncthreads();
#pragma unroll 1
    for (u32 j = 0; j < 3u; ++j) {
      const u32 partner = (wib + 1u + (3u * rp + j) % 15u) % CU_WAVES;
      for (u32 t = 0; t < LD_SLICE / 256u; ++t)
        ld_read_vec<ld_w4, 4u>(partner * LD_SLICE + 4u * (64u * t + lane), n, lane, sink);
    }
    // the partners have read this slice before anything is stored to it
    __syncthreads();
  }
  return n;
}

#endif  // __HIP_DEVICE_COMPILE__

__global__ void __launch_bounds__(CU_BLOCK)
ldscheck_kernel(CuArgs a, const u32* __restrict__ tables) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane, wib = threadIdx.x / WAVE;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % LD_PERIOD;
    // r >> 17 is 0, as rounds <= MAX_ROUNDS, but the compiler cannot know:
    // it would otherwise compute the tag of every address once, ahead of
    // the loop, and keep some sixty of them in scratch memory
    const u32 sl = wib * LD_SLICE + (r >> 17);
    // Each stage's digest is summed over the wave where the stage ends: the
    // sum is a cross-lane operation that stays in its place, so the stage's
    // values are folded while they are in registers.  Left to the end of the
    // round, the compiler moves the folding there too, and keeps every loaded
    // value alive (in scratch memory) until then.
    LdFold f0, f1, f2, f3;
    ld_stage_width(cu_base(a.seed, LD_STAGE0 + 0, rp), sl, lane, f0);
    const u32 d0 = wave_sum(f0.d);
    ld_stage_bank(cu_base(a.seed, LD_STAGE0 + 1, rp), sl, lane, f1);
    const u32 d1 = wave_sum(f1.d);
    ld_stage_dma(cu_base(a.seed, LD_STAGE0 + 2, rp), sl, wib, lane, tables, f2);
    const u32 d2 = wave_sum(f2.d);
    ld_stage_xwave(cu_base(a.seed, LD_STAGE0 + 3, rp), rp, sl, wib, lane, f3);
    u32 dig[N_STAGES] = {d0, d1, d2, wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One full workgroup runs one stage and round, and wave `wave` of it
// writes every value it would fold, out[64 * slot + lane], and the number
// of slots behind the last row.  A digest cannot say which access moved
// what; this can.
__global__ void __launch_bounds__(CU_BLOCK)
ldscheck_values_kernel(u32 seed, u32 stage, u32 r, u32 wave, const u32* __restrict__ tables,
                       u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  const u32 lane = threadIdx.x % WAVE, wib = threadIdx.x / WAVE;
  const u32 rp = r % LD_PERIOD;
  const u32 base = cu_base(seed, LD_STAGE0 + stage, rp);
  const u32 sl = wib * LD_SLICE;
  LdDump sink;
  sink.out = out;
  sink.on = wib == wave;
  u32 n;
  if (stage == 0u) n = ld_stage_width(base, sl, lane, sink);
  else if (stage == 1u) n = ld_stage_bank(base, sl, lane, sink);
  else if (stage == 2u) n = ld_stage_dma(base, sl, wib, lane, tables, sink);
  else n = ld_stage_xwave(base, rp, sl, wib, lane, sink);
  if (threadIdx.x == 0u) out[64u * LD_VALUE_SLOTS] = n;
#endif
}

// ---------------------------------------------------------------- host

static void ld_check_tables(const at::Tensor& tables, const at::Device& device) {
  TORCH_CHECK(tables.is_cuda() && tables.device() == device,
              "ldscheck: tables must be on the GPU that runs the kernel");
  TORCH_CHECK(tables.scalar_type() == at::kInt && tables.is_contiguous(),
              "ldscheck: tables must be a contiguous int32 tensor");
  TORCH_CHECK(tables.numel() == (int64_t)LD_TABLE_DWORDS, "ldscheck: tables must hold ",
              LD_TABLE_DWORDS, " elements (G[16][2560], X[4096]), got ", tables.numel());
}

// `tables` (int32, LD_TABLE_DWORDS elements, probe/ldscheck.py's
// source_tables) is only read.
CucheckOut ldscheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                        int64_t blocks_arg, at::Tensor tables, int64_t max_records,
                        c10::optional<at::Tensor> dump, c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("ldscheck", expected, seed_arg, rounds, blocks_arg, max_records,
                          dump, inject);
  ld_check_tables(tables, expected.device());
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(ldscheck_kernel, l, MAX_LDS_BYTES, (const u32*)tables.data_ptr());
}

// What wave `wave` of a workgroup folds for one stage and round as an
// int32 tensor on the tables' GPU: LD_VALUE_SLOTS rows of 64 lanes, then
// the number of rows the stage filled.
at::Tensor ldscheck_values(int64_t seed_arg, int64_t stage, int64_t round, at::Tensor tables,
                           int64_t wave) {
  cu_check_wave_args("ldscheck", seed_arg, stage, round);
  TORCH_CHECK(wave >= 0 && wave < CU_WAVES, "ldscheck: wave must be in 0..", CU_WAVES - 1,
              ", got ", wave);
  TORCH_CHECK(tables.is_cuda(), "ldscheck: tables must be on the GPU that runs the kernel");
  ld_check_tables(tables, tables.device());
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(tables));
  at::Tensor out = at::zeros({(int64_t)(64 * LD_VALUE_SLOTS + 1)},
                             tables.options().dtype(at::kInt));
  return cu_launch_values(ldscheck_values_kernel, CU_BLOCK, MAX_LDS_BYTES, out, (u32)seed_arg,
                          (u32)stage, (u32)round, (u32)wave, (const u32*)tables.data_ptr(),
                          (u32*)out.data_ptr());
}

typedef std::tuple<int64_t, int64_t> LdRow;

template <size_t N>
static std::vector<LdRow> ld_rows(const LdPair (&t)[N]) {
  std::vector<LdRow> out;
  for (const LdPair& p : t) out.emplace_back(p.a, p.b);
  return out;
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/ldscheck_mi355x.json).
void bind_ldscheck(py::module_& m) {
  m.def("ldscheck_run", &ldscheck_run,
        "LDS integrity run -> (mismatches, first_bad_round, stage_mask, records, waves_on, "
        "elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("tables"), py::arg("max_records") = 16, py::arg("dump") = py::none(),
        py::arg("inject") = py::none());
  m.def("ldscheck_values", &ldscheck_values,
        "values one wave of a workgroup folds for one stage and round as int32 "
        "[256 rows * 64 lanes + 1]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"), py::arg("tables"),
        py::arg("wave") = 0);
  m.def("ldscheck_layout", []() {
          std::vector<int64_t> b32(LD_B32_STRIDES, LD_B32_STRIDES + LD_N_B32);
          std::vector<int64_t> wide(LD_WIDE_STRIDES, LD_WIDE_STRIDES + LD_N_WIDE);
          std::vector<int64_t> sizes = {LD_SLICE, LD_BANK, LD_ST64_K, LD_CHUNK, LD_UNIT,
                                        LD_X_DWORDS, LD_TABLE_DWORDS};
          return std::make_tuple((int64_t)LD_PERIOD, (int64_t)LD_VALUE_SLOTS, sizes, b32, wide,
                                 ld_rows(LD_SCATTERS), ld_rows(LD_PLACED_X4),
                                 ld_rows(LD_PLACED_DWORD));
        },
        "(period, value rows, (slice, bank region, st64 distance / 64, x4 chunk, dword "
        "unit, X and table dwords), b32 strides, wide strides, scatters (stride, offset), "
        "placed x4 and dword copies (modulus, added by the instruction offset))");
}
