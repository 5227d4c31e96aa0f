// What gemmcheck.hip (bf16 / i8), gemmcheck_mx.hip (MXFP8 / MXFP4) and
// gemmcheck_mx6.hip (e5m2, MXFP6 and mixed formats) share: the tile and LDS geometry, the kernels' arguments, the tile walk,
// the two sinks for C, the default grid and the result block.  The header
// comment of gemmcheck.hip explains each piece.

#pragma once

#include "cucheck_common.h"

#include <string>

typedef u32 u32x4 __attribute__((ext_vector_type(4)));

#define GC_THREADS 256
#define GC_WAVES (GC_THREADS / WAVE)
#define GC_TILE 128            // rows and columns of C per workgroup
#define GC_SLAB_BYTES 128      // bytes of K per row and slab
#define GC_ROW_UNITS 8u        // 16-byte units of a slab row
#define GC_OP_UNITS 1024u      // 128 rows: one operand of one stage
#define GC_STAGE_UNITS 2048u   // A and Bt
#define GC_LDS_BYTES (2 * GC_STAGE_UNITS * 16)
#define GC_MAX_STEPS 0x7FFFFFFFLL

// What the kernels take after CuArgs.  Operands in 16-byte units.
struct GcArgs {
  const u32x4* a;   // [128 tm, 8 slabs]
  const u32x4* bt;  // [128 tn, 8 slabs]
  u32* out;         // [128 tm, 128 tn] for GcStore, else null
  u32 tm, tn;       // tiles down and across
  u32 slabs;        // K in slabs
  u32 steps;        // rounds tm tn
};

// Step u of a round -> tile (bi, bj); see "Tile order" in gemmcheck.hip.
__device__ __forceinline__ void gc_tile(u32 u, u32 tm, u32 tn, u32& bi, u32& bj) {
  if (((tm | tn) & 7u) == 0u && (((tm >> 3) * (tn >> 3)) & 7u) == 0u) {
    const u32 v = u >> 3, sb = ((v >> 6) << 3) | (u & 7u), sn = tn >> 3;
    bi = 8u * (sb / sn) + ((v >> 3) & 7u);
    bj = 8u * (sb % sn) + (v & 7u);
  } else {
    bi = u / tn;
    bj = u % tn;
  }
}

// What a wave needs to know at the end of a tile.
struct GcWhere {
  int lane;
  u32 gwave, hw, quadrant;
  u32 round, bi, bj;
  bool first_of_round;  // the workgroup's first tile of this round
};

struct GcStore {
  u32* at;  // the tile's origin in out
  size_t n;
  __device__ __forceinline__ GcStore(const GcArgs& g, u32 bi, u32 bj)
      : at(g.out + ((size_t)bi * GC_TILE * g.tn + bj) * GC_TILE), n((size_t)g.tn * GC_TILE) {}
  __device__ __forceinline__ void put(u32 i, u32 j, u32 bits) { at[i * n + j] = bits; }
  __device__ __forceinline__ void finish(const CuArgs&, const GcArgs&, u32, const GcWhere&) {}
};

struct GcFold {
  u32 part = 0;  // this lane's share of the quadrant's fold
  __device__ __forceinline__ GcFold(const GcArgs&, u32, u32) {}
  __device__ __forceinline__ void put(u32 i, u32 j, u32 bits) {
    part += cu_fmix32(bits + cu_salt(GC_TILE * i + j));
  }
  __device__ __forceinline__ void finish(const CuArgs& a, const GcArgs& g, u32 stage,
                                         const GcWhere& w) {
    u32 d = wave_sum(part);
    if (w.gwave == a.inj_wave && w.round == a.inj_round && w.first_of_round) d ^= a.inj_mask;
    if (w.lane == 0) {
      const u32 want = a.expected[4u * (2u * (w.bi & 1u) + (w.bj & 1u)) + w.quadrant];
      if (d != want)
        log_mismatch(a.res, a.max_records, 4u * (w.bi * g.tn + w.bj) + w.quadrant, w.hw,
                     w.round, stage, want, d);
    }
  }
};

// What the block-scaled kernels take: GcArgs and the scales, in the words
// a slab's scale bytes of one row make: [128 tm, slabs] and [128 tn, slabs].
struct GcmArgs {
  GcArgs g;
  const void* sa;
  const void* sb;
};

__device__ __forceinline__ u32 gcm_f32_bits(float c) {
  u32 b = __float_as_uint(c);
  return (b << 1) == 0u ? 0u : b;
}

// ---------------------------------------------------------------- host

// blocks = 0: two workgroups per CU, or one per step if that is fewer.
static inline int64_t gc_grid(int64_t blocks_arg, int64_t steps) {
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= MAX_BLOCKS, "gemmcheck: blocks must be in 0..",
              MAX_BLOCKS, ", got ", blocks_arg);
  if (blocks_arg != 0) return blocks_arg;
  int64_t full = 2 * (int64_t)at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  return steps < full ? steps : full;
}

// A zeroed result block as cu_prepare makes it.
static inline at::Tensor gc_result_block(const at::Tensor& like, int64_t max_records) {
  at::Tensor res = at::zeros({RES_RECORDS + RECORD_WORDS * max_records},
                             like.options().dtype(at::kInt));
  res.select(0, RES_FIRST).fill_(-1);  // u32 max: identity for atomicMin
  return res;
}

// The block-scaled files' host side.  A launcher starts one instantiation
// of a kernel on `blocks` workgroups; gcm_gemm and gcm_run (gemmcheck_mx.hip)
// are the bodies of gemm_mx_nt and gemmcheck_mx_run for any of them.
typedef void (*GcmLaunch)(int64_t blocks, const CuArgs& ca, const GcmArgs& m);
at::Tensor gcm_gemm(GcmArgs m, GcmLaunch store, const at::Tensor& a, int64_t blocks_arg);
CucheckOut gcm_run(GcmArgs m, u32 stage, GcmLaunch fold, const at::Tensor& a,
                   const at::Tensor& expected, int64_t rounds, int64_t blocks_arg,
                   int64_t max_records, const c10::optional<CuInject>& inject);

// A format of gemmcheck_mx6.hip: its stage of the records, its operand
// checks (which fill the shape) and its two launchers.
struct GcxFormat {
  const char* name;
  u32 stage;
  GcmArgs (*check)(const at::Tensor& a, const at::Tensor& a_scale, const at::Tensor& bt,
                   const at::Tensor& bt_scale);
  GcmLaunch store, fold;
};
// null where `format` is none of that file's
const GcxFormat* gcx_format(const std::string& format);
