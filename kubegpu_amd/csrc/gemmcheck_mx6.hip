// gemmcheck_mx6 — more of the OCP MX family under load: stages 4..7 of
// the full-chip tiled-GEMM load probe (gfx950), compiled into _gpuprobe next
// to gemmcheck_mx.hip, whose kernel stays as it is.
//
//   C[M,N] (f32) = sum over k of A[i][k] 2^(SA[i][k/32] - 127)
//                              . Bt[j][k] 2^(SB[j][k/32] - 127)
// as there, on v_mfma_scale_f32_32x32x64_f8f6f4, but with the element format
// and the LDS geometry chosen per operand (cbsz for A, blgp for Bt):
//   stage 4  mxfp8_e5m2        e5m2 x e5m2                  (cbsz = blgp = 1)
//   stage 5  mxfp6_e2m3        e2m3 x e2m3, packed          (2, 2)
//   stage 6  mxfp6_e3m2        e3m2 x e3m2, packed          (3, 3)
//   stage 7  mxfp8_e5m2:mxfp8  e5m2 x e4m3 (FP8 backward)   (1, 0)
// matcheck proves these forms of the instruction from registers, one wave;
// here their operands come from HBM through LDS with every CU busy: the
// 192-bit fp6 fetch and format fields 1..3.  probe/gemmcheck.py is the
// definition of operands, scales and expected folds; the compare is bit for
// bit.  Left out: e4m3 x e2m1 ("mxfp8:mxfp4", cbsz 0, blgp 4).  It was built
// here as a third geometry (64-byte rows, unit(row, c) = 4 row + (c ^
// ((row>>2) & 3)), one ds_read_b128 into registers 0..3) and on an MI355X
// every element of its product was wrong, as matcheck's e2m1 x e4m3 form is
// (probe/matcheck.py, "Not covered"): how the instruction reads four
// registers of fp4 beside eight of fp8 is not known here.
//
// What is the siblings' (gemmcheck_common.h, the header comments of
// gemmcheck.hip and gemmcheck_mx.hip): 256 threads, four waves 2x2 on a
// 128x128 tile, 2x2 accumulators of 32x32 per wave, two LDS stages with one
// barrier per slab, global -> register -> LDS staging that overlaps the
// MFMAs, the walk over rounds x tiles, the XCD super-block tile order, the
// GcStore / GcFold sinks, the epilogue's DPP move, the scale words.  What is
// new:
//
// Slab.  128 elements of K for every format: KSTEPS = 2 issues of 64, four
// scale blocks, so one aligned 32-bit scale word per row and slab and
// op_sel 0 / 2 exactly as for mxfp8.  A slab row is 128 bytes (fp8) or 96
// (fp6), and A and Bt each have their own format field, staging map, LDS
// region and fragment read (the structs GcxFp8 and GcxFp6 below); a stage
// of LDS is A's region followed by Bt's.
//
// Fragments.  Lane l holds row l&31 and the 32 elements of half h = l>>5 of
// an issue: scale block b = 2 kk + h of the slab.
//   fp8  32 bytes at byte 32 b: the sibling's two ds_read_b128.
//   fp6  24 bytes at byte 24 b, the block's 192-bit little-endian integer,
//        into registers 0..5.  24 b is a multiple of 8 and, for odd b, of
//        nothing more, so the fragment is three ds_read_b64 (the compiler
//        may pair two into a ds_read2_b64); a b128 + b64 split would need
//        its order, and so its target registers, to depend on the lane.
//   Registers the format does not read stay zero and the compiler picks the
//   8- or 6-register form per operand.
//
// Address maps and bank conflicts, counted the sibling's way: the bank line
// is 256 bytes, a b128 access is served sixteen lanes at a time and a b64
// access thirty-two.
//   fp8  the sibling's map, 8 row + (c ^ ((row>>1) & 7)) in 16-byte units,
//        and its argument.
//   fp6  a 96-byte row pitch puts row r's granule at 12 r mod 32 in 8-byte
//        granules: 8 places for 32 rows, a 4-way conflict on every read,
//        and no XOR on a 6-unit row mends it.  The pitch is 104 bytes, 13
//        granules: granule(row, g) = 13 row + g, g = 0..11, the 13th unused;
//        13 KiB per operand and stage.  A fragment read is one g = 3 b + e
//        by the 32 rows of a half-wave: 13 r mod 32 is a bijection (13 is
//        odd), 32 places, conflict-free.  That is two thirds of the
//        operand's LDS traffic and sits in front of the MFMAs, so it is the
//        side that is made free.  Staging: thread t takes the 16-byte units
//        u = t + 256 i, i < 3, row u / 6, chunk u % 6 (six lanes per row and
//        96 contiguous bytes: what the global loads want) and writes each as
//        two b64, granules 2 (u % 6) and + 1, since a row starts 8-byte
//        aligned only.  The 32 units of a half-wave are 64 granules in 5 1/3
//        rows with 5 or 6 unused granules between them, a span of 69 or 70
//        places: some place is hit three times by the two writes together,
//        so one of them has a 2-way conflict whichever granule goes first;
//        the writes are 2-way at worst and 2-way is minimal for this pitch
//        and this thread map.  (Two lanes per row would free the writes: it
//        puts 32 rows instead of 11 under one global load.)
//
// LDS per workgroup, two stages and 2 KiB of scale words: 66 KiB (stages 4
// and 7), 54 KiB (5 and 6); two workgroups fit the CU's 160 KiB.
//
// Resources (gfx950, cross-compiled, -O3), VGPRs with the 64 accumulator
// registers among them: 223 (stages 4 and 7) and 229 (5 and 6) with GcFold,
// 216 and 221 with GcStore; no AGPRs, no scratch, two waves per SIMD.
//
// Measured on MI355X at 8192^3 on the default grid, windows of 2.0 to 2.7 s,
// six kinds alternating, three repetitions, every fold equal to the numpy
// reference (profiles/gemmcheck_mx6_mi355x.json); medians, with the sibling's
// two stages as the session's yardstick (mxfp8 1216 TFLOP/s, 0.904 ms per
// round; mxfp4 2641, 0.416 ms):
//   mxfp8_e5m2 1664 TFLOP/s (0.661 ms)   mxfp8_e5m2:mxfp8 1683 (0.653 ms)
//   mxfp6_e2m3 1080 TFLOP/s (1.018 ms)   mxfp6_e3m2       1078 (1.020 ms)
// The fp6 stages were expected between mxfp8 and mxfp4 and land below
// mxfp8, at 0.65 of this kernel's own fp8 rate with 0.75 of its bytes.  Per
// slab and thread they issue 24 ds_read_b64 where fp8 issues 16
// ds_read_b128 for a third more bytes, 12 b64 staging writes (2-way, above)
// where fp8 issues 8 b128, and the u / 6, u % 6 staging addresses; the
// barrier share is the same.  Which of these costs the time was not
// measured (no counters were collected).  e5m2 was expected to equal mxfp8
// and runs 1.37 times its rate: that compares this kernel with the
// sibling's and e5m2 bit patterns with e4m3 ones, and the two were not
// separated.  Clocks and power: not measured.
//
// No inline assembly, builtins and plain C++ only.

#include "gemmcheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#include <string>

typedef int gcx_i32x8 __attribute__((ext_vector_type(8)));
typedef u32 u32x2 __attribute__((ext_vector_type(2)));

#define GCX_SLAB 128        // elements of K per slab, every format
#define GCX_SCALE_ROWS 256u  // A and Bt rows of one stage, one u32 each

// ------------------------------------------------- operand geometries
//
// Each says how one operand of a 128-row tile moves: ROW_UNITS 16-byte
// units of a slab row in memory, LOADS of them per thread, LDS_UNITS per
// stage; load() fetches the thread's units of the slab at g (the tile's
// first row, row pitch `pitch` units), store() puts them into the region at
// lds, frag() reads the fragment of row `row0 + rl` (row0 a multiple of 32,
// rl < 32) and scale block b of the slab.

template <int FMT_, int64_t TYPE_>
struct GcxFp8 {
  static constexpr int FMT = FMT_;
  static constexpr int64_t TYPE = TYPE_;  // the torch dtype accepted besides uint8
  static constexpr u32 ROW_UNITS = 8, LOADS = 4, LDS_UNITS = 1024;
  static const char* type_name() { return FMT == 0 ? "float8_e4m3fn" : "float8_e5m2"; }

  static __device__ __forceinline__ void load(const u32x4* g, size_t pitch, u32 tid,
                                              u32x4 (&r)[LOADS]) {
    const u32x4* p = g + (size_t)(tid >> 3) * pitch + (tid & 7u);
#pragma unroll
    for (u32 i = 0; i < LOADS; ++i) r[i] = p[32u * i * pitch];
  }
  static __device__ __forceinline__ void store(u32x4* lds, u32 tid, const u32x4 (&r)[LOADS]) {
    const u32 sc = tid & 7u, sr = tid >> 3;  // rows sr + 32 i: the same swizzle
    u32x4* p = lds + 8u * sr + (sc ^ ((sr >> 1) & 7u));
#pragma unroll
    for (u32 i = 0; i < LOADS; ++i) p[256u * i] = r[i];
  }
  static __device__ __forceinline__ gcx_i32x8 frag(const u32x4* lds, u32 row0, u32 rl, u32 b) {
    const u32x4* p = lds + 8u * (row0 + rl);
    const u32 c = (2u * b) ^ ((rl >> 1) & 7u);  // even b: c ^ 1 is the swizzled column + 1
    const u32x4 lo = p[c], hi = p[c ^ 1u];
    return gcx_i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3],
                     (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
  }
};

template <int FMT_>
struct GcxFp6 {
  static constexpr int FMT = FMT_;
  static constexpr int64_t TYPE = -1;
  static constexpr u32 ROW_UNITS = 6, LOADS = 3, PITCH = 13;  // granules of 8 bytes
  static constexpr u32 LDS_UNITS = 128u * PITCH / 2u;
  static const char* type_name() { return nullptr; }

  static __device__ __forceinline__ void load(const u32x4* g, size_t pitch, u32 tid,
                                              u32x4 (&r)[LOADS]) {
#pragma unroll
    for (u32 i = 0; i < LOADS; ++i) {
      const u32 u = tid + 256u * i;
      r[i] = g[(size_t)(u / 6u) * pitch + u % 6u];
    }
  }
  static __device__ __forceinline__ void store(u32x4* lds, u32 tid, const u32x4 (&r)[LOADS]) {
#pragma unroll
    for (u32 i = 0; i < LOADS; ++i) {
      const u32 u = tid + 256u * i;
      u32x2* q = (u32x2*)lds + PITCH * (u / 6u) + 2u * (u % 6u);
      q[0] = u32x2{r[i][0], r[i][1]};
      q[1] = u32x2{r[i][2], r[i][3]};
    }
  }
  static __device__ __forceinline__ gcx_i32x8 frag(const u32x4* lds, u32 row0, u32 rl, u32 b) {
    const u32x2* q = (const u32x2*)lds + PITCH * (row0 + rl) + 3u * b;
    const u32x2 v0 = q[0], v1 = q[1], v2 = q[2];
    return gcx_i32x8{(int)v0[0], (int)v0[1], (int)v1[0], (int)v1[1], (int)v2[0], (int)v2[1], 0, 0};
  }
};

// A stage: A's and Bt's geometry, its number in the records and the K up to
// which the probe's operands keep every partial sum exact.
template <typename A_, typename B_, u32 STAGE_, int64_t MAX_K_>
struct GcxStage {
  typedef A_ A;
  typedef B_ B;
  static constexpr u32 STAGE = STAGE_, STAGE_UNITS = A::LDS_UNITS + B::LDS_UNITS;
  static constexpr int64_t MAX_K = MAX_K_;
  static constexpr size_t LDS_BYTES = 2 * STAGE_UNITS * 16 + 2 * GCX_SCALE_ROWS * sizeof(u32);
};

typedef GcxFp8<0, (int64_t)at::kFloat8_e4m3fn> GcxE4m3;
typedef GcxFp8<1, (int64_t)at::kFloat8_e5m2> GcxE5m2;
// MAX_K: probe/gemmcheck.py, "Bounds"
typedef GcxStage<GcxE5m2, GcxE5m2, 4, 16384> GcxStage4;      // 784 sixteenths . K < 2**24
typedef GcxStage<GcxFp6<2>, GcxFp6<2>, 5, 16384> GcxStage5;  // 900 sixty-fourths
typedef GcxStage<GcxFp6<3>, GcxFp6<3>, 6, 16384> GcxStage6;  // 784 sixteenths
typedef GcxStage<GcxE5m2, GcxE4m3, 7, 32768> GcxStage7;      // 448 quarters

#if __HIP_DEVICE_COMPILE__
extern __shared__ u32x4 gcx_lds[];

// Issue kk of a slab, scale blocks B0 = 2 kk and 2 kk + 1 by the lane's half:
// the fragments of two A and two Bt row blocks and the four MFMAs.  SEL =
// 2 kk is the byte of sa / sb that scales them.
template <typename T, int SEL>
__device__ __forceinline__ void gcx_issue(const u32x4* la, const u32x4* lb, u32 arow, u32 brow,
                                          u32 rl, u32 h, const u32 (&sa)[2], const u32 (&sb)[2],
                                          f32x16 (&acc)[2][2]) {
  gcx_i32x8 fa[2], fb[2];
#pragma unroll
  for (u32 x = 0; x < 2u; ++x) {
    fa[x] = T::A::frag(la, arow + 32u * x, rl, (u32)SEL + h);
    fb[x] = T::B::frag(lb, brow + 32u * x, rl, (u32)SEL + h);
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
      acc[x][y] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          fa[x], fb[y], acc[x][y], T::A::FMT, T::B::FMT, SEL, (int)sa[x], SEL, (int)sb[y]);
}
#endif

template <typename T, typename SINK>
__global__ void __launch_bounds__(GC_THREADS, 2) gemmcheck_mx6_kernel(CuArgs a, GcmArgs m) {
#if __HIP_DEVICE_COMPILE__
  typedef typename T::A A;
  typedef typename T::B B;
  const GcArgs& g = m.g;
  const u32 tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
  GcWhere w;
  w.lane = (int)lane;
  w.gwave = blockIdx.x * GC_WAVES + wv;
  w.hw = cu_locate_wave(a.res, (int)lane);
  w.quadrant = wv;
  const u32 wr = wv >> 1, wc = wv & 1u;

  // a stage is A's region, then Bt's; the scale words [stage][256] follow
  // the two stages: thread tid's is row tid & 127 of operand tid >> 7
  u32* const slds = (u32*)(gcx_lds + 2u * T::STAGE_UNITS);
  // fragments: row rl of each 32-row block, half h of an issue's 64 elements
  const u32 rl = lane & 31u, h = lane >> 5;
  const u32 arow = 64u * wr, brow = 64u * wc;
  const u32 asc = arow + rl, bsc = 128u + brow + rl;  // + 32 x
  const size_t pa = (size_t)g.slabs * A::ROW_UNITS, pb = (size_t)g.slabs * B::ROW_UNITS;
  const u32 tiles = g.tm * g.tn;

  for (u32 t = blockIdx.x; t < g.steps; t += gridDim.x) {
    w.round = t / tiles;
    w.first_of_round = t < gridDim.x || (t - gridDim.x) / tiles != w.round;
    gc_tile(t - w.round * tiles, g.tm, g.tn, w.bi, w.bj);
    const u32x4* ga = g.a + (size_t)w.bi * GC_TILE * pa;
    const u32x4* gb = g.bt + (size_t)w.bj * GC_TILE * pb;
    const u32* gs = tid < 128u
        ? (const u32*)m.sa + ((size_t)w.bi * GC_TILE + tid) * g.slabs
        : (const u32*)m.sb + ((size_t)w.bj * GC_TILE + (tid - 128u)) * g.slabs;

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[x][y][e] = 0.f;

    u32x4 ra[A::LOADS], rb[B::LOADS];
    u32 rs = gs[0];
    A::load(ga, pa, tid, ra);
    B::load(gb, pb, tid, rb);
    A::store(gcx_lds, tid, ra);
    B::store(gcx_lds + A::LDS_UNITS, tid, rb);
    slds[tid] = rs;
    __syncthreads();

    for (u32 s = 0; s < g.slabs; ++s) {
      const u32 cur = (s & 1u) * T::STAGE_UNITS, scur = (s & 1u) * GCX_SCALE_ROWS;
      const bool more = s + 1u < g.slabs;
      if (more) {  // in flight while this slab's MFMAs run
        rs = gs[s + 1u];
        A::load(ga + (size_t)(s + 1u) * A::ROW_UNITS, pa, tid, ra);
        B::load(gb + (size_t)(s + 1u) * B::ROW_UNITS, pb, tid, rb);
      }
      // this lane's rows' scale words, its half's byte lowest: block 2 kk + h
      // is then byte 2 kk
      u32 sa[2], sb[2];
#pragma unroll
      for (u32 x = 0; x < 2u; ++x) {
        sa[x] = slds[scur + asc + 32u * x] >> (8u * h);
        sb[x] = slds[scur + bsc + 32u * x] >> (8u * h);
      }
      const u32x4* la = gcx_lds + cur;
      const u32x4* lb = la + A::LDS_UNITS;
      gcx_issue<T, 0>(la, lb, arow, brow, rl, h, sa, sb, acc);
      gcx_issue<T, 2>(la, lb, arow, brow, rl, h, sa, sb, acc);
      if (more) {
        u32x4* nxt = gcx_lds + (cur ^ T::STAGE_UNITS);
        A::store(nxt, tid, ra);
        B::store(nxt + A::LDS_UNITS, tid, rb);
        slds[(scur ^ GCX_SCALE_ROWS) + tid] = rs;
      }
      // slab s+1 is written, and nobody still reads slab s, which the
      // next iteration (or the next tile's first slab) overwrites
      __syncthreads();
    }

    // as in gemmcheck_mx.hip: the lane number through an identity DPP move,
    // so that the sink's 64 salts or store offsets are made per tile and not
    // kept in VGPRs across the whole walk
    const u32 el = (u32)__builtin_amdgcn_mov_dpp((int)lane, 0xE4, 0xF, 0xF, false);
    const u32 erl = el & 31u, eh = el >> 5;
    SINK sink(g, w.bi, w.bj);
#pragma unroll
    for (u32 x = 0; x < 2u; ++x)
#pragma unroll
      for (u32 y = 0; y < 2u; ++y)
#pragma unroll
        for (u32 e = 0; e < 16u; ++e)
          sink.put(64u * wr + 32u * x + (e & 3u) + 8u * (e >> 2) + 4u * eh,
                   64u * wc + 32u * y + erl, gcm_f32_bits(acc[x][y][e]));
    sink.finish(a, g, T::STAGE, w);
  }
#endif
}

// ---------------------------------------------------------------- host

// One operand and its scales; fills rows and K.
template <typename OP>
static void gcx_check_operand(const char* name, const at::Tensor& x, const at::Tensor& scale,
                              const at::Tensor& a, int64_t& rows, int64_t& k) {
  const char* type = OP::type_name();
  TORCH_CHECK(x.is_cuda() && scale.is_cuda() && x.get_device() == a.get_device() &&
                  scale.get_device() == a.get_device(),
              "gemmcheck: a, bt and their scales must be on the same GPU");
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous(),
              "gemmcheck: a [M, K] and bt [N, K] must be contiguous matrices");
  TORCH_CHECK(x.scalar_type() == at::kByte || (int64_t)x.scalar_type() == OP::TYPE,
              "gemmcheck: ", name, " must be uint8", type ? " or " : "", type ? type : "");
  const int64_t row_bytes = 16 * OP::ROW_UNITS, width = x.size(1);
  rows = x.size(0);
  if (k < 0) {  // a says what K is
    TORCH_CHECK(width >= row_bytes && width % row_bytes == 0,
                "gemmcheck: K must be a positive multiple of ", GCX_SLAB, " elements (", row_bytes,
                " bytes of a), got ", width, " bytes");
    k = width / row_bytes * GCX_SLAB;
  }
  TORCH_CHECK(width == k / GCX_SLAB * row_bytes, "gemmcheck: a is [M, ", a.size(1),
              "] (K = ", k, ") but ", name, " is [", rows, ", ", width, "], not [", rows, ", ",
              k / GCX_SLAB * row_bytes, "]");
  TORCH_CHECK(rows >= GC_TILE && rows % GC_TILE == 0,
              "gemmcheck: M and N must be positive multiples of ", GC_TILE, ", got ", rows,
              " rows of ", name);
  TORCH_CHECK(scale.scalar_type() == at::kByte && scale.dim() == 2 && scale.is_contiguous() &&
                  scale.size(0) == rows && scale.size(1) == k / 32,
              "gemmcheck: ", name, "_scale must be a contiguous uint8 [", rows, ", ", k / 32,
              "] tensor (one E8M0 byte per row and 32 elements of K)");
  TORCH_CHECK((uintptr_t)scale.data_ptr() % sizeof(u32) == 0,
              "gemmcheck: scales must be aligned to ", sizeof(u32), " bytes");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0,
              "gemmcheck: a and bt must be aligned to 16 bytes");
}

// Operand checks shared by gemm_mx_nt and gemmcheck_mx_run; fills the shape.
template <typename T>
static GcmArgs gcx_check_operands(const at::Tensor& a, const at::Tensor& a_scale,
                                  const at::Tensor& bt, const at::Tensor& bt_scale) {
  int64_t m = 0, n = 0, k = -1;
  gcx_check_operand<typename T::A>("a", a, a_scale, a, m, k);
  gcx_check_operand<typename T::B>("bt", bt, bt_scale, a, n, k);
  TORCH_CHECK(k <= T::MAX_K, "gemmcheck: this format needs K <= ", T::MAX_K, ", got ", k);
  TORCH_CHECK((m / GC_TILE) * (n / GC_TILE) <= GC_MAX_STEPS, "gemmcheck: too many tiles");
  GcmArgs args;
  GcArgs& g = args.g;
  g.a = (const u32x4*)a.data_ptr();
  g.bt = (const u32x4*)bt.data_ptr();
  g.out = nullptr;
  g.tm = (u32)(m / GC_TILE);
  g.tn = (u32)(n / GC_TILE);
  g.slabs = (u32)(k / GCX_SLAB);
  g.steps = g.tm * g.tn;
  args.sa = a_scale.data_ptr();
  args.sb = bt_scale.data_ptr();
  return args;
}

template <typename T, typename SINK>
static void gcx_launch(int64_t blocks, const CuArgs& ca, const GcmArgs& m) {
  auto kernel = gemmcheck_mx6_kernel<T, SINK>;
  C10_HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)T::LDS_BYTES));
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GC_THREADS), T::LDS_BYTES,
                     at::hip::getCurrentHIPStream(), ca, m);
}

#define GCX_FORMAT(name, T) \
  {name, T::STAGE, gcx_check_operands<T>, gcx_launch<T, GcStore>, gcx_launch<T, GcFold>}

const GcxFormat* gcx_format(const std::string& format) {
  static const GcxFormat formats[] = {
      GCX_FORMAT("mxfp8_e5m2", GcxStage4),  GCX_FORMAT("mxfp6_e2m3", GcxStage5),
      GCX_FORMAT("mxfp6_e3m2", GcxStage6),  GCX_FORMAT("mxfp8_e5m2:mxfp8", GcxStage7),
  };
  for (const GcxFormat& f : formats)
    if (format == f.name) return &f;
  return nullptr;
}
