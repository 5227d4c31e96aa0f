// gemmcheck_mx — the block-scaled (OCP MX) stages of the full-chip tiled-
// GEMM load probe (gfx950), compiled into _gpuprobe next to gemmcheck.hip.
//
//   C[M,N] (f32) = sum over k of A[i][k] 2^(SA[i][k/32] - 127)
//                              . Bt[j][k] 2^(SB[j][k/32] - 127)
// both operands K-contiguous (NT), one E8M0 scale byte per row and per 32
// elements of K, in two instantiations of one template, both on
// v_mfma_scale_f32_32x32x64_f8f6f4 with f32 accumulators:
//   stage 2  mxfp8  e4m3 elements, one byte each          (cbsz = blgp = 0)
//   stage 3  mxfp4  e2m1 elements, two per byte, the low  (cbsz = blgp = 4)
//                   nibble first
// mxcheck and matcheck prove that one such instruction computes right from
// registers with nothing else busy; here it runs the way a tenant's job
// runs it, with HBM, L2, LDS and the scale path busy on every CU at once.
// probe/gemmcheck.py holds the numpy definition of operands, scales and
// expected folds; every block of a dot product carries the same product
// scale, so every partial sum in any order is exact and the compare is bit
// for bit.
//
// What is gemmcheck.hip's (gemmcheck_common.h, and that file's header
// comment): 256 threads, four waves 2x2 on a 128x128 tile, 2x2 accumulators
// of 32x32 per wave, slabs of 128 bytes per row in two LDS stages, the
// global -> register -> LDS staging with one barrier per slab, the XOR
// swizzle, the walk over rounds x tiles, the XCD super-block tile order and
// the GcStore / GcFold sinks.  What is new:
//
// Fragments.  The instruction takes 64 elements of K per issue; lane l
// holds row l&31 and the 32 elements of half h = l>>5, which are exactly
// one scale block.
//   mxfp8: a slab is 128 elements, KSTEPS = 2 issues.  The lane's fragment
//     is 32 contiguous bytes at byte 64 kk + 32 h of the row: the two
//     16-byte columns 4 kk + 2 h and 4 kk + 2 h + 1, each XORed with the
//     row swizzle, two ds_read_b128 into the eight operand VGPRs.
//   mxfp4: a slab is 256 elements, KSTEPS = 4 issues.  The fragment is 16
//     bytes at byte 32 kk + 16 h, column 2 kk + h: where the bf16 / i8
//     fragment sits.  The upper four operand VGPRs are not read for e2m1
//     and the compiler picks the four-register form of the instruction.
//   In both, column(kk, f) = (FRAG (2 kk + h) + f) ^ ((row >> 1) & 7) with
//   FRAG = 2 or 1 columns per fragment.
//
// Bank conflicts.  The address map is the sibling's, unit(stage, op, row,
// c) = 2048 stage + 1024 op + 8 row + (c ^ ((row>>1) & 7)) in 16-byte
// units, and its argument carries over unchanged: a b128 access is served
// sixteen lanes at a time, the 256-byte bank line holds sixteen units, and
// a unit's place in the line is 8 (row & 1) + (c ^ ((row>>1) & 7)).  Every
// fragment read above is one column c by sixteen consecutive rows (lanes
// 16 g .. 16 g + 15 share h, and c depends on kk, h and f only), so the
// sixteen (row parity, (row>>1) & 7) pairs put it on sixteen different
// places whatever c is: the mxfp8 pair of reads is two such reads, the
// mxfp4 read is the sibling's own.  The staging writes are the sibling's,
// byte for byte.  The map therefore stays.
//
// Scales.  Per slab a row owns KSTEPS x 2 scale bytes: one aligned 32-bit
// word for mxfp8 (4 blocks), one aligned 64-bit word for mxfp4 (8 blocks);
// K is a multiple of the slab, so word s of a row is slab s.  They travel
// with the slab: thread t loads the word of row t & 127 of operand t >> 7
// with the slab's data loads and stores it after the MFMAs to the scale
// area of the other stage, word 256 stage + t behind the 64 KiB of data
// (consecutive threads, consecutive words: conflict-free, as are the reads:
// 32 consecutive rows, both halves the same word).  That is 2 KiB (mxfp8)
// or 4 KiB (mxfp4) more: 66 / 68 KiB per workgroup, two of which fit the
// CU's 160 KiB.  Once per slab a lane reads the words of its two A rows and
// two Bt rows and shifts them right by 8 h; the scale byte of issue kk,
// byte 2 kk + h of the word, is then byte 2 (kk & 1) of 32-bit half kk >> 1:
// op_sel, an immediate, is 0 for even and 2 for odd kk, the way matcheck's
// mt_scaled selects it.  Bytes 1 and 3 of the register hold the other
// half's scales and act as that probe's decoys do.
//
// Resources (gfx950, cross-compiled, -O3).  VGPRs, the 64 accumulator
// registers among them, no AGPRs: 225 (mxfp8) and 230 (mxfp4) with GcFold,
// 218 and 224 with GcStore; no scratch; 66 / 68 KiB of dynamic LDS; two
// workgroups = 2 waves per SIMD per CU, which __launch_bounds__(256, 2)
// asks for.  Left alone the compiler keeps the sink's 64 salts or store
// offsets in registers across the whole tile walk and needs 280 to 292
// (one workgroup per CU), or spills them; the epilogue's DPP move below is
// what prevents that.
//
// Measured on MI355X at 8192^3 on the default grid, windows of 2.0 to 2.1 s
// alternating with the bf16 stage (profiles/gemmcheck_mx_mi355x.json):
// mxfp8 1229 TFLOP/s (0.895 ms per round), mxfp4 2598 TFLOP/s (0.423 ms),
// bf16 519 TFLOP/s (2.12 ms) in the same session; every fold equal to the
// numpy reference.  Clocks and power: not measured.
//
// No inline assembly, builtins and plain C++ only.

#include "gemmcheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#include <string>

typedef int gcm_i32x8 __attribute__((ext_vector_type(8)));

#define GCM_MAX_K_FP8 32768  // 16 . 16 . K <= 2**23 in units of the product scale
#define GCM_MAX_K_FP4 65536  // products <= 144 quarters: 144 K < 2**24

struct GcmFp8 {
  typedef u32 Scale;  // a row's scale bytes of one slab
  static constexpr int FMT = 0;  // e4m3
  static constexpr u32 STAGE = 2, KSTEPS = 2, FRAG = 2;
  static constexpr int64_t ELEMS_PER_BYTE = 1, MAX_K = GCM_MAX_K_FP8;
};

struct GcmFp4 {
  typedef unsigned long long Scale;
  static constexpr int FMT = 4;  // e2m1
  static constexpr u32 STAGE = 3, KSTEPS = 4, FRAG = 1;
  static constexpr int64_t ELEMS_PER_BYTE = 2, MAX_K = GCM_MAX_K_FP4;
};

// GcmArgs (gemmcheck_common.h): the scales in Scale words.

#define GCM_SCALE_ROWS 256u  // A and Bt rows of one stage
template <typename T>
constexpr size_t gcm_lds_bytes() {
  return GC_LDS_BYTES + 2 * GCM_SCALE_ROWS * sizeof(typename T::Scale);
}

#if __HIP_DEVICE_COMPILE__
extern __shared__ u32x4 gcm_lds[];

// Issue kk of a slab: the fragments of two A and two Bt row blocks and the
// four MFMAs.  SEL = 2 (kk & 1) is the byte of sa / sb that scales them.
template <typename T, int SEL>
__device__ __forceinline__ void gcm_issue(u32 aunit, u32 bunit, u32 c0, const u32 (&sa)[2],
                                          const u32 (&sb)[2], f32x16 (&acc)[2][2]) {
  gcm_i32x8 fa[2], fb[2];
#pragma unroll
  for (u32 x = 0; x < 2u; ++x) {
    fa[x] = gcm_i32x8{0, 0, 0, 0, 0, 0, 0, 0};
    fb[x] = gcm_i32x8{0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (u32 f = 0; f < T::FRAG; ++f) {
      // c0 is even for FRAG = 2, so c0 ^ f is the swizzled column + f
      const u32x4 va = gcm_lds[aunit + 256u * x + (c0 ^ f)];
      const u32x4 vb = gcm_lds[bunit + 256u * x + (c0 ^ f)];
#pragma unroll
      for (u32 e = 0; e < 4u; ++e) {
        fa[x][4 * f + e] = (int)va[e];
        fb[x][4 * f + e] = (int)vb[e];
      }
    }
  }
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
      acc[x][y] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
          fa[x], fb[y], acc[x][y], T::FMT, T::FMT, SEL, (int)sa[x], SEL, (int)sb[y]);
}
#endif

template <typename T, typename SINK>
__global__ void __launch_bounds__(GC_THREADS, 2) gemmcheck_mx_kernel(CuArgs a, GcmArgs m) {
#if __HIP_DEVICE_COMPILE__
  typedef typename T::Scale Scale;
  const GcArgs& g = m.g;
  const u32 tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
  GcWhere w;
  w.lane = (int)lane;
  w.gwave = blockIdx.x * GC_WAVES + wv;
  w.hw = cu_locate_wave(a.res, (int)lane);
  w.quadrant = wv;
  const u32 wr = wv >> 1, wc = wv & 1u;

  // staging: chunk sc of rows sr + 32 i of both operands, and the scale
  // word of row tid & 127 of operand tid >> 7
  const u32 sc = tid & 7u, sr = tid >> 3;
  const u32 wunit = GC_ROW_UNITS * sr + (sc ^ ((sr >> 1) & 7u));  // + 256 i
  Scale* const slds = (Scale*)(gcm_lds + 2u * GC_STAGE_UNITS);    // [stage][256]
  // fragments: row rl of each 32-row block, half h of an issue's 64 elements
  const u32 rl = lane & 31u, h = lane >> 5, rswz = (rl >> 1) & 7u;
  const u32 aunit = GC_ROW_UNITS * (64u * wr + rl);
  const u32 bunit = GC_OP_UNITS + GC_ROW_UNITS * (64u * wc + rl);
  const u32 asc = 64u * wr + rl, bsc = 128u + 64u * wc + rl;  // + 32 x
  const size_t pitch = (size_t)g.slabs * GC_ROW_UNITS;
  const u32 tiles = g.tm * g.tn;

  for (u32 t = blockIdx.x; t < g.steps; t += gridDim.x) {
    w.round = t / tiles;
    w.first_of_round = t < gridDim.x || (t - gridDim.x) / tiles != w.round;
    gc_tile(t - w.round * tiles, g.tm, g.tn, w.bi, w.bj);
    const u32x4* ga = g.a + ((size_t)w.bi * GC_TILE + sr) * pitch + sc;
    const u32x4* gb = g.bt + ((size_t)w.bj * GC_TILE + sr) * pitch + sc;
    const Scale* gs = tid < 128u
        ? (const Scale*)m.sa + ((size_t)w.bi * GC_TILE + tid) * g.slabs
        : (const Scale*)m.sb + ((size_t)w.bj * GC_TILE + (tid - 128u)) * g.slabs;

    f32x16 acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[x][y][e] = 0.f;

    u32x4 ra[4], rb[4];
    Scale rs = gs[0];
#pragma unroll
    for (u32 i = 0; i < 4u; ++i) {
      ra[i] = ga[32u * i * pitch];
      rb[i] = gb[32u * i * pitch];
    }
#pragma unroll
    for (u32 i = 0; i < 4u; ++i) {
      gcm_lds[wunit + 256u * i] = ra[i];
      gcm_lds[GC_OP_UNITS + wunit + 256u * i] = rb[i];
    }
    slds[tid] = rs;
    __syncthreads();

    for (u32 s = 0; s < g.slabs; ++s) {
      const u32 cur = (s & 1u) * GC_STAGE_UNITS, scur = (s & 1u) * GCM_SCALE_ROWS;
      const bool more = s + 1u < g.slabs;
      if (more) {  // in flight while this slab's MFMAs run
        rs = gs[s + 1u];
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
          ra[i] = ga[32u * i * pitch + (size_t)(s + 1u) * GC_ROW_UNITS];
          rb[i] = gb[32u * i * pitch + (size_t)(s + 1u) * GC_ROW_UNITS];
        }
      }
      // this lane's rows' scale words, its half's byte lowest
      Scale wa[2], wb[2];
#pragma unroll
      for (u32 x = 0; x < 2u; ++x) {
        wa[x] = slds[scur + asc + 32u * x] >> (8u * h);
        wb[x] = slds[scur + bsc + 32u * x] >> (8u * h);
      }
#pragma unroll
      for (u32 kp = 0; kp < T::KSTEPS / 2u; ++kp) {
        const u32 sa[2] = {(u32)(wa[0] >> (32u * kp)), (u32)(wa[1] >> (32u * kp))};
        const u32 sb[2] = {(u32)(wb[0] >> (32u * kp)), (u32)(wb[1] >> (32u * kp))};
        gcm_issue<T, 0>(cur + aunit, cur + bunit, (T::FRAG * (4u * kp + h)) ^ rswz, sa, sb, acc);
        gcm_issue<T, 2>(cur + aunit, cur + bunit, (T::FRAG * (4u * kp + 2u + h)) ^ rswz, sa, sb,
                        acc);
      }
      if (more) {
        const u32 nxt = cur ^ GC_STAGE_UNITS;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
          gcm_lds[nxt + wunit + 256u * i] = ra[i];
          gcm_lds[nxt + GC_OP_UNITS + wunit + 256u * i] = rb[i];
        }
        slds[(scur ^ GCM_SCALE_ROWS) + tid] = rs;
      }
      // slab s+1 is written, and nobody still reads slab s, which the
      // next iteration (or the next tile's first slab) overwrites
      __syncthreads();
    }

    // C/D map of the 32x32 MFMAs: cu_tile_index.  The lane number comes
    // through an identity DPP move here: a cross-lane operation is never
    // moved out of a loop, so the 64 salts or store offsets of the sink are
    // made per tile and not kept in up to 128 VGPRs across the whole walk,
    // which would cost the second workgroup per CU.
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

// The formats of gemmcheck_mx6.hip are looked up before this is asked.
static bool gcm_is_fp4(const std::string& format) {
  TORCH_CHECK(format == "mxfp8" || format == "mxfp4",
              "gemmcheck: format must be 'mxfp8', 'mxfp4', 'mxfp8_e5m2', 'mxfp6_e2m3', "
              "'mxfp6_e3m2' or 'mxfp8_e5m2:mxfp8', got '", format, "'");
  return format == "mxfp4";
}

// Operand checks shared by gemm_mx_nt and gemmcheck_mx_run; fills the shape.
template <typename T>
static GcmArgs gcm_check_operands(const at::Tensor& a, const at::Tensor& a_scale,
                                  const at::Tensor& bt, const at::Tensor& bt_scale) {
  const bool fp8 = T::ELEMS_PER_BYTE == 1;
  TORCH_CHECK(a.is_cuda() && bt.is_cuda() && a_scale.is_cuda() && bt_scale.is_cuda() &&
                  a.get_device() == bt.get_device() && a.get_device() == a_scale.get_device() &&
                  a.get_device() == bt_scale.get_device(),
              "gemmcheck: a, bt and their scales must be on the same GPU");
  TORCH_CHECK(a.dim() == 2 && bt.dim() == 2 && a.is_contiguous() && bt.is_contiguous(),
              "gemmcheck: a [M, K] and bt [N, K] must be contiguous matrices");
  TORCH_CHECK(a.scalar_type() == bt.scalar_type() &&
                  (a.scalar_type() == at::kByte ||
                   (fp8 && a.scalar_type() == at::kFloat8_e4m3fn)),
              "gemmcheck: a and bt must both be uint8",
              fp8 ? " or both float8_e4m3fn" : " (two e2m1 codes per byte)");
  const int64_t m = a.size(0), n = bt.size(0), k = a.size(1) * T::ELEMS_PER_BYTE;
  const int64_t slab = GC_SLAB_BYTES * T::ELEMS_PER_BYTE;
  TORCH_CHECK(bt.size(1) == a.size(1), "gemmcheck: a is [M, ", a.size(1), "] but bt is [N, ",
              bt.size(1), "]");
  TORCH_CHECK(m >= GC_TILE && n >= GC_TILE && m % GC_TILE == 0 && n % GC_TILE == 0,
              "gemmcheck: M and N must be positive multiples of ", GC_TILE, ", got ", m, " and ", n);
  TORCH_CHECK(k >= slab && k % slab == 0, "gemmcheck: K must be a positive multiple of ", slab,
              " elements, got ", k);
  TORCH_CHECK(k <= T::MAX_K, "gemmcheck: ", fp8 ? "mxfp8" : "mxfp4", " needs K <= ", T::MAX_K,
              ", got ", k);
  TORCH_CHECK((m / GC_TILE) * (n / GC_TILE) <= GC_MAX_STEPS, "gemmcheck: too many tiles");
  const at::Tensor* scales[2] = {&a_scale, &bt_scale};
  const int64_t rows[2] = {m, n};
  for (int i = 0; i < 2; ++i) {
    const at::Tensor& s = *scales[i];
    TORCH_CHECK(s.scalar_type() == at::kByte && s.dim() == 2 && s.is_contiguous() &&
                    s.size(0) == rows[i] && s.size(1) == k / 32,
                "gemmcheck: ", i ? "bt_scale" : "a_scale", " must be a contiguous uint8 [",
                rows[i], ", ", k / 32, "] tensor (one E8M0 byte per row and 32 elements of K)");
    TORCH_CHECK((uintptr_t)s.data_ptr() % sizeof(typename T::Scale) == 0,
                "gemmcheck: scales must be aligned to ", sizeof(typename T::Scale), " bytes");
  }
  TORCH_CHECK((uintptr_t)a.data_ptr() % 16 == 0 && (uintptr_t)bt.data_ptr() % 16 == 0,
              "gemmcheck: a and bt must be aligned to 16 bytes");
  GcmArgs args;
  GcArgs& g = args.g;
  g.a = (const u32x4*)a.data_ptr();
  g.bt = (const u32x4*)bt.data_ptr();
  g.out = nullptr;
  g.tm = (u32)(m / GC_TILE);
  g.tn = (u32)(n / GC_TILE);
  g.slabs = (u32)(k / slab);
  g.steps = g.tm * g.tn;
  args.sa = a_scale.data_ptr();
  args.sb = bt_scale.data_ptr();
  return args;
}

template <typename T, typename SINK>
static void gcm_launch(int64_t blocks, const CuArgs& ca, const GcmArgs& m) {
  auto kernel = gemmcheck_mx_kernel<T, SINK>;
  C10_HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)gcm_lds_bytes<T>()));
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GC_THREADS), gcm_lds_bytes<T>(),
                     at::hip::getCurrentHIPStream(), ca, m);
}

at::Tensor gcm_gemm(GcmArgs m, GcmLaunch store, const at::Tensor& a, int64_t blocks_arg) {
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(a));
  const int64_t blocks = gc_grid(blocks_arg, m.g.steps);
  at::Tensor out = at::empty({(int64_t)m.g.tm * GC_TILE, (int64_t)m.g.tn * GC_TILE},
                             a.options().dtype(at::kFloat));
  at::Tensor res = gc_result_block(out, 0);  // only the per-CU wave table is used
  m.g.out = (u32*)out.data_ptr();
  const CuArgs ca = {0, 1, nullptr, (u32*)res.data_ptr(), 0, nullptr, NO_INJECT, 0, 0, 0};
  store(blocks, ca, m);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// C (float32) = dequantised a . dequantised bt^T on the GPU of the
// operands.  Exact whenever every partial sum is representable in f32.
at::Tensor gemm_mx_nt(at::Tensor a, at::Tensor a_scale, at::Tensor bt, at::Tensor bt_scale,
                      std::string format, int64_t blocks_arg) {
  if (const GcxFormat* x = gcx_format(format))
    return gcm_gemm(x->check(a, a_scale, bt, bt_scale), x->store, a, blocks_arg);
  return gcm_is_fp4(format)
             ? gcm_gemm(gcm_check_operands<GcmFp4>(a, a_scale, bt, bt_scale),
                        gcm_launch<GcmFp4, GcStore>, a, blocks_arg)
             : gcm_gemm(gcm_check_operands<GcmFp8>(a, a_scale, bt, bt_scale),
                        gcm_launch<GcmFp8, GcStore>, a, blocks_arg);
}

CucheckOut gcm_run(GcmArgs m, u32 stage, GcmLaunch fold, const at::Tensor& a,
                   const at::Tensor& expected, int64_t rounds, int64_t blocks_arg,
                   int64_t max_records, const c10::optional<CuInject>& inject) {
  TORCH_CHECK(rounds >= 1 && rounds <= MAX_ROUNDS, "gemmcheck: rounds must be in 1..",
              MAX_ROUNDS, ", got ", rounds);
  TORCH_CHECK(rounds * (int64_t)m.g.steps <= GC_MAX_STEPS,
              "gemmcheck: rounds x tiles must be <= ", GC_MAX_STEPS);
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT,
              "gemmcheck: max_records must be in 0..", MAX_RECORDS_LIMIT);
  TORCH_CHECK(expected.is_cuda() && expected.get_device() == a.get_device() &&
                  expected.scalar_type() == at::kInt && expected.is_contiguous() &&
                  expected.numel() == 16,
              "gemmcheck: expected must be a contiguous int32 [4, 4] tensor on the operands' GPU");
  m.g.steps = (u32)(rounds * (int64_t)m.g.steps);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(a));
  const int64_t blocks = gc_grid(blocks_arg, m.g.steps);
  at::Tensor res = gc_result_block(expected, max_records);
  CuArgs ca = {0, (u32)rounds, (const u32*)expected.data_ptr(), (u32*)res.data_ptr(),
               (int)max_records, nullptr, NO_INJECT, 0, 0, 0};
  if (inject.has_value()) {
    int64_t w = std::get<0>(*inject), r = std::get<1>(*inject);
    int64_t s = std::get<2>(*inject), mask = std::get<3>(*inject);
    TORCH_CHECK(w >= 0 && w < blocks * GC_WAVES && r >= 0 && r < rounds && s == (int64_t)stage &&
                    mask >= 0 && mask <= 0xFFFFFFFFLL,
                "gemmcheck: inject (wave, round, stage, mask) out of range");
    ca.inj_wave = (u32)w;
    ca.inj_round = (u32)r;
    ca.inj_stage = (u32)s;
    ca.inj_mask = (u32)mask;
  }

  auto stream = at::hip::getCurrentHIPStream();
  hipEvent_t t0, t1;
  C10_HIP_CHECK(hipEventCreate(&t0));
  C10_HIP_CHECK(hipEventCreate(&t1));
  C10_HIP_CHECK(hipEventRecord(t0, stream));
  fold(blocks, ca, m);
  hipError_t launch_err = hipGetLastError();
  (void)hipEventRecord(t1, stream);
  hipError_t sync_err = hipEventSynchronize(t1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  C10_HIP_CHECK(launch_err);
  C10_HIP_CHECK(sync_err);
  return cu_read_result(res, max_records, (double)ms / 1e3);
}

// gemmcheck_run for the MX stages: `rounds` GEMMs in one launch, every
// wave's fold compared with expected[class][quadrant]; nothing of C is
// stored.  inject = (wave of the grid, round, the format's stage 2..7, mask).
CucheckOut gemmcheck_mx_run(at::Tensor a, at::Tensor a_scale, at::Tensor bt, at::Tensor bt_scale,
                            std::string format, at::Tensor expected, int64_t rounds,
                            int64_t blocks_arg, int64_t max_records,
                            c10::optional<CuInject> inject) {
  if (const GcxFormat* x = gcx_format(format))
    return gcm_run(x->check(a, a_scale, bt, bt_scale), x->stage, x->fold, a, expected, rounds,
                   blocks_arg, max_records, inject);
  return gcm_is_fp4(format)
             ? gcm_run(gcm_check_operands<GcmFp4>(a, a_scale, bt, bt_scale), GcmFp4::STAGE,
                       gcm_launch<GcmFp4, GcFold>, a, expected, rounds, blocks_arg, max_records,
                       inject)
             : gcm_run(gcm_check_operands<GcmFp8>(a, a_scale, bt, bt_scale), GcmFp8::STAGE,
                       gcm_launch<GcmFp8, GcFold>, a, expected, rounds, blocks_arg, max_records,
                       inject);
}

// Called from gpuprobe.hip's PYBIND11_MODULE, GIL released like gemmcheck's.
void bind_gemmcheck_mx(py::module_& m) {
  m.def("gemm_mx_nt", &gemm_mx_nt,
        "C (float32) = a 2^(a_scale - 127) . (bt 2^(bt_scale - 127))^T, format 'mxfp8' (e4m3), "
        "'mxfp4' (packed e2m1), 'mxfp8_e5m2', 'mxfp6_e2m3', 'mxfp6_e3m2' (packed, 24 bytes per "
        "32 elements) or 'mxfp8_e5m2:mxfp8' (a's format : bt's), one E8M0 scale per "
        "row and 32 elements of K",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("a"), py::arg("a_scale"), py::arg("bt"), py::arg("bt_scale"), py::arg("format"),
        py::arg("blocks") = 0);
  m.def("gemmcheck_mx_run", &gemmcheck_mx_run,
        "block-scaled tiled-GEMM load run -> (mismatches, first_bad_round, stage_mask, records, "
        "waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("a"), py::arg("a_scale"), py::arg("bt"), py::arg("bt_scale"), py::arg("format"),
        py::arg("expected"), py::arg("rounds"), py::arg("blocks") = 0,
        py::arg("max_records") = 16, py::arg("inject") = py::none());
}
