// gemmcheck — full-chip tiled-GEMM load probe (gfx950), compiled into
// _gpuprobe.
//
// The sibling probes isolate one unit each with a short workload made in
// registers.  This one runs the job the GPU is scheduled for: a real GEMM
// with HBM, L2, LDS and the matrix cores busy at once on every CU,
//   C[M,N] = A[M,K] . Bt[N,K]^T        (NT: both operands K-contiguous)
// in two instantiations of one template:
//   stage 0  bf16  v_mfma_f32_32x32x16_bf16, f32 accumulators
//   stage 1  i8    v_mfma_i32_32x32x32_i8,   i32 accumulators
// In both a lane's fragment is 16 contiguous bytes of one row (row l&31,
// bytes 16 (l>>5) .. of the instruction's 32-byte k range), so staging and
// fragment reads are written in bytes and shared.
// probe/gemmcheck.py holds the numpy definition of the operands and of the
// expected folds; its operands are small integers, so every partial sum in
// any order is exact and the compare is bit for bit.
//
// Work split.  A workgroup of 256 threads (4 waves) owns a 128x128 tile of
// C; the waves sit 2x2 (wave w: rows 64 (w>>1).., columns 64 (w&1)..) and
// each owns 64x64 as 2x2 accumulators of 32x32: 64 accumulator registers.
// K goes by in slabs of 128 bytes per row (64 bf16, 128 i8): 16 KiB of A
// and 16 KiB of Bt, two stages = 64 KiB of LDS, two workgroups per CU.
// A slab is four k-steps; a k-step reads two A and two Bt fragments (four
// ds_read_b128) and issues four MFMAs.
//
// Data movement.  Global -> registers -> LDS in 16-byte chunks: thread t
// moves chunk t&7 of rows (t>>3) + 32 i, i = 0..3, of either operand, so
// eight neighbouring threads read one row's 128 contiguous bytes.  The
// loads of slab s+1 are issued before the MFMAs of slab s and stored to
// the other stage after them; one barrier per slab then covers both "slab
// s+1 is written" and "slab s is no longer read".  The barrier is
// __syncthreads(): its wait on outstanding loads costs nothing here, since
// the loads were consumed by the LDS stores just before it; the waits
// inside a slab are the compiler's own counters.
//
// LDS address map, in 16-byte units (gc_lds[] is u32x4):
//   unit(stage, op, row, c) = 2048 stage + 1024 op + 8 row + (c ^ ((row>>1) & 7))
// op 0 = A, 1 = Bt; row 0..127; c = 16-byte column 0..7 of the slab.
// Rows are 128 B apart, so unswizzled the 32 lanes that read one k-column
// would fall on two groups of four banks.  With the XOR, sixteen
// consecutive rows cover all sixteen (row parity, column) positions of the
// 256-byte bank line: a b128 read of one column by consecutive rows and
// the staging writes (eight chunks of a row, then the next row) are both
// conflict-free.  (row>>1)&7 does not change under row += 16, so it is
// hoisted out of every loop.
//
// One launch, many GEMMs.  A workgroup walks t = blockIdx.x; t < rounds
// tiles; t += gridDim.x, round = t / tiles the slow index: a multi-round
// run stays under load with no host gap, and a small grid exercises the
// walk.
//
// Tile order.  Workgroups are dealt round-robin over the 8 XCDs, each with
// its own L2, so with a grid that is a multiple of 8 step u = t % tiles
// lands on XCD u & 7, and the default grid (two workgroups per CU) keeps
// 64 consecutive steps of one XCD resident together.  gc_tile therefore
// makes v = u >> 3, the XCD's own sequence, run through 8x8 super-blocks of
// tiles: super-block 8 (v >> 6) + (u & 7), tile ((v >> 3) & 7, v & 7) in
// it.  The 64 tiles resident on an XCD then share 8 row-panels of A and 8
// column-panels of Bt (16 panel reads for 64 tiles instead of up to 128),
// and different XCDs work on different super-blocks.  This needs the tile
// grid to be a multiple of 8 both ways and the super-block count a
// multiple of 8; any other shape walks row-major.  Placement is not
// assumed anywhere: cu_locate_wave reads HW_ID / XCC_ID.
//
// Sinks.  The tile code is a template over where C goes: GcStore writes
// it to `out` (gemm_nt, the tests), GcFold stores nothing: each wave folds
// its 64x64 quadrant into sum fmix32(bits(c) + salt(128 i + j)), i, j
// tile-local, bits = the i32 or the f32 bit pattern with any zero as +0,
// and lane 0 compares with expected[class][quadrant], class = 2 (bi & 1) +
// (bj & 1): the content has period 256 rows, so a workgroup that reads the
// neighbouring row block folds to another value.  A mismatch goes to
// cucheck's result block: word 0 = 4 (bi tn + bj) + quadrant, stage 0 / 1.
// The inject hook XORs a mask into the fold of one wave of the grid at the
// first tile its workgroup computes in one round.
//
// Resources (gfx950): 158 VGPRs + 64 AGPRs, no scratch, 64 KiB LDS, two
// workgroups = 2 waves per SIMD per CU, as designed.  Measured on MI355X at
// 8192^3 (profiles/gemmcheck_mi355x.json): 530 TFLOP/s bf16, 1252 TOP/s i8
// sustained, 29 % of torch.matmul's bf16 rate.  With 2x2 accumulators each
// MFMA costs one 1 KiB LDS read, the LDS's whole 128 B/clk per CU: larger
// per-wave register tiles are the next step.
//
// No inline assembly, builtins and plain C++ only.

#include "gemmcheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

typedef int gc_i32x4 __attribute__((ext_vector_type(4)));
typedef int gc_i32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 gc_bf16x8 __attribute__((ext_vector_type(8)));

#define GC_MAX_K_BF16 32768    // 16 . 16 . K <= 2**23: f32 sums stay exact
#define GC_MAX_K_I8 131072     // 128 . 128 . K < 2**31 below this

struct GcBf16 {
  typedef f32x16 Acc;
  static constexpr u32 STAGE = 0;
  static __device__ __forceinline__ Acc mfma(const u32x4& a, const u32x4& b, const Acc& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(gc_bf16x8, a),
                                                   __builtin_bit_cast(gc_bf16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ u32 bits(float c) {
    u32 b = __float_as_uint(c);
    return (b << 1) == 0u ? 0u : b;
  }
};

struct GcI8 {
  typedef gc_i32x16 Acc;
  static constexpr u32 STAGE = 1;
  static __device__ __forceinline__ Acc mfma(const u32x4& a, const u32x4& b, const Acc& c) {
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(__builtin_bit_cast(gc_i32x4, a),
                                                 __builtin_bit_cast(gc_i32x4, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ u32 bits(int c) { return (u32)c; }
};

#if __HIP_DEVICE_COMPILE__
extern __shared__ u32x4 gc_lds[];
#endif

template <typename T, typename SINK>
__global__ void __launch_bounds__(GC_THREADS) gemmcheck_kernel(CuArgs a, GcArgs g) {
#if __HIP_DEVICE_COMPILE__
  typedef typename T::Acc Acc;
  const u32 tid = threadIdx.x, lane = tid % WAVE, wv = tid / WAVE;
  GcWhere w;
  w.lane = (int)lane;
  w.gwave = blockIdx.x * GC_WAVES + wv;
  w.hw = cu_locate_wave(a.res, (int)lane);
  w.quadrant = wv;
  const u32 wr = wv >> 1, wc = wv & 1u;

  // staging: chunk sc of rows sr + 32 i of both operands
  const u32 sc = tid & 7u, sr = tid >> 3;
  const u32 wunit = GC_ROW_UNITS * sr + (sc ^ ((sr >> 1) & 7u));  // + 256 i
  // fragments: row rl of each 32-row block, half h of a k-step's 32 bytes
  const u32 rl = lane & 31u, h = lane >> 5, rswz = (rl >> 1) & 7u;
  const u32 aunit = GC_ROW_UNITS * (64u * wr + rl);
  const u32 bunit = GC_OP_UNITS + GC_ROW_UNITS * (64u * wc + rl);
  const size_t pitch = (size_t)g.slabs * GC_ROW_UNITS;
  const u32 tiles = g.tm * g.tn;

  for (u32 t = blockIdx.x; t < g.steps; t += gridDim.x) {
    w.round = t / tiles;
    w.first_of_round = t < gridDim.x || (t - gridDim.x) / tiles != w.round;
    gc_tile(t - w.round * tiles, g.tm, g.tn, w.bi, w.bj);
    const u32x4* ga = g.a + ((size_t)w.bi * GC_TILE + sr) * pitch + sc;
    const u32x4* gb = g.bt + ((size_t)w.bj * GC_TILE + sr) * pitch + sc;

    Acc acc[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[x][y][e] = 0;

    u32x4 ra[4], rb[4];
#pragma unroll
    for (u32 i = 0; i < 4u; ++i) {
      ra[i] = ga[32u * i * pitch];
      rb[i] = gb[32u * i * pitch];
    }
#pragma unroll
    for (u32 i = 0; i < 4u; ++i) {
      gc_lds[wunit + 256u * i] = ra[i];
      gc_lds[GC_OP_UNITS + wunit + 256u * i] = rb[i];
    }
    __syncthreads();

    for (u32 s = 0; s < g.slabs; ++s) {
      const u32 cur = (s & 1u) * GC_STAGE_UNITS;
      const bool more = s + 1u < g.slabs;
      if (more) {  // in flight while this slab's MFMAs run
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
          ra[i] = ga[32u * i * pitch + (size_t)(s + 1u) * GC_ROW_UNITS];
          rb[i] = gb[32u * i * pitch + (size_t)(s + 1u) * GC_ROW_UNITS];
        }
      }
#pragma unroll
      for (u32 kk = 0; kk < 4u; ++kk) {
        const u32 c = (2u * kk + h) ^ rswz;
        u32x4 fa[2], fb[2];
#pragma unroll
        for (u32 x = 0; x < 2u; ++x) {
          fa[x] = gc_lds[cur + aunit + 256u * x + c];
          fb[x] = gc_lds[cur + bunit + 256u * x + c];
        }
#pragma unroll
        for (int x = 0; x < 2; ++x)
#pragma unroll
          for (int y = 0; y < 2; ++y) acc[x][y] = T::mfma(fa[x], fb[y], acc[x][y]);
      }
      if (more) {
        const u32 nxt = cur ^ GC_STAGE_UNITS;
#pragma unroll
        for (u32 i = 0; i < 4u; ++i) {
          gc_lds[nxt + wunit + 256u * i] = ra[i];
          gc_lds[nxt + GC_OP_UNITS + wunit + 256u * i] = rb[i];
        }
      }
      // slab s+1 is written, and nobody still reads slab s, which the
      // next iteration (or the next tile's first slab) overwrites
      __syncthreads();
    }

    // C/D map of the 32x32 MFMAs: cu_tile_index
    SINK sink(g, w.bi, w.bj);
#pragma unroll
    for (u32 x = 0; x < 2u; ++x)
#pragma unroll
      for (u32 y = 0; y < 2u; ++y)
#pragma unroll
        for (u32 e = 0; e < 16u; ++e)
          sink.put(64u * wr + 32u * x + (e & 3u) + 8u * (e >> 2) + 4u * h,
                   64u * wc + 32u * y + rl, T::bits(acc[x][y][e]));
    sink.finish(a, g, T::STAGE, w);
  }
#endif
}

// ---------------------------------------------------------------- host

// Operand checks shared by gemm_nt and gemmcheck_run; fills the shape.
static GcArgs gc_check_operands(const at::Tensor& a, const at::Tensor& bt, bool& is_i8) {
  TORCH_CHECK(a.is_cuda() && bt.is_cuda() && a.get_device() == bt.get_device(),
              "gemmcheck: a and bt must be on the same GPU");
  TORCH_CHECK(a.dim() == 2 && bt.dim() == 2 && a.is_contiguous() && bt.is_contiguous(),
              "gemmcheck: a [M, K] and bt [N, K] must be contiguous matrices");
  TORCH_CHECK(a.scalar_type() == bt.scalar_type() &&
                  (a.scalar_type() == at::kBFloat16 || a.scalar_type() == at::kChar),
              "gemmcheck: a and bt must both be bfloat16 or both int8");
  is_i8 = a.scalar_type() == at::kChar;
  const int64_t m = a.size(0), n = bt.size(0), k = a.size(1);
  const int64_t slab = is_i8 ? GC_SLAB_BYTES : GC_SLAB_BYTES / 2;
  TORCH_CHECK(bt.size(1) == k, "gemmcheck: a is [M, ", k, "] but bt is [N, ", bt.size(1), "]");
  TORCH_CHECK(m >= GC_TILE && n >= GC_TILE && m % GC_TILE == 0 && n % GC_TILE == 0,
              "gemmcheck: M and N must be positive multiples of ", GC_TILE, ", got ", m, " and ", n);
  TORCH_CHECK(k >= slab && k % slab == 0, "gemmcheck: K must be a positive multiple of ", slab,
              ", got ", k);
  TORCH_CHECK(is_i8 || k <= GC_MAX_K_BF16, "gemmcheck: bfloat16 needs K <= ", GC_MAX_K_BF16,
              ", got ", k);
  TORCH_CHECK(!is_i8 || k < GC_MAX_K_I8, "gemmcheck: int8 needs K < ", GC_MAX_K_I8, ", got ", k);
  TORCH_CHECK((m / GC_TILE) * (n / GC_TILE) <= GC_MAX_STEPS, "gemmcheck: too many tiles");
  GcArgs g;
  g.a = (const u32x4*)a.data_ptr();
  g.bt = (const u32x4*)bt.data_ptr();
  g.out = nullptr;
  g.tm = (u32)(m / GC_TILE);
  g.tn = (u32)(n / GC_TILE);
  g.slabs = (u32)(k / slab);
  g.steps = g.tm * g.tn;
  return g;
}

template <typename T, typename SINK>
static void gc_launch(int64_t blocks, const CuArgs& ca, const GcArgs& g) {
  auto kernel = gemmcheck_kernel<T, SINK>;
  C10_HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize, GC_LDS_BYTES));
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(GC_THREADS), (size_t)GC_LDS_BYTES,
                     at::hip::getCurrentHIPStream(), ca, g);
}

// C = a . bt^T on the GPU of the operands: float32 for bfloat16 operands,
// int32 for int8.  Exact whenever every partial sum is representable.
at::Tensor gemm_nt(at::Tensor a, at::Tensor bt, int64_t blocks_arg) {
  bool is_i8;
  GcArgs g = gc_check_operands(a, bt, is_i8);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(a));
  const int64_t blocks = gc_grid(blocks_arg, g.steps);
  at::Tensor out = at::empty({(int64_t)g.tm * GC_TILE, (int64_t)g.tn * GC_TILE},
                             a.options().dtype(is_i8 ? at::kInt : at::kFloat));
  at::Tensor res = gc_result_block(a, 0);  // only the per-CU wave table is used
  g.out = (u32*)out.data_ptr();
  const CuArgs ca = {0, 1, nullptr, (u32*)res.data_ptr(), 0, nullptr, NO_INJECT, 0, 0, 0};
  if (is_i8) gc_launch<GcI8, GcStore>(blocks, ca, g);
  else gc_launch<GcBf16, GcStore>(blocks, ca, g);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return out;
}

// `rounds` GEMMs in one launch, every wave's fold compared with
// expected[class][quadrant] (int32 [4, 4] on the GPU); nothing of C is
// stored.  inject = (wave of the grid, round, stage, mask).
CucheckOut gemmcheck_run(at::Tensor a, at::Tensor bt, at::Tensor expected, int64_t rounds,
                         int64_t blocks_arg, int64_t max_records,
                         c10::optional<CuInject> inject) {
  bool is_i8;
  GcArgs g = gc_check_operands(a, bt, is_i8);
  TORCH_CHECK(rounds >= 1 && rounds <= MAX_ROUNDS, "gemmcheck: rounds must be in 1..",
              MAX_ROUNDS, ", got ", rounds);
  TORCH_CHECK(rounds * (int64_t)g.steps <= GC_MAX_STEPS, "gemmcheck: rounds x tiles must be <= ",
              GC_MAX_STEPS);
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT,
              "gemmcheck: max_records must be in 0..", MAX_RECORDS_LIMIT);
  TORCH_CHECK(expected.is_cuda() && expected.get_device() == a.get_device() &&
                  expected.scalar_type() == at::kInt && expected.is_contiguous() &&
                  expected.numel() == 16,
              "gemmcheck: expected must be a contiguous int32 [4, 4] tensor on the operands' GPU");
  g.steps = (u32)(rounds * (int64_t)g.steps);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(a));
  const int64_t blocks = gc_grid(blocks_arg, g.steps);
  at::Tensor res = gc_result_block(a, max_records);
  CuArgs ca = {0, (u32)rounds, (const u32*)expected.data_ptr(), (u32*)res.data_ptr(),
               (int)max_records, nullptr, NO_INJECT, 0, 0, 0};
  if (inject.has_value()) {
    int64_t w = std::get<0>(*inject), r = std::get<1>(*inject);
    int64_t s = std::get<2>(*inject), m = std::get<3>(*inject);
    TORCH_CHECK(w >= 0 && w < blocks * GC_WAVES && r >= 0 && r < rounds &&
                    s == (is_i8 ? 1 : 0) && m >= 0 && m <= 0xFFFFFFFFLL,
                "gemmcheck: inject (wave, round, stage, mask) out of range");
    ca.inj_wave = (u32)w;
    ca.inj_round = (u32)r;
    ca.inj_stage = (u32)s;
    ca.inj_mask = (u32)m;
  }

  auto stream = at::hip::getCurrentHIPStream();
  hipEvent_t t0, t1;
  C10_HIP_CHECK(hipEventCreate(&t0));
  C10_HIP_CHECK(hipEventCreate(&t1));
  C10_HIP_CHECK(hipEventRecord(t0, stream));
  if (is_i8) gc_launch<GcI8, GcFold>(blocks, ca, g);
  else gc_launch<GcBf16, GcFold>(blocks, ca, g);
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

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about a second.
void bind_gemmcheck(py::module_& m) {
  m.def("gemm_nt", &gemm_nt,
        "C = a . bt^T (bfloat16 -> float32, int8 -> int32) by the gemmcheck tile kernel",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("a"), py::arg("bt"), py::arg("blocks") = 0);
  m.def("gemmcheck_run", &gemmcheck_run,
        "tiled-GEMM load run -> (mismatches, first_bad_round, stage_mask, records, "
        "waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("a"), py::arg("bt"), py::arg("expected"), py::arg("rounds"),
        py::arg("blocks") = 0, py::arg("max_records") = 16, py::arg("inject") = py::none());
}
