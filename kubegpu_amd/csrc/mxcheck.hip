// mxcheck — matrix-core integrity kernel for the f16, OCP fp8, block-scaled
// MXFP4 and f64 paths (gfx950), compiled into _gpuprobe.
//
// The twin of cucheck.hip for the number formats that kernel leaves out.
// Every wave of the launch runs the same deterministic workload and
// compares four 32-bit digests per round with values the host computed
// independently in numpy (probe/mxcheck.py:reference_digests is the
// definition, and defines A, B and the block scales of every stage):
//   stage 0 mfma_f16    32x32 tile, K = 128: eight v_mfma_f32_32x32x16_f16
//   stage 1 mfma_fp8    32x32 tile, K = 128: eight v_mfma_f32_32x32x16_fp8_bf8
//                       (A e4m3fn, B e5m2)
//   stage 2 mfma_mxfp4  32x32 tile, K = 256: four
//                       v_mfma_scale_f32_32x32x64_f8f6f4, A and B e2m1, one
//                       E8M0 scale per 32 elements of k
//   stage 3 mfma_f64    16x16 tile, K = 32: eight v_mfma_f64_16x16x4_f64
// Inputs are word(4 + stage, r, idx) of cucheck_common.h, so they differ
// from cucheck's.  Every operand is chosen so that all partial sums are
// exactly representable in the accumulator type: the result is an integer
// in the stage's unit whatever order the hardware sums in, and rounding
// logic is not covered (fpcheck.hip's ground).
//
// Launch shape and accounting are cucheck's: 1024-thread workgroups (16
// waves), grid 0 = one workgroup per CU, each wave reads HW_ID / XCC_ID
// once and is counted in waves_on.  Nothing here touches the LDS; the
// 160 KiB of dynamic LDS are asked for only so that one workgroup fills
// a CU and the default grid lands one workgroup on every CU.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

#define MX_STAGE0 4u  // stage number fed to cu_base() is MX_STAGE0 + stage
// FMT field of the scaled MFMA (cbsz for A, blgp for B): 0 e4m3, 1 e5m2,
// 2 e2m3, 3 e3m2, 4 e2m1
#define FMT_E2M1 4

// C/D map of the f64 MFMA: lane l, register g holds row (l>>4) + 4g,
// column l&15 (not the f32 16x16 map).  Row-major index of that element.
__device__ __forceinline__ u32 mx_f64_index(int g, int lane) {
  return 16 * ((lane >> 4) + 4 * g) + (lane & 15);
}

// Where a stage's accumulator tile goes, as in cucheck.hip: mxcheck_kernel
// folds it into the digest, mxcheck_tile_kernel stores it; both run the
// same stage code and go through the same two C/D maps.
struct MxFold {
  u32 dig = 0;
  // 32x32 f32 tile in units of 1/unit -> exact integers, cucheck's fold
  __device__ __forceinline__ void tile(f32x16 acc, float unit, int lane) {
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] *= unit;  // power of two: exact
    dig = fold_tile(acc, lane);
  }
  // 16x16 f64 tile: both halves of the two's-complement int64
  __device__ __forceinline__ void tile_f64(const f64x4& acc, int lane) {
    u32 d = 0;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u32 n = mx_f64_index(g, lane);
      long long c = (long long)acc[g];
      d += cu_fmix32((u32)c + cu_salt(n)) + cu_fmix32((u32)(c >> 32) + cu_salt(256u + n));
    }
    dig = wave_sum(d);
  }
};

// Row-major as f64, in the stage's unit.
struct MxDump {
  double* out;
  __device__ __forceinline__ void tile(const f32x16& acc, float unit, int lane) {
#pragma unroll
    for (int g = 0; g < 16; ++g) out[cu_tile_index(g, lane)] = (double)(acc[g] * unit);
  }
  __device__ __forceinline__ void tile_f64(const f64x4& acc, int lane) {
#pragma unroll
    for (int g = 0; g < 4; ++g) out[mx_f64_index(g, lane)] = acc[g];
  }
};

// In all 32x32 stages lane l owns row rc = l&31 of A and column rc of B.
// The k a fragment slot stands for is the same for A and B, and C = A*B
// does not change under a permutation of k applied to both, so only the
// set of k a lane half holds in a step matters: half h = l>>5 of step s
// holds the h-th half of the step's k range.

// stage 0: f16.  Step s, half h: k = 16s + 8h + j, j = 0..7, two k per
// word.  A is the sign-extended low 11 bits of a 16-bit half (the whole
// f16 significand), B the low 5 bits.
template <typename SINK>
__device__ __forceinline__ void mx_stage_f16(u32 base, u32 rc, u32 half, int lane,
                                             SINK& sink) {
  f32x16 acc = {0.f};
#pragma unroll
  for (u32 s = 0; s < 8; ++s) {
    u32 w0 = 64 * rc + 8 * s + 4 * half;
    f16x8 a, b;
#pragma unroll
    for (u32 w = 0; w < 4; ++w) {
      u32 aw = cu_fmix32(base + w0 + w), bw = cu_fmix32(base + 2048u + w0 + w);
      a[2 * w] = (_Float16)(short)((int)(aw << 21) >> 21);
      a[2 * w + 1] = (_Float16)(short)((int)(aw << 5) >> 21);
      b[2 * w] = (_Float16)(short)((int)(bw << 27) >> 27);
      b[2 * w + 1] = (_Float16)(short)((int)(bw << 11) >> 27);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  }
  sink.tile(acc, 1.f, lane);
}

// stage 1: OCP fp8.  Step s, half h: k = 16s + 8h + j, j = 0..7, one byte
// per k.  The raw byte keeps its sign and mantissa; the exponent field is
// forced to bias + 0..3, so no zero, subnormal, Inf or NaN is fed.
__device__ __forceinline__ u32 mx_e4m3_codes(u32 w) {
  return (w & 0x87878787u) | ((0x07070707u + ((w >> 3) & 0x03030303u)) << 3);
}

__device__ __forceinline__ u32 mx_e5m2_codes(u32 w) {
  return (w & 0x83838383u) | ((0x0F0F0F0Fu + ((w >> 2) & 0x03030303u)) << 2);
}

// The tile is in units of 1/32.
template <typename SINK>
__device__ __forceinline__ void mx_stage_fp8(u32 base, u32 rc, u32 half, int lane,
                                             SINK& sink) {
  f32x16 acc = {0.f};
#pragma unroll
  for (u32 s = 0; s < 8; ++s) {
    u32 w0 = 32 * rc + 4 * s + 2 * half;
    unsigned long long a =
        (unsigned long long)mx_e4m3_codes(cu_fmix32(base + w0)) |
        ((unsigned long long)mx_e4m3_codes(cu_fmix32(base + w0 + 1u)) << 32);
    unsigned long long b =
        (unsigned long long)mx_e5m2_codes(cu_fmix32(base + 1024u + w0)) |
        ((unsigned long long)mx_e5m2_codes(cu_fmix32(base + 1024u + w0 + 1u)) << 32);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_fp8_bf8((long)a, (long)b, acc, 0, 0, 0);
  }
  sink.tile(acc, 32.f, lane);
}

// stage 2: block-scaled e2m1.  A lane holds the 32 elements of row /
// column rc and 32-element k-block 2s + h of step s in its first four
// operand VGPRs (eight nibbles per word; the upper four VGPRs are not
// read for this format), and byte 0 of its own scale VGPR (op_sel 0) is
// the E8M0 scale of exactly those 32 elements.  Scales are 127 + two
// bits of the row's / column's scale word, so 2^0 .. 2^3.  The tile is in
// units of 1/4.
template <typename SINK>
__device__ __forceinline__ void mx_stage_mxfp4(u32 base, u32 rc, u32 half, int lane,
                                               SINK& sink) {
  const u32 sa_word = cu_fmix32(base + 2048u + rc);
  const u32 sb_word = cu_fmix32(base + 2080u + rc);
  f32x16 acc = {0.f};
#pragma unroll
  for (u32 s = 0; s < 4; ++s) {
    u32 blk = 2 * s + half;
    u32 w0 = 32 * rc + 4 * blk;
    i32x8 a = {0}, b = {0};
#pragma unroll
    for (u32 w = 0; w < 4; ++w) {
      a[w] = (int)cu_fmix32(base + w0 + w);
      b[w] = (int)cu_fmix32(base + 1024u + w0 + w);
    }
    int sa = (int)(127u + ((sa_word >> (2 * blk)) & 3u));
    int sb = (int)(127u + ((sb_word >> (2 * blk)) & 3u));
    acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, FMT_E2M1, FMT_E2M1,
                                                          0, sa, 0, sb);
  }
  sink.tile(acc, 4.f, lane);
}

// stage 3: f64, 16x16 tile.  Lane l holds A[l&15][4s + (l>>4)] and
// B[4s + (l>>4)][l&15] of step s; operands are the sign-extended low 24
// bits of a word.
template <typename SINK>
__device__ __forceinline__ void mx_stage_f64(u32 base, int lane, SINK& sink) {
  const u32 rc = lane & 15, kq = lane >> 4;
  f64x4 acc = {0.0};
#pragma unroll
  for (u32 s = 0; s < 8; ++s) {
    u32 w = 32 * rc + 4 * s + kq;
    double a = (double)((int)(cu_fmix32(base + w) << 8) >> 8);
    double b = (double)((int)(cu_fmix32(base + 512u + w) << 8) >> 8);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
  }
  sink.tile_f64(acc, lane);
}

__global__ void __launch_bounds__(CU_BLOCK)
mxcheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const int lane = w.lane;
  const u32 rc = lane & 31, half = lane >> 5;

  for (u32 r = 0; r < a.rounds; ++r) {
    MxFold f0, f1, f2, f3;
    mx_stage_f16(cu_base(a.seed, MX_STAGE0 + 0, r), rc, half, lane, f0);
    mx_stage_fp8(cu_base(a.seed, MX_STAGE0 + 1, r), rc, half, lane, f1);
    mx_stage_mxfp4(cu_base(a.seed, MX_STAGE0 + 2, r), rc, half, lane, f2);
    mx_stage_f64(cu_base(a.seed, MX_STAGE0 + 3, r), lane, f3);
    u32 dig[N_STAGES] = {f0.dig, f1.dig, f2.dig, f3.dig};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One workgroup; wave 0 runs one stage of one round and stores its
// accumulator tile (MxDump) in the stage's unit (1, 1/32, 1/4, 1): 32x32
// for stages 0-2, 16x16 for stage 3.  A digest cannot say which element
// is wrong; this can.
__global__ void __launch_bounds__(CU_BLOCK)
mxcheck_tile_kernel(u32 seed, u32 stage, u32 r, double* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  if (threadIdx.x >= WAVE) return;
  const int lane = threadIdx.x;
  const u32 base = cu_base(seed, MX_STAGE0 + stage, r);
  const u32 rc = lane & 31, half = lane >> 5;
  MxDump sink{out};
  if (stage == 0)
    mx_stage_f16(base, rc, half, lane, sink);
  else if (stage == 1)
    mx_stage_fp8(base, rc, half, lane, sink);
  else if (stage == 2)
    mx_stage_mxfp4(base, rc, half, lane, sink);
  else
    mx_stage_f64(base, lane, sink);
#endif
}

// ---------------------------------------------------------------- host

CucheckOut mxcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                       int64_t blocks_arg, int64_t max_records,
                       c10::optional<at::Tensor> dump,
                       c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("mxcheck", expected, seed_arg, rounds, blocks_arg,
                          max_records, dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(mxcheck_kernel, l, MAX_LDS_BYTES);
}

// The accumulator tile of one stage and round as a float64 tensor on the
// current GPU, [32, 32] or [16, 16].
at::Tensor mxcheck_tile(int64_t seed_arg, int64_t stage, int64_t round) {
  cu_check_wave_args("mxcheck", seed_arg, stage, round);
  int64_t n = stage == 3 ? 16 : 32;
  at::Tensor out = at::zeros({n, n}, at::TensorOptions().dtype(at::kDouble).device(at::kCUDA));
  return cu_launch_values(mxcheck_tile_kernel, CU_BLOCK, 0, out, (u32)seed_arg, (u32)stage,
                          (u32)round, (double*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/mxcheck_mi355x.json).
void bind_mxcheck(py::module_& m) {
  m.def("mxcheck_run", &mxcheck_run,
        "matrix-core format integrity run -> (mismatches, first_bad_round, "
        "stage_mask, records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"),
        py::arg("blocks") = 0, py::arg("max_records") = 16,
        py::arg("dump") = py::none(), py::arg("inject") = py::none());
  m.def("mxcheck_tile", &mxcheck_tile,
        "accumulator tile of one stage and round as float64 [n, n]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"));
}
