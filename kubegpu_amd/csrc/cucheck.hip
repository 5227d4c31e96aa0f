// cucheck — compute-unit integrity kernel (gfx950), compiled into _gpuprobe.
//
// The compute twin of memcheck.hip.  Every wave of the launch runs the
// same deterministic workload and compares four 32-bit digests per round
// with values the host computed independently in numpy
// (probe/cucheck.py:reference_digests is the definition):
//   stage 0 mfma_i8    32x32 tile, K = 256: eight v_mfma_i32_32x32x32_i8
//   stage 1 mfma_bf16  32x32 tile, K = 128: eight v_mfma_f32_32x32x16_bf16
//   stage 2 valu       32 steps of integer mul/rotate/mulhi + one f32 FMA
//   stage 3 lds        the wave's 1/16 slice of the workgroup's LDS written,
//                      read back by another lane, complemented, read again
// Inputs are word(stage, r, idx) = fmix32(base(seed, stage, r) + idx) cut
// into signed bytes.  Every floating-point intermediate is an exactly
// representable integer, so rounding logic is not covered (fpcheck.hip's
// ground).
//
// 1024-thread workgroups (16 waves); with the default 160 KiB of dynamic
// LDS one workgroup fills a CU, so a grid of multiProcessorCount puts one
// workgroup on every CU of an idle GPU.  HIP promises no placement: each
// wave reads where it runs from HW_ID / XCC_ID and the host reports the
// coverage (waves_on) instead of assuming it.  Workgroups share nothing,
// waves of a workgroup share only the LDS allocation.
//
// The stage bodies are templates over a sink.  cucheck_kernel folds their
// values into the digests; cucheck_values_kernel, one workgroup of which
// one wave works, stores them, so that the tests can compare every tile
// element, every step of the VALU chain and every LDS word read back with
// numpy, and an operator can ask which element a failing digest hides.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ u32 cu_rotl32(u32 x, int r) {
  return (x << r) | (x >> (32 - r));
}

// bf16 of a signed byte: every integer in [-128, 127] has at most eight
// significant bits, so the top half of its f32 encoding is exact.
__device__ __forceinline__ __bf16 byte_to_bf16(u32 w, int b) {
  float f = (float)(int)(signed char)(w >> (8 * b));
  unsigned short bits = (unsigned short)(__float_as_uint(f) >> 16);
  return __builtin_bit_cast(__bf16, bits);
}

// Where a stage's values go.  The stage bodies below hand every value
// to a sink: cucheck_kernel folds them into the digest that is compared,
// cucheck_values_kernel stores them so that a test, or an operator after
// a failure, can look at each one.  Both run the same stage code.
struct CuFold {
  u32 dig = 0;  // the stage's digest once the stage is done
  u32 acc = 0;  // per-lane running sum of the lds stage
  template <typename ACC>
  __device__ __forceinline__ void tile(const ACC& c, int lane) {
    dig = fold_tile(c, lane);
  }
  __device__ __forceinline__ void valu_step(int, int, u32) {}
  __device__ __forceinline__ void valu_done(int lane, u32 x) {
    dig = wave_sum(cu_fmix32(x + (u32)lane));
  }
  __device__ __forceinline__ void lds_word(u32, u32 d, u32 got) {
    acc += cu_fmix32(got + cu_salt(d));
  }
  __device__ __forceinline__ void lds_done() { dig = wave_sum(acc); }
};

// Layouts (probe/cucheck.py documents them): tile [32, 32] row-major,
// valu [iteration, lane], lds [pass, dword of the slice].
struct CuDump {
  long long* out;
  u32 lds_dwords;
  template <typename ACC>
  __device__ __forceinline__ void tile(const ACC& c, int lane) {
#pragma unroll
    for (int g = 0; g < 16; ++g) out[cu_tile_index(g, lane)] = (long long)c[g];
  }
  __device__ __forceinline__ void valu_step(int it, int lane, u32 x) {
    out[WAVE * it + lane] = x;
  }
  __device__ __forceinline__ void valu_done(int, u32) {}
  __device__ __forceinline__ void lds_word(u32 inv, u32 d, u32 got) {
    out[(size_t)inv * lds_dwords + d] = got;
  }
  __device__ __forceinline__ void lds_done() {}
};

// operand maps of the matrix stages: lane l owns row l&31 of A and column
// l&31 of B (rc), half = l>>5; the k a fragment slot stands for is the
// same for A and B, and C = A*B does not change under a permutation of k
// applied to both

// stage 0: int8 matrix core, slot p of step s is k = 32s + 16*half + p
template <typename SINK>
__device__ __forceinline__ void cu_stage_i8(u32 base, u32 rc, u32 half, int lane,
                                            SINK& sink) {
#if __HIP_DEVICE_COMPILE__
  i32x16 acc = {0};
#pragma unroll
  for (u32 s = 0; s < 8; ++s) {
    u32 w0 = 64 * rc + 8 * s + 4 * half;
    i32x4 a, b;
#pragma unroll
    for (u32 w = 0; w < 4; ++w) {
      a[w] = (int)cu_fmix32(base + w0 + w);
      b[w] = (int)cu_fmix32(base + 2048u + w0 + w);
    }
    acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
  }
  sink.tile(acc, lane);
#endif
}

// stage 1: bf16 matrix core, slot j of step s is k = 16s + 8*half + j
template <typename SINK>
__device__ __forceinline__ void cu_stage_bf16(u32 base, u32 rc, u32 half, int lane,
                                              SINK& sink) {
#if __HIP_DEVICE_COMPILE__
  f32x16 acc = {0.f};
#pragma unroll
  for (u32 s = 0; s < 8; ++s) {
    u32 w0 = 32 * rc + 4 * s + 2 * half;
    u32 aw0 = cu_fmix32(base + w0), aw1 = cu_fmix32(base + w0 + 1u);
    u32 bw0 = cu_fmix32(base + 1024u + w0), bw1 = cu_fmix32(base + 1024u + w0 + 1u);
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = byte_to_bf16(aw0, j);
      a[4 + j] = byte_to_bf16(aw1, j);
      b[j] = byte_to_bf16(bw0, j);
      b[4 + j] = byte_to_bf16(bw1, j);
    }
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
  }
  sink.tile(acc, lane);
#endif
}

// stage 2: vector ALU, integer and f32 FMA
template <typename SINK>
__device__ __forceinline__ void cu_stage_valu(u32 base, int lane, SINK& sink) {
  u32 x = cu_fmix32(base + (u32)lane);
  for (int it = 0; it < 32; ++it) {
    x = x * 0x9E3779B1u + cu_rotl32(x, 13);
    x ^= __umulhi(x, 0x85EBCA6Bu);
    x += (u32)__fmaf_rn((float)(x & 0xFFFu), (float)((x >> 12) & 0xFFFu),
                        (float)(x >> 24));
    sink.valu_step(it, lane, x);
  }
  sink.valu_done(lane, x);
}

// stage 3: LDS march over this wave's slice; lane l writes dword 64t + l
// and reads 64t + 63 - l.  The fences wait for LDS and keep the compiler
// from moving accesses across them.
template <typename SINK>
__device__ __forceinline__ void cu_stage_lds(u32 base, u32* slice, u32 lds_dwords,
                                             int lane, SINK& sink) {
#if __HIP_DEVICE_COMPILE__
  for (u32 inv = 0; inv < 2; ++inv) {
    u32 flip = inv ? 0xFFFFFFFFu : 0u;
    for (u32 t = 0; t < lds_dwords; t += WAVE)
      slice[t + lane] = cu_fmix32(base + t + lane) ^ flip;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (u32 t = 0; t < lds_dwords; t += WAVE) {
      u32 d = t + (WAVE - 1 - lane);
      sink.lds_word(inv, d, slice[d]);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
  sink.lds_done();
#endif
}

__global__ void __launch_bounds__(CU_BLOCK)
cucheck_kernel(CuArgs a, u32 lds_dwords) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ u32 lds[];
  // not w.lane: with it wave_sum's shuffle addresses stay live across the
  // round loop, 82 VGPRs instead of 80, one occupancy step
  const int lane = threadIdx.x % WAVE;
  const CuWave w = cu_wave(a);
  const u32 rc = lane & 31, half = lane >> 5;
  u32* slice = lds + threadIdx.x / WAVE * lds_dwords;

  for (u32 r = 0; r < a.rounds; ++r) {
    CuFold f0, f1, f2, f3;
    cu_stage_i8(cu_base(a.seed, 0, r), rc, half, lane, f0);
    cu_stage_bf16(cu_base(a.seed, 1, r), rc, half, lane, f1);
    cu_stage_valu(cu_base(a.seed, 2, r), lane, f2);
    cu_stage_lds(cu_base(a.seed, 3, r), slice, lds_dwords, lane, f3);
    u32 dig[N_STAGES] = {f0.dig, f1.dig, f2.dig, f3.dig};

    cu_check_round(dig, r, w, a);
  }
  // keep the workgroup's LDS allocated until all its waves are done
  __syncthreads();
#endif
}

// One workgroup with the production kernel's LDS allocation; wave `wave`
// of it runs one stage of one round on its own slice and stores every
// value (CuDump), the other waves return at once.  No barrier: nothing
// waits for a wave that has left.
__global__ void __launch_bounds__(CU_BLOCK)
cucheck_values_kernel(u32 seed, u32 stage, u32 r, u32 lds_dwords, u32 wave,
                      long long* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ u32 lds[];
  if (threadIdx.x / WAVE != wave) return;
  const int lane = threadIdx.x % WAVE;
  const u32 rc = lane & 31, half = lane >> 5;
  const u32 base = cu_base(seed, stage, r);
  CuDump sink;
  sink.out = out;
  sink.lds_dwords = lds_dwords;
  if (stage == 0)
    cu_stage_i8(base, rc, half, lane, sink);
  else if (stage == 1)
    cu_stage_bf16(base, rc, half, lane, sink);
  else if (stage == 2)
    cu_stage_valu(base, lane, sink);
  else
    cu_stage_lds(base, lds + wave * lds_dwords, lds_dwords, lane, sink);
#endif
}

// ---------------------------------------------------------------- host

static void cu_check_lds_bytes(int64_t lds_bytes) {
  TORCH_CHECK(lds_bytes >= LDS_STEP && lds_bytes <= MAX_LDS_BYTES &&
                  lds_bytes % LDS_STEP == 0,
              "cucheck: lds_bytes must be a multiple of ", LDS_STEP, " in ", LDS_STEP,
              "..", MAX_LDS_BYTES, ", got ", lds_bytes);
}

CucheckOut cucheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                       int64_t blocks_arg, int64_t lds_bytes, int64_t max_records,
                       c10::optional<at::Tensor> dump,
                       c10::optional<CuInject> inject) {
  cu_check_lds_bytes(lds_bytes);
  CuLaunch l = cu_prepare("cucheck", expected, seed_arg, rounds, blocks_arg,
                          max_records, dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(cucheck_kernel, l, lds_bytes, (u32)(lds_bytes / 4 / CU_WAVES));
}

// The values wave `wave` of one workgroup computed for one stage and
// round, as an int64 tensor on the current GPU: [32, 32], [32, 64] or
// [2, lds_dwords].  Every refusal comes before the launch.
at::Tensor cucheck_values(int64_t seed_arg, int64_t stage, int64_t round,
                          int64_t lds_bytes, int64_t wave) {
  cu_check_wave_args("cucheck", seed_arg, stage, round);
  cu_check_lds_bytes(lds_bytes);
  TORCH_CHECK(wave >= 0 && wave < CU_WAVES, "cucheck: wave must be in 0..", CU_WAVES - 1,
              ", got ", wave);
  const int64_t lds_dwords = lds_bytes / 4 / CU_WAVES;
  const int64_t rows = stage == 3 ? 2 : 32;
  const int64_t cols = stage == 3 ? lds_dwords : stage == 2 ? WAVE : 32;
  at::Tensor out =
      at::zeros({rows, cols}, at::TensorOptions().dtype(at::kLong).device(at::kCUDA));
  return cu_launch_values(cucheck_values_kernel, CU_BLOCK, lds_bytes, out, (u32)seed_arg,
                          (u32)stage, (u32)round, (u32)lds_dwords, (u32)wave,
                          (long long*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run (22,528 rounds at 22.6 us each on MI355X,
// profiles/cucheck_mi355x.json) holds the GPU for half a second.
void bind_cucheck(py::module_& m) {
  m.def("cucheck_run", &cucheck_run,
        "compute-unit integrity run -> (mismatches, first_bad_round, stage_mask, "
        "records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"),
        py::arg("blocks") = 0, py::arg("lds_bytes") = MAX_LDS_BYTES,
        py::arg("max_records") = 16, py::arg("dump") = py::none(),
        py::arg("inject") = py::none());
  m.def("cucheck_values", &cucheck_values,
        "values of one wave, stage and round as int64 [32, 32], [32, 64] or "
        "[2, lds_dwords]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"),
        py::arg("lds_bytes") = MAX_LDS_BYTES, py::arg("wave") = 0);
}
