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
// representable integer, so rounding logic is not covered.
//
// 1024-thread workgroups (16 waves); with the default 160 KiB of dynamic
// LDS one workgroup fills a CU, so a grid of multiProcessorCount puts one
// workgroup on every CU of an idle GPU.  HIP promises no placement: each
// wave reads where it runs from HW_ID / XCC_ID and the host reports the
// coverage (waves_on) instead of assuming it.  Workgroups share nothing,
// waves of a workgroup share only the LDS allocation.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <tuple>
#include <vector>

#define WAVE 64
#define CU_BLOCK 1024
#define CU_WAVES (CU_BLOCK / WAVE)
#define N_STAGES 4
#define MAX_ROUNDS 65536
#define MAX_BLOCKS 4096
#define MAX_LDS_BYTES 163840
#define LDS_STEP 4096
#define MAX_RECORDS_LIMIT 4096
#define NO_INJECT 0xFFFFFFFFu

typedef unsigned int u32;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// Result block in device memory (u32 slots): header, the per-CU wave
// table indexed xcc<<7 | se<<5 | sh<<4 | cu, then max_records records
// of six u32 each: {global wave, xcc<<16 | HW_ID[15:0], round, stage,
// expected, got}.
#define RES_COUNT 0
#define RES_FIRST 1
#define RES_MASK 2
#define RES_CLAIM 3
#define RES_WAVES_ON 4
#define WAVES_ON_SIZE 1024
#define RES_RECORDS (RES_WAVES_ON + WAVES_ON_SIZE)
#define RECORD_WORDS 6

__device__ __forceinline__ u32 cu_fmix32(u32 h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ u32 cu_rotl32(u32 x, int r) {
  return (x << r) | (x >> (32 - r));
}

__device__ __forceinline__ u32 cu_base(u32 seed, u32 stage, u32 r) {
  return cu_fmix32(seed ^ ((stage + 1u) * 0x9E3779B9u) ^ (r * 0x7F4A7C15u));
}

__device__ __forceinline__ u32 cu_salt(u32 n) { return (n + 1u) * 0x9E3779B9u; }

__device__ __forceinline__ u32 wave_sum(u32 v) {
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// Mismatch path only (never taken on a healthy GPU): count, lowest bad
// round, stage bits and one log slot; slots past max_records are
// dropped, the count is not.
__device__ __noinline__ void log_mismatch(u32* __restrict__ res, int max_records,
                                          u32 gwave, u32 hw, u32 round, u32 stage,
                                          u32 expected, u32 got) {
  atomicAdd(&res[RES_COUNT], 1u);
  atomicMin(&res[RES_FIRST], round);
  atomicOr(&res[RES_MASK], 1u << stage);
  u32 slot = atomicAdd(&res[RES_CLAIM], 1u);
  if (slot < (u32)max_records) {
    u32* rec = res + RES_RECORDS + (size_t)slot * RECORD_WORDS;
    rec[0] = gwave;
    rec[1] = hw;
    rec[2] = round;
    rec[3] = stage;
    rec[4] = expected;
    rec[5] = got;
  }
}

// bf16 of a signed byte: every integer in [-128, 127] has at most eight
// significant bits, so the top half of its f32 encoding is exact.
__device__ __forceinline__ __bf16 byte_to_bf16(u32 w, int b) {
  float f = (float)(int)(signed char)(w >> (8 * b));
  unsigned short bits = (unsigned short)(__float_as_uint(f) >> 16);
  return __builtin_bit_cast(__bf16, bits);
}

// Fold of a 32x32 accumulator tile.  C/D map of the 32x32 MFMAs: lane l,
// register g holds row (g&3) + 8*(g>>2) + 4*(l>>5), column l&31.
template <typename ACC>
__device__ __forceinline__ u32 fold_tile(const ACC& acc, int lane) {
  u32 col = lane & 31, half = lane >> 5, d = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    u32 row = (g & 3) + 8 * (g >> 2) + 4 * half;
    d += cu_fmix32((u32)(int)acc[g] + cu_salt(32 * row + col));
  }
  return wave_sum(d);
}

__global__ void __launch_bounds__(CU_BLOCK)
cucheck_kernel(u32 seed, u32 rounds, const u32* __restrict__ expected,
               u32* __restrict__ res, int max_records, u32* __restrict__ dump,
               u32 lds_dwords, u32 inj_wave, u32 inj_round, u32 inj_stage,
               u32 inj_mask) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ u32 lds[];
  const int lane = threadIdx.x % WAVE;
  const u32 wib = threadIdx.x / WAVE;
  const u32 gwave = blockIdx.x * CU_WAVES + wib;
  // where the hardware says this wave runs, read once
  const u32 hw_id = __builtin_amdgcn_s_getreg(GETREG_IMMED(32 - 1, 0, HW_ID));
  const u32 xcc = __builtin_amdgcn_s_getreg(
      GETREG_IMMED(XCC_ID_XCC_ID_SIZE - 1, XCC_ID_XCC_ID_OFFSET, XCC_ID));
  const u32 hw = (xcc << 16) | (hw_id & 0xFFFFu);
  if (lane == 0) {
    u32 cu = (hw_id >> 8) & 0xFu, sh = (hw_id >> 12) & 1u, se = (hw_id >> 13) & 3u;
    atomicAdd(&res[RES_WAVES_ON + (((xcc & 7u) << 7) | (se << 5) | (sh << 4) | cu)], 1u);
  }

  // operand maps: lane l owns row l&31 of A and column l&31 of B; the
  // k a fragment slot stands for is the same for A and B, and C = A*B
  // does not change under a permutation of k applied to both
  const u32 rc = lane & 31, half = lane >> 5;
  u32* slice = lds + wib * lds_dwords;

  for (u32 r = 0; r < rounds; ++r) {
    u32 dig[N_STAGES];

    {  // stage 0: int8 matrix core, slot p of step s is k = 32s + 16*half + p
      const u32 base = cu_base(seed, 0, r);
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
      dig[0] = fold_tile(acc, lane);
    }

    {  // stage 1: bf16 matrix core, slot j of step s is k = 16s + 8*half + j
      const u32 base = cu_base(seed, 1, r);
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
      dig[1] = fold_tile(acc, lane);
    }

    {  // stage 2: vector ALU, integer and f32 FMA
      u32 x = cu_fmix32(cu_base(seed, 2, r) + (u32)lane);
      for (int it = 0; it < 32; ++it) {
        x = x * 0x9E3779B1u + cu_rotl32(x, 13);
        x ^= __umulhi(x, 0x85EBCA6Bu);
        x += (u32)__fmaf_rn((float)(x & 0xFFFu), (float)((x >> 12) & 0xFFFu),
                            (float)(x >> 24));
      }
      dig[2] = wave_sum(cu_fmix32(x + (u32)lane));
    }

    {  // stage 3: LDS march over this wave's slice; lane l writes dword
       // 64t + l and reads 64t + 63 - l.  The fences wait for LDS and
       // keep the compiler from moving accesses across them.
      const u32 base = cu_base(seed, 3, r);
      u32 d3 = 0;
      for (u32 inv = 0; inv < 2; ++inv) {
        u32 flip = inv ? 0xFFFFFFFFu : 0u;
        for (u32 t = 0; t < lds_dwords; t += WAVE)
          slice[t + lane] = cu_fmix32(base + t + lane) ^ flip;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (u32 t = 0; t < lds_dwords; t += WAVE) {
          u32 d = t + (WAVE - 1 - lane);
          d3 += cu_fmix32(slice[d] + cu_salt(d));
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
      }
      dig[3] = wave_sum(d3);
    }

    // test hook: one scalar compare per round
    if (gwave == inj_wave && r == inj_round) {
#pragma unroll
      for (u32 st = 0; st < N_STAGES; ++st)
        if (st == inj_stage) dig[st] ^= inj_mask;
    }
    if (lane == 0) {
#pragma unroll
      for (u32 st = 0; st < N_STAGES; ++st) {
        u32 want = expected[r * N_STAGES + st];
        if (dig[st] != want)
          log_mismatch(res, max_records, gwave, hw, r, st, want, dig[st]);
        if (dump != nullptr)
          dump[((size_t)gwave * rounds + r) * N_STAGES + st] = dig[st];
      }
    }
  }
  // keep the workgroup's LDS allocated until all its waves are done
  __syncthreads();
#endif
}

// ---------------------------------------------------------------- host

// global wave, packed hw id, round, stage, expected, got
typedef std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> CuRecord;
typedef std::tuple<int64_t, int64_t, int64_t, std::vector<CuRecord>,
                   std::vector<int64_t>, double> CucheckOut;
typedef std::tuple<int64_t, int64_t, int64_t, int64_t> CuInject;

CucheckOut cucheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                       int64_t blocks_arg, int64_t lds_bytes, int64_t max_records,
                       c10::optional<at::Tensor> dump,
                       c10::optional<CuInject> inject) {
  TORCH_CHECK(rounds >= 1 && rounds <= MAX_ROUNDS, "cucheck: rounds must be in 1..",
              MAX_ROUNDS, ", got ", rounds);
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= MAX_BLOCKS,
              "cucheck: blocks must be in 0..", MAX_BLOCKS, ", got ", blocks_arg);
  TORCH_CHECK(lds_bytes >= LDS_STEP && lds_bytes <= MAX_LDS_BYTES &&
                  lds_bytes % LDS_STEP == 0,
              "cucheck: lds_bytes must be a multiple of ", LDS_STEP, " in ", LDS_STEP,
              "..", MAX_LDS_BYTES, ", got ", lds_bytes);
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT,
              "cucheck: max_records must be in 0..", MAX_RECORDS_LIMIT);
  TORCH_CHECK(seed_arg >= 0 && seed_arg <= 0xFFFFFFFFLL, "cucheck: seed must be a u32");
  TORCH_CHECK(expected.is_cuda(), "cucheck: expected must be on GPU");
  TORCH_CHECK(expected.scalar_type() == at::kInt && expected.is_contiguous(),
              "cucheck: expected must be a contiguous int32 tensor");
  TORCH_CHECK(expected.numel() == rounds * N_STAGES, "cucheck: expected must hold ",
              rounds * N_STAGES, " elements (rounds x 4), got ", expected.numel());

  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  int64_t blocks = blocks_arg;
  if (blocks == 0)
    blocks = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  TORCH_CHECK(blocks >= 1 && blocks <= MAX_BLOCKS, "cucheck: default grid ", blocks,
              " out of range");

  u32* dump_ptr = nullptr;
  if (dump.has_value()) {
    const at::Tensor& d = *dump;
    TORCH_CHECK(d.is_cuda() && d.get_device() == expected.get_device(),
                "cucheck: dump must be on the same GPU as expected");
    TORCH_CHECK(d.scalar_type() == at::kInt && d.is_contiguous(),
                "cucheck: dump must be a contiguous int32 tensor");
    TORCH_CHECK(d.numel() == blocks * CU_WAVES * rounds * N_STAGES,
                "cucheck: dump must hold ", blocks * CU_WAVES * rounds * N_STAGES,
                " elements (waves x rounds x 4), got ", d.numel());
    dump_ptr = (u32*)d.data_ptr();
  }

  u32 inj_wave = NO_INJECT, inj_round = 0, inj_stage = 0, inj_mask = 0;
  if (inject.has_value()) {
    int64_t w = std::get<0>(*inject), r = std::get<1>(*inject);
    int64_t s = std::get<2>(*inject), m = std::get<3>(*inject);
    TORCH_CHECK(w >= 0 && w < blocks * CU_WAVES && r >= 0 && r < rounds && s >= 0 &&
                    s < N_STAGES && m >= 0 && m <= 0xFFFFFFFFLL,
                "cucheck: inject (wave, round, stage, mask) out of range");
    inj_wave = (u32)w;
    inj_round = (u32)r;
    inj_stage = (u32)s;
    inj_mask = (u32)m;
  }

  at::Tensor res = at::zeros({RES_RECORDS + RECORD_WORDS * max_records},
                             expected.options().dtype(at::kInt));
  res.select(0, RES_FIRST).fill_(-1);  // u32 max: identity for atomicMin

  // more than 64 KiB of dynamic LDS has to be asked for
  C10_HIP_CHECK(hipFuncSetAttribute((const void*)cucheck_kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
  auto stream = at::hip::getCurrentHIPStream();
  hipEvent_t t0, t1;
  C10_HIP_CHECK(hipEventCreate(&t0));
  C10_HIP_CHECK(hipEventCreate(&t1));
  C10_HIP_CHECK(hipEventRecord(t0, stream));
  hipLaunchKernelGGL(cucheck_kernel, dim3((unsigned)blocks), dim3(CU_BLOCK),
                     (size_t)lds_bytes, stream, (u32)seed_arg, (u32)rounds,
                     (const u32*)expected.data_ptr(), (u32*)res.data_ptr(),
                     (int)max_records, dump_ptr,
                     (u32)(lds_bytes / 4 / CU_WAVES), inj_wave, inj_round, inj_stage,
                     inj_mask);
  hipError_t launch_err = hipGetLastError();
  (void)hipEventRecord(t1, stream);
  hipError_t sync_err = hipEventSynchronize(t1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  C10_HIP_CHECK(launch_err);
  C10_HIP_CHECK(sync_err);

  at::Tensor host = res.cpu();
  const u32* p = (const u32*)host.data_ptr<int32_t>();
  int64_t claimed = p[RES_CLAIM];
  int64_t n = claimed < max_records ? claimed : max_records;
  std::vector<CuRecord> records;
  records.reserve((size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const u32* rec = p + RES_RECORDS + RECORD_WORDS * i;
    records.emplace_back(rec[0], rec[1], rec[2], rec[3], rec[4], rec[5]);
  }
  std::vector<int64_t> waves_on(p + RES_WAVES_ON, p + RES_WAVES_ON + WAVES_ON_SIZE);
  int64_t count = p[RES_COUNT];
  int64_t first = count ? (int64_t)p[RES_FIRST] : -1;
  return CucheckOut(count, first, (int64_t)p[RES_MASK], std::move(records),
                    std::move(waves_on), (double)ms / 1e3);
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
}
