// Hashing, digest folding, the kernels' argument block, the per-round
// compare, mismatch accounting, argument checks, the timed launch and the
// single-wave value launch shared by the integrity kernels that run one
// 16-wave workgroup per compute unit; all seven files compile into
// _gpuprobe and add only their stages, a fold / dump pair of sinks for
// the stages' values and their own kernel arguments:
//   cucheck.hip    i8 / bf16 matrix cores, VALU, LDS (lds_dwords)
//   mxcheck.hip    f16 / fp8 / MXFP4 / f64 matrix cores
//   fpcheck.hip    IEEE rounding of the vector FP units
//   atomcheck.hip  LDS, L2 and memory-side atomics (arena, shared, drop)
//   lanecheck.hip  the cross-lane data paths
//   ldscheck.hip   the LDS array and its access paths (tables)
//   vmemcheck.hip  the vector-memory and cache paths (arena, table)
//
// Every wave compares N_STAGES 32-bit digests per round with a table the
// host computed in numpy.  Inputs are word(stage, r, idx) =
// fmix32(base(seed, stage, r) + idx); the probe/<name>.py of each kernel
// holds the numpy definition.

#pragma once

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
typedef float f32x16 __attribute__((ext_vector_type(16)));

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

__device__ __forceinline__ u32 cu_base(u32 seed, u32 stage, u32 r) {
  return cu_fmix32(seed ^ ((stage + 1u) * 0x9E3779B9u) ^ (r * 0x7F4A7C15u));
}

__device__ __forceinline__ u32 cu_salt(u32 n) { return (n + 1u) * 0x9E3779B9u; }

__device__ __forceinline__ u32 wave_sum(u32 v) {
  for (int off = WAVE / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, WAVE);
  return v;
}

// What every digest kernel takes first, by value (cu_prepare fills it);
// its own arguments follow.  inj_*: the test hook of cu_check_round.
struct CuArgs {
  u32 seed, rounds;
  const u32* expected;  // [rounds, N_STAGES]
  u32* res;             // the result block above
  int max_records;
  u32* dump;  // [waves, rounds, N_STAGES] or null
  u32 inj_wave, inj_round, inj_stage, inj_mask;
};

// Where the hardware says this wave runs, read once: xcc<<16 |
// HW_ID[15:0].  Lane 0 counts the wave in the per-CU table.
__device__ __forceinline__ u32 cu_locate_wave(u32* __restrict__ res, int lane) {
#if __HIP_DEVICE_COMPILE__
  const u32 hw_id = __builtin_amdgcn_s_getreg(GETREG_IMMED(32 - 1, 0, HW_ID));
  const u32 xcc = __builtin_amdgcn_s_getreg(
      GETREG_IMMED(XCC_ID_XCC_ID_SIZE - 1, XCC_ID_XCC_ID_OFFSET, XCC_ID));
  if (lane == 0) {
    u32 cu = (hw_id >> 8) & 0xFu, sh = (hw_id >> 12) & 1u, se = (hw_id >> 13) & 3u;
    atomicAdd(&res[RES_WAVES_ON + (((xcc & 7u) << 7) | (se << 5) | (sh << 4) | cu)], 1u);
  }
  return (xcc << 16) | (hw_id & 0xFFFFu);
#else
  return 0;
#endif
}

// Every kernel opens with this: lane, wave of the grid, where it runs.
struct CuWave {
  int lane;
  u32 gwave, hw;
};

__device__ __forceinline__ CuWave cu_wave(const CuArgs& a) {
  const int lane = threadIdx.x % WAVE;
  return {lane, blockIdx.x * CU_WAVES + threadIdx.x / WAVE, cu_locate_wave(a.res, lane)};
}

// Mismatch path only (never taken on a healthy GPU): count, lowest bad
// round, stage bits and one log slot; slots past max_records are
// dropped, the count is not.
static __device__ __noinline__ void log_mismatch(u32* __restrict__ res, int max_records,
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

// End of a round, the same in every kernel: the test hook (one scalar
// compare per round), then lane 0 compares the wave's digests with the
// table, logs what differs and writes the dump if there is one.  The
// hook works on a copy of the digests: on values the compiler keeps it
// to four selects, through the caller's array it builds a branch tree
// and allocates the kernel's registers differently.
__device__ __forceinline__ void cu_check_round(const u32 (&digests)[N_STAGES], u32 r,
                                               const CuWave& w, const CuArgs& a) {
  u32 dig[N_STAGES];
#pragma unroll
  for (u32 st = 0; st < N_STAGES; ++st) dig[st] = digests[st];
  if (w.gwave == a.inj_wave && r == a.inj_round) {
#pragma unroll
    for (u32 st = 0; st < N_STAGES; ++st)
      if (st == a.inj_stage) dig[st] ^= a.inj_mask;
  }
  if (w.lane == 0) {
#pragma unroll
    for (u32 st = 0; st < N_STAGES; ++st) {
      u32 want = a.expected[r * N_STAGES + st];
      if (dig[st] != want)
        log_mismatch(a.res, a.max_records, w.gwave, w.hw, r, st, want, dig[st]);
      if (a.dump != nullptr)
        a.dump[((size_t)w.gwave * a.rounds + r) * N_STAGES + st] = dig[st];
    }
  }
}

// C/D map of the 32x32 MFMAs: lane l, register g holds row
// (g&3) + 8*(g>>2) + 4*(l>>5), column l&31.  Row-major index of that
// element; the fold and cucheck's element dump both go through it.
__device__ __forceinline__ u32 cu_tile_index(int g, int lane) {
  u32 col = lane & 31, half = lane >> 5;
  u32 row = (g & 3) + 8 * (g >> 2) + 4 * half;
  return 32 * row + col;
}

// Fold of a 32x32 accumulator tile.
template <typename ACC>
__device__ __forceinline__ u32 fold_tile(const ACC& acc, int lane) {
  u32 d = 0;
#pragma unroll
  for (int g = 0; g < 16; ++g)
    d += cu_fmix32((u32)(int)acc[g] + cu_salt(cu_tile_index(g, lane)));
  return wave_sum(d);
}

// ---------------------------------------------------------------- host

// global wave, packed hw id, round, stage, expected, got
typedef std::tuple<int64_t, int64_t, int64_t, int64_t, int64_t, int64_t> CuRecord;
typedef std::tuple<int64_t, int64_t, int64_t, std::vector<CuRecord>,
                   std::vector<int64_t>, double> CucheckOut;
typedef std::tuple<int64_t, int64_t, int64_t, int64_t> CuInject;

// What a launch needs, after the argument checks; `res` owns args.res.
struct CuLaunch {
  int64_t blocks;
  CuArgs args;
  at::Tensor res;
};

// Argument checks of a run, the default grid (one workgroup per CU) and
// a zeroed result block.  `who` prefixes the error messages.
static inline CuLaunch cu_prepare(const char* who, const at::Tensor& expected,
                                  int64_t seed_arg, int64_t rounds, int64_t blocks_arg,
                                  int64_t max_records,
                                  const c10::optional<at::Tensor>& dump,
                                  const c10::optional<CuInject>& inject) {
  TORCH_CHECK(rounds >= 1 && rounds <= MAX_ROUNDS, who, ": rounds must be in 1..",
              MAX_ROUNDS, ", got ", rounds);
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= MAX_BLOCKS, who,
              ": blocks must be in 0..", MAX_BLOCKS, ", got ", blocks_arg);
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT, who,
              ": max_records must be in 0..", MAX_RECORDS_LIMIT);
  TORCH_CHECK(seed_arg >= 0 && seed_arg <= 0xFFFFFFFFLL, who, ": seed must be a u32");
  TORCH_CHECK(expected.is_cuda(), who, ": expected must be on GPU");
  TORCH_CHECK(expected.scalar_type() == at::kInt && expected.is_contiguous(), who,
              ": expected must be a contiguous int32 tensor");
  TORCH_CHECK(expected.numel() == rounds * N_STAGES, who, ": expected must hold ",
              rounds * N_STAGES, " elements (rounds x 4), got ", expected.numel());

  // the caller sets its own guard for the launch once this has returned
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  CuLaunch l;
  l.blocks = blocks_arg;
  if (l.blocks == 0)
    l.blocks = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  TORCH_CHECK(l.blocks >= 1 && l.blocks <= MAX_BLOCKS, who, ": default grid ", l.blocks,
              " out of range");

  CuArgs& a = l.args;  // no dump, no injection; res is set last
  a = {(u32)seed_arg, (u32)rounds, (const u32*)expected.data_ptr(), nullptr,
       (int)max_records, nullptr, NO_INJECT, 0, 0, 0};
  if (dump.has_value()) {
    const at::Tensor& d = *dump;
    TORCH_CHECK(d.is_cuda() && d.get_device() == expected.get_device(), who,
                ": dump must be on the same GPU as expected");
    TORCH_CHECK(d.scalar_type() == at::kInt && d.is_contiguous(), who,
                ": dump must be a contiguous int32 tensor");
    TORCH_CHECK(d.numel() == l.blocks * CU_WAVES * rounds * N_STAGES, who,
                ": dump must hold ", l.blocks * CU_WAVES * rounds * N_STAGES,
                " elements (waves x rounds x 4), got ", d.numel());
    a.dump = (u32*)d.data_ptr();
  }

  if (inject.has_value()) {
    int64_t w = std::get<0>(*inject), r = std::get<1>(*inject);
    int64_t s = std::get<2>(*inject), m = std::get<3>(*inject);
    TORCH_CHECK(w >= 0 && w < l.blocks * CU_WAVES && r >= 0 && r < rounds && s >= 0 &&
                    s < N_STAGES && m >= 0 && m <= 0xFFFFFFFFLL,
                who, ": inject (wave, round, stage, mask) out of range");
    a.inj_wave = (u32)w;
    a.inj_round = (u32)r;
    a.inj_stage = (u32)s;
    a.inj_mask = (u32)m;
  }

  l.res = at::zeros({RES_RECORDS + RECORD_WORDS * max_records},
                    expected.options().dtype(at::kInt));
  l.res.select(0, RES_FIRST).fill_(-1);  // u32 max: identity for atomicMin
  a.res = (u32*)l.res.data_ptr();
  return l;
}

// Unpack a result block (after the stream was waited for) into the
// Python tuple.
static inline CucheckOut cu_read_result(const at::Tensor& res, int64_t max_records,
                                        double elapsed_s) {
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
                    std::move(waves_on), elapsed_s);
}

// One timed launch of a digest kernel on the current stream, after
// cu_prepare and under the caller's device guard: the kernel gets l's
// argument block, then `extras`, its own.  The events are destroyed
// before either error is raised.
template <typename Kernel, typename... Extras>
static inline CucheckOut cu_launch_timed(Kernel kernel, const CuLaunch& l,
                                         int64_t lds_bytes, Extras... extras) {
  // more than 64 KiB of dynamic LDS has to be asked for; a kernel that
  // never touches it asks only to keep a second workgroup off the CU
  C10_HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                    hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)lds_bytes));
  auto stream = at::hip::getCurrentHIPStream();
  hipEvent_t t0, t1;
  C10_HIP_CHECK(hipEventCreate(&t0));
  C10_HIP_CHECK(hipEventCreate(&t1));
  C10_HIP_CHECK(hipEventRecord(t0, stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)l.blocks), dim3(CU_BLOCK), (size_t)lds_bytes,
                     stream, l.args, extras...);
  hipError_t launch_err = hipGetLastError();
  (void)hipEventRecord(t1, stream);
  hipError_t sync_err = hipEventSynchronize(t1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  C10_HIP_CHECK(launch_err);
  C10_HIP_CHECK(sync_err);
  return cu_read_result(l.res, l.args.max_records, (double)ms / 1e3);
}

// Argument checks of the single-wave launchers (<name>_values,
// mxcheck_tile).
static inline void cu_check_wave_args(const char* who, int64_t seed_arg, int64_t stage,
                                      int64_t round) {
  TORCH_CHECK(seed_arg >= 0 && seed_arg <= 0xFFFFFFFFLL, who, ": seed must be a u32");
  TORCH_CHECK(stage >= 0 && stage < N_STAGES, who, ": stage must be in 0..", N_STAGES - 1,
              ", got ", stage);
  TORCH_CHECK(round >= 0 && round < MAX_ROUNDS, who, ": round must be in 0..",
              MAX_ROUNDS - 1, ", got ", round);
}

// The launch of a single-wave launcher, after its argument checks: one
// workgroup of `block_threads` on the current stream with the kernel's
// `args`, waited for; returns `out`, which the kernel has filled.
template <typename Kernel, typename... Args>
static inline at::Tensor cu_launch_values(Kernel kernel, int block_threads,
                                          int64_t lds_bytes, at::Tensor out, Args... args) {
  if (lds_bytes > 64 * 1024)  // more than that has to be asked for
    C10_HIP_CHECK(hipFuncSetAttribute((const void*)kernel,
                                      hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)lds_bytes));
  auto stream = at::hip::getCurrentHIPStream();
  hipLaunchKernelGGL(kernel, dim3(1), dim3(block_threads), (size_t)lds_bytes, stream,
                     args...);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  C10_HIP_CHECK(hipStreamSynchronize(stream));
  return out;
}
