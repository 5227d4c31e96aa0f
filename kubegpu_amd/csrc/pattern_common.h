// Pattern generation, mismatch accounting and the host side's argument
// checks, result block and family dispatch shared by the integrity
// kernels that stream a buffer: memcheck.hip (HBM) and hostlink.hip
// (host memory over the PCIe link); both files compile into _gpuprobe.
//
// Patterns (v = 64-bit vector index: the caller's first_vector, 0 by
// default, plus the index of a 16 B vector from the buffer's first
// byte; j = 32-bit word inside it, ids 0..5, odd id = ~(even id)):
//   0/1 addr     h = fmix32(lo32(v) ^ hi32(v)*0x9E3779B9 ^ seed)
//                word[j] = rotl32(h, 8j) ^ K[j]
//   2/3 checker  c = v even ? 0xAAAAAAAA : 0x55555555; word[j] = j even ? c : ~c
//   4/5 walk1/0  word[j] = 1 << ((4v + j + seed) mod 32)
// probe/memcheck.py:reference_words is the numpy definition the GPU
// tests compare against.

#pragma once

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <tuple>
#include <type_traits>
#include <vector>

#define WAVE 64
#define BLOCK 256
#define N_PATTERNS 6
#define MAX_BLOCKS (1 << 20)
#define MAX_RECORDS_LIMIT 4096

typedef unsigned int uint4v __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

// Result block in device memory (u64 slots), then max_records records
// of two u64 each: {word index, expected << 32 | got}.
#define RES_COUNT 0
#define RES_FIRST 1
#define RES_MASK 2
#define RES_CLAIM 3
#define RES_HEADER 4

__device__ __forceinline__ unsigned int fmix32(unsigned int h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__device__ __forceinline__ unsigned int rotl32(unsigned int x, int r) {
  return (x << r) | (x >> (32 - r));
}

// FAMILY = pattern id >> 1; inv = all-ones for the odd (complement) id.
template <int FAMILY>
__device__ __forceinline__ uint4v pattern_vec(size_t v, unsigned int seed,
                                              unsigned int inv) {
  uint4v w;
  if (FAMILY == 0) {
    unsigned int lo = (unsigned int)v;
    unsigned int hi = (unsigned int)((u64)v >> 32);
    unsigned int h = fmix32(lo ^ (hi * 0x9E3779B9u) ^ seed);
    w.x = h;
    w.y = rotl32(h, 8) ^ 0x9E3779B9u;
    w.z = rotl32(h, 16) ^ 0x7F4A7C15u;
    w.w = rotl32(h, 24) ^ 0xF39CC060u;
  } else if (FAMILY == 1) {
    unsigned int c = (v & 1) ? 0x55555555u : 0xAAAAAAAAu;
    w.x = c;
    w.y = ~c;
    w.z = c;
    w.w = ~c;
  } else {
    // (4v + j + seed) mod 32: 32 divides 2^32, so u32 wraparound is exact
    unsigned int s = ((unsigned int)v << 2) + seed;
    w.x = 1u << (s & 31u);
    w.y = 1u << ((s + 1u) & 31u);
    w.z = 1u << ((s + 2u) & 31u);
    w.w = 1u << ((s + 3u) & 31u);
  }
  w.x ^= inv;
  w.y ^= inv;
  w.z ^= inv;
  w.w ^= inv;
  return w;
}

// Mismatch path only (never taken on healthy memory): claim a log slot
// per bad word; slots past max_records are dropped, the count is not.
static __device__ __noinline__ void log_mismatch(u64* __restrict__ res, int max_records,
                                                 u64 word_index, unsigned int expected,
                                                 unsigned int got) {
  u64 slot = atomicAdd(&res[RES_CLAIM], 1ULL);
  if (slot < (u64)max_records) {
    res[RES_HEADER + 2 * slot] = word_index;
    res[RES_HEADER + 2 * slot + 1] = ((u64)expected << 32) | (u64)got;
  }
}

struct Tally {
  u64 count;
  u64 first;
  unsigned int mask;
};

__device__ __forceinline__ void check_vec(Tally& t, uint4v got, uint4v exp,
                                          size_t i, u64* __restrict__ res,
                                          int max_records) {
  unsigned int dx = got.x ^ exp.x, dy = got.y ^ exp.y;
  unsigned int dz = got.z ^ exp.z, dw = got.w ^ exp.w;
  if ((dx | dy | dz | dw) != 0u) {
    u64 base = (u64)i * 4ULL;
    // descending j so `first` ends at the lowest bad word of the vector
    if (dw) { t.count++; if (base + 3 < t.first) t.first = base + 3; log_mismatch(res, max_records, base + 3, exp.w, got.w); }
    if (dz) { t.count++; if (base + 2 < t.first) t.first = base + 2; log_mismatch(res, max_records, base + 2, exp.z, got.z); }
    if (dy) { t.count++; if (base + 1 < t.first) t.first = base + 1; log_mismatch(res, max_records, base + 1, exp.y, got.y); }
    if (dx) { t.count++; if (base < t.first) t.first = base; log_mismatch(res, max_records, base, exp.x, got.x); }
    t.mask |= dx | dy | dz | dw;
  }
}

// Per-thread tallies -> wave shuffle reduce -> LDS block reduce -> one
// atomic per block per result (the read_sum_kernel shape).  Holds a
// __syncthreads(): every thread of a workgroup that calls it must.
__device__ __forceinline__ void reduce_tally(Tally t, u64* __restrict__ res) {
  __shared__ u64 sh_count[BLOCK / WAVE];
  __shared__ u64 sh_first[BLOCK / WAVE];
  __shared__ unsigned int sh_mask[BLOCK / WAVE];
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    t.count += __shfl_down(t.count, off, WAVE);
    u64 f = __shfl_down(t.first, off, WAVE);
    t.first = f < t.first ? f : t.first;
    t.mask |= __shfl_down(t.mask, off, WAVE);
  }
  int lane = threadIdx.x % WAVE;
  int wid = threadIdx.x / WAVE;
  if (lane == 0) {
    sh_count[wid] = t.count;
    sh_first[wid] = t.first;
    sh_mask[wid] = t.mask;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 count = 0, first = ~0ULL;
    unsigned int mask = 0;
    for (int w = 0; w < BLOCK / WAVE; ++w) {
      count += sh_count[w];
      first = sh_first[w] < first ? sh_first[w] : first;
      mask |= sh_mask[w];
    }
    atomicAdd(&res[RES_COUNT], count);
    if (count != 0) {
      atomicMin(&res[RES_FIRST], first);
      atomicOr(&res[RES_MASK], (u64)mask);
    }
  }
}

// ---------------------------------------------------------------- host
//
// Argument checks, the grid pick, the result block and the family
// dispatch of both files' entry points.  `who` prefixes the error
// messages ("memcheck" or "hostlink").

typedef std::tuple<int64_t, int64_t, int64_t> Record;  // word, expected, got
typedef std::tuple<int64_t, int64_t, int64_t, std::vector<Record>> VerifyOut;

static inline unsigned int check_seed(const char* who, int64_t seed) {
  TORCH_CHECK(seed >= 0 && seed <= 0xFFFFFFFFLL, who, ": seed must be a u32");
  return (unsigned int)seed;
}

static inline void check_pattern(const char* who, int64_t pattern) {
  TORCH_CHECK(pattern >= 0 && pattern < N_PATTERNS, who, ": pattern id ", pattern,
              " out of range 0..", N_PATTERNS - 1);
}

// first_vector -> the kernels' u64 base.  The binding is int64, and
// first_vector + n4 must not wrap: at most 2^63.
static inline u64 check_first(const char* who, int64_t first_vector, size_t n4,
                              const char* what) {
  TORCH_CHECK(first_vector >= 0, who, ": ", what, " must not be negative, got ",
              first_vector);
  TORCH_CHECK((u64)first_vector + (u64)n4 <= (1ULL << 63), who, ": ", what, " ",
              first_vector, " + ", n4, " vectors exceeds 2^63");
  return (u64)first_vector;
}

static inline void check_blocks(const char* who, int64_t blocks_arg) {
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= MAX_BLOCKS, who,
              ": blocks must be in 0..", MAX_BLOCKS, ", got ", blocks_arg);
}

// A checked blocks argument; 0 = the default grid, cut down to the
// buffer; never less than 1.
static inline unsigned int pick_blocks(int64_t blocks_arg, size_t n4, int dflt) {
  if (blocks_arg > 0) return (unsigned int)blocks_arg;
  return (unsigned int)std::min<size_t>((n4 + BLOCK - 1) / BLOCK, (size_t)dflt);
}

static inline void check_max_records(const char* who, int64_t max_records) {
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT, who,
              ": max_records must be in 0..", MAX_RECORDS_LIMIT);
}

// Zeroed result block for a checked max_records on GPU `device`.
static inline at::Tensor make_result(int device, int64_t max_records) {
  at::Tensor res = at::zeros(
      {RES_HEADER + 2 * max_records},
      at::TensorOptions().dtype(at::kLong).device(at::kCUDA, (c10::DeviceIndex)device));
  res.select(0, RES_FIRST).fill_(-1);  // u64 max: identity for atomicMin
  return res;
}

static inline unsigned int inv_of(int64_t pattern) {
  return (pattern & 1) ? 0xFFFFFFFFu : 0u;
}

// Checked pattern id -> compile-time family: calls f with an
// std::integral_constant, so that f can launch kernel<decltype(c)::value>.
// The one place a pattern id picks a template argument.
template <typename F>
static inline void with_family(int64_t pattern, F&& f) {
  switch (pattern >> 1) {
    case 0: f(std::integral_constant<int, 0>{}); break;
    case 1: f(std::integral_constant<int, 1>{}); break;
    default: f(std::integral_constant<int, 2>{}); break;
  }
}

// Wait for the stream, then unpack a result block (int64 tensor on the
// GPU, RES_HEADER + 2 * max_records slots) into the Python tuple.
static inline VerifyOut read_result(const at::Tensor& res, int64_t max_records,
                                    hipStream_t stream) {
  C10_HIP_CHECK(hipStreamSynchronize(stream));
  at::Tensor host = res.cpu();
  const int64_t* p = host.data_ptr<int64_t>();
  int64_t claimed = p[RES_CLAIM];
  int64_t n = claimed < max_records ? claimed : max_records;
  std::vector<Record> records;
  records.reserve((size_t)n);
  for (int64_t r = 0; r < n; ++r) {
    uint64_t eg = (uint64_t)p[RES_HEADER + 2 * r + 1];
    records.emplace_back(p[RES_HEADER + 2 * r], (int64_t)(eg >> 32),
                         (int64_t)(eg & 0xFFFFFFFFULL));
  }
  return VerifyOut(p[RES_COUNT], p[RES_FIRST], p[RES_MASK], std::move(records));
}
