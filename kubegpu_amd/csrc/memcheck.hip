// memcheck — HBM integrity kernels (gfx950), compiled into _gpuprobe.
//
// Moving-inversions style memory test built on the same streaming shape
// as the bandwidth kernels in gpuprobe.hip: 256-thread blocks, 16 B per
// lane, grid-stride over size_t, nontemporal loads and stores so every
// pass goes through HBM instead of sitting in L2 / the 256 MiB Infinity
// Cache.
//
// Patterns, mismatch accounting and the result block are shared with
// hostlink.hip: pattern_common.h.  probe/memcheck.py:reference_words is
// the numpy definition the GPU tests compare against.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <tuple>
#include <vector>

#include "pattern_common.h"

// Same defaults as gpuprobe.hip: the fill is a pure write stream (640
// workgroups), verify-then-fill uses the copy grid (1024).
#define DEFAULT_COPY_BLOCKS 1024
#define DEFAULT_WRITE_BLOCKS 640
// Measured on MI355X at 1 GiB (profiles/memcheck_bw_mi355x.json), all
// three pattern families alike, beside write 6,190 / read 6,135 / copy
// 5,490 GB/s in the same process: fill peaks at 640 wg (5,544 GB/s vs
// 4,767 at 1024) and verify-then-fill at 1024 (5,443 R+W vs 5,059 at
// 640, 4,792 at 2048), as write and copy do.  Verify alone carries more
// integer work per load than read_sum_kernel and wants more waves in
// flight: a plateau from 1280 to 2048 wg (5,534 / 1536: 5,548 / 1792:
// 5,604 / 5,493) against 5,150 at 1024, 5,155 at 3072, 5,175 at 4096
// and 3,348 at 512; 1536 = 6 wg per CU sits in its middle.
#define VERIFY_BLOCKS 1536

// `first` is the pattern's vector index of the buffer's first vector
// (first_vector).  The loops run over the pattern index v = first + i
// and address the buffer with i = v - first, so every reported word
// index stays relative to the buffer start; first + n4 cannot wrap, the
// host keeps it within 2^63.  Written this way the hot loops keep the
// instruction count they had when v was i: looping over i and adding
// first inside cost the addr fill three more VALU instructions per
// vector and 1.5 % of its bandwidth at 1 GiB
// (profiles/memcheck_first_vector_ab_mi355x.json), and the verify
// loops step their pointer so that i is only needed on a mismatch.
template <int FAMILY>
__global__ void fill_pattern_kernel(uint4v* __restrict__ dst, size_t n4, u64 first,
                                    unsigned int seed, unsigned int inv) {
  u64 v = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u64 end = first + n4;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; v < end; v += stride)
    __builtin_nontemporal_store(pattern_vec<FAMILY>(v, seed, inv), &dst[v - first]);
}

template <int FAMILY>
__global__ void verify_pattern_kernel(const uint4v* __restrict__ src, size_t n4,
                                      u64 first, unsigned int seed, unsigned int inv,
                                      u64* __restrict__ res, int max_records) {
  u64 v = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u64 end = first + n4;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  Tally t = {0, ~0ULL, 0};
  for (src += v - first; v < end; v += stride, src += stride) {
    uint4v got = __builtin_nontemporal_load(src);
    check_vec(t, got, pattern_vec<FAMILY>(v, seed, inv), v - first, res, max_records);
  }
  reduce_tally(t, res);
}

// Fused read-check-write pass (the moving-inversions step): every word
// ends up holding the next pattern whether or not it matched.  Both
// patterns count from the same `first`.
template <int EXPECT_FAMILY, int NEXT_FAMILY>
__global__ void verify_then_fill_kernel(uint4v* __restrict__ buf, size_t n4, u64 first,
                                        unsigned int seed, unsigned int expect_inv,
                                        unsigned int next_inv,
                                        u64* __restrict__ res, int max_records) {
  u64 v = first + (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  u64 end = first + n4;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  Tally t = {0, ~0ULL, 0};
  for (buf += v - first; v < end; v += stride, buf += stride) {
    uint4v got = __builtin_nontemporal_load(buf);
    __builtin_nontemporal_store(pattern_vec<NEXT_FAMILY>(v, seed, next_inv), buf);
    check_vec(t, got, pattern_vec<EXPECT_FAMILY>(v, seed, expect_inv), v - first, res,
              max_records);
  }
  reduce_tally(t, res);
}

// ---------------------------------------------------------------- host

static size_t check_buf(const at::Tensor& buf, int64_t pattern) {
  TORCH_CHECK(buf.is_cuda(), "memcheck: tensor must be on GPU");
  TORCH_CHECK(buf.is_contiguous(), "memcheck: tensor must be contiguous");
  TORCH_CHECK(buf.nbytes() > 0 && buf.nbytes() % 16 == 0,
              "memcheck: nbytes must be a positive multiple of 16, got ",
              buf.nbytes());
  TORCH_CHECK((uintptr_t)buf.data_ptr() % 16 == 0,
              "memcheck: tensor storage must be 16-byte aligned");
  TORCH_CHECK(pattern >= 0 && pattern < N_PATTERNS, "memcheck: pattern id ",
              pattern, " out of range 0..", N_PATTERNS - 1);
  return buf.nbytes() / 16;
}

static int pick_blocks(int64_t blocks_arg, size_t n4, int dflt) {
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= (1 << 20),
              "memcheck: blocks out of range");
  if (blocks_arg > 0) return (int)blocks_arg;
  return (int)std::min<size_t>((n4 + BLOCK - 1) / BLOCK, (size_t)dflt);
}

static unsigned int check_seed(int64_t seed) {
  TORCH_CHECK(seed >= 0 && seed <= 0xFFFFFFFFLL, "memcheck: seed must be a u32");
  return (unsigned int)seed;
}

// first_vector -> the kernels' u64 base.  The binding is int64, and
// first_vector + n4 must not wrap: at most 2^63.
static u64 check_first(int64_t first_vector, size_t n4) {
  TORCH_CHECK(first_vector >= 0, "memcheck: first_vector must not be negative, got ",
              first_vector);
  TORCH_CHECK((u64)first_vector + (u64)n4 <= (1ULL << 63), "memcheck: first_vector ",
              first_vector, " + ", n4, " vectors exceeds 2^63");
  return (u64)first_vector;
}

static at::Tensor make_result(const at::Tensor& buf, int64_t max_records) {
  TORCH_CHECK(max_records >= 0 && max_records <= MAX_RECORDS_LIMIT,
              "memcheck: max_records must be in 0..", MAX_RECORDS_LIMIT);
  at::Tensor res = at::zeros({RES_HEADER + 2 * max_records},
                             buf.options().dtype(at::kLong));
  res.select(0, RES_FIRST).fill_(-1);  // u64 max: identity for atomicMin
  return res;
}

void fill_pattern(at::Tensor buf, int64_t pattern, int64_t seed_arg,
                  int64_t blocks_arg, int64_t first_vector) {
  size_t n4 = check_buf(buf, pattern);
  unsigned int seed = check_seed(seed_arg);
  u64 first = check_first(first_vector, n4);
  int blocks = pick_blocks(blocks_arg, n4, DEFAULT_WRITE_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int inv = (pattern & 1) ? 0xFFFFFFFFu : 0u;
  uint4v* p = (uint4v*)buf.data_ptr();
  switch (pattern >> 1) {
    case 0:
      hipLaunchKernelGGL(fill_pattern_kernel<0>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv);
      break;
    case 1:
      hipLaunchKernelGGL(fill_pattern_kernel<1>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv);
      break;
    default:
      hipLaunchKernelGGL(fill_pattern_kernel<2>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv);
      break;
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

VerifyOut verify_pattern(at::Tensor buf, int64_t pattern, int64_t seed_arg,
                         int64_t max_records, int64_t blocks_arg,
                         int64_t first_vector) {
  size_t n4 = check_buf(buf, pattern);
  unsigned int seed = check_seed(seed_arg);
  u64 first = check_first(first_vector, n4);
  int blocks = pick_blocks(blocks_arg, n4, VERIFY_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  at::Tensor res = make_result(buf, max_records);
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int inv =(pattern & 1) ? 0xFFFFFFFFu : 0u;
  const uint4v* p = (const uint4v*)buf.data_ptr();
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  switch (pattern >> 1) {
    case 0:
      hipLaunchKernelGGL(verify_pattern_kernel<0>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv, r, mr);
      break;
    case 1:
      hipLaunchKernelGGL(verify_pattern_kernel<1>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv, r, mr);
      break;
    default:
      hipLaunchKernelGGL(verify_pattern_kernel<2>, dim3(blocks), dim3(BLOCK), 0,
                         stream, p, n4, first, seed, inv, r, mr);
      break;
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

#define VTF_LAUNCH(E, N)                                                       \
  hipLaunchKernelGGL((verify_then_fill_kernel<E, N>), dim3(blocks), dim3(BLOCK), \
                     0, stream, p, n4, first, seed, einv, ninv, r, mr)
#define VTF_NEXT(E)                 \
  switch (next_pattern >> 1) {      \
    case 0: VTF_LAUNCH(E, 0); break; \
    case 1: VTF_LAUNCH(E, 1); break; \
    default: VTF_LAUNCH(E, 2); break; \
  }

VerifyOut verify_then_fill(at::Tensor buf, int64_t expect_pattern,
                           int64_t next_pattern, int64_t seed_arg,
                           int64_t max_records, int64_t blocks_arg,
                           int64_t first_vector) {
  size_t n4 = check_buf(buf, expect_pattern);
  TORCH_CHECK(next_pattern >= 0 && next_pattern < N_PATTERNS,
              "memcheck: pattern id ", next_pattern, " out of range 0..",
              N_PATTERNS - 1);
  unsigned int seed = check_seed(seed_arg);
  u64 first = check_first(first_vector, n4);
  int blocks = pick_blocks(blocks_arg, n4, DEFAULT_COPY_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  at::Tensor res = make_result(buf, max_records);
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int einv = (expect_pattern & 1) ? 0xFFFFFFFFu : 0u;
  unsigned int ninv = (next_pattern & 1) ? 0xFFFFFFFFu : 0u;
  uint4v* p = (uint4v*)buf.data_ptr();
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  switch (expect_pattern >> 1) {
    case 0: VTF_NEXT(0); break;
    case 1: VTF_NEXT(1); break;
    default: VTF_NEXT(2); break;
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

#undef VTF_NEXT
#undef VTF_LAUNCH

// Called from gpuprobe.hip's PYBIND11_MODULE. The GIL is released for
// the same reason as the timed probes: a pass over a large buffer plus
// the stream synchronise must not starve the agent's gRPC threads.
void bind_memcheck(py::module_& m) {
  m.def("fill_pattern", &fill_pattern, "NT fill with a memcheck pattern",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("buf"), py::arg("pattern"), py::arg("seed"),
        py::arg("blocks") = 0, py::arg("first_vector") = 0);
  m.def("verify_pattern", &verify_pattern,
        "verify a memcheck pattern -> (mismatched_words, first_bad_word, "
        "bad_bits_mask, records)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("buf"), py::arg("pattern"), py::arg("seed"),
        py::arg("max_records") = 16, py::arg("blocks") = 0,
        py::arg("first_vector") = 0);
  m.def("verify_then_fill", &verify_then_fill,
        "fused verify(expect_pattern) + fill(next_pattern) pass",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("buf"), py::arg("expect_pattern"), py::arg("next_pattern"),
        py::arg("seed"), py::arg("max_records") = 16, py::arg("blocks") = 0,
        py::arg("first_vector") = 0);
}
