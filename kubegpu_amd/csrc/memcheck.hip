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

static size_t check_buf(const at::Tensor& buf) {
  TORCH_CHECK(buf.is_cuda(), "memcheck: tensor must be on GPU");
  TORCH_CHECK(buf.is_contiguous(), "memcheck: tensor must be contiguous");
  TORCH_CHECK(buf.nbytes() > 0 && buf.nbytes() % 16 == 0,
              "memcheck: nbytes must be a positive multiple of 16, got ",
              buf.nbytes());
  TORCH_CHECK((uintptr_t)buf.data_ptr() % 16 == 0,
              "memcheck: tensor storage must be 16-byte aligned");
  return buf.nbytes() / 16;
}

static const char* const WHO = "memcheck";

void fill_pattern(at::Tensor buf, int64_t pattern, int64_t seed_arg,
                  int64_t blocks_arg, int64_t first_vector) {
  size_t n4 = check_buf(buf);
  check_pattern(WHO, pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  u64 first = check_first(WHO, first_vector, n4, "first_vector");
  check_blocks(WHO, blocks_arg);
  unsigned int blocks = pick_blocks(blocks_arg, n4, DEFAULT_WRITE_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int inv = inv_of(pattern);
  uint4v* p = (uint4v*)buf.data_ptr();
  with_family(pattern, [&](auto f) {
    hipLaunchKernelGGL(fill_pattern_kernel<decltype(f)::value>, dim3(blocks),
                       dim3(BLOCK), 0, stream, p, n4, first, seed, inv);
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

VerifyOut verify_pattern(at::Tensor buf, int64_t pattern, int64_t seed_arg,
                         int64_t max_records, int64_t blocks_arg,
                         int64_t first_vector) {
  size_t n4 = check_buf(buf);
  check_pattern(WHO, pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  u64 first = check_first(WHO, first_vector, n4, "first_vector");
  check_blocks(WHO, blocks_arg);
  unsigned int blocks = pick_blocks(blocks_arg, n4, VERIFY_BLOCKS);
  check_max_records(WHO, max_records);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  at::Tensor res = make_result(buf.get_device(), max_records);
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int inv = inv_of(pattern);
  const uint4v* p = (const uint4v*)buf.data_ptr();
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  with_family(pattern, [&](auto f) {
    hipLaunchKernelGGL(verify_pattern_kernel<decltype(f)::value>, dim3(blocks),
                       dim3(BLOCK), 0, stream, p, n4, first, seed, inv, r, mr);
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

VerifyOut verify_then_fill(at::Tensor buf, int64_t expect_pattern,
                           int64_t next_pattern, int64_t seed_arg,
                           int64_t max_records, int64_t blocks_arg,
                           int64_t first_vector) {
  size_t n4 = check_buf(buf);
  check_pattern(WHO, expect_pattern);
  check_pattern(WHO, next_pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  u64 first = check_first(WHO, first_vector, n4, "first_vector");
  check_blocks(WHO, blocks_arg);
  unsigned int blocks = pick_blocks(blocks_arg, n4, DEFAULT_COPY_BLOCKS);
  check_max_records(WHO, max_records);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(buf));
  at::Tensor res = make_result(buf.get_device(), max_records);
  auto stream = at::hip::getCurrentHIPStream();
  unsigned int einv = inv_of(expect_pattern), ninv = inv_of(next_pattern);
  uint4v* p = (uint4v*)buf.data_ptr();
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  with_family(expect_pattern, [&](auto e) {
    with_family(next_pattern, [&](auto n) {
      hipLaunchKernelGGL((verify_then_fill_kernel<decltype(e)::value, decltype(n)::value>),
                         dim3(blocks), dim3(BLOCK), 0, stream, p, n4, first, seed, einv,
                         ninv, r, mr);
    });
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

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
