// hostlink — host-link integrity kernels (gfx950), compiled into _gpuprobe.
//
// The memcheck patterns (pattern_common.h) streamed between the GPU and
// pinned host memory, so that every access is a transaction on the PCIe
// link rather than an HBM or L2 access: the GPU stores a pattern into
// host memory (device-to-host traffic), loads and verifies host memory
// (host-to-device traffic), or does both at once from one launch
// (duplex), which is the only way to be sure that both directions of
// the full-duplex link carry traffic at the same time.
//
// Access shape as in memcheck.hip: 256-thread workgroups, 16 B per
// lane, so a wave touches 1 KiB of contiguous memory per instruction
// and stores reach the host as whole lines; grid-stride over size_t;
// nontemporal loads and stores.  The buffer hostlink_alloc() returns is
// fine-grained (coherent) memory, which the GPU does not cache.
//
// These kernels dereference host pointers.  Without XNACK a GPU access
// to pageable memory is a fault, not a page-in, so every entry point
// proves on the host that the whole range is pinned (check_host) before
// anything is launched.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "pattern_common.h"

// Workgroups per direction when the caller passes 0: the smallest grid
// within 2 % of the best of its sweep over 8..1024 workgroups, measured
// on MI355X at 256 MiB over a Gen5 x16 link, 5 timed launches each
// (tools/hostlink_sweep.py -> profiles/hostlink_mi355x.json).
// Loads need enough waves to cover the link's round trip: verify
// reaches 25.1 GB/s at 8 workgroups, 48.4 at 16 and 56.7 at 32, then
// stays between 56.8 and 57.1 up to 512 (55.2 at 1024).
#define DEFAULT_READ_BLOCKS 32
// Stores are posted and saturate at once: fill is flat, 54.9 GB/s at 8
// workgroups down to 52.8-53.1 from 64 to 1024 (same file).  The duplex
// kernel with these two defaults (32 readers + 8 writers) moves 73.2
// GB/s, against 38.4 for 8 + 8, 76.9 for 64 + 64 and 82.2 for 1024 +
// 1024 in that file's duplex sweep.
#define DEFAULT_WRITE_BLOCKS 8

// Grid-stride bodies over one role's own buffer with its own block
// count: `block` of `nblocks` (the launch's for the single-role
// kernels, the role's share of it for the duplex kernel).  `first` is
// the pattern's vector index of the buffer's first vector: the pattern
// is generated for first + i, the buffer is addressed with i, and every
// reported word index stays relative to the buffer start.
template <int FAMILY>
__device__ __forceinline__ void fill_host(uint4v* __restrict__ dst, size_t n4, u64 first,
                                          unsigned int seed, unsigned int inv,
                                          size_t block, size_t nblocks) {
  size_t i = block * BLOCK + threadIdx.x;
  size_t stride = nblocks * BLOCK;
  for (; i < n4; i += stride)
    __builtin_nontemporal_store(pattern_vec<FAMILY>(first + i, seed, inv), &dst[i]);
}

template <int FAMILY>
__device__ __forceinline__ void verify_host(const uint4v* __restrict__ src, size_t n4,
                                            u64 first, unsigned int seed, unsigned int inv,
                                            size_t block, size_t nblocks,
                                            u64* __restrict__ res, int max_records) {
  size_t i = block * BLOCK + threadIdx.x;
  size_t stride = nblocks * BLOCK;
  Tally t = {0, ~0ULL, 0};
  for (; i < n4; i += stride) {
    uint4v got = __builtin_nontemporal_load(&src[i]);
    check_vec(t, got, pattern_vec<FAMILY>(first + i, seed, inv), i, res, max_records);
  }
  reduce_tally(t, res);
}

template <int FAMILY>
__global__ void hostlink_fill_kernel(uint4v* __restrict__ dst, size_t n4, u64 first,
                                     unsigned int seed, unsigned int inv) {
  fill_host<FAMILY>(dst, n4, first, seed, inv, blockIdx.x, gridDim.x);
}

template <int FAMILY>
__global__ void hostlink_verify_kernel(const uint4v* __restrict__ src, size_t n4,
                                       u64 first, unsigned int seed, unsigned int inv,
                                       u64* __restrict__ res, int max_records) {
  verify_host<FAMILY>(src, n4, first, seed, inv, blockIdx.x, gridDim.x, res, max_records);
}

// One launch, two roles.  The role depends on blockIdx.x alone, so it is
// uniform over a workgroup: the first read_blocks workgroups verify src,
// the others fill dst.  The only __syncthreads() is inside reduce_tally,
// on the reader path, where every thread of a reader workgroup reaches
// it; the writer path holds no barrier and touches neither LDS nor res.
template <int READ_FAMILY, int WRITE_FAMILY>
__global__ void hostlink_duplex_kernel(const uint4v* __restrict__ src, size_t read_n4,
                                       u64 read_first, unsigned int read_inv,
                                       uint4v* __restrict__ dst, size_t write_n4,
                                       u64 write_first, unsigned int write_inv,
                                       unsigned int seed,
                                       unsigned int read_blocks,
                                       u64* __restrict__ res, int max_records) {
  if (blockIdx.x < read_blocks) {
    verify_host<READ_FAMILY>(src, read_n4, read_first, seed, read_inv, blockIdx.x,
                             read_blocks, res, max_records);
  } else {
    fill_host<WRITE_FAMILY>(dst, write_n4, write_first, seed, write_inv,
                            blockIdx.x - read_blocks, gridDim.x - read_blocks);
  }
}

// ---------------------------------------------------------------- host

static int check_device(int64_t device) {
  int count = 0;
  C10_HIP_CHECK(hipGetDeviceCount(&count));
  TORCH_CHECK(device >= 0 && device < count, "hostlink: device index ", device,
              " out of range 0..", count - 1);
  return (int)device;
}

static bool is_pinned_byte(const void* p) {
  hipPointerAttribute_t attr;
  hipError_t err = hipPointerGetAttributes(&attr, p);
  if (err != hipSuccess) {
    (void)hipGetLastError();  // an unknown pointer is an answer, not a sticky error
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// Everything that must hold before a kernel may dereference the tensor;
// returns the address the GPU uses for its first byte.  The device must
// be current.
static uint4v* check_host(const at::Tensor& host, const char* what) {
  TORCH_CHECK(host.device().is_cpu(), "hostlink: ", what, " must be a CPU tensor");
  TORCH_CHECK(host.is_contiguous(), "hostlink: ", what, " must be contiguous");
  TORCH_CHECK(host.nbytes() > 0 && host.nbytes() % 16 == 0, "hostlink: ", what,
              " nbytes must be a positive multiple of 16, got ", host.nbytes());
  char* p = (char*)host.data_ptr();
  TORCH_CHECK((uintptr_t)p % 16 == 0, "hostlink: ", what,
              " storage must be 16-byte aligned");
  TORCH_CHECK(is_pinned_byte(p) && is_pinned_byte(p + host.nbytes() - 1),
              "hostlink: ", what, " is not pinned host memory (hipMemoryTypeHost) "
              "from its first to its last byte; a kernel must not touch pageable "
              "memory");
  void* dev = nullptr;
  hipError_t err = hipHostGetDevicePointer(&dev, p, 0);
  if (err != hipSuccess) (void)hipGetLastError();
  TORCH_CHECK(err == hipSuccess && dev != nullptr, "hostlink: ", what,
              " has no device mapping: ", hipGetErrorString(err));
  return (uint4v*)dev;
}

static const char* const WHO = "hostlink";

// Pinned, mapped, fine-grained host memory as a CPU uint8 tensor.  The
// coherent flag is explicit: the runtime's default depends on an
// environment variable, and only fine-grained memory makes every GPU
// access a link transaction instead of a possible L2 hit.
at::Tensor hostlink_alloc(int64_t nbytes, int64_t device_arg) {
  TORCH_CHECK(nbytes > 0, "hostlink: nbytes must be positive, got ", nbytes);
  int device = check_device(device_arg);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      at::Device(at::kCUDA, (c10::DeviceIndex)device));
  void* p = nullptr;
  hipError_t err = hipHostMalloc(
      &p, (size_t)nbytes,
      hipHostMallocPortable | hipHostMallocMapped | hipHostMallocCoherent);
  if (err != hipSuccess) (void)hipGetLastError();
  TORCH_CHECK(err == hipSuccess && p != nullptr, "hostlink: hipHostMalloc of ", nbytes,
              " bytes failed: ", hipGetErrorString(err));
  return at::from_blob(
      p, {nbytes}, [](void* q) { (void)hipHostFree(q); },
      at::TensorOptions().dtype(at::kByte).device(at::kCPU));
}

// The stream is synchronised before returning: the CPU reads the buffer
// next, and a pinned tensor released while the kernel still wrote to it
// could be handed to someone else.
void hostlink_fill(at::Tensor host, int64_t pattern, int64_t seed_arg,
                   int64_t device_arg, int64_t blocks_arg, int64_t first_vector) {
  check_pattern(WHO, pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  check_blocks(WHO, blocks_arg);
  int device = check_device(device_arg);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      at::Device(at::kCUDA, (c10::DeviceIndex)device));
  uint4v* p = check_host(host, "host");
  size_t n4 = host.nbytes() / 16;
  u64 first = check_first(WHO, first_vector, n4, "first_vector");
  unsigned int blocks = pick_blocks(blocks_arg, n4, DEFAULT_WRITE_BLOCKS);
  unsigned int inv = inv_of(pattern);
  hipStream_t stream = at::hip::getCurrentHIPStream((c10::DeviceIndex)device);
  with_family(pattern, [&](auto f) {
    hipLaunchKernelGGL(hostlink_fill_kernel<decltype(f)::value>, dim3(blocks),
                       dim3(BLOCK), 0, stream, p, n4, first, seed, inv);
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  C10_HIP_CHECK(hipStreamSynchronize(stream));
}

VerifyOut hostlink_verify(at::Tensor host, int64_t pattern, int64_t seed_arg,
                          int64_t device_arg, int64_t max_records,
                          int64_t blocks_arg, int64_t first_vector) {
  check_pattern(WHO, pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  check_blocks(WHO, blocks_arg);
  check_max_records(WHO, max_records);
  int device = check_device(device_arg);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      at::Device(at::kCUDA, (c10::DeviceIndex)device));
  const uint4v* p = check_host(host, "host");
  size_t n4 = host.nbytes() / 16;
  u64 first = check_first(WHO, first_vector, n4, "first_vector");
  unsigned int blocks = pick_blocks(blocks_arg, n4, DEFAULT_READ_BLOCKS);
  unsigned int inv = inv_of(pattern);
  at::Tensor res = make_result(device, max_records);
  hipStream_t stream = at::hip::getCurrentHIPStream((c10::DeviceIndex)device);
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  with_family(pattern, [&](auto f) {
    hipLaunchKernelGGL(hostlink_verify_kernel<decltype(f)::value>, dim3(blocks),
                       dim3(BLOCK), 0, stream, p, n4, first, seed, inv, r, mr);
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

VerifyOut hostlink_duplex(at::Tensor read_host, int64_t read_pattern,
                          at::Tensor write_host, int64_t write_pattern,
                          int64_t seed_arg, int64_t device_arg, int64_t max_records,
                          int64_t read_blocks_arg, int64_t write_blocks_arg,
                          int64_t read_first_vector, int64_t write_first_vector) {
  check_pattern(WHO, read_pattern);
  check_pattern(WHO, write_pattern);
  unsigned int seed = check_seed(WHO, seed_arg);
  check_blocks(WHO, read_blocks_arg);
  check_blocks(WHO, write_blocks_arg);
  check_max_records(WHO, max_records);
  int device = check_device(device_arg);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(
      at::Device(at::kCUDA, (c10::DeviceIndex)device));
  const uint4v* rp = check_host(read_host, "read_host");
  uint4v* wp = check_host(write_host, "write_host");
  uintptr_t ra = (uintptr_t)read_host.data_ptr(), wa = (uintptr_t)write_host.data_ptr();
  TORCH_CHECK(ra + read_host.nbytes() <= wa || wa + write_host.nbytes() <= ra,
              "hostlink: read_host and write_host overlap");
  size_t rn4 = read_host.nbytes() / 16, wn4 = write_host.nbytes() / 16;
  u64 rfirst = check_first(WHO, read_first_vector, rn4, "read_first_vector");
  u64 wfirst = check_first(WHO, write_first_vector, wn4, "write_first_vector");
  unsigned int rblocks = pick_blocks(read_blocks_arg, rn4, DEFAULT_READ_BLOCKS);
  unsigned int wblocks = pick_blocks(write_blocks_arg, wn4, DEFAULT_WRITE_BLOCKS);
  unsigned int rinv = inv_of(read_pattern), winv = inv_of(write_pattern);
  at::Tensor res = make_result(device, max_records);
  hipStream_t stream = at::hip::getCurrentHIPStream((c10::DeviceIndex)device);
  u64* r = (u64*)res.data_ptr();
  int mr = (int)max_records;
  with_family(read_pattern, [&](auto rf) {
    with_family(write_pattern, [&](auto wf) {
      hipLaunchKernelGGL(
          (hostlink_duplex_kernel<decltype(rf)::value, decltype(wf)::value>),
          dim3(rblocks + wblocks), dim3(BLOCK), 0, stream, rp, rn4, rfirst, rinv, wp, wn4,
          wfirst, winv, seed, rblocks, r, mr);
    });
  });
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return read_result(res, max_records, stream);
}

// Called from gpuprobe.hip's PYBIND11_MODULE.  The GIL is released as
// for the other probes: a pass over the link plus the stream synchronise
// must not starve the agent's gRPC threads.
void bind_hostlink(py::module_& m) {
  m.attr("HOSTLINK_DEFAULT_READ_BLOCKS") = py::int_(DEFAULT_READ_BLOCKS);
  m.attr("HOSTLINK_DEFAULT_WRITE_BLOCKS") = py::int_(DEFAULT_WRITE_BLOCKS);
  m.def("hostlink_alloc", &hostlink_alloc,
        "pinned, mapped, fine-grained host memory as a CPU uint8 tensor",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("nbytes"), py::arg("device"));
  m.def("hostlink_fill", &hostlink_fill,
        "the GPU stores a memcheck pattern into pinned host memory",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("host"), py::arg("pattern"), py::arg("seed"), py::arg("device"),
        py::arg("blocks") = 0, py::arg("first_vector") = 0);
  m.def("hostlink_verify", &hostlink_verify,
        "the GPU loads pinned host memory and verifies a pattern -> "
        "(mismatched_words, first_bad_word, bad_bits_mask, records)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("host"), py::arg("pattern"), py::arg("seed"), py::arg("device"),
        py::arg("max_records") = 16, py::arg("blocks") = 0,
        py::arg("first_vector") = 0);
  m.def("hostlink_duplex", &hostlink_duplex,
        "one launch verifying read_host while filling write_host -> the "
        "verify tuple of the read side",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("read_host"), py::arg("read_pattern"), py::arg("write_host"),
        py::arg("write_pattern"), py::arg("seed"), py::arg("device"),
        py::arg("max_records") = 16, py::arg("read_blocks") = 0,
        py::arg("write_blocks") = 0, py::arg("read_first_vector") = 0,
        py::arg("write_first_vector") = 0);
}
