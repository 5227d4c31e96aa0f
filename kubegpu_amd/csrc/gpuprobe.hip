// gpuprobe — hand-written CDNA4 (gfx950) bandwidth kernels.
//
// Used by the probe subsystem for the k=1 degenerate point of the
// BASELINE.md curve (single-GPU "all-reduce" has no interconnect: the
// meaningful sanity number is HBM3E streaming bandwidth, spec 8 TB/s,
// ≈6.3 TB/s achievable per MI355X_MICROARCH.md) and by GPU numerics
// tests.
//
// Kernel notes (per /opt/skills/guides/cdna_hip_programming.md):
//  * 256-thread blocks = 4 wave64s; 16 B/lane vectorized access
//    (uint4) -> 4 KiB per block per instruction.
//  * read, fill and the copy variants 0..3 are grid-stride with >> 256
//    workgroups so all 8 XCDs / 256 CUs fill.
//  * copy() launches copy_kernel_tiles: one workgroup per contiguous
//    tile, handed out in address order, with the number of workgroups
//    resident per CU capped by an LDS request (see COPY_TILES_*); the
//    float4-copy pattern at ~83% of HBM peak at 1 GiB.

#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <string>

#define WAVE 64
#define BLOCK 256
// Default grid of the grid-stride copy variants 0..3 (copy_variant,
// copy_bw_gbps) and of read_sum; copy() launches the tile kernel.
// Measured on MI355X (copy sweep, 1 GiB buffers): 1024 blocks (4 per
// CU) + nontemporal beats larger grids of the same kernel — 5816 vs
// 4533 GB/s at 4096 blocks; NT avoids LLC pollution on pure streams.
#define DEFAULT_COPY_BLOCKS 1024
// What copy() launches: copy_kernel_tiles<2> (8 KiB tiles, one per
// workgroup) with at most 3 workgroups resident per CU.  Best median of
// the U x resident sweep at 1 GiB, 50 launches x 3 rounds in one
// process: 6,618 GB/s against 5,838 for the grid-stride kernel above
// re-measured between the candidates (its max - min: 58); uncapped
// U=2 gives 6,221, U=1 capped at 6 6,474.  64 MiB 6,602 vs 6,437,
// 256 MiB 6,738 vs 6,344, 4 GiB 6,636 vs 5,604, 1 MiB (launch-bound)
// 666 vs 673 within the spread — profiles/copy_tiles_sweep_mi355x.json.
#define COPY_TILES_UNROLL 2
#define COPY_TILES_RESIDENT 3
// Pure write streams saturate earlier: >≈900 workgroups the write-drain
// path contends and bandwidth collapses (measured: 640 wg 6,229 GB/s,
// 1024 wg 4,300 GB/s at 1 GiB — profiles/write_bw_sweep_mi355x.json).
#define DEFAULT_WRITE_BLOCKS 640

__global__ void copy_kernel_v4(const uint4* __restrict__ src,
                               uint4* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) dst[i] = src[i];
}

// Non-temporal variant: bypasses L2/LLC allocation on both sides, which
// matters for pure streaming (the 256 MiB Infinity Cache otherwise
// absorbs part of the stream and skews small-buffer numbers).
typedef unsigned int uint4v __attribute__((ext_vector_type(4)));

__global__ void copy_kernel_v4_nt(const uint4v* __restrict__ src,
                                  uint4v* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    uint4v v = __builtin_nontemporal_load(&src[i]);
    __builtin_nontemporal_store(v, &dst[i]);
  }
}

// 4x unrolled NT variant: four independent uint4 transfers in flight
// per thread per iteration (more memory-level parallelism per wave).
__global__ void copy_kernel_v4_nt_u4(const uint4v* __restrict__ src,
                                     uint4v* __restrict__ dst, size_t n4) {
  size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  size_t i = tid;
  size_t bound = n4 >= 3 * stride ? n4 - 3 * stride : 0;
  for (; i < bound; i += 4 * stride) {
    uint4v a = __builtin_nontemporal_load(&src[i]);
    uint4v b = __builtin_nontemporal_load(&src[i + stride]);
    uint4v c = __builtin_nontemporal_load(&src[i + 2 * stride]);
    uint4v d = __builtin_nontemporal_load(&src[i + 3 * stride]);
    __builtin_nontemporal_store(a, &dst[i]);
    __builtin_nontemporal_store(b, &dst[i + stride]);
    __builtin_nontemporal_store(c, &dst[i + 2 * stride]);
    __builtin_nontemporal_store(d, &dst[i + 3 * stride]);
  }
  for (; i < n4; i += stride) {
    uint4v v = __builtin_nontemporal_load(&src[i]);
    __builtin_nontemporal_store(v, &dst[i]);
  }
}

// Contiguous-chunk partitioning: block b owns one contiguous region
// (DRAM-page-friendly; each wave still issues coalesced 1 KiB lines).
__global__ void copy_kernel_v4_nt_chunk(const uint4v* __restrict__ src,
                                        uint4v* __restrict__ dst, size_t n4) {
  size_t per_block = (n4 + gridDim.x - 1) / gridDim.x;
  size_t begin = (size_t)blockIdx.x * per_block;
  size_t end = begin + per_block < n4 ? begin + per_block : n4;
  for (size_t i = begin + threadIdx.x; i < end; i += blockDim.x) {
    uint4v v = __builtin_nontemporal_load(&src[i]);
    __builtin_nontemporal_store(v, &dst[i]);
  }
}

// Mixed variant: regular (cache-allocating) loads + nontemporal stores.
// Answers whether letting the read stream allocate in the 256 MiB LLC
// helps or hurts a pure 1 GiB stream (no reuse => expected ~parity,
// measured to settle it).
__global__ void copy_kernel_v4_mixed(const uint4v* __restrict__ src,
                                     uint4v* __restrict__ dst, size_t n4) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    uint4v v = src[i];
    __builtin_nontemporal_store(v, &dst[i]);
  }
}

// Address-ordered tiles: tile t is the BLOCK*U consecutive vectors from
// t*BLOCK*U, and the normal launch has one workgroup per tile, so the
// dispatcher hands the buffer out in address order as workgroups retire
// (a persistent grid-stride loop drifts apart instead).  A thread issues
// its U loads back to back at lane stride BLOCK, so every wave
// instruction still covers 1 KiB contiguous, then its U stores.  The
// outer loop runs more than once only on a grid capped below the tile
// count.  The kernel declares no LDS: what the launch asks for only
// limits how many of these workgroups a CU holds (launch_copy_tiles).
template <int U>
__global__ void __launch_bounds__(BLOCK)
copy_kernel_tiles(const uint4v* __restrict__ src, uint4v* __restrict__ dst, size_t n4) {
  constexpr size_t T = (size_t)BLOCK * U;
  const size_t tiles = (n4 + T - 1) / T;
  for (size_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const size_t base = t * T + threadIdx.x;
    uint4v v[U];
    if (t * T + T <= n4) {  // full tile (uniform over the workgroup): no compares
#pragma unroll
      for (int u = 0; u < U; ++u)
        v[u] = __builtin_nontemporal_load(&src[base + (size_t)u * BLOCK]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        __builtin_nontemporal_store(v[u], &dst[base + (size_t)u * BLOCK]);
    } else {  // the last, partial tile
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (base + (size_t)u * BLOCK < n4)
          v[u] = __builtin_nontemporal_load(&src[base + (size_t)u * BLOCK]);
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (base + (size_t)u * BLOCK < n4)
          __builtin_nontemporal_store(v[u], &dst[base + (size_t)u * BLOCK]);
    }
  }
}

__global__ void copy_kernel_b(const unsigned char* __restrict__ src,
                              unsigned char* __restrict__ dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = src[i];
}

// Read-only streaming: block-sum of uint4 lanes into one u64 per block
// (measures pure HBM read bandwidth; the result write is negligible).
__global__ void read_sum_kernel(const uint4* __restrict__ src, size_t n4,
                                unsigned long long* __restrict__ out) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned long long acc = 0;
  for (; i < n4; i += stride) {
    uint4 v = src[i];
    acc += (unsigned long long)v.x + v.y + v.z + v.w;
  }
  __shared__ unsigned long long sh[BLOCK / WAVE];
  // wave-level reduce via shuffles (64-wide waves on CDNA)
  for (int off = WAVE / 2; off > 0; off >>= 1)
    acc += __shfl_down(acc, off, WAVE);
  int lane = threadIdx.x % WAVE;
  int wid = threadIdx.x / WAVE;
  if (lane == 0) sh[wid] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long total = 0;
    for (int w = 0; w < BLOCK / WAVE; ++w) total += sh[w];
    atomicAdd(out, total);
  }
}

// Write-only streaming: NT fill (completes the read/write/copy triple).
__global__ void fill_kernel_v4_nt(uint4v* __restrict__ dst, size_t n4,
                                  unsigned int word) {
  uint4v v = {word, word, word, word};
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) __builtin_nontemporal_store(v, &dst[i]);
}

// ---------------------------------------------------------------- host

#define MAX_BLOCKS (1 << 20)

static void check_buf(const at::Tensor& t) {
  TORCH_CHECK(t.is_cuda(), "gpuprobe: tensors must be on GPU");
  TORCH_CHECK(t.is_contiguous(), "gpuprobe: tensors must be contiguous");
}

// A 16 B/lane kernel needs a positive whole number of vectors at a
// 16-byte-aligned address; returns that number.
static size_t check_vec_buf(const at::Tensor& t) {
  check_buf(t);
  TORCH_CHECK(t.nbytes() > 0 && t.nbytes() % 16 == 0,
              "gpuprobe: nbytes must be a positive multiple of 16, got ", t.nbytes());
  TORCH_CHECK((uintptr_t)t.data_ptr() % 16 == 0,
              "gpuprobe: tensor storage must be 16-byte aligned");
  return t.nbytes() / 16;
}

// The kernels take __restrict__ pointers: the same range twice is fine
// (every lane reads an element before it writes that element), two
// ranges that overlap in part are not.
static void check_pair(const at::Tensor& dst, const at::Tensor& src) {
  check_buf(dst);
  check_buf(src);
  TORCH_CHECK(src.nbytes() == dst.nbytes(), "gpuprobe: size mismatch");
  TORCH_CHECK(src.device() == dst.device(),
              "gpuprobe: tensors must be on the same device");
  uintptr_t s = (uintptr_t)src.data_ptr(), d = (uintptr_t)dst.data_ptr();
  size_t n = src.nbytes();
  TORCH_CHECK(s == d || s + n <= d || d + n <= s,
              "gpuprobe: dst and src overlap in part");
}

static int check_threads(int64_t threads_arg) {
  TORCH_CHECK(threads_arg >= 0 && threads_arg % WAVE == 0 && threads_arg <= 1024,
              "threads: multiple of 64, <=1024");
  return threads_arg > 0 ? (int)threads_arg : BLOCK;
}

static int pick_blocks(int64_t blocks_arg, size_t n4, int threads, int dflt) {
  TORCH_CHECK(blocks_arg >= 0 && blocks_arg <= MAX_BLOCKS,
              "gpuprobe: blocks out of range 0..", MAX_BLOCKS);
  if (blocks_arg > 0) return (int)blocks_arg;
  return (int)std::min<size_t>((n4 + threads - 1) / threads, (size_t)dflt);
}

static void check_variant(int64_t variant) {
  TORCH_CHECK(variant >= 0 && variant <= 3, "gpuprobe: variant ", variant,
              " out of range 0..3");
}

// The one place each kernel is launched from: the timed probes and the
// untimed entry points below both go through these, so what the tests
// compare with a reference is what the probes time.
static void launch_copy(const void* src, void* dst, size_t n4, int64_t variant,
                        bool nontemporal, int blocks, int threads,
                        hipStream_t stream) {
  if (variant == 1)
    hipLaunchKernelGGL(copy_kernel_v4_nt_u4, dim3(blocks), dim3(threads), 0, stream,
                       (const uint4v*)src, (uint4v*)dst, n4);
  else if (variant == 2)
    hipLaunchKernelGGL(copy_kernel_v4_nt_chunk, dim3(blocks), dim3(threads), 0,
                       stream, (const uint4v*)src, (uint4v*)dst, n4);
  else if (variant == 3)
    hipLaunchKernelGGL(copy_kernel_v4_mixed, dim3(blocks), dim3(threads), 0,
                       stream, (const uint4v*)src, (uint4v*)dst, n4);
  else if (nontemporal)
    hipLaunchKernelGGL(copy_kernel_v4_nt, dim3(blocks), dim3(threads), 0, stream,
                       (const uint4v*)src, (uint4v*)dst, n4);
  else
    hipLaunchKernelGGL(copy_kernel_v4, dim3(blocks), dim3(threads), 0, stream,
                       (const uint4*)src, (uint4*)dst, n4);
}

// LDS of one CU, and the step that the hardware hands it out in.
#define CU_LDS_BYTES (160 * 1024)
#define LDS_GRANULE 1280
#define MAX_DEVICES 64

static void check_tiles_args(int64_t unroll, int64_t resident, int64_t max_blocks) {
  TORCH_CHECK(unroll == 1 || unroll == 2 || unroll == 4 || unroll == 8,
              "gpuprobe: unroll must be 1, 2, 4 or 8, got ", unroll);
  TORCH_CHECK(resident >= 0 && resident <= 8, "gpuprobe: resident ", resident,
              " out of range 0..8");
  TORCH_CHECK(max_blocks >= 0 && max_blocks <= MAX_BLOCKS,
              "gpuprobe: max_blocks out of range 0..", MAX_BLOCKS);
}

template <int U>
static void launch_copy_tiles_u(const void* src, void* dst, size_t n4, int resident,
                                int max_blocks, hipStream_t stream) {
  size_t tiles = (n4 + (size_t)BLOCK * U - 1) / ((size_t)BLOCK * U);
  size_t cap = max_blocks > 0 ? (size_t)max_blocks : (size_t)MAX_BLOCKS;
  // Residency cap: the kernel never touches this LDS.  A CU holds only
  // as many workgroups as its 160 KiB cover, so asking for a 1/resident
  // share of it (rounded down to whole granules) keeps a CU from taking
  // more than `resident` of these workgroups while tiles are still
  // handed out in order; resident == 0 asks for none and leaves the
  // limit to the 32 waves per CU (8 workgroups).
  size_t lds = resident > 0 ? CU_LDS_BYTES / resident / LDS_GRANULE * LDS_GRANULE : 0;
  if (lds > 64 * 1024) {  // more than that has to be asked for, once per device
    static std::atomic<bool> raised[MAX_DEVICES];
    int dev = 0;
    C10_HIP_CHECK(hipGetDevice(&dev));
    TORCH_CHECK(dev >= 0 && dev < MAX_DEVICES, "gpuprobe: device index ", dev);
    if (!raised[dev].load(std::memory_order_acquire)) {
      C10_HIP_CHECK(hipFuncSetAttribute((const void*)copy_kernel_tiles<U>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize,
                                        CU_LDS_BYTES));
      raised[dev].store(true, std::memory_order_release);
    }
  }
  hipLaunchKernelGGL(copy_kernel_tiles<U>, dim3((unsigned)std::min(tiles, cap)),
                     dim3(BLOCK), lds, stream, (const uint4v*)src, (uint4v*)dst, n4);
}

// The one launch of the tile kernel, for copy(), copy_tiles and
// copy_tiles_bw_gbps alike; the arguments have passed check_tiles_args.
static void launch_copy_tiles(const void* src, void* dst, size_t n4, int unroll,
                              int resident, int max_blocks, hipStream_t stream) {
  switch (unroll) {
    case 1: launch_copy_tiles_u<1>(src, dst, n4, resident, max_blocks, stream); break;
    case 2: launch_copy_tiles_u<2>(src, dst, n4, resident, max_blocks, stream); break;
    case 4: launch_copy_tiles_u<4>(src, dst, n4, resident, max_blocks, stream); break;
    default: launch_copy_tiles_u<8>(src, dst, n4, resident, max_blocks, stream); break;
  }
}

// read_sum_kernel sizes its LDS array for BLOCK threads.
static void launch_read_sum(const void* src, size_t n4, void* out, int blocks,
                            hipStream_t stream) {
  hipLaunchKernelGGL(read_sum_kernel, dim3(blocks), dim3(BLOCK), 0, stream,
                     (const uint4*)src, n4, (unsigned long long*)out);
}

static void launch_fill(void* dst, size_t n4, unsigned int word, int blocks,
                        hipStream_t stream) {
  hipLaunchKernelGGL(fill_kernel_v4_nt, dim3(blocks), dim3(BLOCK), 0, stream,
                     (uint4v*)dst, n4, word);
}

void copy(at::Tensor dst, at::Tensor src) {
  check_pair(dst, src);
  size_t nbytes = src.nbytes();
  if (nbytes == 0) return;
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(dst));
  auto stream = at::hip::getCurrentHIPStream();
  // 16 B vectors only for a whole number of them at aligned addresses;
  // a view at a 4-byte offset goes to the byte kernel like an odd size
  if ((((uintptr_t)src.data_ptr() | (uintptr_t)dst.data_ptr() | nbytes) & 15) == 0) {
    launch_copy_tiles(src.data_ptr(), dst.data_ptr(), nbytes / 16, COPY_TILES_UNROLL,
                      COPY_TILES_RESIDENT, 0, stream);
  } else {
    int blocks = (int)std::min<size_t>((nbytes + BLOCK - 1) / BLOCK, 4096);
    hipLaunchKernelGGL(copy_kernel_b, dim3(blocks), dim3(BLOCK), 0, stream,
                       (const unsigned char*)src.data_ptr(),
                       (unsigned char*)dst.data_ptr(), nbytes);
  }
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// One untimed launch of a copy_bw_gbps variant on the caller's tensors
// (same kernel selection, same default grid).
void copy_variant(at::Tensor dst, at::Tensor src, int64_t variant, bool nontemporal,
                  int64_t blocks_arg, int64_t threads_arg) {
  check_pair(dst, src);
  size_t n4 = check_vec_buf(src);
  check_vec_buf(dst);
  check_variant(variant);
  int threads = check_threads(threads_arg);
  int blocks = pick_blocks(blocks_arg, n4, threads, DEFAULT_COPY_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(dst));
  auto stream = at::hip::getCurrentHIPStream();
  launch_copy(src.data_ptr(), dst.data_ptr(), n4, variant, nontemporal, blocks,
              threads, stream);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// One untimed launch of the tile kernel on the caller's tensors;
// max_blocks > 0 caps the grid, so that workgroups loop over tiles.
void copy_tiles(at::Tensor dst, at::Tensor src, int64_t unroll, int64_t resident,
                int64_t max_blocks) {
  check_pair(dst, src);
  size_t n4 = check_vec_buf(src);
  check_vec_buf(dst);
  check_tiles_args(unroll, resident, max_blocks);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(dst));
  auto stream = at::hip::getCurrentHIPStream();
  launch_copy_tiles(src.data_ptr(), dst.data_ptr(), n4, (int)unroll, (int)resident,
                    (int)max_blocks, stream);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

// One launch of read_sum_kernel into a fresh accumulator: the sum of
// all 32-bit words of src, modulo 2^64.
uint64_t read_sum(at::Tensor src, int64_t blocks_arg) {
  size_t n4 = check_vec_buf(src);
  int blocks = pick_blocks(blocks_arg, n4, BLOCK, DEFAULT_COPY_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(src));
  at::Tensor out = at::zeros({1}, src.options().dtype(at::kLong));
  auto stream = at::hip::getCurrentHIPStream();
  launch_read_sum(src.data_ptr(), n4, out.data_ptr(), blocks, stream);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  C10_HIP_CHECK(hipStreamSynchronize(stream));
  return (uint64_t)out.item<int64_t>();
}

// One launch of fill_kernel_v4_nt: every 32-bit word of dst = word.
void fill_word(at::Tensor dst, int64_t word, int64_t blocks_arg) {
  size_t n4 = check_vec_buf(dst);
  TORCH_CHECK(word >= 0 && word <= 0xFFFFFFFFLL, "gpuprobe: word must be a u32");
  int blocks = pick_blocks(blocks_arg, n4, BLOCK, DEFAULT_WRITE_BLOCKS);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(dst));
  auto stream = at::hip::getCurrentHIPStream();
  launch_fill(dst.data_ptr(), n4, (unsigned int)word, blocks, stream);
  C10_HIP_KERNEL_LAUNCH_CHECK();
}

static void check_timed_args(int64_t nbytes, int64_t iters) {
  TORCH_CHECK(nbytes > 0 && nbytes % 16 == 0, "nbytes must be positive, 16-aligned");
  TORCH_CHECK(iters >= 1, "iters must be at least 1");
}

// Byte the timed probes put into a destination before the first launch.
// The caching allocator often hands back the block that the previous
// probe freed, still full of the "expected" 0x01 bytes: without this a
// kernel that wrote nothing would pass the self-check.
#define POISON 0xA5

// The timed loop of the three probes: three untimed launches, then
// `iters` launches between two events; returns their milliseconds.  The
// events are destroyed before a launch error is raised.
template <typename Launch>
static float timed_ms(hipStream_t stream, int64_t iters, Launch&& launch) {
  for (int w = 0; w < 3; ++w) launch();
  hipEvent_t t0, t1;
  (void)hipEventCreate(&t0);
  (void)hipEventCreate(&t1);
  (void)hipEventRecord(t0, stream);
  for (int64_t i = 0; i < iters; ++i) launch();
  (void)hipEventRecord(t1, stream);
  (void)hipEventSynchronize(t1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, t0, t1);
  (void)hipEventDestroy(t0);
  (void)hipEventDestroy(t1);
  C10_HIP_KERNEL_LAUNCH_CHECK();
  return ms;
}

// The body of the timed copy probes: a source of 0x01 bytes and a
// poisoned destination, `launch(src, dst, stream)` timed, the destination
// compared with the source; returns achieved GB/s (bytes read + bytes
// written over wall time, hipEvent-timed).
template <typename Launch>
static double timed_copy_gbps(int64_t nbytes, int64_t iters, const std::string& who,
                              Launch&& launch) {
  auto opts = at::TensorOptions().dtype(at::kByte).device(at::kCUDA);
  at::Tensor src = at::empty({nbytes}, opts);
  at::Tensor dst = at::empty({nbytes}, opts);
  src.fill_(1);
  dst.fill_(POISON);
  auto stream = at::hip::getCurrentHIPStream();
  float ms = timed_ms(stream, iters,
                      [&]() { launch(src.data_ptr(), dst.data_ptr(), stream); });
  TORCH_CHECK(at::equal(dst, src), who, " produced wrong output");
  double sec = ms / 1e3;
  return (double)nbytes * 2.0 * iters / sec / 1e9;
}

// Timed device-to-device streaming copy with one of the variants 0..3.
// blocks=0 picks the default; nontemporal selects the NT variant.
double copy_bw_gbps(int64_t nbytes, int64_t iters, int64_t blocks_arg,
                    bool nontemporal, int64_t variant, int64_t threads_arg) {
  check_timed_args(nbytes, iters);
  check_variant(variant);
  size_t n4 = (size_t)nbytes / 16;
  // workgroup SIZE is a runtime launch dim (the kernels read blockDim),
  // so the wave-granularity axis can be swept without new kernels
  int threads = check_threads(threads_arg);
  int blocks = pick_blocks(blocks_arg, n4, threads, DEFAULT_COPY_BLOCKS);
  return timed_copy_gbps(nbytes, iters, "copy_bw_gbps: variant " + std::to_string(variant),
                         [&](const void* src, void* dst, hipStream_t stream) {
    launch_copy(src, dst, n4, variant, nontemporal, blocks, threads, stream);
  });
}

// The same measurement of the tile kernel (launch_copy_tiles).
double copy_tiles_bw_gbps(int64_t nbytes, int64_t iters, int64_t unroll,
                          int64_t resident, int64_t max_blocks) {
  check_timed_args(nbytes, iters);
  check_tiles_args(unroll, resident, max_blocks);
  size_t n4 = (size_t)nbytes / 16;
  return timed_copy_gbps(nbytes, iters, "copy_tiles_bw_gbps: the tile kernel",
                         [&](const void* src, void* dst, hipStream_t stream) {
    launch_copy_tiles(src, dst, n4, (int)unroll, (int)resident, (int)max_blocks, stream);
  });
}

double write_bw_gbps(int64_t nbytes, int64_t iters, int64_t blocks_arg) {
  check_timed_args(nbytes, iters);
  size_t n4 = (size_t)nbytes / 16;
  int blocks = pick_blocks(blocks_arg, n4, BLOCK, DEFAULT_WRITE_BLOCKS);
  auto opts = at::TensorOptions().dtype(at::kByte).device(at::kCUDA);
  at::Tensor dst = at::empty({nbytes}, opts);
  dst.fill_(POISON);
  auto stream = at::hip::getCurrentHIPStream();
  float ms = timed_ms(stream, iters, [&]() {
    launch_fill(dst.data_ptr(), n4, 0x01010101u, blocks, stream);
  });
  // every byte is 0x01 iff min == max == 1 (a sum alone is met by
  // other contents too)
  TORCH_CHECK(dst.min().item<uint8_t>() == 1 && dst.max().item<uint8_t>() == 1,
              "write_bw_gbps: fill produced wrong output");
  return (double)nbytes * iters / (ms / 1e3) / 1e9;
}

double read_bw_gbps(int64_t nbytes, int64_t iters, int64_t blocks_arg) {
  check_timed_args(nbytes, iters);
  size_t n4 = (size_t)nbytes / 16;
  // Reads peak at 1024 wg (4 waves/CU): 6,115 GB/s vs 5,768 at 4096
  // (profiles/read_bw_sweep_mi355x.json)
  int blocks = pick_blocks(blocks_arg, n4, BLOCK, DEFAULT_COPY_BLOCKS);
  auto opts = at::TensorOptions().dtype(at::kByte).device(at::kCUDA);
  at::Tensor src = at::empty({nbytes}, opts);
  src.fill_(1);
  at::Tensor out = at::zeros({1}, at::TensorOptions().dtype(at::kLong).device(at::kCUDA));
  auto stream = at::hip::getCurrentHIPStream();
  float ms = timed_ms(stream, iters, [&]() {
    launch_read_sum(src.data_ptr(), n4, out.data_ptr(), blocks, stream);
  });
  // every launch adds the whole buffer's words to out: a kernel that
  // read less would report too high a bandwidth
  uint64_t want = (uint64_t)(3 + iters) * ((uint64_t)nbytes / 4) * 0x01010101ULL;
  TORCH_CHECK((uint64_t)out.item<int64_t>() == want,
              "read_bw_gbps: read_sum_kernel produced a wrong sum");
  double sec = ms / 1e3;
  return (double)nbytes * iters / sec / 1e9;
}

// HBM integrity kernels (memcheck.hip, same extension).
void bind_memcheck(py::module_& m);
// Compute-unit integrity kernel (cucheck.hip, same extension).
void bind_cucheck(py::module_& m);
// Matrix-core format integrity kernel (mxcheck.hip, same extension).
void bind_mxcheck(py::module_& m);
// IEEE rounding integrity kernel (fpcheck.hip, same extension).
void bind_fpcheck(py::module_& m);
// Atomic-unit integrity kernel (atomcheck.hip, same extension).
void bind_atomcheck(py::module_& m);
// Cross-lane integrity kernel (lanecheck.hip, same extension).
void bind_lanecheck(py::module_& m);
// LDS integrity kernel (ldscheck.hip, same extension).
void bind_ldscheck(py::module_& m);
// Vector-memory integrity kernel (vmemcheck.hip, same extension).
void bind_vmemcheck(py::module_& m);
// Host-link integrity kernels (hostlink.hip, same extension).
void bind_hostlink(py::module_& m);

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  bind_memcheck(m);
  bind_cucheck(m);
  bind_mxcheck(m);
  bind_fpcheck(m);
  bind_atomcheck(m);
  bind_lanecheck(m);
  bind_ldscheck(m);
  bind_vmemcheck(m);
  bind_hostlink(m);
  // The timed probes release the GIL: a multi-second hipEvent-timed
  // block must not starve other Python threads (the node agent serves
  // gRPC from the same process — measured: with the GIL held, every
  // concurrent RPC hit DEADLINE_EXCEEDED during a probe block).
  m.def("copy", &copy, "streaming uint4 copy kernel (dst, src)",
        py::call_guard<py::gil_scoped_release>());
  m.def("copy_variant", &copy_variant,
        "one untimed launch of a copy_bw_gbps variant (dst, src)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("dst"), py::arg("src"), py::arg("variant") = 0,
        py::arg("nontemporal") = true, py::arg("blocks") = 0,
        py::arg("threads") = 0);
  m.def("copy_tiles", &copy_tiles,
        "one untimed launch of the address-ordered tile copy kernel (dst, src)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("dst"), py::arg("src"), py::arg("unroll"), py::arg("resident"),
        py::arg("max_blocks") = 0);
  m.def("copy_tiles_bw_gbps", &copy_tiles_bw_gbps,
        "timed d2d copy bandwidth of the tile copy kernel",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("nbytes"), py::arg("iters"), py::arg("unroll"), py::arg("resident"),
        py::arg("max_blocks") = 0);
  m.def("read_sum", &read_sum, "u64 sum of all 32-bit words (one launch)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("src"), py::arg("blocks") = 0);
  m.def("fill_word", &fill_word, "NT fill of every 32-bit word (one launch)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("dst"), py::arg("word"), py::arg("blocks") = 0);
  m.def("copy_bw_gbps", &copy_bw_gbps, "timed d2d copy bandwidth",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("nbytes"), py::arg("iters") = 20, py::arg("blocks") = 0,
        py::arg("nontemporal") = true, py::arg("variant") = 0,
        py::arg("threads") = 0);
  m.def("read_bw_gbps", &read_bw_gbps, "timed read bandwidth",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("nbytes"), py::arg("iters") = 20, py::arg("blocks") = 0);
  m.def("write_bw_gbps", &write_bw_gbps, "timed write-only (NT fill) bandwidth",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("nbytes"), py::arg("iters") = 20, py::arg("blocks") = 0);
}
