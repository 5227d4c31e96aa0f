// rcclprobe — in-pod RCCL-over-xGMI all-reduce bandwidth probe.
//
// The verification half of the MI355X scheduler (SURVEY.md §2.2, §5
// "Distributed communication backend"): the scheduler places k-GPU pods
// on the subset with the best xGMI ring; this probe ring-all-reduces
// over the GPUs actually visible in the pod (after ROCR_VISIBLE_DEVICES
// + /dev/dri injection) and reports achieved GB/s, closing the loop
// between the topology model and measured bandwidth.  The reference has
// no analog — its topology tree is an unverified proxy ("same gpugrp0
// => fast", nvidia_gpu_manager.go:177-180).
//
// Single-process multi-GPU (ncclCommInitAll): the pod's GPU set is a
// single node's xGMI hive, which is exactly the regime where one process
// driving k devices over RCCL is the cheapest correct harness.
//
// Build: hipcc --offload-arch=gfx950 -O2 rcclprobe.cpp -lrccl -o bin/rcclprobe
//
// Timed loop: warmup + iters out-of-place bf16 sum all-reduces of a
// constant 1.0 input, exactly the workload of the recorded profiles.
//
// Check (after the timed loop, untimed; --no-check skips all of it):
//   base(seed, r) = fmix32(seed ^ ((r + 1) * 0x9E3779B9 mod 2^32))
//   v(seed, r, i) = fmix32(base(seed, r) ^ i) & 3     r = rank, i = element
//   send_r[i]     = bf16(v)       bits 0x0000, 0x3F80, 0x4000, 0x4040
//   expected[i]   = bf16(sum over r < n of v(seed, r, i))
// Every send is filled with its rank's pattern and every recv with
// 0xFFFF, one more all-reduce runs, then a kernel compares every element
// of every recv with `expected` and every element of every send with its
// own pattern, bitwise.  Every partial sum is an integer <= 3n <= 192
// (n <= 64) and bf16 holds integers up to 256 exactly, so the result does
// not depend on the order RCCL reduces in.  The 0xFFFF poison and the
// timed loop's constant input both differ from the pattern, so an
// all-reduce that writes nothing cannot pass on an earlier result.
// probe/rccl_probe.py:reference_send / reference_sum are the numpy
// definition the tests compare against.
//
// Output (one JSON line, also when the check fails):
//   {"ndev": 8, "bytes": 268435456, "iters": 20, "warmup": 5,
//    "time_ms_per_iter": 3.1, "algbw_gbps": 86.6, "busbw_gbps": 151.6,
//    "dtype": "bf16", "check": "pass", "mode": "rccl", "seed": 0,
//    "checked_elements": 2147483648, "mismatches": 0, "first_bad": null,
//    "records": [], "fill_blocks": 1024, "verify_blocks": 2048,
//    "block_threads": 256}
// check is "pass", "fail" or "skipped" (then the fields from
// checked_elements to records are absent).  first_bad and each record are
// {"rank", "buffer" ("recv" | "send"), "index", "expected", "got"} with
// bf16 bits as integers; at most 16 records per buffer and 64 in all are
// kept, mismatches counts every bad element.
// busbw = algbw * 2*(n-1)/n  (ring all-reduce moves 2*(n-1)/n * bytes
// per rank over its slowest link).
//
// Exit: 0 pass or skipped, 1 could not run, 2 bad arguments (nothing on
// stdout), 3 check failed.

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <sys/stat.h>

#include <cerrno>
#include <chrono>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define HIPCHECK(cmd)                                                          \
  do {                                                                         \
    hipError_t e = (cmd);                                                      \
    if (e != hipSuccess) {                                                     \
      fprintf(stderr, "rcclprobe: HIP error %s at %s:%d\n",                    \
              hipGetErrorString(e), __FILE__, __LINE__);                       \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

#define NCCLCHECK(cmd)                                                         \
  do {                                                                         \
    ncclResult_t r = (cmd);                                                    \
    if (r != ncclSuccess) {                                                    \
      fprintf(stderr, "rcclprobe: RCCL error %s at %s:%d\n",                   \
              ncclGetErrorString(r), __FILE__, __LINE__);                      \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

typedef unsigned long long u64;

#define WAVE 64
#define BLOCK_THREADS 256
// One element per thread per grid-stride sweep.  The two grids differ on
// purpose: a sweep edge of one kernel is then no sweep edge of the other.
#define FILL_BLOCKS 1024
#define VERIFY_BLOCKS 2048
#define REDUCE_BLOCKS 1024
#define MAX_RANKS 64
#define MAX_RECORDS 16        // per verified buffer
#define MAX_JSON_RECORDS 64   // per output line
#define MAX_BYTES (8ll << 30)         // 2^32 bf16 elements: the index is a u32
#define MAX_DUMP_BYTES (64ll << 20)   // per buffer

// Result block of one verify launch (u64 slots), then MAX_RECORDS records
// of two u64 each: {element index, expected bits << 16 | got bits}.
#define RES_COUNT 0
#define RES_FIRST 1
#define RES_CLAIM 2
#define RES_HEADER 3
#define RES_SLOTS (RES_HEADER + 2 * MAX_RECORDS)

__host__ __device__ __forceinline__ unsigned int fmix32(unsigned int h) {
  h ^= h >> 16;
  h *= 0x85EBCA6Bu;
  h ^= h >> 13;
  h *= 0xC2B2AE35u;
  h ^= h >> 16;
  return h;
}

__host__ __device__ __forceinline__ unsigned int rank_base(unsigned int seed, int rank) {
  return fmix32(seed ^ ((unsigned int)(rank + 1) * 0x9E3779B9u));
}

__host__ __device__ __forceinline__ unsigned int pattern_value(unsigned int base,
                                                      unsigned int i) {
  return fmix32(base ^ i) & 3u;
}

// bf16 bits of an integer 0..256: the top half of its f32 encoding, whose
// low half is zero for these values.
__device__ __forceinline__ unsigned short bf16_of_small(unsigned int v) {
  return (unsigned short)(__float_as_uint((float)v) >> 16);
}

__global__ void __launch_bounds__(BLOCK_THREADS)
fill_const_bf16(unsigned short* __restrict__ p, size_t n, unsigned short bits) {
  size_t i = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  size_t stride = (size_t)gridDim.x * BLOCK_THREADS;
  for (; i < n; i += stride) p[i] = bits;
}

__global__ void __launch_bounds__(BLOCK_THREADS)
fill_pattern_bf16(unsigned short* __restrict__ p, size_t n, unsigned int seed,
                  int rank) {
  unsigned int base = rank_base(seed, rank);
  size_t i = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  size_t stride = (size_t)gridDim.x * BLOCK_THREADS;
  for (; i < n; i += stride)
    p[i] = bf16_of_small(pattern_value(base, (unsigned int)i));
}

// Mismatch path only: claim a log slot per bad element; slots past
// MAX_RECORDS are dropped, the count is not.
static __device__ __noinline__ void log_mismatch(u64* __restrict__ res, u64 index,
                                                 unsigned short expected,
                                                 unsigned short got) {
  u64 slot = atomicAdd(&res[RES_CLAIM], 1ULL);
  if (slot < (u64)MAX_RECORDS) {
    res[RES_HEADER + 2 * slot] = index;
    res[RES_HEADER + 2 * slot + 1] = ((u64)expected << 16) | (u64)got;
  }
}

// Compares p[0..n) bitwise with bf16(sum of v(seed, r, i) over
// rank_lo <= r < rank_lo + nranks): nranks = 1 is one rank's send pattern,
// rank_lo = 0 the all-reduce result of nranks ranks.  Per-thread tally ->
// wave shuffle -> LDS block reduce -> one atomic per block per result.
__global__ void __launch_bounds__(BLOCK_THREADS)
verify_pattern_bf16(const unsigned short* __restrict__ p, size_t n,
                    unsigned int seed, int rank_lo, int nranks,
                    u64* __restrict__ res) {
  __shared__ unsigned int sh_base[MAX_RANKS];
  __shared__ u64 sh_count[BLOCK_THREADS / WAVE];
  __shared__ u64 sh_first[BLOCK_THREADS / WAVE];
  if ((int)threadIdx.x < nranks)
    sh_base[threadIdx.x] = rank_base(seed, rank_lo + (int)threadIdx.x);
  __syncthreads();

  u64 count = 0, first = ~0ULL;
  size_t i = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  size_t stride = (size_t)gridDim.x * BLOCK_THREADS;
  for (; i < n; i += stride) {
    unsigned int sum = 0;
    for (int r = 0; r < nranks; ++r)
      sum += pattern_value(sh_base[r], (unsigned int)i);
    unsigned short expected = bf16_of_small(sum);
    unsigned short got = p[i];
    if (got != expected) {
      ++count;
      if ((u64)i < first) first = (u64)i;
      log_mismatch(res, (u64)i, expected, got);
    }
  }

  for (int off = WAVE / 2; off > 0; off >>= 1) {
    count += __shfl_down(count, off, WAVE);
    u64 f = __shfl_down(first, off, WAVE);
    first = f < first ? f : first;
  }
  int lane = threadIdx.x % WAVE;
  int wid = threadIdx.x / WAVE;
  if (lane == 0) {
    sh_count[wid] = count;
    sh_first[wid] = first;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 c = 0, f = ~0ULL;
    for (int w = 0; w < BLOCK_THREADS / WAVE; ++w) {
      c += sh_count[w];
      f = sh_first[w] < f ? sh_first[w] : f;
    }
    if (c != 0) {
      atomicAdd(&res[RES_COUNT], c);
      atomicMin(&res[RES_FIRST], f);
    }
  }
}

struct SrcTable {
  const unsigned short* p[MAX_RANKS];
};

// --loopback stand-in for the all-reduce: f32 sum of n bf16 inputs,
// narrowed to bf16 round-to-nearest-even (finite inputs only).
__global__ void __launch_bounds__(BLOCK_THREADS)
reduce_sum_bf16(SrcTable src, int n, unsigned short* __restrict__ dst,
                size_t count) {
  size_t i = (size_t)blockIdx.x * BLOCK_THREADS + threadIdx.x;
  size_t stride = (size_t)gridDim.x * BLOCK_THREADS;
  for (; i < count; i += stride) {
    float acc = 0.0f;
    for (int r = 0; r < n; ++r)
      acc += __uint_as_float((unsigned int)src.p[r][i] << 16);
    unsigned int u = __float_as_uint(acc);
    u += 0x7FFFu + ((u >> 16) & 1u);
    dst[i] = (unsigned short)(u >> 16);
  }
}

// ---------------------------------------------------------------- host

static const char* USAGE =
    "usage: rcclprobe [--ndev N | --devices 0,1,..] [--bytes B] [--iters I]\n"
    "                 [--warmup W] [--seed S] [--no-check]\n"
    "  --bytes B     per-rank buffer size, a positive even number <= 8 GiB\n"
    "  --seed S      u32 seed of the check pattern (default 0)\n"
    "  --no-check    skip the pattern all-reduce and its verification\n"
    "test hooks:\n"
    "  --corrupt RANK:INDEX:MASK  XOR the 16-bit MASK into element INDEX of\n"
    "                rank RANK's result before it is verified (repeatable)\n"
    "  --dump-dir DIR  write send_<rank>.bin and recv_<rank>.bin (raw bf16)\n"
    "                after verification; buffers of at most 64 MiB\n"
    "  --loopback N  no RCCL: N (1..64) send buffers on the first selected\n"
    "                device, reduced by a plain kernel into one recv\n";

[[noreturn]] static void bad_args(const char* fmt, const char* a = "",
                                  const char* b = "") {
  fprintf(stderr, "rcclprobe: ");
  fprintf(stderr, fmt, a, b);
  fprintf(stderr, "\n");
  exit(2);
}

// Whole string must be one integer; base 0 also takes 0x.. for seeds and masks.
static bool parse_int(const char* s, int base, long long* out) {
  if (!s || !*s || s[0] == ' ' || s[0] == '\t' || s[0] == '\n') return false;
  errno = 0;
  char* end = nullptr;
  long long v = strtoll(s, &end, base);
  if (errno != 0 || end == s || *end != '\0') return false;
  *out = v;
  return true;
}

static long long int_arg(const char* opt, const char* s, int base, long long lo,
                         long long hi) {
  long long v;
  if (!parse_int(s, base, &v)) bad_args("%s: '%s' is not a whole number", opt, s);
  if (v < lo || v > hi) bad_args("%s: %s is out of range", opt, s);
  return v;
}

struct Corrupt {
  int rank;
  size_t index;
  unsigned short mask;
};

struct BadRecord {
  int rank;
  const char* buffer;
  u64 index;
  unsigned int expected, got;
};

struct CheckState {
  u64 checked = 0, mismatches = 0;
  bool have_first = false;
  BadRecord first_bad{};
  std::vector<BadRecord> records;
};

// bf16 bits of the pattern sum at one element, on the host.
static unsigned int host_expected(unsigned int seed, int rank_lo, int nranks,
                                  u64 index) {
  unsigned int sum = 0;
  for (int r = 0; r < nranks; ++r)
    sum += pattern_value(rank_base(seed, rank_lo + r), (unsigned int)index);
  float f = (float)sum;
  unsigned int u;
  memcpy(&u, &f, sizeof(u));
  return u >> 16;
}

// Verify one buffer on the current device and fold the result into st.
static void verify_buffer(CheckState& st, const void* buf, size_t count,
                          unsigned int seed, int rank_lo, int nranks,
                          int rank_label, const char* buffer_label, u64* d_res) {
  u64 h[RES_SLOTS];
  memset(h, 0, sizeof(h));
  h[RES_FIRST] = ~0ULL;
  HIPCHECK(hipMemcpy(d_res, h, sizeof(h), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(verify_pattern_bf16, dim3(VERIFY_BLOCKS), dim3(BLOCK_THREADS),
                     0, nullptr, (const unsigned short*)buf, count, seed, rank_lo,
                     nranks, d_res);
  HIPCHECK(hipGetLastError());
  HIPCHECK(hipDeviceSynchronize());
  HIPCHECK(hipMemcpy(h, d_res, sizeof(h), hipMemcpyDeviceToHost));
  st.checked += count;
  if (h[RES_COUNT] == 0) return;
  st.mismatches += h[RES_COUNT];
  u64 nrec = h[RES_CLAIM] < MAX_RECORDS ? h[RES_CLAIM] : MAX_RECORDS;
  for (u64 r = 0; r < nrec; ++r) {
    BadRecord b{rank_label, buffer_label, h[RES_HEADER + 2 * r],
                (unsigned int)(h[RES_HEADER + 2 * r + 1] >> 16) & 0xFFFFu,
                (unsigned int)(h[RES_HEADER + 2 * r + 1] & 0xFFFFu)};
    if (st.records.size() < MAX_JSON_RECORDS) st.records.push_back(b);
  }
  if (!st.have_first) {
    // the lowest bad element may have lost the race for a record slot, so
    // first_bad never comes from the records: read it back, expected from
    // the host's own evaluation of the pattern
    unsigned short got = 0;
    if (h[RES_FIRST] >= (u64)count) {
      fprintf(stderr, "rcclprobe: verify reported bad index %llu of %zu\n",
              h[RES_FIRST], count);
      exit(1);
    }
    HIPCHECK(hipMemcpy(&got, (const unsigned short*)buf + h[RES_FIRST], 2,
                       hipMemcpyDeviceToHost));
    st.first_bad = BadRecord{rank_label, buffer_label, h[RES_FIRST],
                             host_expected(seed, rank_lo, nranks, h[RES_FIRST]), got};
    st.have_first = true;
  }
}

static void append_record(std::string& s, const BadRecord& b) {
  char tmp[200];
  snprintf(tmp, sizeof(tmp),
           "{\"rank\": %d, \"buffer\": \"%s\", \"index\": %llu, "
           "\"expected\": %u, \"got\": %u}",
           b.rank, b.buffer, b.index, b.expected, b.got);
  s += tmp;
}

static void dump_buffer(const std::string& dir, const char* name, int rank,
                        const void* dbuf, size_t count) {
  std::vector<unsigned short> host(count);
  HIPCHECK(hipMemcpy(host.data(), dbuf, count * 2, hipMemcpyDeviceToHost));
  std::string path = dir + "/" + name + "_" + std::to_string(rank) + ".bin";
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(host.data(), 2, count, f) != count || fclose(f) != 0) {
    fprintf(stderr, "rcclprobe: cannot write %s: %s\n", path.c_str(),
            strerror(errno));
    exit(1);
  }
}

int main(int argc, char** argv) {
  long long bytes = 256ll << 20;  // 256 MiB per rank
  int iters = 20, warmup = 5, ndev = -1, loopback = 0;
  unsigned int seed = 0;
  bool check = true, have_devlist = false;
  std::string devlist, dump_dir;
  std::vector<Corrupt> corrupts;
  std::vector<std::string> corrupt_args;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&]() -> const char* {
      if (i + 1 >= argc) bad_args("missing value for %s", a.c_str());
      return argv[++i];
    };
    if (a == "--bytes") bytes = int_arg("--bytes", next(), 10, 1, MAX_BYTES);
    else if (a == "--iters") iters = (int)int_arg("--iters", next(), 10, 1, INT_MAX);
    else if (a == "--warmup") warmup = (int)int_arg("--warmup", next(), 10, 0, INT_MAX);
    else if (a == "--ndev") ndev = (int)int_arg("--ndev", next(), 10, 1, INT_MAX);
    else if (a == "--devices") { devlist = next(); have_devlist = true; }
    else if (a == "--seed") seed = (unsigned int)int_arg("--seed", next(), 0, 0, 0xFFFFFFFFll);
    else if (a == "--loopback") loopback = (int)int_arg("--loopback", next(), 10, 1, MAX_RANKS);
    else if (a == "--corrupt") corrupt_args.push_back(next());
    else if (a == "--dump-dir") dump_dir = next();
    else if (a == "--no-check") check = false;
    else {
      fputs(USAGE, stderr);
      return 2;
    }
  }
  if (bytes % 2 != 0) bad_args("--bytes: must be even (bf16 elements)");
  size_t count = (size_t)(bytes / 2);  // bf16 elements

  std::vector<int> devs;
  if (have_devlist) {
    // strtok would swallow empty entries ("0,,1", a trailing comma)
    size_t pos = 0;
    for (;;) {
      size_t comma = devlist.find(',', pos);
      std::string tok = devlist.substr(pos, comma == std::string::npos ? comma : comma - pos);
      int d = (int)int_arg("--devices", tok.c_str(), 10, 0, INT_MAX);
      for (int e : devs)
        if (e == d) bad_args("--devices: %s is listed twice", tok.c_str());
      devs.push_back(d);
      if (comma == std::string::npos) break;
      pos = comma + 1;
    }
  }
  if (loopback && ndev >= 0) bad_args("--loopback takes its rank count itself; drop --ndev");
  if (!check && (!corrupt_args.empty() || !dump_dir.empty()))
    bad_args("--corrupt and --dump-dir need the check; drop --no-check");
  if (!dump_dir.empty() && bytes > MAX_DUMP_BYTES)
    bad_args("--dump-dir: buffers above 64 MiB are not dumped");
  // ranks known from the arguments alone (-1: every device present)
  int nranks_known = loopback ? loopback : have_devlist ? (int)devs.size() : ndev;
  for (const std::string& c : corrupt_args) {
    size_t c1 = c.find(':');
    size_t c2 = c1 == std::string::npos ? c1 : c.find(':', c1 + 1);
    if (c2 == std::string::npos) bad_args("--corrupt: '%s' is not RANK:INDEX:MASK", c.c_str());
    std::string r = c.substr(0, c1), x = c.substr(c1 + 1, c2 - c1 - 1), m = c.substr(c2 + 1);
    Corrupt k;
    k.rank = (int)int_arg("--corrupt rank", r.c_str(), 10, 0, MAX_RANKS - 1);
    k.index = (size_t)int_arg("--corrupt index", x.c_str(), 10, 0, (long long)count - 1);
    k.mask = (unsigned short)int_arg("--corrupt mask", m.c_str(), 0, 1, 0xFFFF);
    // loopback has the one result buffer, rank 0
    int nrecv_known = loopback ? 1 : nranks_known;
    if (nrecv_known >= 0 && k.rank >= nrecv_known)
      bad_args("--corrupt: rank %s has no result buffer", r.c_str());
    corrupts.push_back(k);
  }

  int avail = 0;
  HIPCHECK(hipGetDeviceCount(&avail));
  if (!have_devlist) {
    if (loopback) devs.push_back(0);
    else {
      if (ndev < 0) ndev = avail;
      for (int i = 0; i < ndev; ++i) devs.push_back(i);
    }
  }
  if (loopback) devs.resize(1);
  int ngpu = (int)devs.size();
  if (ngpu == 0 || ngpu > avail || ngpu > MAX_RANKS) {
    fprintf(stderr, "rcclprobe: %d devices requested, %d available (at most %d)\n",
            ngpu, avail, MAX_RANKS);
    return 1;
  }
  for (int d : devs)
    if (d >= avail) {
      fprintf(stderr, "rcclprobe: device %d requested, %d available\n", d, avail);
      return 1;
    }
  // n ranks, each with a send buffer; nrecv result buffers
  int n = loopback ? loopback : ngpu;
  int nrecv = loopback ? 1 : ngpu;
  for (const Corrupt& k : corrupts)
    if (k.rank >= nrecv) {
      fprintf(stderr, "rcclprobe: --corrupt: rank %d has no result buffer\n", k.rank);
      return 2;
    }
  auto dev_of = [&](int rank) { return loopback ? devs[0] : devs[rank]; };

  std::vector<void*> send(n), recv(nrecv);
  std::vector<hipStream_t> streams(nrecv);
  for (int i = 0; i < n; ++i) {
    HIPCHECK(hipSetDevice(dev_of(i)));
    HIPCHECK(hipMalloc(&send[i], count * 2));
    // timed loop: bf16 1.0 everywhere, as in the recorded profiles
    hipLaunchKernelGGL(fill_const_bf16, dim3(FILL_BLOCKS), dim3(BLOCK_THREADS), 0,
                       nullptr, (unsigned short*)send[i], count,
                       (unsigned short)0x3F80);
    HIPCHECK(hipGetLastError());
    HIPCHECK(hipDeviceSynchronize());
  }
  for (int i = 0; i < nrecv; ++i) {
    HIPCHECK(hipSetDevice(dev_of(i)));
    HIPCHECK(hipMalloc(&recv[i], count * 2));
    HIPCHECK(hipStreamCreate(&streams[i]));
  }

  std::vector<ncclComm_t> comms;
  SrcTable table;
  memset(&table, 0, sizeof(table));
  if (loopback) {
    for (int i = 0; i < n; ++i) table.p[i] = (const unsigned short*)send[i];
  } else {
    comms.resize(n);
    NCCLCHECK(ncclCommInitAll(comms.data(), n, devs.data()));
  }

  auto run_iter = [&]() {
    if (loopback) {
      hipLaunchKernelGGL(reduce_sum_bf16, dim3(REDUCE_BLOCKS), dim3(BLOCK_THREADS),
                         0, streams[0], table, n, (unsigned short*)recv[0], count);
      HIPCHECK(hipGetLastError());
      return;
    }
    NCCLCHECK(ncclGroupStart());
    for (int i = 0; i < n; ++i)
      NCCLCHECK(ncclAllReduce(send[i], recv[i], count, ncclBfloat16, ncclSum,
                              comms[i], streams[i]));
    NCCLCHECK(ncclGroupEnd());
  };
  auto sync_all = [&]() {
    for (int i = 0; i < nrecv; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      HIPCHECK(hipStreamSynchronize(streams[i]));
    }
  };

  for (int w = 0; w < warmup; ++w) run_iter();
  sync_all();

  auto t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < iters; ++it) run_iter();
  sync_all();
  auto t1 = std::chrono::steady_clock::now();

  CheckState st;
  if (check) {
    // 1. pattern into every send, 0xFFFF into every recv
    for (int i = 0; i < n; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      hipLaunchKernelGGL(fill_pattern_bf16, dim3(FILL_BLOCKS), dim3(BLOCK_THREADS),
                         0, nullptr, (unsigned short*)send[i], count, seed, i);
      HIPCHECK(hipGetLastError());
    }
    for (int i = 0; i < nrecv; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      hipLaunchKernelGGL(fill_const_bf16, dim3(FILL_BLOCKS), dim3(BLOCK_THREADS), 0,
                         nullptr, (unsigned short*)recv[i], count,
                         (unsigned short)0xFFFF);
      HIPCHECK(hipGetLastError());
    }
    for (int i = 0; i < n; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      HIPCHECK(hipDeviceSynchronize());
    }
    // 2. one untimed all-reduce
    run_iter();
    sync_all();
    for (const Corrupt& k : corrupts) {
      HIPCHECK(hipSetDevice(dev_of(k.rank)));
      unsigned short* p = (unsigned short*)recv[k.rank] + k.index;
      unsigned short v = 0;
      HIPCHECK(hipMemcpy(&v, p, 2, hipMemcpyDeviceToHost));
      v ^= k.mask;
      HIPCHECK(hipMemcpy(p, &v, 2, hipMemcpyHostToDevice));
    }
    // 3. every recv against the n-rank sum, 4. every send against its own
    std::vector<u64*> d_res(nrecv, nullptr);
    for (int i = 0; i < nrecv; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      HIPCHECK(hipMalloc(&d_res[i], RES_SLOTS * sizeof(u64)));
      verify_buffer(st, recv[i], count, seed, 0, n, i, "recv", d_res[i]);
    }
    for (int i = 0; i < n; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      verify_buffer(st, send[i], count, seed, i, 1, i, "send",
                    d_res[loopback ? 0 : i]);
    }
    for (int i = 0; i < nrecv; ++i) {
      HIPCHECK(hipSetDevice(dev_of(i)));
      HIPCHECK(hipFree(d_res[i]));
    }
    if (!dump_dir.empty()) {
      if (mkdir(dump_dir.c_str(), 0777) != 0 && errno != EEXIST) {
        fprintf(stderr, "rcclprobe: cannot create %s: %s\n", dump_dir.c_str(),
                strerror(errno));
        return 1;
      }
      for (int i = 0; i < n; ++i) {
        HIPCHECK(hipSetDevice(dev_of(i)));
        dump_buffer(dump_dir, "send", i, send[i], count);
      }
      for (int i = 0; i < nrecv; ++i) {
        HIPCHECK(hipSetDevice(dev_of(i)));
        dump_buffer(dump_dir, "recv", i, recv[i], count);
      }
    }
  }

  double sec = std::chrono::duration<double>(t1 - t0).count();
  double per_iter = sec / iters;
  double algbw = (double)(count * 2) / per_iter / 1e9;  // GB/s per rank payload
  // loopback moves nothing over a bus: busbw repeats algbw there
  double factor = (!loopback && n > 1) ? 2.0 * (n - 1) / n : 1.0;
  double busbw = algbw * factor;
  bool failed = check && st.mismatches != 0;

  char head[512];
  snprintf(head, sizeof(head),
           "{\"ndev\": %d, \"bytes\": %lld, \"iters\": %d, \"warmup\": %d, "
           "\"time_ms_per_iter\": %.3f, \"algbw_gbps\": %.2f, \"busbw_gbps\": %.2f, "
           "\"dtype\": \"bf16\", \"check\": \"%s\", \"mode\": \"%s\", \"seed\": %u",
           n, (long long)(count * 2), iters, warmup, per_iter * 1e3, algbw, busbw,
           !check ? "skipped" : failed ? "fail" : "pass",
           loopback ? "loopback" : "rccl", seed);
  std::string out = head;
  if (check) {
    char tmp[128];
    snprintf(tmp, sizeof(tmp), ", \"checked_elements\": %llu, \"mismatches\": %llu, ",
             st.checked, st.mismatches);
    out += tmp;
    out += "\"first_bad\": ";
    if (st.have_first) append_record(out, st.first_bad);
    else out += "null";
    out += ", \"records\": [";
    for (size_t r = 0; r < st.records.size(); ++r) {
      if (r) out += ", ";
      append_record(out, st.records[r]);
    }
    out += "]";
  }
  char tail[128];
  snprintf(tail, sizeof(tail),
           ", \"fill_blocks\": %d, \"verify_blocks\": %d, \"block_threads\": %d}",
           FILL_BLOCKS, VERIFY_BLOCKS, BLOCK_THREADS);
  out += tail;
  printf("%s\n", out.c_str());
  fflush(stdout);

  for (size_t i = 0; i < comms.size(); ++i) NCCLCHECK(ncclCommDestroy(comms[i]));
  for (int i = 0; i < n; ++i) {
    HIPCHECK(hipSetDevice(dev_of(i)));
    HIPCHECK(hipFree(send[i]));
  }
  for (int i = 0; i < nrecv; ++i) {
    HIPCHECK(hipSetDevice(dev_of(i)));
    HIPCHECK(hipFree(recv[i]));
    HIPCHECK(hipStreamDestroy(streams[i]));
  }
  if (failed) {
    fprintf(stderr, "rcclprobe: NUMERICS CHECK FAILED (%llu bad elements)\n",
            st.mismatches);
    return 3;
  }
  return 0;
}
