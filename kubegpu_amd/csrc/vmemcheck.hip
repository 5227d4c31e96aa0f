// vmemcheck — integrity kernel for the vector-memory and cache paths
// (gfx950), compiled into _gpuprobe.
//
// The twin of ldscheck.hip for global memory: the path between a wave's
// registers and the L2 (address coalescer and data-return formatter, the
// per-CU vector L1, the scalar data cache, the L2's byte-masked partial
// writes, the cache-policy bits, the buffer-resource range check), which
// memcheck reaches only with lane-linear 16-byte nontemporal accesses.
// Every wave of the launch runs the same deterministic workload and
// compares four 32-bit digests per round with a table the host computed in
// numpy (probe/vmemcheck.py holds the definition of every operand, address
// and digest):
//   stage 0 width    global stores and loads of 1, 2, 4, 8, 12 and 16 bytes,
//                    zero- and sign-extending narrow loads, a dword load
//                    behind every narrow store, reads at rotated lanes
//   stage 1 gather   reads of the shared table X: strided and free gathers
//                    of 4, 8 and 16 bytes under the plain, sc1 and nt
//                    policies, narrow gathers, uniform loads of 1 to 16
//                    dwords through the scalar cache and one of them again
//                    through the vector L1
//   stage 2 partial  dwords assembled from four lanes' byte stores and two
//                    lanes' 16-bit stores on top of a fill still in flight,
//                    dword scatters under each store policy, an 8-byte
//                    scatter, read back plain and sc1
//   stage 3 buffer   raw buffer loads of 1 to 16 bytes and stores of 1, 4 and
//                    16 bytes through a resource whose num_records cuts the
//                    region in two: loads beyond it return 0, stores beyond
//                    it are dropped; an soffset and an immediate-offset form
// Every op is a move, so the reference is exact.
//
// Global wave g owns the span of VM_SPAN dwords at arena dword VM_SPAN * g
// and touches no other; X is only read.  Whatever is stored to absolute
// arena dword a is value ^ vm_tag(a), and whatever is loaded from the
// address the lane meant is XORed with that address's tag before it is
// folded: the tags cancel on healthy hardware, so the table is the same
// for every wave, and a line that answers for the wrong address leaves a
// tag difference in the digest.  Between a store and an access to the same
// bytes by another lane stands a workgroup-scope release / acquire fence
// pair, for which the compiler emits no cache maintenance on gfx950; there
// is no agent-scope fence in the round loop.  Inputs are word(40 + stage,
// r % VM_PERIOD, idx) of cucheck_common.h.  No inline assembly: builtins
// and typed accesses only, every store a vector store.  A failed range
// check lands inside the wave's own span.  Launch shape and accounting are
// cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#define VM_DEV __device__ __forceinline__

#define VM_STAGE0 40u  // stage number fed to cu_base() is VM_STAGE0 + stage
#define VM_PERIOD 64u
#define VM_VALUE_SLOTS 128u  // rows of vmemcheck_values' output, >= any stage's
#define VM_SPAN 4096u        // arena dwords of a wave
#define VM_IMG0 4096u        // word index of img(0)
#define VM_WIDTH0 0u         // first span dword and dwords of each stage's region
#define VM_WIDTH 1024u
#define VM_PARTIAL0 1024u
#define VM_PARTIAL 512u
#define VM_BUFFER0 2048u
#define VM_BUFFER 1024u
#define VM_X_DWORDS 65536u
#define VM_X_BYTES (4u * VM_X_DWORDS)
#define VM_CELLS 256u       // 16-byte cells of the buffer region
#define VM_BUFFER_IMM 256u  // immediate offset of the last load variant
static_assert(VM_WIDTH0 + VM_WIDTH <= VM_PARTIAL0 && VM_PARTIAL0 + VM_PARTIAL <= VM_BUFFER0 &&
                  VM_BUFFER0 + VM_BUFFER <= VM_SPAN && 16u * VM_CELLS == 4u * VM_BUFFER,
              "the regions lie inside the span, one behind the other");
static_assert((size_t)MAX_BLOCKS * CU_WAVES * VM_SPAN <= (1ull << 32),
              "an arena dword index fits a u32");

// probe/vmemcheck.py holds the same tables
constexpr u32 VM_GATHER_STRIDES[] = {0, 1, 2, 3, 8, 16, 33};  // in units of the access
constexpr u32 VM_BUFFER_STRIDES[] = {4, 5, 7, 8, 11, 16};     // cells, b8 .. b128
#define VM_N_GATHER 7u
#define VM_N_BUFFER 6u
enum : u32 { VM_PLAIN = 0, VM_SC1 = 1, VM_NT = 2 };  // POLICIES of vmemcheck.py

// Every access to the arena goes through one of these, whole: accesses of
// different widths to the same bytes must stay in program order.  The
// attribute has to sit on a struct: on a typedef it is lost where the type
// becomes a template argument (ldscheck.hip has the story).
typedef u32 vm_v2 __attribute__((ext_vector_type(2)));
typedef u32 vm_v3 __attribute__((ext_vector_type(3)));
typedef u32 vm_v4 __attribute__((ext_vector_type(4)));
typedef unsigned long long vm_u64;
struct __attribute__((may_alias)) vm_b {
  unsigned char x;
};
struct __attribute__((may_alias)) vm_sb {
  signed char x;
};
struct __attribute__((may_alias)) vm_h {
  unsigned short x;
};
struct __attribute__((may_alias)) vm_sh {
  short x;
};
struct __attribute__((may_alias)) vm_w {
  u32 x;
};
struct __attribute__((may_alias)) vm_w2 {
  vm_v2 x;
};
struct __attribute__((may_alias, aligned(4))) vm_w3 {  // 12 bytes aligned to 4
  u32 x[3];
};
struct __attribute__((may_alias)) vm_w4 {
  vm_v4 x;
};
template <u32 N>
struct VmVec;
template <>
struct VmVec<1> {
  typedef vm_w T;
};
template <>
struct VmVec<2> {
  typedef vm_w2 T;
};
template <>
struct VmVec<3> {
  typedef vm_w3 T;
};
template <>
struct VmVec<4> {
  typedef vm_w4 T;
};
// N dwords of the read-only table for one scalar load, naturally aligned
template <u32 N>
using vm_vn = u32 __attribute__((ext_vector_type(N)));

#if __HIP_DEVICE_COMPILE__

VM_DEV u32 vm_tag(u32 a) { return cu_fmix32(0xA5A5A5A5u ^ (a * 0x9E3779B9u)); }
VM_DEV u32 vm_v(u32 base, u32 k, u32 lane) { return cu_fmix32(base + 64u * k + lane); }
VM_DEV u32 vm_u(u32 base, u32 k) { return cu_fmix32(base + 64u * k); }
VM_DEV u32 vm_img(u32 base, u32 i) { return cu_fmix32(base + VM_IMG0 + i); }
// lane (l + u(k)) mod 64, and the bijection ((u(k) | 1) l + (u(k) >> 8)) mod 64
VM_DEV u32 vm_rot(u32 base, u32 k, u32 lane) { return (lane + vm_u(base, k)) & 63u; }
VM_DEV u32 vm_perm(u32 base, u32 k, u32 lane) {
  const u32 u = vm_u(base, k);
  return ((u | 1u) * lane + (u >> 8)) & 63u;
}

// dword c of a value of 1 to 4 dwords
VM_DEV u32 vm_get(const vm_w& v, u32) { return v.x; }
template <typename V>
VM_DEV u32 vm_get(const V& v, u32 c) { return v.x[c]; }
VM_DEV void vm_set(vm_w& v, u32, u32 x) { v.x = x; }
template <typename V>
VM_DEV void vm_set(V& v, u32 c, u32 x) { v.x[c] = x; }

// the first active lane's value of a word that is the same in every lane,
// unsigned (the builtin returns an int, which would be sign-extended where
// it becomes half of a pointer)
VM_DEV u32 vm_first(u32 x) { return (u32)__builtin_amdgcn_readfirstlane(x); }

// A stage's region of the wave's span: where it starts, and the absolute
// arena dword index of that place.  Dword and byte numbers are relative
// to it and reduced into the region before they are used.
struct VmRegion {
  unsigned char* p;
  u32 a0;
};

template <typename T>
VM_DEV T* vm_at(const VmRegion& g, u32 byte) {
  return (T*)(g.p + byte);
}

// the workgroup-scope release / acquire pair between a store and an
// access to the same bytes by another lane
VM_DEV void vm_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Where a stage's values go: into the digest, or into the element dump
// (row `slot`, column lane) of the one wave that is asked for.
struct VmFold {
  u32 d = 0;
  VM_DEV void put(u32 slot, u32 lane, u32 v) { d += cu_fmix32(v + cu_salt(64u * slot + lane)); }
};

struct VmDump {
  u32* out;
  bool on;
  VM_DEV void put(u32 slot, u32 lane, u32 v) {
    if (on) out[64u * slot + lane] = v;
  }
};

// N dwords at p under a cache policy.  sc1 is a relaxed agent-scope atomic
// of 4 or 8 bytes (16 bytes are two of 8: there is no wider one), nt the
// nontemporal builtin.
template <u32 N>
VM_DEV void vm_load(const unsigned char* p, u32 pol, u32 (&x)[N]) {
  static_assert(N == 1u || N == 2u || N == 4u, "policies exist for 4, 8 and 16 bytes");
  if (pol == VM_SC1) {
    if constexpr (N == 1u) {
      x[0] = __hip_atomic_load((const u32*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
#pragma unroll
      for (u32 c = 0; c < N; c += 2u) {
        const vm_u64 q = __hip_atomic_load((const vm_u64*)p + c / 2u, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
        x[c] = (u32)q;
        x[c + 1u] = (u32)(q >> 32);
      }
    }
  } else if (pol == VM_NT) {
    if constexpr (N == 1u) {
      x[0] = __builtin_nontemporal_load((const u32*)p);
    } else if constexpr (N == 2u) {
      const vm_v2 q = __builtin_nontemporal_load((const vm_v2*)p);
      x[0] = q.x, x[1] = q.y;
    } else {
      const vm_v4 q = __builtin_nontemporal_load((const vm_v4*)p);
      x[0] = q.x, x[1] = q.y, x[2] = q.z, x[3] = q.w;
    }
  } else {
    const typename VmVec<N>::T q = *(const typename VmVec<N>::T*)p;
#pragma unroll
    for (u32 c = 0; c < N; ++c) x[c] = vm_get(q, c);
  }
}

// N dwords of operand slots k0 .. at region dword d, tagged, as one store
template <u32 N>
VM_DEV void vm_write(const VmRegion& g, u32 d, u32 base, u32 k0, u32 lane) {
  typename VmVec<N>::T x;
#pragma unroll
  for (u32 c = 0; c < N; ++c) vm_set(x, c, vm_v(base, k0 + c, lane) ^ vm_tag(g.a0 + d + c));
  *vm_at<typename VmVec<N>::T>(g, 4u * d) = x;
}

// N dwords at region dword d into N slots, the tags removed
template <u32 N, typename SINK>
VM_DEV void vm_read(const VmRegion& g, u32 d, u32 pol, u32& n, u32 lane, SINK& sink) {
  u32 x[N];
  if constexpr (N == 3u) {
    const vm_w3 q = *vm_at<vm_w3>(g, 4u * d);
#pragma unroll
    for (u32 c = 0; c < 3u; ++c) x[c] = q.x[c];
  } else {
    vm_load<N>(g.p + 4u * d, pol, x);
  }
#pragma unroll
  for (u32 c = 0; c < N; ++c) sink.put(n++, lane, x[c] ^ vm_tag(g.a0 + d + c));
}

// the first `dwords` dwords of the region from the image, tagged, by
// 16-byte stores, lane-linear
VM_DEV void vm_fill(const VmRegion& g, u32 base, u32 dwords, u32 lane) {
  for (u32 t = 0; t < dwords / 256u; ++t) {
    const u32 i = 4u * (64u * t + lane);
    vm_w4 x;
#pragma unroll
    for (u32 c = 0; c < 4u; ++c) x.x[c] = vm_img(base, i + c) ^ vm_tag(g.a0 + i + c);
    *vm_at<vm_w4>(g, 4u * i) = x;
  }
}

// the tag byte / half a narrow load at `byte` of the region meets,
// extended like the load (spelled so that the compiler does not extend
// after the XOR and load unsigned)
VM_DEV u32 vm_tag8(const VmRegion& g, u32 byte, bool sign) {
  const u32 tb = (vm_tag(g.a0 + (byte >> 2)) >> (8u * (byte & 3u))) & 0xFFu;
  return sign ? tb | ((0u - (tb >> 7)) << 8) : tb;
}
VM_DEV u32 vm_tag16(const VmRegion& g, u32 byte, bool sign) {
  const u32 th = (vm_tag(g.a0 + (byte >> 2)) >> (8u * (byte & 2u))) & 0xFFFFu;
  return sign ? th | ((0u - (th >> 15)) << 16) : th;
}

// ---- stage 0: every access width, inside the width region

template <typename SINK>
VM_DEV u32 vm_stage_width(u32 base, const VmRegion& g, u32 lane, SINK& sink) {
  u32 n = 0;
  vm_fill(g, base, VM_WIDTH, lane);
  vm_fence();
  // narrow stores: each followed by its whole dword and the next one;
  // then a lane reads, zero- and sign-extended, the byte or half that
  // lane (l + u) mod 64 stored
#pragma unroll
  for (u32 j = 0; j < 2u; ++j) {
    const u32 d = 2u * lane + j, b = (lane + vm_u(base, 0u) + j) & 3u;
    const u32 val = (vm_v(base, 1u + j, lane) & 0x7Fu) | (((lane >> 2) & 1u) << 7);
    *vm_at<vm_b>(g, 4u * d + b) = vm_b{(unsigned char)(val ^ vm_tag8(g, 4u * d + b, false))};
    vm_fence();
    vm_read<1u>(g, 2u * lane, VM_PLAIN, n, lane, sink);
    vm_read<1u>(g, 2u * lane + 1u, VM_PLAIN, n, lane, sink);
    {
      const u32 rl = vm_rot(base, 27u, lane);
      const u32 at = 4u * (2u * rl + j) + ((rl + vm_u(base, 0u) + j) & 3u);
      const vm_b x = *vm_at<vm_b>(g, at);
      sink.put(n++, lane, (u32)x.x ^ vm_tag8(g, at, false));
    }
    {
      const u32 rl = vm_rot(base, 28u, lane);
      const u32 at = 4u * (2u * rl + j) + ((rl + vm_u(base, 0u) + j) & 3u);
      const vm_sb x = *vm_at<vm_sb>(g, at);
      sink.put(n++, lane, (u32)(int)x.x ^ vm_tag8(g, at, true));
    }
  }
#pragma unroll
  for (u32 j = 0; j < 2u; ++j) {
    const u32 d = 128u + 2u * lane + j, h = (lane + vm_u(base, 3u) + j) & 1u;
    const u32 val = (vm_v(base, 4u + j, lane) & 0x7FFFu) | (((lane >> 1) & 1u) << 15);
    *vm_at<vm_h>(g, 4u * d + 2u * h) =
        vm_h{(unsigned short)(val ^ vm_tag16(g, 4u * d + 2u * h, false))};
    vm_fence();
    vm_read<1u>(g, 128u + 2u * lane, VM_PLAIN, n, lane, sink);
    vm_read<1u>(g, 129u + 2u * lane, VM_PLAIN, n, lane, sink);
    {
      const u32 rl = vm_rot(base, 29u, lane);
      const u32 at = 4u * (128u + 2u * rl + j) + 2u * ((rl + vm_u(base, 3u) + j) & 1u);
      const vm_h x = *vm_at<vm_h>(g, at);
      sink.put(n++, lane, (u32)x.x ^ vm_tag16(g, at, false));
    }
    {
      const u32 rl = vm_rot(base, 30u, lane);
      const u32 at = 4u * (128u + 2u * rl + j) + 2u * ((rl + vm_u(base, 3u) + j) & 1u);
      const vm_sh x = *vm_at<vm_sh>(g, at);
      sink.put(n++, lane, (u32)(int)x.x ^ vm_tag16(g, at, true));
    }
  }
  // wide accesses: a lane reads what lane (l + u) mod 64 stored
  vm_write<2u>(g, 256u + 2u * lane, base, 7u, lane);
  vm_write<3u>(g, 384u + 4u * lane, base, 9u, lane);
  vm_write<4u>(g, 640u + 4u * lane, base, 14u, lane);
  vm_fence();
  vm_read<2u>(g, 256u + 2u * vm_rot(base, 6u, lane), VM_PLAIN, n, lane, sink);
  vm_read<3u>(g, 384u + 4u * vm_rot(base, 12u, lane), VM_PLAIN, n, lane, sink);
  vm_read<4u>(g, 384u + 4u * vm_rot(base, 13u, lane), VM_PLAIN, n, lane, sink);
  vm_read<4u>(g, 640u + 4u * vm_rot(base, 18u, lane), VM_PLAIN, n, lane, sink);
  return n;
}

// ---- stage 1: gathers from the table X (untagged, only read)

// N dwords of X at byte `at` (reduced into X by the caller) under the
// policy of the first slot's number
template <u32 N, typename SINK>
VM_DEV void vm_gather(const unsigned char* X, u32 at, u32& n, u32 lane, SINK& sink) {
  u32 x[N];
  vm_load<N>(X + at, n % 3u, x);
#pragma unroll
  for (u32 c = 0; c < N; ++c) sink.put(n++, lane, x[c]);
}

// N dwords at the wave-uniform, naturally aligned index (one scalar
// load); lane l takes dword l mod N
template <u32 N>
VM_DEV u32 vm_uniform(const unsigned char* X, u32 index, u32 lane) {
  if constexpr (N == 1u) {
    return *(const u32*)(X + 4u * index);
  } else {
    const vm_vn<N> s = *(const vm_vn<N>*)(X + 4u * N * index);
    u32 x = s[0];
#pragma unroll
    for (u32 c = 1; c < N; ++c) x = (lane % N == c) ? s[c] : x;
    return x;
  }
}

template <typename SINK>
VM_DEV u32 vm_stage_gather(u32 base, const u32* __restrict__ table, u32 lane, SINK& sink) {
  u32 n = 0;
  const unsigned char* X = (const unsigned char*)table;
#pragma unroll
  for (u32 si = 0; si < VM_N_GATHER; ++si)
    vm_gather<1u>(X, 4u * ((lane * VM_GATHER_STRIDES[si] + vm_u(base, si)) & (VM_X_BYTES / 4u - 1u)),
                  n, lane, sink);
#pragma unroll
  for (u32 si = 0; si < VM_N_GATHER; ++si)
    vm_gather<2u>(
        X, 8u * ((lane * VM_GATHER_STRIDES[si] + vm_u(base, 7u + si)) & (VM_X_BYTES / 8u - 1u)), n,
        lane, sink);
#pragma unroll
  for (u32 si = 0; si < VM_N_GATHER; ++si)
    vm_gather<4u>(
        X, 16u * ((lane * VM_GATHER_STRIDES[si] + vm_u(base, 14u + si)) & (VM_X_BYTES / 16u - 1u)),
        n, lane, sink);
  vm_gather<1u>(X, 4u * (vm_v(base, 21u, lane) & (VM_X_BYTES / 4u - 1u)), n, lane, sink);
  vm_gather<2u>(X, 8u * (vm_v(base, 22u, lane) & (VM_X_BYTES / 8u - 1u)), n, lane, sink);
  vm_gather<4u>(X, 16u * (vm_v(base, 23u, lane) & (VM_X_BYTES / 16u - 1u)), n, lane, sink);
  // narrow gathers
  {
    const vm_b x = *(const vm_b*)(X + (vm_v(base, 24u, lane) & (VM_X_BYTES - 1u)));
    sink.put(n++, lane, (u32)x.x);
  }
  {
    const vm_sb x = *(const vm_sb*)(X + (vm_v(base, 25u, lane) & (VM_X_BYTES - 1u)));
    sink.put(n++, lane, (u32)(int)x.x);
  }
  {
    const vm_h x = *(const vm_h*)(X + 2u * (vm_v(base, 26u, lane) & (VM_X_BYTES / 2u - 1u)));
    sink.put(n++, lane, (u32)x.x);
  }
  {
    const vm_sh x = *(const vm_sh*)(X + 2u * (vm_v(base, 27u, lane) & (VM_X_BYTES / 2u - 1u)));
    sink.put(n++, lane, (u32)(int)x.x);
  }
  // uniform loads: the index is wave-uniform, so the scalar unit loads
#define VM_UNI(k) vm_first(vm_u(base, (k)))
  sink.put(n++, lane, vm_uniform<1u>(X, VM_UNI(28u) % (VM_X_DWORDS / 1u), lane));
  sink.put(n++, lane, vm_uniform<2u>(X, VM_UNI(29u) % (VM_X_DWORDS / 2u), lane));
  sink.put(n++, lane, vm_uniform<4u>(X, VM_UNI(30u) % (VM_X_DWORDS / 4u), lane));
  sink.put(n++, lane, vm_uniform<8u>(X, VM_UNI(31u) % (VM_X_DWORDS / 8u), lane));
  // the block that holds the first uniform load's dword, and the same
  // block again through the vector path
  const u32 block = (VM_UNI(28u) % VM_X_DWORDS) / 16u;
  sink.put(n++, lane, vm_uniform<16u>(X, block, lane));
#undef VM_UNI
  {
    const vm_w x = *(const vm_w*)(X + 4u * (16u * block + (lane & 15u)));
    sink.put(n++, lane, x.x);
  }
  return n;
}

// ---- stage 2: partial-line writes, inside the partial region

template <typename SINK>
VM_DEV u32 vm_stage_partial(u32 base, const VmRegion& g, u32 lane, SINK& sink) {
  u32 n = 0;
  vm_fill(g, base, VM_PARTIAL, lane);
  // no fence: the narrow stores meet the fill on its way.  Every byte is
  // stored once after the fill, so the result does not depend on the
  // order of the lanes.
#pragma unroll
  for (u32 j = 0; j < 4u; ++j) {
    const u32 d = vm_perm(base, j, lane), at = 4u * d + ((d + j) & 3u);
    *vm_at<vm_b>(g, at) =
        vm_b{(unsigned char)(vm_v(base, 4u + j, lane) ^ vm_tag8(g, at, false))};
  }
#pragma unroll
  for (u32 j = 0; j < 2u; ++j) {
    const u32 d = 64u + vm_perm(base, 8u + j, lane), at = 4u * d + 2u * ((d + j) & 1u);
    *vm_at<vm_h>(g, at) =
        vm_h{(unsigned short)(vm_v(base, 10u + j, lane) ^ vm_tag16(g, at, false))};
  }
#pragma unroll
  for (u32 j = 0; j < 4u; ++j) {
    const u32 d = 128u + 64u * j + vm_perm(base, 12u + j, lane);
    const u32 val = vm_v(base, 16u + j, lane) ^ vm_tag(g.a0 + d);
    if (j == 1u)
      __hip_atomic_store(vm_at<u32>(g, 4u * d), val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (j == 2u)
      __builtin_nontemporal_store(val, vm_at<u32>(g, 4u * d));
    else
      *vm_at<vm_w>(g, 4u * d) = vm_w{val};
  }
  vm_write<2u>(g, 384u + 2u * vm_perm(base, 20u, lane), base, 21u, lane);
  vm_fence();
  for (u32 t = 0; t < VM_PARTIAL / 256u; ++t)
    vm_read<4u>(g, 4u * (64u * t + lane), VM_PLAIN, n, lane, sink);
  for (u32 t = 0; t < VM_PARTIAL / 256u; ++t)
    vm_read<4u>(g, 4u * (64u * t + lane), VM_SC1, n, lane, sink);
  return n;
}

// ---- stage 3: the buffer-resource range check, inside the buffer region

// what a buffer load of `bytes` bytes at byte `at` returned, into the
// sink: tags removed where the lane is expected in range
template <u32 N, typename SINK>
VM_DEV void vm_buffer_put(const VmRegion& g, const u32 (&x)[N], u32 at, bool in_range, u32& n,
                          u32 lane, SINK& sink) {
#pragma unroll
  for (u32 c = 0; c < N; ++c)
    sink.put(n++, lane, in_range ? x[c] ^ vm_tag(g.a0 + (at >> 2) + c) : x[c]);
}

template <typename SINK>
VM_DEV u32 vm_stage_buffer(u32 base, const VmRegion& g, u32 lane, SINK& sink) {
  u32 n = 0;
  vm_fill(g, base, VM_BUFFER, lane);
  vm_fence();
  // num_records: a multiple of 16 in 1536 .. 3056.  The resource is built
  // from values the compiler can see are wave-uniform.
  const u32 N = 16u * (96u + vm_first(vm_u(base, 0u)) % 96u);
  const vm_u64 pa = (vm_u64)g.p;
  void* p = (void*)(((vm_u64)vm_first((u32)(pa >> 32)) << 32) | vm_first((u32)pa));
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(p, 0, (int)N, 0x00020000);
#define VM_CELL(wi) ((lane * VM_BUFFER_STRIDES[wi] + vm_u(base, 1u + (wi))) & (VM_CELLS - 1u))
  {
    const u32 cell = VM_CELL(0u), at = 16u * cell + (vm_v(base, 8u, lane) & 15u);
    const u32 x = __builtin_amdgcn_raw_buffer_load_b8(rsrc, (int)at, 0, 0);
    sink.put(n++, lane, 16u * cell < N ? x ^ vm_tag8(g, at, false) : x);
  }
  {
    const u32 cell = VM_CELL(1u), at = 16u * cell + 2u * (vm_v(base, 9u, lane) & 7u);
    const u32 x = __builtin_amdgcn_raw_buffer_load_b16(rsrc, (int)at, 0, 0);
    sink.put(n++, lane, 16u * cell < N ? x ^ vm_tag16(g, at, false) : x);
  }
  {
    const u32 cell = VM_CELL(2u), at = 16u * cell + 4u * (vm_v(base, 10u, lane) & 3u);
    const u32 x[1] = {__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)at, 0, 0)};
    vm_buffer_put(g, x, at, 16u * cell < N, n, lane, sink);
  }
  {
    const u32 cell = VM_CELL(3u), at = 16u * cell + 8u * (vm_v(base, 11u, lane) & 1u);
    const vm_v2 q = __builtin_amdgcn_raw_buffer_load_b64(rsrc, (int)at, 0, 0);
    const u32 x[2] = {q.x, q.y};
    vm_buffer_put(g, x, at, 16u * cell < N, n, lane, sink);
  }
  {
    const u32 cell = VM_CELL(4u), at = 16u * cell + 4u * (vm_v(base, 12u, lane) & 1u);
    const vm_v3 q = __builtin_amdgcn_raw_buffer_load_b96(rsrc, (int)at, 0, 0);
    const u32 x[3] = {q.x, q.y, q.z};
    vm_buffer_put(g, x, at, 16u * cell < N, n, lane, sink);
  }
  {
    const u32 cell = VM_CELL(5u), at = 16u * cell;
    const vm_v4 q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)at, 0, 0);
    const u32 x[4] = {q.x, q.y, q.z, q.w};
    vm_buffer_put(g, x, at, 16u * cell < N, n, lane, sink);
  }
#undef VM_CELL
  // with an soffset and with an immediate offset: below 1536 <= N with
  // every part counted, so in range whichever parts the check counts
  {
    const u32 voff = 4u * ((lane * 5u + vm_u(base, 14u)) & 255u);
    const u32 soff = 16u * (vm_first(vm_u(base, 15u)) & 15u);
    const u32 x[1] = {__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)voff, (int)soff, 0)};
    vm_buffer_put(g, x, voff + soff, true, n, lane, sink);
  }
  {
    const u32 voff = 16u * ((lane + vm_u(base, 16u)) & 63u);
    const vm_v4 q = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(voff + VM_BUFFER_IMM), 0, 0);
    const u32 x[4] = {q.x, q.y, q.z, q.w};
    vm_buffer_put(g, x, voff + VM_BUFFER_IMM, true, n, lane, sink);
  }
  vm_fence();
  // stores at bijective cells over the whole region: those at or above N
  // must be dropped
  {
    const u32 at = 16u * (4u * vm_perm(base, 19u, lane));
    vm_v4 q;
#pragma unroll
    for (u32 c = 0; c < 4u; ++c) q[c] = vm_v(base, 20u + c, lane) ^ vm_tag(g.a0 + (at >> 2) + c);
    __builtin_amdgcn_raw_buffer_store_b128(q, rsrc, (int)at, 0, 0);
  }
  {
    const u32 at = 16u * (4u * vm_perm(base, 24u, lane) + 1u) + 4u * (vm_v(base, 28u, lane) & 3u);
    __builtin_amdgcn_raw_buffer_store_b32(vm_v(base, 25u, lane) ^ vm_tag(g.a0 + (at >> 2)), rsrc,
                                          (int)at, 0, 0);
  }
  {
    const u32 at = 16u * (4u * vm_perm(base, 26u, lane) + 2u) + (vm_v(base, 29u, lane) & 15u);
    __builtin_amdgcn_raw_buffer_store_b8(
        (unsigned char)(vm_v(base, 27u, lane) ^ vm_tag8(g, at, false)), rsrc, (int)at, 0, 0);
  }
  vm_fence();
  for (u32 t = 0; t < VM_BUFFER / 256u; ++t)
    vm_read<4u>(g, 4u * (64u * t + lane), VM_PLAIN, n, lane, sink);
  return n;
}

// the region of a stage in the span that starts at arena dword `span`
VM_DEV VmRegion vm_region(u32* arena, u32 span, u32 first) {
  return {(unsigned char*)(arena + (size_t)span + first), span + first};
}

#endif  // __HIP_DEVICE_COMPILE__

__global__ void __launch_bounds__(CU_BLOCK)
vmemcheck_kernel(CuArgs a, u32* arena, const u32* __restrict__ table) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % VM_PERIOD;
    // r >> 17 is 0, as rounds <= MAX_ROUNDS, but the compiler cannot know:
    // it would otherwise compute the tag of every address once, ahead of
    // the loop, and keep them in scratch memory (ldscheck.hip)
    const u32 span = w.gwave * VM_SPAN + (r >> 17);
    // each stage's digest is summed where the stage ends, so that its
    // values are folded while they are in registers (ldscheck.hip)
    VmFold f0, f1, f2, f3;
    vm_stage_width(cu_base(a.seed, VM_STAGE0 + 0, rp), vm_region(arena, span, VM_WIDTH0), lane,
                   f0);
    const u32 d0 = wave_sum(f0.d);
    vm_stage_gather(cu_base(a.seed, VM_STAGE0 + 1, rp), table, lane, f1);
    const u32 d1 = wave_sum(f1.d);
    vm_stage_partial(cu_base(a.seed, VM_STAGE0 + 2, rp), vm_region(arena, span, VM_PARTIAL0),
                     lane, f2);
    const u32 d2 = wave_sum(f2.d);
    vm_stage_buffer(cu_base(a.seed, VM_STAGE0 + 3, rp), vm_region(arena, span, VM_BUFFER0), lane,
                    f3);
    u32 dig[N_STAGES] = {d0, d1, d2, wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One full workgroup runs one stage and round, each wave on its own span,
// and wave `wave` of it writes every value it would fold, out[64 * slot +
// lane], and the number of slots behind the last row.  A digest cannot
// say which access moved what; this can.
__global__ void __launch_bounds__(CU_BLOCK)
vmemcheck_values_kernel(u32 seed, u32 stage, u32 r, u32 wave, u32* arena,
                        const u32* __restrict__ table, u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  const u32 lane = threadIdx.x % WAVE, wib = threadIdx.x / WAVE;
  const u32 base = cu_base(seed, VM_STAGE0 + stage, r % VM_PERIOD);
  const u32 span = wib * VM_SPAN;
  VmDump sink;
  sink.out = out;
  sink.on = wib == wave;
  u32 n;
  if (stage == 0u) n = vm_stage_width(base, vm_region(arena, span, VM_WIDTH0), lane, sink);
  else if (stage == 1u) n = vm_stage_gather(base, table, lane, sink);
  else if (stage == 2u) n = vm_stage_partial(base, vm_region(arena, span, VM_PARTIAL0), lane, sink);
  else n = vm_stage_buffer(base, vm_region(arena, span, VM_BUFFER0), lane, sink);
  if (threadIdx.x == 0u) out[64u * VM_VALUE_SLOTS] = n;
#endif
}

// ---------------------------------------------------------------- host

static void vm_check_memory(const at::Tensor& arena, const at::Tensor& table,
                            const at::Device& device, int64_t blocks) {
  TORCH_CHECK(arena.is_cuda() && arena.device() == device,
              "vmemcheck: arena must be on the GPU that runs the kernel");
  TORCH_CHECK(arena.scalar_type() == at::kInt && arena.is_contiguous(),
              "vmemcheck: arena must be a contiguous int32 tensor");
  TORCH_CHECK(arena.numel() == blocks * CU_WAVES * (int64_t)VM_SPAN,
              "vmemcheck: arena must hold ", blocks * CU_WAVES * (int64_t)VM_SPAN,
              " elements (", blocks, " blocks x 16 waves x 4096), got ", arena.numel());
  TORCH_CHECK(table.is_cuda() && table.device() == device,
              "vmemcheck: table must be on the GPU that runs the kernel");
  TORCH_CHECK(table.scalar_type() == at::kInt && table.is_contiguous(),
              "vmemcheck: table must be a contiguous int32 tensor");
  TORCH_CHECK(table.numel() == (int64_t)VM_X_DWORDS, "vmemcheck: table must hold ", VM_X_DWORDS,
              " elements (X[65536]), got ", table.numel());
}

// `arena` (int32, blocks x 16 x VM_SPAN elements) is the waves' scratch
// memory, `table` (int32, VM_X_DWORDS elements, probe/vmemcheck.py's
// source_table) is only read.
CucheckOut vmemcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                         int64_t blocks_arg, at::Tensor arena, at::Tensor table,
                         int64_t max_records, c10::optional<at::Tensor> dump,
                         c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("vmemcheck", expected, seed_arg, rounds, blocks_arg, max_records,
                          dump, inject);
  vm_check_memory(arena, table, expected.device(), l.blocks);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  // the LDS is asked for only to keep a second workgroup off the CU
  return cu_launch_timed(vmemcheck_kernel, l, MAX_LDS_BYTES, (u32*)arena.data_ptr(),
                         (const u32*)table.data_ptr());
}

// What wave `wave` of a workgroup folds for one stage and round as an
// int32 tensor on the table's GPU: VM_VALUE_SLOTS rows of 64 lanes, then
// the number of rows the stage filled.  `arena` holds one workgroup's
// spans.
at::Tensor vmemcheck_values(int64_t seed_arg, int64_t stage, int64_t round, at::Tensor arena,
                            at::Tensor table, int64_t wave) {
  cu_check_wave_args("vmemcheck", seed_arg, stage, round);
  TORCH_CHECK(wave >= 0 && wave < CU_WAVES, "vmemcheck: wave must be in 0..", CU_WAVES - 1,
              ", got ", wave);
  TORCH_CHECK(table.is_cuda(), "vmemcheck: table must be on the GPU that runs the kernel");
  vm_check_memory(arena, table, table.device(), 1);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(table));
  at::Tensor out = at::zeros({(int64_t)(64 * VM_VALUE_SLOTS + 1)},
                             table.options().dtype(at::kInt));
  return cu_launch_values(vmemcheck_values_kernel, CU_BLOCK, MAX_LDS_BYTES, out, (u32)seed_arg,
                          (u32)stage, (u32)round, (u32)wave, (u32*)arena.data_ptr(),
                          (const u32*)table.data_ptr(), (u32*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/vmemcheck_mi355x.json).
void bind_vmemcheck(py::module_& m) {
  m.def("vmemcheck_run", &vmemcheck_run,
        "vector-memory integrity run -> (mismatches, first_bad_round, stage_mask, records, "
        "waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("arena"), py::arg("table"), py::arg("max_records") = 16,
        py::arg("dump") = py::none(), py::arg("inject") = py::none());
  m.def("vmemcheck_values", &vmemcheck_values,
        "values one wave of a workgroup folds for one stage and round as int32 "
        "[128 rows * 64 lanes + 1]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"), py::arg("arena"),
        py::arg("table"), py::arg("wave") = 0);
  m.def("vmemcheck_layout", []() {
          std::vector<int64_t> gather(VM_GATHER_STRIDES, VM_GATHER_STRIDES + VM_N_GATHER);
          std::vector<int64_t> buffer(VM_BUFFER_STRIDES, VM_BUFFER_STRIDES + VM_N_BUFFER);
          std::vector<int64_t> sizes = {VM_SPAN, VM_WIDTH0, VM_WIDTH, VM_PARTIAL0, VM_PARTIAL,
                                        VM_BUFFER0, VM_BUFFER, VM_X_DWORDS, VM_CELLS,
                                        VM_BUFFER_IMM};
          return std::make_tuple((int64_t)VM_PERIOD, (int64_t)VM_VALUE_SLOTS, sizes, gather,
                                 buffer);
        },
        "(period, value rows, (span dwords, first dword and dwords of the width, partial "
        "and buffer regions, X dwords, buffer cells, immediate offset), gather strides, "
        "buffer strides)");
}
