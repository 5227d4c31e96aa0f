// atomcheck — integrity kernel for the read-modify-write units (gfx950),
// compiled into _gpuprobe.
//
// The twin of cucheck.hip, mxcheck.hip and fpcheck.hip for hardware none
// of them reaches: the LDS atomic ALUs of every CU, the integer atomic
// units in every XCD's L2 and the memory-side units that execute global
// float atomics.  Every wave of the launch runs the same deterministic
// sequence of atomics and compares four 32-bit digests per round with a
// table the host computed in numpy (probe/atomcheck.py holds the
// definition of every operand, sequence and digest):
//   stage 0 lds  LDS u32 / i32 (13 ops), u64 (add, umin, umax), f32, f64,
//                packed f16 and packed bf16 adds, on the wave's LDS slice,
//                and a phase in which all 16 waves hit 64 shared LDS cells
//   stage 1 g32  the 13 u32 / i32 ops on the wave's slice of the arena
//   stage 2 g64  u64 add, sub, umin, umax, and, or, xor, exchange, cas
//   stage 3 gfp  f32 add, f64 add / min / max, packed f16 / bf16 add
// Each stage has an owned phase (lane l alone on cell l: a store, a
// fixed chain of returning atomics, a load; every returned value is
// folded) and a contended phase (eight lanes per cell, one block of
// eight cells per op; what is folded does not depend on arrival order).
// On some rounds every wave of the grid also applies six non-returning
// ops onto one shared region, whose finals the host checks in closed
// form after the kernel: the one place where contention crosses XCDs.
//
// Inputs are word(16 + stage, r % AT_PERIOD, idx) of cucheck_common.h.
// Every access to the arena is a relaxed atomic at agent scope (workgroup
// scope in the LDS), never a plain load or store; the arena is indexed
// from blockIdx.x, threadIdx.x and constants only.  No wave waits for a
// value of another: the only synchronisation is the three barriers of
// stage 0's cross-wave phase, which all 16 waves reach every round.
// Launch shape and accounting are cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#include <type_traits>

typedef unsigned long long u64;
typedef _Float16 at_h2 __attribute__((ext_vector_type(2)));
typedef short at_s2 __attribute__((ext_vector_type(2)));

#define AT_DEV __device__ __forceinline__
#define AT_RLX __ATOMIC_RELAXED
#define AT_WG __HIP_MEMORY_SCOPE_WORKGROUP
#define AT_AG __HIP_MEMORY_SCOPE_AGENT
#define AT_LDS(T) __attribute__((address_space(3))) T*
#define AT_GLB(T) __attribute__((address_space(1))) T*

#define AT_STAGE0 16u  // stage number fed to cu_base() is AT_STAGE0 + stage
#define AT_PERIOD 64u
// A slice, in 8-byte cells: 64 owned cells, then blocks of 8 contended
// cells.  A wave has one slice in the LDS and three (g32, g64, gfp) in
// the arena; the arena ends with the shared region.
#define AT_BLOCKS 17u
#define AT_SLICE (64u + 8u * AT_BLOCKS)
#define AT_WAVE_CELLS (3u * AT_SLICE)
#define AT_SHARED_ROWS 6u
#define AT_SHARED_CELLS (64u * AT_SHARED_ROWS)
#define AT_CROSS_CELLS 64u
#define AT_LDS_USED (CU_WAVES * AT_SLICE * 8u + AT_CROSS_CELLS * 4u)
#define AT_VALUE_SLOTS 64u  // rows of atomcheck_values' output, >= any stage's
#define NO_DROP 0xFFFFFFFFu

// operand slot k of a stage: words 128 k + lane (low) and 128 k + 64 + lane
#define AT_K_O32 0u    // owned u32: 15 slots
#define AT_K_C32 15u   // contended u32: 2 per op
#define AT_K_O64 35u   // owned u64: 15 slots
#define AT_K_C64 50u   // contended u64: 2 per op
#define AT_K_F 70u     // owned float: 13 slots
#define AT_K_CF 83u    // contended float: 1 per op
#define AT_K_XW 96u    // cross-wave phase: words from 128 * 96 on

// owned integer ops, in sequence order
enum { A_ADD, A_SUB, A_UMIN, A_UMAX, A_SMIN, A_SMAX, A_AND, A_OR, A_XOR,
       A_INC, A_DEC, A_XCHG, A_CAS };
#define AT_OWN_ALL 0x1FFFu
#define AT_OWN_L64 ((1u << A_ADD) | (1u << A_UMIN) | (1u << A_UMAX))
#define AT_OWN_G64 (AT_OWN_ALL & ~((1u << A_SMIN) | (1u << A_SMAX) | (1u << A_INC) | \
                                   (1u << A_DEC)))
// contended integer ops, in block order
enum { C_ADD, C_AND, C_OR, C_XOR, C_UMIN, C_UMAX, C_SMIN, C_SMAX, C_TICKET, C_XCHG };
#define AT_CONT_ALL 0x3FFu
#define AT_CONT_RET ((1u << C_TICKET) | (1u << C_XCHG))
#define AT_CONT_L64 ((1u << C_ADD) | (1u << C_UMIN) | (1u << C_UMAX))
#define AT_CONT_G64 (AT_CONT_ALL & ~((1u << C_SMIN) | (1u << C_SMAX)))
// float ops, in block order
enum { F_ADD32, F_ADD64, F_MIN64, F_MAX64, F_ADDH2, F_ADDB2 };
#define AT_F_LDS ((1u << F_ADD32) | (1u << F_ADD64) | (1u << F_ADDH2) | (1u << F_ADDB2))
#define AT_F_ALL 0x3Fu
// magnitude bits of the float operands: +-(1 .. 2**bits)
#define AT_BITS_F32 12u
#define AT_BITS_F64 20u
#define AT_BITS_H 7u
#define AT_BITS_B 5u

#if __HIP_DEVICE_COMPILE__

AT_DEV u32 at_word(u32 base, u32 idx) { return cu_fmix32(base + idx); }

template <typename U>
AT_DEV U at_opnd(u32 base, u32 k, u32 lane) {
  const u32 lo = at_word(base, 128u * k + lane);
  if constexpr (sizeof(U) == 8)
    return (u64)lo | ((u64)at_word(base, 128u * k + 64u + lane) << 32);
  else
    return lo;
}

// Where a stage's values go: into the digest (salted by `key`), or into
// the element dump (row `slot`, column lane).
struct AtFold {
  u32 d = 0;
  AT_DEV void put(u32 slot, u32 key, u64 v) {
    d += cu_fmix32((u32)v ^ cu_fmix32((u32)(v >> 32) + cu_salt(key)));
  }
};

struct AtDump {
  u64* out;
  u32 lane;
  AT_DEV void put(u32 slot, u32 key, u64 v) { out[64u * slot + lane] = v; }
};

// everything this wave has issued to the space is done
template <int SC>
AT_DEV void at_wait() {
  if constexpr (SC == AT_WG)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  else
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int SC, typename T>
AT_DEV void at_store(T* p, T v) { __hip_atomic_store(p, v, AT_RLX, SC); }

template <int SC, typename T>
AT_DEV T at_load(T* p) { return __hip_atomic_load(p, AT_RLX, SC); }

template <int SC, int OP, typename U>
AT_DEV U at_rmw(U* p, U v) {
  typedef typename std::make_signed<U>::type S;
  if constexpr (OP == A_ADD) return __hip_atomic_fetch_add(p, v, AT_RLX, SC);
  else if constexpr (OP == A_SUB) return __hip_atomic_fetch_sub(p, v, AT_RLX, SC);
  else if constexpr (OP == A_UMIN) return __hip_atomic_fetch_min(p, v, AT_RLX, SC);
  else if constexpr (OP == A_UMAX) return __hip_atomic_fetch_max(p, v, AT_RLX, SC);
  else if constexpr (OP == A_SMIN) return (U)__hip_atomic_fetch_min((S*)p, (S)v, AT_RLX, SC);
  else if constexpr (OP == A_SMAX) return (U)__hip_atomic_fetch_max((S*)p, (S)v, AT_RLX, SC);
  else if constexpr (OP == A_AND) return __hip_atomic_fetch_and(p, v, AT_RLX, SC);
  else if constexpr (OP == A_OR) return __hip_atomic_fetch_or(p, v, AT_RLX, SC);
  else if constexpr (OP == A_XOR) return __hip_atomic_fetch_xor(p, v, AT_RLX, SC);
  else if constexpr (OP == A_INC) {
    if constexpr (SC == AT_WG) return __builtin_amdgcn_atomic_inc32(p, v, AT_RLX, "workgroup");
    else return __builtin_amdgcn_atomic_inc32(p, v, AT_RLX, "agent");
  } else if constexpr (OP == A_DEC) {
    if constexpr (SC == AT_WG) return __builtin_amdgcn_atomic_dec32(p, v, AT_RLX, "workgroup");
    else return __builtin_amdgcn_atomic_dec32(p, v, AT_RLX, "agent");
  } else return __hip_atomic_exchange(p, v, AT_RLX, SC);
}

// ---- owned phase, integers: operand slot k0 is the stored word, slot
// k0 + 1 + op the operand of `op`, slot k0 + 14 the cas selector

template <int SC, int OP, u32 MASK, typename U, typename SINK>
AT_DEV void at_own_op(U* cell, u32 base, u32 k0, u32 lane, u32& n, SINK& sink) {
  if constexpr ((MASK >> OP) & 1u) {
    U r;
    if constexpr (OP == A_CAS) {
      // the value the exchange just put there, or its neighbour: hit and
      // miss are decided by an input bit
      r = at_opnd<U>(base, k0 + 1u + A_XCHG, lane) ^ (U)(at_opnd<u32>(base, k0 + 14u, lane) & 1u);
      __hip_atomic_compare_exchange_strong(cell, &r, at_opnd<U>(base, k0 + 1u + A_CAS, lane),
                                           AT_RLX, AT_RLX, SC);
    } else {
      r = at_rmw<SC, OP>(cell, at_opnd<U>(base, k0 + 1u + OP, lane));
    }
    sink.put(n, 64u * n + lane, (u64)r);
    ++n;
  }
}

template <int SC, u32 MASK, typename U, typename SINK>
AT_DEV void at_owned_int(u64* own, u32 base, u32 k0, u32 lane, u32& n, SINK& sink) {
  U* cell = (U*)(own + lane);
  at_store<SC>(cell, at_opnd<U>(base, k0, lane));
  at_own_op<SC, A_ADD, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_SUB, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_UMIN, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_UMAX, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_SMIN, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_SMAX, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_AND, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_OR, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_XOR, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_INC, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_DEC, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_XCHG, MASK>(cell, base, k0, lane, n, sink);
  at_own_op<SC, A_CAS, MASK>(cell, base, k0, lane, n, sink);
  sink.put(n, 64u * n + lane, (u64)at_load<SC>(cell));
  ++n;
}

// ---- contended phase, integers: op `op` has operand slots k0 + 2 op
// (per cell: initial value, ticket step) and k0 + 2 op + 1 (per lane)

template <typename U>
AT_DEV U at_two_bits(u32 w) {
  constexpr u32 m = 8u * sizeof(U) - 1u;
  return (U(1) << (w & m)) | (U(1) << ((w >> 8) & m));
}

template <int OP, typename U>
AT_DEV U at_cont_init(u32 base, u32 k0, u32 cell) {
  constexpr U smax = (U)(~U(0) >> 1);
  if constexpr (OP == C_AND || OP == C_UMIN) return ~U(0);
  else if constexpr (OP == C_OR || OP == C_UMAX) return U(0);
  else if constexpr (OP == C_SMIN) return smax;
  else if constexpr (OP == C_SMAX) return (U)~smax;
  else return at_opnd<U>(base, k0 + 2u * OP, cell);
}

template <int SC, int OP, u32 MASK, int PHASE, typename U, typename SINK>
AT_DEV void at_cont_op(u64* blocks, u32 base, u32 k0, u32 lane, u32 n0, SINK& sink) {
  if constexpr ((MASK >> OP) & 1u) {
    constexpr u32 before = MASK & ((1u << OP) - 1u);
    constexpr u32 b = __builtin_popcount(before);
    constexpr u32 slot_off = b + __builtin_popcount(before & AT_CONT_RET);
    constexpr bool returns = (AT_CONT_RET >> OP) & 1u;
    const u32 cell = lane & 7u, slot = n0 + slot_off;
    U* p = (U*)(blocks + 8u * b + cell);
    if constexpr (PHASE == 0) {
      if (lane < 8u) at_store<SC>(p, at_cont_init<OP, U>(base, k0, cell));
    } else if constexpr (PHASE == 1) {
      const U x = at_opnd<U>(base, k0 + 2u * OP + 1u, lane);
      if constexpr (OP == C_ADD) (void)at_rmw<SC, A_ADD>(p, x);
      else if constexpr (OP == C_AND) (void)at_rmw<SC, A_AND>(p, (U)~at_two_bits<U>((u32)x));
      else if constexpr (OP == C_OR) (void)at_rmw<SC, A_OR>(p, at_two_bits<U>((u32)x));
      else if constexpr (OP == C_XOR) (void)at_rmw<SC, A_XOR>(p, x);
      else if constexpr (OP == C_UMIN) (void)at_rmw<SC, A_UMIN>(p, x);
      else if constexpr (OP == C_UMAX) (void)at_rmw<SC, A_UMAX>(p, x);
      else if constexpr (OP == C_SMIN) (void)at_rmw<SC, A_SMIN>(p, x);
      else if constexpr (OP == C_SMAX) (void)at_rmw<SC, A_SMAX>(p, x);
      else if constexpr (OP == C_TICKET) {
        const U step = at_opnd<U>(base, k0 + 2u * OP + 1u, cell) | U(1);
        sink.put(slot, 64u * slot + cell, (u64)at_rmw<SC, A_ADD>(p, step));
      } else {
        sink.put(slot, 64u * slot + cell, (u64)at_rmw<SC, A_XCHG>(p, x));
      }
    } else {
      // an exchanged cell's final joins the multiset of its returns
      const u32 fslot = slot + (returns ? 1u : 0u);
      const u32 key = OP == C_XCHG ? 64u * slot + cell : 64u * fslot + cell;
      if (lane < 8u) sink.put(fslot, key, (u64)at_load<SC>(p));
    }
  }
}

template <int SC, u32 MASK, int PHASE, typename U, typename SINK>
AT_DEV void at_cont_phase(u64* blocks, u32 base, u32 k0, u32 lane, u32 n0, SINK& sink) {
  at_cont_op<SC, C_ADD, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_AND, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_OR, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_XOR, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_UMIN, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_UMAX, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_SMIN, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_SMAX, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_TICKET, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
  at_cont_op<SC, C_XCHG, MASK, PHASE, U>(blocks, base, k0, lane, n0, sink);
}

// Initial values by lanes 0..7, the ops by all 64 lanes, the finals by
// lanes 0..7, each phase complete before the next is issued.
template <int SC, u32 MASK, typename U, typename SINK>
AT_DEV void at_cont_int(u64* blocks, u32 base, u32 k0, u32 lane, u32& n, SINK& sink) {
  at_cont_phase<SC, MASK, 0, U>(blocks, base, k0, lane, n, sink);
  at_wait<SC>();
  at_cont_phase<SC, MASK, 1, U>(blocks, base, k0, lane, n, sink);
  at_wait<SC>();
  at_cont_phase<SC, MASK, 2, U>(blocks, base, k0, lane, n, sink);
  n += __builtin_popcount(MASK) + __builtin_popcount(MASK & AT_CONT_RET);
}

// ---- floats: every operand is a nonzero integer, every sum exact

AT_DEV int at_fop(u32 w, u32 bits) {
  const int m = (int)(w & ((1u << bits) - 1u)) + 1;
  return (w >> 31) ? -m : m;
}
AT_DEV u32 at_f32_bits(u32 w) { return __builtin_bit_cast(u32, (float)at_fop(w, AT_BITS_F32)); }
AT_DEV u64 at_f64_bits(u32 w) { return __builtin_bit_cast(u64, (double)at_fop(w, AT_BITS_F64)); }
AT_DEV u32 at_h2_bits(u32 lo, u32 hi) {
  const u32 a = __builtin_bit_cast(unsigned short, (_Float16)(float)at_fop(lo, AT_BITS_H));
  const u32 b = __builtin_bit_cast(unsigned short, (_Float16)(float)at_fop(hi, AT_BITS_H));
  return a | (b << 16);
}
// at most six significant bits: the top half of the f32 pattern is exact
AT_DEV u32 at_b2_bits(u32 lo, u32 hi) {
  const u32 a = __builtin_bit_cast(u32, (float)at_fop(lo, AT_BITS_B)) >> 16;
  const u32 b = __builtin_bit_cast(u32, (float)at_fop(hi, AT_BITS_B)) >> 16;
  return a | (b << 16);
}

template <int SC>
AT_DEV u32 at_fadd32(u32* p, u32 bits) {
  const float v = __builtin_bit_cast(float, bits);
  float r;
  if constexpr (SC == AT_WG) r = __hip_atomic_fetch_add((float*)p, v, AT_RLX, SC);
  else r = __builtin_amdgcn_global_atomic_fadd_f32((AT_GLB(float))p, v);
  return __builtin_bit_cast(u32, r);
}

template <int SC>
AT_DEV u64 at_fadd64(u64* p, u64 bits) {
  const double v = __builtin_bit_cast(double, bits);
  double r;
  if constexpr (SC == AT_WG) r = __hip_atomic_fetch_add((double*)p, v, AT_RLX, SC);
  else r = __builtin_amdgcn_global_atomic_fadd_f64((AT_GLB(double))p, v);
  return __builtin_bit_cast(u64, r);
}

AT_DEV u64 at_fmin64(u64* p, u64 bits) {
  return __builtin_bit_cast(u64, __builtin_amdgcn_global_atomic_fmin_f64(
                                     (AT_GLB(double))p, __builtin_bit_cast(double, bits)));
}

AT_DEV u64 at_fmax64(u64* p, u64 bits) {
  return __builtin_bit_cast(u64, __builtin_amdgcn_global_atomic_fmax_f64(
                                     (AT_GLB(double))p, __builtin_bit_cast(double, bits)));
}

template <int SC>
AT_DEV u32 at_addh2(u32* p, u32 bits) {
  const at_h2 v = __builtin_bit_cast(at_h2, bits);
  if constexpr (SC == AT_WG)
    return __builtin_bit_cast(u32, __builtin_amdgcn_ds_atomic_fadd_v2f16((AT_LDS(at_h2))p, v));
  else
    return __builtin_bit_cast(u32,
                              __builtin_amdgcn_global_atomic_fadd_v2f16((AT_GLB(at_h2))p, v));
}

template <int SC>
AT_DEV u32 at_addb2(u32* p, u32 bits) {
  const at_s2 v = __builtin_bit_cast(at_s2, bits);
  if constexpr (SC == AT_WG)
    return __builtin_bit_cast(u32, __builtin_amdgcn_ds_atomic_fadd_v2bf16((AT_LDS(at_s2))p, v));
  else
    return __builtin_bit_cast(u32,
                              __builtin_amdgcn_global_atomic_fadd_v2bf16((AT_GLB(at_s2))p, v));
}

// Owned float chains on cell `lane`: f32 store, add, add; f64 store,
// add, then add (LDS) or min, max (global); packed f16 and packed bf16
// store, add, add; each ends with a load.
template <int SC, bool MINMAX, typename SINK>
AT_DEV void at_owned_float(u64* own, u32 base, u32 lane, u32& n, SINK& sink) {
  const auto lo = [&](u32 k) { return at_opnd<u32>(base, AT_K_F + k, lane); };
  const auto hi = [&](u32 k) { return at_word(base, 128u * (AT_K_F + k) + 64u + lane); };
  const auto put = [&](u64 v) { sink.put(n, 64u * n + lane, v); ++n; };
  u32* c32 = (u32*)(own + lane);
  u64* c64 = own + lane;

  at_store<SC>(c32, at_f32_bits(lo(0)));
  put(at_fadd32<SC>(c32, at_f32_bits(lo(1))));
  put(at_fadd32<SC>(c32, at_f32_bits(lo(2))));
  put(at_load<SC>(c32));

  at_store<SC>(c64, at_f64_bits(lo(3)));
  put(at_fadd64<SC>(c64, at_f64_bits(lo(4))));
  if constexpr (MINMAX) {
    put(at_fmin64(c64, at_f64_bits(lo(5))));
    put(at_fmax64(c64, at_f64_bits(lo(6))));
  } else {
    put(at_fadd64<SC>(c64, at_f64_bits(lo(5))));
  }
  put(at_load<SC>(c64));

  at_store<SC>(c32, at_h2_bits(lo(7), hi(7)));
  put(at_addh2<SC>(c32, at_h2_bits(lo(8), hi(8))));
  put(at_addh2<SC>(c32, at_h2_bits(lo(9), hi(9))));
  put(at_load<SC>(c32));

  at_store<SC>(c32, at_b2_bits(lo(10), hi(10)));
  put(at_addb2<SC>(c32, at_b2_bits(lo(11), hi(11))));
  put(at_addb2<SC>(c32, at_b2_bits(lo(12), hi(12))));
  put(at_load<SC>(c32));
}

template <int SC, int OP, u32 MASK, int PHASE, typename SINK>
AT_DEV void at_cont_fop(u64* blocks, u32 base, u32 lane, u32 n0, SINK& sink) {
  if constexpr ((MASK >> OP) & 1u) {
    constexpr u32 b = __builtin_popcount(MASK & ((1u << OP) - 1u));
    constexpr bool wide = OP == F_ADD64 || OP == F_MIN64 || OP == F_MAX64;
    const u32 cell = lane & 7u, slot = n0 + b;
    u64* p64 = blocks + 8u * b + cell;
    u32* p32 = (u32*)p64;
    if constexpr (PHASE == 0) {
      // zero, or the identity of min / max: plus / minus infinity
      const u64 init = OP == F_MIN64 ? 0x7FF0000000000000ull
                                     : OP == F_MAX64 ? 0xFFF0000000000000ull : 0ull;
      if (lane < 8u) {
        if constexpr (wide) at_store<SC>(p64, init);
        else at_store<SC>(p32, (u32)init);
      }
    } else if constexpr (PHASE == 1) {
      const u32 lo = at_opnd<u32>(base, AT_K_CF + OP, lane);
      const u32 hi = at_word(base, 128u * (AT_K_CF + OP) + 64u + lane);
      if constexpr (OP == F_ADD32) (void)at_fadd32<SC>(p32, at_f32_bits(lo));
      else if constexpr (OP == F_ADD64) (void)at_fadd64<SC>(p64, at_f64_bits(lo));
      else if constexpr (OP == F_MIN64) (void)at_fmin64(p64, at_f64_bits(lo));
      else if constexpr (OP == F_MAX64) (void)at_fmax64(p64, at_f64_bits(lo));
      else if constexpr (OP == F_ADDH2) (void)at_addh2<SC>(p32, at_h2_bits(lo, hi));
      else (void)at_addb2<SC>(p32, at_b2_bits(lo, hi));
    } else {
      if (lane < 8u) {
        if constexpr (wide) sink.put(slot, 64u * slot + cell, at_load<SC>(p64));
        else sink.put(slot, 64u * slot + cell, (u64)at_load<SC>(p32));
      }
    }
  }
}

template <int SC, u32 MASK, int PHASE, typename SINK>
AT_DEV void at_cont_fphase(u64* blocks, u32 base, u32 lane, u32 n0, SINK& sink) {
  at_cont_fop<SC, F_ADD32, MASK, PHASE>(blocks, base, lane, n0, sink);
  at_cont_fop<SC, F_ADD64, MASK, PHASE>(blocks, base, lane, n0, sink);
  at_cont_fop<SC, F_MIN64, MASK, PHASE>(blocks, base, lane, n0, sink);
  at_cont_fop<SC, F_MAX64, MASK, PHASE>(blocks, base, lane, n0, sink);
  at_cont_fop<SC, F_ADDH2, MASK, PHASE>(blocks, base, lane, n0, sink);
  at_cont_fop<SC, F_ADDB2, MASK, PHASE>(blocks, base, lane, n0, sink);
}

template <int SC, u32 MASK, typename SINK>
AT_DEV void at_cont_float(u64* blocks, u32 base, u32 lane, u32& n, SINK& sink) {
  at_cont_fphase<SC, MASK, 0>(blocks, base, lane, n, sink);
  at_wait<SC>();
  at_cont_fphase<SC, MASK, 1>(blocks, base, lane, n, sink);
  at_wait<SC>();
  at_cont_fphase<SC, MASK, 2>(blocks, base, lane, n, sink);
  n += __builtin_popcount(MASK);
}

// ---- stage 0's cross-wave phase: cell c takes op c & 7 (add, xor, or,
// and, umin, umax, add, xor) from eight lanes of each of the 16 waves

AT_DEV u32 at_sparse_bit(u32 w) { return ((w >> 5) & 7u) == 0u ? 1u << (w & 31u) : 0u; }

template <typename SINK>
AT_DEV void at_cross(u32* xc, u32 base, u32 wib, u32 lane, u32& n, SINK& sink) {
  if (lane < 4u) {
    const u32 c = 4u * wib + lane, j = c & 7u;
    const u32 init = (j == 2u || j == 5u) ? 0u
                     : (j == 3u || j == 4u) ? 0xFFFFFFFFu
                                            : at_word(base, 128u * AT_K_XW + 8192u + c);
    at_store<AT_WG>(xc + c, init);
  }
  __syncthreads();
#pragma unroll
  for (u32 j = 0; j < 8u; ++j) {
    u32* p = xc + 8u * ((lane + wib + j) & 7u) + j;
    const u32 w = at_word(base, 128u * AT_K_XW + 1024u * j + 64u * wib + lane);
    if (j == 0u || j == 6u) (void)at_rmw<AT_WG, A_ADD>(p, w);
    else if (j == 1u || j == 7u) (void)at_rmw<AT_WG, A_XOR>(p, w);
    else if (j == 2u) (void)at_rmw<AT_WG, A_OR>(p, at_sparse_bit(w));
    else if (j == 3u) (void)at_rmw<AT_WG, A_AND>(p, ~at_sparse_bit(w));
    else if (j == 4u) (void)at_rmw<AT_WG, A_UMIN>(p, w);
    else (void)at_rmw<AT_WG, A_UMAX>(p, w);
  }
  __syncthreads();
  sink.put(n, 64u * n + lane, (u64)at_load<AT_WG>(xc + lane));
  ++n;
  __syncthreads();
}

// ---- the four stages; every one returns its number of result slots

template <typename SINK>
AT_DEV u32 at_stage_lds(u64* slice, u32* xc, u32 base, u32 wib, u32 lane, SINK& sink) {
  u32 n = 0;
  at_owned_int<AT_WG, AT_OWN_ALL, u32>(slice, base, AT_K_O32, lane, n, sink);
  at_cont_int<AT_WG, AT_CONT_ALL, u32>(slice + 64, base, AT_K_C32, lane, n, sink);
  at_owned_int<AT_WG, AT_OWN_L64, u64>(slice, base, AT_K_O64, lane, n, sink);
  at_cont_int<AT_WG, AT_CONT_L64, u64>(slice + 64 + 8 * 10, base, AT_K_C64, lane, n, sink);
  at_owned_float<AT_WG, false>(slice, base, lane, n, sink);
  at_cont_float<AT_WG, AT_F_LDS>(slice + 64 + 8 * 13, base, lane, n, sink);
  at_cross(xc, base, wib, lane, n, sink);
  return n;
}

template <typename SINK>
AT_DEV u32 at_stage_g32(u64* slice, u32 base, u32 lane, SINK& sink) {
  u32 n = 0;
  at_owned_int<AT_AG, AT_OWN_ALL, u32>(slice, base, AT_K_O32, lane, n, sink);
  at_cont_int<AT_AG, AT_CONT_ALL, u32>(slice + 64, base, AT_K_C32, lane, n, sink);
  return n;
}

template <typename SINK>
AT_DEV u32 at_stage_g64(u64* slice, u32 base, u32 lane, SINK& sink) {
  u32 n = 0;
  at_owned_int<AT_AG, AT_OWN_G64, u64>(slice, base, AT_K_O64, lane, n, sink);
  at_cont_int<AT_AG, AT_CONT_G64, u64>(slice + 64, base, AT_K_C64, lane, n, sink);
  return n;
}

template <typename SINK>
AT_DEV u32 at_stage_gfp(u64* slice, u32 base, u32 lane, SINK& sink) {
  u32 n = 0;
  at_owned_float<AT_AG, true>(slice, base, lane, n, sink);
  at_cont_float<AT_AG, AT_F_ALL>(slice + 64, base, lane, n, sink);
  return n;
}

// ---- the shared region: lane l of every wave of the grid onto cell l
// of six rows.  Operand = a term of (round, lane) combined with a term
// of (global wave, lane), so that the host has the finals in closed form.
AT_DEV void at_shared(u64* sh, u32 seed, u32 rp, u32 gwave, u32 lane) {
  const u32 ba = cu_base(seed, AT_STAGE0 + 4u, rp), bb = cu_base(seed, AT_STAGE0 + 5u, gwave);
  const auto A = [&](u32 i) { return at_word(ba, 64u * i + lane); };
  const auto B = [&](u32 i) { return at_word(bb, 64u * i + lane); };
  // the adds: an odd term plus an even one, never zero
  (void)at_rmw<AT_AG, A_ADD>((u32*)(sh + lane), (A(0) | 1u) + (B(0) & ~1u));
  const u64 a64 = (u64)A(1) | ((u64)A(6) << 32), b64 = (u64)B(1) | ((u64)B(6) << 32);
  (void)at_rmw<AT_AG, A_ADD>(sh + 64 + lane, (a64 | 1ull) + (b64 & ~1ull));
  (void)at_rmw<AT_AG, A_XOR>((u32*)(sh + 128 + lane), A(2) ^ B(2));
  // two 31-bit terms: the sum does not overflow, so max and min separate
  (void)at_rmw<AT_AG, A_UMAX>((u32*)(sh + 192 + lane), (A(3) >> 1) + (B(3) >> 1));
  (void)at_rmw<AT_AG, A_UMIN>((u32*)(sh + 256 + lane), (A(4) >> 1) + (B(4) >> 1));
  const int fa = (int)((A(5) & 0x3FFFEu) | 1u), fb = (int)(B(5) & 0x3FFFEu);
  const double x = (double)((A(5) >> 31) ? -fa : fa) + (double)((B(5) >> 31) ? -fb : fb);
  (void)at_fadd64<AT_AG>(sh + 320 + lane, __builtin_bit_cast(u64, x));
}

#endif  // __HIP_DEVICE_COMPILE__

__global__ void __launch_bounds__(CU_BLOCK)
atomcheck_kernel(CuArgs a, u64* arena, u64* shared, u32 shared_every, u32 drop_wave,
                 u32 drop_round) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ u64 at_lds[];
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane, wib = threadIdx.x / WAVE;
  u64* lslice = at_lds + wib * AT_SLICE;
  u32* xc = (u32*)(at_lds + CU_WAVES * AT_SLICE);
  u64* gslice = arena + (size_t)w.gwave * AT_WAVE_CELLS;

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % AT_PERIOD;
    AtFold f0, f1, f2, f3;
    at_stage_lds(lslice, xc, cu_base(a.seed, AT_STAGE0 + 0, rp), wib, lane, f0);
    at_stage_g32(gslice, cu_base(a.seed, AT_STAGE0 + 1, rp), lane, f1);
    at_stage_g64(gslice + AT_SLICE, cu_base(a.seed, AT_STAGE0 + 2, rp), lane, f2);
    at_stage_gfp(gslice + 2 * AT_SLICE, cu_base(a.seed, AT_STAGE0 + 3, rp), lane, f3);
    if (shared_every != 0u && r % shared_every == 0u &&
        !(w.gwave == drop_wave && r == drop_round))
      at_shared(shared, a.seed, rp, w.gwave, lane);
    u32 dig[N_STAGES] = {wave_sum(f0.d), wave_sum(f1.d), wave_sum(f2.d), wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One workgroup; wave 0 writes every value it would fold for one stage
// and round, out[64 * slot + lane], and the number of slots behind the
// last row.  Stage 0 runs on all 16 waves, as its cross-wave phase needs
// them.  A digest cannot say which op returned what; this can.
__global__ void __launch_bounds__(CU_BLOCK)
atomcheck_values_kernel(u32 seed, u32 stage, u32 r, u64* arena, u64* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  extern __shared__ u64 at_lds[];
  const u32 lane = threadIdx.x % WAVE, wib = threadIdx.x / WAVE;
  const u32 base = cu_base(seed, AT_STAGE0 + stage, r % AT_PERIOD);
  if (stage != 0u && wib != 0u) return;
  u64* gslice = arena + (size_t)wib * AT_WAVE_CELLS;
  AtDump sink;
  sink.out = out;
  sink.lane = lane;
  u32 n;
  if (stage == 0u) {
    u64* lslice = at_lds + wib * AT_SLICE;
    u32* xc = (u32*)(at_lds + CU_WAVES * AT_SLICE);
    if (wib == 0u) {
      n = at_stage_lds(lslice, xc, base, wib, lane, sink);
    } else {
      AtFold rest;
      n = at_stage_lds(lslice, xc, base, wib, lane, rest);
    }
  } else if (stage == 1u) {
    n = at_stage_g32(gslice, base, lane, sink);
  } else if (stage == 2u) {
    n = at_stage_g64(gslice + AT_SLICE, base, lane, sink);
  } else {
    n = at_stage_gfp(gslice + 2 * AT_SLICE, base, lane, sink);
  }
  if (threadIdx.x == 0) out[64u * AT_VALUE_SLOTS] = n;
#endif
}

// ---------------------------------------------------------------- host

typedef std::tuple<int64_t, int64_t> AtDrop;

// `arena` (int64, blocks x 16 x AT_WAVE_CELLS + AT_SHARED_CELLS elements,
// the shared region last, prepared by the caller) is left as the kernel
// left it: the caller checks the shared region.
CucheckOut atomcheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                         int64_t blocks_arg, at::Tensor arena, int64_t shared_every,
                         int64_t max_records, c10::optional<at::Tensor> dump,
                         c10::optional<CuInject> inject, c10::optional<AtDrop> drop) {
  CuLaunch l = cu_prepare("atomcheck", expected, seed_arg, rounds, blocks_arg,
                          max_records, dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  const int64_t waves = l.blocks * CU_WAVES;
  TORCH_CHECK(arena.is_cuda() && arena.get_device() == expected.get_device(),
              "atomcheck: arena must be on the same GPU as expected");
  TORCH_CHECK(arena.scalar_type() == at::kLong && arena.is_contiguous(),
              "atomcheck: arena must be a contiguous int64 tensor");
  TORCH_CHECK(arena.numel() == waves * AT_WAVE_CELLS + AT_SHARED_CELLS,
              "atomcheck: arena must hold ", waves * AT_WAVE_CELLS + AT_SHARED_CELLS,
              " elements for ", l.blocks, " blocks, got ", arena.numel());
  TORCH_CHECK(shared_every >= 0 && shared_every <= MAX_ROUNDS,
              "atomcheck: shared_every must be in 0..", MAX_ROUNDS);
  u32 drop_wave = NO_DROP, drop_round = 0;
  if (drop.has_value()) {
    int64_t w = std::get<0>(*drop), r = std::get<1>(*drop);
    TORCH_CHECK(w >= 0 && w < waves && r >= 0 && r < rounds,
                "atomcheck: drop (wave, round) out of range");
    drop_wave = (u32)w;
    drop_round = (u32)r;
  }
  u64* cells = (u64*)arena.data_ptr();

  return cu_launch_timed(atomcheck_kernel, l, MAX_LDS_BYTES, cells,
                         cells + waves * AT_WAVE_CELLS, (u32)shared_every, drop_wave,
                         drop_round);
}

// What wave 0 folds for one stage and round as an int64 tensor on the
// current GPU: AT_VALUE_SLOTS rows of 64 lanes, then the number of rows
// the stage filled.
at::Tensor atomcheck_values(int64_t seed_arg, int64_t stage, int64_t round) {
  cu_check_wave_args("atomcheck", seed_arg, stage, round);
  auto opts = at::TensorOptions().dtype(at::kLong).device(at::kCUDA);
  at::Tensor out = at::zeros({(int64_t)(64 * AT_VALUE_SLOTS + 1)}, opts);
  at::Tensor arena = at::zeros({(int64_t)(CU_WAVES * AT_WAVE_CELLS)}, opts);
  return cu_launch_values(atomcheck_values_kernel, CU_BLOCK, AT_LDS_USED, out, (u32)seed_arg,
                          (u32)stage, (u32)round, (u64*)arena.data_ptr(),
                          (u64*)out.data_ptr());
}

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/atomcheck_mi355x.json).
void bind_atomcheck(py::module_& m) {
  m.def("atomcheck_run", &atomcheck_run,
        "atomic-unit integrity run -> (mismatches, first_bad_round, stage_mask, "
        "records, waves_on, elapsed_s); the arena's shared region is left for the caller",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("arena"), py::arg("shared_every"), py::arg("max_records") = 16,
        py::arg("dump") = py::none(), py::arg("inject") = py::none(),
        py::arg("drop") = py::none());
  m.def("atomcheck_values", &atomcheck_values,
        "values wave 0 folds for one stage and round as int64 [64 rows * 64 lanes + 1]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"));
  m.def("atomcheck_layout", []() {
          return std::make_tuple((int64_t)AT_WAVE_CELLS, (int64_t)AT_SHARED_CELLS,
                                 (int64_t)AT_VALUE_SLOTS, (int64_t)AT_PERIOD);
        },
        "(arena cells per wave, shared cells, value rows, period)");
}
