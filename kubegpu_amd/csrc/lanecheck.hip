// lanecheck — integrity kernel for the cross-lane data paths (gfx950),
// compiled into _gpuprobe.
//
// The twin of cucheck.hip, mxcheck.hip, fpcheck.hip and atomcheck.hip for
// the hardware that moves a value from one lane of a wave to another,
// which none of them uses as workload: the DPP network, the LDS crossbar
// used without memory, the VGPR -> SGPR -> VGPR path and gfx950's
// permlane swaps.  Every wave of the launch runs the same deterministic
// sequence of cross-lane operations and compares four 32-bit digests per
// round with a table the host computed in numpy (probe/lanecheck.py
// holds the definition of every operand, control table and digest):
//   stage 0 dpp   v_mov_b32_dpp through every entry of LC_DPP: quad_perm,
//                 row_shl / shr / ror, wave_shl / rol / shr / ror,
//                 row_mirror, row_half_mirror, row_bcast:15 / 31,
//                 row_newbcast, with row and bank masks and bound_ctrl
//   stage 1 xbar  ds_bpermute gathers, ds_permute scatters (bijections),
//                 ds_swizzle in bit mode and quad-perm mode
//   stage 2 sgpr  v_readlane with constant and uniform run-time indices,
//                 v_readfirstlane under a partial EXEC, ballots, the
//                 v_mbcnt prefix count, v_permlane16_swap, v_permlane32_swap
//   stage 3 scan  the dependent chains workloads run: inclusive and
//                 exclusive prefix sum by DPP, all-reduce sum / umin /
//                 umax / xor by an xor butterfly, per-row sum by row_ror
// Every op is a permutation or a select, so the reference is exact.
//
// Inputs are word(24 + stage, r % LC_PERIOD, idx) of cucheck_common.h;
// operand slot k is the per-lane word 64 k + lane, u(k) the wave-uniform
// word 64 k.  Nothing depends on the wave number.  The kernel touches no
// memory but the shared result block and the optional dump; the dynamic
// LDS is asked for only to keep a second workgroup off the CU.  Launch
// shape and accounting are cucheck's.

#include "cucheck_common.h"
// named here too: the extension build rewrites a source with kernel
// launches that does not include the runtime header itself
#include <hip/hip_runtime.h>

#include <utility>

#define LC_DEV __device__ __forceinline__

#define LC_STAGE0 24u  // stage number fed to cu_base() is LC_STAGE0 + stage
#define LC_PERIOD 64u
#define LC_VALUE_SLOTS 48u  // rows of lanecheck_values' output, >= any stage's

// DPP controls, as the instruction encodes them
#define LC_QUAD(a, b, c, d) ((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
#define LC_ROW_SHL(n) (0x100u + (n))
#define LC_ROW_SHR(n) (0x110u + (n))
#define LC_ROW_ROR(n) (0x120u + (n))
#define LC_WAVE_SHL1 0x130u
#define LC_WAVE_ROL1 0x134u
#define LC_WAVE_SHR1 0x138u
#define LC_WAVE_ROR1 0x13Cu
#define LC_ROW_MIRROR 0x140u
#define LC_ROW_HALF_MIRROR 0x141u
#define LC_ROW_BCAST15 0x142u
#define LC_ROW_BCAST31 0x143u
#define LC_ROW_NEWBCAST(n) (0x150u + (n))

struct LcDpp {
  u32 ctrl, row_mask, bank_mask, bound_ctrl;
};

// Stage 0's table: entry j is update_dpp(old = v(2j), src = v(2j + 1)).
// probe/lanecheck.py holds the same table as DPP_TABLE.
constexpr LcDpp LC_DPP[] = {
    {LC_QUAD(3u, 2u, 1u, 0u), 0xF, 0xF, 0},
    {LC_QUAD(1u, 0u, 3u, 2u), 0xF, 0xF, 0},
    {LC_QUAD(0u, 0u, 2u, 2u), 0xF, 0xF, 0},
    {LC_ROW_SHL(1u), 0xF, 0xF, 0},
    {LC_ROW_SHL(1u), 0xF, 0xF, 1},
    {LC_ROW_SHL(3u), 0xF, 0xF, 1},
    {LC_ROW_SHL(15u), 0xF, 0xF, 0},
    {LC_ROW_SHR(1u), 0xF, 0xF, 1},
    {LC_ROW_SHR(1u), 0xF, 0xF, 0},
    {LC_ROW_SHR(2u), 0xF, 0xF, 0},
    {LC_ROW_SHR(4u), 0xF, 0xF, 1},
    {LC_ROW_SHR(8u), 0xF, 0xF, 0},
    {LC_ROW_ROR(1u), 0xF, 0xF, 0},
    {LC_ROW_ROR(5u), 0xF, 0xF, 0},
    {LC_ROW_ROR(12u), 0xF, 0xF, 0},
    {LC_WAVE_SHL1, 0xF, 0xF, 0},
    {LC_WAVE_SHL1, 0xF, 0xF, 1},
    {LC_WAVE_ROL1, 0xF, 0xF, 0},
    {LC_WAVE_SHR1, 0xF, 0xF, 1},
    {LC_WAVE_SHR1, 0xF, 0xF, 0},
    {LC_WAVE_ROR1, 0xF, 0xF, 0},
    {LC_ROW_MIRROR, 0xF, 0xF, 0},
    {LC_ROW_HALF_MIRROR, 0xF, 0xF, 0},
    {LC_ROW_BCAST15, 0xA, 0xF, 0},
    {LC_ROW_BCAST31, 0xC, 0xF, 0},
    {LC_ROW_NEWBCAST(0u), 0xF, 0xF, 0},
    {LC_ROW_NEWBCAST(5u), 0xF, 0xF, 0},
    {LC_ROW_NEWBCAST(15u), 0xF, 0xF, 0},
    // partial masks: a lane whose row bit or bank bit is clear keeps old
    {LC_ROW_SHL(1u), 0x5, 0xF, 1},
    {LC_ROW_SHR(1u), 0xF, 0x3, 0},
    {LC_QUAD(2u, 3u, 0u, 1u), 0xA, 0x5, 0},
    {LC_ROW_ROR(5u), 0xC, 0xE, 0},
    {LC_ROW_MIRROR, 0x5, 0xE, 0},
    {LC_WAVE_SHR1, 0xA, 0x3, 1},
    {LC_ROW_NEWBCAST(9u), 0xC, 0x5, 0},
};
#define LC_N_DPP ((u32)(sizeof(LC_DPP) / sizeof(LC_DPP[0])))

// ds_swizzle offsets: bit mode is and | or << 5 | xor << 10 on the lane
// number within its group of 32, quad-perm mode is 0x8000 | selects
#define LC_SWZ_BITS(and_m, or_m, xor_m) ((and_m) | ((or_m) << 5) | ((xor_m) << 10))
#define LC_SWZ_SWAP(x) LC_SWZ_BITS(0x1Fu, 0u, (x))
#define LC_SWZ_QUAD(a, b, c, d) (0x8000u | LC_QUAD(a, b, c, d))
constexpr u32 LC_SWIZZLE[] = {
    LC_SWZ_SWAP(1u),  LC_SWZ_SWAP(2u), LC_SWZ_SWAP(4u),
    LC_SWZ_SWAP(8u),  LC_SWZ_SWAP(16u),
    LC_SWZ_BITS(0x1Fu, 0u, 0x1Fu),  // reverse within 32
    LC_SWZ_BITS(0x18u, 3u, 0u),     // lane 3 of every group of 8, broadcast
    LC_SWZ_QUAD(3u, 2u, 1u, 0u),
    LC_SWZ_QUAD(1u, 1u, 3u, 0u),
};
#define LC_N_SWIZZLE ((u32)(sizeof(LC_SWIZZLE) / sizeof(LC_SWIZZLE[0])))

// stage 2's constant readlane indices
constexpr u32 LC_READLANE[] = {17u, 63u};
#define LC_N_READLANE 2u

#define LC_N_BPERMUTE 4u
#define LC_N_PERMUTE 3u
#define LC_N_READLANE_DYN 4u
// result slots of the stages
#define LC_SLOTS_XBAR (LC_N_BPERMUTE + LC_N_PERMUTE + LC_N_SWIZZLE)
#define LC_SLOTS_SGPR (LC_N_READLANE + LC_N_READLANE_DYN + 1u + 4u + 1u + 2u + 2u)
#define LC_SLOTS_SCAN 7u
static_assert(LC_N_DPP <= LC_VALUE_SLOTS && LC_SLOTS_XBAR <= LC_VALUE_SLOTS &&
                  LC_SLOTS_SGPR <= LC_VALUE_SLOTS && LC_SLOTS_SCAN <= LC_VALUE_SLOTS,
              "lanecheck_values' rows must hold every stage");

#if __HIP_DEVICE_COMPILE__

// operand slot k of this lane, and the slot's wave-uniform word
LC_DEV u32 lc_v(u32 base, u32 k, u32 lane) { return cu_fmix32(base + 64u * k + lane); }
LC_DEV u32 lc_u(u32 base, u32 k) { return cu_fmix32(base + 64u * k); }

// Where a stage's values go: into the digest, or into the element dump
// (row `slot`, column lane).
struct LcFold {
  u32 d = 0;
  LC_DEV void put(u32 slot, u32 lane, u32 v) { d += cu_fmix32(v + cu_salt(64u * slot + lane)); }
};

struct LcDump {
  u32* out;
  LC_DEV void put(u32 slot, u32 lane, u32 v) { out[64u * slot + lane] = v; }
};

template <u32 CTRL, u32 ROW = 0xFu, u32 BANK = 0xFu, bool BC = false>
LC_DEV u32 lc_dpp(u32 old, u32 src) {
  return (u32)__builtin_amdgcn_update_dpp((int)old, (int)src, (int)CTRL, (int)ROW, (int)BANK,
                                          BC);
}

// ---- stage 0: every entry of LC_DPP

template <typename SINK, size_t... J>
LC_DEV void lc_dpp_all(u32 base, u32 lane, SINK& sink, std::index_sequence<J...>) {
  (sink.put((u32)J, lane,
            lc_dpp<LC_DPP[J].ctrl, LC_DPP[J].row_mask, LC_DPP[J].bank_mask,
                   LC_DPP[J].bound_ctrl != 0u>(lc_v(base, 2u * (u32)J, lane),
                                               lc_v(base, 2u * (u32)J + 1u, lane))),
   ...);
}

template <typename SINK>
LC_DEV u32 lc_stage_dpp(u32 base, u32 lane, SINK& sink) {
  lc_dpp_all(base, lane, sink, std::make_index_sequence<LC_N_DPP>());
  return LC_N_DPP;
}

// ---- stage 1: the LDS crossbar without memory.  Operand slots: gather g
// takes 2g (data) and 2g + 1 (indices), scatter p 8 + 2p (data) and
// 9 + 2p (u: the map), swizzle s 14 + s.

template <typename SINK, size_t... S>
LC_DEV void lc_swizzle_all(u32 base, u32 lane, u32 n0, SINK& sink, std::index_sequence<S...>) {
  (sink.put(n0 + (u32)S, lane,
            (u32)__builtin_amdgcn_ds_swizzle((int)lc_v(base, 14u + (u32)S, lane),
                                             (int)LC_SWIZZLE[S])),
   ...);
}

template <typename SINK>
LC_DEV u32 lc_stage_xbar(u32 base, u32 lane, SINK& sink) {
  u32 n = 0;
#pragma unroll
  for (u32 g = 0; g < LC_N_BPERMUTE; ++g) {
    // the last gather leaves 14 bits of index: the hardware takes it mod 64
    const u32 mask = g + 1u == LC_N_BPERMUTE ? 0x3FFFu : 63u;
    const u32 idx = lc_v(base, 2u * g + 1u, lane) & mask;
    sink.put(n++, lane,
             (u32)__builtin_amdgcn_ds_bpermute((int)(4u * idx), (int)lc_v(base, 2u * g, lane)));
  }
#pragma unroll
  for (u32 p = 0; p < LC_N_PERMUTE; ++p) {
    // lane l sends to (a l + b) mod 64 with a odd: a bijection
    const u32 u = lc_u(base, 9u + 2u * p);
    const u32 dst = ((u | 1u) * lane + (u >> 8)) & 63u;
    sink.put(n++, lane,
             (u32)__builtin_amdgcn_ds_permute((int)(4u * dst),
                                              (int)lc_v(base, 8u + 2u * p, lane)));
  }
  lc_swizzle_all(base, lane, n, sink, std::make_index_sequence<LC_N_SWIZZLE>());
  return n + LC_N_SWIZZLE;
}

// ---- stage 2: through the scalar registers, and the permlane swaps

template <typename SINK>
LC_DEV u32 lc_stage_sgpr(u32 base, u32 base0, u32 rp, u32 lane, SINK& sink) {
  u32 n = 0;
  sink.put(n++, lane, (u32)__builtin_amdgcn_readlane((int)lc_v(base, 0u, lane), LC_READLANE[0]));
  sink.put(n++, lane, (u32)__builtin_amdgcn_readlane((int)lc_v(base, 1u, lane), LC_READLANE[1]));
#pragma unroll
  for (u32 i = 0; i < LC_N_READLANE_DYN; ++i) {
    // a uniform index from the data; the last one starts from round 0's
    // word and steps with the round, so a period reads every lane
    const u32 k = 2u + 2u * i;
    const u32 idx = i + 1u == LC_N_READLANE_DYN ? (lc_u(base0, k + 1u) + rp) & 63u
                                                 : lc_u(base, k + 1u) & 63u;
    sink.put(n++, lane, (u32)__builtin_amdgcn_readlane((int)lc_v(base, k, lane), (int)idx));
  }
  {
    // lanes t .. 63 read their first lane's value, lane t's; 1 <= t <= 62
    const u32 t = 1u + lc_u(base, 11u) % 62u;
    u32 r = lc_v(base, 12u, lane);
    if (lane >= t) r = (u32)__builtin_amdgcn_readfirstlane((int)lc_v(base, 10u, lane));
    sink.put(n++, lane, r);
  }
  const unsigned long long b0 = __builtin_amdgcn_ballot_w64((lc_v(base, 13u, lane) & 1u) != 0u);
  const unsigned long long b1 = __builtin_amdgcn_ballot_w64((lc_v(base, 14u, lane) >> 31) != 0u);
  sink.put(n++, lane, (u32)b0);
  sink.put(n++, lane, (u32)(b0 >> 32));
  sink.put(n++, lane, (u32)b1);
  sink.put(n++, lane, (u32)(b1 >> 32));
  // set bits of the second ballot in the lanes below this one
  sink.put(n++, lane,
           __builtin_amdgcn_mbcnt_hi((u32)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((u32)b1, 0u)));
  {
    const auto s = __builtin_amdgcn_permlane16_swap(lc_v(base, 15u, lane),
                                                    lc_v(base, 16u, lane), false, false);
    sink.put(n++, lane, s[0]);
    sink.put(n++, lane, s[1]);
  }
  {
    const auto s = __builtin_amdgcn_permlane32_swap(lc_v(base, 17u, lane),
                                                    lc_v(base, 18u, lane), false, false);
    sink.put(n++, lane, s[0]);
    sink.put(n++, lane, s[1]);
  }
  return n;
}

// ---- stage 3: scans and reductions

// lane ^ OFF's value: DPP within a quad, ds_swizzle within 32 lanes, the
// crossbar across the halves
template <u32 OFF>
LC_DEV u32 lc_xor_lane(u32 x, u32 lane) {
  if constexpr (OFF == 1u) return lc_dpp<LC_QUAD(1u, 0u, 3u, 2u)>(x, x);
  else if constexpr (OFF == 2u) return lc_dpp<LC_QUAD(2u, 3u, 0u, 1u)>(x, x);
  else if constexpr (OFF < 32u) return (u32)__builtin_amdgcn_ds_swizzle((int)x, (int)LC_SWZ_SWAP(OFF));
  else return (u32)__builtin_amdgcn_ds_bpermute((int)(4u * (lane ^ 32u)), (int)x);
}

enum { LC_SUM, LC_UMIN, LC_UMAX, LC_XOR };

template <int OP>
LC_DEV u32 lc_combine(u32 a, u32 b) {
  if constexpr (OP == LC_SUM) return a + b;
  else if constexpr (OP == LC_UMIN) return a < b ? a : b;
  else if constexpr (OP == LC_UMAX) return a > b ? a : b;
  else return a ^ b;
}

template <int OP>
LC_DEV u32 lc_allreduce(u32 x, u32 lane) {
  x = lc_combine<OP>(x, lc_xor_lane<1u>(x, lane));
  x = lc_combine<OP>(x, lc_xor_lane<2u>(x, lane));
  x = lc_combine<OP>(x, lc_xor_lane<4u>(x, lane));
  x = lc_combine<OP>(x, lc_xor_lane<8u>(x, lane));
  x = lc_combine<OP>(x, lc_xor_lane<16u>(x, lane));
  x = lc_combine<OP>(x, lc_xor_lane<32u>(x, lane));
  return x;
}

template <typename SINK>
LC_DEV u32 lc_stage_scan(u32 base, u32 lane, SINK& sink) {
  u32 n = 0;
  // inclusive prefix sum: within the rows by row_shr 1, 2, 4, 8 (a lane
  // with no source keeps old = 0), then row k's total into row k + 1 by
  // row_bcast:15 and the lower half's into the upper by row_bcast:31
  u32 x = lc_v(base, 0u, lane);
  x += lc_dpp<LC_ROW_SHR(1u)>(0u, x);
  x += lc_dpp<LC_ROW_SHR(2u)>(0u, x);
  x += lc_dpp<LC_ROW_SHR(4u)>(0u, x);
  x += lc_dpp<LC_ROW_SHR(8u)>(0u, x);
  x += lc_dpp<LC_ROW_BCAST15, 0xAu>(0u, x);
  x += lc_dpp<LC_ROW_BCAST31, 0xCu>(0u, x);
  sink.put(n++, lane, x);
  // its exclusive form: one lane up, lane 0 keeps old = 0
  sink.put(n++, lane, lc_dpp<LC_WAVE_SHR1>(0u, x));
  sink.put(n++, lane, lc_allreduce<LC_SUM>(lc_v(base, 1u, lane), lane));
  sink.put(n++, lane, lc_allreduce<LC_UMIN>(lc_v(base, 2u, lane), lane));
  sink.put(n++, lane, lc_allreduce<LC_UMAX>(lc_v(base, 3u, lane), lane));
  sink.put(n++, lane, lc_allreduce<LC_XOR>(lc_v(base, 4u, lane), lane));
  // per-row sum, in every lane of the row
  u32 y = lc_v(base, 5u, lane);
  y += lc_dpp<LC_ROW_ROR(8u)>(y, y);
  y += lc_dpp<LC_ROW_ROR(4u)>(y, y);
  y += lc_dpp<LC_ROW_ROR(2u)>(y, y);
  y += lc_dpp<LC_ROW_ROR(1u)>(y, y);
  sink.put(n++, lane, y);
  return n;
}

#endif  // __HIP_DEVICE_COMPILE__

__global__ void __launch_bounds__(CU_BLOCK)
lanecheck_kernel(CuArgs a) {
#if __HIP_DEVICE_COMPILE__
  const CuWave w = cu_wave(a);
  const u32 lane = (u32)w.lane;
  const u32 base0 = cu_base(a.seed, LC_STAGE0 + 2, 0u);

  for (u32 r = 0; r < a.rounds; ++r) {
    const u32 rp = r % LC_PERIOD;
    LcFold f0, f1, f2, f3;
    lc_stage_dpp(cu_base(a.seed, LC_STAGE0 + 0, rp), lane, f0);
    lc_stage_xbar(cu_base(a.seed, LC_STAGE0 + 1, rp), lane, f1);
    lc_stage_sgpr(cu_base(a.seed, LC_STAGE0 + 2, rp), base0, rp, lane, f2);
    lc_stage_scan(cu_base(a.seed, LC_STAGE0 + 3, rp), lane, f3);
    u32 dig[N_STAGES] = {wave_sum(f0.d), wave_sum(f1.d), wave_sum(f2.d), wave_sum(f3.d)};

    cu_check_round(dig, r, w, a);
  }
#endif
}

// One wave writes every value it would fold for one stage and round,
// out[64 * slot + lane], and the number of slots behind the last row.  A
// digest cannot say which op moved what; this can.
__global__ void __launch_bounds__(WAVE)
lanecheck_values_kernel(u32 seed, u32 stage, u32 r, u32* __restrict__ out) {
#if __HIP_DEVICE_COMPILE__
  const u32 lane = threadIdx.x;
  const u32 rp = r % LC_PERIOD;
  const u32 base = cu_base(seed, LC_STAGE0 + stage, rp);
  LcDump sink;
  sink.out = out;
  u32 n;
  if (stage == 0u) n = lc_stage_dpp(base, lane, sink);
  else if (stage == 1u) n = lc_stage_xbar(base, lane, sink);
  else if (stage == 2u) n = lc_stage_sgpr(base, cu_base(seed, LC_STAGE0 + 2, 0u), rp, lane, sink);
  else n = lc_stage_scan(base, lane, sink);
  if (lane == 0u) out[64u * LC_VALUE_SLOTS] = n;
#endif
}

// ---------------------------------------------------------------- host

CucheckOut lanecheck_run(at::Tensor expected, int64_t seed_arg, int64_t rounds,
                         int64_t blocks_arg, int64_t max_records,
                         c10::optional<at::Tensor> dump, c10::optional<CuInject> inject) {
  CuLaunch l = cu_prepare("lanecheck", expected, seed_arg, rounds, blocks_arg, max_records,
                          dump, inject);
  const at::hip::OptionalHIPGuardMasqueradingAsCUDA guard(at::device_of(expected));
  return cu_launch_timed(lanecheck_kernel, l, MAX_LDS_BYTES);
}

// What one wave folds for one stage and round as an int32 tensor on the
// current GPU: LC_VALUE_SLOTS rows of 64 lanes, then the number of rows
// the stage filled.
at::Tensor lanecheck_values(int64_t seed_arg, int64_t stage, int64_t round) {
  cu_check_wave_args("lanecheck", seed_arg, stage, round);
  at::Tensor out = at::zeros({(int64_t)(64 * LC_VALUE_SLOTS + 1)},
                             at::TensorOptions().dtype(at::kInt).device(at::kCUDA));
  return cu_launch_values(lanecheck_values_kernel, WAVE, 0, out, (u32)seed_arg, (u32)stage,
                          (u32)round, (u32*)out.data_ptr());
}

typedef std::tuple<int64_t, int64_t, int64_t, int64_t> LcDppRow;

// Called from gpuprobe.hip's PYBIND11_MODULE; GIL released like the
// other probes: a default run holds the GPU for about half a second
// (profiles/lanecheck_mi355x.json).
void bind_lanecheck(py::module_& m) {
  m.def("lanecheck_run", &lanecheck_run,
        "cross-lane integrity run -> (mismatches, first_bad_round, stage_mask, "
        "records, waves_on, elapsed_s)",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("expected"), py::arg("seed"), py::arg("rounds"), py::arg("blocks"),
        py::arg("max_records") = 16, py::arg("dump") = py::none(),
        py::arg("inject") = py::none());
  m.def("lanecheck_values", &lanecheck_values,
        "values one wave folds for one stage and round as int32 [48 rows * 64 lanes + 1]",
        py::call_guard<py::gil_scoped_release>(),
        py::arg("seed"), py::arg("stage"), py::arg("round"));
  m.def("lanecheck_layout", []() {
          std::vector<LcDppRow> dpp;
          for (u32 j = 0; j < LC_N_DPP; ++j)
            dpp.emplace_back(LC_DPP[j].ctrl, LC_DPP[j].row_mask, LC_DPP[j].bank_mask,
                             LC_DPP[j].bound_ctrl);
          std::vector<int64_t> swizzle(LC_SWIZZLE, LC_SWIZZLE + LC_N_SWIZZLE);
          std::vector<int64_t> readlane(LC_READLANE, LC_READLANE + LC_N_READLANE);
          return std::make_tuple((int64_t)LC_PERIOD, (int64_t)LC_VALUE_SLOTS, dpp, swizzle,
                                 readlane);
        },
        "(period, value rows, DPP table, swizzle offsets, constant readlane indices)");
}
