// Cross-lane reductions and scans of one u32 per lane on DPP (VALU moves, no LDS crossbar), stated once for every kernel that uses them.
// The control words (gfx9 encoding), by name:
//   0xB1  quad_perm [1,0,3,2]      0x4E  quad_perm [2,3,0,1]      0x141 row_half_mirror      0x140 row_mirror
//   0x111, 0x112, 0x114, 0x118  row_shr:1, 2, 4, 8                 0x142 row_bcast:15         0x143 row_bcast:31
// A DPP row is 16 lanes.  The butterflies run with both masks full and bound_ctrl set, so their `old` operand (0) is dead; the two
// broadcasts of the scan run under a row mask without bound_ctrl, and the rows outside the mask add that 0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rhccq {

template <int kCtrl, int kRowMask = 0xF, bool kBound = true>
__device__ __forceinline__ unsigned dpp_move(unsigned v) {
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xF, kBound);
}

// the butterfly: every lane gets op over its aligned group of kWidth lanes (2, 4, 8 or 16: inside one DPP row); op commutes and associates
template <int kWidth, typename Op>
__device__ __forceinline__ unsigned dpp_group_reduce(unsigned v, Op op) {
  static_assert(kWidth == 2 || kWidth == 4 || kWidth == 8 || kWidth == 16, "an aligned group inside one DPP row");
  if (kWidth >= 2) v = op(v, dpp_move<0xB1>(v));
  if (kWidth >= 4) v = op(v, dpp_move<0x4E>(v));
  if (kWidth >= 8) v = op(v, dpp_move<0x141>(v));
  if (kWidth >= 16) v = op(v, dpp_move<0x140>(v));
  return v;
}
template <int kWidth>
__device__ __forceinline__ unsigned dpp_group_sum(unsigned v) { return dpp_group_reduce<kWidth>(v, [](unsigned a, unsigned b) { return a + b; }); }
template <int kWidth>
__device__ __forceinline__ unsigned dpp_group_max(unsigned v) { return dpp_group_reduce<kWidth>(v, [](unsigned a, unsigned b) { return max(a, b); }); }
template <int kWidth>
__device__ __forceinline__ unsigned dpp_group_min(unsigned v) { return dpp_group_reduce<kWidth>(v, [](unsigned a, unsigned b) { return min(a, b); }); }

// inclusive scan over lanes 0 .. kLanes - 1 of every aligned group of kLanes (16, 32 or 64): four shifted adds inside each row, then a
// broadcast a doubling.  At 32, what lanes 32 .. 63 end up with is not a scan of their own.  The group's total must fit 32 bits.
template <int kLanes>
__device__ __forceinline__ unsigned dpp_incscan_u32(unsigned v) {
  static_assert(kLanes == 16 || kLanes == 32 || kLanes == 64, "whole DPP rows");
  v += dpp_move<0x111>(v);
  v += dpp_move<0x112>(v);
  v += dpp_move<0x114>(v);
  v += dpp_move<0x118>(v);                                           // -> scan inside each row of 16
  if (kLanes >= 32) v += dpp_move<0x142, 0xA, false>(v);             // row 0's total into row 1, row 2's into row 3
  if (kLanes >= 64) v += dpp_move<0x143, 0xC, false>(v);             // lane 31's into rows 2 and 3
  return v;
}

// wave-uniform results (scalar): sum (< 2^32 required) / max over the 64 lanes
__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
  v = dpp_group_sum<16>(v);
  return (unsigned)__builtin_amdgcn_readlane((int)v, 0) + (unsigned)__builtin_amdgcn_readlane((int)v, 16) +
         (unsigned)__builtin_amdgcn_readlane((int)v, 32) + (unsigned)__builtin_amdgcn_readlane((int)v, 48);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  v = dpp_group_max<16>(v);
  return max(max((unsigned)__builtin_amdgcn_readlane((int)v, 0), (unsigned)__builtin_amdgcn_readlane((int)v, 16)),
             max((unsigned)__builtin_amdgcn_readlane((int)v, 32), (unsigned)__builtin_amdgcn_readlane((int)v, 48)));
}
// exact u64 inclusive scan of values < 2^32 from two u32 scans of 16-bit limbs (limb totals < 2^32)
__device__ __forceinline__ unsigned long long wave_incscan_limbs(unsigned v) {
  const unsigned hi = dpp_incscan_u32<64>(v >> 16), lo = dpp_incscan_u32<64>(v & 0xffffu);
  return ((unsigned long long)hi << 16) + lo;
}

}  // namespace rhccq
