// The pack / evaluate / carry functions and constants of the nearest-colour remap, shared by its kernel (palette_remap.hip) and by the
// palette refinement that assigns pixels with the same arithmetic (palette_refine.hip) and by the ladder's moments pass
// (palette_ladder.hip), with the rounded mean that the refinement, the reduction's merges and the ladder's rungs share, and the
// reduction's row cap, sum limit and clamp that the ladder shares.  The derivation is in palette_remap.hip.
#pragma once
#include "rhccq_common.h"

namespace rhccq {

constexpr int kRemapBlock = 256;      // lanes of a workgroup
constexpr int kRemapPx = 8;           // pixels a lane keeps in registers: one LDS read of two entries feeds 16 evaluations
constexpr int kRemapTile = 1024;      // palette entries staged in LDS at a time (8 KiB); <= 4096 (12 index bits)
constexpr int kRemapIdxBits = 12;
constexpr int kRemapMaxClasses = 16;
constexpr int kRemapMaxK = 65536;     // the bound of the reference's uint16 mapping array (clustering.py:373)
static_assert(kRemapTile <= (1 << kRemapIdxBits) && kRemapTile % 2 == 0, "tile-local index must fit its 12 bits");

struct RemapEntry { uint32_t inv, w; };

__host__ __device__ __forceinline__ uint32_t remap_dot(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
  return (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u);
#endif
}
__host__ __device__ __forceinline__ uint32_t remap_pack_px(const uint8_t* p) { return ((uint32_t)p[0] << 16) | ((uint32_t)p[1] << 8) | p[2]; }
// entry `local` of a tile from its three bytes
__host__ __device__ __forceinline__ RemapEntry remap_pack_entry(const uint8_t* c, int local) {
  const uint32_t k = remap_pack_px(c);
  return {0x00FFFFFFu - k, (remap_dot(k, k) << kRemapIdxBits) | (uint32_t)local};
}
// (key << 12 | local index) of pixel p against one entry
__host__ __device__ __forceinline__ uint32_t remap_eval(uint32_t p, RemapEntry e) { return (remap_dot(p, e.inv) << (kRemapIdxBits + 1)) + e.w; }
// a tile's winner against the winner so far: strict <, so an equal key of a later tile never replaces an earlier index
__host__ __device__ __forceinline__ void remap_carry(uint32_t tile_best, int tile_base, uint32_t& key, uint32_t& idx) {
  const uint32_t k = tile_best >> kRemapIdxBits;
  if (k < key) {
    key = k;
    idx = (uint32_t)tile_base + (tile_best & ((1u << kRemapIdxBits) - 1u));
  }
}
// ---- shared by the reduction (palette_reduce.hip) and the ladder built on its log (palette_ladder.hip) ----
// rows the reduction's resident workgroup holds: 4096 * 12 bytes = 48 KiB of LDS, which with the reduction scratch stays below the 64 KiB a
// workgroup gets without asking; row ids also fit uint16 slots (0xFFFF = none).  The device forms of the ladder's curve and rung share the
// cap: the reduction is the only producer of a merges log in device memory.
constexpr int kReduceMaxRows = 4096;
constexpr unsigned long long kReduceMaxSum = 0xFFFFFFFFull;      // the counts of a chain add up to at most this
// a count as it enters the sum check: clamped so that 65536 of them cannot overflow
__host__ __device__ __forceinline__ unsigned long long reduce_clamp(unsigned long long v) { return v > kReduceMaxSum ? kReduceMaxSum + 1ull : v; }
// the weighted mean rounded to nearest, halves up (n > 0; s <= 255 n): the rule of the refinement's update and of every merged centre
__host__ __device__ __forceinline__ uint32_t refine_mean(unsigned long long s, unsigned long long n) { return (uint32_t)((2ull * s + n) / (2ull * n)); }
// the squared distance from the winning key
__host__ __device__ __forceinline__ uint32_t remap_dist(uint32_t p, uint32_t key) {
  const int s = (int)((p & 255u) + ((p >> 8) & 255u) + ((p >> 16) & 255u));
  return (uint32_t)((int)key + (int)remap_dot(p, p) - 510 * s);
}

}  // namespace rhccq
