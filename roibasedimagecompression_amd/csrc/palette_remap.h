// The pack / evaluate / carry functions and constants of the nearest-colour remap, shared by its kernel (palette_remap.hip) and by the
// palette refinement that assigns pixels with the same arithmetic (palette_refine.hip) and by the ladder's moments pass
// (palette_ladder.hip), with the rounded mean that the refinement, the reduction's merges and the ladder's rungs share, and the
// reduction's row cap, sum limit and clamp that the ladder shares; and, at the end, the body of the remap kernel and its argument check,
// which the batched form (palette_batch.hip) runs per image.  The derivation is in palette_remap.hip.
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

// ---- the remap kernel's body, shared by palette_remap.hip (one image a launch) and palette_batch.hip (one image per grid row) ----
// A workgroup takes chunks of 256 x 8 pixels (lane l: pixels base + l + 256 q, so index stores coalesce) grid-stride, and walks the
// palette tile by tile through LDS for each.  A palette of one tile is staged once.  The last tile is padded to an even length
// with a copy of its last entry under the next local index: equal key, higher index, never the minimum.
// It is workgroup `bid` of the `nblk` that share the image: the launch's own for one image, those of a grid row for a batch.
template <typename IdxT>
__device__ __forceinline__ void remap_body(const uint8_t* __restrict__ rgb, long long n_px,
                                           const uint8_t* __restrict__ pal, int K,
                                           const uint8_t* __restrict__ cls, int n_classes,
                                           IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums,
                                           long long bid, long long nblk) {
  __shared__ uint4 s_pal[kRemapTile / 2];                                             // two entries per 16-byte read
  __shared__ unsigned long long s_sum[kRemapBlock / 64][kRemapMaxClasses + 1][2];     // per wave: rows {pixels, SSE}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < (kRemapBlock / 64) * (kRemapMaxClasses + 1) * 2; i += kRemapBlock) (&s_sum[0][0][0])[i] = 0ull;
  const int n_tiles = (K + kRemapTile - 1) / kRemapTile;
  constexpr long long kChunk = (long long)kRemapBlock * kRemapPx;
  const long long n_chunks = (n_px + kChunk - 1) / kChunk;
  unsigned long long all_sse = 0ull;
  bool staged = false;

  for (long long chunk = bid; chunk < n_chunks; chunk += nblk) {          // (block uniform: the barriers below are safe)
    const long long base = chunk * kChunk + threadIdx.x;
    uint32_t px[kRemapPx], bkey[kRemapPx], bidx[kRemapPx];
#pragma unroll
    for (int q = 0; q < kRemapPx; ++q) {
      const long long p = base + (long long)q * kRemapBlock;
      px[q] = p < n_px ? remap_pack_px(rgb + p * 3) : 0u;
      bkey[q] = 0xFFFFFFFFu;
      bidx[q] = 0u;
    }
    for (int t = 0; t < n_tiles; ++t) {
      const int tile_base = t * kRemapTile, len = min(kRemapTile, K - tile_base), len2 = (len + 1) & ~1;
      if (n_tiles > 1 || !staged) {
        __syncthreads();                                                               // every wave is done with the previous tile
        RemapEntry* s_e = reinterpret_cast<RemapEntry*>(s_pal);
        for (int j = threadIdx.x; j < len2; j += kRemapBlock) s_e[j] = remap_pack_entry(pal + (long long)(tile_base + min(j, len - 1)) * 3, j);
        __syncthreads();
        staged = true;
      }
      uint32_t best[kRemapPx];
#pragma unroll
      for (int q = 0; q < kRemapPx; ++q) best[q] = 0xFFFFFFFFu;
#pragma unroll 2
      for (int j = 0; j < len2 / 2; ++j) {
        const uint4 e = s_pal[j];                                                      // wave-uniform address: broadcast
#pragma unroll
        for (int q = 0; q < kRemapPx; ++q) {
          best[q] = min(best[q], remap_eval(px[q], RemapEntry{e.x, e.y}));
          best[q] = min(best[q], remap_eval(px[q], RemapEntry{e.z, e.w}));
        }
      }
#pragma unroll
      for (int q = 0; q < kRemapPx; ++q) remap_carry(best[q], tile_base, bkey[q], bidx[q]);
    }
    uint32_t dist[kRemapPx];
#pragma unroll
    for (int q = 0; q < kRemapPx; ++q) {
      const long long p = base + (long long)q * kRemapBlock;
      const bool in = p < n_px;
      dist[q] = in ? remap_dist(px[q], bkey[q]) : 0u;
      if (in) idx_out[p] = (IdxT)bidx[q];
      all_sse += dist[q];
    }
    if (n_classes > 0) {                                                               // per class: lane sums in 64 bits, one wave reduction
      unsigned c[kRemapPx];
#pragma unroll
      for (int q = 0; q < kRemapPx; ++q) {
        const long long p = base + (long long)q * kRemapBlock;
        c[q] = p < n_px ? (unsigned)cls[p] : 0xFFFFFFFFu;
      }
      for (int k = 0; k < n_classes; ++k) {
        unsigned long long v = 0ull, n = 0ull;
#pragma unroll
        for (int q = 0; q < kRemapPx; ++q) {
          v += c[q] == (unsigned)k ? dist[q] : 0u;
          n += c[q] == (unsigned)k ? 1u : 0u;
        }
        v = wave_sum(v);
        n = wave_sum(n);
        if (lane == 0) { s_sum[wv][k][0] += n; s_sum[wv][k][1] += v; }               // this wave's table: no other writer
      }
    }
  }
  all_sse = wave_sum(all_sse);
  if (lane == 0) s_sum[wv][kRemapMaxClasses][1] = all_sse;
  __syncthreads();
  if ((int)threadIdx.x < (n_classes + 1) * 2) {                                        // one atomic per workgroup, row and column
    const int k = threadIdx.x >> 1, col = threadIdx.x & 1;
    unsigned long long t = 0ull;
    if (k < n_classes) {
      for (int i = 0; i < kRemapBlock / 64; ++i) t += s_sum[i][k][col];
    } else if (col == 1) {
      for (int i = 0; i < kRemapBlock / 64; ++i) t += s_sum[i][kRemapMaxClasses][1];
    } else {                                                                           // the pixels of this workgroup's chunks
      for (long long chunk = bid; chunk < n_chunks; chunk += nblk) t += (unsigned long long)min(kChunk, n_px - chunk * kChunk);
    }
    if (t) atomicAdd(&sums[threadIdx.x], t);
  }
}


static inline int remap_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                       const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  if (!rgb || !palette || !idx_out || !sums) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: null argument");
  if (K < 1 || n_pixels < 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: K >= 1 and n_pixels >= 0 are required");
  if (n_classes < 0 || n_classes > kRemapMaxClasses) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: n_classes must be 0..16");
  if (!cls && n_classes != 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: n_classes must be 0 without a class map");
  if (idx_elem_bytes != 1 && idx_elem_bytes != 2 && idx_elem_bytes != 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: idx_elem_bytes must be 1, 2 or 4");
  if ((uintptr_t)idx_out & (uintptr_t)(idx_elem_bytes - 1)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: misaligned indices");
  if ((uintptr_t)sums & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: misaligned sums");
  if (idx_elem_bytes == 1 && K > 256) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: 1-byte indices hold at most 256 colours");
  if (K > kRemapMaxK) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_remap: at most 65536 colours");
  return 0;
}

}  // namespace rhccq
