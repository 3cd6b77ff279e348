// The nearest-colour search: its pack / evaluate / carry functions and constants, and the ONE device loop (remap_search) and the ONE
// host loop (remap_search_host) that run them.  The remap (palette_remap.hip), the refinement's assignment (palette_refine.h) and the
// ladder's moments pass (palette_ladder.hip) each call remap_search with what they do with a chunk's winners; their host forms call
// remap_search_host.  Around it: the argument checks, the grid size and the index-width dispatch these operations share; the rounded
// mean that the refinement, the reduction's merges and the ladder's rungs share; the reduction's row cap, sum limit and clamp that the
// ladder shares; and, at the end, the body of the remap kernel and its argument check, which the batched form (palette_batch.hip) runs
// per image.  The derivation is in palette_remap.hip.
#pragma once
#include "rhccq_common.h"

#include <vector>

namespace rhccq {

constexpr int kRemapBlock = 256;      // lanes of a workgroup
constexpr int kRemapPx = 8;           // pixels a lane keeps in registers: one LDS read of two entries feeds 16 evaluations
constexpr long long kRemapChunk = (long long)kRemapBlock * kRemapPx;      // pixels a workgroup takes at a time
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

// ---- the search on the device: the one loop of the remap, the refinement's assignment and the moments pass ----
// A workgroup takes chunks of 256 x 8 pixels (lane l: pixels base + l + 256 q, so index stores coalesce) grid-stride, and walks the
// palette tile by tile through LDS for each.  A palette of one tile is staged once.  The last tile is padded to an even length
// with a copy of its last entry under the next local index: equal key, higher index, never the minimum.
// It is workgroup `bid` of the `nblk` that share the image: the launch's own for one image, those of a grid row for a batch.
// After each chunk it calls tail(base, px, bkey, bidx): the lane's first pixel, and per pixel q (base + 256 q) the packed pixel (0
// outside the picture), the winner's key and its row.  The whole workgroup must call this together and `tail` must not leave early
// for part of it: the barriers of the staging are workgroup-uniform only then.
template <typename Tail>
__device__ __forceinline__ void remap_search(const uint8_t* __restrict__ rgb, long long n_px, const uint8_t* __restrict__ pal, int K, long long bid,
                                             long long nblk, Tail&& tail) {
  __shared__ uint4 s_pal[kRemapTile / 2];                                             // two entries per 16-byte read
  const int n_tiles = (K + kRemapTile - 1) / kRemapTile;
  const long long n_chunks = (n_px + kRemapChunk - 1) / kRemapChunk;
  bool staged = false;

  for (long long chunk = bid; chunk < n_chunks; chunk += nblk) {          // (block uniform: the barriers below are safe)
    const long long base = chunk * kRemapChunk + threadIdx.x;
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
    tail(base, px, bkey, bidx);
  }
}

// ---- the search on the host: the same pack / evaluate / carry, serially ----
// the palette as the tiles hold it: entry j under its tile-local index
static inline std::vector<RemapEntry> remap_pack_palette(const uint8_t* pal, int K) {
  std::vector<RemapEntry> ent((size_t)K);
  for (int j = 0; j < K; ++j) ent[j] = remap_pack_entry(pal + (int64_t)j * 3, j % kRemapTile);
  return ent;
}
// one packed pixel against the packed palette, tile by tile -> the winner's row; its key through *key
static inline uint32_t remap_search_host(uint32_t px, const std::vector<RemapEntry>& ent, uint32_t* key) {
  const int K = (int)ent.size();
  uint32_t idx = 0u;
  *key = 0xFFFFFFFFu;
  for (int tile_base = 0; tile_base < K; tile_base += kRemapTile) {
    const int len = K - tile_base < kRemapTile ? K - tile_base : kRemapTile;
    uint32_t best = 0xFFFFFFFFu;
    for (int j = 0; j < len; ++j) {
      const uint32_t v = remap_eval(px, ent[tile_base + j]);
      best = v < best ? v : best;
    }
    remap_carry(best, tile_base, *key, idx);
  }
  return idx;
}

// ---- argument checks, grid and index width shared by the remap, the refinement and the moments (`what`: the operation's name) ----
static inline int remap_fail(rhccq_ctx* ctx, int code, const char* what, const char* msg) { return rhccq_fail(ctx, code, (std::string(what) + msg).c_str()); }
// the class map and the number of classes (also of palette_runs.h's check and of the cells, palette_build.h)
static inline int classes_check(rhccq_ctx* ctx, const char* what, const void* cls, int32_t n_classes) {
  if (n_classes < 0 || n_classes > kRemapMaxClasses) return remap_fail(ctx, RHCCQ_E_ARG, what, ": n_classes must be 0..16");
  if (!cls && n_classes != 0) return remap_fail(ctx, RHCCQ_E_ARG, what, ": n_classes must be 0 without a class map");
  return 0;
}
// pixels, palette and class map; any_null: one of the operation's required pointers is null
static inline int search_check(rhccq_ctx* ctx, const char* what, bool any_null, int64_t n_pixels, int32_t K, const void* cls, int32_t n_classes) {
  if (any_null) return remap_fail(ctx, RHCCQ_E_ARG, what, ": null argument");
  if (K < 1 || n_pixels < 0) return remap_fail(ctx, RHCCQ_E_ARG, what, ": K >= 1 and n_pixels >= 0 are required");
  return classes_check(ctx, what, cls, n_classes);
}
// the n_classes + 1 weights of the refinement and the cells (null: all ones) into the kernel's table; *top: the largest, which is > 0
static inline int weights_check(rhccq_ctx* ctx, const char* what, const int32_t* weights, int32_t n_classes, uint32_t* table, uint32_t* top) {
  *top = 0u;
  for (int i = 0; i <= n_classes; ++i) {
    const int32_t w = weights ? weights[i] : 1;
    if (w < 0 || w > 255) return remap_fail(ctx, RHCCQ_E_ARG, what, ": weights must be 0..255");
    table[i] = (uint32_t)w;
    *top = (uint32_t)w > *top ? (uint32_t)w : *top;
  }
  return *top ? 0 : remap_fail(ctx, RHCCQ_E_ARG, what, ": at least one weight must be > 0");
}
// the last test of each: the one that is a limit and not an argument error
static inline int search_limit(rhccq_ctx* ctx, const char* what, int32_t K) {
  return K > kRemapMaxK ? remap_fail(ctx, RHCCQ_E_LIMIT, what, ": at most 65536 colours") : 0;
}
// an index buffer: its element width and alignment, and (apart: each operation tests another buffer in between) what the width holds
static inline int index_check(rhccq_ctx* ctx, const char* what, const void* idx_out, int32_t idx_elem_bytes) {
  if (idx_elem_bytes != 1 && idx_elem_bytes != 2 && idx_elem_bytes != 4) return remap_fail(ctx, RHCCQ_E_ARG, what, ": idx_elem_bytes must be 1, 2 or 4");
  if ((uintptr_t)idx_out & (uintptr_t)(idx_elem_bytes - 1)) return remap_fail(ctx, RHCCQ_E_ARG, what, ": misaligned indices");
  return 0;
}
static inline int index_rows_check(rhccq_ctx* ctx, const char* what, int32_t idx_elem_bytes, int32_t K) {
  return idx_elem_bytes == 1 && K > 256 ? remap_fail(ctx, RHCCQ_E_ARG, what, ": 1-byte indices hold at most 256 colours") : 0;
}

// workgroups of a launch over n_px pixels: one per chunk, at most `cap`, at least one
static inline unsigned remap_blocks(long long n_px, long long cap) {
  const long long chunks = (n_px + kRemapChunk - 1) / kRemapChunk, blocks = chunks < cap ? chunks : cap;
  return (unsigned)(blocks < 1 ? 1 : blocks);
}

// f(a null pointer of the index type of that width): its type picks the template instance
template <typename F>
static inline void index_dispatch(int idx_elem_bytes, F&& f) {
  switch (idx_elem_bytes) {
    case 1: f((uint8_t*)nullptr); break;
    case 2: f((uint16_t*)nullptr); break;
    default: f((uint32_t*)nullptr);
  }
}

// ---- the remap kernel's body, shared by palette_remap.hip (one image a launch) and palette_batch.hip (one image per grid row) ----
template <typename IdxT>
__device__ __forceinline__ void remap_body(const uint8_t* __restrict__ rgb, long long n_px,
                                           const uint8_t* __restrict__ pal, int K,
                                           const uint8_t* __restrict__ cls, int n_classes,
                                           IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums,
                                           long long bid, long long nblk) {
  __shared__ unsigned long long s_sum[kRemapBlock / 64][kRemapMaxClasses + 1][2];     // per wave: rows {pixels, SSE}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < (kRemapBlock / 64) * (kRemapMaxClasses + 1) * 2; i += kRemapBlock) (&s_sum[0][0][0])[i] = 0ull;
  unsigned long long all_sse = 0ull;

  remap_search(rgb, n_px, pal, K, bid, nblk, [&](long long base, auto& px, auto& bkey, auto& bidx) {
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
  });
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
      const long long n_chunks = (n_px + kRemapChunk - 1) / kRemapChunk;
      for (long long chunk = bid; chunk < n_chunks; chunk += nblk) t += (unsigned long long)min(kRemapChunk, n_px - chunk * kRemapChunk);
    }
    if (t) atomicAdd(&sums[threadIdx.x], t);
  }
}

static inline int remap_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                       const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  const char* const what = "palette_remap";
  if (const int rc = search_check(ctx, what, !rgb || !palette || !idx_out || !sums, n_pixels, K, cls, n_classes)) return rc;
  if (const int rc = index_check(ctx, what, idx_out, idx_elem_bytes)) return rc;
  if ((uintptr_t)sums & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap: misaligned sums");
  if (const int rc = index_rows_check(ctx, what, idx_elem_bytes, K)) return rc;
  return search_limit(ctx, what, K);
}

}  // namespace rhccq
