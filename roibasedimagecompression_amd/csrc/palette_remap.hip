// Nearest-colour remap onto a given palette (EXTENSION, no reference counterpart: every reference path builds the palette and the
// index map together).  idx[p] = argmin_j |rgb[p] - palette[j]|^2 in exact integers, ties to the lowest j, and the squared error of
// every pixel summed per class of a class map and over the picture.
//
// Arithmetic.  |p - c|^2 = |p|^2 + |c|^2 - 2 p.c, and with c' = 255 - c (per channel) p.c = 255 (pr + pg + pb) - p.c', so
//     |p - c|^2 = [ |p|^2 - 510 (pr + pg + pb) ]  +  |c|^2 + 2 p.c'
// The bracket does not depend on c: the ordering over the palette is that of key = |c|^2 + 2 p.c', a NON-NEGATIVE integer of at most
// 3 * 255^2 + 2 * 3 * 255^2 = 585 225 < 2^20.  A palette tile has kRemapTile <= 4096 entries, so (key << 12 | index in the tile)
// fits one 32-bit word (585 225 * 4096 + 4095 = 2 397 085 695 < 2^32) whose unsigned minimum is the smallest key and, among equal
// keys, the lowest index.  (The distance itself needs 18 bits and a whole-palette index 16: those two do not fit one word, which is
// why the index is tile-local and the winner is carried from tile to tile on two registers with a strict <.)
// An entry is two words: c' packed as 0x00R'G'B', and w = |c|^2 << 12 | index in the tile.  Two entries are evaluated together:
//     v_dot4_u32_u8 t = p . c'      v_lshl_add_u32 v = (t << 13) + w      (for each)      v_min3_u32 best = min(best, v0, v1)
// 2.5 vector integer operations an evaluation, with the two entries read from LDS by all lanes at one address (a broadcast: no
// bank conflict).
// The host form runs the same pack / evaluate / carry functions serially.
// The pack / evaluate / carry functions themselves are in palette_remap.h (the palette refinement assigns with them too).
#include "palette_remap.h"

namespace rhccq {

// A workgroup takes chunks of 256 x 8 pixels (lane l: pixels base + l + 256 q, so index stores coalesce) grid-stride, and walks the
// palette tile by tile through LDS for each.  A palette of one tile is staged once.  The last tile is padded to an even length
// with a copy of its last entry under the next local index: equal key, higher index, never the minimum.
template <typename IdxT>
__global__ __launch_bounds__(kRemapBlock) void palette_remap_kernel(const uint8_t* __restrict__ rgb, long long n_px,
                                                                    const uint8_t* __restrict__ pal, int K,
                                                                    const uint8_t* __restrict__ cls, int n_classes,
                                                                    IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums) {
  __shared__ uint4 s_pal[kRemapTile / 2];                                             // two entries per 16-byte read
  __shared__ unsigned long long s_sum[kRemapBlock / 64][kRemapMaxClasses + 1][2];     // per wave: rows {pixels, SSE}
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < (kRemapBlock / 64) * (kRemapMaxClasses + 1) * 2; i += kRemapBlock) (&s_sum[0][0][0])[i] = 0ull;
  const int n_tiles = (K + kRemapTile - 1) / kRemapTile;
  constexpr long long kChunk = (long long)kRemapBlock * kRemapPx;
  const long long n_chunks = (n_px + kChunk - 1) / kChunk;
  unsigned long long all_sse = 0ull;
  bool staged = false;

  for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {          // (block uniform: the barriers below are safe)
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
      for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) t += (unsigned long long)min(kChunk, n_px - chunk * kChunk);
    }
    if (t) atomicAdd(&sums[threadIdx.x], t);
  }
}

static int remap_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
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

template <typename IdxT>
static void remap_host(const uint8_t* rgb, int64_t n_px, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, IdxT* idx_out,
                       uint64_t* sums) {
  const int n_tiles = (K + kRemapTile - 1) / kRemapTile;
  RemapEntry* ent = new RemapEntry[K];
  for (int j = 0; j < K; ++j) ent[j] = remap_pack_entry(pal + (int64_t)j * 3, j % kRemapTile);
  for (int64_t p = 0; p < n_px; ++p) {
    const uint32_t px = remap_pack_px(rgb + p * 3);
    uint32_t key = 0xFFFFFFFFu, idx = 0u;
    for (int t = 0; t < n_tiles; ++t) {
      const int tile_base = t * kRemapTile, len = K - tile_base < kRemapTile ? K - tile_base : kRemapTile;
      uint32_t best = 0xFFFFFFFFu;
      for (int j = 0; j < len; ++j) {
        const uint32_t v = remap_eval(px, ent[tile_base + j]);
        best = v < best ? v : best;
      }
      remap_carry(best, tile_base, key, idx);
    }
    const uint32_t d = remap_dist(px, key);
    idx_out[p] = (IdxT)idx;
    if (n_classes > 0 && cls[p] < n_classes) { sums[cls[p] * 2] += 1; sums[cls[p] * 2 + 1] += d; }
    sums[n_classes * 2] += 1;
    sums[n_classes * 2 + 1] += d;
  }
  delete[] ent;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_remap_tile(void) { return kRemapTile; }

int rhccq_palette_remap(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls,
                        int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = remap_check(ctx, rgb, n_pixels, palette, K, cls, n_classes, idx_out, idx_elem_bytes, sums)) return rc;
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)(n_classes + 1) * 2 * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  if (ctx->compute_units <= 0) RHCCQ_HIP(ctx, hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const int cus = ctx->compute_units;
  // 8 workgroups of 4 waves per CU (the kernel needs 9280 bytes of LDS and at most 62 registers), never more than there are chunks
  const long long chunks = (n_pixels + (long long)kRemapBlock * kRemapPx - 1) / ((long long)kRemapBlock * kRemapPx);
  const long long blocks = chunks < (long long)cus * 8 ? chunks : (long long)cus * 8;
  const dim3 grid((unsigned)(blocks < 1 ? 1 : blocks)), block(kRemapBlock);
  switch (idx_elem_bytes) {
    case 1:
      hipLaunchKernelGGL(palette_remap_kernel<uint8_t>, grid, block, 0, ctx->stream, rgb, (long long)n_pixels, palette, (int)K, cls,
                         (int)n_classes, (uint8_t*)idx_out, (unsigned long long*)sums);
      break;
    case 2:
      hipLaunchKernelGGL(palette_remap_kernel<uint16_t>, grid, block, 0, ctx->stream, rgb, (long long)n_pixels, palette, (int)K, cls,
                         (int)n_classes, (uint16_t*)idx_out, (unsigned long long*)sums);
      break;
    default:
      hipLaunchKernelGGL(palette_remap_kernel<uint32_t>, grid, block, 0, ctx->stream, rgb, (long long)n_pixels, palette, (int)K, cls,
                         (int)n_classes, (uint32_t*)idx_out, (unsigned long long*)sums);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_remap_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                             void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = remap_check(nullptr, rgb, n_pixels, palette, K, cls, n_classes, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i < (n_classes + 1) * 2; ++i) sums[i] = 0;
  switch (idx_elem_bytes) {
    case 1: remap_host<uint8_t>(rgb, n_pixels, palette, K, cls, n_classes, (uint8_t*)idx_out, sums); break;
    case 2: remap_host<uint16_t>(rgb, n_pixels, palette, K, cls, n_classes, (uint16_t*)idx_out, sums); break;
    default: remap_host<uint32_t>(rgb, n_pixels, palette, K, cls, n_classes, (uint32_t*)idx_out, sums);
  }
  return 0;
}

}  // extern "C"
