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

// The kernel's body (remap_body) and the argument check are in palette_remap.h: the batched form (palette_batch.hip) runs them per image.
template <typename IdxT>
__global__ __launch_bounds__(kRemapBlock) void palette_remap_kernel(const uint8_t* __restrict__ rgb, long long n_px,
                                                                    const uint8_t* __restrict__ pal, int K,
                                                                    const uint8_t* __restrict__ cls, int n_classes,
                                                                    IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums) {
  remap_body<IdxT>(rgb, n_px, pal, K, cls, n_classes, idx_out, sums, blockIdx.x, gridDim.x);
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
