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
// The pack / evaluate / carry functions, the device loop that runs them (remap_search) and its serial host form (remap_search_host)
// are in palette_remap.h: the palette refinement and the ladder's moments pass search with them too.
#include "palette_remap.h"

namespace rhccq {

// The kernel's body (remap_body: remap_search and what follows a chunk) and the argument check are in palette_remap.h: the batched
// form (palette_batch.hip) runs them per image.
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
  const std::vector<RemapEntry> ent = remap_pack_palette(pal, K);
  for (int64_t p = 0; p < n_px; ++p) {
    const uint32_t px = remap_pack_px(rgb + p * 3);
    uint32_t key;
    const uint32_t idx = remap_search_host(px, ent, &key);
    const uint32_t d = remap_dist(px, key);
    idx_out[p] = (IdxT)idx;
    if (n_classes > 0 && cls[p] < n_classes) { sums[cls[p] * 2] += 1; sums[cls[p] * 2 + 1] += d; }
    sums[n_classes * 2] += 1;
    sums[n_classes * 2 + 1] += d;
  }
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
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  // 8 workgroups of 4 waves per CU (the kernel needs 9280 bytes of LDS and at most 62 registers), never more than there are chunks
  const dim3 grid(remap_blocks(n_pixels, (long long)ctx->compute_units * 8)), block(kRemapBlock);
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(palette_remap_kernel<T>, grid, block, 0, ctx->stream, rgb, (long long)n_pixels, palette, (int)K, cls, (int)n_classes, (T*)idx_out,
                       (unsigned long long*)sums);
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_remap_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                             void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = remap_check(nullptr, rgb, n_pixels, palette, K, cls, n_classes, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i < (n_classes + 1) * 2; ++i) sums[i] = 0;
  index_dispatch(idx_elem_bytes, [&](auto* t) { remap_host(rgb, n_pixels, palette, K, cls, n_classes, (decltype(t))idx_out, sums); });
  return 0;
}

}  // extern "C"
