// Position-only (pattern) dither onto a given palette (EXTENSION, no reference counterpart): Thomas Knoll's pattern dithering in exact
// integers.  With n the size (2, 4 or 8), N = n * n, s the pixel's class's strength (0..256) and p the pixel, per channel
//     e = 0;   for i in 0 .. N-1:   t = clamp(p + floor((s e + 128) / 256), 0, 255);   c_i = the remap's nearest row of t (ties to the lowest);
//                                   e = e + p - palette[c_i]
//     out = the candidates c_0 .. c_N-1 ordered by (299 R + 587 G + 114 B of palette[c], then c), duplicates kept, at place M_n[y mod n][x mod n]
// M_n is the Bayer matrix (palette_pattern.h).  A pixel's index depends on the pixel and its position only: no pixel waits for another.
// The step functions are in palette_pattern.h; the host form runs them serially.
//
// The kernel is the remap's search run N times per pixel.  No workspace, no hand-over, no wait, one barrier (behind the staging).
//   palette  staged once per workgroup in LDS as RemapEntry under its row number (K <= 4096: 12 bits), padded to an even length with an
//            entry that never wins; one 16-byte broadcast read feeds two evaluations of every pixel a lane holds;
//   pixels   a lane holds P pixels side by side (8, 4, 1 for n = 2, 4, 8) with their accumulated errors in registers: P chains in flight
//            hide each other's latency, and a read of two entries feeds 2 P evaluations;
//   strips   candidate i of a pixel goes to the lane's LDS strip as a 16-bit row ([P][N][128 lanes]: a wave's store is 128 contiguous
//            bytes).  P x N is at most 64, so the strips take at most 16 KiB, and with the palette's 32 KiB at the cap a workgroup
//            stays under 64 KiB.  A lane cannot hold N winners per pixel in registers the way remap_search holds one;
//   rank     the threshold picks place r of the ordered candidates.  pattern_select finds it in as many rounds over the strip as r has
//            distinct keys below it; a row's colour (for the luma) is gathered from the LDS palette.  A pixel whose strength is 0, or
//            whose first candidate is exact (e = 0), has N equal candidates and skips the rounds; a wave of such pixels stops after the
//            first search;
//   sums     per class through LDS atomics, the totals through a wave reduction; one global atomic per workgroup, row and column.
// (y, x) comes from the linear pixel index (one 64-bit division per pixel): the kernel needs no image-row structure.  b, the remap's
// index, is c_0: the first target is the pixel itself.
#include "palette_pattern.h"

namespace rhccq {

template <int kSize, typename IdxT>
__global__ __launch_bounds__(kPatternBlock) void palette_pattern_kernel(const uint8_t* __restrict__ rgb, long long n_px, int W,
                                                                        const uint8_t* __restrict__ pal, int K, const uint8_t* __restrict__ cls,
                                                                        int n_classes, PatternStrength strength, IdxT* __restrict__ idx_out,
                                                                        unsigned long long* __restrict__ sums) {
  extern __shared__ uint4 s_dyn[];                                                     // (16-byte aligned: the palette comes first; no static LDS beside it)
  pattern_body<kSize, IdxT>(rgb, n_px, W, pal, K, cls, n_classes, strength, idx_out, sums, blockIdx.x, gridDim.x, s_dyn);
}

template <typename IdxT>
static void pattern_host(const uint8_t* rgb, int H, int W, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, const uint32_t* strength,
                         int size, IdxT* idx, uint64_t* sums) {
  const std::vector<RemapEntry> ent = remap_pack_palette(pal, K);
  const int N = size * size;
  uint32_t cand[kPatternMaxCand];
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) {
      const long long p = (long long)y * W + x;
      const uint32_t px = remap_pack_px(rgb + p * 3), k = runs_class(cls, p, n_classes);
      PatternErr e{0, 0, 0};
      for (int i = 0; i < N; ++i) {
        uint32_t key;
        cand[i] = remap_search_host(pattern_target(px, strength[k], e), ent, &key);
        e = pattern_error(e, px, remap_pack_px(pal + (long long)cand[i] * 3));
      }
      const uint32_t out = pattern_select(N, pattern_threshold(y, x, size), [&](int j) { return cand[j]; },
                                          [&](uint32_t row) { return remap_pack_px(pal + (long long)row * 3); });
      idx[p] = (IdxT)out;
      rows_add_host(sums, k, n_classes, {1, runs_dist(px, remap_pack_px(pal + (long long)out * 3)), out != cand[0] ? 1u : 0u});
    }
  }
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_pattern_max_rows(void) { return kPatternMaxRows; }

int rhccq_palette_pattern(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                          int32_t n_classes, const uint32_t* strength_host, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = pattern_check(ctx, "palette_pattern", rgb, H, W, palette, K, cls, n_classes, strength_host, size, idx_out, idx_elem_bytes, sums))
    return rc;
  if (K > kPatternMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_pattern: the device form holds at most 4096 colours");
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)(n_classes + 1) * 3 * sizeof(uint64_t), ctx->stream));
  const int64_t n = (int64_t)H * W;
  if (n == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  PatternStrength strength{};
  for (int i = 0; i <= n_classes; ++i) strength.v[i] = strength_host[i];
  const long long chunks = (n + pattern_chunk(size) - 1) / pattern_chunk(size), cap = (long long)ctx->compute_units * 16;
  const dim3 grid((unsigned)(chunks < cap ? chunks : cap)), block(kPatternBlock);
  const size_t lds = pattern_lds_bytes(K);
  unsigned long long* s = (unsigned long long*)sums;
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
#define RHCCQ_PATTERN_CASE(N_) \
  case N_: hipLaunchKernelGGL((palette_pattern_kernel<N_, T>), grid, block, lds, ctx->stream, rgb, (long long)n, (int)W, palette, (int)K, cls, \
                              (int)n_classes, strength, (T*)idx_out, s); break;
    switch (size) {
      RHCCQ_PATTERN_CASE(2) RHCCQ_PATTERN_CASE(4)
      default: hipLaunchKernelGGL((palette_pattern_kernel<8, T>), grid, block, lds, ctx->stream, rgb, (long long)n, (int)W, palette, (int)K, cls,
                                  (int)n_classes, strength, (T*)idx_out, s);
    }
#undef RHCCQ_PATTERN_CASE
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_pattern_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                               const uint32_t* strength, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = pattern_check(nullptr, "palette_pattern", rgb, H, W, palette, K, cls, n_classes, strength, size, idx_out, idx_elem_bytes, sums))
    return rc;
  for (int i = 0; i < (n_classes + 1) * 3; ++i) sums[i] = 0;
  index_dispatch(idx_elem_bytes, [&](auto* t) { pattern_host(rgb, H, W, palette, K, cls, n_classes, strength, size, (decltype(t))idx_out, sums); });
  return 0;
}

}  // extern "C"
