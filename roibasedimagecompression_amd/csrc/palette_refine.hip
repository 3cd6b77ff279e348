// Refinement of a given palette on the device (EXTENSION, no reference counterpart): pixel-weighted Lloyd iterations in exact integers.
// One iteration: (1) every pixel goes to its nearest row by the remap's rule (palette_remap.h: exact integers, ties to the lowest row),
// (2) per row j the sums N_j = sum w(p), S_j = sum w(p) p per channel, and E = sum w(p) |p - c_a(p)|^2 over the picture, all 64-bit,
// (3) a row with N_j > 0 becomes floor((2 S_j + N_j) / (2 N_j)) per channel, the weighted mean rounded to nearest with halves up; a row
// with N_j == 0 stays.  history[i] = {E, rows whose bytes changed}.  The refinement stops after the first iteration that changes no row.
//
// Rounding to nearest (not K2's floor mean) is what makes E non-increasing: over the integers sum w (x - c)^2 is smallest at the integer
// nearest to the weighted mean, so the update cannot raise a row's error against its own pixels, and the next assignment cannot raise
// any pixel's error.  (A floor mean can: pixels 10 and 11 give 10.5, floor 10 and nearest 11 tie here, but 10, 11, 11 give 10.67,
// floor 10 with error 2 against 11 with error 1.)
//
// Device form: two launches per iteration, max_iter iterations queued on the stream, no host synchronisation.
//   assign      remap_search (palette_remap.h: 256 lanes x 8 pixels, palette tiles through LDS); after each chunk it adds
//               (w, w r, w g, w b) to the winner's accumulator row and w * dist to a per-lane 64-bit sum.  It stores no index.
//   update      one thread per row: new row, changed rows counted into history[i][1], accumulators cleared for the next iteration.
// An iteration i > 0 runs iff history[i - 1][1] != 0: both kernels read that word first and return at once otherwise (the call zeroes
// the history, so an iteration that did not run leaves 0 there and stops the ones behind it too).  Stream order between launches is
// the only synchronisation: no kernel waits for another workgroup.
// Accumulators are uint64[K][4] in the workspace.  For K <= kRefineLdsRows a workgroup keeps a copy of its own in (dynamic) LDS and
// flushes it with one 64-bit atomicAdd per non-zero field after its chunk loop; larger palettes add to the workspace directly.
// Integer addition: both forms give the same sums in any order.  Every field is 64-bit wherever it lives: a field grows by at most
// 255 * 255 a pixel, so it cannot overflow below 2^64 / 65025 > 2^48 pixels (n_pixels is an int64 count of addressable bytes / 3).
#include "palette_refine.h"

#include <algorithm>

namespace rhccq {

// (the bodies, refine_assign_body and refine_update_body, are in palette_refine.h)
template <bool kLds>
__global__ __launch_bounds__(kRemapBlock) void palette_refine_assign_kernel(const uint8_t* __restrict__ rgb, long long n_px,
                                                                            const uint8_t* __restrict__ pal, int K,
                                                                            const uint8_t* __restrict__ cls, int n_classes, RefineWeights wt,
                                                                            int iter, unsigned long long* __restrict__ history,
                                                                            unsigned long long* __restrict__ acc) {
  extern __shared__ unsigned long long s_acc[];                                         // kLds: [K][4]
  refine_assign_body<kLds>(rgb, n_px, pal, K, cls, n_classes, wt, iter, history, acc, s_acc, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void palette_refine_update_kernel(uint8_t* __restrict__ pal, int K, int iter, unsigned long long* __restrict__ history,
                                                                    unsigned long long* __restrict__ acc, int32_t* __restrict__ n_iter) {
  refine_update_body(pal, K, iter, history, acc, n_iter, blockIdx.x);
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_refine_lds_rows(void) { return kRefineLdsRows; }

int64_t rhccq_palette_refine_bytes(int32_t K) { return K < 1 ? 0 : (int64_t)K * 4 * (int64_t)sizeof(uint64_t); }

int rhccq_palette_refine(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                         const int32_t* weights_host, int32_t max_iter, void* work, int64_t work_bytes, uint64_t* history, int32_t* n_iter) {
  if (!ctx) return RHCCQ_E_ARG;
  RefineWeights wt = {};
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine: null argument");
  if (const int rc = refine_check(ctx, rgb, n_pixels, palette, K, cls, n_classes, weights_host, max_iter, history, n_iter, &wt)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine: misaligned workspace");
  if (work_bytes < rhccq_palette_refine_bytes(K)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine: the workspace is smaller than rhccq_palette_refine_bytes(K)");
  RHCCQ_HIP(ctx, hipMemsetAsync(history, 0, (size_t)max_iter * 2 * sizeof(uint64_t), ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(n_iter, 0, sizeof(int32_t), ctx->stream));
  if (n_pixels == 0) return 0;
  RHCCQ_HIP(ctx, hipMemsetAsync(work, 0, (size_t)rhccq_palette_refine_bytes(K), ctx->stream));
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const long long cap = ctx->opt_refine_max_blocks > 0 ? ctx->opt_refine_max_blocks : (long long)ctx->compute_units * 8;
  const dim3 grid(remap_blocks(n_pixels, cap)), block(kRemapBlock), ugrid((unsigned)((K + 255) / 256));
  const int lds_rows = ctx->opt_refine_lds_rows < 0 ? kRefineLdsRows : ctx->opt_refine_lds_rows;
  const bool lds = K <= lds_rows;
  unsigned long long* acc = (unsigned long long*)work;
  unsigned long long* hist = (unsigned long long*)history;
  for (int it = 0; it < max_iter; ++it) {
    if (lds)
      hipLaunchKernelGGL(palette_refine_assign_kernel<true>, grid, block, (size_t)K * 4 * sizeof(uint64_t), ctx->stream, rgb, (long long)n_pixels,
                         (const uint8_t*)palette, (int)K, cls, (int)n_classes, wt, it, hist, acc);
    else
      hipLaunchKernelGGL(palette_refine_assign_kernel<false>, grid, block, 0, ctx->stream, rgb, (long long)n_pixels, (const uint8_t*)palette, (int)K,
                         cls, (int)n_classes, wt, it, hist, acc);
    hipLaunchKernelGGL(palette_refine_update_kernel, ugrid, dim3(256), 0, ctx->stream, palette, (int)K, it, hist, acc, n_iter);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_refine_host(const uint8_t* rgb, int64_t n_pixels, uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                              const int32_t* weights, int32_t max_iter, uint64_t* history, int32_t* n_iter) {
  RefineWeights wt = {};
  if (const int rc = refine_check(nullptr, rgb, n_pixels, palette, K, cls, n_classes, weights, max_iter, history, n_iter, &wt)) return rc;
  for (int i = 0; i < max_iter * 2; ++i) history[i] = 0;
  *n_iter = 0;
  if (n_pixels == 0) return 0;
  std::vector<uint64_t> acc((size_t)K * 4);
  for (int it = 0; it < max_iter; ++it) {
    const std::vector<RemapEntry> ent = remap_pack_palette(palette, K);
    std::fill(acc.begin(), acc.end(), 0);
    uint64_t err = 0;
    for (int64_t p = 0; p < n_pixels; ++p) {
      const uint32_t px = remap_pack_px(rgb + p * 3);
      uint32_t key;
      const uint32_t idx = remap_search_host(px, ent, &key);
      const uint64_t w = wt.w[n_classes > 0 && cls[p] < n_classes ? cls[p] : n_classes];
      err += w * remap_dist(px, key);
      acc[idx * 4] += w;
      for (int ch = 0; ch < 3; ++ch) acc[idx * 4 + 1 + ch] += w * rgb[p * 3 + ch];
    }
    uint64_t changed = 0;
    for (int j = 0; j < K; ++j) {
      if (!acc[(size_t)j * 4]) continue;
      bool diff = false;
      for (int ch = 0; ch < 3; ++ch) {
        const uint8_t v = (uint8_t)refine_mean(acc[(size_t)j * 4 + 1 + ch], acc[(size_t)j * 4]);
        diff |= v != palette[j * 3 + ch];
        palette[j * 3 + ch] = v;
      }
      changed += diff;
    }
    history[it * 2] = err;
    history[it * 2 + 1] = changed;
    *n_iter = it + 1;
    if (!changed) break;
  }
  return 0;
}

}  // extern "C"
