// The functions of the palette refinement (palette_refine.hip) that its kernels share with the batched form (palette_batch.hip): the
// bodies of the assignment (what it does with the winners of remap_search, palette_remap.h) and of the update, the accumulator add and
// the argument check.  The rule is in include/rhccq.h; the device form is described in palette_refine.hip.
#pragma once
#include "palette_remap.h"

namespace rhccq {

// rows whose accumulators live in LDS: 32 bytes a row, 32 KiB at the limit (beside the 8 KiB tile: three workgroups in a CU's
// 160 KiB; a 256-row palette needs 8 KiB and leaves eight).  One tile, so the LDS form never restages the palette.
constexpr int kRefineLdsRows = kRemapTile;
constexpr int kRefineMaxIter = 64;
static_assert(kRefineLdsRows >= kRemapTile && kRefineLdsRows * 32 + kRemapTile * 8 + 1024 <= 64 * 1024, "accumulators + tile within 64 KiB");
// a wave's sum of one pixel column: 64 lanes x 255 x 255 < 2^32, so the wave-uniform path reduces in 32 bits
static_assert(64ull * 255 * 255 < (1ull << 32), "wave sums fit 32 bits");

struct RefineWeights { uint32_t w[kRemapMaxClasses + 1]; };

// one pixel's (or one wave's) contribution to an accumulator row, in LDS or in global memory
__device__ __forceinline__ void refine_add(unsigned long long* row, uint32_t n, uint32_t r, uint32_t g, uint32_t b) {
  atomicAdd(row + 0, (unsigned long long)n);
  atomicAdd(row + 1, (unsigned long long)r);
  atomicAdd(row + 2, (unsigned long long)g);
  atomicAdd(row + 3, (unsigned long long)b);
}

// the assignment of workgroup `bid` of the `nblk` that share the image (the launch's own for one image, those of a grid row for a
// batch); s_acc: the workgroup's accumulators in dynamic LDS, [K][4], read only when kLds
template <bool kLds>
__device__ __forceinline__ void refine_assign_body(const uint8_t* __restrict__ rgb, long long n_px,
                                                    const uint8_t* __restrict__ pal, int K,
                                                    const uint8_t* __restrict__ cls, int n_classes, RefineWeights wt,
                                                    int iter, unsigned long long* __restrict__ history,
                                                    unsigned long long* __restrict__ acc, unsigned long long* s_acc,
                                                    long long bid, long long nblk) {
  if (iter > 0 && history[(iter - 1) * 2 + 1] == 0ull) return;                          // the iteration before changed no row (or did not run)
  __shared__ unsigned long long s_err[kRemapBlock / 64];
  __shared__ uint32_t s_w[kRemapMaxClasses + 1];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if ((int)threadIdx.x <= n_classes) s_w[threadIdx.x] = wt.w[threadIdx.x];
  if (kLds)
    for (int j = threadIdx.x; j < K * 4; j += kRemapBlock) s_acc[j] = 0ull;
  unsigned long long err = 0ull;
  __syncthreads();

  remap_search(rgb, n_px, pal, K, bid, nblk, [&](long long base, auto& px, auto& bkey, auto& bidx) {
#pragma unroll
    for (int q = 0; q < kRemapPx; ++q) {
      const long long p = base + (long long)q * kRemapBlock;
      uint32_t w = 0u;
      if (p < n_px) {
        const int c = n_classes > 0 ? (int)cls[p] : n_classes;
        w = s_w[c < n_classes ? c : n_classes];
      }
      err += (unsigned long long)w * remap_dist(px[q], bkey[q]);                       // (w = 0 outside the picture)
      const uint32_t wr = w * (px[q] >> 16), wg = w * ((px[q] >> 8) & 255u), wb = w * (px[q] & 255u);
      unsigned long long* tab = kLds ? s_acc : acc;
      // neighbouring lanes hold neighbouring pixels: in flat areas the whole wave has one winner, and one lane adds the wave's sums
      const uint32_t first = __builtin_amdgcn_readfirstlane(bidx[q]);
      if (__ballot(bidx[q] == first) == ~0ull) {
        const uint32_t sn = wave_sum(w), sr = wave_sum(wr), sg = wave_sum(wg), sb = wave_sum(wb);
        if (lane == 0 && sn) refine_add(tab + (size_t)first * 4, sn, sr, sg, sb);
      } else if (w) {
        refine_add(tab + (size_t)bidx[q] * 4, w, wr, wg, wb);
      }
    }
  });
  err = wave_sum(err);
  if (lane == 0) s_err[wv] = err;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0ull;
    for (int i = 0; i < kRemapBlock / 64; ++i) t += s_err[i];
    if (t) atomicAdd(&history[iter * 2], t);
  }
  if (kLds)
    for (int j = threadIdx.x; j < K * 4; j += kRemapBlock) {
      const unsigned long long v = s_acc[j];
      if (v) atomicAdd(&acc[j], v);
    }
}

// the update of the rows bid * 256 .. of one image
__device__ __forceinline__ void refine_update_body(uint8_t* __restrict__ pal, int K, int iter, unsigned long long* __restrict__ history,
                                                  unsigned long long* __restrict__ acc, int32_t* __restrict__ n_iter, int bid) {
  if (iter > 0 && history[(iter - 1) * 2 + 1] == 0ull) return;
  __shared__ int s_red[256 / 64];
  const int j = bid * 256 + threadIdx.x;
  int changed = 0;
  if (j < K) {
    const unsigned long long n = acc[j * 4];
    if (n) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const uint8_t v = (uint8_t)refine_mean(acc[j * 4 + 1 + ch], n);
        changed |= v != pal[j * 3 + ch];
        pal[j * 3 + ch] = v;
        acc[j * 4 + 1 + ch] = 0ull;
      }
      acc[j * 4] = 0ull;
    }
  }
  const int total = block_sum(changed, s_red);
  if (threadIdx.x == 0) {
    if (total) atomicAdd(&history[iter * 2 + 1], (unsigned long long)total);
    if (bid == 0) *n_iter = iter + 1;
  }
}

static inline int refine_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                        const int32_t* weights, int32_t max_iter, const void* history, const void* n_iter, RefineWeights* wt) {
  if (const int rc = search_check(ctx, "palette_refine", !rgb || !palette || !history || !n_iter, n_pixels, K, cls, n_classes)) return rc;
  if (max_iter < 1 || max_iter > kRefineMaxIter) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine: max_iter must be 1..64");
  uint32_t top;
  if (const int rc = weights_check(ctx, "palette_refine", weights, n_classes, wt->w, &top)) return rc;
  if (((uintptr_t)history & 7) || ((uintptr_t)n_iter & 3)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine: misaligned history or n_iter");
  return search_limit(ctx, "palette_refine", K);
}

}  // namespace rhccq
