// Error-diffusing remap onto a given palette (EXTENSION, no reference counterpart): Floyd-Steinberg in exact integers, raster order, no
// serpentine.  With E the error a pixel passes on and s its class's strength (0..256), per channel
//     A = 7 E(y, x-1) + E(y-1, x-1) + 5 E(y-1, x) + 3 E(y-1, x+1)          (terms outside the picture are 0)
//     t = clamp(p + floor((s A + 2048) / 4096), 0, 255);   out = the remap's nearest row of t (ties to the lowest);   E = t - palette[out]
// The step functions are in palette_dither.h; the host form runs them serially.
//
// The kernel.  Pixel (y, x) depends on (y, x-1) and on (y-1, x-1 .. x+1), so it can run at step x + 2 y: a wavefront skewed by two columns
// a row.  A workgroup is ONE wave and owns a band of R consecutive image rows (4, 8, 16 or 32); G = 64 / R lanes share an image row, and
// at step u (counted from 0) the row group r stands at column u - 1 - 2 r.  The step before a row's first column fetches E(y-1, 0).
//   search  the palette is staged once in LDS as RemapEntry under its row number (K <= 4096: 12 bits), padded with entries that never
//           win.  The G lanes of a pixel compute the same target and take every G-th pair of entries (one 16-byte read; the G addresses of a
//           read are consecutive, every other lane gets a broadcast; four reads are in flight ahead of their use, the first four behind
//           the target's arithmetic); their minima of (key << 12 | row) meet in a DPP butterfly inside the DPP row of 16 lanes (quad_perm, row_half_mirror, row_mirror).  The minimum of that word is the lowest row of the smallest
//           key: the remap's tie rule.  The winner's colour is read back from its LDS entry;
//   errors  a lane keeps its left error and the three errors above it unpacked.  Every step it takes ONE packed word from the row group
//           above (ds_bpermute by G lanes): the error that group computed a step ago, which is (y-1, x+1), or 0 when that group was
//           outside the picture; up and up-left are the words of the two steps before;
//   pixels  go through LDS in tiles of 64 steps, skewed like the wavefront (row q of tile T holds columns 64 T - 1 - 2 q ...): all 64 lanes
//           load a row segment per image row (coalesced, clamped at the edges, not branched around), the loads of tile T + 1 are issued
//           before the walk of tile T.  A step's pixel word is read one step ahead of its use;
//   finish  all 64 lanes, a row segment at a time, from LDS: the index is written where it differs from b (rhccq_palette_remap's, which
//           the call has put there), and the squared error against the ORIGINAL pixel and the moved flag go to the sums.
// Between bands.  Row 0 of band n needs the errors of the last row of band n - 1: the hand-over of band_handoff.h, which also holds the
// forward-progress argument (a band that gives up sets *status).  A word is an error and the mark; the last row's words leave a granule
// of 4 per store instruction, and band n fetches a granule of 4 at a time.
#include "palette_dither.h"
#include "wave_dpp.h"

namespace rhccq {

// palette entries in LDS: padded to 128, so that every lane's slice is a multiple of four pairs for any G <= 16
__host__ __device__ __forceinline__ int dither_padded(int K) { return (K + 127) & ~127; }
static size_t dither_lds_bytes(int rows, int K) { return (size_t)dither_padded(K) * 8 + (size_t)3 * rows * kDitherPitch * 4; }

__device__ __forceinline__ uint32_t dither_index_load(const void* idx, int eb, long long p) {
  return eb == 1 ? (uint32_t)((const uint8_t*)idx)[p] : eb == 2 ? (uint32_t)((const uint16_t*)idx)[p] : ((const uint32_t*)idx)[p];
}

// a lane's column of a tile on its way from global memory to LDS, kept exactly as loaded (see palette_runs.hip)
template <int R>
struct DitherTile {
  uint16_t rg[R];
  uint8_t bl[R], k[R];
  uint32_t b[R];
};

// loads only: image rows past the band's last and columns outside the picture repeat the nearest one inside
template <int R>
__device__ __forceinline__ void dither_load(DitherTile<R>& t, const uint8_t* __restrict__ rgb, const void* idx, int eb, const uint8_t* __restrict__ cls,
                                            long long row0, int nrows, int W, long long u0, int lane) {
#pragma unroll
  for (int q = 0; q < R; ++q) {
    const long long x = min(max(u0 + lane - 1 - 2 * q, 0ll), (long long)W - 1);
    const long long p = (row0 + min(q, nrows - 1)) * W + x;
    __builtin_memcpy(&t.rg[q], rgb + p * 3, 2);
    t.bl[q] = rgb[p * 3 + 2];
    t.b[q] = dither_index_load(idx, eb, p);
    t.k[q] = cls ? cls[p] : (uint8_t)255;
  }
}

template <int R>
__global__ __launch_bounds__(kDitherLanes) void palette_dither_kernel(const uint8_t* __restrict__ rgb, int H, int W, const uint8_t* __restrict__ pal, int K,
                                                                      const uint8_t* __restrict__ cls, int n_classes, DitherStrength strength,
                                                                      void* idx, int eb, uint32_t* work, unsigned long long* __restrict__ sums,
                                                                      int* status) {
  constexpr int G = kDitherLanes / R;
  extern __shared__ uint4 s_dyn[];                                                     // (16-byte aligned: the palette comes first)
  __shared__ unsigned long long s_cls[kRemapMaxClasses][3];
  __shared__ uint32_t s_str[kRemapMaxClasses + 1];
  __shared__ uint32_t s_band;
  __shared__ uint32_t s_hand[kDitherGranule];                                          // the last row's words of the granule being filled
  const int lane = threadIdx.x, r = lane / G, g = lane % G;
  const int K2 = dither_padded(K), trips = K2 / 2 / G;                                 // pairs of entries a lane evaluates a step: a multiple of 4
  RemapEntry* s_pal = reinterpret_cast<RemapEntry*>(s_dyn);                            // [K2]
  uint32_t* s_px = reinterpret_cast<uint32_t*>(s_pal + K2);                            // [R][65] each: the pixel | its class row << 24,
  uint32_t* s_b = s_px + R * kDitherPitch;                                             // b,
  uint32_t* s_out = s_b + R * kDitherPitch;                                            // the output index
  band::draw_ticket(work, &s_band, lane);
  for (int j = lane; j < K2; j += kDitherLanes) s_pal[j] = j < K ? remap_pack_entry(pal + (long long)j * 3, j) : RemapEntry{0u, 0xFFFFFFFFu};
  if (lane < kRemapMaxClasses * 3) (&s_cls[0][0])[lane] = 0ull;
  if (lane <= n_classes) s_str[lane] = strength.v[lane];
  __syncthreads();

  const int nbands = (H + R - 1) / R, band = (int)s_band;
  if (band >= nbands) return;                                                          // (the grid has exactly nbands workgroups)
  const long long y0 = (long long)band * R;
  const int nrows = (int)min((long long)R, H - y0);
  const long long nsteps = (long long)W + 2 * nrows - 1;
  const uint32_t* up_words = band::words(work, band - 1, W);                           // (band > 0 only) the last row of the band above
  uint32_t* my_words = band::words(work, band, W);
  const bool hand_on = band + 1 < nbands;

  DitherTile<R> t;
  dither_load<R>(t, rgb, idx, eb, cls, y0, nrows, W, 0ll, lane);
  DitherErr e_left{0, 0, 0}, e_ul{0, 0, 0}, e_up{0, 0, 0}, e_ur{0, 0, 0};
  uint32_t e_last = 0u;                                                                // the error of the step before, packed; 0 outside the picture
  bool waiting = band > 0;                                                             // (wave uniform) false once a band has given up
  uint32_t gran = 0u, pending = 0u;                                                    // lanes 0..3: the band above's words of this granule, of the next
  unsigned long long all_sse = 0ull, all_moved = 0ull;
  const int o_row = r * kDitherPitch;

  for (long long u0 = 0; u0 < nsteps; u0 += kDitherCols) {                             // (wave uniform throughout)
    const int ns = (int)min((long long)kDitherCols, nsteps - u0);
#pragma unroll
    for (int q = 0; q < R; ++q) {
      if (q < nrows) {
        const uint32_t rg = t.rg[q], px = (rg & 255u) << 16 | (rg >> 8) << 8 | t.bl[q];
        s_px[q * kDitherPitch + lane] = px | min((uint32_t)t.k[q], (uint32_t)n_classes) << 24;
        s_b[q * kDitherPitch + lane] = t.b[q];
      }
    }
    __syncthreads();
    if (u0 + kDitherCols < nsteps) dither_load<R>(t, rgb, idx, eb, cls, y0, nrows, W, u0 + kDitherCols, lane);   // lands behind the walk

    uint32_t w_next = s_px[o_row];
    for (int s = 0; s < ns; ++s) {
      const long long u = u0 + s;
      if (waiting && (u & (kDitherGranule - 1)) == 0)                                  // the words of columns u .. u + 3 of the row above
        band::fetch_granule<kDitherGranule>(up_words, u, W, lane, work + band::kAbortWord, (uint32_t*)status, waiting, gran, pending);
      const long long x = u - 1 - 2 * r;
      const bool active = r < nrows && x >= 0 && x < W;
      const uint32_t w = w_next;
      w_next = s_px[o_row + min(s + 1, kDitherCols - 1)];
      uint4 q[4];                                                                      // the slice's first four pairs: they land behind the target's arithmetic
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = s_dyn[g + j * G];
      const uint32_t sv = s_str[w >> 24];
      // the error above-right: from the band above for row 0, else what the row group above computed a step ago
      const uint32_t from_band = (uint32_t)__builtin_amdgcn_readlane((int)gran, (int)(u & (kDitherGranule - 1))) & ~band::kWritten;
      const uint32_t from_row = (uint32_t)__shfl_up((int)e_last, G, kDitherLanes);
      e_ul = e_up;
      e_up = e_ur;
      e_ur = dither_unpack(r == 0 ? from_band : from_row);
      const uint32_t target = dither_target(w, sv, e_left, e_ul, e_up, e_ur);
      uint32_t best = 0xFFFFFFFFu;
      for (int i = 0; i < trips; i += 4) {                                             // (the same trips in every lane)
        uint4 c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = q[j];
        if (i + 4 < trips) {                                                           // the next four land behind these evaluations
#pragma unroll
          for (int j = 0; j < 4; ++j) q[j] = s_dyn[g + (i + 4 + j) * G];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          best = min(best, remap_eval(target, RemapEntry{c[j].x, c[j].y}));
          best = min(best, remap_eval(target, RemapEntry{c[j].z, c[j].w}));
        }
      }
      best = dpp_group_min<G>(best);                                                   // (G <= 16, aligned: inside one DPP row)
      const uint32_t out = best & ((1u << kRemapIdxBits) - 1u);
      const DitherErr e = dither_error(target, dither_entry_colour(s_pal[out]));
      e_left = active ? e : DitherErr{0, 0, 0};
      e_last = active ? dither_pack(e) : 0u;
      if (active && g == 0) {
        s_out[o_row + s] = out;
        if (hand_on && r == R - 1) s_hand[x & (kDitherGranule - 1)] = e_last | band::kWritten;
      }
      // the last row's errors leave a granule at a time: one store instruction, and one wait for it, every fourth step
      const long long xl = u - 1 - 2 * (R - 1);                                        // (wave uniform) the last row's column
      if (hand_on && xl >= 0 && xl < W && ((xl & (kDitherGranule - 1)) == kDitherGranule - 1 || xl == W - 1)) {
        __syncthreads();
        if (lane <= (int)(xl & (kDitherGranule - 1)))
          band::word_store(my_words + (xl & ~(long long)(kDitherGranule - 1)) + lane, s_hand[lane]);
      }
    }
    __syncthreads();

    if (lane < ns) {
#pragma unroll 4
      for (int q = 0; q < nrows; ++q) {
        const long long x = u0 + lane - 1 - 2 * q;
        if (x >= 0 && x < W) {
          const int o = q * kDitherPitch + lane;
          const uint32_t w = s_px[o], out = s_out[o], b = s_b[o], k = w >> 24;
          const long long p = (y0 + q) * W + x;
          if (out != b) {
            if (eb == 1) ((uint8_t*)idx)[p] = (uint8_t)out;
            else if (eb == 2) ((uint16_t*)idx)[p] = (uint16_t)out;
            else ((uint32_t*)idx)[p] = out;
          }
          const uint32_t d = runs_dist(w & 0xFFFFFFu, dither_entry_colour(s_pal[out])), mv = out != b ? 1u : 0u;
          all_sse += d;
          all_moved += mv;
          if (k < (uint32_t)n_classes) {
            atomicAdd(&s_cls[k][0], 1ull);
            atomicAdd(&s_cls[k][1], (unsigned long long)d);
            if (mv) atomicAdd(&s_cls[k][2], 1ull);
          }
        }
      }
    }
    __syncthreads();                                                                   // the next tile overwrites the three arrays
  }
  all_sse = wave_sum(all_sse);
  all_moved = wave_sum(all_moved);
  if (lane == 0) {
    atomicAdd(&sums[n_classes * 3 + 0], (unsigned long long)nrows * (unsigned long long)W);
    if (all_sse) atomicAdd(&sums[n_classes * 3 + 1], all_sse);
    if (all_moved) atomicAdd(&sums[n_classes * 3 + 2], all_moved);
  }
  if (lane < n_classes * 3) {
    const unsigned long long v = (&s_cls[0][0])[lane];
    if (v) atomicAdd(&sums[lane], v);
  }
}

template <typename IdxT>
static void dither_host(const uint8_t* rgb, int H, int W, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, const uint32_t* strength,
                        IdxT* idx, uint64_t* sums) {
  const std::vector<RemapEntry> ent = remap_pack_palette(pal, K);
  std::vector<uint32_t> above((size_t)W + 2, 0u), row((size_t)W + 2, 0u);              // packed errors, column x at [x + 1]: the ends stay 0
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) {
      const long long p = (long long)y * W + x;
      const uint32_t px = remap_pack_px(rgb + p * 3), k = runs_class(cls, p, n_classes), b = (uint32_t)idx[p];
      const uint32_t target = dither_target(px, strength[k], dither_unpack(row[x]), dither_unpack(above[x]), dither_unpack(above[x + 1]),
                                            dither_unpack(above[x + 2]));
      uint32_t key;
      const uint32_t out = remap_search_host(target, ent, &key);
      const uint32_t col = remap_pack_px(pal + (long long)out * 3);
      row[x + 1] = dither_pack(dither_error(target, col));
      idx[p] = (IdxT)out;
      rows_add_host(sums, k, n_classes, {1, runs_dist(px, col), out != b ? 1u : 0u});
    }
    above.swap(row);
  }
}

template <int R>
static void dither_launch(rhccq_ctx* ctx, const uint8_t* rgb, int H, int W, const uint8_t* pal, int K, const uint8_t* cls, int n_classes,
                          const DitherStrength& strength, void* idx, int eb, uint32_t* work, uint64_t* sums, int32_t* status) {
  const dim3 grid((unsigned)dither_bands(H, R)), block(kDitherLanes);
  hipLaunchKernelGGL(palette_dither_kernel<R>, grid, block, dither_lds_bytes(R, K), ctx->stream, rgb, H, W, pal, K, cls, n_classes, strength, idx, eb,
                     work, (unsigned long long*)sums, (int*)status);
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_dither_max_rows(void) { return kDitherMaxRows; }
int32_t rhccq_palette_dither_rows(void) { return kDitherRowsDefault; }

int64_t rhccq_palette_dither_bytes(int32_t H, int32_t W) {
  if (H < 0 || W < 0) return 0;
  return dither_work_bytes(H, W, kDitherRowsMin);
}

int rhccq_palette_dither(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                         int32_t n_classes, const uint32_t* strength_host, void* work, int64_t work_bytes, void* idx_out, int32_t idx_elem_bytes,
                         uint64_t* sums, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = dither_check(ctx, rgb, H, W, palette, K, cls, n_classes, strength_host, idx_out, idx_elem_bytes, sums)) return rc;
  if (!status || ((uintptr_t)status & 3)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_dither: a status word, aligned to 4, is required");
  if (K > kDitherMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_dither: the device form holds at most 4096 colours");
  const size_t sums_bytes = (size_t)(n_classes + 1) * 3 * sizeof(uint64_t);
  const int64_t n = (int64_t)H * W;
  if (n == 0) {
    RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
    RHCCQ_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int32_t), ctx->stream));
    return 0;
  }
  if (!work || ((uintptr_t)work & 3) || work_bytes < rhccq_palette_dither_bytes(H, W))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_dither: a workspace of rhccq_palette_dither_bytes(H, W) bytes, aligned to 4, is required");
  // b into idx_out; the remap's own {pixels, SSE} land in the first two words of sums, which the memset behind it clears again
  if (const int rc = rhccq_palette_remap(ctx, rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, sums)) return rc;
  const int rows = ctx->opt_dither_rows > 0 ? ctx->opt_dither_rows : kDitherRowsDefault;
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(status, 0, sizeof(int32_t), ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(work, 0, (size_t)dither_work_bytes(H, W, rows), ctx->stream));   // the ticket, the abort word, every hand-over word
  DitherStrength strength{};
  for (int i = 0; i <= n_classes; ++i) strength.v[i] = strength_host[i];
#define RHCCQ_DITHER_CASE(R_) \
  case R_: dither_launch<R_>(ctx, rgb, H, W, palette, K, cls, n_classes, strength, idx_out, idx_elem_bytes, (uint32_t*)work, sums, status); break;
  switch (rows) {
    RHCCQ_DITHER_CASE(8) RHCCQ_DITHER_CASE(16) RHCCQ_DITHER_CASE(32)
    default: dither_launch<4>(ctx, rgb, H, W, palette, K, cls, n_classes, strength, idx_out, idx_elem_bytes, (uint32_t*)work, sums, status);
  }
#undef RHCCQ_DITHER_CASE
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_dither_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                              const uint32_t* strength, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = dither_check(nullptr, rgb, H, W, palette, K, cls, n_classes, strength, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i < (n_classes + 1) * 3; ++i) sums[i] = 0;
  const int64_t n = (int64_t)H * W;
  if (n == 0) return 0;
  uint64_t remap_sums[2];
  if (const int rc = rhccq_palette_remap_host(rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, remap_sums)) return rc;
  index_dispatch(idx_elem_bytes, [&](auto* t) { dither_host(rgb, H, W, palette, K, cls, n_classes, strength, (decltype(t))idx_out, sums); });
  return 0;
}

}  // extern "C"
