// Run-carrying remap onto a given palette (EXTENSION, no reference counterpart).  b(y, x) is rhccq_palette_remap's index of the pixel;
// along every image row a pixel keeps its left neighbour's output row while that costs at most `slack` more squared error than b:
//     out(y, 0) = b(y, 0);    c = out(y, x - 1):  out(y, x) = c  if |p - palette[c]|^2 <= |p - palette[b]|^2 + slack(p),  else b(y, x)
// in exact integers, slack(p) = slack[cls[p]] (the last entry for a class value >= n_classes and without a class map).  The index map
// becomes repetitive along rows, which is what the container's zlib stage rewards; image rows are independent by definition.
// The step / limit / distance functions are in palette_runs.h; the host form runs the same functions serially.
//
// The kernel.  The remap has already written b.  A workgroup is ONE wave and owns `rows` consecutive image rows (2, 4 or 8); lane r walks
// row r.  A row-major image puts the lanes of such a walk 3 W bytes apart, so the picture goes through LDS in tiles of rows x 64 columns:
//   load    all 64 lanes load one row segment of 64 pixels per image row (coalesced: 192 bytes of rgb, 64 indices, 64 classes) into
//           registers.  Rows and columns past the edge are clamped, not branched around, so that every load of the tile is in flight
//           before the first wait; the loads of tile t + 1 are issued before the walk of tile t and land behind it;
//   stage   from the registers: gather palette[b] (from a copy of the palette in LDS while K <= 4096, from global memory above: a large
//           palette does not fit beside the tile) and store per pixel four words: the pixel | its class row << 24, palette[b], the limit
//           w(p, palette[b]) - slack, and b;
//   walk    lane r reads its row's words eight columns ahead of the chain (they do not depend on it) and runs the step: one dot product
//           (beside an add and a shift), one compare and three selects are loop-carried; the carried row's colour, |colour|^2 and index stay in
//           registers from tile to tile.  The output index replaces the limit in LDS;
//   finish  all 64 lanes again, a row segment at a time, from LDS alone: the output index is written to global memory where it differs
//           from b, and the pixel's squared error and carried flag go to the sums.
// LDS banks: a tile row is 65 words long.  In the walk lane r reads word r * 65 + x: with ds_read_b32 (32 banks, the two 32-lane halves
// conflict among themselves only) at most 8 lanes at an odd pitch fall on 8 different banks.  Stage and finish use consecutive words.
// Why so few rows a wave: the chain is latency, not throughput.  A wave issues the same walk for 2 lanes as for 64, the device has 1024
// SIMDs, and 2160 image rows in waves of 64 would keep 34 of them busy; small workgroups spread the rows over the device.
// Sums: every lane adds its pixels of class c to its own slot (c, lane) in LDS, so there are no atomics inside the workgroup; 3 (n_classes + 1)
// global atomics per workgroup at the end.
#include "palette_runs.h"

namespace rhccq {

static size_t runs_lds_bytes(int rows, int K, int n_classes) {
  return (size_t)4 * rows * kRunsPitch * 4 + (K <= kRunsLdsPalette ? (size_t)K * 4 : 0) + (size_t)n_classes * kRunsLanes * 16;
}

// a lane's column of a tile on its way from global memory to LDS: red and green (one 16-bit load), blue, b and the class of up to
// kRunsRowsMax image rows, kept exactly as loaded: any arithmetic on them here would make the walk wait for the loads
struct RunsTile {
  uint16_t rg[kRunsRowsMax];
  uint8_t bl[kRunsRowsMax];
  uint32_t b[kRunsRowsMax], k[kRunsRowsMax];
};

// loads only, no use of a loaded value: image rows past the workgroup's last and columns past the picture's last repeat the last one
template <typename IdxT>
__device__ __forceinline__ void runs_load(RunsTile& t, const uint8_t* __restrict__ rgb, const IdxT* idx, const uint8_t* __restrict__ cls,
                                          int n_classes, long long row0, int nrows, int W, long long x0, int lane) {
  const long long x = min(x0 + lane, (long long)W - 1);
#pragma unroll
  for (int q = 0; q < kRunsRowsMax; ++q) {
    const long long p = (row0 + min(q, nrows - 1)) * W + x;
    __builtin_memcpy(&t.rg[q], rgb + p * 3, 2);                                      // (any alignment: a global 16-bit load takes it)
    t.bl[q] = rgb[p * 3 + 2];
    t.b[q] = (uint32_t)idx[p];
    t.k[q] = (uint32_t)n_classes;
  }
  if (cls) {
#pragma unroll
    for (int q = 0; q < kRunsRowsMax; ++q) t.k[q] = cls[(row0 + min(q, nrows - 1)) * W + x];
  }
}

// a lane's walk along its row of the tile: the words of eight columns are read ahead of the chain, which does not feed them.  A full tile
// (every tile of a picture but its last) runs without the per-column test
template <bool kFull>
__device__ __forceinline__ void runs_walk(RunsState& st, const uint32_t* a, const uint32_t* bb, uint32_t* c, const uint32_t* d, int tw) {
  for (int x = 0; x < (kFull ? kRunsCols : tw); x += 8) {                             // x + q <= 63: inside the row's 64 words
    uint32_t w0[8], w1[8], w2[8], w3[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { w0[q] = a[x + q]; w1[q] = bb[x + q]; w2[q] = c[x + q]; w3[q] = d[x + q]; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (kFull || x + q < tw) runs_step(st, w0[q], (int32_t)w2[q], w3[q], w1[q]);
      w2[q] = st.idx;
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (kFull || x + q < tw) c[x + q] = w2[q];
  }
}

template <typename IdxT>
__global__ __launch_bounds__(kRunsLanes) void palette_runs_kernel(const uint8_t* __restrict__ rgb, int H, int W, const uint8_t* __restrict__ pal,
                                                                  int K, const uint8_t* __restrict__ cls, int n_classes, RunsSlack slack, int rows,
                                                                  IdxT* idx, unsigned long long* __restrict__ sums) {
  extern __shared__ unsigned long long s_dyn[];                                       // (8-byte aligned: the class slots come first)
  __shared__ uint32_t s_slack[kRemapMaxClasses + 1];
  __shared__ unsigned long long s_tot[2];
  const int lane = threadIdx.x;
  unsigned long long* s_sse = s_dyn;                                                   // [n_classes][64]
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_sse + n_classes * kRunsLanes);     // [n_classes][64] pixels, then [n_classes][64] carried
  uint32_t* s_a = s_cnt + 2 * n_classes * kRunsLanes;                                // [rows][65] each: the pixel | class row << 24,
  uint32_t* s_b = s_a + rows * kRunsPitch;                                           // palette[b],
  uint32_t* s_c = s_b + rows * kRunsPitch;                                           // the limit, then the output index,
  uint32_t* s_d = s_c + rows * kRunsPitch;                                           // b
  uint32_t* s_pal = s_d + rows * kRunsPitch;                                          // [K] while K <= kRunsLdsPalette
  const bool lds_pal = K <= kRunsLdsPalette;
  const int y0 = blockIdx.x * rows, nrows = min(rows, H - y0);
  RunsTile t;
  runs_load(t, rgb, idx, cls, n_classes, (long long)y0, nrows, W, 0ll, lane);         // the first tile, behind the set-up below
  if (lds_pal)
    for (int j = lane; j < K; j += kRunsLanes) s_pal[j] = remap_pack_px(pal + (long long)j * 3);
  for (int i = lane; i < n_classes * kRunsLanes; i += kRunsLanes) { s_sse[i] = 0ull; s_cnt[i] = 0u; s_cnt[n_classes * kRunsLanes + i] = 0u; }
  if (lane <= n_classes) s_slack[lane] = slack.v[lane];
  __syncthreads();

  RunsState st{0u, 0u, 0u};
  unsigned long long all_sse = 0ull, all_car = 0ull;
  for (long long x0 = 0; x0 < W; x0 += kRunsCols) {                                   // (block uniform: the barriers below are safe)
    const int tw = (int)min((long long)kRunsCols, W - x0);
    if (lane < tw) {
#pragma unroll
      for (int q = 0; q < kRunsRowsMax; ++q) {
        if (q < nrows) {
          const uint32_t rg = t.rg[q], px = (rg & 255u) << 16 | (rg >> 8) << 8 | t.bl[q], b = t.b[q], k = min(t.k[q], (uint32_t)n_classes);
          const uint32_t pb = lds_pal ? s_pal[b] : remap_pack_px(pal + (long long)b * 3);
          const int o = q * kRunsPitch + lane;
          s_a[o] = px | k << 24;
          s_b[o] = pb;
          s_c[o] = (uint32_t)runs_limit(px, pb, s_slack[k], x0 + lane == 0);
          s_d[o] = b;
        }
      }
    }
    __syncthreads();
    if (x0 + kRunsCols < W) runs_load(t, rgb, idx, cls, n_classes, (long long)y0, nrows, W, x0 + kRunsCols, lane);   // lands behind the walk
    if (lane < nrows) {
      const int o = lane * kRunsPitch;
      if (tw == kRunsCols) runs_walk<true>(st, s_a + o, s_b + o, s_c + o, s_d + o, tw);
      else runs_walk<false>(st, s_a + o, s_b + o, s_c + o, s_d + o, tw);
    }
    __syncthreads();
    if (lane < tw) {
#pragma unroll 4
      for (int r = 0; r < nrows; ++r) {
        const int o = r * kRunsPitch + lane;
        const uint32_t w0 = s_a[o], out = s_c[o], b = s_d[o];
        const uint32_t px = w0 & 0xFFFFFFu, k = w0 >> 24;
        uint32_t col = s_b[o];
        if (out != b) {
          col = lds_pal ? s_pal[out] : remap_pack_px(pal + (long long)out * 3);
          idx[(long long)(y0 + r) * W + x0 + lane] = (IdxT)out;
        }
        const uint32_t d = runs_dist(px, col), car = out != b ? 1u : 0u;
        all_sse += d;
        all_car += car;
        if (k < (uint32_t)n_classes) {                                                 // this lane's own slot: no other writer
          const int s = (int)k * kRunsLanes + lane;
          s_sse[s] += d;
          s_cnt[s] += 1u;
          s_cnt[n_classes * kRunsLanes + s] += car;
        }
      }
    }
    __syncthreads();                                                                   // the next tile overwrites the four arrays
  }
  all_sse = wave_sum(all_sse);
  all_car = wave_sum(all_car);
  if (lane == 0) { s_tot[0] = all_sse; s_tot[1] = all_car; }
  __syncthreads();
  if (lane < (n_classes + 1) * 3) {                                                    // one atomic per workgroup, row and column
    const int k = lane / 3, col = lane % 3;
    unsigned long long t = 0ull;
    if (k < n_classes) {
      for (int i = 0; i < kRunsLanes; ++i)
        t += col == 1 ? s_sse[k * kRunsLanes + i] : (unsigned long long)s_cnt[(col == 2 ? n_classes : 0) * kRunsLanes + k * kRunsLanes + i];
    } else {
      t = col == 0 ? (unsigned long long)nrows * (unsigned long long)W : s_tot[col - 1];
    }
    if (t) atomicAdd(&sums[lane], t);
  }
}

static int runs_check(rhccq_ctx* ctx, const void* rgb, int32_t H, int32_t W, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                      const uint32_t* slack, const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  if (const int rc = rows_check(ctx, "palette_runs", rgb, H, W, palette, K, cls, n_classes, slack, idx_out, idx_elem_bytes, sums)) return rc;
  if (const int rc = search_limit(ctx, "palette_runs", K)) return rc;
  for (int i = 0; i <= n_classes; ++i)
    if (slack[i] > kRunsMaxSlack) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_runs: a slack is at most 195075");
  return 0;
}

template <typename IdxT>
static void runs_host(const uint8_t* rgb, int H, int W, const uint8_t* pal, const uint8_t* cls, int n_classes, const uint32_t* slack,
                      IdxT* idx, uint64_t* sums) {
  for (int y = 0; y < H; ++y) {
    RunsState st{0u, 0u, 0u};
    for (int x = 0; x < W; ++x) {
      const long long p = (long long)y * W + x;
      const uint32_t px = remap_pack_px(rgb + p * 3), b = (uint32_t)idx[p], pb = remap_pack_px(pal + (long long)b * 3);
      runs_step(st, px, runs_limit(px, pb, slack[runs_class(cls, p, n_classes)], x == 0), b, pb);
      idx[p] = (IdxT)st.idx;
      rows_add_host(sums, runs_class(cls, p, n_classes), n_classes, {1, runs_dist(px, st.col), st.idx != b ? 1u : 0u});
    }
  }
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_runs_tile_cols(void) { return kRunsCols; }
int32_t rhccq_palette_runs_rows(void) { return kRunsRowsDefault; }

int rhccq_palette_runs(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                       int32_t n_classes, const uint32_t* slack_host, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = runs_check(ctx, rgb, H, W, palette, K, cls, n_classes, slack_host, idx_out, idx_elem_bytes, sums)) return rc;
  const size_t sums_bytes = (size_t)(n_classes + 1) * 3 * sizeof(uint64_t);
  const int64_t n = (int64_t)H * W;
  if (n == 0) {
    RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
    return 0;
  }
  // b into idx_out; the remap's own {pixels, SSE} land in the first two words of sums, which the memset behind it clears again
  if (const int rc = rhccq_palette_remap(ctx, rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, sums)) return rc;
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
  RunsSlack slack{};
  for (int i = 0; i <= n_classes; ++i) slack.v[i] = slack_host[i];
  const int rows = ctx->opt_runs_rows > 0 ? ctx->opt_runs_rows : kRunsRowsDefault;
  const dim3 grid((unsigned)((H + rows - 1) / rows)), block(kRunsLanes);
  const size_t lds = runs_lds_bytes(rows, K, n_classes);                               // at most 41 088 bytes: below the 64 KiB a launch gets unasked
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(palette_runs_kernel<T>, grid, block, lds, ctx->stream, rgb, (int)H, (int)W, palette, (int)K, cls, (int)n_classes, slack, rows,
                       (T*)idx_out, (unsigned long long*)sums);
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_runs_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                            const uint32_t* slack, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = runs_check(nullptr, rgb, H, W, palette, K, cls, n_classes, slack, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i < (n_classes + 1) * 3; ++i) sums[i] = 0;
  const int64_t n = (int64_t)H * W;
  if (n == 0) return 0;
  uint64_t remap_sums[2];
  if (const int rc = rhccq_palette_remap_host(rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, remap_sums)) return rc;
  index_dispatch(idx_elem_bytes, [&](auto* t) { runs_host(rgb, H, W, palette, cls, n_classes, slack, (decltype(t))idx_out, sums); });
  return 0;
}

}  // extern "C"
