// Exact nearest-colour search through a colour-cell candidate grid (EXTENSION, no reference counterpart): the pruned second path beside
// palette_remap.hip's full search, with the same indices and sums bit for bit (definition: include/rhccq.h; argument: DESIGN.md 3o).
//
// Build (rhccq_palette_grid): count, exclusive scan, fill over the 32 768 cells of 8 x 8 x 8 colours.
//   count / fill  A workgroup of four waves takes 32 consecutive cells (one (r, g) column of the grid), eight per wave, and walks the
//                 palette through LDS in the search's tile size as packed 0x00RRGGBB words.  Lane l of a wave takes rows l, l + 64, ...
//                 of the tile (consecutive LDS words: no bank conflict) and evaluates each against the wave's eight cells, which are
//                 wave-uniform: a row is read from LDS once for eight cells.  A WAVE per cell, not a workgroup: the reductions (minimum
//                 of dmax, the count, the fill's ballot) are wave operations with no barrier and no LDS, and a workgroup per cell would
//                 stage the whole palette for one cell's K evaluations, as many bytes as evaluations.  With 32 cells a workgroup the
//                 staging is 1 / 32 of that, and the only barriers are those of the staging.
//                 count: pass 1 reduces U(C) = min dmax, pass 2 counts the rows with dmin <= U(C); a palette of one tile is staged once.
//                 fill: one pass; rows are visited in ascending order, a ballot of (dmin <= U) and the population count of the lower
//                 lanes give every listed row its position.  The entry is remap_pack_entry(row, position); an odd list is padded with a
//                 copy of its last entry under the next position (the search's rule: equal key, higher index, never the minimum).
//   scan          ONE workgroup of 1024 lanes, 32 consecutive cells a lane: block_exscan of the padded lengths, then each lane places
//                 its cells in order (grid_place) and the four stats are reduced in LDS.
// Remap (rhccq_palette_remap_grid): a lane owns kGridPx pixels of a chunk and walks each pixel's own list with 16-byte loads of two
// entries.  Lanes of a wave are in different cells, so nothing is broadcast through LDS: the lists are read through the vector cache
// and stay in L2.  A lane whose lists differ in length reads the last pair of the shorter ones again (a minimum is idempotent), so
// the loop body has no branch and four independent loads in flight.  The row id is fetched once, for the winner.  A pixel of a
// flagged cell is appended to the overflow queue (one atomic per wave and pixel slot, the pixel number and its three bytes with
// vector stores); a second launch runs remap_search, the full search, over the queue's packed pixels and adds to the same sums.
#include "palette_grid.h"

namespace rhccq {

// every lane of the workgroup walks the K rows tile by tile: f(j, row, valid) for j = tile_base + i * 64 + lane, all 64 lanes of a
// wave together (valid: j < K).  `staged`: the single tile of a small palette is already in LDS.
template <typename F>
__device__ __forceinline__ void grid_walk(const uint8_t* __restrict__ pal, int K, uint32_t* s_row, bool& staged, F&& f) {
  const int lane = threadIdx.x & 63;
  const int n_tiles = (K + kRemapTile - 1) / kRemapTile;
  for (int t = 0; t < n_tiles; ++t) {
    const int tile_base = t * kRemapTile, len = min(kRemapTile, K - tile_base);
    if (n_tiles > 1 || !staged) {
      __syncthreads();
      for (int j = threadIdx.x; j < len; j += kGridBlock) s_row[j] = remap_pack_px(pal + (long long)(tile_base + j) * 3);
      __syncthreads();
      staged = true;
    }
    for (int i = 0; i < len; i += 64) {
      const bool valid = i + lane < len;
      f(tile_base + i + lane, valid ? s_row[i + lane] : 0u, valid);
    }
  }
}

__device__ __forceinline__ uint32_t wave_min_all(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o, 64));
  return v;
}

__global__ __launch_bounds__(kGridBlock) void grid_count_kernel(const uint8_t* __restrict__ pal, int K, uint32_t* __restrict__ bound,
                                                                uint32_t* __restrict__ count) {
  __shared__ uint32_t s_row[kRemapTile];
  const int lane = threadIdx.x & 63;
  const uint32_t cell0 = blockIdx.x * kGridBlockCells + (threadIdx.x >> 6) * kGridWaveCells;
  bool staged = false;
  uint32_t u[kGridWaveCells], n[kGridWaveCells];
#pragma unroll
  for (int c = 0; c < kGridWaveCells; ++c) { u[c] = 0xFFFFFFFFu; n[c] = 0u; }
  grid_walk(pal, K, s_row, staged, [&](int, uint32_t row, bool valid) {
#pragma unroll
    for (int c = 0; c < kGridWaveCells; ++c) {
      uint32_t dmin, dmax;
      grid_bounds(row, cell0 + c, dmin, dmax);
      u[c] = valid ? min(u[c], dmax) : u[c];
    }
  });
#pragma unroll
  for (int c = 0; c < kGridWaveCells; ++c) u[c] = wave_min_all(u[c]);
  grid_walk(pal, K, s_row, staged, [&](int, uint32_t row, bool valid) {
#pragma unroll
    for (int c = 0; c < kGridWaveCells; ++c) {
      uint32_t dmin, dmax;
      grid_bounds(row, cell0 + c, dmin, dmax);
      n[c] += valid && dmin <= u[c] ? 1u : 0u;
    }
  });
#pragma unroll
  for (int c = 0; c < kGridWaveCells; ++c) {
    const uint32_t t = wave_sum(n[c]);
    if (lane == 0) { bound[cell0 + c] = u[c]; count[cell0 + c] = t; }
  }
}

constexpr int kGridScanBlock = 1024, kGridScanCells = kGridCells / kGridScanBlock;

__global__ __launch_bounds__(kGridScanBlock) void grid_scan_kernel(const uint32_t* __restrict__ count, uint32_t cap, uint2* __restrict__ cells,
                                                                   unsigned long long* __restrict__ stats) {
  __shared__ uint32_t s_red[kGridScanBlock / 64 + 1];
  __shared__ uint32_t s_stat[4];                                          // listed cells, flagged cells, entries used, longest list
  if (threadIdx.x < 4) s_stat[threadIdx.x] = 0u;
  const uint32_t first = threadIdx.x * kGridScanCells;
  uint32_t mine = 0u, len2;
  for (int i = 0; i < kGridScanCells; ++i) {
    grid_place(count[first + i], 0u, 0u, &len2);
    mine += len2;
  }
  uint32_t off = block_exscan(mine, s_red, (uint32_t*)nullptr);            // (its barriers also order the zeroing of s_stat)
  uint32_t listed = 0u, used = 0u, longest = 0u;
  for (int i = 0; i < kGridScanCells; ++i) {
    const uint32_t n = count[first + i];
    const bool ok = grid_place(n, off, cap, &len2);
    cells[first + i] = ok ? make_uint2(off, n) : make_uint2(0u, 0u);
    if (ok) {
      ++listed;
      used = off + len2;
      longest = max(longest, n);
    }
    off += len2;
  }
  atomicAdd(&s_stat[0], listed);
  atomicAdd(&s_stat[1], (uint32_t)kGridScanCells - listed);
  atomicMax(&s_stat[2], used);
  atomicMax(&s_stat[3], longest);
  __syncthreads();
  if (threadIdx.x < 4) stats[threadIdx.x] = s_stat[threadIdx.x];
}

__global__ __launch_bounds__(kGridBlock) void grid_fill_kernel(const uint8_t* __restrict__ pal, int K, const uint32_t* __restrict__ bound,
                                                               const uint2* __restrict__ cells, RemapEntry* __restrict__ lists,
                                                               uint16_t* __restrict__ rows) {
  __shared__ uint32_t s_row[kRemapTile];
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  const uint32_t cell0 = blockIdx.x * kGridBlockCells + (threadIdx.x >> 6) * kGridWaveCells;
  bool staged = false;
  uint32_t u[kGridWaveCells], off[kGridWaveCells], len[kGridWaveCells], run[kGridWaveCells], last[kGridWaveCells];
#pragma unroll
  for (int c = 0; c < kGridWaveCells; ++c) {
    const uint2 ce = cells[cell0 + c];
    u[c] = bound[cell0 + c];
    off[c] = ce.x;
    len[c] = ce.y;                                                         // 0: flagged, nothing is written
    run[c] = last[c] = 0u;
  }
  grid_walk(pal, K, s_row, staged, [&](int j, uint32_t row, bool valid) {
    const uint32_t j0 = (uint32_t)__builtin_amdgcn_readfirstlane(j - lane);
#pragma unroll
    for (int c = 0; c < kGridWaveCells; ++c) {
      uint32_t dmin, dmax;
      grid_bounds(row, cell0 + c, dmin, dmax);
      const bool take = valid && len[c] != 0u && dmin <= u[c];
      const unsigned long long mask = __ballot(take);
      if (take) {
        const uint32_t pos = run[c] + (uint32_t)__popcll(mask & below);    // < len[c] <= 1024: the count pass counted these same rows
        lists[off[c] + pos] = remap_pack_entry(pal + (long long)j * 3, (int)pos);
        rows[off[c] + pos] = (uint16_t)j;
      }
      if (mask) last[c] = j0 + 63u - (uint32_t)__clzll((long long)mask);
      run[c] += (uint32_t)__popcll(mask);
    }
  });
#pragma unroll
  for (int c = 0; c < kGridWaveCells; ++c)
    if (lane == 0 && (len[c] & 1u)) {                                      // pad to an even length: the last entry under the next position
      lists[off[c] + len[c]] = remap_pack_entry(pal + (long long)last[c] * 3, (int)len[c]);
      rows[off[c] + len[c]] = (uint16_t)last[c];
    }
}

// ---- the sums of a remap: rows {pixels, SSE} per class in a table per wave, the last row in two registers of every lane ----
struct GridSums {
  unsigned long long wave[kGridBlock / 64][kRemapMaxClasses][2];
  unsigned long long all[kGridBlock / 64][2];
};
__device__ __forceinline__ void grid_sums_clear(GridSums& s) {
  for (int i = threadIdx.x; i < (int)(sizeof(GridSums) / 8); i += kGridBlock) ((unsigned long long*)&s)[i] = 0ull;
}
// NPX pixels of every lane: their class (any value >= n_classes: in no class row), distance and whether they count at all
template <int NPX>
__device__ __forceinline__ void grid_sums_add(GridSums& s, int n_classes, const unsigned (&c)[NPX], const uint32_t (&dist)[NPX], const bool (&ok)[NPX],
                                              unsigned long long& all_n, unsigned long long& all_sse) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < NPX; ++q) {
    all_n += ok[q] ? 1u : 0u;
    all_sse += ok[q] ? dist[q] : 0u;
  }
  for (int k = 0; k < n_classes; ++k) {
    unsigned long long v = 0ull, n = 0ull;
#pragma unroll
    for (int q = 0; q < NPX; ++q) {
      v += ok[q] && c[q] == (unsigned)k ? dist[q] : 0u;
      n += ok[q] && c[q] == (unsigned)k ? 1u : 0u;
    }
    v = wave_sum(v);
    n = wave_sum(n);
    if (lane == 0) { s.wave[wv][k][0] += n; s.wave[wv][k][1] += v; }       // this wave's table: no other writer
  }
}
__device__ __forceinline__ void grid_sums_flush(GridSums& s, int n_classes, unsigned long long all_n, unsigned long long all_sse,
                                                unsigned long long* __restrict__ sums) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  all_n = wave_sum(all_n);
  all_sse = wave_sum(all_sse);
  if (lane == 0) { s.all[wv][0] = all_n; s.all[wv][1] = all_sse; }
  __syncthreads();
  if ((int)threadIdx.x < (n_classes + 1) * 2) {                            // one atomic per workgroup, row and column
    const int k = threadIdx.x >> 1, col = threadIdx.x & 1;
    unsigned long long t = 0ull;
    for (int i = 0; i < kGridBlock / 64; ++i) t += k < n_classes ? s.wave[i][k][col] : s.all[i][col];
    if (t) atomicAdd(&sums[threadIdx.x], t);
  }
}

template <typename IdxT>
__global__ __launch_bounds__(kGridBlock) void palette_remap_grid_kernel(const uint8_t* __restrict__ rgb, long long n_px, const uint2* __restrict__ cells,
                                                                        const uint4* __restrict__ lists, const uint16_t* __restrict__ rows,
                                                                        const uint8_t* __restrict__ cls, int n_classes, IdxT* __restrict__ idx_out,
                                                                        unsigned long long* __restrict__ sums, uint32_t* __restrict__ queue,
                                                                        uint8_t* __restrict__ queue_rgb, unsigned long long* __restrict__ overflow) {
  __shared__ GridSums s_sum;
  grid_sums_clear(s_sum);
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const unsigned long long below = (1ull << lane) - 1ull;
  unsigned long long all_n = 0ull, all_sse = 0ull;
  const long long n_chunks = (n_px + kGridChunk - 1) / kGridChunk;
  for (long long chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    const long long base = chunk * kGridChunk + threadIdx.x;               // lane l: pixels base + l + 256 q, so index stores coalesce
    uint32_t px[kGridPx], pair[kGridPx], half[kGridPx], best[kGridPx], dist[kGridPx], top = 1u;
    unsigned c[kGridPx];
    bool ok[kGridPx], queued[kGridPx];
#pragma unroll
    for (int q = 0; q < kGridPx; ++q) {
      const long long p = base + (long long)q * kGridBlock;
      const bool in = p < n_px;
      px[q] = in ? remap_pack_px(rgb + p * 3) : 0u;
      const uint2 ce = cells[grid_cell(px[q])];
      ok[q] = in && ce.y != 0u;
      queued[q] = in && ce.y == 0u;
      pair[q] = ok[q] ? ce.x >> 1 : 0u;                                    // (a pixel without a list reads pair 0 and drops the result)
      half[q] = ok[q] ? (ce.y + 1u) >> 1 : 1u;
      top = max(top, half[q]);
      best[q] = 0xFFFFFFFFu;
    }
    for (uint32_t j = 0; j < top; ++j) {
#pragma unroll
      for (int q = 0; q < kGridPx; ++q) {
        const uint4 e = lists[pair[q] + min(j, half[q] - 1u)];
        best[q] = min(best[q], remap_eval(px[q], RemapEntry{e.x, e.y}));
        best[q] = min(best[q], remap_eval(px[q], RemapEntry{e.z, e.w}));
      }
    }
#pragma unroll
    for (int q = 0; q < kGridPx; ++q) {
      const long long p = base + (long long)q * kGridBlock;
      dist[q] = ok[q] ? remap_dist(px[q], best[q] >> kRemapIdxBits) : 0u;
      if (ok[q]) idx_out[p] = (IdxT)rows[2u * pair[q] + (best[q] & ((1u << kRemapIdxBits) - 1u))];
      c[q] = ok[q] && n_classes > 0 ? (unsigned)cls[p] : 0xFFFFFFFFu;
      const unsigned long long mask = __ballot(queued[q]);
      if (mask) {                                                          // (wave-uniform) one atomic for the wave's pixels of this slot
        unsigned long long at = 0ull;
        if (lane == __ffsll((long long)mask) - 1) at = atomicAdd(overflow, (unsigned long long)__popcll(mask));
        at = __shfl(at, __ffsll((long long)mask) - 1, 64) + (unsigned long long)__popcll(mask & below);
        if (queued[q]) {                                                   // at < n_px: every pixel is queued at most once
          queue[at] = (uint32_t)p;
          queue_rgb[at * 3] = (uint8_t)(px[q] >> 16);
          queue_rgb[at * 3 + 1] = (uint8_t)(px[q] >> 8);
          queue_rgb[at * 3 + 2] = (uint8_t)px[q];
        }
      }
    }
    grid_sums_add<kGridPx>(s_sum, n_classes, c, dist, ok, all_n, all_sse);
  }
  grid_sums_flush(s_sum, n_classes, all_n, all_sse, sums);
}

// the queued pixels through the full search; their number is read on the device
template <typename IdxT>
__global__ __launch_bounds__(kRemapBlock) void palette_remap_overflow_kernel(const uint8_t* __restrict__ queue_rgb, const uint32_t* __restrict__ queue,
                                                                             const unsigned long long* __restrict__ overflow,
                                                                             const uint8_t* __restrict__ pal, int K, const uint8_t* __restrict__ cls,
                                                                             int n_classes, IdxT* __restrict__ idx_out,
                                                                             unsigned long long* __restrict__ sums) {
  static_assert(kRemapBlock == kGridBlock, "the sums' tables are sized per wave of either kernel");
  __shared__ GridSums s_sum;
  grid_sums_clear(s_sum);
  __syncthreads();
  const long long n_q = (long long)*overflow;
  unsigned long long all_n = 0ull, all_sse = 0ull;
  remap_search(queue_rgb, n_q, pal, K, blockIdx.x, gridDim.x, [&](long long base, auto& px, auto& bkey, auto& bidx) {
    uint32_t dist[kRemapPx];
    unsigned c[kRemapPx];
    bool ok[kRemapPx];
#pragma unroll
    for (int q = 0; q < kRemapPx; ++q) {
      const long long at = base + (long long)q * kRemapBlock;
      ok[q] = at < n_q;
      const uint32_t p = ok[q] ? queue[at] : 0u;
      dist[q] = ok[q] ? remap_dist(px[q], bkey[q]) : 0u;
      if (ok[q]) idx_out[p] = (IdxT)bidx[q];
      c[q] = ok[q] && n_classes > 0 ? (unsigned)cls[p] : 0xFFFFFFFFu;
    }
    grid_sums_add<kRemapPx>(s_sum, n_classes, c, dist, ok, all_n, all_sse);
  });
  grid_sums_flush(s_sum, n_classes, all_n, all_sse, sums);
}

// the remap's workspace: the queue's pixel numbers, then their packed bytes
static inline int64_t remap_grid_bytes(int64_t n_pixels) { return align256(n_pixels * 4) + align256(n_pixels * 3); }

static int remap_grid_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                            const void* grid, int64_t entries, const void* idx_out, int32_t idx_elem_bytes, const void* sums, const void* overflow) {
  const char* const what = "palette_remap_grid";
  if (const int rc = search_check(ctx, what, !rgb || !palette || !idx_out || !sums || !grid || !overflow, n_pixels, K, cls, n_classes)) return rc;
  if (const int rc = index_check(ctx, what, idx_out, idx_elem_bytes)) return rc;
  if (((uintptr_t)sums & 7) || ((uintptr_t)overflow & 7) || ((uintptr_t)grid & 15)) return remap_fail(ctx, RHCCQ_E_ARG, what, ": misaligned sums, overflow or grid");
  if (entries < 0 || entries > kGridMaxEntries) return remap_fail(ctx, RHCCQ_E_ARG, what, ": entries must be those the grid was built with");
  if (const int rc = index_rows_check(ctx, what, idx_elem_bytes, K)) return rc;
  if (const int rc = search_limit(ctx, what, K)) return rc;
  return n_pixels > 0xFFFFFFFFll ? remap_fail(ctx, RHCCQ_E_LIMIT, what, ": at most 2^32 - 1 pixels") : 0;
}

template <typename IdxT>
static void remap_grid_host(const uint8_t* rgb, int64_t n_px, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, const GridView& g, IdxT* idx_out,
                            uint64_t* sums, uint64_t* overflow) {
  std::vector<RemapEntry> ent;                                             // the full search's palette, packed when the first pixel needs it
  for (int64_t p = 0; p < n_px; ++p) {
    const uint32_t px = remap_pack_px(rgb + p * 3);
    const uint2 ce = g.cells[grid_cell(px)];
    uint32_t key, idx;
    if (ce.y == 0u) {
      if (ent.empty()) ent = remap_pack_palette(pal, K);
      idx = remap_search_host(px, ent, &key);
      ++*overflow;
    } else {
      uint32_t best = 0xFFFFFFFFu;
      for (uint32_t j = 0; j < ce.y; ++j) {
        const uint32_t v = remap_eval(px, g.lists[ce.x + j]);
        best = v < best ? v : best;
      }
      key = best >> kRemapIdxBits;
      idx = g.rows[ce.x + (best & ((1u << kRemapIdxBits) - 1u))];
    }
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

int32_t rhccq_palette_grid_cell(void) { return kGridCell; }
int32_t rhccq_palette_grid_max_list(void) { return kGridMaxList; }
int32_t rhccq_palette_grid_chunk(void) { return (int32_t)kGridChunk; }

int64_t rhccq_palette_grid_bytes(int32_t K, int64_t entries) {
  return K < 1 || K > kRemapMaxK || entries < 0 || entries > kGridMaxEntries ? -1 : grid_layout(entries).bytes;
}

int rhccq_palette_grid(rhccq_ctx* ctx, const uint8_t* palette, int32_t K, int64_t entries, void* work, int64_t work_bytes, uint64_t* stats) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = grid_check(ctx, "palette_grid", palette, K, entries, work, work_bytes, stats)) return rc;
  const GridLayout lay = grid_layout(entries);
  const GridView g = grid_view(work, lay);
  hipLaunchKernelGGL(grid_count_kernel, dim3(kGridCells / kGridBlockCells), dim3(kGridBlock), 0, ctx->stream, palette, (int)K, g.bound, g.count);
  hipLaunchKernelGGL(grid_scan_kernel, dim3(1), dim3(kGridScanBlock), 0, ctx->stream, g.count, (uint32_t)lay.cap, g.cells, (unsigned long long*)stats);
  hipLaunchKernelGGL(grid_fill_kernel, dim3(kGridCells / kGridBlockCells), dim3(kGridBlock), 0, ctx->stream, palette, (int)K, g.bound, g.cells, g.lists,
                     g.rows);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_grid_host(const uint8_t* palette, int32_t K, int64_t entries, void* work, int64_t work_bytes, uint64_t* stats) {
  if (const int rc = grid_check(nullptr, "palette_grid", palette, K, entries, work, work_bytes, stats)) return rc;
  const GridLayout lay = grid_layout(entries);
  const GridView g = grid_view(work, lay);
  std::vector<uint32_t> row((size_t)K), dmin((size_t)K);
  for (int j = 0; j < K; ++j) row[j] = remap_pack_px(palette + (int64_t)j * 3);
  uint32_t off = 0u, len2;
  stats[0] = stats[1] = stats[2] = stats[3] = 0;
  for (uint32_t cell = 0; cell < (uint32_t)kGridCells; ++cell) {
    uint32_t u = 0xFFFFFFFFu, n = 0u, dmax;
    for (int j = 0; j < K; ++j) {
      grid_bounds(row[j], cell, dmin[j], dmax);
      u = dmax < u ? dmax : u;
    }
    for (int j = 0; j < K; ++j) n += dmin[j] <= u ? 1u : 0u;
    g.bound[cell] = u;
    g.count[cell] = n;
    const bool ok = grid_place(n, off, (uint32_t)lay.cap, &len2);
    g.cells[cell] = ok ? make_uint2(off, n) : make_uint2(0u, 0u);
    ++stats[ok ? 0 : 1];
    if (ok) {
      uint32_t pos = 0u;
      int last = 0;
      for (int j = 0; j < K; ++j)
        if (dmin[j] <= u) {
          g.lists[off + pos] = remap_pack_entry(palette + (int64_t)j * 3, (int)pos);
          g.rows[off + pos++] = (uint16_t)(last = j);
        }
      if (n & 1u) {
        g.lists[off + n] = remap_pack_entry(palette + (int64_t)last * 3, (int)n);
        g.rows[off + n] = (uint16_t)last;
      }
      stats[2] = off + len2;
      stats[3] = n > stats[3] ? n : stats[3];
    }
    off += len2;
  }
  return 0;
}

int64_t rhccq_palette_remap_grid_bytes(int64_t n_pixels) { return n_pixels < 0 || n_pixels > 0xFFFFFFFFll ? -1 : remap_grid_bytes(n_pixels); }

int rhccq_palette_remap_grid(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                             const void* grid, int64_t entries, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums, void* work, int64_t work_bytes,
                             uint64_t* overflow) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = remap_grid_check(ctx, rgb, n_pixels, palette, K, cls, n_classes, grid, entries, idx_out, idx_elem_bytes, sums, overflow)) return rc;
  if (n_pixels > 0 && (!work || ((uintptr_t)work & 15) || work_bytes < remap_grid_bytes(n_pixels)))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap_grid: workspace null, misaligned or too small");
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)(n_classes + 1) * 2 * sizeof(uint64_t), ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(overflow, 0, sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const GridView g = grid_view(const_cast<void*>(grid), grid_layout(entries));
  uint32_t* const queue = (uint32_t*)work;
  uint8_t* const queue_rgb = (uint8_t*)work + align256(n_pixels * 4);
  // 8 workgroups of 4 waves per CU: the walk waits for memory, so every wave slot the registers allow is filled; never more than chunks
  const long long chunks = (n_pixels + kGridChunk - 1) / kGridChunk, cap = (long long)ctx->compute_units * 8;
  const dim3 grid_dim((unsigned)(chunks < cap ? chunks : cap)), over_dim(remap_blocks(n_pixels, cap)), block(kGridBlock);
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(palette_remap_grid_kernel<T>, grid_dim, block, 0, ctx->stream, rgb, (long long)n_pixels, (const uint2*)g.cells, (const uint4*)g.lists,
                       (const uint16_t*)g.rows, cls, (int)n_classes, (T*)idx_out, (unsigned long long*)sums, queue, queue_rgb, (unsigned long long*)overflow);
    hipLaunchKernelGGL(palette_remap_overflow_kernel<T>, over_dim, block, 0, ctx->stream, (const uint8_t*)queue_rgb, (const uint32_t*)queue,
                       (const unsigned long long*)overflow, palette, (int)K, cls, (int)n_classes, (T*)idx_out, (unsigned long long*)sums);
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_remap_grid_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                                  const void* grid, int64_t entries, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums, uint64_t* overflow) {
  if (const int rc = remap_grid_check(nullptr, rgb, n_pixels, palette, K, cls, n_classes, grid, entries, idx_out, idx_elem_bytes, sums, overflow)) return rc;
  for (int i = 0; i < (n_classes + 1) * 2; ++i) sums[i] = 0;
  *overflow = 0;
  const GridView g = grid_view(const_cast<void*>(grid), grid_layout(entries));
  index_dispatch(idx_elem_bytes, [&](auto* t) { remap_grid_host(rgb, n_pixels, palette, K, cls, n_classes, g, (decltype(t))idx_out, sums, overflow); });
  return 0;
}

}  // extern "C"
