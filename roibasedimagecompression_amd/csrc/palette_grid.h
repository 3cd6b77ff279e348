// The colour-cell candidate grid of the nearest-colour search: its constants, the cell of a pixel, a row's nearest and farthest squared
// distance to a cell's box, where a cell's list goes (grid_place) and the layout of the caller's workspace.  The device kernels and the
// serial host forms (palette_grid.hip) run these same functions; the entries of a list are palette_remap.h's RemapEntry, evaluated and
// carried by its remap_eval / remap_dist.  The definition and the exactness argument are in include/rhccq.h and DESIGN.md section 3o.
#pragma once
#include "palette_remap.h"

namespace rhccq {

constexpr int kGridShift = 3;                          // a cell is 8 x 8 x 8 colours: the grid of palette_build.hip's histogram
constexpr int kGridCell = 1 << kGridShift;
constexpr int kGridCells = 32 * 32 * 32;
constexpr int kGridMaxList = 1024;                     // positions of a list: with the pad entry's 1024 still within the 12 index bits
constexpr int64_t kGridMaxEntries = (int64_t)kGridCells * kGridMaxList;
constexpr int kGridBlock = 256;
constexpr int kGridWaveCells = 8;                      // cells a wave of the build carries: a staged row is read once for the eight
constexpr int kGridBlockCells = kGridWaveCells * (kGridBlock / 64);
constexpr int kGridPx = 4;                             // pixels a lane of the remap keeps in flight: four independent 16-byte loads a step
constexpr long long kGridChunk = (long long)kGridBlock * kGridPx;
static_assert(kGridMaxList < (1 << kRemapIdxBits) && kGridCells % kGridBlockCells == 0, "a list position must fit its 12 bits");

// the cell number of a packed pixel 0x00RRGGBB: (r >> 3) << 10 | (g >> 3) << 5 | (b >> 3)
__host__ __device__ __forceinline__ uint32_t grid_cell(uint32_t px) {
  return (((px >> (16 + kGridShift)) & 31u) << 10) | (((px >> (8 + kGridShift)) & 31u) << 5) | ((px >> kGridShift) & 31u);
}
// the squared distance from packed row `c` to the nearest (dmin) and to the farthest (dmax) point of the box of `cell`
__host__ __device__ __forceinline__ void grid_bounds(uint32_t c, uint32_t cell, uint32_t& dmin, uint32_t& dmax) {
  dmin = dmax = 0u;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int lo = (int)((cell >> (5 * ch)) & 31u) << kGridShift;
    const int a = (int)((c >> (8 * ch)) & 255u) - lo, b = kGridCell - 1 - a;       // c - lo and hi - c
    const int far = a > b ? a : b, out = -a > -b ? -a : -b, near = out > 0 ? out : 0;
    dmax += (uint32_t)(far * far);
    dmin += (uint32_t)(near * near);
  }
}
// a cell of `n` rows behind `off` entries of the cells before it, `cap` entries in all: its padded length through *len2 (0 above
// the per-cell cap: such a cell takes no room), and whether it is listed
__host__ __device__ __forceinline__ bool grid_place(uint32_t n, uint32_t off, uint32_t cap, uint32_t* len2) {
  *len2 = n > (uint32_t)kGridMaxList ? 0u : (n + 1u) & ~1u;
  return n <= (uint32_t)kGridMaxList && off + *len2 <= cap;
}

// the workspace of a grid of `entries`: byte offsets of its pieces (each a multiple of 256), pinned in include/rhccq.h
struct GridLayout {
  int64_t cap, cells, bound, count, lists, rows, bytes;
};
static inline GridLayout grid_layout(int64_t entries) {
  GridLayout g;
  g.cap = entries & ~(int64_t)1;
  const int64_t store = g.cap < 2 ? 2 : g.cap;         // a flagged pixel's lane still reads pair 0
  g.cells = 0;
  g.bound = g.cells + (int64_t)kGridCells * 8;
  g.count = g.bound + (int64_t)kGridCells * 4;
  g.lists = g.count + (int64_t)kGridCells * 4;
  g.rows = g.lists + align256(store * 8);
  g.bytes = g.rows + align256(store * 2);
  return g;
}
struct GridView {
  uint2* cells;                 // {first entry (even), rows}; rows == 0: flagged
  uint32_t *bound, *count;      // U(C) and the rows with dmin <= U(C), as the count pass left them
  RemapEntry* lists;
  uint16_t* rows;
};
static inline GridView grid_view(void* work, const GridLayout& g) {
  char* w = (char*)work;
  return {(uint2*)(w + g.cells), (uint32_t*)(w + g.bound), (uint32_t*)(w + g.count), (RemapEntry*)(w + g.lists), (uint16_t*)(w + g.rows)};
}

static inline int grid_check(rhccq_ctx* ctx, const char* what, const void* palette, int32_t K, int64_t entries, const void* work, int64_t work_bytes,
                             const void* stats) {
  if (!palette || !work || !stats) return remap_fail(ctx, RHCCQ_E_ARG, what, ": null argument");
  if (K < 1 || entries < 0) return remap_fail(ctx, RHCCQ_E_ARG, what, ": K >= 1 and entries >= 0 are required");
  if (((uintptr_t)work & 15) || ((uintptr_t)stats & 7)) return remap_fail(ctx, RHCCQ_E_ARG, what, ": misaligned workspace or stats");
  if (const int rc = search_limit(ctx, what, K)) return rc;
  if (entries > kGridMaxEntries) return remap_fail(ctx, RHCCQ_E_LIMIT, what, ": at most 33554432 entries");
  if (work_bytes < grid_layout(entries).bytes) return remap_fail(ctx, RHCCQ_E_ARG, what, ": workspace too small");
  return 0;
}

}  // namespace rhccq
