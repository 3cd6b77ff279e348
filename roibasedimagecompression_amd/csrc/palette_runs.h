// The step function and constants of the run-carrying remap, shared by its kernel and its host form (palette_runs.hip).
//
// Arithmetic.  With w(p, c) = 2 p.c - |c|^2 the squared distance is |p - c|^2 = |p|^2 - w(p, c), and |p|^2 is the same on both sides of
//     |p - cur|^2 <= |p - palette[b]|^2 + slack      <=>      w(p, cur) >= w(p, palette[b]) - slack  =: lim
// and, p.cur being an integer,                        <=>      p.cur >= ceil((lim + |cur|^2) / 2) = (lim + |cur|^2 + 1) >> 1
// lim is known before the chain reaches the pixel and |cur|^2 one step earlier than cur's use, so the loop-carried work of a step is one
// dot product beside one add and one shift, one compare and the selects of the carried row.  |w| <= 2 * 195075 and slack <= 195075:
// everything fits int32.  The first pixel of an image row takes lim = kRunsNever, above every 2 p.c: it never keeps a carried row.
#pragma once
#include "palette_remap.h"

namespace rhccq {

constexpr int kRunsLanes = 64;            // lanes of a workgroup (one wave): a lane walks one image row
constexpr int kRunsCols = 64;             // columns of a staging tile: a wave stages one row segment of 64 pixels per load
constexpr int kRunsPitch = kRunsCols + 1; // dwords between the rows of a tile in LDS: odd, so the lanes walking a tile's rows hit different banks
constexpr int kRunsRowsMax = 8;           // image rows of a workgroup at most: a lane holds a tile column of that many rows in registers
constexpr int kRunsRowsDefault = 4;       // image rows of a workgroup (2, 4 or 8): 2160 rows are 540 workgroups
constexpr int kRunsLdsPalette = 4096;     // palettes of at most this many rows are gathered from LDS, larger ones from global memory
constexpr uint32_t kRunsMaxSlack = 195075u;   // 3 * 255^2
constexpr int32_t kRunsNever = 1 << 30;

struct RunsSlack { uint32_t v[kRemapMaxClasses + 1]; };
// the row a lane carries along its image row: its colour (0x00RRGGBB), |colour|^2 and its index
struct RunsState { uint32_t col, n2, idx; };

__host__ __device__ __forceinline__ int32_t runs_w(uint32_t px, uint32_t col, uint32_t n2) { return 2 * (int32_t)remap_dot(px, col) - (int32_t)n2; }
// the limit of a pixel whose nearest row has the colour pb: w(p, pb) - slack, or `never` for the first pixel of an image row
__host__ __device__ __forceinline__ int32_t runs_limit(uint32_t px, uint32_t pb, uint32_t slack, bool first) {
  return first ? kRunsNever : runs_w(px, pb, remap_dot(pb, pb)) - (int32_t)slack;
}
// one step of the chain: the carried row stays iff it is within the limit, else the pixel's nearest row (b, pb) takes over.  px may carry
// anything in its top byte: it only meets colours there, whose top byte is zero
__host__ __device__ __forceinline__ void runs_step(RunsState& s, uint32_t px, int32_t lim, uint32_t b, uint32_t pb) {
  const uint32_t pbn2 = remap_dot(pb, pb);                                          // (off the chain)
  const int32_t need = (lim + (int32_t)s.n2 + 1) >> 1;                              // (beside the dot product, not behind it)
  const bool keep = (int32_t)remap_dot(px, s.col) >= need;
  s.col = keep ? s.col : pb;
  s.n2 = keep ? s.n2 : pbn2;
  s.idx = keep ? s.idx : b;
}
// the squared distance of a pixel to a colour
__host__ __device__ __forceinline__ uint32_t runs_dist(uint32_t px, uint32_t col) {
  return (uint32_t)((int32_t)remap_dot(px, px) - runs_w(px, col, remap_dot(col, col)));
}
// a pixel's class row: its class below n_classes, else the last row (also without a class map)
__host__ __device__ __forceinline__ uint32_t runs_class(const uint8_t* cls, long long p, int n_classes) {
  if (!cls) return (uint32_t)n_classes;
  const uint32_t c = cls[p];
  return c < (uint32_t)n_classes ? c : (uint32_t)n_classes;
}

// ---- shared by the host side of the run-carrying remap and of the row segmentation (palette_segment.hip), `what` the operation's name ----
// the argument tests both have (`table`: the slack or the penalty of every class row); each appends its own last two in its own order
static inline int rows_check(rhccq_ctx* ctx, const char* what, const void* rgb, int32_t H, int32_t W, const void* palette, int32_t K, const void* cls,
                             int32_t n_classes, const uint32_t* table, const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  if (!rgb || !palette || !idx_out || !sums || !table) return remap_fail(ctx, RHCCQ_E_ARG, what, ": null argument");
  if (K < 1 || H < 0 || W < 0) return remap_fail(ctx, RHCCQ_E_ARG, what, ": K >= 1, H >= 0 and W >= 0 are required");
  if (const int rc = classes_check(ctx, what, cls, n_classes)) return rc;
  if (const int rc = index_check(ctx, what, idx_out, idx_elem_bytes)) return rc;
  if ((uintptr_t)sums & 7) return remap_fail(ctx, RHCCQ_E_ARG, what, ": misaligned sums");
  return index_rows_check(ctx, what, idx_elem_bytes, K);
}
// the host forms: one pixel's row of sums `v` added to its class row k (if it has one) and to the total, the last row
template <int kCols>
static inline void rows_add_host(uint64_t* sums, uint32_t k, int n_classes, const uint64_t (&v)[kCols]) {
  for (int j = 0; j < kCols; ++j) {
    if (k < (uint32_t)n_classes) sums[k * kCols + j] += v[j];
    sums[n_classes * kCols + j] += v[j];
  }
}

}  // namespace rhccq
