// A palette from the image on the device (EXTENSION, no reference counterpart): greedy variance-minimising box splitting over a
// 32 x 32 x 32 colour histogram (Wu's quantiser) with exact rational comparisons.  The definition is in include/rhccq.h; in short:
// rhccq_palette_cells sums weight and weight x channel value per cell (r >> 3, g >> 3, b >> 3) in 64-bit integers; rhccq_palette_build
// starts from the whole cube as box 0 and, while fewer than K_target boxes exist, splits the box whose best cut removes the most squared
// error, |N S1 - N1 S|^2 / (N N1 (N - N1)), ties to the lowest box, axis and position; a box's row is floor((2 S + N) / (2 N)).
//
// Exactness.  The sum of N is at most 2^32 - 1 and S <= 255 N < 2^40, so N S1 and N1 S are below 2^72, their difference squared below 2^144,
// the three channels together below 2^146 (three 64-bit limbs); N N1 < 2^64 and the denominator below 2^96 (two limbs).  Two gains are
// compared by cross-multiplication: each side is below 2^242 and is formed limb by limb (build_cross, palette_build.h).  128 bits are not
// enough: a 512 x 768 picture already needs 138.
//
// Device form of the cells pass: one launch (behind a memset unless the call accumulates).  The table is 1 MiB, six times the LDS of a CU,
// so it stays in global memory and what is reduced is the number of atomics that reach it, above all the ones that meet on the cells of
// a picture's large flat areas (adds to one address serialise).  Two levels.  (1) A lane holds 8 pixels a block apart, so the 64 lanes of
// a wave hold 64 neighbouring pixels of an image row at a time, and neighbouring pixels mostly share cells: the wave takes the cell of its
// first open lane and sums {w, w r, w g, w b} over the lanes of that cell (the sums stay below 2^22); after kCellsRounds such rounds the
// lanes still open go on with their own pixel.  (2) A workgroup owns a contiguous stretch of the picture and a table of kCellsSlots slots
// in LDS, {cell, N, Sr, Sg, Sb} with 64-bit sums (36 bytes a slot, four workgroups a CU): a contribution goes to the slot its cell's low
// coordinate bits name, which the first cell to come claims (one LDS compare-and-swap), and a cell that finds its slot taken by another
// goes straight to global memory; at the end every claimed slot is flushed with four 64-bit global atomics.  One colour costs four global
// atomics a workgroup; noise costs the plain per-pixel form plus the rounds.  The alternatives lose here: a table of N alone in LDS
// (128 KiB) leaves one workgroup a CU and still sends S to global memory; a full partial table per workgroup is 1 MiB of traffic per
// workgroup against the kilobytes of pixels it reads.  Integer addition only: every order gives the same table.
//
// Device form of the build: three launches that turn the planes into the summed-volume table T[33][33][33] of {N, Sr, Sg, Sb} in the
// workspace (a running sum along b, then g, then r; an entry is at most 2^40), then ONE resident workgroup of four waves that runs the
// chain: boxes, their best cut and its gain (48 bytes a box) live in LDS.  A step is three barriers: the candidate cuts of the two boxes
// the last split made, one lane each (two waves a box, 12 table corners of 32 bytes from L2 per lane), wave butterflies on the key | lane
// 0 stores boxes, cuts and gains | the arg-max over the cached gains.  The two errors that only the table shows (N all zero; a sum above
// 2^32 - 1) cannot be returned without a synchronisation: the chain kernel writes RHCCQ_E_ARG or RHCCQ_E_LIMIT to *k_out, zero outputs
// and -1 throughout splits.  N enters the table clamped (reduce_clamp), so that no sum of 32 768 cells wraps.
#include "palette_build.h"

#include <vector>

namespace rhccq {

// (the bodies of the kernels, their constants and the argument checks are in palette_build.h)
__global__ __launch_bounds__(kCellsBlock) void palette_cells_kernel(const uint8_t* __restrict__ rgb, long long n_px, const uint8_t* __restrict__ cls,
                                                                    int n_classes, CellsWeights wt, unsigned long long* __restrict__ cells) {
  palette_cells_body(rgb, n_px, cls, n_classes, wt, cells, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void palette_build_prefix_b_kernel(const unsigned long long* __restrict__ cells, unsigned long long* __restrict__ T) {
  build_prefix_b_body(cells, T, blockIdx.x * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void palette_build_prefix_kernel(unsigned long long* __restrict__ T, int outer_stride, int step) {
  build_prefix_body(T, outer_stride, step, blockIdx.x * 256 + threadIdx.x);
}

__global__ __launch_bounds__(kBuildBlock) void palette_build_chain_kernel(const BuildSum* __restrict__ T, int K_target, uint8_t* __restrict__ pal_out,
                                                                          unsigned long long* __restrict__ counts_out, uint8_t* __restrict__ boxes_out,
                                                                          int32_t* __restrict__ splits, int32_t* __restrict__ k_out) {
  build_chain_body(T, K_target, pal_out, counts_out, boxes_out, splits, k_out);
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_cells_block(void) { return kCellsBlock; }
int32_t rhccq_palette_cells_chunk(void) { return kCellsChunk; }
int32_t rhccq_palette_build_max_rows(void) { return kBuildMaxRows; }
int64_t rhccq_palette_build_bytes(void) { return (int64_t)kBuildTabEntries * (int64_t)sizeof(BuildSum); }

int rhccq_palette_cells(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights_host,
                        int32_t accumulate, uint64_t* cells) {
  if (!ctx) return RHCCQ_E_ARG;
  CellsWeights wt = {};
  if (const int rc = cells_check(ctx, rgb, n_pixels, cls, n_classes, weights_host, cells, &wt)) return rc;
  if (!accumulate) RHCCQ_HIP(ctx, hipMemsetAsync(cells, 0, (size_t)kBuildCells * 4 * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const long long chunks = (n_pixels + kCellsChunk - 1) / kCellsChunk, cap = (long long)ctx->compute_units * 4;
  const long long blocks = chunks < cap ? chunks : cap;
  hipLaunchKernelGGL(palette_cells_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(kCellsBlock), 0, ctx->stream, rgb, (long long)n_pixels, cls,
                     (int)n_classes, wt, (unsigned long long*)cells);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_cells_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights, int32_t accumulate,
                             uint64_t* cells) {
  CellsWeights wt = {};
  if (const int rc = cells_check(nullptr, rgb, n_pixels, cls, n_classes, weights, cells, &wt)) return rc;
  if (!accumulate)
    for (int j = 0; j < kBuildCells * 4; ++j) cells[j] = 0;
  for (int64_t p = 0; p < n_pixels; ++p) {
    const uint64_t w = wt.w[n_classes > 0 && cls[p] < n_classes ? cls[p] : n_classes];
    const int cell = build_cell(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2]);
    cells[cell] += w;
    for (int ch = 0; ch < 3; ++ch) cells[(size_t)(ch + 1) * kBuildCells + cell] += w * rgb[p * 3 + ch];
  }
  return 0;
}

int rhccq_palette_build(rhccq_ctx* ctx, const uint64_t* cells, int32_t K_target, void* work, int64_t work_bytes, uint8_t* palette_out,
                        uint64_t* counts_out, uint8_t* boxes_out, int32_t* splits, int32_t* k_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: null argument");
  if (const int rc = build_check(ctx, cells, K_target, palette_out, counts_out, splits, k_out)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: misaligned workspace");
  if (K_target > kBuildMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build: more rows than rhccq_palette_build_max_rows() (the host form takes up to 32768)");
  if (work_bytes < rhccq_palette_build_bytes()) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: the workspace is smaller than rhccq_palette_build_bytes()");
  unsigned long long* T = (unsigned long long*)work;
  const dim3 grid((unsigned)((kBuildTab * kBuildTab * 4 + 255) / 256)), block(256);
  hipLaunchKernelGGL(palette_build_prefix_b_kernel, grid, block, 0, ctx->stream, (const unsigned long long*)cells, T);
  hipLaunchKernelGGL(palette_build_prefix_kernel, grid, block, 0, ctx->stream, T, kBuildTab * kBuildTab * 4, kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_prefix_kernel, grid, block, 0, ctx->stream, T, kBuildTab * 4, kBuildTab * kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_chain_kernel, dim3(1), dim3(kBuildBlock), 0, ctx->stream, (const BuildSum*)work, (int)K_target, palette_out,
                     (unsigned long long*)counts_out, boxes_out, splits, k_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_build_host(const uint64_t* cells, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out, uint8_t* boxes_out, int32_t* splits,
                             int32_t* k_out) {
  if (const int rc = build_check(nullptr, cells, K_target, palette_out, counts_out, splits, k_out)) return rc;
  std::vector<BuildSum> T((size_t)kBuildTabEntries, BuildSum{0ull, {0ull, 0ull, 0ull}});
  for (int x = 1; x < kBuildTab; ++x)
    for (int y = 1; y < kBuildTab; ++y)
      for (int z = 1; z < kBuildTab; ++z) {
        const int c = ((x - 1) * kBuildSide + (y - 1)) * kBuildSide + (z - 1);
        BuildSum v = {reduce_clamp(cells[c]), {cells[kBuildCells + c], cells[2 * kBuildCells + c], cells[3 * kBuildCells + c]}};
        v = build_add(v, T[build_tab_index(x - 1, y, z)]);
        v = build_add(v, T[build_tab_index(x, y - 1, z)]);
        v = build_add(v, T[build_tab_index(x, y, z - 1)]);
        v = build_sub(v, T[build_tab_index(x - 1, y - 1, z)]);
        v = build_sub(v, T[build_tab_index(x - 1, y, z - 1)]);
        v = build_sub(v, T[build_tab_index(x, y - 1, z - 1)]);
        T[build_tab_index(x, y, z)] = build_add(v, T[build_tab_index(x - 1, y - 1, z - 1)]);
      }
  const unsigned long long total = T[build_tab_index(kBuildSide, kBuildSide, kBuildSide)].n;
  if (total == 0ull) return RHCCQ_E_ARG;
  if (total > kReduceMaxSum) return RHCCQ_E_LIMIT;
  std::vector<BuildBox> box(1, build_whole());
  std::vector<BuildKey> key(1, build_best_cut(T.data(), box[0]));
  int done = 0;
  while ((int)box.size() < K_target) {
    BuildKey best = build_no_key();
    for (size_t j = 0; j < box.size(); ++j) {
      BuildKey c = key[j];
      c.idx = (uint32_t)j;
      if (build_before(c, best)) best = c;
    }
    if (!build_has_cut(best)) break;
    const int a = (int)best.idx, code = (int)key[a].idx;
    box.push_back(build_split(box[a], code));
    key[a] = build_best_cut(T.data(), box[a]);
    key.push_back(build_best_cut(T.data(), box.back()));
    if (splits) {
      splits[done * 3] = a;
      splits[done * 3 + 1] = code >> 5;
      splits[done * 3 + 2] = code & (kBuildSide - 1);
    }
    ++done;
  }
  const int nb = (int)box.size();
  for (int j = 0; j < K_target; ++j) {
    if (j < nb) build_row(build_box_sum(T.data(), box[j]), palette_out + j * 3, (unsigned long long*)counts_out + j);
    else {
      palette_out[j * 3] = palette_out[j * 3 + 1] = palette_out[j * 3 + 2] = 0;
      counts_out[j] = 0;
    }
    if (boxes_out)
      for (int i = 0; i < 3; ++i) {
        boxes_out[j * 6 + i] = j < nb ? box[j].lo[i] : 0;
        boxes_out[j * 6 + 3 + i] = j < nb ? box[j].hi[i] : 0;
      }
  }
  if (splits)
    for (int j = done * 3; j < (K_target - 1) * 3; ++j) splits[j] = -1;
  *k_out = nb;
  return 0;
}

}  // extern "C"
