// Segment tables and label layers of subregion_quantization (encoder/compression/subregions.py:90-683) for all regions of a frame,
// after the nearest-neighbour upscale of their SLIC labels (api/image.py, ImageEncoder).  A region r is a box of the frame and a
// label of one of two connected-component maps (ROI / non-ROI); its SLIC labels are a small map that the upscale reads through
// per-axis index tables (scipy.ndimage.zoom(order=0, grid_mode=True, mode='mirror'), computed on the host as api/slic.py does):
//
//   regions[r][kImgRegionCols] = y0, x0, h, w, map, label, small_off, small_w, yx_off, sid_off, layer
//   seg(r, y, x) = small[small_off + yi[yx_off + y] * small_w + xi[yx_off + h + x]]
//
//   image_seg_counts_kernel   in-mask pixel count of every (region, SLIC id): the segments subregion_quantization keeps and the
//                             "fills its whole box" drop test (count == h * w) both follow from it;
//   image_overlap_kernel      whether region r's mask meets the painted pixels of an earlier region q (pairs of regions of
//                             different maps): the host places regions in layers from these flags;
//   image_paint_kernel        writes every region's segment ids into its int32 layer.
// A region's pixels are covered by consecutive workgroups of 256 (block_item / block_first tables built on the host).
#include "rhccq_common.h"

namespace rhccq {

constexpr int kImgRegionCols = 11;

struct ImgRegion {
  int y0, x0, h, w, map, label, small_off, small_w, yx_off, sid_off, layer;
};

__device__ __forceinline__ ImgRegion img_region(const int32_t* regions, int r) {
  const int32_t* q = regions + (size_t)r * kImgRegionCols;
  return {q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], q[9], q[10]};
}

__device__ __forceinline__ int img_seg(const ImgRegion& g, const int32_t* small, const int32_t* yx, int y, int x) {
  return small[(size_t)g.small_off + (size_t)yx[g.yx_off + y] * g.small_w + yx[g.yx_off + g.h + x]];
}

__device__ __forceinline__ bool img_in(const ImgRegion& g, const int32_t* labels0, const int32_t* labels1, int FW, int fy, int fx) {
  return (g.map ? labels1 : labels0)[(size_t)fy * FW + fx] == g.label;
}

__global__ __launch_bounds__(256) void image_seg_counts_kernel(const int32_t* __restrict__ labels0, const int32_t* __restrict__ labels1, int FW,
                                                               const int32_t* __restrict__ regions, const int32_t* __restrict__ small,
                                                               const int32_t* __restrict__ yx, const int32_t* __restrict__ block_item,
                                                               const int32_t* __restrict__ block_first, int32_t* __restrict__ counts) {
  const int r = block_item[blockIdx.x];
  const ImgRegion g = img_region(regions, r);
  const long long p = (long long)(blockIdx.x - block_first[r]) * 256 + threadIdx.x;
  int s = 0;
  if (p < (long long)g.h * g.w) {
    int y, x;
    rhccq_row_col(p, g.w, y, x);
    if (img_in(g, labels0, labels1, FW, g.y0 + y, g.x0 + x)) s = img_seg(g, small, yx, y, x);
  }
  // neighbouring pixels mostly share a segment: one atomic per distinct id in the wave, not one per pixel
  unsigned long long todo = __ballot(s != 0);
  while (todo) {
    const int s0 = __shfl(s, __builtin_ctzll(todo), 64);
    const unsigned long long same = __ballot(s == s0) & todo;
    if ((int)(threadIdx.x & 63) == __builtin_ctzll(same)) atomicAdd(&counts[g.sid_off + s0], __popcll(same));
    todo &= ~same;
  }
}

// pairs[i] = (r, q): over the intersection of the two boxes, a pixel in both masks whose segment of q is painted (ids[q's sid] > 0)
__global__ __launch_bounds__(256) void image_overlap_kernel(const int32_t* __restrict__ labels0, const int32_t* __restrict__ labels1, int FW,
                                                            const int32_t* __restrict__ regions, const int32_t* __restrict__ small,
                                                            const int32_t* __restrict__ yx, const int32_t* __restrict__ ids,
                                                            const int32_t* __restrict__ pairs, const int32_t* __restrict__ block_item,
                                                            const int32_t* __restrict__ block_first, int32_t* __restrict__ hit) {
  const int i = block_item[blockIdx.x];
  const ImgRegion a = img_region(regions, pairs[2 * i]), b = img_region(regions, pairs[2 * i + 1]);
  const int y0 = max(a.y0, b.y0), x0 = max(a.x0, b.x0), y1 = min(a.y0 + a.h, b.y0 + b.h), x1 = min(a.x0 + a.w, b.x0 + b.w);
  if (y1 <= y0 || x1 <= x0) return;
  const long long p = (long long)(blockIdx.x - block_first[i]) * 256 + threadIdx.x;
  if (p >= (long long)(y1 - y0) * (x1 - x0)) return;
  int y, x;
  rhccq_row_col(p, x1 - x0, y, x);
  const int fy = y0 + y, fx = x0 + x;
  if (!img_in(a, labels0, labels1, FW, fy, fx) || !img_in(b, labels0, labels1, FW, fy, fx)) return;
  const int s = img_seg(b, small, yx, fy - b.y0, fx - b.x0);
  if (s && ids[b.sid_off + s] > 0) hit[i] = 1;              // (every writer stores the same value)
}

__global__ __launch_bounds__(256) void image_paint_kernel(const int32_t* __restrict__ labels0, const int32_t* __restrict__ labels1, int FH, int FW,
                                                          const int32_t* __restrict__ regions, const int32_t* __restrict__ small,
                                                          const int32_t* __restrict__ yx, const int32_t* __restrict__ ids,
                                                          const int32_t* __restrict__ block_item, const int32_t* __restrict__ block_first,
                                                          int32_t* __restrict__ layers) {
  const int r = block_item[blockIdx.x];
  const ImgRegion g = img_region(regions, r);
  if (g.layer < 0) return;
  const long long p = (long long)(blockIdx.x - block_first[r]) * 256 + threadIdx.x;
  if (p >= (long long)g.h * g.w) return;
  int y, x;
  rhccq_row_col(p, g.w, y, x);
  const int fy = g.y0 + y, fx = g.x0 + x;
  if (!img_in(g, labels0, labels1, FW, fy, fx)) return;
  const int s = img_seg(g, small, yx, y, x);
  if (!s) return;
  const int id = ids[g.sid_off + s];
  if (id > 0) layers[((size_t)g.layer * FH + fy) * FW + fx] = id;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

// counts (device int32[n_sid]) is zeroed here; block tables cover every region's h * w pixels
int rhccq_image_seg_counts(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                           const int32_t* small, const int32_t* yx, const int32_t* block_item, const int32_t* block_first, int64_t n_blocks,
                           int32_t* counts, int64_t n_sid) {
  if (!ctx || !labels0 || !labels1 || !regions || !small || !yx || !block_item || !block_first || !counts || H <= 0 || W <= 0 || n_blocks < 0 ||
      n_sid < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "image_seg_counts: bad argument");
  if (n_blocks > 0x7fffffffll) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "image_seg_counts: too many pixels");
  if (n_sid) RHCCQ_HIP(ctx, hipMemsetAsync(counts, 0, sizeof(int32_t) * (size_t)n_sid, ctx->stream));
  if (n_blocks == 0) return 0;
  hipLaunchKernelGGL(image_seg_counts_kernel, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, labels0, labels1, W, regions, small, yx, block_item,
                     block_first, counts);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// hit (device int32[n_pairs]) is zeroed here; block tables cover the intersection of every pair's two boxes
int rhccq_image_overlap(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                        const int32_t* small, const int32_t* yx, const int32_t* ids, const int32_t* pairs, int32_t n_pairs,
                        const int32_t* block_item, const int32_t* block_first, int64_t n_blocks, int32_t* hit) {
  if (!ctx || !labels0 || !labels1 || !regions || !small || !yx || !ids || !pairs || !block_item || !block_first || !hit || H <= 0 || W <= 0 ||
      n_pairs < 0 || n_blocks < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "image_overlap: bad argument");
  if (n_blocks > 0x7fffffffll) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "image_overlap: too many pixels");
  if (n_pairs) RHCCQ_HIP(ctx, hipMemsetAsync(hit, 0, sizeof(int32_t) * (size_t)n_pairs, ctx->stream));
  if (n_blocks == 0) return 0;
  hipLaunchKernelGGL(image_overlap_kernel, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, labels0, labels1, W, regions, small, yx, ids, pairs,
                     block_item, block_first, hit);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// layers (device int32[n_layers][H][W]) must be zeroed by the caller; regions with layer < 0 are skipped
int rhccq_image_paint(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                      const int32_t* small, const int32_t* yx, const int32_t* ids, const int32_t* block_item, const int32_t* block_first,
                      int64_t n_blocks, int32_t* layers) {
  if (!ctx || !labels0 || !labels1 || !regions || !small || !yx || !ids || !block_item || !block_first || !layers || H <= 0 || W <= 0 || n_blocks < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "image_paint: bad argument");
  if (n_blocks > 0x7fffffffll) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "image_paint: too many pixels");
  if (n_blocks == 0) return 0;
  hipLaunchKernelGGL(image_paint_kernel, dim3((unsigned)n_blocks), dim3(256), 0, ctx->stream, labels0, labels1, H, W, regions, small, yx, ids,
                     block_item, block_first, layers);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
