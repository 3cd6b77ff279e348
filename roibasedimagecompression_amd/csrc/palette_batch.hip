// The palette build path for a batch of images (EXTENSION, no reference counterpart): rhccq_palette_cells, rhccq_palette_build,
// rhccq_palette_remap, rhccq_palette_refine and rhccq_palette_pattern over B images that lie back to back in one buffer, every image's result bit for bit what
// the single-image call gives for that image alone.  The definition is in include/rhccq.h.
//
// Why: the split chain is one workgroup for about 2 ms at 256 colours (7 to 8 us a step) and cannot be shortened, but B chains on B
// workgroups take what one takes; and a loop of single calls pays every launch and every host synchronisation once per image.
//
// How.  Every kernel here is the single-image kernel's body (palette_build.h, palette_remap.h, palette_refine.h; the remap and the
// refinement both search through the one remap_search) called with the pointers of one image: blockIdx.y (the chain: blockIdx.x) is
// the image, blockIdx.x the workgroup among the gridDim.x that share it.
// An image's pixels are [px_off[b], px_off[b + 1]) of the concatenation and its chunks count from its own first pixel, so a workgroup
// never holds pixels of two images and the sums of an image are formed by the same additions as in the single call (integers: any
// order gives the same result anyway).  The grid's x extent is sized on the host by the largest image (px_off_host); the kernels read
// the same offsets from px_off_dev, and a workgroup whose image has fewer chunks than its blockIdx.x returns at once.  The rows in use
// per image (k_rows) are read on the device, which is what lets the remap and the refinement follow the build without a host
// synchronisation.  No workgroup waits for another: no flags, no spinning, no cooperative launch, no grid sized to what is resident;
// stream order between launches is the only synchronisation, and a batch larger than the card queues.
#include "palette_build.h"
#include "palette_pattern.h"
#include "palette_refine.h"

#include <vector>

namespace rhccq {

constexpr int kBatchMaxImages = 65535;                // gridDim.y

// image b of the concatenation: its first pixel and its pixel count
__device__ __forceinline__ long long batch_image(const long long* __restrict__ px_off, int b, long long* n_px) {
  const long long first = px_off[b];
  *n_px = px_off[b + 1] - first;
  return first;
}

__global__ __launch_bounds__(kCellsBlock) void palette_cells_batch_kernel(const uint8_t* __restrict__ rgb, const long long* __restrict__ px_off,
                                                                          const uint8_t* __restrict__ cls, int n_classes, CellsWeights wt,
                                                                          unsigned long long* __restrict__ cells) {
  const int b = blockIdx.y;
  long long n_px;
  const long long first = batch_image(px_off, b, &n_px);
  if ((long long)blockIdx.x * kCellsChunk >= n_px) return;                             // (block uniform) more workgroups than this image has chunks
  palette_cells_body(rgb + first * 3, n_px, n_classes > 0 ? cls + first : nullptr, n_classes, wt, cells + (size_t)b * 4 * kBuildCells, blockIdx.x,
                     gridDim.x);
}

__global__ __launch_bounds__(256) void palette_build_prefix_b_batch_kernel(const unsigned long long* __restrict__ cells, unsigned long long* __restrict__ T) {
  build_prefix_b_body(cells + (size_t)blockIdx.y * 4 * kBuildCells, T + (size_t)blockIdx.y * kBuildTabEntries * 4, blockIdx.x * 256 + threadIdx.x);
}
__global__ __launch_bounds__(256) void palette_build_prefix_batch_kernel(unsigned long long* __restrict__ T, int outer_stride, int step) {
  build_prefix_body(T + (size_t)blockIdx.y * kBuildTabEntries * 4, outer_stride, step, blockIdx.x * 256 + threadIdx.x);
}

// workgroup b runs the chain of table b; an empty or oversized table leaves its error code in k_out[b] and zeroes its own rows only
__global__ __launch_bounds__(kBuildBlock) void palette_build_chain_batch_kernel(const BuildSum* __restrict__ T, int K_target, uint8_t* __restrict__ pal_out,
                                                                                unsigned long long* __restrict__ counts_out,
                                                                                uint8_t* __restrict__ boxes_out, int32_t* __restrict__ splits,
                                                                                int32_t* __restrict__ k_out) {
  const size_t b = blockIdx.x;
  build_chain_body(T + b * kBuildTabEntries, K_target, pal_out + b * K_target * 3, counts_out + b * K_target,
                   boxes_out ? boxes_out + b * K_target * 6 : nullptr, splits ? splits + b * (size_t)(K_target - 1) * 3 : nullptr, k_out + b);
}

// rows in use of image b: what the build left in k_out[b]; never more than the stride (a caller's own k_rows may not reach behind it)
__device__ __forceinline__ int batch_rows(const int32_t* __restrict__ k_rows, int b, int K_stride) {
  const int k = k_rows[b];
  return k < K_stride ? k : K_stride;
}

template <typename IdxT>
__global__ __launch_bounds__(kRemapBlock) void palette_remap_batch_kernel(const uint8_t* __restrict__ rgb, const long long* __restrict__ px_off,
                                                                          const uint8_t* __restrict__ pal, int K_stride,
                                                                          const int32_t* __restrict__ k_rows, const uint8_t* __restrict__ cls,
                                                                          int n_classes, IdxT* __restrict__ idx_out,
                                                                          unsigned long long* __restrict__ sums) {
  const int b = blockIdx.y;
  long long n_px;
  const long long first = batch_image(px_off, b, &n_px);
  if ((long long)blockIdx.x * kRemapChunk >= n_px) return;                             // (block uniform)
  const int K = batch_rows(k_rows, b, K_stride);
  if (K < 1) {                                                                         // no palette (a build's error code): index 0, zero sums
    for (long long c = (long long)blockIdx.x * kRemapChunk; c < n_px; c += (long long)gridDim.x * kRemapChunk)
      for (long long p = c + threadIdx.x; p < min(c + kRemapChunk, n_px); p += kRemapBlock) idx_out[first + p] = (IdxT)0;
    return;
  }
  remap_body<IdxT>(rgb + first * 3, n_px, pal + (size_t)b * K_stride * 3, K, n_classes > 0 ? cls + first : nullptr, n_classes, idx_out + first,
                   sums + (size_t)b * (n_classes + 1) * 2, blockIdx.x, gridDim.x);
}

// the pattern dither of image b: its own width gives (y, x) from its own linear pixel index
template <int kSize, typename IdxT>
__global__ __launch_bounds__(kPatternBlock) void palette_pattern_batch_kernel(const uint8_t* __restrict__ rgb, const long long* __restrict__ px_off,
                                                                              const int32_t* __restrict__ widths, const uint8_t* __restrict__ pal,
                                                                              int K_stride, const int32_t* __restrict__ k_rows,
                                                                              const uint8_t* __restrict__ cls, int n_classes, PatternStrength strength,
                                                                              IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums) {
  extern __shared__ uint4 s_dyn[];
  const int b = blockIdx.y;
  long long n_px;
  const long long first = batch_image(px_off, b, &n_px);
  if ((long long)blockIdx.x * pattern_chunk(kSize) >= n_px) return;                    // (block uniform)
  const int K = batch_rows(k_rows, b, K_stride);
  if (K < 1) {                                                                         // no palette (a build's error code): index 0, zero sums
    for (long long c = (long long)blockIdx.x * pattern_chunk(kSize); c < n_px; c += (long long)gridDim.x * pattern_chunk(kSize))
      for (long long p = c + threadIdx.x; p < min(c + pattern_chunk(kSize), n_px); p += kPatternBlock) idx_out[first + p] = (IdxT)0;
    return;
  }
  pattern_body<kSize, IdxT>(rgb + first * 3, n_px, max(widths[b], 1), pal + (size_t)b * K_stride * 3, K, n_classes > 0 ? cls + first : nullptr, n_classes,
                            strength, idx_out + first, sums + (size_t)b * (n_classes + 1) * 3, blockIdx.x, gridDim.x, s_dyn);
}

template <bool kLds>
__global__ __launch_bounds__(kRemapBlock) void palette_refine_assign_batch_kernel(const uint8_t* __restrict__ rgb, const long long* __restrict__ px_off,
                                                                                  const uint8_t* __restrict__ pal, int K_stride,
                                                                                  const int32_t* __restrict__ k_rows,
                                                                                  const uint8_t* __restrict__ cls, int n_classes, RefineWeights wt,
                                                                                  int iter, int max_iter, unsigned long long* __restrict__ history,
                                                                                  unsigned long long* __restrict__ acc) {
  extern __shared__ unsigned long long s_acc[];                                         // kLds: [K_stride][4]
  const int b = blockIdx.y;
  long long n_px;
  const long long first = batch_image(px_off, b, &n_px);
  if ((long long)blockIdx.x * kRemapChunk >= n_px) return;                             // (block uniform)
  const int K = batch_rows(k_rows, b, K_stride);
  if (K < 1) return;
  refine_assign_body<kLds>(rgb + first * 3, n_px, pal + (size_t)b * K_stride * 3, K, n_classes > 0 ? cls + first : nullptr, n_classes, wt, iter,
                           history + (size_t)b * max_iter * 2, acc + (size_t)b * K_stride * 4, s_acc, blockIdx.x, gridDim.x);
}

// an image without pixels or without rows runs no iteration: its n_iter stays 0 and its history zero, as in the single call
__global__ __launch_bounds__(256) void palette_refine_update_batch_kernel(uint8_t* __restrict__ pal, int K_stride, const int32_t* __restrict__ k_rows,
                                                                          const long long* __restrict__ px_off, int iter, int max_iter,
                                                                          unsigned long long* __restrict__ history,
                                                                          unsigned long long* __restrict__ acc, int32_t* __restrict__ n_iter) {
  const int b = blockIdx.y;
  long long n_px;
  batch_image(px_off, b, &n_px);
  const int K = batch_rows(k_rows, b, K_stride);
  if (n_px == 0 || (int)blockIdx.x * 256 >= K) return;                                 // (block uniform; K < 1 included)
  refine_update_body(pal + (size_t)b * K_stride * 3, K, iter, history + (size_t)b * max_iter * 2, acc + (size_t)b * K_stride * 4, n_iter + b,
                     blockIdx.x);
}

// B and the offsets: px_off[0] == 0, non-decreasing -> the pixels of the largest image through *max_px
static int batch_check(rhccq_ctx* ctx, const char* what, int32_t B, const int64_t* px_off, int64_t* max_px) {
  static const char* const kMsg[] = {": B >= 1 is required", ": null px_off", ": px_off must start at 0 and never decrease", ": at most 65535 images"};
  int bad = -1;
  if (B < 1) bad = 0;
  else if (!px_off) bad = 1;
  else if (px_off[0] != 0) bad = 2;
  int64_t top = 0;
  for (int b = 0; bad < 0 && b < B; ++b) {
    if (px_off[b + 1] < px_off[b]) bad = 2;
    else if (px_off[b + 1] - px_off[b] > top) top = px_off[b + 1] - px_off[b];
  }
  if (bad < 0 && B > kBatchMaxImages) bad = 3;
  if (bad >= 0) {
    if (ctx) ctx->err = std::string(what) + kMsg[bad];
    return bad == 3 ? RHCCQ_E_LIMIT : RHCCQ_E_ARG;
  }
  *max_px = top;
  return 0;
}

// workgroups per image: the cap of the single call shared among the images, at least one, never more than the largest image has chunks
static unsigned batch_grid_x(int64_t max_px, long long chunk, long long cap, int B) {
  const long long chunks = (max_px + chunk - 1) / chunk, share = cap / B < 1 ? 1 : cap / B;
  return (unsigned)(chunks < share ? chunks : share);
}

static int build_batch_check(rhccq_ctx* ctx, const void* cells, int32_t B, int32_t K_target, const void* palette_out, const void* counts_out,
                             const void* splits, const void* k_out) {
  if (B < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build_batch: B >= 1 is required");
  if (const int rc = build_check(ctx, cells, K_target, palette_out, counts_out, splits, k_out)) return rc;
  if (B > kBatchMaxImages) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build_batch: at most 65535 images");
  return 0;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int64_t rhccq_palette_build_batch_bytes(int32_t B) { return B < 1 ? 0 : (int64_t)B * rhccq_palette_build_bytes(); }
int64_t rhccq_palette_refine_batch_bytes(int32_t B, int32_t K_stride) { return B < 1 ? 0 : (int64_t)B * rhccq_palette_refine_bytes(K_stride); }

// ---- cells ------------------------------------------------------------------------------------------------------------------------------
int rhccq_palette_cells_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B, const uint8_t* cls,
                              int32_t n_classes, const int32_t* weights_host, uint64_t* cells) {
  if (!ctx) return RHCCQ_E_ARG;
  int64_t max_px = 0;
  if (const int rc = batch_check(ctx, "palette_cells_batch", B, px_off_host, &max_px)) return rc;
  if (!px_off_dev) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells_batch: null px_off_dev");
  CellsWeights wt = {};
  if (const int rc = cells_check(ctx, rgb, max_px, cls, n_classes, weights_host, cells, &wt)) return rc;      // (the limit holds per image)
  RHCCQ_HIP(ctx, hipMemsetAsync(cells, 0, (size_t)B * kBuildCells * 4 * sizeof(uint64_t), ctx->stream));
  if (max_px == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const dim3 grid(batch_grid_x(max_px, kCellsChunk, (long long)ctx->compute_units * 4, B), (unsigned)B);
  hipLaunchKernelGGL(palette_cells_batch_kernel, grid, dim3(kCellsBlock), 0, ctx->stream, rgb, (const long long*)px_off_dev, cls, (int)n_classes, wt,
                     (unsigned long long*)cells);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_cells_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, const uint8_t* cls, int32_t n_classes, const int32_t* weights,
                                   uint64_t* cells) {
  int64_t max_px = 0;
  if (const int rc = batch_check(nullptr, "palette_cells_batch", B, px_off, &max_px)) return rc;
  CellsWeights wt = {};
  if (const int rc = cells_check(nullptr, rgb, max_px, cls, n_classes, weights, cells, &wt)) return rc;
  for (int b = 0; b < B; ++b)
    if (const int rc = rhccq_palette_cells_host(rgb + px_off[b] * 3, px_off[b + 1] - px_off[b], cls ? cls + px_off[b] : nullptr, n_classes, weights, 0,
                                                cells + (size_t)b * 4 * kBuildCells))
      return rc;
  return 0;
}

// ---- build ------------------------------------------------------------------------------------------------------------------------------
int rhccq_palette_build_batch(rhccq_ctx* ctx, const uint64_t* cells, int32_t B, int32_t K_target, void* work, int64_t work_bytes, uint8_t* palette_out,
                              uint64_t* counts_out, uint8_t* boxes_out, int32_t* splits, int32_t* k_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build_batch: null argument");
  if (const int rc = build_batch_check(ctx, cells, B, K_target, palette_out, counts_out, splits, k_out)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build_batch: misaligned workspace");
  if (K_target > kBuildMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build_batch: more rows than rhccq_palette_build_max_rows()");
  if (work_bytes < rhccq_palette_build_batch_bytes(B))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build_batch: the workspace is smaller than rhccq_palette_build_batch_bytes(B)");
  unsigned long long* T = (unsigned long long*)work;
  const dim3 grid((unsigned)((kBuildTab * kBuildTab * 4 + 255) / 256), (unsigned)B), block(256);
  hipLaunchKernelGGL(palette_build_prefix_b_batch_kernel, grid, block, 0, ctx->stream, (const unsigned long long*)cells, T);
  hipLaunchKernelGGL(palette_build_prefix_batch_kernel, grid, block, 0, ctx->stream, T, kBuildTab * kBuildTab * 4, kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_prefix_batch_kernel, grid, block, 0, ctx->stream, T, kBuildTab * 4, kBuildTab * kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_chain_batch_kernel, dim3((unsigned)B), dim3(kBuildBlock), 0, ctx->stream, (const BuildSum*)work, (int)K_target,
                     palette_out, (unsigned long long*)counts_out, boxes_out, splits, k_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_build_batch_host(const uint64_t* cells, int32_t B, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out, uint8_t* boxes_out,
                                   int32_t* splits, int32_t* k_out) {
  if (const int rc = build_batch_check(nullptr, cells, B, K_target, palette_out, counts_out, splits, k_out)) return rc;
  const size_t K = (size_t)K_target;
  for (size_t b = 0; b < (size_t)B; ++b) {
    uint8_t* pal = palette_out + b * K * 3;
    uint8_t* boxes = boxes_out ? boxes_out + b * K * 6 : nullptr;
    int32_t* sp = splits ? splits + b * (K - 1) * 3 : nullptr;
    const int rc = rhccq_palette_build_host(cells + b * 4 * kBuildCells, K_target, pal, counts_out + b * K, boxes, sp, k_out + b);
    if (rc == 0) continue;
    // what only the table shows goes where the device form puts it: the code in k_out[b], zero rows, -1 throughout splits
    for (size_t j = 0; j < K * 3; ++j) pal[j] = 0;
    for (size_t j = 0; j < K; ++j) counts_out[b * K + j] = 0;
    if (boxes)
      for (size_t j = 0; j < K * 6; ++j) boxes[j] = 0;
    if (sp)
      for (size_t j = 0; j < (K - 1) * 3; ++j) sp[j] = -1;
    k_out[b] = rc;
  }
  return 0;
}

// ---- remap ------------------------------------------------------------------------------------------------------------------------------
int rhccq_palette_remap_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B,
                              const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, void* idx_out,
                              int32_t idx_elem_bytes, uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  int64_t max_px = 0;
  if (const int rc = batch_check(ctx, "palette_remap_batch", B, px_off_host, &max_px)) return rc;
  if (!px_off_dev || !k_rows) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap_batch: null px_off_dev or k_rows");
  if ((uintptr_t)k_rows & 3) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_remap_batch: misaligned k_rows");
  if (const int rc = remap_check(ctx, rgb, px_off_host[B], palettes, K_stride, cls, n_classes, idx_out, idx_elem_bytes, sums)) return rc;
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)B * (n_classes + 1) * 2 * sizeof(uint64_t), ctx->stream));
  if (max_px == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const dim3 grid(batch_grid_x(max_px, kRemapChunk, (long long)ctx->compute_units * 8, B), (unsigned)B), block(kRemapBlock);
  const long long* off = (const long long*)px_off_dev;
  unsigned long long* s = (unsigned long long*)sums;
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    hipLaunchKernelGGL(palette_remap_batch_kernel<T>, grid, block, 0, ctx->stream, rgb, off, palettes, (int)K_stride, k_rows, cls, (int)n_classes,
                       (T*)idx_out, s);
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_remap_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows,
                                   const uint8_t* cls, int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  int64_t max_px = 0;
  if (const int rc = batch_check(nullptr, "palette_remap_batch", B, px_off, &max_px)) return rc;
  if (!k_rows || ((uintptr_t)k_rows & 3)) return RHCCQ_E_ARG;
  if (const int rc = remap_check(nullptr, rgb, px_off[B], palettes, K_stride, cls, n_classes, idx_out, idx_elem_bytes, sums)) return rc;
  for (int b = 0; b < B; ++b) {
    const int64_t first = px_off[b], n = px_off[b + 1] - first;
    uint8_t* idx = (uint8_t*)idx_out + first * idx_elem_bytes;
    uint64_t* s = sums + (size_t)b * (n_classes + 1) * 2;
    const int K = k_rows[b] < K_stride ? k_rows[b] : K_stride;
    if (K < 1) {
      for (int64_t j = 0; j < n * idx_elem_bytes; ++j) idx[j] = 0;
      for (int j = 0; j < (n_classes + 1) * 2; ++j) s[j] = 0;
      continue;
    }
    if (const int rc = rhccq_palette_remap_host(rgb + first * 3, n, palettes + (size_t)b * K_stride * 3, K, cls ? cls + first : nullptr, n_classes, idx,
                                                idx_elem_bytes, s))
      return rc;
  }
  return 0;
}

// ---- pattern ----------------------------------------------------------------------------------------------------------------------------
// what both forms test behind batch_check: the single call's arguments over the whole concatenation (H = 1, W = its pixels would overflow
// int32: the tests are rows_check's, spelt for a pixel count), then every image's width
static int pattern_batch_check(rhccq_ctx* ctx, const void* rgb, const int64_t* px_off, const int32_t* widths, int32_t B, const void* palettes,
                               int32_t K_stride, const void* k_rows, const void* cls, int32_t n_classes, const uint32_t* strength, int32_t size,
                               const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  const char* const what = "palette_pattern_batch";
  if (!widths || !k_rows) return remap_fail(ctx, RHCCQ_E_ARG, what, ": null widths or k_rows");
  if ((uintptr_t)k_rows & 3) return remap_fail(ctx, RHCCQ_E_ARG, what, ": misaligned k_rows");
  if (const int rc = pattern_check(ctx, what, rgb, 0, 0, palettes, K_stride, cls, n_classes, strength, size, idx_out, idx_elem_bytes, sums)) return rc;
  for (int b = 0; b < B; ++b) {
    const int64_t n = px_off[b + 1] - px_off[b];
    if (widths[b] < 0 || (n > 0 && (widths[b] < 1 || n % widths[b] != 0 || n / widths[b] > 0x7FFFFFFF)))
      return remap_fail(ctx, RHCCQ_E_ARG, what, ": an image's width must divide its pixels into at most 2^31 - 1 rows");
  }
  return 0;
}

int rhccq_palette_pattern_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, const int32_t* widths_host,
                                const int32_t* widths_dev, int32_t B, const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows, const uint8_t* cls,
                                int32_t n_classes, const uint32_t* strength_host, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  int64_t max_px = 0;
  if (const int rc = batch_check(ctx, "palette_pattern_batch", B, px_off_host, &max_px)) return rc;
  if (!px_off_dev || !widths_dev || ((uintptr_t)widths_dev & 3)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_pattern_batch: null px_off_dev or widths_dev, or misaligned widths_dev");
  if (const int rc = pattern_batch_check(ctx, rgb, px_off_host, widths_host, B, palettes, K_stride, k_rows, cls, n_classes, strength_host, size, idx_out,
                                         idx_elem_bytes, sums))
    return rc;
  if (K_stride > kPatternMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_pattern_batch: the device form holds at most 4096 colours");
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)B * (n_classes + 1) * 3 * sizeof(uint64_t), ctx->stream));
  if (max_px == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  PatternStrength strength{};
  for (int i = 0; i <= n_classes; ++i) strength.v[i] = strength_host[i];
  const dim3 grid(batch_grid_x(max_px, pattern_chunk(size), (long long)ctx->compute_units * 16, B), (unsigned)B), block(kPatternBlock);
  const size_t lds = pattern_lds_bytes(K_stride);
  const long long* off = (const long long*)px_off_dev;
  unsigned long long* s = (unsigned long long*)sums;
  index_dispatch(idx_elem_bytes, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
#define RHCCQ_PATTERN_BATCH_CASE(N_) \
  case N_: hipLaunchKernelGGL((palette_pattern_batch_kernel<N_, T>), grid, block, lds, ctx->stream, rgb, off, widths_dev, palettes, (int)K_stride, k_rows, \
                              cls, (int)n_classes, strength, (T*)idx_out, s); break;
    switch (size) {
      RHCCQ_PATTERN_BATCH_CASE(2) RHCCQ_PATTERN_BATCH_CASE(4)
      default: hipLaunchKernelGGL((palette_pattern_batch_kernel<8, T>), grid, block, lds, ctx->stream, rgb, off, widths_dev, palettes, (int)K_stride,
                                  k_rows, cls, (int)n_classes, strength, (T*)idx_out, s);
    }
#undef RHCCQ_PATTERN_BATCH_CASE
  });
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_pattern_batch_host(const uint8_t* rgb, const int64_t* px_off, const int32_t* widths, int32_t B, const uint8_t* palettes, int32_t K_stride,
                                     const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, const uint32_t* strength, int32_t size, void* idx_out,
                                     int32_t idx_elem_bytes, uint64_t* sums) {
  int64_t max_px = 0;
  if (const int rc = batch_check(nullptr, "palette_pattern_batch", B, px_off, &max_px)) return rc;
  if (const int rc = pattern_batch_check(nullptr, rgb, px_off, widths, B, palettes, K_stride, k_rows, cls, n_classes, strength, size, idx_out,
                                         idx_elem_bytes, sums))
    return rc;
  for (int b = 0; b < B; ++b) {
    const int64_t first = px_off[b], n = px_off[b + 1] - first;
    uint8_t* idx = (uint8_t*)idx_out + first * idx_elem_bytes;
    uint64_t* s = sums + (size_t)b * (n_classes + 1) * 3;
    const int K = k_rows[b] < K_stride ? k_rows[b] : K_stride;
    if (K < 1 || n == 0) {
      for (int64_t j = 0; j < n * idx_elem_bytes; ++j) idx[j] = 0;
      for (int j = 0; j < (n_classes + 1) * 3; ++j) s[j] = 0;
      continue;
    }
    if (const int rc = rhccq_palette_pattern_host(rgb + first * 3, (int32_t)(n / widths[b]), widths[b], palettes + (size_t)b * K_stride * 3, K,
                                                  cls ? cls + first : nullptr, n_classes, strength, size, idx, idx_elem_bytes, s))
      return rc;
  }
  return 0;
}

// ---- refine -----------------------------------------------------------------------------------------------------------------------------
int rhccq_palette_refine_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B, uint8_t* palettes,
                               int32_t K_stride, const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, const int32_t* weights_host,
                               int32_t max_iter, void* work, int64_t work_bytes, uint64_t* history, int32_t* n_iter) {
  if (!ctx) return RHCCQ_E_ARG;
  int64_t max_px = 0;
  if (const int rc = batch_check(ctx, "palette_refine_batch", B, px_off_host, &max_px)) return rc;
  if (!px_off_dev || !k_rows || !work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine_batch: null px_off_dev, k_rows or workspace");
  if ((uintptr_t)k_rows & 3) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine_batch: misaligned k_rows");
  RefineWeights wt = {};
  if (const int rc = refine_check(ctx, rgb, px_off_host[B], palettes, K_stride, cls, n_classes, weights_host, max_iter, history, n_iter, &wt)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine_batch: misaligned workspace");
  const int64_t need = rhccq_palette_refine_batch_bytes(B, K_stride);
  if (work_bytes < need) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_refine_batch: the workspace is smaller than rhccq_palette_refine_batch_bytes(B, K_stride)");
  RHCCQ_HIP(ctx, hipMemsetAsync(history, 0, (size_t)B * max_iter * 2 * sizeof(uint64_t), ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(n_iter, 0, (size_t)B * sizeof(int32_t), ctx->stream));
  if (max_px == 0) return 0;
  RHCCQ_HIP(ctx, hipMemsetAsync(work, 0, (size_t)need, ctx->stream));
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const long long cap = ctx->opt_refine_max_blocks > 0 ? ctx->opt_refine_max_blocks : (long long)ctx->compute_units * 8;
  const dim3 grid(batch_grid_x(max_px, kRemapChunk, cap, B), (unsigned)B), block(kRemapBlock);
  const dim3 ugrid((unsigned)((K_stride + 255) / 256), (unsigned)B);
  // one choice for the batch: accumulators in LDS when the stride (so every image's rows) fits, else in the workspace for every image
  const int lds_rows = ctx->opt_refine_lds_rows < 0 ? kRefineLdsRows : ctx->opt_refine_lds_rows;
  const bool lds = K_stride <= lds_rows;
  const long long* off = (const long long*)px_off_dev;
  unsigned long long* acc = (unsigned long long*)work;
  unsigned long long* hist = (unsigned long long*)history;
  for (int it = 0; it < max_iter; ++it) {
    if (lds)
      hipLaunchKernelGGL(palette_refine_assign_batch_kernel<true>, grid, block, (size_t)K_stride * 4 * sizeof(uint64_t), ctx->stream, rgb, off,
                         (const uint8_t*)palettes, (int)K_stride, k_rows, cls, (int)n_classes, wt, it, (int)max_iter, hist, acc);
    else
      hipLaunchKernelGGL(palette_refine_assign_batch_kernel<false>, grid, block, 0, ctx->stream, rgb, off, (const uint8_t*)palettes, (int)K_stride, k_rows,
                         cls, (int)n_classes, wt, it, (int)max_iter, hist, acc);
    hipLaunchKernelGGL(palette_refine_update_batch_kernel, ugrid, dim3(256), 0, ctx->stream, palettes, (int)K_stride, k_rows, off, it, (int)max_iter, hist,
                       acc, n_iter);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_refine_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, uint8_t* palettes, int32_t K_stride, const int32_t* k_rows,
                                    const uint8_t* cls, int32_t n_classes, const int32_t* weights, int32_t max_iter, uint64_t* history, int32_t* n_iter) {
  int64_t max_px = 0;
  if (const int rc = batch_check(nullptr, "palette_refine_batch", B, px_off, &max_px)) return rc;
  if (!k_rows || ((uintptr_t)k_rows & 3)) return RHCCQ_E_ARG;
  RefineWeights wt = {};
  if (const int rc = refine_check(nullptr, rgb, px_off[B], palettes, K_stride, cls, n_classes, weights, max_iter, history, n_iter, &wt)) return rc;
  for (int b = 0; b < B; ++b) {
    const int64_t first = px_off[b], n = px_off[b + 1] - first;
    uint64_t* h = history + (size_t)b * max_iter * 2;
    const int K = k_rows[b] < K_stride ? k_rows[b] : K_stride;
    if (K < 1) {
      for (int j = 0; j < max_iter * 2; ++j) h[j] = 0;
      n_iter[b] = 0;
      continue;
    }
    if (const int rc = rhccq_palette_refine_host(rgb + first * 3, n, palettes + (size_t)b * K_stride * 3, K, cls ? cls + first : nullptr, n_classes, weights,
                                                 max_iter, h, n_iter + b))
      return rc;
  }
  return 0;
}

}  // extern "C"
