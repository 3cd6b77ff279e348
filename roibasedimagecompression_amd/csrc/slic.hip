// Masked SLIC superpixels: encoder/subregions/slic.py:41-104 enhanced_slic_with_texture ->
// skimage.segmentation.slic(image, n_segments, compactness=10, sigma=1, mask=...).  PARITY UNPINNED (scikit-image is absent
// from the build container): restated from its published algorithm (_slic_cython, _enforce_label_connectivity_cython).
//
//   slic_assign_kernel   one assignment sweep: every masked pixel takes the centroid with the smallest
//                        spatial / step^2 (+ colour) distance among those whose window [c - 2 step, c + 2 step] holds it,
//                        the first one on ties (float64, the same operations in the same order as the restatement, so
//                        the label maps are identical);
//   rhccq_slic_connectivity_host   the sequential connectivity enforcement (raster scan + breadth-first floods) as a
//                        native HOST routine: it is an inherently serial scan over <= 500 x 500 labels.
// The image SLIC sees is the reference's <= 500-pixel downscale, so this stage is small by construction; the centroid
// seeding (RandomState(123) + scipy kmeans2), the Gaussian and the centroid means (numpy bincount = raster-order sums,
// what skimage's loop computes) stay on the host (api/slic.py).
#include <vector>

#include "rhccq_common.h"

namespace rhccq {

__global__ __launch_bounds__(256) void slic_assign_kernel(const double* __restrict__ img /* [H][W][3], scaled by 1/compactness */,
                                                          const uint8_t* __restrict__ mask, const double* __restrict__ seg /* [K][5] = y, x, c0, c1, c2 */,
                                                          int H, int W, int K, double step, int ignore_color, int32_t* __restrict__ labels) {
  extern __shared__ double s_seg[];                      // [K][5] then the windows int[K][4]
  int* s_win = reinterpret_cast<int*>(s_seg + (size_t)K * 5);
  for (int i = threadIdx.x; i < K * 5; i += 256) s_seg[i] = seg[i];
  for (int k = threadIdx.x; k < K; k += 256) {
    const double cy = seg[k * 5], cx = seg[k * 5 + 1];
    s_win[k * 4 + 0] = (int)fmax(cy - 2 * step, 0.0);
    s_win[k * 4 + 1] = (int)fmin(cy + 2 * step + 1, (double)H);
    s_win[k * 4 + 2] = (int)fmax(cx - 2 * step, 0.0);
    s_win[k * 4 + 3] = (int)fmin(cx + 2 * step + 1, (double)W);
  }
  __syncthreads();
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long long)H * W) return;
  int best = 0;
  if (mask[p]) {
    int y, x;
    rhccq_row_col(p, W, y, x);
    const double inv = 1.0 / (step * step);
    const double i0 = img[p * 3], i1 = img[p * 3 + 1], i2 = img[p * 3 + 2];
    double bd = 1.7976931348623157e308;
    for (int k = 0; k < K; ++k) {
      if (y < s_win[k * 4] || y >= s_win[k * 4 + 1] || x < s_win[k * 4 + 2] || x >= s_win[k * 4 + 3]) continue;
      const double dy = s_seg[k * 5] - (double)y, dx = s_seg[k * 5 + 1] - (double)x;
      double d = (dy * dy + dx * dx) * inv;
      if (!ignore_color) {
        const double e0 = i0 - s_seg[k * 5 + 2], e1 = i1 - s_seg[k * 5 + 3], e2 = i2 - s_seg[k * 5 + 4];
        double dc = 0.0;
        dc = dc + e0 * e0;
        dc = dc + e1 * e1;
        dc = dc + e2 * e2;
        d = d + dc;
      }
      if (bd > d) { bd = d; best = k + 1; }
    }
  }
  labels[p] = best;
}

// ---- skimage.transform.resize of enhanced_slic_with_texture (slic.py:42-44,82,101): scipy.ndimage.gaussian_filter (anti-aliasing) and
// scipy.ndimage.zoom(order 0 / 1, mode 'mirror', grid_mode) restated operation for operation (float64, no contraction):
//   correlate1d with a symmetric kernel: t = x[c] w[0]; for j = R .. 1: t += (x[c - j] + x[c + j]) w[j]   (outermost pair first)
//   zoom, order 1: t = 0; for (dy, dx) in (0,0), (0,1), (1,0), (1,1): t += (x[y_dy][x_dx] * wy[dy]) * wx[dx]
// Coordinates, weights and mirrored indices are tiny per-axis tables computed on the host exactly as scipy computes them.
__global__ __launch_bounds__(256) void gauss1d_kernel(const double* __restrict__ in, long long outer, int len, long long inner,
                                                      const double* __restrict__ w /* [R + 1]: centre, then offsets 1 .. R */, int R,
                                                      double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= outer * len * inner) return;
  const long long k = i % inner, c = (i / inner) % len, o = i / (inner * len);
  const double* base = in + o * len * inner + k;
  auto at = [&](long long p) {                             // mode 'mirror': reflect about the centre of the edge samples
    if (len == 1) return base[0];
    const long long period = 2ll * len - 2;
    p %= period;
    if (p < 0) p += period;
    if (p >= len) p = period - p;
    return base[p * inner];
  };
  double t = at(c) * w[0];
  for (int j = R; j >= 1; --j) t += (at(c - j) + at(c + j)) * w[j];
  out[i] = t;
}

__global__ __launch_bounds__(256) void zoom_linear_kernel(const double* __restrict__ in, int W, int C, const int32_t* __restrict__ yi /* [2][oh] */,
                                                          const double* __restrict__ wy /* [2][oh] */, const int32_t* __restrict__ xi /* [2][ow] */,
                                                          const double* __restrict__ wx, int oh, int ow, double lo, double hi, double* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)oh * ow * C) return;
  const int ch = (int)(i % C), x = (int)((i / C) % ow), y = (int)(i / ((long long)C * ow));
  double t = 0.0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      double c = in[((long long)yi[dy * oh + y] * W + xi[dx * ow + x]) * C + ch];
      c *= wy[dy * oh + y];
      c *= wx[dx * ow + x];
      t += c;
    }
  out[i] = t < lo ? lo : (t > hi ? hi : t);                // resize(..., preserve_range) clips to the input's range
}

template <typename T>
__global__ __launch_bounds__(256) void zoom_nearest_kernel(const T* __restrict__ in, int W, int C, const int32_t* __restrict__ yi, const int32_t* __restrict__ xi,
                                                           int oh, int ow, T* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)oh * ow * C) return;
  const int ch = (int)(i % C), x = (int)((i / C) % ow), y = (int)(i / ((long long)C * ow));
  out[i] = in[((long long)yi[y] * W + xi[x]) * C + ch];
}


// ---- the 2 x max_iter sweeps of every region of a frame, with no read-back between them ---------------------------------------------
// Region r's small image is img[px_off ..][3], its mask mask[px_off ..], its centroids seg[seg_off .. + K][5] (y, x, c0, c1, c2);
// regions[r] = (px_off, H, W, K, seg_off) with px_off a multiple of 256, so that no workgroup of the assignment straddles two regions.
// labelled[r] records that a sweep gave some pixel a label; done[r] that _sweeps' loop has broken off for the region.
__global__ __launch_bounds__(256) void slic_assign_regions_kernel(const double* __restrict__ img, const uint8_t* __restrict__ mask,
                                                                  const double* __restrict__ seg, const int32_t* __restrict__ regions,
                                                                  const double* __restrict__ steps, const int32_t* __restrict__ block_region,
                                                                  const int32_t* __restrict__ block_first, int ignore_color,
                                                                  const int32_t* __restrict__ done, int32_t* __restrict__ labelled,
                                                                  int32_t* __restrict__ labels) {
  extern __shared__ double s_seg[];
  const int r = block_region[blockIdx.x];
  if (done[r]) return;                                     // (uniform over the workgroup)
  const int32_t* reg = regions + (size_t)r * 5;
  const long long off = reg[0];
  const int H = reg[1], W = reg[2], K = reg[3];
  const double step = steps[r];
  const double* sg = seg + (size_t)reg[4] * 5;
  int* s_win = reinterpret_cast<int*>(s_seg + (size_t)K * 5);
  for (int i = threadIdx.x; i < K * 5; i += 256) s_seg[i] = sg[i];
  for (int k = threadIdx.x; k < K; k += 256) {
    const double cy = sg[k * 5], cx = sg[k * 5 + 1];
    s_win[k * 4 + 0] = (int)fmax(cy - 2 * step, 0.0);
    s_win[k * 4 + 1] = (int)fmin(cy + 2 * step + 1, (double)H);
    s_win[k * 4 + 2] = (int)fmax(cx - 2 * step, 0.0);
    s_win[k * 4 + 3] = (int)fmin(cx + 2 * step + 1, (double)W);
  }
  __syncthreads();
  const long long p = (long long)(blockIdx.x - block_first[r]) * 256 + threadIdx.x;
  if (p >= (long long)H * W) return;
  int best = 0;
  if (mask[off + p]) {
    int y, x;
    rhccq_row_col(p, W, y, x);
    const double inv = 1.0 / (step * step);
    const double* px = img + (off + p) * 3;
    const double i0 = px[0], i1 = px[1], i2 = px[2];
    double bd = 1.7976931348623157e308;
    for (int k = 0; k < K; ++k) {
      if (y < s_win[k * 4] || y >= s_win[k * 4 + 1] || x < s_win[k * 4 + 2] || x >= s_win[k * 4 + 3]) continue;
      const double dy = s_seg[k * 5] - (double)y, dx = s_seg[k * 5 + 1] - (double)x;
      double d = (dy * dy + dx * dx) * inv;
      if (!ignore_color) {
        const double e0 = i0 - s_seg[k * 5 + 2], e1 = i1 - s_seg[k * 5 + 3], e2 = i2 - s_seg[k * 5 + 4];
        double dc = 0.0;
        dc = dc + e0 * e0;
        dc = dc + e1 * e1;
        dc = dc + e2 * e2;
        d = d + dc;
      }
      if (bd > d) { bd = d; best = k + 1; }
    }
  }
  labels[off + p] = best;
  if (best) labelled[r] = 1;                               // (every writer stores the same value)
}

__device__ __forceinline__ double slic_readlane(double v, int lane) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)b, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// The centroid means of _sweeps: np.bincount(label, weights) / count.  One wave per centroid g (of region seg_region[g]) walks the
// region's labels in raster order and adds the colour values of its pixels one after another in float64, as bincount does; the
// y / x sums are integers (exact in any order).  0 / 0 gives NaN, as in numpy.
constexpr int kSlicUnroll = 8;

__global__ __launch_bounds__(256) void slic_update_regions_kernel(const double* __restrict__ img, const int32_t* __restrict__ regions,
                                                                  const int32_t* __restrict__ seg_region, int n_seg, const int32_t* __restrict__ labels,
                                                                  const int32_t* __restrict__ labelled, int32_t* __restrict__ done,
                                                                  double* __restrict__ seg) {
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (g >= n_seg) return;                                  // (uniform over the wave)
  const int r = seg_region[g];
  if (done[r]) return;
  if (!labelled[r]) {                                      // _sweeps: `if not ok.any(): break`
    if (lane == 0) done[r] = 1;
    return;
  }
  const int32_t* reg = regions + (size_t)r * 5;
  const long long off = reg[0];
  const int W = reg[2], k1 = g - reg[4] + 1;
  const long long n = (long long)reg[1] * W;
  const int32_t* lab = labels + off;
  const double* im = img + off * 3;
  long long sy = 0, sx = 0, cnt = 0;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long base = 0; base < n; base += 64 * kSlicUnroll) {
    bool hit[kSlicUnroll];
#pragma unroll
    for (int u = 0; u < kSlicUnroll; ++u) {
      const long long p = base + u * 64 + lane;
      hit[u] = p < n && lab[p] == k1;
    }
#pragma unroll
    for (int u = 0; u < kSlicUnroll; ++u) {
      const long long p = base + u * 64 + lane;
      double c0 = 0.0, c1 = 0.0, c2 = 0.0;
      if (hit[u]) {
        c0 = im[p * 3];
        c1 = im[p * 3 + 1];
        c2 = im[p * 3 + 2];
        sy += p / W;
        sx += p % W;
        ++cnt;
      }
      unsigned long long m = __ballot(hit[u]);
      while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        s0 = s0 + slic_readlane(c0, b);
        s1 = s1 + slic_readlane(c1, b);
        s2 = s2 + slic_readlane(c2, b);
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sy += __shfl_xor(sy, o, 64);
    sx += __shfl_xor(sx, o, 64);
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) {
    const double c = (double)cnt;
    double* out = seg + (size_t)g * 5;
    out[0] = (double)sy / c;
    out[1] = (double)sx / c;
    out[2] = s0 / c;
    out[3] = s1 / c;
    out[4] = s2 / c;
  }
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int rhccq_slic_assign(rhccq_ctx* ctx, const double* img, const uint8_t* mask, const double* seg, int32_t H, int32_t W, int32_t K, double step,
                      int32_t ignore_color, int32_t* labels) {
  if (!ctx || !img || !mask || !seg || !labels || H <= 0 || W <= 0 || K <= 0 || !(step > 0.0)) return rhccq_fail(ctx, RHCCQ_E_ARG, "slic_assign: bad argument");
  const size_t lds = (size_t)K * (5 * sizeof(double) + 4 * sizeof(int));
  if (lds > 60 * 1024) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "slic_assign: more than ~1000 centroids");
  const unsigned grid = (unsigned)(((long long)H * W + 255) / 256);
  hipLaunchKernelGGL(slic_assign_kernel, dim3(grid), dim3(256), lds, ctx->stream, img, mask, seg, H, W, K, step, ignore_color, labels);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// HOST routine (plain pointers to host memory): skimage _enforce_label_connectivity_cython for a 2-D label map,
// start_label 1, 0 = outside the mask
int rhccq_slic_connectivity_host(const int32_t* labels_host, int32_t H, int32_t W, int32_t min_size, int32_t max_size, int32_t* out_host) {
  if (!labels_host || !out_host || H <= 0 || W <= 0 || max_size < 1) return RHCCQ_E_ARG;
  const long long n = (long long)H * W;
  for (long long i = 0; i < n; ++i) out_host[i] = 0;
  std::vector<int32_t> comp((size_t)max_size + 4);
  const int ddy[4] = {0, 0, 1, -1}, ddx[4] = {1, -1, 0, 0};
  int32_t cur = 1;
  for (int y = 0; y < H; ++y) {
    for (int x = 0; x < W; ++x) {
      const long long p = (long long)y * W + x;
      if (out_host[p] >= 1 || labels_host[p] == 0) continue;
      int32_t adjacent = 0;
      const int32_t label = labels_host[p];
      out_host[p] = cur;
      int size = 1, visited = 0;
      comp[0] = (int32_t)p;
      while (visited < size && size < max_size) {
        const int cy = comp[visited] / W, cx = comp[visited] % W;
        for (int i = 0; i < 4; ++i) {
          const int ny = cy + ddy[i], nx = cx + ddx[i];
          if (ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
          const long long q = (long long)ny * W + nx;
          if (labels_host[q] == label && out_host[q] == 0) {
            out_host[q] = cur;
            comp[size++] = (int32_t)q;
            if (size >= max_size) break;
          } else if (out_host[q] >= 1 && out_host[q] != cur) {
            adjacent = out_host[q];
          }
        }
        ++visited;
      }
      if (size < min_size) {
        for (int i = 0; i < size; ++i) out_host[comp[i]] = adjacent;
      } else {
        ++cur;
      }
    }
  }
  return 0;
}

int rhccq_gauss1d_f64(rhccq_ctx* ctx, const double* in, int64_t outer, int32_t len, int64_t inner, const double* weights, int32_t radius, double* out) {
  if (!ctx || !in || !weights || !out || in == out || outer <= 0 || len <= 0 || inner <= 0 || radius < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gauss1d_f64: bad argument");
  const long long n = (long long)outer * len * inner;
  hipLaunchKernelGGL(gauss1d_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, in, (long long)outer, len, (long long)inner, weights, radius, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_zoom_linear_f64(rhccq_ctx* ctx, const double* in, int32_t H, int32_t W, int32_t C, const int32_t* yi, const double* wy, const int32_t* xi,
                          const double* wx, int32_t oh, int32_t ow, double lo, double hi, double* out) {
  if (!ctx || !in || !yi || !wy || !xi || !wx || !out || H <= 0 || W <= 0 || C <= 0 || oh <= 0 || ow <= 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "zoom_linear_f64: bad argument");
  const long long n = (long long)oh * ow * C;
  hipLaunchKernelGGL(zoom_linear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, in, W, C, yi, wy, xi, wx, oh, ow, lo, hi, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_zoom_nearest(rhccq_ctx* ctx, const void* in, int32_t elem_bytes, int32_t H, int32_t W, int32_t C, const int32_t* yi, const int32_t* xi, int32_t oh,
                       int32_t ow, void* out) {
  if (!ctx || !in || !yi || !xi || !out || H <= 0 || W <= 0 || C <= 0 || oh <= 0 || ow <= 0 || (elem_bytes != 1 && elem_bytes != 4))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "zoom_nearest: bad argument");
  const long long n = (long long)oh * ow * C;
  const unsigned grid = (unsigned)((n + 255) / 256);
  if (elem_bytes == 1) hipLaunchKernelGGL(zoom_nearest_kernel<uint8_t>, dim3(grid), dim3(256), 0, ctx->stream, (const uint8_t*)in, W, C, yi, xi, oh, ow, (uint8_t*)out);
  else hipLaunchKernelGGL(zoom_nearest_kernel<int32_t>, dim3(grid), dim3(256), 0, ctx->stream, (const int32_t*)in, W, C, yi, xi, oh, ow, (int32_t*)out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int64_t rhccq_slic_regions_work_bytes(int32_t n_regions, int32_t max_iter) {
  if (n_regions < 0 || max_iter < 0) return -1;
  return (int64_t)sizeof(int32_t) * n_regions * (2 * (int64_t)max_iter + 2);
}

int rhccq_slic_sweeps_regions(rhccq_ctx* ctx, const double* img, const uint8_t* mask, double* seg, const int32_t* regions, const double* steps,
                              int32_t n_regions, int32_t max_k, const int32_t* block_region, const int32_t* block_first, int64_t n_blocks,
                              const int32_t* seg_region, int32_t n_seg, int32_t max_iter, void* work, int64_t work_bytes, int32_t* labels) {
  if (!ctx || !img || !mask || !seg || !regions || !steps || !block_region || !block_first || !seg_region || !work || !labels || n_regions <= 0 ||
      max_k <= 0 || n_blocks <= 0 || n_seg <= 0 || max_iter < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "slic_sweeps_regions: bad argument");
  if (work_bytes < rhccq_slic_regions_work_bytes(n_regions, max_iter)) return rhccq_fail(ctx, RHCCQ_E_ARG, "slic_sweeps_regions: workspace too small");
  if (n_blocks > 0x7fffffffll) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "slic_sweeps_regions: too many pixels");
  const size_t lds = (size_t)max_k * (5 * sizeof(double) + 4 * sizeof(int));
  if (lds > 60 * 1024) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "slic_sweeps_regions: more than ~1000 centroids in a region");
  int32_t* flags = static_cast<int32_t*>(work);            // [2][max_iter][R] labelled, then [2][R] done
  RHCCQ_HIP(ctx, hipMemsetAsync(flags, 0, (size_t)rhccq_slic_regions_work_bytes(n_regions, max_iter), ctx->stream));
  const unsigned upd_grid = (unsigned)((n_seg + 3) / 4);
  for (int call = 0; call < 2; ++call) {                   // slic_masked: colour ignored, then with colour
    int32_t* done = flags + (size_t)2 * max_iter * n_regions + (size_t)call * n_regions;
    for (int it = 0; it < max_iter; ++it) {
      int32_t* labelled = flags + ((size_t)call * max_iter + it) * n_regions;
      hipLaunchKernelGGL(slic_assign_regions_kernel, dim3((unsigned)n_blocks), dim3(256), lds, ctx->stream, img, mask, seg, regions, steps,
                         block_region, block_first, call == 0 ? 1 : 0, done, labelled, labels);
      RHCCQ_LAUNCH_CHECK(ctx);
      hipLaunchKernelGGL(slic_update_regions_kernel, dim3(upd_grid), dim3(256), 0, ctx->stream, img, regions, seg_region, n_seg, labels, labelled, done,
                         seg);
      RHCCQ_LAUNCH_CHECK(ctx);
    }
  }
  return 0;
}

}  // extern "C"
