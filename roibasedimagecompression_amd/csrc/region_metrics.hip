// Per-class quality metrics (EXTENSION, no reference counterpart: the reference's calculate_quality_metrics gives one figure for the
// whole picture): the error sums and the 7x7 SSIM of metrics.hip, kept apart by a class map (uint8 per pixel, e.g. the 0 / 1 region map
// of the ROI stage).  A class value >= n_classes (255, say) takes the pixel out of every row.
//
// Same arithmetic as metrics.hip: the error sums are integers (order independent), the SSIM window statistics are exact integer sums
// over the 49 pixels, only the final ratio is float64, and every workgroup writes its own partial sums (added in a fixed order inside
// the workgroup and, by the host, over the workgroups).
#include <type_traits>

#include "rhccq_common.h"

namespace rhccq {

constexpr int kMaxClasses = 16, kClassCols = 6;   // columns: sum d^2 R, G, B, sum |d|, max |d|, pixels

// four consecutive elements of p starting at element 4 * g: one vector load when p is aligned to it (wave uniform), else one load each
template <typename T>
__device__ __forceinline__ void load4(const T* __restrict__ p, long long g, bool aligned, unsigned v[4]) {
  if (aligned) {
    if constexpr (sizeof(T) == 1) {
      const uint32_t w = reinterpret_cast<const uint32_t*>(p)[g];
#pragma unroll
      for (int q = 0; q < 4; ++q) v[q] = (w >> (8 * q)) & 255u;
    } else if constexpr (sizeof(T) == 2) {
      const uint2 w = reinterpret_cast<const uint2*>(p)[g];
      v[0] = w.x & 0xFFFFu; v[1] = w.x >> 16; v[2] = w.y & 0xFFFFu; v[3] = w.y >> 16;
    } else {
      const uint4 w = reinterpret_cast<const uint4*>(p)[g];
      v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
    }
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = (unsigned)p[g * 4 + q];
  }
}

template <typename T>
__device__ __forceinline__ bool aligned4(const T* p) { return ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0; }

// One streaming pass, 4 pixels per lane and iteration as error_sums_kernel.  IdxT = void: b is the second image; otherwise b is the index
// plane and the second image is palette[idx] (an index past the palette reads entry 0, as rhccq_decode does), never written out.
// kTwo (n_classes <= 2, the ROI / non-ROI case): both rows live in registers, 32-bit inside one iteration (4 * 65025 per channel),
// 64-bit across iterations, shuffle reduction per wave.  Otherwise the rows live in LDS, one table per wave, LDS atomics per pixel.
// Either way a workgroup ends with at most 6 * n_classes global atomics.
template <typename IdxT, bool kTwo>
__global__ __launch_bounds__(256) void class_error_sums_kernel(const uint8_t* __restrict__ a, const void* __restrict__ b_or_idx,
                                                               const uint8_t* __restrict__ pal, long long pal_n,
                                                               const uint8_t* __restrict__ cls, long long n_px, int n_classes,
                                                               unsigned long long* __restrict__ sums /* [n_classes][6] */) {
  constexpr bool kIndexed = !std::is_same<IdxT, void>::value;
  constexpr int NC = kTwo ? 2 : kMaxClasses;
  __shared__ unsigned long long s_tab[4][NC][kClassCols];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (!kTwo) {
    for (int i = threadIdx.x; i < 4 * NC * kClassCols; i += 256) (&s_tab[0][0][0])[i] = 0ull;
    __syncthreads();
  }
  unsigned long long acc[2][kClassCols] = {};   // kTwo only
  const bool cls_al = aligned4(cls);

  // one pixel: channel values of both images and its class
  auto pixel = [&](const int va[3], const int vb[3], unsigned c, unsigned it[2][kClassCols]) {
    unsigned d[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) d[ch] = (unsigned)abs(va[ch] - vb[ch]);
    const unsigned ab = d[0] + d[1] + d[2], mx = max(d[0], max(d[1], d[2]));
    if constexpr (kTwo) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const bool in = c == (unsigned)k && k < n_classes;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) it[k][ch] += in ? d[ch] * d[ch] : 0u;
        it[k][3] += in ? ab : 0u;
        it[k][4] = max(it[k][4], in ? mx : 0u);
        it[k][5] += in ? 1u : 0u;
      }
    } else if (c < (unsigned)n_classes) {
      unsigned long long* row = s_tab[w][c];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
        if (d[ch]) atomicAdd(&row[ch], (unsigned long long)(d[ch] * d[ch]));
      if (ab) {
        atomicAdd(&row[3], (unsigned long long)ab);
        atomicMax(&row[4], (unsigned long long)mx);
      }
      atomicAdd(&row[5], 1ull);
    }
  };
  auto fold = [&](unsigned it[2][kClassCols]) {
    if constexpr (kTwo) {
#pragma unroll
      for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int q = 0; q < kClassCols; ++q) acc[k][q] = q == 4 ? max(acc[k][q], (unsigned long long)it[k][q]) : acc[k][q] + it[k][q];
    }
  };
  auto second = [&](long long p, int vb[3]) {           // pixel p of the second image, scalar form (tail)
    if constexpr (kIndexed) {
      long long v = (long long)reinterpret_cast<const IdxT*>(b_or_idx)[p];
      if (v >= pal_n) v = 0;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) vb[ch] = pal[v * 3 + ch];
    } else {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) vb[ch] = reinterpret_cast<const uint8_t*>(b_or_idx)[p * 3 + ch];
    }
  };

  const long long n4 = n_px >> 2;
  const uint32_t* a4 = reinterpret_cast<const uint32_t*>(a);
  bool idx_al = false;
  if constexpr (kIndexed) idx_al = aligned4(reinterpret_cast<const IdxT*>(b_or_idx));
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    uint32_t wa[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) wa[j] = a4[i * 3 + j];
    unsigned c4[4];
    load4(cls, i, cls_al, c4);
    int vb[4][3];
    if constexpr (kIndexed) {
      unsigned v4[4];
      load4(reinterpret_cast<const IdxT*>(b_or_idx), i, idx_al, v4);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const long long v = (long long)v4[q] >= pal_n ? 0 : (long long)v4[q];
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) vb[q][ch] = pal[v * 3 + ch];
      }
    } else {
      const uint32_t* b4 = reinterpret_cast<const uint32_t*>(b_or_idx);
      uint32_t wb[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) wb[j] = b4[i * 3 + j];
#pragma unroll
      for (int j = 0; j < 12; ++j) vb[j / 3][j % 3] = (wb[j >> 2] >> ((j & 3) * 8)) & 255;
    }
    unsigned it[2][kClassCols] = {};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      int va[3];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) { const int j = q * 3 + ch; va[ch] = (wa[j >> 2] >> ((j & 3) * 8)) & 255; }
      pixel(va, vb[q], c4[q], it);
    }
    fold(it);
  }
  if (blockIdx.x == 0 && threadIdx.x < (n_px & 3)) {       // tail pixels
    const long long p = (n4 << 2) + threadIdx.x;
    int va[3], vb[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) va[ch] = a[p * 3 + ch];
    second(p, vb);
    unsigned it[2][kClassCols] = {};
    pixel(va, vb, (unsigned)cls[p], it);
    fold(it);
  }
  if constexpr (kTwo) {
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
      for (int q = 0; q < kClassCols; ++q) {
        unsigned long long v = acc[k][q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
          const unsigned long long t = __shfl_down(v, o, 64);
          v = q == 4 ? (t > v ? t : v) : v + t;
        }
        if (lane == 0) s_tab[w][k][q] = v;
      }
  }
  __syncthreads();
  if ((int)threadIdx.x < n_classes * kClassCols) {          // n_classes <= NC: checked by the host entry
    const int k = threadIdx.x / kClassCols, q = threadIdx.x % kClassCols;
    unsigned long long t = s_tab[0][k][q];
    for (int i = 1; i < 4; ++i) t = q == 4 ? (s_tab[i][k][q] > t ? s_tab[i][k][q] : t) : t + s_tab[i][k][q];
    if (t) {                                                // at most 6 * n_classes atomics per workgroup
      if (q == 4) atomicMax(&sums[threadIdx.x], t); else atomicAdd(&sums[threadIdx.x], t);
    }
  }
}

// ---- SSIM, 7x7 uniform window, per class of the window's centre pixel -------------------------------------------------------------
constexpr int kCsTile = 32, kCsWin = 7, kCsPad = 3, kCsIn = kCsTile + kCsWin - 1;   // the tiling of ssim7_kernel
constexpr int kCsPerLane = kCsTile * kCsTile / 256;                                 // 4 window centres per lane

// one workgroup: a 32x32 tile of window centres.  Every lane parks the S of its 4 centres and their classes in LDS slots of its own
// (registers would hold 12 doubles through the window loop and halve the occupancy); the sums of a class are then formed in a fixed
// order (lane's centres, shuffle tree, waves 0..3), so a result does not depend on scheduling.
__global__ __launch_bounds__(256) void class_ssim7_kernel(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b,
                                                          const uint8_t* __restrict__ cls, int H, int W, int n_classes,
                                                          double* __restrict__ partial /* [tiles][n_classes][4] */) {
  __shared__ uint8_t sa[3][kCsIn][kCsIn + 2], sb[3][kCsIn][kCsIn + 2];
  __shared__ double s_S[kCsPerLane][3][256];
  __shared__ int s_k[kCsPerLane][256];
  __shared__ double red[kMaxClasses][4][4];
  const int oy0 = blockIdx.y * kCsTile, ox0 = blockIdx.x * kCsTile;       // interior coordinates: centre = (+3, +3)
  const int IH = H - 2 * kCsPad, IW = W - 2 * kCsPad;
  for (int i = threadIdx.x; i < kCsIn * kCsIn; i += 256) {
    const int r = i / kCsIn, c = i % kCsIn;
    const int y = min(oy0 + r, H - 1), x = min(ox0 + c, W - 1);           // clamped reads feed only discarded outputs
    const long long p = ((long long)y * W + x) * 3;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { sa[ch][r][c] = a[p + ch]; sb[ch][r][c] = b[p + ch]; }
  }
  __syncthreads();
  const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
  const double cov_norm = 49.0 / 48.0;
#pragma unroll 1
  for (int j = 0; j < kCsPerLane; ++j) {
    const int o = threadIdx.x + j * 256;
    const int r = o / kCsTile, c = o % kCsTile;
    const bool inside = oy0 + r < IH && ox0 + c < IW;
    s_k[j][threadIdx.x] = inside ? (int)cls[(long long)(oy0 + r + kCsPad) * W + (ox0 + c + kCsPad)] : -1;
    if (!inside) continue;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;     // 49 * 65025 < 2^22
      for (int dy = 0; dy < kCsWin; ++dy)
#pragma unroll
        for (int dx = 0; dx < kCsWin; ++dx) {
          const int x = sa[ch][r + dy][c + dx], y = sb[ch][r + dy][c + dx];
          sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
        }
      const double ux = (double)sx / 49.0, uy = (double)sy / 49.0;
      const double uxx = (double)sxx / 49.0, uyy = (double)syy / 49.0, uxy = (double)sxy / 49.0;
      const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
      const double A1 = 2.0 * ux * uy + C1, A2 = 2.0 * vxy + C2, B1 = ux * ux + uy * uy + C1, B2 = vx + vy + C2;
      s_S[j][ch][threadIdx.x] = (A1 * A2) / (B1 * B2);
    }
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = 0; k < n_classes; ++k) {                  // wave uniform
    double v[4] = {0.0, 0.0, 0.0, 0.0};                   // sum of S per channel, window centres
#pragma unroll
    for (int j = 0; j < kCsPerLane; ++j) {
      if (s_k[j][threadIdx.x] != k) continue;             // (a slot is read by the lane that wrote it: no barrier)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) v[ch] += s_S[j][ch][threadIdx.x];
      v[3] += 1.0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[q] += __shfl_down(v[q], o, 64);
      if (lane == 0) red[k][q][w] = v[q];
    }
  }
  __syncthreads();
  if ((int)threadIdx.x < n_classes * 4) {
    const int k = threadIdx.x >> 2, q = threadIdx.x & 3;
    const size_t tile = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
    partial[(tile * n_classes + k) * 4 + q] = ((red[k][q][0] + red[k][q][1]) + red[k][q][2]) + red[k][q][3];
  }
}

template <typename IdxT>
static int launch_class_error_sums(rhccq_ctx* ctx, const uint8_t* a, const void* b_or_idx, const uint8_t* pal, int64_t pal_n,
                                   const uint8_t* cls, int64_t n_pixels, int32_t n_classes, uint64_t* sums) {
  long long blocks = (n_pixels / 4 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  if (n_classes <= 2)
    hipLaunchKernelGGL((class_error_sums_kernel<IdxT, true>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a, b_or_idx, pal,
                       (long long)pal_n, cls, (long long)n_pixels, (int)n_classes, (unsigned long long*)sums);
  else
    hipLaunchKernelGGL((class_error_sums_kernel<IdxT, false>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, a, b_or_idx, pal,
                       (long long)pal_n, cls, (long long)n_pixels, (int)n_classes, (unsigned long long*)sums);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int rhccq_class_error_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* cls, int64_t n_pixels, int32_t n_classes,
                           uint64_t* sums) {
  if (!ctx || !a || !b || !cls || !sums || n_pixels < 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums: bad argument");
  if (n_classes < 1 || n_classes > kMaxClasses) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums: n_classes must be 1..16");
  if (((uintptr_t)a & 3) || ((uintptr_t)b & 3)) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums: images must be 4-byte aligned");
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)n_classes * kClassCols * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  return launch_class_error_sums<void>(ctx, a, b, nullptr, 0, cls, n_pixels, n_classes, sums);
}

int rhccq_class_error_sums_indexed(rhccq_ctx* ctx, const uint8_t* a, const void* idx, int32_t idx_elem_bytes, const uint8_t* palette,
                                   int64_t pal_n, const uint8_t* cls, int64_t n_pixels, int32_t n_classes, uint64_t* sums) {
  if (!ctx || !a || !idx || !palette || !cls || !sums || n_pixels < 0 || pal_n <= 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums_indexed: bad argument");
  if (n_classes < 1 || n_classes > kMaxClasses) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums_indexed: n_classes must be 1..16");
  if ((uintptr_t)a & 3) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums_indexed: the image must be 4-byte aligned");
  if (idx_elem_bytes != 1 && idx_elem_bytes != 2 && idx_elem_bytes != 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums_indexed: idx_elem_bytes must be 1, 2 or 4");
  if ((uintptr_t)idx & (uintptr_t)(idx_elem_bytes - 1)) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_error_sums_indexed: misaligned indices");
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)n_classes * kClassCols * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  switch (idx_elem_bytes) {
    case 1: return launch_class_error_sums<uint8_t>(ctx, a, idx, palette, pal_n, cls, n_pixels, n_classes, sums);
    case 2: return launch_class_error_sums<uint16_t>(ctx, a, idx, palette, pal_n, cls, n_pixels, n_classes, sums);
    default: return launch_class_error_sums<uint32_t>(ctx, a, idx, palette, pal_n, cls, n_pixels, n_classes, sums);
  }
}

int64_t rhccq_class_ssim7_blocks(int32_t H, int32_t W) {
  if (H < 7 || W < 7) return 0;
  const int64_t by = (H - 6 + kCsTile - 1) / kCsTile, bx = (W - 6 + kCsTile - 1) / kCsTile;
  return by * bx;
}

int rhccq_class_ssim7_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* cls, int32_t H, int32_t W, int32_t n_classes,
                           double* partial, int64_t n_blocks) {
  if (!ctx || !a || !b || !cls || !partial) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_ssim7: bad argument");
  if (n_classes < 1 || n_classes > kMaxClasses) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_ssim7: n_classes must be 1..16");
  if (H < 7 || W < 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "class_ssim7: win_size exceeds image extent");
  if (n_blocks != rhccq_class_ssim7_blocks(H, W))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "class_ssim7: partial must hold rhccq_class_ssim7_blocks(H, W) x n_classes x 4 doubles");
  const dim3 grid((unsigned)((W - 6 + kCsTile - 1) / kCsTile), (unsigned)((H - 6 + kCsTile - 1) / kCsTile));
  hipLaunchKernelGGL(class_ssim7_kernel, grid, dim3(256), 0, ctx->stream, a, b, cls, (int)H, (int)W, (int)n_classes, partial);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
