// The step functions, the tap-table builder, the constants and the argument tests of the image resampling (EXTENSION, no reference
// counterpart), shared by the kernels and the host form of resize.hip.  The definition (include/rhccq.h "resize") is Pillow's separable
// convolution resampling for 8-bit images restated in exact integers: an axis of n samples resized to m has, per output sample, a window
// [first, first + count) of input samples and count int32 weights of 22 fraction bits; a pass computes
//     out = clamp((2^21 + sum_t weight_t * in[first + t]) >> 22, 0, 255)
// per byte.  The real weights are computed ONCE per axis, on the host, in double (resize_taps below); everything that touches pixels reads
// only the integer table, so the device form, the host form and the tests' reference agree bit for bit, in any order of accumulation.
//
// Arithmetic.  The builder refuses a table with 255 * sum|weight| + 2^21 >= 2^31 for any output sample, so an int32 accumulator never
// overflows, in whatever order the taps arrive.  It also reports the largest |weight|: below 2^23 (every table of the four filters seen so
// far) the kernels multiply with the 24-bit full-rate multiply-add, else with the 32-bit one.
#pragma once
#include <math.h>

#include <vector>

#include "rhccq_common.h"

namespace rhccq {

constexpr int kResizeFilters = 4;                // box, triangle, cubic, lanczos
constexpr int kResizeMaxSide = 65535;            // H, W, OH, OW
constexpr int kResizeMaxBatch = 65535;           // images of a call: a grid dimension
constexpr int kResizeBits = 22;                  // fraction bits of a weight
constexpr int kResizeTileRows = 64;              // rows pass: image rows of a workgroup, a lane a row
constexpr int kResizeRunCols = 32;               // rows pass: output columns of a workgroup, its 4 waves take them in turn
constexpr int kResizeWaves = 4;
constexpr int kResizeColsPerWave = kResizeRunCols / kResizeWaves;
constexpr int kResizeTileDwords = 128;           // rows pass: dwords of a row the LDS tile holds at a time (512 bytes)
constexpr int kResizeTilePitch = kResizeTileDwords + 1;   // odd: 64 lanes on 64 rows, same column, hit distinct banks
constexpr int kResizeOutPitch = kResizeRunCols + 1;       // dwords of a row of the LDS output tile (32 columns x 4 bytes at most), odd
constexpr int kResizeBlock = 256;                // threads of every workgroup
constexpr int kResizeStripBytes = 1024;          // columns pass: bytes of a row a workgroup owns, a lane a dword
constexpr int kResizeRunRows = 4;                // columns pass: output rows a workgroup walks
static_assert(kResizeRunCols * 4 % 16 == 0 && kResizeRunCols % kResizeWaves == 0, "a run of columns starts on a dword for every C");

// one output sample of an axis: the window and where its weights start in the axis's weight array
struct ResizeTap { int32_t first, count, woff, pad; };

// ---- the step functions: one multiply-add of a tap, and the rounding of a finished sum ----
template <bool kMul24>
__host__ __device__ __forceinline__ int32_t resize_mac(int32_t acc, int32_t w, uint32_t byte) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (kMul24) return acc + __mul24(w, (int32_t)byte);                                    // (|w| < 2^23: the full-rate multiply)
#endif
  return acc + w * (int32_t)byte;
}
__host__ __device__ __forceinline__ uint32_t resize_round(int32_t acc) {
  const int32_t v = (acc + (1 << (kResizeBits - 1))) >> kResizeBits;                       // arithmetic shift
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}
__host__ __device__ __forceinline__ int64_t resize_pitch(int64_t row_bytes) { return (row_bytes + 3) & ~(int64_t)3; }

// ---- the filters and the tap table (host only, double; -ffp-contract=off: every operation rounds on its own) ----
static inline double resize_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * 3.14159265358979323846;
  return sin(x) / x;
}
static inline double resize_filter(int f, double x) {
  switch (f) {
    case 0: return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0;
    case 1:
      if (x < 0.0) x = -x;
      return x < 1.0 ? 1.0 - x : 0.0;
    case 2: {
      const double a = -0.5;
      if (x < 0.0) x = -x;
      if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
      if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
      return 0.0;
    }
    default: return (-3.0 <= x && x < 3.0) ? resize_sinc(x) * resize_sinc(x / 3.0) : 0.0;
  }
}
static inline double resize_filter_support(int f) { return f == 0 ? 0.5 : f == 1 ? 1.0 : f == 2 ? 2.0 : 3.0; }

static inline bool resize_side_ok(int64_t v) { return v >= 1 && v <= kResizeMaxSide; }

// weights an axis has at most, whatever the filter: a window is at most 2 * 3 * max(n_in / n_out, 1) + 2 samples and at most n_in
static inline int64_t resize_weights_bound(int64_t n_in, int64_t n_out) {
  const int64_t window = 6 * ((n_in + n_out - 1) / n_out) + 2;
  return n_out * (window < n_in ? window : n_in);
}

// the table of one axis.  taps: n_out entries (or NULL), weights: appended (or NULL: only counted).  Returns 0 or RHCCQ_E_LIMIT (a sample
// whose sum could leave int32); *n_weights the weights of the axis, *max_abs the largest |weight|
static inline int resize_taps(int32_t n_in, int32_t n_out, int filter, ResizeTap* taps, std::vector<int32_t>* weights, int64_t* n_weights,
                              int32_t* max_abs) {
  const double scale = (double)n_in / (double)n_out, fs = scale < 1.0 ? 1.0 : scale, support = resize_filter_support(filter) * fs;
  std::vector<double> w;
  int64_t total = 0;
  int32_t most = 0;
  for (int32_t i = 0; i < n_out; ++i) {
    const double centre = (i + 0.5) * scale;
    int32_t lo = (int32_t)(centre - support + 0.5), hi = (int32_t)(centre + support + 0.5);
    if (lo < 0) lo = 0;
    if (hi > n_in) hi = n_in;
    const int32_t n = hi > lo ? hi - lo : 0;
    w.resize((size_t)n);
    double sum = 0.0;
    for (int32_t t = 0; t < n; ++t) {
      w[(size_t)t] = resize_filter(filter, (t + lo - centre + 0.5) / fs);
      sum += w[(size_t)t];
    }
    int64_t mass = 0;
    for (int32_t t = 0; t < n; ++t) {
      double v = w[(size_t)t];
      if (sum != 0.0) v /= sum;
      const int32_t q = v < 0.0 ? (int32_t)(-0.5 + v * 4194304.0) : (int32_t)(0.5 + v * 4194304.0);
      const int32_t a = q < 0 ? -q : q;
      mass += a;
      if (a > most) most = a;
      if (weights) weights->push_back(q);
    }
    if (255 * mass + (1 << (kResizeBits - 1)) >= ((int64_t)1 << 31)) return RHCCQ_E_LIMIT;
    if (taps) taps[i] = {lo, n, (int32_t)total, 0};
    total += n;
  }
  *n_weights = total;
  if (max_abs) *max_abs = most;
  return 0;
}

static inline int resize_fail(rhccq_ctx* ctx, int code, const char* msg) { return rhccq_fail(ctx, code, msg); }

// the argument tests both forms share, before any work
static inline int resize_check(rhccq_ctx* ctx, const void* src, int32_t B, int32_t H, int32_t W, int32_t C, const void* dst, int32_t OH, int32_t OW,
                               int32_t filter) {
  if (!src || !dst) return resize_fail(ctx, RHCCQ_E_ARG, "resize: a null image");
  if (B < 1) return resize_fail(ctx, RHCCQ_E_ARG, "resize: at least one image is expected");
  if (!resize_side_ok(H) || !resize_side_ok(W) || !resize_side_ok(OH) || !resize_side_ok(OW))
    return resize_fail(ctx, RHCCQ_E_ARG, "resize: H, W, OH and OW must be 1..65535");
  if (C != 1 && C != 3 && C != 4) return resize_fail(ctx, RHCCQ_E_ARG, "resize: C must be 1, 3 or 4");
  if (filter < 0 || filter >= kResizeFilters) return resize_fail(ctx, RHCCQ_E_ARG, "resize: the filter must be 0..3 (box, triangle, cubic, lanczos)");
  if (B > kResizeMaxBatch) return resize_fail(ctx, RHCCQ_E_LIMIT, "resize: at most 65535 images a call");
  return 0;
}

// the workspace of the device form: the intermediate [B][H][pitch(OW C)], then per axis the taps and the weights at their bound
struct ResizeLayout { int64_t mid, xtab, xw, ytab, yw, total; };
static inline ResizeLayout resize_layout(int64_t B, int64_t H, int64_t W, int64_t C, int64_t OH, int64_t OW) {
  ResizeLayout l;
  l.mid = 0;
  l.xtab = align256(B * H * resize_pitch(OW * C));
  l.xw = l.xtab + align256(OW * (int64_t)sizeof(ResizeTap));
  l.ytab = l.xw + align256(resize_weights_bound(W, OW) * 4);
  l.yw = l.ytab + align256(OH * (int64_t)sizeof(ResizeTap));
  l.total = l.yw + align256(resize_weights_bound(H, OH) * 4);
  return l;
}

// ---- one pass of the host form: `lines` lines of `n_out` samples of `step` bytes... the rows pass has stride C between samples and C
// bytes a sample; the columns pass has stride row_bytes between samples and row_bytes bytes a sample ----
static inline void resize_pass_host(const uint8_t* in, uint8_t* out, int64_t lines, int64_t in_line, int64_t out_line, int64_t stride, int64_t width,
                                    int32_t n_out, const ResizeTap* taps, const int32_t* weights) {
  for (int64_t l = 0; l < lines; ++l)
    for (int32_t i = 0; i < n_out; ++i) {
      const ResizeTap e = taps[i];
      for (int64_t c = 0; c < width; ++c) {
        int32_t acc = 0;
        for (int32_t t = 0; t < e.count; ++t) acc = resize_mac<false>(acc, weights[e.woff + t], in[l * in_line + (int64_t)(e.first + t) * stride + c]);
        out[l * out_line + (int64_t)i * stride + c] = (uint8_t)resize_round(acc);
      }
    }
}

}  // namespace rhccq
