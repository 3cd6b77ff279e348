// Image resampling (EXTENSION, no reference counterpart): separable convolution resampling of uint8 images with the box, triangle, cubic
// (Keys, a = -0.5) and Lanczos-3 filters, the filter stretched by the scale factor when shrinking, in exact integers.  The definition, the
// tap table and the step functions are in resize.h; include/rhccq.h pins the rounding.
//
// Two launches a call, a batch of B equal-sized images as grid.z, a uint8 intermediate [B][H][pitch] between them (pitch = OW C rounded
// up to 4, so every row of it starts on a dword).  No matrix instruction fits: the weights need 23 bits and the operator is a narrow band.
//
// rows pass (width)    Neighbouring outputs have different windows and weights, so a lane takes an image ROW and the wave walks output
//   columns: window and weights are wave-uniform (scalar loads, weights in SGPRs, one uniform loop, no divergence).  A workgroup of 4 waves
//   takes 64 rows by a run of 32 output columns.  The input span of the run is walked in chunks of 512 bytes a row, staged in LDS at a
//   pitch of 129 dwords (64 lanes on 64 rows hit distinct banks) by 16-byte loads where source and row length allow, else by pairs of
//   dwords joined with v_alignbyte; a wave holds the sums of its 8 columns x C channels in registers across the chunks, so a window of any
//   length (600 -> 3, 65535 -> 1) costs only more chunks.  Results go to an LDS output tile and leave as dword stores along the rows.
//   LDS: 64 x 129 x 4 + 64 x 33 x 4 = 41 472 bytes a workgroup.
// columns pass (height)    Every byte column is independent, so channels vanish: a lane owns one dword of a row, a workgroup a 1 KiB
//   strip of the row and a run of 4 output rows.  Per output row window and weights are wave-uniform; a tap is one coalesced dword load,
//   four multiply-adds against an SGPR weight; the four results leave as one dword (bytes where the output row does not start on a dword,
//   and in a row's last, partial dword).  Consecutive output rows share most of their window: that reuse is left to L2.
// An axis whose size does not change is a copy (resize_copy_kernel) through the same intermediate.
#include "resize.h"

#include <array>
#include <deque>
#include <memory>
#include <mutex>

namespace rhccq {

// dword q of a buffer of `total` bytes that starts on a dword; bytes past its end read as 0 and are never touched
__device__ __forceinline__ uint32_t resize_load_dword(const uint8_t* __restrict__ base, long long q, long long total) {
  if (4 * q + 4 <= total) return reinterpret_cast<const uint32_t*>(base)[q];
  uint32_t v = 0u;
  for (int k = 0; k < 4; ++k)
    if (4 * q + k < total) v |= (uint32_t)base[4 * q + k] << (8 * k);
  return v;
}

template <int C, bool kMul24>
__global__ __launch_bounds__(kResizeBlock) void resize_rows_kernel(const uint8_t* __restrict__ src, long long total, int H, int W, int OW,
                                                                   const ResizeTap* __restrict__ taps, const int32_t* __restrict__ weights,
                                                                   uint32_t* __restrict__ mid, int pitch_dwords, int aligned16) {
  __shared__ uint32_t s_in[kResizeTileRows * kResizeTilePitch];
  __shared__ uint32_t s_out[kResizeTileRows * kResizeOutPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ox0 = blockIdx.x * kResizeRunCols, ox1 = min(ox0 + kResizeRunCols, OW);
  const int y0 = blockIdx.y * kResizeTileRows;
  const long long b = blockIdx.z, row_bytes = (long long)W * C;
  const ResizeTap last = taps[ox1 - 1];
  const int span_hi = last.first + last.count;
  int32_t acc[kResizeColsPerWave][C];
#pragma unroll
  for (int j = 0; j < kResizeColsPerWave; ++j)
#pragma unroll
    for (int c = 0; c < C; ++c) acc[j][c] = 0;
  const uint8_t* s_row = reinterpret_cast<const uint8_t*>(s_in + lane * kResizeTilePitch);

  for (int pb = taps[ox0].first; pb < span_hi;) {                                      // chunks of the run's input span: pixels [pb, pe)
    const int tb0 = (int)(((long long)pb * C) & ~15ll);                                // the chunk's first byte in a row
    const int pe = min(span_hi, (tb0 + kResizeTileDwords * 4) / C);                    // pixels that lie in the tile with all their bytes
    if (aligned16) {                                                                   // (uniform) every row, and tb0 in it, starts on 16 bytes
      for (int i = tid; i < kResizeTileRows * (kResizeTileDwords / 4); i += kResizeBlock) {
        const int r = i / (kResizeTileDwords / 4), c = i % (kResizeTileDwords / 4), y = y0 + r;
        const long long o = tb0 + 16ll * c;
        uint4 v = {0u, 0u, 0u, 0u};
        if (y < H && o < row_bytes) v = *reinterpret_cast<const uint4*>(src + (b * H + y) * row_bytes + o);
        uint32_t* d = s_in + r * kResizeTilePitch + 4 * c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    } else {
      for (int i = tid; i < kResizeTileRows * kResizeTileDwords; i += kResizeBlock) {
        const int r = i / kResizeTileDwords, d = i % kResizeTileDwords, y = y0 + r;
        const long long o = tb0 + 4ll * d;
        uint32_t v = 0u;
        if (y < H && o < row_bytes) {
          const long long g = (b * H + y) * row_bytes + o, q = g >> 2;
          const uint32_t s = (uint32_t)(g & 3), lo = resize_load_dword(src, q, total);
          v = s ? __builtin_amdgcn_alignbyte(resize_load_dword(src, q + 1, total), lo, s) : lo;
        }
        s_in[r * kResizeTilePitch + d] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kResizeColsPerWave; ++j) {
      const int col = ox0 + wave + j * kResizeWaves;                                   // (wave uniform)
      if (col < ox1) {
        const ResizeTap e = taps[col];
        const int ta = max(e.first, pb), te = min(e.first + e.count, pe);
        const int32_t* w = weights + e.woff - e.first;
#pragma unroll 4
        for (int t = ta; t < te; ++t) {
          const int32_t wt = w[t];
          const int o = t * C - tb0;
          if (C == 4) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(s_row + o);
#pragma unroll
            for (int c = 0; c < C; ++c) acc[j][c] = resize_mac<kMul24>(acc[j][c], wt, (v >> (8 * c)) & 255u);
          } else {
#pragma unroll
            for (int c = 0; c < C; ++c) acc[j][c] = resize_mac<kMul24>(acc[j][c], wt, s_row[o + c]);
          }
        }
      }
    }
    __syncthreads();
    pb = pe;
  }

  uint8_t* o_row = reinterpret_cast<uint8_t*>(s_out + lane * kResizeOutPitch);
#pragma unroll
  for (int j = 0; j < kResizeColsPerWave; ++j) {
    const int col = wave + j * kResizeWaves;
    if (ox0 + col < ox1) {
#pragma unroll
      for (int c = 0; c < C; ++c) o_row[col * C + c] = (uint8_t)resize_round(acc[j][c]);
    }
  }
  __syncthreads();
  const int nd = ((ox1 - ox0) * C + 3) >> 2;                                            // dwords of the run in a row: the last may end in the pitch's padding
  for (int i = tid; i < kResizeTileRows * kResizeRunCols; i += kResizeBlock) {
    const int r = i / kResizeRunCols, d = i % kResizeRunCols, y = y0 + r;
    if (y < H && d < nd) mid[(b * H + y) * pitch_dwords + (ox0 * C >> 2) + d] = s_out[r * kResizeOutPitch + d];
  }
}

template <bool kMul24>
__global__ __launch_bounds__(kResizeBlock) void resize_cols_kernel(const uint32_t* __restrict__ mid, int H, int pitch_dwords, int row_bytes, int OH,
                                                                   const ResizeTap* __restrict__ taps, const int32_t* __restrict__ weights,
                                                                   uint8_t* __restrict__ dst) {
  const int d = blockIdx.x * kResizeBlock + threadIdx.x;                               // the lane's dword of a row
  if (d >= pitch_dwords) return;
  const long long b = blockIdx.z;
  const uint32_t* in = mid + b * H * pitch_dwords + d;
  const int oy0 = blockIdx.y * kResizeRunRows, oy1 = min(oy0 + kResizeRunRows, OH);
  const int valid = min(4, row_bytes - 4 * d);                                         // bytes of the dword that lie in the row
  for (int oy = oy0; oy < oy1; ++oy) {                                                 // (uniform)
    const ResizeTap e = taps[oy];
    const int32_t* w = weights + e.woff;
    const uint32_t* p = in + (long long)e.first * pitch_dwords;
    int32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll 4
    for (int t = 0; t < e.count; ++t) {
      const uint32_t v = p[(long long)t * pitch_dwords];
      const int32_t wt = w[t];
      a0 = resize_mac<kMul24>(a0, wt, v & 255u);
      a1 = resize_mac<kMul24>(a1, wt, (v >> 8) & 255u);
      a2 = resize_mac<kMul24>(a2, wt, (v >> 16) & 255u);
      a3 = resize_mac<kMul24>(a3, wt, v >> 24);
    }
    // The four bytes are made opaque before they are joined: left to itself the compiler fuses shift, clamp and join of a0 and a1 into
    // gfx950's v_ashr_pk_u8_i32 written over one of its own sources and takes the result's upper half for zero; the card keeps the
    // source's upper half there, which then lands in bytes 2 and 3 (seen on the device: byte 2 came out as itself | (a0 + 2^21) >> 16).
    uint32_t r0 = resize_round(a0), r1 = resize_round(a1), r2 = resize_round(a2), r3 = resize_round(a3);
    asm volatile("" : "+v"(r0), "+v"(r1), "+v"(r2), "+v"(r3));
    const uint32_t out = r0 | r1 << 8 | r2 << 16 | r3 << 24;
    uint8_t* q = dst + (b * OH + oy) * row_bytes + 4ll * d;
    if (valid == 4 && (reinterpret_cast<uintptr_t>(q) & 3u) == 0) {
      *reinterpret_cast<uint32_t*>(q) = out;
    } else {
      for (int k = 0; k < valid; ++k) q[k] = (uint8_t)(out >> (8 * k));
    }
  }
}

// rows of row_bytes bytes from one pitch to another: [grid.z images][rows][pitch] on both sides; a lane four bytes
__global__ __launch_bounds__(kResizeBlock) void resize_copy_kernel(const uint8_t* __restrict__ src, long long src_pitch, uint8_t* __restrict__ dst,
                                                                   long long dst_pitch, int row_bytes, int rows) {
  const int o = 4 * (blockIdx.x * kResizeBlock + threadIdx.x);
  if (o >= row_bytes) return;
  const long long line = (long long)blockIdx.z * rows + blockIdx.y;
  const uint8_t* s = src + line * src_pitch + o;
  uint8_t* d = dst + line * dst_pitch + o;
  const int n = min(4, row_bytes - o);
  if (n == 4 && ((reinterpret_cast<uintptr_t>(s) | reinterpret_cast<uintptr_t>(d)) & 3u) == 0) {
    *reinterpret_cast<uint32_t*>(d) = *reinterpret_cast<const uint32_t*>(s);
  } else {
    for (int k = 0; k < n; ++k) d[k] = s[k];
  }
}

struct ResizeAxis {
  std::vector<ResizeTap> taps;
  std::vector<int32_t> weights;
  int32_t max_abs = 0;
};
// the table of an axis, kept for the process: a Lanczos table of a 4K side is some 10^4 calls of sin, more host time than both launches
// take on the card, and a sequence asks for the same two axes call after call.  The last 16 axes are kept (first in, first out).
static std::shared_ptr<const ResizeAxis> resize_axis(rhccq_ctx* ctx, int32_t n_in, int32_t n_out, int filter, int* rc) {
  static std::mutex mu;
  static std::deque<std::pair<std::array<int32_t, 3>, std::shared_ptr<const ResizeAxis>>> kept;
  const std::array<int32_t, 3> key{n_in, n_out, filter};
  {
    std::lock_guard<std::mutex> lock(mu);
    for (const auto& e : kept)
      if (e.first == key) return e.second;
  }
  auto a = std::make_shared<ResizeAxis>();
  a->taps.resize((size_t)n_out);
  int64_t n = 0;
  if (resize_taps(n_in, n_out, filter, a->taps.data(), &a->weights, &n, &a->max_abs)) {
    *rc = resize_fail(ctx, RHCCQ_E_LIMIT, "resize: a sample's weights could overflow the 32-bit sum");
    return nullptr;
  }
  std::lock_guard<std::mutex> lock(mu);
  kept.emplace_back(key, a);
  if (kept.size() > 16) kept.pop_front();
  return a;
}

static void resize_copy(rhccq_ctx* ctx, const uint8_t* src, int64_t src_pitch, uint8_t* dst, int64_t dst_pitch, int row_bytes, int rows, int B) {
  const dim3 grid((unsigned)((row_bytes + 4 * kResizeBlock - 1) / (4 * kResizeBlock)), (unsigned)rows, (unsigned)B);
  hipLaunchKernelGGL(resize_copy_kernel, grid, dim3(kResizeBlock), 0, ctx->stream, src, (long long)src_pitch, dst, (long long)dst_pitch, row_bytes, rows);
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_resize_tile_rows(void) { return kResizeTileRows; }
int32_t rhccq_resize_run_cols(void) { return kResizeRunCols; }
int32_t rhccq_resize_strip_bytes(void) { return kResizeStripBytes; }

int rhccq_resize_taps_host(int32_t n_in, int32_t n_out, int32_t filter, int32_t* first, int32_t* count, int32_t* weights, int64_t weights_cap,
                           int64_t* n_weights) {
  if (!resize_side_ok(n_in) || !resize_side_ok(n_out) || filter < 0 || filter >= kResizeFilters || !n_weights || weights_cap < 0) return RHCCQ_E_ARG;
  int rc = 0;
  const auto held = resize_axis(nullptr, n_in, n_out, filter, &rc);
  if (!held) return rc;
  const ResizeAxis& a = *held;
  *n_weights = (int64_t)a.weights.size();
  if (!weights) return 0;                                                              // the sizing query
  if (!first || !count) return RHCCQ_E_ARG;
  if (weights_cap < *n_weights) return RHCCQ_E_LIMIT;
  for (int32_t i = 0; i < n_out; ++i) {
    first[i] = a.taps[(size_t)i].first;
    count[i] = a.taps[(size_t)i].count;
  }
  for (size_t i = 0; i < a.weights.size(); ++i) weights[i] = a.weights[i];
  return 0;
}

int64_t rhccq_resize_workspace_bytes(int32_t B, int32_t H, int32_t W, int32_t C, int32_t OH, int32_t OW) {
  if (B < 1 || B > kResizeMaxBatch || !resize_side_ok(H) || !resize_side_ok(W) || !resize_side_ok(OH) || !resize_side_ok(OW) || (C != 1 && C != 3 && C != 4))
    return RHCCQ_E_ARG;
  return resize_layout(B, H, W, C, OH, OW).total;
}

int rhccq_resize(rhccq_ctx* ctx, const uint8_t* src, int32_t B, int32_t H, int32_t W, int32_t C, uint8_t* dst, int32_t OH, int32_t OW, int32_t filter,
                 void* workspace, int64_t workspace_bytes) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = resize_check(ctx, src, B, H, W, C, dst, OH, OW, filter)) return rc;
  if ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 3u) return resize_fail(ctx, RHCCQ_E_ARG, "resize: src and dst must be aligned to 4");
  const ResizeLayout lay = resize_layout(B, H, W, C, OH, OW);
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 255u) || workspace_bytes < lay.total)
    return resize_fail(ctx, RHCCQ_E_ARG, "resize: a workspace of rhccq_resize_workspace_bytes, aligned to 256, is expected");
  const int row_bytes = OW * C;
  const int64_t pitch = resize_pitch(row_bytes);
  uint8_t* ws = static_cast<uint8_t*>(workspace);
  uint8_t* mid = ws + lay.mid;
  const dim3 block(kResizeBlock);
  if (W == OW && H == OH) {
    resize_copy(ctx, src, (int64_t)W * C, dst, (int64_t)W * C, row_bytes, H, B);
    RHCCQ_LAUNCH_CHECK(ctx);
    return 0;
  }
  if (W != OW) {
    int rc = 0;
    const auto held = resize_axis(ctx, W, OW, filter, &rc);
    if (!held) return rc;
    const ResizeAxis& x = *held;
    ResizeTap* d_tab = reinterpret_cast<ResizeTap*>(ws + lay.xtab);
    int32_t* d_w = reinterpret_cast<int32_t*>(ws + lay.xw);
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_tab, x.taps.data(), x.taps.size() * sizeof(ResizeTap), hipMemcpyHostToDevice, ctx->stream));   // pageable: staged on return
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_w, x.weights.data(), x.weights.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const long long total = (long long)B * H * W * C;
    const int aligned16 = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 && ((long long)W * C) % 16 == 0;
    const dim3 grid((unsigned)((OW + kResizeRunCols - 1) / kResizeRunCols), (unsigned)((H + kResizeTileRows - 1) / kResizeTileRows), (unsigned)B);
    const bool m24 = x.max_abs < (1 << 23);
#define RHCCQ_RESIZE_ROWS(C_, M_) \
  hipLaunchKernelGGL((resize_rows_kernel<C_, M_>), grid, block, 0, ctx->stream, src, total, (int)H, (int)W, (int)OW, (const ResizeTap*)d_tab, \
                     (const int32_t*)d_w, reinterpret_cast<uint32_t*>(mid), (int)(pitch / 4), aligned16)
    if (C == 1) { if (m24) RHCCQ_RESIZE_ROWS(1, true); else RHCCQ_RESIZE_ROWS(1, false); }
    else if (C == 3) { if (m24) RHCCQ_RESIZE_ROWS(3, true); else RHCCQ_RESIZE_ROWS(3, false); }
    else { if (m24) RHCCQ_RESIZE_ROWS(4, true); else RHCCQ_RESIZE_ROWS(4, false); }
#undef RHCCQ_RESIZE_ROWS
  } else {
    resize_copy(ctx, src, (int64_t)W * C, mid, pitch, row_bytes, H, B);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  if (H != OH) {
    int rc = 0;
    const auto held = resize_axis(ctx, H, OH, filter, &rc);
    if (!held) return rc;
    const ResizeAxis& y = *held;
    ResizeTap* d_tab = reinterpret_cast<ResizeTap*>(ws + lay.ytab);
    int32_t* d_w = reinterpret_cast<int32_t*>(ws + lay.yw);
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_tab, y.taps.data(), y.taps.size() * sizeof(ResizeTap), hipMemcpyHostToDevice, ctx->stream));
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_w, y.weights.data(), y.weights.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const dim3 grid((unsigned)((pitch / 4 + kResizeBlock - 1) / kResizeBlock), (unsigned)((OH + kResizeRunRows - 1) / kResizeRunRows), (unsigned)B);
    if (y.max_abs < (1 << 23))
      hipLaunchKernelGGL((resize_cols_kernel<true>), grid, block, 0, ctx->stream, reinterpret_cast<const uint32_t*>(mid), (int)H, (int)(pitch / 4), row_bytes,
                         (int)OH, (const ResizeTap*)d_tab, (const int32_t*)d_w, dst);
    else
      hipLaunchKernelGGL((resize_cols_kernel<false>), grid, block, 0, ctx->stream, reinterpret_cast<const uint32_t*>(mid), (int)H, (int)(pitch / 4), row_bytes,
                         (int)OH, (const ResizeTap*)d_tab, (const int32_t*)d_w, dst);
  } else {
    resize_copy(ctx, mid, pitch, dst, row_bytes, row_bytes, H, B);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_resize_host(const uint8_t* src, int32_t B, int32_t H, int32_t W, int32_t C, uint8_t* dst, int32_t OH, int32_t OW, int32_t filter) {
  if (const int rc = resize_check(nullptr, src, B, H, W, C, dst, OH, OW, filter)) return rc;
  int rc = 0;
  std::shared_ptr<const ResizeAxis> x, y;
  if (W != OW && !(x = resize_axis(nullptr, W, OW, filter, &rc))) return rc;
  if (H != OH && !(y = resize_axis(nullptr, H, OH, filter, &rc))) return rc;
  const int64_t L = (int64_t)OW * C;
  std::vector<uint8_t> mid(W != OW ? (size_t)((int64_t)B * H * L) : 0);
  const uint8_t* in = src;
  if (W != OW) {
    resize_pass_host(src, mid.data(), (int64_t)B * H, (int64_t)W * C, L, C, C, OW, x->taps.data(), x->weights.data());
    in = mid.data();
  }
  if (H != OH) {
    for (int64_t b = 0; b < B; ++b) resize_pass_host(in + b * H * L, dst + b * OH * L, 1, 0, 0, L, L, OH, y->taps.data(), y->weights.data());
  } else {
    for (int64_t i = 0; i < (int64_t)B * H * L; ++i) dst[i] = in[i];
  }
  return 0;
}

}  // extern "C"
