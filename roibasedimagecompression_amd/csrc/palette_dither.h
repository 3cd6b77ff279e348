// The step functions and constants of the error-diffusing remap, shared by its kernel and its host form (palette_dither.hip).
//
// Arithmetic.  A pixel's quantisation error E is three channel differences in -255..255: nine signed bits each, three of them in one 32-bit
// word (bits 0-8 blue, 9-17 green, 18-26 red, two's complement), so the word 0 is "no error" and serves every term outside the picture.
// Bit 31 is free: the words a band hands to the next one through global memory carry it as their "written" mark.
// Per channel the weighted sum A = 7 E(left) + E(up-left) + 5 E(up) + 3 E(up-right) has |A| <= 16 * 255 = 4080; with a strength of at
// most 256, |s A + 2048| < 2^21: int32 throughout.  The shift by 12 is arithmetic, so the quotient is floored toward minus infinity.
#pragma once
#include "band_handoff.h"
#include "palette_runs.h"

namespace rhccq {

constexpr uint32_t kDitherMaxStrength = 256u;  // Floyd-Steinberg in full: s / 256 of the weights 7, 1, 5, 3 over 16
constexpr int kDitherMaxRows = 4096;           // palette rows of the device form: packed as RemapEntry they are 32 KiB of LDS, and a row's index 12 bits
constexpr int kDitherLanes = 64;               // lanes of a workgroup (one wave)
constexpr int kDitherCols = 64;                // steps of a staging tile
constexpr int kDitherPitch = kDitherCols + 1;  // dwords between the rows of a tile in LDS (odd: the rows' lanes hit different banks)
constexpr int kDitherRowsMin = 4;              // image rows of a band, a power of two in [min, max]: 64 / rows lanes share a pixel's search,
constexpr int kDitherRowsMax = 32;             // and 2..16 lanes are inside one DPP row
constexpr int kDitherRowsDefault = 4;
constexpr int kDitherGranule = 4;              // hand-over words a band fetches from its predecessor at a time (band_handoff.h)

struct DitherStrength { uint32_t v[kRemapMaxClasses + 1]; };
struct DitherErr { int32_t r, g, b; };

__host__ __device__ __forceinline__ uint32_t dither_pack(DitherErr e) {
  return ((uint32_t)e.r & 511u) << 18 | ((uint32_t)e.g & 511u) << 9 | ((uint32_t)e.b & 511u);
}
// (bit 31 and the unused bits above the red field are shifted out)
__host__ __device__ __forceinline__ DitherErr dither_unpack(uint32_t w) {
  return {(int32_t)(w << 5) >> 23, (int32_t)(w << 14) >> 23, (int32_t)(w << 23) >> 23};
}
// the weighted sum of the four errors that reach a pixel, one channel
__host__ __device__ __forceinline__ int32_t dither_asum(int32_t left, int32_t up_left, int32_t up, int32_t up_right) {
  return 7 * left + up_left + 5 * up + 3 * up_right;
}
// one channel of the target: the pixel's value plus the scaled sum, floored and clamped
__host__ __device__ __forceinline__ uint32_t dither_channel(uint32_t p, uint32_t strength, int32_t a) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int32_t t = (int32_t)p + ((__mul24((int32_t)strength, a) + 2048) >> 12);      // (both factors are inside 24 bits: the full-rate multiply)
#else
  const int32_t t = (int32_t)p + (((int32_t)strength * a + 2048) >> 12);
#endif
  return (uint32_t)(t < 0 ? 0 : t > 255 ? 255 : t);
}
// the target of a pixel (0x00RRGGBB, as remap_pack_px packs it; px may carry anything in its top byte) from the errors around it
__host__ __device__ __forceinline__ uint32_t dither_target(uint32_t px, uint32_t strength, DitherErr left, DitherErr up_left, DitherErr up,
                                                           DitherErr up_right) {
  return dither_channel((px >> 16) & 255u, strength, dither_asum(left.r, up_left.r, up.r, up_right.r)) << 16 |
         dither_channel((px >> 8) & 255u, strength, dither_asum(left.g, up_left.g, up.g, up_right.g)) << 8 |
         dither_channel(px & 255u, strength, dither_asum(left.b, up_left.b, up.b, up_right.b));
}
// the error a pixel passes on: its (clamped) target minus the colour of the row it took
__host__ __device__ __forceinline__ DitherErr dither_error(uint32_t target, uint32_t col) {
  return {(int32_t)((target >> 16) & 255u) - (int32_t)((col >> 16) & 255u), (int32_t)((target >> 8) & 255u) - (int32_t)((col >> 8) & 255u),
          (int32_t)(target & 255u) - (int32_t)(col & 255u)};
}
// a packed palette entry's colour back (remap_pack_entry stores 0x00FFFFFF - colour)
__host__ __device__ __forceinline__ uint32_t dither_entry_colour(RemapEntry e) { return 0x00FFFFFFu - e.inv; }

// bands of `rows` image rows
static inline int64_t dither_bands(int64_t H, int64_t rows) { return (H + rows - 1) / rows; }
// the workspace: the head and one word per pixel of every band's last row but the last band's, for the band height that needs the most
static inline int64_t dither_work_bytes(int64_t H, int64_t W, int64_t rows) { return band::work_bytes(dither_bands(H, rows), W); }

// the argument tests of both forms, in rhccq_palette_runs' order, then the strengths; the device form appends its own
static inline int dither_check(rhccq_ctx* ctx, const void* rgb, int32_t H, int32_t W, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                               const uint32_t* strength, const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  const char* const what = "palette_dither";
  if (const int rc = rows_check(ctx, what, rgb, H, W, palette, K, cls, n_classes, strength, idx_out, idx_elem_bytes, sums)) return rc;
  if (const int rc = search_limit(ctx, what, K)) return rc;
  for (int i = 0; i <= n_classes; ++i)
    if (strength[i] > kDitherMaxStrength) return remap_fail(ctx, RHCCQ_E_ARG, what, ": a strength is at most 256");
  return 0;
}

}  // namespace rhccq
