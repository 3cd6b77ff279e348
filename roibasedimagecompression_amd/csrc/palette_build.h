// The functions of the palette build (palette_build.hip) that its kernels and its host form share: the cell of a pixel, the summed-volume
// table and a box's sums from it, the gain of a cut as an exact rational, the 256-bit comparison of two gains, the best cut of a box and
// the split.  The rule is in include/rhccq.h; the derivation of the bit widths is in palette_build.hip.
#pragma once
#include "palette_remap.h"

namespace rhccq {

constexpr int kBuildSide = 32;                        // cells per axis: a cell is (r >> 3, g >> 3, b >> 3)
constexpr int kBuildCells = kBuildSide * kBuildSide * kBuildSide;
constexpr int kBuildTab = kBuildSide + 1;             // entries per axis of the summed-volume table: T(x, y, z) sums the cells below (x, y, z)
constexpr int kBuildTabEntries = kBuildTab * kBuildTab * kBuildTab;
constexpr int kBuildCodes = 3 * kBuildSide;           // a cut's code is axis * 32 + t; 93 of the 96 codes can be cuts (t = 0 never is)
constexpr int kBuildHostMaxRows = kBuildCells;        // the host form's K_target: no more boxes than cells
constexpr uint32_t kBuildNoIdx = 0xFFFFFFFFu;
constexpr uint8_t kBuildNoCut = 0xFFu;

typedef unsigned __int128 build_u128;
typedef __int128 build_i128;

// {N, Sr, Sg, Sb} of a cell, a box, or an entry of the summed-volume table (the table interleaves the planes: one corner is 32 bytes)
struct BuildSum { unsigned long long n, s[3]; };
// a box: the half-open cell range [lo, hi) per axis
struct BuildBox { uint8_t lo[3], hi[3]; };
// a cut's gain num / den (num < 2^146 in three limbs, den < 2^96 in two); den == 0: no valid cut.  idx orders equal gains: the cut's code
// inside a box (lowest axis, then lowest t), the box's index among boxes
struct BuildKey { unsigned long long num[3], den[2]; uint32_t idx; };

__host__ __device__ __forceinline__ int build_cell(uint32_t r, uint32_t g, uint32_t b) { return (int)((((r >> 3) * kBuildSide) + (g >> 3)) * kBuildSide + (b >> 3)); }
__host__ __device__ __forceinline__ int build_tab_index(int x, int y, int z) { return (x * kBuildTab + y) * kBuildTab + z; }
__host__ __device__ __forceinline__ BuildBox build_whole() { return {{0, 0, 0}, {kBuildSide, kBuildSide, kBuildSide}}; }

__host__ __device__ __forceinline__ BuildSum build_add(BuildSum a, const BuildSum& b) {
  a.n += b.n;
  for (int ch = 0; ch < 3; ++ch) a.s[ch] += b.s[ch];
  return a;
}
// (differences of table entries: the unsigned arithmetic wraps and the result is exact)
__host__ __device__ __forceinline__ BuildSum build_sub(BuildSum a, const BuildSum& b) {
  a.n -= b.n;
  for (int ch = 0; ch < 3; ++ch) a.s[ch] -= b.s[ch];
  return a;
}

// the box's cross-section at coordinate v of `axis`: the four corners over the other two axes.  face(hi) - face(lo) is the 8-corner box sum,
// face(t) - face(lo) the lower half of the cut (axis, t)
__host__ __device__ __forceinline__ BuildSum build_face(const BuildSum* __restrict__ T, const BuildBox& box, int axis, int v) {
  const int u = axis == 2 ? 0 : axis + 1, w = axis == 0 ? 2 : axis - 1;
  int c[3];
  c[axis] = v;
  c[u] = box.hi[u], c[w] = box.hi[w];
  BuildSum f = T[build_tab_index(c[0], c[1], c[2])];
  c[u] = box.lo[u];
  f = build_sub(f, T[build_tab_index(c[0], c[1], c[2])]);
  c[w] = box.lo[w];
  f = build_add(f, T[build_tab_index(c[0], c[1], c[2])]);
  c[u] = box.hi[u];
  return build_sub(f, T[build_tab_index(c[0], c[1], c[2])]);
}
__host__ __device__ __forceinline__ BuildSum build_box_sum(const BuildSum* __restrict__ T, const BuildBox& box) {
  return build_sub(build_face(T, box, 0, box.hi[0]), build_face(T, box, 0, box.lo[0]));
}

__host__ __device__ __forceinline__ BuildKey build_no_key() { return {{0ull, 0ull, 0ull}, {0ull, 0ull}, kBuildNoIdx}; }
__host__ __device__ __forceinline__ bool build_has_cut(const BuildKey& k) { return (k.den[0] | k.den[1]) != 0ull; }

// the gain |N S1 - N1 S|^2 / (N N1 (N - N1)) of a cut with 0 < N1 < N <= 2^32 - 1 and S <= 255 N: a channel's |N S1 - N1 S| is below 2^72
// and is squared limb by limb; the three squares add up below 2^146
__host__ __device__ __forceinline__ BuildKey build_gain(const BuildSum& box, const BuildSum& low, uint32_t idx) {
  BuildKey k = {{0ull, 0ull, 0ull}, {0ull, 0ull}, idx};
  for (int ch = 0; ch < 3; ++ch) {
    const build_i128 d = (build_i128)((build_u128)box.n * low.s[ch]) - (build_i128)((build_u128)low.n * box.s[ch]);
    const build_u128 a = (build_u128)(d < 0 ? -d : d);
    const unsigned long long al = (unsigned long long)a, ah = (unsigned long long)(a >> 64);          // ah < 2^8
    const build_u128 p0 = (build_u128)al * al, p1 = (build_u128)al * ah;
    const build_u128 mid = (p0 >> 64) + 2 * p1;
    const unsigned long long sq[3] = {(unsigned long long)p0, (unsigned long long)mid, (unsigned long long)(mid >> 64) + ah * ah};
    build_u128 carry = 0;
    for (int i = 0; i < 3; ++i) {
      carry += (build_u128)k.num[i] + sq[i];
      k.num[i] = (unsigned long long)carry;
      carry >>= 64;
    }
  }
  const build_u128 den = (build_u128)(box.n * low.n) * (box.n - low.n);                               // N N1 < 2^64, the product < 2^96
  k.den[0] = (unsigned long long)den;
  k.den[1] = (unsigned long long)(den >> 64);
  return k;
}

// num (three limbs) x den (two limbs): five limbs, of which a cross product (< 2^242) fills less than four
__host__ __device__ __forceinline__ void build_cross(const unsigned long long* num, const unsigned long long* den, unsigned long long* r) {
  for (int i = 0; i < 5; ++i) r[i] = 0ull;
  for (int i = 0; i < 3; ++i) {
    unsigned long long carry = 0ull;
    for (int j = 0; j < 2; ++j) {
      const build_u128 t = (build_u128)num[i] * den[j] + r[i + j] + carry;
      r[i + j] = (unsigned long long)t;
      carry = (unsigned long long)(t >> 64);
    }
    r[i + 2] = carry;
  }
}

// limbs (least significant first) as a double: every conversion, product with 2^64 and sum rounds once or not at all, so the result is
// within a few 2^-53 of the value
__host__ __device__ __forceinline__ double build_approx(const unsigned long long* v, int limbs) {
  double d = 0.0;
  for (int i = limbs - 1; i >= 0; --i) d = d * 18446744073709551616.0 + (double)v[i];
  return d;
}

// x before y: the larger gain, exactly (x.num y.den against y.num x.den); equal gains: the lower idx; a key without a cut is behind every other.
// The cross products are first formed in doubles (below 2^242: no overflow), each within 2^-49 of its value: when they differ by more than
// 2^-40 of the larger one the order is decided; every closer pair, ties among them, takes the exact comparison
__host__ __device__ __forceinline__ bool build_before(const BuildKey& x, const BuildKey& y) {
  if (!build_has_cut(x)) return false;
  if (!build_has_cut(y)) return true;
  const double fl = build_approx(x.num, 3) * build_approx(y.den, 2), fr = build_approx(y.num, 3) * build_approx(x.den, 2);
  const double gap = fl > fr ? fl - fr : fr - fl;
  if (gap > (fl > fr ? fl : fr) * 9.094947017729282e-13) return fl > fr;                // (2^-40)
  unsigned long long l[5], r[5];
  build_cross(x.num, y.den, l);
  build_cross(y.num, x.den, r);
  for (int i = 4; i >= 0; --i)
    if (l[i] != r[i]) return l[i] > r[i];
  return x.idx < y.idx;
}

// the key of the cut `code` = axis * 32 + t of a box (idx = code), or no key when the code is no valid cut of it
__host__ __device__ __forceinline__ BuildKey build_cut_key(const BuildSum* __restrict__ T, const BuildBox& box, int code) {
  const int axis = code >> 5, t = code & (kBuildSide - 1);
  if (code >= kBuildCodes || t <= (int)box.lo[axis] || t >= (int)box.hi[axis]) return build_no_key();
  const BuildSum base = build_face(T, box, axis, box.lo[axis]);
  const BuildSum all = build_sub(build_face(T, box, axis, box.hi[axis]), base), low = build_sub(build_face(T, box, axis, t), base);
  if (low.n == 0ull || low.n >= all.n) return build_no_key();
  return build_gain(all, low, (uint32_t)code);
}

// the best cut of a box: ascending codes and a strict comparison keep the lowest axis, then the lowest t
__host__ __device__ __forceinline__ BuildKey build_best_cut(const BuildSum* __restrict__ T, const BuildBox& box) {
  BuildKey best = build_no_key();
  for (int code = 0; code < kBuildCodes; ++code) {
    const BuildKey k = build_cut_key(T, box, code);
    if (build_before(k, best)) best = k;
  }
  return best;
}

// the split: `box` becomes the lower half of the cut, the upper half is returned
__host__ __device__ __forceinline__ BuildBox build_split(BuildBox& box, int code) {
  const int axis = code >> 5, t = code & (kBuildSide - 1);
  BuildBox up = box;
  up.lo[axis] = (uint8_t)t;
  box.hi[axis] = (uint8_t)t;
  return up;
}

// a box's palette row and count
__host__ __device__ __forceinline__ void build_row(const BuildSum& s, uint8_t* row, unsigned long long* count) {
  for (int ch = 0; ch < 3; ++ch) row[ch] = (uint8_t)refine_mean(s.s[ch], s.n);
  *count = s.n;
}

}  // namespace rhccq
