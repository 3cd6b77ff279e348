// The functions of the palette build (palette_build.hip) that its kernels and its host form share: the cell of a pixel, the summed-volume
// table and a box's sums from it, the gain of a cut as an exact rational, the 256-bit comparison of two gains, the best cut of a box and
// the split; and, behind them, the bodies of its kernels with their constants and the argument checks, which the batched form
// (palette_batch.hip) runs per image.  The rule is in include/rhccq.h; the derivation of the bit widths is in palette_build.hip.
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

// ---- the kernels' bodies, shared by palette_build.hip (one image a launch) and palette_batch.hip (one image per grid row) -----------
constexpr int kCellsBlock = 256;                      // lanes of a workgroup of the cells pass
constexpr int kCellsPx = 8;                           // pixels of a lane, a block apart
constexpr int kCellsChunk = kCellsBlock * kCellsPx;   // pixels of a workgroup at a time
constexpr int kCellsRounds = 4;                       // cells a wave aggregates per 64 pixels before its lanes add on their own
constexpr int kCellsSlots = 1024;                     // slots of a workgroup's table in LDS: 36 bytes a slot, four workgroups a CU
constexpr uint32_t kCellsFree = 0xFFFFFFFFu;
constexpr unsigned long long kCellsMaxSum = kReduceMaxSum;
static_assert(64ull * 255 * 255 < (1ull << 32), "a wave's sums of one pixel column fit 32 bits");

constexpr int kBuildBlock = 256;                      // lanes of the chain's resident workgroup: two waves per new box
constexpr int kBuildWaves = kBuildBlock / 64;
constexpr int kBuildMaxRows = 1024;                   // boxes whose state the LDS of the chain holds (48 bytes a box)
static_assert(kBuildWaves == 4 && kBuildCodes <= 128, "two waves cover the codes of a box");
static_assert(kBuildMaxRows * 48 + 1024 <= 64 * 1024 && kBuildMaxRows <= kBuildCells, "LDS layout of the chain kernel");
static_assert(sizeof(BuildSum) == 32, "a table entry is four 64-bit words");

struct CellsWeights { uint32_t w[kRemapMaxClasses + 1]; };

__device__ __forceinline__ void cells_add(unsigned long long* __restrict__ cells, int cell, unsigned long long n, unsigned long long r,
                                          unsigned long long g, unsigned long long b) {
  atomicAdd(cells + cell, n);
  atomicAdd(cells + kBuildCells + cell, r);
  atomicAdd(cells + 2 * kBuildCells + cell, g);
  atomicAdd(cells + 3 * kBuildCells + cell, b);
}

// the slot of a cell in the workgroup's table: the low bits of the three coordinates, so that the cells of a 16 x 8 x 8 neighbourhood
// of the colour cube, what a stretch of a picture mostly holds, never share a slot
__device__ __forceinline__ int cells_slot(int cell) { return ((cell >> 10) & 15) << 6 | ((cell >> 5) & 7) << 3 | (cell & 7); }

// one contribution to the workgroup's table, or, when another cell holds the slot, straight to global memory
__device__ __forceinline__ void cells_put(uint32_t* s_tag, unsigned long long* s_acc, unsigned long long* __restrict__ cells, int cell, uint32_t n,
                                          uint32_t r, uint32_t g, uint32_t b) {
  const int slot = cells_slot(cell);
  uint32_t tag = s_tag[slot];
  if (tag == kCellsFree) {
    tag = atomicCAS(&s_tag[slot], kCellsFree, (uint32_t)cell);
    if (tag == kCellsFree) tag = (uint32_t)cell;
  }
  if (tag == (uint32_t)cell) {
    atomicAdd(&s_acc[slot * 4], (unsigned long long)n);
    atomicAdd(&s_acc[slot * 4 + 1], (unsigned long long)r);
    atomicAdd(&s_acc[slot * 4 + 2], (unsigned long long)g);
    atomicAdd(&s_acc[slot * 4 + 3], (unsigned long long)b);
  } else {
    cells_add(cells, cell, n, r, g, b);
  }
}

// the cells pass of workgroup `bid` of the `nblk` that share the image: a contiguous stretch of its chunks
__device__ __forceinline__ void palette_cells_body(const uint8_t* __restrict__ rgb, long long n_px, const uint8_t* __restrict__ cls,
                                                   int n_classes, CellsWeights wt, unsigned long long* __restrict__ cells, long long bid,
                                                   long long nblk) {
  __shared__ uint32_t s_w[kRemapMaxClasses + 1];
  __shared__ uint32_t s_tag[kCellsSlots];                                              // the cell that holds the slot, or kCellsFree
  __shared__ unsigned long long s_acc[kCellsSlots * 4];                                // its {N, Sr, Sg, Sb} over this workgroup's pixels
  const int lane = threadIdx.x & 63;
  if ((int)threadIdx.x <= n_classes) s_w[threadIdx.x] = wt.w[threadIdx.x];
  for (int j = threadIdx.x; j < kCellsSlots; j += kCellsBlock) s_tag[j] = kCellsFree;
  for (int j = threadIdx.x; j < kCellsSlots * 4; j += kCellsBlock) s_acc[j] = 0ull;
  __syncthreads();
  const long long n_chunks = (n_px + kCellsChunk - 1) / kCellsChunk, per = (n_chunks + nblk - 1) / nblk;
  const long long last = min(n_chunks, (bid + 1) * per);             // a contiguous stretch: its pixels share cells
  for (long long chunk = bid * per; chunk < last; ++chunk) {
    const long long base = chunk * kCellsChunk + threadIdx.x;
    uint32_t px[kCellsPx], w[kCellsPx];
#pragma unroll
    for (int q = 0; q < kCellsPx; ++q) {
      const long long p = base + (long long)q * kCellsBlock;
      px[q] = 0u;
      w[q] = 0u;
      if (p < n_px) {
        px[q] = remap_pack_px(rgb + p * 3);
        const int c = n_classes > 0 ? (int)cls[p] : n_classes;
        w[q] = s_w[c < n_classes ? c : n_classes];
      }
    }
#pragma unroll
    for (int q = 0; q < kCellsPx; ++q) {
      const uint32_t r = px[q] >> 16, g = (px[q] >> 8) & 255u, b = px[q] & 255u;
      const int cell = build_cell(r, g, b);
      const uint32_t wr = w[q] * r, wg = w[q] * g, wb = w[q] * b;
      unsigned long long open = __ballot(w[q] != 0u);                                  // (wave uniform, as is the loop below)
      for (int round = 0; round < kCellsRounds && open; ++round) {
        const int first = __ffsll((long long)open) - 1;
        const int lead = __shfl(cell, first, 64);
        const bool mine = ((open >> lane) & 1ull) && cell == lead;
        const uint32_t sn = wave_sum(mine ? w[q] : 0u), sr = wave_sum(mine ? wr : 0u), sg = wave_sum(mine ? wg : 0u), sb = wave_sum(mine ? wb : 0u);
        if (lane == 0) cells_put(s_tag, s_acc, cells, lead, sn, sr, sg, sb);
        open &= ~__ballot(mine);
      }
      if ((open >> lane) & 1ull) cells_put(s_tag, s_acc, cells, cell, w[q], wr, wg, wb);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kCellsSlots; j += kCellsBlock) {
    const uint32_t tag = s_tag[j];
    if (tag != kCellsFree) cells_add(cells, (int)tag, s_acc[j * 4], s_acc[j * 4 + 1], s_acc[j * 4 + 2], s_acc[j * 4 + 3]);
  }
}

// ---- the summed-volume table -------------------------------------------------------------------------------------------------------
// a running sum along b: thread i per (x, y, plane) of the table, the borders x == 0 and y == 0 included (they are zero)
__device__ __forceinline__ void build_prefix_b_body(const unsigned long long* __restrict__ cells, unsigned long long* __restrict__ T, int i) {
  if (i >= kBuildTab * kBuildTab * 4) return;
  const int plane = i & 3, y = (i >> 2) % kBuildTab, x = (i >> 2) / kBuildTab;
  unsigned long long* row = T + (size_t)build_tab_index(x, y, 0) * 4 + plane;
  row[0] = 0ull;
  unsigned long long run = 0ull;
  for (int z = 1; z < kBuildTab; ++z) {
    if (x > 0 && y > 0) {
      const unsigned long long v = cells[(size_t)plane * kBuildCells + ((x - 1) * kBuildSide + (y - 1)) * kBuildSide + (z - 1)];
      run += plane == 0 ? reduce_clamp(v) : v;
    }
    row[(size_t)z * 4] = run;
  }
}
// a running sum in place along g (outer = x, step = one y) or along r (outer = y, step = one x): thread i per line and (z, plane)
__device__ __forceinline__ void build_prefix_body(unsigned long long* __restrict__ T, int outer_stride, int step, int i) {
  if (i >= kBuildTab * kBuildTab * 4) return;
  unsigned long long* p = T + (size_t)(i / (kBuildTab * 4)) * outer_stride + i % (kBuildTab * 4);
  unsigned long long run = 0ull;
  for (int k = 0; k < kBuildTab; ++k) {
    run += p[(size_t)k * step];
    p[(size_t)k * step] = run;
  }
}

// ---- the chain ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ BuildKey build_shfl_xor(const BuildKey& k, int o) {
  BuildKey t;
#pragma unroll
  for (int i = 0; i < 3; ++i) t.num[i] = __shfl_xor(k.num[i], o, 64);
  t.den[0] = __shfl_xor(k.den[0], o, 64);
  t.den[1] = __shfl_xor(k.den[1], o, 64);
  t.idx = __shfl_xor(k.idx, o, 64);
  return t;
}
// the first key of the wave in every lane: the order is total (no two live keys share an idx), so every lane ends on the same key
__device__ __forceinline__ BuildKey build_wave_first(BuildKey k) {
  for (int o = 32; o > 0; o >>= 1) {
    const BuildKey t = build_shfl_xor(k, o);
    if (build_before(t, k)) k = t;
  }
  return k;
}

// the chain of one table, run by one workgroup of kBuildBlock lanes
__device__ __forceinline__ void build_chain_body(const BuildSum* __restrict__ T, int K_target, uint8_t* __restrict__ pal_out,
                                                 unsigned long long* __restrict__ counts_out, uint8_t* __restrict__ boxes_out,
                                                 int32_t* __restrict__ splits, int32_t* __restrict__ k_out) {
  __shared__ unsigned long long s_num[3][kBuildMaxRows], s_den[2][kBuildMaxRows];      // the gain of every box's best cut
  __shared__ BuildBox s_box[kBuildMaxRows];
  __shared__ uint8_t s_cut[kBuildMaxRows];                                              // its code, kBuildNoCut: the box has no valid cut
  __shared__ BuildKey s_new[kBuildWaves], s_best[kBuildWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  const unsigned long long total = T[build_tab_index(kBuildSide, kBuildSide, kBuildSide)].n;
  if (total == 0ull || total > kReduceMaxSum) {                                        // (block uniform)
    for (int j = tid; j < K_target * 3; j += kBuildBlock) pal_out[j] = 0;
    for (int j = tid; j < K_target; j += kBuildBlock) counts_out[j] = 0ull;
    if (boxes_out)
      for (int j = tid; j < K_target * 6; j += kBuildBlock) boxes_out[j] = 0;
    if (splits)
      for (int j = tid; j < (K_target - 1) * 3; j += kBuildBlock) splits[j] = -1;
    if (tid == 0) *k_out = total == 0ull ? RHCCQ_E_ARG : RHCCQ_E_LIMIT;
    return;
  }

  int nb = 1, done = 0;
  int id_a = 0, id_b = -1;                                                             // the boxes whose best cut is not known yet
  BuildBox box_a = build_whole(), box_b = build_whole();
  for (;;) {
    // the candidate cuts of the new boxes: waves 0 and 1 take box a, waves 2 and 3 box b, a lane one code
    BuildKey k = build_no_key();
    if (wv < 2 || id_b >= 0) k = build_cut_key(T, wv < 2 ? box_a : box_b, (wv & 1) * 64 + lane);
    k = build_wave_first(k);
    if (lane == 0) s_new[wv] = k;
    __syncthreads();
    if (tid == 0) {
      for (int h = 0; h < (id_b >= 0 ? 2 : 1); ++h) {
        const BuildKey best = build_before(s_new[h * 2 + 1], s_new[h * 2]) ? s_new[h * 2 + 1] : s_new[h * 2];
        const int id = h ? id_b : id_a;
        for (int i = 0; i < 3; ++i) s_num[i][id] = best.num[i];
        s_den[0][id] = best.den[0];
        s_den[1][id] = best.den[1];
        s_cut[id] = build_has_cut(best) ? (uint8_t)best.idx : kBuildNoCut;
        s_box[id] = h ? box_b : box_a;
      }
    }
    __syncthreads();
    if (nb >= K_target) break;

    // arg-max over the boxes: the largest gain, the lowest box among equals
    BuildKey best = build_no_key();
    for (int j = tid; j < nb; j += kBuildBlock) {
      if (s_cut[j] == kBuildNoCut) continue;
      const BuildKey c = {{s_num[0][j], s_num[1][j], s_num[2][j]}, {s_den[0][j], s_den[1][j]}, (uint32_t)j};
      if (build_before(c, best)) best = c;
    }
    best = build_wave_first(best);
    if (lane == 0) s_best[wv] = best;
    __syncthreads();
    best = s_best[0];
    for (int i = 1; i < kBuildWaves; ++i)
      if (build_before(s_best[i], best)) best = s_best[i];
    if (!build_has_cut(best)) break;                                                   // no box has a valid cut (block uniform)

    // the split: the box keeps its index and becomes the lower half, the upper half takes the next index (stored by lane 0 above, behind
    // the next barrier: every lane has read s_box and s_cut by then)
    id_a = (int)best.idx;
    id_b = nb++;
    const int code = (int)s_cut[id_a];
    box_a = s_box[id_a];
    box_b = build_split(box_a, code);
    if (tid == 0 && splits) {
      splits[done * 3] = id_a;
      splits[done * 3 + 1] = code >> 5;
      splits[done * 3 + 2] = code & (kBuildSide - 1);
    }
    ++done;
  }

  for (int j = tid; j < nb; j += kBuildBlock) {
    const BuildBox box = s_box[j];
    build_row(build_box_sum(T, box), pal_out + j * 3, counts_out + j);
    if (boxes_out)
      for (int i = 0; i < 3; ++i) {
        boxes_out[j * 6 + i] = box.lo[i];
        boxes_out[j * 6 + 3 + i] = box.hi[i];
      }
  }
  for (int j = nb * 3 + tid; j < K_target * 3; j += kBuildBlock) pal_out[j] = 0;
  for (int j = nb + tid; j < K_target; j += kBuildBlock) counts_out[j] = 0ull;
  if (boxes_out)
    for (int j = nb * 6 + tid; j < K_target * 6; j += kBuildBlock) boxes_out[j] = 0;
  if (splits)
    for (int j = done * 3 + tid; j < (K_target - 1) * 3; j += kBuildBlock) splits[j] = -1;
  if (tid == 0) *k_out = nb;
}

static inline int cells_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* cls, int32_t n_classes, const int32_t* weights, const void* cells,
                       CellsWeights* wt) {
  if (!rgb || !cells) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: null argument");
  if (n_pixels < 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: n_pixels >= 0 is required");
  if (const int rc = classes_check(ctx, "palette_cells", cls, n_classes)) return rc;
  uint32_t top;
  if (const int rc = weights_check(ctx, "palette_cells", weights, n_classes, wt->w, &top)) return rc;
  if ((uintptr_t)cells & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: misaligned cells (8)");
  if ((uint64_t)n_pixels > kCellsMaxSum / top) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_cells: n_pixels x the largest weight exceeds 2^32 - 1");
  return 0;
}

static inline int build_check(rhccq_ctx* ctx, const void* cells, int32_t K_target, const void* palette_out, const void* counts_out, const void* splits,
                       const void* k_out) {
  if (!cells || !palette_out || !counts_out || !k_out) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: null argument");
  if (K_target < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: K_target >= 1 is required");
  if (((uintptr_t)cells & 7) || ((uintptr_t)counts_out & 7) || ((uintptr_t)splits & 3) || ((uintptr_t)k_out & 3))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: misaligned cells, counts_out (8), splits or k_out (4)");
  if (K_target > kBuildHostMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build: at most 32768 colours");
  return 0;
}

}  // namespace rhccq
