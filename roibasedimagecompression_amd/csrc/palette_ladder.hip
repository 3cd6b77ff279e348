// The palette ladder (EXTENSION, no reference counterpart): what a byte or PSNR target needs on top of the reduction of
// palette_reduce.hip, without running its merge chain once per probe.  The definitions are in include/rhccq.h; in short:
//   moments   one pass over the pixels: a(p), the remap's index, and per class table and palette row the integer moments
//             {N, Sr, Sg, Sb, Q = sum |p|^2} of the pixels with a(p) = that row.
//   curve     the merges log of ONE chain run to a single row is replayed over those moments: the squared error of the picture shown
//             through the merged rows, sum over clusters of (Q - 2 c.S + N |c|^2), after every step and per table.  It bounds the error
//             of every rung from above: the nearest-row remap that follows a reduction can only lower each pixel's error.
//   rung      the rows of any rung from a prefix of the log: a cluster's centre is the rounded mean of the exact sums of its
//             original rows (refine_mean), so it does not depend on the order its rows met in.
//
// Exactness.  The counts add up to at most 2^32 - 1 and the unweighted N of a table is a pixel count no larger, so with
// |p|^2, |c|^2 <= 3 * 255^2 < 2^18 every one of Q, c.S and N |c|^2 is below 2^50, 2 c.S below 2^51, and a whole table's sum of any of
// them as well (the clusters partition the pixels): every term and every sum fits 64 bits with room to spare.  Each term
// Q - 2 c.S + N |c|^2 = sum |p - c|^2 is non-negative, so unsigned arithmetic (wrapping in between) gives the exact value.
//
// Device forms (async on the context stream, stream order the only synchronisation: no kernel waits for another workgroup):
//   moments   memset | remap_search (palette_remap.h: 256 lanes x 8 pixels, palette tiles through LDS) with accumulators as the
//             refinement's assign kernel keeps them: a copy per workgroup in (dynamic) LDS while (tables x K x 40 bytes) fits beside the
//             tile in 64 KiB, flushed with 64-bit atomics, global atomics above that | a finish launch that adds the class tables into the last
//             one (during the pass it holds the pixels of no class, afterwards every pixel).
//   curve     copy of the moments into the workspace | one thread per (table, row): row state and the initial sums | ONE wave that
//             replays the log: lanes 0..2 own a channel of S, lane t owns table t; n and c live in LDS.  Latency bound, like the chain.
//   rung      ONE workgroup (K <= 4096): parent links from the log's prefix in LDS, pointer jumping to the roots, then n and n * row
//             added per root through one 32 KiB LDS buffer, a pass per field, then refine_mean.
#include "palette_remap.h"

#include <algorithm>
#include <vector>

namespace rhccq {

constexpr int kLadderMaxRows = kReduceMaxRows;         // the reduction is the only producer of a device log (palette_remap.h)
constexpr int kLadderFields = 5;                       // N, Sr, Sg, Sb, Q
constexpr int kLadderMaxTables = kRemapMaxClasses + 1;
constexpr int kMomentsLdsBytes = 64 * 1024 - kRemapTile * 8 - 1024;      // what the accumulators may take beside the tile
constexpr int kRungBlock = 1024;
constexpr int kRungRows = kLadderMaxRows / kRungBlock; // rows a lane of the rung kernel numbers
// a wave's sum of one pixel column: 64 lanes x 3 x 255^2 < 2^32, so the wave-uniform path reduces in 32 bits
static_assert(64ull * 3 * 255 * 255 < (1ull << 32), "wave sums fit 32 bits");
// 2 c.S <= 2 * 3 * 255^2 * N < 2^19 * 2^32
static_assert(2ull * 3 * 255 * 255 < (1ull << 19) && kReduceMaxSum < (1ull << 32), "every term of the curve is below 2^51");
static_assert(kLadderMaxRows * 2 * 2 + kLadderMaxRows * 8 + 1024 <= 64 * 1024 && kRungRows * kRungBlock == kLadderMaxRows, "LDS layout of the rung kernel");
static_assert(kLadderMaxRows * 8 <= 64 * 1024, "n and c of the curve's replay in LDS");

__host__ __device__ __forceinline__ int moments_lds_rows(int n_classes) { return kMomentsLdsBytes / (kLadderFields * 8 * (n_classes + 1)); }

// sum |p - c|^2 over the pixels whose moments m = {N, Sr, Sg, Sb, Q} are, c packed as 0x00RRGGBB
__host__ __device__ __forceinline__ unsigned long long curve_sse(const unsigned long long* m, uint32_t c) {
  const unsigned long long cr = c >> 16, cg = (c >> 8) & 255u, cb = c & 255u;
  return m[4] - 2ull * (cr * m[1] + cg * m[2] + cb * m[3]) + m[0] * (cr * cr + cg * cg + cb * cb);
}

// a step of the log is a merge iff it names two rows a < b inside the palette
__host__ __device__ __forceinline__ bool ladder_step_ok(int a, int b, int K) { return a >= 0 && a < b && b < K; }

// ---- moments ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void moments_add(unsigned long long* row, uint32_t n, uint32_t r, uint32_t g, uint32_t b, uint32_t q) {
  atomicAdd(row + 0, (unsigned long long)n);
  atomicAdd(row + 1, (unsigned long long)r);
  atomicAdd(row + 2, (unsigned long long)g);
  atomicAdd(row + 3, (unsigned long long)b);
  atomicAdd(row + 4, (unsigned long long)q);
}

template <typename IdxT, bool kLds>
__global__ __launch_bounds__(kRemapBlock) void palette_moments_kernel(const uint8_t* __restrict__ rgb, long long n_px, const uint8_t* __restrict__ pal,
                                                                      int K, const uint8_t* __restrict__ cls, int n_classes,
                                                                      IdxT* __restrict__ idx_out, unsigned long long* __restrict__ mom) {
  extern __shared__ unsigned long long s_acc[];                                         // kLds: [n_classes + 1][K][5]
  const int lane = threadIdx.x & 63;
  const int n_acc = (n_classes + 1) * K * kLadderFields;
  if (kLds)
    for (int j = threadIdx.x; j < n_acc; j += kRemapBlock) s_acc[j] = 0ull;
  __syncthreads();

  remap_search(rgb, n_px, pal, K, blockIdx.x, gridDim.x, [&](long long base, auto& px, auto&, auto& bidx) {
    unsigned long long* tab = kLds ? s_acc : mom;
#pragma unroll
    for (int q = 0; q < kRemapPx; ++q) {
      const long long p = base + (long long)q * kRemapBlock;
      const bool in = p < n_px;
      if (__ballot(in) == 0ull) continue;                                              // (wave uniform; p grows with the lane: lane 0 is inside below)
      int t = n_classes;
      if (in) {
        if (idx_out) idx_out[p] = (IdxT)bidx[q];
        if (n_classes > 0) {
          const int c = (int)cls[p];
          t = c < n_classes ? c : n_classes;
        }
      }
      const uint32_t slot = (uint32_t)t * (uint32_t)K + bidx[q];                       // the accumulator row: exactly one table per pixel
      const uint32_t w = in ? 1u : 0u, r = px[q] >> 16, g = (px[q] >> 8) & 255u, b = px[q] & 255u, qq = remap_dot(px[q], px[q]);
      // neighbouring lanes hold neighbouring pixels: in flat areas the whole wave has one winner and one class, and one lane adds the wave's sums
      const uint32_t first = __builtin_amdgcn_readfirstlane(slot);
      if (__ballot(!in || slot == first) == ~0ull) {
        const uint32_t sn = wave_sum(w), sr = wave_sum(r), sg = wave_sum(g), sb = wave_sum(b), sq = wave_sum(qq);     // (px = 0 outside the picture)
        if (lane == 0) moments_add(tab + (size_t)first * kLadderFields, sn, sr, sg, sb, sq);
      } else if (in) {
        moments_add(tab + (size_t)slot * kLadderFields, 1u, r, g, b, qq);
      }
    }
  });
  if (kLds) {
    __syncthreads();
    for (int j = threadIdx.x; j < n_acc; j += kRemapBlock) {
      const unsigned long long v = s_acc[j];
      if (v) atomicAdd(&mom[j], v);
    }
  }
}

// the last table held the pixels of no class: with the class tables added it holds every pixel
__global__ __launch_bounds__(256) void palette_moments_finish_kernel(unsigned long long* __restrict__ mom, int K, int n_classes) {
  const int j = blockIdx.x * 256 + threadIdx.x, n = K * kLadderFields;
  if (j >= n) return;
  unsigned long long v = mom[(size_t)n_classes * n + j];
  for (int c = 0; c < n_classes; ++c) v += mom[(size_t)c * n + j];
  mom[(size_t)n_classes * n + j] = v;
}

static int moments_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                         const void* idx_out, int32_t idx_elem_bytes, const void* moments) {
  const char* const what = "palette_moments";
  if (const int rc = search_check(ctx, what, !rgb || !palette || !moments, n_pixels, K, cls, n_classes)) return rc;
  if (idx_out) {
    if (const int rc = index_check(ctx, what, idx_out, idx_elem_bytes)) return rc;
    if (const int rc = index_rows_check(ctx, what, idx_elem_bytes, K)) return rc;
  }
  if ((uintptr_t)moments & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_moments: misaligned moments");
  return search_limit(ctx, what, K);
}

template <typename IdxT>
static void moments_host(const uint8_t* rgb, int64_t n_px, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, IdxT* idx_out, uint64_t* mom) {
  const std::vector<RemapEntry> ent = remap_pack_palette(pal, K);
  for (int64_t p = 0; p < n_px; ++p) {
    const uint32_t px = remap_pack_px(rgb + p * 3);
    uint32_t key;
    const uint32_t idx = remap_search_host(px, ent, &key);
    if (idx_out) idx_out[p] = (IdxT)idx;
    const int t = n_classes > 0 && cls[p] < n_classes ? cls[p] : n_classes;
    uint64_t* row = mom + ((size_t)t * K + idx) * kLadderFields;
    row[0] += 1;
    for (int ch = 0; ch < 3; ++ch) row[1 + ch] += rgb[p * 3 + ch];
    row[4] += remap_dot(px, px);
  }
  const size_t n = (size_t)K * kLadderFields;
  for (int c = 0; c < n_classes; ++c)
    for (size_t j = 0; j < n; ++j) mom[(size_t)n_classes * n + j] += mom[(size_t)c * n + j];
}

// ---- curve -----------------------------------------------------------------------------------------------------------------------
struct CurveWork { unsigned long long *M, *S; };                                       // M: the moments, merged as the replay goes; S uint64[K][3]

static CurveWork curve_carve(void* work, int K, int n_tables) {
  CurveWork w;
  w.M = (unsigned long long*)work;
  w.S = w.M + (size_t)n_tables * K * kLadderFields;
  return w;
}

// one thread per (row, table): the row's term of curve[t][0]; table 0's threads also write the row state S = n * row
__global__ __launch_bounds__(256) void palette_curve_init_kernel(const uint8_t* __restrict__ pal, const unsigned long long* __restrict__ counts, int K,
                                                                 CurveWork w, unsigned long long* __restrict__ curve) {
  __shared__ unsigned long long s_red[256 / 64];
  const int j = blockIdx.x * 256 + threadIdx.x, t = blockIdx.y;
  unsigned long long term = 0ull;
  if (j < K) {
    term = curve_sse(w.M + ((size_t)t * K + j) * kLadderFields, remap_pack_px(pal + (size_t)j * 3));
    if (t == 0) {
      const uint32_t n = (uint32_t)counts[j];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) w.S[(size_t)j * 3 + ch] = (unsigned long long)n * pal[(size_t)j * 3 + ch];
    }
  }
  const unsigned long long total = block_sum(term, s_red);
  if (threadIdx.x == 0 && total) atomicAdd(&curve[(size_t)t * K], total);
}

__global__ __launch_bounds__(64) void palette_curve_chain_kernel(const uint8_t* __restrict__ pal, const unsigned long long* __restrict__ counts, int K,
                                                                 const int32_t* __restrict__ merges, int n_tables, CurveWork w,
                                                                 unsigned long long* __restrict__ curve) {
  __shared__ uint32_t s_n[kLadderMaxRows], s_c[kLadderMaxRows];
  const int lane = threadIdx.x;
  for (int j = lane; j < K; j += 64) {
    s_n[j] = (uint32_t)counts[j];
    s_c[j] = remap_pack_px(pal + (size_t)j * 3);
  }
  __syncthreads();
  unsigned long long cur = lane < n_tables ? curve[(size_t)lane * K] : 0ull;
  for (int s = 0; s < K - 1; ++s) {
    const int a = merges[s * 2], b = merges[s * 2 + 1];                                // (wave uniform, as everything that ends the loop)
    if (!ladder_step_ok(a, b, K)) break;
    const uint32_t na = s_n[a], nb = s_n[b], ca = s_c[a], cb = s_c[b], nn = na + nb;
    if (!na || !nb || nn < na) break;                                                  // not a merge of two live rows: the log ends here
    uint32_t ch = 0u;
    if (lane < 3) {                                                                    // lane ch owns channel ch of every S
      const unsigned long long sum = w.S[(size_t)a * 3 + lane] + w.S[(size_t)b * 3 + lane];
      w.S[(size_t)a * 3 + lane] = sum;
      ch = refine_mean(sum, nn) & 255u;
    }
    const uint32_t cn = (__shfl(ch, 0, 64) << 16) | (__shfl(ch, 1, 64) << 8) | __shfl(ch, 2, 64);
    if (lane < n_tables) {                                                             // lane t owns table t
      unsigned long long* ma = w.M + ((size_t)lane * K + a) * kLadderFields;
      const unsigned long long* mb = w.M + ((size_t)lane * K + b) * kLadderFields;
      unsigned long long m[kLadderFields];
      cur -= curve_sse(ma, ca) + curve_sse(mb, cb);
#pragma unroll
      for (int f = 0; f < kLadderFields; ++f) m[f] = ma[f] + mb[f];
      cur += curve_sse(m, cn);
#pragma unroll
      for (int f = 0; f < kLadderFields; ++f) ma[f] = m[f];
      curve[(size_t)lane * K + s + 1] = cur;
    }
    __syncthreads();                                                                   // every lane has read the two rows
    if (lane == 0) {
      s_n[a] = nn;
      s_c[a] = cn;
      s_n[b] = 0u;
    }
    __syncthreads();
  }
}

static int curve_check(rhccq_ctx* ctx, const void* palette, const void* counts, int32_t K, const void* merges, const void* moments, int32_t n_tables,
                       const void* curve) {
  if (!palette || !counts || !merges || !moments || !curve) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: null argument");
  if (K < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: K >= 1 is required");
  if (n_tables < 1 || n_tables > kLadderMaxTables) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: n_tables must be 1..17");
  if (((uintptr_t)counts & 7) || ((uintptr_t)moments & 7) || ((uintptr_t)curve & 7) || ((uintptr_t)merges & 3))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: misaligned counts, moments, curve (8) or merges (4)");
  if (K > kRemapMaxK) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_curve: at most 65536 colours");
  return 0;
}

// ---- rung ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRungBlock) void palette_rung_kernel(const uint8_t* __restrict__ pal, const unsigned long long* __restrict__ counts, int K,
                                                                  const int32_t* __restrict__ merges, int K_target, uint8_t* __restrict__ pal_out,
                                                                  unsigned long long* __restrict__ counts_out, int32_t* __restrict__ map,
                                                                  int32_t* __restrict__ k_out) {
  __shared__ uint16_t s_par[kLadderMaxRows], s_row[kLadderMaxRows];                    // a row's root (after the jumps); a root's output row
  __shared__ unsigned long long s_buf[kLadderMaxRows];                                 // one field per root at a time
  __shared__ unsigned long long s_sum[kRungBlock / 64];
  __shared__ int s_cnt[kRungBlock / 64], s_len[kRungBlock / 64], s_scan[kRungBlock / 64 + 1];
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;

  unsigned long long sum = 0ull;
  int live = 0, len = K - 1;                                                           // len: the steps before the first entry that is no merge
  for (int j = tid; j < K; j += nt) {
    const unsigned long long v = counts[j];
    sum += reduce_clamp(v);
    live += v != 0ull;
    s_par[j] = (uint16_t)j;
  }
  for (int s = tid; s < K - 1; s += nt)
    if (!ladder_step_ok(merges[s * 2], merges[s * 2 + 1], K)) len = min(len, s);
  sum = wave_sum(sum);
  live = wave_sum(live);
  for (int o = 32; o > 0; o >>= 1) len = min(len, __shfl_down(len, o, 64));
  if (lane == 0) {
    s_sum[wv] = sum;
    s_cnt[wv] = live;
    s_len[wv] = len;
  }
  __syncthreads();
  sum = 0ull;
  live = 0;
  for (int i = 0; i < nw; ++i) {
    sum += s_sum[i];
    live += s_cnt[i];
    len = min(len, s_len[i]);
  }
  if (live == 0 || sum > kReduceMaxSum) {                                              // (block uniform) the reduction's two data errors
    for (int j = tid; j < K_target * 3; j += nt) pal_out[j] = 0;
    for (int j = tid; j < K_target; j += nt) counts_out[j] = 0ull;
    for (int j = tid; j < K; j += nt) map[j] = -1;
    if (tid == 0) *k_out = live == 0 ? RHCCQ_E_ARG : RHCCQ_E_LIMIT;
    return;
  }
  const int steps = min(live > K_target ? live - K_target : 0, len);
  // a log written by rhccq_palette_reduce names every b once (a row dies once): no two lanes write one slot.  A log that repeats a b
  // stays in bounds but which link wins is not defined here (the host form keeps the last), so the forms agree on the reduction's logs only
  for (int s = tid; s < steps; s += nt) s_par[merges[s * 2 + 1]] = (uint16_t)merges[s * 2];     // (checked above: a < b < K; links go to lower rows)
  __syncthreads();
  // pointer jumping: a chain of links is shorter than K <= 2^12, and a round at least halves it (a racing read sees an ancestor too)
  for (int round = 0; (1 << round) < K; ++round) {
    for (int j = tid; j < K; j += nt) s_par[j] = s_par[s_par[j]];
    __syncthreads();
  }

  // n, then n * row per channel, per root: a pass per field through s_buf; lane t keeps the fields of the roots among rows [t R, (t + 1) R)
  const int R = (K + nt - 1) / nt, lo = min(K, tid * R), hi = min(K, lo + R);
  unsigned long long val[4][kRungRows];
#pragma unroll
  for (int f = 0; f < 4; ++f) {
    for (int j = tid; j < K; j += nt) s_buf[j] = 0ull;
    __syncthreads();
    for (int j = tid; j < K; j += nt) {
      const unsigned long long n = counts[j];
      if (n) atomicAdd(&s_buf[s_par[j]], f == 0 ? n : n * pal[(size_t)j * 3 + f - 1]);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kRungRows; ++i) val[f][i] = lo + i < hi ? s_buf[lo + i] : 0ull;
    __syncthreads();
  }
  // the clusters in ascending id order: a cluster is a root that gathered weight
  int mine = 0, k_live = 0;
#pragma unroll
  for (int i = 0; i < kRungRows; ++i) mine += val[0][i] != 0ull;
  int base = block_exscan(mine, s_scan, &k_live);
#pragma unroll
  for (int i = 0; i < kRungRows; ++i) {
    if (val[0][i] == 0ull) continue;
    s_row[lo + i] = (uint16_t)base;
    if (base < K_target) {                                                             // (more clusters than K_target: only under a log that ends early)
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) pal_out[base * 3 + ch] = (uint8_t)refine_mean(val[1 + ch][i], val[0][i]);
      counts_out[base] = val[0][i];
    }
    ++base;
  }
  __syncthreads();
  for (int j = tid; j < K; j += nt) map[j] = counts[j] ? (int)s_row[s_par[j]] : -1;
  for (int j = k_live * 3 + tid; j < K_target * 3; j += nt) pal_out[j] = 0;
  for (int j = k_live + tid; j < K_target; j += nt) counts_out[j] = 0ull;
  if (tid == 0) *k_out = k_live;
}

static int rung_check(rhccq_ctx* ctx, const void* palette, const void* counts, int32_t K, const void* merges, int32_t K_target, const void* palette_out,
                      const void* counts_out, const void* map, const void* k_out) {
  if (!palette || !counts || !merges || !palette_out || !counts_out || !map || !k_out) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_rung: null argument");
  if (K < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_rung: K >= 1 is required");
  if (K > kRemapMaxK) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_rung: at most 65536 colours");
  if (K_target < 1 || K_target > K) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_rung: K_target must be 1..K");
  if (((uintptr_t)counts & 7) || ((uintptr_t)counts_out & 7) || ((uintptr_t)map & 3) || ((uintptr_t)merges & 3) || ((uintptr_t)k_out & 3))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_rung: misaligned counts, counts_out (8), map, merges or k_out (4)");
  return 0;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_moments_lds_rows(int32_t n_classes) { return n_classes < 0 || n_classes > kRemapMaxClasses ? 0 : moments_lds_rows(n_classes); }

int rhccq_palette_moments(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                          void* idx_out, int32_t idx_elem_bytes, uint64_t* moments) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = moments_check(ctx, rgb, n_pixels, palette, K, cls, n_classes, idx_out, idx_elem_bytes, moments)) return rc;
  const size_t n_acc = (size_t)(n_classes + 1) * K * kLadderFields;
  RHCCQ_HIP(ctx, hipMemsetAsync(moments, 0, n_acc * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const dim3 grid(remap_blocks(n_pixels, (long long)ctx->compute_units * 8)), block(kRemapBlock);
  const bool lds = K <= moments_lds_rows(n_classes);
  unsigned long long* mom = (unsigned long long*)moments;
  index_dispatch(idx_out ? idx_elem_bytes : 4, [&](auto* t) {                          // (no index buffer: the 4-byte instance)
    using T = std::remove_pointer_t<decltype(t)>;
    if (lds)
      hipLaunchKernelGGL((palette_moments_kernel<T, true>), grid, block, n_acc * sizeof(uint64_t), ctx->stream, rgb, (long long)n_pixels, palette, (int)K,
                         cls, (int)n_classes, (T*)idx_out, mom);
    else
      hipLaunchKernelGGL((palette_moments_kernel<T, false>), grid, block, 0, ctx->stream, rgb, (long long)n_pixels, palette, (int)K, cls, (int)n_classes,
                         (T*)idx_out, mom);
  });
  if (n_classes > 0)
    hipLaunchKernelGGL(palette_moments_finish_kernel, dim3((unsigned)((K * kLadderFields + 255) / 256)), dim3(256), 0, ctx->stream, mom, (int)K,
                       (int)n_classes);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_moments_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                               void* idx_out, int32_t idx_elem_bytes, uint64_t* moments) {
  if (const int rc = moments_check(nullptr, rgb, n_pixels, palette, K, cls, n_classes, idx_out, idx_elem_bytes, moments)) return rc;
  for (size_t j = 0; j < (size_t)(n_classes + 1) * K * kLadderFields; ++j) moments[j] = 0;
  index_dispatch(idx_out ? idx_elem_bytes : 4, [&](auto* t) { moments_host(rgb, n_pixels, palette, K, cls, n_classes, (decltype(t))idx_out, moments); });
  return 0;
}

// the moments as the replay merges them, and S uint64[K][3]
int64_t rhccq_palette_curve_bytes(int32_t K, int32_t n_tables) {
  return K < 1 || n_tables < 1 || n_tables > kLadderMaxTables ? 0 : ((int64_t)n_tables * K * kLadderFields + (int64_t)K * 3) * (int64_t)sizeof(uint64_t);
}

int rhccq_palette_curve(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, const uint64_t* moments,
                        int32_t n_tables, void* work, int64_t work_bytes, uint64_t* curve) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: null argument");
  if (const int rc = curve_check(ctx, palette, counts, K, merges, moments, n_tables, curve)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: misaligned workspace");
  if (K > kLadderMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_curve: more rows than rhccq_palette_reduce_max_rows() (the host form takes up to 65536)");
  if (work_bytes < rhccq_palette_curve_bytes(K, n_tables)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_curve: the workspace is smaller than rhccq_palette_curve_bytes(K, n_tables)");
  const CurveWork w = curve_carve(work, K, n_tables);
  const size_t n_mom = (size_t)n_tables * K * kLadderFields;
  RHCCQ_HIP(ctx, hipMemcpyAsync(w.M, moments, n_mom * sizeof(uint64_t), hipMemcpyDeviceToDevice, ctx->stream));
  RHCCQ_HIP(ctx, hipMemsetAsync(curve, 0, (size_t)n_tables * K * sizeof(uint64_t), ctx->stream));
  const unsigned long long* cnt = (const unsigned long long*)counts;
  hipLaunchKernelGGL(palette_curve_init_kernel, dim3((unsigned)((K + 255) / 256), (unsigned)n_tables), dim3(256), 0, ctx->stream, palette, cnt, (int)K, w,
                     (unsigned long long*)curve);
  hipLaunchKernelGGL(palette_curve_chain_kernel, dim3(1), dim3(64), 0, ctx->stream, palette, cnt, (int)K, merges, (int)n_tables, w,
                     (unsigned long long*)curve);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_curve_host(const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, const uint64_t* moments, int32_t n_tables,
                             uint64_t* curve) {
  if (const int rc = curve_check(nullptr, palette, counts, K, merges, moments, n_tables, curve)) return rc;
  const size_t n_mom = (size_t)n_tables * K * kLadderFields;
  std::vector<unsigned long long> M(moments, moments + n_mom), S((size_t)K * 3);
  std::vector<uint32_t> n(K), c(K);
  for (size_t j = 0; j < (size_t)n_tables * K; ++j) curve[j] = 0;
  for (int j = 0; j < K; ++j) {
    n[j] = (uint32_t)counts[j];
    c[j] = remap_pack_px(palette + (size_t)j * 3);
    for (int ch = 0; ch < 3; ++ch) S[(size_t)j * 3 + ch] = (unsigned long long)n[j] * palette[(size_t)j * 3 + ch];
    for (int t = 0; t < n_tables; ++t) curve[(size_t)t * K] += curve_sse(&M[((size_t)t * K + j) * kLadderFields], c[j]);
  }
  for (int s = 0; s < K - 1; ++s) {
    const int a = merges[s * 2], b = merges[s * 2 + 1];
    if (!ladder_step_ok(a, b, K)) break;
    const uint32_t na = n[a], nb = n[b], ca = c[a], cb = c[b], nn = na + nb;
    if (!na || !nb || nn < na) break;
    uint32_t ch[3];
    for (int i = 0; i < 3; ++i) {
      S[(size_t)a * 3 + i] += S[(size_t)b * 3 + i];
      ch[i] = refine_mean(S[(size_t)a * 3 + i], nn) & 255u;
    }
    const uint32_t cn = (ch[0] << 16) | (ch[1] << 8) | ch[2];
    for (int t = 0; t < n_tables; ++t) {
      unsigned long long* ma = &M[((size_t)t * K + a) * kLadderFields];
      const unsigned long long* mb = &M[((size_t)t * K + b) * kLadderFields];
      unsigned long long cur = curve[(size_t)t * K + s] - (curve_sse(ma, ca) + curve_sse(mb, cb));
      for (int f = 0; f < kLadderFields; ++f) ma[f] += mb[f];
      curve[(size_t)t * K + s + 1] = cur + curve_sse(ma, cn);
    }
    n[a] = nn;
    c[a] = cn;
    n[b] = 0u;
  }
  return 0;
}

int rhccq_palette_rung(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, int32_t K_target,
                       uint8_t* palette_out, uint64_t* counts_out, int32_t* map, int32_t* k_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = rung_check(ctx, palette, counts, K, merges, K_target, palette_out, counts_out, map, k_out)) return rc;
  if (K > kLadderMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_rung: more rows than rhccq_palette_reduce_max_rows() (the host form takes up to 65536)");
  const int lanes = K >= kRungBlock ? kRungBlock : (K + 63) / 64 * 64;
  hipLaunchKernelGGL(palette_rung_kernel, dim3(1), dim3((unsigned)lanes), 0, ctx->stream, palette, (const unsigned long long*)counts, (int)K, merges,
                     (int)K_target, palette_out, (unsigned long long*)counts_out, map, k_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_rung_host(const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, int32_t K_target, uint8_t* palette_out,
                            uint64_t* counts_out, int32_t* map, int32_t* k_out) {
  if (const int rc = rung_check(nullptr, palette, counts, K, merges, K_target, palette_out, counts_out, map, k_out)) return rc;
  unsigned long long sum = 0ull;
  int live = 0, len = 0;
  for (int j = 0; j < K; ++j) {
    sum += reduce_clamp(counts[j]);
    live += counts[j] != 0;
  }
  if (live == 0) return RHCCQ_E_ARG;
  if (sum > kReduceMaxSum) return RHCCQ_E_LIMIT;
  while (len < K - 1 && ladder_step_ok(merges[len * 2], merges[len * 2 + 1], K)) ++len;
  const int steps = std::min(live > K_target ? live - K_target : 0, len);
  std::vector<int32_t> par(K), row(K, -1);
  for (int j = 0; j < K; ++j) par[j] = j;
  for (int s = 0; s < steps; ++s) par[merges[s * 2 + 1]] = merges[s * 2];
  for (int j = 0; j < K; ++j) par[j] = par[par[j]];                                    // (links go to lower rows: those are at their roots already)
  std::vector<unsigned long long> val((size_t)K * 4, 0ull);
  for (int j = 0; j < K; ++j) {
    if (!counts[j]) continue;
    val[(size_t)par[j] * 4] += counts[j];
    for (int ch = 0; ch < 3; ++ch) val[(size_t)par[j] * 4 + 1 + ch] += counts[j] * palette[(size_t)j * 3 + ch];
  }
  int k_live = 0;
  for (int j = 0; j < K; ++j) {
    if (!val[(size_t)j * 4]) continue;
    row[j] = k_live;
    if (k_live < K_target) {
      for (int ch = 0; ch < 3; ++ch) palette_out[k_live * 3 + ch] = (uint8_t)refine_mean(val[(size_t)j * 4 + 1 + ch], val[(size_t)j * 4]);
      counts_out[k_live] = val[(size_t)j * 4];
    }
    ++k_live;
  }
  for (int j = 0; j < K; ++j) map[j] = counts[j] ? row[par[j]] : -1;
  for (int j = k_live; j < K_target; ++j) {
    palette_out[j * 3] = palette_out[j * 3 + 1] = palette_out[j * 3 + 2] = 0;
    counts_out[j] = 0;
  }
  *k_out = k_live;
  return 0;
}

}  // extern "C"
