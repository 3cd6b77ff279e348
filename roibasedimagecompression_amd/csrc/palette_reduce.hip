// Reduction of a given palette to K_target rows on the device (EXTENSION, no reference counterpart): pairwise-nearest-neighbour merging,
// Ward's criterion, in exact integers.  The definition is in include/rhccq.h; in short: a live cluster has a weight n, 64-bit channel
// sums S and an integer centre c; the pair a < b of least cost n_a n_b D(c_a, c_b) / (n_a + n_b) merges (ties: smallest a, then smallest
// b), a takes n_a + n_b, S_a + S_b and the centre floor((2 S + n) / (2 n)), b dies; rows of weight 0 never take part.
//
// Exactness.  The sum of the weights is at most 2^32 - 1, so n_a n_b < 2^62 and n_a + n_b < 2^32; D <= 3 * 255^2 < 2^18.  Two costs are
// compared by cross-multiplication, (n_a n_b D) (n_c + n_d) against (n_c n_d D') (n_a + n_b): each side is below 2^112 and is formed
// in unsigned __int128 (reduce_less).  A key carries {n_a n_b, D, n_a + n_b, index}; the index breaks ties and makes the order total.
//
// Structure.  Every live row r remembers its nearest partner of HIGHER id, nn[r] = argmin over live s > r of cost(r, s), ties to the
// lowest s.  The pair of least cost with the smallest a, then the smallest b, is then (r, nn[r]) for the lowest r among the rows of
// minimal cost(r, nn[r]): one arg-min over the rows finds it.  After the merge of (a, b) only these entries can be stale:
//   nn[r] == a or nn[r] == b   r's partner moved or died: r scans its partners again,
//   r == a                      a moved: it scans again,
//   any other live r < a        cost(r, a) changed: r compares its partner with the moved a (a cost that went up does not matter:
//                               a was not r's partner, so r's partner was already no worse, and still is).
// Rows above a that did not point at b are untouched: their partners lie above them and none of those changed.
//
// Device form: three launches on the context stream, no host synchronisation.
//   prep    one thread per row: n = counts, c = the packed row, S = n * row into the workspace.
//   table   one wave per row: the initial nn (K^2 / 2 costs over as many workgroups as it takes), into the workspace.
//   chain   ONE resident workgroup (the merge chain is sequential): n, c, nn and the list of rows to scan again live in LDS, 12 bytes
//           a row; S, touched only by the two rows of a merge, stays in the workspace.  A step is four barriers: arg-min (wave
//           butterflies on the key, 16 wave results through LDS) | merge (three lanes of wave 0, one per channel) | repair (every
//           row looks at its own entry; rows to scan again go on the list) | scan (one wave per listed row).  A dead row keeps the
//           row it merged into in its nn slot; the map follows those links at the end.
// Errors that only the data show (all counts zero; their sum above 2^32 - 1) cannot be returned without a synchronisation: the chain
// kernel writes RHCCQ_E_ARG or RHCCQ_E_LIMIT to *k_out and zero outputs (map and merges -1).
#include "palette_remap.h"

#include <vector>

namespace rhccq {

// kReduceMaxRows, kReduceMaxSum, reduce_clamp and refine_mean (the merged centre) are in palette_remap.h: the ladder shares them
constexpr int kReduceBlock = 1024;                    // lanes of the resident workgroup at K >= 1024 (smaller palettes take fewer waves)
constexpr int kReduceWaves = kReduceBlock / 64;
constexpr uint32_t kReduceNoIdx = 0xFFFFFFFFu;
constexpr uint16_t kReduceNoRow = 0xFFFFu;
static_assert(kReduceMaxRows < kReduceNoRow && kReduceMaxRows * 12 + 1024 <= 64 * 1024 && kReduceWaves == 16, "LDS layout of the chain kernel");

typedef unsigned __int128 reduce_u128;

// cost = w * d / den of the pair the key stands for; idx: the row (arg-min over rows) or the partner (scan) it belongs to
struct ReduceKey { unsigned long long w; uint32_t d, den, idx; };

// the squared distance of two packed centres, the remap's arithmetic (|a|^2 + |b|^2 - 2 a.b in integers)
__host__ __device__ __forceinline__ uint32_t reduce_dist(uint32_t a, uint32_t b) { return remap_dot(a, a) + remap_dot(b, b) - 2u * remap_dot(a, b); }

__host__ __device__ __forceinline__ ReduceKey reduce_key(uint32_t na, uint32_t ca, uint32_t nb, uint32_t cb, uint32_t idx) {
  return {(unsigned long long)na * nb, reduce_dist(ca, cb), na + nb, idx};
}
__host__ __device__ __forceinline__ ReduceKey reduce_no_key() { return {0ull, 0u, 1u, kReduceNoIdx}; }

// x before y: the smaller cost, exactly; equal costs: the lower index; a key without a pair is after every other
__host__ __device__ __forceinline__ bool reduce_less(const ReduceKey& x, const ReduceKey& y) {
  if (y.idx == kReduceNoIdx) return x.idx != kReduceNoIdx;
  if (x.idx == kReduceNoIdx) return false;
  const reduce_u128 l = (reduce_u128)x.w * x.d * y.den, r = (reduce_u128)y.w * y.d * x.den;
  return l < r || (l == r && x.idx < y.idx);
}

// r's best partner among the live rows first, first + step, ... < K (first > r); ascending order and a strict comparison keep the lowest
__host__ __device__ __forceinline__ ReduceKey reduce_scan(int r, int K, const uint32_t* n, const uint32_t* c, int first, int step) {
  ReduceKey best = reduce_no_key();
  const uint32_t nr = n[r], cr = c[r];
  for (int s = first; s < K; s += step) {
    if (!n[s]) continue;
    const ReduceKey k = reduce_key(nr, cr, n[s], c[s], (uint32_t)s);
    if (reduce_less(k, best)) best = k;
  }
  return best;
}

__device__ __forceinline__ ReduceKey reduce_shfl_xor(const ReduceKey& k, int o) {
  ReduceKey t;
  t.w = __shfl_xor(k.w, o, 64);
  t.d = __shfl_xor(k.d, o, 64);
  t.den = __shfl_xor(k.den, o, 64);
  t.idx = __shfl_xor(k.idx, o, 64);
  return t;
}
// the first key of the wave's (of its lowest 2 * from lanes') in every lane: the order is total, so every lane ends on the same key
__device__ __forceinline__ ReduceKey reduce_wave_min(ReduceKey k, int from = 32) {
  for (int o = from; o > 0; o >>= 1) {
    const ReduceKey t = reduce_shfl_xor(k, o);
    if (reduce_less(t, k)) k = t;
  }
  return k;
}

struct ReduceWork { unsigned long long* S; uint32_t *n, *c; uint16_t* nn; };

static ReduceWork reduce_carve(void* work, int K) {
  char* p = (char*)work;
  ReduceWork w;
  w.S = (unsigned long long*)p;
  w.n = (uint32_t*)(p + (size_t)K * 24);
  w.c = w.n + K;
  w.nn = (uint16_t*)(w.c + K);
  return w;
}

__global__ __launch_bounds__(256) void palette_reduce_prep_kernel(const uint8_t* __restrict__ pal, const unsigned long long* __restrict__ counts, int K,
                                                                  ReduceWork w) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  const uint32_t n = (uint32_t)counts[j];                                              // (a count that does not fit ends the chain kernel before it is used)
  w.n[j] = n;
  w.c[j] = remap_pack_px(pal + (size_t)j * 3);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) w.S[(size_t)j * 3 + ch] = (unsigned long long)n * pal[(size_t)j * 3 + ch];
}

__global__ __launch_bounds__(256) void palette_reduce_table_kernel(int K, ReduceWork w) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= K) return;                                                                  // (wave uniform)
  ReduceKey k = reduce_no_key();
  if (w.n[r]) k = reduce_wave_min(reduce_scan(r, K, w.n, w.c, r + 1 + lane, 64));
  if (lane == 0) w.nn[r] = k.idx == kReduceNoIdx ? kReduceNoRow : (uint16_t)k.idx;
}

__global__ __launch_bounds__(kReduceBlock) void palette_reduce_chain_kernel(const unsigned long long* __restrict__ counts, int K, int K_target, ReduceWork w,
                                                                            uint8_t* __restrict__ pal_out, unsigned long long* __restrict__ counts_out,
                                                                            int32_t* __restrict__ map, int32_t* __restrict__ merges, int32_t* __restrict__ k_out) {
  __shared__ uint32_t s_n[kReduceMaxRows], s_c[kReduceMaxRows];
  __shared__ uint16_t s_nn[kReduceMaxRows], s_list[kReduceMaxRows];                    // s_list: rows to scan again; at the end a live row's output row
  __shared__ ReduceKey s_key[kReduceWaves];
  __shared__ unsigned long long s_sum[kReduceWaves];
  __shared__ int s_cnt[kReduceWaves];
  __shared__ int s_nlist;
  const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wv = tid >> 6, nw = nt >> 6;

  unsigned long long sum = 0ull;
  int live = 0;
  for (int j = tid; j < K; j += nt) {
    s_n[j] = w.n[j];
    s_c[j] = w.c[j];
    s_nn[j] = w.nn[j];
    const unsigned long long v = counts[j];
    sum += reduce_clamp(v);
    live += v != 0ull;
  }
  sum = wave_sum(sum);
  live = wave_sum(live);
  if (lane == 0) {
    s_sum[wv] = sum;
    s_cnt[wv] = live;
  }
  __syncthreads();
  sum = 0ull;
  live = 0;
  for (int i = 0; i < nw; ++i) {
    sum += s_sum[i];
    live += s_cnt[i];
  }
  if (live == 0 || sum > kReduceMaxSum) {                                              // (block uniform)
    for (int j = tid; j < K_target * 3; j += nt) pal_out[j] = 0;
    for (int j = tid; j < K_target; j += nt) counts_out[j] = 0ull;
    for (int j = tid; j < K; j += nt) map[j] = -1;
    if (merges)
      for (int j = tid; j < (K - 1) * 2; j += nt) merges[j] = -1;
    if (tid == 0) *k_out = live == 0 ? RHCCQ_E_ARG : RHCCQ_E_LIMIT;
    return;
  }
  const int steps = live > K_target ? live - K_target : 0;
  __syncthreads();                                                                     // (s_cnt is used again below)

  int done = 0;
  for (; done < steps; ++done) {
    // arg-min over the rows: the lowest row among those of least cost to their partner
    ReduceKey best = reduce_no_key();
    for (int r = tid; r < K; r += nt) {
      const uint32_t p = s_nn[r];
      if (!s_n[r] || p == kReduceNoRow) continue;
      const ReduceKey k = reduce_key(s_n[r], s_c[r], s_n[p], s_c[p], (uint32_t)r);
      if (reduce_less(k, best)) best = k;
    }
    best = reduce_wave_min(best);
    if (lane == 0) s_key[wv] = best;
    __syncthreads();
    best = (lane & (kReduceWaves - 1)) < nw ? s_key[lane & (kReduceWaves - 1)] : reduce_no_key();
    best = reduce_wave_min(best, kReduceWaves / 2);
    if (best.idx == kReduceNoIdx) break;                                               // (fewer than two live rows: cannot happen while done < steps; block uniform)
    const int a = (int)best.idx, b = (int)s_nn[a];

    // the merge: lanes 0..2 of wave 0 take one channel each
    if (wv == 0) {
      const uint32_t nn_ = s_n[a] + s_n[b];
      uint32_t ch = 0u;
      if (lane < 3) {
        const unsigned long long s = w.S[(size_t)a * 3 + lane] + w.S[(size_t)b * 3 + lane];
        w.S[(size_t)a * 3 + lane] = s;
        ch = refine_mean(s, nn_);
      }
      const uint32_t c = (__shfl(ch, 0, 64) << 16) | (__shfl(ch, 1, 64) << 8) | __shfl(ch, 2, 64);
      if (lane == 0) {
        s_n[a] = nn_;
        s_c[a] = c;
        s_n[b] = 0u;
        s_nn[b] = (uint16_t)a;                                                         // a dead row's slot: the row it went into
        s_nlist = 0;
        if (merges) {
          merges[done * 2] = a;
          merges[done * 2 + 1] = b;
        }
      }
    }
    __syncthreads();

    // repair: every live row looks at its own entry
    const uint32_t na = s_n[a], ca = s_c[a];
    for (int r = tid; r < K; r += nt) {
      if (!s_n[r]) continue;
      const uint32_t p = s_nn[r];
      if (r == a || p == (uint32_t)a || p == (uint32_t)b) {
        s_list[atomicAdd(&s_nlist, 1)] = (uint16_t)r;                                  // (each row at most once: at most K entries)
      } else if (r < a) {                                                              // (a live row below a live row has a partner)
        const ReduceKey ka = reduce_key(s_n[r], s_c[r], na, ca, (uint32_t)a), kp = reduce_key(s_n[r], s_c[r], s_n[p], s_c[p], p);
        if (reduce_less(ka, kp)) s_nn[r] = (uint16_t)a;
      }
    }
    __syncthreads();

    // scan: one wave per listed row
    const int nl = s_nlist;
    for (int i = wv; i < nl; i += nw) {
      const int r = (int)s_list[i];
      const ReduceKey k = reduce_wave_min(reduce_scan(r, K, s_n, s_c, r + 1 + lane, 64));
      if (lane == 0) s_nn[r] = k.idx == kReduceNoIdx ? kReduceNoRow : (uint16_t)k.idx;
    }
    __syncthreads();
  }

  // the live rows in ascending order: thread t numbers the rows [t R, (t + 1) R)
  const int R = (K + nt - 1) / nt, lo = min(K, tid * R), hi = min(K, lo + R);
  int mine = 0;
  for (int r = lo; r < hi; ++r) mine += s_n[r] != 0u;
  int inc = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_cnt[wv] = inc;
  __syncthreads();
  int base = inc - mine;
  for (int i = 0; i < wv; ++i) base += s_cnt[i];
  for (int r = lo; r < hi; ++r)
    if (s_n[r]) s_list[r] = (uint16_t)base++;
  __syncthreads();

  const int k_live = live - done;                                                      // = min(K_target, live)
  for (int j = tid; j < K; j += nt) {
    if (s_n[j]) {
      const int i = (int)s_list[j];
      map[j] = i;
      if (i >= K_target) continue;                                                     // (cannot happen: the chain ends at K_target live rows)
      pal_out[i * 3] = (uint8_t)(s_c[j] >> 16);
      pal_out[i * 3 + 1] = (uint8_t)(s_c[j] >> 8);
      pal_out[i * 3 + 2] = (uint8_t)s_c[j];
      counts_out[i] = s_n[j];
    } else if (s_nn[j] == kReduceNoRow) {
      map[j] = -1;                                                                     // empty from the start
    } else {
      int r = (int)s_nn[j];
      for (int g = 0; g < K && r < K && !s_n[r]; ++g) r = (int)s_nn[r];                // (links go to lower rows: at most K of them)
      map[j] = r < K ? (int)s_list[r] : -1;
    }
  }
  for (int j = k_live * 3 + tid; j < K_target * 3; j += nt) pal_out[j] = 0;
  for (int j = k_live + tid; j < K_target; j += nt) counts_out[j] = 0ull;
  if (merges)
    for (int j = done * 2 + tid; j < (K - 1) * 2; j += nt) merges[j] = -1;
  if (tid == 0) *k_out = k_live;
}

static int reduce_check(rhccq_ctx* ctx, const void* palette, const void* counts, int32_t K, int32_t K_target, const void* palette_out,
                        const void* counts_out, const void* map, const void* merges, const void* k_out) {
  if (!palette || !counts || !palette_out || !counts_out || !map || !k_out) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: null argument");
  if (K < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: K >= 1 is required");
  if (K > kRemapMaxK) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_reduce: at most 65536 colours");
  if (K_target < 1 || K_target > K) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: K_target must be 1..K");
  if (((uintptr_t)counts & 7) || ((uintptr_t)counts_out & 7) || ((uintptr_t)map & 3) || ((uintptr_t)merges & 3) || ((uintptr_t)k_out & 3))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: misaligned counts, counts_out (8), map, merges or k_out (4)");
  return 0;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_reduce_max_rows(void) { return kReduceMaxRows; }

// S uint64[K][3], n and c uint32[K], nn uint16[K], rounded up to 8 bytes
int64_t rhccq_palette_reduce_bytes(int32_t K) { return K < 1 ? 0 : (int64_t)K * 32 + (((int64_t)K * 2 + 7) & ~(int64_t)7); }

int rhccq_palette_reduce(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, int32_t K_target, void* work, int64_t work_bytes,
                         uint8_t* palette_out, uint64_t* counts_out, int32_t* map, int32_t* merges, int32_t* k_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: null argument");
  if (const int rc = reduce_check(ctx, palette, counts, K, K_target, palette_out, counts_out, map, merges, k_out)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: misaligned workspace");
  if (K > kReduceMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_reduce: more rows than rhccq_palette_reduce_max_rows() (the host form takes up to 65536)");
  if (work_bytes < rhccq_palette_reduce_bytes(K)) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_reduce: the workspace is smaller than rhccq_palette_reduce_bytes(K)");
  const ReduceWork w = reduce_carve(work, K);
  const unsigned long long* cnt = (const unsigned long long*)counts;
  hipLaunchKernelGGL(palette_reduce_prep_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, ctx->stream, palette, cnt, (int)K, w);
  hipLaunchKernelGGL(palette_reduce_table_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, ctx->stream, (int)K, w);
  const int lanes = K >= kReduceBlock ? kReduceBlock : (K + 63) / 64 * 64;
  hipLaunchKernelGGL(palette_reduce_chain_kernel, dim3(1), dim3((unsigned)lanes), 0, ctx->stream, cnt, (int)K, (int)K_target, w, palette_out,
                     (unsigned long long*)counts_out, map, merges, k_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_reduce_host(const uint8_t* palette, const uint64_t* counts, int32_t K, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out,
                              int32_t* map, int32_t* merges, int32_t* k_out) {
  if (const int rc = reduce_check(nullptr, palette, counts, K, K_target, palette_out, counts_out, map, merges, k_out)) return rc;
  unsigned long long sum = 0ull;
  int live = 0;
  for (int j = 0; j < K; ++j) {
    sum += reduce_clamp(counts[j]);
    live += counts[j] != 0;
  }
  if (live == 0) return RHCCQ_E_ARG;
  if (sum > kReduceMaxSum) return RHCCQ_E_LIMIT;
  std::vector<uint32_t> n(K), c(K), nn(K);                                             // nn: the partner; of a dead row, the row it went into
  std::vector<unsigned long long> S((size_t)K * 3);
  for (int j = 0; j < K; ++j) {
    n[j] = (uint32_t)counts[j];
    c[j] = remap_pack_px(palette + (size_t)j * 3);
    for (int ch = 0; ch < 3; ++ch) S[(size_t)j * 3 + ch] = (unsigned long long)n[j] * palette[(size_t)j * 3 + ch];
  }
  for (int r = 0; r < K; ++r) nn[r] = n[r] ? reduce_scan(r, K, n.data(), c.data(), r + 1, 1).idx : kReduceNoIdx;
  const int steps = live > K_target ? live - K_target : 0;
  for (int done = 0; done < steps; ++done) {
    ReduceKey best = reduce_no_key();
    for (int r = 0; r < K; ++r) {
      const uint32_t p = nn[r];
      if (!n[r] || p == kReduceNoIdx) continue;
      const ReduceKey k = reduce_key(n[r], c[r], n[p], c[p], (uint32_t)r);
      if (reduce_less(k, best)) best = k;
    }
    const uint32_t a = best.idx, b = nn[a];
    n[a] += n[b];
    uint32_t ch[3];
    for (int i = 0; i < 3; ++i) {
      S[(size_t)a * 3 + i] += S[(size_t)b * 3 + i];
      ch[i] = refine_mean(S[(size_t)a * 3 + i], n[a]);
    }
    c[a] = (ch[0] << 16) | (ch[1] << 8) | ch[2];
    n[b] = 0u;
    nn[b] = a;
    if (merges) {
      merges[done * 2] = (int32_t)a;
      merges[done * 2 + 1] = (int32_t)b;
    }
    for (int r = 0; r < K; ++r) {
      if (!n[r]) continue;
      const uint32_t p = nn[r];
      if ((uint32_t)r == a || p == a || p == b) {
        nn[r] = reduce_scan(r, K, n.data(), c.data(), r + 1, 1).idx;
      } else if ((uint32_t)r < a) {
        if (reduce_less(reduce_key(n[r], c[r], n[a], c[a], a), reduce_key(n[r], c[r], n[p], c[p], p))) nn[r] = a;
      }
    }
  }
  std::vector<int32_t> row(K, -1);
  int k_live = 0;
  for (int j = 0; j < K; ++j) {
    if (!n[j]) continue;
    row[j] = k_live;
    palette_out[k_live * 3] = (uint8_t)(c[j] >> 16);
    palette_out[k_live * 3 + 1] = (uint8_t)(c[j] >> 8);
    palette_out[k_live * 3 + 2] = (uint8_t)c[j];
    counts_out[k_live++] = n[j];
  }
  for (int j = 0; j < K; ++j) {
    uint32_t r = (uint32_t)j;
    while (r != kReduceNoIdx && !n[r]) r = nn[r];                                      // (links go to lower rows; an empty row's is none)
    map[j] = r == kReduceNoIdx ? -1 : row[r];
  }
  for (int j = k_live; j < K_target; ++j) {
    palette_out[j * 3] = palette_out[j * 3 + 1] = palette_out[j * 3 + 2] = 0;
    counts_out[j] = 0;
  }
  if (merges)
    for (int j = steps * 2; j < (K - 1) * 2; ++j) merges[j] = -1;
  *k_out = k_live;
  return 0;
}

}  // extern "C"
