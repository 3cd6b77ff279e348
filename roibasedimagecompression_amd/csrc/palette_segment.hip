// Exact row segmentation onto a given palette (EXTENSION, no reference counterpart).  For every image row the labelling out(x) that minimises
//     sum_x |p(x) - palette[out(x)]|^2  +  sum_{x >= 1, out(x) != out(x-1)} pen(x)
// (the 1-D Potts problem) by its K-state dynamic programme, in exact integers; pen(x) = penalty[cls(y, x)] with the class convention of
// rhccq_palette_runs.  The rule, pinned bit for bit (include/rhccq.h states it in full):
//     forward    C_0(c) = d(0, c);  x >= 1:  m = min_c C_{x-1}(c), a(x) the lowest c attaining it, stay(x, c) <=> C_{x-1}(c) <= m + pen(x),
//                C_x(c) = d(x, c) + min(C_{x-1}(c), m + pen(x))
//     backward   out(W-1) = the lowest c attaining min C_{W-1};  out(x-1) = stay(x, out(x)) ? out(x) : a(x)
// The step / key / pack functions are in palette_segment.h; the host form runs them serially.
//
// The kernel.  A workgroup is ONE wave and owns ONE image row.  State c lives in lane c % 64, slot c / 64; the kernel is a template on
// the slots S = ceil(K / 64) (1..16), so the per-state loops unroll and costs, inverted rows and |row|^2 stay in registers.
//   forward   the row goes by in tiles of 32 columns.  All lanes load the tile's pixels and classes (one pixel a lane, the next tile's
//             loads in flight behind this tile's steps); a column's pixel and penalty reach the scalar unit with v_readlane.  A step of one
//             state is v_dot4_u32_u8, v_lshl_add (the key), a subtraction, v_alignbit (the stay bit into the slot's dword), a minimum
//             and a three-operand addition; they are independent across states.  The loop-carried part is the wave-wide minimum: a
//             lane's minimum over its slots (costs are kept packed with their slot, palette_segment.h), four DPP steps (two quad permutations, row_half_mirror, row_mirror) that leave
//             every row of 16 lanes with its minimum, four v_readlane and three scalar minima.  No LDS on the chain.  a(x) is the
//             packed minimum's slot and the lowest lane that holds it (one compare, one s_ff1); lane j of the tile keeps that of column j.
//             After 32 columns the lane stores its S dwords of stay bits (column j of the tile in bit 31 - j) and lanes 0..31 their
//             a(x): coalesced vector stores, 256 S + 64 bytes a tile.
//   backward  behind the forward pass of the same row, tiles from the right.  The record of a tile does not depend on the chain: every
//             lane loads back the dwords it stored itself (so no fence is needed), one tile ahead, with the tile's pixels, classes and nearest rows, and
//             puts the stay words into LDS, indexed by state.  The walk is wave-uniform and takes one step per BREAK, not per pixel:
//             the current row's word, bit-reversed and inverted, shows the next column (from the right) where it does not stay; all
//             columns up to it take the row, and the row becomes a(x) there.  Lanes 0..31 then write out(x) in the caller's width and add
//             the squared error, out != b and the breaks to their sums.
// The workspace is the full plane: H x ceil(W / 32) tile records (282 MB at 3840 x 2160 with K = 230).  A persistent grid with only the rows in
// flight would need far less, but the plane keeps the launch a plain one-row-per-workgroup grid and the workspace comes from the caller.
// b (for the third sum) is rhccq_palette_remap's, run into idx_out before the launch, as rhccq_palette_runs does.
// Sums: a lane's class slots in LDS as in palette_runs.hip; 4 (n_classes + 1) global atomics per workgroup at the end.
#include <new>
#include <vector>

#include "palette_segment.h"
#include "wave_dpp.h"

namespace rhccq {

static int seg_slots(int K) { return (K + kSegLanes - 1) / kSegLanes; }

// unsigned minimum over the wave, returned wave-uniform.  DPP moves only: the butterfly of wave_dpp.h gives every row of 16 lanes its
// minimum; lanes 0, 16, 32 and 48 go to the scalar unit
__device__ __forceinline__ uint32_t seg_wave_min(uint32_t v) {
  v = dpp_group_min<16>(v);
  const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), r1 = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
  const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), r3 = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
  // scalar minima, by name: the compiler would move the four values back to vector registers for one v_min3 and keep every use of the
  // minimum (the compare, a(x), the column constants) on the vector unit, where the chain of the wave's other rows competes for issue
  uint32_t m01, m23, m;
  asm("s_min_u32 %0, %1, %2" : "=s"(m01) : "s"(r0), "s"(r1) : "scc");
  asm("s_min_u32 %0, %1, %2" : "=s"(m23) : "s"(r2), "s"(r3) : "scc");
  asm("s_min_u32 %0, %1, %2" : "=s"(m) : "s"(m01), "s"(m23) : "scc");
  return m;
}

// the minimum of the packed costs (<< 4, as the steps take it) and the lowest state that attains it
template <int S>
__device__ __forceinline__ void seg_min(const int32_t (&cost)[S], int32_t& m, uint32_t& a) {
  uint32_t lm = (uint32_t)cost[0];
#pragma unroll
  for (int s = 1; s < S; ++s) lm = min(lm, (uint32_t)cost[s]);
  const uint32_t wm = seg_wave_min(lm);
  const unsigned long long who = __ballot(lm == wm);
  m = (int32_t)(wm & ~15u);
  a = (wm & 15u) * kSegLanes + (uint32_t)__builtin_ctzll(who);
}

// a lane's pixel of a tile as loaded: nothing is computed from it before the tile's turn
struct SegTile {
  uint16_t rg;
  uint8_t bl;
  uint32_t k;
};

__device__ __forceinline__ void seg_load(SegTile& t, const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ cls, int n_classes, long long row,
                                         int W, int x0, int lane) {
  const long long p = row * W + min(x0 + (lane & (kSegCols - 1)), W - 1);
  __builtin_memcpy(&t.rg, rgb + p * 3, 2);
  t.bl = rgb[p * 3 + 2];
  t.k = cls ? (uint32_t)cls[p] : (uint32_t)n_classes;
}
__device__ __forceinline__ uint32_t seg_px(const SegTile& t) { return ((uint32_t)t.rg & 255u) << 16 | ((uint32_t)t.rg >> 8) << 8 | t.bl; }

__device__ __forceinline__ uint32_t seg_load_idx(const void* idx, int eb, long long p) {
  return eb == 1 ? (uint32_t)((const uint8_t*)idx)[p] : eb == 2 ? (uint32_t)((const uint16_t*)idx)[p] : ((const uint32_t*)idx)[p];
}

template <int S>
__global__ __launch_bounds__(kSegLanes) void palette_segment_kernel(const uint8_t* __restrict__ rgb, int H, int W, const uint8_t* __restrict__ pal, int K,
                                                                    const uint8_t* __restrict__ cls, int n_classes, SegPenalty pen, uint32_t* work,
                                                                    void* idx, int eb, unsigned long long* __restrict__ sums) {
  extern __shared__ unsigned long long s_dyn[];                                       // [n_classes][64] squared errors, then the counts
  __shared__ uint32_t s_pen[kRemapMaxClasses + 1];
  __shared__ uint32_t s_pal[S * kSegLanes];                                           // the palette's colours, by state
  __shared__ uint32_t s_bits[S * kSegLanes];                                          // the stay words of the tile the walk is in, by state
  __shared__ unsigned long long s_tot[3];
  const int lane = threadIdx.x;
  const long long y = blockIdx.x;
  const int nT = (W + kSegCols - 1) / kSegCols;
  uint32_t* wrow = work + y * nT * seg_tile_words(S);
  unsigned long long* s_sse = s_dyn;
  uint32_t* s_cnt = reinterpret_cast<uint32_t*>(s_sse + n_classes * kSegLanes);      // [3][n_classes][64]: pixels, out != b, breaks

  SegTile t;
  seg_load(t, rgb, cls, n_classes, y, W, 0, lane);
  uint32_t inv[S];
  int32_t n2[S], cost[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const int c = s * kSegLanes + lane;
    const uint32_t col = c < K ? remap_pack_px(pal + (long long)c * 3) : 0u;
    s_pal[c] = col;
    inv[s] = c < K ? seg_inv(col) : 0u;
    n2[s] = (c < K ? (int32_t)remap_dot(col, col) : kSegPad) << 4;
    cost[s] = s;
  }
  for (int i = lane; i < n_classes * kSegLanes; i += kSegLanes) { s_sse[i] = 0ull; s_cnt[i] = 0u; s_cnt[n_classes * kSegLanes + i] = 0u; s_cnt[2 * n_classes * kSegLanes + i] = 0u; }
  if (lane <= n_classes) s_pen[lane] = pen.v[lane];
  __syncthreads();

  // ---- forward
  for (int ti = 0; ti < nT; ++ti) {
    const int x0 = ti * kSegCols, tw = min(kSegCols, W - x0);
    const uint32_t px_v = seg_px(t);
    const uint32_t pen_v = x0 + lane == 0 ? 0u : s_pen[min(t.k, (uint32_t)n_classes)];   // all costs are 0 before column 0: C_0 = the key
    if (ti + 1 < nT) seg_load(t, rgb, cls, n_classes, y, W, x0 + kSegCols, lane);         // lands behind the steps below
    uint32_t bits[S], a_v = 0u;
#pragma unroll
    for (int s = 0; s < S; ++s) bits[s] = 0u;
    auto column = [&](int j) {                                                            // (j is wave uniform)
      const uint32_t p = (uint32_t)__builtin_amdgcn_readlane((int)px_v, j);
      const int32_t pn = __builtin_amdgcn_readlane((int)pen_v, j);
      int32_t m;
      uint32_t a;
      seg_min<S>(cost, m, a);
      a_v = lane == j ? a : a_v;
      // the two column constants through readfirstlane and the key through an empty asm: left to itself the compiler takes the sums
      // apart again and spends two more additions a state
      const int32_t pen1 = __builtin_amdgcn_readfirstlane((pn + 1) << 4), mp1 = __builtin_amdgcn_readfirstlane(m + pen1);
#pragma unroll
      for (int s = 0; s < S; ++s) {
        int32_t key = seg_key(p, inv[s], n2[s]);
        asm("" : "+v"(key));
        seg_step(cost[s], bits[s], key, mp1, pen1, s);
      }
    };
    if (tw == kSegCols) {                                                                 // every tile of a row but its last
#pragma unroll 4
      for (int j = 0; j < kSegCols; ++j) column(j);
    } else {
#pragma nounroll
      for (int j = 0; j < tw; ++j) column(j);
    }
    uint32_t* rec = wrow + ti * seg_tile_words(S);
#pragma unroll
    for (int s = 0; s < S; ++s) rec[s * kSegLanes + lane] = bits[s] << (kSegCols - tw);   // column j of the tile in bit 31 - j
    if (lane < kSegCols) reinterpret_cast<uint16_t*>(rec + S * kSegLanes)[lane] = (uint16_t)a_v;
  }
  int32_t m_last;
  uint32_t c;                                                                             // the row of the column the walk stands on
  seg_min<S>(cost, m_last, c);
  (void)m_last;

  // ---- backward: the walk, then the tile's outputs and sums
  unsigned long long all_sse = 0ull;
  uint32_t all_mov = 0u, all_brk = 0u;
  uint32_t bw[S], av, bv;
  auto load_back = [&](int ti) {
    const uint32_t* rec = wrow + ti * seg_tile_words(S);
#pragma unroll
    for (int s = 0; s < S; ++s) bw[s] = rec[s * kSegLanes + lane];                        // this lane's own stores
    av = reinterpret_cast<const uint16_t*>(rec + S * kSegLanes)[lane & (kSegCols - 1)];
    seg_load(t, rgb, cls, n_classes, y, W, ti * kSegCols, lane);
    bv = seg_load_idx(idx, eb, y * W + min(ti * kSegCols + (lane & (kSegCols - 1)), W - 1));
  };
  load_back(nT - 1);
  for (int ti = nT - 1; ti >= 0; --ti) {
    const int x0 = ti * kSegCols, tw = min(kSegCols, W - x0);
#pragma unroll
    for (int s = 0; s < S; ++s) s_bits[s * kSegLanes + lane] = __brev(bw[s]);            // column j in bit j
    const uint32_t a_t = av, b = bv, px = seg_px(t), k = min(t.k, (uint32_t)n_classes);
    __syncthreads();
    if (ti > 0) load_back(ti - 1);                                                        // lands behind the walk
    uint32_t out = 0u;
    int pos = tw - 1;
    while (pos >= 0) {                                                                    // (wave uniform: one turn per break)
      const uint32_t stay = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_bits[c]);
      const uint32_t leave = ~stay & (0xFFFFFFFFu >> (31 - pos));                         // columns <= pos whose left neighbour has another row
      const int j = leave ? 31 - __builtin_clz(leave) : 0;                                // the rightmost of them
      if (lane >= j && lane <= pos) out = c;
      if (leave) c = (uint32_t)__builtin_amdgcn_readlane((int)a_t, j);
      pos = leave ? j - 1 : -1;
    }
    // c is now out(x0 - 1)
    uint32_t left = (uint32_t)__shfl_up((int)out, 1, kSegLanes);
    if (lane == 0) left = c;
    if (lane < tw) {
      const long long p = y * W + x0 + lane;
      if (eb == 1) ((uint8_t*)idx)[p] = (uint8_t)out;
      else if (eb == 2) ((uint16_t*)idx)[p] = (uint16_t)out;
      else ((uint32_t*)idx)[p] = out;
      const uint32_t d = runs_dist(px, s_pal[out]), mov = out != b ? 1u : 0u, brk = (x0 + lane > 0 && out != left) ? 1u : 0u;
      all_sse += d;
      all_mov += mov;
      all_brk += brk;
      if (k < (uint32_t)n_classes) {                                                      // this lane's own slot: no other writer
        const int s = (int)k * kSegLanes + lane;
        s_sse[s] += d;
        s_cnt[s] += 1u;
        s_cnt[n_classes * kSegLanes + s] += mov;
        s_cnt[2 * n_classes * kSegLanes + s] += brk;
      }
    }
    __syncthreads();                                                                      // the next tile overwrites s_bits
  }
  all_sse = wave_sum(all_sse);
  all_mov = wave_sum(all_mov);
  all_brk = wave_sum(all_brk);
  if (lane == 0) { s_tot[0] = all_sse; s_tot[1] = all_mov; s_tot[2] = all_brk; }
  __syncthreads();
  for (int i = lane; i < (n_classes + 1) * 4; i += kSegLanes) {                           // one atomic per workgroup, row and column
    const int k = i / 4, col = i % 4;
    unsigned long long v = 0ull;
    if (k < n_classes) {
      for (int l = 0; l < kSegLanes; ++l)
        v += col == 1 ? s_sse[k * kSegLanes + l] : (unsigned long long)s_cnt[((col == 0 ? 0 : col - 1) * n_classes + k) * kSegLanes + l];
    } else {
      v = col == 0 ? (unsigned long long)W : s_tot[col - 1];
    }
    if (v) atomicAdd(&sums[i], v);
  }
}

static int seg_check(rhccq_ctx* ctx, const void* rgb, int32_t H, int32_t W, const void* palette, int32_t K, const void* cls, int32_t n_classes,
                     const uint32_t* penalty, const void* idx_out, int32_t idx_elem_bytes, const void* sums) {
  if (const int rc = rows_check(ctx, "palette_segment", rgb, H, W, palette, K, cls, n_classes, penalty, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i <= n_classes; ++i)
    if (penalty[i] > kSegMaxPenalty) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_segment: a penalty is at most 16777215");
  return search_limit(ctx, "palette_segment", K);
}

// the (packed, slot 0) cost of column x from that of column x - 1, and the column's a and stay bits (bit c % 64 of word c / 64 of `stay`)
static void seg_host_column(int32_t* cost, const uint32_t* inv, const int32_t* n2, int K, uint32_t px, int32_t pn, uint64_t* stay, uint32_t* a) {
  int32_t m = cost[0];
  uint32_t am = 0;
  for (int c = 1; c < K; ++c)
    if (cost[c] < m) { m = cost[c]; am = (uint32_t)c; }
  *a = am;
  for (int c = 0; c < K; ++c) {
    uint32_t bit = 0u;
    seg_step(cost[c], bit, seg_key(px, inv[c], n2[c]), m + ((pn + 1) << 4), (pn + 1) << 4, 0);
    if (bit & 1u) stay[c >> 6] |= 1ull << (c & 63);
  }
}

template <typename IdxT>
static int seg_host(const uint8_t* rgb, int H, int W, const uint8_t* pal, int K, const uint8_t* cls, int n_classes, const uint32_t* penalty,
                    IdxT* idx, uint64_t* sums) {
  const size_t nw = (size_t)(K + 63) / 64;
  std::vector<uint32_t> inv_v, a_v;
  std::vector<int32_t> n2_v, cost_v;
  std::vector<uint64_t> stay_v;
  try {
    inv_v.resize(K); n2_v.resize(K); cost_v.resize(K); a_v.resize(W); stay_v.resize(nw * W);
  } catch (const std::bad_alloc&) {
    return RHCCQ_E_LIMIT;
  }
  uint32_t *inv = inv_v.data(), *a = a_v.data();
  int32_t *n2 = n2_v.data(), *cost = cost_v.data();
  uint64_t* stay = stay_v.data();
  for (int c = 0; c < K; ++c) {
    const uint32_t col = remap_pack_px(pal + (long long)c * 3);
    inv[c] = seg_inv(col);
    n2[c] = (int32_t)remap_dot(col, col) << 4;
  }
  for (int y = 0; y < H; ++y) {
    for (int c = 0; c < K; ++c) cost[c] = 0;
    for (size_t i = 0; i < nw * W; ++i) stay[i] = 0ull;
    for (int x = 0; x < W; ++x) {
      const long long p = (long long)y * W + x;
      const int32_t pn = x == 0 ? 0 : (int32_t)penalty[runs_class(cls, p, n_classes)];
      seg_host_column(cost, inv, n2, K, remap_pack_px(rgb + p * 3), pn, stay + nw * x, a + x);
    }
    uint32_t c = 0;
    for (int j = 1; j < K; ++j)
      if (cost[j] < cost[c]) c = (uint32_t)j;
    for (int x = W - 1; x >= 0; --x) {
      const long long p = (long long)y * W + x;
      const uint32_t left = (stay[nw * x + (c >> 6)] >> (c & 63)) & 1ull ? c : a[x];     // out(x - 1); unused at x == 0
      const uint32_t b = (uint32_t)idx[p], k = runs_class(cls, p, n_classes);
      const uint64_t d = runs_dist(remap_pack_px(rgb + p * 3), remap_pack_px(pal + (long long)c * 3));
      const uint64_t mov = c != b ? 1 : 0, brk = x > 0 && c != left ? 1 : 0;
      idx[p] = (IdxT)c;
      rows_add_host(sums, k, n_classes, {1, d, mov, brk});
      c = left;
    }
  }
  return 0;
}

template <int S>
static void seg_launch(rhccq_ctx* ctx, const uint8_t* rgb, int H, int W, const uint8_t* pal, int K, const uint8_t* cls, int n_classes,
                       const SegPenalty& pen, void* work, void* idx, int eb, uint64_t* sums) {
  const size_t lds = (size_t)n_classes * kSegLanes * (8 + 3 * 4);                        // at most 20 480 bytes beside 8 KiB of static LDS
  hipLaunchKernelGGL(palette_segment_kernel<S>, dim3((unsigned)H), dim3(kSegLanes), lds, ctx->stream, rgb, H, W, pal, K, cls, n_classes, pen,
                     (uint32_t*)work, idx, eb, (unsigned long long*)sums);
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_segment_max_rows(void) { return kSegMaxRows; }
int32_t rhccq_palette_segment_tile_cols(void) { return kSegCols; }

int64_t rhccq_palette_segment_bytes(int32_t H, int32_t W, int32_t K) {
  if (H < 0 || W < 0 || K < 1 || K > kSegMaxRows) return 0;
  return (int64_t)H * ((W + kSegCols - 1) / kSegCols) * seg_tile_words(seg_slots(K)) * 4;
}

int rhccq_palette_segment(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                          int32_t n_classes, const uint32_t* penalty_host, void* work, int64_t work_bytes, void* idx_out, int32_t idx_elem_bytes,
                          uint64_t* sums) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = seg_check(ctx, rgb, H, W, palette, K, cls, n_classes, penalty_host, idx_out, idx_elem_bytes, sums)) return rc;
  if (K > kSegMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_segment: the device form holds at most 1024 colours");
  const size_t sums_bytes = (size_t)(n_classes + 1) * 4 * sizeof(uint64_t);
  const int64_t n = (int64_t)H * W;
  if (n == 0) {
    RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
    return 0;
  }
  if (!work || ((uintptr_t)work & 7) || work_bytes < rhccq_palette_segment_bytes(H, W, K))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_segment: a workspace of rhccq_palette_segment_bytes(H, W, K) bytes, aligned to 8, is required");
  // b into idx_out; the remap's own {pixels, SSE} land in the first two words of sums, which the memset behind it clears again
  if (const int rc = rhccq_palette_remap(ctx, rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, sums)) return rc;
  RHCCQ_HIP(ctx, hipMemsetAsync(sums, 0, sums_bytes, ctx->stream));
  SegPenalty pen{};
  for (int i = 0; i <= n_classes; ++i) pen.v[i] = penalty_host[i];
#define RHCCQ_SEG_CASE(S_) \
  case S_: seg_launch<S_>(ctx, rgb, H, W, palette, K, cls, n_classes, pen, work, idx_out, idx_elem_bytes, sums); break;
  switch (seg_slots(K)) {
    RHCCQ_SEG_CASE(1) RHCCQ_SEG_CASE(2) RHCCQ_SEG_CASE(3) RHCCQ_SEG_CASE(4) RHCCQ_SEG_CASE(5) RHCCQ_SEG_CASE(6) RHCCQ_SEG_CASE(7) RHCCQ_SEG_CASE(8)
    RHCCQ_SEG_CASE(9) RHCCQ_SEG_CASE(10) RHCCQ_SEG_CASE(11) RHCCQ_SEG_CASE(12) RHCCQ_SEG_CASE(13) RHCCQ_SEG_CASE(14) RHCCQ_SEG_CASE(15)
    default: seg_launch<16>(ctx, rgb, H, W, palette, K, cls, n_classes, pen, work, idx_out, idx_elem_bytes, sums);
  }
#undef RHCCQ_SEG_CASE
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_segment_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                               const uint32_t* penalty, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums) {
  if (const int rc = seg_check(nullptr, rgb, H, W, palette, K, cls, n_classes, penalty, idx_out, idx_elem_bytes, sums)) return rc;
  for (int i = 0; i < (n_classes + 1) * 4; ++i) sums[i] = 0;
  const int64_t n = (int64_t)H * W;
  if (n == 0) return 0;
  uint64_t remap_sums[2];
  if (const int rc = rhccq_palette_remap_host(rgb, n, palette, K, nullptr, 0, idx_out, idx_elem_bytes, remap_sums)) return rc;
  int rc = 0;
  index_dispatch(idx_elem_bytes, [&](auto* t) { rc = seg_host(rgb, H, W, palette, K, cls, n_classes, penalty, (decltype(t))idx_out, sums); });
  return rc;
}

}  // extern "C"
