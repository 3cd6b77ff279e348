// JPEG files written with Huffman tables made for the picture (EXTENSION, include/rhccq.h): a stage between the writer's blocks and its
// entropy launches that counts the scan's symbols and builds libjpeg's optimal tables from the counts, all on the device.  The definitions
// both sides share are in jpeg_optimize.h; the host forms at the end run them serially.
//
//   clear_kernel       the 4 x 256 counts.
//   histogram_kernel   a wave a block, a lane a zig-zag position, as the writer's count launch: one ballot gives the non-zero mask and every
//                      lane its run and symbol (lane_sym).  Lane 0 holds the DC size, lanes 1 .. 63 AC symbols.  Eight more ballots, one
//                      a symbol bit, give every lane the set of lanes that hold its symbol: the lowest of them adds the set's size with
//                      ONE LDS atomic, so a block of nothing but 0x01 codes costs one atomic, not 63 on one word.  ZRL counts (rare) go
//                      straight to 0xF0.  Workgroups are persistent: the grid is sized to the card and strides over the blocks in scan
//                      order; a workgroup's 4 x 256 LDS counts go out once, the non-zero ones, by global atomics.
//   huffman_kernel     one workgroup, a wave a table.  Lane l holds symbols l, l + 64, l + 128, l + 192 (lane 0 also the reserved 256):
//                      count, root, length, in registers.  A merge step: every lane's best and second-best (count ascending, symbol
//                      descending) from its five slots; a wave minimum of the counts and a wave maximum of the symbols at it give c1;
//                      the same over the other lanes' best and c1's lane's second-best give c2; then the update of jpeg_optimize.h's
//                      merge_serial on every slot.  At most 256 steps, four DPP reductions each.  Lengths -> bits[] by ballots, the fold
//                      by lane 0 in LDS, ranks by counting smaller keys in LDS, canonical codes.  After the barrier the waves write
//                      their DHT segments where the counts of codes in front of them put them, and all lanes copy the rest.
#include "jpeg_optimize.h"
#include "rhccq_common.h"
#include "wave_dpp.h"

#include <vector>

namespace rhccq {
namespace jpego {

using jpegw::args_ok;
using jpegw::frame_of;
using jpegw::kBlockBitsOpt;
using jpegw::kThreads;

// ---- counts --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void clear_kernel(uint32_t* __restrict__ counts) {
  for (int i = threadIdx.x; i < 4 * 256; i += kThreads) counts[i] = 0u;
}

__global__ __launch_bounds__(kThreads) void histogram_kernel(Frame f, const int16_t* __restrict__ coef, uint32_t* __restrict__ counts) {
  __shared__ uint32_t s_cnt[4 * 256];
  const Geo& g = f.g;
  for (int i = threadIdx.x; i < 4 * 256; i += kThreads) s_cnt[i] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long stride = 4ll * gridDim.x;
  for (long long A = 4ll * blockIdx.x + wave; A < g.blocks; A += stride) {   // (wave-uniform)
    const int t = comp_of(g, (int)(A % g.bpm)) ? 2 : 0;
    int32_t v = coef[64 * block_at(g, A) + zigzag(lane)];
    if (lane == 0) v -= jpegw::dc_pred(g, coef, A);
    const uint64_t mask = __ballot(lane > 0 && v != 0);
    const jpegw::LaneSym y = jpegw::lane_sym(lane, v, mask);
    if (lane == 0) atomicAdd(&s_cnt[256 * t + y.sym], 1u);
    const bool ac = lane > 0 && y.sym >= 0;
    uint64_t same = __ballot(ac);                            // the lanes that hold this lane's AC symbol
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = y.sym >> b & 1;
      const uint64_t set = __ballot(bit);
      same &= bit ? set : ~set;
    }
    if (ac && lane == __ffsll((long long)same) - 1) atomicAdd(&s_cnt[256 * (t + 1) + y.sym], (uint32_t)__popcll(same));
    if (y.zrl) atomicAdd(&s_cnt[256 * (t + 1) + 0xF0], (uint32_t)y.zrl);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 4 * 256; i += kThreads)
    if (s_cnt[i]) atomicAdd(&counts[i], s_cnt[i]);
}

// ---- tables --------------------------------------------------------------------------------------------------------------------------
// what one lane of another is to see of a wave's LDS: the stores in front are done and stay in front
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__global__ __launch_bounds__(kThreads) void huffman_kernel(Plan p, const uint32_t* __restrict__ counts, const Tables* __restrict__ in, Tables* __restrict__ out) {
  __shared__ uint32_t s_bits[4][kLenMax + 1];
  __shared__ uint32_t s_key[4][256];
  __shared__ int32_t s_codes[4];
  const int lane = threadIdx.x & 63, t = threadIdx.x >> 6;
  const bool live = t < p.n_tables;                        // (wave-uniform)
  uint32_t cnt[5];
  int32_t sym[5], root[5], len[5], rank[4];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    sym[j] = j < 4 ? lane + 64 * j : (lane == 0 ? 256 : -1);
    const uint32_t c = j < 4 ? (live ? counts[256 * t + lane + 64 * j] : 0u) : (lane == 0 ? 1u : 0u);
    cnt[j] = c == kNone ? 0u : c;
    root[j] = sym[j], len[j] = 0;
  }
#pragma unroll 1
  for (int step = 0; step < 256 && live; ++step) {
    uint32_t c_a = kNone, c_b = kNone;                     // this lane's best and second-best: in ascending symbols <= prefers the larger
    int32_t s_a = 0, s_b = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (cnt[j] && cnt[j] <= c_a) c_b = c_a, s_b = s_a, c_a = cnt[j], s_a = sym[j];
      else if (cnt[j] && cnt[j] <= c_b) c_b = cnt[j], s_b = sym[j];
    }
    const uint32_t v1 = wave_min_u32(c_a);
    const int32_t c1 = (int32_t)wave_max_u32(c_a == v1 ? (uint32_t)s_a : 0u);
    const bool owner = c_a == v1 && s_a == c1;
    const uint32_t c_o = owner ? c_b : c_a;
    const int32_t s_o = owner ? s_b : s_a;
    const uint32_t v2 = wave_min_u32(c_o);
    if (v1 == kNone || v2 == kNone) break;                  // one tree is left
    const int32_t c2 = (int32_t)wave_max_u32(c_o == v2 ? (uint32_t)s_o : 0u);
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      if (sym[j] == c1) cnt[j] += v2;
      if (sym[j] == c2) cnt[j] = 0u;
      if (root[j] == c1 || root[j] == c2) root[j] = c1, ++len[j];
    }
  }
  if (lane != 0) len[4] = 0;                                 // (the reserved symbol is lane 0's alone)

  // bits[] of the lengths, the reserved symbol's among them; the fold; every symbol's place in huffval; its code
  for (int i = lane; i <= kLenMax; i += 64) s_bits[t][i] = 0u;
  uint32_t longest = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) longest = max(longest, (uint32_t)len[j]);
  longest = wave_max_u32(longest);
  wave_sync();
  for (uint32_t l = 1; l <= longest; ++l) {                  // (wave-uniform)
    int n = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) n += __popcll(__ballot(len[j] == (int32_t)l));
    if (lane == 0) s_bits[t][l] = (uint32_t)n;
  }
  wave_sync();
  if (lane == 0) fold_bits(s_bits[t], (int)longest);
#pragma unroll
  for (int j = 0; j < 4; ++j) s_key[t][lane + 64 * j] = key_of(len[j], sym[j]);
  wave_sync();
  int n_codes = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) rank[j] = 0, n_codes += __popcll(__ballot(len[j] > 0));
#pragma unroll 4
  for (int o = 0; o < 256; ++o) {
    const uint32_t k = s_key[t][o];
#pragma unroll
    for (int j = 0; j < 4; ++j) rank[j] += k < key_of(len[j], sym[j]);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    uint16_t code = 0;
    uint8_t bits = 0;
    if (len[j] > 0) code_of_rank(s_bits[t], rank[j], &code, &bits);
    out->code[t][sym[j]] = code;
    out->len[t][sym[j]] = bits;
  }
  if (lane == 0) s_codes[t] = n_codes;
  __syncthreads();

  // div, the header around the new DHT segments, header_len
  const int tail_to = dht_at(p, s_codes, p.n_tables), tail_from = tail_of(p, in->header_len);
  const bool fits = tail_to + p.tail_len <= kHeaderMax;
  const int hl = fits ? tail_to + p.tail_len : 0;
  if (threadIdx.x < 192) out->div[threadIdx.x >> 6][threadIdx.x & 63] = in->div[threadIdx.x >> 6][threadIdx.x & 63];
  if (threadIdx.x == 0) out->header_len = hl, out->pad = 0;
  for (int i = threadIdx.x; i < kHeaderMax; i += kThreads) {
    if (fits && i < p.dht_at) out->header[i] = in->header[i];
    else if (fits && i >= tail_to && i < hl) out->header[i] = in->header[tail_from + i - tail_to];
    else if (i >= hl) out->header[i] = 0;
  }
  if (live && fits) {
    uint8_t* h = out->header + dht_at(p, s_codes, t);
    if (lane == 0) h[0] = 0xFF, h[1] = 0xC4, h[2] = (uint8_t)((19 + n_codes) >> 8), h[3] = (uint8_t)((19 + n_codes) & 255), h[4] = (uint8_t)((t & 1) << 4 | t >> 1);
    if (lane >= 1 && lane <= 16) h[4 + lane] = (uint8_t)s_bits[t][lane];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (len[j] > 0) h[21 + rank[j]] = (uint8_t)sym[j];
  }
}

// ---- launches ------------------------------------------------------------------------------------------------------------------------
static int histogram_launch(rhccq_ctx* ctx, const Frame& f, const int16_t* coef, uint32_t* counts) {
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const int64_t want = (f.g.blocks + 4 * kHistWaveBlocks - 1) / (4 * kHistWaveBlocks), most = (int64_t)kHistGroupsPerCu * ctx->compute_units;
  hipLaunchKernelGGL(clear_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, counts);
  hipLaunchKernelGGL(histogram_kernel, dim3((unsigned)(want < most ? want : most)), dim3(kThreads), 0, ctx->stream, f, coef, counts);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}
static int huffman_launch(rhccq_ctx* ctx, const Frame& f, const uint32_t* counts, const Tables* in, Tables* out) {
  hipLaunchKernelGGL(huffman_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, plan_of(f), counts, in, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// the optimising encode's workspace: the entropy stage's (sized for kBlockBitsOpt), the coefficients, the counts, the second struct
struct Layout { int64_t o_coef, o_counts, o_tables, total; };
static Layout layout_of(const Frame& f) {
  Layout l;
  l.o_coef = jpegw::entropy_workspace(f, kBlockBitsOpt);
  l.o_counts = l.o_coef + align256(128 * f.g.blocks);
  l.o_tables = l.o_counts + 4 * 256 * (int64_t)sizeof(uint32_t);
  l.total = l.o_tables + align256((int64_t)sizeof(Tables));
  return l;
}
// RHCCQ_OK, or what refuses the frame
static int frame_status(int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, bool file) {
  if (!args_ok(H, W, mode, quality, restart_rows)) return RHCCQ_E_ARG;
  const Frame f = frame_of(H, W, mode, restart_rows);
  if (!blocks_ok(f)) return RHCCQ_E_LIMIT;
  return file && jpegw::file_cap(f, kBlockBitsOpt) > jpegw::kFileMax ? RHCCQ_E_ARG : RHCCQ_OK;
}

}  // namespace jpego
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::jpego;

extern "C" {

int rhccq_jpeg_optimize_sizes(int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, int64_t* coefficients, int64_t* entropy_bytes, int64_t* encode_bytes,
                              int64_t* file_bytes) {
  if (!coefficients || !entropy_bytes || !encode_bytes || !file_bytes) return RHCCQ_E_ARG;
  if (const int rc = frame_status(H, W, mode, quality, restart_rows, true)) return rc;
  const Frame f = frame_of(H, W, mode, restart_rows);
  *coefficients = 64 * f.g.blocks;
  *entropy_bytes = jpegw::entropy_workspace(f, kBlockBitsOpt);
  *encode_bytes = layout_of(f).total;
  *file_bytes = jpegw::file_cap(f, kBlockBitsOpt);
  return RHCCQ_OK;
}

int rhccq_jpeg_histogram(rhccq_ctx* ctx, const int16_t* coef, int32_t H, int32_t W, int32_t mode, int32_t restart_rows, uint32_t* counts) {
  if (!ctx) return RHCCQ_E_ARG;
  const int rc = frame_status(H, W, mode, 1, restart_rows, false);
  if (rc == RHCCQ_E_LIMIT) return rhccq_fail(ctx, rc, "jpeg_histogram: 64 * blocks + 1 reaches 10^9, where libjpeg's search for the least count starts");
  if (rc || !coef || !counts || (uintptr_t)coef % 16 || (uintptr_t)counts % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_histogram: an unknown mode, H or W outside 1..65535, negative restart rows, or a null or misaligned pointer");
  return histogram_launch(ctx, frame_of(H, W, mode, restart_rows), coef, counts);
}

int rhccq_jpeg_huffman(rhccq_ctx* ctx, const uint32_t* counts, int32_t H, int32_t W, int32_t mode, int32_t restart_rows, const void* tables_dev, void* tables_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!args_ok(H, W, mode, 1, restart_rows) || !counts || !tables_dev || !tables_out || tables_dev == tables_out || (uintptr_t)counts % 4 || (uintptr_t)tables_dev % 4 ||
      (uintptr_t)tables_out % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_huffman: an unknown mode, H or W outside 1..65535, negative restart rows, a null or misaligned pointer, or one struct for both");
  return huffman_launch(ctx, frame_of(H, W, mode, restart_rows), counts, (const Tables*)tables_dev, (Tables*)tables_out);
}

int rhccq_jpeg_optimize(rhccq_ctx* ctx, const int16_t* coef, int32_t H, int32_t W, int32_t mode, int32_t restart_rows, const void* tables_dev, uint32_t* counts,
                        void* tables_out) {
  if (const int rc = rhccq_jpeg_histogram(ctx, coef, H, W, mode, restart_rows, counts)) return rc;
  return rhccq_jpeg_huffman(ctx, counts, H, W, mode, restart_rows, tables_dev, tables_out);
}

int rhccq_jpeg_entropy_optimized(rhccq_ctx* ctx, const int16_t* coef, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, const void* tables_dev,
                                 void* workspace, uint8_t* out, int64_t cap, int64_t* length) {
  if (!ctx) return RHCCQ_E_ARG;
  const int rc = frame_status(H, W, mode, quality, restart_rows, true);
  if (rc == RHCCQ_E_LIMIT) return rhccq_fail(ctx, rc, "jpeg_entropy_optimized: 64 * blocks + 1 reaches 10^9");
  if (rc) return rhccq_fail(ctx, rc, "jpeg_entropy_optimized: quality outside 1..100, an unknown mode, H or W outside 1..65535, negative restart rows, or too large a file");
  const Frame f = frame_of(H, W, mode, restart_rows);
  if (!coef || !tables_dev || !workspace || !out || !length || (uintptr_t)coef % 16 || (uintptr_t)tables_dev % 4 || (uintptr_t)workspace % 256 || (uintptr_t)length % 8 ||
      cap < jpegw::file_cap(f, kBlockBitsOpt))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_entropy_optimized: a null or misaligned pointer, or cap below rhccq_jpeg_optimize_sizes' file_bytes");
  return jpegw::entropy_launch(ctx, f, kBlockBitsOpt, (const Tables*)tables_dev, coef, workspace, out, cap, length);
}

int rhccq_jpeg_encode_optimize(rhccq_ctx* ctx, const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, int32_t optimize,
                               const void* tables_dev, void* workspace, uint8_t* out, int64_t cap, int64_t* length) {
  if (!optimize) return rhccq_jpeg_encode(ctx, image, H, W, mode, quality, restart_rows, tables_dev, workspace, out, cap, length);
  if (!ctx) return RHCCQ_E_ARG;
  const int rc = frame_status(H, W, mode, quality, restart_rows, true);
  if (rc == RHCCQ_E_LIMIT) return rhccq_fail(ctx, rc, "jpeg_encode_optimize: 64 * blocks + 1 reaches 10^9");
  if (rc) return rhccq_fail(ctx, rc, "jpeg_encode_optimize: quality outside 1..100, an unknown mode, H or W outside 1..65535, negative restart rows, or too large a file");
  if (!image || !tables_dev || !workspace || (uintptr_t)image % 16 || (uintptr_t)tables_dev % 4 || (uintptr_t)workspace % 256)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_encode_optimize: a null or misaligned image, table struct or workspace");
  const Frame f = frame_of(H, W, mode, restart_rows);
  const Layout l = layout_of(f);
  uint8_t* ws = (uint8_t*)workspace;
  int16_t* coef = (int16_t*)(ws + l.o_coef);
  uint32_t* counts = (uint32_t*)(ws + l.o_counts);
  Tables* made = (Tables*)(ws + l.o_tables);
  if (const int rc2 = jpegw::blocks_launch(ctx, f, (const Tables*)tables_dev, image, coef)) return rc2;
  if (const int rc2 = rhccq_jpeg_optimize(ctx, coef, H, W, mode, restart_rows, tables_dev, counts, made)) return rc2;
  return rhccq_jpeg_entropy_optimized(ctx, coef, H, W, mode, quality, restart_rows, made, workspace, out, cap, length);
}

int rhccq_jpeg_histogram_host(const int16_t* coef, int32_t H, int32_t W, int32_t mode, int32_t restart_rows, uint32_t* counts) {
  if (const int rc = frame_status(H, W, mode, 1, restart_rows, false)) return rc;
  if (!coef || !counts) return RHCCQ_E_ARG;
  histogram_serial(frame_of(H, W, mode, restart_rows), coef, (uint32_t(*)[256])counts);
  return RHCCQ_OK;
}

int rhccq_jpeg_huffman_host(const uint32_t* counts, int32_t H, int32_t W, int32_t mode, int32_t restart_rows, const void* tables, void* tables_out) {
  if (!args_ok(H, W, mode, 1, restart_rows) || !counts || !tables || !tables_out || tables == tables_out) return RHCCQ_E_ARG;
  for (int t = 0; t < 4; ++t) {                            // (a table's counts with the reserved 1: below where libjpeg's search starts)
    int64_t of_table = 1;
    for (int i = 0; i < 256; ++i) of_table += counts[256 * t + i];
    if (of_table >= kCountMax) return RHCCQ_E_LIMIT;
  }
  huffman_serial(frame_of(H, W, mode, restart_rows), (const uint32_t(*)[256])counts, *(const Tables*)tables, (Tables*)tables_out);
  return RHCCQ_OK;
}

int rhccq_jpeg_encode_optimize_host(const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, int32_t optimize, uint8_t* out,
                                    int64_t cap, int64_t* length) {
  if (!optimize) return rhccq_jpeg_encode_host(image, H, W, mode, quality, restart_rows, out, cap, length);
  if (const int rc = frame_status(H, W, mode, quality, restart_rows, true)) return rc;
  if (!image || !out || !length || cap < 0) return RHCCQ_E_ARG;
  const Frame f = frame_of(H, W, mode, restart_rows);
  std::vector<Tables> T(2);
  jpegw::tables_build(f, quality, &T[0]);
  std::vector<int16_t> coef((size_t)(64 * f.g.blocks));
  jpegw::blocks_serial(f, T[0], image, coef.data());
  std::vector<uint32_t> counts(4 * 256);
  histogram_serial(f, coef.data(), (uint32_t(*)[256])counts.data());
  huffman_serial(f, (const uint32_t(*)[256])counts.data(), T[0], &T[1]);
  *length = jpegw::encode_serial(f, T[1], coef.data(), out, cap);
  return *length < 0 ? RHCCQ_E_ARG : RHCCQ_OK;
}

}  // extern "C"
