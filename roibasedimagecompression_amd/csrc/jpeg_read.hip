// JPEG files read on the device (EXTENSION, include/rhccq.h): the unstuffing, the self-synchronising Huffman decode, the DC sums, the IDCT
// and the upsampling with the colour conversion.  The definitions both sides share are in jpeg_read.h; the host forms at the end run
// them serially.
//
//   head_kernel        the workspace's eight words.
//   unstuff_kernel<false / true>  a lane 16 bytes of the scan, a workgroup a tile of kTileBytes: which bytes stay (kept), their number a
//                      tile; then, behind scan_kernel's prefix sum over the tiles, the same test again and the scatter.
//   sync_kernel        a lane a subsequence, 256 of them a workgroup, the Huffman tables in LDS.  Every lane decodes from its guess, then
//                      takes the state its left neighbour left in (over LDS) and decodes again while its entry changes; the workgroup's
//                      first lane keeps its guess (the stream's first one the truth).  Ends when no entry changed: at most 256 rounds.
//   boundary_kernel    one workgroup, a lane a boundary between two workgroups of sync_kernel, 256 boundaries at a time in order: from
//                      the state the workgroup on the left ends in, the lane re-decodes the subsequences of the one on the right until an
//                      entry it meets is the recorded one.  Only a walk that reaches the workgroup's last subsequence changes what the
//                      next boundary starts from, so the rounds go on until none did.  A lane writes only its own workgroup's rows.
//   place_kernel       one workgroup: the subsequences' counts -> the block each starts in.  A count taken behind an interval's start is
//                      a block number and restarts the sum (seg_block_scan).
//   write_kernel       sync_kernel's decode once more from the true entries, writing.
//   dc_kernel<false / true>, dc_carry_kernel  the DC differences of a component in decode order, 256 a tile: the tiles' sums (restarted
//                      at an interval's first block), their exclusive prefix, then the tiles again with their carries.
//   idct_kernel        eight lanes a block, 32 blocks a workgroup: a lane a column (dequantised from LDS), the 8 x 8 intermediate through
//                      LDS (rows of 9 words), a lane a row, 8 bytes a store.  (The rounding between the two passes is part of libjpeg's
//                      definition, so the transform is no matrix product an MFMA could take: DESIGN.md.)
//   colour_kernel      a lane four pixels of the flat image: 12 bytes, three aligned words.
//   finish_kernel      the lowest bad interval -> status[2].
#include "jpeg_read.h"
#include "rhccq_common.h"

#include <vector>

namespace rhccq {
namespace jpegr {

__global__ void head_kernel(uint32_t* __restrict__ head, uint32_t n_sub) {
  if (threadIdx.x < 8) head[threadIdx.x] = threadIdx.x == 0 ? kNoInterval : threadIdx.x == 1 ? n_sub : 0u;
}
__global__ void finish_kernel(const uint32_t* __restrict__ head, int32_t* __restrict__ status) {
  status[0] = head[0] == kNoInterval ? RHCCQ_JPEG_OK : RHCCQ_JPEG_BAD_SCAN;
  status[1] = head[0] == kNoInterval ? 0 : (int32_t)head[0];
}
__global__ void set_status_kernel(int32_t a, int32_t b, int32_t* __restrict__ status) {
  status[0] = a;
  status[1] = b;
}

// ---- unstuff -------------------------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void unstuff_kernel(const uint8_t* __restrict__ file, long long n, long long lo, long long len,
                                                           uint32_t* __restrict__ tiles, uint8_t* __restrict__ stream, long long stream_bytes) {
  __shared__ uint32_t s_red[kThreads / 64 + 1];
  const long long p0 = lo + ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
  uint32_t mask = 0;
#pragma unroll
  for (int j = 0; j < 16; ++j)
    if (p0 + j < lo + len && kept(file, n, lo, p0 + j)) mask |= 1u << j;
  uint32_t total;
  const uint32_t excl = block_exscan<uint32_t>(__popc(mask), s_red, &total);
  if (!SCATTER) {
    if (threadIdx.x == 0) tiles[blockIdx.x] = total;
    return;
  }
  long long at = (long long)tiles[blockIdx.x] + excl;
  for (int j = 0; j < 16; ++j)
    if (mask >> j & 1u) {
      if (at < stream_bytes) stream[at] = file[p0 + j];
      ++at;
    }
  if (blockIdx.x == 0 && threadIdx.x < kStreamPad) stream[stream_bytes + threadIdx.x] = 0;
}
// exclusive prefix sums of count words in place, one workgroup
__global__ __launch_bounds__(kThreads) void scan_kernel(uint32_t* __restrict__ v, long long count) {
  __shared__ uint32_t s_red[kThreads / 64 + 1];
  uint32_t run = 0;
  for (long long i0 = 0; i0 < count; i0 += kThreads) {    // (uniform)
    const long long i = i0 + threadIdx.x;
    uint32_t total;
    const uint32_t x = i < count ? v[i] : 0u, excl = block_exscan<uint32_t>(x, s_red, &total);
    if (i < count) v[i] = run + excl;
    run += total;
  }
}

// ---- sync ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sync_kernel(Dec d, const rhccq_jpeg_tables* __restrict__ tables, int S, long long n_sub, SubRow* __restrict__ rows,
                                                        uint32_t* __restrict__ head) {
  __shared__ rhccq_jpeg_tables s_T;
  __shared__ uint64_t s_leave[kThreads];
  tables_to_lds(&s_T, tables);
  d.T = &s_T;
  const int tid = threadIdx.x;
  const long long g = (long long)blockIdx.x * kThreads + tid;
  const bool live = g < n_sub;
  const long long end = sub_end(d, S, g);
  uint64_t entry = pack(g * S, 0, 0), leave = 0;
  uint32_t count = 0;
  if (live) run<false>(d, entry, g == 0, end, 0, nullptr, nullptr, &leave, &count);
  uint32_t rounds = 0;
  for (int r = 0; r < kThreads; ++r) {                               // (uniform: the vote decides)
    s_leave[tid] = leave;
    __syncthreads();
    const uint64_t want = live && tid > 0 ? s_leave[tid - 1] : entry;
    const bool changed = want != entry;
    if (!__syncthreads_or(changed)) break;
    if (changed) {
      entry = want;
      run<false>(d, entry, false, end, 0, nullptr, nullptr, &leave, &count);
    }
    ++rounds;
  }
  if (live) rows[g] = SubRow{entry, leave, count, 0u};
  if (tid == 0) atomicMax(&head[2], rounds);
}

__global__ __launch_bounds__(kThreads) void boundary_kernel(Dec d, const rhccq_jpeg_tables* __restrict__ tables, int S, long long n_sub, SubRow* __restrict__ rows,
                                                            uint32_t* __restrict__ head) {
  __shared__ rhccq_jpeg_tables s_T;
  __shared__ uint64_t s_tail[kThreads];
  tables_to_lds(&s_T, tables);
  d.T = &s_T;
  const int tid = threadIdx.x;
  const long long n_wg = (n_sub + kThreads - 1) / kThreads;
  uint64_t carry = rows[kThreads - 1].leave;                         // (n_wg > 1: the row is there)
  uint32_t rounds = 0, walk = 0;
  for (long long c0 = 1; c0 < n_wg; c0 += kThreads) {               // (uniform)
    const long long w = c0 + tid, g_lo = w * kThreads, g_hi = g_lo + kThreads < n_sub ? g_lo + kThreads : n_sub;
    const bool live = w < n_wg;
    uint64_t tail = live ? rows[g_hi - 1].leave : 0;
    s_tail[tid] = tail;
    for (int r = 0; r <= kThreads; ++r) {                            // (uniform)
      __syncthreads();
      uint64_t want = tid == 0 ? carry : s_tail[tid - 1];
      bool moved = false;
      if (live) {
        long long g = g_lo;
        uint32_t steps = 0;
        while (g < g_hi && rows[g].entry != want) {
          uint64_t leave;
          uint32_t count;
          run<false>(d, want, false, sub_end(d, S, g), 0, nullptr, nullptr, &leave, &count);
          rows[g] = SubRow{want, leave, count, 0u};
          want = leave;
          ++g;
          ++steps;
        }
        walk = steps > walk ? steps : walk;
        moved = steps > 0 && g == g_hi && want != tail;
      }
      const int any = __syncthreads_or(moved);                       // (every lane has read its neighbour's tail)
      if (moved) s_tail[tid] = tail = want;
      if (!any) break;
      ++rounds;
    }
    __syncthreads();
    carry = s_tail[kThreads - 1];
    __syncthreads();
  }
  atomicMax(&head[4], walk);
  if (tid == 0) head[3] = rounds;
}

__global__ __launch_bounds__(kThreads) void place_kernel(const SubRow* __restrict__ rows, long long n_sub, uint32_t* __restrict__ first) {
  __shared__ uint64_t s_w[kThreads / 64];
  uint64_t run = 1ull << 32;                                         // block 0, absolute
  if (threadIdx.x == 0) first[0] = 0u;
  for (long long g0 = 0; g0 < n_sub; g0 += kThreads) {              // (uniform)
    const long long g = g0 + threadIdx.x;
    const uint32_t c = g < n_sub ? rows[g].count : 0u;
    uint64_t total;
    const uint64_t incl = seg_block_scan((uint64_t)(c >> 31) << 32 | (c & ~kAbs), s_w, &total);
    if (g < n_sub) first[g + 1] = (uint32_t)seg_combine(run, incl);
    run = seg_combine(run, total);
  }
}

__global__ __launch_bounds__(kThreads) void write_kernel(Dec d, const rhccq_jpeg_tables* __restrict__ tables, int S, long long n_sub, const SubRow* __restrict__ rows,
                                                         const uint32_t* __restrict__ first, int16_t* __restrict__ coef, uint32_t* __restrict__ head) {
  __shared__ rhccq_jpeg_tables s_T;
  tables_to_lds(&s_T, tables);
  d.T = &s_T;
  const long long g = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (g >= n_sub) return;
  uint64_t leave;
  uint32_t count;
  run<true>(d, rows[g].entry, g == 0, sub_end(d, S, g), (long long)first[g], coef, &head[0], &leave, &count);
}

// ---- dc ------------------------------------------------------------------------------------------------------------------------------
template <bool FINAL>
__global__ __launch_bounds__(kThreads) void dc_kernel(Geo g, int16_t* __restrict__ coef, uint64_t* __restrict__ agg) {
  __shared__ uint64_t s_w[kThreads / 64];
  int c = 0;
  long long t = blockIdx.x;
  DcSeq s = dc_seq(g, 0);
  while (c + 1 < g.n_comp && t >= s.tiles) {                         // (uniform)
    t -= s.tiles;
    s = dc_seq(g, ++c);
  }
  const long long q = t * kThreads + threadIdx.x;
  const bool live = q < s.len;
  const long long mcu = q / s.nb;
  const int j = (int)(q - mcu * s.nb);
  int16_t* at = coef + 64 * block_at(g, live ? mcu * g.bpm + s.b0 + j : 0);
  const bool starts = live && j == 0 && (g.R ? mcu % g.R == 0 : mcu == 0);
  const uint32_t v = live ? (uint32_t)(int32_t)*at : 0u;
  uint64_t total;
  const uint64_t incl = seg_block_scan((uint64_t)starts << 32 | v, s_w, &total);
  if (!FINAL) {
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
    return;
  }
  if (live) *at = (int16_t)(uint32_t)seg_combine(agg[blockIdx.x], incl);
}
// the tiles' sums -> what every tile starts from (flagged words: seg_combine takes them as they are), a component after the other
__global__ __launch_bounds__(kThreads) void dc_carry_kernel(Geo g, uint64_t* __restrict__ agg) {
  __shared__ uint64_t s_w[kThreads / 64];
  __shared__ uint64_t s_x[kThreads];
  long long base = 0;
  for (int c = 0; c < g.n_comp; ++c) {                               // (uniform)
    const DcSeq s = dc_seq(g, c);
    uint64_t run = 0;
    for (long long t0 = 0; t0 < s.tiles; t0 += kThreads) {          // (uniform)
      const long long t = t0 + threadIdx.x;
      uint64_t total;
      const uint64_t incl = seg_block_scan(t < s.tiles ? agg[base + t] : 0ull, s_w, &total);
      s_x[threadIdx.x] = incl;
      __syncthreads();
      if (t < s.tiles) agg[base + t] = seg_combine(run, threadIdx.x ? s_x[threadIdx.x - 1] : 0ull) & 0xFFFFFFFFull;
      run = seg_combine(run, total);
      __syncthreads();
    }
    base += s.tiles;
  }
}

// ---- idct, colour --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void idct_kernel(Geo g, const rhccq_jpeg_tables* __restrict__ tables, const int16_t* __restrict__ coef,
                                                        uint8_t* __restrict__ planes) {
  __shared__ uint16_t s_q[3][64];
  __shared__ int32_t s_ws[kIdctBlocks][8][9];
  if (threadIdx.x < 192) s_q[threadIdx.x >> 6][threadIdx.x & 63] = tables->quant[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const int slot = threadIdx.x >> 3, l = threadIdx.x & 7;
  const long long B = (long long)blockIdx.x * kIdctBlocks + slot;
  const bool live = B < g.blocks;
  const int c = g.n_comp == 3 && B >= g.base[2] ? 2 : g.n_comp == 3 && B >= g.base[1] ? 1 : 0;
  if (live) {
    int32_t y[8];
    idct_column(coef + 64 * B, s_q[c], l, y);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_ws[slot][r][l] = y[r];
  }
  __syncthreads();
  if (!live) return;
  int32_t x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = s_ws[slot][l][k];
  union { uint8_t b[8]; uint2 w; } out;
  idct_row(x, out.b);
  const long long blk = B - g.base[c], by = blk / g.bw[c], bx = blk - by * g.bw[c];
  *(uint2*)(planes + 64 * g.base[c] + (8 * by + l) * (8 * (long long)g.bw[c]) + 8 * bx) = out.w;
}

__global__ __launch_bounds__(kThreads) void colour_kernel(Geo g, const uint8_t* __restrict__ planes, uint8_t* __restrict__ rgb) {
  const long long p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4, hw = (long long)g.H * g.W;
  if (p0 >= hw) return;
  union { uint8_t b[12]; uint32_t w[3]; } out;
  const int n = hw - p0 < 4 ? (int)(hw - p0) : 4;
  for (int k = 0; k < n; ++k) {
    int y, x;
    rhccq_row_col(p0 + k, g.W, y, x);
    rgb_at(g, planes, y, x, out.b + 3 * k);
  }
  if (n == 4) {
    uint32_t* dst = (uint32_t*)(rgb + 3 * p0);
    dst[0] = out.w[0], dst[1] = out.w[1], dst[2] = out.w[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) rgb[3 * p0 + k] = out.b[k];
  }
}

// ---- layouts and launches ------------------------------------------------------------------------------------------------------------
// rhccq_jpeg_coefficients' workspace: the head, the unstuff tiles, the stream, the subsequences' rows and first blocks, the DC tiles
struct CoefLayout { int64_t n_tiles, n_sub, o_tiles, o_stream, o_rows, o_first, o_agg, total; };
static CoefLayout coef_layout(const rhccq_jpeg_info& f, int S) {
  CoefLayout l;
  l.n_tiles = f.scan_bytes > 0 ? (f.scan_bytes + kTileBytes - 1) / kTileBytes : 1;
  l.n_sub = sub_count(f.stream_bytes, S);
  l.o_tiles = 256;
  l.o_stream = align256(l.o_tiles + 4 * l.n_tiles);
  l.o_rows = align256(l.o_stream + f.stream_bytes + kStreamPad);
  l.o_first = align256(l.o_rows + (int64_t)sizeof(SubRow) * l.n_sub);
  l.o_agg = align256(l.o_first + 4 * (l.n_sub + 1));
  l.total = align256(l.o_agg + 8 * dc_tiles(geo_of(f)));
  return l;
}
static int64_t planes_bytes(const rhccq_jpeg_info& f) { return align256(64 * f.blocks); }

static int coefficients_launch(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_jpeg_info& f, const rhccq_jpeg_tables* tables_dev,
                               const rhccq_segment* intervals_dev, int S, void* workspace, int16_t* coef, int32_t* status) {
  const CoefLayout l = coef_layout(f, S);
  uint8_t* ws = (uint8_t*)workspace;
  uint32_t* head = (uint32_t*)ws;
  uint32_t* tiles = (uint32_t*)(ws + l.o_tiles);
  uint8_t* stream = ws + l.o_stream;
  SubRow* rows = (SubRow*)(ws + l.o_rows);
  uint32_t* first = (uint32_t*)(ws + l.o_first);
  uint64_t* agg = (uint64_t*)(ws + l.o_agg);
  Dec d;
  d.words = (const uint32_t*)stream;
  d.T = nullptr;
  d.iv = intervals_dev;
  d.n_iv = f.n_intervals;
  d.total_bits = 8 * f.stream_bytes;
  d.g = geo_of(f);
  const hipStream_t st = ctx->stream;
  const dim3 wg(kThreads), one(1), per_tile((unsigned)(l.n_tiles < 1 ? 1 : l.n_tiles)), per_sub((unsigned)((l.n_sub + kThreads - 1) / kThreads));
  hipLaunchKernelGGL(head_kernel, one, dim3(64), 0, st, head, (uint32_t)(l.n_sub > 0xFFFFFFFFll ? 0xFFFFFFFFll : l.n_sub));
  RHCCQ_HIP(ctx, hipMemsetAsync(coef, 0, (size_t)(128 * f.blocks), st));
  hipLaunchKernelGGL(unstuff_kernel<false>, per_tile, wg, 0, st, file, (long long)n, (long long)f.scan_offset, (long long)f.scan_bytes, tiles, stream,
                     (long long)f.stream_bytes);
  hipLaunchKernelGGL(scan_kernel, one, wg, 0, st, tiles, (long long)l.n_tiles);
  hipLaunchKernelGGL(unstuff_kernel<true>, per_tile, wg, 0, st, file, (long long)n, (long long)f.scan_offset, (long long)f.scan_bytes, tiles, stream,
                     (long long)f.stream_bytes);
  hipLaunchKernelGGL(sync_kernel, per_sub, wg, 0, st, d, tables_dev, S, (long long)l.n_sub, rows, head);
  if (l.n_sub > kThreads) hipLaunchKernelGGL(boundary_kernel, one, wg, 0, st, d, tables_dev, S, (long long)l.n_sub, rows, head);
  hipLaunchKernelGGL(place_kernel, one, wg, 0, st, (const SubRow*)rows, (long long)l.n_sub, first);
  hipLaunchKernelGGL(write_kernel, per_sub, wg, 0, st, d, tables_dev, S, (long long)l.n_sub, (const SubRow*)rows, (const uint32_t*)first, coef, head);
  const dim3 per_dc((unsigned)dc_tiles(d.g));
  hipLaunchKernelGGL(dc_kernel<false>, per_dc, wg, 0, st, d.g, coef, agg);
  hipLaunchKernelGGL(dc_carry_kernel, one, wg, 0, st, d.g, agg);
  hipLaunchKernelGGL(dc_kernel<true>, per_dc, wg, 0, st, d.g, coef, agg);
  hipLaunchKernelGGL(finish_kernel, one, one, 0, st, (const uint32_t*)head, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static int pixels_launch(rhccq_ctx* ctx, const rhccq_jpeg_info& f, const rhccq_jpeg_tables* tables_dev, const int16_t* coef, uint8_t* planes, uint8_t* rgb) {
  const Geo g = geo_of(f);
  const int64_t hw = (int64_t)g.H * g.W;
  hipLaunchKernelGGL(idct_kernel, dim3((unsigned)((g.blocks + kIdctBlocks - 1) / kIdctBlocks)), dim3(kThreads), 0, ctx->stream, g, tables_dev, coef, planes);
  hipLaunchKernelGGL(colour_kernel, dim3((unsigned)((hw + 4 * kThreads - 1) / (4 * kThreads))), dim3(kThreads), 0, ctx->stream, g, (const uint8_t*)planes, rgb);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static int sub_bits(int32_t s) { return s ? s : kSubBits; }

// the host forms' decode: the parse, the unstuffed stream, one run of the decoder over all of it, the DC sums
static int coefficients_host(const uint8_t* file, int64_t n, rhccq_jpeg_info* f, rhccq_jpeg_tables* T, int16_t* coef, int32_t* status) {
  jpeg_parse(file, n, f, T, nullptr, 0);
  status[0] = f->status;
  status[1] = f->detail;
  if (f->status != RHCCQ_JPEG_OK) return RHCCQ_OK;
  if (!coef) return RHCCQ_E_ARG;
  std::vector<rhccq_segment> iv((size_t)f->n_intervals);
  jpeg_parse(file, n, f, T, iv.data(), (int64_t)iv.size());
  std::vector<uint32_t> words((size_t)((f->stream_bytes + kStreamPad) / 4 + 2), 0u);
  unstuff_serial(file, n, *f, (uint8_t*)words.data());
  Dec d;
  d.words = words.data();
  d.T = T;
  d.iv = iv.data();
  d.n_iv = f->n_intervals;
  d.total_bits = 8 * f->stream_bytes;
  d.g = geo_of(*f);
  memset(coef, 0, (size_t)(128 * f->blocks));
  uint32_t bad = kNoInterval, count;
  uint64_t leave;
  run<true>(d, pack(0, 0, 0), true, d.total_bits, 0, coef, &bad, &leave, &count);
  dc_serial(d.g, coef);
  if (bad != kNoInterval) {
    status[0] = RHCCQ_JPEG_BAD_SCAN;
    status[1] = (int32_t)bad;
  }
  return RHCCQ_OK;
}

}  // namespace jpegr
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::jpegr;

extern "C" {

int rhccq_jpeg_parse_host(const uint8_t* file, int64_t n, rhccq_jpeg_info* info, rhccq_jpeg_tables* tables, rhccq_segment* intervals, int64_t cap,
                          int64_t* n_intervals) {
  if (n < 0 || (n > 0 && !file) || !info || !tables || !n_intervals || cap < 0 || (cap > 0 && !intervals)) return RHCCQ_E_ARG;
  jpeg_parse(file, n, info, tables, intervals, cap);
  *n_intervals = info->n_intervals;
  return RHCCQ_OK;
}

int32_t rhccq_jpeg_subsequence_bits(void) { return kSubBits; }
int32_t rhccq_jpeg_tables_bytes(void) { return (int32_t)sizeof(rhccq_jpeg_tables); }

int rhccq_jpeg_read_sizes(const rhccq_jpeg_info* info, int64_t n, int32_t subsequence_bits, int64_t* decode_bytes, int64_t* coefficients_bytes,
                          int64_t* pixels_bytes) {
  if (!info || !decode_bytes || !coefficients_bytes || !pixels_bytes || n < 0 || !sub_bits_ok(subsequence_bits)) return RHCCQ_E_ARG;
  if (info->status != RHCCQ_JPEG_OK) {
    *decode_bytes = *coefficients_bytes = *pixels_bytes = 256;
    return RHCCQ_OK;
  }
  if (!info_sound(*info, n)) return RHCCQ_E_ARG;
  *coefficients_bytes = coef_layout(*info, sub_bits(subsequence_bits)).total;
  *pixels_bytes = planes_bytes(*info);
  *decode_bytes = *coefficients_bytes + align256(128 * info->blocks) + *pixels_bytes;
  return RHCCQ_OK;
}

int rhccq_jpeg_coefficients(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_jpeg_info* info, const rhccq_jpeg_tables* tables_dev,
                            const rhccq_segment* intervals_dev, int32_t subsequence_bits, void* workspace, int16_t* coef, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!info || !status || (uintptr_t)status % 4) return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_coefficients: a null info or status");
  if (info->status != RHCCQ_JPEG_OK) {                               // decided on the host: no device work but the status itself
    hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(1), 0, ctx->stream, info->status, info->detail, status);
    RHCCQ_LAUNCH_CHECK(ctx);
    return RHCCQ_OK;
  }
  if (!file || !tables_dev || !intervals_dev || !workspace || !coef || (uintptr_t)tables_dev % 4 || (uintptr_t)intervals_dev % 8 || (uintptr_t)workspace % 256 ||
      (uintptr_t)coef % 4 || !sub_bits_ok(subsequence_bits))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_coefficients: a null or misaligned pointer, or subsequence_bits not 0 or a multiple of 32 in 128..65536");
  if (!info_sound(*info, n)) return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_coefficients: info does not describe a file of n bytes (it is rhccq_jpeg_parse_host's)");
  return coefficients_launch(ctx, file, n, *info, tables_dev, intervals_dev, sub_bits(subsequence_bits), workspace, coef, status);
}

int rhccq_jpeg_pixels(rhccq_ctx* ctx, const rhccq_jpeg_info* info, const rhccq_jpeg_tables* tables_dev, const int16_t* coef, void* workspace, uint8_t* rgb) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!info || !tables_dev || !coef || !workspace || !rgb || (uintptr_t)tables_dev % 4 || (uintptr_t)coef % 4 || (uintptr_t)workspace % 256 || (uintptr_t)rgb % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_pixels: a null or misaligned pointer");
  if (info->status != RHCCQ_JPEG_OK || !info_sound(*info, info->scan_offset + info->scan_bytes))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_pixels: info is not that of a file rhccq_jpeg_parse_host accepts");
  return pixels_launch(ctx, *info, tables_dev, coef, (uint8_t*)workspace, rgb);
}

int rhccq_jpeg_decode(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_jpeg_info* info, const rhccq_jpeg_tables* tables_dev,
                      const rhccq_segment* intervals_dev, int32_t subsequence_bits, void* workspace, uint8_t* rgb, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (info && info->status == RHCCQ_JPEG_OK && (!rgb || (uintptr_t)rgb % 4 || !workspace || !sub_bits_ok(subsequence_bits) || !info_sound(*info, n)))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_decode: a null or misaligned rgb or workspace, a bad subsequence_bits, or an info that is not the parse's");
  uint8_t* ws = (uint8_t*)workspace;
  const int64_t o_coef = info && info->status == RHCCQ_JPEG_OK ? coef_layout(*info, sub_bits(subsequence_bits)).total : 0;
  if (const int rc = rhccq_jpeg_coefficients(ctx, file, n, info, tables_dev, intervals_dev, subsequence_bits, workspace, (int16_t*)(ws + o_coef), status)) return rc;
  if (info->status != RHCCQ_JPEG_OK) return RHCCQ_OK;
  return pixels_launch(ctx, *info, tables_dev, (const int16_t*)(ws + o_coef), ws + o_coef + align256(128 * info->blocks), rgb);
}

int rhccq_jpeg_coefficients_host(const uint8_t* file, int64_t n, int16_t* coef, int32_t* status) {
  if (n < 0 || (n > 0 && !file) || !status) return RHCCQ_E_ARG;
  rhccq_jpeg_info f;
  rhccq_jpeg_tables T;
  return coefficients_host(file, n, &f, &T, coef, status);
}

int rhccq_jpeg_pixels_host(const rhccq_jpeg_info* info, const rhccq_jpeg_tables* tables, const int16_t* coef, uint8_t* rgb) {
  if (!info || !tables || !coef || !rgb || info->status != RHCCQ_JPEG_OK || !info_sound(*info, info->scan_offset + info->scan_bytes)) return RHCCQ_E_ARG;
  const Geo g = geo_of(*info);
  std::vector<uint8_t> planes((size_t)(64 * g.blocks));
  planes_serial(g, *tables, coef, planes.data());
  rgb_serial(g, planes.data(), rgb);
  return RHCCQ_OK;
}

int rhccq_jpeg_decode_host(const uint8_t* file, int64_t n, uint8_t* rgb, int32_t* status) {
  if (n < 0 || (n > 0 && !file) || !status) return RHCCQ_E_ARG;
  rhccq_jpeg_info f;
  rhccq_jpeg_tables T;
  jpeg_parse(file, n, &f, &T, nullptr, 0);
  std::vector<int16_t> coef(f.status == RHCCQ_JPEG_OK ? (size_t)(64 * f.blocks) : 1);
  if (const int rc = coefficients_host(file, n, &f, &T, coef.data(), status)) return rc;
  if (f.status != RHCCQ_JPEG_OK) return RHCCQ_OK;
  if (!rgb) return RHCCQ_E_ARG;
  return rhccq_jpeg_pixels_host(&f, &T, coef.data(), rgb);
}

}  // extern "C"
