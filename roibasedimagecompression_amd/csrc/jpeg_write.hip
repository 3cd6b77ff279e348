// JPEG files written on the device (EXTENSION, include/rhccq.h): colour conversion, downsampling, the islow FDCT and the quantiser; then the
// Huffman coding of every block by one wave, a restarting prefix sum for the blocks' places, the packing through LDS, and the byte
// stuffing.  The definitions both sides share are in jpeg_write.h; the host forms at the end run them serially.
//
//   blocks_kernel      a workgroup a strip of MCUs of one MCU row (at most 32 blocks).  The strip's rows arrive as aligned 16-byte loads in
//                      LDS (a row's ragged ends included, the image's last row standing in for rows below it); eight lanes take a block:
//                      a lane converts and averages the eight samples of its row from LDS and runs the row pass, the 8 x 8 intermediate
//                      goes through LDS (rows of 9 words), the lane runs a column and divides by the divisors in LDS; dummy blocks take
//                      their DC from their source block's slot; 16 bytes a store.  (The rounding between the two passes is part of
//                      libjpeg's definition, so the transform is no matrix product an MFMA could take, as with the reader's IDCT.)
//   count_kernel       a wave a block, a lane a zig-zag position (lane_symbol); 8 blocks a wave, 32 a workgroup, in scan order -> bits a
//                      block.
//   place_kernel<false / true>, place_carry_kernel  the blocks' bits in scan order, 256 a tile: the tiles' sums (restarted at an
//                      interval's first block), their exclusive prefix, then the tiles again -> every block's first bit in its interval
//                      and every interval's bytes.
//   scan_kernel        one workgroup: the intervals' bytes -> their first bytes in the unstuffed stream, and its length.
//   zero_kernel        the stream's words up to that length.
//   pack_kernel        count_kernel's pass again: a DPP scan of the lanes' lengths places every lane's bits, LDS atomics OR them into
//                      the workgroup's window, whole words go out big-endian; the first and the last by a global atomic OR.
//   ff_kernel          a lane 16 bytes of the stream, a workgroup a tile of kTileBytes: the 0xFF bytes a tile.
//   scan_kernel        again: the tiles' exclusive prefix, the total.
//   stuff_kernel       the same lanes again: every byte to its place behind the header, a zero behind an 0xFF, RSTm in front of an
//                      interval's first byte; the first lane copies nothing but writes EOI and the file's length; the header's bytes by
//                      the first workgroup.
#include "jpeg_write.h"
#include "rhccq_common.h"
#include "wave_dpp.h"

#include <vector>

namespace rhccq {
namespace jpegw {

constexpr uint64_t kFlag = (uint64_t)1 << 63;
// head words (uint64): the unstuffed stream's bytes, its 0xFF bytes, the file's length
enum { kHeadStream = 0, kHeadFF = 1, kHeadLength = 2 };

// ---- blocks --------------------------------------------------------------------------------------------------------------------------
struct LdsPx {
  const uint8_t* rows;                                     // the staged rows, kRowBytes each
  long long W;
  int C, y0, x0;
  __device__ __forceinline__ int32_t operator()(int y, int x, int ch) const {
    const int off = (int)(((y * W + x0) * C) & 15);
    return rows[(y - y0) * kRowBytes + off + (x - x0) * C + ch];
  }
};

__global__ __launch_bounds__(kThreads) void blocks_kernel(Frame f, const Tables* __restrict__ tables, const uint8_t* __restrict__ img, int strip,
                                                          int16_t* __restrict__ coef) {
  __shared__ __attribute__((aligned(16))) uint8_t s_rows[16 * kRowBytes];
  __shared__ uint16_t s_div[3][64];
  __shared__ int32_t s_ws[kPackBlocks][8][9];
  __shared__ __attribute__((aligned(16))) int16_t s_out[kPackBlocks][64];
  const Geo& g = f.g;
  const int tid = threadIdx.x, C = g.n_comp, mw = 8 * g.hs, mh = 8 * g.vs;
  const int my = blockIdx.y, mx0 = blockIdx.x * strip, n_m = min(strip, g.mcus_x - mx0);
  const int x0 = mx0 * mw, xe = min(x0 + n_m * mw, g.W), y0 = my * mh;
  const long long total = (long long)g.H * g.W * C;
  if (tid < 192) s_div[tid >> 6][tid & 63] = tables->div[tid >> 6][tid & 63];
  constexpr int kChunks = kRowBytes / 16;
  for (int i = tid; i < mh * kChunks; i += kThreads) {     // (uniform bound)
    const int r = i / kChunks, c = i - r * kChunks, y = min(y0 + r, g.H - 1);
    const long long b0 = ((long long)y * g.W + x0) * C, b1 = ((long long)y * g.W + xe) * C, a = (b0 & ~15ll) + 16 * c;
    if (a >= b1) continue;
    uint8_t* dst = s_rows + r * kRowBytes + 16 * c;
    if (a + 16 <= total) {
      *(uint4*)dst = *(const uint4*)(img + a);
    } else {
      for (int k = 0; k < 16; ++k) dst[k] = a + k < total ? img[a + k] : 0;
    }
  }
  __syncthreads();
  const int slot = tid >> 3, l = tid & 7;
  const bool live = slot < n_m * g.bpm;
  const int m = slot / g.bpm, b = slot - m * g.bpm, c = comp_of(g, b), mx = mx0 + m;
  const int yi = c ? 0 : b / g.hs, xi = c ? 0 : b - yi * g.hs;
  const int by = c ? my : my * g.vs + yi, bx = c ? mx : mx * g.hs + xi;
  int sy = 0, sx = 0;
  const bool dummy = live && c == 0 && dummy_source(f, by, bx, &sy, &sx);
  if (live && !dummy) {
    const LdsPx px{s_rows, g.W, C, y0, x0};
    int32_t d[8], o[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = sample_at(px, g, c, 8 * by + l, 8 * bx + k) - 128;
    fdct8(d, true, o);
#pragma unroll
    for (int k = 0; k < 8; ++k) s_ws[slot][l][k] = o[k];
  }
  __syncthreads();
  if (live) {
    int32_t d[8], o[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) d[r] = dummy ? 0 : s_ws[slot][r][l];
    fdct8(d, false, o);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_out[slot][8 * r + l] = dummy ? (int16_t)0 : quantise(o[r], s_div[c][8 * r + l]);
  }
  __syncthreads();
  int16_t dc = 0;
  if (dummy && l == 0) dc = s_out[m * g.bpm + (sy - my * g.vs) * g.hs + (sx - mx * g.hs)][0];   // (a real block of the same MCU)
  __syncthreads();
  if (dummy && l == 0) s_out[slot][0] = dc;
  __syncthreads();
  if (live) *(uint4*)(coef + 64 * (g.base[c] + (long long)by * g.bw[c] + bx) + 8 * l) = *(const uint4*)&s_out[slot][8 * l];
}

// ---- count, pack ---------------------------------------------------------------------------------------------------------------------
struct Codes {
  uint16_t code[4][256];
  uint8_t len[4][256];
};
__device__ __forceinline__ void codes_to_lds(Codes* dst, const Tables* __restrict__ tables) {
  for (int i = threadIdx.x; i < 4 * 256; i += kThreads) {
    (&dst->code[0][0])[i] = (&tables->code[0][0])[i];
    (&dst->len[0][0])[i] = (&tables->len[0][0])[i];
  }
  __syncthreads();
}
// block A's lane: its bits and the length of all it emits; *t: the DC table of the block's component
__device__ __forceinline__ LaneBits block_lane(const Geo& g, const Codes& cd, const int16_t* __restrict__ coef, long long A, int lane, int* t, int* length) {
  const int c = comp_of(g, (int)(A % g.bpm));
  *t = c ? 2 : 0;
  int32_t v = coef[64 * block_at(g, A) + zigzag(lane)];
  if (lane == 0) v -= dc_pred(g, coef, A);
  const uint64_t mask = __ballot(lane > 0 && v != 0);
  const LaneBits lb = lane_symbol(cd.code[*t], cd.len[*t], lane, v, mask);
  *length = lane_length(lb, cd.len[*t]);
  return lb;
}

__global__ __launch_bounds__(kThreads) void count_kernel(Frame f, const Tables* __restrict__ tables, const int16_t* __restrict__ coef, uint32_t* __restrict__ bits) {
  __shared__ Codes s_cd;
  codes_to_lds(&s_cd, tables);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < kPackBlocks / 4; ++j) {              // (wave-uniform)
    const long long A = (long long)blockIdx.x * kPackBlocks + wave * (kPackBlocks / 4) + j;
    if (A >= f.g.blocks) break;
    int t, length;
    block_lane(f.g, s_cd, coef, A, lane, &t, &length);
    const uint32_t total = wave_sum_u32((uint32_t)length);
    if (lane == 0) bits[A] = total;
  }
}

// a flagged element restarts the sum: (a then b) -> b if b is flagged, else a's flag and both values' sum
__device__ __forceinline__ uint64_t seg_combine(uint64_t a, uint64_t b) { return b & kFlag ? b : (a & kFlag) | ((a + b) & ~kFlag); }
// inclusive over the workgroup's kThreads lanes; s_w: kThreads / 64 words; *total: all of them
__device__ __forceinline__ uint64_t seg_block_scan(uint64_t x, uint64_t* s_w, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)x, o, 64);
    if (lane >= o) x = seg_combine(t, x);
  }
  __syncthreads();
  if (lane == 63) s_w[wave] = x;
  __syncthreads();
  uint64_t pre = 0, tot = 0;
  for (int i = 0; i < kThreads / 64; ++i) {
    if (i < wave) pre = seg_combine(pre, s_w[i]);
    tot = seg_combine(tot, s_w[i]);
  }
  *total = tot;
  return seg_combine(pre, x);
}

template <bool FINAL>
__global__ __launch_bounds__(kThreads) void place_kernel(Frame f, const uint32_t* __restrict__ bits, uint64_t* __restrict__ agg, uint64_t* __restrict__ within,
                                                         uint32_t* __restrict__ iv_bytes) {
  __shared__ uint64_t s_w[kThreads / 64];
  const long long A = (long long)blockIdx.x * kThreads + threadIdx.x;
  const bool live = A < f.g.blocks;
  const uint64_t v = live ? bits[A] : 0u;
  uint64_t total;
  const uint64_t incl = seg_block_scan(live && starts_interval(f.g, A) ? kFlag | v : v, s_w, &total);
  if (!FINAL) {
    if (threadIdx.x == 0) agg[blockIdx.x] = total;
    return;
  }
  if (!live) return;
  const uint64_t end = seg_combine(agg[blockIdx.x], incl) & ~kFlag;
  within[A] = end - v;
  if (ends_interval(f.g, A)) iv_bytes[interval_of(f.g, A)] = (uint32_t)((end + 7) >> 3);
}
// the tiles' sums -> what every tile starts from
__global__ __launch_bounds__(kThreads) void place_carry_kernel(uint64_t* __restrict__ agg, long long tiles) {
  __shared__ uint64_t s_w[kThreads / 64];
  __shared__ uint64_t s_x[kThreads];
  uint64_t run = 0;
  for (long long t0 = 0; t0 < tiles; t0 += kThreads) {     // (uniform)
    const long long t = t0 + threadIdx.x;
    uint64_t total;
    const uint64_t incl = seg_block_scan(t < tiles ? agg[t] : 0ull, s_w, &total);
    s_x[threadIdx.x] = incl;
    __syncthreads();
    if (t < tiles) agg[t] = seg_combine(run, threadIdx.x ? s_x[threadIdx.x - 1] : 0ull) & ~kFlag;
    run = seg_combine(run, total);
    __syncthreads();
  }
}
// exclusive prefix sums of count u32 words -> u64, one workgroup; the total to *sum
__global__ __launch_bounds__(kThreads) void scan_kernel(const uint32_t* __restrict__ v, long long count, uint64_t* __restrict__ out, uint64_t* __restrict__ sum) {
  __shared__ unsigned long long s_red[kThreads / 64 + 1];
  unsigned long long run = 0;
  for (long long i0 = 0; i0 < count; i0 += kThreads) {     // (uniform)
    const long long i = i0 + threadIdx.x;
    unsigned long long total;
    const unsigned long long x = i < count ? v[i] : 0u, excl = block_exscan<unsigned long long>(x, s_red, &total);
    if (i < count) out[i] = run + excl;
    run += total;
  }
  if (threadIdx.x == 0) *sum = run;
}

__global__ __launch_bounds__(kThreads) void zero_kernel(const uint64_t* __restrict__ head, uint4* __restrict__ stream) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (16 * i < (long long)head[kHeadStream] + 16) stream[i] = uint4{0u, 0u, 0u, 0u};
}

// ORs the low n bits of v (n <= 32) into the window at bit `at`, the first bit a word's top bit
__device__ __forceinline__ void window_put(uint32_t* win, uint32_t at, uint32_t v, int n) {
  if (n == 0) return;
  const uint64_t w = (uint64_t)v << (64 - n) >> (at & 31);
  atomicOr(&win[at >> 5], (uint32_t)(w >> 32));
  if ((uint32_t)w) atomicOr(&win[(at >> 5) + 1], (uint32_t)w);
}

// kWin: window_words of the most bits a block takes with the tables in use
template <int kWin>
__global__ __launch_bounds__(kThreads) void pack_kernel(Frame f, const Tables* __restrict__ tables, const int16_t* __restrict__ coef, const uint64_t* __restrict__ within,
                                                        const uint64_t* __restrict__ iv_start, const uint64_t* __restrict__ head, uint32_t* __restrict__ stream) {
  __shared__ Codes s_cd;
  __shared__ uint32_t s_win[kWin];
  const Geo& g = f.g;
  const long long g0 = (long long)blockIdx.x * kPackBlocks, g1 = min(g0 + kPackBlocks, (long long)g.blocks);
  auto first_bit = [&](long long A) { return 8 * iv_start[interval_of(g, A)] + within[A]; };
  const uint64_t lo = first_bit(g0), hi = g1 < g.blocks ? first_bit(g1) : 8 * head[kHeadStream];
  const long long base = (long long)(lo >> 5);
  const int words = (int)min((long long)((hi + 31) >> 5) - base, (long long)kWin - 1);   // (the bound on a block's bits bounds it; never cut)
  for (int i = threadIdx.x; i <= words; i += kThreads) s_win[i] = 0u;
  codes_to_lds(&s_cd, tables);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int j = 0; j < kPackBlocks / 4; ++j) {              // (wave-uniform)
    const long long A = g0 + wave * (kPackBlocks / 4) + j;
    if (A >= g1) break;
    int t, length;
    const LaneBits lb = block_lane(g, s_cd, coef, A, lane, &t, &length);
    const uint32_t incl = dpp_incscan_u32<64>((uint32_t)length);
    const uint32_t start = (uint32_t)(first_bit(A) - 32 * (uint64_t)base);
    uint32_t at = start + incl - (uint32_t)length;
    if (at + (uint32_t)length > 32u * (uint32_t)words) continue;       // (never: the window holds every block's most bits)
    for (int z = 0; z < lb.zrl; ++z) {                     // (at most 3)
      window_put(s_win, at, s_cd.code[t + 1][0xF0], s_cd.len[t + 1][0xF0]);
      at += s_cd.len[t + 1][0xF0];
    }
    window_put(s_win, at, lb.bits, lb.n);
    if (lane == 63 && ends_interval(g, A)) {               // the pad: ones up to the byte
      const uint32_t end = start + incl, pad = (0u - end) & 7u;
      window_put(s_win, end, (1u << pad) - 1u, (int)pad);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < words; i += kThreads) {
    const uint32_t v = bswap(s_win[i]);
    if (i == 0 || i == words - 1) {
      if (v) atomicOr(&stream[base + i], v);
    } else {
      stream[base + i] = v;
    }
  }
}

// ---- stuff ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ff_kernel(const uint8_t* __restrict__ stream, const uint64_t* __restrict__ head, uint32_t* __restrict__ tiles) {
  __shared__ uint32_t s_red[kThreads / 64];
  const long long n = (long long)head[kHeadStream], p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
  uint32_t count = 0;
  if (p0 < n) {
    union { uint4 w; uint8_t b[16]; } in;
    in.w = *(const uint4*)(stream + p0);
#pragma unroll
    for (int j = 0; j < 16; ++j) count += p0 + j < n && in.b[j] == 0xFF;
  }
  const uint32_t total = block_sum<uint32_t>(count, s_red);
  if (threadIdx.x == 0) tiles[blockIdx.x] = total;
}

__global__ __launch_bounds__(kThreads) void stuff_kernel(Frame f, const Tables* __restrict__ tables, const uint8_t* __restrict__ stream, uint64_t* __restrict__ head,
                                                         const uint64_t* __restrict__ tile_ff, const uint64_t* __restrict__ iv_start, uint8_t* __restrict__ out,
                                                         long long cap, int64_t* __restrict__ length) {
  __shared__ uint32_t s_red[kThreads / 64 + 1];
  const long long n = (long long)head[kHeadStream], hl = tables->header_len, p0 = ((long long)blockIdx.x * kThreads + threadIdx.x) * 16;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < hl && i < kHeaderMax && i < cap; i += kThreads) out[i] = tables->header[i];
    if (threadIdx.x == 0) {
      const long long end = hl + n + (long long)head[kHeadFF] + 2 * (f.n_iv - 1);
      if (end + 2 <= cap) out[end] = 0xFF, out[end + 1] = 0xD9;
      *length = end + 2;
    }
  }
  union { uint4 w; uint8_t b[16]; } in;
  in.w = uint4{0u, 0u, 0u, 0u};
  uint32_t count = 0;
  if (p0 < n) {
    in.w = *(const uint4*)(stream + p0);
#pragma unroll
    for (int j = 0; j < 16; ++j) count += p0 + j < n && in.b[j] == 0xFF;
  }
  const uint32_t excl = block_exscan<uint32_t>(count, s_red, nullptr);
  if (p0 >= n) return;
  long long lo = 0, hi = f.n_iv;                             // the last interval that starts at or in front of byte p0
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)iv_start[mid] <= p0) lo = mid; else hi = mid;
  }
  long long k = lo, at = hl + p0 + (long long)tile_ff[blockIdx.x] + excl + 2 * k;
  for (int j = 0; j < 16 && p0 + j < n; ++j) {
    if (j > 0 && k + 1 < f.n_iv && (long long)iv_start[k + 1] == p0 + j) ++k, at += 2;
    if (k > 0 && (long long)iv_start[k] == p0 + j && at <= cap) out[at - 2] = 0xFF, out[at - 1] = (uint8_t)(0xD0 + ((k - 1) & 7));
    if (at < cap) out[at] = in.b[j];
    ++at;
    if (in.b[j] == 0xFF) {
      if (at < cap) out[at] = 0;
      ++at;
    }
  }
}

// ---- layouts and launches ------------------------------------------------------------------------------------------------------------
// the entropy stage's workspace: the head, the blocks' bits and places, the place tiles, the intervals' bytes and first bytes, the stuff
// tiles' counts and their prefix, the unstuffed stream (a tile's worth behind it: the stuff launches read whole 16 bytes)
struct Layout { int64_t place_tiles, stuff_tiles, o_bits, o_within, o_agg, o_ivb, o_ivs, o_tiles, o_tff, o_stream, total; };
static Layout layout_of(const Frame& f, int block_bits = kBlockBits) {
  Layout l;
  l.place_tiles = (f.g.blocks + kThreads - 1) / kThreads;
  l.stuff_tiles = (stream_cap(f, block_bits) + kTileBytes - 1) / kTileBytes;
  l.o_bits = 256;
  l.o_within = align256(l.o_bits + 4 * f.g.blocks);
  l.o_agg = align256(l.o_within + 8 * f.g.blocks);
  l.o_ivb = align256(l.o_agg + 8 * l.place_tiles);
  l.o_ivs = align256(l.o_ivb + 4 * f.n_iv);
  l.o_tiles = align256(l.o_ivs + 8 * f.n_iv);
  l.o_tff = align256(l.o_tiles + 4 * l.stuff_tiles);
  l.o_stream = align256(l.o_tff + 8 * l.stuff_tiles);
  l.total = align256(l.o_stream + (l.stuff_tiles + 1) * kTileBytes);
  return l;
}
static int strip_of(const Geo& g) {
  const int by_blocks = kPackBlocks / g.bpm, by_px = (g.n_comp == 1 ? 2 : 1) * kStripPx / (8 * g.hs);
  return by_blocks < by_px ? by_blocks : by_px;
}

int blocks_launch(rhccq_ctx* ctx, const Frame& f, const Tables* tables_dev, const uint8_t* img, int16_t* coef) {
  const int strip = strip_of(f.g);
  hipLaunchKernelGGL(blocks_kernel, dim3((unsigned)((f.g.mcus_x + strip - 1) / strip), (unsigned)(f.g.mcus / f.g.mcus_x)), dim3(kThreads), 0, ctx->stream, f, tables_dev,
                     img, strip, coef);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int64_t entropy_workspace(const Frame& f, int block_bits) { return layout_of(f, block_bits).total; }

int entropy_launch(rhccq_ctx* ctx, const Frame& f, int block_bits, const Tables* tables_dev, const int16_t* coef, void* workspace, uint8_t* out, int64_t cap, int64_t* length) {
  const Layout l = layout_of(f, block_bits);
  uint8_t* ws = (uint8_t*)workspace;
  uint64_t* head = (uint64_t*)ws;
  uint32_t* bits = (uint32_t*)(ws + l.o_bits);
  uint64_t* within = (uint64_t*)(ws + l.o_within);
  uint64_t* agg = (uint64_t*)(ws + l.o_agg);
  uint32_t* iv_bytes = (uint32_t*)(ws + l.o_ivb);
  uint64_t* iv_start = (uint64_t*)(ws + l.o_ivs);
  uint32_t* tiles = (uint32_t*)(ws + l.o_tiles);
  uint64_t* tile_ff = (uint64_t*)(ws + l.o_tff);
  uint8_t* stream = ws + l.o_stream;
  const hipStream_t st = ctx->stream;
  const dim3 wg(kThreads), one(1), per_pack((unsigned)((f.g.blocks + kPackBlocks - 1) / kPackBlocks)), per_place((unsigned)l.place_tiles),
      per_stuff((unsigned)l.stuff_tiles);
  hipLaunchKernelGGL(count_kernel, per_pack, wg, 0, st, f, tables_dev, coef, bits);
  hipLaunchKernelGGL(place_kernel<false>, per_place, wg, 0, st, f, (const uint32_t*)bits, agg, within, iv_bytes);
  hipLaunchKernelGGL(place_carry_kernel, one, wg, 0, st, agg, (long long)l.place_tiles);
  hipLaunchKernelGGL(place_kernel<true>, per_place, wg, 0, st, f, (const uint32_t*)bits, agg, within, iv_bytes);
  hipLaunchKernelGGL(scan_kernel, one, wg, 0, st, (const uint32_t*)iv_bytes, (long long)f.n_iv, iv_start, head + kHeadStream);
  hipLaunchKernelGGL(zero_kernel, dim3((unsigned)(l.stuff_tiles + 1)), wg, 0, st, (const uint64_t*)head, (uint4*)stream);
  if (block_bits == kBlockBits)
    hipLaunchKernelGGL(pack_kernel<kWindowWords>, per_pack, wg, 0, st, f, tables_dev, coef, (const uint64_t*)within, (const uint64_t*)iv_start, (const uint64_t*)head, (uint32_t*)stream);
  else
    hipLaunchKernelGGL(pack_kernel<window_words(kBlockBitsOpt)>, per_pack, wg, 0, st, f, tables_dev, coef, (const uint64_t*)within, (const uint64_t*)iv_start, (const uint64_t*)head,
                       (uint32_t*)stream);
  hipLaunchKernelGGL(ff_kernel, per_stuff, wg, 0, st, (const uint8_t*)stream, (const uint64_t*)head, tiles);
  hipLaunchKernelGGL(scan_kernel, one, wg, 0, st, (const uint32_t*)tiles, (long long)l.stuff_tiles, tile_ff, head + kHeadFF);
  hipLaunchKernelGGL(stuff_kernel, per_stuff, wg, 0, st, f, tables_dev, (const uint8_t*)stream, head, (const uint64_t*)tile_ff, (const uint64_t*)iv_start, out,
                     (long long)cap, length);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static bool sized(const Frame& f) { return file_cap(f) <= kFileMax; }

}  // namespace jpegw
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::jpegw;

extern "C" {

int32_t rhccq_jpeg_write_tables_bytes(void) { return (int32_t)sizeof(Tables); }

int rhccq_jpeg_write_tables_host(int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, void* tables) {
  if (!tables || !args_ok(H, W, mode, quality, restart_rows)) return RHCCQ_E_ARG;
  tables_build(frame_of(H, W, mode, restart_rows), quality, (Tables*)tables);
  return RHCCQ_OK;
}

int rhccq_jpeg_write_sizes(int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, int64_t* coefficients, int64_t* entropy_bytes, int64_t* encode_bytes,
                           int64_t* file_bytes) {
  if (!coefficients || !entropy_bytes || !encode_bytes || !file_bytes || !args_ok(H, W, mode, quality, restart_rows)) return RHCCQ_E_ARG;
  const Frame f = frame_of(H, W, mode, restart_rows);
  if (!sized(f)) return RHCCQ_E_ARG;
  *coefficients = 64 * f.g.blocks;
  *entropy_bytes = layout_of(f).total;
  *encode_bytes = *entropy_bytes + align256(128 * f.g.blocks);
  *file_bytes = file_cap(f);
  return RHCCQ_OK;
}

int rhccq_jpeg_blocks(rhccq_ctx* ctx, const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, const void* tables_dev, int16_t* coef) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!args_ok(H, W, mode, quality, 0)) return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_blocks: quality outside 1..100, an unknown mode, or H or W outside 1..65535");
  if (!image || !tables_dev || !coef || (uintptr_t)image % 16 || (uintptr_t)tables_dev % 4 || (uintptr_t)coef % 16)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_blocks: a null or misaligned pointer (image and coef: 16 bytes)");
  return blocks_launch(ctx, frame_of(H, W, mode, 0), (const Tables*)tables_dev, image, coef);
}

int rhccq_jpeg_entropy(rhccq_ctx* ctx, const int16_t* coef, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, const void* tables_dev,
                       void* workspace, uint8_t* out, int64_t cap, int64_t* length) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!args_ok(H, W, mode, quality, restart_rows))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_entropy: quality outside 1..100, an unknown mode, H or W outside 1..65535, or negative restart rows");
  const Frame f = frame_of(H, W, mode, restart_rows);
  if (!coef || !tables_dev || !workspace || !out || !length || (uintptr_t)coef % 16 || (uintptr_t)tables_dev % 4 || (uintptr_t)workspace % 256 || (uintptr_t)length % 8 ||
      !sized(f) || cap < file_cap(f))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_entropy: a null or misaligned pointer, or cap below rhccq_jpeg_write_sizes' file_bytes");
  return entropy_launch(ctx, f, kBlockBits, (const Tables*)tables_dev, coef, workspace, out, cap, length);
}

int rhccq_jpeg_encode(rhccq_ctx* ctx, const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, const void* tables_dev,
                      void* workspace, uint8_t* out, int64_t cap, int64_t* length) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!args_ok(H, W, mode, quality, restart_rows))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_encode: quality outside 1..100, an unknown mode, H or W outside 1..65535, or negative restart rows");
  const Frame f = frame_of(H, W, mode, restart_rows);
  if (!image || !workspace || (uintptr_t)image % 16 || (uintptr_t)workspace % 256 || !sized(f))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_encode: a null or misaligned image or workspace");
  int16_t* coef = (int16_t*)((uint8_t*)workspace + layout_of(f).total);
  if (!tables_dev || (uintptr_t)tables_dev % 4) return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_encode: a null or misaligned table pointer");
  if (const int rc = blocks_launch(ctx, f, (const Tables*)tables_dev, image, coef)) return rc;
  return rhccq_jpeg_entropy(ctx, coef, H, W, mode, quality, restart_rows, tables_dev, workspace, out, cap, length);
}

int rhccq_jpeg_blocks_host(const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, int16_t* coef) {
  if (!image || !coef || !args_ok(H, W, mode, quality, 0)) return RHCCQ_E_ARG;
  const Frame f = frame_of(H, W, mode, 0);
  std::vector<Tables> T(1);
  tables_build(f, quality, T.data());
  blocks_serial(f, T[0], image, coef);
  return RHCCQ_OK;
}

int rhccq_jpeg_encode_host(const uint8_t* image, int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows, uint8_t* out, int64_t cap, int64_t* length) {
  if (!image || !out || !length || cap < 0 || !args_ok(H, W, mode, quality, restart_rows)) return RHCCQ_E_ARG;
  const Frame f = frame_of(H, W, mode, restart_rows);
  std::vector<Tables> T(1);
  tables_build(f, quality, T.data());
  std::vector<int16_t> coef((size_t)(64 * f.g.blocks));
  blocks_serial(f, T[0], image, coef.data());
  *length = encode_serial(f, T[0], coef.data(), out, cap);
  return *length < 0 ? RHCCQ_E_ARG : RHCCQ_OK;
}

}  // extern "C"
