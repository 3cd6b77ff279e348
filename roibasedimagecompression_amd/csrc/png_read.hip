// PNG files read on the device (EXTENSION, include/rhccq.h): chunk CRCs, the IDAT join, the row filters undone and the pixels expanded,
// around the stream decoder of zlib_inflate.hip.  The definitions both sides share are in png_read.h; the host forms at the end run them
// serially.
//
//   crc_seg_partials   a workgroup per (segment, 16 KiB piece): it finds its segment by a search over the table's first_piece column and
//                      takes the piece's plain remainder with the function rhccq_crc32's kernel uses (png_write.h).
//   crc_seg_join       a wave per segment: a lane folds a run of consecutive pieces (Horner), lane 0 joins the 64 runs, takes the zero
//                      bytes behind the message off again and brings the standard start and end in.
//   idat_join_kernel   one launch over the joined stream: a lane builds 16 bytes of it; it finds the chunk of its first byte by a search
//                      over the IDAT rows' dst column and walks on from there (empty IDATs share their dst with the chunk behind them).
//                      A pass of its own, not fused with the CRC's (a fused pass was not built, so not measured): the CRC reads aligned
//                      16-byte words of whole chunks (type field included), the join writes aligned words of the stream, and the two
//                      alignments differ per chunk.  At 7 to 23 us on a 4K file it is not where the time goes.
//   unfilter_kernel    see below.
//   expand_kernel      a lane a pixel.
//   finish_kernel      one workgroup: the first chunk whose stored CRC differs, the inflater's status and length, the unfilter's words ->
//                      status[2] by the precedence of include/rhccq.h.
//
// The unfilter.  Raw byte (y, i) depends on (y, i - bpp), (y - 1, i) and (y - 1, i - bpp): with a filter unit of bpp bytes, unit (y, x) can
// run at step x + y.  A workgroup is ONE wave and owns a band of 64 consecutive rows, a lane a row; at step u lane r stands at unit u - r.
//   above       what lane r - 1 produced a step ago, taken across lanes (__shfl_up: ds_bpermute); upper left is the "above" of the step
//               before, left the lane's own last unit: all in registers, a unit as two dwords;
//   bytes       go through LDS in tiles of 32 steps, skewed like the wavefront (row q of a tile holds the units u0 - q ...): all lanes load
//               a row segment per row (consecutive bytes: a row starts at any byte offset, a row being rowbytes + 1 bytes long; outside
//               the row they are zero, not branched around), the walk reads and writes LDS only, and the raw bytes leave the same way.
//               The loads are aligned dwords (the row's misalignment is an offset into its LDS row), a lane takes every 64th dword of
//               the tile, and the loads of tile T + 1 are issued before the walk of tile T and land behind it;
//   between bands   row 0 of band n needs the last row of band n - 1: the hand-over of band_handoff.h, which also holds the
//               forward-progress argument (a band that gives up sets the stalled word).  That row's lane stores every unit as one to three
//               words (three bytes and the mark each) as it produces them; band n fetches a granule of 16 units at a time.  A band whose
//               first row has filter type 0 or 1 reads nothing of the row above and does not wait at all.
#include "png_read.h"
#include "rhccq_common.h"

#include <vector>

namespace rhccq {
namespace pngr {

// ---- segment CRCs --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kCrcBlock) void crc_seg_partials(const uint8_t* __restrict__ data, long long n, const rhccq_segment* __restrict__ table,
                                                              long long n_seg, long long extra, CrcConsts k, uint32_t* __restrict__ partials) {
  __shared__ CrcPieceLds lds;
  const long long b = blockIdx.x;
  long long lo = 0, hi = n_seg;                                      // the last row whose first_piece is <= b (empty rows stand in front of it)
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (table[mid].first_piece <= b) lo = mid; else hi = mid;
  }
  const rhccq_segment seg = table[lo];
  const long long len = seg_bytes(seg.offset, seg.length, extra, n), rel = b - seg.first_piece;
  const long long front = seg.offset & 15, end = front + len;
  if (rel < 0 || len == 0 || rel > (end - 1) / kCrcPiece) {          // (uniform) a table that does not hold what the plan wrote
    if (threadIdx.x == 0) partials[b] = 0u;
    return;
  }
  const uint32_t r = crc_piece_remainder(lds, data + (seg.offset - front), front, end, rel * kCrcPiece, k);
  if (threadIdx.x == 0) partials[b] = r;
}

__global__ __launch_bounds__(64) void crc_seg_join(const rhccq_segment* __restrict__ table, long long extra, long long n, long long total, CrcConsts k,
                                                   const uint32_t* __restrict__ partials, uint32_t* __restrict__ crc_out) {
  const long long s = blockIdx.x;
  const int lane = threadIdx.x;
  const rhccq_segment seg = table[s];
  const long long len = seg_bytes(seg.offset, seg.length, extra, n), front = seg.offset & 15;
  const long long pieces = len == 0 ? 0 : crc_pieces(front, len);
  if (pieces == 0 || seg.first_piece < 0 || seg.first_piece > total - pieces) {   // (uniform) the CRC of no bytes
    if (lane == 0) crc_out[s] = 0u;
    return;
  }
  const long long run = (pieces + 63) / 64, i0 = lane * run, i1 = i0 + run < pieces ? i0 + run : pieces;
  uint32_t r = 0;
  for (long long i = i0; i < i1; ++i) r = crc_mul(r, k.piece) ^ partials[seg.first_piece + i];
  const long long mine = i1 > i0 ? i1 - i0 : 0;
  const uint32_t p_run = crc_xpow(k.x2n, 8ull * kCrcPiece * (unsigned long long)run);
  uint32_t all = 0;
  for (int i = 0; i < 64; ++i) {                                     // (the same in every lane)
    const uint32_t ri = __shfl(r, i, 64);
    const long long ci = __shfl((int)mine, i, 64);
    if (ci == 0) continue;
    all = crc_mul(all, ci == run ? p_run : crc_xpow(k.x2n, 8ull * kCrcPiece * (unsigned long long)ci)) ^ ri;
  }
  if (lane == 0) {
    const unsigned long long z = (unsigned long long)(pieces * kCrcPiece - (front + len));
    const uint64_t e_back = (kCrcOrder - (8ull * z) % kCrcOrder) % kCrcOrder;
    crc_out[s] = crc_mul(0xFFFFFFFFu, crc_xpow(k.x2n, 8ull * (unsigned long long)len)) ^ crc_mul(all, crc_xpow(k.x2n, e_back)) ^ 0xFFFFFFFFu;
  }
}

static int crc_segments_launch(rhccq_ctx* ctx, const uint8_t* data, int64_t n, const rhccq_segment* table_dev, int64_t n_seg, int64_t extra,
                               int64_t total, uint32_t* partials, uint32_t* crc_out) {
  if (n_seg == 0) return 0;
  const CrcConsts k = crc_consts(1);
  if (total > 0)
    hipLaunchKernelGGL(crc_seg_partials, dim3((unsigned)total), dim3(kCrcBlock), 0, ctx->stream, data, (long long)n, table_dev, (long long)n_seg,
                       (long long)extra, k, partials);
  hipLaunchKernelGGL(crc_seg_join, dim3((unsigned)n_seg), dim3(64), 0, ctx->stream, table_dev, (long long)extra, (long long)n, (long long)total, k,
                     (const uint32_t*)partials, crc_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// ---- the IDAT join -------------------------------------------------------------------------------------------------------------------
// table: the `count` IDAT rows (dst ascending); stream is aligned to 16 and holds total rounded up to 16 bytes
__global__ __launch_bounds__(256) void idat_join_kernel(const uint8_t* __restrict__ file, long long n, const rhccq_segment* __restrict__ table, int count,
                                                        long long total, uint8_t* __restrict__ stream) {
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= total) return;
  int lo = 0, hi = count;                                            // the last row whose dst is <= p0
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid].dst <= p0) lo = mid; else hi = mid;
  }
  int c = lo;
  rhccq_segment seg = table[c];
  long long next = c + 1 < count ? table[c + 1].dst : total;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const long long p = p0 + j;
    if (p >= total) break;
    while (c + 1 < count && next <= p) {
      seg = table[++c];
      next = c + 1 < count ? table[c + 1].dst : total;
    }
    const long long off = p - seg.dst, src = seg.offset + 4 + off;
    const uint32_t v = off >= 0 && off < seg.length && src >= 0 && src < n ? file[src] : 0u;
    w[j >> 2] |= v << (8 * (j & 3));
  }
  *(uint4*)(stream + p0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- unfilter ------------------------------------------------------------------------------------------------------------------------
struct Unit { uint32_t w[2]; };
__device__ __forceinline__ uint32_t unit_byte(const Unit& v, int j) { return (v.w[j >> 2] >> (8 * (j & 3))) & 255u; }

// the dwords of a tile's rows on their way from global memory to LDS, kept exactly as loaded
template <int DW>
struct UnfTile { uint32_t w[DW]; };

// loads only: pair p = i * 64 + lane is dword p % DW of the tile's row p / DW.  Row q of the tile that starts at step u0 holds the bytes
// from (u0 - q) * BPP of image row y0 + q on, and its dwords are laid from the 4-byte aligned address at or below the first of them: a row
// starts at any byte offset.  Rows past the band's last repeat it, and an address outside the dwords that hold a byte of the scanlines is
// moved to the nearest one that does (such bytes are only ever read by steps that are not active).
template <int BPP, int DW>
__device__ __forceinline__ void unf_load(UnfTile<DW>& t, const uint8_t* base, int rel0, int in_pitch, int y0, int nrows, int u0, int span, int lane) {
  // base: the aligned address at or below the scanlines, rel0 their first byte behind it, span the last dword that holds a byte of them;
  // the scanlines are below 2 GiB, so every offset is an int (negative in front of the first row)
#pragma unroll
  for (int i = 0; i < DW; ++i) {
    const int p = i * kUnfRows + lane, q = p / DW, k = p - q * DW;
    const int g = rel0 + (y0 + min(q, nrows - 1)) * in_pitch + 1 + (u0 - q) * BPP;
    const int a = min(max((g & ~3) + 4 * k, 0), span);
    t.w[i] = *(const uint32_t*)(base + (uint32_t)a);
  }
}

template <int BPP>
__global__ __launch_bounds__(kUnfRows) void unfilter_kernel(const uint8_t* __restrict__ scan, int H, long long rowbytes, uint8_t* __restrict__ raw,
                                                            uint32_t* work) {
  constexpr int WPU = (BPP + 2) / 3, NW = BPP > 4 ? 2 : 1;
  constexpr int kTileBytes = kUnfTile * BPP;
  constexpr int DW = (kTileBytes + 3) / 4 + 1, kInPitch = DW | 1;    // dwords of a tile row whatever its misalignment; an odd pitch: the rows' lanes hit different banks
  constexpr int kOutPitch = kTileBytes + 4;                          // (bytes: consecutive rows start a bank apart)
  __shared__ uint32_t s_in[kUnfRows * kInPitch];
  __shared__ __attribute__((aligned(4))) uint8_t s_out[kUnfRows * kOutPitch];
  __shared__ uint32_t s_band;
  const int lane = threadIdx.x, r = lane;
  band::draw_ticket(work, &s_band, lane);
  __syncthreads();

  const int nbands = (H + kUnfRows - 1) / kUnfRows, band = (int)s_band;
  if (band >= nbands) return;                                        // (the grid has exactly nbands workgroups)
  const long long y0 = (long long)band * kUnfRows;
  const int nrows = (int)min((long long)kUnfRows, H - y0);
  const long long units = rowbytes / BPP, nsteps = units + nrows - 1, nwords = units * WPU;
  const long long in_pitch = rowbytes + 1;
  const int rel0 = (int)((uintptr_t)scan & 3), span = (int)((rel0 + H * in_pitch - 1) & ~3ll);   // (H * in_pitch < 2^31: the argument test)
  const uint8_t* base = scan - rel0;
  const uint32_t* up_words = band::words(work, band - 1, nwords);    // (band > 0 only) the last row of the band above
  uint32_t* my_words = band::words(work, band, nwords);
  const bool hand_on = band + 1 < nbands;

  UnfTile<DW> tile;
  unf_load<BPP, DW>(tile, base, rel0, (int)in_pitch, (int)y0, nrows, 0, span, lane);
  int t = r < nrows ? (int)scan[(y0 + r) * in_pitch] : 0;
  if (t > 4) {
    __hip_atomic_fetch_max(&work[kUnfBadWord], (uint32_t)(H - (y0 + r)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // H - row: the first bad row wins
    t = 0;
  }
  bool waiting = band > 0 && __builtin_amdgcn_readfirstlane(t) >= 2; // (wave uniform) false once a band has given up
  uint32_t gran = 0u, pending = 0u;                                  // lanes 0 .. 16 WPU - 1: the band above's words of this granule, of the next
  Unit left{{0u, 0u}}, up{{0u, 0u}}, last{{0u, 0u}};
  const uint8_t* s_in_bytes = reinterpret_cast<const uint8_t*>(s_in);
  const int row_byte0 = rel0 + (int)((y0 + min(r, nrows - 1)) * in_pitch) + 1 - r * BPP;   // the lane's row: its byte at step 0, counted from base

  for (long long u0 = 0; u0 < nsteps; u0 += kUnfTile) {              // (wave uniform throughout)
    const int ns = (int)min((long long)kUnfTile, nsteps - u0);
#pragma unroll
    for (int i = 0; i < DW; ++i) {
      const int p = i * kUnfRows + lane, q = p / DW;
      s_in[q * kInPitch + (p - q * DW)] = tile.w[i];
    }
    __syncthreads();
    if (u0 + kUnfTile < nsteps) unf_load<BPP, DW>(tile, base, rel0, (int)in_pitch, (int)y0, nrows, (int)u0 + kUnfTile, span, lane);   // lands behind the walk
    const int o_in = r * kInPitch * 4 + ((row_byte0 + (int)u0 * BPP) & 3), o_out = r * kOutPitch;
    Unit cur_next{{0u, 0u}};                                         // a step's bytes are read one step ahead of their use
#pragma unroll
    for (int j = 0; j < BPP; ++j) cur_next.w[j >> 2] |= (uint32_t)s_in_bytes[o_in + j] << (8 * (j & 3));

    for (int s = 0; s < ns; ++s) {
      const long long u = u0 + s;
      if (waiting && (u & (kUnfGranule - 1)) == 0)                   // the words of the units u .. u + 15 of the row above
        band::fetch_granule<kUnfGranule * WPU>(up_words, u * WPU, nwords, lane, work + band::kAbortWord, work + kUnfStalledWord, waiting, gran, pending);
      const long long x = u - r;
      const bool active = r < nrows && x >= 0 && x < units;
      const Unit cur = cur_next;
      cur_next = Unit{{0u, 0u}};
#pragma unroll
      for (int j = 0; j < BPP; ++j) cur_next.w[j >> 2] |= (uint32_t)s_in_bytes[o_in + min(s + 1, kUnfTile - 1) * BPP + j] << (8 * (j & 3));
      // the unit above: from the band above for row 0, else what the lane above produced a step ago
      Unit above{{0u, 0u}};
#pragma unroll
      for (int kk = 0; kk < WPU; ++kk) {
        const uint32_t word = (uint32_t)__builtin_amdgcn_readlane((int)gran, (int)(u & (kUnfGranule - 1)) * WPU + kk) & 0xFFFFFFu;
#pragma unroll
        for (int j = 3 * kk; j < 3 * kk + 3 && j < BPP; ++j) above.w[j >> 2] |= ((word >> (8 * (j - 3 * kk))) & 255u) << (8 * (j & 3));
      }
      Unit from_row;
#pragma unroll
      for (int i = 0; i < 2; ++i) from_row.w[i] = i < NW ? (uint32_t)__shfl_up((int)last.w[i], 1, kUnfRows) : 0u;
      if (r != 0) above = from_row;
      const Unit ul = up;
      up = above;
      Unit out{{0u, 0u}};
#pragma unroll
      for (int j = 0; j < BPP; ++j)
        out.w[j >> 2] |= unf_byte(t, unit_byte(cur, j), unit_byte(left, j), unit_byte(up, j), unit_byte(ul, j)) << (8 * (j & 3));
      if (!active) out = Unit{{0u, 0u}};
      last = out;
      if (active) {
        left = out;
#pragma unroll
        for (int j = 0; j < BPP; ++j) s_out[o_out + s * BPP + j] = (uint8_t)unit_byte(out, j);
        if (hand_on && r == kUnfRows - 1) {
#pragma unroll
          for (int kk = 0; kk < WPU; ++kk) {
            uint32_t word = band::kWritten;
#pragma unroll
            for (int j = 3 * kk; j < 3 * kk + 3 && j < BPP; ++j) word |= unit_byte(out, j) << (8 * (j - 3 * kk));
            band::word_store(my_words + x * WPU + kk, word);
          }
        }
      }
    }
    __syncthreads();

    // the raw bytes leave: pair p = i * 64 + lane is byte p % (32 BPP) of the tile's row p / (32 BPP); a wave's store is consecutive bytes
#pragma unroll 8
    for (int i = 0; i < kTileBytes; ++i) {
      const int p = i * kUnfRows + lane, q = p / kTileBytes, j = p - q * kTileBytes;
      const long long bi = (u0 - q) * BPP + j;
      if (q < nrows && j < ns * BPP && bi >= 0 && bi < rowbytes) raw[(y0 + q) * rowbytes + bi] = s_out[q * kOutPitch + j];
    }
    __syncthreads();                                                 // the next tile overwrites both arrays
  }
}

__global__ void unfilter_status_kernel(const uint32_t* __restrict__ work, int H, int32_t* __restrict__ status) {
  const Verdict v = png_verdict(-1, RHCCQ_ZS_OK, 0, 0, work[kUnfBadWord], H, work[kUnfStalledWord]);
  status[0] = v.status;
  status[1] = v.detail;
}

static int unfilter_check(int64_t H, int64_t rowbytes, int bpp) {
  return H < 1 || rowbytes < 1 || !bpp_allowed(bpp) || rowbytes % bpp || (rowbytes + 1) > kReadMax / H ? RHCCQ_E_ARG : 0;
}

static int unfilter_launch(rhccq_ctx* ctx, const uint8_t* scan, int H, int64_t rowbytes, int bpp, uint8_t* raw, uint32_t* work) {
  RHCCQ_HIP(ctx, hipMemsetAsync(work, 0, (size_t)unf_work_bytes(H, rowbytes, bpp), ctx->stream));   // the ticket, the abort word, every hand-over word
  const dim3 grid((unsigned)unf_bands(H)), block(kUnfRows);
#define RHCCQ_UNF_CASE(B_) \
  case B_: hipLaunchKernelGGL(unfilter_kernel<B_>, grid, block, 0, ctx->stream, scan, H, (long long)rowbytes, raw, work); break;
  switch (bpp) {
    RHCCQ_UNF_CASE(1) RHCCQ_UNF_CASE(2) RHCCQ_UNF_CASE(3) RHCCQ_UNF_CASE(4) RHCCQ_UNF_CASE(6) RHCCQ_UNF_CASE(8)
    default: return rhccq_fail(ctx, RHCCQ_E_ARG, "png_unfilter: bpp must be 1, 2, 3, 4, 6 or 8");
  }
#undef RHCCQ_UNF_CASE
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// ---- expand --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void expand_kernel(const uint8_t* __restrict__ raw, int H, int W, int ct, int depth, long long rowbytes,
                                                     const uint8_t* __restrict__ palette, int K, const uint8_t* __restrict__ trns, int trns_bytes,
                                                     uint8_t* __restrict__ rgb, uint8_t* __restrict__ alpha, uint8_t* __restrict__ idx) {
  const long long total = (long long)H * W;
  for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < total; o += (long long)gridDim.x * blockDim.x) {
    const long long y = o / W, x = o - y * W;
    const Pixel p = expand_pixel(raw + y * rowbytes, x, ct, depth, palette, K, trns, trns_bytes);
    rgb[3 * o] = p.r;
    rgb[3 * o + 1] = p.g;
    rgb[3 * o + 2] = p.b;
    if (alpha) alpha[o] = p.a;
    if (idx && ct == 3) idx[o] = p.idx;
  }
}

static int expand_launch(rhccq_ctx* ctx, const uint8_t* raw, int H, int W, int ct, int depth, const uint8_t* palette, int K, const uint8_t* trns,
                         int trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const int64_t total = (int64_t)H * W, blocks = (total + 255) / 256, cap = (int64_t)ctx->compute_units * 32;
  hipLaunchKernelGGL(expand_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, ctx->stream, raw, H, W, ct, depth,
                     (long long)rowbytes_of(W, ct, depth), palette, K, trns, trns_bytes, rgb, alpha, idx);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// ---- the whole file ------------------------------------------------------------------------------------------------------------------
__global__ void set_status_kernel(int32_t a, int32_t b, int32_t* __restrict__ status) {
  status[0] = a;
  status[1] = b;
}

// crcs: NULL when the CRCs are not checked
__global__ __launch_bounds__(256) void finish_kernel(const uint8_t* __restrict__ file, long long n, const rhccq_segment* __restrict__ table, int n_chunks,
                                                     const uint32_t* __restrict__ crcs, const long long* __restrict__ zlen, const int32_t* __restrict__ zs,
                                                     long long scan_bytes, const uint32_t* __restrict__ unf, int H, int32_t* __restrict__ status) {
  __shared__ int s_first;
  if (threadIdx.x == 0) s_first = 0x7FFFFFFF;
  __syncthreads();
  if (crcs) {
    for (int i = threadIdx.x; i < n_chunks; i += 256) {
      const rhccq_segment seg = table[i];
      bool ok = seg_bytes(seg.offset, seg.length, 8, n) != 0;        // type, data and the stored CRC lie inside the file
      if (ok) {
        const uint8_t* p = file + seg.offset + 4 + seg.length;
        ok = ((uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]) == crcs[i];
      }
      if (!ok) atomicMin(&s_first, i);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const Verdict v = png_verdict(s_first == 0x7FFFFFFF ? -1 : s_first, *zs, *zlen, scan_bytes, unf[kUnfBadWord], H, unf[kUnfStalledWord]);
    status[0] = v.status;
    status[1] = v.detail;
  }
}

struct ReadLayout {
  int64_t o_head, o_crc, o_part, o_stream, o_scan, o_raw, o_unf, o_inf, total;
};
static int read_layout(const rhccq_png_info& f, ReadLayout& l) {
  int64_t inf = 0;
  if (const int rc = rhccq_zlib_inflate_sizes(f.idat_bytes, f.scan_bytes, &inf)) return rc;
  l.o_head = 0;                                                      // the stream's length (int64), the inflater's status (int32 at + 8)
  l.o_crc = 256;
  l.o_part = align256(l.o_crc + 4 * (int64_t)f.n_chunks);
  l.o_stream = align256(l.o_part + 4 * (f.crc_pieces + 1));
  l.o_scan = align256(l.o_stream + f.idat_bytes + 16);
  l.o_raw = align256(l.o_scan + f.scan_bytes);
  l.o_unf = align256(l.o_raw + f.rowbytes * f.height);
  l.o_inf = align256(l.o_unf + unf_work_bytes(f.height, f.rowbytes, f.bpp));
  l.total = l.o_inf + inf;
  return 0;
}

// what rhccq_png_decode asks of an info it did not make itself: the fields a kernel's bounds rest on
static bool info_sound(const rhccq_png_info& f, int64_t n) {
  if (f.width < 1 || f.height < 1 || !depth_allowed(f.colour_type, f.depth)) return false;
  if (f.channels != channels_of(f.colour_type) || f.bpp != bpp_of(f.colour_type, f.depth) || f.rowbytes != rowbytes_of(f.width, f.colour_type, f.depth)) return false;
  if (f.rowbytes + 1 > kReadMax / f.height || f.scan_bytes != (f.rowbytes + 1) * f.height) return false;
  if (f.n_chunks < 1 || f.n_chunks > n / 12 || f.n_idat < 1 || f.first_idat < 0 || f.first_idat > f.n_chunks - f.n_idat) return false;
  if (f.idat_bytes < 0 || f.idat_bytes > n || f.crc_pieces < 0 || f.crc_pieces > n / kCrcPiece + 2 * (int64_t)f.n_chunks) return false;
  if (f.colour_type == 3 && (f.palette_rows < 1 || f.palette_rows > 256 || f.plte_offset < 0 || f.plte_offset > n - 3 * f.palette_rows)) return false;
  if (f.trns_bytes < 0 || f.trns_bytes > 256 || (f.trns_bytes > 0 && (f.trns_offset < 0 || f.trns_offset > n - f.trns_bytes))) return false;
  return true;
}

}  // namespace pngr
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::png;
using namespace rhccq::pngr;

extern "C" {

int rhccq_png_parse_host(const uint8_t* file, int64_t n, rhccq_png_info* info, rhccq_segment* chunks, int64_t chunks_cap, int64_t* n_chunks) {
  if (n < 0 || (n > 0 && !file) || !info || !n_chunks || chunks_cap < 0 || (chunks_cap > 0 && !chunks)) return RHCCQ_E_ARG;
  *n_chunks = png_parse(file, n, info, chunks, chunks_cap);
  return RHCCQ_OK;
}

int rhccq_crc32_segments_plan(rhccq_segment* table, int64_t n_seg, int64_t extra, int64_t* total_pieces) {
  if (n_seg < 0 || (n_seg > 0 && !table) || extra < 0 || !total_pieces) return RHCCQ_E_ARG;
  *total_pieces = seg_plan(table, n_seg, extra);
  return RHCCQ_OK;
}

int rhccq_crc32_segments(rhccq_ctx* ctx, const uint8_t* data, int64_t n, const rhccq_segment* table_dev, int64_t n_seg, int64_t extra,
                         int64_t total_pieces, void* workspace, uint32_t* crc_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || (n > 0 && !data) || n_seg < 0 || n_seg > kReadMax || extra < 0 || total_pieces < 0 || total_pieces > kReadMax ||
      (n_seg > 0 && (!table_dev || !crc_out || !workspace)) || (uintptr_t)data % 16 || (uintptr_t)table_dev % 8 || (uintptr_t)workspace % 4 ||
      (uintptr_t)crc_out % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "crc32_segments: a negative size, a null pointer, data not aligned to 16 or a misaligned table, workspace or crc_out");
  return crc_segments_launch(ctx, data, n, table_dev, n_seg, extra, total_pieces, (uint32_t*)workspace, crc_out);
}

int rhccq_crc32_segments_host(const uint8_t* data, int64_t n, const rhccq_segment* table, int64_t n_seg, int64_t extra, uint32_t* crc_out) {
  if (n < 0 || (n > 0 && !data) || n_seg < 0 || extra < 0 || (n_seg > 0 && (!table || !crc_out))) return RHCCQ_E_ARG;
  for (int64_t i = 0; i < n_seg; ++i) {
    const int64_t len = seg_bytes(table[i].offset, table[i].length, extra, n);
    crc_out[i] = len ? crc32_serial(data + table[i].offset, len) : 0u;
  }
  return RHCCQ_OK;
}

int32_t rhccq_png_unfilter_band_rows(void) { return kUnfRows; }
int32_t rhccq_png_unfilter_tile(void) { return kUnfTile; }
int32_t rhccq_png_unfilter_granule(void) { return kUnfGranule; }
int64_t rhccq_png_unfilter_bytes(int32_t H, int64_t rowbytes, int32_t bpp) {
  return unfilter_check(H, rowbytes, bpp) ? (int64_t)RHCCQ_E_ARG : unf_work_bytes(H, rowbytes, bpp);
}

int rhccq_png_unfilter(rhccq_ctx* ctx, const uint8_t* scan, int32_t H, int64_t rowbytes, int32_t bpp, uint8_t* raw_out, void* workspace,
                       int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (unfilter_check(H, rowbytes, bpp)) return rhccq_fail(ctx, RHCCQ_E_ARG, "png_unfilter: H >= 1, rowbytes >= 1 a multiple of bpp, bpp 1, 2, 3, 4, 6 or 8, below 2 GiB");
  if (!scan || !raw_out || !workspace || !status || (uintptr_t)workspace % 4 || (uintptr_t)status % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "png_unfilter: a null pointer or a misaligned workspace or status");
  if (const int rc = unfilter_launch(ctx, scan, H, rowbytes, bpp, raw_out, (uint32_t*)workspace)) return rc;
  hipLaunchKernelGGL(unfilter_status_kernel, dim3(1), dim3(1), 0, ctx->stream, (const uint32_t*)workspace, (int)H, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_png_unfilter_host(const uint8_t* scan, int32_t H, int64_t rowbytes, int32_t bpp, uint8_t* raw_out, int32_t* status) {
  if (unfilter_check(H, rowbytes, bpp) || !scan || !raw_out || !status) return RHCCQ_E_ARG;
  const Verdict v = png_verdict(-1, RHCCQ_ZS_OK, 0, 0, unfilter_serial(scan, H, rowbytes, bpp, raw_out), H, 0u);
  status[0] = v.status;
  status[1] = v.detail;
  return RHCCQ_OK;
}

int rhccq_png_expand(rhccq_ctx* ctx, const uint8_t* raw, int32_t H, int32_t W, int32_t colour_type, int32_t depth, const uint8_t* palette,
                     int32_t K, const uint8_t* trns, int32_t trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!raw || !rgb || expand_check(H, W, colour_type, depth, palette, K, trns, trns_bytes))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "png_expand: H, W >= 1, a colour type and depth PNG allows, a palette of 1..256 rows for colour type 3, tRNS of 0..256 bytes");
  return expand_launch(ctx, raw, H, W, colour_type, depth, palette, K, trns, trns_bytes, rgb, alpha, idx);
}

int rhccq_png_expand_host(const uint8_t* raw, int32_t H, int32_t W, int32_t colour_type, int32_t depth, const uint8_t* palette, int32_t K,
                          const uint8_t* trns, int32_t trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  if (!raw || !rgb || expand_check(H, W, colour_type, depth, palette, K, trns, trns_bytes)) return RHCCQ_E_ARG;
  expand_serial(raw, H, W, colour_type, depth, palette, K, trns, trns_bytes, rgb, alpha, idx);
  return RHCCQ_OK;
}

int rhccq_png_join(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_segment* idat_dev, int32_t n_idat, int64_t total, uint8_t* stream) {
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || n_idat < 0 || total < 0 || total > n || (total > 0 && (!file || !idat_dev || !stream || n_idat < 1)) || (uintptr_t)idat_dev % 8 || (uintptr_t)stream % 16)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "png_join: a negative size, total above n, a null pointer, a misaligned table or a stream not aligned to 16");
  if (total == 0) return RHCCQ_OK;
  hipLaunchKernelGGL(idat_join_kernel, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, ctx->stream, file, (long long)n, idat_dev, (int)n_idat,
                     (long long)total, stream);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_png_read_sizes(const rhccq_png_info* info, int64_t n, int64_t* workspace_bytes) {
  if (!info || !workspace_bytes || n < 0) return RHCCQ_E_ARG;
  if (info->status != RHCCQ_PNG_OK) {
    *workspace_bytes = 256;
    return RHCCQ_OK;
  }
  if (!info_sound(*info, n)) return RHCCQ_E_ARG;
  ReadLayout l;
  if (const int rc = read_layout(*info, l)) return rc;
  *workspace_bytes = l.total;
  return RHCCQ_OK;
}

int64_t rhccq_png_read_scan_offset(const rhccq_png_info* info) {
  ReadLayout l;
  if (!info || info->status != RHCCQ_PNG_OK || read_layout(*info, l)) return RHCCQ_E_ARG;
  return l.o_scan;
}

int rhccq_png_decode(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_png_info* info, const rhccq_segment* table_dev, int32_t flags,
                     void* workspace, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!info || !status || (uintptr_t)status % 4 || (flags & ~RHCCQ_PNG_READ_NO_CRC)) return rhccq_fail(ctx, RHCCQ_E_ARG, "png_decode: a null info or status, or unknown flag bits");
  if (info->status != RHCCQ_PNG_OK) {                                // decided on the host: no device work but the status itself
    hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(1), 0, ctx->stream, info->status, info->detail, status);
    RHCCQ_LAUNCH_CHECK(ctx);
    return RHCCQ_OK;
  }
  const rhccq_png_info& f = *info;
  if (n < 0 || !file || !table_dev || !workspace || !rgb || (uintptr_t)file % 16 || (uintptr_t)table_dev % 8 || (uintptr_t)workspace % 256)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "png_decode: a null pointer, a file not aligned to 16, a misaligned table or a workspace not aligned to 256");
  if (!info_sound(f, n)) return rhccq_fail(ctx, RHCCQ_E_ARG, "png_decode: info does not describe a file of n bytes (it is rhccq_png_parse_host's)");
  ReadLayout l;
  if (const int rc = read_layout(f, l)) return rhccq_fail(ctx, rc, "png_decode: the inflater refuses the stream's size");
  uint8_t* ws = (uint8_t*)workspace;
  int64_t* zlen = (int64_t*)(ws + l.o_head);
  int32_t* zs = (int32_t*)(ws + l.o_head + 8);
  uint32_t* crcs = (uint32_t*)(ws + l.o_crc);
  uint8_t* stream = ws + l.o_stream;
  uint8_t* scan = ws + l.o_scan;
  uint8_t* raw = ws + l.o_raw;
  uint32_t* unf = (uint32_t*)(ws + l.o_unf);
  const bool check = !(flags & RHCCQ_PNG_READ_NO_CRC);
  if (check)
    if (const int rc = crc_segments_launch(ctx, file, n, table_dev, f.n_chunks, 4, f.crc_pieces, (uint32_t*)(ws + l.o_part), crcs)) return rc;
  if (const int rc = rhccq_png_join(ctx, file, n, table_dev + f.first_idat, f.n_idat, f.idat_bytes, stream)) return rc;
  if (const int rc = rhccq_zlib_decompress(ctx, stream, f.idat_bytes, ws + l.o_inf, scan, f.scan_bytes, zlen, zs)) return rc;
  if (const int rc = unfilter_launch(ctx, scan, f.height, f.rowbytes, f.bpp, raw, unf)) return rc;
  if (const int rc = expand_launch(ctx, raw, f.height, f.width, f.colour_type, f.depth, f.colour_type == 3 ? file + f.plte_offset : nullptr, f.palette_rows,
                                   f.trns_bytes ? file + f.trns_offset : nullptr, f.trns_bytes, rgb, alpha, idx))
    return rc;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, ctx->stream, file, (long long)n, table_dev, (int)f.n_chunks, check ? (const uint32_t*)crcs : nullptr,
                     (const long long*)zlen, (const int32_t*)zs, (long long)f.scan_bytes, (const uint32_t*)unf, (int)f.height, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_png_decode_host(const uint8_t* file, int64_t n, int32_t flags, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status) {
  if (n < 0 || (n > 0 && !file) || !status || (flags & ~RHCCQ_PNG_READ_NO_CRC)) return RHCCQ_E_ARG;
  rhccq_png_info f;
  std::vector<rhccq_segment> table((size_t)(n / 12) + 1);
  const int64_t count = png_parse(file, n, &f, table.data(), (int64_t)table.size());
  status[0] = f.status;
  status[1] = f.detail;
  if (f.status != RHCCQ_PNG_OK) return RHCCQ_OK;
  if (!rgb) return RHCCQ_E_ARG;
  int64_t first_bad = -1;
  if (!(flags & RHCCQ_PNG_READ_NO_CRC))
    for (int64_t i = 0; i < count && first_bad < 0; ++i)
      if (crc32_serial(file + table[i].offset, table[i].length + 4) != get_be32(file + table[i].offset + 4 + table[i].length)) first_bad = i;
  std::vector<uint8_t> stream((size_t)f.idat_bytes + 1), scan((size_t)f.scan_bytes, 0), raw((size_t)(f.rowbytes * f.height));
  for (int64_t i = f.first_idat; i < f.first_idat + f.n_idat; ++i)
    for (int64_t j = 0; j < table[i].length; ++j) stream[(size_t)(table[i].dst + j)] = file[table[i].offset + 4 + j];
  int64_t zlen = 0;
  int32_t zs = 0;
  if (const int rc = rhccq_zlib_decompress_host(stream.data(), f.idat_bytes, scan.data(), f.scan_bytes, &zlen, &zs)) return rc;
  const int64_t bad = unfilter_serial(scan.data(), f.height, f.rowbytes, f.bpp, raw.data());
  expand_serial(raw.data(), f.height, f.width, f.colour_type, f.depth, f.colour_type == 3 ? file + f.plte_offset : nullptr, f.palette_rows,
                f.trns_bytes ? file + f.trns_offset : nullptr, f.trns_bytes, rgb, alpha, idx);
  const Verdict v = png_verdict(first_bad, zs, zlen, f.scan_bytes, bad, f.height, 0u);
  status[0] = v.status;
  status[1] = v.detail;
  return RHCCQ_OK;
}

}  // extern "C"
