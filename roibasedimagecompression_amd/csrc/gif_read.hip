// GIF files read on the device (EXTENSION, include/rhccq.h): the sub-block join, the Clear-to-Clear parallel LZW decode and the
// composition.  The definitions both sides share are in gif_read.h; the host forms at the end run them serially.
//
//   join_kernel      one launch over the joined streams of all frames: a lane builds 16 bytes; it finds the sub-block of its first byte by
//                    a search over the rows' dst column and walks on from there.  Bytes no sub-block covers (the gaps between two frames'
//                    streams) are zero.
//   scan_kernel      a workgroup a frame.  Behind a Clear the width of code j depends on j alone, so lane t of a step reads code j0 + t at
//                    its closed-form offset (four tiles of codes a step, a lane one code of each) and tests it for Clear, End and the end
//                    of the bits; the lowest hit closes the segment.  Serial from segment to segment and from step to step, nothing else.
//                    Every step ends a segment or moves kScanStep codes on, and every segment takes m + 1 bits or more, so the stream's
//                    bit length bounds both loops.
//   plan_kernel      one workgroup: exclusive prefix sums of the frames' segment counts -> the work list's frame boundaries.
//   segments_kernel<false> ("lengths")  workgroups take (frame, segment) items off the work list, strided.  seg_build makes the dictionary in LDS; the codes'
//                    lengths are summed into the segment's row.
//   offsets_kernel   a workgroup a frame: the rows' totals become the pixels in front of each (saturating), the frame's count, BAD_LENGTH.
//   segments_kernel<true> ("emit")  as lengths, then a tile of codes a step: an exclusive scan of len[code j] places every string, and each lane writes
//                    its own backwards along the prefix links.  Every store is tested against the frame's w x h.
//   compose_kernel   a thread a screen pixel, the frames in order.
//   finish_kernel    the two fault words -> status[2].
//
// seg_build.  Code j >= 1 creates entry e = clear + 1 + j with prefix = code j - 1, so the prefix links are known once the codes are
// loaded: anc[e] = code j - 1, dist[e] = 1, and for a literal anc = itself, dist = 0.  Twelve rounds of anc[e] = anc[anc[e]], dist[e] +=
// dist[anc[e]] (pointer doubling; a chain is at most 4 094 deep) leave first[e] in anc[e] and len[e] - 1 in dist[e]; a literal absorbs
// every further jump, so no round tests anything.  suffix[e] = first[code j]: for the KwKwK code j == e that is first[e] itself, which the
// chain has given by then.  RHCCQ_OPT_GIF_READ_CHAIN = 1 resolves the chains by one lane's pass over e in order instead (an entry's prefix
// lies below it): up to 4 094 dependent LDS round trips against 12 rounds of 16 entries a lane.  It lost the measurement
// and is kept for it.
#include "gif_read.h"
#include "rhccq_common.h"

#include <vector>

namespace rhccq {
namespace gifr {

// ---- join ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void join_kernel(const uint8_t* __restrict__ file, long long n, const rhccq_segment* __restrict__ table, long long count,
                                                   long long total, uint8_t* __restrict__ stream) {
  const long long p0 = ((long long)blockIdx.x * 256 + threadIdx.x) * 16;
  if (p0 >= total) return;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if (count > 0) {
    long long lo = 0, hi = count;                                    // the last row whose dst is <= p0
    while (hi - lo > 1) {
      const long long mid = (lo + hi) >> 1;
      if (table[mid].dst <= p0) lo = mid; else hi = mid;
    }
    long long c = lo;
    rhccq_segment seg = table[c];
    long long next = c + 1 < count ? table[c + 1].dst : total;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const long long p = p0 + j;
      while (c + 1 < count && next <= p) {
        seg = table[++c];
        next = c + 1 < count ? table[c + 1].dst : total;
      }
      const long long off = p - seg.dst, src = seg.offset + off;
      const uint32_t v = off >= 0 && off < seg.length && src >= 0 && src < n ? file[src] : 0u;
      w[j >> 2] |= v << (8 * (j & 3));
    }
  }
  *(uint4*)(stream + p0) = make_uint4(w[0], w[1], w[2], w[3]);
}

// ---- scan ----------------------------------------------------------------------------------------------------------------------------
struct Totals { long long stream, pixels, rows; };
constexpr int kScanCodes = 4;                                        // codes a lane tests a step: a step of the scan is kScanCodes tiles
constexpr int kScanStep = kScanCodes * kTile;

__global__ __launch_bounds__(kThreads) void scan_kernel(const uint8_t* __restrict__ streams, const rhccq_gif_frame* __restrict__ frames, Totals tot,
                                                        SegRow* __restrict__ rows, uint32_t* __restrict__ n_seg) {
  __shared__ int s_hit;
  __shared__ long long s_next;
  __shared__ int s_last;
  const int f = blockIdx.x, tid = threadIdx.x;
  const rhccq_gif_frame fr = frames[f];
  if (!frame_lzw_sound(fr, tot.stream, tot.pixels, tot.rows)) {      // (uniform)
    if (tid == 0) n_seg[f] = 0u;
    return;
  }
  const uint8_t* s = streams + fr.stream_offset;
  const long long bits = 8 * fr.stream_bytes, cap = seg_bound(fr.stream_bytes, fr.m);
  const uint32_t clear = 1u << fr.m;
  SegRow* out = rows + fr.first_row;
  long long s0 = 0, count = 0;
  while (s0 < bits) {                                                // (uniform) a segment a turn
    long long j0 = 0, jh = 0;
    for (;;) {                                                       // kScanCodes tiles of codes a turn
      int mine = kScanStep, mine_last = 0;                           // the lane's first hit: its place in the step
      long long mine_next = 0;
#pragma unroll
      for (int k = 0; k < kScanCodes; ++k) {
        const long long j = j0 + k * kTile + tid, off = s0 + code_bits(fr.m, j);
        const int w = code_width(fr.m, j);
        const bool past = off + w > bits;
        const uint32_t c = code_at(s, past ? 0 : off, w);            // (no branch around the loads: the four codes' bytes are in flight together)
        if (mine == kScanStep && (past || c == clear || c == clear + 1)) {
          mine = k * kTile + tid;
          mine_next = off + w;
          mine_last = past || c == clear + 1;
        }
      }
      if (tid == 0) s_hit = kScanStep;
      __syncthreads();
      if (mine < kScanStep) atomicMin(&s_hit, mine);
      __syncthreads();
      const int h = s_hit;
      if (h == mine && h < kScanStep) {
        s_next = mine_next;
        s_last = mine_last;
      }
      __syncthreads();                                               // (s_hit is written again only behind this)
      if (h < kScanStep) {
        jh = j0 + h;
        break;
      }
      j0 += kScanStep;
    }
    if (jh > 0 && count < cap) {
      if (tid == 0) out[count] = SegRow{s0, (uint32_t)jh, 0u};
      ++count;
    }
    if (s_last) break;
    s0 = s_next;
  }
  if (tid == 0) n_seg[f] = (uint32_t)count;
}

// ---- block-wide sums -----------------------------------------------------------------------------------------------------------------
// inclusive prefix sums over the workgroup's kThreads lanes; s_w: kThreads / 64 words
__device__ __forceinline__ unsigned long long block_scan(unsigned long long v, unsigned long long* s_w) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long t = __shfl_up(v, d, 64);
    if (lane >= d) v += t;
  }
  __syncthreads();                                                   // (the words' last readers are done)
  if (lane == 63) s_w[wave] = v;
  __syncthreads();
  unsigned long long add = 0;
  for (int i = 0; i < wave; ++i) add += s_w[i];
  return v + add;
}
__device__ __forceinline__ unsigned long long block_total(const unsigned long long* s_w) {
  unsigned long long t = 0;
  for (int i = 0; i < kThreads / 64; ++i) t += s_w[i];
  return t;
}

__global__ __launch_bounds__(kThreads) void plan_kernel(const uint32_t* __restrict__ n_seg, int n_frames, unsigned long long* __restrict__ seg_base,
                                                        uint32_t* __restrict__ head) {
  __shared__ unsigned long long s_w[kThreads / 64];
  unsigned long long run = 0;
  for (int f0 = 0; f0 < n_frames; f0 += kThreads) {                  // (uniform)
    const int f = f0 + threadIdx.x;
    const unsigned long long v = f < n_frames ? n_seg[f] : 0u;
    const unsigned long long incl = block_scan(v, s_w);
    if (f < n_frames) seg_base[f] = run + incl - v;
    run += block_total(s_w);
  }
  if (threadIdx.x == 0) {
    seg_base[n_frames] = run;
    head[2] = sat32(run);
    head[3] = 0u;
  }
}

// ---- a segment's dictionary ----------------------------------------------------------------------------------------------------------
struct SegLds {
  uint32_t ent[kMaxCode];                                            // prefix 12 | suffix 8 | len 12
  uint16_t anc[kMaxCode], dist[kMaxCode];
};

// -> true in the lanes that met an invalid code
__device__ __forceinline__ bool seg_build(SegLds& L, const uint8_t* __restrict__ s, long long s0, int m, long long n_codes, int in_order) {
  const int tid = threadIdx.x;
  const uint32_t clear = 1u << m;
  const long long n_tab = n_codes < table_codes(m) ? n_codes : table_codes(m);
  bool bad = false;
  __syncthreads();                                                   // (the item before is done with the arrays)
  for (int e = tid; e < kMaxCode; e += kThreads) {
    L.anc[e] = (uint16_t)e;
    L.dist[e] = 0;
    L.ent[e] = (uint32_t)e < clear ? (uint32_t)e | (uint32_t)e << 12 | 1u << 20 : 0u;
  }
  __syncthreads();
  for (long long j = 1 + tid; j < n_tab; j += kThreads) {
    const uint32_t e = clear + 1 + (uint32_t)j;
    L.anc[e] = (uint16_t)code_load(s, s0, m, j - 1, &bad);
    L.dist[e] = 1;
  }
  __syncthreads();
  if (in_order) {                                                    // (uniform) RHCCQ_OPT_GIF_READ_CHAIN = 1: an entry's prefix is below it, so it is resolved
    if (tid == 0)
      for (uint32_t e = clear + 2; e < clear + 1 + (uint32_t)n_tab; ++e) {
        const uint16_t up = L.anc[e];
        L.dist[e] = (uint16_t)(L.dist[up] + 1);
        L.anc[e] = L.anc[up];
      }
    __syncthreads();
  }
  for (int round = 0; round < (in_order ? 0 : 12); ++round) {
    uint16_t a[kMaxCode / kThreads], d[kMaxCode / kThreads];
#pragma unroll
    for (int k = 0; k < kMaxCode / kThreads; ++k) {
      const int e = tid + k * kThreads;
      const uint16_t up = L.anc[e];
      a[k] = L.anc[up];
      d[k] = (uint16_t)(L.dist[e] + L.dist[up]);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kMaxCode / kThreads; ++k) {
      const int e = tid + k * kThreads;
      L.anc[e] = a[k];
      L.dist[e] = d[k];
    }
    __syncthreads();
  }
  for (long long j = 1 + tid; j < n_tab; j += kThreads) {
    const uint32_t e = clear + 1 + (uint32_t)j;
    const uint32_t prefix = code_load(s, s0, m, j - 1, &bad), c = code_load(s, s0, m, j, &bad);
    L.ent[e] = prefix | ((uint32_t)L.anc[c] & 255u) << 12 | ((uint32_t)L.dist[e] + 1u) << 20;
  }
  __syncthreads();
  return bad;
}

// the work list's item -> its frame (the last one whose base is <= item; frames without segments share their base with the next)
__device__ __forceinline__ int item_frame(const unsigned long long* __restrict__ seg_base, int n_frames, unsigned long long item) {
  int lo = 0, hi = n_frames;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_base[mid] <= item) lo = mid; else hi = mid;
  }
  return lo;
}

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void segments_kernel(const uint8_t* __restrict__ streams, const rhccq_gif_frame* __restrict__ frames, int n_frames,
                                                            Totals tot, SegRow* __restrict__ rows, const unsigned long long* __restrict__ seg_base,
                                                            uint32_t* __restrict__ head, uint8_t* __restrict__ pixels, int in_order) {
  __shared__ SegLds L;
  __shared__ unsigned long long s_w[kThreads / 64];
  const int tid = threadIdx.x;
  const unsigned long long total = seg_base[n_frames];
  for (unsigned long long item = blockIdx.x; item < total; item += gridDim.x) {   // (uniform)
    const int f = item_frame(seg_base, n_frames, item);
    const rhccq_gif_frame fr = frames[f];
    if (!frame_lzw_sound(fr, tot.stream, tot.pixels, tot.rows)) continue;
    const long long r = (long long)(item - seg_base[f]);
    if (r >= seg_bound(fr.stream_bytes, fr.m)) continue;
    SegRow* row = rows + fr.first_row + r;
    const long long s0 = row->start_bit, n_codes = row->n_codes;
    const uint8_t* s = streams + fr.stream_offset;
    // (what the scan wrote lies inside the stream; a row that does not is skipped)
    if (s0 < 0 || n_codes < 1 || s0 + code_bits(fr.m, n_codes) > 8 * fr.stream_bytes) continue;
    bool bad = seg_build(L, s, s0, fr.m, n_codes, in_order);
    const uint32_t clear = 1u << fr.m;
    const long long wh = (long long)fr.w * fr.h, base = EMIT ? (long long)row->pixels : 0;
    uint8_t* out = pixels + fr.pixel_offset;
    unsigned long long run = 0;
    for (long long j0 = 0; j0 < n_codes; j0 += kTile) {              // (uniform)
      const long long j = j0 + tid;
      uint32_t c = 0u, len = 0u;
      if (j < n_codes) {
        c = code_load(s, s0, fr.m, j, &bad);
        len = L.ent[c] >> 20;
      }
      if (EMIT) {
        const unsigned long long incl = block_scan(len, s_w);
        if (j < n_codes && len > 0u) {
          long long p = base + (long long)(run + incl) - 1;
          for (int guard = 0; c >= clear + 2 && guard < kMaxCode; ++guard) {
            const uint32_t e = L.ent[c];
            if (p >= 0 && p < wh) out[p] = (uint8_t)(e >> 12);
            --p;
            c = e & 4095u;
          }
          if (p >= 0 && p < wh) out[p] = (uint8_t)c;
        }
        run += block_total(s_w);
      } else {
        run += len;
      }
    }
    if (!EMIT) {
      block_scan(run, s_w);
      if (tid == 0) row->pixels = sat32(block_total(s_w));
      if (bad) atomicMin(&head[0], (uint32_t)f);
    }
  }
}

__global__ __launch_bounds__(kThreads) void offsets_kernel(const rhccq_gif_frame* __restrict__ frames, Totals tot, SegRow* __restrict__ rows,
                                                           const uint32_t* __restrict__ n_seg, long long* __restrict__ counts, uint32_t* __restrict__ head) {
  __shared__ unsigned long long s_w[kThreads / 64];
  const int f = blockIdx.x, tid = threadIdx.x;
  const rhccq_gif_frame fr = frames[f];
  const bool sound = frame_lzw_sound(fr, tot.stream, tot.pixels, tot.rows);
  const long long n = sound ? (long long)n_seg[f] : 0;
  unsigned long long run = 0;
  for (long long i0 = 0; i0 < n; i0 += kThreads) {                   // (uniform)
    const long long i = i0 + tid;
    const unsigned long long v = i < n ? rows[fr.first_row + i].pixels : 0u;
    const unsigned long long incl = block_scan(v, s_w);
    if (i < n) rows[fr.first_row + i].pixels = sat32(run + incl - v);
    run += block_total(s_w);
  }
  if (tid == 0) {
    counts[f] = (long long)run;
    if (sound && run != (unsigned long long)fr.w * (unsigned long long)fr.h) atomicMin(&head[1], (uint32_t)f);
  }
}

__global__ void finish_kernel(const uint32_t* __restrict__ head, int32_t* __restrict__ status) {
  const Verdict v = gif_verdict(head[0], head[1]);
  status[0] = v.status;
  status[1] = v.detail;
}
__global__ void set_status_kernel(int32_t a, int32_t b, int32_t* __restrict__ status) {
  status[0] = a;
  status[1] = b;
}

// ---- compose -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void compose_kernel(const uint8_t* __restrict__ pixels, long long n_pixels, const uint8_t* __restrict__ file, long long n,
                                                      const rhccq_gif_frame* __restrict__ frames, int n_frames, int H, int W, uint8_t* __restrict__ rgb,
                                                      uint8_t* __restrict__ alpha, uint8_t* __restrict__ idx) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x, hw = (long long)H * W;
  if (o >= hw) return;
  const int Y = (int)(o / W), X = (int)(o - (long long)Y * W);
  Canvas cur{0, 0, 0, 0};
  for (int f = 0; f < n_frames; ++f) {
    const rhccq_gif_frame fr = frames[f];                            // (uniform: scalar loads)
    Canvas shown = cur;
    if (frame_paint_sound(fr, n, n_pixels)) {
      uint32_t index = 0;
      const long long at = compose_step(fr, file, pixels, X, Y, cur, &shown, &index);
      if (at >= 0 && idx) idx[fr.pixel_offset + at] = (uint8_t)index;
    }
    const long long q = (long long)f * hw + o;
    rgb[3 * q] = shown.r;
    rgb[3 * q + 1] = shown.g;
    rgb[3 * q + 2] = shown.b;
    if (alpha) alpha[q] = shown.covered ? 255 : 0;
  }
}

// ---- layouts and launches ------------------------------------------------------------------------------------------------------------
// rhccq_gif_unlzw's workspace: the head, the frames' segment counts, the work list's bases, the segment table
struct LzwLayout { int64_t o_nseg, o_base, o_rows, total; };
static LzwLayout lzw_layout(int64_t n_frames, int64_t seg_rows) {
  LzwLayout l;
  l.o_nseg = 256;
  l.o_base = align256(l.o_nseg + 4 * n_frames);
  l.o_rows = align256(l.o_base + 8 * (n_frames + 1));
  l.total = align256(l.o_rows + (int64_t)sizeof(SegRow) * seg_rows);
  return l;
}
// rhccq_gif_decode's: rhccq_gif_unlzw's, the counts, the joined streams, the pixel strings
struct ReadLayout { int64_t o_counts, o_stream, o_pixels, total; };
static ReadLayout read_layout(const rhccq_gif_info& f) {
  ReadLayout l;
  l.o_counts = lzw_layout(f.n_frames, f.seg_rows).total;
  l.o_stream = align256(l.o_counts + 8 * (int64_t)f.n_frames);
  l.o_pixels = align256(l.o_stream + f.stream_bytes);
  l.total = align256(l.o_pixels + f.pixels);
  return l;
}

// the host table against the sizes given; -> the rows of the segment table, negative when it does not fit
static int64_t frames_rows(const rhccq_gif_frame* frames, int64_t n_frames, int64_t stream_total, int64_t n_pixels) {
  int64_t rows = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    const rhccq_gif_frame& fr = frames[f];
    if (!frame_lzw_sound(fr, stream_total, n_pixels, kReadMax) || fr.first_row != rows) return -1;
    rows += seg_bound(fr.stream_bytes, fr.m);
    if (rows > kReadMax / (int64_t)sizeof(SegRow)) return -1;
  }
  return rows;
}

static int unlzw_launch(rhccq_ctx* ctx, const uint8_t* streams, int64_t stream_total, const rhccq_gif_frame* frames_dev, int n_frames, int64_t seg_rows,
                        void* workspace, uint8_t* pixels, int64_t n_pixels, int64_t* counts, int32_t* status) {
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  const LzwLayout l = lzw_layout(n_frames, seg_rows);
  uint8_t* ws = (uint8_t*)workspace;
  uint32_t* head = (uint32_t*)ws;
  uint32_t* n_seg = (uint32_t*)(ws + l.o_nseg);
  unsigned long long* seg_base = (unsigned long long*)(ws + l.o_base);
  SegRow* rows = (SegRow*)(ws + l.o_rows);
  const Totals tot{(long long)stream_total, (long long)n_pixels, (long long)seg_rows};
  RHCCQ_HIP(ctx, hipMemsetAsync(head, 0xFF, 8, ctx->stream));        // the two fault words: no frame
  hipLaunchKernelGGL(scan_kernel, dim3((unsigned)n_frames), dim3(kThreads), 0, ctx->stream, streams, frames_dev, tot, rows, n_seg);
  hipLaunchKernelGGL(plan_kernel, dim3(1), dim3(kThreads), 0, ctx->stream, (const uint32_t*)n_seg, n_frames, seg_base, head);
  const int64_t cap = (int64_t)ctx->compute_units * 8;
  const dim3 grid((unsigned)(seg_rows < cap ? (seg_rows < 1 ? 1 : seg_rows) : cap));
  hipLaunchKernelGGL(segments_kernel<false>, grid, dim3(kThreads), 0, ctx->stream, streams, frames_dev, n_frames, tot, rows,
                     (const unsigned long long*)seg_base, head, pixels, ctx->opt_gif_read_chain);
  hipLaunchKernelGGL(offsets_kernel, dim3((unsigned)n_frames), dim3(kThreads), 0, ctx->stream, frames_dev, tot, rows, (const uint32_t*)n_seg,
                     (long long*)counts, head);
  hipLaunchKernelGGL(segments_kernel<true>, grid, dim3(kThreads), 0, ctx->stream, streams, frames_dev, n_frames, tot, rows,
                     (const unsigned long long*)seg_base, head, pixels, ctx->opt_gif_read_chain);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(1), 0, ctx->stream, (const uint32_t*)head, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static int compose_launch(rhccq_ctx* ctx, const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames_dev,
                          int n_frames, int H, int W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  const int64_t hw = (int64_t)H * W;
  hipLaunchKernelGGL(compose_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, ctx->stream, pixels, (long long)n_pixels, file, (long long)n,
                     frames_dev, n_frames, H, W, rgb, alpha, idx);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static int join_launch(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_segment* blocks_dev, int64_t n_blocks, int64_t total, uint8_t* streams) {
  if (total == 0) return 0;
  hipLaunchKernelGGL(join_kernel, dim3((unsigned)((total + 4095) / 4096)), dim3(256), 0, ctx->stream, file, (long long)n, blocks_dev, (long long)n_blocks,
                     (long long)total, streams);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

static bool compose_args_ok(int64_t n_pixels, int64_t n, int32_t n_frames, int32_t H, int32_t W) {
  return n_pixels >= 0 && n >= 0 && n_frames >= 1 && n_frames <= kMaxFrames && H >= 1 && W >= 1 && H <= 65535 && W <= 65535;
}
static bool compose_limit_ok(int32_t n_frames, int32_t H, int32_t W) { return (int64_t)n_frames * ((int64_t)H * W) <= kReadMax / 3; }

// what rhccq_gif_decode asks of an info it did not make itself
static bool info_sound(const rhccq_gif_info& f, int64_t n) {
  if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535 || f.n_frames < 1 || f.n_frames > kMaxFrames) return false;
  if (n < 14 || n > kReadMax || f.n_blocks < 0 || f.n_blocks > n) return false;
  if (f.stream_bytes < 0 || (f.stream_bytes & 15) || f.stream_bytes > 2 * n + 32 * (int64_t)f.n_frames) return false;
  if (f.pixels < f.n_frames || f.pixels > (int64_t)f.n_frames * ((int64_t)f.width * f.height)) return false;
  if (f.seg_rows < f.n_frames || f.seg_rows > kReadMax / (int64_t)sizeof(SegRow)) return false;
  return compose_limit_ok(f.n_frames, f.height, f.width);
}

}  // namespace gifr
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::gifr;

extern "C" {

int rhccq_gif_parse_host(const uint8_t* file, int64_t n, rhccq_gif_info* info, rhccq_gif_frame* frames, int64_t frames_cap, int64_t* n_frames,
                         rhccq_segment* blocks, int64_t blocks_cap, int64_t* n_blocks) {
  if (n < 0 || (n > 0 && !file) || !info || !n_frames || !n_blocks || frames_cap < 0 || blocks_cap < 0 || (frames_cap > 0 && !frames) ||
      (blocks_cap > 0 && !blocks))
    return RHCCQ_E_ARG;
  gif_parse(file, n, info, frames, frames_cap, blocks, blocks_cap);
  *n_frames = info->n_frames;
  *n_blocks = info->n_blocks;
  return RHCCQ_OK;
}

int32_t rhccq_gif_read_tile(void) { return kTile; }
int32_t rhccq_gif_read_scan_step(void) { return kScanStep; }
int32_t rhccq_gif_read_threads(void) { return kThreads; }

int rhccq_gif_read_sizes(const rhccq_gif_info* info, int64_t n, int64_t* workspace_bytes) {
  if (!info || !workspace_bytes || n < 0) return RHCCQ_E_ARG;
  if (info->status != RHCCQ_GIFR_OK) {
    *workspace_bytes = 256;
    return RHCCQ_OK;
  }
  if (!info_sound(*info, n)) return RHCCQ_E_ARG;
  *workspace_bytes = read_layout(*info).total;
  return RHCCQ_OK;
}

int64_t rhccq_gif_unlzw_bytes(const rhccq_gif_frame* frames, int32_t n_frames) {
  if (!frames || n_frames < 1 || n_frames > kMaxFrames) return RHCCQ_E_ARG;
  const int64_t rows = frames_rows(frames, n_frames, kReadMax, kReadMax);
  return rows < 0 ? (int64_t)RHCCQ_E_ARG : lzw_layout(n_frames, rows).total;
}

int rhccq_gif_join(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_segment* blocks_dev, int64_t n_blocks, int64_t total, uint8_t* streams) {
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || n_blocks < 0 || total < 0 || (total & 15) || (total > 0 && !streams) || (n_blocks > 0 && (!file || !blocks_dev)) ||
      (uintptr_t)blocks_dev % 8 || (uintptr_t)streams % 16)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_join: a negative size, a total that is no multiple of 16, a null pointer, a misaligned table or streams not aligned to 16");
  if (n > kReadMax || n_blocks > kReadMax || total > 2 * kReadMax) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "gif_join: a size of 2^31 or more");
  return join_launch(ctx, file, n, blocks_dev, n_blocks, total, streams);
}

int rhccq_gif_unlzw(rhccq_ctx* ctx, const uint8_t* streams, int64_t stream_bytes, const rhccq_gif_frame* frames, const rhccq_gif_frame* frames_dev,
                    int32_t n_frames, void* workspace, uint8_t* pixels, int64_t n_pixels, int64_t* counts, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!streams || !frames || !frames_dev || !workspace || !pixels || !counts || !status || stream_bytes < 0 || n_pixels < 0 || n_frames < 1)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_unlzw: a null pointer, a negative size or no frame");
  if (n_frames > kMaxFrames || stream_bytes > 2 * kReadMax || n_pixels > 2 * kReadMax) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "gif_unlzw: more than 2^20 frames or a size of 2^32 or more");
  if ((uintptr_t)streams % 16 || (uintptr_t)frames_dev % 8 || (uintptr_t)workspace % 256 || (uintptr_t)counts % 8 || (uintptr_t)status % 4)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_unlzw: streams not aligned to 16, a misaligned frame table, counts or status, or a workspace not aligned to 256");
  const int64_t rows = frames_rows(frames, n_frames, stream_bytes, n_pixels);
  if (rows < 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_unlzw: the frame table does not fit stream_bytes and n_pixels (it is rhccq_gif_parse_host's)");
  return unlzw_launch(ctx, streams, stream_bytes, frames_dev, n_frames, rows, workspace, pixels, n_pixels, counts, status);
}

int rhccq_gif_compose(rhccq_ctx* ctx, const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames_dev,
                      int32_t n_frames, int32_t H, int32_t W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!pixels || !file || !frames_dev || !rgb || (uintptr_t)frames_dev % 8 || !compose_args_ok(n_pixels, n, n_frames, H, W))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_compose: a null pointer, a misaligned frame table, a negative size, no frame, or H, W outside 1..65535");
  if (!compose_limit_ok(n_frames, H, W)) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "gif_compose: images of 2^31 bytes or more");
  return compose_launch(ctx, pixels, n_pixels, file, n, frames_dev, n_frames, H, W, rgb, alpha, idx);
}

int rhccq_gif_decode(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_gif_info* info, const rhccq_gif_frame* frames,
                     const rhccq_gif_frame* frames_dev, const rhccq_segment* blocks_dev, void* workspace, uint8_t* rgb, uint8_t* alpha, uint8_t* idx,
                     int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!info || !status || (uintptr_t)status % 4) return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_decode: a null info or status");
  if (info->status != RHCCQ_GIFR_OK) {                               // decided on the host: no device work but the status itself
    hipLaunchKernelGGL(set_status_kernel, dim3(1), dim3(1), 0, ctx->stream, info->status, info->detail, status);
    RHCCQ_LAUNCH_CHECK(ctx);
    return RHCCQ_OK;
  }
  const rhccq_gif_info& f = *info;
  if (n < 0 || !file || !frames || !frames_dev || !workspace || !rgb || (f.n_blocks > 0 && !blocks_dev) ||
      (uintptr_t)frames_dev % 8 || (uintptr_t)blocks_dev % 8 || (uintptr_t)workspace % 256)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_decode: a null pointer, a misaligned table or a workspace not aligned to 256");
  if (!info_sound(f, n) || frames_rows(frames, f.n_frames, f.stream_bytes, f.pixels) != f.seg_rows)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_decode: info and frames do not describe a file of n bytes (they are rhccq_gif_parse_host's)");
  const ReadLayout l = read_layout(f);
  uint8_t* ws = (uint8_t*)workspace;
  uint8_t* streams = ws + l.o_stream;
  uint8_t* pixels = ws + l.o_pixels;
  if (const int rc = join_launch(ctx, file, n, blocks_dev, f.n_blocks, f.stream_bytes, streams)) return rc;
  if (const int rc = unlzw_launch(ctx, streams, f.stream_bytes, frames_dev, f.n_frames, f.seg_rows, ws, pixels, f.pixels, (int64_t*)(ws + l.o_counts), status))
    return rc;
  return compose_launch(ctx, pixels, f.pixels, file, n, frames_dev, f.n_frames, f.height, f.width, rgb, alpha, idx);
}

int rhccq_gif_unlzw_host(const uint8_t* streams, int64_t stream_bytes, const rhccq_gif_frame* frames, int32_t n_frames, uint8_t* pixels, int64_t n_pixels,
                         int64_t* counts, int32_t* status, int64_t* n_segments) {
  if (!streams || !frames || !pixels || !counts || !status || stream_bytes < 0 || n_pixels < 0 || n_frames < 1) return RHCCQ_E_ARG;
  if (n_frames > kMaxFrames) return RHCCQ_E_LIMIT;
  if (frames_rows(frames, n_frames, stream_bytes, n_pixels) < 0) return RHCCQ_E_ARG;
  uint32_t bc, bl;
  unlzw_serial(streams, stream_bytes, frames, n_frames, pixels, n_pixels, counts, &bc, &bl, n_segments);
  const Verdict v = gif_verdict(bc, bl);
  status[0] = v.status;
  status[1] = v.detail;
  return RHCCQ_OK;
}

int rhccq_gif_compose_host(const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames, int32_t n_frames,
                           int32_t H, int32_t W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  if (!pixels || !file || !frames || !rgb || !compose_args_ok(n_pixels, n, n_frames, H, W)) return RHCCQ_E_ARG;
  if (!compose_limit_ok(n_frames, H, W)) return RHCCQ_E_LIMIT;
  compose_serial(pixels, n_pixels, file, n, frames, n_frames, H, W, rgb, alpha, idx);
  return RHCCQ_OK;
}

int rhccq_gif_decode_host(const uint8_t* file, int64_t n, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status) {
  if (n < 0 || (n > 0 && !file) || !status) return RHCCQ_E_ARG;
  rhccq_gif_info f;
  gif_parse(file, n, &f, nullptr, 0, nullptr, 0);
  status[0] = f.status;
  status[1] = f.detail;
  if (f.status != RHCCQ_GIFR_OK) return RHCCQ_OK;
  if (!rgb) return RHCCQ_E_ARG;
  std::vector<rhccq_gif_frame> frames((size_t)f.n_frames);
  std::vector<rhccq_segment> blocks((size_t)f.n_blocks + 1);
  gif_parse(file, n, &f, frames.data(), (int64_t)frames.size(), blocks.data(), (int64_t)blocks.size());
  std::vector<uint8_t> streams((size_t)f.stream_bytes, 0), pixels((size_t)f.pixels, 0);
  for (int64_t i = 0; i < f.n_blocks; ++i)
    for (int64_t j = 0; j < blocks[i].length; ++j) streams[(size_t)(blocks[i].dst + j)] = file[blocks[i].offset + j];
  std::vector<int64_t> counts((size_t)f.n_frames);
  uint32_t bc, bl;
  unlzw_serial(streams.data(), f.stream_bytes, frames.data(), f.n_frames, pixels.data(), f.pixels, counts.data(), &bc, &bl, nullptr);
  compose_serial(pixels.data(), f.pixels, file, n, frames.data(), f.n_frames, f.height, f.width, rgb, alpha, idx);
  const Verdict v = gif_verdict(bc, bl);
  status[0] = v.status;
  status[1] = v.detail;
  return RHCCQ_OK;
}

}  // extern "C"
