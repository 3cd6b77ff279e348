// GIF files written on the device (EXTENSION, include/rhccq.h): a frame's pixels are cut into segments of kSegment pixels that each end in
// a Clear code, so every segment is an LZW problem of its own; the segments' code streams are joined bit by bit afterwards.  The definitions
// both sides share are in gif_write.h; the host forms at the end run them serially.
//
//   gif_table_kernel    the per-frame table (palette rows, delay) comes by value, 256 frames a launch, and is laid into the workspace.
//   gif_lzw_kernel      a ONE-wave workgroup per (frame, segment).  The dictionary is an open-addressed table of 8 192 32-bit slots in LDS
//                       ((prefix, pixel) -> code; 32 KiB, four workgroups a CU), or with RHCCQ_GIF_TRIE a sibling-linked trie of 4 096
//                       nodes (16 KiB, eight a CU; measured slower on a frame and on a batch).  Pixels come in tiles of
//                       1 024: every lane loads aligned 16-byte blocks of the index map (and of the frame in front under delta) for the
//                       NEXT tile before the chain walks the current one, the blocks go to LDS as loaded, and all lanes then build the
//                       tile's bytes from them (clamp, delta substitution), which also takes the misalignment of a segment's start out.
//                       The chain runs in scalar registers (all lanes in step, a slot read broadcast and made scalar, the tile's pixels
//                       held one a lane and read by lane number): one dependent LDS read a probe.  Codes leave as packed 32-bit words into
//                       the segment's slot; the segment's bit count goes beside it.  A table-full Clear makes the wave zero the dictionary.
//   gif_offsets_kernel  a workgroup per frame: the exclusive prefix sum of its segments' bit counts, the stream's byte length.
//   gif_layout_kernel   one workgroup: a prefix sum of the frames' bytes gives where each starts in the file, and the file's length.
//   gif_join_kernel     a lane per 32-bit word of a frame's stream: a binary search over the prefix finds the first segment that covers
//                       the word, a loop takes every further one (a short last segment lets more than two meet in a word); the word's bytes
//                       go to their sub-blocked positions with the length bytes and the terminator.  Gather only.
//   gif_frame_kernel    a workgroup per frame: extension, descriptor, local table, minimum code size; workgroup 0 also header, global
//                       table, loop extension, trailer and the file's length.
#include "gif_write.h"
#include "palette_remap.h"

#include <algorithm>
#include <string>
#include <vector>

namespace rhccq {
namespace gif {

constexpr int kTile = 1024;                                           // pixels the chain walks between two loads
constexpr int kTableChunk = 256;                                      // frames of one gif_table_kernel launch
constexpr int64_t kFileMax = ((int64_t)1 << 31) - 1;
constexpr int64_t kSegmentsMax = (int64_t)1 << 30;                    // (frame, segment) pairs of a call: the LZW launch's grid

// a frame's table entry: palette rows - 1 in bits 0..7, the delay above
static inline uint32_t frame_entry(int k, int delay) { return (uint32_t)(k - 1) | (uint32_t)delay << 8; }
RHCCQ_GIF_HD int entry_rows(uint32_t e) { return (int)(e & 255u) + 1; }
RHCCQ_GIF_HD int entry_delay(uint32_t e) { return (int)(e >> 8); }

struct TableChunk { uint32_t e[kTableChunk]; };

__global__ __launch_bounds__(kTableChunk) void gif_table_kernel(TableChunk c, int count, uint32_t* __restrict__ ftab) {
  if ((int)threadIdx.x < count) ftab[threadIdx.x] = c.e[threadIdx.x];
}

// ---- LZW -----------------------------------------------------------------------------------------------------------------------------
// the aligned 16-byte block at `at`, or zero when none of it lies in [lo, hi).  The first and the last block of a segment may begin up to
// 15 bytes in front of lo or end up to 15 bytes behind hi, so where idx (or a frame's start) is not aligned to 16 this reads bytes
// outside the index map: never across a page (an aligned 16-byte block lies in one) and always together with a byte of the map; the
// bytes read there are not used (include/rhccq.h says so to the caller)
__device__ __forceinline__ uint4 gif_block(const uint8_t* at, const uint8_t* lo, const uint8_t* hi) {
  if (at + 16 > lo && at < hi) return *(const uint4*)at;
  return make_uint4(0u, 0u, 0u, 0u);
}

// the dictionary as the chain sees it: EVERY lane of the wave runs the chain on the same values, and a slot read is brought into a scalar
// register, so the compiler keeps the chain's state in scalar registers and its branches uniform (with one lane alone in the chain every
// step is a cascade of exec-mask saves and restores: 275 ns a pixel)
struct UniformDict {
  uint32_t* d;
  struct Slot {
    uint32_t* p;
    __device__ __forceinline__ operator uint32_t() const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)*p); }
    __device__ __forceinline__ void operator=(uint32_t v) const { *p = v; }      // (every lane stores the same word)
  };
  __device__ __forceinline__ Slot operator[](uint32_t h) const { return Slot{d + h}; }
};

template <typename T, bool TRIE>
__global__ __launch_bounds__(64) void gif_lzw_kernel(const T* __restrict__ idx, long long P, int nseg, const uint32_t* __restrict__ ftab, int flags,
                                                     uint32_t* __restrict__ words, long long slot, uint32_t* __restrict__ seg_bits) {
  constexpr int EB = sizeof(T), PPB = 16 / EB, TB = kTile / PPB;      // pixels of a block, blocks of a tile: 64 EB
  constexpr int kWords = TRIE ? kTrieNodes : kDictSlots;             // the dictionary: 16 KiB of trie nodes or 32 KiB of hash slots
  __shared__ uint32_t dict[kWords];
  __shared__ uint4 raw_cur[TB + 1], raw_prev[TB + 1];
  __shared__ uint8_t fin[kTile];
  const int lane = threadIdx.x;
  const long long f = blockIdx.x / (unsigned)nseg, s = blockIdx.x - f * nseg;
  const uint32_t K = (uint32_t)entry_rows(ftab[f]);
  const int m = gif_min_code(gif_table_bits(gif_entries((int)K, flags)));
  const bool delta = (flags & RHCCQ_GIF_DELTA) && f > 0;
  const long long p0 = s * kSegment;
  const int len = (int)(P - p0 < kSegment ? P - p0 : kSegment);
  // the segment is the pixels fp .. fp + len - 1 of the string that starts at the aligned address `base` (fp2, base2: the frame in front)
  const uint8_t* a = (const uint8_t*)(idx + f * P + p0);
  const uint8_t* a_end = a + (long long)len * EB;
  const int fp = (int)((uintptr_t)a & 15) / EB;
  const uint8_t* base = a - ((uintptr_t)a & 15);
  const uint8_t* a2 = delta ? a - P * EB : a;
  const uint8_t* a2_end = a2 + (long long)len * EB;
  const int fp2 = (int)((uintptr_t)a2 & 15) / EB;
  const uint8_t* base2 = a2 - ((uintptr_t)a2 & 15);

  uint4 cur[EB + 1], prev[EB + 1];
  auto load = [&](int t) {
#pragma unroll
    for (int j = 0; j <= EB; ++j) {
      const bool on = j < EB || lane == 0;                            // block TB of the tile: the misaligned segment's last pixels
      const long long b = (long long)t * TB + j * 64 + lane;
      cur[j] = on ? gif_block(base + 16 * b, a, a_end) : make_uint4(0u, 0u, 0u, 0u);
      prev[j] = on && delta ? gif_block(base2 + 16 * b, a2, a2_end) : make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto zero_dict = [&]() {
    uint4* d = (uint4*)dict;
    for (int i = lane; i < kWords / 4; i += 64) d[i] = make_uint4(0u, 0u, 0u, 0u);
  };

  Lzw z;
  BitSink sink;
  sink_begin(sink, words + (long long)blockIdx.x * slot, lane == 0);
  lzw_begin(z, m, s == 0, sink);
  zero_dict();
  load(0);
  const int ntiles = (len + kTile - 1) / kTile;
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();                                                  // the chain has left the tile in front
#pragma unroll
    for (int j = 0; j <= EB; ++j) {
      if (j < EB || lane == 0) {
        raw_cur[j * 64 + lane] = cur[j];
        raw_prev[j * 64 + lane] = prev[j];
      }
    }
    __syncthreads();
    const T* rc = (const T*)raw_cur;
    const T* rp = (const T*)raw_prev;
#pragma unroll
    for (int e = 0; e < kTile / 64; ++e) {
      const int i = e * 64 + lane;
      fin[i] = (uint8_t)gif_substitute((uint32_t)rc[fp + i], (uint32_t)rp[fp2 + i], K, delta);
    }
    if (t + 1 < ntiles) load(t + 1);                                  // in flight while the chain walks
    __syncthreads();
    const int cnt = len - t * kTile < kTile ? len - t * kTile : kTile;
    for (int c = 0; c < cnt; c += 64) {                               // (uniform: all lanes walk together)
      const int mine = (int)fin[c + lane];                            // 64 pixels of the tile, one a lane: the chain reads them by lane number
      const int run = cnt - c < 64 ? cnt - c : 64;
      for (int j = 0; j < run; ++j) {
        const uint32_t px = (uint32_t)__builtin_amdgcn_readlane(mine, j);
        if (TRIE ? lzw_pixel_trie(z, UniformDict{dict}, px, sink) : lzw_pixel(z, UniformDict{dict}, px, sink)) {
          __syncthreads();
          zero_dict();
          __syncthreads();
        }
      }
    }
  }
  const long long bits = lzw_finish(z, s == nseg - 1, sink);
  if (lane == 0) seg_bits[blockIdx.x] = (uint32_t)bits;
}

// ---- offsets -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_offsets_kernel(const uint32_t* __restrict__ seg_bits, int nseg, unsigned long long* __restrict__ off,
                                                          long long* __restrict__ flen) {
  __shared__ unsigned long long part[256];
  const int t = threadIdx.x;
  const long long f = blockIdx.x;
  const uint32_t* bits = seg_bits + f * nseg;
  unsigned long long* o = off + f * ((long long)nseg + 1);
  const int chunk = (nseg + 255) / 256, lo = t * chunk < nseg ? t * chunk : nseg, hi = lo + chunk < nseg ? lo + chunk : nseg;
  unsigned long long sum = 0;
  for (int i = lo; i < hi; ++i) sum += bits[i];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                                 // inclusive scan of the 256 partial sums
    const unsigned long long v = t >= d ? part[t - d] : 0ull;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  unsigned long long run = part[t] - sum;
  for (int i = lo; i < hi; ++i) {
    o[i] = run;
    run += bits[i];
  }
  if (t == 255) {
    o[nseg] = part[255];
    flen[f] = (long long)((part[255] + 7) >> 3);
  }
}

__global__ __launch_bounds__(256) void gif_layout_kernel(const uint32_t* __restrict__ ftab, const long long* __restrict__ flen, int n, int flags,
                                                         long long front, long long* __restrict__ foff, long long* __restrict__ out_len) {
  __shared__ long long part[256];
  const int t = threadIdx.x;
  const int chunk = (n + 255) / 256, lo = t * chunk < n ? t * chunk : n, hi = lo + chunk < n ? lo + chunk : n;
  auto bytes = [&](int f) { return gif_frame_front(entry_rows(ftab[f]), flags) + gif_sub_len(flen[f]); };
  long long sum = 0;
  for (int f = lo; f < hi; ++f) sum += bytes(f);
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {                                 // inclusive scan of the 256 partial sums
    const long long v = t >= d ? part[t - d] : 0ll;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  long long at = front + part[t] - sum;
  for (int f = lo; f < hi; ++f) {
    foff[f] = at;
    at += bytes(f);
  }
  if (t == 255) {
    foff[n] = front + part[255];
    *out_len = front + part[255] + 1;
  }
}

// ---- join ----------------------------------------------------------------------------------------------------------------------------
// sub = 1: frame f's bytes go to out + foff[f] + its front bytes in sub-blocks; sub = 0: as they are to out + f * stride
__global__ __launch_bounds__(256) void gif_join_kernel(const uint32_t* __restrict__ words, long long slot, const uint32_t* __restrict__ seg_bits,
                                                       const unsigned long long* __restrict__ off, const long long* __restrict__ flen, int nseg,
                                                       unsigned bpf, const uint32_t* __restrict__ ftab, int flags, const long long* __restrict__ foff,
                                                       int sub, long long stride, uint8_t* __restrict__ out) {
  const long long f = blockIdx.x / bpf;
  const unsigned bx = blockIdx.x - (unsigned)f * bpf;
  const unsigned long long* o = off + f * ((long long)nseg + 1);
  const long long L = flen[f], nw = (L + 3) >> 2;
  uint8_t* dst = sub ? out + foff[f] + gif_frame_front(entry_rows(ftab[f]), flags) : out + f * stride;
  for (long long w = (long long)bx * 256 + threadIdx.x; w < nw; w += (long long)bpf * 256) {
    const unsigned long long bit0 = 32ull * (unsigned long long)w;
    int lo = 0, hi = nseg - 1;                                        // the last segment that starts at or before bit0
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (o[mid] <= bit0) lo = mid; else hi = mid - 1;
    }
    uint32_t word = 0;
    for (int s = lo; s < nseg && o[s] < bit0 + 32; ++s) {
      const uint32_t* sw = words + (f * nseg + s) * slot;
      const long long bits = seg_bits[f * nseg + s];
      if (o[s] <= bit0) word |= gif_bits_at(sw, bits, (long long)(bit0 - o[s]));
      else word |= gif_bits_at(sw, bits, 0) << (int)(o[s] - bit0);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long b = 4 * w + j;
      if (b >= L) break;
      const uint8_t v = (uint8_t)(word >> (8 * j));
      if (!sub) {
        dst[b] = v;
        continue;
      }
      const long long p = gif_sub_pos(b);
      dst[p] = v;
      if (b % 255 == 0) dst[p - 1] = (uint8_t)(L - b < 255 ? L - b : 255);
      if (b == L - 1) dst[p + 1] = 0;
    }
  }
}

// ---- framing -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gif_frame_kernel(const uint8_t* __restrict__ pal, int k_stride, const uint32_t* __restrict__ ftab, int n, int H, int W,
                                                        int flags, int loop, const long long* __restrict__ foff, uint8_t* __restrict__ out) {
  const int f = blockIdx.x, t = threadIdx.x;
  const uint32_t e = ftab[f];
  const int k = entry_rows(e);
  const bool local = flags & RHCCQ_GIF_LOCAL;
  uint8_t* p = out + foff[f];
  if (t == 0) gif_put_frame_head(p, W, H, k, flags, entry_delay(e), (flags & RHCCQ_GIF_DELTA) && f > 0);
  if (local && t < (1 << gif_table_bits(k))) gif_put_entry(p + kFrameHeadBytes, pal + 3ll * f * k_stride, k, t);
  if (f) return;
  if (t == 0) {
    gif_put_head(out, W, H, n, k, flags, loop);
    out[foff[n]] = 0x3B;
  }
  if (!local && t < (1 << gif_table_bits(gif_entries(k, flags)))) gif_put_entry(out + kHeadBytes, pal, k, t);
}

// ---- arguments -----------------------------------------------------------------------------------------------------------------------
struct Sizes {
  int64_t P, nseg, slot, stream, o_ftab, o_flen, o_foff, o_bits, o_off, o_words, work, bound;
};

static int gif_shape(rhccq_ctx* ctx, const char* fn, int n, int H, int W, int flags, Sizes& s) {
  static thread_local std::string msg;
  auto fail = [&](int code, const char* what) {
    msg = std::string(fn) + ": " + what;
    return rhccq_fail(ctx, code, msg.c_str());
  };
  if (n < 1 || n > kMaxFrames) return fail(RHCCQ_E_ARG, "n_frames must be 1..2^20");
  if (H < 1 || W < 1 || H > 65535 || W > 65535) return fail(RHCCQ_E_ARG, "H and W must be 1..65535");
  if (flags & ~kFlagsAll) return fail(RHCCQ_E_ARG, "unknown flag bits");
  if ((flags & RHCCQ_GIF_LOCAL) && (flags & RHCCQ_GIF_DELTA)) return fail(RHCCQ_E_ARG, "delta needs a global table");
  s.P = (int64_t)H * W;
  s.nseg = gif_segments(s.P);
  s.slot = gif_slot_words(s.P);
  s.stream = gif_stream_bound(s.P);
  if (n * s.nseg > kSegmentsMax) return fail(RHCCQ_E_LIMIT, "more than 2^30 segments");
  const int64_t frame = kFrameHeadBytes + 768 + 1 + gif_sub_len(s.stream);
  if (frame > kFileMax / n) return fail(RHCCQ_E_LIMIT, "a file of 2 GiB or more");
  s.bound = kHeadBytes + 768 + kLoopBytes + n * frame + 1;
  if (s.bound > kFileMax) return fail(RHCCQ_E_LIMIT, "a file of 2 GiB or more");
  s.o_flen = 0;                                                       // (the entries' callers read the lengths there)
  s.o_ftab = align256(s.o_flen + 8 * (int64_t)n);
  s.o_foff = align256(s.o_ftab + 4 * (int64_t)n);
  s.o_bits = align256(s.o_foff + 8 * ((int64_t)n + 1));
  s.o_off = align256(s.o_bits + 4 * n * s.nseg);
  s.o_words = align256(s.o_off + 8 * n * (s.nseg + 1));
  s.work = s.o_words + 4 * n * s.nseg * s.slot;
  return 0;
}

// idx, the rows per table (one, or n with local tables) and the flags against the definition
static int gif_check(rhccq_ctx* ctx, const char* fn, const void* idx, int eb, int n, const int32_t* k_rows, int flags) {
  static thread_local std::string msg;
  auto fail = [&](const char* what) {
    msg = std::string(fn) + ": " + what;
    return rhccq_fail(ctx, RHCCQ_E_ARG, msg.c_str());
  };
  if (!idx || !k_rows) return fail("a null idx or k_rows");
  if (eb != 1 && eb != 2 && eb != 4) return fail("idx_elem_bytes must be 1, 2 or 4");
  if ((uintptr_t)idx % (unsigned)eb) return fail("idx is not aligned to its element");
  const int tables = flags & RHCCQ_GIF_LOCAL ? n : 1;
  for (int i = 0; i < tables; ++i)
    if (k_rows[i] < 1 || k_rows[i] > kMaxRows) return fail("a table must have 1..256 rows");
  if ((flags & RHCCQ_GIF_DELTA) && k_rows[0] > kMaxRows - 1) return fail("delta needs a table of at most 255 rows");
  return 0;
}
static int gif_times(rhccq_ctx* ctx, const char* fn, int n, const int32_t* delays, int loop) {
  static thread_local std::string msg;
  auto fail = [&](const char* what) {
    msg = std::string(fn) + ": " + what;
    return rhccq_fail(ctx, RHCCQ_E_ARG, msg.c_str());
  };
  if (!delays) return fail("a null delays");
  for (int i = 0; i < n; ++i)
    if (delays[i] < 0 || delays[i] > 65535) return fail("a delay must be 0..65535");
  if (loop < 0 || loop > 65535) return fail("loop must be 0..65535");
  return 0;
}
static inline int rows_of(const int32_t* k_rows, int flags, int f) { return k_rows[flags & RHCCQ_GIF_LOCAL ? f : 0]; }

// the launches both device entries share: table, LZW, offsets
static int lzw_launch(rhccq_ctx* ctx, const void* idx, int eb, int n, const Sizes& s, const int32_t* k_rows, const int32_t* delays, int flags, uint8_t* ws) {
  uint32_t* ftab = (uint32_t*)(ws + s.o_ftab);
  for (int f0 = 0; f0 < n; f0 += kTableChunk) {
    TableChunk c{};
    const int count = n - f0 < kTableChunk ? n - f0 : kTableChunk;
    for (int i = 0; i < count; ++i) c.e[i] = frame_entry(rows_of(k_rows, flags, f0 + i), delays ? delays[f0 + i] : 0);
    hipLaunchKernelGGL(gif_table_kernel, dim3(1), dim3(kTableChunk), 0, ctx->stream, c, count, ftab + f0);
  }
  index_dispatch(eb, [&](auto* t) {
    using T = std::remove_pointer_t<decltype(t)>;
    if (flags & RHCCQ_GIF_TRIE)
      hipLaunchKernelGGL((gif_lzw_kernel<T, true>), dim3((unsigned)(n * s.nseg)), dim3(64), 0, ctx->stream, (const T*)idx, (long long)s.P, (int)s.nseg,
                         (const uint32_t*)ftab, flags, (uint32_t*)(ws + s.o_words), (long long)s.slot, (uint32_t*)(ws + s.o_bits));
    else
      hipLaunchKernelGGL((gif_lzw_kernel<T, false>), dim3((unsigned)(n * s.nseg)), dim3(64), 0, ctx->stream, (const T*)idx, (long long)s.P, (int)s.nseg,
                         (const uint32_t*)ftab, flags, (uint32_t*)(ws + s.o_words), (long long)s.slot, (uint32_t*)(ws + s.o_bits));
  });
  hipLaunchKernelGGL(gif_offsets_kernel, dim3((unsigned)n), dim3(256), 0, ctx->stream, (const uint32_t*)(ws + s.o_bits), (int)s.nseg,
                     (unsigned long long*)(ws + s.o_off), (long long*)(ws + s.o_flen));
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}
static int join_launch(rhccq_ctx* ctx, int n, const Sizes& s, int flags, uint8_t* ws, int sub, int64_t stride, uint8_t* out) {
  const int64_t want = ((s.stream + 3) / 4 + 255) / 256, most = kSegmentsMax / n;
  const unsigned bpf = (unsigned)(want < most ? want : most);
  hipLaunchKernelGGL(gif_join_kernel, dim3((unsigned)n * bpf), dim3(256), 0, ctx->stream, (const uint32_t*)(ws + s.o_words), (long long)s.slot,
                     (const uint32_t*)(ws + s.o_bits), (const unsigned long long*)(ws + s.o_off), (const long long*)(ws + s.o_flen), (int)s.nseg, bpf,
                     (const uint32_t*)(ws + s.o_ftab), flags, (const long long*)(ws + s.o_foff), sub, (long long)stride, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

// ---- host forms ----------------------------------------------------------------------------------------------------------------------
// frame f's code stream appended to `stream` (bytes)
template <typename T>
static void lzw_frame_host(const T* idx, int64_t P, int f, int K, int flags, std::vector<uint8_t>& stream) {
  const int m = gif_min_code(gif_table_bits(gif_entries(K, flags)));
  const bool delta = (flags & RHCCQ_GIF_DELTA) && f > 0;
  const int64_t nseg = gif_segments(P);
  const bool trie = flags & RHCCQ_GIF_TRIE;
  std::vector<uint32_t> dict(trie ? kTrieNodes : kDictSlots), words((size_t)gif_slot_words(P));
  uint64_t acc = 0;
  int fill = 0;
  stream.clear();
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t p0 = s * kSegment, len = P - p0 < kSegment ? P - p0 : kSegment;
    std::fill(dict.begin(), dict.end(), 0u);
    Lzw z;
    BitSink sink;
    sink_begin(sink, words.data());
    lzw_begin(z, m, s == 0, sink);
    const T* cur = idx + (int64_t)f * P + p0;
    for (int64_t i = 0; i < len; ++i) {
      const uint32_t px = gif_substitute((uint32_t)cur[i], delta ? (uint32_t)cur[i - P] : 0u, (uint32_t)K, delta);
      if (trie ? lzw_pixel_trie(z, dict.data(), px, sink) : lzw_pixel(z, dict.data(), px, sink)) std::fill(dict.begin(), dict.end(), 0u);
    }
    const int64_t bits = lzw_finish(z, s == nseg - 1, sink);
    for (int64_t r = 0; r < bits; r += 32) {                          // the join, serially
      const int take = (int)(bits - r < 32 ? bits - r : 32);
      acc |= (uint64_t)gif_bits_at(words.data(), bits, r) << fill;
      fill += take;
      while (fill >= 8) {
        stream.push_back((uint8_t)acc);
        acc >>= 8;
        fill -= 8;
      }
    }
  }
  if (fill) stream.push_back((uint8_t)acc);
}

}  // namespace gif
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::gif;

extern "C" {

int32_t rhccq_gif_segment_pixels(void) { return kSegment; }

int rhccq_gif_sizes(int32_t n_frames, int32_t H, int32_t W, int32_t flags, int64_t* workspace_bytes, int64_t* stream_bound, int64_t* out_bound) {
  Sizes s;
  if (const int rc = gif_shape(nullptr, "gif_sizes", n_frames, H, W, flags, s)) return rc;
  if (workspace_bytes) *workspace_bytes = s.work;
  if (stream_bound) *stream_bound = s.stream;
  if (out_bound) *out_bound = s.bound;
  return RHCCQ_OK;
}

int rhccq_gif_lzw(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const int32_t* k_rows, int32_t flags,
                  void* workspace, uint8_t* streams, int64_t stream_stride, int64_t* stream_bytes) {
  if (!ctx) return RHCCQ_E_ARG;
  Sizes s;
  if (const int rc = gif_shape(ctx, "gif_lzw", n_frames, H, W, flags, s)) return rc;
  if (const int rc = gif_check(ctx, "gif_lzw", idx, idx_elem_bytes, n_frames, k_rows, flags)) return rc;
  if (!workspace || !streams || !stream_bytes || (uintptr_t)workspace % 256 || (uintptr_t)stream_bytes % 8)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_lzw: a null workspace, streams or stream_bytes, a workspace not aligned to 256 or a misaligned stream_bytes");
  if (stream_stride < s.stream) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "gif_lzw: stream_stride below the stream bound of rhccq_gif_sizes");
  uint8_t* ws = (uint8_t*)workspace;
  if (const int rc = lzw_launch(ctx, idx, idx_elem_bytes, n_frames, s, k_rows, nullptr, flags, ws)) return rc;
  if (const int rc = join_launch(ctx, n_frames, s, flags, ws, 0, stream_stride, streams)) return rc;
  RHCCQ_HIP(ctx, hipMemcpyAsync(stream_bytes, ws + s.o_flen, 8 * (size_t)n_frames, hipMemcpyDeviceToDevice, ctx->stream));
  return RHCCQ_OK;
}

int rhccq_gif_encode(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const uint8_t* palettes,
                     int32_t k_stride, const int32_t* k_rows, const int32_t* delays, int32_t loop, int32_t flags, void* workspace, uint8_t* out,
                     int64_t out_cap, int64_t* out_len) {
  if (!ctx) return RHCCQ_E_ARG;
  Sizes s;
  if (const int rc = gif_shape(ctx, "gif_encode", n_frames, H, W, flags, s)) return rc;
  if (const int rc = gif_check(ctx, "gif_encode", idx, idx_elem_bytes, n_frames, k_rows, flags)) return rc;
  if (const int rc = gif_times(ctx, "gif_encode", n_frames, delays, loop)) return rc;
  if (!palettes || k_stride < 1 || k_stride > kMaxRows) return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_encode: a null palettes or a k_stride outside 1..256");
  for (int f = 0; f < (flags & RHCCQ_GIF_LOCAL ? n_frames : 1); ++f)
    if (k_rows[f] > k_stride) return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_encode: a table of more rows than k_stride");
  if (!workspace || !out || !out_len || (uintptr_t)workspace % 256 || (uintptr_t)out_len % 8)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "gif_encode: a null workspace, out or out_len, a workspace not aligned to 256 or a misaligned out_len");
  if (out_cap < s.bound) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "gif_encode: out_cap below the bound of rhccq_gif_sizes");
  uint8_t* ws = (uint8_t*)workspace;
  if (const int rc = lzw_launch(ctx, idx, idx_elem_bytes, n_frames, s, k_rows, delays, flags, ws)) return rc;
  hipLaunchKernelGGL(gif_layout_kernel, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t*)(ws + s.o_ftab), (const long long*)(ws + s.o_flen), (int)n_frames,
                     (int)flags, (long long)gif_front_bytes(n_frames, k_rows[0], flags), (long long*)(ws + s.o_foff), (long long*)out_len);
  hipLaunchKernelGGL(gif_frame_kernel, dim3((unsigned)n_frames), dim3(256), 0, ctx->stream, palettes, (int)k_stride, (const uint32_t*)(ws + s.o_ftab),
                     (int)n_frames, (int)H, (int)W, (int)flags, (int)loop, (const long long*)(ws + s.o_foff), out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return join_launch(ctx, n_frames, s, flags, ws, 1, 0, out);
}

int rhccq_gif_lzw_host(const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const int32_t* k_rows, int32_t flags,
                       uint8_t* streams, int64_t stream_stride, int64_t* stream_bytes) {
  Sizes s;
  if (const int rc = gif_shape(nullptr, "gif_lzw", n_frames, H, W, flags, s)) return rc;
  if (const int rc = gif_check(nullptr, "gif_lzw", idx, idx_elem_bytes, n_frames, k_rows, flags)) return rc;
  if (!streams || !stream_bytes) return RHCCQ_E_ARG;
  if (stream_stride < s.stream) return RHCCQ_E_LIMIT;
  std::vector<uint8_t> stream;
  for (int f = 0; f < n_frames; ++f) {
    index_dispatch(idx_elem_bytes, [&](auto* t) { lzw_frame_host((decltype(t))idx, s.P, f, rows_of(k_rows, flags, f), flags, stream); });
    std::copy(stream.begin(), stream.end(), streams + (int64_t)f * stream_stride);
    stream_bytes[f] = (int64_t)stream.size();
  }
  return RHCCQ_OK;
}

int rhccq_gif_encode_host(const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const uint8_t* palettes, int32_t k_stride,
                          const int32_t* k_rows, const int32_t* delays, int32_t loop, int32_t flags, uint8_t* out, int64_t out_cap, int64_t* out_len,
                          int64_t* stream_bytes) {
  Sizes s;
  if (const int rc = gif_shape(nullptr, "gif_encode", n_frames, H, W, flags, s)) return rc;
  if (const int rc = gif_check(nullptr, "gif_encode", idx, idx_elem_bytes, n_frames, k_rows, flags)) return rc;
  if (const int rc = gif_times(nullptr, "gif_encode", n_frames, delays, loop)) return rc;
  if (!palettes || k_stride < 1 || k_stride > kMaxRows || !out || !out_len) return RHCCQ_E_ARG;
  for (int f = 0; f < (flags & RHCCQ_GIF_LOCAL ? n_frames : 1); ++f)
    if (k_rows[f] > k_stride) return RHCCQ_E_ARG;
  if (out_cap < s.bound) return RHCCQ_E_LIMIT;
  const bool local = flags & RHCCQ_GIF_LOCAL;
  gif_put_head(out, W, H, n_frames, k_rows[0], flags, loop);
  if (!local)
    for (int e = 0; e < 1 << gif_table_bits(gif_entries(k_rows[0], flags)); ++e) gif_put_entry(out + kHeadBytes, palettes, k_rows[0], e);
  uint8_t* p = out + gif_front_bytes(n_frames, k_rows[0], flags);
  std::vector<uint8_t> stream;
  for (int f = 0; f < n_frames; ++f) {
    const int k = rows_of(k_rows, flags, f);
    gif_put_frame_head(p, W, H, k, flags, delays[f], (flags & RHCCQ_GIF_DELTA) && f > 0);
    if (local)
      for (int e = 0; e < 1 << gif_table_bits(k); ++e) gif_put_entry(p + kFrameHeadBytes, palettes + 3ll * f * k_stride, k, e);
    p += gif_frame_front(k, flags);
    index_dispatch(idx_elem_bytes, [&](auto* t) { lzw_frame_host((decltype(t))idx, s.P, f, k, flags, stream); });
    const int64_t L = (int64_t)stream.size();
    for (int64_t b = 0; b < L; ++b) {
      if (b % 255 == 0) p[gif_sub_pos(b) - 1] = (uint8_t)(L - b < 255 ? L - b : 255);
      p[gif_sub_pos(b)] = stream[(size_t)b];
    }
    p += gif_sub_len(L);
    p[-1] = 0;
    if (stream_bytes) stream_bytes[f] = L;
  }
  *p++ = 0x3B;
  *out_len = p - out;
  return RHCCQ_OK;
}

}  // extern "C"
