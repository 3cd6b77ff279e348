// GIF writing (EXTENSION, include/rhccq.h "GIF files written on the device"): the functions the device kernels of gif_write.hip and the
// serial host twins share.  Plain C++ over <stdint.h>: a host-only program may include this file without the HIP headers.
//   geometry    gif_table_bits / gif_min_code, the bytes in front of a frame's code stream, gif_sub_pos / gif_sub_len (a stream of L bytes in
//               sub-blocks of 255), the bounds of a segment's and a frame's stream;
//   pixels      gif_clamp and gif_substitute (the delta substitution on top of the clamp);
//   LZW         one segment's state (Lzw), its output (BitSink: codes packed least significant bit first into 32-bit words) and the steps
//               lzw_begin / lzw_pixel / lzw_finish over a dictionary of kDictSlots open-addressed 32-bit slots (lzw_pixel_trie: of kTrieNodes
//               trie nodes) that the caller owns (LDS on the device, an array on the host) and clears to zero at the start and whenever
//               the step says so;
//   framing     gif_put_head / gif_put_frame_head: every byte outside the code streams.
#pragma once
#include <stdint.h>

#include "../../include/rhccq.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RHCCQ_GIF_HD __host__ __device__ __forceinline__
#else
#define RHCCQ_GIF_HD inline
#endif

namespace rhccq {
namespace gif {

constexpr int kSegment = 16384;                            // pixels of a segment (rhccq_gif_segment_pixels)
constexpr int kMaxCode = 4096;                             // codes are 12 bits at the most
constexpr int kDictSlots = 8192;                           // slots of a segment's dictionary: at most 4096 - 6 entries, so half of them stay empty
constexpr int kTrieNodes = 4096;                           // nodes of the other dictionary, a sibling-linked trie: one a code
constexpr int kFlagsAll = RHCCQ_GIF_LOCAL | RHCCQ_GIF_DELTA | RHCCQ_GIF_TRIE;
constexpr int kMaxRows = 256;
constexpr int kMaxFrames = 1 << 20;

// ---- the file's geometry -------------------------------------------------------------------------------------------------------------
// a colour table of `entries` entries has 2^tb of them
RHCCQ_GIF_HD int gif_table_bits(int entries) {
  int tb = 1;
  while ((1 << tb) < entries) ++tb;
  return tb;
}
RHCCQ_GIF_HD int gif_min_code(int tb) { return tb < 2 ? 2 : tb; }
// entries of the table that holds K rows: the transparent index counts under delta
RHCCQ_GIF_HD int gif_entries(int K, int flags) { return K + (flags & RHCCQ_GIF_DELTA ? 1 : 0); }
// where byte o of a stream stands behind the minimum code size byte, and what a stream of L bytes takes there (terminator included)
RHCCQ_GIF_HD int64_t gif_sub_pos(int64_t o) { return o + o / 255 + 1; }
RHCCQ_GIF_HD int64_t gif_sub_len(int64_t L) { return L + (L + 254) / 255 + 1; }
constexpr int kHeadBytes = 13;                             // "GIF89a" and the logical screen descriptor
constexpr int kLoopBytes = 19;                             // the NETSCAPE2.0 application extension
constexpr int kFrameHeadBytes = 8 + 10;                    // graphic control extension, image descriptor
// bytes in front of frame 0's graphic control extension
RHCCQ_GIF_HD int64_t gif_front_bytes(int n_frames, int k0, int flags) {
  return kHeadBytes + (flags & RHCCQ_GIF_LOCAL ? 0 : 3 * ((int64_t)1 << gif_table_bits(gif_entries(k0, flags)))) + (n_frames > 1 ? kLoopBytes : 0);
}
// bytes of a frame in front of its first sub-block: extension, descriptor, local table, minimum code size
RHCCQ_GIF_HD int64_t gif_frame_front(int k, int flags) {
  return kFrameHeadBytes + (flags & RHCCQ_GIF_LOCAL ? 3 * ((int64_t)1 << gif_table_bits(k)) : 0) + 1;
}
RHCCQ_GIF_HD int64_t gif_segments(int64_t pixels) { return (pixels + kSegment - 1) / kSegment; }
// no segment of `len` pixels has more bits: the opening Clear, a data code a pixel, a table-full Clear every 4096 - 258 data codes at the
// soonest, the closing code; 12 bits each
RHCCQ_GIF_HD int64_t gif_segment_bits(int64_t len) { return 12 * (len + len / (kMaxCode - 258) + 3); }
// 32-bit words of a segment's slot in the workspace
RHCCQ_GIF_HD int64_t gif_slot_words(int64_t pixels) { return (gif_segment_bits(pixels < kSegment ? pixels : kSegment) + 31) / 32 + 1; }
// no frame's stream has more bytes
RHCCQ_GIF_HD int64_t gif_stream_bound(int64_t pixels) {
  const int64_t full = pixels / kSegment, rest = pixels - full * kSegment;
  return (full * gif_segment_bits(kSegment) + (rest ? gif_segment_bits(rest) : 0) + 7) / 8;
}

// ---- pixels --------------------------------------------------------------------------------------------------------------------------
RHCCQ_GIF_HD uint32_t gif_clamp(uint32_t v, uint32_t K) { return v < K ? v : 0u; }
// the pixel written for position p of a frame: T where the frame in front shows the same (clamped) index
RHCCQ_GIF_HD uint32_t gif_substitute(uint32_t cur, uint32_t prev, uint32_t K, bool delta) {
  const uint32_t c = gif_clamp(cur, K);
  return delta && c == gif_clamp(prev, K) ? K : c;
}

// ---- LZW -----------------------------------------------------------------------------------------------------------------------------
struct BitSink {
  uint32_t* out;
  uint64_t acc;
  int fill;          // bits in acc, below 32 between calls
  int64_t words;     // words stored
  bool live;         // false: counts, but stores nothing (the lanes of a wave that run the chain beside the one that writes)
};
RHCCQ_GIF_HD void sink_begin(BitSink& s, uint32_t* out, bool live = true) {
  s.out = out;
  s.live = live;
  s.acc = 0;
  s.fill = 0;
  s.words = 0;
}
RHCCQ_GIF_HD void sink_put(BitSink& s, uint32_t code, int width) {
  s.acc |= (uint64_t)code << s.fill;
  s.fill += width;
  if (s.fill >= 32) {
    if (s.live) s.out[s.words] = (uint32_t)s.acc;
    ++s.words;
    s.acc >>= 32;
    s.fill -= 32;
  }
}
// the last partial word (zero above the stream's bits); -> the bits of the whole stream
RHCCQ_GIF_HD int64_t sink_end(BitSink& s) {
  const int64_t bits = 32 * s.words + s.fill;
  if (s.fill) {
    if (s.live) s.out[s.words] = (uint32_t)s.acc;
    ++s.words;
  }
  return bits;
}

struct Lzw {
  int m, width;
  int32_t cur;       // the current string's code, -1 in front of a segment's first pixel
  uint32_t next;
};
RHCCQ_GIF_HD void lzw_reset(Lzw& z) {
  z.next = (1u << z.m) + 2;
  z.width = z.m + 1;
}
// a segment starts: the dictionary is all zero.  opening: the frame's first segment writes the stream's opening Clear
RHCCQ_GIF_HD void lzw_begin(Lzw& z, int m, bool opening, BitSink& s) {
  z.m = m;
  z.cur = -1;
  lzw_reset(z);
  if (opening) sink_put(s, 1u << m, m + 1);
}
// what follows every data code: entry `next` is consumed, the width rule, next += 1
RHCCQ_GIF_HD void lzw_count(Lzw& z) {
  if (z.next == (1u << z.width) && z.width < 12) ++z.width;
  ++z.next;
}
// behind a data code that px forced out: the count, px opens the next string, and the table-full Clear (px follows) -> true with it
RHCCQ_GIF_HD bool lzw_after_code(Lzw& z, uint32_t px, BitSink& s) {
  lzw_count(z);
  z.cur = (int32_t)px;
  if (z.next == (uint32_t)kMaxCode) {
    sink_put(s, 1u << z.m, z.width);
    lzw_reset(z);
    return true;
  }
  return false;
}
RHCCQ_GIF_HD uint32_t lzw_hash(uint32_t key) { return (key * 0x9E3779B1u) >> 19; }   // 13 bits: kDictSlots
// a slot holds (prefix << 8 | pixel) << 12 | code; no entry's code is 0, so 0 is the empty slot
// -> true when the table-full Clear went out: the caller zeroes the dictionary before the next call
template <typename Dict>
RHCCQ_GIF_HD bool lzw_pixel(Lzw& z, Dict dict, uint32_t px, BitSink& s) {
  if (z.cur < 0) {
    z.cur = (int32_t)px;
    return false;
  }
  const uint32_t key = (uint32_t)z.cur << 8 | px;
  uint32_t h = lzw_hash(key);
  for (int probe = 0; probe < kDictSlots; ++probe) {       // (bounded: an empty slot is met long before)
    const uint32_t slot = dict[h];
    if (slot == 0u) break;
    if (slot >> 12 == key) {
      z.cur = (int32_t)(slot & 4095u);
      return false;
    }
    h = (h + 1) & (kDictSlots - 1);
  }
  sink_put(s, (uint32_t)z.cur, z.width);
  if (z.next < (uint32_t)kMaxCode) dict[h] = key << 12 | z.next;
  return lzw_after_code(z, px, s);
}
// the same step over the other dictionary (RHCCQ_GIF_TRIE): kTrieNodes 32-bit nodes, one a code, first child << 20 | next sibling << 8 |
// pixel; no entry's code is 0, so 0 ends a chain.  A step walks the children of the current string, at most one a palette row; a new
// entry goes in front of its siblings.  The codes that go out are the same: which strings exist does not depend on how they are found.
template <typename Dict>
RHCCQ_GIF_HD bool lzw_pixel_trie(Lzw& z, Dict node, uint32_t px, BitSink& s) {
  if (z.cur < 0) {
    z.cur = (int32_t)px;
    return false;
  }
  const uint32_t parent = node[(uint32_t)z.cur];
  uint32_t c = parent >> 20;
  for (int probe = 0; probe < kTrieNodes && c != 0u; ++probe) {    // (bounded: a chain holds every code once at the most)
    const uint32_t n = node[c];
    if ((n & 255u) == px) {
      z.cur = (int32_t)c;
      return false;
    }
    c = (n >> 8) & 4095u;
  }
  sink_put(s, (uint32_t)z.cur, z.width);
  if (z.next < (uint32_t)kMaxCode) {
    node[z.next] = (parent >> 20) << 8 | px;
    node[(uint32_t)z.cur] = (parent & 0xFFFFFu) | z.next << 20;
  }
  return lzw_after_code(z, px, s);
}
// the segment's last data code and its closing code (End behind the frame's last segment, else Clear) -> the segment's bits
RHCCQ_GIF_HD int64_t lzw_finish(Lzw& z, bool last, BitSink& s) {
  sink_put(s, (uint32_t)z.cur, z.width);
  lzw_count(z);
  sink_put(s, (1u << z.m) + (last ? 1u : 0u), z.width);
  return sink_end(s);
}

// ---- joining segments ----------------------------------------------------------------------------------------------------------------
// 32 bits of a segment's words from bit r on (r >= 0), zero from the segment's end on
RHCCQ_GIF_HD uint32_t gif_bits_at(const uint32_t* words, int64_t bits, int64_t r) {
  if (r >= bits) return 0u;
  const int64_t nw = (bits + 31) >> 5, i = r >> 5;
  const int sh = (int)(r & 31);
  const uint64_t lo = words[i], hi = i + 1 < nw ? words[i + 1] : 0u;
  return (uint32_t)((lo | hi << 32) >> sh);
}

// ---- framing -------------------------------------------------------------------------------------------------------------------------
RHCCQ_GIF_HD void gif_put16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
}
// "GIF89a", the logical screen descriptor and, with more than one frame, the loop extension behind the global table's place
RHCCQ_GIF_HD void gif_put_head(uint8_t* out, int W, int H, int n_frames, int k0, int flags, int loop) {
  const char* sig = "GIF89a";
  for (int i = 0; i < 6; ++i) out[i] = (uint8_t)sig[i];
  gif_put16(out + 6, (uint32_t)W);
  gif_put16(out + 8, (uint32_t)H);
  const bool local = flags & RHCCQ_GIF_LOCAL;
  const int tb = gif_table_bits(gif_entries(k0, flags));
  out[10] = (uint8_t)(local ? 0x70 : 0x80 | (tb - 1) << 4 | (tb - 1));
  out[11] = 0;
  out[12] = 0;
  if (n_frames > 1) {
    uint8_t* e = out + gif_front_bytes(n_frames, k0, flags) - kLoopBytes;
    const char* app = "NETSCAPE2.0";
    e[0] = 0x21;
    e[1] = 0xFF;
    e[2] = 11;
    for (int i = 0; i < 11; ++i) e[3 + i] = (uint8_t)app[i];
    e[14] = 3;
    e[15] = 1;
    gif_put16(e + 16, (uint32_t)loop);
    e[18] = 0;
  }
}
// a frame's graphic control extension, image descriptor and minimum code size (the local table lies between the last two)
RHCCQ_GIF_HD void gif_put_frame_head(uint8_t* p, int W, int H, int k, int flags, int delay, bool transparent) {
  const bool local = flags & RHCCQ_GIF_LOCAL;
  const int tb = gif_table_bits(local ? k : gif_entries(k, flags));
  p[0] = 0x21;
  p[1] = 0xF9;
  p[2] = 4;
  p[3] = (uint8_t)(1 << 2 | (transparent ? 1 : 0));
  gif_put16(p + 4, (uint32_t)delay);
  p[6] = (uint8_t)(transparent ? k : 0);
  p[7] = 0;
  p[8] = 0x2C;
  gif_put16(p + 9, 0);
  gif_put16(p + 11, 0);
  gif_put16(p + 13, (uint32_t)W);
  gif_put16(p + 15, (uint32_t)H);
  p[17] = (uint8_t)(local ? 0x80 | (tb - 1) : 0);
  p[gif_frame_front(k, flags) - 1] = (uint8_t)gif_min_code(tb);
}
// colour table entry e of a table over `rows` palette rows: the row, or zero past them
RHCCQ_GIF_HD void gif_put_entry(uint8_t* table, const uint8_t* pal, int rows, int e) {
  for (int ch = 0; ch < 3; ++ch) table[3 * e + ch] = e < rows ? pal[3 * e + ch] : (uint8_t)0;
}

}  // namespace gif
}  // namespace rhccq
