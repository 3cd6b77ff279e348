// GIF reading (EXTENSION, include/rhccq.h "GIF files read on the device"): the functions the kernels of gif_read.hip and the serial host
// forms share.  Plain C++ over <stdint.h> (and gif_write.h for its macro and limits): a host-only program may include this file without
// the HIP headers.
//   parse      gif_parse: the file's framing, a pure function of its bytes; every offset and length it reports lies inside the file;
//   codes      code_width / code_bits (where code j of a segment stands: a closed form of j), code_at, code_load (the validity test),
//              seg_bound (the segment table's size from the stream's bytes);
//   pixels     src_row (the four-pass order), compose_step (one pixel of the canvas under one frame), gif_verdict;
//   serial     unlzw_serial, compose_serial: the host forms.
#pragma once
#include "gif_write.h"

namespace rhccq {
namespace gifr {
using namespace gif;

constexpr int kTile = 256;                                 // codes a step (rhccq_gif_read_tile)
constexpr int kThreads = 256;                              // threads of a workgroup (rhccq_gif_read_threads)
constexpr int64_t kReadMax = ((int64_t)1 << 31) - 1;
constexpr uint32_t kNoFrame = 0xFFFFFFFFu;                 // the fault words: no frame has one
constexpr int kStreamPad = 16;                             // zero bytes behind every frame's stream, which starts at a multiple of 16

// a row of the segment table: 16 bytes.  pixels: the segment's total, then (the offsets launch) the pixels in front of it; both saturate
struct SegRow {
  int64_t start_bit;
  uint32_t n_codes, pixels;
};

// ---- codes ---------------------------------------------------------------------------------------------------------------------------
RHCCQ_GIF_HD int code_width(int m, int64_t j) {
  const int64_t v = ((int64_t)1 << m) + 1 + j;
  return v >= 2048 ? 12 : 32 - __builtin_clz((uint32_t)v);
}
// bits of the codes 0 .. j - 1 of a segment
RHCCQ_GIF_HD int64_t code_bits(int m, int64_t j) {
  const int64_t clear = (int64_t)1 << m;
  int64_t bits = 0, start = 0;
  for (int w = m + 1; w < 12; ++w) {
    const int64_t end = ((int64_t)1 << w) - clear - 1;     // the first code wider than w
    if (j <= end) return bits + (j - start) * w;
    bits += (end - start) * w;
    start = end;
  }
  return bits + (j - start) * 12;
}
// the code of w bits at `bit` of a stream that has 3 readable bytes from bit / 8 on
RHCCQ_GIF_HD uint32_t code_at(const uint8_t* s, int64_t bit, int w) {
  const int64_t b = bit >> 3;
  const uint32_t v = (uint32_t)s[b] | (uint32_t)s[b + 1] << 8 | (uint32_t)s[b + 2] << 16;
  return (v >> (int)(bit & 7)) & ((1u << w) - 1u);
}
RHCCQ_GIF_HD uint32_t code_limit(int m, int64_t j) {
  const int64_t clear = (int64_t)1 << m;
  return (uint32_t)(j == 0 ? clear - 1 : clear + 1 + j < 4095 ? clear + 1 + j : 4095);
}
// codes of a segment that make entries: j = 1 .. table_codes(m) - 1
RHCCQ_GIF_HD int64_t table_codes(int m) { return kMaxCode - ((int64_t)1 << m) - 1; }
// data code j of the segment at bit s0; an invalid one counts as 0 and sets *bad
RHCCQ_GIF_HD uint32_t code_load(const uint8_t* s, int64_t s0, int m, int64_t j, bool* bad) {
  const uint32_t c = code_at(s, s0 + code_bits(m, j), code_width(m, j)), clear = 1u << m;
  if (c > code_limit(m, j) || c == clear || c == clear + 1) {
    *bad = true;
    return 0u;
  }
  return c;
}
// no stream of `bytes` bytes has more segments that are not empty: a data code and the code that closes it, m + 1 bits each at the least
RHCCQ_GIF_HD int64_t seg_bound(int64_t bytes, int m) { return 8 * bytes / (2 * (m + 1)) + 1; }
RHCCQ_GIF_HD uint32_t sat32(uint64_t v) { return v > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)v; }

// what a kernel's bounds rest on, tested against the buffers' sizes
RHCCQ_GIF_HD bool frame_lzw_sound(const rhccq_gif_frame& f, int64_t stream_total, int64_t n_pixels, int64_t seg_rows) {
  if (f.w < 1 || f.h < 1 || f.w > 65535 || f.h > 65535 || f.m < 2 || f.m > 8) return false;
  if (f.stream_offset < 0 || (f.stream_offset & 15) || f.stream_bytes < 0 || f.stream_bytes > stream_total ||
      f.stream_offset > stream_total - f.stream_bytes - kStreamPad)
    return false;
  const int64_t wh = (int64_t)f.w * f.h;
  if (f.pixel_offset < 0 || wh > n_pixels || f.pixel_offset > n_pixels - wh) return false;
  const int64_t rows = seg_bound(f.stream_bytes, f.m);
  return f.first_row >= 0 && rows <= seg_rows && f.first_row <= seg_rows - rows;
}
RHCCQ_GIF_HD bool frame_paint_sound(const rhccq_gif_frame& f, int64_t n, int64_t n_pixels) {
  if (f.w < 1 || f.h < 1 || f.w > 65535 || f.h > 65535 || f.x < 0 || f.y < 0 || f.x > 65535 || f.y > 65535) return false;
  const int64_t wh = (int64_t)f.w * f.h;
  if (f.pixel_offset < 0 || wh > n_pixels || f.pixel_offset > n_pixels - wh) return false;
  return f.table_rows >= 0 && f.table_rows <= 256 && f.table_offset >= 0 && 3 * (int64_t)f.table_rows <= n && f.table_offset <= n - 3 * (int64_t)f.table_rows;
}

// ---- pixels --------------------------------------------------------------------------------------------------------------------------
// where row r of a frame of h rows stands in the stream's order
RHCCQ_GIF_HD int src_row(int r, int h, bool interlaced) {
  if (!interlaced) return r;
  const int n1 = (h + 7) / 8, n2 = (h + 3) / 8, n3 = (h + 1) / 4;
  if ((r & 7) == 0) return r >> 3;
  if ((r & 7) == 4) return n1 + (r >> 3);
  if ((r & 3) == 2) return n1 + n2 + (r >> 2);
  return n1 + n2 + n3 + (r >> 1);
}
struct Canvas { uint8_t r, g, b, covered; };
// pixel (X, Y) of the screen under frame f: `cur` is the canvas in front of the frame and behind its disposal afterwards, *shown what
// images[f] / alpha[f] hold; -> the pixel's place in the frame's rectangle (ry * w + rx), -1 outside, and its index
RHCCQ_GIF_HD int64_t compose_step(const rhccq_gif_frame& f, const uint8_t* file, const uint8_t* pixels, int X, int Y, Canvas& cur, Canvas* shown,
                                  uint32_t* index) {
  const int rx = X - f.x, ry = Y - f.y;
  if (rx < 0 || ry < 0 || rx >= f.w || ry >= f.h) {
    *shown = cur;
    return -1;
  }
  const Canvas before = cur;
  const uint32_t i = pixels[f.pixel_offset + (int64_t)src_row(ry, f.h, f.interlace != 0) * f.w + rx];
  *index = i;
  if ((int32_t)i != f.transparent) {
    const uint8_t* row = file + f.table_offset + 3 * (int64_t)i;
    const bool in = i < (uint32_t)f.table_rows;
    cur = Canvas{in ? row[0] : (uint8_t)0, in ? row[1] : (uint8_t)0, in ? row[2] : (uint8_t)0, 1};
  }
  *shown = cur;
  if (f.disposal == 2) cur = Canvas{0, 0, 0, 0};
  else if (f.disposal == 3) cur = before;
  return (int64_t)ry * f.w + rx;
}
struct Verdict { int32_t status, detail; };
RHCCQ_GIF_HD Verdict gif_verdict(uint32_t bad_code, uint32_t bad_length) {
  if (bad_code == kNoFrame && bad_length == kNoFrame) return {RHCCQ_GIFR_OK, 0};
  if (bad_code <= bad_length) return {RHCCQ_GIFR_BAD_CODE, (int32_t)bad_code};
  return {RHCCQ_GIFR_BAD_LENGTH, (int32_t)bad_length};
}

// ---- parse ---------------------------------------------------------------------------------------------------------------------------
inline uint32_t get_le16(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
inline bool bytes_are(const uint8_t* p, const char* t, int k) {
  for (int i = 0; i < k; ++i)
    if (p[i] != (uint8_t)t[i]) return false;
  return true;
}
// fills *info and the first rows of `frames` and `blocks`; the full numbers are in info->n_frames / n_blocks
inline void gif_parse(const uint8_t* f, int64_t n, rhccq_gif_info* info, rhccq_gif_frame* frames, int64_t fcap, rhccq_segment* blocks, int64_t bcap) {
  rhccq_gif_info z{};
  z.loop = -1;
  z.global_offset = -1;
  int64_t count = 0, nblocks = 0, cursor = 0, pixels = 0, rows = 0;
  auto done = [&](int status, int64_t detail) {
    z.status = status;
    z.detail = (int32_t)(detail > kReadMax ? kReadMax : detail);
    z.n_frames = (int32_t)count;
    z.n_blocks = (int32_t)(nblocks > kReadMax ? kReadMax : nblocks);
    z.stream_bytes = cursor;
    z.pixels = pixels;
    z.seg_rows = rows;
    *info = z;
  };
  if (n < 6 || !(bytes_are(f, "GIF87a", 6) || bytes_are(f, "GIF89a", 6))) return done(RHCCQ_GIFR_BAD_SIGNATURE, 0);
  if (n < 13) return done(RHCCQ_GIFR_TRUNCATED, 6);
  z.width = (int32_t)get_le16(f + 6);
  z.height = (int32_t)get_le16(f + 8);
  if (z.width == 0 || z.height == 0) return done(RHCCQ_GIFR_BAD_HEADER, 6);
  int64_t pos = 13;
  if (f[10] & 0x80) {
    z.global_rows = 2 << (f[10] & 7);
    if (n - pos < 3 * z.global_rows) return done(RHCCQ_GIFR_TRUNCATED, 13);
    z.global_offset = pos;
    pos += 3 * z.global_rows;
  }
  int32_t g_disposal = 0, g_transparent = -1, g_delay = 0;   // the pending graphic control extension
  for (;;) {
    if (pos >= n) return done(RHCCQ_GIFR_TRUNCATED, n);
    const uint8_t intro = f[pos];
    if (intro == 0x3B) break;
    if (intro == 0x21) {
      if (n - pos < 2) return done(RHCCQ_GIFR_TRUNCATED, pos);
      const uint8_t label = f[pos + 1];
      int64_t q = pos + 2;
      bool netscape = false, loop_seen = z.loop >= 0;
      for (int sub = 0;; ++sub) {
        if (q >= n) return done(RHCCQ_GIFR_TRUNCATED, pos);
        const int len = f[q];
        if (len == 0) {
          ++q;
          break;
        }
        if (n - q - 1 < len) return done(RHCCQ_GIFR_TRUNCATED, pos);
        const uint8_t* d = f + q + 1;
        if (label == 0xF9 && sub == 0 && len >= 4) {
          g_disposal = (d[0] >> 2) & 7;
          g_transparent = d[0] & 1 ? (int32_t)d[3] : -1;
          g_delay = (int32_t)get_le16(d + 1);
        }
        if (label == 0xFF && sub == 0) netscape = len == 11 && (bytes_are(d, "NETSCAPE2.0", 11) || bytes_are(d, "ANIMEXTS1.0", 11));
        if (label == 0xFF && sub > 0 && netscape && !loop_seen && len >= 3 && d[0] == 1) {
          z.loop = (int32_t)get_le16(d + 1);
          loop_seen = true;
        }
        q += 1 + len;
        if (sub > 1) sub = 1;                              // (only "first" and "later" matter)
      }
      pos = q;
      continue;
    }
    if (intro != 0x2C) return done(RHCCQ_GIFR_BAD_BLOCK, pos);
    if (n - pos < 10) return done(RHCCQ_GIFR_TRUNCATED, pos);
    if (count >= kMaxFrames) return done(RHCCQ_GIFR_LIMIT, 0);
    rhccq_gif_frame fr{};
    fr.x = (int32_t)get_le16(f + pos + 1);
    fr.y = (int32_t)get_le16(f + pos + 3);
    fr.w = (int32_t)get_le16(f + pos + 5);
    fr.h = (int32_t)get_le16(f + pos + 7);
    const uint8_t packed = f[pos + 9];
    fr.interlace = packed & 0x40 ? 1 : 0;
    if (fr.w == 0 || fr.h == 0 || fr.x + fr.w > z.width || fr.y + fr.h > z.height) return done(RHCCQ_GIFR_BAD_FRAME, count);
    int64_t q = pos + 10;
    if (packed & 0x80) {
      fr.table_rows = 2 << (packed & 7);
      if (n - q < 3 * fr.table_rows) return done(RHCCQ_GIFR_TRUNCATED, pos);
      fr.table_offset = q;
      q += 3 * fr.table_rows;
    } else if (z.global_rows) {
      fr.table_rows = z.global_rows;
      fr.table_offset = z.global_offset;
    } else {
      return done(RHCCQ_GIFR_NO_TABLE, count);
    }
    if (q >= n) return done(RHCCQ_GIFR_TRUNCATED, pos);
    fr.m = f[q];
    if (fr.m < 2 || fr.m > 8) return done(RHCCQ_GIFR_BAD_HEADER, q);
    ++q;
    fr.first_block = (int32_t)(nblocks > kReadMax ? kReadMax : nblocks);
    fr.stream_offset = cursor;
    int64_t acc = 0, nb = 0;
    for (;;) {
      if (q >= n) return done(RHCCQ_GIFR_TRUNCATED, pos);
      const int len = f[q];
      if (len == 0) {
        ++q;
        break;
      }
      if (n - q - 1 < len) return done(RHCCQ_GIFR_TRUNCATED, pos);
      if (nblocks + nb < bcap) blocks[nblocks + nb] = rhccq_segment{q + 1, len, count, cursor + acc};
      ++nb;
      acc += len;
      q += 1 + len;
    }
    fr.n_blocks = (int32_t)nb;
    fr.stream_bytes = acc;
    fr.transparent = g_transparent;
    fr.disposal = g_disposal;
    fr.delay = g_delay;
    g_disposal = 0;
    g_transparent = -1;
    g_delay = 0;
    fr.pixel_offset = pixels;
    fr.first_row = rows;
    if (count < fcap) frames[count] = fr;
    nblocks += nb;
    cursor = ((cursor + acc + 15) & ~(int64_t)15) + kStreamPad;
    pixels += (int64_t)fr.w * fr.h;
    rows += seg_bound(acc, fr.m);
    ++count;
    pos = q;
  }
  if (count == 0) return done(RHCCQ_GIFR_NO_FRAMES, 0);
  // (F <= 2^20 and H W < 2^32: the product is inside int64)
  if (n > kReadMax || count * ((int64_t)z.width * z.height) > kReadMax / 3 || rows > kReadMax / (int64_t)sizeof(SegRow) || nblocks > kReadMax)
    return done(RHCCQ_GIFR_LIMIT, 0);
  return done(RHCCQ_GIFR_OK, 0);
}

// ---- the serial forms ----------------------------------------------------------------------------------------------------------------
// one frame's stream -> its strings at out (clipped to wh bytes); -> the pixels the stream holds.  *bad: an invalid code was met
inline int64_t unlzw_frame_serial(const uint8_t* s, int64_t bytes, int m, uint8_t* out, int64_t wh, bool* bad, int64_t* n_segments) {
  const int64_t bits = 8 * bytes;
  const uint32_t clear = 1u << m;
  static thread_local uint32_t ent[kMaxCode];              // prefix 12 | suffix 8 | len 12, as the kernels pack them
  static thread_local uint8_t first[kMaxCode];
  int64_t s0 = 0, total = 0;
  for (;;) {
    // the segment: its codes up to Clear, End or the end of the bits
    int64_t j = 0, next = 0;
    bool last = false;
    for (;; ++j) {
      const int64_t off = s0 + code_bits(m, j);
      const int w = code_width(m, j);
      if (off + w > bits) { last = true; break; }
      const uint32_t c = code_at(s, off, w);
      if (c == clear) { next = off + w; break; }
      if (c == clear + 1) { last = true; break; }
    }
    if (j > 0) {
      ++*n_segments;
      for (uint32_t c = 0; c < clear; ++c) {
        ent[c] = c | c << 12 | 1u << 20;
        first[c] = (uint8_t)c;
      }
      uint32_t prev = 0;
      for (int64_t k = 0; k < j; ++k) {
        const uint32_t c = code_load(s, s0, m, k, bad);
        if (k >= 1 && k < table_codes(m)) {
          const uint32_t e = clear + 1 + (uint32_t)k;
          first[e] = first[prev];
          ent[e] = prev | (uint32_t)first[c] << 12 | ((ent[prev] >> 20) + 1) << 20;
        }
        const int64_t len = ent[c] >> 20;
        int64_t p = total + len - 1;
        uint32_t t = c;
        for (int64_t guard = 0; t >= clear + 2 && guard < kMaxCode; ++guard) {
          if (p >= 0 && p < wh) out[p] = (uint8_t)(ent[t] >> 12);
          --p;
          t = ent[t] & 4095u;
        }
        if (p >= 0 && p < wh) out[p] = (uint8_t)t;
        total += len;
        prev = c;
      }
    }
    if (last) break;
    s0 = next;
  }
  return total;
}
// streams as the parser lays them out; -> the fault words
inline void unlzw_serial(const uint8_t* streams, int64_t stream_total, const rhccq_gif_frame* frames, int64_t n_frames, uint8_t* pixels, int64_t n_pixels,
                         int64_t* counts, uint32_t* bad_code, uint32_t* bad_length, int64_t* n_segments) {
  *bad_code = *bad_length = kNoFrame;
  int64_t segs = 0;
  for (int64_t f = 0; f < n_frames; ++f) {
    const rhccq_gif_frame& fr = frames[f];
    if (counts) counts[f] = 0;
    if (!frame_lzw_sound(fr, stream_total, n_pixels, kReadMax)) continue;
    bool bad = false;
    const int64_t wh = (int64_t)fr.w * fr.h;
    const int64_t got = unlzw_frame_serial(streams + fr.stream_offset, fr.stream_bytes, fr.m, pixels + fr.pixel_offset, wh, &bad, &segs);
    if (counts) counts[f] = got;
    if (bad && *bad_code == kNoFrame) *bad_code = (uint32_t)f;
    if (got != wh && *bad_length == kNoFrame) *bad_length = (uint32_t)f;
  }
  if (n_segments) *n_segments = segs;
}
inline void compose_serial(const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames, int64_t n_frames, int H,
                           int W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  for (int Y = 0; Y < H; ++Y)
    for (int X = 0; X < W; ++X) {
      Canvas cur{0, 0, 0, 0};
      for (int64_t f = 0; f < n_frames; ++f) {
        Canvas shown = cur;
        if (frame_paint_sound(frames[f], n, n_pixels)) {
          uint32_t index = 0;
          const int64_t at = compose_step(frames[f], file, pixels, X, Y, cur, &shown, &index);
          if (at >= 0 && idx) idx[frames[f].pixel_offset + at] = (uint8_t)index;
        }
        const int64_t o = (f * H + Y) * W + X;
        rgb[3 * o] = shown.r;
        rgb[3 * o + 1] = shown.g;
        rgb[3 * o + 2] = shown.b;
        if (alpha) alpha[o] = shown.covered ? 255 : 0;
      }
    }
}

}  // namespace gifr
}  // namespace rhccq
