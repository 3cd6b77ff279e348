// JPEG reading (EXTENSION, include/rhccq.h "JPEG files read on the device"): the functions the kernels of jpeg_read.hip and the serial host
// forms share.  Plain C++ over <stdint.h>: a host-only program may include this file without the HIP headers.
//   parse      jpeg_parse: the file's framing, its tables and its restart intervals, a pure function of the bytes;
//   bytes      kept (which bytes of the scan stay in the unstuffed stream), peek32;
//   entropy    pack / unpack (a decoder state in 64 bits), run: the one decoder every stage uses -- from a state to a bit, counting or
//              writing;
//   pixels     idct8 (one pass of the islow IDCT), idct_block, rgb_at (upsampling and colour for one pixel);
//   serial     unstuff_serial, dc_serial, planes_serial, rgb_serial: the host forms;
//   kernels    (under hipcc only) SubRow, seg_combine / seg_block_scan (sums that restart), tables_to_lds, sub_end, dc_seq: what the kernels
//              of jpeg_read.hip and of jpeg_batch.hip share.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/rhccq.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RHCCQ_JPEG_HD __host__ __device__ __forceinline__
#else
#define RHCCQ_JPEG_HD inline
#endif

namespace rhccq {
namespace jpegr {

constexpr int kSubBits = 512;                              // the default subsequence (rhccq_jpeg_subsequence_bits)
constexpr int kThreads = 256;                              // lanes of a workgroup: subsequences of a workgroup of the sync launch
constexpr int kTileBytes = 16 * kThreads;                  // scan bytes of a workgroup of the unstuff launches
constexpr int kStreamPad = 16;                             // zero bytes behind the unstuffed stream (peek32 reads up to 7 of them)
constexpr int64_t kReadMax = ((int64_t)1 << 31) - 1;
constexpr uint32_t kNoInterval = 0xFFFFFFFFu;

RHCCQ_JPEG_HD int zigzag(int k) {
  static constexpr uint8_t z[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                    41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                    30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return z[k & 63];
}

// ---- geometry ------------------------------------------------------------------------------------------------------------------------
// the planes: component c has bw[c] x bh[c] blocks from block base[c] on; whole MCUs
struct Geo {
  int32_t W, H, n_comp, hs, vs, bpm, mcus_x, R;
  int64_t mcus, blocks, base[3];
  int32_t bw[3], bh[3];
};
RHCCQ_JPEG_HD Geo geo_of(const rhccq_jpeg_info& f) {
  Geo g;
  g.W = f.width, g.H = f.height, g.n_comp = f.n_comp, g.hs = f.hs, g.vs = f.vs, g.bpm = f.blocks_per_mcu, g.mcus_x = f.mcus_x, g.R = f.restart_interval;
  g.mcus = (int64_t)f.mcus_x * f.mcus_y;
  int64_t at = 0;
  for (int c = 0; c < 3; ++c) {
    g.bw[c] = f.mcus_x * (c == 0 ? f.hs : 1);
    g.bh[c] = f.mcus_y * (c == 0 ? f.vs : 1);
    g.base[c] = at;
    if (c < f.n_comp) at += (int64_t)g.bw[c] * g.bh[c];
  }
  g.blocks = at;
  return g;
}
// what every kernel's bounds rest on: an info that is the parse's own
RHCCQ_JPEG_HD bool info_sound(const rhccq_jpeg_info& f, int64_t n) {
  if (f.width < 1 || f.height < 1 || f.width > 65535 || f.height > 65535 || (f.n_comp != 1 && f.n_comp != 3)) return false;
  if (f.hs < 1 || f.hs > 2 || f.vs < 1 || f.vs > f.hs || (f.n_comp == 1 && f.hs != 1)) return false;
  const int mw = 8 * f.hs, mh = 8 * f.vs;
  if (f.mcus_x != (f.width + mw - 1) / mw || f.mcus_y != (f.height + mh - 1) / mh) return false;
  if (f.blocks_per_mcu != (f.n_comp == 1 ? 1 : f.hs * f.vs + 2) || f.restart_interval < 0 || f.restart_interval > 65535) return false;
  const int64_t mcus = (int64_t)f.mcus_x * f.mcus_y;
  const int64_t want = f.restart_interval ? (mcus + f.restart_interval - 1) / f.restart_interval : 1;
  if (f.n_intervals != want || f.blocks != mcus * f.blocks_per_mcu) return false;
  if (n < 0 || n > kReadMax || f.scan_offset < 0 || f.scan_bytes < 0 || f.scan_offset > n - f.scan_bytes) return false;
  return f.stream_bytes >= 0 && f.stream_bytes <= f.scan_bytes;
}
RHCCQ_JPEG_HD bool sub_bits_ok(int32_t s) { return s == 0 || (s >= 128 && s <= 65536 && s % 32 == 0); }
RHCCQ_JPEG_HD int64_t sub_count(int64_t stream_bytes, int32_t s) {
  const int64_t n = (8 * stream_bytes + s - 1) / s;
  return n < 1 ? 1 : n;
}

// ---- bytes ---------------------------------------------------------------------------------------------------------------------------
// does byte i of the scan [lo, hi) stay?  Not behind an 0xFF (a stuffed zero, a marker's second byte, fill), and not an 0xFF in front of
// anything but a zero (a marker's first byte, fill).  hi < n in a parsed file: EOI stands there
RHCCQ_JPEG_HD bool kept(const uint8_t* f, int64_t n, int64_t lo, int64_t i) {
  if (i > lo && f[i - 1] == 0xFF) return false;
  return !(f[i] == 0xFF && (i + 1 >= n || f[i + 1] != 0));
}
RHCCQ_JPEG_HD uint32_t bswap(uint32_t v) { return v >> 24 | (v >> 8 & 0xFF00u) | (v << 8 & 0xFF0000u) | v << 24; }
// 32 bits from bit `pos` of the unstuffed stream, the first in the top bit; reads the words pos / 32 and pos / 32 + 1
RHCCQ_JPEG_HD uint32_t peek32(const uint32_t* w, int64_t pos) {
  const int64_t i = pos >> 5;
  const int sh = (int)(pos & 31);
  const uint32_t hi = bswap(w[i]), lo = bswap(w[i + 1]);
  return sh ? hi << sh | lo >> (32 - sh) : hi;
}

// ---- entropy -------------------------------------------------------------------------------------------------------------------------
RHCCQ_JPEG_HD uint64_t pack(int64_t pos, int b, int z) { return (uint64_t)pos << 10 | (uint64_t)b << 6 | (uint64_t)z; }
constexpr uint32_t kAbs = 0x80000000u;                     // a count that is a block number, not a number of blocks

struct Dec {
  const uint32_t* words;                                   // the unstuffed stream
  const rhccq_jpeg_tables* T;
  const rhccq_segment* iv;
  int64_t n_iv, total_bits;
  Geo g;
};
RHCCQ_JPEG_HD int64_t first_block(const Geo& g, int64_t k) {
  const int64_t m = g.R ? k * g.R : (k ? g.mcus : 0);
  return (m < g.mcus ? m : g.mcus) * g.bpm;
}
// where block A of the scan's order stands in the planes
RHCCQ_JPEG_HD int64_t block_at(const Geo& g, int64_t A) {
  const int64_t mcu = A / g.bpm, my = mcu / g.mcus_x;
  const int b = (int)(A - mcu * g.bpm), mx = (int)(mcu - my * g.mcus_x);
  if (b < g.hs * g.vs) return (my * g.vs + b / g.hs) * g.bw[0] + mx * g.hs + b % g.hs;
  const int c = b - g.hs * g.vs + 1;
  return g.base[c] + my * g.bw[c] + mx;
}
RHCCQ_JPEG_HD int comp_of(const Geo& g, int b) { return g.n_comp == 1 || b < g.hs * g.vs ? 0 : b - g.hs * g.vs + 1; }
// the last interval that starts at or in front of bit pos; n_iv behind the last bit
RHCCQ_JPEG_HD int64_t interval_of(const Dec& d, int64_t pos) {
  if (pos >= d.total_bits) return d.n_iv;
  int64_t lo = 0, hi = d.n_iv;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (8 * d.iv[mid].dst <= pos) lo = mid; else hi = mid;
  }
  return lo;
}
RHCCQ_JPEG_HD void note_bad(uint32_t* bad, int64_t k) {
#if defined(__HIP_DEVICE_COMPILE__)
  atomicMin(bad, (uint32_t)k);
#else
  if ((uint32_t)k < *bad) *bad = (uint32_t)k;
#endif
}

// Decodes from `entry` until a symbol starts at or behind end_bit.  first: the entry is the stream's start (interval 0, whatever its
// length).  WRITE: A is the number of the block the entry stands in; coefficients go to coef (blocks g.blocks), faults to *bad.  ->
// *leave: the state at the end; *count: blocks completed, or kAbs | the number of the block the end stands in where an interval's start
// was crossed.  Every turn of the loop moves pos on by a bit or more, or k by one: at most (end_bit - pos) + 31 + n_iv turns.
// A fault (no code, a run past 63, a DC category above 11) is noted and the decoder goes on one bit further on, in front of a block.
template <bool WRITE>
RHCCQ_JPEG_HD void run(const Dec& d, uint64_t entry, bool first, int64_t end_bit, int64_t A, int16_t* coef, uint32_t* bad, uint64_t* leave, uint32_t* count) {
  const Geo& g = d.g;
  int64_t pos = (int64_t)(entry >> 10);
  int b = (int)(entry >> 6 & 15), z = (int)(entry & 63);
  if (pos > d.total_bits) pos = d.total_bits;
  if (b >= g.bpm) b = 0;
  int64_t k = first ? 0 : interval_of(d, pos);
  bool abs = false;
  int64_t cnt = 0;
  if (k < d.n_iv && (first || (pos == 8 * d.iv[k].dst && b == 0 && z == 0))) {
    abs = true;
    cnt = first_block(g, k);
    if (WRITE) A = cnt;
  }
  int64_t at = 0;                                          // (WRITE) the block's coefficients, -1: none to write
  if (WRITE) at = A < first_block(g, k + 1) ? 64 * block_at(g, A) : -1;
  while (k < d.n_iv) {
    const int64_t next = k + 1 < d.n_iv ? 8 * d.iv[k + 1].dst : d.total_bits;
    bool over = pos >= next, err = false;
    if (!over && pos >= end_bit) break;
    int len = 0, s = 0, nz = z;
    uint32_t v = 0;
    if (!over) {
      v = peek32(d.words, pos);
      const int t = 2 * comp_of(g, b) + (z ? 1 : 0);
      const uint32_t e = d.T->look[t][v >> 23];
      int sym = (int)(e & 255u);
      len = (int)(e >> 8);
      if (len == 0) {
        for (int l = 10; l <= 16 && len == 0; ++l) {
          const int32_t c = (int32_t)(v >> (32 - l));
          if (c <= d.T->maxcode[t][l]) {
            len = l;
            sym = d.T->vals[t][(d.T->valoff[t][l] + c) & 255];
          }
        }
        err = len == 0;
      }
      if (err && next - pos < 16) {                        // the pad: what is left of the interval is no whole code
        err = false;
        len = 32;
      } else if (z == 0) {
        s = sym;
        err = err || s > 11;
        nz = 1;
      } else {
        s = sym & 15;
        const int r = sym >> 4;
        if (s == 0) nz = r == 15 ? z + 16 : 64;
        else nz = z + r + 1;
        err = err || (nz > 64 && !(s == 0 && r != 15)) || (s == 0 && r == 15 && nz > 63);
      }
      over = !err && pos + len + s > next;
    }
    if (err) {                                             // no symbol here: a bit further on, in front of a block.  (A lane that guessed wrongly
      if (WRITE) note_bad(bad, k);                         // meets this often; leaving the interval instead would end every guess's chance
      ++pos;                                               // to fall into step in a file without restart markers)
      z = 0;
      continue;
    }
    if (over) {                                            // the interval ends here
      if (WRITE && (b != 0 || z != 0 || next - pos >= 8 || A != first_block(g, k + 1))) note_bad(bad, k);
      ++k;
      pos = next;
      b = z = 0;
      abs = true;
      cnt = first_block(g, k);
      if (WRITE) {
        A = cnt;
        at = k < d.n_iv && A < first_block(g, k + 1) ? 64 * block_at(g, A) : -1;
      }
      continue;
    }
    if (WRITE && s && at >= 0) {
      const int32_t bits = (int32_t)((v << len) >> (32 - s));
      const int32_t val = bits < (1 << (s - 1)) ? bits - (1 << s) + 1 : bits;
      coef[at + (z ? zigzag(nz - 1) : 0)] = (int16_t)val;
    }
    pos += len + s;
    z = nz;
    if (z >= 64) {
      z = 0;
      b = b + 1 == g.bpm ? 0 : b + 1;
      ++cnt;
      if (WRITE) {
        ++A;
        at = A < first_block(g, k + 1) ? 64 * block_at(g, A) : -1;
      }
    }
  }
  if (k >= d.n_iv) pos = d.total_bits;
  *leave = pack(pos, b, z);
  *count = abs ? kAbs | (uint32_t)cnt : (uint32_t)cnt;
}

// ---- pixels --------------------------------------------------------------------------------------------------------------------------
// one pass of jidctint.c's jpeg_idct_islow over eight values; the sums wrap as 32-bit two's complement
RHCCQ_JPEG_HD void idct8(const int32_t* x, int shift, int32_t* y) {
  typedef uint32_t U;
  const U x0 = (U)x[0], x1 = (U)x[1], x2 = (U)x[2], x3 = (U)x[3], x4 = (U)x[4], x5 = (U)x[5], x6 = (U)x[6], x7 = (U)x[7];
  U z1 = (x2 + x6) * 4433u;
  const U e2 = z1 - x6 * 15137u, e3 = z1 + x2 * 6270u;
  const U e0 = (x0 + x4) << 13, e1 = (x0 - x4) << 13;
  const U t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
  U t0 = x7, t1 = x5, t2 = x3, t3 = x1;
  z1 = t0 + t3;
  U z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
  const U z5 = (z3 + z4) * 9633u;
  t0 *= 2446u, t1 *= 16819u, t2 *= 25172u, t3 *= 12299u;
  z1 *= (U)-7373, z2 *= (U)-20995, z3 *= (U)-16069, z4 *= (U)-3196;
  z3 += z5, z4 += z5;
  t0 += z1 + z3, t1 += z2 + z4, t2 += z2 + z3, t3 += z1 + z4;
  const U r = 1u << (shift - 1);
  y[0] = (int32_t)(t10 + t3 + r) >> shift, y[7] = (int32_t)(t10 - t3 + r) >> shift;
  y[1] = (int32_t)(t11 + t2 + r) >> shift, y[6] = (int32_t)(t11 - t2 + r) >> shift;
  y[2] = (int32_t)(t12 + t1 + r) >> shift, y[5] = (int32_t)(t12 - t1 + r) >> shift;
  y[3] = (int32_t)(t13 + t0 + r) >> shift, y[4] = (int32_t)(t13 - t0 + r) >> shift;
}
RHCCQ_JPEG_HD void idct_column(const int16_t* coef, const uint16_t* q, int c, int32_t* ws) {
  int32_t x[8];
  for (int r = 0; r < 8; ++r) x[r] = (int32_t)((uint32_t)(int32_t)coef[8 * r + c] * (uint32_t)q[8 * r + c]);
  idct8(x, 11, ws);
}
RHCCQ_JPEG_HD uint8_t clamp255(int32_t v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
RHCCQ_JPEG_HD void idct_row(const int32_t* ws, uint8_t* out) {
  int32_t y[8];
  idct8(ws, 18, y);
  for (int c = 0; c < 8; ++c) out[c] = clamp255((int32_t)((uint32_t)y[c] + 128u));
}

// a chroma sample at output column x of a row of true width cw: libjpeg's triangle filter over a(i), the row's value at column i
template <class Row>
RHCCQ_JPEG_HD int32_t fancy(const Row& a, int x, int cw, int mid, int lo_round, int hi_round, int shift) {
  const int i = x >> 1;
  if (x == 0) return (mid * a(0) + (mid == 4 ? lo_round : 0)) >> (mid == 4 ? shift : 0);
  if (x & 1) {
    if (i + 1 < cw) return (3 * a(i) + a(i + 1) + hi_round) >> shift;
    return (mid * a(i) + (mid == 4 ? hi_round : 0)) >> (mid == 4 ? shift : 0);
  }
  return (3 * a(i) + a(i - 1) + lo_round) >> shift;
}
struct Row1 {
  const uint8_t* s;
  RHCCQ_JPEG_HD int32_t operator()(int i) const { return s[i]; }
};
struct Row2 {
  const uint8_t *s0, *s1;
  RHCCQ_JPEG_HD int32_t operator()(int i) const { return 3 * s0[i] + s1[i]; }
};
// component c (1 or 2) at pixel (y, x)
RHCCQ_JPEG_HD int32_t chroma_at(const Geo& g, const uint8_t* planes, int c, int y, int x) {
  const int64_t pw = 8 * (int64_t)g.bw[c];
  const uint8_t* p = planes + 64 * g.base[c];
  if (g.hs == 1) return p[y * pw + x];
  const int cw = (g.W + 1) / 2;
  if (cw <= 2) return p[(g.vs == 1 ? y : y >> 1) * pw + (x >> 1)];   // libjpeg replicates a component of one or two columns
  if (g.vs == 1) return fancy(Row1{p + y * pw}, x, cw, 1, 1, 2, 2);
  const int ch = (g.H + 1) / 2, r0 = y >> 1;
  int r1 = r0 + (y & 1 ? 1 : -1);
  r1 = r1 < 0 ? 0 : r1 > ch - 1 ? ch - 1 : r1;
  return fancy(Row2{p + r0 * pw, p + r1 * pw}, x, cw, 4, 8, 7, 4);
}
RHCCQ_JPEG_HD void rgb_at(const Geo& g, const uint8_t* planes, int y, int x, uint8_t* out) {
  const int32_t Y = planes[y * (8 * (int64_t)g.bw[0]) + x];
  if (g.n_comp == 1) {
    out[0] = out[1] = out[2] = (uint8_t)Y;
    return;
  }
  const int32_t cb = chroma_at(g, planes, 1, y, x) - 128, cr = chroma_at(g, planes, 2, y, x) - 128;
  out[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  out[1] = clamp255(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16));
  out[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// ---- parse ---------------------------------------------------------------------------------------------------------------------------
inline uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }

struct HuffSrc {
  bool seen;
  uint8_t counts[16], vals[256];
};
// the decoder's tables of one code: nothing here can fail, the counts were tested
inline void huff_build(const HuffSrc& h, rhccq_jpeg_tables* T, int t) {
  memset(T->look[t], 0, sizeof T->look[t]);
  memcpy(T->vals[t], h.vals, 256);
  int code = 0, at = 0;
  for (int l = 1; l <= 16; ++l) {
    const int cnt = h.counts[l - 1];
    T->maxcode[t][l] = cnt ? code + cnt - 1 : -1;
    T->valoff[t][l] = at - code;
    if (l <= 9)
      for (int i = 0; i < cnt; ++i)
        for (int j = 0; j < 1 << (9 - l); ++j) T->look[t][((code + i) << (9 - l)) + j] = (uint16_t)(l << 8 | h.vals[at + i]);
    code = (code + cnt) << 1;
    at += cnt;
  }
  T->maxcode[t][0] = T->maxcode[t][17] = -1;
  T->valoff[t][0] = T->valoff[t][17] = 0;
}

// fills *info, *T and the first rows of iv; the full number of intervals is info->n_intervals
inline void jpeg_parse(const uint8_t* f, int64_t n, rhccq_jpeg_info* info, rhccq_jpeg_tables* T, rhccq_segment* iv, int64_t cap) {
  rhccq_jpeg_info z{};
  memset(T, 0, sizeof *T);
  auto done = [&](int status, int64_t detail) {
    z.status = status;
    z.detail = (int32_t)(detail > kReadMax ? kReadMax : detail);
    *info = z;
  };
  if (n < 2 || f[0] != 0xFF || f[1] != 0xD8) return done(RHCCQ_JPEG_BAD_SIGNATURE, 0);
  if (n > kReadMax) return done(RHCCQ_JPEG_LIMIT, 0);
  uint16_t qt[4][64] = {};
  HuffSrc huff[2][4] = {};
  bool qt_seen[4] = {false, false, false, false}, sof = false, jfif = false;
  int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0}, adobe = -1;
  int64_t pos = 2;
  for (;;) {
    if (pos + 2 > n || f[pos] != 0xFF) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
    while (pos + 2 < n && f[pos + 1] == 0xFF) ++pos;       // fill
    const int m = f[pos + 1];
    if (m == 0 || m == 0x01 || (m >= 0xD0 && m <= 0xD9) || pos + 4 > n) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
    const int64_t L = be16(f + pos + 2);
    if (L < 2 || pos + 2 + L > n) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
    const uint8_t* p = f + pos + 4;                        // L - 2 bytes
    if (m == 0xC4) {
      int64_t q = 0;
      while (q < L - 2) {
        if (L - 2 - q < 17) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
        const int tc = p[q] >> 4, th = p[q] & 15;
        if (tc > 1 || th > 3) return done(RHCCQ_JPEG_BAD_TABLE, pos);
        HuffSrc& h = huff[tc][th];
        int total = 0, code = 0;
        for (int l = 0; l < 16; ++l) {
          h.counts[l] = p[q + 1 + l];
          total += h.counts[l];
          code += h.counts[l];
          if (code > 1 << (l + 1)) return done(RHCCQ_JPEG_BAD_TABLE, pos);
          code <<= 1;
        }
        if (total > 256) return done(RHCCQ_JPEG_BAD_TABLE, pos);
        if (L - 2 - q - 17 < total) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
        memset(h.vals, 0, 256);
        for (int i = 0; i < total; ++i) {
          h.vals[i] = p[q + 17 + i];
          if (tc == 0 && h.vals[i] > 15) return done(RHCCQ_JPEG_BAD_TABLE, pos);
        }
        h.seen = true;
        q += 17 + total;
      }
    } else if (m == 0xDB) {
      int64_t q = 0;
      while (q < L - 2) {
        const int pq = p[q] >> 4, tq = p[q] & 15;
        if (pq > 1 || tq > 3) return done(RHCCQ_JPEG_BAD_TABLE, pos);
        if (L - 2 - q < 1 + 64 * (pq + 1)) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
        for (int i = 0; i < 64; ++i) qt[tq][zigzag(i)] = (uint16_t)(pq ? be16(p + q + 1 + 2 * i) : p[q + 1 + i]);
        qt_seen[tq] = true;
        q += 1 + 64 * (pq + 1);
      }
    } else if (m == 0xDD) {
      if (L != 4) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
      z.restart_interval = (int32_t)be16(p);
    } else if (m == 0xE0) {
      if (L >= 7 && memcmp(p, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {
      if (L >= 14 && memcmp(p, "Adobe", 5) == 0) adobe = p[11];
    } else if (m == 0xC0 || m == 0xC1) {
      if (sof || L < 8 || L != 8 + 3 * (int64_t)p[5]) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
      sof = true;
      if (p[0] != 8 || be16(p + 1) == 0) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      z.height = (int32_t)be16(p + 1);
      z.width = (int32_t)be16(p + 3);
      z.n_comp = p[5];
      if (z.width == 0) return done(RHCCQ_JPEG_BAD_HEADER, pos);
      if (z.n_comp != 1 && z.n_comp != 3) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      z.hs = z.vs = 1;
      for (int c = 0; c < z.n_comp; ++c) {
        const int h = p[7 + 3 * c] >> 4, v = p[7 + 3 * c] & 15;
        comp_id[c] = p[6 + 3 * c];
        comp_tq[c] = p[8 + 3 * c];
        if (h == 0 || v == 0 || comp_tq[c] > 3) return done(RHCCQ_JPEG_BAD_HEADER, pos);
        if (z.n_comp == 3 && c == 0) {
          if (!((h == 1 && v == 1) || (h == 2 && v == 1) || (h == 2 && v == 2))) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
          z.hs = h, z.vs = v;
        }
        if (z.n_comp == 3 && c > 0 && (h != 1 || v != 1)) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      }
      z.mcus_x = (z.width + 8 * z.hs - 1) / (8 * z.hs);
      z.mcus_y = (z.height + 8 * z.vs - 1) / (8 * z.vs);
      z.blocks_per_mcu = z.n_comp == 1 ? 1 : z.hs * z.vs + 2;
      z.blocks = (int64_t)z.mcus_x * z.mcus_y * z.blocks_per_mcu;
    } else if ((m >= 0xC2 && m <= 0xCF) || m == 0xDC) {
      return done(RHCCQ_JPEG_UNSUPPORTED, pos);
    } else if (m == 0xDA) {
      if (!sof || L < 6 || L != 6 + 2 * (int64_t)p[0]) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
      if (p[0] != z.n_comp) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      if (z.n_comp == 3 && adobe >= 0 && adobe != 1) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      // (libjpeg's rule without a JFIF or an Adobe segment: components named 'R', 'G', 'B' are RGB, not converted)
      if (z.n_comp == 3 && adobe < 0 && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      for (int c = 0; c < z.n_comp; ++c) {
        const int td = p[2 + 2 * c] >> 4, ta = p[2 + 2 * c] & 15;
        if (p[1 + 2 * c] != comp_id[c]) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
        if (td > 3 || ta > 3) return done(RHCCQ_JPEG_BAD_HEADER, pos);
        if (!huff[0][td].seen || !huff[1][ta].seen || !qt_seen[comp_tq[c]]) return done(RHCCQ_JPEG_BAD_SEGMENT, pos);
        memcpy(T->quant[c], qt[comp_tq[c]], sizeof T->quant[c]);
        huff_build(huff[0][td], T, 2 * c);
        huff_build(huff[1][ta], T, 2 * c + 1);
      }
      const uint8_t* tail = p + 1 + 2 * z.n_comp;
      if (tail[0] != 0 || tail[1] != 63 || tail[2] != 0) return done(RHCCQ_JPEG_UNSUPPORTED, pos);
      pos += 2 + L;
      break;
    }
    pos += 2 + L;
  }
  // the scan: its markers, and what stays of its bytes
  const int64_t mcus = (int64_t)z.mcus_x * z.mcus_y, R = z.restart_interval;
  z.scan_offset = pos;
  int64_t count = 0, stay = 0, start = pos, start_dst = 0, p = pos;
  auto close = [&](int64_t end) {
    if (count < cap) iv[count] = rhccq_segment{start, end - start, R ? count * R : 0, start_dst};
    ++count;
  };
  for (;;) {
    const uint8_t* q = p < n ? (const uint8_t*)memchr(f + p, 0xFF, (size_t)(n - p)) : nullptr;
    if (!q || q + 1 >= f + n) return done(RHCCQ_JPEG_BAD_SEGMENT, n);
    int64_t i = q - f;
    stay += i - p;
    if (f[i + 1] == 0) {
      ++stay;
      p = i + 2;
      continue;
    }
    const int64_t ff = i;
    while (i + 1 < n && f[i + 1] == 0xFF) ++i;
    if (i + 1 >= n) return done(RHCCQ_JPEG_BAD_SEGMENT, n);
    const int m = f[i + 1];
    if (m == 0xD9) {
      close(ff);
      z.scan_bytes = ff - z.scan_offset;
      break;
    }
    if (m >= 0xD0 && m <= 0xD7) {
      if (R == 0 || m != 0xD0 + (int)(count & 7)) return done(RHCCQ_JPEG_BAD_RESTART, count);
      close(ff);
      start = p = i + 2;
      start_dst = stay;
      continue;
    }
    return done(RHCCQ_JPEG_UNSUPPORTED, ff);               // (a zero behind fill included)
  }
  z.n_intervals = (int32_t)(count > kReadMax ? kReadMax : count);
  z.stream_bytes = stay;
  if (count != (R ? (mcus + R - 1) / R : 1)) return done(RHCCQ_JPEG_BAD_RESTART, count);
  return done(RHCCQ_JPEG_OK, 0);
}

// ---- the serial forms ----------------------------------------------------------------------------------------------------------------
inline void unstuff_serial(const uint8_t* f, int64_t n, const rhccq_jpeg_info& info, uint8_t* stream) {
  int64_t at = 0;
  for (int64_t i = info.scan_offset; i < info.scan_offset + info.scan_bytes; ++i)
    if (kept(f, n, info.scan_offset, i) && at < info.stream_bytes) stream[at++] = f[i];
}
// the DC differences -> the DC values, in the scan's order
inline void dc_serial(const Geo& g, int16_t* coef) {
  for (int c = 0; c < g.n_comp; ++c) {
    const int nb = c == 0 && g.n_comp == 3 ? g.hs * g.vs : 1, b0 = g.n_comp == 1 ? 0 : c == 0 ? 0 : g.hs * g.vs + c - 1;
    int32_t pred = 0;
    for (int64_t mcu = 0; mcu < g.mcus; ++mcu)
      for (int j = 0; j < nb; ++j) {
        if (j == 0 && (g.R ? mcu % g.R == 0 : mcu == 0)) pred = 0;
        int16_t* dc = coef + 64 * block_at(g, mcu * g.bpm + b0 + j);
        pred = (int32_t)((uint32_t)pred + (uint32_t)(int32_t)*dc);
        *dc = (int16_t)pred;
      }
  }
}
inline void planes_serial(const Geo& g, const rhccq_jpeg_tables& T, const int16_t* coef, uint8_t* planes) {
  for (int c = 0; c < g.n_comp; ++c)
    for (int64_t blk = 0; blk < (int64_t)g.bw[c] * g.bh[c]; ++blk) {
      int32_t ws[8][8], row[8];
      for (int col = 0; col < 8; ++col) {
        int32_t y[8];
        idct_column(coef + 64 * (g.base[c] + blk), T.quant[c], col, y);
        for (int r = 0; r < 8; ++r) ws[r][col] = y[r];
      }
      const int64_t by = blk / g.bw[c], bx = blk % g.bw[c];
      for (int r = 0; r < 8; ++r) {
        for (int col = 0; col < 8; ++col) row[col] = ws[r][col];
        idct_row(row, planes + 64 * g.base[c] + (8 * by + r) * (8 * (int64_t)g.bw[c]) + 8 * bx);
      }
    }
}
inline void rgb_serial(const Geo& g, const uint8_t* planes, uint8_t* rgb) {
  for (int y = 0; y < g.H; ++y)
    for (int x = 0; x < g.W; ++x) rgb_at(g, planes, y, x, rgb + 3 * ((int64_t)y * g.W + x));
}

// ---- what the kernels of jpeg_read.hip and jpeg_batch.hip share ----------------------------------------------------------------------
// the DC tiles of all components
inline int64_t dc_tiles(const Geo& g) {
  int64_t t = 0;
  for (int c = 0; c < g.n_comp; ++c) t += (g.mcus * (c == 0 && g.n_comp == 3 ? g.hs * g.vs : 1) + kThreads - 1) / kThreads;
  return t;
}

#if defined(__HIPCC__)
// what the sync launch records of a subsequence
struct SubRow {
  uint64_t entry, leave;
  uint32_t count, pad;
};

constexpr int kIdctBlocks = kThreads / 8;                   // blocks of a workgroup of the idct launch: eight lanes a block

// ---- sums that restart ---------------------------------------------------------------------------------------------------------------
// an element is flag << 32 | value; a flagged one restarts the sum.  (a then b) -> b if b is flagged, else a's flag and both values' sum
__device__ __forceinline__ uint64_t seg_combine(uint64_t a, uint64_t b) {
  return b >> 32 ? b : (a & 0xFFFFFFFF00000000ull) | (uint32_t)((uint32_t)a + (uint32_t)b);
}
// inclusive over the workgroup's kThreads lanes; s_w: kThreads / 64 words; *total: all of them
__device__ __forceinline__ uint64_t seg_block_scan(uint64_t x, uint64_t* s_w, uint64_t* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint64_t t = __shfl_up((unsigned long long)x, o, 64);
    if (lane >= o) x = seg_combine(t, x);
  }
  __syncthreads();                                                   // (the words' last readers are done)
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

__device__ __forceinline__ void tables_to_lds(rhccq_jpeg_tables* dst, const rhccq_jpeg_tables* __restrict__ src) {
  for (int i = threadIdx.x; i < (int)(sizeof(rhccq_jpeg_tables) / 4); i += kThreads) ((uint32_t*)dst)[i] = ((const uint32_t*)src)[i];
  __syncthreads();
}
__device__ __forceinline__ long long sub_end(const Dec& d, int S, long long g) {
  const long long e = (g + 1) * S;
  return e < d.total_bits ? e : d.total_bits;
}

// a component's blocks in decode order: nb of them an MCU, the MCU's blocks b0 ..
struct DcSeq { int nb, b0; long long len, tiles; };
__device__ __forceinline__ DcSeq dc_seq(const Geo& g, int c) {
  DcSeq s;
  s.nb = c == 0 && g.n_comp == 3 ? g.hs * g.vs : 1;
  s.b0 = c == 0 ? 0 : g.hs * g.vs + c - 1;
  s.len = g.mcus * s.nb;
  s.tiles = (s.len + kThreads - 1) / kThreads;
  return s;
}
#endif

}  // namespace jpegr
}  // namespace rhccq
