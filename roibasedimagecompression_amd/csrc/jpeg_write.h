// JPEG writing (EXTENSION, include/rhccq.h "JPEG files written on the device"): the functions the kernels of jpeg_write.hip and the serial
// host forms share.  Plain C++ over <stdint.h>: a host-only program may include this file without the HIP headers.
//   frame      args_ok, frame_of: the planes of whole MCUs (jpeg_read.h's Geo), the first component's true size in blocks, the intervals;
//   tables     quant_tables, tables_build: the divisors, the Annex K codes as code / length per symbol, the file's header;
//   blocks     ycc, sample_at (edge replication, chroma downsampling), fdct8 (one pass of the islow FDCT), quantise, dummy_source;
//   entropy    dc_pred, lane_sym, lane_symbol: what one zig-zag position of one block puts into the scan (the symbol; its code and bits);
//   serial     blocks_serial, encode_serial: the host forms.
#pragma once
#include "jpeg_read.h"

namespace rhccq {
namespace jpegw {

using jpegr::block_at;
using jpegr::bswap;
using jpegr::comp_of;
using jpegr::Geo;
using jpegr::zigzag;

constexpr int kThreads = 256;
constexpr int kPackBlocks = 32;                            // blocks of a workgroup of the count and pack launches: 8 a wave
constexpr int kBlockBits = 20 + 63 * 26;                   // the most a block takes: a DC code of 9 bits and 11 value bits, 63 codes of 16 and 10
constexpr int kBlockBitsOpt = 23 + 63 * 26;                // with tables made for the picture (jpeg_optimize.h): a DC code of 12 bits
constexpr int window_words(int block_bits) { return (kPackBlocks * (block_bits + 7) + 31) / 32 + 2; }
constexpr int kWindowWords = window_words(kBlockBits);     // LDS words of a pack workgroup, pads and both ragged ends included
constexpr int kTileBytes = 16 * kThreads;                  // stream bytes of a workgroup of the stuff launches
constexpr int kHeaderMax = 640;                            // SOI .. SOS is 623 bytes at most (colour, with DRI)
constexpr int kStripPx = 128;                              // the widest strip of the blocks launch in pixels of a colour frame (grey: 256)
constexpr int kRowBytes = 3 * kStripPx + 32;               // LDS bytes of a staged row: the strip's bytes and the ragged 16-byte ends
constexpr int64_t kFileMax = ((int64_t)1 << 31) - 1;

// Annex K, in natural order
static constexpr uint8_t kBaseQ[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};
static constexpr uint8_t kDcBits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
static constexpr uint8_t kAcBits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
static constexpr uint8_t kAcVals[2][162] = {
    {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,  66,  177,
     193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,  52,  53,  54,  55,
     56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105, 106,
     115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163,
     164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211,
     212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
    {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161, 177, 193,
     9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,  41,  42,  53,  54,
     55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100, 101, 102, 103, 104, 105,
     106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154,
     162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202,
     210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};

// ---- frame ---------------------------------------------------------------------------------------------------------------------------
struct Frame {
  Geo g;                                                   // the planes of whole MCUs, g.R the restart interval in MCUs
  int32_t wib, hib;                                        // the first component's true size in blocks: what lies outside is dummy
  int64_t n_iv;
};
RHCCQ_JPEG_HD bool args_ok(int32_t H, int32_t W, int32_t mode, int32_t quality, int32_t restart_rows) {
  return H >= 1 && H <= 65535 && W >= 1 && W <= 65535 && mode >= RHCCQ_JPEG_GREY && mode <= RHCCQ_JPEG_420 && quality >= 1 && quality <= 100 && restart_rows >= 0;
}
RHCCQ_JPEG_HD Frame frame_of(int32_t H, int32_t W, int32_t mode, int32_t restart_rows) {
  rhccq_jpeg_info i{};
  i.width = W, i.height = H;
  i.n_comp = mode == RHCCQ_JPEG_GREY ? 1 : 3;
  i.hs = mode >= RHCCQ_JPEG_422 ? 2 : 1;
  i.vs = mode == RHCCQ_JPEG_420 ? 2 : 1;
  i.mcus_x = (W + 8 * i.hs - 1) / (8 * i.hs);
  i.mcus_y = (H + 8 * i.vs - 1) / (8 * i.vs);
  i.blocks_per_mcu = i.n_comp == 1 ? 1 : i.hs * i.vs + 2;
  const int64_t nominal = (int64_t)restart_rows * i.mcus_x;   // (libjpeg: rows of MCUs, at most 65535 MCUs)
  i.restart_interval = (int32_t)(nominal > 65535 ? 65535 : nominal);
  Frame f;
  f.g = jpegr::geo_of(i);
  f.wib = (W + 7) / 8, f.hib = (H + 7) / 8;
  f.n_iv = f.g.R ? (f.g.mcus + f.g.R - 1) / f.g.R : 1;
  return f;
}
RHCCQ_JPEG_HD int64_t interval_of(const Geo& g, int64_t A) { return g.R ? A / g.bpm / g.R : 0; }
RHCCQ_JPEG_HD bool starts_interval(const Geo& g, int64_t A) { return g.R ? A % ((int64_t)g.bpm * g.R) == 0 : A == 0; }
RHCCQ_JPEG_HD bool ends_interval(const Geo& g, int64_t A) { return A + 1 == g.blocks || starts_interval(g, A + 1); }
// the most bytes of the unstuffed stream, and of the file
RHCCQ_JPEG_HD int64_t stream_cap(const Frame& f, int block_bits = kBlockBits) { return (f.g.blocks * block_bits + 7) / 8 + f.n_iv; }
RHCCQ_JPEG_HD int64_t file_cap(const Frame& f, int block_bits = kBlockBits) { return kHeaderMax + 2 * stream_cap(f, block_bits) + 2 * f.n_iv + 2; }

// ---- tables --------------------------------------------------------------------------------------------------------------------------
// what the kernels read: table t of code / len is DC0, AC0, DC1, AC1; component c codes with tables 2 (c > 0) and 2 (c > 0) + 1
struct Tables {
  uint16_t div[3][64];                                     // 8 Q per component, natural order
  uint16_t code[4][256];
  uint8_t len[4][256];
  int32_t header_len, pad;
  uint8_t header[kHeaderMax];
};
inline void quant_tables(int quality, uint8_t q[2][64]) {
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 64; ++i) {
      const int v = (kBaseQ[t][i] * scale + 50) / 100;
      q[t][i] = (uint8_t)(v < 1 ? 1 : v > 255 ? 255 : v);
    }
}
inline void tables_build(const Frame& f, int quality, Tables* T) {
  memset(T, 0, sizeof *T);
  uint8_t q[2][64];
  quant_tables(quality, q);
  for (int c = 0; c < 3; ++c)
    for (int i = 0; i < 64; ++i) T->div[c][i] = (uint16_t)(8 * q[c ? 1 : 0][i]);
  for (int t = 0; t < 4; ++t) {
    const uint8_t* bits = t & 1 ? kAcBits[t >> 1] : kDcBits[t >> 1];
    int code = 0, at = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++at, ++code) {
        const int sym = t & 1 ? kAcVals[t >> 1][at] : at;
        T->code[t][sym] = (uint16_t)code;
        T->len[t][sym] = (uint8_t)l;
      }
      code <<= 1;
    }
  }
  const Geo& g = f.g;
  const int nt = g.n_comp == 1 ? 1 : 2;
  uint8_t* h = T->header;
  int n = 0;
  auto put = [&](int v) { h[n++] = (uint8_t)v; };
  auto put16 = [&](int v) { put(v >> 8), put(v & 255); };
  put16(0xFFD8);
  put16(0xFFE0), put16(16);
  for (const char* s = "JFIF"; *s; ++s) put(*s);
  put(0), put16(0x0101), put(0), put16(1), put16(1), put16(0);
  for (int t = 0; t < nt; ++t) {
    put16(0xFFDB), put16(67), put(t);
    for (int i = 0; i < 64; ++i) put(q[t][zigzag(i)]);
  }
  put16(0xFFC0), put16(8 + 3 * g.n_comp), put(8), put16(g.H), put16(g.W), put(g.n_comp);
  for (int c = 0; c < g.n_comp; ++c) put(c + 1), put(c == 0 ? g.hs << 4 | g.vs : 0x11), put(c ? 1 : 0);
  for (int t = 0; t < 2 * nt; ++t) {
    const uint8_t* bits = t & 1 ? kAcBits[t >> 1] : kDcBits[t >> 1];
    const int count = t & 1 ? 162 : 12;
    put16(0xFFC4), put16(19 + count), put((t & 1) << 4 | t >> 1);
    for (int i = 0; i < 16; ++i) put(bits[i]);
    for (int i = 0; i < count; ++i) put(t & 1 ? kAcVals[t >> 1][i] : i);
  }
  if (g.R) put16(0xFFDD), put16(4), put16(g.R);
  put16(0xFFDA), put16(6 + 2 * g.n_comp), put(g.n_comp);
  for (int c = 0; c < g.n_comp; ++c) put(c + 1), put(c ? 0x11 : 0);
  put(0), put(63), put(0);
  T->header_len = n;
}

// ---- blocks --------------------------------------------------------------------------------------------------------------------------
// jccolor.c
RHCCQ_JPEG_HD void ycc(int32_t r, int32_t g, int32_t b, int32_t* y, int32_t* cb, int32_t* cr) {
  *y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  *cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  *cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}
// the sample of component c at (y, x) of its plane; px(y, x, channel) reads a pixel inside the image.  The image's last column and row
// are replicated, then chroma is averaged over 2 x 1 or 2 x 2 converted samples with jcsample.c's alternating bias
template <class Px>
RHCCQ_JPEG_HD int32_t sample_at(const Px& px, const Geo& g, int c, int y, int x) {
  const int hs = c ? g.hs : 1, vs = c ? g.vs : 1;
  if (vs == 2 && y > (g.H - 1) / 2) y = (g.H - 1) / 2;     // (below the image the component's own last row is repeated, not the image's)
  int32_t sum = 0;
  for (int dy = 0; dy < vs; ++dy)
    for (int dx = 0; dx < hs; ++dx) {
      const int yy = vs * y + dy < g.H ? vs * y + dy : g.H - 1, xx = hs * x + dx < g.W ? hs * x + dx : g.W - 1;
      if (g.n_comp == 1) return px(yy, xx, 0);
      int32_t v[3];
      ycc(px(yy, xx, 0), px(yy, xx, 1), px(yy, xx, 2), &v[0], &v[1], &v[2]);
      sum += v[c];
    }
  if (hs == 1) return sum;
  return vs == 1 ? (sum + (x & 1)) >> 1 : (sum + 1 + (x & 1)) >> 2;
}
// one pass of jfdctint.c's jpeg_fdct_islow over eight values: rows first (the sums scaled by 4), then columns
RHCCQ_JPEG_HD void fdct8(const int32_t* d, bool rows, int32_t* o) {
  const int32_t t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
  const int32_t t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
  const int32_t t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  const int sh = rows ? 11 : 15;
  const int32_t r = 1 << (sh - 1);
  o[0] = rows ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  o[4] = rows ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  int32_t z1 = (t12 + t13) * 4433;
  o[2] = (z1 + t13 * 6270 + r) >> sh;
  o[6] = (z1 - t12 * 15137 + r) >> sh;
  z1 = t4 + t7;
  int32_t z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int32_t z5 = (z3 + z4) * 9633;
  const int32_t a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  o[7] = (a4 + z1 + z3 + r) >> sh;
  o[5] = (a5 + z2 + z4 + r) >> sh;
  o[3] = (a6 + z2 + z3 + r) >> sh;
  o[1] = (a7 + z1 + z4 + r) >> sh;
}
// jcdctmgr.c: the transform's output is scaled by 8, so is the divisor
RHCCQ_JPEG_HD int16_t quantise(int32_t c, int32_t div) {
  const int32_t a = ((c < 0 ? -c : c) + (div >> 1)) / div;
  return (int16_t)(c < 0 ? -a : a);
}
// is block (by, bx) of the first component's plane a dummy block of libjpeg's coefficient controller?  Then (*sy, *sx) is the block whose
// DC it repeats: its left neighbour, or, for a row below the image, the upper right block of its MCU (or that one's left neighbour)
RHCCQ_JPEG_HD bool dummy_source(const Frame& f, int by, int bx, int* sy, int* sx) {
  if (by < f.hib && bx < f.wib) return false;
  if (by < f.hib) {
    *sy = by, *sx = bx - 1;
    return true;
  }
  const int right = bx | (f.g.hs - 1);
  *sy = by - 1, *sx = right < f.wib ? right : right - 1;
  return true;
}
// the quantised coefficients of one real block of component c, natural order
template <class Px>
RHCCQ_JPEG_HD void block_of(const Px& px, const Geo& g, const uint16_t* div, int c, int by, int bx, int16_t* out) {
  int32_t ws[8][8];
  for (int r = 0; r < 8; ++r) {
    int32_t d[8];
    for (int k = 0; k < 8; ++k) d[k] = sample_at(px, g, c, 8 * by + r, 8 * bx + k) - 128;
    fdct8(d, true, ws[r]);
  }
  for (int k = 0; k < 8; ++k) {
    int32_t d[8], o[8];
    for (int r = 0; r < 8; ++r) d[r] = ws[r][k];
    fdct8(d, false, o);
    for (int r = 0; r < 8; ++r) out[8 * r + k] = quantise(o[r], div[8 * r + k]);
  }
}

// ---- entropy -------------------------------------------------------------------------------------------------------------------------
RHCCQ_JPEG_HD int bit_size(int32_t v) {
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
#if defined(__HIP_DEVICE_COMPILE__)
  return 32 - __clz((int)a);
#else
  return a ? 32 - __builtin_clz(a) : 0;
#endif
}
RHCCQ_JPEG_HD int top_bit(uint64_t m) {                    // m != 0
#if defined(__HIP_DEVICE_COMPILE__)
  return 63 - __clzll((long long)m);
#else
  return 63 - __builtin_clzll(m);
#endif
}
// the DC the difference of block A (scan order) is taken against: the component's previous block of the scan, 0 at an interval's start
RHCCQ_JPEG_HD int32_t dc_pred(const Geo& g, const int16_t* coef, int64_t A) {
  const int64_t mcu = A / g.bpm;
  const int b = (int)(A - mcu * g.bpm), ny = g.n_comp == 1 ? 1 : g.hs * g.vs;
  if (b > 0 && b < ny) return coef[64 * block_at(g, A - 1)];
  if (g.R ? mcu % g.R == 0 : mcu == 0) return 0;
  return coef[64 * block_at(g, b == 0 ? (mcu - 1) * g.bpm + ny - 1 : A - g.bpm)];
}
// What zig-zag position k of a block puts into the scan.  v: the coefficient there (k = 0: the DC difference); mask: bit j set where
// position j >= 1 holds a non-zero coefficient.  -> the symbol (-1: none), its value bits' count, and the number of ZRL codes in front.
// Position 63 carries EOB when its coefficient is 0.
struct LaneSym {
  int32_t sym, s, zrl;
};
RHCCQ_JPEG_HD LaneSym lane_sym(int k, int32_t v, uint64_t mask) {
  LaneSym o{-1, 0, 0};
  if (k == 0) {
    o.sym = o.s = bit_size(v);
  } else if (v != 0) {
    const uint64_t below = mask & (((uint64_t)1 << k) - 2);
    const int run = k - 1 - (below ? top_bit(below) : 0);
    o.zrl = run >> 4;
    o.s = bit_size(v);
    o.sym = (run & 15) << 4 | o.s;
  } else if (k == 63) {
    o.sym = 0;
  }
  return o;
}
// code, len: the component's DC table and, 256 entries on, its AC table.  -> the number of ZRL codes in front, then `n` bits `bits` (the
// code and the value bits)
struct LaneBits {
  uint32_t bits;
  int32_t n, zrl;
};
RHCCQ_JPEG_HD LaneBits lane_symbol(const uint16_t* code, const uint8_t* len, int k, int32_t v, uint64_t mask) {
  const LaneSym y = lane_sym(k, v, mask);
  LaneBits o{0u, 0, y.zrl};
  if (y.sym < 0) return o;
  const int at = (k ? 256 : 0) + y.sym;
  const uint32_t value = (uint32_t)(v < 0 ? v - 1 : v) & (((uint32_t)1 << y.s) - 1);
  o.bits = (uint32_t)code[at] << y.s | value;
  o.n = len[at] + y.s;
  return o;
}
RHCCQ_JPEG_HD int lane_length(const LaneBits& b, const uint8_t* len) { return b.zrl * len[256 + 0xF0] + b.n; }

// ---- the serial forms ----------------------------------------------------------------------------------------------------------------
struct HostPx {
  const uint8_t* img;
  int64_t W;
  int C;
  int32_t operator()(int y, int x, int ch) const { return img[(y * W + x) * C + ch]; }
};
inline void blocks_serial(const Frame& f, const Tables& T, const uint8_t* img, int16_t* coef) {
  const Geo& g = f.g;
  const HostPx px{img, g.W, g.n_comp};
  for (int c = 0; c < g.n_comp; ++c)
    for (int by = 0; by < g.bh[c]; ++by)
      for (int bx = 0; bx < g.bw[c]; ++bx) {
        int sy, sx;
        int16_t* out = coef + 64 * (g.base[c] + (int64_t)by * g.bw[c] + bx);
        if (c == 0 && dummy_source(f, by, bx, &sy, &sx)) memset(out, 0, 128);
        else block_of(px, g, T.div[c], c, by, bx, out);
      }
  for (int by = 0; by < g.bh[0]; ++by)                      // (a dummy block's source is a real block)
    for (int bx = 0; bx < g.bw[0]; ++bx) {
      int sy, sx;
      if (dummy_source(f, by, bx, &sy, &sx)) coef[64 * ((int64_t)by * g.bw[0] + bx)] = coef[64 * ((int64_t)sy * g.bw[0] + sx)];
    }
}
// header, scan and EOI into out[cap] -> the file's length, -1 where cap is too small
inline int64_t encode_serial(const Frame& f, const Tables& T, const int16_t* coef, uint8_t* out, int64_t cap) {
  const Geo& g = f.g;
  int64_t n = 0;
  bool full = false;
  auto byte = [&](int v) {
    if (n < cap) out[n++] = (uint8_t)v;
    else full = true;
  };
  for (int i = 0; i < T.header_len; ++i) byte(T.header[i]);
  uint64_t acc = 0;
  int held = 0;
  auto bits = [&](uint32_t v, int count) {
    acc = acc << count | v;
    held += count;
    while (held >= 8) {
      const int b = (int)(acc >> (held - 8) & 255);
      byte(b);
      if (b == 255) byte(0);
      held -= 8;
    }
  };
  for (int64_t A = 0; A < g.blocks; ++A) {
    if (A && starts_interval(g, A)) byte(0xFF), byte(0xD0 + (int)((interval_of(g, A) - 1) & 7));
    const int c = comp_of(g, (int)(A % g.bpm)), t = c ? 2 : 0;
    const int16_t* blk = coef + 64 * block_at(g, A);
    uint64_t mask = 0;
    for (int k = 1; k < 64; ++k) mask |= (uint64_t)(blk[zigzag(k)] != 0) << k;
    for (int k = 0; k < 64; ++k) {
      const LaneBits b = lane_symbol(T.code[t], T.len[t], k, k ? blk[zigzag(k)] : blk[0] - dc_pred(g, coef, A), mask);
      for (int i = 0; i < b.zrl; ++i) bits(T.code[t + 1][0xF0], T.len[t + 1][0xF0]);
      if (b.n) bits(b.bits, b.n);
    }
    if (ends_interval(g, A) && held) bits((1u << (8 - held)) - 1, 8 - held);
  }
  byte(0xFF), byte(0xD9);
  return full ? -1 : n;
}

// ---- what jpeg_optimize.hip takes from jpeg_write.hip ---------------------------------------------------------------------------------
// the entropy stage sized for block_bits a block (kBlockBits or kBlockBitsOpt): its workspace's bytes, its launches
int64_t entropy_workspace(const Frame& f, int block_bits);
int entropy_launch(rhccq_ctx* ctx, const Frame& f, int block_bits, const Tables* tables_dev, const int16_t* coef, void* workspace, uint8_t* out, int64_t cap, int64_t* length);
int blocks_launch(rhccq_ctx* ctx, const Frame& f, const Tables* tables_dev, const uint8_t* img, int16_t* coef);

}  // namespace jpegw
}  // namespace rhccq
