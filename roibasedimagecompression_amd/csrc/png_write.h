// PNG writing (EXTENSION, include/rhccq.h "indexed PNG files on the device"): the functions the device kernels of png_write.hip and the
// serial host twins share.  Plain C++ over <stdint.h>: a host-only program may include this file without the HIP headers.
//   scanlines   png_depth / png_row_bytes / png_index / png_packed_byte (colour type 3) and png_rgb / png_filter / png_cost / png_best
//               (colour type 2: the five row filters and the minimum-sum-of-absolute-differences rule, ties to the lowest type);
//   CRC-32      the reflected polynomial 0xEDB88320 in zlib's crc32_combine algebra.  A piece's PLAIN remainder r(M) = M(x) x^32 mod P
//               (register 0 at the start, no final inversion) obeys r(A || B) = r(A) x^(8 |B|) + r(B), zero bytes in front of a piece
//               change nothing, and the standard CRC of n bytes is 0xFFFFFFFF x^(8 n) + r(M) + 0xFFFFFFFF.  x is invertible modulo P
//               (P is primitive: x^(2^32 - 1) = 1), so zero bytes BEHIND a message are taken off again by x^(-8 z).
#pragma once
#include <stdint.h>

#include "../../include/rhccq.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RHCCQ_PNG_HD __host__ __device__ __forceinline__
#else
#define RHCCQ_PNG_HD inline
#endif

namespace rhccq {
namespace png {

// ---- the file's geometry -------------------------------------------------------------------------------------------------------------
constexpr int kMaxRows = 65536;                            // palette rows
constexpr int kFlagsAll = RHCCQ_PNG_EXACT | RHCCQ_PNG_DEPTH8 | RHCCQ_PNG_NO_FILTER;

RHCCQ_PNG_HD bool png_indexed(int K) { return K <= 256; }
RHCCQ_PNG_HD int png_depth(int K, int flags) {
  if (K > 16 || (flags & RHCCQ_PNG_DEPTH8)) return 8;
  return K <= 2 ? 1 : K <= 4 ? 2 : 4;
}
// bytes of one scanline, the filter byte included
RHCCQ_PNG_HD int64_t png_row_bytes(int W, int K, int flags) {
  return png_indexed(K) ? 1 + ((int64_t)W * png_depth(K, flags) + 7) / 8 : 1 + 3 * (int64_t)W;
}
// signature + IHDR + PLTE: where IDAT's length field starts
RHCCQ_PNG_HD int64_t png_idat_offset(int K) { return 8 + 25 + (png_indexed(K) ? 12 + 3 * (int64_t)K : 0); }

// ---- colour type 3 -------------------------------------------------------------------------------------------------------------------
// the index a decoder shows: one past the palette is row 0 (int16 / int32 storage is read as unsigned)
template <typename IdxT>
RHCCQ_PNG_HD uint32_t png_index(const IdxT* idx, int64_t p, uint32_t K) {
  const uint32_t v = (uint32_t)idx[p];
  return v < K ? v : 0u;
}
// byte c (behind the filter byte) of the row whose first pixel is idx[row0]: 8 / d pixels, most significant bits first, zero past W
template <typename IdxT>
RHCCQ_PNG_HD uint32_t png_packed_byte(const IdxT* idx, int64_t row0, int W, uint32_t K, int d, int64_t c) {
  if (d == 8) return png_index(idx, row0 + c, K);
  const int ppb = 8 / d;
  const int64_t x0 = c * ppb;
  uint32_t b = 0;
  for (int j = 0; j < ppb; ++j) {
    b <<= d;
    if (x0 + j < W) b |= png_index(idx, row0 + x0 + j, K);
  }
  return b;
}

// ---- colour type 2 -------------------------------------------------------------------------------------------------------------------
// a palette row as R | G << 8 | B << 16
RHCCQ_PNG_HD uint32_t png_rgb(const uint8_t* pal, uint32_t row) {
  const uint8_t* p = pal + 3 * (int64_t)row;
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}
RHCCQ_PNG_HD int png_paeth(int a, int b, int c) {
  const int p = a + b - c;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
  if (pa <= pb && pa <= pc) return a;
  if (pb <= pc) return b;
  return c;
}
// the filtered byte of x under filter type t with a = left, b = above, c = upper left
RHCCQ_PNG_HD uint32_t png_filter(int t, int x, int a, int b, int c) {
  const int pred = t == 0 ? 0 : t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
  return (uint32_t)(x - pred) & 255u;
}
RHCCQ_PNG_HD uint32_t png_cost(uint32_t v) { return v < 128u ? v : 256u - v; }
// adds the five costs of one pixel (packed as png_rgb packs them) to cost[5]
RHCCQ_PNG_HD void png_pixel_costs(uint32_t x, uint32_t a, uint32_t b, uint32_t c, uint32_t* cost) {
  for (int ch = 0; ch < 24; ch += 8) {
    const int xv = (x >> ch) & 255, av = (a >> ch) & 255, bv = (b >> ch) & 255, cv = (c >> ch) & 255;
    for (int t = 0; t < 5; ++t) cost[t] += png_cost(png_filter(t, xv, av, bv, cv));
  }
}
// the filter type of the smallest cost; a tie goes to the lowest type
RHCCQ_PNG_HD int png_best(const uint64_t* cost) {
  int best = 0;
  for (int t = 1; t < 5; ++t)
    if (cost[t] < cost[best]) best = t;
  return best;
}

// ---- CRC-32 --------------------------------------------------------------------------------------------------------------------------
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr int kCrcLane = 64;                               // bytes a lane takes
constexpr int kCrcBlock = 256;                             // lanes of a workgroup
constexpr int kCrcWave = kCrcLane * 64;                    // bytes a wave takes
constexpr int kCrcPiece = kCrcLane * kCrcBlock;            // bytes a workgroup takes: one partial remainder
constexpr uint32_t kCrcOne = 0x80000000u;                  // the polynomial 1 (bit 31 is x^0)
constexpr uint64_t kCrcOrder = 0xFFFFFFFFull;              // x^(2^32 - 1) = 1

// c(x) x^8 mod P
RHCCQ_PNG_HD uint32_t crc_shift8(uint32_t c) {
  for (int i = 0; i < 8; ++i) c = (c >> 1) ^ (kCrcPoly & (0u - (c & 1u)));
  return c;
}
// the register after one more byte
RHCCQ_PNG_HD uint32_t crc_byte(uint32_t c, uint32_t b) { return crc_shift8(c ^ b); }
// a(x) b(x) mod P (zlib's multmodp without its early exit)
RHCCQ_PNG_HD uint32_t crc_mul(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (int i = 0; i < 32; ++i) {
    p ^= b & (0u - (a >> 31));
    a <<= 1;
    b = (b >> 1) ^ (kCrcPoly & (0u - (b & 1u)));
  }
  return p;
}

// what the host works out once per call and the kernels take by value
struct CrcConsts {
  uint32_t x2n[32];   // x^(2^k)
  uint32_t lane[6];   // x^(8 kCrcLane 2^j): joins 2^j lanes' bytes to the 2^j lanes in front of them
  uint32_t wave;      // x^(8 kCrcWave)
  uint32_t piece;     // x^(8 kCrcPiece)
  uint32_t seg[8];    // x^(8 kCrcPiece S 2^j): the combining workgroup's tree over lanes that folded S partials each
};

inline void crc_x2n(uint32_t* x2n) {
  uint32_t p = kCrcOne >> 1;                               // x^1
  x2n[0] = p;
  for (int k = 1; k < 32; ++k) x2n[k] = p = crc_mul(p, p);
}
// x^e mod P (zlib's x2nmodp: the table wraps because x^(2^32) = x)
RHCCQ_PNG_HD uint32_t crc_xpow(const uint32_t* x2n, uint64_t e) {
  uint32_t p = kCrcOne;
  for (int k = 0; e; e >>= 1, ++k)
    if (e & 1) p = crc_mul(x2n[k & 31], p);
  return p;
}
inline CrcConsts crc_consts(int64_t seg_pieces) {
  CrcConsts c;
  crc_x2n(c.x2n);
  for (int j = 0; j < 6; ++j) c.lane[j] = crc_xpow(c.x2n, 8ull * kCrcLane << j);
  c.wave = crc_xpow(c.x2n, 8ull * kCrcWave);
  c.piece = crc_xpow(c.x2n, 8ull * kCrcPiece);
  c.seg[0] = crc_xpow(c.x2n, 8ull * kCrcPiece * (uint64_t)seg_pieces);
  for (int j = 1; j < 8; ++j) c.seg[j] = crc_mul(c.seg[j - 1], c.seg[j - 1]);
  return c;
}
// pieces of kCrcPiece bytes that cover `front` zero bytes and n bytes behind them
RHCCQ_PNG_HD int64_t crc_pieces(int64_t front, int64_t n) { return (front + n + kCrcPiece - 1) / kCrcPiece; }

// the serial form: plain remainders of kCrcPiece-byte pieces joined by the same algebra (the last piece may be short)
inline uint32_t crc32_serial(const uint8_t* data, int64_t n) {
  uint32_t table[256], x2n[32];
  for (uint32_t i = 0; i < 256; ++i) table[i] = crc_shift8(i);
  crc_x2n(x2n);
  const uint32_t full = crc_xpow(x2n, 8ull * kCrcPiece);
  uint32_t r = 0;
  for (int64_t s = 0; s < n; s += kCrcPiece) {
    const int64_t len = n - s < kCrcPiece ? n - s : kCrcPiece;
    uint32_t c = 0;
    for (int64_t i = 0; i < len; ++i) c = table[(c ^ data[s + i]) & 255u] ^ (c >> 8);
    r = crc_mul(r, len == kCrcPiece ? full : crc_xpow(x2n, 8ull * (uint64_t)len)) ^ c;
  }
  return crc_mul(0xFFFFFFFFu, crc_xpow(x2n, 8ull * (uint64_t)n)) ^ r ^ 0xFFFFFFFFu;
}
// the register (before the final inversion) after `n` more bytes, from the register `state` in front of them
inline uint32_t crc_state(uint32_t state, const uint8_t* data, int64_t n) {
  for (int64_t i = 0; i < n; ++i) state = crc_byte(state, data[i]);
  return state;
}

#if defined(__HIPCC__)
// ---- CRC-32 on the device: what the kernels of png_write.hip and png_read.hip share ---------------------------------------------------
// the bytes lo .. hi - 1 (of 0..3) of a word kept, the others zero
__device__ __forceinline__ uint32_t crc_keep(uint32_t w, long long lo, long long hi) {
  const int l = lo < 0 ? 0 : lo > 4 ? 4 : (int)lo, h = hi < 0 ? 0 : hi > 4 ? 4 : (int)hi;
  if (h <= l) return 0u;
  const uint32_t mh = h == 4 ? 0xFFFFFFFFu : (1u << (8 * h)) - 1u, ml = (1u << (8 * l)) - 1u;   // l < 4 here
  return w & mh & ~ml;
}

struct CrcPieceLds {
  uint32_t tab[4][256];
  uint4 data[kCrcBlock / 64][64 * 5];                                // a lane's 64 bytes in an 80-byte strip
  uint32_t wave[kCrcBlock / 64];
};

// a workgroup of kCrcBlock lanes: the plain remainder of the piece that starts at the virtual byte v0 of the string at base (aligned to 16),
// of which the bytes front .. end - 1 are the message and all others count as zero; v0 < end.  Valid in thread 0; two barriers.
__device__ __forceinline__ uint32_t crc_piece_remainder(CrcPieceLds& lds, const uint8_t* __restrict__ base, long long front, long long end, long long v0,
                                                        const CrcConsts& k) {
  {
    uint32_t c = threadIdx.x;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      c = crc_shift8(c);
      lds.tab[t][threadIdx.x] = c;                                     // byte, then t zero bytes
    }
  }
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int u = lane + 64 * j;
    const long long v = v0 + (long long)w * kCrcWave + 16 * u;
    uint4 x = make_uint4(0u, 0u, 0u, 0u);
    if (v + 16 > front && v < end) {
      x = *(const uint4*)(base + v);
      if (v < front || v + 16 > end) {
        x.x = crc_keep(x.x, front - v, end - v);
        x.y = crc_keep(x.y, front - v - 4, end - v - 4);
        x.z = crc_keep(x.z, front - v - 8, end - v - 8);
        x.w = crc_keep(x.w, front - v - 12, end - v - 12);
      }
    }
    lds.data[w][(u >> 2) * 5 + (u & 3)] = x;
  }
  __syncthreads();
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint4 x = lds.data[w][lane * 5 + j];
    const uint32_t q[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c ^= q[i];
      c = lds.tab[3][c & 255u] ^ lds.tab[2][(c >> 8) & 255u] ^ lds.tab[1][(c >> 16) & 255u] ^ lds.tab[0][c >> 24];
    }
  }
#pragma unroll
  for (int j = 0; j < 6; ++j) {                                      // lane i takes in the 2^j lanes behind it
    const uint32_t right = __shfl_down(c, 1 << j, 64);
    c = crc_mul(c, k.lane[j]) ^ right;
  }
  if (lane == 0) lds.wave[w] = c;
  __syncthreads();
  uint32_t r = 0;
  if (threadIdx.x == 0) {
    r = lds.wave[0];
    for (int i = 1; i < kCrcBlock / 64; ++i) r = crc_mul(r, k.wave) ^ lds.wave[i];
  }
  return r;
}
#endif

// ---- chunk framing the host knows in full --------------------------------------------------------------------------------------------
inline void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v;
}
constexpr int kHeadBytes = 33;                             // signature + IHDR
struct Head { uint8_t b[kHeadBytes + 3]; };
inline Head png_head(int H, int W, int K, int flags) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  Head h{};
  for (int i = 0; i < 8; ++i) h.b[i] = sig[i];
  uint8_t* c = h.b + 8;
  put_be32(c, 13);
  c[4] = 'I'; c[5] = 'H'; c[6] = 'D'; c[7] = 'R';
  put_be32(c + 8, (uint32_t)W);
  put_be32(c + 12, (uint32_t)H);
  c[16] = (uint8_t)(png_indexed(K) ? png_depth(K, flags) : 8);
  c[17] = (uint8_t)(png_indexed(K) ? 3 : 2);
  c[18] = c[19] = c[20] = 0;
  put_be32(c + 21, crc_state(0xFFFFFFFFu, c + 4, 17) ^ 0xFFFFFFFFu);
  return h;
}
static const uint8_t kIend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};

}  // namespace png
}  // namespace rhccq
