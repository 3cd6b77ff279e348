// Indexed PNG files written on the device (EXTENSION, include/rhccq.h): scanline packing, the five row filters, a parallel CRC-32 and the
// chunk framing around the stream of rhccq_zlib_compress / rhccq_zlib9_compress.  The definitions both sides share are in png_write.h; the
// host forms at the end run them serially.
//
//   png_pack_kernel   colour type 3.  The scanlines are ONE byte string (every row is its filter byte and ceil(W d / 8) packed bytes), and
//                     a lane builds an aligned 4-byte word of it from up to 32 indices and stores it once: a wave's store is 256 contiguous
//                     bytes, its loads a contiguous run of the index map.  Row starts fall anywhere in a word (a row is one byte longer
//                     than its pixels), so a lane finds (row, byte) of its first byte by one 32-bit division and walks on from there; only
//                     the bytes in front of the first and behind the last whole word of a misaligned `scan` go bytewise.
//   png_rgb_kernel    colour type 2.  A workgroup per image row: pass 1 adds the five costs of the lane's pixels (the left and upper-left
//                     pixels are gathered again; they are the neighbours' cache lines), a wave reduction and one barrier pick the type,
//                     pass 2 reads the row again (it is in cache) and writes the filtered bytes.  Both passes are chains of dependent
//                     index -> palette loads, so the waves in flight decide: a wave per row (2 160 waves on a 4K frame) took 232 us, this 156 us.
//   crc_partials      a workgroup takes the plain remainder of a 16 KiB piece: the wave's 4 KiB come in as coalesced aligned 16-byte
//                     loads, go through LDS (80-byte strips: no bank conflict on the way back) so that a lane holds 64 contiguous bytes,
//                     slice-by-4 over tables in LDS, then six multiplications join the wave and three the workgroup.  Pieces are laid
//                     from the 16-byte aligned address at or below `data`: the bytes in front of data[0] are masked to zero (leading
//                     zeros do not change a plain remainder) and so are the bytes behind data[n).
//   crc_combine       ONE workgroup: a lane folds S consecutive partials (Horner), a tree of eight multiplications joins the 256 lanes,
//                     x^(-8 z) takes the z trailing zero bytes off and 0xFFFFFFFF x^(8 n) brings the standard start and end in.  The two
//                     powers are products of table entries, formed by 32 lanes each in five multiplications.
//   png_head_kernel / png_tail_kernel   the framing: what the host knows (signature, IHDR) comes by value, PLTE is copied from the device
//                     palette with its CRC formed by the same algebra (a lane per entry), the tail reads the stream's length and CRC.
#include "png_write.h"
#include "palette_remap.h"

#include <vector>

namespace rhccq {
namespace png {

constexpr int64_t kScanMax = ((int64_t)1 << 31) - 1;                 // the level-9 encoder's limit
constexpr int64_t kFastMax = ((int64_t)1 << 31) - (1 << 16) - 1;     // the fast encoder refuses n >= 2^31 - its block (65536 bytes)

// ---- colour type 3 -------------------------------------------------------------------------------------------------------------------
template <typename IdxT>
__global__ __launch_bounds__(256) void png_pack_kernel(const IdxT* __restrict__ idx, int H, int W, uint32_t K, int d, uint32_t rb, uint8_t* base,
                                                       int mis, uint32_t total, long long* __restrict__ filter_rows) {
  // word q = base[4 q .. 4 q + 3] holds the bytes 4 q - mis .. 4 q - mis + 3 of the scanlines; base = scan - mis is aligned to 4
  const long long nq = ((long long)mis + total + 3) >> 2;
  if (filter_rows && blockIdx.x == 0 && threadIdx.x < 5) filter_rows[threadIdx.x] = threadIdx.x == 0 ? H : 0;
  for (long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (long long)gridDim.x * blockDim.x) {
    const long long o0 = 4 * q - mis;
    const uint32_t first = o0 < 0 ? 0u : (uint32_t)o0;
    uint32_t y = first / rb, c = first - y * rb;
    uint32_t word = 0;
    int valid = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long o = o0 + j;
      if (o < 0 || o >= (long long)total) continue;
      const uint32_t b = c == 0 ? 0u : png_packed_byte(idx, (int64_t)y * W, W, K, d, (int64_t)c - 1);
      word |= b << (8 * j);
      valid |= 1 << j;
      if (++c == rb) {
        c = 0;
        ++y;
      }
    }
    if (valid == 15) {
      *(uint32_t*)(base + 4 * q) = word;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (valid >> j & 1) base[4 * q + j] = (uint8_t)(word >> (8 * j));
    }
  }
}

// ---- colour type 2 -------------------------------------------------------------------------------------------------------------------
constexpr int kRgbBlock = 256;                                       // lanes of a workgroup: one image row

template <typename IdxT>
__global__ __launch_bounds__(kRgbBlock) void png_rgb_kernel(const IdxT* __restrict__ idx, int W, const uint8_t* __restrict__ pal, uint32_t K, int no_filter,
                                                            uint8_t* __restrict__ scan, unsigned long long* __restrict__ filter_rows) {
  __shared__ unsigned long long s_cost[kRgbBlock / 64][5];
  const long long y = blockIdx.x;
  const int lane = threadIdx.x;
  const IdxT* cur = idx + y * W;
  const bool has_up = y > 0;
  int best = 0;
  if (!no_filter) {
    uint32_t cost[5] = {0, 0, 0, 0, 0};
    for (int x = lane; x < W; x += kRgbBlock) {
      const uint32_t px = png_rgb(pal, png_index(cur, x, K));
      const uint32_t a = x > 0 ? png_rgb(pal, png_index(cur, x - 1, K)) : 0u;
      const uint32_t b = has_up ? png_rgb(pal, png_index(cur, (int64_t)x - W, K)) : 0u;
      const uint32_t c = has_up && x > 0 ? png_rgb(pal, png_index(cur, (int64_t)x - 1 - W, K)) : 0u;
      png_pixel_costs(px, a, b, c, cost);
    }
    uint64_t tot[5];
#pragma unroll
    for (int t = 0; t < 5; ++t) tot[t] = wave_sum((unsigned long long)cost[t]);
    if ((lane & 63) == 0)
      for (int t = 0; t < 5; ++t) s_cost[lane >> 6][t] = tot[t];
    __syncthreads();                                                 // (no_filter is the launch's: every lane is here)
    for (int t = 0; t < 5; ++t) {
      tot[t] = 0;
      for (int w = 0; w < kRgbBlock / 64; ++w) tot[t] += s_cost[w][t];
    }
    best = png_best(tot);
  }
  uint8_t* row = scan + y * (1 + 3 * (long long)W);
  if (lane == 0) {
    row[0] = (uint8_t)best;
    if (filter_rows) atomicAdd(&filter_rows[best], 1ull);
  }
  for (int x = lane; x < W; x += kRgbBlock) {
    const uint32_t px = png_rgb(pal, png_index(cur, x, K));
    uint32_t a = 0, b = 0, c = 0;
    if (best == 1 || best >= 3) a = x > 0 ? png_rgb(pal, png_index(cur, x - 1, K)) : 0u;
    if (best >= 2) b = has_up ? png_rgb(pal, png_index(cur, (int64_t)x - W, K)) : 0u;
    if (best == 4) c = has_up && x > 0 ? png_rgb(pal, png_index(cur, (int64_t)x - 1 - W, K)) : 0u;
    uint8_t* o = row + 1 + 3 * (long long)x;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      o[ch] = (uint8_t)png_filter(best, (px >> (8 * ch)) & 255, (a >> (8 * ch)) & 255, (b >> (8 * ch)) & 255, (c >> (8 * ch)) & 255);
  }
}

// ---- CRC-32 --------------------------------------------------------------------------------------------------------------------------
// the message's length on the device: *n_dev + n_add clamped to 0..n_cap, or n_cap
__device__ __forceinline__ long long crc_len(const long long* n_dev, long long n_add, long long n_cap) {
  if (!n_dev) return n_cap;
  const long long n = *n_dev + n_add;
  return n < 0 ? 0 : n > n_cap ? n_cap : n;
}

// base = data - front is aligned to 16; the message is the virtual bytes front .. front + n - 1 of the string that starts at base
__global__ __launch_bounds__(kCrcBlock) void crc_partials(const uint8_t* __restrict__ base, int front, long long n_cap, const long long* __restrict__ n_dev,
                                                          long long n_add, CrcConsts k, uint32_t* __restrict__ partials) {
  __shared__ CrcPieceLds lds;
  const long long end = front + crc_len(n_dev, n_add, n_cap), v0 = (long long)blockIdx.x * kCrcPiece;
  if (v0 >= end || end == front) {                                   // a piece past the message, or no message (uniform)
    if (threadIdx.x == 0) partials[blockIdx.x] = 0u;
    return;
  }
  const uint32_t r = crc_piece_remainder(lds, base, front, end, v0, k);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// x^e for e < 2^32 - 1 as the product of the table entries of e's bits: 32 lanes of a wave (lanes 32..63 may hold another e), valid in every lane
__device__ __forceinline__ uint32_t crc_xpow_lanes(const CrcConsts& k, uint32_t e, int lane) {
  uint32_t v = (e >> (lane & 31)) & 1u ? k.x2n[lane & 31] : kCrcOne;
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) v = crc_mul(v, __shfl_xor(v, o, 64));
  return v;
}

__global__ __launch_bounds__(256) void crc_combine(const uint32_t* __restrict__ partials, long long seg, int front, long long n_cap,
                                                   const long long* __restrict__ n_dev, long long n_add, CrcConsts k, uint32_t* __restrict__ crc_out) {
  __shared__ uint32_t s[256];
  const long long n = crc_len(n_dev, n_add, n_cap), pieces = crc_pieces(front, n);
  const int t = threadIdx.x;
  uint32_t r = 0;
  for (long long i = t * seg; i < (t + 1) * seg; ++i) r = crc_mul(r, k.piece) ^ (i < pieces ? partials[i] : 0u);
  s[t] = r;
  __syncthreads();
  for (int j = 0; j < 8; ++j) {
    const int o = 1 << j;
    if ((t & (2 * o - 1)) == 0) s[t] = crc_mul(s[t], k.seg[j]) ^ s[t + o];
    __syncthreads();
  }
  if (t < 64) {
    // s[0] is the remainder of front zeros, the message and z zeros; lanes 0..31 form x^(-8 z), lanes 32..63 x^(8 n)
    const unsigned long long z = 256ull * (unsigned long long)seg * kCrcPiece - (unsigned long long)(front + n);
    const uint32_t e_back = (uint32_t)((kCrcOrder - (8ull * z) % kCrcOrder) % kCrcOrder), e_len = (uint32_t)((8ull * (unsigned long long)n) % kCrcOrder);
    const uint32_t p = crc_xpow_lanes(k, t < 32 ? e_back : e_len, t);
    const uint32_t p_len = __shfl(p, 32, 64);
    if (t == 0) *crc_out = crc_mul(0xFFFFFFFFu, p_len) ^ crc_mul(s[0], p) ^ 0xFFFFFFFFu;
  }
}

// the launches of rhccq_crc32; n = *n_dev + n_add (or n_cap)
static int crc_launch(rhccq_ctx* ctx, const uint8_t* data, int64_t n_cap, const int64_t* n_dev, int64_t n_add, uint32_t* partials, uint32_t* crc_out) {
  const int front = (int)((uintptr_t)data & 15);
  const int64_t pieces = crc_pieces(front, n_cap), seg = pieces > 256 ? (pieces + 255) / 256 : 1;
  const CrcConsts k = crc_consts(seg);
  if (pieces > 0)
    hipLaunchKernelGGL(crc_partials, dim3((unsigned)pieces), dim3(kCrcBlock), 0, ctx->stream, data - front, front, (long long)n_cap, (const long long*)n_dev,
                       (long long)n_add, k, partials);
  hipLaunchKernelGGL(crc_combine, dim3(1), dim3(256), 0, ctx->stream, (const uint32_t*)partials, (long long)seg, front, (long long)n_cap,
                     (const long long*)n_dev, (long long)n_add, k, crc_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}
static int64_t crc_work_bytes(int64_t n_cap) { return 4 * (crc_pieces(15, n_cap) + 1); }

// ---- framing -------------------------------------------------------------------------------------------------------------------------
struct PlteConsts {
  uint32_t front;     // the register after "PLTE", times x^(24 K): what stands in front of the entries
  uint32_t join[8];   // x^(24 2^j)
};

// K_plte = 0: colour type 2, no PLTE.  off_idat: where IDAT's length field starts
__global__ __launch_bounds__(256) void png_head_kernel(Head head, const uint8_t* __restrict__ pal, int K_plte, PlteConsts k, long long off_idat,
                                                       uint8_t* __restrict__ out) {
  __shared__ uint32_t s[256];
  const int t = threadIdx.x;
  if (t < kHeadBytes) out[t] = head.b[t];
  if (t < 4) out[off_idat + 4 + t] = (uint8_t)"IDAT"[t];
  if (K_plte == 0) return;                                           // (uniform)
  uint8_t* chunk = out + kHeadBytes;
  // a lane per entry, the entries at the END of the 256 lanes: the lanes in front hold zero bytes, which a plain remainder ignores
  const int e = t - (256 - K_plte);
  uint32_t r = 0;
  if (e >= 0) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const uint8_t v = pal[3 * e + ch];
      chunk[8 + 3 * e + ch] = v;
      r = crc_byte(r, v);
    }
  }
  s[t] = r;
  __syncthreads();
  for (int j = 0; j < 8; ++j) {
    const int o = 1 << j;
    if ((t & (2 * o - 1)) == 0) s[t] = crc_mul(s[t], k.join[j]) ^ s[t + o];
    __syncthreads();
  }
  if (t < 4) {
    const uint32_t len = 3u * (uint32_t)K_plte, crc = k.front ^ s[0] ^ 0xFFFFFFFFu;
    chunk[t] = (uint8_t)(len >> (24 - 8 * t));
    chunk[4 + t] = (uint8_t)"PLTE"[t];
    chunk[8 + len + t] = (uint8_t)(crc >> (24 - 8 * t));
  }
}

__global__ void png_tail_kernel(uint8_t* __restrict__ out, long long off_idat, const long long* __restrict__ len_dev, long long len_cap,
                                const uint32_t* __restrict__ crc_dev, long long* __restrict__ out_len) {
  const int t = threadIdx.x;
  long long len = *len_dev;
  len = len < 0 ? 0 : len > len_cap ? len_cap : len;
  uint8_t* tail = out + off_idat + 8 + len;
  if (t < 4) {
    out[off_idat + t] = (uint8_t)((uint32_t)len >> (24 - 8 * t));
    tail[t] = (uint8_t)(*crc_dev >> (24 - 8 * t));
  }
  if (t < 12) tail[4 + t] = kIend[t];
  if (t == 0) *out_len = off_idat + 8 + len + 16;
}

// ---- arguments -----------------------------------------------------------------------------------------------------------------------
static int png_check(rhccq_ctx* ctx, const char* fn, const void* idx, int eb, int H, int W, const uint8_t* pal, int K, int flags, int64_t limit) {
  static thread_local std::string msg;
  auto fail = [&](int code, const char* what) {
    msg = std::string(fn) + ": " + what;
    return rhccq_fail(ctx, code, msg.c_str());
  };
  if (!idx || !pal) return fail(RHCCQ_E_ARG, "a null idx or palette");
  if (H < 1 || W < 1) return fail(RHCCQ_E_ARG, "H >= 1 and W >= 1 are expected");
  if (K < 1 || K > kMaxRows) return fail(RHCCQ_E_ARG, "K must be 1..65536");
  if (eb != 1 && eb != 2 && eb != 4) return fail(RHCCQ_E_ARG, "idx_elem_bytes must be 1, 2 or 4");
  if ((uintptr_t)idx % (unsigned)eb) return fail(RHCCQ_E_ARG, "idx is not aligned to its element");
  if (flags & ~kFlagsAll) return fail(RHCCQ_E_ARG, "unknown flag bits");
  if ((int64_t)H * png_row_bytes(W, K, flags) > limit) return fail(RHCCQ_E_LIMIT, "scanlines of 2 GiB or more");
  return 0;
}
static int64_t png_limit(int flags) { return flags & RHCCQ_PNG_EXACT ? kScanMax : kFastMax; }

struct Sizes {
  int64_t scan, enc_work, enc_bound, o_misc, o_crc, o_enc, work, bound;
};
static int png_layout(int H, int W, int K, int flags, Sizes& s) {
  s.scan = (int64_t)H * png_row_bytes(W, K, flags);
  const int rc = flags & RHCCQ_PNG_EXACT ? rhccq_zlib9_sizes(s.scan, &s.enc_work, &s.enc_bound) : rhccq_zlib_sizes(s.scan, &s.enc_work, &s.enc_bound);
  if (rc) return rc;
  s.o_misc = align256(s.scan);                                       // the stream's length (int64), the CRC (uint32 at + 8), filter_rows (int64[5] at + 16)
  s.o_crc = s.o_misc + 256;
  s.o_enc = align256(s.o_crc + crc_work_bytes(s.enc_bound + 4));
  s.work = s.o_enc + s.enc_work;
  s.bound = png_idat_offset(K) + 8 + s.enc_bound + 16;
  return 0;
}

static int scanlines_launch(rhccq_ctx* ctx, const void* idx, int eb, int H, int W, const uint8_t* pal, int K, int flags, uint8_t* scan, int64_t* filter_rows) {
  if (const int rc = rhccq_compute_units(ctx)) return rc;
  if (png_indexed(K)) {
    const int d = png_depth(K, flags), mis = (int)((uintptr_t)scan & 3);
    const int64_t rb = png_row_bytes(W, K, flags), total = H * rb, nq = (mis + total + 3) / 4, cap = (int64_t)ctx->compute_units * 16;
    const int64_t blocks = (nq + 255) / 256;
    const dim3 grid((unsigned)(blocks < cap ? blocks : cap)), block(256);
    index_dispatch(eb, [&](auto* t) {
      using T = std::remove_pointer_t<decltype(t)>;
      hipLaunchKernelGGL((png_pack_kernel<T>), grid, block, 0, ctx->stream, (const T*)idx, (int)H, (int)W, (uint32_t)K, d, (uint32_t)rb, scan - mis, mis,
                         (uint32_t)total, (long long*)filter_rows);
    });
  } else {
    if (filter_rows) RHCCQ_HIP(ctx, hipMemsetAsync(filter_rows, 0, 5 * sizeof(int64_t), ctx->stream));
    index_dispatch(eb, [&](auto* t) {
      using T = std::remove_pointer_t<decltype(t)>;
      hipLaunchKernelGGL((png_rgb_kernel<T>), dim3((unsigned)H), dim3(kRgbBlock), 0, ctx->stream, (const T*)idx, (int)W, pal, (uint32_t)K,
                         (int)(flags & RHCCQ_PNG_NO_FILTER ? 1 : 0), scan, (unsigned long long*)filter_rows);
    });
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

template <typename IdxT>
static void scanlines_host(const IdxT* idx, int H, int W, const uint8_t* pal, int K, int flags, uint8_t* scan, int64_t* filter_rows) {
  int64_t rows[5] = {0, 0, 0, 0, 0};
  const int64_t rb = png_row_bytes(W, K, flags);
  if (png_indexed(K)) {
    const int d = png_depth(K, flags);
    for (int64_t y = 0; y < H; ++y) {
      scan[y * rb] = 0;
      for (int64_t c = 0; c + 1 < rb; ++c) scan[y * rb + 1 + c] = (uint8_t)png_packed_byte(idx, y * W, W, (uint32_t)K, d, c);
    }
    rows[0] = H;
  } else {
    for (int64_t y = 0; y < H; ++y) {
      const IdxT* cur = idx + y * W;
      auto at = [&](int64_t yy, int64_t x) { return yy < 0 || x < 0 ? 0u : png_rgb(pal, png_index(cur, (yy - y) * W + x, (uint32_t)K)); };
      int best = 0;
      if (!(flags & RHCCQ_PNG_NO_FILTER)) {
        uint64_t tot[5] = {0, 0, 0, 0, 0};
        for (int64_t x = 0; x < W; ++x) {
          uint32_t cost[5] = {0, 0, 0, 0, 0};
          png_pixel_costs(at(y, x), at(y, x - 1), at(y - 1, x), at(y - 1, x - 1), cost);
          for (int t = 0; t < 5; ++t) tot[t] += cost[t];
        }
        best = png_best(tot);
      }
      scan[y * rb] = (uint8_t)best;
      ++rows[best];
      for (int64_t x = 0; x < W; ++x) {
        const uint32_t px = at(y, x), a = at(y, x - 1), b = at(y - 1, x), c = at(y - 1, x - 1);
        for (int ch = 0; ch < 3; ++ch)
          scan[y * rb + 1 + 3 * x + ch] =
              (uint8_t)png_filter(best, (px >> (8 * ch)) & 255, (a >> (8 * ch)) & 255, (b >> (8 * ch)) & 255, (c >> (8 * ch)) & 255);
      }
    }
  }
  if (filter_rows)
    for (int t = 0; t < 5; ++t) filter_rows[t] = rows[t];
}

}  // namespace png
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::png;

extern "C" {

int rhccq_png_sizes(int32_t H, int32_t W, int32_t K, int32_t flags, int64_t* scan_bytes, int64_t* workspace_bytes, int64_t* out_bound) {
  static const uint8_t none = 0;
  if (const int rc = png_check(nullptr, "png_sizes", &none, 1, H, W, &none, K, flags, png_limit(flags))) return rc;
  Sizes s;
  if (const int rc = png_layout(H, W, K, flags, s)) return rc;
  if (scan_bytes) *scan_bytes = s.scan;
  if (workspace_bytes) *workspace_bytes = s.work;
  if (out_bound) *out_bound = s.bound;
  return RHCCQ_OK;
}

int rhccq_png_scanlines(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags,
                        uint8_t* scan, int64_t* filter_rows) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = png_check(ctx, "png_scanlines", idx, idx_elem_bytes, H, W, palette, K, flags, kScanMax)) return rc;
  if (!scan || (uintptr_t)filter_rows % 8) return rhccq_fail(ctx, RHCCQ_E_ARG, "png_scanlines: a null scan or a misaligned filter_rows");
  return scanlines_launch(ctx, idx, idx_elem_bytes, H, W, palette, K, flags, scan, filter_rows);
}

int64_t rhccq_crc32_bytes(int64_t n_cap) { return n_cap < 0 ? RHCCQ_E_ARG : crc_work_bytes(n_cap); }

int rhccq_crc32(rhccq_ctx* ctx, const uint8_t* data, int64_t n_cap, const int64_t* n_dev, void* workspace, uint32_t* crc_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (n_cap < 0 || (n_cap > 0 && !data) || !workspace || !crc_out || (uintptr_t)workspace % 4 || (uintptr_t)crc_out % 4 || (uintptr_t)n_dev % 8)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "crc32: n_cap < 0, a null data, workspace or crc_out, or a misaligned workspace, crc_out or n_dev");
  return crc_launch(ctx, data, n_cap, n_dev, 0, (uint32_t*)workspace, crc_out);
}

int rhccq_png_encode(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags,
                     void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!ctx) return RHCCQ_E_ARG;
  if (const int rc = png_check(ctx, "png_encode", idx, idx_elem_bytes, H, W, palette, K, flags, png_limit(flags))) return rc;
  if (!workspace || !out || !out_len || (uintptr_t)workspace % 256 || (uintptr_t)out_len % 8)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "png_encode: a null workspace, out or out_len, a workspace not aligned to 256 or a misaligned out_len");
  Sizes s;
  if (const int rc = png_layout(H, W, K, flags, s)) return rhccq_fail(ctx, rc, "png_encode: the encoder refuses the scanlines' size");
  if (out_cap < s.bound) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "png_encode: out_cap below the bound of rhccq_png_sizes");
  uint8_t* ws = (uint8_t*)workspace;
  uint8_t* scan = ws;
  int64_t* zlen = (int64_t*)(ws + s.o_misc);
  uint32_t* crc = (uint32_t*)(ws + s.o_misc + 8);
  const int64_t off = png_idat_offset(K);
  const int k_plte = png_indexed(K) ? K : 0;
  PlteConsts pk{};
  if (k_plte) {
    uint32_t x2n[32];
    crc_x2n(x2n);
    pk.front = crc_mul(crc_state(0xFFFFFFFFu, (const uint8_t*)"PLTE", 4), crc_xpow(x2n, 24ull * (uint64_t)K));
    for (int j = 0; j < 8; ++j) pk.join[j] = crc_xpow(x2n, 24ull << j);
  }
  hipLaunchKernelGGL(png_head_kernel, dim3(1), dim3(256), 0, ctx->stream, png_head(H, W, K, flags), palette, k_plte, pk, (long long)off, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  if (const int rc = scanlines_launch(ctx, idx, idx_elem_bytes, H, W, palette, K, flags, scan, (int64_t*)(ws + s.o_misc + 16))) return rc;
  uint8_t* stream = out + off + 8;
  const int rc = flags & RHCCQ_PNG_EXACT ? rhccq_zlib9_compress(ctx, scan, s.scan, ws + s.o_enc, stream, s.enc_bound, zlen)
                                         : rhccq_zlib_compress(ctx, scan, s.scan, ws + s.o_enc, stream, s.enc_bound, zlen);
  if (rc) return rc;
  if (const int rc2 = crc_launch(ctx, stream - 4, s.enc_bound + 4, zlen, 4, (uint32_t*)(ws + s.o_crc), crc)) return rc2;
  hipLaunchKernelGGL(png_tail_kernel, dim3(1), dim3(64), 0, ctx->stream, out, (long long)off, (const long long*)zlen, (long long)s.enc_bound,
                     (const uint32_t*)crc, (long long*)out_len);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_png_scanlines_host(const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags,
                             uint8_t* scan, int64_t* filter_rows) {
  if (const int rc = png_check(nullptr, "png_scanlines", idx, idx_elem_bytes, H, W, palette, K, flags, kScanMax)) return rc;
  if (!scan) return RHCCQ_E_ARG;
  index_dispatch(idx_elem_bytes, [&](auto* t) { scanlines_host((decltype(t))idx, H, W, palette, K, flags, scan, filter_rows); });
  return RHCCQ_OK;
}

int rhccq_crc32_host(const uint8_t* data, int64_t n, uint32_t* crc_out) {
  if (n < 0 || (n > 0 && !data) || !crc_out) return RHCCQ_E_ARG;
  *crc_out = crc32_serial(data, n);
  return RHCCQ_OK;
}

int rhccq_png_encode_host(const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags, uint8_t* out,
                          int64_t out_cap, int64_t* out_len) {
  if (const int rc = png_check(nullptr, "png_encode", idx, idx_elem_bytes, H, W, palette, K, flags, kScanMax)) return rc;
  if (!(flags & RHCCQ_PNG_EXACT) || !out || !out_len) return RHCCQ_E_ARG;
  Sizes s;
  if (const int rc = png_layout(H, W, K, flags, s)) return rc;
  if (out_cap < s.bound) return RHCCQ_E_LIMIT;
  std::vector<uint8_t> scan((size_t)s.scan);
  index_dispatch(idx_elem_bytes, [&](auto* t) { scanlines_host((decltype(t))idx, H, W, palette, K, flags, scan.data(), nullptr); });
  const Head head = png_head(H, W, K, flags);
  uint8_t* p = out;
  for (int i = 0; i < kHeadBytes; ++i) *p++ = head.b[i];
  auto chunk_crc = [](uint8_t* type, int64_t n) { put_be32(type + n, crc32_serial(type, n)); };
  if (png_indexed(K)) {
    put_be32(p, 3u * (uint32_t)K);
    p[4] = 'P'; p[5] = 'L'; p[6] = 'T'; p[7] = 'E';
    for (int i = 0; i < 3 * K; ++i) p[8 + i] = palette[i];
    chunk_crc(p + 4, 4 + 3 * (int64_t)K);
    p += 12 + 3 * K;
  }
  int64_t zlen = 0;
  if (const int rc = rhccq_zlib9_compress_host(scan.data(), s.scan, p + 8, s.enc_bound, &zlen)) return rc;
  put_be32(p, (uint32_t)zlen);
  p[4] = 'I'; p[5] = 'D'; p[6] = 'A'; p[7] = 'T';
  chunk_crc(p + 4, 4 + zlen);
  p += 12 + zlen;
  for (int i = 0; i < 12; ++i) *p++ = kIend[i];
  *out_len = p - out;
  return RHCCQ_OK;
}

}  // extern "C"
