// The step functions and constants of the position-only (pattern) dither, the argument tests of its host side and the body of its
// kernel, which the batched form (palette_batch.hip) runs per image.  The definition and the kernel's shape are in palette_pattern.hip.
//
// Arithmetic.  A pixel's accumulated error e grows by p - palette[c] (-255..255 per channel) for each of the N <= 64 candidates:
// |e| <= 64 * 255 = 16320, inside 24 bits, and with a strength of at most 256, |s e + 128| < 2^23: int32 throughout.  The shift by 8 is
// arithmetic, so the quotient is floored toward minus infinity.  A row's luma 299 R + 587 G + 114 B is at most 255000 (18 bits); the
// order key (luma + 1) << 32 | row is never 0, so 0 serves as "below every key".
#pragma once
#include "palette_dither.h"

namespace rhccq {

constexpr uint32_t kPatternMaxStrength = 256u;
constexpr int kPatternMaxRows = 4096;            // palette rows of the device form: packed as RemapEntry they are 32 KiB of LDS, and a row's index 12 bits
constexpr int kPatternBlock = 128;               // lanes of a workgroup
constexpr int kPatternMaxCand = 64;              // candidates of a pixel at the largest size
constexpr int kPatternStripBytes = 16384;        // LDS of a workgroup's candidate strips at most: 128 lanes x pixels x candidates x 2
constexpr int kPatternMaxPx = 8;                 // pixels a lane holds at most: their errors, targets and winners are registers

struct PatternStrength { uint32_t v[kRemapMaxClasses + 1]; };
struct PatternErr { int32_t r, g, b; };

// pixels a lane works on side by side: 8, 4, 1 for the sizes 2, 4, 8, so that a workgroup's strips fit kPatternStripBytes
__host__ __device__ constexpr int pattern_px(int size) {
  return kPatternStripBytes / (kPatternBlock * size * size * 2) < kPatternMaxPx ? kPatternStripBytes / (kPatternBlock * size * size * 2) : kPatternMaxPx;
}
__host__ __device__ constexpr long long pattern_chunk(int size) { return (long long)kPatternBlock * pattern_px(size); }
static_assert(pattern_px(2) == 8 && pattern_px(4) == 4 && pattern_px(8) == 1, "a lane's strips");

static inline bool pattern_size_ok(int32_t size) { return size == 2 || size == 4 || size == 8; }

// one channel of a candidate's target: the pixel's value plus the scaled accumulated error, floored and clamped
__host__ __device__ __forceinline__ uint32_t pattern_channel(uint32_t p, uint32_t strength, int32_t e) {
#if defined(__HIP_DEVICE_COMPILE__)
  const int32_t t = (int32_t)p + ((__mul24((int32_t)strength, e) + 128) >> 8);          // (both factors are inside 24 bits: the full-rate multiply)
#else
  const int32_t t = (int32_t)p + (((int32_t)strength * e + 128) >> 8);
#endif
  return (uint32_t)(t < 0 ? 0 : t > 255 ? 255 : t);
}
// the target of the next candidate (0x00RRGGBB, as remap_pack_px packs it; px may carry anything in its top byte)
__host__ __device__ __forceinline__ uint32_t pattern_target(uint32_t px, uint32_t strength, PatternErr e) {
  return pattern_channel((px >> 16) & 255u, strength, e.r) << 16 | pattern_channel((px >> 8) & 255u, strength, e.g) << 8 |
         pattern_channel(px & 255u, strength, e.b);
}
// the accumulated error behind a candidate of colour col: e + p - col, against the ORIGINAL pixel
__host__ __device__ __forceinline__ PatternErr pattern_error(PatternErr e, uint32_t px, uint32_t col) {
  return {e.r + (int32_t)((px >> 16) & 255u) - (int32_t)((col >> 16) & 255u), e.g + (int32_t)((px >> 8) & 255u) - (int32_t)((col >> 8) & 255u),
          e.b + (int32_t)(px & 255u) - (int32_t)(col & 255u)};
}
// the order of the candidates: by the luma of the row's colour, then by the row; never 0
__host__ __device__ __forceinline__ uint64_t pattern_key(uint32_t col, uint32_t row) {
  const uint32_t luma = 299u * ((col >> 16) & 255u) + 587u * ((col >> 8) & 255u) + 114u * (col & 255u);
  return (uint64_t)(luma + 1u) << 32 | row;
}
// the threshold of position (y, x): the Bayer matrix M_2 = [[0, 2], [3, 1]], M_2n = [[4 M_n, 4 M_n + 2], [4 M_n + 3, 4 M_n + 1]], whose
// entry is the base-4 number of the digits M_2[y bit][x bit], bit 0 the most significant
__host__ __device__ __forceinline__ uint32_t pattern_threshold(long long y, long long x, int size) {
  uint32_t r = 0u;
  for (int bit = 0; (1 << bit) < size; ++bit) {
    const uint32_t a = (uint32_t)(y >> bit) & 1u, b = (uint32_t)(x >> bit) & 1u;
    r = r * 4u + ((a ^ b) << 1 | a);
  }
  return r;
}
// rank selection: entry r (from 0) of the n candidates row_at(0 .. n - 1) in ascending key order, duplicates kept; colour_of(row) is the
// row's colour.  Round by round the smallest key above the last one and how often it occurs: as many rounds as the rank has distinct
// keys below it, and most pixels have few
template <typename RowAt, typename ColourOf>
__host__ __device__ __forceinline__ uint32_t pattern_select(int n, uint32_t r, RowAt&& row_at, ColourOf&& colour_of) {
  uint64_t last = 0ull;
  for (;;) {
    uint64_t m = ~0ull;
    uint32_t cnt = 0u;
    for (int j = 0; j < n; ++j) {
      const uint32_t row = row_at(j);
      const uint64_t k = pattern_key(colour_of(row), row);
      if (k > last && k <= m) {
        cnt = k < m ? 1u : cnt + 1u;
        m = k;
      }
    }
    if (r < cnt || cnt == 0u) return (uint32_t)m;                                       // (cnt == 0 cannot happen for r < n: the loop must end)
    r -= cnt;
    last = m;
  }
}

// the argument tests of both forms, in rhccq_palette_dither's order (the colours before the strength), then the size; the device form appends its own
static inline int pattern_check(rhccq_ctx* ctx, const char* what, const void* rgb, int32_t H, int32_t W, const void* palette, int32_t K, const void* cls,
                                int32_t n_classes, const uint32_t* strength, int32_t size, const void* idx_out, int32_t idx_elem_bytes,
                                const void* sums) {
  if (const int rc = rows_check(ctx, what, rgb, H, W, palette, K, cls, n_classes, strength, idx_out, idx_elem_bytes, sums)) return rc;
  if (const int rc = search_limit(ctx, what, K)) return rc;
  for (int i = 0; i <= n_classes; ++i)
    if (strength[i] > kPatternMaxStrength) return remap_fail(ctx, RHCCQ_E_ARG, what, ": a strength is at most 256");
  if (!pattern_size_ok(size)) return remap_fail(ctx, RHCCQ_E_ARG, what, ": the size must be 2, 4 or 8");
  return 0;
}

// palette entries in LDS: an even number, the odd one out an entry that never wins
__host__ __device__ __forceinline__ int pattern_padded(int K) { return (K + 1) & ~1; }
// a workgroup's dynamic LDS: the packed palette (16-byte reads), the candidate strips, the class sums [16][3], the totals [2] and the strengths [17]
static inline size_t pattern_lds_bytes(int K) {
  return (size_t)pattern_padded(K) * 8 + kPatternStripBytes + (size_t)(kRemapMaxClasses * 3 + 2) * sizeof(unsigned long long) +
         (size_t)(kRemapMaxClasses + 1) * sizeof(uint32_t);
}

// ---- the kernel's body, shared by palette_pattern.hip (one image a launch) and palette_batch.hip (one image per grid row) ----
// Workgroup `bid` of the `nblk` that share the image takes chunks of 128 x P pixels grid-stride (lane l: pixels base + l + 128 q, so
// loads and index stores coalesce).  s_dyn is the workgroup's dynamic LDS, 16-byte aligned, pattern_lds_bytes(K) long.
template <int kSize, typename IdxT>
__device__ __forceinline__ void pattern_body(const uint8_t* __restrict__ rgb, long long n_px, int W, const uint8_t* __restrict__ pal, int K,
                                             const uint8_t* __restrict__ cls, int n_classes, const PatternStrength& strength,
                                             IdxT* __restrict__ idx_out, unsigned long long* __restrict__ sums, long long bid, long long nblk,
                                             uint4* s_dyn) {
  constexpr int N = kSize * kSize, P = pattern_px(kSize);
  constexpr long long kChunk = pattern_chunk(kSize);
  const int K2 = pattern_padded(K), tid = threadIdx.x;
  RemapEntry* s_pal = reinterpret_cast<RemapEntry*>(s_dyn);                            // [K2], entry j under its row number (K <= 4096: 12 bits)
  uint16_t* s_strip = reinterpret_cast<uint16_t*>(s_pal + K2);                         // [P][N][128]: candidate i of the lane's pixel q
  unsigned long long* s_cls = reinterpret_cast<unsigned long long*>(s_strip + kPatternStripBytes / 2);   // [16][3]
  unsigned long long* s_tot = s_cls + kRemapMaxClasses * 3;                            // {squared error, moved}
  for (int j = tid; j < K2; j += kPatternBlock) s_pal[j] = j < K ? remap_pack_entry(pal + (long long)j * 3, j) : RemapEntry{0u, 0xFFFFFFFFu};
  uint32_t* s_str = reinterpret_cast<uint32_t*>(s_tot + 2);                            // [17]
  if (tid < kRemapMaxClasses * 3 + 2) s_cls[tid] = 0ull;
  if (tid <= n_classes) s_str[tid] = strength.v[tid];
  __syncthreads();

  const long long n_chunks = (n_px + kChunk - 1) / kChunk;
  unsigned long long all_sse = 0ull, all_moved = 0ull;
  for (long long chunk = bid; chunk < n_chunks; chunk += nblk) {                        // (no barrier inside: a lane's strips are its own)
    const long long base = chunk * kChunk + tid;
    uint32_t px[P], sv[P], kc[P];
    PatternErr e[P];
    bool flat[P];                                                                      // the pixel's candidates are N times the first one
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const long long p = base + (long long)q * kPatternBlock;
      const bool in = p < n_px;
      px[q] = in ? remap_pack_px(rgb + p * 3) : 0u;
      kc[q] = in ? runs_class(cls, p, n_classes) : (uint32_t)n_classes;
      sv[q] = s_str[kc[q]];
      e[q] = {0, 0, 0};
      flat[q] = false;
    }
    for (int i = 0; i < N; ++i) {
      uint32_t target[P], best[P];
#pragma unroll
      for (int q = 0; q < P; ++q) {
        target[q] = pattern_target(px[q], sv[q], e[q]);
        best[q] = 0xFFFFFFFFu;
      }
#pragma unroll 2
      for (int j = 0; j < K2 / 2; ++j) {
        const uint4 c = s_dyn[j];                                                      // wave-uniform address: broadcast
#pragma unroll
        for (int q = 0; q < P; ++q) {
          best[q] = min(best[q], remap_eval(target[q], RemapEntry{c.x, c.y}));
          best[q] = min(best[q], remap_eval(target[q], RemapEntry{c.z, c.w}));
        }
      }
#pragma unroll
      for (int q = 0; q < P; ++q) {
        const uint32_t row = best[q] & ((1u << kRemapIdxBits) - 1u);
        s_strip[(q * N + i) * kPatternBlock + tid] = (uint16_t)row;
        e[q] = pattern_error(e[q], px[q], dither_entry_colour(s_pal[row]));
        if (i == 0) flat[q] = sv[q] == 0u || (e[q].r | e[q].g | e[q].b) == 0;           // every target is the pixel itself: N equal candidates
      }
      if (i == 0) {
        bool done = true;
#pragma unroll
        for (int q = 0; q < P; ++q) done = done && flat[q];
        if (__all(done)) break;                                                        // (wave uniform) nothing in this wave has a second row
      }
    }
#pragma unroll
    for (int q = 0; q < P; ++q) {
      const long long p = base + (long long)q * kPatternBlock;
      if (p < n_px) {
        const uint16_t* strip = s_strip + q * N * kPatternBlock + tid;
        const uint32_t b = strip[0];                                                   // the first candidate's target is the pixel itself: the remap's row
        const long long y = p / W, x = p - y * W;
        const uint32_t out = flat[q] ? b
                                     : pattern_select(N, pattern_threshold(y, x, kSize), [&](int j) { return (uint32_t)strip[j * kPatternBlock]; },
                                                      [&](uint32_t row) { return dither_entry_colour(s_pal[row]); });
        idx_out[p] = (IdxT)out;
        const uint32_t d = runs_dist(px[q], dither_entry_colour(s_pal[out])), mv = out != b ? 1u : 0u;
        all_sse += d;
        all_moved += mv;
        if (kc[q] < (uint32_t)n_classes) {
          atomicAdd(&s_cls[kc[q] * 3 + 0], 1ull);
          atomicAdd(&s_cls[kc[q] * 3 + 1], (unsigned long long)d);
          if (mv) atomicAdd(&s_cls[kc[q] * 3 + 2], 1ull);
        }
      }
    }
  }
  all_sse = wave_sum(all_sse);
  all_moved = wave_sum(all_moved);
  if ((tid & 63) == 0) {
    if (all_sse) atomicAdd(&s_tot[0], all_sse);
    if (all_moved) atomicAdd(&s_tot[1], all_moved);
  }
  __syncthreads();
  if (tid < n_classes * 3) {                                                           // one atomic per workgroup, row and column
    if (s_cls[tid]) atomicAdd(&sums[tid], s_cls[tid]);
  } else if (tid < n_classes * 3 + 3) {
    const int col = tid - n_classes * 3;
    unsigned long long t = 0ull;
    if (col == 0) {                                                                    // the pixels of this workgroup's chunks
      for (long long chunk = bid; chunk < n_chunks; chunk += nblk) t += (unsigned long long)min(kChunk, n_px - chunk * kChunk);
    } else {
      t = s_tot[col - 1];
    }
    if (t) atomicAdd(&sums[tid], t);
  }
}

}  // namespace rhccq
