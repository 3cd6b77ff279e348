// The RFC 1950 / 1951 facts the device zlib codecs share: zlib_deflate.hip (the fast encoder), zlib_deflate9.hip (the byte-exact level-9
// encoder) and zlib_inflate.hip.  The functions are plain C++ over <stdint.h>: a host-only program may include this file without the HIP
// headers (tests/native/deflate_core_test.cpp does).  The kernels at the end exist under hipcc only.
//   symbols     length 3..258 <-> code 0..28 (symbol - 257), distance 1..32768 <-> code 0..29, their extra bits and bases, the fixed
//               literal/length code, the code-length alphabet's extra bits and transmission order, bit reversal of a Huffman code.
//               No table indexed at run time by a hot loop: it would live in scratch memory on the device.
//   Adler-32    a chunk's partial sums (sum b, sum (L - k) b_k) mod 65521 and their fold, in order, to the checksum
//   kernels     adler_partials_kernel<kChunk>, hash_chain_kernel<Hash> (the 3-byte hash is the encoder's own), words_zero, words_copy
// What stays apart on purpose ("One RFC 1950 / 1951 core"): the two bit writers, the Block structs and Layouts, match
// search, parsing, tree construction, inflate's reader and tables, and the one line of inflate's worker that writes out the fixed
// code's lengths (zlib_inflate.hip says why).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "rhccq_common.h"
#define RHCCQ_DEFLATE_HD __host__ __device__ inline
#else
#define RHCCQ_DEFLATE_HD inline
#endif

namespace rhccq {
namespace deflate {

constexpr int kWindow = 32768;             // RFC 1951 distance limit
constexpr int kHashBits = 15;
constexpr int kHashChunk = 65536;          // positions a hash_chain_kernel workgroup owns
constexpr uint32_t kAdlerMod = 65521u;

// ---- symbols (RFC 1951 3.2.5 - 3.2.7) ----------------------------------------------------------------------------------------------
// length 3..258 -> code 0..28 (symbol - 257), extra bits, extra value
RHCCQ_DEFLATE_HD int len_code(int len, int& extra_bits, int& extra_val) {
  const int l = len - 3;
  if (l == 255) { extra_bits = 0; extra_val = 0; return 28; }
  if (l < 8) { extra_bits = 0; extra_val = 0; return l; }
  const int e = 29 - __builtin_clz((uint32_t)l);                  // floor(log2 l) - 2
  extra_bits = e;
  extra_val = l & ((1 << e) - 1);
  return 4 * e + 4 + ((l >> e) & 3);
}

// distance 1..32768 -> code 0..29, extra bits, extra value
RHCCQ_DEFLATE_HD int dist_code(int dist, int& extra_bits, int& extra_val) {
  const int d = dist - 1;
  if (d < 4) { extra_bits = 0; extra_val = 0; return d; }
  const int e = 30 - __builtin_clz((uint32_t)d);                  // floor(log2 d) - 1
  extra_bits = e;
  extra_val = d & ((1 << e) - 1);
  return 2 * e + 2 + ((d >> e) & 1);
}

RHCCQ_DEFLATE_HD int len_extra(int code) { return (code < 8 || code == 28) ? 0 : (code - 4) >> 2; }
RHCCQ_DEFLATE_HD int dist_extra(int code) { return code < 4 ? 0 : (code >> 1) - 1; }
RHCCQ_DEFLATE_HD int len_base(int code) {
  if (code < 8) return code + 3;
  if (code == 28) return 258;
  return ((4 + (code & 3)) << ((code - 4) >> 2)) + 3;
}
RHCCQ_DEFLATE_HD int dist_base(int code) {
  if (code < 4) return code + 1;
  return ((2 + (code & 1)) << ((code >> 1) - 1)) + 1;
}

RHCCQ_DEFLATE_HD int fixed_litlen_bits(int sym) { return sym < 144 ? 8 : sym < 256 ? 9 : sym < 280 ? 7 : 8; }   // 0..287; distances: 5
RHCCQ_DEFLATE_HD int codelen_extra(int sym) { return sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0; }
// the order in which a dynamic block sends the code-length code's lengths, k = 0..18.  A local array, indexed only by unrolled
// constants or once per block, never by a hot loop: no scratch memory.
RHCCQ_DEFLATE_HD constexpr int codelen_order(int k) {
  constexpr int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  return order[k];
}

// a Huffman code of len bits, first bit last: as DEFLATE's LSB-first packing wants it
RHCCQ_DEFLATE_HD uint32_t bit_reverse(uint32_t code, int len) {
  uint32_t r = 0;
  for (int k = 0; k < len; ++k) {
    r = (r << 1) | (code & 1);
    code >>= 1;
  }
  return r;
}

// ---- Adler-32 (RFC 1950) --------------------------------------------------------------------------------------------------------------
// part[0] = sum b_k, part[1] = sum (L - k) b_k over bytes[0..L), both mod 65521: what the chunk adds to s1, and to s2 beyond L s1.
// L < 2^28 keeps the sums inside 64 bits.
RHCCQ_DEFLATE_HD void adler_chunk_sums(const uint8_t* bytes, int64_t L, uint32_t* part) {
  uint64_t a = 0, w = 0;
  for (int64_t k = 0; k < L; ++k) {
    a += bytes[k];
    w += (uint64_t)(L - k) * bytes[k];
  }
  part[0] = (uint32_t)(a % kAdlerMod);
  part[1] = (uint32_t)(w % kAdlerMod);
}

// the checksum of `total` bytes from the partial sums of their chunks of `chunk` bytes (the last one shorter), folded in order
RHCCQ_DEFLATE_HD uint32_t adler_fold(const uint32_t* part, int64_t total, int64_t chunk) {
  uint64_t s1 = 1, s2 = 0;
  for (int64_t c = 0; c * chunk < total; ++c) {
    const int64_t L = total - c * chunk < chunk ? total - c * chunk : chunk;
    s2 = (s2 + (uint64_t)L % kAdlerMod * s1 + part[2 * c + 1]) % kAdlerMod;
    s1 = (s1 + part[2 * c]) % kAdlerMod;
  }
  return (uint32_t)(s2 << 16 | s1);
}

#if defined(__HIPCC__)
// ---- kernels ----------------------------------------------------------------------------------------------------------------------------
// one workgroup per chunk of kChunk input bytes: adl[2 c], adl[2 c + 1] = adler_chunk_sums of chunk c (zeros for a chunk past the end)
template <int kChunk>
static __global__ __launch_bounds__(256) void adler_partials_kernel(const uint8_t* __restrict__ in, int64_t n, uint32_t* __restrict__ adl) {
  __shared__ unsigned long long red[8];
  const int64_t c = blockIdx.x;
  const int64_t s = c * kChunk;
  const int64_t L = n - s < kChunk ? n - s : kChunk;
  unsigned long long a = 0, b = 0;
  for (int64_t k = threadIdx.x; k < L; k += 256) {
    const unsigned long long v = in[s + k];
    a += v;
    b += (unsigned long long)(L - k) * v;
  }
  a = block_sum(a, red);
  b = block_sum(b, red);
  if (threadIdx.x == 0) {
    adl[2 * c] = (uint32_t)(a % kAdlerMod);
    adl[2 * c + 1] = (uint32_t)(b % kAdlerMod);
  }
}

// one wave per hash chunk: prev[i] = distance to the nearest earlier position with the same 3-byte hash (0: none within 32 KiB).
// Hash(in, i) < 2^kHashBits reads in[i .. i + 2].  The chunk re-inserts its 32 KiB look-back into an LDS head table of the last
// position (+1) of every hash seen so far, so prev[] is one global function of the input and chains run across chunk boundaries.
template <uint32_t (*Hash)(const uint8_t*, int64_t)>
static __global__ __launch_bounds__(64) void hash_chain_kernel(const uint8_t* __restrict__ in, int64_t n, uint16_t* __restrict__ prev) {
  __shared__ uint32_t head[1 << kHashBits];
  const int lane = threadIdx.x;
  for (int k = lane; k < (1 << kHashBits); k += 64) head[k] = 0;
  __syncthreads();
  const int64_t cs = (int64_t)blockIdx.x * kHashChunk;
  const int64_t ce = cs + kHashChunk < n ? cs + kHashChunk : n;
  const int64_t ws = cs > kWindow ? cs - kWindow : 0;
  for (int64_t base = ws; base < ce; base += 64) {
    const int64_t i = base + lane;
    const bool valid = i < ce && i + 2 < n;
    const uint32_t h = valid ? Hash(in, i) : (0xFFFF0000u | (uint32_t)lane);
    // nearest earlier lane of this batch with the same hash: bit k of eq = lane - k has it (63 independent shuffles,
    // unrolled so that they are in flight together instead of one wait each)
    uint64_t eq = 0;
#pragma unroll
    for (int k = 1; k < 64; ++k) eq |= (uint64_t)(__shfl(h, (lane - k) & 63, 64) == h) << k;
    eq &= (2ull << lane) - 2ull;                   // bits 1..lane: lanes below this one
    const int pl = eq ? lane - __builtin_ctzll(eq) : -1;
    int64_t p = -1;
    if (valid) p = pl >= 0 ? base + pl : (int64_t)head[h] - 1;
    __syncthreads();
    if (valid) atomicMax(&head[h], (uint32_t)(i + 1));
    __syncthreads();
    if (i >= cs && i < ce) {
      const int64_t d = p >= 0 ? i - p : 0;
      prev[i] = (uint16_t)((p >= 0 && d <= kWindow) ? d : 0);
    }
  }
}

// clear the packing words (the encoders assemble their output by OR-ing bits into 32-bit words), and kStats statistics words with them
template <int kStats>
static __global__ void words_zero(uint32_t* w, int64_t nw, int64_t* stats) {
  const int64_t t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < nw; i += (int64_t)gridDim.x * blockDim.x) w[i] = 0;
  if (t0 < kStats) stats[t0] = 0;
}

// packing words -> bytes of the caller's output buffer (a template, like the others, so that only an object that launches it carries it)
template <typename Byte>
static __global__ void words_copy(const uint32_t* __restrict__ words, int64_t nbytes, Byte* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nbytes; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (Byte)(words[i >> 2] >> (8 * (i & 3)));
}
#endif

}  // namespace deflate
}  // namespace rhccq
