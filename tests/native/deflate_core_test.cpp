// csrc/deflate_core.h without a device: the symbol algebra against RFC 1951's tables written out, the fixed code, the code-length order,
// bit reversal, and Adler-32 by chunk sums and fold against the byte-serial definition.  Plain C++17, no HIP header
// (tests/test_deflate_core_cpu.py builds it with g++ and the host sanitizers, and compares the printed checksums with zlib.adler32).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "deflate_core.h"

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

using namespace rhccq::deflate;

// RFC 1951 section 3.2.5: extra bits and first length of codes 257..285, extra bits and first distance of codes 0..29
static const int kLenExtra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
static const int kLenBase[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
static const int kDistExtra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
static const int kDistBase[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                  8193, 12289, 16385, 24577};
// section 3.2.7
static const int kOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

static uint32_t adler_serial(const std::vector<uint8_t>& v) {
  uint32_t s1 = 1, s2 = 0;
  for (uint8_t b : v) {
    s1 = (s1 + b) % 65521u;
    s2 = (s2 + s1) % 65521u;
  }
  return s2 << 16 | s1;
}

static uint32_t adler_chunked(const std::vector<uint8_t>& v, int64_t chunk) {
  const int64_t n = (int64_t)v.size();
  std::vector<uint32_t> part((size_t)(2 * ((n + chunk - 1) / chunk)));
  for (int64_t c = 0; c * chunk < n; ++c) adler_chunk_sums(v.data() + c * chunk, n - c * chunk < chunk ? n - c * chunk : chunk, &part[(size_t)(2 * c)]);
  return adler_fold(part.data(), n, chunk);
}

int main() {
  // the published tables
  for (int c = 0; c < 29; ++c) CHECK(len_base(c) == kLenBase[c] && len_extra(c) == kLenExtra[c]);
  for (int c = 0; c < 30; ++c) CHECK(dist_base(c) == kDistBase[c] && dist_extra(c) == kDistExtra[c]);

  // every length and every distance: the encoder's mapping and the decoder's bases are inverses
  int last = 0;
  for (int len = 3; len <= 258; ++len) {
    int eb = -1, ev = -1;
    const int c = len_code(len, eb, ev);
    CHECK(c >= 0 && c <= 28 && c >= last);
    CHECK(eb == len_extra(c) && ev >= 0 && ev < (1 << eb));
    CHECK(len_base(c) + ev == len);
    last = c;
  }
  {
    int eb, ev;
    CHECK(len_code(258, eb, ev) == 28 && eb == 0 && ev == 0);
  }
  last = 0;
  for (int dist = 1; dist <= 32768; ++dist) {
    int eb = -1, ev = -1;
    const int c = dist_code(dist, eb, ev);
    CHECK(c >= 0 && c <= 29 && c >= last);
    CHECK(eb == dist_extra(c) && ev >= 0 && ev < (1 << eb));
    CHECK(dist_base(c) + ev == dist);
    last = c;
  }
  CHECK(kWindow == 32768 && last == 29);

  // the fixed literal/length code: 8, 9, 7, 8 bits on the four ranges, a complete code (Kraft sum exactly 1, counted in units of 2^-9)
  for (int s = 0; s <= 143; ++s) CHECK(fixed_litlen_bits(s) == 8);
  for (int s = 144; s <= 255; ++s) CHECK(fixed_litlen_bits(s) == 9);
  for (int s = 256; s <= 279; ++s) CHECK(fixed_litlen_bits(s) == 7);
  for (int s = 280; s <= 287; ++s) CHECK(fixed_litlen_bits(s) == 8);
  int kraft = 0;
  for (int s = 0; s < 288; ++s) kraft += 1 << (9 - fixed_litlen_bits(s));
  CHECK(kraft == 1 << 9);

  // the code-length alphabet: the published order, a permutation of 0..18; extra bits of 16, 17, 18
  int seen = 0;
  for (int k = 0; k < 19; ++k) {
    CHECK(codelen_order(k) == kOrder[k]);
    seen |= 1 << codelen_order(k);
  }
  CHECK(seen == (1 << 19) - 1);
  static_assert(codelen_order(0) == 16 && codelen_order(18) == 15, "usable in constant expressions");
  for (int s = 0; s <= 15; ++s) CHECK(codelen_extra(s) == 0);
  CHECK(codelen_extra(16) == 2 && codelen_extra(17) == 3 && codelen_extra(18) == 7);

  // bit reversal: an involution on the codes of every length, and the first bit goes last
  for (int len = 1; len <= 15; ++len)
    for (uint32_t code = 0; code < (1u << len); ++code) {
      const uint32_t r = bit_reverse(code, len);
      CHECK(r < (1u << len) && bit_reverse(r, len) == code);
      CHECK((r & 1u) == (code >> (len - 1)));
    }
  CHECK(bit_reverse(0x1u, 15) == 0x4000u && bit_reverse(0x6u, 3) == 0x3u && bit_reverse(0x7FFFu, 0) == 0u);

  // Adler-32: chunk sums + fold == the byte-serial definition; all 0xFF gives the largest sums.  One line per case for the caller.
  CHECK(kAdlerMod == 65521u);
  const int64_t sizes[] = {0, 1, 4095, 4096, 4097, 65535, 65536, 65537, 5 * (int64_t)1048576 + 3};
  for (int fill = 0; fill < 2; ++fill)
    for (int64_t n : sizes) {
      std::vector<uint8_t> v((size_t)n);
      for (int64_t i = 0; i < n; ++i) v[(size_t)i] = fill == 0 ? 0xFF : (uint8_t)i;
      const uint32_t want = adler_serial(v);
      for (int64_t chunk : {(int64_t)4096, (int64_t)65536}) {
        const uint32_t got = adler_chunked(v, chunk);
        CHECK(got == want);
        std::printf("adler %s %lld %lld %08x\n", fill == 0 ? "ff" : "counter", (long long)n, (long long)chunk, got);
      }
    }
  std::printf("deflate_core ok\n");
  return 0;
}
