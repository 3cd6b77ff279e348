// Huffman tables made for the picture (EXTENSION, include/rhccq.h "JPEG files written with optimised Huffman tables"): the functions the
// kernels of jpeg_optimize.hip and the serial host forms share.  Plain C++ over <stdint.h>, as jpeg_write.h.
//   counts     blocks_ok (libjpeg's search starts from 10^9), histogram_serial over jpeg_write.h's lane_sym and dc_pred;
//   lengths    merge_serial: libjpeg's jpeg_gen_optimal_table with a root per symbol in place of its others[] chains;
//   codes      fold_bits (the fold above 16 bits and the reserved code's removal), key_of and code_of_rank (huffval's order, the
//              canonical codes);
//   header     plan_of, dht_at: where the new DHT segments and the old DRI and SOS go;
//   serial     huffman_serial: the host form of the table launch.
#pragma once
#include "jpeg_write.h"

namespace rhccq {
namespace jpego {

using jpegr::block_at;
using jpegr::comp_of;
using jpegr::Geo;
using jpegr::zigzag;
using jpegw::Frame;
using jpegw::kHeaderMax;
using jpegw::Tables;

constexpr int64_t kCountMax = 1000000000;                  // libjpeg's search for the least count starts from here
constexpr uint32_t kNone = 0xFFFFFFFFu;                    // a count that is not there
constexpr int kLenMax = 256;                               // 257 leaves: no code is deeper
constexpr int kHistWaveBlocks = 8;                         // blocks a wave of the histogram launch takes where the card has room ...
constexpr int kHistGroupsPerCu = 2;                        // ... else this many workgroups a CU stride over them

// every count, and their sum with the reserved symbol's 1, stays below kCountMax
RHCCQ_JPEG_HD bool blocks_ok(const Frame& f) { return 64 * f.g.blocks + 1 < kCountMax; }

// ---- counts --------------------------------------------------------------------------------------------------------------------------
// counts[t][symbol], t = DC0, AC0, DC1, AC1; a ZRL code counts as AC symbol 0xF0
inline void histogram_serial(const Frame& f, const int16_t* coef, uint32_t counts[4][256]) {
  const Geo& g = f.g;
  memset(counts, 0, 4 * 256 * sizeof(uint32_t));
  for (int64_t A = 0; A < g.blocks; ++A) {
    const int t = comp_of(g, (int)(A % g.bpm)) ? 2 : 0;
    const int16_t* blk = coef + 64 * block_at(g, A);
    uint64_t mask = 0;
    for (int k = 1; k < 64; ++k) mask |= (uint64_t)(blk[zigzag(k)] != 0) << k;
    for (int k = 0; k < 64; ++k) {
      const jpegw::LaneSym y = jpegw::lane_sym(k, k ? blk[zigzag(k)] : blk[0] - jpegw::dc_pred(g, coef, A), mask);
      if (y.sym >= 0) ++counts[t + (k > 0)][y.sym];
      counts[t + 1][0xF0] += (uint32_t)y.zrl;
    }
  }
}

// ---- lengths -------------------------------------------------------------------------------------------------------------------------
// jchuff.c's jpeg_gen_optimal_table up to its codesize[]: symbol 256 is reserved with count 1 (no code of all ones); the least count
// wins, the larger symbol among equals, for c1 and then for c2 != c1; c1 takes c2's count.  libjpeg walks two others[] chains to add a
// bit to every symbol of both trees; here every symbol knows its tree's root (the c1 that took it in last), and the step is: every
// symbol whose root is c1 or c2 adds one, root c2 becomes c1.  freq[257] is used up; -> the deepest length
inline int merge_serial(uint32_t* freq, int32_t* len) {
  int32_t root[257];
  for (int i = 0; i <= 256; ++i) root[i] = i, len[i] = 0;
  freq[256] = 1;
  int longest = 0;
  for (int step = 0; step < 256; ++step) {
    int c1 = -1, c2 = -1;
    uint32_t v = kNone;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] != kNone && freq[i] <= v) v = freq[i], c1 = i;
    v = kNone;
    for (int i = 0; i <= 256; ++i)
      if (freq[i] && freq[i] != kNone && freq[i] <= v && i != c1) v = freq[i], c2 = i;
    if (c2 < 0) break;
    freq[c1] += freq[c2], freq[c2] = 0;
    for (int i = 0; i <= 256; ++i)
      if (root[i] == c1 || root[i] == c2) {
        root[i] = c1;
        if (++len[i] > longest) longest = len[i];
      }
  }
  return longest;
}

// ---- codes ---------------------------------------------------------------------------------------------------------------------------
// bits[l]: the codes of l bits, l = 1 .. longest (bits[0] = 0; kLenMax + 1 words).  libjpeg's fold: while a length above 16 holds codes,
// two of them go: one takes their prefix (a bit shorter), the other hangs with a code of the deepest shorter length j that has one, both
// at j + 1.  Then the reserved symbol's code, the longest, is taken away.  (libjpeg gives up above 32 bits; this folds any depth.)
RHCCQ_JPEG_HD void fold_bits(uint32_t* bits, int longest) {
  for (int i = longest; i > 16; --i)
    while (bits[i] > 0) {
      int j = i - 2;
      while (j > 0 && bits[j] == 0) --j;
      if (j == 0 || bits[i] < 2) return;                    // (no lengths of a full code tree)
      bits[i] -= 2, ++bits[i - 1], bits[j + 1] += 2, --bits[j];
    }
  int i = 16;
  while (i > 0 && bits[i] == 0) --i;
  if (i > 0) --bits[i];
}
// huffval lists the symbols by length, then by value: the order of this key (a symbol without a count last)
RHCCQ_JPEG_HD uint32_t key_of(int32_t len, int sym) { return len > 0 ? (uint32_t)len << 8 | (uint32_t)sym : kNone; }
// the canonical code of huffval's entry p (below the number of codes) from the folded bits[1 .. 16]
RHCCQ_JPEG_HD void code_of_rank(const uint32_t* bits, int p, uint16_t* code, uint8_t* len) {
  uint32_t first = 0, at = 0;
  *code = 0, *len = 0;
  for (int l = 1; l <= 16; ++l) {
    if ((uint32_t)p < at + bits[l]) {
      *code = (uint16_t)(first + ((uint32_t)p - at));
      *len = (uint8_t)l;
      return;
    }
    first = (first + bits[l]) << 1, at += bits[l];
  }
}

// ---- header --------------------------------------------------------------------------------------------------------------------------
// tables_build's header: SOI and APP0 (20 bytes), the DQT segments (69 each), SOF0, then the DHT segments; behind them DRI (6, with an
// interval) and SOS to the header's end
struct Plan {
  int32_t n_tables, dht_at, tail_len;
};
RHCCQ_JPEG_HD Plan plan_of(const Frame& f) {
  const int nt = f.g.n_comp == 1 ? 1 : 2;
  return Plan{2 * nt, 20 + 69 * nt + 10 + 3 * f.g.n_comp, (f.g.R ? 6 : 0) + 8 + 2 * f.g.n_comp};
}
// a DHT segment: ffc4, its length 19 + codes, class << 4 | table, bits[1 .. 16], huffval.  -> where table t's starts; t = n_tables:
// where DRI / SOS go
RHCCQ_JPEG_HD int dht_at(const Plan& p, const int32_t* n_codes, int t) {
  int at = p.dht_at;
  for (int u = 0; u < t; ++u) at += 21 + n_codes[u];
  return at;
}
// where the input header's DRI / SOS start: its last tail_len bytes
RHCCQ_JPEG_HD int tail_of(const Plan& p, int32_t header_len) {
  const int hl = header_len < 0 ? 0 : header_len > kHeaderMax ? kHeaderMax : header_len;
  return hl < p.tail_len ? 0 : hl - p.tail_len;
}

// ---- the serial form -----------------------------------------------------------------------------------------------------------------
// counts and the struct of tables_build -> the struct with the counts' own codes.  A header that would pass kHeaderMax (more symbols
// than a scan can hold) is left out: header_len 0
inline void huffman_serial(const Frame& f, const uint32_t counts[4][256], const Tables& in, Tables* out) {
  const Plan p = plan_of(f);
  memset(out, 0, sizeof *out);
  memcpy(out->div, in.div, sizeof in.div);
  int32_t n_codes[4] = {0, 0, 0, 0}, len[4][257];
  uint32_t bits[4][kLenMax + 1];
  uint8_t vals[4][256];
  for (int t = 0; t < p.n_tables; ++t) {
    uint32_t freq[257];
    memcpy(freq, counts[t], 256 * sizeof(uint32_t));
    const int longest = merge_serial(freq, len[t]);
    memset(bits[t], 0, sizeof bits[t]);
    for (int i = 0; i <= 256; ++i) ++bits[t][len[t][i]];
    bits[t][0] = 0;
    fold_bits(bits[t], longest);
    for (int s = 0; s < 256; ++s) {
      if (!len[t][s]) continue;
      int rank = 0;
      for (int o = 0; o < 256; ++o) rank += key_of(len[t][o], o) < key_of(len[t][s], s);
      code_of_rank(bits[t], rank, &out->code[t][s], &out->len[t][s]);
      vals[t][rank] = (uint8_t)s;
      ++n_codes[t];
    }
  }
  const int tail_to = dht_at(p, n_codes, p.n_tables), tail_from = tail_of(p, in.header_len);
  if (tail_to + p.tail_len > kHeaderMax) return;
  memcpy(out->header, in.header, (size_t)p.dht_at);
  for (int t = 0; t < p.n_tables; ++t) {
    uint8_t* h = out->header + dht_at(p, n_codes, t);
    h[0] = 0xFF, h[1] = 0xC4, h[2] = (uint8_t)((19 + n_codes[t]) >> 8), h[3] = (uint8_t)((19 + n_codes[t]) & 255), h[4] = (uint8_t)((t & 1) << 4 | t >> 1);
    for (int l = 1; l <= 16; ++l) h[4 + l] = (uint8_t)bits[t][l];
    memcpy(h + 21, vals[t], (size_t)n_codes[t]);
  }
  memcpy(out->header + tail_to, in.header + tail_from, (size_t)p.tail_len);
  out->header_len = tail_to + p.tail_len;
}

}  // namespace jpego
}  // namespace rhccq
