// zlib level 9 on the device, byte for byte: the stream zlib 1.2.11's compress(data, 9) returns (deflate_slow with
// max_chain 4096, good 32, lazy 258, nice 258; windowBits 15, memLevel 8, the default strategy; trees.c's block rules).
// zlib_deflate.hip stays the fast, format-compatible encoder; this one is for files byte-identical to the host path.
//
// zlib's parse is serial, but every input to it is a function of the position alone:
//   * every position p <= n-3 is inserted into the 15-bit hash chains whatever the parse does, so the candidates of p are
//     the earlier positions with the same hash, most recent first (prev[] below); window index 0 reads as NIL, which only
//     matters for position 0 and for the head at distance 32506 of the one node where an end-of-input slide can land;
//   * the longest_match walk of p depends on the pending match length only through the chain limit (1024 candidates when
//     it is >= 32, else 4096) and through "longer than the pending match", so one walk records both answers;
//   * the window slides at the first loop top with strstart >= 65275 (window-relative) while input is left to read, and
//     at the first loop top with strstart >= 65274 and lookahead < 262 at the end: the slide base of a node is z9_base(p, n).
// So the lazy parse is a successor function over (position, state), state in {fresh, pending literal, pending match of
// the 4096-candidate walk at p-1, pending match of the 1024-candidate walk at p-1}.
//
// Pipeline of one rhccq_zlib9_compress call (every launch on the context stream, all memory in the caller's workspace):
//   words_zero   clear the packing words and the statistics; deflate_core.h
//   hash_chain_kernel<hash3>   one wave per 64 KiB: prev[p] = distance to the nearest earlier position with the same zlib hash
//                (0: none in 32 KiB); deflate_core.h
//   z9_search    one thread per position: the chain walk, (length, distance) after 1024 and after 4096 candidates
//   z9_seg       one workgroup per 4 KiB segment: successors of its 4 x 4096 nodes, pointer jumping in LDS until every node
//                points past the segment: exit node and symbol count of each of the 258 x 4 possible entry nodes
//   z9_link      one lane: the real parse's entry node and first symbol of every segment, the symbol count
//   z9_walk      one thread per segment: the parse from its entry node, symbols written at their ranks
//   adler_partials_kernel<kAdler>   one workgroup per 4 KiB: Adler-32 partial sums; deflate_core.h
//   z9_block     one workgroup per block of 16 383 symbols: histograms, then zlib's build_tree / gen_bitlen / gen_codes,
//                build_bl_tree and _tr_flush_block's choice of stored / fixed / dynamic
//   z9_offsets   one lane: bit offset of every block, zlib header, Adler-32 trailer, length
//   z9_emit      one workgroup per block: block header and trees (lane 0), symbols at their bit offsets (exclusive scan),
//                or the stored bytes
//   words_copy   packing words -> the caller's output buffer; deflate_core.h
// rhccq_zlib9_compress_host runs the same functions serially (the search only at the nodes the parse visits, as zlib does).
#include "deflate_core.h"
#include "rhccq_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#define Z9_HD __host__ __device__ inline

namespace z9 {

using namespace rhccq::deflate;            // the symbol algebra, Adler-32, kHashChunk and the shared kernels
using rhccq::align256;

constexpr int kWSize = 32768;
constexpr int kMaxDist = kWSize - 262;     // MAX_DIST: 32 506
constexpr int kTooFar = 4096;
constexpr int kNice = 258;
constexpr int kChainLong = 4096, kChainShort = 1024, kGood = 32;
constexpr int kBlockSyms = 16383;          // lit_bufsize - 1: a block is flushed after this many symbols
constexpr int kSeg = 4096;                 // positions of a z9_seg / z9_walk segment
constexpr int kEntries = 258 * 4;          // possible entry nodes of a segment: the first node at or past its start
constexpr int kAdler = 4096;
constexpr int kHeap = 2 * 286 + 1;         // HEAP_SIZE
constexpr int64_t kMaxIn = ((int64_t)1 << 31) - 1;

// statistics (int64) kept in the workspace
enum { ST_CAND = 0, ST_NODES, ST_ROUNDS, ST_STORED, ST_FIXED, ST_DYN, ST_N };

struct Block {
  int32_t type;          // 0 stored, 1 fixed, 2 dynamic (= BTYPE)
  int32_t last;
  int32_t nsym;
  int32_t lcodes, dcodes, blcodes;
  int64_t sym0;          // first symbol
  int64_t start, len;    // input bytes [start, start + len)
  int64_t bits;          // fixed / dynamic: bits after the 3-bit header (tree description + symbols + end of block)
  int64_t hdr_bits;      // dynamic: bits of the tree description
  uint32_t lcode[286];   // bit-reversed code | length << 16
  uint32_t dcode[30];
  uint32_t blcode[19];
  uint16_t llen[287];    // code lengths for send_tree (guard entry after max_code)
  uint16_t dlen[31];
};

Z9_HD uint32_t hash3(const uint8_t* in, int64_t p) {
  return (((uint32_t)in[p] << 10) ^ ((uint32_t)in[p + 1] << 5) ^ (uint32_t)in[p + 2]) & 0x7FFFu;
}

// window base (absolute position of window index 0) at the loop top of node p
Z9_HD int64_t base_at(int64_t p, int64_t n) {
  const int64_t k1 = n > 65536 ? (n - 65536 + kWSize - 1) / kWSize : 0;   // slides while input is left to read
  const int64_t k2 = p >= 65275 ? (p - 65275) / kWSize + 1 : 0;
  const int64_t k = k1 < k2 ? k1 : k2;
  int64_t b = k * kWSize;
  if (k == k1 && p > n - 262 && p - b >= 65274) b += kWSize;              // the slide at the end of the input
  return b;
}

// the node where an end-of-input slide can make the head at distance 32 506 read as NIL (-1: none)
Z9_HD int64_t nil_head_node(int64_t n) {
  const int64_t k1 = n > 65536 ? (n - 65536 + kWSize - 1) / kWSize : 0;
  const int64_t p = k1 * kWSize + 65274;
  return (p > n - 262 && p <= n - 3) ? p : -1;
}

// longest_match of p: r1 / r4 = length << 16 | distance after 1024 / 4096 candidates, TOO_FAR applied, 0: none.
// Returns the number of candidates examined.
Z9_HD int search(const uint8_t* in, int64_t n, const uint16_t* prev, int64_t p, int64_t pnil, uint32_t& r1, uint32_t& r4) {
  r1 = r4 = 0;
  if (p > n - 3) return 0;
  const int d0 = prev[p];
  if (!d0 || d0 > kMaxDist || p - d0 <= 0 || (p == pnil && d0 == kMaxDist)) return 0;
  const int64_t look = n - p;
  const int nice = look < kNice ? (int)look : kNice;
  const int64_t limit = p > kMaxDist ? p - kMaxDist : 0;
  const uint8_t* s = in + p;
  int best = 2;
  int64_t bq = -1;
  int64_t q = p - d0;
  int c = 0;
  uint32_t b1 = 0;
  bool have1 = false;
  for (;;) {
    ++c;
    const uint8_t* m = in + q;
    if (m[best] == s[best] && m[best - 1] == s[best - 1] && m[0] == s[0] && m[1] == s[1]) {
      int len = 2;
      while (len < nice && m[len] == s[len]) ++len;
      if (len > best) {
        best = len;
        bq = q;
        if (len >= nice) break;
      }
    }
    if (c == kChainShort) {
      b1 = (uint32_t)best << 16 | (uint32_t)(bq >= 0 ? p - bq : 0);
      have1 = true;
    }
    if (c == kChainLong) break;
    const int d = prev[q];
    if (!d) break;
    q -= d;
    if (q <= limit) break;
  }
  uint32_t b4 = (uint32_t)best << 16 | (uint32_t)(bq >= 0 ? p - bq : 0);
  if (!have1) b1 = b4;
  auto fix = [](uint32_t v) -> uint32_t {
    const uint32_t L = v >> 16, D = v & 0xFFFF;
    if (L < 3 || (L == 3 && D > (uint32_t)kTooFar)) return 0u;
    return v;
  };
  r1 = fix(b1);
  r4 = fix(b4);
  return c;
}

// one loop top of deflate_slow at node (p, s), p < n.  s: 0 fresh, 1 pending literal, 2 / 3 pending match of the
// 4096 / 1024-candidate walk at p-1.  -> next node; returns 1 when a symbol is tallied (sym_pos = p - 1, sym_ld = 0 for
// a literal, length << 16 | distance for a match).
Z9_HD int step(const uint32_t* r1, const uint32_t* r4, int64_t p, int s, int64_t& np, int& ns, uint32_t& sym_ld) {
  int P = 2, D = 0;
  if (s >= 2 && p > 0) {
    const uint32_t v = (s == 2 ? r4 : r1)[p - 1];
    if (v) {
      P = (int)(v >> 16);
      D = (int)(v & 0xFFFF);
    }
  }
  const bool shortc = P >= kGood;
  int M = 2;
  if (P < kNice) {
    const uint32_t v = (shortc ? r1 : r4)[p];
    if (v) M = (int)(v >> 16);
  }
  if (P >= 3 && M <= P) {
    sym_ld = (uint32_t)P << 16 | (uint32_t)D;
    np = p - 1 + P;
    ns = 0;
    return 1;
  }
  np = p + 1;
  ns = M >= 3 ? (shortc ? 3 : 2) : 1;
  sym_ld = 0;
  return s != 0 ? 1 : 0;
}

// ---- trees.c ---------------------------------------------------------------------------------------------------

// len_code / dist_code (zlib's _length_code / d_code), len_extra / dist_extra / codelen_extra (extra_lbits / extra_dbits / extra_blbits),
// fixed_litlen_bits (static_ltree), codelen_order (bl_order) and bit_reverse (bi_reverse) are deflate_core.h's

struct Tree {
  uint32_t freq[kHeap];
  uint16_t len[kHeap + 1];
  uint16_t dad[kHeap];
  uint16_t code[kHeap];
};

struct Work {
  Tree lt, dt, bt;
  int heap[kHeap];
  int heap_len, heap_max;
  uint8_t depth[kHeap];
  int bl_count[16];
  uint64_t opt_len, static_len;
  int lmax, dmax, bmax;
};

Z9_HD bool smaller(const Tree& t, const Work& w, int a, int b) {
  return t.freq[a] < t.freq[b] || (t.freq[a] == t.freq[b] && w.depth[a] <= w.depth[b]);
}

Z9_HD void pqdownheap(Work& w, const Tree& t, int k) {
  const int v = w.heap[k];
  int j = k << 1;
  while (j <= w.heap_len) {
    if (j < w.heap_len && smaller(t, w, w.heap[j + 1], w.heap[j])) j++;
    if (smaller(t, w, v, w.heap[j])) break;
    w.heap[k] = w.heap[j];
    k = j;
    j <<= 1;
  }
  w.heap[k] = v;
}

// which: 0 literal/length (static lengths), 1 distance (static length 5), 2 code lengths (no static tree)
Z9_HD void gen_bitlen(Work& w, Tree& t, int max_code, int which) {
  const int max_length = which == 2 ? 7 : 15;
  for (int b = 0; b <= 15; ++b) w.bl_count[b] = 0;
  t.len[w.heap[w.heap_max]] = 0;
  int overflow = 0;
  int h;
  for (h = w.heap_max + 1; h < kHeap; h++) {
    const int n = w.heap[h];
    int bits = t.len[t.dad[n]] + 1;
    if (bits > max_length) bits = max_length, overflow++;
    t.len[n] = (uint16_t)bits;
    if (n > max_code) continue;
    w.bl_count[bits]++;
    int xbits = 0;
    if (which == 0 && n >= 257) xbits = len_extra(n - 257);
    if (which == 1) xbits = dist_extra(n);
    if (which == 2) xbits = codelen_extra(n);
    const uint64_t f = t.freq[n];
    w.opt_len += f * (uint64_t)(bits + xbits);
    if (which == 0) w.static_len += f * (uint64_t)(fixed_litlen_bits(n) + xbits);
    if (which == 1) w.static_len += f * (uint64_t)(5 + xbits);
  }
  if (overflow == 0) return;
  do {
    int bits = max_length - 1;
    while (w.bl_count[bits] == 0) bits--;
    w.bl_count[bits]--;
    w.bl_count[bits + 1] += 2;
    w.bl_count[max_length]--;
    overflow -= 2;
  } while (overflow > 0);
  for (int bits = max_length; bits != 0; bits--) {
    int n = w.bl_count[bits];
    while (n != 0) {
      const int m = w.heap[--h];
      if (m > max_code) continue;
      if ((int)t.len[m] != bits) {
        w.opt_len += ((uint64_t)bits - (uint64_t)t.len[m]) * (uint64_t)t.freq[m];
        t.len[m] = (uint16_t)bits;
      }
      n--;
    }
  }
}

Z9_HD void gen_codes(Tree& t, int max_code, const int* bl_count) {
  uint32_t next[16];
  uint32_t code = 0;
  for (int b = 1; b <= 15; b++) {
    code = (code + (uint32_t)bl_count[b - 1]) << 1;
    next[b] = code;
  }
  for (int n = 0; n <= max_code; n++) {
    const int l = t.len[n];
    if (l == 0) continue;
    t.code[n] = (uint16_t)bit_reverse(next[l]++, l);
  }
}

Z9_HD int build_tree(Work& w, Tree& t, int elems, int which) {
  w.heap_len = 0;
  w.heap_max = kHeap;
  int max_code = -1;
  for (int n = 0; n < elems; n++) {
    if (t.freq[n] != 0) {
      w.heap[++w.heap_len] = max_code = n;
      w.depth[n] = 0;
    } else {
      t.len[n] = 0;
    }
  }
  while (w.heap_len < 2) {
    const int node = w.heap[++w.heap_len] = (max_code < 2 ? ++max_code : 0);
    t.freq[node] = 1;
    w.depth[node] = 0;
    w.opt_len--;
    if (which == 0) w.static_len -= (uint64_t)fixed_litlen_bits(node);
    if (which == 1) w.static_len -= 5;
  }
  for (int n = w.heap_len / 2; n >= 1; n--) pqdownheap(w, t, n);
  int node = elems;
  do {
    const int n = w.heap[1];
    w.heap[1] = w.heap[w.heap_len--];
    pqdownheap(w, t, 1);
    const int m = w.heap[1];
    w.heap[--w.heap_max] = n;
    w.heap[--w.heap_max] = m;
    t.freq[node] = t.freq[n] + t.freq[m];
    w.depth[node] = (uint8_t)((w.depth[n] >= w.depth[m] ? w.depth[n] : w.depth[m]) + 1);
    t.dad[n] = t.dad[m] = (uint16_t)node;
    w.heap[1] = node++;
    pqdownheap(w, t, 1);
  } while (w.heap_len >= 2);
  w.heap[--w.heap_max] = w.heap[1];
  gen_bitlen(w, t, max_code, which);
  gen_codes(t, max_code, w.bl_count);
  return max_code;
}

Z9_HD void scan_tree(Work& w, Tree& t, int max_code) {
  int prevlen = -1, nextlen = t.len[0], count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) max_count = 138, min_count = 3;
  t.len[max_code + 1] = 0xFFFF;
  for (int n = 0; n <= max_code; n++) {
    const int curlen = nextlen;
    nextlen = t.len[n + 1];
    if (++count < max_count && curlen == nextlen) {
      continue;
    } else if (count < min_count) {
      w.bt.freq[curlen] += count;
    } else if (curlen != 0) {
      if (curlen != prevlen) w.bt.freq[curlen]++;
      w.bt.freq[16]++;
    } else if (count <= 10) {
      w.bt.freq[17]++;
    } else {
      w.bt.freq[18]++;
    }
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) max_count = 138, min_count = 3;
    else if (curlen == nextlen) max_count = 6, min_count = 3;
    else max_count = 7, min_count = 4;
  }
}

// bit writer: OR into 32-bit words (disjoint bits), or count only when w == nullptr
Z9_HD void put_bits(uint32_t* w, int64_t nw, uint64_t off, uint32_t v, int nb) {
  if (!w || nb <= 0) return;
  const uint64_t q = off >> 5;
  const int sh = (int)(off & 31);
  const uint64_t lo = (uint64_t)v << sh;
#ifdef __HIP_DEVICE_COMPILE__
  if ((int64_t)q < nw && (uint32_t)lo) atomicOr(w + q, (uint32_t)lo);
  if (sh + nb > 32 && (int64_t)q + 1 < nw) atomicOr(w + q + 1, (uint32_t)(lo >> 32));
#else
  if ((int64_t)q < nw) w[q] |= (uint32_t)lo;
  if (sh + nb > 32 && (int64_t)q + 1 < nw) w[q + 1] |= (uint32_t)(lo >> 32);
#endif
}

Z9_HD uint64_t send_tree(const uint16_t* len, int max_code, const uint32_t* bl, uint32_t* w, int64_t nw, uint64_t off) {
  int prevlen = -1, nextlen = len[0], count = 0, max_count = 7, min_count = 4;
  if (nextlen == 0) max_count = 138, min_count = 3;
  auto code = [&](int c) {
    put_bits(w, nw, off, bl[c] & 0xFFFF, (int)(bl[c] >> 16));
    off += bl[c] >> 16;
  };
  auto bits = [&](uint32_t v, int nb) {
    put_bits(w, nw, off, v, nb);
    off += (uint64_t)nb;
  };
  for (int n = 0; n <= max_code; n++) {
    const int curlen = nextlen;
    nextlen = len[n + 1];
    if (++count < max_count && curlen == nextlen) {
      continue;
    } else if (count < min_count) {
      do { code(curlen); } while (--count != 0);
    } else if (curlen != 0) {
      if (curlen != prevlen) {
        code(curlen);
        count--;
      }
      code(16);
      bits((uint32_t)(count - 3), 2);
    } else if (count <= 10) {
      code(17);
      bits((uint32_t)(count - 3), 3);
    } else {
      code(18);
      bits((uint32_t)(count - 11), 7);
    }
    count = 0;
    prevlen = curlen;
    if (nextlen == 0) max_count = 138, min_count = 3;
    else if (curlen == nextlen) max_count = 6, min_count = 3;
    else max_count = 7, min_count = 4;
  }
  return off;
}

// _tr_flush_block's trees and choice for one block whose histograms are in w.lt.freq[0..286) / w.dt.freq[0..30)
// (end of block not yet counted).  stored_ok: block_start >= 0 in zlib's window.
Z9_HD void plan_block(Work& w, Block& B, bool stored_ok) {
  for (int s = 286; s < kHeap; ++s) w.lt.freq[s] = 0;
  for (int s = 30; s < kHeap; ++s) w.dt.freq[s] = 0;
  for (int s = 0; s < kHeap; ++s) w.bt.freq[s] = 0;
  w.lt.freq[256] += 1;
  w.opt_len = w.static_len = 0;
  const int lmax = build_tree(w, w.lt, 286, 0);
  const int dmax = build_tree(w, w.dt, 30, 1);
  scan_tree(w, w.lt, lmax);
  scan_tree(w, w.dt, dmax);
  build_tree(w, w.bt, 19, 2);
  int max_blindex;
  for (max_blindex = 18; max_blindex >= 3; max_blindex--)
    if (w.bt.len[codelen_order(max_blindex)] != 0) break;
  w.opt_len += 3 * ((uint64_t)max_blindex + 1) + 5 + 5 + 4;
  uint64_t opt_lenb = (w.opt_len + 3 + 7) >> 3;
  const uint64_t static_lenb = (w.static_len + 3 + 7) >> 3;
  if (static_lenb <= opt_lenb) opt_lenb = static_lenb;
  B.lcodes = lmax + 1;
  B.dcodes = dmax + 1;
  B.blcodes = max_blindex + 1;
  if ((uint64_t)B.len + 4 <= opt_lenb && stored_ok) {
    B.type = 0;
    B.bits = 0;
    B.hdr_bits = 0;
  } else if (static_lenb == opt_lenb) {
    B.type = 1;
    B.bits = (int64_t)w.static_len;
    B.hdr_bits = 0;
    uint16_t sl[288];
    int cnt[16];
    for (int b = 0; b < 16; ++b) cnt[b] = 0;
    for (int s = 0; s < 288; ++s) cnt[sl[s] = (uint16_t)fixed_litlen_bits(s)]++;
    uint32_t next[16], code = 0;
    cnt[0] = 0;
    for (int b = 1; b <= 15; b++) {
      code = (code + (uint32_t)cnt[b - 1]) << 1;
      next[b] = code;
    }
    for (int s = 0; s < 288; ++s) {
      const uint32_t c = bit_reverse(next[sl[s]]++, sl[s]);
      if (s < 286) B.lcode[s] = c | (uint32_t)sl[s] << 16;
    }
    for (int s = 0; s < 30; ++s) B.dcode[s] = bit_reverse((uint32_t)s, 5) | 5u << 16;
  } else {
    B.type = 2;
    B.bits = (int64_t)w.opt_len;
    for (int s = 0; s < 286; ++s) B.lcode[s] = s <= lmax && w.lt.len[s] ? (w.lt.code[s] | (uint32_t)w.lt.len[s] << 16) : 0u;
    for (int s = 0; s < 30; ++s) B.dcode[s] = s <= dmax && w.dt.len[s] ? (w.dt.code[s] | (uint32_t)w.dt.len[s] << 16) : 0u;
    for (int s = 0; s < 19; ++s) B.blcode[s] = w.bt.len[s] ? (w.bt.code[s] | (uint32_t)w.bt.len[s] << 16) : 0u;
    for (int s = 0; s <= lmax + 1; ++s) B.llen[s] = w.lt.len[s];
    for (int s = 0; s <= dmax + 1; ++s) B.dlen[s] = w.dt.len[s];
    uint64_t off = 14 + 3 * (uint64_t)B.blcodes;
    off = send_tree(B.llen, lmax, B.blcode, nullptr, 0, off);
    off = send_tree(B.dlen, dmax, B.blcode, nullptr, 0, off);
    B.hdr_bits = (int64_t)off;
  }
}

Z9_HD int sym_bits(const Block& B, uint32_t ld, uint8_t lit) {
  if (!ld) return (int)(B.lcode[lit] >> 16);
  int le, lv, de, dv;
  const int lc = len_code((int)(ld >> 16), le, lv);
  const int dc = dist_code((int)(ld & 0xFFFF), de, dv);
  return (int)(B.lcode[257 + lc] >> 16) + le + (int)(B.dcode[dc] >> 16) + de;
}

Z9_HD uint64_t put_sym(const Block& B, uint32_t ld, uint8_t lit, uint32_t* w, int64_t nw, uint64_t off) {
  if (!ld) {
    const uint32_t c = B.lcode[lit];
    put_bits(w, nw, off, c & 0xFFFF, (int)(c >> 16));
    return off + (c >> 16);
  }
  int le, lv, de, dv;
  const int lc = len_code((int)(ld >> 16), le, lv);
  const int dc = dist_code((int)(ld & 0xFFFF), de, dv);
  const uint32_t c = B.lcode[257 + lc], d = B.dcode[dc];
  put_bits(w, nw, off, c & 0xFFFF, (int)(c >> 16));
  off += c >> 16;
  put_bits(w, nw, off, (uint32_t)lv, le);
  off += le;
  put_bits(w, nw, off, d & 0xFFFF, (int)(d >> 16));
  off += d >> 16;
  put_bits(w, nw, off, (uint32_t)dv, de);
  return off + de;
}

Z9_HD void put_byte(uint32_t* w, int64_t nw, uint64_t pos, uint32_t b) { put_bits(w, nw, pos * 8, b & 255u, 8); }

// block header, tree description and (stored) LEN / NLEN; returns the bit offset of the first symbol
Z9_HD uint64_t block_header(const Block& B, uint64_t off, uint32_t* w, int64_t nw) {
  put_bits(w, nw, off, (uint32_t)(B.type << 1 | B.last), 3);
  off += 3;
  if (B.type == 0) {
    const uint64_t a = (off + 7) >> 3;
    const uint32_t L = (uint32_t)B.len & 0xFFFF;
    put_bits(w, nw, a * 8, L | (~L & 0xFFFF) << 16, 32);
    return (a + 4) * 8;
  }
  if (B.type == 2) {
    put_bits(w, nw, off, (uint32_t)(B.lcodes - 257), 5);
    put_bits(w, nw, off + 5, (uint32_t)(B.dcodes - 1), 5);
    put_bits(w, nw, off + 10, (uint32_t)(B.blcodes - 4), 4);
    off += 14;
    for (int r = 0; r < B.blcodes; ++r, off += 3) put_bits(w, nw, off, B.blcode[codelen_order(r)] >> 16, 3);
    off = send_tree(B.llen, B.lcodes - 1, B.blcode, w, nw, off);
    off = send_tree(B.dlen, B.dcodes - 1, B.blcode, w, nw, off);
  }
  return off;
}

// bit offset of every block after the 2-byte header; returns the stream length (header, blocks, Adler-32)
Z9_HD int64_t block_offsets(const Block* blocks, int64_t nb, int64_t* boff) {
  uint64_t off = 16;
  for (int64_t b = 0; b < nb; ++b) {
    const Block& B = blocks[b];
    boff[b] = (int64_t)off;
    if (B.type == 0) off = ((off + 3 + 7) & ~(uint64_t)7) + 32 + 8 * (uint64_t)B.len;
    else off += 3 + (uint64_t)B.bits;
  }
  return (int64_t)((off + 7) >> 3) + 4;
}

Z9_HD void put_frame(uint32_t* w, int64_t nw, int64_t len, uint32_t adler) {
  put_bits(w, nw, 0, 0xDA78u, 16);                   // CMF 0x78, FLG 0xDA: level 9 (FLEVEL 3), 0x78DA % 31 == 0
  for (int k = 0; k < 4; ++k) put_byte(w, nw, (uint64_t)(len - 4 + k), adler >> (24 - 8 * k));
}

Z9_HD int64_t bound(int64_t n) {
  const int64_t zb = n + (n >> 12) + (n >> 14) + (n >> 25) + 13;          // compressBound
  const int64_t ours = n + (n >> 3) + 4 * (n / kBlockSyms + 2) + 16;      // <= 9 bits a byte + block overhead
  return zb > ours ? zb : ours;
}

// ---- layout ----------------------------------------------------------------------------------------------------

struct Layout {
  int64_t nseg, nbmax, nad, words, bnd;
  int64_t o_prev, o_r1, o_r4, o_summ, o_sent, o_sbase, o_misc, o_spos, o_sld, o_blk, o_boff, o_adl, o_words, o_stats, total;
};

inline Layout layout(int64_t n) {
  Layout L;
  L.nseg = (n + kSeg - 1) / kSeg;
  L.nbmax = n / kBlockSyms + 2;
  L.nad = n > 0 ? (n + kAdler - 1) / kAdler : 1;
  L.bnd = bound(n);
  L.words = (L.bnd + 3) / 4 + 2;
  int64_t o = 0;
  L.o_prev = o; o = align256(o + 2 * (n + 1));
  L.o_r1 = o; o = align256(o + 4 * (n + 1));
  L.o_r4 = o; o = align256(o + 4 * (n + 1));
  L.o_summ = o; o = align256(o + 4 * kEntries * (L.nseg + 1));
  L.o_sent = o; o = align256(o + 4 * (L.nseg + 1));
  L.o_sbase = o; o = align256(o + 8 * (L.nseg + 1));
  L.o_misc = o; o = align256(o + 8 * 8);
  L.o_spos = o; o = align256(o + 4 * (n + 1));
  L.o_sld = o; o = align256(o + 4 * (n + 1));
  L.o_blk = o; o = align256(o + (int64_t)sizeof(Block) * L.nbmax);
  L.o_boff = o; o = align256(o + 8 * L.nbmax);
  L.o_adl = o; o = align256(o + 8 * L.nad);
  L.o_words = o; o = align256(o + 4 * L.words);
  L.o_stats = o; o = align256(o + 8 * ST_N);
  L.total = o;
  return L;
}

// ---- kernels ---------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void z9_search(const uint8_t* __restrict__ in, int64_t n, const uint16_t* __restrict__ prev,
                                                 uint32_t* __restrict__ r1, uint32_t* __restrict__ r4, int64_t* __restrict__ stats) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int c = 0;
  if (p < n) {
    uint32_t a, b;
    c = search(in, n, prev, p, nil_head_node(n), a, b);
    r1[p] = a;
    r4[p] = b;
  }
  const unsigned long long s = rhccq::wave_sum((unsigned long long)c);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)&stats[ST_CAND], s);
}

// node code inside a segment: (p - S) * 4 + s; past it: 0x8000 | (p - E) * 4 + s
__global__ __launch_bounds__(256) void z9_seg(const uint32_t* __restrict__ r1, const uint32_t* __restrict__ r4, int64_t n,
                                              uint32_t* __restrict__ summ, int64_t* __restrict__ stats) {
  __shared__ uint16_t nx[2][kSeg * 4];
  __shared__ uint16_t ct[2][kSeg * 4];
  const int64_t S = (int64_t)blockIdx.x * kSeg;
  const int64_t E = S + kSeg < n ? S + kSeg : n;
  const int m = (int)(E - S) * 4;
  for (int v = threadIdx.x; v < m; v += 256) {
    int64_t np;
    int ns;
    uint32_t ld;
    const int e = step(r1, r4, S + (v >> 2), v & 3, np, ns, ld);
    nx[0][v] = np >= E ? (uint16_t)(0x8000 | ((np - E) * 4 + ns)) : (uint16_t)((np - S) * 4 + ns);
    ct[0][v] = (uint16_t)e;
  }
  __syncthreads();
  int cur = 0, rounds = 0;
  for (;;) {
    int changed = 0;
    for (int v = threadIdx.x; v < m; v += 256) {
      const uint16_t a = nx[cur][v];
      if (!(a & 0x8000)) {
        nx[cur ^ 1][v] = nx[cur][a];
        ct[cur ^ 1][v] = (uint16_t)(ct[cur][v] + ct[cur][a]);
        changed = 1;
      } else {
        nx[cur ^ 1][v] = a;
        ct[cur ^ 1][v] = ct[cur][v];
      }
    }
    cur ^= 1;
    const int any = __syncthreads_or(changed);
    if (!any) break;
    ++rounds;
  }
  // an entry at or past E (only the end of the input, in a last segment shorter than 258 positions) is its own exit
  for (int e = threadIdx.x; e < kEntries; e += 256)
    summ[(int64_t)blockIdx.x * kEntries + e] =
        e < m ? ((uint32_t)(nx[cur][e] & 0x7FFF) | (uint32_t)ct[cur][e] << 11) : (uint32_t)((S + (e >> 2) - E) * 4 + (e & 3));
  if (threadIdx.x == 0) atomicMax((unsigned long long*)&stats[ST_ROUNDS], (unsigned long long)rounds);
}

// misc: [0] symbols, [1] final literal (0 / 1), [2] blocks
__global__ void z9_link(const uint32_t* __restrict__ summ, int64_t nseg, uint32_t* __restrict__ sent, int64_t* __restrict__ sbase,
                        int64_t* __restrict__ misc) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  uint32_t e = 0;
  int64_t tot = 0;
  for (int64_t b = 0; b < nseg; ++b) {
    sent[b] = e;
    sbase[b] = tot;
    const uint32_t w = summ[b * kEntries + e];
    tot += w >> 11;
    e = w & 0x7FF;
  }
  const int64_t fin = (e & 3) == 1 ? 1 : 0;         // the pending literal at the end of the input
  tot += fin;
  const int64_t loop = tot - fin;
  misc[0] = tot;
  misc[1] = fin;
  misc[2] = loop / kBlockSyms + 1;
}

__global__ __launch_bounds__(64) void z9_walk(const uint32_t* __restrict__ r1, const uint32_t* __restrict__ r4, int64_t n, int64_t nseg,
                                              const uint32_t* __restrict__ sent, const int64_t* __restrict__ sbase,
                                              const int64_t* __restrict__ misc, uint32_t* __restrict__ spos, uint32_t* __restrict__ sld,
                                              int64_t* __restrict__ stats) {
  const int64_t b = (int64_t)blockIdx.x * 64 + threadIdx.x;
  unsigned long long nodes = 0;
  if (b < nseg) {
    const int64_t S = b * kSeg, E = S + kSeg < n ? S + kSeg : n;
    int64_t p = S + (sent[b] >> 2);
    int s = (int)(sent[b] & 3);
    int64_t k = sbase[b];
    while (p < E) {
      int64_t np;
      int ns;
      uint32_t ld;
      if (step(r1, r4, p, s, np, ns, ld)) {
        spos[k] = (uint32_t)(p - 1);
        sld[k] = ld;
        ++k;
      }
      ++nodes;
      p = np;
      s = ns;
    }
    if (b == nseg - 1 && misc[1]) {
      spos[k] = (uint32_t)(n - 1);
      sld[k] = 0;
    }
  }
  nodes = rhccq::wave_sum(nodes);
  if (threadIdx.x == 0 && nodes) atomicAdd((unsigned long long*)&stats[ST_NODES], nodes);
}

// symbol range, input range and stored eligibility of block b (nb blocks, tot symbols)
Z9_HD void block_range(const uint32_t* spos, const uint32_t* sld, int64_t n, int64_t tot, int64_t nb, int64_t b, Block& B, bool& stored_ok) {
  B.sym0 = b * kBlockSyms;
  B.nsym = (int32_t)(b < nb - 1 ? kBlockSyms : tot - B.sym0);
  B.last = b == nb - 1;
  auto sym_end = [&](int64_t i) -> int64_t { return (int64_t)spos[i] + (sld[i] ? (int64_t)(sld[i] >> 16) : 1); };
  B.start = b == 0 ? 0 : sym_end(B.sym0 - 1);
  const int64_t end = B.last ? n : sym_end(B.sym0 + B.nsym - 1);
  B.len = end - B.start;
  const int64_t flush_node = B.last ? n : (int64_t)spos[B.sym0 + B.nsym - 1] + 1;
  stored_ok = B.start >= base_at(flush_node, n);
}

__global__ __launch_bounds__(256) void z9_block(const uint8_t* __restrict__ in, int64_t n, const uint32_t* __restrict__ spos,
                                                const uint32_t* __restrict__ sld, const int64_t* __restrict__ misc, Block* __restrict__ blocks,
                                                int64_t* __restrict__ stats) {
  __shared__ Work w;
  __shared__ uint32_t fl[286], fd[30];
  const int64_t nb = misc[2];
  const int64_t b = blockIdx.x;
  if (b >= nb) return;
  const int64_t tot = misc[0];
  for (int s = threadIdx.x; s < 286; s += 256) fl[s] = 0;
  if (threadIdx.x < 30) fd[threadIdx.x] = 0;
  __syncthreads();
  const int64_t s0 = b * kBlockSyms;
  const int64_t s1 = b < nb - 1 ? s0 + kBlockSyms : tot;
  for (int64_t i = s0 + threadIdx.x; i < s1; i += 256) {
    const uint32_t ld = sld[i];
    if (!ld) {
      atomicAdd(&fl[in[spos[i]]], 1u);
    } else {
      int le, lv, de, dv;
      atomicAdd(&fl[257 + len_code((int)(ld >> 16), le, lv)], 1u);
      atomicAdd(&fd[dist_code((int)(ld & 0xFFFF), de, dv)], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Block& B = blocks[b];
    bool ok;
    block_range(spos, sld, n, tot, nb, b, B, ok);
    for (int s = 0; s < 286; ++s) w.lt.freq[s] = fl[s];
    for (int s = 0; s < 30; ++s) w.dt.freq[s] = fd[s];
    plan_block(w, B, ok);
    atomicAdd((unsigned long long*)&stats[ST_STORED + B.type], 1ull);
  }
}

__global__ void z9_offsets(const Block* __restrict__ blocks, const int64_t* __restrict__ misc, int64_t* __restrict__ boff,
                           const uint32_t* __restrict__ adl, int64_t n, uint32_t* __restrict__ words, int64_t nw,
                           int64_t* __restrict__ out_len) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const int64_t len = block_offsets(blocks, misc[2], boff);
  put_frame(words, nw, len, adler_fold(adl, n, kAdler));
  *out_len = len;
}

constexpr int kEmitPer = (kBlockSyms + 1 + 255) / 256;

__global__ __launch_bounds__(256) void z9_emit(const uint8_t* __restrict__ in, const uint32_t* __restrict__ spos, const uint32_t* __restrict__ sld,
                                               const int64_t* __restrict__ misc, const Block* __restrict__ blocks,
                                               const int64_t* __restrict__ boff, uint32_t* __restrict__ words, int64_t nw) {
  __shared__ long long red[8];
  __shared__ unsigned long long data0;
  const int64_t b = blockIdx.x;
  if (b >= misc[2]) return;
  const Block& B = blocks[b];
  if (threadIdx.x == 0) data0 = block_header(B, (uint64_t)boff[b], words, nw);
  __syncthreads();
  if (B.type == 0) {
    const uint64_t a = data0 >> 3;
    for (int64_t k = threadIdx.x; k < B.len; k += 256) put_byte(words, nw, a + (uint64_t)k, in[B.start + k]);
    return;
  }
  const int k0 = threadIdx.x * kEmitPer;
  const int k1 = k0 + kEmitPer < B.nsym ? k0 + kEmitPer : B.nsym;
  long long bits = 0;
  for (int k = k0; k < k1; ++k) {
    const int64_t i = B.sym0 + k;
    bits += sym_bits(B, sld[i], in[spos[i]]);
  }
  long long tot;
  uint64_t off = data0 + (uint64_t)rhccq::block_exscan(bits, red, &tot);
  for (int k = k0; k < k1; ++k) {
    const int64_t i = B.sym0 + k;
    off = put_sym(B, sld[i], in[spos[i]], words, nw, off);
  }
  if (threadIdx.x == 0) {
    const uint32_t eob = B.lcode[256];
    put_bits(words, nw, data0 + (uint64_t)tot, eob & 0xFFFF, (int)(eob >> 16));
  }
}

__global__ void z9_stats_copy(const int64_t* __restrict__ src, int64_t* __restrict__ dst) {
  if (threadIdx.x < ST_N) dst[threadIdx.x] = src[threadIdx.x];
}

}  // namespace z9

extern "C" {

int rhccq_zlib9_sizes(int64_t n, int64_t* workspace_bytes, int64_t* out_bound) {
  if (n < 0 || !workspace_bytes || !out_bound) return RHCCQ_E_ARG;
  if (n > z9::kMaxIn) return RHCCQ_E_LIMIT;
  const z9::Layout L = z9::layout(n);
  *workspace_bytes = L.total;
  *out_bound = L.bnd;
  return RHCCQ_OK;
}

int rhccq_zlib9_compress(rhccq_ctx* ctx, const void* in, int64_t n, void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  using namespace z9;
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || (n > 0 && !in) || !workspace || !out || !out_len) return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib9_compress: bad argument");
  if (n > kMaxIn) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib9_compress: input of 2 GiB or more");
  const Layout L = layout(n);
  if (out_cap < L.bnd) return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib9_compress: out_cap below the bound of rhccq_zlib9_sizes");
  char* ws = (char*)workspace;
  const uint8_t* src = (const uint8_t*)in;
  uint16_t* prev = (uint16_t*)(ws + L.o_prev);
  uint32_t* r1 = (uint32_t*)(ws + L.o_r1);
  uint32_t* r4 = (uint32_t*)(ws + L.o_r4);
  uint32_t* summ = (uint32_t*)(ws + L.o_summ);
  uint32_t* sent = (uint32_t*)(ws + L.o_sent);
  int64_t* sbase = (int64_t*)(ws + L.o_sbase);
  int64_t* misc = (int64_t*)(ws + L.o_misc);
  uint32_t* spos = (uint32_t*)(ws + L.o_spos);
  uint32_t* sld = (uint32_t*)(ws + L.o_sld);
  Block* blk = (Block*)(ws + L.o_blk);
  int64_t* boff = (int64_t*)(ws + L.o_boff);
  uint32_t* adl = (uint32_t*)(ws + L.o_adl);
  uint32_t* words = (uint32_t*)(ws + L.o_words);
  int64_t* stats = (int64_t*)(ws + L.o_stats);
  hipStream_t st = ctx->stream;
  const int zgrid = (int)((L.words + 255) / 256 < 4096 ? (L.words + 255) / 256 : 4096);
  words_zero<ST_N><<<zgrid, 256, 0, st>>>(words, L.words, stats);
  if (n > 0) {
    hash_chain_kernel<hash3><<<(int)((n + kHashChunk - 1) / kHashChunk), 64, 0, st>>>(src, n, prev);
    z9_search<<<(int)((n + 255) / 256), 256, 0, st>>>(src, n, prev, r1, r4, stats);
    z9_seg<<<(int)L.nseg, 256, 0, st>>>(r1, r4, n, summ, stats);
  }
  z9_link<<<1, 64, 0, st>>>(summ, L.nseg, sent, sbase, misc);
  if (n > 0) {
    z9_walk<<<(int)((L.nseg + 63) / 64), 64, 0, st>>>(r1, r4, n, L.nseg, sent, sbase, misc, spos, sld, stats);
    adler_partials_kernel<kAdler><<<(int)L.nad, 256, 0, st>>>(src, n, adl);
  }
  z9_block<<<(int)L.nbmax, 256, 0, st>>>(src, n, spos, sld, misc, blk, stats);
  z9_offsets<<<1, 64, 0, st>>>(blk, misc, boff, adl, n, words, L.words, out_len);
  z9_emit<<<(int)L.nbmax, 256, 0, st>>>(src, spos, sld, misc, blk, boff, words, L.words);
  const int cgrid = (int)((L.bnd + 255) / 256 < 8192 ? (L.bnd + 255) / 256 : 8192);
  words_copy<<<cgrid, 256, 0, st>>>(words, L.bnd, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_zlib9_stats(rhccq_ctx* ctx, int64_t n, const void* workspace, int64_t* stats) {
  using namespace z9;
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || !workspace || !stats) return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib9_stats: bad argument");
  if (n > kMaxIn) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib9_stats: input of 2 GiB or more");
  const Layout L = layout(n);
  z9_stats_copy<<<1, 64, 0, ctx->stream>>>((const int64_t*)((const char*)workspace + L.o_stats), stats);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_zlib9_compress_host(const void* in, int64_t n, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  using namespace z9;
  if (n < 0 || (n > 0 && !in) || !out || !out_len) return RHCCQ_E_ARG;
  if (n > kMaxIn) return RHCCQ_E_LIMIT;
  const int64_t bnd = bound(n);
  if (out_cap < bnd) return RHCCQ_E_ARG;
  const uint8_t* src = (const uint8_t*)in;
  // hash chains as hash_chain_kernel<hash3> builds them
  std::vector<uint16_t> prev((size_t)n + 1, 0);
  {
    std::vector<int64_t> head(1 << 15, -1);
    for (int64_t p = 0; p + 2 < n; ++p) {
      const uint32_t h = hash3(src, p);
      const int64_t q = head[h];
      prev[p] = (uint16_t)((q >= 0 && p - q <= kWSize) ? p - q : 0);
      head[h] = p;
    }
  }
  // the parse, searching only where it lands
  std::vector<uint32_t> r1((size_t)n + 1, 0), r4((size_t)n + 1, 0);
  std::vector<uint8_t> done((size_t)n + 1, 0);
  std::vector<uint32_t> spos, sld;
  const int64_t pnil = nil_head_node(n);
  int64_t p = 0;
  int s = 0;
  while (p < n) {
    if (!done[p]) {
      search(src, n, prev.data(), p, pnil, r1[p], r4[p]);
      done[p] = 1;
    }
    int64_t np;
    int ns;
    uint32_t ld;
    if (step(r1.data(), r4.data(), p, s, np, ns, ld)) {
      spos.push_back((uint32_t)(p - 1));
      sld.push_back(ld);
    }
    p = np;
    s = ns;
  }
  const int64_t fin = s == 1 ? 1 : 0;
  if (fin) {
    spos.push_back((uint32_t)(n - 1));
    sld.push_back(0);
  }
  const int64_t tot = (int64_t)spos.size();
  const int64_t nb = (tot - fin) / kBlockSyms + 1;
  std::vector<Block> blocks((size_t)nb);
  std::vector<Work> wv(1);
  Work& w = wv[0];
  for (int64_t b = 0; b < nb; ++b) {
    Block& B = blocks[b];
    bool ok;
    block_range(spos.data(), sld.data(), n, tot, nb, b, B, ok);
    for (int k = 0; k < 286; ++k) w.lt.freq[k] = 0;
    for (int k = 0; k < 30; ++k) w.dt.freq[k] = 0;
    for (int64_t i = B.sym0; i < B.sym0 + B.nsym; ++i) {
      if (!sld[i]) {
        w.lt.freq[src[spos[i]]]++;
      } else {
        int le, lv, de, dv;
        w.lt.freq[257 + len_code((int)(sld[i] >> 16), le, lv)]++;
        w.dt.freq[dist_code((int)(sld[i] & 0xFFFF), de, dv)]++;
      }
    }
    plan_block(w, B, ok);
  }
  std::vector<int64_t> boff((size_t)nb);
  const int64_t len = block_offsets(blocks.data(), nb, boff.data());
  const int64_t nw = (bnd + 3) / 4 + 2;
  std::vector<uint32_t> words((size_t)nw, 0);
  for (int64_t b = 0; b < nb; ++b) {
    const Block& B = blocks[b];
    uint64_t off = block_header(B, (uint64_t)boff[b], words.data(), nw);
    if (B.type == 0) {
      for (int64_t k = 0; k < B.len; ++k) put_byte(words.data(), nw, (off >> 3) + (uint64_t)k, src[B.start + k]);
      continue;
    }
    for (int64_t i = B.sym0; i < B.sym0 + B.nsym; ++i) off = put_sym(B, sld[i], src[spos[i]], words.data(), nw, off);
    put_bits(words.data(), nw, off, B.lcode[256] & 0xFFFF, (int)(B.lcode[256] >> 16));
  }
  std::vector<uint32_t> adl((size_t)(2 * ((n + kAdler - 1) / kAdler)));
  for (int64_t c = 0; c * kAdler < n; ++c) adler_chunk_sums(src + c * kAdler, n - c * kAdler < kAdler ? n - c * kAdler : kAdler, &adl[2 * c]);
  put_frame(words.data(), nw, len, adler_fold(adl.data(), n, kAdler));
  for (int64_t i = 0; i < len; ++i) out[i] = (uint8_t)(words[(size_t)(i >> 2)] >> (8 * (i & 3)));
  *out_len = len;
  return RHCCQ_OK;
}

}  // extern "C"
