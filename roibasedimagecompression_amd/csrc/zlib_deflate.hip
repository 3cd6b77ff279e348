// zlib stream (RFC 1950 / 1951) encoder on the device: the outer and inner layers of a .rhccq container
// (encoder/compression/compression.py's zlib.compress(level=9)) without a device-to-host copy of the input or
// a single host core doing the work.  Format-compatible with zlib's inflate, not byte-identical to zlib's deflate.
//
// Pipeline of one rhccq_zlib_compress call (every launch on the context stream, all memory in the caller's workspace):
//   words_zero   clear the packing words (the output is assembled by OR-ing bits into 32-bit words); deflate_core.h
//   hash_chain_kernel<zl_hash>   one wave per 64 KiB hash chunk: prev[i] = distance to the nearest earlier position with
//                the same 3-byte hash (0: none within 32 KiB), one global function of the input; deflate_core.h
//   zl_match     one thread per position: walk the chain (at most kMaxChain candidates), longest match, nearest on
//                ties; lengths clamped to the position's 4 KiB parse chunk; 3-byte matches farther than 4 KiB dropped
//   zl_parse     one thread per parse chunk: lazy rule next(i) -- the match at i unless i+1 has a longer one
//   adler_partials_kernel<kParse>   one workgroup per parse chunk: (sum b, sum (L-k) b_k) of its bytes, folded in zl_scan;
//                deflate_core.h
//   zl_plan      one workgroup per 64 KiB block: symbol histograms, length-limited Huffman codes with the tie order
//                (frequency, symbol), run-length coded code lengths, cheapest of dynamic / fixed / stored
//   zl_bits      one workgroup per parse chunk: bits of its symbols under its block's code
//   zl_scan      one lane: bit offset of every block and parse chunk, Adler-32, zlib header, trailer, length
//   zl_emit      one workgroup per parse chunk: symbols at their bit offsets (exclusive scan), or raw bytes of a stored block
//   zl_header    one thread per block: block header, tree description, end-of-block code, stored LEN / NLEN
//   words_copy   packing words -> the caller's output buffer; deflate_core.h
// The output bytes are a function of the input bytes alone: no atomic whose order matters (only histogram adds,
// maxima and ORs of disjoint bits), no read of workspace memory this call did not write first.
#include "deflate_core.h"
#include "rhccq_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#define ZL_HD __host__ __device__ inline

namespace zl {

using namespace rhccq::deflate;            // the symbol algebra, Adler-32, kWindow, kHashBits, kHashChunk and the shared kernels
using rhccq::align256;

constexpr int kParse = 4096;               // parse chunk: matches never cross its end
constexpr int kChunksPerBlock = 16;
constexpr int kBlock = kParse * kChunksPerBlock;   // input bytes of one DEFLATE block (up to two stored pieces)
constexpr int kMaxChain = 128;             // candidates one position examines (the ratio / time knob)
constexpr int kNice = 258;
constexpr int kTooFar = 4096;              // a 3-byte match farther than this is worth less than 3 literals
constexpr int kStoredMax = 65535;
constexpr int kPlanTmp = 2560;             // int32 scratch of zl_plan_block

struct Block {
  int32_t type;       // 0 stored, 1 fixed, 2 dynamic (= BTYPE)
  int32_t hlit, hdist, hclen, ntok;
  int32_t pad;
  int64_t len;        // input bytes
  int64_t hdr_bits;   // dynamic: bits of the tree description after the 3-bit block header
  uint32_t lcode[288];  // bit-reversed code | length << 16
  uint32_t dcode[32];
  uint32_t ccode[19];
  uint16_t tok[320];  // code-length symbol | extra value << 5
};

ZL_HD void zl_or(uint32_t* w, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  atomicOr(w, v);
#else
  *w |= v;
#endif
}

// nb <= 32 bits of v at bit offset off (LSB-first, as DEFLATE packs them)
ZL_HD void zl_put(uint32_t* w, uint64_t off, uint32_t v, int nb) {
  if (nb <= 0) return;
  const uint64_t q = off >> 5;
  const int sh = (int)(off & 31);
  zl_or(w + q, v << sh);
  if (sh + nb > 32) zl_or(w + q + 1, v >> (32 - sh));
}

ZL_HD void zl_put_byte(uint32_t* w, uint64_t pos, uint32_t b) { zl_or(w + (pos >> 2), (b & 255u) << (8 * (pos & 3))); }

// symbols of the parse: literal byte b, or 0x80000000 | (len - 3) << 16 | (dist - 1)
ZL_HD int zl_sym_bits(uint32_t s, const uint32_t* lc, const uint32_t* dc) {
  if (!(s >> 31)) return (int)(lc[s & 255] >> 16);
  int le, lv, de, dv;
  const int ls = 257 + len_code((int)((s >> 16) & 255) + 3, le, lv);
  const int ds = dist_code((int)(s & 0xFFFF) + 1, de, dv);
  return (int)(lc[ls] >> 16) + le + (int)(dc[ds] >> 16) + de;
}

ZL_HD uint64_t zl_put_sym(uint32_t* w, uint64_t off, uint32_t s, const uint32_t* lc, const uint32_t* dc) {
  if (!(s >> 31)) {
    const uint32_t c = lc[s & 255];
    zl_put(w, off, c & 0xFFFF, (int)(c >> 16));
    return off + (c >> 16);
  }
  int le, lv, de, dv;
  const int ls = 257 + len_code((int)((s >> 16) & 255) + 3, le, lv);
  const int ds = dist_code((int)(s & 0xFFFF) + 1, de, dv);
  const uint32_t c = lc[ls], d = dc[ds];
  zl_put(w, off, c & 0xFFFF, (int)(c >> 16));
  off += c >> 16;
  zl_put(w, off, (uint32_t)lv, le);
  off += le;
  zl_put(w, off, d & 0xFFFF, (int)(d >> 16));
  off += d >> 16;
  zl_put(w, off, (uint32_t)dv, de);
  return off + de;
}

ZL_HD uint32_t zl_hash(const uint8_t* in, int64_t i) {
  const uint32_t v = (uint32_t)in[i] | (uint32_t)in[i + 1] << 8 | (uint32_t)in[i + 2] << 16;
  return (v * 2654435761u) >> (32 - kHashBits);
}

// longest match at i over the chain of prev[] (distances), at most `limit` bytes; returns len | (dist - 1) << 16, 0: none
ZL_HD uint32_t zl_longest(const uint8_t* in, const uint16_t* prev, int64_t i, int limit) {
  if (limit < 3) return 0;
  int best = 2, bdist = 0;
  int64_t cur = i;
  int64_t dist = 0;
  for (int c = 0; c < kMaxChain; ++c) {
    const int d = prev[cur];
    if (!d) break;
    cur -= d;
    dist = i - cur;
    if (dist > kWindow) break;
    const uint8_t* a = in + cur;
    const uint8_t* b = in + i;
    if (a[best] != b[best] || a[0] != b[0] || a[1] != b[1]) continue;
    int l = 2;
    while (l < limit && a[l] == b[l]) ++l;
    if (l > best) {
      best = l;
      bdist = (int)dist;
      if (l >= limit || l >= kNice) break;
    }
  }
  if (best < 3 || (best == 3 && bdist > kTooFar)) return 0;
  return (uint32_t)best | (uint32_t)(bdist - 1) << 16;
}

// lazy parse of [s, e): the match at i unless i+1 has a longer one; returns the number of symbols
ZL_HD int zl_parse_chunk(const uint32_t* m, const uint8_t* in, int64_t s, int64_t e, uint32_t* sym) {
  int k = 0;
  for (int64_t i = s; i < e;) {
    const uint32_t mi = m[i];
    int L = (int)(mi & 0xFFFF);
    if (L >= 3 && i + 1 < e && (int)(m[i + 1] & 0xFFFF) > L) L = 0;
    if (L >= 3) {
      sym[k++] = 0x80000000u | (uint32_t)(L - 3) << 16 | (mi >> 16);
      i += L;
    } else {
      sym[k++] = in[i];
      ++i;
    }
  }
  return k;
}

// canonical codes (RFC 1951 3.2.2) of lengths len[0..n), bit-reversed for LSB-first packing
ZL_HD void zl_canon(const uint8_t* len, int n, uint32_t* out) {
  int bl[16];
  uint32_t next[16];
  for (int b = 0; b < 16; ++b) bl[b] = 0;
  for (int s = 0; s < n; ++s) bl[len[s]]++;
  bl[0] = 0;
  uint32_t code = 0;
  next[0] = 0;
  for (int b = 1; b < 16; ++b) {
    code = (code + (uint32_t)bl[b - 1]) << 1;
    next[b] = code;
  }
  for (int s = 0; s < n; ++s) {
    const int L = len[s];
    out[s] = L ? (bit_reverse(next[L]++, L) | (uint32_t)L << 16) : 0u;
  }
}

// Huffman code lengths <= limit for the m >= 2 symbols order[0..m), sorted by (frequency, symbol); tmp: 6 m ints.
// Two-queue Huffman, then the overflow moved down the length counts until the code is complete again; lengths are
// handed out longest first in the sorted order (so the result is a function of the frequencies and the tie order).
ZL_HD void zl_huff_lengths(const uint32_t* freq, const int16_t* order, int m, int limit, uint8_t* len, int32_t* tmp) {
  uint32_t* w = (uint32_t*)tmp;
  int32_t* parent = tmp + 2 * m;
  int32_t* depth = tmp + 4 * m;
  for (int k = 0; k < m; ++k) w[k] = freq[order[k]];
  int li = 0, ii = m;
  for (int nn = m; nn < 2 * m - 1; ++nn) {
    int pick[2];
    for (int t = 0; t < 2; ++t) pick[t] = (li < m && (ii >= nn || w[li] <= w[ii])) ? li++ : ii++;
    w[nn] = w[pick[0]] + w[pick[1]];
    parent[pick[0]] = parent[pick[1]] = nn;
  }
  depth[2 * m - 2] = 0;
  for (int k = 2 * m - 3; k >= 0; --k) depth[k] = depth[parent[k]] + 1;
  int cnt[16];
  for (int d = 0; d < 16; ++d) cnt[d] = 0;
  for (int k = 0; k < m; ++k) cnt[depth[k] < limit ? depth[k] : limit]++;
  uint32_t total = 0;
  for (int d = 1; d <= limit; ++d) total += (uint32_t)cnt[d] << (limit - d);
  while (total > (1u << limit)) {
    cnt[limit]--;
    for (int d = limit - 1; d > 0; --d)
      if (cnt[d]) {
        cnt[d]--;
        cnt[d + 1] += 2;
        break;
      }
    total--;
  }
  int k = 0;
  for (int d = limit; d >= 1; --d)
    for (int c = 0; c < cnt[d]; ++c) len[order[k++]] = (uint8_t)d;
}

// order of the used symbols of freq[0..n) by (frequency, symbol) when fewer than two are used: zero-frequency
// symbols of the lowest numbers go in front (inflate wants every code complete, so every code gets two symbols)
ZL_HD int zl_pad_order(const uint32_t* freq, const int16_t* order, int m, int n, int16_t* out) {
  int k = 0;
  for (int s = 0; s < n && m + k < 2; ++s)
    if (!freq[s]) out[k++] = (int16_t)s;
  for (int j = 0; j < m; ++j) out[k + j] = order[j];
  return m + k;
}

// plan of one block from its histograms: fl[288] (EOB counted), fd[32]; ol / od: used symbols by (frequency, symbol)
ZL_HD void zl_plan_block(Block* B, const uint32_t* fl, const int16_t* ol, int ml, const uint32_t* fd, const int16_t* od, int md,
                         int64_t blen, int32_t* tmp) {
  int16_t* ordl = (int16_t*)tmp;                 // 290
  int16_t* ordd = ordl + 290;                    // 34
  int16_t* ordc = ordd + 34;                     // 20
  uint8_t* ll = (uint8_t*)(ordc + 20);           // 288 + 32 (contiguous: the code-length sequence runs across)
  uint8_t* dl = ll + 288;
  uint8_t* cl = dl + 32;                         // 19 (+1)
  uint32_t* fc = (uint32_t*)(tmp + 272);         // 19
  int32_t* htmp = tmp + 300;                     // 6 * 290
  for (int s = 0; s < 288 + 32 + 20; ++s) ll[s] = 0;
  const int nl = zl_pad_order(fl, ol, ml, 286, ordl);
  const int nd = zl_pad_order(fd, od, md, 30, ordd);
  zl_huff_lengths(fl, ordl, nl, 15, ll, htmp);
  zl_huff_lengths(fd, ordd, nd, 15, dl, htmp);
  int hlit = 286, hdist = 30;
  while (hlit > 257 && !ll[hlit - 1]) --hlit;
  while (hdist > 1 && !dl[hdist - 1]) --hdist;
  // code lengths of the lit/len and distance alphabets as one sequence (a repeat may run across), coded with 16 / 17 / 18
  for (int s = 0; s < 19; ++s) fc[s] = 0;
  int nt = 0;
  const int total = hlit + hdist;
  for (int i = 0; i < total;) {
    const uint8_t v = i < hlit ? ll[i] : dl[i - hlit];
    int run = 1;
    while (i + run < total && (i + run < hlit ? ll[i + run] : dl[i + run - hlit]) == v) ++run;
    i += run;
    if (!v) {
      while (run >= 11) {
        const int r = run < 138 ? run : 138;
        B->tok[nt++] = (uint16_t)(18 | (r - 11) << 5);
        fc[18]++;
        run -= r;
      }
      if (run >= 3) {
        B->tok[nt++] = (uint16_t)(17 | (run - 3) << 5);
        fc[17]++;
        run = 0;
      }
    } else {
      B->tok[nt++] = v;
      fc[v]++;
      --run;
      while (run >= 3) {
        const int r = run < 6 ? run : 6;
        B->tok[nt++] = (uint16_t)(16 | (r - 3) << 5);
        fc[16]++;
        run -= r;
      }
    }
    for (; run > 0; --run) {
      B->tok[nt++] = v;
      fc[v]++;
    }
  }
  // code-length code: 19 symbols, insertion sort by (frequency, symbol), lengths <= 7
  int16_t used[19];
  int mc = 0;
  for (int s = 0; s < 19; ++s)
    if (fc[s]) {
      int j = mc++;
      while (j > 0 && fc[used[j - 1]] > fc[s]) {
        used[j] = used[j - 1];
        --j;
      }
      used[j] = (int16_t)s;
    }
  const int ncl = zl_pad_order(fc, used, mc, 19, ordc);
  zl_huff_lengths(fc, ordc, ncl, 7, cl, htmp);
  int hclen = 19;
  while (hclen > 4 && !cl[codelen_order(hclen - 1)]) --hclen;
  zl_canon(cl, 19, B->ccode);
  // costs
  int64_t hdr = 14 + 3 * hclen;
  for (int t = 0; t < nt; ++t) {
    const int s = B->tok[t] & 31;
    hdr += cl[s] + codelen_extra(s);
  }
  int64_t dyn = 3 + hdr, fix = 3;
  for (int s = 0; s < 286; ++s)
    if (fl[s]) {
      const int e = s > 256 ? len_extra(s - 257) : 0;
      dyn += (int64_t)fl[s] * (ll[s] + e);
      fix += (int64_t)fl[s] * (fixed_litlen_bits(s) + e);
    }
  for (int s = 0; s < 30; ++s)
    if (fd[s]) {
      dyn += (int64_t)fd[s] * (dl[s] + dist_extra(s));
      fix += (int64_t)fd[s] * (5 + dist_extra(s));
    }
  const int64_t pieces = blen > 0 ? (blen + kStoredMax - 1) / kStoredMax : 1;
  const int64_t stored = pieces * 42 + 8 * blen;      // worst-case alignment: 3 + 7 + 32 per piece
  B->len = blen;
  B->hlit = hlit;
  B->hdist = hdist;
  B->hclen = hclen;
  B->ntok = nt;
  B->pad = 0;
  if (stored < dyn && stored < fix) {
    B->type = 0;
    B->hdr_bits = 0;
  } else if (fix <= dyn) {
    B->type = 1;
    B->hdr_bits = 0;
    for (int s = 0; s < 288; ++s) ll[s] = (uint8_t)fixed_litlen_bits(s);
    for (int s = 0; s < 32; ++s) dl[s] = 5;
  } else {
    B->type = 2;
    B->hdr_bits = hdr;                              // 14 + 3 hclen + tokens (the 3-bit block header is counted apart)
  }
  zl_canon(ll, 288, B->lcode);
  zl_canon(dl, 32, B->dcode);
}

// bit offsets of every block and parse chunk, the Adler-32 of the input, the zlib header and trailer; returns the length
ZL_HD int64_t zl_scan(const Block* blocks, int nb, const int64_t* chunk_bits, int nc, const uint32_t* adl, int64_t n,
                      int64_t* chunk_off, int64_t* block_off, uint32_t* words) {
  uint64_t off = 16;
  for (int b = 0; b < nb; ++b) {
    const Block& B = blocks[b];
    block_off[b] = (int64_t)off;
    const int c0 = b * kChunksPerBlock, c1 = (c0 + kChunksPerBlock < nc) ? c0 + kChunksPerBlock : nc;
    if (B.type == 0) {
      int64_t left = B.len;
      do {
        const int64_t l = left < kStoredMax ? left : kStoredMax;
        off = ((off + 3 + 7) & ~(uint64_t)7) + 32 + 8 * (uint64_t)l;
        left -= l;
      } while (left > 0);
      for (int c = c0; c < c1; ++c) chunk_off[c] = 0;
    } else {
      off += 3 + (uint64_t)B.hdr_bits;
      for (int c = c0; c < c1; ++c) {
        chunk_off[c] = (int64_t)off;
        off += (uint64_t)chunk_bits[c];
      }
      off += B.lcode[256] >> 16;
    }
  }
  const uint64_t end = (off + 7) >> 3;
  zl_put(words, 0, 0x9C78u, 16);                   // CMF 0x78 (deflate, 32 KiB window), FLG 0x9C: FCHECK makes 0x789C % 31 == 0
  const uint32_t adler = adler_fold(adl, n, kParse);
  for (int k = 0; k < 4; ++k) zl_put_byte(words, end + k, adler >> (24 - 8 * k));
  return (int64_t)end + 4;
}

// block header, tree description, end-of-block code (or the stored pieces' headers) of block b
ZL_HD void zl_block_header(const Block& B, int b, int nb, int nc, const int64_t* block_off, const int64_t* chunk_off,
                           const int64_t* chunk_bits, uint32_t* words) {
  const bool last = b == nb - 1;
  uint64_t off = (uint64_t)block_off[b];
  if (B.type == 0) {
    int64_t left = B.len;
    do {
      const int64_t l = left < kStoredMax ? left : kStoredMax;
      left -= l;
      zl_put(words, off, (last && left == 0) ? 1u : 0u, 3);
      off = (off + 3 + 7) & ~(uint64_t)7;
      zl_put(words, off, (uint32_t)l | (uint32_t)(~l & 0xFFFF) << 16, 32);
      off += 32 + 8 * (uint64_t)l;
    } while (left > 0);
    return;
  }
  zl_put(words, off, (last ? 1u : 0u) | (uint32_t)B.type << 1, 3);
  off += 3;
  if (B.type == 2) {
    zl_put(words, off, (uint32_t)(B.hlit - 257), 5);
    zl_put(words, off + 5, (uint32_t)(B.hdist - 1), 5);
    zl_put(words, off + 10, (uint32_t)(B.hclen - 4), 4);
    off += 14;
    for (int k = 0; k < B.hclen; ++k, off += 3) zl_put(words, off, B.ccode[codelen_order(k)] >> 16, 3);
    for (int t = 0; t < B.ntok; ++t) {
      const int s = B.tok[t] & 31, x = B.tok[t] >> 5;
      const uint32_t c = B.ccode[s];
      zl_put(words, off, c & 0xFFFF, (int)(c >> 16));
      off += c >> 16;
      const int eb = codelen_extra(s);
      zl_put(words, off, (uint32_t)x, eb);
      off += eb;
    }
  }
  const int cl = ((b + 1) * kChunksPerBlock < nc ? (b + 1) * kChunksPerBlock : nc) - 1;
  const uint32_t eob = B.lcode[256];
  zl_put(words, (uint64_t)(chunk_off[cl] + chunk_bits[cl]), eob & 0xFFFF, (int)(eob >> 16));
}

// ---- layout --------------------------------------------------------------------------------------------------------

struct Layout {
  int64_t nc, nb, nhc, bound, words;
  int64_t o_prev, o_m, o_sym, o_nsym, o_bits, o_coff, o_adl, o_blk, o_boff, o_words, total;
};

inline Layout layout(int64_t n) {
  Layout L;
  L.nc = n > 0 ? (n + kParse - 1) / kParse : 1;
  L.nb = (L.nc + kChunksPerBlock - 1) / kChunksPerBlock;
  L.nhc = (n + kHashChunk - 1) / kHashChunk;
  L.bound = n + 16 + 12 * L.nb;
  L.words = (L.bound + 3) / 4 + 2;
  int64_t o = 0;
  L.o_prev = o; o = align256(o + 2 * n);
  L.o_m = o; o = align256(o + 4 * n);
  L.o_sym = o; o = align256(o + 4 * L.nc * kParse);
  L.o_nsym = o; o = align256(o + 4 * L.nc);
  L.o_bits = o; o = align256(o + 8 * L.nc);
  L.o_coff = o; o = align256(o + 8 * L.nc);
  L.o_adl = o; o = align256(o + 8 * L.nc);
  L.o_blk = o; o = align256(o + (int64_t)sizeof(Block) * L.nb);
  L.o_boff = o; o = align256(o + 8 * L.nb);
  L.o_words = o; o = align256(o + 4 * L.words);
  L.total = o;
  return L;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void zl_match(const uint8_t* __restrict__ in, int64_t n, const uint16_t* __restrict__ prev,
                                                uint32_t* __restrict__ m) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t pe = (i / kParse + 1) * kParse;
  const int64_t lim = (pe < n ? pe : n) - i;
  m[i] = zl_longest(in, prev, i, lim < kNice ? (int)lim : kNice);
}

__global__ __launch_bounds__(64) void zl_parse(const uint32_t* __restrict__ m, const uint8_t* __restrict__ in, int64_t n, int nc,
                                               uint32_t* __restrict__ sym, int32_t* __restrict__ nsym) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= nc) return;
  const int64_t s = (int64_t)c * kParse;
  const int64_t e = s + kParse < n ? s + kParse : n;
  nsym[c] = s < e ? zl_parse_chunk(m, in, s, e, sym + s) : 0;
}

__global__ __launch_bounds__(256) void zl_plan(const uint32_t* __restrict__ sym, const int32_t* __restrict__ nsym, int64_t n, int nc,
                                               Block* __restrict__ blocks) {
  __shared__ uint32_t fl[288], fd[32];
  __shared__ int16_t ol[288], od[32];
  __shared__ int cnt[2];
  __shared__ int32_t tmp[kPlanTmp];
  const int b = blockIdx.x, t = threadIdx.x;
  for (int s = t; s < 288; s += 256) fl[s] = 0;
  if (t < 32) fd[t] = 0;
  if (t < 2) cnt[t] = 0;
  __syncthreads();
  const int c0 = b * kChunksPerBlock, c1 = c0 + kChunksPerBlock < nc ? c0 + kChunksPerBlock : nc;
  for (int c = c0; c < c1; ++c) {
    const uint32_t* sc = sym + (int64_t)c * kParse;
    const int ns = nsym[c];
    for (int k = t; k < ns; k += 256) {
      const uint32_t s = sc[k];
      if (!(s >> 31)) {
        atomicAdd(&fl[s & 255], 1u);
      } else {
        int le, lv, de, dv;
        atomicAdd(&fl[257 + len_code((int)((s >> 16) & 255) + 3, le, lv)], 1u);
        atomicAdd(&fd[dist_code((int)(s & 0xFFFF) + 1, de, dv)], 1u);
      }
    }
  }
  __syncthreads();
  if (t == 0) fl[256] += 1;                        // end of block
  __syncthreads();
  // rank of every used symbol in the order (frequency, symbol)
  for (int s = t; s < 288 + 32; s += 256) {
    const bool isl = s < 288;
    const uint32_t* f = isl ? fl : fd;
    const int ss = isl ? s : s - 288, ns = isl ? 288 : 32;
    const uint32_t v = f[ss];
    if (!v) continue;
    int r = 0;
    for (int u = 0; u < ns; ++u) r += (f[u] && (f[u] < v || (f[u] == v && u < ss))) ? 1 : 0;
    (isl ? ol : od)[r] = (int16_t)ss;
    atomicAdd(&cnt[isl ? 0 : 1], 1);
  }
  __syncthreads();
  if (t == 0) {
    const int64_t s = (int64_t)c0 * kParse;
    const int64_t e = (int64_t)c1 * kParse < n ? (int64_t)c1 * kParse : n;
    zl_plan_block(&blocks[b], fl, ol, cnt[0], fd, od, cnt[1], e > s ? e - s : 0, tmp);
  }
}

__global__ __launch_bounds__(256) void zl_bits(const uint32_t* __restrict__ sym, const int32_t* __restrict__ nsym, const Block* __restrict__ blocks,
                                               int64_t* __restrict__ chunk_bits) {
  __shared__ long long red[8];
  const int c = blockIdx.x;
  const Block& B = blocks[c / kChunksPerBlock];
  long long bits = 0;
  if (B.type != 0) {
    const uint32_t* sc = sym + (int64_t)c * kParse;
    const int ns = nsym[c];
    for (int k = threadIdx.x; k < ns; k += 256) bits += zl_sym_bits(sc[k], B.lcode, B.dcode);
  }
  bits = rhccq::block_sum(bits, red);
  if (threadIdx.x == 0) chunk_bits[c] = bits;
}

__global__ void zl_scan_k(const Block* __restrict__ blocks, int nb, const int64_t* __restrict__ chunk_bits, int nc, const uint32_t* __restrict__ adl,
                          int64_t n, int64_t* __restrict__ chunk_off, int64_t* __restrict__ block_off, uint32_t* __restrict__ words,
                          int64_t* __restrict__ out_len) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *out_len = zl_scan(blocks, nb, chunk_bits, nc, adl, n, chunk_off, block_off, words);
}

constexpr int kEmitPer = kParse / 256;             // symbols per thread of zl_emit

__global__ __launch_bounds__(256) void zl_emit(const uint32_t* __restrict__ sym, const int32_t* __restrict__ nsym, const Block* __restrict__ blocks,
                                               const int64_t* __restrict__ chunk_off, const int64_t* __restrict__ block_off,
                                               const uint8_t* __restrict__ in, int64_t n, uint32_t* __restrict__ words) {
  __shared__ long long red[8];
  const int c = blockIdx.x, b = c / kChunksPerBlock;
  const Block& B = blocks[b];
  const int64_t s = (int64_t)c * kParse;
  if (B.type == 0) {
    const int64_t e = s + kParse < n ? s + kParse : n;
    const uint64_t data0 = (((uint64_t)block_off[b] + 3 + 7) >> 3) + 4;
    for (int64_t p = s + threadIdx.x; p < e; p += 256) {
      const int64_t j = p - (int64_t)b * kBlock;
      zl_put_byte(words, data0 + (uint64_t)j + 5 * (uint64_t)(j / kStoredMax), in[p]);
    }
    return;
  }
  const uint32_t* sc = sym + s;
  const int ns = nsym[c];
  const int k0 = threadIdx.x * kEmitPer;
  const int k1 = k0 + kEmitPer < ns ? k0 + kEmitPer : ns;
  long long bits = 0;
  for (int k = k0; k < k1; ++k) bits += zl_sym_bits(sc[k], B.lcode, B.dcode);
  long long tot;
  uint64_t off = (uint64_t)chunk_off[c] + (uint64_t)rhccq::block_exscan(bits, red, &tot);
  for (int k = k0; k < k1; ++k) off = zl_put_sym(words, off, sc[k], B.lcode, B.dcode);
}

__global__ void zl_header(const Block* __restrict__ blocks, int nb, int nc, const int64_t* __restrict__ block_off,
                          const int64_t* __restrict__ chunk_off, const int64_t* __restrict__ chunk_bits, uint32_t* __restrict__ words) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < nb) zl_block_header(blocks[b], b, nb, nc, block_off, chunk_off, chunk_bits, words);
}

}  // namespace zl

extern "C" {

int rhccq_zlib_sizes(int64_t n, int64_t* workspace_bytes, int64_t* out_bound) {
  if (n < 0 || n > ((int64_t)1 << 40)) return RHCCQ_E_ARG;
  const zl::Layout L = zl::layout(n);
  if (workspace_bytes) *workspace_bytes = L.total;
  if (out_bound) *out_bound = L.bound;
  return RHCCQ_OK;
}

int rhccq_zlib_compress(rhccq_ctx* ctx, const void* in, int64_t n, void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  using namespace zl;
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || (n > 0 && !in) || !workspace || !out || !out_len) return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib_compress: bad argument");
  if (n >= ((int64_t)1 << 31) - kBlock) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib_compress: input of 2 GiB or more");
  const Layout L = layout(n);
  if (out_cap < L.bound) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib_compress: out_cap below the bound of rhccq_zlib_sizes");
  char* ws = (char*)workspace;
  const uint8_t* src = (const uint8_t*)in;
  uint16_t* prev = (uint16_t*)(ws + L.o_prev);
  uint32_t* m = (uint32_t*)(ws + L.o_m);
  uint32_t* sym = (uint32_t*)(ws + L.o_sym);
  int32_t* nsym = (int32_t*)(ws + L.o_nsym);
  int64_t* bits = (int64_t*)(ws + L.o_bits);
  int64_t* coff = (int64_t*)(ws + L.o_coff);
  uint32_t* adl = (uint32_t*)(ws + L.o_adl);
  Block* blk = (Block*)(ws + L.o_blk);
  int64_t* boff = (int64_t*)(ws + L.o_boff);
  uint32_t* words = (uint32_t*)(ws + L.o_words);
  hipStream_t st = ctx->stream;
  const int nc = (int)L.nc, nb = (int)L.nb;
  const int zgrid = (int)((L.words + 255) / 256 < 4096 ? (L.words + 255) / 256 : 4096);
  words_zero<0><<<zgrid, 256, 0, st>>>(words, L.words, nullptr);
  if (n > 0) {
    hash_chain_kernel<zl_hash><<<(int)L.nhc, 64, 0, st>>>(src, n, prev);
    zl_match<<<(int)((n + 255) / 256), 256, 0, st>>>(src, n, prev, m);
  }
  zl_parse<<<(nc + 63) / 64, 64, 0, st>>>(m, src, n, nc, sym, nsym);
  adler_partials_kernel<kParse><<<nc, 256, 0, st>>>(src, n, adl);
  zl_plan<<<nb, 256, 0, st>>>(sym, nsym, n, nc, blk);
  zl_bits<<<nc, 256, 0, st>>>(sym, nsym, blk, bits);
  zl_scan_k<<<1, 64, 0, st>>>(blk, nb, bits, nc, adl, n, coff, boff, words, out_len);
  zl_emit<<<nc, 256, 0, st>>>(sym, nsym, blk, coff, boff, src, n, words);
  zl_header<<<(nb + 63) / 64, 64, 0, st>>>(blk, nb, nc, boff, coff, bits, words);
  const int cgrid = (int)((L.bound + 255) / 256 < 8192 ? (L.bound + 255) / 256 : 8192);
  words_copy<<<cgrid, 256, 0, st>>>(words, L.bound, out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

}  // extern "C"
