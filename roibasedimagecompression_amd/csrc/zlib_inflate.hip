// zlib stream (RFC 1950 / 1951) decoder on the device: the read side of the .rhccq container layers.  Accepts what
// zlib.decompress accepts (stored, fixed and dynamic blocks, flushes, bytes after the Adler-32 trailer ignored, FDICT and
// CINFO > 7 rejected).  One documented deviation: a distance is checked against the start of the output and the 32 KiB
// limit only, not against a smaller window the header may declare.
//
// DEFLATE is serial inside a block and a block's start is only known once the block before it is decoded, so the
// stream is decoded speculatively from plausible block headers and the genuine chain is picked out afterwards.
// Pipeline of one rhccq_zlib_decompress call (every launch on the context stream, all memory in the caller's workspace):
//   zi_find     one workgroup per 8 KiB span of the input: the first bit offset in the span where a plausible stored or
//               dynamic block header begins (one lane per bit offset, the minimum wins).  Span 0's candidate is bit 16,
//               right after the zlib header: always genuine.
//   zi_spec     one wave per candidate: decode blocks from it, counting output bytes only, until the bit position lands
//               exactly on another candidate's start at a block boundary, or the final block ends, or an error stops it
//   zi_chain    one lane: zlib header, the chain of "landed on" links from candidate 0, output offsets (exclusive scan),
//               the capacity check -- the total is known here, before any output byte is written
//   zi_write    one wave per chained worker: the same decode again, writing 32-bit entries at final offsets through a
//               32 KiB ring in LDS.  An entry is a byte, or a marker (bit 31 | source position) for a byte copied from
//               before the worker's start, which only an earlier worker knows.
//   zi_resolve  pointer jumping over the markers: every round replaces a marker by what its source holds; a chain of
//               markers crosses at most one worker per hop, so ceil(log2(candidates)) + 1 rounds resolve all of them
//   zi_emit     entries -> output bytes, and (sum b, sum (L - k) b_k) per 64 KiB chunk (the sums of deflate_core.h's
//               adler_chunk_sums, accumulated in the pass that writes the bytes)
//   zi_final    one lane: Adler-32 of the chunks (deflate_core.h's adler_fold) against the trailer
// The symbol bases and extra bits, the code-length order, the bit reversal, the Adler-32 modulus and fold are deflate_core.h's,
// shared with the encoders whose mapping they invert.  Only the fixed code's lengths are written out in zi_worker (see there).
// The parsing, table construction, block decoding, candidate test and chain walk are __host__ __device__ functions;
// rhccq_zlib_decompress_host runs the same functions serially on the CPU (a test vehicle, never a fallback).
// Malformed input never faults: every input read is bounds-checked against n (bits past the end read as zero and end
// the decode as TRUNCATED), every write against out_cap and the workspace, every table index against its table, every
// loop has a bound, and errors travel through the status word.
#include "deflate_core.h"
#include "rhccq_common.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#define ZI_HD __host__ __device__ inline
// called once per block: kept out of line, which keeps the workers' register allocation small (inlined, it reached
// 256 VGPRs and the backend rejected zi_write)
#define ZI_HD_NOINLINE __host__ __device__ __attribute__((noinline))

#ifdef __HIP_DEVICE_COMPILE__
// a worker is one wave: LDS operations of a wave complete in issue order, so a wave-scope fence (a compiler barrier)
// is all that orders one lane's LDS store before another lane's load
#define ZI_WSYNC()                                          \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
  } while (0)
#else
#define ZI_WSYNC() \
  do {             \
  } while (0)
#endif

namespace zi {

using namespace rhccq::deflate;            // the symbol algebra and Adler-32
using rhccq::align256;

constexpr int64_t kSpan = 8192;            // input bytes per candidate search span (the parallelism knob)
constexpr int64_t kSpanBits = kSpan * 8;
constexpr int kRing = 32768;               // RFC 1951 window = the LDS ring of zi_write
constexpr int kWin = 4096;                 // input bytes a worker stages in LDS
constexpr int kFast = 10;                  // bits of the direct Huffman lookup
constexpr int64_t kAdlChunk = 65536;
constexpr uint32_t kMark = 0x80000000u;

// worker states besides the public RHCCQ_ZS_* errors
constexpr int32_t kNone = -1;              // no candidate in this span
constexpr int32_t kLand = 16;              // landed on another candidate's start
constexpr int32_t kFinal = 17;             // decoded through the final block

struct Rec {
  int64_t end;     // bit position where the worker stopped
  int64_t nout;    // output bytes
  int64_t reach;   // min over matches of (local position - distance): < 0 reaches before the worker's start
  int32_t land;    // candidate index landed on (kLand)
  int32_t status;
  int32_t blocks;
  int32_t pad;
};

struct Ctl {
  int64_t total;   // decoded bytes of the chain
  int64_t tpos;    // byte offset of the Adler-32 trailer
  int32_t nchain, go, status, pad;
  int64_t stats[4];  // candidates, candidates whose decode failed, chained workers, blocks on the chain
};

struct Tab {
  uint16_t fast[1 << kFast];  // symbol << 4 | length for codes of <= kFast bits; 0: longer code or none
  int16_t cnt[16];
  int16_t sym[288];           // symbols sorted by (length, symbol)
  int16_t offs[17], base[16];
  int32_t next[16];
};

struct Lds {
  Tab lt, dt;
  uint8_t lens[320];
  uint8_t win[kWin];
};

// ---- bit reader ---------------------------------------------------------------------------------------------
// LSB-first over in[0..n); bytes past the end read as zero and pos() > nbits tells.  With win != nullptr the bytes
// come from an LDS window of kWin bytes the wave restages cooperatively (all lanes hold the same reader state).
struct BR {
  const uint8_t* in;
  int64_t n;
  int64_t bp;     // next byte to load into buf
  uint64_t buf;
  int cnt;
  uint8_t* win;
  int64_t wbase;
  ZI_HD int64_t pos() const { return bp * 8 - cnt; }
  ZI_HD bool over() const { return pos() > n * 8; }
};

ZI_HD void br_seek_byte(BR& r, int64_t byte) {
  r.bp = byte;
  r.buf = 0;
  r.cnt = 0;
}

ZI_HD void br_init(BR& r, const uint8_t* in, int64_t n, int64_t bit, uint8_t* win) {
  r.in = in;
  r.n = n;
  r.win = win;
  r.wbase = -2 * (int64_t)kWin;
  br_seek_byte(r, bit >> 3);
}

ZI_HD void br_refill(BR& r, int lane, int nl) {
  if (r.win && r.bp < r.n && (r.bp < r.wbase || r.bp + 8 > r.wbase + kWin)) {
    ZI_WSYNC();
    r.wbase = r.bp;
    for (int i = lane; i < kWin; i += nl) r.win[i] = r.wbase + i < r.n ? r.in[r.wbase + i] : 0;
    ZI_WSYNC();
  }
  for (int k = 0; k < 8 && r.cnt <= 56; ++k) {
    uint64_t b = 0;
    if (r.bp >= 0 && r.bp < r.n) b = r.win ? r.win[r.bp - r.wbase] : r.in[r.bp];
    r.buf |= b << r.cnt;
    r.cnt += 8;
    r.bp++;
  }
}

ZI_HD uint32_t br_get(BR& r, int nb, int lane, int nl) {
  if (nb <= 0) return 0;
  if (r.cnt < nb) br_refill(r, lane, nl);
  const uint32_t v = (uint32_t)(r.buf & ((1ull << nb) - 1));
  r.buf >>= nb;
  r.cnt -= nb;
  return v;
}

ZI_HD void br_skip_to(BR& r, int64_t bit, int lane, int nl) {
  // position a fresh reader at an arbitrary bit offset
  br_refill(r, lane, nl);
  br_get(r, (int)(bit & 7), lane, nl);
}

ZI_HD void br_align(BR& r) {
  const int d = r.cnt & 7;
  r.buf >>= d;
  r.cnt -= d;
}

// ---- code lengths and tables ---------------------------------------------------------------------------------
// zlib's inflate_table rule: an over-subscribed code is an error; an incomplete one is an error for the code length
// code, and for a literal / distance code unless its only length is 1 (a single code); a distance code with no codes
// at all is accepted (any distance then is invalid)
enum { kCodes = 0, kLens = 1, kDists = 2 };

// kraft = sum of 2^(15 - L) over the codes (over-subscribed at some length <=> over-subscribed at 15), mx = longest length;
// kept in registers (per-length count arrays indexed at run time live in scratch memory)
ZI_HD bool zi_code_ok(int kraft, int mx, int kind) {
  if (kraft > (1 << 15)) return false;
  if (mx == 0) return kind == kDists;
  if (kraft < (1 << 15) && (kind == kCodes || mx != 1)) return false;
  return true;
}

// cooperative table build from len[0..n) (n <= 288), read by every lane after the call
ZI_HD_NOINLINE void zi_build(Tab* t, const uint8_t* len, int n, int lane, int nl) {
  ZI_WSYNC();
  if (lane == 0) {
    int16_t* offs = t->offs;
    for (int b = 0; b < 16; ++b) t->cnt[b] = 0;
    for (int s = 0; s < n; ++s) t->cnt[len[s] & 15]++;
    t->cnt[0] = 0;
    offs[1] = 0;
    for (int b = 1; b < 16; ++b) offs[b + 1] = (int16_t)(offs[b] + t->cnt[b]);
    for (int s = 0; s < n; ++s) {
      const int L = len[s] & 15;
      if (L && offs[L] < 288) t->sym[offs[L]++] = (int16_t)s;
    }
    int code = 0, m = 0;
    t->next[0] = 0;
    t->base[0] = 0;
    for (int L = 1; L < 16; ++L) {
      code = (code + (L > 1 ? t->cnt[L - 1] : 0)) << 1;
      t->next[L] = code;
      t->base[L] = (int16_t)m;
      m += t->cnt[L];
    }
    t->offs[0] = (int16_t)(m > 288 ? 288 : m);
  }
  for (int i = lane; i < (1 << kFast); i += nl) t->fast[i] = 0;
  ZI_WSYNC();
  const int m = t->offs[0];
  for (int k = lane; k < m; k += nl) {
    const int s = t->sym[k];
    const int L = (s >= 0 && s < n) ? (len[s] & 15) : 0;
    if (L < 1 || L > kFast) continue;
    const uint32_t c = (uint32_t)(t->next[L] + (k - t->base[L]));
    if (c >= (1u << L)) continue;                    // only an invalid (over-subscribed) code gets here; never built
    for (uint32_t x = bit_reverse(c, L); x < (1u << kFast); x += 1u << L) t->fast[x] = (uint16_t)(s << 4 | L);
  }
  ZI_WSYNC();
}

// next symbol under t, or -1 for a bit pattern that is no code
ZI_HD int zi_decode(BR& r, const Tab* t, int lane, int nl) {
  if (r.cnt < 15) br_refill(r, lane, nl);
  const uint32_t bits = (uint32_t)(r.buf & 0x7FFF);
  const uint16_t e = t->fast[bits & ((1u << kFast) - 1)];
  if (e) {
    r.buf >>= (e & 15);
    r.cnt -= (e & 15);
    return e >> 4;
  }
  int code = 0, first = 0, index = 0;
  for (int L = 1; L <= 15; ++L) {
    code |= (int)((bits >> (L - 1)) & 1);
    const int count = t->cnt[L];
    if (code - count < first) {
      const int k = index + (code - first);
      if (k < 0 || k >= 288) return -1;
      r.buf >>= L;
      r.cnt -= L;
      return t->sym[k];
    }
    index += count;
    first += count;
    first <<= 1;
    code <<= 1;
  }
  return -1;
}

ZI_HD int zi_bad_or_short(const BR& r) { return r.n * 8 - r.pos() < 15 ? RHCCQ_ZS_TRUNCATED : RHCCQ_ZS_BAD_DATA; }

// dynamic block tree description after the 3-bit block header: lens[0..nlen + ndist) (written by lane 0), validated
// as zlib validates it.  Returns RHCCQ_ZS_OK, BAD_DATA or TRUNCATED.  The reader is copied in and out so that the
// caller's stays in registers; every array here is indexed by unrolled constants for the same reason.
ZI_HD_NOINLINE int zi_dynamic(BR* rp, uint8_t* lens, int* nlen_out, int* ndist_out, int lane, int nl) {
  BR r = *rp;
  int st = RHCCQ_ZS_OK;
  const int nlen = (int)br_get(r, 5, lane, nl) + 257;
  const int ndist = (int)br_get(r, 5, lane, nl) + 1;
  const int ncode = (int)br_get(r, 4, lane, nl) + 4;
  *nlen_out = nlen;
  *ndist_out = ndist;
  uint32_t cl[19], rc[19];
#pragma unroll
  for (int k = 0; k < 19; ++k) cl[k] = 0;
  if (r.over()) {
    st = RHCCQ_ZS_TRUNCATED;
  } else if (nlen > 286 || ndist > 30) {
    st = RHCCQ_ZS_BAD_DATA;
  } else {
    uint32_t got[19];
#pragma unroll
    for (int k = 0; k < 19; ++k) got[k] = k < ncode ? br_get(r, 3, lane, nl) : 0u;
#pragma unroll
    for (int k = 0; k < 19; ++k) cl[codelen_order(k)] = got[k];
    if (r.over()) st = RHCCQ_ZS_TRUNCATED;
  }
  if (st == RHCCQ_ZS_OK) {
    int kraft = 0, mx = 0;
#pragma unroll
    for (int k = 0; k < 19; ++k) {
      kraft += cl[k] ? 1 << (15 - cl[k]) : 0;
      mx = (int)cl[k] > mx ? (int)cl[k] : mx;
    }
    if (!zi_code_ok(kraft, mx, kCodes)) st = RHCCQ_ZS_BAD_DATA;
  }
  if (st == RHCCQ_ZS_OK) {
    // canonical code of every code length symbol, bit-reversed: first code of its length + its rank among equal lengths
    uint32_t first[8];
    uint32_t code = 0;
    first[0] = 0;
#pragma unroll
    for (int L = 1; L < 8; ++L) {
      uint32_t c = 0;
#pragma unroll
      for (int k = 0; k < 19; ++k) c += cl[k] == (uint32_t)(L - 1) && L > 1 ? 1u : 0u;
      code = (code + c) << 1;
      first[L] = code;
    }
#pragma unroll
    for (int k = 0; k < 19; ++k) {
      uint32_t rank = 0, f = 0;
#pragma unroll
      for (int q = 0; q < k; ++q) rank += cl[q] == cl[k] ? 1u : 0u;
#pragma unroll
      for (int L = 1; L < 8; ++L) f = cl[k] == (uint32_t)L ? first[L] : f;
      rc[k] = cl[k] ? bit_reverse(f + rank, (int)cl[k]) : 0xFFFFu;
    }
    int lk = 0, lm = 0, dk = 0, dm = 0;
    const int total = nlen + ndist;
    int i = 0, prev = 0;
    bool eob = false;
    for (int guard = 0; i < total && guard < 320; ++guard) {
      if (r.cnt < 7) br_refill(r, lane, nl);
      const uint32_t b = (uint32_t)(r.buf & 127);
      int sym = -1, sl = 0;
#pragma unroll
      for (int k = 0; k < 19; ++k)
        if (cl[k] && (b & ((1u << cl[k]) - 1)) == rc[k]) {
          sym = k;
          sl = (int)cl[k];
        }
      r.buf >>= sl;
      r.cnt -= sl;
      if (r.over()) { st = RHCCQ_ZS_TRUNCATED; break; }
      if (sym < 0) { st = RHCCQ_ZS_BAD_DATA; break; }        // complete code: cannot happen
      int rep = 1, val = sym;
      if (sym == 16) {
        rep = 3 + (int)br_get(r, 2, lane, nl);
        if (r.over()) { st = RHCCQ_ZS_TRUNCATED; break; }
        if (i == 0) { st = RHCCQ_ZS_BAD_DATA; break; }
        val = prev;
      } else if (sym == 17) {
        rep = 3 + (int)br_get(r, 3, lane, nl);
        val = 0;
      } else if (sym == 18) {
        rep = 11 + (int)br_get(r, 7, lane, nl);
        val = 0;
      }
      if (r.over()) { st = RHCCQ_ZS_TRUNCATED; break; }
      if (i + rep > total) { st = RHCCQ_ZS_BAD_DATA; break; }
      if (lane == 0 && lens)
        for (int k = 0; k < rep; ++k) lens[i + k] = (uint8_t)val;
      // this run's share of the literal/length and distance codes
      const int nl_part = i < nlen ? (i + rep <= nlen ? rep : nlen - i) : 0;
      const int nd_part = rep - nl_part;
      if (val) {
        lk += nl_part << (15 - val);
        dk += nd_part << (15 - val);
        if (nl_part) lm = val > lm ? val : lm;
        if (nd_part) dm = val > dm ? val : dm;
      }
      if (val && i <= 256 && 256 < i + nl_part) eob = true;
      if (lk > (1 << 16)) lk = (1 << 16);      // over-subscribed already: clamp so the sums cannot overflow
      if (dk > (1 << 16)) dk = (1 << 16);
      i += rep;
      prev = val;
    }
    if (st == RHCCQ_ZS_OK) {
      if (i < total || !eob) st = RHCCQ_ZS_BAD_DATA;
      else if (!zi_code_ok(lk, lm, kLens) || !zi_code_ok(dk, dm, kDists)) st = RHCCQ_ZS_BAD_DATA;
    }
  }
  *rp = r;
  return st;
}

// is there a plausible non-final stored or dynamic block header at `bit`?  (one lane, reading global memory)
ZI_HD bool zi_plausible(const uint8_t* in, int64_t n, int64_t bit) {
  BR r;
  br_init(r, in, n, bit, nullptr);
  br_skip_to(r, bit, 0, 1);
  const uint32_t h = br_get(r, 3, 0, 1);
  if (r.over() || (h & 1)) return false;
  if ((h >> 1) == 0) {
    br_align(r);
    const uint32_t len = br_get(r, 16, 0, 1), nlen = br_get(r, 16, 0, 1);
    return !r.over() && len == (~nlen & 0xFFFFu);
  }
  if ((h >> 1) != 2) return false;
  int nlen, ndist;
  BR t = r;
  return zi_dynamic(&t, nullptr, &nlen, &ndist, 0, 1) == RHCCQ_ZS_OK;
}

// candidate index of a block boundary at bit p, or -1
ZI_HD int zi_cand_at(const int64_t* cand, int64_t ns, int64_t p) {
  if (p < 0) return -1;
  const int64_t sp = p / kSpanBits;
  return (sp < ns && cand[sp] == p) ? (int)sp : -1;
}

// ---- one worker --------------------------------------------------------------------------------------------
// Decode blocks from bit `start` until a block boundary lands on another candidate, the final block ends or an error
// stops it.  WRITE = false: count only (rec receives the result).  WRITE = true: entries for local positions [0, lim)
// go to tok[off + j] (j < lim, off + j < cap) through the ring (kRing entries).
template <bool WRITE>
ZI_HD void zi_worker(const uint8_t* in, int64_t n, int64_t start, const int64_t* cand, int64_t ns, Lds* L, uint32_t* ring, uint32_t* tok,
                     int64_t off, int64_t lim, int64_t cap, Rec* rec, int lane, int nl) {
  BR r;
  br_init(r, in, n, start, L->win);
  br_skip_to(r, start, lane, nl);
  int64_t j = 0, reach = 0;
  int32_t status = RHCCQ_ZS_TRUNCATED, land = -1, blocks = 0;
  bool fixed = false;
  const int64_t nbits = n * 8;
  for (int64_t blk = 0; blk <= nbits / 3 + 1; ++blk) {
    const int64_t p = r.pos();
    if (blk > 0) {
      const int c = zi_cand_at(cand, ns, p);
      if (c >= 0) {
        status = kLand;
        land = c;
        break;
      }
    }
    const uint32_t h = br_get(r, 3, lane, nl);
    if (r.over()) {
      status = RHCCQ_ZS_TRUNCATED;
      break;
    }
    blocks++;
    const int bt = (int)(h >> 1);
    int err = RHCCQ_ZS_OK;
    if (bt == 0) {
      br_align(r);
      const uint32_t len = br_get(r, 16, lane, nl), nlen = br_get(r, 16, lane, nl);
      if (r.over()) {
        status = RHCCQ_ZS_TRUNCATED;
        break;
      }
      if (len != (~nlen & 0xFFFFu)) {
        status = RHCCQ_ZS_BAD_DATA;
        break;
      }
      const int64_t bp = r.pos() >> 3;
      if (bp + (int64_t)len > n) {
        status = RHCCQ_ZS_TRUNCATED;
        break;
      }
      if (WRITE) {
        ZI_WSYNC();
        for (int64_t k = lane; k < (int64_t)len; k += nl) {
          const uint32_t v = in[bp + k];
          const int64_t q = j + k;
          ring[q & (kRing - 1)] = v;
          if (q < lim && off + q < cap) tok[off + q] = v;
        }
        ZI_WSYNC();
      }
      j += len;
      br_seek_byte(r, bp + len);
    } else if (bt == 3) {
      status = RHCCQ_ZS_BAD_DATA;
      break;
    } else {
      if (bt == 1) {
        if (!fixed) {
          ZI_WSYNC();
          // deflate_core.h's fixed_litlen_bits(s) for s < 288, then distance codes of 5 bits.  Written out on purpose: as
          // s < 288 ? fixed_litlen_bits(s) : 5 the compiler gives zi_write 185 VGPRs for 180 and 14 more SGPR spills (zi_spec: 14 too)
          for (int s = lane; s < 318; s += nl) L->lens[s] = s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5;
          zi_build(&L->lt, L->lens, 288, lane, nl);
          zi_build(&L->dt, L->lens + 288, 30, lane, nl);
          fixed = true;
        }
      } else {
        int nlen = 0, ndist = 0;
        ZI_WSYNC();
        BR t = r;                                       // r itself never has its address taken
        err = zi_dynamic(&t, L->lens, &nlen, &ndist, lane, nl);
        r = t;
        if (err) {
          status = err;
          break;
        }
        fixed = false;
        zi_build(&L->lt, L->lens, nlen, lane, nl);
        zi_build(&L->dt, L->lens + nlen, ndist, lane, nl);
      }
      // symbols: every symbol consumes at least one bit, so nbits + 1 iterations bound the loop
      bool eob = false;
      for (int64_t it = 0; it <= nbits + 1; ++it) {
        const int s = zi_decode(r, &L->lt, lane, nl);
        if (s < 0) {
          err = zi_bad_or_short(r);
          break;
        }
        if (r.over()) {
          err = RHCCQ_ZS_TRUNCATED;
          break;
        }
        if (s < 256) {
          if (WRITE && lane == 0) {
            ring[j & (kRing - 1)] = (uint32_t)s;
            if (j < lim && off + j < cap) tok[off + j] = (uint32_t)s;
          }
          ++j;
          continue;
        }
        if (s == 256) {
          eob = true;
          break;
        }
        if (s > 285) {
          err = RHCCQ_ZS_BAD_DATA;
          break;
        }
        const int len = len_base(s - 257) + (int)br_get(r, len_extra(s - 257), lane, nl);
        const int ds = zi_decode(r, &L->dt, lane, nl);
        if (ds < 0) {
          err = zi_bad_or_short(r);
          break;
        }
        if (ds > 29) {
          err = RHCCQ_ZS_BAD_DATA;
          break;
        }
        const int dist = dist_base(ds) + (int)br_get(r, dist_extra(ds), lane, nl);
        if (r.over()) {
          err = RHCCQ_ZS_TRUNCATED;
          break;
        }
        if (j - dist < reach) reach = j - dist;
        if (WRITE) {
          ZI_WSYNC();
          for (int k = lane; k < len; k += nl) {
            const int64_t q = j - dist + (k % dist);
            uint32_t e;
            if (q >= 0) e = ring[q & (kRing - 1)];
            else e = off + q >= 0 ? (kMark | (uint32_t)(off + q)) : 0u;   // off + q < 0 never survives the chain walk
            const int64_t d = j + k;
            ring[d & (kRing - 1)] = e;
            if (d < lim && off + d < cap) tok[off + d] = e;
          }
          ZI_WSYNC();
        }
        j += len;
      }
      if (!eob) {
        status = err ? err : RHCCQ_ZS_TRUNCATED;
        break;
      }
    }
    if (h & 1) {
      status = kFinal;
      break;
    }
  }
  if (!WRITE && lane == 0) {
    rec->end = r.pos();
    rec->nout = j;
    rec->reach = reach;
    rec->land = land;
    rec->status = status;
    rec->blocks = blocks;
    rec->pad = 0;
  }
}

// ---- chain walk (one lane) -------------------------------------------------------------------------------------
ZI_HD void zi_chain(const uint8_t* in, int64_t n, const int64_t* cand, const Rec* rec, int64_t ns, int64_t out_cap, int32_t* chain,
                    int64_t* choff, Ctl* ctl, int64_t* out_len, int32_t* status) {
  int32_t st = RHCCQ_ZS_OK;
  int64_t off = 0, tpos = 0, blocks = 0;
  int32_t k = 0;
  if (n < 2) {
    st = RHCCQ_ZS_TRUNCATED;
  } else {
    const uint32_t cmf = in[0], flg = in[1];
    if ((cmf * 256 + flg) % 31 || (cmf & 15) != 8 || (cmf >> 4) > 7 || (flg & 0x20)) st = RHCCQ_ZS_BAD_HEADER;
  }
  if (st == RHCCQ_ZS_OK) {
    st = RHCCQ_ZS_BAD_DATA;
    int64_t c = 0;
    for (int64_t it = 0; it < ns; ++it) {
      const Rec R = rec[c];
      if (R.status == kNone) break;
      if (off + R.reach < 0) break;                       // a distance before the start of the output
      chain[k] = (int32_t)c;
      choff[k] = off;
      ++k;
      off += R.nout;
      blocks += R.blocks;
      if (R.status == kFinal) {
        tpos = (R.end + 7) >> 3;
        st = tpos + 4 > n ? RHCCQ_ZS_TRUNCATED : RHCCQ_ZS_OK;
        break;
      }
      if (R.status == kLand && R.land > c && R.land < ns) {
        c = R.land;
        continue;
      }
      st = R.status == kLand ? RHCCQ_ZS_BAD_DATA : R.status;
      break;
    }
  }
  int64_t nc = 0, nf = 0;
  for (int64_t c = 0; c < ns; ++c) {
    if (rec[c].status == kNone) continue;
    ++nc;
    if (rec[c].status != kLand && rec[c].status != kFinal) ++nf;
  }
  int32_t go = 0;
  if (st == RHCCQ_ZS_OK && off > out_cap) st = RHCCQ_ZS_CAPACITY;
  else if (st == RHCCQ_ZS_OK) go = 1;
  ctl->total = off;
  ctl->tpos = tpos;
  ctl->nchain = go ? k : 0;
  ctl->go = go;
  ctl->status = st;
  ctl->pad = 0;
  ctl->stats[0] = nc;
  ctl->stats[1] = nf;
  ctl->stats[2] = k;
  ctl->stats[3] = blocks;
  *out_len = st == RHCCQ_ZS_CAPACITY ? off : 0;
  *status = st;
}

ZI_HD void zi_finish(const uint8_t* in, int64_t n, const Ctl* ctl, const uint32_t* part, int64_t* out_len, int32_t* status) {
  if (!ctl->go) return;
  const int64_t t = ctl->tpos;
  if (t < 0 || t + 4 > n) {
    *status = RHCCQ_ZS_TRUNCATED;
    return;
  }
  const uint32_t want = (uint32_t)in[t] << 24 | (uint32_t)in[t + 1] << 16 | (uint32_t)in[t + 2] << 8 | (uint32_t)in[t + 3];
  if (adler_fold(part, ctl->total, kAdlChunk) != want) {
    *status = RHCCQ_ZS_ADLER;
    *out_len = 0;
    return;
  }
  *status = RHCCQ_ZS_OK;
  *out_len = ctl->total;
}

struct Layout {
  int64_t ns, nadl, rounds;
  int64_t o_cand, o_rec, o_chain, o_choff, o_ctl, o_adl, o_tok, total;
};

inline Layout layout(int64_t n, int64_t out_cap) {
  Layout L;
  L.ns = n > 0 ? (n + kSpan - 1) / kSpan : 1;
  L.nadl = out_cap > 0 ? (out_cap + kAdlChunk - 1) / kAdlChunk : 1;
  L.rounds = 1;
  for (int64_t v = 1; v < L.ns; v <<= 1) L.rounds++;
  int64_t o = 0;
  L.o_cand = o;
  o = align256(o + 8 * L.ns);
  L.o_rec = o;
  o = align256(o + (int64_t)sizeof(Rec) * L.ns);
  L.o_chain = o;
  o = align256(o + 4 * L.ns);
  L.o_choff = o;
  o = align256(o + 8 * L.ns);
  L.o_ctl = o;
  o = align256(o + (int64_t)sizeof(Ctl));
  L.o_adl = o;
  o = align256(o + 8 * L.nadl);
  L.o_tok = o;
  o = align256(o + 4 * (out_cap > 0 ? out_cap : 1));
  L.total = o;
  return L;
}

// ---- kernels --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void zi_find(const uint8_t* __restrict__ in, int64_t n, int64_t ns, int64_t* __restrict__ cand) {
  __shared__ unsigned long long best;
  const int64_t b = blockIdx.x;
  if (b >= ns) return;
  if (b == 0) {
    if (threadIdx.x == 0) cand[0] = 16;
    return;
  }
  constexpr unsigned long long kNo = ~0ull;
  if (threadIdx.x == 0) best = kNo;
  __syncthreads();
  const int64_t base = b * kSpanBits, nbits = n * 8;
  for (int64_t c = 0; c < kSpanBits; c += 256) {
    const int64_t bit = base + c + threadIdx.x;
    if (bit + 3 <= nbits && zi_plausible(in, n, bit)) atomicMin(&best, (unsigned long long)bit);
    __syncthreads();
    const unsigned long long f = best;
    __syncthreads();
    if (f != kNo) break;
  }
  if (threadIdx.x == 0) cand[b] = best == kNo ? -1 : (int64_t)best;
}

__global__ __launch_bounds__(64) void zi_spec(const uint8_t* __restrict__ in, int64_t n, const int64_t* __restrict__ cand, int64_t ns,
                                              Rec* __restrict__ rec) {
  __shared__ Lds L;
  const int64_t b = blockIdx.x;
  if (b >= ns) return;
  const int64_t start = cand[b];
  if (start < 0) {
    if (threadIdx.x == 0) {
      rec[b].end = -1;
      rec[b].nout = 0;
      rec[b].reach = 0;
      rec[b].land = -1;
      rec[b].status = kNone;
      rec[b].blocks = 0;
      rec[b].pad = 0;
    }
    return;
  }
  zi_worker<false>(in, n, start, cand, ns, &L, nullptr, nullptr, 0, 0, 0, &rec[b], threadIdx.x, 64);
}

__global__ void zi_chain_k(const uint8_t* __restrict__ in, int64_t n, const int64_t* __restrict__ cand, const Rec* __restrict__ rec, int64_t ns,
                           int64_t out_cap, int32_t* __restrict__ chain, int64_t* __restrict__ choff, Ctl* __restrict__ ctl,
                           int64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  if (threadIdx.x == 0 && blockIdx.x == 0) zi_chain(in, n, cand, rec, ns, out_cap, chain, choff, ctl, out_len, status);
}

__global__ __launch_bounds__(64) void zi_write(const uint8_t* __restrict__ in, int64_t n, const int64_t* __restrict__ cand, int64_t ns,
                                               const Rec* __restrict__ rec, const int32_t* __restrict__ chain, const int64_t* __restrict__ choff,
                                               const Ctl* __restrict__ ctl, uint32_t* __restrict__ tok, int64_t cap) {
  __shared__ Lds L;
  __shared__ uint32_t ring[kRing];
  const int b = blockIdx.x;
  if (!ctl->go || b >= ctl->nchain) return;
  const int c = chain[b];
  if (c < 0 || c >= ns) return;
  zi_worker<true>(in, n, cand[c], cand, ns, &L, ring, tok, choff[b], rec[c].nout, cap, nullptr, threadIdx.x, 64);
}

__global__ __launch_bounds__(256) void zi_resolve(const Ctl* __restrict__ ctl, uint32_t* tok) {
  if (!ctl->go) return;
  const int64_t total = ctl->total;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (int64_t)gridDim.x * blockDim.x) {
    const uint32_t e = __hip_atomic_load(&tok[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!(e & kMark)) continue;
    const int64_t s = e & ~kMark;
    const uint32_t v = s < p ? __hip_atomic_load(&tok[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    __hip_atomic_store(&tok[p], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void zi_emit(const Ctl* __restrict__ ctl, const uint32_t* __restrict__ tok, uint8_t* __restrict__ out,
                                               uint32_t* __restrict__ part) {
  __shared__ unsigned long long red[8];
  if (!ctl->go) return;
  const int64_t total = ctl->total, nch = (total + kAdlChunk - 1) / kAdlChunk;
  for (int64_t c = blockIdx.x; c < nch; c += gridDim.x) {
    const int64_t s = c * kAdlChunk, L = total - s < kAdlChunk ? total - s : kAdlChunk;
    unsigned long long a = 0, w = 0;
    for (int64_t k = threadIdx.x; k < L; k += 256) {
      const uint32_t v = tok[s + k] & 255u;       // a marker left here would mean a resolution bug: it shows as a bad Adler-32
      out[s + k] = (uint8_t)v;
      a += v;
      w += (unsigned long long)(L - k) * v;
    }
    a = rhccq::block_sum(a, red);
    w = rhccq::block_sum(w, red);
    if (threadIdx.x == 0) {
      part[2 * c] = (uint32_t)(a % kAdlerMod);
      part[2 * c + 1] = (uint32_t)(w % kAdlerMod);
    }
    __syncthreads();
  }
}

__global__ void zi_final(const uint8_t* __restrict__ in, int64_t n, const Ctl* __restrict__ ctl, const uint32_t* __restrict__ part,
                         int64_t* __restrict__ out_len, int32_t* __restrict__ status) {
  if (threadIdx.x == 0 && blockIdx.x == 0) zi_finish(in, n, ctl, part, out_len, status);
}

__global__ void zi_stats(const Ctl* __restrict__ ctl, int64_t* __restrict__ stats) {
  if (threadIdx.x < 4) stats[threadIdx.x] = ctl->stats[threadIdx.x];
}

constexpr int64_t kMaxOut = ((int64_t)1 << 31) - 1;

}  // namespace zi

extern "C" {

int rhccq_zlib_inflate_sizes(int64_t n, int64_t out_cap, int64_t* workspace_bytes) {
  if (n < 0 || out_cap < 0 || !workspace_bytes) return RHCCQ_E_ARG;
  if (n > zi::kMaxOut || out_cap > zi::kMaxOut) return RHCCQ_E_LIMIT;
  *workspace_bytes = zi::layout(n, out_cap).total;
  return RHCCQ_OK;
}

int rhccq_zlib_decompress(rhccq_ctx* ctx, const uint8_t* in, int64_t n, void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len,
                          int32_t* status) {
  using namespace zi;
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || out_cap < 0 || (n > 0 && !in) || !workspace || !out || !out_len || !status)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib_decompress: bad argument");
  if (n > kMaxOut || out_cap > kMaxOut) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib_decompress: n and out_cap must be below 2^31");
  const Layout Ly = layout(n, out_cap);
  char* ws = (char*)workspace;
  int64_t* cand = (int64_t*)(ws + Ly.o_cand);
  Rec* rec = (Rec*)(ws + Ly.o_rec);
  int32_t* chain = (int32_t*)(ws + Ly.o_chain);
  int64_t* choff = (int64_t*)(ws + Ly.o_choff);
  Ctl* ctl = (Ctl*)(ws + Ly.o_ctl);
  uint32_t* part = (uint32_t*)(ws + Ly.o_adl);
  uint32_t* tok = (uint32_t*)(ws + Ly.o_tok);
  hipStream_t st = ctx->stream;
  const int ns = (int)Ly.ns;
  zi_find<<<ns, 256, 0, st>>>(in, n, Ly.ns, cand);
  zi_spec<<<ns, 64, 0, st>>>(in, n, cand, Ly.ns, rec);
  zi_chain_k<<<1, 64, 0, st>>>(in, n, cand, rec, Ly.ns, out_cap, chain, choff, ctl, out_len, status);
  zi_write<<<ns, 64, 0, st>>>(in, n, cand, Ly.ns, rec, chain, choff, ctl, tok, out_cap);
  const int rgrid = (int)((out_cap + 255) / 256 < 4096 ? (out_cap + 255) / 256 : 4096);
  for (int64_t k = 0; k < Ly.rounds; ++k) zi_resolve<<<rgrid > 0 ? rgrid : 1, 256, 0, st>>>(ctl, tok);
  const int egrid = (int)(Ly.nadl < 2048 ? Ly.nadl : 2048);
  zi_emit<<<egrid > 0 ? egrid : 1, 256, 0, st>>>(ctl, tok, out, part);
  zi_final<<<1, 64, 0, st>>>(in, n, ctl, part, out_len, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_zlib_inflate_stats(rhccq_ctx* ctx, int64_t n, int64_t out_cap, const void* workspace, int64_t* stats) {
  using namespace zi;
  if (!ctx) return RHCCQ_E_ARG;
  if (n < 0 || out_cap < 0 || !workspace || !stats) return rhccq_fail(ctx, RHCCQ_E_ARG, "rhccq_zlib_inflate_stats: bad argument");
  if (n > kMaxOut || out_cap > kMaxOut) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "rhccq_zlib_inflate_stats: n and out_cap must be below 2^31");
  const Layout Ly = layout(n, out_cap);
  zi_stats<<<1, 64, 0, ctx->stream>>>((const Ctl*)((const char*)workspace + Ly.o_ctl), stats);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

int rhccq_zlib_decompress_host(const uint8_t* in, int64_t n, uint8_t* out, int64_t out_cap, int64_t* out_len, int32_t* status) {
  using namespace zi;
  if (n < 0 || out_cap < 0 || (n > 0 && !in) || !out || !out_len || !status) return RHCCQ_E_ARG;
  if (n > kMaxOut || out_cap > kMaxOut) return RHCCQ_E_LIMIT;
  const Layout Ly = layout(n, out_cap);
  const int64_t ns = Ly.ns, nbits = n * 8;
  std::vector<int64_t> cand(ns, -1);
  cand[0] = 16;
  for (int64_t b = 1; b < ns; ++b)
    for (int64_t bit = b * kSpanBits; bit < (b + 1) * kSpanBits && bit + 3 <= nbits; ++bit)
      if (zi_plausible(in, n, bit)) {
        cand[b] = bit;
        break;
      }
  std::vector<Rec> rec(ns);
  std::vector<Lds> lds(1);
  for (int64_t b = 0; b < ns; ++b) {
    if (cand[b] < 0) {
      rec[b] = Rec{-1, 0, 0, -1, kNone, 0, 0};
      continue;
    }
    zi_worker<false>(in, n, cand[b], cand.data(), ns, &lds[0], nullptr, nullptr, 0, 0, 0, &rec[b], 0, 1);
  }
  std::vector<int32_t> chain(ns);
  std::vector<int64_t> choff(ns);
  Ctl ctl;
  zi_chain(in, n, cand.data(), rec.data(), ns, out_cap, chain.data(), choff.data(), &ctl, out_len, status);
  if (!ctl.go) return RHCCQ_OK;
  std::vector<uint32_t> tok(ctl.total > 0 ? ctl.total : 1), ring(kRing);
  for (int32_t k = 0; k < ctl.nchain; ++k) {
    const int c = chain[k];
    zi_worker<true>(in, n, cand[c], cand.data(), ns, &lds[0], ring.data(), tok.data(), choff[k], rec[c].nout, ctl.total, nullptr, 0, 1);
  }
  // markers point strictly backwards, so one ascending pass resolves them
  for (int64_t p = 0; p < ctl.total; ++p)
    if (tok[p] & kMark) {
      const int64_t s = tok[p] & ~kMark;
      tok[p] = s < p ? tok[s] : 0u;
    }
  std::vector<uint32_t> part(2 * Ly.nadl);
  for (int64_t p = 0; p < ctl.total; ++p) out[p] = (uint8_t)(tok[p] & 255u);
  for (int64_t c = 0; c * kAdlChunk < ctl.total; ++c) {
    const int64_t s = c * kAdlChunk;
    adler_chunk_sums(out + s, ctl.total - s < kAdlChunk ? ctl.total - s : kAdlChunk, &part[2 * c]);
  }
  zi_finish(in, n, &ctl, part.data(), out_len, status);
  return RHCCQ_OK;
}

}  // extern "C"
