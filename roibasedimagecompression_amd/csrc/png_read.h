// PNG reading (EXTENSION, include/rhccq.h "PNG files read on the device"): the functions the kernels of png_read.hip and the serial host
// forms share.  Plain C++ over <stdint.h> (and png_write.h for Paeth and the CRC algebra): a host-only program may include this file
// without the HIP headers.
//   parse      png_parse: the file's framing, a pure function of its bytes; every offset and length it reports lies inside the file;
//   unfilter   unf_byte (one byte under one of the five filters) and the geometry of the banded wavefront and its hand-over words;
//   expand     expand_pixel: one pixel of any colour type and depth to R, G, B, alpha and index.
#pragma once
#include "band_handoff.h"
#include "png_write.h"

namespace rhccq {
namespace pngr {
using namespace png;

// ---- the file's geometry -------------------------------------------------------------------------------------------------------------
RHCCQ_PNG_HD int channels_of(int colour_type) { return colour_type == 0 ? 1 : colour_type == 2 ? 3 : colour_type == 3 ? 1 : colour_type == 4 ? 2 : 4; }
RHCCQ_PNG_HD bool depth_allowed(int colour_type, int depth) {
  const bool d816 = depth == 8 || depth == 16, low = depth == 1 || depth == 2 || depth == 4;
  switch (colour_type) {
    case 0: return low || d816;
    case 3: return low || depth == 8;
    case 2: case 4: case 6: return d816;
    default: return false;
  }
}
RHCCQ_PNG_HD int bpp_of(int colour_type, int depth) {
  const int b = channels_of(colour_type) * depth / 8;
  return b < 1 ? 1 : b;
}
RHCCQ_PNG_HD int64_t rowbytes_of(int64_t W, int colour_type, int depth) { return (W * channels_of(colour_type) * depth + 7) / 8; }
RHCCQ_PNG_HD bool bpp_allowed(int bpp) { return bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8; }

inline uint32_t get_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | (uint32_t)p[3]; }
inline bool type_is(const uint8_t* p, const char* t) { return p[0] == (uint8_t)t[0] && p[1] == (uint8_t)t[1] && p[2] == (uint8_t)t[2] && p[3] == (uint8_t)t[3]; }

constexpr int64_t kReadMax = ((int64_t)1 << 31) - 1;       // the inflater's limit on both of its lengths

// pieces of the CRC over a table row (rhccq_crc32_segments): laid from the 16-byte aligned offset at or below the row's
RHCCQ_PNG_HD int64_t seg_pieces(int64_t offset, int64_t length) { return length <= 0 ? 0 : crc_pieces(offset & 15, length); }
// a row's range tested against the buffer: the bytes it covers, or 0 when it does not lie inside
RHCCQ_PNG_HD int64_t seg_bytes(int64_t offset, int64_t length, int64_t extra, int64_t n) {
  if (offset < 0 || length < 0 || extra < 0 || offset > n || length > n - offset || extra > n - offset - length) return 0;
  return length + extra;
}
inline int64_t seg_plan(rhccq_segment* table, int64_t n_seg, int64_t extra) {
  int64_t total = 0;
  for (int64_t i = 0; i < n_seg; ++i) {
    table[i].first_piece = total;
    total += seg_pieces(table[i].offset, table[i].length < 0 ? 0 : table[i].length + extra);
  }
  return total;
}

// ---- parse ---------------------------------------------------------------------------------------------------------------------------
// fills *info and the first `cap` rows of `chunks`; returns the number of chunks walked
inline int64_t png_parse(const uint8_t* f, int64_t n, rhccq_png_info* info, rhccq_segment* chunks, int64_t cap) {
  static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
  rhccq_png_info z{};
  z.plte_offset = z.trns_offset = -1;
  z.first_idat = -1;
  auto done = [&](int status, int64_t detail, int64_t count) {
    z.status = status;
    z.detail = (int32_t)(detail > kReadMax ? kReadMax : detail);
    z.n_chunks = (int32_t)count;
    *info = z;
    return count;
  };
  if (n < 8) return done(RHCCQ_PNG_BAD_SIGNATURE, 0, 0);
  for (int i = 0; i < 8; ++i)
    if (f[i] != sig[i]) return done(RHCCQ_PNG_BAD_SIGNATURE, 0, 0);

  // the walk: what the chunks' framing shows without the header's contents
  int64_t pos = 8, count = 0, plte_len = -1, trns_len = -1, ihdr_len = -1, idat_total = 0;
  int framing = 0;                                         // RHCCQ_PNG_BAD_CHUNK once a fault shows
  int64_t framing_at = 0;
  bool seen_idat = false, seen_iend = false, last_idat = false, trns_before_plte = false;
  auto bad = [&](int64_t at) {
    framing = RHCCQ_PNG_BAD_CHUNK;
    framing_at = at;
  };
  while (!seen_iend) {
    if (n - pos < 12) { bad(count); break; }                                               // (no IEND, or a chunk cut short)
    const uint64_t len = get_be32(f + pos);
    if (len > (uint64_t)kReadMax || (int64_t)len > n - pos - 12) { bad(count); break; }
    const uint8_t* type = f + pos + 4;
    const int64_t data = pos + 8;
    rhccq_segment row{pos + 4, (int64_t)len, 0, -1};
    bool stop = false;
    if (count == 0 && !type_is(type, "IHDR")) { bad(0); break; }
    if (type_is(type, "IHDR")) {
      if (count > 0) stop = true;
      else ihdr_len = (int64_t)len;
    } else if (type_is(type, "PLTE")) {
      if (plte_len >= 0 || seen_idat) stop = true;
      plte_len = (int64_t)len;
      z.plte_offset = data;
      last_idat = false;
    } else if (type_is(type, "tRNS")) {
      if (trns_len >= 0 || seen_idat) stop = true;
      trns_len = (int64_t)len;
      z.trns_offset = data;
      trns_before_plte = plte_len < 0;
      last_idat = false;
    } else if (type_is(type, "IDAT")) {
      if (seen_idat && !last_idat) stop = true;
      if (!seen_idat) z.first_idat = (int32_t)count;
      if (!stop) {
        row.dst = idat_total;
        idat_total += (int64_t)len;
        ++z.n_idat;
      }
      seen_idat = last_idat = true;
    } else if (type_is(type, "IEND")) {
      if (len != 0 || !seen_idat) stop = true;
      seen_iend = true;
    } else {
      if (!(type[0] & 0x20)) stop = true;                                                  // an unknown critical chunk
      last_idat = false;
    }
    if (stop) { bad(count); break; }
    if (count < cap) chunks[count] = row;
    ++count;
    pos += 12 + (int64_t)len;
  }
  z.idat_bytes = idat_total;
  z.crc_pieces = 0;
  {
    int64_t total = 0;
    const int64_t rows = count < cap ? count : cap;
    for (int64_t i = 0; i < rows; ++i) {
      chunks[i].first_piece = total;
      total += seg_pieces(chunks[i].offset, chunks[i].length + 4);
    }
    z.crc_pieces = total;
  }

  // the header
  int header = 0;
  if (ihdr_len >= 0) {
    if (ihdr_len != 13) {
      header = RHCCQ_PNG_BAD_HEADER;
    } else {
      const uint8_t* h = f + 16;
      const uint32_t w = get_be32(h), hh = get_be32(h + 4);
      z.depth = h[8];
      z.colour_type = h[9];
      z.interlace = h[12];
      if (w < 1 || hh < 1 || w > (uint32_t)kReadMax || hh > (uint32_t)kReadMax || !depth_allowed(z.colour_type, z.depth) || h[10] != 0 || h[11] != 0 || h[12] > 1) {
        header = RHCCQ_PNG_BAD_HEADER;
      } else {
        z.width = (int32_t)w;
        z.height = (int32_t)hh;
        z.channels = channels_of(z.colour_type);
        z.bpp = bpp_of(z.colour_type, z.depth);
        z.rowbytes = rowbytes_of(w, z.colour_type, z.depth);
      }
    }
  }
  if (framing) return done(framing, framing_at, count);
  if (header) return done(header, 0, count);
  // what the header decides about PLTE and tRNS
  const int ct = z.colour_type;
  if (ct == 3) {
    if (plte_len < 3 || plte_len % 3 || plte_len > 768 || trns_before_plte || trns_len > plte_len / 3) return done(RHCCQ_PNG_BAD_CHUNK, count, count);
    z.palette_rows = (int32_t)(plte_len / 3);
  } else {
    if ((ct == 0 || ct == 4) && plte_len >= 0) return done(RHCCQ_PNG_BAD_CHUNK, count, count);
    if (trns_len >= 0 && ((ct == 0 && trns_len != 2) || (ct == 2 && trns_len != 6) || ct == 4 || ct == 6)) return done(RHCCQ_PNG_BAD_CHUNK, count, count);
    z.plte_offset = -1;                                                                    // ignored for colour types 2 and 6
  }
  z.trns_bytes = (int32_t)(trns_len > 0 ? trns_len : 0);
  if (trns_len <= 0) z.trns_offset = -1;
  if (z.interlace) return done(RHCCQ_PNG_UNSUPPORTED, 1, count);
  // (1 + rowbytes <= 2^34 and H < 2^31: the product is inside int64)
  if ((1 + z.rowbytes) > kReadMax / z.height || idat_total > kReadMax) return done(RHCCQ_PNG_LIMIT, 0, count);
  z.scan_bytes = (1 + z.rowbytes) * z.height;
  return done(RHCCQ_PNG_OK, 0, count);
}

// ---- unfilter ------------------------------------------------------------------------------------------------------------------------
constexpr int kUnfRows = 64;                               // rows of a band: a lane a row
constexpr int kUnfTile = 32;                               // steps of a staging tile
constexpr int kUnfGranule = 16;                            // filter units a band fetches from its predecessor at a time (band_handoff.h)
constexpr int kUnfBadWord = 2, kUnfStalledWord = 3;        // the caller's words of the workspace's head: H - (first bad row), stalled

RHCCQ_PNG_HD int unf_unit_words(int bpp) { return (bpp + 2) / 3; }
inline int64_t unf_bands(int64_t H) { return (H + kUnfRows - 1) / kUnfRows; }
// words of one handed-over row
inline int64_t unf_row_words(int64_t rowbytes, int bpp) { return rowbytes / bpp * unf_unit_words(bpp); }
inline int64_t unf_work_bytes(int64_t H, int64_t rowbytes, int bpp) { return band::work_bytes(unf_bands(H), unf_row_words(rowbytes, bpp)); }

// the raw byte of the filtered byte x under type t (0..4) with a = left, b = above, c = upper left (raw bytes)
RHCCQ_PNG_HD uint32_t unf_byte(int t, uint32_t x, uint32_t a, uint32_t b, uint32_t c) {
  const uint32_t paeth = (uint32_t)png_paeth((int)a, (int)b, (int)c);
  const uint32_t pred = t == 1 ? a : t == 2 ? b : t == 3 ? (a + b) >> 1 : t == 4 ? paeth : 0u;
  return (x + pred) & 255u;
}

// the serial form; returns H - (first bad row), 0 for none
inline int64_t unfilter_serial(const uint8_t* scan, int64_t H, int64_t rowbytes, int bpp, uint8_t* raw) {
  int64_t first_bad = -1;
  for (int64_t y = 0; y < H; ++y) {
    const uint8_t* in = scan + y * (rowbytes + 1);
    uint8_t* out = raw + y * rowbytes;
    const uint8_t* up = y > 0 ? out - rowbytes : nullptr;
    int t = in[0];
    if (t > 4) {
      if (first_bad < 0) first_bad = y;
      t = 0;
    }
    for (int64_t i = 0; i < rowbytes; ++i) {
      const uint32_t a = i >= bpp ? out[i - bpp] : 0u, b = up ? up[i] : 0u, c = up && i >= bpp ? up[i - bpp] : 0u;
      out[i] = (uint8_t)unf_byte(t, in[1 + i], a, b, c);
    }
  }
  return first_bad < 0 ? 0 : H - first_bad;
}

// ---- expand --------------------------------------------------------------------------------------------------------------------------
struct Pixel { uint8_t r, g, b, a, idx; };

// sample s (of `depth` bits, counted from the row's start) of a raw row, at its full depth
RHCCQ_PNG_HD uint32_t expand_sample(const uint8_t* row, int64_t s, int depth) {
  if (depth == 8) return row[s];
  if (depth == 16) return (uint32_t)row[2 * s] << 8 | row[2 * s + 1];
  const int64_t bit = s * depth;
  return (row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1u << depth) - 1u);
}
RHCCQ_PNG_HD uint32_t expand_key(const uint8_t* trns, int i, int depth) {
  const uint32_t k = (uint32_t)trns[2 * i] << 8 | trns[2 * i + 1];
  return depth == 16 ? k : k & ((1u << depth) - 1u);
}
// a sample as 8 bits: scaled below 8 (255 / (2^d - 1) is 255, 85 or 17), the high byte at 16
RHCCQ_PNG_HD uint32_t expand_to8(uint32_t v, int depth) {
  return depth == 8 ? v : depth == 16 ? v >> 8 : depth == 1 ? v * 255u : depth == 2 ? v * 85u : v * 17u;
}
RHCCQ_PNG_HD Pixel expand_pixel(const uint8_t* row, int64_t x, int colour_type, int depth, const uint8_t* palette, int K, const uint8_t* trns, int trns_bytes) {
  Pixel p{0, 0, 0, 255, 0};
  if (colour_type == 3) {
    uint32_t i = expand_sample(row, x, depth);
    p.idx = (uint8_t)i;
    if (i < (uint32_t)trns_bytes) p.a = trns[i];
    if (i >= (uint32_t)K) i = 0;
    p.r = palette[3 * i];
    p.g = palette[3 * i + 1];
    p.b = palette[3 * i + 2];
  } else if (colour_type == 0 || colour_type == 4) {
    const int ch = colour_type == 0 ? 1 : 2;
    const uint32_t v = expand_sample(row, x * ch, depth);
    p.r = p.g = p.b = (uint8_t)expand_to8(v, depth);
    if (ch == 2) p.a = (uint8_t)expand_to8(expand_sample(row, x * 2 + 1, depth), depth);
    else if (trns_bytes >= 2 && v == expand_key(trns, 0, depth)) p.a = 0;
  } else {
    const int ch = colour_type == 2 ? 3 : 4;
    const uint32_t r = expand_sample(row, x * ch, depth), g = expand_sample(row, x * ch + 1, depth), b = expand_sample(row, x * ch + 2, depth);
    p.r = (uint8_t)expand_to8(r, depth);
    p.g = (uint8_t)expand_to8(g, depth);
    p.b = (uint8_t)expand_to8(b, depth);
    if (ch == 4) p.a = (uint8_t)expand_to8(expand_sample(row, x * 4 + 3, depth), depth);
    else if (trns_bytes >= 6 && r == expand_key(trns, 0, depth) && g == expand_key(trns, 1, depth) && b == expand_key(trns, 2, depth)) p.a = 0;
  }
  return p;
}
inline void expand_serial(const uint8_t* raw, int64_t H, int64_t W, int colour_type, int depth, const uint8_t* palette, int K, const uint8_t* trns,
                          int trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx) {
  const int64_t rb = rowbytes_of(W, colour_type, depth);
  for (int64_t y = 0; y < H; ++y)
    for (int64_t x = 0; x < W; ++x) {
      const Pixel p = expand_pixel(raw + y * rb, x, colour_type, depth, palette, K, trns, trns_bytes);
      const int64_t o = y * W + x;
      rgb[3 * o] = p.r;
      rgb[3 * o + 1] = p.g;
      rgb[3 * o + 2] = p.b;
      if (alpha) alpha[o] = p.a;
      if (idx && colour_type == 3) idx[o] = p.idx;
    }
}
inline int expand_check(int64_t H, int64_t W, int colour_type, int depth, const void* palette, int K, const void* trns, int trns_bytes) {
  if (H < 1 || W < 1 || !depth_allowed(colour_type, depth)) return RHCCQ_E_ARG;
  if (colour_type == 3 && (!palette || K < 1 || K > 256)) return RHCCQ_E_ARG;
  if (trns_bytes < 0 || trns_bytes > 256 || (trns_bytes > 0 && !trns)) return RHCCQ_E_ARG;
  return 0;
}

// the last stages' words folded into one status by the precedence of include/rhccq.h (the host framing statuses never reach here)
struct Verdict { int32_t status, detail; };
RHCCQ_PNG_HD Verdict png_verdict(int64_t first_bad_crc, int32_t zs, int64_t zlen, int64_t scan_bytes, int64_t bad_from_end, int64_t H, uint32_t stalled) {
  const int64_t cap = ((int64_t)1 << 31) - 1;
  if (first_bad_crc >= 0) return {RHCCQ_PNG_BAD_CRC, (int32_t)first_bad_crc};
  if (zs == RHCCQ_ZS_CAPACITY || (zs == RHCCQ_ZS_OK && zlen != scan_bytes)) return {RHCCQ_PNG_BAD_LENGTH, (int32_t)(zlen < 0 ? 0 : zlen > cap ? cap : zlen)};
  if (zs != RHCCQ_ZS_OK) return {RHCCQ_PNG_BAD_STREAM, zs};
  if (bad_from_end > 0) return {RHCCQ_PNG_BAD_FILTER, (int32_t)(H - bad_from_end)};
  if (stalled) return {RHCCQ_PNG_STALLED, 0};
  return {RHCCQ_PNG_OK, 0};
}

}  // namespace pngr
}  // namespace rhccq
