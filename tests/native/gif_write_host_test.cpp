// The GIF writer's step functions without a device and without the library (csrc/gif_write.h is plain C++): every case of
// tests/gif_cases.py is encoded from the header's functions alone -- the segment loop over BOTH dictionaries, the bit join, the sub-blocks, the framing -- into
// buffers of exactly the sizes the header's bounds promise, and compared with the reference's file.  Built with the host sanitizers by
// tests/test_gif_write_cpu.py, which writes the corpus: argv[1] is a directory holding `manifest` (a case name a line) and, for every
// NAME, NAME.in (int32 n, H, W, flags, loop, k_stride, k_rows[n], delays[n]; the palettes uint8[tables][k_stride][3]; the indices
// uint32[n][H][W]) and NAME.gif.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "gif_write.h"

using namespace rhccq::gif;

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::fprintf(stderr, __VA_ARGS__); \
      std::fprintf(stderr, "\n");        \
      return 1;                          \
    }                                    \
  } while (0)

// frame f's stream: a buffer of exactly gif_stream_bound bytes, segments in slots of exactly gif_slot_words words
static int frame_stream(const uint32_t* idx, int64_t P, int f, int K, int flags, bool trie, std::vector<uint8_t>& stream, const char* name) {
  const int m = gif_min_code(gif_table_bits(gif_entries(K, flags)));
  const bool delta = (flags & RHCCQ_GIF_DELTA) && f > 0;
  const int64_t nseg = gif_segments(P), slot = gif_slot_words(P);
  std::vector<uint32_t> dict(trie ? kTrieNodes : kDictSlots);     // (exactly the dictionary's size: a probe past it is a report)
  std::vector<uint8_t> out((size_t)gif_stream_bound(P));
  uint64_t acc = 0;
  int fill = 0;
  int64_t at = 0;
  for (int64_t s = 0; s < nseg; ++s) {
    const int64_t p0 = s * kSegment, len = P - p0 < kSegment ? P - p0 : kSegment;
    std::vector<uint32_t> words((size_t)slot);                       // (a fresh exact-size slot: a store past it is a report)
    std::fill(dict.begin(), dict.end(), 0u);
    Lzw z;
    BitSink sink;
    sink_begin(sink, words.data());
    lzw_begin(z, m, s == 0, sink);
    const uint32_t* cur = idx + (int64_t)f * P + p0;
    for (int64_t i = 0; i < len; ++i) {
      const uint32_t px = gif_substitute(cur[i], delta ? cur[i - P] : 0u, (uint32_t)K, delta);
      if (trie ? lzw_pixel_trie(z, dict.data(), px, sink) : lzw_pixel(z, dict.data(), px, sink)) std::fill(dict.begin(), dict.end(), 0u);
    }
    const int64_t bits = lzw_finish(z, s == nseg - 1, sink);
    CHECK(bits <= gif_segment_bits(len) && sink.words <= slot, "%s: segment %lld of frame %d breaks its bound", name, (long long)s, f);
    for (int64_t r = 0; r < bits; r += 32) {
      acc |= (uint64_t)gif_bits_at(words.data(), bits, r) << fill;
      fill += (int)(bits - r < 32 ? bits - r : 32);
      for (; fill >= 8; fill -= 8, acc >>= 8) out[(size_t)at++] = (uint8_t)acc;
    }
  }
  if (fill) out[(size_t)at++] = (uint8_t)acc;
  out.resize((size_t)at);
  stream.swap(out);
  return 0;
}

static int one_case(const std::string& dir, const std::string& name) {
  const std::vector<uint8_t> in = slurp(dir + "/" + name + ".in"), want = slurp(dir + "/" + name + ".gif");
  CHECK(in.size() >= 24, "%s: short input", name.c_str());
  int32_t head[6];
  std::memcpy(head, in.data(), sizeof head);
  const int n = head[0], H = head[1], W = head[2], flags = head[3], loop = head[4], stride = head[5];
  const bool local = flags & RHCCQ_GIF_LOCAL;
  const int tables = local ? n : 1;
  const int64_t P = (int64_t)H * W;
  CHECK(in.size() == 24 + 8 * (size_t)n + 3 * (size_t)tables * stride + 4 * (size_t)n * P, "%s: input size", name.c_str());
  std::vector<int32_t> k_rows((size_t)n), delays((size_t)n);
  std::memcpy(k_rows.data(), in.data() + 24, 4 * (size_t)n);
  std::memcpy(delays.data(), in.data() + 24 + 4 * (size_t)n, 4 * (size_t)n);
  const uint8_t* pal = in.data() + 24 + 8 * (size_t)n;
  std::vector<uint32_t> idx((size_t)(n * P));
  std::memcpy(idx.data(), pal + 3 * (size_t)tables * stride, 4 * idx.size());

  std::vector<uint8_t> out(want.size());                              // (exactly the reference's length)
  const int64_t front = gif_front_bytes(n, k_rows[0], flags);
  CHECK(front + 1 <= (int64_t)out.size(), "%s: front bytes", name.c_str());
  gif_put_head(out.data(), W, H, n, k_rows[0], flags, loop);
  if (!local)
    for (int e = 0; e < 1 << gif_table_bits(gif_entries(k_rows[0], flags)); ++e) gif_put_entry(out.data() + kHeadBytes, pal, k_rows[0], e);
  int64_t at = front;
  std::vector<uint8_t> stream;
  for (int f = 0; f < n; ++f) {
    const int k = k_rows[(size_t)f];
    std::vector<uint8_t> other;
    if (frame_stream(idx.data(), P, f, k, flags, false, stream, name.c_str()) || frame_stream(idx.data(), P, f, k, flags, true, other, name.c_str())) return 1;
    CHECK(other == stream, "%s: frame %d: the trie's stream differs from the hash table's", name.c_str(), f);
    const int64_t L = (int64_t)stream.size();
    CHECK(L <= gif_stream_bound(P), "%s: frame %d breaks the stream bound", name.c_str(), f);
    CHECK(at + gif_frame_front(k, flags) + gif_sub_len(L) + 1 <= (int64_t)out.size(), "%s: frame %d leaves the file", name.c_str(), f);
    uint8_t* p = out.data() + at;
    gif_put_frame_head(p, W, H, k, flags, delays[(size_t)f], (flags & RHCCQ_GIF_DELTA) && f > 0);
    if (local)
      for (int e = 0; e < 1 << gif_table_bits(k); ++e) gif_put_entry(p + kFrameHeadBytes, pal + 3 * (size_t)f * stride, k, e);
    p += gif_frame_front(k, flags);
    for (int64_t b = 0; b < L; ++b) {
      if (b % 255 == 0) p[gif_sub_pos(b) - 1] = (uint8_t)(L - b < 255 ? L - b : 255);
      p[gif_sub_pos(b)] = stream[(size_t)b];
    }
    p[gif_sub_len(L) - 1] = 0;
    at += gif_frame_front(k, flags) + gif_sub_len(L);
  }
  out[(size_t)at++] = 0x3B;
  CHECK(at == (int64_t)want.size(), "%s: %lld bytes, %zu expected", name.c_str(), (long long)at, want.size());
  CHECK(out == want, "%s: the file differs from the reference", name.c_str());
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  static const int64_t at[8] = {0, 1, 254, 255, 256, 509, 510, 511}, pos[8] = {1, 2, 255, 257, 258, 511, 513, 514};
  for (int i = 0; i < 8; ++i) CHECK(gif_sub_pos(at[i]) == pos[i], "gif_sub_pos(%lld)", (long long)at[i]);
  CHECK(gif_sub_len(1) == 3 && gif_sub_len(255) == 257 && gif_sub_len(256) == 259, "gif_sub_len");
  CHECK(gif_table_bits(1) == 1 && gif_table_bits(2) == 1 && gif_table_bits(3) == 2 && gif_table_bits(256) == 8 && gif_min_code(1) == 2, "table bits");
  std::ifstream manifest(dir + "/manifest");
  std::string name;
  int count = 0;
  while (std::getline(manifest, name)) {
    if (name.empty()) continue;
    if (one_case(dir, name)) return 1;
    ++count;
  }
  std::printf("gif_write_host ok %d\n", count);
  return 0;
}
