// The host side of the GIF reader without a device and without the library (csrc/gif_read.h is plain C++): the parser over a corpus of
// valid and malformed files, over every prefix of each of them and with tables too small for them, then the serial decoder and composer
// over buffers of exactly the sizes the parse promises.  Built with the host sanitizers by tests/test_gif_read_cpu.py, which writes the
// corpus: argv[1] is a directory holding `manifest` (lines "file status detail has_pixels") and the files it names; for a file F with
// has_pixels = 1, F.rgb and F.alpha hold the expected images.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "gif_read.h"

using namespace rhccq::gifr;

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

struct Parsed {
  rhccq_gif_info info;
  std::vector<rhccq_gif_frame> frames;
  std::vector<rhccq_segment> blocks;
};

static Parsed parse(const uint8_t* f, int64_t n) {
  Parsed p;
  gif_parse(f, n, &p.info, nullptr, 0, nullptr, 0);
  p.frames.resize((size_t)p.info.n_frames);
  p.blocks.resize((size_t)p.info.n_blocks);
  gif_parse(f, n, &p.info, p.frames.data(), (int64_t)p.frames.size(), p.blocks.data(), (int64_t)p.blocks.size());
  return p;
}

// what a parse promises whatever the bytes were: every row and every offset it reports lies inside the n bytes, and the places it assigns
// in the joined streams, the pixel strings and the segment table do not overlap
static int sound(const Parsed& p, int64_t n, const char* name) {
  const rhccq_gif_info& f = p.info;
  CHECK(f.n_frames >= 0 && f.n_blocks >= 0 && f.n_blocks <= n && (int64_t)f.n_frames * 12 <= n, "%s: counts", name);
  int64_t stream = 0, pixels = 0, rows = 0, block = 0;
  for (int64_t i = 0; i < f.n_frames; ++i) {
    const rhccq_gif_frame& g = p.frames[(size_t)i];
    CHECK(g.w >= 1 && g.h >= 1 && g.x >= 0 && g.y >= 0 && g.x + g.w <= f.width && g.y + g.h <= f.height, "%s: frame %lld leaves the screen", name, (long long)i);
    CHECK(g.m >= 2 && g.m <= 8 && g.table_rows >= 2 && g.table_rows <= 256 && g.table_offset >= 13 && g.table_offset + 3 * g.table_rows <= n, "%s: table of frame %lld",
          name, (long long)i);
    CHECK(g.stream_offset == stream && g.pixel_offset == pixels && g.first_row == rows && g.first_block == block, "%s: places of frame %lld", name, (long long)i);
    int64_t acc = 0;
    for (int64_t b = block; b < block + g.n_blocks; ++b) {
      const rhccq_segment& s = p.blocks[(size_t)b];
      CHECK(s.offset >= 13 && s.length >= 1 && s.length <= 255 && s.offset + s.length < n && s.first_piece == i && s.dst == stream + acc, "%s: sub-block %lld", name,
            (long long)b);
      acc += s.length;
    }
    CHECK(acc == g.stream_bytes, "%s: stream bytes of frame %lld", name, (long long)i);
    block += g.n_blocks;
    stream = ((stream + acc + 15) & ~(int64_t)15) + kStreamPad;
    pixels += (int64_t)g.w * g.h;
    rows += seg_bound(acc, g.m);
    CHECK(frame_lzw_sound(g, stream, pixels, rows) && frame_paint_sound(g, n, pixels), "%s: frame %lld fails the kernels' own test", name, (long long)i);
  }
  CHECK(block == f.n_blocks && stream == f.stream_bytes && pixels == f.pixels && rows == f.seg_rows, "%s: totals", name);
  if (f.status == RHCCQ_GIFR_OK) CHECK(f.n_frames >= 1 && f.width >= 1 && f.height >= 1, "%s: an accepted file without a frame", name);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  std::ifstream manifest(dir + "/manifest");
  std::string line;
  int files = 0;
  while (std::getline(manifest, line)) {
    std::istringstream in(line);
    std::string name;
    int status = 0, detail = 0, has_pixels = 0;
    in >> name >> status >> detail >> has_pixels;
    const std::vector<uint8_t> file = slurp(dir + "/" + name);
    const int64_t n = (int64_t)file.size();
    const Parsed p = parse(file.data(), n);
    const rhccq_gif_info& f = p.info;
    if (status <= RHCCQ_GIFR_LIMIT) CHECK(f.status == status && f.detail == detail, "%s: status %d detail %d, expected %d %d", name.c_str(), f.status, f.detail, status, detail);
    else CHECK(f.status == RHCCQ_GIFR_OK, "%s: the parser refuses a file the decoder is to refuse", name.c_str());
    if (sound(p, n, name.c_str())) return 1;
    // every prefix, in a buffer of exactly that size (a read past it is the sanitizer's to see), and tables of 0, 1 and 2 rows
    for (int64_t m = 0; m <= n; m += (n > 4096 && m > 64 && m < n - 64 ? 61 : 1)) {   // (a long file: not every prefix in its middle)
      const std::vector<uint8_t> cut(file.begin(), file.begin() + m);
      const Parsed g = parse(cut.data(), m);
      if (sound(g, m, name.c_str())) return 1;
      for (int64_t cap = 0; cap <= 2 && m % 7 == 0; ++cap) {
        std::vector<rhccq_gif_frame> t3((size_t)cap);
        std::vector<rhccq_segment> b3((size_t)cap);
        rhccq_gif_info h;
        gif_parse(cut.data(), m, &h, cap ? t3.data() : nullptr, cap, cap ? b3.data() : nullptr, cap);
        CHECK(h.status == g.info.status && h.detail == g.info.detail && h.n_frames == g.info.n_frames && h.n_blocks == g.info.n_blocks && h.seg_rows == g.info.seg_rows,
              "%s: small tables change the parse", name.c_str());
      }
    }
    if (f.status == RHCCQ_GIFR_OK) {
      // the decoder and the composer over buffers of exactly the promised sizes
      std::vector<uint8_t> streams((size_t)f.stream_bytes, 0), pixels((size_t)f.pixels, 0);
      for (const rhccq_segment& s : p.blocks)
        for (int64_t j = 0; j < s.length; ++j) streams[(size_t)(s.dst + j)] = file[(size_t)(s.offset + j)];
      std::vector<int64_t> counts((size_t)f.n_frames);
      uint32_t bc = 0, bl = 0;
      int64_t segs = 0;
      unlzw_serial(streams.data(), f.stream_bytes, p.frames.data(), f.n_frames, pixels.data(), f.pixels, counts.data(), &bc, &bl, &segs);
      const Verdict v = gif_verdict(bc, bl);
      CHECK(segs <= f.seg_rows, "%s: more segments than the table's rows", name.c_str());
      if (status > RHCCQ_GIFR_LIMIT) CHECK(v.status == status && v.detail == detail, "%s: status %d detail %d, expected %d %d", name.c_str(), v.status, v.detail, status, detail);
      else CHECK(v.status == RHCCQ_GIFR_OK, "%s: the decoder refuses the file (%d, %d)", name.c_str(), v.status, v.detail);
      const size_t hw = (size_t)f.width * f.height * f.n_frames;
      std::vector<uint8_t> rgb(3 * hw), alpha(hw), idx((size_t)f.pixels);
      compose_serial(pixels.data(), f.pixels, file.data(), n, p.frames.data(), f.n_frames, f.height, f.width, rgb.data(), alpha.data(), idx.data());
      if (has_pixels) {
        CHECK(rgb == slurp(dir + "/" + name + ".rgb") && alpha == slurp(dir + "/" + name + ".alpha"), "%s: pixels differ", name.c_str());
      }
    }
    ++files;
  }
  CHECK(files > 0, "an empty manifest");
  std::printf("gif_read_host ok %d\n", files);
  return 0;
}
