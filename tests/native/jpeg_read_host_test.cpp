// The host side of the JPEG reader without a device and without the library (csrc/jpeg_read.h is plain C++): the parse and the serial
// decode over a corpus of valid and malformed files and over each of them cut at 20 places, in buffers of exactly the sizes the parse
// promises.  Built with the host sanitizers by tests/test_jpeg_read_cpu.py, which writes the corpus: argv[1] is a directory holding
// `manifest` (lines "file has_pixels") and the files it names; for a file F with has_pixels = 1, F.rgb holds the expected image.  Prints
// "name status detail" a file, which the test compares with the library's host form.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "jpeg_read.h"

using namespace rhccq::jpegr;

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path.c_str());
    std::exit(2);
  }
  return std::vector<uint8_t>((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
}

struct Decoded {
  int32_t status, detail;
  std::vector<uint8_t> rgb;
};

// the file in a buffer of exactly n bytes; every other buffer of exactly the size the parse names
static Decoded decode(const std::vector<uint8_t>& file) {
  const int64_t n = (int64_t)file.size();
  rhccq_jpeg_info f;
  rhccq_jpeg_tables T;
  jpeg_parse(file.data(), n, &f, &T, nullptr, 0);
  Decoded out{f.status, f.detail, {}};
  if (f.status != RHCCQ_JPEG_OK) return out;
  if (!info_sound(f, n)) {
    std::fprintf(stderr, "an accepted file whose info fails the kernels' own test\n");
    std::exit(1);
  }
  std::vector<rhccq_segment> iv((size_t)f.n_intervals);
  jpeg_parse(file.data(), n, &f, &T, iv.data(), (int64_t)iv.size());
  std::vector<uint32_t> words((size_t)((f.stream_bytes + kStreamPad) / 4 + 2), 0u);
  unstuff_serial(file.data(), n, f, (uint8_t*)words.data());
  Dec d{words.data(), &T, iv.data(), f.n_intervals, 8 * f.stream_bytes, geo_of(f)};
  std::vector<int16_t> coef((size_t)(64 * f.blocks), 0);
  uint32_t bad = kNoInterval, count;
  uint64_t leave;
  run<true>(d, pack(0, 0, 0), true, d.total_bits, 0, coef.data(), &bad, &leave, &count);
  // the same stream cut into subsequences from true entries: what the kernels' lanes do
  std::vector<int16_t> coef2((size_t)(64 * f.blocks), 0);
  uint32_t bad2 = kNoInterval;
  uint64_t entry = pack(0, 0, 0);
  int64_t A = 0;
  for (int64_t g = 0; g < sub_count(f.stream_bytes, 128); ++g) {
    const int64_t end = (g + 1) * 128 < d.total_bits ? (g + 1) * 128 : d.total_bits;
    run<true>(d, entry, g == 0, end, A, coef2.data(), &bad2, &leave, &count);
    A = count & kAbs ? (int64_t)(count & ~kAbs) : A + count;
    entry = leave;
  }
  if (coef != coef2 || bad != bad2) {
    std::fprintf(stderr, "the decode in subsequences differs from the decode in one piece\n");
    std::exit(1);
  }
  dc_serial(d.g, coef.data());
  std::vector<uint8_t> planes((size_t)(64 * f.blocks));
  planes_serial(d.g, T, coef.data(), planes.data());
  out.rgb.resize((size_t)3 * f.width * f.height);
  rgb_serial(d.g, planes.data(), out.rgb.data());
  if (bad != kNoInterval) out.status = RHCCQ_JPEG_BAD_SCAN, out.detail = (int32_t)bad;
  return out;
}

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const std::string dir = argv[1];
  std::ifstream manifest(dir + "/manifest");
  std::string line;
  while (std::getline(manifest, line)) {
    std::istringstream in(line);
    std::string name;
    int has_pixels = 0;
    in >> name >> has_pixels;
    const std::vector<uint8_t> file = slurp(dir + "/" + name);
    const Decoded d = decode(file);
    if (has_pixels && d.rgb != slurp(dir + "/" + name + ".rgb")) {
      std::fprintf(stderr, "%s: pixels differ\n", name.c_str());
      return 1;
    }
    std::printf("%s %d %d\n", name.c_str(), d.status, d.detail);
    for (int cut = 0; cut < 20; ++cut) {
      const size_t m = file.size() * (size_t)cut / 20 + (size_t)cut % 3;
      decode(std::vector<uint8_t>(file.begin(), file.begin() + (m < file.size() ? m : file.size())));
    }
  }
  return 0;
}
