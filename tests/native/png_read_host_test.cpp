// The host side of the PNG reader without a device and without the library (csrc/png_read.h is plain C++): the parser over a corpus of
// valid and malformed files, over every prefix of each of them and with chunk tables too small for them, then the unfilter and expand
// step functions over the inflated scanlines of the valid ones.  Built with the host sanitizers by tests/test_png_read_cpu.py, which
// writes the corpus: argv[1] is a directory holding `manifest` (lines "file status detail has_scan") and the files it names; for a file
// F with has_scan = 1, F.scan holds the inflated scanlines and F.rgb the expected pixels.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iterator>
#include <sstream>
#include <string>
#include <vector>

#include "png_read.h"

using namespace rhccq::pngr;

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

// what a parse promises whatever the bytes were: every row and every offset it reports lies inside the n bytes
static int sound(const rhccq_png_info& f, const std::vector<rhccq_segment>& t, int64_t count, int64_t n, const char* name) {
  CHECK(count >= 0 && count <= n / 12 + 1 && f.n_chunks == count, "%s: chunk count %lld", name, (long long)count);
  const int64_t rows = count < (int64_t)t.size() ? count : (int64_t)t.size();
  for (int64_t i = 0; i < rows; ++i)
    CHECK(t[i].offset >= 12 && t[i].length >= 0 && t[i].offset + 4 + t[i].length + 4 <= n, "%s: chunk %lld leaves the file", name, (long long)i);
  if (f.status != RHCCQ_PNG_OK) return 0;
  CHECK(f.width >= 1 && f.height >= 1 && f.scan_bytes == (f.rowbytes + 1) * f.height && f.scan_bytes <= kReadMax, "%s: geometry", name);
  CHECK(f.n_idat >= 1 && f.first_idat >= 1 && f.first_idat + f.n_idat <= count, "%s: IDAT rows", name);
  if (f.colour_type == 3) CHECK(f.palette_rows >= 1 && f.plte_offset >= 0 && f.plte_offset + 3 * f.palette_rows <= n, "%s: PLTE leaves the file", name);
  if (f.trns_bytes) CHECK(f.trns_offset >= 0 && f.trns_offset + f.trns_bytes <= n, "%s: tRNS leaves the file", name);
  int64_t total = 0;
  for (int64_t i = 0; i < rows; ++i) {
    const bool idat = i >= f.first_idat && i < f.first_idat + f.n_idat;
    CHECK(idat ? t[i].dst == total : t[i].dst == -1, "%s: dst of chunk %lld", name, (long long)i);
    if (idat) total += t[i].length;
  }
  if (rows == count) CHECK(total == f.idat_bytes, "%s: IDAT bytes", name);
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
    int status = 0, detail = 0, has_scan = 0;
    in >> name >> status >> detail >> has_scan;
    const std::vector<uint8_t> file = slurp(dir + "/" + name);
    const int64_t n = (int64_t)file.size();
    rhccq_png_info f;
    std::vector<rhccq_segment> table((size_t)(n / 12 + 1));
    const int64_t count = png_parse(file.data(), n, &f, table.data(), (int64_t)table.size());
    CHECK(f.status == status && f.detail == detail, "%s: status %d detail %d, expected %d %d", name.c_str(), f.status, f.detail, status, detail);
    if (sound(f, table, count, n, name.c_str())) return 1;
    // every prefix, in a buffer of exactly that size (a read past it is the sanitizer's to see), and tables of 0, 1 and 2 rows
    for (int64_t m = 0; m <= n; m += (n > 4096 && m > 64 && m < n - 64 ? 61 : 1)) {   // (a long file: not every prefix in its middle)
      const std::vector<uint8_t> cut(file.begin(), file.begin() + m);
      rhccq_png_info g;
      std::vector<rhccq_segment> t2((size_t)(m / 12 + 1));
      const int64_t c2 = png_parse(cut.data(), m, &g, t2.data(), (int64_t)t2.size());
      if (sound(g, t2, c2, m, name.c_str())) return 1;
      if (m < n) CHECK(g.status != RHCCQ_PNG_OK || m >= n - 32, "%s: prefix %lld parsed as a whole file", name.c_str(), (long long)m);
      for (int64_t cap = 0; cap <= 2 && m % 7 == 0; ++cap) {
        std::vector<rhccq_segment> t3((size_t)cap);
        rhccq_png_info h;
        CHECK(png_parse(cut.data(), m, &h, cap ? t3.data() : nullptr, cap) == c2 && h.status == g.status && h.detail == g.detail, "%s: a small table changes the parse",
              name.c_str());
      }
    }
    if (has_scan) {
      CHECK(f.status == RHCCQ_PNG_OK, "%s: a scan for a refused file", name.c_str());
      const std::vector<uint8_t> scan = slurp(dir + "/" + name + ".scan"), want = slurp(dir + "/" + name + ".rgb");
      CHECK((int64_t)scan.size() == f.scan_bytes && (int64_t)want.size() == 3 * (int64_t)f.width * f.height, "%s: sizes of .scan / .rgb", name.c_str());
      std::vector<uint8_t> raw((size_t)(f.rowbytes * f.height)), rgb(want.size()), alpha(want.size() / 3), idx(want.size() / 3);
      CHECK(unfilter_serial(scan.data(), f.height, f.rowbytes, f.bpp, raw.data()) == 0, "%s: a bad filter row", name.c_str());
      expand_serial(raw.data(), f.height, f.width, f.colour_type, f.depth, f.colour_type == 3 ? file.data() + f.plte_offset : nullptr, f.palette_rows,
                    f.trns_bytes ? file.data() + f.trns_offset : nullptr, f.trns_bytes, rgb.data(), alpha.data(), idx.data());
      CHECK(rgb == want, "%s: pixels differ", name.c_str());
    }
    ++files;
  }
  CHECK(files > 0, "an empty manifest");
  std::printf("png_read_host ok %d\n", files);
  return 0;
}
