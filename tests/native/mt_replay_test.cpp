// csrc/mt_replay.h without a device: the generator's words for seed 42 against constants taken from numpy's RandomState(42), snapshots
// of the word table across a growth, and mbk_draws against the draws made one by one.  Plain C++17 (tests/test_mt_replay_cpu.py builds
// it with g++ and the host sanitizers).
#include <cstdio>
#include <cstdlib>

#include "mt_replay.h"

#define CHECK(cond)                                                          \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

int main() {
  using rhccq_mt::Words;
  Words& mt = Words::get();

  // np.random.RandomState(42).randint(0, 1 << 32, size, dtype=np.uint32): words 0 .. 7, both sides of the first refill of the key, and
  // both sides of the table's first size
  const uint32_t first8[8] = {0x5fe1dc66u, 0xcbea3db3u, 0xf362035cu, 0x2ef5950eu, 0xbb63f46au, 0xc799d447u, 0x9941aebcu, 0x98cb2c14u};
  const auto small = mt.host(8);
  CHECK(small->size() == (size_t)1 << 20);                // the first table
  for (int i = 0; i < 8; ++i) CHECK((*small)[(size_t)i] == first8[i]);
  CHECK((*small)[623] == 0x40386559u && (*small)[624] == 0x067d62e4u);
  CHECK((*small)[((size_t)1 << 20) - 1] == 0x83161c9bu);
  // random_sample() is ((a >> 5) 2^26 + (b >> 6)) / 2^53 of two words
  CHECK(mt.dbl(0) == ((double)(first8[0] >> 5) * 67108864.0 + (double)(first8[1] >> 6)) / 9007199254740992.0);
  CHECK(mt.dbl(3) == ((double)(first8[3] >> 5) * 67108864.0 + (double)(first8[4] >> 6)) / 9007199254740992.0);

  // growth: a new table behind the snapshot, which stays what it was (the sanitizer sees a freed or moved one)
  const uint32_t* small_data = small->data();
  const auto grown = mt.host(((int64_t)1 << 20) + 8);
  CHECK(grown->size() == (size_t)2 << 20 && grown.get() != small.get());
  CHECK(small->size() == (size_t)1 << 20 && small->data() == small_data);
  for (size_t i = 0; i < small->size(); ++i) CHECK((*small)[i] == (*grown)[i]);
  CHECK((*grown)[(size_t)1 << 20] == 0xec4d906fu && (*grown)[((size_t)1 << 20) + 7] == 0x41c4165eu);
  CHECK(mt.host(100).get() == grown.get());               // no growth: the same table

  // randint over a table that ends early, bad arguments, the one-value range
  int32_t out[4];
  CHECK(rhccq_mt::randint(grown->data(), 2, 0, 1000, 4, out) == -1);
  CHECK(rhccq_mt::randint(nullptr, 8, 0, 5, 4, out) == -2 && rhccq_mt::randint(grown->data(), 8, 0, 0, 4, out) == -2);
  CHECK(mt.randint(5, 1, 4, out) == 0 && out[0] == 0 && out[3] == 0);
  // mask 7 for n = 5: the first words & 7 are 6 3 4 6 2 7 4 4 -> 3 4 2 4 after 7 words
  CHECK(mt.randint(0, 5, 4, out) == 7 && out[0] == 3 && out[1] == 4 && out[2] == 2 && out[3] == 4);

  // mbk_draws = problem(n, k) + the validation draw (position only), the init sample, the first centre's uniform, chain_at
  const int64_t cases[][2] = {{1500000, 30000}, {10000, 20}, {999, 5}, {2500, 1000}, {65537, 40}, {3, 2}, {12000, 130}, {1, 1}};
  for (const auto& nk : cases) {
    const int64_t n = nk[0], k = nk[1];
    const rhccq_mt::MbkDraws d = rhccq_mt::mbk_draws(n, k);
    rhccq_fit::Problem want = rhccq_fit::problem(n, k);
    CHECK((int64_t)d.init_idx.size() == want.init_size);
    std::vector<int32_t> idx((size_t)want.init_size);
    int64_t pos = mt.randint(0, n, want.init_size, nullptr);
    if (want.init_size < n) pos += mt.randint(pos, n, want.init_size, idx.data());
    else for (int64_t i = 0; i < n; ++i) idx[(size_t)i] = (int32_t)i;
    rhccq_fit::chain_at(want, pos + 2, rhccq_mt::first_centre_index(want.init_size, mt.dbl(pos)));
    CHECK(d.init_idx == idx);
    CHECK(d.c.n == n && d.c.k == k && d.c.batch == want.batch && d.c.limit == want.limit && d.c.init_size == want.init_size);
    CHECK(d.c.T == want.T && d.c.n_uniforms == want.n_uniforms && d.c.pos == want.pos && d.c.cursor0 == want.cursor0 && d.c.first == want.first);
    CHECK(d.c.cursor0 == d.c.pos + 2 * (k - 1) * d.c.T && d.c.first >= 0 && d.c.first < d.c.init_size);
    for (int32_t v : d.init_idx) CHECK(v >= 0 && v < n);
  }
  std::puts("mt_replay ok");
  return 0;
}
