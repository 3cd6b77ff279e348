// numpy's legacy RandomState(42), replayed from its raw MT19937 words, and the draws sklearn's MiniBatchKMeans.fit makes ahead of its
// k-means++ chain, as plain C++17: no HIP header, no device (tests/native/mt_replay_test.cpp compiles it with g++ and the host sanitizers).
// Every k-means fit of the reference restarts from random_state=42 (clustering.py:211-218, 751-752), so all of its random draws are
// functions of ONE fixed sequence of 32-bit outputs.  This header is the only replay of it: rhccq_encode_frame calls it directly, the
// Python host through rhccq_mbk_draws / rhccq_mt_words / rhccq_mt_double_host / rhccq_first_centre_index (api.hip, which also keeps
// the one word table per device).
//
//   randint            RandomState.randint(0, n, size): masked rejection, candidates word & (2^b - 1 >= n - 1), one word each, kept
//                      when <= n - 1 (_bounded_integers.pyx, legacy path for ranges below 2^32)
//   Words              the generator and its growing host table; randint and random_sample() at a word position
//   first_centre_index RandomState.choice(n, p = ones / n) from its one uniform
//   mbk_draws          validation sample, init sample, first centre of a fit: rhccq_fit::Problem complete, and the init indices
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "mbk_fit_host.h"

namespace rhccq_mt {

// randint(0, n, size) from words[pos ..) of a table of n_words.  out: int32[size], or NULL when only the stream position matters
// (sklearn's validation draw).  Returns the words consumed, -1 when the table ends first, -2 for a bad argument.
inline int64_t randint(const uint32_t* words, int64_t n_words, int64_t pos, int64_t n, int64_t size, int32_t* out) {
  if (!words || pos < 0 || n <= 0 || n > 0x7fffffffll || size < 0 || n_words < 0) return -2;
  if (size == 0) return 0;
  const uint32_t rng = (uint32_t)(n - 1);
  if (rng == 0u) {                                         // numpy draws nothing for a one-value range
    if (out) memset(out, 0, sizeof(int32_t) * (size_t)size);
    return 0;
  }
  uint32_t mask = rng;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  int64_t got = 0;
  if (out) {
    for (int64_t i = pos; i < n_words; ++i) {
      const uint32_t v = words[i] & mask;
      out[got] = (int32_t)v;                               // (kept only when accepted: `got` moves on)
      got += v <= rng;
      if (got == size) return i + 1 - pos;
    }
  } else {
    for (int64_t i = pos; i < n_words; ++i) {
      got += (words[i] & mask) <= rng;
      if (got == size) return i + 1 - pos;
    }
  }
  return -1;
}

// MT19937(seed 42) and its outputs so far, one per process.  Safe from several threads: the draws of a frame's problems run side by side.
class Words {
 public:
  static Words& get() {
    static Words t;
    return t;
  }
  // raw words [0, n) (snapshot: stays valid while the table grows behind it)
  std::shared_ptr<const std::vector<uint32_t>> host(int64_t n) {
    std::lock_guard<std::mutex> g(mu_);
    if ((int64_t)words_->size() < n) {
      const size_t have = words_->size();
      const size_t want = std::max<size_t>({(size_t)n, 2 * have, (size_t)1 << 20});
      auto nw = std::make_shared<std::vector<uint32_t>>(*words_);
      nw->resize(want);
      for (size_t i = have; i < want; ++i) (*nw)[i] = next();
      words_ = nw;
    }
    return words_;
  }
  // randint(0, n, size) at raw word `pos`, 1 <= n < 2^31: words consumed (out may be NULL: stream position only)
  int64_t randint(int64_t pos, int64_t n, int64_t size, int32_t* out) {
    if (n <= 1) {
      if (out) std::fill(out, out + size, 0);
      return 0;                                            // numpy draws nothing for a one-value range
    }
    int bits = 0;
    while (((int64_t)1 << bits) < n) ++bits;
    int64_t win = (int64_t)((double)size / ((double)n / (double)((int64_t)1 << bits)) * 1.05) + 256;
    while (true) {
      auto w = host(pos + win);
      const int64_t used = rhccq_mt::randint(w->data(), (int64_t)w->size(), pos, n, size, out);
      if (used != -1) return used;
      win = 2 * win + 1024;
    }
  }
  // random_sample() at raw word `pos` (two words)
  double dbl(int64_t pos) {
    auto w = host(pos + 2);
    return ((double)((*w)[pos] >> 5) * 67108864.0 + (double)((*w)[pos + 1] >> 6)) / 9007199254740992.0;
  }

 private:
  Words() : words_(std::make_shared<std::vector<uint32_t>>()) {
    uint32_t seed = 42u;
    for (int i = 0; i < 624; ++i) {
      key_[i] = seed;
      seed = 1812433253u * (seed ^ (seed >> 30)) + (uint32_t)i + 1u;
    }
    pos_ = 624;
  }
  uint32_t next() {
    if (pos_ == 624) {
      uint32_t* k = key_;
      int i;
      for (i = 0; i < 624 - 397; ++i) {
        const uint32_t y = (k[i] & 0x80000000u) | (k[i + 1] & 0x7fffffffu);
        k[i] = k[i + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      for (; i < 623; ++i) {
        const uint32_t y = (k[i] & 0x80000000u) | (k[i + 1] & 0x7fffffffu);
        k[i] = k[i + (397 - 624)] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      const uint32_t y = (k[623] & 0x80000000u) | (k[0] & 0x7fffffffu);
      k[623] = k[396] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      pos_ = 0;
    }
    uint32_t y = key_[pos_++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  std::mutex mu_;
  std::shared_ptr<std::vector<uint32_t>> words_;
  uint32_t key_[624];
  int pos_;
};

// RandomState.choice(n, p = ones / n): searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right') -- numpy's cumsum adds sequentially
inline int32_t first_centre_index(int64_t n, double u) {
  const double p = 1.0 / (double)n;
  std::vector<double> cdf((size_t)n);
  double acc = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    acc = acc + p;
    cdf[(size_t)i] = acc;
  }
  const double last = cdf[(size_t)n - 1];
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[(size_t)mid] / last <= u) lo = mid + 1;
    else hi = mid;
  }
  return (int32_t)std::min(lo, n - 1);
}

// The draws of one fit ahead of its k-means++ chain (sklearn _init_centroids with init_size, then kmeans_plusplus), 1 <= k <= n < 2^31.
// init_idx: int32[rhccq_fit::problem(n, k).init_size], the init sample in draw order
inline rhccq_fit::Problem mbk_draws(int64_t n, int64_t k, int32_t* init_idx) {
  Words& mt = Words::get();
  rhccq_fit::Problem c = rhccq_fit::problem(n, k);
  int64_t pos = 0;
  pos += mt.randint(pos, n, c.init_size, nullptr);                       // validation_indices: stream position only
  if (c.init_size < n) pos += mt.randint(pos, n, c.init_size, init_idx);
  else for (int64_t i = 0; i < n; ++i) init_idx[(size_t)i] = (int32_t)i;
  rhccq_fit::chain_at(c, pos + 2, first_centre_index(c.init_size, mt.dbl(pos)));
  return c;
}

struct MbkDraws {
  rhccq_fit::Problem c;
  std::vector<int32_t> init_idx;
};

inline MbkDraws mbk_draws(int64_t n, int64_t k) {
  MbkDraws d;
  d.init_idx.resize((size_t)rhccq_fit::problem(n, k).init_size);
  d.c = mbk_draws(n, k, d.init_idx.data());
  return d;
}

}  // namespace rhccq_mt
