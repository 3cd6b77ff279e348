// What the host decides while it drives sklearn's MiniBatchKMeans.fit for 1 .. 32 problems that share their launches (mbk_fit and
// frame_chains in encode_frame.hip), as plain C++17: no HIP header, no device (tests/native/mbk_fit_host_test.cpp compiles it with g++
// and the host sanitizers).  A lone fit is a batch of one: every rule below is stated once, per problem, and a problem gets in a batch
// the decisions it gets alone.
//
//   slots     the names of the double[16] state of a problem (include/rhccq.h, rhccq_mbk_steps) and a view that reads them
//   Problem   what follows from (n, k) alone, and from where the MT19937 replay left the stream (mt_replay.h does the replay)
//   Totals    the problems of a batch laid out into rhccq_mbk_problem, with the sums the set-up allocates by
//   Plan      between two launches of steps: who runs, on which schedule, for how many steps, with how many MT19937 words
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/rhccq.h"

namespace rhccq_fit {

constexpr int64_t kBatchSize = 1000;                   // MiniBatchKMeans(batch_size=1000) (clustering.py:211-218)
constexpr int64_t kMaxIter = 100;                      // sklearn's max_iter: the fit ends after 100 n / batch steps at the latest
constexpr int64_t kReassignEvery = 10;                 // sklearn _random_reassign: every 10 k samples
constexpr int64_t kTileCentres = 512;                  // centres per LDS tile of the tiled E-step
constexpr int64_t kSplitWorkgroups = 1536;             // the E-step splits a point over 1, 2, 4 or 8 threads until tiles * 2 * split reaches this
constexpr int64_t kGridFromK = 200000;                 // the largest problem has this many centres: the grid E-step
constexpr int64_t kOverlapFromK = 1024;                // a problem with fewer centres never takes the overlapped schedule
constexpr int64_t kWordsPerStep = 16384;               // kWordsMargin of mbk_update_kernel: the most MT19937 words a step consumes
constexpr int64_t kWordsPerOverlappedStep = 4200;      // the same for a step that cannot reassign 500 centres (no centre without weight)
constexpr int kFirstLook = 16;                         // most problems converge within a dozen steps: look early once
constexpr int kChunk = 64;                             // steps per launch sequence afterwards
constexpr int kMaxProblems = 32;                       // one bit of a mask each

// ---- the state of a problem ------------------------------------------------------------------------------------------------------------
enum Slot {
  kEwa = 0, kEwaMin = 1, kNoImprovement = 2,
  kSince = 3,                                          // samples since the last reassignment
  kStop = 4,                                           // 0 running, 1 converged, 2 out of steps, 3 .. 5 errors (stop_error)
  kStepsDone = 5, kHaveEwa = 6, kHaveMin = 7,
  kZeroWeight = 8,                                     // centres without weight
  kCursor = 9,                                         // MT19937 words consumed so far
  kFirstDrawn = 10,
  kStopAt = 11,                                        // steps done when it stopped, 0 while running
  kSinceOdd = 12, kZeroWeightOdd = 13, kCursorOdd = 14,   // the twins an odd step reads (a step reads its parity's slots and writes the other's)
  kStateDoubles = 16
};

struct StateView {
  const double* s;
  int64_t since(int64_t step) const { return (int64_t)s[(step & 1) ? kSinceOdd : kSince]; }
  int64_t zero_weight(int64_t step) const { return (int64_t)s[(step & 1) ? kZeroWeightOdd : kZeroWeight]; }
  int64_t cursor() const { return (int64_t)std::max(s[kCursor], s[kCursorOdd]); }   // of the later step: the cursor only grows
  int64_t steps_done() const { return (int64_t)s[kStepsDone]; }
  int stop_code() const { return (int)s[kStop]; }
  int64_t stop_at() const { return (int64_t)s[kStopAt]; }
};

// the state a fit starts from: every centre without weight, the stream behind the k-means++ uniforms
inline void init_state(double* s, int64_t k, int64_t cursor0) {
  std::fill(s, s + kStateDoubles, 0.0);
  s[kZeroWeight] = (double)k;
  s[kCursor] = (double)cursor0;
}

// the stop codes that are errors (all RHCCQ_E_LIMIT); NULL: the problem runs, or has ended as a fit ends
inline const char* stop_error(int code) {
  switch (code) {
    case 3: return "mini-batch steps ran past the end of the MT19937 word table (internal sizing error)";
    case 4: return "the sharded k-means++ chain gave up waiting for a partner workgroup";
    case 5: return "the overlapped mini-batch schedule and the device state disagree about a reassignment";
    default: return nullptr;
  }
}

// ---- one problem -----------------------------------------------------------------------------------------------------------------------
struct Problem {
  int64_t n = 0, k = 0;
  int64_t batch = 0;                                   // min(1000, n)
  int64_t limit = 0;                                   // steps at most
  int64_t init_size = 0;                               // sklearn _init_centroids: 3 batch, 3 k if that is below k, n at most
  int T = 0;                                           // n_local_trials of kmeans_plusplus: 2 + floor(ln k)
  int64_t n_uniforms = 0;                              // uniforms of the chain
  // where the replay of the draws ahead of the chain (validation sample, init sample, first centre) left the stream
  int64_t pos = 0;                                     // raw MT19937 word of the first k-means++ uniform
  int64_t cursor0 = 0;                                 // stream position behind the k-means++ uniforms
  int32_t first = 0;                                   // first centre (position in the init sample)
  int64_t chain_words() const { return pos + 2 * n_uniforms; }   // the word table the chain's uniforms need
};

inline Problem problem(int64_t n, int64_t k) {
  Problem c;
  c.n = n;
  c.k = k;
  c.batch = std::min(kBatchSize, n);
  c.limit = c.batch > 0 ? (kMaxIter * n) / c.batch : 0;
  c.init_size = 3 * c.batch;
  if (c.init_size < k) c.init_size = 3 * k;
  c.init_size = std::min(c.init_size, n);
  c.T = 2 + (int)std::log((double)k);
  c.n_uniforms = std::max<int64_t>((k - 1) * c.T, 1);
  return c;
}

inline void chain_at(Problem& c, int64_t pos, int32_t first) {
  c.pos = pos;
  c.first = first;
  c.cursor0 = pos + 2 * (c.k - 1) * c.T;
}

// ---- a batch laid out: problem after problem in centres / weights, init samples and uniforms ---------------------------------------------
struct Totals {
  int64_t ktot = 0, itot = 0, utot = 0;
  int64_t words = 1;                                   // MT19937 words the chains' uniforms need
  int64_t k_max = 0, tiles = 0;
  // q.off / n / k are the caller's; the rest of q is the next place in the batch
  void add(rhccq_mbk_problem& q, const Problem& c) {
    q.koff = ktot; q.init_off = itot; q.init_n = c.init_size; q.rand_off = utot; q.first = c.first; q.T = c.T;
    ktot += c.k;
    itot += c.init_size;
    utot += c.n_uniforms;
    words = std::max(words, c.chain_words());
    k_max = std::max(k_max, c.k);
    tiles += (c.k + kTileCentres - 1) / kTileCentres;
  }
  bool tiled() const { return k_max < kGridFromK; }    // (same results either way)
  int split() const {
    for (int sp : {1, 2, 4}) if (tiles * 2 * sp >= kSplitWorkgroups) return sp;
    return 8;
  }
};

// ---- the step loop's decisions ---------------------------------------------------------------------------------------------------------
struct Chunk {
  int ns = 0;                                          // steps of this launch sequence
  uint32_t fast_mask = 0u;                             // problems on the overlapped schedule
  uint32_t classic_mask = 0u;                          // problems on the classic sequence
  uint32_t entered = 0u;                               // problems of fast_mask that are there from this chunk on
  bool no_reassign = false;                            // RHCCQ_STEPS_NO_REASSIGN for the classic problems: none of them reassigns in these steps
  int64_t need = 0;                                    // MT19937 words the device table must hold
  bool any() const { return (fast_mask | classic_mask) != 0u; }
};

// All problems share the launch index `step`.  A classic problem's snapshot is always the one of `step` (the driver waits for it); an
// overlapped problem's may be chunks old: its word horizon counts the steps launched since.  A problem never leaves the overlapped
// schedule: sklearn's update takes no weight away.
struct Plan {
  std::vector<Problem> c;
  bool tiled;
  std::vector<double> st;                              // the latest state snapshot, [N][16]
  std::vector<char> running, fast;
  std::vector<int64_t> since, overlapped_from;         // overlapped problems: samples since the last reassignment as `step` sees it; entry step (-1: never)
  std::vector<int32_t> carry;                          // rhccq_mbk_steps_batch's, 0 at entry

  Plan(const std::vector<Problem>& cs, bool tiled_)
      : c(cs), tiled(tiled_), st(cs.size() * kStateDoubles), running(cs.size(), 1), fast(cs.size(), 0), since(cs.size(), 0),
        overlapped_from(cs.size(), -1), carry(cs.size(), 0) {
    for (size_t p = 0; p < c.size(); ++p) init_state(&st[p * kStateDoubles], c[p].k, c[p].cursor0);
  }
  int size() const { return (int)c.size(); }
  StateView view(int p) const { return StateView{&st[(size_t)p * kStateDoubles]}; }

  // a state snapshot of all problems
  void take(const double* snap) {
    std::memcpy(st.data(), snap, st.size() * sizeof(double));
    for (int p = 0; p < size(); ++p) {
      const StateView s = view(p);
      running[(size_t)p] = s.stop_code() < 3 && s.stop_at() == 0 && s.steps_done() < c[(size_t)p].limit;
    }
  }
  // the first stop code among the problems that is an error
  const char* error() const {
    for (int p = 0; p < size(); ++p)
      if (const char* e = stop_error(view(p).stop_code())) return e;
    return nullptr;
  }

  // the launch sequence that starts at `step` (nothing to launch: !any())
  Chunk next(int64_t step) {
    Chunk ch;
    int64_t left = 0;
    for (int p = 0; p < size(); ++p) {
      if (!running[(size_t)p]) continue;
      const Problem& q = c[(size_t)p];
      // all centres carry weight: from here on the next E-step starts beside the update
      if (!fast[(size_t)p] && step > 0 && tiled && q.k >= kOverlapFromK && view(p).zero_weight(step) == 0) {
        fast[(size_t)p] = 1;
        overlapped_from[(size_t)p] = step;
        since[(size_t)p] = view(p).since(step);
        carry[(size_t)p] = 0;
        ch.entered |= 1u << p;
      }
      left = std::max(left, q.limit - step);
    }
    ch.ns = (int)std::min<int64_t>(step ? kChunk : kFirstLook, left);
    if (ch.ns <= 0) return Chunk();
    bool quiet = true;
    for (int p = 0; p < size(); ++p) {
      if (!running[(size_t)p]) continue;
      const Problem& q = c[(size_t)p];
      const StateView s = view(p);
      if (fast[(size_t)p]) {
        ch.fast_mask |= 1u << p;
        ch.need = std::max(ch.need, s.cursor() + (step - s.steps_done() + ch.ns + 4) * kWordsPerOverlappedStep + 8 * kWordsPerStep);
      } else {
        ch.classic_mask |= 1u << p;
        ch.need = std::max(ch.need, s.cursor() + (ch.ns + 3) * kWordsPerStep);
        quiet = quiet && s.zero_weight(step) == 0 && s.since(step) + ch.ns * q.batch < kReassignEvery * q.k;
      }
    }
    ch.no_reassign = ch.classic_mask != 0u && quiet;
    return ch;
  }

  // behind the launches of `ch`: the overlapped schedule's own arithmetic (sklearn _random_reassign)
  void advance(const Chunk& ch) {
    for (int p = 0; p < size(); ++p) {
      if (!((ch.fast_mask >> p) & 1u)) continue;
      for (int i = 0; i < ch.ns; ++i) {
        since[(size_t)p] += c[(size_t)p].batch;
        if (since[(size_t)p] >= kReassignEvery * c[(size_t)p].k) since[(size_t)p] = 0;
      }
    }
  }
};

}  // namespace rhccq_fit
