// The host side of the "wide" Lloyd path of rhccq_kmeans (k7_kmeans.hip, RHCCQ_OPT_KMEANS_WIDE_PAIRS / RHCCQ_OPT_KMEANS_CHUNK), as plain
// C++17: no HIP header, no device (tests/native/km_wide_host_test.cpp compiles it with g++).
//
// A wide problem runs its load, mean / tolerance and k-means++ in kmeans_kernel, which leaves the initial centres and a state record
// behind.  Its Lloyd iterations are then LAUNCHES on the context's stream: an E-step over tiles of points on many CUs, an M-step of one
// workgroup per problem.  A launch boundary is the only synchronisation between workgroups: no kernel waits for what another workgroup of
// the same launch writes, so a chain of launches cannot hang on a partner.  The kernels look at the problem's state record and return at
// once when there is nothing for them to do:
//
//   state            E-step launch                                   M-step launch
//   kRunning         labels, "changed" word, integer member sums     empty clusters, new centres, shifts, stop rules; n_iter + 1;
//                                                                    -> kDone (labels unchanged: strict), -> kFinalPending (the shifts
//                                                                    are within the tolerance, or n_iter reached the limit), else stays
//   kFinalPending    labels only, from the last centres              -> kDone (an E-step launch always lies between two M-step launches)
//   kDone            nothing                                         nothing
//
// The host enqueues chunks of C (E, M) pairs, reads the records back in one small copy behind each chunk, goes on while any problem is
// running and at the end issues ONE more E-step launch when a problem is still kFinalPending: a stop on the last iteration of a chunk.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rhccq_km_wide {

enum State : int32_t { kRunning = 0, kFinalPending = 1, kDone = 2 };

// one per wide problem, in the context's scratch; written by kmeans_kernel (mean, tolerance, state) and the two wide kernels
struct Record {
  double m0, m1, m2;      // the mean the Lloyd coordinates are centred on
  double tol;
  int32_t state;          // State
  int32_t changed;        // an E-step launch stores 1 when a label differs from the previous one; the M-step clears it
  int32_t n_iter, strict, relocated;
  int32_t reserved[3];
};
static_assert(sizeof(Record) == 64, "one record per 64-byte line");

// a tile of points of one wide problem: what one workgroup of an E-step launch works on
struct Tile {
  int32_t prob;           // problem index of the call
  int32_t rec;            // index of its record
  int32_t first;          // first point of the tile
  int32_t reserved;
};

// the one rule: the path supports k centres in LDS, and the problem has at least `wide_pairs` (point, centre) pairs.
// wide_pairs = 0: never; 1: every problem the path supports
inline bool takes_wide(int64_t n, int64_t k, int64_t wide_pairs, int64_t cent_lds) {
  return wide_pairs > 0 && n >= 1 && k >= 1 && k <= cent_lds && n * k >= wide_pairs;
}

// can a call whose largest problem has max_n points hold a wide problem at all (k <= n)?  Saves reading `desc` back when not
inline bool may_hold_wide(int64_t max_n, int64_t wide_pairs, int64_t cent_lds) {
  return max_n >= 1 && takes_wide(max_n, max_n < cent_lds ? max_n : cent_lds, wide_pairs, cent_lds);
}

// the wide problems of a call, ascending; desc = int32[n_prob][6] = {off, n, k, ...} of rhccq_kmeans
inline std::vector<int32_t> wide_problems(const int32_t* desc, int32_t n_prob, int64_t wide_pairs, int64_t cent_lds) {
  std::vector<int32_t> out;
  for (int32_t p = 0; p < n_prob; ++p)
    if (takes_wide(desc[6 * p + 1], desc[6 * p + 2], wide_pairs, cent_lds)) out.push_back(p);
  return out;
}

// tiles of `tile_points` points over all wide problems, problem after problem
inline std::vector<Tile> build_tiles(const int32_t* desc, const std::vector<int32_t>& wide, int32_t tile_points) {
  std::vector<Tile> out;
  for (size_t w = 0; w < wide.size(); ++w) {
    const int32_t n = desc[6 * wide[w] + 1];
    for (int32_t first = 0; first < n; first += tile_points) out.push_back(Tile{wide[w], (int32_t)w, first, 0});
  }
  return out;
}

inline bool problem_over(const Record& r) { return r.state == kDone; }

inline bool any_running(const Record* recs, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (recs[i].state == kRunning) return true;
  return false;
}

// how many (E, M) pairs to enqueue next, from the records as last read (before the first chunk: as kmeans_kernel leaves them, all
// running) and the pairs enqueued so far: 0 = the loop is over
inline int next_chunk(const Record* recs, size_t n, int chunk, int max_iter, int enqueued) {
  if (enqueued >= max_iter || !any_running(recs, n)) return 0;
  if (chunk < 1) chunk = 1;
  return chunk < max_iter - enqueued ? chunk : max_iter - enqueued;
}

// behind the loop: does a problem still wait for its final labelling (one more E-step launch)?
inline bool final_pending(const Record* recs, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (recs[i].state == kFinalPending) return true;
  return false;
}

// The whole loop.  estep() / mstep(): enqueue one launch; read_back(Record*): fill the records from the device behind everything
// enqueued so far.  Each returns 0 or an error code, which ends the loop and is returned.  `recs` comes in as kmeans_kernel leaves the
// records (all running) and goes out as last read.  *pairs = the (E, M) pairs enqueued.
template <typename EStep, typename MStep, typename ReadBack>
int drive(std::vector<Record>& recs, int chunk, int max_iter, EStep&& estep, MStep&& mstep, ReadBack&& read_back, int* pairs = nullptr) {
  int enqueued = 0, rc = 0;
  for (int c; (c = next_chunk(recs.data(), recs.size(), chunk, max_iter, enqueued)) > 0;) {
    for (int i = 0; i < c; ++i) {
      if ((rc = estep()) != 0) return rc;
      if ((rc = mstep()) != 0) return rc;
    }
    enqueued += c;
    if (pairs) *pairs = enqueued;
    if ((rc = read_back(recs.data())) != 0) return rc;
  }
  if (pairs) *pairs = enqueued;
  if (final_pending(recs.data(), recs.size())) rc = estep();
  return rc;
}

}  // namespace rhccq_km_wide
