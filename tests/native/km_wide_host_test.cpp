// Host-only checks of csrc/km_wide_host.h: which problems of a rhccq_kmeans call take the wide Lloyd path, how their points are cut into
// tiles, and the loop that enqueues (E, M) launches in chunks and reads the state records back.  The two kernels are scripted by the
// state table of the header; no device.  tests/test_km_wide_host_cpu.py compiles this with g++ -std=c++17 and runs it as a child process;
// exit status 0 = every check held, otherwise the line that failed is on stderr.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "km_wide_host.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

using namespace rhccq_km_wide;

enum Rule { kStrict, kTol, kNever };                    // how a scripted problem stops: unchanged labels, the tolerance, or not at all

// the device side of the header's state table: every launch acts on the device's records, the host sees them only through read_back
struct Device {
  struct Prob { int stop_iter; Rule rule; };
  std::vector<Prob> probs;
  std::vector<Record> recs;
  int max_iter;
  std::vector<int> e_work, finals, final_at_iter;        // E-steps that did an iteration's work; final labellings, and n_iter at the last of them
  int e_launches = 0, m_launches = 0, reads = 0;
  bool last_was_e = false, order_ok = true;
  Device(std::vector<Prob> p, int mi) : probs(p), recs(p.size()), max_iter(mi), e_work(p.size(), 0), finals(p.size(), 0), final_at_iter(p.size(), -1) {
    for (auto& r : recs) r = Record{};
  }
  int estep() {
    ++e_launches;
    last_was_e = true;
    for (size_t i = 0; i < recs.size(); ++i) {
      if (recs[i].state == kRunning) { ++e_work[i]; recs[i].changed = 1; }
      else if (recs[i].state == kFinalPending) { ++finals[i]; final_at_iter[i] = recs[i].n_iter; }
    }
    return 0;
  }
  int mstep() {
    ++m_launches;
    if (!last_was_e) order_ok = false;                   // an E-step launch lies between any two M-step launches
    last_was_e = false;
    for (size_t i = 0; i < recs.size(); ++i) {
      Record& r = recs[i];
      if (r.state == kDone) continue;
      if (r.state == kFinalPending) { r.state = kDone; continue; }
      if (!r.changed) order_ok = false;
      r.changed = 0;
      ++r.n_iter;
      const bool stop = r.n_iter == probs[i].stop_iter && probs[i].rule != kNever;
      if (stop && probs[i].rule == kStrict) { r.strict = 1; r.state = kDone; }
      else if (stop || r.n_iter >= max_iter) r.state = kFinalPending;
    }
    return 0;
  }
  int read_back(Record* out) {
    ++reads;
    for (size_t i = 0; i < recs.size(); ++i) out[i] = recs[i];
    return 0;
  }
  int run(int chunk, int* pairs) {
    std::vector<Record> host(recs.size(), Record{});
    return drive(host, chunk, max_iter, [&] { return estep(); }, [&] { return mstep(); }, [&](Record* o) { return read_back(o); }, pairs);
  }
  // every problem got exactly the iterations of its script, and its final labelling once, behind its last iteration, iff it did not stop strictly
  bool results_ok() const {
    for (size_t i = 0; i < probs.size(); ++i) {
      const int want = probs[i].rule == kNever ? max_iter : probs[i].stop_iter;
      const bool strict = probs[i].rule == kStrict;
      if (e_work[i] != want || recs[i].n_iter != want || recs[i].strict != (strict ? 1 : 0)) return false;
      if (finals[i] != (strict ? 0 : 1)) return false;
      if (!strict && final_at_iter[i] != want) return false;
    }
    return order_ok;
  }
};

// (a) the rule and the tiles
static int rule_and_tiles() {
  CHECK(!takes_wide(10240, 1024, 0, 1024));              // 0 = never
  CHECK(takes_wide(1, 1, 1, 1024) && takes_wide(10241, 1024, 1, 1024) && !takes_wide(7000, 1025, 1, 1024));
  CHECK(!takes_wide(0, 0, 1, 1024) && !takes_wide(5, 0, 1, 1024));
  CHECK(takes_wide(3883, 389, 3883 * 389, 1024) && !takes_wide(3883, 389, 3883 * 389 + 1, 1024));
  CHECK(takes_wide(1 << 24, 1024, 1ll << 30, 1024));     // no 32-bit overflow in n x k
  CHECK(may_hold_wide(3883, 1, 1024) && !may_hold_wide(3883, 0, 1024) && !may_hold_wide(0, 1, 1024));
  CHECK(may_hold_wide(100, 10000, 1024) && !may_hold_wide(99, 10000, 1024));          // k <= n
  CHECK(may_hold_wide(5000, 5000 * 1024, 1024) && !may_hold_wide(5000, 5000 * 1024 + 1, 1024));
  // desc rows {off, n, k, rand_off, first, T}
  const int32_t desc[] = {0, 50, 20, 0, 0, 4,  50, 7000, 1025, 0, 0, 8,  7050, 129, 3, 0, 0, 3,  7179, 1, 1, 0, 0, 2,  7180, 64, 64, 0, 0, 6};
  CHECK(wide_problems(desc, 5, 0, 1024).empty());
  CHECK((wide_problems(desc, 5, 1, 1024) == std::vector<int32_t>{0, 2, 3, 4}));
  CHECK((wide_problems(desc, 5, 1000, 1024) == std::vector<int32_t>{0, 4}));
  const std::vector<int32_t> wide = wide_problems(desc, 5, 1, 1024);
  const std::vector<Tile> t = build_tiles(desc, wide, 64);
  CHECK(t.size() == 1 + 3 + 1 + 1);                      // 50, 129 (64 + 64 + 1), 1, 64 points
  CHECK(t[0].prob == 0 && t[0].rec == 0 && t[0].first == 0);
  CHECK(t[1].prob == 2 && t[1].rec == 1 && t[1].first == 0 && t[3].prob == 2 && t[3].first == 128);
  CHECK(t[4].prob == 3 && t[4].rec == 2 && t[5].prob == 4 && t[5].rec == 3 && t[5].first == 0);
  CHECK(build_tiles(desc, {}, 64).empty());
  return 0;
}

// (b) several problems ending in different chunks, by either rule, two of them on a chunk's last iteration
static int different_chunks() {
  Device d({{3, kStrict}, {4, kTol}, {9, kTol}, {8, kStrict}, {1, kTol}, {12, kTol}}, 300);
  int pairs = 0;
  CHECK(d.run(4, &pairs) == 0);
  CHECK(d.results_ok());
  CHECK(pairs == 12 && d.reads == 3 && d.m_launches == 12);
  CHECK(d.e_launches == 13);                             // the stop of the last problem on the last iteration of the last chunk: one more E-step
  // the tolerance stop on the last iteration of the FIRST chunk was labelled by the first E-step of the second chunk, not by an extra launch
  CHECK(d.finals[1] == 1);
  return 0;
}

// (c) a lone problem that stops on a chunk's last iteration: by the tolerance it still gets its final labelling, strictly it gets none
static int stop_on_chunk_end() {
  for (int chunk : {1, 7, 11}) {
    Device t({{chunk * 2, kTol}}, 300);
    int pairs = 0;
    CHECK(t.run(chunk, &pairs) == 0 && t.results_ok());
    CHECK(pairs == 2 * chunk && t.reads == 2 && t.e_launches == 2 * chunk + 1 && t.m_launches == 2 * chunk);
    Device s({{chunk * 2, kStrict}}, 300);
    CHECK(s.run(chunk, &pairs) == 0 && s.results_ok());
    CHECK(pairs == 2 * chunk && s.reads == 2 && s.e_launches == 2 * chunk && s.m_launches == 2 * chunk);
    // one behind the boundary: a whole further chunk is enqueued, its launches behind the end return at once
    Device b({{chunk * 2 + 1, kTol}}, 300);
    CHECK(b.run(chunk, &pairs) == 0 && b.results_ok());
    CHECK(pairs == 3 * chunk && b.reads == 3);
    CHECK(b.e_launches == (chunk == 1 ? 4 : 3 * chunk)); // chunk 1: iteration, read, ... the final labelling is the extra launch
    // one before the boundary: the final labelling is the chunk's last E-step
    if (chunk > 1) {
      Device a({{chunk * 2 - 1, kTol}}, 300);
      CHECK(a.run(chunk, &pairs) == 0 && a.results_ok());
      CHECK(pairs == 2 * chunk && a.e_launches == 2 * chunk);
    }
  }
  return 0;
}

// (d) the iteration limit: a problem that never stops runs max_iter iterations and gets its final labelling; nothing is enqueued past it
static int iteration_limit() {
  for (int chunk : {1, 7, 64, 300}) {
    Device d({{0, kNever}, {5, kStrict}}, 300);
    int pairs = 0;
    CHECK(d.run(chunk, &pairs) == 0 && d.results_ok());
    CHECK(pairs == 300 && d.m_launches == 300 && d.e_launches == 301);
    CHECK(d.reads == (300 + chunk - 1) / chunk);
  }
  // a stop on the very last allowed iteration, by either rule
  Device s({{300, kStrict}}, 300), t({{300, kTol}}, 300);
  int pairs = 0;
  CHECK(s.run(16, &pairs) == 0 && s.results_ok() && s.e_launches == 300);
  CHECK(t.run(16, &pairs) == 0 && t.results_ok() && t.e_launches == 301);
  // a chunk length below 1 counts as 1
  Device z({{3, kTol}}, 300);
  CHECK(z.run(0, &pairs) == 0 && z.results_ok() && pairs == 3);
  return 0;
}

// (e) a call with no wide problem: nothing is enqueued, nothing is read
static int no_wide_problem() {
  Device d({}, 300);
  int pairs = -1;
  CHECK(d.run(16, &pairs) == 0);
  CHECK(pairs == 0 && d.e_launches == 0 && d.m_launches == 0 && d.reads == 0);
  CHECK(next_chunk(nullptr, 0, 16, 300, 0) == 0 && !final_pending(nullptr, 0) && !any_running(nullptr, 0));
  return 0;
}

// (f) an error of a launch or of the copy ends the loop and is handed on
static int errors_end_the_loop() {
  std::vector<Record> host(1, Record{});
  int e = 0, m = 0;
  CHECK(drive(host, 4, 300, [&] { return ++e == 3 ? -2 : 0; }, [&] { ++m; return 0; }, [&](Record*) { return 0; }) == -2);
  CHECK(e == 3 && m == 2);
  e = m = 0;
  CHECK(drive(host, 4, 300, [&] { ++e; return 0; }, [&] { ++m; return 0; }, [&](Record*) { return -2; }) == -2);
  CHECK(e == 4 && m == 4);
  Record r{};
  r.state = kDone;
  CHECK(problem_over(r));
  r.state = kFinalPending;
  CHECK(!problem_over(r));
  return 0;
}

int main() {
  if (rule_and_tiles() || different_chunks() || stop_on_chunk_end() || iteration_limit() || no_wide_problem() || errors_end_the_loop()) return 1;
  printf("km_wide_host ok\n");
  return 0;
}
