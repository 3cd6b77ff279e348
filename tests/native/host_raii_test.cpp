// Host-only checks of csrc/host_raii.h's first section (ThreadGroup, run_lanes, Err): no HIP header, no device.  tests/test_host_raii_cpu.py
// compiles this with g++ -std=c++17 -pthread and runs it as a child process; exit status 0 = every check held, otherwise the line that failed
// is on stderr (std::terminate, which an unjoined thread would cause, ends the process with SIGABRT).
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <set>
#include <stdexcept>
#include <thread>

#include "host_raii.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

static void no_failure(size_t) {}

// (a) four bodies, each exactly once, on four distinct threads that are alive at the same time: every body waits (5 s at most: a guard
// against a hang, not a measurement) until all four have started, which bodies run one after the other on one thread never see
static int one_thread_per_index() {
  std::mutex mu;
  std::condition_variable cv;
  int started = 0;
  int runs[4] = {0, 0, 0, 0};
  bool met[4] = {false, false, false, false};
  std::set<std::thread::id> ids;
  run_lanes(
      4,
      [&](size_t i) {
        std::unique_lock<std::mutex> lk(mu);
        ++runs[i];
        ids.insert(std::this_thread::get_id());
        ++started;
        cv.notify_all();
        met[i] = cv.wait_for(lk, std::chrono::seconds(5), [&] { return started == 4; });
      },
      no_failure);
  for (int i = 0; i < 4; ++i) CHECK(runs[i] == 1 && met[i]);
  CHECK(ids.size() == 4 && ids.count(std::this_thread::get_id()) == 0);
  // ... and a single lane is a thread of its own too
  std::thread::id lone;
  run_lanes(1, [&](size_t) { lone = std::this_thread::get_id(); }, no_failure);
  CHECK(lone != std::thread::id() && lone != std::this_thread::get_id());
  return 0;
}

// (b) bodies 1 and 3 of 4 throw: the call throws body 1's Err unchanged, after all four bodies have finished, and on_failure ran for {1, 3}
static int smallest_failing_index_wins() {
  std::atomic<int> finished{0};
  std::mutex mu;
  std::multiset<size_t> failed;
  bool thrown = false;
  try {
    run_lanes(
        4,
        [&](size_t i) {
          // the failing bodies end first, the others well after them: the call must still wait for all
          std::this_thread::sleep_for(std::chrono::milliseconds(i % 2 ? 0 : 200));
          ++finished;
          if (i == 1) throw Err{RHCCQ_E_ARG, "lane one"};
          if (i == 3) throw Err{RHCCQ_E_LIMIT, "lane three"};
        },
        [&](size_t i) {
          std::lock_guard<std::mutex> g(mu);
          failed.insert(i);
        });
  } catch (const Err& e) {
    thrown = true;
    CHECK(finished.load() == 4);
    CHECK(e.code == RHCCQ_E_ARG && e.msg == "lane one");
  }
  CHECK(thrown);
  CHECK((failed == std::multiset<size_t>{1, 3}));
  return 0;
}

// (c) an exception of the standard library comes out as Err{RHCCQ_E_HIP, what()}
static int std_exception_becomes_err() {
  int failures = 0;
  bool thrown = false;
  try {
    run_lanes(2, [](size_t i) { if (i == 1) throw std::runtime_error("x"); }, [&](size_t i) { failures += i == 1 ? 1 : 100; });
  } catch (const Err& e) {
    thrown = true;
    CHECK(e.code == RHCCQ_E_HIP && e.msg == "x");
  }
  CHECK(thrown && failures == 1);
  return 0;
}

// (d) a scope that has started threads and is left by an exception joins them first (no std::terminate, their work is complete)
static int thread_group_joins_when_unwound() {
  std::atomic<int> done{0};
  bool caught = false;
  try {
    ThreadGroup g;
    for (int t = 0; t < 2; ++t)
      g.spawn([&] {
        std::this_thread::sleep_for(std::chrono::milliseconds(100));
        ++done;
      });
    throw std::runtime_error("leaving with threads running");
  } catch (const std::runtime_error&) {
    caught = true;
    CHECK(done.load() == 2);
  }
  CHECK(caught);
  // join_all() by hand, then the destructor finds nothing left to join
  ThreadGroup g;
  g.spawn([&] { ++done; });
  g.join_all();
  CHECK(done.load() == 3);
  return 0;
}

int main() {
  if (one_thread_per_index()) return 1;
  if (smallest_failing_index_wins()) return 2;
  if (std_exception_becomes_err()) return 3;
  if (thread_group_joins_when_unwound()) return 4;
  printf("host_raii ok\n");
  return 0;
}
