// Host-only checks of what rhccq_encode_frame's level-2 stage does without a device: csrc/frame_level2_host.h (the hand-over of the classes'
// components and level-2 jobs, the clocks behind the timing keys) and csrc/mbk_schedule.h (the launch schedule of a batch of overlapped
// mini-batch fits).  tests/test_frame_level2_host_cpu.py compiles this with g++ -std=c++17 -fsanitize=address,undefined and runs it as a
// child process; exit status 0 = every check held, otherwise the line that failed is on stderr.
#include <cstdint>
#include <cstdio>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "frame_level2_host.h"
#include "mbk_schedule.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

// ---- the hand-over -----------------------------------------------------------------------------------------------------------------
struct FakeJob {
  std::vector<uint32_t> keys;
  int quality = 0;
  int clustered_in_call = -1;
};
struct FakeOut {
  std::shared_ptr<int> comp2;
  FakeJob job2;
  std::shared_ptr<int> comp3;
  double ms[4] = {0, 0, 0, 0};
};

static FakeOut with_component(int tag, size_t n_keys, int quality) {
  FakeOut o;
  o.comp2 = std::make_shared<int>(tag);
  o.job2.keys.assign(n_keys, (uint32_t)tag);
  o.job2.quality = quality;
  o.ms[0] = 100.0 + tag;                               // what the class thread clocked before
  o.ms[1] = 1.0;
  return o;
}

// (a) three classes, the middle one without a component: the jobs of classes 0 and 2 reach ONE clustering call in class order, moved out
// of their classes; the call's time is level2_cluster of both and of nobody else; each class is finished with its own job
static int handover_order_and_clocks() {
  std::vector<FakeOut> outs;
  outs.push_back(with_component(7, 5, 40));
  outs.push_back(FakeOut());
  outs.push_back(with_component(9, 3, 80));
  const std::vector<int> cis = level2_classes(outs);
  CHECK(cis.size() == 2 && cis[0] == 0 && cis[1] == 2);
  double clock = 0.0;
  int calls = 0;
  std::vector<int> finished;
  level2_handover<FakeJob>(
      outs, cis,
      [&](std::vector<FakeJob>& jobs) {
        ++calls;
        clock += 11.0;                                 // the joined clustering takes 11 ms
        for (auto& j : jobs) j.clustered_in_call = calls;
        if (jobs.size() != 2 || jobs[0].keys.size() != 5 || jobs[0].keys[0] != 7u || jobs[0].quality != 40 || jobs[1].keys.size() != 3 ||
            jobs[1].keys[0] != 9u || jobs[1].quality != 80)
          throw std::runtime_error("jobs out of order");
      },
      [&](int ci, FakeOut& out, const FakeJob& jb) {
        clock += ci == 0 ? 0.25 : 0.5;
        finished.push_back(ci);
        if (jb.clustered_in_call != 1 || jb.keys[0] != (uint32_t)*out.comp2) throw std::runtime_error("a class was finished with another class's job");
        out.comp3 = std::make_shared<int>(*out.comp2 + 1000);
      },
      [&]() { return clock; });
  CHECK(calls == 1);
  CHECK(finished.size() == 2 && finished[0] == 0 && finished[1] == 2);
  CHECK(outs[0].job2.keys.empty() && outs[2].job2.keys.empty());             // handed over, not copied
  CHECK(outs[0].ms[2] == 11.0 && outs[2].ms[2] == 11.0 && outs[1].ms[2] == 0.0);
  CHECK(outs[0].ms[3] == 0.25 && outs[2].ms[3] == 0.5 && outs[1].ms[3] == 0.0);
  CHECK(outs[0].ms[0] == 107.0 && outs[0].ms[1] == 1.0 && outs[2].ms[0] == 109.0);   // the other keys are the class thread's
  CHECK(outs[0].comp3 && *outs[0].comp3 == 1007 && outs[2].comp3 && *outs[2].comp3 == 1009 && !outs[1].comp3);
  return 0;
}

// (b) nobody has a component: no clustering call, no clock touched; one class alone (the per-class path): its own call
static int handover_empty_and_single() {
  std::vector<FakeOut> outs(2);
  int calls = 0;
  level2_handover<FakeJob>(
      outs, level2_classes(outs), [&](std::vector<FakeJob>&) { ++calls; }, [&](int, FakeOut&, const FakeJob&) { ++calls; }, [&]() { return 1.0; });
  CHECK(calls == 0 && outs[0].ms[2] == 0.0 && outs[1].ms[3] == 0.0);
  outs[1] = with_component(3, 2, 20);
  double clock = 5.0;
  level2_handover<FakeJob>(
      outs, std::vector<int>(1, 1), [&](std::vector<FakeJob>& jobs) { calls += (int)jobs.size(); clock += 2.0; },
      [&](int ci, FakeOut&, const FakeJob&) { calls += 10 * ci; }, [&]() { return clock; });
  CHECK(calls == 11 && outs[1].ms[2] == 2.0 && outs[0].ms[2] == 0.0);
  return 0;
}

// (c) a clustering call that throws leaves through the hand-over and finishes nobody
static int handover_error() {
  std::vector<FakeOut> outs;
  outs.push_back(with_component(1, 4, 40));
  outs.push_back(with_component(2, 4, 40));
  bool finished = false, caught = false;
  try {
    level2_handover<FakeJob>(
        outs, level2_classes(outs), [&](std::vector<FakeJob>&) { throw std::runtime_error("boom"); },
        [&](int, FakeOut&, const FakeJob&) { finished = true; }, [&]() { return 0.0; });
  } catch (const std::runtime_error& e) {
    caught = std::string(e.what()) == "boom";
  }
  CHECK(caught && !finished && !outs[0].comp3 && !outs[1].comp3);
  return 0;
}

// ---- the schedule ------------------------------------------------------------------------------------------------------------------
using rhccq_sched::BatchSchedule;
using rhccq_sched::Launch;

// what problem p sees of a step's launches: kinds and parameters, without the masks and the other problems' tiles
struct Seen {
  int kind;
  long long draw_first;
  int draw_count, reassign_draws;
  bool spec_next;
  bool operator==(const Seen& o) const {
    return kind == o.kind && draw_first == o.draw_first && draw_count == o.draw_count && reassign_draws == o.reassign_draws && spec_next == o.spec_next;
  }
};
static std::vector<Seen> seen_by(const std::vector<Launch>& ls, int p) {
  std::vector<Seen> v;
  for (const Launch& l : ls)
    if ((l.mask >> p) & 1u) v.push_back(Seen{l.kind, l.draw_first, l.draw_count, l.reassign_draws, l.spec_next});
  return v;
}

// (d) in a batch, over several calls with the carries handed on, every problem sees exactly the launches it sees alone; every launch
// serves problems of the fast mask only, each fast problem is in exactly one update launch per step, a pipe launch has tiles for the
// largest of its problems; a problem outside the fast mask sees nothing
static int batch_equals_alone() {
  const int N = 4;
  const long long k[N] = {2314, 1569, 1024, 5000}, n[N] = {57837, 39214, 10240, 900};     // (the last problem's batch is its 900 points)
  const int64_t since_first[N] = {16000, 16000, 3000, 14400};
  const unsigned fast = 0xbu;                                                              // problem 2 is not on the overlapped schedule
  int64_t since_b[N], since_a[N];
  int32_t carry_b[N] = {0, 0, 0, 0}, carry_a[N] = {0, 0, 0, 0};
  for (int p = 0; p < N; ++p) since_b[p] = since_a[p] = since_first[p];
  long long step0 = 16;
  int shared = 0, launches_total = 0, reassigns = 0;
  for (int call = 0; call < 6; ++call) {
    const int ns = call == 5 ? 37 : 64;
    BatchSchedule batch(N, k, n, fast, step0, ns, since_b, carry_b, 256);
    std::vector<std::unique_ptr<BatchSchedule>> alone;
    for (int p = 0; p < N; ++p) alone.emplace_back(new BatchSchedule(1, &k[p], &n[p], 1u, step0, ns, &since_a[p], &carry_a[p], 256));
    std::vector<Launch> lb, la;
    for (int s = 0; s < ns; ++s) {
      CHECK(batch.step(s, lb));
      unsigned updated = 0u;
      for (const Launch& l : lb) {
        CHECK(l.mask != 0u && (l.mask & ~fast) == 0u);
        ++launches_total;
        if ((l.mask & (l.mask - 1u)) != 0u) ++shared;
        if (l.kind == rhccq_sched::kPipe || l.kind == rhccq_sched::kReassign) {
          CHECK((updated & l.mask) == 0u);
          updated |= l.mask;
          if (l.kind == rhccq_sched::kReassign) ++reassigns;
          for (int p = 0; p < N; ++p)
            if (((l.mask >> p) & 1u) && l.kind == rhccq_sched::kPipe && l.spec_next) CHECK(l.spec_tiles >= (int)((k[p] + 255) / 256));
        }
      }
      CHECK(updated == fast);
      CHECK(seen_by(lb, 2).empty());
      for (int p = 0; p < N; ++p) {
        if (!((fast >> p) & 1u)) continue;
        CHECK(alone[(size_t)p]->step(s, la));
        CHECK(seen_by(lb, p) == seen_by(la, 0));
      }
    }
    for (int p = 0; p < N; ++p) {
      if (!((fast >> p) & 1u)) continue;
      carry_b[p] = batch.carry(p);
      carry_a[p] = alone[(size_t)p]->carry(0);
      CHECK(carry_b[p] == carry_a[p]);
      const long long bs = n[p] < 1000 ? n[p] : 1000;
      for (int i = 0; i < ns; ++i) {                     // the caller's arithmetic between calls (encode_frame.hip)
        since_b[p] += bs;
        if (since_b[p] >= 10 * k[p]) since_b[p] = 0;
      }
      since_a[p] = since_b[p];
    }
    step0 += ns;
  }
  CHECK(reassigns > 10);                                 // (k = 1 569 reassigns every 16th step)
  CHECK(shared * 2 > launches_total);                    // most launches serve more than one problem: that is the point of the batch
  return 0;
}

// (e) a lone problem's steady state is two launches per step; the first two steps of a sequence (the batch of the second is not drawn
// when the first starts, so nothing can be speculated for it) and the step behind a reassignment add the classic E-step
static int lone_steady_state() {
  const long long k = 2000, n = 50000;
  const int64_t since0 = 0;
  const int32_t carry0 = 0;
  BatchSchedule one(1, &k, &n, 1u, 16, 64, &since0, &carry0, 256);
  std::vector<Launch> l;
  int n_reassign = 0;
  bool after_reassign = false;
  for (int s = 0; s < 64; ++s) {
    CHECK(one.step(s, l));
    if (after_reassign || s < 2) CHECK(l.size() == 3 && l[0].kind == rhccq_sched::kEstep && l[1].kind == rhccq_sched::kFixPlain);
    else CHECK(l.size() == 2 && l[0].kind == rhccq_sched::kFixSpec);
    after_reassign = l.back().kind == rhccq_sched::kReassign;
    n_reassign += after_reassign;
    CHECK(after_reassign == ((s + 1) % 20 == 0));        // 10 k / 1000 = every 20th step
  }
  CHECK(n_reassign == 3);
  return 0;
}

int main() {
  if (handover_order_and_clocks()) return 1;
  if (handover_empty_and_single()) return 1;
  if (handover_error()) return 1;
  if (batch_equals_alone()) return 1;
  if (lone_steady_state()) return 1;
  printf("frame_level2_host ok\n");
  return 0;
}
