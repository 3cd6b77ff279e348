// Host-only checks of csrc/mbk_fit_host.h: what the driver of the MiniBatchKMeans fits (mbk_fit, encode_frame.hip) decides between its
// launches, replayed against scripted state snapshots without a device.  tests/test_mbk_fit_host_cpu.py compiles this with
// g++ -std=c++17 -fsanitize=address,undefined and runs it as a child process; exit status 0 = every check held, otherwise the line that
// failed is on stderr.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <string>
#include <vector>

#include "mbk_fit_host.h"

using namespace rhccq_fit;

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

// (a) sklearn's rules, the values written out: batch = min(1000, n); init_size = 3 batch, 3 k if that is below k, n at most;
// T = 2 + floor(ln k); (k - 1) T uniforms; at most 100 n / batch steps; the stream stands 2 (k - 1) T words behind the first uniform
static int constants() {
  struct Row { int64_t n, k, batch, init_size; int T; int64_t uniforms, limit; };
  const Row rows[] = {
      {10000, 200, 1000, 3000, 7, 1393, 1000},         // ln 200 = 5.30
      {12040, 964, 1000, 3000, 8, 7704, 1204},         // ln 964 = 6.87
      {39214, 1569, 1000, 3000, 9, 14112, 3921},       // ln 1 569 = 7.36
      {1506366, 30128, 1000, 90384, 12, 361524, 150636},   // 3 000 < k: 3 k; ln 30 128 = 10.31
      {999, 20, 999, 999, 4, 76, 100},                 // the batch is the 999 points; 2 997 capped at n; ln 20 = 2.996
      {3000, 1500, 1000, 3000, 9, 13491, 300},         // ln 1 500 = 7.31
  };
  for (const Row& r : rows) {
    Problem c = problem(r.n, r.k);
    CHECK(c.n == r.n && c.k == r.k && c.batch == r.batch && c.init_size == r.init_size && c.T == r.T && c.n_uniforms == r.uniforms && c.limit == r.limit);
    chain_at(c, 6001, 17);
    CHECK(c.pos == 6001 && c.first == 17 && c.cursor0 == 6001 + 2 * r.uniforms && c.chain_words() == c.cursor0);
  }
  Problem one = problem(10000, 1);                     // k = 1: numpy still draws one uniform's worth of table, the stream does not move
  chain_at(one, 500, 0);
  CHECK(one.T == 2 && one.n_uniforms == 1 && one.cursor0 == 500 && one.chain_words() == 502);
  return 0;
}

// ---- a scripted device: what the state of a problem looks like after `launched` steps have been queued for it ------------------------------
struct Script {
  int64_t weighted_from;                               // steps done from which no centre is without weight
  int64_t stop_at;                                     // converges after this many steps (0: runs to its limit)
  int code;                                            // the stop code it ends with
};
constexpr int64_t kScriptWords = 1500;                 // MT19937 words a scripted step consumes

static int64_t script_since(const Problem& c, int64_t steps) {          // sklearn _random_reassign, from 0
  int64_t since = 0;
  for (int64_t i = 0; i < steps; ++i) {
    since += c.batch;
    if (since >= 10 * c.k) since = 0;
  }
  return since;
}
static int64_t script_end(const Problem& c, const Script& sc) { return sc.stop_at ? sc.stop_at : c.limit; }

static void script_state(const Problem& c, const Script& sc, int64_t launched, double* s) {
  const int64_t end = script_end(c, sc), d = launched < end ? launched : end;
  for (int i = 0; i < kStateDoubles; ++i) s[i] = 0.0;
  for (int64_t t = d > 0 ? d - 1 : 0; t <= d; ++t) {                     // the slots of the step before, then (other parity) the current ones
    s[(t & 1) ? kSinceOdd : kSince] = (double)script_since(c, t);
    s[(t & 1) ? kZeroWeightOdd : kZeroWeight] = t >= sc.weighted_from ? 0.0 : 7.0;
    s[(t & 1) ? kCursorOdd : kCursor] = (double)(c.cursor0 + t * kScriptWords);
  }
  s[kStepsDone] = (double)d;
  s[kFirstDrawn] = 1.0;
  if (d == end) {
    s[kStop] = (double)(sc.stop_at ? sc.code : 2);
    s[kStopAt] = (double)d;
  }
}

// ---- the driver's loop (mbk_fit) over the scripted device: a classic problem's next chunk waits for the newest snapshot, overlapped
// problems alone read the one two chunks behind ---------------------------------------------------------------------------------------------
struct Rec {
  int64_t step;
  Chunk ch;
  std::vector<int64_t> cursor, steps_known, since, zero;                 // what the plan knew of every problem when it decided
};

static std::vector<Rec> drive(Plan& plan, const std::vector<Script>& scripts) {
  const int N = plan.size();
  std::vector<Rec> recs;
  std::deque<std::vector<double>> pending;
  int64_t step = 0;
  while (true) {
    Rec r;
    r.step = step;
    for (int p = 0; p < N; ++p) {
      r.cursor.push_back(plan.view(p).cursor());
      r.steps_known.push_back(plan.view(p).steps_done());
      r.since.push_back(plan.view(p).since(step));
      r.zero.push_back(plan.view(p).zero_weight(step));
    }
    r.ch = plan.next(step);
    if (!r.ch.any() && pending.empty()) break;
    if (r.ch.any()) {
      recs.push_back(r);
      plan.advance(r.ch);
      step += r.ch.ns;
      std::vector<double> snap((size_t)N * kStateDoubles);
      for (int p = 0; p < N; ++p) script_state(plan.c[(size_t)p], scripts[(size_t)p], step, &snap[(size_t)p * kStateDoubles]);
      pending.push_back(snap);
    }
    if (r.ch.classic_mask) {
      plan.take(pending.back().data());
      pending.clear();
    } else if (pending.size() >= 2 || !r.ch.any()) {
      plan.take(pending.front().data());
      pending.pop_front();
    }
    if (plan.error()) break;
  }
  return recs;
}

static Problem at(int64_t n, int64_t k, int64_t pos) {
  Problem c = problem(n, k);
  chain_at(c, pos, 0);
  return c;
}

// (b) a lone problem: the first look of 16 classic steps, then chunks of 64; overlapped from the first snapshot without a zero-weight
// centre if k >= 1 024 and the E-step is tiled; both word horizons; `since` by the batch per step, back to 0 at 10 k
static int lone_replay() {
  {  // k = 1 569: every centre weighted after 10 steps -> overlapped from step 16, converges after 300 steps
    const Problem c = at(39214, 1569, 7000);
    Plan plan({c}, true);
    CHECK(plan.view(0).zero_weight(0) == 1569 && plan.view(0).cursor() == c.cursor0 && plan.view(0).steps_done() == 0);
    const std::vector<Rec> r = drive(plan, {Script{10, 300, 1}});
    CHECK(r.size() == 7);                              // two chunks are in flight when the stop comes back: they return at once
    CHECK(r[0].step == 0 && r[0].ch.ns == 16 && r[0].ch.classic_mask == 1u && r[0].ch.fast_mask == 0u && !r[0].ch.no_reassign && r[0].ch.entered == 0u);
    CHECK(r[0].ch.need == c.cursor0 + (16 + 3) * 16384);
    CHECK(r[1].step == 16 && r[1].ch.ns == 64 && r[1].ch.fast_mask == 1u && r[1].ch.classic_mask == 0u && r[1].ch.entered == 1u && !r[1].ch.no_reassign);
    const int64_t steps_known[7] = {0, 16, 16, 80, 144, 208, 272};       // the state two chunks behind
    for (size_t i = 1; i < 7; ++i) {
      CHECK(r[i].step == 16 + 64 * ((int64_t)i - 1) && r[i].ch.ns == 64 && r[i].ch.fast_mask == 1u && r[i].ch.classic_mask == 0u);
      CHECK(r[i].ch.entered == (i == 1 ? 1u : 0u));
      CHECK(r[i].steps_known[0] == steps_known[i]);
      CHECK(r[i].ch.need == c.cursor0 + steps_known[i] * kScriptWords + (r[i].step - steps_known[i] + 64 + 4) * 4200 + 8 * 16384);
    }
    CHECK(plan.overlapped_from[0] == 16 && plan.view(0).steps_done() == 300 && plan.view(0).stop_code() == 1 && plan.view(0).stop_at() == 300 && !plan.running[0]);
    // 10 k = 15 690: the 16th batch since a reassignment passes it
    CHECK(plan.since[0] == ((16 + 6 * 64) % 16) * 1000 && plan.since[0] == script_since(c, 16 + 6 * 64));
  }
  {  // `since` step by step: entry value from the snapshot, + batch per step, 0 when it reaches 10 k; a short batch (n = 900)
    const Problem c = at(900, 1100, 100);
    CHECK(c.batch == 900 && c.limit == 100);
    Plan plan({c}, true);
    const std::vector<Rec> r = drive(plan, {Script{3, 0, 0}});
    CHECK(r.size() == 3 && r[1].ch.entered == 1u && r[1].since[0] == script_since(c, 16) && r[2].step == 80 && r[2].ch.ns == 20 && r[2].ch.fast_mask == 1u);
    CHECK(script_since(c, 12) == 10800 && script_since(c, 13) == 0);     // 13 x 900 = 11 700 >= 11 000
    CHECK(plan.since[0] == script_since(c, 100) && plan.view(0).stop_code() == 2 && plan.view(0).steps_done() == 100);
  }
  {  // zero-weight centres until step 20: a classic chunk of 64 that may reassign, overlapped from the snapshot of step 80
    const Problem c = at(39214, 1569, 7000);
    Plan plan({c}, true);
    const std::vector<Rec> r = drive(plan, {Script{20, 200, 1}});
    CHECK(r.size() >= 3 && r[1].step == 16 && r[1].ch.ns == 64 && r[1].ch.classic_mask == 1u && r[1].ch.fast_mask == 0u && !r[1].ch.no_reassign);
    CHECK(r[1].zero[0] == 7 && r[1].ch.need == c.cursor0 + 16 * kScriptWords + (64 + 3) * 16384);
    CHECK(r[2].step == 80 && r[2].ch.entered == 1u && r[2].ch.fast_mask == 1u && plan.overlapped_from[0] == 80);
  }
  {  // k = 964: never overlapped.  10 k = 9 640 samples are 10 batches: a chunk of 64 always holds a reassignment, the last chunk of 3 steps
     // (limit 1 043 = 16 + 16 x 64 + 3; 1 040 steps are 104 periods) does not
    const Problem c = at(10430, 964, 6500);
    CHECK(c.limit == 1043);
    Plan plan({c}, true);
    const std::vector<Rec> r = drive(plan, {Script{5, 0, 0}});
    CHECK(r.size() == 18);
    for (size_t i = 0; i < r.size(); ++i) {
      CHECK(r[i].ch.classic_mask == 1u && r[i].ch.fast_mask == 0u && r[i].ch.entered == 0u);
      CHECK(r[i].steps_known[0] == r[i].step);         // a classic problem decides on the state of its launch index
      CHECK(r[i].ch.need == c.cursor0 + r[i].step * kScriptWords + (r[i].ch.ns + 3) * 16384);
      if (i > 0 && i < 17) CHECK(r[i].ch.ns == 64 && !r[i].ch.no_reassign);
    }
    CHECK(r[17].step == 1040 && r[17].ch.ns == 3 && r[17].since[0] == 0 && r[17].ch.no_reassign);
    CHECK(plan.overlapped_from[0] == -1 && plan.view(0).steps_done() == 1043);
  }
  {  // the grid E-step (the driver passes tiled = false from 200 000 centres on; the planner takes its word): never overlapped, whatever k;
     // classic chunks of 64 without the reassignment launch while since + 64 000 < 10 k = 301 280, with it around the reassigning step
    const Problem c = at(1506366, 30128, 90000);
    Plan plan({c}, false);
    const std::vector<Rec> r = drive(plan, {Script{10, 400, 1}});
    CHECK(r.size() == 7 && plan.overlapped_from[0] == -1);
    CHECK(!r[0].ch.no_reassign);                       // centres without weight
    for (size_t i = 1; i < r.size(); ++i) {
      CHECK(r[i].ch.ns == 64 && r[i].ch.classic_mask == 1u && r[i].ch.fast_mask == 0u);
      CHECK(r[i].since[0] == r[i].step * 1000 % 302000);                 // (the 302nd batch passes 301 280)
      CHECK(r[i].ch.no_reassign == (r[i].since[0] + 64000 < 301280));
    }
    // steps 16 .. 208 end below 301 280 samples (208 000 + 64 000), 272 .. 335 hold the 302nd batch, 336 starts 34 batches behind it
    CHECK(r[1].ch.no_reassign && r[2].ch.no_reassign && r[3].ch.no_reassign && r[4].ch.no_reassign && !r[5].ch.no_reassign && r[6].ch.no_reassign);
    // ... and with centres without weight it never is
    Plan plan2({c}, false);
    const std::vector<Rec> r2 = drive(plan2, {Script{1000, 100, 1}});
    for (const Rec& q : r2) CHECK(!q.ch.no_reassign && q.ch.classic_mask == 1u);
  }
  return 0;
}

// (c) three problems in one batch: one overlapped from step 16, one classic throughout (k < 1 024), one that stops at its 12th step.
// Every problem is in the batch's chunks, up to the step at which it stops, on the schedule and for the steps it gets alone (alone, an
// overlapped problem has up to two more chunks queued when its stop comes back two chunks late: launches that return at once); the
// batch's RHCCQ_STEPS_NO_REASSIGN is the AND of what its classic problems get alone; `need` is the largest of the problems' horizons
static int batch_equals_alone() {
  const std::vector<Problem> cs = {at(39214, 1569, 7000), at(10430, 964, 6500), at(45500, 4549, 30000)};
  const std::vector<Script> scripts = {Script{10, 200, 1}, Script{5, 150, 1}, Script{1000, 12, 1}};
  Plan batch(cs, true);
  const std::vector<Rec> rb = drive(batch, scripts);
  CHECK(rb.size() == 4);                               // 0, 16, 80, 144: both stops are in the snapshot of step 208
  CHECK(batch.overlapped_from[0] == 16 && batch.overlapped_from[1] == -1 && batch.overlapped_from[2] == -1);
  CHECK(batch.view(0).steps_done() == 200 && batch.view(1).steps_done() == 150 && batch.view(2).steps_done() == 12);
  for (const Rec& r : rb) CHECK((r.ch.fast_mask & r.ch.classic_mask) == 0u);
  CHECK(rb[0].ch.classic_mask == 7u && rb[0].ch.fast_mask == 0u);
  for (size_t i = 1; i < rb.size(); ++i) CHECK(rb[i].ch.fast_mask == 1u && rb[i].ch.classic_mask == 2u);   // the stopped one is in neither mask
  for (int p = 0; p < 3; ++p) {
    Plan alone({cs[(size_t)p]}, true);
    const std::vector<Rec> ra = drive(alone, {scripts[(size_t)p]});
    const int64_t end = script_end(cs[(size_t)p], scripts[(size_t)p]);
    size_t ia = 0;
    for (const Rec& r : rb) {
      const bool fast = (r.ch.fast_mask >> p) & 1u, classic = (r.ch.classic_mask >> p) & 1u;
      if (r.step >= end) { CHECK(!fast && !classic); continue; }
      CHECK(ia < ra.size() && ra[ia].step == r.step && ra[ia].ch.ns == r.ch.ns);
      CHECK(fast == (ra[ia].ch.fast_mask == 1u) && classic == (ra[ia].ch.classic_mask == 1u));
      CHECK(((r.ch.entered >> p) & 1u) == ra[ia].ch.entered);
      if (classic && r.ch.no_reassign) CHECK(ra[ia].ch.no_reassign);
      ++ia;
    }
    for (; ia < ra.size(); ++ia) CHECK(ra[ia].step >= end || ra[ia].step + ra[ia].ch.ns > end);   // alone, nothing else did work
    CHECK(alone.view(0).steps_done() == batch.view(p).steps_done() && alone.overlapped_from[0] == batch.overlapped_from[(size_t)p]);
    if (batch.fast[(size_t)p]) CHECK(alone.since[0] == script_since(cs[(size_t)p], 16 + 64 * ((int64_t)ra.size() - 1)));
  }
  for (const Rec& r : rb) {
    bool all_quiet = true;
    int64_t need = 0;
    for (int p = 0; p < 3; ++p) {
      const Problem& c = cs[(size_t)p];
      if ((r.ch.classic_mask >> p) & 1u) {
        all_quiet = all_quiet && r.zero[(size_t)p] == 0 && r.since[(size_t)p] + r.ch.ns * c.batch < 10 * c.k;
        need = std::max(need, r.cursor[(size_t)p] + (r.ch.ns + 3) * 16384);
      } else if ((r.ch.fast_mask >> p) & 1u) {
        need = std::max(need, r.cursor[(size_t)p] + (r.step - r.steps_known[(size_t)p] + r.ch.ns + 4) * 4200 + 8 * 16384);
      }
    }
    CHECK(r.ch.no_reassign == all_quiet && r.ch.need == need);
  }
  CHECK(rb[0].ch.need == cs[2].cursor0 + 19 * 16384);                    // the longest chain stands furthest in the stream
  // a batch whose only classic problem is quiet gets the flag beside an overlapped one: 3 steps left of k = 964 (as in lone_replay)
  Plan two({cs[0], cs[1]}, true);
  const std::vector<Rec> r2 = drive(two, {Script{10, 0, 0}, Script{5, 0, 0}});
  bool seen = false;
  for (const Rec& r : r2)
    if (r.step == 1040) {
      // (the batch's chunk is 64 steps, the other problem runs on: k = 964 would reassign in it, and only its last 3 steps count for it)
      CHECK(r.ch.ns == 64 && r.ch.classic_mask == 2u && r.ch.fast_mask == 1u && !r.ch.no_reassign);
      seen = true;
    }
  CHECK(seen);
  return 0;
}

// (d) three problems laid out back to back: centres, init samples, uniforms; the sums the set-up allocates by; split and grid rules
static int layout() {
  const std::vector<Problem> cs = {at(39214, 1569, 7000), at(12040, 964, 6500), at(45500, 4549, 30000)};
  rhccq_mbk_problem q[3];
  Totals t;
  for (int p = 0; p < 3; ++p) {
    std::memset(&q[p], 0, sizeof(q[p]));
    q[p].off = 1000 * p; q[p].n = cs[(size_t)p].n; q[p].k = cs[(size_t)p].k;
    Problem c = cs[(size_t)p];
    c.first = 40 + p;
    t.add(q[p], c);
  }
  CHECK(q[0].koff == 0 && q[1].koff == 1569 && q[2].koff == 1569 + 964);
  CHECK(q[0].init_off == 0 && q[1].init_off == 3000 && q[2].init_off == 6000);
  CHECK(q[0].init_n == 3000 && q[1].init_n == 3000 && q[2].init_n == 13647);          // 3 000 < 4 549: 3 k
  CHECK(q[0].rand_off == 0 && q[1].rand_off == 14112 && q[2].rand_off == 14112 + 7704);
  CHECK(q[0].T == 9 && q[1].T == 8 && q[2].T == 10 && q[0].first == 40 && q[1].first == 41 && q[2].first == 42);
  CHECK(q[0].off == 0 && q[1].off == 1000 && q[2].off == 2000 && q[2].n == 45500 && q[2].k == 4549);   // the caller's, untouched
  CHECK(t.ktot == 1569 + 964 + 4549 && t.itot == 19647 && t.utot == 14112 + 7704 + 45480);
  CHECK(t.words == 30000 + 2 * 45480 && t.k_max == 4549 && t.tiles == 4 + 2 + 9 && t.tiled() && t.split() == 8);
  Totals none;
  CHECK(none.words == 1 && none.ktot == 0);
  // the E-step split: the first of 1, 2, 4, 8 that brings tiles * 2 * split to 1 536, else 8; the grid from 200 000 centres in one problem
  const int64_t ks[] = {768 * 512, 767 * 512, 384 * 512, 383 * 512, 192 * 512, 191 * 512 + 1, 191 * 512, 30128, 199999, 200000};
  const int splits[] = {1, 2, 2, 4, 4, 4, 8, 8, 2, 2};
  const bool tiled[] = {false, false, true, true, true, true, true, true, true, false};
  for (int i = 0; i < 10; ++i) {
    rhccq_mbk_problem one;
    std::memset(&one, 0, sizeof(one));
    Totals u;
    u.add(one, problem(10 * ks[i], ks[i]));
    CHECK(u.split() == splits[i] && u.tiled() == tiled[i]);
  }
  return 0;
}

// (e) stop codes 3, 4, 5 are the three errors; 0 (running), 1 (converged), 2 (out of steps) are none; a plan reports its first error
static int stop_codes() {
  CHECK(std::string(stop_error(3)) == "mini-batch steps ran past the end of the MT19937 word table (internal sizing error)");
  CHECK(std::string(stop_error(4)) == "the sharded k-means++ chain gave up waiting for a partner workgroup");
  CHECK(std::string(stop_error(5)) == "the overlapped mini-batch schedule and the device state disagree about a reassignment");
  CHECK(!stop_error(0) && !stop_error(1) && !stop_error(2) && !stop_error(6));
  const std::vector<Problem> cs = {at(39214, 1569, 7000), at(12040, 964, 6500)};
  Plan plan(cs, true);
  CHECK(!plan.error());
  const std::vector<Rec> r = drive(plan, {Script{10, 0, 0}, Script{5, 40, 5}});
  CHECK(r.size() == 2 && plan.error() == stop_error(5) && !plan.running[1] && plan.running[0]);
  return 0;
}

int main() {
  if (constants()) return 1;
  if (lone_replay()) return 1;
  if (batch_equals_alone()) return 1;
  if (layout()) return 1;
  if (stop_codes()) return 1;
  printf("mbk_fit_host ok\n");
  return 0;
}
