// The launch schedule of overlapped mini-batch steps for a batch of problems (rhccq_mbk_steps_batch, k8_minibatch.hip / k8_overlap.h), as
// plain C++17: no HIP header, no device (tests/native/frame_level2_host_test.cpp compiles it with g++ and the host sanitizers).
//
// Every kernel of the overlapped sequence takes ONE set of launch parameters: whether the tile minima it reads are speculative, whether
// the step reassigns, which batches it draws.  A problem's parameters follow from its own k, batch size, "samples since the last
// reassignment" and what the previous call left drawn (carry); two problems of a batch differ only around their reassigning steps
// (every 10 k / batch steps).  The schedule gives every problem exactly the launches it gets alone, and lets problems whose parameters
// agree at a step share them: a launch names its problems in a bit mask, the workgroups of the others return at once.
#pragma once
#include <cstdint>
#include <vector>

namespace rhccq_sched {

enum LaunchKind {
  kEstep = 0,      // classic E-step over all centres (no speculative tile minima: first step of a sequence, the step behind a reassignment)
  kFixPlain = 1,   // labels + inertia terms from the classic tile minima
  kFixSpec = 2,    // labels + inertia terms from the speculative tile minima and the centres the previous step touched
  kReassign = 3,   // a reassigning step: classic update, reassignment (it draws reassign_draws batches itself), inertia
  kPipe = 4,       // update + draw_count batches from draw_first + inertia + (spec_next) the speculative E-step of the next step
};

struct Launch {
  int kind = 0;
  unsigned mask = 0u;                  // problems of this launch
  long long draw_first = 0;
  int draw_count = 0, reassign_draws = 0;
  bool spec_next = false;
  int spec_tiles = 0;                  // kPipe with spec_next: most tiles of a problem of the launch
};

class BatchSchedule {
 public:
  // k[p], n[p]: centres and points of problem p; fast_mask: the problems on the overlapped schedule (the others get no launch here);
  // since0[p], carry[p]: as rhccq_mbk_steps_batch takes them; tile_s: centres per speculative tile
  BatchSchedule(int n_prob, const long long* k, const long long* n, unsigned fast_mask, long long step0, int n_steps, const int64_t* since0,
                const int32_t* carry, int tile_s)
      : n_prob_(n_prob), fast_(fast_mask), step0_(step0), n_steps_(n_steps), p_((size_t)n_prob) {
    for (int p = 0; p < n_prob; ++p) {
      if (!((fast_mask >> p) & 1u)) continue;
      Prob& q = p_[(size_t)p];
      const long long bs = n[p] < 1000 ? n[p] : 1000;
      // which steps of this call reassign (sklearn _random_reassign with no zero-weight centre left)
      q.R.assign((size_t)n_steps + 2, 0);
      long long since = since0[p];
      for (int s = 0; s < n_steps + 2; ++s) {
        since += bs;
        q.R[(size_t)s] = since >= 10 * k[p];
        if (q.R[(size_t)s]) since = 0;
      }
      q.drawn = step0 + ((carry[p] & 1) ? 1 : 0);
      q.have_spec = (carry[p] & 2) != 0;
      q.spec_tiles = (int)((k[p] + tile_s - 1) / tile_s);
    }
  }

  // the launches of step step0 + s in issue order (call with s = 0, 1, ..., n_steps - 1); false: a batch was drawn past a reassignment
  // (internal error of the schedule)
  bool step(int s, std::vector<Launch>& out) {
    out.clear();
    const long long step = step0_ + s;
    unsigned m_nospec = 0u, m_spec = 0u;
    for (int p = 0; p < n_prob_; ++p)
      if ((fast_ >> p) & 1u) (p_[(size_t)p].have_spec ? m_spec : m_nospec) |= 1u << p;
    if (m_nospec) {
      out.push_back(make(kEstep, m_nospec));
      out.push_back(make(kFixPlain, m_nospec));
    }
    if (m_spec) out.push_back(make(kFixSpec, m_spec));
    unsigned todo = fast_;
    while (todo) {
      int lead = 0;
      while (!((todo >> lead) & 1u)) ++lead;
      Launch l;
      if (!params(p_[(size_t)lead], s, step, l)) return false;
      for (int p = lead; p < n_prob_; ++p) {
        if (!((todo >> p) & 1u)) continue;
        Launch o;
        if (!params(p_[(size_t)p], s, step, o)) return false;
        if (o.kind != l.kind || o.draw_first != l.draw_first || o.draw_count != l.draw_count || o.reassign_draws != l.reassign_draws ||
            o.spec_next != l.spec_next)
          continue;
        l.mask |= 1u << p;
        if (o.spec_tiles > l.spec_tiles) l.spec_tiles = o.spec_tiles;
      }
      todo &= ~l.mask;
      out.push_back(l);
      for (int p = 0; p < n_prob_; ++p) {
        if (!((l.mask >> p) & 1u)) continue;
        Prob& q = p_[(size_t)p];
        if (l.kind == kReassign) {
          q.drawn = step + l.reassign_draws;
          q.have_spec = false;
        } else {
          q.drawn += l.draw_count;
          q.have_spec = l.spec_next;
        }
      }
    }
    return true;
  }

  // what problem p hands to the next call
  int32_t carry(int p) const {
    const Prob& q = p_[(size_t)p];
    return (q.drawn > step0_ + n_steps_ ? 1 : 0) | (q.have_spec ? 2 : 0);
  }

 private:
  struct Prob {
    std::vector<char> R;
    long long drawn = 0;               // newest batch in the ring
    bool have_spec = false;
    int spec_tiles = 0;
  };
  static Launch make(int kind, unsigned mask) {
    Launch l;
    l.kind = kind;
    l.mask = mask;
    return l;
  }
  // the update launch problem q gets at step s, alone
  static bool params(const Prob& q, int s, long long step, Launch& l) {
    l = Launch();
    l.draw_first = q.drawn + 1;
    if (q.R[(size_t)s]) {
      if (q.drawn != step) return false;
      l.kind = kReassign;
      l.reassign_draws = q.R[(size_t)s + 1] ? 1 : 2;
      return true;
    }
    l.kind = kPipe;
    l.spec_next = q.drawn >= step + 1;  // the speculative E-step of step + 1 needs its batch before this launch starts
    const long long target = q.R[(size_t)s + 1] ? step + 1 : step + 2;
    l.draw_count = target > q.drawn ? (int)(target - q.drawn) : 0;
    l.spec_tiles = l.spec_next ? q.spec_tiles : 0;
    return true;
  }

  int n_prob_;
  unsigned fast_;
  long long step0_;
  int n_steps_;
  std::vector<Prob> p_;
};

}  // namespace rhccq_sched
