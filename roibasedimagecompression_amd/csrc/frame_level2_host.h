// The hand-over between the class threads of rhccq_encode_frame and its level-2 stage (encode_frame.hip, RHCCQ_OPT_FRAME_LEVEL2), as plain
// C++17: no HIP header, no device (tests/native/frame_level2_host_test.cpp compiles it with g++ and the host sanitizers).
//
// A class thread ends with the class's merged component (`comp2`, empty: the class has none and contributes nothing) and the level-2 job
// made from it (`job2`).  The stage takes the jobs of the classes it serves, in class order, through ONE clustering call and finishes
// every class with its own job.  Clocks: the call's time is level2_cluster (ms[2]) of EVERY class it served -- each of them waited for
// all of it, and a per-class report (level1_cluster, first_positions_merge, level2_cluster, level2_finish) still adds up to the class's
// share of the frame -- and a class's finish is its level2_finish (ms[3]).
#pragma once
#include <utility>
#include <vector>

// the classes that have a component, ascending
template <typename ClassOutT>
std::vector<int> level2_classes(const std::vector<ClassOutT>& outs) {
  std::vector<int> cis;
  for (size_t ci = 0; ci < outs.size(); ++ci)
    if (outs[ci].comp2) cis.push_back((int)ci);
  return cis;
}

// cluster(std::vector<JobT>&): all jobs in one call; finish(ci, out, job): the class's level-2 result from its clustered job;
// now_ms(): a monotonic clock.  An exception of either leaves through the call; the jobs taken so far are gone with it (the frame fails).
template <typename JobT, typename ClassOutT, typename Cluster, typename Finish, typename Clock>
void level2_handover(std::vector<ClassOutT>& outs, const std::vector<int>& cis, Cluster&& cluster, Finish&& finish, Clock&& now_ms) {
  if (cis.empty()) return;
  double t_prev = now_ms();
  std::vector<JobT> jobs(cis.size());
  for (size_t i = 0; i < cis.size(); ++i) jobs[i] = std::move(outs[(size_t)cis[i]].job2);
  cluster(jobs);
  const double t = now_ms();
  for (int ci : cis) outs[(size_t)ci].ms[2] += t - t_prev;
  for (size_t i = 0; i < cis.size(); ++i) {
    ClassOutT& out = outs[(size_t)cis[i]];
    t_prev = now_ms();
    finish(cis[i], out, jobs[i]);
    out.ms[3] += now_ms() - t_prev;
  }
}
