// How a lane of rhccq_encode_frame waits for its problem's k-means++ chain inside the frame's one chain launch (encode_frame.hip,
// RHCCQ_OPT_CHAIN_RELEASE), as plain C++17: no HIP header, no device (tests/native/chain_release_host_test.cpp compiles it with g++ and
// the host sanitizers).
//
// The chain kernel publishes a problem the moment its own chain has ended: it stores the launch's tag (a non-zero frame serial) into the
// problem's flag in mapped host memory, behind a release of the problem's centres.  The launch's event fires when ALL chains have ended.
// A lane waits ON THE HOST and enqueues nothing before its chain has ended: a wait queued in its stream would sit in a hardware queue that
// other lanes' streams share and hold them up for the rest of the longest chain.
//
//   flag == tag            the problem's chain has ended: go
//   event complete         every chain has ended: go (the launch of a kernel that publishes nothing ends the wait this way; not an error)
//   event query fails      throw: the launch is lost, the flag may never come
//   neither                sleep (a few tens of microseconds; up to 8 lanes per class wait at once, so no busy spin), look again
//
// The loop never waits on the flag alone: a launch that ends for any reason ends the wait.  A flag left by an earlier frame carries that
// frame's tag and never matches, so flags are never cleared.
#pragma once
#include <cstdint>
#include <utility>

namespace rhccq_release {

enum Query { kComplete = 0, kNotReady = 1 };            // what query_event() answers; any other value is an error of the runtime's
enum Released { kByFlag = 0, kByEvent = 1 };

// flags of neighbouring problems never share a 64-byte line (the device writes one, the lanes of the others poll theirs)
constexpr int kFlagStrideWords = 16;

// a frame's tag: the serial after `prev`, never 0 (0 is what a flag holds before its first launch)
inline uint32_t next_tag(uint32_t prev) {
  const uint32_t t = prev + 1u;
  return t ? t : 1u;
}

// read_flag() -> uint32_t (an acquiring read of the problem's flag); query_event() -> int (Query, or the runtime's error code);
// nap(): sleep once; fail(int code): must throw.  Returns what ended the wait.
template <typename ReadFlag, typename QueryEvent, typename Nap, typename Fail>
Released wait_released(uint32_t tag, ReadFlag&& read_flag, QueryEvent&& query_event, Nap&& nap, Fail&& fail) {
  while (true) {
    if (tag != 0u && read_flag() == tag) return kByFlag;
    const int q = query_event();
    if (q == kComplete) return kByEvent;
    if (q != kNotReady) fail(q);
    nap();
  }
}

}  // namespace rhccq_release
