// Host-only checks of csrc/chain_release_host.h: how a lane of rhccq_encode_frame waits for its problem's chain inside the frame's chain
// launch.  The flag read, the event query and the sleep are scripted; no device.  tests/test_chain_release_host_cpu.py compiles this with
// g++ -std=c++17 -fsanitize=address,undefined and runs it as a child process; exit status 0 = every check held, otherwise the line that
// failed is on stderr.
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <vector>

#include "chain_release_host.h"

#define CHECK(cond)                                                      \
  do {                                                                   \
    if (!(cond)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      return 1;                                                          \
    }                                                                    \
  } while (0)

using namespace rhccq_release;

// a scripted launch: what the flag holds and what the event query answers at every look (the last entry repeats)
struct Script {
  std::vector<uint32_t> flag;
  std::vector<int> event;
  int flag_reads = 0, queries = 0, naps = 0;
  int look = 0;                                          // a nap moves on to the next entry
  uint32_t read_flag() {
    ++flag_reads;
    return flag[(size_t)(look < (int)flag.size() ? look : (int)flag.size() - 1)];
  }
  int query() {
    ++queries;
    return event[(size_t)(look < (int)event.size() ? look : (int)event.size() - 1)];
  }
  void nap() {
    ++naps;
    ++look;
    if (naps > 1000) throw std::logic_error("the wait does not end");
  }
  Released run(uint32_t tag) {
    return wait_released(
        tag, [&] { return read_flag(); }, [&] { return query(); }, [&] { nap(); }, [&](int code) { throw std::runtime_error("query failed " + std::to_string(code)); });
  }
};

// (a) the flag fires before the event: released by the flag at the look that shows it, no sleep after that, the event not asked again
static int flag_before_event() {
  Script s;
  s.flag = {0u, 0u, 0u, 7u};
  s.event = {kNotReady};
  CHECK(s.run(7u) == kByFlag);
  CHECK(s.naps == 3 && s.flag_reads == 4 && s.queries == 3);
  Script now;                                            // already there at the first look: no query, no sleep
  now.flag = {7u};
  now.event = {kNotReady};
  CHECK(now.run(7u) == kByFlag && now.naps == 0 && now.queries == 0 && now.flag_reads == 1);
  return 0;
}

// (b) the event completes and the flag is never set (a kernel that publishes nothing): go, not an error
static int event_fallback() {
  Script s;
  s.flag = {0u};
  s.event = {kNotReady, kNotReady, kComplete};
  CHECK(s.run(5u) == kByEvent);
  CHECK(s.naps == 2 && s.queries == 3 && s.flag_reads == 3);
  Script both;                                           // both hold at the same look: the flag is looked at first
  both.flag = {0u, 9u};
  both.event = {kNotReady, kComplete};
  CHECK(both.run(9u) == kByFlag && both.naps == 1);
  Script notag;                                          // tag 0 = no flag to look at: the event alone
  notag.flag = {0u};
  notag.event = {kNotReady, kComplete};
  CHECK(notag.run(0u) == kByEvent && notag.flag_reads == 0 && notag.naps == 1);
  return 0;
}

// (c) the previous frame's tag in the flag is not taken; this frame's is
static int stale_tag() {
  Script s;
  s.flag = {41u, 41u, 41u, 42u};
  s.event = {kNotReady};
  CHECK(s.run(42u) == kByFlag && s.naps == 3);
  Script never;                                          // only the stale tag ever: the event ends the wait
  never.flag = {41u};
  never.event = {kNotReady, kNotReady, kNotReady, kNotReady, kComplete};
  CHECK(never.run(42u) == kByEvent && never.naps == 4);
  CHECK(next_tag(0u) == 1u && next_tag(41u) == 42u && next_tag(0xffffffffu) == 1u);      // never 0
  return 0;
}

// (d) an event query that reports an error: the policy throws at that look and does not sleep again
static int query_error() {
  Script s;
  s.flag = {0u};
  s.event = {kNotReady, kNotReady, 719};
  bool caught = false;
  try {
    s.run(3u);
  } catch (const std::runtime_error& e) {
    caught = std::string(e.what()) == "query failed 719";
  }
  CHECK(caught && s.naps == 2 && s.queries == 3);
  return 0;
}

// (e) once either condition holds nothing sleeps again: the wait returns at that look whatever the script would say later
static int no_sleep_after_release() {
  for (int at = 0; at < 6; ++at) {
    Script f;
    f.flag.assign((size_t)at, 0u);
    f.flag.push_back(11u);
    f.flag.push_back(0u);                                // (never looked at)
    f.event = {kNotReady};
    CHECK(f.run(11u) == kByFlag && f.naps == at && f.look == at);
    Script e;
    e.flag = {0u};
    e.event.assign((size_t)at, kNotReady);
    e.event.push_back(kComplete);
    e.event.push_back(kNotReady);
    CHECK(e.run(11u) == kByEvent && e.naps == at && e.look == at);
  }
  return 0;
}

int main() {
  static_assert(kFlagStrideWords * 4 == 64, "a flag per 64-byte line");
  if (flag_before_event()) return 1;
  if (event_fallback()) return 1;
  if (stale_tag()) return 1;
  if (query_error()) return 1;
  if (no_sleep_after_release()) return 1;
  printf("chain_release_host ok\n");
  return 0;
}
