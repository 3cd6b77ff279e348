// Owners for what the native host (encode_frame.hip) starts and creates: host threads, HIP events, streams, pinned memory and the sibling
// contexts of its lanes.  Everything is released by a destructor, so no exit path -- a return, an Err, an exception of the standard library --
// can forget it.  The first section is plain C++17 (tests/native/host_raii_test.cpp compiles it with g++); the HIP owners follow under hipcc.
#pragma once
#include <exception>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rhccq.h"

// what the host code throws; the extern "C" entry turns it into its return value and rhccq_last_error()
struct Err {
  int code;
  std::string msg;
};

// Host threads that are joined on every way out of the scope, an exception among them (a joinable std::thread that is destroyed ends the
// process: std::terminate)
class ThreadGroup {
 public:
  ThreadGroup() = default;
  ThreadGroup(const ThreadGroup&) = delete;
  ThreadGroup& operator=(const ThreadGroup&) = delete;
  ~ThreadGroup() { join_all(); }
  template <typename Fn>
  void spawn(Fn&& fn) {
    threads_.emplace_back(std::forward<Fn>(fn));
  }
  void join_all() {
    for (auto& t : threads_)
      if (t.joinable()) t.join();
  }

 private:
  std::vector<std::thread> threads_;
};

// body(i) for i in [0, n), every index on a thread of its own (also for n == 1: the caller's thread only waits).  An Err or a
// std::exception (-> RHCCQ_E_HIP) that leaves a body is kept and on_failure(i) runs on that thread (it must not throw); every thread is
// joined before the call returns or throws, also when a thread cannot be started; then the error of the smallest failing index is thrown.
template <typename Body, typename OnFailure>
void run_lanes(size_t n, Body&& body, OnFailure&& on_failure) {
  std::vector<Err> errs(n, Err{0, ""});
  {
    ThreadGroup group;
    for (size_t i = 0; i < n; ++i)
      group.spawn([&, i]() {
        try {
          body(i);
          return;
        } catch (const Err& e) {
          errs[i] = e;
        } catch (const std::exception& e) {
          errs[i] = Err{RHCCQ_E_HIP, e.what()};
        }
        on_failure(i);
      });
  }
  for (auto& e : errs)
    if (e.code) throw e;
}

#ifdef __HIPCC__
#include <hip/hip_runtime_api.h>

#include <type_traits>

#define EF_HIP(expr)                                                                                   \
  do {                                                                                                 \
    const hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) throw Err{RHCCQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)};   \
  } while (0)

// Move-only owners (get() is the plain handle; users that do not own, such as PreChain::done, keep plain handles)
struct HipRelease {
  void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); }
  void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); }
  void operator()(rhccq_ctx* c) const { rhccq_ctx_destroy(c); }
  void operator()(void* pinned) const { (void)hipHostFree(pinned); }
};
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, HipRelease>;
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, HipRelease>;
using Ctx = std::unique_ptr<rhccq_ctx, HipRelease>;
template <typename T>
using Pinned = std::unique_ptr<T[], HipRelease>;

// (all on the current device)
inline Event make_event() {
  hipEvent_t e = nullptr;
  EF_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return Event(e);
}
inline Stream make_stream() {
  hipStream_t s = nullptr;
  EF_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return Stream(s);
}
inline Ctx make_ctx(int device, hipStream_t stream) {
  rhccq_ctx* c = nullptr;
  if (rhccq_ctx_create(device, stream, &c)) throw Err{RHCCQ_E_HIP, "rhccq_ctx_create failed"};
  return Ctx(c);
}
template <typename T>
Pinned<T> make_pinned(size_t n) {
  void* p = nullptr;
  EF_HIP(hipHostMalloc(&p, n * sizeof(T)));
  return Pinned<T>((T*)p);
}

// Declared AFTER the host buffers that asynchronous copies on `stream` read or write, so that it is destroyed before them: when the scope
// is left by an exception, the stream is drained first and no copy still in flight finds its buffer gone.  Nothing on the way that succeeds.
class SyncOnUnwind {
 public:
  explicit SyncOnUnwind(hipStream_t stream) : stream_(stream), pending_(std::uncaught_exceptions()) {}
  SyncOnUnwind(const SyncOnUnwind&) = delete;
  SyncOnUnwind& operator=(const SyncOnUnwind&) = delete;
  ~SyncOnUnwind() {
    if (std::uncaught_exceptions() > pending_) (void)hipStreamSynchronize(stream_);
  }

 private:
  hipStream_t stream_;
  int pending_;
};
#endif  // __HIPCC__
