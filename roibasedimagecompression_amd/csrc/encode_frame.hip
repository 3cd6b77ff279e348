// rhccq_encode_frame: the fused frame encoder as native host code (include/rhccq.h).
//
// What roibasedimagecompression_amd/frame.py + palette.py + the MiniBatchKMeans driver of ops.py do in Python, restated in C++ over
// the same C entry points of this library: the three-level palette hierarchy of rhccq.ipynb:978-1039 for one frame whose segment
// label maps are given.  Reference semantics (paths relative to the reference root):
//   encoder/compression/subregions.py:315-449,634-679  per-segment crop (+2 px), black-in-segment fix, unique colours, cluster(q),
//                                                      merge per region
//   encoder/compression/clustering.py:160-437          cluster_palette_colors_parallel: black rows first, clusters <= mc in label order
//                                                      (floor means), oversize clusters split by KMeans depth-first, uint16 mapping
//   encoder/compression/merging.py:16-21,52-82         single-component passthrough, reversed painting, first-seen global palette
//   encoder/compression/regions.py:9-70, image.py:243-286   per class merge + cluster(2q); classes merged + cluster(q3); index dtype
// Host structure: the calling thread runs the per-pixel passes on the context's stream; every region class is a host thread with a
// sibling context (HIP stream + device arena of its own) that runs level 1 -> merges of its class; the MiniBatchKMeans problems of a
// class (>= 10 000 colours) run side by side on further sibling contexts.  The class threads end with their merged component and
// level-2 job; the calling thread clusters the level-2 palettes of all classes in one call on one lane, their MiniBatchKMeans
// problems as one batch (RHCCQ_OPT_FRAME_LEVEL2; 0: level 2 stays in the class threads).  No interpreter, no global lock; the only
// synchronisation points are the k-sized read-backs the ordering rules need.
// Ownership (host_raii.h): threads, events, streams, pinned memory and sibling contexts belong to owners whose destructors release them.
// The invariant on every exit path, an exception included: no host buffer that an asynchronous copy reads or writes is destroyed before
// its stream has been synchronised, and no event is destroyed while a thread that may still record or wait on it is running.  The second
// half is declaration order (events before the run_lanes call that joins the threads).  The first half is Lane::download for single
// copies (complete on return) and a SyncOnUnwind declared after the buffers wherever something can throw between a copy and its
// synchronisation; a pageable source of a host-to-device copy is staged before the call returns (Lane::upload) and needs neither.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

#include "chain_release_host.h"
#include "frame_level2_host.h"
#include "host_raii.h"
#include "mbk_fit_host.h"
#include "mt_replay.h"
#include "rhccq_common.h"

namespace {

constexpr int32_t kIntMax = 0x7fffffff;
constexpr int64_t kFpNone = kIntMax;
constexpr int64_t kMinibatchThreshold = 10000;      // clustering.py:207
constexpr int kMaxJobs = 2048;

#define EF_RC(ctx, call)                                                                               \
  do {                                                                                                 \
    const int rc_ = (call);                                                                            \
    if (rc_) throw Err{rc_, std::string(#call) + ": " + rhccq_last_error(ctx)};                        \
  } while (0)

// RHCCQ_TRACE=1: per-phase host clocks of every MiniBatchKMeans fit on stderr (diagnostic: adds stream synchronisations)
bool trace_on() {
  static const bool on = [] { const char* e = getenv("RHCCQ_TRACE"); return e && e[0] == '1'; }();
  return on;
}

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// numpy's RandomState(42) and the draws ahead of a fit's k-means++ chain: mt_replay.h; the word table of a device: rhccq_mt_words
using rhccq_mt::first_centre_index;
using rhccq_mt::mbk_draws;
using rhccq_mt::MbkDraws;

// ---- a sibling context: HIP stream + bump arena of device memory, kept between frames -----------------------------------------
struct Arena {
  struct Block {
    char* p;
    size_t cap;
  };
  std::vector<Block> blocks;
  size_t used = 0;
  void* alloc(size_t bytes) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (bytes == 0) bytes = 256;
    if (blocks.empty() || used + bytes > blocks.back().cap) {
      size_t cap = std::max<size_t>(bytes, (size_t)64 << 20);
      if (!blocks.empty()) cap = std::max(cap, 2 * blocks.back().cap);
      void* p = nullptr;
      EF_HIP(hipMalloc(&p, cap));
      blocks.push_back(Block{(char*)p, cap});
      used = 0;
    }
    void* out = blocks.back().p + used;
    used += bytes;
    return out;
  }
  // between frames (every stream idle): several blocks -> one of their total size, so that the next frame allocates nothing
  void reset() {
    if (blocks.size() > 1) {
      size_t total = 0;
      for (auto& b : blocks) {
        total += b.cap;
        (void)hipFree(b.p);
      }
      blocks.clear();
      void* p = nullptr;
      if (hipMalloc(&p, total) == hipSuccess) blocks.push_back(Block{(char*)p, total});
    }
    used = 0;
  }
  ~Arena() {
    for (auto& b : blocks) (void)hipFree(b.p);
  }
};

struct Lane {
  // (members are released in the reverse of this order: sub-lanes, events, pinned buffer, context, stream, arena)
  int device = 0;
  Arena arena;
  Stream stream;
  Ctx ctx;
  Pinned<double> pinned;                               // 3 x 32 x 16 doubles: landing buffers of the asynchronous state polls of a fit (mbk_fit)
  Event ev[3];
  std::vector<std::unique_ptr<Lane>> sub;              // further siblings (the MiniBatchKMeans problems of a class)

  explicit Lane(int dev) : device(dev) {               // (a throw half way releases what exists: the members are complete objects by now)
    EF_HIP(hipSetDevice(dev));
    stream = make_stream();
    ctx = make_ctx(dev, stream.get());
    pinned = make_pinned<double>(3 * rhccq_fit::kMaxProblems * rhccq_fit::kStateDoubles);
    for (auto& e : ev) e = make_event();
  }
  Lane& sublane(size_t i) {
    while (sub.size() <= i) {
      sub.push_back(std::make_unique<Lane>(device));
      sub.back()->adopt_options(ctx.get());
    }
    return *sub[i];
  }
  void adopt_options(const rhccq_ctx* root) {
    ctx->opt_init_lds_blocks = root->opt_init_lds_blocks;
    ctx->opt_init_max_items = root->opt_init_max_items;
    ctx->opt_init_kernel = root->opt_init_kernel;
    ctx->opt_init_cands_per_wave = root->opt_init_cands_per_wave;
    ctx->opt_reassign_lds = root->opt_reassign_lds;
    ctx->opt_reassign_order = root->opt_reassign_order;
    ctx->opt_init_shards = root->opt_init_shards;
    ctx->opt_kmeans_wide_pairs = root->opt_kmeans_wide_pairs;
    ctx->opt_kmeans_chunk = root->opt_kmeans_chunk;
    for (auto& s : sub) s->adopt_options(root);
  }
  void reset() {
    arena.reset();
    for (auto& s : sub) s->reset();
  }
  template <typename T>
  T* dalloc(size_t n) {
    return (T*)arena.alloc(n * sizeof(T));
  }
  template <typename T>
  T* dzeros(size_t n) {
    T* p = dalloc<T>(n);
    EF_HIP(hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), stream.get()));
    return p;
  }
  template <typename T>
  T* upload(const T* host, size_t n) {                 // pageable source: the copy is staged before the call returns
    T* p = dalloc<T>(n);
    if (n) EF_HIP(hipMemcpyAsync(p, host, n * sizeof(T), hipMemcpyHostToDevice, stream.get()));
    return p;
  }
  template <typename T>
  void download(T* host, const T* dev, size_t n) {     // complete on return
    if (n) EF_HIP(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, stream.get()));
    EF_HIP(hipStreamSynchronize(stream.get()));
  }
  void sync() { EF_HIP(hipStreamSynchronize(stream.get())); }
};

struct FreeReleaseFlags {
  void operator()(uint32_t* host) const { rhccq_release_flags_free(host); }
};
using ReleaseFlags = std::unique_ptr<uint32_t, FreeReleaseFlags>;

struct Level2Fit {                                       // one MiniBatchKMeans fit of the frame's level-2 stage
  int32_t cls = 0;
  int64_t n = 0, k = 0, steps = 0;
  int32_t schedule = 0;                                // 0 = a fit of its own (lone problem), 1 = in a batch, classic steps only, 2 = in a batch, overlapped
  int64_t overlapped_from = -1;                        // in a batch: the step at which it went to the overlapped schedule (-1: never)
};
struct FrameState {
  std::vector<std::unique_ptr<Lane>> classes;
  Arena root_arena;                                    // the per-pixel tables of a frame (allocated and used on the caller's stream)
  std::vector<Level2Fit> level2_fits;                  // the last frame's level-2 MiniBatchKMeans fits (rhccq_encode_frame_level2_info)
  // RHCCQ_OPT_CHAIN_RELEASE: one flag per problem of the frame's chain launch (mapped host memory, a 64-byte line each), the tag of the
  // last launch.  Never cleared: a launch's tag is new, so what an earlier frame left never matches.
  ReleaseFlags release_flags;
  uint32_t* release_flags_dev = nullptr;               // their device address
  int32_t release_cap = 0;                             // problems the flags have room for
  uint32_t release_tag = 0;
};
void free_frame_state(void* p) { delete (FrameState*)p; }

// ---- MiniBatchKMeans(k, batch_size=1000, random_state=42, n_init='auto').fit_predict of 1 .. 32 palettes resident on the device
// (ops.py::minibatch_kmeans; reference call site clustering.py:207-218).  What the host decides on the way is mbk_fit_host.h, its draws mt_replay.h -
// A chain run ahead for one fit (RHCCQ_OPT_FRAME_CHAINS): its centres once `done` has fired, or, with RHCCQ_OPT_CHAIN_RELEASE, once
// *flag shows `tag` (chain_release_host.h); tag 0: the kernel publishes nothing, the event alone
struct PreChain {
  MbkDraws draws;
  double* centres = nullptr;                           // [k][4], written by the chain, then the fit's own
  hipEvent_t done = nullptr;
  const uint32_t* flag = nullptr;                      // host address of the problem's release flag
  uint32_t tag = 0;
  bool host_wait = false;                              // the lane waits on the host (flag or event) and queues nothing before
};

// The lane's wait for its chain on the host: nothing is queued on the lane's stream until the chain has ended
rhccq_release::Released wait_for_chain(const PreChain& pre) {
  const rhccq_release::Released how = rhccq_release::wait_released(
      pre.tag, [&] { return __atomic_load_n(pre.flag, __ATOMIC_ACQUIRE); },
      [&]() -> int {
        const hipError_t e = hipEventQuery(pre.done);
        if (e == hipSuccess) return rhccq_release::kComplete;
        if (e == hipErrorNotReady) return rhccq_release::kNotReady;
        (void)hipGetLastError();
        return 2 + (int)e;
      },
      [] { std::this_thread::sleep_for(std::chrono::microseconds(30)); },
      [](int code) { throw Err{RHCCQ_E_HIP, std::string("the frame's chain launch: hipEventQuery: ") + hipGetErrorString((hipError_t)(code - 2))}; });
  (void)hipGetLastError();                             // ("not ready" is an answer, not an error the next launch check of this thread should find)
  return how;
}

// the third-generation chain's LDS limit (k8_init3.h): problems above it are left to their lanes, so that a frame's launch never
// moves a problem to another generation of the chain than the one it gets alone
constexpr int64_t kFrameChainMaxInit = 98304;

// (RHCCQ_TRACE) the clocks of a chain set-up, taken behind the stream's work up to there (sync) or as host time only
struct ChainClocks {
  bool sync = true;
  double words = 0, uploaded = 0, ordered = 0, chained = 0;
};

// The k-means++ chains of `probs` (off / n / k the caller's, the rest laid out: rhccq_fit::Totals) as ONE launch on c's stream: every
// problem's uniforms from its own MT19937 word, the init samples in one upload, one Morton order, zeroed centres and `chosen`,
// rhccq_mbk_init with a workgroup per problem (the kernels treat the problems of a batch independently).  Returns the centres [ktot][4].
// flags / tag / published (frame_chains, RHCCQ_OPT_CHAIN_RELEASE): the launch publishes every problem when its own chain has ended.
double* mbk_chains(rhccq_ctx* c, Arena& A, const uint32_t* keys, const std::vector<rhccq_mbk_problem>& probs, const std::vector<const MbkDraws*>& draws,
                   const rhccq_fit::Totals& tot, ChainClocks* clk, uint32_t* flags = nullptr, uint32_t tag = 0, int32_t* published = nullptr) {
  const hipStream_t stream = c->stream;
  auto mark = [&](double ChainClocks::*t, bool sync) {
    if (!clk) return;
    if (sync && clk->sync) EF_HIP(hipStreamSynchronize(stream));
    clk->*t = now_ms();
  };
  const int32_t N = (int32_t)probs.size();
  const uint32_t* words;
  int64_t n_words;
  EF_RC(c, rhccq_mt_words(c, tot.words, &words, &n_words));
  mark(&ChainClocks::words, false);
  double* d_rand = (double*)A.alloc((size_t)tot.utot * 8);
  std::vector<int32_t> init_idx;
  init_idx.reserve((size_t)tot.itot);
  for (int32_t p = 0; p < N; ++p) {
    const MbkDraws& d = *draws[(size_t)p];
    EF_RC(c, rhccq_mt_uniforms(c, words, d.c.pos, d.c.n_uniforms, d_rand + probs[(size_t)p].rand_off));
    init_idx.insert(init_idx.end(), d.init_idx.begin(), d.init_idx.end());
  }
  int32_t* d_init = (int32_t*)A.alloc((size_t)tot.itot * 4);
  EF_HIP(hipMemcpyAsync(d_init, init_idx.data(), (size_t)tot.itot * 4, hipMemcpyHostToDevice, stream));   // pageable: staged on return
  mark(&ChainClocks::uploaded, true);
  const int64_t obytes = rhccq_mbk_order_bytes(tot.itot);
  void* otmp = A.alloc((size_t)obytes);
  int32_t* d_perm = (int32_t*)A.alloc((size_t)tot.itot * 4);
  EF_RC(c, rhccq_mbk_order(c, keys, probs.data(), N, d_init, d_perm, otmp, obytes));
  double* centres = (double*)A.alloc((size_t)tot.ktot * 4 * 8);
  int32_t* chosen = (int32_t*)A.alloc((size_t)tot.ktot * 4);
  EF_HIP(hipMemsetAsync(centres, 0, (size_t)tot.ktot * 4 * 8, stream));
  EF_HIP(hipMemsetAsync(chosen, 0, (size_t)tot.ktot * 4, stream));
  mark(&ChainClocks::ordered, true);
  if (flags) EF_RC(c, rhccq_mbk_init_released(c, keys, probs.data(), N, d_init, d_perm, d_rand, centres, chosen, flags, tag, published));
  else EF_RC(c, rhccq_mbk_init(c, keys, probs.data(), N, d_init, d_perm, d_rand, centres, chosen));
  mark(&ChainClocks::chained, true);
  return centres;
}

struct BatchFit {
  int64_t steps = 0;                                   // out: steps the problem ran
  int64_t overlapped_from = -1;                        // out: the step at which it went to the overlapped schedule (-1: never)
};

// The fit of 1 .. 32 problems on one lane and one stream.  probs: off / n / k set by the caller (key offsets into `keys`); labels_out at
// the key offsets.  Every problem keeps its own MT19937 positions, draws, init samples, T, first centre, step count and stopping rule;
// what a batch shares is the launches: one ordering, one chain launch, one step sequence (rhccq_fit::Plan: the first 16 steps classic,
// then chunks of 64 with every problem on the schedule its state asks for, masked out once it has stopped), one assignment.
// pre (one problem only): its chain ran in the frame's launch.  Nothing between the chain and the first steps waits on the host.
void mbk_fit(Lane& L, const uint32_t* keys, std::vector<rhccq_mbk_problem>& probs, int32_t* labels_out, std::vector<BatchFit>* fits = nullptr,
             const PreChain* pre = nullptr) {
  rhccq_ctx* c = L.ctx.get();
  const int N = (int)probs.size();
  if (N < 1 || N > rhccq_fit::kMaxProblems) throw Err{RHCCQ_E_ARG, "mbk_fit: 1 .. 32 problems"};
  if (pre && (N != 1 || pre->draws.c.n != probs[0].n || pre->draws.c.k != probs[0].k))
    throw Err{RHCCQ_E_ARG, "mbk_fit: the frame's chain was run for another problem"};
  const bool tr = trace_on();
  const double t0 = now_ms();
  std::vector<MbkDraws> own(pre ? 0 : (size_t)N);
  std::vector<const MbkDraws*> draws((size_t)N);
  std::vector<rhccq_fit::Problem> cs((size_t)N);
  rhccq_fit::Totals tot;
  for (int p = 0; p < N; ++p) {
    if (!pre) own[(size_t)p] = mbk_draws(probs[(size_t)p].n, probs[(size_t)p].k);
    draws[(size_t)p] = pre ? &pre->draws : &own[(size_t)p];
    cs[(size_t)p] = draws[(size_t)p]->c;
    tot.add(probs[(size_t)p], cs[(size_t)p]);
  }
  const double t_draws = now_ms();
  ChainClocks clk;
  double* centres;
  bool by_flag = false;
  if (pre) {                                                             // the frame's launch ran the chain: wait for it
    // RHCCQ_OPT_CHAIN_RELEASE: on the host, for this problem's flag or the launch's event, and queue nothing before -- a wait in the
    // stream would sit in a hardware queue that other lanes share until the LONGEST chain has ended.  Otherwise: the event, in the stream.
    if (pre->host_wait) by_flag = wait_for_chain(*pre) == rhccq_release::kByFlag;
    else EF_HIP(hipStreamWaitEvent(L.stream.get(), pre->done, 0));
    centres = pre->centres;
    if (tr) { L.sync(); clk.chained = now_ms(); }
  } else {
    centres = mbk_chains(c, L.arena, keys, probs, draws, tot, tr ? &clk : nullptr);
  }
  // ---- steps
  double* weights = L.dzeros<double>((size_t)tot.ktot);
  rhccq_fit::Plan plan(cs, tot.tiled());
  double* state = L.upload(plan.st.data(), plan.st.size());
  const int64_t wbytes = rhccq_mbk_work_bytes(probs.data(), N);
  void* work = L.arena.alloc((size_t)std::max<int64_t>(wbytes, 8));
  const int split = tot.split();
  const size_t snap = plan.st.size();
  double* landing = L.pinned.get();
  std::vector<int> pending;                                              // landing slots of the snapshots in flight
  int n_chunk = 0;
  int64_t step = 0;
  while (true) {
    const rhccq_fit::Chunk ch = plan.next(step);
    if (!ch.any() && pending.empty()) break;
    if (ch.any()) {
      const uint32_t* words;
      int64_t n_words;
      EF_RC(c, rhccq_mt_words(c, ch.need, &words, &n_words));
      if (step == 0 || !plan.tiled)                                      // (the first call writes the problem tables; the grid E-step: nobody is overlapped)
        EF_RC(c, rhccq_mbk_steps(c, keys, probs.data(), N, step, ch.ns, words, n_words, centres, weights, state, work, wbytes,
                                 (plan.tiled ? RHCCQ_ESTEP_TILES : RHCCQ_ESTEP_GRID) | (ch.no_reassign ? RHCCQ_STEPS_NO_REASSIGN : 0), split));
      else
        EF_RC(c, rhccq_mbk_steps_batch(c, keys, probs.data(), N, step, ch.ns, words, n_words, centres, weights, state, work, wbytes, split, ch.fast_mask,
                                       ch.classic_mask, ch.no_reassign ? 1 : 0, plan.since.data(), plan.carry.data()));
      plan.advance(ch);
      step += ch.ns;
      const int slot = n_chunk % 3;
      ++n_chunk;
      EF_HIP(hipMemcpyAsync(landing + (size_t)slot * snap, state, snap * sizeof(double), hipMemcpyDeviceToHost, L.stream.get()));
      EF_HIP(hipEventRecord(L.ev[slot].get(), L.stream.get()));
      pending.push_back(slot);
    }
    if (ch.classic_mask) {                                               // a classic problem's next chunk depends on its state: wait for the newest
      EF_HIP(hipEventSynchronize(L.ev[pending.back()].get()));
      plan.take(landing + (size_t)pending.back() * snap);
      pending.clear();
    } else if (pending.size() >= 2 || !ch.any()) {                       // overlapped problems only: the state two chunks behind
      EF_HIP(hipEventSynchronize(L.ev[pending.front()].get()));
      plan.take(landing + (size_t)pending.front() * snap);
      pending.erase(pending.begin());
    }
    if (const char* e = plan.error()) throw Err{RHCCQ_E_LIMIT, e};
  }
  if (fits) {
    fits->assign((size_t)N, BatchFit());
    for (int p = 0; p < N; ++p) (*fits)[(size_t)p] = BatchFit{plan.view(p).steps_done(), plan.overlapped_from[(size_t)p]};
  }
  double t_steps = 0;
  if (tr) { L.sync(); t_steps = now_ms(); }
  EF_RC(c, rhccq_mbk_assign(c, keys, probs.data(), N, centres, work, wbytes, labels_out));
  if (!tr) return;
  L.sync();
  const double t_assign = now_ms();
  const long long n0 = (long long)probs[0].n, k0 = (long long)probs[0].k, steps0 = (long long)plan.view(0).steps_done();
  if (pre) {
    fprintf(stderr, "[rhccq] mbk n=%lld k=%lld: chain in the frame's launch, waited %.2f ms for it (%s), %lld steps %.2f ms, assign %.2f ms\n", n0, k0,
            clk.chained - t0, by_flag ? "its own flag" : "the launch's event", steps0, t_steps - clk.chained, t_assign - t_steps);
  } else if (N == 1) {
    fprintf(stderr, "[rhccq] mbk n=%lld k=%lld: draws+order %.2f ms (host draws %.2f, word table %.2f, uniforms+upload %.2f, order %.2f), chain %.2f ms "
            "(%.2f us/pick), %lld steps %.2f ms, assign %.2f ms\n", n0, k0, clk.ordered - t0, t_draws - t0, clk.words - t_draws, clk.uploaded - clk.words,
            clk.ordered - clk.uploaded, clk.chained - clk.ordered, (clk.chained - clk.ordered) * 1e3 / (double)k0, steps0, t_steps - clk.chained,
            t_assign - t_steps);
  } else {
    std::string names;
    for (int p = 0; p < N; ++p) {
      char buf[96];
      snprintf(buf, sizeof(buf), "%s n=%lld k=%lld %lld steps%s", p ? "," : "", (long long)probs[(size_t)p].n, (long long)probs[(size_t)p].k,
               (long long)plan.view(p).steps_done(), plan.overlapped_from[(size_t)p] >= 0 ? " (overlapped)" : "");
      names += buf;
    }
    fprintf(stderr, "[rhccq] mbk batch of %d:%s: draws+order %.2f ms, chains %.2f ms, steps %.2f ms (%d chunks), assign %.2f ms\n", N, names.c_str(),
            clk.ordered - t0, clk.chained - clk.ordered, t_steps - clk.chained, n_chunk, t_assign - t_steps);
  }
}

// ---- cluster_palette_colors_parallel for a list of palettes (palette.py::cluster_palettes) ------------------------------------
struct Job {
  // in
  const uint32_t* keys_dev = nullptr;                  // resident sorted palette (MiniBatch branch of level 1), or
  std::vector<uint32_t> keys;                          // the palette on the host (palette order)
  int64_t P = 0;
  bool has_black = false;                              // resident palettes: black sits at index 0
  int quality = 0;
  double eps = 0.0;
  int64_t mc = 0;
  int32_t* lut_dev = nullptr;                          // where base + mapping goes on the device (level 1), or NULL
  int32_t base = 0;                                    // added to the mapping when it is written to lut_dev
  // out
  std::vector<uint32_t> new_keys;
  std::vector<int32_t> mapping;                        // host mapping (uint16-valued), empty for a resident job that stayed resident
  bool wrapped = false;                                // more than 65 536 entries: the reference's uint16 mapping_array wraps
  // work
  std::vector<int32_t> nb;                             // indices of the non-black rows
  std::vector<int32_t> labels;
  bool have_labels = false;
  int32_t* labels_dev = nullptr;
  int64_t k = 0;
  const PreChain* pre = nullptr;                       // its k-means++ chain ran in the frame's launch (resident level-1 jobs)
  int64_t mbk_n = 0, mbk_steps = -1;                   // out (MiniBatchKMeans branch): points, steps run
  int mbk_schedule = 0;                                // out: Level2Fit::schedule
  int64_t mbk_overlapped_from = -1;                    // out: Level2Fit::overlapped_from
};

int64_t n_splits(int64_t n, int64_t mc) {             // split_large_cluster's n_splits (clustering.py:739-747); 0 = do not split
  if (n <= mc) return 0;
  int64_t ns = std::max<int64_t>(2, (n + mc - 1) / mc);
  ns = std::min(ns, n);
  if (n <= 2 || ns < 2) return 0;
  return ns;
}

int64_t mbk_k(int64_t n, int q) { return (int64_t)std::ceil((double)n * ((double)q / 100.0) / 10.0); }   // clustering.py:210

struct Node {
  int job;
  std::vector<int32_t> members;                        // positions in the job's non-black list, ascending
  std::vector<int> children;
  bool split = false;
};

void run_mbk_tasks(Lane& L, std::vector<Job*>& tasks) {
  // every problem a pipeline of its own: host thread + sibling context (stream), as ops.py::_minibatch_lanes
  if (tasks.empty()) return;
  const Event ready = make_event();
  EF_HIP(hipEventRecord(ready.get(), L.stream.get()));
  const size_t n_lanes = std::min<size_t>(tasks.size(), 8);
  for (size_t i = 0; i < n_lanes; ++i) L.sublane(i);   // (created here: the vector must not grow under the threads)
  // longest chains first, each to the lane with the least work so far
  std::vector<size_t> order(tasks.size());
  for (size_t i = 0; i < order.size(); ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return tasks[a]->k > tasks[b]->k; });
  std::vector<std::vector<size_t>> groups(n_lanes);
  std::vector<int64_t> load(n_lanes, 0);
  for (size_t i : order) {
    const size_t g = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
    groups[g].push_back(i);
    load[g] += tasks[i]->k;
  }
  // RHCCQ_OPT_CHAIN_RELEASE: a lane takes its problems of the frame's chain launch as their chains end, shortest chain first, and behind
  // them the problems that run their own chain on the lane (nothing holds those up).  Same results: the problems are independent.
  for (auto& grp : groups)
    std::stable_sort(grp.begin(), grp.end(), [&](size_t a, size_t b) {
      const bool ra = tasks[a]->pre && tasks[a]->pre->host_wait, rb = tasks[b]->pre && tasks[b]->pre->host_wait;
      if (ra != rb) return ra;
      return ra && tasks[a]->k < tasks[b]->k;
    });
  run_lanes(
      n_lanes,
      [&](size_t g) {
        Lane& S = *L.sub[g];
        EF_HIP(hipSetDevice(S.device));
        EF_HIP(hipStreamWaitEvent(S.stream.get(), ready.get(), 0));
        for (size_t i : groups[g]) {
          Job& jb = *tasks[i];
          const uint32_t* keys;
          int64_t n;
          if (jb.keys_dev) {
            keys = jb.keys_dev + (jb.has_black ? 1 : 0);
            n = jb.P - (jb.has_black ? 1 : 0);
          } else {
            std::vector<uint32_t> nbk(jb.nb.size());
            for (size_t t = 0; t < nbk.size(); ++t) nbk[t] = jb.keys[(size_t)jb.nb[t]];
            keys = S.upload(nbk.data(), nbk.size());
            S.sync();                                   // (the staging vector dies here)
            n = (int64_t)nbk.size();
          }
          jb.labels_dev = S.dalloc<int32_t>((size_t)n);
          std::vector<rhccq_mbk_problem> prob(1);
          prob[0].off = 0; prob[0].n = n; prob[0].k = jb.k;
          mbk_fit(S, keys, prob, jb.labels_dev, nullptr, jb.pre);
        }
        S.sync();
      },
      [&](size_t g) { (void)hipStreamSynchronize(L.sub[g]->stream.get()); });
}

// The MiniBatchKMeans problems of `tasks` as batches of at most 32 on L's own stream (mbk_fit); a batch of one reports as a lone fit.
// Host palettes only (the level-2 stage's): their non-black keys go to the device in one copy.
void run_mbk_batch(Lane& L, std::vector<Job*>& tasks) {
  for (size_t lo = 0; lo < tasks.size(); lo += 32) {
    const size_t hi = std::min(tasks.size(), lo + 32);
    std::vector<rhccq_mbk_problem> probs(hi - lo);
    std::vector<uint32_t> cat;
    for (size_t i = lo; i < hi; ++i) {
      Job& jb = *tasks[i];
      rhccq_mbk_problem& q = probs[i - lo];
      q = rhccq_mbk_problem();
      q.off = (int64_t)cat.size(); q.n = (int64_t)jb.nb.size(); q.k = jb.k;
      for (int32_t t : jb.nb) cat.push_back(jb.keys[(size_t)t]);
      jb.mbk_n = q.n;
    }
    const uint32_t* keys = L.upload(cat.data(), cat.size());
    L.sync();                                           // (`cat` is staged)
    int32_t* labels = L.dalloc<int32_t>(cat.size());
    std::vector<BatchFit> fits;
    mbk_fit(L, keys, probs, labels, &fits);
    const bool lone = probs.size() == 1;
    for (size_t i = lo; i < hi; ++i) {
      Job& jb = *tasks[i];
      jb.labels_dev = labels + probs[i - lo].off;
      jb.mbk_steps = fits[i - lo].steps;
      jb.mbk_schedule = lone ? 0 : fits[i - lo].overlapped_from >= 0 ? 2 : 1;
      jb.mbk_overlapped_from = lone ? -1 : fits[i - lo].overlapped_from;
    }
    L.sync();
  }
}

// batch_mbk: the MiniBatchKMeans problems of host palettes run as one batch on L's own stream (run_mbk_batch) instead of side by side
// on sibling lanes
void cluster_jobs(Lane& L, std::vector<Job>& jobs, bool batch_mbk = false) {
  rhccq_ctx* c = L.ctx.get();
  const size_t S = jobs.size();
  // ---- which branch: resident MiniBatch jobs, host MiniBatch jobs, DBSCAN jobs, only-black palettes
  std::vector<Job*> mbk;
  std::vector<size_t> db;
  for (size_t s = 0; s < S; ++s) {
    Job& jb = jobs[s];
    if (jb.keys_dev) {
      const int64_t n = jb.P - (jb.has_black ? 1 : 0);
      jb.k = mbk_k(n, jb.quality);
      mbk.push_back(&jb);
      continue;
    }
    jb.nb.clear();
    for (int64_t i = 0; i < jb.P; ++i)
      if (jb.keys[(size_t)i] != 0u) jb.nb.push_back((int32_t)i);
    const int64_t n = (int64_t)jb.nb.size();
    if (n == 0) continue;
    if (n >= kMinibatchThreshold) {
      jb.k = mbk_k(n, jb.quality);
      mbk.push_back(&jb);
    } else {
      db.push_back(s);
    }
  }
  // ---- DBSCAN(eps / 255, min_samples = 1) labels of all small palettes in one launch (clustering.py:233-235)
  const double t_db = now_ms();
  if (!db.empty()) {
    std::vector<int32_t> desc(db.size() * 4);
    std::vector<double> r2(db.size());
    std::vector<uint32_t> cat;
    int32_t max_n = 0;
    for (size_t i = 0; i < db.size(); ++i) {
      Job& jb = jobs[db[i]];
      int32_t thr, bnd;
      double rr;
      if (rhccq_eps_threshold(jb.eps, &thr, &bnd, &rr)) throw Err{RHCCQ_E_ARG, "rhccq_eps_threshold failed"};
      desc[4 * i] = (int32_t)cat.size();
      desc[4 * i + 1] = (int32_t)jb.nb.size();
      desc[4 * i + 2] = thr;
      desc[4 * i + 3] = bnd;
      r2[i] = rr;
      max_n = std::max<int32_t>(max_n, (int32_t)jb.nb.size());
      for (int32_t t : jb.nb) cat.push_back(jb.keys[(size_t)t]);
    }
    uint32_t* d_keys = L.upload(cat.data(), cat.size());
    int32_t* d_desc = L.upload(desc.data(), desc.size());
    double* d_r2 = L.upload(r2.data(), r2.size());
    int32_t* d_lab = L.dalloc<int32_t>(cat.size());
    int32_t* d_nc = L.dalloc<int32_t>(db.size());
    EF_RC(c, rhccq_eps_components(c, d_keys, d_desc, d_r2, (int32_t)db.size(), max_n, d_lab, d_nc));
    std::vector<int32_t> lab(cat.size());
    L.download(lab.data(), d_lab, lab.size());
    for (size_t i = 0; i < db.size(); ++i) {
      Job& jb = jobs[db[i]];
      jb.labels.assign(lab.begin() + desc[4 * i], lab.begin() + desc[4 * i] + desc[4 * i + 1]);
      jb.have_labels = true;
    }
  }
  if (trace_on() && !db.empty()) fprintf(stderr, "[rhccq] dbscan: %zu palettes, %.2f ms\n", db.size(), now_ms() - t_db);
  // ---- MiniBatchKMeans problems: side by side, or (the frame's level-2 stage) the host palettes as one batch
  if (batch_mbk) {
    std::vector<Job*> host_jobs, resident;
    for (Job* pj : mbk) (pj->keys_dev ? resident : host_jobs).push_back(pj);
    run_mbk_batch(L, host_jobs);
    run_mbk_tasks(L, resident);
  } else {
    run_mbk_tasks(L, mbk);
  }
  for (Job* pj : mbk) {
    Job& jb = *pj;
    if (jb.keys_dev) {
      // resident: member sums -> floor means of the non-empty clusters in label order + the uint16 mapping (one native pass);
      // only k-sized tables cross PCIe.  A cluster above mc needs the k-means split: the job goes to the host path with its labels
      const int64_t n = jb.P - (jb.has_black ? 1 : 0);
      const int32_t nblack = jb.has_black ? 1 : 0;
      unsigned long long* d_sums = L.dzeros<unsigned long long>((size_t)jb.k * 4);
      EF_RC(c, rhccq_cluster_sums(c, jb.keys_dev + nblack, jb.labels_dev, n, jb.k, d_sums));
      std::vector<unsigned long long> sums((size_t)jb.k * 4);
      L.download(sums.data(), d_sums, sums.size());
      std::vector<uint32_t> nk((size_t)(nblack + jb.k));
      std::vector<int32_t> lut((size_t)jb.k);
      const int64_t n_present = rhccq_cluster_plan_host(sums.data(), jb.k, jb.mc, nblack, nk.data(), lut.data());
      if (n_present == -1) {
        jb.keys.resize((size_t)jb.P);
        L.download(jb.keys.data(), jb.keys_dev, (size_t)jb.P);
        jb.labels.resize((size_t)n);
        L.download(jb.labels.data(), jb.labels_dev, (size_t)n);
        jb.have_labels = true;
        jb.keys_dev = nullptr;
        jb.nb.clear();
        for (int64_t i = 0; i < jb.P; ++i)
          if (jb.keys[(size_t)i] != 0u) jb.nb.push_back((int32_t)i);
        continue;
      }
      if (n_present < 0) throw Err{RHCCQ_E_ARG, "rhccq_cluster_plan_host: bad argument"};
      nk.resize((size_t)(nblack + n_present));
      jb.new_keys = nk;
      jb.wrapped = nblack + n_present > 65536;
      if (jb.lut_dev) {
        for (auto& v : lut) v += jb.base;
        int32_t* d_lut = L.upload(lut.data(), lut.size());
        EF_RC(c, rhccq_remap(c, jb.labels_dev, n, d_lut, jb.k, jb.lut_dev + nblack));
        if (nblack) EF_HIP(hipMemcpyAsync(jb.lut_dev, &jb.base, 4, hipMemcpyHostToDevice, L.stream.get()));
        L.sync();                                       // (`lut` is staged: it may die now)
      } else {
        std::vector<int32_t> lab((size_t)n);
        L.download(lab.data(), jb.labels_dev, (size_t)n);
        jb.mapping.assign((size_t)jb.P, 0);
        for (int64_t i = 0; i < n; ++i) jb.mapping[(size_t)(i + nblack)] = lut[(size_t)lab[(size_t)i]];
      }
    } else {
      jb.labels.resize(jb.nb.size());
      L.download(jb.labels.data(), jb.labels_dev, jb.labels.size());
      jb.have_labels = true;
    }
  }
  // ---- classify the clusters, build the split trees of the oversize ones (breadth first on the device, depth-first output order)
  std::vector<Node> nodes;
  std::vector<std::vector<int>> larges(S);
  std::vector<std::vector<int32_t>> small_leaf(S);
  std::vector<int32_t> n_small(S, 0);
  std::vector<int> frontier;
  for (size_t s = 0; s < S; ++s) {
    Job& jb = jobs[s];
    if (!jb.have_labels) continue;
    int32_t nl = 0;
    for (int32_t v : jb.labels) nl = std::max(nl, v + 1);
    std::vector<int64_t> cnt((size_t)nl, 0);
    for (int32_t v : jb.labels) cnt[(size_t)v]++;
    small_leaf[s].assign((size_t)nl, -1);
    std::vector<int> node_of((size_t)nl, -1);
    for (int32_t l = 0; l < nl; ++l) {
      if (cnt[(size_t)l] == 0) continue;
      if (cnt[(size_t)l] > jb.mc) {
        node_of[(size_t)l] = (int)nodes.size();
        larges[s].push_back((int)nodes.size());
        nodes.push_back(Node{(int)s, {}, {}, false});
        nodes.back().members.reserve((size_t)cnt[(size_t)l]);
      } else {
        small_leaf[s][(size_t)l] = n_small[s]++;         // ascending label order
      }
    }
    if (!larges[s].empty())
      for (size_t i = 0; i < jb.labels.size(); ++i) {
        const int nd = node_of[(size_t)jb.labels[i]];
        if (nd >= 0) nodes[(size_t)nd].members.push_back((int32_t)i);   // ascending index inside
      }
    for (int nd : larges[s]) frontier.push_back(nd);
  }
  const double u0 = rhccq_mt::Words::get().dbl(0);              // RandomState(42).random_sample()[0]: the first centre's draw of every KMeans fit
  while (!frontier.empty()) {
    std::vector<std::pair<int, int64_t>> run;
    for (int nd : frontier) {
      const int64_t k = n_splits((int64_t)nodes[(size_t)nd].members.size(), jobs[(size_t)nodes[(size_t)nd].job].mc);
      if (k > 0) run.emplace_back(nd, k);
    }
    frontier.clear();
    if (run.empty()) break;
    // KMeans(k, random_state=42).fit_predict of every node of this level in one launch (clustering.py:751-752)
    std::vector<int32_t> desc(run.size() * 6);
    std::vector<int64_t> koff(run.size());
    std::vector<uint32_t> cat;
    int64_t ktot = 0, need = 1;
    int32_t max_n = 0;
    for (size_t i = 0; i < run.size(); ++i) {
      const Node& nd = nodes[(size_t)run[i].first];
      const Job& jb = jobs[(size_t)nd.job];
      const int64_t n = (int64_t)nd.members.size(), k = run[i].second;
      const int T = 2 + (int)std::log((double)k);
      desc[6 * i] = (int32_t)cat.size();
      desc[6 * i + 1] = (int32_t)n;
      desc[6 * i + 2] = (int32_t)k;
      desc[6 * i + 3] = 0;
      desc[6 * i + 4] = first_centre_index(n, u0);
      desc[6 * i + 5] = T;
      koff[i] = ktot;
      ktot += k;
      need = std::max<int64_t>(need, (k - 1) * T);
      max_n = std::max<int32_t>(max_n, (int32_t)n);
      for (int32_t m : nd.members) cat.push_back(jb.keys[(size_t)jb.nb[(size_t)m]]);
    }
    const uint32_t* words;
    int64_t n_words;
    EF_RC(c, rhccq_mt_words(c, 2 + 2 * need, &words, &n_words));
    double* d_rand = L.dalloc<double>((size_t)need);
    EF_RC(c, rhccq_mt_uniforms(c, words, 2, need, d_rand));             // the doubles behind u0
    uint32_t* d_keys = L.upload(cat.data(), cat.size());
    int32_t* d_desc = L.upload(desc.data(), desc.size());
    int64_t* d_koff = L.upload(koff.data(), koff.size());
    double* work = L.dalloc<double>((size_t)(8 * ktot + 8));
    int32_t* d_lab = L.dalloc<int32_t>(cat.size());
    int32_t* d_info = L.dzeros<int32_t>(run.size() * 4);
    const double t_km = now_ms();
    EF_RC(c, rhccq_kmeans(c, d_keys, d_desc, d_koff, d_rand, (int32_t)run.size(), max_n, work, d_lab, d_info));
    std::vector<int32_t> lab(cat.size());
    L.download(lab.data(), d_lab, lab.size());
    if (trace_on()) {
      std::vector<int32_t> inf(run.size() * 4);
      L.download(inf.data(), d_info, inf.size());
      int it_max = 0, n_wide = 0;
      for (size_t i = 0; i < run.size(); ++i) {
        it_max = std::max(it_max, inf[4 * i]);
        n_wide += inf[4 * i + 3] == 1;                   // rhccq_kmeans: the wide Lloyd path
      }
      fprintf(stderr, "[rhccq] kmeans split round: %zu nodes (%d wide), %zu points, largest %d, %lld clusters, %.2f ms, most Lloyd iterations %d (node 0: %d)\n",
              run.size(), n_wide, cat.size(), max_n, (long long)ktot, now_ms() - t_km, it_max, inf[0]);
    }
    for (size_t i = 0; i < run.size(); ++i) {
      const int ndi = run[i].first;
      const int64_t k = run[i].second;
      const int32_t* l = lab.data() + desc[6 * i];
      const size_t n = nodes[(size_t)ndi].members.size();
      std::vector<int> child_of((size_t)k, -1);
      std::vector<int64_t> cc((size_t)k, 0);
      for (size_t t = 0; t < n; ++t) cc[(size_t)l[t]]++;
      nodes[(size_t)ndi].split = true;
      for (int64_t q = 0; q < k; ++q) {                                 // children in ascending label order; empty labels give none
        if (!cc[(size_t)q]) continue;
        child_of[(size_t)q] = (int)nodes.size();
        nodes.push_back(Node{nodes[(size_t)ndi].job, {}, {}, false});
        nodes.back().members.reserve((size_t)cc[(size_t)q]);
        nodes[(size_t)ndi].children.push_back(child_of[(size_t)q]);
      }
      for (size_t t = 0; t < n; ++t) nodes[(size_t)child_of[(size_t)l[t]]].members.push_back(nodes[(size_t)ndi].members[t]);
      const int64_t mc = jobs[(size_t)nodes[(size_t)ndi].job].mc;
      for (int ch : nodes[(size_t)ndi].children) {
        const int64_t cn = (int64_t)nodes[(size_t)ch].members.size();
        if (cn > mc && n_splits(cn, mc) > 0) frontier.push_back(ch);
      }
    }
  }
  // ---- leaves in reference order, floor means (np.mean(...).astype(uint8) == integer floor division of the channel sums,
  // clustering.py:305,347), the old -> new table stored as uint16 (clustering.py:373)
  for (size_t s = 0; s < S; ++s) {
    Job& jb = jobs[s];
    if (jb.keys_dev && !jb.new_keys.empty()) continue;   // stayed resident
    if (jb.keys_dev) continue;
    if (!jb.have_labels) {                               // only black (or empty): returned unchanged (clustering.py:197-199)
      jb.new_keys = jb.keys;
      jb.mapping.resize((size_t)jb.P);
      for (int64_t i = 0; i < jb.P; ++i) jb.mapping[(size_t)i] = (int32_t)i;
      if (jb.lut_dev && jb.P) {
        std::vector<int32_t> m(jb.mapping);
        for (auto& v : m) v += jb.base;
        EF_HIP(hipMemcpyAsync(jb.lut_dev, m.data(), m.size() * 4, hipMemcpyHostToDevice, L.stream.get()));
        L.sync();
      }
      continue;
    }
    std::vector<int32_t> leaf_of(jb.nb.size());
    for (size_t i = 0; i < leaf_of.size(); ++i) leaf_of[i] = small_leaf[s][(size_t)jb.labels[i]];
    int32_t n_leaves = n_small[s];
    std::vector<int> stack;
    for (int root : larges[s]) {                         // ascending label; each contributes its children depth first
      stack.assign(1, root);
      while (!stack.empty()) {
        const int nd = stack.back();
        stack.pop_back();
        if (!nodes[(size_t)nd].split) {
          for (int32_t m : nodes[(size_t)nd].members) leaf_of[(size_t)m] = n_leaves;
          ++n_leaves;
        } else {
          for (auto it = nodes[(size_t)nd].children.rbegin(); it != nodes[(size_t)nd].children.rend(); ++it) stack.push_back(*it);
        }
      }
    }
    std::vector<uint64_t> sums((size_t)n_leaves * 4, 0);
    for (size_t i = 0; i < leaf_of.size(); ++i) {
      const uint32_t kk = jb.keys[(size_t)jb.nb[i]];
      uint64_t* a = &sums[(size_t)leaf_of[i] * 4];
      a[0] += (kk >> 16) & 255u;
      a[1] += (kk >> 8) & 255u;
      a[2] += kk & 255u;
      a[3] += 1;
    }
    int32_t nblack = 0;
    for (int64_t i = 0; i < jb.P; ++i) nblack += jb.keys[(size_t)i] == 0u;
    jb.new_keys.assign((size_t)(nblack + n_leaves), 0u);
    for (int32_t l = 0; l < n_leaves; ++l) {
      const uint64_t* a = &sums[(size_t)l * 4];
      const uint64_t cn = std::max<uint64_t>(a[3], 1);
      jb.new_keys[(size_t)(nblack + l)] = ((uint32_t)(a[0] / cn) << 16) | ((uint32_t)(a[1] / cn) << 8) | (uint32_t)(a[2] / cn);
    }
    jb.mapping.assign((size_t)jb.P, 0);
    int32_t b = 0;
    for (int64_t i = 0; i < jb.P; ++i)
      if (jb.keys[(size_t)i] == 0u) jb.mapping[(size_t)i] = b++;
    for (size_t i = 0; i < leaf_of.size(); ++i) jb.mapping[(size_t)jb.nb[i]] = (nblack + leaf_of[i]) & 0xFFFF;
    jb.wrapped = nblack + n_leaves > 65536;
    if (jb.lut_dev) {
      std::vector<int32_t> m(jb.mapping);
      for (auto& v : m) v += jb.base;
      EF_HIP(hipMemcpyAsync(jb.lut_dev, m.data(), m.size() * 4, hipMemcpyHostToDevice, L.stream.get()));
      L.sync();
    }
  }
}

// ---- components of the hierarchy in palette space (frame.py::_Comp, _merge, level2_finish) ------------------------------------
struct Comp {
  std::vector<uint32_t> keys;                          // palette keys (palette order)
  std::vector<int64_t> fp;                             // first absolute raster position showing the entry
  int32_t top_left[2] = {0, 0};
  int32_t shape[2] = {0, 0};
  std::map<int, std::vector<int32_t>> maps;            // job -> (index in the job's CLUSTERED level-1 palette -> index into keys)
  bool merged = false;                                 // canvas semantics (index 0 = black = uncovered)
};

// merge_region_components_simple in palette space (merging.py:8-120): one component is returned as it is (:16-21)
std::shared_ptr<Comp> merge_comps(const std::vector<std::shared_ptr<Comp>>& comps, int32_t minr, int32_t minc, int32_t maxr, int32_t maxc) {
  if (comps.empty()) return nullptr;
  if (comps.size() == 1) return comps[0];
  const int n = (int)comps.size();
  std::vector<const uint32_t*> pk((size_t)n);
  std::vector<const int64_t*> pf((size_t)n);
  std::vector<std::vector<int32_t>> luts((size_t)n);
  std::vector<int32_t*> pl((size_t)n);
  std::vector<int32_t> counts((size_t)n);
  size_t total = 0;
  static const uint32_t dummy_k = 0;
  static const int64_t dummy_f = 0;
  for (int i = 0; i < n; ++i) {
    counts[(size_t)i] = (int32_t)comps[(size_t)i]->keys.size();
    luts[(size_t)i].resize(std::max<size_t>(comps[(size_t)i]->keys.size(), 1));
    pk[(size_t)i] = counts[(size_t)i] ? comps[(size_t)i]->keys.data() : &dummy_k;
    pf[(size_t)i] = counts[(size_t)i] ? comps[(size_t)i]->fp.data() : &dummy_f;
    pl[(size_t)i] = luts[(size_t)i].data();
    total += (size_t)counts[(size_t)i];
  }
  std::vector<uint32_t> gkeys(total + 1);
  std::vector<int64_t> gfp(total + 1);
  int64_t n_out = 0;
  const int rc = rhccq_merge_palettes_host(n, pk.data(), pf.data(), counts.data(), kFpNone, gkeys.data(), gfp.data(), pl.data(), &n_out);
  if (rc) throw Err{rc, "rhccq_merge_palettes_host failed"};
  auto out = std::make_shared<Comp>();
  out->keys.assign(gkeys.begin(), gkeys.begin() + n_out);
  out->fp.assign(gfp.begin(), gfp.begin() + n_out);
  for (int i = 0; i < n; ++i)
    for (const auto& kv : comps[(size_t)i]->maps) {
      std::vector<int32_t> m(kv.second.size());
      for (size_t t = 0; t < m.size(); ++t) m[t] = luts[(size_t)i][(size_t)kv.second[t]];
      out->maps[kv.first] = std::move(m);
    }
  out->top_left[0] = minr; out->top_left[1] = minc;
  out->shape[0] = maxr - minr; out->shape[1] = maxc - minc;
  out->merged = true;
  return out;
}

// a clustered component: new palette, first positions carried through the mapping (scatter-min), job maps composed
std::shared_ptr<Comp> clustered(const Comp& comp, const Job& jb) {
  auto out = std::make_shared<Comp>();
  out->keys = jb.new_keys;
  out->fp.assign(jb.new_keys.size(), kFpNone);
  if (!jb.mapping.empty())
    if (rhccq_scatter_min_host((int64_t)out->fp.size(), jb.mapping.data(), comp.fp.data(), (int64_t)jb.mapping.size(), out->fp.data()))
      throw Err{RHCCQ_E_ARG, "rhccq_scatter_min_host: index outside the table"};
  for (const auto& kv : comp.maps) {
    std::vector<int32_t> m(kv.second.size());
    for (size_t t = 0; t < m.size(); ++t) m[t] = jb.mapping[(size_t)kv.second[t]];
    out->maps[kv.first] = std::move(m);
  }
  std::memcpy(out->top_left, comp.top_left, sizeof(out->top_left));
  std::memcpy(out->shape, comp.shape, sizeof(out->shape));
  out->merged = comp.merged;
  return out;
}

struct FrameCtx {
  rhccq_ctx* root;
  const uint8_t* rgb;
  int32_t H, W;
  const rhccq_class_desc* classes;
  int32_t n_classes;
  std::vector<int32_t> job_base;                       // [n_classes + 1]
  int32_t n_jobs;
  std::vector<int64_t> P, pal_off;                     // palette sizes, offsets ([n_jobs + 1])
  std::vector<uint8_t> present, has_black;
  std::vector<int32_t> job_class, job_region;
  std::vector<int64_t> r0, r1, c0, c1;
  uint32_t* bitmaps = nullptr;
  uint32_t* prefix = nullptr;
  uint32_t* keys_dev = nullptr;
  int64_t* d_pal_off = nullptr;
  uint32_t* fix_key = nullptr;
  int32_t* lut1 = nullptr;                             // (job, rank) -> frame-wide entry id of the clustered level-1 palettes
  int32_t* e1map = nullptr;                            // [n_classes][H * W] entry every pixel shows
  std::vector<int64_t> ebase;                          // first entry id of a class's slice (= palette entries of the classes before)
  Event ready;
  std::map<int, PreChain> pre;                         // job -> its level-1 chain in the frame's launch (RHCCQ_OPT_FRAME_CHAINS)
  Event chains_done;
};

struct ClassOut {
  std::map<int, std::pair<int64_t, int64_t>> k1_off;   // job -> [first entry id, end)
  std::shared_ptr<Comp> comp2;                         // the class's merged component (NULL: the class has no component) and
  Job job2;                                            // its level-2 job: what the class thread hands to the level-2 stage
  std::shared_ptr<Comp> comp3;                         // the class's level-2 result (NULL: the class contributes nothing)
  int q2 = 0;
  double ms[4] = {0, 0, 0, 0};
  Event done;
};

// level 2 of the classes `cis` in one clustering call on lane L (one class: that class's own lane, RHCCQ_OPT_FRAME_LEVEL2 = 0; all
// classes with a component: the frame's level-2 stage).  The call's time is reported as level2_cluster of every class it served.
void level2_stage(Lane& L, std::vector<ClassOut>& outs, const std::vector<int>& cis, bool batch_mbk, std::vector<Level2Fit>* fits) {
  level2_handover<Job>(
      outs, cis, [&](std::vector<Job>& j2) { cluster_jobs(L, j2, batch_mbk); },
      [&](int ci, ClassOut& out, const Job& jb) {
        out.comp3 = clustered(*out.comp2, jb);
        if (fits && jb.mbk_steps >= 0) {
          Level2Fit f;
          f.cls = ci; f.n = jb.mbk_n; f.k = jb.k; f.steps = jb.mbk_steps; f.schedule = jb.mbk_schedule; f.overlapped_from = jb.mbk_overlapped_from;
          fits->push_back(f);
        }
      },
      now_ms);
}

// level 1 -> merge per region -> merge per class of one class on its own lane (frame.py::_class_pipeline); with level2_here also the
// class's level 2, on the same lane
void class_pipeline(FrameCtx& F, int ci, Lane& L, std::vector<ClassOut>& outs, bool level2_here) {
  ClassOut& out = outs[(size_t)ci];
  rhccq_ctx* c = L.ctx.get();
  EF_HIP(hipSetDevice(L.device));
  EF_HIP(hipStreamWaitEvent(L.stream.get(), F.ready.get(), 0));
  double t_prev = now_ms();
  auto mark = [&](int slot) {
    const double t = now_ms();
    out.ms[slot] += t - t_prev;
    t_prev = t;
  };
  const rhccq_class_desc& cls = F.classes[ci];
  const int jb0 = F.job_base[(size_t)ci], jb1 = F.job_base[(size_t)ci + 1];
  // ---- level-1 jobs (subregions.py:426-449): palettes of >= 10 000 colours stay in HBM, the small ones come to the host in ONE copy
  std::vector<int> ids;
  for (int j = jb0; j < jb1; ++j)
    if (F.present[(size_t)j]) ids.push_back(j);
  std::vector<Job> jobs(ids.size());
  int small_lo = -1, small_hi = -1;
  for (size_t i = 0; i < ids.size(); ++i) {
    const int j = ids[i];
    const bool big = F.P[(size_t)j] - (F.has_black[(size_t)j] ? 1 : 0) >= kMinibatchThreshold;
    if (!big) {
      if (small_lo < 0) small_lo = j;
      small_hi = j;
    }
  }
  std::vector<uint32_t> chunk;
  if (small_lo >= 0) {
    chunk.resize((size_t)(F.pal_off[(size_t)small_hi + 1] - F.pal_off[(size_t)small_lo]));
    L.download(chunk.data(), F.keys_dev + F.pal_off[(size_t)small_lo], chunk.size());
  }
  for (size_t i = 0; i < ids.size(); ++i) {
    const int j = ids[i];
    Job& jb = jobs[i];
    jb.P = F.P[(size_t)j];
    jb.quality = cls.quality;
    if (rhccq_params(jb.P, (double)cls.quality, &jb.eps, &jb.mc)) throw Err{RHCCQ_E_ARG, "rhccq_params: quality 0 divides by zero (clustering.py:129)"};
    const bool big = jb.P - (F.has_black[(size_t)j] ? 1 : 0) >= kMinibatchThreshold;
    if (big) {
      jb.keys_dev = F.keys_dev + F.pal_off[(size_t)j];
      jb.has_black = F.has_black[(size_t)j] != 0;
      const auto it = F.pre.find(j);
      if (it != F.pre.end()) jb.pre = &it->second;
    } else {
      const size_t a = (size_t)(F.pal_off[(size_t)j] - F.pal_off[(size_t)small_lo]);
      jb.keys.assign(chunk.begin() + a, chunk.begin() + a + (size_t)jb.P);
    }
  }
  // entry ids: a job's clustered palette never has more entries than the palette itself, so the job's slice of the frame-wide id
  // space starts at ebase[class] + (palette entries of the class's jobs before it) -- known BEFORE the clustering, which lets the
  // device-resident mappings be written straight into lut1 (frame.py reserves a tighter heuristic bound and falls back when a
  // palette outgrows it; with exact upper bounds there is nothing to fall back from)
  for (size_t i = 0; i < ids.size(); ++i) {
    const int j = ids[i];
    jobs[i].lut_dev = F.lut1 + F.pal_off[(size_t)j];
    jobs[i].base = (int32_t)(F.ebase[(size_t)ci] + (F.pal_off[(size_t)j] - F.pal_off[(size_t)jb0]));
  }
  cluster_jobs(L, jobs);
  mark(0);
  // ---- first raster position of every clustered entry of THIS class: one pass over the class's label map, which also keeps every
  // pixel's entry for the final remap (merging.py:77-79)
  const int64_t class_entries = F.pal_off[(size_t)jb1] - F.pal_off[(size_t)jb0];
  int32_t* fp = L.dalloc<int32_t>((size_t)std::max<int64_t>(class_entries, 1));
  for (size_t i = 0; i < ids.size(); ++i)               // INT_MAX over the entries in use (a 32-bit pattern fill per job)
    if (!jobs[i].new_keys.empty())
      EF_HIP(hipMemsetD32Async((hipDeviceptr_t)(fp + (F.pal_off[(size_t)ids[i]] - F.pal_off[(size_t)jb0])), (int)kIntMax, jobs[i].new_keys.size(), L.stream.get()));
  const int32_t* lab_ptr[1] = {cls.labels};
  const int32_t jbase[1] = {jb0};
  EF_RC(c, rhccq_job_index_entries(c, F.rgb, F.H, F.W, 1, lab_ptr, jbase, F.bitmaps, F.prefix, F.d_pal_off, F.fix_key,
                                    fp - F.ebase[(size_t)ci], F.lut1, F.e1map + (size_t)ci * (size_t)F.H * (size_t)F.W));
  // (only the clustered entries come back: a job's slice is as long as its palette, its clustered palette ~100x shorter)
  std::vector<std::vector<int32_t>> fp_host(ids.size());
  const SyncOnUnwind drain(L.stream.get());
  for (size_t i = 0; i < ids.size(); ++i) {
    const int64_t lo = F.pal_off[(size_t)ids[i]] - F.pal_off[(size_t)jb0];
    fp_host[i].resize(jobs[i].new_keys.size());
    if (!jobs[i].new_keys.empty())
      EF_HIP(hipMemcpyAsync(fp_host[i].data(), fp + lo, jobs[i].new_keys.size() * 4, hipMemcpyDeviceToHost, L.stream.get()));
  }
  L.sync();
  std::map<int, std::shared_ptr<Comp>> seg_comp;
  for (size_t i = 0; i < ids.size(); ++i) {
    const int j = ids[i];
    const Job& jb = jobs[i];
    auto cp = std::make_shared<Comp>();
    cp->keys = jb.new_keys;
    const int64_t lo = F.pal_off[(size_t)j] - F.pal_off[(size_t)jb0];
    cp->fp.resize(jb.new_keys.size());
    for (size_t t = 0; t < cp->fp.size(); ++t) cp->fp[t] = fp_host[i][t];
    cp->top_left[0] = (int32_t)F.r0[(size_t)j]; cp->top_left[1] = (int32_t)F.c0[(size_t)j];
    cp->shape[0] = (int32_t)(F.r1[(size_t)j] - F.r0[(size_t)j] + 1); cp->shape[1] = (int32_t)(F.c1[(size_t)j] - F.c0[(size_t)j] + 1);
    std::vector<int32_t> id(jb.new_keys.size());
    for (size_t t = 0; t < id.size(); ++t) id[t] = (int32_t)t;
    cp->maps[j] = std::move(id);
    seg_comp[j] = cp;
    out.k1_off[j] = {F.ebase[(size_t)ci] + lo, F.ebase[(size_t)ci] + lo + (int64_t)jb.new_keys.size()};
  }
  // ---- merge per region (subregions.py:634-679), then per class on the frame canvas (regions.py:34-46)
  std::vector<std::shared_ptr<Comp>> live;
  for (int r = 0; r < cls.n_region; ++r) {
    std::vector<std::shared_ptr<Comp>> segs;
    for (int j = jb0; j < jb1; ++j)
      if (F.job_region[(size_t)j] == r && seg_comp.count(j)) segs.push_back(seg_comp[j]);
    if (segs.empty()) continue;
    const int32_t* bb = cls.region_bbox + 4 * r;
    live.push_back(merge_comps(segs, bb[0], bb[1], bb[2], bb[3]));
  }
  out.q2 = std::min(cls.quality * 2, 100);
  mark(1);
  if (!live.empty()) {                                  // rhccq.ipynb:1009-1013: a class without components contributes nothing
    out.comp2 = merge_comps(live, 0, 0, F.H, F.W);
    Job& j2 = out.job2;
    j2.keys = out.comp2->keys;
    j2.P = (int64_t)out.comp2->keys.size();
    j2.quality = out.q2;
    if (rhccq_params(j2.P, (double)out.q2, &j2.eps, &j2.mc)) throw Err{RHCCQ_E_ARG, "rhccq_params failed"};
    mark(1);
    if (level2_here) level2_stage(L, outs, std::vector<int>(1, ci), false, nullptr);
  }
  EF_HIP(hipEventRecord(out.done.get(), L.stream.get()));
  L.sync();
}

// RHCCQ_OPT_FRAME_CHAINS: the k-means++ chains of every resident level-1 MiniBatchKMeans problem of the frame in ONE launch on the
// caller's stream (one workgroup per problem, as a batch), before the class pipelines start.  The lanes' streams share the
// runtime's few hardware queues; a chain on a queue holds up every other stream mapped there for its whole length (a 106 ms chain
// of one class delayed the other class's set-up or steps by as much).  Nothing after the chains can start before they end, so
// one launch costs no time and leaves no chain to block another stream.  Draws and chain set-up are the fit's own (mbk_draws, mbk_chains).
void frame_chains(FrameCtx& F, hipStream_t stream) {
  rhccq_ctx* c = F.root;
  FrameState& FS = *(FrameState*)c->frame_state;
  const bool tr = trace_on();
  const double t0 = now_ms();
  std::vector<int> ids;
  std::vector<rhccq_mbk_problem> probs;
  std::vector<const MbkDraws*> draws;
  rhccq_fit::Totals tot;
  for (int ci = 0; ci < F.n_classes; ++ci)
    for (int j = F.job_base[(size_t)ci]; j < F.job_base[(size_t)ci + 1]; ++j) {
      const int64_t hb = F.has_black[(size_t)j] ? 1 : 0;
      const int64_t n = F.P[(size_t)j] - hb;
      if (!F.present[(size_t)j] || n < kMinibatchThreshold) continue;
      const int64_t k = mbk_k(n, F.classes[ci].quality);
      if (k < 1) continue;                              // (a quality rhccq_params refuses: the class's own pipeline reports it)
      PreChain pc;
      pc.draws = mbk_draws(n, k);
      if (pc.draws.c.init_size > kFrameChainMaxInit) continue;
      rhccq_mbk_problem q;
      q.off = F.pal_off[(size_t)j] + hb; q.n = n; q.k = k;
      tot.add(q, pc.draws.c);
      // (a released problem's steps rewrite its centres while a neighbour's chain has yet to write its own: no 128-byte line -- 4 centres,
      // 32 entries of `chosen` -- belongs to two problems.  The lanes' own fits lay their problems out themselves: nothing else moves.)
      tot.ktot = (tot.ktot + 31) & ~(int64_t)31;
      probs.push_back(q);
      ids.push_back(j);
      F.pre[j] = std::move(pc);
      draws.push_back(&F.pre[j].draws);
    }
  if (probs.empty()) return;
  ChainClocks clk;
  clk.sync = false;
  // RHCCQ_OPT_CHAIN_RELEASE: a flag per problem and a tag no earlier launch used
  const bool release = c->opt_chain_release != 0;
  uint32_t* flags_dev = nullptr;
  if (release) {
    if (FS.release_cap < (int32_t)probs.size()) {       // (between frames: no launch uses the old flags)
      uint32_t *h = nullptr, *d = nullptr;
      const int32_t cap = std::max<int32_t>((int32_t)probs.size(), 64);
      if (rhccq_release_flags_alloc(cap, &h, &d)) throw Err{RHCCQ_E_HIP, "rhccq_release_flags_alloc failed"};
      FS.release_flags.reset(h);
      FS.release_flags_dev = d;
      FS.release_cap = cap;
    }
    flags_dev = FS.release_flags_dev;
    FS.release_tag = rhccq_release::next_tag(FS.release_tag);
  }
  int32_t published = 0;
  double* centres = mbk_chains(c, FS.root_arena, F.keys_dev, probs, draws, tot, tr ? &clk : nullptr, flags_dev, FS.release_tag, &published);
  F.chains_done = make_event();
  EF_HIP(hipEventRecord(F.chains_done.get(), stream));
  for (size_t i = 0; i < probs.size(); ++i) {
    PreChain& pc = F.pre[ids[i]];
    pc.centres = centres + 4 * probs[i].koff;
    pc.done = F.chains_done.get();
    pc.host_wait = release;
    if (release && published) {
      pc.flag = FS.release_flags.get() + i * (size_t)rhccq_release::kFlagStrideWords;
      pc.tag = FS.release_tag;
    }
  }
  if (tr) fprintf(stderr, "[rhccq] frame chains: %zu problems, %lld init samples, set-up %.2f ms (host), launched after %.2f ms, %s\n", probs.size(),
                  (long long)tot.itot, clk.ordered - t0, now_ms() - t0,
                  !release ? "lanes wait for the launch" : published ? "every problem released by its own flag" : "this chain kernel publishes nothing: lanes wait for the launch on the host");
}

int encode_frame(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const rhccq_class_desc* classes, int32_t n_classes, uint8_t* palette_out,
                 int32_t pal_cap, void* indices_out, int64_t* n_unique_out, rhccq_frame_result* res) {
  const double t_start = now_ms();
  EF_HIP(hipSetDevice(ctx->device));
  if (!ctx->frame_state) {
    ctx->frame_state = new FrameState();
    ctx->frame_state_free = free_frame_state;
  }
  FrameState& FS = *(FrameState*)ctx->frame_state;
  while ((int)FS.classes.size() < n_classes) FS.classes.push_back(std::make_unique<Lane>(ctx->device));
  for (auto& l : FS.classes) {
    l->adopt_options(ctx);
    l->reset();
  }
  FS.root_arena.reset();
  Arena& A = FS.root_arena;
  hipStream_t stream = ctx->stream;
  FrameCtx F;
  F.root = ctx; F.rgb = rgb; F.H = H; F.W = W; F.classes = classes; F.n_classes = n_classes;
  F.job_base.assign((size_t)n_classes + 1, 0);
  for (int ci = 0; ci < n_classes; ++ci) F.job_base[(size_t)ci + 1] = F.job_base[(size_t)ci] + classes[ci].n_seg;
  const int n_jobs = F.n_jobs = F.job_base[(size_t)n_classes];
  if (n_jobs <= 0) throw Err{RHCCQ_E_ARG, "encode_frame: no segments"};
  if (n_jobs > kMaxJobs) throw Err{RHCCQ_E_LIMIT, "encode_frame: more than 2048 segments (the sort-based unique path is the Python FrameEncoder's)"};
  const size_t n_px = (size_t)H * (size_t)W;
  std::vector<const int32_t*> labels((size_t)n_classes);
  for (int ci = 0; ci < n_classes; ++ci) labels[(size_t)ci] = classes[ci].labels;
  // ---- pass 1 (K0 + K1a): per-segment statistics and colour flags
  double t0 = now_ms();
  uint32_t* bitmaps = (uint32_t*)A.alloc((size_t)n_jobs * RHCCQ_BITMAP_WORDS * 4);
  EF_HIP(hipMemsetAsync(bitmaps, 0, (size_t)n_jobs * RHCCQ_BITMAP_WORDS * 4, stream));
  std::vector<int32_t> st_init((size_t)n_jobs * 6);
  for (int j = 0; j < n_jobs; ++j) {
    int32_t* s = &st_init[(size_t)j * 6];
    s[0] = kIntMax; s[1] = -1; s[2] = kIntMax; s[3] = -1; s[4] = 0; s[5] = 0;
  }
  int32_t* stats = (int32_t*)A.alloc(st_init.size() * 4);
  EF_HIP(hipMemcpyAsync(stats, st_init.data(), st_init.size() * 4, hipMemcpyHostToDevice, stream));
  if (n_jobs <= 64) {                                   // byte flags (plain stores) packed into the bitmaps; many jobs: atomics on bits
    uint8_t* bytemaps = (uint8_t*)A.alloc((size_t)n_jobs << 24);
    EF_HIP(hipMemsetAsync(bytemaps, 0, (size_t)n_jobs << 24, stream));
    EF_RC(ctx, rhccq_job_scan_bytes(ctx, rgb, H, W, n_classes, labels.data(), F.job_base.data(), 0, bytemaps, stats));
    EF_RC(ctx, rhccq_bytemap_pack(ctx, bytemaps, n_jobs, bitmaps));
  } else {
    EF_RC(ctx, rhccq_job_scan(ctx, rgb, H, W, n_classes, labels.data(), F.job_base.data(), 0, bitmaps, stats));
  }
  std::vector<int32_t> st((size_t)n_jobs * 6);
  EF_HIP(hipMemcpyAsync(st.data(), stats, st.size() * 4, hipMemcpyDeviceToHost, stream));
  EF_HIP(hipStreamSynchronize(stream));
  res->ms[0] = now_ms() - t0;
  t0 = now_ms();
  // ---- crop = tight bbox +-2 px clamped to the region (subregions.py:346-352); which segments need the black fix (:393-421)
  F.present.assign((size_t)n_jobs, 0); F.has_black.assign((size_t)n_jobs, 0);
  F.job_class.resize((size_t)n_jobs); F.job_region.resize((size_t)n_jobs);
  F.r0.resize((size_t)n_jobs); F.r1.resize((size_t)n_jobs); F.c0.resize((size_t)n_jobs); F.c1.resize((size_t)n_jobs);
  std::vector<uint8_t> needs_fix((size_t)n_jobs, 0);
  std::vector<int32_t> black_jobs;
  bool any_fix = false;
  for (int ci = 0; ci < n_classes; ++ci)
    for (int s = 0; s < classes[ci].n_seg; ++s) {
      const int j = F.job_base[(size_t)ci] + s;
      const int32_t* q = &st[(size_t)j * 6];
      const int reg = classes[ci].seg_region[s];
      if (reg < 0 || reg >= classes[ci].n_region) throw Err{RHCCQ_E_ARG, "encode_frame: seg_region names a region that does not exist"};
      const int32_t* rb = classes[ci].region_bbox + 4 * reg;
      F.job_class[(size_t)j] = ci;
      F.job_region[(size_t)j] = reg;
      const int64_t count = q[4], n_black = q[5];
      F.present[(size_t)j] = count > 0;
      F.r0[(size_t)j] = std::max<int64_t>(rb[0], (int64_t)q[0] - 2);
      F.r1[(size_t)j] = std::min<int64_t>((int64_t)rb[2] - 1, (int64_t)q[1] + 2);
      F.c0[(size_t)j] = std::max<int64_t>(rb[1], (int64_t)q[2] - 2);
      F.c1[(size_t)j] = std::min<int64_t>((int64_t)rb[3] - 1, (int64_t)q[3] + 2);
      const int64_t area = (F.r1[(size_t)j] - F.r0[(size_t)j] + 1) * (F.c1[(size_t)j] - F.c0[(size_t)j] + 1);
      const bool has_bg = count > 0 && area > count;
      const bool all_black = count > 0 && n_black > 0 && count == n_black;
      needs_fix[(size_t)j] = count > 0 && n_black > 0 && count > n_black;
      any_fix = any_fix || needs_fix[(size_t)j];
      F.has_black[(size_t)j] = has_bg || all_black;
      if (F.has_black[(size_t)j]) black_jobs.push_back(j);
    }
  if (any_fix) {
    uint8_t* d_need = (uint8_t*)A.alloc((size_t)n_jobs);
    EF_HIP(hipMemcpyAsync(d_need, needs_fix.data(), (size_t)n_jobs, hipMemcpyHostToDevice, stream));
    unsigned long long* best = (unsigned long long*)A.alloc((size_t)n_jobs * 8);
    EF_HIP(hipMemsetAsync(best, 0xff, (size_t)n_jobs * 8, stream));
    EF_RC(ctx, rhccq_job_blackfix(ctx, rgb, H, W, n_classes, labels.data(), F.job_base.data(), d_need, best));
    std::vector<unsigned long long> hb((size_t)n_jobs);
    EF_HIP(hipMemcpyAsync(hb.data(), best, (size_t)n_jobs * 8, hipMemcpyDeviceToHost, stream));
    EF_HIP(hipStreamSynchronize(stream));
    std::vector<uint32_t> fk((size_t)n_jobs, 0u);
    std::vector<uint8_t> px((size_t)n_jobs * 3, 0);
    const SyncOnUnwind drain_px(stream);
    for (int j = 0; j < n_jobs; ++j)
      if (needs_fix[(size_t)j]) {
        const unsigned long long pos = hb[(size_t)j] & ((1ull << 40) - 1ull);
        EF_HIP(hipMemcpyAsync(&px[(size_t)j * 3], rgb + pos * 3, 3, hipMemcpyDeviceToHost, stream));
      }
    EF_HIP(hipStreamSynchronize(stream));
    for (int j = 0; j < n_jobs; ++j)
      if (needs_fix[(size_t)j]) fk[(size_t)j] = ((uint32_t)px[(size_t)j * 3] << 16) | ((uint32_t)px[(size_t)j * 3 + 1] << 8) | px[(size_t)j * 3 + 2];
    F.fix_key = (uint32_t*)A.alloc((size_t)n_jobs * 4);
    EF_HIP(hipMemcpyAsync(F.fix_key, fk.data(), (size_t)n_jobs * 4, hipMemcpyHostToDevice, stream));
    EF_HIP(hipStreamSynchronize(stream));
  }
  // ---- K1b: sorted unique colours of every segment (np.unique(axis=0) order, clustering.py:21-23)
  if (!black_jobs.empty()) {
    int32_t* d_bj = (int32_t*)A.alloc(black_jobs.size() * 4);
    EF_HIP(hipMemcpyAsync(d_bj, black_jobs.data(), black_jobs.size() * 4, hipMemcpyHostToDevice, stream));
    EF_RC(ctx, rhccq_job_set_black(ctx, bitmaps, d_bj, (int32_t)black_jobs.size()));
  }
  uint32_t* chunk = (uint32_t*)A.alloc((size_t)n_jobs * 512 * 4);
  int32_t* d_counts = (int32_t*)A.alloc((size_t)n_jobs * 4);
  EF_RC(ctx, rhccq_bitmap_count(ctx, bitmaps, n_jobs, chunk, d_counts));
  std::vector<int32_t> counts((size_t)n_jobs);
  EF_HIP(hipMemcpyAsync(counts.data(), d_counts, (size_t)n_jobs * 4, hipMemcpyDeviceToHost, stream));
  EF_HIP(hipStreamSynchronize(stream));
  F.P.resize((size_t)n_jobs);
  F.pal_off.assign((size_t)n_jobs + 1, 0);
  for (int j = 0; j < n_jobs; ++j) {
    F.P[(size_t)j] = counts[(size_t)j];
    F.pal_off[(size_t)j + 1] = F.pal_off[(size_t)j] + counts[(size_t)j];
    if (n_unique_out) n_unique_out[j] = counts[(size_t)j];
  }
  const int64_t total = F.pal_off[(size_t)n_jobs];
  F.d_pal_off = (int64_t*)A.alloc((size_t)n_jobs * 8);
  EF_HIP(hipMemcpyAsync(F.d_pal_off, F.pal_off.data(), (size_t)n_jobs * 8, hipMemcpyHostToDevice, stream));
  F.prefix = (uint32_t*)A.alloc((size_t)n_jobs * RHCCQ_BITMAP_WORDS * 8);
  F.keys_dev = (uint32_t*)A.alloc((size_t)std::max<int64_t>(total, 1) * 4);
  EF_RC(ctx, rhccq_bitmap_emit(ctx, bitmaps, n_jobs, chunk, F.d_pal_off, F.prefix, F.keys_dev));
  F.bitmaps = bitmaps;
  F.lut1 = (int32_t*)A.alloc((size_t)std::max<int64_t>(total, 1) * 4);
  EF_HIP(hipMemsetAsync(F.lut1, 0, (size_t)std::max<int64_t>(total, 1) * 4, stream));
  F.e1map = (int32_t*)A.alloc((size_t)n_classes * n_px * 4);
  F.ebase.assign((size_t)n_classes + 1, 0);
  for (int ci = 0; ci < n_classes; ++ci) F.ebase[(size_t)ci + 1] = F.pal_off[(size_t)F.job_base[(size_t)ci + 1]];
  F.ready = make_event();
  EF_HIP(hipEventRecord(F.ready.get(), stream));
  EF_HIP(hipStreamSynchronize(stream));                  // (the host tables above are staged; pal_off is read by the lanes)
  res->ms[1] = now_ms() - t0;
  t0 = now_ms();
  if (ctx->opt_frame_chains) frame_chains(F, stream);
  // ---- levels 1 and 2: every class a pipeline of its own (nothing of a class's chain depends on the other class; only
  // quantize_image needs both: regions.py:9-70 is called once per class, rhccq.ipynb:1001-1013)
  std::vector<ClassOut> outs((size_t)n_classes);
  for (auto& o : outs) o.done = make_event();            // (all of them before the first thread starts)
  const SyncOnUnwind drain(stream);                      // (F, outs and the host tables above outlive whatever the caller's stream still does)
  const bool frame_level2 = ctx->opt_frame_level2 != 0;
  run_lanes(
      (size_t)n_classes, [&](size_t ci) { class_pipeline(F, (int)ci, *FS.classes[ci], outs, !frame_level2); },
      [&](size_t ci) { (void)hipStreamSynchronize(FS.classes[ci]->stream.get()); });
  FS.level2_fits.clear();
  if (frame_level2) {
    // ---- level 2 of every class in ONE clustering call on the first class's lane: the class threads have ended and their streams
    // are idle, so nothing of the frame queues launches beside it (RHCCQ_OPT_FRAME_LEVEL2)
    Lane& L2 = *FS.classes[0];
    level2_stage(L2, outs, level2_classes(outs), true, &FS.level2_fits);
    L2.sync();
  }
  res->ms[2] = now_ms() - t0;
  for (int ci = 0; ci < n_classes && ci < 4; ++ci) std::memcpy(res->class_ms[ci], outs[(size_t)ci].ms, sizeof(outs[(size_t)ci].ms));
  t0 = now_ms();
  // ---- level 3: merge ROI + non-ROI (image.py:246-256), cluster(q3)
  std::vector<std::shared_ptr<Comp>> comps3;
  int q3 = 0;
  for (int ci = 0; ci < n_classes; ++ci) {
    EF_HIP(hipStreamWaitEvent(stream, outs[(size_t)ci].done.get(), 0));
    q3 += outs[(size_t)ci].q2;
    if (outs[(size_t)ci].comp3) comps3.push_back(outs[(size_t)ci].comp3);
  }
  q3 = std::min(q3, 100);
  if (comps3.empty()) throw Err{RHCCQ_E_ARG, "encode_frame: no components"};
  auto m3c = merge_comps(comps3, 0, 0, H, W);
  Lane& L3 = *FS.classes[0];
  std::vector<Job> j3(1);
  j3[0].keys = m3c->keys;
  j3[0].P = (int64_t)m3c->keys.size();
  j3[0].quality = q3;
  if (rhccq_params(j3[0].P, (double)q3, &j3[0].eps, &j3[0].mc)) throw Err{RHCCQ_E_ARG, "rhccq_params failed"};
  cluster_jobs(L3, j3);
  L3.sync();
  res->ms[3] = now_ms() - t0;
  t0 = now_ms();
  // ---- compose levels 2-3 into one table over the clustered level-1 entries (frame.py::finish)
  const std::vector<uint32_t>& fk3 = j3[0].new_keys;
  const std::vector<int32_t>& mp3 = j3[0].mapping;
  const bool multi = comps3.size() > 1;
  int32_t* d_lut2 = (int32_t*)A.alloc((size_t)std::max<int64_t>(total, 1) * 4);
  int64_t max_index = 0;
  std::vector<std::vector<int32_t>> staged;             // (kept alive until the copies are issued and the stream has taken them)
  const SyncOnUnwind drain_staged(stream);
  for (auto& c2 : comps3)
    for (auto& kv : c2->maps) {
      const int job = kv.first;
      const std::vector<int32_t>& m = kv.second;
      std::vector<int32_t> v(m.size());
      for (size_t t = 0; t < m.size(); ++t) {
        if (multi) {
          const bool painted = c2->keys[(size_t)m[t]] != 0u;        // black = transparent (merging.py:75)
          v[t] = painted ? mp3[(size_t)m3c->maps[job][t]] : -1;
        } else {
          v[t] = mp3[(size_t)m[t]];
        }
        max_index = std::max<int64_t>(max_index, v[t]);
      }
      const int ci = F.job_class[(size_t)job];
      const auto& off = outs[(size_t)ci].k1_off[job];
      if (!v.empty()) EF_HIP(hipMemcpyAsync(d_lut2 + off.first, v.data(), v.size() * 4, hipMemcpyHostToDevice, stream));
      staged.push_back(std::move(v));
    }
  int32_t default_index = 0;
  if (multi) default_index = mp3[0];
  else
    for (size_t t = 0; t < fk3.size(); ++t)
      if (fk3[t] == 0u) { default_index = (int32_t)t; break; }
  max_index = std::max<int64_t>(max_index, default_index);
  const int elem = max_index < 256 ? 1 : (max_index < 65536 ? 2 : 4);          // compression.py:360-372
  res->ms[4] = now_ms() - t0;
  t0 = now_ms();
  EF_RC(ctx, rhccq_frame_remap_entries(ctx, H, W, n_classes, labels.data(), F.job_base.data(), F.e1map, d_lut2, default_index, indices_out, elem));
  EF_HIP(hipStreamSynchronize(stream));
  res->ms[5] = now_ms() - t0;
  res->n_colours = (int32_t)fk3.size();
  res->index_bytes = elem;
  res->quality3 = q3;
  res->n_jobs = n_jobs;
  if (multi) {
    res->shape[0] = H; res->shape[1] = W; res->top_left[0] = 0; res->top_left[1] = 0;
  } else {
    res->shape[0] = m3c->shape[0]; res->shape[1] = m3c->shape[1]; res->top_left[0] = m3c->top_left[0]; res->top_left[1] = m3c->top_left[1];
  }
  res->ms[6] = now_ms() - t_start;
  if ((int64_t)fk3.size() > pal_cap) throw Err{RHCCQ_E_LIMIT, "encode_frame: palette_out too small (res->n_colours entries are needed)"};
  for (size_t t = 0; t < fk3.size(); ++t) {
    palette_out[3 * t] = (uint8_t)(fk3[t] >> 16);
    palette_out[3 * t + 1] = (uint8_t)(fk3[t] >> 8);
    palette_out[3 * t + 2] = (uint8_t)fk3[t];
  }
  return 0;
}

}  // namespace

extern "C" int32_t rhccq_encode_frame_level2_info(const rhccq_ctx* ctx, int32_t cap, int64_t* out) {
  if (!ctx || cap < 0 || (cap > 0 && !out)) return -1;
  if (!ctx->frame_state) return 0;
  const FrameState& FS = *(const FrameState*)ctx->frame_state;
  for (size_t i = 0; i < FS.level2_fits.size() && (int32_t)i < cap; ++i) {
    const Level2Fit& f = FS.level2_fits[i];
    int64_t* o = out + 6 * i;
    o[0] = f.cls; o[1] = f.n; o[2] = f.k; o[3] = f.steps; o[4] = f.schedule; o[5] = f.overlapped_from;
  }
  return (int32_t)FS.level2_fits.size();
}

extern "C" int rhccq_encode_frame(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const rhccq_class_desc* classes, int32_t n_classes,
                                  uint8_t* palette_out, int32_t pal_cap, void* indices_out, int64_t* n_unique_out, rhccq_frame_result* res) {
  if (!ctx || !rgb || !classes || !palette_out || !indices_out || !res || H <= 0 || W <= 0 || n_classes <= 0 || pal_cap < 0 ||
      (int64_t)H * W > INT32_MAX)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "encode_frame: bad argument");
  for (int ci = 0; ci < n_classes; ++ci)
    if (!classes[ci].labels || classes[ci].n_seg < 0 || classes[ci].n_region < 0 || (classes[ci].n_seg > 0 && !classes[ci].seg_region) ||
        (classes[ci].n_region > 0 && !classes[ci].region_bbox))
      return rhccq_fail(ctx, RHCCQ_E_ARG, "encode_frame: bad class descriptor");
  std::memset(res, 0, sizeof(*res));
  try {
    return encode_frame(ctx, rgb, H, W, classes, n_classes, palette_out, pal_cap, indices_out, n_unique_out, res);
  } catch (const Err& e) {
    // (second line of defence, kept: the lanes and encode_frame drain their own streams while they unwind, but a throw ahead of
    // encode_frame's first guard leaves kernels on the caller's stream that read rgb and the label maps, which the caller may free now)
    (void)hipDeviceSynchronize();
    ctx->err = e.msg;
    return e.code;
  } catch (const std::exception& e) {
    (void)hipDeviceSynchronize();
    ctx->err = std::string("encode_frame: ") + e.what();
    return RHCCQ_E_HIP;
  }
}
