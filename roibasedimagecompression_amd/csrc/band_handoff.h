// The hand-over between the bands of a banded wavefront kernel, stated once: palette_dither_kernel (palette_dither.hip) and
// pngr::unfilter_kernel (png_read.hip) call it.  A one-wave workgroup owns a band of image rows, and row 0 of band n needs the last row of
// band n - 1.  That row reaches it through 32-bit words in a workspace the caller zeroes on the stream before the launch.
//   layout    a head of 64 words: word 0 the ticket, word 1 the abort word, words 2 and 3 the caller's; behind it row_words words for
//             every band but the last.  The layout, the constants and work_bytes are plain C++ over <stdint.h>; the rest exists under
//             hipcc only.
//   a word    carries its value and, in bit 31, the "written" mark.  Value and mark share a word, so a word validates itself: there is no
//             flag beside it, and with no second location to order against, no fence.  Words are stored and re-read with relaxed
//             agent-scope atomics.
//   a fetch   a band re-reads a granule of words (a lane a word) until all of them carry the mark; the next granule is requested a
//             granule ahead and has usually landed when it is needed.
// Forward progress.  A band's number is a ticket drawn from the workspace when the workgroup starts, not blockIdx: the band it waits for
// drew its ticket earlier, so it has started, and by induction waits only for bands that have; band 0 waits for nothing.  No workgroup
// waits for one that may not be resident, whatever the grid and the device.  The wait is bounded all the same: every 256 re-reads the
// waiter looks at the abort word, past 2^24 re-reads it raises it and sets the caller's give-up word.  A band that gave up, or saw the
// abort word, waits no more: it runs on with zeros for the words it did not get and ends in the time an unhindered band takes; what it
// writes means nothing.
// Each kernel keeps its packing, its stores, its rule for skipping the wait and its memset.  The k-means++ sharded chain's jx_wait
// (k8_minibatch.hip) is another protocol (granules tagged with the pick number, no ticket, both directions) and stays where it is.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace rhccq {
namespace band {

constexpr int kHeadWords = 64;                  // the workspace's head; the hand-over words follow
constexpr int kTicketWord = 0, kAbortWord = 1;  // (words 2 and 3 belong to the caller)
constexpr uint32_t kWritten = 0x80000000u;      // the mark of a hand-over word
constexpr uint32_t kSpinCheck = 256u;           // a waiter looks at the abort word every so many re-reads
constexpr uint32_t kSpinBound = 1u << 24;       // and gives up after so many

// the workspace of `bands` bands that hand on rows of row_words words
inline int64_t work_bytes(int64_t bands, int64_t row_words) { return 4 * (kHeadWords + (bands > 1 ? (bands - 1) * row_words : 0)); }

#if defined(__HIPCC__)
// the words band b hands on (b = -1, the "band above" of band 0, is formed and never read)
__device__ __forceinline__ uint32_t* words(uint32_t* work, long long b, long long row_words) { return work + kHeadWords + b * row_words; }

__device__ __forceinline__ uint32_t word_load(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void word_store(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the ticket: lane 0 draws the band's number into a __shared__ word; the caller's next barrier publishes it
__device__ __forceinline__ void draw_ticket(uint32_t* work, uint32_t* s_band, int lane) {
  if (lane == 0) *s_band = __hip_atomic_fetch_add(work + kTicketWord, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The granule of kWords words that starts at word `first` of the row above (up_words, row_words long): lane l < kWords gets word first + l
// in `gran` (with its mark; 0 past the row's end and in the other lanes), and `pending` becomes the request for the granule behind it.
// Called wave-uniformly while `waiting` (wave uniform), which it clears when the band gives up or is told to: lane 0 then raises the abort
// word and *gave_up.  Every lane loads, from a clamped address, and there is no early return for a band that gave up: a masked load, or
// a way out of the caller's walk, makes the compiler wait for all outstanding memory traffic in every step of the walk.
template <int kWords>
__device__ __forceinline__ void fetch_granule(const uint32_t* up_words, long long first, long long row_words, int lane, uint32_t* abort_word,
                                              uint32_t* gave_up, bool& waiting, uint32_t& gran, uint32_t& pending) {
  const long long i = first + lane;
  const bool on = lane < kWords && i < row_words;
  for (uint32_t spins = 0; !__all(!on || (pending & kWritten) != 0u); ++spins) {
    if ((spins & (kSpinCheck - 1u)) == kSpinCheck - 1u) {
      const bool told = __any(word_load(abort_word) != 0u);          // another band gave up
      if (told || spins > kSpinBound) {                              // stop waiting, here and for the rest of the band
        if (!told && lane == 0) {                                    // this one gives up: the others and the caller are told
          word_store(abort_word, 1u);
          word_store(gave_up, 1u);
        }
        waiting = false;
        break;
      }
    }
    if (spins) __builtin_amdgcn_s_sleep(2);
    pending = word_load(up_words + min(i, row_words - 1));
  }
  gran = on ? pending : 0u;                                          // (consumed before the next request is issued)
  pending = word_load(up_words + min(i + kWords, row_words - 1));    // (the lanes that are not `on` then are ignored then)
}
#endif

}  // namespace band
}  // namespace rhccq
