// The step functions and constants of the exact row segmentation onto a given palette, shared by its kernel and its host form
// (palette_segment.hip).
//
// Arithmetic.  Every decision of the dynamic programme compares costs of one pixel with each other, so a term that is the same for
// every state of a pixel may be dropped.  Two such terms go:
//   * of the squared distance |p - c|^2 = |p|^2 - 2 p.c + |c|^2 only key(p, c) = 2 p.(255 - c) + |c|^2 = |p - c|^2 - |p|^2 + 510 (r + g + b)
//     is formed (the remap's dot product against the inverted row, so the key is never negative);
//   * the minimum m of the previous column is subtracted in every step.
// With u = C(c) - (m + pen + 1):   stay <=> C(c) <= m + pen <=> u < 0,   and   min(C(c) - m, pen) = pen + 1 + min(u, -1),   so a state's step is
// one subtraction, the sign bit shifted into the state's word of stay bits, one minimum and one three-operand addition behind the key's
// dot product and shift-add.  0 <= key <= 585 225 and pen <= 2^24 - 1: a cost stays below 2^25, a padding state (kSegPad) below 2^27.
// Packed costs.  For the minimum AND the lowest state that attains it every cost is kept as (cost << 4 | slot), slot = c / 64 (c % 64 is the
// lane; the host form uses slot 0 throughout), below 2^31.  Keys, m and pen enter shifted by 4; min(u, -1) becomes min(u, slot - 16), which
// keeps the slot in the low bits, and the sign of u is unchanged, so no step packs or unpacks anything.  The unsigned minimum of the packed
// words over the wave is the minimal cost with the lowest slot, and the lowest lane that holds it gives the state slot * 64 + lane.
#pragma once
#include "palette_runs.h"

namespace rhccq {

constexpr int kSegLanes = 64;                         // lanes of a workgroup (one wave): the wave owns one image row
constexpr int kSegCols = 32;                          // columns of a tile: the stay bits of one state over a tile are one dword
constexpr int kSegMaxS = 16;                          // states a lane holds at most: state c lives in lane c % 64, slot c / 64
constexpr int kSegMaxRows = kSegLanes * kSegMaxS;     // the largest palette of the device form
constexpr uint32_t kSegMaxPenalty = (1u << 24) - 1u;
constexpr int32_t kSegPad = 1 << 26;                  // the key of a state past the palette's last row: above every real cost

struct SegPenalty { uint32_t v[kRemapMaxClasses + 1]; };

// dwords of one tile's record in the workspace: slots x 64 words of stay bits, then 32 uint16 a(x)
__host__ __device__ __forceinline__ long long seg_tile_words(int slots) { return (long long)slots * kSegLanes + kSegCols / 2; }

// the inverted row the key's dot product runs against
__host__ __device__ __forceinline__ uint32_t seg_inv(uint32_t col) { return 0x00FFFFFFu - col; }
// the packed key from |row|^2 << 4
__host__ __device__ __forceinline__ int32_t seg_key(uint32_t px, uint32_t inv, int32_t n2p) { return (int32_t)(remap_dot(px, inv) << 5) + n2p; }
// one state's step on packed words: cost is C_{x-1}(c) on entry and C_x(c) on return, each less the terms all states of its column share;
// the stay bit enters `bits` from the right.  mp1 = (m + pen + 1) << 4, pen1 = (pen + 1) << 4
__host__ __device__ __forceinline__ void seg_step(int32_t& cost, uint32_t& bits, int32_t key, int32_t mp1, int32_t pen1, int slot) {
  const int32_t u = cost - mp1, top = slot - 16;
  bits = bits << 1 | (uint32_t)u >> 31;
  cost = key + pen1 + (u < top ? u : top);
}

}  // namespace rhccq
