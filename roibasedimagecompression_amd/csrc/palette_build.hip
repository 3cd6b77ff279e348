// A palette from the image on the device (EXTENSION, no reference counterpart): greedy variance-minimising box splitting over a
// 32 x 32 x 32 colour histogram (Wu's quantiser) with exact rational comparisons.  The definition is in include/rhccq.h; in short:
// rhccq_palette_cells sums weight and weight x channel value per cell (r >> 3, g >> 3, b >> 3) in 64-bit integers; rhccq_palette_build
// starts from the whole cube as box 0 and, while fewer than K_target boxes exist, splits the box whose best cut removes the most squared
// error, |N S1 - N1 S|^2 / (N N1 (N - N1)), ties to the lowest box, axis and position; a box's row is floor((2 S + N) / (2 N)).
//
// Exactness.  The sum of N is at most 2^32 - 1 and S <= 255 N < 2^40, so N S1 and N1 S are below 2^72, their difference squared below 2^144,
// the three channels together below 2^146 (three 64-bit limbs); N N1 < 2^64 and the denominator below 2^96 (two limbs).  Two gains are
// compared by cross-multiplication: each side is below 2^242 and is formed limb by limb (build_cross, palette_build.h).  128 bits are not
// enough: a 512 x 768 picture already needs 138.
//
// Device form of the cells pass: one launch (behind a memset unless the call accumulates).  The table is 1 MiB, six times the LDS of a CU,
// so it stays in global memory and what is reduced is the number of atomics that reach it, above all the ones that meet on the cells of
// a picture's large flat areas (adds to one address serialise).  Two levels.  (1) A lane holds 8 pixels a block apart, so the 64 lanes of
// a wave hold 64 neighbouring pixels of an image row at a time, and neighbouring pixels mostly share cells: the wave takes the cell of its
// first open lane and sums {w, w r, w g, w b} over the lanes of that cell (the sums stay below 2^22); after kCellsRounds such rounds the
// lanes still open go on with their own pixel.  (2) A workgroup owns a contiguous stretch of the picture and a table of kCellsSlots slots
// in LDS, {cell, N, Sr, Sg, Sb} with 64-bit sums (36 bytes a slot, four workgroups a CU): a contribution goes to the slot its cell's low
// coordinate bits name, which the first cell to come claims (one LDS compare-and-swap), and a cell that finds its slot taken by another
// goes straight to global memory; at the end every claimed slot is flushed with four 64-bit global atomics.  One colour costs four global
// atomics a workgroup; noise costs the plain per-pixel form plus the rounds.  The alternatives lose here: a table of N alone in LDS
// (128 KiB) leaves one workgroup a CU and still sends S to global memory; a full partial table per workgroup is 1 MiB of traffic per
// workgroup against the kilobytes of pixels it reads.  Integer addition only: every order gives the same table.
//
// Device form of the build: three launches that turn the planes into the summed-volume table T[33][33][33] of {N, Sr, Sg, Sb} in the
// workspace (a running sum along b, then g, then r; an entry is at most 2^40), then ONE resident workgroup of four waves that runs the
// chain: boxes, their best cut and its gain (48 bytes a box) live in LDS.  A step is three barriers: the candidate cuts of the two boxes
// the last split made, one lane each (two waves a box, 12 table corners of 32 bytes from L2 per lane), wave butterflies on the key | lane
// 0 stores boxes, cuts and gains | the arg-max over the cached gains.  The two errors that only the table shows (N all zero; a sum above
// 2^32 - 1) cannot be returned without a synchronisation: the chain kernel writes RHCCQ_E_ARG or RHCCQ_E_LIMIT to *k_out, zero outputs
// and -1 throughout splits.  N enters the table clamped (reduce_clamp), so that no sum of 32 768 cells wraps.
#include "palette_build.h"

#include <vector>

namespace rhccq {

constexpr int kCellsBlock = 256;                      // lanes of a workgroup of the cells pass
constexpr int kCellsPx = 8;                           // pixels of a lane, a block apart
constexpr int kCellsChunk = kCellsBlock * kCellsPx;   // pixels of a workgroup at a time
constexpr int kCellsRounds = 4;                       // cells a wave aggregates per 64 pixels before its lanes add on their own
constexpr int kCellsSlots = 1024;                     // slots of a workgroup's table in LDS: 36 bytes a slot, four workgroups a CU
constexpr uint32_t kCellsFree = 0xFFFFFFFFu;
constexpr unsigned long long kCellsMaxSum = kReduceMaxSum;
static_assert(64ull * 255 * 255 < (1ull << 32), "a wave's sums of one pixel column fit 32 bits");

constexpr int kBuildBlock = 256;                      // lanes of the chain's resident workgroup: two waves per new box
constexpr int kBuildWaves = kBuildBlock / 64;
constexpr int kBuildMaxRows = 1024;                   // boxes whose state the LDS of the chain holds (48 bytes a box)
static_assert(kBuildWaves == 4 && kBuildCodes <= 128, "two waves cover the codes of a box");
static_assert(kBuildMaxRows * 48 + 1024 <= 64 * 1024 && kBuildMaxRows <= kBuildCells, "LDS layout of the chain kernel");
static_assert(sizeof(BuildSum) == 32, "a table entry is four 64-bit words");

struct CellsWeights { uint32_t w[kRemapMaxClasses + 1]; };

__device__ __forceinline__ void cells_add(unsigned long long* __restrict__ cells, int cell, unsigned long long n, unsigned long long r,
                                          unsigned long long g, unsigned long long b) {
  atomicAdd(cells + cell, n);
  atomicAdd(cells + kBuildCells + cell, r);
  atomicAdd(cells + 2 * kBuildCells + cell, g);
  atomicAdd(cells + 3 * kBuildCells + cell, b);
}

// the slot of a cell in the workgroup's table: the low bits of the three coordinates, so that the cells of a 16 x 8 x 8 neighbourhood
// of the colour cube, what a stretch of a picture mostly holds, never share a slot
__device__ __forceinline__ int cells_slot(int cell) { return ((cell >> 10) & 15) << 6 | ((cell >> 5) & 7) << 3 | (cell & 7); }

// one contribution to the workgroup's table, or, when another cell holds the slot, straight to global memory
__device__ __forceinline__ void cells_put(uint32_t* s_tag, unsigned long long* s_acc, unsigned long long* __restrict__ cells, int cell, uint32_t n,
                                          uint32_t r, uint32_t g, uint32_t b) {
  const int slot = cells_slot(cell);
  uint32_t tag = s_tag[slot];
  if (tag == kCellsFree) {
    tag = atomicCAS(&s_tag[slot], kCellsFree, (uint32_t)cell);
    if (tag == kCellsFree) tag = (uint32_t)cell;
  }
  if (tag == (uint32_t)cell) {
    atomicAdd(&s_acc[slot * 4], (unsigned long long)n);
    atomicAdd(&s_acc[slot * 4 + 1], (unsigned long long)r);
    atomicAdd(&s_acc[slot * 4 + 2], (unsigned long long)g);
    atomicAdd(&s_acc[slot * 4 + 3], (unsigned long long)b);
  } else {
    cells_add(cells, cell, n, r, g, b);
  }
}

__global__ __launch_bounds__(kCellsBlock) void palette_cells_kernel(const uint8_t* __restrict__ rgb, long long n_px, const uint8_t* __restrict__ cls,
                                                                    int n_classes, CellsWeights wt, unsigned long long* __restrict__ cells) {
  __shared__ uint32_t s_w[kRemapMaxClasses + 1];
  __shared__ uint32_t s_tag[kCellsSlots];                                              // the cell that holds the slot, or kCellsFree
  __shared__ unsigned long long s_acc[kCellsSlots * 4];                                // its {N, Sr, Sg, Sb} over this workgroup's pixels
  const int lane = threadIdx.x & 63;
  if ((int)threadIdx.x <= n_classes) s_w[threadIdx.x] = wt.w[threadIdx.x];
  for (int j = threadIdx.x; j < kCellsSlots; j += kCellsBlock) s_tag[j] = kCellsFree;
  for (int j = threadIdx.x; j < kCellsSlots * 4; j += kCellsBlock) s_acc[j] = 0ull;
  __syncthreads();
  const long long n_chunks = (n_px + kCellsChunk - 1) / kCellsChunk, per = (n_chunks + gridDim.x - 1) / gridDim.x;
  const long long last = min(n_chunks, (long long)(blockIdx.x + 1) * per);             // a contiguous stretch: its pixels share cells
  for (long long chunk = blockIdx.x * per; chunk < last; ++chunk) {
    const long long base = chunk * kCellsChunk + threadIdx.x;
    uint32_t px[kCellsPx], w[kCellsPx];
#pragma unroll
    for (int q = 0; q < kCellsPx; ++q) {
      const long long p = base + (long long)q * kCellsBlock;
      px[q] = 0u;
      w[q] = 0u;
      if (p < n_px) {
        px[q] = remap_pack_px(rgb + p * 3);
        const int c = n_classes > 0 ? (int)cls[p] : n_classes;
        w[q] = s_w[c < n_classes ? c : n_classes];
      }
    }
#pragma unroll
    for (int q = 0; q < kCellsPx; ++q) {
      const uint32_t r = px[q] >> 16, g = (px[q] >> 8) & 255u, b = px[q] & 255u;
      const int cell = build_cell(r, g, b);
      const uint32_t wr = w[q] * r, wg = w[q] * g, wb = w[q] * b;
      unsigned long long open = __ballot(w[q] != 0u);                                  // (wave uniform, as is the loop below)
      for (int round = 0; round < kCellsRounds && open; ++round) {
        const int first = __ffsll((long long)open) - 1;
        const int lead = __shfl(cell, first, 64);
        const bool mine = ((open >> lane) & 1ull) && cell == lead;
        const uint32_t sn = wave_sum(mine ? w[q] : 0u), sr = wave_sum(mine ? wr : 0u), sg = wave_sum(mine ? wg : 0u), sb = wave_sum(mine ? wb : 0u);
        if (lane == 0) cells_put(s_tag, s_acc, cells, lead, sn, sr, sg, sb);
        open &= ~__ballot(mine);
      }
      if ((open >> lane) & 1ull) cells_put(s_tag, s_acc, cells, cell, w[q], wr, wg, wb);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < kCellsSlots; j += kCellsBlock) {
    const uint32_t tag = s_tag[j];
    if (tag != kCellsFree) cells_add(cells, (int)tag, s_acc[j * 4], s_acc[j * 4 + 1], s_acc[j * 4 + 2], s_acc[j * 4 + 3]);
  }
}

// ---- the summed-volume table -------------------------------------------------------------------------------------------------------
// a running sum along b: one thread per (x, y, plane) of the table, the borders x == 0 and y == 0 included (they are zero)
__global__ __launch_bounds__(256) void palette_build_prefix_b_kernel(const unsigned long long* __restrict__ cells, unsigned long long* __restrict__ T) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= kBuildTab * kBuildTab * 4) return;
  const int plane = i & 3, y = (i >> 2) % kBuildTab, x = (i >> 2) / kBuildTab;
  unsigned long long* row = T + (size_t)build_tab_index(x, y, 0) * 4 + plane;
  row[0] = 0ull;
  unsigned long long run = 0ull;
  for (int z = 1; z < kBuildTab; ++z) {
    if (x > 0 && y > 0) {
      const unsigned long long v = cells[(size_t)plane * kBuildCells + ((x - 1) * kBuildSide + (y - 1)) * kBuildSide + (z - 1)];
      run += plane == 0 ? reduce_clamp(v) : v;
    }
    row[(size_t)z * 4] = run;
  }
}
// a running sum in place along g (outer = x, step = one y) or along r (outer = y, step = one x): one thread per line and (z, plane)
__global__ __launch_bounds__(256) void palette_build_prefix_kernel(unsigned long long* __restrict__ T, int outer_stride, int step) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= kBuildTab * kBuildTab * 4) return;
  unsigned long long* p = T + (size_t)(i / (kBuildTab * 4)) * outer_stride + i % (kBuildTab * 4);
  unsigned long long run = 0ull;
  for (int k = 0; k < kBuildTab; ++k) {
    run += p[(size_t)k * step];
    p[(size_t)k * step] = run;
  }
}

// ---- the chain ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ BuildKey build_shfl_xor(const BuildKey& k, int o) {
  BuildKey t;
#pragma unroll
  for (int i = 0; i < 3; ++i) t.num[i] = __shfl_xor(k.num[i], o, 64);
  t.den[0] = __shfl_xor(k.den[0], o, 64);
  t.den[1] = __shfl_xor(k.den[1], o, 64);
  t.idx = __shfl_xor(k.idx, o, 64);
  return t;
}
// the first key of the wave in every lane: the order is total (no two live keys share an idx), so every lane ends on the same key
__device__ __forceinline__ BuildKey build_wave_first(BuildKey k) {
  for (int o = 32; o > 0; o >>= 1) {
    const BuildKey t = build_shfl_xor(k, o);
    if (build_before(t, k)) k = t;
  }
  return k;
}

__global__ __launch_bounds__(kBuildBlock) void palette_build_chain_kernel(const BuildSum* __restrict__ T, int K_target, uint8_t* __restrict__ pal_out,
                                                                          unsigned long long* __restrict__ counts_out, uint8_t* __restrict__ boxes_out,
                                                                          int32_t* __restrict__ splits, int32_t* __restrict__ k_out) {
  __shared__ unsigned long long s_num[3][kBuildMaxRows], s_den[2][kBuildMaxRows];      // the gain of every box's best cut
  __shared__ BuildBox s_box[kBuildMaxRows];
  __shared__ uint8_t s_cut[kBuildMaxRows];                                              // its code, kBuildNoCut: the box has no valid cut
  __shared__ BuildKey s_new[kBuildWaves], s_best[kBuildWaves];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;

  const unsigned long long total = T[build_tab_index(kBuildSide, kBuildSide, kBuildSide)].n;
  if (total == 0ull || total > kReduceMaxSum) {                                        // (block uniform)
    for (int j = tid; j < K_target * 3; j += kBuildBlock) pal_out[j] = 0;
    for (int j = tid; j < K_target; j += kBuildBlock) counts_out[j] = 0ull;
    if (boxes_out)
      for (int j = tid; j < K_target * 6; j += kBuildBlock) boxes_out[j] = 0;
    if (splits)
      for (int j = tid; j < (K_target - 1) * 3; j += kBuildBlock) splits[j] = -1;
    if (tid == 0) *k_out = total == 0ull ? RHCCQ_E_ARG : RHCCQ_E_LIMIT;
    return;
  }

  int nb = 1, done = 0;
  int id_a = 0, id_b = -1;                                                             // the boxes whose best cut is not known yet
  BuildBox box_a = build_whole(), box_b = build_whole();
  for (;;) {
    // the candidate cuts of the new boxes: waves 0 and 1 take box a, waves 2 and 3 box b, a lane one code
    BuildKey k = build_no_key();
    if (wv < 2 || id_b >= 0) k = build_cut_key(T, wv < 2 ? box_a : box_b, (wv & 1) * 64 + lane);
    k = build_wave_first(k);
    if (lane == 0) s_new[wv] = k;
    __syncthreads();
    if (tid == 0) {
      for (int h = 0; h < (id_b >= 0 ? 2 : 1); ++h) {
        const BuildKey best = build_before(s_new[h * 2 + 1], s_new[h * 2]) ? s_new[h * 2 + 1] : s_new[h * 2];
        const int id = h ? id_b : id_a;
        for (int i = 0; i < 3; ++i) s_num[i][id] = best.num[i];
        s_den[0][id] = best.den[0];
        s_den[1][id] = best.den[1];
        s_cut[id] = build_has_cut(best) ? (uint8_t)best.idx : kBuildNoCut;
        s_box[id] = h ? box_b : box_a;
      }
    }
    __syncthreads();
    if (nb >= K_target) break;

    // arg-max over the boxes: the largest gain, the lowest box among equals
    BuildKey best = build_no_key();
    for (int j = tid; j < nb; j += kBuildBlock) {
      if (s_cut[j] == kBuildNoCut) continue;
      const BuildKey c = {{s_num[0][j], s_num[1][j], s_num[2][j]}, {s_den[0][j], s_den[1][j]}, (uint32_t)j};
      if (build_before(c, best)) best = c;
    }
    best = build_wave_first(best);
    if (lane == 0) s_best[wv] = best;
    __syncthreads();
    best = s_best[0];
    for (int i = 1; i < kBuildWaves; ++i)
      if (build_before(s_best[i], best)) best = s_best[i];
    if (!build_has_cut(best)) break;                                                   // no box has a valid cut (block uniform)

    // the split: the box keeps its index and becomes the lower half, the upper half takes the next index (stored by lane 0 above, behind
    // the next barrier: every lane has read s_box and s_cut by then)
    id_a = (int)best.idx;
    id_b = nb++;
    const int code = (int)s_cut[id_a];
    box_a = s_box[id_a];
    box_b = build_split(box_a, code);
    if (tid == 0 && splits) {
      splits[done * 3] = id_a;
      splits[done * 3 + 1] = code >> 5;
      splits[done * 3 + 2] = code & (kBuildSide - 1);
    }
    ++done;
  }

  for (int j = tid; j < nb; j += kBuildBlock) {
    const BuildBox box = s_box[j];
    build_row(build_box_sum(T, box), pal_out + j * 3, counts_out + j);
    if (boxes_out)
      for (int i = 0; i < 3; ++i) {
        boxes_out[j * 6 + i] = box.lo[i];
        boxes_out[j * 6 + 3 + i] = box.hi[i];
      }
  }
  for (int j = nb * 3 + tid; j < K_target * 3; j += kBuildBlock) pal_out[j] = 0;
  for (int j = nb + tid; j < K_target; j += kBuildBlock) counts_out[j] = 0ull;
  if (boxes_out)
    for (int j = nb * 6 + tid; j < K_target * 6; j += kBuildBlock) boxes_out[j] = 0;
  if (splits)
    for (int j = done * 3 + tid; j < (K_target - 1) * 3; j += kBuildBlock) splits[j] = -1;
  if (tid == 0) *k_out = nb;
}

static int cells_check(rhccq_ctx* ctx, const void* rgb, int64_t n_pixels, const void* cls, int32_t n_classes, const int32_t* weights, const void* cells,
                       CellsWeights* wt) {
  if (!rgb || !cells) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: null argument");
  if (n_pixels < 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: n_pixels >= 0 is required");
  if (n_classes < 0 || n_classes > kRemapMaxClasses) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: n_classes must be 0..16");
  if (!cls && n_classes != 0) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: n_classes must be 0 without a class map");
  uint32_t top = 0u;
  for (int i = 0; i <= n_classes; ++i) {
    const int32_t w = weights ? weights[i] : 1;
    if (w < 0 || w > 255) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: weights must be 0..255");
    wt->w[i] = (uint32_t)w;
    top = (uint32_t)w > top ? (uint32_t)w : top;
  }
  if (!top) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: at least one weight must be > 0");
  if ((uintptr_t)cells & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_cells: misaligned cells (8)");
  if ((uint64_t)n_pixels > kCellsMaxSum / top) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_cells: n_pixels x the largest weight exceeds 2^32 - 1");
  return 0;
}

static int build_check(rhccq_ctx* ctx, const void* cells, int32_t K_target, const void* palette_out, const void* counts_out, const void* splits,
                       const void* k_out) {
  if (!cells || !palette_out || !counts_out || !k_out) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: null argument");
  if (K_target < 1) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: K_target >= 1 is required");
  if (((uintptr_t)cells & 7) || ((uintptr_t)counts_out & 7) || ((uintptr_t)splits & 3) || ((uintptr_t)k_out & 3))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: misaligned cells, counts_out (8), splits or k_out (4)");
  if (K_target > kBuildHostMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build: at most 32768 colours");
  return 0;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int32_t rhccq_palette_cells_block(void) { return kCellsBlock; }
int32_t rhccq_palette_cells_chunk(void) { return kCellsChunk; }
int32_t rhccq_palette_build_max_rows(void) { return kBuildMaxRows; }
int64_t rhccq_palette_build_bytes(void) { return (int64_t)kBuildTabEntries * (int64_t)sizeof(BuildSum); }

int rhccq_palette_cells(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights_host,
                        int32_t accumulate, uint64_t* cells) {
  if (!ctx) return RHCCQ_E_ARG;
  CellsWeights wt = {};
  if (const int rc = cells_check(ctx, rgb, n_pixels, cls, n_classes, weights_host, cells, &wt)) return rc;
  if (!accumulate) RHCCQ_HIP(ctx, hipMemsetAsync(cells, 0, (size_t)kBuildCells * 4 * sizeof(uint64_t), ctx->stream));
  if (n_pixels == 0) return 0;
  if (ctx->compute_units <= 0) RHCCQ_HIP(ctx, hipDeviceGetAttribute(&ctx->compute_units, hipDeviceAttributeMultiprocessorCount, ctx->device));
  const long long chunks = (n_pixels + kCellsChunk - 1) / kCellsChunk, cap = (long long)ctx->compute_units * 4;
  const long long blocks = chunks < cap ? chunks : cap;
  hipLaunchKernelGGL(palette_cells_kernel, dim3((unsigned)(blocks < 1 ? 1 : blocks)), dim3(kCellsBlock), 0, ctx->stream, rgb, (long long)n_pixels, cls,
                     (int)n_classes, wt, (unsigned long long*)cells);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_cells_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights, int32_t accumulate,
                             uint64_t* cells) {
  CellsWeights wt = {};
  if (const int rc = cells_check(nullptr, rgb, n_pixels, cls, n_classes, weights, cells, &wt)) return rc;
  if (!accumulate)
    for (int j = 0; j < kBuildCells * 4; ++j) cells[j] = 0;
  for (int64_t p = 0; p < n_pixels; ++p) {
    const uint64_t w = wt.w[n_classes > 0 && cls[p] < n_classes ? cls[p] : n_classes];
    const int cell = build_cell(rgb[p * 3], rgb[p * 3 + 1], rgb[p * 3 + 2]);
    cells[cell] += w;
    for (int ch = 0; ch < 3; ++ch) cells[(size_t)(ch + 1) * kBuildCells + cell] += w * rgb[p * 3 + ch];
  }
  return 0;
}

int rhccq_palette_build(rhccq_ctx* ctx, const uint64_t* cells, int32_t K_target, void* work, int64_t work_bytes, uint8_t* palette_out,
                        uint64_t* counts_out, uint8_t* boxes_out, int32_t* splits, int32_t* k_out) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!work) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: null argument");
  if (const int rc = build_check(ctx, cells, K_target, palette_out, counts_out, splits, k_out)) return rc;
  if ((uintptr_t)work & 7) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: misaligned workspace");
  if (K_target > kBuildMaxRows) return rhccq_fail(ctx, RHCCQ_E_LIMIT, "palette_build: more rows than rhccq_palette_build_max_rows() (the host form takes up to 32768)");
  if (work_bytes < rhccq_palette_build_bytes()) return rhccq_fail(ctx, RHCCQ_E_ARG, "palette_build: the workspace is smaller than rhccq_palette_build_bytes()");
  unsigned long long* T = (unsigned long long*)work;
  const dim3 grid((unsigned)((kBuildTab * kBuildTab * 4 + 255) / 256)), block(256);
  hipLaunchKernelGGL(palette_build_prefix_b_kernel, grid, block, 0, ctx->stream, (const unsigned long long*)cells, T);
  hipLaunchKernelGGL(palette_build_prefix_kernel, grid, block, 0, ctx->stream, T, kBuildTab * kBuildTab * 4, kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_prefix_kernel, grid, block, 0, ctx->stream, T, kBuildTab * 4, kBuildTab * kBuildTab * 4);
  hipLaunchKernelGGL(palette_build_chain_kernel, dim3(1), dim3(kBuildBlock), 0, ctx->stream, (const BuildSum*)work, (int)K_target, palette_out,
                     (unsigned long long*)counts_out, boxes_out, splits, k_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_palette_build_host(const uint64_t* cells, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out, uint8_t* boxes_out, int32_t* splits,
                             int32_t* k_out) {
  if (const int rc = build_check(nullptr, cells, K_target, palette_out, counts_out, splits, k_out)) return rc;
  std::vector<BuildSum> T((size_t)kBuildTabEntries, BuildSum{0ull, {0ull, 0ull, 0ull}});
  for (int x = 1; x < kBuildTab; ++x)
    for (int y = 1; y < kBuildTab; ++y)
      for (int z = 1; z < kBuildTab; ++z) {
        const int c = ((x - 1) * kBuildSide + (y - 1)) * kBuildSide + (z - 1);
        BuildSum v = {reduce_clamp(cells[c]), {cells[kBuildCells + c], cells[2 * kBuildCells + c], cells[3 * kBuildCells + c]}};
        v = build_add(v, T[build_tab_index(x - 1, y, z)]);
        v = build_add(v, T[build_tab_index(x, y - 1, z)]);
        v = build_add(v, T[build_tab_index(x, y, z - 1)]);
        v = build_sub(v, T[build_tab_index(x - 1, y - 1, z)]);
        v = build_sub(v, T[build_tab_index(x - 1, y, z - 1)]);
        v = build_sub(v, T[build_tab_index(x, y - 1, z - 1)]);
        T[build_tab_index(x, y, z)] = build_add(v, T[build_tab_index(x - 1, y - 1, z - 1)]);
      }
  const unsigned long long total = T[build_tab_index(kBuildSide, kBuildSide, kBuildSide)].n;
  if (total == 0ull) return RHCCQ_E_ARG;
  if (total > kReduceMaxSum) return RHCCQ_E_LIMIT;
  std::vector<BuildBox> box(1, build_whole());
  std::vector<BuildKey> key(1, build_best_cut(T.data(), box[0]));
  int done = 0;
  while ((int)box.size() < K_target) {
    BuildKey best = build_no_key();
    for (size_t j = 0; j < box.size(); ++j) {
      BuildKey c = key[j];
      c.idx = (uint32_t)j;
      if (build_before(c, best)) best = c;
    }
    if (!build_has_cut(best)) break;
    const int a = (int)best.idx, code = (int)key[a].idx;
    box.push_back(build_split(box[a], code));
    key[a] = build_best_cut(T.data(), box[a]);
    key.push_back(build_best_cut(T.data(), box.back()));
    if (splits) {
      splits[done * 3] = a;
      splits[done * 3 + 1] = code >> 5;
      splits[done * 3 + 2] = code & (kBuildSide - 1);
    }
    ++done;
  }
  const int nb = (int)box.size();
  for (int j = 0; j < K_target; ++j) {
    if (j < nb) build_row(build_box_sum(T.data(), box[j]), palette_out + j * 3, (unsigned long long*)counts_out + j);
    else {
      palette_out[j * 3] = palette_out[j * 3 + 1] = palette_out[j * 3 + 2] = 0;
      counts_out[j] = 0;
    }
    if (boxes_out)
      for (int i = 0; i < 3; ++i) {
        boxes_out[j * 6 + i] = j < nb ? box[j].lo[i] : 0;
        boxes_out[j * 6 + 3 + i] = j < nb ? box[j].hi[i] : 0;
      }
  }
  if (splits)
    for (int j = done * 3; j < (K_target - 1) * 3; ++j) splits[j] = -1;
  *k_out = nb;
  return 0;
}

}  // extern "C"
