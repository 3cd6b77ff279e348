// JPEG files read as a batch (EXTENSION, include/rhccq.h "JPEG files read as a batch"): the stages of jpeg_read.hip with workgroups that
// belong to files.  The step functions (kept, run<>, pack, geo_of, block_at, the sums that restart, the IDCT and the colour arithmetic)
// are jpeg_read.h's, unchanged, so a file decodes to the bytes it decodes to alone.
//
// A kernel takes the batch (the upload with the job table at its start, the workspace) and, where its grid is a padded one, a map: row w
// is {file, first unit in the file} of workgroup w.  A workgroup reads its job through one uniform index, so the job's fields come in
// as scalar loads, and builds from them what the single-file launch passes by value (Dec, Geo).
//
//   head_b             uint32[n_files][8]: the heads.
//   unstuff_b<false / true>  a workgroup a tile of one file; the counts go to the file's own tiles, the scatter to its own stream.
//   scan_b             a workgroup a file: the exclusive prefix sums of its tiles, from 0.
//   sync_b             256 subsequences of one file a workgroup, that file's tables in LDS; the first lane of a file's first workgroup
//                      holds the truth.  The rounds go to the file's head[2].
//   boundary_b         a workgroup a file walks that file's boundaries; a file of one workgroup returns at once.  The files' walks run
//                      side by side, where a loop of single-file decodes runs them one after the other.
//   place_b            a workgroup a file.
//   write_b            as sync_b's first decode, from the true entries, into the file's coefficients; faults to the file's head[0].
//   dc_b<false / true>, dc_carry_b  a tile is one (file, component)'s; the carries a workgroup a file.
//   idct_b, colour_b   32 blocks or 256 quads of one file; the image starts at a multiple of 16 bytes, so the quads' words are aligned.
//   finish_b           a lane a file: status[n_files][2], from the parse's status or from head[0].
#include "jpeg_read.h"
#include "rhccq_common.h"

#include <vector>

namespace rhccq {
namespace jpegr {

constexpr int kBatchMaxFiles = 65536;
constexpr int kMaps = 5;

struct Batch {
  const uint8_t* up;                                       // the upload: rhccq_jpeg_job[n_files] at 0
  uint8_t* ws;                                             // the workspace: uint32[n_files][8] at 0
  __device__ __forceinline__ const rhccq_jpeg_job& job(uint32_t f) const { return ((const rhccq_jpeg_job*)up)[f]; }
  __device__ __forceinline__ uint32_t* head(uint32_t f) const { return (uint32_t*)ws + 8 * (size_t)f; }
  __device__ __forceinline__ const rhccq_jpeg_tables* tables(const rhccq_jpeg_job& j) const { return (const rhccq_jpeg_tables*)(up + j.tables_offset); }
  __device__ __forceinline__ SubRow* rows(const rhccq_jpeg_job& j) const { return (SubRow*)(ws + j.o_rows); }
  __device__ __forceinline__ uint32_t* first(const rhccq_jpeg_job& j) const { return (uint32_t*)(ws + j.o_first); }
  __device__ __forceinline__ int16_t* coef(const rhccq_jpeg_job& j) const { return (int16_t*)(ws + j.o_coef); }
  __device__ __forceinline__ uint64_t* agg(const rhccq_jpeg_job& j) const { return (uint64_t*)(ws + j.o_agg); }
  // the file's decoder; T is the caller's copy in LDS
  __device__ __forceinline__ Dec dec(const rhccq_jpeg_job& j, const rhccq_jpeg_tables* T) const {
    Dec d;
    d.words = (const uint32_t*)(ws + j.o_stream);
    d.T = T;
    d.iv = (const rhccq_segment*)(up + j.intervals_offset);
    d.n_iv = j.info.n_intervals;
    d.total_bits = 8 * j.info.stream_bytes;
    d.g = geo_of(j.info);
    return d;
  }
};

__global__ __launch_bounds__(kThreads) void head_b(Batch b, int n_files) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 8ll * n_files) return;
  const int k = (int)(i & 7);
  ((uint32_t*)b.ws)[i] = k == 0 ? kNoInterval : k == 1 ? (uint32_t)b.job((uint32_t)(i >> 3)).n_sub : 0u;
}
__global__ __launch_bounds__(kThreads) void finish_b(Batch b, int n_files, int32_t* __restrict__ status) {
  const int f = blockIdx.x * kThreads + threadIdx.x;
  if (f >= n_files) return;
  const rhccq_jpeg_info& info = b.job(f).info;
  const uint32_t bad = b.head(f)[0];
  status[2 * f] = info.status ? info.status : bad == kNoInterval ? RHCCQ_JPEG_OK : RHCCQ_JPEG_BAD_SCAN;
  status[2 * f + 1] = info.status ? info.detail : bad == kNoInterval ? 0 : (int32_t)bad;
}

// ---- unstuff -------------------------------------------------------------------------------------------------------------------------
template <bool SCATTER>
__global__ __launch_bounds__(kThreads) void unstuff_b(Batch b, const uint2* __restrict__ map) {
  __shared__ uint32_t s_red[kThreads / 64 + 1];
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  const uint8_t* file = b.up + j.file_offset;
  const long long n = j.file_bytes, lo = j.info.scan_offset, len = j.info.scan_bytes, stream_bytes = j.info.stream_bytes;
  uint32_t* tiles = (uint32_t*)(b.ws + j.o_tiles);
  uint8_t* stream = b.ws + j.o_stream;
  const long long p0 = lo + ((long long)m.y * kThreads + threadIdx.x) * 16;
  uint32_t mask = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k)
    if (p0 + k < lo + len && kept(file, n, lo, p0 + k)) mask |= 1u << k;
  uint32_t total;
  const uint32_t excl = block_exscan<uint32_t>(__popc(mask), s_red, &total);
  if (!SCATTER) {
    if (threadIdx.x == 0) tiles[m.y] = total;
    return;
  }
  long long at = (long long)tiles[m.y] + excl;
  for (int k = 0; k < 16; ++k)
    if (mask >> k & 1u) {
      if (at < stream_bytes) stream[at] = file[p0 + k];
      ++at;
    }
  if (m.y == 0 && threadIdx.x < kStreamPad) stream[stream_bytes + threadIdx.x] = 0;
}
// a file's tiles -> their exclusive prefix sums in place: the sum restarts with the file, so its stream lands at its own base
__global__ __launch_bounds__(kThreads) void scan_b(Batch b) {
  __shared__ uint32_t s_red[kThreads / 64 + 1];
  const rhccq_jpeg_job& j = b.job(blockIdx.x);
  uint32_t* v = (uint32_t*)(b.ws + j.o_tiles);
  const long long count = j.n_tiles;                                 // (0 for a file with a status)
  uint32_t run = 0;
  for (long long i0 = 0; i0 < count; i0 += kThreads) {               // (uniform)
    const long long i = i0 + threadIdx.x;
    uint32_t total;
    const uint32_t x = i < count ? v[i] : 0u, excl = block_exscan<uint32_t>(x, s_red, &total);
    if (i < count) v[i] = run + excl;
    run += total;
  }
}

// ---- sync ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void sync_b(Batch b, const uint2* __restrict__ map, int S) {
  __shared__ rhccq_jpeg_tables s_T;
  __shared__ uint64_t s_leave[kThreads];
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  tables_to_lds(&s_T, b.tables(j));
  const Dec d = b.dec(j, &s_T);
  const int tid = threadIdx.x;
  const long long g = (long long)m.y + tid;                          // the subsequence in its file
  const bool live = g < j.n_sub;
  const long long end = sub_end(d, S, g);
  uint64_t entry = pack(g * S, 0, 0), leave = 0;
  uint32_t count = 0;
  if (live) run<false>(d, entry, g == 0, end, 0, nullptr, nullptr, &leave, &count);
  uint32_t rounds = 0;
  for (int r = 0; r < kThreads; ++r) {                               // (uniform: the vote decides)
    s_leave[tid] = leave;
    __syncthreads();
    const uint64_t want = live && tid > 0 ? s_leave[tid - 1] : entry;
    const bool changed = want != entry;
    if (!__syncthreads_or(changed)) break;
    if (changed) {
      entry = want;
      run<false>(d, entry, false, end, 0, nullptr, nullptr, &leave, &count);
    }
    ++rounds;
  }
  if (live) b.rows(j)[g] = SubRow{entry, leave, count, 0u};
  if (tid == 0) atomicMax(&b.head(m.x)[2], rounds);
}

// jpeg_read.hip's boundary_kernel over the file blockIdx.x names: rounds bounded by the file's own workgroups
__global__ __launch_bounds__(kThreads) void boundary_b(Batch b, int S) {
  __shared__ rhccq_jpeg_tables s_T;
  __shared__ uint64_t s_tail[kThreads];
  const rhccq_jpeg_job& j = b.job(blockIdx.x);
  const long long n_sub = j.n_sub;
  if (n_sub <= kThreads) return;                                     // (uniform) one workgroup, or a file with a status: no boundary
  tables_to_lds(&s_T, b.tables(j));
  const Dec d = b.dec(j, &s_T);
  SubRow* rows = b.rows(j);
  uint32_t* head = b.head(blockIdx.x);
  const int tid = threadIdx.x;
  const long long n_wg = (n_sub + kThreads - 1) / kThreads;
  uint64_t carry = rows[kThreads - 1].leave;
  uint32_t rounds = 0, walk = 0;
  for (long long c0 = 1; c0 < n_wg; c0 += kThreads) {               // (uniform)
    const long long w = c0 + tid, g_lo = w * kThreads, g_hi = g_lo + kThreads < n_sub ? g_lo + kThreads : n_sub;
    const bool live = w < n_wg;
    uint64_t tail = live ? rows[g_hi - 1].leave : 0;
    s_tail[tid] = tail;
    for (int r = 0; r <= kThreads; ++r) {                            // (uniform)
      __syncthreads();
      uint64_t want = tid == 0 ? carry : s_tail[tid - 1];
      bool moved = false;
      if (live) {
        long long g = g_lo;
        uint32_t steps = 0;
        while (g < g_hi && rows[g].entry != want) {
          uint64_t leave;
          uint32_t count;
          run<false>(d, want, false, sub_end(d, S, g), 0, nullptr, nullptr, &leave, &count);
          rows[g] = SubRow{want, leave, count, 0u};
          want = leave;
          ++g;
          ++steps;
        }
        walk = steps > walk ? steps : walk;
        moved = steps > 0 && g == g_hi && want != tail;
      }
      const int any = __syncthreads_or(moved);                       // (every lane has read its neighbour's tail)
      if (moved) s_tail[tid] = tail = want;
      if (!any) break;
      ++rounds;
    }
    __syncthreads();
    carry = s_tail[kThreads - 1];
    __syncthreads();
  }
  atomicMax(&head[4], walk);
  if (tid == 0) head[3] = rounds;
}

__global__ __launch_bounds__(kThreads) void place_b(Batch b) {
  __shared__ uint64_t s_w[kThreads / 64];
  const rhccq_jpeg_job& j = b.job(blockIdx.x);
  const long long n_sub = j.n_sub;
  if (n_sub < 1) return;                                             // (uniform) a file with a status
  const SubRow* rows = b.rows(j);
  uint32_t* first = b.first(j);
  uint64_t run = 1ull << 32;                                         // block 0, absolute
  if (threadIdx.x == 0) first[0] = 0u;
  for (long long g0 = 0; g0 < n_sub; g0 += kThreads) {              // (uniform)
    const long long g = g0 + threadIdx.x;
    const uint32_t c = g < n_sub ? rows[g].count : 0u;
    uint64_t total;
    const uint64_t incl = seg_block_scan((uint64_t)(c >> 31) << 32 | (c & ~kAbs), s_w, &total);
    if (g < n_sub) first[g + 1] = (uint32_t)seg_combine(run, incl);
    run = seg_combine(run, total);
  }
}

__global__ __launch_bounds__(kThreads) void write_b(Batch b, const uint2* __restrict__ map, int S) {
  __shared__ rhccq_jpeg_tables s_T;
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  tables_to_lds(&s_T, b.tables(j));
  const Dec d = b.dec(j, &s_T);
  const long long g = (long long)m.y + threadIdx.x;
  if (g >= j.n_sub) return;
  uint64_t leave;
  uint32_t count;
  run<true>(d, b.rows(j)[g].entry, g == 0, sub_end(d, S, g), (long long)b.first(j)[g], b.coef(j), &b.head(m.x)[0], &leave, &count);
}

// ---- dc ------------------------------------------------------------------------------------------------------------------------------
template <bool FINAL>
__global__ __launch_bounds__(kThreads) void dc_b(Batch b, const uint2* __restrict__ map) {
  __shared__ uint64_t s_w[kThreads / 64];
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  const Geo g = geo_of(j.info);
  int16_t* coef = b.coef(j);
  uint64_t* agg = b.agg(j);
  int c = 0;
  long long t = m.y;                                                 // the tile in its file, through the components
  DcSeq s = dc_seq(g, 0);
  while (c + 1 < g.n_comp && t >= s.tiles) {                         // (uniform)
    t -= s.tiles;
    s = dc_seq(g, ++c);
  }
  const long long q = t * kThreads + threadIdx.x;
  const bool live = q < s.len;
  const long long mcu = q / s.nb;
  const int k = (int)(q - mcu * s.nb);
  int16_t* at = coef + 64 * block_at(g, live ? mcu * g.bpm + s.b0 + k : 0);
  const bool starts = live && k == 0 && (g.R ? mcu % g.R == 0 : mcu == 0);
  const uint32_t v = live ? (uint32_t)(int32_t)*at : 0u;
  uint64_t total;
  const uint64_t incl = seg_block_scan((uint64_t)starts << 32 | v, s_w, &total);
  if (!FINAL) {
    if (threadIdx.x == 0) agg[m.y] = total;
    return;
  }
  if (live) *at = (int16_t)(uint32_t)seg_combine(agg[m.y], incl);
}
__global__ __launch_bounds__(kThreads) void dc_carry_b(Batch b) {
  __shared__ uint64_t s_w[kThreads / 64];
  __shared__ uint64_t s_x[kThreads];
  const rhccq_jpeg_job& j = b.job(blockIdx.x);
  if (j.n_dc_tiles < 1) return;                                      // (uniform) a file with a status
  const Geo g = geo_of(j.info);
  uint64_t* agg = b.agg(j);
  long long base = 0;
  for (int c = 0; c < g.n_comp; ++c) {                               // (uniform)
    const DcSeq s = dc_seq(g, c);
    uint64_t run = 0;
    for (long long t0 = 0; t0 < s.tiles; t0 += kThreads) {          // (uniform)
      const long long t = t0 + threadIdx.x;
      uint64_t total;
      const uint64_t incl = seg_block_scan(t < s.tiles ? agg[base + t] : 0ull, s_w, &total);
      s_x[threadIdx.x] = incl;
      __syncthreads();
      if (t < s.tiles) agg[base + t] = seg_combine(run, threadIdx.x ? s_x[threadIdx.x - 1] : 0ull) & 0xFFFFFFFFull;
      run = seg_combine(run, total);
      __syncthreads();
    }
    base += s.tiles;
  }
}

// ---- idct, colour --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void idct_b(Batch b, const uint2* __restrict__ map) {
  __shared__ uint16_t s_q[3][64];
  __shared__ int32_t s_ws[kIdctBlocks][8][9];
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  const Geo g = geo_of(j.info);
  const int16_t* coef = b.coef(j);
  uint8_t* planes = b.ws + j.o_planes;
  if (threadIdx.x < 192) s_q[threadIdx.x >> 6][threadIdx.x & 63] = b.tables(j)->quant[threadIdx.x >> 6][threadIdx.x & 63];
  __syncthreads();
  const int slot = threadIdx.x >> 3, l = threadIdx.x & 7;
  const long long B = (long long)m.y + slot;                         // the block in its file
  const bool live = B < g.blocks;
  const int c = g.n_comp == 3 && B >= g.base[2] ? 2 : g.n_comp == 3 && B >= g.base[1] ? 1 : 0;
  if (live) {
    int32_t y[8];
    idct_column(coef + 64 * B, s_q[c], l, y);
#pragma unroll
    for (int r = 0; r < 8; ++r) s_ws[slot][r][l] = y[r];
  }
  __syncthreads();
  if (!live) return;
  int32_t x[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) x[k] = s_ws[slot][l][k];
  union { uint8_t b[8]; uint2 w; } out;
  idct_row(x, out.b);
  const long long blk = B - g.base[c], by = blk / g.bw[c], bx = blk - by * g.bw[c];
  *(uint2*)(planes + 64 * g.base[c] + (8 * by + l) * (8 * (long long)g.bw[c]) + 8 * bx) = out.w;
}

__global__ __launch_bounds__(kThreads) void colour_b(Batch b, const uint2* __restrict__ map, uint8_t* __restrict__ rgb_all) {
  const uint2 m = map[blockIdx.x];
  const rhccq_jpeg_job& j = b.job(m.x);
  const Geo g = geo_of(j.info);
  const uint8_t* planes = b.ws + j.o_planes;
  uint8_t* rgb = rgb_all + j.o_rgb;                                  // a multiple of 16: 3 p0 is one of 12, the words are aligned
  const long long p0 = ((long long)m.y + threadIdx.x) * 4, hw = (long long)g.H * g.W;
  if (p0 >= hw) return;
  union { uint8_t b[12]; uint32_t w[3]; } out;
  const int n = hw - p0 < 4 ? (int)(hw - p0) : 4;
  for (int k = 0; k < n; ++k) {
    int y, x;
    rhccq_row_col(p0 + k, g.W, y, x);
    rgb_at(g, planes, y, x, out.b + 3 * k);
  }
  if (n == 4) {
    uint32_t* dst = (uint32_t*)(rgb + 3 * p0);
    dst[0] = out.w[0], dst[1] = out.w[1], dst[2] = out.w[2];
  } else {
    for (int k = 0; k < 3 * n; ++k) rgb[3 * p0 + k] = out.b[k];
  }
}

// ---- the layout ----------------------------------------------------------------------------------------------------------------------
static int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }
static int sub_bits(int32_t s) { return s ? s : kSubBits; }

// a file's workgroups in the five padded grids and the units one of them holds
struct Units { int64_t n_tiles, n_sub, n_dc, rows[kMaps], step[kMaps]; };
static Units units_of(const rhccq_jpeg_info& f, int S) {
  Units u{};
  if (f.status != RHCCQ_JPEG_OK) return u;
  u.n_tiles = f.scan_bytes > 0 ? (f.scan_bytes + kTileBytes - 1) / kTileBytes : 1;
  u.n_sub = sub_count(f.stream_bytes, S);
  u.n_dc = dc_tiles(geo_of(f));
  const int64_t quads = ((int64_t)f.width * f.height + 3) / 4;
  u.rows[RHCCQ_JPEG_MAP_UNSTUFF] = u.n_tiles, u.step[RHCCQ_JPEG_MAP_UNSTUFF] = 1;
  u.rows[RHCCQ_JPEG_MAP_SUB] = (u.n_sub + kThreads - 1) / kThreads, u.step[RHCCQ_JPEG_MAP_SUB] = kThreads;
  u.rows[RHCCQ_JPEG_MAP_DC] = u.n_dc, u.step[RHCCQ_JPEG_MAP_DC] = 1;
  u.rows[RHCCQ_JPEG_MAP_IDCT] = (f.blocks + kIdctBlocks - 1) / kIdctBlocks, u.step[RHCCQ_JPEG_MAP_IDCT] = kIdctBlocks;
  u.rows[RHCCQ_JPEG_MAP_COLOUR] = (quads + kThreads - 1) / kThreads, u.step[RHCCQ_JPEG_MAP_COLOUR] = kThreads;
  return u;
}

// the sizes, and with `upload` the job table and the maps written into it
static int plan(const rhccq_jpeg_info* infos, const int64_t* file_bytes, int32_t n_files, int32_t subsequence_bits, uint8_t* upload, int64_t cap,
                rhccq_jpeg_batch* out, std::vector<rhccq_jpeg_job>& jobs) {
  if (!infos || !file_bytes || !out || n_files < 1 || !sub_bits_ok(subsequence_bits)) return RHCCQ_E_ARG;
  if (n_files > kBatchMaxFiles) return RHCCQ_E_LIMIT;
  const int S = sub_bits(subsequence_bits);
  rhccq_jpeg_batch b{};
  for (int i = 0; i < n_files; ++i) {
    if (infos[i].status == RHCCQ_JPEG_OK && !info_sound(infos[i], file_bytes[i])) return RHCCQ_E_ARG;
    const Units u = units_of(infos[i], S);
    for (int k = 0; k < kMaps; ++k) b.map_rows[k] += u.rows[k];
  }
  int64_t up = align16((int64_t)sizeof(rhccq_jpeg_job) * n_files);
  for (int k = 0; k < kMaps; ++k) {
    if (b.map_rows[k] > kReadMax) return RHCCQ_E_LIMIT;
    b.o_maps[k] = up;
    up = align16(up + 8 * b.map_rows[k]);
  }
  // the workspace: the heads, every file's small arrays, all coefficients, all planes
  int64_t ws = align256(32 * (int64_t)n_files), coef = 0, planes = 0, rgb = 0;
  jobs.resize((size_t)n_files);
  for (int i = 0; i < n_files; ++i) {
    const rhccq_jpeg_info& f = infos[i];
    rhccq_jpeg_job& j = jobs[(size_t)i];
    memset(&j, 0, sizeof j);
    j.info = f;
    j.file_bytes = file_bytes[i];
    if (f.status != RHCCQ_JPEG_OK) continue;
    const Units u = units_of(f, S);
    j.n_tiles = u.n_tiles, j.n_sub = u.n_sub, j.n_dc_tiles = u.n_dc;
    j.tables_offset = up;
    j.intervals_offset = up + (int64_t)sizeof(rhccq_jpeg_tables);
    j.file_offset = j.intervals_offset + (int64_t)sizeof(rhccq_segment) * f.n_intervals;
    up = align16(j.file_offset + j.file_bytes);
    j.o_tiles = ws;
    j.o_stream = align256(j.o_tiles + 4 * u.n_tiles);
    j.o_rows = align256(j.o_stream + f.stream_bytes + kStreamPad);
    j.o_first = align256(j.o_rows + (int64_t)sizeof(SubRow) * u.n_sub);
    j.o_agg = align256(j.o_first + 4 * (u.n_sub + 1));
    ws = align256(j.o_agg + 8 * u.n_dc);
    j.o_coef = coef;                                       // (from the first file's; moved behind the small arrays below)
    coef += align256(128 * f.blocks);
    j.o_planes = planes;
    planes += align256(64 * f.blocks);
    j.o_rgb = rgb;
    rgb = align16(rgb + 3 * (int64_t)f.width * f.height);
    if (up > kReadMax || rgb > kReadMax) return RHCCQ_E_LIMIT;
  }
  b.o_coef = ws;
  b.coef_bytes = coef;
  b.upload_bytes = up;
  b.workspace_bytes = ws + coef + planes;
  b.rgb_bytes = rgb < 16 ? 16 : rgb;
  for (rhccq_jpeg_job& j : jobs)
    if (j.info.status == RHCCQ_JPEG_OK) j.o_coef += ws, j.o_planes += ws + coef;
  *out = b;
  if (!upload) return RHCCQ_OK;
  if (cap < b.upload_bytes || (uintptr_t)upload % 16) return RHCCQ_E_ARG;
  memcpy(upload, jobs.data(), sizeof(rhccq_jpeg_job) * (size_t)n_files);
  int64_t row[kMaps] = {0, 0, 0, 0, 0};
  for (int i = 0; i < n_files; ++i) {
    const Units u = units_of(infos[i], S);
    for (int k = 0; k < kMaps; ++k) {
      uint32_t* map = (uint32_t*)(upload + b.o_maps[k]);
      for (int64_t w = 0; w < u.rows[k]; ++w, ++row[k]) map[2 * row[k]] = (uint32_t)i, map[2 * row[k] + 1] = (uint32_t)(w * u.step[k]);
    }
  }
  return RHCCQ_OK;
}

}  // namespace jpegr
}  // namespace rhccq

using namespace rhccq;
using namespace rhccq::jpegr;

extern "C" {

int32_t rhccq_jpeg_batch_max_files(void) { return kBatchMaxFiles; }

int rhccq_jpeg_batch_sizes(const rhccq_jpeg_info* infos, const int64_t* file_bytes, int32_t n_files, int32_t subsequence_bits, rhccq_jpeg_batch* batch) {
  std::vector<rhccq_jpeg_job> jobs;
  return plan(infos, file_bytes, n_files, subsequence_bits, nullptr, 0, batch, jobs);
}

int rhccq_jpeg_batch_plan_host(const rhccq_jpeg_info* infos, const int64_t* file_bytes, int32_t n_files, int32_t subsequence_bits, void* upload, int64_t cap,
                               rhccq_jpeg_batch* batch) {
  if (!upload) return RHCCQ_E_ARG;
  std::vector<rhccq_jpeg_job> jobs;
  return plan(infos, file_bytes, n_files, subsequence_bits, (uint8_t*)upload, cap, batch, jobs);
}

int rhccq_jpeg_decode_batch(rhccq_ctx* ctx, const void* upload_dev, const rhccq_jpeg_job* jobs, int32_t n_files, int32_t subsequence_bits, void* workspace,
                            uint8_t* rgb, int32_t* status) {
  if (!ctx) return RHCCQ_E_ARG;
  if (!upload_dev || !jobs || !workspace || !rgb || !status || (uintptr_t)upload_dev % 256 || (uintptr_t)workspace % 256 || (uintptr_t)rgb % 16 ||
      (uintptr_t)status % 4 || n_files < 1 || n_files > kBatchMaxFiles)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_decode_batch: a null or misaligned pointer, or n_files outside 1..rhccq_jpeg_batch_max_files()");
  // the layout once more from the jobs' infos: the kernels' bounds rest on a job table that is the plan's
  std::vector<rhccq_jpeg_info> infos((size_t)n_files);
  std::vector<int64_t> sizes((size_t)n_files);
  for (int i = 0; i < n_files; ++i) infos[(size_t)i] = jobs[i].info, sizes[(size_t)i] = jobs[i].file_bytes;
  rhccq_jpeg_batch bt;
  std::vector<rhccq_jpeg_job> mine;
  if (plan(infos.data(), sizes.data(), n_files, subsequence_bits, nullptr, 0, &bt, mine))
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_decode_batch: the jobs' infos are not the parse's, or a bad subsequence_bits");
  if (memcmp(mine.data(), jobs, sizeof(rhccq_jpeg_job) * (size_t)n_files) != 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "jpeg_decode_batch: jobs is not rhccq_jpeg_batch_plan_host's table");
  const int S = sub_bits(subsequence_bits);
  Batch b{(const uint8_t*)upload_dev, (uint8_t*)workspace};
  const hipStream_t st = ctx->stream;
  const dim3 wg(kThreads), per_file((unsigned)n_files);
  auto map = [&](int k) { return (const uint2*)(b.up + bt.o_maps[k]); };
  auto grid = [&](int k) { return dim3((unsigned)bt.map_rows[k]); };
  hipLaunchKernelGGL(head_b, dim3((unsigned)((8 * n_files + kThreads - 1) / kThreads)), wg, 0, st, b, n_files);
  if (bt.map_rows[RHCCQ_JPEG_MAP_SUB] > 0) {                         // (else every file has a status)
    RHCCQ_HIP(ctx, hipMemsetAsync(b.ws + bt.o_coef, 0, (size_t)bt.coef_bytes, st));
    hipLaunchKernelGGL(unstuff_b<false>, grid(RHCCQ_JPEG_MAP_UNSTUFF), wg, 0, st, b, map(RHCCQ_JPEG_MAP_UNSTUFF));
    hipLaunchKernelGGL(scan_b, per_file, wg, 0, st, b);
    hipLaunchKernelGGL(unstuff_b<true>, grid(RHCCQ_JPEG_MAP_UNSTUFF), wg, 0, st, b, map(RHCCQ_JPEG_MAP_UNSTUFF));
    hipLaunchKernelGGL(sync_b, grid(RHCCQ_JPEG_MAP_SUB), wg, 0, st, b, map(RHCCQ_JPEG_MAP_SUB), S);
    hipLaunchKernelGGL(boundary_b, per_file, wg, 0, st, b, S);
    hipLaunchKernelGGL(place_b, per_file, wg, 0, st, b);
    hipLaunchKernelGGL(write_b, grid(RHCCQ_JPEG_MAP_SUB), wg, 0, st, b, map(RHCCQ_JPEG_MAP_SUB), S);
    hipLaunchKernelGGL(dc_b<false>, grid(RHCCQ_JPEG_MAP_DC), wg, 0, st, b, map(RHCCQ_JPEG_MAP_DC));
    hipLaunchKernelGGL(dc_carry_b, per_file, wg, 0, st, b);
    hipLaunchKernelGGL(dc_b<true>, grid(RHCCQ_JPEG_MAP_DC), wg, 0, st, b, map(RHCCQ_JPEG_MAP_DC));
    hipLaunchKernelGGL(idct_b, grid(RHCCQ_JPEG_MAP_IDCT), wg, 0, st, b, map(RHCCQ_JPEG_MAP_IDCT));
    hipLaunchKernelGGL(colour_b, grid(RHCCQ_JPEG_MAP_COLOUR), wg, 0, st, b, map(RHCCQ_JPEG_MAP_COLOUR), rgb);
  }
  hipLaunchKernelGGL(finish_b, dim3((unsigned)((n_files + kThreads - 1) / kThreads)), wg, 0, st, b, n_files, status);
  RHCCQ_LAUNCH_CHECK(ctx);
  return RHCCQ_OK;
}

}  // extern "C"
