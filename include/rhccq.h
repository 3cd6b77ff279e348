/* rhccq.h -- C ABI of the MI355X-native RHCCQ encoder hot path (librhccq_hip.so).
 *
 * Boundary: the reference has no FFI; its "interface" for this path is the Python
 * import surface encoder.compression.{clustering,merging,subregions,regions,image}.  The host side
 * stays in Python (roibasedimagecompression_amd/, mirrored under encoder/ and decoder/) and calls
 * the entry points below through ctypes.  Each entry point is a thin launcher of hand-written
 * gfx950 kernels; the reference function it replaces is cited next to it (paths relative to the
 * reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HIP, same device as the context) unless the parameter
 *     name ends in _host; buffers are caller-allocated (the Python side uses torch tensors);
 *   - every call is asynchronous on the context's HIP stream unless documented "synchronises";
 *   - return value: 0 on success, negative on error (RHCCQ_E_*); rhccq_last_error() gives text;
 *   - no exceptions cross the boundary; a context is not thread-safe, use one per thread;
 *   - colours travel as "keys": uint32 = R<<16 | G<<8 | B  (lexicographic order == numeric order).
 */
#ifndef RHCCQ_H
#define RHCCQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHCCQ_OK 0
#define RHCCQ_E_ARG (-1)     /* bad argument / shape */
#define RHCCQ_E_HIP (-2)     /* HIP runtime error */
#define RHCCQ_E_LIMIT (-3)   /* size beyond what the kernel supports */

#define RHCCQ_BITMAP_WORDS 524288u /* 2^24 colours / 32 bits: one unique-colour bitmap per job */
#define RHCCQ_EPS_LDS_MAX 10240    /* eps-components: problems up to this size run from LDS */
#define RHCCQ_KM_LDS_MAX 10240     /* k-means: problems up to this size keep their points in LDS */

typedef struct rhccq_ctx rhccq_ctx;

/* ---- context ------------------------------------------------------------------------------ */
int rhccq_ctx_create(int device, void* hip_stream /* NULL = the default (null) stream */, rhccq_ctx** out);
void rhccq_ctx_destroy(rhccq_ctx* ctx);
const char* rhccq_last_error(const rhccq_ctx* ctx);
/* Tuning knobs.  They only move the thresholds at which a kernel switches between two implementations of the
 * same computation (results never change); the test-suite lowers them to drive the large-input paths with inputs
 * the oracle can still check.
 *   RHCCQ_OPT_INIT_LDS_BLOCKS  k-means++ (rhccq_mbk_init): block tables live in LDS while the init sample has at
 *                              most this many 64-sample blocks (0..4096, default 4096), in global memory beyond;
 *   RHCCQ_OPT_INIT_MAX_ITEMS   capacity of the shared (candidate, block) work list (1..12288, default 12288);
 *                              picks that exceed it evaluate each candidate by its own enumeration instead;
 *   RHCCQ_OPT_INIT_KERNEL      0 (default): the newest k-means++ chain whose tables fit LDS -- third generation (leaves of 16
 *                              samples, box pruning) up to 98 304 init samples, second generation (blocks of 64) up to 262 144,
 *                              first generation beyond; 1: the first-generation chain always; 2: the second generation whenever
 *                              its tables fit; 3: same as 0; 4: brute force with the samples in registers (kpp_flat.h, at most
 *                              8 192 init samples; the chain KMeans uses); 5: the third generation with every candidate's improvement
 *                              summed by the wave that found it (no shared work list, two barriers per pick instead of three: measured
 *                              5 % SLOWER).  Same picks everywhere; the other chains serve other sizes and as
 *                              cross-checks;
 *   RHCCQ_OPT_INIT_CANDS_PER_WAVE  third-generation chain: how many of a pick's candidates ONE search wave finds and descends for,
 *                              as interleaved dependency chains of one instruction stream (1, 2 or 3; same picks);
 *   RHCCQ_OPT_REASSIGN_LDS     mini-batch steps that reassign low-count centres: 1 (default) = the five sweeps over the weights read
 *                              a 32-bit copy in LDS when k <= 30 720, 0 = always global memory (the path of larger k; same results);
 *   RHCCQ_OPT_INIT_SHARDS      workgroups (CUs) per problem of the second-generation chain: 1 (default) = one; 2 / 4 / 8 =
 *                              up to that many, each owning a range of the draws, when every shard keeps >= 4096 init
 *                              samples and at most 64 workgroups result (they wait for each other inside the launch, so
 *                              all must be resident).  Same picks; measured SLOWER than one workgroup (two cross-CU
 *                              exchanges per pick), kept as a checked alternative. */
#define RHCCQ_OPT_INIT_LDS_BLOCKS 1
#define RHCCQ_OPT_INIT_MAX_ITEMS 2
#define RHCCQ_OPT_INIT_KERNEL 3
#define RHCCQ_OPT_INIT_SHARDS 4
#define RHCCQ_OPT_INIT_CANDS_PER_WAVE 5
#define RHCCQ_OPT_REASSIGN_LDS 6
/*   RHCCQ_OPT_REASSIGN_ORDER   THE ONE OPTION THAT CHANGES RESULTS.  Which tied low-count centres a capped reassignment of a mini-batch
 *                              step takes (sklearn _mini_batch_step: np.argsort(weight_sums)[:batch / 2], an unstable sort):
 *                              1 (default) = the slots numpy's scalar aquicksort_<double> fills (csrc/k8_npysort.h; the whole fit then
 *                              equals scikit-learn's untouched fit_predict under NPY_DISABLE_CPU_FEATURES = <AVX512 family> AVX2
 *                              FMA3, the host setting of record), 0 = the stable order (weight, index) of rounds 1-3 (= sklearn
 *                              with that call forced to kind='stable'). */
#define RHCCQ_OPT_REASSIGN_ORDER 7
/*   RHCCQ_OPT_FRAME_CHAINS     rhccq_encode_frame: 1 (default) = the k-means++ chains of every level-1 MiniBatchKMeans problem of a
 *                              frame (init samples <= 98 304 each) are drawn, ordered and run in ONE launch on the context's
 *                              stream before the class pipelines start, which then wait for it; 0 = every problem draws and
 *                              runs its chain on its own lane.  Same results.  Why: the runtime maps the lanes' streams onto
 *                              GPU_MAX_HW_QUEUES hardware queues (4 by default); two streams on one queue run their kernels
 *                              one after the other, so a chain of one class could hold up the other class for its whole
 *                              length.  Every step after the chains needs them all, so one launch loses nothing. */
#define RHCCQ_OPT_FRAME_CHAINS 8
/*   RHCCQ_OPT_FRAME_LEVEL2     rhccq_encode_frame: 1 (default) = the class threads end with their merged component and the level-2
 *                              palettes of all classes are clustered in ONE call on one lane, with no other stream of the
 *                              frame at work: their MiniBatchKMeans problems are drawn, ordered, initialised, stepped
 *                              (rhccq_mbk_steps_batch) and assigned as one batch; 0 = every class clusters its level-2 palette on
 *                              its own lane.  Same results.  Why: two host threads and two streams that queue ~700 launches each
 *                              on the same few hardware queues ran their steps at twice the period of either alone. */
#define RHCCQ_OPT_FRAME_LEVEL2 9
/*   RHCCQ_OPT_REFINE_LDS_ROWS  rhccq_palette_refine: palettes of at most this many rows keep their accumulators in LDS per workgroup,
 *                              larger ones add to the workspace in global memory (0 .. rhccq_palette_refine_lds_rows(), default that
 *                              maximum; 0 = always global memory).  Same results: integer sums in any order;
 *   RHCCQ_OPT_REFINE_MAX_BLOCKS  rhccq_palette_refine: 0 (default) = 8 workgroups per CU, never more than there are chunks of 2048
 *                              pixels; 1..65535 = at most that many workgroups, so that one workgroup takes many chunks.  Same results. */
#define RHCCQ_OPT_REFINE_LDS_ROWS 10
#define RHCCQ_OPT_REFINE_MAX_BLOCKS 11
/*   RHCCQ_OPT_CHAIN_RELEASE    rhccq_encode_frame with RHCCQ_OPT_FRAME_CHAINS = 1 (no effect with 0): 1 (default) = every level-1 problem goes
 *                              on the moment ITS chain has ended inside the frame's chain launch (rhccq_mbk_init_released: the kernel
 *                              publishes a flag per problem; the problem's lane waits for it on the host and queues nothing before) -- a
 *                              class with shorter chains runs its steps, assignments and merges beside the longest chain instead of
 *                              behind it; 0 = every lane waits for the event behind the whole launch.  A chain kernel that publishes
 *                              nothing (RHCCQ_OPT_INIT_KERNEL other than the third generation) is waited for by that event either way.
 *                              Same results. */
#define RHCCQ_OPT_CHAIN_RELEASE 12
/*   RHCCQ_OPT_RUNS_ROWS        rhccq_palette_runs: the image rows one workgroup (one wave, a lane per row) walks: 0 (default) =
 *                              rhccq_palette_runs_rows(), or 2, 4 or 8.  Fewer rows put more workgroups on more CUs and leave more
 *                              lanes of each wave idle in the walk.  Same results. */
#define RHCCQ_OPT_RUNS_ROWS 13
/*   RHCCQ_OPT_DITHER_ROWS      rhccq_palette_dither: the image rows of a band (one wave; 64 / rows lanes share a pixel's palette search):
 *                              0 (default) = rhccq_palette_dither_rows(), or 4, 8, 16 or 32.  Fewer rows give every step of the wavefront
 *                              a shorter search and the picture more bands to hand errors through.  Same results. */
#define RHCCQ_OPT_DITHER_ROWS 14
/*   RHCCQ_OPT_KMEANS_WIDE_PAIRS  rhccq_kmeans: a problem of k <= 1024 centres and at least this many (point, centre) pairs, n x k, takes the
 *                              "wide" Lloyd path: load, mean / tolerance and k-means++ as ever in the problem's one workgroup, then every
 *                              Lloyd iteration as two launches on the context's stream, an E-step over tiles of 64 points on many CUs and
 *                              an M-step of one workgroup; launches, not waits between workgroups, are the synchronisation.  0 = never;
 *                              1 = every problem the path supports (0 .. 2^30).  Every other problem of the call runs the one-workgroup
 *                              kernel.  Same results: the same per-pair arithmetic, centres in ascending order, exact integer member sums.
 *   RHCCQ_OPT_KMEANS_CHUNK     rhccq_kmeans: how many Lloyd iterations of the wide path are enqueued between two looks of the host at the
 *                              problems' state records (1 .. 300); launches behind a problem's end return at once.  Same results. */
#define RHCCQ_OPT_KMEANS_WIDE_PAIRS 15
#define RHCCQ_OPT_KMEANS_CHUNK 16
/*   RHCCQ_OPT_GIF_READ_CHAIN   rhccq_gif_unlzw / rhccq_gif_decode: how a segment's len / first chains are resolved in LDS: 0 (default) =
 *                              pointer doubling by the whole workgroup (12 rounds), 1 = one lane walks the entries in order.  Same results;
 *                              kept for the measurement of tools/gifreadbench.py. */
#define RHCCQ_OPT_GIF_READ_CHAIN 17
int rhccq_ctx_set_int(rhccq_ctx* ctx, int32_t option, int64_t value);
int rhccq_sync(rhccq_ctx* ctx);                 /* hipStreamSynchronize on the context stream */
void* rhccq_stream(rhccq_ctx* ctx);             /* the hipStream_t in use */
/* Launch the following entry points on another HIP stream (not owned).  The Python side calls this whenever torch's
 * current stream differs from the bound one, so that the caller's allocations / memsets (torch, current stream) and the
 * kernels stay ordered on ONE stream -- e.g. inside `with torch.cuda.stream(s):`.  Work already queued on the previous
 * stream is not waited for: ordering across streams is the caller's business, as with torch itself. */
int rhccq_ctx_set_stream(rhccq_ctx* ctx, void* hip_stream);
int rhccq_abi_version(void);

/* ---- parameters: compute_clustering_params (encoder/compression/clustering.py:108-135) ----- */
int rhccq_params(int64_t n_colors, double quality, double* eps_host, int64_t* max_colors_host);
/* integer form of the eps predicate: thr, boundary (-1 if none), r2 = (eps/255)^2 */
int rhccq_eps_threshold(double eps, int32_t* thr_host, int32_t* boundary_host, double* r2_host);

/* ---- K0/K1: per-job unique colours ----------------------------------------------------------
 * A "job" is one set of pixels whose unique colours are wanted: a whole crop
 * (get_all_unique_colors, clustering.py:4-103) or one SLIC segment of a region
 * (subregion_quantization, subregions.py:315-426).  Each job owns a 2^24-bit bitmap.
 *
 * rhccq_job_scan: one pass over the pixels.  For class c (0..n_class-1) pixel p belongs to job
 *   job_base[c] + labels[c][p] - 1 when labels[c][p] > 0 (labels[c] == NULL: every pixel belongs
 *   to job job_base[c]).  Sets the colour bit of every non-black pixel, accumulates per-job
 *   stats {min_r, max_r, min_c, max_c, count, n_black} (int32[6] each, caller-initialised to
 *   {INT_MAX,-1,INT_MAX,-1,0,0}); black pixels set their bit only when black_is_colour != 0.
 *
 * Alignment.  rgb on 4 bytes for rhccq_job_scan, rhccq_job_scan_bytes, rhccq_job_stats, rhccq_job_blackfix, rhccq_job_index,
 *   rhccq_job_index_entries and rhccq_frame_remap (their kernels read 4 pixels as three dwords; RHCCQ_E_ARG otherwise);
 *   rhccq_job_sort_unique reads rgb byte by byte and takes any address.  Every label map labels[c] on 16 bytes (read as int4),
 *   for every entry point of this section.  The per-class planes of idx_out, entries / entries_out and rankmap are
 *   int32[n_class][H*W] with no padding: class c starts at c*H*W elements, so the buffers need 4-byte alignment only, whatever
 *   H*W is -- the kernels' 16-byte vector accesses to them rely on gfx950's unaligned global access (tests/job_cases.py holds
 *   the shapes with H*W mod 4 != 0). */
int rhccq_job_scan(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                   const int32_t* const* labels_host /* host array of device ptrs */,
                   const int32_t* job_base_host, int32_t black_is_colour, uint32_t* bitmaps,
                   int32_t* stats);
/* Same pass with BYTE colour flags (bytemaps: uint8[n_jobs][2^24], zero-initialised): plain idempotent
 * stores instead of scattered device-scope atomics (which run at the memory side on MI355X).
 * rhccq_bytemap_pack then ORs the flags into the 2 MiB bitmaps (32 bytes -> one word). */
int rhccq_job_scan_bytes(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                         const int32_t* const* labels_host, const int32_t* job_base_host,
                         int32_t black_is_colour, uint8_t* bytemaps, int32_t* stats);
int rhccq_bytemap_pack(rhccq_ctx* ctx, const uint8_t* bytemaps, int32_t n_jobs, uint32_t* bitmaps);
/* set bit 0 (black) of the bitmaps of the jobs listed (device int32 list) */
int rhccq_job_set_black(rhccq_ctx* ctx, uint32_t* bitmaps, const int32_t* jobs, int32_t n_jobs);
/* popcount of every job's bitmap -> counts[n_jobs] (device) and chunk sums workspace
 * chunk_sums[n_jobs*512] */
int rhccq_bitmap_count(rhccq_ctx* ctx, const uint32_t* bitmaps, int32_t n_jobs, uint32_t* chunk_sums,
                       int32_t* counts);
/* word_prefix[n_jobs*BITMAP_WORDS][2] = (bitmap word, exclusive prefix of the set bits before it) pairs -- the table the
 * per-pixel passes gather from, one 8-byte load per rank lookup -- and the sorted palette keys of each
 * job written at keys_out[pal_off[j] ...) (np.unique order, clustering.py:22) */
int rhccq_bitmap_emit(rhccq_ctx* ctx, const uint32_t* bitmaps, int32_t n_jobs, const uint32_t* chunk_sums,
                      const int64_t* pal_off /* device int64[n_jobs] */, uint32_t* word_prefix,
                      uint32_t* keys_out);
/* black-in-segment fix (subregions.py:393-421): per job the in-mask non-black pixel with the
 * smallest R^2+G^2+B^2, first in raster order; best[job] = (norm2<<40 | pixel index), init ~0 */
int rhccq_job_blackfix(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                       const int32_t* const* labels_host, const int32_t* job_base_host,
                       const uint8_t* job_needs_fix /* device u8[n_jobs] */, unsigned long long* best);
/* ---- frames with very many segments: unique colours by one device sort instead of 6 MiB of bitmap tables per job.
 * rhccq_job_stats: the statistics half of rhccq_job_scan alone (stats as there).
 * rhccq_job_sort_unique: every masked pixel of every class becomes the key (job << 24 | colour) -- in-mask black recoloured by fix_key[job] when
 *   that is non-zero, and one synthetic (job, colour 0) entry per job listed in black_jobs (crops that show background, all-black segments) --;
 *   one radix sort + head flags + an exclusive scan give, per job in job order, its sorted distinct colours (np.unique order) in
 *   keys_out[job_start[job] ...) (job_start[job] = -1: the job has no colour; *n_unique = their total) and, per (class, pixel), the rank of the
 *   pixel's colour inside its job's palette in rankmap (int32[n_class][H*W], -1 where the pixel has no job).  tmp: rhccq_job_sort_unique_bytes
 *   (n_class * H * W + n_black) bytes of device scratch; keys_out must hold that many entries.
 * rhccq_job_index_ranked / rhccq_frame_remap_ranked: rhccq_job_index (first positions only) / rhccq_frame_remap reading the stored ranks. */
int rhccq_job_stats(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class, const int32_t* const* labels_host,
                    const int32_t* job_base_host, int32_t* stats);
int64_t rhccq_job_sort_unique_bytes(int64_t n_entries);
int rhccq_job_sort_unique(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class, const int32_t* const* labels_host,
                          const int32_t* job_base_host, int32_t n_jobs, const uint32_t* fix_key /* device, may be NULL */,
                          const int32_t* black_jobs /* device int32[n_black] */, int32_t n_black, void* tmp, int64_t tmp_bytes, int32_t* rankmap,
                          uint32_t* keys_out, int32_t* job_start /* device int32[n_jobs] */, int32_t* n_unique /* device int32 */);
int rhccq_job_index_ranked(rhccq_ctx* ctx, int32_t H, int32_t W, int32_t n_class, const int32_t* const* labels_host, const int32_t* job_base_host,
                           const int32_t* rankmap, const int64_t* pal_off, int32_t* first_pos, const int32_t* fp_lut);
int rhccq_frame_remap_ranked(rhccq_ctx* ctx, int32_t H, int32_t W, int32_t n_class, const int32_t* const* labels_host, const int32_t* job_base_host,
                             const int32_t* rankmap, const int64_t* pal_off, const int32_t* lut, const int32_t* lut2, int32_t default_index, void* out,
                             int32_t out_elem_bytes);
/* per-pixel palette index (rank of the pixel's colour in its job's palette) and/or first raster
 * position of every palette entry.  fix_key[job] (device, may be NULL) = key that replaces in-mask
 * black pixels (0 = no fix).  idx_out (int32[n_class][H*W], may be NULL): -1 where the pixel has no
 * job.  first_pos (may be NULL) must be initialised to INT_MAX; entry = pal_off[job]+rank, or
 * fp_lut[pal_off[job]+rank] when fp_lut != NULL (first positions of a clustered, smaller palette). */
int rhccq_job_index(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                    const int32_t* const* labels_host, const int32_t* job_base_host,
                    const uint32_t* bitmaps, const uint32_t* word_prefix, const int64_t* pal_off,
                    const uint32_t* fix_key, int32_t* idx_out, int32_t* first_pos, const int32_t* fp_lut);
/* rhccq_job_index with first positions AND, per (class, pixel), the table entry the pixel shows (fp_lut[pal_off[job] + rank], or
 * pal_off[job] + rank without fp_lut; -1 where the pixel has no job) in entries_out (int32[n_class][H*W]): what the final remap needs,
 * so that it reads neither the pixels nor the rank tables again.  rhccq_frame_remap_entries: the index map from those entries --
 * for every pixel the first class (in the order given) whose label is > 0 decides: out = lut2[entry] (lut2 may be NULL: the entry
 * itself), default_index where no class covers the pixel (clustering.py:373-377 composed with merging.py:64-82). */
int rhccq_job_index_entries(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                            const int32_t* const* labels_host, const int32_t* job_base_host, const uint32_t* bitmaps,
                            const uint32_t* word_prefix, const int64_t* pal_off, const uint32_t* fix_key, int32_t* first_pos,
                            const int32_t* fp_lut, int32_t* entries_out);
int rhccq_frame_remap_entries(rhccq_ctx* ctx, int32_t H, int32_t W, int32_t n_class, const int32_t* const* labels_host,
                              const int32_t* job_base_host, const int32_t* entries, const int32_t* lut2, int32_t default_index,
                              void* out, int32_t out_elem_bytes);

/* ---- K3/K4: DBSCAN(min_samples=1) labels = eps-graph components (clustering.py:233-235) -------
 * problems p = 0..n_prob-1: keys[off[p] .. off[p]+n[p]); labels in sklearn order (rank of the
 * component's smallest member index).  desc: int32[n_prob][4] = {off, n, thr, boundary},
 * r2: double[n_prob].  labels_out int32 (same offsets), ncomp_out int32[n_prob]. */
int rhccq_eps_components(rhccq_ctx* ctx, const uint32_t* keys, const int32_t* desc, const double* r2,
                         int32_t n_prob, int32_t max_n, int32_t* labels_out, int32_t* ncomp_out);
/* DBSCAN with min_samples > 1 (clustering.py:233-271: noise points exist then).  rhccq_eps_counts: counts[i] = number of palette points
 * within eps of point i, itself included (a core point has >= min_samples); rhccq_eps_border: labels_out[i] = core_label[i] for a core
 * point (its component's label from rhccq_eps_components on the core subset, in sklearn's order), else the smallest label among its
 * core neighbours, -1 (noise) if it has none.  thr / boundary / r2 as in rhccq_eps_components (rhccq_eps_threshold). */
int rhccq_eps_counts(rhccq_ctx* ctx, const uint32_t* keys, int32_t n, int32_t thr, int32_t boundary, double r2, int32_t* counts);
int rhccq_eps_border(rhccq_ctx* ctx, const uint32_t* keys, int32_t n, int32_t thr, int32_t boundary, double r2, const int32_t* core_label,
                     int32_t* labels_out);

/* ---- K2: per-cluster floor-mean colour (clustering.py:304-310,346-355) ----------------------
 * sums[k*4] (uint64 r,g,b,count) zero-initialised by the caller (one call per buffer: up to 2^24 points the sums are gathered
 * as two packed words per label and spread over the four fields at the end); labels in [0, k) or < 0 (skipped). */
int rhccq_cluster_sums(rhccq_ctx* ctx, const uint32_t* keys, const int32_t* labels, int64_t n, int64_t k,
                       unsigned long long* sums);
int rhccq_cluster_means(rhccq_ctx* ctx, const unsigned long long* sums, int64_t k, uint32_t* keys_out);

/* ---- K7: KMeans split of oversize clusters (clustering.py:720-775 -> sklearn KMeans) ---------
 * desc: int32[n_prob][6] = {off, n, k, rand_off, first_index, T}; rand: the MT19937 uniforms
 * (k-1)*T per problem at rand_off (numpy RandomState(42).uniform stream, generated on the host);
 * work: double workspace, 8*k doubles per problem at 8*koff (koff = desc-order prefix of k, given
 * as koff int64[n_prob]); labels_out int32 at the same offsets as keys; info int32[n_prob][4] =
 * {n_iter, strict, relocations, path}, path = 1 for a problem that took the wide Lloyd path (RHCCQ_OPT_KMEANS_WIDE_PAIRS; it needs
 * context scratch for its state records, and the call then reads `desc` and the records back), 0 for the one-workgroup kernel. */
int rhccq_kmeans(rhccq_ctx* ctx, const uint32_t* keys, const int32_t* desc, const int64_t* koff,
                 const double* rand, int32_t n_prob, int32_t max_n, double* work, int32_t* labels_out,
                 int32_t* info);
/* ---- K8: MiniBatchKMeans branch (clustering.py:207-230 -> sklearn MiniBatchKMeans(n_clusters, batch_size=1000,
 * random_state=42, n_init='auto').fit_predict) -------------------------------------------------------------------
 * The fit is sklearn's, operation for operation: the RandomState(42) stream is replayed from its raw MT19937 words
 * (`words`, resident on the device), k-means++ runs over the init sample in draw order, batches are
 * randint(0, n, 1000), centre updates add the batch members in batch order, reassigned centres take the rows
 * choice(1000, replace=False) names.  Where sklearn keeps np.argsort(counts)[:500] -- an unstable sort over tied counts --
 * the slots numpy's scalar quicksort fills are taken (RHCCQ_OPT_REASSIGN_ORDER, csrc/k8_npysort.h): the fit equals
 * scikit-learn's untouched fit_predict under numpy's scalar sort kernels.  oracle.minibatch_kmeans_labels states the same. */
typedef struct rhccq_mbk_problem {
  int64_t off;        /* first key of the problem in keys[] */
  int64_t n;          /* number of points */
  int64_t k;          /* n_clusters */
  int64_t koff;       /* offset (in clusters) into centres / weights / work arrays */
  int64_t init_off;   /* offset into init_idx / perm */
  int64_t init_n;     /* init sample size */
  int64_t rand_off;   /* offset into rand (k-1)*T uniforms */
  int32_t first;      /* first centre (position in the init sample, draw order) */
  int32_t T;          /* n_local_trials */
} rhccq_mbk_problem;
/* Internal pruning index of rhccq_mbk_init: perm (device, int32, same offsets as init_idx) receives, per problem, the
 * positions 0 .. init_n-1 of its init sample ordered by (Morton code of the sampled colour, position).  init_idx
 * (device; problem i's sample rows in RandomState draw order at [init_off, init_off + init_n), the problems back to
 * back) is only read.  Replaces nothing in the reference: 64 Morton-consecutive samples form a compact colour box,
 * which is what lets the k-means++ kernel skip blocks exactly.  tmp: rhccq_mbk_order_bytes(sum init_n) bytes. */
int64_t rhccq_mbk_order_bytes(int64_t total_samples);
int rhccq_mbk_order(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                    int32_t n_prob, const int32_t* init_idx, int32_t* perm, void* tmp, int64_t tmp_bytes);
/* out[idx[i]] = min(out[idx[i]], val[i]), i < count: the first raster position of a palette entry that several entries of the level
 * below map to (merging.py:77-79 carried through clustering.py:373-377).  Host code; RHCCQ_E_ARG for an index outside [0, n_out). */
int rhccq_scatter_min_host(int64_t n_out, const int32_t* idx, const int64_t* val, int64_t count, int64_t* out);
/* The bookkeeping behind one clustered palette whose clusters need no split (clustering.py:296-377), host code: from the member
 * sums of the k clusters (rhccq_cluster_sums layout) the floor-mean colour of every non-empty cluster in label order behind
 * `nblack` black rows (new_keys: room for nblack + k) and lut[label] = new palette index (uint16-valued like the reference's
 * mapping_array; empty clusters map to the first row).  Returns the number of non-empty clusters, -1 when a cluster holds more
 * than mc colours (it takes the KMeans split instead), -2 for a bad argument. */
int64_t rhccq_cluster_plan_host(const unsigned long long* sums, int64_t k, int64_t mc, int32_t nblack, uint32_t* new_keys, int32_t* lut);
/* merge_region_components_simple in palette space (encoder/compression/merging.py:8-120), host code: the components are painted
 * in REVERSED order, every component's entries in the order of their first raster positions fp; a colour gets the index of its
 * first appearance in that sequence (index 0 = canvas black) and the smallest first position of its members.  Entries with key
 * 0 or fp >= fp_none do not appear (lut 0).  gkeys / gfp: room for 1 + sum(counts); lut[c]: counts[c] ints.  Pure host code. */
int rhccq_merge_palettes_host(int32_t n_comp, const uint32_t* const* keys, const int64_t* const* fp, const int32_t* counts,
                              int64_t fp_none, uint32_t* gkeys, int64_t* gfp, int32_t* const* lut, int64_t* n_out);
/* ---- numpy's legacy RandomState(42), replayed from its raw MT19937 words (csrc/mt_replay.h: the one replay of the process) ----
 * RandomState.randint(0, n, size) ON THE HOST from raw words in host memory (masked rejection, one word per attempt): sklearn
 * MiniBatchKMeans draws its validation and init samples this way before k-means++ (clustering.py:207-218 -> _kmeans.py
 * MiniBatchKMeans.fit).  out: int32[size] or NULL (stream position only).
 * Returns the words consumed, -1 when the table ends first, -2 for a bad argument.  Pure host code, no ctx. */
int64_t rhccq_mt_randint_host(const uint32_t* words, int64_t n_words, int64_t pos, int64_t n, int64_t size, int32_t* out);
/* out[i] = raw word pos + i of MT19937(seed 42), i < count (host memory; what the tests compare with numpy's generator).  Host only. */
int rhccq_mt_words_host(int64_t pos, int64_t count, uint32_t* out);
/* random_sample() with the stream at raw word `pos` (two words; -1.0 for pos < 0), and RandomState.choice(n, p = ones / n) from its one
 * uniform u (-1 for n outside 1 .. 2^31 - 1): the first centre of k-means++.  Host only, safe from several threads. */
double rhccq_mt_double_host(int64_t pos);
int32_t rhccq_first_centre_index(int64_t n, double u);
/* What MiniBatchKMeans(k, batch_size=1000, random_state=42).fit of n points fixes ahead of its k-means++ chain. */
typedef struct rhccq_mbk_draw {
  int64_t batch;      /* min(1000, n) */
  int64_t limit;      /* steps at most: 100 n / batch */
  int64_t init_size;  /* 3 batch, 3 k if that is below k, n at most */
  int64_t n_uniforms; /* uniforms of the chain: max((k - 1) T, 1) */
  int64_t pos;        /* raw word of the first k-means++ uniform: behind the validation draw, the init sample and the first centre */
  int64_t cursor0;    /* stream position behind the k-means++ uniforms: pos + 2 (k - 1) T */
  int32_t T;          /* n_local_trials: 2 + floor(ln k) */
  int32_t first;      /* first centre (position in the init sample) */
} rhccq_mbk_draw;
/* Fills *out and init_idx (int32[cap], cap >= init_size: the init sample in draw order, 0 .. n-1 when init_size == n).  init_idx NULL:
 * only what follows from (n, k) alone (pos, cursor0, first stay 0), so that a caller can size the buffer.  RHCCQ_E_ARG, and nothing
 * written, unless 1 <= k <= n < 2^31 and cap suffices.  Host only, safe from several threads. */
int rhccq_mbk_draws(int64_t n, int64_t k, rhccq_mbk_draw* out, int32_t* init_idx, int64_t cap);
/* At least the first n raw words on the context's device, complete on return: *words_dev, *count >= n.  One table per device and
 * process, shared by every context; a pointer handed out stays readable for the life of the process. */
int rhccq_mt_words(rhccq_ctx* ctx, int64_t n, const uint32_t** words_dev, int64_t* count);
/* out[i] = the i-th double numpy's legacy RandomState.uniform(size=count) / random_sample() yields when its
 * MT19937 stream stands at raw word `pos`: ((w[pos+2i] >> 5) * 2^26 + (w[pos+2i+1] >> 6)) / 2^53.  words: the raw
 * 32-bit outputs of MT19937(seed 42), resident on the device (rhccq_mt_words).
 * Serves the uniform(size=n_local_trials) draws of k-means++ (sklearn `_kmeans_plusplus`). */
int rhccq_mt_uniforms(rhccq_ctx* ctx, const uint32_t* words, int64_t pos, int64_t count, double* out);
/* greedy k-means++ (sklearn _kmeans_plusplus) on the init sample in exact integers, candidates searched over the
 * cumulative closest-distance sums in DRAW order; writes centres[(koff+j)*4 + {0,1,2}] (doubles, raw 0..255
 * coordinates; [3] = squared norm) and chosen[koff+j] (position in the init sample, draw order) */
int rhccq_mbk_init(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                   int32_t n_prob, const int32_t* init_idx, const int32_t* perm, const double* rand,
                   double* centres, int32_t* chosen);
/* The same launch, publishing every problem the moment ITS chain has ended (the launch goes on for the longer chains of the other
 * problems): flags_dev[16 p] (a 64-byte line per problem, device address of mapped host memory: rhccq_release_flags_alloc) receives
 * `tag` (non-zero; use a new one per launch, then a flag never has to be cleared and a stale value never matches) once problem p's slice
 * of `centres` is complete and released at system scope -- a later launch on ANOTHER stream may then read and rewrite that slice while
 * this launch still runs, provided the slices of two problems share no 128-byte line of `centres` (koff a multiple of 4) or of `chosen`,
 * which the launch writes too (koff a multiple of 32: what rhccq_encode_frame lays out).  *published_host
 * = 1 when the kernel chosen publishes (the third-generation chain), 0 when it does not (any other generation or option setting: the
 * flags stay untouched and only the end of the launch says that the centres are there).  Otherwise as rhccq_mbk_init. */
int rhccq_mbk_init_released(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                            int32_t n_prob, const int32_t* init_idx, const int32_t* perm, const double* rand,
                            double* centres, int32_t* chosen, uint32_t* flags_dev, uint32_t tag, int32_t* published_host);
/* n_prob release flags, zeroed, in page-locked host memory mapped to the current device: *flags_host for the host's reads (volatile /
 * atomic loads of flags_host[16 p]), *flags_dev for rhccq_mbk_init_released.  rhccq_release_flags_free(flags_host) once no launch uses them. */
int rhccq_release_flags_alloc(int32_t n_prob, uint32_t** flags_host, uint32_t** flags_dev);
void rhccq_release_flags_free(uint32_t* flags_host);
/* np.argsort(w)[:cap] AS A SET under numpy's scalar sort kernel (numpy/_core/src/npysort/quicksort.cpp aquicksort_<double>,
 * heapsort.cpp behind its depth limit) -- the selection inside a capped reassignment of rhccq_mbk_steps, exposed for tests.
 * w: double[k] on the device, non-negative integers < 2^32; 0 < cap < k; depth0 < 0 = numpy's depth limit 2 floor(log2 k)
 * (tests lower it to drive the heapsort branch); use_lds != 0: the part that still matters moves to LDS once it has shrunk to 7 680
 * elements (what rhccq_mbk_steps does), 0: global memory throughout; scratch: 16 k bytes; mask_out: uint32[(k + 31) / 32], bit j set
 * <=> j is among the first cap entries. */
int rhccq_npysort_head(rhccq_ctx* ctx, const double* w, int32_t k, int32_t cap, int32_t depth0, int32_t use_lds, void* scratch, uint32_t* mask_out);
/* run mini-batch steps step0 .. step0 + n_steps - 1 for every problem that has not stopped (call with step0 = 0 first -- that
 * call writes the problem tables at the head of `work`, later calls only queue kernels -- then with the number of steps launched so far; all problems of a call sequence share the step index).  state:
 * double[n_prob][16] = {[0] ewa, [1] ewa_min, [2] no_improvement, [3] samples since the last reassignment, [4] why the
 * problem stopped (0 running, 1 converged, 2 out of steps, 3 word table exhausted -- fatal: size `words` so that it
 * cannot happen; 4 sharded chain hand-off lost; 5 overlapped schedule diverged), [5] steps done, [6] have_ewa, [7] have_min, [8] zero-weight centres (initialise to k), [9] MT cursor
 * = raw words consumed so far (initialise to the position behind the k-means++ uniforms), [10] first batch drawn, [11]
 * stop_at (steps done when it stopped, 0 while running), [12..14] the odd-step twins of [3], [8], [9] (a step reads the
 * slots of its parity and writes the other's; after s steps the current values sit in the slots of parity s & 1)};
 * initialise everything but [8] and [9] to 0.  weights double[sum k]; words / n_words: raw MT19937(42) words on the
 * device -- a step consumes at most 16 384 of them. */
int rhccq_mbk_steps(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                    int32_t n_prob, int64_t step0, int32_t n_steps, const uint32_t* words, int64_t n_words,
                    double* centres, double* weights, double* state, void* work, int64_t work_bytes,
                    int32_t estep_mode, int32_t estep_split);
/* estep_mode: how the batch E-step finds each point's nearest centre -- identical results either way:
 * RHCCQ_ESTEP_TILES brute force over LDS tiles of centres (few problems in flight), RHCCQ_ESTEP_GRID centres
 * re-binned into a 32^3 grid every step and searched ring by ring (many problems in flight: a batch of frames),
 * RHCCQ_ESTEP_AUTO grid when the problems handed over hold >= 200 000 centres.
 * estep_split (tiled E-step only; 0 or 1, 2, 4, 8): threads sharing one batch point, each walking 1/split of a
 * tile's centres -- shortens the per-thread chain when only a straggler problem is still running; same results. */
#define RHCCQ_ESTEP_AUTO 0
#define RHCCQ_ESTEP_TILES 1
#define RHCCQ_ESTEP_GRID 2
/* ORed into estep_mode: the caller has read the state and knows that no running problem reassigns during this call (state[8] /
 * [13] == 0 and fewer than 10 k samples since the last reassignment throughout): the second launch of a reassigning step
 * (the centres move, the next batch is drawn behind the shuffle) is left out; a problem that wants to reassign all the same
 * stops with state[4] = 5 */
#define RHCCQ_STEPS_NO_REASSIGN 0x100
int64_t rhccq_mbk_work_bytes(const rhccq_mbk_problem* probs_host, int32_t n_prob);
/* The same steps for ONE problem (n_prob == 1) that has no zero-weight centre left (state[8] / [13] == 0), with the batch
 * E-step of step t + 1 started BESIDE the update of step t: a step that does not reassign changes only the <= 1000 centres its
 * batch touched, so the next batch is first compared with every untouched centre (same launch as the update) and then with
 * the touched ones at their new values -- the same distances and the same first arg-min, off the chain of dependent
 * launches (a 4K frame ends in one problem that runs all its ~2000 steps: sklearn MiniBatchKMeans.fit,
 * clustering.py:207-218).  since0: "samples since the last reassignment" as step0 sees it (state[3] for an even step0,
 * state[12] for an odd one): the host derives from it which steps reassign (those run the classic E-step); a device state
 * that disagrees stops the problem with state[4] = 5.  *carry: in/out, 0 before the first call and after any rhccq_mbk_steps
 * call; bit 0 = the batch of step0 + 1 is drawn, bit 1 = the speculative tile minima of step0 are in `work`.  A step may
 * draw one batch ahead: size `words` for n_steps + 3 steps.  State, work and results as rhccq_mbk_steps (bit-identical). */
int rhccq_mbk_steps_overlapped(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                               int32_t n_prob, int64_t step0, int32_t n_steps, const uint32_t* words, int64_t n_words,
                               double* centres, double* weights, double* state, void* work, int64_t work_bytes,
                               int32_t estep_split, int64_t since0, int32_t* carry);
/* The same for a batch of 1 .. 32 problems that share the step index, each on the schedule its state asks for: bit p of
 * fast_mask = problem p takes the overlapped schedule above (no zero-weight centre left, k >= 1024), bit p of classic_mask =
 * it takes the classic sequence of rhccq_mbk_steps (tiled E-step; classic_no_reassign != 0 = RHCCQ_STEPS_NO_REASSIGN for
 * them), neither = every launch leaves it out (its workgroups return at once).  since0[n_prob] / carry[n_prob]: as above, per
 * problem (read and written for the problems of fast_mask only).  Problems whose launch parameters agree at a step share its
 * launches; they differ only around their reassigning steps, so nearly every step is two launches for the whole batch.
 * Bit-identical to running every problem alone. */
int rhccq_mbk_steps_batch(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                          int32_t n_prob, int64_t step0, int32_t n_steps, const uint32_t* words, int64_t n_words,
                          double* centres, double* weights, double* state, void* work, int64_t work_bytes,
                          int32_t estep_split, uint32_t fast_mask, uint32_t classic_mask, int32_t classic_no_reassign,
                          const int64_t* since0, int32_t* carry);
/* final E-step over all points: labels_out int32 at the key offsets (first arg-min of
 * csq_j + (-2 * dot), brute force order-independent; uses a centre grid for pruning) */
int rhccq_mbk_assign(rhccq_ctx* ctx, const uint32_t* keys, const rhccq_mbk_problem* probs_host,
                     int32_t n_prob, const double* centres, void* work, int64_t work_bytes,
                     int32_t* labels_out);

/* ---- the fused frame encoder as ONE native entry ----------------------------------------------------------
 * rhccq.ipynb:978-1039 for one frame whose ROI / non-ROI segment label maps are given: per segment crop + black fix + unique colours
 * (subregions.py:315-449), cluster(q) per segment and merge per region (:634-679), per class merge on the frame canvas + cluster(2q)
 * (regions.py:9-70), merge of the classes + cluster(q3) + index dtype (image.py:243-286, compression.py:360-372) -- the ordering rules
 * of clustering.py:249-377 and merging.py:52-82 as native host code (csrc/encode_frame.hip), the kernels above underneath.  The region
 * classes run as host threads with HIP streams of their own, the MiniBatchKMeans problems of a class side by side on further streams;
 * nothing of the interpreter is on the path.  Result identical to roibasedimagecompression_amd.frame.FrameEncoder.encode (tests).
 *   classes[c]: labels = DEVICE int32[H*W] (0 = pixel not in the class, s >= 1 = segment id, ids global within the class and ascending
 *     inside each region); seg_region = HOST int32[n_seg] (region of segment id s at [s - 1]); region_bbox = HOST int32[n_region][4]
 *     (minr, minc, maxr, maxc); quality = the class's level-1 quality.  Classes in precedence order (ROI first).
 *   palette_out: HOST uint8[pal_cap][3]; indices_out: DEVICE buffer of H * W * 4 bytes, written as uint8 / uint16 / uint32 [H][W]
 *     (res->index_bytes) on the context's stream, complete when the call returns; n_unique_out (HOST int64[n_jobs], may be NULL):
 *     unique colours per segment.  At most 2048 segments per frame (beyond: the sort-based path of the Python FrameEncoder).
 * Returns 0, RHCCQ_E_ARG, RHCCQ_E_HIP or RHCCQ_E_LIMIT (too many segments, or pal_cap too small: res->n_colours says how many).
 * One call at a time per context (the context keeps the lanes' streams and device arenas between frames; use one context per host
 * thread that encodes); the call returns with every lane idle. */
typedef struct rhccq_class_desc {
  const int32_t* labels;
  int32_t n_seg;
  int32_t n_region;
  const int32_t* seg_region;
  const int32_t* region_bbox;
  int32_t quality;
  int32_t reserved;
} rhccq_class_desc;
typedef struct rhccq_frame_result {
  int32_t n_colours;       /* palette entries */
  int32_t index_bytes;     /* 1, 2 or 4 */
  int32_t shape[2];        /* (H, W), or the single component's box when only one component reaches level 3 (merging.py:16-21) */
  int32_t top_left[2];
  int32_t quality3;
  int32_t n_jobs;
  double ms[8];            /* host clocks: [0] scan [1] unique [2] levels 1-2 (slowest class) [3] level 3 [4] compose [5] remap [6] total */
  double class_ms[4][4];   /* per class (first four): level-1 clustering, first positions + merges, level-2 clustering, level-2 finish */
} rhccq_frame_result;
int rhccq_encode_frame(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const rhccq_class_desc* classes, int32_t n_classes,
                       uint8_t* palette_out, int32_t pal_cap, void* indices_out, int64_t* n_unique_out, rhccq_frame_result* res);
/* The MiniBatchKMeans fits of the level-2 stage of the context's last rhccq_encode_frame (RHCCQ_OPT_FRAME_LEVEL2 = 1; none with 0):
 * out[6 i ..] = {class, points, k, steps run, schedule: 0 = a lone problem's own fit, 1 = in a batch, classic steps only, 2 = in a
 * batch and on the overlapped schedule, the step at which it went there (-1: never)} for the first `cap` of them; returns how many
 * there are (-1: bad argument). */
int32_t rhccq_encode_frame_level2_info(const rhccq_ctx* ctx, int32_t cap, int64_t* out);

/* ---- K6: index remap gather (clustering.py:373-377) ------------------------------------------ */
int rhccq_remap(rhccq_ctx* ctx, const int32_t* idx, int64_t n, const int32_t* lut, int64_t lut_n,
                int32_t* out);
/* fused final remap of a frame: class precedence = class order; value = lut[pal_off[job]+rank], then
 * lut2[value] when lut2 != NULL (lut = level-1 mapping, lut2 = the composed levels 2-3 over the clustered
 * palettes); values < 0 are transparent; out_elem_bytes in {1,2,4} */
int rhccq_frame_remap(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t n_class,
                      const int32_t* const* labels_host, const int32_t* job_base_host,
                      const uint32_t* bitmaps, const uint32_t* word_prefix, const int64_t* pal_off,
                      const uint32_t* fix_key, const int32_t* lut, const int32_t* lut2, int32_t default_index,
                      void* out, int32_t out_elem_bytes);

/* ---- K5: merge_region_components_simple (encoder/compression/merging.py:8-120) ---------------
 * one component at a time (the host assigns first-seen global indices between the two calls):
 * first_pos[idx] = min raster position (component raster) of in-canvas pixels showing palette
 * entry idx (entries >= pal_n are skipped, merging.py:72); paint writes lut[idx] where >= 0. */
int rhccq_merge_firstpos(rhccq_ctx* ctx, const int32_t* idx, int32_t h, int32_t w, int32_t top, int32_t left,
                         int32_t canvas_h, int32_t canvas_w, int32_t pal_n, int32_t* first_pos);
int rhccq_merge_paint(rhccq_ctx* ctx, const int32_t* idx, int32_t h, int32_t w, int32_t top, int32_t left,
                      int32_t canvas_h, int32_t canvas_w, const int32_t* lut, int32_t pal_n, int32_t* canvas);

/* ---- decode: palette[index] LUT gather (decoder/uncompression/uncompression.py:209) ---------- */
int rhccq_decode(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int64_t n, const uint8_t* palette,
                 int64_t pal_n, uint8_t* rgb_out);

/* ---- quality metrics (decoder/uncompression/comparison.py:30-80 calculate_quality_metrics) ------
 * a, b: uint8 RGB interleaved device images (4-byte aligned), n_pixels = H*W.
 * sums5 (device): [0..2] sum of squared differences per channel, [3] sum of |differences|, [4] max |difference|
 * -> MSE / RMSE / MAE / max error / per-channel MSE / PSNR (comparison.py:40,63-78) on the host. */
int rhccq_error_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t n_pixels, uint64_t* sums5);
/* calculate_adaptive_quality_metrics (comparison.py:345-536): tab768 (device, uint64[256][3]) row e = {pixels, sum of squared
 * differences over the 3 channels, sum of |differences|} of the pixels whose largest channel error is e; maxerr (device,
 * uint8[n_pixels], may be NULL) = that largest channel error per pixel (the outlier mask for the masked SSIM).  Percentiles,
 * outlier thresholds, the metrics of every pixel subset the reference forms and its error histogram follow on the host. */
int rhccq_error_tables(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t n_pixels, uint64_t* tab768, uint8_t* maxerr);
/* structural_similarity(a, b, data_range=255, channel_axis=2, win_size=7) (comparison.py:47-49; algorithm of
 * scikit-image, unpinned by the reference): partial (device) receives, per workgroup tile, the sum over its
 * window centres of S for each channel; mean SSIM = sum(partial) / ((H-6)*(W-6)) averaged over the channels.
 * rhccq_ssim7_blocks gives the number of tiles (host only). */
int64_t rhccq_ssim7_blocks(int32_t H, int32_t W);
int rhccq_ssim7_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, int32_t H, int32_t W, double* partial,
                     int64_t n_blocks);

/* ---- per-class quality metrics (EXTENSION: no reference counterpart; csrc/region_metrics.hip) -----------------------------
 * The sums above kept apart by a class map: cls (device, uint8 per pixel, any alignment) names the row a pixel goes to; a
 * value >= n_classes (255, say) leaves the pixel out of every row.  n_classes: 1..16, else RHCCQ_E_ARG.
 * sums (device, uint64[n_classes][6]): row c = {sum of squared differences R, G, B, sum of |differences|, max |difference|,
 * pixels} over the pixels of class c; a and b as for the whole-picture entry above.  The _indexed form compares a with
 * palette[idx] without writing that image out: idx (1, 2 or 4 bytes per element, unsigned) and palette as for the decode
 * entry (an index past the palette reads entry 0). */
int rhccq_class_error_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* cls, int64_t n_pixels,
                           int32_t n_classes, uint64_t* sums);
int rhccq_class_error_sums_indexed(rhccq_ctx* ctx, const uint8_t* a, const void* idx, int32_t idx_elem_bytes,
                                   const uint8_t* palette, int64_t pal_n, const uint8_t* cls, int64_t n_pixels,
                                   int32_t n_classes, uint64_t* sums);
/* SSIM per class: a window belongs to the class of its centre pixel.  partial (device, double[n_blocks][n_classes][4]) receives
 * per workgroup tile and class the sum of S for R, G, B and the number of window centres; the host adds the tiles in order.
 * The window statistics are the exact integer sums of the whole-picture entry. */
int64_t rhccq_class_ssim7_blocks(int32_t H, int32_t W);
int rhccq_class_ssim7_sums(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, const uint8_t* cls, int32_t H, int32_t W,
                           int32_t n_classes, double* partial, int64_t n_blocks);

/* ---- split score of a region (encoder/subregions/split_score.py:15-142 calculate_split_score) ------------
 * One pass over the region image (uint8 RGB interleaved, device) and its mask (uint8, 0 / non-0, may be NULL: then
 * gray > 0.01 as the reference does): gray + CIE-Lab per pixel (scikit-image's rgb2gray / rgb2lab, float64), Sobel magnitude
 * of the four planes ('reflect' borders), uniform LBP(8,1) code of the gray plane (zeros outside the image).
 * partial (device, double[n_blocks][12]) receives per workgroup tile the masked sums {count, L, L^2, a, a^2, b, b^2,
 * sum over Lab planes of sqrt(2 sobel^2), sobel(gray), sobel(gray)^2, gray, gray^2}; hist42 (device, int32[42]) the LBP
 * histogram (10 bins) followed by the intensity histogram (32 bins over [0, 1]).  The host turns them into the three
 * scores (roibasedimagecompression_amd/api/split_score.py).  PARITY UNPINNED: scikit-image is absent from the build
 * container; the algorithms are restated from their published definitions. */
int64_t rhccq_split_stats_blocks(int32_t H, int32_t W);
int rhccq_split_stats(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* mask, double* partial,
                      int64_t n_blocks, int32_t* hist42);

/* ---- masked SLIC (encoder/subregions/slic.py:41-104 -> skimage.segmentation.slic(mask=...); SURVEY 8f-2, parity unpinned)
 * rhccq_slic_assign: one assignment sweep of _slic_cython on a 2-D image: img (device, double[H][W][3], the Gaussian-smoothed
 * Lab image times 1 / compactness), mask (device u8), seg (device, double[K][5] = y, x, c0, c1, c2), step = the seed spacing;
 * labels (device int32[H][W]) = 1 + index of the nearest centroid whose window [c - 2 step, c + 2 step] holds the pixel
 * (first on ties), 0 outside the mask / in no window.  ignore_color != 0: spatial term only (the seed-relaxation sweeps).
 * rhccq_slic_connectivity_host: _enforce_label_connectivity_cython, a serial raster scan with breadth-first floods, as a
 * native HOST routine (both pointers are host memory; no context, no GPU). */
int rhccq_slic_assign(rhccq_ctx* ctx, const double* img, const uint8_t* mask, const double* seg, int32_t H, int32_t W, int32_t K,
                      double step, int32_t ignore_color, int32_t* labels);
int rhccq_slic_connectivity_host(const int32_t* labels_host, int32_t H, int32_t W, int32_t min_size, int32_t max_size,
                                 int32_t* out_host);

/* resize of enhanced_slic_with_texture (slic.py:42-44,82,101 -> skimage.transform.resize): scipy.ndimage.gaussian_filter1d along one axis of
 * a device float64 array viewed as [outer][len][inner] (mode 'mirror'; weights: device double[radius + 1] = centre, then offsets
 * 1..radius; scipy's summation order), scipy.ndimage.zoom order 1 / 0 with the per-axis index and weight tables computed on the host
 * (yi, wy: [2][oh]; xi, wx: [2][ow] for order 1; [oh], [ow] for order 0); zoom_linear clips to [lo, hi] as resize does. */
int rhccq_gauss1d_f64(rhccq_ctx* ctx, const double* in, int64_t outer, int32_t len, int64_t inner, const double* weights, int32_t radius, double* out);
int rhccq_zoom_linear_f64(rhccq_ctx* ctx, const double* in, int32_t H, int32_t W, int32_t C, const int32_t* yi, const double* wy, const int32_t* xi,
                          const double* wx, int32_t oh, int32_t ow, double lo, double hi, double* out);
int rhccq_zoom_nearest(rhccq_ctx* ctx, const void* in, int32_t elem_bytes, int32_t H, int32_t W, int32_t C, const int32_t* yi, const int32_t* xi,
                       int32_t oh, int32_t ow, void* out);

/* ---- ROI stage, region extraction (encoder/ROI/roi.py)
 * Connected components of a binary mask with statistics: what the reference takes from
 * cv2.connectedComponentsWithStats (roi.py:285-294 extract_connected_regions_fast, :229 fuse_adjacent_regions_optimized, and every
 * clean-up step of the encoder/ROI modules).  PARITY UNPINNED for the label NUMBERING: OpenCV is absent from the build container; its
 * published block-based algorithms (Grana's BBDT / Bolelli's Spaghetti, 8-connectivity) number components by their first
 * 2x2 block in block-raster order, the pixel-based 4-connectivity one by their first pixel; the partition itself is unambiguous.
 * rhccq_ccl: mask (device u8[H][W], nonzero = foreground), connectivity 4 or 8; numbering 0 = OpenCV's (above), 1 = by first
 *   pixel in raster order (scipy.ndimage.label / skimage.measure.label, roi.py:262 extract_connected_regions), 2 = unordered ids
 *   1..count and NO statistics (stats may be NULL; cap unused): enough to tell components apart, e.g. for Canny's hysteresis;
 *   work: rhccq_ccl_work_bytes(H, W, cap) bytes of device scratch; labels (device int32[H][W]): 0 = background, 1..count;
 *   stats (device int32[cap + 1][5]): row l = {CC_STAT_LEFT, TOP, WIDTH, HEIGHT, AREA} of label l, row 0 = the background;
 *   count (device int32): number of components.  When count > cap the labels are all 0 and the statistics meaningless:
 *   call again with cap >= count.  No host synchronisation inside.
 * rhccq_ccl_select: out[p] = lut[labels[p]] (u8 look-up per label: keep / drop whole components).
 * rhccq_roi_buffer = extract_roi_nonroi (roi.py:685-718): region_map (device u8, 1 = ROI core, 0 = non-ROI core), both cores
 * dilated buffer_size times with scipy's default cross (= L1 ball, border value 0), buffer zone = both dilations; outputs the
 * two masks (u8 0/1) and the two masked copies of rgb.  This one is pinned: the reference calls scipy.ndimage.binary_dilation. */
int64_t rhccq_ccl_work_bytes(int32_t H, int32_t W, int32_t cap);
int rhccq_ccl(rhccq_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t connectivity, int32_t numbering, void* work, int64_t work_bytes,
              int32_t cap, int32_t* labels, int32_t* stats, int32_t* count);
int rhccq_ccl_select(rhccq_ctx* ctx, const int32_t* labels, const uint8_t* lut, int64_t n_pixels, uint8_t* out);
/* tile-parallel labelling (one tile per GPU, seams stitched through one all-gather: roibasedimagecompression_amd/parallel.py tiled_ccl):
 * keys[l] (device u32[n_labels + 1], 0xffffffff where a label has no pixel) = the ordering key of component l of a TILE whose top-left
 * pixel sits at (y0, x0) of a frame frame_w pixels wide, in FRAME coordinates -- the key rhccq_ccl numbers by (numbering 0 with
 * connectivity 8: first 2x2 block in block-raster order, even y0 / x0 required; otherwise first pixel in raster order).  A component
 * that several tiles share takes the minimum of its parts' keys. */
int rhccq_ccl_keys(rhccq_ctx* ctx, const int32_t* labels, int32_t H, int32_t W, int32_t y0, int32_t x0, int32_t frame_w, int32_t numbering,
                   int32_t connectivity, int32_t n_labels, uint32_t* keys);
int rhccq_roi_buffer(rhccq_ctx* ctx, const uint8_t* region_map, const uint8_t* rgb, int32_t H, int32_t W, int32_t buffer_size,
                     uint8_t* roi_mask, uint8_t* nonroi_mask, uint8_t* roi_image, uint8_t* nonroi_image);

/* ---- ROI stage, edge front end (encoder/ROI/edges.py:35-71,173-195: get_edge_map = 20 adaptive threshold pairs scored on a
 * Canny edge map each + the final Canny; compute_local_density).  PARITY UNPINNED (OpenCV absent from the build container):
 * integer restatements of cvtColor(RGB2GRAY), Sobel 3x3, Canny (L1 gradient, aperture 3) -- csrc/edges.hip.
 * rhccq_edges_gray: gray (device u8[n]) + its 256-bin histogram (device int32[256]: Otsu's threshold on the host).
 * rhccq_edges_grad_hist: histogram (device int32[rhccq_edges_m2_bins()]) of gx^2 + gy^2, Sobel 3x3 with BORDER_REFLECT_101.
 * rhccq_canny_nms: img (device u8[H][W][channels], 1 or 3) -> nm (device u16[H][W]): Canny's L1 gradient magnitude where the
 *   pixel is a local maximum along its gradient direction, 0 elsewhere (threshold independent); mag_tmp u16[H*W], dxy_tmp int32[H*W].
 * rhccq_edges_above: mask[p] = nm[p] > low.
 * rhccq_label_reduce: red (device u64[n_labels + 1][4]) = per label {max of val16, sum of val8, sum of val8^2, pixel count} (either plane may
 *   be NULL: zeros).
 *   With rhccq_ccl on the mask this is Canny's hysteresis: a component is an edge iff its max exceeds `high`.
 * rhccq_box_count: out (device u16[H][W]) = number of non-zero pixels in the kernel_size x kernel_size window (odd, <= 31),
 *   BORDER_REFLECT_101: the integer content of compute_local_density's normalised box filter. */
int64_t rhccq_edges_m2_bins(void);
int rhccq_edges_gray(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, uint8_t* gray, int32_t* hist256);
int rhccq_edges_grad_hist(rhccq_ctx* ctx, const uint8_t* gray, int32_t H, int32_t W, int32_t* hist_m2);
int rhccq_canny_nms(rhccq_ctx* ctx, const uint8_t* img, int32_t H, int32_t W, int32_t channels, uint16_t* mag_tmp, int32_t* dxy_tmp,
                    uint16_t* nm);
int rhccq_edges_above(rhccq_ctx* ctx, const uint16_t* nm, int64_t n_pixels, int32_t low, uint8_t* mask);
int rhccq_label_reduce(rhccq_ctx* ctx, const int32_t* labels, const uint16_t* val16, const uint8_t* val8, int64_t n_pixels,
                       int32_t n_labels, uint64_t* red);
/* Canny's hysteresis verdict and the quality score's sums on the device: red = rhccq_label_reduce's (device u64[n + 1][4]);
 * out4 (device u64[4]) = {components whose max exceeds high, their pixels, their sum of val8, their sum of val8^2}; lut (device u8[n + 1], may
 * be NULL) = 255 for those components (for rhccq_ccl_select) */
int rhccq_edge_score(rhccq_ctx* ctx, const uint64_t* red, int32_t n_labels, int32_t high, uint64_t* out4, uint8_t* lut);
/* The scores of SEVERAL threshold pairs with nothing crossing to the host in between (find_best_edges_by_quality tries 20 pairs,
 * encoder/ROI/edges.py:40-71): per distinct `low` one mask + one labelling of {nm > low} (component count kept on the device) + one per-label
 * reduction capped at `cap` labels; per pair one verdict.  lows / highs: HOST int32[n_pairs], pairs with equal `low` adjacent.  out: DEVICE
 * uint64[n_pairs][5] = {edge components, edge pixels, sum gray, sum gray^2, components of {nm > low}}; a pair whose last number exceeds `cap`
 * must be scored through rhccq_label_reduce / rhccq_edge_score instead.  work: rhccq_canny_scores_bytes(H, W, cap) bytes. */
/* rhccq_canny_scores_nested: the same scores from ONE union-find grown over the thresholds in descending `low` (the sets {nm > low} nest):
 * every pixel is linked once over the whole search, a pair's verdict marks the roots of the pixels above `high` with a generation number and
 * sums the pixels under marked roots -- no component numbering, no per-label tables, no capacity.  Pairs in any order; out[i][4] = 0.
 * work: rhccq_canny_scores_nested_bytes(H, W) bytes. */
int64_t rhccq_canny_scores_nested_bytes(int32_t H, int32_t W);
int rhccq_canny_scores_nested(rhccq_ctx* ctx, const uint16_t* nm, const uint8_t* gray, int32_t H, int32_t W, const int32_t* lows_host,
                              const int32_t* highs_host, int32_t n_pairs, void* work, int64_t work_bytes, uint64_t* out);
int64_t rhccq_canny_scores_bytes(int32_t H, int32_t W, int32_t cap);
int rhccq_canny_scores(rhccq_ctx* ctx, const uint16_t* nm, const uint8_t* gray, int32_t H, int32_t W, const int32_t* lows_host,
                       const int32_t* highs_host, int32_t n_pairs, int32_t cap, void* work, int64_t work_bytes, uint64_t* out);
int rhccq_box_count(rhccq_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, int32_t kernel_size, uint16_t* out);
/* the same window, summing the pixel VALUES (maps that are not 0 / one value: the notebook's 0 / 1 / 255 planes) */
int rhccq_box_sum(rhccq_ctx* ctx, const uint8_t* plane, int32_t H, int32_t W, int32_t kernel_size, uint32_t* out);

/* ---- ROI stage, clean-up chain (encoder/ROI/{roi,small_regions,small_gaps,thin_regions2}.py): binary-mask operators.  PARITY
 * UNPINNED (OpenCV absent from the build container); masks are device u8 planes, set = non-zero, outputs 0 / 255.
 * rhccq_morph_dilate: dilation by a structuring element given as one half-width per row dy = -radius .. radius (-1 = empty row;
 *   radius <= 15), nothing set outside the image (cv2.dilate's default border); invert_in / invert_out = the erosion by the same
 *   symmetric element with cv2.erode's border rule (outside = set).  cv2.morphologyEx(MORPH_CLOSE) = dilate, then erode.
 * rhccq_mask_op: out = a | b (op 0), a & b (1), a & ~b (2), ~a (3).
 * rhccq_gap_bridge = bridge_small_gaps_fast (small_gaps.py:221-271): an unset pixel whose window count (rhccq_box_count; or window
 *   sum, rhccq_box_sum) is at least min_count is set when both opposite rays of one of the four direction pairs meet a set pixel within `reach` steps.
 * rhccq_dist_chamfer = cv2.distanceTransform(mask, DIST_L2, 3) in OpenCV's fixed point (16 fractional bits; hz_tmp: u16[H*W]).
 * rhccq_binary_sobel: m2 (device u8[H*W]) = gx^2 + gy^2 of the 3x3 Sobel of the 0/1 image (BORDER_REFLECT_101), max_out = its
 *   maximum (device int32); rhccq_lut_u8: out[p] = lut256[in[p]].
 * rhccq_label_sum: sums (device u64[n_labels + 1]) = per label (background 0 included) the sum of a u16 (value_bytes 2) or a
 *   non-negative int32 (value_bytes 4) plane. */
int rhccq_morph_dilate(rhccq_ctx* ctx, const uint8_t* in, int32_t H, int32_t W, int32_t radius, const int32_t* half_widths /* host */,
                       int32_t invert_in, int32_t invert_out, uint8_t* out);
/* the general form: rows dy = -up .. down, row i spans dx = -left[i] .. right[i] (both -1: empty row).  An even k x k OpenCV element
 * (protect_border_regions' default is 18, roi.py:824) has its anchor at k / 2: up = left = k / 2, down = right = k - 1 - k / 2. */
int rhccq_morph_dilate_spans(rhccq_ctx* ctx, const uint8_t* in, int32_t H, int32_t W, int32_t up, int32_t down, const int32_t* left /* host */,
                             const int32_t* right /* host */, int32_t invert_in, int32_t invert_out, uint8_t* out);
/* compute_local_density (edges.py:173-195) on ANY u8 plane for odd kernels up to 11 x 11 = OpenCV's direct filter2D path: float32 accumulator
 * over the taps in row-major order, BORDER_REFLECT_101; scale255 != 0: plane / 255.0 first.  (Binary planes go through rhccq_box_count and a table.) */
int rhccq_box_filter_seq(rhccq_ctx* ctx, const uint8_t* plane, int32_t H, int32_t W, int32_t kernel_size, int32_t scale255, float* out);
int rhccq_mask_op(rhccq_ctx* ctx, const uint8_t* a, const uint8_t* b, int64_t n, int32_t op, uint8_t* out);
int rhccq_gap_bridge(rhccq_ctx* ctx, const uint8_t* in, const void* counts /* u16 (count_bytes 2) or u32 (4) */, int32_t count_bytes, int32_t H,
                     int32_t W, int64_t min_count, int32_t reach, uint8_t* out);
int rhccq_dist_chamfer(rhccq_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, uint16_t* hz_tmp, int32_t* dist);
int rhccq_binary_sobel(rhccq_ctx* ctx, const uint8_t* mask, int32_t H, int32_t W, uint8_t* m2, int32_t* max_out);
int rhccq_lut_u8(rhccq_ctx* ctx, const uint8_t* in, const uint8_t* lut256, int64_t n, uint8_t* out);
/* out[p] = table[values[p]]: float32 table (device, n_table entries) indexed by a u16 plane (window counts -> densities) */
int rhccq_lut_u16_f32(rhccq_ctx* ctx, const uint16_t* values, const float* table, int32_t n_table, int64_t n, float* out);
int rhccq_label_sum(rhccq_ctx* ctx, const int32_t* labels, const void* values, int32_t value_bytes, int64_t n_pixels, int32_t n_labels,
                    uint64_t* sums);
/* hist (device u64[n_bins], n_bins <= 4096): histogram of the u16 plane over the pixels where mask is set (larger values ignored);
 * rhccq_value_mask: out = 255 where values[p] >= min_value and (mask is NULL or set), else 0 */
int rhccq_masked_hist(rhccq_ctx* ctx, const uint8_t* mask, const uint16_t* values, int64_t n_pixels, int32_t n_bins, uint64_t* hist);
int rhccq_value_mask(rhccq_ctx* ctx, const uint8_t* mask, const uint16_t* values, int64_t n_pixels, int32_t min_value, uint8_t* out);

/* ---- EXTENSION (no reference counterpart; named by BASELINE.json's north_star only): pixel-space DBSCAN ----
 * Features (x, y, L, a, b); q is a neighbour of p when dx^2 + dy^2 <= radius^2 (radius 0..4) and
 * dL^2 + da^2 + db^2 + spatial_weight^2 (dx^2 + dy^2) <= eps^2 (float32, operation order fixed in
 * csrc/px_dbscan_ext.hip and oracle.px_dbscan).  lin_lut: device float[256 + 2048]: 8-bit sRGB -> linear, then
 * 1024 pairs (f(i / 1024), f((i + 1) / 1024) - f(i / 1024)) of the Lab transfer function, interpolated linearly;
 * see Rhccq.px_tables().
 * rhccq_px_neighbours (the "fixed-radius neighbour pass": 3 B read + 4 B written per pixel): parent_out[p] = p for
 * a core pixel (>= min_pts neighbours, itself included), -1 otherwise; count_out (may be NULL) = neighbour count.
 * rhccq_px_expand (the "region growing"): lock-free union-find over the core pixels, then
 * labels_out[p] = 1 + smallest pixel index of p's cluster; non-core pixels take the smallest cluster among their
 * core neighbours, 0 = noise.  `parent` is the array rhccq_px_neighbours produced (modified in place). */
int rhccq_px_neighbours(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t radius, float eps,
                        float spatial_weight, int32_t min_pts, const float* lin_lut, int32_t* parent_out,
                        uint8_t* count_out);
int rhccq_px_expand(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, int32_t radius, float eps,
                    float spatial_weight, const float* lin_lut, int32_t* parent, int32_t* labels_out);

/* ---- EXTENSION (no reference counterpart): block DCT-II + region quantisation --
 * plane: float32[H*W]; block in {8,16}; qstep: float32 per tile [(H/block)*(W/block)];
 * coef_out float32[H*W] (may be NULL), q_out int16[H*W]. */
int rhccq_dct_quant(rhccq_ctx* ctx, const float* plane, int32_t H, int32_t W, int32_t block,
                    const float* qstep, float* coef_out, int16_t* q_out);
/* RGB u8 -> luma float32 (BT.601) plus per-tile qstep from a ROI mask (u8, may be NULL) */
int rhccq_luma_qstep(rhccq_ctx* ctx, const uint8_t* rgb, const uint8_t* roi_mask, int32_t H, int32_t W,
                     int32_t block, float q_roi, float q_bg, float* luma_out, float* qstep_out);

/* ---- EXTENSION: zlib stream (RFC 1950 / 1951) on the device, for the .rhccq container layers --------------------
 * Format-compatible with zlib's inflate (zlib.decompress reads it), not byte-identical to zlib.compress(level=9)
 * (rhccq_zlib9_compress below is);
 * the output bytes are a function of the input bytes alone (not of the stream, earlier calls or the workspace's
 * contents).  Each DEFLATE block takes the cheapest of dynamic, fixed and stored, so *out_len <= out_bound. */
/* host only: workspace and worst-case output size for n input bytes */
int rhccq_zlib_sizes(int64_t n, int64_t* workspace_bytes, int64_t* out_bound);
/* zlib stream (RFC 1950/1951) of in[0..n) into out; async on the context stream; *out_len (device int64) receives the length */
int rhccq_zlib_compress(rhccq_ctx* ctx, const void* in, int64_t n, void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len);

/* ---- EXTENSION: zlib stream (RFC 1950 / 1951) decoder on the device, the read side of the container layers ----------
 * Accepts what zlib.decompress accepts (bytes after the Adler-32 trailer ignored; FDICT and CINFO > 7 rejected).  A distance
 * is checked against the start of the output and the 32 KiB limit only, not against a smaller window the header declares.
 * Output positions are int32: n and out_cap must be below 2^31 (RHCCQ_E_LIMIT otherwise).  The workspace is not sized by the
 * call: the caller passes one of at least rhccq_zlib_inflate_sizes bytes. */
#define RHCCQ_ZS_OK 0
#define RHCCQ_ZS_BAD_HEADER 1   /* zlib header is invalid (check, method, window, preset dictionary) */
#define RHCCQ_ZS_BAD_DATA 2     /* invalid block type, code lengths, symbol or distance */
#define RHCCQ_ZS_TRUNCATED 3    /* stream ends early */
#define RHCCQ_ZS_ADLER 4        /* Adler-32 does not match */
#define RHCCQ_ZS_CAPACITY 5     /* output is larger than out_cap; *out_len holds the length needed */
/* host only: workspace bytes for decoding n compressed bytes into at most out_cap bytes */
int rhccq_zlib_inflate_sizes(int64_t n, int64_t out_cap, int64_t* workspace_bytes);
/* async on the context stream; *out_len (device int64): decoded length, or the length needed when *status is
   RHCCQ_ZS_CAPACITY; *status (device int32): RHCCQ_ZS_* */
int rhccq_zlib_decompress(rhccq_ctx* ctx, const uint8_t* in, int64_t n, void* workspace,
                          uint8_t* out, int64_t out_cap, int64_t* out_len, int32_t* status);
/* async: after rhccq_zlib_decompress with the same n, out_cap and workspace, stats (device int64[4]) receives the number of
   candidate block starts, candidates whose speculative decode failed, chained workers, and blocks on the chain */
int rhccq_zlib_inflate_stats(rhccq_ctx* ctx, int64_t n, int64_t out_cap, const void* workspace, int64_t* stats);
/* the same decoder functions run serially on the host (tests; no GPU needed) */
int rhccq_zlib_decompress_host(const uint8_t* in, int64_t n, uint8_t* out, int64_t out_cap,
                               int64_t* out_len, int32_t* status);

/* ---- EXTENSION: zlib level 9, byte for byte, on the device (csrc/zlib_deflate9.hip) ---------------------------------
 * The output is exactly zlib 1.2.11's compress(data, 9) (windowBits 15, memLevel 8, default strategy), a function of the
 * input bytes alone.  n must be below 2^31 (RHCCQ_E_LIMIT); null pointers, n < 0 and out_cap below the bound: RHCCQ_E_ARG. */
/* host only: workspace and output bound (>= zlib's compressBound(n)) for n input bytes */
int rhccq_zlib9_sizes(int64_t n, int64_t* workspace_bytes, int64_t* out_bound);
/* async on the context stream; *out_len (device int64) receives the length */
int rhccq_zlib9_compress(rhccq_ctx* ctx, const void* in, int64_t n, void* workspace,
                         uint8_t* out, int64_t out_cap, int64_t* out_len);
/* the same functions run serially on the host (tests; no GPU needed) */
int rhccq_zlib9_compress_host(const void* in, int64_t n, uint8_t* out, int64_t out_cap, int64_t* out_len);
/* async: after rhccq_zlib9_compress with the same n and workspace, stats (device int64[6]) receives candidates examined,
   parse nodes, pointer-jumping rounds (max over segments), and stored / fixed / dynamic blocks */
int rhccq_zlib9_stats(rhccq_ctx* ctx, int64_t n, const void* workspace, int64_t* stats);

/* ---- EXTENSION: image -> .rhccq in one device-resident flow (api/image.py ImageEncoder) -------------------------------------
 * Regions are boxes of a frame W wide whose mask is (labels0 or labels1)[y][x] == label.  All calls are async on the context stream;
 * every table is device memory, block tables (block_item / block_region int32[n_blocks], block_first int32[items]) cover each item
 * with consecutive workgroups of 256 pixels (split_stats_regions: one workgroup per 32 x 8 tile of the region's box). */
/* rhccq_split_stats for every region at once: regions int32[n][6] = (y0, x0, h, w, map, label); partial double[n_blocks][12] (row b:
   tile b - block_first[r] of region r, as rhccq_split_stats numbers the tiles of the crop); hist int32[n][42] (zeroed here) */
int rhccq_split_stats_regions(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const int32_t* labels0, const int32_t* labels1,
                              const int32_t* regions, int32_t n_regions, const int32_t* block_region, const int32_t* block_first,
                              int64_t n_blocks, double* partial, int32_t* hist);
/* host only: workspace bytes of rhccq_slic_sweeps_regions */
int64_t rhccq_slic_regions_work_bytes(int32_t n_regions, int32_t max_iter);
/* the two _slic_cython loops of max_iter sweeps (colour ignored, then used) of every region's small image: img double[][3], mask
   uint8[], labels int32[] (out) at px_off (a multiple of 256) of regions int32[n][5] = (px_off, H, W, K, seg_off); seg double[][5]
   (in: the seeded centroids; out: the final ones); steps double[n]; seg_region int32[n_seg]: region of every centroid; max_k: the
   largest K.  Centroid means are np.bincount's raster-order float64 sums; a region whose sweep labels nothing stops, as _sweeps does. */
int rhccq_slic_sweeps_regions(rhccq_ctx* ctx, const double* img, const uint8_t* mask, double* seg, const int32_t* regions, const double* steps,
                              int32_t n_regions, int32_t max_k, const int32_t* block_region, const int32_t* block_first, int64_t n_blocks,
                              const int32_t* seg_region, int32_t n_seg, int32_t max_iter, void* work, int64_t work_bytes, int32_t* labels);
/* regions int32[n][11] = (y0, x0, h, w, map, label, small_off, small_w, yx_off, sid_off, layer); a region's SLIC id at (y, x) of its
   box is small[small_off + yx[yx_off + y] * small_w + yx[yx_off + h + x]] (the nearest-neighbour upscale).
   seg_counts: counts int32[n_sid] (zeroed here) += the in-mask pixels of every (region, id) at sid_off + id */
int rhccq_image_seg_counts(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                           const int32_t* small, const int32_t* yx, const int32_t* block_item, const int32_t* block_first, int64_t n_blocks,
                           int32_t* counts, int64_t n_sid);
/* hit int32[n_pairs] (zeroed here): 1 when, for pairs[i] = (r, q), a pixel of both masks holds a segment of q with ids[q's sid] > 0;
   the block tables cover the intersection of the two boxes */
int rhccq_image_overlap(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                        const int32_t* small, const int32_t* yx, const int32_t* ids, const int32_t* pairs, int32_t n_pairs,
                        const int32_t* block_item, const int32_t* block_first, int64_t n_blocks, int32_t* hit);
/* layers int32[][H][W] (zeroed by the caller): layers[layer][y0 + y][x0 + x] = ids[sid_off + id] for the in-mask pixels with id > 0 and
   ids[...] > 0; regions with layer < 0 are skipped */
int rhccq_image_paint(rhccq_ctx* ctx, const int32_t* labels0, const int32_t* labels1, int32_t H, int32_t W, const int32_t* regions,
                      const int32_t* small, const int32_t* yx, const int32_t* ids, const int32_t* block_item, const int32_t* block_first,
                      int64_t n_blocks, int32_t* layers);

/* ---- EXTENSION: nearest-colour remap onto a given palette (no reference counterpart; csrc/palette_remap.hip) ----------------------
 * idx_out[p] = argmin over j of the squared distance (dr^2 + dg^2 + db^2, uint8 channels, exact integers) between rgb[p] and
 * palette[j]; ties go to the lowest j; duplicate rows and a black row are ordinary entries.  rgb (n_pixels x 3) and palette (K x 3)
 * are interleaved uint8 of any alignment; idx_out has idx_elem_bytes (1, 2 or 4) per element, unsigned, aligned to its element.
 * sums (uint64[n_classes + 1][2], zeroed by the call): row c = {pixels, sum of the minimal distances} over the pixels with
 * cls[p] == c; a class value >= n_classes leaves the pixel out of every class row (the rule of the per-class error sums above);
 * the last row counts every pixel.  cls == NULL: n_classes must be 0 and only that last row is written.
 * RHCCQ_E_ARG: a null rgb, palette, idx_out or sums; K < 1; n_pixels < 0; n_classes outside 0..16 (or not 0 with cls == NULL);
 * idx_elem_bytes not 1, 2 or 4; K > 256 with 1-byte indices; a misaligned idx_out or sums.  RHCCQ_E_LIMIT: K > 65536 (the bound of
 * the reference's uint16 mapping array).  n_pixels == 0 succeeds with zero sums.
 * Device form: every pointer is device memory; async on the context stream; a grid-stride launch sized to the device; nothing is
 * allocated.  Host form: the same pack / evaluate / carry functions run serially on host memory (tests; no GPU needed). */
int rhccq_palette_remap(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K,
                        const uint8_t* cls, int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_remap_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls,
                             int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
/* host only: the palette entries the kernel stages at a time; the winner is carried from one such tile to the next */
int32_t rhccq_palette_remap_tile(void);

/* ---- EXTENSION: refinement of a given palette, exact integer Lloyd iterations (no reference counterpart; csrc/palette_refine.hip) ----
 * A pixel's weight is weights[cls[p]] when cls[p] < n_classes and weights[n_classes] otherwise (and for every pixel when cls == NULL);
 * weights are 0..255 with at least one > 0, NULL = all ones.  Iteration i: (1) a(p) = rhccq_palette_remap's index of p (nearest row in
 * exact integers, ties to the lowest row: a later duplicate never receives a pixel); (2) per row j, over the pixels with a(p) = j, in
 * 64-bit integers N_j = sum w(p), S_j = sum w(p) p per channel, and E = sum w(p) |p - palette[a(p)]|^2 over all pixels; (3) a row with
 * N_j > 0 becomes floor((2 S_j + N_j) / (2 N_j)) per channel (the weighted mean rounded to nearest, halves up), a row with N_j == 0 stays;
 * history[i] = {E, rows whose three bytes changed}.  The refinement stops after the first iteration that changes no row or after
 * max_iter; *n_iter = iterations that ran; history rows from n_iter on are zero.  E never increases from one iteration to the next.
 * palette (K x 3, IN/OUT), rgb and cls are uint8 of any alignment; history is uint64[max_iter][2], n_iter one int32, both zeroed by the call.
 * RHCCQ_E_ARG: a null rgb, palette, history, n_iter or work; K < 1; n_pixels < 0; n_classes outside 0..16 (or not 0 with cls == NULL);
 * max_iter outside 1..64; a weight outside 0..255 or all weights 0; a misaligned history (8), n_iter (4) or work (8); work_bytes below
 * rhccq_palette_refine_bytes(K).  RHCCQ_E_LIMIT: K > 65536.  n_pixels == 0 succeeds with *n_iter = 0, a zero history, the palette untouched.
 * Device form: every pointer but weights_host is device memory; async on the context stream (two launches per iteration, later
 * iterations return at once after convergence), no host synchronisation, nothing allocated.  history is control state as well as
 * output while the call's launches are in flight: iteration i runs iff history[i - 1][1] != 0, so no other work on the stream or on
 * another stream may write history (or palette, n_iter, work) before those launches have finished; a foreign write there would change
 * how many iterations run.  Host form: the same functions run serially. */
int32_t rhccq_palette_refine_lds_rows(void);            /* host only: the largest K whose accumulators live in LDS */
int64_t rhccq_palette_refine_bytes(int32_t K);          /* host only: workspace bytes */
int rhccq_palette_refine(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, uint8_t* palette, int32_t K, const uint8_t* cls,
                         int32_t n_classes, const int32_t* weights_host, int32_t max_iter, void* work, int64_t work_bytes,
                         uint64_t* history, int32_t* n_iter);
int rhccq_palette_refine_host(const uint8_t* rgb, int64_t n_pixels, uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                              const int32_t* weights, int32_t max_iter, uint64_t* history, int32_t* n_iter);

/* ---- EXTENSION: reduction of a given palette to K_target rows, exact pairwise merging (no reference counterpart; csrc/palette_reduce.hip) ----
 * Pairwise-nearest-neighbour reduction with Ward's criterion.  palette is uint8[K][3], counts uint64[K] the weight of every row (the
 * histogram of an index map, say), 1 <= K_target <= K.  A live cluster has a weight n, per-channel sums S in 64-bit integers and an integer
 * centre c; row j starts with n_j = counts[j], S_j = n_j * palette[j], c_j = palette[j]; a cluster's id is the lowest original row in it.
 * (1) Rows with counts[j] == 0 are dropped first: they never merge and map to -1.  (2) The cost of the pair a < b is the exact rational
 * n_a n_b D(c_a, c_b) / (n_a + n_b), D the squared distance of the integer centres (rhccq_palette_remap's arithmetic).  (3) While more
 * than K_target clusters live, the pair of least cost merges; costs are compared exactly (cross-multiplied in 128 bits), ties go to the
 * smallest a, then the smallest b (duplicate rows have D = 0 and merge first): n_a += n_b, S_a += S_b, c_a = floor((2 S_a + n_a) / (2 n_a))
 * per channel (rhccq_palette_refine's rounding: nearest, halves up), b dies.  (4) The live clusters come out in ascending id order:
 * *k_out = min(K_target, non-empty rows); palette_out uint8[K_target][3] and counts_out uint64[K_target], zero from row k_out on;
 * map int32[K]: old row -> new row, -1 for an empty row; merges int32[K - 1][2] (may be NULL): the (a, b) of every step in order, -1 past
 * the last step.  The centre is an integer because it is the row a decoder will use; with the sum of the counts at most 2^32 - 1,
 * n_a n_b < 2^62, D < 2^18 and n_a + n_b < 2^32, so every cross product is below 2^112.
 * RHCCQ_E_ARG: a null palette, counts, palette_out, counts_out, map, k_out (or work); K < 1; K_target outside 1..K; every count zero; a
 * misaligned counts, counts_out, work (8), map, merges or k_out (4); work_bytes below rhccq_palette_reduce_bytes(K).  RHCCQ_E_LIMIT:
 * K > 65536; the sum of the counts above 2^32 - 1; in the device form K > rhccq_palette_reduce_max_rows().
 * Device form: every pointer is device memory; async on the context stream (three launches: row state, the table of nearest partners,
 * then ONE resident workgroup that runs the merge chain with its per-row state in LDS), no host synchronisation, nothing allocated.  The
 * two errors that only the counts show (all zero; sum above 2^32 - 1) cannot be returned without reading them: the call returns 0 and the
 * kernel writes RHCCQ_E_ARG / RHCCQ_E_LIMIT to *k_out, zero palette_out and counts_out, and -1 throughout map and merges.
 * Host form: the same key / compare / scan / merge functions run serially on host memory, for any K <= 65536. */
int32_t rhccq_palette_reduce_max_rows(void);            /* host only: the largest K of the device form (the rows one workgroup's LDS holds) */
int64_t rhccq_palette_reduce_bytes(int32_t K);          /* host only: workspace bytes */
int rhccq_palette_reduce(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, int32_t K_target, void* work,
                         int64_t work_bytes, uint8_t* palette_out, uint64_t* counts_out, int32_t* map, int32_t* merges /* may be NULL */,
                         int32_t* k_out);
int rhccq_palette_reduce_host(const uint8_t* palette, const uint64_t* counts, int32_t K, int32_t K_target, uint8_t* palette_out,
                              uint64_t* counts_out, int32_t* map, int32_t* merges, int32_t* k_out);

/* ---- EXTENSION: the palette ladder: moments, the error curve of every rung, any rung from the log (no reference counterpart;
 * csrc/palette_ladder.hip) ----
 * rhccq_palette_moments: one pass over the pixels.  a(p) is rhccq_palette_remap's index of p (exact integers, ties to the lowest row);
 * idx_out (may be NULL; otherwise idx_elem_bytes 1, 2 or 4 per element as the remap takes it) receives it.  moments is
 * uint64[n_classes + 1][K][5] = {N, Sr, Sg, Sb, Q}: table c sums the pixels with cls[p] == c, the last table every pixel (the remap's
 * rule for cls == NULL and for values >= n_classes: those pixels are in the last table only); per row j = a(p), N counts the pixels,
 * S adds the channel values and Q adds r^2 + g^2 + b^2.  The moments are unweighted.  The call zeroes the array; n_pixels == 0 leaves it
 * zero.  Integer addition only: every order gives the same sums.
 * RHCCQ_E_ARG: a null rgb, palette or moments; K < 1; n_pixels < 0; n_classes outside 0..16 (or not 0 with cls == NULL); with idx_out:
 * idx_elem_bytes not 1, 2 or 4, a misaligned idx_out, K > 256 with 1-byte indices; a misaligned moments (8).  RHCCQ_E_LIMIT: K > 65536.
 * Device form: async on the context stream, nothing allocated: a memset, the remap's chunk loop with the accumulators in LDS while
 * K <= rhccq_palette_moments_lds_rows(n_classes) and in global memory above, and a finish launch that forms the last table.
 *
 * rhccq_palette_curve: the squared error of every rung of rhccq_palette_reduce's ladder, without a remap.  palette, counts (the weights
 * the chain was run with) and merges (int32[K - 1][2] as rhccq_palette_reduce writes it, -1 behind the last step) define the replay:
 * row state n_j = counts[j], S_j = n_j * palette[j], c_j = palette[j]; step s merges (a, b) as the reduction does (n and S add, c_a =
 * floor((2 S + n) / (2 n)) per channel) and b's moments go into a's.  moments is uint64[n_tables][K][5] as rhccq_palette_moments writes
 * it (n_tables = n_classes + 1, 1..17); curve is uint64[n_tables][K]: curve[t][0] = sum over rows of (Q - 2 c.S + N |c|^2) over table t,
 * curve[t][s] the same sum over the clusters after s steps; entries behind the last step are 0.  A row of count 0 never merges and
 * keeps contributing its own term.  The replay ends at the first entry that is not a merge of two live rows a < b < K.  curve[t][s] is
 * the error of table t's pixels shown through the clusters their rows went into, so it bounds from above the error of the nearest-row
 * remap onto the rung of (non-empty rows - s) rows.  Every term is below 2^51 (sum of the counts at most 2^32 - 1, unweighted N no larger).
 * RHCCQ_E_ARG: a null argument; K < 1; n_tables outside 1..17; misaligned counts, moments, curve, work (8) or merges (4); work_bytes
 * below rhccq_palette_curve_bytes(K, n_tables).  RHCCQ_E_LIMIT: K > 65536; in the device form K > rhccq_palette_reduce_max_rows().
 * Device form: a copy of the moments, one launch for the row state and curve[t][0], then ONE wave that replays the log.
 *
 * rhccq_palette_rung: the rung of K_target rows from the log, without the chain: identical in every byte to what
 * rhccq_palette_reduce(K_target) writes to palette_out, counts_out, map and k_out for the same palette and counts (clusters in
 * ascending id order, empty rows -1, zero rows from k_out on).  Every row is resolved through the first (non-empty rows - K_target)
 * steps, n and n * palette are added per cluster, and the centre is floor((2 S + n) / (2 n)).  A log that ends before K_target is
 * reached gives the clusters it has: *k_out is their number, map holds their rows, and only the first K_target are written.
 * The log is expected to name every b once, as rhccq_palette_reduce writes it (a row dies once); an entry that is not a < b < K ends it.
 * A log that repeats a b stays in bounds, but the device form does not define which of its links wins (the host form keeps the last).
 * Errors as rhccq_palette_reduce's (no workspace; merges must be given); the two that only the counts show come back through *k_out
 * in the device form.  Host forms: the same functions run serially on host memory, for any K <= 65536. */
int32_t rhccq_palette_moments_lds_rows(int32_t n_classes);   /* host only: the largest K whose accumulators live in LDS (0: bad n_classes) */
int rhccq_palette_moments(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls,
                          int32_t n_classes, void* idx_out /* may be NULL */, int32_t idx_elem_bytes, uint64_t* moments);
int rhccq_palette_moments_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* palette, int32_t K, const uint8_t* cls,
                               int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* moments);
int64_t rhccq_palette_curve_bytes(int32_t K, int32_t n_tables);   /* host only: workspace bytes */
int rhccq_palette_curve(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges,
                        const uint64_t* moments, int32_t n_tables, void* work, int64_t work_bytes, uint64_t* curve);
int rhccq_palette_curve_host(const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, const uint64_t* moments,
                             int32_t n_tables, uint64_t* curve);
int rhccq_palette_rung(rhccq_ctx* ctx, const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, int32_t K_target,
                       uint8_t* palette_out, uint64_t* counts_out, int32_t* map, int32_t* k_out);
int rhccq_palette_rung_host(const uint8_t* palette, const uint64_t* counts, int32_t K, const int32_t* merges, int32_t K_target,
                            uint8_t* palette_out, uint64_t* counts_out, int32_t* map, int32_t* k_out);

/* ---- EXTENSION: run-carrying remap onto a given palette (no reference counterpart; csrc/palette_runs.hip) ----------------------------
 * rgb uint8[H][W][3], palette uint8[K][3], cls uint8[H][W] or NULL, slack uint32[n_classes + 1], each entry 0..195075 (3 * 255^2).  A pixel's
 * slack is slack[cls[p]] when cls[p] < n_classes and slack[n_classes] otherwise (and for every pixel when cls == NULL): the rule of
 * rhccq_palette_refine's weights.  (1) b(y, x) is rhccq_palette_remap's index of the pixel (nearest row in exact integers, ties to the lowest
 * row) and db(y, x) its squared distance.  (2) Every image row is independent: out(y, 0) = b(y, 0); for x >= 1, with c = out(y, x - 1),
 * out(y, x) = c if |rgb(y, x) - palette[c]|^2 <= db(y, x) + slack(y, x), else b(y, x).  A carry never crosses from one image row to the
 * next, and at an exact tie the carried row wins (so slack 0 keeps the remap's squared error but not always its indices).  (3) idx_out
 * (idx_elem_bytes 1, 2 or 4 per element, as the remap takes it) receives out; sums is uint64[n_classes + 1][3], zeroed by the call: row c =
 * {pixels, sum of |rgb - palette[out]|^2, carried} over the pixels with cls[p] == c, the last row over every pixel (the rows of the remap's
 * sums); carried counts the pixels with out != b.  Per row, SSE(out) <= SSE(b) + the slack summed over its carried pixels.
 * RHCCQ_E_ARG: as rhccq_palette_remap, and a null slack, H < 0, W < 0, a slack above 195075.  RHCCQ_E_LIMIT: K > 65536.  H * W == 0
 * succeeds with zero sums.
 * Device form: every pointer but slack_host (copied by value into the launch) is device memory; async on the context stream, no host
 * synchronisation, nothing allocated: rhccq_palette_remap into idx_out, a memset, then one launch that walks the rows in place (every
 * position reads b before it writes out), one wave per RHCCQ_OPT_RUNS_ROWS image rows, the picture staged through LDS in tiles of
 * rows x rhccq_palette_runs_tile_cols() pixels.  palette[b] is gathered from a copy of the palette in LDS while K <= 4096 and from global
 * memory above.  Host form: the same step functions (csrc/palette_runs.h) run serially on host memory. */
int32_t rhccq_palette_runs_tile_cols(void);             /* host only: the columns of a staging tile */
int32_t rhccq_palette_runs_rows(void);                  /* host only: the image rows of a workgroup by default */
int rhccq_palette_runs(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                       int32_t n_classes, const uint32_t* slack_host, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_runs_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                            const uint32_t* slack, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);

/* ---- EXTENSION: exact row segmentation onto a given palette (no reference counterpart; csrc/palette_segment.hip) ----------------------
 * rgb, palette, cls, n_classes, idx_out and idx_elem_bytes as rhccq_palette_runs takes them; penalty uint32[n_classes + 1], each entry
 * 0..16777215 (2^24 - 1).  pen(y, x) = penalty[cls[p]] when cls[p] < n_classes and penalty[n_classes] otherwise (and for every pixel when
 * cls == NULL).  Image rows are independent.  With d(x, c) = |rgb(y, x) - palette[c]|^2, per image row the call returns the labelling that
 * minimises   sum_x d(x, out(x))  +  sum over x >= 1 with out(x) != out(x - 1) of pen(x)   (the 1-D Potts segmentation), by this rule:
 *   forward   C_0(c) = d(0, c).  For x >= 1: m = min_c C_{x-1}(c), a(x) the lowest c that attains it; stay(x, c) <=> C_{x-1}(c) <= m + pen(x)
 *             (an exact tie stays); C_x(c) = d(x, c) + min(C_{x-1}(c), m + pen(x)).
 *   backward  out(W - 1) = the lowest c that attains min C_{W-1};  out(x - 1) = out(x) if stay(x, out(x)), else a(x).
 * Every comparison is between costs of one column, so the implementation subtracts m after every step and drops the part of d that all
 * rows of a pixel share; every cost stays below 2^25 and the arithmetic is int32 for any W (csrc/palette_segment.h).  What follows:
 * every pixel is within the penalties of its two boundaries of its nearest row, d(x, out(x)) <= db(x) + [x > 0] pen(x) + [x < W - 1] pen(x + 1);
 * penalty 0 keeps the remap's squared error (the indices may differ at ties); a row with W * 195075 < penalty is constant.
 * sums is uint64[n_classes + 1][4], zeroed by the call: row c = {pixels, sum of |rgb - palette[out]|^2, pixels with out != b
 * (b = rhccq_palette_remap's index), breaks} over the pixels with cls[p] == c, the last row over every pixel; a break is an x >= 1 with
 * out(x) != out(x - 1), counted in the class of pixel x.
 * RHCCQ_E_ARG: as rhccq_palette_runs, and a null penalty, a penalty above 2^24 - 1; device form: a null workspace, one not aligned to 8, or
 * work_bytes below rhccq_palette_segment_bytes(H, W, K).  RHCCQ_E_LIMIT: K > 65536; device form: K > rhccq_palette_segment_max_rows()
 * (1024: a wave owns an image row and holds the K states in registers, 16 per lane at most); host form: its tables could not be
 * allocated.  H * W == 0 succeeds with zero sums (and needs no workspace).
 * Device form: every pointer but penalty_host (copied by value into the launch) is device memory; async on the context stream, no host
 * synchronisation, nothing allocated: rhccq_palette_remap into idx_out (b), a memset, then ONE launch, a one-wave workgroup per image
 * row, that runs the row's forward pass and behind it its backward pass.  The workspace is the FULL PLANE of decisions, not only the rows in
 * flight: per image row and tile of rhccq_palette_segment_tile_cols() (32) columns, ceil(K / 64) x 64 dwords of stay bits and 32 uint16 a(x),
 * i.e. H x ceil(W / 32) x (256 ceil(K / 64) + 64) bytes (282 MB for 3840 x 2160 at K = 230).  Its contents before and after the call mean nothing.
 * Host form: the same step functions (csrc/palette_segment.h) run serially on host memory, for any K <= 65536. */
int32_t rhccq_palette_segment_max_rows(void);                         /* host only: the largest K of the device form */
int32_t rhccq_palette_segment_tile_cols(void);                        /* host only: the columns of a tile of the workspace */
int64_t rhccq_palette_segment_bytes(int32_t H, int32_t W, int32_t K); /* host only: workspace bytes (0 for arguments the device form refuses) */
int rhccq_palette_segment(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                          int32_t n_classes, const uint32_t* penalty_host, void* work, int64_t work_bytes, void* idx_out, int32_t idx_elem_bytes,
                          uint64_t* sums);
int rhccq_palette_segment_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                               const uint32_t* penalty, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);

/* ---- EXTENSION: error-diffusing remap onto a given palette (no reference counterpart; csrc/palette_dither.hip) -------------------------
 * rgb, palette, cls, n_classes, idx_out and idx_elem_bytes as rhccq_palette_runs takes them; strength uint32[n_classes + 1], each entry
 * 0..256.  s(y, x) = strength[cls[p]] when cls[p] < n_classes and strength[n_classes] otherwise (and for every pixel when cls == NULL).
 * Floyd-Steinberg error diffusion in exact integers, raster order (rows top to bottom, every row left to right, no serpentine).  With
 * E(y, x, c) the error pixel (y, x) passes on in channel c (0 outside the picture), per pixel and channel:
 *   A = 7 E(y, x-1) + E(y-1, x-1) + 5 E(y-1, x) + 3 E(y-1, x+1)                          |A| <= 4080
 *   t = clamp(rgb + floor((s A + 2048) / 4096), 0, 255)                                   floor toward minus infinity
 *   out(y, x) = rhccq_palette_remap's row of the uint8 triple t (nearest in exact integers, ties to the lowest row)
 *   E(y, x, c) = t - palette[out(y, x)][c]                                                from the clamped t, -255..255
 * The strength scales what a pixel RECEIVES: a pixel of strength 0 gets exactly the remap's index b(y, x) and still passes its own
 * error on.  Strength 0 everywhere reproduces rhccq_palette_remap's indices; 256 is Floyd-Steinberg.  idx_out receives out; sums is
 * uint64[n_classes + 1][3], zeroed by the call: row c = {pixels, sum of |rgb - palette[out]|^2 against the ORIGINAL pixel, pixels with
 * out != b} over the pixels with cls[p] == c, the last row over every pixel.
 * RHCCQ_E_ARG: as rhccq_palette_runs, and a null strength, a strength above 256; device form: a null status or one not aligned to 4, and
 * with pixels a null workspace, one not aligned to 4, or work_bytes below rhccq_palette_dither_bytes(H, W).  RHCCQ_E_LIMIT: K > 65536;
 * device form: K > rhccq_palette_dither_max_rows() (4096: the packed palette is 32 KiB of LDS and a row number 12 bits of the search's
 * word).  H * W == 0 succeeds with zero sums and *status = 0 (and needs no workspace).
 * Device form: every pointer but strength_host (copied by value into the launch) is device memory; async on the context stream, no host
 * synchronisation, nothing allocated: rhccq_palette_remap into idx_out (b), memsets of sums, status and the workspace, then ONE launch
 * that overwrites the indices where they differ.  A one-wave workgroup owns a band of RHCCQ_OPT_DITHER_ROWS image rows and walks them as a
 * wavefront, pixel (y, x) at step x + 2 y; the last row of a band hands its errors to the next band through the workspace, one 32-bit
 * word per pixel whose top bit marks it written (relaxed agent-scope atomics, no flag, no fence).  Bands take their numbers from a
 * ticket in the workspace, so a band only ever waits for one that has started: no cooperative launch, no grid sized to residency.  The
 * wait is bounded: if a band gives up, every band stops waiting and runs to its end, *status (device memory, written by the call) is
 * non-zero and the indices and sums are unspecified; *status == 0 otherwise.  The workspace's contents before and after the call mean nothing.
 * Host form: the same step functions (csrc/palette_dither.h) run serially on host memory, for any K <= 65536. */
int32_t rhccq_palette_dither_max_rows(void);                  /* host only: the largest K of the device form */
int32_t rhccq_palette_dither_rows(void);                      /* host only: the image rows of a band by default */
int64_t rhccq_palette_dither_bytes(int32_t H, int32_t W);     /* host only: workspace bytes for any RHCCQ_OPT_DITHER_ROWS (0 for H < 0 or W < 0) */
int rhccq_palette_dither(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                         int32_t n_classes, const uint32_t* strength_host, void* work, int64_t work_bytes, void* idx_out, int32_t idx_elem_bytes,
                         uint64_t* sums, int32_t* status);
int rhccq_palette_dither_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                              const uint32_t* strength, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);

/* ---- EXTENSION: a palette from the image, exact variance splits over a colour histogram (no reference counterpart; csrc/palette_build.hip) ----
 * Greedy variance-minimising box splitting over a 32 x 32 x 32 histogram (Wu's quantiser) with exact rational comparisons: the top-down
 * counterpart of rhccq_palette_reduce (the gain of a split is Ward's cost of merging the two halves back).
 *
 * rhccq_palette_cells: one pass over the pixels.  The cell of a pixel is (r >> 3, g >> 3, b >> 3).  cells is uint64[4][32][32][32] =
 * planes {N, Sr, Sg, Sb}, indexed [r >> 3][g >> 3][b >> 3]: N adds the pixel's weight, S the weight x the full 8-bit channel value, so a
 * box's mean is the exact mean of its pixels, not of cell centres.  Weights follow rhccq_palette_refine's rule: weights[cls[p]] when
 * cls[p] < n_classes and weights[n_classes] otherwise (and for every pixel when cls == NULL); 0..255 with at least one > 0, NULL = all
 * ones.  accumulate == 0: the call zeroes cells first; accumulate != 0: it adds to what is there, so the tables of several frames sum
 * into one (a shared palette for a set of images).  Integer addition only: every order gives the same table.
 * RHCCQ_E_ARG: a null rgb or cells; n_pixels < 0; n_classes outside 0..16 (or not 0 with cls == NULL); a weight outside 0..255 or all
 * weights 0; cells not aligned to 8.  RHCCQ_E_LIMIT: n_pixels x the largest weight above 2^32 - 1.  n_pixels == 0 succeeds.
 * Device form: every pointer but weights_host is device memory; rgb and cls of any alignment; async on the context stream (a memset
 * unless accumulating, one launch), nothing allocated.  A workgroup takes rhccq_palette_cells_chunk() pixels at a time, a lane 8 of them
 * rhccq_palette_cells_block() apart; a wave sums the pixels of equal cells, a workgroup collects them in a table of 1 024 cells in LDS, and
 * what is left goes to global memory with 64-bit atomics.
 *
 * rhccq_palette_build: the split chain.  A box is a half-open range of cells [lo, hi) per axis (order r, g, b); box 0 is the whole cube;
 * a box's N and S are the sums of its cells.  A cut of a box is (axis a, position t with lo_a < t < hi_a): the lower half [lo_a, t), the
 * upper half [t, hi_a); it is valid iff both halves have N > 0.  With (N, S) the box and (N1, S1) the lower half its gain is the exact
 * rational |N S1 - N1 S|^2 / (N N1 (N - N1)) (the squared norm over the three channels): the squared error the split removes.  A gain of
 * 0 is a valid cut.  The best cut of a box is the valid cut of largest gain, ties to the lowest axis, then the lowest t.  One step: among
 * the boxes that have a valid cut the one whose best cut has the largest gain is split, ties to the lowest box index; the box keeps its
 * index and becomes the lower half, the upper half gets the next free index.  The chain ends at K_target boxes or when no box has a
 * valid cut.  Gains are compared exactly by cross-multiplication: with the sum of N at most 2^32 - 1 and S <= 255 N per cell (the
 * caller's duty for a table not made by rhccq_palette_cells) a numerator is below 2^146, a denominator below 2^96, a cross product below
 * 2^242 (128 bits are not enough: a 512 x 768 picture needs 138).
 * *k_out = the number of boxes; palette_out uint8[K_target][3]: row i = floor((2 S + N) / (2 N)) per channel of box i (the refinement's
 * rounding), rows in creation order; counts_out uint64[K_target]: N of each box; boxes_out uint8[K_target][6] (may be NULL): lo then hi;
 * splits int32[K_target - 1][3] (may be NULL): (box, axis, t) per step, -1 behind the last step; rows from k_out on are zero.
 * Colours that share a cell are never separated (two colours in one cell give one row), and two boxes may round to the same row.
 * RHCCQ_E_ARG: a null cells, palette_out, counts_out, k_out (or work); K_target < 1; N all zero; misaligned cells, counts_out, work (8),
 * splits or k_out (4); work_bytes below rhccq_palette_build_bytes().  RHCCQ_E_LIMIT: K_target > 32768; the sum of N above 2^32 - 1; in
 * the device form K_target > rhccq_palette_build_max_rows().
 * Device form: every pointer is device memory; async on the context stream (three launches that form the 33^3 summed-volume tables of
 * the four planes in the workspace, then ONE resident workgroup that runs the chain with boxes and cached best cuts in LDS), no host
 * synchronisation, nothing allocated.  The two errors that only the table shows (N all zero; sum above 2^32 - 1) cannot be returned
 * without reading it: the call returns 0 and the kernel writes RHCCQ_E_ARG / RHCCQ_E_LIMIT to *k_out, zero palette_out, counts_out and
 * boxes_out, and -1 throughout splits.  Host form: the same functions (csrc/palette_build.h) run serially, for K_target <= 32768. */
int32_t rhccq_palette_cells_block(void);                /* host only: pixels between two pixels of one lane (the lanes of a workgroup) */
int32_t rhccq_palette_cells_chunk(void);                /* host only: pixels a workgroup takes at a time */
int rhccq_palette_cells(rhccq_ctx* ctx, const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights_host,
                        int32_t accumulate, uint64_t* cells);
int rhccq_palette_cells_host(const uint8_t* rgb, int64_t n_pixels, const uint8_t* cls, int32_t n_classes, const int32_t* weights,
                             int32_t accumulate, uint64_t* cells);
int32_t rhccq_palette_build_max_rows(void);             /* host only: the largest K_target of the device form (the boxes one workgroup's LDS holds) */
int64_t rhccq_palette_build_bytes(void);                /* host only: workspace bytes */
int rhccq_palette_build(rhccq_ctx* ctx, const uint64_t* cells, int32_t K_target, void* work, int64_t work_bytes, uint8_t* palette_out,
                        uint64_t* counts_out, uint8_t* boxes_out /* may be NULL */, int32_t* splits /* may be NULL */, int32_t* k_out);
int rhccq_palette_build_host(const uint64_t* cells, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out, uint8_t* boxes_out,
                             int32_t* splits, int32_t* k_out);

/* ---- EXTENSION: the palette build path for a batch of images (no reference counterpart; csrc/palette_batch.hip) ----
 * rhccq_palette_cells, rhccq_palette_build, rhccq_palette_remap and rhccq_palette_refine over B images in one call each.  Every image's
 * result is bit for bit what the single-image call gives for that image alone; nothing of one image enters another's.  The split chain of
 * one image is one workgroup for milliseconds and the rest of the card idles: B chains run on B workgroups side by side, and no call here
 * needs a host synchronisation before the next, so cells, build, refine and remap of a batch queue behind one another.
 *
 * Layout common to the four.  The B images lie back to back in one buffer: rgb is interleaved uint8 of any alignment, image b the pixels
 * [px_off[b], px_off[b + 1]) of it.  px_off is int64[B + 1] with px_off[0] == 0, never decreasing; an image of 0 pixels is legal.  The
 * device forms take it twice: px_off_host (host memory: checked, and it sizes the grid) and px_off_dev (the same values in device memory:
 * what the kernels read).  KEEPING THE TWO EQUAL IS THE CALLER'S DUTY: the call cannot compare them without a synchronisation, and
 * offsets in px_off_dev that reach outside the buffers make the kernels read and write out of bounds.  cls (may be NULL) is one uint8
 * per pixel over the same concatenation; classes and weights follow the single calls' rules, one n_classes and one weight table for the
 * batch.  Outputs per image are planes strided by image, as stated per entry.
 * RHCCQ_E_ARG, beside the single calls' rules: B < 1; a null px_off_host, px_off_dev or k_rows; px_off_host[0] != 0 or a decreasing
 * px_off_host; K_stride < 1; misaligned outputs, k_rows (4) or workspace (8); a short workspace.  RHCCQ_E_LIMIT: B > 65535 (slice the
 * batch), and the single calls' limits.
 * Device forms: every pointer but px_off_host and weights_host is device memory; async on the context stream, no host synchronisation,
 * nothing allocated, nothing copied.  In every kernel a grid row (the chain: a workgroup) is one image, so a workgroup never holds pixels
 * of two images and chunking restarts at every image boundary.  No workgroup waits for another (no flags, no spinning, no cooperative
 * launch, no grid sized to what is resident): stream order between launches is the only synchronisation, and a batch larger than the
 * card queues.  Host forms (px_off and k_rows in host memory, one px_off): a loop over the single-image host functions behind the same
 * argument checks.
 *
 * rhccq_palette_cells_batch: cells is uint64[B][4][32][32][32]; the call zeroes it (there is no accumulate mode).  A memset and one
 * launch.  RHCCQ_E_LIMIT (pixels x the largest weight above 2^32 - 1) applies per image.
 *
 * rhccq_palette_build_batch: one K_target for the batch, at most rhccq_palette_build_max_rows() in the device form.  palette_out uint8[B]
 * [K_target][3], counts_out uint64[B][K_target], k_out int32[B], boxes_out uint8[B][K_target][6] (may be NULL), splits int32[B]
 * [K_target - 1][3] (may be NULL).  The workspace is rhccq_palette_build_batch_bytes(B) = B x rhccq_palette_build_bytes().  Three prefix
 * launches over all tables, then ONE launch of B workgroups, workgroup b the chain of table b.  A table whose N is all zero, or adds up
 * to more than 2^32 - 1, gets RHCCQ_E_ARG / RHCCQ_E_LIMIT in its own k_out[b], zero rows and -1 throughout its splits; the call returns
 * 0 and its neighbours are untouched.  The host form does the same (it does not return the table's error).
 *
 * rhccq_palette_remap_batch: palettes is uint8[B][K_stride][3], k_rows int32[B] the rows in use per image (device memory in the device
 * form: rhccq_palette_build_batch's k_out goes in as it is).  Rows from k_rows[b] on are never read; a k_rows[b] above K_stride counts as
 * K_stride.  An image with k_rows[b] < 1 (a build's error code included) gets index 0 throughout and zero sums.  idx_out is concatenated
 * like rgb, idx_elem_bytes (1, 2 or 4) per element for the whole batch; 1 byte needs K_stride <= 256.  sums is uint64[B][n_classes + 1]
 * [2], rows as rhccq_palette_remap's, zeroed by the call.  A memset and one launch.
 *
 * rhccq_palette_refine_batch: rhccq_palette_refine per image, in place in palettes (uint8[B][K_stride][3], rows from k_rows[b] on
 * untouched), two launches per iteration for the whole batch.  history is uint64[B][max_iter][2], n_iter int32[B].  Image b runs
 * iteration i > 0 iff its own history[b][i - 1][1] != 0: images stop independently.  As in the single call THE HISTORY IS CONTROL STATE
 * while the call's launches are in flight: the kernels read it to decide whether to run, so it must not be written or reused before they
 * have finished.  An image of 0 pixels or with k_rows[b] < 1 runs no iteration (n_iter[b] = 0, zero history).  The workspace is
 * rhccq_palette_refine_batch_bytes(B, K_stride) = B x rhccq_palette_refine_bytes(K_stride).  The accumulators live in LDS when K_stride
 * <= rhccq_palette_refine_lds_rows() (RHCCQ_OPT_REFINE_LDS_ROWS applies), else in the workspace FOR THE WHOLE BATCH: the choice goes by the
 * stride, not by each image's rows.  Both give the same sums. */
int64_t rhccq_palette_build_batch_bytes(int32_t B);                      /* host only: workspace bytes (0 for B < 1) */
int64_t rhccq_palette_refine_batch_bytes(int32_t B, int32_t K_stride);   /* host only: workspace bytes (0 for B < 1 or K_stride < 1) */
int rhccq_palette_cells_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B, const uint8_t* cls,
                              int32_t n_classes, const int32_t* weights_host, uint64_t* cells);
int rhccq_palette_cells_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, const uint8_t* cls, int32_t n_classes, const int32_t* weights,
                                   uint64_t* cells);
int rhccq_palette_build_batch(rhccq_ctx* ctx, const uint64_t* cells, int32_t B, int32_t K_target, void* work, int64_t work_bytes, uint8_t* palette_out,
                              uint64_t* counts_out, uint8_t* boxes_out /* may be NULL */, int32_t* splits /* may be NULL */, int32_t* k_out);
int rhccq_palette_build_batch_host(const uint64_t* cells, int32_t B, int32_t K_target, uint8_t* palette_out, uint64_t* counts_out, uint8_t* boxes_out,
                                   int32_t* splits, int32_t* k_out);
int rhccq_palette_remap_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B,
                              const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, void* idx_out,
                              int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_remap_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows,
                                   const uint8_t* cls, int32_t n_classes, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_refine_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, int32_t B, uint8_t* palettes,
                               int32_t K_stride, const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, const int32_t* weights_host,
                               int32_t max_iter, void* work, int64_t work_bytes, uint64_t* history, int32_t* n_iter);
int rhccq_palette_refine_batch_host(const uint8_t* rgb, const int64_t* px_off, int32_t B, uint8_t* palettes, int32_t K_stride, const int32_t* k_rows,
                                    const uint8_t* cls, int32_t n_classes, const int32_t* weights, int32_t max_iter, uint64_t* history, int32_t* n_iter);

/* ---- EXTENSION: position-only (pattern) dither onto a given palette (no reference counterpart; csrc/palette_pattern.hip) ----------------
 * rgb, palette, cls, n_classes, idx_out and idx_elem_bytes as rhccq_palette_runs takes them; strength uint32[n_classes + 1], each entry
 * 0..256, chosen per pixel as rhccq_palette_dither chooses it: s = strength[cls[p]] when cls[p] < n_classes and strength[n_classes]
 * otherwise (and for every pixel when cls == NULL).  size n is 2, 4 or 8, N = n * n.  Thomas Knoll's pattern dithering in exact integers.
 * Per pixel p = rgb(y, x), with e an error triple that starts at (0, 0, 0), for i = 0 .. N-1 and per channel:
 *   t   = clamp(p + floor((s e + 128) / 256), 0, 255)                                     floor toward minus infinity
 *   c_i = rhccq_palette_remap's row of the uint8 triple t (nearest in exact integers, ties to the lowest row)
 *   e   = e + p - palette[c_i]                                                            against the ORIGINAL pixel; |e| <= 64 * 255
 * The N candidates, duplicates kept, are ordered by (299 R + 587 G + 114 B of palette[c_i], then c_i) ascending, and
 *   out(y, x) = ordered[M_n[y mod n][x mod n]],   M_2 = [[0, 2], [3, 1]],   M_2n = [[4 M_n, 4 M_n + 2], [4 M_n + 3, 4 M_n + 1]]   (Bayer)
 * out depends on the pixel's value, class and position modulo n only: the same pixel at the same (y mod n, x mod n) gets the same index in
 * any picture, tile, frame or batch slot.  c_0 is rhccq_palette_remap's index b (the first target is the pixel itself), and a strength
 * of 0 makes every candidate b: strength 0 everywhere reproduces rhccq_palette_remap's indices for every size.  idx_out receives out; sums
 * is uint64[n_classes + 1][3], zeroed by the call: row c = {pixels, sum of |rgb - palette[out]|^2 against the ORIGINAL pixel, pixels with
 * out != b} over the pixels with cls[p] == c, the last row over every pixel, exactly as rhccq_palette_dither defines it.
 * RHCCQ_E_ARG: as rhccq_palette_runs, and a null strength, a strength above 256, a size other than 2, 4, 8.  RHCCQ_E_LIMIT: K > 65536
 * (tested before the strengths); device form: K > rhccq_palette_pattern_max_rows() (4096: the packed palette is 32 KiB of LDS and a row
 * number 12 bits of the search's word).  H * W == 0 succeeds with zero sums.
 * Device form: every pointer but strength_host (copied by value into the launch) is device memory; async on the context stream, no host
 * synchronisation, nothing allocated, no workspace and no status word: a memset of sums and ONE launch.  Pixels are independent: the kernel
 * is the remap's search run N times per pixel against the whole palette in LDS, a lane's candidates in an LDS strip of 16-bit rows; no
 * workgroup waits for another.  (y, x) comes from the linear pixel index.
 * Host form: the same step functions (csrc/palette_pattern.h) run serially on host memory, for any K <= 65536.
 * Batched form: B images laid out as rhccq_palette_remap_batch takes them (px_off host and device, palettes uint8[B][K_stride][3], k_rows
 * int32[B] read on the device, one n_classes, strength table and size for the batch), and the width of every image twice, as px_off:
 * widths_host int32[B] (checked) and widths_dev (what the kernel reads; KEEPING THE TWO EQUAL IS THE CALLER'S DUTY).  An image's width
 * must divide its pixels; an image of 0 pixels may have width 0.  Image b's indices and sums (uint64[B][n_classes + 1][3]) are bit for bit
 * what the single call gives for it alone; an image with k_rows[b] < 1 gets index 0 throughout and zero sums.  RHCCQ_E_ARG beside the
 * single call's and rhccq_palette_remap_batch's: a null widths_host or widths_dev, a misaligned widths_dev, a width that is negative or
 * does not divide its image's pixels.  RHCCQ_E_LIMIT: K_stride > 4096 (device form), B > 65535.  A memset and one launch, one image per
 * grid row; the host form loops over rhccq_palette_pattern_host. */
int32_t rhccq_palette_pattern_max_rows(void);                 /* host only: the largest K of the device form */
int rhccq_palette_pattern(rhccq_ctx* ctx, const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls,
                          int32_t n_classes, const uint32_t* strength_host, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_pattern_host(const uint8_t* rgb, int32_t H, int32_t W, const uint8_t* palette, int32_t K, const uint8_t* cls, int32_t n_classes,
                               const uint32_t* strength, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_pattern_batch(rhccq_ctx* ctx, const uint8_t* rgb, const int64_t* px_off_host, const int64_t* px_off_dev, const int32_t* widths_host,
                                const int32_t* widths_dev, int32_t B, const uint8_t* palettes, int32_t K_stride, const int32_t* k_rows, const uint8_t* cls,
                                int32_t n_classes, const uint32_t* strength_host, int32_t size, void* idx_out, int32_t idx_elem_bytes, uint64_t* sums);
int rhccq_palette_pattern_batch_host(const uint8_t* rgb, const int64_t* px_off, const int32_t* widths, int32_t B, const uint8_t* palettes, int32_t K_stride,
                                     const int32_t* k_rows, const uint8_t* cls, int32_t n_classes, const uint32_t* strength, int32_t size, void* idx_out,
                                     int32_t idx_elem_bytes, uint64_t* sums);

/* ---- EXTENSION: indexed PNG files written on the device (no reference counterpart; csrc/png_write.hip, csrc/png_write.h) ------------------
 * The file of an index map idx[H][W] (idx_elem_bytes 1, 2 or 4, read as unsigned) and a palette uint8[K][3], H, W >= 1, 1 <= K <= 65536:
 *   index clamp   an index >= K is written as 0, the row rhccq_decode shows for it.
 *   K <= 256      colour type 3.  Bit depth d = 1 (K <= 2), 2 (K <= 4), 4 (K <= 16), else 8; RHCCQ_PNG_DEPTH8 forces 8.  PLTE holds exactly K
 *                 entries.  Every row has filter type 0.  Pixels are packed most significant bits first, the unused low bits of a row's
 *                 last byte are zero; a row is 1 + ceil(W d / 8) bytes.
 *   K > 256       colour type 2, depth 8: a row's raw bytes are palette[idx], R G B, bpp = 3, a row is 1 + 3 W bytes.  Each row takes the
 *                 filter type among 0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth that minimises the sum over its filtered bytes v of
 *                 (v < 128 ? v : 256 - v); a tie goes to the lowest type.  Left and upper left of the first pixel and the row above row 0
 *                 are zero; Average is floor((a + b) / 2); Paeth prefers a, then b, then c, with <= as the specification words it; Up reads
 *                 the raw row above, so rows are independent.  RHCCQ_PNG_NO_FILTER writes type 0 on every row.
 *   chunks        signature, IHDR (W, H, depth, colour type, 0, 0, 0), PLTE (colour type 3 only), ONE IDAT holding the zlib stream of all
 *                 scanlines, IEND, and nothing else.  The stream is rhccq_zlib_compress's, or rhccq_zlib9_compress's with
 *                 RHCCQ_PNG_EXACT (then the file is a function of idx, palette and flags alone, byte for byte what zlib.compress(scan, 9)
 *                 gives inside the same framing).  Every CRC is the standard CRC-32 (zlib.crc32) over chunk type and data.
 * RHCCQ_E_ARG: H < 1, W < 1, K outside 1..65536, idx_elem_bytes not 1, 2 or 4, flag bits other than the three below, a null pointer
 * (filter_rows and n_dev may be null), an idx not aligned to its element.  RHCCQ_E_LIMIT: scanline bytes (H rows) beyond what the chosen
 * encoder takes (both refuse 2 GiB; rhccq_png_scanlines applies the level-9 encoder's limit), out_cap below the bound.
 * Device forms: every pointer is device memory; async on the context stream, no host synchronisation, nothing allocated.
 *   rhccq_png_scanlines   scan receives H rows; filter_rows (device int64[5], may be NULL) how many rows took each filter type.  Colour type 3 is
 *                         one launch over the output's 4-byte words (a lane builds a whole word and stores it once; the first and last
 *                         bytes of a misaligned scan go bytewise); colour type 2 is one launch with a workgroup per image row: the five costs
 *                         in one pass, a reduction, the winner written in a second pass.
 *   rhccq_crc32           zlib.crc32 of data[0 .. n), n = *n_dev (device int64, clamped to 0..n_cap) or n_cap when n_dev is NULL, into
 *                         *crc_out (device).  Two launches: a workgroup takes the plain remainder of a 16 KiB piece (slice-by-4 tables in
 *                         LDS), then ONE workgroup joins the remainders by multiplying with x^(8 len) mod P as a tree (zlib's crc32_combine
 *                         algebra).  No workgroup waits for another; pieces past n contribute nothing; bytes outside data[0 .. n) are
 *                         read only within the 16-byte aligned blocks that hold a byte of it, and masked.  workspace: at least
 *                         rhccq_crc32_bytes(n_cap) bytes, aligned to 4.
 *   rhccq_png_encode      the whole file into out, its length into *out_len (device int64).  workspace (aligned to 256) and out_cap come from
 *                         rhccq_png_sizes.  One launch writes signature, IHDR, PLTE (the palette is device memory) and IDAT's type, one the
 *                         scanlines into the workspace, the encoder writes its stream behind IDAT's type, the CRC runs over type and stream
 *                         with the stream's device-side length, and a last launch writes IDAT's length, its CRC and IEND.  Afterwards the
 *                         workspace holds the scanlines at its start and, 16 bytes behind them rounded up to 256, filter_rows (int64[5]).
 * Host forms (serial, no GPU, host memory): the same functions of csrc/png_write.h.  rhccq_png_encode_host needs RHCCQ_PNG_EXACT (RHCCQ_E_ARG
 * without it: the fast encoder has no host form) and an out_cap of at least rhccq_png_sizes' bound. */
#define RHCCQ_PNG_EXACT 1
#define RHCCQ_PNG_DEPTH8 2
#define RHCCQ_PNG_NO_FILTER 4
/* host only: bytes of the scanlines, of rhccq_png_encode's workspace and the bound of the file (any of the three may be NULL) */
int rhccq_png_sizes(int32_t H, int32_t W, int32_t K, int32_t flags, int64_t* scan_bytes, int64_t* workspace_bytes, int64_t* out_bound);
int rhccq_png_scanlines(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K,
                        int32_t flags, uint8_t* scan, int64_t* filter_rows);
int64_t rhccq_crc32_bytes(int64_t n_cap);                     /* host only: rhccq_crc32's workspace; negative for n_cap < 0 */
int rhccq_crc32(rhccq_ctx* ctx, const uint8_t* data, int64_t n_cap, const int64_t* n_dev, void* workspace, uint32_t* crc_out);
int rhccq_png_encode(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K,
                     int32_t flags, void* workspace, uint8_t* out, int64_t out_cap, int64_t* out_len);
int rhccq_png_scanlines_host(const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags,
                             uint8_t* scan, int64_t* filter_rows);
int rhccq_crc32_host(const uint8_t* data, int64_t n, uint32_t* crc_out);
int rhccq_png_encode_host(const void* idx, int32_t idx_elem_bytes, int32_t H, int32_t W, const uint8_t* palette, int32_t K, int32_t flags,
                          uint8_t* out, int64_t out_cap, int64_t* out_len);

/* ---- EXTENSION: PNG files read on the device (no reference counterpart; csrc/png_read.hip, csrc/png_read.h) --------------------------------
 * Files accepted.  The 8-byte signature, then chunks (length, type, data, CRC-32 over type and data).  IHDR first, 13 bytes, W, H in
 * 1..2^31 - 1; (colour type, depth) one of 0:{1,2,4,8,16}, 2:{8,16}, 3:{1,2,4,8}, 4:{8,16}, 6:{8,16}; compression 0, filter method 0;
 * interlace 0 (interlace 1: RHCCQ_PNG_UNSUPPORTED).  PLTE (3 K bytes, 1 <= K <= 256) is required before IDAT for colour type 3, ignored for
 * types 2 and 6, an error for types 0 and 4.  tRNS (before IDAT; behind PLTE for type 3) is optional: type 3 up to K alpha bytes (missing
 * ones are 255), type 0 one 16-bit key, type 2 three, types 4 and 6 an error.  At least one IDAT; IDATs are consecutive, of any lengths
 * (zero included), their payloads joined are ONE zlib stream.  IEND (empty) is required, bytes behind it are ignored.  Any other chunk
 * whose first type byte has bit 5 set is skipped (its CRC is still checked); an unknown critical chunk is an error.
 * Status.  One RHCCQ_PNG_* status and one detail word; of several faults the one that stands first below is reported:
 *   BAD_SIGNATURE
 *   BAD_CHUNK      framing: a chunk that runs past the end of the file (or a length above 2^31 - 1), IHDR not first or repeated, PLTE / tRNS
 *                  repeated or behind IDAT, IDATs not consecutive, a non-empty IEND, no IDAT, no IEND, an unknown critical chunk; and, where
 *                  the header is valid, what it decides: PLTE missing (type 3) or present (types 0, 4), PLTE's or tRNS's length, tRNS in front
 *                  of PLTE (type 3) or present at all (types 4, 6).  detail: the index of the chunk at which the fault shows, or the number
 *                  of chunks where one is missing
 *   BAD_HEADER     IHDR's length or contents
 *   UNSUPPORTED    interlace 1
 *   LIMIT          scanline bytes H (1 + rowbytes), or IDAT bytes, of 2^31 or more: the inflater's limit
 *   BAD_CRC        detail: the index of the first chunk whose CRC does not match
 *   BAD_STREAM     detail: the RHCCQ_ZS_* code of the zlib stream
 *   BAD_LENGTH     the stream does not inflate to exactly H (1 + rowbytes) bytes (it is inflated with that out_cap); detail: the length it
 *                  has (or needs), clamped to 2^31 - 1
 *   BAD_FILTER     detail: the first row whose filter type byte is above 4
 *   STALLED        the unfilter's bounded wait between bands ran out (see below); never seen on a device that makes progress
 * BAD_SIGNATURE .. LIMIT are decided by rhccq_png_parse_host, a pure function of the file's bytes, before any device work.
 * Unfilter.  The PNG specification's: bpp = max(1, channels * depth / 8) bytes, rowbytes = ceil(W * channels * depth / 8); bytes left of a
 * row and the row above row 0 are zero; arithmetic modulo 256; Average adds floor((a + b) / 2) computed in 9 bits; Paeth has p = a + b - c
 * and prefers a, then b, then c, with <= as the specification words it.  A row whose type byte is above 4 is copied as type 0.
 * Expand.  Samples below 8 bits are unpacked most significant bits first; grey at depth d < 8 is scaled by 255 / (2^d - 1), exactly; a 16-bit
 * sample gives its high byte; grey goes to R = G = B; colour type 3 gives palette[idx], an index at or past K shows row 0 (rhccq_decode's
 * rule).  Alpha is the alpha channel (its high byte at 16 bits), or the tRNS entry of the index (255 past the entries), or 0 where the
 * full-depth samples equal the tRNS key (its low `depth` bits) and 255 elsewhere, or 255 where the file has none.
 * Device forms: every pointer but info is device memory; async on the context stream, no host synchronisation, nothing allocated.  Every
 * stage stays inside its buffers for ANY bytes: offsets and lengths of a table are tested against n again inside the kernels.
 *   rhccq_crc32_segments  crc_out[i] = zlib.crc32(data[offset_i .. offset_i + length_i + extra)) for the n_seg rows of a table in TWO launches
 *                         whatever n_seg is: a workgroup per (segment, 16 KiB piece) takes a plain remainder as rhccq_crc32 does (it finds
 *                         its segment by a search over first_piece), then a wave per segment joins its pieces.  No workgroup waits for
 *                         another.  data must be aligned to 16; the table's first_piece column and total_pieces come from
 *                         rhccq_crc32_segments_plan (host only), workspace is 4 * total_pieces bytes (at least 4), aligned to 4.  A row that
 *                         does not lie inside data[0 .. n) counts as empty.
 *   rhccq_png_unfilter    scan: H rows of 1 + rowbytes bytes (rowbytes a multiple of bpp, bpp 1, 2, 3, 4, 6 or 8) -> raw_out: H rows of
 *                         rowbytes bytes.  A one-wave workgroup owns a band of rhccq_png_unfilter_band_rows() rows, a lane a row; at step u
 *                         lane r stands at the filter unit (bpp bytes) u - r, takes "above" from lane r - 1 across lanes and keeps left and
 *                         upper left in registers; bytes go through LDS tiles of rhccq_png_unfilter_tile() steps.  The last row of a band
 *                         reaches the next band through words of the workspace that carry three bytes and a mark, fetched
 *                         rhccq_png_unfilter_granule() units at a time.  A band's number is a ticket drawn at its start, so it waits only
 *                         for bands that have started; a band whose first row has type 0 or 1 waits for nothing; every wait is bounded (past
 *                         the bound: STALLED, and the output means nothing).  status (device int32[2]): OK, BAD_FILTER or STALLED and the
 *                         detail.  workspace: rhccq_png_unfilter_bytes(H, rowbytes, bpp) bytes, aligned to 4.
 *   rhccq_png_expand      raw rows -> rgb[H][W][3], alpha[H][W] (may be NULL), idx[H][W] (may be NULL; written for colour type 3 only).
 *                         palette: K rows of 3 bytes (type 3), trns: trns_bytes bytes as the chunk holds them (may be NULL with 0).
 *   rhccq_png_decode      segment CRCs (unless RHCCQ_PNG_READ_NO_CRC), IDAT join (one launch over the joined stream: a lane finds the chunk
 *                         of its 16 bytes by a search over the table), rhccq_zlib_decompress, unfilter, expand, and one launch that keeps
 *                         the first failing stage's status by the precedence above in status (device int32[2]).  Later stages run on whatever
 *                         they get.  info and the table are rhccq_png_parse_host's (the table copied to the device, file aligned to 16);
 *                         with info->status set nothing runs but the launch that writes it to status.  workspace: rhccq_png_read_sizes,
 *                         aligned to 256; afterwards the scanlines lie at rhccq_png_read_scan_offset(info) in it.
 * Host forms (serial, no GPU, host memory): the same step functions of csrc/png_read.h. */
#define RHCCQ_PNG_OK 0
#define RHCCQ_PNG_BAD_SIGNATURE 1
#define RHCCQ_PNG_BAD_CHUNK 2
#define RHCCQ_PNG_BAD_HEADER 3
#define RHCCQ_PNG_UNSUPPORTED 4
#define RHCCQ_PNG_LIMIT 5
#define RHCCQ_PNG_BAD_CRC 6
#define RHCCQ_PNG_BAD_STREAM 7
#define RHCCQ_PNG_BAD_LENGTH 8
#define RHCCQ_PNG_BAD_FILTER 9
#define RHCCQ_PNG_STALLED 10
#define RHCCQ_PNG_READ_NO_CRC 1
/* a byte range of one buffer.  As a PNG chunk: offset is that of the chunk's type field, length its data length (the CRC covers
   length + 4 bytes from offset), dst the offset of an IDAT's payload in the joined stream, -1 for every other chunk */
typedef struct rhccq_segment {
  int64_t offset, length, first_piece, dst;
} rhccq_segment;
typedef struct rhccq_png_info {
  int32_t status, detail;                 /* RHCCQ_PNG_OK .. RHCCQ_PNG_LIMIT */
  int32_t width, height, depth, colour_type, interlace, channels, bpp;
  int32_t palette_rows, trns_bytes;       /* K (0 unless colour type 3); bytes of tRNS (0: none) */
  int32_t n_chunks, first_idat, n_idat;   /* chunks walked; the IDATs are chunks first_idat .. first_idat + n_idat - 1 */
  int64_t rowbytes, scan_bytes;           /* H (1 + rowbytes) */
  int64_t plte_offset, trns_offset;       /* of the chunks' data, -1 without */
  int64_t idat_bytes, crc_pieces;         /* the joined stream; total_pieces of the chunk table (extra 4) */
} rhccq_png_info;
/* host only.  RHCCQ_E_ARG for a null file (with n > 0), info or n_chunks, n < 0, or chunks_cap < 0; otherwise RHCCQ_OK with info->status set.
   chunks (may be NULL with chunks_cap 0) receives the first chunks_cap rows, *n_chunks their full number (at most n / 12) */
int rhccq_png_parse_host(const uint8_t* file, int64_t n, rhccq_png_info* info, rhccq_segment* chunks, int64_t chunks_cap, int64_t* n_chunks);
/* host only: fills first_piece of every row and *total_pieces */
int rhccq_crc32_segments_plan(rhccq_segment* table, int64_t n_seg, int64_t extra, int64_t* total_pieces);
int rhccq_crc32_segments(rhccq_ctx* ctx, const uint8_t* data, int64_t n, const rhccq_segment* table_dev, int64_t n_seg, int64_t extra,
                         int64_t total_pieces, void* workspace, uint32_t* crc_out);
int rhccq_crc32_segments_host(const uint8_t* data, int64_t n, const rhccq_segment* table, int64_t n_seg, int64_t extra, uint32_t* crc_out);
int32_t rhccq_png_unfilter_band_rows(void);
int32_t rhccq_png_unfilter_tile(void);
int32_t rhccq_png_unfilter_granule(void);
int64_t rhccq_png_unfilter_bytes(int32_t H, int64_t rowbytes, int32_t bpp);       /* host only; negative for bad arguments */
int rhccq_png_unfilter(rhccq_ctx* ctx, const uint8_t* scan, int32_t H, int64_t rowbytes, int32_t bpp, uint8_t* raw_out, void* workspace,
                       int32_t* status);
int rhccq_png_unfilter_host(const uint8_t* scan, int32_t H, int64_t rowbytes, int32_t bpp, uint8_t* raw_out, int32_t* status);
int rhccq_png_expand(rhccq_ctx* ctx, const uint8_t* raw, int32_t H, int32_t W, int32_t colour_type, int32_t depth, const uint8_t* palette,
                     int32_t K, const uint8_t* trns, int32_t trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx);
int rhccq_png_expand_host(const uint8_t* raw, int32_t H, int32_t W, int32_t colour_type, int32_t depth, const uint8_t* palette, int32_t K,
                          const uint8_t* trns, int32_t trns_bytes, uint8_t* rgb, uint8_t* alpha, uint8_t* idx);
/* the IDAT join alone: idat_dev holds the n_idat IDAT rows of a chunk table (dst ascending from 0), stream (aligned to 16) receives
   `total` bytes, rounded up to 16 with zeros */
int rhccq_png_join(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_segment* idat_dev, int32_t n_idat, int64_t total, uint8_t* stream);
/* host only: rhccq_png_decode's workspace for a parsed file of n bytes */
int rhccq_png_read_sizes(const rhccq_png_info* info, int64_t n, int64_t* workspace_bytes);
int64_t rhccq_png_read_scan_offset(const rhccq_png_info* info);
int rhccq_png_decode(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_png_info* info, const rhccq_segment* table_dev, int32_t flags,
                     void* workspace, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status);
/* file in host memory; parses it itself; status: host int32[2] */
int rhccq_png_decode_host(const uint8_t* file, int64_t n, int32_t flags, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status);

/* ---- EXTENSION: GIF files written on the device (no reference counterpart; csrc/gif_write.hip, csrc/gif_write.h) ---------------------------
 * The file of n_frames >= 1 index maps idx[n_frames][H][W] (idx_elem_bytes 1, 2 or 4, read as unsigned), H, W in 1..65535, over palettes of
 * 1..256 rows uint8[K][3].  The file is a pure function of the arguments; device form and host form agree byte for byte.
 *   layout        "GIF89a", the logical screen descriptor (W, H, packed, 0, 0).  EITHER one global colour table (packed = 0x80 | (tb - 1) << 4
 *                 | (tb - 1)) OR, with RHCCQ_GIF_LOCAL, a local table in every frame (packed = 0x70), never both.  A table has 2^tb
 *                 entries, tb = max(1, bits(entries - 1)): the palette's rows first, zeros behind them.  With more than one frame a
 *                 NETSCAPE2.0 application extension carries the loop count (0..65535).  Every frame: a graphic control extension (4 bytes:
 *                 disposal method 1 "do not dispose", the frame's delay in centiseconds 0..65535, transparency flag and index), an image
 *                 descriptor at (0, 0) of W x H, not interlaced, the local table if any, the minimum code size m = max(2, tb), the code
 *                 stream in sub-blocks of 255 bytes (the last one shorter), a zero byte.  The trailer 0x3B.  The file stays below 2^31 bytes.
 *   pixels        an index at or past the palette's rows is written as 0 (rhccq_png_encode's rule).
 *   delta         RHCCQ_GIF_DELTA: global table and K <= 255 only.  The transparent index T = K counts as an entry for tb and m.  In every
 *                 frame f > 0 a pixel whose clamped index equals frame f - 1's at the same position is written as T, and the frame's
 *                 extension carries the transparency flag and T; frame 0 is written in full, without the flag.
 *   code stream   clear = 2^m, end = clear + 1.  The stream opens with Clear at m + 1 bits.  The frame's pixels in raster order are cut into
 *                 segments of S = rhccq_gif_segment_pixels() = 16 384 pixels (the last may be shorter).  A segment starts with next = clear
 *                 + 2, width = m + 1 and an empty dictionary and runs the greedy LZW: the current string is extended while (string, pixel)
 *                 is in the dictionary, else the string's code goes out at `width` bits.  After EVERY data code, the segment's last
 *                 included: entry `next` is consumed (it holds (string, pixel) where a pixel follows, nothing behind the segment's last
 *                 code); if next == 2^width and width < 12 then width += 1; next += 1.  If next == 4096 and another pixel of the segment
 *                 follows, Clear goes out at `width` bits and the segment's state starts again.  Behind its last data code a segment emits,
 *                 at the width that step left, Clear if another segment follows and End otherwise.  Codes are packed least significant
 *                 bit first; the stream is padded with zero bits to a byte.
 * RHCCQ_E_ARG (before any device work): n_frames < 1 (or above 2^20), H or W outside 1..65535, a table of 0 or more than 256 rows or more than
 * k_stride, idx_elem_bytes not 1, 2 or 4, unknown flag bits, RHCCQ_GIF_DELTA with RHCCQ_GIF_LOCAL or with 256 rows, a delay or loop outside
 * 0..65535, a null pointer, an idx not aligned to its element, a workspace not aligned to 256, out_len / stream_bytes not aligned to 8.
 * RHCCQ_E_LIMIT: a bound of 2^31 bytes or more, more than 2^30 segments, out_cap or stream_stride below rhccq_gif_sizes' bounds.
 * k_rows, delays: HOST tables.  k_rows has one entry (global table) or n_frames (RHCCQ_GIF_LOCAL); delays has n_frames.  palettes: device,
 * uint8[K][3] (global) or uint8[n_frames][k_stride][3] (local; frame f shows the first k_rows[f] rows of its block).
 * Device forms: async on the context stream, no host synchronisation, nothing allocated, no workgroup waits for another.  idx is read in
 * aligned 16-byte blocks: where idx or a frame's first pixel is not aligned to 16, up to 15 bytes in front of the first and behind the last
 * index are read (never across a page, always together with a byte of idx) and not used.  RHCCQ_GIF_TRIE picks the other dictionary of
 * the LZW launch; the file does not change.
 *   rhccq_gif_lzw      the n code streams alone: frame f's bytes at streams + f * stream_stride, its length in stream_bytes[f] (device int64).
 *   rhccq_gif_encode   the whole file into out, its length into *out_len (device int64).  One launch runs the LZW of all (frame, segment)
 *                      pairs (a one-wave workgroup each, the dictionary in LDS, packed 32-bit words into the segment's slot of the workspace),
 *                      one the prefix sums of the segments' bit counts, one the frames' places in the file, one the framing, and one joins
 *                      the segments: a lane per 32-bit word of a frame's stream gathers the segments that cover it and stores its bytes
 *                      at their sub-blocked places.  Afterwards the workspace holds the frames' stream lengths (int64[n_frames]) at its start.
 * Host forms (serial, no GPU, host memory): the same step functions of csrc/gif_write.h; stream_bytes (host int64[n_frames]) may be NULL in
 * rhccq_gif_encode_host. */
#define RHCCQ_GIF_LOCAL 1
#define RHCCQ_GIF_DELTA 2
#define RHCCQ_GIF_TRIE 4      /* the segments' dictionary is a sibling-linked trie (16 KiB of LDS) instead of the hash table (32 KiB): the same bytes */
int32_t rhccq_gif_segment_pixels(void);
/* host only: bytes of the workspace, the bound of one frame's code stream and of the file (any of the three may be NULL) */
int rhccq_gif_sizes(int32_t n_frames, int32_t H, int32_t W, int32_t flags, int64_t* workspace_bytes, int64_t* stream_bound, int64_t* out_bound);
int rhccq_gif_lzw(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const int32_t* k_rows, int32_t flags,
                  void* workspace, uint8_t* streams, int64_t stream_stride, int64_t* stream_bytes);
int rhccq_gif_encode(rhccq_ctx* ctx, const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const uint8_t* palettes,
                     int32_t k_stride, const int32_t* k_rows, const int32_t* delays, int32_t loop, int32_t flags, void* workspace, uint8_t* out,
                     int64_t out_cap, int64_t* out_len);
int rhccq_gif_lzw_host(const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const int32_t* k_rows, int32_t flags,
                       uint8_t* streams, int64_t stream_stride, int64_t* stream_bytes);
int rhccq_gif_encode_host(const void* idx, int32_t idx_elem_bytes, int32_t n_frames, int32_t H, int32_t W, const uint8_t* palettes, int32_t k_stride,
                          const int32_t* k_rows, const int32_t* delays, int32_t loop, int32_t flags, uint8_t* out, int64_t out_cap, int64_t* out_len,
                          int64_t* stream_bytes);

/* ---- EXTENSION: GIF files read on the device (no reference counterpart; csrc/gif_read.hip, csrc/gif_read.h) --------------------------------
 * Framing.  "GIF87a" or "GIF89a", the logical screen descriptor (W, H, packed, background, aspect), a global colour table of 2 << (packed & 7)
 * rows if packed & 0x80.  Then any sequence of extensions (0x21, a label, sub-blocks up to a zero length) and images (0x2C) up to the trailer
 * 0x3B; bytes behind the trailer are ignored.  Of the extensions the graphic control extension (label 0xF9, first sub-block of 4 bytes or
 * more: disposal = (flags >> 2) & 7, the transparent index if flags & 1, the delay in centiseconds) and the loop count of an application
 * extension (label 0xFF, first sub-block the 11 bytes "NETSCAPE2.0" or "ANIMEXTS1.0", then a sub-block of 3 bytes or more that starts with
 * 1: the first one counts) are read, every other one is skipped sub-block by sub-block.  A graphic control extension applies to the next
 * image only (the last one in front of it).  An image: x, y, w, h, packed (0x80 a local table of 2 << (packed & 7) rows follows, 0x40
 * interlaced), the local table, the minimum code size m in 2..8, data sub-blocks of 1..255 bytes, a zero byte.
 * Code stream.  A frame's sub-blocks joined; codes are packed least significant bit first.  clear = 2^m, end = clear + 1.  The decoder
 * starts in the state behind a Clear (an opening Clear is usual, not required).  Behind a Clear (or the start) the codes are counted
 * j = 0, 1, ...; code j has width(j) = min(12, bit_length(clear + 1 + j)) bits.  Code j >= 1 creates entry e = clear + 1 + j = (string of
 * code j - 1) + (first pixel of the string of code j) while e < 4096; once the table is full 12-bit codes go on and create nothing until a
 * Clear (a deferred Clear).  The stream ends at End or where fewer bits remain than the next code needs; bits and sub-blocks behind End are
 * ignored.  A valid code j is < clear for j = 0 and <= min(clear + 1 + j, 4095) otherwise (code j == e is the string of code j - 1 and its
 * own first pixel).
 * Pixels.  A frame must decode to exactly w x h pixels.  The rows of an interlaced frame arrive in four passes (rows 0, 8, ..; 4, 12, ..;
 * 2, 6, ..; 1, 3, ..) and are put back.  Index i shows row i of the frame's table, the local one if there is one, else the global one; an
 * index at or past the table's rows shows (0, 0, 0).
 * Composition.  The canvas is the logical screen; a pixel is a colour and a covered bit, at the start (0, 0, 0) and not covered.  Frame f
 * paints every pixel of its rectangle whose index is not its transparent index: colour, covered.  images[f] and alpha[f] (255 covered, 0
 * not) are the canvas after painting.  Then the frame's disposal: 0, 1, 4..7 keep the canvas; 2 makes the rectangle (0, 0, 0), not
 * covered; 3 puts the rectangle back to what it was before the frame painted.
 * Status.  One RHCCQ_GIFR_* status and one detail word.  The host parser walks the file once and reports the first fault it meets:
 *   BAD_SIGNATURE  fewer than 6 bytes or another signature; detail 0
 *   TRUNCATED      the file ends inside a block or without a trailer; detail: the offset of that block's first byte (6 for the screen
 *                  descriptor, 13 for the global table, the introducer's offset for an extension or image, n where the trailer is missing)
 *   BAD_BLOCK      an introducer other than 0x21, 0x2C, 0x3B; detail: its offset
 *   BAD_HEADER     a screen of zero width or height (detail 6), or m outside 2..8 (detail: the offset of m)
 *   BAD_FRAME      an image of zero width or height or one that leaves the screen; detail: the frame (tested before its table and m)
 *   NO_TABLE       neither a local nor a global table; detail: the frame
 *   NO_FRAMES      the trailer is met and no image was; detail 0
 *   LIMIT          at the image 2^20 + 1, or at the trailer: the file, the images F x H x W x 3, or the segment table (below) of 2^31
 *                  bytes or more; detail 0
 * and the device, for a file the parser accepts, the lowest frame with a fault:
 *   BAD_CODE       an invalid code; detail: the frame
 *   BAD_LENGTH     the frame's strings are not w x h pixels in all; detail: the frame (BAD_CODE wins in the same frame)
 * An invalid code is decoded as code 0; a refused file's outputs mean nothing, and no stage leaves its buffers whatever the bytes are.
 * Decoding.  A segment is the run of data codes between two Clears (or the start, End, the end of the bits); an empty one is dropped.  All
 * bit offsets in a segment are a closed form of j, so nothing but the walk from segment to segment is serial:
 *   join      the sub-blocks of all frames -> one stream a frame, each at a 16-byte aligned offset with at least 16 zero bytes behind it;
 *   scan      a workgroup a frame: rhccq_gif_read_scan_step() codes a step (four tiles of rhccq_gif_read_tile()) are tested for Clear, End
 *             and the end of the bits; the first hit closes the segment (start bit, codes) into the frame's rows of the segment table;
 *   plan      the frames' segment counts -> their places in one work list;
 *   lengths   a workgroup takes (frame, segment) pairs off the list: the codes are loaded by offset and tested, prefix links go to LDS, the
 *             chains len[e] = len[prefix[e]] + 1, first[e] = first[prefix[e]] are resolved by pointer doubling (12 rounds), the entries
 *             packed prefix 12 | suffix 8 | len 12 bits; the segment's pixel total goes to its row;
 *   offsets   a workgroup a frame: prefix sums of the totals (saturating at 2^32 - 1), the frame's pixel count, BAD_LENGTH;
 *   emit      as lengths, then a tile of codes at a time: a prefix sum of len[code j], and every lane writes its code's string backwards
 *             along the prefix links, every write clipped to the frame's w x h;
 *   compose   a thread a screen pixel walks the frames in order with the canvas state and the disposal-3 backup in registers.
 * No workgroup waits for another.  rhccq_gif_frame.first_row and rhccq_gif_info.seg_rows size the segment table from the file alone: a
 * frame of B stream bytes has at most 8 B / (2 (m + 1)) + 1 segments that are not empty (a data code and the code that closes it), 16 bytes
 * a row.
 * Device forms: every pointer but info and `frames` is device memory; async on the context stream, no host synchronisation, nothing
 * allocated.  frames_dev is a copy of `frames`; every kernel tests the offsets it takes from it against the buffers' sizes again.
 * RHCCQ_E_ARG: a null pointer, a negative size, tables not aligned to 8, a workspace not aligned to 256, streams not aligned to 16, status
 * or counts not aligned to 4 / 8, a frame table that does not fit the sizes given.  The file itself may start at any byte: it is read
 * byte by byte.  RHCCQ_E_LIMIT: n_frames above
 * 2^20 or a size of 2^31 or more.
 * Host forms (serial, no GPU, host memory): the same step functions of csrc/gif_read.h. */
#define RHCCQ_GIFR_OK 0
#define RHCCQ_GIFR_BAD_SIGNATURE 1
#define RHCCQ_GIFR_TRUNCATED 2
#define RHCCQ_GIFR_BAD_BLOCK 3
#define RHCCQ_GIFR_BAD_HEADER 4
#define RHCCQ_GIFR_BAD_FRAME 5
#define RHCCQ_GIFR_NO_TABLE 6
#define RHCCQ_GIFR_NO_FRAMES 7
#define RHCCQ_GIFR_LIMIT 8
#define RHCCQ_GIFR_BAD_CODE 9
#define RHCCQ_GIFR_BAD_LENGTH 10
typedef struct rhccq_gif_info {
  int32_t status, detail;                 /* RHCCQ_GIFR_OK .. RHCCQ_GIFR_LIMIT */
  int32_t width, height;                  /* the logical screen */
  int32_t global_rows, loop;              /* rows of the global table (0: none); the loop count, -1 where the file has none */
  int32_t n_frames, n_blocks;             /* images; data sub-blocks of all images */
  int64_t global_offset;                  /* of the global table in the file, -1 without */
  int64_t stream_bytes;                   /* the joined streams: every frame's at a 16-byte aligned offset, 16 bytes or more between two */
  int64_t pixels;                         /* the sum of w x h over the frames */
  int64_t seg_rows;                       /* rows of the segment table */
} rhccq_gif_info;
typedef struct rhccq_gif_frame {
  int32_t x, y, w, h;
  int32_t m, interlace;
  int32_t table_rows, transparent;        /* rows of the frame's table; the transparent index, -1 without */
  int32_t disposal, delay;                /* 0..7; centiseconds */
  int32_t first_block, n_blocks;          /* its rows of the sub-block table */
  int64_t table_offset;                   /* of the frame's colour table in the file */
  int64_t stream_offset, stream_bytes;    /* its code stream in the joined streams */
  int64_t pixel_offset;                   /* the sum of w x h over the frames in front */
  int64_t first_row;                      /* its rows of the segment table: first_row .. the next frame's (seg_rows behind the last) */
} rhccq_gif_frame;
/* host only.  blocks: one rhccq_segment a data sub-block (offset of its first data byte, length, first_piece = its frame, dst = the byte's
   place in the joined streams).  frames / blocks receive the first frames_cap / blocks_cap rows (may be NULL with 0), *n_frames / *n_blocks
   the full numbers.  RHCCQ_E_ARG for a null file (with n > 0), info or counter, or a negative size; else RHCCQ_OK with info->status set */
int rhccq_gif_parse_host(const uint8_t* file, int64_t n, rhccq_gif_info* info, rhccq_gif_frame* frames, int64_t frames_cap, int64_t* n_frames,
                         rhccq_segment* blocks, int64_t blocks_cap, int64_t* n_blocks);
int32_t rhccq_gif_read_tile(void);        /* codes a step of the lengths and the emit launches (a lane a code) */
int32_t rhccq_gif_read_scan_step(void);   /* codes a step of the scan launch: a whole number of tiles, a lane one code of each */
int32_t rhccq_gif_read_threads(void);     /* threads of all three launches' workgroups; the segments a step of a frame's prefix sums takes */
/* host only: rhccq_gif_decode's workspace for a parsed file of n bytes; rhccq_gif_unlzw's for a frame table alone */
int rhccq_gif_read_sizes(const rhccq_gif_info* info, int64_t n, int64_t* workspace_bytes);
int64_t rhccq_gif_unlzw_bytes(const rhccq_gif_frame* frames, int32_t n_frames);   /* negative for bad arguments */
/* the join alone: blocks_dev holds the n_blocks rows (dst ascending), streams (aligned to 16) receives `total` bytes (a multiple of 16),
   zero where no sub-block lies */
int rhccq_gif_join(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_segment* blocks_dev, int64_t n_blocks, int64_t total, uint8_t* streams);
/* streams: stream_bytes joined bytes as the parser lays them out -> pixels: frame f's strings in stream order (not yet de-interlaced) from
   pixels + frames[f].pixel_offset, n_pixels bytes in all.  counts (device int64[n_frames]): the pixels every frame's stream holds; the
   device form adds segment totals that saturate at 2^32 - 1 each, more than any frame has, so such a count is only a lower bound.
   status: device int32[2].  Afterwards the workspace holds uint32[4] at its start: the lowest frame with a bad code, the lowest with a
   bad length (2^32 - 1: none), the segments of all frames, 0 */
int rhccq_gif_unlzw(rhccq_ctx* ctx, const uint8_t* streams, int64_t stream_bytes, const rhccq_gif_frame* frames, const rhccq_gif_frame* frames_dev,
                    int32_t n_frames, void* workspace, uint8_t* pixels, int64_t n_pixels, int64_t* counts, int32_t* status);
/* pixels as rhccq_gif_unlzw leaves them; the colour tables are read from the file -> rgb[F][H][W][3], alpha[F][H][W] (may be NULL), idx:
   frame f's de-interlaced indices h x w from idx + frames[f].pixel_offset (may be NULL) */
int rhccq_gif_compose(rhccq_ctx* ctx, const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames_dev,
                      int32_t n_frames, int32_t H, int32_t W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx);
/* the whole read: join, rhccq_gif_unlzw, rhccq_gif_compose.  info, frames and the blocks are rhccq_gif_parse_host's; with info->status set
   nothing runs but the launch that writes it to status.  Afterwards the workspace starts as rhccq_gif_unlzw's does */
int rhccq_gif_decode(rhccq_ctx* ctx, const uint8_t* file, int64_t n, const rhccq_gif_info* info, const rhccq_gif_frame* frames,
                     const rhccq_gif_frame* frames_dev, const rhccq_segment* blocks_dev, void* workspace, uint8_t* rgb, uint8_t* alpha, uint8_t* idx,
                     int32_t* status);
int rhccq_gif_unlzw_host(const uint8_t* streams, int64_t stream_bytes, const rhccq_gif_frame* frames, int32_t n_frames, uint8_t* pixels, int64_t n_pixels,
                         int64_t* counts, int32_t* status, int64_t* n_segments);   /* n_segments may be NULL */
int rhccq_gif_compose_host(const uint8_t* pixels, int64_t n_pixels, const uint8_t* file, int64_t n, const rhccq_gif_frame* frames, int32_t n_frames,
                           int32_t H, int32_t W, uint8_t* rgb, uint8_t* alpha, uint8_t* idx);
/* file in host memory; parses it itself; outputs sized by the parse (they may be NULL for a file the parser refuses); status: host int32[2] */
int rhccq_gif_decode_host(const uint8_t* file, int64_t n, uint8_t* rgb, uint8_t* alpha, uint8_t* idx, int32_t* status);

#ifdef __cplusplus
}
#endif
#endif /* RHCCQ_H */
