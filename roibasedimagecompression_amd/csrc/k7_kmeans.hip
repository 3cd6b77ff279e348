// K7: KMeans(n_clusters = k, random_state = 42, n_init = 1, lloyd) used by the reference to split
// oversize colour clusters (encoder/compression/clustering.py:720-775, sklearn 1.7.2 underneath).
//
// Canonical arithmetic "KM64" (see oracle/rhccq_oracle.py): greedy k-means++ on EXACT integer
// squared distances (cumulative sums / potentials are order independent), MT19937 uniforms supplied
// by the host exactly as numpy's RandomState(42) emits them; Lloyd in float64 on mean-centred
// coordinates, E-step distance csq + (-2 * fma-chain dot) exactly as sklearn's dgemm / einsum evaluate it
// (rhccq_common.h; the file is built with -ffp-contract=off, the only fused operations are explicit), centres from exact integer member sums, sklearn's convergence rules.
//
// MI355X design: one 1024-thread workgroup per split problem (problems of a frame are batched in one
// launch, grid = #problems); points, labels, centres and integer accumulators live in LDS
// (<= 10240 points: 40 + 40 + 32 + 16 KB); the k-means++ cumulative-sum search is a block scan +
// per-thread chunk search; candidate potentials are 64-bit integer block reductions.  float64 VALU
// bound (K = 3: not an MFMA shape).
//
// Large problems take the "wide" Lloyd path (RHCCQ_OPT_KMEANS_WIDE_PAIRS, km_wide_host.h): load, mean / tolerance and k-means++ stay in
// kmeans_kernel, which then leaves the initial centres in the problem's `work` slots and returns; the Lloyd iterations run as launches,
// an E-step over tiles of points on many CUs (km_wide_estep_kernel) and an M-step of one workgroup (km_wide_mstep_kernel, the same
// km_mstep code as the one-workgroup loop).  A launch boundary is the only synchronisation between workgroups.
#include <algorithm>
#include <vector>

#include "km_wide_host.h"
#include "rhccq_common.h"
#include "wave_dpp.h"

namespace rhccq {

using KmWideRec = rhccq_km_wide::Record;
using KmWideTile = rhccq_km_wide::Tile;

#include "kpp_flat.h"

constexpr int kKmThreads = 1024;
constexpr int kKmWaves = kKmThreads / 64;
constexpr int kKmCentLds = 1024;   // centres kept in LDS up to this k
constexpr int kTMax = 16;
constexpr int kKmPts = 4;          // points a thread holds in registers per pass of the Lloyd E-step
constexpr int kKmFlatS = 10;       // k-means++ with every point in a register up to this many points per thread (LDS-resident inputs)
static_assert(sizeof(FlatShared) <= sizeof(unsigned) * kKmCentLds * 4, "the register k-means++ borrows the member-sum table");
constexpr int kKmWideTile = 64;    // wide E-step: points of a tile, one per lane: small tiles are what spread a few thousand points over the CUs
constexpr int kKmWideWaves = 4;    // ... and waves of a tile's workgroup, one per SIMD: each walks a quarter of the centres for the tile's points
constexpr int kKmWideThreads = kKmWideTile * kKmWideWaves;

#ifdef RHCCQ_KM_STAMPS   // diagnostic build only (tools/build_dbg.sh, tools/kmstamps.py): where problem 0's thread 0 spends kmeans_kernel, in
__device__ unsigned long long g_km_stamps[8];   // ticks of the 100 MHz wall clock: load, k-means++, E-step, M-step, empty-cluster branch, final labelling
#define KM_STAMP(slot)                                                                      \
  do {                                                                                      \
    const unsigned long long _t = wall_clock64();                                           \
    if (blockIdx.x == 0 && threadIdx.x == 0) g_km_stamps[slot] += _t - _km_last;            \
    _km_last = _t;                                                                          \
  } while (0)
#define KM_STAMP_START() unsigned long long _km_last = wall_clock64()
#define KM_STAMP_PARAM , unsigned long long& _km_last
#define KM_STAMP_ARG , _km_last
#else
#define KM_STAMP(slot) do {} while (0)
#define KM_STAMP_START() do {} while (0)
#define KM_STAMP_PARAM
#define KM_STAMP_ARG
#endif

struct KmShared {
  unsigned long long red64[kKmWaves * kTMax];
  unsigned long long scan_red[kKmWaves + 1];
  double dred[kKmWaves];
  int ired[kKmWaves];
  int cand[kTMax];
  unsigned long long pots[kTMax];
  int flag;
  int best;
  double bestd;
  int besti;
};

__device__ __forceinline__ unsigned long long block_exscan64(unsigned long long v, KmShared& sh, unsigned long long* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  unsigned long long inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    unsigned long long t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  __syncthreads();
  if (lane == 63) sh.scan_red[w] = inc;
  __syncthreads();
  unsigned long long base = 0, tot = 0;
  for (int i = 0; i < kKmWaves; ++i) {
    if (i < w) base += sh.scan_red[i];
    tot += sh.scan_red[i];
  }
  *total = tot;
  return base + inc - v;
}

// KM64 distance: csq + (-2 * fma(x2, c2, fma(x1, c1, x0*c0)))   (rhccq_common.h)
__device__ __forceinline__ double km64_dist(double x0, double x1, double x2, const double* c) {
  return c[3] + (-2.0 * km64_dot(x0, x1, x2, c[0], c[1], c[2]));
}

// lane `l` (a compile-time constant at the call) of a wave's double
__device__ __forceinline__ double km_readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// The nearest centre of kPts points a thread holds in registers, centres in the OUTER loop: every centre is read once for all of
// them (the first version walked the centres once per point: with all threads reading the same centre the LDS broadcast reads, two
// b128 per pair, were the whole iteration).  Centres are visited in ascending order and compared by strict <: the first arg-min
// (bj, with its distance bd; INFINITY and 0 for k = 0).  With one point per thread a pair is one chain of dependent float64
// operations and a wave alone on its SIMD has nothing to fill their latencies with: four centres are then in flight at a time
// (the distances of four centres side by side, the comparisons still one after the other in ascending order).
template <int kPts>
__device__ __forceinline__ void km_nearest(const double* C, int k, const double (&x0)[kPts], const double (&x1)[kPts], const double (&x2)[kPts],
                                           int (&bj)[kPts], double (&bd)[kPts]) {
#pragma unroll
  for (int q = 0; q < kPts; ++q) { bd[q] = INFINITY; bj[q] = 0; }
  int j = 0;
  if (kPts == 1) {
    for (; j + 4 <= k; j += 4) {
      double d[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const double* c = C + 4 * (j + u);
        d[u] = c[3] + (-2.0 * km64_dot(x0[0], x1[0], x2[0], c[0], c[1], c[2]));
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (d[u] < bd[0]) { bd[0] = d[u]; bj[0] = j + u; }
    }
  }
  for (; j < k; ++j) {
    const double c0 = C[4 * j], c1 = C[4 * j + 1], c2 = C[4 * j + 2], cs = C[4 * j + 3];
#pragma unroll
    for (int q = 0; q < kPts; ++q) {
      const double d = cs + (-2.0 * km64_dot(x0[q], x1[q], x2[q], c0, c1, c2));
      if (d < bd[q]) { bd[q] = d; bj[q] = j; }
    }
  }
}

// What follows the E-step in a Lloyd iteration, by one 1024-thread workgroup: the empty-cluster branch, the new centres and the stop
// rules.  P: packed colours; aux: the labels of this E-step (bit 31 = "taken" during relocation); C [k][4] = x, y, z, csq; S [k][4] =
// sum r, g, b, count; shift: [k] doubles of scratch.  Returns 0 = go on, 1 = the labels did not change (strict stop), 2 = the shifts
// are within the tolerance.  The one-workgroup loop of kmeans_kernel and km_wide_mstep_kernel share it.
__device__ __forceinline__ int km_mstep(const uint32_t* P, uint32_t* aux, double* C, unsigned* S, double* shift, const int n, const int k, const double m0,
                                        const double m1, const double m2, const double tol, const int any_changed, int& relocated, KmShared& sh KM_STAMP_PARAM) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // empty clusters (sklearn _relocate_empty_clusters_dense)
  int n_empty = 0;
  for (int j = tid; j < k; j += kKmThreads) n_empty += S[j * 4 + 3] == 0u;
  n_empty = block_sum<int>(n_empty, sh.ired);
  KM_STAMP(3);
  if (n_empty > 0) {
    // only the clusters that were empty BEFORE any relocation are refilled (oracle: `empty` is
    // computed once); mark them so that clusters emptied by a relocation are not picked up
    for (int j = tid; j < k; j += kKmThreads)
      if (S[j * 4 + 3] == 0u) S[j * 4 + 2] = 0xffffffffu;
    __syncthreads();
    for (int e = 0, done = 0; e < k && done < n_empty; ++e) {
      if (!(S[e * 4 + 3] == 0u && S[e * 4 + 2] == 0xffffffffu)) { continue; }
      // farthest not-yet-taken point from its own (old) centre: (distance desc, index asc)
      double bd = -1.0;
      int bi = 0x7fffffff;
      for (int i = tid; i < n; i += kKmThreads) {
        const uint32_t l = aux[i];
        if (l & 0x80000000u) continue;
        const uint32_t kk = P[i];
        const double* cc = C + 4 * l;
        const double d0 = ((double)key_r(kk) - m0) - cc[0], d1 = ((double)key_g(kk) - m1) - cc[1], d2 = ((double)key_b(kk) - m2) - cc[2];
        const double d = (d0 * d0 + d1 * d1) + d2 * d2;
        if (d > bd || (d == bd && i < bi)) { bd = d; bi = i; }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_down(bd, o, 64);
        const int oi = __shfl_down(bi, o, 64);
        if (od > bd || (od == bd && oi < bi)) { bd = od; bi = oi; }
      }
      __syncthreads();
      if (lane == 0) { sh.dred[wave] = bd; sh.ired[wave] = bi; }
      __syncthreads();
      if (tid == 0) {
        double gd = sh.dred[0];
        int gi = sh.ired[0];
        for (int w = 1; w < kKmWaves; ++w)
          if (sh.dred[w] > gd || (sh.dred[w] == gd && sh.ired[w] < gi)) { gd = sh.dred[w]; gi = sh.ired[w]; }
        sh.bestd = gd; sh.besti = gi;
      }
      __syncthreads();
      if (done == 0 && !(sh.bestd > 0.0)) break;       // dist.max() == 0: nothing to relocate
      if (tid == 0) {
        const int f = sh.besti;
        const uint32_t old = aux[f] & 0x7fffffffu;
        const uint32_t kk = P[f];
        S[old * 4 + 0] -= key_r(kk); S[old * 4 + 1] -= key_g(kk); S[old * 4 + 2] -= key_b(kk); S[old * 4 + 3] -= 1u;
        S[e * 4 + 0] = key_r(kk); S[e * 4 + 1] = key_g(kk); S[e * 4 + 2] = key_b(kk); S[e * 4 + 3] = 1u;
        aux[f] |= 0x80000000u;
      }
      ++done; ++relocated;
      __syncthreads();
    }
    for (int i = tid; i < n; i += kKmThreads) aux[i] &= 0x7fffffffu;
    for (int j = tid; j < k; j += kKmThreads)
      if (S[j * 4 + 3] == 0u) S[j * 4 + 2] = 0u;
    __syncthreads();
  }
  // new centres, per-centre squared shift kept in the csq slot of a scratch copy
  // heaviest cluster (first arg-max of the counts) for still-empty clusters
  int hv = 0;
  if (n_empty > 0) {
    unsigned bc = 0; int bj = 0x7fffffff;
    for (int j = tid; j < k; j += kKmThreads) {
      const unsigned cnt = S[j * 4 + 3];
      if (cnt > bc || (cnt == bc && j < bj)) { bc = cnt; bj = j; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned oc = __shfl_down(bc, o, 64);
      const int oj = __shfl_down(bj, o, 64);
      if (oc > bc || (oc == bc && oj < bj)) { bc = oc; bj = oj; }
    }
    __syncthreads();
    if (lane == 0) { sh.scan_red[wave] = bc; sh.ired[wave] = bj; }
    __syncthreads();
    if (tid == 0) {
      unsigned long long gc = sh.scan_red[0]; int gj = sh.ired[0];
      for (int w = 1; w < kKmWaves; ++w)
        if (sh.scan_red[w] > gc || (sh.scan_red[w] == gc && sh.ired[w] < gj)) { gc = sh.scan_red[w]; gj = sh.ired[w]; }
      sh.best = gj;
    }
    __syncthreads();
    hv = sh.best;
  }
  double hx = 0, hy = 0, hz = 0;
  if (n_empty > 0) {
    const unsigned cnt = S[hv * 4 + 3];
    hx = (double)S[hv * 4 + 0] / (double)cnt - m0;
    hy = (double)S[hv * 4 + 1] / (double)cnt - m1;
    hz = (double)S[hv * 4 + 2] / (double)cnt - m2;
  }
  KM_STAMP(4);
  __syncthreads();
  for (int j = tid; j < k; j += kKmThreads) {
    const unsigned cnt = S[j * 4 + 3];
    double c0, c1, c2;
    if (cnt > 0) {
      c0 = (double)S[j * 4 + 0] / (double)cnt - m0;
      c1 = (double)S[j * 4 + 1] / (double)cnt - m1;
      c2 = (double)S[j * 4 + 2] / (double)cnt - m2;
    } else { c0 = hx; c1 = hy; c2 = hz; }
    const double d0 = c0 - C[j * 4 + 0], d1 = c1 - C[j * 4 + 1], d2 = c2 - C[j * 4 + 2];
    shift[j] = (d0 * d0 + d1 * d1) + d2 * d2;
    C[j * 4 + 0] = c0; C[j * 4 + 1] = c1; C[j * 4 + 2] = c2;
    C[j * 4 + 3] = km64_csq(c0, c1, c2);
  }
  __threadfence_block();
  __syncthreads();
  if (!any_changed) return 1;
  if (wave == 0) {
    // sum of the shifts in index order, as the oracle adds them: the wave loads 64 at a time (one coalesced
    // access instead of k dependent ones by a single thread) and folds them through readlane, left to right.
    // The lane is a constant of the unrolled loop: v_readlane_b32 with an immediate lane, not the ds_bpermute pair per
    // element that __shfl with a loop variable compiles to (~17 us of a 20 us M-step at k = 389: a dependent LDS round
    // trip per centre), and no branch per element either: the lanes behind the last centre hold + 0.0, and tot + 0.0 == tot
    // bit for bit, because tot is never - 0.0 (it starts as + 0.0 and every shift is a sum of squares)
    double tot = 0.0;
    for (int j0 = 0; j0 < k; j0 += 64) {
      const double v = j0 + lane < k ? shift[j0 + lane] : 0.0;
#pragma unroll
      for (int l = 0; l < 64; ++l) tot = tot + km_readlane(v, l);
    }
    if (lane == 0) sh.flag = tot <= tol;
  }
  __syncthreads();
  const int stop = sh.flag;
  __syncthreads();
  return stop ? 2 : 0;
}

__global__ __launch_bounds__(kKmThreads) void kmeans_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ desc,
                                                             const int64_t* __restrict__ koff, const double* __restrict__ rand,
                                                             double* __restrict__ work, int32_t* __restrict__ labels_out,
                                                             int32_t* __restrict__ info, uint32_t* __restrict__ gpts, int gstride,
                                                             int max_iter, const int32_t* __restrict__ wide_of, KmWideRec* __restrict__ recs) {
  __shared__ uint32_t s_keys[RHCCQ_KM_LDS_MAX];
  __shared__ uint32_t s_aux[RHCCQ_KM_LDS_MAX];
  __shared__ double s_cent[kKmCentLds * 4];
  __shared__ __align__(16) unsigned s_sum[kKmCentLds * 4];
  __shared__ KmShared sh;

  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int off = desc[p * 6 + 0], n = desc[p * 6 + 1], k = desc[p * 6 + 2], rand_off = desc[p * 6 + 3];
  const int first = desc[p * 6 + 4], T = desc[p * 6 + 5];
  int32_t* lab_out = labels_out + off;
  if (n <= 0 || k <= 0) return;
  const int wide = wide_of ? wide_of[p] : -1;          // >= 0: the problem's record of the wide Lloyd path (km_wide_host.h)
  KM_STAMP_START();

  uint32_t* P;      // packed colours
  uint32_t* aux;    // closest (k-means++) then labels (Lloyd); bit 31 = "taken" during relocation
  if (n <= RHCCQ_KM_LDS_MAX) { P = s_keys; aux = s_aux; }
  else { P = gpts + (size_t)p * 2 * gstride; aux = P + gstride; }
  double* wk = work + 8 * koff[p];
  double* C;        // [k][4] = x, y, z, csq
  unsigned* S;      // [k][4] = sum r, g, b, count
  if (k <= kKmCentLds) { C = s_cent; S = s_sum; }
  else { C = wk; S = reinterpret_cast<unsigned*>(wk + 4 * (size_t)k); }
  int* chosen = reinterpret_cast<int*>(wk + 6 * (size_t)k);   // [k] init indices (global, small)

  // ---- load, mean, tolerance ----------------------------------------------------------------
  unsigned long long sr = 0, sg = 0, sb = 0, qr = 0, qg = 0, qb = 0;
  for (int i = tid; i < n; i += kKmThreads) {
    const uint32_t kk = keys[off + i];
    P[i] = kk;
    const unsigned r = key_r(kk), g = key_g(kk), b = key_b(kk);
    sr += r; sg += g; sb += b;
    qr += r * r; qg += g * g; qb += b * b;
  }
  sr = block_sum<unsigned long long>(sr, sh.red64);
  sg = block_sum<unsigned long long>(sg, sh.red64);
  sb = block_sum<unsigned long long>(sb, sh.red64);
  qr = block_sum<unsigned long long>(qr, sh.red64);
  qg = block_sum<unsigned long long>(qg, sh.red64);
  qb = block_sum<unsigned long long>(qb, sh.red64);
  const double dn = (double)n;
  const double m0 = (double)sr / dn, m1 = (double)sg / dn, m2 = (double)sb / dn;
  const double v0 = (double)((long long)((unsigned long long)n * qr - sr * sr)) / (dn * dn);
  const double v1 = (double)((long long)((unsigned long long)n * qg - sg * sg)) / (dn * dn);
  const double v2 = (double)((long long)((unsigned long long)n * qb - sb * sb)) / (dn * dn);
  const double tol = ((v0 + v1) + v2) / 3.0 * 1e-4;
  KM_STAMP(0);

  // ---- k-means++ in exact integers ----------------------------------------------------------
  // (up to 10 points per thread: every point in a register, two barriers per pick -- kpp_flat.h; the loop below, a block scan, a
  // candidate search and a block reduction per pick, ~7 us each, serves larger inputs)
  if (n <= 16 * 64 * 4) {
    __syncthreads();      // (small inputs -- the one large split of a 4K frame's level 3 has 3 900 colours: four working waves, see kpp_flat.h)
    kpp_flat<16, 4>([&](int i) { return P[i]; }, n, k, T, first, rand + rand_off, chosen, *reinterpret_cast<FlatShared*>(s_sum));
  } else if (n <= kKmFlatS * kKmThreads) {
    __syncthreads();
    kpp_flat<kKmFlatS, kKmWaves>([&](int i) { return P[i]; }, n, k, T, first, rand + rand_off, chosen, *reinterpret_cast<FlatShared*>(s_sum));
  } else {
    const int per = (n + kKmThreads - 1) / kKmThreads;
    const int lo = min(tid * per, n), hi = min(lo + per, n);
    unsigned long long pot;
    {
      const uint32_t kf = P[first];
      unsigned long long s = 0;
      for (int i = tid; i < n; i += kKmThreads) {
        const unsigned d = (unsigned)dist2_keys(P[i], kf);
        aux[i] = d;
        s += d;
      }
      pot = block_sum<unsigned long long>(s, sh.red64);
      if (tid == 0) chosen[0] = first;
    }
    for (int c = 1; c < k; ++c) {
      const double* u = rand + rand_off + (size_t)(c - 1) * T;
      const double dpot = (double)pot;
      // cumulative-sum search (np.searchsorted(cumsum(closest), u*pot, 'left'), clipped to n-1)
      unsigned long long loc = 0;
      for (int i = lo; i < hi; ++i) loc += aux[i];
      unsigned long long tot;
      const unsigned long long base = block_exscan64(loc, sh, &tot);
      if (tid < T) sh.cand[tid] = (u[tid] * dpot <= 0.0) ? 0 : n - 1;
      __syncthreads();
      if (loc > 0) {
        for (int t = 0; t < T; ++t) {
          const double r = u[t] * dpot;
          if ((double)base < r && r <= (double)(base + loc)) {
            unsigned long long cum = base;
            int i = lo;
            for (; i < hi; ++i) {
              cum += aux[i];
              if ((double)cum >= r) break;
            }
            sh.cand[t] = i < hi ? i : hi - 1;
          }
        }
      }
      __syncthreads();
      // potentials of the T candidates
      uint32_t ck[kTMax];
      unsigned long long acc[kTMax];
  #pragma unroll
      for (int t = 0; t < kTMax; ++t) { acc[t] = 0; ck[t] = t < T ? P[sh.cand[t]] : 0u; }
      for (int i = tid; i < n; i += kKmThreads) {
        const uint32_t ki = P[i];
        const unsigned cl = aux[i];
  #pragma unroll
        for (int t = 0; t < kTMax; ++t)
          if (t < T) acc[t] += min(cl, (unsigned)dist2_keys(ki, ck[t]));
      }
  #pragma unroll
      for (int t = 0; t < kTMax; ++t) {
        if (t < T) {
          const unsigned long long w = wave_sum(acc[t]);
          if (lane == 0) sh.red64[t * kKmWaves + wave] = w;
        }
      }
      __syncthreads();
      if (tid < T) {
        unsigned long long s = 0;
        for (int w = 0; w < kKmWaves; ++w) s += sh.red64[tid * kKmWaves + w];
        sh.pots[tid] = s;
      }
      __syncthreads();
      int best = 0;
      unsigned long long bp = sh.pots[0];
      for (int t = 1; t < T; ++t)
        if (sh.pots[t] < bp) { bp = sh.pots[t]; best = t; }
      pot = bp;
      const int bi = sh.cand[best];
      const uint32_t kb = P[bi];
      for (int i = tid; i < n; i += kKmThreads) aux[i] = min(aux[i], (unsigned)dist2_keys(P[i], kb));
      if (tid == 0) chosen[c] = bi;
      __syncthreads();
    }
  }
  __threadfence_block();
  __syncthreads();

  KM_STAMP(1);

  // ---- Lloyd --------------------------------------------------------------------------------
  if (wide >= 0) { C = wk; S = reinterpret_cast<unsigned*>(wk + 4 * (size_t)k); }   // the launches of the wide path find them there
  for (int j = tid; j < k; j += kKmThreads) {
    const uint32_t kk = P[chosen[j]];
    const double c0 = (double)key_r(kk) - m0, c1 = (double)key_g(kk) - m1, c2 = (double)key_b(kk) - m2;
    C[j * 4 + 0] = c0; C[j * 4 + 1] = c1; C[j * 4 + 2] = c2;
    C[j * 4 + 3] = km64_csq(c0, c1, c2);
  }
  if (wide >= 0) {
    // the wide path goes on from here (rhccq_kmeans): cleared sums, labels_old = -1 in the output itself, and the problem's record
    for (int j = tid; j < 4 * k; j += kKmThreads) S[j] = 0;
    for (int i = tid; i < n; i += kKmThreads) lab_out[i] = 0x7fffffff;
    if (tid == 0) {
      KmWideRec r = {};
      r.m0 = m0; r.m1 = m1; r.m2 = m2; r.tol = tol;
      r.state = rhccq_km_wide::kRunning;
      recs[wide] = r;
      info[p * 4 + 0] = 0; info[p * 4 + 1] = 0; info[p * 4 + 2] = 0; info[p * 4 + 3] = 1;
    }
    return;
  }
  for (int i = tid; i < n; i += kKmThreads) aux[i] = 0x7fffffffu;   // labels_old = -1
  __syncthreads();
  double* shift = wk + 7 * (size_t)k;                   // [k] doubles of scratch (global)
  int n_iter = 0, strict = 0, relocated = 0;
  for (int it = 0; it < max_iter; ++it) {
    n_iter = it + 1;
    for (int j = tid; j < 4 * k; j += kKmThreads) S[j] = 0;
    if (tid == 0) sh.flag = 0;
    __syncthreads();
    int changed = 0;
    // E-step: a thread keeps up to kKmPts of its points in registers (km_nearest)
    for (int i0 = tid; i0 < n; i0 += kKmThreads * kKmPts) {
      double x0[kKmPts], x1[kKmPts], x2[kKmPts];
      int bj[kKmPts];
      double bd[kKmPts];
      uint32_t kk[kKmPts];
#pragma unroll
      for (int q = 0; q < kKmPts; ++q) {
        const int i = i0 + q * kKmThreads;
        kk[q] = i < n ? P[i] : 0u;
        x0[q] = (double)key_r(kk[q]) - m0; x1[q] = (double)key_g(kk[q]) - m1; x2[q] = (double)key_b(kk[q]) - m2;
      }
      km_nearest<kKmPts>(C, k, x0, x1, x2, bj, bd);
#pragma unroll
      for (int q = 0; q < kKmPts; ++q) {
        const int i = i0 + q * kKmThreads;
        if (i >= n) continue;
        if ((uint32_t)bj[q] != aux[i]) changed = 1;
        aux[i] = (uint32_t)bj[q];
        atomicAdd(&S[bj[q] * 4 + 0], key_r(kk[q]));
        atomicAdd(&S[bj[q] * 4 + 1], key_g(kk[q]));
        atomicAdd(&S[bj[q] * 4 + 2], key_b(kk[q]));
        atomicAdd(&S[bj[q] * 4 + 3], 1u);
      }
    }
    if (changed) sh.flag = 1;                           // benign race: all writers store 1
    __syncthreads();
    const int any_changed = sh.flag;
    KM_STAMP(2);
    const int stop = km_mstep(P, aux, C, S, shift, n, k, m0, m1, m2, tol, any_changed, relocated, sh KM_STAMP_ARG);
    KM_STAMP(3);
    if (stop == 1) { strict = 1; break; }
    if (stop) break;
  }
  if (!strict) {
    // the final labelling, by the same centre-outer tiles as the E-step
    for (int i0 = tid; i0 < n; i0 += kKmThreads * kKmPts) {
      double x0[kKmPts], x1[kKmPts], x2[kKmPts];
      int bj[kKmPts];
      double bd[kKmPts];
#pragma unroll
      for (int q = 0; q < kKmPts; ++q) {
        const int i = i0 + q * kKmThreads;
        const uint32_t kk = i < n ? P[i] : 0u;
        x0[q] = (double)key_r(kk) - m0; x1[q] = (double)key_g(kk) - m1; x2[q] = (double)key_b(kk) - m2;
      }
      km_nearest<kKmPts>(C, k, x0, x1, x2, bj, bd);
#pragma unroll
      for (int q = 0; q < kKmPts; ++q) {
        const int i = i0 + q * kKmThreads;
        if (i < n) aux[i] = (uint32_t)bj[q];
      }
    }
    __syncthreads();
  }
  KM_STAMP(5);
  for (int i = tid; i < n; i += kKmThreads) lab_out[i] = (int32_t)aux[i];
  if (tid == 0) {
    info[p * 4 + 0] = n_iter; info[p * 4 + 1] = strict; info[p * 4 + 2] = relocated; info[p * 4 + 3] = 0;
  }
}

// ---- the wide Lloyd path: one iteration = an E-step launch and an M-step launch (km_wide_host.h) ------------------------------------
// E-step: a workgroup of kKmWideWaves waves per tile of 64 points of one wide problem.  It copies the problem's centres into LDS
// (k <= kKmCentLds).  Every wave keeps the tile's points in registers, a point per lane, and walks ITS contiguous share of the
// centres in ascending order with the per-pair expression of the one-workgroup E-step (km_nearest); wave 0 then takes, per point, the
// shares' results in ascending order by strict <, which is the first arg-min over all centres.  The labels live in labels_out, which
// also holds the previous ones (0x7fffffff at first); the integer member sums go to the problem's `work` slots by two packed 64-bit
// atomics per point (r | g << 32, b | count << 32: the four 32-bit fields of a cluster, none of which can carry, 255 x 2^24 < 2^32)
// and are exact in any order.  In state kFinalPending only the labels are written.
__global__ __launch_bounds__(kKmWideThreads) void km_wide_estep_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ desc,
                                                                        const int64_t* __restrict__ koff, double* __restrict__ work,
                                                                        int32_t* __restrict__ labels_out, const KmWideTile* __restrict__ tiles,
                                                                        KmWideRec* __restrict__ recs) {
  extern __shared__ double s_wcent[];                   // [k][4] of the launch's largest k
  __shared__ double s_bd[kKmWideWaves][kKmWideTile];
  __shared__ int s_bj[kKmWideWaves][kKmWideTile];
  const KmWideTile t = tiles[blockIdx.x];
  KmWideRec* rec = recs + t.rec;
  const int state = rec->state;
  if (state == rhccq_km_wide::kDone) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = t.prob;
  const int off = desc[p * 6 + 0], n = desc[p * 6 + 1], k = desc[p * 6 + 2];
  double* wk = work + 8 * koff[p];
  const double m0 = rec->m0, m1 = rec->m1, m2 = rec->m2;
  for (int j = tid; j < 4 * k; j += kKmWideThreads) s_wcent[j] = wk[j];
  __syncthreads();
  const int i = t.first + lane;
  const uint32_t kk = i < n ? keys[off + i] : 0u;
  const double x0[1] = {(double)key_r(kk) - m0}, x1[1] = {(double)key_g(kk) - m1}, x2[1] = {(double)key_b(kk) - m2};
  const int share = (k + kKmWideWaves - 1) / kKmWideWaves, j0 = min(k, wave * share), j1 = min(k, j0 + share);
  int bj[1];
  double bd[1];
  km_nearest<1>(s_wcent + 4 * j0, j1 - j0, x0, x1, x2, bj, bd);
  s_bd[wave][lane] = bd[0];
  s_bj[wave][lane] = j0 + bj[0];
  __syncthreads();
  if (wave != 0 || i >= n) return;
  double d = s_bd[0][lane];
  int b = s_bj[0][lane];
#pragma unroll
  for (int w = 1; w < kKmWideWaves; ++w)
    if (s_bd[w][lane] < d) { d = s_bd[w][lane]; b = s_bj[w][lane]; }
  int32_t* lab = labels_out + off;
  if (state == rhccq_km_wide::kFinalPending) { lab[i] = b; return; }
  if (b != lab[i]) rec->changed = 1;                    // benign race: all writers store 1
  lab[i] = b;
  unsigned long long* S = reinterpret_cast<unsigned long long*>(wk + 4 * (size_t)k);
  atomicAdd(&S[b * 2 + 0], (unsigned long long)key_r(kk) | ((unsigned long long)key_g(kk) << 32));
  atomicAdd(&S[b * 2 + 1], (unsigned long long)key_b(kk) | (1ull << 32));
}

// M-step: one workgroup per wide problem; km_mstep on the centres and sums in the problem's `work` slots, the points read from the
// input and the labels in labels_out.  It counts the iteration, applies the stop rules and the iteration limit to the problem's
// record, writes `info` when the problem ends, and clears the sums and the "changed" word for the next E-step.
__global__ __launch_bounds__(kKmThreads) void km_wide_mstep_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ desc,
                                                                    const int64_t* __restrict__ koff, double* __restrict__ work,
                                                                    int32_t* __restrict__ labels_out, int32_t* __restrict__ info,
                                                                    const int32_t* __restrict__ wide_list, KmWideRec* __restrict__ recs, int max_iter) {
  __shared__ KmShared sh;
  KmWideRec* rec = recs + blockIdx.x;
  const int tid = threadIdx.x, p = wide_list[blockIdx.x];
  const int state = rec->state;
  if (state == rhccq_km_wide::kDone) return;
  if (state == rhccq_km_wide::kFinalPending) {          // the E-step launch before this one wrote the final labels
    if (tid == 0) rec->state = rhccq_km_wide::kDone;
    return;
  }
  KM_STAMP_START();
  const int off = desc[p * 6 + 0], n = desc[p * 6 + 1], k = desc[p * 6 + 2];
  double* wk = work + 8 * koff[p];
  unsigned* S = reinterpret_cast<unsigned*>(wk + 4 * (size_t)k);
  const int any_changed = rec->changed;
  int relocated = rec->relocated;
  const int n_iter = rec->n_iter + 1;
  const int stop = km_mstep(keys + off, reinterpret_cast<uint32_t*>(labels_out + off), wk, S, wk + 7 * (size_t)k, n, k, rec->m0, rec->m1, rec->m2, rec->tol,
                            any_changed, relocated, sh KM_STAMP_ARG);
  for (int j = tid; j < 4 * k; j += kKmThreads) S[j] = 0;
  if (tid == 0) {
    const int strict = stop == 1;
    int next = rhccq_km_wide::kRunning;
    if (strict) next = rhccq_km_wide::kDone;
    else if (stop || n_iter >= max_iter) next = rhccq_km_wide::kFinalPending;
    rec->changed = 0;
    rec->n_iter = n_iter; rec->strict = strict; rec->relocated = relocated;
    rec->state = next;
    if (next != rhccq_km_wide::kRunning) {
      info[p * 4 + 0] = n_iter; info[p * 4 + 1] = strict; info[p * 4 + 2] = relocated; info[p * 4 + 3] = 1;
    }
  }
}

// ---- K2: integer sums per label -> floor mean ---------------------------------------------------
__global__ __launch_bounds__(256) void cluster_sums_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ labels, int64_t n,
                                                           unsigned long long* __restrict__ sums) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int32_t l = labels[i];
    if (l < 0) continue;
    const uint32_t kk = keys[i];
    atomicAdd(&sums[(size_t)l * 4 + 0], (unsigned long long)key_r(kk));
    atomicAdd(&sums[(size_t)l * 4 + 1], (unsigned long long)key_g(kk));
    atomicAdd(&sums[(size_t)l * 4 + 2], (unsigned long long)key_b(kk));
    atomicAdd(&sums[(size_t)l * 4 + 3], 1ull);
  }
}

// The same sums for up to 2^24 points (a palette: 255 x 2^24 < 2^32, so two 32-bit fields share one 64-bit word without carries):
// (r | g) and (b | count) = TWO atomics per flush instead of four, and a thread walks 8 consecutive points and flushes only when
// the label changes -- a palette is sorted by colour and clusters are compact, so neighbours mostly share their label.  The
// scattered 64-bit atomics execute at the memory side: 12 M of them were 1 ms between level 1 and level 2 of a 4K frame.
// cluster_unpack_kernel then spreads the two words of every label over the four documented fields, in place.
constexpr int kSumRun = 8;
__global__ __launch_bounds__(256) void cluster_sums_packed_kernel(const uint32_t* __restrict__ keys, const int32_t* __restrict__ labels, int64_t n,
                                                                  unsigned long long* __restrict__ sums) {
  const int64_t chunks = (n + kSumRun - 1) / kSumRun;
  for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i0 = c * kSumRun;
    int32_t lab[kSumRun];
    uint32_t kk[kSumRun];
#pragma unroll
    for (int q = 0; q < kSumRun; ++q) {
      const int64_t i = min(i0 + q, n - 1);
      lab[q] = i0 + q < n ? labels[i] : -1;
      kk[q] = keys[i];
    }
    int32_t cur = -1;
    unsigned long long w0 = 0, w1 = 0;
#pragma unroll
    for (int q = 0; q < kSumRun; ++q) {
      if (lab[q] != cur) {
        if (cur >= 0) { atomicAdd(&sums[(size_t)cur * 4 + 0], w0); atomicAdd(&sums[(size_t)cur * 4 + 1], w1); }
        cur = lab[q]; w0 = 0; w1 = 0;
      }
      w0 += ((unsigned long long)key_r(kk[q]) << 32) | key_g(kk[q]);
      w1 += ((unsigned long long)key_b(kk[q]) << 32) | 1ull;
    }
    if (cur >= 0) { atomicAdd(&sums[(size_t)cur * 4 + 0], w0); atomicAdd(&sums[(size_t)cur * 4 + 1], w1); }
  }
}

__global__ void cluster_unpack_kernel(unsigned long long* __restrict__ sums, int64_t k) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const unsigned long long w0 = sums[j * 4 + 0], w1 = sums[j * 4 + 1];
  sums[j * 4 + 0] = w0 >> 32; sums[j * 4 + 1] = w0 & 0xffffffffull;
  sums[j * 4 + 2] = w1 >> 32; sums[j * 4 + 3] = w1 & 0xffffffffull;
}

__global__ void cluster_means_kernel(const unsigned long long* __restrict__ sums, int64_t k, uint32_t* __restrict__ keys_out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= k) return;
  const unsigned long long c = sums[j * 4 + 3];
  uint32_t out = 0;
  if (c) out = ((uint32_t)(sums[j * 4 + 0] / c) << 16) | ((uint32_t)(sums[j * 4 + 1] / c) << 8) | (uint32_t)(sums[j * 4 + 2] / c);
  keys_out[j] = out;
}

}  // namespace rhccq

using namespace rhccq;

extern "C" {

int rhccq_kmeans(rhccq_ctx* ctx, const uint32_t* keys, const int32_t* desc, const int64_t* koff, const double* rand,
                 int32_t n_prob, int32_t max_n, double* work, int32_t* labels_out, int32_t* info) {
  if (!ctx || !keys || !desc || !koff || !rand || !work || !labels_out || !info || n_prob <= 0 || max_n < 0)
    return rhccq_fail(ctx, RHCCQ_E_ARG, "kmeans: bad argument");
  namespace W = rhccq_km_wide;
  constexpr int kMaxIter = 300;
  // which problems take the wide Lloyd path: one rule per problem, from `desc` (read back only when the call's largest problem could)
  std::vector<int32_t> hdesc, wide, wide_of;
  std::vector<KmWideTile> tiles;
  if (W::may_hold_wide(max_n, ctx->opt_kmeans_wide_pairs, kKmCentLds)) {
    hdesc.resize((size_t)n_prob * 6);
    RHCCQ_HIP(ctx, hipMemcpyAsync(hdesc.data(), desc, hdesc.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    RHCCQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    wide = W::wide_problems(hdesc.data(), n_prob, ctx->opt_kmeans_wide_pairs, kKmCentLds);
  }
  // scratch: the points and labels of problems too large for LDS, then the records and tables of the wide path
  int stride = 0;
  size_t pts_bytes = 0, bytes = 0;
  if (max_n > RHCCQ_KM_LDS_MAX) {
    stride = (max_n + 63) & ~63;
    pts_bytes = (size_t)n_prob * 2 * stride * sizeof(uint32_t);           // a multiple of 256
  }
  bytes = pts_bytes;
  size_t rec_at = 0, of_at = 0, list_at = 0, tile_at = 0;
  if (!wide.empty()) {
    tiles = W::build_tiles(hdesc.data(), wide, kKmWideTile);
    wide_of.assign((size_t)n_prob, -1);
    for (size_t w = 0; w < wide.size(); ++w) wide_of[(size_t)wide[w]] = (int32_t)w;
    auto take = [&](size_t b) { const size_t at = bytes; bytes += (b + 255) & ~(size_t)255; return at; };
    rec_at = take(wide.size() * sizeof(KmWideRec));
    of_at = take(wide_of.size() * sizeof(int32_t));
    list_at = take(wide.size() * sizeof(int32_t));
    tile_at = take(tiles.size() * sizeof(KmWideTile));
  }
  if (ctx->scratch_bytes < bytes) {
    if (ctx->scratch) RHCCQ_HIP(ctx, hipFree(ctx->scratch));
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    RHCCQ_HIP(ctx, hipMalloc(&ctx->scratch, bytes));
    ctx->scratch_bytes = bytes;
  }
  char* base = (char*)ctx->scratch;
  uint32_t* gpts = pts_bytes ? (uint32_t*)base : nullptr;
  KmWideRec* d_recs = nullptr;
  int32_t *d_of = nullptr, *d_list = nullptr;
  KmWideTile* d_tiles = nullptr;
  if (!wide.empty()) {
    d_recs = (KmWideRec*)(base + rec_at);
    d_of = (int32_t*)(base + of_at);
    d_list = (int32_t*)(base + list_at);
    d_tiles = (KmWideTile*)(base + tile_at);
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_of, wide_of.data(), wide_of.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_list, wide.data(), wide.size() * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    RHCCQ_HIP(ctx, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(KmWideTile), hipMemcpyHostToDevice, ctx->stream));
  }
  hipLaunchKernelGGL(kmeans_kernel, dim3(n_prob), dim3(kKmThreads), 0, ctx->stream, keys, desc, koff, rand, work, labels_out, info, gpts, stride, kMaxIter,
                     (const int32_t*)d_of, d_recs);
  RHCCQ_LAUNCH_CHECK(ctx);
  if (wide.empty()) return 0;
  // the Lloyd loop of the wide problems as launches: chunks of (E, M) pairs, the records read back behind each chunk (km_wide_host.h)
  int k_max = 1;
  for (int32_t p : wide) k_max = std::max(k_max, (int)hdesc[(size_t)p * 6 + 2]);
  const size_t lds = (size_t)k_max * 4 * sizeof(double);
  auto estep = [&]() -> int {
    hipLaunchKernelGGL(km_wide_estep_kernel, dim3((unsigned)tiles.size()), dim3(kKmWideThreads), lds, ctx->stream, keys, desc, koff, work, labels_out,
                       (const KmWideTile*)d_tiles, d_recs);
    RHCCQ_LAUNCH_CHECK(ctx);
    return 0;
  };
  auto mstep = [&]() -> int {
    hipLaunchKernelGGL(km_wide_mstep_kernel, dim3((unsigned)wide.size()), dim3(kKmThreads), 0, ctx->stream, keys, desc, koff, work, labels_out, info,
                       (const int32_t*)d_list, d_recs, kMaxIter);
    RHCCQ_LAUNCH_CHECK(ctx);
    return 0;
  };
  auto read_back = [&](KmWideRec* out) -> int {
    RHCCQ_HIP(ctx, hipMemcpyAsync(out, d_recs, wide.size() * sizeof(KmWideRec), hipMemcpyDeviceToHost, ctx->stream));
    RHCCQ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
  };
  std::vector<KmWideRec> hrec(wide.size());              // all running, as kmeans_kernel leaves them
  return W::drive(hrec, ctx->opt_kmeans_chunk, kMaxIter, estep, mstep, read_back);
}

#ifdef RHCCQ_KM_STAMPS
int rhccq_debug_km_stamps(unsigned long long* out, int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_km_stamps), sizeof(unsigned long long) * 8) != hipSuccess) return -1;
  if (reset) {
    const unsigned long long z[8] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_km_stamps), z, sizeof(z)) != hipSuccess) return -1;
  }
  return 0;
}
#endif

int rhccq_cluster_sums(rhccq_ctx* ctx, const uint32_t* keys, const int32_t* labels, int64_t n, int64_t k, unsigned long long* sums) {
  if (!ctx || n < 0 || k < 0 || (n > 0 && (!keys || !labels || !sums))) return rhccq_fail(ctx, RHCCQ_E_ARG, "cluster_sums: bad argument");
  if (n == 0) return 0;
  if (n <= (1ll << 24) && k > 0) {
    int64_t b = ((n + kSumRun - 1) / kSumRun + 255) / 256;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(cluster_sums_packed_kernel, dim3((int)b), dim3(256), 0, ctx->stream, keys, labels, n, sums);
    hipLaunchKernelGGL(cluster_unpack_kernel, dim3((int)((k + 255) / 256)), dim3(256), 0, ctx->stream, sums, k);
  } else {
    int64_t b = (n + 255) / 256;
    if (b > 2048) b = 2048;
    hipLaunchKernelGGL(cluster_sums_kernel, dim3((int)b), dim3(256), 0, ctx->stream, keys, labels, n, sums);
  }
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

int rhccq_cluster_means(rhccq_ctx* ctx, const unsigned long long* sums, int64_t k, uint32_t* keys_out) {
  if (!ctx || k < 0 || (k > 0 && (!sums || !keys_out))) return rhccq_fail(ctx, RHCCQ_E_ARG, "cluster_means: bad argument");
  if (k == 0) return 0;
  hipLaunchKernelGGL(cluster_means_kernel, dim3((int)((k + 255) / 256)), dim3(256), 0, ctx->stream, sums, k, keys_out);
  RHCCQ_LAUNCH_CHECK(ctx);
  return 0;
}

}  // extern "C"
