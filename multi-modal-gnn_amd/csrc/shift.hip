// Per-lab two-sample tests between two cohorts with permutation p-values (include/mmgnn_shift.h; mmgnn/shift.py):
// Kolmogorov-Smirnov, Wasserstein-1, standardised mean difference and coverage difference of every lab under the given
// labelling and under `replicates` relabellings of the units, the single-step maxT statistic, and the p-values.
//   k_sh_thresholds  one workgroup per replicate: U and U_A by a pass over `group`, then a radix select of the U_A-th
//                    smallest key_b(u): eight 8-bit digits from the top, the hash recomputed in every pass, the 256-bin
//                    histogram in LDS (integer atomics), the digit picked by one thread's walk over the bins.
//   k_sh_keys        ONE read of the pairs: sort key = lab << 32 | orderable(value) (n_seg << 32 for a dropped pair: sorts
//                    last), payload = the pair's position; the unit as uint32 with the given label in bit 31; the four
//                    kinds of dropped pairs (drop_flush of segsort.h).
//   segsort_run      the stable sort of segsort.h over the four digits of the value and the 1-2 of the lab.
//   k_seg_bounds     (segsort.h) bounds[s] = the first sorted position of lab s (s = n_seg: the number of kept pairs).
//   k_sh_walk<false> the counting pass: workgroup (c, y) walks chunk c (SH_CHUNK consecutive sorted pairs) for the SH_RB
//                    replicates y * SH_RB + thread.  Tiles of SH_TILE pairs are staged in LDS once; every thread reads
//                    the same LDS word (broadcast), hashes once per pair, compares with its threshold and counts.  All
//                    threads see the same lab boundaries: no divergence.  At a boundary the count goes to the chunk's
//                    HEAD slot, straight to n_a or to the chunk's TAIL slot: the chunk protocol stated at SegChunks
//                    (segsort.h).
//   k_sh_combine<false>  one thread per (lab, replicate): n_a = the slots in chunk order, and on the way the running
//                    count at the start of every chunk the lab heads.
//   k_sh_walk<true>  the same walk with the statistics: the running d = c_a n_b - c_b n_a = c_a n - c n_a moves by
//                    +n for a pair of A and by -n_a for every pair (one 64-bit add per pair, no multiply); at a tie
//                    group's end (a flag staged with the tile) the two maxima and the term of W.
//   k_sh_combine<true>   K by maximum, the fp64 sums in chunk order from 0; a lab without pairs gets zeros; a lab the walk
//                    wrote itself is left alone.  Every element of the outputs is written exactly once.
//   k_sh_finish      one thread per (replicate, row).   k_sh_summary  one workgroup per row: integer counts.
// fp64 contraction is OFF for the whole file: finish and summary restate numpy arithmetic operation by operation, and
// the term of W is a rounded product that is then added.
// Built into libmmgnn_shift.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "cells.h"
#include "radix_sort.h"
#include "../../include/mmgnn_shift.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SH_NTHR = 256;
constexpr int SH_RB = MMG_SHIFT_RB;
constexpr int SH_CHUNK = MMG_SHIFT_CHUNK;
constexpr int SH_TILE = 256;              // pairs staged in LDS at a time
constexpr int SH_MAX_GRID = 2048;
constexpr int SH_PART = 7;                // 8-byte words of a statistics slot: K_plus, K_minus, W, S_a, S_b, Q_a, Q_b
static_assert(SH_RB == SH_NTHR, "one replicate per thread");
static_assert(SH_TILE == SH_NTHR, "a thread stages one pair of a tile");
static_assert(SH_CHUNK % SH_TILE == 0, "a chunk is whole tiles");
static_assert(MMG_SHIFT_MAX_SEG < 65536, "the sort runs over two digits of the lab");
static_assert(SH_PART == 2 + MMG_SHIFT_SUM_FIELDS, "a slot is the two maxima and the sums");

// the first word of the group hash of unit u (u < 2^31: the high half of the 64-bit group index is 0)
__device__ __forceinline__ uint32_t sh_hash(uint32_t key, uint32_t u) {
  uint32_t w0, w1;
  mmg_rng_group(key, (uint64_t)u, &w0, &w1);       // w1 is dead code: only the first word is used
  return w0;
}

// ---------------------------------------------------------------------------------- thresholds
__global__ __launch_bounds__(SH_NTHR) void k_sh_thresholds(const uint8_t* __restrict__ group, uint32_t n_units,
                                                           uint64_t seed, unsigned long long* __restrict__ T,
                                                           long long* __restrict__ counts) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_cnt[2][SH_NTHR / WAVE];
  __shared__ unsigned long long s_prefix;
  __shared__ uint32_t s_k;
  const int b = blockIdx.x;
  int cu = 0, ca = 0;                              // per thread at most 2^31 / 256
  for (uint32_t u = threadIdx.x; u < n_units; u += SH_NTHR) {
    const uint32_t g = group[u];
    cu += g <= 1u ? 1 : 0;
    ca += g == 1u ? 1 : 0;
  }
  cu = wave_sum_i(cu);
  ca = wave_sum_i(ca);
  if ((threadIdx.x & 63) == 0) {
    s_cnt[0][threadIdx.x >> 6] = (uint32_t)cu;
    s_cnt[1][threadIdx.x >> 6] = (uint32_t)ca;
  }
  __syncthreads();
  uint32_t U = 0, UA = 0;
#pragma unroll
  for (int q = 0; q < SH_NTHR / WAVE; ++q) {
    U += s_cnt[0][q];
    UA += s_cnt[1][q];
  }
  const bool ok = UA >= 1u && UA < U;
  if (b == 0) {
    if (threadIdx.x == 0) {
      counts[0] = (long long)U;
      counts[1] = (long long)UA;
      counts[2] = ok ? MMG_SHIFT_OK : MMG_SHIFT_BAD_COHORTS;
      T[0] = 0ull;
    }
    return;
  }
  if (!ok) {
    if (threadIdx.x == 0) T[b] = 0ull;
    return;
  }
  const uint32_t key = mmg_rng_key(seed, (uint32_t)MMG_SHIFT_SITE + (uint32_t)b);
  unsigned long long prefix = 0ull;                // the digits chosen so far: key >> (shift + 8) of the wanted key
  uint32_t k = UA;                                 // the wanted key is the k-th smallest of those that share the prefix
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass;
    hist[threadIdx.x] = 0u;
    __syncthreads();
    for (uint32_t u = threadIdx.x; u < n_units; u += SH_NTHR) {
      if (group[u] <= 1) {
        const unsigned long long kk = ((unsigned long long)sh_hash(key, u) << 32) | u;
        if (pass == 0 || (kk >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(kk >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t run = 0u;
      int d = 0;
      for (; d < 255; ++d) {                       // the bins sum to >= k: the walk ends at 255 at the latest
        if (run + hist[d] >= k) break;
        run += hist[d];
      }
      s_k = k - run;
      s_prefix = (prefix << 8) | (unsigned long long)d;
    }
    __syncthreads();
    k = s_k;
    prefix = s_prefix;
  }
  if (threadIdx.x == 0) T[b] = prefix;
}

// ---------------------------------------------------------------------------------- keys
template <class IT>
__global__ __launch_bounds__(SH_NTHR) void k_sh_keys(const float* __restrict__ value, const IT* __restrict__ seg,
                                                     const IT* __restrict__ unit, const uint8_t* __restrict__ group,
                                                     int64_t n, int64_t n_units, int n_seg,
                                                     unsigned long long* __restrict__ key, int32_t* __restrict__ id,
                                                     uint32_t* __restrict__ unit32,
                                                     unsigned long long* __restrict__ dropped) {
  int cnt[MMG_SHIFT_DROP_KINDS] = {0, 0, 0, 0};
  const int64_t step = (int64_t)gridDim.x * SH_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * SH_NTHR + threadIdx.x; i < n; i += step) {
    const int64_t s = (int64_t)seg[i], u = (int64_t)unit[i];
    const float v = value[i];
    int kind = -1;
    uint32_t g = 0u;
    if (s < 0 || s >= n_seg) kind = 0;
    else if (u < 0 || u >= n_units) kind = 1;
    else if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) kind = 2;
    else {
      g = group[u];                                  // u is inside [0, n_units)
      if (g > 1u) kind = 3;
    }
    if (kind >= 0) cnt[kind] += 1;
    uint32_t vb = __float_as_uint(v);
    if ((vb << 1) == 0u) vb = 0u;                    // -0.0 is taken as +0.0
    key[i] = kind < 0 ? ((unsigned long long)s << 32) | bits_orderable(vb) : (unsigned long long)n_seg << 32;
    id[i] = (int32_t)i;
    unit32[i] = kind < 0 ? (uint32_t)u | (g << 31) : 0u;
  }
  drop_flush(cnt, dropped);
}

// ---------------------------------------------------------------------------------- the walk
// slot (chunk c, which: 0 head / 1 tail, replicate r) of the counting pass; word f of the statistics slot
__device__ __forceinline__ size_t sh_cslot(int64_t c, int which, int r, int R1) { return ((size_t)c * 2 + which) * R1 + r; }
__device__ __forceinline__ size_t sh_sslot(int64_t c, int which, int f, int r, int R1) {
  return (((size_t)c * 2 + which) * SH_PART + f) * R1 + r;
}

struct ShStat {
  long long kp, km;
  double w, sa, sb, qa, qb;
  __device__ __forceinline__ void clear() {
    kp = km = 0ll;
    w = sa = sb = qa = qb = 0.0;
  }
};

template <bool STATS>
__global__ __launch_bounds__(SH_NTHR) void k_sh_walk(const unsigned long long* __restrict__ K, const int32_t* __restrict__ id,
                                                     const uint32_t* __restrict__ unit32,
                                                     const int32_t* __restrict__ bounds, int n_seg, int replicates,
                                                     uint64_t seed, const unsigned long long* __restrict__ T,
                                                     uint32_t* __restrict__ cpart, int32_t* __restrict__ na,
                                                     const uint32_t* __restrict__ start, double* __restrict__ spart,
                                                     long long* __restrict__ counts, double* __restrict__ sums) {
  __shared__ uint32_t s_lab[SH_TILE], s_u[SH_TILE];
  __shared__ double s_v[STATS ? SH_TILE : 1], s_q[STATS ? SH_TILE : 1], s_dv[STATS ? SH_TILE : 1];
  __shared__ unsigned char s_end[STATS ? SH_TILE : 1];
  const int R1 = replicates + 1;
  const int r = blockIdx.y * SH_RB + threadIdx.x;
  const bool live = r < R1;
  const int64_t nk = bounds[n_seg];                                  // kept pairs
  const int64_t c = blockIdx.x, begin = c * SH_CHUNK;
  if (begin >= nk) return;                                           // the whole workgroup
  const int64_t end = begin + SH_CHUNK < nk ? begin + SH_CHUNK : nk;
  const uint32_t key = mmg_rng_key(seed, (uint32_t)MMG_SHIFT_SITE + (uint32_t)r);
  const unsigned long long Tr = live && r > 0 ? T[r] : 0ull;
  const uint32_t first = (uint32_t)(K[begin] >> 32);
  uint32_t cur = (uint32_t)n_seg;                                    // n_seg: no open lab
  uint32_t ca = 0u;                                                  // pairs of A: of the lab in the chunk (counting pass), of the lab so far
  long long d = 0ll, n_a = 0ll, n_tot = 0ll;
  ShStat acc;
  acc.clear();
  for (int64_t base = begin; base < end; base += SH_TILE) {
    __syncthreads();                                                 // the previous tile is consumed
    {
      const int64_t j = base + threadIdx.x;
      uint32_t lab = (uint32_t)n_seg;
      if (j < end) {
        const unsigned long long kj = K[j];
        lab = (uint32_t)(kj >> 32);
        s_u[threadIdx.x] = unit32[id[j]];
        if (STATS) {
          const unsigned long long kn = j + 1 < nk ? K[j + 1] : (unsigned long long)n_seg << 32;
          const bool same_lab = (uint32_t)(kn >> 32) == lab;
          const double v = (double)orderable_float((uint32_t)kj);
          s_v[threadIdx.x] = v;
          s_q[threadIdx.x] = v * v;
          s_end[threadIdx.x] = kn != kj ? 1 : 0;                     // equal keys: equal values of one lab
          s_dv[threadIdx.x] = same_lab ? (double)orderable_float((uint32_t)kn) - v : 0.0;
        }
      }
      s_lab[threadIdx.x] = lab;
    }
    __syncthreads();
    const int m = (int)(end - base < SH_TILE ? end - base : SH_TILE);
    for (int j = 0; j < m; ++j) {
      const uint32_t s = s_lab[j];                                   // the same word for every thread
      if (s != cur) {                                                // the open lab ends in front of a pair of s
        // HEAD slot or direct: the protocol at SegChunks
        if (cur < (uint32_t)n_seg && live) {
          if (!STATS) {
            if (cur == first) cpart[sh_cslot(c, 0, r, R1)] = ca;
            else na[(size_t)cur * R1 + r] = (int32_t)ca;
          } else if (cur == first) {
            spart[sh_sslot(c, 0, 0, r, R1)] = __longlong_as_double(acc.kp);
            spart[sh_sslot(c, 0, 1, r, R1)] = __longlong_as_double(acc.km);
            spart[sh_sslot(c, 0, 2, r, R1)] = acc.w;
            spart[sh_sslot(c, 0, 3, r, R1)] = acc.sa;
            spart[sh_sslot(c, 0, 4, r, R1)] = acc.sb;
            spart[sh_sslot(c, 0, 5, r, R1)] = acc.qa;
            spart[sh_sslot(c, 0, 6, r, R1)] = acc.qb;
          } else {
            long long* __restrict__ ci = counts + ((size_t)r * n_seg + cur) * MMG_SHIFT_INT_FIELDS;
            double* __restrict__ cd = sums + ((size_t)r * n_seg + cur) * MMG_SHIFT_SUM_FIELDS;
            ci[0] = n_a;
            ci[1] = n_tot - n_a;
            ci[2] = acc.kp;
            ci[3] = acc.km;
            cd[0] = acc.w;
            cd[1] = acc.sa;
            cd[2] = acc.sb;
            cd[3] = acc.qa;
            cd[4] = acc.qb;
          }
        }
        cur = s;
        ca = 0u;
        if (STATS) {
          acc.clear();
          const long long lo = bounds[s];
          n_tot = (long long)bounds[s + 1] - lo;
          n_a = live ? (long long)na[(size_t)s * R1 + r] : 0ll;
          if (s == first && live) ca = start[(size_t)c * R1 + r];
          d = (long long)ca * n_tot - ((long long)(base + j) - lo) * n_a;
        }
      }
      const uint32_t uw = s_u[j];
      const uint32_t u = uw & 0x7fffffffu;
      const uint32_t h = sh_hash(key, u);
      const bool a = r == 0 ? (uw >> 31) != 0u : (((unsigned long long)h << 32) | u) <= Tr;      // a select, not a branch
      ca += a ? 1u : 0u;
      if (STATS) {
        d += (a ? n_tot : 0ll) - n_a;
        const double v = s_v[j], q = s_q[j];
        acc.sa += a ? v : 0.0;
        acc.sb += a ? 0.0 : v;
        acc.qa += a ? q : 0.0;
        acc.qb += a ? 0.0 : q;
        if (s_end[j]) {                                              // the same for every thread
          const long long ad = d < 0 ? -d : d;
          acc.kp = d > acc.kp ? d : acc.kp;
          acc.km = -d > acc.km ? -d : acc.km;
          const double term = (double)ad * s_dv[j];
          acc.w += term;
        }
      }
    }
  }
  if (cur < (uint32_t)n_seg && live) {
    const int which = cur == first ? 0 : 1;
    if (!STATS) {
      cpart[sh_cslot(c, which, r, R1)] = ca;
    } else {
      spart[sh_sslot(c, which, 0, r, R1)] = __longlong_as_double(acc.kp);
      spart[sh_sslot(c, which, 1, r, R1)] = __longlong_as_double(acc.km);
      spart[sh_sslot(c, which, 2, r, R1)] = acc.w;
      spart[sh_sslot(c, which, 3, r, R1)] = acc.sa;
      spart[sh_sslot(c, which, 4, r, R1)] = acc.sb;
      spart[sh_sslot(c, which, 5, r, R1)] = acc.qa;
      spart[sh_sslot(c, which, 6, r, R1)] = acc.qb;
    }
  }
}

template <bool STATS>
__global__ __launch_bounds__(SH_NTHR) void k_sh_combine(const int32_t* __restrict__ bounds, int n_seg, int replicates,
                                                        const uint32_t* __restrict__ cpart, int32_t* __restrict__ na,
                                                        uint32_t* __restrict__ start, const double* __restrict__ spart,
                                                        long long* __restrict__ counts, double* __restrict__ sums) {
  const int R1 = replicates + 1;
  const int s = blockIdx.x;
  const SegChunks<SH_CHUNK> ch(bounds[s], bounds[s + 1], bounds[n_seg]);
  if (ch.written_by_walk()) return;
  for (int r = blockIdx.y * SH_NTHR + threadIdx.x; r < R1; r += gridDim.y * SH_NTHR) {
    if (!STATS) {
      uint32_t run = 0u;
      if (!ch.empty())
        for (int64_t c = ch.c0; c <= ch.c1; ++c) {
          const int which = ch.which(c);
          if (which == 0) start[(size_t)c * R1 + r] = run;
          run += cpart[sh_cslot(c, which, r, R1)];
        }
      na[(size_t)s * R1 + r] = (int32_t)run;
    } else {
      ShStat a;
      a.clear();
      if (!ch.empty())
        for (int64_t c = ch.c0; c <= ch.c1; ++c) {
          const int which = ch.which(c);
          const long long kp = __double_as_longlong(spart[sh_sslot(c, which, 0, r, R1)]);
          const long long km = __double_as_longlong(spart[sh_sslot(c, which, 1, r, R1)]);
          a.kp = kp > a.kp ? kp : a.kp;
          a.km = km > a.km ? km : a.km;
          a.w += spart[sh_sslot(c, which, 2, r, R1)];
          a.sa += spart[sh_sslot(c, which, 3, r, R1)];
          a.sb += spart[sh_sslot(c, which, 4, r, R1)];
          a.qa += spart[sh_sslot(c, which, 5, r, R1)];
          a.qb += spart[sh_sslot(c, which, 6, r, R1)];
        }
      const long long n_a = !ch.empty() ? (long long)na[(size_t)s * R1 + r] : 0ll;
      long long* __restrict__ ci = counts + ((size_t)r * n_seg + s) * MMG_SHIFT_INT_FIELDS;
      double* __restrict__ cd = sums + ((size_t)r * n_seg + s) * MMG_SHIFT_SUM_FIELDS;
      ci[0] = n_a;
      ci[1] = (long long)(ch.hi - ch.lo) - n_a;
      ci[2] = a.kp;
      ci[3] = a.km;
      cd[0] = a.w;
      cd[1] = a.sa;
      cd[2] = a.sb;
      cd[3] = a.qa;
      cd[4] = a.qb;
    }
  }
}

// ---------------------------------------------------------------------------------- finish
// the six statistics of one (replicate, lab); every operation rounded on its own (contraction is off)
__device__ __forceinline__ void sh_stats6(const long long* __restrict__ ci, const double* __restrict__ cd, double UA,
                                          double UB, double* __restrict__ out) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const long long n_a = ci[0], n_b = ci[1], kp = ci[2], km = ci[3];
  const double na = (double)n_a, nb = (double)n_b;
  out[5] = na / UA - nb / UB;
  if (n_a <= 0 || n_b <= 0) {
    out[0] = out[1] = out[2] = out[3] = out[4] = nan;
    return;
  }
  const double P = (double)(n_a * n_b);
  const double D = (double)(kp > km ? kp : km) / P;
  out[0] = D;
  out[1] = kp >= km ? D : -D;
  out[2] = cd[0] / P;
  double smd = nan;
  if (n_a >= 2 && n_b >= 2) {
    const double sa = cd[1], sb = cd[2];
    double va = (cd[3] - sa * sa / na) / (na - 1.0), vb = (cd[4] - sb * sb / nb) / (nb - 1.0);
    va = va > 0.0 ? va : 0.0;
    vb = vb > 0.0 ? vb : 0.0;
    const double num = sa / na - sb / nb, den = __dsqrt_rn((va + vb) / 2.0);
    smd = num == 0.0 && den == 0.0 ? 0.0 : num / den;
  }
  out[3] = smd;
  out[4] = D * __dsqrt_rn(P / (na + nb));
}

__global__ __launch_bounds__(SH_NTHR) void k_sh_finish(const long long* __restrict__ counts, const double* __restrict__ sums,
                                                       const long long* __restrict__ cohort, int n_seg, int replicates,
                                                       double* __restrict__ stats) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const double UA = (double)cohort[1], UB = (double)(cohort[0] - cohort[1]);
  const int64_t cells = (int64_t)(replicates + 1) * (n_seg + 1);
  for (int64_t q = (int64_t)blockIdx.x * SH_NTHR + threadIdx.x; q < cells; q += (int64_t)gridDim.x * SH_NTHR) {
    // the rows of the maximum first: they are the long ones
    const int r = (int)(q % (replicates + 1));
    const int row = n_seg - (int)(q / (replicates + 1));
    double* __restrict__ out = stats + ((size_t)r * (n_seg + 1) + row) * MMG_SHIFT_STAT_FIELDS;
    double v[MMG_SHIFT_STAT_FIELDS];
    if (row < n_seg) {
      const size_t cell = (size_t)r * n_seg + row;
      sh_stats6(counts + cell * MMG_SHIFT_INT_FIELDS, sums + cell * MMG_SHIFT_SUM_FIELDS, UA, UB, v);
#pragma unroll
      for (int f = 0; f < MMG_SHIFT_STAT_FIELDS; ++f) out[f] = v[f];
    } else {
      double best = nan;
      for (int s = 0; s < n_seg; ++s) {
        const size_t cell = (size_t)r * n_seg + s;
        sh_stats6(counts + cell * MMG_SHIFT_INT_FIELDS, sums + cell * MMG_SHIFT_SUM_FIELDS, UA, UB, v);
        const double z = v[4];
        if (z == z && !(best >= z)) best = z;                        // the first value, then the larger one
      }
#pragma unroll
      for (int f = 0; f < MMG_SHIFT_STAT_FIELDS; ++f) out[f] = f == 4 ? best : nan;
    }
  }
}

// ---------------------------------------------------------------------------------- summary
constexpr int SH_TALLY = 10;                 // >= and not-NaN counts of D, W1, |smd|, |cov|, maxz

__global__ __launch_bounds__(SH_NTHR) void k_sh_summary(const double* __restrict__ stats, int n_seg, int replicates,
                                                        double* __restrict__ summary) {
  __shared__ int s_c[SH_TALLY][SH_NTHR / WAVE];
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  const int row = blockIdx.x;
  const size_t stride = (size_t)(n_seg + 1) * MMG_SHIFT_STAT_FIELDS;       // between two replicates
  const double* __restrict__ src = stats + (size_t)row * MMG_SHIFT_STAT_FIELDS;
  const double* __restrict__ top = stats + (size_t)n_seg * MMG_SHIFT_STAT_FIELDS;
  const bool lab = row < n_seg;
  // row n_seg: only the maximum against itself (src[4] is maxz_0 there)
  const double x0[5] = {lab ? src[0] : nan, lab ? src[2] : nan, lab ? fabs(src[3]) : nan, lab ? fabs(src[5]) : nan, src[4]};
  int cnt[SH_TALLY];
#pragma unroll
  for (int k = 0; k < SH_TALLY; ++k) cnt[k] = 0;
  for (int b = 1 + threadIdx.x; b <= replicates; b += SH_NTHR) {
    const double* __restrict__ p = src + (size_t)b * stride;
    const double xb[5] = {p[0], p[2], fabs(p[3]), fabs(p[5]), top[(size_t)b * stride + 4]};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      cnt[2 * k] += xb[k] >= x0[k] ? 1 : 0;
      cnt[2 * k + 1] += xb[k] == xb[k] ? 1 : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < SH_TALLY; ++k) {
    const int t = wave_sum_i(cnt[k]);
    if ((threadIdx.x & 63) == 0) s_c[k][threadIdx.x >> 6] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot[SH_TALLY];
#pragma unroll
    for (int k = 0; k < SH_TALLY; ++k) {
      tot[k] = 0;
      for (int q = 0; q < SH_NTHR / WAVE; ++q) tot[k] += s_c[k][q];
    }
    double* __restrict__ out = summary + (size_t)row * MMG_SHIFT_SUMMARY_FIELDS;
#pragma unroll
    for (int k = 0; k < 5; ++k)
      out[k] = x0[k] == x0[k] ? (1.0 + (double)tot[2 * k]) / (1.0 + (double)tot[2 * k + 1]) : nan;
    out[5] = lab ? (double)tot[0] : nan;
    out[6] = (double)tot[8];
  }
}

struct ShiftWs {
  SegSortWs<unsigned long long> sort;
  uint32_t *unit32, *cpart, *start;
  int32_t *bounds, *na;
  double* spart;
};
inline int64_t sh_chunks(int64_t n) { return n > 0 ? (n + SH_CHUNK - 1) / SH_CHUNK : 1; }
size_t shift_carve(void* ws, int64_t n, int n_seg, int replicates, ShiftWs* w) {
  MmgCarver c(ws);
  const size_t nn = (size_t)(n > 0 ? n : 1), R1 = (size_t)replicates + 1, ch = (size_t)sh_chunks(n);
  segsort_carve(c, n, &w->sort);
  w->unit32 = c.take<uint32_t>(nn);
  w->bounds = c.take<int32_t>((size_t)n_seg + 2);
  w->na = c.take<int32_t>((size_t)n_seg * R1);
  w->cpart = c.take<uint32_t>(ch * 2 * R1);
  w->start = c.take<uint32_t>(ch * R1);
  w->spart = c.take<double>(ch * 2 * SH_PART * R1);
  return c.need();
}

bool shape_ok(int n_seg, int replicates) {
  return n_seg >= 1 && n_seg <= MMG_SHIFT_MAX_SEG && replicates >= 0 && replicates <= MMG_SHIFT_MAX_REPLICATES;
}
int shape_check(const char* what, int n_seg, int replicates) {
  MMG_CHECK_ARG(replicates >= 0 && replicates <= MMG_SHIFT_MAX_REPLICATES, "%s: %d replicates outside [0, %d]", what,
                replicates, MMG_SHIFT_MAX_REPLICATES);
  MMG_CHECK_ARG(n_seg >= 1 && n_seg <= MMG_SHIFT_MAX_SEG, "%s: %d segments outside [1, %d]", what, n_seg, MMG_SHIFT_MAX_SEG);
  return MMG_OK;
}

}  // namespace

extern "C" int mmg_shift_thresholds(const uint8_t* group, int64_t n_units, int replicates, uint64_t seed, uint64_t* T,
                                    int64_t* counts, void* stream) {
  MMG_CHECK_ARG(replicates >= 0 && replicates <= MMG_SHIFT_MAX_REPLICATES, "shift_thresholds: %d replicates outside [0, %d]",
                replicates, MMG_SHIFT_MAX_REPLICATES);
  MMG_CHECK_ARG(n_units >= 0 && n_units <= INT32_MAX, "shift_thresholds: %lld units outside [0, 2^31)", (long long)n_units);
  MMG_CHECK_ARG(n_units == 0 || group, "shift_thresholds: null group");
  MMG_CHECK_ARG(T && counts, "shift_thresholds: null output");
  hipLaunchKernelGGL(k_sh_thresholds, dim3((unsigned)(replicates + 1)), dim3(SH_NTHR), 0, (hipStream_t)stream, group,
                     (uint32_t)n_units, seed, (unsigned long long*)T, (long long*)counts);
  MMG_CHECK_LAUNCH("shift_thresholds");
  return MMG_OK;
}

extern "C" size_t mmg_shift_stats_ws_bytes(int64_t n, int n_seg, int replicates) {
  if (n < 0 || n > INT32_MAX || !shape_ok(n_seg, replicates)) return 0;
  ShiftWs w;
  return shift_carve(nullptr, n, n_seg, replicates, &w);
}

extern "C" int mmg_shift_stats(const float* value, const void* seg, const void* unit, int index_bytes, int64_t n, int n_seg,
                               const uint8_t* group, int64_t n_units, int replicates, uint64_t seed, const uint64_t* T,
                               int64_t* counts, double* sums, int64_t* dropped, void* ws, size_t ws_bytes, void* stream) {
  int rc = shape_check("shift_stats", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(index_bytes == 4 || index_bytes == 8, "shift_stats: index_bytes %d is neither 4 nor 8", index_bytes);
  MMG_CHECK_ARG(n >= 0 && n <= INT32_MAX, "shift_stats: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_units >= 0 && n_units <= INT32_MAX, "shift_stats: %lld units outside [0, 2^31)", (long long)n_units);
  MMG_CHECK_ARG(n == 0 || (value && seg && unit), "shift_stats: null value, seg or unit");
  MMG_CHECK_ARG(n_units == 0 || group, "shift_stats: null group");
  MMG_CHECK_ARG(T, "shift_stats: null thresholds");
  MMG_CHECK_ARG(counts && sums && dropped, "shift_stats: null output");
  ShiftWs w;
  MMG_CHECK_WS("shift_stats", shift_carve(ws, n, n_seg, replicates, &w));
  const RadixPairs<unsigned long long>& kv = w.sort.kv;       // the sort leaves its result here
  hipStream_t st = (hipStream_t)stream;
  MMG_CHECK_HIP(mmg_zero_async(dropped, MMG_SHIFT_DROP_KINDS * sizeof(int64_t), st), "shift_stats(zero)");
  const unsigned rblocks = (unsigned)((replicates + 1 + SH_RB - 1) / SH_RB);
  if (n > 0) {
    index_dispatch(index_bytes, [&](auto it) {
      using IT = decltype(it);
      hipLaunchKernelGGL(k_sh_keys<IT>, dim3(launch_grid(n, SH_NTHR, SH_MAX_GRID)), dim3(SH_NTHR), 0, st, value,
                         (const IT*)seg, (const IT*)unit, group, n, n_units, n_seg, kv.keys, kv.vals, w.unit32,
                         (unsigned long long*)dropped);
    });
    MMG_CHECK_LAUNCH("shift_stats(keys)");
    segsort_run(w.sort, n, 32 + bits_of((unsigned)n_seg), st);           // the value, and a lab digit that reaches n_seg
    MMG_CHECK_LAUNCH("shift_stats(sort)");
  }
  seg_bounds(kv.keys, n, n_seg, 32, w.bounds, st);
  MMG_CHECK_LAUNCH("shift_stats(bounds)");
  const dim3 wgrid((unsigned)sh_chunks(n), rblocks), cgrid((unsigned)n_seg, rblocks), block(SH_NTHR);
  const unsigned long long* Tu = (const unsigned long long*)T;
  if (n > 0) {
    hipLaunchKernelGGL(k_sh_walk<false>, wgrid, block, 0, st, kv.keys, kv.vals, w.unit32, w.bounds, n_seg, replicates, seed,
                       Tu, w.cpart, w.na, w.start, w.spart, (long long*)counts, sums);
    MMG_CHECK_LAUNCH("shift_stats(count)");
    hipLaunchKernelGGL(k_sh_combine<false>, cgrid, block, 0, st, w.bounds, n_seg, replicates, w.cpart, w.na, w.start, w.spart,
                       (long long*)counts, sums);
    MMG_CHECK_LAUNCH("shift_stats(prefix)");
    hipLaunchKernelGGL(k_sh_walk<true>, wgrid, block, 0, st, kv.keys, kv.vals, w.unit32, w.bounds, n_seg, replicates, seed,
                       Tu, w.cpart, w.na, w.start, w.spart, (long long*)counts, sums);
    MMG_CHECK_LAUNCH("shift_stats(walk)");
  }
  hipLaunchKernelGGL(k_sh_combine<true>, cgrid, block, 0, st, w.bounds, n_seg, replicates, w.cpart, w.na, w.start, w.spart,
                     (long long*)counts, sums);
  MMG_CHECK_LAUNCH("shift_stats(combine)");
  return MMG_OK;
}

extern "C" int mmg_shift_finish(const int64_t* counts, const double* sums, const int64_t* cohort, int n_seg, int replicates,
                                double* stats, void* stream) {
  int rc = shape_check("shift_finish", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(counts && sums && cohort && stats, "shift_finish: null counts, sums, cohort or stats");
  const int64_t cells = (int64_t)(replicates + 1) * (n_seg + 1);
  hipLaunchKernelGGL(k_sh_finish, dim3(launch_grid(cells, SH_NTHR, SH_MAX_GRID, 1)), dim3(SH_NTHR), 0, (hipStream_t)stream,
                     (const long long*)counts, sums, (const long long*)cohort, n_seg, replicates, stats);
  MMG_CHECK_LAUNCH("shift_finish");
  return MMG_OK;
}

extern "C" int mmg_shift_summary(const double* stats, int n_seg, int replicates, double* summary, void* stream) {
  int rc = shape_check("shift_summary", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(stats && summary, "shift_summary: null stats or summary");
  hipLaunchKernelGGL(k_sh_summary, dim3((unsigned)(n_seg + 1)), dim3(SH_NTHR), 0, (hipStream_t)stream, stats, n_seg,
                     replicates, summary);
  MMG_CHECK_LAUNCH("shift_summary");
  return MMG_OK;
}
