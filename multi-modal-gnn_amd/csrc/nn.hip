// Exact nearest neighbours and neighbour ranks of fp32 rows X [n, D] (include/mmgnn_nn.h; mmgnn/neighbors.py): what
// sklearn.neighbors.NearestNeighbors(algorithm="brute") and the rank count of sklearn.manifold.trustworthiness compute,
// without an n x n matrix.
//   distance  s(q, j) = sum_d (q_d - x_jd)^2, the difference form in fp64 from the widened fp32 inputs, columns
//             ascending, one fma per column: the patch arithmetic of k_tsne_sqdist (csrc/tsne.hip), here for any D;
//   key       (s, j) compared lexicographically, a non-finite s taken as +inf: a TOTAL order, so the k smallest keys of
//             a query and their order do not depend on the tiling, the candidate split or the order of insertion.
// nn_tile_dist is the shared tile machinery: a 256-thread workgroup owns NN_B = 64 query rows, stages NN_DC columns of
// them and of NN_T = 64 candidate rows in LDS as doubles, every thread accumulates a 4 x 4 patch, and the 64 x 64 block
// of sums is left in LDS (over the staging buffers) with one query row per wave-wide read.
//   k_nn_search  a work item = (query block, candidate range).  Every query of the block keeps its k best keys sorted
//                in LDS ([64][k] doubles + ints).  Per tile a wave walks its 16 query rows: lane l holds candidate l of
//                the tile, a ballot against the row's k-th key finds the candidates that enter (usually none), and each
//                of them is inserted by the whole wave: its position is a ballot count, the shift is a lane shuffle (the
//                list sits in registers, slot e in lane e & 63, while the row is worked).  One range: the lists are the
//                result.  Several: they go to the workspace and
//   k_nn_merge   one wave per query merges the ranges' sorted lists: lane r holds the head of range r, a butterfly
//                minimum over the keys picks the next output, k times.
//   k_nn_rank    per query block, the keys of the row's k listed neighbours are the thresholds ([64][k] in LDS, the
//                sums by the same fma chain).  Per tile a lane owns thresholds c = lane and lane + 64 of each of its
//                wave's 16 rows and counts the tile's keys below them -- only the candidates a ballot finds at or below
//                the row's largest threshold are walked (for the neighbours of a faithful map: few); the counts stay in
//                registers until the block is done.  rank = 1 + count; the penalty is summed per wave and added with
//                one integer atomic.
//
// Built into libmmgnn_nn.so (include/mmgnn_nn.h), beside libmmgnn.so and on top of it (mmg_set_error, the launch probe):
// the training library is then built from exactly the sources it had.
#include "common.h"
#include "../../include/mmgnn_nn.h"
#include <math.h>

namespace {

constexpr int NN_NTHR = 256;
constexpr int NN_B = MMG_NN_QUERY_BLOCK;           // query rows of a workgroup
constexpr int NN_T = MMG_NN_TILE;                  // candidate rows per LDS tile = lanes of a wave
constexpr int NN_DC = 32;                          // columns per staged chunk
constexpr int NN_LD = NN_T + 1;                    // LDS row stride of the staging buffers and of the block of sums
constexpr int NN_ROWS_PER_WAVE = NN_B / (NN_NTHR / 64);
constexpr int NN_MIN_TILES = 4;                    // a candidate range is at least this many tiles
constexpr int NN_MAX_SPLIT = 64;                   // ranges per query: one lane each in the merge
constexpr int NN_JNONE = 0x7fffffff;               // the index of an empty list slot: above every row (n < 2^31)
constexpr int NN_LDS_MAX = NN_B * MMG_NN_MAX_K * 12;
static_assert(NN_B == 64 && NN_T == 64 && NN_NTHR == 256, "a thread owns a 4 x 4 patch of the 64 x 64 block; a wave spans a tile");
static_assert(2 * NN_DC * NN_LD >= NN_B * NN_LD, "the block of sums lies over the staging buffers");
static_assert(MMG_NN_MAX_K <= 128, "a lane holds two list slots");

struct NnPlan {
  int64_t nqb, ntiles, tps, items;   // query blocks, candidate tiles, tiles per range, work items
  int nsplit;                        // candidate ranges
  unsigned grid;
};
inline NnPlan nn_plan(int64_t n, int64_t nq) {
  NnPlan p;
  p.nqb = (nq + NN_B - 1) / NN_B;
  p.ntiles = (n + NN_T - 1) / NN_T;
  const int64_t want = p.nqb >= MMG_NN_MAX_GRID ? 1 : (MMG_NN_MAX_GRID + p.nqb - 1) / p.nqb;
  int64_t most = p.ntiles / NN_MIN_TILES;
  most = most < 1 ? 1 : most > NN_MAX_SPLIT ? NN_MAX_SPLIT : most;
  const int64_t ns = want < most ? want : most;
  p.tps = (p.ntiles + ns - 1) / ns;
  p.nsplit = (int)((p.ntiles + p.tps - 1) / p.tps);          // no empty range
  p.items = p.nqb * p.nsplit;
  p.grid = (unsigned)(p.items < MMG_NN_MAX_GRID ? p.items : MMG_NN_MAX_GRID);
  return p;
}

__device__ __forceinline__ bool key_less(double sa, int ja, double sb, int jb) { return sa < sb || (sa == sb && ja < jb); }

// sm[r * NN_LD + c] = s(query q0 + r, candidate j0 + c) for the 64 x 64 block (rows past nq / n: sums over zeros, never
// used).  Begins and ends with a barrier: the previous reader of sm is done, the block is visible.
__device__ __forceinline__ void nn_tile_dist(const float* __restrict__ Qp, int64_t ld_q, int64_t nq, int64_t q0,
                                             const float* __restrict__ X, int64_t ld_x, int64_t n, int64_t j0, int D,
                                             double* __restrict__ sm) {
  double(*xi)[NN_LD] = reinterpret_cast<double(*)[NN_LD]>(sm);
  double(*xj)[NN_LD] = reinterpret_cast<double(*)[NN_LD]>(sm + NN_DC * NN_LD);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int d0 = 0; d0 < D; d0 += NN_DC) {
    const int cw = D - d0 < NN_DC ? D - d0 : NN_DC;
    __syncthreads();                                 // the previous chunk (or block of sums) has been consumed
    for (int e = tid; e < NN_B * NN_DC; e += NN_NTHR) {
      const int r = e / NN_DC, c = e % NN_DC;
      if (c >= cw) continue;
      const int64_t ri = q0 + r, rj = j0 + r;
      xi[c][r] = ri < nq ? (double)Qp[ri * ld_q + d0 + c] : 0.0;
      xj[c][r] = rj < n ? (double)X[rj * ld_x + d0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < cw; ++c) {
      double a[4], b[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) { a[p] = xi[c][4 * ty + p]; b[p] = xj[c][4 * tx + p]; }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double df = a[p] - b[q];
          acc[p][q] = fma(df, df, acc[p][q]);
        }
    }
  }
  __syncthreads();                                   // the last chunk has been read: the block of sums overwrites it
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) sm[(4 * ty + p) * NN_LD + 4 * tx + q] = isfinite(acc[p][q]) ? acc[p][q] : (double)INFINITY;
  __syncthreads();
}

__global__ __launch_bounds__(NN_NTHR) void k_nn_search(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                       const float* __restrict__ Qp, int64_t nq, int64_t ld_q, int self,
                                                       int k, int nsplit, int64_t tps, int64_t ntiles, int64_t items,
                                                       float* __restrict__ dist_out, int64_t ld_dist,
                                                       int64_t* __restrict__ idx_out, int64_t ld_idx,
                                                       double* __restrict__ part_s, int32_t* __restrict__ part_j) {
  __shared__ double sm[2 * NN_DC * NN_LD];
  extern __shared__ double nn_dyn[];
  double* ls = nn_dyn;                                           // [NN_B][k] sums of the lists, ascending by key
  int* lj = reinterpret_cast<int*>(ls + (size_t)NN_B * k);       // [NN_B][k] their rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool two = k > 64;                                       // slots 64 .. k - 1 exist (uniform)
  const int e0 = lane, e1 = lane + 64;
  const int last_lane = (k - 1) & 63;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t qb = item / nsplit, q0 = qb * NN_B;
    const int sp = (int)(item - qb * nsplit);
    const int64_t t0 = sp * tps, t1 = t0 + tps < ntiles ? t0 + tps : ntiles;
    __syncthreads();                                 // the previous item's lists have been written out
    for (int e = tid; e < NN_B * k; e += NN_NTHR) { ls[e] = (double)INFINITY; lj[e] = NN_JNONE; }
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t j0 = t * NN_T;
      nn_tile_dist(Qp, ld_q, nq, q0, X, ld_x, n, j0, D, sm);     // (its barriers order the list initialisation too)
      for (int rr = 0; rr < NN_ROWS_PER_WAVE; ++rr) {
        const int r = wave * NN_ROWS_PER_WAVE + rr;
        const int64_t q = q0 + r;
        if (q >= nq) break;                          // wave-uniform
        const int64_t jl64 = j0 + lane;
        const int jl = (int)jl64;
        const double s = sm[r * NN_LD + lane];
        double thr_s = ls[r * k + k - 1];
        int thr_j = lj[r * k + k - 1];
        const bool ok = jl64 < n && !(self && jl64 == q) && key_less(s, jl, thr_s, thr_j);
        unsigned long long mask = __ballot(ok);
        if (!mask) continue;
        double s0 = e0 < k ? ls[r * k + e0] : (double)INFINITY, s1 = (two && e1 < k) ? ls[r * k + e1] : (double)INFINITY;
        int i0 = e0 < k ? lj[r * k + e0] : NN_JNONE, i1 = (two && e1 < k) ? lj[r * k + e1] : NN_JNONE;
        while (mask) {                               // the entering candidates in ascending row order; all lanes take part
          const int b = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          const double cs = __shfl(s, b, 64);
          const int cj = __shfl(jl, b, 64);
          if (!key_less(cs, cj, thr_s, thr_j)) continue;         // the k-th key has moved since the ballot
          int p = __popcll(__ballot(e0 < k && key_less(s0, i0, cs, cj)));
          if (two) p += __popcll(__ballot(e1 < k && key_less(s1, i1, cs, cj)));
          const double up_s0 = __shfl_up(s0, 1, 64);
          const int up_i0 = __shfl_up(i0, 1, 64);
          if (two) {
            double up_s1 = __shfl_up(s1, 1, 64);
            int up_i1 = __shfl_up(i1, 1, 64);
            const double w_s = __shfl(s0, 63, 64);
            const int w_i = __shfl(i0, 63, 64);
            if (lane == 0) { up_s1 = w_s; up_i1 = w_i; }
            s1 = e1 < p ? s1 : e1 == p ? cs : up_s1;
            i1 = e1 < p ? i1 : e1 == p ? cj : up_i1;
          }
          s0 = e0 < p ? s0 : e0 == p ? cs : up_s0;
          i0 = e0 < p ? i0 : e0 == p ? cj : up_i0;
          thr_s = __shfl(two ? s1 : s0, last_lane, 64);
          thr_j = __shfl(two ? i1 : i0, last_lane, 64);
        }
        if (e0 < k) { ls[r * k + e0] = s0; lj[r * k + e0] = i0; }
        if (two && e1 < k) { ls[r * k + e1] = s1; lj[r * k + e1] = i1; }
      }
    }
    __syncthreads();
    for (int e = tid; e < NN_B * k; e += NN_NTHR) {
      const int r = e / k, c = e - r * k;
      const int64_t q = q0 + r;
      if (q >= nq) continue;
      if (nsplit == 1) {
        dist_out[q * ld_dist + c] = (float)sqrt(ls[e]);
        idx_out[q * ld_idx + c] = (int64_t)lj[e];
      } else {
        const int64_t o = (q * nsplit + sp) * k + c;
        part_s[o] = ls[e];
        part_j[o] = lj[e];
      }
    }
  }
}

// the ranges' lists of a query -> its k smallest keys.  One wave per query, lane r reads range r.
__global__ __launch_bounds__(NN_NTHR) void k_nn_merge(const double* __restrict__ part_s, const int32_t* __restrict__ part_j,
                                                      int64_t nq, int nsplit, int k, float* __restrict__ dist_out,
                                                      int64_t ld_dist, int64_t* __restrict__ idx_out, int64_t ld_idx) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * (NN_NTHR / 64) + (threadIdx.x >> 6);
  if (q >= nq) return;                               // wave-uniform
  const bool live = lane < nsplit;
  const int64_t base = (q * nsplit + (live ? lane : 0)) * k;
  int head = 0;
  double cur_s = live ? part_s[base] : (double)INFINITY;
  int cur_j = live ? part_j[base] : NN_JNONE;
  for (int c = 0; c < k; ++c) {
    double ms = cur_s;
    int mj = cur_j;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double os = __shfl_xor(ms, o, 64);
      const int oj = __shfl_xor(mj, o, 64);
      if (key_less(os, oj, ms, mj)) { ms = os; mj = oj; }
    }
    if (lane == 0) {
      dist_out[q * ld_dist + c] = (float)sqrt(ms);
      idx_out[q * ld_idx + c] = (int64_t)mj;
    }
    if (live && cur_j == mj && mj != NN_JNONE) {     // the rows of the ranges are disjoint: one owner
      ++head;
      cur_s = head < k ? part_s[base + head] : (double)INFINITY;
      cur_j = head < k ? part_j[base + head] : NN_JNONE;
    }
  }
}

__global__ __launch_bounds__(NN_NTHR) void k_nn_rank(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                     const int64_t* __restrict__ nbr, int64_t ld_nbr, int k, int64_t nqb,
                                                     int64_t ntiles, int32_t* __restrict__ rank_out, int64_t ld_rank,
                                                     unsigned long long* __restrict__ penalty_out) {
  __shared__ double sm[2 * NN_DC * NN_LD];
  extern __shared__ double nn_dyn[];
  double* ts = nn_dyn;                                           // [NN_B][k] the thresholds' sums
  int* tj = reinterpret_cast<int*>(ts + (size_t)NN_B * k);       // [NN_B][k] their rows, -1: not a valid entry
  __shared__ double smax[NN_B];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool two = k > 64;
  const int c0 = lane, c1 = lane + 64;
  for (int64_t qb = blockIdx.x; qb < nqb; qb += gridDim.x) {
    const int64_t q0 = qb * NN_B;
    __syncthreads();                                 // the previous block's thresholds have been read
    for (int e = tid; e < NN_B * k; e += NN_NTHR) {
      const int r = e / k, c = e - r * k;
      const int64_t i = q0 + r;
      double s = -(double)INFINITY;                  // no key is below it
      int jj = -1;
      if (i < n) {
        const int64_t j = nbr[i * ld_nbr + c];
        if (j >= 0 && j < n && j != i) {
          const float* __restrict__ xi = X + i * ld_x;
          const float* __restrict__ xj = X + j * ld_x;
          double acc = 0.0;
          for (int d = 0; d < D; ++d) {
            const double df = (double)xi[d] - (double)xj[d];
            acc = fma(df, df, acc);
          }
          s = isfinite(acc) ? acc : (double)INFINITY;
          jj = (int)j;
        }
      }
      ts[e] = s;
      tj[e] = jj;
    }
    __syncthreads();
    if (tid < NN_B) {                                // the row's largest threshold: a sum above it is below no key
      double m = -(double)INFINITY;
      for (int c = 0; c < k; ++c) m = fmax(m, ts[tid * k + c]);
      smax[tid] = m;
    }
    int cnt0[NN_ROWS_PER_WAVE], cnt1[NN_ROWS_PER_WAVE];
#pragma unroll
    for (int rr = 0; rr < NN_ROWS_PER_WAVE; ++rr) { cnt0[rr] = 0; cnt1[rr] = 0; }
    for (int64_t t = 0; t < ntiles; ++t) {
      const int64_t j0 = t * NN_T;
      nn_tile_dist(X, ld_x, n, q0, X, ld_x, n, j0, D, sm);       // (its barriers order the thresholds too)
      const int lim = n - j0 < NN_T ? (int)(n - j0) : NN_T;
#pragma unroll
      for (int rr = 0; rr < NN_ROWS_PER_WAVE; ++rr) {
        const int r = wave * NN_ROWS_PER_WAVE + rr;
        const int64_t i = q0 + r;
        if (i < n) {                                 // wave-uniform
          const double a_s0 = c0 < k ? ts[r * k + c0] : -(double)INFINITY;
          const int a_j0 = c0 < k ? tj[r * k + c0] : -1;
          const double a_s1 = (two && c1 < k) ? ts[r * k + c1] : -(double)INFINITY;
          const int a_j1 = (two && c1 < k) ? tj[r * k + c1] : -1;
          const int skip = (i >= j0 && i < j0 + lim) ? (int)(i - j0) : -1;      // l == i is not counted
          int n0 = 0, n1 = 0;
          // lane l holds candidate l: only the candidates at or below the row's largest threshold can count
          unsigned long long mask = __ballot(lane < lim && lane != skip && sm[r * NN_LD + lane] <= smax[r]);
          while (mask) {                             // wave-uniform
            const int l = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const double ds = sm[r * NN_LD + l];                 // one address for the wave: a broadcast
            const int jl = (int)(j0 + l);
            n0 += key_less(ds, jl, a_s0, a_j0) ? 1 : 0;
            if (two) n1 += key_less(ds, jl, a_s1, a_j1) ? 1 : 0;
          }
          cnt0[rr] += n0;
          cnt1[rr] += n1;
        }
      }
    }
    long long pen = 0;
#pragma unroll
    for (int rr = 0; rr < NN_ROWS_PER_WAVE; ++rr) {
      const int r = wave * NN_ROWS_PER_WAVE + rr;
      const int64_t i = q0 + r;
      if (i < n) {
        if (c0 < k) {
          const int rank = tj[r * k + c0] >= 0 ? 1 + cnt0[rr] : 0;
          if (rank_out) rank_out[i * ld_rank + c0] = rank;
          pen += rank > k ? rank - k : 0;
        }
        if (two && c1 < k) {
          const int rank = tj[r * k + c1] >= 0 ? 1 + cnt1[rr] : 0;
          if (rank_out) rank_out[i * ld_rank + c1] = rank;
          pen += rank > k ? rank - k : 0;
        }
      }
    }
    if (penalty_out) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) pen += __shfl_xor(pen, o, 64);
      if (lane == 0 && pen != 0) atomicAdd(penalty_out, (unsigned long long)pen);
    }
  }
}

inline bool nn_shape_ok(int64_t n, int D, int k) {
  return n >= 1 && n < (1ll << 31) && D >= 1 && D <= MMG_NN_MAX_D && k >= 1 && k <= MMG_NN_MAX_K;
}
struct SearchWs { double* part_s; int32_t* part_j; };
size_t search_carve(void* ws, int64_t nq, int k, const NnPlan& p, SearchWs* w) {
  const size_t cnt = p.nsplit > 1 ? (size_t)nq * (size_t)p.nsplit * (size_t)k : 0;
  MmgCarver c(ws);
  *w = SearchWs{c.take<double>(cnt), c.take<int32_t>(cnt)};
  return c.need();
}

}  // namespace

extern "C" int mmg_nn_plan(int64_t n, int64_t nq, int64_t* plan_out) {
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31) && nq >= 1 && nq < (1ll << 31), "nn_plan: n %lld or nq %lld outside [1, 2^31)",
                (long long)n, (long long)nq);
  MMG_CHECK_ARG(plan_out, "nn_plan: null pointer (plan_out)");
  const NnPlan p = nn_plan(n, nq);
  plan_out[0] = p.nsplit;
  plan_out[1] = p.items;
  plan_out[2] = p.grid;
  return MMG_OK;
}

extern "C" size_t mmg_nn_search_ws_bytes(int64_t n, int D, int64_t nq, int k) {
  if (!nn_shape_ok(n, D, k) || nq < 1 || nq >= (1ll << 31) || k > n) return 0;
  SearchWs w;
  return search_carve(nullptr, nq, k, nn_plan(n, nq), &w);
}

extern "C" int mmg_nn_search(const float* X, int64_t n, int D, int64_t ld_x, const float* Q, int64_t nq, int64_t ld_q, int k,
                             float* dist_out, int64_t ld_dist, int64_t* idx_out, int64_t ld_idx, void* ws, size_t ws_bytes,
                             void* stream) {
  const int self = Q == nullptr;
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31), "nn_search: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(D >= 1 && D <= MMG_NN_MAX_D, "nn_search: D %d outside [1, %d]", D, MMG_NN_MAX_D);
  MMG_CHECK_ARG(ld_x >= D, "nn_search: ld_x %lld < D %d", (long long)ld_x, D);
  MMG_CHECK_ARG(nq >= 1 && nq < (1ll << 31), "nn_search: nq %lld outside [1, 2^31)", (long long)nq);
  MMG_CHECK_ARG(!self || nq == n, "nn_search: self mode (Q = NULL) with nq %lld != n %lld", (long long)nq, (long long)n);
  MMG_CHECK_ARG(self || ld_q >= D, "nn_search: ld_q %lld < D %d", (long long)ld_q, D);
  MMG_CHECK_ARG(k >= 1 && k <= MMG_NN_MAX_K, "nn_search: k %d outside [1, %d]", k, MMG_NN_MAX_K);
  MMG_CHECK_ARG(k <= n - self, "nn_search: k %d exceeds the %lld candidates of a query", k, (long long)(n - self));
  MMG_CHECK_ARG(ld_dist >= k && ld_idx >= k, "nn_search: ld_dist %lld or ld_idx %lld < k %d", (long long)ld_dist,
                (long long)ld_idx, k);
  MMG_CHECK_ARG(X && dist_out && idx_out, "nn_search: null pointer (X, dist_out, idx_out)");
  const NnPlan p = nn_plan(n, nq);
  SearchWs w;
  MMG_CHECK_WS("nn_search", search_carve(ws, nq, k, p, &w));
  hipStream_t st = (hipStream_t)stream;
  MMG_CHECK_HIP((MmgMaxLds<&k_nn_search, NN_LDS_MAX>::set()), "nn_search(attr)");
  const size_t lds = (size_t)NN_B * k * 12;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nq, D, k, 0, k_nn_search, dim3(p.grid), dim3(NN_NTHR), lds, st, X, n, D, ld_x,
             self ? X : Q, nq, self ? ld_x : ld_q, self, k, p.nsplit, p.tps, p.ntiles, p.items, dist_out, ld_dist, idx_out,
             ld_idx, w.part_s, w.part_j);
  MMG_CHECK_LAUNCH("nn_search");
  if (p.nsplit > 1) {
    const unsigned g = (unsigned)((nq + NN_NTHR / 64 - 1) / (NN_NTHR / 64));
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nq, p.nsplit, k, 1, k_nn_merge, dim3(g), dim3(NN_NTHR), 0, st, (const double*)w.part_s,
               (const int32_t*)w.part_j, nq, p.nsplit, k, dist_out, ld_dist, idx_out, ld_idx);
    MMG_CHECK_LAUNCH("nn_search(merge)");
  }
  return MMG_OK;
}

// nothing is kept between kernels today: the carver's slack alone
extern "C" size_t mmg_nn_rank_ws_bytes(int64_t n, int D, int k) {
  if (!nn_shape_ok(n, D, k)) return 0;
  return MmgCarver(nullptr).need();
}

extern "C" int mmg_nn_rank(const float* X, int64_t n, int D, int64_t ld_x, const int64_t* nbr, int64_t ld_nbr, int k,
                           int32_t* rank_out, int64_t ld_rank, int64_t* penalty_out, void* ws, size_t ws_bytes,
                           void* stream) {
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31), "nn_rank: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(D >= 1 && D <= MMG_NN_MAX_D, "nn_rank: D %d outside [1, %d]", D, MMG_NN_MAX_D);
  MMG_CHECK_ARG(ld_x >= D, "nn_rank: ld_x %lld < D %d", (long long)ld_x, D);
  MMG_CHECK_ARG(k >= 1 && k <= MMG_NN_MAX_K, "nn_rank: k %d outside [1, %d]", k, MMG_NN_MAX_K);
  MMG_CHECK_ARG(ld_nbr >= k, "nn_rank: ld_nbr %lld < k %d", (long long)ld_nbr, k);
  MMG_CHECK_ARG(!rank_out || ld_rank >= k, "nn_rank: ld_rank %lld < k %d", (long long)ld_rank, k);
  MMG_CHECK_ARG(X && nbr, "nn_rank: null pointer (X, nbr)");
  MMG_CHECK_ARG(rank_out || penalty_out, "nn_rank: neither rank_out nor penalty_out is given");
  MMG_CHECK_WS("nn_rank", MmgCarver(nullptr).need());
  hipStream_t st = (hipStream_t)stream;
  MMG_CHECK_HIP((MmgMaxLds<&k_nn_rank, NN_LDS_MAX>::set()), "nn_rank(attr)");
  if (penalty_out) MMG_CHECK_HIP(mmg_zero_async(penalty_out, sizeof(int64_t), st), "nn_rank(zero)");
  const int64_t nqb = (n + NN_B - 1) / NN_B, ntiles = (n + NN_T - 1) / NN_T;
  const unsigned grid = (unsigned)(nqb < MMG_NN_MAX_GRID ? nqb : MMG_NN_MAX_GRID);
  const size_t lds = (size_t)NN_B * k * 12;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 2, k_nn_rank, dim3(grid), dim3(NN_NTHR), lds, st, X, n, D, ld_x, nbr, ld_nbr, k, nqb,
             ntiles, rank_out, ld_rank, reinterpret_cast<unsigned long long*>(penalty_out));
  MMG_CHECK_LAUNCH("nn_rank");
  return MMG_OK;
}
