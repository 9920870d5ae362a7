// K-means (Lloyd) over fp32 rows X [n, D] with fp64 centres, and the cluster scores (include/mmgnn_cluster.h;
// mmgnn/cluster.py): what sklearn.cluster.KMeans(init=array, n_init=1, algorithm="lloyd") and
// sklearn.metrics.silhouette_samples compute, every result defined by a total order or a stated order of summation.
//   km_tile_dist   the tile machinery of nn_tile_dist (csrc/nn.hip) with the second operand fp32 rows or fp64 centres and
//                  the first one optionally gathered through a row list: a 256-thread workgroup owns 64 rows, stages 32
//                  columns of them and of 64 rows of the other side in LDS as doubles, every thread accumulates a 4 x 4
//                  patch, the 64 x 64 block of sums is left in LDS over the staging buffers.
//   k_km_assign    a workgroup strides over blocks of 64 rows; the centres stream through LDS in tiles of 64; per tile
//                  lane (row = lane % 16, quarter = lane / 16) of a wave scans 16 centres of its row, the quarters are
//                  merged by the key (s, c), and the tile's best is merged into the row's running minimum.
//   k_km_sums      grid = row ranges x 32-column chunks; thread (g = tid / 32, col = tid % 32) owns the slots (c, col)
//                  with c % 8 == g in registers and walks the staged rows in row order: one owner per slot, so the order
//                  of a sum is the row order.  The ranges' sums go to the workspace.
//   k_km_reloc     one workgroup: the counts, the empty clusters, and for each the next-largest key (min_s, row) by one
//                  pass over min_s per empty cluster (rare; no pass without one).
//   k_km_finish    one workgroup per cluster adds the ranges in range order, applies the relocation, divides, writes the
//                  centre and its squared shift; k_km_status adds the shifts in cluster order.
//   k_km_sil       the shape of k_nn_rank: a work item = (block of 64 query rows, candidate range); per tile the block of
//                  sums becomes square roots in place, and lane (row = lane % 16, q = lane / 16) of a wave adds the
//                  candidates whose label has label % 4 == q into the row's [k] table in LDS, candidates ascending.
//
// Built into libmmgnn_cluster.so beside libmmgnn.so and on top of it (mmg_set_error, the launch probe).
#include "common.h"
#include "../../include/mmgnn_cluster.h"
#include <math.h>

namespace {

constexpr int KM_NTHR = 256;
constexpr int KM_B = MMG_KM_ROW_TILE;              // rows of a workgroup's block = rows of the other side per tile
constexpr int KM_DC = 32;                          // columns per staged chunk
constexpr int KM_LD = KM_B + 1;                    // LDS row stride of the staging buffers and of the block of sums
constexpr int KM_ROWS_PER_WAVE = KM_B / (KM_NTHR / 64);
constexpr int KM_NONE = 0x7fffffff;
constexpr int KM_SIL_MIN_TILES = 4;                // a candidate range of the silhouette is at least this many tiles
constexpr int KM_SIL_MAX_SPLIT = 64;
constexpr int KM_SIL_LDS_MAX = KM_B * (MMG_KM_MAX_K + 1) * 8;
static_assert(KM_B == 64 && KM_NTHR == 256, "a thread owns a 4 x 4 patch of the 64 x 64 block; a wave spans a tile");
static_assert(2 * KM_DC * KM_LD >= KM_B * KM_LD, "the block of sums lies over the staging buffers");
static_assert(MMG_KM_MAX_K <= 128 && MMG_KM_MAX_D <= KM_NTHR, "a thread per cluster / per column in the small kernels");

struct KmPlan { int64_t ranges, rpr; unsigned grid_assign; };
inline KmPlan km_plan(int64_t n) {
  KmPlan p;
  const int64_t tiles = (n + KM_B - 1) / KM_B;
  const int64_t tpr = (tiles + MMG_KM_MAX_RANGES - 1) / MMG_KM_MAX_RANGES;
  p.rpr = tpr * KM_B;
  p.ranges = (n + p.rpr - 1) / p.rpr;
  p.grid_assign = (unsigned)(tiles < MMG_KM_MAX_GRID ? tiles : MMG_KM_MAX_GRID);
  return p;
}
struct SilPlan { int64_t nqb, ntiles, tps, items; int nsplit; unsigned grid; };
inline SilPlan sil_plan(int64_t n, int64_t nq) {
  SilPlan p;
  p.nqb = (nq + KM_B - 1) / KM_B;
  p.ntiles = (n + KM_B - 1) / KM_B;
  const int64_t want = p.nqb >= MMG_KM_MAX_GRID ? 1 : (MMG_KM_MAX_GRID + p.nqb - 1) / p.nqb;
  int64_t most = p.ntiles / KM_SIL_MIN_TILES;
  most = most < 1 ? 1 : most > KM_SIL_MAX_SPLIT ? KM_SIL_MAX_SPLIT : most;
  const int64_t ns = want < most ? want : most;
  p.tps = (p.ntiles + ns - 1) / ns;
  p.nsplit = (int)((p.ntiles + p.tps - 1) / p.tps);            // no empty range
  p.items = p.nqb * p.nsplit;
  p.grid = (unsigned)(p.items < MMG_KM_MAX_GRID ? p.items : MMG_KM_MAX_GRID);
  return p;
}

__device__ __forceinline__ bool key_less(double sa, int ja, double sb, int jb) { return sa < sb || (sa == sb && ja < jb); }

// sm[r * KM_LD + c] = s(row a(r), row b0 + c of B) for the 64 x 64 block.  a(r) = arow[r] (an LDS list, -1: no row)
// when given, a0 + r otherwise; rows past na / nb are zeros, their sums never used.  Begins and ends with a barrier.
template <class TB>
__device__ __forceinline__ void km_tile_dist(const float* __restrict__ A, int64_t ld_a, int64_t na, int64_t a0,
                                             const int* arow, const TB* __restrict__ B, int64_t ld_b, int64_t nb,
                                             int64_t b0, int D, double* __restrict__ sm) {
  double(*xi)[KM_LD] = reinterpret_cast<double(*)[KM_LD]>(sm);
  double(*xj)[KM_LD] = reinterpret_cast<double(*)[KM_LD]>(sm + KM_DC * KM_LD);
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  for (int d0 = 0; d0 < D; d0 += KM_DC) {
    const int cw = D - d0 < KM_DC ? D - d0 : KM_DC;
    __syncthreads();                                 // the previous chunk (or block of sums) has been consumed
    for (int e = tid; e < KM_B * KM_DC; e += KM_NTHR) {
      const int r = e / KM_DC, c = e % KM_DC;
      if (c >= cw) continue;
      int64_t ri = a0 + r;
      if (arow) ri = arow[r];
      const int64_t rj = b0 + r;
      xi[c][r] = (ri >= 0 && ri < na) ? (double)A[ri * ld_a + d0 + c] : 0.0;
      xj[c][r] = rj < nb ? (double)B[rj * ld_b + d0 + c] : 0.0;
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
    for (int q = 0; q < 4; ++q) sm[(4 * ty + p) * KM_LD + 4 * tx + q] = isfinite(acc[p][q]) ? acc[p][q] : (double)INFINITY;
  __syncthreads();
}

__global__ __launch_bounds__(KM_NTHR) void k_km_assign(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                       const double* __restrict__ C, int k, const int32_t* prev,
                                                       int32_t* labels, double* __restrict__ min_s,
                                                       unsigned long long* __restrict__ changed, int64_t nrb) {
  __shared__ double sm[2 * KM_DC * KM_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int nchanged = 0;
  for (int64_t rb = blockIdx.x; rb < nrb; rb += gridDim.x) {
    const int64_t i0 = rb * KM_B;
    double best_s = (double)INFINITY;                // the running minimum of row lane % 16 of the wave
    int best_c = KM_NONE;
    for (int c0 = 0; c0 < k; c0 += KM_B) {
      km_tile_dist<double>(X, ld_x, n, i0, nullptr, C, (int64_t)D, (int64_t)k, (int64_t)c0, D, sm);
      {
        // lane (row = lane % 16, quarter = lane / 16) scans 16 centres of its row in ascending order, the four quarters
        // are merged by key: a total order, so the split changes nothing
        const int r = wave * KM_ROWS_PER_WAVE + (lane & 15);
        const int cb = (lane >> 4) * 16;
        double ms = (double)INFINITY;
        int mc = KM_NONE;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int c = c0 + cb + u;
          const double v = sm[r * KM_LD + cb + u];
          if (c < k && key_less(v, c, ms, mc)) { ms = v; mc = c; }
        }
#pragma unroll
        for (int o = 16; o <= 32; o <<= 1) {
          const double os = __shfl_xor(ms, o, 64);
          const int oc = __shfl_xor(mc, o, 64);
          if (key_less(os, oc, ms, mc)) { ms = os; mc = oc; }
        }
        if (key_less(ms, mc, best_s, best_c)) { best_s = ms; best_c = mc; }
      }
    }
    const double ws_ = best_s;                       // lanes 0..15 hold rows 0..15 of the wave (every quarter agrees)
    const int wc = best_c;                           // (k >= 1: the key (+inf, 0) is below the initial (+inf, none))
    const int64_t i = i0 + wave * KM_ROWS_PER_WAVE + lane;
    if (lane < KM_ROWS_PER_WAVE && i < n) {
      const int before = prev ? prev[i] : -1;        // (prev may be labels: read before the write, by the same lane)
      labels[i] = wc;
      min_s[i] = ws_;
      nchanged += before != wc ? 1 : 0;
    }
  }
  if (changed) {
    nchanged = wave_sum_i(nchanged);
    if (lane == 0 && nchanged != 0) atomicAdd(changed, (unsigned long long)nchanged);
  }
}

// a thread per row, the fma chain of the definition
__global__ __launch_bounds__(KM_NTHR) void k_km_label_dist(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                           const double* __restrict__ C, int k,
                                                           const int32_t* __restrict__ labels, double* __restrict__ out_s) {
  const int64_t i = (int64_t)blockIdx.x * KM_NTHR + threadIdx.x;
  if (i >= n) return;
  const int lab = labels[i];
  double acc = (double)INFINITY;
  if ((unsigned)lab < (unsigned)k) {
    const float* __restrict__ x = X + i * ld_x;
    const double* __restrict__ c = C + (size_t)lab * D;
    acc = 0.0;
    for (int d = 0; d < D; ++d) {
      const double df = (double)x[d] - c[d];
      acc = fma(df, df, acc);
    }
  }
  out_s[i] = isfinite(acc) ? acc : (double)INFINITY;
}

// KPT = the clusters of a thread: thread (g = tid / 32, col = tid % 32) owns the slots (c, col) with c = g + 8 j, j < KPT, in
// registers.  Every thread walks every staged row; a row that is not the slot's is skipped or adds +0.0, which changes no sum.  The
// next tile's rows are on their way from memory while the current one is walked.
template <int KPT>
__global__ __launch_bounds__(KM_NTHR) void k_km_sums(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                     const int32_t* __restrict__ labels, int k, int64_t rpr,
                                                     double* __restrict__ part_sum, int32_t* __restrict__ part_cnt) {
  constexpr int PER = KM_B * KM_DC / KM_NTHR;        // staged values per thread and tile
  __shared__ float xs[KM_B][KM_DC + 1];
  __shared__ int ls[KM_B];
  const int tid = threadIdx.x, col = tid & 31, g = tid >> 5;
  const int64_t range = blockIdx.x;
  const int d0 = (int)blockIdx.y * KM_DC;
  const int cw = D - d0 < KM_DC ? D - d0 : KM_DC;
  const int64_t r0 = range * rpr, r1 = r0 + rpr < n ? r0 + rpr : n;
  double acc[KPT];
  int cnt[KPT];
#pragma unroll
  for (int j = 0; j < KPT; ++j) { acc[j] = 0.0; cnt[j] = 0; }
  float pre[PER];
  int pre_l = -1;
  auto fetch = [&](int64_t t0) {
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * KM_NTHR, r = e / KM_DC, c = e % KM_DC;
      const int64_t row = t0 + r;
      pre[u] = (row < r1 && c < cw) ? X[row * ld_x + d0 + c] : 0.f;
    }
    pre_l = (tid < KM_B && t0 + tid < r1) ? labels[t0 + tid] : -1;
  };
  fetch(r0);
  for (int64_t t0 = r0; t0 < r1; t0 += KM_B) {
    __syncthreads();                                 // the previous tile has been walked
#pragma unroll
    for (int u = 0; u < PER; ++u) {
      const int e = tid + u * KM_NTHR;
      xs[e / KM_DC][e % KM_DC] = pre[u];
    }
    if (tid < KM_B) ls[tid] = pre_l;
    __syncthreads();
    if (t0 + KM_B < r1) fetch(t0 + KM_B);
#pragma unroll 8
    for (int r = 0; r < KM_B; ++r) {
      const int lab = ls[r];
      const double x = (double)xs[r][col];
      if constexpr (KPT == 1) {
        const bool hit = lab == g;
        acc[0] += hit ? x : 0.0;
        cnt[0] += hit ? 1 : 0;
      } else if ((lab & 7) == g) {                   // uniform over the 32 lanes of a group: one row in eight
        const int jj = lab >> 3;
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
          const bool hit = jj == j;
          acc[j] += hit ? x : 0.0;
          cnt[j] += hit ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int c = g + 8 * j;
    if (c < k) {
      if (col < cw) part_sum[((size_t)range * k + c) * D + d0 + col] = acc[j];
      if (blockIdx.y == 0 && col == 0) part_cnt[(size_t)range * k + c] = cnt[j];
    }
  }
}

struct RelocWs { int32_t* cnt; int32_t* m; int32_t* row; int32_t* to; int32_t* from; };

__global__ __launch_bounds__(KM_NTHR) void k_km_reloc(const int32_t* __restrict__ labels, const double* __restrict__ min_s,
                                                      int64_t n, int k, int64_t ranges,
                                                      const int32_t* __restrict__ part_cnt, RelocWs w,
                                                      int32_t* __restrict__ counts, int64_t* __restrict__ reloc_rows) {
  __shared__ int cnt[MMG_KM_MAX_K];
  __shared__ int empt[MMG_KM_MAX_K];
  __shared__ int m_sh;
  __shared__ double red_s[KM_NTHR];
  __shared__ int red_j[KM_NTHR];
  const int tid = threadIdx.x;
  if (tid < k) {
    int c = 0;
    for (int64_t r = 0; r < ranges; ++r) c += part_cnt[(size_t)r * k + tid];
    cnt[tid] = c;
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int c = 0; c < k; ++c)
      if (cnt[c] == 0) empt[m++] = c;
    m_sh = m;
  }
  __syncthreads();
  const int m = m_sh;
  double prev_s = 0.0;
  int prev_j = -1;
  for (int e = 0; e < m; ++e) {                      // the e-th largest key (min_s descending, row ascending)
    double bs = -1.0;                                // below every sum
    int bj = -1;
    for (int64_t i = tid; i < n; i += KM_NTHR) {
      double s = min_s[i];
      s = (s >= 0.0 && isfinite(s)) ? s : (double)INFINITY;
      const bool after = e == 0 || s < prev_s || (s == prev_s && (int)i > prev_j);
      if (after && (s > bs || (s == bs && (int)i < bj))) { bs = s; bj = (int)i; }
    }
    red_s[tid] = bs;
    red_j[tid] = bj;
    __syncthreads();
    for (int o = KM_NTHR / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const double os = red_s[tid + o];
        const int oj = red_j[tid + o];
        if (oj >= 0 && (red_j[tid] < 0 || os > red_s[tid] || (os == red_s[tid] && oj < red_j[tid]))) {
          red_s[tid] = os;
          red_j[tid] = oj;
        }
      }
      __syncthreads();
    }
    prev_s = red_s[0];
    prev_j = red_j[0];
    if (tid == 0) {
      int from = -1;
      if (prev_j >= 0) {
        from = labels[prev_j];
        if ((unsigned)from < (unsigned)k) cnt[from] -= 1; else from = -1;
        cnt[empt[e]] = 1;
      }
      w.row[e] = prev_j;
      w.to[e] = empt[e];
      w.from[e] = from;
    }
    __syncthreads();
  }
  if (tid < k) {
    w.cnt[tid] = cnt[tid];
    counts[tid] = cnt[tid];
    if (reloc_rows) reloc_rows[tid] = tid < m ? (int64_t)w.row[tid] : -1;      // (w.row[tid] was written before the barrier)
  }
  if (tid == 0) w.m[0] = m;
}

__global__ __launch_bounds__(KM_NTHR) void k_km_finish(const float* __restrict__ X, int D, int64_t ld_x, int k, int64_t ranges,
                                                       const double* __restrict__ part_sum, RelocWs w,
                                                       const double* C_old, double* C_new, double* __restrict__ shift_part) {
  __shared__ double sq[MMG_KM_MAX_D];
  const int c = blockIdx.x, d = threadIdx.x;
  if (d < D) {
    double sum = 0.0;
    for (int64_t r = 0; r < ranges; ++r) sum += part_sum[((size_t)r * k + c) * D + d];
    const int m = w.m[0];
    for (int e = 0; e < m; ++e) {
      const int row = w.row[e];
      if (row < 0) continue;
      if (w.from[e] == c) sum -= (double)X[(int64_t)row * ld_x + d];
      if (w.to[e] == c) sum += (double)X[(int64_t)row * ld_x + d];
    }
    const int cn = w.cnt[c];
    const double old = C_old[(size_t)c * D + d];     // (C_new may be C_old: read before the write, by the same thread)
    const double nw = cn > 0 ? sum / (double)cn : old;
    C_new[(size_t)c * D + d] = nw;
    const double df = nw - old;
    sq[d] = df * df;
  }
  __syncthreads();
  if (d == 0) {
    double t = 0.0;
    for (int e = 0; e < D; ++e) t += sq[e];
    shift_part[c] = t;
  }
}

__global__ __launch_bounds__(64) void k_km_status(const double* __restrict__ shift_part, int k, const int32_t* __restrict__ m,
                                                  const long long* __restrict__ changed, double* __restrict__ status) {
  if (threadIdx.x != 0) return;
  double t = 0.0;
  for (int c = 0; c < k; ++c) t += shift_part[c];
  status[0] = changed ? (double)changed[0] : 0.0;
  status[1] = t;
  status[2] = (double)m[0];
}

__global__ __launch_bounds__(KM_NTHR) void k_km_colstats(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                         int64_t rpr, double* __restrict__ part) {
  __shared__ double red[2][8][KM_DC];
  const int tid = threadIdx.x, col = tid & 31, g = tid >> 5;
  const int64_t range = blockIdx.x;
  const int d = (int)blockIdx.y * KM_DC + col;
  const int64_t r0 = range * rpr, r1 = r0 + rpr < n ? r0 + rpr : n;
  double s1 = 0.0, s2 = 0.0;
  if (d < D)
    for (int64_t row = r0 + g; row < r1; row += 8) {           // rpr is a multiple of 8: row % 8 == g
      const double x = (double)X[row * ld_x + d];
      s1 += x;
      s2 = fma(x, x, s2);                                      // the product of two widened fp32 values is exact
    }
  red[0][g][col] = s1;
  red[1][g][col] = s2;
  __syncthreads();
  if (g == 0 && d < D) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < 8; ++q) { a += red[0][q][col]; b += red[1][q][col]; }
    part[((size_t)range * 2 + 0) * D + d] = a;
    part[((size_t)range * 2 + 1) * D + d] = b;
  }
}

__global__ __launch_bounds__(KM_NTHR) void k_km_colstats_fin(const double* __restrict__ part, int64_t n, int D, int64_t ranges,
                                                             double* __restrict__ col_mean, double* __restrict__ mean_var) {
  __shared__ double var[MMG_KM_MAX_D];
  const int d = threadIdx.x;
  if (d < D) {
    double a = 0.0, b = 0.0;
    for (int64_t r = 0; r < ranges; ++r) { a += part[((size_t)r * 2 + 0) * D + d]; b += part[((size_t)r * 2 + 1) * D + d]; }
    const double mu = a / (double)n;
    const double v = b / (double)n - mu * mu;
    col_mean[d] = mu;
    var[d] = v > 0.0 ? v : 0.0;
  }
  __syncthreads();
  if (d == 0) {
    double t = 0.0;
    for (int e = 0; e < D; ++e) t += var[e];
    mean_var[0] = t / (double)D;
  }
}

__global__ __launch_bounds__(KM_NTHR) void k_km_scores(const int32_t* __restrict__ labels, const double* __restrict__ min_s,
                                                       int64_t n, int k, int64_t rpr, double* __restrict__ part_sd,
                                                       int32_t* __restrict__ part_cnt, double* __restrict__ part_in) {
  __shared__ int lab[KM_NTHR];
  __shared__ double ms[KM_NTHR];
  __shared__ double rt[KM_NTHR];
  const int tid = threadIdx.x;
  const int64_t range = blockIdx.x;
  const int64_t r0 = range * rpr, r1 = r0 + rpr < n ? r0 + rpr : n;
  double acc = 0.0;
  int cnt = 0;
  for (int64_t t0 = r0; t0 < r1; t0 += KM_NTHR) {
    __syncthreads();
    const int64_t row = t0 + tid;
    const int lim = r1 - t0 < KM_NTHR ? (int)(r1 - t0) : KM_NTHR;
    if (tid < lim) {
      const double s = min_s[row];
      lab[tid] = labels[row];
      ms[tid] = s;
      rt[tid] = sqrt(s);
    }
    __syncthreads();
    if (tid < k) {                                   // the owner of cluster tid: its rows in row order
      for (int r = 0; r < lim; ++r)
        if (lab[r] == tid) { acc += rt[r]; ++cnt; }
    } else if (tid == MMG_KM_MAX_K) {                // the owner of the inertia
      for (int r = 0; r < lim; ++r) acc += ms[r];
    }
  }
  if (tid < k) {
    part_sd[(size_t)range * k + tid] = acc;
    part_cnt[(size_t)range * k + tid] = cnt;
  } else if (tid == MMG_KM_MAX_K) {
    part_in[range] = acc;
  }
}

__global__ __launch_bounds__(KM_NTHR) void k_km_scores_fin(const double* __restrict__ part_sd, const int32_t* __restrict__ part_cnt,
                                                           const double* __restrict__ part_in, int k, int64_t ranges,
                                                           double* __restrict__ inertia, double* __restrict__ sdist,
                                                           int32_t* __restrict__ counts) {
  const int tid = threadIdx.x;
  if (tid < k) {
    double a = 0.0;
    int c = 0;
    for (int64_t r = 0; r < ranges; ++r) { a += part_sd[(size_t)r * k + tid]; c += part_cnt[(size_t)r * k + tid]; }
    sdist[tid] = a;
    counts[tid] = c;
  } else if (tid == MMG_KM_MAX_K) {
    double a = 0.0;
    for (int64_t r = 0; r < ranges; ++r) a += part_in[r];
    inertia[0] = a;
  }
}

__global__ __launch_bounds__(KM_NTHR) void k_km_sil(const float* __restrict__ X, int64_t n, int D, int64_t ld_x,
                                                    const int32_t* __restrict__ labels, int k,
                                                    const int32_t* __restrict__ queries, int64_t nq, int nsplit, int64_t tps,
                                                    int64_t ntiles, int64_t items, double* __restrict__ part) {
  __shared__ double sm[2 * KM_DC * KM_LD];
  __shared__ int tl[KM_B];
  __shared__ int qrow[KM_B];
  extern __shared__ double km_dyn[];                 // [KM_B][k + 1]: S(row, cluster)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ks = k + 1;
  const int myr = wave * KM_ROWS_PER_WAVE + (lane & 15), myq = lane >> 4;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t qb = item / nsplit, q0 = qb * KM_B;
    const int sp = (int)(item - qb * nsplit);
    const int64_t t0 = sp * tps, t1 = t0 + tps < ntiles ? t0 + tps : ntiles;
    __syncthreads();                                 // the previous item's table has been written out
    for (int e = tid; e < KM_B * ks; e += KM_NTHR) km_dyn[e] = 0.0;
    if (tid < KM_B) {
      int64_t i = -1;
      if (q0 + tid < nq) i = queries ? (int64_t)queries[q0 + tid] : q0 + tid;
      qrow[tid] = (i >= 0 && i < n) ? (int)i : -1;   // an id outside [0, n) is never used as an address
    }
    for (int64_t t = t0; t < t1; ++t) {
      const int64_t j0 = t * KM_B;
      km_tile_dist<float>(X, ld_x, n, 0, qrow, X, ld_x, n, j0, D, sm);      // (its barriers order qrow and the table too)
      for (int e = tid; e < KM_B * KM_B; e += KM_NTHR) {
        const int r = e >> 6, c = e & 63;
        const double v = sm[r * KM_LD + c];
        sm[r * KM_LD + c] = (j0 + c == (int64_t)qrow[r]) ? 0.0 : sqrt(v);
      }
      if (tid < KM_B) tl[tid] = j0 + tid < n ? labels[j0 + tid] : -1;
      __syncthreads();
      for (int c = 0; c < KM_B; ++c) {
        const int lab = tl[c];
        if ((unsigned)lab < (unsigned)k && (lab & 3) == myq) km_dyn[myr * ks + lab] += sm[myr * KM_LD + c];
      }
    }
    __syncthreads();
    for (int e = tid; e < KM_B * k; e += KM_NTHR) {
      const int r = e / k, c = e - r * k;
      const int64_t q = q0 + r;
      if (q < nq) part[((size_t)q * nsplit + sp) * k + c] = km_dyn[r * ks + c];
    }
  }
}

// one wave per query: lane l holds clusters l and l + 64
__global__ __launch_bounds__(KM_NTHR) void k_km_sil_fin(const double* __restrict__ part, const int32_t* __restrict__ labels,
                                                        const int32_t* __restrict__ counts, int k, int64_t n,
                                                        const int32_t* __restrict__ queries, int64_t nq, int nsplit,
                                                        double* __restrict__ sil) {
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * (KM_NTHR / 64) + (threadIdx.x >> 6);
  if (q >= nq) return;                               // wave-uniform
  const int64_t i = queries ? (int64_t)queries[q] : q;
  int own = -1;
  if (i >= 0 && i < n) own = labels[i];
  if ((unsigned)own >= (unsigned)k) {                // wave-uniform: no such row or label
    if (lane == 0) sil[q] = 0.0;
    return;
  }
  double S[2];
  int cn[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    double a = 0.0;
    if (c < k)
      for (int sp = 0; sp < nsplit; ++sp) a += part[((size_t)q * nsplit + sp) * k + c];
    S[h] = a;
    cn[h] = c < k ? counts[c] : 0;
  }
  const double own_s = __shfl(own < 64 ? S[0] : S[1], own & 63, 64);
  const int own_n = __shfl(own < 64 ? cn[0] : cn[1], own & 63, 64);
  double b = (double)INFINITY;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int c = lane + 64 * h;
    if (c < k && c != own && cn[h] > 0) b = fmin(b, S[h] / (double)cn[h]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) b = fmin(b, __shfl_xor(b, o, 64));
  if (lane == 0) {
    double v = 0.0;
    if (own_n > 1) {
      const double a = own_s / (double)(own_n - 1);
      const double den = a > b ? a : b;
      if (den > 0.0 && isfinite(den)) v = (b - a) / den;
    }
    sil[q] = v;
  }
}

__global__ __launch_bounds__(KM_NTHR) void k_km_mean(const double* __restrict__ v, int64_t n, double* __restrict__ out) {
  __shared__ double red[KM_NTHR];
  const int tid = threadIdx.x;
  double a = 0.0;
  for (int64_t i = tid; i < n; i += KM_NTHR) a += v[i];
  red[tid] = a;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
    for (int e = 0; e < KM_NTHR; ++e) t += red[e];
    out[0] = t / (double)n;
  }
}

inline bool km_shape_ok(int64_t n, int D, int k) {
  return n >= 1 && n < (1ll << 31) && D >= 1 && D <= MMG_KM_MAX_D && k >= 1 && k <= MMG_KM_MAX_K && k <= n;
}
struct UpdateWs { double* part_sum; int32_t* part_cnt; RelocWs rw; double* shift_part; };
size_t update_carve(void* ws, int D, int k, const KmPlan& p, UpdateWs* w) {
  MmgCarver c(ws);
  w->part_sum = c.take<double>((size_t)p.ranges * k * D);
  w->part_cnt = c.take<int32_t>((size_t)p.ranges * k);
  w->rw.cnt = c.take<int32_t>(k);
  w->rw.m = c.take<int32_t>(1);
  w->rw.row = c.take<int32_t>(k);
  w->rw.to = c.take<int32_t>(k);
  w->rw.from = c.take<int32_t>(k);
  w->shift_part = c.take<double>(k);
  return c.need();
}
struct ScoresWs { double* part_sd; int32_t* part_cnt; double* part_in; };
size_t scores_carve(void* ws, int k, const KmPlan& p, ScoresWs* w) {
  MmgCarver c(ws);
  w->part_sd = c.take<double>((size_t)p.ranges * k);
  w->part_cnt = c.take<int32_t>((size_t)p.ranges * k);
  w->part_in = c.take<double>((size_t)p.ranges);
  return c.need();
}
size_t colstats_carve(void* ws, int D, const KmPlan& p, double** part) {
  MmgCarver c(ws);
  *part = c.take<double>((size_t)p.ranges * 2 * D);
  return c.need();
}
size_t sil_carve(void* ws, int64_t nq, int k, const SilPlan& p, double** part) {
  MmgCarver c(ws);
  *part = c.take<double>((size_t)nq * (size_t)p.nsplit * (size_t)k);
  return c.need();
}

}  // namespace

#define KM_CHECK_X(name)                                                                                   \
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31), name ": n %lld outside [1, 2^31)", (long long)n);               \
  MMG_CHECK_ARG(D >= 1 && D <= MMG_KM_MAX_D, name ": D %d outside [1, %d]", D, MMG_KM_MAX_D);              \
  MMG_CHECK_ARG(ld_x >= D, name ": ld_x %lld < D %d", (long long)ld_x, D)
#define KM_CHECK_K(name, lo)                                                                               \
  MMG_CHECK_ARG(k >= lo && k <= MMG_KM_MAX_K, name ": k %d outside [%d, %d]", k, lo, MMG_KM_MAX_K);        \
  MMG_CHECK_ARG(k <= n, name ": k %d exceeds the %lld rows", k, (long long)n)

extern "C" int mmg_km_plan(int64_t n, int64_t* plan_out) {
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31), "km_plan: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(plan_out, "km_plan: null pointer (plan_out)");
  const KmPlan p = km_plan(n);
  plan_out[0] = p.ranges;
  plan_out[1] = p.rpr;
  plan_out[2] = p.grid_assign;
  return MMG_OK;
}

extern "C" int mmg_km_sil_plan(int64_t n, int64_t nq, int64_t* plan_out) {
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31) && nq >= 1 && nq <= n, "km_sil_plan: n %lld outside [1, 2^31) or nq %lld outside [1, n]",
                (long long)n, (long long)nq);
  MMG_CHECK_ARG(plan_out, "km_sil_plan: null pointer (plan_out)");
  const SilPlan p = sil_plan(n, nq);
  plan_out[0] = p.nsplit;
  plan_out[1] = p.items;
  plan_out[2] = p.grid;
  return MMG_OK;
}

// nothing is kept between kernels: the carver's slack alone
extern "C" size_t mmg_km_assign_ws_bytes(int64_t n, int D, int k) {
  if (!km_shape_ok(n, D, k)) return 0;
  return MmgCarver(nullptr).need();
}

extern "C" int mmg_km_assign(const float* X, int64_t n, int D, int64_t ld_x, const double* C, int k, const int32_t* prev_labels,
                             int32_t* labels, double* min_s, int64_t* changed, void* ws, size_t ws_bytes, void* stream) {
  KM_CHECK_X("km_assign");
  KM_CHECK_K("km_assign", 1);
  MMG_CHECK_ARG(X && C && labels && min_s, "km_assign: null pointer (X, C, labels, min_s)");
  MMG_CHECK_WS("km_assign", MmgCarver(nullptr).need());
  hipStream_t st = (hipStream_t)stream;
  const KmPlan p = km_plan(n);
  if (changed) MMG_CHECK_HIP(mmg_zero_async(changed, sizeof(int64_t), st), "km_assign(zero)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 0, k_km_assign, dim3(p.grid_assign), dim3(KM_NTHR), 0, st, X, n, D, ld_x, C, k,
             prev_labels, labels, min_s, reinterpret_cast<unsigned long long*>(changed), (n + KM_B - 1) / KM_B);
  MMG_CHECK_LAUNCH("km_assign");
  return MMG_OK;
}

extern "C" int mmg_km_label_dist(const float* X, int64_t n, int D, int64_t ld_x, const double* C, int k, const int32_t* labels,
                                 double* out_s, void* stream) {
  KM_CHECK_X("km_label_dist");
  KM_CHECK_K("km_label_dist", 1);
  MMG_CHECK_ARG(X && C && labels && out_s, "km_label_dist: null pointer (X, C, labels, out_s)");
  hipStream_t st = (hipStream_t)stream;
  const unsigned g = (unsigned)((n + KM_NTHR - 1) / KM_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 12, k_km_label_dist, dim3(g), dim3(KM_NTHR), 0, st, X, n, D, ld_x, C, k, labels, out_s);
  MMG_CHECK_LAUNCH("km_label_dist");
  return MMG_OK;
}

extern "C" size_t mmg_km_update_ws_bytes(int64_t n, int D, int k) {
  if (!km_shape_ok(n, D, k)) return 0;
  UpdateWs w;
  return update_carve(nullptr, D, k, km_plan(n), &w);
}

extern "C" int mmg_km_update(const float* X, int64_t n, int D, int64_t ld_x, const int32_t* labels, const double* min_s,
                             const double* C_old, int k, double* C_new, int32_t* counts, const int64_t* changed,
                             double* status, int64_t* reloc_rows, void* ws, size_t ws_bytes, void* stream) {
  KM_CHECK_X("km_update");
  KM_CHECK_K("km_update", 1);
  MMG_CHECK_ARG(X && labels && min_s && C_old && C_new && counts && status,
                "km_update: null pointer (X, labels, min_s, C_old, C_new, counts, status)");
  const KmPlan p = km_plan(n);
  UpdateWs w;
  MMG_CHECK_WS("km_update", update_carve(ws, D, k, p, &w));
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)p.ranges, (unsigned)((D + KM_DC - 1) / KM_DC));
#define KM_SUMS(KPT)                                                                                                   \
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 1, k_km_sums<KPT>, g, dim3(KM_NTHR), 0, st, X, n, D, ld_x, labels, k, p.rpr, \
             w.part_sum, w.part_cnt)
  if (k <= 8) KM_SUMS(1);
  else if (k <= 16) KM_SUMS(2);
  else if (k <= 32) KM_SUMS(4);
  else if (k <= 64) KM_SUMS(8);
  else KM_SUMS(16);
#undef KM_SUMS
  MMG_CHECK_LAUNCH("km_update(sums)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 2, k_km_reloc, dim3(1), dim3(KM_NTHR), 0, st, labels, min_s, n, k, p.ranges,
             (const int32_t*)w.part_cnt, w.rw, counts, reloc_rows);
  MMG_CHECK_LAUNCH("km_update(reloc)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 3, k_km_finish, dim3((unsigned)k), dim3(KM_NTHR), 0, st, X, D, ld_x, k, p.ranges,
             (const double*)w.part_sum, w.rw, C_old, C_new, w.shift_part);
  MMG_CHECK_LAUNCH("km_update(finish)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 4, k_km_status, dim3(1), dim3(64), 0, st, (const double*)w.shift_part, k,
             (const int32_t*)w.rw.m, reinterpret_cast<const long long*>(changed), status);
  MMG_CHECK_LAUNCH("km_update(status)");
  return MMG_OK;
}

extern "C" size_t mmg_km_colstats_ws_bytes(int64_t n, int D) {
  if (!km_shape_ok(n, D, 1)) return 0;
  double* part;
  return colstats_carve(nullptr, D, km_plan(n), &part);
}

extern "C" int mmg_km_colstats(const float* X, int64_t n, int D, int64_t ld_x, double* col_mean, double* mean_var, void* ws,
                               size_t ws_bytes, void* stream) {
  KM_CHECK_X("km_colstats");
  MMG_CHECK_ARG(X && col_mean && mean_var, "km_colstats: null pointer (X, col_mean, mean_var)");
  const KmPlan p = km_plan(n);
  double* part;
  MMG_CHECK_WS("km_colstats", colstats_carve(ws, D, p, &part));
  hipStream_t st = (hipStream_t)stream;
  const dim3 g((unsigned)p.ranges, (unsigned)((D + KM_DC - 1) / KM_DC));
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, 0, 5, k_km_colstats, g, dim3(KM_NTHR), 0, st, X, n, D, ld_x, p.rpr, part);
  MMG_CHECK_LAUNCH("km_colstats");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, 0, 6, k_km_colstats_fin, dim3(1), dim3(KM_NTHR), 0, st, (const double*)part, n, D,
             p.ranges, col_mean, mean_var);
  MMG_CHECK_LAUNCH("km_colstats(fin)");
  return MMG_OK;
}

extern "C" size_t mmg_km_scores_ws_bytes(int64_t n, int k) {
  if (!km_shape_ok(n, 1, k)) return 0;
  ScoresWs w;
  return scores_carve(nullptr, k, km_plan(n), &w);
}

extern "C" int mmg_km_scores(const int32_t* labels, const double* min_s, int64_t n, int k, double* inertia, double* sdist,
                             int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 1 && n < (1ll << 31), "km_scores: n %lld outside [1, 2^31)", (long long)n);
  KM_CHECK_K("km_scores", 1);
  MMG_CHECK_ARG(labels && min_s && inertia && sdist && counts, "km_scores: null pointer (labels, min_s, inertia, sdist, counts)");
  const KmPlan p = km_plan(n);
  ScoresWs w;
  MMG_CHECK_WS("km_scores", scores_carve(ws, k, p, &w));
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, k, 7, k_km_scores, dim3((unsigned)p.ranges), dim3(KM_NTHR), 0, st, labels, min_s, n, k,
             p.rpr, w.part_sd, w.part_cnt, w.part_in);
  MMG_CHECK_LAUNCH("km_scores");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, k, 8, k_km_scores_fin, dim3(1), dim3(KM_NTHR), 0, st, (const double*)w.part_sd,
             (const int32_t*)w.part_cnt, (const double*)w.part_in, k, p.ranges, inertia, sdist, counts);
  MMG_CHECK_LAUNCH("km_scores(fin)");
  return MMG_OK;
}

extern "C" size_t mmg_km_silhouette_ws_bytes(int64_t n, int D, int64_t nq, int k) {
  if (!km_shape_ok(n, D, k) || k < 2 || nq < 1 || nq > n) return 0;
  double* part;
  return sil_carve(nullptr, nq, k, sil_plan(n, nq), &part);
}

extern "C" int mmg_km_silhouette(const float* X, int64_t n, int D, int64_t ld_x, const int32_t* labels, const int32_t* counts,
                                 int k, const int32_t* queries, int64_t nq, double* sil, double* sil_mean, void* ws,
                                 size_t ws_bytes, void* stream) {
  KM_CHECK_X("km_silhouette");
  KM_CHECK_K("km_silhouette", 2);
  MMG_CHECK_ARG(nq >= 1 && nq <= n, "km_silhouette: nq %lld outside [1, n = %lld]", (long long)nq, (long long)n);
  MMG_CHECK_ARG(queries || nq == n, "km_silhouette: queries = NULL with nq %lld != n %lld", (long long)nq, (long long)n);
  MMG_CHECK_ARG(X && labels && counts && sil, "km_silhouette: null pointer (X, labels, counts, sil)");
  const SilPlan p = sil_plan(n, nq);
  double* part;
  MMG_CHECK_WS("km_silhouette", sil_carve(ws, nq, k, p, &part));
  hipStream_t st = (hipStream_t)stream;
  MMG_CHECK_HIP((MmgMaxLds<&k_km_sil, KM_SIL_LDS_MAX>::set()), "km_silhouette(attr)");
  const size_t lds = (size_t)KM_B * (k + 1) * 8;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nq, D, k, 9, k_km_sil, dim3(p.grid), dim3(KM_NTHR), lds, st, X, n, D, ld_x, labels, k, queries,
             nq, p.nsplit, p.tps, p.ntiles, p.items, part);
  MMG_CHECK_LAUNCH("km_silhouette");
  const unsigned g = (unsigned)((nq + KM_NTHR / 64 - 1) / (KM_NTHR / 64));
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nq, p.nsplit, k, 10, k_km_sil_fin, dim3(g), dim3(KM_NTHR), 0, st, (const double*)part, labels,
             counts, k, n, queries, nq, p.nsplit, sil);
  MMG_CHECK_LAUNCH("km_silhouette(fin)");
  if (sil_mean) {
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nq, 0, 0, 11, k_km_mean, dim3(1), dim3(KM_NTHR), 0, st, (const double*)sil, nq, sil_mean);
    MMG_CHECK_LAUNCH("km_silhouette(mean)");
  }
  return MMG_OK;
}
