// Per-lab measurement propensity models (include/mmgnn_prop.h; mmgnn/missingness.py): L logistic regressions over the
// same rows by Newton's method, every lab in the same launches, a converged lab frozen by a flag on the device.
//   k_pr_indicator  Y = isfinite(X) as uint8, optionally as fp32 0 / 1 features.
//   k_pr_count      one workgroup per lab: the rows that have it (integers).
//   k_pr_link       64 rows of X staged in LDS as fp32; a wave owns one lab at a time, a lane one row: z in ascending
//                   feature order, p and q from the branch of the logistic that does not cancel, s = p q, r = p - y, the
//                   loss term folded over the wave in a fixed tree.  The same kernel writes the fp32 propensities.
//   k_pr_moments    grid (64 x 64 block pairs of the upper block triangle, row slabs, labs): the walk of gram64.h over the
//                   (D + 2)-wide table [r | s u~] x [0 | u~] on v_mfma_f64_16x16x4_f64.  Both sides are staged on a diagonal
//                   block pair too (the weight sits on ONE side), whose tiles below the diagonal are skipped.
//   k_pr_sum        one thread per cell a <= b: slabs in ascending order; g from row 0, H mirrored.
//   k_pr_solve      one workgroup per lab: H + diag(1 / C, 0), packed lower triangle in LDS (129 x 130 / 2 doubles =
//                   67,080 bytes), the solve of chol64.h, the decrement.
//   k_pr_update     one thread per lab: accept or halve, test convergence, freeze, count.
//   k_pr_pkeys .. k_pr_pall   the weighted error sums over pairs: one stable sort by lab (segsort.h), the labs'
//                   bounds and chunk bases by one workgroup, one workgroup per chunk of 256 pairs of one lab (a fixed tree
//                   in LDS), a lab's chunk sums in ascending order, the labs' sums in ascending order.
// fp64 contraction is OFF for the whole file (chol64.h switches it off for itself): link, solve and update restate numpy
// arithmetic operation by operation.
// Built into libmmgnn_prop.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "chol64.h"
#include "gram64.h"
#include "segsort.h"
#include "../../include/mmgnn_prop.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int PR_NTHR = GRAM64_NTHR;
constexpr int PR_MD = MMG_PR_MAX_FEATURES;
constexpr int PR_MM = PR_MD + 1;                                                  // the widest system
constexpr int PR_ROWS = MMG_PR_LINK_ROWS;
constexpr int PR_XLD = PR_MD + 1;                                                 // odd: a lane per row, no bank conflict
constexpr int PR_SOLVE_NTHR = 512;           // 16 rows x 32 columns of the trailing update at a time
constexpr int PR_TRI = chol64_packed_size(PR_MM);
constexpr int PR_SOLVE_LDS = (PR_TRI + 4 * PR_MM) * (int)sizeof(double);
static_assert(MMG_PR_TILE == GRAM64_TILE && MMG_PR_CHUNK == GRAM64_CHUNK, "the header publishes gram64.h's tile and chunk");
static_assert(MMG_PR_MIN_ROWS % MMG_PR_CHUNK == 0, "a slab is whole chunks");
static_assert(PR_ROWS == 64, "a wave folds the loss terms of one block of rows");
static_assert(PR_SOLVE_LDS <= 160 * 1024, "the solve's system lives in one CU's LDS");

inline Gram64Plan pr_plan(int64_t n, int D) { return gram64_plan(n, D + 2, MMG_PR_BLOCKS, MMG_PR_MIN_ROWS); }  // pairs <= 6
inline bool pr_shape_ok(int64_t n, int D) { return n >= 1 && n < INT32_MAX && D >= 1 && D <= PR_MD; }
inline size_t pr_table_bytes(int64_t n, int D) { return (size_t)pr_plan(n, D).slabs * (D + 2) * (D + 2) * sizeof(double); }
inline int pr_batch(int64_t n, int D) {
  const size_t per_lab = 16 * (size_t)n + pr_table_bytes(n, D);
  const size_t b = (size_t)MMG_PR_WS_BUDGET / per_lab;
  return b < 1 ? 1 : b > MMG_PR_MAX_BATCH ? MMG_PR_MAX_BATCH : (int)b;
}
inline int64_t pr_blocks(int64_t n) { return (n + PR_ROWS - 1) / PR_ROWS; }

// ---- Y = isfinite(X)
__global__ __launch_bounds__(PR_NTHR) void k_pr_indicator(const float* __restrict__ X, int64_t n, int L, int64_t ld,
                                                          uint8_t* __restrict__ Y, int64_t ld_y, float* __restrict__ F,
                                                          int64_t ld_f) {
  const int64_t total = n * L, step = (int64_t)gridDim.x * PR_NTHR;
  for (int64_t e = (int64_t)blockIdx.x * PR_NTHR + threadIdx.x; e < total; e += step) {
    const int64_t r = e / L;
    const int a = (int)(e - r * L);
    const bool in = mmg_finite(X[r * ld + a]);
    Y[r * ld_y + a] = in ? 1 : 0;
    if (F) F[r * ld_f + a] = in ? 1.0f : 0.0f;
  }
}

__global__ __launch_bounds__(PR_NTHR) void k_pr_count(const uint8_t* __restrict__ Y, int64_t n, int64_t ld_y,
                                                      long long* __restrict__ count) {
  __shared__ long long red[PR_NTHR];
  const int tid = threadIdx.x, j = (int)blockIdx.x;
  long long c = 0;
  for (int64_t r = tid; r < n; r += PR_NTHR) c += Y[r * ld_y + j] ? 1 : 0;
  red[tid] = c;
  __syncthreads();
  for (int o = PR_NTHR / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) count[j] = red[0];
}

// ---- link: grid ceil(n / 64); wave w takes the labs k = w, w + 4, ..
template <bool PREDICT>
__global__ __launch_bounds__(PR_NTHR) void k_pr_link(const float* __restrict__ X, int64_t n, int D, int64_t ld,
                                                     const double* __restrict__ mean, const uint8_t* __restrict__ Y,
                                                     int64_t ld_y, int j0, int nb, const double* __restrict__ coef,
                                                     const int* __restrict__ state, double* __restrict__ zo,
                                                     double* __restrict__ pq, double* __restrict__ sr,
                                                     double* __restrict__ lossp, float* __restrict__ out, int64_t ld_out) {
  __shared__ float xs[PR_ROWS * PR_XLD];
  __shared__ double smean[PR_MD];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * PR_ROWS, nblk = gridDim.x;
  for (int e = tid; e < PR_ROWS * D; e += PR_NTHR) {
    const int row = e / D, a = e - row * D;
    xs[row * PR_XLD + a] = r0 + row < n ? X[(r0 + row) * ld + a] : 0.0f;
  }
  if (tid < D) smean[tid] = mean[tid];
  __syncthreads();
  const int64_t i = r0 + lane;
  const bool live = i < n;
  const float* __restrict__ xr = xs + lane * PR_XLD;
  const int M = D + 1;
  for (int k = w; k < nb; k += PR_NTHR / 64) {
    const int j = j0 + k;
    if (!PREDICT && state && state[j * MMG_PR_STATE + MMG_PR_ACTIVE] == 0) continue;       // frozen (wave-uniform)
    const double* __restrict__ cj = coef + (size_t)j * M;
    double z = cj[D];
    for (int a = 0; a < D; ++a) z = z + ((double)xr[a] - smean[a]) * cj[a];
    const double e = exp(-fabs(z)), d = 1.0 + e;
    const double big = 1.0 / d, small = e / d;
    const double p = z >= 0.0 ? big : small, q = z >= 0.0 ? small : big;
    if (PREDICT) {
      if (live) out[i * ld_out + j] = (float)p;
      continue;
    }
    const bool y = live && Y[i * ld_y + j] != 0;
    double t = ((z > 0.0 ? z : 0.0) - (y ? z : 0.0)) + log1p(e);
    if (live) {
      sr[(size_t)k * n + i] = p * q;
      sr[(size_t)(nb + k) * n + i] = y ? -q : p;
      if (zo) zo[(size_t)k * n + i] = z;
      if (pq) {
        pq[(size_t)k * n + i] = p;
        pq[(size_t)(nb + k) * n + i] = q;
      }
    } else {
      t = 0.0;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t = t + __shfl_down(t, o, 64);          // lane 0: v_l + v_{l+o}, l < o
    if (lane == 0) lossp[(size_t)k * nblk + blockIdx.x] = t;
  }
}

// ---- moments: grid (block pairs of the upper triangle, slabs, labs of the batch)
struct PrAcc {
  gram64_d4 aT[4] = {};
  double av;
  int first;                                 // a diagonal block pair: the wave's first tile on or above the diagonal
  __device__ __forceinline__ void row(double a, bool) { av = a; }
  __device__ __forceinline__ void tile(int j, double bv, bool) {
    if (j >= first) aT[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, aT[j], 0, 0, 0);
  }
};

__global__ __launch_bounds__(PR_NTHR, 2) void k_pr_moments(const float* __restrict__ X, int64_t n, int D, int64_t ld,
                                                        const double* __restrict__ mean, const double* __restrict__ sr,
                                                        int j0, int nbat, const int* __restrict__ state,
                                                        int64_t rows_per_slab, int nblocks, int slabs,
                                                        double* __restrict__ part) {
  __shared__ double As[GRAM64_SIDE], Bs[GRAM64_SIDE];
  const int k = (int)blockIdx.z, T = D + 2;
  if (state && state[(j0 + k) * MMG_PR_STATE + MMG_PR_ACTIVE] == 0) return;       // frozen (the whole workgroup)
  const Gram64Tile t(nblocks, T, n, rows_per_slab);
  Gram64Tile tw = t;
  tw.diag = false;                           // the walk stages both sides and offers every tile; PrAcc skips the lower ones
  const double* __restrict__ S = sr + (size_t)k * n;
  const double* __restrict__ R = sr + (size_t)(nbat + k) * n;
  const int ca = t.ca, cb = t.cb;
  const bool a_u = ca >= 1 && ca <= D, b_u = cb >= 1 && cb <= D;
  const double mua = a_u ? mean[ca - 1] : 0.0, mub = b_u ? mean[cb - 1] : 0.0;
  PrAcc acc;
  acc.first = t.diag ? t.w : 0;
  gram64_walk(tw, T, As, Bs, acc, [=](int64_t r, bool live, double& a, double& b) {
    a = 0.0, b = 0.0;
    if (!live) return;
    if (ca == 0) a = R[r];
    else if (a_u) a = S[r] * ((double)X[r * ld + ca - 1] - mua);
    else if (ca == D + 1) a = S[r];
    if (b_u) b = (double)X[r * ld + cb - 1] - mub;
    else if (cb == D + 1) b = 1.0;
  });
  double* __restrict__ out = part + ((size_t)k * slabs + blockIdx.y) * T * T;
  gram64_store_tiles(t, T, [&](int j, bool) { gram64_put(t, T, j, acc.aT[j], out); });
}

// one thread per cell of the table, a <= b; grid (cells, labs of the batch)
__global__ __launch_bounds__(PR_NTHR) void k_pr_sum(const double* __restrict__ part, int slabs, int D, int j0,
                                                    const int* __restrict__ state, double* __restrict__ H,
                                                    double* __restrict__ g) {
  const int k = (int)blockIdx.y, T = D + 2, M = D + 1;
  if (state && state[(j0 + k) * MMG_PR_STATE + MMG_PR_ACTIVE] == 0) return;
  const int idx = (int)blockIdx.x * PR_NTHR + threadIdx.x;
  if (idx >= T * T) return;
  const int a = idx / T, b = idx - a * T;
  if (a > b || b == 0) return;
  const double s = gram64_sum_slabs<double, 16>(part + (size_t)k * slabs * T * T + idx, (size_t)T * T, slabs);
  if (a == 0) {
    g[(size_t)k * M + b - 1] = s;
  } else {
    double* __restrict__ Hk = H + (size_t)k * M * M;
    Hk[(size_t)(a - 1) * M + b - 1] = s;
    if (a < b) Hk[(size_t)(b - 1) * M + a - 1] = s;
  }
}

// ---- the Newton system of one lab: one workgroup, the packed lower triangle in LDS
__global__ __launch_bounds__(PR_SOLVE_NTHR) void k_pr_solve(const double* __restrict__ H, const double* __restrict__ g,
                                                            const double* __restrict__ trial, int D, int j0, double C,
                                                            int* __restrict__ state, double* __restrict__ delta,
                                                            double* __restrict__ dec) {
  extern __shared__ double pr_sm[];
  const int k = (int)blockIdx.x, j = j0 + k, m = D + 1;
  if (state[j * MMG_PR_STATE + MMG_PR_ACTIVE] == 0) return;
  double* tri = pr_sm;                       // [PR_TRI]
  double* dg = pr_sm + PR_TRI;               // the pivots' square roots
  double* y = dg + PR_MM;
  double* z = y + PR_MM;
  double* rhs = z + PR_MM;
  const int tid = threadIdx.x;
  const double* __restrict__ Hk = H + (size_t)k * m * m;
  const double ridge = 1.0 / C;
  for (int e = tid; e < m * m; e += PR_SOLVE_NTHR) {
    const int i = e / m, l = e - i * m;
    if (l <= i) {
      double c = Hk[(size_t)i * m + l];
      if (i == l && i < D) c = c + ridge;
      tri[chol64_packed()(i, l)] = c;
    }
  }
  if (tid < m) {
    double v = g[(size_t)k * m + tid];
    if (tid < D) v = v + trial[(size_t)j * m + tid] / C;
    y[tid] = v;
    rhs[tid] = v;
  }
  const int nbad = chol64_solve<PR_SOLVE_NTHR>(tri, chol64_packed(), m, dg, y, z);
  if (tid < m) delta[(size_t)k * m + tid] = y[tid];
  if (tid == 0) {
    double v = 0.0;
    for (int a = 0; a < m; ++a) v = v + rhs[a] * y[a];
    dec[k] = v;
    if (nbad) state[j * MMG_PR_STATE + MMG_PR_BAD] += nbad;
  }
}

// ---- the state machine: one thread per lab of the batch
__global__ __launch_bounds__(64) void k_pr_update(const double* __restrict__ lossp, int64_t nblk, int D, int j0, int nb,
                                                  const double* __restrict__ delta, const double* __restrict__ dec,
                                                  double C, double threshold, int max_iter, double* __restrict__ beta,
                                                  double* __restrict__ trial, double* __restrict__ step,
                                                  double* __restrict__ fstate, int* __restrict__ state) {
  const int k = (int)blockIdx.x * 64 + threadIdx.x;
  if (k >= nb) return;
  const int j = j0 + k, M = D + 1;
  int* __restrict__ st = state + j * MMG_PR_STATE;
  if (st[MMG_PR_ACTIVE] == 0) return;
  double* __restrict__ fs = fstate + (size_t)j * MMG_PR_FSTATE;
  double* __restrict__ bj = beta + (size_t)j * M;
  double* __restrict__ tj = trial + (size_t)j * M;
  double* __restrict__ sj = step + (size_t)j * M;
  const double* __restrict__ dj = delta + (size_t)k * M;
  const double loss = gram64_sum_slabs<double, 16>(lossp + (size_t)k * nblk, (size_t)1, (int)nblk);
  double pen = 0.0;
  for (int a = 0; a < D; ++a) pen = pen + tj[a] * tj[a];
  const double F = loss + pen / (2.0 * C);
  const double d = dec[k];
  const bool started = st[MMG_PR_STARTED] != 0;
  int it = st[MMG_PR_N_ITER];
  if (started) st[MMG_PR_N_ITER] = ++it;
  fs[3] = F;
  if (!started || d <= threshold || F <= fs[0]) {
    fs[0] = F, fs[1] = 1.0, fs[2] = d;
    st[MMG_PR_STARTED] = 1;
    if (d <= threshold) {                    // converged: the last step is taken, not evaluated
      for (int a = 0; a < M; ++a) bj[a] = tj[a] - dj[a];
      st[MMG_PR_CONVERGED] = 1;
      st[MMG_PR_ACTIVE] = 0;
      return;
    }
    for (int a = 0; a < M; ++a) bj[a] = tj[a];
    if (it >= max_iter) {
      st[MMG_PR_ACTIVE] = 0;
    } else {
      for (int a = 0; a < M; ++a) {
        const double s = dj[a];
        sj[a] = s;
        tj[a] = bj[a] - s;
      }
    }
  } else {
    st[MMG_PR_HALVINGS] += 1;
    const double scale = fs[1] * 0.5;
    fs[1] = scale;
    if (it >= max_iter) {
      st[MMG_PR_ACTIVE] = 0;
    } else {
      for (int a = 0; a < M; ++a) tj[a] = bj[a] - scale * sj[a];
    }
  }
}

// ---- inverse-probability-weighted error sums over pairs
constexpr int PR_PC = MMG_PR_PAIR_CHUNK;
constexpr int PR_PF = MMG_PR_PAIR_FIELDS;
static_assert(PR_PC == PR_NTHR, "one thread per pair of a chunk");
inline int64_t pr_chunk_cap(int64_t m, int L) { return m / PR_PC + L + 1; }

struct PairWs {
  SegSortWs<uint32_t> sort;
  uint32_t *start, *cbase;
  double* part;
};
size_t pair_carve(void* ws, int64_t m, int L, PairWs* w) {
  MmgCarver c(ws);
  segsort_carve(c, m, &w->sort);
  w->start = c.take<uint32_t>((size_t)L + 2);
  w->cbase = c.take<uint32_t>((size_t)L + 2);
  w->part = c.take<double>((size_t)pr_chunk_cap(m, L) * PR_PF);
  return c.need();
}

// key = the lab, L for a pair that is in no sum
__global__ __launch_bounds__(PR_NTHR) void k_pr_pkeys(const long long* __restrict__ patient, const long long* __restrict__ lab,
                                                      int64_t m, int64_t n, int L, uint32_t* __restrict__ keys,
                                                      int32_t* __restrict__ vals) {
  const int64_t step = (int64_t)gridDim.x * PR_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * PR_NTHR + threadIdx.x; i < m; i += step) {
    const long long j = lab[i], r = patient[i];
    keys[i] = (j >= 0 && j < L && r >= 0 && r < n) ? (uint32_t)j : (uint32_t)L;
    vals[i] = (int32_t)i;
  }
}

// one workgroup: start[j] = the first sorted position with key >= j (j = 0 .. L + 1), cbase[j] = the chunks before lab j
__global__ __launch_bounds__(PR_NTHR) void k_pr_pbounds(const uint32_t* __restrict__ keys, int64_t m, int L,
                                                        uint32_t* __restrict__ start, uint32_t* __restrict__ cbase) {
  for (int j = threadIdx.x; j <= L + 1; j += PR_NTHR) start[j] = (uint32_t)lower_bound(keys, m, (uint32_t)j);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t c = 0;
    for (int j = 0; j <= L; ++j) {
      cbase[j] = c;
      if (j < L) c += (start[j + 1] - start[j] + PR_PC - 1) / PR_PC;
    }
  }
}

// one workgroup per chunk of one lab
__global__ __launch_bounds__(PR_NTHR) void k_pr_pchunk(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const long long* __restrict__ patient, const int32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ start, const uint32_t* __restrict__ cbase,
                                                       const float* __restrict__ P, int64_t ld_p, int L,
                                                       const double* __restrict__ cov, double clip, int stabilized,
                                                       double* __restrict__ part) {
  __shared__ double red[PR_PF][PR_NTHR];
  __shared__ int s_lab;
  const uint32_t q = blockIdx.x;
  if (q >= cbase[L]) return;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int lo = 0, hi = L - 1;                  // the last lab whose chunk base is <= q and that has a chunk
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (cbase[mid] <= q) lo = mid; else hi = mid - 1;
    }
    s_lab = lo;
  }
  __syncthreads();
  const int j = s_lab;
  const int64_t pos = (int64_t)start[j] + (int64_t)(q - cbase[j]) * PR_PC + tid;
  double t[PR_PF] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (pos < (int64_t)start[j + 1]) {
    const int64_t i = vals[pos];
    const double e = (double)pred[i] - (double)target[i];
    const double ae = fabs(e), e2 = e * e;
    const double pc = fmax((double)P[patient[i] * ld_p + j], clip);
    const double w = stabilized ? cov[j] / pc : 1.0 / pc;
    t[0] = w, t[1] = w * w, t[2] = w * ae, t[3] = w * e2, t[4] = ae, t[5] = e2;
  }
#pragma unroll
  for (int f = 0; f < PR_PF; ++f) red[f][tid] = t[f];
  __syncthreads();
  for (int o = PR_NTHR / 2; o > 0; o >>= 1) {
    if (tid < o) {
#pragma unroll
      for (int f = 0; f < PR_PF; ++f) red[f][tid] = red[f][tid] + red[f][tid + o];
    }
    __syncthreads();
  }
  if (tid < PR_PF) part[(size_t)q * PR_PF + tid] = red[tid][0];
}

// one workgroup per lab: its chunk sums in ascending order, its count
__global__ __launch_bounds__(64) void k_pr_plab(const double* __restrict__ part, const uint32_t* __restrict__ start,
                                                const uint32_t* __restrict__ cbase, long long* __restrict__ count,
                                                double* __restrict__ sums) {
  const int j = (int)blockIdx.x, f = threadIdx.x;
  if (f < PR_PF)
    sums[(size_t)j * PR_PF + f] = gram64_sum_slabs<double, 16>(part + (size_t)cbase[j] * PR_PF + f, (size_t)PR_PF,
                                                                (int)(cbase[j + 1] - cbase[j]));
  else if (f == PR_PF)
    count[j] = (long long)(start[j + 1] - start[j]);
}

// the overall row: the labs in ascending order
__global__ __launch_bounds__(64) void k_pr_pall(int L, const uint32_t* __restrict__ start, long long* __restrict__ count,
                                                double* __restrict__ sums) {
  const int f = threadIdx.x;
  if (f < PR_PF)
    sums[(size_t)L * PR_PF + f] = gram64_sum_slabs<double, 16>(sums + f, (size_t)PR_PF, L);
  else if (f == PR_PF)
    count[L] = (long long)start[L];
}

inline unsigned cell_grid(int64_t n, int L) {
  int64_t g = (n * L + PR_NTHR - 1) / PR_NTHR;
  return (unsigned)(g > 8192 ? 8192 : g);
}

int pr_check_shape(const char* what, int64_t n, int D, int64_t ld_x) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "%s: n %lld outside [1, 2^31)", what, (long long)n);
  MMG_CHECK_ARG(D >= 1 && D <= PR_MD, "%s: %d features outside [1, %d]", what, D, PR_MD);
  MMG_CHECK_ARG(ld_x >= D, "%s: ld_x %lld < D %d", what, (long long)ld_x, D);
  return MMG_OK;
}

int pr_check_batch(const char* what, int64_t n, int D, int L, int j0, int nb) {
  MMG_CHECK_ARG(L >= 1 && L <= MMG_PR_MAX_LABS, "%s: %d labs outside [1, %d]", what, L, MMG_PR_MAX_LABS);
  MMG_CHECK_ARG(j0 >= 0 && nb >= 1 && nb <= L - j0, "%s: labs [%d, %d + %d) outside [0, %d)", what, j0, j0, nb, L);
  MMG_CHECK_ARG(n < 1 || nb <= pr_batch(n, D), "%s: %d labs in one call, the batch is %d", what, nb, pr_batch(n, D));
  return MMG_OK;
}

}  // namespace

extern "C" int mmg_prop_plan(int64_t n, int D, int64_t* rows_per_slab, int* slabs) {
  MMG_CHECK_ARG(pr_shape_ok(n, D), "prop_plan: n %lld outside [1, 2^31) or %d features outside [1, %d]", (long long)n, D,
                PR_MD);
  MMG_CHECK_ARG(rows_per_slab && slabs, "prop_plan: null pointer (rows_per_slab, slabs)");
  const Gram64Plan p = pr_plan(n, D);
  *rows_per_slab = p.rows;
  *slabs = p.slabs;
  return MMG_OK;
}

extern "C" int mmg_prop_batch(int64_t n, int D) { return pr_shape_ok(n, D) ? pr_batch(n, D) : 0; }

extern "C" int mmg_prop_indicator(const float* X, int64_t n, int L, int64_t ld_x, uint8_t* Y, int64_t ld_y, float* F,
                                  int64_t ld_f, void* stream) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "prop_indicator: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= MMG_PR_MAX_LABS, "prop_indicator: %d columns outside [1, %d]", L, MMG_PR_MAX_LABS);
  MMG_CHECK_ARG(ld_x >= L && ld_y >= L && (!F || ld_f >= L), "prop_indicator: a row stride (%lld, %lld, %lld) < L %d",
                (long long)ld_x, (long long)ld_y, (long long)ld_f, L);
  MMG_CHECK_ARG(X && Y, "prop_indicator: null pointer (X, Y)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_pr_indicator, dim3(cell_grid(n, L)), dim3(PR_NTHR), 0, (hipStream_t)stream,
             X, n, L, ld_x, Y, ld_y, F, ld_f);
  MMG_CHECK_LAUNCH("prop_indicator");
  return MMG_OK;
}

extern "C" int mmg_prop_count(const uint8_t* Y, int64_t n, int L, int64_t ld_y, int64_t* count, void* stream) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "prop_count: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= MMG_PR_MAX_LABS, "prop_count: %d labs outside [1, %d]", L, MMG_PR_MAX_LABS);
  MMG_CHECK_ARG(ld_y >= L, "prop_count: ld_y %lld < L %d", (long long)ld_y, L);
  MMG_CHECK_ARG(Y && count, "prop_count: null pointer (Y, count)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_pr_count, dim3((unsigned)L), dim3(PR_NTHR), 0, (hipStream_t)stream, Y, n,
             ld_y, (long long*)count);
  MMG_CHECK_LAUNCH("prop_count");
  return MMG_OK;
}

extern "C" int mmg_prop_link(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const uint8_t* Y,
                             int64_t ld_y, int L, int j0, int nb, const double* coef, const int32_t* state, double* z,
                             double* pq, double* sr, double* lossp, void* stream) {
  if (int rc = pr_check_shape("prop_link", n, D, ld_x)) return rc;
  if (int rc = pr_check_batch("prop_link", n, D, L, j0, nb)) return rc;
  MMG_CHECK_ARG(ld_y >= L, "prop_link: ld_y %lld < L %d", (long long)ld_y, L);
  MMG_CHECK_ARG(X && mean && Y && coef && sr && lossp, "prop_link: null pointer (X, mean, Y, coef, sr, lossp)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, nb, D, 0, k_pr_link<false>, dim3((unsigned)pr_blocks(n)), dim3(PR_NTHR), 0,
             (hipStream_t)stream, X, n, D, ld_x, mean, Y, ld_y, j0, nb, coef, (const int*)state, z, pq, sr, lossp,
             (float*)nullptr, (int64_t)0);
  MMG_CHECK_LAUNCH("prop_link");
  return MMG_OK;
}

extern "C" size_t mmg_prop_moments_ws_bytes(int64_t n, int D, int nb) {
  if (!pr_shape_ok(n, D) || nb < 1 || nb > pr_batch(n, D)) return 0;
  MmgCarver c(nullptr);
  c.take<double>((size_t)nb * pr_plan(n, D).slabs * (D + 2) * (D + 2));
  return c.need();
}

extern "C" int mmg_prop_moments(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* sr, int L,
                                int j0, int nb, const int32_t* state, double* H, double* g, void* ws, size_t ws_bytes,
                                void* stream) {
  if (int rc = pr_check_shape("prop_moments", n, D, ld_x)) return rc;
  if (int rc = pr_check_batch("prop_moments", n, D, L, j0, nb)) return rc;
  MMG_CHECK_ARG(X && mean && sr && H && g, "prop_moments: null pointer (X, mean, sr, H, g)");
  const Gram64Plan p = pr_plan(n, D);
  const int T = D + 2;
  MmgCarver c(ws);
  double* part = c.take<double>((size_t)nb * p.slabs * T * T);
  MMG_CHECK_WS("prop_moments", c.need());
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, T, T, 0, k_pr_moments, dim3((unsigned)p.pairs, (unsigned)p.slabs, (unsigned)nb),
             dim3(PR_NTHR), 0, st, X, n, D, ld_x, mean, sr, j0, nb, (const int*)state, p.rows, p.nb, p.slabs, part);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.slabs, T, T, 0, k_pr_sum, dim3((unsigned)((T * T + PR_NTHR - 1) / PR_NTHR), (unsigned)nb),
             dim3(PR_NTHR), 0, st, part, p.slabs, D, j0, (const int*)state, H, g);
  MMG_CHECK_LAUNCH("prop_moments");
  return MMG_OK;
}

extern "C" int mmg_prop_solve(const double* H, const double* g, const double* trial, int D, int L, int j0, int nb, double C,
                              int32_t* state, double* delta, double* dec, void* stream) {
  MMG_CHECK_ARG(D >= 1 && D <= PR_MD, "prop_solve: %d features outside [1, %d]", D, PR_MD);
  if (int rc = pr_check_batch("prop_solve", 0, D, L, j0, nb)) return rc;
  MMG_CHECK_ARG(nb <= MMG_PR_MAX_BATCH, "prop_solve: %d labs in one call, at most %d", nb, MMG_PR_MAX_BATCH);
  MMG_CHECK_ARG(C > 0.0 && C <= 1.7976931348623157e308, "prop_solve: C %g is not a positive finite number", C);
  MMG_CHECK_ARG(H && g && trial && state && delta && dec, "prop_solve: null pointer (H, g, trial, state, delta, dec)");
  MMG_CHECK_HIP((MmgMaxLds<&k_pr_solve, PR_SOLVE_LDS>::set()), "prop_solve(attr)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nb, D + 1, D + 1, 0, k_pr_solve, dim3((unsigned)nb), dim3(PR_SOLVE_NTHR), PR_SOLVE_LDS,
             (hipStream_t)stream, H, g, trial, D, j0, C, (int*)state, delta, dec);
  MMG_CHECK_LAUNCH("prop_solve");
  return MMG_OK;
}

extern "C" int mmg_prop_update(const double* lossp, int64_t n, int D, int L, int j0, int nb, const double* delta,
                               const double* dec, double C, double threshold, int max_iter, double* beta, double* trial,
                               double* step, double* fstate, int32_t* state, void* stream) {
  if (int rc = pr_check_shape("prop_update", n, D, D)) return rc;
  if (int rc = pr_check_batch("prop_update", n, D, L, j0, nb)) return rc;
  MMG_CHECK_ARG(C > 0.0 && C <= 1.7976931348623157e308, "prop_update: C %g is not a positive finite number", C);
  MMG_CHECK_ARG(threshold >= 0.0 && threshold <= 1.7976931348623157e308, "prop_update: threshold %g is not in [0, inf)",
                threshold);
  MMG_CHECK_ARG(max_iter >= 1, "prop_update: max_iter %d < 1", max_iter);
  MMG_CHECK_ARG(lossp && delta && dec && beta && trial && step && fstate && state,
                "prop_update: null pointer (lossp, delta, dec, beta, trial, step, fstate, state)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nb, D + 1, 0, 0, k_pr_update, dim3((unsigned)((nb + 63) / 64)), dim3(64), 0,
             (hipStream_t)stream, lossp, pr_blocks(n), D, j0, nb, delta, dec, C, threshold, max_iter, beta, trial, step,
             fstate, (int*)state);
  MMG_CHECK_LAUNCH("prop_update");
  return MMG_OK;
}

extern "C" int mmg_prop_predict(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* coef,
                                int L, float* out, int64_t ld_out, void* stream) {
  if (int rc = pr_check_shape("prop_predict", n, D, ld_x)) return rc;
  MMG_CHECK_ARG(L >= 1 && L <= MMG_PR_MAX_LABS, "prop_predict: %d labs outside [1, %d]", L, MMG_PR_MAX_LABS);
  MMG_CHECK_ARG(ld_out >= L, "prop_predict: ld_out %lld < L %d", (long long)ld_out, L);
  MMG_CHECK_ARG(X && mean && coef && out, "prop_predict: null pointer (X, mean, coef, out)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, D, 0, k_pr_link<true>, dim3((unsigned)pr_blocks(n)), dim3(PR_NTHR), 0,
             (hipStream_t)stream, X, n, D, ld_x, mean, (const uint8_t*)nullptr, (int64_t)0, 0, L, coef, (const int*)nullptr,
             (double*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr, out, ld_out);
  MMG_CHECK_LAUNCH("prop_predict");
  return MMG_OK;
}

extern "C" size_t mmg_prop_pair_sums_ws_bytes(int64_t m, int L) {
  if (m < 0 || m >= INT32_MAX || L < 1 || L > MMG_PR_MAX_LABS) return 0;
  PairWs w;
  return pair_carve(nullptr, m, L, &w);
}

extern "C" int mmg_prop_pair_sums(const float* pred, const float* target, const int64_t* patient, const int64_t* lab,
                                  int64_t m, const float* P, int64_t n, int L, int64_t ld_p, const double* cov, double clip,
                                  int stabilized, int64_t* count, double* sums, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(m >= 0 && m < INT32_MAX, "prop_pair_sums: %lld pairs outside [0, 2^31)", (long long)m);
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "prop_pair_sums: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= MMG_PR_MAX_LABS, "prop_pair_sums: %d labs outside [1, %d]", L, MMG_PR_MAX_LABS);
  MMG_CHECK_ARG(ld_p >= L, "prop_pair_sums: ld_p %lld < L %d", (long long)ld_p, L);
  MMG_CHECK_ARG(clip > 0.0 && clip <= 1.0, "prop_pair_sums: clip %g outside (0, 1]", clip);
  MMG_CHECK_ARG(m == 0 || (pred && target && patient && lab), "prop_pair_sums: null pointer (pred, target, patient, lab)");
  MMG_CHECK_ARG(P && count && sums && (!stabilized || cov), "prop_pair_sums: null pointer (P, count, sums, cov)");
  PairWs w;
  MMG_CHECK_WS("prop_pair_sums", pair_carve(ws, m, L, &w));
  hipStream_t st = (hipStream_t)stream;
  const RadixPairs<uint32_t>& b = w.sort.kv;        // the sort leaves its result here
  if (m > 0) {
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, m, L, 0, 0, k_pr_pkeys, dim3(cell_grid(m, 1)), dim3(PR_NTHR), 0, st,
               (const long long*)patient, (const long long*)lab, m, n, L, b.keys, b.vals);
    segsort_run(w.sort, m, bits_of((unsigned)L), st);            // keys 0 .. L
  }
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, m, L, 1, 0, k_pr_pbounds, dim3(1), dim3(PR_NTHR), 0, st, b.keys, m, L, w.start, w.cbase);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, m, L, 2, 0, k_pr_pchunk, dim3((unsigned)pr_chunk_cap(m, L)), dim3(PR_NTHR), 0, st, pred,
             target, (const long long*)patient, b.vals, w.start, w.cbase, P, ld_p, L, cov, clip, stabilized ? 1 : 0, w.part);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, m, L, 3, 0, k_pr_plab, dim3((unsigned)L), dim3(64), 0, st, w.part, w.start, w.cbase,
             (long long*)count, sums);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, L, PR_PF, 4, 0, k_pr_pall, dim3(1), dim3(64), 0, st, L, w.start, (long long*)count, sums);
  MMG_CHECK_LAUNCH("prop_pair_sums");
  return MMG_OK;
}
