// Lab imputation by chained equations (include/mmgnn_chain.h; mmgnn/chained.py): every lab in turn is regressed, by a
// ridge regression over the rows that have it, on all the other labs of the fp64 working matrix W, and its missing cells
// are rewritten from the fit -- sklearn.impute.IterativeImputer(Ridge(alpha), skip_complete=False).
//   k_ch_init     W = observed ? (double)X : center.
//   k_ch_moments  grid (64 x 64 block pairs of the upper block triangle, row slabs): the walk of gram64.h.
//                 The mask is one bit per ROW here: a chunk of 32 rows is staged in LDS as u = W - center,
//                 zeros for a row without the target lab, so one accumulation per 16 x 16 tile on v_mfma_f64_16x16x4_f64
//                 is G; the diagonal block pairs add s as the product with a column of ones, block pair 0 counts n_j.
//   k_ch_sum      one thread per cell of G (a <= b, written to both halves), of s and of n_j: slabs in ascending order.
//   k_ch_solve    one workgroup: C = G - s s^T / n_j over the predictors, + alpha, packed lower triangle in LDS (127 x 128
//                 / 2 doubles = 65,024 bytes), the solve of chol64.h.
//   k_ch_apply    one thread per row without the target lab: the prediction in ascending predictor order, clipped; the
//                 block's largest |new - old| to ws.  k_ch_maxfin: one workgroup folds the blocks' maxima into delta.
//   k_ch_finish   fp32 out: observed cells bit for bit, NaN for a lab nobody has, else (float)W.
// fp64 contraction is OFF for the whole file (chol64.h switches it off for itself): solve and apply restate numpy
// arithmetic operation by operation.  Built into libmmgnn_chain.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "chol64.h"
#include "gram64.h"
#include "../../include/mmgnn_chain.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int CH_NTHR = GRAM64_NTHR;
constexpr int CH_ML = MMG_CH_MAX_LABS;
constexpr int CH_SOLVE_NTHR = 512;           // 16 rows x 32 columns of the trailing update at a time
constexpr int CH_TRI = chol64_packed_size(CH_ML - 1);                             // packed lower triangle, 127 x 127
constexpr int CH_SOLVE_LDS = (CH_TRI + 3 * CH_ML) * (int)sizeof(double) + CH_ML * (int)sizeof(int);
static_assert(MMG_CH_TILE == GRAM64_TILE && MMG_CH_CHUNK == GRAM64_CHUNK, "the header publishes gram64.h's tile and chunk");
static_assert(MMG_CH_MIN_ROWS % MMG_CH_CHUNK == 0, "a slab is whole chunks");
static_assert(MMG_CH_APPLY_ROWS == CH_NTHR, "one thread per row");
static_assert(CH_SOLVE_LDS <= 160 * 1024, "the solve's system lives in one CU's LDS");

inline Gram64Plan ch_plan(int64_t n, int L) { return gram64_plan(n, L, MMG_CH_BLOCKS, MMG_CH_MIN_ROWS); }     // pairs <= 3
inline bool ch_shape_ok(int64_t n, int L) { return n >= 1 && n < INT32_MAX && L >= 1 && L <= CH_ML; }

// ---- W = observed ? X : center
__global__ __launch_bounds__(CH_NTHR) void k_ch_init(const float* __restrict__ X, int64_t n, int L, int64_t ld,
                                                     const double* __restrict__ center, double* __restrict__ W) {
  const int64_t total = n * L, step = (int64_t)gridDim.x * CH_NTHR;
  for (int64_t e = (int64_t)blockIdx.x * CH_NTHR + threadIdx.x; e < total; e += step) {
    const int64_t r = e / L;
    const int a = (int)(e - r * L);
    const float x = X[r * ld + a];
    W[e] = mmg_finite(x) ? (double)x : center[a];
  }
}

// ---- moments: grid (block pairs of the upper triangle, slabs)
struct ChAcc {
  gram64_d4 aG[4] = {}, aS = {};
  double av;
  __device__ __forceinline__ void row(double a, bool diag) {
    av = a;
    if (diag) aS = __builtin_amdgcn_mfma_f64_16x16x4f64(av, 1.0, aS, 0, 0, 0);     // s: the product with ones
  }
  __device__ __forceinline__ void tile(int t, double bv, bool) {
    aG[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, aG[t], 0, 0, 0);
  }
};

__global__ __launch_bounds__(CH_NTHR, 2) void k_ch_moments(const double* __restrict__ W, const float* __restrict__ X,
                                                        int64_t n, int L, int64_t ld, int j,
                                                        const double* __restrict__ center, int64_t rows_per_slab, int nb,
                                                        double* __restrict__ pG, double* __restrict__ ps,
                                                        long long* __restrict__ pn) {
  __shared__ double As[GRAM64_SIDE], Bs[GRAM64_SIDE];
  __shared__ int scnt[4];
  const Gram64Tile t(nb, L, n, rows_per_slab);
  const double mua = t.a_in ? center[t.ca] : 0.0, mub = t.b_in ? center[t.cb] : 0.0;
  int cnt = 0;                                                  // a slab has fewer than 2^31 rows
  ChAcc acc;
  gram64_walk(t, L, As, Bs, acc, [=, &cnt](int64_t r, bool live, double& a, double& b) {
    bool in = false;                                            // the row has the target lab
    if (live) in = mmg_finite(X[r * ld + j]);
    if (in && t.lc == 0) ++cnt;
    a = 0.0, b = 0.0;
    if (in && t.a_in) a = W[r * L + t.ca] - mua;
    if (!t.diag && in && t.b_in) b = W[r * L + t.cb] - mub;
  });
  if (t.lc == 0) scnt[t.lr] = cnt;
  __syncthreads();
  if (threadIdx.x == 0 && blockIdx.x == 0) pn[blockIdx.y] = (long long)scnt[0] + scnt[1] + scnt[2] + scnt[3];
  double* __restrict__ out = pG + (size_t)blockIdx.y * L * L;
  gram64_store_tiles(t, L, [&](int k, bool) { gram64_put(t, L, k, acc.aG[k], out); });
  if (t.strip && t.diag && t.kc == 0) {
#pragma unroll
    for (int g = 0; g < 4; ++g)
      if (t.row(g) < L) ps[(size_t)blockIdx.y * L + t.row(g)] = acc.aS[g];
  }
}

// one thread per cell of G, of s and of n_j; sixteen loads in flight (at 478 slabs the kernel is their latency)
__global__ __launch_bounds__(CH_NTHR) void k_ch_sum(const double* __restrict__ pG, const double* __restrict__ ps,
                                                    const long long* __restrict__ pn, int slabs, int L,
                                                    double* __restrict__ G, double* __restrict__ s,
                                                    long long* __restrict__ n_j) {
  const int idx = (int)blockIdx.x * CH_NTHR + threadIdx.x;
  const int ll = L * L;
  if (idx < ll) {
    gram64_sum_cell<16>(pG, (size_t)ll, slabs, L, idx, true, G);
  } else if (idx < ll + L) {
    const int a = idx - ll;
    s[a] = gram64_sum_slabs<double, 16>(ps + a, (size_t)L, slabs);
  } else if (idx == ll + L) {
    n_j[0] = gram64_sum_slabs<long long, 16>(pn, (size_t)1, slabs);
  }
}

// ---- the ridge system of one target: one workgroup, the packed lower triangle in LDS
__global__ __launch_bounds__(CH_SOLVE_NTHR) void k_ch_solve(const double* __restrict__ G, const double* __restrict__ s,
                                                            const long long* __restrict__ n_j,
                                                            const long long* __restrict__ count, int L, int j,
                                                            double alpha, double* __restrict__ w, double* __restrict__ mu,
                                                            long long* __restrict__ bad) {
  extern __shared__ double ch_sm[];
  double* tri = ch_sm;                       // [CH_TRI]
  double* dg = ch_sm + CH_TRI;               // the pivots' square roots
  double* y = dg + CH_ML;
  double* z = y + CH_ML;
  int* pidx = reinterpret_cast<int*>(z + CH_ML);
  __shared__ int sm_m;
  const int tid = threadIdx.x;
  if (tid == 0) {
    int m = 0;
    for (int a = 0; a < L; ++a)
      if (a != j && count[a] > 0) pidx[m++] = a;
    sm_m = m;
  }
  __syncthreads();
  const int m = sm_m;                        // <= L - 1 <= 127
  const double nj = (double)n_j[0];
  const double sj = s[j];
  for (int e = tid; e < m * m; e += CH_SOLVE_NTHR) {
    const int i = e / m, l = e - i * m;
    if (l <= i) {
      const int a = pidx[i], b = pidx[l];
      double c = G[(size_t)a * L + b] - (s[a] * s[b]) / nj;
      if (i == l) c = c + alpha;
      tri[chol64_packed()(i, l)] = c;
    }
  }
  if (tid < m) {
    const int a = pidx[tid];
    y[tid] = G[(size_t)a * L + j] - (s[a] * sj) / nj;
  }
  const int nbad = chol64_solve<CH_SOLVE_NTHR>(tri, chol64_packed(), m, dg, y, z);
  if (tid < m) w[pidx[tid]] = y[tid];
  for (int a = tid; a < L; a += CH_SOLVE_NTHR) {
    if (a == j || !(count[a] > 0)) w[a] = 0.0;
    mu[a] = s[a] / nj;
  }
  if (tid == 0 && nbad) bad[0] += nbad;
}

// ---- apply: one thread per row
__global__ __launch_bounds__(CH_NTHR) void k_ch_apply(double* __restrict__ W, const float* __restrict__ X, int64_t n, int L,
                                                      int64_t ld, int j, const long long* __restrict__ count,
                                                      const double* __restrict__ center, const double* __restrict__ w,
                                                      const double* __restrict__ mu, const double* __restrict__ lo,
                                                      const double* __restrict__ hi, double* __restrict__ pmax) {
  __shared__ double sw[CH_ML], sc[CH_ML], smu[CH_ML], red[CH_NTHR];
  __shared__ int pidx[CH_ML];
  __shared__ int sm_m;
  const int tid = threadIdx.x;
  if (tid < L) { sw[tid] = w[tid]; sc[tid] = center[tid]; smu[tid] = mu[tid]; }
  if (tid == 0) {
    int m = 0;
    for (int a = 0; a < L; ++a)
      if (a != j && count[a] > 0) pidx[m++] = a;
    sm_m = m;
  }
  __syncthreads();
  const int m = sm_m;
  const int64_t r = (int64_t)blockIdx.x * CH_NTHR + tid;
  double d = 0.0;
  if (r < n && !mmg_finite(X[r * ld + j])) {
    double* __restrict__ row = W + r * L;
    double t = 0.0;
    for (int k = 0; k < m; ++k) {
      const int a = pidx[k];
      t = t + sw[a] * ((row[a] - sc[a]) - smu[a]);
    }
    double v = (sc[j] + smu[j]) + t;
    v = fmax(v, lo[j]);
    v = fmin(v, hi[j]);
    d = fabs(v - row[j]);
    row[j] = v;
  }
  red[tid] = d;
  __syncthreads();
  for (int o = CH_NTHR / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (tid == 0) pmax[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(CH_NTHR) void k_ch_maxfin(const double* __restrict__ pmax, int64_t blocks, int accumulate,
                                                       double* __restrict__ delta) {
  __shared__ double red[CH_NTHR];
  const int tid = threadIdx.x;
  double d = 0.0;
  for (int64_t q = tid; q < blocks; q += CH_NTHR) d = fmax(d, pmax[q]);
  red[tid] = d;
  __syncthreads();
  for (int o = CH_NTHR / 2; o > 0; o >>= 1) {
    if (tid < o) red[tid] = fmax(red[tid], red[tid + o]);
    __syncthreads();
  }
  if (tid == 0) delta[0] = accumulate ? fmax(delta[0], red[0]) : red[0];
}

// ---- the fp32 result
__global__ __launch_bounds__(CH_NTHR) void k_ch_finish(const double* __restrict__ W, const float* __restrict__ X, int64_t n,
                                                       int L, int64_t ld, const long long* __restrict__ count,
                                                       float* __restrict__ out, int64_t ld_out) {
  const int64_t total = n * L, step = (int64_t)gridDim.x * CH_NTHR;
  for (int64_t e = (int64_t)blockIdx.x * CH_NTHR + threadIdx.x; e < total; e += step) {
    const int64_t r = e / L;
    const int a = (int)(e - r * L);
    const float x = X[r * ld + a];
    float v;
    if (mmg_finite(x)) v = x;
    else if (!(count[a] > 0)) v = __builtin_nanf("");
    else v = (float)W[e];
    out[r * ld_out + a] = v;
  }
}

size_t moments_carve(void* ws, int64_t n, int L, double** pG, double** ps, long long** pn) {
  const Gram64Plan p = ch_plan(n, L);
  MmgCarver c(ws);
  *pG = c.take<double>((size_t)p.slabs * L * L);
  *ps = c.take<double>((size_t)p.slabs * L);
  *pn = c.take<long long>((size_t)p.slabs);
  return c.need();
}
inline int64_t apply_blocks(int64_t n) { return (n + CH_NTHR - 1) / CH_NTHR; }
size_t apply_carve(void* ws, int64_t n, double** pmax) {
  MmgCarver c(ws);
  *pmax = c.take<double>((size_t)apply_blocks(n));
  return c.need();
}
inline unsigned cell_grid(int64_t n, int L) {
  int64_t g = (n * L + CH_NTHR - 1) / CH_NTHR;
  return (unsigned)(g > 8192 ? 8192 : g);
}

int ch_check_shape(const char* what, int64_t n, int L, int64_t ld_x) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "%s: n %lld outside [1, 2^31)", what, (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= CH_ML, "%s: %d labs outside [1, %d]", what, L, CH_ML);
  MMG_CHECK_ARG(ld_x >= L, "%s: ld_x %lld < L %d", what, (long long)ld_x, L);
  return MMG_OK;
}

}  // namespace

extern "C" int mmg_chain_plan(int64_t n, int L, int64_t* rows_per_slab, int* slabs) {
  MMG_CHECK_ARG(ch_shape_ok(n, L), "chain_plan: n %lld outside [1, 2^31) or %d labs outside [1, %d]", (long long)n, L,
                CH_ML);
  MMG_CHECK_ARG(rows_per_slab && slabs, "chain_plan: null pointer (rows_per_slab, slabs)");
  const Gram64Plan p = ch_plan(n, L);
  *rows_per_slab = p.rows;
  *slabs = p.slabs;
  return MMG_OK;
}

extern "C" int mmg_chain_init(const float* X, int64_t n, int L, int64_t ld_x, const double* center, double* W,
                              void* stream) {
  if (int rc = ch_check_shape("chain_init", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(X && center && W, "chain_init: null pointer (X, center, W)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_ch_init, dim3(cell_grid(n, L)), dim3(CH_NTHR), 0, (hipStream_t)stream, X,
             n, L, ld_x, center, W);
  MMG_CHECK_LAUNCH("chain_init");
  return MMG_OK;
}

extern "C" size_t mmg_chain_moments_ws_bytes(int64_t n, int L) {
  if (!ch_shape_ok(n, L)) return 0;
  double *pG, *ps;
  long long* pn;
  return moments_carve(nullptr, n, L, &pG, &ps, &pn);
}

extern "C" int mmg_chain_moments(const double* W, const float* X, int64_t n, int L, int64_t ld_x, int j,
                                 const double* center, int64_t* n_j, double* s, double* G, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (int rc = ch_check_shape("chain_moments", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(j >= 0 && j < L, "chain_moments: target %d outside [0, %d)", j, L);
  MMG_CHECK_ARG(W && X && center && n_j && s && G, "chain_moments: null pointer (W, X, center, n_j, s, G)");
  double *pG, *ps;
  long long* pn;
  MMG_CHECK_WS("chain_moments", moments_carve(ws, n, L, &pG, &ps, &pn));
  const Gram64Plan p = ch_plan(n, L);
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, L, 0, k_ch_moments, dim3((unsigned)p.pairs, (unsigned)p.slabs), dim3(CH_NTHR), 0,
             st, W, X, n, L, ld_x, j, center, p.rows, p.nb, pG, ps, pn);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.slabs, L, L, 0, k_ch_sum, dim3((unsigned)((L * L + L + 1 + CH_NTHR - 1) / CH_NTHR)),
             dim3(CH_NTHR), 0, st, pG, ps, pn, p.slabs, L, G, s, (long long*)n_j);
  MMG_CHECK_LAUNCH("chain_moments");
  return MMG_OK;
}

extern "C" int mmg_chain_solve(const double* G, const double* s, const int64_t* n_j, const int64_t* count, int L, int j,
                               double alpha, double* w, double* mu, int64_t* bad, void* stream) {
  MMG_CHECK_ARG(L >= 1 && L <= CH_ML, "chain_solve: %d labs outside [1, %d]", L, CH_ML);
  MMG_CHECK_ARG(j >= 0 && j < L, "chain_solve: target %d outside [0, %d)", j, L);
  MMG_CHECK_ARG(alpha > 0.0 && alpha <= 1.7976931348623157e308, "chain_solve: alpha %g is not a positive finite number",
                alpha);
  MMG_CHECK_ARG(G && s && n_j && count && w && mu && bad, "chain_solve: null pointer (G, s, n_j, count, w, mu, bad)");
  MMG_CHECK_HIP((MmgMaxLds<&k_ch_solve, CH_SOLVE_LDS>::set()), "chain_solve(attr)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, L, L, L, 0, k_ch_solve, dim3(1), dim3(CH_SOLVE_NTHR), CH_SOLVE_LDS, (hipStream_t)stream,
             G, s, (const long long*)n_j, (const long long*)count, L, j, alpha, w, mu, (long long*)bad);
  MMG_CHECK_LAUNCH("chain_solve");
  return MMG_OK;
}

extern "C" size_t mmg_chain_apply_ws_bytes(int64_t n, int L) {
  if (!ch_shape_ok(n, L)) return 0;
  double* pmax;
  return apply_carve(nullptr, n, &pmax);
}

extern "C" int mmg_chain_apply(double* W, const float* X, int64_t n, int L, int64_t ld_x, int j, const int64_t* count,
                               const double* center, const double* w, const double* mu, const double* lo, const double* hi,
                               int accumulate, double* delta, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = ch_check_shape("chain_apply", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(j >= 0 && j < L, "chain_apply: target %d outside [0, %d)", j, L);
  MMG_CHECK_ARG(W && X && count && center && w && mu && lo && hi && delta,
                "chain_apply: null pointer (W, X, count, center, w, mu, lo, hi, delta)");
  double* pmax;
  MMG_CHECK_WS("chain_apply", apply_carve(ws, n, &pmax));
  const int64_t blocks = apply_blocks(n);
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_ch_apply, dim3((unsigned)blocks), dim3(CH_NTHR), 0, st, W, X, n, L, ld_x, j,
             (const long long*)count, center, w, mu, lo, hi, pmax);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, blocks, 1, 0, 0, k_ch_maxfin, dim3(1), dim3(CH_NTHR), 0, st, pmax, blocks,
             accumulate ? 1 : 0, delta);
  MMG_CHECK_LAUNCH("chain_apply");
  return MMG_OK;
}

extern "C" int mmg_chain_finish(const double* W, const float* X, int64_t n, int L, int64_t ld_x, const int64_t* count,
                                float* out, int64_t ld_out, void* stream) {
  if (int rc = ch_check_shape("chain_finish", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(ld_out >= L, "chain_finish: ld_out %lld < L %d", (long long)ld_out, L);
  MMG_CHECK_ARG(W && X && count && out, "chain_finish: null pointer (W, X, count, out)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_ch_finish, dim3(cell_grid(n, L)), dim3(CH_NTHR), 0, (hipStream_t)stream, W,
             X, n, L, ld_x, (const long long*)count, out, ld_out);
  MMG_CHECK_LAUNCH("chain_finish");
  return MMG_OK;
}
