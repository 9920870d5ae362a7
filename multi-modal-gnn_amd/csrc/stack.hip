// Per-lab stacked recalibration of imputed lab values (include/mmgnn_stack.h; mmgnn/stacking.py): the normal-equation
// sums of a ridge regression of the target on K predictors per (fold, lab, degree bin), the coefficients of every cell
// from the first usable of (cell, lab, all pairs), and the epilogues that apply them and score the result.
//   k_st_keys        ONE read of the indices and values: sort key = fold * n_cells + cell (n_seg for a dropped pair: sorts
//                    last), payload = the pair's position, the four kinds of dropped pairs (drop_flush of segsort.h).
//   segsort_run      the stable sort of segsort.h over the 1-3 digits of the segment.
//   k_seg_bounds     (segsort.h) one thread per segment: where it begins in the sorted keys (a binary search).
//   k_st_chunks      workgroup (x, y) walks the chunks y, y + grid.y, .. of the segments x, x + grid.x, ..: a chunk is
//                    ST_CHUNK consecutive sorted pairs of ONE segment, so no thread ever looks at a key.  Thread t gathers
//                    the pairs t, t + 256, .. of the chunk, forms their terms in fp64 (each a product of two fp32 values:
//                    exact) and adds them to F registers; the waves are folded by the butterfly of wave_sum_d, the four waves
//                    through LDS in wave order.  The chunk's F sums go to its own slot: slot = (position of the chunk's
//                    first pair) / ST_CHUNK + segment, which is different for every chunk and needs no scan.
//   k_st_combine     one thread per (segment, sum): the segment's slots added in chunk order; every element of `sums` is
//                    written exactly once, nothing is zero-filled, nothing is accumulated in memory.
//   k_st_train / k_st_group   the training sums of every fold-out, then of every lab and of all pairs, in fixed order.
//   k_st_solve       one thread per (fold-out, cell): the unrolled Cholesky of the header at the cell, then its lab, then
//                    all pairs, until one is usable.
//   k_st_apply_pairs / k_st_apply_matrix   one thread per prediction; the coefficient table is small and stays in cache.
// fp64 contraction is OFF for the whole file: the solve and the apply restate numpy arithmetic operation by operation.
// Built into libmmgnn_stack.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "cells.h"
#include "radix_sort.h"
#include "../../include/mmgnn_conformal.h"
#include "../../include/mmgnn_stack.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int ST_NTHR = 256;
constexpr int ST_CHUNK = MMG_ST_CHUNK;
constexpr int ST_MAX_GRID = 2048;
constexpr int ST_MAX_K = MMG_ST_MAX_FEATURES;
constexpr double ST_PIVOT_REL = 1e-10;
static_assert(MMG_ST_PIVOT_REL_LOG10 == -10, "ST_PIVOT_REL is 10^MMG_ST_PIVOT_REL_LOG10");
static_assert(MMG_ST_MAX_LABS == MMG_CF_MAX_LABS && MMG_ST_MAX_BINS == MMG_CF_MAX_BINS &&
              MMG_ST_MAX_CELLS == MMG_CF_MAX_CELLS && MMG_ST_DROP_KINDS == MMG_CF_DROP_KINDS,
              "the cells of the conformal library");
static_assert(ST_CHUNK % ST_NTHR == 0, "a chunk is whole rounds of the workgroup");
static_assert((int64_t)MMG_ST_MAX_FOLDS * MMG_ST_MAX_CELLS < (1 << 24), "the sort runs over three digits of the segment");

constexpr int st_fields(int K) { return (K + 1) * (K + 2) / 2 + K + 2; }

struct StFeats {
  const float* f[ST_MAX_K];
  int64_t ld[ST_MAX_K];      // the matrix epilogue's row strides
  int K;
};

__device__ __forceinline__ int st_fold(uint32_t key, int patient, int folds) {
  uint32_t w0, w1;
  mmg_rng_group(key, (uint64_t)(uint32_t)patient, &w0, &w1);       // w1 is dead code: only the first word is used
  return (int)(w0 % (uint32_t)folds);
}

// ---------------------------------------------------------------------------------- keys
// values: the K features and, when given, the target -- a NaN in any of them drops the pair
template <class IT>
__global__ __launch_bounds__(ST_NTHR) void k_st_keys(StFeats ft, const float* __restrict__ target,
                                                     const IT* __restrict__ patient, const IT* __restrict__ lab, int64_t n,
                                                     int L, const int32_t* __restrict__ deg, int64_t n_pat, int B,
                                                     CellEdges ed, int folds, uint32_t rng_key, uint32_t* __restrict__ key,
                                                     int32_t* __restrict__ id, unsigned long long* __restrict__ dropped) {
  int cnt[MMG_ST_DROP_KINDS] = {0, 0, 0, 0};
  const int n_cells = L * B, n_seg = folds * n_cells;
  const int64_t step = (int64_t)gridDim.x * ST_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; i < n; i += step) {
    int kind = -1, seg = n_seg;
    const int l = cell_index(lab, i, L);
    const int p = l >= 0 ? cell_index(patient, i, n_pat) : -1;
    const int b = p >= 0 ? cell_bin(deg[p], ed, B) : -1;
    if (l < 0) kind = 0;
    else if (p < 0) kind = 1;
    else if (b < 0) kind = 2;
    else {
      bool nan = target ? target[i] != target[i] : false;
      for (int k = 0; k < ft.K; ++k) {
        const float v = ft.f[k][i];
        nan = nan || v != v;
      }
      if (nan) kind = 3;
      else seg = (folds > 1 ? st_fold(rng_key, p, folds) : 0) * n_cells + l * B + b;
    }
#pragma unroll
    for (int q = 0; q < MMG_ST_DROP_KINDS; ++q) cnt[q] += kind == q ? 1 : 0;
    key[i] = (uint32_t)seg;
    id[i] = (int32_t)i;
  }
  drop_flush(cnt, dropped);
}

// ---------------------------------------------------------------------------------- terms
template <int K_>
struct FitTerms {
  static constexpr int NF = st_fields(K_);
  const float* f[K_];
  const float* t;
  __device__ __forceinline__ void load(int32_t i, double* __restrict__ x) const {
    double phi[K_ + 1];
    phi[0] = 1.0;
#pragma unroll
    for (int k = 0; k < K_; ++k) phi[k + 1] = (double)f[k][i];
    const double td = (double)t[i];
    int q = 0;
#pragma unroll
    for (int a = 0; a <= K_; ++a)
#pragma unroll
      for (int b = a; b <= K_; ++b) x[q++] = phi[a] * phi[b];
#pragma unroll
    for (int a = 0; a <= K_; ++a) x[q++] = phi[a] * td;
    x[q] = td * td;
  }
};
struct ScoreTerms {
  static constexpr int NF = MMG_ST_SCORE_FIELDS;
  const float *raw, *stacked, *t;
  __device__ __forceinline__ void load(int32_t i, double* __restrict__ x) const {
    const float tv = t[i];
    const float e0 = tv - raw[i], e1 = tv - stacked[i];
    x[0] = 1.0;
    x[1] = (double)fabsf(e0);
    x[2] = (double)e0 * (double)e0;
    x[3] = (double)fabsf(e1);
    x[4] = (double)e1 * (double)e1;
  }
};

__device__ __forceinline__ int64_t st_slot(int64_t first_pair, int s) { return first_pair / ST_CHUNK + s; }

template <class T>
__global__ __launch_bounds__(ST_NTHR) void k_st_chunks(const int32_t* __restrict__ id, const int64_t* __restrict__ seg_lo,
                                                       int n_seg, T terms, double* __restrict__ part) {
  constexpr int NF = T::NF;
  __shared__ double s_w[ST_NTHR / WAVE][NF];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int s = blockIdx.x; s < n_seg; s += gridDim.x) {
    const int64_t lo = seg_lo[s], hi = seg_lo[s + 1];              // the same for every thread of the workgroup
    const int64_t n_chunks = (hi - lo + ST_CHUNK - 1) / ST_CHUNK;
    for (int64_t j = blockIdx.y; j < n_chunks; j += gridDim.y) {
      const int64_t begin = lo + j * ST_CHUNK;
      const int64_t end = begin + ST_CHUNK < hi ? begin + ST_CHUNK : hi;
      double acc[NF];
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = 0.0;
      for (int64_t p = begin + threadIdx.x; p < end; p += ST_NTHR) {
        double x[NF];
        terms.load(id[p], x);
#pragma unroll
        for (int f = 0; f < NF; ++f) acc[f] = acc[f] + x[f];
      }
#pragma unroll
      for (int f = 0; f < NF; ++f) acc[f] = wave_sum_d(acc[f]);
      __syncthreads();                                             // the previous chunk's shared values are consumed
      if (lane == 0) {
#pragma unroll
        for (int f = 0; f < NF; ++f) s_w[wid][f] = acc[f];
      }
      __syncthreads();
      if (threadIdx.x < NF) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < ST_NTHR / WAVE; ++q) t = t + s_w[q][threadIdx.x];
        part[(size_t)st_slot(begin, s) * NF + threadIdx.x] = t;
      }
    }
  }
}

__global__ __launch_bounds__(ST_NTHR) void k_st_combine(const int64_t* __restrict__ seg_lo, int n_seg, int NF,
                                                        const double* __restrict__ part, double* __restrict__ sums) {
  const int64_t total = (int64_t)n_seg * NF;
  for (int64_t e = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST_NTHR) {
    const int s = (int)(e / NF), f = (int)(e - (int64_t)s * NF);
    const int64_t lo = seg_lo[s], hi = seg_lo[s + 1];
    double t = 0.0;
    for (int64_t b = lo; b < hi; b += ST_CHUNK) t = t + part[(size_t)st_slot(b, s) * NF + f];
    sums[e] = t;
  }
}

// ---------------------------------------------------------------------------------- solve
// T [folds_out][n_cells * F]: row jo adds the folds but jo in fold order (leave = -1: every fold)
__global__ __launch_bounds__(ST_NTHR) void k_st_train(const double* __restrict__ sums, int64_t per_fold, int folds,
                                                      int folds_out, double* __restrict__ T) {
  const int64_t total = per_fold * folds_out;
  for (int64_t e = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST_NTHR) {
    const int jo = (int)(e / per_fold);
    const int64_t rem = e - (int64_t)jo * per_fold;
    const int leave = jo < folds && folds > 1 ? jo : -1;
    double t = 0.0;
    for (int fo = 0; fo < folds; ++fo)
      if (fo != leave) t = t + sums[(int64_t)fo * per_fold + rem];
    T[e] = t;
  }
}
// dst [n_groups][F] = the rows g * gs .. g * gs + gs - 1 of src [n_groups * gs][F] added in that order from 0
__global__ __launch_bounds__(ST_NTHR) void k_st_group(const double* __restrict__ src, int64_t n_groups, int gs, int F,
                                                      double* __restrict__ dst) {
  const int64_t total = n_groups * F;
  for (int64_t e = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST_NTHR) {
    const int64_t g = e / F;
    const int f = (int)(e - g * F);
    double t = 0.0;
    for (int i = 0; i < gs; ++i) t = t + src[(g * gs + i) * F + f];
    dst[e] = t;
  }
}

// the system of the header over the sums S [F]; false: not usable (w is then undefined); *m = the pairs behind it
template <int K_>
__device__ __forceinline__ bool st_system(const double* __restrict__ S, double ridge, double need, double* __restrict__ w,
                                          double* __restrict__ m) {
  constexpr int P = K_ + 1;
  double A[P][P], r[P], L[P][P], z[P];
  int q = 0;
#pragma unroll
  for (int a = 0; a < P; ++a)
#pragma unroll
    for (int b = a; b < P; ++b) {
      A[a][b] = S[q];
      A[b][a] = S[q];
      ++q;
    }
#pragma unroll
  for (int a = 0; a < P; ++a) r[a] = S[q + a];
  *m = A[0][0];
  if (!(A[0][0] >= need)) return false;
  r[1] = r[1] + ridge * A[1][1];
#pragma unroll
  for (int a = 0; a < P; ++a) {
    const double g = A[a][a];
    A[a][a] = g + ridge * g;
  }
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      if (j < i) {
        L[i][j] = s / L[j][j];
      } else {
        if (!(s > ST_PIVOT_REL * A[i][i])) return false;
        L[i][i] = __dsqrt_rn(s);
      }
    }
#pragma unroll
  for (int i = 0; i < P; ++i) {
    double s = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s = s - L[i][k] * z[k];
    z[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = P - 1; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k < P; ++k) s = s - L[k][i] * w[k];
    w[i] = s / L[i][i];
  }
  return true;
}

template <int K_>
__global__ __launch_bounds__(ST_NTHR) void k_st_solve(const double* __restrict__ T, const double* __restrict__ labs,
                                                      const double* __restrict__ all, int n_cells, int B, int folds_out,
                                                      double ridge, double need, double* __restrict__ coef,
                                                      int32_t* __restrict__ level, int32_t* __restrict__ n_used) {
  constexpr int P = K_ + 1, F = st_fields(K_);
  const int64_t total = (int64_t)folds_out * n_cells;
  const int n_labs = n_cells / B;
  for (int64_t e = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; e < total; e += (int64_t)gridDim.x * ST_NTHR) {
    const int jo = (int)(e / n_cells), c = (int)(e - (int64_t)jo * n_cells);
    double w[P], m = 0.0;
    int lv = 0;
    if (!st_system<K_>(T + e * F, ridge, need, w, &m)) {
      lv = 1;
      if (!st_system<K_>(labs + ((int64_t)jo * n_labs + c / B) * F, ridge, need, w, &m)) {
        lv = 2;
        if (!st_system<K_>(all + (int64_t)jo * F, ridge, need, w, &m)) {
          lv = 3;
          m = 0.0;
#pragma unroll
          for (int a = 0; a < P; ++a) w[a] = a == 1 ? 1.0 : 0.0;
        }
      }
    }
#pragma unroll
    for (int a = 0; a < P; ++a) coef[e * P + a] = w[a];
    level[e] = lv;
    n_used[e] = (int32_t)m;
  }
}

// ---------------------------------------------------------------------------------- apply
__device__ __forceinline__ float st_apply(const double* __restrict__ w, const float* v, int K) {
  double y = w[0];
  for (int k = 0; k < K; ++k) {
    const double prod = w[k + 1] * (double)v[k];
    y = y + prod;
  }
  return (float)y;
}

template <class IT>
__global__ __launch_bounds__(ST_NTHR) void k_st_apply_pairs(StFeats ft, const IT* __restrict__ patient,
                                                            const IT* __restrict__ lab, int64_t n, int L,
                                                            const int32_t* __restrict__ deg, int64_t n_pat, int B, CellEdges ed,
                                                            const double* __restrict__ coef, int folds, uint32_t rng_key,
                                                            int cross, float* __restrict__ out) {
  const int n_cells = L * B, P = ft.K + 1;
  const int last = folds > 1 ? folds : 0;
  const int64_t step = (int64_t)gridDim.x * ST_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; i < n; i += step) {
    float v[ST_MAX_K];
    for (int k = 0; k < ft.K; ++k) v[k] = ft.f[k][i];
    const int l = cell_index(lab, i, L);
    const int p = l >= 0 ? cell_index(patient, i, n_pat) : -1;
    const int b = p >= 0 ? cell_bin(deg[p], ed, B) : -1;
    float y = v[0];
    if (b >= 0) {
      const int row = cross ? st_fold(rng_key, p, folds) : last;
      y = st_apply(coef + ((size_t)row * n_cells + l * B + b) * P, v, ft.K);
    }
    out[i] = y;
  }
}

template <class IT>
__global__ __launch_bounds__(ST_NTHR) void k_st_apply_matrix(StFeats ft, int64_t n_rows, int L, const IT* __restrict__ rows,
                                                             const int32_t* __restrict__ deg, int64_t n_pat, int B,
                                                             CellEdges ed, const double* __restrict__ coef, int folds,
                                                             uint32_t rng_key, int cross, float* __restrict__ out,
                                                             int64_t ld_out) {
  const int n_cells = L * B, P = ft.K + 1;
  const int last = folds > 1 ? folds : 0;
  const int64_t total = n_rows * L, step = (int64_t)gridDim.x * ST_NTHR;
  for (int64_t e = (int64_t)blockIdx.x * ST_NTHR + threadIdx.x; e < total; e += step) {
    const int64_t r = e / L;
    const int c = (int)(e - r * L);
    float v[ST_MAX_K];
    for (int k = 0; k < ft.K; ++k) v[k] = ft.f[k][r * ft.ld[k] + c];
    int p;
    if (rows) p = cell_index(rows, r, n_pat);
    else p = r < n_pat ? (int)r : -1;
    const int b = p >= 0 ? cell_bin(deg[p], ed, B) : -1;
    float y = v[0];
    if (b >= 0) {
      const int row = cross ? st_fold(rng_key, p, folds) : last;
      y = st_apply(coef + ((size_t)row * n_cells + c * B + b) * P, v, ft.K);
    }
    out[r * ld_out + c] = y;
  }
}

// ---------------------------------------------------------------------------------- host
bool shape_ok(int64_t n, int L, int B) {
  return n >= 0 && n <= INT32_MAX && L >= 1 && L <= MMG_ST_MAX_LABS && B >= 1 && B <= MMG_ST_MAX_BINS &&
         (int64_t)L * B <= MMG_ST_MAX_CELLS;
}
bool model_ok(int K, int folds) { return K >= 1 && K <= MMG_ST_MAX_FEATURES && folds >= 1 && folds <= MMG_ST_MAX_FOLDS; }

int pairs_check(const char* what, const void* patient, const void* lab, int index_bytes, int64_t n, int L, const int32_t* deg,
                int64_t n_pat, const double* edges, int B, CellEdges* ed) {
  const int rc = cells_check(what, index_bytes, n, L, n_pat, edges, B, ed);      // the limits are equal by the assert above
  if (rc != MMG_OK) return rc;
  MMG_CHECK_ARG(n == 0 || (patient && lab), "%s: null patient or lab", what);
  MMG_CHECK_ARG(n_pat == 0 || deg, "%s: null deg", what);
  return MMG_OK;
}
int model_check(const char* what, int K, int folds) {
  MMG_CHECK_ARG(K >= 1 && K <= MMG_ST_MAX_FEATURES, "%s: %d features outside [1, %d]", what, K, MMG_ST_MAX_FEATURES);
  MMG_CHECK_ARG(folds >= 1 && folds <= MMG_ST_MAX_FOLDS, "%s: %d folds outside [1, %d]", what, folds, MMG_ST_MAX_FOLDS);
  return MMG_OK;
}
int feats_check(const char* what, const float* const* feats, int K, bool need, StFeats* ft) {
  MMG_CHECK_ARG(feats, "%s: null feature list", what);
  *ft = StFeats{};
  ft->K = K;
  for (int k = 0; k < K; ++k) {
    MMG_CHECK_ARG(!need || feats[k], "%s: null feature %d", what, k);
    ft->f[k] = feats[k];
  }
  return MMG_OK;
}

struct SumsWs {
  SegSortWs<uint32_t> sort;
  int64_t* seg_lo;           // [n_seg + 1]: seg_lo[n_seg] = the number of kept pairs
  double* part;
};
size_t sums_carve(void* ws, int64_t n, int n_seg, int NF, SumsWs* w) {
  MmgCarver c(ws);
  segsort_carve(c, n, &w->sort);
  w->seg_lo = c.take<int64_t>((size_t)n_seg + 1);
  w->part = c.take<double>(((size_t)(n / ST_CHUNK) + (size_t)n_seg + 1) * NF);      // slot < n / C + n_seg
  return c.need();
}

// keys -> sort -> bounds -> chunks -> combine: sums [n_seg][T::NF]
template <class T>
int sums_run(const char* what, const StFeats& ft, const float* target, const void* patient, const void* lab, int index_bytes,
             int64_t n, int L, const int32_t* deg, int64_t n_pat, int B, const CellEdges& ed, int folds, uint64_t seed,
             const T& terms, double* sums, int64_t* dropped, SumsWs w, hipStream_t st) {
  const int n_seg = folds * L * B;
  const uint32_t rng_key = mmg_rng_key(seed, (uint32_t)MMG_ST_SITE);
  const RadixPairs<uint32_t>& kv = w.sort.kv;       // the sort leaves its result here (w is a copy: its buffers swap)
  MMG_CHECK_HIP(mmg_zero_async(dropped, MMG_ST_DROP_KINDS * sizeof(int64_t), st), what);
  if (n > 0) {
    index_dispatch(index_bytes, [&](auto it) {
      using IT = decltype(it);
      hipLaunchKernelGGL(k_st_keys<IT>, dim3(launch_grid(n, ST_NTHR, ST_MAX_GRID)), dim3(ST_NTHR), 0, st, ft, target,
                         (const IT*)patient, (const IT*)lab, n, L, deg, n_pat, B, ed, folds, rng_key, kv.keys, kv.vals,
                         (unsigned long long*)dropped);
    });
    MMG_CHECK_LAUNCH(what);
    segsort_run(w.sort, n, bits_of((unsigned)n_seg), st);                // the key reaches n_seg itself
    MMG_CHECK_LAUNCH(what);
  }
  seg_bounds(kv.keys, n, n_seg, 0, w.seg_lo, st);
  MMG_CHECK_LAUNCH(what);
  if (n > 0) {
    const int64_t max_chunks = (n + ST_CHUNK - 1) / ST_CHUNK;
    const unsigned gx = (unsigned)(n_seg < 4096 ? n_seg : 4096);
    int64_t gy = 8192 / gx;
    gy = gy < 1 ? 1 : gy > max_chunks ? max_chunks : gy;
    hipLaunchKernelGGL(k_st_chunks<T>, dim3(gx, (unsigned)gy), dim3(ST_NTHR), 0, st, kv.vals, w.seg_lo, n_seg, terms, w.part);
    MMG_CHECK_LAUNCH(what);
  }
  hipLaunchKernelGGL(k_st_combine, dim3(launch_grid((int64_t)n_seg * T::NF, ST_NTHR, ST_MAX_GRID, 1)), dim3(ST_NTHR), 0, st,
                     w.seg_lo, n_seg, T::NF, w.part, sums);
  MMG_CHECK_LAUNCH(what);
  return MMG_OK;
}

template <int K_>
int fit_sums(const StFeats& ft, const float* target, const void* patient, const void* lab, int index_bytes, int64_t n, int L,
             const int32_t* deg, int64_t n_pat, int B, const CellEdges& ed, int folds, uint64_t seed, double* sums,
             int64_t* dropped, const SumsWs& w, hipStream_t st) {
  FitTerms<K_> terms;
  for (int k = 0; k < K_; ++k) terms.f[k] = ft.f[k];
  terms.t = target;
  return sums_run("stack_sums", ft, target, patient, lab, index_bytes, n, L, deg, n_pat, B, ed, folds, seed, terms, sums,
                  dropped, w, st);
}

struct SolveWs {
  double *T, *labs, *all;
};
size_t solve_carve(void* ws, int L, int B, int K, int folds, SolveWs* w) {
  MmgCarver c(ws);
  const size_t fo = folds > 1 ? (size_t)folds + 1 : 1, F = (size_t)st_fields(K);
  w->T = c.take<double>(fo * L * B * F);
  w->labs = c.take<double>(fo * L * F);
  w->all = c.take<double>(fo * F);
  return c.need();
}

}  // namespace

extern "C" size_t mmg_stack_sums_ws_bytes(int64_t n, int n_labs, int n_bins, int n_features, int folds) {
  if (!shape_ok(n, n_labs, n_bins) || !model_ok(n_features, folds)) return 0;
  SumsWs w;
  return sums_carve(nullptr, n, folds * n_labs * n_bins, st_fields(n_features), &w);
}

extern "C" int mmg_stack_sums(const float* const* feats, int n_features, const float* target, const void* patient,
                              const void* lab, int index_bytes, int64_t n, int n_labs, const int32_t* deg,
                              int64_t n_patients, const double* bin_edges, int n_bins, int folds, uint64_t seed, double* sums,
                              int64_t* dropped, void* ws, size_t ws_bytes, void* stream) {
  CellEdges ed = {};
  StFeats ft;
  int rc = pairs_check("stack_sums", patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  if ((rc = model_check("stack_sums", n_features, folds))) return rc;
  if ((rc = feats_check("stack_sums", feats, n_features, n > 0, &ft))) return rc;
  MMG_CHECK_ARG(n == 0 || target, "stack_sums: null target");
  MMG_CHECK_ARG(sums && dropped, "stack_sums: null output");
  SumsWs w;
  MMG_CHECK_WS("stack_sums", sums_carve(ws, n, folds * n_labs * n_bins, st_fields(n_features), &w));
  hipStream_t st = (hipStream_t)stream;
#define ST_FIT_SUMS(K_) \
  fit_sums<K_>(ft, target, patient, lab, index_bytes, n, n_labs, deg, n_patients, n_bins, ed, folds, seed, sums, dropped, w, st)
  switch (n_features) {
    case 1: return ST_FIT_SUMS(1);
    case 2: return ST_FIT_SUMS(2);
    case 3: return ST_FIT_SUMS(3);
    default: return ST_FIT_SUMS(4);
  }
#undef ST_FIT_SUMS
}

extern "C" size_t mmg_stack_solve_ws_bytes(int n_labs, int n_bins, int n_features, int folds) {
  if (!shape_ok(0, n_labs, n_bins) || !model_ok(n_features, folds)) return 0;
  SolveWs w;
  return solve_carve(nullptr, n_labs, n_bins, n_features, folds, &w);
}

extern "C" int mmg_stack_solve(const double* sums, int n_labs, int n_bins, int n_features, int folds, double ridge,
                               int64_t min_count, double* coef, int32_t* level, int32_t* n_used, void* ws, size_t ws_bytes,
                               void* stream) {
  MMG_CHECK_ARG(shape_ok(0, n_labs, n_bins), "stack_solve: %d labs x %d bins outside [1, %d] x [1, %d] or above %d cells",
                n_labs, n_bins, MMG_ST_MAX_LABS, MMG_ST_MAX_BINS, MMG_ST_MAX_CELLS);
  int rc = model_check("stack_solve", n_features, folds);
  if (rc) return rc;
  MMG_CHECK_ARG(ridge >= 0.0 && ridge <= 1.79e308, "stack_solve: ridge %g is negative or not finite", ridge);
  MMG_CHECK_ARG(min_count >= 0, "stack_solve: negative min_count");
  MMG_CHECK_ARG(sums && coef && level && n_used, "stack_solve: null sums or output");
  SolveWs w;
  MMG_CHECK_WS("stack_solve", solve_carve(ws, n_labs, n_bins, n_features, folds, &w));
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = n_labs * n_bins, F = st_fields(n_features), fo = folds > 1 ? folds + 1 : 1;
  const int64_t per_fold = (int64_t)n_cells * F;
  hipLaunchKernelGGL(k_st_train, dim3(launch_grid(per_fold * fo, ST_NTHR, ST_MAX_GRID, 1)), dim3(ST_NTHR), 0, st, sums,
                     per_fold, folds, fo, w.T);
  hipLaunchKernelGGL(k_st_group, dim3(launch_grid((int64_t)fo * n_labs * F, ST_NTHR, ST_MAX_GRID, 1)), dim3(ST_NTHR), 0, st,
                     w.T, (int64_t)fo * n_labs, n_bins, F, w.labs);
  hipLaunchKernelGGL(k_st_group, dim3(launch_grid((int64_t)fo * F, ST_NTHR, ST_MAX_GRID, 1)), dim3(ST_NTHR), 0, st, w.labs,
                     (int64_t)fo, n_labs, F, w.all);
  MMG_CHECK_LAUNCH("stack_solve(training sums)");
  const int64_t need_i = min_count > n_features + 2 ? min_count : n_features + 2;
  const double need = (double)need_i;
  const dim3 grid(launch_grid((int64_t)fo * n_cells, ST_NTHR, ST_MAX_GRID, 1)), block(ST_NTHR);
#define ST_SOLVE(K_) \
  hipLaunchKernelGGL(k_st_solve<K_>, grid, block, 0, st, w.T, w.labs, w.all, n_cells, n_bins, fo, ridge, need, coef, level, n_used)
  switch (n_features) {
    case 1: ST_SOLVE(1); break;
    case 2: ST_SOLVE(2); break;
    case 3: ST_SOLVE(3); break;
    default: ST_SOLVE(4); break;
  }
#undef ST_SOLVE
  MMG_CHECK_LAUNCH("stack_solve");
  return MMG_OK;
}

extern "C" int mmg_stack_apply_pairs(const float* const* feats, int n_features, const void* patient, const void* lab,
                                     int index_bytes, int64_t n, int n_labs, const int32_t* deg, int64_t n_patients,
                                     const double* bin_edges, int n_bins, const double* coef, int folds, uint64_t seed,
                                     int cross, float* out, void* stream) {
  CellEdges ed = {};
  StFeats ft;
  int rc = pairs_check("stack_apply_pairs", patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  if ((rc = model_check("stack_apply_pairs", n_features, folds))) return rc;
  if ((rc = feats_check("stack_apply_pairs", feats, n_features, n > 0, &ft))) return rc;
  MMG_CHECK_ARG(!cross || folds >= 2, "stack_apply_pairs: out-of-fold coefficients need folds >= 2, got %d", folds);
  MMG_CHECK_ARG(coef, "stack_apply_pairs: null coef");
  MMG_CHECK_ARG(n == 0 || out, "stack_apply_pairs: null output");
  if (n == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t rng_key = mmg_rng_key(seed, (uint32_t)MMG_ST_SITE);
  index_dispatch(index_bytes, [&](auto it) {
    using IT = decltype(it);
    hipLaunchKernelGGL(k_st_apply_pairs<IT>, dim3(launch_grid(n, ST_NTHR, ST_MAX_GRID)), dim3(ST_NTHR), 0, st, ft,
                       (const IT*)patient, (const IT*)lab, n, n_labs, deg, n_patients, n_bins, ed, coef, folds, rng_key,
                       cross, out);
  });
  MMG_CHECK_LAUNCH("stack_apply_pairs");
  return MMG_OK;
}

extern "C" int mmg_stack_apply_matrix(const float* const* feats, const int64_t* strides, int n_features, int64_t n_rows,
                                      int n_labs, const void* rows, int index_bytes, const int32_t* deg, int64_t n_patients,
                                      const double* bin_edges, int n_bins, const double* coef, int folds, uint64_t seed,
                                      int cross, float* out, int64_t ld_out, void* stream) {
  CellEdges ed = {};
  StFeats ft;
  const int some = 0;        // (a matrix has no index lists to be null)
  int rc = pairs_check("stack_apply_matrix", &some, &some, index_bytes, n_rows, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  if ((rc = model_check("stack_apply_matrix", n_features, folds))) return rc;
  if ((rc = feats_check("stack_apply_matrix", feats, n_features, n_rows > 0, &ft))) return rc;
  MMG_CHECK_ARG(strides, "stack_apply_matrix: null strides");
  for (int k = 0; k < n_features; ++k) {
    MMG_CHECK_ARG(strides[k] == 0 || strides[k] >= n_labs, "stack_apply_matrix: row stride %lld of feature %d (0 or >= %d)",
                  (long long)strides[k], k, n_labs);
    ft.ld[k] = strides[k];
  }
  MMG_CHECK_ARG(ld_out >= n_labs, "stack_apply_matrix: output row stride %lld below %d labs", (long long)ld_out, n_labs);
  MMG_CHECK_ARG(!cross || folds >= 2, "stack_apply_matrix: out-of-fold coefficients need folds >= 2, got %d", folds);
  MMG_CHECK_ARG(coef, "stack_apply_matrix: null coef");
  MMG_CHECK_ARG(n_rows == 0 || out, "stack_apply_matrix: null output");
  if (n_rows == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t rng_key = mmg_rng_key(seed, (uint32_t)MMG_ST_SITE);
  const dim3 grid(launch_grid(n_rows * n_labs, ST_NTHR, ST_MAX_GRID)), block(ST_NTHR);
  index_dispatch(rows ? index_bytes : 8, [&](auto it) {           // no row list: the int64 instance, which never reads it
    using IT = decltype(it);
    hipLaunchKernelGGL(k_st_apply_matrix<IT>, grid, block, 0, st, ft, n_rows, n_labs, (const IT*)rows, deg, n_patients,
                       n_bins, ed, coef, folds, rng_key, cross, out, ld_out);
  });
  MMG_CHECK_LAUNCH("stack_apply_matrix");
  return MMG_OK;
}

extern "C" size_t mmg_stack_scores_ws_bytes(int64_t n, int n_labs, int n_bins) {
  if (!shape_ok(n, n_labs, n_bins)) return 0;
  SumsWs w;
  return sums_carve(nullptr, n, n_labs * n_bins, MMG_ST_SCORE_FIELDS, &w);
}

extern "C" int mmg_stack_scores(const float* raw, const float* stacked, const float* target, const void* patient,
                                const void* lab, int index_bytes, int64_t n, int n_labs, const int32_t* deg,
                                int64_t n_patients, const double* bin_edges, int n_bins, double* scores, int64_t* dropped,
                                void* ws, size_t ws_bytes, void* stream) {
  CellEdges ed = {};
  int rc = pairs_check("stack_scores", patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(n == 0 || (raw && stacked && target), "stack_scores: null raw, stacked or target");
  MMG_CHECK_ARG(scores && dropped, "stack_scores: null output");
  const int n_cells = n_labs * n_bins, F = MMG_ST_SCORE_FIELDS;
  SumsWs w;
  MMG_CHECK_WS("stack_scores", sums_carve(ws, n, n_cells, F, &w));
  hipStream_t st = (hipStream_t)stream;
  StFeats ft = {};
  ft.K = 2;
  ft.f[0] = raw;
  ft.f[1] = stacked;
  ScoreTerms terms = {raw, stacked, target};
  // the cells land in the first n_cells rows of scores itself
  rc = sums_run("stack_scores", ft, target, patient, lab, index_bytes, n, n_labs, deg, n_patients, n_bins, ed, 1, 0, terms,
                scores, dropped, w, st);
  if (rc) return rc;
  double* lab_rows = scores + (size_t)n_cells * F;
  hipLaunchKernelGGL(k_st_group, dim3(launch_grid((int64_t)n_labs * F, ST_NTHR, ST_MAX_GRID, 1)), dim3(ST_NTHR), 0, st,
                     scores, (int64_t)n_labs, n_bins, F, lab_rows);
  hipLaunchKernelGGL(k_st_group, dim3(1), dim3(ST_NTHR), 0, st, lab_rows, (int64_t)1, n_labs, F, lab_rows + (size_t)n_labs * F);
  MMG_CHECK_LAUNCH("stack_scores(rows)");
  return MMG_OK;
}
