// Lab imputation by low-rank matrix completion (include/mmgnn_mf.h; mmgnn/lowrank.py): regularised alternating least
// squares over the observed (patient, lab, value) triples.  Every patient and every lab has one vector of r <= 32
// doubles; a half-sweep solves, for every segment of one ordering, the r x r ridge system of its pairs.
//   k_mf_keys .. k_mf_y   the index: one stable radix sort by (patient, lab), one by lab on top of it, the pointers from
//                         the sorted keys, the lab centres by the sum rule, y = value - centre in both orderings.
//   k_mf_jobcount         chunks of every segment longer than MMG_MF_SPLIT; their exclusive scan is the job list.
//   k_mf_jobs<NE>         one wave per (long segment, chunk): the chunk's sums of A | b to the workspace.
//   k_mf_segment<NE>      one wave per segment: the sums (chunk after chunk, or the workspace's chunk sums in ascending
//                         order), + reg, the Cholesky solve in LDS, the segment's vector.
//                         One lane owns NE of the r (r + 1) / 2 + r entries of A | b and adds a chunk's pairs to them one
//                         after the other from an LDS tile of MF_T gathered factor rows: the order of the header's rule.
//   k_mf_obj0 / k_mf_objsum   the three sums of the objective, level after level of the same rule.
//   k_mf_predict / k_mf_impute   clip(centre + u . v), one rounding; a patient's own values pass through.
// fp64 contraction is OFF for the whole file (solve and prediction restate numpy arithmetic operation by operation); the
// sums of A | b ask for their fused multiply-adds by name.  Built into libmmgnn_mf.so beside libmmgnn.so and on top of
// it (mmg_set_error).
#include "common.h"
#include "radix_sort.h"
#include "../../include/mmgnn_mf.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int MF_NTHR = 256;
constexpr int MF_CH = MMG_MF_CHUNK;
constexpr int MF_SPLIT = MMG_MF_SPLIT;
constexpr int MF_MR = MMG_MF_MAX_RANK;
constexpr int MF_ML = MMG_MF_MAX_LABS;
constexpr int MF_T = 32;                     // pairs whose factor rows are staged in LDS at a time
constexpr int MF_LD = MF_MR + 2;             // LDS row stride (doubles): r factor values, then y
constexpr int MF_JOB_GRID = 16384;           // workgroups of k_mf_jobs at the most
static_assert(MF_SPLIT % MF_CH == 0 && MF_CH % MF_T == 0 && MF_CH == 4 * WAVE, "whole chunks, whole tiles, 4 items a lane");
static_assert((MF_MR * (MF_MR + 1) / 2 + MF_MR + WAVE - 1) / WAVE <= 9, "at most nine entries of A | b per lane");

inline int mf_bits(int64_t n) {              // bits of the largest index n - 1
  int b = 0;
  while (b < 63 && ((int64_t)1 << b) < n) ++b;
  return b;
}
inline int mf_entries(int r) { return r * (r + 1) / 2 + r; }
inline int64_t mf_chunks(int64_t n) { return (n + MF_CH - 1) / MF_CH; }
// jobs of the split path at the most: a long segment has more than SPLIT = 8 CHUNK pairs, so its ceil(len / CHUNK)
// chunks are fewer than len / CHUNK * (1 + 1 / 8)
inline int64_t mf_job_cap(int64_t nnz) { return nnz * (MF_SPLIT / MF_CH + 1) / ((int64_t)MF_SPLIT) + 1; }
inline bool mf_finite_pos(double x) { return x > 0.0 && x <= 1.7976931348623157e308; }

__device__ __forceinline__ int64_t mf_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ============================================================================ the index
__global__ __launch_bounds__(MF_NTHR) void k_mf_keys(const long long* __restrict__ patient, const long long* __restrict__ lab,
                                                     int64_t nnz, int bl, unsigned long long* __restrict__ key,
                                                     int32_t* __restrict__ val) {
  const int64_t e = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (e >= nnz) return;
  key[e] = ((unsigned long long)patient[e] << bl) | ((unsigned long long)lab[e] & ((1ull << bl) - 1ull));
  val[e] = (int32_t)e;
}

__global__ __launch_bounds__(MF_NTHR) void k_mf_gather_a(const unsigned long long* __restrict__ key,
                                                         const int32_t* __restrict__ val, const float* __restrict__ value,
                                                         int64_t nnz, int bl, int32_t* __restrict__ p_idx,
                                                         float* __restrict__ p_val, int32_t* __restrict__ pat,
                                                         uint32_t* __restrict__ key_b, int32_t* __restrict__ val_b) {
  const int64_t q = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (q >= nnz) return;
  const unsigned long long k = key[q];
  const int32_t e = val[q];
  const uint32_t lb = (uint32_t)(k & ((1ull << bl) - 1ull));
  p_idx[q] = (int32_t)lb;
  p_val[q] = (e >= 0 && e < nnz) ? value[e] : 0.f;
  pat[q] = (int32_t)((k >> bl) & 0x7fffffffull);
  key_b[q] = lb;
  val_b[q] = (int32_t)q;
}

// ptr from the sorted segment ids: thread q writes the pointers of the segments that begin at q (thread nnz: the tail)
template <class Seg>
__global__ __launch_bounds__(MF_NTHR) void k_mf_ptr(const Seg* __restrict__ seg, int64_t nnz, int64_t n_seg,
                                                    long long* __restrict__ ptr) {
  const int64_t q = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (q > nnz) return;
  const int64_t prev = q > 0 ? (int64_t)seg[q - 1] : -1;
  int64_t cur = q < nnz ? (int64_t)seg[q] : n_seg;
  if (cur > n_seg) cur = n_seg;
  for (int64_t s = prev + 1; s <= cur; ++s) ptr[s] = q;
}

__global__ __launch_bounds__(MF_NTHR) void k_mf_gather_b(const int32_t* __restrict__ val_b, const int32_t* __restrict__ pat,
                                                         const float* __restrict__ p_val, int64_t nnz,
                                                         int32_t* __restrict__ l_idx, float* __restrict__ l_val) {
  const int64_t q = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (q >= nnz) return;
  const int32_t qa = val_b[q];
  const bool ok = qa >= 0 && qa < nnz;
  l_idx[q] = ok ? pat[qa] : 0;
  l_val[q] = ok ? p_val[qa] : 0.f;
}

// one workgroup per lab: the chunk sums of its values to the workspace, then thread 0 adds them in ascending order
__global__ __launch_bounds__(MF_NTHR) void k_mf_center(const long long* __restrict__ l_ptr, const float* __restrict__ l_val,
                                                       int64_t nnz, const double* __restrict__ fixed,
                                                       double* __restrict__ part, long long* __restrict__ count,
                                                       double* __restrict__ center) {
  const int l = (int)blockIdx.x;
  const int64_t beg = mf_clamp(l_ptr[l], 0, nnz), end = mf_clamp(l_ptr[l + 1], beg, nnz);
  const int64_t len = end - beg, nch = (len + MF_CH - 1) / MF_CH;
  double* __restrict__ mine = part + beg / MF_CH + l;                 // slots beg / CHUNK + l .. : disjoint lab to lab
  for (int64_t c = threadIdx.x; c < nch; c += MF_NTHR) {
    const int64_t q0 = beg + c * MF_CH, q1 = q0 + MF_CH < end ? q0 + MF_CH : end;
    double a = 0.0;
    for (int64_t q = q0; q < q1; ++q) a = a + (double)l_val[q];
    mine[c] = a;
  }
  __threadfence_block();
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    if (nch > 0) t = mine[0];
    for (int64_t c = 1; c < nch; ++c) t = t + mine[c];
    count[l] = (long long)len;
    center[l] = fixed ? fixed[l] : (len > 0 ? t / (double)len : 0.0);
  }
}

__global__ __launch_bounds__(MF_NTHR) void k_mf_y(const uint32_t* __restrict__ lab_sorted, const int32_t* __restrict__ val_b,
                                                  const float* __restrict__ l_val, const double* __restrict__ center,
                                                  int64_t nnz, int n_labs, double* __restrict__ l_y,
                                                  double* __restrict__ p_y) {
  const int64_t q = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (q >= nnz) return;
  const uint32_t lb = lab_sorted[q];
  const double yv = (double)l_val[q] - (lb < (uint32_t)n_labs ? center[lb] : 0.0);
  l_y[q] = yv;
  const int32_t qa = val_b[q];
  if (qa >= 0 && qa < nnz) p_y[qa] = yv;
}

// ============================================================================ the half-sweep
__global__ __launch_bounds__(MF_NTHR) void k_mf_jobcount(const long long* __restrict__ ptr, int64_t n_seg, int64_t nnz,
                                                         uint32_t* __restrict__ jp) {
  const int64_t s = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (s > n_seg) return;
  uint32_t c = 0;
  if (s < n_seg) {
    const int64_t beg = mf_clamp(ptr[s], 0, nnz), end = mf_clamp(ptr[s + 1], beg, nnz);
    if (end - beg > MF_SPLIT) c = (uint32_t)((end - beg + MF_CH - 1) / MF_CH);
  }
  jp[s] = c;
}

// entry e of A | b -> the two tile columns whose product it sums: (i, j <= i) of A, or (k, r) -- f_k times y -- of b
__device__ __forceinline__ void mf_entry(int e, int r, int& i, int& j) {
  const int tri = r * (r + 1) / 2;
  if (e >= tri + r) { i = 0; j = 0; return; }                 // no entry: a harmless product, never written
  if (e >= tri) { i = e - tri; j = r; return; }
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= e) ++i;
  j = e - i * (i + 1) / 2;
}

// the sums of one chunk q0 .. q1 (at most MF_CH pairs) onto 0, pair after pair; the whole wave calls it
template <int NE>
__device__ __forceinline__ void mf_chunk_sum(const int32_t* __restrict__ idx, const double* __restrict__ y, int64_t q0,
                                             int64_t q1, const double* __restrict__ F, int64_t m, int r, double* tile,
                                             const int (&ei)[NE], const int (&ej)[NE], double (&acc)[NE], int lane) {
#pragma unroll
  for (int q = 0; q < NE; ++q) acc[q] = 0.0;
  const int w = r + 1;
  for (int64_t t0 = q0; t0 < q1; t0 += MF_T) {
    const int cnt = (int)(q1 - t0 < MF_T ? q1 - t0 : MF_T);
    __syncthreads();                                          // the previous tile has been consumed
    for (int x = lane; x < cnt * w; x += WAVE) {
      const int p = x / w, k = x - p * w;
      double v;
      if (k == r) {
        v = y[t0 + p];
      } else {
        const int64_t id = idx[t0 + p];
        v = (id >= 0 && id < m) ? F[id * r + k] : 0.0;
      }
      tile[p * MF_LD + k] = v;
    }
    __syncthreads();
    for (int p = 0; p < cnt; ++p) {
      const double* row = tile + p * MF_LD;
#pragma unroll
      for (int q = 0; q < NE; ++q) acc[q] = fma(row[ei[q]], row[ej[q]], acc[q]);
    }
  }
}

__device__ __forceinline__ void mf_segment_range(const long long* __restrict__ ptr, int64_t s, int64_t nnz, int64_t& beg,
                                                 int64_t& end) {
  beg = mf_clamp(ptr[s], 0, nnz);
  end = mf_clamp(ptr[s + 1], beg, nnz);
}

template <int NE>
__global__ __launch_bounds__(WAVE) void k_mf_jobs(const long long* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                  const double* __restrict__ y, int64_t n_seg, int64_t nnz,
                                                  const double* __restrict__ F, int64_t m, int r,
                                                  const uint32_t* __restrict__ jp, int64_t cap,
                                                  double* __restrict__ part) {
  __shared__ double tile[MF_T * MF_LD];
  const int lane = threadIdx.x, E = r * (r + 1) / 2 + r;
  int ei[NE], ej[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) mf_entry(lane + WAVE * q, r, ei[q], ej[q]);
  int64_t total = jp[n_seg];
  if (total > cap) total = cap;
  for (int64_t job = blockIdx.x; job < total; job += gridDim.x) {
    int64_t lo = 0, hi = n_seg;                               // the largest s with jp[s] <= job
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)jp[mid] <= job) lo = mid; else hi = mid;
    }
    int64_t beg, end;
    mf_segment_range(ptr, lo, nnz, beg, end);
    const int64_t q0 = beg + (job - (int64_t)jp[lo]) * MF_CH;
    const int64_t q1 = q0 + MF_CH < end ? q0 + MF_CH : end;
    double acc[NE];
    mf_chunk_sum<NE>(idx, y, q0 < end ? q0 : end, q1, F, m, r, tile, ei, ej, acc, lane);
#pragma unroll
    for (int q = 0; q < NE; ++q) {
      const int e = lane + WAVE * q;
      if (e < E) part[job * E + e] = acc[q];
    }
  }
}

template <int NE>
__global__ __launch_bounds__(WAVE) void k_mf_segment(const long long* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ y, int64_t nnz,
                                                     const double* __restrict__ F, int64_t m, int r, double reg,
                                                     const uint32_t* __restrict__ jp, int64_t cap,
                                                     const double* __restrict__ part, double* __restrict__ out,
                                                     unsigned long long* __restrict__ bad, double* __restrict__ normal_out) {
  __shared__ double tile[MF_T * MF_LD];
  __shared__ double A[MF_MR * MF_LD];
  __shared__ double bv[MF_MR], dg[MF_MR];
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x, tri = r * (r + 1) / 2, E = tri + r;
  int64_t beg, end;
  mf_segment_range(ptr, s, nnz, beg, end);
  const int64_t len = end - beg;
  if (len == 0 && !normal_out) {                              // uniform over the workgroup
    if (lane < r) out[s * r + lane] = 0.0;
    return;
  }
  int ei[NE], ej[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) mf_entry(lane + WAVE * q, r, ei[q], ej[q]);
  double tot[NE], acc[NE];
#pragma unroll
  for (int q = 0; q < NE; ++q) tot[q] = 0.0;
  if (len > MF_SPLIT) {                                       // the chunk sums of k_mf_jobs, ascending
    const int64_t j0 = jp[s], nch = (len + MF_CH - 1) / MF_CH;
    for (int64_t c = 0; c < nch && j0 + c < cap; ++c) {
#pragma unroll
      for (int q = 0; q < NE; ++q) {
        const int e = lane + WAVE * q;
        const double v = e < E ? part[(j0 + c) * E + e] : 0.0;
        tot[q] = c == 0 ? v : tot[q] + v;
      }
    }
  } else {
    for (int64_t c0 = beg; c0 < end; c0 += MF_CH) {
      mf_chunk_sum<NE>(idx, y, c0, c0 + MF_CH < end ? c0 + MF_CH : end, F, m, r, tile, ei, ej, acc, lane);
#pragma unroll
      for (int q = 0; q < NE; ++q) tot[q] = c0 == beg ? acc[q] : tot[q] + acc[q];
    }
  }
#pragma unroll
  for (int q = 0; q < NE; ++q) {
    const int e = lane + WAVE * q;
    if (e < tri) {
      const double v = ei[q] == ej[q] ? tot[q] + reg : tot[q];
      A[ei[q] * MF_LD + ej[q]] = v;
      A[ej[q] * MF_LD + ei[q]] = v;
    } else if (e < E) {
      bv[ei[q]] = tot[q];
    }
  }
  __syncthreads();
  if (normal_out) {
    double* __restrict__ no = normal_out + s * (int64_t)(r * r + r);
    for (int x = lane; x < r * r + r; x += WAVE) no[x] = x < r * r ? A[(x / r) * MF_LD + x % r] : bv[x - r * r];
  }
  // the arithmetic of chol64.h (mmgnn/cholesky.py) on the lower triangle, element for element, in a mapping of its own:
  // every lane takes cells of the whole trailing block, where chol64.h's 32-column rows would leave most of a wave idle
  int nbad = 0;
  for (int k = 0; k < r; ++k) {
    __syncthreads();                                          // the trailing update of step k - 1 is complete
    const double piv = A[k * MF_LD + k];
    if (!(piv > 0.0)) ++nbad;
    const double d = sqrt(piv);
    if (lane == 0) dg[k] = d;
    const int i0 = k + 1 + lane;
    if (i0 < r) A[i0 * MF_LD + k] = A[i0 * MF_LD + k] / d;
    __syncthreads();
    const int mm = r - k - 1;
    for (int x = lane; x < mm * mm; x += WAVE) {
      const int i = k + 1 + x / mm, l = k + 1 + x % mm;
      if (l <= i) A[i * MF_LD + l] = A[i * MF_LD + l] - A[i * MF_LD + k] * A[l * MF_LD + k];
    }
  }
  for (int k = 0; k < r; ++k) {                               // forward: L z = b
    __syncthreads();
    const double yk = bv[k] / dg[k];
    __syncthreads();
    if (lane == 0) bv[k] = yk;
    const int i = k + 1 + lane;
    if (i < r) bv[i] = bv[i] - A[i * MF_LD + k] * yk;
  }
  for (int k = r - 1; k >= 0; --k) {                          // back: L^T x = z
    __syncthreads();
    const double xk = bv[k] / dg[k];
    __syncthreads();
    if (lane == 0) bv[k] = xk;
    if (lane < k) bv[lane] = bv[lane] - A[k * MF_LD + lane] * xk;
  }
  __syncthreads();
  if (lane < r) out[s * r + lane] = bv[lane];
  if (lane == 0 && nbad) atomicAdd(bad, (unsigned long long)nbad);        // an integer count: any order gives it
}

// ============================================================================ the objective
__device__ __forceinline__ double mf_dot(const double* __restrict__ u, const double* __restrict__ v, int r) {
  double t = 0.0;
  for (int k = 0; k < r; ++k) t = t + u[k] * v[k];
  return t;
}

// level 0: one wave per chunk of MF_CH items; MODE 0: item q = (y_q - u . v)^2 of pair q, MODE 1: item q = x_q^2
template <int MODE>
__global__ __launch_bounds__(WAVE) void k_mf_obj0(const long long* __restrict__ p_ptr, const int32_t* __restrict__ p_idx,
                                                  const double* __restrict__ x, int64_t n, int64_t n_patients, int n_labs,
                                                  const double* __restrict__ U, const double* __restrict__ V, int r,
                                                  double* __restrict__ out) {
  __shared__ double vals[MF_CH];
  const int lane = threadIdx.x;
  const int64_t q0 = (int64_t)blockIdx.x * MF_CH;
  const int cnt = (int)(n - q0 < MF_CH ? n - q0 : MF_CH);
  for (int t = lane; t < cnt; t += WAVE) {
    const int64_t q = q0 + t;
    double v;
    if (MODE == 1) {
      v = x[q] * x[q];
    } else {
      int64_t lo = 0, hi = n_patients;                        // the largest i with p_ptr[i] <= q
      while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (p_ptr[mid] <= q) lo = mid; else hi = mid;
      }
      const int lb = p_idx[q];
      const double tt = (lb >= 0 && lb < n_labs) ? mf_dot(U + lo * r, V + (int64_t)lb * r, r) : 0.0;
      const double d = x[q] - tt;
      v = d * d;
    }
    vals[t] = v;
  }
  __syncthreads();
  if (lane == 0) {
    double a = 0.0;
    for (int t = 0; t < cnt; ++t) a = a + vals[t];
    out[blockIdx.x] = a;
  }
}

// a further level: one thread per chunk of MF_CH chunk sums
__global__ __launch_bounds__(MF_NTHR) void k_mf_objsum(const double* __restrict__ in, int64_t n, double* __restrict__ out) {
  const int64_t c = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  const int64_t q0 = c * MF_CH;
  if (q0 >= n) return;
  const int64_t q1 = q0 + MF_CH < n ? q0 + MF_CH : n;
  double a = 0.0;
  for (int64_t q = q0; q < q1; ++q) a = a + in[q];
  out[c] = a;
}

__global__ void k_mf_set0(double* __restrict__ out) { out[0] = 0.0; }

// ============================================================================ prediction
__device__ __forceinline__ float mf_predict(const double* __restrict__ u, const double* __restrict__ v, int r, double c,
                                            double lo, double hi) {
  double t = c + mf_dot(u, v, r);
  t = fmax(t, lo);
  t = fmin(t, hi);
  return (float)t;
}

__global__ __launch_bounds__(MF_NTHR) void k_mf_predict(const long long* __restrict__ patient, const long long* __restrict__ lab,
                                                        int64_t n, const double* __restrict__ U, int64_t n_patients,
                                                        const double* __restrict__ V, int n_labs, int r,
                                                        const double* __restrict__ center, const long long* __restrict__ count,
                                                        double lo, double hi, float* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * MF_NTHR + threadIdx.x;
  if (e >= n) return;
  const int64_t i = patient[e], l = lab[e];
  float v = __builtin_nanf("");
  if (i >= 0 && i < n_patients && l >= 0 && l < n_labs && count[l] > 0) v = mf_predict(U + i * r, V + l * r, r, center[l], lo, hi);
  out[e] = v;
}

__global__ __launch_bounds__(MF_NTHR) void k_mf_impute(const long long* __restrict__ rows, const double* __restrict__ U,
                                                       int64_t n_patients, const double* __restrict__ V, int n_labs, int r,
                                                       const double* __restrict__ center, const long long* __restrict__ count,
                                                       double lo, double hi, const long long* __restrict__ p_ptr,
                                                       const int32_t* __restrict__ p_idx, const float* __restrict__ p_val,
                                                       int64_t nnz, float* __restrict__ out, int64_t ld_out) {
  __shared__ double su[MF_MR];
  const int64_t j = blockIdx.x;
  const int64_t i = rows ? rows[j] : j;
  const bool ok = i >= 0 && i < n_patients;                   // uniform over the workgroup
  float* __restrict__ o = out + j * ld_out;
  if (ok && threadIdx.x < r) su[threadIdx.x] = U[i * r + threadIdx.x];
  __syncthreads();
  for (int l = threadIdx.x; l < n_labs; l += MF_NTHR)
    o[l] = (ok && count[l] > 0) ? mf_predict(su, V + (int64_t)l * r, r, center[l], lo, hi) : __builtin_nanf("");
  if (!ok || !p_ptr) return;
  __threadfence_block();
  __syncthreads();                                            // the predictions of the row are written
  const int64_t beg = mf_clamp(p_ptr[i], 0, nnz), end = mf_clamp(p_ptr[i + 1], beg, nnz);
  for (int64_t q = beg + threadIdx.x; q < end; q += MF_NTHR) {
    const int lb = p_idx[q];
    if (lb >= 0 && lb < n_labs) o[lb] = p_val[q];
  }
}

// ============================================================================ host side
inline unsigned mf_grid(int64_t n) { return (unsigned)((n + MF_NTHR - 1) / MF_NTHR); }

struct IndexWs {
  unsigned long long *ka, *ka_alt;
  int32_t *va, *va_alt, *vb, *vb_alt, *pat;
  uint32_t *kb, *kb_alt, *hist, *scratch;
  float* l_val;
  double* part;
};
size_t index_carve(void* ws, int64_t nnz, int n_labs, IndexWs* w) {
  const size_t n = (size_t)(nnz > 0 ? nnz : 1);
  const RadixSizes rs = radix_sizes(nnz);
  MmgCarver c(ws);
  w->ka = c.take<unsigned long long>(n);
  w->ka_alt = c.take<unsigned long long>(n);
  w->va = c.take<int32_t>(n);
  w->va_alt = c.take<int32_t>(n);
  w->vb = c.take<int32_t>(n);
  w->vb_alt = c.take<int32_t>(n);
  w->pat = c.take<int32_t>(n);
  w->kb = c.take<uint32_t>(n);
  w->kb_alt = c.take<uint32_t>(n);
  w->hist = c.take<uint32_t>(rs.hist_elems);
  w->scratch = c.take<uint32_t>(rs.scratch_elems);
  w->l_val = c.take<float>(n);
  w->part = c.take<double>((size_t)(nnz / MF_CH + n_labs + 1));
  return c.need();
}

struct SweepWs {
  uint32_t *jp, *scratch;
  double* part;
};
size_t sweep_carve(void* ws, int64_t n_seg, int64_t nnz, int r, SweepWs* w) {
  MmgCarver c(ws);
  w->jp = c.take<uint32_t>((size_t)(n_seg + 1));
  w->scratch = c.take<uint32_t>(scan_scratch_elems(n_seg + 1));
  w->part = c.take<double>((size_t)mf_job_cap(nnz) * (size_t)mf_entries(r));
  return c.need();
}

struct ObjWs {
  double *a, *b;
};
size_t obj_carve(void* ws, int64_t nnz, int64_t n_patients, int n_labs, int r, ObjWs* w) {
  int64_t n = nnz;
  if (n_patients * r > n) n = n_patients * r;
  if ((int64_t)n_labs * r > n) n = (int64_t)n_labs * r;
  MmgCarver c(ws);
  w->a = c.take<double>((size_t)mf_chunks(n) + 1);
  w->b = c.take<double>((size_t)mf_chunks(mf_chunks(n)) + 1);
  return c.need();
}

inline bool mf_sizes_ok(int64_t nnz, int64_t n_patients, int n_labs) {
  return nnz >= 0 && nnz < INT32_MAX && n_patients >= 1 && n_patients < INT32_MAX && n_labs >= 1 && n_labs <= MF_ML;
}
inline bool mf_rank_ok(int r) { return r >= 1 && r <= MF_MR; }

int mf_check_sizes(const char* what, int64_t nnz, int64_t n_patients, int n_labs) {
  MMG_CHECK_ARG(nnz >= 0 && nnz < INT32_MAX, "%s: %lld pairs outside [0, 2^31)", what, (long long)nnz);
  MMG_CHECK_ARG(n_patients >= 1 && n_patients < INT32_MAX, "%s: %lld patients outside [1, 2^31)", what, (long long)n_patients);
  MMG_CHECK_ARG(n_labs >= 1 && n_labs <= MF_ML, "%s: %d labs outside [1, %d]", what, n_labs, MF_ML);
  return MMG_OK;
}
int mf_check_rank(const char* what, int r) {
  MMG_CHECK_ARG(mf_rank_ok(r), "%s: rank %d outside [1, %d]", what, r, MF_MR);
  return MMG_OK;
}

template <int NE>
void sweep_launch(const int64_t* ptr, const int32_t* idx, const double* y, int64_t n_seg, int64_t nnz, const double* other,
                  int64_t m, int r, double reg, double* out, int64_t* bad, double* normal_out, const SweepWs& w,
                  hipStream_t st) {
  const int64_t cap = mf_job_cap(nnz);
  if (nnz > MF_SPLIT) {                                       // else no segment can be long
    const unsigned g = (unsigned)(cap < MF_JOB_GRID ? cap : MF_JOB_GRID);
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, r, 1, 0, (k_mf_jobs<NE>), dim3(g), dim3(WAVE), 0, st, (const long long*)ptr, idx,
               y, n_seg, nnz, other, m, r, w.jp, cap, w.part);
  }
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, r, 2, 0, (k_mf_segment<NE>), dim3((unsigned)n_seg), dim3(WAVE), 0, st,
             (const long long*)ptr, idx, y, nnz, other, m, r, reg, w.jp, cap, w.part, out, (unsigned long long*)bad,
             normal_out);
}

// one of the three sums of the objective: level 0, then level after level until one value is left, which lands in dst
template <int MODE>
void obj_reduce(const int64_t* p_ptr, const int32_t* p_idx, const double* x, int64_t n, int64_t n_patients, int n_labs,
                const double* U, const double* V, int r, const ObjWs& w, double* dst, hipStream_t st) {
  if (n == 0) {
    hipLaunchKernelGGL(k_mf_set0, dim3(1), dim3(1), 0, st, dst);
    return;
  }
  int64_t cnt = mf_chunks(n);
  double *cur = cnt == 1 ? dst : w.a, *nxt = w.b;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, r, 3, 0, (k_mf_obj0<MODE>), dim3((unsigned)cnt), dim3(WAVE), 0, st,
             (const long long*)p_ptr, p_idx, x, n, n_patients, n_labs, U, V, r, cur);
  while (cnt > 1) {
    const int64_t up = mf_chunks(cnt);
    double* o = up == 1 ? dst : nxt;
    hipLaunchKernelGGL(k_mf_objsum, dim3(mf_grid(up)), dim3(MF_NTHR), 0, st, cur, cnt, o);
    nxt = cur;
    cur = o;
    cnt = up;
  }
}

}  // namespace

extern "C" int mmg_mf_plan(int64_t length, int* path, int64_t* chunks) {
  MMG_CHECK_ARG(length >= 0 && length < INT32_MAX, "mf_plan: length %lld outside [0, 2^31)", (long long)length);
  MMG_CHECK_ARG(path && chunks, "mf_plan: null pointer (path, chunks)");
  *path = length == 0 ? MMG_MF_PATH_EMPTY : (length <= MF_SPLIT ? MMG_MF_PATH_WAVE : MMG_MF_PATH_SPLIT);
  *chunks = mf_chunks(length);
  return MMG_OK;
}

extern "C" size_t mmg_mf_index_ws_bytes(int64_t nnz, int64_t n_patients, int n_labs) {
  if (!mf_sizes_ok(nnz, n_patients, n_labs)) return 0;
  IndexWs w;
  return index_carve(nullptr, nnz, n_labs, &w);
}

extern "C" int mmg_mf_index(const int64_t* patient, const int64_t* lab, const float* value, int64_t nnz, int64_t n_patients,
                            int n_labs, const double* center_fixed, int64_t* p_ptr, int32_t* p_idx, float* p_val, double* p_y,
                            int64_t* l_ptr, int32_t* l_idx, double* l_y, int64_t* count, double* center, void* ws,
                            size_t ws_bytes, void* stream) {
  if (int rc = mf_check_sizes("mf_index", nnz, n_patients, n_labs)) return rc;
  MMG_CHECK_ARG(nnz == 0 || (patient && lab && value && p_idx && p_val && p_y && l_idx && l_y),
                "mf_index: null pointer (patient, lab, value, p_idx, p_val, p_y, l_idx, l_y)");
  MMG_CHECK_ARG(p_ptr && l_ptr && count && center, "mf_index: null pointer (p_ptr, l_ptr, count, center)");
  IndexWs w;
  MMG_CHECK_WS("mf_index", index_carve(ws, nnz, n_labs, &w));
  hipStream_t st = (hipStream_t)stream;
  const int bl = mf_bits(n_labs), bp = mf_bits(n_patients);
  const unsigned g = mf_grid(nnz);
  RadixPairs<unsigned long long> a{w.ka, w.ka_alt, w.va, w.va_alt};
  RadixPairs<uint32_t> b{w.kb, w.kb_alt, w.vb, w.vb_alt};
  if (nnz > 0) {
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 0, 0, k_mf_keys, dim3(g), dim3(MF_NTHR), 0, st, (const long long*)patient,
               (const long long*)lab, nnz, bl, a.keys, a.vals);
    for (int shift = 0; shift < bl + bp; shift += 8) radix_pass<false>(a, nnz, shift, nullptr, w.hist, w.scratch, st);
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 1, 0, k_mf_gather_a, dim3(g), dim3(MF_NTHR), 0, st, a.keys, a.vals, value,
               nnz, bl, p_idx, p_val, w.pat, b.keys, b.vals);
  }
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 2, 0, (k_mf_ptr<int32_t>), dim3(mf_grid(nnz + 1)), dim3(MF_NTHR), 0, st, w.pat,
             nnz, n_patients, (long long*)p_ptr);
  if (nnz > 0) {
    for (int shift = 0; shift < bl; shift += 8) radix_pass<false>(b, nnz, shift, nullptr, w.hist, w.scratch, st);
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 3, 0, k_mf_gather_b, dim3(g), dim3(MF_NTHR), 0, st, b.vals, w.pat, p_val, nnz,
               l_idx, w.l_val);
  }
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 4, 0, (k_mf_ptr<uint32_t>), dim3(mf_grid(nnz + 1)), dim3(MF_NTHR), 0, st, b.keys,
             nnz, (int64_t)n_labs, (long long*)l_ptr);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 5, 0, k_mf_center, dim3((unsigned)n_labs), dim3(MF_NTHR), 0, st,
             (const long long*)l_ptr, w.l_val, nnz, center_fixed, w.part, (long long*)count, center);
  if (nnz > 0)
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nnz, n_labs, 6, 0, k_mf_y, dim3(g), dim3(MF_NTHR), 0, st, b.keys, b.vals, w.l_val, center,
               nnz, n_labs, l_y, p_y);
  MMG_CHECK_LAUNCH("mf_index");
  return MMG_OK;
}

extern "C" size_t mmg_mf_half_sweep_ws_bytes(int64_t segments, int64_t nnz, int r) {
  if (!(segments >= 1 && segments < INT32_MAX && nnz >= 0 && nnz < INT32_MAX && mf_rank_ok(r))) return 0;
  SweepWs w;
  return sweep_carve(nullptr, segments, nnz, r, &w);
}

extern "C" int mmg_mf_half_sweep(const int64_t* ptr, const int32_t* idx, const double* y, int64_t segments, int64_t nnz,
                                 const double* other, int64_t m, int r, double reg, double* out, int64_t* bad,
                                 double* normal_out, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(segments >= 1 && segments < INT32_MAX, "mf_half_sweep: %lld segments outside [1, 2^31)", (long long)segments);
  MMG_CHECK_ARG(nnz >= 0 && nnz < INT32_MAX, "mf_half_sweep: %lld pairs outside [0, 2^31)", (long long)nnz);
  MMG_CHECK_ARG(m >= 1 && m < INT32_MAX, "mf_half_sweep: %lld rows of the other side outside [1, 2^31)", (long long)m);
  if (int rc = mf_check_rank("mf_half_sweep", r)) return rc;
  MMG_CHECK_ARG(mf_finite_pos(reg), "mf_half_sweep: reg %g is not a positive finite number", reg);
  MMG_CHECK_ARG(ptr && other && out && bad, "mf_half_sweep: null pointer (ptr, other, out, bad)");
  MMG_CHECK_ARG(nnz == 0 || (idx && y), "mf_half_sweep: null pointer (idx, y)");
  SweepWs w;
  MMG_CHECK_WS("mf_half_sweep", sweep_carve(ws, segments, nnz, r, &w));
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, segments, r, 0, 0, k_mf_jobcount, dim3(mf_grid(segments + 1)), dim3(MF_NTHR), 0, st,
             (const long long*)ptr, segments, nnz, w.jp);
  exclusive_scan_u32(w.jp, segments + 1, w.scratch, st);
  const int ne = (mf_entries(r) + WAVE - 1) / WAVE;
#define MF_SWEEP(NE) sweep_launch<NE>(ptr, idx, y, segments, nnz, other, m, r, reg, out, bad, normal_out, w, st)
  if (ne <= 1) MF_SWEEP(1);
  else if (ne <= 2) MF_SWEEP(2);
  else if (ne <= 3) MF_SWEEP(3);
  else if (ne <= 4) MF_SWEEP(4);
  else if (ne <= 6) MF_SWEEP(6);
  else MF_SWEEP(9);
#undef MF_SWEEP
  MMG_CHECK_LAUNCH("mf_half_sweep");
  return MMG_OK;
}

extern "C" size_t mmg_mf_objective_ws_bytes(int64_t nnz, int64_t n_patients, int n_labs, int r) {
  if (!mf_sizes_ok(nnz, n_patients, n_labs) || !mf_rank_ok(r)) return 0;
  ObjWs w;
  return obj_carve(nullptr, nnz, n_patients, n_labs, r, &w);
}

extern "C" int mmg_mf_objective(const int64_t* p_ptr, const int32_t* p_idx, const double* p_y, int64_t nnz,
                                int64_t n_patients, int n_labs, const double* U, const double* V, int r, double* out,
                                void* ws, size_t ws_bytes, void* stream) {
  if (int rc = mf_check_sizes("mf_objective", nnz, n_patients, n_labs)) return rc;
  if (int rc = mf_check_rank("mf_objective", r)) return rc;
  MMG_CHECK_ARG(p_ptr && U && V && out, "mf_objective: null pointer (p_ptr, U, V, out)");
  MMG_CHECK_ARG(nnz == 0 || (p_idx && p_y), "mf_objective: null pointer (p_idx, p_y)");
  ObjWs w;
  MMG_CHECK_WS("mf_objective", obj_carve(ws, nnz, n_patients, n_labs, r, &w));
  hipStream_t st = (hipStream_t)stream;
  obj_reduce<0>(p_ptr, p_idx, p_y, nnz, n_patients, n_labs, U, V, r, w, out, st);
  obj_reduce<1>(nullptr, nullptr, U, n_patients * r, n_patients, n_labs, U, V, r, w, out + 1, st);
  obj_reduce<1>(nullptr, nullptr, V, (int64_t)n_labs * r, n_patients, n_labs, U, V, r, w, out + 2, st);
  MMG_CHECK_LAUNCH("mf_objective");
  return MMG_OK;
}

extern "C" int mmg_mf_predict_pairs(const int64_t* patient, const int64_t* lab, int64_t n, const double* U,
                                    int64_t n_patients, const double* V, int n_labs, int r, const double* center,
                                    const int64_t* count, double lo, double hi, float* out, void* stream) {
  if (int rc = mf_check_sizes("mf_predict_pairs", n, n_patients, n_labs)) return rc;
  if (int rc = mf_check_rank("mf_predict_pairs", r)) return rc;
  MMG_CHECK_ARG(lo < hi, "mf_predict_pairs: the clip [%g, %g] is empty", lo, hi);
  MMG_CHECK_ARG(U && V && center && count, "mf_predict_pairs: null pointer (U, V, center, count)");
  MMG_CHECK_ARG(n == 0 || (patient && lab && out), "mf_predict_pairs: null pointer (patient, lab, out)");
  if (n == 0) return MMG_OK;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, r, 0, 0, k_mf_predict, dim3(mf_grid(n)), dim3(MF_NTHR), 0, (hipStream_t)stream,
             (const long long*)patient, (const long long*)lab, n, U, n_patients, V, n_labs, r, center,
             (const long long*)count, lo, hi, out);
  MMG_CHECK_LAUNCH("mf_predict_pairs");
  return MMG_OK;
}

extern "C" int mmg_mf_impute_matrix(const int64_t* rows, int64_t n_rows, const double* U, int64_t n_patients, const double* V,
                                    int n_labs, int r, const double* center, const int64_t* count, double lo, double hi,
                                    const int64_t* p_ptr, const int32_t* p_idx, const float* p_val, int64_t nnz, float* out,
                                    int64_t ld_out, void* stream) {
  if (int rc = mf_check_sizes("mf_impute_matrix", nnz, n_patients, n_labs)) return rc;
  if (int rc = mf_check_rank("mf_impute_matrix", r)) return rc;
  MMG_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX, "mf_impute_matrix: %lld rows outside [0, 2^31)", (long long)n_rows);
  MMG_CHECK_ARG(ld_out >= n_labs, "mf_impute_matrix: ld_out %lld < n_labs %d", (long long)ld_out, n_labs);
  MMG_CHECK_ARG(lo < hi, "mf_impute_matrix: the clip [%g, %g] is empty", lo, hi);
  MMG_CHECK_ARG(U && V && center && count && p_ptr, "mf_impute_matrix: null pointer (U, V, center, count, p_ptr)");
  MMG_CHECK_ARG(nnz == 0 || (p_idx && p_val), "mf_impute_matrix: null pointer (p_idx, p_val)");
  MMG_CHECK_ARG(n_rows == 0 || out, "mf_impute_matrix: null pointer (out)");
  if (n_rows == 0) return MMG_OK;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n_rows, n_labs, r, 0, k_mf_impute, dim3((unsigned)n_rows), dim3(MF_NTHR), 0,
             (hipStream_t)stream, (const long long*)rows, U, n_patients, V, n_labs, r, center, (const long long*)count, lo, hi,
             (const long long*)p_ptr, p_idx, p_val, nnz, out, ld_out);
  MMG_CHECK_LAUNCH("mf_impute_matrix");
  return MMG_OK;
}
