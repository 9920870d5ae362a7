// The fp64 Cholesky solve of one small symmetric positive-definite system by one workgroup in LDS -- the solve of
// k_ch_solve (chain.hip, m <= 127) and k_pr_solve (prop.hip, m <= 129).  The host states the same arithmetic once,
// operation by operation (mmgnn/cholesky.py, host_cholesky_solve), and the tests hold the kernels EQUAL to it:
//   factor    right-looking and in place, k ascending: d_k = sqrt(a_kk); a pivot that is not > 0 is counted and the
//             arithmetic goes on; column k becomes a_ik / d_k; the trailing update a_il - a_ik * a_lk, l <= i, taken
//             NTHR / 32 rows by 32 columns at a time;
//   forward   k ascending: yk = y[k] / d_k into z[k], then y[i] - a_ik * yk for i > k;
//   back      k descending: wk = z[k] / d_k into y[k], then z[i] - a_ki * wk for i < k.
// A user writes the lower triangle of its system into `a` through an index functor (chol64_packed) and the right-hand
// side into y[0, m).  A product and a sum are two roundings: the function switches fp contraction off for its own body,
// wherever the includer put its pragma.
// k_mf_segment (mf.hip, m <= 32, one wave per system) does the same arithmetic per element with a thread mapping of its
// own: on this one a row of its trailing update fills at most m - 1 of 32 lanes, and its patient half-sweep at the x100
// shape measured 19 % (rank 8) and 13 % (rank 32) slower (profiles/solve_time.json).
#pragma once
#include <hip/hip_runtime.h>

constexpr int chol64_packed_size(int m) { return m * (m + 1) / 2; }              // doubles of the packed triangle

struct chol64_packed {                                                            // (i, l), l <= i
  __device__ __forceinline__ int operator()(int i, int l) const { return i * (i + 1) / 2 + l; }
};

// Every thread of a workgroup of NTHR threads calls it, no barrier needed before.  a, dg, y, z: LDS; dg, y and z hold m
// doubles.  On return (behind a barrier) y[0, m) is the solution and dg the pivots' square roots; a and z are used up.
// -> the pivots that were not > 0, the same in every thread.
template <int NTHR, class At>
__device__ __forceinline__ int chol64_solve(double* a, At at, int m, double* dg, double* y, double* z) {
#pragma clang fp contract(off)
  static_assert(NTHR >= 32 && NTHR % 32 == 0, "the trailing update takes NTHR / 32 rows by 32 columns at a time");
  const int tid = threadIdx.x, ty = tid >> 5, tx = tid & 31;
  int nbad = 0;
  for (int k = 0; k < m; ++k) {
    __syncthreads();                         // the trailing update of step k - 1 is complete
    const double piv = a[at(k, k)];
    if (!(piv > 0.0)) ++nbad;
    const double d = sqrt(piv);
    if (tid == 0) dg[k] = d;
    for (int i = k + 1 + tid; i < m; i += NTHR) a[at(i, k)] = a[at(i, k)] / d;
    __syncthreads();
    for (int i = k + 1 + ty; i < m; i += NTHR / 32) {
      const double aik = a[at(i, k)];
      for (int l = k + 1 + tx; l <= i; l += 32) a[at(i, l)] = a[at(i, l)] - aik * a[at(l, k)];
    }
  }
  for (int k = 0; k < m; ++k) {              // forward: L z = y
    __syncthreads();
    const double yk = y[k] / dg[k];
    if (tid == 0) z[k] = yk;
    for (int i = k + 1 + tid; i < m; i += NTHR) y[i] = y[i] - a[at(i, k)] * yk;
  }
  for (int k = m - 1; k >= 0; --k) {         // back: L^T y = z
    __syncthreads();
    const double wk = z[k] / dg[k];
    if (tid == 0) y[k] = wk;
    for (int i = tid; i < k; i += NTHR) z[i] = z[i] - a[at(k, i)] * wk;
  }
  __syncthreads();
  return nbad;
}
