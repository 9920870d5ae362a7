// Lab co-measurement and pairwise-complete correlation (include/mmgnn_assoc.h; mmgnn/association.py): over a patient x
// lab fp32 matrix with NaN for "not measured", the second moments of every lab pair over the rows that have BOTH labs --
// what pandas.DataFrame.corr / .cov(min_periods=) compute pair by pair on the host -- and the co-observation counts M^T M.
//   k_as_colsum   one read of X: per (64 columns, row slab) the fp64 sum, the count and the infinite cells of a column.
//   k_as_colfin   one workgroup: the slabs of a column in ascending order, ONE division; the infinite cells of all columns.
//   k_as_moments  grid (64 x 64 block pairs of the upper block triangle, row slabs): the walk of gram64.h.  A
//                 chunk of 32 rows is staged in LDS as ONE fp64 array per side: v = observed ? (double)x - center : NaN.
//                 The three operands of a side are derived from it in registers -- m = [v == v], u = m ? v : 0, q = u * u --
//                 so a side costs 32 x 66 doubles instead of three times that (two sides: 33,792 bytes; six staged operands
//                 would be 101,376 of the CU's 160 KB: one workgroup per CU).  NaN is
//                 the mask bit: an observed value equal to its centre is u = 0 with m = 1, which a zero could not tell.
//                 Each wave owns a 16 x 64 strip and six accumulations per 16 x 16 tile on v_mfma_f64_16x16x4_f64:
//                 m_a m_b, u_a m_b, q_a m_b, u_a u_b and, stored transposed for the lower halves of SX and SXX, m_a u_b and
//                 m_a q_b (not on a diagonal tile, whose direct products already cover both halves).
//   k_as_sum      one thread per cell and plane: the slabs in ascending order; N and SXY from a <= b to both (a, b), (b, a).
//   k_as_finish   one thread per cell: r, cov, jaccard, lift.
// fp64 contraction is OFF for the whole file: k_as_finish restates numpy arithmetic operation by operation, and q = u * u
// is a product rounded on its own.  Built into libmmgnn_assoc.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "gram64.h"
#include "../../include/mmgnn_assoc.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int AS_NTHR = GRAM64_NTHR;
constexpr int AS_PLANES = MMG_AS_PLANES;
static_assert(MMG_AS_TILE == GRAM64_TILE && MMG_AS_CHUNK == GRAM64_CHUNK, "the header publishes gram64.h's tile and chunk");
static_assert(MMG_AS_MIN_ROWS % MMG_AS_CHUNK == 0, "a slab is whole chunks");
static_assert(MMG_AS_MAX_LABS <= 512, "k_as_colfin is one workgroup of 512 threads");

struct AsPlan : Gram64Plan {
  int64_t stat_rows;
  int stat_slabs;
};
inline AsPlan as_plan(int64_t n, int L) {
  AsPlan p;
  static_cast<Gram64Plan&>(p) = gram64_plan(n, L, MMG_AS_BLOCKS, MMG_AS_MIN_ROWS);      // pairs <= 36
  p.stat_rows = (n + MMG_AS_STAT_SLABS - 1) / MMG_AS_STAT_SLABS;
  if (p.stat_rows < MMG_AS_STAT_MIN_ROWS) p.stat_rows = MMG_AS_STAT_MIN_ROWS;
  p.stat_slabs = (int)((n + p.stat_rows - 1) / p.stat_rows);
  return p;
}
inline bool as_shape_ok(int64_t n, int L) { return n >= 1 && n < INT32_MAX && L >= 1 && L <= MMG_AS_MAX_LABS; }

// ---- column statistics: grid (64-column blocks, slabs)
__global__ __launch_bounds__(AS_NTHR) void k_as_colsum(const float* __restrict__ X, int64_t n, int L, int64_t ld,
                                                       int64_t rows_per_slab, double* __restrict__ psum,
                                                       long long* __restrict__ pcnt, long long* __restrict__ pinf) {
  __shared__ double ss[4][64];
  __shared__ int sc[4][64];
  __shared__ int si[4][64];
  const int lc = threadIdx.x & 63, lr = threadIdx.x >> 6;
  const int col = 64 * (int)blockIdx.x + lc;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
  double s = 0.0;
  int c = 0, inf = 0;                                                 // a slab has fewer than 2^31 rows
  if (col < L) {
    const float* __restrict__ xc = X + col;
    for (int64_t r = r0 + lr; r < r1; r += 4) {
      const float x = xc[r * ld];
      if (mmg_finite(x)) { s += (double)x; ++c; }
      else if (x == x) ++inf;
    }
  }
  ss[lr][lc] = s; sc[lr][lc] = c; si[lr][lc] = inf;
  __syncthreads();
  if (lr == 0 && col < L) {
    double t = ss[0][lc];
    t += ss[1][lc]; t += ss[2][lc]; t += ss[3][lc];
    const size_t o = (size_t)blockIdx.y * L + col;
    psum[o] = t;
    pcnt[o] = (long long)sc[0][lc] + sc[1][lc] + sc[2][lc] + sc[3][lc];
    pinf[o] = (long long)si[0][lc] + si[1][lc] + si[2][lc] + si[3][lc];
  }
}

__global__ __launch_bounds__(512) void k_as_colfin(const double* __restrict__ psum, const long long* __restrict__ pcnt,
                                                   const long long* __restrict__ pinf, int slabs, int L,
                                                   long long* __restrict__ count, double* __restrict__ mean,
                                                   long long* __restrict__ n_inf) {
  __shared__ long long sinf[512];
  const int c = threadIdx.x;
  double s = 0.0;
  long long cnt = 0, inf = 0;
  if (c < L) {
    int q = 0;
    for (; q + 7 < slabs; q += 8) {                             // eight slabs' loads in flight, added in slab order
      double v[8];
      long long vc[8], vi[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const size_t o = (size_t)(q + k) * L + c;
        v[k] = psum[o]; vc[k] = pcnt[o]; vi[k] = pinf[o];
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) { s += v[k]; cnt += vc[k]; inf += vi[k]; }
    }
    for (; q < slabs; ++q) {
      const size_t o = (size_t)q * L + c;
      s += psum[o]; cnt += pcnt[o]; inf += pinf[o];
    }
    count[c] = cnt;
    mean[c] = cnt > 0 ? s / (double)cnt : 0.0;
  }
  sinf[c] = inf;
  __syncthreads();
  if (c == 0) {
    long long t = 0;
    for (int q = 0; q < L; ++q) t += sinf[q];
    n_inf[0] = t;
  }
}

// ---- moments: grid (block pairs of the upper triangle, slabs).  Two workgroups per CU: the 96 accumulator doubles of a
// lane and the rest fit 256 registers without scratch, and a second workgroup covers the other's staging of a chunk.
struct AsAcc {
  gram64_d4 aN[4] = {}, aX[4] = {}, aXX[4] = {}, aXY[4] = {}, tX[4] = {}, tXX[4] = {};
  double am, au, aq;
  __device__ __forceinline__ void row(double av, bool) {
    const bool ao = av == av;
    am = ao ? 1.0 : 0.0;
    au = ao ? av : 0.0;
    aq = au * au;
  }
  __device__ __forceinline__ void tile(int j, double bv, bool both) {
    const bool bo = bv == bv;
    const double bm = bo ? 1.0 : 0.0, bu = bo ? bv : 0.0;
    aN[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bm, aN[j], 0, 0, 0);
    aX[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bm, aX[j], 0, 0, 0);
    aXX[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(aq, bm, aXX[j], 0, 0, 0);
    aXY[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(au, bu, aXY[j], 0, 0, 0);
    if (both) {
      const double bq = bu * bu;
      tX[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bu, tX[j], 0, 0, 0);
      tXX[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(am, bq, tXX[j], 0, 0, 0);
    }
  }
};

__global__ __launch_bounds__(AS_NTHR, 2) void k_as_moments(const float* __restrict__ X, int64_t n, int L, int64_t ld,
                                                        const double* __restrict__ center, int64_t rows_per_slab, int nb,
                                                        double* __restrict__ partial) {
  __shared__ double As[GRAM64_SIDE], Bs[GRAM64_SIDE];
  const Gram64Tile t(nb, L, n, rows_per_slab);
  const double mua = t.a_in ? center[t.ca] : 0.0, mub = t.b_in ? center[t.cb] : 0.0;
  const double missing = __builtin_nan("");
  AsAcc acc;
  gram64_walk(t, L, As, Bs, acc, [=](int64_t r, bool live, double& a, double& b) {
    float xa = 0.f, xb = 0.f;
    if (live && t.a_in) xa = X[r * ld + t.ca];
    if (!t.diag && live && t.b_in) xb = X[r * ld + t.cb];
    a = (live && t.a_in && mmg_finite(xa)) ? (double)xa - mua : missing;
    if (!t.diag) b = (live && t.b_in && mmg_finite(xb)) ? (double)xb - mub : missing;
  });
  const size_t ll = (size_t)L * L;
  double* __restrict__ out = partial + (size_t)blockIdx.y * AS_PLANES * ll;
  gram64_store_tiles(t, L, [&](int j, bool both) {
    gram64_put(t, L, j, acc.aN[j], out);
    gram64_put(t, L, j, acc.aX[j], out + ll);
    gram64_put(t, L, j, acc.aXX[j], out + 2 * ll);
    gram64_put(t, L, j, acc.aXY[j], out + 3 * ll);
    if (both) {                                                 // the lower halves of SX and SXX
      gram64_put(t, L, j, acc.tX[j], out + ll, true);
      gram64_put(t, L, j, acc.tXX[j], out + 2 * ll, true);
    }
  });
}

// grid (cells / 256, planes): N and SXY are symmetric, SX and SXX are not
__global__ __launch_bounds__(AS_NTHR) void k_as_sum(const double* __restrict__ partial, int slabs, int L,
                                                    double* __restrict__ out) {
  const int idx = (int)blockIdx.x * AS_NTHR + threadIdx.x;
  const int plane = (int)blockIdx.y;
  const size_t ll = (size_t)L * L;
  const bool sym = plane == 0 || plane == 3;
  if (idx < L * L) gram64_sum_cell<4>(partial + plane * ll, AS_PLANES * ll, slabs, L, idx, sym, out + plane * ll);
}

// ---- r, cov, jaccard, lift: one thread per cell, every operation rounded on its own
__global__ __launch_bounds__(AS_NTHR) void k_as_finish(const double* __restrict__ mom, const long long* __restrict__ count,
                                                       int L, double n, double min_periods, double* __restrict__ r_out,
                                                       double* __restrict__ cov_out, double* __restrict__ jac_out,
                                                       double* __restrict__ lift_out) {
  const int idx = (int)blockIdx.x * AS_NTHR + threadIdx.x;
  if (idx >= L * L) return;
  const int a = idx / L, b = idx % L;
  const size_t ll = (size_t)L * L, ab = (size_t)idx, ba = (size_t)b * L + a;
  const double nan = __builtin_nan("");
  const double nab = mom[ab], sx = mom[ll + ab], sy = mom[ll + ba], sxx = mom[2 * ll + ab], syy = mom[2 * ll + ba],
               sxy = mom[3 * ll + ab];
  const double ca = (double)count[a], cb = (double)count[b];
  const double cxy = sxy - sx * sy / nab, vx = sxx - sx * sx / nab, vy = syy - sy * sy / nab;
  const double need_cov = min_periods > 2.0 ? min_periods : 2.0, need_r = min_periods > 1.0 ? min_periods : 1.0;
  cov_out[idx] = nab >= need_cov ? cxy / (nab - 1.0) : nan;
  const double den = vx * vy;
  double r = nan;
  if (nab >= need_r && den > 0.0) {
    r = cxy / sqrt(den);
    r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
  }
  r_out[idx] = r;
  const double uni = ca + cb - nab;
  jac_out[idx] = uni == 0.0 ? nan : nab / uni;
  lift_out[idx] = (nab * n) / (ca * cb);
}

struct StatWs {
  double* psum;
  long long *pcnt, *pinf;
};
size_t stat_carve(void* ws, int64_t n, int L, StatWs* w) {
  const AsPlan p = as_plan(n, L);
  MmgCarver c(ws);
  const size_t m = (size_t)p.stat_slabs * L;
  *w = StatWs{c.take<double>(m), c.take<long long>(m), c.take<long long>(m)};
  return c.need();
}
size_t moments_carve(void* ws, int64_t n, int L, double** partial) {
  const AsPlan p = as_plan(n, L);
  MmgCarver c(ws);
  *partial = c.take<double>((size_t)p.slabs * AS_PLANES * L * L);
  return c.need();
}

int as_check_shape(const char* what, int64_t n, int L, int64_t ld_x) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "%s: n %lld outside [1, 2^31)", what, (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= MMG_AS_MAX_LABS, "%s: %d labs outside [1, %d]", what, L, MMG_AS_MAX_LABS);
  MMG_CHECK_ARG(ld_x >= L, "%s: ld_x %lld < L %d", what, (long long)ld_x, L);
  return MMG_OK;
}

}  // namespace

extern "C" int mmg_assoc_plan(int64_t n, int L, int64_t* rows_per_slab, int* slabs) {
  MMG_CHECK_ARG(as_shape_ok(n, L), "assoc_plan: n %lld outside [1, 2^31) or %d labs outside [1, %d]", (long long)n, L,
                MMG_AS_MAX_LABS);
  MMG_CHECK_ARG(rows_per_slab && slabs, "assoc_plan: null pointer (rows_per_slab, slabs)");
  const AsPlan p = as_plan(n, L);
  *rows_per_slab = p.rows;
  *slabs = p.slabs;
  return MMG_OK;
}

extern "C" size_t mmg_assoc_colstats_ws_bytes(int64_t n, int L) {
  if (!as_shape_ok(n, L)) return 0;
  StatWs w;
  return stat_carve(nullptr, n, L, &w);
}

extern "C" int mmg_assoc_colstats(const float* X, int64_t n, int L, int64_t ld_x, int64_t* count, double* mean,
                                  int64_t* n_inf, void* ws, size_t ws_bytes, void* stream) {
  if (int rc = as_check_shape("assoc_colstats", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(X && count && mean && n_inf, "assoc_colstats: null pointer (X, count, mean, n_inf)");
  StatWs w;
  MMG_CHECK_WS("assoc_colstats", stat_carve(ws, n, L, &w));
  const AsPlan p = as_plan(n, L);
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, 0, 0, k_as_colsum, dim3((unsigned)((L + 63) / 64), (unsigned)p.stat_slabs),
             dim3(AS_NTHR), 0, st, X, n, L, ld_x, p.stat_rows, w.psum, w.pcnt, w.pinf);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.stat_slabs, L, 0, 0, k_as_colfin, dim3(1), dim3(512), 0, st, w.psum, w.pcnt, w.pinf,
             p.stat_slabs, L, (long long*)count, mean, (long long*)n_inf);
  MMG_CHECK_LAUNCH("assoc_colstats");
  return MMG_OK;
}

extern "C" size_t mmg_assoc_moments_ws_bytes(int64_t n, int L) {
  if (!as_shape_ok(n, L)) return 0;
  double* partial;
  return moments_carve(nullptr, n, L, &partial);
}

extern "C" int mmg_assoc_moments(const float* X, int64_t n, int L, int64_t ld_x, const double* center, double* out,
                                 void* ws, size_t ws_bytes, void* stream) {
  if (int rc = as_check_shape("assoc_moments", n, L, ld_x)) return rc;
  MMG_CHECK_ARG(X && center && out, "assoc_moments: null pointer (X, center, out)");
  double* partial;
  MMG_CHECK_WS("assoc_moments", moments_carve(ws, n, L, &partial));
  const AsPlan p = as_plan(n, L);
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, L, L, 0, k_as_moments, dim3((unsigned)p.pairs, (unsigned)p.slabs), dim3(AS_NTHR), 0,
             st, X, n, L, ld_x, center, p.rows, p.nb, partial);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.slabs, L, L, 0, k_as_sum, dim3((unsigned)((L * L + AS_NTHR - 1) / AS_NTHR), AS_PLANES),
             dim3(AS_NTHR), 0, st, partial, p.slabs, L, out);
  MMG_CHECK_LAUNCH("assoc_moments");
  return MMG_OK;
}

// one launch that keeps nothing: no workspace today (ws may be null)
extern "C" size_t mmg_assoc_finish_ws_bytes(int L) { return 0; }

extern "C" int mmg_assoc_finish(const double* moments, const int64_t* count, int L, int64_t n, int64_t min_periods,
                                double* r, double* cov, double* jaccard, double* lift, void* ws, size_t ws_bytes,
                                void* stream) {
  MMG_CHECK_ARG(L >= 1 && L <= MMG_AS_MAX_LABS, "assoc_finish: %d labs outside [1, %d]", L, MMG_AS_MAX_LABS);
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "assoc_finish: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(min_periods >= 0 && min_periods <= INT32_MAX, "assoc_finish: min_periods %lld outside [0, 2^31)",
                (long long)min_periods);
  MMG_CHECK_ARG(moments && count && r && cov && jaccard && lift,
                "assoc_finish: null pointer (moments, count, r, cov, jaccard, lift)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, L, L, 0, 0, k_as_finish, dim3((unsigned)((L * L + AS_NTHR - 1) / AS_NTHR)), dim3(AS_NTHR),
             0, (hipStream_t)stream, moments, (const long long*)count, L, (double)n, (double)min_periods, r, cov, jaccard, lift);
  MMG_CHECK_LAUNCH("assoc_finish");
  return MMG_OK;
}
