// Split-conformal prediction intervals for imputed labs (include/mmgnn_conformal.h; mmgnn/conformal.py): exact order
// statistics of the residuals per (lab, degree bin) cell, per lab and over all pairs, the table that takes the first
// usable of the three, and the epilogues that turn predictions into (point, lower, upper) and count their coverage.
//   k_sos_keys        key = (segment << 32) | float_orderable (segsort.h); rows of no segment (and NaN keys) go under segment
//                     n_seg and sort last.  The lab and the all-pairs level of a fit are the cell ids divided by n_bins
//                     and by n_cells: one array of cell ids serves the three sorts.
//   segsort_run       the stable sort of segsort.h over the 4 key digits and the 1-2 segment digits that can
//                     differ (the host knows n_seg: the digits above it are never sorted).  The int32 payload the sort
//                     carries is not used here and is never initialised.
//   k_sos_pick        one thread per segment: two binary searches for its bounds in the sorted keys, the fp64 rank
//                     arithmetic (contraction off: every operation rounded on its own, as Python forms it), the picks.
//   k_cf_prepare      ONE read of the pairs: fp32 residual key, cell id, the four kinds of dropped pairs (integer counts:
//                     per-wave sums, one integer atomic per workgroup and kind).
//   k_cf_resolve      one thread per cell: first usable of (cell, lab, all).
//   k_cf_apply_pairs  one thread per pair; the table sits in LDS when it fits (<= CF_LDS_CELLS cells), the bin edges are
//                     kernel arguments (scalar loads).
//   k_cf_apply_matrix pure streaming, 4 B read and 12 B written per cell.  A workgroup walks blocks of R consecutive rows:
//                     the degree bin of each row is taken once into LDS, then the block's cells are walked in memory
//                     order, lane after lane along the lab axis, VEC = 4 / 2 / 1 floats per lane as the alignment of the
//                     four matrices allows (a [n, 50] matrix has 8-byte aligned rows: VEC = 2).
//   k_cf_cov_keys / k_cf_cov_cells   coverage: a stable sort of the pair ids by cell groups every cell's pairs in input
//                     order; one workgroup per cell then holds the cell's table row in registers, gathers its pairs and
//                     sums in a fixed order.  No atomics.
// Built into libmmgnn_conformal.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "cells.h"
#include "radix_sort.h"
#include "../../include/mmgnn_conformal.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int CF_NTHR = 256;
constexpr int CF_MAX_GRID = 2048;
constexpr int CF_LDS_CELLS = 4096;        // 3 fp32 per cell: 48 KB of LDS
constexpr int CF_MAX_ROWS = 256;          // rows of a block of the matrix kernel
constexpr int CF_BLOCK_CELLS = 8192;      // cells of a block: R = CF_BLOCK_CELLS / n_labs rows
static_assert(MMG_CF_MAX_BINS == MMG_AN_MAX_BINS, "the degree bins of mmg_pair_analysis");
static_assert(MMG_CF_MAX_CELLS <= 65536, "the coverage sort runs over two digits of the cell");

struct CfRanks {
  double a_lo, a_hi;      // alpha / 2 and 1 - alpha / 2 (signed), unused and 1 - alpha (absolute)
  int mode;
  long long min_count;
};

// the fp32 value in the low half of a sort key
__device__ __forceinline__ float cf_key_value(unsigned long long k) { return orderable_float((uint32_t)k); }

// ---------------------------------------------------------------------------------- segmented order statistics
__global__ __launch_bounds__(CF_NTHR) void k_sos_keys(const float* __restrict__ keys, const int32_t* __restrict__ seg,
                                                      int64_t n, int n_seg_in, int div, int n_seg,
                                                      unsigned long long* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * CF_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * CF_NTHR + threadIdx.x; i < n; i += step) {
    const float x = keys[i];
    const int s = seg[i];
    const bool ok = s >= 0 && s < n_seg_in && x == x;
    const uint32_t se = ok ? (uint32_t)(s / div) : (uint32_t)n_seg;
    out[i] = ((unsigned long long)se << 32) | (unsigned long long)(ok ? float_orderable(x) : 0u);
  }
}

__global__ __launch_bounds__(CF_NTHR) void k_sos_pick(const unsigned long long* __restrict__ K, int64_t n, int n_seg,
                                                      CfRanks rk, int32_t* __restrict__ count, float* __restrict__ q_lo,
                                                      float* __restrict__ q_hi, float* __restrict__ shift,
                                                      int32_t* __restrict__ usable) {
#pragma clang fp contract(off)
  const int s = blockIdx.x * CF_NTHR + threadIdx.x;
  if (s >= n_seg) return;
  const int64_t lo = lower_bound(K, n, (unsigned long long)s << 32);
  const int64_t hi = lower_bound(K, n, (unsigned long long)(s + 1) << 32);
  const int64_t m = hi - lo;
  const double m1 = (double)(m + 1);
  const int64_t k_hi = (int64_t)ceil(m1 * rk.a_hi);
  const bool has_hi = k_hi <= m;                              // (k_hi >= 1 always)
  const float h = has_hi ? cf_key_value(K[lo + k_hi - 1]) : INFINITY;
  float l, sh = 0.f;
  bool ok = has_hi;
  if (rk.mode == MMG_CF_SIGNED) {
    const int64_t k_lo = (int64_t)floor(m1 * rk.a_lo);        // <= m for m >= 1
    ok = ok && k_lo >= 1;
    l = k_lo >= 1 ? cf_key_value(K[lo + k_lo - 1]) : -INFINITY;
    if (m > 0) {
      if (m & 1) {
        sh = cf_key_value(K[lo + (m >> 1)]);
      } else {
        const float a = cf_key_value(K[lo + (m >> 1) - 1]), b = cf_key_value(K[lo + (m >> 1)]);
        const float sum = a + b;
        sh = sum * 0.5f;
      }
    }
  } else {
    l = -h;
  }
  count[s] = (int32_t)m;
  q_lo[s] = l;
  q_hi[s] = h;
  shift[s] = sh;
  usable[s] = (ok && m >= rk.min_count) ? 1 : 0;
}

using SosWs = SegSortWs<unsigned long long>;
size_t sos_carve(MmgCarver& c, int64_t n, SosWs* w) {
  segsort_carve(c, n, w);
  return c.need();
}

struct SosOut {
  int32_t* count;
  float *q_lo, *q_hi, *shift;
  int32_t* usable;
};

// the statistics of the segments seg[i] / div (seg[i] in [0, n_seg_in), anything else: no segment); w by value: the
// passes swap its buffers
int sos_run(const char* what, const float* keys, const int32_t* seg, int64_t n, int n_seg_in, int div, const CfRanks& rk,
            const SosOut& o, SosWs w, hipStream_t st) {
  const int n_seg = (n_seg_in + div - 1) / div;
  if (n > 0) {
    hipLaunchKernelGGL(k_sos_keys, dim3(launch_grid(n, CF_NTHR, CF_MAX_GRID)), dim3(CF_NTHR), 0, st, keys, seg, n, n_seg_in,
                       div, n_seg, w.kv.keys);
    MMG_CHECK_LAUNCH(what);
    segsort_run(w, n, 32 + bits_of((unsigned)n_seg), st);              // segment values reach n_seg itself
    MMG_CHECK_LAUNCH(what);
  }
  hipLaunchKernelGGL(k_sos_pick, dim3((n_seg + CF_NTHR - 1) / CF_NTHR), dim3(CF_NTHR), 0, st, w.kv.keys, n, n_seg, rk,
                     o.count, o.q_lo, o.q_hi, o.shift, o.usable);
  MMG_CHECK_LAUNCH(what);
  return MMG_OK;
}

int ranks_check(const char* what, double alpha, int mode, int64_t min_count, CfRanks* rk) {
  MMG_CHECK_ARG(alpha > 0.0 && alpha < 1.0, "%s: alpha %g outside (0, 1)", what, alpha);
  MMG_CHECK_ARG(mode == MMG_CF_SIGNED || mode == MMG_CF_ABSOLUTE, "%s: unknown score mode %d", what, mode);
  MMG_CHECK_ARG(min_count >= 0, "%s: negative min_count", what);
  rk->mode = mode;
  rk->min_count = (long long)min_count;
  const double half = alpha / 2.0;
  rk->a_lo = half;
  rk->a_hi = mode == MMG_CF_SIGNED ? 1.0 - half : 1.0 - alpha;
  return MMG_OK;
}

// ---------------------------------------------------------------------------------- pairs -> cells
int pairs_check(const char* what, const void* pred, const void* patient, const void* lab, int index_bytes, int64_t n, int L,
                const int32_t* deg, int64_t n_pat, const double* edges, int B, CellEdges* ed) {
  const int rc = cells_check(what, index_bytes, n, L, n_pat, edges, B, ed);
  if (rc != MMG_OK) return rc;
  MMG_CHECK_ARG(n == 0 || (pred && patient && lab), "%s: null pred, patient or lab", what);
  MMG_CHECK_ARG(n_pat == 0 || deg, "%s: null deg", what);
  return MMG_OK;
}

template <class IT>
__global__ __launch_bounds__(CF_NTHR) void k_cf_prepare(const float* __restrict__ pred, const float* __restrict__ target,
                                                        const IT* __restrict__ patient, const IT* __restrict__ lab,
                                                        int64_t n, int L, const int32_t* __restrict__ deg, int64_t n_pat,
                                                        int B, CellEdges ed, int mode, float* __restrict__ key,
                                                        int32_t* __restrict__ cell, unsigned long long* dropped) {
  __shared__ int s_drop[CF_NTHR / WAVE][MMG_CF_DROP_KINDS];
  int drop[MMG_CF_DROP_KINDS] = {0, 0, 0, 0};
  const int64_t step = (int64_t)gridDim.x * CF_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * CF_NTHR + threadIdx.x; i < n; i += step) {
    int c = pair_cell(patient, lab, i, L, deg, n_pat, ed, B);
    const float r = target[i] - pred[i];
    const float k = mode == MMG_CF_SIGNED ? r : fabsf(r);
    if (c >= 0 && k != k) c = -4;
#pragma unroll
    for (int q = 0; q < MMG_CF_DROP_KINDS; ++q) drop[q] += (c == -1 - q) ? 1 : 0;
    key[i] = k;
    cell[i] = c >= 0 ? c : L * B;
  }
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < MMG_CF_DROP_KINDS; ++q) {
    const int s = wave_sum_i(drop[q]);           // a thread takes at most 2^31 / (grid x 256) pairs: no overflow
    if (lane == 0) s_drop[wid][q] = s;
  }
  __syncthreads();
  if (threadIdx.x < MMG_CF_DROP_KINDS) {
    unsigned long long t = 0;
    for (int w = 0; w < CF_NTHR / WAVE; ++w) t += (unsigned long long)s_drop[w][threadIdx.x];
    if (t) atomicAdd(&dropped[threadIdx.x], t);  // integer: the order cannot change the result
  }
}

__global__ __launch_bounds__(CF_NTHR) void k_cf_resolve(SosOut c, SosOut l, SosOut a, int n_cells, int B,
                                                        float* __restrict__ table, int32_t* __restrict__ level,
                                                        int32_t* __restrict__ n_used) {
  const int i = blockIdx.x * CF_NTHR + threadIdx.x;
  if (i >= n_cells) return;
  const int lab = i / B;
  float lo = -INFINITY, hi = INFINITY, sh = 0.f;
  int lv = 3, nu = 0;
  if (c.usable[i]) {
    lo = c.q_lo[i]; hi = c.q_hi[i]; sh = c.shift[i]; nu = c.count[i]; lv = 0;
  } else if (l.usable[lab]) {
    lo = l.q_lo[lab]; hi = l.q_hi[lab]; sh = l.shift[lab]; nu = l.count[lab]; lv = 1;
  } else if (a.usable[0]) {
    lo = a.q_lo[0]; hi = a.q_hi[0]; sh = a.shift[0]; nu = a.count[0]; lv = 2;
  }
  table[i] = lo;
  table[n_cells + i] = hi;
  table[2 * n_cells + i] = sh;
  level[i] = lv;
  n_used[i] = nu;
}

void sos_out_carve(MmgCarver& c, int n_seg, SosOut* o) {
  o->count = c.take<int32_t>(n_seg);
  o->q_lo = c.take<float>(n_seg);
  o->q_hi = c.take<float>(n_seg);
  o->shift = c.take<float>(n_seg);
  o->usable = c.take<int32_t>(n_seg);
}
struct FitWs {
  float* key;
  int32_t* cell;
  SosOut lv[3];
  SosWs sos;
};
size_t fit_carve(void* ws, int64_t n, int L, int B, FitWs* w) {
  MmgCarver c(ws);
  const size_t nn = (size_t)(n > 0 ? n : 1);
  w->key = c.take<float>(nn);
  w->cell = c.take<int32_t>(nn);
  sos_out_carve(c, L * B, &w->lv[0]);
  sos_out_carve(c, L, &w->lv[1]);
  sos_out_carve(c, 1, &w->lv[2]);
  return sos_carve(c, n, &w->sos);
}

// ---------------------------------------------------------------------------------- apply
template <class IT, bool LDS>
__global__ __launch_bounds__(CF_NTHR) void k_cf_apply_pairs(const float* __restrict__ pred, const IT* __restrict__ patient,
                                                            const IT* __restrict__ lab, int64_t n, int L,
                                                            const int32_t* __restrict__ deg, int64_t n_pat, int B,
                                                            CellEdges ed, const float* __restrict__ table, int use_shift,
                                                            float* __restrict__ point, float* __restrict__ lower,
                                                            float* __restrict__ upper) {
  extern __shared__ float cf_lds[];
  const int n_cells = L * B;
  const float* T = table;
  if (LDS) {
    for (int e = threadIdx.x; e < 3 * n_cells; e += CF_NTHR) cf_lds[e] = table[e];
    __syncthreads();
    T = cf_lds;
  }
  const int64_t step = (int64_t)gridDim.x * CF_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * CF_NTHR + threadIdx.x; i < n; i += step) {
    const float p = pred[i];
    const int c = pair_cell(patient, lab, i, L, deg, n_pat, ed, B);
    float lo = -INFINITY, hi = INFINITY, sh = 0.f;
    if (c >= 0) {
      lo = T[c]; hi = T[n_cells + c]; sh = T[2 * n_cells + c];
    }
    lower[i] = p + lo;
    upper[i] = p + hi;
    point[i] = use_shift ? p + sh : p;
  }
}

template <int VEC> struct CfVec;
template <> struct CfVec<1> { using type = float; };
template <> struct CfVec<2> { using type = float2; };
template <> struct CfVec<4> { using type = float4; };

template <class IT, int VEC, bool LDS>
__global__ __launch_bounds__(CF_NTHR) void k_cf_apply_matrix(const float* __restrict__ pred, int64_t n_rows, int L, int64_t ld,
                                                             const IT* __restrict__ rows, const int32_t* __restrict__ deg,
                                                             int64_t n_pat, int B, CellEdges ed,
                                                             const float* __restrict__ table, int use_shift,
                                                             float* __restrict__ point, float* __restrict__ lower,
                                                             float* __restrict__ upper, int64_t ld_out, int R,
                                                             int64_t n_blocks) {
  using V = typename CfVec<VEC>::type;
  extern __shared__ float cf_lds[];
  int* rowbin = reinterpret_cast<int*>(cf_lds);            // [CF_MAX_ROWS]
  const int n_cells = L * B;
  const float* T = table;
  if (LDS) {
    float* tl = cf_lds + CF_MAX_ROWS;
    for (int e = threadIdx.x; e < 3 * n_cells; e += CF_NTHR) tl[e] = table[e];
    T = tl;
  }
  const unsigned cpr = (unsigned)((L + VEC - 1) / VEC);    // chunks per row
  for (int64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
    __syncthreads();                                       // the table is staged; the previous block's bins are consumed
    const int64_t r0 = blk * R;
    const int nr = (int)(n_rows - r0 < R ? n_rows - r0 : R);
    for (int t = threadIdx.x; t < nr; t += CF_NTHR) {      // the degree bin: once per row
      int p;
      if (rows) p = cell_index(rows, r0 + t, n_pat);
      else p = r0 + t < n_pat ? (int)(r0 + t) : -1;
      rowbin[t] = p >= 0 ? cell_bin(deg[p], ed, B) : -1;
    }
    __syncthreads();
    const unsigned items = (unsigned)nr * cpr;
    for (unsigned it = threadIdx.x; it < items; it += CF_NTHR) {
      const unsigned r = it / cpr;
      const int c0 = (int)(it - r * cpr) * VEC;
      const int b = rowbin[r];
      const float* src = pred + (r0 + r) * ld + c0;
      const int64_t dst = (r0 + r) * ld_out + c0;
      float p[VEC], lo[VEC], hi[VEC], pt[VEC];
      const bool full = c0 + VEC <= L;
      if (VEC > 1 && full) {
        const V v = *reinterpret_cast<const V*>(src);
#pragma unroll
        for (int j = 0; j < VEC; ++j) p[j] = reinterpret_cast<const float*>(&v)[j];
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) p[j] = c0 + j < L ? src[j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        float ql = -INFINITY, qh = INFINITY, sh = 0.f;
        if (b >= 0 && c0 + j < L) {
          const int c = (c0 + j) * B + b;
          ql = T[c]; qh = T[n_cells + c]; sh = T[2 * n_cells + c];
        }
        lo[j] = p[j] + ql;
        hi[j] = p[j] + qh;
        pt[j] = use_shift ? p[j] + sh : p[j];
      }
      if (VEC > 1 && full) {
        *reinterpret_cast<V*>(point + dst) = *reinterpret_cast<const V*>(pt);
        *reinterpret_cast<V*>(lower + dst) = *reinterpret_cast<const V*>(lo);
        *reinterpret_cast<V*>(upper + dst) = *reinterpret_cast<const V*>(hi);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (c0 + j < L) {
            point[dst + j] = pt[j];
            lower[dst + j] = lo[j];
            upper[dst + j] = hi[j];
          }
      }
    }
  }
}

// ---------------------------------------------------------------------------------- coverage
template <class IT>
__global__ __launch_bounds__(CF_NTHR) void k_cf_cov_keys(const IT* __restrict__ patient, const IT* __restrict__ lab,
                                                         int64_t n, int L, const int32_t* __restrict__ deg, int64_t n_pat,
                                                         int B, CellEdges ed, uint32_t* __restrict__ key,
                                                         int32_t* __restrict__ id) {
  const int64_t step = (int64_t)gridDim.x * CF_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * CF_NTHR + threadIdx.x; i < n; i += step) {
    const int c = pair_cell(patient, lab, i, L, deg, n_pat, ed, B);
    key[i] = c >= 0 ? (uint32_t)c : (uint32_t)(L * B);
    id[i] = (int32_t)i;
  }
}

// segment s of the cell-sorted pair ids: s < n_cells a cell, s = n_cells the pairs without one
__global__ __launch_bounds__(CF_NTHR) void k_cf_cov_cells(const uint32_t* __restrict__ K, const int32_t* __restrict__ id,
                                                          int64_t n, int n_cells, const float* __restrict__ pred,
                                                          const float* __restrict__ target, const float* __restrict__ table,
                                                          long long* __restrict__ counts, double* __restrict__ width) {
  __shared__ int64_t s_bounds[2];
  __shared__ int s_cnt[CF_NTHR / WAVE][MMG_CF_COV_FIELDS];
  __shared__ double s_w[CF_NTHR / WAVE];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  for (int s = blockIdx.x; s <= n_cells; s += gridDim.x) {
    __syncthreads();                                         // the previous segment's shared values are consumed
    if (threadIdx.x < 2) s_bounds[threadIdx.x] = lower_bound(K, n, (uint32_t)s + threadIdx.x);
    __syncthreads();
    const int64_t lo = s_bounds[0], hi = s_bounds[1];
    const bool cell = s < n_cells;
    const float ql = cell ? table[s] : 0.f, qh = cell ? table[n_cells + s] : 0.f;
    int cnt[MMG_CF_COV_FIELDS] = {0, 0, 0, 0, 0, 0};
    double w = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += CF_NTHR) {
      if (!cell) { cnt[5] += 1; continue; }
      const int32_t i = id[j];
      const float p = pred[i], t = target[i];
      if (p != p || t != t) { cnt[5] += 1; continue; }
      const float lower = p + ql, upper = p + qh;
      cnt[0] += 1;
      cnt[1] += (lower <= t && t <= upper) ? 1 : 0;
      cnt[2] += t < lower ? 1 : 0;
      cnt[3] += t > upper ? 1 : 0;
      if (isfinite(lower) && isfinite(upper)) {
        const float d = upper - lower;
        w += (double)d;
      } else {
        cnt[4] += 1;
      }
    }
#pragma unroll
    for (int f = 0; f < MMG_CF_COV_FIELDS; ++f) {
      const int t = wave_sum_i(cnt[f]);
      if (lane == 0) s_cnt[wid][f] = t;
    }
    w = wave_sum_d(w);
    if (lane == 0) s_w[wid] = w;
    __syncthreads();
    if (threadIdx.x < MMG_CF_COV_FIELDS) {
      long long t = 0;
      for (int q = 0; q < CF_NTHR / WAVE; ++q) t += s_cnt[q][threadIdx.x];
      counts[(size_t)s * MMG_CF_COV_FIELDS + threadIdx.x] = t;
    }
    if (threadIdx.x == 0) {
      double t = 0.0;
      for (int q = 0; q < CF_NTHR / WAVE; ++q) t += s_w[q];
      width[s] = t;
    }
  }
}

using CovWs = SegSortWs<uint32_t>;
size_t cov_carve(void* ws, int64_t n, CovWs* w) {
  MmgCarver c(ws);
  segsort_carve(c, n, w);
  return c.need();
}

bool shape_ok(int64_t n, int L, int B) {
  return n >= 0 && n <= INT32_MAX && L >= 1 && L <= MMG_CF_MAX_LABS && B >= 1 && B <= MMG_CF_MAX_BINS &&
         (int64_t)L * B <= MMG_CF_MAX_CELLS;
}
inline bool aligned_to(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" size_t mmg_seg_order_stats_ws_bytes(int64_t n, int n_seg) {
  if (n < 0 || n > INT32_MAX || n_seg < 1 || n_seg > MMG_CF_MAX_CELLS) return 0;
  MmgCarver c(nullptr);
  SosWs w;
  return sos_carve(c, n, &w);
}

extern "C" int mmg_seg_order_stats(const float* keys, const int32_t* seg, int64_t n, int n_seg, double alpha, int mode,
                                   int64_t min_count, int32_t* count, float* q_lo, float* q_hi, float* shift,
                                   int32_t* usable, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 0 && n <= INT32_MAX, "seg_order_stats: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_seg >= 1 && n_seg <= MMG_CF_MAX_CELLS, "seg_order_stats: %d segments outside [1, %d]", n_seg,
                MMG_CF_MAX_CELLS);
  CfRanks rk;
  int rc = ranks_check("seg_order_stats", alpha, mode, min_count, &rk);
  if (rc) return rc;
  MMG_CHECK_ARG(n == 0 || (keys && seg), "seg_order_stats: null keys or segment ids");
  MMG_CHECK_ARG(count && q_lo && q_hi && shift && usable, "seg_order_stats: null output");
  MmgCarver c(ws);
  SosWs w;
  MMG_CHECK_WS("seg_order_stats", sos_carve(c, n, &w));
  const SosOut o = {count, q_lo, q_hi, shift, usable};
  return sos_run("seg_order_stats", keys, seg, n, n_seg, 1, rk, o, w, (hipStream_t)stream);
}

extern "C" size_t mmg_cf_fit_ws_bytes(int64_t n, int n_labs, int n_bins) {
  if (!shape_ok(n, n_labs, n_bins)) return 0;
  FitWs w;
  return fit_carve(nullptr, n, n_labs, n_bins, &w);
}

extern "C" int mmg_cf_fit(const float* pred, const float* target, const void* patient, const void* lab, int index_bytes,
                          int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                          double alpha, int mode, int64_t min_count, float* table, int32_t* level, int32_t* n_used,
                          int64_t* dropped, void* ws, size_t ws_bytes, void* stream) {
  CellEdges ed = {};
  int rc = pairs_check("cf_fit", pred, patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  CfRanks rk;
  rc = ranks_check("cf_fit", alpha, mode, min_count, &rk);
  if (rc) return rc;
  MMG_CHECK_ARG(n == 0 || target, "cf_fit: null target");
  MMG_CHECK_ARG(table && level && n_used && dropped, "cf_fit: null output");
  FitWs w;
  MMG_CHECK_WS("cf_fit", fit_carve(ws, n, n_labs, n_bins, &w));
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = n_labs * n_bins;
  MMG_CHECK_HIP(mmg_zero_async(dropped, MMG_CF_DROP_KINDS * sizeof(int64_t), st), "cf_fit(zero)");
  if (n > 0) {
    index_dispatch(index_bytes, [&](auto it) {
      using IT = decltype(it);
      hipLaunchKernelGGL(k_cf_prepare<IT>, dim3(launch_grid(n, CF_NTHR, CF_MAX_GRID)), dim3(CF_NTHR), 0, st, pred, target,
                         (const IT*)patient, (const IT*)lab, n, n_labs, deg, n_patients, n_bins, ed, mode, w.key, w.cell,
                         (unsigned long long*)dropped);
    });
    MMG_CHECK_LAUNCH("cf_fit(prepare)");
  }
  const int divs[3] = {1, n_bins, n_cells};
  for (int lv = 0; lv < 3; ++lv) {
    rc = sos_run("cf_fit(order statistics)", w.key, w.cell, n, n_cells, divs[lv], rk, w.lv[lv], w.sos, st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_cf_resolve, dim3((n_cells + CF_NTHR - 1) / CF_NTHR), dim3(CF_NTHR), 0, st, w.lv[0], w.lv[1], w.lv[2],
                     n_cells, n_bins, table, level, n_used);
  MMG_CHECK_LAUNCH("cf_fit(resolve)");
  return MMG_OK;
}

extern "C" int mmg_cf_apply_pairs(const float* pred, const void* patient, const void* lab, int index_bytes, int64_t n,
                                  int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                                  const float* table, int use_shift, float* point, float* lower, float* upper,
                                  void* stream) {
  CellEdges ed = {};
  int rc = pairs_check("cf_apply_pairs", pred, patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins,
                       &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(table, "cf_apply_pairs: null table");
  MMG_CHECK_ARG(n == 0 || (point && lower && upper), "cf_apply_pairs: null output");
  if (n == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = n_labs * n_bins;
  const bool lds = n_cells <= CF_LDS_CELLS;
  const size_t lds_bytes = lds ? (size_t)3 * n_cells * sizeof(float) : 0;
  // a workgroup that stages the table takes at least 8 pairs per thread
  const dim3 grid(launch_grid(n, CF_NTHR, CF_MAX_GRID, lds ? 8 : 4)), block(CF_NTHR);
  index_dispatch(index_bytes, [&](auto it) {
    using IT = decltype(it);
#define CF_APPLY_PAIRS(LDS_)                                                                                              \
  hipLaunchKernelGGL((k_cf_apply_pairs<IT, LDS_>), grid, block, lds_bytes, st, pred, (const IT*)patient, (const IT*)lab, n, \
                     n_labs, deg, n_patients, n_bins, ed, table, use_shift, point, lower, upper)
    if (lds) CF_APPLY_PAIRS(true);
    else CF_APPLY_PAIRS(false);
#undef CF_APPLY_PAIRS
  });
  MMG_CHECK_LAUNCH("cf_apply_pairs");
  return MMG_OK;
}

extern "C" int mmg_cf_apply_matrix(const float* pred, int64_t n_rows, int n_labs, int64_t ld, const void* rows,
                                   int index_bytes, const int32_t* deg, int64_t n_patients, const double* bin_edges,
                                   int n_bins, const float* table, int use_shift, float* point, float* lower, float* upper,
                                   int64_t ld_out, void* stream) {
  CellEdges ed = {};
  int rc = pairs_check("cf_apply_matrix", pred, pred, pred, index_bytes, n_rows, n_labs, deg, n_patients, bin_edges, n_bins,
                       &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(ld >= n_labs && ld_out >= n_labs, "cf_apply_matrix: row strides %lld / %lld below %d labs", (long long)ld,
                (long long)ld_out, n_labs);
  MMG_CHECK_ARG(table, "cf_apply_matrix: null table");
  MMG_CHECK_ARG(n_rows == 0 || (point && lower && upper), "cf_apply_matrix: null output");
  if (n_rows == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = n_labs * n_bins;
  const bool lds = n_cells <= CF_LDS_CELLS;
  const size_t lds_bytes = (size_t)CF_MAX_ROWS * sizeof(int) + (lds ? (size_t)3 * n_cells * sizeof(float) : 0);
  int vec = 1;
  for (int v = 4; v > 1 && vec == 1; v >>= 1)
    if (ld % v == 0 && ld_out % v == 0 && aligned_to(pred, 4 * v) && aligned_to(point, 4 * v) && aligned_to(lower, 4 * v) &&
        aligned_to(upper, 4 * v))
      vec = v;
  int R = CF_BLOCK_CELLS / n_labs;
  R = R < 1 ? 1 : R > CF_MAX_ROWS ? CF_MAX_ROWS : R;
  const int64_t n_blocks = (n_rows + R - 1) / R;
  const unsigned grid = (unsigned)(n_blocks < CF_MAX_GRID ? n_blocks : CF_MAX_GRID);
#define CF_APPLY_MATRIX(IT, VEC_, LDS_)                                                                                   \
  hipLaunchKernelGGL((k_cf_apply_matrix<IT, VEC_, LDS_>), dim3(grid), dim3(CF_NTHR), lds_bytes, st, pred, n_rows, n_labs, ld, \
                     (const IT*)rows, deg, n_patients, n_bins, ed, table, use_shift, point, lower, upper, ld_out, R, n_blocks)
#define CF_APPLY_MATRIX_VEC(IT, VEC_)          \
  do {                                         \
    if (lds) CF_APPLY_MATRIX(IT, VEC_, true);  \
    else CF_APPLY_MATRIX(IT, VEC_, false);     \
  } while (0)
#define CF_APPLY_MATRIX_IT(IT)                 \
  do {                                         \
    if (vec == 4) CF_APPLY_MATRIX_VEC(IT, 4);  \
    else if (vec == 2) CF_APPLY_MATRIX_VEC(IT, 2); \
    else CF_APPLY_MATRIX_VEC(IT, 1);           \
  } while (0)
  index_dispatch(rows ? index_bytes : 8, [&](auto it) {           // no row list: the int64 instance, which never reads it
    using IT = decltype(it);
    CF_APPLY_MATRIX_IT(IT);
  });
#undef CF_APPLY_MATRIX_IT
#undef CF_APPLY_MATRIX_VEC
#undef CF_APPLY_MATRIX
  MMG_CHECK_LAUNCH("cf_apply_matrix");
  return MMG_OK;
}

extern "C" size_t mmg_cf_coverage_ws_bytes(int64_t n, int n_labs, int n_bins) {
  if (!shape_ok(n, n_labs, n_bins)) return 0;
  CovWs w;
  return cov_carve(nullptr, n, &w);
}

extern "C" int mmg_cf_coverage(const float* pred, const float* target, const void* patient, const void* lab,
                               int index_bytes, int64_t n, int n_labs, const int32_t* deg, int64_t n_patients,
                               const double* bin_edges, int n_bins, const float* table, int64_t* counts, double* width,
                               void* ws, size_t ws_bytes, void* stream) {
  CellEdges ed = {};
  int rc = pairs_check("cf_coverage", pred, patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges, n_bins, &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(n == 0 || target, "cf_coverage: null target");
  MMG_CHECK_ARG(table && counts && width, "cf_coverage: null table or output");
  CovWs w;
  MMG_CHECK_WS("cf_coverage", cov_carve(ws, n, &w));
  hipStream_t st = (hipStream_t)stream;
  const int n_cells = n_labs * n_bins;
  if (n > 0) {
    index_dispatch(index_bytes, [&](auto it) {
      using IT = decltype(it);
      hipLaunchKernelGGL(k_cf_cov_keys<IT>, dim3(launch_grid(n, CF_NTHR, CF_MAX_GRID)), dim3(CF_NTHR), 0, st,
                         (const IT*)patient, (const IT*)lab, n, n_labs, deg, n_patients, n_bins, ed, w.kv.keys, w.kv.vals);
    });
    MMG_CHECK_LAUNCH("cf_coverage(keys)");
    segsort_run(w, n, bits_of((unsigned)n_cells), st);                   // the key reaches n_cells itself
    MMG_CHECK_LAUNCH("cf_coverage(sort)");
  }
  const unsigned grid = (unsigned)(n_cells + 1 < CF_MAX_GRID ? n_cells + 1 : CF_MAX_GRID);
  hipLaunchKernelGGL(k_cf_cov_cells, dim3(grid), dim3(CF_NTHR), 0, st, w.kv.keys, w.kv.vals, n, n_cells, pred, target, table,
                     (long long*)counts, width);
  MMG_CHECK_LAUNCH("cf_coverage(cells)");
  return MMG_OK;
}
