// Lab-event preprocessing (reference src/preprocess.py:28-164, src/utils.py:309-481; mmgnn/preprocess.py):
//   mmg_prep_sort      stable LSD radix sort of row ids by (group = lab * n_patients + patient, 64-bit secondary key)
//   mmg_lab_stats      per-lab n / mean / std / min / max / rows over a lab-sorted value array (two passes, fp64)
//   mmg_lab_quantiles  per-lab q25 / median / q75 of a (lab, value)-sorted array, numpy's linear interpolation in fp64
//   mmg_lab_aggregate  one value per (patient, lab) segment of the sorted events, outliers masked on the fly
//   mmg_lab_transform  outlier masking / normalise / inverse-normalise, element-wise over a [n_labs, MMG_LS_FIELDS] table
//   mmg_lab_inverse_matrix  the inverse over a dense fp32 [n_rows, n_labs] matrix
//
// Sort.  Two chained stable sorts of (uint64 key, int32 row id) pairs by radix_sort.h: first by the secondary key (the
// time with the sign bit flipped, or the order-preserving image of the fp64 value with every NaN at the top), then by
// the group, whose bit width the host knows.  The secondary keys' OR and AND are reduced with integer atomics while the keys are
// formed: the sort's skip words, which turn the pass over a digit that every key shares into a tile copy.
//
// Sums.  A lab's slice of the sorted array is cut into LS_SPLIT contiguous chunks; one workgroup sums a chunk (a fixed
// stride per thread, a fixed LDS tree), one thread per lab adds the chunk rows in index order: no floating-point atomic
// anywhere, bitwise reproducible.  The variance is pandas' nanvar: the mean first, then the centred squares.
#include "common.h"
#include "radix_sort.h"

namespace {

constexpr int PS_NTHR = 256;
constexpr int LS_SPLIT = 32;       // chunks per lab
constexpr int LS_NTHR = 256;
constexpr int LS_PART = 6;         // n, sum, min, max, rows, centred squares
constexpr int F = MMG_LS_FIELDS;

__device__ __forceinline__ uint64_t value_key(double v) {
  if (v != v) return ~0ull;                                  // every NaN last, as pandas' and numpy's sorts put them
  const uint64_t u = (uint64_t)__double_as_longlong(v);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t time_key(int64_t t) { return (uint64_t)t ^ 0x8000000000000000ull; }

__global__ void k_ps_bits_init(unsigned long long* bits) {
  bits[0] = 0ull;          // OR of the secondary keys
  bits[1] = ~0ull;         // AND
}

__global__ __launch_bounds__(PS_NTHR) void k_ps_init(const void* __restrict__ secondary, int kind, uint64_t* keys,
                                                     int32_t* vals, int64_t n, unsigned long long* bits) {
  const int64_t e = (int64_t)blockIdx.x * PS_NTHR + threadIdx.x;
  uint64_t k = 0ull;
  if (e < n) {
    k = kind == MMG_PS_VALUE ? value_key(static_cast<const double*>(secondary)[e])
                             : time_key(static_cast<const int64_t*>(secondary)[e]);
    keys[e] = k;
    vals[e] = (int32_t)e;
  }
  uint64_t o = e < n ? k : 0ull, a = e < n ? k : ~0ull;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    o |= (uint64_t)__shfl_xor((unsigned long long)o, s, WAVE);
    a &= (uint64_t)__shfl_xor((unsigned long long)a, s, WAVE);
  }
  if ((threadIdx.x & 63) == 0) {
    // integer: exact whatever the order.  The words only gain (OR) / lose (AND) bits, so a wave that a possibly stale
    // read shows to add nothing skips the atomic: after the first waves nearly all do (every wave hitting the same two
    // addresses cost 13 ms of a 23 ms call at 37 M events)
    if (o & ~__atomic_load_n(&bits[0], __ATOMIC_RELAXED)) atomicOr(&bits[0], (unsigned long long)o);
    if (~a & __atomic_load_n(&bits[1], __ATOMIC_RELAXED)) atomicAnd(&bits[1], (unsigned long long)a);
  }
}

// row ids in input order (no secondary key: the group sort alone, stable)
__global__ __launch_bounds__(PS_NTHR) void k_ps_iota(int32_t* vals, int64_t n) {
  const int64_t e = (int64_t)blockIdx.x * PS_NTHR + threadIdx.x;
  if (e < n) vals[e] = (int32_t)e;
}

// group of the row at every sorted position.  A code outside its range is never used as an address: the row is filed
// under the sentinel group n_groups, behind every real one.
__global__ __launch_bounds__(PS_NTHR) void k_ps_group(const int64_t* __restrict__ lab, const int64_t* __restrict__ patient,
                                                      const int32_t* __restrict__ vals, uint64_t* keys, int64_t n,
                                                      int64_t n_patients, int64_t n_labs) {
  const int64_t i = (int64_t)blockIdx.x * PS_NTHR + threadIdx.x;
  if (i >= n) return;
  const int32_t e = vals[i];
  const int64_t l = lab[e], p = patient ? patient[e] : 0;
  const bool ok = l >= 0 && l < n_labs && p >= 0 && p < n_patients;
  keys[i] = ok ? (uint64_t)(l * n_patients + p) : (uint64_t)(n_labs * n_patients);
}

__global__ __launch_bounds__(PS_NTHR) void k_ps_finish(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                       const double* __restrict__ value_src, int32_t* __restrict__ perm,
                                                       int64_t* __restrict__ group_sorted,
                                                       double* __restrict__ value_sorted, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * PS_NTHR + threadIdx.x;
  if (i >= n) return;
  const int32_t e = vals[i];
  perm[i] = e;
  group_sorted[i] = (int64_t)keys[i];
  if (value_sorted) value_sorted[i] = value_src[e];
}

inline int bits_of(int64_t n_keys) {       // digits needed for keys in [0, n_keys)
  int bits = 1;
  while (bits < 63 && ((int64_t)1 << bits) < n_keys) ++bits;
  return bits;
}

// the sort's workspace, listed once: over a null base the carver only adds the sizes up
struct PsWs { unsigned long long* bits; RadixPairs<uint64_t> kv; uint32_t *thist, *scr; };      // bits: OR / AND words
size_t ps_carve(void* ws, int64_t n, PsWs* w) {
  const RadixSizes rs = radix_sizes(n);
  const size_t m = (size_t)n;
  MmgCarver c(ws);                   // (a braced list is evaluated left to right)
  *w = PsWs{c.take<unsigned long long>(2),
            {c.take<uint64_t>(m), c.take<uint64_t>(m), c.take<int32_t>(m), c.take<int32_t>(m)},
            c.take<uint32_t>(rs.hist_elems), c.take<uint32_t>(rs.scratch_elems)};
  return c.need();
}

// ------------------------------------------------------------------------------------------ per-lab slices
// ptr[l] = first position whose group is >= l * div (l = 0 .. n_labs): the slice of lab l in a lab-sorted array
__global__ __launch_bounds__(256) void k_lab_ptr(const int64_t* __restrict__ group, int64_t n, int64_t div, int n_labs,
                                                 int64_t* __restrict__ ptr) {
  const int l = blockIdx.x * 256 + threadIdx.x;
  if (l > n_labs) return;
  const int64_t want = (int64_t)l * div;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (group[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  ptr[l] = lo;
}

// ------------------------------------------------------------------------------------------ statistics
template <int PASS>
__global__ __launch_bounds__(LS_NTHR) void k_ls_part(const double* __restrict__ value, const int64_t* __restrict__ ptr,
                                                     const double* __restrict__ stats, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double s_acc[LS_NTHR];
  const int lab = blockIdx.x, y = blockIdx.y, t = threadIdx.x;
  const int64_t s = ptr[lab], e = ptr[lab + 1];
  const int64_t chunk = (e - s + LS_SPLIT - 1) / LS_SPLIT;
  const int64_t cs = s + (int64_t)y * chunk;
  const int64_t ce = cs + chunk < e ? cs + chunk : e;
  const double mean = PASS == 1 ? stats[(size_t)lab * F + MMG_LS_MEAN] : 0.0;
  double cnt = 0.0, sum = 0.0, rows = 0.0;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  for (int64_t i = cs + t; i < ce; i += LS_NTHR) {
    const double v = value[i];
    rows += 1.0;
    if (v != v) continue;                                    // NaN-skipping, as pandas
    if (PASS == 0) {
      cnt += 1.0;
      sum += v;
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    } else {
      const double d = mean - v;
      sum += d * d;
    }
  }
  double* row = part + ((size_t)lab * LS_SPLIT + y) * LS_PART;
  const int first = PASS == 0 ? 0 : 5, last = PASS == 0 ? 5 : 6;
  for (int f = first; f < last; ++f) {
    s_acc[t] = f == 0 ? cnt : f == 1 ? sum : f == 2 ? mn : f == 3 ? mx : f == 4 ? rows : sum;
    __syncthreads();
    for (int h = LS_NTHR / 2; h > 0; h >>= 1) {              // fixed tree: reproducible
      if (t < h) {
        const double o = s_acc[t + h];
        s_acc[t] = f == 2 ? fmin(s_acc[t], o) : f == 3 ? fmax(s_acc[t], o) : s_acc[t] + o;
      }
      __syncthreads();
    }
    if (t == 0) row[f] = s_acc[0];
    __syncthreads();
  }
}

template <int PASS>
__global__ __launch_bounds__(64) void k_ls_comb(const double* __restrict__ part, int n_labs, double* __restrict__ stats) {
#pragma clang fp contract(off)
  const int lab = blockIdx.x * 64 + threadIdx.x;
  if (lab >= n_labs) return;
  const double* p = part + (size_t)lab * LS_SPLIT * LS_PART;
  double* st = stats + (size_t)lab * F;
  const double nan = __builtin_nan("");
  if (PASS == 0) {
    double cnt = 0.0, sum = 0.0, rows = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
    for (int y = 0; y < LS_SPLIT; ++y) {
      cnt += p[y * LS_PART + 0];
      sum += p[y * LS_PART + 1];
      mn = fmin(mn, p[y * LS_PART + 2]);
      mx = fmax(mx, p[y * LS_PART + 3]);
      rows += p[y * LS_PART + 4];
    }
    st[MMG_LS_N] = cnt;
    st[MMG_LS_MEAN] = cnt > 0.0 ? sum / cnt : nan;
    st[MMG_LS_MIN] = cnt > 0.0 ? mn : nan;
    st[MMG_LS_MAX] = cnt > 0.0 ? mx : nan;
    st[MMG_LS_ROWS] = rows;
    st[MMG_LS_Q25] = nan;
    st[MMG_LS_MEDIAN] = nan;
    st[MMG_LS_Q75] = nan;
  } else {
    double ss = 0.0;
    for (int y = 0; y < LS_SPLIT; ++y) ss += p[y * LS_PART + 5];
    const double cnt = st[MMG_LS_N];
    st[MMG_LS_STD] = cnt > 1.0 ? sqrt(ss / (cnt - 1.0)) : nan;          // ddof = 1: one value has no spread
  }
}

size_t ls_ws_need(int n_labs) {
  return mmg_align256((size_t)(n_labs + 1) * sizeof(int64_t)) +
         mmg_align256((size_t)n_labs * LS_SPLIT * LS_PART * sizeof(double));
}

// numpy's "linear" quantile of m ascending values (lib/function_base _lerp, both branches), fp64, every operation
// rounded on its own
__device__ __forceinline__ double lq_quantile(const double* __restrict__ x, int64_t m, double q) {
#pragma clang fp contract(off)
  const double vi = (double)(m - 1) * q;
  if (vi >= (double)(m - 1)) return x[m - 1];
  const double fl = floor(vi);
  const int64_t i = (int64_t)fl;
  const double g = vi - fl;
  const double a = x[i], b = x[i + 1 < m ? i + 1 : m - 1];
  const double d = b - a;
  return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

__global__ __launch_bounds__(64) void k_lq(const double* __restrict__ value, const int64_t* __restrict__ ptr, int n_labs,
                                           double* __restrict__ stats) {
#pragma clang fp contract(off)
  const int lab = blockIdx.x * 64 + threadIdx.x;
  if (lab >= n_labs) return;
  const int64_t s = ptr[lab], e = ptr[lab + 1];
  int64_t lo = s, hi = e;                                     // the NaN sit at the end of the slice
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    const double v = value[mid];
    if (v == v) lo = mid + 1;
    else hi = mid;
  }
  const int64_t m = lo - s;
  double* st = stats + (size_t)lab * F;
  const double nan = __builtin_nan("");
  if (m == 0) {
    st[MMG_LS_Q25] = nan;
    st[MMG_LS_MEDIAN] = nan;
    st[MMG_LS_Q75] = nan;
    return;
  }
  const double* x = value + s;
  st[MMG_LS_Q25] = lq_quantile(x, m, 0.25);
  st[MMG_LS_Q75] = lq_quantile(x, m, 0.75);
  st[MMG_LS_MEDIAN] = (m & 1) ? x[m / 2] : (x[m / 2 - 1] + x[m / 2]) / 2.0;   // pandas' median: the mean of the two
}

// ------------------------------------------------------------------------------------------ element-wise
struct Bounds { double lo, hi; };
__device__ __forceinline__ Bounds outlier_bounds(const double* __restrict__ st, int method, double thr) {
#pragma clang fp contract(off)
  Bounds b;
  if (method == MMG_OUT_STD) {
    const double w = thr * st[MMG_LS_STD];
    b.lo = st[MMG_LS_MEAN] - w;
    b.hi = st[MMG_LS_MEAN] + w;
  } else {
    const double iqr = st[MMG_LS_Q75] - st[MMG_LS_Q25];
    const double w = thr * iqr;
    b.lo = st[MMG_LS_Q25] - w;
    b.hi = st[MMG_LS_Q75] + w;
  }
  return b;                        // a NaN bound removes nothing: comparisons with NaN are false
}

__device__ __forceinline__ double lt_normalize(const double* __restrict__ st, int method, double v) {
#pragma clang fp contract(off)
  if (!(st[MMG_LS_N] > 0.0)) return v;                       // stats[lab] = None: the values pass through
  if (method == MMG_NORM_ZSCORE) {
    const double sd = st[MMG_LS_STD];
    return (sd == 0.0 || sd != sd) ? v - st[MMG_LS_MEAN] : (v - st[MMG_LS_MEAN]) / sd;
  }
  if (method == MMG_NORM_MINMAX) {
    const double r = st[MMG_LS_MAX] - st[MMG_LS_MIN];
    return (r == 0.0 || r != r) ? v * 0.0 : (v - st[MMG_LS_MIN]) / r;
  }
  const double iqr = st[MMG_LS_Q75] - st[MMG_LS_Q25];
  return (iqr == 0.0 || iqr != iqr) ? v - st[MMG_LS_MEDIAN] : (v - st[MMG_LS_MEDIAN]) / iqr;
}

// the reference's inverse does not special-case a zero spread
__device__ __forceinline__ double lt_inverse(const double* __restrict__ st, int method, double v) {
#pragma clang fp contract(off)
  if (!(st[MMG_LS_N] > 0.0)) return v;
  if (method == MMG_NORM_ZSCORE) return v * st[MMG_LS_STD] + st[MMG_LS_MEAN];
  if (method == MMG_NORM_MINMAX) return v * (st[MMG_LS_MAX] - st[MMG_LS_MIN]) + st[MMG_LS_MIN];
  return v * (st[MMG_LS_Q75] - st[MMG_LS_Q25]) + st[MMG_LS_MEDIAN];
}

__global__ __launch_bounds__(256) void k_lt(int mode, int method, double thr, const int64_t* __restrict__ lab,
                                            const double* __restrict__ value, int64_t n, int n_labs,
                                            const double* __restrict__ stats, double* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
    const double v = value[i];
    const int64_t l = lab ? lab[i] : 0;
    if (l < 0 || l >= n_labs) {                               // not a selected lab: untouched, never an address
      out[i] = v;
      continue;
    }
    const double* st = stats + (size_t)l * F;
    if (mode == MMG_LT_OUTLIER) {
      const Bounds b = outlier_bounds(st, method, thr);
      out[i] = (v < b.lo || v > b.hi) ? __builtin_nan("") : v;
    } else if (mode == MMG_LT_NORMALIZE) {
      out[i] = lt_normalize(st, method, v);
    } else {
      out[i] = lt_inverse(st, method, v);
    }
  }
}

__global__ __launch_bounds__(256) void k_lt_matrix(int method, const float* __restrict__ pred, int64_t n_rows, int n_labs,
                                                   int64_t ld, const double* __restrict__ stats, float* __restrict__ out,
                                                   int64_t ld_out) {
  const int64_t total = n_rows * n_labs, stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int64_t r = i / n_labs;
    const int c = (int)(i - r * n_labs);
    out[r * ld_out + c] = (float)lt_inverse(stats + (size_t)c * F, method, (double)pred[r * ld + c]);
  }
}

int ew_grid(int64_t n) {
  int64_t g = (n + 256 * 4 - 1) / (256 * 4);
  return (int)(g < 1 ? 1 : g > 8192 ? 8192 : g);
}

// ------------------------------------------------------------------------------------------ aggregation
// One thread per segment head walks its segment (a handful of events) in sorted order.
__global__ __launch_bounds__(256) void k_ag_heads(const int64_t* __restrict__ group, const double* __restrict__ value,
                                                  int64_t n, int64_t n_groups, int64_t n_patients, int method,
                                                  int remove, int out_method, double thr,
                                                  const double* __restrict__ stats, uint32_t* __restrict__ keep,
                                                  uint32_t* __restrict__ pos, double* __restrict__ segval) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t g = group[i];
  if (g >= n_groups || (i > 0 && group[i - 1] == g)) {
    keep[i] = 0u;
    pos[i] = 0u;
    return;
  }
  Bounds b;
  b.lo = b.hi = __builtin_nan("");
  if (remove) b = outlier_bounds(stats + (size_t)(g / n_patients) * F, out_method, thr);
  const double nan = __builtin_nan("");
  int64_t rows = 0, cnt = 0, first = -1;
  double lastv = nan, sum = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  for (int64_t j = i; j < n && group[j] == g; ++j) {
    const double v = value[j];
    const bool valid = v == v && !(remove && (v < b.lo || v > b.hi));
    if (remove ? valid : true) {                              // rows with a NaN value leave only with outlier removal
      ++rows;
      lastv = v;
    }
    if (valid) {
      if (first < 0) first = j;
      ++cnt;
      sum += v;
      mn = fmin(mn, v);
      mx = fmax(mx, v);
    }
  }
  double r = nan;
  if (method == MMG_AGG_LAST) r = lastv;
  else if (cnt > 0) {
    if (method == MMG_AGG_MEAN) r = sum / (double)cnt;
    else if (method == MMG_AGG_MIN) r = mn;
    else if (method == MMG_AGG_MAX) r = mx;
    else {                                                    // median: the valid values are one ascending run
      const int64_t h = first + cnt / 2;
      r = (cnt & 1) ? value[h] : (value[h - 1] + value[h]) / 2.0;
    }
  }
  const uint32_t k = rows > 0 ? 1u : 0u;
  keep[i] = k;
  pos[i] = k;
  segval[i] = r;
}

__global__ __launch_bounds__(256) void k_ag_compact(const int64_t* __restrict__ group, const uint32_t* __restrict__ keep,
                                                    const uint32_t* __restrict__ pos, const double* __restrict__ segval,
                                                    int64_t n, int64_t n_patients, int64_t* __restrict__ out_patient,
                                                    int64_t* __restrict__ out_lab, double* __restrict__ out_value,
                                                    int64_t* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  if (keep[i]) {
    const uint32_t p = pos[i];                                // < the number of kept heads <= n
    const int64_t g = group[i];
    out_lab[p] = g / n_patients;
    out_patient[p] = g % n_patients;
    out_value[p] = segval[i];
  }
  if (i == n - 1) count[0] = (int64_t)pos[i] + (int64_t)keep[i];
}

size_t ag_ws_need(int64_t n) {
  const int64_t m = n > 0 ? n : 1;
  return 256 + 2 * mmg_align256((size_t)m * 4) + mmg_align256((size_t)m * 8) + mmg_align256(scan_scratch_elems(m) * 4) +
         256;
}

bool sizes_ok(int64_t n, int64_t n_patients, int n_labs) {
  return n >= 0 && n < INT32_MAX && n_patients >= 1 && n_patients < INT32_MAX && n_labs >= 1 && n_labs <= MMG_PREP_MAX_LABS;
}

}  // namespace

extern "C" size_t mmg_prep_sort_ws_bytes(int64_t n) {
  PsWs w;
  return ps_carve(nullptr, n < 0 ? 0 : n, &w);
}

extern "C" int mmg_prep_sort(const int64_t* lab, const int64_t* patient, const void* secondary, int kind, int64_t n,
                             int64_t n_patients, int n_labs, const double* value_src, int32_t* perm,
                             int64_t* group_sorted, double* value_sorted, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(sizes_ok(n, n_patients, n_labs),
                "prep_sort: n %lld, n_patients %lld, n_labs %d outside [0, 2^31) / [1, 2^31) / [1, %d]", (long long)n,
                (long long)n_patients, n_labs, MMG_PREP_MAX_LABS);
  MMG_CHECK_ARG(kind == MMG_PS_TIME || kind == MMG_PS_VALUE, "prep_sort: secondary kind %d", kind);
  MMG_CHECK_ARG(n == 0 || (lab && perm && group_sorted), "prep_sort: null buffer");
  MMG_CHECK_ARG((value_sorted == nullptr) == (value_src == nullptr) || n == 0,
                "prep_sort: value_src and value_sorted go together");
  PsWs w;
  MMG_CHECK_WS("prep_sort", ps_carve(ws, n, &w));
  if (n == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const unsigned eb = (unsigned)((n + PS_NTHR - 1) / PS_NTHR);
  if (secondary) {
    MMG_CHECK_HIP(mmg_zero_async(w.thist, radix_sizes(n).hist_elems * 4, st), "prep_sort(zero)");   // a skipped first pass
    hipLaunchKernelGGL(k_ps_bits_init, dim3(1), dim3(1), 0, st, w.bits);
    hipLaunchKernelGGL(k_ps_init, dim3(eb), dim3(PS_NTHR), 0, st, secondary, kind, w.kv.keys, w.kv.vals, n, w.bits);
    MMG_CHECK_LAUNCH("prep_sort(init)");
    for (int ps = 0; ps < 8; ++ps) radix_pass<true>(w.kv, n, 8 * ps, w.bits, w.thist, w.scr, st);
    MMG_CHECK_LAUNCH("prep_sort(secondary)");
  } else {
    hipLaunchKernelGGL(k_ps_iota, dim3(eb), dim3(PS_NTHR), 0, st, w.kv.vals, n);
  }
  hipLaunchKernelGGL(k_ps_group, dim3(eb), dim3(PS_NTHR), 0, st, lab, patient, w.kv.vals, w.kv.keys, n,
                     patient ? n_patients : (int64_t)1, (int64_t)n_labs);
  const int gp = (bits_of((patient ? n_patients : (int64_t)1) * n_labs + 1) + 7) / 8;   // + the sentinel group
  for (int ps = 0; ps < gp; ++ps) radix_pass<true>(w.kv, n, 8 * ps, nullptr, w.thist, w.scr, st);
  hipLaunchKernelGGL(k_ps_finish, dim3(eb), dim3(PS_NTHR), 0, st, w.kv.keys, w.kv.vals, value_src, perm, group_sorted,
                     value_sorted, n);
  MMG_CHECK_LAUNCH("prep_sort");
  return MMG_OK;
}

extern "C" size_t mmg_lab_stats_ws_bytes(int n_labs) { return ls_ws_need(n_labs < 1 ? 1 : n_labs) + 256; }

extern "C" int mmg_lab_stats(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients,
                             int n_labs, double* stats, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(sizes_ok(n, n_patients, n_labs), "lab_stats: n %lld, n_patients %lld, n_labs %d out of range",
                (long long)n, (long long)n_patients, n_labs);
  MMG_CHECK_ARG(stats && (n == 0 || (group_sorted && value_sorted)), "lab_stats: null buffer");
  MMG_CHECK_WS("lab_stats", ls_ws_need(n_labs) + 256);
  hipStream_t st = (hipStream_t)stream;
  MmgCarver c(ws);
  int64_t* ptr = c.take<int64_t>((size_t)n_labs + 1);
  double* part = c.take<double>((size_t)n_labs * LS_SPLIT * LS_PART);
  hipLaunchKernelGGL(k_lab_ptr, dim3((n_labs + 256) / 256), dim3(256), 0, st, group_sorted, n, n_patients, n_labs, ptr);
  const dim3 grid(n_labs, LS_SPLIT), cg((n_labs + 63) / 64);
  hipLaunchKernelGGL(k_ls_part<0>, grid, dim3(LS_NTHR), 0, st, value_sorted, ptr, stats, part);
  hipLaunchKernelGGL(k_ls_comb<0>, cg, dim3(64), 0, st, part, n_labs, stats);
  hipLaunchKernelGGL(k_ls_part<1>, grid, dim3(LS_NTHR), 0, st, value_sorted, ptr, stats, part);
  hipLaunchKernelGGL(k_ls_comb<1>, cg, dim3(64), 0, st, part, n_labs, stats);
  MMG_CHECK_LAUNCH("lab_stats");
  return MMG_OK;
}

extern "C" size_t mmg_lab_quantiles_ws_bytes(int n_labs) {
  return mmg_align256((size_t)((n_labs < 1 ? 1 : n_labs) + 1) * sizeof(int64_t)) + 256;
}

extern "C" int mmg_lab_quantiles(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients,
                                 int n_labs, double* stats, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(sizes_ok(n, n_patients, n_labs), "lab_quantiles: n %lld, n_patients %lld, n_labs %d out of range",
                (long long)n, (long long)n_patients, n_labs);
  MMG_CHECK_ARG(stats && (n == 0 || (group_sorted && value_sorted)), "lab_quantiles: null buffer");
  MMG_CHECK_WS("lab_quantiles", mmg_lab_quantiles_ws_bytes(n_labs));
  hipStream_t st = (hipStream_t)stream;
  int64_t* ptr = MmgCarver(ws).take<int64_t>((size_t)n_labs + 1);
  hipLaunchKernelGGL(k_lab_ptr, dim3((n_labs + 256) / 256), dim3(256), 0, st, group_sorted, n, n_patients, n_labs, ptr);
  hipLaunchKernelGGL(k_lq, dim3((n_labs + 63) / 64), dim3(64), 0, st, value_sorted, ptr, n_labs, stats);
  MMG_CHECK_LAUNCH("lab_quantiles");
  return MMG_OK;
}

extern "C" size_t mmg_lab_aggregate_ws_bytes(int64_t n) { return ag_ws_need(n); }

extern "C" int mmg_lab_aggregate(const int64_t* group_sorted, const double* value_sorted, int64_t n, int64_t n_patients,
                                 int n_labs, int method, int outlier_method, double threshold, const double* stats,
                                 int64_t* out_patient, int64_t* out_lab, double* out_value, int64_t* n_pairs, void* ws,
                                 size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(sizes_ok(n, n_patients, n_labs), "lab_aggregate: n %lld, n_patients %lld, n_labs %d out of range",
                (long long)n, (long long)n_patients, n_labs);
  MMG_CHECK_ARG(method >= MMG_AGG_LAST && method <= MMG_AGG_MAX, "lab_aggregate: method %d", method);
  MMG_CHECK_ARG(outlier_method == MMG_OUT_NONE || outlier_method == MMG_OUT_STD || outlier_method == MMG_OUT_IQR,
                "lab_aggregate: outlier method %d", outlier_method);
  MMG_CHECK_ARG(outlier_method == MMG_OUT_NONE || stats, "lab_aggregate: outlier removal needs the stats table");
  MMG_CHECK_ARG(n_pairs, "lab_aggregate: n_pairs is null");
  MMG_CHECK_ARG(n == 0 || (group_sorted && value_sorted && out_patient && out_lab && out_value),
                "lab_aggregate: null buffer");
  MMG_CHECK_WS("lab_aggregate", ag_ws_need(n));
  *n_pairs = 0;
  if (n == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  MmgCarver c(ws);
  int64_t* count = c.take<int64_t>(1);
  uint32_t* keep = c.take<uint32_t>((size_t)n);
  uint32_t* pos = c.take<uint32_t>((size_t)n);
  double* segval = c.take<double>((size_t)n);
  uint32_t* scr = c.take<uint32_t>(scan_scratch_elems(n));
  const unsigned eb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(k_ag_heads, dim3(eb), dim3(256), 0, st, group_sorted, value_sorted, n,
                     (int64_t)n_labs * n_patients, n_patients, method, outlier_method != MMG_OUT_NONE ? 1 : 0,
                     outlier_method, threshold, stats, keep, pos, segval);
  exclusive_scan_u32(pos, n, scr, st);
  hipLaunchKernelGGL(k_ag_compact, dim3(eb), dim3(256), 0, st, group_sorted, keep, pos, segval, n, n_patients,
                     out_patient, out_lab, out_value, count);
  MMG_CHECK_LAUNCH("lab_aggregate");
  MMG_CHECK_HIP(hipMemcpyAsync(n_pairs, count, sizeof(int64_t), hipMemcpyDeviceToHost, st), "lab_aggregate(count)");
  MMG_CHECK_HIP(hipStreamSynchronize(st), "lab_aggregate(sync)");      // the count sizes the caller's outputs
  return MMG_OK;
}

extern "C" int mmg_lab_transform(int mode, int method, double threshold, const int64_t* lab, const double* value,
                                 int64_t n, int n_labs, const double* stats, double* out, void* stream) {
  MMG_CHECK_ARG(n >= 0 && n < INT32_MAX && n_labs >= 1 && n_labs <= MMG_PREP_MAX_LABS,
                "lab_transform: n %lld, n_labs %d out of range", (long long)n, n_labs);
  MMG_CHECK_ARG(mode == MMG_LT_OUTLIER || mode == MMG_LT_NORMALIZE || mode == MMG_LT_INVERSE, "lab_transform: mode %d",
                mode);
  if (mode == MMG_LT_OUTLIER)
    MMG_CHECK_ARG(method == MMG_OUT_STD || method == MMG_OUT_IQR, "lab_transform: outlier method %d", method);
  else
    MMG_CHECK_ARG(method >= MMG_NORM_ZSCORE && method <= MMG_NORM_ROBUST, "lab_transform: normalisation %d", method);
  MMG_CHECK_ARG(stats && (n == 0 || (value && out)), "lab_transform: null buffer");
  if (n == 0) return MMG_OK;
  hipLaunchKernelGGL(k_lt, dim3(ew_grid(n)), dim3(256), 0, (hipStream_t)stream, mode, method, threshold, lab, value, n,
                     n_labs, stats, out);
  MMG_CHECK_LAUNCH("lab_transform");
  return MMG_OK;
}

extern "C" int mmg_lab_inverse_matrix(int method, const float* pred, int64_t n_rows, int n_labs, int64_t ld,
                                      const double* stats, float* out, int64_t ld_out, void* stream) {
  MMG_CHECK_ARG(n_rows >= 0 && n_rows < INT32_MAX && n_labs >= 1 && n_labs <= MMG_PREP_MAX_LABS,
                "lab_inverse_matrix: n_rows %lld, n_labs %d out of range", (long long)n_rows, n_labs);
  MMG_CHECK_ARG(ld >= n_labs && ld_out >= n_labs, "lab_inverse_matrix: leading dimensions %lld / %lld < n_labs %d",
                (long long)ld, (long long)ld_out, n_labs);
  MMG_CHECK_ARG(method >= MMG_NORM_ZSCORE && method <= MMG_NORM_ROBUST, "lab_inverse_matrix: normalisation %d", method);
  MMG_CHECK_ARG(stats && (n_rows == 0 || (pred && out)), "lab_inverse_matrix: null buffer");
  if (n_rows == 0) return MMG_OK;
  hipLaunchKernelGGL(k_lt_matrix, dim3(ew_grid(n_rows * n_labs)), dim3(256), 0, (hipStream_t)stream, method, pred, n_rows,
                     n_labs, ld, stats, out, ld_out);
  MMG_CHECK_LAUNCH("lab_inverse_matrix");
  return MMG_OK;
}
