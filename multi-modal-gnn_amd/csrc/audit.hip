// Leakage-audit reducers (reference src/audit_leakage.py; mmgnn/audit.py):
//   mmg_order_stats      exact order statistics of an fp32 array (or of |a - b|) by a three-pass radix select
//   mmg_robust_sums      one pass over (pred, target) for every field of compute_robust_metrics, winsorising bounds
//                        interpolated on the device from the order statistics (numpy's "linear" percentile)
//   mmg_split_membership patients per train / val / test membership class and edges in several splits
//
// Order statistics.  Every value maps to a monotone uint32 key (sign flip; every NaN to 0xFFFFFFFF, so NaN sorts last as
// numpy's sort does).  Three passes select the key of each requested rank 11, 11 and 10 bits at a time:
//   k_os_hist<P>  every workgroup builds integer LDS histograms of the digit of pass P over the keys whose higher digits
//                 match the prefix of a rank ("slot": ranks that share a prefix share one), then adds its nonzero bins to
//                 the global histogram with integer atomics -- exact and independent of the order of the adds;
//   k_os_pick<P>  one wave per rank scans its slot's histogram for the bucket that holds its rank, extends the prefix and
//                 rebases the rank; the last pass turns the key back into the value.
// The passes hand over through global memory at kernel boundaries (no grid barrier: the XCD L2s are not coherent) and
// never through the host, so the whole call can be captured into a hipGraph.
//
// Robust sums.  Per-workgroup rows of fp64 sums (a fixed grid-stride order per thread, a fixed LDS tree per workgroup),
// then one workgroup adds the rows in index order: the result is bitwise the same from run to run.
#include "common.h"

namespace {

constexpr int OS_THREADS = 512;              // 64 KiB of LDS histograms: two workgroups per CU
constexpr int OS_BINS = 2048;               // 11-bit digits (the last pass uses 1024 of them)
constexpr int OS_MAX_GRID = 1024;
constexpr int RS_THREADS = 256;
constexpr int RS_MAX_GRID = 1024;
constexpr int SM_THREADS = 256;
constexpr int SM_MAX_GRID = 2048;

struct OsRanks {
  int64_t r[MMG_OS_MAX_RANKS];
};

// select state, in the workspace between the launches
struct OsState {
  uint32_t prefix[MMG_OS_MAX_RANKS];        // key bits fixed so far, per rank
  int64_t rank[MMG_OS_MAX_RANKS];           // rank among the keys that carry the prefix
  int32_t slot_of[MMG_OS_MAX_RANKS];
  uint32_t slot_prefix[MMG_OS_MAX_RANKS];
  int32_t n_slots;
  int32_t pad;
};

__device__ __forceinline__ uint32_t os_key(float v) {
  const uint32_t u = __float_as_uint(v);
  if (v != v) return 0xFFFFFFFFu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float os_value(uint32_t k) {
  if (k == 0xFFFFFFFFu) return __builtin_nanf("");
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k);
}

// numpy forms abs(y_pred - y_true) in fp32
__device__ __forceinline__ float os_load(const float* __restrict__ a, const float* __restrict__ b, int64_t i) {
  return b ? fabsf(__fsub_rn(a[i], b[i])) : a[i];
}

constexpr int os_shift(int pass) { return pass == 0 ? 21 : pass == 1 ? 10 : 0; }
constexpr uint32_t os_mask(int pass) { return pass == 2 ? 0x3FFu : 0x7FFu; }

__global__ __launch_bounds__(OS_THREADS) void k_os_init(OsState* st, int n_ranks, OsRanks ranks) {
  const int t = threadIdx.x;
  if (t < MMG_OS_MAX_RANKS) {
    st->prefix[t] = 0u;
    st->rank[t] = t < n_ranks ? ranks.r[t] : 0;
    st->slot_of[t] = 0;
    st->slot_prefix[t] = 0u;
  }
  if (t == 0) st->n_slots = 1;
}

template <int PASS>
__global__ __launch_bounds__(OS_THREADS) void k_os_hist(const float* __restrict__ a, const float* __restrict__ b,
                                                         int64_t n, const OsState* __restrict__ st,
                                                         uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_hist[MMG_OS_MAX_RANKS * OS_BINS];
  __shared__ uint32_t s_pre[MMG_OS_MAX_RANKS];
  const int ns = st->n_slots;
  for (int i = threadIdx.x; i < ns * OS_BINS; i += OS_THREADS) s_hist[i] = 0u;
  if (threadIdx.x < MMG_OS_MAX_RANKS) s_pre[threadIdx.x] = st->slot_prefix[threadIdx.x];
  __syncthreads();
  constexpr int sh = os_shift(PASS);
  constexpr uint32_t dm = os_mask(PASS);
  const int64_t stride = (int64_t)gridDim.x * OS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * OS_THREADS + threadIdx.x; i < n; i += stride) {
    const uint32_t k = os_key(os_load(a, b, i));
    const uint32_t d = (k >> sh) & dm;
    if (PASS == 0) {
      atomicAdd(&s_hist[d], 1u);
    } else {
      const uint32_t hi = k >> (sh + (PASS == 1 ? 11 : 10));
      for (int s = 0; s < ns; ++s) {
        if (hi == s_pre[s]) {                // the slot prefixes are distinct: at most one match
          atomicAdd(&s_hist[s * OS_BINS + d], 1u);
          break;
        }
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ns * OS_BINS; i += OS_THREADS) {
    const uint32_t c = s_hist[i];
    if (c) atomicAdd(&hist[i], c);
  }
}

// one wave per rank: lane l owns the 32 buckets [32 l, 32 l + 32)
template <int PASS>
__global__ __launch_bounds__(MMG_OS_MAX_RANKS * WAVE) void k_os_pick(OsState* st, const uint32_t* __restrict__ hist,
                                                                      int n_ranks, float* __restrict__ out,
                                                                      int64_t* __restrict__ nan_count) {
  __shared__ uint32_t s_prefix[MMG_OS_MAX_RANKS];
  const int w = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
  constexpr int bits = PASS == 2 ? 10 : 11;
  constexpr int nb = 1 << bits, per = nb / WAVE;
  if (PASS == 0 && threadIdx.x == 0 && nan_count) nan_count[0] = (int64_t)hist[0x7FF];   // only NaN keys reach 0x7FF
  if (w < n_ranks) {
    const uint32_t* h = hist + (size_t)st->slot_of[w] * OS_BINS;
    const int64_t k = st->rank[w];
    uint32_t c[32];
    int64_t own = 0;
#pragma unroll
    for (int i = 0; i < per; ++i) {
      c[i] = h[lane * per + i];
      own += c[i];
    }
    int64_t incl = own;                      // inclusive scan over the lanes
#pragma unroll
    for (int o = 1; o < WAVE; o <<= 1) {
      const int64_t v = __shfl_up(incl, o, WAVE);
      if (lane >= o) incl += v;
    }
    const int64_t excl = incl - own;
    const unsigned long long hit = __ballot(k < incl);
    const int first = hit ? __ffsll((long long)hit) - 1 : WAVE - 1;   // (always hit while the rank is < n)
    if (lane == first) {
      int64_t base = excl;
      int bkt = lane * per + per - 1;
#pragma unroll
      for (int i = 0; i < per; ++i) {
        if (k < base + (int64_t)c[i]) {
          bkt = lane * per + i;
          break;
        }
        base += c[i];
      }
      const uint32_t pre = (st->prefix[w] << bits) | (uint32_t)bkt;
      st->prefix[w] = pre;
      st->rank[w] = k - base;
      s_prefix[w] = pre;
      if (PASS == 2) out[w] = os_value(pre);
    }
  }
  __syncthreads();
  if (PASS < 2 && threadIdx.x == 0) {        // distinct prefixes -> slots of the next pass
    int ns = 0;
    for (int r = 0; r < n_ranks; ++r) {
      int s = 0;
      while (s < ns && st->slot_prefix[s] != s_prefix[r]) ++s;
      if (s == ns) st->slot_prefix[ns++] = s_prefix[r];
      st->slot_of[r] = s;
    }
    st->n_slots = ns;
  }
}

size_t os_hist_bytes() { return (size_t)3 * MMG_OS_MAX_RANKS * OS_BINS * sizeof(uint32_t); }
size_t os_ws_need() { return os_hist_bytes() + mmg_align256(sizeof(OsState)); }

int os_grid(int64_t n) {
  int64_t g = (n + OS_THREADS * 16 - 1) / (OS_THREADS * 16);
  return (int)(g < 1 ? 1 : g > OS_MAX_GRID ? OS_MAX_GRID : g);
}

// ------------------------------------------------------------------------------------------ robust sums
// numpy's "linear" percentile from two order statistics, every operation rounded on its own: plain operators under
// contract(off) (the __f*_rn helpers are header functions compiled with contraction on, and fuse once inlined)
__device__ __forceinline__ float rs_percentile(const float* __restrict__ xs, const mmg_percentile_t& p, bool any_nan) {
#pragma clang fp contract(off)
  if (any_nan) return __builtin_nanf("");
  const float xi = xs[p.lo], xj = xs[p.hi];
  const float d = xj - xi;
  return p.g >= 0.5f ? xj - d * (1.0f - p.g) : xi + d * p.g;
}

// np.clip: NaN in any operand gives NaN
__device__ __forceinline__ float rs_clip(float x, float lo, float hi) {
  if (x != x || lo != lo || hi != hi) return __builtin_nanf("");
  return fminf(fmaxf(x, lo), hi);
}

constexpr int RS_SUMS = 9;                  // fp64 fields summed per workgroup row
constexpr int RS_ROW = 12;                  // + outside count, NaN count (as doubles: exact below 2^53), max |r|

__global__ __launch_bounds__(RS_THREADS) void k_rs_partial(const float* __restrict__ pred, const float* __restrict__ target,
                                                           int64_t n, const float* __restrict__ xs,
                                                           const int64_t* __restrict__ nan_count, mmg_percentile_t plo,
                                                           mmg_percentile_t phi, double* __restrict__ rows) {
  __shared__ double s_acc[RS_THREADS];
  const bool any_nan = nan_count[0] > 0;
  const float lo = rs_percentile(xs, plo, any_nan), hi = rs_percentile(xs, phi, any_nan);
  const float nhi = -hi;
  double acc[RS_SUMS] = {};
  int64_t outside = 0, nans = 0;
  float mx = 0.f;
  const int64_t stride = (int64_t)gridDim.x * RS_THREADS;
  for (int64_t i = (int64_t)blockIdx.x * RS_THREADS + threadIdx.x; i < n; i += stride) {
    const float p = pred[i], t = target[i];
    const float r = __fsub_rn(p, t);
    const float ar = fabsf(r);
    const float den = __fadd_rn(__fadd_rn(fabsf(t), fabsf(p)), 1e-8f);
    const float sm = __fdiv_rn(ar, den);
    const float cw = rs_clip(ar, lo, hi);
    const float cr = rs_clip(r, nhi, hi);
    acc[0] += 1.0;
    acc[1] += (double)ar;
    acc[2] += (double)r * (double)r;
    acc[3] += (double)t;
    acc[4] += (double)t * (double)t;
    acc[5] += (double)sm;
    acc[6] += (double)fabsf(t);
    acc[7] += (double)cw;
    acc[8] += (double)cr * (double)cr;
    outside += (ar < lo) || (ar > hi);
    if (ar != ar) ++nans;
    else mx = fmaxf(mx, ar);
  }
  double* row = rows + (size_t)blockIdx.x * RS_ROW;
  const double extra[3] = {(double)outside, (double)nans, (double)mx};
  for (int f = 0; f < RS_ROW; ++f) {
    s_acc[threadIdx.x] = f < RS_SUMS ? acc[f] : extra[f - RS_SUMS];
    __syncthreads();
    for (int h = RS_THREADS / 2; h > 0; h >>= 1) {      // fixed tree: reproducible
      if (threadIdx.x < h) {
        const double o = s_acc[threadIdx.x + h];
        s_acc[threadIdx.x] = f == RS_ROW - 1 ? fmax(s_acc[threadIdx.x], o) : s_acc[threadIdx.x] + o;
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) row[f] = s_acc[0];
    __syncthreads();
  }
}

// one workgroup: thread f sums column f of the rows in row order
__global__ __launch_bounds__(64) void k_rs_final(const double* __restrict__ rows, int n_rows, const float* __restrict__ xs,
                                                 const int64_t* __restrict__ nan_count, mmg_percentile_t plo,
                                                 mmg_percentile_t phi, mmg_percentile_t pq, double* __restrict__ out) {
  const int f = threadIdx.x;
  if (f < RS_ROW) {
    double s = 0.0;
    for (int r = 0; r < n_rows; ++r) {
      const double v = rows[(size_t)r * RS_ROW + f];
      s = f == RS_ROW - 1 ? (r == 0 ? v : fmax(s, v)) : s + v;
    }
    if (f == RS_ROW - 1 && nan_count[0] > 0) s = __builtin_nan("");   // np.max propagates NaN
    out[f] = s;
  }
  if (f == 0) {
    const bool any_nan = nan_count[0] > 0;
    out[MMG_RS_LOWER] = (double)rs_percentile(xs, plo, any_nan);
    out[MMG_RS_UPPER] = (double)rs_percentile(xs, phi, any_nan);
    out[MMG_RS_P95] = (double)rs_percentile(xs, pq, any_nan);
  }
}
int rs_grid(int64_t n) {
  int64_t g = (n + RS_THREADS * 8 - 1) / (RS_THREADS * 8);
  return (int)(g < 1 ? 1 : g > RS_MAX_GRID ? RS_MAX_GRID : g);
}
size_t rs_ws_need(int64_t n) { return (size_t)rs_grid(n) * RS_ROW * sizeof(double); }

// ------------------------------------------------------------------------------------------ split membership
__global__ __launch_bounds__(SM_THREADS) void k_sm_mark(const int64_t* __restrict__ pid, const uint8_t* __restrict__ m0,
                                                        const uint8_t* __restrict__ m1, const uint8_t* __restrict__ m2,
                                                        int64_t n_edges, int64_t n_pat, uint32_t* __restrict__ word,
                                                        unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_c[2];
  if (threadIdx.x < 2) s_c[threadIdx.x] = 0ull;
  __syncthreads();
  unsigned long long multi = 0, train_other = 0;
  const int64_t stride = (int64_t)gridDim.x * SM_THREADS;
  for (int64_t e = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; e < n_edges; e += stride) {
    const uint32_t m = (m0[e] ? 1u : 0u) | (m1[e] ? 2u : 0u) | (m2[e] ? 4u : 0u);
    if (!m) continue;
    multi += (m & (m - 1)) != 0;
    train_other += (m & 1u) && (m & 6u);
    const int64_t p = pid[e];
    if (p >= 0 && p < n_pat) atomicOr(&word[p], m);
  }
  if (multi) atomicAdd(&s_c[0], multi);
  if (train_other) atomicAdd(&s_c[1], train_other);
  __syncthreads();
  if (threadIdx.x < 2 && s_c[threadIdx.x]) atomicAdd(&counts[8 + threadIdx.x], s_c[threadIdx.x]);
}

__global__ __launch_bounds__(SM_THREADS) void k_sm_count(const uint32_t* __restrict__ word, int64_t n_pat,
                                                         unsigned long long* __restrict__ counts) {
  __shared__ unsigned long long s_c[8];
  if (threadIdx.x < 8) s_c[threadIdx.x] = 0ull;
  __syncthreads();
  const int64_t stride = (int64_t)gridDim.x * SM_THREADS;
  for (int64_t p = (int64_t)blockIdx.x * SM_THREADS + threadIdx.x; p < n_pat; p += stride) {
    const uint32_t w = word[p];
    if (w) atomicAdd(&s_c[w & 7u], 1ull);
  }
  __syncthreads();
  if (threadIdx.x > 0 && threadIdx.x < 8 && s_c[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_c[threadIdx.x]);
}

size_t sm_ws_need(int64_t n_pat) { return mmg_align256((size_t)(n_pat > 0 ? n_pat : 1) * sizeof(uint32_t)); }

int sm_grid(int64_t n) {
  int64_t g = (n + SM_THREADS * 8 - 1) / (SM_THREADS * 8);
  return (int)(g < 1 ? 1 : g > SM_MAX_GRID ? SM_MAX_GRID : g);
}

}  // namespace

extern "C" size_t mmg_order_stats_ws_bytes(int64_t n) {
  (void)n;
  return os_ws_need();
}

extern "C" int mmg_order_stats(const float* a, const float* b, int64_t n, const int64_t* ranks, int n_ranks, float* out,
                               int64_t* nan_count, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 1 && n <= INT32_MAX, "order_stats: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_ranks >= 1 && n_ranks <= MMG_OS_MAX_RANKS, "order_stats: %d ranks, 1..%d allowed", n_ranks,
                MMG_OS_MAX_RANKS);
  MMG_CHECK_ARG(a && out && ranks, "order_stats: null buffer");
  OsRanks rk = {};
  for (int r = 0; r < n_ranks; ++r) {
    MMG_CHECK_ARG(ranks[r] >= 0 && ranks[r] < n, "order_stats: rank %lld outside [0, %lld)", (long long)ranks[r],
                  (long long)n);
    rk.r[r] = ranks[r];
  }
  MMG_CHECK_WS("order_stats", os_ws_need());
  hipStream_t st = (hipStream_t)stream;
  uint32_t* hist = static_cast<uint32_t*>(ws);
  OsState* state = reinterpret_cast<OsState*>(static_cast<unsigned char*>(ws) + os_hist_bytes());
  const size_t hstep = (size_t)MMG_OS_MAX_RANKS * OS_BINS;
  MMG_CHECK_HIP(mmg_zero_async(hist, os_hist_bytes(), st), "order_stats(zero)");
  hipLaunchKernelGGL(k_os_init, dim3(1), dim3(OS_THREADS), 0, st, state, n_ranks, rk);
  MMG_CHECK_LAUNCH("order_stats(init)");
  const dim3 grid(os_grid(n)), pick(MMG_OS_MAX_RANKS * WAVE);
  hipLaunchKernelGGL(k_os_hist<0>, grid, dim3(OS_THREADS), 0, st, a, b, n, state, hist);
  MMG_CHECK_LAUNCH("order_stats(hist 0)");
  hipLaunchKernelGGL(k_os_pick<0>, dim3(1), pick, 0, st, state, hist, n_ranks, out, nan_count);
  MMG_CHECK_LAUNCH("order_stats(pick 0)");
  hipLaunchKernelGGL(k_os_hist<1>, grid, dim3(OS_THREADS), 0, st, a, b, n, state, hist + hstep);
  MMG_CHECK_LAUNCH("order_stats(hist 1)");
  hipLaunchKernelGGL(k_os_pick<1>, dim3(1), pick, 0, st, state, hist + hstep, n_ranks, out, nullptr);
  MMG_CHECK_LAUNCH("order_stats(pick 1)");
  hipLaunchKernelGGL(k_os_hist<2>, grid, dim3(OS_THREADS), 0, st, a, b, n, state, hist + 2 * hstep);
  MMG_CHECK_LAUNCH("order_stats(hist 2)");
  hipLaunchKernelGGL(k_os_pick<2>, dim3(1), pick, 0, st, state, hist + 2 * hstep, n_ranks, out, nullptr);
  MMG_CHECK_LAUNCH("order_stats(pick 2)");
  return MMG_OK;
}

extern "C" size_t mmg_robust_sums_ws_bytes(int64_t n) { return rs_ws_need(n < 1 ? 1 : n); }

extern "C" int mmg_robust_sums(const float* pred, const float* target, int64_t n, const float* xs, int n_xs,
                               const int64_t* nan_count, mmg_percentile_t lower, mmg_percentile_t upper,
                               mmg_percentile_t p95, double* out, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 1, "robust_sums: n %lld < 1", (long long)n);
  MMG_CHECK_ARG(n_xs >= 1 && n_xs <= MMG_OS_MAX_RANKS, "robust_sums: %d order statistics, 1..%d allowed", n_xs,
                MMG_OS_MAX_RANKS);
  const mmg_percentile_t* ps[3] = {&lower, &upper, &p95};
  for (const mmg_percentile_t* p : ps)
    MMG_CHECK_ARG(p->lo >= 0 && p->lo < n_xs && p->hi >= 0 && p->hi < n_xs,
                  "robust_sums: percentile reads order statistics %d / %d of %d", p->lo, p->hi, n_xs);
  MMG_CHECK_ARG(pred && target && xs && nan_count && out, "robust_sums: null buffer");
  MMG_CHECK_WS("robust_sums", rs_ws_need(n));
  hipStream_t st = (hipStream_t)stream;
  const int g = rs_grid(n);
  double* rows = static_cast<double*>(ws);
  hipLaunchKernelGGL(k_rs_partial, dim3(g), dim3(RS_THREADS), 0, st, pred, target, n, xs, nan_count, lower, upper, rows);
  MMG_CHECK_LAUNCH("robust_sums(partial)");
  hipLaunchKernelGGL(k_rs_final, dim3(1), dim3(64), 0, st, rows, g, xs, nan_count, lower, upper, p95, out);
  MMG_CHECK_LAUNCH("robust_sums(final)");
  return MMG_OK;
}

extern "C" size_t mmg_split_membership_ws_bytes(int64_t n_patients) { return sm_ws_need(n_patients); }

extern "C" int mmg_split_membership(const int64_t* patient, const uint8_t* train_mask, const uint8_t* val_mask,
                                    const uint8_t* test_mask, int64_t n_edges, int64_t n_patients, int64_t* counts,
                                    void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n_edges >= 0 && n_patients >= 0, "split_membership: negative size");
  MMG_CHECK_ARG(counts, "split_membership: null counts");
  MMG_CHECK_ARG(n_edges == 0 || (patient && train_mask && val_mask && test_mask), "split_membership: null buffer");
  MMG_CHECK_WS("split_membership", sm_ws_need(n_patients));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* word = static_cast<uint32_t*>(ws);
  auto* c = reinterpret_cast<unsigned long long*>(counts);
  MMG_CHECK_HIP(mmg_zero_async(counts, MMG_SM_FIELDS * sizeof(int64_t), st), "split_membership(zero counts)");
  if (n_patients == 0 || n_edges == 0) return MMG_OK;
  MMG_CHECK_HIP(mmg_zero_async(word, (size_t)n_patients * sizeof(uint32_t), st), "split_membership(zero words)");
  hipLaunchKernelGGL(k_sm_mark, dim3(sm_grid(n_edges)), dim3(SM_THREADS), 0, st, patient, train_mask, val_mask, test_mask,
                     n_edges, n_patients, word, c);
  MMG_CHECK_LAUNCH("split_membership(mark)");
  hipLaunchKernelGGL(k_sm_count, dim3(sm_grid(n_patients)), dim3(SM_THREADS), 0, st, word, n_patients, c);
  MMG_CHECK_LAUNCH("split_membership(count)");
  return MMG_OK;
}
