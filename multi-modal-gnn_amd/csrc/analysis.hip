// Prediction-analysis reducers (reference src/advanced_visualizations.py: per-lab calibration :169-267, error against
// patient lab-degree :105-166, parity by lab-frequency decile :32-102; mmgnn/analysis.py).  A pair is (pred f32,
// target f32, patient index, lab index); every table of that file is a set of sums over ALL pairs:
//   mmg_pair_analysis        one read of the pairs -> per lab  n, sum t, sum p, sum t^2, sum t p, sum |p - t|,
//                            sum (p - t)^2, min t, max t;  per degree bin  n, sum |p - t|  (bin of deg[patient])
//   mmg_pair_calibrated_abs  second read, with the line (a, b) of every lab and the mean error of every bin from the
//                            first:  per lab sum |(a t + b) - t|,  per bin sum (|p - t| - mean_bin)^2
// The elementwise terms are formed in fp32 as numpy forms them on fp32 arrays (p - t, |.|, the square, a * t + b with
// every operation rounded on its own); everything is summed in fp64.
//
// Reduction order (fixed, so the result is bitwise the same from run to run).  The pairs are cut into one contiguous
// chunk per WAVE; a wave walks its chunk 64 pairs at a time, lane l taking pair base + l.
//   labs  every lane keeps the sums of its current run of equal lab indices in registers and flushes them into the
//         wave's OWN LDS table when its lab changes (in lab-major edge order that is once per lab, in patient-major or
//         shuffled order at every pair).  A flush is a wave-wide step: while the lowest flushing lane's lab is shared by
//         >= 4 flushing lanes, that group is summed across the lanes by a fixed butterfly and added by lane 0.  This
//         stage stops at the FIRST small group (looking further would cost a step per distinct lab, ~40 in shuffled
//         order), even if a later group is large; every lane still flushing then takes its turn, lowest lane first per
//         lab (an integer ds_min picks it; a turn is that atomic, two wavefront fences and plain LDS reads and writes of
//         the lane's registers).  In shuffled or patient-major order this second stage does nearly all the work.  No
//         floating-point atomic anywhere.
//   bins  every lane owns one LDS slot per bin ([bin][lane]: conflict-free), summed across the lanes at the end.
// The waves of a workgroup add their tables in wave order into one row of the workspace; one wave per output adds the
// rows in a fixed order.  Which lane adds what when depends only on n, the table sizes and the order of the pairs.
//
// LDS of a wave: 64 n_labs + 768 n_bins bytes in the first pass (50 labs, 4 bins: 6.1 KB -- four waves per workgroup and
// several workgroups per CU), 16 n_labs + 768 n_bins in the second; a workgroup has 4, 2 or 1 waves, as many as fit
// 160 KB.  2048 labs fit with up to 42 bins, 64 bins with up to 1792 labs.
#include "common.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int AN_MAX_LABS = 2048;
constexpr int AN_LDS_BYTES = 160 * 1024;
constexpr int AN_BIG = 4;               // lanes sharing a lab from which the cross-lane sum beats taking turns
constexpr int AN_UNROLL = 2;            // 64-pair steps whose loads are issued together

struct AnEdges {
  double e[MMG_AN_MAX_BINS + 1];
};

struct AnGeom {
  int waves, grid, row_len;
  int64_t chunk;
  size_t lds;
};

constexpr int an_nf(bool pass2) { return pass2 ? 1 : 6; }
constexpr int an_doubles(bool pass2, int L, int B) { return an_nf(pass2) * L + 64 * B; }
constexpr int an_ints(bool pass2, int L, int B) { return (pass2 ? 2 : 4) * L + 64 * B; }

bool an_geom(bool pass2, int64_t n, int L, int B, AnGeom* g) {
  const size_t per = (size_t)an_doubles(pass2, L, B) * 8 + (size_t)an_ints(pass2, L, B) * 4;
  if (per > (size_t)AN_LDS_BYTES) return false;
  g->waves = 4 * per <= (size_t)AN_LDS_BYTES ? 4 : 2 * per <= (size_t)AN_LDS_BYTES ? 2 : 1;
  const int cap = 256 * g->waves;                     // <= 1024 workgroups: the rows of the workspace
  int64_t wg = (n + 64 * 16 * g->waves - 1) / (64 * 16 * g->waves);
  g->grid = (int)(wg < 1 ? 1 : wg > cap ? cap : wg);
  const int64_t nw = (int64_t)g->grid * g->waves;
  g->chunk = ((n + nw - 1) / nw + 63) / 64 * 64;
  g->row_len = pass2 ? L + B : MMG_AN_LAB_FIELDS * L + MMG_AN_BIN_FIELDS * B;
  g->lds = per * g->waves;
  return true;
}

__device__ __forceinline__ void an_wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// |(a t + b) - t| as numpy forms it on fp32 operands: every operation rounded on its own
__device__ __forceinline__ float an_calibrated_abs(float a, float b, float t) {
#pragma clang fp contract(off)
  const float c = a * t + b;
  return fabsf(c - t);
}
__device__ __forceinline__ float an_square(float r) {
#pragma clang fp contract(off)
  return r * r;
}

// the table of one wave
template <int NF, bool MM>
struct AnTab {
  double* sum;      // [NF][n_labs]
  double* bsum;     // [n_bins][64]
  float* mm;        // [2][n_labs]: min t, max t (MM)
  int* cnt;         // [n_labs]
  int* claim;       // [n_labs]: the lane whose turn it is
  int* bcnt;        // [n_bins][64]
  int L;
};

// the run a lane holds in registers
template <int NF>
struct AnRun {
  double v[NF];
  float mn, mx;
  int c, key;
  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int f = 0; f < NF; ++f) v[f] = 0.0;
    mn = INFINITY; mx = -INFINITY; c = 0; key = -1;
  }
};

// Every lane of the wave calls this (uniform control flow); the lanes with fl add their run to the wave's table.
template <int NF, bool MM>
__device__ __forceinline__ void an_flush(bool fl, const AnRun<NF>& r, const AnTab<NF, MM>& T, int lane) {
  unsigned long long rem = __ballot(fl);
  while (rem) {
    const int src = __ffsll((long long)rem) - 1;
    const int k0 = __shfl(r.key, src, 64);
    const bool in = fl && r.key == k0;
    const unsigned long long m = __ballot(in);
    if (__popcll(m) < AN_BIG) break;
#pragma unroll
    for (int f = 0; f < NF; ++f) {
      const double s = wave_sum_d(in ? r.v[f] : 0.0);
      if (lane == 0) T.sum[f * T.L + k0] += s;
    }
    const int cs = wave_sum_i(in ? r.c : 0);
    if (lane == 0) T.cnt[k0] += cs;
    if (MM) {
      const float lo = wave_min_f(in ? r.mn : INFINITY), hi = wave_max_f(in ? r.mx : -INFINITY);
      if (lane == 0) {
        T.mm[k0] = fminf(T.mm[k0], lo);
        T.mm[T.L + k0] = fmaxf(T.mm[T.L + k0], hi);
      }
    }
    fl = fl && !in;
    rem &= ~m;
    an_wave_fence();
  }
  while (__ballot(fl)) {
    if (fl) atomicMin(&T.claim[r.key], lane);
    an_wave_fence();
    if (fl && T.claim[r.key] == lane) {
#pragma unroll
      for (int f = 0; f < NF; ++f) T.sum[f * T.L + r.key] += r.v[f];
      T.cnt[r.key] += r.c;
      if (MM) {
        T.mm[r.key] = fminf(T.mm[r.key], r.mn);
        T.mm[T.L + r.key] = fmaxf(T.mm[T.L + r.key], r.mx);
      }
      T.claim[r.key] = INT_MAX;
      fl = false;
    }
    an_wave_fence();
  }
}

template <typename IT>
__device__ __forceinline__ int an_index(const IT* __restrict__ p, int64_t i, int64_t limit) {
  const int64_t v = (int64_t)p[i];
  return v >= 0 && v < limit ? (int)v : -1;
}

template <typename IT, bool PASS2>
__global__ __launch_bounds__(256) void k_pair_analysis(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const IT* __restrict__ patient, const IT* __restrict__ lab,
                                                       int64_t n, int64_t chunk, int L, const int32_t* __restrict__ deg,
                                                       int64_t n_pat, int B, AnEdges edges, const float* __restrict__ ca,
                                                       const float* __restrict__ cb, const double* __restrict__ bmean,
                                                       double* __restrict__ partial) {
  constexpr int NF = an_nf(PASS2);
  constexpr bool MM = !PASS2;
  extern __shared__ double an_lds[];
  const int W = blockDim.x / WAVE;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE), lane = threadIdx.x % WAVE;
  const int nd = an_doubles(PASS2, L, B), ni = an_ints(PASS2, L, B);
  AnTab<NF, MM> T;
  T.L = L;
  T.sum = an_lds + (size_t)w * nd;
  T.bsum = T.sum + NF * L;
  int* ib = reinterpret_cast<int*>(an_lds + (size_t)W * nd) + (size_t)w * ni;
  T.mm = reinterpret_cast<float*>(ib);
  T.cnt = ib + (MM ? 2 * L : 0);
  T.claim = T.cnt + L;
  T.bcnt = T.claim + L;
  for (int i = lane; i < nd; i += WAVE) T.sum[i] = 0.0;
  for (int i = lane; i < L; i += WAVE) {
    if (MM) {
      T.mm[i] = INFINITY;
      T.mm[L + i] = -INFINITY;
    }
    T.cnt[i] = 0;
    T.claim[i] = INT_MAX;
  }
  for (int i = lane; i < 64 * B; i += WAVE) T.bcnt[i] = 0;
  an_wave_fence();

  const bool labs = L > 0, bins = B > 0;
  AnRun<NF> run;
  run.reset();
  const int64_t c0 = ((int64_t)blockIdx.x * W + w) * chunk;
  const int64_t c1 = c0 + chunk < n ? c0 + chunk : n;
  for (int64_t base = c0; base < c1; base += (int64_t)WAVE * AN_UNROLL) {
    float p[AN_UNROLL], t[AN_UNROLL];
    int k[AN_UNROLL], d[AN_UNROLL];
#pragma unroll
    for (int u = 0; u < AN_UNROLL; ++u) {
      const int64_t i = base + u * WAVE + lane;
      const bool ok = i < c1;
      p[u] = 0.f; t[u] = 0.f; k[u] = -1; d[u] = -1;
      if (ok) {
        t[u] = target[i];
        if (!PASS2 || bins) p[u] = pred[i];
        if (labs) k[u] = an_index(lab, i, L);
        if (bins) d[u] = an_index(patient, i, n_pat);     // bounds-checked before it is used as an address
      }
    }
#pragma unroll
    for (int u = 0; u < AN_UNROLL; ++u)
      if (d[u] >= 0) d[u] = deg[d[u]];
#pragma unroll
    for (int u = 0; u < AN_UNROLL; ++u) {
      if (base + u * WAVE >= c1) break;                     // (uniform)
      const float r = p[u] - t[u];
      const float ae = fabsf(r);
      if (labs) {
        const bool fl = run.key >= 0 && run.key != k[u];
        if (__ballot(fl)) an_flush<NF, MM>(fl, run, T, lane);
        if (fl) run.reset();
        if (k[u] >= 0) {
          run.key = k[u];
          run.c += 1;
          if (PASS2) {
            run.v[0] += (double)an_calibrated_abs(ca[k[u]], cb[k[u]], t[u]);
          } else {
            const double td = (double)t[u], pd = (double)p[u];
            run.v[0] += td;
            run.v[1] += pd;
            run.v[2] += td * td;                            // (exact products of fp32 values: fusing changes nothing)
            run.v[3] += td * pd;
            run.v[4] += (double)ae;
            run.v[NF - 1] += (double)an_square(r);
            run.mn = fminf(run.mn, t[u]);
            run.mx = fmaxf(run.mx, t[u]);
          }
        }
      }
      if (bins && d[u] >= 0) {
        const double dd = (double)d[u];
        int b = -1;
        for (int j = 0; j < B; ++j)
          if (dd >= edges.e[j] && dd < edges.e[j + 1]) b = j;
        if (b >= 0) {
          if (PASS2) {
            const double x = (double)ae - bmean[b];
            T.bsum[b * WAVE + lane] += x * x;
          } else {
            T.bsum[b * WAVE + lane] += (double)ae;
            T.bcnt[b * WAVE + lane] += 1;
          }
        }
      }
    }
  }
  if (labs) {
    const bool fl = run.key >= 0;
    if (__ballot(fl)) an_flush<NF, MM>(fl, run, T, lane);
  }
  an_wave_fence();
  for (int b = 0; b < B; ++b) {
    const double s = wave_sum_d(T.bsum[b * WAVE + lane]);
    const int c = wave_sum_i(T.bcnt[b * WAVE + lane]);
    an_wave_fence();
    if (lane == 0) {
      T.bsum[b * WAVE] = s;
      T.bcnt[b * WAVE] = c;
    }
  }
  __syncthreads();

  // the waves' tables in wave order -> one row
  const int row_len = PASS2 ? L + B : MMG_AN_LAB_FIELDS * L + MMG_AN_BIN_FIELDS * B;
  double* row = partial + (size_t)blockIdx.x * row_len;
  const int* ib0 = reinterpret_cast<const int*>(an_lds + (size_t)W * nd);
  for (int i = threadIdx.x; i < row_len; i += blockDim.x) {
    double s;
    if (i < NF * L) {
      s = 0.0;
      for (int q = 0; q < W; ++q) s += an_lds[(size_t)q * nd + i];
    } else if (!PASS2 && i < 7 * L) {
      int c = 0;
      for (int q = 0; q < W; ++q) c += ib0[(size_t)q * ni + 2 * L + (i - 6 * L)];
      s = (double)c;
    } else if (!PASS2 && i < 9 * L) {
      const bool mx = i >= 8 * L;
      const int j = i - 7 * L;                               // [0, 2 L): the (min | max) array
      float v = mx ? -INFINITY : INFINITY;
      for (int q = 0; q < W; ++q) {
        const float x = reinterpret_cast<const float*>(ib0 + (size_t)q * ni)[j];
        v = mx ? fmaxf(v, x) : fminf(v, x);
      }
      s = (double)v;
    } else {
      const int j = i - (PASS2 ? L : 9 * L);                 // [0, B) sums, [B, 2 B) counts (first pass)
      if (j < B) {
        s = 0.0;
        for (int q = 0; q < W; ++q) s += an_lds[(size_t)q * nd + NF * L + j * WAVE];
      } else {
        int c = 0;
        for (int q = 0; q < W; ++q) c += ib0[(size_t)q * ni + 4 * L + (j - B) * WAVE];
        s = (double)c;
      }
    }
    row[i] = s;
  }
}

// one wave per row element: the rows in a fixed order, then into the caller's layout
template <bool PASS2>
__global__ __launch_bounds__(256) void k_pair_analysis_final(const double* __restrict__ partial, int n_rows, int L, int B,
                                                             double* __restrict__ lab_out, double* __restrict__ bin_out) {
  const int row_len = PASS2 ? L + B : MMG_AN_LAB_FIELDS * L + MMG_AN_BIN_FIELDS * B;
  const int lane = threadIdx.x & 63;
  const int i = (blockIdx.x * 256 + threadIdx.x) >> 6;
  if (i >= row_len) return;
  const int mode = (!PASS2 && i >= 7 * L && i < 9 * L) ? (i >= 8 * L ? 2 : 1) : 0;
  double s = mode == 0 ? 0.0 : mode == 1 ? (double)INFINITY : -(double)INFINITY;
  for (int b = lane; b < n_rows; b += 64) {
    const double v = partial[(size_t)b * row_len + i];
    s = mode == 0 ? s + v : mode == 1 ? fmin(s, v) : fmax(s, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double v = __shfl_xor(s, o, 64);
    s = mode == 0 ? s + v : mode == 1 ? fmin(s, v) : fmax(s, v);
  }
  if (lane) return;
  if (PASS2) {
    if (i < L) lab_out[i] = s;
    else bin_out[i - L] = s;
    return;
  }
  if (i < 9 * L) {
    // row order: 6 sums, count, min, max -> fields n, sum t, sum p, sum t^2, sum t p, sum |e|, sum e^2, min t, max t
    const int f = i / L, k = i - f * L;
    const int field = f < 6 ? f + 1 : f == 6 ? 0 : f;
    lab_out[(size_t)k * MMG_AN_LAB_FIELDS + field] = s;
  } else {
    const int j = i - 9 * L;
    if (j < B) bin_out[j * MMG_AN_BIN_FIELDS + 1] = s;
    else bin_out[(j - B) * MMG_AN_BIN_FIELDS] = s;
  }
}

size_t an_ws_need(const AnGeom& g) { return (size_t)g.grid * g.row_len * sizeof(double) + 256; }

int an_check(const char* what, const void* pred, const void* target, const void* patient, const void* lab, int index_bytes,
             int64_t n, int L, const int32_t* deg, int64_t n_pat, const double* edges, int B, AnEdges* ed) {
  MMG_CHECK_ARG(n >= 0 && n <= INT32_MAX, "%s: n %lld outside [0, 2^31)", what, (long long)n);
  MMG_CHECK_ARG(L >= 0 && L <= AN_MAX_LABS, "%s: %d labs, at most %d (use the host arithmetic beyond)", what, L,
                AN_MAX_LABS);
  MMG_CHECK_ARG(B >= 0 && B <= MMG_AN_MAX_BINS, "%s: %d degree bins, at most %d", what, B, MMG_AN_MAX_BINS);
  MMG_CHECK_ARG(L > 0 || B > 0, "%s: neither labs nor degree bins requested", what);
  MMG_CHECK_ARG(index_bytes == 4 || index_bytes == 8, "%s: indices of %d bytes (int32 or int64)", what, index_bytes);
  MMG_CHECK_ARG(n == 0 || target, "%s: null target", what);
  MMG_CHECK_ARG(n == 0 || L == 0 || lab, "%s: null lab indices", what);
  if (B > 0) {
    MMG_CHECK_ARG(edges, "%s: null bin edges", what);
    MMG_CHECK_ARG(n_pat >= 0 && n_pat <= INT32_MAX, "%s: %lld patients outside [0, 2^31)", what, (long long)n_pat);
    MMG_CHECK_ARG(n == 0 || (pred && patient && deg), "%s: degree bins need pred, the patient indices and deg", what);
    for (int j = 0; j <= B; ++j) {
      MMG_CHECK_ARG(edges[j] == edges[j] && (j == 0 || edges[j] > edges[j - 1]),
                    "%s: bin edges must be ascending (edge %d)", what, j);
      ed->e[j] = edges[j];
    }
  }
  return MMG_OK;
}

}  // namespace

extern "C" size_t mmg_pair_analysis_ws_bytes(int64_t n, int n_labs, int n_bins) {
  AnGeom g;
  if (n < 0 || n_labs < 0 || n_labs > AN_MAX_LABS || n_bins < 0 || n_bins > MMG_AN_MAX_BINS || n_labs + n_bins == 0 ||
      !an_geom(false, n, n_labs, n_bins, &g))
    return 0;
  return an_ws_need(g);
}

extern "C" int mmg_pair_analysis(const float* pred, const float* target, const void* patient, const void* lab,
                                 int index_bytes, int64_t n, int n_labs, const int32_t* deg, int64_t n_patients,
                                 const double* bin_edges, int n_bins, double* lab_sums, double* bin_sums, void* ws,
                                 size_t ws_bytes, void* stream) {
  AnEdges ed = {};
  int rc = an_check("pair_analysis", pred, target, patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges,
                    n_bins, &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(n == 0 || pred, "pair_analysis: null pred");
  MMG_CHECK_ARG((n_labs == 0 || lab_sums) && (n_bins == 0 || bin_sums), "pair_analysis: null output");
  AnGeom g;
  MMG_CHECK_ARG(an_geom(false, n, n_labs, n_bins, &g),
                "pair_analysis: %d labs and %d bins need more than %d bytes of LDS (64 per lab, 768 per bin)", n_labs,
                n_bins, AN_LDS_BYTES);
  MMG_CHECK_WS("pair_analysis", an_ws_need(g));
  hipStream_t st = (hipStream_t)stream;
  double* partial = MmgCarver(ws).take<double>((size_t)g.grid * g.row_len);
  const dim3 grid(g.grid), block(g.waves * WAVE);
  if (index_bytes == 8) {
    MMG_CHECK_HIP((MmgMaxLds<&k_pair_analysis<int64_t, false>, AN_LDS_BYTES>::set()), "pair_analysis(attr)");
    hipLaunchKernelGGL((k_pair_analysis<int64_t, false>), grid, block, g.lds, st, pred, target, (const int64_t*)patient,
                       (const int64_t*)lab, n, g.chunk, n_labs, deg, n_patients, n_bins, ed, nullptr, nullptr, nullptr,
                       partial);
  } else {
    MMG_CHECK_HIP((MmgMaxLds<&k_pair_analysis<int32_t, false>, AN_LDS_BYTES>::set()), "pair_analysis(attr)");
    hipLaunchKernelGGL((k_pair_analysis<int32_t, false>), grid, block, g.lds, st, pred, target, (const int32_t*)patient,
                       (const int32_t*)lab, n, g.chunk, n_labs, deg, n_patients, n_bins, ed, nullptr, nullptr, nullptr,
                       partial);
  }
  MMG_CHECK_LAUNCH("pair_analysis");
  hipLaunchKernelGGL(k_pair_analysis_final<false>, dim3((g.row_len + 3) / 4), dim3(256), 0, st, partial, g.grid, n_labs,
                     n_bins, lab_sums, bin_sums);
  MMG_CHECK_LAUNCH("pair_analysis(final)");
  return MMG_OK;
}

extern "C" size_t mmg_pair_calibrated_abs_ws_bytes(int64_t n, int n_labs, int n_bins) {
  AnGeom g;
  if (n < 0 || n_labs < 0 || n_labs > AN_MAX_LABS || n_bins < 0 || n_bins > MMG_AN_MAX_BINS || n_labs + n_bins == 0 ||
      !an_geom(true, n, n_labs, n_bins, &g))
    return 0;
  return an_ws_need(g);
}

extern "C" int mmg_pair_calibrated_abs(const float* pred, const float* target, const void* patient, const void* lab,
                                       int index_bytes, int64_t n, int n_labs, const float* a, const float* b,
                                       const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                                       const double* bin_mean, double* lab_abs, double* bin_sq, void* ws, size_t ws_bytes,
                                       void* stream) {
  AnEdges ed = {};
  int rc = an_check("pair_calibrated_abs", pred, target, patient, lab, index_bytes, n, n_labs, deg, n_patients, bin_edges,
                    n_bins, &ed);
  if (rc) return rc;
  MMG_CHECK_ARG(n_labs == 0 || (a && b && lab_abs), "pair_calibrated_abs: labs need a, b and lab_abs");
  MMG_CHECK_ARG(n_bins == 0 || (bin_mean && bin_sq), "pair_calibrated_abs: degree bins need bin_mean and bin_sq");
  AnGeom g;
  MMG_CHECK_ARG(an_geom(true, n, n_labs, n_bins, &g),
                "pair_calibrated_abs: %d labs and %d bins need more than %d bytes of LDS", n_labs, n_bins, AN_LDS_BYTES);
  MMG_CHECK_WS("pair_calibrated_abs", an_ws_need(g));
  hipStream_t st = (hipStream_t)stream;
  double* partial = MmgCarver(ws).take<double>((size_t)g.grid * g.row_len);
  const dim3 grid(g.grid), block(g.waves * WAVE);
  if (index_bytes == 8) {
    MMG_CHECK_HIP((MmgMaxLds<&k_pair_analysis<int64_t, true>, AN_LDS_BYTES>::set()), "pair_calibrated_abs(attr)");
    hipLaunchKernelGGL((k_pair_analysis<int64_t, true>), grid, block, g.lds, st, pred, target, (const int64_t*)patient,
                       (const int64_t*)lab, n, g.chunk, n_labs, deg, n_patients, n_bins, ed, a, b, bin_mean, partial);
  } else {
    MMG_CHECK_HIP((MmgMaxLds<&k_pair_analysis<int32_t, true>, AN_LDS_BYTES>::set()), "pair_calibrated_abs(attr)");
    hipLaunchKernelGGL((k_pair_analysis<int32_t, true>), grid, block, g.lds, st, pred, target, (const int32_t*)patient,
                       (const int32_t*)lab, n, g.chunk, n_labs, deg, n_patients, n_bins, ed, a, b, bin_mean, partial);
  }
  MMG_CHECK_LAUNCH("pair_calibrated_abs");
  hipLaunchKernelGGL(k_pair_analysis_final<true>, dim3((g.row_len + 3) / 4), dim3(256), 0, st, partial, g.grid, n_labs,
                     n_bins, lab_abs, bin_sq);
  MMG_CHECK_LAUNCH("pair_calibrated_abs(final)");
  return MMG_OK;
}
