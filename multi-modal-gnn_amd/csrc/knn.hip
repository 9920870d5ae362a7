// Nearest-neighbour lab imputation (mmg_knn_impute): sklearn KNNImputer(n_neighbors = k, weights) .fit_transform(X)
// over a dense patient x lab matrix with NaN = missing, every row both donor and receiver (include/mmgnn.h).
//
// Two launches:
//   k_knn_col_mean   one workgroup per lab: fp64 mean of the observed cells (the all-NaN-distance fallback; NaN for a
//                    lab nobody has, which is then every missing cell's value).
//   k_knn_impute<KT> one workgroup per RT requested rows.  It streams the donor rows through LDS in tiles of T
//                    (lab-major, row stride T + 4), and per tile
//                      1. every (receiver, donor) pair of the tile gets q = S / c, S = sum over the labs both observe of
//                         (x_r - x_d)^2 in lab order, c = their number (NaN when c = 0): one wave per receiver, a lane per
//                         donor, a loop over the receiver's observed labs only;
//                      2. every lane that owns a (receiver, missing lab) cell scans the tile in donor order and keeps the
//                         KT smallest q of the donors that observe its lab in a sorted register list.
//                    q ranks like the distance sqrt(L * q) (L does not change the order), and because the donors arrive in
//                    increasing index order a strict comparison breaks ties by the lower index.  A cell list longer than
//                    the workgroup (RT * L > 256 missing cells) is worked in passes over the donors.
// Every cell's value depends only on its own row, the donors and k: the pair sums run in lab order and the selection is
// a total order, so results are bitwise the same whatever the tiling and whichever other rows are requested.
#include "common.h"

namespace {

constexpr int KNN_THREADS = 256;
constexpr int KNN_MAX_RT = 16;
constexpr int KNN_LDS_MAX = 150 * 1024;    // dynamic LDS limit raised once: the L = 512 shape takes 142 KiB (+ 128 B static)

struct KnnShape {
  int T;        // donors per tile (64, 128 or 256: one wave spans a receiver's row of the tile)
  int ldt;      // LDS row stride of the tile and of the q table (T + 4: 16-byte rows, lab rows spread over the banks)
  int RT;       // receivers per workgroup
  size_t lds;   // dynamic LDS bytes
};

static KnnShape knn_shape(int L) {
  KnnShape s;
  int T = 256;
  while (T > 64 && (size_t)T * (L + 4) * sizeof(float) > 40 * 1024) T >>= 1;
  s.T = T;
  s.ldt = T + 4;
  int rt = 384 / L;                     // ~1.5 workgroups of cells at half the labs missing
  s.RT = rt < 1 ? 1 : rt > KNN_MAX_RT ? KNN_MAX_RT : rt;
  // tile [L + 1][ldt] (+ a NaN row) + q [RT][ldt] floats, observed (value, lab offset) [RT][pad4(L)] float2, missing labs
  // [RT][L] int
  s.lds = ((size_t)(L + 1) * s.ldt + (size_t)s.RT * s.ldt) * sizeof(float) +
          (size_t)s.RT * (((L + 3) & ~3) * 2 * sizeof(float) + L * sizeof(int));
  return s;
}

__global__ __launch_bounds__(256) void k_knn_col_mean(const float* __restrict__ X, int64_t n_rows, int64_t ld_x,
                                                      float* __restrict__ col_mean) {
  __shared__ double s_sum[256];
  __shared__ int s_cnt[256];
  const int l = blockIdx.x, t = threadIdx.x;
  double s = 0.0;
  int c = 0;
#pragma unroll 4
  for (int64_t r = t; r < n_rows; r += 256) {
    const float v = X[r * ld_x + l];
    if (v == v) {
      s += (double)v;
      ++c;
    }
  }
  s_sum[t] = s;
  s_cnt[t] = c;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {          // fixed tree: reproducible
    if (t < h) {
      s_sum[t] += s_sum[t + h];
      s_cnt[t] += s_cnt[t + h];
    }
    __syncthreads();
  }
  if (t == 0) col_mean[l] = s_cnt[0] > 0 ? (float)(s_sum[0] / (double)s_cnt[0]) : __builtin_nanf("");
}

// Sorted (q, x) list of the KT best donors so far; the candidate arrives after every listed donor (higher index), so it
// goes behind the entries of equal q.
template <int KT>
__device__ __forceinline__ void knn_insert(float (&lq)[KT], float (&lx)[KT], float q, float x) {
  bool sh = false;
  float cq = q, cx = x;
#pragma unroll
  for (int s = 0; s < KT; ++s) {
    sh = sh || q < lq[s];
    const float tq = lq[s], tx = lx[s];
    lq[s] = sh ? cq : tq;
    lx[s] = sh ? cx : tx;
    cq = sh ? tq : cq;
    cx = sh ? tx : cx;
  }
}

template <int KT>
__global__ __launch_bounds__(KNN_THREADS) void k_knn_impute(
    const float* __restrict__ X, int n_rows, int L, int64_t ld_x, const int32_t* __restrict__ rows, int64_t n_out,
    int k, int weights, const float* __restrict__ col_mean, float* __restrict__ out, int64_t ld_out, int T, int RT) {
  extern __shared__ float4 knn_lds4[];
  __shared__ int s_nobs[KNN_MAX_RT], s_nmiss[KNN_MAX_RT];
  const int ldt = T + 4;
  const int Lp = (L + 3) & ~3;
  float* sD = reinterpret_cast<float*>(knn_lds4);        // [L][ldt] donor tile, lab-major; row L: NaN
  float* sQ = sD + (size_t)(L + 1) * ldt;                // [RT][ldt] q per (receiver, donor of the tile)
  float2* sR = reinterpret_cast<float2*>(sQ + (size_t)RT * ldt);   // [RT][Lp] (x_r, lab * ldt) of the observed labs,
                                                                   // padded to a multiple of 4 with (0, the NaN row)
  int* sMiss = reinterpret_cast<int*>(sR + (size_t)RT * Lp);       // [RT][L] the missing labs
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * RT;
  for (int dd = t; dd < T; dd += KNN_THREADS) sD[L * ldt + dd] = __builtin_nanf("");

  // receivers: observed labs (compacted, in lab order; their values go straight to out) and missing labs
  for (int i = wave; i < RT; i += KNN_THREADS / 64) {
    const int64_t gi = i0 + i;
    const int r = gi < n_out ? rows[gi] : -1;
    int nobs = 0, nmiss = 0;
    if (r >= 0 && r < n_rows) {
      const float* xr = X + (int64_t)r * ld_x;
      float* o = out + gi * ld_out;
      for (int jb = 0; jb < L; jb += 64) {
        const int j = jb + lane;
        const float v = j < L ? xr[j] : 0.f;
        const bool ob = j < L && v == v, mi = j < L && !(v == v);
        const uint64_t bo = __ballot(ob), bm = __ballot(mi);
        const int below_o = __builtin_amdgcn_mbcnt_hi((uint32_t)(bo >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bo, 0));
        const int below_m = __builtin_amdgcn_mbcnt_hi((uint32_t)(bm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bm, 0));
        if (ob) {
          sR[i * Lp + nobs + below_o] = make_float2(v, __int_as_float(j * ldt));
          o[j] = v;
        }
        if (mi) sMiss[i * L + nmiss + below_m] = j;
        nobs += __popcll(bo);
        nmiss += __popcll(bm);
      }
    }
    if (lane < ((nobs + 3) & ~3) - nobs) sR[i * Lp + nobs + lane] = make_float2(0.f, __int_as_float(L * ldt));
    if (lane == 0) {
      s_nobs[i] = nobs;
      s_nmiss[i] = nmiss;
    }
  }
  __syncthreads();
  int n_cells = 0;
  for (int i = 0; i < RT; ++i) n_cells += s_nmiss[i];

  for (int base = 0; base < n_cells; base += KNN_THREADS) {
    // this lane's cell: (receiver ci, lab cl)
    const int cell = base + t;
    const bool active = cell < n_cells;
    int ci = 0, cl = 0;
    if (active) {
      int c = cell;
      while (c >= s_nmiss[ci]) c -= s_nmiss[ci++];
      cl = sMiss[ci * L + c];
    }
    float lq[KT], lx[KT];
#pragma unroll
    for (int s = 0; s < KT; ++s) {
      lq[s] = __builtin_inff();
      lx[s] = 0.f;
    }

    for (int64_t d0 = 0; d0 < n_rows; d0 += T) {
      __syncthreads();                                   // the previous tile's scan is done with sD / sQ
      // stage the tile: a wave writes 8 donors x 8 labs per step (conflict-free: banks 4 * lab + donor)
      for (int rb = wave * 8; rb < T; rb += 8 * (KNN_THREADS / 64)) {
        const int dd = rb + (lane >> 3);
        const int64_t d = d0 + dd;
        const float* xd = X + d * ld_x;
        for (int jb = 0; jb < L; jb += 8) {
          const int j = jb + (lane & 7);
          if (j < L) sD[j * ldt + dd] = d < n_rows ? xd[j] : __builtin_nanf("");
        }
      }
      __syncthreads();
      // 1. q of every (receiver, donor) pair of the tile (T is a multiple of 64: one receiver per wave)
      for (int p = t; p < RT * T; p += KNN_THREADS) {
        const int i = p / T, dd = p - i * T;
        const int n4 = (s_nobs[i] + 3) & ~3;
        const float4* ri = reinterpret_cast<const float4*>(sR + i * Lp);   // two (x_r, offset) entries each
        float s = 0.f;
        int c = 0;
        // four labs per step (their tile reads issued together); the padding reads the NaN row and adds nothing
        for (int o = 0; o < n4 / 2; o += 2) {
          const float4 e01 = ri[o], e23 = ri[o + 1];
          const float x0 = sD[__float_as_int(e01.y) + dd], x1 = sD[__float_as_int(e01.w) + dd];
          const float x2 = sD[__float_as_int(e23.y) + dd], x3 = sD[__float_as_int(e23.w) + dd];
          const float d0 = e01.x - x0, d1 = e01.z - x1, d2 = e23.x - x2, d3 = e23.z - x3;
          s += x0 == x0 ? d0 * d0 : 0.f;
          s += x1 == x1 ? d1 * d1 : 0.f;
          s += x2 == x2 ? d2 * d2 : 0.f;
          s += x3 == x3 ? d3 * d3 : 0.f;
          c += (x0 == x0) + (x1 == x1) + (x2 == x2) + (x3 == x3);
        }
        sQ[i * ldt + dd] = c > 0 ? s / (float)c : __builtin_nanf("");
      }
      __syncthreads();
      // 2. the cells' running selection over the tile's donors, in donor order (NaN x: not a donor; NaN q: never listed)
      if (active) {
        const float* qrow = sQ + ci * ldt;
        const float* xrow = sD + cl * ldt;
        for (int dd = 0; dd < T; dd += 4) {
          const float4 q4 = *reinterpret_cast<const float4*>(qrow + dd);
          const float4 x4 = *reinterpret_cast<const float4*>(xrow + dd);
          const float thr = lq[KT - 1];
          // one branch per 4 donors on the common path (nothing enters); the entries re-test the moving threshold
          if ((x4.x == x4.x && q4.x < thr) || (x4.y == x4.y && q4.y < thr) || (x4.z == x4.z && q4.z < thr) ||
              (x4.w == x4.w && q4.w < thr)) {
            if (x4.x == x4.x && q4.x < lq[KT - 1]) knn_insert<KT>(lq, lx, q4.x, x4.x);
            if (x4.y == x4.y && q4.y < lq[KT - 1]) knn_insert<KT>(lq, lx, q4.y, x4.y);
            if (x4.z == x4.z && q4.z < lq[KT - 1]) knn_insert<KT>(lq, lx, q4.z, x4.z);
            if (x4.w == x4.w && q4.w < lq[KT - 1]) knn_insert<KT>(lq, lx, q4.w, x4.w);
          }
        }
      }
    }

    if (active) {
      // the first min(k, listed) donors: the donors at a NaN distance that sklearn may also pick weigh 0
      float v;
      {
        int kk = 0;
        bool zero = false;
#pragma unroll
        for (int s = 0; s < KT; ++s) {
          const bool in = s < k && lq[s] < __builtin_inff();
          kk += in;
          zero = zero || (in && lq[s] == 0.f);
        }
        if (kk == 0) {
          v = col_mean[cl];                              // every donor at a NaN distance, or no donor (NaN)
        } else {
          double sw = 0.0, swx = 0.0;
#pragma unroll
          for (int s = 0; s < KT; ++s) {
            if (s < kk) {
              double w = 1.0;
              if (weights == 1) w = zero ? (lq[s] == 0.f ? 1.0 : 0.0) : 1.0 / (double)sqrtf((float)L * lq[s]);
              sw += w;
              swx += w * (double)lx[s];
            }
          }
          v = (float)(swx / sw);
        }
      }
      out[(i0 + ci) * ld_out + cl] = v;
    }
  }
}

template <int KT>
static int knn_launch(const KnnShape& sh, unsigned grid, hipStream_t st, const float* X, int n_rows, int L, int64_t ld_x,
                      const int32_t* rows, int64_t n_out, int k, int weights, const float* col_mean, float* out,
                      int64_t ld_out) {
  MMG_CHECK_HIP((MmgMaxLds<&k_knn_impute<KT>, KNN_LDS_MAX>::set()), "knn_impute(attr)");
  MMG_LAUNCH(MMG_PROBE_KNN_IMPUTE, n_out, L, k, weights, k_knn_impute<KT>, dim3(grid), dim3(KNN_THREADS), sh.lds, st,
             X, n_rows, L, ld_x, rows, n_out, k, weights, col_mean, out, ld_out, sh.T, sh.RT);
  MMG_CHECK_LAUNCH("knn_impute");
  return MMG_OK;
}

static size_t knn_ws_need(int n_cols) { return mmg_align256((size_t)n_cols * sizeof(float)); }

}  // namespace

extern "C" size_t mmg_knn_impute_ws_bytes(int64_t n_rows, int n_cols, int64_t n_out, int n_neighbors) {
  (void)n_rows;
  (void)n_out;
  (void)n_neighbors;
  return knn_ws_need(n_cols < 1 ? 1 : n_cols > 512 ? 512 : n_cols);
}

extern "C" int mmg_knn_impute(const float* X, int64_t n_rows, int n_cols, int64_t ld_x, const int32_t* rows,
                              int64_t n_out, int n_neighbors, int weights, float* out, int64_t ld_out, void* ws,
                              size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n_cols >= 1 && n_cols <= 512, "knn_impute: n_cols %d outside [1, 512]", n_cols);
  MMG_CHECK_ARG(n_neighbors >= 1 && n_neighbors <= 32, "knn_impute: n_neighbors %d outside [1, 32]", n_neighbors);
  MMG_CHECK_ARG(weights == 0 || weights == 1, "knn_impute: weights %d is neither 0 (uniform) nor 1 (distance)", weights);
  MMG_CHECK_ARG(n_rows >= 0 && n_rows < (1ll << 31), "knn_impute: n_rows %lld outside [0, 2^31)", (long long)n_rows);
  MMG_CHECK_ARG(ld_x >= n_cols, "knn_impute: ld_x %lld < n_cols %d", (long long)ld_x, n_cols);
  MMG_CHECK_ARG(ld_out >= n_cols, "knn_impute: ld_out %lld < n_cols %d", (long long)ld_out, n_cols);
  MMG_CHECK_ARG(n_out >= 0 && n_out < (1ll << 31), "knn_impute: n_out %lld outside [0, 2^31)", (long long)n_out);
  if (n_out == 0 || n_rows == 0) return MMG_OK;          // nothing requested / every requested row out of range
  MMG_CHECK_ARG(X && rows && out, "knn_impute: null buffer");
  MMG_CHECK_WS("knn_impute", knn_ws_need(n_cols));
  const KnnShape sh = knn_shape(n_cols);
  const int64_t grid = (n_out + sh.RT - 1) / sh.RT;
  float* col_mean = static_cast<float*>(ws);
  hipStream_t st = (hipStream_t)stream;
  MMG_LAUNCH(MMG_PROBE_KNN_IMPUTE, n_rows, n_cols, 0, 0, k_knn_col_mean, dim3((unsigned)n_cols), dim3(256), 0, st, X,
             n_rows, ld_x, col_mean);
  MMG_CHECK_LAUNCH("knn_impute(col_mean)");
  const int k = n_neighbors;
#define KNN_ARGS sh, (unsigned)grid, st, X, (int)n_rows, n_cols, ld_x, rows, n_out, k, weights, col_mean, out, ld_out
  if (k == 1) return knn_launch<1>(KNN_ARGS);
  if (k <= 2) return knn_launch<2>(KNN_ARGS);
  if (k <= 4) return knn_launch<4>(KNN_ARGS);
  if (k <= 8) return knn_launch<8>(KNN_ARGS);
  if (k <= 16) return knn_launch<16>(KNN_ARGS);
  return knn_launch<32>(KNN_ARGS);
#undef KNN_ARGS
}
