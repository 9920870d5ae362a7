// Embedding maps (reference src/advanced_visualizations.py create_embedding_visualizations, src/visualize.py
// plot_embeddings_umap with visualization.dim_reduction = "pca"; mmgnn/embed.py): the arithmetic over all rows of a
// PCA of fp32 node embeddings X [n, D] and of the 2-D density grid of the projected patients.
//   mmg_centered_gram  column means in fp64, then S = sum_i (x_i - mu)(x_i - mu)^T: centred in fp64 from the fp32 input
//                      (two passes, never X^T X - n mu mu^T), products and sums in fp64 on v_mfma_f64_16x16x4_f64.
//   mmg_project_rows   out[i, c] = scale[c] * sum_d (x_id - mu_d) comps[c, d], fp64 sum rounded once to fp32.
//   mmg_grid2d         numpy.histogram2d with explicit float64 edges: int64 count and integer weight sum per cell.
//
// Reduction order (fixed by n and D alone, so every output is bitwise the same from call to call and eager against a
// replayed hipGraph; no floating-point atomics anywhere):
//   means  the rows are cut into slabs of pca_plan().mean_rows rows; in a slab thread (rr, col) adds rows rr, rr + nr, ...
//          (nr = 256 / D) in ascending order, the nr partials are added in ascending rr, the slabs in ascending order,
//          and the sum is DIVIDED by n (one rounding, as numpy's mean);
//   Gram   the rows are cut into slabs of pca_plan().gram_rows rows (a multiple of 32); a workgroup owns one 64 x 64
//          block of S of the upper block triangle and one slab, walks the slab in chunks of 32 rows (centred to fp64 in
//          LDS, rows past the end and columns past D are zeros) and feeds them four rows at a time, ascending, to the
//          MFMA; each wave owns a 16 x 64 strip (four 16 x 16 accumulators), of a diagonal block only the tiles on and
//          above the diagonal.  The slabs of an element are added in ascending order; element (a, b), a <= b, is
//          written to both (a, b) and (b, a): S is exactly symmetric.
//   rows   16 lanes per row: lane s adds columns s, s + 16, ... in ascending order by fma, then an xor butterfly 8, 4,
//          2, 1 (a + b == b + a bit for bit: every lane holds the same sum).
// The Gram kernel is the walk of gram64.h, which also explains the f64 MFMA's C/D layout.
#include "common.h"
#include "gram64.h"

namespace {

constexpr int PCA_NTHR = GRAM64_NTHR;
constexpr int PCA_MAX_D = 256;
constexpr int PCA_MAX_K = 8;
constexpr int PCA_MAX_GRID = 256;
constexpr int PCA_MEAN_SLABS = 512;
constexpr int PCA_MEAN_MIN_ROWS = 256;
constexpr int PCA_GRAM_BLOCKS = 768;         // workgroups aimed at: about three per CU
constexpr int PCA_GRAM_MIN_ROWS = 64;

struct PcaPlan {
  int64_t mean_rows, gram_rows;
  int mean_slabs, gram_slabs, nb, pairs;
};
inline PcaPlan pca_plan(int64_t n, int D) {
  PcaPlan p;
  p.mean_rows = (n + PCA_MEAN_SLABS - 1) / PCA_MEAN_SLABS;
  if (p.mean_rows < PCA_MEAN_MIN_ROWS) p.mean_rows = PCA_MEAN_MIN_ROWS;
  p.mean_slabs = (int)((n + p.mean_rows - 1) / p.mean_rows);
  const Gram64Plan g = gram64_plan(n, D, PCA_GRAM_BLOCKS, PCA_GRAM_MIN_ROWS);           // pairs <= 10
  p.gram_rows = g.rows;
  p.gram_slabs = g.slabs;
  p.nb = g.nb;
  p.pairs = g.pairs;
  return p;
}
inline bool pca_shape_ok(int64_t n, int D) {
  return n >= 2 && n < INT32_MAX && D >= 4 && D <= PCA_MAX_D && (D & 3) == 0;
}

// ---- means
__global__ __launch_bounds__(PCA_NTHR) void k_pca_colsum(const float* __restrict__ X, int64_t n, int D, int64_t ld,
                                                         int64_t rows_per_slab, double* __restrict__ partial) {
  __shared__ double part[PCA_NTHR];
  const int tid = threadIdx.x, nr = PCA_NTHR / D;               // nr >= 1
  const int col = tid % D, rr = tid / D;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
  double s = 0.0;
  if (rr < nr) {
    const float* __restrict__ xc = X + col;
    int64_t r = r0 + rr;
    for (; r + 3 * (int64_t)nr < r1; r += 4 * (int64_t)nr) {    // four loads in flight, added in row order
      const float v0 = xc[r * ld], v1 = xc[(r + nr) * ld], v2 = xc[(r + 2 * nr) * ld], v3 = xc[(r + 3 * nr) * ld];
      s += (double)v0; s += (double)v1; s += (double)v2; s += (double)v3;
    }
    for (; r < r1; r += nr) s += (double)xc[r * ld];
  }
  part[tid] = s;
  __syncthreads();
  if (tid < D) {
    double t = part[tid];
    for (int q = 1; q < nr; ++q) t += part[q * D + tid];
    partial[(size_t)blockIdx.x * D + tid] = t;
  }
}

__global__ __launch_bounds__(PCA_NTHR) void k_pca_mean(const double* __restrict__ partial, int slabs, int D, int64_t n,
                                                       double* __restrict__ mean) {
  const int c = threadIdx.x;
  if (c >= D) return;
  double s = 0.0;
  for (int q = 0; q < slabs; ++q) s += partial[(size_t)q * D + c];
  mean[c] = s / (double)n;
}

// ---- Gram: grid (block pairs of the upper triangle, slabs), the walk of gram64.h.  Staged: x - mean, zeros for the rows
// past the end and the columns past D; one product per tile.
struct PcaAcc {
  gram64_d4 acc[4] = {};
  double av;
  __device__ __forceinline__ void row(double a, bool) { av = a; }
  __device__ __forceinline__ void tile(int j, double bv, bool) {
    acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[j], 0, 0, 0);
  }
};

__global__ __launch_bounds__(PCA_NTHR) void k_pca_gram(const float* __restrict__ X, int64_t n, int D, int64_t ld,
                                                       const double* __restrict__ mean, int64_t rows_per_slab, int nb,
                                                       double* __restrict__ partial) {
  __shared__ double As[GRAM64_SIDE], Bs[GRAM64_SIDE];
  const Gram64Tile t(nb, D, n, rows_per_slab);
  const double mua = t.a_in ? mean[t.ca] : 0.0, mub = t.b_in ? mean[t.cb] : 0.0;
  PcaAcc acc;
  gram64_walk(t, D, As, Bs, acc, [=](int64_t r, bool live, double& a, double& b) {
    a = (live && t.a_in) ? (double)X[r * ld + t.ca] - mua : 0.0;
    if (!t.diag) b = (live && t.b_in) ? (double)X[r * ld + t.cb] - mub : 0.0;
  });
  double* __restrict__ out = partial + (size_t)blockIdx.y * (size_t)D * (size_t)D;
  gram64_store_tiles(t, D, [&](int j, bool) { gram64_put(t, D, j, acc.acc[j], out); });
}

__global__ __launch_bounds__(PCA_NTHR) void k_pca_gram_sum(const double* __restrict__ partial, int slabs, int D,
                                                           double* __restrict__ gram) {
  const int idx = (int)blockIdx.x * PCA_NTHR + threadIdx.x;
  if (idx < D * D) gram64_sum_cell<4>(partial, (size_t)D * D, slabs, D, idx, true, gram);
}

// ---- projection: 16 lanes per row, 16 rows per workgroup pass
__global__ __launch_bounds__(PCA_NTHR) void k_pca_project(const float* __restrict__ X, int64_t n, int D, int64_t ld,
                                                          const double* __restrict__ mean,
                                                          const double* __restrict__ comps,
                                                          const double* __restrict__ scale, int k,
                                                          float* __restrict__ out, int64_t ld_out) {
  __shared__ double smean[PCA_MAX_D];
  __shared__ double scomp[PCA_MAX_K * PCA_MAX_D];
  const int tid = threadIdx.x;
  for (int i = tid; i < D; i += PCA_NTHR) smean[i] = mean[i];
  for (int i = tid; i < k * D; i += PCA_NTHR) scomp[i] = comps[i];
  __syncthreads();
  const int sub = tid & 15, rloc = tid >> 4;
  const double sc = (scale && sub < k) ? scale[sub] : 1.0;
  const int64_t step = (int64_t)gridDim.x * 16;
  const int64_t passes = (n + step - 1) / step;                 // the same for every lane: the shuffles stay converged
  for (int64_t ps = 0; ps < passes; ++ps) {
    const int64_t r = ps * step + (int64_t)blockIdx.x * 16 + rloc;
    const bool live = r < n;
    double acc[PCA_MAX_K];
#pragma unroll
    for (int c = 0; c < PCA_MAX_K; ++c) acc[c] = 0.0;
    if (live) {
      const float* __restrict__ xr = X + r * ld;
      for (int d = sub; d < D; d += 16) {
        const double xc = (double)xr[d] - smean[d];
#pragma unroll
        for (int c = 0; c < PCA_MAX_K; ++c)
          if (c < k) acc[c] = fma(xc, scomp[c * D + d], acc[c]);
      }
    }
    double mine = 0.0;
#pragma unroll
    for (int c = 0; c < PCA_MAX_K; ++c) {
      if (c < k) {
        double v = acc[c];
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 16);
        if (sub == c) mine = v;
      }
    }
    if (live && sub < k) out[r * ld_out + sub] = (float)(sc * mine);
  }
}

// ---- 2-D histogram
// numpy.histogram2d's bin of v over the g + 1 ascending edges e: [e_j, e_j+1), the last edge inclusive; -1 = not counted
__device__ __forceinline__ int pca_bin(const double* e, int g, double v) {
  if (!(v >= e[0]) || !(v <= e[g])) return -1;                  // outside, or NaN
  if (v == e[g]) return g - 1;
  int lo = 0, hi = g + 1;                                       // the number of edges <= v, in [1, g]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (e[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo <= g ? lo - 1 : -1;                                  // (edges out of order: never a cell past the grid)
}

__global__ __launch_bounds__(PCA_NTHR) void k_pca_grid2d(const float* __restrict__ Y, int64_t ld,
                                                         const int32_t* __restrict__ w, int64_t n,
                                                         const double* __restrict__ ex, const double* __restrict__ ey,
                                                         int gx, int gy, unsigned long long* __restrict__ count,
                                                         unsigned long long* __restrict__ wsum) {
  __shared__ double sx[PCA_MAX_GRID + 1];
  __shared__ double sy[PCA_MAX_GRID + 1];
  for (int i = threadIdx.x; i <= gx; i += PCA_NTHR) sx[i] = ex[i];
  for (int i = threadIdx.x; i <= gy; i += PCA_NTHR) sy[i] = ey[i];
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * PCA_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * PCA_NTHR + threadIdx.x; i < n; i += step) {
    const int bx = pca_bin(sx, gx, (double)Y[i * ld]);
    const int by = pca_bin(sy, gy, (double)Y[i * ld + 1]);
    if (bx < 0 || by < 0) continue;
    const int cell = bx * gy + by;                              // < gx * gy
    atomicAdd(&count[cell], 1ull);                              // integer: the result does not depend on the order
    if (w) atomicAdd(&wsum[cell], (unsigned long long)(long long)w[i]);
  }
}

struct GramWs {
  double *mean_partial, *gram_partial;
};
size_t gram_carve(void* ws, int64_t n, int D, GramWs* w) {
  const PcaPlan p = pca_plan(n, D);
  MmgCarver c(ws);
  *w = GramWs{c.take<double>((size_t)p.mean_slabs * D), c.take<double>((size_t)p.gram_slabs * D * D)};
  return c.need();
}

}  // namespace

extern "C" size_t mmg_centered_gram_ws_bytes(int64_t n, int D) {
  if (!pca_shape_ok(n, D)) return 0;
  GramWs w;
  return gram_carve(nullptr, n, D, &w);
}

extern "C" int mmg_centered_gram(const float* X, int64_t n, int D, int64_t ld_x, double* mean_out, double* gram_out,
                                 void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 2 && n < INT32_MAX, "centered_gram: n %lld outside [2, 2^31)", (long long)n);
  MMG_CHECK_ARG(D >= 4 && D <= PCA_MAX_D && (D & 3) == 0, "centered_gram: D %d is not a multiple of 4 in [4, %d]", D,
                PCA_MAX_D);
  MMG_CHECK_ARG(ld_x >= D, "centered_gram: ld_x %lld < D %d", (long long)ld_x, D);
  MMG_CHECK_ARG(X && mean_out && gram_out, "centered_gram: null pointer (X, mean_out, gram_out)");
  GramWs w;
  MMG_CHECK_WS("centered_gram", gram_carve(ws, n, D, &w));
  const PcaPlan p = pca_plan(n, D);
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(PCA_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, 0, 0, k_pca_colsum, dim3((unsigned)p.mean_slabs), blk, 0, st, X, n, D, ld_x,
             p.mean_rows, w.mean_partial);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.mean_slabs, D, 0, 0, k_pca_mean, dim3(1), blk, 0, st, w.mean_partial, p.mean_slabs, D,
             n, mean_out);
  MMG_CHECK_LAUNCH("centered_gram(means)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, D, 0, k_pca_gram, dim3((unsigned)p.pairs, (unsigned)p.gram_slabs), blk, 0, st, X,
             n, D, ld_x, mean_out, p.gram_rows, p.nb, w.gram_partial);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, p.gram_slabs, D, D, 0, k_pca_gram_sum, dim3((unsigned)((D * D + PCA_NTHR - 1) / PCA_NTHR)),
             blk, 0, st, w.gram_partial, p.gram_slabs, D, gram_out);
  MMG_CHECK_LAUNCH("centered_gram(gram)");
  return MMG_OK;
}

// the projection and the grid keep nothing between their kernels: no workspace today (ws may be null)
extern "C" size_t mmg_project_rows_ws_bytes(int64_t n, int D, int k) { return 0; }

extern "C" int mmg_project_rows(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* comps,
                                const double* scale, int k, float* out, int64_t ld_out, void* ws, size_t ws_bytes,
                                void* stream) {
  MMG_CHECK_ARG(n >= 1 && n < INT32_MAX, "project_rows: n %lld outside [1, 2^31)", (long long)n);
  MMG_CHECK_ARG(D >= 4 && D <= PCA_MAX_D && (D & 3) == 0, "project_rows: D %d is not a multiple of 4 in [4, %d]", D,
                PCA_MAX_D);
  MMG_CHECK_ARG(k >= 1 && k <= PCA_MAX_K, "project_rows: k %d outside [1, %d]", k, PCA_MAX_K);
  MMG_CHECK_ARG(ld_x >= D, "project_rows: ld_x %lld < D %d", (long long)ld_x, D);
  MMG_CHECK_ARG(ld_out >= k, "project_rows: ld_out %lld < k %d", (long long)ld_out, k);
  MMG_CHECK_ARG(X && mean && comps && out, "project_rows: null pointer (X, mean, comps, out)");
  int64_t g = (n + 15) / 16;
  if (g > 4096) g = 4096;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, k, 0, k_pca_project, dim3((unsigned)g), dim3(PCA_NTHR), 0, (hipStream_t)stream, X,
             n, D, ld_x, mean, comps, scale, k, out, ld_out);
  MMG_CHECK_LAUNCH("project_rows");
  return MMG_OK;
}

extern "C" size_t mmg_grid2d_ws_bytes(int64_t n, int gx, int gy) { return 0; }

extern "C" int mmg_grid2d(const float* Y, int64_t ld_y, const int32_t* w, int64_t n, const double* ex, const double* ey,
                          int gx, int gy, int64_t* count, int64_t* wsum, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 0 && n < INT32_MAX, "grid2d: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(gx >= 1 && gx <= PCA_MAX_GRID && gy >= 1 && gy <= PCA_MAX_GRID, "grid2d: grid %d x %d outside [1, %d]", gx,
                gy, PCA_MAX_GRID);
  MMG_CHECK_ARG(ld_y >= 2, "grid2d: ld_y %lld < 2", (long long)ld_y);
  MMG_CHECK_ARG(ex && ey && count, "grid2d: null pointer (ex, ey, count)");
  MMG_CHECK_ARG(n == 0 || Y, "grid2d: Y is null");
  MMG_CHECK_ARG(!w || wsum, "grid2d: weights without wsum");
  hipStream_t st = (hipStream_t)stream;
  const size_t cells = (size_t)gx * gy;
  MMG_CHECK_HIP(mmg_zero_async(count, cells * sizeof(int64_t), st), "grid2d(zero)");
  if (wsum) MMG_CHECK_HIP(mmg_zero_async(wsum, cells * sizeof(int64_t), st), "grid2d(zero)");
  if (n == 0) return MMG_OK;
  int64_t g = (n + PCA_NTHR - 1) / PCA_NTHR;
  if (g > 2048) g = 2048;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, gx, gy, 0, k_pca_grid2d, dim3((unsigned)g), dim3(PCA_NTHR), 0, st, Y, ld_y, w, n, ex,
             ey, gx, gy, (unsigned long long*)count, (unsigned long long*)wsum);
  MMG_CHECK_LAUNCH("grid2d");
  return MMG_OK;
}
