// Exact t-SNE of fp32 node embeddings X [n, D] (reference src/advanced_visualizations.py create_embedding_visualizations,
// which calls sklearn.manifold.TSNE; mmgnn/embed.py tsne): the O(n^2) algorithm of TSNE(method="exact") over one
// caller-owned n x n fp32 buffer A that holds the squared distances, then the joint probabilities, in place.
//   mmg_tsne_sqdist   A[i][j] = sum_d (x_id - x_jd)^2 in the difference form, fp64 from the widened fp32 inputs, rounded
//                     once to fp32; the upper triangle is computed and mirrored, the diagonal is 0.
//   mmg_tsne_joint_p  sklearn's _binary_search_perplexity per row in fp64, the conditional row rounded to fp32 over row i,
//                     then P_ij = max((C_ij + C_ji) / S, eps) in place.
//   mmg_tsne_step     one iteration of _gradient_descent on _kl_divergence in fp64: Z, then gradient (and KL), then the
//                     gains / momentum update.
//
// Reduction order (fixed by n and D alone: every output is bitwise the same from call to call and eager against a
// replayed hipGraph; no floating-point atomics, no memset node, nothing to zero):
//   distances  element (i, j): columns d ascending, one fma per column (columns past D add fma(0, 0, acc) = acc);
//   block sum  TS_NTHR threads: each thread's own terms in ascending order, an xor butterfly 32 .. 1 inside the wave
//              (a + b == b + a bit for bit: every lane holds the same sum), the four wave sums added in ascending order;
//   search     row i, one workgroup: thread t adds j = t, t + TS_NTHR, ... (j != i), then the block sum -- per step;
//   S          one partial per 64 x 64 block pair (bi <= bj): thread t adds elements t, t + TS_NTHR, ... of the block
//              (row-major), block sum, an off-diagonal block counted twice (exact); the nb * nb partials (zeros below the
//              diagonal) by thread t adding partials t, t + TS_NTHR, ..., block sum;
//   step       a workgroup owns TS_RB rows; for row i thread t adds j = 512 k + t and 512 k + 256 + t over the Y tiles
//              k = 0, 1, ... (TS_TILE = 512 points staged in LDS), block sum per row; Z and KL add the rows of a workgroup in
//              ascending order and the workgroups by thread t adding t, t + TS_NTHR, ..., block sum.
#include "common.h"
#include <math.h>

namespace {

constexpr int TS_NTHR = MMG_TSNE_SEARCH_WIDTH;      // threads of every kernel here = width of the row-search reduction
constexpr int TS_BT = 64;                          // a workgroup's block of A
constexpr int TS_DC = 32;                          // columns of X per LDS chunk
constexpr int TS_TILE = MMG_TSNE_TILE;             // points of Y per LDS tile of the step kernels
constexpr int TS_RB = 8;                           // rows of A per workgroup of the step kernels
constexpr int TS_MAX_STEPS = 100;
constexpr double TS_EPS = 2.220446049250313e-16;   // 2^-52: sklearn's MACHINE_EPSILON
constexpr double TS_TOL = 1e-5;
static_assert(TS_NTHR == 256 && TS_TILE == 2 * TS_NTHR, "the step kernels walk a tile in two strides of the block");

inline bool tsne_n_ok(int64_t n) { return n >= 4 && n <= MMG_TSNE_MAX_N; }

// the sum over the block in the fixed order of the header; every thread returns it.  red: TS_NTHR / 64 doubles
__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum_d(v);
  __syncthreads();                                   // the previous use of red has been read
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}
// sum of cnt doubles: thread t adds t, t + TS_NTHR, ...
__device__ __forceinline__ double strided_sum(const double* __restrict__ p, int cnt, double* red) {
  double s = 0.0;
  for (int q = threadIdx.x; q < cnt; q += TS_NTHR) s += p[q];
  return block_sum(s, red);
}

// ---- squared distances: grid (nb, nb), the blocks below the diagonal leave at once
__global__ __launch_bounds__(TS_NTHR) void k_tsne_sqdist(const float* __restrict__ X, int n, int D, int64_t ld_x,
                                                         float* __restrict__ A, int64_t ld_a) {
  __shared__ double xi[TS_DC][TS_BT + 1];
  __shared__ double xj[TS_DC][TS_BT + 1];
  const int bj = (int)blockIdx.x, bi = (int)blockIdx.y;
  if (bi > bj) return;                               // block-uniform
  const bool diag = bi == bj;
  const int i0 = bi * TS_BT, j0 = bj * TS_BT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  double acc[4][4];
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[p][q] = 0.0;
  const double(*xb)[TS_BT + 1] = diag ? xi : xj;
  for (int d0 = 0; d0 < D; d0 += TS_DC) {
    __syncthreads();                                 // the previous chunk has been consumed
    for (int e = tid; e < TS_BT * TS_DC; e += TS_NTHR) {
      const int r = e / TS_DC, c = e % TS_DC;
      const bool col = d0 + c < D;
      const int ri = i0 + r, rj = j0 + r;
      xi[c][r] = (col && ri < n) ? (double)X[(int64_t)ri * ld_x + d0 + c] : 0.0;
      if (!diag) xj[c][r] = (col && rj < n) ? (double)X[(int64_t)rj * ld_x + d0 + c] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int c = 0; c < TS_DC; ++c) {
      double a[4], b[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) { a[p] = xi[c][4 * ty + p]; b[p] = xb[c][4 * tx + p]; }
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const double df = a[p] - b[q];
          acc[p][q] = fma(df, df, acc[p][q]);
        }
    }
  }
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int i = i0 + 4 * ty + p;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = j0 + 4 * tx + q;
      if (i >= n || j >= n) continue;
      if (i < j) {
        const float v = (float)acc[p][q];
        A[(int64_t)i * ld_a + j] = v;
        A[(int64_t)j * ld_a + i] = v;
      } else if (i == j) {
        A[(int64_t)i * ld_a + i] = 0.f;
      }
    }
  }
}

// ---- the perplexity search: one workgroup per row
__global__ __launch_bounds__(TS_NTHR) void k_tsne_search(float* __restrict__ A, int n, int64_t ld_a, double log_perp,
                                                         double* __restrict__ beta_out, int32_t* __restrict__ steps_out) {
  __shared__ double red[TS_NTHR / 64];
  const int i = (int)blockIdx.x, tid = threadIdx.x;
  float* __restrict__ row = A + (int64_t)i * ld_a;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, s = 0.0;
  int steps = 0;
  for (;;) {                                         // every decision below is block-uniform
    double sp = 0.0, sdp = 0.0;
    for (int j = tid; j < n; j += TS_NTHR) {
      if (j == i) continue;
      const double d = (double)row[j];
      const double p = exp(-beta * d);
      sp += p;
      sdp += d * p;
    }
    sp = block_sum(sp, red);
    sdp = block_sum(sdp, red);
    s = sp == 0.0 ? 1e-8 : sp;
    const double diff = log(s) + beta * sdp / s - log_perp;
    ++steps;
    if (fabs(diff) <= TS_TOL || steps == TS_MAX_STEPS) break;
    if (diff > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  // a thread reads the distances it overwrites: no other thread touches them
  for (int j = tid; j < n; j += TS_NTHR) {
    const double d = (double)row[j];
    row[j] = j == i ? 0.f : (float)(exp(-beta * d) / s);
  }
  if (tid == 0) { beta_out[i] = beta; steps_out[i] = steps; }
}

// ---- C -> P in place.  WRITE = false: the block pair's part of S; WRITE = true: P from S.  Grid (nb, nb).
template <bool WRITE>
__global__ __launch_bounds__(TS_NTHR) void k_tsne_sym(float* __restrict__ A, int n, int64_t ld_a, int nb,
                                                      double* __restrict__ partial, const double* __restrict__ S) {
  __shared__ float t1[TS_BT][TS_BT + 1];
  __shared__ float t2[TS_BT][TS_BT + 1];
  __shared__ double red[TS_NTHR / 64];
  const int bj = (int)blockIdx.x, bi = (int)blockIdx.y, tid = threadIdx.x;
  if (bi > bj) {                                     // block-uniform
    if (!WRITE && tid == 0) partial[bi * nb + bj] = 0.0;
    return;
  }
  const bool diag = bi == bj;
  const int i0 = bi * TS_BT, j0 = bj * TS_BT;
  for (int e = tid; e < TS_BT * TS_BT; e += TS_NTHR) {
    const int r = e / TS_BT, c = e % TS_BT;
    t1[r][c] = (i0 + r < n && j0 + c < n) ? A[(int64_t)(i0 + r) * ld_a + j0 + c] : 0.f;
    if (!diag) t2[r][c] = (j0 + r < n && i0 + c < n) ? A[(int64_t)(j0 + r) * ld_a + i0 + c] : 0.f;
  }
  __syncthreads();                                   // both blocks are in LDS before either is overwritten
  const float(*u)[TS_BT + 1] = diag ? t1 : t2;
  if (!WRITE) {
    double acc = 0.0;
    for (int e = tid; e < TS_BT * TS_BT; e += TS_NTHR) {
      const int r = e / TS_BT, c = e % TS_BT;
      acc += (double)(t1[r][c] + u[c][r]);           // the sum in fp32, as sklearn has it
    }
    acc = block_sum(acc, red);
    if (tid == 0) partial[bi * nb + bj] = diag ? acc : 2.0 * acc;
  } else {
    const double sm = fmax(S[0], TS_EPS);
    for (int e = tid; e < TS_BT * TS_BT; e += TS_NTHR) {
      const int r = e / TS_BT, c = e % TS_BT;
      if (i0 + r < n && j0 + c < n) {
        const float v = (float)fmax((double)(t1[r][c] + u[c][r]) / sm, TS_EPS);
        A[(int64_t)(i0 + r) * ld_a + j0 + c] = (i0 + r == j0 + c) ? 0.f : v;
      }
      if (!diag && j0 + r < n && i0 + c < n)         // the mirrored block: c_ji + c_ij, the same sum bit for bit
        A[(int64_t)(j0 + r) * ld_a + i0 + c] = (float)fmax((double)(t2[r][c] + t1[c][r]) / sm, TS_EPS);
    }
  }
}

__global__ __launch_bounds__(TS_NTHR) void k_tsne_sum(const double* __restrict__ partial, int cnt, double* __restrict__ out) {
  __shared__ double red[TS_NTHR / 64];
  const double s = strided_sum(partial, cnt, red);
  if (threadIdx.x == 0) out[0] = s;
}

// ---- one iteration.  The two passes over the pairs share the walk: TS_RB rows per workgroup, Y in tiles of TS_TILE.
// GRAD = false: zblk[workgroup] = sum over its rows of sum_{j != i} num_ij.
// GRAD = true:  grad[i] = 4 sum_j (Pe_ij - Q_ij) num_ij (y_i - y_j), klblk[workgroup] = its part of KL (want_kl).
template <bool GRAD>
__global__ __launch_bounds__(TS_NTHR) void k_tsne_pairs(const float* __restrict__ A, int n, int64_t ld_a,
                                                        double exaggeration, const double* __restrict__ Y, int nblk,
                                                        double* __restrict__ zblk, double* __restrict__ klblk,
                                                        double* __restrict__ grad, double* __restrict__ grad_out,
                                                        int want_kl) {
#pragma clang fp contract(off)                       // every term is rounded as numpy rounds it: only the ORDER of a sum differs
  __shared__ double2 ys[TS_TILE];
  __shared__ double red[TS_NTHR / 64];
  const int tid = threadIdx.x, i0 = (int)blockIdx.x * TS_RB;
  double Z = 1.0;
  if (GRAD) Z = strided_sum(zblk, nblk, red);
  double yix[TS_RB], yiy[TS_RB], ax[TS_RB], ay[TS_RB], ak[TS_RB];
#pragma unroll
  for (int r = 0; r < TS_RB; ++r) {
    const bool live = i0 + r < n;
    yix[r] = live ? Y[2 * (i0 + r)] : 0.0;
    yiy[r] = live ? Y[2 * (i0 + r) + 1] : 0.0;
    ax[r] = 0.0; ay[r] = 0.0; ak[r] = 0.0;
  }
  for (int t0 = 0; t0 < n; t0 += TS_TILE) {
    __syncthreads();                                 // the previous tile has been consumed
#pragma unroll
    for (int h = 0; h < TS_TILE / TS_NTHR; ++h) {
      const int e = tid + h * TS_NTHR, j = t0 + e;
      ys[e] = j < n ? double2{Y[2 * j], Y[2 * j + 1]} : double2{0.0, 0.0};
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < TS_TILE / TS_NTHR; ++h) {
      const int e = tid + h * TS_NTHR, j = t0 + e;
      if (j >= n) continue;
      const double2 yj = ys[e];
#pragma unroll
      for (int r = 0; r < TS_RB; ++r) {
        const int i = i0 + r;
        if (i >= n || i == j) continue;
        const double dx = yix[r] - yj.x, dy = yiy[r] - yj.y;
        const double num = 1.0 / (1.0 + (dx * dx + dy * dy));
        if (!GRAD) {
          ax[r] += num;
        } else {
          const double pe = exaggeration * (double)A[(int64_t)i * ld_a + j];
          const double q = fmax(num / Z, TS_EPS);
          const double w = (pe - q) * num;
          ax[r] += w * dx;
          ay[r] += w * dy;
          if (want_kl) ak[r] += pe * log(fmax(pe, TS_EPS) / q);
        }
      }
    }
  }
  double zsum = 0.0, ksum = 0.0;
#pragma unroll
  for (int r = 0; r < TS_RB; ++r) {                  // the reductions are block-uniform: rows past n add zeros
    const double sx = block_sum(ax[r], red);
    if (!GRAD) {
      zsum += sx;
    } else {
      const double sy = block_sum(ay[r], red);
      if (want_kl) ksum += block_sum(ak[r], red);
      if (tid == 0 && i0 + r < n) {
        const double gx = 4.0 * sx, gy = 4.0 * sy;
        grad[2 * (i0 + r)] = gx;
        grad[2 * (i0 + r) + 1] = gy;
        if (grad_out) { grad_out[2 * (i0 + r)] = gx; grad_out[2 * (i0 + r) + 1] = gy; }
      }
    }
  }
  if (tid == 0) {
    if (!GRAD) zblk[blockIdx.x] = zsum;
    else if (want_kl) klblk[blockIdx.x] = ksum;
  }
}

// the gains / momentum update of _gradient_descent and the three statistics: one workgroup.  No fused multiply-add
// here: every product and sum is rounded on its own, as numpy does, so the update is bit-equal to the host's.
__global__ __launch_bounds__(TS_NTHR) void k_tsne_update(int n, int nblk, const double* __restrict__ zblk,
                                                         const double* __restrict__ klblk, const double* __restrict__ grad,
                                                         double* __restrict__ Y, double* __restrict__ U, double* __restrict__ G,
                                                         double momentum, double learning_rate, double min_gain, int want_kl,
                                                         int update, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double red[TS_NTHR / 64];
  const double Z = strided_sum(zblk, nblk, red);
  const double kl = want_kl ? strided_sum(klblk, nblk, red) : (double)NAN;
  double g2 = 0.0;
  for (int e = threadIdx.x; e < 2 * n; e += TS_NTHR) {
    const double g = grad[e], u = U[e];
    double gain = G[e];
    gain = (u * g < 0.0) ? gain + 0.2 : gain * 0.8;
    gain = fmax(gain, min_gain);
    const double gg = g * gain;
    g2 += gg * gg;
    if (update) {
      const double a = momentum * u, b = learning_rate * gg;
      const double un = a - b;
      G[e] = gain;
      U[e] = un;
      Y[e] = Y[e] + un;
    }
  }
  g2 = block_sum(g2, red);
  if (threadIdx.x == 0) { stats[0] = kl; stats[1] = g2; stats[2] = Z; }
}

struct JointWs { double *partial, *S; };
size_t joint_carve(void* ws, int64_t n, JointWs* w) {
  const size_t nb = (size_t)((n + TS_BT - 1) / TS_BT);
  MmgCarver c(ws);
  *w = JointWs{c.take<double>(nb * nb), c.take<double>(1)};
  return c.need();
}
struct StepWs { double *zblk, *klblk, *grad; };
size_t step_carve(void* ws, int64_t n, StepWs* w) {
  const size_t nblk = (size_t)((n + TS_RB - 1) / TS_RB);
  MmgCarver c(ws);
  *w = StepWs{c.take<double>(nblk), c.take<double>(nblk), c.take<double>(2 * (size_t)n)};
  return c.need();
}

}  // namespace

// the distances keep nothing between kernels: no workspace today (ws may be null)
extern "C" size_t mmg_tsne_sqdist_ws_bytes(int64_t n, int D) { return 0; }

extern "C" int mmg_tsne_sqdist(const float* X, int64_t n, int D, int64_t ld_x, float* A, int64_t ld_a, void* ws,
                               size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(tsne_n_ok(n), "tsne_sqdist: n %lld outside [4, %d]", (long long)n, MMG_TSNE_MAX_N);
  MMG_CHECK_ARG(D >= 4 && D <= 256 && (D & 3) == 0, "tsne_sqdist: D %d is not a multiple of 4 in [4, 256]", D);
  MMG_CHECK_ARG(ld_x >= D, "tsne_sqdist: ld_x %lld < D %d", (long long)ld_x, D);
  MMG_CHECK_ARG(ld_a >= n, "tsne_sqdist: ld_a %lld < n %lld", (long long)ld_a, (long long)n);
  MMG_CHECK_ARG(X && A, "tsne_sqdist: null pointer (X, A)");
  const unsigned nb = (unsigned)((n + TS_BT - 1) / TS_BT);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, D, 0, 0, k_tsne_sqdist, dim3(nb, nb), dim3(TS_NTHR), 0, (hipStream_t)stream, X, (int)n,
             D, ld_x, A, ld_a);
  MMG_CHECK_LAUNCH("tsne_sqdist");
  return MMG_OK;
}

extern "C" size_t mmg_tsne_joint_p_ws_bytes(int64_t n) {
  if (!tsne_n_ok(n)) return 0;
  JointWs w;
  return joint_carve(nullptr, n, &w);
}

extern "C" int mmg_tsne_joint_p(float* A, int64_t n, int64_t ld_a, double perplexity, double* beta_out, int32_t* steps_out,
                                void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(tsne_n_ok(n), "tsne_joint_p: n %lld outside [4, %d]", (long long)n, MMG_TSNE_MAX_N);
  MMG_CHECK_ARG(ld_a >= n, "tsne_joint_p: ld_a %lld < n %lld", (long long)ld_a, (long long)n);
  MMG_CHECK_ARG(perplexity > 0.0 && perplexity < (double)n, "tsne_joint_p: perplexity %g outside (0, n = %lld)", perplexity,
                (long long)n);
  MMG_CHECK_ARG(A && beta_out && steps_out, "tsne_joint_p: null pointer (A, beta_out, steps_out)");
  JointWs w;
  MMG_CHECK_WS("tsne_joint_p", joint_carve(ws, n, &w));
  hipStream_t st = (hipStream_t)stream;
  const unsigned nb = (unsigned)((n + TS_BT - 1) / TS_BT);
  const dim3 blk(TS_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_tsne_search, dim3((unsigned)n), blk, 0, st, A, (int)n, ld_a, log(perplexity),
             beta_out, steps_out);
  MMG_CHECK_LAUNCH("tsne_joint_p(search)");
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_tsne_sym<false>, dim3(nb, nb), blk, 0, st, A, (int)n, ld_a, (int)nb, w.partial,
             (const double*)w.S);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, nb * nb, 0, 0, 0, k_tsne_sum, dim3(1), blk, 0, st, (const double*)w.partial, (int)(nb * nb),
             w.S);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 1, k_tsne_sym<true>, dim3(nb, nb), blk, 0, st, A, (int)n, ld_a, (int)nb, w.partial,
             (const double*)w.S);
  MMG_CHECK_LAUNCH("tsne_joint_p(joint)");
  return MMG_OK;
}

extern "C" size_t mmg_tsne_step_ws_bytes(int64_t n) {
  if (!tsne_n_ok(n)) return 0;
  StepWs w;
  return step_carve(nullptr, n, &w);
}

extern "C" int mmg_tsne_step(const float* A, int64_t n, int64_t ld_a, double exaggeration, double* Y, double* U, double* G,
                             double momentum, double learning_rate, double min_gain, int want_kl, double* stats_out,
                             double* grad_out, int update, void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(tsne_n_ok(n), "tsne_step: n %lld outside [4, %d]", (long long)n, MMG_TSNE_MAX_N);
  MMG_CHECK_ARG(ld_a >= n, "tsne_step: ld_a %lld < n %lld", (long long)ld_a, (long long)n);
  MMG_CHECK_ARG(A && Y && U && G && stats_out, "tsne_step: null pointer (A, Y, U, G, stats_out)");
  StepWs w;
  MMG_CHECK_WS("tsne_step", step_carve(ws, n, &w));
  hipStream_t st = (hipStream_t)stream;
  const int nblk = (int)((n + TS_RB - 1) / TS_RB);
  const dim3 blk(TS_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_tsne_pairs<false>, dim3((unsigned)nblk), blk, 0, st, A, (int)n, ld_a,
             exaggeration, (const double*)Y, nblk, w.zblk, w.klblk, w.grad, grad_out, 0);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 1, k_tsne_pairs<true>, dim3((unsigned)nblk), blk, 0, st, A, (int)n, ld_a,
             exaggeration, (const double*)Y, nblk, w.zblk, w.klblk, w.grad, grad_out, want_kl ? 1 : 0);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 2, k_tsne_update, dim3(1), blk, 0, st, (int)n, nblk, (const double*)w.zblk,
             (const double*)w.klblk, (const double*)w.grad, Y, U, G, momentum, learning_rate, min_gain, want_kl ? 1 : 0,
             update ? 1 : 0, stats_out);
  MMG_CHECK_LAUNCH("tsne_step");
  return MMG_OK;
}
