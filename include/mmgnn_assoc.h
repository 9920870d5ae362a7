/* C ABI of libmmgnn_assoc.so: lab co-measurement and pairwise-complete correlation (csrc/assoc.hip, mmgnn/association.py).
 * A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return codes MMG_OK /
 * MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a workspace as the three
 * parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_ASSOC_H
#define MMGNN_ASSOC_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The pairwise-complete second moments of every pair of columns ("labs") of a patient x lab matrix, and what
 * pandas.DataFrame.corr(min_periods=) / .cov(min_periods=) and the co-observation counts M^T M make of them.  The numpy
 * restatement in mmgnn/association.py is the definition; tests/assoc_ref.py restates it pair by pair.
 *
 * X is fp32 [n, ld_x], ld_x >= L, 1 <= L <= MMG_AS_MAX_LABS, 1 <= n < 2^31.  NaN means "not measured" (the contract of
 * mmg_knn_impute).  A cell that is +-inf is treated as not measured as well and counted (n_inf of mmg_assoc_colstats), so
 * a mask of 0 never multiplies an infinity.  Columns at and past L are never read.
 *
 * mmg_assoc_colstats: count (int64 [L]) the observed cells of every lab, mean (fp64 [L]) the sum of its observed values
 *   (each widened to fp64) DIVIDED once by the count -- 0 for a lab nobody has --, n_inf (int64 [1]) the infinite cells.
 *   Order of the sum: the rows are cut into slabs of R = max(MMG_AS_STAT_MIN_ROWS, ceil(n / MMG_AS_STAT_SLABS)) rows;
 *   inside a slab, phase p = 0 .. 3 adds the slab's rows p, p + 4, p + 8, .. in ascending order from 0, the four phases are
 *   added in the order 0, 1, 2, 3, and the slabs in ascending order.
 * mmg_assoc_moments: with m_ia = [X_ia observed], u_ia = m_ia * ((double)X_ia - center[a]) and q_ia = u_ia * u_ia
 *   (rounded once), out (fp64 [MMG_AS_PLANES][L][L]) holds the planes
 *     0  N[a,b]   = sum_i m_ia m_ib        1  SX[a,b]  = sum_i u_ia m_ib
 *     2  SXX[a,b] = sum_i q_ia m_ib        3  SXY[a,b] = sum_i u_ia u_ib
 *   (SY and SYY are the transposes of SX and SXX).  center (fp64 [L], device) is any finite shift; the correlation and
 *   the covariance do not depend on it, and with the column means the step SXY - SX * SY / N cancels little.
 *   The products run on v_mfma_f64_16x16x4_f64.  The L x L table is cut into MMG_AS_TILE-wide blocks; a workgroup owns one
 *   block pair (bi <= bj) and one slab of rows and keeps six accumulations: m_a m_b, u_a m_b, q_a m_b, u_a u_b, and for the
 *   lower halves of SX and SXX m_a u_b and m_a q_b, stored transposed.  N and SXY are computed for a <= b only and written
 *   to (a, b) and (b, a): exactly symmetric.  Every cell of out is written exactly once.
 *   Order of every sum: the rows are cut into the slabs of mmg_assoc_plan; a slab is walked in chunks of MMG_AS_CHUNK rows,
 *   a chunk four rows at a time, ascending, each group of four one MFMA onto the running accumulator (the order inside one
 *   instruction is the hardware's and fixed; rows past n enter as unobserved).  The partial planes of the slabs go to ws
 *   and are added in ascending slab order from 0.  All of it is a function of (n, L) alone.
 * mmg_assoc_plan: the slab plan of mmg_assoc_moments (a HOST function): rows_per_slab (a multiple of MMG_AS_CHUNK) and
 *   slabs = ceil(n / rows_per_slab).
 * mmg_assoc_finish: moments (the four planes), count (int64 [L]) -> r, cov, jaccard, lift (fp64 [L][L] each), one thread
 *   per cell.  With nab = N[a,b], SY = SX[b,a], SYY = SXX[b,a]:
 *     cxy = SXY - SX * SY / nab    vx = SXX - SX * SX / nab    vy = SYY - SY * SY / nab
 *     cov = cxy / (nab - 1);                            NaN when nab < max(min_periods, 2)
 *     r = cxy / sqrt(vx * vy), clamped to [-1, 1];      NaN when nab < max(min_periods, 1) or not vx * vy > 0
 *     jaccard = nab / (count[a] + count[b] - nab);      NaN when that is 0
 *     lift = (nab * n) / (count[a] * count[b])          (0 / 0 = NaN for a lab nobody has)
 *   every operation rounded on its own in fp64 (no fused multiply-add; division and square root correctly rounded): it
 *   EQUALS the numpy restatement on the same moments.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.
 * ------------------------------------------------------------------------------------- */
#define MMG_AS_MAX_LABS 512
#define MMG_AS_TILE 64                /* a workgroup's block of the L x L table */
#define MMG_AS_CHUNK 32               /* rows staged in LDS at a time */
#define MMG_AS_PLANES 4               /* N, SX, SXX, SXY */
#define MMG_AS_BLOCKS 512             /* workgroups the slab plan aims at */
#define MMG_AS_MIN_ROWS 256           /* the shortest slab */
#define MMG_AS_STAT_SLABS 512
#define MMG_AS_STAT_MIN_ROWS 256
int mmg_assoc_plan(int64_t n, int L, int64_t* rows_per_slab, int* slabs);
size_t mmg_assoc_colstats_ws_bytes(int64_t n, int L);                                           /* 0: unsupported shape */
int mmg_assoc_colstats(const float* X, int64_t n, int L, int64_t ld_x, int64_t* count, double* mean, int64_t* n_inf,
                       void* ws, size_t ws_bytes, void* stream);
size_t mmg_assoc_moments_ws_bytes(int64_t n, int L);                                            /* 0: unsupported shape */
int mmg_assoc_moments(const float* X, int64_t n, int L, int64_t ld_x, const double* center, double* out, void* ws,
                      size_t ws_bytes, void* stream);
size_t mmg_assoc_finish_ws_bytes(int L);                                                        /* 0: none is needed */
int mmg_assoc_finish(const double* moments, const int64_t* count, int L, int64_t n, int64_t min_periods, double* r,
                     double* cov, double* jaccard, double* lift, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_ASSOC_H */
