/* C ABI of libmmgnn_chain.so: lab imputation by chained equations (csrc/chain.hip, mmgnn/chained.py).
 * A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return codes MMG_OK /
 * MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a workspace as the three
 * parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_CHAIN_H
#define MMGNN_CHAIN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Multivariate imputation by chained equations with a ridge regression per lab: what
 * sklearn.impute.IterativeImputer(estimator=Ridge(alpha), skip_complete=False) computes.  The numpy restatement in
 * mmgnn/chained.py is the definition; tests/chain_ref.py restates it in loops and 80-bit arithmetic.
 *
 * X is fp32 [n, ld_x], ld_x >= L, 1 <= L <= MMG_CH_MAX_LABS, 1 <= n < 2^31; NaN means "not measured" (the contract of
 * mmg_knn_impute; a cell that is +-inf is refused in Python and enters here as not measured).  Columns at and past L
 * are never read.  W is the fp64 working matrix [n, L], rows contiguous.  count (int64 [L]) and center (fp64 [L]) are
 * the outputs of mmg_assoc_colstats; a lab with count 0 is INACTIVE: never a target, never a predictor.  0 <= j < L is
 * the target lab of a step, S_j the rows whose X_ij is observed.
 *
 * mmg_chain_plan: the slab plan of mmg_chain_moments (a HOST function): rows_per_slab (a multiple of MMG_CH_CHUNK) and
 *   slabs = ceil(n / rows_per_slab), a function of (n, L) alone.
 * mmg_chain_init: W_ia = X_ia observed ? (double)X_ia : center[a].
 * mmg_chain_moments: with u_ia = W_ia - center[a] (rounded once) over the rows i of S_j
 *     n_j (int64 [1]) = |S_j|      s (fp64 [L]): s_a = sum_i u_ia      G (fp64 [L][L]): G_ab = sum_i u_ia u_ib
 *   The mask is one bit per ROW: a row outside S_j or past n enters as zeros.  The products run on
 *   v_mfma_f64_16x16x4_f64 (s as the product with a column of ones).  The L x L table is cut into MMG_CH_TILE-wide
 *   blocks; a workgroup owns one block pair (bi <= bj) and one slab of rows.  G is computed for a <= b only and written
 *   to (a, b) and (b, a): exactly symmetric.  Every cell of n_j, s and G is written exactly once.
 *   Order of every sum: the rows are cut into the slabs of mmg_chain_plan; a slab is walked in chunks of MMG_CH_CHUNK
 *   rows, a chunk four rows at a time, ascending, each group of four one MFMA onto the running accumulator (the order
 *   inside one instruction is the hardware's and fixed).  The partial tables of the slabs go to ws and are added in
 *   ascending slab order from 0.  All of it is a function of (n, L) alone.
 * mmg_chain_solve: ONE workgroup; the ridge system of target j from n_j, s, G.  Every operation is rounded on its own
 *   (no fused multiply-add; division and square root correctly rounded): it EQUALS the numpy restatement.
 *     C_ab = G_ab - (s_a * s_b) / n_j            (product, division, subtraction)
 *     A = C over the predictors p(0) < p(1) < .. (the labs a != j with count[a] > 0), A_kk += alpha;  rhs_k = C[p(k)][j]
 *   Right-looking Cholesky in place on the lower triangle: for k ascending  d_k = sqrt(A_kk);  A_ik = A_ik / d_k (i > k);
 *   A_il = A_il - A_ik * A_lk (k < l <= i).  A pivot A_kk that is not > 0 adds one to bad (int64 [1], which the caller
 *   zeroes once) and the arithmetic goes on as IEEE has it.  Forward substitution, k ascending:  y_k = y_k / d_k;
 *   y_i = y_i - A_ik * y_k (i > k).  Back substitution, k descending:  y_k = y_k / d_k;  y_i = y_i - A_ki * y_k (i < k).
 *   w (fp64 [L]): w[p(k)] = y_k, 0 elsewhere (w_j = 0);  mu (fp64 [L]): mu_a = s_a / n_j.
 * mmg_chain_apply: for every row i of X outside S_j, one thread per row,
 *     t = 0;  for the predictors a ascending:  t = t + w_a * ((W_ia - center[a]) - mu_a)
 *     W_ij = min(max((center[j] + mu_j) + t, lo[j]), hi[j])
 *   every operation rounded on its own, and delta (fp64 [1]) = the maximum of |new - old| over those rows (0 without
 *   any), or the larger of that and delta's value when accumulate != 0.  The maximum goes through per-block partials in
 *   ws and one final pass: it does not depend on any order.  X and W may be new rows (transform): only count, center
 *   and the coefficients come from the fit.  lo, hi: fp64 [L], -inf / +inf for no clip.
 * mmg_chain_finish: out (fp32 [n, ld_out], ld_out >= L) = X_ia where observed (bit for bit), NaN where count[a] == 0,
 *   else (float)W_ia: one rounding.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.
 * ------------------------------------------------------------------------------------- */
#define MMG_CH_MAX_LABS 128
#define MMG_CH_TILE 64                /* a workgroup's block of the L x L table */
#define MMG_CH_CHUNK 32               /* rows staged in LDS at a time */
#define MMG_CH_BLOCKS 512             /* workgroups the slab plan aims at */
#define MMG_CH_MIN_ROWS 256           /* the shortest slab */
#define MMG_CH_APPLY_ROWS 256         /* rows per workgroup of mmg_chain_apply */
int mmg_chain_plan(int64_t n, int L, int64_t* rows_per_slab, int* slabs);
int mmg_chain_init(const float* X, int64_t n, int L, int64_t ld_x, const double* center, double* W, void* stream);
size_t mmg_chain_moments_ws_bytes(int64_t n, int L);                                            /* 0: unsupported shape */
int mmg_chain_moments(const double* W, const float* X, int64_t n, int L, int64_t ld_x, int j, const double* center,
                      int64_t* n_j, double* s, double* G, void* ws, size_t ws_bytes, void* stream);
int mmg_chain_solve(const double* G, const double* s, const int64_t* n_j, const int64_t* count, int L, int j,
                    double alpha, double* w, double* mu, int64_t* bad, void* stream);
size_t mmg_chain_apply_ws_bytes(int64_t n, int L);                                              /* 0: unsupported shape */
int mmg_chain_apply(double* W, const float* X, int64_t n, int L, int64_t ld_x, int j, const int64_t* count,
                    const double* center, const double* w, const double* mu, const double* lo, const double* hi,
                    int accumulate, double* delta, void* ws, size_t ws_bytes, void* stream);
int mmg_chain_finish(const double* W, const float* X, int64_t n, int L, int64_t ld_x, const int64_t* count, float* out,
                     int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_CHAIN_H */
