/* C ABI of libmmgnn_prop.so: per-lab measurement propensity models (csrc/prop.hip, mmgnn/missingness.py).
 * A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return codes MMG_OK /
 * MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a workspace as the three
 * parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_PROP_H
#define MMGNN_PROP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * L logistic regressions over the same rows, one per lab: P(lab j measured | x), the minimiser of
 *     F(w, b) = sum_i [ log(1 + e^{z_i}) - y_ij z_i ] + ||w||^2 / (2 C),    z_i = u_i . w + b,    u = x - mean
 * (sklearn.linear_model.LogisticRegression(C, penalty="l2", fit_intercept=True); the intercept is not penalised, so
 * centring moves only b), by Newton's method with step halving, every lab in the same launches.  The numpy restatement
 * in mmgnn/missingness.py is the definition; tests/prop_ref.py restates it in loops and 80-bit arithmetic.
 *
 * X is fp32 [n, ld_x], ld_x >= D, 1 <= D <= MMG_PR_MAX_FEATURES, 1 <= n < 2^31, every cell finite (Python refuses NaN
 * and inf).  Columns at and past D are never read.  mean is fp64 [D]; u_ia = (double)X_ia - mean[a], rounded once.
 * Y is uint8 [n, ld_y], ld_y >= L, 1 <= L <= MMG_PR_MAX_LABS, every cell 0 or 1.  M = D + 1: a coefficient vector is
 * fp64 [M], w_0 .. w_{D-1} and then b (the intercept of the CENTRED features).  Vectors of all labs are [L][M].
 * A call works on the labs j0 .. j0 + nb - 1, nb <= mmg_prop_batch(n, D); its per-batch arrays are indexed by k = j - j0.
 * state is int32 [L][MMG_PR_STATE]: ACTIVE, N_ITER, CONVERGED, HALVINGS, STARTED, BAD.  Where a call takes state, a lab
 * with ACTIVE == 0 is FROZEN: its workgroups leave at once, and nothing of it is written.  state may be NULL for
 * mmg_prop_link and mmg_prop_moments: every lab of the batch is worked on.
 *
 * mmg_prop_plan: the slab plan of mmg_prop_moments (a HOST function): rows_per_slab (a multiple of MMG_PR_CHUNK) and
 *   slabs, gram64_plan(n, D + 2, MMG_PR_BLOCKS, MMG_PR_MIN_ROWS): a function of (n, D) alone.
 * mmg_prop_batch: the labs of one batch (a HOST function; 0: unsupported shape):
 *     per_lab = 16 n + slabs (D + 2)^2 8 bytes;   batch = min(MMG_PR_MAX_BATCH, max(1, floor(MMG_PR_WS_BUDGET / per_lab)))
 *   so that the s, r arrays and the partial tables of a batch stay under 1 GiB while one lab fits: at n = 183,400,
 *   D = 128 (85 slabs) per_lab = 14.4 MB and the batch is 64 labs, 0.92 GB.
 * mmg_prop_indicator: Y_ij = X_ij is finite (NaN and +-inf: 0), and, where F is not NULL, F_ij = (float)Y_ij
 *   (fp32 [n, ld_f]).  X here is any fp32 [n, ld_x] matrix with L columns: the contract of mmg_knn_impute.
 * mmg_prop_count: count_j (int64 [L]) = sum_i Y_ij: integers, exact.
 * mmg_prop_link: for every lab of the batch and every row, coef being [L][M],
 *     z = b;  for a ascending:  z = z + u_ia * w_a          (every operation rounded on its own, no fused multiply-add:
 *                                                            it EQUALS numpy)
 *     e = exp(-|z|);  d = 1 + e;  z >= 0:  p = 1 / d, q = e / d;   z < 0:  p = e / d, q = 1 / d       (no cancellation)
 *     s = p * q;   r = y ? -q : p   (= p - y without the cancellation at p near 1)
 *     t = max(z, 0) - y z + log1p(e)   (y z is z or 0; the additions left to right)
 *   s to sr[k][i], r to sr[nb + k][i] (fp64 [2][nb][n]); where z / pq are not NULL, z to z[k][i] (fp64 [nb][n]) and p, q to
 *   pq[k][i], pq[nb + k][i].  exp and log1p are the device library's: s, r and t are within a few ulp of numpy's, not
 *   equal to them.  Order of the loss sum: the rows are cut into blocks of MMG_PR_LINK_ROWS = 64; inside a block
 *   (rows past n count as 0) v_l = v_l + v_{l+o} for l < o, o = 32, 16, 8, 4, 2, 1; the block sums go to
 *   lossp[k][block] (fp64 [nb][ceil(n / 64)]) and are added by mmg_prop_update in ascending block order from 0.
 * mmg_prop_moments: per lab of the batch (grid.z), with u~ = [u, 1] and the table columns c = 0 .. D + 1,
 *     A_i0 = r_i,  A_ic = s_i * u~_i,c-1 (rounded once);    B_i0 = 0,  B_ic = u~_i,c-1
 *     T_ab = sum_i A_ia B_ib   for a <= b:   g_c = T_0,c+1  (fp64 [nb][M]),   H_ac = T_a+1,c+1  (fp64 [nb][M][M])
 *   on v_mfma_f64_16x16x4_f64.  The weight enters ONE side: lattice inputs stay exact.  A diagonal block pair stages both
 *   sides and skips the tiles below the diagonal.  H is computed for a <= c only and written to both (a, c) and (c, a):
 *   exactly symmetric.  Every cell of g and H of a lab that is not frozen is written exactly once.  Order of every sum:
 *   the rows are cut into the slabs of mmg_prop_plan; a slab is walked in chunks of MMG_PR_CHUNK rows, a chunk four rows
 *   at a time, ascending, each group of four one MFMA onto the running accumulator (the order inside one instruction is
 *   the hardware's and fixed).  The partial tables of the slabs go to ws and are added in ascending slab order from 0.
 * mmg_prop_solve: one workgroup per lab; the Newton system at the trial point t = trial[j] (fp64 [L][M]).  Every
 *   operation is rounded on its own (no fused multiply-add; division and square root correctly rounded): it EQUALS the
 *   numpy restatement.
 *     A = H, A_aa = A_aa + 1 / C (a < D);     y_a = g_a + t_a / C (a < D),  y_D = g_D;     rhs = y
 *   Right-looking Cholesky in place on the packed lower triangle in LDS: for k ascending  d_k = sqrt(A_kk);
 *   A_ik = A_ik / d_k (i > k);  A_il = A_il - A_ik * A_lk (k < l <= i).  A pivot A_kk that is not > 0 adds one to
 *   state[j][BAD] and the arithmetic goes on as IEEE has it.  Forward, k ascending:  y_k = y_k / d_k;  y_i = y_i - A_ik *
 *   y_k (i > k).  Back, k descending:  y_k = y_k / d_k;  y_i = y_i - A_ki * y_k (i < k).  delta[k] (fp64 [nb][M]) = y;
 *   dec[k] (fp64 [nb]) = the Newton decrement g~ . H~^{-1} g~:  v = 0;  for a ascending  v = v + rhs_a * y_a.
 * mmg_prop_update: the state machine of one lab, one thread per lab of the batch.  A frozen lab is left alone.  Else
 *     F = (sum of lossp[k], blocks ascending from 0) + (sum_a<D t_a * t_a, ascending from 0) / (2 C)
 *     STARTED:  N_ITER += 1         (N_ITER counts the trial points after the start; a halved retry is one)
 *     accept  =  not STARTED  or  dec <= threshold  or  F <= F_old      -- the decrement first: at the last step F moves
 *                                                                          by rounding only and F <= F_old is a coin
 *     accept:  fstate = (F, 1, dec, F);  STARTED = 1
 *              dec <= threshold:  beta_a = t_a - delta_a (the last step is taken, not evaluated), CONVERGED = 1, ACTIVE = 0
 *              else  beta = t;   N_ITER >= max_iter:  ACTIVE = 0;   else  step = delta;  trial_a = beta_a - step_a
 *     else:    HALVINGS += 1;  scale = scale * 0.5;  N_ITER >= max_iter:  ACTIVE = 0;  else trial_a = beta_a - scale * step_a
 *   fstate is fp64 [L][MMG_PR_FSTATE]: F_old, scale, dec of beta, F of the last trial.  threshold = tol * n is the
 *   caller's.  A fit is max_iter + 1 rounds of link, moments, solve, update over every batch; nothing is read back
 *   between them.
 * mmg_prop_predict: out (fp32 [n, ld_out], ld_out >= L) = (float)p of mmg_prop_link for every lab, any rows: one rounding.
 *   A lab whose b is -inf / +inf and whose w is 0 gives exactly 0 / 1.
 * mmg_prop_pair_sums: inverse-probability-weighted error sums over m pairs (patient_i, lab_i, pred_i, target_i), 0 <= m <
 *   2^31, with P (fp32 [n, ld_p], ld_p >= L) the propensities of mmg_prop_predict.  Per pair, every operation rounded on
 *   its own (division correctly rounded, no fused multiply-add): it EQUALS the numpy restatement.
 *     e = (double)pred - (double)target;  ae = |e|;  e2 = e * e;  pc = max((double)P[patient][lab], clip)
 *     w = stabilized ? cov[lab] / pc : 1 / pc          (cov: fp64 [L], the numerator of the stabilised weight: mean y_j)
 *     terms:  w,  w * w,  w * ae,  w * e2,  ae,  e2
 *   count (int64 [L + 1]): the pairs of every lab, and of all.  sums (fp64 [L + 1][MMG_PR_PAIR_FIELDS]): the six sums per
 *   lab, and overall in row L.  A pair whose lab is outside [0, L) or whose patient is outside [0, n) is in neither
 *   (Python refuses it).  Order of every sum: the pairs are sorted by lab with the stable radix sort of radix_sort.h, so a
 *   lab's pairs keep the order they were given in; a lab's pairs are cut into chunks of MMG_PR_PAIR_CHUNK = 256 from its
 *   first; inside a chunk (missing pairs count as 0) v_l = v_l + v_{l+o} for l < o, o = 128, 64, .., 1; the chunk sums of a
 *   lab are added in ascending chunk order from 0, and the overall row is the labs' sums added in ascending lab order
 *   from 0.  It depends on the order of the pairs inside every lab and on nothing else.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.
 * ------------------------------------------------------------------------------------- */
#define MMG_PR_MAX_FEATURES 128
#define MMG_PR_MAX_LABS 512
#define MMG_PR_MAX_BATCH 64
#define MMG_PR_WS_BUDGET 1000000000   /* bytes of s, r and partial tables of one batch */
#define MMG_PR_TILE 64                /* a workgroup's block of the (D + 2) x (D + 2) table */
#define MMG_PR_CHUNK 32               /* rows staged in LDS at a time */
#define MMG_PR_BLOCKS 512             /* workgroups per lab the slab plan aims at */
#define MMG_PR_MIN_ROWS 256           /* the shortest slab */
#define MMG_PR_LINK_ROWS 64           /* rows per workgroup of mmg_prop_link and mmg_prop_predict */
#define MMG_PR_STATE 8                /* int32 per lab: */
#define MMG_PR_ACTIVE 0
#define MMG_PR_N_ITER 1
#define MMG_PR_CONVERGED 2
#define MMG_PR_HALVINGS 3
#define MMG_PR_STARTED 4
#define MMG_PR_BAD 5
#define MMG_PR_FSTATE 4               /* fp64 per lab: F_old, scale, dec, F of the last trial */
#define MMG_PR_PAIR_CHUNK 256         /* pairs per chunk of mmg_prop_pair_sums */
#define MMG_PR_PAIR_FIELDS 6          /* sum w, sum w^2, sum w |e|, sum w e^2, sum |e|, sum e^2 */
int mmg_prop_plan(int64_t n, int D, int64_t* rows_per_slab, int* slabs);
int mmg_prop_batch(int64_t n, int D);                                                           /* 0: unsupported shape */
int mmg_prop_indicator(const float* X, int64_t n, int L, int64_t ld_x, uint8_t* Y, int64_t ld_y, float* F, int64_t ld_f,
                       void* stream);
int mmg_prop_count(const uint8_t* Y, int64_t n, int L, int64_t ld_y, int64_t* count, void* stream);
int mmg_prop_link(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const uint8_t* Y, int64_t ld_y,
                  int L, int j0, int nb, const double* coef, const int32_t* state, double* z, double* pq, double* sr,
                  double* lossp, void* stream);
size_t mmg_prop_moments_ws_bytes(int64_t n, int D, int nb);                                     /* 0: unsupported shape */
int mmg_prop_moments(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* sr, int L, int j0,
                     int nb, const int32_t* state, double* H, double* g, void* ws, size_t ws_bytes, void* stream);
int mmg_prop_solve(const double* H, const double* g, const double* trial, int D, int L, int j0, int nb, double C,
                   int32_t* state, double* delta, double* dec, void* stream);
int mmg_prop_update(const double* lossp, int64_t n, int D, int L, int j0, int nb, const double* delta, const double* dec,
                    double C, double threshold, int max_iter, double* beta, double* trial, double* step, double* fstate,
                    int32_t* state, void* stream);
int mmg_prop_predict(const float* X, int64_t n, int D, int64_t ld_x, const double* mean, const double* coef, int L,
                     float* out, int64_t ld_out, void* stream);
size_t mmg_prop_pair_sums_ws_bytes(int64_t m, int L);                                          /* 0: unsupported shape */
int mmg_prop_pair_sums(const float* pred, const float* target, const int64_t* patient, const int64_t* lab, int64_t m,
                       const float* P, int64_t n, int L, int64_t ld_p, const double* cov, double clip, int stabilized,
                       int64_t* count, double* sums, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_PROP_H */
