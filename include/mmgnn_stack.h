/* C ABI of libmmgnn_stack.so: per-lab stacked recalibration of imputed lab values (csrc/stack.hip, mmgnn/stacking.py).
 * A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return codes MMG_OK /
 * MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a workspace as the three
 * parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_STACK_H
#define MMGNN_STACK_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * A ridge regression of the TARGET on K predictors per (lab, patient lab-degree bin) cell, fitted out of sample and
 * applied to predictions.  The numpy restatement in mmgnn/stacking.py is the definition; device results EQUAL it.
 *
 * A pair is (feats[0][i] .. feats[K - 1][i], target[i], patient[i], lab[i]): feats is a HOST array of K device pointers
 * to fp32 [n] (1 <= K <= MMG_ST_MAX_FEATURES; feats[0] is by convention the model's own prediction), the indices are
 * int64 (index_bytes 8) or int32 (4).  phi = (1, f_1, .., f_K).  Cells are those of include/mmgnn_conformal.h: deg int32
 * [n_patients], bin j takes deg[patient] in [bin_edges[j], bin_edges[j + 1]) (a HOST array of n_bins + 1 ascending
 * values, +-inf allowed), cell = lab * n_bins + bin, n_cells = n_labs * n_bins.  An index out of range is never used as
 * an address.  A pair is dropped and counted in dropped (int64 [4]) under the FIRST of: lab outside [0, n_labs); patient
 * outside [0, n_patients); degree in no bin; a NaN in the target or in any feature.
 *
 * Folds.  fold(patient) = (the first word of mmg_rng_group(mmg_rng_key(seed, MMG_ST_SITE), patient)) mod folds, 1 <= folds
 * <= MMG_ST_MAX_FOLDS: a function of the patient alone, so all pairs of a patient share a fold.
 *
 * mmg_stack_sums: sums (fp64 [folds][n_cells][F], F = (K + 1)(K + 2) / 2 + K + 2) per (fold, cell) over its kept pairs:
 *   the upper triangle of sum phi phi^T row-major ((0,0), (0,1), .., (0,K), (1,1), .., (K,K); entry (0,0) is the count),
 *   then sum phi_j t (j = 0 .. K), then sum t^2.  Every term is the product of two fp32 values formed in fp64: exact, so only
 *   the ORDER of the additions matters, and it is fixed.  The kept pairs are brought into segment order (segment = fold *
 *   n_cells + cell) by a stable radix sort (ties: ascending pair position).  The m pairs of a segment are cut into its own
 *   chunks of C = MMG_ST_CHUNK consecutive sorted pairs, chunk j = the segment's pairs [j C, min((j + 1) C, m)): a chunk never
 *   holds pairs of two segments.  Inside a chunk, slot t (0 .. 255) adds the chunk's pairs t, t + 256, t + 512, .. in that
 *   order from 0; the 64 slots 64 w .. 64 w + 63 are added by the butterfly v = v + v[slot ^ o], o = 32, 16, 8, 4, 2, 1; the four
 *   results w = 0 .. 3 are added in that order from 0.  The chunks of a segment are then added in chunk order from 0.  Nothing
 *   of this depends on the launch grid; there is no floating-point atomic (the dropped counters are integer atomics).
 * mmg_stack_solve: sums -> coef (fp64 [folds_out][n_cells][K + 1]), level, n_used (int32 [folds_out][n_cells]).  folds_out
 *   = 1 for folds = 1, else folds + 1.  The training sums of row j < folds ("fold-out j") are the sums of all folds but j
 *   added in fold order from 0; the last row (the only one for folds = 1) adds every fold: all pairs.  Three levels: the
 *   cell; its lab (the cells' training sums added in bin order from 0); all pairs (the labs' sums added in lab order from 0).
 *   A system, with G = sum phi phi^T, h = sum phi t, m = G_00, e = (0, 1, 0, .., 0) -- the ridge pulls toward "keep f_1":
 *     A = G, but A_ii = G_ii + ridge * G_ii;   rhs = h, but rhs_1 = h_1 + ridge * G_11
 *     Cholesky A = L L^T by rows i = 0 .. K, columns j = 0 .. i:  s = A_ij;  s = s - L_ik * L_jk for k = 0 .. j - 1 in that
 *       order;  j < i: L_ij = s / L_jj;  j = i: the pivot s must exceed MMG_ST_PIVOT_REL * A_ii, L_ii = sqrt(s)
 *     forward   z_i = (rhs_i - L_i0 z_0 - .. - L_i,i-1 z_i-1) / L_ii,  i = 0 .. K, subtracted in that order
 *     backward  w_i = (z_i - L_i+1,i w_i+1 - .. - L_Ki w_K) / L_ii,    i = K .. 0, subtracted in that order
 *   all in fp64, every operation rounded on its own (no fused multiply-add).  A level is usable when m >= max(min_count,
 *   K + 2) and every pivot passes.  A cell takes the first usable level of (cell, lab, all): level 0 / 1 / 2, n_used = that
 *   level's m; with none usable level 3, n_used 0 and coef = e, which leaves f_1 as it is.  MMG_ST_PIVOT_REL = 1e-10
 *   (MMG_ST_PIVOT_REL_LOG10).  ridge >= 0 and finite, min_count >= 0.
 * mmg_stack_apply_pairs: out[i] (fp32) = y rounded once, y = w_0; y = y + w_k * f_k for k = 1 .. K in that order, each
 *   operation rounded on its own in fp64, with the coefficients of the pair's cell: of the last row of coef (cross = 0),
 *   or of row fold(patient) -- the out-of-fold prediction (cross != 0, folds >= 2).  A pair without a cell (index out of
 *   range, degree in no bin) keeps f_1.  A NaN feature gives NaN.
 * mmg_stack_apply_matrix: the same for dense [n_rows, n_labs] fp32 features (column c = lab c): feature k is feats[k] with
 *   row stride strides[k] (a HOST array; >= n_labs, or 0: a per-lab vector [n_labs] broadcast over the rows); rows (int64 /
 *   int32 [n_rows] by index_bytes, nullable: row i is patient i) names the patient of every row; out has row stride ld_out
 *   and nothing outside its [n_rows, n_labs] cells is written.
 * mmg_stack_scores: raw, stacked, target fp32 [n] -> scores (fp64 [n_cells + n_labs + 1][MMG_ST_SCORE_FIELDS]): n, sum |t -
 *   raw|, sum (t - raw)^2, sum |t - stacked|, sum (t - stacked)^2, with e = t - p formed in fp32 and the terms (double)|e| and
 *   (double)e * (double)e as mmg_seg_metrics forms them.  Rows 0 .. n_cells - 1 are the cells, summed in the order of
 *   mmg_stack_sums (one fold); row n_cells + l is lab l, its cells added in bin order from 0; the last row is all pairs,
 *   the lab rows added in lab order from 0.  dropped (int64 [4]) as above, the NaN test over raw, stacked and target.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.  n = 0 is valid
 * everywhere.  0 <= n < 2^31; the limits on labs, bins and cells are those of the conformal library.
 * ------------------------------------------------------------------------------------- */
#define MMG_ST_SITE 1398033201        /* 0x53544B31, "STK1" */
#define MMG_ST_MAX_FEATURES 4
#define MMG_ST_MAX_FOLDS 8
#define MMG_ST_MAX_LABS 2048
#define MMG_ST_MAX_BINS 64
#define MMG_ST_MAX_CELLS 32768
#define MMG_ST_CHUNK 4096             /* C: sorted pairs of one segment per chunk */
#define MMG_ST_DROP_KINDS 4
#define MMG_ST_SCORE_FIELDS 5
#define MMG_ST_PIVOT_REL_LOG10 (-10)
size_t mmg_stack_sums_ws_bytes(int64_t n, int n_labs, int n_bins, int n_features, int folds);   /* 0: unsupported shape */
int mmg_stack_sums(const float* const* feats, int n_features, const float* target, const void* patient, const void* lab,
                   int index_bytes, int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges,
                   int n_bins, int folds, uint64_t seed, double* sums, int64_t* dropped, void* ws, size_t ws_bytes,
                   void* stream);
size_t mmg_stack_solve_ws_bytes(int n_labs, int n_bins, int n_features, int folds);             /* 0: unsupported shape */
int mmg_stack_solve(const double* sums, int n_labs, int n_bins, int n_features, int folds, double ridge, int64_t min_count,
                    double* coef, int32_t* level, int32_t* n_used, void* ws, size_t ws_bytes, void* stream);
int mmg_stack_apply_pairs(const float* const* feats, int n_features, const void* patient, const void* lab, int index_bytes,
                          int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                          const double* coef, int folds, uint64_t seed, int cross, float* out, void* stream);
int mmg_stack_apply_matrix(const float* const* feats, const int64_t* strides, int n_features, int64_t n_rows, int n_labs,
                           const void* rows, int index_bytes, const int32_t* deg, int64_t n_patients,
                           const double* bin_edges, int n_bins, const double* coef, int folds, uint64_t seed, int cross,
                           float* out, int64_t ld_out, void* stream);
size_t mmg_stack_scores_ws_bytes(int64_t n, int n_labs, int n_bins);                            /* 0: unsupported shape */
int mmg_stack_scores(const float* raw, const float* stacked, const float* target, const void* patient, const void* lab,
                     int index_bytes, int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges,
                     int n_bins, double* scores, int64_t* dropped, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_STACK_H */
