/* C ABI of libmmgnn_conformal.so: split-conformal prediction intervals for imputed labs (csrc/conformal.hip,
 * mmgnn/conformal.py).  A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return
 * codes MMG_OK / MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a
 * workspace as the three parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_CONFORMAL_H
#define MMGNN_CONFORMAL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Order statistics of residuals per (lab, degree bin) cell, and the intervals they give.  The numpy restatement in
 * mmgnn/conformal.py is the definition; device results EQUAL it (integer and order-statistic work; the only sums are
 * the interval widths of mmg_cf_coverage).
 *
 * mmg_seg_order_stats: keys fp32 [n], seg int32 [n].  Row i belongs to segment seg[i] when 0 <= seg[i] < n_seg and
 *   keys[i] is not NaN; every other row (seg[i] = n_seg is the documented "ignored") belongs to none.  With the m keys
 *   of a segment in ascending order x_(1) <= ... <= x_(m) (-0 before +0):
 *     MMG_CF_SIGNED    k_lo = floor((m + 1) * (alpha / 2)),  k_hi = ceil((m + 1) * (1 - alpha / 2)),
 *                      q_lo = x_(k_lo) (k_lo >= 1, else -inf),  q_hi = x_(k_hi) (k_hi <= m, else +inf),
 *                      shift = the median: x_((m + 1) / 2) for odd m, (x_(m / 2) + x_(m / 2 + 1)) / 2 in fp32 for even m,
 *                      0 for m = 0
 *     MMG_CF_ABSOLUTE  k_hi = ceil((m + 1) * (1 - alpha)),  q_hi = x_(k_hi) (k_hi <= m, else +inf),  q_lo = -q_hi,
 *                      shift = 0
 *   The rank arithmetic is fp64, every operation rounded on its own.  usable = every rank exists and m >= min_count.
 *   Outputs per segment: count (int32), q_lo, q_hi, shift (fp32), usable (int32 0 / 1).  One stable LSD radix sort of
 *   (segment << 32 | orderable key bits), two binary searches and the picks by one thread per segment.
 *   0 <= n < 2^31, 1 <= n_seg <= MMG_CF_MAX_CELLS, 0 < alpha < 1, min_count >= 0.
 *
 * A calibration / evaluation pair is (pred[i], target[i], patient[i], lab[i]); the indices are int64 (index_bytes 8) or
 * int32 (4).  deg is int32 [n_patients]; bin j takes deg[patient] in [bin_edges[j], bin_edges[j + 1]) (a HOST array of
 * n_bins + 1 ascending values, +-inf allowed).  cell = lab * n_bins + bin, n_cells = n_labs * n_bins.  An index out of
 * range is never used as an address.
 *
 * mmg_cf_fit: r = target - pred in fp32; the key is r (MMG_CF_SIGNED) or |r| (MMG_CF_ABSOLUTE).  A pair is dropped and
 *   counted in dropped (int64 [4]) under the FIRST of: lab outside [0, n_labs); patient outside [0, n_patients); degree in
 *   no bin; NaN key.  The statistics above are taken at three levels -- the cell, the lab, all pairs -- and row c of the
 *   table takes the first usable level of (cell c, its lab, all): table (fp32 [3][n_cells]: the rows q_lo, q_hi, shift),
 *   level (int32 [n_cells]: 0 cell, 1 lab, 2 all, 3 none: -inf, +inf, 0), n_used (int32 [n_cells]: the pairs of the
 *   segment taken, 0 at level 3).
 * mmg_cf_apply_pairs: lower = p + q_lo, upper = p + q_hi (one fp32 addition each), point = p + shift (use_shift != 0) or p,
 *   with the table row of the pair's cell; a pair without a cell (index out of range, degree in no bin) takes
 *   (-inf, +inf, 0).  A NaN p gives NaN.
 * mmg_cf_apply_matrix: the same for a dense fp32 [n_rows, n_labs] matrix (column c = lab c) with row stride ld; rows
 *   (int64 / int32 [n_rows] by index_bytes, nullable: row i is patient i) names the patient of every row; the outputs
 *   have row stride ld_out, and nothing outside their [n_rows, n_labs] cells is written.
 * mmg_cf_coverage: counts (int64 [n_cells + 1][MMG_CF_COV_FIELDS]) per cell over the evaluation pairs: n, covered
 *   (lower <= t <= upper), below (t < lower), above (t > upper), infinite (a bound that is not finite), dropped (a NaN
 *   pred or target; such a pair is in none of the others).  Row n_cells counts, under dropped, the pairs without a cell.
 *   width (fp64 [n_cells + 1]) = the sum of (double)(upper - lower), the difference formed in fp32, over the cell's
 *   pairs with two finite bounds: the pairs are grouped by a stable sort on the cell, thread t of one 256-thread
 *   workgroup per cell adds the pairs t, t + 256, ... of the group in that order, the 64 lanes of a wave are added by a
 *   fixed butterfly and the four waves in wave order.  No atomics: bitwise reproducible.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed.  n = 0 is valid everywhere.
 * ------------------------------------------------------------------------------------- */
#define MMG_CF_SIGNED 0
#define MMG_CF_ABSOLUTE 1
#define MMG_CF_MAX_LABS 2048
#define MMG_CF_MAX_BINS 64
#define MMG_CF_MAX_CELLS 32768
#define MMG_CF_DROP_KINDS 4
#define MMG_CF_COV_FIELDS 6
size_t mmg_seg_order_stats_ws_bytes(int64_t n, int n_seg);                /* 0 for an unsupported shape */
int mmg_seg_order_stats(const float* keys, const int32_t* seg, int64_t n, int n_seg, double alpha, int mode,
                        int64_t min_count, int32_t* count, float* q_lo, float* q_hi, float* shift, int32_t* usable,
                        void* ws, size_t ws_bytes, void* stream);
size_t mmg_cf_fit_ws_bytes(int64_t n, int n_labs, int n_bins);            /* 0 for an unsupported shape */
int mmg_cf_fit(const float* pred, const float* target, const void* patient, const void* lab, int index_bytes, int64_t n,
               int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins, double alpha,
               int mode, int64_t min_count, float* table, int32_t* level, int32_t* n_used, int64_t* dropped, void* ws,
               size_t ws_bytes, void* stream);
int mmg_cf_apply_pairs(const float* pred, const void* patient, const void* lab, int index_bytes, int64_t n, int n_labs,
                       const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins, const float* table,
                       int use_shift, float* point, float* lower, float* upper, void* stream);
int mmg_cf_apply_matrix(const float* pred, int64_t n_rows, int n_labs, int64_t ld, const void* rows, int index_bytes,
                        const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins, const float* table,
                        int use_shift, float* point, float* lower, float* upper, int64_t ld_out, void* stream);
size_t mmg_cf_coverage_ws_bytes(int64_t n, int n_labs, int n_bins);       /* 0 for an unsupported shape */
int mmg_cf_coverage(const float* pred, const float* target, const void* patient, const void* lab, int index_bytes,
                    int64_t n, int n_labs, const int32_t* deg, int64_t n_patients, const double* bin_edges, int n_bins,
                    const float* table, int64_t* counts, double* width, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_CONFORMAL_H */
