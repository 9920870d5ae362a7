/* C ABI of libmmgnn_cluster.so: k-means (Lloyd) over an embedding space and the cluster scores (csrc/cluster.hip,
 * mmgnn/cluster.py).  A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return
 * codes MMG_OK / MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a
 * workspace as the three parameters ws, ws_bytes, stream, a *_ws_bytes companion per call. */
#ifndef MMGNN_CLUSTER_H
#define MMGNN_CLUSTER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * What sklearn.cluster.KMeans(init=array, n_init=1, algorithm="lloyd") and sklearn.metrics.silhouette_samples compute.
 * X is fp32 [n, D] with row stride ld_x >= D, 1 <= D <= MMG_KM_MAX_D, 1 <= n < 2^31.  The centres C are fp64 [k, D],
 * contiguous, 1 <= k <= MMG_KM_MAX_K and k <= n.
 *   distance    s(i, c) = sum_d ((double)x_id - C_cd)^2: the difference form in fp64 (never the Gram form), columns in
 *               ascending order, one fma per column; a non-finite sum orders as +inf (and is stored as +inf).
 *   assignment  label(i) = the centre with the smallest key (s(i, c), c): equal sums go to the smaller centre index.  A
 *               TOTAL order: the result does not depend on the tiling.
 *   mmg_km_assign: labels (int32 [n]) and min_s (fp64 [n]) = s(i, label(i)).  prev_labels (int32 [n], nullable, MAY be
 *     labels itself) and changed (int64 [1], nullable): changed = #{i : label(i) != prev_labels(i)}, every row when
 *     prev_labels is NULL; zeroed by a kernel and summed with integer atomics, whose order cannot change the result.
 *   mmg_km_label_dist: out_s (fp64 [n]) = s(i, labels(i)), the same sum against the row's OWN centre (the scores of a
 *     labelling that is not an assignment); +inf for a label outside [0, k), which is never used as an address.  The one
 *     call without a workspace.
 *   mmg_km_update: from labels and min_s of an assignment against C_old
 *       count_c = #{i : label(i) = c},  sum_c = sum of (double)x_i over those rows, per column.
 *     Order of summation (it depends on n alone): the rows are cut into R = ceil(n / rows_per_range) ranges of
 *     rows_per_range = MMG_KM_ROW_TILE * ceil(ceil(n / MMG_KM_ROW_TILE) / MMG_KM_MAX_RANGES) consecutive rows; inside a
 *     range a (cluster, column) sum takes its rows in ascending row order starting from 0.0, and the ranges' sums are
 *     added in ascending range order starting from 0.0.  No floating-point atomics.
 *     Empty clusters (sklearn's _relocate_empty_clusters_dense made a total order): let the m clusters with count 0 be
 *     taken in ascending index; the e-th of them takes the row with the e-th largest key (min_s descending, then the
 *     SMALLER row index).  For e ascending that row is subtracted from the sum and the count of the cluster it is
 *     labelled with, and becomes the sum (count 1) of the empty cluster.  Labels are not changed.  A cluster whose count
 *     is 0 afterwards keeps its old centre.
 *       C_new[c][d] = sum_c[d] / count_c;  shift = sum_c (sum_d (C_new[c][d] - C_old[c][d])^2, d ascending), c ascending.
 *     C_new MAY be C_old.  counts (int32 [k]) are the counts after relocation.  status (fp64 [3]) = (changed, shift, m)
 *     with changed read from the int64 `changed` of mmg_km_assign (nullable: 0).
 *   mmg_km_colstats: col_mean (fp64 [D]) and mean_var (fp64 [1]) = mean_d of the population variance of column d, from
 *     ONE pass: per column sum x and sum x^2 in fp64, the rows of a range (as above) with row % 8 == g summed in
 *     ascending order per g = 0..7, the eight added in ascending g, the ranges in ascending order;
 *     var_d = max(0, sum x^2 / n - mean_d^2).  tol_abs of sklearn's KMeans is mean_var * tol.
 *   mmg_km_scores: from labels and min_s: inertia (fp64 [1]) = sum_i min_s(i); sdist (fp64 [k]) = sum over the rows of
 *     cluster c of sqrt(min_s(i)); counts (int32 [k]).  Rows ascending within a range, ranges ascending.
 *   mmg_km_silhouette: for the nq rows i = queries[q] (int32 [nq]; NULL: i = q, nq must equal n), labels int32 [n] in
 *     [0, k) and counts int32 [k] (the rows per label), 2 <= k <= MMG_KM_MAX_K:
 *       S(i, c) = sum over j with label(j) = c of sqrt(s_xx(i, j)),  s_xx(i, j) = sum_d ((double)x_id - (double)x_jd)^2
 *     (the row-to-row distance of mmg_nn_search; j = i contributes 0).  The candidates are cut into ranges of whole
 *     MMG_KM_ROW_TILE-row tiles (mmg_km_sil_plan); inside a range j ascends from 0.0, the ranges are added in ascending
 *     order.  a = S(i, own) / (count_own - 1); b = min over c != own with count_c > 0 of S(i, c) / count_c;
 *     sil(i) = (b - a) / max(a, b), 0 where count_own == 1 or max(a, b) is 0 or not finite.  sil is fp64 [nq]; sil_mean
 *     (fp64 [1], nullable) = (sum_t (sum of sil[q], q = t, t + 256, ... ascending), t = 0..255 ascending) / nq.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: results are
 * bitwise the same from run to run and eager against a replayed hipGraph.
 * ------------------------------------------------------------------------------------- */
#define MMG_KM_MAX_K 128
#define MMG_KM_MAX_D 256
#define MMG_KM_ROW_TILE 64
#define MMG_KM_MAX_RANGES 128
#define MMG_KM_MAX_GRID 1024
size_t mmg_km_assign_ws_bytes(int64_t n, int D, int k);                   /* 0 for an unsupported shape */
int mmg_km_assign(const float* X, int64_t n, int D, int64_t ld_x, const double* C, int k, const int32_t* prev_labels,
                  int32_t* labels, double* min_s, int64_t* changed, void* ws, size_t ws_bytes, void* stream);
int mmg_km_label_dist(const float* X, int64_t n, int D, int64_t ld_x, const double* C, int k, const int32_t* labels,
                      double* out_s, void* stream);
size_t mmg_km_update_ws_bytes(int64_t n, int D, int k);                   /* 0 for an unsupported shape */
int mmg_km_update(const float* X, int64_t n, int D, int64_t ld_x, const int32_t* labels, const double* min_s,
                  const double* C_old, int k, double* C_new, int32_t* counts, const int64_t* changed, double* status,
                  int64_t* reloc_rows, void* ws, size_t ws_bytes, void* stream);
/* reloc_rows (int64 [k], nullable): the row taken by the e-th empty cluster for e < m, -1 beyond */
size_t mmg_km_colstats_ws_bytes(int64_t n, int D);                        /* 0 for an unsupported shape */
int mmg_km_colstats(const float* X, int64_t n, int D, int64_t ld_x, double* col_mean, double* mean_var, void* ws,
                    size_t ws_bytes, void* stream);
size_t mmg_km_scores_ws_bytes(int64_t n, int k);                          /* 0 for an unsupported shape */
int mmg_km_scores(const int32_t* labels, const double* min_s, int64_t n, int k, double* inertia, double* sdist,
                  int32_t* counts, void* ws, size_t ws_bytes, void* stream);
size_t mmg_km_silhouette_ws_bytes(int64_t n, int D, int64_t nq, int k);   /* 0 for an unsupported shape */
int mmg_km_silhouette(const float* X, int64_t n, int D, int64_t ld_x, const int32_t* labels, const int32_t* counts, int k,
                      const int32_t* queries, int64_t nq, double* sil, double* sil_mean, void* ws, size_t ws_bytes,
                      void* stream);
/* host only: plan_out (HOST, int64 [3]) = (row ranges of mmg_km_update, rows per range, workgroups of mmg_km_assign) */
int mmg_km_plan(int64_t n, int64_t* plan_out);
/* host only: plan_out (HOST, int64 [3]) = (candidate ranges of mmg_km_silhouette, work items, workgroups launched) */
int mmg_km_sil_plan(int64_t n, int64_t nq, int64_t* plan_out);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_CLUSTER_H */
