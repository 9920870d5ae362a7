/* C ABI of libmmgnn_nn.so: exact nearest neighbours and neighbour ranks in an embedding space (csrc/nn.hip,
 * mmgnn/neighbors.py).  A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return
 * codes MMG_OK / MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a
 * workspace as the three parameters ws, ws_bytes, stream, a *_ws_bytes companion per call. */
#ifndef MMGNN_NN_H
#define MMGNN_NN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * What sklearn.neighbors.NearestNeighbors(algorithm="brute") and sklearn.manifold.trustworthiness compute, without the
 * n x n matrix.  X is fp32 [n, D] with row stride ld_x >= D, 1 <= D <= MMG_NN_MAX_D (ANY D: a map has D = 2), 1 <= n < 2^31.
 *   distance  s(q, j) = sum_d (q_d - x_jd)^2: the difference form in fp64 from the widened fp32 inputs (never the Gram
 *             form), columns in ascending order, one fma per column -- the arithmetic of mmg_tsne_sqdist;
 *   key       key(q, j) = (s(q, j), j), compared lexicographically: equal sums are ordered by the smaller index, a
 *             non-finite sum orders as +inf.  A TOTAL order: the result does not depend on how the work is split.
 *   mmg_nn_search: row q of the outputs holds the k candidates with the smallest keys in ascending key order:
 *     dist_out (fp32 [nq, k], ld_dist >= k) = (float)sqrt(s), the fp64 square root rounded once; idx_out (int64
 *     [nq, k], ld_idx >= k) = j.  Q (fp32 [nq, D], ld_q >= D) are the queries; Q == NULL is SELF mode: the queries are
 *     the rows of X (nq must equal n) and candidate j == q is skipped, as NearestNeighbors.kneighbors() without X.
 *     1 <= k <= MMG_NN_MAX_K; k <= n - 1 in self mode, k <= n otherwise; 1 <= nq < 2^31.
 *   mmg_nn_rank: for nbr (int64 [n, k], ld_nbr >= k) rank_out[i][c] (int32 [n, k], ld_rank >= k, nullable) =
 *     1 + #{ l != i : key(i, l) < key(i, j) } with j = nbr[i][c]: j's 1-based position in row i's full neighbour order.
 *     An entry with j < 0, j >= n or j == i gets rank 0 and is never used as an address.  penalty_out (int64 [1],
 *     nullable) = sum over all entries of max(0, rank - k): sklearn's trustworthiness is
 *     1 - penalty * 2 / (n k (2n - 3k - 1)) with nbr = the k nearest neighbours in the OTHER space.  It is zeroed by a
 *     kernel and summed with integer atomics, whose order cannot change the result.  1 <= k <= MMG_NN_MAX_K.
 *   mmg_nn_plan (host only): how mmg_nn_search walks a shape -- plan_out (HOST, int64 [3]) = (the number of candidate
 *     ranges, work items = query blocks x candidate ranges, workgroups launched).
 * A workgroup owns MMG_NN_QUERY_BLOCK query rows and streams the candidates through LDS in tiles of MMG_NN_TILE rows;
 * every query keeps a sorted list of its k best keys in LDS and a candidate enters only if its key beats the k-th.  At
 * most MMG_NN_MAX_GRID workgroups are launched; each walks the work items blockIdx.x, blockIdx.x + gridDim.x, ...  With
 * few query blocks the candidates are split into ranges (a work item = one query block x one range, its list left in
 * the workspace) and a second kernel merges the ranges' lists by key.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: results are
 * bitwise the same from run to run and eager against a replayed hipGraph.
 * ------------------------------------------------------------------------------------- */
#define MMG_NN_MAX_K 128
#define MMG_NN_MAX_D 256
#define MMG_NN_QUERY_BLOCK 64
#define MMG_NN_TILE 64
#define MMG_NN_MAX_GRID 1024
size_t mmg_nn_search_ws_bytes(int64_t n, int D, int64_t nq, int k);       /* 0 for an unsupported shape */
int mmg_nn_search(const float* X, int64_t n, int D, int64_t ld_x, const float* Q, int64_t nq, int64_t ld_q, int k,
                  float* dist_out, int64_t ld_dist, int64_t* idx_out, int64_t ld_idx, void* ws, size_t ws_bytes,
                  void* stream);
size_t mmg_nn_rank_ws_bytes(int64_t n, int D, int k);                     /* 0 for an unsupported shape */
int mmg_nn_rank(const float* X, int64_t n, int D, int64_t ld_x, const int64_t* nbr, int64_t ld_nbr, int k,
                int32_t* rank_out, int64_t ld_rank, int64_t* penalty_out, void* ws, size_t ws_bytes, void* stream);
int mmg_nn_plan(int64_t n, int64_t nq, int64_t* plan_out);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_NN_H */
