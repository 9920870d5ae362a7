/* C ABI of libmmgnn_mf.so: lab imputation by low-rank matrix completion, regularised alternating least squares
 * (csrc/mf.hip, mmgnn/lowrank.py).  A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it
 * keeps: return codes MMG_OK / MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of
 * libmmgnn.so, a workspace as the three parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_MF_H
#define MMGNN_MF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The model: every patient i has a vector u_i, every lab l a vector v_l (fp64, r values each, 1 <= r <=
 * MMG_MF_MAX_RANK), and the value of lab l for patient i is center_l + u_i . v_l.  The factors minimise
 *     F = sum over the observed pairs (y - u_i . v_l)^2 + reg (|U|^2 + |V|^2),      y = value - center_lab,
 * by alternating least squares over the observed (patient, lab, value) triples alone.  The numpy functions of
 * mmgnn/lowrank.py are the definition; tests/mf_ref.py restates them in loops, math.fsum and 80-bit arithmetic.
 *
 * SEGMENTS.  The pairs are held twice: by patient (labs ascending inside a patient) and by lab (patients ascending
 * inside a lab).  An ordering is ptr (int64 [segments + 1], ptr[0] = 0, ptr[segments] = nnz, ascending), idx (int32
 * [nnz]: the OTHER side's index of every pair) and y (fp64 [nnz]).  0 <= nnz < 2^31, 1 <= segments < 2^31.
 *
 * THE SUM RULE.  Every floating-point sum of this library over the items of a segment takes them in stored order,
 * cut into chunks of MMG_MF_CHUNK items counted from the segment's start.  A chunk's items are added one after the
 * other, ascending, onto 0; the chunk sums are added one after the other, ascending, onto the first.  A product that
 * enters such a sum may be formed inside a fused multiply-add.  The order depends on the segment's length alone: not on
 * the grid, on the neighbouring segments or on where the segment lies in the array.  No floating-point atomics.
 *
 * mmg_mf_index: the triples (patient int64 [nnz], lab int64 [nnz], value fp32 [nnz]; every pair at most once, indices in
 *   range, no NaN -- the caller's checks) -> both orderings, built with the stable radix sort of radix_sort.h and the
 *   scan of scan.h:  p_ptr [n_patients + 1], p_idx (labs), p_val (the fp32 values, bit for bit), p_y;  l_ptr
 *   [n_labs + 1], l_idx (patients), l_y;  count (int64 [n_labs]) = the pairs of a lab;  center (fp64 [n_labs]) = the sum
 *   of the lab's values as doubles in the lab ordering, by the sum rule, divided by count (0 for count 0).
 *   center_fixed (nullable, fp64 [n_labs]): used INSTEAD of the means (center is a copy of it).  y = (double)value -
 *   center[lab], one rounding.  1 <= n_labs <= MMG_MF_MAX_LABS, 1 <= n_patients < 2^31.
 * mmg_mf_plan: how a segment of `length` pairs is summed (a HOST function).  path MMG_MF_PATH_EMPTY: length 0;
 *   MMG_MF_PATH_WAVE: length <= MMG_MF_SPLIT, one wave sums chunk after chunk and solves, nothing leaves LDS and
 *   registers;  MMG_MF_PATH_SPLIT: longer, every chunk is one job of a grid-wide launch, the chunk sums go through the
 *   workspace and the segment's wave adds them in ascending order before it solves.  chunks = ceil(length /
 *   MMG_MF_CHUNK).  All three give the sums of the rule above.
 * mmg_mf_half_sweep: for every segment s, with F = other (fp64 [m, r], rows contiguous) and f_q = F[idx[q]]
 *     A_s = sum_q f_q f_q^T  (+ reg on the diagonal: one addition after the sum)      b_s = sum_q f_q y_q
 *     out[s] (fp64 [segments, r]) = A_s^{-1} b_s
 *   A is computed for k <= l only: exactly symmetric.  The solve is the right-looking Cholesky in place on the lower
 *   triangle and the two column-oriented substitutions of mmg_chain_solve (include/mmgnn_chain.h), every operation
 *   rounded on its own, no fused multiply-add, division and square root correctly rounded: it EQUALS
 *   lowrank.host_solve.  A pivot that is not > 0 adds one to bad (int64 [1], which the caller zeroes once) and the
 *   arithmetic goes on as IEEE has it.  An empty segment gets the zero vector.  normal_out (nullable; NULL in
 *   production): fp64 [segments, r * r + r], every segment's A (row-major, both halves) then b.  An idx outside [0, m)
 *   enters as a zero row; a ptr outside [0, nnz] is clamped.
 * mmg_mf_objective: out (fp64 [3]) = { sum over the pairs of the by-patient ordering of (y - t)^2, |U|^2, |V|^2 }, t = the
 *   dot product as in mmg_mf_predict_pairs.  Each of the three is ONE segment under the sum rule (the pairs in stored
 *   order; U and V row-major), with the chunk sums themselves summed by the rule again, level after level, until one is
 *   left.  F = out[0] + reg (out[1] + out[2]) is the caller's.
 * mmg_mf_predict_pairs: out[e] (fp32) = count[lab] == 0 ? NaN : (float)min(max(center[lab] + t, lo), hi) with t = 0;
 *   t = t + U[patient][k] * V[lab][k] for k ascending, every operation rounded on its own; one rounding to fp32.
 *   patient, lab: int64 [n], in range (the caller's check; an index out of range gives NaN).
 * mmg_mf_impute_matrix: out (fp32 [n_rows, ld_out], ld_out >= n_labs): row j is patient i = rows[j] (int64; NULL: i = j):
 *   every lab's prediction as above from U[i], then the patient's own values p_val over p_ptr[i] .. p_ptr[i + 1], bit
 *   for bit.  0 <= i < n_patients.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.
 * ------------------------------------------------------------------------------------- */
#define MMG_MF_MAX_LABS 2048
#define MMG_MF_MAX_RANK 32
#define MMG_MF_CHUNK 256              /* pairs per chunk of the sum rule */
#define MMG_MF_SPLIT 2048             /* the longest segment one wave sums on its own (a multiple of the chunk) */
#define MMG_MF_PATH_EMPTY 0
#define MMG_MF_PATH_WAVE 1
#define MMG_MF_PATH_SPLIT 2
int mmg_mf_plan(int64_t length, int* path, int64_t* chunks);
size_t mmg_mf_index_ws_bytes(int64_t nnz, int64_t n_patients, int n_labs);                      /* 0: unsupported shape */
int mmg_mf_index(const int64_t* patient, const int64_t* lab, const float* value, int64_t nnz, int64_t n_patients,
                 int n_labs, const double* center_fixed, int64_t* p_ptr, int32_t* p_idx, float* p_val, double* p_y,
                 int64_t* l_ptr, int32_t* l_idx, double* l_y, int64_t* count, double* center, void* ws, size_t ws_bytes,
                 void* stream);
size_t mmg_mf_half_sweep_ws_bytes(int64_t segments, int64_t nnz, int r);                       /* 0: unsupported shape */
int mmg_mf_half_sweep(const int64_t* ptr, const int32_t* idx, const double* y, int64_t segments, int64_t nnz,
                      const double* other, int64_t m, int r, double reg, double* out, int64_t* bad, double* normal_out,
                      void* ws, size_t ws_bytes, void* stream);
size_t mmg_mf_objective_ws_bytes(int64_t nnz, int64_t n_patients, int n_labs, int r);          /* 0: unsupported shape */
int mmg_mf_objective(const int64_t* p_ptr, const int32_t* p_idx, const double* p_y, int64_t nnz, int64_t n_patients,
                     int n_labs, const double* U, const double* V, int r, double* out, void* ws, size_t ws_bytes,
                     void* stream);
int mmg_mf_predict_pairs(const int64_t* patient, const int64_t* lab, int64_t n, const double* U, int64_t n_patients,
                         const double* V, int n_labs, int r, const double* center, const int64_t* count, double lo,
                         double hi, float* out, void* stream);
int mmg_mf_impute_matrix(const int64_t* rows, int64_t n_rows, const double* U, int64_t n_patients, const double* V,
                         int n_labs, int r, const double* center, const int64_t* count, double lo, double hi,
                         const int64_t* p_ptr, const int32_t* p_idx, const float* p_val, int64_t nnz, float* out,
                         int64_t ld_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_MF_H */
