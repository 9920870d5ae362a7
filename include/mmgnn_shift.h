/* C ABI of libmmgnn_shift.so: per-lab two-sample tests between two cohorts of lab values or residuals -- Kolmogorov-
 * Smirnov, Wasserstein-1, standardised mean difference, coverage difference -- with permutation p-values over the units
 * (patients) and the single-step maxT adjustment over the labs (csrc/shift.hip, mmgnn/shift.py).  A library of its own
 * beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return codes MMG_OK / MMG_E_ARG / MMG_E_WS /
 * MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a workspace as the three parameters ws, ws_bytes,
 * stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_SHIFT_H
#define MMGNN_SHIFT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The cohorts.  group (uint8 [n_units]): 1 = cohort A, 0 = cohort B, any other value: the unit takes part in neither.
 * U = the number of participating units, U_A = those of them in A.
 *
 * mmg_shift_thresholds: the labels of every replicate, without a stored permutation.  Replicate 0 is the labelling
 *   given.  Replicate b (1 .. replicates) relabels the participating units and keeps U_A:
 *     key_b(u) = (uint64)(the first word of mmg_rng_group(mmg_rng_key(seed, MMG_SHIFT_SITE + b), u)) << 32 | u
 *     T[b]     = the U_A-th smallest key_b(u) over the participating units  (numpy.partition(keys, U_A - 1)[U_A - 1])
 *     unit u is in A in replicate b  iff  key_b(u) <= T[b]
 *   The keys of two units differ in their low word, so exactly U_A units are in A.  T is uint64 [replicates + 1]; T[0] is
 *   written as 0 and not used.  One workgroup per replicate runs a radix select: eight 8-bit digit passes from the top
 *   digit down, the hashes recomputed in every pass and never stored, the 256-bin histogram in LDS (integer atomics: the
 *   counts do not depend on their order).
 *   counts (int64 [MMG_SHIFT_COUNTS]) = {U, U_A, status}: status is MMG_SHIFT_OK, or MMG_SHIFT_BAD_COHORTS unless
 *   1 <= U_A < U.  The two sizes are counted on the device, so this ONE requirement is a status word and not a return
 *   code: the caller reads it (mmgnn.shift raises on it).  With MMG_SHIFT_BAD_COHORTS every T[b] is 0; the calls below
 *   still write every element of their outputs, which then mean nothing.
 *   0 <= n_units < 2^31, 0 <= replicates <= MMG_SHIFT_MAX_REPLICATES.
 *
 * mmg_shift_stats: value fp32 [n]; seg (the lab) and unit int64 (index_bytes 8) or int32 (4) [n].  A pair is dropped, and
 *   counted in dropped (int64 [MMG_SHIFT_DROP_KINDS]), under the FIRST of: seg outside [0, n_seg); unit outside
 *   [0, n_units); a NaN or infinite value; a group of the unit that is neither 0 nor 1.  The kept pairs are brought into
 *   (lab, value) order by one stable radix sort of the key  lab << 32 | orderable(value)  (orderable: the bits of the
 *   value with the sign bit set for a value >= 0 and all bits inverted for one < 0; -0.0 is taken as +0.0 first), ties
 *   in ascending pair position.  A TIE GROUP is a maximal run of equal values inside a lab.  With c_a, c_b the running
 *   counts of the two cohorts at the END of a tie group and n_a, n_b the lab's totals, all under the labels of the
 *   replicate, per (replicate r, lab):
 *     counts (int64 [replicates + 1][n_seg][MMG_SHIFT_INT_FIELDS]) = n_a, n_b,
 *            K_plus = max(c_a n_b - c_b n_a), K_minus = max(c_b n_a - c_a n_b) over the group ends (both >= 0: the last
 *            group gives 0); all exact.
 *     sums   (fp64 [replicates + 1][n_seg][MMG_SHIFT_SUM_FIELDS]) =
 *            W = the sum over the group ends but the lab's last of (double)|c_a n_b - c_b n_a| * ((double)v_next - (double)v)
 *                (v_next: the value of the next group; the conversion is exact below 2^53, the difference is rounded
 *                once and is exact for values within 2^29 of each other in magnitude, the product is rounded once),
 *            S_a, S_b = the sums of the values of the two cohorts, Q_a, Q_b = the sums of (double)v * (double)v (exact).
 *   The ORDER of every fp64 sum is a function of the sorted position alone: the sorted kept pairs are cut into chunks of
 *   MMG_SHIFT_CHUNK; inside a chunk a lab's terms are added left to right from 0 (the term of W belongs to the chunk of
 *   its group end; a pair adds 0 to the sums of the cohort it is not in); a lab's chunk sums are then added in chunk order
 *   from 0.  Nothing depends on the launch grid; there is no floating-point atomic (the dropped counters are integer
 *   atomics).  A workgroup serves MMG_SHIFT_RB replicates of one chunk, one per thread; the running counts at a chunk's
 *   start come from an integer counting pass over the same layout and a prefix over the chunks of a lab.  A lab without
 *   kept pairs has zeros everywhere.
 *   0 <= n < 2^31 (n = 0 is valid), 1 <= n_seg <= MMG_SHIFT_MAX_SEG, 0 <= n_units < 2^31,
 *   0 <= replicates <= MMG_SHIFT_MAX_REPLICATES.  T: what mmg_shift_thresholds wrote for the same group, seed, replicates.
 *
 * mmg_shift_finish: -> stats (fp64 [replicates + 1][n_seg + 1][MMG_SHIFT_STAT_FIELDS]); every operation rounded in fp64 on
 *   its own (no fused multiply-add); (double) of an int64 rounds to nearest.  With P = (double)(n_a * n_b), na = (double)n_a,
 *   nb = (double)n_b:
 *     0 D        = (double)max(K_plus, K_minus) / P
 *     1 D_signed = D for K_plus >= K_minus, else -D
 *     2 W1       = W / P
 *     3 smd      = num / den,  num = S_a / na - S_b / nb,  den = sqrt((var_a + var_b) / 2),
 *                  var_x = max((Q_x - S_x * S_x / nx) / (nx - 1), 0);  NaN for n_a < 2 or n_b < 2;  0 for num == 0 and den == 0
 *     4 z        = D * sqrt(P / (na + nb))
 *     5 cov      = na / (double)U_A - nb / (double)(U - U_A)        (counts of mmg_shift_thresholds)
 *   A lab with n_a = 0 or n_b = 0 is NaN in fields 0 - 4.  Row n_seg: field 4 is the maximum of z over the labs where it
 *   is not NaN (NaN without one) -- the single-step maxT statistic of the replicate; its other fields are NaN.
 * mmg_shift_summary: stats -> summary (fp64 [n_seg + 1][MMG_SHIFT_SUMMARY_FIELDS]).  For a statistic x with x_0 that of
 *   replicate 0: count = #{b in 1 .. replicates : x_b >= x_0}, m = #{b : x_b is not NaN}, p = (1 + count) / (1 + m); NaN
 *   when x_0 is NaN.  Row `lab`:
 *     0 p of D   1 p of W1   2 p of |smd|   3 p of |cov|
 *     4 p_adj = (1 + #{b : maxz_b >= z_0(lab)}) / (1 + #{b : maxz_b is not NaN}),  maxz_b = stats[b][n_seg][4]
 *     5 the count behind field 0   6 the count behind field 4        (integers, exactly representable)
 *   Row n_seg: fields 4 and 6 for x = maxz itself, the other fields NaN.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.
 * ------------------------------------------------------------------------------------- */
#define MMG_SHIFT_SITE 1397245524     /* 0x53484654, "SHFT" */
#define MMG_SHIFT_MAX_REPLICATES 4096
#define MMG_SHIFT_MAX_SEG 2048
#define MMG_SHIFT_CHUNK 2048         /* C: sorted pairs per chunk */
#define MMG_SHIFT_RB 256             /* RB: replicates per workgroup, one per thread */
#define MMG_SHIFT_DROP_KINDS 4
#define MMG_SHIFT_COUNTS 3
#define MMG_SHIFT_OK 0
#define MMG_SHIFT_BAD_COHORTS 1
#define MMG_SHIFT_INT_FIELDS 4
#define MMG_SHIFT_SUM_FIELDS 5
#define MMG_SHIFT_STAT_FIELDS 6
#define MMG_SHIFT_SUMMARY_FIELDS 7
int mmg_shift_thresholds(const uint8_t* group, int64_t n_units, int replicates, uint64_t seed, uint64_t* T, int64_t* counts,
                         void* stream);
size_t mmg_shift_stats_ws_bytes(int64_t n, int n_seg, int replicates);      /* 0 for an unsupported shape */
int mmg_shift_stats(const float* value, const void* seg, const void* unit, int index_bytes, int64_t n, int n_seg,
                    const uint8_t* group, int64_t n_units, int replicates, uint64_t seed, const uint64_t* T,
                    int64_t* counts, double* sums, int64_t* dropped, void* ws, size_t ws_bytes, void* stream);
int mmg_shift_finish(const int64_t* counts, const double* sums, const int64_t* cohort, int n_seg, int replicates,
                     double* stats, void* stream);
int mmg_shift_summary(const double* stats, int n_seg, int replicates, double* summary, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_SHIFT_H */
