/* C ABI of libmmgnn_boot.so: patient-cluster bootstrap intervals of the evaluation metrics (csrc/boot.hip,
 * mmgnn/bootstrap.py).  A library of its own beside libmmgnn.so (include/mmgnn.h), whose conventions it keeps: return
 * codes MMG_OK / MMG_E_ARG / MMG_E_WS / MMG_E_LAUNCH, the error text through mmg_last_error() of libmmgnn.so, a
 * workspace as the three parameters ws, ws_bytes, stream, a *_ws_bytes companion per call that takes one. */
#ifndef MMGNN_BOOT_H
#define MMGNN_BOOT_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * The weights.  Replicate b (1 .. replicates) gives unit u (0 .. n_units - 1) the integer weight
 *     k_b   = mmg_rng_key(seed, MMG_BOOT_SITE + b)
 *     w0    = the first word of mmg_rng_group(k_b, u >> 1)        (the second word is not used)
 *     field = (u & 1) ? w0 >> 16 : w0 & 0xFFFF
 *     w     = #{ j : field >= T[j] },  T = {24109, 48219, 60273, 64292, 65296, 65497, 65531, 65535}
 * T[j] = round(65536 * PoissonCDF(j; 1)); the sum of 65536 - T[j] is 65536, so over the 65,536 field values the weight has
 * mean exactly 1 (variance 131070 / 65536 - 1, largest value 8): the Poisson(1) bootstrap on a 16-bit grid.  Replicate 0
 * is the sample itself: every weight is 1.  The numpy restatement in mmgnn/bootstrap.py is the definition.
 *
 * mmg_boot_sums: pred, target (and, with_b != 0, pred_b: a second predictor on the same pairs; ignored otherwise) fp32
 *   [n]; unit, seg int64 (index_bytes 8) or int32 (4) [n].  A pair is left out of every replicate and counted in dropped (int64 [3]) under the
 *   FIRST of: seg outside [0, n_seg); unit outside [0, n_units); a NaN in pred, target or pred_b.  Per pair, as
 *   mmg_seg_metrics forms them: e = t - p in fp32, then the terms 1, |e| (fp32), (double)e * (double)e, t, (double)t *
 *   (double)t, |e / t| in fp32 and 1 for t != 0 (else both 0); with pred_b also |e_b|, e_b^2, |e_b / t|.
 *   sums (fp64 [replicates + 1][n_seg][F], F = 7 or 10 with pred_b) = per replicate and segment the sum of weight * term.
 *   Every weighted term is exact in fp64 (at most 52 significant bits), so only the ORDER of the additions matters, and it
 *   is fixed: the kept pairs are brought into segment order by a stable radix sort (ties: ascending pair position) and cut
 *   into chunks of MMG_BOOT_CHUNK consecutive sorted pairs.  The sum of a segment inside one chunk is taken left to right
 *   from 0; the sums of a segment that spans several chunks are then added in chunk order from 0.  Neither depends on the
 *   launch grid; there is no floating-point atomic (the dropped counters are integer atomics).  The counts (fields 0 and
 *   6) are integers below 2^53 and exact.  A workgroup serves MMG_BOOT_RB replicates of one chunk, one per thread.
 *   0 <= n < 2^31, 1 <= n_seg <= MMG_BOOT_MAX_SEG, 0 <= n_units < 2^31, 1 <= replicates <= MMG_BOOT_MAX_REPLICATES.
 * mmg_boot_metrics: sums -> metrics (fp64 [replicates + 1][n_seg + 1][M]); row n_seg is all segments together, its sums
 *   added in segment order from 0.  M = 4: mae, rmse, r2, mape; with_b != 0: M = 12, the four of pred, the four of pred_b,
 *   and the differences pred - pred_b (paired: both are taken under the same weights).  The rules, each operation rounded
 *   in fp64 on its own (no fused multiply-add):  n <= 0: all NaN;  mae = s_abs / n;  rmse = sqrt(s_sq / n);
 *   ss_tot = s_t2 - s_t * s_t / n;  r2 = NaN for n < 2, 1 for s_sq == 0, 1 - s_sq / ss_tot for
 *   ss_tot > 1e-12 * max(s_t2, 1e-300), else 0;  mape = s_ape / n_nz * 100, NaN for n_nz <= 0.
 * mmg_boot_summary: metrics -> summary (fp64 [n_seg + 1][M][MMG_BOOT_SUMMARY_FIELDS]) over the FINITE values x_b of
 *   replicates b = 1 .. replicates of every (row, metric):
 *     0 the estimate (replicate 0, whatever it is)   1 their mean   2 their standard deviation (two passes, ddof = 1; NaN
 *     below two values)   3, 4 numpy.percentile(x, p) under the "linear" rule at p = 100 * ((1 - confidence) / 2) and
 *     100 * ((1 + confidence) / 2)   5 the number of finite values   6 the share of them below zero
 *   Fields 1 - 4 and 6 are NaN without a finite value.  Sums: thread t of the 256 adds the finite replicates t + 1,
 *   t + 257, ... in that order, the 64 lanes of a wave are added by a fixed butterfly, the four waves in wave order.  The
 *   percentile, with q = p / 100 and m finite values sorted ascending x[0 .. m):  v = (m - 1) * q;
 *   v >= m - 1: x[m - 1];  v < 0: x[0];  else i = floor(v), g = v - i, d = x[i + 1] - x[i],
 *   value = g >= 0.5 ? x[i + 1] - d * (1 - g) : x[i] + d * g -- the form mmg_robust_sums documents, in fp64.
 * Every argument is checked on the host before anything is enqueued (MMG_E_ARG; a short or missing workspace
 * MMG_E_WS).  No call synchronises with the host, allocates, uses a memset node or a floating-point atomic: each one can
 * be captured into a hipGraph and replayed, and its results are bitwise the same from run to run.  n = 0 is valid.
 * ------------------------------------------------------------------------------------- */
#define MMG_BOOT_SITE 1112493908      /* 0x424F4F54, "BOOT" */
#define MMG_BOOT_MAX_REPLICATES 4096
#define MMG_BOOT_MAX_SEG 2048
#define MMG_BOOT_CHUNK 4096          /* C: sorted pairs per chunk */
#define MMG_BOOT_RB 256              /* RB: replicates per workgroup, one per thread */
#define MMG_BOOT_DROP_KINDS 3
#define MMG_BOOT_FIELDS 7
#define MMG_BOOT_FIELDS_B 10
#define MMG_BOOT_METRICS 4
#define MMG_BOOT_METRICS_B 12
#define MMG_BOOT_SUMMARY_FIELDS 7
size_t mmg_boot_sums_ws_bytes(int64_t n, int n_seg, int replicates, int with_b);      /* 0 for an unsupported shape */
int mmg_boot_sums(const float* pred, const float* target, const float* pred_b, int with_b, const void* unit,
                  const void* seg, int index_bytes, int64_t n, int64_t n_units, int n_seg, int replicates, uint64_t seed,
                  double* sums, int64_t* dropped, void* ws, size_t ws_bytes, void* stream);
int mmg_boot_metrics(const double* sums, int n_seg, int replicates, int with_b, double* metrics, void* stream);
int mmg_boot_summary(const double* metrics, int n_seg, int replicates, int with_b, double confidence, double* summary,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MMGNN_BOOT_H */
