// Feature-space selection (reference src/io_mimic.py filter_labs_for_cohort, src/preprocess.py process_diagnoses /
// process_medications; mmgnn/preprocess.py): which codes (labs, diagnoses, drugs) become nodes, and which event rows stay.
//   mmg_code_select   distinct patients and rows per code, the rank of every eligible code in (patients descending, code
//                     ascending) order, the selected codes (>= min_patient_count patients, the top_k first of the rank)
//                     and the kept rows: every counted row of a selected code, or the first row of each (patient, code)
//                     pair, in ascending row order.
//
// One stable LSD radix sort (radix_sort.h) of (code * n_patients + patient, row); ignored rows are filed under the
// sentinel key n_codes * n_patients behind every real one and are never used as an address.  The OR / AND of the keys are
// reduced while the keys are formed: the sort's skip words.  In the sorted order
//   a segment head (key differs from its predecessor) is the pair's first row -- the sort is stable, the values start as
//   0 .. n-1 -- so the heads of a code count its distinct patients;
//   a code's slice is found by two binary searches over the sorted keys, its row count is the slice's length and its
//   patient count the difference of the scanned head flags at the slice's ends.
// The codes are ranked by a second stable sort of (max_count - patients, code): code order breaks the ties.  The keep flag
// is formed per ROW (every row is written exactly once), scanned, and the kept rows are compacted in row order.
// Integer work throughout, no atomics on the data path: every output is exact and the same from call to call.
#include "common.h"
#include "radix_sort.h"

namespace {

constexpr int CS_NTHR = 256;

__global__ void k_cs_bits_init(unsigned long long* bits) {
  bits[0] = 0ull;          // OR of the keys
  bits[1] = ~0ull;         // AND
}

__global__ __launch_bounds__(CS_NTHR) void k_cs_keys(const int64_t* __restrict__ code, const int64_t* __restrict__ patient,
                                                     const uint8_t* __restrict__ valid, int64_t n, int64_t n_patients,
                                                     int64_t n_codes, uint64_t* __restrict__ keys,
                                                     int32_t* __restrict__ vals, unsigned long long* bits) {
  const int64_t e = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  uint64_t k = 0ull;
  if (e < n) {
    const int64_t c = code[e], p = patient[e];
    const bool ok = c >= 0 && c < n_codes && p >= 0 && p < n_patients && (!valid || valid[e] != 0);
    k = ok ? (uint64_t)(c * n_patients + p) : (uint64_t)(n_codes * n_patients);
    keys[e] = k;
    vals[e] = (int32_t)e;
  }
  uint64_t o = e < n ? k : 0ull, a = e < n ? k : ~0ull;
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    o |= (uint64_t)__shfl_xor((unsigned long long)o, s, WAVE);
    a &= (uint64_t)__shfl_xor((unsigned long long)a, s, WAVE);
  }
  // the words only gain (OR) / lose (AND) bits: a wave that a possibly stale read shows to add nothing skips the atomic
  if ((threadIdx.x & 63) == 0) {
    if (o & ~__atomic_load_n(&bits[0], __ATOMIC_RELAXED)) atomicOr(&bits[0], (unsigned long long)o);
    if (~a & __atomic_load_n(&bits[1], __ATOMIC_RELAXED)) atomicAnd(&bits[1], (unsigned long long)a);
  }
}

// flag[i] = 1 where sorted position i starts a (patient, code) pair; flag[n] = 0 so that the scan leaves the total there
__global__ __launch_bounds__(CS_NTHR) void k_cs_heads(const uint64_t* __restrict__ keys, int64_t n, uint64_t sentinel,
                                                      uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (i > n) return;
  uint32_t h = 0u;
  if (i < n) {
    const uint64_t k = keys[i];
    h = (k != sentinel && (i == 0 || keys[i - 1] != k)) ? 1u : 0u;
  }
  flag[i] = h;
}

__device__ __forceinline__ int64_t cs_lower_bound(const uint64_t* __restrict__ keys, int64_t n, uint64_t want) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// per code: rows = the length of its slice of the sorted keys, patients = the heads inside it; + the key of the rank sort
__global__ __launch_bounds__(CS_NTHR) void k_cs_counts(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ hpos,
                                                       int64_t n, int64_t n_patients, int64_t n_codes, int64_t min_count,
                                                       uint64_t max_count, int64_t* __restrict__ n_pat,
                                                       int64_t* __restrict__ n_rows, uint64_t* __restrict__ rkeys,
                                                       int32_t* __restrict__ rvals) {
  const int64_t c = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (c >= n_codes) return;
  const int64_t s = cs_lower_bound(keys, n, (uint64_t)(c * n_patients));
  const int64_t e = cs_lower_bound(keys, n, (uint64_t)((c + 1) * n_patients));     // c + 1 = n_codes: the sentinel
  const int64_t rows = e - s, pats = (int64_t)hpos[e] - (int64_t)hpos[s];          // s, e <= n: hpos has n + 1 entries
  n_rows[c] = rows;
  n_pat[c] = pats;
  const bool eligible = rows > 0 && pats >= min_count;
  rkeys[c] = eligible ? max_count - (uint64_t)pats : max_count + 1ull;             // pats <= max_count = min(n, n_patients)
  rvals[c] = (int32_t)c;
}

// n = 0: no row, no eligible code
__global__ __launch_bounds__(CS_NTHR) void k_cs_empty(int64_t n_codes, int64_t* __restrict__ n_pat,
                                                      int64_t* __restrict__ n_rows, int32_t* __restrict__ rank,
                                                      uint8_t* __restrict__ selected) {
  const int64_t c = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (c >= n_codes) return;
  n_pat[c] = 0;
  n_rows[c] = 0;
  rank[c] = -1;
  selected[c] = 0;
}

__global__ __launch_bounds__(CS_NTHR) void k_cs_rank(const uint64_t* __restrict__ rkeys, const int32_t* __restrict__ rvals,
                                                     int64_t n_codes, uint64_t max_count, int64_t top_k,
                                                     int32_t* __restrict__ rank, uint8_t* __restrict__ selected) {
  const int64_t j = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (j >= n_codes) return;
  const int32_t c = rvals[j];                                  // a permutation of 0 .. n_codes - 1
  const bool eligible = rkeys[j] <= max_count;
  rank[c] = eligible ? (int32_t)j : -1;
  selected[c] = (eligible && (top_k < 0 || j < top_k)) ? 1 : 0;
}

// MMG_SEL_ROWS_ALL: in row order, nothing of the sort is needed.  flag has n + 1 entries.
__global__ __launch_bounds__(CS_NTHR) void k_cs_keep_all(const int64_t* __restrict__ code, const int64_t* __restrict__ patient,
                                                         const uint8_t* __restrict__ valid, int64_t n, int64_t n_patients,
                                                         int64_t n_codes, const uint8_t* __restrict__ selected,
                                                         uint32_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (e > n) return;
  uint32_t k = 0u;
  if (e < n) {
    const int64_t c = code[e], p = patient[e];
    const bool ok = c >= 0 && c < n_codes && p >= 0 && p < n_patients && (!valid || valid[e] != 0);
    k = (ok && selected[c]) ? 1u : 0u;
  }
  flag[e] = k;
}

// MMG_SEL_ROWS_FIRST: over the sorted positions; the row of position i is vals[i] (each row once), a counted row's code is
// in range
__global__ __launch_bounds__(CS_NTHR) void k_cs_keep_first(const uint64_t* __restrict__ keys, const int32_t* __restrict__ vals,
                                                           const int64_t* __restrict__ code, int64_t n, uint64_t sentinel,
                                                           const uint8_t* __restrict__ selected,
                                                           uint32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (i > n) return;
  if (i == n) {
    flag[n] = 0u;
    return;
  }
  const uint64_t k = keys[i];
  const int32_t row = vals[i];                                 // in [0, n)
  const bool head = k != sentinel && (i == 0 || keys[i - 1] != k);
  flag[row] = (head && selected[code[row]]) ? 1u : 0u;
}

// pos = the exclusive scan of the n + 1 flags: row e is kept where pos steps, pos[n] is the count
__global__ __launch_bounds__(CS_NTHR) void k_cs_compact(const uint32_t* __restrict__ pos, int64_t n,
                                                        int32_t* __restrict__ out_rows) {
  const int64_t e = (int64_t)blockIdx.x * CS_NTHR + threadIdx.x;
  if (e >= n) return;
  const uint32_t p = pos[e];
  if (pos[e + 1] != p) out_rows[p] = (int32_t)e;              // p < the number of kept rows <= n
}

inline int cs_bits_of(uint64_t n_keys) {     // digits needed for keys in [0, n_keys)
  int bits = 1;
  while (bits < 64 && (1ull << bits) < n_keys) ++bits;
  return bits;
}

// the workspace, listed once: over a null base the carver only adds the sizes up
struct CsWs {
  unsigned long long* bits;
  RadixPairs<uint64_t> rows, codes;
  uint32_t *thist, *scr, *flag, *fscr;
};
size_t cs_carve(void* ws, int64_t n, int64_t n_codes, CsWs* w) {
  const RadixSizes rs = radix_sizes(n > n_codes ? n : n_codes);
  const size_t m = (size_t)n, k = (size_t)n_codes;
  MmgCarver c(ws);
  *w = CsWs{c.take<unsigned long long>(2),
            {c.take<uint64_t>(m), c.take<uint64_t>(m), c.take<int32_t>(m), c.take<int32_t>(m)},
            {c.take<uint64_t>(k), c.take<uint64_t>(k), c.take<int32_t>(k), c.take<int32_t>(k)},
            c.take<uint32_t>(rs.hist_elems), c.take<uint32_t>(rs.scratch_elems),
            c.take<uint32_t>(m + 1), c.take<uint32_t>(scan_scratch_elems(n + 1))};
  return c.need();
}

inline dim3 cs_grid(int64_t items) { return dim3((unsigned)((items + CS_NTHR - 1) / CS_NTHR)); }

}  // namespace

extern "C" size_t mmg_code_select_ws_bytes(int64_t n, int64_t n_codes) {
  CsWs w;
  return cs_carve(nullptr, n < 0 ? 0 : n, n_codes < 1 ? 1 : n_codes, &w);
}

extern "C" int mmg_code_select(const int64_t* code, const int64_t* patient, const uint8_t* valid, int64_t n,
                               int64_t n_patients, int64_t n_codes, int64_t min_patient_count, int64_t top_k,
                               int rows_mode, int64_t* n_patients_per_code, int64_t* n_rows_per_code, int32_t* rank,
                               uint8_t* selected, int32_t* out_rows, int64_t* n_out, void* ws, size_t ws_bytes,
                               void* stream) {
  MMG_CHECK_ARG(n >= 0 && n < INT32_MAX, "code_select: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_patients >= 1, "code_select: n_patients %lld < 1", (long long)n_patients);
  MMG_CHECK_ARG(n_codes >= 1, "code_select: n_codes %lld < 1", (long long)n_codes);
  MMG_CHECK_ARG(n_codes <= (INT64_MAX - 1) / n_patients,
                "code_select: n_codes %lld * n_patients %lld + 1 does not fit 63 bits", (long long)n_codes,
                (long long)n_patients);
  MMG_CHECK_ARG(n_patients < INT32_MAX, "code_select: n_patients %lld outside [1, 2^31)", (long long)n_patients);
  MMG_CHECK_ARG(n_codes < INT32_MAX, "code_select: n_codes %lld outside [1, 2^31)", (long long)n_codes);
  MMG_CHECK_ARG(rows_mode == MMG_SEL_ROWS_ALL || rows_mode == MMG_SEL_ROWS_FIRST, "code_select: rows_mode %d", rows_mode);
  MMG_CHECK_ARG(n_out, "code_select: n_out is null");
  MMG_CHECK_ARG(n_patients_per_code && n_rows_per_code && rank && selected,
                "code_select: null output (n_patients_per_code, n_rows_per_code, rank, selected)");
  MMG_CHECK_ARG(n == 0 || out_rows, "code_select: out_rows is null");
  MMG_CHECK_ARG(n == 0 || (code && patient), "code_select: null input (code, patient)");
  CsWs w;
  MMG_CHECK_WS("code_select", cs_carve(ws, n, n_codes, &w));
  *n_out = 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(CS_NTHR);
  if (n == 0) {
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n_codes, 0, 0, 0, k_cs_empty, cs_grid(n_codes), blk, 0, st, n_codes,
               n_patients_per_code, n_rows_per_code, rank, selected);
    MMG_CHECK_LAUNCH("code_select(empty)");
    return MMG_OK;
  }
  const uint64_t sentinel = (uint64_t)(n_codes * n_patients);
  const uint64_t max_count = (uint64_t)(n < n_patients ? n : n_patients);

  // ---- the rows by (code, patient), stable
  MMG_CHECK_HIP(mmg_zero_async(w.thist, radix_sizes(n > n_codes ? n : n_codes).hist_elems * 4, st),
                "code_select(zero)");                                                   // a skipped first pass
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, 2, 0, 0, 0, k_cs_bits_init, dim3(1), dim3(1), 0, st, w.bits);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_cs_keys, cs_grid(n), blk, 0, st, code, patient, valid, n, n_patients,
             n_codes, w.rows.keys, w.rows.vals, w.bits);
  MMG_CHECK_LAUNCH("code_select(keys)");
  const int row_passes = (cs_bits_of(sentinel + 1ull) + 7) / 8;
  for (int ps = 0; ps < row_passes; ++ps) radix_pass<true>(w.rows, n, 8 * ps, w.bits, w.thist, w.scr, st);
  MMG_CHECK_LAUNCH("code_select(sort)");

  // ---- counts per code
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_cs_heads, cs_grid(n + 1), blk, 0, st, w.rows.keys, n, sentinel, w.flag);
  exclusive_scan_u32(w.flag, n + 1, w.fscr, st);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n_codes, 0, 0, 0, k_cs_counts, cs_grid(n_codes), blk, 0, st, w.rows.keys, w.flag, n,
             n_patients, n_codes, min_patient_count, max_count, n_patients_per_code, n_rows_per_code, w.codes.keys,
             w.codes.vals);
  MMG_CHECK_LAUNCH("code_select(counts)");

  // ---- rank: (patients descending, code ascending)
  const int rank_passes = (cs_bits_of(max_count + 2ull) + 7) / 8;
  for (int ps = 0; ps < rank_passes; ++ps) radix_pass<true>(w.codes, n_codes, 8 * ps, nullptr, w.thist, w.scr, st);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n_codes, 0, 0, 0, k_cs_rank, cs_grid(n_codes), blk, 0, st, w.codes.keys, w.codes.vals,
             n_codes, max_count, top_k, rank, selected);
  MMG_CHECK_LAUNCH("code_select(rank)");

  // ---- the kept rows, ascending
  if (rows_mode == MMG_SEL_ROWS_ALL)
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_cs_keep_all, cs_grid(n + 1), blk, 0, st, code, patient, valid, n,
               n_patients, n_codes, selected, w.flag);
  else
    MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 1, k_cs_keep_first, cs_grid(n + 1), blk, 0, st, w.rows.keys, w.rows.vals, code,
               n, sentinel, selected, w.flag);
  exclusive_scan_u32(w.flag, n + 1, w.fscr, st);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_cs_compact, cs_grid(n), blk, 0, st, w.flag, n, out_rows);
  MMG_CHECK_LAUNCH("code_select(compact)");
  uint32_t count = 0;
  MMG_CHECK_HIP(hipMemcpyAsync(&count, w.flag + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "code_select(count)");
  MMG_CHECK_HIP(hipStreamSynchronize(st), "code_select(sync)");        // the count sizes the caller's view of out_rows
  *n_out = (int64_t)count;
  return MMG_OK;
}
