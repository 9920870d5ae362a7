// CSR construction for the edge_index contract of src/graph_build.py (reference) --
// SURVEY.md section 8 row a2.  Integer-exact with torch.sort(stable=True)+bincount+cumsum.
//
// Stable LSD radix sort (radix_sort.h) of (key = edge_index[sort_row][e], value = e): deterministic, O(E * ceil(bits/8)).
#include "common.h"
#include "radix_sort.h"

namespace {

constexpr int NTHR = 256;

// ---------------------------------------------------------------- sort keys
// A key outside [0, n_rows) is never used as an address: it is filed under the sentinel bucket n_rows, i.e. it sorts
// behind the last row and rowptr[n_rows] < n_edges tells the caller (include/mmgnn.h).
__global__ __launch_bounds__(NTHR) void k_prep(const int64_t* __restrict__ key_src, uint32_t* keys,
                                               int32_t* vals, uint32_t* counts, int64_t n, int64_t n_rows) {
  const int64_t e = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (e < n) {
    const int64_t k64 = key_src[e];
    const uint32_t k = (k64 < 0 || k64 >= n_rows) ? (uint32_t)n_rows : (uint32_t)k64;
    keys[e] = k;
    vals[e] = (int32_t)e;
    atomicAdd(&counts[k], 1u);   // integer histogram -> rowptr (order-independent result)
  }
}

__global__ __launch_bounds__(NTHR) void k_finish(const int64_t* __restrict__ other, const int32_t* __restrict__ perm,
                                                 int32_t* __restrict__ col, int64_t n) {
  const int64_t k = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (k < n) col[k] = (int32_t)other[perm[k]];
}

__global__ __launch_bounds__(NTHR) void k_row_degree(const int32_t* __restrict__ rowptr, int64_t n, int32_t* deg,
                                                     float* inv) {
  const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i < n) {
    const int32_t d = rowptr[i + 1] - rowptr[i];
    if (deg) deg[i] = d;
    if (inv) inv[i] = 1.0f / (float)(d > 1 ? d : 1);
  }
}
// column histogram: per-workgroup counts in LDS (the vocabularies have 50..200 entries: global atomics onto so few
// counters serialise -- 2.9 ms for 6 M edges), one global add per non-empty bin and workgroup at the end
constexpr int CC_BINS = 4096;
__global__ __launch_bounds__(NTHR) void k_col_count(const int32_t* __restrict__ col, int64_t n, int32_t* cnt,
                                                    int n_cols) {
  __shared__ int h[CC_BINS];
  const bool local = n_cols <= CC_BINS;
  if (local) {
    for (int i = threadIdx.x; i < n_cols; i += NTHR) h[i] = 0;
    __syncthreads();
  }
  for (int64_t k = (int64_t)blockIdx.x * NTHR + threadIdx.x; k < n; k += (int64_t)gridDim.x * NTHR) {
    const int c = col[k];
    if ((unsigned)c >= (unsigned)n_cols) continue;           // never index outside the table
    if (local) atomicAdd(&h[c], 1);
    else atomicAdd(&cnt[c], 1);
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < n_cols; i += NTHR)
      if (h[i]) atomicAdd(&cnt[i], h[i]);
  }
}
__global__ __launch_bounds__(NTHR) void k_inv_count(const int32_t* __restrict__ cnt, int64_t n, float* inv) {
  const int64_t i = (int64_t)blockIdx.x * NTHR + threadIdx.x;
  if (i < n) inv[i] = 1.0f / (float)(cnt[i] > 1 ? cnt[i] : 1);
}

inline int key_passes(int64_t n_rows) {
  int bits = 1;
  while (((int64_t)1 << bits) < n_rows) ++bits;
  return (bits + 7) / 8;
}

// the workspace, listed once: over a null base the carver only adds the sizes up
struct CsrWs { RadixPairs<uint32_t> kv; uint32_t *thist, *scr1, *scr2; };   // kv.vals_alt: the caller's perm
size_t csr_carve(void* ws, int64_t n_edges, int64_t n_rows, int32_t* perm, CsrWs* w) {
  const RadixSizes rs = radix_sizes(n_edges);
  const size_t m = (size_t)n_edges;
  MmgCarver c(ws);                   // (a braced list is evaluated left to right)
  *w = CsrWs{{c.take<uint32_t>(m), c.take<uint32_t>(m), c.take<int32_t>(m), perm}, c.take<uint32_t>(rs.hist_elems),
             c.take<uint32_t>(rs.scratch_elems), c.take<uint32_t>(scan_scratch_elems(n_rows + 1))};
  return c.need();
}

}  // namespace

extern "C" size_t mmg_csr_build_ws_bytes(int64_t n_edges, int64_t n_rows) {
  CsrWs w;
  return (n_edges < 0 || n_rows < 0) ? 0 : csr_carve(nullptr, n_edges, n_rows, nullptr, &w);
}

extern "C" int mmg_csr_build(const int64_t* edge_index, int64_t n_edges, int64_t n_rows, int sort_row,
                             int32_t* rowptr, int32_t* col, int32_t* perm, void* ws, size_t ws_bytes,
                             void* stream) {
  MMG_CHECK_ARG(n_edges >= 0 && n_rows >= 0, "csr_build: negative size");
  MMG_CHECK_ARG(n_edges < 2147483647LL && n_rows < 2147483647LL, "csr_build: int32 index range exceeded");
  MMG_CHECK_ARG(sort_row == 0 || sort_row == 1, "csr_build: sort_row must be 0 or 1");
  MMG_CHECK_ARG(rowptr, "csr_build: rowptr is null");
  MMG_CHECK_ARG(n_edges == 0 || (edge_index && col && perm && ws), "csr_build: null buffer");
  CsrWs w;
  MMG_CHECK_WS("csr_build", csr_carve(ws, n_edges, n_rows, perm, &w));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* cnt = (uint32_t*)rowptr;   // histogram is built in place, then scanned into rowptr
  MMG_CHECK_HIP(mmg_zero_async(cnt, (size_t)(n_rows + 1) * 4, st), "csr_build(memset)");
  if (n_edges == 0) {
    MMG_CHECK_LAUNCH("csr_build(memset)");
    return MMG_OK;
  }
  const int passes = key_passes(n_rows + 1);        // + the sentinel bucket of out-of-range keys
  const unsigned eb = (unsigned)((n_edges + NTHR - 1) / NTHR);
  const int64_t* key_src = edge_index + (int64_t)sort_row * n_edges;
  const int64_t* oth_src = edge_index + (int64_t)(1 - sort_row) * n_edges;

  // the last pass must land in `perm`: an odd pass count starts from the workspace's values, an even one from perm
  if (passes % 2 == 0) std::swap(w.kv.vals, w.kv.vals_alt);

  hipLaunchKernelGGL(k_prep, dim3(eb), dim3(NTHR), 0, st, key_src, w.kv.keys, w.kv.vals, cnt, n_edges, n_rows);
  exclusive_scan_u32(cnt, n_rows + 1, w.scr2, st);   // rowptr = exclusive scan of the row histogram

  for (int ps = 0; ps < passes; ++ps) radix_pass<false>(w.kv, n_edges, 8 * ps, nullptr, w.thist, w.scr1, st);
  // w.kv.vals == perm here
  hipLaunchKernelGGL(k_finish, dim3(eb), dim3(NTHR), 0, st, oth_src, perm, col, n_edges);
  MMG_CHECK_LAUNCH("csr_build");
  return MMG_OK;
}

extern "C" int mmg_row_degree(const int32_t* rowptr, int64_t n_rows, int32_t* deg, float* inv_deg, void* stream) {
  MMG_CHECK_ARG(n_rows >= 0 && rowptr, "row_degree: bad args");
  if (n_rows == 0) return MMG_OK;
  hipLaunchKernelGGL(k_row_degree, dim3((unsigned)((n_rows + NTHR - 1) / NTHR)), dim3(NTHR), 0,
                     (hipStream_t)stream, rowptr, n_rows, deg, inv_deg);
  MMG_CHECK_LAUNCH("row_degree");
  return MMG_OK;
}

extern "C" int mmg_col_degree(const int32_t* col, int64_t n_edges, int64_t n_cols, int32_t* cnt, float* inv_cnt,
                              void* stream) {
  MMG_CHECK_ARG(n_edges >= 0 && n_cols >= 0 && n_cols < 2147483647LL && cnt, "col_degree: bad args");
  hipStream_t st = (hipStream_t)stream;
  if (n_cols > 0) MMG_CHECK_HIP(mmg_zero_async(cnt, (size_t)n_cols * 4, st), "col_degree(memset)");
  if (n_edges > 0 && n_cols > 0) {
    int64_t nb = (n_edges + NTHR * 8 - 1) / (NTHR * 8);      // >= 8 edges per thread: the flush is amortised
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(k_col_count, dim3((unsigned)nb), dim3(NTHR), 0, st, col, n_edges, cnt, (int)n_cols);
  }
  if (n_cols > 0 && inv_cnt)
    hipLaunchKernelGGL(k_inv_count, dim3((unsigned)((n_cols + NTHR - 1) / NTHR)), dim3(NTHR), 0, st, cnt, n_cols, inv_cnt);
  MMG_CHECK_LAUNCH("col_degree");
  return MMG_OK;
}
