// Device graph build (reference src/graph_build.py NodeIndexer :34-97 and :163-173, create_patient_*_edges :476-586, the
// flip(0) reverse relations :222; mmgnn/graph_build.py build_graph_from_events): the step between the preprocessed
// event tensors and mmg_csr_build.
//   mmg_first_seen_index   code -> node index in the order of the codes' first counted rows, and the inverse
//   mmg_edge_build         one edge per event row whose two codes have an index, row order kept, + the flipped relation
//                          and the fp32 edge values
//
// First-seen order without a sort: first_row[c] = the smallest counted row that carries c (integer atomicMin on a table a
// kernel filled with INT32_MAX: a minimum does not depend on the order it is taken in), row e is a HEAD where
// first_row[code[e]] == e, and the index of a code is the exclusive scan (scan.h) of the head flags at its head.  A
// vocabulary of 50 labs puts 6 M rows onto 50 addresses, so a workgroup reduces into LDS first when the table fits there,
// and no atomic is issued where a possibly stale read already shows a row that is not larger (the table only decreases:
// a stale value is an upper bound, skipping on it is always right).  The edges are flags, the same scan and a scatter
// in which every output is written once.  Integer work throughout; the one conversion, fp64 -> fp32 of the edge values,
// is a single round-to-nearest-even per element.  Every output is exact and the same from call to call.
#include "common.h"
#include "scan.h"

namespace {

constexpr int GB_NTHR = 256;
constexpr int GB_BINS = 4096;            // codes a workgroup pre-reduces in LDS (16 KiB)
constexpr int GB_ROWS_PER_THREAD = 8;    // of k_fs_min: the flush of the LDS table is amortised
constexpr int GB_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(GB_NTHR) void k_fs_fill(int64_t n_codes, int32_t* __restrict__ first_row,
                                                     int32_t* __restrict__ index_of_code) {
  const int64_t c = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x;
  if (c >= n_codes) return;
  first_row[c] = INT32_MAX;
  index_of_code[c] = -1;
}

__device__ __forceinline__ bool fs_counted(const int64_t* __restrict__ code, const uint8_t* __restrict__ valid, int64_t e,
                                           int64_t n_codes, int64_t* c) {
  *c = code[e];
  return *c >= 0 && *c < n_codes && (!valid || valid[e] != 0);
}

__global__ __launch_bounds__(GB_NTHR) void k_fs_min(const int64_t* __restrict__ code, const uint8_t* __restrict__ valid,
                                                    int64_t n, int64_t n_codes, int32_t* first_row) {
  __shared__ int32_t h[GB_BINS];
  const bool local = n_codes <= GB_BINS;
  if (local) {
    for (int i = threadIdx.x; i < (int)n_codes; i += GB_NTHR) h[i] = INT32_MAX;
    __syncthreads();
  }
  // a thread's rows ascend: after its first row of a code every later one is skipped on the read alone
  for (int64_t e = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x; e < n; e += (int64_t)gridDim.x * GB_NTHR) {
    int64_t c;
    if (!fs_counted(code, valid, e, n_codes, &c)) continue;          // c in [0, n_codes) from here on
    if (local) {
      if (__atomic_load_n(&h[c], __ATOMIC_RELAXED) > (int32_t)e) atomicMin(&h[c], (int32_t)e);
    } else {
      if (__atomic_load_n(&first_row[c], __ATOMIC_RELAXED) > (int32_t)e) atomicMin(&first_row[c], (int32_t)e);
    }
  }
  if (local) {
    __syncthreads();
    for (int i = threadIdx.x; i < (int)n_codes; i += GB_NTHR) {
      const int32_t m = h[i];
      if (m != INT32_MAX && __atomic_load_n(&first_row[i], __ATOMIC_RELAXED) > m) atomicMin(&first_row[i], m);
    }
  }
}

// flag[e] = 1 where row e is the first counted row of its code; flag[n] = 0 so that the scan leaves the total there
__global__ __launch_bounds__(GB_NTHR) void k_fs_heads(const int64_t* __restrict__ code, const uint8_t* __restrict__ valid,
                                                      int64_t n, int64_t n_codes, const int32_t* __restrict__ first_row,
                                                      uint32_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x;
  if (e > n) return;
  uint32_t f = 0u;
  if (e < n) {
    int64_t c;
    if (fs_counted(code, valid, e, n_codes, &c)) f = first_row[c] == (int32_t)e ? 1u : 0u;
  }
  flag[e] = f;
}

// pos = the exclusive scan of the n + 1 flags.  A head's code is counted, so it is in range; every code has one head:
// each entry of both tables is written at most once.
__global__ __launch_bounds__(GB_NTHR) void k_fs_index(const int64_t* __restrict__ code, const uint32_t* __restrict__ pos,
                                                      int64_t n, int32_t* __restrict__ index_of_code,
                                                      int64_t* __restrict__ code_of_index) {
  const int64_t e = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x;
  if (e >= n) return;
  const uint32_t p = pos[e];
  if (pos[e + 1] == p) return;
  const int64_t c = code[e];
  index_of_code[c] = (int32_t)p;             // p < the number of codes seen <= min(n, n_codes)
  code_of_index[p] = c;
}

__device__ __forceinline__ bool eb_kept(const int64_t* __restrict__ patient, const int64_t* __restrict__ item, int64_t e,
                                        const int32_t* __restrict__ patient_index, int64_t n_patient_codes,
                                        const int32_t* __restrict__ item_index, int64_t n_item_codes, int32_t* pi,
                                        int32_t* ii) {
  const int64_t p = patient[e], i = item[e];
  if (p < 0 || p >= n_patient_codes || i < 0 || i >= n_item_codes) return false;
  *pi = patient_index[p];
  *ii = item_index[i];
  return *pi >= 0 && *ii >= 0;
}

__global__ __launch_bounds__(GB_NTHR) void k_eb_flags(const int64_t* __restrict__ patient, const int64_t* __restrict__ item,
                                                      int64_t n, const int32_t* __restrict__ patient_index,
                                                      int64_t n_patient_codes, const int32_t* __restrict__ item_index,
                                                      int64_t n_item_codes, uint32_t* __restrict__ flag) {
  const int64_t e = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x;
  if (e > n) return;
  int32_t pi, ii;
  flag[e] = (e < n && eb_kept(patient, item, e, patient_index, n_patient_codes, item_index, n_item_codes, &pi, &ii)) ? 1u : 0u;
}

// the k-th kept row writes column k of fwd (and rev, attr): k < the number of kept rows <= n <= ld
__global__ __launch_bounds__(GB_NTHR) void k_eb_scatter(const int64_t* __restrict__ patient, const int64_t* __restrict__ item,
                                                        const double* __restrict__ value, int64_t n,
                                                        const int32_t* __restrict__ patient_index, int64_t n_patient_codes,
                                                        const int32_t* __restrict__ item_index, int64_t n_item_codes,
                                                        const uint32_t* __restrict__ pos, int64_t* __restrict__ fwd,
                                                        int64_t* __restrict__ rev, int64_t ld, float* __restrict__ attr) {
  const int64_t e = (int64_t)blockIdx.x * GB_NTHR + threadIdx.x;
  if (e >= n) return;
  const uint32_t k = pos[e];
  if (pos[e + 1] == k) return;
  int32_t pi, ii;
  if (!eb_kept(patient, item, e, patient_index, n_patient_codes, item_index, n_item_codes, &pi, &ii)) return;   // (as flagged)
  fwd[k] = (int64_t)pi;
  fwd[ld + k] = (int64_t)ii;
  if (rev) {
    rev[k] = (int64_t)ii;
    rev[ld + k] = (int64_t)pi;
  }
  if (attr) attr[k] = (float)value[e];       // v_cvt_f32_f64: one round-to-nearest-even
}

// the workspaces, listed once: over a null base the carver only adds the sizes up
struct FsWs { int32_t* first_row; uint32_t *flag, *fscr; };
size_t fs_carve(void* ws, int64_t n, int64_t n_codes, FsWs* w) {
  MmgCarver c(ws);
  *w = FsWs{c.take<int32_t>((size_t)n_codes), c.take<uint32_t>((size_t)n + 1), c.take<uint32_t>(scan_scratch_elems(n + 1))};
  return c.need();
}
struct EbWs { uint32_t *flag, *fscr; };
size_t eb_carve(void* ws, int64_t n, EbWs* w) {
  MmgCarver c(ws);
  *w = EbWs{c.take<uint32_t>((size_t)n + 1), c.take<uint32_t>(scan_scratch_elems(n + 1))};
  return c.need();
}

inline dim3 gb_grid(int64_t items) { return dim3((unsigned)((items + GB_NTHR - 1) / GB_NTHR)); }

}  // namespace

extern "C" size_t mmg_first_seen_index_ws_bytes(int64_t n, int64_t n_codes) {
  FsWs w;
  return fs_carve(nullptr, n < 0 ? 0 : n, n_codes < 1 ? 1 : n_codes, &w);
}

extern "C" int mmg_first_seen_index(const int64_t* code, const uint8_t* valid, int64_t n, int64_t n_codes,
                                    int32_t* index_of_code, int64_t* code_of_index, int64_t* n_nodes, void* ws,
                                    size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 0 && n < INT32_MAX, "first_seen_index: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_codes >= 1 && n_codes < INT32_MAX, "first_seen_index: n_codes %lld outside [1, 2^31)",
                (long long)n_codes);
  MMG_CHECK_ARG(n_nodes, "first_seen_index: n_nodes is null");
  MMG_CHECK_ARG(index_of_code, "first_seen_index: index_of_code is null");
  MMG_CHECK_ARG(n == 0 || (code && code_of_index), "first_seen_index: null buffer (code, code_of_index)");
  FsWs w;
  MMG_CHECK_WS("first_seen_index", fs_carve(ws, n, n_codes, &w));
  *n_nodes = 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(GB_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n_codes, 0, 0, 0, k_fs_fill, gb_grid(n_codes), blk, 0, st, n_codes, w.first_row,
             index_of_code);
  MMG_CHECK_LAUNCH("first_seen_index(fill)");
  if (n == 0) return MMG_OK;
  int64_t nb = (n + (int64_t)GB_NTHR * GB_ROWS_PER_THREAD - 1) / ((int64_t)GB_NTHR * GB_ROWS_PER_THREAD);
  if (nb > GB_MAX_BLOCKS) nb = GB_MAX_BLOCKS;
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_fs_min, dim3((unsigned)nb), blk, 0, st, code, valid, n, n_codes,
             w.first_row);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 1, k_fs_heads, gb_grid(n + 1), blk, 0, st, code, valid, n, n_codes,
             w.first_row, w.flag);
  exclusive_scan_u32(w.flag, n + 1, w.fscr, st);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 2, k_fs_index, gb_grid(n), blk, 0, st, code, w.flag, n, index_of_code,
             code_of_index);
  MMG_CHECK_LAUNCH("first_seen_index");
  uint32_t count = 0;
  MMG_CHECK_HIP(hipMemcpyAsync(&count, w.flag + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "first_seen_index(count)");
  MMG_CHECK_HIP(hipStreamSynchronize(st), "first_seen_index(sync)");     // the count sizes the caller's view of code_of_index
  *n_nodes = (int64_t)count;
  return MMG_OK;
}

extern "C" size_t mmg_edge_build_ws_bytes(int64_t n) {
  EbWs w;
  return eb_carve(nullptr, n < 0 ? 0 : n, &w);
}

extern "C" int mmg_edge_build(const int64_t* patient, const int64_t* item, const double* value, int64_t n,
                              const int32_t* patient_index, int64_t n_patient_codes, const int32_t* item_index,
                              int64_t n_item_codes, int64_t* fwd, int64_t* rev, int64_t ld, float* attr, int64_t* n_edges,
                              void* ws, size_t ws_bytes, void* stream) {
  MMG_CHECK_ARG(n >= 0 && n < INT32_MAX, "edge_build: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_patient_codes >= 1 && n_patient_codes < INT32_MAX, "edge_build: n_patient_codes %lld outside [1, 2^31)",
                (long long)n_patient_codes);
  MMG_CHECK_ARG(n_item_codes >= 1 && n_item_codes < INT32_MAX, "edge_build: n_item_codes %lld outside [1, 2^31)",
                (long long)n_item_codes);
  MMG_CHECK_ARG(ld >= n, "edge_build: ld %lld < n %lld", (long long)ld, (long long)n);
  MMG_CHECK_ARG(n_edges, "edge_build: n_edges is null");
  MMG_CHECK_ARG(patient_index && item_index, "edge_build: null index table (patient_index, item_index)");
  MMG_CHECK_ARG(n == 0 || (patient && item && fwd), "edge_build: null buffer (patient, item, fwd)");
  MMG_CHECK_ARG(n == 0 || !attr || value, "edge_build: attr without value");
  EbWs w;
  MMG_CHECK_WS("edge_build", eb_carve(ws, n, &w));
  *n_edges = 0;
  if (n == 0) return MMG_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 blk(GB_NTHR);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 0, k_eb_flags, gb_grid(n + 1), blk, 0, st, patient, item, n, patient_index,
             n_patient_codes, item_index, n_item_codes, w.flag);
  exclusive_scan_u32(w.flag, n + 1, w.fscr, st);
  MMG_LAUNCH(MMG_PROBE_ELEMENTWISE, n, 0, 0, 1, k_eb_scatter, gb_grid(n), blk, 0, st, patient, item, value, n,
             patient_index, n_patient_codes, item_index, n_item_codes, w.flag, fwd, rev, ld, attr);
  MMG_CHECK_LAUNCH("edge_build");
  uint32_t count = 0;
  MMG_CHECK_HIP(hipMemcpyAsync(&count, w.flag + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "edge_build(count)");
  MMG_CHECK_HIP(hipStreamSynchronize(st), "edge_build(sync)");           // the count sizes the caller's views
  *n_edges = (int64_t)count;
  return MMG_OK;
}
