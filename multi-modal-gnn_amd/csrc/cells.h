// What conformal.hip, stack.hip and boot.hip share around the cells of a (patient, lab) pair: the bounds-checked index
// load, the degree bins and the cell of a pair (lab x degree bin: the cells of include/mmgnn_conformal.h), and the host
// check of a call that names cells.  The sorted pair list itself is segsort.h, which this header includes.  Only for the
// satellite libraries: no source of libmmgnn.so includes it.
#pragma once
#include "common.h"
#include "segsort.h"
#include "../../include/mmgnn_conformal.h"
#include <limits.h>

// p[i] as an index below limit; -1 for one outside [0, limit)
template <class IT>
__device__ __forceinline__ int cell_index(const IT* __restrict__ p, int64_t i, int64_t limit) {
  const int64_t v = (int64_t)p[i];
  return v >= 0 && v < limit ? (int)v : -1;
}

struct CellEdges {
  double e[MMG_CF_MAX_BINS + 1];
};
// the bin [e[b], e[b + 1]) of degree d; -1: in none
__device__ __forceinline__ int cell_bin(int d, const CellEdges& ed, int B) {
  const double dd = (double)d;
  int b = -1;
  for (int j = 0; j < B; ++j)
    if (dd >= ed.e[j] && dd < ed.e[j + 1]) b = j;
  return b;
}
// the cell of a pair; -1 - kind for a pair without one (kind 0: lab, 1: patient, 2: degree in no bin)
template <class IT>
__device__ __forceinline__ int pair_cell(const IT* __restrict__ patient, const IT* __restrict__ lab, int64_t i, int L,
                                         const int32_t* __restrict__ deg, int64_t n_pat, const CellEdges& ed, int B) {
  const int l = cell_index(lab, i, L);
  if (l < 0) return -1;
  const int p = cell_index(patient, i, n_pat);
  if (p < 0) return -2;
  const int b = cell_bin(deg[p], ed, B);
  return b < 0 ? -3 : l * B + b;
}

// the shape of a call over n pairs (or rows) in L labs x B degree bins; fills ed.  The caller's own null-pointer checks
// come after it.
inline int cells_check(const char* what, int index_bytes, int64_t n, int L, int64_t n_pat, const double* edges, int B,
                       CellEdges* ed) {
  MMG_CHECK_ARG(n >= 0 && n <= INT32_MAX, "%s: n %lld outside [0, 2^31)", what, (long long)n);
  MMG_CHECK_ARG(L >= 1 && L <= MMG_CF_MAX_LABS, "%s: %d labs outside [1, %d]", what, L, MMG_CF_MAX_LABS);
  MMG_CHECK_ARG(B >= 1 && B <= MMG_CF_MAX_BINS, "%s: %d degree bins outside [1, %d]", what, B, MMG_CF_MAX_BINS);
  MMG_CHECK_ARG((int64_t)L * B <= MMG_CF_MAX_CELLS, "%s: %d labs x %d bins, at most %d cells", what, L, B, MMG_CF_MAX_CELLS);
  MMG_CHECK_ARG(index_bytes == 4 || index_bytes == 8, "%s: indices of %d bytes (int32 or int64)", what, index_bytes);
  MMG_CHECK_ARG(n_pat >= 0 && n_pat <= INT32_MAX, "%s: %lld patients outside [0, 2^31)", what, (long long)n_pat);
  MMG_CHECK_ARG(edges, "%s: null bin edges", what);
  for (int j = 0; j <= B; ++j) {
    MMG_CHECK_ARG(edges[j] == edges[j] && (j == 0 || edges[j] > edges[j - 1]), "%s: bin edges must be ascending (edge %d)",
                  what, j);
    ed->e[j] = edges[j];
  }
  return MMG_OK;
}
