// The fp64 slab Gram: sum over rows r of a(r, .)^T b(r, .) for every column pair of a tall matrix, products and sums in
// fp64 on v_mfma_f64_16x16x4_f64 -- the skeleton of k_pca_gram (pca.hip), k_as_moments (assoc.hip) and k_ch_moments
// (chain.hip).  The rows are cut into slabs (gram64_plan); the grid is (64 x 64 block pairs of the upper block triangle,
// slabs).  A workgroup walks its slab in chunks of 32 rows, staged in LDS as ONE fp64 array per side (a diagonal block
// pair stages one side), and feeds them four rows at a time, ascending, to the MFMAs; each wave owns a 16 x 64 strip:
// four 16 x 16 tiles, of a diagonal block pair only those on and above the diagonal.  A second kernel adds the slabs of
// a cell in ascending order.  A user writes, beside its kernel:
//   a stager        stage(int64_t r, bool live, double& a, double& b): what the loader thread stages of row r (live: r is
//                   in the slab) for its A column and, off the diagonal, its B column; a dead row adds nothing.  A lambda
//                   that captures BY VALUE: behind a reference the input pointer is no longer __restrict__, and every
//                   load of a chunk is waited for on its own (k_as_moments: 3 % slower);
//   an accumulator  row(double av, bool diag), once per four rows with the A operand, then tile(int j, double bv, bool
//                   both) per computed tile j with the B operand: the MFMAs (both: the tile is not on the diagonal);
//   a store         (int j, bool both) per computed tile: its vectors through gram64_put.
// Nothing here multiplies and adds in fp64 outside an MFMA: a user's fp contraction setting cannot change a bit of it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int GRAM64_NTHR = 256;             // four waves
constexpr int GRAM64_TILE = 64;              // a workgroup's block of the table
constexpr int GRAM64_CHUNK = 32;             // rows per LDS chunk: four rows per MFMA
constexpr int GRAM64_LD = GRAM64_TILE + 2;   // LDS row stride (doubles)
constexpr int GRAM64_SIDE = GRAM64_CHUNK * GRAM64_LD;       // doubles of one staged side

typedef double gram64_d4 __attribute__((ext_vector_type(4)));

struct Gram64Plan {
  int64_t rows;
  int slabs, nb, pairs;
};
// `blocks` workgroups aimed at, shared among the block pairs; a slab is whole chunks and at least min_rows rows
inline Gram64Plan gram64_plan(int64_t n, int L, int blocks, int min_rows) {
  Gram64Plan p;
  p.nb = (L + GRAM64_TILE - 1) / GRAM64_TILE;
  p.pairs = p.nb * (p.nb + 1) / 2;
  const int64_t target = blocks / p.pairs;
  int64_t rows = (n + target - 1) / target;
  rows = (rows + GRAM64_CHUNK - 1) / GRAM64_CHUNK * GRAM64_CHUNK;
  if (rows < min_rows) rows = min_rows;
  p.rows = rows;
  p.slabs = (int)((n + rows - 1) / rows);
  return p;
}

__device__ __forceinline__ bool mmg_finite(float x) { return fabsf(x) <= 3.402823466e+38f; }     // false for NaN and inf

// what a workgroup and a thread own, from blockIdx and threadIdx
struct Gram64Tile {
  int bi, bj, A0, B0;                        // the block pair, bi <= bj < nb, and its first columns
  bool diag, strip;                          // bi == bj; the wave's strip has a column of the table (wave-uniform)
  int lc, lr, ca, cb;                        // the loader's column and first row of a chunk; its columns of the table
  bool a_in, b_in;                           // ... which exist
  int kr, kc, w;                             // the MFMA's row of four and column of sixteen; the wave
  int64_t r0, r1;                            // the slab's rows

  __device__ __forceinline__ Gram64Tile(int nb, int L, int64_t n, int64_t rows_per_slab) {
    int p = (int)blockIdx.x;
    bi = 0;
    while (p >= nb - bi) { p -= nb - bi; ++bi; }
    bj = bi + p;
    diag = bi == bj;
    A0 = GRAM64_TILE * bi, B0 = GRAM64_TILE * bj;
    const int tid = threadIdx.x, lane = tid & 63;
    w = tid >> 6, lc = tid & 63, lr = tid >> 6, kr = lane >> 4, kc = lane & 15;
    ca = A0 + lc, cb = B0 + lc;
    a_in = ca < L, b_in = cb < L;
    strip = A0 + 16 * w < L;
    r0 = (int64_t)blockIdx.y * rows_per_slab;
    r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
  }
  // tile j of the strip is computed (wave-uniform); it is not on the diagonal of the table: both its halves are new
  __device__ __forceinline__ bool has(int j, int L) const { return B0 + 16 * j < L && (!diag || j >= w); }
  __device__ __forceinline__ bool both(int j) const { return !diag || j > w; }
  // The f64 MFMA's C/D layout is its own, not the f32 map: lane l, register g hold row (l >> 4) + 4 g, column l & 15.
  __device__ __forceinline__ int row(int g) const { return A0 + 16 * w + kr + 4 * g; }
  __device__ __forceinline__ int col(int j) const { return B0 + 16 * j + kc; }
};

// As, Bs: GRAM64_SIDE doubles of LDS each
template <class Acc, class Stage>
__device__ __forceinline__ void gram64_walk(const Gram64Tile& t, int L, double* As, double* Bs, Acc& acc, Stage stage) {
  const double* Bp = t.diag ? As : Bs;
  for (int64_t rc = t.r0; rc < t.r1; rc += GRAM64_CHUNK) {
    __syncthreads();                                            // the previous chunk has been consumed
#pragma unroll
    for (int i = 0; i < GRAM64_CHUNK / 4; ++i) {
      const int row = t.lr + 4 * i;
      double a, b;
      stage(rc + row, rc + row < t.r1, a, b);
      As[row * GRAM64_LD + t.lc] = a;
      if (!t.diag) Bs[row * GRAM64_LD + t.lc] = b;
    }
    __syncthreads();
    if (t.strip) {
#pragma unroll
      for (int ks = 0; ks < GRAM64_CHUNK / 4; ++ks) {
        const int row = 4 * ks + t.kr;
        acc.row(As[row * GRAM64_LD + 16 * t.w + t.kc], t.diag);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (t.has(j, L)) acc.tile(j, Bp[row * GRAM64_LD + 16 * j + t.kc], t.both(j));
      }
    }
  }
}

template <class Store>
__device__ __forceinline__ void gram64_store_tiles(const Gram64Tile& t, int L, Store store) {
  if (!t.strip) return;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (t.has(j, L)) store(j, t.both(j));
}

// one accumulator vector of tile j to an L x L plane, direct or transposed (a diagonal tile's a > b half is never read)
__device__ __forceinline__ void gram64_put(const Gram64Tile& t, int L, int j, gram64_d4 v, double* __restrict__ plane,
                                           bool transposed = false) {
  const int b = t.col(j);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    const int a = t.row(g);
    if (a < L && b < L) plane[transposed ? (size_t)b * L + a : (size_t)a * L + b] = v[g];
  }
}

// The slabs of one cell: the adds are serial in slab order, INFLIGHT loads are in flight at a time (the kernels are the
// latency of their dependent loads, not their bytes).
template <class T, int INFLIGHT>
__device__ __forceinline__ T gram64_sum_slabs(const T* __restrict__ src, size_t stride, int slabs) {
  T t = 0;
  int q = 0;
  for (; q + INFLIGHT - 1 < slabs; q += INFLIGHT) {
    T v[INFLIGHT];
#pragma unroll
    for (int k = 0; k < INFLIGHT; ++k) v[k] = src[(size_t)(q + k) * stride];
#pragma unroll
    for (int k = 0; k < INFLIGHT; ++k) t += v[k];
  }
  for (; q < slabs; ++q) t += src[(size_t)q * stride];
  return t;
}

// cell idx = a L + b of an L x L plane whose slabs lie `stride` apart.  Every cell of a plane that is not symmetric lies
// in a computed tile of every slab; of a symmetric one every a <= b, written to both (a, b) and (b, a).
template <int INFLIGHT>
__device__ __forceinline__ void gram64_sum_cell(const double* __restrict__ partial, size_t stride, int slabs, int L, int idx,
                                                bool sym, double* __restrict__ out) {
  const int a = idx / L, b = idx % L;
  if (sym && a > b) return;
  const double s = gram64_sum_slabs<double, INFLIGHT>(partial + idx, stride, slabs);
  out[idx] = s;
  if (sym && a < b) out[(size_t)b * L + a] = s;
}
