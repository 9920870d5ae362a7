// The sorted pair list of the satellite libraries (boot.hip, shift.hip, stack.hip, conformal.hip, prop.hip): a key and an
// int32 payload per pair, the stable radix sort of radix_sort.h over the digits the key can differ in, where every segment
// begins, the walk of the sorted list in chunks and the combination of the chunks' slots in chunk order.  What the five
// files keep is what differs: how a key is formed, what a walk adds up, what a slot holds.  Only for the satellite
// libraries: no source of libmmgnn.so includes it.
#pragma once
#include "common.h"
#include "radix_sort.h"

inline int bits_of(unsigned v) {         // bits needed to write v
  int b = 0;
  while (v) { ++b; v >>= 1; }
  return b;
}
// workgroups of `threads` for n items, per_thread items to a thread, at most max_grid (the kernels stride by the grid)
inline unsigned launch_grid(int64_t n, int threads, int max_grid, int per_thread = 4) {
  int64_t g = (n + (int64_t)threads * per_thread - 1) / ((int64_t)threads * per_thread);
  return (unsigned)(g < 1 ? 1 : g > max_grid ? max_grid : g);
}

// first position in the ascending K [0, n) whose key is >= v
template <class KT>
__device__ __forceinline__ int64_t lower_bound(const KT* __restrict__ K, int64_t n, KT v) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (K[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// fp32 -> uint32 that orders as the value does (-0.0 below +0.0, NaN outside the finite keys), and back; bits_orderable
// takes the value's bits (shift.hip folds -0.0 onto +0.0 in them first)
__device__ __forceinline__ uint32_t bits_orderable(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ uint32_t float_orderable(float x) { return bits_orderable(__float_as_uint(x)); }
__device__ __forceinline__ float orderable_float(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// f(IT()) with IT = int64_t or int32_t, the width of the caller's index lists: one launch where there were two
template <class F>
inline void index_dispatch(int index_bytes, F&& f) {
  if (index_bytes == 8) f(int64_t());
  else f(int32_t());
}

// The close of a key kernel's count of the pairs it leaves out, by kind: cnt is the thread's own count (at most 2^31 /
// (grid x workgroup) pairs: no overflow), summed per wave, one integer atomic per wave and kind (integers: any order, one
// result).  The counting stays where the pair is classified: an array indexed by the kind stays in registers only as a
// plain local of the kernel.
template <int KINDS>
__device__ __forceinline__ void drop_flush(const int (&cnt)[KINDS], unsigned long long* __restrict__ dropped) {
#pragma unroll
  for (int k = 0; k < KINDS; ++k) {
    const int t = wave_sum_i(cnt[k]);
    if ((threadIdx.x & 63) == 0 && t) atomicAdd(dropped + k, (unsigned long long)t);
  }
}

// The chunk protocol of a walk over the kept pairs [0, nk) of a sorted list in chunks of CHUNK consecutive positions
// (k_boot_sums, k_sh_walk) and of the kernel that combines what the walk left (k_boot_combine, k_sh_combine).  A walk has
// one open segment at a time and closes it
//   - into its chunk's HEAD slot (0) when the segment is the chunk's first (`cur == first`: it may have begun earlier),
//   - straight into the result when the segment begins and ends inside the chunk and a kept pair of the chunk follows it,
//   - into its chunk's TAIL slot (1) at the chunk's end or in front of the first dropped pair, if it is not the first.
// So of segment [lo, hi) the chunks c0 .. c1 each hold one slot, HEAD where the segment reaches the chunk's first position
// and TAIL in c0 otherwise, and combine adds them in chunk order -- except for a segment the walk wrote itself, which it
// must leave alone: every element of the result is written exactly once.  This is the one statement of that rule.
template <int CHUNK>
struct SegChunks {
  int64_t lo, hi, nk, c0, c1;
  __device__ __forceinline__ SegChunks(int64_t lo_, int64_t hi_, int64_t nk_)
      : lo(lo_), hi(hi_), nk(nk_), c0(lo_ / CHUNK), c1(hi_ > lo_ ? (hi_ - 1) / CHUNK : lo_ / CHUNK) {}
  __device__ __forceinline__ bool empty() const { return hi <= lo; }     // no slot anywhere: the result is zeros
  // inside one chunk, not its first segment, and a kept pair of the chunk follows it
  __device__ __forceinline__ bool written_by_walk() const {
    return hi > lo && c0 == c1 && lo > c0 * CHUNK && hi < (c0 + 1) * CHUNK && hi < nk;
  }
  // the slot of chunk c in [c0, c1]: the segment heads the chunk, or ends it
  __device__ __forceinline__ int which(int64_t c) const { return lo <= c * CHUNK ? 0 : 1; }
};

namespace {

// what a sort of n (Key, int32) pairs works in: the double-buffered pairs, a pass's histogram and scan scratch
template <class Key>
struct SegSortWs {
  RadixPairs<Key> kv;
  uint32_t *hist, *scr;
};
template <class Key>
inline void segsort_carve(MmgCarver& c, int64_t n, SegSortWs<Key>* w) {
  const RadixSizes rs = radix_sizes(n);
  const size_t nn = (size_t)(n > 0 ? n : 1);
  w->kv.keys = c.take<Key>(nn);
  w->kv.keys_alt = c.take<Key>(nn);
  w->kv.vals = c.take<int32_t>(nn);
  w->kv.vals_alt = c.take<int32_t>(nn);
  w->hist = c.take<uint32_t>(rs.hist_elems);
  w->scr = c.take<uint32_t>(rs.scratch_elems);
}
// the stable sort by the low key_bits bits of the key (n > 0); the result is in w.kv.keys / w.kv.vals.  A key that marks
// a dropped pair is n_seg itself, so the callers pass bits_of(n_seg), above a 32-bit value 32 + bits_of(n_seg).
template <class Key>
inline void segsort_run(SegSortWs<Key>& w, int64_t n, int key_bits, hipStream_t st) {
  for (int shift = 0; shift < key_bits; shift += 8) radix_pass<false>(w.kv, n, shift, nullptr, w.hist, w.scr, st);
}

// out[s], s = 0 .. n_seg: the first sorted position whose key is >= s << shift (out[n_seg]: the number of kept pairs)
constexpr int SEG_BOUNDS_NTHR = 256;
template <class Key, class Out>
__global__ __launch_bounds__(SEG_BOUNDS_NTHR) void k_seg_bounds(const Key* __restrict__ K, int64_t n, int n_seg, int shift,
                                                                Out* __restrict__ out) {
  const int s = blockIdx.x * SEG_BOUNDS_NTHR + threadIdx.x;
  if (s <= n_seg) out[s] = (Out)lower_bound(K, n, (Key)s << shift);
}
template <class Key, class Out>
inline void seg_bounds(const Key* K, int64_t n, int n_seg, int shift, Out* out, hipStream_t st) {
  hipLaunchKernelGGL((k_seg_bounds<Key, Out>), dim3((unsigned)((n_seg + 1 + SEG_BOUNDS_NTHR - 1) / SEG_BOUNDS_NTHR)),
                     dim3(SEG_BOUNDS_NTHR), 0, st, K, n, n_seg, shift, out);
}

}  // namespace
