// The one stable LSD radix sort (8-bit digits) of (key, int32 value) pairs on a stream: csr.hip sorts edges by a uint32
// row, prep.hip sorts lab events by uint64 keys.  No atomics on the data path, so the result is deterministic; work is
// O(n * ceil(bits / 8)).
//   per pass:  tile histogram (digit-major) -> exclusive scan (scan.h) -> stable scatter
//   in-tile stable rank: wave-level match-any by ballots + per-group digit counts in LDS.
// The caller owns the buffers and decides where a sort starts, so that its last pass lands where it wants the result.
//
// Skip words (nullable): {OR, AND} of every key, on the device.  A digit in which they agree is the same in every key; its
// pass degenerates to a tile copy and leaves the histogram alone (the decision is taken on the device: nothing comes back
// to the host).  The branch is uniform over the grid.  SKIP = false compiles it out: csr.hip's instances are the kernels
// it had before the sorts were merged, register for register.
#pragma once
#include "common.h"
#include "scan.h"
#include <utility>

namespace {

constexpr int RADIX_TILE = 1024;      // items per workgroup tile (256 threads x 4)
constexpr int RADIX_NTHR = 256;
constexpr int RADIX_GROUPS = RADIX_TILE / WAVE;   // 16 groups of 64 consecutive items

__device__ __forceinline__ bool radix_skip(const unsigned long long* bits, int shift) {
  return bits && (((bits[0] ^ bits[1]) >> shift) & 255ull) == 0ull;
}

template <class Key, bool SKIP>
__global__ __launch_bounds__(RADIX_NTHR) void k_radix_hist(const Key* __restrict__ keys, uint32_t* tile_hist, int64_t n,
                                                     int shift, int64_t n_tiles, const unsigned long long* bits) {
  __shared__ uint32_t h[256];
  if (SKIP && radix_skip(bits, shift)) return;
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * RADIX_TILE;
#pragma unroll
  for (int i = 0; i < RADIX_TILE / RADIX_NTHR; ++i) {
    const int64_t e = base + i * RADIX_NTHR + threadIdx.x;
    if (e < n) atomicAdd(&h[(uint32_t)(keys[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  tile_hist[(int64_t)threadIdx.x * n_tiles + blockIdx.x] = h[threadIdx.x];
}

template <class Key, bool SKIP>
__global__ __launch_bounds__(RADIX_NTHR) void k_radix_scatter(const Key* __restrict__ keys_in,
                                                        const int32_t* __restrict__ vals_in,
                                                        Key* __restrict__ keys_out, int32_t* __restrict__ vals_out,
                                                        const uint32_t* __restrict__ tile_off, int64_t n, int shift,
                                                        int64_t n_tiles, const unsigned long long* bits) {
  __shared__ uint32_t gcnt[RADIX_GROUPS][256];   // per 64-item group: count of each digit -> exclusive offset
  const int64_t base = (int64_t)blockIdx.x * RADIX_TILE;
  if (SKIP && radix_skip(bits, shift)) {               // one digit for every key: the pass is the identity
#pragma unroll
    for (int i = 0; i < RADIX_TILE / RADIX_NTHR; ++i) {
      const int64_t e = base + i * RADIX_NTHR + threadIdx.x;
      if (e < n) {
        keys_out[e] = keys_in[e];
        vals_out[e] = vals_in[e];
      }
    }
    return;
  }
  for (int i = threadIdx.x; i < RADIX_GROUPS * 256; i += RADIX_NTHR) (&gcnt[0][0])[i] = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  Key key[RADIX_TILE / RADIX_NTHR];
  int32_t val[RADIX_TILE / RADIX_NTHR];
  uint32_t rank[RADIX_TILE / RADIX_NTHR];
  // wave w owns groups 4w .. 4w+3 (consecutive 64-item runs) => item order is preserved
#pragma unroll
  for (int i = 0; i < RADIX_TILE / RADIX_NTHR; ++i) {
    const int g = wid * (RADIX_TILE / RADIX_NTHR) + i;
    const int64_t e = base + (int64_t)g * 64 + lane;
    const bool valid = e < n;
    key[i] = valid ? keys_in[e] : (Key)0;
    val[i] = valid ? vals_in[e] : 0;
    const uint32_t d = (uint32_t)(key[i] >> shift) & 255u;
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(bit);
      m &= bit ? bal : ~bal;
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    rank[i] = (uint32_t)__popcll(m & lt);
    if (valid && rank[i] == 0) gcnt[g][d] = (uint32_t)__popcll(m);
  }
  __syncthreads();
  {  // thread d: exclusive scan of digit d over the 16 groups, plus the tile's global offset
    const int d = threadIdx.x;
    uint32_t run = tile_off[(int64_t)d * n_tiles + blockIdx.x];
#pragma unroll
    for (int g = 0; g < RADIX_GROUPS; ++g) {
      const uint32_t c = gcnt[g][d];
      gcnt[g][d] = run;
      run += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < RADIX_TILE / RADIX_NTHR; ++i) {
    const int g = wid * (RADIX_TILE / RADIX_NTHR) + i;
    const int64_t e = base + (int64_t)g * 64 + lane;
    if (e < n) {
      const uint32_t d = (uint32_t)(key[i] >> shift) & 255u;
      const uint32_t pos = gcnt[g][d] + rank[i];      // < n: the offsets are a scan of counts that sum to n
      keys_out[pos] = key[i];
      vals_out[pos] = val[i];
    }
  }
}

// tiles of a sort over n items, and what a pass needs besides the pairs (in uint32 elements)
struct RadixSizes {
  int64_t n_tiles;
  size_t hist_elems, scratch_elems;
};
inline RadixSizes radix_sizes(int64_t n) {
  RadixSizes s;
  s.n_tiles = n > 0 ? (n + RADIX_TILE - 1) / RADIX_TILE : 1;
  s.hist_elems = (size_t)(256 * s.n_tiles);
  s.scratch_elems = scan_scratch_elems(256 * s.n_tiles);
  return s;
}

// the double-buffered pairs: a pass reads (keys, vals), writes (keys_alt, vals_alt) and swaps
template <class Key>
struct RadixPairs {
  Key *keys, *keys_alt;
  int32_t *vals, *vals_alt;
};

// one pass over the digit at `shift` (n > 0); hist [radix_sizes(n).hist_elems], scratch [.scratch_elems]; skip_bits is
// read only by the SKIP = true instances
template <bool SKIP, class Key>
void radix_pass(RadixPairs<Key>& b, int64_t n, int shift, const unsigned long long* skip_bits, uint32_t* hist,
                uint32_t* scratch, hipStream_t st) {
  const int64_t n_tiles = radix_sizes(n).n_tiles;
  const dim3 grid((unsigned)n_tiles), block(RADIX_NTHR);
  hipLaunchKernelGGL((k_radix_hist<Key, SKIP>), grid, block, 0, st, b.keys, hist, n, shift, n_tiles, skip_bits);
  exclusive_scan_u32(hist, 256 * n_tiles, scratch, st);
  hipLaunchKernelGGL((k_radix_scatter<Key, SKIP>), grid, block, 0, st, b.keys, b.vals, b.keys_alt, b.vals_alt, hist, n,
                     shift, n_tiles, skip_bits);
  std::swap(b.keys, b.keys_alt);
  std::swap(b.vals, b.vals_alt);
}

}  // namespace
