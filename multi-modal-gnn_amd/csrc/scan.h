// In-place exclusive scan of a uint32 array on a stream (csr.hip's radix sort and rowptr, prep.hip's sort and
// compaction): local scan of 2048-item chunks, recursive scan of the chunk sums, add-back.  Integer: exact and
// order-independent.
#pragma once
#include "common.h"

namespace {

constexpr int SCAN_NTHR = 256;
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_CHUNK = SCAN_NTHR * SCAN_ITEMS;

__global__ __launch_bounds__(SCAN_NTHR) void k_scan_local(uint32_t* data, uint32_t* block_sums, int64_t n) {
  __shared__ uint32_t s_wave[SCAN_NTHR / WAVE];
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_ITEMS;
  uint32_t v[SCAN_ITEMS];
  uint32_t tsum = 0;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    v[i] = (base + i < n) ? data[base + i] : 0u;
    tsum += v[i];
  }
  // inclusive scan of tsum across the wave
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = tsum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wid] = inc;
  __syncthreads();
  uint32_t woff = 0;
  for (int w = 0; w < wid; ++w) woff += s_wave[w];
  uint32_t run = woff + inc - tsum;   // exclusive prefix of this thread
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i) {
    if (base + i < n) data[base + i] = run;
    run += v[i];
  }
  if (threadIdx.x == SCAN_NTHR - 1 && block_sums) block_sums[blockIdx.x] = run;
}

__global__ __launch_bounds__(SCAN_NTHR) void k_scan_add(uint32_t* data, const uint32_t* block_prefix, int64_t n) {
  const uint32_t add = block_prefix[blockIdx.x];
  const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_ITEMS;
#pragma unroll
  for (int i = 0; i < SCAN_ITEMS; ++i)
    if (base + i < n) data[base + i] += add;
}

// scratch needed for the block-sum levels of a scan over n items (in uint32 elements)
size_t scan_scratch_elems(int64_t n) {
  size_t tot = 0;
  while (n > SCAN_CHUNK) {
    n = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
    tot += (size_t)n;
  }
  return tot + 1;
}

void exclusive_scan_u32(uint32_t* data, int64_t n, uint32_t* scratch, hipStream_t st) {
  if (n <= 0) return;
  const int64_t nb = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
  if (nb == 1) {
    hipLaunchKernelGGL(k_scan_local, dim3(1), dim3(SCAN_NTHR), 0, st, data, (uint32_t*)nullptr, n);
    return;
  }
  hipLaunchKernelGGL(k_scan_local, dim3((unsigned)nb), dim3(SCAN_NTHR), 0, st, data, scratch, n);
  exclusive_scan_u32(scratch, nb, scratch + nb, st);
  hipLaunchKernelGGL(k_scan_add, dim3((unsigned)nb), dim3(SCAN_NTHR), 0, st, data, scratch, n);
}

}  // namespace
