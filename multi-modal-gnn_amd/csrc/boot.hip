// Patient-cluster bootstrap of the evaluation metrics (include/mmgnn_boot.h; mmgnn/bootstrap.py): replicates x pairs
// weighted updates of the seven (ten, with a second predictor) additive terms of mmg_seg_metrics, the metrics of every
// replicate, and their summary (mean, standard error, percentile interval).
//   k_boot_keys     ONE read of the indices: sort key = the segment (n_seg for a dropped pair: sorts last), payload = the
//                   pair's position, the unit as uint32, the three kinds of dropped pairs (drop_flush of segsort.h).
//   segsort_run     the stable sort of segsort.h over the 1-2 digits of the segment.
//   k_boot_sums     workgroup (c, y) walks chunk c (BT_CHUNK consecutive sorted pairs) for the BT_RB replicates
//                   y * BT_RB + thread: tiles of BT_TILE pairs are gathered into LDS once (terms formed in fp32 / fp64 as
//                   k_seg_metrics forms them), then every thread walks the tile -- all threads read the same LDS word
//                   (broadcast), hash once per pair, count the thresholds, and add weight * term to registers.  Every
//                   thread of the workgroup sees the same segment boundaries: no divergence.  A tile whose first and last
//                   key agree (sorted keys: one segment) is walked unrolled, without reading the keys -- the same
//                   additions in the same order.  At a boundary the registers go to the chunk's HEAD slot, straight to
//                   `sums` or to the chunk's TAIL slot: the chunk protocol stated at SegChunks (segsort.h).
//   k_boot_combine  one thread per (segment, replicate): the segment's bounds and the number of kept pairs by three binary
//                   searches, then SegChunks: the segment's chunks' slots added in chunk order; a segment without pairs
//                   gets zeros; a segment k_boot_sums wrote itself is left alone.  Every element of `sums` is written
//                   exactly once: nothing is zero-filled, nothing is accumulated in memory.
//   k_boot_metrics  one thread per (replicate, row).   k_boot_summary  one workgroup per (row, metric): sums in a fixed
//                   order, a bitonic sort of up to 4096 doubles in LDS, numpy's "linear" percentile.
// fp64 contraction is OFF for the whole file (the metric rules and the percentile restate Python arithmetic operation by
// operation); the weighted update asks for its fused multiply-add by name -- the product weight * term is exact, so the
// fused and the unfused form round alike.
// Built into libmmgnn_boot.so beside libmmgnn.so and on top of it (mmg_set_error).
#include "common.h"
#include "cells.h"
#include "radix_sort.h"
#include "../../include/mmgnn_boot.h"
#include <limits.h>
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int BT_NTHR = 256;
constexpr int BT_RB = MMG_BOOT_RB;
constexpr int BT_CHUNK = MMG_BOOT_CHUNK;
constexpr int BT_TILE = 256;              // pairs staged in LDS at a time
constexpr int BT_MAX_GRID = 2048;
static_assert(BT_RB == BT_NTHR, "one replicate per thread");
static_assert(BT_CHUNK % BT_TILE == 0, "a chunk is whole tiles");
static_assert(MMG_BOOT_MAX_REPLICATES <= 4096, "the summary sorts the replicates of a cell in 32 KB of LDS");
static_assert(MMG_BOOT_MAX_SEG < 65536, "the sort runs over two digits of the segment");

// T[j] = round(65536 * PoissonCDF(j; 1)): the weight of a 16-bit field is the number of thresholds it reaches
constexpr uint32_t BT_T[8] = {24109u, 48219u, 60273u, 64292u, 65296u, 65497u, 65531u, 65535u};

__device__ __forceinline__ uint32_t bt_weight(uint32_t key, uint32_t half_unit, uint32_t shift) {
  uint32_t w0, w1;
  mmg_rng_group(key, (uint64_t)half_unit, &w0, &w1);       // w1 is dead code: only the first word is used
  const uint32_t field = (w0 >> shift) & 0xFFFFu;
  uint32_t w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) w += field >= BT_T[j] ? 1u : 0u;
  return w;
}

// ---------------------------------------------------------------------------------- keys
template <class IT>
__global__ __launch_bounds__(BT_NTHR) void k_boot_keys(const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ pred_b, const IT* __restrict__ unit,
                                                       const IT* __restrict__ seg, int64_t n, int64_t n_units, int n_seg,
                                                       uint32_t* __restrict__ key, int32_t* __restrict__ id,
                                                       uint32_t* __restrict__ unit32,
                                                       unsigned long long* __restrict__ dropped) {
  int cnt[MMG_BOOT_DROP_KINDS] = {0, 0, 0};
  const int64_t step = (int64_t)gridDim.x * BT_NTHR;
  for (int64_t i = (int64_t)blockIdx.x * BT_NTHR + threadIdx.x; i < n; i += step) {
    const int64_t s = (int64_t)seg[i], u = (int64_t)unit[i];
    const float p = pred[i], t = target[i], pb = pred_b ? pred_b[i] : 0.f;
    int kind = -1;
    if (s < 0 || s >= n_seg) kind = 0;
    else if (u < 0 || u >= n_units) kind = 1;
    else if (p != p || t != t || pb != pb) kind = 2;
    if (kind >= 0) cnt[kind] += 1;
    key[i] = kind < 0 ? (uint32_t)s : (uint32_t)n_seg;
    id[i] = (int32_t)i;
    unit32[i] = kind < 0 ? (uint32_t)u : 0u;
  }
  drop_flush(cnt, dropped);
}

// ---------------------------------------------------------------------------------- sums
template <int F>
struct BtAcc {
  double a[F];               // fields 0 and 6 are kept in the integers below
  uint32_t n, nz;            // <= 8 * BT_CHUNK: no overflow inside a chunk
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int f = 0; f < F; ++f) a[f] = 0.0;
    n = 0u;
    nz = 0u;
  }
  __device__ __forceinline__ void store(double* __restrict__ dst) const {
#pragma unroll
    for (int f = 0; f < F; ++f) dst[f] = f == 0 ? (double)n : f == 6 ? (double)nz : a[f];
  }
};

// slot (chunk c, which: 0 head / 1 tail, replicate r) of the partials
__device__ __forceinline__ size_t bt_slot(int64_t c, int which, int r, int R1, int F) {
  return (((size_t)c * 2 + which) * R1 + r) * F;
}

template <bool WITH_B>
__global__ __launch_bounds__(BT_NTHR) void k_boot_sums(const uint32_t* __restrict__ K, const int32_t* __restrict__ id,
                                                       const uint32_t* __restrict__ unit32, int64_t n, int n_seg,
                                                       const float* __restrict__ pred, const float* __restrict__ target,
                                                       const float* __restrict__ pred_b, int replicates, uint64_t seed,
                                                       double* __restrict__ part, double* __restrict__ sums) {
  constexpr int F = WITH_B ? MMG_BOOT_FIELDS_B : MMG_BOOT_FIELDS;
  __shared__ double s_abs[BT_TILE], s_sq[BT_TILE], s_t[BT_TILE], s_t2[BT_TILE], s_ape[BT_TILE];
  __shared__ double s_babs[WITH_B ? BT_TILE : 1], s_bsq[WITH_B ? BT_TILE : 1], s_bape[WITH_B ? BT_TILE : 1];
  __shared__ uint32_t s_half[BT_TILE], s_seg[BT_TILE];
  __shared__ unsigned char s_shift[BT_TILE], s_nz[BT_TILE];
  const int R1 = replicates + 1;
  const int r = blockIdx.y * BT_RB + threadIdx.x;
  const bool live = r < R1;
  const uint32_t key = mmg_rng_key(seed, (uint32_t)MMG_BOOT_SITE + (uint32_t)r);
  const int64_t c = blockIdx.x, begin = c * BT_CHUNK;
  const int64_t end = begin + BT_CHUNK < n ? begin + BT_CHUNK : n;
  BtAcc<F> acc;
  acc.clear();
  uint32_t cur = (uint32_t)n_seg, first = (uint32_t)n_seg;          // n_seg: no open segment
  bool more = true;
  for (int64_t base = begin; base < end && more; base += BT_TILE) {
    __syncthreads();                                                 // the previous tile is consumed
    {
      const int64_t j = base + threadIdx.x;
      uint32_t s = (uint32_t)n_seg;
      if (j < end) s = K[j];
      if (s < (uint32_t)n_seg) {
        const int32_t i = id[j];
        const uint32_t u = unit32[i];
        const float p = pred[i], t = target[i];
        const float e = t - p;
        s_abs[threadIdx.x] = (double)fabsf(e);
        s_sq[threadIdx.x] = (double)e * (double)e;
        s_t[threadIdx.x] = (double)t;
        s_t2[threadIdx.x] = (double)t * (double)t;
        s_ape[threadIdx.x] = t != 0.f ? (double)fabsf(e / t) : 0.0;
        s_nz[threadIdx.x] = t != 0.f ? 1 : 0;
        if (WITH_B) {
          const float eb = t - pred_b[i];
          s_babs[threadIdx.x] = (double)fabsf(eb);
          s_bsq[threadIdx.x] = (double)eb * (double)eb;
          s_bape[threadIdx.x] = t != 0.f ? (double)fabsf(eb / t) : 0.0;
        }
        s_half[threadIdx.x] = u >> 1;
        s_shift[threadIdx.x] = (unsigned char)((u & 1u) * 16u);
      }
      s_seg[threadIdx.x] = s;
    }
    __syncthreads();
    if (base == begin) first = s_seg[0];
    auto flush_to = [&](uint32_t s) {                                // the open segment ends in front of a pair of s
      if (cur < (uint32_t)n_seg && live)                             // HEAD slot or direct: the protocol at SegChunks
        acc.store(cur == first ? part + bt_slot(c, 0, r, R1, F) : sums + ((size_t)r * n_seg + cur) * F);
      acc.clear();
      cur = s;
    };
    auto update = [&](int j) {
      const uint32_t h = bt_weight(key, s_half[j], s_shift[j]);
      const uint32_t w = r == 0 ? 1u : h;                            // a select, not a branch
      const double wd = (double)w;
      acc.n += w;
      acc.nz += s_nz[j] ? w : 0u;
      acc.a[1] = fma(wd, s_abs[j], acc.a[1]);
      acc.a[2] = fma(wd, s_sq[j], acc.a[2]);
      acc.a[3] = fma(wd, s_t[j], acc.a[3]);
      acc.a[4] = fma(wd, s_t2[j], acc.a[4]);
      acc.a[5] = fma(wd, s_ape[j], acc.a[5]);
      if (WITH_B) {
        acc.a[F - 3] = fma(wd, s_babs[j], acc.a[F - 3]);
        acc.a[F - 2] = fma(wd, s_bsq[j], acc.a[F - 2]);
        acc.a[F - 1] = fma(wd, s_bape[j], acc.a[F - 1]);
      }
    };
    if (s_seg[0] == s_seg[BT_TILE - 1] && s_seg[0] < (uint32_t)n_seg) {
      // the keys are sorted: a whole tile of one segment (the common case: segments are thousands of pairs long) is
      // walked without a look at the keys -- the same additions in the same order as the loop below
      if (s_seg[0] != cur) flush_to(s_seg[0]);
#pragma unroll 8
      for (int j = 0; j < BT_TILE; ++j) update(j);
    } else {
      for (int j = 0; j < BT_TILE; ++j) {
        const uint32_t s = s_seg[j];                                 // the same word for every thread
        if (s >= (uint32_t)n_seg) {                                  // past the chunk's end or into the dropped pairs
          more = false;
          break;
        }
        if (s != cur) flush_to(s);
        update(j);
      }
    }
  }
  if (cur < (uint32_t)n_seg && live) acc.store(part + bt_slot(c, cur == first ? 0 : 1, r, R1, F));
}

template <int F>
__global__ __launch_bounds__(BT_NTHR) void k_boot_combine(const uint32_t* __restrict__ K, int64_t n, int n_seg,
                                                          int replicates, const double* __restrict__ part,
                                                          double* __restrict__ sums) {
  __shared__ int64_t s_b[3];                                         // the segment's bounds and the number of kept pairs
  const int R1 = replicates + 1;
  const uint32_t s = blockIdx.x;
  if (threadIdx.x < 3) s_b[threadIdx.x] = lower_bound(K, n, threadIdx.x < 2 ? s + threadIdx.x : (uint32_t)n_seg);
  __syncthreads();
  const SegChunks<BT_CHUNK> ch(s_b[0], s_b[1], s_b[2]);
  if (ch.written_by_walk()) return;                                  // the whole workgroup
  for (int r = blockIdx.y * BT_NTHR + threadIdx.x; r < R1; r += gridDim.y * BT_NTHR) {
    double a[F];
#pragma unroll
    for (int f = 0; f < F; ++f) a[f] = 0.0;
    if (!ch.empty())
      for (int64_t c = ch.c0; c <= ch.c1; ++c) {
        const double* __restrict__ src = part + bt_slot(c, ch.which(c), r, R1, F);
#pragma unroll
        for (int f = 0; f < F; ++f) a[f] += src[f];
      }
    double* __restrict__ dst = sums + ((size_t)r * n_seg + s) * F;
#pragma unroll
    for (int f = 0; f < F; ++f) dst[f] = a[f];
  }
}

// ---------------------------------------------------------------------------------- metrics
// evaluate.metrics_from_sums, line for line; every operation rounded on its own (contraction is off)
__device__ __forceinline__ void bt_metrics4(double n, double s_abs, double s_sq, double s_t, double s_t2, double s_ape,
                                            double n_nz, double* __restrict__ out) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (n <= 0.0) {
    out[0] = out[1] = out[2] = out[3] = nan;
    return;
  }
  const double ss_tot = s_t2 - s_t * s_t / n;
  double r2;
  if (n < 2.0) r2 = nan;
  else if (s_sq == 0.0) r2 = 1.0;
  else if (ss_tot > 1e-12 * (1e-300 > s_t2 ? 1e-300 : s_t2)) r2 = 1.0 - s_sq / ss_tot;
  else r2 = 0.0;
  out[0] = s_abs / n;
  out[1] = __dsqrt_rn(s_sq / n);
  out[2] = r2;
  out[3] = n_nz > 0.0 ? s_ape / n_nz * 100.0 : nan;
}

template <bool WITH_B>
__global__ __launch_bounds__(BT_NTHR) void k_boot_metrics(const double* __restrict__ sums, int n_seg, int replicates,
                                                          double* __restrict__ metrics) {
  constexpr int F = WITH_B ? MMG_BOOT_FIELDS_B : MMG_BOOT_FIELDS;
  constexpr int M = WITH_B ? MMG_BOOT_METRICS_B : MMG_BOOT_METRICS;
  const int64_t cells = (int64_t)(replicates + 1) * (n_seg + 1);
  for (int64_t q = (int64_t)blockIdx.x * BT_NTHR + threadIdx.x; q < cells; q += (int64_t)gridDim.x * BT_NTHR) {
    // the rows of all segments together first: they are the long ones
    const int r = (int)(q % (replicates + 1));
    const int row = n_seg - (int)(q / (replicates + 1));
    double a[F];
    const double* __restrict__ src = sums + (size_t)r * n_seg * F;
    if (row < n_seg) {
#pragma unroll
      for (int f = 0; f < F; ++f) a[f] = src[(size_t)row * F + f];
    } else {
#pragma unroll
      for (int f = 0; f < F; ++f) a[f] = 0.0;
      for (int s = 0; s < n_seg; ++s)
#pragma unroll
        for (int f = 0; f < F; ++f) a[f] += src[(size_t)s * F + f];
    }
    double* __restrict__ out = metrics + ((size_t)r * (n_seg + 1) + row) * M;
    double m[4];
    bt_metrics4(a[0], a[1], a[2], a[3], a[4], a[5], a[6], m);
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = m[k];
    if (WITH_B) {
      double mb[4];
      bt_metrics4(a[0], a[F - 3], a[F - 2], a[3], a[4], a[F - 1], a[6], mb);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        out[4 + k] = mb[k];
        out[8 + k] = m[k] - mb[k];
      }
    }
  }
}

// ---------------------------------------------------------------------------------- summary
__device__ __forceinline__ double bt_percentile(const double* __restrict__ x, int m, double q) {
  const double v = (double)(m - 1) * q;
  if (v >= (double)(m - 1)) return x[m - 1];
  if (v < 0.0) return x[0];
  const double fl = floor(v);
  const int i = (int)fl;
  const double g = v - fl, a = x[i], b = x[i + 1], d = b - a;
  return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// the workgroup's total of v, by the fixed order of the header, known to every thread
__device__ __forceinline__ double bt_block_sum(double v, double* __restrict__ s_w) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
#pragma unroll
  for (int q = 0; q < BT_NTHR / WAVE; ++q) t += s_w[q];
  return t;
}

__global__ __launch_bounds__(BT_NTHR) void k_boot_summary(const double* __restrict__ metrics, int n_seg, int replicates,
                                                          int M, double q_lo, double q_hi, double* __restrict__ summary) {
  __shared__ double x[MMG_BOOT_MAX_REPLICATES];
  __shared__ double s_w[BT_NTHR / WAVE];
  __shared__ int s_c[2][BT_NTHR / WAVE];
  const double inf = __longlong_as_double(0x7ff0000000000000ll), nan = __longlong_as_double(0x7ff8000000000000ll);
  const size_t stride = (size_t)(n_seg + 1) * M;                     // between two replicates of one (row, metric)
  int P = 2;
  while (P < replicates) P <<= 1;                                    // <= 4096
  for (int cell = blockIdx.x; cell < (n_seg + 1) * M; cell += gridDim.x) {
    __syncthreads();                                                 // the previous cell's shared values are consumed
    const double* __restrict__ src = metrics + cell;
    double sum = 0.0;
    int cnt = 0, below = 0;
    for (int i = threadIdx.x; i < P; i += BT_NTHR) {
      double v = inf;
      if (i < replicates) {
        v = src[(size_t)(i + 1) * stride];
        if (isfinite(v)) {
          sum += v;
          cnt += 1;
          below += v < 0.0 ? 1 : 0;
        } else {
          v = inf;
        }
      }
      x[i] = v;
    }
    cnt = wave_sum_i(cnt);
    below = wave_sum_i(below);
    if ((threadIdx.x & 63) == 0) {
      s_c[0][threadIdx.x >> 6] = cnt;
      s_c[1][threadIdx.x >> 6] = below;
    }
    sum = bt_block_sum(sum, s_w);                                    // (its barriers also publish x and s_c)
    int m = 0, n_below = 0;
#pragma unroll
    for (int q = 0; q < BT_NTHR / WAVE; ++q) {
      m += s_c[0][q];
      n_below += s_c[1][q];
    }
    const double mean = m > 0 ? sum / (double)m : nan;
    double ss = 0.0;
    for (int i = threadIdx.x; i < replicates; i += BT_NTHR) {
      const double v = x[i];
      if (v != inf) {
        const double d = v - mean;
        ss += d * d;
      }
    }
    ss = bt_block_sum(ss, s_w);
    // bitonic sort of x[0 .. P), ascending; the values that are not finite are +inf and end up behind the m finite ones
    for (int k = 2; k <= P; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        __syncthreads();
        for (int i = threadIdx.x; i < P; i += BT_NTHR) {
          const int l = i ^ j;
          if (l > i) {
            const double a = x[i], b = x[l];
            const bool up = (i & k) == 0;
            if (up ? a > b : a < b) {
              x[i] = b;
              x[l] = a;
            }
          }
        }
      }
    __syncthreads();
    if (threadIdx.x == 0) {
      double* __restrict__ out = summary + (size_t)cell * MMG_BOOT_SUMMARY_FIELDS;
      out[0] = src[0];
      out[1] = mean;
      out[2] = m > 1 ? __dsqrt_rn(ss / (double)(m - 1)) : nan;
      out[3] = m > 0 ? bt_percentile(x, m, q_lo) : nan;
      out[4] = m > 0 ? bt_percentile(x, m, q_hi) : nan;
      out[5] = (double)m;
      out[6] = m > 0 ? (double)n_below / (double)m : nan;
    }
  }
}

struct BootWs {
  SegSortWs<uint32_t> sort;
  uint32_t* unit32;
  double* part;
};
inline int64_t bt_chunks(int64_t n) { return n > 0 ? (n + BT_CHUNK - 1) / BT_CHUNK : 1; }
size_t boot_carve(void* ws, int64_t n, int replicates, int F, BootWs* w) {
  MmgCarver c(ws);
  segsort_carve(c, n, &w->sort);
  w->unit32 = c.take<uint32_t>((size_t)(n > 0 ? n : 1));
  w->part = c.take<double>((size_t)bt_chunks(n) * 2 * (size_t)(replicates + 1) * F);
  return c.need();
}

bool shape_ok(int n_seg, int replicates) {
  return n_seg >= 1 && n_seg <= MMG_BOOT_MAX_SEG && replicates >= 1 && replicates <= MMG_BOOT_MAX_REPLICATES;
}
int shape_check(const char* what, int n_seg, int replicates) {
  MMG_CHECK_ARG(replicates >= 1 && replicates <= MMG_BOOT_MAX_REPLICATES, "%s: %d replicates outside [1, %d]", what,
                replicates, MMG_BOOT_MAX_REPLICATES);
  MMG_CHECK_ARG(n_seg >= 1 && n_seg <= MMG_BOOT_MAX_SEG, "%s: %d segments outside [1, %d]", what, n_seg, MMG_BOOT_MAX_SEG);
  return MMG_OK;
}

}  // namespace

extern "C" size_t mmg_boot_sums_ws_bytes(int64_t n, int n_seg, int replicates, int with_b) {
  if (n < 0 || n > INT32_MAX || !shape_ok(n_seg, replicates)) return 0;
  BootWs w;
  return boot_carve(nullptr, n, replicates, with_b ? MMG_BOOT_FIELDS_B : MMG_BOOT_FIELDS, &w);
}

extern "C" int mmg_boot_sums(const float* pred, const float* target, const float* pred_b, int with_b, const void* unit,
                             const void* seg, int index_bytes, int64_t n, int64_t n_units, int n_seg, int replicates,
                             uint64_t seed, double* sums, int64_t* dropped, void* ws, size_t ws_bytes, void* stream) {
  int rc = shape_check("boot_sums", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(index_bytes == 4 || index_bytes == 8, "boot_sums: index_bytes %d is neither 4 nor 8", index_bytes);
  MMG_CHECK_ARG(n >= 0 && n <= INT32_MAX, "boot_sums: n %lld outside [0, 2^31)", (long long)n);
  MMG_CHECK_ARG(n_units >= 0 && n_units <= INT32_MAX, "boot_sums: %lld units outside [0, 2^31)", (long long)n_units);
  MMG_CHECK_ARG(n == 0 || (pred && target && unit && seg), "boot_sums: null pred, target, unit or seg");
  MMG_CHECK_ARG(n == 0 || !with_b || pred_b, "boot_sums: null pred_b");
  MMG_CHECK_ARG(sums && dropped, "boot_sums: null output");
  if (!with_b) pred_b = nullptr;                    // the layout of sums follows with_b, never the pointer (n = 0)
  const int F = with_b ? MMG_BOOT_FIELDS_B : MMG_BOOT_FIELDS;
  BootWs w;
  MMG_CHECK_WS("boot_sums", boot_carve(ws, n, replicates, F, &w));
  const RadixPairs<uint32_t>& kv = w.sort.kv;       // the sort leaves its result here
  hipStream_t st = (hipStream_t)stream;
  MMG_CHECK_HIP(mmg_zero_async(dropped, MMG_BOOT_DROP_KINDS * sizeof(int64_t), st), "boot_sums(zero)");
  const unsigned rblocks = (unsigned)((replicates + 1 + BT_RB - 1) / BT_RB);
  if (n > 0) {
    index_dispatch(index_bytes, [&](auto it) {
      using IT = decltype(it);
      hipLaunchKernelGGL(k_boot_keys<IT>, dim3(launch_grid(n, BT_NTHR, BT_MAX_GRID)), dim3(BT_NTHR), 0, st, pred, target,
                         pred_b, (const IT*)unit, (const IT*)seg, n, n_units, n_seg, kv.keys, kv.vals, w.unit32,
                         (unsigned long long*)dropped);
    });
    MMG_CHECK_LAUNCH("boot_sums(keys)");
    segsort_run(w.sort, n, bits_of((unsigned)n_seg), st);                // the key reaches n_seg itself
    MMG_CHECK_LAUNCH("boot_sums(sort)");
    const dim3 grid((unsigned)bt_chunks(n), rblocks);
    if (with_b)
      hipLaunchKernelGGL(k_boot_sums<true>, grid, dim3(BT_NTHR), 0, st, kv.keys, kv.vals, w.unit32, n, n_seg, pred, target,
                         pred_b, replicates, seed, w.part, sums);
    else
      hipLaunchKernelGGL(k_boot_sums<false>, grid, dim3(BT_NTHR), 0, st, kv.keys, kv.vals, w.unit32, n, n_seg, pred, target,
                         pred_b, replicates, seed, w.part, sums);
    MMG_CHECK_LAUNCH("boot_sums(chunks)");
  }
  const dim3 grid((unsigned)n_seg, rblocks);
  if (with_b)
    hipLaunchKernelGGL(k_boot_combine<MMG_BOOT_FIELDS_B>, grid, dim3(BT_NTHR), 0, st, kv.keys, n, n_seg, replicates, w.part,
                       sums);
  else
    hipLaunchKernelGGL(k_boot_combine<MMG_BOOT_FIELDS>, grid, dim3(BT_NTHR), 0, st, kv.keys, n, n_seg, replicates, w.part,
                       sums);
  MMG_CHECK_LAUNCH("boot_sums(combine)");
  return MMG_OK;
}

extern "C" int mmg_boot_metrics(const double* sums, int n_seg, int replicates, int with_b, double* metrics, void* stream) {
  int rc = shape_check("boot_metrics", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(sums && metrics, "boot_metrics: null sums or metrics");
  const int64_t cells = (int64_t)(replicates + 1) * (n_seg + 1);
  const dim3 grid(launch_grid(cells, BT_NTHR, BT_MAX_GRID, 1)), block(BT_NTHR);
  hipStream_t st = (hipStream_t)stream;
  if (with_b) hipLaunchKernelGGL(k_boot_metrics<true>, grid, block, 0, st, sums, n_seg, replicates, metrics);
  else hipLaunchKernelGGL(k_boot_metrics<false>, grid, block, 0, st, sums, n_seg, replicates, metrics);
  MMG_CHECK_LAUNCH("boot_metrics");
  return MMG_OK;
}

extern "C" int mmg_boot_summary(const double* metrics, int n_seg, int replicates, int with_b, double confidence,
                                double* summary, void* stream) {
  int rc = shape_check("boot_summary", n_seg, replicates);
  if (rc) return rc;
  MMG_CHECK_ARG(confidence > 0.0 && confidence < 1.0, "boot_summary: confidence %g outside (0, 1)", confidence);
  MMG_CHECK_ARG(metrics && summary, "boot_summary: null metrics or summary");
  const int M = with_b ? MMG_BOOT_METRICS_B : MMG_BOOT_METRICS;
  // numpy.percentile(x, p) works with q = p / 100 of p = 100 * ((1 -+ confidence) / 2)
  const double p_lo = (1.0 - confidence) / 2.0 * 100.0, p_hi = (1.0 + confidence) / 2.0 * 100.0;
  const double q_lo = p_lo / 100.0, q_hi = p_hi / 100.0;
  const int cells = (n_seg + 1) * M;
  hipLaunchKernelGGL(k_boot_summary, dim3((unsigned)(cells < 8192 ? cells : 8192)), dim3(BT_NTHR), 0, (hipStream_t)stream,
                     metrics, n_seg, replicates, M, q_lo, q_hi, summary);
  MMG_CHECK_LAUNCH("boot_summary");
  return MMG_OK;
}
