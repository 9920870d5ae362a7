// Dense layers.  Replaces nn.Linear (+ the BatchNorm/ReLU/Dropout in front of it) of src/model.py:93-105 and the
// lin_l / lin_r of PyG SAGEConv (call site src/model.py:125-131).
//
// fp32 products on the bf16 matrix cores, exactly: an fp32 value is the sum of three bf16 pieces (8 significant bits
// each) and x.w = x1w1 + (x1w2 + x2w1) + (x2w2 + x1w3 + x3w1) + O(2^-24 |x||w|) -- six v_mfma_f32_32x32x16_bf16 with
// fp32 accumulation per product tile (k_linear_fwd_x6, k_linear_wgrad_x6, k_linear_wgrad_ws).
// 6/16 of the fp32 matrix time turns the [P,128] x [128,128] layers from matrix-bound into HBM-bound.
//
// linear_fwd : Y[M,N] = prologue(X)[M,K] . W[N,K]^T + b.  The W pieces stay resident in registers; X tiles are
//              prologue'd and split ONCE while staged to three bf16 LDS planes (double-buffered, one barrier per
//              32-row tile).  k_linear_small serves the vocab-side tables (M <= 512).
// linear_wgrad: dW[N,K] = dY^T . prologue(X): contraction over the rows; every workgroup reduces a set of 32-row
//              stages into a [TN,TK] register tile, writes one partial slab, a second kernel sums the slabs in
//              fixed order (bitwise reproducible).  The bias gradient (column sums of dY) rides in the same pass.
#include "common.h"
#include "mma.h"

namespace {

// ---------------------------------------------------------------------------------- fp32 GEMM on the bf16 matrix cores
// The split (MMG_SPLIT3), its error bound and the six-product sequence (MMG_X6_ALO in every kernel here): mma.h.
// Layout: the three W pieces stay in registers for the whole kernel (lane (n = l&31, h = l>>5) holds
// W[n][16 ks + 8 h + 0..7]); every 64-row X tile is prologue'd AND split once while it is staged to LDS (three
// bf16 planes, double-buffered: tile t+1 is staged while tile t is multiplied, one barrier per tile), and an A
// fragment is one conflict-free ds_read_b128 per piece.

// XCD-aware block -> (tile, row-set) map for 2-D grids whose x index selects an output tile (a column slice of the
// forward, an [TN, TK] tile of the weight gradient) and whose y index selects the rows.  Every tile of one row-set reads
// the same rows of the streamed operand(s); workgroups are dealt round-robin over the 8 XCDs (linear id b and b + 8 share
// an XCD and its 4 MB L2, MI355X_MICROARCH.md), so with the natural map (x fastest) the tiles of a row-set land on
// DIFFERENT XCDs and every one of them fetches its rows from HBM.  Here ids 8 apart -- same XCD, dispatched together --
// become the tiles of one row-set: the first reader's lines are in L2 for the others.  Speed only: a bijection of the
// grid for gridDim.y % 8 == 0, the identity otherwise.
__device__ __forceinline__ void xcd_tile_map(int* bx, int* by) {
  const unsigned nx = gridDim.x, ny = gridDim.y;
  *bx = (int)blockIdx.x; *by = (int)blockIdx.y;
  if (nx > 1u && (ny & 7u) == 0u) {
    const unsigned L = blockIdx.x + nx * blockIdx.y, j = L >> 3;
    *bx = (int)(j % nx);
    *by = (int)((j / nx) * 8u + (L & 7u));
  }
}

// Memory pipeline: every global access goes through a per-tile buffer descriptor (rows past M and tiles past the end
// read 0 / are dropped by the range check), so the tile loop is straight-line code without a branch around a load or a
// store and the compiler's vmcnt waits are exact: X runs two tiles ahead in registers, the epilogue's stores are never
// waited for (gfx9 counts stores in vmcnt, in order: a conservative wait exposes the full store-acknowledge latency
// once per tile, which is what the first version of this kernel did), and in accumulate mode the old output tile is
// loaded INTO the accumulator before the next tile is staged, so its latency hides under the split.
// cache policy of the streamed operands (aux = 2: the `nt` bit -- X is read once, Y written once: -1.3 % on the step)
#ifndef MMG_NT_LD
#define MMG_NT_LD 2
#endif
#ifndef MMG_NT_ST
#define MMG_NT_ST 2
#endif
#ifndef MMG_NT_WG
#define MMG_NT_WG 0
#endif

// (NextBnDev and its epilogue arithmetic: common.h)
// the Y values of this lane's 16 tile elements; vo = byte offset of (row 4h, this lane's column) in the tile
__device__ __forceinline__ void next_bn_load(const NextBnDev& nb, int64_t tile, int rows, int N, int c0, int vo, float* yv) {
  const size_t off = (size_t)(rows ? tile : 0) * 32 * N + c0;
  const int bytes = rows ? (rows * N - c0) * 4 : 0;
  const __amdgpu_buffer_rsrc_t ysrc = mmg_rsrc(nb.Y + off, bytes);
#pragma unroll
  for (int i = 0; i < 16; ++i)
    yv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ysrc, vo, mmg_c_row(i) * N * 4, MMG_NT_LD));
}
// L2: the row L2 normalisation that follows the layer (F.normalize, src/model.py:232) in the epilogue -- the workgroup
// holds whole rows (N == 32 * WN), so Y receives  y / max(|y|, eps)  and rn_out[row] = 1 / max(|y|, eps); the separate
// pass read and wrote the [M, N] tensor once more.
// NBN: stat_partial receives the statistics of the NEXT BatchNorm backward (nb, see NextBnDev) instead of the forward ones.
// RIDER (L2 instances): a second, compact problem on the SAME W and bias rides in the launch -- the listed rows of another
// tensor under their own prologue (the first encode_nodes pass of a training step, which only feeds the tabular head: its
// third linear runs on the low-degree rows alone, mmg_linear_fwd_rider).  A workgroup walks its dense tiles t0, t0 + G, ...
// exactly as without the rider (same grid, same tile map, same code) and then goes on in the same round-robin over the
// rider's ceil(n_sel / 32) tiles: tile j of the rider is tile n_tiles + j of the walk.  A rider tile gathers its rows
// through the int64 list, applies mmg_pro_apply4 with the masks of the ORIGINAL rows (what k_affine_act_drop_rows does,
// and stores: act), splits, multiplies in the k-step order of the PRO = false instance and runs the same L2 epilogue into
// the compact outputs: act, Y and rn are bit for bit those of mmg_affine_act_drop_rows + the compact L2 launch.
struct FwdRiderDev {
  const float* X; ProDev pr; const int64_t* rows; int64_t n_sel; float* act; float* Y; float* rn;
};
static inline FwdRiderDev fwd_rider_none() { return FwdRiderDev{nullptr, mmg_pro_dev(nullptr), nullptr, 0, nullptr, nullptr, nullptr}; }

template <int K, int WN, bool PRO, bool ACC, bool L2 = false, bool NBN = false, bool RIDER = false>   // WN waves along N (32 columns each) over a 32-row tile: 64 * WN threads
__global__ __launch_bounds__(64 * WN, (WN == 4 && K <= 128) ? 2 : 1) void k_linear_fwd_x6(
    const float* __restrict__ X, ProDev pr, const float* __restrict__ W, const float* __restrict__ bias,
    float* __restrict__ Y, int64_t M, int N, int flags, double* __restrict__ stat_partial, float* __restrict__ rn_out,
    float l2_eps, NextBnDev nb, FwdRiderDev rd) {
  static_assert(!(NBN && L2), "one epilogue at a time");
  static_assert(!RIDER || (L2 && !ACC), "the rider comes with the L2 instances");
  __shared__ float l2_part[L2 ? WN * 32 : 1], l2_rn[L2 ? 32 : 1];
  if (PRO) pr.resolve();
  double cs1 = 0.0, cs2 = 0.0;          // column statistics of the output (BatchNorm batch stats) ride along: lane = column
  constexpr int LDP = K + 8;            // plane row stride in bf16 (K*2 + 16 bytes: fragment reads hit 64 distinct banks)
  constexpr int BN = 32 * WN, NK = K / 16, NTHR = 64 * WN, BM = 32;
  extern __shared__ __attribute__((aligned(16))) __bf16 planes[];     // [2 buffers][3 pieces][BM][LDP]
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  int bx, by;
  xcd_tile_map(&bx, &by);                 // (column slice, row-set): the slices of one row-set share an XCD's L2
  const int col = bx * BN + wn * 32 + l31;

  bf16x8 wb[NK][3];
  {
    const bool wkn = (flags & MMG_LIN_W_KN) != 0;
    const float* wp = wkn ? W + (size_t)(8 * h) * N + col : W + (size_t)col * K + 8 * h;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      f32x4 w0, w1;
      if (wkn) {
#pragma unroll
        for (int j = 0; j < 4; ++j) { w0[j] = wp[(size_t)(ks * 16 + j) * N]; w1[j] = wp[(size_t)(ks * 16 + 4 + j) * N]; }
      } else {
        w0 = *reinterpret_cast<const f32x4*>(wp + ks * 16); w1 = *reinterpret_cast<const f32x4*>(wp + ks * 16 + 4);
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = j < 4 ? w0[j] : w1[j - 4];
        MMG_SPLIT3(v, wb[ks][0][j], wb[ks][1][j], wb[ks][2][j]);
      }
    }
  }
  const float bv = bias ? bias[col] : 0.f;
  NextBnCol nbc = {};
  if constexpr (NBN) nbc = next_bn_col(nb, col);

  constexpr int K4 = K / 4;
  const int kc4 = tid % K4;                 // float4 column: this thread always touches the same 4 k's
  constexpr int ROWS_PER_PASS = NTHR / K4;
  constexpr int NP = BM / ROWS_PER_PASS;    // 16-B loads per thread per tile
  const int prow = tid / K4;
  // prologue constants, loaded once (identity when a part is absent: x*1+0, max(x,-inf))
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  float floor_v = -__builtin_inff();
  bool drop = false;
  if (PRO) {
    if (pr.scale) {
      sc = *reinterpret_cast<const f32x4*>(pr.scale + kc4 * 4);
      sh = *reinterpret_cast<const f32x4*>(pr.shift + kc4 * 4);
    }
    if (pr.relu) floor_v = 0.f;
    drop = pr.p > 0.f;
  }
  const int64_t n_tiles = (M + BM - 1) / BM;
  const int64_t G = gridDim.y, t0 = by;
  if (t0 >= n_tiles) return;
  const int n_my = (int)((n_tiles - t0 + G - 1) / G);      // tiles t0, t0+G, ... of this workgroup
  auto rows_of = [&](int64_t tile) -> int {                // valid rows of a tile (0 past the end)
    const int64_t r = M - tile * BM;
    return r <= 0 ? 0 : (r < BM ? (int)r : BM);
  };
  f32x4 nxa[NP], nxb[NP];                   // two tiles of X in flight: tiles alternate between them
  const int xvo = (prow * K + kc4 * 4) * 4;
  auto fetch = [&](int64_t tile, f32x4* nx) {
    const int rows = rows_of(tile);
    const __amdgpu_buffer_rsrc_t rs = mmg_rsrc(X + (size_t)(rows ? tile : 0) * BM * K, rows * K * 4);
#pragma unroll
    for (int p = 0; p < NP; ++p)
      nx[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
  };
  auto stage_pass = [&](int64_t tile, int buf, const f32x4* nx, int p) __attribute__((always_inline)) {   // one 16-B element per thread
    const int64_t row0 = tile * BM;
    __bf16* pb = planes + (size_t)buf * 3 * BM * LDP;
    {
      const int r = p * ROWS_PER_PASS + prow;
      f32x4 v = nx[p];
      if (PRO) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], sc[j], sh[j]), floor_v);
        if (drop)
          mmg_drop4(v, pr.key, (uint64_t)(pr.row_offset + row0 + r) * (uint64_t)K + (uint64_t)(kc4 * 4), pr.thr, pr.inv_keep);
      }
      bf16x4 q0, q1, q2;
#pragma unroll
      for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
      *reinterpret_cast<bf16x4*>(pb + (0 * BM + r) * LDP + kc4 * 4) = q0;
      *reinterpret_cast<bf16x4*>(pb + (1 * BM + r) * LDP + kc4 * 4) = q1;
      *reinterpret_cast<bf16x4*>(pb + (2 * BM + r) * LDP + kc4 * 4) = q2;
    }
  };
  auto stage = [&](int64_t tile, int buf, const f32x4* nx) __attribute__((always_inline)) {  // prologue + split + three plane writes
#pragma unroll
    for (int p = 0; p < NP; ++p) stage_pass(tile, buf, nx, p);
  };
  // K = 256 keeps ONE workgroup per CU (192 registers of W pieces per wave, 101 KB of planes): no second workgroup stages
  // its tile while this one multiplies, so the staging of tile t+1 is dealt out between the k-steps of tile t here (the
  // matrix pipe runs a 32 x 32 x 16 product for 32 clocks; the vector and LDS instructions of a staging pass issue in
  // its shadow).  The two tiles use different plane buffers, the barrier at the end of the tile orders both.
  constexpr bool WEAVE = (K >= 128) && !L2 && (NP <= NK) && (NK % NP == 0);
  fetch(t0, nxa);
  stage(t0, 0, nxa);
  fetch(t0 + G, nxa);
  fetch(t0 + 2 * G, nxb);
  __syncthreads();
  const int yvo = ((4 * h) * N + wn * 32 + l31) * 4;     // C/D map: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
  const int c0 = bx * BN;
  // (L2) the epilogue of one tile: acc -> Y rows through ys, 1 / max(norm, eps) of its rows -> rn_dst[r0 .. r0 + rows)
  auto l2_epilogue = [&](const f32x16& acc, const __amdgpu_buffer_rsrc_t ys, int rows, float* rn_dst, int64_t r0) __attribute__((always_inline)) {
    // row sums of squares: 32 lanes of a half-wave hold the 32 columns of this wave for 16 rows each; the WN waves'
    // partials meet in LDS, 32 threads turn them into 1 / max(norm, eps), every lane scales its 16 values
    float vv[16], ss[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) { vv[i] = acc[i] + bv; ss[i] = vv[i] * vv[i]; }
    // 32-lane sums on the vector ALU's data-parallel primitives (five v_add_f32 with a DPP operand per value; the
    // first version went through 80 ds_bpermute round trips per tile): xor 1, xor 2 inside a quad, mirror inside 8,
    // mirror inside 16, then the row total of lanes 0..15 broadcast onto lanes 16..31 -- those hold the half's sum
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float v = ss[i];
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));   // quad_perm [1,0,3,2]
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));   // quad_perm [2,3,0,1]
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));  // row_half_mirror
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));  // row_mirror
      v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x142, 0xA, 0xF, false)); // row_bcast:15 -> rows 1, 3
      ss[i] = v;
    }
    if (l31 == 31) {
#pragma unroll
      for (int i = 0; i < 16; ++i) l2_part[wn * 32 + (i & 3) + 8 * (i >> 2) + 4 * h] = ss[i];
    }
    __syncthreads();                       // partials complete; also: buf fully read, buf^1 fully written
    if (tid < 32) {
      float tot = l2_part[tid];
#pragma unroll
      for (int w = 1; w < WN; ++w) tot += l2_part[w * 32 + tid];
      const float rinv = 1.0f / fmaxf(sqrtf(tot), l2_eps);
      l2_rn[tid] = rinv;
      if (tid < rows) rn_dst[r0 + tid] = rinv;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int r = mmg_c_row(i);
      const float v = vv[i] * l2_rn[r + 4 * h];
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ys, yvo, r * N * 4, MMG_NT_ST);
    }
  };
  auto tile_body = [&](int64_t tt, int buf, f32x4* nx) {
    // nx holds tile tt+G (fetched two tiles ago); after staging it, the registers take tile tt+3G
    const int rows = rows_of(tt);
    const __amdgpu_buffer_rsrc_t ys = mmg_rsrc(Y + (size_t)(rows ? tt : 0) * BM * N + c0, rows ? (rows * N - c0) * 4 : 0);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i)
      acc[i] = ACC ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ys, yvo, mmg_c_row(i) * N * 4, 0))
                   : 0.f;
    float nby[NBN ? 16 : 1];
    if constexpr (NBN) next_bn_load(nb, tt, rows, N, c0, yvo, nby);   // in flight under the products
    if constexpr (!WEAVE) {
      stage(tt + G, buf ^ 1, nx);              // the other buffer: its readers passed the barrier of the last tile
      fetch(tt + 3 * G, nx);
      __builtin_amdgcn_sched_barrier(0);       // keep the fetch ahead of the matrix loop (the scheduler sinks it otherwise)
    }
    const __bf16* ap = planes + (size_t)buf * 3 * BM * LDP + l31 * LDP + 8 * h;
    if constexpr (!WEAVE) {
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + BM * LDP + ks * 16);
        const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(ap + 2 * BM * LDP + ks * 16);
        MMG_X6_ALO(acc, a1, a2, a3, wb[ks][0], wb[ks][1], wb[ks][2]);
      }
    } else {
      // A wave that is alone on its SIMD hides nothing by itself: the fragments of k-step ks+1 are fetched before the
      // products of k-step ks (their LDS latency then passes under six matrix instructions), and one staging pass of the
      // NEXT tile is dealt out between the products of every KS_PER_PASS-th k-step (sched_group_barrier: a dependent
      // MFMA chain issues one instruction per 32 clocks, the vector / LDS work of the pass issues in between).
      constexpr int KS_PER_PASS = NK / NP;
      bf16x8 fr[2][3];
      auto ldfrag = [&](int ks, bf16x8* f) __attribute__((always_inline)) {
        f[0] = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
        f[1] = *reinterpret_cast<const bf16x8*>(ap + BM * LDP + ks * 16);
        f[2] = *reinterpret_cast<const bf16x8*>(ap + 2 * BM * LDP + ks * 16);
      };
      ldfrag(0, fr[0]);
#pragma unroll
      for (int pg = 0; pg < NP; ++pg) {          // one scheduling region = the k-steps that carry one staging pass
#pragma unroll
        for (int kk = 0; kk < KS_PER_PASS; ++kk) {
          const int ks = pg * KS_PER_PASS + kk;
          if (ks + 1 < NK) ldfrag(ks + 1, fr[(ks + 1) & 1]);
          const bf16x8* f = fr[ks & 1];
          MMG_X6_ALO(acc, f[0], f[1], f[2], wb[ks][0], wb[ks][1], wb[ks][2]);
        }
        stage_pass(tt + G, buf ^ 1, nx, pg);
        // a lone wave hides 2-3 vector instructions behind a matrix instruction (profiles/probes/mfma_shadow): the pass
        // (~25 of them, ~45 with a prologue) is dealt out over all 6 * KS_PER_PASS products of its k-steps
        constexpr int NM = 6 * KS_PER_PASS, VPER = ((PRO ? 48 : 26) + NM - 1) / NM;
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
          if (i % 6 < 3) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);         // one fragment read of the next k-step
          __builtin_amdgcn_sched_group_barrier(0x002, VPER, 0);                     // a slice of the staging pass
          if (i >= NM - 3) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);       // its plane writes at the end
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    if constexpr (WEAVE) fetch(tt + 3 * G, nx);  // (its registers are free only now: two tiles stay in flight all the same)
    if constexpr (L2) {
      l2_epilogue(acc, ys, rows, rn_out, tt * BM);
      return;
    }
    if constexpr (NBN) {
      float vv[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        vv[i] = acc[i] + bv;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vv[i]), ys, yvo, mmg_c_row(i) * N * 4, MMG_NT_ST);
      }
      next_bn_tile(nb, nbc, vv, nby, rows, tt * BM, N, col, lane, cs1, cs2);
    } else {
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = mmg_c_row(i);
        const float v = acc[i] + bv;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ys, yvo, r * N * 4, MMG_NT_ST);
        const float vs = r + 4 * h < rows ? v : 0.f;
        t1 += vs; t2 = fmaf(vs, vs, t2);
      }
      if (stat_partial) { cs1 += (double)t1; cs2 += (double)t2; }     // 16 rows in fp32, tiles in fp64
    }
    __syncthreads();                         // buf fully read, buf^1 fully written
  };
  // A tile index past the end is harmless (zero-sized descriptors).  The first pair is peeled: the loop is then entered
  // with the same loads / stores in flight as on its back edge, and the wait counts the compiler derives (the minimum
  // over both edges) are the steady-state ones.
  tile_body(t0, 0, nxa);
  tile_body(t0 + G, 1, nxb);
  for (int i = 2; i < n_my; i += 2) {
    tile_body(t0 + (int64_t)i * G, 0, nxa);
    tile_body(t0 + (int64_t)(i + 1) * G, 1, nxb);
  }
  if constexpr (RIDER) {
    // the rider's tiles, dealt on in the same round-robin: tile j is tile n_tiles + j of the walk.  Every wave is past the
    // barriers of its last dense tile: the planes are free (what the last staging passes left there is never read).
    rd.pr.resolve();
    f32x4 rsc = {1.f, 1.f, 1.f, 1.f}, rsh = {0.f, 0.f, 0.f, 0.f};
    if (rd.pr.scale) {
      rsc = *reinterpret_cast<const f32x4*>(rd.pr.scale + kc4 * 4);
      rsh = *reinterpret_cast<const f32x4*>(rd.pr.shift + kc4 * 4);
    }
    const int64_t nt_r = (rd.n_sel + BM - 1) / BM;
    for (int64_t j = t0 + (int64_t)n_my * G - n_tiles; j < nt_r; j += G) {
      const int64_t s0 = j * BM;
      const int rows = rd.n_sel - s0 < BM ? (int)(rd.n_sel - s0) : BM;
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const int r = p * ROWS_PER_PASS + prow;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};            // rows past the end of the list: what the compact launch reads there
        if (r < rows) {
          const int64_t row = rd.rows[s0 + r];
          v = *reinterpret_cast<const f32x4*>(rd.X + (size_t)row * K + kc4 * 4);
          mmg_pro_apply4(rd.pr, v, rsc, rsh, row, kc4 * 4, K);
          *reinterpret_cast<f32x4*>(rd.act + (size_t)(s0 + r) * K + kc4 * 4) = v;
        }
        bf16x4 q0, q1, q2;
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) MMG_SPLIT3(v[jj], q0[jj], q1[jj], q2[jj]);
        *reinterpret_cast<bf16x4*>(planes + (0 * BM + r) * LDP + kc4 * 4) = q0;
        *reinterpret_cast<bf16x4*>(planes + (1 * BM + r) * LDP + kc4 * 4) = q1;
        *reinterpret_cast<bf16x4*>(planes + (2 * BM + r) * LDP + kc4 * 4) = q2;
      }
      __syncthreads();
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const __bf16* ap = planes + l31 * LDP + 8 * h;
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
        const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + BM * LDP + ks * 16);
        const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(ap + 2 * BM * LDP + ks * 16);
        MMG_X6_ALO(acc, a1, a2, a3, wb[ks][0], wb[ks][1], wb[ks][2]);
      }
      // (the first barrier of the epilogue: the planes are read; its second: the next tile may be staged)
      l2_epilogue(acc, mmg_rsrc(rd.Y + (size_t)s0 * N + c0, (rows * N - c0) * 4), rows, rd.rn, s0);
    }
  }
  if (stat_partial) {
    // two partials per column (the lane halves) -> one: partial[row-set][2][N], fixed order
    double* red = reinterpret_cast<double*>(planes);          // the planes are dead: every wave passed the last barrier
    red[(h * 2 + 0) * BN + wn * 32 + l31] = cs1;
    red[(h * 2 + 1) * BN + wn * 32 + l31] = cs2;
    __syncthreads();
    for (int e = tid; e < 2 * BN; e += NTHR) {
      const int which = e / BN, c = e % BN;
      stat_partial[((size_t)by * 2 + which) * N + bx * BN + c] = red[which * BN + c] + red[(2 + which) * BN + c];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// k_linear_fwd_h3_k256 (round 4): the same layer on THREE f16 products instead of six bf16 ones -- half the matrix
// instructions of a shape that is matrix-bound.  Every row of X and every row of W (an output column) gets its own power
// of two: X = x * 2^ex with the row's largest magnitude in [2^13, 2^14), likewise W = w * 2^ew; each is split into
//   hi = f16(V),  lo = f16((V - hi) * 2^11)          (22 significant bits; the low piece is scaled up by 2^11 so that it
// is a NORMAL f16 wherever hi is: |V| >= 2^-14, i.e. within 2^-27 of the row's largest magnitude), and
//   x . w * 2^(ex + ew) = Xh Wh + 2^-11 (Xh Wl + Xl Wh) + O(2^-22 |X||W|):
// the first product goes to one fp32 accumulator, the two cross terms to a second one, combined and unscaled in the
// epilogue.  The dropped Xl Wl is 2^-22 of a product, as are the two roundings of the low pieces: ~3 * 2^-22 = 7e-7 per
// product against 2^-24 for the six-term bf16 split -- tests/test_ops_gpu.py holds the layer to 2e-6 of an fp64 reference
// like the other kernels.  A row's scale comes from the row itself (wave = row while a tile is staged: one DPP reduction),
// so the operand range is the fp32 range; an element more than 2^27 below its row's maximum loses relative precision, but
// what it can add to a dot product with that row is below the rounding of the fp32 sum.  inf / NaN in a row of X: NaN in that
// row of Y (as the bf16 kernels).  One workgroup of eight waves owns all 256 output columns (a wave: one 32-column tile, its W
// pieces -- 128 registers -- resident; two waves per SIMD) and persists over 32-row tiles of X dealt round-robin: a tile is
// staged ONCE per CU (prologue, row scale, split, two f16 planes in LDS, double-buffered), the staging of tile t+1 is woven
// between the products of tile t, two tiles of X are in flight in registers.  Round 3's six-term kernel for this shape (four
// waves, two column tiles and 384 registers of W pieces per wave) measured 147 us per [183400, 256] x [256, 256] call, this
// one 102-112 (179 -> 122 with BatchNorm fold + ReLU + dropout in the prologue); its parts add up -- staging and epilogue
// alone 48 us, + matrix instructions 32, + memory 29 -- the two waves of a SIMD run the same phase between the per-tile barriers.

// exponent e with  m * 2^e in [2^13, 2^14)  for a normal m (0 for zero / denormal / inf / NaN), from the exponent field of m:
// integer arithmetic only, so that a wave-uniform m (wave_max_dpp) keeps all of it on the scalar unit
__device__ __forceinline__ int h3_exponent(float m) {
  const int E = (int)((__builtin_bit_cast(unsigned, m) >> 23) & 0xFFu);     // m = 1.f * 2^(E - 127)
  const int e = 140 - E;
  return (E == 0 || E == 255) ? 0 : (e > 126 ? 126 : e);
}

template <int PRO, bool ACC, bool STATS, int WN>      // WN = 4: two column tiles per wave; 8: one (two waves per SIMD)
__global__ __launch_bounds__(64 * WN, 1) void k_linear_fwd_h3_k256(
    const float* __restrict__ X, ProDev pr, const float* __restrict__ W, const float* __restrict__ bias,
    float* __restrict__ Y, int64_t M, int N, int flags, double* __restrict__ stat_partial) {
  constexpr int K = 256, CT = 8 / WN, LDP = K + 8, BN = 256, NK = K / 16, NTHR = 64 * WN, BM = 32;
  constexpr int PLANE = BM * LDP;            // one piece of one buffer, in f16 elements
  if (PRO) pr.resolve();
  extern __shared__ __attribute__((aligned(16))) _Float16 hplanes[];     // [2 buffers][2 pieces][BM][LDP], then float ex2[2][BM]
  float* rowf = reinterpret_cast<float*>(hplanes + 2 * 2 * PLANE);       // 2^-ex of the staged rows, per buffer
  const int tid = threadIdx.x, lane = tid & 63;
  const int wn = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int h = lane >> 5, l31 = lane & 31;
  const int bx = blockIdx.x, by = blockIdx.y;
  const int c0 = bx * BN;
  f16x8 wh[CT][NK], wl[CT][NK];
  float bv[CT], cf[CT];                      // bias and 2^-ew of this lane's two columns
  {
    const bool wkn = (flags & MMG_LIN_W_KN) != 0;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int col = c0 + (wn * CT + ct) * 32 + l31;
      bv[ct] = bias ? bias[col] : 0.f;
      const float* wp = wkn ? W + (size_t)(8 * h) * N + col : W + (size_t)col * K + 8 * h;
      float wv[NK][8];
      float m = 0.f;
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        if (wkn) {
#pragma unroll
          for (int j = 0; j < 8; ++j) wv[ks][j] = wp[(size_t)(ks * 16 + j) * N];
        } else {
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + ks * 16), w1 = *reinterpret_cast<const f32x4*>(wp + ks * 16 + 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) { wv[ks][j] = w0[j]; wv[ks][4 + j] = w1[j]; }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float a = fabsf(wv[ks][j]);
          m = fmaxf(m, a < __builtin_inff() ? a : 0.f);
        }
      }
      m = fmaxf(m, __shfl_xor(m, 32, 64));             // the other half of the column's K (lane ^ 32)
      const int ew = h3_exponent(m);
      const float sw = mmg_pow2(ew > 126 ? 126 : ew);
      cf[ct] = mmg_pow2(-(ew > 126 ? 126 : ew));
#pragma unroll
      for (int ks = 0; ks < NK; ++ks)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float v = wv[ks][j] * sw;
          const _Float16 a = (_Float16)v;
          wh[ct][ks][j] = a;
          wl[ct][ks][j] = (_Float16)((v - (float)a) * 2048.f);
        }
    }
  }
  constexpr int K4 = K / 4, ROWS_PER_PASS = NTHR / K4, NP = BM / ROWS_PER_PASS;      // 64 quads, 4 rows per pass, 8 passes
  constexpr int KPP = NK / NP;               // k-steps per staging pass (2 | 4)
  static_assert(NK % NP == 0 && K4 == 64, "a staging pass every KPP k-steps; a wave stages one row per pass");
  const int kc4 = lane, prow = wn;           // (tid % K4, tid / K4)
  float floor_v = -__builtin_inff();
  bool drop = false;
  if (PRO) {
    if (pr.relu) floor_v = 0.f;
    drop = pr.p > 0.f;
  }
  const int64_t n_tiles = (M + BM - 1) / BM;
  const int64_t G = gridDim.y, t0 = by;
  if (t0 >= n_tiles) return;
  const int n_my = (int)((n_tiles - t0 + G - 1) / G);
  auto rows_of = [&](int64_t tile) -> int {
    const int64_t r = M - tile * BM;
    return r <= 0 ? 0 : (r < BM ? (int)r : BM);
  };
  auto x_rsrc = [&](int64_t tile) __attribute__((always_inline)) {
    const int rows = rows_of(tile);
    return mmg_rsrc(X + (size_t)(rows ? tile : 0) * BM * K, rows * K * 4);
  };
  const int xvo = (prow * K + kc4 * 4) * 4;
  // TWO tiles of X in registers (the six-term kernel had room for one): a workgroup per CU with one 32 KB tile in flight
  // is 8 MB on the chip -- at ~2 us of loaded HBM latency a ceiling of ~4 TB/s; the freed W-piece registers hold the second
  f32x4 nx[2][NP];
  auto fetch_pass = [&](__amdgpu_buffer_rsrc_t rs, int slot, int p) __attribute__((always_inline)) {
    nx[slot][p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
  };
  auto stage_pass = [&](int64_t tile, int buf, int slot, int p) __attribute__((always_inline)) {
    const int64_t row0 = tile * BM;
    _Float16* pb = hplanes + (size_t)buf * 2 * PLANE;
    const int r = p * ROWS_PER_PASS + prow;
    f32x4 v = nx[slot][p];
    if (PRO) {
      f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
      if (PRO == 2 || pr.scale) {
        sc = *reinterpret_cast<const f32x4*>(pr.scale + kc4 * 4);
        sh = *reinterpret_cast<const f32x4*>(pr.shift + kc4 * 4);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], sc[j], sh[j]), floor_v);
      if (PRO == 2 || drop)
        mmg_drop4(v, pr.key, (uint64_t)(pr.row_offset + row0 + r) * (uint64_t)K + (uint64_t)(kc4 * 4), pr.thr, pr.inv_keep);
    }
    // the row's scale: this wave holds the whole row (64 quads)
    float m = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fmaxf(fabsf(v[2]), fabsf(v[3])));
    m = wave_max_dpp(m);
    const int ex = h3_exponent(m);
    const float sx = mmg_pow2(ex);
    f16x4 qh, ql;
#pragma unroll
    for (int j = 0; j < 4; j += 2) {
      const f32x2 a = {v[j] * sx, v[j + 1] * sx};
      const f16x2 hh = __builtin_convertvector(a, f16x2);
      const f32x2 rr = {(a[0] - (float)hh[0]) * 2048.f, (a[1] - (float)hh[1]) * 2048.f};
      const f16x2 ll = __builtin_convertvector(rr, f16x2);
      qh[j] = hh[0]; qh[j + 1] = hh[1]; ql[j] = ll[0]; ql[j + 1] = ll[1];
    }
    *reinterpret_cast<f16x4*>(pb + (0 * BM + r) * LDP + kc4 * 4) = qh;
    *reinterpret_cast<f16x4*>(pb + (1 * BM + r) * LDP + kc4 * 4) = ql;
    if (lane == 0) rowf[buf * BM + r] = mmg_pow2(-ex);
  };
  {
    const __amdgpu_buffer_rsrc_t r0 = x_rsrc(t0), r1 = x_rsrc(t0 + G), r2 = x_rsrc(t0 + 2 * G);
#pragma unroll
    for (int p = 0; p < NP; ++p) fetch_pass(r0, 0, p);
#pragma unroll
    for (int p = 0; p < NP; ++p) fetch_pass(r1, 1, p);
#pragma unroll
    for (int p = 0; p < NP; ++p) { stage_pass(t0, 0, 0, p); fetch_pass(r2, 0, p); }
  }
  __syncthreads();
  double cs1[CT] = {}, cs2[CT] = {};
  // (two tiles per trip: the register slot of a tile is its parity, a compile-time index)
  for (int i2 = 0; i2 < n_my; i2 += 2) {
#pragma unroll
  for (int par = 0; par < 2; ++par) {
    const int i = i2 + par;
    if (i >= n_my) break;
    const int64_t tt = t0 + (int64_t)i * G;
    const int buf = par;
    const int rows = rows_of(tt);
    const __amdgpu_buffer_rsrc_t ys = mmg_rsrc(Y + (size_t)(rows ? tt : 0) * BM * N + c0, rows ? (rows * N - c0) * 4 : 0);
    const __amdgpu_buffer_rsrc_t xs3 = x_rsrc(tt + 3 * G);     // refills: three tiles ahead (slot of tile t + 1)
    f32x16 ah[CT], al[CT];
    float yold[ACC ? CT : 1][16];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int yvo = ((4 * h) * N + (wn * CT + ct) * 32 + l31) * 4;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ah[ct][r] = 0.f; al[ct][r] = 0.f;
        if (ACC) yold[ct][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ys, yvo, mmg_c_row(r) * N * 4, 0));
      }
    }
    const _Float16* ap = hplanes + (size_t)buf * 2 * PLANE + l31 * LDP + 8 * h;
    f16x8 fr[2][2];
    auto ldfrag = [&](int ks, f16x8* f) __attribute__((always_inline)) {
      f[0] = *reinterpret_cast<const f16x8*>(ap + ks * 16);
      f[1] = *reinterpret_cast<const f16x8*>(ap + PLANE + ks * 16);
    };
    ldfrag(0, fr[0]);
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const bool pass = (ks % KPP) == KPP - 1;
      if (ks + 1 < NK) ldfrag(ks + 1, fr[(ks + 1) & 1]);
      const f16x8* f = fr[ks & 1];
#pragma unroll
      for (int ct = 0; ct < CT; ++ct) {
        al[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[1], wh[ct][ks], al[ct], 0, 0, 0);   // Xl Wh
        al[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[0], wl[ct][ks], al[ct], 0, 0, 0);   // Xh Wl
        ah[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f[0], wh[ct][ks], ah[ct], 0, 0, 0);   // Xh Wh

      }
      if (pass) { stage_pass(tt + G, buf ^ 1, par ^ 1, ks / KPP); fetch_pass(xs3, par ^ 1, ks / KPP); }
#pragma unroll
      for (int q = 0; q < 3 * CT; ++q) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                          // one MFMA
        if (q < 2) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);               // a fragment read of the next k-step
        if (pass) __builtin_amdgcn_sched_group_barrier(0x002, (PRO ? 72 : 42) / (3 * CT), 0);   // a slice of the staging pass
        if (pass && q >= 3 * CT - 3 && q < 3 * CT - 1) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);   // its plane writes
        if (pass && q == 3 * CT - 1) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);      // the refill load
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    // epilogue: y = (ah + 2^-11 al) * 2^-ex[row] * 2^-ew[col] + bias (+ the old tile)
    const float* rf = rowf + buf * BM + 4 * h;
    f32x4 rf4[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) rf4[g4] = *reinterpret_cast<const f32x4*>(rf + 8 * g4);
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int yvo = ((4 * h) * N + (wn * CT + ct) * 32 + l31) * 4;
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int r16 = 0; r16 < 16; ++r16) {
        const int r = mmg_c_row(r16);
        float v = fmaf(al[ct][r16], 1.f / 2048.f, ah[ct][r16]) * (rf4[r16 >> 2][r16 & 3] * cf[ct]) + bv[ct];
        if (ACC) v += yold[ct][r16];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ys, yvo, r * N * 4, MMG_NT_ST);
        if (STATS) {
          const float vs = r + 4 * h < rows ? v : 0.f;
          t1 += vs; t2 = fmaf(vs, vs, t2);
        }
      }
      if (STATS) { cs1[ct] += (double)t1; cs2[ct] += (double)t2; }
    }
    __syncthreads();                         // buf fully read, buf^1 fully written
  }
  }
  if (STATS) {
    double* red = reinterpret_cast<double*>(hplanes);         // the planes are dead: every wave passed the last barrier
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      red[(h * 2 + 0) * BN + (wn * CT + ct) * 32 + l31] = cs1[ct];
      red[(h * 2 + 1) * BN + (wn * CT + ct) * 32 + l31] = cs2[ct];
    }
    __syncthreads();
    for (int e = tid; e < 2 * BN; e += NTHR) {
      const int which = e / BN, c = e % BN;
      stat_partial[((size_t)by * 2 + which) * N + c0 + c] = red[which * BN + c] + red[(2 + which) * BN + c];
    }
  }
}

template <int PRO, bool ACC, bool STATS>
int launch_fwd_h3_k256_vs(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                          int flags, hipStream_t st, double* stat_partial, int64_t gy) {
  constexpr int lds = 2 * 2 * 32 * (256 + 8) * 2 + 2 * 32 * 4;
  // eight waves (WN = 4 -- two column tiles per wave, 424+ registers -- measured 122 us against 108); the literal is
  // written out so that the probe records the instantiated symbol
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_fwd_h3_k256<PRO, ACC, STATS, 8>, lds>::set()), "linear_fwd(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, 256, (flags & MMG_LIN_ACCUMULATE) | (PRO ? 4 : 0),
             (k_linear_fwd_h3_k256<PRO, ACC, STATS, 8>), dim3((unsigned)(N / 256), (unsigned)gy), dim3(64 * 8), lds, st, X, pr,
             W, bias, Y, M, N, flags, stat_partial);
  return 0;
}
template <int PRO, bool ACC>
int launch_fwd_h3_k256_v(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                         int flags, hipStream_t st, double* stat_partial, int64_t gy) {
  return stat_partial ? launch_fwd_h3_k256_vs<PRO, ACC, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy)
                      : launch_fwd_h3_k256_vs<PRO, ACC, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy);
}

// rows of partial statistics = grid.y of the K = 256, 256-column kernel
inline int64_t fwd_k256_rows(int64_t M, int N) {
  const int64_t n_tiles = (M + 31) / 32;
  int64_t gy = 256 / (N / 256);
  if (gy < 1) gy = 1;
  return gy > n_tiles ? n_tiles : gy;
}

int launch_fwd_h3_k256(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                       int flags, hipStream_t st, double* stat_partial) {
  const bool pro = pr.scale || pr.relu || pr.p > 0.f, acc = (flags & MMG_LIN_ACCUMULATE) != 0;
  const int64_t gy = fwd_k256_rows(M, N);
  if (pro && pr.scale && pr.p > 0.f)
    return acc ? launch_fwd_h3_k256_v<2, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy)
               : launch_fwd_h3_k256_v<2, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy);
  if (pro) return acc ? launch_fwd_h3_k256_v<1, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy)
                      : launch_fwd_h3_k256_v<1, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy);
  return acc ? launch_fwd_h3_k256_v<0, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy)
             : launch_fwd_h3_k256_v<0, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, gy);
}

inline int64_t fwd_x6_rows(int64_t M, int N, int BN, int K = 128) {   // grid.y of the bf16-split forward (= partial stat rows)
  const int n_slices = N / BN;
  const int64_t n_tiles = (M + 31) / 32;
  // persistent workgroups: two per CU (52 KB of LDS, <= 256 registers) up to K = 128; K = 256 keeps 192 registers of
  // W pieces per wave and 101 KB of planes: one per CU
  // (a 64-column workgroup is two waves: three of them fit a CU -- 52 KB of planes, <= 256 registers -- and a layer with
  //  N = 64 has a single slice, so 768 workgroups instead of 512 put six waves on every CU)
  int64_t gy = (K <= 128 ? (BN == 64 ? 768 : 512) : 256) / n_slices;
  if (gy < 1) gy = 1;
  if (gy > n_tiles) gy = n_tiles;
  return gy;
}

template <int K, int WN, bool PRO, bool ACC, bool L2 = false, bool NBN = false>
int launch_fwd_x6_v(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                    int flags, hipStream_t st, double* stat_partial, float* rn_out = nullptr, float l2_eps = 0.f,
                    const NextBnDev& nb = next_bn_none()) {
  constexpr int BN = 32 * WN;
  const int n_slices = N / BN;
  const int64_t gy = fwd_x6_rows(M, N, BN, K);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_fwd_x6<K, WN, PRO, ACC, L2, NBN>, lds>::set()), "linear_fwd(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, (flags & MMG_LIN_ACCUMULATE) | (PRO ? 4 : 0) | (L2 ? 32 : 0) | (NBN ? 512 : 0),
             (k_linear_fwd_x6<K, WN, PRO, ACC, L2, NBN>), dim3((unsigned)n_slices, (unsigned)gy), dim3(64 * WN), lds, st, X,
             pr, W, bias, Y, M, N, flags, stat_partial, rn_out, l2_eps, nb, fwd_rider_none());
  return 0;
}

// the L2 launch of a [M, 128] x [128, 128] layer with a rider (mmg_linear_fwd_rider): the dense launch's grid and LDS
int launch_fwd_x6_rider(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M,
                        hipStream_t st, float* rn_out, float l2_eps, const FwdRiderDev& rd) {
  constexpr int K = 128, N = 128;
  const int64_t gy = fwd_x6_rows(M, N, 128, K);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_fwd_x6<128, 4, true, false, true, false, true>, lds>::set()), "linear_fwd_rider(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, 4 | 32 | 32768, (k_linear_fwd_x6<128, 4, true, false, true, false, true>),
             dim3(1u, (unsigned)gy), dim3(256), lds, st, X, pr, W, bias, Y, M, N, 0, nullptr, rn_out, l2_eps, next_bn_none(), rd);
  return 0;
}

// PRO / ACC from the prologue and the flags; the forward statistics when stat_partial is set.  epi = MMG_EPI_L2 / _NEXT_BN
// (the caller checked that the launch takes them) pick the instances with that epilogue: K <= 128, no accumulate, and for
// NEXT_BN no prologue and 128-column slices, stat_partial then receiving the next BatchNorm's partial rows
template <int K, int WN>
int launch_fwd_x6(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                  int flags, hipStream_t st, double* stat_partial, int epi, float* rn_out, float l2_eps, const NextBnDev& nb) {
  const bool pro = pr.scale || pr.relu || pr.p > 0.f, acc = (flags & MMG_LIN_ACCUMULATE) != 0;
  if constexpr (K <= 128) {
    if (epi == MMG_EPI_L2)
      return pro ? launch_fwd_x6_v<K, WN, true, false, true>(X, pr, W, bias, Y, M, N, flags, st, nullptr, rn_out, l2_eps)
                 : launch_fwd_x6_v<K, WN, false, false, true>(X, pr, W, bias, Y, M, N, flags, st, nullptr, rn_out, l2_eps);
    if constexpr (WN == 4)
      if (epi == MMG_EPI_NEXT_BN)
        return launch_fwd_x6_v<K, 4, false, false, false, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial, nullptr, 0.f, nb);
  }
  if (pro) return acc ? launch_fwd_x6_v<K, WN, true, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial)
                      : launch_fwd_x6_v<K, WN, true, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial);
  return acc ? launch_fwd_x6_v<K, WN, false, true>(X, pr, W, bias, Y, M, N, flags, st, stat_partial)
             : launch_fwd_x6_v<K, WN, false, false>(X, pr, W, bias, Y, M, N, flags, st, stat_partial);
}

// ---------------------------------------------------------------------------------------------------------------------
// k_linear_fwd_x6_dual: the SAME [M, 128] x [128, 128] layer under two dropout masks in one launch -- the encoder's second
// linear of the two encode_nodes passes of a training step.  The passes share X, the BatchNorm fold, the ReLU and
// inv_keep; only the RNG site differs, so a staged element is  v * inv_keep  where its pass keeps it and zero where not.
// Every 16-byte element is loaded once, affine + ReLU + scaling + MMG_SPLIT3 run once, the two passes' keep fields mask
// the three pieces (split(0) = three +0 pieces: the bits k_linear_fwd_x6 stages for a dropped element), six plane writes.
// Eight waves: waves 0..3 multiply the planes of pass 0 and waves 4..7 those of pass 1, each with the W pieces of its 32
// columns in registers and the products of k_linear_fwd_x6<128, 4, true, false> in the same k-step order, so Y and the
// statistics partials of a pass are that kernel's, bit for bit.  A workgroup walks row sets  blockIdx.x, + gridDim.x, ...
// of the n_sets = fwd_x6_rows(M, 128, 128) the single launch has (tiles by, by + n_sets, ... in that order) and writes
// partial[by][2][128] of each pass as the single kernel does.  Loads and stores go through per-tile buffer descriptors
// (no branch around them), one barrier per tile, the first tile pair peeled -- see k_linear_fwd_x6.
__global__ __launch_bounds__(512, 1) void k_linear_fwd_x6_dual(
    const float* __restrict__ X, ProDev pr, ProDev prb, const float* __restrict__ W, const float* __restrict__ bias,
    float* __restrict__ Y0, float* __restrict__ Y1, int64_t M, int n_sets, double* __restrict__ part0,
    double* __restrict__ part1) {
  constexpr int K = 128, N = 128, BN = 128, LDP = K + 8, NK = K / 16, NTHR = 512, BM = 32;
  constexpr int PLANE = BM * LDP;            // one piece of one pass of one buffer, in bf16 elements
  pr.resolve();
  prb.resolve();
  extern __shared__ __attribute__((aligned(16))) __bf16 planes[];     // [2 buffers][2 passes][3 pieces][BM][LDP]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pass = wv >> 2, wn = wv & 3;
  const int h = lane >> 5, l31 = lane & 31;
  const int col = wn * 32 + l31;
  float* __restrict__ const Y = pass ? Y1 : Y0;
  double* __restrict__ const stat_partial = pass ? part1 : part0;

  bf16x8 wb[NK][3];
  {
    const float* wp = W + (size_t)col * K + 8 * h;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp + ks * 16), w1 = *reinterpret_cast<const f32x4*>(wp + ks * 16 + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = j < 4 ? w0[j] : w1[j - 4];
        MMG_SPLIT3(v, wb[ks][0][j], wb[ks][1][j], wb[ks][2][j]);
      }
    }
  }
  const float bv = bias ? bias[col] : 0.f;

  constexpr int K4 = K / 4, ROWS_PER_PASS = NTHR / K4, NP = BM / ROWS_PER_PASS;      // 32 quads, 16 rows per pass, 2 passes
  constexpr int KS_PER_PASS = NK / NP;
  const int kc4 = tid % K4, prow = tid / K4;
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  if (pr.scale) {
    sc = *reinterpret_cast<const f32x4*>(pr.scale + kc4 * 4);
    sh = *reinterpret_cast<const f32x4*>(pr.shift + kc4 * 4);
  }
  const float floor_v = pr.relu ? 0.f : -__builtin_inff();
  const uint32_t thr = pr.thr, key0 = pr.key, key1 = prb.key;
  const float inv_keep = pr.inv_keep;
  const int64_t n_tiles = (M + BM - 1) / BM;
  const int64_t G = n_sets;
  auto rows_of = [&](int64_t tile) -> int {
    const int64_t r = M - tile * BM;
    return r <= 0 ? 0 : (r < BM ? (int)r : BM);
  };
  const int xvo = (prow * K + kc4 * 4) * 4;
  auto fetch = [&](int64_t tile, f32x4* nx) {
    const int rows = rows_of(tile);
    const __amdgpu_buffer_rsrc_t rs = mmg_rsrc(X + (size_t)(rows ? tile : 0) * BM * K, rows * K * 4);
#pragma unroll
    for (int p = 0; p < NP; ++p)
      nx[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
  };
  // 16-bit lanes of a piece pair kept (all ones) or dropped (zero): fields 0, 1 of a hash word against the threshold
  auto keep_mask = [&](uint32_t w) __attribute__((always_inline)) -> uint32_t {
    return ((w & 0xFFFFu) >= thr ? 0x0000FFFFu : 0u) | ((w >> 16) >= thr ? 0xFFFF0000u : 0u);
  };
  auto stage_pass = [&](int64_t tile, int buf, const f32x4* nx, int p) __attribute__((always_inline)) {
    const int r = p * ROWS_PER_PASS + prow;
    __bf16* pb = planes + (size_t)buf * 6 * PLANE + r * LDP + kc4 * 4;
    f32x4 v = nx[p];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float s = fmaxf(fmaf(v[j], sc[j], sh[j]), floor_v) * inv_keep;
      // the ROUNDED product is what gets split: in k_linear_fwd_x6 the dropout select stands between this multiply and the
      // split's subtraction; without it the compiler contracts the two into one fma (an exact product minus the high
      // piece) and the middle and low pieces come out an ulp off.  An empty asm keeps the multiply a multiply.
      asm("" : "+v"(s));
      v[j] = s;
    }
    const uint64_t grp = ((uint64_t)(pr.row_offset + tile * BM + r) * (uint64_t)K + (uint64_t)(kc4 * 4)) >> 2;
    uint32_t a0, a1, b0, b1;
    mmg_rng_group(key0, grp, &a0, &a1);
    mmg_rng_group(key1, grp, &b0, &b1);
    bf16x4 q[3];
#pragma unroll
    for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q[0][j], q[1][j], q[2][j]);
    const u32x2 ma = {keep_mask(a0), keep_mask(a1)}, mb = {keep_mask(b0), keep_mask(b1)};
#pragma unroll
    for (int pc = 0; pc < 3; ++pc) {
      const u32x2 bits = __builtin_bit_cast(u32x2, q[pc]);
      *reinterpret_cast<u32x2*>(pb + pc * PLANE) = bits & ma;
      *reinterpret_cast<u32x2*>(pb + (3 + pc) * PLANE) = bits & mb;
    }
  };
  const int yvo = ((4 * h) * N + col) * 4;     // C/D map: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)

  for (int by = blockIdx.x; by < n_sets; by += gridDim.x) {
    const int64_t t0 = by;
    const int n_my = (int)((n_tiles - t0 + G - 1) / G);      // tiles t0, t0+G, ... of this row set
    double cs1 = 0.0, cs2 = 0.0;
    f32x4 nxa[NP], nxb[NP];                   // two tiles of X in flight: tiles alternate between them
    fetch(t0, nxa);
#pragma unroll
    for (int p = 0; p < NP; ++p) stage_pass(t0, 0, nxa, p);
    fetch(t0 + G, nxa);
    fetch(t0 + 2 * G, nxb);
    __syncthreads();
    auto tile_body = [&](int64_t tt, int buf, f32x4* nx) {
      // nx holds tile tt+G (fetched two tiles ago); after staging it, the registers take tile tt+3G
      const int rows = rows_of(tt);
      const __amdgpu_buffer_rsrc_t ys = mmg_rsrc(Y + (size_t)(rows ? tt : 0) * BM * N, rows * N * 4);
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      const __bf16* ap = planes + (size_t)(buf * 6 + pass * 3) * PLANE + l31 * LDP + 8 * h;
      bf16x8 fr[2][3];
      auto ldfrag = [&](int ks, bf16x8* f) __attribute__((always_inline)) {
        f[0] = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
        f[1] = *reinterpret_cast<const bf16x8*>(ap + PLANE + ks * 16);
        f[2] = *reinterpret_cast<const bf16x8*>(ap + 2 * PLANE + ks * 16);
      };
      ldfrag(0, fr[0]);
#pragma unroll
      for (int pg = 0; pg < NP; ++pg) {          // one scheduling region = the k-steps that carry one staging pass
#pragma unroll
        for (int kk = 0; kk < KS_PER_PASS; ++kk) {
          const int ks = pg * KS_PER_PASS + kk;
          if (ks + 1 < NK) ldfrag(ks + 1, fr[(ks + 1) & 1]);
          const bf16x8* f = fr[ks & 1];
          MMG_X6_ALO(acc, f[0], f[1], f[2], wb[ks][0], wb[ks][1], wb[ks][2]);
        }
        stage_pass(tt + G, buf ^ 1, nx, pg);
        // the pass (~90 vector instructions: prologue, two hashes, split, masks) is dealt out over the 24 products of
        // its k-steps, its six plane writes behind the last six
        constexpr int NM = 6 * KS_PER_PASS, VPER = 4;
#pragma unroll
        for (int i = 0; i < NM; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);                        // one MFMA
          if (i % 6 < 3) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);         // one fragment read of the next k-step
          __builtin_amdgcn_sched_group_barrier(0x002, VPER, 0);                     // a slice of the staging pass
          if (i >= NM - 6) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);       // its plane writes at the end
        }
        __builtin_amdgcn_sched_barrier(0);
      }
      fetch(tt + 3 * G, nx);                     // (its registers are free only now: two tiles stay in flight all the same)
      float t1 = 0.f, t2 = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int r = mmg_c_row(i);
        const float v = acc[i] + bv;
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ys, yvo, r * N * 4, MMG_NT_ST);
        const float vs = r + 4 * h < rows ? v : 0.f;
        t1 += vs; t2 = fmaf(vs, vs, t2);
      }
      cs1 += (double)t1; cs2 += (double)t2;      // 16 rows in fp32, tiles in fp64
      __syncthreads();                           // buf fully read, buf^1 fully written
    };
    tile_body(t0, 0, nxa);
    tile_body(t0 + G, 1, nxb);
    for (int i = 2; i < n_my; i += 2) {
      tile_body(t0 + (int64_t)i * G, 0, nxa);
      tile_body(t0 + (int64_t)(i + 1) * G, 1, nxb);
    }
    // two partials per column (the lane halves) -> one: partial[row-set][2][N] of each pass, fixed order
    double* red = reinterpret_cast<double*>(planes) + pass * 4 * BN;      // the planes are dead: every wave passed the last barrier
    red[(h * 2 + 0) * BN + col] = cs1;
    red[(h * 2 + 1) * BN + col] = cs2;
    __syncthreads();
    {
      const int e = tid & 255, which = e / BN, c = e % BN;      // threads 0..255: pass 0, 256..511: pass 1 (their own waves' sums)
      stat_partial[((size_t)by * 2 + which) * N + c] = red[which * BN + c] + red[(2 + which) * BN + c];
    }
    __syncthreads();                             // the next row set stages over `red`
  }
}

// one workgroup per CU (104 KB of planes).  The n_sets row sets are those of the single launch; they are dealt to
// MMG_DUAL_WGS workgroups, a workgroup keeping its W pieces over its row sets (256: two row sets each at n_sets = 512)
#ifndef MMG_DUAL_WGS
#define MMG_DUAL_WGS 256
#endif
int launch_fwd_x6_dual(const float* X, const ProDev& pr, const ProDev& prb, const float* W, const float* bias, float* Y0,
                       float* Y1, int64_t M, hipStream_t st, double* part0, double* part1) {
  constexpr int lds = 2 * 2 * 3 * 32 * (128 + 8) * 2;
  const int n_sets = (int)fwd_x6_rows(M, 128, 128, 128);
  const int wgs = n_sets < MMG_DUAL_WGS ? n_sets : MMG_DUAL_WGS;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_fwd_x6_dual, lds>::set()), "linear_fwd_dual(attr)");
  // N is reported as 256: the launch computes 2 M N K products, reads X and W once and writes two [M, 128] outputs;
  // flag 2048 = dual
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, 256, 128, 4 | 2048, k_linear_fwd_x6_dual, dim3((unsigned)wgs), dim3(512), lds, st, X,
             pr, prb, W, bias, Y0, Y1, M, n_sets, part0, part1);
  return 0;
}

// rows +0..3 and +4..7 of this lane's column through the transposing LDS read (see the wgrad section)
__device__ __forceinline__ bf16x8 tr_frag(const __bf16* p, int row_stride) { return mmg_tr_pair(p, p + 4 * row_stride); }

// ---------------------------------------------------------------------------- BatchNorm backward inside the data-gradient GEMM
// dX = dZ . W  with  dZ = the backward of  dropout(relu(BN(y)))  at the upstream gradient G  (mmg_bn_bwd_apply's
// arithmetic), computed WHILE the tile is staged: the kernel reads G and Y once, writes dZ once (the weight gradient of
// the same layer reads it afterwards) and dX -- the separate apply pass read G and Y, wrote dZ, and this GEMM read dZ
// again: 94 MB less per layer at the x100 shape.  Same skeleton as k_linear_fwd_x6 (W pieces in registers, three bf16
// planes double-buffered in LDS, per-tile buffer descriptors, peeled tile pair); both inputs run ONE tile ahead in
// registers (two tiles of two tensors would not fit 256 registers beside the W pieces).  One workgroup covers all N
// output columns, so every dZ tile is produced exactly once.
// MODE 1: the same skeleton with the backward of the row L2 normalisation in the staging phase (mmg_l2norm_bwd's
// arithmetic: dZ = rn * (G - out * <G, out>), the row dot product over the K / 4 lanes that hold a row): Y = the
// normalised rows, mean = rn [M].
// MODE 2: MODE 0 with TWO upstream gradients through the same BatchNorm + ReLU, each with its own dropout mask
// (mmg_bn_bwd_apply2: the two encode_nodes passes of a training step share their first layer).
// MODE 3: MODE 0 with an upstream gradient that is ZERO outside a short list of rows (mmg_bn_bwd_apply with G = NULL +
// mmg_bn_bwd_apply_rows): G holds the listed rows back to back, row_pos[row] = position in that list or -1.
struct BnBwdDev {
  const float* Y; const float* mean; const float* rstd; const double* sums; double inv_count;
  float* dZ; float* dbeta; float* dgamma; float l2_eps; const float* G2; const int32_t* row_pos; int64_t n_sel;
};

// NBN: the statistics of the NEXT BatchNorm backward -- the one that consumes DX -- from the epilogue (NextBnDev),
// partial[row-set][2][N] -> mmg_partial_sum.
// FW: the weight gradient of the same layer rides along (K = N = 128 only): dW[K, N] = dZ^T . pro(X) and db = sum dZ,
// contracted from the dZ planes while they are in LDS -- the separate weight-gradient kernel read dZ back from HBM and
// split it again.  The workgroup doubles to eight waves, one per CU: waves 0..3 are the ones above (dZ staging, dX
// products, NBN epilogue), waves 4..7 stage the matching 32-row tile of X (prologue: BN affine + ReLU + dropout with
// the masks regenerated from the counter RNG, as k_linear_wgrad_x6<..., PRO = true>; split into three bf16 planes beside
// dZ's) and each hold one 64 x 64 dW quadrant, read through the transposing LDS read like k_linear_wgrad_x6.  Tiles are
// dealt round-robin over gridDim.y = plan_wgrad's n_split, so a workgroup reduces exactly the row set of the separate
// kernel's slab, in the same order; one slab per workgroup (dW + column sums of dZ), summed by the grouped reduce.
// Both sums are taken in the separate kernels' own order, so the slabs are theirs bit for bit: dW with the same six
// products per accumulator and 16-row step, the column sums of dZ (reassembled exactly from the three planes: hi + mid +
// lo is the fp32 value) with the partial sums of the kernel linear_wgrad picks for that X -- bias_order 0:
// k_linear_wgrad_ws (four 8-row groups, ((g0 + g1) + g2) + g3), 1: k_linear_wgrad_x6<128, 128, 4, 2, true> (16 row
// residues mod 16 of every 32-row tile, summed in order).
// dZ is stored only where bb.dZ is set (a zero-sized descriptor drops the stores otherwise).
// MSK (FW, MODE 0 / 3): the dX store applies the dropout of wg.xpr -- the mask the consumer of dX would apply first, and
// the one the X stagers hash anyway.  They leave the four keep bits of every group as one byte beside the X planes
// ([buffer][column quad][row], read by the dX waves in the body that multiplies that buffer); 1: DX = kept ? dx * inv_keep
// : 0, 2: DX += the same (the two encoder passes of a step hand ONE tensor to the BatchNorm they share).
struct BnWgDev {
  const float* X; ProDev xpr; float* slab; int64_t slab_stride; int bias_order;
};
static inline BnWgDev bn_wg_none() { return BnWgDev{nullptr, mmg_pro_dev(nullptr), nullptr, 0, 0}; }
// MSK 3, the DUAL form (FW, MODE 0): BOTH passes' launches of one layer -- MSK 1 of MODE 0 (G, bb, pr, wg: "pass B") and then
// MSK 2 of MODE 3 (the fields below: "pass A") on the same W, X and DX -- in one walk over the tiles.  The two bodies of the
// peeled tile pair become the two passes of ONE tile: the body on LDS buffer 0 is pass B of tile t, the body on buffer 1
// pass A of tile t.  Every register set that runs a tile ahead stays single and alternates between the passes; the dX
// waves hold pass B's masked product in registers where MSK 2 holds the tile it re-read, so DX is written once and never
// read; the X stagers fetch, fold and scale a tile once and mask its pieces with each pass's keep bits (split(0) = three
// +0 pieces, as in k_linear_fwd_x6_dual); the dW waves keep one accumulator set and one slab series per pass, each fed
// the fragments and the order of its own launch.  The per-column BatchNorm constants of both passes live in an LDS table
// behind the keep bits.  Every output is that of the two launches bit for bit.
struct BnDualDev {
  const float* G; BnBwdDev bb; ProDev pr; BnWgDev wg;
};
static inline BnDualDev bn_dual_none() { return BnDualDev{nullptr, BnBwdDev{}, mmg_pro_dev(nullptr), bn_wg_none()}; }
template <int V> struct PassMode { static constexpr int value = V; };      // a pass's MODE as a compile-time lambda argument
// RIDER (MODE 1 without FW): a second, compact problem of the same mode on the SAME W rides in the launch -- the L2 backward
// of the first encode_nodes pass of a training step, which reaches the low-degree rows alone (mmg_linear_bnbwd_rider).  A
// workgroup walks its dense tiles exactly as without the rider (same grid, same tile map, same code, same partial
// statistics) and then goes on in the same round-robin over the ceil(n_sel / 32) tiles of (rd.G, rd.bb) -> (rd.bb.dZ, rd.DX):
// the kernel's own fetch and stage on the rider's tensors, the same products in the same order, a plain store.  The rider's
// tiles take no part in the next-BatchNorm epilogue.
struct BnRiderDev { const float* G; BnBwdDev bb; float* DX; int64_t n_sel; };
static inline BnRiderDev bn_rider_none() { return BnRiderDev{nullptr, BnBwdDev{}, nullptr, 0}; }

template <int K, int WN, int MODE = 0, bool NBN = false, bool FW = false, int MSK = 0, bool RIDER = false>
__global__ __launch_bounds__(64 * WN * (FW ? 2 : 1), (WN == 4 && !FW) ? 2 : 1) void k_linear_bnbwd_x6(
    const float* __restrict__ G, BnBwdDev bb, ProDev pr, const float* __restrict__ W, float* __restrict__ DX, int64_t M,
    ProDev pr2, NextBnDev nb, double* __restrict__ stat_partial, BnWgDev wg, BnDualDev du, BnRiderDev rd) {
  static_assert(!FW || (K == 128 && WN == 4), "the fused weight gradient covers K = N = 128");
  static_assert(!RIDER || (MODE == 1 && !FW && MSK == 0), "the rider comes with the plain L2 backward");
  static_assert(MSK == 0 || (FW && !NBN && (MODE == 0 || MODE == 3)), "the masked dX store rides on the X stagers' hashes");
  static_assert(MSK != 3 || MODE == 0, "the dual form: pass B is MODE 0, pass A MODE 3");
  constexpr bool DUAL = MSK == 3;
  if (MODE != 1) pr.resolve();
  if (MODE == 2) pr2.resolve();
  if (FW) wg.xpr.resolve();
  if (DUAL) { du.pr.resolve(); du.wg.xpr.resolve(); }
  constexpr int LDP = K + 8, N = 32 * WN, NK = K / 16, NTHR = 64 * WN, BM = 32;
  constexpr int SX = N + 32;               // X plane row stride (FW): +64 B puts the 4 rows of a transposing read on disjoint banks
  constexpr int KBS = BM + 4;              // keep-bit row stride (MSK): [column quad][tile row] bytes, +4 B spreads the quads over the banks
  extern __shared__ __attribute__((aligned(16))) __bf16 planes[];     // [2 buffers][3 pieces][BM][LDP] (FW: + [2][3][BM][SX] of X; MSK: + [2][N / 4][KBS] keep bits; MSK 3: + the constants table)
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const int col = wn * 32 + l31;
  const bool xrole = FW && tid >= NTHR;    // (wave-uniform) the X stagers / dW multipliers
  bf16x8 wb[NK][3];                       // W stored [K, N] (the forward weight, read in place)
  if (!xrole) {
    const float* wp = W + (size_t)(8 * h) * N + col;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = wp[(size_t)(ks * 16 + j) * N];
        MMG_SPLIT3(v, wb[ks][0][j], wb[ks][1][j], wb[ks][2][j]);
      }
  }
  NextBnCol nbc = {};
  double cs1 = 0.0, cs2 = 0.0;
  if constexpr (NBN) if (!xrole) nbc = next_bn_col(nb, col);
  constexpr int K4 = K / 4;
  const int kc4 = tid % K4, c = kc4 * 4;    // this thread always touches the same 4 columns of G / Y / dZ
  constexpr int ROWS_PER_PASS = NTHR / K4;
  constexpr int NP = BM / ROWS_PER_PASS;
  const int prow = tid / K4;
  const f32x4 one = {1.f, 1.f, 1.f, 1.f}, zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 sc = one, sh = zero, mu = zero, rs = one, a0 = zero, a1 = zero;
  auto col_consts = [&](const ProDev& p_, const BnBwdDev& b_) __attribute__((always_inline)) {
    sc = one; sh = zero; mu = zero; rs = one; a0 = zero; a1 = zero;
    if (MODE != 1 && p_.scale) {
      sc = *reinterpret_cast<const f32x4*>(p_.scale + c); sh = *reinterpret_cast<const f32x4*>(p_.shift + c);
      mu = *reinterpret_cast<const f32x4*>(b_.mean + c); rs = *reinterpret_cast<const f32x4*>(b_.rstd + c);
      if (b_.sums) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          a0[j] = (float)(b_.sums[c + j] * b_.inv_count);
          a1[j] = (float)(b_.sums[K + c + j] * b_.inv_count);
        }
      }
    }
  };
  // DUAL: [pass][sc, sh, mu, rs, a0, a1][K] behind the keep bits, read by `stage` (a second register set does not fit)
  float* const ctab = reinterpret_cast<float*>(reinterpret_cast<unsigned char*>(planes) + 2 * 3 * BM * LDP * 2 +
                                               2 * 3 * BM * SX * 2 + 2 * (N / 4) * KBS);
  if constexpr (DUAL) {
    if (tid < K4) {
#pragma unroll
      for (int ps = 0; ps < 2; ++ps) {
        col_consts(ps ? du.pr : pr, ps ? du.bb : bb);
        const f32x4 six[6] = {sc, sh, mu, rs, a0, a1};
#pragma unroll
        for (int e = 0; e < 6; ++e) *reinterpret_cast<f32x4*>(ctab + (ps * 6 + e) * K + c) = six[e];
      }
      // + the fold of the X prologue [scale, shift][N] for the X stagers, whose second accumulator set leaves no room for it
      *reinterpret_cast<f32x4*>(ctab + 12 * K + c) = wg.xpr.scale ? *reinterpret_cast<const f32x4*>(wg.xpr.scale + c) : one;
      *reinterpret_cast<f32x4*>(ctab + 12 * K + N + c) = wg.xpr.scale ? *reinterpret_cast<const f32x4*>(wg.xpr.shift + c) : zero;
    }
    __syncthreads();
  } else {
    col_consts(pr, bb);
  }
  // (the row-set index through readfirstlane: behind the lane-dependent branch below the compiler otherwise carries
  //  blockIdx.y -- known to be 0 inside it -- in a VECTOR register, every tile index and buffer descriptor derived from it
  //  becomes "divergent", and each of the ~135 buffer accesses of the kernel is wrapped in a waterfall loop)
  const int by_u = __builtin_amdgcn_readfirstlane((int)blockIdx.y);
  auto ride = [&](const BnBwdDev& b_) __attribute__((always_inline)) {      // d beta / d gamma ride along
    if (MODE != 1 && b_.sums && by_u == 0 && tid < K4) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (b_.dbeta) b_.dbeta[c + j] = (float)b_.sums[c + j];
        if (b_.dgamma) b_.dgamma[c + j] = (float)b_.sums[K + c + j];
      }
    }
  };
  ride(bb);
  if constexpr (DUAL) ride(du.bb);
  const bool drop2 = MODE == 2 && pr2.p > 0.f;
  const int64_t n_tiles = (M + BM - 1) / BM;
  const int64_t GY = gridDim.y, t0 = by_u;
  if (t0 >= n_tiles) return;
  const int n_my = (int)((n_tiles - t0 + GY - 1) / GY);
  auto rows_of = [&](int64_t tile) __attribute__((always_inline)) -> int {
    const int64_t r = M - tile * BM;
    return r <= 0 ? 0 : (r < BM ? (int)r : BM);
  };
  f32x4 ng[NP], ny[NP], ng2[MODE == 2 ? NP : 1];      // the NEXT tile of G and Y (and G2)
  const int xvo = (prow * K + kc4 * 4) * 4;
  const BnBwdDev& bbr = DUAL ? du.bb : bb;     // the pass with the row list
  int ridx[MODE == 3 || DUAL ? NP : 1];             // MODE 3: list positions of the rows of the tile the NEXT fetch serves
  auto fetch_idx = [&](int64_t tile) __attribute__((always_inline)) {
    const int rows = rows_of(tile);
    const __amdgpu_buffer_rsrc_t ps = mmg_rsrc(bbr.row_pos + (size_t)(rows ? tile : 0) * BM, rows * 4);
#pragma unroll
    for (int p = 0; p < NP; ++p) ridx[p] = rows ? (int)__builtin_amdgcn_raw_buffer_load_b32(ps, (p * ROWS_PER_PASS + prow) * 4, 0, 0) : -1;
  };
  // (pm: the MODE of the pass the call serves -- MODE itself, or in the dual form 0 for pass B and 3 for pass A)
  auto fetch = [&](int64_t tile, auto pm) __attribute__((always_inline)) {
    constexpr int PM = decltype(pm)::value;
    constexpr bool second = DUAL && PM == 3;
    const BnBwdDev& b_ = second ? du.bb : bb;
    const float* const G_ = second ? du.G : G;
    const int rows = rows_of(tile);
    const size_t off = (size_t)(rows ? tile : 0) * BM * K;
    const __amdgpu_buffer_rsrc_t ysrc = mmg_rsrc(b_.Y + off, rows * K * 4);
    if constexpr (PM == 3) {
      // the listed rows through one descriptor over the whole list: a row that is not listed (or past the end) gets an
      // offset behind the list and reads 0
      const __amdgpu_buffer_rsrc_t gs = mmg_rsrc(G_, (int)(b_.n_sel * K * 4));
#pragma unroll
      for (int p = 0; p < NP; ++p) {
        const unsigned vo = ridx[p] >= 0 && p * ROWS_PER_PASS + prow < rows ? (unsigned)ridx[p] * (unsigned)(K * 4) + (unsigned)(kc4 * 16) : 0xFFFFFF00u;
        ng[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(gs, vo, 0, 0));
        ny[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ysrc, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
      }
      fetch_idx(tile + GY);
      return;
    }
    const __amdgpu_buffer_rsrc_t gs = mmg_rsrc(G_ + off, rows * K * 4);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      ng[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(gs, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
      ny[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ysrc, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
    }
    if constexpr (MODE == 2) {
      const __amdgpu_buffer_rsrc_t g2s = mmg_rsrc(bb.G2 + off, rows * K * 4);
#pragma unroll
      for (int p = 0; p < NP; ++p)
        ng2[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(g2s, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
    }
  };
  auto stage = [&](int64_t tile, int buf, auto pm) __attribute__((always_inline)) {   // BatchNorm backward of the tile in ng / ny, dZ out, split, three plane writes
    constexpr bool second = DUAL && decltype(pm)::value == 3;
    const BnBwdDev& b_ = second ? du.bb : bb;
    const ProDev& pr_ = second ? du.pr : pr;
    const bool relu = MODE != 1 && pr_.relu == MMG_ACT_RELU, drop = MODE != 1 && pr_.p > 0.f, has_bn = MODE != 1 && pr_.scale != nullptr;
    f32x4 sc_ = sc, sh_ = sh, mu_ = mu, rs_ = rs, a0_ = a0, a1_ = a1;
    if constexpr (DUAL) {
      const float* ct = ctab + (second ? 6 * K : 0) + c;
      sc_ = *reinterpret_cast<const f32x4*>(ct); sh_ = *reinterpret_cast<const f32x4*>(ct + K);
      mu_ = *reinterpret_cast<const f32x4*>(ct + 2 * K); rs_ = *reinterpret_cast<const f32x4*>(ct + 3 * K);
      a0_ = *reinterpret_cast<const f32x4*>(ct + 4 * K); a1_ = *reinterpret_cast<const f32x4*>(ct + 5 * K);
    }
    const int64_t row0 = tile * BM;
    const int rows = rows_of(tile);
    const __amdgpu_buffer_rsrc_t zs = mmg_rsrc(b_.dZ + (size_t)(rows && b_.dZ ? tile : 0) * BM * K, b_.dZ ? rows * K * 4 : 0);
    __bf16* pb = planes + (size_t)buf * 3 * BM * LDP;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const int r = p * ROWS_PER_PASS + prow;
      const f32x4 y4 = ny[p];
      f32x4 gm = ng[p], v;
      if constexpr (MODE == 1) {
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) dot = fmaf(gm[j], y4[j], dot);
#pragma unroll
        for (int o = 1; o < K4; o <<= 1) dot += __shfl_xor(dot, o, 64);      // the K / 4 lanes of a row are adjacent
        const int64_t grow = row0 + r;
        const float rr = grow < M ? b_.mean[grow] : 0.f;
        if (!(rr * b_.l2_eps < 1.0f)) dot = 0.f;           // ||z|| <= eps: the denominator was the constant eps
#pragma unroll
        for (int j = 0; j < 4; ++j) gm[j] = rr * (gm[j] - y4[j] * dot);
      }
      f32x4 gm2 = zero;
      if constexpr (MODE == 2) gm2 = ng2[p];
      if (relu) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float act = has_bn ? fmaf(y4[j], sc_[j], sh_[j]) : y4[j];
          if (!(act > 0.f)) { gm[j] = 0.f; gm2[j] = 0.f; }
        }
      }
      if (drop)
        mmg_drop4(gm, pr_.key, (uint64_t)(pr_.row_offset + row0 + r) * (uint64_t)K + (uint64_t)c, pr_.thr, pr_.inv_keep);
      if constexpr (MODE == 2) {
        if (drop2)
          mmg_drop4(gm2, pr2.key, (uint64_t)(pr2.row_offset + row0 + r) * (uint64_t)K + (uint64_t)c, pr2.thr, pr2.inv_keep);
        gm += gm2;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float g = gm[j];
        if (has_bn) {
          const float xh = (y4[j] - mu_[j]) * rs_[j];
          g = sc_[j] * (g - a0_[j] - xh * a1_[j]);
        }
        v[j] = g;
      }
      if constexpr (FW)
        if (r >= rows) v = zero;           // rows past the end: nothing to the weight gradient (their stores are dropped)
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), zs, xvo, p * ROWS_PER_PASS * K * 4, 0);
      bf16x4 q0, q1, q2;
#pragma unroll
      for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
      *reinterpret_cast<bf16x4*>(pb + (0 * BM + r) * LDP + kc4 * 4) = q0;
      *reinterpret_cast<bf16x4*>(pb + (1 * BM + r) * LDP + kc4 * 4) = q1;
      *reinterpret_cast<bf16x4*>(pb + (2 * BM + r) * LDP + kc4 * 4) = q2;
    }
  };
  if (xrole) {
    // ---------------------------------------------------------------- FW: X stagers and dW multipliers (waves 4..7)
    const int t = tid - NTHR, w = wn - WN;
    const int xc4 = t & 31, xr = t >> 5;            // a thread stages the column quad xc4 of rows xr + 8 u
    constexpr int XU = BM * N / 4 / NTHR;           // 16-B loads per thread per tile
    const int xvo2 = (xr * N + xc4 * 4) * 4;
    f32x4 nx[XU];                                   // the NEXT tile of X
    auto xfetch = [&](int64_t tile) __attribute__((always_inline)) {
      const int rows = rows_of(tile);
      const __amdgpu_buffer_rsrc_t xsrc = mmg_rsrc(wg.X + (size_t)(rows ? tile : 0) * BM * N, rows * N * 4);
#pragma unroll
      for (int u = 0; u < XU; ++u)
        nx[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, xvo2, u * (NTHR / 32) * N * 4, MMG_NT_LD));
    };
    f32x4 xsc = one, xsh = zero;
    float xfloor = -__builtin_inff();
    const bool xaff = wg.xpr.scale != nullptr || wg.xpr.relu, xdrop = wg.xpr.p > 0.f;
    if (!DUAL && wg.xpr.scale) {
      xsc = *reinterpret_cast<const f32x4*>(wg.xpr.scale + xc4 * 4);
      xsh = *reinterpret_cast<const f32x4*>(wg.xpr.shift + xc4 * 4);
    }
    if (wg.xpr.relu) xfloor = 0.f;
    __bf16* xplanes = planes + 2 * 3 * BM * LDP;
    unsigned char* keepb = reinterpret_cast<unsigned char*>(xplanes + 2 * 3 * BM * SX);
    auto xstage = [&](int64_t tile, int buf) __attribute__((always_inline)) {
      __bf16* xb = xplanes + (size_t)buf * 3 * BM * SX;
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int r = xr + u * (NTHR / 32);
        f32x4 v = nx[u];
        if (xaff) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], xsc[j], xsh[j]), xfloor);
        }
        if constexpr (MSK != 0) {
          // the keep bits of this group of four go to the dX waves, whose masked store applies the SAME mask
          uint32_t kb = 0xFu;
          if (xdrop)
            kb = mmg_drop4_bits(v, wg.xpr.key, (uint64_t)(wg.xpr.row_offset + tile * BM + r) * (uint64_t)N + (uint64_t)(xc4 * 4),
                                wg.xpr.thr, wg.xpr.inv_keep);
          keepb[(buf * (N / 4) + xc4) * KBS + r] = (unsigned char)kb;
        } else if (xdrop)
          mmg_drop4(v, wg.xpr.key, (uint64_t)(wg.xpr.row_offset + tile * BM + r) * (uint64_t)N + (uint64_t)(xc4 * 4),
                    wg.xpr.thr, wg.xpr.inv_keep);
        // rows past the end need no zeroing: their dZ rows are zero
        bf16x4 q0, q1, q2;
#pragma unroll
        for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
        *reinterpret_cast<bf16x4*>(xb + (0 * BM + r) * SX + xc4 * 4) = q0;
        *reinterpret_cast<bf16x4*>(xb + (1 * BM + r) * SX + xc4 * 4) = q1;
        *reinterpret_cast<bf16x4*>(xb + (2 * BM + r) * SX + xc4 * 4) = q2;
      }
    };
    // DUAL: the tile in nx goes through the affine, the ReLU and the scaling ONCE (xscale, in place: the product rounded
    // before the split -- an empty asm keeps it a multiply, see k_linear_fwd_x6_dual) and stays in nx while each pass
    // masks its pieces with its own keep bits (xput: the hash of mmg_drop4_bits under the pass's key; a dropped element
    // is three +0 pieces, split(0)) into the buffer its body multiplies, the keep bytes beside them as xstage leaves them
    auto xscale = [&]() __attribute__((always_inline)) {
      const f32x4 xsc = *reinterpret_cast<const f32x4*>(ctab + 12 * K + xc4 * 4);
      const f32x4 xsh = *reinterpret_cast<const f32x4*>(ctab + 12 * K + N + xc4 * 4);
#pragma unroll
      for (int u = 0; u < XU; ++u)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float s = nx[u][j];
          if (xaff) s = fmaxf(fmaf(s, xsc[j], xsh[j]), xfloor);
          if (xdrop) {
            s *= wg.xpr.inv_keep;
            asm("" : "+v"(s));
          }
          nx[u][j] = s;
        }
    };
    auto xput = [&](int64_t tile, int buf, uint32_t key) __attribute__((always_inline)) {
      __bf16* xb = xplanes + (size_t)buf * 3 * BM * SX;
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int r = xr + u * (NTHR / 32);
        u32x2 km = {0xFFFFFFFFu, 0xFFFFFFFFu};
        uint32_t kb = 0xFu;
        if (xdrop) {
          uint32_t w0, w1;
          mmg_rng_group(key, ((uint64_t)(wg.xpr.row_offset + tile * BM + r) * (uint64_t)N + (uint64_t)(xc4 * 4)) >> 2, &w0, &w1);
          const bool k0 = MMG_KEPT(w0, w1, 0, wg.xpr.thr), k1 = MMG_KEPT(w0, w1, 1, wg.xpr.thr),
                     k2 = MMG_KEPT(w0, w1, 2, wg.xpr.thr), k3 = MMG_KEPT(w0, w1, 3, wg.xpr.thr);
          km[0] = (k0 ? 0x0000FFFFu : 0u) | (k1 ? 0xFFFF0000u : 0u);
          km[1] = (k2 ? 0x0000FFFFu : 0u) | (k3 ? 0xFFFF0000u : 0u);
          kb = (k0 ? 1u : 0u) | (k1 ? 2u : 0u) | (k2 ? 4u : 0u) | (k3 ? 8u : 0u);
        }
        keepb[(buf * (N / 4) + xc4) * KBS + r] = (unsigned char)kb;
        bf16x4 q0, q1, q2;
#pragma unroll
        for (int j = 0; j < 4; ++j) MMG_SPLIT3(nx[u][j], q0[j], q1[j], q2[j]);
        *reinterpret_cast<u32x2*>(xb + (0 * BM + r) * SX + xc4 * 4) = __builtin_bit_cast(u32x2, q0) & km;
        *reinterpret_cast<u32x2*>(xb + (1 * BM + r) * SX + xc4 * 4) = __builtin_bit_cast(u32x2, q1) & km;
        *reinterpret_cast<u32x2*>(xb + (2 * BM + r) * SX + xc4 * 4) = __builtin_bit_cast(u32x2, q2) & km;
      }
    };
    // wave w owns the quadrant (w >> 1, w & 1) of dW [K, N]; transposing-read lane roles as in k_linear_wgrad_x6
    const int qn = w >> 1, qk = w & 1;
    const int g4 = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
    const int tr_row = 8 * (g4 >> 1) + q, tr_col = 16 * (g4 & 1) + 4 * p4;
    constexpr int NPS = DUAL ? 2 : 1;               // passes: an accumulator set, bias partials and a slab series each
    f32x16 wacc[NPS][2][2];
    // the column sums of dZ (the bias gradient) as the partial sums the separate kernel keeps (see BnWgDev), each row
    // reassembled from the three planes.  bias_order 0: thread t owns group t >> 6 and the columns 2 (t & 63) + 0..1;
    // 1: thread t owns residue t >> 4 and the columns 8 (t & 15) + 0..7 (one ds_read_b128 per plane and row)
    const int bg = wg.bias_order == 0 ? t >> 6 : t >> 4;
    const int bc0 = wg.bias_order == 0 ? 2 * (t & 63) : 8 * (t & 15);
    float bacc[NPS][8];
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bacc[ps][e] = 0.f;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int i = 0; i < 16; ++i) wacc[ps][x][y][i] = 0.f;
    }
    xfetch(t0);
    if constexpr (DUAL) {
      xscale();
      xput(t0, 0, wg.xpr.key);
    } else {
      xstage(t0, 0);
      xfetch(t0 + GY);
    }
    __syncthreads();
    auto wbody = [&](int64_t tt, int buf, auto pm) __attribute__((always_inline)) {
      constexpr int ps = DUAL && decltype(pm)::value == 3 ? 1 : 0;
      const bool has_bias = (ps ? du.wg.slab_stride : wg.slab_stride) > (int64_t)K * N;
      // the products first and the staging behind them -- the dZ wave that shares the SIMD stages first and multiplies
      // second, so one wave's vector work runs under the other's matrix work instead of both queueing for the same pipe
      // (either order is free: a body reads buf and writes buf ^ 1)
      auto xwork = [&]() __attribute__((always_inline)) {
        if constexpr (!DUAL) {
          xstage(tt + GY, buf ^ 1);
          xfetch(tt + 2 * GY);
        } else if constexpr (ps == 0) {          // pass B of tile tt: its planes of pass A, then nx is free for the next tile
          xput(tt, 1, du.wg.xpr.key);
          xfetch(tt + GY);
        } else {                                 // pass A of tile tt: the next tile, and its planes of pass B
          xscale();
          xput(tt + GY, 0, wg.xpr.key);
        }
        __builtin_amdgcn_sched_barrier(0);
      };
      const __bf16* zb = planes + (size_t)buf * 3 * BM * LDP + tr_row * LDP + qn * 64 + tr_col;
      const __bf16* xb = xplanes + (size_t)buf * 3 * BM * SX + tr_row * SX + qk * 64 + tr_col;
#pragma unroll
      for (int ks = 0; ks < BM / 16; ++ks) {
        bf16x8 fa[2][3], fb[2][3];
        // small terms first, the order of k_linear_wgrad_ws / k_linear_wgrad_x6 for every accumulator
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
        if constexpr (DUAL) {
          // the dZ fragments one x half at a time (12 registers less in flight beside the second accumulator set); every
          // accumulator still takes its six products in the order above
#pragma unroll
          for (int y = 0; y < 2; ++y)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) fb[y][pc] = tr_frag(xb + pc * BM * SX + ks * 16 * SX + y * 32, SX);
#pragma unroll
          for (int x = 0; x < 2; ++x) {
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) fa[0][pc] = tr_frag(zb + pc * BM * LDP + ks * 16 * LDP + x * 32, LDP);
#pragma unroll
            for (int tm = 0; tm < 6; ++tm)
#pragma unroll
              for (int y = 0; y < 2; ++y)
                wacc[ps][x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[0][PA[tm]], fb[y][PB[tm]], wacc[ps][x][y], 0, 0, 0);
          }
        } else {
#pragma unroll
          for (int x = 0; x < 2; ++x)
#pragma unroll
            for (int pc = 0; pc < 3; ++pc) {
              fa[x][pc] = tr_frag(zb + pc * BM * LDP + ks * 16 * LDP + x * 32, LDP);
              fb[x][pc] = tr_frag(xb + pc * BM * SX + ks * 16 * SX + x * 32, SX);
            }
#pragma unroll
          for (int tm = 0; tm < 6; ++tm)
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
              for (int y = 0; y < 2; ++y)
                wacc[ps][x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[x][PA[tm]], fb[y][PB[tm]], wacc[ps][x][y], 0, 0, 0);
        }
      }
      if (has_bias) {
        const __bf16* zp = planes + (size_t)buf * 3 * BM * LDP + bc0;
        if (wg.bias_order == 0) {              // k_linear_wgrad_ws: group g, rows 8 g .. 8 g + 7 in order
          typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int r = 8 * bg + j;
            const bf16x2 a = *reinterpret_cast<const bf16x2*>(zp + r * LDP);
            const bf16x2 b = *reinterpret_cast<const bf16x2*>(zp + (BM + r) * LDP);
            const bf16x2 c = *reinterpret_cast<const bf16x2*>(zp + (2 * BM + r) * LDP);
#pragma unroll
            for (int e = 0; e < 2; ++e) bacc[ps][e] += ((float)a[e] + (float)b[e]) + (float)c[e];
          }
        } else {                               // k_linear_wgrad_x6: residue q, rows q then q + 16
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int r = bg + 16 * u;
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(zp + r * LDP);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(zp + (BM + r) * LDP);
            const bf16x8 c = *reinterpret_cast<const bf16x8*>(zp + (2 * BM + r) * LDP);
#pragma unroll
            for (int e = 0; e < 8; ++e) bacc[ps][e] += ((float)a[e] + (float)b[e]) + (float)c[e];
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      xwork();
      __syncthreads();                         // buf fully read, buf^1 fully written
    };
    if constexpr (DUAL) {                      // every tile of the row set: pass B on buffer 0, then pass A on buffer 1
      for (int i = 0; i < n_my; ++i) {
        wbody(t0 + (int64_t)i * GY, 0, PassMode<0>{});
        wbody(t0 + (int64_t)i * GY, 1, PassMode<3>{});
      }
    } else {
      wbody(t0, 0, PassMode<MODE>{});
      wbody(t0 + GY, 1, PassMode<MODE>{});
      for (int i = 2; i < n_my; i += 2) {
        wbody(t0 + (int64_t)i * GY, 0, PassMode<MODE>{});
        wbody(t0 + (int64_t)(i + 1) * GY, 1, PassMode<MODE>{});
      }
    }
    if constexpr (NBN) __syncthreads();        // pairs with the barrier of the statistics epilogue below
#pragma unroll
    for (int ps = 0; ps < NPS; ++ps) {
      const BnWgDev& w_ = ps ? du.wg : wg;
      if (w_.slab_stride > (int64_t)K * N) {   // the partial sums -> the X planes (dead: every wave passed the last barrier)
        float* red = reinterpret_cast<float*>(xplanes) + ps * 16 * K;          // [pass][group / residue][K]
        const int np = wg.bias_order == 0 ? 2 : 8;
#pragma unroll
        for (int e = 0; e < 8; ++e)
          if (e < np) red[bg * K + bc0 + e] = bacc[ps][e];
      }
      // slab[row-set][K * N (+ K column sums of dZ)]
      float* dst = w_.slab + (size_t)by_u * w_.slab_stride;
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const int n = qn * 64 + x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            const int k = qk * 64 + y * 32 + l31;
            dst[(size_t)n * N + k] = wacc[ps][x][y][i];
          }
    }
  } else {
    if constexpr (MODE == 3 || DUAL) fetch_idx(t0);
    fetch(t0, PassMode<MODE>{});
    stage(t0, 0, PassMode<MODE>{});
    if constexpr (DUAL) fetch(t0, PassMode<3>{});
    else fetch(t0 + GY, PassMode<MODE>{});
    __syncthreads();
    const int yvo = ((4 * h) * N + wn * 32 + l31) * 4;     // C/D map: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
    float held[DUAL ? 16 : 1];                   // DUAL: pass B's masked product of the tile, until pass A adds its own
    auto tile_body = [&](int64_t tt, int buf, auto pm) __attribute__((always_inline)) {
      constexpr bool second = DUAL && decltype(pm)::value == 3;
      const int rows = rows_of(tt);
      const __amdgpu_buffer_rsrc_t xs = mmg_rsrc(DX + (size_t)(rows ? tt : 0) * BM * N, rows * N * 4);
      f32x16 acc;
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[i] = 0.f;
      if constexpr (!DUAL) {
        stage(tt + GY, buf ^ 1, pm);             // the other buffer: its readers passed the barrier of the last tile
        fetch(tt + 2 * GY, pm);
      } else if constexpr (!second) {            // pass B of tile tt: pass A's dZ of the same tile, pass B's inputs of the next
        stage(tt, 1, PassMode<3>{});
        fetch(tt + GY, PassMode<0>{});
      } else {                                   // pass A of tile tt: pass B's dZ of the next tile, pass A's inputs of the next
        stage(tt + GY, 0, PassMode<0>{});
        fetch(tt + GY, PassMode<3>{});
      }
      float nby[NBN ? 16 : 1];
      if constexpr (NBN) next_bn_load(nb, tt, rows, N, 0, yvo, nby);   // in flight under the products
      float old[MSK == 2 ? 16 : 1];              // MSK 2: the tile the masked store adds to, in flight under the products too
      if constexpr (MSK == 2) {
#pragma unroll
        for (int i = 0; i < 16; ++i)
          old[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(xs, yvo, mmg_c_row(i) * N * 4, MMG_NT_LD));
      }
      __builtin_amdgcn_sched_barrier(0);         // keep the fetch ahead of the matrix loop
      const __bf16* ap = planes + (size_t)buf * 3 * BM * LDP + l31 * LDP + 8 * h;
#pragma unroll
      for (int ks = 0; ks < NK; ++ks) {
        const bf16x8 a1f = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
        const bf16x8 a2f = *reinterpret_cast<const bf16x8*>(ap + BM * LDP + ks * 16);
        const bf16x8 a3f = *reinterpret_cast<const bf16x8*>(ap + 2 * BM * LDP + ks * 16);
        MMG_X6_ALO(acc, a1f, a2f, a3f, wb[ks][0], wb[ks][1], wb[ks][2]);
      }
      float vv[16];
      if constexpr (MSK != 0) {
        // DX (+)= dropout(dX) under the mask of wg.xpr (mmg_drop4's expression; the product is rounded before the add: an
        // empty asm keeps it a multiply, as in k_linear_fwd_x6_dual).  The X stagers left the keep bits of this buffer's
        // tile beside the X planes before the barrier that released it: rows 8 g + 4 h + 0..3 of this lane's column quad
        const unsigned char* kq = reinterpret_cast<const unsigned char*>(planes + 2 * 3 * BM * LDP + 2 * 3 * BM * SX) +
                                  (buf * (N / 4) + (col >> 2)) * KBS + 4 * h;
        const int sub = col & 3;
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const uint32_t kw = *reinterpret_cast<const uint32_t*>(kq + 8 * g4) >> sub;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int i = 4 * g4 + j;
            float s = acc[i] * wg.xpr.inv_keep;
            asm("" : "+v"(s));
            s = (kw >> (8 * j)) & 1u ? s : 0.f;
            if constexpr (DUAL && !second) held[i] = s;
            else vv[i] = MSK == 2 ? old[i] + s : (DUAL ? held[i] + s : s);
          }
        }
        if constexpr (!DUAL || second) {
#pragma unroll
          for (int i = 0; i < 16; ++i)
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vv[i]), xs, yvo, mmg_c_row(i) * N * 4, MMG_NT_ST);
        }
      } else {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          vv[i] = acc[i];                        // (a bit_cast straight from the vector element stored element 0 sixteen times)
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vv[i]), xs, yvo, mmg_c_row(i) * N * 4,
                                                MMG_NT_ST);
        }
      }
      if constexpr (NBN) next_bn_tile(nb, nbc, vv, nby, rows, tt * BM, N, col, lane, cs1, cs2);
      __syncthreads();                         // buf fully read, buf^1 fully written
    };
    if constexpr (DUAL) {
      for (int i = 0; i < n_my; ++i) {
        tile_body(t0 + (int64_t)i * GY, 0, PassMode<0>{});
        tile_body(t0 + (int64_t)i * GY, 1, PassMode<3>{});
      }
    } else {
      tile_body(t0, 0, PassMode<MODE>{});
      tile_body(t0 + GY, 1, PassMode<MODE>{});
      for (int i = 2; i < n_my; i += 2) {
        tile_body(t0 + (int64_t)i * GY, 0, PassMode<MODE>{});
        tile_body(t0 + (int64_t)(i + 1) * GY, 1, PassMode<MODE>{});
      }
    }
    if constexpr (RIDER) {
      // the rider's tiles, dealt on in the same round-robin: tile j is tile n_tiles + j of the walk.  Every wave is past the
      // barrier of its last dense tile, so the planes are free; from here on G, bb, DX and M are the rider's (fetch, stage
      // and rows_of read them by reference), one tile at a time through LDS buffer 0.
      const int64_t j0 = t0 + (int64_t)n_my * GY - n_tiles, nt_r = (rd.n_sel + BM - 1) / BM;
      G = rd.G; bb = rd.bb; DX = rd.DX; M = rd.n_sel;
      for (int64_t j = j0; j < nt_r; j += GY) {
        fetch(j, PassMode<MODE>{});
        stage(j, 0, PassMode<MODE>{});
        __syncthreads();
        const int rows = rows_of(j);
        const __amdgpu_buffer_rsrc_t xs = mmg_rsrc(DX + (size_t)j * BM * N, rows * N * 4);
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        const __bf16* ap = planes + l31 * LDP + 8 * h;
#pragma unroll
        for (int ks = 0; ks < NK; ++ks) {
          const bf16x8 a1f = *reinterpret_cast<const bf16x8*>(ap + ks * 16);
          const bf16x8 a2f = *reinterpret_cast<const bf16x8*>(ap + BM * LDP + ks * 16);
          const bf16x8 a3f = *reinterpret_cast<const bf16x8*>(ap + 2 * BM * LDP + ks * 16);
          MMG_X6_ALO(acc, a1f, a2f, a3f, wb[ks][0], wb[ks][1], wb[ks][2]);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const float v = acc[i];
          __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), xs, yvo, mmg_c_row(i) * N * 4, MMG_NT_ST);
        }
        __syncthreads();                         // buffer 0 fully read: the next tile may be staged
      }
    }
    if constexpr (NBN) {
      // two partials per column (the lane halves) -> one: partial[row-set][2][N], fixed order
      double* red = reinterpret_cast<double*>(planes);          // the planes are dead: every wave passed the last barrier
      red[(h * 2 + 0) * N + col] = cs1;
      red[(h * 2 + 1) * N + col] = cs2;
      __syncthreads();
      for (int e = tid; e < 2 * N; e += NTHR) {
        const int which = e / N, cc = e % N;
        stat_partial[((size_t)by_u * 2 + which) * N + cc] = red[which * N + cc] + red[(2 + which) * N + cc];
      }
    }
  }
  if constexpr (FW) {
    __syncthreads();                           // the partial column sums of dZ are in LDS
    const int cc = tid - NTHR;
#pragma unroll
    for (int ps = 0; ps < (DUAL ? 2 : 1); ++ps) {
      const BnWgDev& w_ = ps ? du.wg : wg;
      if (xrole && cc < K && w_.slab_stride > (int64_t)K * N) {
        const float* red = reinterpret_cast<const float*>(planes + 2 * 3 * BM * LDP) + ps * 16 * K;
        float v;
        if (wg.bias_order == 0) {
          v = ((red[cc] + red[K + cc]) + red[2 * K + cc]) + red[3 * K + cc];
        } else {
          v = 0.f;
#pragma unroll
          for (int qq = 0; qq < 16; ++qq) v += red[qq * K + cc];
        }
        w_.slab[(size_t)by_u * w_.slab_stride + (size_t)K * N + cc] = v;
      }
    }
  }
}

inline int64_t bnbwd_x6_rows(int64_t M, int K) {       // grid.y of k_linear_bnbwd_x6 (= rows of its partial statistics)
  // one workgroup spans all N columns; two workgroups per CU whatever the width (register-bound), one at K = 256
  const int64_t n_tiles_ = (M + 31) / 32, want_ = K <= 128 ? 512 : 256;
  return want_ < n_tiles_ ? want_ : (n_tiles_ > 0 ? n_tiles_ : 1);
}

template <int K, int WN, int MODE = 0, bool NBN = false>
int launch_bnbwd_x6(const float* G, const BnBwdDev& bb, const ProDev& pr, const float* W, float* DX, int64_t M, hipStream_t st,
                    const ProDev& pr2 = mmg_pro_dev(nullptr), const NextBnDev& nb = next_bn_none(),
                    double* stat_partial = nullptr) {
  constexpr int N = 32 * WN;
  const int64_t gy = bnbwd_x6_rows(M, K);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_bnbwd_x6<K, WN, MODE, NBN>, lds>::set()), "linear_bnbwd(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, (MODE == 1 ? 64 : (MODE == 2 ? 16 | 128 : (MODE == 3 ? 16 | 256 : 16))) | (NBN ? 512 : 0),
             (k_linear_bnbwd_x6<K, WN, MODE, NBN>), dim3(1u, (unsigned)gy),
             dim3(64 * WN), lds, st, G, bb, pr, W, DX, M, pr2, nb, stat_partial, bn_wg_none(), bn_dual_none(), bn_rider_none());
  return 0;
}

// the L2 backward of a [M, 128] x [128, 128] layer with a rider (mmg_linear_bnbwd_rider): the dense launch's grid, LDS and
// probe row + the flag 32768
template <bool NBN>
int launch_bnbwd_x6_rider(const float* G, const BnBwdDev& bb, const float* W, float* DX, int64_t M, hipStream_t st,
                          const NextBnDev& nb, double* stat_partial, const BnRiderDev& rd) {
  constexpr int K = 128, N = 128;
  const int64_t gy = bnbwd_x6_rows(M, K);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_bnbwd_x6<128, 4, 1, NBN, false, 0, true>, lds>::set()), "linear_bnbwd_rider(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, 64 | (NBN ? 512 : 0) | 32768, (k_linear_bnbwd_x6<128, 4, 1, NBN, false, 0, true>),
             dim3(1u, (unsigned)gy), dim3(256), lds, st, G, bb, mmg_pro_dev(nullptr), W, DX, M, mmg_pro_dev(nullptr), nb,
             stat_partial, bn_wg_none(), bn_dual_none(), rd);
  return 0;
}

// Small M (the vocab-side tables: 50..200 rows): one 256-thread workgroup per 32x32 output tile, the k axis split
// over its four waves (and over the lane halves inside a wave), every operand load issued up front straight from
// L2 into registers, the four partial tiles summed through LDS.  These launches are pure latency (a dependent chain
// load -> MFMAs -> store): a quarter of the chain per wave, one load round trip.
template <int K>
__global__ __launch_bounds__(256) void k_linear_small(const float* __restrict__ X, ProDev pr,
                                                      const float* __restrict__ W, const float* __restrict__ bias,
                                                      float* __restrict__ Y, int64_t M, int N, int flags) {
  pr.resolve();
  __shared__ float part[4][16][64];
  const int accumulate = flags & MMG_LIN_ACCUMULATE;
  const bool wkn = (flags & MMG_LIN_W_KN) != 0;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, h = lane >> 5, l31 = lane & 31;
  constexpr int KW = K / 8;                       // k values per (wave, lane half)
  const int kb = wid * (K / 4) + h * KW;
  const int n0 = blockIdx.x * 32;
  const int64_t row0 = (int64_t)blockIdx.y * 32;
  const int64_t ar = row0 + l31;
  const float* xp = X + (size_t)(ar < M ? ar : 0) * K + kb;
  const float* wp = wkn ? W + (size_t)kb * N + n0 + l31 : W + (size_t)(n0 + l31) * K + kb;
  f32x4 a[KW / 4], w[KW / 4];
#pragma unroll
  for (int q = 0; q < KW / 4; ++q) {
    a[q] = *reinterpret_cast<const f32x4*>(xp + q * 4);
    if (wkn) {
#pragma unroll
      for (int j = 0; j < 4; ++j) w[q][j] = wp[(size_t)(q * 4 + j) * N];
    } else {
      w[q] = *reinterpret_cast<const f32x4*>(wp + q * 4);
    }
  }
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
  for (int q = 0; q < KW / 4; ++q) {
    if (pr.scale || pr.relu || pr.p > 0.f) {
      const int k0 = kb + q * 4;
      f32x4 s4 = {1.f, 1.f, 1.f, 1.f}, sh4 = {0.f, 0.f, 0.f, 0.f};
      if (pr.scale) { s4 = *reinterpret_cast<const f32x4*>(pr.scale + k0); sh4 = *reinterpret_cast<const f32x4*>(pr.shift + k0); }
      mmg_pro_apply4(pr, a[q], s4, sh4, ar, k0, K);
    }
    if (ar >= M) a[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q][j], w[q][j], acc, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) part[wid][i][lane] = acc[i];
  __syncthreads();
  // wave w finishes accumulator registers 4w .. 4w+3 (rows (i & 3) + 8 w + 4 h)
  const int col = n0 + l31;
  const float bv = bias ? bias[col] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = 4 * wid + e;
    const float v0 = part[0][i][lane] + part[1][i][lane] + part[2][i][lane] + part[3][i][lane];
    const int64_t gr = row0 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (gr < M) {
      float* dst = Y + (size_t)gr * N + col;
      float v = v0 + bv;
      if (accumulate) v += *dst;
      *dst = v;
    }
  }
}

// ---------------------------------------------------------------------------------- wgrad
constexpr int WG_ROWS = 32;   // rows reduced per LDS stage

// wgrad on the bf16 matrix cores: dW[n, k] = sum_m dY[m, n] * pro(X)[m, k] with the same exact 6-term split.  Both
// operands are contracted over their ROW index, so the fragments are column slices of the row-major tiles: the
// three bf16 planes of dY and X are staged row-major (coalesced 16-B loads, one split per element) and read back
// through the gfx950 transposing LDS read (ds_read_b64_tr_b16: a 16-lane group fetches 4 rows x 16 columns and
// each lane receives 4 consecutive rows of ITS column).  Row stride = tile bytes + 64: the 4 rows of a group then
// sit on 4 disjoint 16-bank spans (conflict-free).  32-row stages, double-buffered, one barrier per stage.

template <int TN, int TK, int WNN, int WNK, bool PRO>      // WNN x WNK waves over the [TN, TK] output tile
__global__ __launch_bounds__(64 * WNN * WNK) void k_linear_wgrad_x6(const float* __restrict__ dY, const float* __restrict__ X,
                                                         ProDev pr, float* __restrict__ slab, int64_t M, int N, int K,
                                                         int64_t rows_per_split, int direct_accumulate,
                                                         int64_t slab_stride, float* __restrict__ dbias) {
  if (PRO) pr.resolve();
  constexpr int NTHR = 64 * WNN * WNK;
  constexpr int MT = TN / (32 * WNN), KT = TK / (32 * WNK);      // 32x32 tiles per wave along n and k
  static_assert(MT >= 1 && KT >= 1, "tile too small for the wave grid");
  constexpr int SY = TN + 32, SX = TK + 32;      // plane row strides in bf16 (+64 B)
  constexpr int PY = 3 * WG_ROWS * SY, PX = 3 * WG_ROWS * SX;
  extern __shared__ __attribute__((aligned(16))) __bf16 wplanes[];   // [2][ dY: 3 x 32 x SY | X: 3 x 32 x SX ]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wn = wid / WNK, wk = wid % WNK;
  const int tiles_k = K / TK;
  int bx, by;
  xcd_tile_map(&bx, &by);                 // (output tile, stage set): the tiles that stream the same rows share an XCD's L2
  const int tn0 = (bx / tiles_k) * TN, tk0 = (bx % tiles_k) * TK;
  // 32-row stages are dealt round-robin: workgroup y takes stages y, y + G, y + 2G, ...  At any moment the grid reads
  // one contiguous window of dY and X (G x 16 KB each), which spreads over every HBM channel; a contiguous chunk per
  // workgroup makes G streams advance in lockstep a fixed (power-of-two-ish) stride apart and pile onto few channels.
  (void)rows_per_split;
  const int64_t total_st = (M + WG_ROWS - 1) / WG_ROWS;
  const int64_t G = gridDim.y;
  const int n_st = (int64_t)by < total_st ? (int)((total_st - by + G - 1) / G) : 0;

  f32x16 acc[MT][KT];
#pragma unroll
  for (int a = 0; a < MT; ++a)
#pragma unroll
    for (int b = 0; b < KT; ++b)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;

  // Memory pipeline: a ring of RING 32-row stages in registers on top of the double-buffered LDS planes (the stage
  // time is far below the HBM latency: with one stage in flight the kernel ran at the pace of one round trip per 32
  // rows).  All loads go through per-stage buffer descriptors (rows past the end read 0, stages past the end have a
  // zero-sized descriptor), so the loop has no branch around a load and the vmcnt waits are exact.
  constexpr int RING = 4;
  constexpr int NY = WG_ROWS * (TN / 4) / NTHR, NX = WG_ROWS * (TK / 4) / NTHR;   // 16-B loads per thread per stage
  static_assert(NY >= 1 && NX >= 1, "stage smaller than the workgroup");
  static_assert(NTHR % (TN / 4) == 0 && NTHR % (TK / 4) == 0, "a thread keeps its column quad across passes");
  constexpr int RY = NTHR / (TN / 4), RX = NTHR / (TK / 4);      // rows covered per pass
  const int yr = tid / (TN / 4), yc4 = tid % (TN / 4), xr = tid / (TK / 4), xc4 = tid % (TK / 4);
  const int yvo = (yr * N + yc4 * 4) * 4, xvo = (xr * K + xc4 * 4) * 4;
  f32x4 ny[RING][NY], nxr[RING][NX];
  auto fetch = [&](int st, f32x4* fy, f32x4* fx) {
    const int64_t r0 = ((int64_t)by + (int64_t)st * G) * WG_ROWS;
    const int64_t left = M - r0;
    const int rows = st < n_st ? (left < WG_ROWS ? (int)left : WG_ROWS) : 0;
    const int64_t rb = rows ? r0 : 0;
    const __amdgpu_buffer_rsrc_t ys = mmg_rsrc(dY + (size_t)rb * N + tn0, rows ? (rows * N - tn0) * 4 : 0);
    const __amdgpu_buffer_rsrc_t xs = mmg_rsrc(X + (size_t)rb * K + tk0, rows ? (rows * K - tk0) * 4 : 0);
#pragma unroll
    for (int u = 0; u < NY; ++u)
      fy[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(ys, yvo, u * RY * N * 4, MMG_NT_WG));
#pragma unroll
    for (int u = 0; u < NX; ++u)
      fx[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xs, xvo, u * RX * K * 4, MMG_NT_WG));
  };
  auto split_store = [&](f32x4 v, __bf16* plane0, int plane_elems, int off) {
    bf16x4 q0, q1, q2;
#pragma unroll
    for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
    *reinterpret_cast<bf16x4*>(plane0 + off) = q0;
    *reinterpret_cast<bf16x4*>(plane0 + plane_elems + off) = q1;
    *reinterpret_cast<bf16x4*>(plane0 + 2 * plane_elems + off) = q2;
  };
  // prologue constants of this thread's column quad (identity when a part is absent: x*1+0, max(x,-inf))
  f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
  float floor_v = -__builtin_inff();
  bool drop = false;
  if (PRO) {
    if (pr.scale) {
      sc = *reinterpret_cast<const f32x4*>(pr.scale + tk0 + xc4 * 4);
      sh = *reinterpret_cast<const f32x4*>(pr.shift + tk0 + xc4 * 4);
    }
    if (pr.relu) floor_v = 0.f;
    drop = pr.p > 0.f;
  }
  f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
  auto stage = [&](int st, int buf, const f32x4* fy, const f32x4* fx) {
    __bf16* yb = wplanes + (size_t)buf * (PY + PX);
    __bf16* xb = yb + PY;
    const int64_t r0 = ((int64_t)by + (int64_t)st * G) * WG_ROWS;
#pragma unroll
    for (int u = 0; u < NY; ++u) {
      const f32x4 v = fy[u];                     // rows past the end arrive as zeros
      bsum += v;                                 // column sums of dY (the bias gradient) ride along: the quad is fixed per thread
      split_store(v, yb, WG_ROWS * SY, (yr + u * RY) * SY + yc4 * 4);
    }
#pragma unroll
    for (int u = 0; u < NX; ++u) {
      f32x4 v = fx[u];
      if (PRO) {
        const int64_t gr = r0 + xr + u * RX;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], sc[j], sh[j]), floor_v);
        if (drop)
          mmg_drop4(v, pr.key, (uint64_t)(pr.row_offset + gr) * (uint64_t)K + (uint64_t)(tk0 + xc4 * 4), pr.thr, pr.inv_keep);
        // no zeroing of the rows past the end: their dY rows are zero, so they contribute 0 to every product
      }
      split_store(v, xb, WG_ROWS * SX, (xr + u * RX) * SX + xc4 * 4);
    }
  };
  // transposing-read lane roles: group g = lane >> 4 fetches rows 8 (g >> 1) + q, columns 16 (g & 1) + 4 p
  const int g = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
  const int tr_row = 8 * (g >> 1) + q, tr_col = 16 * (g & 1) + 4 * p4;
  const int h = lane >> 5, l31 = lane & 31;

  // stage s lives in ring slot s % RING and LDS buffer s & 1
#pragma unroll
  for (int j = 0; j < RING; ++j) fetch(j, ny[j], nxr[j]);
  stage(0, 0, ny[0], nxr[0]);
  fetch(RING, ny[0], nxr[0]);
  __syncthreads();
  auto body = [&](int st, int j) {               // j = st % RING (compile-time after unrolling), RING is even: buf = j & 1
    constexpr int dummy = 0; (void)dummy;
    const int jn = (j + 1) % RING;
    stage(st + 1, (j + 1) & 1, ny[jn], nxr[jn]);
    fetch(st + 1 + RING, ny[jn], nxr[jn]);
    __builtin_amdgcn_sched_barrier(0);           // keep the fetch ahead of the matrix loop
    const int buf = j & 1;
    const __bf16* yb = wplanes + (size_t)buf * (PY + PX) + tr_row * SY + wn * (TN / WNN) + tr_col;
    const __bf16* xb = wplanes + (size_t)buf * (PY + PX) + PY + tr_row * SX + wk * (TK / WNK) + tr_col;
#pragma unroll
    for (int ks = 0; ks < WG_ROWS / 16; ++ks) {
      bf16x8 a[MT][3], b[KT][3];
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) a[x][pc] = tr_frag(yb + pc * WG_ROWS * SY + ks * 16 * SY + x * 32, SY);
#pragma unroll
      for (int x = 0; x < KT; ++x)
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) b[x][pc] = tr_frag(xb + pc * WG_ROWS * SX + ks * 16 * SX + x * 32, SX);
#pragma unroll
      for (int x = 0; x < MT; ++x)
#pragma unroll
        for (int y = 0; y < KT; ++y) MMG_X6_ALO(acc[x][y], a[x][0], a[x][1], a[x][2], b[y][0], b[y][1], b[y][2]);
    }
    __syncthreads();
  };
  static_assert(RING % 2 == 0, "the LDS buffer parity must follow the ring slot");
  for (int s = 0; s < n_st; s += RING) {         // stages past the end multiply zeros (at most RING - 1 per workgroup)
#pragma unroll
    for (int j = 0; j < RING; ++j) body(s + j, j);
  }
  // slab[split][N*K (+N bias sums)]; with a single split `slab` is dW itself (direct_accumulate: 1 = overwrite, 2 = add)
  float* dst = slab + (size_t)by * slab_stride;
#pragma unroll
  for (int x = 0; x < MT; ++x)
#pragma unroll
    for (int y = 0; y < KT; ++y)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int n = tn0 + wn * (TN / WNN) + x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
        const int k = tk0 + wk * (TK / WNK) + y * 32 + l31;
        float v = acc[x][y][i];
        if (direct_accumulate == 2) v += dst[(size_t)n * K + k];
        dst[(size_t)n * K + k] = v;
      }
  if (dbias && tk0 == 0) {                       // one k-tile column of workgroups owns the bias sums of its TN columns
    float* red = reinterpret_cast<float*>(wplanes);          // the planes are dead: every wave passed the last barrier
    constexpr int GROUPS = NTHR / (TN / 4);
    const int c4 = tid % (TN / 4), grp = tid / (TN / 4);
    *reinterpret_cast<f32x4*>(red + grp * TN + c4 * 4) = bsum;
    __syncthreads();
    if (tid < TN) {
      float t = 0.f;
#pragma unroll
      for (int q = 0; q < GROUPS; ++q) t += red[q * TN + tid];
      float* bdst = direct_accumulate ? dbias : dst + (size_t)N * K;
      if (direct_accumulate == 2) t += bdst[tn0 + tid];
      bdst[tn0 + tid] = t;
    }
  }
}

// Role-specialised variant for the plain (no prologue) 128 x 128 tile.  Waves 0..3 only multiply (a 64 x 64 quadrant
// each, one wave per SIMD), waves 4..7 only stage (loads -> 3-way split -> LDS for stage s+1 while the multipliers work on
// stage s).  The stagers transpose in registers: a stager thread owns an 8-row x 4-column block (8 coalesced 16-B loads),
// splits it and writes, per piece and column, the 8 rows as ONE 16-B entry of a fragment-ordered plane
// [operand][piece][8-row group][column (swizzled)][8 rows]; a multiplier lane fetches a whole MFMA operand fragment with
// one conflict-free ds_read_b128: 24 reads per 48 MFMAs instead of 96 ds_read_b64_tr_b16 (which move 64 B/clk).
// Ablations at [183400 x 128]^T [183400 x 128] (us): empty skeleton 12, loads only 31-33, stagers only 35, multipliers
// only 33 (1075 MFMAs per wave: 42 clocks each against 32 issue-bound), staging + multiplying without loads 46, all 50.
// Staging and multiplying still do not overlap fully (they share the VALU issue port and the LDS), and the fixed
// part (launch, ring priming, slab write, tail) is a quarter of the kernel; the HBM floor of the 188 MB is ~31 us.
__global__ __launch_bounds__(512) void k_linear_wgrad_ws(const float* __restrict__ dY, const float* __restrict__ X,
                                                         float* __restrict__ slab, int64_t M, int N, int K,
                                                         int direct_accumulate, int64_t slab_stride,
                                                         float* __restrict__ dbias) {
  constexpr int TN = 128, TK = 128;
  constexpr int GRP = 128 * 8;                   // one (operand, piece, row group): 128 columns x 8 rows (bf16 elements)
  constexpr int BUF = 2 * 3 * 4 * GRP;           // one stage: 2 operands x 3 pieces x 4 row groups = 48 KB
  extern __shared__ __attribute__((aligned(16))) __bf16 wplanes[];   // [2 buffers][BUF]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tiles_k = K / TK;
  int bx, by;
  xcd_tile_map(&bx, &by);                 // (output tile, stage set): see k_linear_wgrad_x6
  const int tn0 = (bx / tiles_k) * TN, tk0 = (bx % tiles_k) * TK;
  const int64_t total_st = (M + WG_ROWS - 1) / WG_ROWS;
  const int64_t G = gridDim.y;                   // stages are dealt round-robin (see k_linear_wgrad_x6)
  const int n_st = (int64_t)by < total_st ? (int)((total_st - by + G - 1) / G) : 0;
  constexpr int RING = 4;
  const int n_pad = (n_st + RING - 1) / RING * RING;
  float* dst = slab + (size_t)by * slab_stride;

  if (wid >= 4) {
    // ------------------------------------------------------------------ stagers: waves 4,5 stage dY, waves 6,7 stage X
    const int op = wid >> 1 & 1;                             // wave-uniform
    const int t = tid & 127, g = t >> 5, c4 = t & 31;        // 8-row group, column quad
    const float* src = op ? X : dY;
    const int ld = op ? K : N, c0 = op ? tk0 : tn0;
    const int vo = (8 * g * ld + c4 * 4) * 4;
    f32x4 ring[RING][8];
    auto fetch = [&](int st, f32x4* f) {
      const int64_t r0 = ((int64_t)by + (int64_t)st * G) * WG_ROWS;
      const int64_t left = M - r0;
      const int rows = st < n_st ? (left < WG_ROWS ? (int)left : WG_ROWS) : 0;
      const __amdgpu_buffer_rsrc_t rs = mmg_rsrc(src + (size_t)(rows ? r0 : 0) * ld + c0, rows ? (rows * ld - c0) * 4 : 0);
#pragma unroll
      for (int j = 0; j < 8; ++j)
        f[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, vo, j * ld * 4, MMG_NT_WG));
    };
    f32x4 bsum = {0.f, 0.f, 0.f, 0.f};
    auto stage = [&](int st, int buf, const f32x4* f) {
      bf16x8 q[3][4];                             // [piece][column of the quad] = 8 rows
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const f32x4 v = f[j];                      // rows past the end arrive as zeros
        bsum += v;                                 // column sums of dY (the bias gradient); ignored by the X waves
#pragma unroll
        for (int e = 0; e < 4; ++e) MMG_SPLIT3(v[e], q[0][e][j], q[1][e][j], q[2][e][j]);
      }
      // column c of a group sits at entry (c & ~15) | ((c / 4 + 4 (c % 4)) & 15): 16 consecutive lanes then touch 16
      // distinct 16-B bank groups both here (lane = column quad, fixed e) and in the fragment reads (lane = column)
      __bf16* base = wplanes + (size_t)buf * BUF + (size_t)(op * 3 * 4 + g) * GRP + (c4 >> 2) * 128;
#pragma unroll
      for (int pc = 0; pc < 3; ++pc)
#pragma unroll
        for (int e = 0; e < 4; ++e)
          *reinterpret_cast<bf16x8*>(base + pc * 4 * GRP + ((c4 + 4 * e) & 15) * 8) = q[pc][e];
    };
#pragma unroll
    for (int j = 0; j < RING; ++j) fetch(j, ring[j]);
    stage(0, 0, ring[0]);
    fetch(RING, ring[0]);
    __syncthreads();
    for (int s = 0; s < n_pad; s += RING) {
#pragma unroll
      for (int j = 0; j < RING; ++j) {             // stage s+j+1 lives in ring slot (j+1) % RING, LDS buffer (j+1) & 1
        constexpr int dummy = 0; (void)dummy;
        const int jn = (j + 1) % RING;
        stage(s + j + 1, (j + 1) & 1, ring[jn]);
        __builtin_amdgcn_sched_barrier(0);
        fetch(s + j + 1 + RING, ring[jn]);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
      }
    }
    const bool own_bias = dbias && tk0 == 0;       // one k-tile column of workgroups owns the bias sums of its TN columns
    if (own_bias && !op) {
      float* red = reinterpret_cast<float*>(wplanes);        // the planes are dead: every wave passed the last barrier
      *reinterpret_cast<f32x4*>(red + g * TN + c4 * 4) = bsum;
    }
    __syncthreads();
    if (own_bias && !op) {
      const float* red = reinterpret_cast<const float*>(wplanes);
      const float v = red[t] + red[TN + t] + red[2 * TN + t] + red[3 * TN + t];
      float* bdst = direct_accumulate ? dbias : dst + (size_t)N * K;
      bdst[tn0 + t] = direct_accumulate == 2 ? bdst[tn0 + t] + v : v;
    }
  } else {
    // ------------------------------------------------------------------ multipliers: wave w owns quadrant (w >> 1, w & 1)
    const int wn = wid >> 1, wk = wid & 1;
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[a][b][i] = 0.f;
    const int h = lane >> 5, l31 = lane & 31;
    auto entry = [](int c) { return (c & ~15) | (((c >> 2) + 4 * (c & 3)) & 15); };     // the stagers' column swizzle
    int ya[2], xa[2];                              // dY / X entries: row group 2 ks + h, column x * 32 + l31 of the quadrant
#pragma unroll
    for (int x = 0; x < 2; ++x) {
      ya[x] = h * GRP + entry(wn * 64 + x * 32 + l31) * 8;
      xa[x] = 3 * 4 * GRP + h * GRP + entry(wk * 64 + x * 32 + l31) * 8;
    }
    __syncthreads();
    for (int s = 0; s < n_pad; s += 2) {
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (s + j < n_st) {
          const __bf16* pb = wplanes + (size_t)j * BUF;
#pragma unroll
          for (int ks = 0; ks < WG_ROWS / 16; ++ks) {
            bf16x8 a[2][3], b[2][3];
#pragma unroll
            for (int x = 0; x < 2; ++x)
#pragma unroll
              for (int pc = 0; pc < 3; ++pc) {
                a[x][pc] = *reinterpret_cast<const bf16x8*>(pb + ya[x] + (pc * 4 + 2 * ks) * GRP);
                b[x][pc] = *reinterpret_cast<const bf16x8*>(pb + xa[x] + (pc * 4 + 2 * ks) * GRP);
              }
            // small terms first; consecutive MFMAs go to different accumulators
            constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
            for (int tm = 0; tm < 6; ++tm)
#pragma unroll
              for (int x = 0; x < 2; ++x)
#pragma unroll
                for (int y = 0; y < 2; ++y)
                  acc[x][y] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[x][PA[tm]], b[y][PB[tm]], acc[x][y], 0, 0, 0);
          }
        }
        __syncthreads();
      }
    }
    // slab[split][N*K (+N bias sums)]; with a single split `slab` is dW itself (direct_accumulate: 1 = overwrite, 2 = add)
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          const int n = tn0 + wn * 64 + x * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
          const int k = tk0 + wk * 64 + y * 32 + l31;
          float v = acc[x][y][i];
          if (direct_accumulate == 2) v += dst[(size_t)n * K + k];
          dst[(size_t)n * K + k] = v;
        }
    __syncthreads();                               // pairs with the stagers' bias-sum barrier
  }
}

int launch_wgrad_ws(dim3 grid, hipStream_t st, const float* dY, const float* X, float* target, int64_t M, int N, int K,
                    int direct, int64_t slab_stride, float* dbias) {
  constexpr int lds = 2 * 2 * 3 * 4 * 128 * 8 * 2;             // two stages of fragment-ordered planes: 96 KB
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_wgrad_ws, lds>::set()), "linear_wgrad(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD, M, N, K, 0, k_linear_wgrad_ws, grid, dim3(512), lds, st, dY, X, target, M, N, K,
             direct, slab_stride, dbias);
  return MMG_OK;
}

template <int TN, int TK, int WNN, int WNK, bool PRO>
int launch_wgrad_x6_v(dim3 grid, hipStream_t st, const float* dY, const float* X, const ProDev& pr, float* target, int64_t M,
                      int N, int K, int64_t rps, int direct, int64_t slab_stride, float* dbias) {
  constexpr int lds = 2 * 3 * WG_ROWS * ((TN + 32) + (TK + 32)) * 2;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_wgrad_x6<TN, TK, WNN, WNK, PRO>, lds>::set()), "linear_wgrad(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD, M, N, K, PRO ? 4 : 0, (k_linear_wgrad_x6<TN, TK, WNN, WNK, PRO>), grid,
             dim3(64 * WNN * WNK), lds, st, dY, X, pr, target, M, N, K, rps, direct, slab_stride, dbias);
  return MMG_OK;
}

template <int TN, int TK, int WNN, int WNK>
int launch_wgrad_x6(dim3 grid, hipStream_t st, const float* dY, const float* X, const ProDev& pr, float* target, int64_t M,
                    int N, int K, int64_t rps, int direct, int64_t slab_stride, float* dbias) {
  if (pr.scale || pr.relu || pr.p > 0.f)
    return launch_wgrad_x6_v<TN, TK, WNN, WNK, true>(grid, st, dY, X, pr, target, M, N, K, rps, direct, slab_stride, dbias);
  return launch_wgrad_x6_v<TN, TK, WNN, WNK, false>(grid, st, dY, X, pr, target, M, N, K, rps, direct, slab_stride, dbias);
}

struct EpiStore {
  float* out; int accumulate;
  float* out2; int64_t n4_first;          // elements past n4_first float4s go to out2 (the bias sums behind a dW slab)
  __device__ void operator()(int64_t i4, f32x4 v) const {
    f32x4* o = i4 < n4_first ? reinterpret_cast<f32x4*>(out) + i4 : reinterpret_cast<f32x4*>(out2) + (i4 - n4_first);
    *o = accumulate ? (*o + v) : v;
  }
};

struct WgradPlan { int TN, TK, n_tiles, n_split; int64_t rows_per_split; };
WgradPlan plan_wgrad(int64_t M, int N, int K) {
  WgradPlan p;
  p.TN = (N % 128 == 0) ? 128 : 64;
  p.TK = (K % 128 == 0) ? 128 : 64;
  p.n_tiles = (N / p.TN) * (K / p.TK);
  int64_t max_split = (M + WG_ROWS - 1) / WG_ROWS;
  if (max_split < 1) max_split = 1;
  int64_t want = 256 / p.n_tiles;         // one workgroup per CU
  if (want < 1) want = 1;
  p.n_split = (int)(want < max_split ? want : max_split);
  if (M <= 256) p.n_split = 1;            // vocab-side tables: one workgroup per output tile, direct write
  int64_t rps = (M + p.n_split - 1) / p.n_split;
  rps = (rps + WG_ROWS - 1) / WG_ROWS * WG_ROWS;
  if (rps < WG_ROWS) rps = WG_ROWS;
  p.rows_per_split = rps;
  p.n_split = (int)((M + rps - 1) / rps);
  if (p.n_split < 1) p.n_split = 1;
  return p;
}

// the FW form (K = N = 128): grid.y = plan_wgrad's n_split, one eight-wave workgroup per CU
inline int64_t bnbwd_fw_rows(int64_t M) { return plan_wgrad(M, 128, 128).n_split; }

template <int MODE>
int launch_bnbwd_fw(const float* G, const BnBwdDev& bb, const ProDev& pr, const ProDev& pr2, const float* W, float* DX,
                    int64_t M, const BnWgDev& wg, hipStream_t st) {
  constexpr int K = 128, N = 128;
  const int64_t gy = bnbwd_fw_rows(M);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2 + 2 * 3 * 32 * (N + 32) * 2;    // dZ planes + X planes: 111 KB
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_bnbwd_x6<K, 4, MODE, false, true>, lds>::set()), "linear_bnbwd_wgrad(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, (MODE == 1 ? 64 : (MODE == 2 ? 16 | 128 : (MODE == 3 ? 16 | 256 : 16))) | 1024,
             (k_linear_bnbwd_x6<K, 4, MODE, false, true>), dim3(1u, (unsigned)gy), dim3(512), lds, st, G, bb, pr, W, DX, M,
             pr2, next_bn_none(), nullptr, wg, bn_dual_none(), bn_rider_none());
  return 0;
}

// the FW form with the masked dX store (MSK 1: DX = dropout(dX), 2: DX += dropout(dX), under the mask of wg.xpr): + the keep
// bits of both buffers' tiles behind the X planes; flag 8192 = masked
template <int MODE, int MSK>
int launch_bnbwd_fw_masked(const float* G, const BnBwdDev& bb, const ProDev& pr, const float* W, float* DX, int64_t M,
                           const BnWgDev& wg, hipStream_t st) {
  constexpr int K = 128, N = 128;
  const int64_t gy = bnbwd_fw_rows(M);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2 + 2 * 3 * 32 * (N + 32) * 2 + 2 * (N / 4) * (32 + 4);    // + 2.3 KB: 113 KB
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_bnbwd_x6<K, 4, MODE, false, true, MSK>, lds>::set()), "linear_bnbwd_masked(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, (MODE == 3 ? 16 | 256 : 16) | 1024 | 8192,
             (k_linear_bnbwd_x6<K, 4, MODE, false, true, MSK>), dim3(1u, (unsigned)gy), dim3(512), lds, st, G, bb, pr, W, DX, M,
             mmg_pro_dev(nullptr), next_bn_none(), nullptr, wg, bn_dual_none(), bn_rider_none());
  return 0;
}

// the dual form (MSK 3): pass B = MODE 0 / MSK 1 and pass A = MODE 3 / MSK 2 of the same layer in one launch; + the two
// passes' BatchNorm constants and the X fold behind the keep bits (7 KB: 120 KB).  The row prices G_B, y_B, y_A and X in and dX out
// (flag 128: one more [M, K] input); flag 16384 = dual backward
int launch_bnbwd_fw_dual(const float* Gb, const BnBwdDev& bbb, const ProDev& prb, const BnWgDev& wgb, const float* Ga,
                         const BnBwdDev& bba, const ProDev& pra, const BnWgDev& wga, const float* W, float* DX, int64_t M,
                         hipStream_t st) {
  constexpr int K = 128, N = 128;
  const int64_t gy = bnbwd_fw_rows(M);
  constexpr int lds = 2 * 3 * 32 * (K + 8) * 2 + 2 * 3 * 32 * (N + 32) * 2 + 2 * (N / 4) * (32 + 4) + (2 * 6 * K + 2 * N) * 4;
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_bnbwd_x6<K, 4, 0, false, true, 3>, lds>::set()), "linear_bnbwd_dual(attr)");
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, 16 | 128 | 1024 | 8192 | 16384, (k_linear_bnbwd_x6<K, 4, 0, false, true, 3>),
             dim3(1u, (unsigned)gy), dim3(512), lds, st, Gb, bbb, prb, W, DX, M, mmg_pro_dev(nullptr), next_bn_none(), nullptr,
             wgb, BnDualDev{Ga, bba, pra, wga}, bn_rider_none());
  return 0;
}

// ---------------------------------------------------------------------------- data gradient + weight gradient of a pair head's first layer
// k_linear_dgrad_wgrad_x6: DX [M, 128] = dY . W (W [64, 128], the forward weight in place) AND the slabs of
// dW [64, 128] = dY^T . pro(X) in one pass over dY [M, 64] and X [M, 128] -- k_linear_fwd_x6<64, 4, false, false, false, NBN>
// and k_linear_wgrad_x6<64, 128, 2, 4, PRO> each read both tensors (with NBN, X is the next BatchNorm's y) and split dY.
// The skeleton of k_linear_bnbwd_x6<..., FW = true>: one 512-thread workgroup per CU, tiles dealt round-robin over
// gridDim.y = plan_wgrad(M, 64, 128).n_split workgroups -- the row set and the 32-row stage order of the separate
// weight-gradient kernel's slab -- one barrier per tile, per-tile buffer descriptors, the first tile pair peeled.
//   waves 0..3  the body of k_linear_fwd_x6<64, 4, ...>: stage the 32 x 64 dY tile (MMG_SPLIT3, three bf16 planes, two tiles
//               in flight in registers), the W pieces of the wave's 32 columns in 48 registers, MMG_X6_ALO over the four
//               k-steps in order, store, next_bn_tile -> DX and the per-tile statistics are that kernel's bit for bit
//   waves 4..7  stage the 32 x 128 tile of X (affine + ReLU, one split; two tiles in flight) and each hold the 64 x 32 column
//               block w of dW as two accumulators; the operands come through the transposing LDS read from the dY planes
//               and the X planes, the six products per accumulator and 16-row step in k_linear_wgrad_x6's order (both
//               kernels split dY with MMG_SPLIT3: the pieces are the same), so the slab is that kernel's bit for bit
// dY planes: 128-byte rows without padding, the 16-byte chunk c of row r stored at chunk  c ^ f(r),
// f(r) = 4 ((r >> 1) & 1) | ((r >> 2) & 3).  No plain row stride serves both readers: the row reads (ds_read_b128, a
// 16-lane group = 16 rows, one chunk each) need stride / 16 B odd, the transposing reads (4 rows x 64 B per half wave) need
// it = 64 or 192 B mod 256.  With the XOR the 8 rows of one parity in a 16-lane group get 8 distinct chunks (all 64 banks),
// and the rows q, q + 2 of a transposed block land in different 64-byte halves of their 128 bytes (bit 2 of f), q and q + 1
// in different 128-byte halves of the 256-byte bank line: both reads are conflict-free, and the planes take 24 KB instead of
// the 27 (row-read stride) or 37 KB (transposing stride).  X planes: row stride + 64 B as in k_linear_wgrad_x6.
struct DgWgDev { const float* X; ProDev xpr; float* slab; int64_t slab_stride; };

template <bool NBN>
__global__ __launch_bounds__(512, 1) void k_linear_dgrad_wgrad_x6(
    const float* __restrict__ dY, const float* __restrict__ W, float* __restrict__ DX, int64_t M, NextBnDev nb,
    double* __restrict__ stat_partial, DgWgDev wg) {
  constexpr int K = 64, N = 128, NK = K / 16, NTHR = 256, BM = 32;
  constexpr int PZ = BM * K;               // one dY plane (bf16 elements)
  constexpr int SX = N + 32;               // X plane row stride: +64 B puts the 4 rows of a transposing read on disjoint banks
  extern __shared__ __attribute__((aligned(16))) __bf16 planes[];     // [2 buffers][3 pieces][BM][K] of dY + [2][3][BM][SX] of X
  const int tid = threadIdx.x, lane = tid & 63, wn = tid >> 6;
  const int h = lane >> 5, l31 = lane & 31;
  const bool xrole = tid >= NTHR;          // (wave-uniform) the X stagers / dW multipliers
  // element offset of (row r, column c) in a dY plane
  auto zoff = [](int r, int c) __attribute__((always_inline)) -> int {
    const int f = (((r >> 1) & 1) << 2) | ((r >> 2) & 3);
    return r * K + ((((c >> 3) ^ f)) << 3) + (c & 7);
  };
  // (the row-set index through readfirstlane: see k_linear_bnbwd_x6)
  const int by_u = __builtin_amdgcn_readfirstlane((int)blockIdx.y);
  const int64_t n_tiles = (M + BM - 1) / BM;
  const int64_t GY = gridDim.y, t0 = by_u;
  const int n_my = t0 < n_tiles ? (int)((n_tiles - t0 + GY - 1) / GY) : 0;     // tiles t0, t0 + GY, ... (0: a slab of zeros)
  auto rows_of = [&](int64_t tile) __attribute__((always_inline)) -> int {     // valid rows of a tile (0 past the end)
    const int64_t r = M - tile * BM;
    return r <= 0 ? 0 : (r < BM ? (int)r : BM);
  };
  __bf16* xplanes = planes + 2 * 3 * PZ;
  if (xrole) {
    // ---------------------------------------------------------------- X stagers and dW multipliers (waves 4..7)
    wg.xpr.resolve();
    const int t = tid - NTHR, w = wn - 4;
    const int xc4 = t & 31, xr = t >> 5;            // a thread stages the column quad xc4 of rows xr + 8 u
    constexpr int XU = BM * N / 4 / NTHR;           // 16-B loads per thread per tile
    const int xvo = (xr * N + xc4 * 4) * 4;
    f32x4 nxa[XU], nxb[XU];                         // two tiles of X in flight: tiles alternate between them
    auto xfetch = [&](int64_t tile, f32x4* nx) __attribute__((always_inline)) {
      const int rows = rows_of(tile);
      const __amdgpu_buffer_rsrc_t xsrc = mmg_rsrc(wg.X + (size_t)(rows ? tile : 0) * BM * N, rows * N * 4);
#pragma unroll
      for (int u = 0; u < XU; ++u)
        nx[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(xsrc, xvo, u * (NTHR / 32) * N * 4, MMG_NT_WG));
    };
    f32x4 xsc = {1.f, 1.f, 1.f, 1.f}, xsh = {0.f, 0.f, 0.f, 0.f};
    float xfloor = -__builtin_inff();
    const bool xaff = wg.xpr.scale != nullptr || wg.xpr.relu;
    if (wg.xpr.scale) {
      xsc = *reinterpret_cast<const f32x4*>(wg.xpr.scale + xc4 * 4);
      xsh = *reinterpret_cast<const f32x4*>(wg.xpr.shift + xc4 * 4);
    }
    if (wg.xpr.relu) xfloor = 0.f;
    auto xstage = [&](int buf, const f32x4* nx) __attribute__((always_inline)) {
      __bf16* xb = xplanes + (size_t)buf * 3 * BM * SX;
#pragma unroll
      for (int u = 0; u < XU; ++u) {
        const int r = xr + u * (NTHR / 32);
        f32x4 v = nx[u];
        if (xaff) {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaf(v[j], xsc[j], xsh[j]), xfloor);
        }
        // rows past the end need no zeroing: their dY rows are zero
        bf16x4 q0, q1, q2;
#pragma unroll
        for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
        *reinterpret_cast<bf16x4*>(xb + (0 * BM + r) * SX + xc4 * 4) = q0;
        *reinterpret_cast<bf16x4*>(xb + (1 * BM + r) * SX + xc4 * 4) = q1;
        *reinterpret_cast<bf16x4*>(xb + (2 * BM + r) * SX + xc4 * 4) = q2;
      }
    };
    // transposing-read lane roles as in k_linear_wgrad_x6: group g4 fetches rows 8 (g4 >> 1) + q, columns 16 (g4 & 1) + 4 p4
    const int g4 = lane >> 4, q = (lane >> 2) & 3, p4 = lane & 3;
    const int tr_row = 8 * (g4 >> 1) + q, tr_col = 16 * (g4 & 1) + 4 * p4;
    // dY planes: rows +0..3 and +4..7 of the 32-column block x (f does not change with the 16-row step: 16 ks adds 0 to
    // (r >> 1) & 1 and to (r >> 2) & 3)
    int zo[2][2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int u = 0; u < 2; ++u) zo[x][u] = zoff(tr_row + 4 * u, x * 32 + tr_col);
    f32x16 wacc[2];
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int i = 0; i < 16; ++i) wacc[x][i] = 0.f;
    xfetch(t0, nxa);
    xstage(0, nxa);
    xfetch(t0 + GY, nxa);
    xfetch(t0 + 2 * GY, nxb);
    __syncthreads();
    auto wbody = [&](int64_t tt, int buf, f32x4* nx) __attribute__((always_inline)) {
      // nx holds tile tt + GY (fetched two tiles ago); after staging it, the registers take tile tt + 3 GY
      xstage(buf ^ 1, nx);
      xfetch(tt + 3 * GY, nx);
      __builtin_amdgcn_sched_barrier(0);         // keep the fetch ahead of the matrix loop
      const __bf16* zb = planes + (size_t)buf * 3 * PZ;
      const __bf16* xb = xplanes + (size_t)buf * 3 * BM * SX + tr_row * SX + w * 32 + tr_col;
#pragma unroll
      for (int ks = 0; ks < BM / 16; ++ks) {
        bf16x8 fa[2][3], fb[3];
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
#pragma unroll
          for (int x = 0; x < 2; ++x)
            fa[x][pc] = mmg_tr_pair(zb + pc * PZ + ks * 16 * K + zo[x][0], zb + pc * PZ + ks * 16 * K + zo[x][1]);
          fb[pc] = tr_frag(xb + pc * BM * SX + ks * 16 * SX, SX);
        }
        // MMG_X6_ALO's order for each accumulator, the two accumulators' chains interleaved
        constexpr int PA[6] = {2, 0, 1, 1, 0, 0}, PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
        for (int tm = 0; tm < 6; ++tm)
#pragma unroll
          for (int x = 0; x < 2; ++x)
            wacc[x] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[x][PA[tm]], fb[PB[tm]], wacc[x], 0, 0, 0);
      }
      __syncthreads();                           // buf fully read, buf^1 fully written
    };
    wbody(t0, 0, nxa);
    wbody(t0 + GY, 1, nxb);
    for (int i = 2; i < n_my; i += 2) {
      wbody(t0 + (int64_t)i * GY, 0, nxa);
      wbody(t0 + (int64_t)(i + 1) * GY, 1, nxb);
    }
    if constexpr (NBN) __syncthreads();          // pairs with the barrier of the statistics epilogue below
    // slab[row-set][64 x 128], the layout of k_linear_wgrad_x6
    float* dst = wg.slab + (size_t)by_u * wg.slab_stride;
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int i = 0; i < 16; ++i) dst[(size_t)(x * 32 + mmg_c_row(i) + 4 * h) * N + w * 32 + l31] = wacc[x][i];
    return;
  }
  // -------------------------------------------------------------------- dY stagers and DX multipliers (waves 0..3)
  const int col = wn * 32 + l31;
  bf16x8 wb[NK][3];                         // W stored [K, N] (the forward weight, read in place)
  {
    const float* wp = W + (size_t)(8 * h) * N + col;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = wp[(size_t)(ks * 16 + j) * N];
        MMG_SPLIT3(v, wb[ks][0][j], wb[ks][1][j], wb[ks][2][j]);
      }
  }
  NextBnCol nbc = {};
  double cs1 = 0.0, cs2 = 0.0;
  if constexpr (NBN) nbc = next_bn_col(nb, col);
  constexpr int K4 = K / 4, ROWS_PER_PASS = NTHR / K4, NP = BM / ROWS_PER_PASS;
  const int kc4 = tid % K4, prow = tid / K4;
  f32x4 nxa[NP], nxb[NP];                   // two tiles of dY in flight: tiles alternate between them
  const int xvo = (prow * K + kc4 * 4) * 4;
  auto fetch = [&](int64_t tile, f32x4* nx) __attribute__((always_inline)) {
    const int rows = rows_of(tile);
    const __amdgpu_buffer_rsrc_t rs = mmg_rsrc(dY + (size_t)(rows ? tile : 0) * BM * K, rows * K * 4);
#pragma unroll
    for (int p = 0; p < NP; ++p)
      nx[p] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, xvo, p * ROWS_PER_PASS * K * 4, MMG_NT_LD));
  };
  const int zst = zoff(prow, kc4 * 4);      // (f is the same for the rows prow and prow + 16 of the two passes)
  auto stage = [&](int buf, const f32x4* nx) __attribute__((always_inline)) {      // split + three plane writes (rows past the end: zeros)
    __bf16* pb = planes + (size_t)buf * 3 * PZ + zst;
#pragma unroll
    for (int p = 0; p < NP; ++p) {
      const f32x4 v = nx[p];
      bf16x4 q0, q1, q2;
#pragma unroll
      for (int j = 0; j < 4; ++j) MMG_SPLIT3(v[j], q0[j], q1[j], q2[j]);
      *reinterpret_cast<bf16x4*>(pb + 0 * PZ + p * ROWS_PER_PASS * K) = q0;
      *reinterpret_cast<bf16x4*>(pb + 1 * PZ + p * ROWS_PER_PASS * K) = q1;
      *reinterpret_cast<bf16x4*>(pb + 2 * PZ + p * ROWS_PER_PASS * K) = q2;
    }
  };
  int ao[NK];                               // this lane's A fragment of k-step ks: row l31, columns 16 ks + 8 h + 0..7
#pragma unroll
  for (int ks = 0; ks < NK; ++ks) ao[ks] = zoff(l31, ks * 16 + 8 * h);
  fetch(t0, nxa);
  stage(0, nxa);
  fetch(t0 + GY, nxa);
  fetch(t0 + 2 * GY, nxb);
  __syncthreads();
  const int yvo = ((4 * h) * N + col) * 4;     // C/D map: col = lane&31, row = (i&3) + 8*(i>>2) + 4*(lane>>5)
  auto tile_body = [&](int64_t tt, int buf, f32x4* nx) __attribute__((always_inline)) {
    // nx holds tile tt + GY (fetched two tiles ago); after staging it, the registers take tile tt + 3 GY
    const int rows = rows_of(tt);
    const __amdgpu_buffer_rsrc_t xs = mmg_rsrc(DX + (size_t)(rows ? tt : 0) * BM * N, rows * N * 4);
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
    float nby[NBN ? 16 : 1];
    if constexpr (NBN) next_bn_load(nb, tt, rows, N, 0, yvo, nby);   // in flight under the products
    stage(buf ^ 1, nx);                        // the other buffer: its readers passed the barrier of the last tile
    fetch(tt + 3 * GY, nx);
    __builtin_amdgcn_sched_barrier(0);         // keep the fetch ahead of the matrix loop
    const __bf16* ap = planes + (size_t)buf * 3 * PZ;
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const bf16x8 a1 = *reinterpret_cast<const bf16x8*>(ap + ao[ks]);
      const bf16x8 a2 = *reinterpret_cast<const bf16x8*>(ap + PZ + ao[ks]);
      const bf16x8 a3 = *reinterpret_cast<const bf16x8*>(ap + 2 * PZ + ao[ks]);
      MMG_X6_ALO(acc, a1, a2, a3, wb[ks][0], wb[ks][1], wb[ks][2]);
    }
    float vv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      vv[i] = acc[i] + 0.f;                    // (k_linear_fwd_x6 adds its absent bias as +0: a sum that underflowed to -0 becomes +0)
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, vv[i]), xs, yvo, mmg_c_row(i) * N * 4, MMG_NT_ST);
    }
    if constexpr (NBN) next_bn_tile(nb, nbc, vv, nby, rows, tt * BM, N, col, lane, cs1, cs2);
    __syncthreads();                           // buf fully read, buf^1 fully written
  };
  tile_body(t0, 0, nxa);
  tile_body(t0 + GY, 1, nxb);
  for (int i = 2; i < n_my; i += 2) {
    tile_body(t0 + (int64_t)i * GY, 0, nxa);
    tile_body(t0 + (int64_t)(i + 1) * GY, 1, nxb);
  }
  if constexpr (NBN) {
    // two partials per column (the lane halves) -> one: partial[row-set][2][N], fixed order
    double* red = reinterpret_cast<double*>(planes);          // the planes are dead: every wave passed the last barrier
    red[(h * 2 + 0) * N + col] = cs1;
    red[(h * 2 + 1) * N + col] = cs2;
    __syncthreads();
    for (int e = tid; e < 2 * N; e += NTHR) {
      const int which = e / N, cc = e % N;
      stat_partial[((size_t)by_u * 2 + which) * N + cc] = red[which * N + cc] + red[(2 + which) * N + cc];
    }
  }
}

template <bool NBN>
int launch_dgrad_wgrad(const float* dY, const float* W, float* DX, int64_t M, const NextBnDev& nb, double* stat_partial,
                       const DgWgDev& wg, int n_split, bool has_pro, hipStream_t st) {
  constexpr int lds = 2 * 3 * 32 * 64 * 2 + 2 * 3 * 32 * (128 + 32) * 2;      // dY planes + X planes: 84 KB
  MMG_CHECK_HIP((MmgMaxLds<&k_linear_dgrad_wgrad_x6<NBN>, lds>::set()), "linear_dgrad_wgrad(attr)");
  // flags: 4 = the X prologue, 512 = the next-BatchNorm epilogue, 4096 = the weight gradient rides along
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, 128, 64, (has_pro ? 4 : 0) | (NBN ? 512 : 0) | 4096, (k_linear_dgrad_wgrad_x6<NBN>),
             dim3(1u, (unsigned)n_split), dim3(512), lds, st, dY, W, DX, M, nb, stat_partial, wg);
  return 0;
}

template <int K>
int launch_small(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                 int accumulate, hipStream_t st) {
  // (through the probe like the split kernels: a test reads from it on which side of M = 512 a call ran)
  MMG_LAUNCH(MMG_PROBE_LINEAR_FWD, M, N, K, (accumulate & MMG_LIN_ACCUMULATE) | ((pr.scale || pr.relu || pr.p > 0.f) ? 4 : 0),
             (k_linear_small<K>), dim3((unsigned)(N / 32), (unsigned)((M + 31) / 32)), dim3(256), 0, st, X, pr, W, bias, Y, M,
             N, accumulate);
  return 0;
}

}  // namespace

// ---- producer epilogues (mmg_fwd_epi_t, mmg_next_bn_t; include/mmgnn.h): host side shared with aggregate.hip

// workspace: <= 768 partial rows of a fused producer, or (fallback) one row of sums + the separate statistics pass
extern "C" size_t mmg_epi_ws_bytes(int64_t M, int N) {
  if (M < 0 || N <= 0) return 0;
  const size_t a = (size_t)768 * 2 * N * sizeof(double) + 256;
  const size_t b = (size_t)2 * N * sizeof(double) + 512 + mmg_col_reduce2_ws_bytes(M, N);
  return a > b ? a : b;
}

extern "C" int mmg_next_bn_dev(const mmg_next_bn_t* next, int64_t M, int N, const char* what, NextBnDev* d, double** partial) {
  MMG_CHECK_ARG(next->y && next->pro && next->mean && next->rstd && next->sums, "%s: next-BatchNorm descriptor with a null field", what);
  MMG_CHECK_ARG(!next->pro->scale || next->pro->shift, "%s: next BatchNorm: scale without shift", what);
  MMG_CHECK_ARG(next->ws && next->ws_bytes >= mmg_epi_ws_bytes(M, N), "%s: next BatchNorm: workspace too small", what);
  d->Y = next->y; d->mean = next->mean; d->rstd = next->rstd;
  d->pr = mmg_pro_dev(next->pro);
  *partial = MmgCarver(next->ws).take<double>((size_t)768 * 2 * N);
  return MMG_OK;
}
extern "C" int mmg_next_bn_finish(const mmg_next_bn_t* next, const double* partial, int N, int rows, void* stream) {
  return mmg_partial_sum_add(partial, next->sums, 2 * N, rows, next->accumulate ? next->sums : nullptr, stream);
}
extern "C" int mmg_next_bn_fallback(const float* G, int64_t M, int N, const mmg_next_bn_t* next, const char* what, void* stream) {
  NextBnDev d;
  double* tmp;
  int rc = mmg_next_bn_dev(next, M, N, what, &d, &tmp);
  if (rc) return rc;
  unsigned char* rest = (unsigned char*)(tmp + 2 * N);
  const size_t used = (size_t)(rest - (unsigned char*)next->ws);
  rc = mmg_bn_bwd_stats(G, next->y, next->pro, next->mean, next->rstd, next->accumulate ? tmp : next->sums, M, N, rest,
                        next->ws_bytes - used, stream);
  if (rc || !next->accumulate) return rc;
  return mmg_partial_sum_add(tmp, next->sums, 2 * N, 1, next->sums, stream);
}

// what each mode requires of the descriptor (the fields a mode does not name are ignored)
static const struct {
  bool col_sums, next, rnorm;
} kFwdEpiMode[4] = {
    // col_sums next   rnorm
    {false,     false, false},    // NONE
    {true,      false, false},    // STATS (fin nullable)
    {false,     true,  false},    // NEXT_BN
    {false,     false, true},     // L2
};

int mmg_epi_prepare(const mmg_fwd_epi_t* e, int64_t M, int N, const char* what, double** partial, NextBnDev* nb) {
  *partial = nullptr;
  *nb = next_bn_none();
  if (!e) return MMG_OK;
  MMG_CHECK_ARG(e->mode >= MMG_EPI_NONE && e->mode <= MMG_EPI_L2, "%s: unknown epilogue mode %d", what, e->mode);
  const auto& m = kFwdEpiMode[e->mode];
  MMG_CHECK_ARG((e->col_sums || !m.col_sums) && (e->next || !m.next) && (e->rnorm || !m.rnorm),
                "%s: epilogue descriptor with a null field", what);
  MMG_CHECK_ARG(!(e->col_sums && e->next), "%s: forward statistics and next-BatchNorm statistics are exclusive", what);
  if (e->mode == MMG_EPI_NEXT_BN) return mmg_next_bn_dev(e->next, M, N, what, nb, partial);
  if (e->mode != MMG_EPI_STATS) return MMG_OK;
  MMG_CHECK_ARG(M > 0, "%s: statistics of an empty output", what);
  MMG_CHECK_ARG(!e->fin || (e->fin->count > 0 && e->fin->scale && e->fin->shift),
                "%s: BatchNorm fold without count, scale or shift", what);
  MMG_CHECK_ARG(e->ws && e->ws_bytes >= mmg_epi_ws_bytes(M, N), "%s: statistics workspace too small", what);
  *partial = MmgCarver(e->ws).take<double>((size_t)768 * 2 * N);
  return MMG_OK;
}

int mmg_epi_finish(const mmg_fwd_epi_t* e, const float* Y, int64_t M, int N, bool fused, const double* partial, int rows,
                   const char* what, void* stream) {
  if (!e || e->mode == MMG_EPI_NONE || e->mode == MMG_EPI_L2) return MMG_OK;
  if (e->mode == MMG_EPI_NEXT_BN)
    return fused ? mmg_next_bn_finish(e->next, partial, N, rows, stream) : mmg_next_bn_fallback(Y, M, N, e->next, what, stream);
  if (fused) return mmg_partial_sum_bn(partial, e->col_sums, N, rows, e->fin, stream);
  const int rc = mmg_col_reduce2(Y, nullptr, e->col_sums, M, N, e->ws, e->ws_bytes, stream);
  const mmg_bn_fin_t* f = e->fin;
  if (rc || !f) return rc;
  return mmg_bn_finalize(e->col_sums, f->count, f->gamma, f->beta, f->running_mean, f->running_var, 1, f->n_updates, f->momentum,
                         f->eps, f->scale, f->shift, f->mean, f->rstd, N, stream);
}

extern "C" int mmg_linear_fwd_supported(int mode, int64_t M, int N, int K) {
  if (mode < MMG_EPI_NONE || mode > MMG_EPI_L2) return 0;
  if (mode == MMG_EPI_L2) return (M > 512 && (N == 64 || N == 128) && (K == 64 || K == 128)) ? 1 : 0;
  return (M >= 0 && (K == 64 || K == 128 || K == 256) && N > 0 && N % 64 == 0 && N <= 4096) ? 1 : 0;
}

// the launch of a shape, whichever the epilogue: the fp32 kernel for the vocab-side tables (M <= 512), else the exact-product
// 6-term bf16 split on the bf16 matrix cores; epi = the epilogue the launch fuses (mmg_linear_fwd checked that it can)
static int linear_fwd_launch(const float* X, const ProDev& pr, const float* W, const float* bias, float* Y, int64_t M, int N,
                             int K, int flags, int epi, double* partial, float* rnorm, float eps, const NextBnDev& nb,
                             hipStream_t st) {
  if (M <= 512) {
    if (K == 64) return launch_small<64>(X, pr, W, bias, Y, M, N, flags, st);
    if (K == 128) return launch_small<128>(X, pr, W, bias, Y, M, N, flags, st);
    return launch_small<256>(X, pr, W, bias, Y, M, N, flags, st);
  }
  if (K == 64)
    return N % 128 == 0 ? launch_fwd_x6<64, 4>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb)
                        : launch_fwd_x6<64, 2>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb);
  if (K == 128)
    return N % 128 == 0 ? launch_fwd_x6<128, 4>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb)
                        : launch_fwd_x6<128, 2>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb);
  if (N % 256 == 0) return launch_fwd_h3_k256(X, pr, W, bias, Y, M, N, flags, st, partial);   // one workgroup spans 256 columns
  // (K = 256 with a 64-wide output: the heads' first layer at 256-d)
  return N % 128 == 0 ? launch_fwd_x6<256, 4>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb)
                      : launch_fwd_x6<256, 2>(X, pr, W, bias, Y, M, N, flags, st, partial, epi, rnorm, eps, nb);
}

extern "C" int mmg_linear_fwd(const float* X, const mmg_prologue_t* pro, const float* W, const float* bias, float* Y,
                              int64_t M, int N, int K, int flags, const mmg_fwd_epi_t* epi, void* stream) {
  const char* what = "linear_fwd";
  const int mode = epi ? epi->mode : MMG_EPI_NONE;
  double* partial;
  NextBnDev nb;
  int rc = mmg_epi_prepare(epi, M, N, what, &partial, &nb);
  if (rc) return rc;
  MMG_CHECK_ARG(mmg_linear_fwd_supported(mode, M, N, K), "%s: M=%lld N=%d K=%d unsupported (%s)", what, (long long)M, N, K,
                mode == MMG_EPI_L2 ? "L2 epilogue: M > 512, N and K in {64,128}"
                                   : "K in {64,128,256}, N a multiple of 64 up to 4096");
  MMG_CHECK_ARG((flags & ~(MMG_LIN_ACCUMULATE | MMG_LIN_W_KN)) == 0, "%s: unknown flag bits", what);
  MMG_CHECK_ARG(mode != MMG_EPI_L2 || flags == 0, "%s: the L2 epilogue takes no flags", what);
  if (M == 0) return mmg_epi_finish(epi, Y, 0, N, false, nullptr, 0, what, stream);
  MMG_CHECK_ARG(X && W && Y, "%s: null buffer", what);
  MMG_CHECK_ARG(!pro || !pro->scale || pro->shift, "%s: prologue scale without shift", what);
  MMG_CHECK_ARG(!pro || pro->relu == MMG_ACT_NONE || pro->relu == MMG_ACT_RELU, "%s: the prologue takes relu only", what);
  const ProDev pr = mmg_pro_dev(pro);
  // STATS and L2 come with every bf16-split launch; NEXT_BN only with the instances of a plain K <= 128 linear
  bool fused = mode != MMG_EPI_NONE && M > 512;
  if (mode == MMG_EPI_NEXT_BN)
    fused = fused && N % 128 == 0 && K <= 128 && !(flags & MMG_LIN_ACCUMULATE) && !(pr.scale || pr.relu || pr.p > 0.f) &&
            mmg_next_bn_fusable(epi->next);
  hipStream_t st = (hipStream_t)stream;
  rc = linear_fwd_launch(X, pr, W, bias, Y, M, N, K, flags, fused ? mode : MMG_EPI_NONE, fused ? partial : nullptr,
                         mode == MMG_EPI_L2 ? epi->rnorm : nullptr, mode == MMG_EPI_L2 ? epi->eps : 0.f, nb, st);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  const int rows = (int)(K == 256 && N % 256 == 0 ? fwd_k256_rows(M, N) : fwd_x6_rows(M, N, N % 128 == 0 ? 128 : 64, K));
  return mmg_epi_finish(epi, Y, M, N, fused, partial, rows, what, stream);
}

extern "C" int mmg_linear_fwd_dual_supported(int64_t M, int N, int K) { return (M > 512 && N == 128 && K == 128) ? 1 : 0; }

extern "C" int mmg_linear_fwd_dual(const float* X, const mmg_prologue_t* pro0, const mmg_prologue_t* pro1, const float* W,
                                   const float* bias, float* Y0, float* Y1, int64_t M, int N, int K,
                                   const mmg_fwd_epi_t* epi0, const mmg_fwd_epi_t* epi1, void* stream) {
  const char* what = "linear_fwd_dual";
  MMG_CHECK_ARG(mmg_linear_fwd_dual_supported(M, N, K), "%s: M=%lld N=%d K=%d unsupported (M > 512, N = K = 128)", what,
                (long long)M, N, K);
  MMG_CHECK_ARG(X && W && Y0 && Y1 && Y0 != Y1 && pro0 && pro1, "%s: null buffer or prologue, or one output for both passes", what);
  MMG_CHECK_ARG(pro0->drop_p > 0.f, "%s: the two passes differ by their dropout masks only: drop_p > 0", what);
  MMG_CHECK_ARG(pro0->scale == pro1->scale && pro0->shift == pro1->shift && pro0->relu == pro1->relu &&
                    pro0->drop_p == pro1->drop_p && pro0->seed == pro1->seed && pro0->seed_ptr == pro1->seed_ptr &&
                    pro0->row_offset == pro1->row_offset,
                "%s: the two prologues must agree in everything but the site", what);
  MMG_CHECK_ARG(pro0->site != pro1->site, "%s: the two prologues have the same site", what);
  MMG_CHECK_ARG(!pro0->scale || pro0->shift, "%s: prologue scale without shift", what);
  MMG_CHECK_ARG(pro0->relu == MMG_ACT_NONE || pro0->relu == MMG_ACT_RELU, "%s: the prologue takes relu only", what);
  MMG_CHECK_ARG(epi0 && epi1 && epi0->mode == MMG_EPI_STATS && epi1->mode == MMG_EPI_STATS, "%s: both epilogues are MMG_EPI_STATS", what);
  double *part0, *part1;
  NextBnDev nb;
  int rc = mmg_epi_prepare(epi0, M, N, what, &part0, &nb);
  if (rc) return rc;
  rc = mmg_epi_prepare(epi1, M, N, what, &part1, &nb);
  if (rc) return rc;
  const size_t part_bytes = (size_t)768 * 2 * N * sizeof(double);
  const uintptr_t a = (uintptr_t)part0, b = (uintptr_t)part1;
  MMG_CHECK_ARG((a > b ? a - b : b - a) >= part_bytes && epi0->col_sums != epi1->col_sums,
                "%s: the two epilogues share a workspace or their sums", what);
  hipStream_t st = (hipStream_t)stream;
  rc = launch_fwd_x6_dual(X, mmg_pro_dev(pro0), mmg_pro_dev(pro1), W, bias, Y0, Y1, M, st, part0, part1);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  return mmg_partial_sum_bn2(part0, part1, epi0->col_sums, epi1->col_sums, N, (int)fwd_x6_rows(M, N, 128, K), epi0->fin,
                             epi1->fin, stream);
}

extern "C" int mmg_linear_fwd_rider_supported(int64_t M, int N, int K, int64_t n_sel) {
  // the dense launch: the L2 instance of the 128 x 128 layer; the rider: nothing, or a list the library's own compact
  // launch would hand to that same instance (up to 512 rows it takes the fp32 kernel of the small tables, whose sums the
  // matrix-core arithmetic does not reproduce)
  if (!(M > 512 && N == 128 && K == 128)) return 0;
  return (n_sel == 0 || (n_sel > 512 && n_sel <= M)) ? 1 : 0;
}

extern "C" int mmg_linear_fwd_rider(const float* X, const mmg_prologue_t* pro, const float* W, const float* bias, float* Y,
                                    int64_t M, int N, int K, const mmg_fwd_epi_t* epi, const float* X_a,
                                    const mmg_prologue_t* pro_a, const int64_t* rows, int64_t n_sel, const float* W_a,
                                    const float* bias_a, float* act_a, float* Y_a, const mmg_fwd_epi_t* epi_a, void* stream) {
  const char* what = "linear_fwd_rider";
  MMG_CHECK_ARG(mmg_linear_fwd_rider_supported(M, N, K, n_sel),
                "%s: M=%lld N=%d K=%d n_sel=%lld unsupported (M > 512, N = K = 128, n_sel = 0 or 512 < n_sel <= M)", what,
                (long long)M, N, K, (long long)n_sel);
  MMG_CHECK_ARG(epi && epi->mode == MMG_EPI_L2 && epi->rnorm, "%s: the dense launch takes the L2 epilogue", what);
  MMG_CHECK_ARG(X && W && Y, "%s: null buffer", what);
  MMG_CHECK_ARG(pro && (pro->scale || pro->relu || pro->drop_p > 0.f), "%s: the dense launch needs a prologue", what);
  MMG_CHECK_ARG(!pro->scale || pro->shift, "%s: prologue scale without shift", what);
  MMG_CHECK_ARG(pro->relu == MMG_ACT_NONE || pro->relu == MMG_ACT_RELU, "%s: the prologue takes relu only", what);
  if (n_sel == 0) return mmg_linear_fwd(X, pro, W, bias, Y, M, N, K, 0, epi, stream);
  MMG_CHECK_ARG(W_a == W && bias_a == bias, "%s: the rider runs on the dense launch's W and bias", what);
  MMG_CHECK_ARG(epi_a && epi_a->mode == MMG_EPI_L2 && epi_a->rnorm && epi_a->eps == epi->eps,
                "%s: the rider takes the L2 epilogue with the dense launch's eps", what);
  MMG_CHECK_ARG(X_a && rows && act_a && Y_a, "%s: null rider buffer", what);
  MMG_CHECK_ARG(!pro_a || !pro_a->scale || pro_a->shift, "%s: rider prologue scale without shift", what);
  {
    // the rider's outputs against the dense launch's outputs and everything either of them reads
    struct Span { const void* p; size_t n; };
    const size_t mk = (size_t)M * K * 4, sk = (size_t)n_sel * K * 4;
    const Span outs[3] = {{act_a, sk}, {Y_a, (size_t)n_sel * N * 4}, {epi_a->rnorm, (size_t)n_sel * 4}};
    const Span others[6] = {{X, mk}, {Y, (size_t)M * N * 4}, {epi->rnorm, (size_t)M * 4}, {X_a, mk},
                            {rows, (size_t)n_sel * 8}, {W, (size_t)N * K * 4}};
    auto overlap = [](const Span& a, const Span& b) {
      const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
      return a0 < b0 + b.n && b0 < a0 + a.n;
    };
    bool alias = false;
    for (int i = 0; i < 3; ++i) {
      for (int j = 0; j < 6; ++j) alias = alias || overlap(outs[i], others[j]);
      for (int j = i + 1; j < 3; ++j) alias = alias || overlap(outs[i], outs[j]);
    }
    MMG_CHECK_ARG(!alias, "%s: a rider output aliases a tensor of the launch", what);
  }
  FwdRiderDev rd;
  rd.X = X_a; rd.pr = mmg_pro_dev(pro_a); rd.rows = rows; rd.n_sel = n_sel;
  rd.act = act_a; rd.Y = Y_a; rd.rn = epi_a->rnorm;
  const int rc = launch_fwd_x6_rider(X, mmg_pro_dev(pro), W, bias, Y, M, (hipStream_t)stream, epi->rnorm, epi->eps, rd);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  return MMG_OK;
}

extern "C" int mmg_linear_bnbwd_supported(int mode, int64_t M, int N, int K, int with_wgrad) {
  if (mode < MMG_BNBWD_BN || mode > MMG_BNBWD_ROWS || M <= 512) return 0;
  // BN and L2 have instances for K, N in {64, 128}; BN2, ROWS and the FW form only K = N = 128
  if (mode == MMG_BNBWD_BN2 || mode == MMG_BNBWD_ROWS || with_wgrad) return (K == 128 && N == 128) ? 1 : 0;
  return ((K == 64 || K == 128) && (N == 64 || N == 128)) ? 1 : 0;
}

extern "C" size_t mmg_linear_bnbwd_wgrad_ws_bytes(int64_t M, int N, int K) {
  return mmg_linear_wgrad_ws_bytes(M, K, N);            // the slabs of the separate weight gradient of dZ [M, K], X [M, N]
}

// the FW launch of one mode (k_linear_bnbwd_x6<128, 4, MODE, NBN, true>): the weight-gradient descriptor, the next
// BatchNorm's statistics (fused, or the separate pass over dX), the slab sum (deferred to wg->job, or now)
// the weight-gradient descriptor of an FW launch: the job reset, the checks, the slabs carved from wg->ws
static int bnbwd_wgrad_prepare(const mmg_bnbwd_wgrad_t* wg, int64_t M, const char* what, BnWgDev* wd) {
  constexpr int N = 128, K = 128;
  mmg_wgrad_reduce_t* job = wg->job;
  if (job) { job->slab = nullptr; job->n4 = 0; job->n_split = 0; job->dW = wg->dW; job->dbias = wg->dbias; job->nk4 = (int64_t)K * N / 4; job->accumulate = wg->accumulate; }
  MMG_CHECK_ARG(wg->X && wg->dW && wg->ws, "%s: null weight-gradient buffer", what);
  MMG_CHECK_ARG(!wg->pro || wg->pro->relu == MMG_ACT_NONE || wg->pro->relu == MMG_ACT_RELU, "%s: the X prologue takes relu only", what);
  MMG_CHECK_ARG(!wg->pro || !wg->pro->scale || wg->pro->shift, "%s: X prologue: scale without shift", what);
  void* const ws = wg->ws;
  const size_t ws_bytes = wg->ws_bytes, need = mmg_linear_bnbwd_wgrad_ws_bytes(M, N, K);
  MMG_CHECK_WS(what, need);
  float* slab = MmgCarver(ws).take<float>((need - 256) / sizeof(float));
  const int64_t stride = (int64_t)K * N + (wg->dbias ? K : 0);
  const ProDev xpr = mmg_pro_dev(wg->pro);
  // the column sums of dZ in the order of the kernel linear_wgrad runs for this X (see linear_wgrad_impl)
  *wd = BnWgDev{wg->X, xpr, slab, stride, (xpr.scale || xpr.relu || xpr.p > 0.f) ? 1 : 0};
  return MMG_OK;
}
// the slab sum of an FW launch: deferred to wg->job, or now
static int bnbwd_wgrad_finish(const mmg_bnbwd_wgrad_t* wg, const BnWgDev& wd, int64_t M, const char* what, hipStream_t st) {
  constexpr int N = 128, K = 128;
  mmg_wgrad_reduce_t* job = wg->job;
  float* const slab = wd.slab;
  const int64_t stride = wd.slab_stride;
  const int n_split = (int)bnbwd_fw_rows(M);
  if (job) {                        // the caller sums the slabs later, together with those of other layers
    job->slab = slab; job->n4 = stride / 4; job->n_split = n_split;
  } else {
    MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD_REDUCE, M, K, N, 0, (mmg_k_reduce_slabs<EpiStore>),
               dim3((unsigned)((stride / 4 + 15) / 16)), dim3(256), 0, st, slab, stride / 4, n_split,
               EpiStore{wg->dW, wg->accumulate, wg->dbias, (int64_t)K * N / 4});
    MMG_CHECK_LAUNCH(what);
  }
  return MMG_OK;
}

template <int MODE>
static int bnbwd_wgrad_run(const float* G, const BnBwdDev& bb, const ProDev& pr, const ProDev& pr2, const float* W, float* dX,
                           int64_t M, const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, const char* what,
                           hipStream_t st, int msk = 0) {
  constexpr int N = 128;
  BnWgDev wd;
  int rc = bnbwd_wgrad_prepare(wg, M, what, &wd);
  if (rc) return rc;
  // the next BatchNorm's statistics always come from the separate pass over dX: the epilogue that sums them does not fit
  // beside the dW waves (k_linear_bnbwd_x6<128, 4, MODE, true, true> spills 124..220 B per lane at the 256-register budget
  // of two waves per SIMD, which the plain NBN instances already exceed by 40..136 B)
  rc = MMG_E_ARG;
  if (!msk) rc = launch_bnbwd_fw<MODE>(G, bb, pr, pr2, W, dX, M, wd, st);
  if constexpr (MODE == MMG_BNBWD_BN || MODE == MMG_BNBWD_ROWS) {      // msk: the masked dX store (mmg_linear_bnbwd_masked)
    if (msk == 1) rc = launch_bnbwd_fw_masked<MODE, 1>(G, bb, pr, W, dX, M, wd, st);
    if (msk == 2) rc = launch_bnbwd_fw_masked<MODE, 2>(G, bb, pr, W, dX, M, wd, st);
  }
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  rc = next ? mmg_next_bn_fallback(dX, M, N, next, what, st) : MMG_OK;
  if (rc) return rc;
  return bnbwd_wgrad_finish(wg, wd, M, what, st);
}

// one mode: the FW instance when the weight gradient rides along; else the NBN instance when the next BatchNorm's
// statistics fit its epilogue; else the plain instance of the shape (+ the separate statistics pass over dX)
template <int MODE>
static int bnbwd_run(const float* G, const BnBwdDev& bb, const ProDev& pr, const ProDev& pr2, const float* W, float* dX,
                     int64_t M, int N, int K, const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, const char* what,
                     hipStream_t st, int msk) {
  if (wg) return bnbwd_wgrad_run<MODE>(G, bb, pr, pr2, W, dX, M, next, wg, what, st, msk);
  int rc;
  if constexpr (MODE != MMG_BNBWD_BN2) {          // no NBN instance (the entry point refuses next)
    if (next && K == 128 && N == 128 && mmg_next_bn_fusable(next)) {
      NextBnDev nb;
      double* partial;
      rc = mmg_next_bn_dev(next, M, N, what, &nb, &partial);
      if (rc) return rc;
      rc = launch_bnbwd_x6<128, 4, MODE, true>(G, bb, pr, W, dX, M, st, pr2, nb, partial);
      if (rc) return rc;
      MMG_CHECK_LAUNCH(what);
      return mmg_next_bn_finish(next, partial, N, (int)bnbwd_x6_rows(M, K), st);
    }
  }
  if constexpr (MODE == MMG_BNBWD_BN2 || MODE == MMG_BNBWD_ROWS) rc = launch_bnbwd_x6<128, 4, MODE>(G, bb, pr, W, dX, M, st, pr2);
  else if (K == 128) rc = N == 128 ? launch_bnbwd_x6<128, 4, MODE>(G, bb, pr, W, dX, M, st) : launch_bnbwd_x6<128, 2, MODE>(G, bb, pr, W, dX, M, st);
  else rc = N == 128 ? launch_bnbwd_x6<64, 4, MODE>(G, bb, pr, W, dX, M, st) : launch_bnbwd_x6<64, 2, MODE>(G, bb, pr, W, dX, M, st);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  return next ? mmg_next_bn_fallback(dX, M, N, next, what, st) : MMG_OK;
}

// what each mode requires of the descriptor besides y (the fields a mode does not name are ignored)
static const struct {
  const char* name;
  bool G, G2, row_pos, pro, pro2, rnorm;
} kBnBwdMode[4] = {
    //                       G      G2     row_pos pro    pro2   rnorm
    {"linear_bnbwd",         true,  false, false,  false, false, false},    // pro NULL: relu only, no BatchNorm
    {"linear_l2bwd",         true,  false, false,  false, false, true},
    {"linear_bnbwd2",        true,  true,  false,  true,  true,  false},
    {"linear_bnbwd_rows",    false, false, true,   true,  false, false},    // G NULL iff n_sel == 0 (checked below)
};

// a validated call: the device descriptors of its mode
struct BnBwdCall {
  BnBwdDev bb; ProDev pr, pr2; const float* G; const char* what;
};
static int bnbwd_marshal(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                         const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, BnBwdCall* call) {
  MMG_CHECK_ARG(a, "linear_bnbwd: null descriptor");
  MMG_CHECK_ARG(a->mode >= MMG_BNBWD_BN && a->mode <= MMG_BNBWD_ROWS, "linear_bnbwd: unknown mode %d", a->mode);
  const auto& m = kBnBwdMode[a->mode];
  const char* what = m.name;
  MMG_CHECK_ARG(!next || a->mode != MMG_BNBWD_BN2, "%s: no next-BatchNorm statistics with two upstream gradients", what);
  MMG_CHECK_ARG(mmg_linear_bnbwd_supported(a->mode, M, N, K, wg != nullptr), "%s: M=%lld N=%d K=%d%s unsupported", what,
                (long long)M, N, K, wg ? " with a weight gradient" : "");
  MMG_CHECK_ARG(a->y && W && (dZ || wg) && dX && (a->G || !m.G) && (a->G2 || !m.G2) && (a->row_pos || !m.row_pos) &&
                    (a->pro || !m.pro) && (a->pro2 || !m.pro2) && (a->rnorm || !m.rnorm),
                "%s: null buffer", what);
  const bool l2 = a->mode == MMG_BNBWD_L2, rows = a->mode == MMG_BNBWD_ROWS;
  if (rows)
    MMG_CHECK_ARG(a->n_sel >= 0 && a->n_sel * (int64_t)K * 4 < (int64_t)0x7FFFFFFF && (a->G || a->n_sel == 0),
                  "%s: bad row list", what);
  if (!l2) {
    const mmg_prologue_t* pro = a->pro;
    MMG_CHECK_ARG(!pro || !pro->scale || (pro->shift && a->mean && a->rstd), "%s: BatchNorm fold without shift / mean / rstd", what);
    MMG_CHECK_ARG(!pro || pro->relu == MMG_ACT_NONE || pro->relu == MMG_ACT_RELU, "%s: relu only", what);
    MMG_CHECK_ARG(!a->sums || (pro && pro->scale), "%s: sums without a BatchNorm fold", what);
  }
  call->bb = l2 ? BnBwdDev{a->y, a->rnorm, nullptr, nullptr, 0.0, dZ, nullptr, nullptr, a->eps, nullptr, nullptr, 0}
                         : BnBwdDev{a->y, a->mean, a->rstd, a->sums, a->inv_count, dZ, a->dbeta, a->dgamma, 0.f,
                                    a->mode == MMG_BNBWD_BN2 ? a->G2 : nullptr, rows ? a->row_pos : nullptr, rows ? a->n_sel : 0};
  call->pr = mmg_pro_dev(l2 ? nullptr : a->pro);
  call->pr2 = mmg_pro_dev(a->mode == MMG_BNBWD_BN2 ? a->pro2 : nullptr);
  call->G = rows && !a->G ? a->y : a->G;   // an empty row list: no row of G is read
  call->what = what;
  return MMG_OK;
}

// msk: 0, or the masked dX store of mmg_linear_bnbwd_masked (1: write, 2: accumulate; validated there)
static int linear_bnbwd_impl(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                             const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, int msk, void* stream) {
  BnBwdCall call;
  const int rc_ = bnbwd_marshal(a, W, dZ, dX, M, N, K, next, wg, &call);
  if (rc_) return rc_;
  const BnBwdDev& bb = call.bb;
  const ProDev &pr = call.pr, &pr2 = call.pr2;
  const float* G = call.G;
  const char* what = call.what;
  hipStream_t st = (hipStream_t)stream;
  switch (a->mode) {
    case MMG_BNBWD_BN: return bnbwd_run<MMG_BNBWD_BN>(G, bb, pr, pr2, W, dX, M, N, K, next, wg, what, st, msk);
    case MMG_BNBWD_L2: return bnbwd_run<MMG_BNBWD_L2>(G, bb, pr, pr2, W, dX, M, N, K, next, wg, what, st, msk);
    case MMG_BNBWD_BN2: return bnbwd_run<MMG_BNBWD_BN2>(G, bb, pr, pr2, W, dX, M, N, K, next, wg, what, st, msk);
    default: return bnbwd_run<MMG_BNBWD_ROWS>(G, bb, pr, pr2, W, dX, M, N, K, next, wg, what, st, msk);
  }
}

extern "C" int mmg_linear_bnbwd(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                                const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, void* stream) {
  return linear_bnbwd_impl(a, W, dZ, dX, M, N, K, next, wg, 0, stream);
}

extern "C" int mmg_linear_bnbwd_rider_supported(int64_t M, int N, int K, int64_t n_sel) {
  // the dense launch: the L2 backward of the 128 x 128 layer; the rider: nothing, or a list the library's own compact call
  // hands to that same kernel (mmg_linear_bnbwd_supported: more than 512 rows)
  if (!(M > 512 && N == 128 && K == 128)) return 0;
  return (n_sel == 0 || (n_sel > 512 && n_sel <= M)) ? 1 : 0;
}

extern "C" int mmg_linear_bnbwd_rider(const mmg_bnbwd_t* b, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                                      const mmg_next_bn_t* next, const mmg_bnbwd_t* a, const float* W_a, float* dZ_a,
                                      float* dX_a, int64_t n_sel, const int64_t* rows, const mmg_next_bn_t* next_a,
                                      void* stream) {
  const char* what = "linear_bnbwd_rider";
  MMG_CHECK_ARG(b, "%s: null descriptor", what);
  MMG_CHECK_ARG(mmg_linear_bnbwd_rider_supported(M, N, K, n_sel),
                "%s: M=%lld N=%d K=%d n_sel=%lld unsupported (M > 512, N = K = 128, n_sel = 0 or 512 < n_sel <= M)", what,
                (long long)M, N, K, (long long)n_sel);
  MMG_CHECK_ARG(b->mode == MMG_BNBWD_L2 && (n_sel == 0 || (a && a->mode == MMG_BNBWD_L2)),
                "%s: both problems are MMG_BNBWD_L2", what);
  const bool stats = next_a != nullptr;
  if (stats)
    MMG_CHECK_ARG(next_a->sums && next_a->mean && next_a->rstd && !next_a->accumulate,
                  "%s: statistics of the listed rows: null field, or accumulate", what);
  hipStream_t st = (hipStream_t)stream;
  if (n_sel == 0) {             // the dense call alone (+ the statistics of an empty list: zeros)
    const int rc = mmg_linear_bnbwd(b, W, dZ, dX, M, N, K, next, nullptr, stream);
    if (rc || !stats) return rc;
    return mmg_bn_bwd_stats_rows(nullptr, nullptr, nullptr, 0, next_a->pro, next_a->mean, next_a->rstd, next_a->sums, N,
                                 next_a->ws, next_a->ws_bytes, stream);
  }
  MMG_CHECK_ARG(W_a == W, "%s: the rider runs on the dense launch's W", what);
  MMG_CHECK_ARG(dZ && dZ_a && dX_a, "%s: null buffer", what);
  MMG_CHECK_ARG(b->eps == a->eps, "%s: the two L2 normalisations have different eps", what);
  BnBwdCall cb, ca;
  int rc = bnbwd_marshal(b, W, dZ, dX, M, N, K, next, nullptr, &cb);
  if (rc) return rc;
  rc = bnbwd_marshal(a, W, dZ_a, dX_a, n_sel, N, K, nullptr, nullptr, &ca);
  if (rc) return rc;
  if (stats)
    MMG_CHECK_ARG(next_a->y && rows && next_a->ws && next_a->ws_bytes >= mmg_bn_bwd_stats_rows_ws_bytes(N),
                  "%s: statistics of the listed rows: null buffer or workspace too small", what);
  if (stats && next && next->ws) {
    // both sets of partial rows stay in their workspaces until the one launch that sums them
    const uintptr_t a0 = (uintptr_t)next_a->ws, a1 = a0 + next_a->ws_bytes, b0 = (uintptr_t)next->ws, b1 = b0 + next->ws_bytes;
    MMG_CHECK_ARG(a1 <= b0 || b1 <= a0, "%s: the statistics of the listed rows share the next BatchNorm's workspace", what);
  }
  {
    // the rider's outputs against the dense launch's outputs and everything either problem reads
    struct Span { const void* p; size_t n; };
    const size_t mk = (size_t)M * K * 4, sk = (size_t)n_sel * K * 4;
    const Span outs[2] = {{dZ_a, sk}, {dX_a, (size_t)n_sel * N * 4}};
    const Span others[9] = {{b->G, mk}, {b->y, mk}, {b->rnorm, (size_t)M * 4}, {dZ, mk}, {dX, (size_t)M * N * 4},
                            {a->G, sk}, {a->y, sk}, {a->rnorm, (size_t)n_sel * 4}, {W, (size_t)N * K * 4}};
    auto overlap = [](const Span& x, const Span& c) {
      const uintptr_t x0 = (uintptr_t)x.p, c0 = (uintptr_t)c.p;
      return x0 < c0 + c.n && c0 < x0 + x.n;
    };
    bool alias = overlap(outs[0], outs[1]);
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 9; ++j) alias = alias || overlap(outs[i], others[j]);
    MMG_CHECK_ARG(!alias, "%s: a rider output aliases a tensor of the launch", what);
  }
  const BnRiderDev rd{ca.G, ca.bb, dX_a, n_sel};
  // the dense launch as bnbwd_run picks it: the NBN instance where the next BatchNorm's statistics fit its epilogue
  const bool nbn = next && mmg_next_bn_fusable(next);
  NextBnDev nb = next_bn_none();
  double* partial = nullptr;
  if (nbn) {
    rc = mmg_next_bn_dev(next, M, N, what, &nb, &partial);
    if (rc) return rc;
    rc = launch_bnbwd_x6_rider<true>(cb.G, cb.bb, W, dX, M, st, nb, partial, rd);
  } else {
    rc = launch_bnbwd_x6_rider<false>(cb.G, cb.bb, W, dX, M, st, nb, nullptr, rd);
  }
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  // behind it: the statistics of the listed rows up to their partial rows, then ONE launch sums both passes' partial rows
  MmgPartialJob ja{nullptr, nullptr, 0, 0, nullptr};
  if (stats) {
    rc = mmg_bn_bwd_stats_rows_partial(dX_a, next_a->y, rows, n_sel, next_a->pro, next_a->mean, next_a->rstd,
                                       next_a->sums, N, next_a->ws, next_a->ws_bytes, stream, &ja);
    if (rc) return rc;
  }
  if (nbn && ja.partial) {
    const MmgPartialJob jb{partial, next->sums, 2 * N, (int)bnbwd_x6_rows(M, K), next->accumulate ? next->sums : nullptr};
    return mmg_partial_sum_jobs(&jb, &ja, stream);
  }
  if (nbn) rc = mmg_next_bn_finish(next, partial, N, (int)bnbwd_x6_rows(M, K), st);
  else if (next) rc = mmg_next_bn_fallback(dX, M, N, next, what, st);
  if (rc || !ja.partial) return rc;
  return mmg_partial_sum(ja.partial, ja.out, ja.n, ja.n_rows, stream);
}

extern "C" int mmg_linear_bnbwd_masked_supported(int mode, int64_t M, int N, int K, int with_wgrad) {
  return (mode == MMG_BNBWD_BN || mode == MMG_BNBWD_ROWS) && with_wgrad && mmg_linear_bnbwd_supported(mode, M, N, K, 1) ? 1 : 0;
}

// what mmg_linear_bnbwd_masked refuses before it marshals the call
static int bnbwd_masked_check(const mmg_bnbwd_t* a, int64_t M, int N, int K, const mmg_prologue_t* mask,
                              const mmg_bnbwd_wgrad_t* wg, const char* what) {
  MMG_CHECK_ARG(a, "%s: null descriptor", what);
  MMG_CHECK_ARG(mmg_linear_bnbwd_masked_supported(a->mode, M, N, K, wg != nullptr), "%s: mode %d M=%lld N=%d K=%d%s unsupported",
                what, a->mode, (long long)M, N, K, wg ? "" : " without a weight gradient");
  MMG_CHECK_ARG(mask, "%s: null mask", what);
  // the keep bits are those the X stagers hash for the weight gradient: the mask IS the dropout of wg->pro
  const mmg_prologue_t* xp = wg->pro;
  const float xp_p = xp ? xp->drop_p : 0.f;
  MMG_CHECK_ARG(mask->drop_p == xp_p &&
                    (!(xp_p > 0.f) || (mask->seed_ptr == xp->seed_ptr && (mask->seed_ptr || mask->seed == xp->seed) &&
                                       mask->site == xp->site && mask->row_offset == xp->row_offset)),
                "%s: the mask is not the dropout of the X prologue", what);
  return MMG_OK;
}

extern "C" int mmg_linear_bnbwd_masked(const mmg_bnbwd_t* a, const float* W, float* dZ, float* dX, int64_t M, int N, int K,
                                       const mmg_prologue_t* mask, int accumulate, const mmg_bnbwd_wgrad_t* wg, void* stream) {
  const int rc = bnbwd_masked_check(a, M, N, K, mask, wg, "linear_bnbwd_masked");
  if (rc) return rc;
  return linear_bnbwd_impl(a, W, dZ, dX, M, N, K, nullptr, wg, accumulate ? 2 : 1, stream);
}

extern "C" int mmg_linear_bnbwd_dual_supported(int64_t M, int N, int K) {
  return mmg_linear_bnbwd_masked_supported(MMG_BNBWD_BN, M, N, K, 1) && mmg_linear_bnbwd_masked_supported(MMG_BNBWD_ROWS, M, N, K, 1);
}

extern "C" int mmg_linear_bnbwd_dual(const mmg_bnbwd_t* b, const mmg_bnbwd_wgrad_t* wg_b, const mmg_bnbwd_t* a,
                                     const mmg_bnbwd_wgrad_t* wg_a, const float* W, float* dZ_b, float* dZ_a, float* dX,
                                     int64_t M, int N, int K, void* stream) {
  const char* what = "linear_bnbwd_dual";
  MMG_CHECK_ARG(b && a && wg_b && wg_a, "%s: null descriptor", what);
  MMG_CHECK_ARG(b->mode == MMG_BNBWD_BN && a->mode == MMG_BNBWD_ROWS, "%s: modes (%d, %d), not (BN, ROWS)", what, b->mode, a->mode);
  MMG_CHECK_ARG(mmg_linear_bnbwd_dual_supported(M, N, K), "%s: M=%lld N=%d K=%d unsupported", what, (long long)M, N, K);
  // each pass masks dX with the dropout of its own X prologue, as in  masked(b, ..., wg_b->pro, 0, wg_b)  and
  // masked(a, ..., wg_a->pro, 1, wg_a); the passes stage ONE X tile, so their X prologues may differ in the dropout site only
  static const mmg_prologue_t no_pro = {};
  const mmg_prologue_t *xb = wg_b->pro ? wg_b->pro : &no_pro, *xa = wg_a->pro ? wg_a->pro : &no_pro;
  int rc = bnbwd_masked_check(b, M, N, K, xb, wg_b, what);
  if (!rc) rc = bnbwd_masked_check(a, M, N, K, xa, wg_a, what);
  if (rc) return rc;
  MMG_CHECK_ARG(wg_b->X == wg_a->X, "%s: the passes read different X", what);
  MMG_CHECK_ARG(wg_b->ws != wg_a->ws, "%s: the passes share a slab workspace", what);
  MMG_CHECK_ARG(xb->scale == xa->scale && xb->shift == xa->shift && xb->relu == xa->relu && xb->drop_p == xa->drop_p &&
                    xb->seed_ptr == xa->seed_ptr && (xb->seed_ptr || xb->seed == xa->seed) && xb->row_offset == xa->row_offset,
                "%s: the X prologues differ in more than the dropout site", what);
  BnBwdCall cb, ca;
  rc = bnbwd_marshal(b, W, dZ_b, dX, M, N, K, nullptr, wg_b, &cb);
  if (!rc) rc = bnbwd_marshal(a, W, dZ_a, dX, M, N, K, nullptr, wg_a, &ca);
  BnWgDev wb, wa;
  if (!rc) rc = bnbwd_wgrad_prepare(wg_b, M, what, &wb);
  if (!rc) rc = bnbwd_wgrad_prepare(wg_a, M, what, &wa);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  rc = launch_bnbwd_fw_dual(cb.G, cb.bb, cb.pr, wb, ca.G, ca.bb, ca.pr, wa, W, dX, M, st);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  rc = bnbwd_wgrad_finish(wg_b, wb, M, what, st);
  return rc ? rc : bnbwd_wgrad_finish(wg_a, wa, M, what, st);
}

extern "C" size_t mmg_linear_wgrad_ws_bytes(int64_t M, int N, int K) {
  if (M < 0 || N <= 0 || K <= 0 || N % 64 || K % 64) return 0;
  WgradPlan p = plan_wgrad(M, N, K);
  return (size_t)p.n_split * ((size_t)N * K + N) * 4 + 256;       // + N: the optional bias sums behind every slab
}

static int linear_wgrad_impl(const float* dY, const float* X, const mmg_prologue_t* pro, float* dW, float* dbias,
                             int64_t M, int N, int K, int accumulate, void* ws, size_t ws_bytes, void* stream,
                             mmg_wgrad_reduce_t* job) {
  if (job) { job->slab = nullptr; job->n4 = 0; job->n_split = 0; job->dW = dW; job->dbias = dbias; job->nk4 = (int64_t)N * K / 4; job->accumulate = accumulate; }
  MMG_CHECK_ARG(M >= 0 && N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0, "linear_wgrad: N=%d K=%d must be multiples of 64", N, K);
  MMG_CHECK_ARG(dW, "linear_wgrad: dW is null");
  hipStream_t st = (hipStream_t)stream;
  if (M == 0) {
    if (!accumulate) {
      MMG_CHECK_HIP(mmg_zero_async(dW, (size_t)N * K * 4, st), "linear_wgrad(memset)");
      if (dbias) MMG_CHECK_HIP(mmg_zero_async(dbias, (size_t)N * 4, st), "linear_wgrad(memset)");
    }
    return MMG_OK;
  }
  MMG_CHECK_ARG(dY && X && ws, "linear_wgrad: null buffer");
  MMG_CHECK_ARG(!pro || pro->relu == MMG_ACT_NONE || pro->relu == MMG_ACT_RELU, "linear_wgrad: the prologue takes relu only");
  const size_t need = mmg_linear_wgrad_ws_bytes(M, N, K);
  MMG_CHECK_WS("linear_wgrad", need);
  WgradPlan p = plan_wgrad(M, N, K);
  float* slab = MmgCarver(ws).take<float>((need - 256) / sizeof(float));
  const ProDev pr = mmg_pro_dev(pro);
  dim3 grid((unsigned)p.n_tiles, (unsigned)p.n_split);
  const int direct = p.n_split == 1 ? (accumulate ? 2 : 1) : 0;     // small M: no slab, no reduce launch
  float* target = direct ? dW : slab;
  const int64_t stride = (int64_t)N * K + (dbias ? N : 0);
  {
    // eight waves (two per SIMD: one stages while the other multiplies) wherever the tile has 8 sub-tiles
    const int64_t rps = p.rows_per_split;
    // role-specialised kernel for the plain 128 x 128 case; with a prologue the X stagers would also carry the dropout
    // hashes and the symmetric kernel is faster (53 vs 64 us)
    const bool has_pro = pr.scale || pr.relu || pr.p > 0.f;
    int rc = 0;
    if (p.TN == 128 && p.TK == 128 && !has_pro) rc = launch_wgrad_ws(grid, st, dY, X, target, M, N, K, direct, stride, dbias);
    else if (p.TN == 128 && p.TK == 128) rc = launch_wgrad_x6<128, 128, 4, 2>(grid, st, dY, X, pr, target, M, N, K, rps, direct, stride, dbias);
    else if (p.TN == 128) rc = launch_wgrad_x6<128, 64, 4, 2>(grid, st, dY, X, pr, target, M, N, K, rps, direct, stride, dbias);
    else if (p.TK == 128) rc = launch_wgrad_x6<64, 128, 2, 4>(grid, st, dY, X, pr, target, M, N, K, rps, direct, stride, dbias);
    else rc = launch_wgrad_x6<64, 64, 2, 2>(grid, st, dY, X, pr, target, M, N, K, rps, direct, stride, dbias);
    if (rc) return rc;
  }
  if (!direct) {
    if (job) {                      // the caller sums the slabs later, together with those of other layers
      job->slab = slab; job->n4 = stride / 4; job->n_split = p.n_split;
    } else {
      MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD_REDUCE, M, N, K, 0, (mmg_k_reduce_slabs<EpiStore>),
                 dim3((unsigned)((stride / 4 + 15) / 16)), dim3(256), 0, st, slab, stride / 4, p.n_split,
                 EpiStore{dW, accumulate, dbias, (int64_t)N * K / 4});
    }
  }
  MMG_CHECK_LAUNCH("linear_wgrad");
  return MMG_OK;
}

extern "C" int mmg_linear_wgrad(const float* dY, const float* X, const mmg_prologue_t* pro, float* dW, float* dbias,
                                int64_t M, int N, int K, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return linear_wgrad_impl(dY, X, pro, dW, dbias, M, N, K, accumulate, ws, ws_bytes, stream, nullptr);
}

extern "C" int mmg_linear_wgrad_is_direct(int64_t M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 64 || K % 64) return 1;
  return plan_wgrad(M, N, K).n_split == 1 ? 1 : 0;
}

extern "C" int mmg_linear_wgrad_deferred(const float* dY, const float* X, const mmg_prologue_t* pro, float* dW, float* dbias,
                                         int64_t M, int N, int K, int accumulate, void* ws, size_t ws_bytes, void* stream,
                                         mmg_wgrad_reduce_t* job) {
  MMG_CHECK_ARG(job, "linear_wgrad_deferred: job is null");
  return linear_wgrad_impl(dY, X, pro, dW, dbias, M, N, K, accumulate, ws, ws_bytes, stream, job);
}

extern "C" int mmg_linear_dgrad_wgrad_supported(int64_t M, int N, int K, float drop_p) {
  return (M > 512 && N == 128 && K == 64 && !(drop_p > 0.f)) ? 1 : 0;
}

extern "C" size_t mmg_linear_dgrad_wgrad_ws_bytes(int64_t M, int N, int K) {
  return mmg_linear_wgrad_ws_bytes(M, K, N);            // the slabs of the separate weight gradient of dY [M, K], X [M, N]
}

extern "C" int mmg_linear_dgrad_wgrad(const float* dY, const float* W, float* dX, int64_t M, int N, int K,
                                      const mmg_next_bn_t* next, const mmg_bnbwd_wgrad_t* wg, void* stream) {
  const char* what = "linear_dgrad_wgrad";
  MMG_CHECK_ARG(wg, "%s: null weight-gradient descriptor", what);
  mmg_wgrad_reduce_t* job = wg->job;
  if (job) { job->slab = nullptr; job->n4 = 0; job->n_split = 0; job->dW = wg->dW; job->dbias = nullptr; job->nk4 = (int64_t)K * N / 4; job->accumulate = wg->accumulate; }
  float drop_p = wg->pro ? wg->pro->drop_p : 0.f;
  if (next && next->pro && next->pro->drop_p > drop_p) drop_p = next->pro->drop_p;
  MMG_CHECK_ARG(mmg_linear_dgrad_wgrad_supported(M, N, K, drop_p), "%s: M=%lld N=%d K=%d drop_p=%g unsupported (M > 512, N = 128, K = 64, no dropout)",
                what, (long long)M, N, K, (double)drop_p);
  MMG_CHECK_ARG(dY && W && dX && wg->X && wg->dW && wg->ws, "%s: null buffer", what);
  MMG_CHECK_ARG(!wg->dbias, "%s: the layer's bias gradient comes from the lab side: dbias must be NULL", what);
  MMG_CHECK_ARG(!wg->pro || wg->pro->relu == MMG_ACT_NONE || wg->pro->relu == MMG_ACT_RELU, "%s: the X prologue takes relu only", what);
  MMG_CHECK_ARG(!wg->pro || !wg->pro->scale || wg->pro->shift, "%s: X prologue: scale without shift", what);
  const ProDev xpr = mmg_pro_dev(wg->pro);
  NextBnDev nb = next_bn_none();
  double* partial = nullptr;
  if (next) {
    MMG_CHECK_ARG(next->y == wg->X, "%s: the next BatchNorm's y must be the layer input wg->X", what);
    MMG_CHECK_ARG(next->pro && mmg_next_bn_fusable(next), "%s: the next BatchNorm takes relu only", what);
    MMG_CHECK_ARG(next->pro->scale == xpr.scale && next->pro->shift == xpr.shift && next->pro->relu == xpr.relu,
                  "%s: the X prologue and the next BatchNorm's prologue must agree", what);
    const int rc = mmg_next_bn_dev(next, M, N, what, &nb, &partial);
    if (rc) return rc;
  }
  void* const ws = wg->ws;
  const size_t ws_bytes = wg->ws_bytes, need = mmg_linear_dgrad_wgrad_ws_bytes(M, N, K);
  MMG_CHECK_WS(what, need);
  float* slab = MmgCarver(ws).take<float>((need - 256) / sizeof(float));
  const int64_t stride = (int64_t)K * N;
  const int n_split = plan_wgrad(M, K, N).n_split;
  const DgWgDev wd{wg->X, xpr, slab, stride};
  const bool has_pro = xpr.scale || xpr.relu;
  hipStream_t st = (hipStream_t)stream;
  int rc = next ? launch_dgrad_wgrad<true>(dY, W, dX, M, nb, partial, wd, n_split, has_pro, st)
                : launch_dgrad_wgrad<false>(dY, W, dX, M, nb, nullptr, wd, n_split, has_pro, st);
  if (rc) return rc;
  MMG_CHECK_LAUNCH(what);
  if (next) {
    rc = mmg_next_bn_finish(next, partial, N, n_split, st);
    if (rc) return rc;
  }
  if (job) {                        // the caller sums the slabs later, together with those of other layers
    job->slab = slab; job->n4 = stride / 4; job->n_split = n_split;
  } else {                          // the launch of mmg_linear_wgrad(dY, X, ., dW, NULL, M, K, N, ...): the same sum, the same probe row
    MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD_REDUCE, M, K, N, 0, (mmg_k_reduce_slabs<EpiStore>),
               dim3((unsigned)((stride / 4 + 15) / 16)), dim3(256), 0, st, slab, stride / 4, n_split,
               EpiStore{wg->dW, wg->accumulate, nullptr, (int64_t)K * N / 4});
    MMG_CHECK_LAUNCH(what);
  }
  return MMG_OK;
}

namespace {
struct WgradReduceTable { mmg_wgrad_reduce_t j[MMG_WGRAD_REDUCE_MAX]; };
// the slab sums of several weight gradients in ONE launch: blockIdx.y = job, the body of mmg_k_reduce_slabs<EpiStore>
__global__ __launch_bounds__(256) void k_wgrad_reduce_group(WgradReduceTable tb) {
  __shared__ f32x4 part[16][16];
  const mmg_wgrad_reduce_t jb = tb.j[blockIdx.y];
  const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t i4 = (int64_t)blockIdx.x * 16 + e;
  if ((int64_t)blockIdx.x * 16 >= jb.n4) return;               // (uniform per block)
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (i4 < jb.n4) {
    const f32x4* base = reinterpret_cast<const f32x4*>(jb.slab) + i4;
    int sidx = g;
    for (; sidx + 7 * 16 < jb.n_split; sidx += 8 * 16) {
      f32x4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(sidx + u * 16) * jb.n4];
#pragma unroll
      for (int u = 0; u < 8; ++u) acc += v[u];
    }
    for (; sidx < jb.n_split; sidx += 16) acc += base[(size_t)sidx * jb.n4];
  }
  part[g][e] = acc;
  __syncthreads();
  if (g == 0 && i4 < jb.n4) {
    f32x4 t = part[0][e];
#pragma unroll
    for (int q = 1; q < 16; ++q) t += part[q][e];
    EpiStore{jb.dW, jb.accumulate, jb.dbias, jb.nk4}(i4, t);
  }
}
}  // namespace

extern "C" int mmg_wgrad_reduce_group(const mmg_wgrad_reduce_t* jobs, int n_jobs, void* stream) {
  MMG_CHECK_ARG(jobs && n_jobs >= 1 && n_jobs <= MMG_WGRAD_REDUCE_MAX, "wgrad_reduce_group: 1..%d jobs", MMG_WGRAD_REDUCE_MAX);
  WgradReduceTable tb;
  int64_t max_n4 = 0;
  int n = 0;
  for (int j = 0; j < n_jobs; ++j) {
    if (!jobs[j].slab) continue;                                // (a small-M launch wrote its gradient directly)
    MMG_CHECK_ARG(jobs[j].dW && jobs[j].n4 > 0 && jobs[j].n_split > 0, "wgrad_reduce_group: bad job %d", j);
    for (int q = 0; q < n; ++q)
      MMG_CHECK_ARG(tb.j[q].dW != jobs[j].dW, "wgrad_reduce_group: two jobs of one launch write the same gradient (job %d)", j);
    tb.j[n++] = jobs[j];
    if (jobs[j].n4 > max_n4) max_n4 = jobs[j].n4;
  }
  if (n == 0) return MMG_OK;
  MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD_REDUCE, 0, 0, 0, 0, (k_wgrad_reduce_group), dim3((unsigned)((max_n4 + 15) / 16), (unsigned)n),
             dim3(256), 0, (hipStream_t)stream, tb);
  MMG_CHECK_LAUNCH("wgrad_reduce_group");
  return MMG_OK;
}
