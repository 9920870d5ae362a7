// Split-precision arithmetic on the gfx950 matrix cores: the one home of the vector types, the fp32 -> bf16 / f16 splits,
// the product sequences, 2^e, the 32 x 32 C-layout row map and the transposing LDS read that gemm.hip, pairs.hip,
// aggregate.hip, small.hip and elementwise.hip share (common.h keeps the ABI, RNG and workspace helpers).
//
// The split and the product sequences are MACROS on purpose: they expand to the statements the kernels used to spell out,
// and the compiler emits the same machine code.  The same split as a __forceinline__ function returning three __bf16
// kept the instruction count but moved the schedules of every kernel that uses it, and the
// kernels are scheduling-sensitive; a function also cannot bind a vector element (q0[j]) by reference.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- vector types: one name per type
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------- fp32 products on the bf16 matrix cores
// An fp32 value is EXACTLY hi + mid + lo with three bf16 pieces (8 significant bits each), so
//     x . w = x1 w1 + (x1 w2 + x2 w1) + (x2 w2 + x1 w3 + x3 w1) + O(2^-24 |x||w|)
// Six v_mfma_f32_32x32x16_bf16 products (each exact, accumulated in fp32) reproduce the fp32 product to within
// its own rounding error at 6/16 of the fp32 matrix time: the dropped terms x2 w3 + x3 w2 + x3 w3 are below
// 3 * 2^-25 |x||w| -- less than the rounding of the fp32 FMA chain they replace.  Where one operand is a 0/1 indicator
// (exact in bf16) three products do: Ind . x = Ind x1 + Ind x2 + Ind x3, every product exact.
// (tests/test_split_cpu.py runs these statements on the host over random bit patterns.)
#define MMG_SPLIT3(v, hi, mid, lo)                   \
  do {                                               \
    const __bf16 a__ = (__bf16)(v);                  \
    const float r1__ = (v) - (float)a__;             \
    const __bf16 b__ = (__bf16)r1__;                 \
    (hi) = a__; (mid) = b__; (lo) = (__bf16)(r1__ - (float)b__); \
  } while (0)

__host__ __device__ __forceinline__ void mmg_split8(const float* v, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
#pragma unroll
  for (int j = 0; j < 8; ++j) MMG_SPLIT3(v[j], p0[j], p1[j], p2[j]);
}

// the three bf16 pieces of 8 values by TRUNCATION (upper 16 bits of a, of a - hi, of a - hi - mid: each exactly a bf16,
// their sum is a): v_perm / v_and / v_sub only.  Element j of a piece sits in half j & 1 of dword j / 2 = the MFMA
// operand order.
__device__ __forceinline__ void split8_tr(const float* v, u32x4& p0, u32x4& p1, u32x4& p2) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const unsigned a0 = __builtin_bit_cast(unsigned, v[2 * j]), a1 = __builtin_bit_cast(unsigned, v[2 * j + 1]);
    p0[j] = __builtin_amdgcn_perm(a1, a0, 0x07060302u);
    const float r0 = v[2 * j] - __builtin_bit_cast(float, a0 & 0xFFFF0000u);
    const float r1 = v[2 * j + 1] - __builtin_bit_cast(float, a1 & 0xFFFF0000u);
    const unsigned b0 = __builtin_bit_cast(unsigned, r0), b1 = __builtin_bit_cast(unsigned, r1);
    p1[j] = __builtin_amdgcn_perm(b1, b0, 0x07060302u);
    const float s0 = r0 - __builtin_bit_cast(float, b0 & 0xFFFF0000u);
    const float s1 = r1 - __builtin_bit_cast(float, b1 & 0xFFFF0000u);
    p2[j] = __builtin_amdgcn_perm(__builtin_bit_cast(unsigned, s1), __builtin_bit_cast(unsigned, s0), 0x07060302u);
  }
}

// (the scatter kernels' split since round 3: 44 plain vector instructions per 8 values instead of 56 with conversions;
//  same-box A/B 44.9 -> 44.4 us without, 55.7 -> 54.4 us with a rowscale)
__device__ inline void split8x(const float* v, bf16x8& p0, bf16x8& p1, bf16x8& p2) {
  u32x4 q0, q1, q2;
  split8_tr(v, q0, q1, q2);
  p0 = __builtin_bit_cast(bf16x8, q0); p1 = __builtin_bit_cast(bf16x8, q1); p2 = __builtin_bit_cast(bf16x8, q2);
}

// ---- two f16 pieces of X = x * 2^e: hi = f16(X), lo = f16(X - hi): 22 significant bits, relative error <= 2^-22 of X
// while 2^-3 <= |X| < 65504; below that the residual is an f16 denormal (absolute error 2^-25 in units of X).  Who picks e,
// and how: H2Scale / h2_decide_uniform below (used by strip_main_h, aggregate.hip).
__host__ __device__ __forceinline__ void split8_h2(const float* v, float scale, f16x8& p0, f16x8& p1) {
  u32x4 q0, q1;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x2 a = {v[2 * j] * scale, v[2 * j + 1] * scale};
    const f16x2 hh = __builtin_convertvector(a, f16x2);
    const f32x2 r = {a[0] - (float)hh[0], a[1] - (float)hh[1]};
    const f16x2 ll = __builtin_convertvector(r, f16x2);
    q0[j] = __builtin_bit_cast(unsigned, hh); q1[j] = __builtin_bit_cast(unsigned, ll);
  }
  p0 = __builtin_bit_cast(f16x8, q0); p1 = __builtin_bit_cast(f16x8, q1);
}

// ---- the product sequences: `acc` += A . B over pieces a0 (hi), a1, a2 (lo) and b0, b1, b2, small terms first.
// The six terms come in TWO orders, and fp32 accumulation makes the order part of the result's bits (the bit-for-bit
// tests hold each kernel to its own):
//   ALO, A's low piece first: (a2,b0) (a0,b2) (a1,b1) (a1,b0) (a0,b1) (a0,b0)
//        gemm.hip: k_linear_fwd_x6, k_linear_bnbwd_x6 (dX), k_linear_wgrad_x6 -- and, table-driven with the same order,
//        k_linear_wgrad_ws and the fused weight gradient of k_linear_bnbwd_x6;
//        pairs.hip: k_pair_fwd_mfma and k_pair_dense_fwd (A = the W2 pieces, B = the pieces of h1).
//   BLO, B's low piece first: (a0,b2) (a2,b0) (a1,b1) (a0,b1) (a1,b0) (a0,b0)
//        pairs.hip: k_pair_bwd_duo6 (H2pre recomputed, dW2, dH1).  Its recomputed H2pre has A = the pieces of h1 and
//        B = the W2 pieces -- the forward's operands swapped -- so BLO there adds the forward's terms in the forward's
//        order, and the recomputed pre-activation is the forward's bit for bit.
#define MMG_X6_ALO(acc, a0, a1, a2, b0, b1, b2)                               \
  do {                                                                        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);      \
  } while (0)
#define MMG_X6_BLO(acc, a0, a1, a2, b0, b1, b2)                               \
  do {                                                                        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, acc, 0, 0, 0);      \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, acc, 0, 0, 0);      \
  } while (0)
// indicator (exact in bf16) x the three pieces, largest first: aggregate.hip's gather and scatter kernels
#define MMG_X3(acc, a, p0, p1, p2)                                            \
  do {                                                                        \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, p0, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, p1, acc, 0, 0, 0);       \
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, p2, acc, 0, 0, 0);       \
  } while (0)

// 2^e from the exponent field, -126 <= e <= 127: integer arithmetic only, so a wave-uniform e stays on the scalar unit
__host__ __device__ __forceinline__ float mmg_pow2(int e) { return __builtin_bit_cast(float, (unsigned)(e + 127) << 23); }

// ---- the scale of the two f16 pieces: block floating point over ONE WAVE's row range of a 32-column strip (the forward
// scatter, strip_main_h in aggregate.hip).  The rule is host + device code so that tests/split_cpu.hip runs THESE statements
// on the host against the numpy restatement tests/h2_ref.py; the wave maximum and the readfirstlane stay in the kernel.
// e: the pieces are those of x * 2^e.  The first block (16 rows x 32 columns) with a finite non-zero value sets e so that its
// largest magnitude lands in [2^12, 2^13) and anchors e_floor = e - 10; from then on a block that does not fit
// (an element beyond 2^15 / 2^e) either lowers e (not below e_floor: the data grew, the accumulators are multiplied by the
// power of two, nothing is lost) or -- an outlier more than ~2^12 above anything seen before -- is multiplied exactly on its own.
// Every term is therefore kept to 2^-22 of itself while it is within [2^-16, 2^2] of the wave's reference magnitude 2^(13 - e)
// (at least 2^-6 of the first block's maximum), exactly if it is an outlier above, and to an absolute 2^-25 * 2^-e below.
constexpr int H2_E_INIT = 120, H2_E_MIN = -110;
struct H2Scale {
  int e, e_floor, seen;
  float sc, lim;                                       // 2^e, 2^(15 - e): wave-uniform
  __host__ __device__ __forceinline__ void set(int en) { e = en; sc = mmg_pow2(en); lim = mmg_pow2(15 - en); }
  __host__ __device__ __forceinline__ void init() { seen = 0; e_floor = H2_E_MIN; set(H2_E_INIT); }
};
constexpr int H2_E_DROP = 10;

// floor(log2 m) + 1 of a finite m > 0
__host__ __device__ __forceinline__ int h2_frexp_exp(float m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_frexp_expf(m);
#else
  int fe;
  (void)frexpf(m, &fe);
  return fe;
#endif
}

// m = the wave's finite magnitude maximum of the block (uniform).  Returns 1: multiply this block exactly (bf16 pieces), scale
// unchanged; 0: split it as f16 pieces at the (possibly lowered) scale after multiplying the accumulators by 2^d.
// The kernel asks only for a block with an element beyond hs.lim (an infinity included) and for the first block of the wave.
__host__ __device__ __forceinline__ int h2_decide_uniform(float m, H2Scale& hs, int& d) {
  d = 0;
  if (!(m > 0.f)) return 0;                            // nothing finite and non-zero: the block cannot move the scale
  const int fe = h2_frexp_exp(m);
  int en = 13 - fe;
  en = en < H2_E_MIN ? H2_E_MIN : en;
  en = en > hs.e ? hs.e : en;
  if (!hs.seen) { hs.seen = 1; hs.e_floor = en - H2_E_DROP; hs.set(en); return 0; }   // (the accumulators are still zero)
  if (en >= hs.e_floor) { d = en - hs.e; hs.set(en); return 0; }
  if (fe + hs.e >= 100) {                              // x * 2^e would leave the fp32 range: re-anchor.  d may reach -230: the
    // kernel multiplies the accumulators by 2^max(d, -126) and later unscales them by 2^-e, so a sum more than 2^126 below the
    // new scale comes out as a SMALL WRONG number, not a rounded one.  It is then more than 2^100 below the absolute floor
    // 2^-25 * 2^-e of the contract: such values are unspecified (within the floor), like anything else below it.
    d = en - hs.e; hs.e_floor = en - H2_E_DROP; hs.set(en); return 0;
  }
  return 1;
}

// C / D layout of the 32 x 32 MFMAs: lane l holds column l & 31; its accumulator register i holds tile row
// mmg_c_row(i) + 4 * (l >> 5)
__host__ __device__ constexpr int mmg_c_row(int i) { return (i & 3) + 8 * (i >> 2); }

// the gfx950 transposing LDS read of an MFMA operand that is contracted over its ROW index (ds_read_b64_tr_b16: a
// 16-lane group fetches 4 rows x 16 columns and each lane receives 4 consecutive rows of ITS column): the 4 + 4 rows at
// p_lo and p_hi of this lane's column
__device__ __forceinline__ bf16x8 mmg_tr_pair(const __bf16* p_lo, const __bf16* p_hi) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p_lo);
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p_hi);
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
