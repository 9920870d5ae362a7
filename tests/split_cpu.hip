// Host-side check of the split arithmetic of multi-modal-gnn_amd/csrc/mma.h (built and run by tests/test_split_cpu.py:
// hipcc --cuda-host-only, no GPU).  Every check prints one line "name key=value ..."; the assertions are in the test.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "../multi-modal-gnn_amd/csrc/mma.h"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next64() {                       // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static float from_bits(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// `draws` random 32-bit patterns, kept where the exponent field lies in [e_lo, e_hi]
static std::vector<float> sample(int draws, int e_lo, int e_hi) {
  std::vector<float> v;
  for (int i = 0; i < draws; ++i) {
    const uint32_t u = (uint32_t)next64();
    const int e = (int)((u >> 23) & 0xFFu);
    if (e >= e_lo && e <= e_hi) v.push_back(from_bits(u));
  }
  return v;
}

// the two orders of MMG_X6_ALO / MMG_X6_BLO on one scalar pair: fp32 sums of the six exact piece products (each product
// of two bf16 pieces has 16 significant bits: exact in fp32, so an fma contraction of a sum changes nothing)
static void pieces(float v, float* p) {
  __bf16 a, b, c;
  MMG_SPLIT3(v, a, b, c);
  p[0] = (float)a; p[1] = (float)b; p[2] = (float)c;
}
static float sum6(const float* a, const float* b, const int (*order)[2]) {
  float acc = 0.f;
  for (int t = 0; t < 6; ++t) acc = acc + a[order[t][0]] * b[order[t][1]];
  return acc;
}
static const int ALO[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};
static const int BLO[6][2] = {{0, 2}, {2, 0}, {1, 1}, {0, 1}, {1, 0}, {0, 0}};

int main() {
  std::vector<float> vals = sample(4000000, 127 - 60, 127 + 60);
  vals.push_back(0.f);
  vals.push_back(-0.f);
  const long n = (long)vals.size();

  // MMG_SPLIT3: hi + mid + lo == v (fp64 adds three fp32 values of this spread exactly); mmg_split8 gives the same pieces
  long bad = 0, bad8 = 0;
  for (long i = 0; i < n; ++i) {
    const float v = vals[i];
    __bf16 hi, mid, lo;
    MMG_SPLIT3(v, hi, mid, lo);
    if ((double)(float)hi + (double)(float)mid + (double)(float)lo != (double)v) ++bad;
  }
  for (long i = 0; i + 8 <= n; i += 8) {
    bf16x8 p0, p1, p2;
    mmg_split8(&vals[i], p0, p1, p2);
    for (int j = 0; j < 8; ++j) {
      __bf16 hi, mid, lo;
      MMG_SPLIT3(vals[i + j], hi, mid, lo);
      if ((float)p0[j] != (float)hi || (float)p1[j] != (float)mid || (float)p2[j] != (float)lo) ++bad8;
    }
  }
  printf("split3 n=%ld failures=%ld\n", n, bad);
  printf("split8 n=%ld failures=%ld\n", n / 8 * 8, bad8);

  // split8_tr's arithmetic, restated (v_perm_b32 has no host form): a piece is the UPPER HALF of a, of a - hi, of
  // a - hi - mid.  Each remainder must already have its low 16 bits clear where it is cut, and the pieces must add up.
  long tr_low = 0, tr_sum = 0;
  for (long i = 0; i < n; ++i) {
    const float v = vals[i];
    const float hi = from_bits(bits_of(v) & 0xFFFF0000u);
    const float r = v - hi;
    const float mid = from_bits(bits_of(r) & 0xFFFF0000u);
    const float s = r - mid;                     // the third piece is the upper half of s
    const float lo = from_bits(bits_of(s) & 0xFFFF0000u);
    if ((bits_of(hi) | bits_of(mid) | bits_of(lo)) & 0xFFFFu) ++tr_low;
    if (bits_of(s) & 0xFFFFu) ++tr_low;          // nothing is cut off the third piece
    if ((double)hi + (double)mid + (double)lo != (double)v) ++tr_sum;
  }
  printf("trunc n=%ld low_bits_set=%ld sum_failures=%ld\n", n, tr_low, tr_sum);

  // split8_h2 on X with 2^-3 <= |X| < 65504: |hi + lo - X| <= 2^-22 |X|, in fp64
  {
    std::vector<float> xs;
    while (xs.size() < 2000000 + 8) {
      const uint32_t u = (uint32_t)next64();
      const int e = (int)((u >> 23) & 0xFFu);
      const float x = from_bits(u);
      if (e >= 124 && e <= 142 && fabsf(x) < 65504.f) xs.push_back(x);
    }
    long nh = 0, badh = 0;
    double worst = 0.0;
    for (size_t i = 0; i + 8 <= xs.size(); i += 8) {
      f16x8 p0, p1;
      split8_h2(&xs[i], 1.0f, p0, p1);
      for (int j = 0; j < 8; ++j) {
        const double X = (double)xs[i + j];
        const double err = fabs((double)(float)p0[j] + (double)(float)p1[j] - X) / fabs(X);
        if (err > worst) worst = err;
        if (!(err <= ldexp(1.0, -22))) ++badh;
        ++nh;
      }
    }
    printf("h2 n=%ld failures=%ld worst=%.17g bound=%.17g\n", nh, badh, worst, ldexp(1.0, -22));
  }

  // mmg_pow2 against ldexpf over the normal range
  {
    int badp = 0;
    for (int e = -126; e <= 127; ++e)
      if (bits_of(mmg_pow2(e)) != bits_of(ldexpf(1.f, e))) ++badp;
    printf("pow2 n=%d failures=%d\n", 127 + 126 + 1, badp);
  }

  // mmg_c_row(i) + 4 h, i in 0..15, h in 0..1: a bijection onto 0..31
  {
    int hit[32] = {0}, outside = 0;
    for (int h = 0; h < 2; ++h)
      for (int i = 0; i < 16; ++i) {
        const int r = mmg_c_row(i) + 4 * h;
        if (r < 0 || r > 31) ++outside; else ++hit[r];
      }
    int once = 0;
    for (int r = 0; r < 32; ++r) once += hit[r] == 1;
    printf("c_row rows_hit_once=%d outside=%d\n", once, outside);
  }

  // the two product orders over consecutive sampled values as (x, w): both within 3 * 2^-24 |x||w| of the fp64 product
  // (exact in fp64), and not the same fp32 bits for every pair
  {
    long np = 0, bad_alo = 0, bad_blo = 0, differ = 0;
    double worst_alo = 0.0, worst_blo = 0.0;
    for (long i = 0; i + 1 < n - 2; i += 2) {      // (the two zeros at the end are left out: no relative error)
      const float x = vals[i], w = vals[i + 1];
      float xp[3], wp[3];
      pieces(x, xp);
      pieces(w, wp);
      const float alo = sum6(xp, wp, ALO), blo = sum6(xp, wp, BLO);
      const double ref = (double)x * (double)w, tol = 3.0 * ldexp(1.0, -24) * fabs(ref);
      const double ea = fabs((double)alo - ref), eb = fabs((double)blo - ref);
      if (!(ea <= tol)) ++bad_alo;
      if (!(eb <= tol)) ++bad_blo;
      if (ea / fabs(ref) > worst_alo) worst_alo = ea / fabs(ref);
      if (eb / fabs(ref) > worst_blo) worst_blo = eb / fabs(ref);
      if (bits_of(alo) != bits_of(blo)) ++differ;
      ++np;
    }
    printf("x6 n=%ld alo_failures=%ld blo_failures=%ld differ=%ld worst_alo=%.17g worst_blo=%.17g bound=%.17g\n", np, bad_alo,
           bad_blo, differ, worst_alo, worst_blo, 3.0 * ldexp(1.0, -24));
  }
  return 0;
}
