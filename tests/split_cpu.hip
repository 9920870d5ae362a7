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

// ---------------------------------------------------------------------------------- the wave's scale rule (H2Scale, mma.h)
static double uni() { return (double)(next64() >> 11) * (1.0 / 9007199254740992.0); }          // [0, 1)
static double gauss() {                                                                        // Box-Muller
  const double u = 1.0 - uni(), v = uni();
  return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
}
enum { P_NOTHING = 0, P_FIRST = 1, P_LOWER = 2, P_OUTLIER = 3, P_REANCHOR = 4 };

// one block through the header's rule, asked as strip_main_h asks: the first block of the wave, and a block with an element
// (an infinity included) beyond hs.lim.  The path is read off the state: the rule itself returns only "exact or not" and d.
static int h2_step(int b, float m_finite, bool has_inf, H2Scale& hs, int& d) {
  d = 0;
  if (!(b == 0 || has_inf || m_finite > hs.lim)) return P_NOTHING;
  const H2Scale was = hs;
  if (h2_decide_uniform(m_finite, hs, d)) return P_OUTLIER;
  if (!was.seen && hs.seen) return P_FIRST;
  if (hs.e_floor != was.e_floor) return P_REANCHOR;
  return hs.e != was.e ? P_LOWER : P_NOTHING;
}

// One column of a wave, one item per block: block b's 16 values go to item b alone.  f16 pieces by split8_h2 at the rule's
// scale (an outlier block: the three exact bf16 pieces at the unchanged scale), fp32 accumulation piece by piece, the
// accumulators rescaled as the kernel rescales them (2^max(d, -126)) and unscaled by 2^-e_out.  mblk[b] >= max |x| of the
// block: the maximum over the strip's 32 columns that the wave's rule sees.
constexpr int SIM_NB = 24;
struct SimOut { float out[SIM_NB]; int e[SIM_NB], path[SIM_NB], e_floor_of[SIM_NB], e_out; };
static void sim_wave(const float (*x)[16], const float* mblk, SimOut& so) {
  H2Scale hs;
  hs.init();
  float acc[SIM_NB];
  for (int b = 0; b < SIM_NB; ++b) acc[b] = 0.f;
  for (int b = 0; b < SIM_NB; ++b) {
    int d;
    const int path = h2_step(b, mblk[b], false, hs, d);
    if (path == P_OUTLIER) {
      for (int g = 0; g < 2; ++g) {
        float xs[8];
        for (int j = 0; j < 8; ++j) xs[j] = x[b][8 * g + j] * hs.sc;
        bf16x8 p0, p1, p2;
        mmg_split8(xs, p0, p1, p2);              // (the kernel's truncating split is exact as well: checked above)
        for (int j = 0; j < 8; ++j) acc[b] += (float)p0[j];
        for (int j = 0; j < 8; ++j) acc[b] += (float)p1[j];
        for (int j = 0; j < 8; ++j) acc[b] += (float)p2[j];
      }
    } else {
      if (d != 0) {
        const float f = mmg_pow2(d < -126 ? -126 : d);
        for (int t = 0; t < SIM_NB; ++t) acc[t] *= f;
      }
      f16x8 hi[2], lo[2];
      for (int g = 0; g < 2; ++g) split8_h2(&x[b][8 * g], hs.sc, hi[g], lo[g]);
      for (int g = 0; g < 2; ++g)
        for (int j = 0; j < 8; ++j) acc[b] += (float)hi[g][j];
      for (int g = 0; g < 2; ++g)
        for (int j = 0; j < 8; ++j) acc[b] += (float)lo[g][j];
    }
    so.e[b] = hs.e; so.path[b] = path;
  }
  const float un = mmg_pow2(-hs.e);
  for (int b = 0; b < SIM_NB; ++b) so.out[b] = acc[b] * un;
  // the exponent of a term's absolute floor: that of its block, or of a LATER re-anchor of the wave if lower (lowering
  // inside e_floor rescales the accumulators exactly; a re-anchor may push an earlier sum below what fp32 holds)
  so.e_out = hs.e;
  int lowest = 1 << 20;
  for (int b = SIM_NB - 1; b >= 0; --b) {
    so.e_floor_of[b] = so.e[b] < lowest ? so.e[b] : lowest;
    if (so.path[b] == P_REANCHOR && so.e[b] < lowest) lowest = so.e[b];
  }
}

// the two bars of the contract on one simulated wave.  An item is in the window when every term of it is at least 2^-3 in
// units of 2^-e (= 2^-16 of the reference magnitude 2^(13 - e)) or its block went the exact way, AND the wave ends within
// 2^100 of the scale it was summed at (the rescaled sum then keeps every bit in fp32) -> |err| <= 6e-7 mag; every item:
// |err| <= 6e-7 mag + 16 terms * 2^-25 * 2^-e.  whole_profile: 1 = the profile is in-window by its definition (every item is
// held to the first bar), 0 = below the window (the second bar alone), -1 = item by item as above.
struct SimStat { long n_items, bad_in, bad_floor, n_in, paths[5]; double worst_in, worst_all; };
static bool sim_check(const float (*x)[16], const SimOut& so, SimStat& st, int whole_profile) {
  bool all_in = true;
  for (int b = 0; b < SIM_NB; ++b) {
    double ref = 0.0, mag = 0.0, xmin = INFINITY;
    for (int j = 0; j < 16; ++j) {
      ref += (double)x[b][j]; mag += fabs((double)x[b][j]);
      if (fabs((double)x[b][j]) < xmin) xmin = fabs((double)x[b][j]);
    }
    const double err = fabs((double)so.out[b] - ref);
    const bool in = whole_profile >= 0 ? whole_profile == 1
                  : (so.path[b] == P_OUTLIER || mag == 0.0 || xmin >= ldexp(1.0, -3 - so.e[b])) && so.e[b] - so.e_out <= 100;
    ++st.n_items; ++st.paths[so.path[b]];
    if (!std::isfinite(so.out[b]) || (mag == 0.0 && so.out[b] != 0.f)) { ++st.bad_in; ++st.bad_floor; continue; }
    if (!(err <= 6e-7 * mag + 16.0 * ldexp(1.0, -25 - so.e_floor_of[b]))) ++st.bad_floor;
    const double r = mag > 0.0 ? err / mag : 0.0;
    if (r > st.worst_all) st.worst_all = r;
    if (in) {
      ++st.n_in;
      if (!(err <= 6e-7 * mag)) ++st.bad_in;
      if (r > st.worst_in) st.worst_in = r;
    } else all_in = false;
  }
  return all_in;
}

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
  // ---- the scale rule, trajectories: random walks of the block maximum's exponent (steps up to +-150, clamped to the normal
  // range), with all-zero blocks and infinities (with and without finite company) strewn in.  One line per walk: the maxima
  // as bit patterns, the infinity flags, and what the header's rule made of them; tests/h2_ref.py must agree block for block.
  for (int w = 0; w < 600; ++w) {
    const int nb = 8 + (int)(next64() % 40);
    std::vector<uint32_t> mb(nb);
    std::vector<int> inf(nb), es(nb), ps(nb);
    double ex = -120.0 + 240.0 * uni();
    const double span = w % 3 == 0 ? 150.0 : (w % 3 == 1 ? 12.0 : 3.0);
    H2Scale hs;
    hs.init();
    for (int b = 0; b < nb; ++b) {
      ex += span * (2.0 * uni() - 1.0);
      ex = ex < -126.0 ? -126.0 : (ex > 127.0 ? 127.0 : ex);
      float m = ldexpf(1.0f + (float)uni(), (int)floor(ex));
      if (!(m < INFINITY)) m = 3.0e38f;
      const unsigned kind = (unsigned)(next64() % 16);
      if (kind == 0 || kind == 1) m = 0.f;                  // nothing finite and non-zero in the block
      inf[b] = kind == 1 || kind == 2;                      // an infinity alone (1) or beside finite values (2)
      int d;
      ps[b] = h2_step(b, m, inf[b] != 0, hs, d);
      mb[b] = bits_of(m); es[b] = hs.e;
    }
    printf("h2walk");
    for (int b = 0; b < nb; ++b) printf(" %08x:%d:%d:%d", mb[b], inf[b], es[b], ps[b]);
    printf(" out:%d\n", hs.e);
  }

  // ---- the named profiles inside one wave's range (tests/test_scatter_scale_gpu.py runs the same on the device): block b's
  // values are gaussian times 2^prof(b); the wave sees the maximum of 512 such values (3 .. 4.5 standard deviations here).
  // cols14 / cols20: THIS column lies 2^14 / 2^20 below its neighbours, which set the maximum.
  {
    // kind 0: slope a per block; 1: a before block 8, b from it on; 2: b at block 8 alone, else a; 3: zero before block 8,
    // then b; 4: this column 2^a below the strip's maximum.  below: the profile leaves the window (second bar).
    struct Prof { const char* name; int kind; double a, b; bool below; };
    const Prof profs[] = {
      {"flat", 0, 0, 0, false}, {"rise9", 0, 0.4, 0, false}, {"fall14", 0, -0.6, 0, false}, {"step12", 1, 0, 12, false},
      {"step30", 1, 0, 30, false}, {"spike", 2, 0, 60, false}, {"step95", 1, -40, 55, false}, {"zero_head", 3, 0, -40, false},
      {"cols14", 4, -14, 0, false}, {"fall23", 0, -1.0, 0, true}, {"fall46", 0, -2.0, 0, true}, {"cols20", 4, -20, 0, true},
      {"step140", 1, -80, 60, true}};
    for (const Prof& pf : profs) {
      SimStat st;
      memset(&st, 0, sizeof st);
      long waves = 0, waves_with[5] = {0, 0, 0, 0, 0};
      for (int rep = 0; rep < 2000; ++rep) {
        float x[SIM_NB][16], mblk[SIM_NB];
        for (int b = 0; b < SIM_NB; ++b) {
          double p = pf.kind == 0 ? pf.a * b : pf.kind == 1 ? (b < 8 ? pf.a : pf.b) : pf.kind == 2 ? (b == 8 ? pf.b : pf.a)
                   : pf.kind == 3 ? pf.b : 0.0;
          const bool zero = pf.kind == 3 && b < 8;
          float mx = 0.f;
          for (int j = 0; j < 16; ++j) {
            const float v = zero ? 0.f : (float)(gauss() * exp2(p));
            mx = fmaxf(mx, fabsf(v));
            x[b][j] = pf.kind == 4 ? (float)((double)v * exp2(pf.a)) : v;
          }
          mblk[b] = zero ? 0.f : fmaxf(mx, (float)((3.0 + 1.5 * uni()) * exp2(p)));
        }
        SimOut so;
        sim_wave(x, mblk, so);
        sim_check(x, so, st, pf.below ? 0 : 1);
        bool has[5] = {false, false, false, false, false};
        for (int b = 0; b < SIM_NB; ++b) has[so.path[b]] = true;
        for (int k = 0; k < 5; ++k) waves_with[k] += has[k];
        ++waves;
      }
      printf("h2sim_%s waves=%ld items=%ld in_window=%ld bad_in=%ld bad_floor=%ld worst_in=%.6g worst_all=%.6g "
             "w_first=%ld w_lower=%ld w_outlier=%ld w_reanchor=%ld\n", pf.name, waves, st.n_items, st.n_in, st.bad_in,
             st.bad_floor, st.worst_in, st.worst_all, waves_with[P_FIRST], waves_with[P_LOWER], waves_with[P_OUTLIER],
             waves_with[P_REANCHOR]);
    }
  }

  // ---- random walks inside the window: values +-[0.5, 1) * 2^p, p moving by -0.9 .. +0.6 per block, with upward jumps of
  // 2^11 .. 2^45 (outlier blocks) and of 2^100 and more (re-anchor) now and then.  A walk counts as in-window when every item
  // of it is (sim_check); every in-window item must meet 6e-7 of its own magnitude, every item the floor.
  {
    SimStat st;
    memset(&st, 0, sizeof st);
    long walks = 0, walks_in = 0;
    for (int rep = 0; rep < 160000; ++rep) {
      float x[SIM_NB][16], mblk[SIM_NB];
      double p = -110.0 + 150.0 * uni();
      for (int b = 0; b < SIM_NB; ++b) {
        const unsigned kind = (unsigned)(next64() % 64);
        if (b > 0) {
          p += 1.5 * uni() - 0.9;
          if (kind == 0) p += 11.0 + 34.0 * uni();
          if (kind == 1 && p < 0.0) p += 100.0 + 20.0 * uni();
        }
        p = p > 120.0 ? 120.0 : p;
        float mx = 0.f;
        for (int j = 0; j < 16; ++j) {
          const float v = (float)((0.5 + 0.5 * uni()) * exp2(p)) * ((next64() & 1) ? 1.f : -1.f);
          mx = fmaxf(mx, fabsf(v));
          x[b][j] = v;
        }
        mblk[b] = fminf(mx * (float)(1.0 + uni()), 3.0e38f);
      }
      SimOut so;
      sim_wave(x, mblk, so);
      walks_in += sim_check(x, so, st, -1);
      ++walks;
    }
    printf("h2sim_walks walks=%ld walks_in_window=%ld items=%ld in_window=%ld bad_in=%ld bad_floor=%ld worst_in=%.6g "
           "worst_all=%.6g first=%ld lower=%ld outlier=%ld reanchor=%ld\n", walks, walks_in, st.n_items, st.n_in, st.bad_in,
           st.bad_floor, st.worst_in, st.worst_all, st.paths[P_FIRST], st.paths[P_LOWER], st.paths[P_OUTLIER],
           st.paths[P_REANCHOR]);
  }
  return 0;
}
