// The launch that finishes the gradients of a step (mmg_grad_finish_group, include/mmgnn.h): the fixed-order slab sums of
// the weight gradients (the body of mmg_k_reduce_slabs / k_wgrad_reduce_group, gemm.hip), a second accumulating series on
// the same gradient, the sums of further contributions (k_vec_sums, optim.hip) and the placement of a sum inside a wider
// matrix -- one job per destination, blockIdx.y = job.  Every element keeps the order of additions the separate launches
// give it, so the results are theirs bit for bit:
//   series s:  part[g] = slab[g] + slab[g + 16] + ... (in turn);  t_s = part[0] + part[1] + ... + part[15]
//   value   :  t_0, or old + t_0 with accumulate;  then + t_1, + t_2, ...;  then + src[0] + src[1] + src[2]
// The job table travels by value and is read at the wave-uniform blockIdx.y only (scalar loads; a lane-indexed read of
// the kernarg segment is a trip over the host link, see k_adam in optim.hip).
#include "common.h"
#include <vector>

namespace {

// one job = one destination, as the kernel reads it (built on the host from the caller's series and sums)
struct GfJob {
  const float* slab[MMG_GRAD_FINISH_SERIES]; int n_split[MMG_GRAD_FINISH_SERIES]; int n_series;
  int64_t n4;                                           // float4s per slab; n_series = 0: ELEMENTS of the dense job
  float* dW; float* dbias; int64_t nk4;                 // dW: where the value is stored
  int accumulate;
  const float* src[4]; int n_src; int ld_src[4];
  int cols; int ld_dst;
};
struct GradFinishTable { GfJob j[MMG_GRAD_FINISH_MAX]; };
static_assert(sizeof(GradFinishTable) <= 4096 - 64, "the job table must fit the kernarg segment");

// element offset of float4 / element `e` of a [., cols] matrix with row stride ld (cols = 0: flat)
__device__ __forceinline__ size_t gf_offset(int64_t e, int cols, int ld) {
  if (cols == 0) return (size_t)e;
  const int64_t r = e / cols;
  return (size_t)(r * ld + (e - r * cols));
}

__global__ __launch_bounds__(256) void k_grad_finish_group(GradFinishTable tb) {
  __shared__ f32x4 part[16][16];
  const GfJob& jb = tb.j[blockIdx.y];
  if (jb.n_series == 0) {                                       // a dense job: k_vec_sums' loop over n4 ELEMENTS
    const int64_t n = jb.n4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
      float s = jb.src[0][gf_offset(i, jb.cols, jb.ld_src[0])];
      for (int q = 1; q < jb.n_src; ++q) s += jb.src[q][gf_offset(i, jb.cols, jb.ld_src[q])];       // fixed order
      jb.dW[gf_offset(i, jb.cols, jb.ld_dst)] = s;
    }
    return;
  }
  const int e = threadIdx.x & 15, g = threadIdx.x >> 4;
  const int64_t i4 = (int64_t)blockIdx.x * 16 + e;
  if ((int64_t)blockIdx.x * 16 >= jb.n4) return;               // (uniform per block)
  const bool live = i4 < jb.n4, in_w = i4 < jb.nk4;
  f32x4* o = nullptr;
  if (g == 0 && live)
    o = in_w ? reinterpret_cast<f32x4*>(jb.dW + gf_offset(i4 * 4, jb.cols, jb.ld_dst))
             : reinterpret_cast<f32x4*>(jb.dbias) + (i4 - jb.nk4);
  f32x4 val = {0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < jb.n_series; ++s) {                      // (uniform per block)
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int n_split = jb.n_split[s];
    if (live) {
      const f32x4* base = reinterpret_cast<const f32x4*>(jb.slab[s]) + i4;
      int sidx = g;
      for (; sidx + 7 * 16 < n_split; sidx += 8 * 16) {
        f32x4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[(size_t)(sidx + u * 16) * jb.n4];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc += v[u];
      }
      for (; sidx < n_split; sidx += 16) acc += base[(size_t)sidx * jb.n4];
    }
    if (s) __syncthreads();                                    // the previous series' partials have been read
    part[g][e] = acc;
    __syncthreads();
    if (o) {
      f32x4 t = part[0][e];
#pragma unroll
      for (int q = 1; q < 16; ++q) t += part[q][e];
      if (s == 0) val = jb.accumulate ? (*o + t) : t;
      else val = val + t;
    }
  }
  if (o) {
    if (in_w)
      for (int q = 0; q < jb.n_src; ++q)
        val = val + *reinterpret_cast<const f32x4*>(jb.src[q] + gf_offset(i4 * 4, jb.cols, jb.ld_src[q]));
    *o = val;
  }
}

// what a job writes or reads, as a matrix: `rows` rows of `cols` elements, `ld` apart
struct GfRect { const float* p; int64_t rows, cols, ld; };

static bool gf_overlap(const GfRect& a, const GfRect& b) {
  if (!a.p || !b.p || a.rows <= 0 || b.rows <= 0 || a.cols <= 0 || b.cols <= 0) return false;
  const uintptr_t a0 = (uintptr_t)a.p, a1 = (uintptr_t)(a.p + (a.rows - 1) * a.ld + a.cols);
  const uintptr_t b0 = (uintptr_t)b.p, b1 = (uintptr_t)(b.p + (b.rows - 1) * b.ld + b.cols);
  if (a1 <= b0 || b1 <= a0) return false;
  // inside each other's hull: disjoint only as column slices of one wider matrix (the same row stride, columns apart)
  if (a.rows > 1 && b.rows > 1 && a.ld == b.ld && (a0 - b0) % 4 == 0) {
    const int64_t ld = a.ld;
    int64_t d = ((int64_t)b0 - (int64_t)a0) / 4 % ld;            // column of b's first element in a's frame
    if (d < 0) d += ld;
    if (d >= a.cols && d + b.cols <= ld) return false;
  }
  return true;
}

static GfRect gf_rect(const float* p, int64_t n_elem, int cols, int ld) {
  if (cols > 0) return GfRect{p, n_elem / cols, cols, ld};
  return GfRect{p, 1, n_elem, n_elem};
}

}  // namespace

extern "C" int mmg_grad_finish_group(const mmg_wgrad_reduce_t* series, int n_series, const mmg_sum_job_t* sums, int n_sums,
                                     void* stream) {
  const char* what = "grad_finish_group";
  MMG_CHECK_ARG(n_series >= 0 && n_sums >= 0 && n_series + n_sums >= 1, "%s: no jobs", what);
  MMG_CHECK_ARG((series || n_series == 0) && (sums || n_sums == 0), "%s: null job list", what);
  std::vector<GfJob> jobs;
  std::vector<const float*> unwritten;       // per job: the dW of its series when the value lands elsewhere, else NULL
  jobs.reserve((size_t)n_series + n_sums);
  // (a) the series: one job per dW, later entries of the same dW are further series of it
  for (int i = 0; i < n_series; ++i) {
    const mmg_wgrad_reduce_t& e = series[i];
    MMG_CHECK_ARG(e.dW, "%s: series %d: null destination", what, i);
    MMG_CHECK_ARG(e.slab && e.n_split > 0 && (uintptr_t)e.slab % 16 == 0, "%s: series %d: bad slabs", what, i);
    MMG_CHECK_ARG(e.n4 > 0 && e.n4 < ((int64_t)1 << 40) && e.nk4 >= 0 && e.nk4 <= e.n4, "%s: series %d: bad n4 / nk4", what, i);
    MMG_CHECK_ARG(e.nk4 == e.n4 || e.dbias, "%s: series %d: a bias tail without dbias", what, i);
    GfJob* host = nullptr;
    for (GfJob& b : jobs)
      if (b.dW == e.dW) host = &b;
    if (host) {
      MMG_CHECK_ARG(e.accumulate && host->n4 == e.n4 && host->nk4 == e.nk4 && host->dbias == e.dbias &&
                        host->n_series < MMG_GRAD_FINISH_SERIES,
                    "%s: series %d cannot join the job that writes its dW (it belongs in a later launch)", what, i);
      host->slab[host->n_series] = e.slab; host->n_split[host->n_series] = e.n_split; ++host->n_series;
      continue;
    }
    GfJob b = {};
    b.slab[0] = e.slab; b.n_split[0] = e.n_split; b.n_series = 1;
    b.n4 = e.n4; b.dW = e.dW; b.dbias = e.dbias; b.nk4 = e.nk4; b.accumulate = e.accumulate;
    jobs.push_back(b);
    unwritten.push_back(nullptr);
  }
  const size_t n_slab_jobs = jobs.size();
  std::vector<const float*> key(n_slab_jobs);
  std::vector<bool> consumed(n_slab_jobs, false);
  for (size_t j = 0; j < n_slab_jobs; ++j) key[j] = jobs[j].dW;
  // (b), (c) the sums: behind the series whose dW is their first source, or jobs of their own
  for (int i = 0; i < n_sums; ++i) {
    const mmg_sum_job_t& e = sums[i];
    MMG_CHECK_ARG(e.dst && e.n_src >= 1 && e.n_src <= 4 && e.len >= 0, "%s: sum %d: bad job", what, i);
    for (int q = 0; q < e.n_src; ++q) MMG_CHECK_ARG(e.src[q], "%s: sum %d has a null source", what, i);
    MMG_CHECK_ARG(e.cols >= 0 && (e.cols == 0 || (e.len % e.cols == 0 && e.ld_dst >= e.cols)), "%s: sum %d: bad cols / ld_dst", what, i);
    for (int q = 0; q < e.n_src; ++q) MMG_CHECK_ARG(e.cols == 0 || e.ld_src[q] >= e.cols, "%s: sum %d: ld_src < cols", what, i);
    // the series job whose dW (as its series named it) is this sum's first source; one sum per dW: a second one would
    // read a value that is not stored yet, and is refused below like every job that reads another job's destination
    size_t h = n_slab_jobs;
    for (size_t j = 0; j < n_slab_jobs; ++j)
      if (key[j] == e.src[0]) h = j;
    if (h < n_slab_jobs && !consumed[h] && (int64_t)e.len == jobs[h].nk4 * 4) {
      GfJob& b = jobs[h];
      MMG_CHECK_ARG(!b.accumulate || e.dst == key[h], "%s: sum %d: an accumulating series keeps its dW as the destination", what, i);
      consumed[h] = true;
      if (e.dst != key[h]) unwritten[h] = key[h];
      b.dW = e.dst; b.cols = e.cols; b.ld_dst = e.cols ? e.ld_dst : 0;
      b.n_src = e.n_src - 1;
      for (int q = 1; q < e.n_src; ++q) { b.src[q - 1] = e.src[q]; b.ld_src[q - 1] = e.cols ? e.ld_src[q] : 0; }
      continue;
    }
    GfJob b = {};
    b.n4 = e.len; b.dW = e.dst; b.n_src = e.n_src; b.cols = e.cols; b.ld_dst = e.cols ? e.ld_dst : 0;
    for (int q = 0; q < e.n_src; ++q) { b.src[q] = e.src[q]; b.ld_src[q] = e.cols ? e.ld_src[q] : 0; }
    jobs.push_back(b);
    unwritten.push_back(nullptr);
  }
  const int n_jobs = (int)jobs.size();
  for (int j = 0; j < n_jobs; ++j) {
    const GfJob& b = jobs[j];
    if (b.n_series == 0) continue;
    bool al = (uintptr_t)b.dW % 16 == 0 && (uintptr_t)b.dbias % 16 == 0 && b.cols % 4 == 0 && b.ld_dst % 4 == 0 &&
              (b.cols == 0 || (b.nk4 * 4) % b.cols == 0);
    for (int q = 0; q < b.n_src; ++q) al = al && (uintptr_t)b.src[q] % 16 == 0 && b.ld_src[q] % 4 == 0;
    MMG_CHECK_ARG(al, "%s: job %d: with slabs, addresses, cols and strides are multiples of four elements", what, j);
  }
  // the jobs run concurrently (also across the launches of one call: nothing orders a caller's list): no job may write
  // what another writes or reads, or read a dW that is left unwritten
  for (int j = 0; j < n_jobs; ++j) {
    const GfJob& b = jobs[j];
    const int64_t nw = b.n_series > 0 ? b.nk4 * 4 : b.n4;
    const GfRect dw = gf_rect(b.dW, nw, b.cols, b.ld_dst);
    const GfRect db = b.n_series > 0 && b.nk4 < b.n4 ? GfRect{b.dbias, 1, (b.n4 - b.nk4) * 4, 0} : GfRect{nullptr, 0, 0, 0};
    const GfRect un = unwritten[j] ? GfRect{unwritten[j], 1, nw, nw} : GfRect{nullptr, 0, 0, 0};
    MMG_CHECK_ARG(!gf_overlap(dw, db), "%s: job %d: dW and dbias overlap", what, j);
    for (int i = 0; i < n_jobs; ++i) {
      if (i == j) continue;
      const GfJob& a = jobs[i];
      const int64_t na = a.n_series > 0 ? a.nk4 * 4 : a.n4;
      if (i < j) {
        const GfRect aw = gf_rect(a.dW, na, a.cols, a.ld_dst);
        const GfRect ab = a.n_series > 0 && a.nk4 < a.n4 ? GfRect{a.dbias, 1, (a.n4 - a.nk4) * 4, 0} : GfRect{nullptr, 0, 0, 0};
        MMG_CHECK_ARG(!gf_overlap(dw, aw) && !gf_overlap(dw, ab) && !gf_overlap(db, aw) && !gf_overlap(db, ab),
                      "%s: jobs %d and %d write overlapping destinations", what, i, j);
      }
      for (int q = 0; q < a.n_src; ++q) {
        const GfRect sr = gf_rect(a.src[q], na, a.cols, a.ld_src[q]);
        MMG_CHECK_ARG(!gf_overlap(dw, sr) && !gf_overlap(db, sr) && !gf_overlap(un, sr),
                      "%s: job %d reads the destination of job %d (it belongs in a later launch)", what, i, j);
      }
    }
  }
  for (int j0 = 0; j0 < n_jobs; j0 += MMG_GRAD_FINISH_MAX) {
    GradFinishTable tb;
    const int n = n_jobs - j0 < MMG_GRAD_FINISH_MAX ? n_jobs - j0 : MMG_GRAD_FINISH_MAX;
    int64_t nb = 0;
    for (int j = 0; j < n; ++j) {
      const GfJob& b = tb.j[j] = jobs[j0 + j];
      // slabs: 16 float4 per workgroup; dense: four elements per thread up to 64 workgroups (k_vec_sums' grid)
      int64_t need = b.n_series > 0 ? (b.n4 + 15) / 16 : (b.n4 + 256 * 4 - 1) / (256 * 4);
      if (b.n_series == 0 && need > 64) need = 64;
      if (need > nb) nb = need;
    }
    if (nb == 0) continue;
    MMG_CHECK_ARG(nb <= 0x7FFFFFFF, "%s: too many workgroups", what);
    MMG_LAUNCH(MMG_PROBE_LINEAR_WGRAD_REDUCE, 0, 0, 0, 0, (k_grad_finish_group), dim3((unsigned)nb, (unsigned)n), dim3(256), 0,
               (hipStream_t)stream, tb);
    MMG_CHECK_LAUNCH(what);
  }
  return MMG_OK;
}
