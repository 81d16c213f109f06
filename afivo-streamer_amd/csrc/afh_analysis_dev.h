// The reductions behind output_log and output_fld_maxima
// (include/afivo_hip_analysis.h), shared by libafivo_hip.so (ND = 3) and
// libafivo_hip_2d.so (ND = 2): af_tree_max_fc / af_tree_min_fc,
// analysis_zmin_zmax_threshold, analysis_max_var_region, analysis_get_maxima
// (m_af_utils.f90:803-952, src/m_analysis.f90:23-186).
//
// A team of T lanes reduces one leaf: 16 lanes for boxes of at most 16 values
// (four 4^2 boxes per wave), a wave up to 64 values, else the whole workgroup,
// so every box size takes the same kernels. Every reduction is a selection:
// (value, linear index) pairs are folded by a wave butterfly in which the
// lower index wins a tie, the per-leaf results go to scratch in leaf-list
// order, and one workgroup folds them with the lower list position winning.
// No atomics, nothing depends on the order the workgroups run in. Everything
// has internal linkage: both libraries may live in one process.
#pragma once

#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/afivo_hip.h"
#include "afh_common.h"

namespace afh_an {
namespace {

constexpr int AN_NT = 256;

// How the values of one box are addressed: value t of the index range n[0] x
// n[1] x n[2] (first index fastest; n[2] = 1 in 2-D) lies at
// off + i + pitch * (j + pitch * k) of the box's array.
struct Geo {
  int nd;
  int n[3];
  int pitch;
  int off;
  size_t stride;  // doubles per box of the variable's pool
};

// box%cc(1:nc, 1:nc[, 1:nc]) of an array with one ghost layer
inline Geo geo_cc(int nd, int nc, size_t bsz) {
  const int ng = nc + 2;
  Geo g;
  g.nd = nd;
  g.n[0] = g.n[1] = nc;
  g.n[2] = nd == 3 ? nc : 1;
  g.pitch = ng;
  g.off = 1 + ng + (nd == 3 ? ng * ng : 0);
  g.stride = bsz;
  return g;
}

// box%fc(1:nc+dix(1), 1:nc+dix(2)[, 1:nc+dix(3)], dim) with dix(dim) = 1: the
// upper-boundary faces are in the range (box_max_fc); dim 0-based
inline Geo geo_fc(int nd, int nc, size_t fsz, int dim) {
  const int nf = nc + 1;
  Geo g;
  g.nd = nd;
  g.n[0] = g.n[1] = nc;
  g.n[2] = nd == 3 ? nc : 1;
  g.n[dim] = nf;
  g.pitch = nf;
  g.off = dim * (nd == 3 ? nf * nf * nf : nf * nf);
  g.stride = fsz;
  return g;
}

struct Region {
  int on;  // 0: every leaf takes part
  double r0[3], r1[3];
};

__device__ __forceinline__ int geo_at(const Geo &g, int t, int &i, int &j, int &k) {
  i = t % g.n[0];
  j = (t / g.n[0]) % g.n[1];
  k = t / (g.n[0] * g.n[1]);
  return i + g.pitch * (j + g.pitch * k);
}

__device__ __forceinline__ bool better(double b, int ib, double v, int ix, bool is_min) {
  return (is_min ? b < v : b > v) || (b == v && ib < ix);
}

// The best (value, index) pair of a team, left in every lane of it. T = AN_NT:
// the team is the workgroup, and every thread of it must call.
template <int T>
__device__ __forceinline__ void team_best(double &v, int &ix, bool is_min) {
  constexpr int W = T < 64 ? T : 64;
  for (int o = W / 2; o > 0; o >>= 1) {
    const double b = __shfl_xor(v, o, 64);
    const int ib = __shfl_xor(ix, o, 64);
    if (better(b, ib, v, ix, is_min)) v = b, ix = ib;
  }
  if (T > 64) {
    __shared__ double s_v[AN_NT / 64];
    __shared__ int s_i[AN_NT / 64];
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_v[threadIdx.x >> 6] = v, s_i[threadIdx.x >> 6] = ix;
    __syncthreads();
    v = s_v[0], ix = s_i[0];
    for (int w = 1; w < AN_NT / 64; w++)
      if (better(s_v[w], s_i[w], v, ix, is_min)) v = s_v[w], ix = s_i[w];
  }
}

// Per leaf the extremum of the range g and its first position (Fortran's
// maxloc / minloc), as (value, linear index) in part[2 q ..]. With a region
// (box_max_region): a leaf with any(r_min > r1) or any(r_min + nc dr < r0)
// gives (-1e100, -1).
template <int T>
__global__ void __launch_bounds__(AN_NT)
    k_box_best(const double *__restrict__ v, Geo g, const int32_t *__restrict__ ids, int nl,
               int is_min, const afh_box_meta *__restrict__ meta, Region R, int nc,
               double *__restrict__ part) {
  const int lt = threadIdx.x % T;
  const int q = blockIdx.x * (AN_NT / T) + threadIdx.x / T;
  double best = is_min ? HUGE_VAL : -HUGE_VAL;
  int bix = INT_MAX;
  bool in = q < nl;
  if (in && R.on) {
    const afh_box_meta &m = meta[ids[q] - 1];
    for (int d = 0; d < g.nd; d++) {
      const double r_max = m.r_min[d] + nc * m.dr[d];
      if (m.r_min[d] > R.r1[d] || r_max < R.r0[d]) in = false;
    }
  }
  if (in) {
    const double *c = v + (size_t)(ids[q] - 1) * g.stride + g.off;
    const int ntot = g.n[0] * g.n[1] * g.n[2];
    for (int t = lt; t < ntot; t += T) {
      int i, j, k;
      const double x = c[geo_at(g, t, i, j, k)];
      if (is_min ? x < best : x > best) best = x, bix = t;
    }
  }
  team_best<T>(best, bix, is_min != 0);
  if (lt == 0 && q < nl) {
    part[2 * q] = in ? best : -1e100;
    // (no value compared true, a box of NaN: the first position, as maxloc)
    part[2 * q + 1] = in ? (double)(bix == INT_MAX ? 0 : bix) : -1.0;
  }
}

// af_reduction_loc over the per-leaf results: the first leaf in list order
// whose value is strictly better than init takes the result, later equal
// ones do not replace it. out = (value, box id, linear index), or (init, -1,
// -1). One workgroup.
__global__ void __launch_bounds__(AN_NT)
    k_fold_loc(const double *__restrict__ part, const int32_t *__restrict__ ids, int nl,
               int is_min, double init, double *__restrict__ out) {
  double best = is_min ? HUGE_VAL : -HUGE_VAL;
  int bq = INT_MAX;
  for (int q = threadIdx.x; q < nl; q += AN_NT) {
    const double x = part[2 * q];
    if (is_min ? x < best : x > best) best = x, bq = q;
  }
  team_best<AN_NT>(best, bq, is_min != 0);
  if (threadIdx.x == 0) {
    const bool take = bq != INT_MAX && (is_min ? best < init : best > init);
    out[0] = take ? best : init;
    out[1] = take ? (double)ids[bq] : -1.0;
    out[2] = take ? part[2 * bq + 1] : -1.0;
  }
}

// box_minmax_z: per leaf the first plane n along the last dimension with a
// value above the threshold; both entries are that plane's cell centre
// r_min + (n - 0.5) dr (the reference's zmax entry uses the first plane's
// index too), or (1e100, -1e100) without one.
template <int T>
__global__ void __launch_bounds__(AN_NT)
    k_box_zfirst(const double *__restrict__ v, Geo g, const int32_t *__restrict__ ids, int nl,
                 double threshold, const afh_box_meta *__restrict__ meta,
                 double *__restrict__ part) {
  const int lt = threadIdx.x % T;
  const int q = blockIdx.x * (AN_NT / T) + threadIdx.x / T;
  double first = HUGE_VAL;  // plane index, 1-based
  int none = 0;
  if (q < nl) {
    const double *c = v + (size_t)(ids[q] - 1) * g.stride + g.off;
    const int ntot = g.n[0] * g.n[1] * g.n[2];
    for (int t = lt; t < ntot; t += T) {
      int i, j, k;
      const double x = c[geo_at(g, t, i, j, k)];
      const double n = (g.nd == 3 ? k : j) + 1;
      if (x > threshold && n < first) first = n;
    }
  }
  team_best<T>(first, none, true);
  if (lt == 0 && q < nl) {
    const afh_box_meta &m = meta[ids[q] - 1];
    const bool any = first < HUGE_VAL;
    const double z = m.r_min[g.nd - 1] + (first - 0.5) * m.dr[g.nd - 1];
    part[2 * q] = any ? z : 1e100;
    part[2 * q + 1] = any ? z : -1e100;
  }
}

// reduce_minmax from limits over the per-leaf pairs (min and max select, so
// the order does not enter). One workgroup.
__global__ void __launch_bounds__(AN_NT)
    k_fold_minmax(const double *__restrict__ part, int nl, double lim0, double lim1,
                  double *__restrict__ out) {
  double lo = lim0, hi = lim1;
  int a = 0, b = 0;
  for (int q = threadIdx.x; q < nl; q += AN_NT) {
    lo = fmin(lo, part[2 * q]);
    hi = fmax(hi, part[2 * q + 1]);
  }
  team_best<AN_NT>(lo, a, true);
  team_best<AN_NT>(hi, b, false);
  if (threadIdx.x == 0) out[0] = lo, out[1] = hi;
}

// analysis_get_maxima's test of cell t of a box (c: the cell (1, 1[, 1])):
// above the threshold, not below any of the 2 ND face neighbours, above at
// least one. The neighbours of a boundary cell are the ghost cells as stored.
__device__ __forceinline__ bool is_maximum(const double *c, const Geo &g, int t, double thr,
                                           int &i, int &j, int &k) {
  const double *p = c + geo_at(g, t, i, j, k);
  const double val = *p;
  bool all = true, any = false;
  int step = 1;
  for (int d = 0; d < g.nd; d++, step *= g.pitch) {
    const double lo = p[-step], hi = p[step];
    all = all && val >= lo && val >= hi;
    any = any || val > lo || val > hi;
  }
  return val > thr && all && any;
}

// The local maxima of every leaf, T = 16 or 64 lanes per leaf. offs == null:
// count them into counts[q]. Else write those at positions offs[q] + (rank in
// cell order, i fastest) < n_max into coord_val ((ND + 1) x n_max, coordinates
// then value): the list is ordered by leaf, then cell.
template <int T>
__global__ void __launch_bounds__(AN_NT)
    k_box_maxima(const double *__restrict__ v, Geo g, const int32_t *__restrict__ ids, int nl,
                 double threshold, const afh_box_meta *__restrict__ meta,
                 int32_t *__restrict__ counts, const int32_t *__restrict__ offs, int n_max,
                 double *__restrict__ coord_val) {
  static_assert(T == 16 || T == 64, "a team lies within one wave");
  const int lt = threadIdx.x % T;
  const int q = blockIdx.x * (AN_NT / T) + threadIdx.x / T;
  const int shift = (threadIdx.x & 63) / T * T;  // the team's first lane in its wave
  const bool in = q < nl;
  const int id = in ? ids[q] : 1;
  const double *c = v + (size_t)(id - 1) * g.stride + g.off;
  const int ntot = g.n[0] * g.n[1] * g.n[2];
  int pos = in && offs ? offs[q] : 0;
  for (int t0 = 0; t0 < ntot; t0 += T) {
    const int t = t0 + lt;
    int i = 0, j = 0, k = 0;
    const bool f = in && t < ntot && is_maximum(c, g, t, threshold, i, j, k);
    unsigned long long m = __ballot(f) >> shift;
    if (T < 64) m &= (1ull << T) - 1;
    if (offs && f) {
      const int at = pos + __popcll(m & ((1ull << lt) - 1));
      if (at < n_max) {
        const afh_box_meta &b = meta[id - 1];
        double *o = coord_val + (size_t)(g.nd + 1) * at;
        o[0] = b.r_min[0] + (i + 1 - 0.5) * b.dr[0];
        o[1] = b.r_min[1] + (j + 1 - 0.5) * b.dr[1];
        if (g.nd == 3) o[2] = b.r_min[2] + (k + 1 - 0.5) * b.dr[2];
        o[g.nd] = c[geo_at(g, t, i, j, k)];
      }
    }
    pos += __popcll(m);
  }
  if (!offs && lt == 0 && in) counts[q] = pos;
}

// Exclusive scan of counts[0 .. nl) into offs, the total into *total. One
// workgroup: each thread a contiguous chunk, the chunk sums scanned in LDS.
__global__ void __launch_bounds__(AN_NT)
    k_scan_counts(const int32_t *__restrict__ counts, int nl, int32_t *__restrict__ offs,
                  double *__restrict__ total) {
  __shared__ int s[AN_NT];
  const int per = (nl + AN_NT - 1) / AN_NT;
  const int q0 = min(nl, (int)threadIdx.x * per), q1 = min(nl, q0 + per);
  int sum = 0;
  for (int q = q0; q < q1; q++) sum += counts[q];
  s[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int w = 0; w < AN_NT; w++) {
      const int x = s[w];
      s[w] = run;
      run += x;
    }
    *total = (double)run;
  }
  __syncthreads();
  int run = s[threadIdx.x];
  for (int q = q0; q < q1; q++) {
    offs[q] = run;
    run += counts[q];
  }
}

// ---------------------------------------------------------------- host side
// What the launchers need of a tree (either library's): the leaf list in the
// reference's loop order, the box records, per-leaf scratch of 2 nl doubles
// and a result buffer of 4 + (nd + 1) n_max doubles.
struct Ctx {
  hipStream_t stream;
  int nd, nc, nl;
  const int32_t *leaves;
  const afh_box_meta *meta;
  double *part, *res;
};

inline int team_of(const Geo &g) {
  const int n = g.n[0] * g.n[1] * g.n[2];
  return n <= 16 ? 16 : (n <= 64 ? 64 : AN_NT);
}

#define AFH_AN_TRY(call)               \
  do {                                 \
    hipError_t _e = (call);            \
    if (_e != hipSuccess) return _e;   \
  } while (0)

// af_reduction_loc of the per-leaf extrema of range g: *out and loc = (id,
// index 1-based per dimension, 0 past nd) or -1; one synchronisation
inline hipError_t best_loc(const Ctx &c, const double *v, const Geo &g, bool is_min,
                           const Region &R, double init, double *out, int32_t *loc) {
  double h[3] = {init, -1.0, -1.0};
  if (c.nl > 0) {
    const int T = team_of(g);
    const dim3 grid((c.nl + AN_NT / T - 1) / (AN_NT / T)), blk(AN_NT);
    auto kern = T == 16 ? k_box_best<16> : (T == 64 ? k_box_best<64> : k_box_best<AN_NT>);
    hipLaunchKernelGGL(kern, grid, blk, 0, c.stream, v, g, c.leaves, c.nl, (int)is_min, c.meta,
                       R, c.nc, c.part);
    AFH_AN_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fold_loc, dim3(1), blk, 0, c.stream, c.part, c.leaves, c.nl,
                       (int)is_min, init, c.res);
    AFH_AN_TRY(hipGetLastError());
    AFH_AN_TRY(hipMemcpyAsync(h, c.res, sizeof h, hipMemcpyDeviceToHost, c.stream));
    AFH_AN_TRY(hipStreamSynchronize(c.stream));
  }
  *out = h[0];
  if (loc) {
    const int lix = (int)h[2];
    loc[0] = (int32_t)h[1];
    loc[1] = lix < 0 ? -1 : lix % g.n[0] + 1;
    loc[2] = lix < 0 ? -1 : (lix / g.n[0]) % g.n[1] + 1;
    loc[3] = c.nd == 3 ? (lix < 0 ? -1 : lix / (g.n[0] * g.n[1]) + 1) : 0;
  }
  return hipSuccess;
}

inline hipError_t zminmax(const Ctx &c, const double *v, const Geo &g, double threshold,
                          const double *limits, double *out) {
  out[0] = limits[0], out[1] = limits[1];
  if (c.nl == 0) return hipSuccess;
  const int T = team_of(g);
  const dim3 grid((c.nl + AN_NT / T - 1) / (AN_NT / T)), blk(AN_NT);
  auto kern = T == 16 ? k_box_zfirst<16> : (T == 64 ? k_box_zfirst<64> : k_box_zfirst<AN_NT>);
  hipLaunchKernelGGL(kern, grid, blk, 0, c.stream, v, g, c.leaves, c.nl, threshold, c.meta,
                     c.part);
  AFH_AN_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_fold_minmax, dim3(1), blk, 0, c.stream, c.part, c.nl, limits[0],
                     limits[1], c.res);
  AFH_AN_TRY(hipGetLastError());
  AFH_AN_TRY(hipMemcpyAsync(out, c.res, 2 * sizeof(double), hipMemcpyDeviceToHost, c.stream));
  return hipStreamSynchronize(c.stream);
}

// count, scan, write; the found entries (at most n_max) and the count come
// back in one transfer
inline hipError_t maxima(const Ctx &c, const double *v, const Geo &g, double threshold,
                         int n_max, double *coord_val, int32_t *n_found) {
  *n_found = 0;
  if (c.nl == 0) return hipSuccess;
  const int T = g.n[0] * g.n[1] * g.n[2] <= 16 ? 16 : 64;
  const dim3 grid((c.nl + AN_NT / T - 1) / (AN_NT / T)), blk(AN_NT);
  auto kern = T == 16 ? k_box_maxima<16> : k_box_maxima<64>;
  int32_t *counts = reinterpret_cast<int32_t *>(c.part), *offs = counts + c.nl;
  double *d_cv = c.res + 4;
  const int32_t *no_offs = nullptr;
  hipLaunchKernelGGL(kern, grid, blk, 0, c.stream, v, g, c.leaves, c.nl, threshold, c.meta,
                     counts, no_offs, n_max, d_cv);
  AFH_AN_TRY(hipGetLastError());
  hipLaunchKernelGGL(k_scan_counts, dim3(1), blk, 0, c.stream, counts, c.nl, offs, c.res);
  AFH_AN_TRY(hipGetLastError());
  if (n_max > 0) {
    hipLaunchKernelGGL(kern, grid, blk, 0, c.stream, v, g, c.leaves, c.nl, threshold, c.meta,
                       counts, (const int32_t *)offs, n_max, d_cv);
    AFH_AN_TRY(hipGetLastError());
  }
  // (the whole buffer in one copy: what lies past the found entries is not
  // handed on)
  const size_t w = (size_t)(c.nd + 1) * n_max;
  double *h = new double[4 + w];
  hipError_t e = hipMemcpyAsync(h, c.res, sizeof(double) * (4 + w), hipMemcpyDeviceToHost,
                                c.stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e == hipSuccess) {
    *n_found = (int32_t)h[0];
    const size_t n = (size_t)(c.nd + 1) * (size_t)(*n_found < n_max ? *n_found : n_max);
    for (size_t x = 0; x < n; x++) coord_val[x] = h[4 + x];
  }
  delete[] h;
  return e;
}

// ---------------------------------------------------------- the entry points
// The four functions of afivo_hip_analysis.h on a tree of either library (ND
// = 3 or 2), after the library's guard of the handle. The 2-D shapes: loc =
// (id, i, j, 0), r0 and r1 read to their second entry, coord_val 3 x n_max.
//
// The launchers' view of the tree, with the per-leaf scratch and the result
// buffer (4 + n_list doubles) grown to fit.
template <int ND, class Tree>
inline int32_t an_ctx(Tree *t, size_t n_list, const char *what, Ctx &c) {
  using afhc::set_error;
  if constexpr (ND == 3)
    if (t->hook || t->dev_reduce)
      return set_error(AFH_ERR_UNSUPPORTED, "%s: the fold over the ranks of a sharded tree is "
                       "not built", what);
  const int nl = t->leaves.off[t->nlvl];
  if (nl > t->boxred_cap) {
    AFH_HIP(hipStreamSynchronize(t->stream));
    hipFree(t->d_boxred);
    t->d_boxred = nullptr, t->boxred_cap = 0;
    AFH_HIP(hipMalloc(&t->d_boxred, sizeof(double) * 2 * nl));
    t->boxred_cap = nl;
  }
  if (4 + n_list > t->an_cap) {
    AFH_HIP(hipStreamSynchronize(t->stream));
    hipFree(t->d_an);
    t->d_an = nullptr, t->an_cap = 0;
    AFH_HIP(hipMalloc(&t->d_an, sizeof(double) * (4 + n_list)));
    t->an_cap = 4 + n_list;
  }
  c.stream = t->stream;
  c.nd = ND, c.nc = t->nc, c.nl = nl;
  c.leaves = t->leaves.d;
  c.meta = t->d_boxes;
  c.part = t->d_boxred, c.res = t->d_an;
  return AFH_OK;
}

template <int ND, class Tree>
inline int32_t reduce_fc(Tree *t, int32_t ivf, int32_t dim, int32_t op, double *out,
                         int32_t *loc) {
  if (ivf < 1 || ivf > t->nvf || dim < 1 || dim > ND || !out ||
      (op != AFH_RED_MAX && op != AFH_RED_MIN))
    return afhc::set_error(AFH_ERR_ARG, "afh_tree_reduce_fc: bad argument");
  Ctx c;
  if (int32_t e = an_ctx<ND>(t, 0, "afh_tree_reduce_fc", c)) return e;
  const bool is_min = op == AFH_RED_MIN;
  Region none = {};
  AFH_HIP(best_loc(c, t->fcv(ivf), geo_fc(ND, t->nc, t->fsz, dim - 1), is_min, none,
                   (is_min ? 1 : -1) * (DBL_MAX / 10), out, loc));
  return AFH_OK;
}

template <int ND, class Tree>
inline int32_t zminmax_threshold(Tree *t, int32_t iv, double threshold, const double *limits,
                                 double *out) {
  if (iv < 1 || iv > t->nvc || !limits || !out)
    return afhc::set_error(AFH_ERR_ARG, "afh_tree_zminmax_threshold: bad argument");
  Ctx c;
  if (int32_t e = an_ctx<ND>(t, 0, "afh_tree_zminmax_threshold", c)) return e;
  AFH_HIP(zminmax(c, t->ccv(iv), geo_cc(ND, t->nc, t->bsz), threshold, limits, out));
  return AFH_OK;
}

template <int ND, class Tree>
inline int32_t max_region(Tree *t, int32_t iv, const double *r0, const double *r1, double *out,
                          int32_t *loc) {
  if (iv < 1 || iv > t->nvc || !r0 || !r1 || !out)
    return afhc::set_error(AFH_ERR_ARG, "afh_tree_max_region: bad argument");
  Ctx c;
  if (int32_t e = an_ctx<ND>(t, 0, "afh_tree_max_region", c)) return e;
  Region R = {};
  R.on = 1;
  for (int d = 0; d < ND; d++) R.r0[d] = r0[d], R.r1[d] = r1[d];
  AFH_HIP(best_loc(c, t->ccv(iv), geo_cc(ND, t->nc, t->bsz), false, R, -1e100, out, loc));
  return AFH_OK;
}

template <int ND, class Tree>
inline int32_t local_maxima(Tree *t, int32_t iv, double threshold, int32_t n_max,
                            double *coord_val, int32_t *n_found) {
  if (iv < 1 || iv > t->nvc || n_max < 0 || (n_max > 0 && !coord_val) || !n_found)
    return afhc::set_error(AFH_ERR_ARG, "afh_tree_local_maxima: bad argument");
  Ctx c;
  if (int32_t e = an_ctx<ND>(t, (size_t)(ND + 1) * n_max, "afh_tree_local_maxima", c)) return e;
  AFH_HIP(maxima(c, t->ccv(iv), geo_cc(ND, t->nc, t->bsz), threshold, n_max, coord_val,
                 n_found));
  return AFH_OK;
}

}  // namespace
}  // namespace afh_an
