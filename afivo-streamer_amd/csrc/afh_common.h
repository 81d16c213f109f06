// What libafivo_hip.so (afh_internal.h) and libafivo_hip_2d.so (afh2d.hip)
// share: everything that does not depend on the dimension, stated once.
// Device arithmetic that must give the reference's bits in both libraries
// (limiter, table lookup, the field rate forms, the Fortran runtime's NORM2,
// the ordered keys of the max / min reductions, the rate-sum folds) and the
// host plumbing behind the common ABI (error text, level lists, kernel timing,
// rate sums, source factor, reaction upload, the per-leaf folds). The trees
// and fluids of the two libraries stay separate types: the host helpers reach
// them through templates or through the member structs Prof and RateSums.
// Everything is inline or a template, and what depends on a library's own
// types has internal linkage, so both libraries may live in one process.
#pragma once

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/afivo_hip.h"
#include "../../include/afivo_hip_srcfac.h"

namespace afhc {

// ------------------------------------------------------------ errors
// the thread's message behind afh_last_error
inline char *err_text() {
  static thread_local char buf[512] = "";
  return buf;
}

inline int32_t set_error(int32_t code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(err_text(), 512, fmt, ap);
  va_end(ap);
  return code;
}

inline int32_t check_hip(hipError_t e, const char *what) {
  return set_error(AFH_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
}

#define AFH_HIP(call)                                                         \
  do {                                                                        \
    hipError_t _e = (call);                                                   \
    if (_e != hipSuccess) return ::afhc::check_hip(_e, #call);                \
  } while (0)
#define AFH_LAUNCH_CHECK(what)                                                \
  do {                                                                        \
    hipError_t _e = hipGetLastError();                                        \
    if (_e != hipSuccess) return ::afhc::check_hip(_e, what);                 \
  } while (0)

// ------------------------------------------------------------ ordered keys
// Orderable encoding of doubles for atomicMax/Min on 64-bit integers.
__device__ __forceinline__ unsigned long long dbl_to_ord(double x) {
  unsigned long long u = __double_as_longlong(x);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
inline double ord_to_dbl(unsigned long long o) {
  unsigned long long u =
      (o & 0x8000000000000000ull) ? (o & ~0x8000000000000000ull) : ~o;
  double d;
  memcpy(&d, &u, sizeof d);
  return d;
}
inline unsigned long long host_dbl_to_ord(double x) {
  unsigned long long u;
  memcpy(&u, &x, sizeof u);
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

// ------------------------------------------------------------ limiter
// af_limiter_apply (m_af_limiters.f90:41-149)
__device__ __forceinline__ double limiter(int lim, double a, double b) {
  const double third = 1 / 3.0;
  switch (lim) {
  case AFH_LIM_KOREN: {
    const double aa = a * a, ab = a * b;
    if (ab <= 0) return 0;
    if (aa <= 0.25 * ab) return 2 * a;
    if (aa <= 2.5 * ab) return third * (b + 2 * a);
    return 2 * b;
  }
  case AFH_LIM_VANLEER: {
    const double ab = a * b;
    return ab > 0 ? 2 * ab / (a + b) : 0;
  }
  case AFH_LIM_NONE: return 0.5 * (a + b);
  case AFH_LIM_ZERO: return 0.0;
  default: {
    const double th =
        lim == AFH_LIM_MINMOD ? 1.0 : lim == AFH_LIM_MC ? 2.0 : 4 / 3.0;
    if (a * b > 0) {
      double m = fabs(th * a);
      const double y = fabs(th * b), z = fabs(0.5 * (a + b));
      if (y < m) m = y;
      if (z < m) m = z;
      return copysign(m, a);
    }
    return 0.0;
  }
  }
}

// ------------------------------------------------------------ lookup tables
// A lookup table on the device, column-major [col][row] (LT_get_col reads one
// column). The 3-D chemistry table derives from it (afh_species.hip DevLTrm).
struct DevLT {
  int n_points, n_cols;
  double x_min, inv_fac;
  const double *rc;
};

// LT_get_loc + LT_get_col_at_loc (m_lookup_table.f90:330-406)
__device__ __forceinline__ double lt_col(const DevLT &lt, int col, double x) {
  const double frac = (x - lt.x_min) * lt.inv_fac;
  int low;
  double lf;
  if (frac <= 0) {
    low = 1;
    lf = 1;
  } else if (frac >= lt.n_points - 1) {
    low = lt.n_points - 1;
    lf = 0;
  } else {
    low = (int)ceil(frac);
    lf = low - frac;
  }
  const double *r = lt.rc + (size_t)(col - 1) * lt.n_points;
  return lf * r[low - 1] + (1 - lf) * r[low];
}

// ------------------------------------------------------------ reactions
struct DevReaction {
  int rate_type, table_col, n_in, n_out;
  double rate_factor, c[4];
  int ix_in[4], ix_out[4], mult_out[4];
};

// get_rates for the field forms (src/m_chemistry.f90:565-620), T the rate
// type, c0 and c the reaction's rate_factor and c; tab(col) is the library's
// lookup of the chemistry table at the field. Each library's rate_of switches
// over the reaction's type itself (c0 and c read before the switch; the 2-D
// one has no case for the types it refuses): the shape of that switch is
// what the update kernels' instructions depend on.
template <int T, class Tab>
__device__ __forceinline__ double field_form(double c0, const double *c, int col, double field,
                                             Tab tab) {
  static_assert(T >= AFH_RATE_TABULATED_FIELD && T <= AFH_RATE_EXP_V2, "not a field form");
  if constexpr (T == AFH_RATE_TABULATED_FIELD) {
    return c0 * tab(col);
  } else if constexpr (T == AFH_RATE_CONSTANT) {
    return c0 * c[0];
  } else if constexpr (T == AFH_RATE_LINEAR) {
    return c0 * c[0] * (field - c[1]);
  } else if constexpr (T == AFH_RATE_EXP_V1) {
    const double z = c[1] / (c[2] + field);
    return c0 * c[0] * exp(-(z * z));
  } else {
    const double z = field / c[1];
    return c0 * c[0] * exp(-(z * z));
  }
}
// of reaction R with the compile-time type T
template <int T, class Tab>
__device__ __forceinline__ double field_rate(const DevReaction &R, double field, Tab tab) {
  const double c0 = R.rate_factor;
  const double *c = R.c;
  return field_form<T>(c0, c, R.table_col, field, tab);
}

// ------------------------------------------------------------ NORM2
// NORM2 as the Fortran runtime of the reference build evaluates it (element
// by element: the largest magnitude m so far, s = the sum of (x / m)^2 over
// the others, rescaled when m grows; m sqrt(1 + s)) -- not sqrt(a a + b b +
// c c), which differs in the last bit for about a third of all inputs.
// afh.electrode.norm2 is the same evaluation on the host.
__device__ __forceinline__ void norm2_acc(double x, double &m, double &s) {
  const double a = fabs(x);
  if (m == 0.0) {
    m = a;
  } else if (a > m) {
    const double t = m / a, tsq = t * t;
    s = s * tsq;
    s = s + tsq;
    m = a;
  } else {
    const double t = a / m;
    s = s + t * t;
  }
}
__device__ __forceinline__ double norm2_3(double a, double b, double c) {
  double m = 0.0, s = 0.0;
  norm2_acc(a, m, s);
  norm2_acc(b, m, s);
  norm2_acc(c, m, s);
  return m * sqrt(1 + s);
}
// of (a, b): the largest magnitude m, the other over m squared
__device__ __forceinline__ double norm2_2(double a, double b) {
  a = fabs(a), b = fabs(b);
  if (a == 0.0) return b * sqrt(1 + 0.0);
  const double t = b > a ? a / b : b / a;
  return (b > a ? b : a) * sqrt(1 + t * t);
}

// ------------------------------------------------------------ rate sums
// the wave's sum in a fixed order (the xor butterfly: every lane ends with
// the same bits); every lane of the wave must be active
__device__ __forceinline__ double wave_sum(double v) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
  return v;
}
// the wave partials of an update workgroup that forms the rate and J.E sums:
// [nr + 1][4 waves]
__device__ __forceinline__ double *rate_sum_lds() {
  __shared__ double w[(AFH_MAX_REACTIONS + 1) * 4];
  return w;
}

// k_rate_fold / k2_rate_fold: adds the rows of part in a fixed order: one
// workgroup of 256 per column (reaction, J.E), lane q the rows q, q + 256, ...
// in turn, then the lanes' sums by halving through LDS
__device__ __forceinline__ void rate_fold(const double *__restrict__ part, int n_rows,
                                          int n_col, double *__restrict__ out) {
  const int c = blockIdx.x;
  double s = 0.0;
  for (int r = threadIdx.x; r < n_rows; r += 256) s = s + part[(size_t)r * n_col + c];
  __shared__ double w[256];
  w[threadIdx.x] = s;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) w[threadIdx.x] = w[threadIdx.x] + w[threadIdx.x + h];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = w[0];
}

// afh_fluid_set_rate_sums / afh_fluid_fetch_rate_sums (include/
// afivo_hip_rates.h): on, whether a last step has filled the result, the
// workgroups' partial rows (cap rows of n_reactions + 1 doubles, regrown when
// a step has more workgroups) and the folded result on the device
struct RateSums {
  bool on = false, valid = false;
  double *part = nullptr, *out = nullptr;
  size_t cap = 0;
  int32_t reserve(size_t rows, size_t ncol, hipStream_t stream) {
    if (!out) AFH_HIP(hipMalloc(&out, ncol * sizeof(double)));
    if (rows > cap) {
      // (a queued fold may still read the old rows)
      AFH_HIP(hipStreamSynchronize(stream));
      hipFree(part);
      part = nullptr;
      cap = 0;
      AFH_HIP(hipMalloc(&part, rows * ncol * sizeof(double)));
      cap = rows;
    }
    return AFH_OK;
  }
  int32_t fetch(int nr, hipStream_t stream, double *rates, double *jdote) {
    if (!on) return set_error(AFH_ERR_STATE, "afh_fluid_fetch_rate_sums: the sums are off");
    if (!valid)
      return set_error(AFH_ERR_STATE,
                       "afh_fluid_fetch_rate_sums: no last step since the sums were switched on");
    double h[AFH_MAX_REACTIONS + 1];
    AFH_HIP(hipMemcpyAsync(h, out, (nr + 1) * sizeof(double), hipMemcpyDeviceToHost, stream));
    AFH_HIP(hipStreamSynchronize(stream));
    for (int r = 0; r < nr; r++) rates[r] = h[r];
    *jdote = h[nr];
    return AFH_OK;
  }
  // afh_fluid_set_rate_sums after the library's guards; rows: the update
  // workgroups of a step on the tree as it is
  int32_t set(bool want, size_t rows, size_t ncol, hipStream_t stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    AFH_HIP(hipStreamIsCapturing(stream, &cs));
    if (cs != hipStreamCaptureStatusNone)
      return set_error(AFH_ERR_STATE, "afh_fluid_set_rate_sums during a graph capture");
    if (want && !on) {
      if (int32_t e = reserve(rows, ncol, stream)) return e;
      valid = false;
    }
    on = want;
    return AFH_OK;
  }
  void release() { hipFree(part), hipFree(out); }
};

// ------------------------------------------------------------ level lists
struct LevelList {
  std::vector<int32_t> off;  // highest_lvl + 1 offsets
  int32_t *d = nullptr;      // device, concatenated 1-based ids
  int n(int lvl) const { return off[lvl] - off[lvl - 1]; }
  const int32_t *at(int lvl) const { return d + off[lvl - 1]; }
};

// per-level id lists -> one device array with offsets (frees L's old array;
// an empty list still gets an allocation, so d is never null afterwards)
inline int32_t upload_list(LevelList &L, const std::vector<std::vector<int32_t>> &lists) {
  if (L.d) hipFree(L.d), L.d = nullptr;
  L.off.assign(lists.size() + 1, 0);
  std::vector<int32_t> flat;
  for (size_t l = 0; l < lists.size(); l++) {
    flat.insert(flat.end(), lists[l].begin(), lists[l].end());
    L.off[l + 1] = (int32_t)flat.size();
  }
  AFH_HIP(hipMalloc(&L.d, sizeof(int32_t) * (flat.size() + 1)));
  if (!flat.empty())
    AFH_HIP(hipMemcpy(L.d, flat.data(), sizeof(int32_t) * flat.size(),
                      hipMemcpyHostToDevice));
  return AFH_OK;
}

inline void free_list(LevelList &L) {
  if (L.d) hipFree(L.d);
  L.d = nullptr;
}

// a host id list on the device (at least one entry allocated)
inline int32_t device_list(const std::vector<int32_t> &h, int32_t **d) {
  AFH_HIP(hipMalloc(d, sizeof(int32_t) * std::max<size_t>(1, h.size())));
  if (!h.empty())
    AFH_HIP(hipMemcpy(*d, h.data(), sizeof(int32_t) * h.size(), hipMemcpyHostToDevice));
  return AFH_OK;
}

// Workgroup lanes for a per-box launch of `work` items: the work rounded up
// to whole waves, at most 256 (an 8^3 box's 64-cell face or 96 edge cells, an
// 8^2 box's cells, without the idle waves of a 256-lane workgroup).
inline int fit_blk(int work) {
  return work < 256 ? ((work + 63) / 64) * 64 : 256;
}

// ------------------------------------------------------------ kernel timing
// afh_profile_enable / afh_profile_read: HIP events around every launch of
// one kernel class on the tree's stream. A member `prof` of both trees.
struct Prof {
  int cls = 0;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  double bytes = 0;
  int64_t launches = 0;
  hipEvent_t next_event() {
    if (ev_used == ev_pool.size()) {
      hipEvent_t e;
      hipEventCreate(&e);
      ev_pool.push_back(e);
    }
    return ev_pool[ev_used++];
  }
  void reset() {
    ev_used = 0;
    bytes = 0;
    launches = 0;
  }
};

// The templates over a library's tree or fluid type have internal linkage
// (both libraries name theirs afh_tree and afh_fluid, with different
// layouts: an instantiation must never be shared between them).
namespace {

// bracket one launch of class `kc` (no-op unless enabled)
template <class Tree> inline void prof_begin(Tree *t, int kc) {
  if (t->prof.cls != kc) return;
  hipEventRecord(t->prof.next_event(), t->stream);
}
template <class Tree> inline void prof_count(Tree *t, double bytes) {
  t->prof.bytes += bytes;
  t->prof.launches++;
}
template <class Tree> inline void prof_end(Tree *t, int kc, double bytes) {
  if (t->prof.cls != kc) return;
  hipEventRecord(t->prof.next_event(), t->stream);
  prof_count(t, bytes);
}
// or: a start / end event pair for a launch that records them itself
// (hipExtLaunchKernelGGL; false: class not timed), then prof_count
template <class Tree> inline bool prof_ext(Tree *t, int kc, hipEvent_t &e0, hipEvent_t &e1) {
  if (t->prof.cls != kc) return false;
  e0 = t->prof.next_event();
  e1 = t->prof.next_event();
  return true;
}

// afh_profile_enable / afh_profile_read after the library's guards
template <class Tree> inline int32_t profile_enable(Tree *t, int32_t kclass) {
  AFH_HIP(hipStreamSynchronize(t->stream));
  t->prof.cls = kclass;
  t->prof.reset();
  return AFH_OK;
}
template <class Tree>
inline int32_t profile_read(Tree *t, double *total_ms, int64_t *launches, double *bytes) {
  AFH_HIP(hipStreamSynchronize(t->stream));
  double ms = 0;
  for (size_t q = 0; q + 1 < t->prof.ev_used; q += 2) {
    float e = 0;
    AFH_HIP(hipEventElapsedTime(&e, t->prof.ev_pool[q], t->prof.ev_pool[q + 1]));
    ms += e;
  }
  *total_ms = ms;
  *launches = t->prof.launches;
  *bytes = t->prof.bytes;
  t->prof.reset();
  return AFH_OK;
}

// ------------------------------------------------------------ source factor
// afh_fluid_set_source_factor (include/afivo_hip_srcfac.h) after the
// library's guards. used_too: i_srcfac is a variable the step uses besides
// those both libraries know (the 3-D rhs output).
template <class Fluid>
inline int32_t set_source_factor(Fluid *f, int32_t mode, const uint8_t *ionization,
                                 double min_electrons_per_cell, int32_t i_srcfac,
                                 bool used_too) {
  auto *t = f->t;
  if (mode != AFH_SRCFAC_NONE && mode != AFH_SRCFAC_FLUX)
    return set_error(AFH_ERR_ARG, "afh_fluid_set_source_factor: unknown mode %d", mode);
  if (mode == AFH_SRCFAC_FLUX && !ionization)
    return set_error(AFH_ERR_ARG, "afh_fluid_set_source_factor: no ionization flags");
  if (i_srcfac < 0 || i_srcfac > t->nvc)
    return set_error(AFH_ERR_ARG, "afh_fluid_set_source_factor: bad i_srcfac %d", i_srcfac);
  // (the other states of the species: the update, with the states of the step)
  bool used = i_srcfac > 0 && (i_srcfac == f->d.i_efld || i_srcfac == f->d.i_photo ||
                               i_srcfac == f->d.i_gas_dens || i_srcfac == f->mask_iv ||
                               used_too);
  for (int s = 0; s < f->d.n_species && i_srcfac > 0; s++)
    used = used || i_srcfac == f->d.species_iv[s];
  if (used)
    return set_error(AFH_ERR_ARG,
                     "afh_fluid_set_source_factor: i_srcfac %d is a variable the step uses",
                     i_srcfac);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  AFH_HIP(hipStreamIsCapturing(t->stream, &cs));
  if (cs != hipStreamCaptureStatusNone)
    return set_error(AFH_ERR_STATE, "afh_fluid_set_source_factor during a graph capture");
  if (mode == AFH_SRCFAC_FLUX && f->d.n_reactions > 0) {
    // (a queued update may still read the previous flags)
    AFH_HIP(hipStreamSynchronize(t->stream));
    if (!f->d_sf_ion) AFH_HIP(hipMalloc(&f->d_sf_ion, AFH_MAX_REACTIONS));
    uint8_t flags[AFH_MAX_REACTIONS];
    for (int r = 0; r < f->d.n_reactions; r++) flags[r] = ionization[r] ? 1 : 0;
    AFH_HIP(hipMemcpy(f->d_sf_ion, flags, f->d.n_reactions, hipMemcpyHostToDevice));
  }
  f->sf_mode = mode;
  f->sf_min_e = min_electrons_per_cell;
  f->sf_iv = i_srcfac;
  return AFH_OK;
}

}  // namespace

// ------------------------------------------------------------ reaction upload
// The reaction list of a fluid (validated by the library) on the device;
// remap(ix): the kernels' species slot + 1 of the reference's 1-based species
// index ix (entries past n_in / n_out are copied as they are)
template <class Remap>
inline int32_t upload_reactions(const afh_fluid_desc *d, Remap remap, DevReaction **d_reac) {
  std::vector<DevReaction> R(std::max(1, d->n_reactions));
  for (int r = 0; r < d->n_reactions; r++) {
    const afh_reaction &a = d->reactions[r];
    DevReaction &b = R[r];
    b.rate_type = a.rate_type;
    b.table_col = a.table_col;
    b.n_in = a.n_in;
    b.n_out = a.n_out;
    b.rate_factor = a.rate_factor;
    for (int q = 0; q < 4; q++) {
      b.c[q] = a.c[q];
      b.ix_in[q] = q < a.n_in ? remap(a.ix_in[q]) : a.ix_in[q];
      b.ix_out[q] = q < a.n_out ? remap(a.ix_out[q]) : a.ix_out[q];
      b.mult_out[q] = a.mult_out[q];
    }
  }
  AFH_HIP(hipMalloc(d_reac, sizeof(DevReaction) * R.size()));
  AFH_HIP(hipMemcpy(*d_reac, R.data(), sizeof(DevReaction) * R.size(),
                    hipMemcpyHostToDevice));
  return AFH_OK;
}

// ------------------------------------------------------------ per-leaf folds
// afh_tree_sum_cc's fold of the per-leaf (sum, -) pairs res, leaves in level
// order: my_sum = my_sum + fac * tmp with fac = weight[l - 1], the level's
// cell volume; skip (or null): per box id - 1, a leaf another rank counts
inline double fold_leaf_sums(const std::vector<double> &res, const std::vector<double> &weight,
                             const std::vector<std::vector<int32_t>> &leaves,
                             const std::vector<char> *skip = nullptr) {
  double sum = 0.0;
  size_t q = 0;
  for (size_t l = 0; l < leaves.size(); l++) {
    const double fac = weight[l];
    for (size_t b = 0; b < leaves[l].size(); b++, q++)
      if (!skip || skip->empty() || !(*skip)[leaves[l][b] - 1]) sum = sum + fac * res[2 * q];
  }
  return sum;
}

// af_reduction_loc over the per-leaf (value, linear index) pairs res: init
// -huge/10 (max) or huge/10 (min); a box replaces the running value when
// reduction(tmp, val) differs from val. lid, lix: its box id and linear
// index, or -1
inline double fold_leaf_best(const std::vector<double> &res,
                             const std::vector<std::vector<int32_t>> &leaves, bool is_min,
                             int32_t &lid, int32_t &lix) {
  double val = (is_min ? 1 : -1) * (DBL_MAX / 10);
  lid = -1, lix = -1;
  size_t q = 0;
  for (size_t l = 0; l < leaves.size(); l++)
    for (size_t b = 0; b < leaves[l].size(); b++, q++) {
      const double tmp = res[2 * q];
      const double nv = is_min ? std::min(tmp, val) : std::max(tmp, val);
      if (std::fabs(nv - val) > 0) {
        val = tmp;
        lid = leaves[l][b];
        lix = (int32_t)res[2 * q + 1];
      }
    }
  return val;
}

}  // namespace afhc
