// crosslink.hip -- crosslinkers that bind and unbind: the kinetic Monte Carlo stage of the reference's HP1 app
// (scrap/.../HP1.cpp:3264-3438 rates, :3440-3594 sampling, :3597-3748 state changes, :4728-4739 place in the step;
// NgpHP1.cpp:1830-2137 the same over a per-crosslinker list of bind sites), which the reference runs serially on the
// host inside an STK modification cycle.  Here the spring set changes on the device:
//   candidate rows   the CSR of a neighbour search (sources: beads with a crosslinker, targets: bind sites), each row
//                    sorted by original body id once per list build
//   KMC              one lane per crosslinker: one Philox uniform, two passes over the left bead's row (total rate, then
//                    the running sum that picks the site), nothing stored per candidate
//   incidence        body -> crosslinker lists of the left ends (static) and of the right ends of the doubly bound ones
//                    (rebuilt after every KMC step: count, scan, fill, per-body sort)
//   force            one lane per body, its left and right lists merged in ascending crosslinker index, no atomics
// All of it gathers a few rows per lane: bound by the latency of those gathers.
//
// Periphery bind sites (include/mundy_hip_periphery_binding.h; HP1.cpp:3340-3398 their rates, :3473-3529 the
// one draw over both kinds of site): P immobile points with rate constants of their own.  right[c] == -(s + 1) is "bound
// to site s".  The KMC lane walks a second candidate row (sites, ascending index) after the bead row in the same two
// sums; the force lane takes the far end from the site array; nothing indexed by a body ever sees a negative right.
// One text serves both: the force, KMC and renumber kernels are SITES = false / true instantiations of one body each (the
// KMC's behind two entry points, k_xl_kmc and k_xl_kmc_periphery, which keep the grid-stride loop and their own argument
// lists), and one incidence source (force_device.hpp's ListedAtBody) builds the right lists of either kind of handle.
#include "mhip_internal.hpp"
#include "force_device.hpp"
#include "../../include/mundy_hip_periphery_binding.h"

#include <cmath>

namespace mhip {

struct XlParams {
  double k, r, A, k_off, inv_kt, cap;
};

// binding rate of a singly bound crosslinker to a site at distance d (HP1.cpp:3320, :3332-3334, their association)
template <int TYPE>
__device__ inline double xl_rate(double d, const XlParams& p) {
  if (TYPE == MHIP_SPRING_HOOKEAN) return p.A * exp(-0.5 * p.inv_kt * p.k * (d - p.r) * (d - p.r));
  return d < p.r ? p.A * pow(1.0 - (d / p.r) * (d / p.r), 0.5 * p.inv_kt * p.k * p.r * p.r) : 0.0;
}

// ---- candidate rows: sorted by original body id when the list is built ---------------------------------------------
__global__ void __launch_bounds__(kBlock) k_xl_entry_keys(size_t entries, const int32_t* __restrict__ col,
                                                         const int64_t* __restrict__ ids, int64_t* __restrict__ key) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < entries; e += (size_t)gridDim.x * blockDim.x)
    key[e] = ids ? ids[col[e]] : static_cast<int64_t>(col[e]);
}
// one row per lane, insertion sort of (key, col): rows hold the bind sites within reach of one bead (tens)
__global__ void __launch_bounds__(kBlock) k_xl_row_sort(size_t n, const int32_t* __restrict__ ptr,
                                                       int64_t* __restrict__ key, int32_t* __restrict__ col) {
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    for (int32_t a = lo + 1; a < hi; ++a) {
      const int64_t kv = key[a];
      const int32_t cv = col[a];
      int32_t j = a - 1;
      while (j >= lo && (key[j] > kv || (key[j] == kv && col[j] > cv))) {
        key[j + 1] = key[j];
        col[j + 1] = col[j];
        --j;
      }
      key[j + 1] = kv;
      col[j + 1] = cv;
    }
  }
}

// ---- KMC: one lane per crosslinker ---------------------------------------------------------------------------------
// u = philox_u53 2^-53 in [0, 1) from block 0 at (key, counter); the counter advances whatever the state
// (HP1.cpp:3487-3491, :3560-3565).  Every lane reads and writes the state of its own crosslinker only and the rates do
// not depend on the other crosslinkers (no site exclusivity in the reference), so sampling from the state at the start
// of the step and applying afterwards (:3757-3764) is what the in-place update computes.
__device__ __forceinline__ double xl_draw(const uint64_t* __restrict__ keys, uint64_t* __restrict__ ctrs, size_t c) {
  const uint64_t ctr = ctrs[c];
  const uint4 w = philox_draw(keys[c], ctr, 0u);
  ctrs[c] = ctr + 1;
  return static_cast<double>(philox_u53(w)) * 0x1p-53;
}

// One candidate row of a left bead: entries col[lo .. hi), the positions the columns index and the constants that rate
// them.  The bead row (SITE = false) holds body indices and never follows `skip`, the left bead itself (the self site,
// HP1.cpp:3298-3306); the site row holds site indices and never follows a column outside [0, skip = P).
template <bool SITE>
struct XlRow {
  int32_t lo, hi;
  const int32_t* col;
  const double* pos;
  const XlParams& p;
  int32_t skip;
};
// f(column, rate) for every entry of the row that can be bound to, in row order, until f returns true
template <int TYPE, bool SITE, class F>
__device__ __forceinline__ void xl_row_walk(const XlRow<SITE>& row, V3 xl, F&& f) {
  for (int32_t e = row.lo; e < row.hi; ++e) {
    const int32_t s = row.col[e];
    if (SITE ? static_cast<uint32_t>(s) >= static_cast<uint32_t>(row.skip) : s == row.skip) continue;
    const double d = norm(load3(row.pos, s) - xl);
    if (!(d <= row.p.cap)) continue;  // beyond the capture radius: rate 0 exactly, whatever the list still holds
    if (f(s, xl_rate<TYPE>(d, row.p))) break;
  }
}
// the running sum z of dt rate, continued over the row
template <int TYPE, bool SITE>
__device__ __forceinline__ double xl_row_total(const XlRow<SITE>& row, V3 xl, double dt, double z) {
  xl_row_walk<TYPE>(row, xl, [&](int32_t, double rate) {
    z += dt * rate;
    return false;
  });
  return z;
}
// the running sum of scale rate, continued over the row: the first column at which it exceeds u (HP1.cpp:3518-3527), -1
// where none does
template <int TYPE, bool SITE>
__device__ __forceinline__ int32_t xl_row_pick(const XlRow<SITE>& row, V3 xl, double scale, double u, double& cumsum) {
  int32_t chosen = -1;
  xl_row_walk<TYPE>(row, xl, [&](int32_t s, double rate) {
    cumsum += scale * rate;
    if (u < cumsum) chosen = s;
    return chosen >= 0;
  });
  return chosen;
}

// The periphery's bind sites as the KMC lane sees them: the second candidate row of every bead (ptr [n + 1], col: site
// indices, ascending), the P site positions, the sites' own (k, r, A, k_off, 1 / kT, capture radius), and where the
// number of periphery-bound crosslinkers after the step is added (null: nowhere).
struct XlSites {
  const int32_t* ptr;
  const int32_t* col;
  const double* center;
  uint32_t count;
  XlParams p;
  int* bound;
};

// What one lane does for crosslinker c.  Doubly bound, to a bead or (right < 0) to a site: it unbinds at the rate
// constant of what it is bound to (what HP1.cpp:3554-3573 reduces to).  Singly bound: z_tot over the bead row, then
// (SITES) on over the site row; with u < 1 - exp(-z_tot) the second pass over the same rows picks the column.
// -> what happened, for the launch's counts: kXlBound / kXlUnbound, and kXlAtWall where it ends the step on a site
// (returned and counted by the kernel: counters handed in by reference, the compiler kept in scratch).
enum : int { kXlBound = 1, kXlUnbound = 2, kXlAtWall = 4 };
template <int TYPE, bool SITES>
__device__ __forceinline__ int xl_kmc_one(size_t c, const int32_t* __restrict__ left, int32_t* __restrict__ right,
                                          const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                                          const double* __restrict__ center, const uint64_t* __restrict__ keys,
                                          uint64_t* __restrict__ ctrs, const XlParams& p, double dt,
                                          double* __restrict__ z_out, [[maybe_unused]] const XlSites& ps) {
  const double u = xl_draw(keys, ctrs, c);
  const int32_t l = left[c];
  const int32_t r0 = right[c];
  if (r0 != l) {
    bool on_site = false;
    if constexpr (SITES) on_site = r0 < 0;
    const bool unbinds = u < 1.0 - exp(-(dt * (on_site ? ps.p.k_off : p.k_off)));
    if (unbinds) right[c] = l;
    if (z_out) z_out[c] = 0.0;
    return unbinds ? kXlUnbound : on_site ? kXlAtWall : 0;
  }
  const V3 xl = load3(center, l);
  const XlRow<false> beads{ptr[l], ptr[l + 1], col, center, p, l};
  const XlRow<true> sites{SITES ? ps.ptr[l] : 0, SITES ? ps.ptr[l + 1] : 0, ps.col, ps.center, ps.p,
                          static_cast<int32_t>(ps.count)};  // (without SITES: never walked)
  double z_tot = xl_row_total<TYPE>(beads, xl, dt, 0.0);
  if constexpr (SITES) z_tot = xl_row_total<TYPE>(sites, xl, dt, z_tot);
  if (z_out) z_out[c] = z_tot;
  const double p_bind = 1.0 - exp(-z_tot);
  if (!(u < p_bind)) return 0;  // (z_tot = 0: p_bind = 0, never)
  const double scale = p_bind * dt / z_tot;
  double cumsum = 0.0;
  int32_t s = xl_row_pick<TYPE>(beads, xl, scale, u, cumsum);
  if (s >= 0) {
    right[c] = s;
    return kXlBound;
  }
  if constexpr (SITES) {
    s = xl_row_pick<TYPE>(sites, xl, scale, u, cumsum);
    if (s >= 0) {
      right[c] = -(s + 1);
      return kXlBound | kXlAtWall;
    }
  }
  return 0;
}

// The two entry points keep the grid-stride loop and their argument lists: with the loop in the shared function, or one
// argument list for both, the compiler groups the scalar loads of the kernel without sites differently.
template <int TYPE>
__global__ void __launch_bounds__(kBlock)
    k_xl_kmc(size_t m, const int32_t* __restrict__ left, int32_t* __restrict__ right, const int32_t* __restrict__ ptr,
             const int32_t* __restrict__ col, const double* __restrict__ center, const uint64_t* __restrict__ keys,
             uint64_t* __restrict__ ctrs, XlParams p, double dt, int* __restrict__ events,
             double* __restrict__ z_out) {
  int binds = 0, unbinds = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < m; c += (size_t)gridDim.x * blockDim.x) {
    const int what = xl_kmc_one<TYPE, false>(c, left, right, ptr, col, center, keys, ctrs, p, dt, z_out, XlSites{});
    binds += (what & kXlBound) != 0;
    unbinds += (what & kXlUnbound) != 0;
  }
  wave_stat_add(binds, &events[0]);
  wave_stat_add(unbinds, &events[1]);
}
template <int TYPE>
__global__ void __launch_bounds__(kBlock)
    k_xl_kmc_periphery(size_t m, const int32_t* __restrict__ left, int32_t* __restrict__ right,
                       const int32_t* __restrict__ ptr, const int32_t* __restrict__ col,
                       const double* __restrict__ center, const uint64_t* __restrict__ keys,
                       uint64_t* __restrict__ ctrs, XlParams p, double dt, int* __restrict__ events,
                       double* __restrict__ z_out, XlSites ps) {
  int binds = 0, unbinds = 0, at_wall = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < m; c += (size_t)gridDim.x * blockDim.x) {
    const int what = xl_kmc_one<TYPE, true>(c, left, right, ptr, col, center, keys, ctrs, p, dt, z_out, ps);
    binds += (what & kXlBound) != 0;
    unbinds += (what & kXlUnbound) != 0;
    at_wall += (what & kXlAtWall) != 0;
  }
  wave_stat_add(binds, &events[0]);
  wave_stat_add(unbinds, &events[1]);
  wave_stat_add(at_wall, ps.bound);  // one atomic per wave, none for 0 or a null counter
}

// a periphery-bound head (SITES, right < 0) keeps its value -- the sites are not bodies -- and never indexes new_of_old
template <bool SITES>
__global__ void __launch_bounds__(kBlock) k_xl_renumber(size_t m, const int32_t* __restrict__ new_of_old,
                                                       int32_t* __restrict__ left, int32_t* __restrict__ right) {
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < m; c += (size_t)gridDim.x * blockDim.x) {
    left[c] = new_of_old[left[c]];
    const int32_t r = right[c];
    if (!SITES || r >= 0) right[c] = new_of_old[r];
  }
}

// ---- the periphery's candidate rows: site index = column - col_offset, every row ascending ---------------------------
__global__ void __launch_bounds__(kBlock) k_xl_site_cols(size_t entries, const int32_t* __restrict__ col_in,
                                                        int32_t col_offset, int32_t* __restrict__ col,
                                                        int64_t* __restrict__ key) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < entries; e += (size_t)gridDim.x * blockDim.x) {
    const int32_t s = col_in[e] - col_offset;
    col[e] = s;
    key[e] = s;
  }
}

// ---- force: one body per lane ----------------------------------------------------------------------------------------
// The body's left list (crosslinkers anchored here, doubly bound or not) and right list (doubly bound ones whose right
// head sits here) are merged in ascending crosslinker index.  A doubly bound crosslinker is the spring (left, right) of
// mhip_springs_force: d = x_right - x_left, L, fm and fm d in the same operations at both ends, + at the left end and -
// at the right, summed from +0.0.  Its statistics are taken at the left end only.
// SITES: a crosslinker of the left list with right == -(s + 1) is the spring between x_left and the site y_s, the same
// term at its place in the merge, added to the left bead only (the site receives nothing: nothing ever moves it).
template <int TYPE, bool ACCUMULATE, bool SITES>
__device__ __forceinline__ void xl_force(size_t first, size_t stride, size_t n, const int32_t* __restrict__ lptr,
                                         const int32_t* __restrict__ lent, const int32_t* __restrict__ rptr,
                                         const int32_t* __restrict__ rent, const int32_t* __restrict__ left,
                                         const int32_t* __restrict__ right, const double* __restrict__ center,
                                         double k, double r, double* __restrict__ force,
                                         int* __restrict__ overstretched,
                                         unsigned long long* __restrict__ max_length_bits,
                                         [[maybe_unused]] const double* __restrict__ site) {
  double lmax = 0.0;
  for (size_t b = first; b < n; b += stride) {
    V3 f{0.0, 0.0, 0.0};
    int32_t a = lptr[b], e = rptr[b];
    const int32_t ae = lptr[b + 1], ee = rptr[b + 1];
    while (a < ae || e < ee) {
      const int32_t ca = a < ae ? lent[a] : 0x7fffffff;
      const int32_t ce = e < ee ? rent[e] : 0x7fffffff;
      const bool at_left = ca < ce;  // (never equal: a crosslinker in the right list has right != left)
      const int32_t c = at_left ? ca : ce;
      if (at_left) ++a;
      else ++e;
      const int32_t i = at_left ? static_cast<int32_t>(b) : left[c];
      const int32_t j = at_left ? right[c] : static_cast<int32_t>(b);
      if (i == j) continue;  // singly bound: no force
      V3 d;
      if constexpr (SITES) d = (j < 0 ? load3(site, -(j + 1)) : load3(center, j)) - load3(center, i);
      else d = load3(center, j) - load3(center, i);
      const SpringTerm t = spring_term<TYPE>(d, k, r);
      if (TYPE == MHIP_SPRING_FENE && at_left && !(t.L < r)) atomicAdd(overstretched, 1);
      if (at_left) lmax = t.L > lmax ? t.L : lmax;
      add_term(f, !at_left, t.fm, d);
    }
    write_force<ACCUMULATE>(force, b, f);
  }
  block_stat_max(lmax, max_length_bits);
}

template <int TYPE, bool ACCUMULATE>
__global__ void __launch_bounds__(kBlock)
    k_xl_force(size_t n, const int32_t* __restrict__ lptr, const int32_t* __restrict__ lent,
               const int32_t* __restrict__ rptr, const int32_t* __restrict__ rent, const int32_t* __restrict__ left,
               const int32_t* __restrict__ right, const double* __restrict__ center, double k, double r,
               double* __restrict__ force, int* __restrict__ overstretched,
               unsigned long long* __restrict__ max_length_bits) {
  xl_force<TYPE, ACCUMULATE, false>(blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, n,
                                    lptr, lent, rptr, rent, left, right, center, k, r, force, overstretched,
                                    max_length_bits, nullptr);
}
template <int TYPE, bool ACCUMULATE>
__global__ void __launch_bounds__(kBlock)
    k_xl_force_periphery(size_t n, const int32_t* __restrict__ lptr, const int32_t* __restrict__ lent,
                         const int32_t* __restrict__ rptr, const int32_t* __restrict__ rent,
                         const int32_t* __restrict__ left, const int32_t* __restrict__ right,
                         const double* __restrict__ center, double k, double r, double* __restrict__ force,
                         int* __restrict__ overstretched, unsigned long long* __restrict__ max_length_bits,
                         const double* __restrict__ site) {
  xl_force<TYPE, ACCUMULATE, true>(blockIdx.x * (size_t)blockDim.x + threadIdx.x, (size_t)gridDim.x * blockDim.x, n,
                                   lptr, lent, rptr, rent, left, right, center, k, r, force, overstretched,
                                   max_length_bits, site);
}

}  // namespace mhip

using namespace mhip;

struct mhip_crosslinkers {
  size_t n = 0, m = 0;
  int type = MHIP_SPRING_HOOKEAN;
  XlParams p{};
  HandleBuffer left, right, lptr, lent, rptr, rent, cursor, ws;
  struct Candidates {  // the rows of every bead, sorted; valid: set since the last event that outdates them
    HandleBuffer ptr, col, key;
    bool valid = false;
  } beads, sites;
  // periphery bind sites (mundy_hip_periphery_binding.h): positions, their own constants (their rows: `sites`)
  HandleBuffer site;
  size_t num_sites = 0;
  XlParams pp{};
  bool has_sites = false;
};

namespace {

// The five constants of one kind of bind site, refused in each caller's words: `spring` goes before the spring's two
// ("crosslinker " / "periphery "), `rate` before the other three ("" / "periphery "), r is called r_name and must be
// > 0 (r_positive) or >= 0.
int check_constants(const char* spring, const char* rate, const char* r_name, bool r_positive, double k, double r,
                    double bind_rate, double unbind_rate, double capture_radius) {
  MHIP_REQUIRE(std::isfinite(k) && k >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "%sspring constant k must be finite and >= 0, got %g", spring, k);
  MHIP_REQUIRE(std::isfinite(r) && (r_positive ? r > 0.0 : r >= 0.0), MHIP_ERR_INVALID_ARGUMENT,
               "%s%s must be finite and %s 0, got %g", spring, r_name, r_positive ? ">" : ">=", r);
  MHIP_REQUIRE(std::isfinite(bind_rate) && bind_rate >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "%sbind_rate must be finite and >= 0, got %g", rate, bind_rate);
  MHIP_REQUIRE(std::isfinite(unbind_rate) && unbind_rate >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "%sunbind_rate must be finite and >= 0, got %g", rate, unbind_rate);
  MHIP_REQUIRE(std::isfinite(capture_radius) && capture_radius > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "%scapture_radius must be finite and > 0, got %g", rate, capture_radius);
  return MHIP_SUCCESS;
}

// the crosslinkers listed at their left ends, and at their right ends where doubly bound
int build_left(mhip_crosslinkers* h, hipStream_t s) {
  return build_incidence(h->n, h->m, ListedAt{h->left.as<int32_t>(), nullptr}, h->cursor.as<int32_t>(),
                         h->lptr.as<int32_t>(), h->lent.as<int32_t>(), h->ws.ptr, s);
}
int build_right(mhip_crosslinkers* h, hipStream_t s) {  // (a periphery-bound head is listed at no body)
  return build_incidence(h->n, h->m, ListedAtBody{h->right.as<int32_t>(), h->left.as<int32_t>()},
                         h->cursor.as<int32_t>(), h->rptr.as<int32_t>(), h->rent.as<int32_t>(), h->ws.ptr, s);
}

// The first n rows of a device CSR become the handle's bead rows (sites = false: columns are bodies, sorted by ids, or
// by index where ids is null) or its periphery rows (columns - col_offset are sites, sorted by index).
int set_candidates(mhip_crosslinkers* h, bool sites, const int32_t* row_ptr, const int32_t* col, size_t num_entries,
                   const int64_t* ids, int32_t col_offset, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(row_ptr != nullptr, MHIP_ERR_INVALID_ARGUMENT, "row_ptr is null");
  MHIP_REQUIRE(num_entries == 0 || col, MHIP_ERR_INVALID_ARGUMENT, "col is null");
  MHIP_REQUIRE(num_entries < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many candidates for a 32-bit row_ptr");
  MHIP_REQUIRE(!sites || h->has_sites, MHIP_ERR_RUNTIME, "mhip_crosslinkers_set_periphery_sites has not been called");
  hipStream_t s = as_stream(stream);
  mhip_crosslinkers::Candidates& c = sites ? h->sites : h->beads;
  c.valid = false;
  if (int e = c.ptr.reserve((h->n + 1) * sizeof(int32_t))) return e;
  if (int e = c.col.reserve(num_entries * sizeof(int32_t) + 8)) return e;
  if (int e = c.key.reserve(num_entries * sizeof(int64_t) + 8)) return e;
  MHIP_HIP(hipMemcpyAsync(c.ptr.ptr, row_ptr, (h->n + 1) * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (num_entries > 0) {
    if (sites) {
      k_xl_site_cols<<<grid_for(num_entries), kBlock, 0, s>>>(num_entries, col, col_offset, c.col.as<int32_t>(),
                                                             c.key.as<int64_t>());
    } else {
      MHIP_HIP(hipMemcpyAsync(c.col.ptr, col, num_entries * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
      k_xl_entry_keys<<<grid_for(num_entries), kBlock, 0, s>>>(num_entries, c.col.as<int32_t>(), ids,
                                                              c.key.as<int64_t>());
    }
    MHIP_LAUNCH_CHECK();
    k_xl_row_sort<<<grid_for(h->n), kBlock, 0, s>>>(h->n, c.ptr.as<int32_t>(), c.key.as<int64_t>(), c.col.as<int32_t>());
    MHIP_LAUNCH_CHECK();
  }
  c.valid = true;
  return MHIP_SUCCESS;
}

// one KMC step: mhip_crosslinkers_kmc_step and, with the periphery's rows, mhip_crosslinkers_kmc_step_periphery
int kmc_step(mhip_crosslinkers* h, const double* center, double dt, const uint64_t* keys, uint64_t* counters,
             int* events, int* periphery_bound, double* z_total, bool need_sites, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt > 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and > 0, got %g", dt);
  MHIP_REQUIRE(events != nullptr, MHIP_ERR_INVALID_ARGUMENT, "events is null");
  MHIP_REQUIRE(h->m == 0 || (center && keys && counters), MHIP_ERR_INVALID_ARGUMENT,
               "center / keys / counters is null");
  MHIP_REQUIRE(h->beads.valid, MHIP_ERR_RUNTIME,
               "mhip_crosslinkers_set_candidates has not been called since the handle was created or renumbered");
  MHIP_REQUIRE(h->sites.valid || !(need_sites || h->has_sites), MHIP_ERR_RUNTIME,
               "mhip_crosslinkers_set_periphery_candidates has not been called since the sites were set or the handle "
               "was renumbered");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(events, 0, 2 * sizeof(int), s));
  if (h->m == 0) return MHIP_SUCCESS;
  const unsigned grid = grid_for(h->m);
  if (h->has_sites) {
    const XlSites ps{h->sites.ptr.as<int32_t>(), h->sites.col.as<int32_t>(), h->site.as<double>(),
                     static_cast<uint32_t>(h->num_sites), h->pp, periphery_bound};
    dispatch<MHIP_SPRING_FENE, MHIP_SPRING_HOOKEAN>(h->type, [&](auto type) {
      k_xl_kmc_periphery<decltype(type)::value><<<grid, kBlock, 0, s>>>(
          h->m, h->left.as<int32_t>(), h->right.as<int32_t>(), h->beads.ptr.as<int32_t>(), h->beads.col.as<int32_t>(),
          center, keys, counters, h->p, dt, events, z_total, ps);
    });
  } else {
    dispatch<MHIP_SPRING_FENE, MHIP_SPRING_HOOKEAN>(h->type, [&](auto type) {
      k_xl_kmc<decltype(type)::value><<<grid, kBlock, 0, s>>>(
          h->m, h->left.as<int32_t>(), h->right.as<int32_t>(), h->beads.ptr.as<int32_t>(), h->beads.col.as<int32_t>(),
          center, keys, counters, h->p, dt, events, z_total);
    });
  }
  MHIP_LAUNCH_CHECK();
  // the right ends moved (or not: the rebuild is cheaper than a host round trip to find out)
  return build_right(h, s);
}

}  // namespace

extern "C" {

int mhip_crosslinkers_create(mhip_crosslinkers_t* handle, size_t n, size_t m, const int32_t* left, const int32_t* right,
                             const unsigned char* is_site, int type, double k, double r, double bind_rate,
                             double unbind_rate, double kt, double capture_radius, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(type != MHIP_SPRING_FENEWCA, MHIP_ERR_INVALID_ARGUMENT,
               "crosslinkers take no FENE-WCA springs: the reference's binding rates have no such branch");
  MHIP_REQUIRE(type == MHIP_SPRING_HOOKEAN || type == MHIP_SPRING_FENE, MHIP_ERR_INVALID_ARGUMENT,
               "unknown spring type %d", type);
  MHIP_REQUIRE(m == 0 || left, MHIP_ERR_INVALID_ARGUMENT, "left is null");
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit crosslinker heads");
  MHIP_REQUIRE(m < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many crosslinkers for 32-bit incidence entries");
  const bool fene = type == MHIP_SPRING_FENE;
  if (int e = check_constants("crosslinker ", "", fene ? "r_max" : "rest length", fene, k, r, bind_rate, unbind_rate,
                              capture_radius))
    return e;
  MHIP_REQUIRE(std::isfinite(kt) && kt > 0.0, MHIP_ERR_INVALID_ARGUMENT, "kt must be finite and > 0, got %g", kt);
  // host arrays: every crosslinker is checked here, before anything reaches the device
  for (size_t c = 0; c < m; ++c) {
    const int32_t l = left[c], rr = right ? right[c] : l;
    MHIP_REQUIRE(l >= 0 && static_cast<size_t>(l) < n, MHIP_ERR_INVALID_ARGUMENT,
                 "crosslinker %zu: left head at %d, an index outside [0, %zu)", c, l, n);
    MHIP_REQUIRE(rr >= 0 && static_cast<size_t>(rr) < n, MHIP_ERR_INVALID_ARGUMENT,
                 "crosslinker %zu: right head at %d, an index outside [0, %zu)", c, rr, n);
    MHIP_REQUIRE(rr == l || !is_site || is_site[rr], MHIP_ERR_INVALID_ARGUMENT,
                 "crosslinker %zu: right head at body %d, which is not a bind site", c, rr);
  }
  auto h = std::make_unique<mhip_crosslinkers>();
  h->n = n;
  h->m = m;
  h->type = type;
  h->p = XlParams{k, r, bind_rate, unbind_rate, 1.0 / kt, capture_radius};
  hipStream_t s = as_stream(stream);
  int e = MHIP_SUCCESS;
  if ((e = h->left.reserve(m * sizeof(int32_t) + 8)) || (e = h->right.reserve(m * sizeof(int32_t) + 8)) ||
      (e = h->lent.reserve(m * sizeof(int32_t) + 8)) || (e = h->rent.reserve(m * sizeof(int32_t) + 8)) ||
      (e = h->lptr.reserve((n + 1) * sizeof(int32_t))) || (e = h->rptr.reserve((n + 1) * sizeof(int32_t))) ||
      (e = h->cursor.reserve((n + 1) * sizeof(int32_t))) || (e = h->ws.reserve(scan_workspace_bytes(n) + 8)))
    return e;
  if (m > 0) {
    if ((e = upload(__func__, h->left, left, m * sizeof(int32_t), s))) return e;
    if ((e = upload(__func__, h->right, right ? right : left, m * sizeof(int32_t), s))) return e;
  }
  if ((e = build_left(h.get(), s)) || (e = build_right(h.get(), s))) return e;
  // the caller's host arrays may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_crosslinkers_destroy(mhip_crosslinkers_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_crosslinkers_set_candidates(mhip_crosslinkers_t h, const int32_t* row_ptr, const int32_t* col,
                                     size_t num_entries, const int64_t* ids, mhip_stream_t stream) {
  return set_candidates(h, false, row_ptr, col, num_entries, ids, 0, stream);
}

int mhip_crosslinkers_kmc_step(mhip_crosslinkers_t h, const double* center, double dt, const uint64_t* keys,
                               uint64_t* counters, int* events, double* z_total, mhip_stream_t stream) {
  return kmc_step(h, center, dt, keys, counters, events, nullptr, z_total, false, stream);
}

int mhip_crosslinkers_kmc_step_periphery(mhip_crosslinkers_t h, const double* center, double dt, const uint64_t* keys,
                                         uint64_t* counters, int* events, int* periphery_bound, double* z_total,
                                         mhip_stream_t stream) {
  return kmc_step(h, center, dt, keys, counters, events, periphery_bound, z_total, true, stream);
}

int mhip_crosslinkers_set_periphery_sites(mhip_crosslinkers_t h, size_t P, const double* site_center, double bind_rate,
                                          double k, double r, double unbind_rate, double capture_radius,
                                          mhip_stream_t stream) {
  // what needs no handle first, so that every refusal can be checked without a device
  MHIP_REQUIRE(P > 0, MHIP_ERR_INVALID_ARGUMENT, "periphery sites: P must be > 0");
  MHIP_REQUIRE(P < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many periphery sites for a 32-bit right head");
  if (int e = check_constants("periphery ", "periphery ", "rest length / r_max", false, k, r, bind_rate, unbind_rate,
                              capture_radius))
    return e;
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(site_center != nullptr, MHIP_ERR_INVALID_ARGUMENT, "site_center is null");
  MHIP_REQUIRE(h->type != MHIP_SPRING_FENE || r > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "periphery r_max must be > 0 for FENE crosslinkers, got %g", r);
  MHIP_REQUIRE(!h->has_sites || P == h->num_sites, MHIP_ERR_INVALID_ARGUMENT,
               "periphery sites: P = %zu, but an earlier call set %zu sites", P, h->num_sites);
  hipStream_t s = as_stream(stream);
  h->sites.valid = false;
  if (int e = h->site.reserve(P * 3 * sizeof(double))) return e;
  MHIP_HIP(hipMemcpyAsync(h->site.ptr, site_center, P * 3 * sizeof(double), hipMemcpyDeviceToDevice, s));
  h->num_sites = P;
  h->pp = XlParams{k, r, bind_rate, unbind_rate, h->p.inv_kt, capture_radius};
  h->has_sites = true;
  return MHIP_SUCCESS;
}

int mhip_crosslinkers_set_periphery_candidates(mhip_crosslinkers_t h, const int32_t* row_ptr, const int32_t* col,
                                               size_t num_entries, int32_t col_offset, mhip_stream_t stream) {
  return set_candidates(h, true, row_ptr, col, num_entries, nullptr, col_offset, stream);
}

int mhip_crosslinkers_force(mhip_crosslinkers_t h, const double* center, double* force, int accumulate,
                            int* overstretched, double* max_length, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(overstretched != nullptr && max_length != nullptr, MHIP_ERR_INVALID_ARGUMENT,
               "overstretched / max_length is null");
  MHIP_REQUIRE(h->n == 0 || (center && force), MHIP_ERR_INVALID_ARGUMENT, "center / force is null");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(overstretched, 0, sizeof(int), s));
  MHIP_HIP(hipMemsetAsync(max_length, 0, sizeof(double), s));  // +0.0: also the answer without a doubly bound one
  if (h->n == 0) return MHIP_SUCCESS;
  const unsigned grid = grid_for(h->n);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(max_length);
  dispatch<MHIP_SPRING_FENE, MHIP_SPRING_HOOKEAN>(h->type, [&](auto type) {
    dispatch<true, false>(accumulate != 0, [&](auto acc) {
      if (h->has_sites)
        k_xl_force_periphery<decltype(type)::value, decltype(acc)::value><<<grid, kBlock, 0, s>>>(
            h->n, h->lptr.as<int32_t>(), h->lent.as<int32_t>(), h->rptr.as<int32_t>(), h->rent.as<int32_t>(),
            h->left.as<int32_t>(), h->right.as<int32_t>(), center, h->p.k, h->p.r, force, overstretched, mx,
            h->site.as<double>());
      else
        k_xl_force<decltype(type)::value, decltype(acc)::value><<<grid, kBlock, 0, s>>>(
            h->n, h->lptr.as<int32_t>(), h->lent.as<int32_t>(), h->rptr.as<int32_t>(), h->rent.as<int32_t>(),
            h->left.as<int32_t>(), h->right.as<int32_t>(), center, h->p.k, h->p.r, force, overstretched, mx);
    });
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_crosslinkers_get_state(mhip_crosslinkers_t h, int32_t* left, int32_t* right, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  hipStream_t s = as_stream(stream);
  if (h->m == 0) return MHIP_SUCCESS;
  if (left) MHIP_HIP(hipMemcpyAsync(left, h->left.ptr, h->m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (right) MHIP_HIP(hipMemcpyAsync(right, h->right.ptr, h->m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return MHIP_SUCCESS;
}

int mhip_crosslinkers_set_state(mhip_crosslinkers_t h, const int32_t* left, const int32_t* right,
                                mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(h->m == 0 || right, MHIP_ERR_INVALID_ARGUMENT, "right is null");
  hipStream_t s = as_stream(stream);
  if (h->m == 0) return MHIP_SUCCESS;
  if (left) {
    MHIP_HIP(hipMemcpyAsync(h->left.ptr, left, h->m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (int e = build_left(h, s)) return e;
  }
  MHIP_HIP(hipMemcpyAsync(h->right.ptr, right, h->m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  return build_right(h, s);
}

int mhip_crosslinkers_renumber(mhip_crosslinkers_t h, const int32_t* new_of_old, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "crosslinkers handle is null");
  MHIP_REQUIRE(h->n == 0 || new_of_old, MHIP_ERR_INVALID_ARGUMENT, "new_of_old is null");
  hipStream_t s = as_stream(stream);
  h->beads.valid = false;  // the candidate rows are in the old numbering
  h->sites.valid = false;
  if (h->m > 0) {
    dispatch<true, false>(h->has_sites, [&](auto sites) {
      k_xl_renumber<decltype(sites)::value><<<grid_for(h->m), kBlock, 0, s>>>(h->m, new_of_old, h->left.as<int32_t>(),
                                                                             h->right.as<int32_t>());
    });
    MHIP_LAUNCH_CHECK();
  }
  if (int e = build_left(h, s)) return e;
  return build_right(h, s);
}

}  // extern "C"
