// hertz_friction.hip -- the reference's frictional Hertzian rod contact, per linker, and the carry of its per-pair
// history across neighbour-list rebuilds and body renumberings
// (scrap/parameter_interface/linkers/src/mundy_linkers/evaluate_linker_potentials/kernels/
//  SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:384-518, run every step by
//  CollidingOverdampedFrictionalSperm.cpp:1553-1731).
// Per contact: pair and signed separation are read; only a pair in the contact branch (sep <= 0, or NaN: the reference
// tests `sep > 0`) gathers its normal, arclengths, the two bodies' previous velocity rows, axes, radii and materials and
// its history row.  A pair out of contact owns two +0.0 rows (history, force); they are read and only written where
// they are not +0.0 already, so a list whose separated pairs stay separated is never written there.
#include "mhip_internal.hpp"
#include "force_device.hpp"
#include "scratch_owner.hpp"

#include <cmath>

namespace mhip {


// velocity of the contact point of a rigid rod: U + W x ((s - 1/2)(p1 - p0)) -- the arm of the rod-compressed operator
// (get_contact_point_velocity, :357-380, for a rod whose nodes move rigidly; the twist is dropped there too)
__device__ inline V3 contact_point_velocity(const double* __restrict__ vel, const double* __restrict__ seg, int b,
                                            double arc) {
  const double* v = vel + 6 * (size_t)b;
  const double* r = seg + 8 * (size_t)b;
  const V3 axis = V3{r[3], r[4], r[5]} - V3{r[0], r[1], r[2]};
  const V3 arm = rod_arm_coef(arc) * axis;
  return V3{v[0], v[1], v[2]} + cross(V3{v[3], v[4], v[5]}, arm);
}

// One contact per lane and pass, grid-stride.  stats[0]: bits of max(0, -sep) (atomic max, as k_hertz_force);
// stats[1]: number of contacts whose tangential force was capped.  One atomic per workgroup for each.
template <bool E_ARRAY, bool NU_ARRAY>
__global__ void __launch_bounds__(kBlock)
    k_hertz_friction_force(size_t C, size_t N, const int2* __restrict__ pairs, const double* __restrict__ sep,
                           const double* __restrict__ normal, const double* __restrict__ arc_s,
                           const double* __restrict__ arc_t, const double* __restrict__ seg,
                           const double* __restrict__ radius, const double* __restrict__ E, double E0,
                           const double* __restrict__ nu, double nu0, const double* __restrict__ vel_prev,
                           mhip_hertz_friction_params prm, double* __restrict__ tang_disp, double* __restrict__ force,
                           unsigned long long* __restrict__ stats) {
  double dmax = 0.0;
  unsigned capped = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < C; c += (size_t)gridDim.x * blockDim.x) {
    const int2 p = pairs[c];
    const double s = sep[c];
    if (static_cast<unsigned>(p.x) >= N || static_cast<unsigned>(p.y) >= N) {  // never dereferenced
      const double q = __builtin_nan("");
      store3(tang_disp, c, V3{q, q, q});
      store3(force, c, V3{q, q, q});
      continue;
    }
    if (s > 0.0) {  // no contact: the history is reset (:433-435), the force is +0.0
      if (!row_is_pos_zero(tang_disp, c)) store3(tang_disp, c, V3{0.0, 0.0, 0.0});
      if (!row_is_pos_zero(force, c)) store3(force, c, V3{0.0, 0.0, 0.0});
      continue;
    }
    const V3 n = load3(normal, c);
    const V3 vi = contact_point_velocity(vel_prev, seg, p.x, arc_s[c]);
    const V3 vj = contact_point_velocity(vel_prev, seg, p.y, arc_t[c]);
    const V3 rel = vj - vi;                                                           // :468
    const HertzPair h = hertz_pair<E_ARRAY, NU_ARRAY>(p, radius, E, E0, nu, nu0);
    const FrictionContact r = hertz_friction_law(rel, n, s, h, prm, load3(tang_disp, c));
    capped += r.capped ? 1u : 0u;
    store3(tang_disp, c, r.td);
    store3(force, c, r.force);  // on body i; body j receives the negative
    dmax = -s > dmax ? -s : dmax;
  }
  block_stat_max(dmax, stats);
  block_stat_add(capped, stats + 1);
}

// ---- history carry ---------------------------------------------------------------------------------------------------
constexpr unsigned long long kNoKey = ~0ull;
constexpr unsigned kFlipBit = 0x80000000u;

// key of an old pair in the new numbering: (min << 32) | max of its renumbered endpoints; value = its row, bit 31 set
// when the renumbering swapped the orientation.  A pair with an endpoint outside [0, n_old), a negative image (the body
// is gone) or both endpoints on one body carries nothing.  Without a renumbering the keys are searched as they stand:
// *disorder is set where they do not ascend strictly (a list that is not canonical, or holds a pair without a key).
__global__ void __launch_bounds__(kBlock)
    k_history_keys(size_t c_old, const int2* __restrict__ pairs_old, const int32_t* __restrict__ new_of_old,
                   size_t n_old, unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                   unsigned long long* __restrict__ disorder) {
  for (size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x; k < c_old; k += (size_t)gridDim.x * blockDim.x) {
    const int2 p = pairs_old[k];
    if (new_of_old == nullptr) {
      bool bad = p.x < 0 || p.y < 0 || p.x >= p.y;
      if (k > 0) {  // (i, j) ascending lexicographically
        const int2 q = pairs_old[k - 1];
        bad = bad || q.x > p.x || (q.x == p.x && q.y >= p.y);
      }
      if (bad) atomicOr(disorder, 1ull);  // (never taken on a canonical list: no contention)
    }
    int a = p.x, b = p.y;
    bool ok = a >= 0 && b >= 0;
    if (new_of_old != nullptr) {
      ok = ok && static_cast<size_t>(a) < n_old && static_cast<size_t>(b) < n_old;
      a = ok ? new_of_old[a] : -1;
      b = ok ? new_of_old[b] : -1;
      ok = ok && a >= 0 && b >= 0;
    }
    ok = ok && a != b;
    const bool flip = a > b;
    const unsigned lo = static_cast<unsigned>(flip ? b : a), hi = static_cast<unsigned>(flip ? a : b);
    keys[k] = ok ? (static_cast<unsigned long long>(lo) << 32) | hi : kNoKey;
    vals[k] = static_cast<unsigned>(k) | (flip ? kFlipBit : 0u);
  }
}

// one binary search per new pair over the sorted keys
__global__ void __launch_bounds__(kBlock)
    k_history_carry(size_t c_old, const unsigned long long* __restrict__ keys, const unsigned* __restrict__ vals,
                    const double* __restrict__ hist_old, size_t c_new, const int2* __restrict__ pairs_new,
                    double* __restrict__ hist_new, unsigned long long* __restrict__ carried) {
  unsigned found = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < c_new; c += (size_t)gridDim.x * blockDim.x) {
    const int2 p = pairs_new[c];
    V3 h{0.0, 0.0, 0.0};
    if (p.x >= 0 && p.y >= 0 && p.x != p.y) {
      const unsigned lo = static_cast<unsigned>(p.x < p.y ? p.x : p.y), hi = static_cast<unsigned>(p.x < p.y ? p.y : p.x);
      const unsigned long long key = (static_cast<unsigned long long>(lo) << 32) | hi;
      size_t a = 0, b = c_old;  // first position with keys[pos] >= key
      while (a < b) {
        const size_t m = a + (b - a) / 2;
        if (keys[m] < key) a = m + 1;
        else b = m;
      }
      if (a < c_old && keys[a] == key) {
        const unsigned v = vals[a];
        h = load3(hist_old, static_cast<size_t>(v & ~kFlipBit));
        // the history is "j relative to i": a pair listed the other way round than before sees its negative
        if (((v & kFlipBit) != 0u) != (p.x > p.y)) h = V3{-h.x, -h.y, -h.z};
        ++found;
      }
    }
    store3(hist_new, c, h);
  }
  block_stat_add(found, carried);
}

struct CarryScratch {
  DeviceBuffer keys, keys_tmp, vals, vals_tmp, ws, count;
  ScratchOwner owner;
};
static CarryScratch& carry_scratch() {
  thread_local CarryScratch s;
  return s;
}

}  // namespace mhip

using namespace mhip;

extern "C" {

int mhip_hertz_friction_force(size_t c, size_t n, const int32_t* pairs, const double* sep, const double* normal,
                              const double* arc_s, const double* arc_t, const double* seg, const double* radius,
                              const double* youngs_modulus, double youngs_modulus_scalar, const double* poisson_ratio,
                              double poisson_ratio_scalar, const double* velocity_prev,
                              const mhip_hertz_friction_params* params, double* tang_disp, double* force, void* stats,
                              mhip_stream_t stream) {
  MHIP_REQUIRE(params != nullptr, MHIP_ERR_INVALID_ARGUMENT, "params is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(c == 0 || (pairs && sep && normal && arc_s && arc_t && tang_disp && force), MHIP_ERR_INVALID_ARGUMENT,
               "pairs / sep / normal / arc_s / arc_t / tang_disp / force is null");
  MHIP_REQUIRE(n == 0 || (seg && radius && velocity_prev), MHIP_ERR_INVALID_ARGUMENT,
               "seg / radius / velocity_prev is null");
  MHIP_REQUIRE(params->mu >= 0.0 && std::isfinite(params->mu), MHIP_ERR_INVALID_ARGUMENT,
               "mu must be finite and >= 0, got %g", params->mu);
  MHIP_REQUIRE(params->normal_damping >= 0.0 && std::isfinite(params->normal_damping) &&
                   params->tangential_damping >= 0.0 && std::isfinite(params->tangential_damping),
               MHIP_ERR_INVALID_ARGUMENT, "damping coefficients must be finite and >= 0, got %g, %g",
               params->normal_damping, params->tangential_damping);
  MHIP_REQUIRE(params->density >= 0.0 && std::isfinite(params->density), MHIP_ERR_INVALID_ARGUMENT,
               "density must be finite and >= 0, got %g", params->density);
  MHIP_REQUIRE(params->dt >= 0.0 && std::isfinite(params->dt), MHIP_ERR_INVALID_ARGUMENT,
               "dt must be finite and >= 0, got %g", params->dt);
  MHIP_REQUIRE(youngs_modulus || (youngs_modulus_scalar > 0.0 && std::isfinite(youngs_modulus_scalar)),
               MHIP_ERR_INVALID_ARGUMENT, "youngs_modulus must be finite and > 0, got %g", youngs_modulus_scalar);
  MHIP_REQUIRE(poisson_ratio || (poisson_ratio_scalar > 0.0 && poisson_ratio_scalar < 1.0), MHIP_ERR_INVALID_ARGUMENT,
               "poisson_ratio must lie in (0, 1), got %g", poisson_ratio_scalar);
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_RUNTIME, "too many bodies for 32-bit pair indices");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s));
  if (c == 0) return MHIP_SUCCESS;
  const int2* p2 = reinterpret_cast<const int2*>(pairs);
  unsigned long long* st = static_cast<unsigned long long*>(stats);
  const double E0 = youngs_modulus_scalar, nu0 = poisson_ratio_scalar;
  const unsigned grid = grid_for(c);
  dispatch_bools(youngs_modulus != nullptr, poisson_ratio != nullptr, [&](auto ea, auto na) {
    k_hertz_friction_force<decltype(ea)::value, decltype(na)::value><<<grid, kBlock, 0, s>>>(
        c, n, p2, sep, normal, arc_s, arc_t, seg, radius, youngs_modulus, E0, poisson_ratio, nu0, velocity_prev, *params,
        tang_disp, force, st);
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_contact_history_carry(size_t c_old, const int32_t* pairs_old, const double* hist_old,
                               const int32_t* new_of_old, size_t n_old, size_t c_new, const int32_t* pairs_new,
                               double* hist_new, size_t* carried, mhip_stream_t stream) {
  MHIP_REQUIRE(c_old == 0 || (pairs_old && hist_old), MHIP_ERR_INVALID_ARGUMENT, "pairs_old / hist_old is null");
  MHIP_REQUIRE(c_new == 0 || (pairs_new && hist_new), MHIP_ERR_INVALID_ARGUMENT, "pairs_new / hist_new is null");
  MHIP_REQUIRE(hist_new == nullptr || hist_new != hist_old, MHIP_ERR_INVALID_ARGUMENT, "the carry cannot run in place");
  MHIP_REQUIRE(c_old < (1ull << 31), MHIP_ERR_RUNTIME, "too many old pairs for 31-bit row indices");
  if (carried) *carried = 0;
  if (c_new == 0) return MHIP_SUCCESS;
  hipStream_t s = as_stream(stream);
  CarryScratch& cs = carry_scratch();
  if (int e = cs.owner.claim(s)) return e;
  if (int e = cs.count.reserve(2 * sizeof(unsigned long long))) return e;  // (rows carried, disorder flag)
  MHIP_HIP(hipMemsetAsync(cs.count.ptr, 0, 2 * sizeof(unsigned long long), s));
  if (c_old > 0) {
    if (int e = cs.keys.reserve(c_old * sizeof(unsigned long long))) return e;
    if (int e = cs.vals.reserve(c_old * sizeof(unsigned))) return e;
    k_history_keys<<<grid_for(c_old), kBlock, 0, s>>>(c_old, reinterpret_cast<const int2*>(pairs_old), new_of_old, n_old,
                                                      cs.keys.as<unsigned long long>(), cs.vals.as<unsigned>(),
                                                      cs.count.as<unsigned long long>() + 1);
    MHIP_LAUNCH_CHECK();
    if (new_of_old != nullptr) {  // a canonical list is sorted by (i, j) already: only a renumbering needs the sort
      if (int e = cs.keys_tmp.reserve(c_old * sizeof(unsigned long long))) return e;
      if (int e = cs.vals_tmp.reserve(c_old * sizeof(unsigned))) return e;
      if (int e = cs.ws.reserve(radix_sort_workspace_bytes(c_old))) return e;
      if (int e = radix_sort_u64(c_old, cs.keys.as<unsigned long long>(), cs.vals.as<unsigned>(),
                                 cs.keys_tmp.as<unsigned long long>(), cs.vals_tmp.as<unsigned>(), 8, cs.ws.ptr, s))
        return e;
    }
  }
  k_history_carry<<<grid_for(c_new), kBlock, 0, s>>>(c_old, cs.keys.as<unsigned long long>(), cs.vals.as<unsigned>(),
                                                     hist_old, c_new, reinterpret_cast<const int2*>(pairs_new), hist_new,
                                                     cs.count.as<unsigned long long>());
  MHIP_LAUNCH_CHECK();
  if (carried || (c_old > 0 && new_of_old == nullptr)) {
    unsigned long long k[2] = {0, 0};
    MHIP_HIP(hipMemcpyAsync(k, cs.count.ptr, sizeof(k), hipMemcpyDeviceToHost, s));
    MHIP_HIP(hipStreamSynchronize(s));
    // an unsorted list would have been searched all the same, and silently wrong: hist_new is not to be used
    MHIP_REQUIRE(k[1] == 0, MHIP_ERR_INVALID_ARGUMENT,
                 "pairs_old is not canonical (strictly ascending (i, j) with 0 <= i < j): pass new_of_old, which sorts");
    if (carried) *carried = static_cast<size_t>(k[0]);
  }
  return MHIP_SUCCESS;
}

}  // extern "C"
