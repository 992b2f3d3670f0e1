// hertz.hip -- the per-linker Hertzian soft-contact force of the reference's production loops
// (scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:755-804; kernels
// .../evaluate_linker_potentials/kernels/{SphereSphere,SphereSpherocylinder,SpherocylinderSpherocylinder}
// HertzianContact.cpp).  Per contact: a pair and its signed separation are read, for overlapping pairs only the two
// bodies' (r, E, nu) are gathered, and one force magnitude is written.  Elementwise and HBM bound.
#include "mhip_internal.hpp"
#include "force_device.hpp"

namespace mhip {

// The largest overlap max(0, -sep) of the launch goes to *max_overlap_bits (block_stat_max).
// One contact per lane and pass.  (Four contacts a grid stride apart per lane, all their loads issued before the first is
// used: 0.0692 against 0.0705 ms per launch at 10^6 rods, profiles/hertz_ab_unroll.txt -- not kept.)
template <bool E_ARRAY, bool NU_ARRAY>
__global__ void __launch_bounds__(kBlock)
    k_hertz_force(size_t C, size_t N, const int2* __restrict__ pairs, const double* __restrict__ sep,
                  const double* __restrict__ radius, const double* __restrict__ E, double E0,
                  const double* __restrict__ nu, double nu0, double* __restrict__ force,
                  unsigned long long* __restrict__ max_overlap_bits) {
  double dmax = 0.0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < C; c += (size_t)gridDim.x * blockDim.x) {
    const int2 p = pairs[c];
    const double s = sep[c];
    double f = 0.0;  // a pair that does not overlap (sep >= 0, or NaN) carries exactly +0.0 (:210-219)
    if (static_cast<unsigned>(p.x) >= N || static_cast<unsigned>(p.y) >= N) {
      f = __builtin_nan("");  // a pair outside [0, N) is never dereferenced
    } else if (s < 0.0) {
      const HertzPair h = hertz_pair<E_ARRAY, NU_ARRAY>(p, radius, E, E0, nu, nu0);
      f = hertz_force_magnitude(h.Es, h.Rs, s);
      dmax = -s > dmax ? -s : dmax;
    }
    force[c] = f;
  }
  block_stat_max(dmax, max_overlap_bits);
}

}  // namespace mhip

using namespace mhip;

extern "C" {

int mhip_hertz_contact_force(size_t c, size_t n, const int32_t* pairs, const double* sep, const double* radius,
                             const double* youngs_modulus, double youngs_modulus_scalar, const double* poisson_ratio,
                             double poisson_ratio_scalar, double* force, double* max_overlap, mhip_stream_t stream) {
  MHIP_REQUIRE(max_overlap != nullptr, MHIP_ERR_INVALID_ARGUMENT, "max_overlap is null");
  MHIP_REQUIRE(c == 0 || (pairs && sep && force), MHIP_ERR_INVALID_ARGUMENT, "pairs / sep / force is null");
  MHIP_REQUIRE(n == 0 || radius, MHIP_ERR_INVALID_ARGUMENT, "radius is null");
  // scalars stand for every body: E > 0 (Bacteria.cpp:392-395) and 0 < nu < 1 (E* finite and positive)
  MHIP_REQUIRE(youngs_modulus || (youngs_modulus_scalar > 0.0 && std::isfinite(youngs_modulus_scalar)),
               MHIP_ERR_INVALID_ARGUMENT, "youngs_modulus must be finite and > 0, got %g", youngs_modulus_scalar);
  MHIP_REQUIRE(poisson_ratio || (poisson_ratio_scalar > 0.0 && poisson_ratio_scalar < 1.0), MHIP_ERR_INVALID_ARGUMENT,
               "poisson_ratio must lie in (0, 1), got %g", poisson_ratio_scalar);
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_RUNTIME, "too many bodies for 32-bit pair indices");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(max_overlap, 0, sizeof(double), s));  // +0.0: also the answer for an empty list
  if (c == 0) return MHIP_SUCCESS;
  const int2* p2 = reinterpret_cast<const int2*>(pairs);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(max_overlap);
  const double E0 = youngs_modulus_scalar, nu0 = poisson_ratio_scalar;
  const unsigned grid = grid_for(c);
  dispatch_bools(youngs_modulus != nullptr, poisson_ratio != nullptr, [&](auto ea, auto na) {
    k_hertz_force<decltype(ea)::value, decltype(na)::value><<<grid, kBlock, 0, s>>>(
        c, n, p2, sep, radius, youngs_modulus, E0, poisson_ratio, nu0, force, mx);
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

}  // extern "C"
