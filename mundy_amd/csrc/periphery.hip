// periphery.hip -- the nuclear periphery of the reference's HP1 app: a wall that confines every bead in a sphere or an
// ellipsoid (scrap/.../HP1.cpp:4063-4284; the device restatement NgpHP1.cpp:2409-2527).  One body per lane, grid-stride,
// no atomics on forces:
//   sphere            ssd = R - |c - center| - r, a linear spring along the inward normal where ssd < 0 (HP1.cpp:4208-4238)
//   ellipsoid         the reference's coarse filter (level set at the eight corners of the bead's box), then the exact
//                     signed point - ellipsoid distance of segment_ellipsoid.hpp for the beads that fail it; the reference
//                     calls a shared-normal distance that its tree does not define
//   ellipsoid, fast   the level set of the ellipsoid shrunk by r and its gradient as the force (HP1.cpp:4148-4206)
// The sphere and fast kernels stream 32 B per body (+ 48 B read-modify-write for a colliding one): HBM bound.  The exact
// kernel runs its Newton iteration on the minority of lanes next to the wall.
#include "mhip_internal.hpp"
#include "force_device.hpp"
#include "segment_ellipsoid.hpp"

#include <cmath>

namespace mhip {

struct PeripheryD {
  V3 c;
  Quat q;
  V3 e;
  double K;
};

// (b0 b0 inv_a2 + b1 b1 inv_b2 + b2 b2 inv_c2) - 1, the reference's association
__device__ inline double level_set(V3 b, double ia, double ib, double ic) {
  return (b.x * b.x * ia + b.y * b.y * ib + b.z * b.z * ic) - 1.0;
}

template <int SHAPE, bool ACCUMULATE>
__global__ void __launch_bounds__(kBlock)
    k_periphery_force(size_t n, PeripheryD P, const double* __restrict__ center, const double* __restrict__ radius,
                      double* __restrict__ force, int* __restrict__ colliding,
                      unsigned long long* __restrict__ max_overlap_bits) {
  double omax = 0.0;
  int hits = 0;
  const Quat qc{P.q.w, -P.q.x, -P.q.y, -P.q.z};
  const double ia = 1.0 / (P.e.x * P.e.x), ib = 1.0 / (P.e.y * P.e.y), ic = 1.0 / (P.e.z * P.e.z);
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    const V3 c = load3(center, b);
    const double r = radius[b];
    bool hit = false;
    double fx = 0.0, fy = 0.0, fz = 0.0, over = 0.0;
    if (SHAPE == MHIP_PERIPHERY_SPHERE) {
      const V3 x = c - P.c;
      const double nrm = sqrt(x.x * x.x + (x.y * x.y + x.z * x.z));  // two_norm's fold
      const double ssd = P.e.x - nrm - r;
      if (ssd < 0.0) {
        const double inv = 1.0 / nrm;
        hit = true;
        over = -ssd;
        fx = (P.K * (-x.x * inv)) * ssd;
        fy = (P.K * (-x.y * inv)) * ssd;
        fz = (P.K * (-x.z * inv)) * ssd;
      }
    } else if (SHAPE == MHIP_PERIPHERY_ELLIPSOID_FAST) {
      const V3 x = c - P.c;
      const double ja = 1.0 / ((P.e.x - r) * (P.e.x - r)), jb = 1.0 / ((P.e.y - r) * (P.e.y - r)),
                   jc = 1.0 / ((P.e.z - r) * (P.e.z - r));
      const double g = level_set(x, ja, jb, jc);
      if (g > 0.0) {
        hit = true;
        over = g;
        fx = P.K * (2.0 * x.x * ja);
        fy = P.K * (2.0 * x.y * jb);
        fz = P.K * (2.0 * x.z * jc);
      }
    } else {
      // coarse filter: the bead's box lies inside the ellipsoid when all eight corners do (NgpHP1.cpp:2462-2500)
      bool all_inside = true;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const V3 corner{(k & 1) ? c.x + r : c.x - r, (k & 2) ? c.y + r : c.y - r, (k & 4) ? c.z + r : c.z - r};
        all_inside = all_inside && (level_set(qrot(qc, corner - P.c), ia, ib, ic) < 0.0);
      }
      if (!all_inside) {
        const segell::PointResult pr = segell::point_ellipsoid_body(qrot(qc, c - P.c), P.e);
        const double ssd = -pr.sdist - r;
        if (ssd < 0.0) {
          const V3 nl = qrot(P.q, pr.n);
          hit = true;
          over = -ssd;
          fx = (P.K * (-nl.x)) * ssd;
          fy = (P.K * (-nl.y)) * ssd;
          fz = (P.K * (-nl.z)) * ssd;
        }
      }
    }
    if (hit) {
      ++hits;
      omax = over > omax ? over : omax;
      // the wall force is taken off the row, or off +0.0: x - f is x + (-f) exactly, but 0.0 - f is not -f for f = +0.0
      write_force<ACCUMULATE>(force, b, ACCUMULATE ? V3{-fx, -fy, -fz} : V3{0.0 - fx, 0.0 - fy, 0.0 - fz});
    } else if (!ACCUMULATE) {  // accumulate: untouched without contact
      write_force<false>(force, b, V3{0.0, 0.0, 0.0});
    }
  }
  wave_stat_add(hits, colliding);
  block_stat_max(omax, max_overlap_bits);
}

}  // namespace mhip

using namespace mhip;

extern "C" {

int mhip_periphery_force(const mhip_periphery* cfg, size_t n, const double* center, const double* radius, double* force,
                         int accumulate, int* colliding, double* max_overlap, mhip_stream_t stream) {
  MHIP_REQUIRE(cfg != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery is null");
  const int shape = cfg->shape;
  MHIP_REQUIRE(shape == MHIP_PERIPHERY_SPHERE || shape == MHIP_PERIPHERY_ELLIPSOID ||
                   shape == MHIP_PERIPHERY_ELLIPSOID_FAST,
               MHIP_ERR_INVALID_ARGUMENT, "unknown periphery shape %d", shape);
  const int num_radii = shape == MHIP_PERIPHERY_SPHERE ? 1 : 3;
  for (int k = 0; k < num_radii; ++k)
    MHIP_REQUIRE(std::isfinite(cfg->radii[k]) && cfg->radii[k] > 0.0, MHIP_ERR_INVALID_ARGUMENT,
                 "periphery radii[%d] must be finite and > 0, got %g", k, cfg->radii[k]);
  MHIP_REQUIRE(std::isfinite(cfg->k) && cfg->k >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "periphery spring constant k must be finite and >= 0, got %g", cfg->k);
  for (int k = 0; k < 3; ++k)
    MHIP_REQUIRE(std::isfinite(cfg->center[k]), MHIP_ERR_INVALID_ARGUMENT, "periphery center[%d] is not finite", k);
  double q2 = 0.0;
  for (int k = 0; k < 4; ++k) {
    MHIP_REQUIRE(std::isfinite(cfg->quat[k]), MHIP_ERR_INVALID_ARGUMENT, "periphery quat[%d] is not finite", k);
    q2 += cfg->quat[k] * cfg->quat[k];
  }
  MHIP_REQUIRE(std::fabs(q2 - 1.0) <= 1e-12, MHIP_ERR_INVALID_ARGUMENT,
               "periphery quat must be a unit quaternion to 1e-12, |q|^2 - 1 = %g", q2 - 1.0);
  MHIP_REQUIRE(shape != MHIP_PERIPHERY_ELLIPSOID_FAST ||
                   (cfg->quat[0] == 1.0 && cfg->quat[1] == 0.0 && cfg->quat[2] == 0.0 && cfg->quat[3] == 0.0),
               MHIP_ERR_INVALID_ARGUMENT,
               "MHIP_PERIPHERY_ELLIPSOID_FAST has no orientation (HP1.cpp:4155-4159): quat must be (1, 0, 0, 0)");
  MHIP_REQUIRE(n == 0 || (center && radius && force), MHIP_ERR_INVALID_ARGUMENT, "center / radius / force is null");
  hipStream_t s = as_stream(stream);
  if (colliding) MHIP_HIP(hipMemsetAsync(colliding, 0, sizeof(int), s));
  if (max_overlap) MHIP_HIP(hipMemsetAsync(max_overlap, 0, sizeof(double), s));  // +0.0: the answer without contact
  if (n == 0) return MHIP_SUCCESS;
  const double r1 = num_radii == 3 ? cfg->radii[1] : cfg->radii[0], r2 = num_radii == 3 ? cfg->radii[2] : cfg->radii[0];
  const PeripheryD P{V3{cfg->center[0], cfg->center[1], cfg->center[2]},
                     Quat{cfg->quat[0], cfg->quat[1], cfg->quat[2], cfg->quat[3]}, V3{cfg->radii[0], r1, r2}, cfg->k};
  const unsigned grid = grid_for(n);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(max_overlap);
  dispatch<MHIP_PERIPHERY_SPHERE, MHIP_PERIPHERY_ELLIPSOID, MHIP_PERIPHERY_ELLIPSOID_FAST>(shape, [&](auto sh) {
    dispatch<true, false>(accumulate != 0, [&](auto acc) {
      k_periphery_force<decltype(sh)::value, decltype(acc)::value><<<grid, kBlock, 0, s>>>(n, P, center, radius, force,
                                                                                          colliding, mx);
    });
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

}  // extern "C"
