// chain.hip -- bead-spring chains driven by thermal noise: the per-step kernels of the reference's chromatin loop
// (scrap/.../NgpHP1.cpp:3802-3990; SpringsUpdated.cpp, BrownianMotion.cpp) that the contact step does not already have.
//   spring forces   per body, over a body -> spring incidence built once on the device (no atomics on forces)
//   angular springs the three-body bending term (AngularSpringsKernel.cpp:107-197), per body over a body -> triplet
//                   incidence: every body evaluates the whole triplet and keeps its own row (mundy_hip_bending.h)
//   Philox4x32-10   the counter-based generator every reference app draws from (Salmon et al., SC'11)
//   Brownian        sqrt(2 kT m_t / dt) z added into the translational velocity rows, one counter step per body
//   drag velocity   U = M F of a per-body force (the U_ext = M F_ext of resolve_collisions, NgpHP1.cpp:1488-1531)
// All elementwise or per-body gathers of a few rows: HBM bound.
#include "mhip_internal.hpp"
#include "force_device.hpp"
#include "../../include/mundy_hip_bending.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mhip {

__global__ void __launch_bounds__(kBlock) k_philox(size_t count, const uint64_t* __restrict__ keys,
                                                  const uint64_t* __restrict__ ctrs, uint32_t block,
                                                  uint4* __restrict__ out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
    out[i] = philox_draw(keys[i], ctrs[i], block);
}

// uniform -> normal (documented in mundy_hip.h): u1 = (m + 1) 2^-53 in (0, 1] from the 53-bit integer m of the first two
// words, u2 = m' 2^-53 in [0, 1) from the other two words; Box-Muller
__device__ inline void box_muller(uint4 w, double& z0, double& z1) {
  const double u1 = static_cast<double>(philox_u53(w) + 1) * 0x1p-53;
  const double u2 = static_cast<double>(philox_u53(make_uint4(w.z, w.w, 0u, 0u))) * 0x1p-53;
  const double rad = sqrt(-2.0 * log(u1));
  const double th = 6.283185307179586 * u2;
  z0 = rad * cos(th);
  z1 = rad * sin(th);
}

// One body per lane: blocks 0 and 1 at (key, counter) -> four normals, the first three used; counter += 1
// (NgpHP1.cpp's rng_counter[0]++).  The coefficient sqrt(2 D / dt), D = kT m_t (BrownianMotion.cpp:571).
__global__ void __launch_bounds__(kBlock) k_brownian(size_t n, const uint64_t* __restrict__ keys,
                                                    uint64_t* __restrict__ ctrs, double kt, double dt,
                                                    const double* __restrict__ mt, double* __restrict__ vel) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const uint64_t key = keys[i], ctr = ctrs[i];
    double z0, z1, z2, z3;
    box_muller(philox_draw(key, ctr, 0u), z0, z1);
    box_muller(philox_draw(key, ctr, 1u), z2, z3);
    const double coef = sqrt(2.0 * kt * mt[i] / dt);
    double* v = vel + 6 * i;
    v[0] = v[0] + coef * z0;
    v[1] = v[1] + coef * z1;
    v[2] = v[2] + coef * z2;
    ctrs[i] = ctr + 1;
  }
}

// U = (m_t F, 0): the dry drag of a per-body force; force == nullptr stands for F = 0
__global__ void __launch_bounds__(kBlock) k_drag_velocity(size_t n, const double* __restrict__ mt,
                                                         const double* __restrict__ force, double* __restrict__ vel) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double m = mt[i];
    double* v = vel + 6 * i;
    if (force) {
      v[0] = m * force[3 * i];
      v[1] = m * force[3 * i + 1];
      v[2] = m * force[3 * i + 2];
    } else {
      v[0] = 0.0; v[1] = 0.0; v[2] = 0.0;
    }
    v[3] = 0.0; v[4] = 0.0; v[5] = 0.0;
  }
}

// ---- body -> entry incidence (force_device.hpp) ------------------------------------------------------------------
template <class SRC>
__global__ void __launch_bounds__(kBlock) k_incidence_count(size_t m, SRC src, int32_t* __restrict__ deg) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    src(i, [&](int32_t b, int32_t) { atomicAdd(&deg[b], 1); });
}
template <class SRC>
__global__ void __launch_bounds__(kBlock) k_incidence_fill(size_t m, SRC src, const int32_t* __restrict__ ptr,
                                                          int32_t* __restrict__ cursor, int32_t* __restrict__ ent) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < m; i += (size_t)gridDim.x * blockDim.x)
    src(i, [&](int32_t b, int32_t e) { ent[ptr[b] + atomicAdd(&cursor[b], 1)] = e; });
}
// the fill order depends on atomic arrival: each body sorts its own short list (chains: 2 entries)
__global__ void __launch_bounds__(kBlock) k_incidence_sort(size_t n, const int32_t* __restrict__ ptr,
                                                          int32_t* __restrict__ ent) {
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    for (int32_t a = lo + 1; a < hi; ++a) {
      const int32_t v = ent[a];
      int32_t k = a - 1;
      while (k >= lo && ent[k] > v) {
        ent[k + 1] = ent[k];
        --k;
      }
      ent[k + 1] = v;
    }
  }
}

template <class SRC>
int build_incidence(size_t n, size_t m, SRC src, int32_t* deg, int32_t* ptr, int32_t* ent, void* ws, hipStream_t s) {
  MHIP_HIP(hipMemsetAsync(deg, 0, (n + 1) * sizeof(int32_t), s));
  if (m > 0) k_incidence_count<<<grid_for(m), kBlock, 0, s>>>(m, src, deg);
  MHIP_LAUNCH_CHECK();
  if (n > 0) {
    if (int e = exclusive_scan_i32(deg, ptr, n, ws, s)) return e;
  } else {
    MHIP_HIP(hipMemsetAsync(ptr, 0, sizeof(int32_t), s));
  }
  MHIP_HIP(hipMemsetAsync(deg, 0, (n + 1) * sizeof(int32_t), s));
  if (m > 0) {
    k_incidence_fill<<<grid_for(m), kBlock, 0, s>>>(m, src, ptr, deg, ent);
    MHIP_LAUNCH_CHECK();
    k_incidence_sort<<<grid_for(n), kBlock, 0, s>>>(n, ptr, ent);
    MHIP_LAUNCH_CHECK();
  }
  return MHIP_SUCCESS;
}
template int build_incidence(size_t, size_t, PairEnds, int32_t*, int32_t*, int32_t*, void*, hipStream_t);
template int build_incidence(size_t, size_t, ListedAt, int32_t*, int32_t*, int32_t*, void*, hipStream_t);
template int build_incidence(size_t, size_t, ListedAtBody, int32_t*, int32_t*, int32_t*, void*, hipStream_t);
template int build_incidence(size_t, size_t, TripletEnds, int32_t*, int32_t*, int32_t*, void*, hipStream_t);

// ---- springs -----------------------------------------------------------------------------------------------------
// One body per lane: walk its springs in ascending index, recompute each spring's d = x_j - x_i, L = |d| and term
// fm d in the same operations at both ends (so the two ends receive exactly negated vectors), sum from +0.0.
// The spring's own statistics (longest L, overstretched FENE, clamped FENE-WCA) are taken at its first end only.
template <int TYPE, bool K_ARRAY, bool R_ARRAY>
__global__ void __launch_bounds__(kBlock)
    k_spring_force(size_t n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                   const int2* __restrict__ pairs, const double* __restrict__ center, const double* __restrict__ kk,
                   double k0, const double* __restrict__ rr, double r0, WcaParams wca, double* __restrict__ force,
                   int* __restrict__ overstretched, unsigned long long* __restrict__ max_length_bits) {
  double lmax = 0.0;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    V3 f{0.0, 0.0, 0.0};
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    for (int32_t e = lo; e < hi; ++e) {
      const int32_t en = ent[e];
      const int32_t s = en >> 1;
      const bool first = (en & 1) == 0;
      const int2 p = pairs[s];
      const V3 d = load3(center, p.y) - load3(center, p.x);
      const double r = R_ARRAY ? rr[s] : r0;
      const SpringTerm t = spring_term<TYPE>(d, K_ARRAY ? kk[s] : k0, r, wca);
      if (TYPE == MHIP_SPRING_FENE && first && !(t.L < r)) atomicAdd(overstretched, 1);
      if (TYPE == MHIP_SPRING_FENEWCA && first && !(t.L < r - kFeneWcaClamp)) atomicAdd(overstretched, 1);
      if (first) lmax = t.L > lmax ? t.L : lmax;
      add_term(f, !first, t.fm, d);
    }
    store3(force, b, f);
  }
  block_stat_max(lmax, max_length_bits);
}

// ---- angular springs (mundy_hip_bending.h) -------------------------------------------------------------------------
// The three rows of one triplet and what its statistics need, in the reference's expressions and association
// (AngularSpringsKernel.cpp:143-168): -grad of U = 1/2 k (cos(theta) - cos_rest)^2.
struct AngularTerm {
  V3 fa, fb, fc;
  double L1, L2, deviation;
};
__device__ inline AngularTerm angular_term(V3 xa, V3 xb, V3 xc, double k, double cos_rest) {
  const V3 v1 = xa - xc, v2 = xb - xc;
  const double s1 = dot(v1, v1), s2 = dot(v2, v2);
  const double L1 = sqrt(s1), L2 = sqrt(s2);
  const double c = dot(v1, v2) / (L1 * L2);
  const double tau = k * (c - cos_rest);
  const double a11 = tau * c / s1;
  const double a13 = -tau / (L1 * L2);
  const double a33 = tau * c / s2;
  const V3 fa = a11 * v1 + a13 * v2;
  const V3 fb = a33 * v2 + a13 * v1;
  const V3 fc{-fa.x - fb.x, -fa.y - fb.y, -fa.z - fb.z};
  return {fa, fb, fc, L1, L2, fabs(c - cos_rest)};
}
__global__ void __launch_bounds__(kBlock) k_triplet_renumber(size_t m, const int32_t* __restrict__ new_of_old,
                                                            Triplet* __restrict__ triplets) {
  for (size_t t = blockIdx.x * (size_t)blockDim.x + threadIdx.x; t < m; t += (size_t)gridDim.x * blockDim.x) {
    const Triplet q = triplets[t];
    triplets[t] = Triplet{new_of_old[q.a], new_of_old[q.b], new_of_old[q.c], 0};
  }
}
// One body per lane: its entries in ascending order from +0.0; the whole triplet is evaluated at each of its three
// bodies in the same operations, and the lane keeps the row of its role.  The triplet's own statistics are taken at its
// role-0 entry only.
template <bool ACCUMULATE, bool K_ARRAY, bool C_ARRAY>
__global__ void __launch_bounds__(kBlock)
    k_angular_force(size_t n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                    const Triplet* __restrict__ triplets, const double* __restrict__ center,
                    const double* __restrict__ kk, double k0, const double* __restrict__ cc, double c0,
                    double* __restrict__ force, int* __restrict__ degenerate,
                    unsigned long long* __restrict__ max_deviation_bits) {
  double dmax = 0.0;
  int count = 0;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    V3 f{0.0, 0.0, 0.0};
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    for (int32_t e = lo; e < hi; ++e) {
      const int32_t en = ent[e];
      const int32_t t = en >> 2, role = en & 3;
      const Triplet q = triplets[t];
      const AngularTerm a = angular_term(load3(center, q.a), load3(center, q.b), load3(center, q.c),
                                         K_ARRAY ? kk[t] : k0, C_ARRAY ? cc[t] : c0);
      if (role == 0) {
        if (a.L1 == 0.0 || a.L2 == 0.0) ++count;
        dmax = a.deviation > dmax ? a.deviation : dmax;
      }
      f = f + (role == 0 ? a.fa : role == 1 ? a.fb : a.fc);
    }
    if (ACCUMULATE && lo == hi) continue;  // untouched on no triplet
    write_force<ACCUMULATE>(force, b, f);
  }
  wave_stat_add(count, degenerate);
  block_stat_max(dmax, max_deviation_bits);
}

}  // namespace mhip

using namespace mhip;

struct mhip_springs {
  size_t n = 0, m = 0;
  int type = MHIP_SPRING_HOOKEAN;
  double k0 = 0.0, r0 = 0.0;
  bool k_array = false, r_array = false;
  WcaParams wca;  // MHIP_SPRING_FENEWCA: epsilon, sigma and the cutoff 2^(1/6) sigma (mhip_springs_set_wca)
  HandleBuffer pairs, k, r, ptr, ent, cursor, ws;
};

struct mhip_angular_springs {
  size_t n = 0, m = 0;
  double k0 = 0.0, c0 = 0.0;
  bool k_array = false, c_array = false;
  std::vector<double> host_k, host_cos;  // what the device holds, for mhip_angular_springs_get
  HandleBuffer triplets, k, cos_rest, ptr, ent, cursor, ws;
};

namespace {

double wca_cutoff(double sigma) { return std::pow(2.0, 1.0 / 6.0) * sigma; }  // FENEWCASpringsKernel.cpp:168

int build_lists(mhip_angular_springs* h, hipStream_t s) {
  return build_incidence(h->n, h->m, TripletEnds{h->triplets.as<Triplet>()}, h->cursor.as<int32_t>(),
                         h->ptr.as<int32_t>(), h->ent.as<int32_t>(), h->ws.ptr, s);
}

}  // namespace

extern "C" {

int mhip_springs_create(mhip_springs_t* handle, size_t n, size_t m, const int32_t* pairs, int type, const double* k,
                        double k_scalar, const double* r, double r_scalar, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(type == MHIP_SPRING_HOOKEAN || type == MHIP_SPRING_FENE || type == MHIP_SPRING_FENEWCA,
               MHIP_ERR_INVALID_ARGUMENT, "unknown spring type %d", type);
  MHIP_REQUIRE(m == 0 || pairs, MHIP_ERR_INVALID_ARGUMENT, "pairs is null");
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit spring endpoints");
  MHIP_REQUIRE(m < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many springs for 31-bit incidence entries");
  const bool fene = type != MHIP_SPRING_HOOKEAN;  // r is r_max
  const char* rname = fene ? "r_max" : "rest length";
  // host arrays: every spring is checked here, before anything reaches the device
  auto k_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  auto r_ok = [fene](double v) { return std::isfinite(v) && (fene ? v > 0.0 : v >= 0.0); };
  MHIP_REQUIRE(k || k_ok(k_scalar), MHIP_ERR_INVALID_ARGUMENT, "spring constant k must be finite and >= 0, got %g",
               k_scalar);
  MHIP_REQUIRE(r || r_ok(r_scalar), MHIP_ERR_INVALID_ARGUMENT, "%s must be finite and %s 0, got %g", rname,
               fene ? ">" : ">=", r_scalar);
  for (size_t s = 0; s < m; ++s) {
    const int32_t i = pairs[2 * s], j = pairs[2 * s + 1];
    MHIP_REQUIRE(i >= 0 && j >= 0 && static_cast<size_t>(i) < n && static_cast<size_t>(j) < n,
                 MHIP_ERR_INVALID_ARGUMENT, "spring %zu joins (%d, %d): an index outside [0, %zu)", s, i, j, n);
    MHIP_REQUIRE(i != j, MHIP_ERR_INVALID_ARGUMENT, "spring %zu joins body %d to itself", s, i);
    if (k) MHIP_REQUIRE(k_ok(k[s]), MHIP_ERR_INVALID_ARGUMENT, "spring %zu: k must be finite and >= 0, got %g", s, k[s]);
    if (r) MHIP_REQUIRE(r_ok(r[s]), MHIP_ERR_INVALID_ARGUMENT, "spring %zu: %s must be finite and %s 0, got %g", s, rname,
                        fene ? ">" : ">=", r[s]);
  }
  auto h = std::make_unique<mhip_springs>();
  h->n = n;
  h->m = m;
  h->type = type;
  h->k0 = k_scalar;
  h->r0 = r_scalar;
  h->k_array = k != nullptr;
  h->r_array = r != nullptr;
  h->wca.cutoff = wca_cutoff(h->wca.sigma);
  hipStream_t s = as_stream(stream);
  int e = MHIP_SUCCESS;
  if ((e = h->ptr.reserve((n + 1) * sizeof(int32_t))) || (e = h->cursor.reserve((n + 1) * sizeof(int32_t))) ||
      (e = h->pairs.reserve(2 * m * sizeof(int32_t) + 8)) || (e = h->ent.reserve(2 * m * sizeof(int32_t) + 8)) ||
      (e = h->ws.reserve(scan_workspace_bytes(n) + 8)))
    return e;
  if (k && (e = h->k.reserve(m * sizeof(double) + 8))) return e;
  if (r && (e = h->r.reserve(m * sizeof(double) + 8))) return e;
  if (m > 0) {
    if ((e = upload(__func__, h->pairs, pairs, 2 * m * sizeof(int32_t), s))) return e;
    if (k && (e = upload(__func__, h->k, k, m * sizeof(double), s))) return e;
    if (r && (e = upload(__func__, h->r, r, m * sizeof(double), s))) return e;
  }
  if ((e = build_incidence(n, m, PairEnds{h->pairs.as<int2>()}, h->cursor.as<int32_t>(), h->ptr.as<int32_t>(),
                           h->ent.as<int32_t>(), h->ws.ptr, s)))
    return e;
  // the caller's host arrays may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_springs_destroy(mhip_springs_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_springs_force(mhip_springs_t h, const double* center, double* force, int* overstretched, double* max_length,
                       mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "springs handle is null");
  MHIP_REQUIRE(overstretched != nullptr && max_length != nullptr, MHIP_ERR_INVALID_ARGUMENT,
               "overstretched / max_length is null");
  MHIP_REQUIRE(h->n == 0 || (center && force), MHIP_ERR_INVALID_ARGUMENT, "center / force is null");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(overstretched, 0, sizeof(int), s));
  MHIP_HIP(hipMemsetAsync(max_length, 0, sizeof(double), s));  // +0.0: also the answer without springs
  if (h->n == 0) return MHIP_SUCCESS;
  const unsigned grid = grid_for(h->n);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(max_length);
  const int32_t* ptr = h->ptr.as<int32_t>();
  const int32_t* ent = h->ent.as<int32_t>();
  const int2* p2 = h->pairs.as<int2>();
  const double* kk = h->k_array ? h->k.as<double>() : nullptr;
  const double* rr = h->r_array ? h->r.as<double>() : nullptr;
  dispatch<MHIP_SPRING_FENEWCA, MHIP_SPRING_FENE, MHIP_SPRING_HOOKEAN>(h->type, [&](auto type) {
    dispatch_bools(kk != nullptr, rr != nullptr, [&](auto ka, auto ra) {
      k_spring_force<decltype(type)::value, decltype(ka)::value, decltype(ra)::value><<<grid, kBlock, 0, s>>>(
          h->n, ptr, ent, p2, center, kk, h->k0, rr, h->r0, h->wca, force, overstretched, mx);
    });
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_springs_set_wca(mhip_springs_t h, double epsilon, double sigma) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "springs handle is null");
  MHIP_REQUIRE(h->type == MHIP_SPRING_FENEWCA, MHIP_ERR_INVALID_ARGUMENT,
               "epsilon and sigma belong to MHIP_SPRING_FENEWCA: this spring set has type %d", h->type);
  MHIP_REQUIRE(std::isfinite(epsilon) && epsilon > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "WCA epsilon must be finite and > 0, got %g", epsilon);
  MHIP_REQUIRE(std::isfinite(sigma) && sigma > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "WCA sigma must be finite and > 0, got %g", sigma);
  h->wca = WcaParams{epsilon, sigma, wca_cutoff(sigma)};
  return MHIP_SUCCESS;
}

int mhip_angular_springs_create(mhip_angular_springs_t* handle, size_t n, size_t m, const int32_t* triplets,
                                const double* k, double k_scalar, const double* rest_angle,
                                double rest_angle_scalar, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(m == 0 || triplets, MHIP_ERR_INVALID_ARGUMENT, "triplets is null");
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit triplet indices");
  MHIP_REQUIRE(m < (1ull << 29), MHIP_ERR_INVALID_ARGUMENT, "too many triplets for 31-bit incidence entries");
  // host arrays: every triplet is checked here, before anything reaches the device
  auto k_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  auto a_ok = [](double v) { return std::isfinite(v) && v >= 0.0 && v <= M_PI; };
  MHIP_REQUIRE(k || k_ok(k_scalar), MHIP_ERR_INVALID_ARGUMENT,
               "angular spring constant k must be finite and >= 0, got %g", k_scalar);
  MHIP_REQUIRE(rest_angle || a_ok(rest_angle_scalar), MHIP_ERR_INVALID_ARGUMENT,
               "rest angle must be finite and in [0, pi], got %g", rest_angle_scalar);
  std::vector<Triplet> packed(m);
  for (size_t t = 0; t < m; ++t) {
    const int32_t a = triplets[3 * t], b = triplets[3 * t + 1], c = triplets[3 * t + 2];
    MHIP_REQUIRE(a >= 0 && b >= 0 && c >= 0 && static_cast<size_t>(a) < n && static_cast<size_t>(b) < n &&
                     static_cast<size_t>(c) < n,
                 MHIP_ERR_INVALID_ARGUMENT, "triplet %zu joins (%d, %d, %d): an index outside [0, %zu)", t, a, b, c, n);
    MHIP_REQUIRE(a != b && a != c && b != c, MHIP_ERR_INVALID_ARGUMENT,
                 "triplet %zu joins (%d, %d, %d): its three bodies are not distinct", t, a, b, c);
    if (k) MHIP_REQUIRE(k_ok(k[t]), MHIP_ERR_INVALID_ARGUMENT, "triplet %zu: k must be finite and >= 0, got %g", t, k[t]);
    if (rest_angle)
      MHIP_REQUIRE(a_ok(rest_angle[t]), MHIP_ERR_INVALID_ARGUMENT,
                   "triplet %zu: rest angle must be finite and in [0, pi], got %g", t, rest_angle[t]);
    packed[t] = Triplet{a, b, c, 0};
  }
  auto h = std::make_unique<mhip_angular_springs>();
  h->n = n;
  h->m = m;
  h->k0 = k_scalar;
  h->c0 = std::cos(rest_angle_scalar);
  h->k_array = k != nullptr;
  h->c_array = rest_angle != nullptr;
  h->host_k.assign(m, k_scalar);
  h->host_cos.assign(m, h->c0);
  for (size_t t = 0; t < m; ++t) {
    if (k) h->host_k[t] = k[t];
    if (rest_angle) h->host_cos[t] = std::cos(rest_angle[t]);
  }
  hipStream_t s = as_stream(stream);
  int e = MHIP_SUCCESS;
  if ((e = h->ptr.reserve((n + 1) * sizeof(int32_t))) || (e = h->cursor.reserve((n + 1) * sizeof(int32_t))) ||
      (e = h->triplets.reserve(m * sizeof(Triplet) + 16)) || (e = h->ent.reserve(3 * m * sizeof(int32_t) + 8)) ||
      (e = h->ws.reserve(scan_workspace_bytes(n) + 8)))
    return e;
  if (k && (e = h->k.reserve(m * sizeof(double) + 8))) return e;
  if (rest_angle && (e = h->cos_rest.reserve(m * sizeof(double) + 8))) return e;
  if (m > 0) {
    if ((e = upload(__func__, h->triplets, packed.data(), m * sizeof(Triplet), s))) return e;
    if (k && (e = upload(__func__, h->k, h->host_k.data(), m * sizeof(double), s))) return e;
    if (rest_angle && (e = upload(__func__, h->cos_rest, h->host_cos.data(), m * sizeof(double), s))) return e;
  }
  if ((e = build_lists(h.get(), s))) return e;
  // the caller's host arrays (and packed) may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_angular_springs_destroy(mhip_angular_springs_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_angular_springs_force(mhip_angular_springs_t h, const double* center, double* force, int accumulate,
                               int* degenerate, double* max_deviation, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "angular springs handle is null");
  MHIP_REQUIRE(degenerate != nullptr && max_deviation != nullptr, MHIP_ERR_INVALID_ARGUMENT,
               "degenerate / max_deviation is null");
  MHIP_REQUIRE(accumulate == 0 || accumulate == 1, MHIP_ERR_INVALID_ARGUMENT, "accumulate must be 0 or 1, got %d",
               accumulate);
  MHIP_REQUIRE(h->n == 0 || (center && force), MHIP_ERR_INVALID_ARGUMENT, "center / force is null");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(degenerate, 0, sizeof(int), s));
  MHIP_HIP(hipMemsetAsync(max_deviation, 0, sizeof(double), s));  // +0.0: also the answer without triplets
  if (h->n == 0) return MHIP_SUCCESS;
  const unsigned grid = grid_for(h->n);
  unsigned long long* mx = reinterpret_cast<unsigned long long*>(max_deviation);
  const double* kk = h->k_array ? h->k.as<double>() : nullptr;
  const double* cc = h->c_array ? h->cos_rest.as<double>() : nullptr;
  dispatch<true, false>(accumulate != 0, [&](auto acc) {
    dispatch_bools(kk != nullptr, cc != nullptr, [&](auto ka, auto ca) {
      k_angular_force<decltype(acc)::value, decltype(ka)::value, decltype(ca)::value><<<grid, kBlock, 0, s>>>(
          h->n, h->ptr.as<int32_t>(), h->ent.as<int32_t>(), h->triplets.as<Triplet>(), center, kk, h->k0, cc, h->c0,
          force, degenerate, mx);
    });
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_angular_springs_renumber(mhip_angular_springs_t h, const int32_t* new_of_old, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "angular springs handle is null");
  MHIP_REQUIRE(h->n == 0 || new_of_old, MHIP_ERR_INVALID_ARGUMENT, "new_of_old is null");
  hipStream_t s = as_stream(stream);
  if (h->m > 0) {
    k_triplet_renumber<<<grid_for(h->m), kBlock, 0, s>>>(h->m, new_of_old, h->triplets.as<Triplet>());
    MHIP_LAUNCH_CHECK();
  }
  return build_lists(h, s);
}

int mhip_angular_springs_get(mhip_angular_springs_t h, int32_t* triplets, double* k, double* cos_rest) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "angular springs handle is null");
  const size_t m = h->m;
  if (k) std::copy(h->host_k.begin(), h->host_k.end(), k);
  if (cos_rest) std::copy(h->host_cos.begin(), h->host_cos.end(), cos_rest);
  if (triplets && m > 0) {  // (a renumbering may be in flight on any stream)
    std::vector<Triplet> packed(m);
    MHIP_HIP(hipDeviceSynchronize());
    MHIP_HIP(hipMemcpy(packed.data(), h->triplets.ptr, m * sizeof(Triplet), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < m; ++t) {
      triplets[3 * t] = packed[t].a;
      triplets[3 * t + 1] = packed[t].b;
      triplets[3 * t + 2] = packed[t].c;
    }
  }
  return MHIP_SUCCESS;
}

int mhip_philox4x32_10(size_t count, const uint64_t* keys, const uint64_t* counters, uint32_t block, uint32_t* out,
                       mhip_stream_t stream) {
  MHIP_REQUIRE(count == 0 || (keys && counters && out), MHIP_ERR_INVALID_ARGUMENT, "keys / counters / out is null");
  if (count == 0) return MHIP_SUCCESS;
  hipStream_t s = as_stream(stream);
  k_philox<<<grid_for(count), kBlock, 0, s>>>(count, keys, counters, block, reinterpret_cast<uint4*>(out));
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_brownian_velocity(size_t n, const uint64_t* keys, uint64_t* counters, double kt, double dt,
                           const double* mob_trans, double* velocity, mhip_stream_t stream) {
  MHIP_REQUIRE(std::isfinite(kt) && kt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "kt must be finite and >= 0, got %g", kt);
  MHIP_REQUIRE(std::isfinite(dt) && dt > 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and > 0, got %g", dt);
  MHIP_REQUIRE(n == 0 || (keys && counters && mob_trans && velocity), MHIP_ERR_INVALID_ARGUMENT,
               "keys / counters / mob_trans / velocity is null");
  if (n == 0) return MHIP_SUCCESS;
  hipStream_t s = as_stream(stream);
  k_brownian<<<grid_for(n), kBlock, 0, s>>>(n, keys, counters, kt, dt, mob_trans, velocity);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_drag_velocity(size_t n, const double* mob_trans, const double* force, double* velocity, mhip_stream_t stream) {
  MHIP_REQUIRE(n == 0 || (mob_trans && velocity), MHIP_ERR_INVALID_ARGUMENT, "mob_trans / velocity is null");
  if (n == 0) return MHIP_SUCCESS;
  hipStream_t s = as_stream(stream);
  k_drag_velocity<<<grid_for(n), kBlock, 0, s>>>(n, mob_trans, force, velocity);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

}  // extern "C"
