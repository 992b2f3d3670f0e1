// chain.hip -- bead-spring chains driven by thermal noise: the per-step kernels of the reference's chromatin loop
// (scrap/.../NgpHP1.cpp:3802-3990; SpringsUpdated.cpp, BrownianMotion.cpp) that the contact step does not already have.
//   spring forces   per body, over a body -> spring incidence built once on the device (no atomics on forces)
//   Philox4x32-10   the counter-based generator every reference app draws from (Salmon et al., SC'11)
//   Brownian        sqrt(2 kT m_t / dt) z added into the translational velocity rows, one counter step per body
//   drag velocity   U = M F of a per-body force (the U_ext = M F_ext of resolve_collisions, NgpHP1.cpp:1488-1531)
// All elementwise or per-body gathers of a few rows: HBM bound.
#include "mhip_internal.hpp"
#include "force_device.hpp"

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

// ---- springs -----------------------------------------------------------------------------------------------------
// One body per lane: walk its springs in ascending index, recompute each spring's d = x_j - x_i, L = |d| and term
// fm d in the same operations at both ends (so the two ends receive exactly negated vectors), sum from +0.0.
// The spring's own statistics (longest L, overstretched FENE) are taken at its first end only.
template <int TYPE, bool K_ARRAY, bool R_ARRAY>
__global__ void __launch_bounds__(kBlock)
    k_spring_force(size_t n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                   const int2* __restrict__ pairs, const double* __restrict__ center, const double* __restrict__ kk,
                   double k0, const double* __restrict__ rr, double r0, double* __restrict__ force,
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
      const SpringTerm t = spring_term<TYPE>(d, K_ARRAY ? kk[s] : k0, r);
      if (TYPE == MHIP_SPRING_FENE && first && !(t.L < r)) atomicAdd(overstretched, 1);
      if (first) lmax = t.L > lmax ? t.L : lmax;
      add_term(f, !first, t.fm, d);
    }
    store3(force, b, f);
  }
  block_stat_max(lmax, max_length_bits);
}

}  // namespace mhip

using namespace mhip;

struct mhip_springs {
  size_t n = 0, m = 0;
  int type = MHIP_SPRING_HOOKEAN;
  double k0 = 0.0, r0 = 0.0;
  bool k_array = false, r_array = false;
  HandleBuffer pairs, k, r, ptr, ent, cursor, ws;
};

extern "C" {

int mhip_springs_create(mhip_springs_t* handle, size_t n, size_t m, const int32_t* pairs, int type, const double* k,
                        double k_scalar, const double* r, double r_scalar, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(type == MHIP_SPRING_HOOKEAN || type == MHIP_SPRING_FENE, MHIP_ERR_INVALID_ARGUMENT,
               "unknown spring type %d", type);
  MHIP_REQUIRE(m == 0 || pairs, MHIP_ERR_INVALID_ARGUMENT, "pairs is null");
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit spring endpoints");
  MHIP_REQUIRE(m < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many springs for 31-bit incidence entries");
  const char* rname = type == MHIP_SPRING_FENE ? "r_max" : "rest length";
  // host arrays: every spring is checked here, before anything reaches the device
  auto k_ok = [](double v) { return std::isfinite(v) && v >= 0.0; };
  auto r_ok = [type](double v) { return std::isfinite(v) && (type == MHIP_SPRING_FENE ? v > 0.0 : v >= 0.0); };
  MHIP_REQUIRE(k || k_ok(k_scalar), MHIP_ERR_INVALID_ARGUMENT, "spring constant k must be finite and >= 0, got %g",
               k_scalar);
  MHIP_REQUIRE(r || r_ok(r_scalar), MHIP_ERR_INVALID_ARGUMENT, "%s must be finite and %s 0, got %g", rname,
               type == MHIP_SPRING_FENE ? ">" : ">=", r_scalar);
  for (size_t s = 0; s < m; ++s) {
    const int32_t i = pairs[2 * s], j = pairs[2 * s + 1];
    MHIP_REQUIRE(i >= 0 && j >= 0 && static_cast<size_t>(i) < n && static_cast<size_t>(j) < n,
                 MHIP_ERR_INVALID_ARGUMENT, "spring %zu joins (%d, %d): an index outside [0, %zu)", s, i, j, n);
    MHIP_REQUIRE(i != j, MHIP_ERR_INVALID_ARGUMENT, "spring %zu joins body %d to itself", s, i);
    if (k) MHIP_REQUIRE(k_ok(k[s]), MHIP_ERR_INVALID_ARGUMENT, "spring %zu: k must be finite and >= 0, got %g", s, k[s]);
    if (r) MHIP_REQUIRE(r_ok(r[s]), MHIP_ERR_INVALID_ARGUMENT, "spring %zu: %s must be finite and %s 0, got %g", s, rname,
                        type == MHIP_SPRING_FENE ? ">" : ">=", r[s]);
  }
  auto h = std::make_unique<mhip_springs>();
  h->n = n;
  h->m = m;
  h->type = type;
  h->k0 = k_scalar;
  h->r0 = r_scalar;
  h->k_array = k != nullptr;
  h->r_array = r != nullptr;
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
  dispatch<MHIP_SPRING_FENE, MHIP_SPRING_HOOKEAN>(h->type, [&](auto type) {
    dispatch_bools(kk != nullptr, rr != nullptr, [&](auto ka, auto ra) {
      k_spring_force<decltype(type)::value, decltype(ka)::value, decltype(ra)::value><<<grid, kBlock, 0, s>>>(
          h->n, ptr, ent, p2, center, kk, h->k0, rr, h->r0, force, overstretched, mx);
    });
  });
  MHIP_LAUNCH_CHECK();
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
