// active.hip -- the active euchromatin force dipoles of the reference's HP1 app: every listed spring switches on and off
// as a two-state Poisson process and, while on, pushes its two beads apart with a force of constant magnitude
// (scrap/.../HP1.cpp:2796-2826 initial timers, :3770-3833 sampling, :3835-3853 timers, :4286-4354 forces).
//   sample    one lane per spring: a spring whose elapsed time reached its next switching time draws one Philox
//             uniform, flips its state and draws the dwell time of the new state; the others draw nothing
//   force     one lane per body over a body -> spring incidence built once (count, scan, fill, per-body sort as
//             chain.hip), ascending spring index from +0.0, no atomics on forces
//   advance   elapsed += dt
// All elementwise or per-body gathers of a few rows: HBM bound.
#include "mhip_internal.hpp"
#include "force_device.hpp"

#include <cmath>
#include <vector>

namespace mhip {

// u = (philox_u53 + 1) 2^-53 in (0, 1] from block 0 at (key, counter): log(u) is finite
__device__ inline double active_uniform(uint64_t key, uint64_t ctr) {
  return static_cast<double>(philox_u53(philox_draw(key, ctr, 0u)) + 1) * 0x1p-53;
}

// every spring inactive, its first switching time drawn at the rate kon (HP1.cpp:2796-2826)
__global__ void __launch_bounds__(kBlock)
    k_active_init(size_t m, const uint64_t* __restrict__ keys, uint64_t* __restrict__ ctrs, double inv_kon,
                  int32_t* __restrict__ state, double* __restrict__ next_time, double* __restrict__ elapsed) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < m; s += (size_t)gridDim.x * blockDim.x) {
    const uint64_t ctr = ctrs[s];
    state[s] = 0;
    next_time[s] = -log(active_uniform(keys[s], ctr)) * inv_kon;
    elapsed[s] = 0.0;
    ctrs[s] = ctr + 1;
  }
}

__global__ void __launch_bounds__(kBlock)
    k_active_sample(size_t m, const uint64_t* __restrict__ keys, uint64_t* __restrict__ ctrs, double inv_kon,
                    double inv_koff, int32_t* __restrict__ state, double* __restrict__ next_time,
                    double* __restrict__ elapsed, int* __restrict__ switches) {
  int on = 0, off = 0;
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < m; s += (size_t)gridDim.x * blockDim.x) {
    if (!(elapsed[s] >= next_time[s])) continue;
    const uint64_t ctr = ctrs[s];
    const double u = active_uniform(keys[s], ctr);
    ctrs[s] = ctr + 1;
    if (state[s] == 0) {  // HP1.cpp:3806-3810
      state[s] = 1;
      next_time[s] = -log(u) * inv_koff;
      ++on;
    } else {              // :3811-3815
      state[s] = 0;
      next_time[s] = -log(u) * inv_kon;
      ++off;
    }
    elapsed[s] = 0.0;
  }
  wave_stat_add(on, &switches[0]);
  wave_stat_add(off, &switches[1]);
}

__global__ void __launch_bounds__(kBlock) k_active_advance(size_t m, double dt, double* __restrict__ elapsed) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < m; s += (size_t)gridDim.x * blockDim.x)
    elapsed[s] = elapsed[s] + dt;
}

__global__ void __launch_bounds__(kBlock) k_active_renumber(size_t m, const int32_t* __restrict__ new_of_old,
                                                           int2* __restrict__ pairs) {
  for (size_t s = blockIdx.x * (size_t)blockDim.x + threadIdx.x; s < m; s += (size_t)gridDim.x * blockDim.x) {
    const int2 p = pairs[s];
    pairs[s] = make_int2(new_of_old[p.x], new_of_old[p.y]);
  }
}

// One body per lane: its active springs in ascending index.  nvec = x_j - x_i, nsqr folded left to right,
// t = (sigma / sqrt(nsqr)) nvec in the same operations at both ends: body i receives -t, body j +t (HP1.cpp:4325-4347).
template <bool ACCUMULATE>
__global__ void __launch_bounds__(kBlock)
    k_active_force(size_t n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                   const int2* __restrict__ pairs, const int32_t* __restrict__ state,
                   const double* __restrict__ center, double sigma, double* __restrict__ force,
                   int* __restrict__ active) {
  int count = 0;
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    V3 f{0.0, 0.0, 0.0};
    bool any = false;
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    for (int32_t e = lo; e < hi; ++e) {
      const int32_t en = ent[e];
      const int32_t s = en >> 1;
      if (state[s] != 1) continue;
      any = true;
      const int2 p = pairs[s];
      const V3 nv = load3(center, p.y) - load3(center, p.x);
      const double nsqr = nv.x * nv.x + nv.y * nv.y + nv.z * nv.z;
      const V3 t = (sigma / sqrt(nsqr)) * nv;
      if (en & 1) {
        f = f + t;
      } else {
        f = f - t;
        ++count;  // a spring is counted at its first end
      }
    }
    if (ACCUMULATE && !any) continue;  // untouched without an active spring
    write_force<ACCUMULATE>(force, b, f);
  }
  wave_stat_add(count, active);
}

}  // namespace mhip

using namespace mhip;

struct mhip_active_springs {
  size_t n = 0, m = 0;
  double sigma = 0.0, inv_kon = 0.0, inv_koff = 0.0;
  HandleBuffer pairs, keys, ctrs, state, next_time, elapsed, ptr, ent, cursor, ws;
};

namespace {

int build_lists(mhip_active_springs* h, hipStream_t s) {
  return build_incidence(h->n, h->m, PairEnds{h->pairs.as<int2>()}, h->cursor.as<int32_t>(), h->ptr.as<int32_t>(),
                         h->ent.as<int32_t>(), h->ws.ptr, s);
}

}  // namespace

extern "C" {

int mhip_active_springs_create(mhip_active_springs_t* handle, size_t n, size_t m, const int32_t* pairs, double sigma,
                               double kon, double koff, const uint64_t* keys, const uint64_t* counters,
                               mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(m == 0 || pairs, MHIP_ERR_INVALID_ARGUMENT, "pairs is null");
  MHIP_REQUIRE(n < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit spring endpoints");
  MHIP_REQUIRE(m < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many springs for 31-bit incidence entries");
  MHIP_REQUIRE(std::isfinite(sigma), MHIP_ERR_INVALID_ARGUMENT, "sigma must be finite, got %g", sigma);
  MHIP_REQUIRE(std::isfinite(kon) && kon > 0.0, MHIP_ERR_INVALID_ARGUMENT, "kon must be finite and > 0, got %g", kon);
  MHIP_REQUIRE(std::isfinite(koff) && koff > 0.0, MHIP_ERR_INVALID_ARGUMENT, "koff must be finite and > 0, got %g",
               koff);
  // host arrays: every spring is checked here, before anything reaches the device
  for (size_t s = 0; s < m; ++s) {
    const int32_t i = pairs[2 * s], j = pairs[2 * s + 1];
    MHIP_REQUIRE(i >= 0 && j >= 0 && static_cast<size_t>(i) < n && static_cast<size_t>(j) < n,
                 MHIP_ERR_INVALID_ARGUMENT, "active spring %zu joins (%d, %d): an index outside [0, %zu)", s, i, j, n);
    MHIP_REQUIRE(i != j, MHIP_ERR_INVALID_ARGUMENT, "active spring %zu joins body %d to itself", s, i);
    if (keys)
      MHIP_REQUIRE(keys[s] < (1ull << 63), MHIP_ERR_INVALID_ARGUMENT, "active spring %zu: key outside [0, 2^63)", s);
    if (counters)
      MHIP_REQUIRE(counters[s] < (1ull << 63), MHIP_ERR_INVALID_ARGUMENT, "active spring %zu: counter outside [0, 2^63)",
                   s);
  }
  auto h = std::make_unique<mhip_active_springs>();
  h->n = n;
  h->m = m;
  h->sigma = sigma;
  h->inv_kon = 1.0 / kon;
  h->inv_koff = 1.0 / koff;
  hipStream_t s = as_stream(stream);
  int e = MHIP_SUCCESS;
  if ((e = h->ptr.reserve((n + 1) * sizeof(int32_t))) || (e = h->cursor.reserve((n + 1) * sizeof(int32_t))) ||
      (e = h->pairs.reserve(2 * m * sizeof(int32_t) + 8)) || (e = h->ent.reserve(2 * m * sizeof(int32_t) + 8)) ||
      (e = h->ws.reserve(scan_workspace_bytes(n) + 8)) || (e = h->keys.reserve(m * sizeof(uint64_t) + 8)) ||
      (e = h->ctrs.reserve(m * sizeof(uint64_t) + 8)) || (e = h->state.reserve(m * sizeof(int32_t) + 8)) ||
      (e = h->next_time.reserve(m * sizeof(double) + 8)) || (e = h->elapsed.reserve(m * sizeof(double) + 8)))
    return e;
  std::vector<uint64_t> seq;
  if (m > 0) {
    if (!keys) {  // the spring's index keys its stream
      seq.resize(m);
      for (size_t i = 0; i < m; ++i) seq[i] = i;
    }
    if ((e = upload(__func__, h->pairs, pairs, 2 * m * sizeof(int32_t), s)) ||
        (e = upload(__func__, h->keys, keys ? keys : seq.data(), m * sizeof(uint64_t), s)))
      return e;
    if (counters) e = upload(__func__, h->ctrs, counters, m * sizeof(uint64_t), s);
    else e = hip_status(__func__, hipMemsetAsync(h->ctrs.ptr, 0, m * sizeof(uint64_t), s));
    if (e) return e;
    k_active_init<<<grid_for(m), kBlock, 0, s>>>(m, h->keys.as<uint64_t>(), h->ctrs.as<uint64_t>(), h->inv_kon,
                                                h->state.as<int32_t>(), h->next_time.as<double>(),
                                                h->elapsed.as<double>());
    if ((e = hip_status(__func__, hipGetLastError()))) return e;
  }
  if ((e = build_lists(h.get(), s))) return e;
  // the caller's host arrays (and seq) may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_active_springs_destroy(mhip_active_springs_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_active_springs_sample(mhip_active_springs_t h, int* switches, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  MHIP_REQUIRE(switches != nullptr, MHIP_ERR_INVALID_ARGUMENT, "switches is null");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(switches, 0, 2 * sizeof(int), s));
  if (h->m == 0) return MHIP_SUCCESS;
  k_active_sample<<<grid_for(h->m), kBlock, 0, s>>>(h->m, h->keys.as<uint64_t>(), h->ctrs.as<uint64_t>(), h->inv_kon,
                                                   h->inv_koff, h->state.as<int32_t>(), h->next_time.as<double>(),
                                                   h->elapsed.as<double>(), switches);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_active_springs_force(mhip_active_springs_t h, const double* center, double* force, int accumulate, int* active,
                              mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  MHIP_REQUIRE(h->n == 0 || (center && force), MHIP_ERR_INVALID_ARGUMENT, "center / force is null");
  hipStream_t s = as_stream(stream);
  if (active) MHIP_HIP(hipMemsetAsync(active, 0, sizeof(int), s));
  if (h->n == 0) return MHIP_SUCCESS;
  const unsigned grid = grid_for(h->n);
  dispatch<true, false>(accumulate != 0, [&](auto acc) {
    k_active_force<decltype(acc)::value><<<grid, kBlock, 0, s>>>(h->n, h->ptr.as<int32_t>(), h->ent.as<int32_t>(),
                                                                 h->pairs.as<int2>(), h->state.as<int32_t>(), center,
                                                                 h->sigma, force, active);
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_active_springs_advance(mhip_active_springs_t h, double dt, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  if (h->m == 0) return MHIP_SUCCESS;
  k_active_advance<<<grid_for(h->m), kBlock, 0, as_stream(stream)>>>(h->m, dt, h->elapsed.as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_active_springs_get_state(mhip_active_springs_t h, int32_t* state, double* next_time, double* elapsed,
                                  uint64_t* counters, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  hipStream_t s = as_stream(stream);
  const size_t m = h->m;
  if (m == 0) return MHIP_SUCCESS;
  if (state) MHIP_HIP(hipMemcpyAsync(state, h->state.ptr, m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (next_time) MHIP_HIP(hipMemcpyAsync(next_time, h->next_time.ptr, m * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (elapsed) MHIP_HIP(hipMemcpyAsync(elapsed, h->elapsed.ptr, m * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (counters) MHIP_HIP(hipMemcpyAsync(counters, h->ctrs.ptr, m * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  return MHIP_SUCCESS;
}

int mhip_active_springs_set_state(mhip_active_springs_t h, const int32_t* state, const double* next_time,
                                  const double* elapsed, const uint64_t* counters, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  hipStream_t s = as_stream(stream);
  const size_t m = h->m;
  if (m == 0) return MHIP_SUCCESS;
  if (state) MHIP_HIP(hipMemcpyAsync(h->state.ptr, state, m * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
  if (next_time) MHIP_HIP(hipMemcpyAsync(h->next_time.ptr, next_time, m * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (elapsed) MHIP_HIP(hipMemcpyAsync(h->elapsed.ptr, elapsed, m * sizeof(double), hipMemcpyDeviceToDevice, s));
  if (counters) MHIP_HIP(hipMemcpyAsync(h->ctrs.ptr, counters, m * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
  return MHIP_SUCCESS;
}

int mhip_active_springs_renumber(mhip_active_springs_t h, const int32_t* new_of_old, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "active springs handle is null");
  MHIP_REQUIRE(h->n == 0 || new_of_old, MHIP_ERR_INVALID_ARGUMENT, "new_of_old is null");
  hipStream_t s = as_stream(stream);
  if (h->m > 0) {
    k_active_renumber<<<grid_for(h->m), kBlock, 0, s>>>(h->m, new_of_old, h->pairs.as<int2>());
    MHIP_LAUNCH_CHECK();
  }
  return build_lists(h, s);
}

}  // extern "C"
