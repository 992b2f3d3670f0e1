// growth.hip -- the body population of the reference's bacterial colony loop changes on the device
// (scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:1033-1080):
//   divide_bacteria (:926-966; subdivide_flagged_spherocylinders :219-300, subdivide_spherocylinders :159-210)
//   grow_bacteria (:905-920), and the rebuild rule of growing bodies, check_update_neighbor_list (:685-748).
// Selection is an order-preserving wavefront-ballot compaction (the filter_view structure of halo.hip); division and
// growth are one elementwise pass; the corner test is one elementwise pass with a wave-or.  fp64, no contraction.
#include "geom_device.hpp"

namespace mhip {

struct GrowthScratch {
  DeviceBuffer counts, bases, scanws, flag;
  int* host = nullptr;  // pinned
  int ensure(size_t ntiles) {
    if (int e = counts.reserve((ntiles + 2) * sizeof(int32_t))) return e;
    if (int e = bases.reserve((ntiles + 2) * sizeof(int32_t))) return e;
    if (int e = scanws.reserve(scan_workspace_bytes(ntiles + 2) + 64)) return e;
    if (int e = flag.reserve(sizeof(int))) return e;
    if (!host) MHIP_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), 64));
    return MHIP_SUCCESS;
  }
};
GrowthScratch& growth_scratch() {
  thread_local GrowthScratch s;
  return s;
}

// ---- selection: ascending indices of the bodies with length > division_length ---------------------------------------
// A workgroup owns kDivTile consecutive bodies in kDivRounds rounds of kBlock, so each wave ballots 64 CONSECUTIVE
// bodies: the popcount of the mask is the segment's count, a body's slot in the segment the popcount below its lane.
// Pass 1 writes one count per tile; exclusive_scan_i32 turns them into tile bases (the partial_sum of :243-254);
// pass 2 re-evaluates the predicate and writes parent_of in index order.  The strict test: NaN and L == D never divide.
constexpr int kDivRounds = 4;
constexpr int kDivTile = kBlock * kDivRounds;
constexpr int kDivSegs = kDivRounds * (kBlock / 64);

__global__ void __launch_bounds__(kBlock) k_divide_count(size_t n, const double* __restrict__ length, double division,
                                                        int32_t* __restrict__ tile_count) {
  __shared__ int seg[kDivSegs];
  const size_t base = (size_t)blockIdx.x * kDivTile;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < kDivRounds; ++r) {
    const size_t i = base + (size_t)r * kBlock + threadIdx.x;
    const bool div = (i < n) && (length[i] > division);
    const unsigned long long mask = __ballot(div);
    if ((threadIdx.x & 63) == 0) seg[r * (kBlock / 64) + wave] = __popcll(mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
    for (int k = 0; k < kDivSegs; ++k) total += seg[k];
    tile_count[blockIdx.x] = total;
  }
}

__global__ void __launch_bounds__(kBlock) k_divide_emit(size_t n, const double* __restrict__ length, double division,
                                                       const int32_t* __restrict__ tile_base,
                                                       int32_t* __restrict__ parent_of) {
  __shared__ int seg[kDivSegs];
  const size_t base = (size_t)blockIdx.x * kDivTile;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bool div[kDivRounds];
  unsigned long long mask[kDivRounds];
#pragma unroll
  for (int r = 0; r < kDivRounds; ++r) {
    const size_t i = base + (size_t)r * kBlock + threadIdx.x;
    div[r] = (i < n) && (length[i] > division);
    mask[r] = __ballot(div[r]);
    if (lane == 0) seg[r * (kBlock / 64) + wave] = __popcll(mask[r]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // exclusive prefix over the tile's segments
    int run = 0;
    for (int k = 0; k < kDivSegs; ++k) {
      const int c = seg[k];
      seg[k] = run;
      run += c;
    }
  }
  __syncthreads();
  const int out0 = tile_base[blockIdx.x];
#pragma unroll
  for (int r = 0; r < kDivRounds; ++r) {
    if (!div[r]) continue;
    const int below = __popcll(mask[r] & ((1ull << lane) - 1ull));
    parent_of[out0 + seg[r * (kBlock / 64) + wave] + below] = static_cast<int32_t>(base + (size_t)r * kBlock + threadIdx.x);
  }
}

// ---- division and growth: one pass over the n bodies that were there before the step --------------------------------
// Body i finds its birth rank k by a binary search of the ascending parent_of[0, nb) (a few dozen entries at steady
// state, cache resident).  A body that does not divide reads and writes its length only; a dividing body writes its own
// row and row n + k of its child, both already grown.  Every row is written by exactly one lane: no atomics, no second
// pass.  Rows written: [0, n) and [n, n + nb), whatever parent_of holds.
__device__ inline int find_birth(const int32_t* __restrict__ parent_of, int nb, int i) {
  int lo = 0, hi = nb;  // lower_bound
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (parent_of[mid] < i)
      lo = mid + 1;
    else
      hi = mid;
  }
  return (lo < nb && parent_of[lo] == i) ? lo : -1;
}

template <bool PERIODIC>
__global__ void __launch_bounds__(kBlock)
    k_divide_grow(size_t n, int nb, const int32_t* __restrict__ parent_of, double g, Periodic pm,
                  double* __restrict__ center, double* __restrict__ quat, double* __restrict__ radius,
                  double* __restrict__ length) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int k = nb > 0 ? find_birth(parent_of, nb, static_cast<int>(i)) : -1;
    if (k < 0) {  // grow_bacteria: L += dt * rate (:917)
      length[i] = length[i] + g;
      continue;
    }
    // subdivide_spherocylinders (:190-209) along the library's rod axis q * zhat (geom_device.hpp rod_half_axis)
    const Quat q{quat[4 * i], quat[4 * i + 1], quat[4 * i + 2], quat[4 * i + 3]};
    const V3 c = load3(center, i);
    const double L = length[i], r = radius[i];
    const V3 t = qrot(q, V3{0.0, 0.0, 1.0});
    const double cl = 0.5 * L - r;
    const double s = r + 0.5 * cl;
    const V3 off{t.x * s, t.y * s, t.z * s};
    V3 child = c + off, parent = c - off;
    if (PERIODIC) {  // wrap_rigid of both rods (periodicity.hpp:1094-1113)
      child = periodic_wrap(pm, child);
      parent = periodic_wrap(pm, parent);
    }
    const double grown = cl + g;
    const size_t j = n + static_cast<size_t>(k);
    store3(center, i, parent);
    length[i] = grown;
    store3(center, j, child);
    for (int a = 0; a < 4; ++a) quat[4 * j + a] = quat[4 * i + a];
    radius[j] = r;
    length[j] = grown;
  }
}

// ---- check_update_neighbor_list (:710-741): some min or max corner moved by |d|^2 >= threshold^2 -------------------
__global__ void __launch_bounds__(kBlock) k_aabb_moved(size_t n, const double* __restrict__ aabb,
                                                      const double* __restrict__ ref, double thr2,
                                                      int* __restrict__ flag) {
  int moved = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double* a = aabb + 6 * i;
    const double* b = ref + 6 * i;
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
    const double d3 = a[3] - b[3], d4 = a[4] - b[4], d5 = a[5] - b[5];
    const double lo2 = d0 * d0 + d1 * d1 + d2 * d2;  // left to right, as :727-735
    const double hi2 = d3 * d3 + d4 * d4 + d5 * d5;
    moved |= (lo2 >= thr2 || hi2 >= thr2) ? 1 : 0;
  }
  moved = wave_or(moved);
  if ((threadIdx.x & 63) == 0 && moved) atomicOr(flag, 1);
}

}  // namespace mhip

using namespace mhip;

extern "C" {

int mhip_select_dividing(size_t n, const double* length, double division_length, int32_t* parent_of,
                         size_t* num_born, mhip_stream_t stream) {
  MHIP_REQUIRE(num_born != nullptr, MHIP_ERR_INVALID_ARGUMENT, "num_born is null");
  *num_born = 0;
  MHIP_REQUIRE(division_length >= 0.0 && std::isfinite(division_length), MHIP_ERR_INVALID_ARGUMENT,
               "division_length must be finite and >= 0, got %g", division_length);
  MHIP_REQUIRE(n == 0 || (length && parent_of), MHIP_ERR_INVALID_ARGUMENT, "length / parent_of is null");
  MHIP_REQUIRE(n < (1u << 30), MHIP_ERR_RUNTIME, "too many bodies");
  if (n == 0) return MHIP_SUCCESS;
  TraceRange trace_range("divide_bacteria (mark + partial_sum)");
  hipStream_t s = as_stream(stream);
  GrowthScratch& gs = growth_scratch();
  const size_t ntiles = (n + kDivTile - 1) / kDivTile;
  if (int e = gs.ensure(ntiles)) return e;
  int32_t* counts = gs.counts.as<int32_t>();
  int32_t* bases = gs.bases.as<int32_t>();
  k_divide_count<<<static_cast<unsigned>(ntiles), kBlock, 0, s>>>(n, length, division_length, counts);
  MHIP_LAUNCH_CHECK();
  if (int e = exclusive_scan_i32(counts, bases, ntiles, gs.scanws.ptr, s)) return e;
  k_divide_emit<<<static_cast<unsigned>(ntiles), kBlock, 0, s>>>(n, length, division_length, bases, parent_of);
  MHIP_LAUNCH_CHECK();
  MHIP_HIP(hipMemcpyAsync(gs.host, bases + ntiles, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  MHIP_HIP(hipStreamSynchronize(s));
  *num_born = static_cast<size_t>(gs.host[0]);
  return MHIP_SUCCESS;
}

int mhip_divide_grow_spherocylinders(size_t n, size_t num_born, const int32_t* parent_of, double dt,
                                     double growth_rate, const double* box, double* center, double* quat,
                                     double* radius, double* length, mhip_stream_t stream) {
  MHIP_REQUIRE(dt >= 0.0 && std::isfinite(dt), MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  MHIP_REQUIRE(growth_rate >= 0.0 && std::isfinite(growth_rate), MHIP_ERR_INVALID_ARGUMENT,
               "growth_rate must be finite and >= 0, got %g", growth_rate);
  MHIP_REQUIRE(num_born <= n, MHIP_ERR_INVALID_ARGUMENT, "num_born %zu exceeds n %zu", num_born, n);
  MHIP_REQUIRE(num_born == 0 || parent_of, MHIP_ERR_INVALID_ARGUMENT, "parent_of is null");
  MHIP_REQUIRE(n == 0 || length, MHIP_ERR_INVALID_ARGUMENT, "length is null");
  MHIP_REQUIRE(num_born == 0 || (center && quat && radius), MHIP_ERR_INVALID_ARGUMENT,
               "center / quat / radius is null");
  MHIP_REQUIRE(box == nullptr || (box[0] > 0 && box[1] > 0 && box[2] > 0 && std::isfinite(box[0]) &&
                                  std::isfinite(box[1]) && std::isfinite(box[2])),
               MHIP_ERR_INVALID_ARGUMENT, "periodic box must be positive and finite");
  MHIP_REQUIRE(n < (1u << 30), MHIP_ERR_RUNTIME, "too many bodies");
  if (n == 0) return MHIP_SUCCESS;
  TraceRange trace_range("grow_bacteria (subdivide + grow)");
  const double g = dt * growth_rate;  // once, as timestep_size * bacteria_growth_rate (:917)
  const int nb = static_cast<int>(num_born);
  hipStream_t s = as_stream(stream);
  if (box)
    k_divide_grow<true><<<grid_for(n), kBlock, 0, s>>>(n, nb, parent_of, g, make_periodic(box), center, quat, radius,
                                                       length);
  else
    k_divide_grow<false><<<grid_for(n), kBlock, 0, s>>>(n, nb, parent_of, g, Periodic{}, center, quat, radius, length);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_aabb_moved(size_t n, const double* aabb, const double* aabb_ref, double threshold, int* flag,
                    mhip_stream_t stream) {
  MHIP_REQUIRE(flag != nullptr, MHIP_ERR_INVALID_ARGUMENT, "flag is null");
  *flag = 0;
  MHIP_REQUIRE(threshold >= 0.0 && std::isfinite(threshold), MHIP_ERR_INVALID_ARGUMENT,
               "threshold must be finite and >= 0, got %g", threshold);
  MHIP_REQUIRE(n == 0 || (aabb && aabb_ref), MHIP_ERR_INVALID_ARGUMENT, "aabb / aabb_ref is null");
  if (n == 0) return MHIP_SUCCESS;
  TraceRange trace_range("check_update_neighbor_list");
  hipStream_t s = as_stream(stream);
  GrowthScratch& gs = growth_scratch();
  if (int e = gs.ensure(1)) return e;
  int* d = gs.flag.as<int>();
  MHIP_HIP(hipMemsetAsync(d, 0, sizeof(int), s));
  k_aabb_moved<<<grid_for(n), kBlock, 0, s>>>(n, aabb, aabb_ref, threshold * threshold, d);
  MHIP_LAUNCH_CHECK();
  MHIP_HIP(hipMemcpyAsync(gs.host, d, sizeof(int), hipMemcpyDeviceToHost, s));
  MHIP_HIP(hipStreamSynchronize(s));
  *flag = gs.host[0] != 0 ? 1 : 0;
  return MHIP_SUCCESS;
}

}  // extern "C"
