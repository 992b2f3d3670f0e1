// filament_contact.hip -- frictional Hertzian contacts between the segments of centerline-twist filaments: the contact half
// of the force stage of the reference's sperm apps (compute_hertzian_contact_force_and_torque,
// scrap/parameter_interface/alens/tests/performance_tests/CollidingOverdampedFrictionalSperm.cpp:1553-1731, run in the
// loop at :2013-2021).  A segment is indexed by its left node, as every per-edge array of filament.hip: N rows, the row of
// a filament's last node a degenerate record that the search never lists (mhip_broadphase_set_sets).
//   segment view   .../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161          one node per lane
//   velocity copy  the StateN velocities the force reads (FHC :388)                      one node per lane
//   linker pass    ...SpherocylinderSegmentSpherocylinderSegmentLinker.cpp:204-237 (distance) and
//                  ...SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp (FHC) :357-380, :429-516
//                  in ONE pass: normal, contact points and arclengths never travel through HBM          one linker per lane
//   reduction      .../linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221: a gather, no atomic on
//                  a force; a tile of nodes per workgroup with a one-segment halo in LDS
// Byte counts and the accumulation order: DESIGN.md 5k.
#include "segment_linkers.hpp"
#include "../../include/mundy_hip_filament_inertial.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mhip {

constexpr int kTile = kBlock;

// seg[i] = (x_i, x_{i+1}, r_i, 0) and the box of reach r_i; a filament's last node: (x_i, x_i, r_i, 0)
__global__ void __launch_bounds__(kBlock)
    k_segment_view(size_t n, const uint8_t* __restrict__ has_right, const double* __restrict__ x,
                   const double* __restrict__ radius, double skin, double* __restrict__ seg, double* __restrict__ aabb) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const V3 x0 = load3(x, i);
    const V3 x1 = has_right[i] ? load3(x, i + 1) : x0;  // has_right: i + 1 < n
    const double r = radius[i];
    store_segment_view(seg, aabb, i, x0, x1, r, r, skin);
  }
}

// v(t) as the force reads it: apply_monolayer has zeroed component 0 before rotate_field_states (:1999-2003)
template <bool MONOLAYER>
__global__ void __launch_bounds__(kBlock)
    k_save_velocity(size_t n, const double* __restrict__ vel, double* __restrict__ vel_prev) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    V3 v = load3(vel, i);
    if (MONOLAYER) v.x = 0.0;
    store3(vel_prev, i, v);
  }
}

// get_contact_point_velocity, FHC :357-380: the velocity of the point cp of a segment whose end nodes move with v0, v1
__device__ inline V3 segment_point_velocity(V3 x0, V3 x1, V3 v0, V3 v1, V3 cp) {
  const V3 rv = v1 - v0, lc = cp - x0, lr = x1 - x0;
  const double iL = 1.0 / norm(lr);
  const V3 t = lr * iL;
  const V3 term1 = (dot(lc, rv) * t) * iL;
  const V3 term2 = (dot(lc, t) * (rv - dot(t, rv) * t)) * iL;
  return (v0 + term1) + term2;
}
// One linker per lane and pass, grid-stride.  stats[0]: bits of max(0, -sep) over the contact branch; stats[1]: number of
// contacts whose tangential force was capped.  One atomic per workgroup for each.
// FRICTION = false: the frictionless law of ...SpherocylinderSegmentSpherocylinderSegmentHertzianContact.cpp:208-225
// (mundy_hip_filament_inertial.h): the branch is sep < 0, the force on the left segment (-F) n with hertz_force_magnitude,
// no velocity is read, tang_disp stays +0.0 and nothing is counted.
template <bool FRICTION>
__global__ void __launch_bounds__(kBlock)
    k_filament_linkers(size_t C, size_t N, const int* __restrict__ pairs, const double* __restrict__ seg,
                       const double* __restrict__ vel_prev, double E0, double nu0, mhip_hertz_friction_params prm,
                       double* __restrict__ sep, double* __restrict__ tang_disp, double* __restrict__ force,
                       double* __restrict__ share, unsigned long long* __restrict__ stats) {
  double dmax = 0.0;
  unsigned capped = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < C; c += (size_t)gridDim.x * blockDim.x) {
    const int2 p = load_pair_once(pairs, c);
    // a segment's right node is p + 1: row N - 1 is the last node of the last filament, never a segment
    if (N < 2 || static_cast<unsigned>(p.x) >= N - 1 || static_cast<unsigned>(p.y) >= N - 1) {
      refuse_linker(sep, force, share, c);
      store_row_nan(tang_disp, c);
      continue;
    }
    const SegmentLinker k = measure_linker(seg, p);
    const double s = k.s;
    sep[c] = s;
    // no contact: the history is reset (FHC :433-435), force and shares are +0.0
    if (FRICTION ? s > 0.0 : !(s < 0.0)) {
      reset_row(tang_disp, c);
      reset_linker(force, share, c);
      continue;
    }
    const V3 n = k.normal();
    if (!FRICTION) {
      reset_row(tang_disp, c);
      store_linker_force(force, share, c, k, (-segment_hertz(E0, nu0, k.a.r, k.b.r, s)) * n);  // :225
      dmax = -s > dmax ? -s : dmax;
      continue;
    }
    const V3 vi = segment_point_velocity(k.a.p0, k.a.p1, load3(vel_prev, p.x), load3(vel_prev, (size_t)p.x + 1), k.r.cp1);
    const V3 vj = segment_point_velocity(k.b.p0, k.b.p1, load3(vel_prev, p.y), load3(vel_prev, (size_t)p.y + 1), k.r.cp2);
    HertzPair h;  // hertz_pair's expressions, the radii being the segments' and the material one scalar pair
    h.ri = k.a.r, h.rj = k.b.r;
    h.Ei = E0, h.Ej = E0, h.vi = nu0, h.vj = nu0;
    h.Rs = (h.ri * h.rj) / (h.ri + h.rj);
    h.Es = (h.Ei * h.Ej) / (h.Ej - h.Ej * h.vi * h.vi + h.Ei - h.Ei * h.vj * h.vj);
    const FrictionContact f = hertz_friction_law(vj - vi, n, s, h, prm, load3(tang_disp, c));
    capped += f.capped ? 1u : 0u;
    store3(tang_disp, c, f.td);
    store_linker_force(force, share, c, k, f.force);
    dmax = -s > dmax ? -s : dmax;
  }
  block_stat_max(dmax, stats);
  block_stat_add(capped, stats + 1);
}

// Per tile of kTile nodes [s, s + kTile): the sums (a0, a1) of the segments s - 1 .. s + kTile - 1 are formed once each
// into LDS by sum_segment_entries (a separated linker, sep > 0, is passed over) -- then node i adds
// ((external or +0.0) + a0[i]) + a1[i - 1], a term whose segment does not exist left out.
// A segment's sums are one function of the same inputs in whichever tile they are formed.
template <bool EXTERNAL>
__global__ void __launch_bounds__(kBlock)
    k_filament_contact_reduce(long long n, long long tiles, const uint8_t* __restrict__ has_right,
                              const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                              const double* __restrict__ sep, const double* __restrict__ force,
                              const double* __restrict__ share,
                              const double* __restrict__ external, double* __restrict__ node_force) {
  __shared__ double A[6][kTile + 1];  // slot k = segment s - 1 + k; rows 0-2: a0, rows 3-5: a1
  const int tid = threadIdx.x;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long s = tile * kTile;
    for (int k = tid; k < kTile + 1; k += kBlock) {
      const long long e = s - 1 + k;
      SegmentSums q{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
      if (e >= 0 && e < n)  // 8 bytes of sep stand for a separated linker's rows
        q = sum_segment_entries(ptr, ent, static_cast<size_t>(e), force, share, [&](size_t c) { return sep[c] > 0.0; });
      A[0][k] = q.a0.x, A[1][k] = q.a0.y, A[2][k] = q.a0.z;
      A[3][k] = q.a1.x, A[4][k] = q.a1.y, A[5][k] = q.a1.z;
    }
    __syncthreads();
    const long long i = s + tid;
    if (i < n) {
      V3 f = EXTERNAL ? load3(external, i) : V3{0.0, 0.0, 0.0};
      if (has_right[i]) f = f + V3{A[0][tid + 1], A[1][tid + 1], A[2][tid + 1]};
      if (i > 0 && has_right[i - 1]) f = f + V3{A[3][tid], A[4][tid], A[5][tid]};
      store3(node_force, i, f);
    }
    __syncthreads();  // the next tile overwrites the LDS image
  }
}

}  // namespace mhip

using namespace mhip;

struct mhip_filament_contacts {
  mhip_filaments_t filaments = nullptr;
  size_t n = 0;
  mhip_filament_contact_params prm{};
  hipStream_t stream = nullptr;
  bool saved = false;
  int law = MHIP_FILAMENT_CONTACT_FRICTIONAL;  // mundy_hip_filament_inertial.h
  int cur = 0;                                 // which copy of (pairs, hist) is the current list, of length list.c
  LinkerList list;
  HandleBuffer has_right, radius, vel_prev, node_force;
  HandleBuffer pairs[2], hist[2];
};

extern "C" {

int mhip_filament_contacts_create(mhip_filament_contacts_t* handle, mhip_filaments_t filaments, const int32_t* node_ptr,
                                  const double* segment_radius, const mhip_filament_contact_params* params,
                                  mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(params != nullptr, MHIP_ERR_INVALID_ARGUMENT, "params is null");
  const mhip_filament_contact_params& p = *params;
  if (int e = check_linker_params(p.skin, p.youngs_modulus, p.poisson_ratio, true)) return e;
  MHIP_REQUIRE(std::isfinite(p.mu) && p.mu >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "mu must be finite and >= 0, got %g", p.mu);
  MHIP_REQUIRE(std::isfinite(p.normal_damping) && p.normal_damping >= 0.0 && std::isfinite(p.tangential_damping) &&
                   p.tangential_damping >= 0.0,
               MHIP_ERR_INVALID_ARGUMENT, "damping coefficients must be finite and >= 0, got %g, %g", p.normal_damping,
               p.tangential_damping);
  MHIP_REQUIRE(std::isfinite(p.density) && p.density >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "density must be finite and >= 0, got %g", p.density);
  MHIP_REQUIRE(std::isfinite(p.history_dt), MHIP_ERR_INVALID_ARGUMENT, "history_dt must be finite, got %g", p.history_dt);
  MHIP_REQUIRE(p.bonded_exclusion >= 1, MHIP_ERR_INVALID_ARGUMENT, "bonded_exclusion must be >= 1, got %d",
               p.bonded_exclusion);
  MHIP_REQUIRE(filaments != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(node_ptr != nullptr, MHIP_ERR_INVALID_ARGUMENT, "node_ptr is null");
  mhip_filament_fields fields;
  if (int e = mhip_filaments_get(filaments, &fields)) return e;  // (no HIP call)
  const size_t n = fields.num_nodes, F = fields.num_filaments;
  MHIP_REQUIRE(node_ptr[0] == 0 && static_cast<size_t>(node_ptr[F]) == n, MHIP_ERR_INVALID_ARGUMENT,
               "node_ptr does not describe the filaments of the handle (%zu nodes in %zu filaments)", n, F);
  for (size_t f = 0; f < F; ++f)
    MHIP_REQUIRE(node_ptr[f + 1] - node_ptr[f] >= 2, MHIP_ERR_INVALID_ARGUMENT, "filament %zu has fewer than 2 nodes", f);
  if (segment_radius)
    for (size_t i = 0; i < n; ++i)
      if (int e = check_segment_radius(i, segment_radius[i])) return e;
  // who may pair with whom: every real segment is source and target; segments at most bonded_exclusion apart along one
  // filament never pair (DestroyBoundNeighbors.cpp:150-170 for 1)
  std::vector<uint8_t> has_right(n, 0);
  std::vector<int32_t> ex_ptr(n + 1, 0), ex_idx;
  for (size_t f = 0; f < F; ++f) {
    const long long lo = node_ptr[f], last = static_cast<long long>(node_ptr[f + 1]) - 2;  // segments lo .. last
    for (long long i = lo; i <= last; ++i) {
      has_right[i] = 1;
      const long long a = std::max(lo, i - p.bonded_exclusion), b = std::min(last, i + p.bonded_exclusion);
      for (long long j = a; j <= b; ++j)
        if (j != i) ex_idx.push_back(static_cast<int32_t>(j));
      ex_ptr[i + 1] = static_cast<int32_t>(ex_idx.size());
    }
    ex_ptr[last + 2] = static_cast<int32_t>(ex_idx.size());
  }
  for (size_t i = 0; i < n; ++i) ex_ptr[i + 1] = std::max(ex_ptr[i + 1], ex_ptr[i]);
  auto h = std::make_unique<mhip_filament_contacts>();
  h->filaments = filaments;
  h->n = n;
  h->prm = p;
  hipStream_t s = as_stream(stream);
  h->stream = s;
  const size_t d = sizeof(double);
  int e = MHIP_SUCCESS;
  if ((e = h->list.create(__func__, n, n, ex_ptr, ex_idx, s))) return e;
  if ((e = h->has_right.reserve(n + 8)) || (e = h->radius.reserve(n * d + 8)) ||
      (e = h->vel_prev.reserve(3 * n * d + 8)) || (e = h->node_force.reserve(3 * n * d + 8)))
    return e;
  if (n > 0) {
    if ((e = upload(__func__, h->has_right, has_right.data(), n, s))) return e;
    if (segment_radius) {
      if ((e = upload(__func__, h->radius, segment_radius, n * d, s))) return e;
    } else {
      MHIP_HIP(hipMemcpyAsync(h->radius.ptr, fields.radius, n * d, hipMemcpyDeviceToDevice, s));
    }
    MHIP_HIP(hipMemsetAsync(h->vel_prev.ptr, 0, 3 * n * d, s));
    MHIP_HIP(hipMemsetAsync(h->node_force.ptr, 0, 3 * n * d, s));
  }
  if ((e = mhip_broadphase_set_sets(h->list.bp, n, h->has_right.as<unsigned char>(), h->has_right.as<unsigned char>(),
                                    stream)))
    return e;
  // the host arrays built here may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_destroy(mhip_filament_contacts_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_save_velocity(mhip_filament_contacts_t h) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  mhip_filament_fields fields;
  if (int e = mhip_filaments_get(h->filaments, &fields)) return e;
  h->saved = true;
  if (h->n == 0) return MHIP_SUCCESS;
  dispatch<true, false>(h->prm.monolayer != 0, [&](auto ml) {
    k_save_velocity<decltype(ml)::value><<<grid_for(h->n), kBlock, 0, h->stream>>>(h->n, fields.velocity,
                                                                                  h->vel_prev.as<double>());
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_segment_view(mhip_filament_contacts_t h) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  mhip_filament_fields fields;
  if (int e = mhip_filaments_get(h->filaments, &fields)) return e;
  if (h->n == 0) return MHIP_SUCCESS;
  k_segment_view<<<grid_for(h->n), kBlock, 0, h->stream>>>(h->n, h->has_right.as<uint8_t>(), fields.center,
                                                           h->radius.as<double>(), h->prm.skin, h->list.seg.as<double>(),
                                                           h->list.aabb.as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_update(mhip_filament_contacts_t h, int* rebuilt) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  MHIP_REQUIRE(rebuilt != nullptr, MHIP_ERR_INVALID_ARGUMENT, "rebuilt is null");
  *rebuilt = 0;
  if (int e = mhip_filament_contacts_segment_view(h)) return e;
  mhip_filament_fields fields;
  if (int e = mhip_filaments_get(h->filaments, &fields)) return e;
  const size_t n = h->n;
  hipStream_t s = h->stream;
  LinkerList& l = h->list;
  int moved = 1;  // the first call builds
  if (l.has_list)
    if (int e = l.moved(n, h->prm.skin, &moved, s)) return e;
  if (!moved) return MHIP_SUCCESS;
  // rebuild (:1612-1717): every pair of box-overlapping segments that are not neighbours along a filament
  const int old = h->cur, nw = old ^ 1;
  if (int e = l.rebuild(n, fields.center, h->pairs[nw], s, [&](size_t c_new) {
        // surviving linkers keep their tang_disp, new ones start from +0.0
        if (int e = h->hist[nw].reserve(3 * c_new * sizeof(double) + 8)) return e;
        return mhip_contact_history_carry(l.c, h->pairs[old].as<int32_t>(), h->hist[old].as<double>(), nullptr, n, c_new,
                                          h->pairs[nw].as<int32_t>(), h->hist[nw].as<double>(), nullptr,
                                          reinterpret_cast<mhip_stream_t>(s));
      }))
    return e;
  h->cur = nw;
  *rebuilt = 1;
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_linker_pass(mhip_filament_contacts_t h, double dt, void* stats) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  MHIP_REQUIRE(h->saved || h->law == MHIP_FILAMENT_CONTACT_HERTZ, MHIP_ERR_RUNTIME,
               "mhip_filament_contacts_linker_pass before mhip_filament_contacts_save_velocity");
  const LinkerList& l = h->list;
  MHIP_REQUIRE(l.has_list, MHIP_ERR_RUNTIME, "mhip_filament_contacts_linker_pass before mhip_filament_contacts_update");
  hipStream_t s = h->stream;
  MHIP_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s));
  const size_t n = h->n, c = l.c;
  if (n == 0 || c == 0) return MHIP_SUCCESS;
  const mhip_filament_contact_params& p = h->prm;
  const mhip_hertz_friction_params law{p.mu, p.normal_damping, p.tangential_damping, p.density,
                                       p.history_dt < 0.0 ? dt : p.history_dt};
  dispatch<true, false>(h->law == MHIP_FILAMENT_CONTACT_FRICTIONAL, [&](auto fr) {
    k_filament_linkers<decltype(fr)::value><<<grid_for(c), kBlock, 0, s>>>(
        c, n, h->pairs[h->cur].as<int>(), l.seg.as<double>(), h->vel_prev.as<double>(), p.youngs_modulus,
        p.poisson_ratio, law, l.sep.as<double>(), h->hist[h->cur].as<double>(), l.force.as<double>(),
        l.share.as<double>(), static_cast<unsigned long long*>(stats));
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_reduce(mhip_filament_contacts_t h, const double* external_force) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  const LinkerList& l = h->list;
  MHIP_REQUIRE(l.has_list, MHIP_ERR_RUNTIME, "mhip_filament_contacts_reduce before mhip_filament_contacts_update");
  const size_t n = h->n;
  if (n == 0) return MHIP_SUCCESS;
  const long long tiles = static_cast<long long>((n + kTile - 1) / kTile);
  dispatch<true, false>(external_force != nullptr, [&](auto ex) {
    k_filament_contact_reduce<decltype(ex)::value><<<grid_for(n), kBlock, 0, h->stream>>>(
        static_cast<long long>(n), tiles, h->has_right.as<uint8_t>(), l.inc_ptr.as<int32_t>(), l.inc_ent.as<int32_t>(),
        l.sep.as<double>(), l.force.as<double>(), l.share.as<double>(), external_force, h->node_force.as<double>());
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_force(mhip_filament_contacts_t h, double dt, const double* external_force, void* stats) {
  // every refusal comes before the first launch
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  MHIP_REQUIRE(h->saved || h->law == MHIP_FILAMENT_CONTACT_HERTZ, MHIP_ERR_RUNTIME,
               "mhip_filament_contacts_force before mhip_filament_contacts_save_velocity");
  MHIP_REQUIRE(h->list.has_list, MHIP_ERR_RUNTIME, "mhip_filament_contacts_force before mhip_filament_contacts_update");
  if (int e = mhip_filament_contacts_linker_pass(h, dt, stats)) return e;
  return mhip_filament_contacts_reduce(h, external_force);
}

int mhip_filament_contacts_set_history(mhip_filament_contacts_t h, size_t c, const int32_t* pairs,
                                       const double* tang_disp) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  MHIP_REQUIRE(c == 0 || (pairs && tang_disp), MHIP_ERR_INVALID_ARGUMENT, "pairs / tang_disp is null");
  MHIP_REQUIRE(c < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many pairs");
  hipStream_t s = h->stream;
  mhip_stream_t ms = reinterpret_cast<mhip_stream_t>(s);
  const size_t d = sizeof(double);
  int e = MHIP_SUCCESS;
  if (!h->list.has_list) {  // a restart: the first update carries these rows into its list
    if ((e = h->pairs[h->cur].reserve(c * sizeof(int2) + 8)) || (e = h->hist[h->cur].reserve(3 * c * d + 8))) return e;
    if (c > 0) {
      MHIP_HIP(hipMemcpyAsync(h->pairs[h->cur].ptr, pairs, c * sizeof(int2), hipMemcpyDeviceToDevice, s));
      MHIP_HIP(hipMemcpyAsync(h->hist[h->cur].ptr, tang_disp, 3 * c * d, hipMemcpyDeviceToDevice, s));
    }
    h->list.c = c;
    return MHIP_SUCCESS;
  }
  if (h->list.c == 0) return MHIP_SUCCESS;
  HandleBuffer& tmp = h->hist[h->cur ^ 1];
  if ((e = tmp.reserve(3 * h->list.c * d + 8))) return e;
  if ((e = mhip_contact_history_carry(c, pairs, tang_disp, nullptr, h->n, h->list.c, h->pairs[h->cur].as<int32_t>(),
                                      tmp.as<double>(), nullptr, ms)))
    return e;
  MHIP_HIP(hipMemcpyAsync(h->hist[h->cur].ptr, tmp.ptr, 3 * h->list.c * d, hipMemcpyDeviceToDevice, s));
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_get(mhip_filament_contacts_t h, mhip_filament_contact_fields* out) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  MHIP_REQUIRE(out != nullptr, MHIP_ERR_INVALID_ARGUMENT, "fields is null");
  out->num_nodes = h->n;
  out->num_pairs = h->list.has_list ? h->list.c : 0;
  out->pairs = h->list.has_list ? h->pairs[h->cur].as<int32_t>() : nullptr;
  out->sep = h->list.sep.as<double>();
  out->tang_disp = h->list.has_list ? h->hist[h->cur].as<double>() : nullptr;
  out->force = h->list.force.as<double>();
  out->share = h->list.share.as<double>();
  out->node_force = h->node_force.as<double>();
  out->seg = h->list.seg.as<double>();
  out->aabb = h->list.aabb.as<double>();
  out->velocity_prev = h->vel_prev.as<double>();
  return MHIP_SUCCESS;
}

int mhip_filament_contacts_set_law(mhip_filament_contacts_t h, int law) {
  MHIP_REQUIRE(law == MHIP_FILAMENT_CONTACT_FRICTIONAL || law == MHIP_FILAMENT_CONTACT_HERTZ, MHIP_ERR_INVALID_ARGUMENT,
               "unknown filament contact law %d", law);
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filament contacts handle is null");
  h->law = law;
  return MHIP_SUCCESS;
}

}  // extern "C"
