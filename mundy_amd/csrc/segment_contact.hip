// segment_contact.hip -- frictionless contacts between backbone segments: the excluded volume of the reference's HP1 app
// (compute_hertzian_contact_forces, scrap/parameter_interface/alens/tests/performance_tests/HP1.cpp:4356-4496, the first
// term of its force field, :4737).  A segment joins two bodies given by an end-index list; connectivity is general.
//   segment view   .../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161                        one segment per lane
//   linker pass    ...SpherocylinderSegmentSpherocylinderSegmentLinker.cpp:204-237 (distance) and
//                  ...SegmentHertzianContact.cpp:192-225 or ...SegmentWCA.cpp:187-210 in ONE pass     one linker per lane
//   segment sums   .../linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221 as a gather, then the
//                  end-segment correction (HP1.cpp:4395-4434, :4451-4490)                            one segment per lane
//   node gather    each body adds the sums of its (segment, side) entries: no atomic on a force       one body per lane
// Orders, byte counts and the wider WCA box: include/mundy_hip_segment_contact.h, DESIGN.md 5s.
#include "segment_linkers.hpp"
#include "../../include/mundy_hip_segment_contact.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace mhip {

// seg[e] = (x_a, x_b, r_e, 0) and the box of (x_a, x_b, max(r_e, min_reach)) grown by the skin; min_reach: cutoff / 2
// for WCA, 0 for Hertz (r_e > 0)
__global__ void __launch_bounds__(kBlock)
    k_segment_view_ends(size_t m, const int2* __restrict__ ends, const double* __restrict__ x,
                        const double* __restrict__ radius, double min_reach, double skin, double* __restrict__ seg,
                        double* __restrict__ aabb) {
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < m; e += (size_t)gridDim.x * blockDim.x) {
    const int2 ab = ends[e];  // checked against [0, n) at creation
    const V3 x0 = load3(x, ab.x), x1 = load3(x, ab.y);
    const double r = radius[e];
    store_segment_view(seg, aabb, e, x0, x1, r, dmax(r, min_reach), skin);
  }
}

// the two laws: Hertz (segment_hertz, segment_linkers.hpp) at the signed separation, WCA at the centreline distance
struct SegmentLaw {
  double E, nu, epsilon, sigma, cutoff;
};
// the end-segment correction's Hertz magnitude: segment_hertz's expression at sep = L - 2 r, Rs = r r / (r + r), with
// x^(3/2) rounded once (force_device.hpp), so that it is the host's value in bits
__device__ inline double segment_hertz_end(const SegmentLaw& w, double r, double s) {
  const double Rs = (r * r) / (r + r);
  const double Es = (w.E * w.E) / (w.E - w.E * w.nu * w.nu + w.E - w.E * w.nu * w.nu);
  return (4.0 / 3.0) * Es * sqrt(Rs) * pow_three_halves(-s);
}
__device__ inline double segment_wca(const SegmentLaw& w, double d) {  // d: the centreline distance
  const double rho2 = w.sigma * w.sigma / (d * d);
  const double rho6 = rho2 * rho2 * rho2;
  const double rho12 = rho6 * rho6;
  return 24.0 * w.epsilon * (2.0 * rho12 - rho6) / d;
}

// One linker per lane and pass, grid-stride.  in_branch[c]: the linker takes part in the sums (its rows are not +0.0 by
// construction).  stats[0]: bits of max(0, -sep) over the force branch; stats[1]: linkers in it.
template <int KIND>
__global__ void __launch_bounds__(kBlock)
    k_segment_linkers(size_t C, size_t M, const int* __restrict__ pairs, const double* __restrict__ seg, SegmentLaw law,
                      double* __restrict__ sep, double* __restrict__ force, double* __restrict__ share,
                      uint8_t* __restrict__ in_branch, unsigned long long* __restrict__ stats) {
  double dmax_ = 0.0;
  unsigned count = 0;
  for (size_t c = blockIdx.x * (size_t)blockDim.x + threadIdx.x; c < C; c += (size_t)gridDim.x * blockDim.x) {
    const int2 p = load_pair_once(pairs, c);
    if (static_cast<unsigned>(p.x) >= M || static_cast<unsigned>(p.y) >= M) {
      refuse_linker(sep, force, share, c);
      in_branch[c] = 1;
      continue;
    }
    const SegmentLinker k = measure_linker(seg, p);
    const double s = k.s;
    sep[c] = s;
    const bool in = KIND == MHIP_SEGMENT_CONTACT_HERTZ ? s < 0.0 : k.r.dist < law.cutoff;
    in_branch[c] = in ? 1 : 0;
    if (!in) {
      reset_linker(force, share, c);
      continue;
    }
    // WCA: the distance as the reference recomputes it from the stored separation (...SegmentWCA.cpp:195-196)
    const double fm = KIND == MHIP_SEGMENT_CONTACT_HERTZ ? segment_hertz(law.E, law.nu, k.a.r, k.b.r, s)
                                                         : segment_wca(law, s + (k.a.r + k.b.r));
    store_linker_force(force, share, c, k, (-fm) * k.normal());
    dmax_ = -s > dmax_ ? -s : dmax_;
    ++count;
  }
  block_stat_max(dmax_, stats);
  block_stat_add(count, stats + 1);
}

// One segment per lane: sum_segment_entries (a linker outside the force branch is passed over on its byte of in_branch),
// then the end correction.  sums[e] = (a0, a1): 48 bytes.
template <int KIND>
__global__ void __launch_bounds__(kBlock)
    k_segment_sums(size_t M, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                   const uint8_t* __restrict__ in_branch, const double* __restrict__ force,
                   const double* __restrict__ share, const double* __restrict__ seg,
                   const uint8_t* __restrict__ end_correction, SegmentLaw law, double* __restrict__ sums,
                   unsigned long long* __restrict__ stats) {
  double dmax_ = 0.0;
  for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < M; e += (size_t)gridDim.x * blockDim.x) {
    const SegmentSums q = sum_segment_entries(ptr, ent, e, force, share, [&](size_t c) { return !in_branch[c]; });
    V3 a0 = q.a0, a1 = q.a1;
    if (end_correction[e]) {  // the missing neighbour of a chain's first or last segment (HP1.cpp:4367-4372)
      const SegmentRow s = load_segment(seg, e);
      const V3 d = s.p1 - s.p0;
      const double L = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
      const V3 t{d.x / L, d.y / L, d.z / L};
      const double gap = L - 2.0 * s.r;
      const bool in = KIND == MHIP_SEGMENT_CONTACT_HERTZ ? gap < 0.0 : L < law.cutoff;
      if (in) {
        const double fm = KIND == MHIP_SEGMENT_CONTACT_HERTZ ? segment_hertz_end(law, s.r, gap) : segment_wca(law, L);
        const V3 ft = fm * t;
        a0 = a0 - ft;
        a1 = a1 + ft;
        dmax_ = -gap > dmax_ ? -gap : dmax_;
      }
    }
    double* o = sums + 6 * e;
    o[0] = a0.x, o[1] = a0.y, o[2] = a0.z;
    o[3] = a1.x, o[4] = a1.y, o[5] = a1.z;
  }
  block_stat_max(dmax_, stats);
}

// One body per lane: +0.0 + the sums of its (segment, side) entries in ascending segment index.  A body on no segment
// gets +0.0, or is left alone when accumulating.
template <bool ACCUMULATE>
__global__ void __launch_bounds__(kBlock)
    k_segment_node_gather(size_t n, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                          const double* __restrict__ sums, double* __restrict__ force) {
  for (size_t b = blockIdx.x * (size_t)blockDim.x + threadIdx.x; b < n; b += (size_t)gridDim.x * blockDim.x) {
    const int32_t lo = ptr[b], hi = ptr[b + 1];
    if (ACCUMULATE && lo == hi) continue;
    V3 f{0.0, 0.0, 0.0};
    for (int32_t j = lo; j < hi; ++j) f = f + load3(sums, static_cast<size_t>(ent[j]));  // row 2 e + side
    write_force<ACCUMULATE>(force, b, f);
  }
}

}  // namespace mhip

using namespace mhip;

struct mhip_segment_contacts {
  size_t n = 0, m = 0;
  mhip_segment_contact_params prm{};
  LinkerList list;
  HandleBuffer ends, radius, end_correction, sums;
  HandleBuffer pairs, in_branch;
  HandleBuffer body_ptr, body_ent;  // body -> (segment << 1) | side
  SegmentLaw law() const { return {prm.youngs_modulus, prm.poisson_ratio, prm.epsilon, prm.sigma, prm.cutoff}; }
  bool wca() const { return prm.kind == MHIP_SEGMENT_CONTACT_WCA; }
};

namespace {

int segment_view(mhip_segment_contacts_t h, const double* center, hipStream_t s) {
  if (h->m == 0) return MHIP_SUCCESS;
  k_segment_view_ends<<<grid_for(h->m), kBlock, 0, s>>>(h->m, h->ends.as<int2>(), center, h->radius.as<double>(),
                                                        h->wca() ? 0.5 * h->prm.cutoff : 0.0, h->prm.skin,
                                                        h->list.seg.as<double>(), h->list.aabb.as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

}  // namespace

extern "C" {

int mhip_segment_contacts_create(mhip_segment_contacts_t* handle, size_t n, size_t m, const int32_t* ends,
                                 const double* radius, double radius_scalar, const unsigned char* end_correction,
                                 const mhip_segment_contact_params* params, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(params != nullptr, MHIP_ERR_INVALID_ARGUMENT, "params is null");
  const mhip_segment_contact_params& p = *params;
  MHIP_REQUIRE(p.kind == MHIP_SEGMENT_CONTACT_HERTZ || p.kind == MHIP_SEGMENT_CONTACT_WCA, MHIP_ERR_INVALID_ARGUMENT,
               "unknown segment contact kind %d", p.kind);
  const bool hertz = p.kind == MHIP_SEGMENT_CONTACT_HERTZ;
  if (int e = check_linker_params(p.skin, p.youngs_modulus, p.poisson_ratio, hertz)) return e;
  if (!hertz) {
    MHIP_REQUIRE(std::isfinite(p.epsilon) && p.epsilon >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
                 "epsilon must be finite and >= 0, got %g", p.epsilon);
    MHIP_REQUIRE(std::isfinite(p.sigma) && p.sigma > 0.0, MHIP_ERR_INVALID_ARGUMENT, "sigma must be finite and > 0, got %g",
                 p.sigma);
    MHIP_REQUIRE(std::isfinite(p.cutoff) && p.cutoff > 0.0, MHIP_ERR_INVALID_ARGUMENT,
                 "cutoff must be finite and > 0, got %g", p.cutoff);
  }
  MHIP_REQUIRE(m == 0 || ends, MHIP_ERR_INVALID_ARGUMENT, "ends is null");
  MHIP_REQUIRE(n < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many bodies for 32-bit segment ends");
  MHIP_REQUIRE(m < (1ull << 30), MHIP_ERR_INVALID_ARGUMENT, "too many segments for 31-bit incidence entries");
  MHIP_REQUIRE(radius || (std::isfinite(radius_scalar) && radius_scalar > 0.0), MHIP_ERR_INVALID_ARGUMENT,
               "radius must be finite and > 0, got %g", radius_scalar);
  for (size_t e = 0; e < m; ++e) {
    const int32_t a = ends[2 * e], b = ends[2 * e + 1];
    MHIP_REQUIRE(a >= 0 && b >= 0 && static_cast<size_t>(a) < n && static_cast<size_t>(b) < n, MHIP_ERR_INVALID_ARGUMENT,
                 "segment %zu joins (%d, %d): an index outside [0, %zu)", e, a, b, n);
    MHIP_REQUIRE(a != b, MHIP_ERR_INVALID_ARGUMENT, "segment %zu joins body %d to itself", e, a);
    if (radius)
      if (int err = check_segment_radius(e, radius[e])) return err;
  }
  // who may not pair with whom: for segment e every other segment incident to either of its end nodes
  // (DestroyBoundNeighbors.cpp:150-170), ascending, once each
  std::vector<int32_t> node_ptr(n + 1, 0), node_seg(2 * m);
  for (size_t k = 0; k < 2 * m; ++k) ++node_ptr[ends[k] + 1];
  for (size_t b = 0; b < n; ++b) node_ptr[b + 1] += node_ptr[b];
  {
    std::vector<int32_t> fill(node_ptr.begin(), node_ptr.end() - 1);
    for (size_t k = 0; k < 2 * m; ++k) node_seg[fill[ends[k]]++] = static_cast<int32_t>(k >> 1);
  }
  std::vector<int32_t> ex_ptr(m + 1, 0), ex_idx, row;
  for (size_t e = 0; e < m; ++e) {
    row.clear();
    for (int side = 0; side < 2; ++side) {
      const int32_t b = ends[2 * e + side];
      for (int32_t k = node_ptr[b]; k < node_ptr[b + 1]; ++k)
        if (static_cast<size_t>(node_seg[k]) != e) row.push_back(node_seg[k]);
    }
    std::sort(row.begin(), row.end());
    row.erase(std::unique(row.begin(), row.end()), row.end());
    ex_idx.insert(ex_idx.end(), row.begin(), row.end());
    MHIP_REQUIRE(ex_idx.size() < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many shared-node exclusions");
    ex_ptr[e + 1] = static_cast<int32_t>(ex_idx.size());
  }
  std::vector<double> rad(m, radius_scalar);
  if (radius) std::copy(radius, radius + m, rad.begin());
  std::vector<uint8_t> corr(m, 0);
  if (end_correction)
    for (size_t e = 0; e < m; ++e) corr[e] = end_correction[e] ? 1 : 0;

  auto h = std::make_unique<mhip_segment_contacts>();
  h->n = n;
  h->m = m;
  h->prm = p;
  hipStream_t s = as_stream(stream);
  const size_t d = sizeof(double);
  int e = MHIP_SUCCESS;
  // (cursor and ws serve the body incidence below as well: the larger of the two row counts)
  if ((e = h->list.create(__func__, m, std::max(n, m), ex_ptr, ex_idx, s))) return e;
  if ((e = h->ends.reserve(m * sizeof(int2) + 8)) || (e = h->radius.reserve(m * d + 8)) ||
      (e = h->end_correction.reserve(m + 8)) || (e = h->sums.reserve(6 * m * d + 8)) ||
      (e = h->body_ptr.reserve((n + 1) * sizeof(int32_t))) || (e = h->body_ent.reserve(2 * m * sizeof(int32_t) + 8)))
    return e;
  if (m > 0) {
    if ((e = upload(__func__, h->ends, ends, m * sizeof(int2), s))) return e;
    if ((e = upload(__func__, h->radius, rad.data(), m * d, s))) return e;
    if ((e = upload(__func__, h->end_correction, corr.data(), m, s))) return e;
  }
  if ((e = build_incidence(n, m, PairEnds{h->ends.as<int2>()}, h->list.cursor.as<int32_t>(), h->body_ptr.as<int32_t>(),
                           h->body_ent.as<int32_t>(), h->list.ws.ptr, s)))
    return e;
  // the host arrays built here may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_segment_contacts_destroy(mhip_segment_contacts_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_segment_contacts_update(mhip_segment_contacts_t h, const double* center, int force_rebuild, int* rebuilt,
                                 mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "segment contacts handle is null");
  MHIP_REQUIRE(rebuilt != nullptr, MHIP_ERR_INVALID_ARGUMENT, "rebuilt is null");
  MHIP_REQUIRE(center != nullptr || h->m == 0, MHIP_ERR_INVALID_ARGUMENT, "center is null");
  *rebuilt = 0;
  hipStream_t s = as_stream(stream);
  if (int e = segment_view(h, center, s)) return e;
  LinkerList& l = h->list;
  int moved = 1;  // the first call builds
  if (l.has_list && !force_rebuild)
    if (int e = l.moved(h->m, h->prm.skin, &moved, s)) return e;
  if (!moved) return MHIP_SUCCESS;
  // rebuild (HP1.cpp:3053-3175): every pair of box-overlapping segments that share no node
  // (the search snapshots its `center` argument for mhip_broadphase_needs_rebuild, which this handle never asks: the
  //  boxes stand in for it, 6 m doubles where 3 m are read)
  if (int e = l.rebuild(h->m, l.aabb.as<double>(), h->pairs, s, [&](size_t c_new) {
        if (int e = h->in_branch.reserve(c_new + 8)) return e;
        return c_new > 0 ? hip_status(__func__, hipMemsetAsync(h->in_branch.ptr, 0, c_new, s)) : MHIP_SUCCESS;
      }))
    return e;
  *rebuilt = 1;
  return MHIP_SUCCESS;
}

int mhip_segment_contacts_linker_pass(mhip_segment_contacts_t h, void* stats, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "segment contacts handle is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(h->list.has_list, MHIP_ERR_RUNTIME, "mhip_segment_contacts_linker_pass before mhip_segment_contacts_update");
  hipStream_t s = as_stream(stream);
  MHIP_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(unsigned long long), s));
  const LinkerList& l = h->list;
  const size_t c = l.c;
  if (h->m == 0 || c == 0) return MHIP_SUCCESS;
  dispatch<MHIP_SEGMENT_CONTACT_WCA, MHIP_SEGMENT_CONTACT_HERTZ>(h->prm.kind, [&](auto kind) {
    k_segment_linkers<decltype(kind)::value><<<grid_for(c), kBlock, 0, s>>>(
        c, h->m, h->pairs.as<int>(), l.seg.as<double>(), h->law(), l.sep.as<double>(), l.force.as<double>(),
        l.share.as<double>(), h->in_branch.as<uint8_t>(), static_cast<unsigned long long*>(stats));
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_segment_contacts_reduce(mhip_segment_contacts_t h, double* force, int accumulate, void* stats,
                                 mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "segment contacts handle is null");
  MHIP_REQUIRE(force != nullptr || h->n == 0, MHIP_ERR_INVALID_ARGUMENT, "force is null");
  MHIP_REQUIRE(h->list.has_list, MHIP_ERR_RUNTIME, "mhip_segment_contacts_reduce before mhip_segment_contacts_update");
  hipStream_t s = as_stream(stream);
  const size_t n = h->n, m = h->m;
  const LinkerList& l = h->list;
  if (n == 0) return MHIP_SUCCESS;
  if (m > 0) {
    dispatch<MHIP_SEGMENT_CONTACT_WCA, MHIP_SEGMENT_CONTACT_HERTZ>(h->prm.kind, [&](auto kind) {
      k_segment_sums<decltype(kind)::value><<<grid_for(m), kBlock, 0, s>>>(
          m, l.inc_ptr.as<int32_t>(), l.inc_ent.as<int32_t>(), h->in_branch.as<uint8_t>(), l.force.as<double>(),
          l.share.as<double>(), l.seg.as<double>(), h->end_correction.as<uint8_t>(), h->law(), h->sums.as<double>(),
          static_cast<unsigned long long*>(stats));
    });
    MHIP_LAUNCH_CHECK();
  }
  // (m == 0: every row of body_ptr is empty, and the gather writes +0.0 or leaves the rows alone)
  dispatch<true, false>(accumulate != 0, [&](auto acc) {
    k_segment_node_gather<decltype(acc)::value><<<grid_for(n), kBlock, 0, s>>>(
        n, h->body_ptr.as<int32_t>(), h->body_ent.as<int32_t>(), h->sums.as<double>(), force);
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_segment_contacts_force(mhip_segment_contacts_t h, const double* center, double* force, int accumulate,
                                void* stats, mhip_stream_t stream) {
  // every refusal comes before the first launch
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "segment contacts handle is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(center != nullptr || h->m == 0, MHIP_ERR_INVALID_ARGUMENT, "center is null");
  MHIP_REQUIRE(force != nullptr || h->n == 0, MHIP_ERR_INVALID_ARGUMENT, "force is null");
  MHIP_REQUIRE(h->list.has_list, MHIP_ERR_RUNTIME, "mhip_segment_contacts_force before mhip_segment_contacts_update");
  if (int e = segment_view(h, center, as_stream(stream))) return e;
  if (int e = mhip_segment_contacts_linker_pass(h, stats, stream)) return e;
  return mhip_segment_contacts_reduce(h, force, accumulate, stats, stream);
}

int mhip_segment_contacts_get(mhip_segment_contacts_t h, mhip_segment_contact_fields* out) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "segment contacts handle is null");
  MHIP_REQUIRE(out != nullptr, MHIP_ERR_INVALID_ARGUMENT, "fields is null");
  out->num_bodies = h->n;
  out->num_segments = h->m;
  out->num_pairs = h->list.has_list ? h->list.c : 0;
  out->pairs = h->list.has_list ? h->pairs.as<int32_t>() : nullptr;
  out->sep = h->list.sep.as<double>();
  out->force = h->list.force.as<double>();
  out->share = h->list.share.as<double>();
  out->seg = h->list.seg.as<double>();
  out->aabb = h->list.aabb.as<double>();
  return MHIP_SUCCESS;
}

}  // extern "C"
