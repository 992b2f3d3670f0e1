// segment_linkers.hpp -- what filament_contact.hip and segment_contact.hip share: the segment row and its box, one
// linker's measurement and result rows, the per-segment sums, the host's linker list.  The invariant that spans a linker
// pass and its reduction stands here once: a linker outside the force branch has +0.0 rows, so the reduction passes it
// over on one flag.  The laws, index bounds, history, branch byte and statistics stay per file.
#pragma once
#include "force_device.hpp"
#include "geom_device.hpp"

#include <cmath>
#include <vector>

namespace mhip {

// ---- device: segment rows ----------------------------------------------------------------------------------------
// seg[i] = (p0, p1, r, 0): one 64-byte line, read as four double2
struct SegmentRow {
  V3 p0, p1;
  double r;
};
__device__ inline SegmentRow load_segment(const double* __restrict__ seg, size_t i) {
  const double2* q = reinterpret_cast<const double2*>(seg + 8 * i);  // a 64-byte line
  const double2 a = q[0], b = q[1], c = q[2], d = q[3];
  return {{a.x, a.y, b.x}, {b.y, c.x, c.y}, d.x};
}
// seg[i] = (x0, x1, r, 0) and the reference's buffered box: min - reach, max + reach, then the skin
// (.../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161)
__device__ inline void store_segment_view(double* __restrict__ seg, double* __restrict__ aabb, size_t i, V3 x0, V3 x1,
                                          double r, double reach, double skin) {
  double2* q = reinterpret_cast<double2*>(seg + 8 * i);
  q[0] = make_double2(x0.x, x0.y);
  q[1] = make_double2(x0.z, x1.x);
  q[2] = make_double2(x1.y, x1.z);
  q[3] = make_double2(r, 0.0);
  const Box b = aabb_segment(x0, x1, reach);
  double* o = aabb + 6 * i;
  o[0] = b.lo.x - skin, o[1] = b.lo.y - skin, o[2] = b.lo.z - skin;
  o[3] = b.hi.x + skin, o[4] = b.hi.y + skin, o[5] = b.hi.z + skin;
}
// what the right end node receives of the linker force Fs acting at cp; the left one receives Fs - this (RED :206-221).
// The `+` inside term2 is the reference's (the velocity map has `-`): DESIGN.md 5k.
__device__ inline V3 segment_share(V3 x0, V3 x1, V3 cp, V3 Fs) {
  const V3 lc = cp - x0, lr = x1 - x0;
  const double iL = 1.0 / norm(lr);
  const V3 t = lr * iL;
  const V3 term1 = (dot(t, Fs) * lc) * iL;
  const V3 term2 = (dot(lc, t) * (Fs + dot(t, Fs) * t)) * iL;
  return term2 - term1;
}

// ---- device: one linker --------------------------------------------------------------------------------------------
// the list is read once per step
__device__ inline int2 load_pair_once(const int* __restrict__ pairs, size_t c) {
  return int2{__builtin_nontemporal_load(pairs + 2 * c), __builtin_nontemporal_load(pairs + 2 * c + 1)};
}
// the two rows, the segment-segment distance (...SpherocylinderSegmentSpherocylinderSegmentLinker.cpp:204-237) and the
// signed separation s = dist - (ra + rb)
struct SegmentLinker {
  SegmentRow a, b;
  SegSeg r;
  double s;
  // left to right (linker kernel :226); dist == 0: NaN rows
  __device__ V3 normal() const { return (r.cp2 - r.cp1) * (1.0 / r.dist); }
};
__device__ inline SegmentLinker measure_linker(const double* __restrict__ seg, int2 p) {
  const SegmentRow a = load_segment(seg, p.x), b = load_segment(seg, p.y);
  const SegSeg r = dist_segment_segment(a.p0, a.p1, b.p0, b.p1);
  return {a, b, r, r.dist - (a.r + b.r)};
}
// F acts on the left segment; the right one receives the negative
__device__ inline void store_linker_force(double* __restrict__ force, double* __restrict__ share, size_t c,
                                          const SegmentLinker& k, V3 F) {
  store3(force, c, F);
  store3(share, 2 * c, segment_share(k.a.p0, k.a.p1, k.r.cp1, F));
  store3(share, 2 * c + 1, segment_share(k.b.p0, k.b.p1, k.r.cp2, V3{-F.x, -F.y, -F.z}));
}
__device__ inline void store_row_nan(double* p, size_t c) {
  const double q = __builtin_nan("");
  store3(p, c, V3{q, q, q});
}
__device__ inline void reset_row(double* p, size_t c) {  // +0.0, written only where it is not +0.0 already
  if (!row_is_pos_zero(p, c)) store3(p, c, V3{0.0, 0.0, 0.0});
}
// outside the force branch: force and both shares are +0.0 (what sum_segment_entries relies on)
__device__ inline void reset_linker(double* __restrict__ force, double* __restrict__ share, size_t c) {
  reset_row(force, c);
  reset_row(share, 2 * c);
  reset_row(share, 2 * c + 1);
}
// a pair outside the caller's index bound: NaN rows, the segments never dereferenced
__device__ inline void refuse_linker(double* __restrict__ sep, double* __restrict__ force, double* __restrict__ share,
                                     size_t c) {
  sep[c] = __builtin_nan("");
  store_row_nan(force, c);
  store_row_nan(share, 2 * c);
  store_row_nan(share, 2 * c + 1);
}
// the frictionless Hertz magnitude at the signed separation s of two segments of radii ri, rj and one material (E, nu)
// (...SpherocylinderSegmentSpherocylinderSegmentHertzianContact.cpp:208-225)
__device__ inline double segment_hertz(double E, double nu, double ri, double rj, double s) {
  const double Rs = (ri * rj) / (ri + rj);
  const double Es = (E * E) / (E - E * nu * nu + E - E * nu * nu);
  return hertz_force_magnitude(Es, Rs, s);
}

// ---- device: the sums of one segment (.../linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221) --
// a0 = +0.0 + sum of (Fs - share), a1 = +0.0 + sum of share over the entries (linker << 1) | side of segment e in
// ascending order.  skip(c): linker c is outside the force branch, as its pass recorded it.  Its rows are +0.0 (the
// linker pass of this step saw to it), and a sum that started from +0.0 is never -0.0: adding them changes no bit, so
// the one word skip reads stands for 48 bytes of rows.
struct SegmentSums {
  V3 a0, a1;
};
template <class SKIP>
__device__ inline SegmentSums sum_segment_entries(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                                  size_t e, const double* __restrict__ force,
                                                  const double* __restrict__ share, SKIP skip) {
  SegmentSums q{{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
  const int32_t lo = ptr[e], hi = ptr[e + 1];
  for (int32_t j = lo; j < hi; ++j) {
    const int32_t en = ent[j];
    const size_t c = static_cast<size_t>(en >> 1);
    if (skip(c)) continue;
    const V3 F = load3(force, c);
    const V3 Fs = (en & 1) ? V3{-F.x, -F.y, -F.z} : F;
    const V3 sm = load3(share, static_cast<size_t>(en));  // row 2 c + side
    q.a0 = q.a0 + (Fs - sm);
    q.a1 = q.a1 + sm;
  }
  return q;
}

// ---- host: the refusals both creates share, at the position each holds them ----------------------------------------
// elastic: the law reads the material (the WCA kind of segment_contact.hip does not)
inline int check_linker_params(double skin, double youngs_modulus, double poisson_ratio, bool elastic) {
  MHIP_REQUIRE(std::isfinite(skin) && skin >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "skin must be finite and >= 0, got %g", skin);
  if (!elastic) return MHIP_SUCCESS;
  MHIP_REQUIRE(std::isfinite(youngs_modulus) && youngs_modulus > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "youngs_modulus must be finite and > 0, got %g", youngs_modulus);
  MHIP_REQUIRE(poisson_ratio > 0.0 && poisson_ratio < 1.0, MHIP_ERR_INVALID_ARGUMENT,
               "poisson_ratio must lie in (0, 1), got %g", poisson_ratio);
  return MHIP_SUCCESS;
}
inline int check_segment_radius(size_t i, double r) {
  MHIP_REQUIRE(std::isfinite(r) && r > 0.0, MHIP_ERR_INVALID_ARGUMENT, "segment %zu: radius must be finite and > 0, got %g",
               i, r);
  return MHIP_SUCCESS;
}

// ---- host: the linker list of `rows` segment rows -----------------------------------------------------------------
// The search with its exclusions, the segment view, the rows of the current list and the segment -> linker incidence.
// The pair buffer is the caller's (the filament handle keeps two, with a history row each).
struct LinkerList {
  mhip_broadphase_t bp = nullptr;
  bool has_list = false;
  size_t c = 0;  // length of the list (filaments, before the first update: the length of a planted list)
  HandleBuffer ex_ptr, ex_idx;
  HandleBuffer seg, aabb, aabb_ref;
  HandleBuffer sep, force, share;
  HandleBuffer inc_ptr, inc_ent;  // segment -> (linker << 1) | side
  HandleBuffer cursor, ws;        // for scan_rows >= rows rows: the caller may build other incidences with them
  ~LinkerList() {
    if (bp) (void)mhip_broadphase_destroy(bp);
  }

  // the buffers whose size the row count fixes, and who may not pair with whom: row i of (ex_ptr [rows + 1], ex_idx)
  // lists, ascending, the rows that never pair with i.  fn: the caller, for a HIP error's text
  int create(const char* fn, size_t rows, size_t scan_rows, const std::vector<int32_t>& ex_ptr_host,
             const std::vector<int32_t>& ex_idx_host, hipStream_t s) {
    if (int e = mhip_broadphase_create(&bp)) return e;
    const size_t d = sizeof(double), w = sizeof(int32_t);
    int e = MHIP_SUCCESS;
    if ((e = ex_ptr.reserve((rows + 1) * w)) || (e = ex_idx.reserve(ex_idx_host.size() * w + 8)) ||
        (e = seg.reserve(8 * rows * d + 8)) || (e = aabb.reserve(6 * rows * d + 8)) ||
        (e = aabb_ref.reserve(6 * rows * d + 8)) || (e = inc_ptr.reserve((rows + 1) * w)) ||
        (e = cursor.reserve((scan_rows + 1) * w)) || (e = ws.reserve(scan_workspace_bytes(scan_rows) + 8)))
      return e;
    if ((e = upload(fn, ex_ptr, ex_ptr_host.data(), (rows + 1) * w, s))) return e;
    if (!ex_idx_host.empty() && (e = upload(fn, ex_idx, ex_idx_host.data(), ex_idx_host.size() * w, s))) return e;
    return mhip_broadphase_set_exclusions(bp, rows, ex_ptr.as<int32_t>(), ex_idx.as<int32_t>(), ex_idx_host.size(),
                                          reinterpret_cast<mhip_stream_t>(s));
  }

  // has a corner of a box moved by skin / 2 since the list was built?  (synchronises)
  int moved(size_t rows, double skin, int* flag, hipStream_t s) {
    return mhip_aabb_moved(rows, aabb.as<double>(), aabb_ref.as<double>(), 0.5 * skin, flag,
                           reinterpret_cast<mhip_stream_t>(s));
  }

  // Every pair of box-overlapping rows that the exclusions allow, into `pairs`; the linker rows cleared; the incidence;
  // the boxes remembered for moved().  center: what the search snapshots.  hook(c_new) runs once the new pairs stand,
  // while `c` and the rows of the old list still do: there a caller carries what it keeps per linker across.
  template <class HOOK>
  int rebuild(size_t rows, const double* center, HandleBuffer& pairs, hipStream_t s, HOOK&& hook) {
    mhip_stream_t ms = reinterpret_cast<mhip_stream_t>(s);
    const size_t d = sizeof(double);
    mhip_broadphase_config cfg{};
    cfg.search_kind = MHIP_SEARCH_AABB;
    cfg.symmetric = 0;
    cfg.buffer = 0.0;  // the boxes carry the skin
    size_t c_new = 0;
    if (int e = mhip_broadphase_build(bp, &cfg, rows, aabb.as<double>(), center, nullptr, &c_new, ms)) return e;
    MHIP_REQUIRE(c_new < (1ull << 30), MHIP_ERR_RUNTIME, "too many linkers for 32-bit incidence entries");
    int e = MHIP_SUCCESS;
    if ((e = pairs.reserve(c_new * sizeof(int2) + 8)) || (e = inc_ent.reserve(2 * c_new * sizeof(int32_t) + 8))) return e;
    if ((e = mhip_broadphase_get_pairs(bp, pairs.as<int32_t>(), nullptr, nullptr, ms))) return e;
    if ((e = hook(c_new))) return e;
    // (after the hook: sep, force and share of the old list are dead, and reserve may move the buffers)
    if ((e = sep.reserve(c_new * d + 8)) || (e = force.reserve(3 * c_new * d + 8)) ||
        (e = share.reserve(6 * c_new * d + 8)))
      return e;
    if (c_new > 0) {
      MHIP_HIP(hipMemsetAsync(sep.ptr, 0, c_new * d, s));
      MHIP_HIP(hipMemsetAsync(force.ptr, 0, 3 * c_new * d, s));
      MHIP_HIP(hipMemsetAsync(share.ptr, 0, 6 * c_new * d, s));
    }
    if ((e = build_incidence(rows, c_new, PairEnds{pairs.as<int2>()}, cursor.as<int32_t>(), inc_ptr.as<int32_t>(),
                             inc_ent.as<int32_t>(), ws.ptr, s)))
      return e;
    if (rows > 0) MHIP_HIP(hipMemcpyAsync(aabb_ref.ptr, aabb.ptr, 6 * rows * d, hipMemcpyDeviceToDevice, s));
    c = c_new;
    has_list = true;
    return MHIP_SUCCESS;
  }
};

}  // namespace mhip
