// stepper.hpp -- the per-timestep contact hot path for spherocylinders as a C++ host loop over the C ABI: what a
// MundyMech-style timestep loop would hold (the reference's only such loops are its scrap apps,
// scrap/lcp_spheres/NgpLcp.cpp:835-920; scrap/.../Bacteria.cpp:1013-1110).  Host code only sequences kernels:
//   [Z-order reorder] -> compute_aabb -> GenNeighborLinks::generate -> segment records -> contact_spherocylinders
//   -> ContactOperator (rod-compressed) -> solve_lcp (fused BBPGD) -> body velocities -> Euler + quaternion update
// Opt-in soft contact (SpherocylinderStepper::set_hertz_contact): the solve is replaced by the Hertz force per linker
// and the operator's body sweep on it, U = M D f (Bacteria.cpp:755-848).
// Opt-in friction on top of it (SpherocylinderStepper::set_hertz_friction): the reference's frictional Hertzian rod
// contact with a tangential history per pair (...FrictionalHertzianContact.cpp:384-518), a force vector per linker and
// the operator's vector body sweep; the history follows the pairs through list rebuilds and reorder_bodies.
// Opt-in growth (SpherocylinderStepper::set_growth): the colony step of the same app (Bacteria.cpp:1033-1080) in front
// of compute_aabb -- divide_bacteria (:926-966) -> grow_bacteria (:905-920) -- on a body population that lives in
// grow-only device storage, with the rebuild rule of growing bodies (check_update_neighbor_list, :685-748).
// All arrays stay on the device; the only host reads are the pair count and the solver's convergence polls (Hertz
// mode: the largest overlap; growth mode: the birth count and the corner-test flag).
// FilamentStepper is the elastic half of the sperm apps' step (CollidingOverdampedFrictionalSperm.cpp:1999-2027):
//   advance -> edge pass + node pass (centerline-twist forces and twist torques at x(t + dt)) -> node drag
// SphereChainStepper is the bead-spring chain step of the chromatin apps (NgpHP1.cpp:3802-3990) on spheres, in four
// stages a host program puts its own force and velocity terms between:
//   neighbour list -> spring forces -> U_ext = M F + U_brown -> contacts, LCP on sep + dt D^T U_ext, U_ext + M D lambda
// Its opt-in stages are the rest of the HP1 step (HP1.cpp:4728-4803): crosslinker KMC and springs, periphery bind sites,
// the nuclear wall and active dipoles in the force stage, n-body hydrodynamics with the periphery's no-slip correction
// in the velocity stage; set_backbone_collision adds that app's excluded volume, frictionless contacts between the
// backbone segments (HP1.cpp:4356-4496), as the term at the head of the force stage, and set_sphere_contacts(false)
// then leaves the sphere contact out, the reference's own configuration.
#pragma once
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "mundy_hip/adapter.hpp"

#include "../mundy_hip_segment_contact.h"
#include "../mundy_hip_filament_inertial.h"

namespace mundy_hip {
namespace mech {

/// grow-only workspace: reallocates only when the buffer is too small, so a time loop stops allocating after its
/// first steps (hipMalloc / hipFree cost more than most kernels of a step)
template <class T>
inline T* workspace(DeviceArray<T>& a, size_t n) {
  if (a.size() < n) a = DeviceArray<T>(n + n / 8 + 16);
  return a.data();
}

struct StepStats {
  size_t num_contacts = 0;
  unsigned num_iters = 0;
  double residual = 0.0;
  bool converged = false, rebuilt = false;
  double max_overlap = 0.0;  // Hertz mode: max(0, -sep) over the step's contacts (what dt is chosen from)
  size_t num_born = 0;       // growth mode: bodies that divided this step (children are rows n_before + k)
  size_t num_sliding = 0;    // frictional Hertz mode: contacts whose tangential force was capped at mu |F_n|
  size_t num_carried = 0;    // frictional Hertz mode: history rows carried to a rebuilt list this step
  double max_stretch = 0.0;              // FilamentStepper: the largest |l - l0| / l0 over the edges
  double max_curvature_deviation = 0.0;  // FilamentStepper: the largest component of |kappa - kappa_rest|
  double kinetic_energy = 0.0;           // FilamentStepper::set_inertial: of the velocities the corrector wrote
  double max_spring_length = 0.0;        // SphereChainStepper: the longest spring at the start of the step
  int springs_overstretched = 0;         // SphereChainStepper: springs past their limit (FENE: L >= r_max)
  int angular_degenerate = 0;            // ... set_angular_springs: triplets with an arm of zero length (no force)
  double max_angle_deviation = 0.0;      // ... the largest |cos(theta) - cos(rest_angle)| at the force evaluation
  // SphereChainStepper with crosslinkers, a periphery or active springs: the step's statistics array
  int crosslinker_binds = 0, crosslinker_unbinds = 0;  // this step's KMC events
  int crosslinker_periphery_bound = 0;                 // crosslinkers bound to a periphery site after the KMC step
  int crosslinkers_overstretched = 0;
  double max_crosslinker_length = 0.0;
  int periphery_colliding = 0;  // beads that touch the wall
  double max_periphery_overlap = 0.0;
  int active_springs = 0, active_switches_on = 0, active_switches_off = 0;
  // SphereChainStepper with set_backbone_collision: the segment contacts' own statistics
  double max_segment_overlap = 0.0;    // max(0, -sep) over the force branch, corrected end segments included
  size_t segment_contacts = 0;         // segment pairs in the force branch
  size_t num_segment_pairs = 0;        // segment pairs in the neighbour list
  bool segment_list_rebuilt = false;   // whether this step rebuilt that list
};

/// Frictionless Hertzian or WCA contacts between segments given by an end-index list over n bodies
/// (mhip_segment_contacts_*, include/mundy_hip_segment_contact.h): RAII over the handle.  Host arrays ends [m][2],
/// radius [m] or empty (then radius_scalar), end_correction [m] bytes or empty (none corrected).
class SegmentContacts {
 public:
  SegmentContacts(size_t num_bodies, const std::vector<int32_t>& ends, const std::vector<double>& radius,
                  double radius_scalar, const std::vector<unsigned char>& end_correction,
                  const mhip_segment_contact_params& params, mhip_stream_t stream = nullptr)
      : m_(ends.size() / 2) {
    if (!radius.empty() && radius.size() != m_) throw std::invalid_argument("SegmentContacts: one radius per segment");
    if (!end_correction.empty() && end_correction.size() != m_)
      throw std::invalid_argument("SegmentContacts: one end_correction byte per segment");
    check(mhip_segment_contacts_create(&h_, num_bodies, m_, ends.data(), radius.empty() ? nullptr : radius.data(),
                                       radius_scalar, end_correction.empty() ? nullptr : end_correction.data(), &params,
                                       stream));
  }
  ~SegmentContacts() { mhip_segment_contacts_destroy(h_); }
  SegmentContacts(const SegmentContacts&) = delete;
  SegmentContacts& operator=(const SegmentContacts&) = delete;
  /// the segment view at center [n][3] and, when due, the list; returns whether it was rebuilt
  bool update(const double* center, bool force_rebuild = false, mhip_stream_t stream = nullptr) {
    int rebuilt = 0;
    check(mhip_segment_contacts_update(h_, center, force_rebuild ? 1 : 0, &rebuilt, stream));
    return rebuilt != 0;
  }
  /// force [n][3] written or added to; stats [device, 16 bytes] = (bits of the max overlap, linkers in the force branch)
  void force(const double* center, double* force, bool accumulate, void* stats, mhip_stream_t stream = nullptr) {
    check(mhip_segment_contacts_force(h_, center, force, accumulate ? 1 : 0, stats, stream));
  }
  mhip_segment_contact_fields fields() const {
    mhip_segment_contact_fields f{};
    check(mhip_segment_contacts_get(h_, &f));
    return f;
  }
  size_t size() const { return m_; }
  mhip_segment_contacts_t handle() const { return h_; }

 private:
  mhip_segment_contacts_t h_ = nullptr;
  size_t m_;
};

/// the LCP of a contact operator with right-hand side q: fused BBPGD from lambda = 0 (NgpLcp.cpp:890-891); x receives
/// the multipliers, g, x_tmp and g_tmp [C] are work vectors.  mobility: the LCP against the hydrodynamic mobility
/// (mhip_bbpgd_solve_contact_hydro); null: the operator's dry one
inline mhip_solve_result solve_lcp_from_zero(ContactOperator& op, size_t C, const double* q,
                                             const convex::PGDConfig<double>& cfg, double* x, double* g, double* x_tmp,
                                             double* g_tmp, const HydroMobility* mobility = nullptr) {
  check(mhip_fill(C, x, 0.0, nullptr));
  const mhip_space lcp{MHIP_SPACE_LOWER_BOUND, 0.0, 0.0};
  const mhip_pgd_config pc{cfg.max_iters, cfg.tol, MHIP_RESIDUAL_PROJECTED_DIFF};
  mhip_solve_result res{};
  if (mobility)
    check(mhip_bbpgd_solve_contact_hydro(op.handle(), mobility->c_mobility(), q, &lcp, &pc, x, g, x_tmp, g_tmp, &res,
                                         nullptr));
  else
    check(mhip_bbpgd_solve_contact(op.handle(), q, &lcp, &pc, x, g, x_tmp, g_tmp, &res, nullptr));
  return res;
}

/// grow-only storage that keeps its first `live` doubles: reallocates with headroom only when `need` does not fit
inline void grow_keep(DeviceVector& a, size_t need, size_t live) {
  if (a.size() >= need) return;
  DeviceVector b(need + need / 8 + 16);
  if (live) check(mhip_deep_copy(live, b.data(), a.data(), nullptr));
  a = std::move(b);
}

class SpherocylinderStepper {
 public:
  /// host arrays: center [n][3], quat [n][4] (w, x, y, z), radius [n], length [n], mob_trans [n], mob_rot [n]
  SpherocylinderStepper(const std::vector<double>& center, const std::vector<double>& quat,
                        const std::vector<double>& radius, const std::vector<double>& length,
                        const std::vector<double>& mob_trans, const std::vector<double>& mob_rot, double dt,
                        double search_buffer, convex::PGDConfig<double> cfg, const double* periodic_box = nullptr)
      : n_(radius.size()), dt_(dt), cfg_(cfg), center_(center), quat_(quat), radius_(radius), length_(length),
        mob_t_(mob_trans), mob_r_(mob_rot), brad_(n_), aabb_(6 * n_), seg_(8 * n_), tmp_(4 * n_),
        buffer_(search_buffer), perm_(n_) {
    check(mhip_bounding_radius_spherocylinders(n_, radius_.data(), length_.data(), brad_.data(), nullptr));
    links_.set_search_buffer(search_buffer).set_search_kind(MHIP_SEARCH_AABB);
    if (periodic_box) {  // orthorhombic periodic box [0, L): periodic search, nearest-image contacts, wrap_rigid
      periodic_ = true;
      for (int k = 0; k < 3; ++k) box_[k] = periodic_box[k];
      links_.set_periodic_box(box_[0], box_[1], box_[2]);
    }
    links_.concretize();
  }

  /// Z-order permutation of every per-body array by centre
  void reorder_bodies(double cell_size, const double lo[3]) {
    check(mhip_morton_order(n_, center_.data(), lo, cell_size, perm_.data(), nullptr));
    gather(center_, 3);
    gather(quat_, 4);
    gather(radius_, 1);
    gather(length_, 1);
    gather(brad_, 1);
    gather(mob_t_, 1);
    gather(mob_r_, 1);
    if (friction_) renumber_history();
    // the neighbour list and the operator's incidence index are in the old numbering
    links_.invalidate();
    op_.reset();
    have_ref_ = false;
  }

  /// Hertzian soft contact instead of the LCP (opt-in; the LCP is the default): each step evaluates the Hertz force
  /// per linker (rod radius, E > 0, 0 < nu < 1 for every body) and sums it per body through the operator's body sweep
  /// -- no solve (num_iters = 0, converged).  The reference's production loop: Bacteria.cpp:755-848, :1033-1080.
  void set_hertz_contact(double youngs_modulus = 1000.0, double poisson_ratio = 0.3) {
    if (!(youngs_modulus > 0.0 && youngs_modulus < HUGE_VAL) || !(poisson_ratio > 0.0 && poisson_ratio < 1.0))
      throw std::invalid_argument("set_hertz_contact: E must be finite and > 0, 0 < nu < 1");
    hertz_ = true;
    material_.youngs_modulus = youngs_modulus;
    material_.poisson_ratio = poisson_ratio;
  }

  /// Friction on top of the Hertz contact (opt-in, after set_hertz_contact): the reference's frictional Hertzian rod
  /// contact, mu >= 0, damping coefficients and density >= 0 (defaults: the reference's).  The stepper then owns the
  /// previous step's body velocities (zero before the first step) and the tangential displacement of every listed
  /// pair, carried through list rebuilds and reorder_bodies.  Not combined with growth.
  void set_hertz_friction(double mu, double gamma_n = 0.0, double gamma_t = 0.0, double density = 1.0) {
    if (!hertz_) throw std::logic_error("set_hertz_friction: call set_hertz_contact first");
    if (growth_) throw std::logic_error("set_hertz_friction: not combined with set_growth");
    for (double v : {mu, gamma_n, gamma_t, density})
      if (!(v >= 0.0 && v < HUGE_VAL))
        throw std::invalid_argument("set_hertz_friction: mu, the damping coefficients and the density must be finite "
                                    "and >= 0");
    friction_ = true;
    friction_params_ = linkers::FrictionalHertzParams{mu, gamma_n, gamma_t, density};
    prev_vel_ = DeviceVector(6 * n_ + 1);
    check(mhip_fill(6 * n_, prev_vel_.data(), 0.0, nullptr));
    num_hist_ = 0;
    have_hist_ = have_renumber_ = false;
  }

  /// The bacterial colony step (Bacteria.cpp:1033-1080), opt-in: every step first divides the rods with length >
  /// division_length (children appended as rows n + k, parent_of()[k] their parent) and grows every length by
  /// dt * growth_rate, then rebuilds the list iff there were births, force_rebuild, or some AABB corner moved by
  /// >= search_buffer since the last build -- the centre rule is not consulted.  Mobilities are carried as given
  /// (children copy their parent's).  Buffers are sized max(capacity_hint, n + n/8 + 16) and grow with headroom.
  void set_growth(double growth_rate, double division_length, size_t capacity_hint = 0) {
    if (friction_) throw std::logic_error("set_growth: not combined with set_hertz_friction");
    if (!(growth_rate >= 0.0 && growth_rate < HUGE_VAL))
      throw std::invalid_argument("set_growth: growth_rate must be finite and >= 0");
    if (!(division_length >= 0.0 && division_length < HUGE_VAL))
      throw std::invalid_argument("set_growth: division_length must be finite and >= 0");
    double rmax = 0.0;
    for (double r : radius_.download()) rmax = r > rmax ? r : rmax;
    if (division_length < 2.0 * rmax)
      throw std::invalid_argument("set_growth: division_length < 2 * max(radius): a child would have no length");
    growth_ = true;
    rate_ = growth_rate;
    division_ = division_length;
    reserve(capacity_hint > n_ + n_ / 8 + 16 ? capacity_hint : n_ + n_ / 8 + 16);
    have_ref_ = false;
  }

  StepStats step(bool integrate = true, bool force_rebuild = false) {
    StepStats st;
    if (growth_) st.num_born = grow_and_divide();
    double *sep = nullptr, *normal = nullptr, *s = nullptr, *t = nullptr;
    const size_t C = contacts(st, force_rebuild, sep, normal, s, t);
    if (friction_) {
      st.num_carried = carry_history(C);
      linkers::evaluate_frictional_linker_potentials(C, n_, pairs_.data(), sep, normal, s, t, seg_.data(), radius_.data(),
                                                     material_, prev_vel_.data(), friction_params_, dt_,
                                                     tang_disp_.data(), force_.data(), workspace(w_mx_, 2));
    } else if (hertz_) {
      double* f = workspace(lambda_, C);
      double* mx = workspace(w_mx_, 1);
      linkers::evaluate_linker_potentials(C, n_, pairs_.data(), sep, radius_.data(), material_, f, mx);
      num_lambda_ = C;
    }
    // the operator follows the contact list: rebuilt with it, otherwise only its geometry is refreshed
    if (st.rebuilt || !op_)
      op_.reset(new ContactOperator(C, n_, pairs_.data(), normal, ContactOperator::Rods{s, t, seg_.data()},
                                    mob_t_.data(), mob_r_.data(), dt_, nullptr, /*priority=*/sep));
    else
      op_->refresh(normal, ContactOperator::Rods{s, t, seg_.data()});
    ContactOperator& op = *op_;
    if (friction_) {
      op.linker_potential_force_reduction_vector(force_.data());
      st.converged = true;
      double h[2];
      check(mhip_memcpy_d2h(h, w_mx_.data(), sizeof h, nullptr));
      st.max_overlap = h[0];
      std::uint64_t k;
      std::memcpy(&k, &h[1], sizeof k);
      st.num_sliding = static_cast<size_t>(k);
    } else if (hertz_) {
      op.linker_potential_force_reduction(lambda_.data());
      st.converged = true;
      check(mhip_memcpy_d2h(&st.max_overlap, w_mx_.data(), sizeof(double), nullptr));
    } else {
      solve(op, C, sep, st);
    }
    if (integrate) {
      const double* vel = op.compute_generalized_velocity();
      if (friction_) check(mhip_deep_copy(6 * n_, prev_vel_.data(), vel, nullptr));  // the next step's StateN
      check(mhip_integrate_euler(n_, dt_, vel, center_.data(), quat_.data(), nullptr));
      // wrap_rigid_inplace(Spherocylinder): the centre goes back into the box (periodicity.hpp:1094-1113)
      if (periodic_) check(mhip_wrap_rigid(n_, box_, center_.data(), nullptr));
    }
    check(mhip_stream_synchronize(nullptr));
    return st;
  }

  size_t num_bodies() const { return n_; }
  /// per-body arrays: the first num_bodies() rows (growth mode: the buffers hold spare rows beyond)
  const DeviceVector& center() const { return center_; }
  const DeviceVector& quat() const { return quat_; }
  const DeviceVector& length() const { return length_; }
  /// growth mode: the parents of the last step's births, ascending (the first num_born entries)
  const DeviceArray<int32_t>& parent_of() const { return parent_of_; }
  /// multipliers of the last step (Hertz mode: the linker forces): the first num_lambda() entries (the buffer only
  /// ever grows)
  const DeviceVector& lambda() const { return lambda_; }
  size_t num_lambda() const { return num_lambda_; }
  const DeviceArray<int32_t>& pairs() const { return pairs_; }
  /// frictional Hertz mode: the linker forces [C][3] (on body i) and tangential displacements [C][3] of the last step,
  /// rows of pairs() (the first 3 * num_contacts entries)
  const DeviceVector& contact_force() const { return force_; }
  const DeviceVector& tang_disp() const { return tang_disp_; }

 private:
  /// compute_aabb -> neighbour list (rebuild rule) -> segments -> narrow phase; returns the number of contacts
  size_t contacts(StepStats& st, bool force_rebuild, double*& sep, double*& normal, double*& s, double*& t) {
    check(mhip_compute_aabb_spherocylinders(n_, center_.data(), quat_.data(), radius_.data(), length_.data(),
                                            aabb_.data(), nullptr));
    if (growth_) {
      // check_update_neighbor_list (Bacteria.cpp:685-748) against the AABBs of the last build; births force a rebuild
      int moved = 1;
      if (have_ref_ && !force_rebuild && st.num_born == 0)
        check(mhip_aabb_moved(n_, aabb_.data(), aabb_ref_.data(), buffer_, &moved, nullptr));
      st.rebuilt = moved != 0 && links_.generate(n_, aabb_.data(), center_.data(), brad_.data(), nullptr, true);
      if (st.rebuilt) {
        grow_keep(aabb_ref_, 6 * n_, 0);
        check(mhip_deep_copy(6 * n_, aabb_ref_.data(), aabb_.data(), nullptr));
        have_ref_ = true;
      }
    } else {
      st.rebuilt = links_.generate(n_, aabb_.data(), center_.data(), brad_.data(), nullptr, force_rebuild);
    }
    if (st.rebuilt) {
      links_.links_into(pairs_);
      ++links_generation_;
    }
    const size_t C = links_.num_links();
    st.num_contacts = C;
    check(mhip_spherocylinder_segments(n_, center_.data(), quat_.data(), radius_.data(), length_.data(), seg_.data(),
                                       nullptr));
    sep = workspace(w_sep_, C);
    normal = workspace(w_normal_, 3 * C);
    s = workspace(w_s_, C);
    t = workspace(w_t_, C);
    if (periodic_)
      check(mhip_contact_spherocylinders_periodic(C, pairs_.data(), seg_.data(), center_.data(), box_, sep, normal,
                                                  nullptr, nullptr, nullptr, nullptr, s, t, nullptr));
    else
      check(mhip_contact_spherocylinders(C, pairs_.data(), seg_.data(), nullptr, sep, normal, nullptr, nullptr,
                                         nullptr, nullptr, s, t, nullptr));
    return C;
  }
  /// frictional Hertz mode: the history follows the list.  After a rebuild (or a renumbering) every pair of the new list
  /// receives the row of the same pair of the list the history belongs to, every other pair +0.0.
  size_t carry_history(size_t C) {
    const bool moved = !have_hist_ || have_renumber_ || hist_list_ != links_generation_;
    if (!moved) return 0;
    DeviceVector next(3 * C + 1);
    size_t carried = 0;
    if (have_hist_)
      carried = linkers::carry_linker_history(num_hist_, hist_pairs_.data(), tang_disp_.data(),
                                              have_renumber_ ? renumber_.data() : nullptr, n_, C, pairs_.data(),
                                              next.data());
    else
      check(mhip_fill(3 * C, next.data(), 0.0, nullptr));
    tang_disp_ = std::move(next);
    force_ = DeviceVector(3 * C + 1);
    check(mhip_fill(3 * C, force_.data(), 0.0, nullptr));
    // a copy of the list the history now belongs to (pairs_ is overwritten by the next rebuild): 8 bytes per pair
    if (hist_pairs_.size() < 2 * C) hist_pairs_ = DeviceArray<int32_t>(2 * C + C / 4 + 16);
    check(mhip_deep_copy(C, reinterpret_cast<double*>(hist_pairs_.data()),
                         reinterpret_cast<const double*>(pairs_.data()), nullptr));
    num_hist_ = C;
    hist_list_ = links_generation_;
    have_hist_ = true;
    have_renumber_ = false;
    return carried;
  }
  /// reorder_bodies in frictional Hertz mode: the previous velocities move with their rows; the history keeps its old
  /// pair list and is carried through new_of_old (the inverse permutation) at the rebuild that follows
  void renumber_history() {
    DeviceVector moved(6 * n_ + 1);
    check(mhip_gather_rows(n_, 6, perm_.data(), prev_vel_.data(), moved.data(), nullptr));
    prev_vel_ = std::move(moved);
    if (!have_hist_) return;
    std::vector<int32_t> perm = perm_.download();
    perm.resize(n_);
    std::vector<int32_t> inv(n_);
    for (size_t k = 0; k < n_; ++k) inv[static_cast<size_t>(perm[k])] = static_cast<int32_t>(k);
    if (have_renumber_) {  // two reorders without a step between them compose
      const std::vector<int32_t> first = renumber_.download();
      std::vector<int32_t> both(n_);
      for (size_t b = 0; b < n_; ++b) both[b] = inv[static_cast<size_t>(first[b])];
      inv.swap(both);
    }
    renumber_ = DeviceArray<int32_t>(inv);
    have_renumber_ = true;
  }
  /// the LCP on the separations
  void solve(ContactOperator& op, size_t C, const double* sep, StepStats& st) {
    double *x = workspace(lambda_, C), *g = workspace(w_g_, C), *x_tmp = workspace(w_xt_, C),
           *g_tmp = workspace(w_gt_, C);
    num_lambda_ = C;
    const mhip_solve_result res = solve_lcp_from_zero(op, C, sep, cfg_, x, g, x_tmp, g_tmp);
    st.num_iters = res.num_iters;
    st.residual = res.residual;
    st.converged = res.converged != 0;
  }
  /// every per-body buffer holds at least `cap` rows (live rows kept)
  void reserve(size_t cap) {
    grow_keep(center_, 3 * cap, 3 * n_);
    grow_keep(quat_, 4 * cap, 4 * n_);
    grow_keep(radius_, cap, n_);
    grow_keep(length_, cap, n_);
    grow_keep(mob_t_, cap, n_);
    grow_keep(mob_r_, cap, n_);
    grow_keep(brad_, cap, n_);
    grow_keep(aabb_, 6 * cap, 0);
    grow_keep(seg_, 8 * cap, 0);
    grow_keep(tmp_, 4 * cap, 0);
    workspace(perm_, cap);
  }
  /// divide_bacteria -> grow_bacteria (Bacteria.cpp:926-966, :905-920) on the device; returns the birth count
  size_t grow_and_divide() {
    size_t nb = 0;
    // sized before the selection and never reallocated after it: nb <= n_, and reserve() leaves parent_of_ alone, so
    // the list the selection wrote is what the division and the row copies read
    workspace(parent_of_, n_ ? n_ : 1);
    check(mhip_select_dividing(n_, length_.data(), division_, parent_of_.data(), &nb, nullptr));
    if (nb) reserve(n_ + nb);
    check(mhip_divide_grow_spherocylinders(n_, nb, parent_of_.data(), dt_, rate_, periodic_ ? box_ : nullptr,
                                           center_.data(), quat_.data(), radius_.data(), length_.data(), nullptr));
    if (nb) {  // the other per-body fields of the parent go to the child
      check(mhip_gather_rows(nb, 1, parent_of_.data(), mob_t_.data(), mob_t_.data() + n_, nullptr));
      check(mhip_gather_rows(nb, 1, parent_of_.data(), mob_r_.data(), mob_r_.data() + n_, nullptr));
      n_ += nb;
    }
    check(mhip_bounding_radius_spherocylinders(n_, radius_.data(), length_.data(), brad_.data(), nullptr));
    return nb;
  }
  void gather(DeviceVector& a, size_t width) {
    check(mhip_gather_rows(n_, width, perm_.data(), a.data(), tmp_.data(), nullptr));
    check(mhip_deep_copy(width * n_, a.data(), tmp_.data(), nullptr));
  }
  size_t n_;
  double dt_;
  bool periodic_ = false;
  double box_[3] = {0.0, 0.0, 0.0};
  convex::PGDConfig<double> cfg_;
  DeviceVector center_, quat_, radius_, length_, mob_t_, mob_r_, brad_, aabb_, seg_, tmp_, lambda_;
  DeviceVector w_sep_, w_normal_, w_s_, w_t_, w_g_, w_xt_, w_gt_, w_mx_;  // per-step workspaces (grow-only)
  size_t num_lambda_ = 0;
  bool hertz_ = false;
  linkers::HertzMaterial material_;
  bool friction_ = false, have_hist_ = false, have_renumber_ = false;
  linkers::FrictionalHertzParams friction_params_;
  DeviceVector prev_vel_, tang_disp_, force_;  // [n][6] previous velocities; [C][3] history and linker forces
  DeviceArray<int32_t> hist_pairs_, renumber_;  // the list tang_disp_ belongs to; new index of every old body
  size_t num_hist_ = 0;
  unsigned long long links_generation_ = 0, hist_list_ = 0;
  bool growth_ = false, have_ref_ = false;
  double rate_ = 0.0, division_ = 0.0, buffer_ = 0.0;
  DeviceVector aabb_ref_;  // growth mode: the AABBs of the last build
  DeviceArray<int32_t> perm_, pairs_, parent_of_;
  mesh::GenNeighborLinks links_;
  std::unique_ptr<ContactOperator> op_;
};

// One rank's share of a spherocylinder system cut along a space-filling curve: this rank owns the bodies
// with global ids [gid_first, gid_first + n), ranks own increasing ranges.  step() =
//   compute_aabb(owned) -> ghost plan + body-record exchange (coarse_search(comm) + change_ghosting,
//   GenNeighborLinkers.hpp:658, :687-711) -> neighbour list over owned + ghosts, ghost-ghost pairs dropped, interior
//   contacts first -> contacts -> rod operator with the owned range -> domain-decomposed BBPGD (velocity halo + 3-double
//   all-gather per iteration, NGPSpheresLCP.cpp:371, :450-452) -> Euler update of the owned bodies.
// The communicator is the caller's (mhip_comm_create_rccl with an id the launcher hands round, or a host transport).
class DistributedSpherocylinderStepper {
 public:
  // gid, centre 3, quaternion 4, radius, length, translational / rotational mobility, entity id (what a body keeps when
  // it changes owner; the gid is its position in the current ownership order)
  static constexpr size_t kRecord = 13;

  DistributedSpherocylinderStepper(mhip_comm_t comm, size_t gid_first, const std::vector<double>& center,
                                   const std::vector<double>& quat, const std::vector<double>& radius,
                                   const std::vector<double>& length, const std::vector<double>& mob_trans,
                                   const std::vector<double>& mob_rot, double dt, double search_buffer,
                                   convex::PGDConfig<double> cfg)
      : comm_(comm), n_(radius.size()), dt_(dt), buffer_(search_buffer), cfg_(cfg), center_(center), quat_(quat),
        radius_(radius), length_(length), mob_t_(mob_trans), mob_r_(mob_rot), aabb_(6 * n_), rec_(kRecord * n_) {
    std::vector<double> gid(n_);
    for (size_t i = 0; i < n_; ++i) gid[i] = static_cast<double>(gid_first + i);
    gid_ = DeviceVector(gid);
    entity_ = DeviceVector(gid);  // until set_entity_ids: a body's id is its first global position
    links_.set_search_buffer(search_buffer).set_search_kind(MHIP_SEARCH_AABB).concretize();
  }

  /// ids the bodies keep for life (integer-valued, below 2^40); default: the global position at construction
  void set_entity_ids(const std::vector<double>& ids) {
    if (ids.size() != n_) throw std::invalid_argument("set_entity_ids: one id per owned body");
    check_entity_ids(ids);
    entity_ = DeviceVector(ids);
  }
  /// throws std::invalid_argument unless every id is an integer in [0, 2^40): rebalance() orders the owned bodies by
  /// (cell key << 40) | id (mhip_compose_keys_u64), which a larger, negative or fractional id would corrupt
  static void check_entity_ids(const std::vector<double>& ids) {
    constexpr double kBound = 1099511627776.0;  // 2^40
    for (size_t i = 0; i < ids.size(); ++i) {
      const double e = ids[i];
      if (!(e >= 0.0 && e < kBound && e == std::floor(e)))  // NaN and +-inf fail too
        throw std::invalid_argument("set_entity_ids: entity ids must be integers in [0, 2^40); id " +
                                    std::to_string(e) + " at index " + std::to_string(i) + " is not");
    }
  }
  /// The lattice the ownership is cut on: (2^level)^3 cells over [lo, hi], visited along mundy::math::hilbert_3d
  /// (Hilbert.hpp:48-83).  Needed by rebalance() / step(..., migrate = true).
  void set_domain(const double lo[3], const double hi[3], int curve_level = 4, int recut_every = 4) {
    for (int a = 0; a < 3; ++a) {
      dom_lo_[a] = lo[a];
      dom_hi_[a] = hi[a];
    }
    level_ = curve_level;
    recut_every_ = recut_every;
    const size_t side = static_cast<size_t>(1) << level_;
    std::vector<int32_t> table(side * side * side);
    check(mhip_hilbert_key_table(level_, table.data()));
    key_table_ = DeviceArray<int32_t>(table);
    have_domain_ = true;
  }

  struct MigrateStats {
    size_t sent = 0, received = 0, owned = 0;
    bool recut = false;
  };
  /// Ownership follows the bodies (replaces stk::balance::balanceStkMesh, NGPSpheresLCP.cpp:956, called every
  /// load_balance_frequency steps, Bacteria.cpp:1076-1078): every owned body moves to the rank that owns its lattice
  /// cell; recut first re-cuts the curve at equal work (1 + contacts per body in the last step).  The owned set ends up
  /// in (cell, entity id) order -- the order a single rank would hold it in.  Collective.
  MigrateStats rebalance(bool recut = true) {
    if (!have_domain_) throw std::runtime_error("rebalance() needs set_domain(lo, hi, level) first");
    int rank = 0, world = 1;
    check(mhip_comm_info(comm_, &rank, &world, nullptr));
    DeviceArray<uint32_t> keys(n_ ? n_ : 1);
    check(mhip_curve_keys(n_, center_.data(), dom_lo_, dom_hi_, level_, key_table_.data(), keys.data(), nullptr));
    MigrateStats ms;
    if (recut || splitters_.size() + 1 != static_cast<size_t>(world)) {
      splitters_.assign(world > 1 ? static_cast<size_t>(world - 1) : 1, 0);
      const size_t ncell = static_cast<size_t>(1) << (3 * level_);
      check(mhip_curve_cut(comm_, n_, keys.data(), weight_.size() == n_ && n_ ? weight_.data() : nullptr, ncell,
                           splitters_.data(), nullptr));
      splitters_.resize(static_cast<size_t>(world - 1));
      ms.recut = true;
    }
    pack_records();
    size_t n_new = 0;
    const int64_t none = 0;
    check(mhip_migrate_plan(comm_, n_, keys.data(), world > 1 ? splitters_.data() : &none, &n_new, &ms.sent, &ms.received,
                            nullptr));
    DeviceVector arrived(kRecord * (n_new ? n_new : 1)), sorted(kRecord * (n_new ? n_new : 1));
    check(mhip_migrate_exchange(comm_, kRecord, rec_.data(), arrived.data(), nullptr));
    // (cell, entity id) order
    DeviceVector c_new(3 * (n_new ? n_new : 1)), e_new(n_new ? n_new : 1);
    check(mhip_copy_strided(n_new, 3, arrived.data() + 1, kRecord, c_new.data(), 3, nullptr));
    check(mhip_copy_strided(n_new, 1, arrived.data() + 12, kRecord, e_new.data(), 1, nullptr));
    DeviceArray<uint32_t> k_new(n_new ? n_new : 1);
    DeviceArray<uint64_t> k64(n_new ? n_new : 1);
    DeviceArray<int32_t> perm(n_new ? n_new : 1);
    check(mhip_curve_keys(n_new, c_new.data(), dom_lo_, dom_hi_, level_, key_table_.data(), k_new.data(), nullptr));
    check(mhip_compose_keys_u64(n_new, k_new.data(), e_new.data(), 40, k64.data(), nullptr));
    check(mhip_sort_by_key_u64(n_new, k64.data(), perm.data(), nullptr));
    check(mhip_gather_rows(n_new, kRecord, perm.data(), arrived.data(), sorted.data(), nullptr));
    // the new owned set, global positions = after the lower ranks' bodies
    n_ = n_new;
    double mine = static_cast<double>(n_);
    DeviceVector sizes(1 + static_cast<size_t>(world));
    check(mhip_memcpy_h2d(sizes.data(), &mine, sizeof mine, nullptr));
    check(mhip_comm_all_gather(comm_, sizes.data(), 1, sizes.data() + 1, nullptr));
    std::vector<double> all(static_cast<size_t>(world));
    check(mhip_memcpy_d2h(all.data(), sizes.data() + 1, all.size() * sizeof(double), nullptr));
    double gid_first = 0.0;
    for (int r = 0; r < rank; ++r) gid_first += all[static_cast<size_t>(r)];
    const size_t cap = n_ ? n_ : 1;
    gid_ = DeviceVector(cap); center_ = DeviceVector(3 * cap); quat_ = DeviceVector(4 * cap); radius_ = DeviceVector(cap);
    length_ = DeviceVector(cap); mob_t_ = DeviceVector(cap); mob_r_ = DeviceVector(cap); entity_ = DeviceVector(cap);
    aabb_ = DeviceVector(6 * cap); rec_ = DeviceVector(kRecord * cap);
    check(mhip_fill_sequence(n_, gid_first, gid_.data(), nullptr));
    struct { DeviceVector* v; size_t w, col; } out[] = {{&center_, 3, 1}, {&quat_, 4, 4}, {&radius_, 1, 8}, {&length_, 1, 9},
                                                        {&mob_t_, 1, 10}, {&mob_r_, 1, 11}, {&entity_, 1, 12}};
    for (const auto& f : out) check(mhip_copy_strided(n_, f.w, sorted.data() + f.col, kRecord, f.v->data(), f.w, nullptr));
    check(mhip_stream_synchronize(nullptr));
    // everything indexed by the old numbering goes
    links_.invalidate();
    op_.reset();
    lay_ = mhip_ghost_layout{};
    weight_ = DeviceVector();
    ++rebalances_;
    ms.owned = n_;
    return ms;
  }

  struct DistStats : StepStats {
    size_t ghosts = 0, local_contacts = 0, interior_contacts = 0, owned_contacts = 0;
    size_t migrated_out = 0, migrated_in = 0;
  };

  /// force_rebuild = false applies the reference's rebuild rule across the ranks: the ghosts' current state travels
  /// through the plan of the last rebuild, every rank tests its local bodies (owned + ghosts) against half the search
  /// buffer (GenNeighborLinkers.hpp:603-615), one all-gather of the flags decides for everybody; without a rebuild the
  /// ghost layout, the partitioned pair list and the operator's incidence index are kept.
  DistStats step(bool integrate = true, bool force_rebuild = true, bool migrate = false) {
    DistStats st;
    if (migrate && (force_rebuild || !op_)) {  // bodies change owner at a rebuild only (the lists are rebuilt anyway)
      const bool recut = splitters_.empty() || (recut_every_ > 0 && rebalances_ % static_cast<unsigned>(recut_every_) == 0);
      const MigrateStats ms = rebalance(recut);
      st.migrated_out = ms.sent;
      st.migrated_in = ms.received;
    }
    // the owned fields interleaved into records (what travels to the ranks that hold these bodies as ghosts)
    const struct { const DeviceVector* v; size_t w; } fields[] = {{&gid_, 1},    {&center_, 3}, {&quat_, 4},  {&radius_, 1},
                                                                  {&length_, 1}, {&mob_t_, 1},  {&mob_r_, 1}, {&entity_, 1}};
    pack_records();
    auto exchange_and_split = [&]() {  // records through the current plan, then split into fields again
      const size_t nl = lay_.num_ghost_lo + n_ + lay_.num_ghost_hi;
      double* local = workspace(w_local_, kRecord * nl);
      check(mhip_ghost_exchange(comm_, kRecord, rec_.data(), local, nullptr));
      double* l_field[8] = {workspace(l_gid_, nl),    workspace(l_center_, 3 * nl), workspace(l_quat_, 4 * nl),
                            workspace(l_radius_, nl), workspace(l_length_, nl),     workspace(l_mt_, nl),
                            workspace(l_mr_, nl),     workspace(l_entity_, nl)};
      size_t c0 = 0;
      for (size_t k = 0; k < 8; ++k) {
        check(mhip_copy_strided(nl, fields[k].w, local + c0, kRecord, l_field[k], fields[k].w, nullptr));
        c0 += fields[k].w;
      }
      return nl;
    };
    bool reuse = false;
    size_t nl = 0;
    if (!force_rebuild && op_) {
      nl = exchange_and_split();
      double flag = links_.objects_moved_too_much(nl, l_center_.data()) ? 1.0 : 0.0;
      int world = 1;
      check(mhip_comm_info(comm_, nullptr, &world, nullptr));
      double* d = workspace(w_flags_, 1 + static_cast<size_t>(world));
      check(mhip_memcpy_h2d(d, &flag, sizeof flag, nullptr));
      check(mhip_comm_all_gather(comm_, d, 1, d + 1, nullptr));
      std::vector<double> all(static_cast<size_t>(world));
      check(mhip_memcpy_d2h(all.data(), d + 1, all.size() * sizeof(double), nullptr));
      reuse = true;
      for (double f : all) reuse = reuse && f == 0.0;
    }
    if (!reuse) {
      check(mhip_compute_aabb_spherocylinders(n_, center_.data(), quat_.data(), radius_.data(), length_.data(),
                                              aabb_.data(), nullptr));
      check(mhip_ghost_plan(comm_, n_, aabb_.data(), buffer_, &lay_, nullptr));
      nl = exchange_and_split();
    }
    const size_t n_lo = lay_.num_ghost_lo;
    st.ghosts = nl - n_;
    st.rebuilt = !reuse;
    double *l_center = l_center_.data(), *l_quat = l_quat_.data(), *l_radius = l_radius_.data(),
           *l_length = l_length_.data();
    double* seg = workspace(w_seg_, 8 * nl);
    if (!reuse) {
      // neighbour list over owned + ghosts; ghost-ghost pairs dropped, interior contacts first
      double *l_aabb = workspace(w_aabb_, 6 * nl), *l_brad = workspace(w_brad_, nl);
      check(mhip_compute_aabb_spherocylinders(nl, l_center, l_quat, l_radius, l_length, l_aabb, nullptr));
      check(mhip_bounding_radius_spherocylinders(nl, l_radius, l_length, l_brad, nullptr));
      links_.generate(nl, l_aabb, l_center, l_brad, nullptr, /*force=*/true);
      const int32_t* all_pairs = links_.links_into(w_all_pairs_);
      const size_t c_all = links_.num_links();
      int32_t* pairs = workspace(w_pairs_, 2 * c_all + 2);
      unsigned char* counted = workspace(w_counted_, c_all + 1);
      check(mhip_partition_pairs_owned(c_all, all_pairs, n_lo, n_, pairs, counted, &n_int_, &num_contacts_, nullptr));
      // work per owned body for the next re-cut of the curve: 1 + its contacts
      if (have_domain_) {
        weight_ = DeviceVector(n_ ? n_ : 1);
        check(mhip_body_work_weights(num_contacts_, pairs, n_lo, n_, weight_.data(), nullptr));
      }
    }
    const size_t C = num_contacts_;
    const int32_t* pairs = w_pairs_.data();
    st.num_contacts = st.local_contacts = C;
    st.interior_contacts = n_int_;
    check(mhip_spherocylinder_segments(nl, l_center, l_quat, l_radius, l_length, seg, nullptr));
    double *sep = workspace(w_sep_, C), *normal = workspace(w_normal_, 3 * C), *s = workspace(w_s_, C),
           *t = workspace(w_t_, C);
    check(mhip_contact_spherocylinders(C, pairs, seg, nullptr, sep, normal, nullptr, nullptr, nullptr, nullptr, s, t,
                                       nullptr));
    if (reuse)
      op_->refresh(normal, ContactOperator::Rods{s, t, seg});
    else
      op_.reset(new ContactOperator(C, nl, pairs, normal, ContactOperator::Rods{s, t, seg}, l_mt_.data(), l_mr_.data(),
                                    dt_, nullptr, /*priority=*/sep));
    ContactOperator& op = *op_;
    double* vel = workspace(w_vel_, 6 * nl);
    check(mhip_fill(6 * nl, vel, 0.0, nullptr));
    check(mhip_contact_op_set_partition(op.handle(), n_lo, n_, w_counted_.data(), vel));
    lay_.halo.velocity = vel;
    double *x = workspace(lambda_, C), *g = workspace(w_g_, C), *x_tmp = workspace(w_xt_, C),
           *g_tmp = workspace(w_gt_, C);
    check(mhip_fill(C, x, 0.0, nullptr));
    num_lambda_ = C;
    const mhip_space lcp{MHIP_SPACE_LOWER_BOUND, 0.0, 0.0};
    const mhip_pgd_config pc{cfg_.max_iters, cfg_.tol, MHIP_RESIDUAL_PROJECTED_DIFF};
    mhip_solve_result res{};
    check(mhip_bbpgd_solve_contact_distributed(op.handle(), comm_, &lay_.halo, n_int_, sep, &lcp, &pc, x, g, x_tmp,
                                               g_tmp, /*poll_every=*/64, &res, nullptr, nullptr));
    st.num_iters = res.num_iters;
    st.residual = res.residual;
    st.converged = res.converged != 0;
    if (integrate) {
      const double* v = nullptr;
      check(mhip_contact_op_body_velocity(op.handle(), &v));
      check(mhip_integrate_euler(n_, dt_, v + 6 * n_lo, l_center + 3 * n_lo, l_quat + 4 * n_lo, nullptr));
      check(mhip_deep_copy(3 * n_, center_.data(), l_center + 3 * n_lo, nullptr));
      check(mhip_deep_copy(4 * n_, quat_.data(), l_quat + 4 * n_lo, nullptr));
    }
    check(mhip_stream_synchronize(nullptr));
    return st;
  }

  size_t num_bodies() const { return n_; }
  const DeviceVector& center() const { return center_; }
  const DeviceVector& quat() const { return quat_; }
  const DeviceVector& entity_ids() const { return entity_; }
  const std::vector<int64_t>& splitters() const { return splitters_; }
  /// multipliers of the last step: the first num_lambda() entries (the buffer only ever grows)
  const DeviceVector& lambda() const { return lambda_; }
  size_t num_lambda() const { return num_lambda_; }

 private:
  void pack_records() {
    const struct { const DeviceVector* v; size_t w; } fields[] = {{&gid_, 1},    {&center_, 3}, {&quat_, 4},  {&radius_, 1},
                                                                  {&length_, 1}, {&mob_t_, 1},  {&mob_r_, 1}, {&entity_, 1}};
    size_t col = 0;
    for (const auto& f : fields) {
      check(mhip_copy_strided(n_, f.w, f.v->data(), f.w, rec_.data() + col, kRecord, nullptr));
      col += f.w;
    }
  }
  mhip_comm_t comm_;
  size_t n_;
  double dt_, buffer_;
  convex::PGDConfig<double> cfg_;
  DeviceVector center_, quat_, radius_, length_, mob_t_, mob_r_, aabb_, rec_, gid_, entity_, weight_, lambda_;
  // ownership lattice (set_domain) and the current cuts of the curve
  bool have_domain_ = false;
  double dom_lo_[3] = {0, 0, 0}, dom_hi_[3] = {1, 1, 1};
  int level_ = 4, recut_every_ = 4;
  unsigned rebalances_ = 0;
  DeviceArray<int32_t> key_table_;
  std::vector<int64_t> splitters_;
  // per-step workspaces (grow-only): local records and fields, geometry, contacts, solver vectors
  DeviceVector w_local_, l_gid_, l_center_, l_quat_, l_radius_, l_length_, l_mt_, l_mr_, l_entity_, w_aabb_, w_brad_, w_seg_,
      w_sep_, w_normal_, w_s_, w_t_, w_vel_, w_g_, w_xt_, w_gt_;
  DeviceVector w_flags_;
  DeviceArray<int32_t> w_pairs_, w_all_pairs_;
  DeviceArray<unsigned char> w_counted_;
  size_t num_lambda_ = 0, n_int_ = 0, num_contacts_ = 0;
  mhip_ghost_layout lay_{};  // of the last rebuild; its lists live in the communicator until the next plan
  mesh::GenNeighborLinks links_;
  std::unique_ptr<ContactOperator> op_;
};

/// The bead-spring chain step of the chromatin / HP1 family (NgpHP1.cpp:3802-3990) on spheres in free space, with the
/// contact LCP: springs, Brownian noise, contacts, Euler update.  The step is four stages, called in this order; a host
/// program adds its own terms to force() and u_ext() between them, where the reference's step has them
/// (HP1.cpp:4733-4803):
///   neighbors() -> forces() -> external_velocity() -> resolve()
/// set_hertz_contact(E, nu, true) makes it the reference's own order with the Hertzian soft contact (HP1.cpp:4728-4803):
/// the contact force is the first term of the force field, so everything computed from force() sees it, and no solve
/// and no body sweep follow:
///   neighbors() -> contact_forces() -> forces() -> external_velocity() -> resolve()      (U = U_ext)
/// step() is the stages in a row.  The only host reads of a step are the neighbour list's rebuild test, the solver's
/// convergence polls and, at the end of every resolve(), two small blocking downloads: the longest spring and the
/// overstretched count, whether the caller looks at them or not.  They are what resolve() waits for the step with.
/// The HP1 stages are options, each a setter called before the first step:
///   set_crosslinkers [+ set_periphery_sites], set_periphery, set_active_springs     terms of forces(), in the
///     reference's order (HP1.cpp:4733-4741): KMC -> active sampling -> springs -> crosslinker springs -> periphery
///     -> active dipoles; their statistics share one device array that resolve() downloads once
///   set_hydrodynamics [+ set_hydro_periphery]     u_hydro of force(), added to U_ext after the noise (:4744-4803)
///   set_angular_springs, set_spring_wca     the bending term after the springs, and the WCA part of FENE-WCA bonds
///     (mundy_hip_bending.h); the angular statistics have a device array of their own
class SphereChainStepper {
 public:
  /// host arrays: center [n][3], radius [n], mob_trans [n]; spring_pairs [m][2] with one stiffness and one rest length
  /// (Hookean) or r_max (FENE, FENE-WCA) for all, spring_type MHIP_SPRING_*; keys [n] of the noise or empty = the body indices
  /// (the counters start at 0)
  SphereChainStepper(const std::vector<double>& center, const std::vector<double>& radius,
                     const std::vector<double>& mob_trans, double dt, double search_buffer,
                     convex::PGDConfig<double> cfg, const std::vector<int32_t>& spring_pairs, int spring_type,
                     double spring_k, double spring_r, double kt, const std::vector<std::uint64_t>& keys = {})
      : n_(radius.size()), dt_(dt), kt_(kt), cfg_(cfg), center_(center), radius_(radius), mob_t_(mob_trans),
        aabb_(6 * n_), force_(3 * n_), u_ext_(6 * n_), vel_(6 * n_), counters_(std::vector<std::uint64_t>(n_, 0)),
        springs_(n_, spring_pairs, spring_type, {}, spring_k, {}, spring_r) {
    if (!keys.empty() && keys.size() != n_) throw std::invalid_argument("SphereChainStepper: one key per body");
    std::vector<std::uint64_t> k(keys);
    if (k.empty())
      for (size_t i = 0; i < n_; ++i) k.push_back(i);
    keys_ = DeviceArray<std::uint64_t>(k);
    links_.set_search_buffer(search_buffer).set_search_kind(MHIP_SEARCH_AABB).concretize();
  }

  /// the neighbour list by the rebuild rule; returns whether it was rebuilt (pairs() changes only then)
  bool neighbors() {
    if (!sphere_contacts_) return false;
    check(mhip_compute_aabb_spheres(n_, center_.data(), radius_.data(), aabb_.data(), nullptr));
    rebuilt_ = links_.generate(n_, aabb_.data(), center_.data(), radius_.data(), nullptr, false);
    if (rebuilt_) links_.links_into(pairs_);
    return rebuilt_;
  }
  /// The Hertzian soft contact (E > 0, 0 < nu < 1) instead of the LCP.  contact_forces_in_force_stage must be true: the
  /// Hertz force is then the first term of force() (contact_forces()), as the reference has it; the other order -- a body
  /// sweep after U_ext -- is the Python stepper's default and is not wired here.
  void set_hertz_contact(double youngs_modulus, double poisson_ratio, bool contact_forces_in_force_stage) {
    if (!(youngs_modulus > 0.0) || !(poisson_ratio > 0.0 && poisson_ratio < 1.0))
      throw std::invalid_argument("SphereChainStepper: youngs_modulus must be > 0 and 0 < poisson_ratio < 1");
    if (!contact_forces_in_force_stage)
      throw std::invalid_argument("SphereChainStepper: the Hertz contact runs with its force in the force stage only");
    if (hydro_solve_)
      throw std::invalid_argument("SphereChainStepper: the hydrodynamic solve is the LCP's: no Hertz contact with it");
    material_.youngs_modulus = youngs_modulus;
    material_.poisson_ratio = poisson_ratio;
    hertz_ = true;
    if (max_overlap_.size() == 0) max_overlap_ = DeviceVector(1);
    if (spring_term_.size() == 0) spring_term_ = DeviceVector(3 * n_);
  }
  /// Hertz mode, between neighbors() and forces(): contacts -> Hertz force per linker -> operator (built after a rebuild,
  /// otherwise refreshed) -> the contact force of every body F = D f into force() [n][3]; returns it
  double* contact_forces() {
    if (!sphere_contacts_) return force_.data();
    if (!hertz_) throw std::logic_error("SphereChainStepper: contact_forces() needs set_hertz_contact");
    const size_t C = links_.num_links(), cap = C ? C : 1;  // no workspace is null without contacts
    double *sep = workspace(w_sep_, cap), *normal = workspace(w_normal_, 3 * cap), *f = workspace(lambda_, cap);
    check(mhip_contact_spheres(C, pairs_.data(), center_.data(), radius_.data(), nullptr, sep, normal, nullptr));
    linkers::evaluate_linker_potentials(C, n_, pairs_.data(), sep, radius_.data(), material_, f, max_overlap_.data());
    if (rebuilt_ || !op_)
      op_.reset(new ContactOperator(C, n_, pairs_.data(), normal, nullptr, nullptr, mob_t_.data(), nullptr, dt_,
                                    nullptr, /*priority=*/sep));
    else
      op_->refresh(normal, nullptr, nullptr);
    num_lambda_ = C;
    op_->body_force(f, force_.data(), 3);
    have_contact_force_ = true;
    return force_.data();
  }
  /// The backbone excluded volume (mech::SegmentContacts; host arrays ends [m][2], radius [m] or empty with
  /// radius_scalar, end_correction [m] bytes or empty): the term at the head of forces() after the sampling, added to the
  /// contact force in Hertz mode, written first otherwise; the springs then go through a buffer of their own.  Its list is
  /// brought up to date at the start of forces().
  void set_backbone_collision(const mhip_segment_contact_params& params, const std::vector<int32_t>& ends,
                              const std::vector<double>& radius, double radius_scalar,
                              const std::vector<unsigned char>& end_correction) {
    backbone_.reset(new SegmentContacts(n_, ends, radius, radius_scalar, end_correction, params));
    backbone_stats_ = DeviceArray<std::uint64_t>(std::vector<std::uint64_t>(2, 0));
    if (spring_term_.size() == 0) spring_term_ = DeviceVector(3 * n_);
  }
  /// false: no sphere contact at all -- neighbors() and contact_forces() do nothing and resolve() is U = U_ext, the
  /// reference's own configuration.  Needs set_backbone_collision first: something has to keep the chains apart.
  void set_sphere_contacts(bool on) {
    if (!on && !backbone_)
      throw std::logic_error("SphereChainStepper: set_sphere_contacts(false) needs set_backbone_collision first");
    if (!on && hydro_solve_)
      throw std::invalid_argument("SphereChainStepper: the hydrodynamic solve needs the sphere contacts");
    sphere_contacts_ = on;
  }
  /// Crosslinkers that bind and unbind (mech::Crosslinkers; host arrays left [mx], is_site [n] bytes): their KMC step
  /// opens forces(), the doubly bound ones follow the backbone as springs of `type`.  Every crosslinker starts singly
  /// bound; rng keys are the crosslinker indices, counters start at 0, candidate rows are walked by body index.  The
  /// candidate list is a search of its own (reach capture_radius / 2, buffer skin) under the displacement rule.
  void set_crosslinkers(const std::vector<int32_t>& left, const std::vector<unsigned char>& is_site, int type, double k,
                        double r, double bind_rate, double unbind_rate, double kt, double capture_radius, double skin) {
    xl_.reset(new Crosslinkers(n_, left, is_site, type, k, r, bind_rate, unbind_rate, kt, capture_radius));
    std::vector<std::uint64_t> key(left.size());
    for (size_t c = 0; c < key.size(); ++c) key[c] = c;
    xl_keys_ = DeviceArray<std::uint64_t>(key);
    xl_counters_ = DeviceArray<std::uint64_t>(std::vector<std::uint64_t>(left.size(), 0));
    std::vector<std::int64_t> id(n_);
    for (size_t i = 0; i < n_; ++i) id[i] = static_cast<std::int64_t>(i);
    ids_ = DeviceArray<std::int64_t>(id);
    xl_sources_.assign(n_, 0);
    for (int32_t l : left) xl_sources_[static_cast<size_t>(l)] = 1;
    xl_skin_ = skin;
    xl_search_.reset(new CandidateSearch(xl_sources_, is_site, 0.5 * capture_radius, skin));
    use_stats();
  }
  /// Immobile bind sites on the periphery (points [P][3], host), after set_crosslinkers: a second candidate list over
  /// the beads followed by the sites, sources the same beads, targets the sites
  void set_periphery_sites(const std::vector<double>& points, double bind_rate, double k, double r, double unbind_rate,
                           double capture_radius) {
    if (!xl_) throw std::logic_error("SphereChainStepper: set_periphery_sites needs set_crosslinkers first");
    const size_t P = points.size() / 3;
    std::vector<double> all = center_.download();
    all.insert(all.end(), points.begin(), points.end());
    site_all_ = DeviceVector(all);
    xl_->set_periphery_sites(P, site_all_.data() + 3 * n_, bind_rate, k, r, unbind_rate, capture_radius);
    std::vector<unsigned char> sources(xl_sources_), targets(n_, 0);
    sources.resize(n_ + P, 0);
    targets.resize(n_ + P, 1);
    site_search_.reset(new CandidateSearch(sources, targets, 0.5 * capture_radius, xl_skin_));
  }
  /// The nuclear wall (mhip_periphery_force): one term of forces()
  void set_periphery(const mhip_periphery& wall) {
    wall_ = wall;
    have_wall_ = true;
    use_stats();
  }
  /// The WCA part of MHIP_SPRING_FENEWCA backbone springs (epsilon, sigma > 0; 1 and 1 until set)
  void set_spring_wca(double epsilon, double sigma) { springs_.set_wca(epsilon, sigma); }
  /// Angular springs (mech::AngularSprings; host triplets [ma][3] = (end, end, centre), one stiffness and one rest angle
  /// for all): the term of forces() after the springs and before the crosslinker springs (SpringsUpdated.cpp:1844)
  void set_angular_springs(const std::vector<int32_t>& triplets, double k, double rest_angle) {
    angular_.reset(new AngularSprings(n_, triplets, {}, k, {}, rest_angle));
    angular_stats_ = DeviceVector(2);  // (max deviation, the degenerate count in the low int of the second word)
  }
  /// Active force dipoles (mech::ActiveSprings; host pairs [ma][2]): sampled in forces() before the springs, their
  /// force its last term, their timers advanced by resolve()
  void set_active_springs(const std::vector<int32_t>& pairs, double sigma, double kon, double koff) {
    active_.reset(new ActiveSprings(n_, pairs, sigma, kon, koff));
    use_stats();
  }
  /// N-body hydrodynamics (kind MHIP_HYDRO_*, the beads' own radii): external_velocity() adds the stored u_hydro of
  /// force() to U_ext on every step and recomputes it when step_index() % update_every == 0
  void set_hydrodynamics(int kind, double viscosity, int update_every) {
    if (update_every < 1) throw std::invalid_argument("SphereChainStepper: update_every must be >= 1");
    if (hydro_solve_ && kind != MHIP_HYDRO_RPYC && kind != MHIP_HYDRO_RPY)
      throw std::invalid_argument("SphereChainStepper: the hydrodynamic solve needs MHIP_HYDRO_RPYC or MHIP_HYDRO_RPY");
    hydro_.reset(new Hydrodynamics());
    hydro_kind_ = kind;
    viscosity_ = viscosity;
    update_every_ = static_cast<size_t>(update_every);
    u_hydro_ = DeviceVector(3 * n_);
  }
  /// true: resolve() solves the LCP against M_h = m_t + hydro_kind (+ the periphery's correction, where one is set) at
  /// the current positions, as the reference's newer chromatin app does (NgpHP1.cpp:1487-1645), so U = U_ext + M_h D
  /// lambda; U_ext and q are unchanged.  Needs set_hydrodynamics (RPYC or RPY: the Stokeslet is not positive
  /// semi-definite at bead separations) and the LCP model with sphere contacts.  false: the dry solve, the default.
  void set_hydrodynamic_solve(bool on) {
    if (on) {
      if (!hydro_) throw std::logic_error("SphereChainStepper: set_hydrodynamic_solve needs set_hydrodynamics first");
      if (hertz_ || !sphere_contacts_)
        throw std::invalid_argument("SphereChainStepper: the hydrodynamic solve needs the LCP contact model");
      if (hydro_kind_ != MHIP_HYDRO_RPYC && hydro_kind_ != MHIP_HYDRO_RPY)
        throw std::invalid_argument("SphereChainStepper: the hydrodynamic solve needs MHIP_HYDRO_RPYC or MHIP_HYDRO_RPY");
    }
    hydro_solve_ = on;
  }
  /// The no-slip periphery of the hydrodynamics (host quadrature arrays), after set_hydrodynamics: its matrix is filled
  /// and inverted here (min_pivot()), its correction goes into u_hydro at every update
  void set_hydro_periphery(const std::vector<double>& points, const std::vector<double>& weights,
                           const std::vector<double>& normals, bool skip_same_index) {
    if (!hydro_) throw std::logic_error("SphereChainStepper: set_hydro_periphery needs set_hydrodynamics first");
    hydro_periphery_.reset(new HydroPeriphery(points, weights, normals, viscosity_));
    hydro_periphery_->fill_matrix();
    min_pivot_ = hydro_periphery_->invert();
    skip_same_index_ = skip_same_index;
  }
  /// The force stage in the reference's order (HP1.cpp:4733-4741) into force() [n][3]: crosslinker KMC, active sampling,
  /// backbone segment contacts (Hertz mode: added to the contact force that contact_forces() left there), springs (added
  /// to what is there in Hertz mode or after the segment contacts), angular springs, crosslinker springs, periphery,
  /// active dipoles, every term after the springs added to them.  Returns force() for the caller to accumulate further
  /// terms into.
  double* forces() {
    const bool first_term = hertz_ && sphere_contacts_;  // force() holds D f
    if (first_term && !have_contact_force_) throw std::logic_error("SphereChainStepper: forces() before contact_forces()");
    const double* x = center_.data();
    double* f = force_.data();
    if (stats_.size()) check(mhip_fill(stats_.size(), stats_.data(), 0.0, nullptr));
    if (backbone_) segment_list_rebuilt_ = backbone_->update(x);
    if (xl_) crosslinker_kmc();
    if (active_) active_->sample(stat_int(8, 0));
    if (backbone_) backbone_->force(x, f, first_term, backbone_stats_.data());
    if (first_term || backbone_) {  // (the spring kernel overwrites: its term goes through a buffer of its own)
      springs_.compute_forces(x, spring_term_.data());
      check(mhip_axpby(3 * n_, 1.0, spring_term_.data(), 1.0, f, nullptr));
    } else {
      springs_.compute_forces(x, f);
    }
    if (angular_)
      angular_->force(x, f, true, reinterpret_cast<int*>(angular_stats_.data() + 1), angular_stats_.data());
    if (xl_) xl_->force(x, f, true, stat_int(5, 0), stat_double(4));
    if (have_wall_)
      check(mhip_periphery_force(&wall_, n_, x, radius_.data(), f, 1, stat_int(7, 0), stat_double(6), nullptr));
    if (active_) active_->force(x, f, true, stat_int(7, 1));
    return f;
  }
  /// U_ext = M F + U_brown (+ u_hydro) into u_ext() [n][6] (the counters advance); returns it for the caller to add to
  double* external_velocity() {
    check(mhip_drag_velocity(n_, mob_t_.data(), force_.data(), u_ext_.data(), nullptr));
    compute_brownian_velocity(n_, keys_.data(), counters_.data(), kt_, dt_, mob_t_.data(), u_ext_.data());
    if (hydro_) {
      if (step_index_ % update_every_ == 0) {
        const double *x = center_.data(), *a = radius_.data();
        hydro_->velocity(hydro_kind_, viscosity_, n_, x, a, force_.data(), u_hydro_.data());
        if (hydro_periphery_)
          hydro_periphery_->correct(*hydro_, hydro_kind_, n_, x, a, force_.data(), u_hydro_.data(), 3, skip_same_index_);
      }
      Hydrodynamics::add_velocity(n_, u_hydro_.data(), u_ext_.data(), 6);
    }
    return u_ext_.data();
  }
  /// contacts -> operator (built after a rebuild, otherwise refreshed) -> q = sep + dt D^T U_ext (NgpHP1.cpp:1488-1531)
  /// -> BBPGD from lambda = 0 -> U = U_ext + M D lambda -> Euler update
  /// Hertz mode: U = U_ext (the contact force is inside it) -> Euler update; max_overlap is read with the springs' two
  StepStats resolve(bool integrate = true) {
    StepStats st;
    st.rebuilt = rebuilt_;
    if (!sphere_contacts_) {  // U = U_ext: the segment contacts are inside it
      st.converged = true;
      check(mhip_deep_copy(6 * n_, vel_.data(), u_ext_.data(), nullptr));
      integrate_and_read(integrate, st);
      return st;
    }
    if (hertz_) {
      if (!have_contact_force_) throw std::logic_error("SphereChainStepper: resolve() before contact_forces()");
      have_contact_force_ = false;
      rebuilt_ = false;
      st.num_contacts = num_lambda_;
      st.converged = true;
      check(mhip_deep_copy(6 * n_, vel_.data(), u_ext_.data(), nullptr));
      integrate_and_read(integrate, st);
      st.max_overlap = max_overlap_.download()[0];
      return st;
    }
    const size_t C = links_.num_links(), cap = C ? C : 1;  // no workspace is null without contacts
    st.num_contacts = C;
    double *sep = workspace(w_sep_, cap), *normal = workspace(w_normal_, 3 * cap), *q = workspace(w_q_, cap),
           *x = workspace(lambda_, cap), *g = workspace(w_g_, cap), *x_tmp = workspace(w_xt_, cap),
           *g_tmp = workspace(w_gt_, cap);
    check(mhip_contact_spheres(C, pairs_.data(), center_.data(), radius_.data(), nullptr, sep, normal, nullptr));
    if (rebuilt_ || !op_)
      op_.reset(new ContactOperator(C, n_, pairs_.data(), normal, nullptr, nullptr, mob_t_.data(), nullptr, dt_,
                                    nullptr, /*priority=*/sep));
    else
      op_->refresh(normal, nullptr, nullptr);
    rebuilt_ = false;
    check(mhip_contact_op_constraint_rate(op_->handle(), u_ext_.data(), q, nullptr));
    check(mhip_axpby(C, 1.0, sep, dt_, q, nullptr));
    num_lambda_ = C;
    // (the hydrodynamic solve: M_h at the current positions; the rows then hold M_h D lambda)
    mhip_solve_result res{};
    if (hydro_solve_) {
      const HydroMobility mobility(*hydro_, hydro_kind_, viscosity_, n_, center_.data(), radius_.data(),
                                   hydro_periphery_.get(), skip_same_index_);
      res = solve_lcp_from_zero(*op_, C, q, cfg_, x, g, x_tmp, g_tmp, &mobility);
    } else {
      res = solve_lcp_from_zero(*op_, C, q, cfg_, x, g, x_tmp, g_tmp);
    }
    st.num_iters = res.num_iters;
    st.residual = res.residual;
    st.converged = res.converged != 0;
    check(mhip_deep_copy(6 * n_, vel_.data(), op_->compute_generalized_velocity(), nullptr));
    check(mhip_axpby(6 * n_, 1.0, u_ext_.data(), 1.0, vel_.data(), nullptr));
    integrate_and_read(integrate, st);
    return st;
  }
  /// the plain chain step
  StepStats step(bool integrate = true) {
    neighbors();
    if (hertz_) contact_forces();
    forces();
    external_velocity();
    return resolve(integrate);
  }

  size_t num_bodies() const { return n_; }
  const DeviceVector& center() const { return center_; }
  const DeviceVector& radius() const { return radius_; }
  /// device pointers: the force [n][3] and U_ext [n][6] the stages work on, and U [n][6] of the last resolve()
  double* force() { return force_.data(); }
  double* u_ext() { return u_ext_.data(); }
  const double* velocity() const { return vel_.data(); }
  /// multipliers of the last step: the first num_lambda() entries (the buffer only ever grows)
  const DeviceVector& lambda() const { return lambda_; }
  size_t num_lambda() const { return num_lambda_; }
  const DeviceArray<int32_t>& pairs() const { return pairs_; }
  const Springs& springs() const { return springs_; }
  size_t step_index() const { return step_index_; }
  /// the optional stages' handles (null before their setter)
  const Crosslinkers* crosslinkers() const { return xl_.get(); }
  const ActiveSprings* active_springs() const { return active_.get(); }
  const AngularSprings* angular_springs() const { return angular_.get(); }
  /// the smallest pivot of set_hydro_periphery's inversion
  double min_pivot() const { return min_pivot_; }

 private:
  /// A candidate list of the crosslinkers: bounding spheres of one reach, both orientations, sources and targets as
  /// byte masks over the searched points, rebuilt by the displacement rule (buffer = skin); the rows as a CSR
  struct CandidateSearch {
    CandidateSearch(const std::vector<unsigned char>& sources, const std::vector<unsigned char>& targets, double r,
                    double skin)
        : n(sources.size()), reach(std::vector<double>(n, r)) {
      DeviceArray<unsigned char> s(sources), t(targets);
      links.set_search_kind(MHIP_SEARCH_SPHERES).set_enforce_source_target_symmetry(true).set_search_buffer(skin);
      links.acts_on(n, s.data(), targets.empty() ? nullptr : t.data()).concretize();
      check(mhip_stream_synchronize(nullptr));  // the masks are copied; the two uploads go out of scope here
    }
    /// true when the list was rebuilt: row_ptr / col / entries are new
    bool update(const double* points) {
      if (!links.generate(n, nullptr, points, reach.data())) return false;
      entries = links.rows_into(row_ptr, col);
      return true;
    }
    size_t n, entries = 0;
    DeviceVector reach;
    DeviceArray<int32_t> row_ptr, col;
    mesh::GenNeighborLinks links;
  };
  /// candidate lists (the beads' own; with periphery sites the one over beads followed by sites, the beads' rows copied
  /// in every step, the sites' columns offset by n) -> one KMC step at the positions of the start of the step
  void crosslinker_kmc() {
    const double* x = center_.data();
    if (xl_search_->update(x))
      xl_->set_candidates(xl_search_->row_ptr.data(), xl_search_->col.data(), xl_search_->entries, ids_.data());
    if (site_search_) {
      check(mhip_deep_copy(3 * n_, site_all_.data(), x, nullptr));
      if (site_search_->update(site_all_.data()))
        xl_->set_periphery_candidates(site_search_->row_ptr.data(), site_search_->col.data(), site_search_->entries,
                                      static_cast<int32_t>(n_));
    }
    xl_->kmc_step(x, dt_, xl_keys_.data(), xl_counters_.data(), stat_int(3, 0), stat_int(5, 1));
  }
  /// the statistics array of the optional force terms, in the layout of DESIGN.md 5h: 9 doubles, the int32 entries two
  /// to a slot; zeroed by forces(), downloaded once by resolve()
  void use_stats() {
    if (stats_.size() == 0) stats_ = DeviceVector(9);
  }
  double* stat_double(size_t slot) { return stats_.data() + slot; }
  int* stat_int(size_t slot, size_t lane) { return reinterpret_cast<int*>(stats_.data()) + 2 * slot + lane; }
  /// the end of resolve(): Euler update, the active timers, and the step's blocking reads
  void integrate_and_read(bool integrate, StepStats& st) {
    if (integrate) {
      check(mhip_integrate_euler(n_, dt_, vel_.data(), center_.data(), nullptr, nullptr));
      if (active_) active_->advance(dt_);
    }
    st.max_spring_length = springs_.max_length();  // these reads wait for the step
    st.springs_overstretched = springs_.overstretched();
    if (stats_.size()) {
      const std::vector<double> d = stats_.download();
      int i[18];
      std::memcpy(i, d.data(), sizeof i);
      st.crosslinker_binds = i[6];
      st.crosslinker_unbinds = i[7];
      st.max_crosslinker_length = d[4];
      st.crosslinkers_overstretched = i[10];
      st.crosslinker_periphery_bound = i[11];
      st.max_periphery_overlap = d[6];
      st.periphery_colliding = i[14];
      st.active_springs = i[15];
      st.active_switches_on = i[16];
      st.active_switches_off = i[17];
    }
    if (angular_) {
      const std::vector<double> a = angular_stats_.download();
      st.max_angle_deviation = a[0];
      std::memcpy(&st.angular_degenerate, &a[1], sizeof(int));
    }
    if (backbone_) {
      const std::vector<std::uint64_t> b = backbone_stats_.download();
      std::memcpy(&st.max_segment_overlap, &b[0], sizeof(double));
      st.segment_contacts = static_cast<size_t>(b[1]);
      st.num_segment_pairs = backbone_->fields().num_pairs;
      st.segment_list_rebuilt = segment_list_rebuilt_;
    }
    ++step_index_;
  }
  size_t n_;
  double dt_, kt_;
  convex::PGDConfig<double> cfg_;
  DeviceVector center_, radius_, mob_t_, aabb_, force_, u_ext_, vel_, lambda_;
  DeviceVector w_sep_, w_normal_, w_q_, w_g_, w_xt_, w_gt_;  // per-step workspaces (grow-only)
  DeviceArray<std::uint64_t> keys_, counters_;
  Springs springs_;
  size_t num_lambda_ = 0, step_index_ = 0;
  bool rebuilt_ = false;
  // the Hertzian contact (set_hertz_contact): material, the device word of max_overlap, the springs' own term
  bool hertz_ = false, have_contact_force_ = false;
  linkers::HertzMaterial material_;
  DeviceVector max_overlap_, spring_term_;
  DeviceArray<int32_t> pairs_;
  mesh::GenNeighborLinks links_;
  std::unique_ptr<ContactOperator> op_;
  // the optional stages (their setters)
  DeviceVector stats_;  // the statistics array of crosslinkers, periphery and active springs
  std::unique_ptr<Crosslinkers> xl_;
  std::unique_ptr<CandidateSearch> xl_search_, site_search_;
  DeviceArray<std::uint64_t> xl_keys_, xl_counters_;
  DeviceArray<std::int64_t> ids_;
  std::vector<unsigned char> xl_sources_;  // bytes [n]: the beads that carry a crosslinker
  double xl_skin_ = 0.0;
  DeviceVector site_all_;  // [n + P][3]: the beads' centres followed by the periphery sites
  bool have_wall_ = false;
  mhip_periphery wall_{};
  std::unique_ptr<ActiveSprings> active_;
  std::unique_ptr<AngularSprings> angular_;
  DeviceVector angular_stats_;
  std::unique_ptr<Hydrodynamics> hydro_;
  std::unique_ptr<HydroPeriphery> hydro_periphery_;
  int hydro_kind_ = MHIP_HYDRO_RPYC;
  double viscosity_ = 0.0, min_pivot_ = 0.0;
  size_t update_every_ = 1;
  bool skip_same_index_ = false;
  bool hydro_solve_ = false;  // set_hydrodynamic_solve
  DeviceVector u_hydro_;  // [n][3]: the stored hydrodynamic velocity
  // the backbone segment contacts (set_backbone_collision) and whether the spheres collide at all (set_sphere_contacts)
  std::unique_ptr<SegmentContacts> backbone_;
  DeviceArray<std::uint64_t> backbone_stats_;  // (bits of the max overlap, linkers in the force branch)
  bool segment_list_rebuilt_ = false, sphere_contacts_ = true;
};

/// Centerline-twist elastic filaments (mhip_filaments_*), stepped in the reference's order: the state lives in the
/// library handle, fields() hands out its device pointers (those of the edge state change places at every step).
/// set_contacts adds the frictional Hertzian contacts between their segments (mhip_filament_contacts_*);
/// set_inertial gives the nodes mass (mundy_hip_filament_inertial.h: the Newmark step of CollidingSperm.cpp and
/// CollidingFrictionalSperm.cpp), set_contact_law chooses the frictionless Hertz law, equilibrate is the stiffness ramp.
class FilamentStepper {
 public:
  /// host arrays: node_ptr [F + 1]; center [N][3], twist [N], edge_orientation [N][4] (w, x, y, z; by left node: the
  /// initial triad of :1057-1068 is the caller's), radius [N], rest_curvature [N][3], arclength [N]; phase [F] or empty
  FilamentStepper(const std::vector<int32_t>& node_ptr, const std::vector<double>& center,
                  const std::vector<double>& twist, const std::vector<double>& edge_orientation,
                  const std::vector<double>& radius, const std::vector<double>& rest_curvature,
                  const std::vector<double>& arclength, const std::vector<double>& phase,
                  const mhip_filament_params& params)
      : node_ptr_(node_ptr), monolayer_(params.monolayer), youngs_modulus_(params.youngs_modulus), stats_(5) {
    if (node_ptr.empty()) throw std::invalid_argument("FilamentStepper: node_ptr is empty");
    const size_t f = node_ptr.size() - 1, n = static_cast<size_t>(node_ptr.back() < 0 ? 0 : node_ptr.back());
    if (center.size() != 3 * n || twist.size() != n || edge_orientation.size() != 4 * n || radius.size() != n ||
        rest_curvature.size() != 3 * n || arclength.size() != n || !(phase.empty() || phase.size() == f))
      throw std::invalid_argument("FilamentStepper: array sizes do not match node_ptr");
    check(mhip_filaments_create(&h_, f, node_ptr.data(), radius.data(), rest_curvature.data(), arclength.data(),
                                phase.empty() ? nullptr : phase.data(), &params, nullptr));
    try {
      DeviceVector c(center), t(twist), q(edge_orientation);
      check(mhip_filaments_set_state(h_, c.data(), t.data(), q.data()));
      check(mhip_stream_synchronize(nullptr));  // the three uploads go out of scope here
    } catch (...) {
      mhip_filaments_destroy(h_);
      throw;
    }
  }
  FilamentStepper(const FilamentStepper&) = delete;
  FilamentStepper& operator=(const FilamentStepper&) = delete;
  ~FilamentStepper() {
    mhip_filament_contacts_destroy(contacts_);
    mhip_filaments_destroy(h_);
  }

  /// contacts between the segments from the next step on; segment_radius [N] or empty = the left node's radius;
  /// params.monolayer is set to the filaments' flag
  void set_contacts(mhip_filament_contact_params params, const std::vector<double>& segment_radius = {}) {
    if (!segment_radius.empty() && segment_radius.size() != static_cast<size_t>(node_ptr_.back()))
      throw std::invalid_argument("FilamentStepper: segment_radius does not have one entry per node");
    params.monolayer = monolayer_;
    mhip_filament_contacts_t c = nullptr;
    check(mhip_filament_contacts_create(&c, h_, node_ptr_.data(), segment_radius.empty() ? nullptr : segment_radius.data(),
                                        &params, nullptr));
    mhip_filament_contacts_destroy(contacts_);
    contacts_ = c;
  }

  /// nodes with mass from the next step on (call before the first step: mhip_filaments_set_state has zeroed the
  /// accelerations only if the handle was inertial then, and this call zeroes them too); fixed_filament [F] or empty
  void set_inertial(const mhip_filament_inertial_params& params, const std::vector<unsigned char>& fixed_filament = {}) {
    if (!fixed_filament.empty() && fixed_filament.size() + 1 != node_ptr_.size())
      throw std::invalid_argument("FilamentStepper: fixed_filament does not have one entry per filament");
    check(mhip_filaments_set_inertial(h_, &params, fixed_filament.empty() ? nullptr : fixed_filament.data()));
    inertial_ = true;
  }
  /// MHIP_FILAMENT_CONTACT_FRICTIONAL (the default) or MHIP_FILAMENT_CONTACT_HERTZ; after set_contacts
  void set_contact_law(int law) {
    if (!contacts_) throw std::logic_error("FilamentStepper: set_contact_law before set_contacts");
    check(mhip_filament_contacts_set_law(contacts_, law));
    law_ = law;
  }

  /// The stiffness ramp of CollidingFrictionalSperm.cpp:1781-1865: E = relaxed; while E < the stepper's modulus:
  /// inertial steps without contacts until the kinetic energy is <= threshold (at least one per level), then
  /// E *= growth.  The step index is not advanced (a wave stays frozen).  poll_every: the kinetic energy is read once
  /// per poll_every steps (1: the reference's loop).  More than max_steps steps in all: std::runtime_error.  On return
  /// the modulus is the stepper's own again.  -> the steps per level
  std::vector<size_t> equilibrate(double dt, double relaxed_youngs_modulus, double threshold = 1e-6, double growth = 1.1,
                                  size_t poll_every = 1, size_t max_steps = 1000000) {
    if (!inertial_) throw std::logic_error("FilamentStepper: equilibrate before set_inertial");
    if (!(relaxed_youngs_modulus > 0.0) || !(growth > 1.0) || poll_every < 1)
      throw std::invalid_argument("FilamentStepper: equilibrate needs relaxed_youngs_modulus > 0, growth > 1, poll_every >= 1");
    struct Restore {
      FilamentStepper* s;
      ~Restore() { mhip_filaments_set_youngs_modulus(s->h_, s->youngs_modulus_); }
    } restore{this};
    const double time = static_cast<double>(step_index_) * dt;
    std::vector<size_t> levels;
    size_t total = 0;
    for (double E = relaxed_youngs_modulus; E < youngs_modulus_; E *= growth) {
      check(mhip_filaments_set_youngs_modulus(h_, E));
      size_t count = 0;
      double energy = std::numeric_limits<double>::infinity();
      while (energy > threshold) {
        if (total + poll_every > max_steps) throw std::runtime_error("FilamentStepper: equilibrate exceeded max_steps");
        for (size_t k = 0; k < poll_every; ++k) {
          check(mhip_filaments_predict(h_, dt));
          check(mhip_filaments_force(h_, time, nullptr, stats_.data()));
          check(mhip_filaments_correct(h_, dt, stats_.data() + 4));
        }
        count += poll_every;
        total += poll_every;
        energy = stats_.download()[4];
      }
      levels.push_back(count);
    }
    return levels;
  }

  /// advance -> forces at x(t + dt), time = step index * dt as the reference counts it (:1115) -> velocities;
  /// external_force [device, N x 3, or null] is added first.  With contacts (:2013-2021): save_velocity -> advance ->
  /// update -> contact force with external_force -> forces with the contacts' node forces -> velocities.
  /// After set_inertial: save_velocity (frictional law only) -> predict -> update -> contact force -> forces -> correct.
  StepStats step(double dt, const double* external_force = nullptr) {
    StepStats st;
    if (contacts_ && law_ == MHIP_FILAMENT_CONTACT_FRICTIONAL) check(mhip_filament_contacts_save_velocity(contacts_));
    if (inertial_) check(mhip_filaments_predict(h_, dt));
    else check(mhip_filaments_advance(h_, dt));
    if (contacts_) {
      int rebuilt = 0;
      check(mhip_filament_contacts_update(contacts_, &rebuilt));
      check(mhip_filament_contacts_force(contacts_, dt, external_force, stats_.data() + 2));
      const mhip_filament_contact_fields cf = contact_fields();
      external_force = cf.node_force;
      st.rebuilt = rebuilt != 0;
      st.num_contacts = cf.num_pairs;
    }
    check(mhip_filaments_force(h_, static_cast<double>(step_index_) * dt, external_force, stats_.data()));
    if (inertial_) check(mhip_filaments_correct(h_, dt, stats_.data() + 4));
    else check(mhip_filaments_velocity(h_));
    ++step_index_;
    const auto s = stats_.download();  // the one host read of the step
    st.max_stretch = s[0];
    st.max_curvature_deviation = s[1];
    if (inertial_) st.kinetic_energy = s[4];
    if (contacts_) {
      st.max_overlap = s[2];
      unsigned long long sliding = 0;
      std::memcpy(&sliding, &s[3], sizeof sliding);
      st.num_sliding = static_cast<size_t>(sliding);
    }
    return st;
  }
  mhip_filament_contact_fields contact_fields() const {
    mhip_filament_contact_fields f{};
    if (contacts_) check(mhip_filament_contacts_get(contacts_, &f));
    return f;
  }
  mhip_filament_fields fields() const {
    mhip_filament_fields f{};
    check(mhip_filaments_get(h_, &f));
    return f;
  }
  mhip_filament_inertial_fields inertial_fields() const {
    mhip_filament_inertial_fields f{};
    check(mhip_filaments_get_inertial(h_, &f));
    return f;
  }
  size_t step_index() const { return step_index_; }

 private:
  mhip_filaments_t h_ = nullptr;
  mhip_filament_contacts_t contacts_ = nullptr;
  std::vector<int32_t> node_ptr_;
  int monolayer_ = 0, law_ = MHIP_FILAMENT_CONTACT_FRICTIONAL;
  bool inertial_ = false;
  double youngs_modulus_ = 0.0;
  DeviceVector stats_;  // (max_stretch, max_curvature_deviation, max_overlap, the bits of num_sliding, kinetic energy)
  size_t step_index_ = 0;
};

}  // namespace mech
}  // namespace mundy_hip
