// filament.hip -- centerline-twist (discrete Kirchhoff rod) elastic filaments: the rod forces of the reference's sperm
// apps (scrap/parameter_interface/alens/tests/performance_tests/CollidingOverdampedFrictionalSperm.cpp; the same text in
// CollidingFrictionalSperm.cpp, CollidingSperm.cpp, NonInteractingSperm.cpp and scrap/Sperm.cpp):
//   edge pass    compute_edge_information, :1171-1257                 one edge per lane
//   node pass    compute_node_curvature_and_rotation_gradient :1259-1318, propagate_rest_curvature :1095-1169,
//                compute_internal_force_and_twist_torque :1320-1509   one node per lane, a tile of nodes per workgroup
//   velocity     compute_generalized_velocity, :1733-1777             one node per lane
//   advance      disable_twist / apply_monolayer / rotate_field_states / update_generalized_position /
//                zero_out_transient_node_fields, :1832-1862, :1080-1093, :1779-1811, in the order of the loop :1999-2010
// Node i of N; edge i joins nodes i and i + 1 of one filament (the slot of a filament's last node is unused); element i
// is (i - 1, i, i + 1) around an interior node.  The reference scatters element and edge terms into the nodes with
// `omp atomic`; here every node GATHERS its terms in one fixed order and there is no atomic on a force:
//   external force -> element i - 1 (as its right node) -> element i (centre) -> element i + 1 (as its left node)
//   -> edge i - 1 -> edge i;  twist torque: element i, then element i + 1.
// Node pass, per tile of kBlock nodes [s, s + kBlock): the edge records (t, b, l, q) of the edges s - 2 .. s + kBlock are
// staged once in LDS, with 1 / l (element i - 1 of the tile's first node reaches back to edge s - 2), then the rotated torque of the
// elements s - 1 .. s + kBlock is formed once each into LDS, then every node adds up its six terms from the LDS image.
// Each element's torque is one function of the same inputs wherever it is evaluated, so the result does not depend on
// the tile a node falls in.  All streaming: HBM bound (byte counts: DESIGN.md 5j).
#include "mhip_internal.hpp"
#include "force_device.hpp"
#include "geom_device.hpp"
#include "../../include/mundy_hip_filament_inertial.h"

#include <cmath>
#include <vector>

namespace mhip {

// what a node has around it inside its filament (built on the host at create)
constexpr unsigned kHasL = 1u;   // edge i - 1 exists: i is not the first node
constexpr unsigned kHasR = 2u;   // edge i exists: i is not the last node
constexpr unsigned kElemL = 4u;  // element i - 1 exists
constexpr unsigned kElemR = 8u;  // element i + 1 exists
constexpr unsigned kInterior = kHasL | kHasR;  // element i exists

constexpr int kTile = kBlock;
constexpr int kTileEdges = kTile + 3;  // edges s - 2 .. s + kTile
constexpr int kTileElems = kTile + 2;  // elements s - 1 .. s + kTile

struct FilamentD {  // mhip_filament_params as the kernels use it; shear = 0.5 E / (1 + nu) (:1413) and inv_l0 = 1 / l0
  double E, l0, A, k, shear, inv_l0;  // (:1414) are formed once on the host: the same IEEE operations, the same bits
};

__device__ inline void store4q(double* p, size_t i, Quat q) {
  *reinterpret_cast<double2*>(p + 4 * i) = make_double2(q.w, q.x);
  *reinterpret_cast<double2*>(p + 4 * i + 2) = make_double2(q.y, q.z);
}

struct EdgeRecord {
  V3 t, b;
  double l;
  Quat q;
};

// :1223-1240.  v /= s divides componentwise; v / s multiplies by 1 / s (mundy_math/impl/VectorImpl.hpp:240-267).
// quat_from_parallel_transport: mundy_math/Quaternion.hpp:1489-1506.  No renormalisation, as in the reference.
__device__ inline EdgeRecord edge_update(V3 x0, V3 x1, double twist, V3 t_old, Quat q_old) {
  EdgeRecord e;
  const V3 d = x1 - x0;
  e.l = sqrt(dot(d, d));
  e.t = V3{d.x / e.l, d.y / e.l, d.z / e.l};
  const V3 c = cross(t_old, e.t);
  const double tt = dot(t_old, e.t);
  const double ib = 1.0 / (1.0 + tt);
  e.b = V3{(2.0 * c.x) * ib, (2.0 * c.y) * ib, (2.0 * c.z) * ib};
  double sh, ch;
  det_sincos(0.5 * twist, sh, ch);
  const Quat rot_twist{ch, sh * t_old.x, sh * t_old.y, sh * t_old.z};
  const double w = sqrt(0.5 * (1.0 + tt));
  const double iw = 1.0 / w;
  const Quat rot_pt{w, (0.5 * c.x) * iw, (0.5 * c.y) * iw, (0.5 * c.z) * iw};
  e.q = qmul(qmul(rot_pt, rot_twist), q_old);
  return e;
}

__global__ void __launch_bounds__(kBlock)
    k_filament_edges(size_t n, const uint8_t* __restrict__ flag, const double* __restrict__ x,
                     const double* __restrict__ twist, const double* __restrict__ t_old,
                     const double* __restrict__ q_old, double* __restrict__ t_new, double* __restrict__ q_new,
                     double* __restrict__ len, double* __restrict__ binormal) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (!(flag[i] & kHasR)) continue;  // i + 1 < n from here on
    // the old state is read once and not again before two more steps have overwritten it
    const V3 to{__builtin_nontemporal_load(t_old + 3 * i), __builtin_nontemporal_load(t_old + 3 * i + 1),
                __builtin_nontemporal_load(t_old + 3 * i + 2)};
    const Quat qo{__builtin_nontemporal_load(q_old + 4 * i), __builtin_nontemporal_load(q_old + 4 * i + 1),
                  __builtin_nontemporal_load(q_old + 4 * i + 2), __builtin_nontemporal_load(q_old + 4 * i + 3)};
    const EdgeRecord e = edge_update(load3(x, i), load3(x, i + 1), twist[i], to, qo);
    store3(t_new, i, e.t);
    store3(binormal, i, e.b);
    len[i] = e.l;
    store4q(q_new, i, e.q);
  }
}

// set_state: tangent and length from the centres (:1053-1055), for both copies of the state
__global__ void __launch_bounds__(kBlock)
    k_filament_init_edges(size_t n, const uint8_t* __restrict__ flag, const double* __restrict__ x,
                          double* __restrict__ t_a, double* __restrict__ len_a, double* __restrict__ t_b,
                          double* __restrict__ len_b) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (!(flag[i] & kHasR)) continue;
    const V3 d = load3(x, i + 1) - load3(x, i);
    const double l = sqrt(dot(d, d));
    const V3 t{d.x / l, d.y / l, d.z / l};
    store3(t_a, i, t);
    store3(t_b, i, t);
    len_a[i] = l;
    len_b[i] = l;
  }
}

// ---- element and edge terms (:1411-1458, :1490-1492) ---------------------------------------------------------------
struct ElementTorque {
  V3 kappa, dk, m;
};
// curvature of the element between the edge orientations ql (edge i - 1) and qr (edge i), the Lagrangian torque of its
// deviation from the rest curvature, rotated to the lab frame
__device__ inline ElementTorque element_torque(const FilamentD& P, Quat ql, Quat qr, V3 rest, double r) {
  ElementTorque e;
  const Quat g = qmul(Quat{ql.w, -ql.x, -ql.y, -ql.z}, qr);                       // :1315
  e.kappa = V3{2.0 * g.x, 2.0 * g.y, 2.0 * g.z};                                  // :1316
  e.dk = e.kappa - rest;                                                          // :1411
  const double inertia = 0.25 * M_PI * r * r * r * r;
  const V3 bt{-P.inv_l0 * P.E * inertia * e.dk.x, -P.inv_l0 * P.E * inertia * e.dk.y,
              -P.inv_l0 * 2 * P.shear * inertia * e.dk.z};                        // :1415-1418
  const V3 gv{g.x, g.y, g.z};
  e.m = qrot(ql, g.w * bt + cross(gv, bt));                                       // :1421-1423
  return e;
}
// tmp_force_ip1 (:1426-1430), on the element's right node; t, b and il = 1.0 / l of its right edge.  `- b` sits outside
// the 0.5 (t.m)(...) factor, as the reference writes it.
__device__ inline V3 force_right(V3 m, V3 t, V3 b, double il) {
  const V3 inner = (cross(m, t) + (0.5 * dot(t, m)) * (dot(t, b) * t)) - b;
  return il * inner;
}
// tmp_force_im1 (:1431-1435), on the element's left node; t, b, il of its left edge
__device__ inline V3 force_left(V3 m, V3 t, V3 b, double il) {
  const V3 inner = cross(m, t) + (0.5 * dot(t, m)) * (dot(t, b) * t - b);
  return il * inner;
}
// right_node_force (:1490-1492): r is the radius of the edge's right node
__device__ inline V3 stretch_right(const FilamentD& P, V3 t, double l, double r) {
  const double k = P.E * M_PI * r * r / P.l0;
  return (-k * (l - P.l0)) * t;
}

struct EdgeTile {
  // t (0-2), b (3-5), l (6), q (7-10), 1.0 / l (11: four terms divide by it); one row per component: lane k reads word k
  double v[12][kTileEdges];
  __device__ V3 t(int k) const { return {v[0][k], v[1][k], v[2][k]}; }
  __device__ V3 b(int k) const { return {v[3][k], v[4][k], v[5][k]}; }
  __device__ double l(int k) const { return v[6][k]; }
  __device__ double il(int k) const { return v[11][k]; }
  __device__ Quat q(int k) const { return {v[7][k], v[8][k], v[9][k], v[10][k]}; }
};

// stats[0]: bits of the largest |l - l0| / l0 over the edges; stats[1]: of the largest |kappa - kappa_rest| component
// over the elements (atomic max on the bits of non-negative doubles: order independent)
template <bool WAVE, bool EXTERNAL>
__global__ void __launch_bounds__(kBlock)
    k_filament_nodes(long long n, long long tiles, FilamentD P, double wt, const uint8_t* __restrict__ flag,
                     const int32_t* __restrict__ fid, const double* __restrict__ phase,
                     const double* __restrict__ radius, const double* __restrict__ rest,
                     const double* __restrict__ arclength, const double* __restrict__ et,
                     const double* __restrict__ eb, const double* __restrict__ el, const double* __restrict__ eq,
                     const double* __restrict__ external, double* __restrict__ force, double* __restrict__ torque,
                     double* __restrict__ curvature, unsigned long long* __restrict__ stats) {
  __shared__ EdgeTile E;
  __shared__ double M[3][kTileElems];
  double smax = 0.0, kmax = 0.0;
  const int tid = threadIdx.x;
  for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const long long s = tile * kTile;
    for (int k = tid; k < kTileEdges; k += kBlock) {  // slot k = edge s - 2 + k
      const long long e = s - 2 + k;
      if (e >= 0 && e < n && (flag[e] & kHasR)) {
        const V3 t = load3(et, e), b = load3(eb, e);
        const Quat q = load4q(eq, e);
        E.v[0][k] = t.x, E.v[1][k] = t.y, E.v[2][k] = t.z;
        E.v[3][k] = b.x, E.v[4][k] = b.y, E.v[5][k] = b.z;
        const double l = el[e];
        E.v[6][k] = l;
        E.v[11][k] = 1.0 / l;
        E.v[7][k] = q.w, E.v[8][k] = q.x, E.v[9][k] = q.y, E.v[10][k] = q.z;
      }
    }
    __syncthreads();
    for (int k = tid; k < kTileElems; k += kBlock) {  // slot k = element s - 1 + k: edges in the slots k and k + 1
      const long long j = s - 1 + k;
      if (j >= 0 && j < n && (flag[j] & kInterior) == kInterior) {
        V3 kr = load3(rest, j);
        if (WAVE) {  // :1166-1167; wt = temporal frequency * time
          double sn, cs;
          det_sincos(P.k * arclength[j] + wt + phase[fid[j]], sn, cs);
          kr.x = P.A * sn;
        }
        const ElementTorque e = element_torque(P, E.q(k), E.q(k + 1), kr, radius[j]);
        M[0][k] = e.m.x, M[1][k] = e.m.y, M[2][k] = e.m.z;
        if (k >= 1 && k <= kTile) {  // a node of this tile
          store3(curvature, j, e.kappa);
          const double a = fabs(e.dk.x), b = fabs(e.dk.y), c = fabs(e.dk.z);
          const double d = a > b ? (a > c ? a : c) : (b > c ? b : c);
          kmax = d > kmax ? d : kmax;
        }
      }
    }
    __syncthreads();
    const long long i = s + tid;
    if (i < n) {
      const unsigned fl = flag[i];
      // edge i - 1: slot tid + 1, edge i: slot tid + 2; element i - 1: slot tid, i: tid + 1, i + 1: tid + 2
      const int eL = tid + 1, eR = tid + 2;
      V3 f = EXTERNAL ? load3(external, i) : V3{0.0, 0.0, 0.0};
      double tq = 0.0;
      if (fl & kElemL) f = f + force_right(V3{M[0][tid], M[1][tid], M[2][tid]}, E.t(eL), E.b(eL), E.il(eL));
      if ((fl & kInterior) == kInterior) {
        const V3 m{M[0][tid + 1], M[1][tid + 1], M[2][tid + 1]};
        const V3 fr = force_right(m, E.t(eR), E.b(eR), E.il(eR));
        const V3 fm = force_left(m, E.t(eL), E.b(eL), E.il(eL));
        f = f - (fr + fm);                                                        // :1448-1452
        tq = tq + dot(E.t(eR), m);                                                // :1438
      }
      if (fl & kElemR) {
        const V3 m{M[0][tid + 2], M[1][tid + 2], M[2][tid + 2]};
        f = f + force_left(m, E.t(eR), E.b(eR), E.il(eR));
        tq = tq - dot(E.t(eR), m);                                                // :1440
      }
      if (fl & kHasL) f = f + stretch_right(P, E.t(eL), E.l(eL), radius[i]);
      if (fl & kHasR) {
        f = f - stretch_right(P, E.t(eR), E.l(eR), radius[i + 1]);
        const double st = fabs(E.l(eR) - P.l0) / P.l0;
        smax = st > smax ? st : smax;
      }
      store3(force, i, f);
      torque[i] = tq;
    }
    __syncthreads();  // the next tile overwrites the LDS image
  }
  block_stat_max(smax, stats);
  __syncthreads();  // block_stat_max's LDS slots are used again
  block_stat_max(kmax, stats + 1);
}

// :1772-1775; c6 = 1 / (6 pi eta), c8 = 1 / (8 pi eta)
__global__ void __launch_bounds__(kBlock)
    k_filament_velocity(size_t n, double c6, double c8, const double* __restrict__ radius,
                        const double* __restrict__ force, const double* __restrict__ torque, double* __restrict__ vel,
                        double* __restrict__ twist_vel) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const double inv_r = 1.0 / radius[i];
    const double inv_r3 = inv_r * inv_r * inv_r;
    store3(vel, i, (c6 * inv_r) * load3(force, i));
    twist_vel[i] = (c8 * inv_r3) * torque[i];
  }
}

// the head of the time loop (:1999-2010) for one node; the old <-> new swap of the edge state is a swap of pointers on
// the host
template <bool NO_TWIST, bool MONOLAYER>
__global__ void __launch_bounds__(kBlock)
    k_filament_advance(size_t n, double dt, double* __restrict__ x, double* __restrict__ twist, double* __restrict__ vel,
                       double* __restrict__ twist_vel, double* __restrict__ force, double* __restrict__ torque) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    V3 c = load3(x, i), v = load3(vel, i);
    double tw = twist[i], tv = twist_vel[i];
    if (NO_TWIST) tw = 0.0, tv = 0.0;      // :1836-1837
    if (MONOLAYER) c.x = 0.0, v.x = 0.0;   // :1859-1860
    store3(x, i, c + dt * v);              // :1804-1809
    twist[i] = tw + dt * tv;
    store3(vel, i, V3{0.0, 0.0, 0.0});     // :1087-1090
    store3(force, i, V3{0.0, 0.0, 0.0});
    twist_vel[i] = 0.0;
    torque[i] = 0.0;
  }
}

// ---- inertial nodes: the Newmark step of CollidingSperm.cpp and CollidingFrictionalSperm.cpp ---------------------------
// (include/mundy_hip_filament_inertial.h restates both kernels operation for operation.)
//   predict   disable_twist :1699-1706 / apply_monolayer :1708-1737 / rotate_field_states / update_generalized_position
//             :968-1018, in the order of the loop :1902-1921                                       one node per lane
//   correct   update_generalized_position_velocity_and_acceleration :1616-1672 and, fused, the node's term of
//             global_kinetic_energy :1739-1779                                                     one node per lane
// zero_out_transient_node_fields (:955-966) is not restated: the node pass writes force and torque from +0.0 or the
// external force and the corrector overwrites velocity and acceleration, so no zeroed value is ever read.  The
// reference's StateN / StateNP1 copies of velocity and acceleration collapse into one: both kernels are node-local and
// read a node's old values before they overwrite them.  All streaming (byte counts: DESIGN.md 5v).
struct NewmarkD {  // formed once on the host: the same IEEE operations, the same bits
  double c1;      // (1.0 - gamma) dt, :1647
  double c2;      // (dt dt) beta, :1665
  double c3;      // dt gamma, :1669
  double density, E, ct, cr;
};

template <bool NO_TWIST, bool MONOLAYER>
__global__ void __launch_bounds__(kBlock)
    k_filament_predict(size_t n, double dt, double coeff, double* __restrict__ x, double* __restrict__ twist,
                       double* __restrict__ vel, double* __restrict__ twist_vel, double* __restrict__ acc,
                       double* __restrict__ twist_acc) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    V3 c = load3(x, i), v = load3(vel, i), a = load3(acc, i);
    double tw = 0.0, tv = 0.0, ta = 0.0;
    if (NO_TWIST) {  // :1703-1705: the corrector reads the two zeroed fields
      twist_vel[i] = 0.0;
      twist_acc[i] = 0.0;
    } else {
      tw = twist[i], tv = twist_vel[i], ta = twist_acc[i];
    }
    if (MONOLAYER) {  // :1733-1735
      c.x = 0.0, v.x = 0.0, a.x = 0.0;
      vel[3 * i] = 0.0;
      acc[3 * i] = 0.0;
    }
    store3(x, i, (c + dt * v) + coeff * a);  // :1014
    twist[i] = (tw + dt * tv) + coeff * ta;  // :1015-1016
  }
}

// mass and moment of inertia of the sphere lumped at a node (:1633-1636)
__device__ inline void node_mass(double r, double rho, double& m, double& I) {
  const double r2 = r * r;
  const double r3 = r2 * r;
  m = 4.0 / 3.0 * M_PI * r3 * rho;
  I = 2.0 / 5.0 * m * r2;
}
// :1767-1769
__device__ inline double node_kinetic_energy(double m, double I, V3 v, double w) {
  return 0.5 * m * dot(v, v) + 0.5 * I * w * w;
}
// the lanes' double-double sums -> one pair per workgroup, partials[2 b], partials[2 b + 1]
__device__ inline void store_energy_partial(DD acc, double* __restrict__ partials) {
  __shared__ double scratch[2 * (kBlock / 64)];
  const DD r = block_sum(acc, scratch);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = r.hi;
    partials[2 * blockIdx.x + 1] = r.lo;
  }
}

template <bool CRITICAL, bool FIXED, bool ENERGY>
__global__ void __launch_bounds__(kBlock)
    k_filament_correct(size_t n, NewmarkD P, const double* __restrict__ radius, const uint8_t* __restrict__ fixed,
                       const double* __restrict__ force, const double* __restrict__ torque, double* __restrict__ x,
                       double* __restrict__ twist, double* __restrict__ vel, double* __restrict__ twist_vel,
                       double* __restrict__ acc, double* __restrict__ twist_acc, double* __restrict__ partials) {
  DD sum{0.0, 0.0};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    if (FIXED && fixed[i]) {  // :1652-1656; its term of the energy is +0.0
      store3(vel, i, V3{0.0, 0.0, 0.0});
      store3(acc, i, V3{0.0, 0.0, 0.0});
      twist_vel[i] = 0.0;
      twist_acc[i] = 0.0;
      continue;
    }
    double m, I;
    node_mass(radius[i], P.density, m, I);
    const double ct = CRITICAL ? sqrt(m * P.E) : P.ct;  // :1645-1646; CollidingSperm.cpp:1576-1577
    const double cr = CRITICAL ? ct : P.cr;
    const V3 v = load3(vel, i), a = load3(acc, i);
    const double tv = twist_vel[i], ta = twist_acc[i];
    const V3 pv = v + P.c1 * a;                                     // :1648
    const double ptv = tv + P.c1 * ta;                              // :1649
    const V3 an = (1.0 / m) * (load3(force, i) - ct * v);           // :1658
    const double tan_ = 1.0 / I * (torque[i] - cr * tv);            // :1659-1660
    store3(x, i, load3(x, i) + P.c2 * an);                          // :1666
    twist[i] = twist[i] + P.c2 * tan_;                              // :1667
    const V3 vn = pv + P.c3 * an;                                   // :1670
    const double tvn = ptv + P.c3 * tan_;                           // :1671
    store3(acc, i, an);
    twist_acc[i] = tan_;
    store3(vel, i, vn);
    twist_vel[i] = tvn;
    if (ENERGY) dd_add(sum, node_kinetic_energy(m, I, vn, tvn));
  }
  if (ENERGY) store_energy_partial(sum, partials);
}

// global_kinetic_energy (:1739-1779) from the velocities as they stand: the lanes, the grid and so the partial sums of
// k_filament_correct<.., true>
__global__ void __launch_bounds__(kBlock)
    k_filament_energy(size_t n, double density, const double* __restrict__ radius, const double* __restrict__ vel,
                      const double* __restrict__ twist_vel, double* __restrict__ partials) {
  DD sum{0.0, 0.0};
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    double m, I;
    node_mass(radius[i], density, m, I);
    dd_add(sum, node_kinetic_energy(m, I, load3(vel, i), twist_vel[i]));
  }
  store_energy_partial(sum, partials);
}

// One workgroup: lane t adds the pairs t, t + kBlock, .. in ascending order, the lanes' sums are added as block_sum adds
// them, one rounding.  kBlock pairs per pass: a grid of more than kBlock workgroups (n > kBlock * kBlock nodes) takes
// the loop's second pass.
__global__ void __launch_bounds__(kBlock)
    k_filament_energy_fold(unsigned parts, const double* __restrict__ partials, double* __restrict__ out) {
  __shared__ double scratch[2 * (kBlock / 64)];
  DD sum{0.0, 0.0};
  for (unsigned k = threadIdx.x; k < parts; k += kBlock) dd_add(sum, DD{partials[2 * k], partials[2 * k + 1]});
  const DD r = block_sum(sum, scratch);
  if (threadIdx.x == 0) out[0] = dd_value(r);
}

}  // namespace mhip

using namespace mhip;

struct mhip_filaments {
  size_t n = 0, f = 0;
  mhip_filament_params prm{};
  hipStream_t stream = nullptr;
  bool has_state = false;
  int cur = 0;  // the copy of the edge state that is "new"
  HandleBuffer flag, fid, node_ptr, phase, radius, rest, arclength;
  HandleBuffer center, twist, vel, twist_vel, force, torque, curvature;
  HandleBuffer tangent[2], orient[2], length[2], binormal[2];
  // mundy_hip_filament_inertial.h
  bool inertial = false, any_fixed = false;
  mhip_filament_inertial_params iprm{};
  HandleBuffer acc, twist_acc, fixed, energy_partials;
  std::vector<int32_t> host_node_ptr;  // the per-node flag of the fixed filaments is built from it
};

extern "C" {

int mhip_filaments_create(mhip_filaments_t* handle, size_t num_filaments, const int32_t* node_ptr, const double* radius,
                          const double* rest_curvature, const double* arclength, const double* phase,
                          const mhip_filament_params* params, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = nullptr;
  MHIP_REQUIRE(params != nullptr, MHIP_ERR_INVALID_ARGUMENT, "params is null");
  MHIP_REQUIRE(node_ptr != nullptr, MHIP_ERR_INVALID_ARGUMENT, "node_ptr is null");
  MHIP_REQUIRE(num_filaments < (1ull << 31), MHIP_ERR_INVALID_ARGUMENT, "too many filaments for 32-bit indices");
  const mhip_filament_params& p = *params;
  MHIP_REQUIRE(std::isfinite(p.youngs_modulus) && p.youngs_modulus >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "youngs_modulus must be finite and >= 0, got %g", p.youngs_modulus);
  MHIP_REQUIRE(std::isfinite(p.poisson_ratio) && p.poisson_ratio > -1.0, MHIP_ERR_INVALID_ARGUMENT,
               "poisson_ratio must be finite and > -1, got %g", p.poisson_ratio);
  MHIP_REQUIRE(std::isfinite(p.rest_length) && p.rest_length > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "rest_length must be finite and > 0, got %g", p.rest_length);
  MHIP_REQUIRE(std::isfinite(p.viscosity) && p.viscosity > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "viscosity must be finite and > 0, got %g", p.viscosity);
  MHIP_REQUIRE(std::isfinite(p.wave_amplitude) && std::isfinite(p.wave_number) && std::isfinite(p.wave_frequency),
               MHIP_ERR_INVALID_ARGUMENT, "the wave's amplitude, number and frequency must be finite");
  MHIP_REQUIRE(node_ptr[0] == 0, MHIP_ERR_INVALID_ARGUMENT, "node_ptr[0] must be 0, got %d", node_ptr[0]);
  for (size_t f = 0; f < num_filaments; ++f) {
    MHIP_REQUIRE(node_ptr[f + 1] >= node_ptr[f], MHIP_ERR_INVALID_ARGUMENT,
                 "node_ptr is not monotone at filament %zu: %d after %d", f, node_ptr[f + 1], node_ptr[f]);
    MHIP_REQUIRE(node_ptr[f + 1] - node_ptr[f] >= 2, MHIP_ERR_INVALID_ARGUMENT,
                 "filament %zu has %d node(s): a filament has at least 2", f, node_ptr[f + 1] - node_ptr[f]);
  }
  const size_t n = static_cast<size_t>(node_ptr[num_filaments]);
  MHIP_REQUIRE(n == 0 || (radius && rest_curvature && arclength), MHIP_ERR_INVALID_ARGUMENT,
               "radius / rest_curvature / arclength is null");
  for (size_t i = 0; i < n; ++i) {
    MHIP_REQUIRE(std::isfinite(radius[i]) && radius[i] > 0.0, MHIP_ERR_INVALID_ARGUMENT,
                 "node %zu: radius must be finite and > 0, got %g", i, radius[i]);
    MHIP_REQUIRE(std::isfinite(arclength[i]), MHIP_ERR_INVALID_ARGUMENT, "node %zu: arclength is not finite", i);
  }
  // what every node has around it, and the filament it belongs to
  std::vector<uint8_t> flag(n, 0);
  std::vector<int32_t> fid(n, 0);
  for (size_t f = 0; f < num_filaments; ++f) {
    const int32_t lo = node_ptr[f], hi = node_ptr[f + 1];
    for (int32_t i = lo; i < hi; ++i) {
      unsigned fl = 0;
      if (i > lo) fl |= kHasL;
      if (i + 1 < hi) fl |= kHasR;
      if (i - 1 > lo) fl |= kElemL;      // i - 1 is interior: i - 1 > lo and i - 1 + 1 < hi
      if (i + 2 < hi) fl |= kElemR;      // i + 1 is interior
      flag[i] = static_cast<uint8_t>(fl);
      fid[i] = static_cast<int32_t>(f);
    }
  }
  std::vector<double> zero_phase;
  if (!phase) {
    zero_phase.assign(num_filaments, 0.0);
    phase = zero_phase.data();
  }
  auto h = std::make_unique<mhip_filaments>();
  h->n = n;
  h->f = num_filaments;
  h->prm = p;
  h->host_node_ptr.assign(node_ptr, node_ptr + num_filaments + 1);
  hipStream_t s = as_stream(stream);
  h->stream = s;
  const size_t d = sizeof(double);
  int e = MHIP_SUCCESS;
  if ((e = h->flag.reserve(n + 8)) || (e = h->fid.reserve(n * sizeof(int32_t) + 8)) ||
      (e = h->node_ptr.reserve((num_filaments + 1) * sizeof(int32_t))) || (e = h->phase.reserve(num_filaments * d + 8)) ||
      (e = h->radius.reserve(n * d + 8)) || (e = h->rest.reserve(3 * n * d + 8)) ||
      (e = h->arclength.reserve(n * d + 8)) || (e = h->center.reserve(3 * n * d + 8)) ||
      (e = h->twist.reserve(n * d + 8)) || (e = h->vel.reserve(3 * n * d + 8)) ||
      (e = h->twist_vel.reserve(n * d + 8)) || (e = h->force.reserve(3 * n * d + 8)) ||
      (e = h->torque.reserve(n * d + 8)) || (e = h->curvature.reserve(3 * n * d + 8)))
    return e;
  for (int c = 0; c < 2; ++c)
    if ((e = h->tangent[c].reserve(3 * n * d + 8)) || (e = h->orient[c].reserve(4 * n * d + 8)) ||
        (e = h->length[c].reserve(n * d + 8)) || (e = h->binormal[c].reserve(3 * n * d + 8)))
      return e;
  if ((e = upload(__func__, h->node_ptr, node_ptr, (num_filaments + 1) * sizeof(int32_t), s))) return e;
  if (num_filaments > 0 && (e = upload(__func__, h->phase, phase, num_filaments * d, s))) return e;
  if (n > 0) {
    if ((e = upload(__func__, h->flag, flag.data(), n, s)) ||
        (e = upload(__func__, h->fid, fid.data(), n * sizeof(int32_t), s)) ||
        (e = upload(__func__, h->radius, radius, n * d, s)) ||
        (e = upload(__func__, h->rest, rest_curvature, 3 * n * d, s)) ||
        (e = upload(__func__, h->arclength, arclength, n * d, s)))
      return e;
  }
  // the caller's host arrays (and the two built here) may go as soon as this returns
  if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_filaments_destroy(mhip_filaments_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_filaments_set_state(mhip_filaments_t h, const double* center, const double* twist,
                             const double* edge_orientation) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(h->n == 0 || (center && twist && edge_orientation), MHIP_ERR_INVALID_ARGUMENT,
               "center / twist / edge_orientation is null");
  const size_t n = h->n, d = sizeof(double);
  hipStream_t s = h->stream;
  h->cur = 0;
  h->has_state = true;
  if (n == 0) return MHIP_SUCCESS;
  MHIP_HIP(hipMemcpyAsync(h->center.ptr, center, 3 * n * d, hipMemcpyDeviceToDevice, s));
  MHIP_HIP(hipMemcpyAsync(h->twist.ptr, twist, n * d, hipMemcpyDeviceToDevice, s));
  for (int c = 0; c < 2; ++c) {
    MHIP_HIP(hipMemcpyAsync(h->orient[c].ptr, edge_orientation, 4 * n * d, hipMemcpyDeviceToDevice, s));
    MHIP_HIP(hipMemsetAsync(h->tangent[c].ptr, 0, 3 * n * d, s));  // the unused slots stay +0.0
    MHIP_HIP(hipMemsetAsync(h->length[c].ptr, 0, n * d, s));
    MHIP_HIP(hipMemsetAsync(h->binormal[c].ptr, 0, 3 * n * d, s));
  }
  for (HandleBuffer* b : {&h->vel, &h->force, &h->curvature}) MHIP_HIP(hipMemsetAsync(b->ptr, 0, 3 * n * d, s));
  for (HandleBuffer* b : {&h->twist_vel, &h->torque}) MHIP_HIP(hipMemsetAsync(b->ptr, 0, n * d, s));
  if (h->inertial) {
    MHIP_HIP(hipMemsetAsync(h->acc.ptr, 0, 3 * n * d, s));
    MHIP_HIP(hipMemsetAsync(h->twist_acc.ptr, 0, n * d, s));
  }
  k_filament_init_edges<<<grid_for(n), kBlock, 0, s>>>(n, h->flag.as<uint8_t>(), h->center.as<double>(),
                                                       h->tangent[0].as<double>(), h->length[0].as<double>(),
                                                       h->tangent[1].as<double>(), h->length[1].as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_advance(mhip_filaments_t h, double dt) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_advance before mhip_filaments_set_state");
  h->cur ^= 1;  // rotate_field_states: what was new is old
  if (h->n == 0) return MHIP_SUCCESS;
  dispatch_bools(h->prm.disable_twist != 0, h->prm.monolayer != 0, [&](auto nt, auto ml) {
    k_filament_advance<decltype(nt)::value, decltype(ml)::value><<<grid_for(h->n), kBlock, 0, h->stream>>>(
        h->n, dt, h->center.as<double>(), h->twist.as<double>(), h->vel.as<double>(), h->twist_vel.as<double>(),
        h->force.as<double>(), h->torque.as<double>());
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_edge_pass(mhip_filaments_t h) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_edge_pass before mhip_filaments_set_state");
  const size_t n = h->n;
  if (n == 0) return MHIP_SUCCESS;
  const int cur = h->cur, old = cur ^ 1;
  k_filament_edges<<<grid_for(n), kBlock, 0, h->stream>>>(
      n, h->flag.as<uint8_t>(), h->center.as<double>(), h->twist.as<double>(), h->tangent[old].as<double>(),
      h->orient[old].as<double>(), h->tangent[cur].as<double>(), h->orient[cur].as<double>(),
      h->length[cur].as<double>(), h->binormal[cur].as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_node_pass(mhip_filaments_t h, double time, const double* external_force, double* stats) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(std::isfinite(time), MHIP_ERR_INVALID_ARGUMENT, "time must be finite, got %g", time);
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_node_pass before mhip_filaments_set_state");
  hipStream_t s = h->stream;
  MHIP_HIP(hipMemsetAsync(stats, 0, 2 * sizeof(double), s));  // +0.0: also the answer without edges / elements
  const size_t n = h->n;
  if (n == 0) return MHIP_SUCCESS;
  const int cur = h->cur;
  const mhip_filament_params& p = h->prm;
  const FilamentD P{p.youngs_modulus, p.rest_length, p.wave_amplitude, p.wave_number,
                    0.5 * p.youngs_modulus / (1.0 + p.poisson_ratio), 1.0 / p.rest_length};
  const long long tiles = static_cast<long long>((n + kTile - 1) / kTile);
  dispatch_bools(p.wave != 0, external_force != nullptr, [&](auto wv, auto ex) {
    k_filament_nodes<decltype(wv)::value, decltype(ex)::value><<<grid_for(n), kBlock, 0, s>>>(
        static_cast<long long>(n), tiles, P, p.wave_frequency * time, h->flag.as<uint8_t>(), h->fid.as<int32_t>(),
        h->phase.as<double>(), h->radius.as<double>(), h->rest.as<double>(), h->arclength.as<double>(),
        h->tangent[cur].as<double>(), h->binormal[cur].as<double>(), h->length[cur].as<double>(),
        h->orient[cur].as<double>(), external_force, h->force.as<double>(), h->torque.as<double>(),
        h->curvature.as<double>(), reinterpret_cast<unsigned long long*>(stats));
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_force(mhip_filaments_t h, double time, const double* external_force, double* stats) {
  // every refusal comes before the first launch
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(stats != nullptr, MHIP_ERR_INVALID_ARGUMENT, "stats is null");
  MHIP_REQUIRE(std::isfinite(time), MHIP_ERR_INVALID_ARGUMENT, "time must be finite, got %g", time);
  if (int e = mhip_filaments_edge_pass(h)) return e;
  return mhip_filaments_node_pass(h, time, external_force, stats);
}

int mhip_filaments_velocity(mhip_filaments_t h) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_velocity before mhip_filaments_set_state");
  if (h->n == 0) return MHIP_SUCCESS;
  const double c6 = 1.0 / (6.0 * M_PI * h->prm.viscosity), c8 = 1.0 / (8.0 * M_PI * h->prm.viscosity);  // :1755-1756
  k_filament_velocity<<<grid_for(h->n), kBlock, 0, h->stream>>>(h->n, c6, c8, h->radius.as<double>(),
                                                                h->force.as<double>(), h->torque.as<double>(),
                                                                h->vel.as<double>(), h->twist_vel.as<double>());
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_get(mhip_filaments_t h, mhip_filament_fields* out) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(out != nullptr, MHIP_ERR_INVALID_ARGUMENT, "fields is null");
  const int cur = h->cur, old = cur ^ 1;
  out->num_nodes = h->n;
  out->num_filaments = h->f;
  out->center = h->center.as<double>();
  out->twist = h->twist.as<double>();
  out->velocity = h->vel.as<double>();
  out->twist_velocity = h->twist_vel.as<double>();
  out->force = h->force.as<double>();
  out->twist_torque = h->torque.as<double>();
  out->radius = h->radius.as<double>();
  out->rest_curvature = h->rest.as<double>();
  out->arclength = h->arclength.as<double>();
  out->curvature = h->curvature.as<double>();
  out->phase = h->phase.as<double>();
  out->edge_tangent = h->tangent[cur].as<double>();
  out->edge_orientation = h->orient[cur].as<double>();
  out->edge_length = h->length[cur].as<double>();
  out->edge_binormal = h->binormal[cur].as<double>();
  out->edge_tangent_old = h->tangent[old].as<double>();
  out->edge_orientation_old = h->orient[old].as<double>();
  out->edge_length_old = h->length[old].as<double>();
  out->edge_binormal_old = h->binormal[old].as<double>();
  return MHIP_SUCCESS;
}

// ---- mundy_hip_filament_inertial.h ------------------------------------------------------------------------------------
int mhip_filaments_set_inertial(mhip_filaments_t h, const mhip_filament_inertial_params* params,
                                const unsigned char* fixed_filament) {
  // the arguments that need no handle first, so that every refusal can be had without a device
  MHIP_REQUIRE(params != nullptr, MHIP_ERR_INVALID_ARGUMENT, "params is null");
  const mhip_filament_inertial_params& p = *params;
  MHIP_REQUIRE(std::isfinite(p.density) && p.density > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "density must be finite and > 0, got %g", p.density);
  MHIP_REQUIRE(p.damping_kind == MHIP_FILAMENT_DAMPING_CONSTANT || p.damping_kind == MHIP_FILAMENT_DAMPING_CRITICAL,
               MHIP_ERR_INVALID_ARGUMENT, "unknown damping kind %d", p.damping_kind);
  if (p.damping_kind == MHIP_FILAMENT_DAMPING_CONSTANT)
    MHIP_REQUIRE(std::isfinite(p.translational_damping) && p.translational_damping >= 0.0 &&
                     std::isfinite(p.twist_damping) && p.twist_damping >= 0.0,
                 MHIP_ERR_INVALID_ARGUMENT, "damping coefficients must be finite and >= 0, got %g, %g",
                 p.translational_damping, p.twist_damping);
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  const size_t n = h->n, d = sizeof(double);
  hipStream_t s = h->stream;
  std::vector<uint8_t> fixed;
  bool any = false;
  if (fixed_filament) {
    fixed.assign(n, 0);
    const std::vector<int32_t>& ptr = h->host_node_ptr;
    for (size_t f = 0; f < h->f; ++f)
      if (fixed_filament[f]) {
        any = true;
        for (int32_t i = ptr[f]; i < ptr[f + 1]; ++i) fixed[i] = 1;
      }
  }
  int e = MHIP_SUCCESS;
  if ((e = h->acc.reserve(3 * n * d + 8)) || (e = h->twist_acc.reserve(n * d + 8)) || (e = h->fixed.reserve(n + 8)) ||
      (e = h->energy_partials.reserve(2 * kMaxGrid * d)))
    return e;
  if (n > 0) {
    MHIP_HIP(hipMemsetAsync(h->acc.ptr, 0, 3 * n * d, s));
    MHIP_HIP(hipMemsetAsync(h->twist_acc.ptr, 0, n * d, s));
    if (any) {
      if ((e = upload(__func__, h->fixed, fixed.data(), n, s))) return e;
      if ((e = hip_status(__func__, hipStreamSynchronize(s)))) return e;  // `fixed` goes when this returns
    }
  }
  h->iprm = p;
  h->any_fixed = any;
  h->inertial = true;
  return MHIP_SUCCESS;
}

int mhip_filaments_set_motion(mhip_filaments_t h, const double* velocity, const double* twist_velocity,
                              const double* acceleration, const double* twist_acceleration) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(h->inertial, MHIP_ERR_RUNTIME, "mhip_filaments_set_motion before mhip_filaments_set_inertial");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_set_motion before mhip_filaments_set_state");
  const size_t n = h->n, d = sizeof(double);
  if (n == 0) return MHIP_SUCCESS;
  hipStream_t s = h->stream;
  const struct {
    HandleBuffer* dst;
    const double* src;
    size_t bytes;
  } rows[] = {{&h->vel, velocity, 3 * n * d},
              {&h->twist_vel, twist_velocity, n * d},
              {&h->acc, acceleration, 3 * n * d},
              {&h->twist_acc, twist_acceleration, n * d}};
  for (const auto& r : rows) {
    if (r.src) MHIP_HIP(hipMemcpyAsync(r.dst->ptr, r.src, r.bytes, hipMemcpyDeviceToDevice, s));
    else MHIP_HIP(hipMemsetAsync(r.dst->ptr, 0, r.bytes, s));
  }
  return MHIP_SUCCESS;
}

int mhip_filaments_predict(mhip_filaments_t h, double dt) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  MHIP_REQUIRE(h->inertial, MHIP_ERR_RUNTIME, "mhip_filaments_predict before mhip_filaments_set_inertial");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_predict before mhip_filaments_set_state");
  h->cur ^= 1;  // rotate_field_states: what was new is old
  if (h->n == 0) return MHIP_SUCCESS;
  const double beta = 0.25;
  const double coeff = 0.5 * dt * dt * (1.0 - 2.0 * beta);  // :1012-1013
  dispatch_bools(h->prm.disable_twist != 0, h->prm.monolayer != 0, [&](auto nt, auto ml) {
    k_filament_predict<decltype(nt)::value, decltype(ml)::value><<<grid_for(h->n), kBlock, 0, h->stream>>>(
        h->n, dt, coeff, h->center.as<double>(), h->twist.as<double>(), h->vel.as<double>(), h->twist_vel.as<double>(),
        h->acc.as<double>(), h->twist_acc.as<double>());
  });
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

static int filament_energy_fold(mhip_filaments_t h, double* out) {
  k_filament_energy_fold<<<1, kBlock, 0, h->stream>>>(grid_for(h->n), h->energy_partials.as<double>(), out);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

int mhip_filaments_correct(mhip_filaments_t h, double dt, double* kinetic_energy) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(std::isfinite(dt) && dt >= 0.0, MHIP_ERR_INVALID_ARGUMENT, "dt must be finite and >= 0, got %g", dt);
  MHIP_REQUIRE(h->inertial, MHIP_ERR_RUNTIME, "mhip_filaments_correct before mhip_filaments_set_inertial");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_correct before mhip_filaments_set_state");
  hipStream_t s = h->stream;
  if (h->n == 0) {
    if (kinetic_energy) MHIP_HIP(hipMemsetAsync(kinetic_energy, 0, sizeof(double), s));
    return MHIP_SUCCESS;
  }
  const double gamma = 0.5, beta = 0.25;
  const mhip_filament_inertial_params& p = h->iprm;
  const NewmarkD P{(1.0 - gamma) * dt, dt * dt * beta, dt * gamma, p.density, h->prm.youngs_modulus,
                   p.translational_damping, p.twist_damping};
  dispatch_bools(p.damping_kind == MHIP_FILAMENT_DAMPING_CRITICAL, h->any_fixed, [&](auto cr, auto fx) {
    dispatch<true, false>(kinetic_energy != nullptr, [&](auto en) {
      k_filament_correct<decltype(cr)::value, decltype(fx)::value, decltype(en)::value>
          <<<grid_for(h->n), kBlock, 0, s>>>(h->n, P, h->radius.as<double>(), h->fixed.as<uint8_t>(),
                                             h->force.as<double>(), h->torque.as<double>(), h->center.as<double>(),
                                             h->twist.as<double>(), h->vel.as<double>(), h->twist_vel.as<double>(),
                                             h->acc.as<double>(), h->twist_acc.as<double>(),
                                             h->energy_partials.as<double>());
    });
  });
  MHIP_LAUNCH_CHECK();
  return kinetic_energy ? filament_energy_fold(h, kinetic_energy) : MHIP_SUCCESS;
}

int mhip_filaments_kinetic_energy(mhip_filaments_t h, double* out) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(out != nullptr, MHIP_ERR_INVALID_ARGUMENT, "out is null");
  MHIP_REQUIRE(h->inertial, MHIP_ERR_RUNTIME, "mhip_filaments_kinetic_energy before mhip_filaments_set_inertial");
  MHIP_REQUIRE(h->has_state, MHIP_ERR_RUNTIME, "mhip_filaments_kinetic_energy before mhip_filaments_set_state");
  hipStream_t s = h->stream;
  if (h->n == 0) {
    MHIP_HIP(hipMemsetAsync(out, 0, sizeof(double), s));
    return MHIP_SUCCESS;
  }
  k_filament_energy<<<grid_for(h->n), kBlock, 0, s>>>(h->n, h->iprm.density, h->radius.as<double>(),
                                                      h->vel.as<double>(), h->twist_vel.as<double>(),
                                                      h->energy_partials.as<double>());
  MHIP_LAUNCH_CHECK();
  return filament_energy_fold(h, out);
}

int mhip_filaments_set_youngs_modulus(mhip_filaments_t h, double youngs_modulus) {
  MHIP_REQUIRE(std::isfinite(youngs_modulus) && youngs_modulus >= 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "youngs_modulus must be finite and >= 0, got %g", youngs_modulus);
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  h->prm.youngs_modulus = youngs_modulus;  // the node pass forms the shear modulus from it at every call
  return MHIP_SUCCESS;
}

int mhip_filaments_get_inertial(mhip_filaments_t h, mhip_filament_inertial_fields* out) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "filaments handle is null");
  MHIP_REQUIRE(out != nullptr, MHIP_ERR_INVALID_ARGUMENT, "fields is null");
  out->acceleration = h->acc.as<double>();
  out->twist_acceleration = h->twist_acc.as<double>();
  return MHIP_SUCCESS;
}

}  // extern "C"
