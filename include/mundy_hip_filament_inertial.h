/* mundy_hip_filament_inertial.h -- inertial filaments: the Newmark step of the reference's sperm apps CollidingSperm.cpp
 * and CollidingFrictionalSperm.cpp (scrap/parameter_interface/alens/tests/performance_tests/), and the frictionless
 * Hertz law their segments may collide with.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (FILAMENT_INERTIAL_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives: tests/test_capi_symbols.py requires
 * the bindings of SIGNATURES to be exactly what mundy_hip.h declares, and the change that added these entry points could
 * edit no existing test.  tests/test_filament_inertial_host.py and tests/test_gpu_filament_inertial_streams.py make the
 * same checks over this header.  The contract is mundy_hip.h's: every call runs on the stream of its handle, none
 * synchronises but set_inertial (which uploads a host array).
 *
 * The handles are those of mundy_hip.h (mhip_filaments_t, mhip_filament_contacts_t).  The forces, the segment lists and
 * the reduction are the overdamped app's; what differs is how the nodes move.  Nodes have mass (a sphere of the node's
 * radius, lumped), and one step of the loop (CollidingFrictionalSperm.cpp:1890-1948) is
 *     predict -> [contacts: update, force] -> mhip_filaments_force(time, external_force) -> correct
 * with beta = 1/4, gamma = 1/2 (constant average acceleration).  The handle keeps acceleration [N][3] and
 * twist_acceleration [N] beside mundy_hip.h's fields.  There is no second copy of velocity or acceleration: the
 * reference's StateN / StateNP1 pair collapses, because both kernels are node-local, each reads a node's old values
 * before it overwrites them, and the force passes read neither field.
 *
 * set_inertial  allocates the two fields (+0.0) and stores the parameters.  fixed_filament [host, F bytes or NULL]: a
 *   non-zero byte marks a filament of the reference's BOUNDARY_SPERM part; the per-node flag is built here.  damping_kind
 *   MHIP_FILAMENT_DAMPING_CONSTANT: c_t = translational_damping, c_r = twist_damping (CollidingSperm.cpp:1576-1577);
 *   MHIP_FILAMENT_DAMPING_CRITICAL: c_t = c_r = sqrt(m E), E the handle's Young's modulus at the time of the call of
 *   correct (CollidingFrictionalSperm.cpp:1645-1646), the two numbers unused.  May be called again; mhip_filaments_set_state
 *   sets both fields to +0.0.  Refused before any HIP call with MHIP_ERR_INVALID_ARGUMENT: null params, density <= 0 or
 *   not finite, an unknown kind, a negative or non-finite damping (kind CONSTANT), a null handle.
 * set_motion  velocity [N][3], twist_velocity [N], acceleration [N][3], twist_acceleration [N]: device arrays copied into
 *   the handle, NULL = +0.0.  For restarts and tests.
 * predict  one kernel, per node in this order (the head of the loop, :1902-1921):
 *     disable_twist (:1699-1706)     twist = twist_velocity = twist_acceleration = +0.0
 *     apply_monolayer (:1708-1737)   center[0] = velocity[0] = acceleration[0] = +0.0
 *     rotate_field_states            the swap of the edge state, as mhip_filaments_advance does it (on the host)
 *     update_generalized_position (:968-1018)
 *         coeff = ((0.5 dt) dt) (1.0 - 2.0 beta)           formed once on the host
 *         x = (x + dt v) + coeff a,   twist = (twist + dt twist_velocity) + coeff twist_acceleration
 *   zero_out_transient_node_fields (:955-966) is not restated: the node pass writes force and torque from +0.0 or the
 *   external force, and the corrector overwrites velocity and acceleration, so no zeroed value is ever read.
 * correct  update_generalized_position_velocity_and_acceleration (:1616-1672; CollidingSperm.cpp:1563-1595), one kernel,
 *   per node, F and T the handle's force and twist_torque:
 *     m = (((4.0 / 3.0) pi) r3) rho,  r3 = (r r) r;     I = ((2.0 / 5.0) m) (r r)
 *     pv = v + ((1.0 - gamma) dt) a                     (v, a: the values before the call)
 *     a = (1.0 / m) (F - c_t v);   x += ((dt dt) beta) a;   v = pv + (dt gamma) a
 *     and the same for the twist with I, c_r and T.
 *   A node of a fixed filament (:1652-1656) gets velocity = acceleration = twist_velocity = twist_acceleration = +0.0 and
 *   no correction.  kinetic_energy [device, 1 double] or NULL: the sum over the nodes of
 *     (0.5 m) dot(v, v) + ((0.5 I) w) w          (:1767-1769; dot a right fold, v and w the values just written)
 *   accumulated in double-double pairs per lane and per workgroup, the workgroups' pairs folded by one workgroup in a fixed
 *   order and rounded once: the correctly rounded sum, whatever the grid.  NULL skips the sum and changes no other output.
 * kinetic_energy  the same number from the handle's current velocities, by the same partial sums and fold.
 * set_youngs_modulus  replaces the modulus the rod forces (E and the shear modulus formed from it on the host) and the
 *   critical damping read: the stiffness ramp of equilibriate (:1781-1865).  The contacts' modulus is a parameter of
 *   their own and does not move.  Refused: a modulus < 0 or not finite.
 * get_inertial  the two device pointers (NULL before set_inertial).
 * predict / correct / kinetic_energy before set_inertial or mhip_filaments_set_state: MHIP_ERR_RUNTIME, the message
 * names the missing call.  dt must be finite and >= 0.  mhip_filaments_advance and mhip_filaments_velocity keep working on
 * an inertial handle.
 *
 * mhip_filament_contacts_set_law  MHIP_FILAMENT_CONTACT_FRICTIONAL (the default: mundy_hip.h's law) or
 *   MHIP_FILAMENT_CONTACT_HERTZ, the frictionless law of
 *   .../linkers/src/mundy_linkers/.../SpherocylinderSegmentSpherocylinderSegmentHertzianContact.cpp:208-225:
 *     R = (ri rj) / (ri + rj),  E* as written there,  F = (4.0 / 3.0) E* sqrt(R) pow(-sep, 1.5) for sep < 0,
 *     force on the left segment = (-F) n
 *   (hertz_force_magnitude of the sphere and backbone laws; pow is the math library's, correct to an ulp, so a host
 *   restatement agrees to ~1e-15 relative and the reduction of the device's own rows bit for bit).  The linker pass then
 *   reads no velocity, needs no save_velocity, leaves tang_disp at +0.0 and counts nothing in stats[1].  The segment
 *   view, the list, the shares and the reduction are untouched.  Refused: a null handle, an unknown law.
 *
 * Not built: clamp_edge1 (commented out in every loop of the reference), the two-component rest-curvature form of
 * CollidingFrictionalSperm.cpp:1072-1082 (the wave stays mundy_hip.h's), periodic cells, several GPUs. */
#ifndef MUNDY_HIP_FILAMENT_INERTIAL_H_
#define MUNDY_HIP_FILAMENT_INERTIAL_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_FILAMENT_DAMPING_CONSTANT 0
#define MHIP_FILAMENT_DAMPING_CRITICAL 1
#define MHIP_FILAMENT_CONTACT_FRICTIONAL 0
#define MHIP_FILAMENT_CONTACT_HERTZ 1

typedef struct mhip_filament_inertial_params {
  double density;
  int damping_kind;
  double translational_damping, twist_damping;
} mhip_filament_inertial_params;
typedef struct mhip_filament_inertial_fields {
  double* acceleration;       /* [N][3] */
  double* twist_acceleration; /* [N] */
} mhip_filament_inertial_fields;

int mhip_filaments_set_inertial(mhip_filaments_t handle, const mhip_filament_inertial_params* params,
                                const unsigned char* fixed_filament /*[host] F bytes or NULL*/);
int mhip_filaments_set_motion(mhip_filaments_t handle, const double* velocity, const double* twist_velocity,
                              const double* acceleration, const double* twist_acceleration);
int mhip_filaments_predict(mhip_filaments_t handle, double dt);
int mhip_filaments_correct(mhip_filaments_t handle, double dt, double* kinetic_energy /*[device] or NULL*/);
int mhip_filaments_kinetic_energy(mhip_filaments_t handle, double* out /*[device]*/);
int mhip_filaments_set_youngs_modulus(mhip_filaments_t handle, double youngs_modulus);
int mhip_filaments_get_inertial(mhip_filaments_t handle, mhip_filament_inertial_fields* fields /*[host]*/);
int mhip_filament_contacts_set_law(mhip_filament_contacts_t handle, int law);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_FILAMENT_INERTIAL_H_ */
