/* mundy_hip_contact_force.h -- the per-body force and torque of a contact operator, F = D x.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (CONTACT_FORCE_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives: tests/test_gpu_streams.py fails for any
 * stream-taking prototype of mundy_hip.h that its case table does not call, tests/test_capi_symbols.py for a binding of
 * SIGNATURES that mundy_hip.h does not declare, tests/test_hydro_periphery_host.py and
 * tests/test_gpu_hydro_periphery_streams.py pin the periphery header to exactly its 11 prototypes, and the change that
 * added these entry points could edit none of those files.  tests/test_contact_force_host.py and
 * tests/test_gpu_contact_force_streams.py make the same checks over this header.  A later change that may edit those
 * files folds this header back into mundy_hip.h.  The contract is mundy_hip.h's: both entry points take a mhip_stream_t
 * and are ordered on it, neither synchronises.
 *
 * The library turns multipliers into velocities (mhip_contact_op_body_sweep[_vector]: U = M D x); these two hand out
 * F = D x itself, what the reference computes in SumCollisionForce (NgpLcp.cpp:442-474) and in
 * LinkerPotentialForceReduction (.../linker_potential_force_reduction/kernels/Spherocylinder.cpp:173-207): contact
 * stresses, force output, and the contact term of any other force consumer (the hydrodynamics of the chain step).
 *
 * out is caller-owned, [N][stride], stride 3 or 6.  Words 0-2 of row b: F_b = sum f over the contacts incident to b,
 *   scalar form (x [C]):        f = -(x_c n_c) at the source body (pairs[c].x), +(x_c n_c) at the target
 *   vector form (force [C][3]): f = +F_c at the source, -F_c at the target
 * -- the signs and per-term expressions of mhip_contact_op_body_sweep and mhip_contact_op_body_sweep_vector.  With
 * stride 6, words 3-5: the torque about the body centre from the operator's own lever arms,
 *   vector arms: T_b = sum r x f;   rods: T_b = u x sum coef f (u = p1 - p0, coef = s - 1/2);   spheres: +0.0.
 * A contact with x_c == 0, or F_c == (0, 0, 0), is never added (nor is its record read).  A sum without a term is +0.0;
 * of a rod without one the torque is u x (+0.0), whose components may be -0.0, as in the sweeps' rows.
 *
 * - Every sum is a double-double pair accumulated in the incidence index's fixed order and rounded once; the mobility is
 *   never applied.  The result does not depend on the operator's work mapping.
 * - accumulate = 1 adds the rounded sum to the old value: out = old + sum, one more rounding.  0 overwrites.
 * - Nothing of the operator is written: its rows (mhip_contact_op_body_velocity), omega and the solver state stay as
 *   they are, so a call after a solve leaves the solve's velocities valid.
 * - Bit relation to the sweeps: mhip_contact_op_body_sweep(x) gives U_b = m_t F_b, and W_b = m_r T_b for vector arms
 *   and rods, of this F_b and T_b, bit for bit (likewise the vector forms).
 * - C = 0 writes +0.0 rows (accumulate: leaves out alone); N = 0 does nothing.
 *
 * Refused before any HIP call with MHIP_ERR_INVALID_ARGUMENT: a null handle, null x / force with C > 0, null out with
 * N > 0, a stride other than 3 or 6, accumulate other than 0 or 1; with MHIP_ERR_RUNTIME: a staged solve in progress
 * (as the sweeps refuse it); with MHIP_ERR_LOGIC: an operator partitioned by mhip_contact_op_set_partition (the force
 * of a body whose contacts live on another rank is not this rank's to sum). */
#ifndef MUNDY_HIP_CONTACT_FORCE_H_
#define MUNDY_HIP_CONTACT_FORCE_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int mhip_contact_op_body_force(mhip_contact_op_t handle, const double* x /*[C]*/, double* out /*[N][stride]*/,
                               int stride, int accumulate, mhip_stream_t stream);
int mhip_contact_op_body_force_vector(mhip_contact_op_t handle, const double* force /*[C][3]*/,
                                      double* out /*[N][stride]*/, int stride, int accumulate, mhip_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_CONTACT_FORCE_H_ */
