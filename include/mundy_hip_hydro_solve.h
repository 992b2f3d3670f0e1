/* mundy_hip_hydro_solve.h -- the sphere LCP solved against a hydrodynamic mobility: A = dt D^T M_h D.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (HYDRO_SOLVE_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives: tests/test_gpu_streams.py fails for any
 * stream-taking prototype of mundy_hip.h that its case table does not call, tests/test_capi_symbols.py for a binding of
 * SIGNATURES that mundy_hip.h does not declare, and the change that added these entry points could edit neither file.
 * tests/test_hydro_solve_host.py and tests/test_gpu_hydro_solve_streams.py make the same checks over this header.  The
 * contract is mundy_hip.h's: the two stream-taking entry points are ordered on their stream; the solve synchronises it
 * at its polls and before it returns, apply_hydro never.
 *
 * The reference's newer chromatin app resolves collisions through a mobility operator: every BBPGD iteration is
 * F = D lambda -> U = M F -> sdot = D^T U (resolve_collisions over an ApplyMobilityOp,
 * scrap/parameter_interface/alens/tests/performance_tests/NgpHP1.cpp:1487-1645), with M the local drag, RPY + local drag
 * (SphereRpyMobilityOp, :677-701, :833-925) or RPY + no-slip periphery + local drag (SphereConfinedRpyMobilityOp,
 * :703-766, :927-1023).  mhip_bbpgd_solve_contact is the first; this header adds the other two on the library's own pair
 * kernels.
 *
 * The mobility.  n spheres, C contacts, a sphere-kinematics operator (no lever arms, no mob_rot).  On the per-body
 * forces F [n][3], in this order and association:
 *     U_b  = m_t[b] * F_b                    the operator's mob_trans, rounded as the body sweep rounds it
 *     U   += hydro_kind(F)                   mhip_hydro_velocity, accumulate = 1, targets = sources = all n bodies
 *     U   += periphery_correction(F)         only with a periphery: mhip_hydro_periphery_correct on the same rows
 * and A x = dt D^T M_h D x; the LCP is 0 <= x  _|_  A x + q >= 0.  Kinds: MHIP_HYDRO_RPYC and MHIP_HYDRO_RPY; the
 * Stokeslet is refused (it is not positive semi-definite at bead separations).  The hydrodynamic radii are the
 * mobility's own array, m_t stays the operator's: keeping the two consistent is the caller's job, as in the velocity
 * stage.  Free space only.
 *
 * mhip_hydro_mobility describes M_h without its dry part.  The arrays are device memory the caller keeps alive; center
 * and radius are read by every call.  periphery: a handle holding its inverse (mhip_hydro_periphery_invert /
 * _set_inverse), or NULL; skip_same_index is the periphery correction's argument of that name.  viscosity is the pair
 * kernel's; the periphery's correction is mhip_hydro_periphery_correct's and uses the viscosity its handle was created
 * with, as everywhere: the two have to agree, which is the caller's job (the composition above is the contract).
 * The workspace is used as by mhip_hydro_velocity (its grow-only buffer: one call at a time, as for every mhip_hydro_t)
 * and nothing of it is changed: the calls' own launches compact their source tiles whatever its sparse-source switch
 * says, and the switch stays as the caller set it.
 *
 * mhip_contact_op_apply_hydro (NgpHP1.cpp:1487-1645, one application; :833-925, :927-1023): y = dt D^T M_h D x, and the
 * operator's rows (mhip_contact_op_body_velocity) hold M_h D x afterwards.  y and the rows equal, bit for bit, the
 * composition of the public calls in the order above: mhip_contact_op_body_force(x) at stride 3, m_t F as
 * mhip_contact_op_body_sweep(x) leaves it, mhip_hydro_velocity accumulating at stride 6, mhip_hydro_periphery_correct,
 * then dt * mhip_contact_op_constraint_rate.
 *
 * mhip_bbpgd_solve_contact_hydro (NgpHP1.cpp:1487-1645; the algorithm of convex.hpp:592-681): mhip_bbpgd_solve_contact
 * with that operator.  Step size and residual stay on the device, the host polls at the fused driver's cadence, and the
 * four vectors have the fused driver's post-conditions.  On return the rows hold M_h D x of the returned x.  Per
 * iteration: one body sweep that leaves F_b (rounded once: the bits of mhip_contact_op_body_force) beside U_b = m_t F_b,
 * the pair kernel accumulating into the rows, the periphery's three stages, the constraint sweep, the finalize.  All
 * launches go on the caller's stream; nothing is captured.  The solve's own pair sums walk compacted source tiles (below),
 * whatever the workspace's switch says.  The cold tier never runs here whatever mhip_contact_op_set_tiering says: with a
 * long-range mobility a body none of whose contacts is active still moves, so a sleeping contact's gradient changes
 * with forces far away, which the tier's drift bookkeeping (fed by a body's own contacts) would miss.  The body-side
 * activity masks stay valid: a body's force still comes from its own contacts only.
 * C == 0: converged in 0 iterations, the rows are +0.0.
 *
 * mhip_hydro_set_sparse_sources (a sibling of mhip_hydro_set_path; off by default): when a workgroup of
 * mhip_hydro_velocity stages a tile of 256 sources it keeps, in order, only those with a non-zero force component and
 * walks those.  A source with f = (+-0, +-0, +-0) adds +-0.0 to every target (finite inputs) and a sum started from
 * +0.0 is unchanged by +-0.0 terms, so every bit stays; the chunks are still MHIP_HYDRO_CHUNK consecutive indices of
 * the full list.  Both launch shapes; never the double layer.
 *
 * Refused before any HIP call with MHIP_ERR_INVALID_ARGUMENT: a null handle, struct, workspace, center or radius (n > 0),
 * null x / y or solver vectors with C > 0, an operator with lever arms, rods or mob_rot, mob.n other than the operator's
 * body count, a space other than LowerBound{0}, the Stokeslet or an unknown kind, a viscosity that is not finite and
 * positive; with MHIP_ERR_RUNTIME: a staged solve in progress; with MHIP_ERR_LOGIC: an operator partitioned by
 * mhip_contact_op_set_partition, a periphery without its inverse (as mhip_hydro_periphery_correct refuses it). */
#ifndef MUNDY_HIP_HYDRO_SOLVE_H_
#define MUNDY_HIP_HYDRO_SOLVE_H_

#include "mundy_hip.h"
#include "mundy_hip_hydro_periphery.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mhip_hydro_mobility {
  mhip_hydro_t workspace;
  int kind; /* MHIP_HYDRO_RPYC | MHIP_HYDRO_RPY */
  double viscosity;
  size_t n;
  const double* center; /* [n][3] */
  const double* radius; /* [n] hydrodynamic radii */
  mhip_hydro_periphery_t periphery; /* or NULL */
  int skip_same_index;
} mhip_hydro_mobility;

int mhip_hydro_set_sparse_sources(mhip_hydro_t handle, int on);
int mhip_contact_op_apply_hydro(mhip_contact_op_t handle, const mhip_hydro_mobility* mobility, const double* x /*[C]*/,
                                double* y /*[C]*/, mhip_stream_t stream);
int mhip_bbpgd_solve_contact_hydro(mhip_contact_op_t handle, const mhip_hydro_mobility* mobility, const double* q,
                                   const mhip_space* space, const mhip_pgd_config* config, double* x, double* g,
                                   double* x_tmp, double* g_tmp, mhip_solve_result* result, mhip_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_HYDRO_SOLVE_H_ */
