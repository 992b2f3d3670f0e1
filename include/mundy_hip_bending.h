/* mundy_hip_bending.h -- semiflexible chains: angular (three-body) springs, and the parameters of the FENE-WCA bond.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (BENDING_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives.  tests/test_bending_host.py and
 * tests/test_gpu_bending_streams.py make over this header the checks that tests/test_capi_symbols.py and
 * tests/test_gpu_streams.py make over mundy_hip.h.  The contract is mundy_hip.h's: every entry point that takes a
 * mhip_stream_t is ordered on it; only create (which frees the caller's host arrays on return) and get synchronise.
 *
 * ---- MHIP_SPRING_FENEWCA (a third type of mhip_springs_create; r = r_max > 0, k >= 0) -------------------------------
 * The Kremer-Grest bond of the reference (FENEWCASpringsKernel.cpp:147-176), in its expressions and association.  With
 * d = x_j - x_i and L = sqrt(d.d) (right fold) as for the other two types:
 *   L_adj  = min(L, r_max - 1e-4)                              (its hard-coded epsilon_reg; a NaN L stays NaN)
 *   spring = k L_adj / (1 - (L_adj / r_max) (L_adj / r_max))
 *   rho2   = sigma sigma / (L_adj L_adj),  rho6 = rho2 rho2 rho2,  rho12 = rho6 rho6
 *   lj     = 6 4 epsilon (2 rho12 - rho6) / L_adj  where L_adj < cutoff,  0 otherwise
 *   fm     = (spring - lj) (1 / L)
 * and body i receives +fm d, body j -fm d, the sign convention of the other two types: the bond attracts when stretched
 * and repels inside the cutoff.  (The reference scales d by 1 / L first and multiplies by the magnitude afterwards; the
 * library keeps one fm d for every type, so the last two roundings differ from that text.)
 * cutoff = 2^(1/6) sigma is computed once on the host, at create and at set_wca, and kept in the handle: no kernel calls
 * pow.  The bond never goes without force: past the clamp it pulls with the finite force of L_adj = r_max - 1e-4.
 * *overstretched of mhip_springs_force counts the clamped bonds, those with !(L < r_max - 1e-4).
 * epsilon and sigma are 1 and 1 after create, as the reference hard-codes them.  set_wca replaces them: both finite and
 * > 0; refused for a handle of another type.  A host call: it touches no stream, and holds for every later force. */
#ifndef MUNDY_HIP_BENDING_H_
#define MUNDY_HIP_BENDING_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int mhip_springs_set_wca(mhip_springs_t handle, double epsilon, double sigma);

/* ---- angular springs (AngularSpringsKernel.cpp:107-197; generated per bead triple by ChainOfSprings.cpp:436-467) ------
 * m triplets (a, b, c) = triplets[t] between n bodies: the two ends first, the centre last, the reference's BEAM_3 node
 * order.  k [m] / rest_angle [m] per triplet [host], or NULL: then the scalar stands for every triplet.
 * create copies them and refuses (MHIP_ERR_INVALID_ARGUMENT, before any HIP call) an index outside [0, n), a triplet
 * whose three bodies are not distinct, k < 0, a rest angle outside [0, pi], anything not finite, m >= 2^29.  It takes
 * cos(rest_angle) with std::cos once, on the host, and stores that double: the device evaluates no trigonometric
 * function, and get hands the stored values out, so a host model shares them to the bit.  It builds the
 * body -> entry incidence on the device (entry (t << 2) | role, role 0 = end a, 1 = end b, 2 = centre c) and
 * synchronises `stream`.
 *
 * force, in the reference's association and with the library's right-fold dot:
 *   v1 = x_a - x_c,  v2 = x_b - x_c,  s1 = v1.v1,  s2 = v2.v2,  L1 = sqrt(s1),  L2 = sqrt(s2)
 *   c = (v1.v2) / (L1 L2),  tau = k (c - cos_rest)
 *   a11 = tau c / s1,  a13 = -tau / (L1 L2),  a33 = tau c / s2
 *   F_a = a11 v1 + a13 v2,  F_b = a33 v2 + a13 v1,  F_c = -F_a - F_b
 * which is -grad of U = 1/2 k (cos(theta) - cos_rest)^2.  One body per lane: it adds the rows of its entries in
 * ascending entry order from +0.0 and evaluates the whole triplet, in the same operations, at each of its three bodies;
 * the three rows of a triplet are one function of the same inputs, and F_c is exactly the negated sum of the other two.
 * No atomics on forces.  accumulate = 0 writes every row of force [n][3] (a body on no triplet gets +0.0 exactly);
 * accumulate = 1 adds each body's sum to its row and leaves the rows of bodies on no triplet alone.
 * A triplet with L1 == 0 or L2 == 0 gives NaN rows, as in the reference; *degenerate [device, 1 int] counts those
 * triplets (each once, at its role-0 entry).  *max_deviation [device, 1 double] = the largest |c - cos_rest|
 * (+0.0 without triplets; a NaN is never taken), order independent.
 *
 * renumber: the bodies were permuted; every index i becomes new_of_old[i] ([device] n int32) and the incidence is
 * rebuilt on the device.  Triplet order, k and cos_rest stay.
 * get: host copies of what the handle holds -- triplets [m][3] int32 (after any renumbering; the call waits for the
 * device), k [m] and cos_rest [m] (a scalar repeated); any pointer may be NULL. */
typedef struct mhip_angular_springs* mhip_angular_springs_t;
int mhip_angular_springs_create(mhip_angular_springs_t* handle, size_t n, size_t m,
                                const int32_t* triplets /*[host] m x 3: end a, end b, centre c*/,
                                const double* k /*[host] m or NULL*/, double k_scalar,
                                const double* rest_angle /*[host] m or NULL*/, double rest_angle_scalar,
                                mhip_stream_t stream);
int mhip_angular_springs_force(mhip_angular_springs_t handle, const double* center, double* force, int accumulate,
                               int* degenerate /*[device]*/, double* max_deviation /*[device]*/, mhip_stream_t stream);
int mhip_angular_springs_renumber(mhip_angular_springs_t handle, const int32_t* new_of_old /*[device] n*/,
                                  mhip_stream_t stream);
int mhip_angular_springs_get(mhip_angular_springs_t handle, int32_t* triplets /*[host] m x 3*/, double* k /*[host] m*/,
                             double* cos_rest /*[host] m*/);
int mhip_angular_springs_destroy(mhip_angular_springs_t handle);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_BENDING_H_ */
