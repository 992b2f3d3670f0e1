/* mundy_hip_hydro_periphery.h -- the periphery's no-slip correction of the n-body hydrodynamics.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (PERIPHERY_SIGNATURES): tests/test_gpu_streams.py fails for any stream-taking prototype of mundy_hip.h that its case
 * table does not call, and tests/test_capi_symbols.py for a binding of SIGNATURES that mundy_hip.h does not declare, and
 * the change that added these entry points could edit neither file.  tests/test_gpu_hydro_periphery_streams.py and
 * tests/test_hydro_periphery_host.py make the same two checks over this header.  A later change that may edit those
 * files folds this header back into mundy_hip.h.  The contract is mundy_hip.h's: every entry point that launches work
 * takes a mhip_stream_t and is ordered on it; only entry points that return host scalars synchronise.
 *
 * The second and third thirds of the reference's compute_rpy_hydro (scrap/.../HP1.cpp:3942-4059; :4005-4037), which
 * follow the beads-to-beads sum of mhip_hydro_velocity when enable_periphery_hydrodynamics is on (the default):
 *   u_surf = K(beads -> nodes) F              mhip_hydro_velocity, rectangular, node radius 0
 *   f_surf = -(Minv u_surf)                   Periphery.hpp:2125-2140
 *   u_bead += DL(nodes -> beads) f_surf       apply_stokes_double_layer_kernel, Periphery.hpp:1221-1313
 * The surface: S nodes with positions y [S][3], inward normals n [S][3] and quadrature weights w [S]; N = 3 S.  The
 * library generates no quadrature (the reference's FROM_FILE mode); mundy_amd.synth.sphere_quadrature restates
 * gen_sphere_quadrature (Periphery.hpp:90-167).
 *
 * The matrix (fill_skfie_matrix, Periphery.hpp:1370-1597; what its code does: no 1/2 I is added anywhere), row-major
 * [N][N], rows 3t+i, columns 3s+j, d = y_t - y_s, r2 = dx dx + dy dy + dz dz (left to right, as every sum below):
 *   T[3t+i][3s+j] = d_i (((scale rinv5) (dx nw0 + dy nw1 + dz nw2)) d_j),  nw = n_s w_s,
 *       scale = -3.0 / (4.0 * M_PI * viscosity), rinv = r2 < 1e-12 ? 0 : quake_inv_sqrt(r2), rinv5 = rinv rinv2 rinv2
 *   singularity subtraction: W[3t+i][c] = ROWSUM_s T[3t+i][3s+c] (c = 0, 1, 2);  T[3t+i][3t+c] += W[3t+i][c]
 *   complementary matrix:    M[3t+i][3s+j] = T[3t+i][3s+j] + n_t,i (n_s,j w_s)
 * ROWSUM, the summation order of the row sums and of mhip_hydro_periphery_surface_forces, a function of the length L
 * of the sequence a_0 .. a_{L-1} alone: 64 partial sums p_l = a_l + a_{l+64} + a_{l+128} + ... in ascending index from
 * +0.0 (every product a_j = Minv[r][j] u[j] is rounded before it is added), then six halvings p_l = p_l + p_{l+h} for
 * l < h, h = 32, 16, 8, 4, 2, 1; the sum is p_0.  One wave computes a row, whatever the grid.
 *
 * The inverse (the reference solves M X = I with KokkosBlas::gesv, Periphery.hpp:175-210): an in-place Gauss-Jordan
 * elimination with partial pivoting in fp64, every element operation independent of the launch shape.  For column
 * k = 0 .. N-1:
 *   the pivot row p is the row of k .. N-1 with the largest |A[i][k]|, the lowest index on a tie; rows k and p swap;
 *   with pv = A[k][k]:  A[k][k] = 1.0, then A[k][j] = A[k][j] / pv for every j (an IEEE division);
 *   for every row i != k: f = A[i][k], A[i][k] = 0.0, then A[i][j] = A[i][j] - f A[k][j] for every j (two roundings).
 * Then the column swaps k <-> p_k are undone for k = N-1 .. 0.  Three launches per column and one at the end, no host
 * round trip per column.  min_pivot is the smallest |pv|.  A pivot that is zero or not finite ends the elimination:
 * MHIP_ERR_RUNTIME, and the handle is left without a matrix.  Not the hot path: it runs once per simulation.
 *
 * The handle owns ONE [N][N] buffer: it holds M after a fill (or set_matrix), Minv after invert (or set_inverse);
 * mhip_hydro_periphery_matrix returns the device pointer and which of the two it holds.  It also owns u_surf and
 * f_surf [N] and copies of the quadrature.
 *
 * mhip_hydro_double_layer: u_t (+)= sum_s DL_ts with d = x_t - y_s and s_ij = (n_i f_j) w of source s,
 *   coeff = s_xx dx dx + s_yy dy dy + s_zz dz dz;  coeff += (s_xy + s_yx) dx dy;  coeff += (s_xz + s_zx) dx dz;
 *   coeff += (s_yz + s_zy) dy dz;  coeff *= (-scale_dl) rinv5;  u += d coeff
 *   scale_dl = 3.0 / (4.0 * M_PI * viscosity), rinv and rinv5 as above.
 * The summation order, the launch shapes (mhip_hydro_set_path), the handle's grow-only buffer and velocity_stride /
 * accumulate are those of mhip_hydro_velocity (MHIP_HYDRO_CHUNK).
 * skip_same_index, A REPRODUCED QUIRK: the reference's kernel returns early when the target index equals the source
 * index (Periphery.hpp:1274), which is right for nodes onto nodes; in the app's call, surface nodes onto beads, it
 * drops node i's contribution to bead i for every i < S.  != 0 (what the reference computes) skips the term of source
 * t onto target t, the index being the row index of the arrays passed in; 0 adds every term.
 *
 * mhip_hydro_periphery_correct: the three steps above with kind / n / center / radius / force the beads' (as in
 * mhip_hydro_velocity) accumulated into velocity (stride 3 or 6); `ws` serves both rectangular sums.
 *
 * Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: null arguments, S = 0 or 3 S > 65535, a viscosity that is
 * not finite or <= 0, a stride other than 3 or 6, an unknown kind; with MHIP_ERR_LOGIC: surface_forces or correct
 * before an inverse is present, invert without a matrix. */
#ifndef MUNDY_HIP_HYDRO_PERIPHERY_H_
#define MUNDY_HIP_HYDRO_PERIPHERY_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_HYDRO_PERIPHERY_EMPTY 0
#define MHIP_HYDRO_PERIPHERY_MATRIX 1
#define MHIP_HYDRO_PERIPHERY_INVERSE 2
#define MHIP_HYDRO_PERIPHERY_DOUBLE_LAYER 3 /* T alone: fill_double_layer (tests) */
typedef struct mhip_hydro_periphery* mhip_hydro_periphery_t;
int mhip_hydro_periphery_create(mhip_hydro_periphery_t* handle, size_t num_nodes, const double* points /*[S][3]*/,
                                const double* weights /*[S]*/, const double* normals /*[S][3]*/, double viscosity,
                                mhip_stream_t stream);
int mhip_hydro_periphery_destroy(mhip_hydro_periphery_t handle);
int mhip_hydro_periphery_fill_double_layer(mhip_hydro_periphery_t handle, mhip_stream_t stream);
int mhip_hydro_periphery_fill_matrix(mhip_hydro_periphery_t handle, mhip_stream_t stream);
int mhip_hydro_periphery_set_matrix(mhip_hydro_periphery_t handle, const double* matrix /*[N][N]*/,
                                    mhip_stream_t stream);
int mhip_hydro_periphery_invert(mhip_hydro_periphery_t handle, double* min_pivot /*[host]*/, mhip_stream_t stream);
int mhip_hydro_periphery_set_inverse(mhip_hydro_periphery_t handle, const double* inverse /*[N][N]*/,
                                     mhip_stream_t stream);
int mhip_hydro_periphery_matrix(mhip_hydro_periphery_t handle, const double** matrix /*[host]*/, int* state /*[host]*/);
int mhip_hydro_periphery_surface_forces(mhip_hydro_periphery_t handle, const double* u_surf /*[N]*/,
                                        double* f_surf /*[N]*/, mhip_stream_t stream);
int mhip_hydro_double_layer(mhip_hydro_t ws, double viscosity, size_t ns, const double* center, const double* normal,
                            const double* weight, const double* force, size_t nt, const double* target_center,
                            double* velocity, int velocity_stride, int accumulate, int skip_same_index,
                            mhip_stream_t stream);
int mhip_hydro_periphery_correct(mhip_hydro_periphery_t handle, mhip_hydro_t ws, int kind, size_t n,
                                 const double* center, const double* radius, const double* force, double* velocity,
                                 int velocity_stride, int skip_same_index, mhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
