/* mundy_hip.h -- C ABI of the MI355X (gfx950) implementation of MuNDy's contact hot path.
 *
 * One shared library, libmundy_hip.so, hand-written HIP underneath.  Every entry point returns an int status
 * (MHIP_SUCCESS == 0) and records a message retrievable with mhip_last_error() (thread local).  Unless a parameter is
 * marked [host], every pointer is a DEVICE pointer (hipMalloc / torch.cuda memory); `stream` is a hipStream_t passed
 * as void* (NULL = the null stream).  Entry points that return host scalars synchronise `stream`, exactly where the
 * reference's Kokkos parallel_reduce / deep_copy-to-host calls block; everything else is asynchronous.
 * Handles are not thread safe; use one handle per host thread / stream.
 * Handle-free entry points that need scratch (the orderings and the key sort, the ellipsoid and mixed distance
 * routines, the history carry) keep it per host thread, whatever the stream: their calls from ONE host thread are
 * ordered per scratch -- a call on another stream than the thread's previous call of the same family waits, on the
 * device, for that call to finish (an event recorded on the previous stream, which must still exist).  Calls on one
 * stream pay nothing for this; calls from different host threads share nothing.
 *
 * All floating point is fp64; the device code is built with -ffp-contract=off and follows the reference's operation
 * order (right-fold dot, q*(0,v)*inverse(q), tolerance constants, branch structure), so per-element results are
 * bit-identical to a scalar evaluation of the reference formulas.
 *
 * "Replaces" lines cite the reference interface (path:line under the MuNDy tree) that a maintainer would route
 * through each entry point; INTEGRATION.md shows the C++ binding.  Layouts: centre [n][3], quaternion [n][4] as
 * (w,x,y,z), AABB [n][6] as (min xyz, max xyz), pairs [c][2] int32 (source, target).
 */
#ifndef MUNDY_HIP_H_
#define MUNDY_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mhip_stream_t;

/* Status codes.  The C++ adapter (include/mundy_hip/adapter.hpp) maps them back to the exception types the reference
 * throws through MUNDY_THROW_REQUIRE (mundy/core/src/mundy_core/throw_assert.hpp:135-203). */
enum {
  MHIP_SUCCESS = 0,
  MHIP_ERR_INVALID_ARGUMENT = 1, /* std::invalid_argument: size mismatch, null pointer, bad enum */
  MHIP_ERR_LOGIC = 2,            /* std::logic_error */
  MHIP_ERR_RUNTIME = 3,          /* std::runtime_error: builder misuse, capacity */
  MHIP_ERR_HIP = 4,              /* a HIP runtime call failed (message carries hipGetErrorString) */
  MHIP_ERR_NO_DEVICE = 5         /* no gfx950 device visible: the library never falls back to the CPU */
};

const char* mhip_last_error(void);
int mhip_version(void);
/* roctx ranges around the stages of the path, named after the reference's functions / Kokkos kernel labels (visible to
 * rocprofv3 --marker-trace).  Off by default; MHIP_TRACE=1 in the environment enables it too. */
int mhip_set_tracing(int enable);
/* Fails with MHIP_ERR_NO_DEVICE when no GPU is visible. [host] out pointers. */
int mhip_device_info(int* device_count, char* arch_name, size_t arch_name_len);

/* Plain device memory for hosts that do not bring their own allocator. */
int mhip_malloc(void** ptr, size_t bytes);
int mhip_free(void* ptr);
/* What the library itself holds in this process, without a HIP call (any pointer may be null):
 *   handle_bytes   device bytes owned by live handles (broad phase, operators, communicators, force handles, ...), the
 *                  spare workspace set of destroyed operators included (mhip_release_cached_workspaces frees that);
 *   scratch_bytes  device bytes of the grow-only per-thread / per-process scratch, which lives until the process exits;
 *   pinned_bytes   pinned host bytes owned by live handles and the spare set;
 *   allocations    how many hipMalloc / hipHostMalloc calls those three have made so far (never decreases): constant
 *                  across the warm steps of a time loop.
 * Not counted: mhip_malloc, the IPC-mapped boxes of a communicator, the scratch's 64-byte pinned words. */
int mhip_memory_stats(size_t* handle_bytes, size_t* scratch_bytes, size_t* pinned_bytes, size_t* allocations);
int mhip_memcpy_h2d(void* dst, const void* src_host, size_t bytes, mhip_stream_t stream); /* synchronises: src_host is reusable */
int mhip_memcpy_d2h(void* dst_host, const void* src, size_t bytes, mhip_stream_t stream); /* synchronises */
int mhip_stream_synchronize(mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Per-body geometry (seam S4).
 * Replaces: compute_aabb(Sphere/Spherocylinder/Ellipsoid/SpherocylinderSegment)
 *           mundy/geom/src/mundy_geom/compute_aabb.hpp:72-143
 *           compute_bounding_radius(...) mundy/geom/src/mundy_geom/compute_bounding_radius.hpp:61-93
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_compute_aabb_spheres(size_t n, const double* center, const double* radius, double* aabb, mhip_stream_t stream);
int mhip_compute_aabb_spherocylinders(size_t n, const double* center, const double* quat, const double* radius,
                                      const double* length, double* aabb, mhip_stream_t stream);
int mhip_compute_aabb_ellipsoids(size_t n, const double* center, const double* quat, const double* radii,
                                 double* aabb, mhip_stream_t stream);
/* Build extension, the flagged option of SURVEY row a7: the reference's ellipsoid box (min/max of centre -/+ q*radii)
 * is exact only for axis-aligned rotations and is NOT conservative in general; this one is the tight box of the
 * rotated ellipsoid (half extent_k = sqrt(sum_j (r_j (q*e_j)_k)^2)).  No reference implementation: parity unpinned. */
int mhip_compute_aabb_ellipsoids_conservative(size_t n, const double* center, const double* quat, const double* radii,
                                              double* aabb, mhip_stream_t stream);
/* segment records seg[n][8] = (p0 xyz, p1 xyz, radius, 0) */
int mhip_compute_aabb_segments(size_t n, const double* seg, double* aabb, mhip_stream_t stream);
int mhip_bounding_radius_spherocylinders(size_t n, const double* radius, const double* length, double* out,
                                         mhip_stream_t stream);
int mhip_bounding_radius_ellipsoids(size_t n, const double* radii, double* out, mhip_stream_t stream);
/* Spherocylinder -> SpherocylinderSegment records: endpoints c -/+ 0.5*L*(q*zhat) (compute_aabb.hpp:115-117),
 * one 64-byte record per body so the pair kernels gather a single line per body. */
int mhip_spherocylinder_segments(size_t n, const double* center, const double* quat, const double* radius,
                                 const double* length, double* seg, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Narrow phase (seam S4).
 * Replaces: distance(SharedNormalSigned, Sphere, Sphere[, sep])     mundy/geom/src/mundy_geom/distance/SphereSphere.hpp:54-76
 *           distance(Point, LineSegment, cp, t, sep)                .../distance/PointLineSegment.hpp:128-172
 *           distance(LineSegment, LineSegment, cp1, cp2, s, t, sep) .../distance/LineSegmentLineSegment.hpp:189-318
 *           the per-linker contact kernels of the (deprecated) operator
 *           ComputeSignedSeparationDistanceAndContactNormal: scrap/lcp_spheres/NgpLcp.cpp:332-374 (spheres) and
 *           scrap/parameter_interface/linkers/.../SpherocylinderSpherocylinderLinker.cpp:207-247 (rods).
 * Any output pointer may be NULL to skip that output.
 * ---------------------------------------------------------------------------------------------------------------- */
/* element-wise batches over n independent object pairs (test / adapter entry points) */
int mhip_distance_sphere_sphere(size_t n, const double* c1, const double* r1, const double* c2, const double* r2,
                                double* dist, double* sep, mhip_stream_t stream);
int mhip_distance_point_segment(size_t n, const double* p, const double* a0, const double* a1, double* dist,
                                double* cp, double* t, double* sep, mhip_stream_t stream);
/* Replaces: distance(SharedNormalSigned, Point, Sphere[, sep])       .../distance/PointSphere.hpp:46-80
 *           distance(SharedNormalSigned, LineSegment, Sphere[, cp, arch_length, sep])
 *                                                                    .../distance/LineSegmentSphere.hpp:47-100
 * (the centre's distance to the point / to the segment, minus the radius; sep rescaled to the sphere's surface:
 * point -> surface, and for the segment the separation PointLineSegment hands back, centre -> closest point). */
int mhip_distance_point_sphere(size_t n, const double* p, const double* c, const double* r, double* dist, double* sep,
                               mhip_stream_t stream);
int mhip_distance_segment_sphere(size_t n, const double* a0, const double* a1, const double* c, const double* r,
                                 double* dist, double* cp, double* t, double* sep, mhip_stream_t stream);
int mhip_distance_segment_segment(size_t n, const double* a0, const double* a1, const double* b0, const double* b1,
                                  double* dist, double* cp1, double* cp2, double* s, double* t, double* sep,
                                  mhip_stream_t stream);
/* Ellipsoids: shared-normal signed distance by 3x3 multistart L-BFGS(10) over the normal's (theta, phi).
 * Replaces: distance(SharedNormalSigned, Ellipsoid, Ellipsoid, cp1, cp2, n1, n2)
 *           mundy/geom/src/mundy_geom/distance/EllipsoidEllipsoid.hpp:106-151, distance(Point, Ellipsoid, cp, n)
 *           .../PointEllipsoid.hpp:94-135, minimiser mundy/math/src/mundy_math/impl/minimize_impl.hpp:151-605.
 * radii [n][3] = body-frame semi-axes.  Tolerance against the host: 1e-4 (the reference's own,
 * UnitTestEllipsoidEllipsoid.cpp:52-53): device sin/cos differ from libm in the last bits. */
int mhip_distance_ellipsoid_ellipsoid(size_t n, const double* c1, const double* q1, const double* r1,
                                      const double* c2, const double* q2, const double* r2, double* dist, double* cp1,
                                      double* cp2, double* n1, double* n2, mhip_stream_t stream);
int mhip_distance_point_ellipsoid(size_t n, const double* p, const double* c, const double* q, const double* r,
                                  double* dist, double* cp, double* normal, mhip_stream_t stream);
/* neighbour-list form: sep, normal = n1, foot points cp1/cp2, lever arms ra/rb about the body centres */
int mhip_contact_ellipsoids(size_t c, const int32_t* pairs, const double* center, const double* quat,
                            const double* radii, double* sep, double* normal, double* cp1, double* cp2, double* ra,
                            double* rb, mhip_stream_t stream);
/* contact generation over a neighbour list: sep = |c_j - c_i| - r_i - r_j, normal = (c_j - c_i)/|c_j - c_i|.
 * box [host] = NULL (free space) or 3 doubles: PeriodicScaledMetric::sep (periodicity.hpp:812-816) minimum image. */
int mhip_contact_spheres(size_t c, const int32_t* pairs, const double* center, const double* radius,
                         const double* box, double* sep, double* normal, mhip_stream_t stream);
/* rods: seg from mhip_spherocylinder_segments; sep = dist(seg_i, seg_j) - (r_i + r_j); normal = (cp2 - cp1)/dist;
 * cp1/cp2 centreline closest points; ra/rb = cp - body centre (lever arms); s/t arclength parameters. */
int mhip_contact_spherocylinders(size_t c, const int32_t* pairs, const double* seg, const double* center, double* sep,
                                 double* normal, double* cp1, double* cp2, double* ra, double* rb, double* s,
                                 double* t, mhip_stream_t stream);
/* The same in an orthorhombic periodic box [host: 3 edge lengths]: rod j is taken at the lattice image whose centre is
 * nearest to rod i's centre -- shift = (c_i + PeriodicScaledMetric::sep(c_i, c_j)) - c_j (periodicity.hpp:812-816), a
 * rigid translation as wrap_rigid applies to a spherocylinder (:1094-1113).  Contact points are in rod i's image; rb is
 * taken from the shifted centre of rod j.  center is required. */
int mhip_contact_spherocylinders_periodic(size_t c, const int32_t* pairs, const double* seg, const double* center,
                                          const double* box /*[host] 3*/, double* sep, double* normal, double* cp1,
                                          double* cp2, double* ra, double* rb, double* s, double* t,
                                          mhip_stream_t stream);
/* Hertzian soft contact, per linker (c = (i, j), sep and normal from the contact routines above):
 *   R* = r_i r_j / (r_i + r_j)     E* = E_i E_j / (E_j - E_j nu_i^2 + E_i - E_i nu_j^2)
 *   force[c] = (4/3) E* sqrt(R*) (-sep)^1.5 if sep < 0, else +0.0
 * in the reference's association.  force[c] is the magnitude the contact operator takes as x (mhip_contact_op_body_sweep:
 * body i receives -force n, body j +force n).  radius [n] = sphere radius or rod radius (not the bounding radius).
 * youngs_modulus / poisson_ratio [n] per body, or NULL: then the scalar stands for every body (E > 0, 0 < nu < 1;
 * per-body arrays must satisfy the same).  *max_overlap [device, 1 double] = max(0, -sep) over the list (+0.0 for an
 * empty list), order independent.  A pair index outside [0, n) gives NaN and is never dereferenced.
 * Replaces: EvaluateLinkerPotentials with the Hertzian contact kernels,
 *           .../evaluate_linker_potentials/kernels/SphereSphereHertzianContact.cpp:198-219,
 *           SphereSpherocylinderHertzianContact.cpp:203-219, SpherocylinderSpherocylinderHertzianContact.cpp:205-219
 *           (called from scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:755-804). */
int mhip_hertz_contact_force(size_t c, size_t n, const int32_t* pairs, const double* sep, const double* radius,
                             const double* youngs_modulus, double youngs_modulus_scalar, const double* poisson_ratio,
                             double poisson_ratio_scalar, double* force, double* max_overlap, mhip_stream_t stream);
/* Frictional Hertzian contact of two rods with a per-pair tangential history, per linker.  For sep > 0 the history row
 * is reset and the force is +0.0 (both rows are written only where they are not +0.0 already); otherwise
 *   v_cp,b = U_b + W_b x ((s_b - 1/2)(p1_b - p0_b))   from velocity_prev [n][6] (U, W), the previous step's rows, and the
 *                                                     arm of the rod-compressed operator (arclength clamped to [0, 1])
 *   rel = v_cp,j - v_cp,i,  rel_n = (rel . n) n,  rel_t = rel - rel_n
 *   tang_disp += rel_t dt,  tang_disp -= (tang_disp . n) n
 *   R* = r_i r_j / (r_i + r_j),  m* = m_i m_j / (m_i + m_j) with m = 4/3 pi r^3 density,  hp = sqrt(-R* sep)
 *   F_n = hp (k_n sep n + m* normal_damping rel_n),  F_t = hp (k_t tang_disp + m* tangential_damping rel_t)
 *   if |F_t| > mu |F_n|: tang_disp and F_t are rescaled onto the Coulomb bound (F_t = 0 if |tang_disp| == 0)
 *   force[c] = F_n + F_t   on body i; body j receives its negative (mhip_contact_op_body_sweep_vector)
 * with k_n = 4/3 E* (E* as in mhip_hertz_contact_force) and k_t = 8 G*, G* = G_i G_j / (G_j (2 - nu_i) + G_i (2 - nu_j)),
 * G = 0.5 E / (1 + nu): for equal materials the reference's 4/3 G / (1 - nu) and 4 G / (2 - nu).  Right-fold dot and
 * norm, the reference's association.  Materials as in mhip_hertz_contact_force.  tang_disp [c][3] is read and written,
 * "j relative to i".  stats [device, 16 bytes]: a double max(0, -sep) over the contact branch, then a uint64 count of
 * the contacts whose tangential force was capped; both order independent.  A pair index outside [0, n) gives NaN rows
 * and is never dereferenced.  Refused before any HIP call: mu < 0, a negative damping, density or dt, anything not
 * finite, a null pointer that would be dereferenced.
 * Replaces: SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:384-518 (rigid rods). */
typedef struct {
  double mu, normal_damping, tangential_damping, density, dt;
} mhip_hertz_friction_params;
int mhip_hertz_friction_force(size_t c, size_t n, const int32_t* pairs, const double* sep, const double* normal,
                              const double* arc_s, const double* arc_t, const double* seg /*[n][8]*/,
                              const double* radius, const double* youngs_modulus, double youngs_modulus_scalar,
                              const double* poisson_ratio, double poisson_ratio_scalar,
                              const double* velocity_prev /*[n][6]*/,
                              const mhip_hertz_friction_params* params /*[host]*/, double* tang_disp /*[c][3] in/out*/,
                              double* force /*[c][3]*/, void* stats /*[device]*/, mhip_stream_t stream);
/* Carries a per-pair history [c][3] from one contact list to the next.  Each new pair (i, j) receives the row of the old
 * pair whose endpoints, renumbered through new_of_old [n_old] (NULL: the numbering is unchanged; a negative image: the
 * body is gone), are {i, j} -- negated when the orientation came out swapped, the history being "j relative to i" --
 * and +0.0 otherwise.  64-bit pair keys, the radix sort, one binary search per new pair; with new_of_old == NULL the old
 * list must be canonical (sorted by (i, j), i < j, as the broad phase returns it) and nothing is sorted.  An old pair with
 * an endpoint outside [0, n_old) carries nothing.  *carried [host] or NULL = number of new pairs that found their old
 * row.  Synchronises when carried is given or new_of_old is NULL: in the latter case an old list that does not ascend
 * strictly is refused with MHIP_ERR_INVALID_ARGUMENT after the fact (hist_new is then not to be used).  hist_new must
 * not be hist_old. */
int mhip_contact_history_carry(size_t c_old, const int32_t* pairs_old, const double* hist_old,
                               const int32_t* new_of_old /*[n_old] or NULL*/, size_t n_old, size_t c_new,
                               const int32_t* pairs_new, double* hist_new, size_t* carried /*[host] or NULL*/,
                               mhip_stream_t stream);

/* Growth and division of spherocylinders: the body population of the colony loop changes on the device
 * (scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:1033-1080).  Per step, before the AABBs:
 *   mhip_select_dividing  divide_bacteria's mark + partial_sum (:926-935, :243-254): parent_of [<= n] = ascending indices
 *                         i with length[i] > division_length (strict: L == D and NaN never divide), by wavefront
 *                         ballot + prefix sum; *num_born [host] (synchronises).  Birth k becomes row n + k.
 *   mhip_divide_grow_spherocylinders
 *                         subdivide_spherocylinders (:159-210) then grow_bacteria (:905-920) in one pass over [0, n).
 *                         parent_of = the ascending list above.  For birth k of parent i, with t = q_i * zhat (the
 *                         library's rod axis, not the app's q * xhat), cl = 0.5 L - r, s = r + 0.5 cl, off = t s:
 *                         child row n + k = (c + off, q, r, cl + g), parent row i = (c - off, q, r, cl + g); every
 *                         other body gets L + g, g = dt * growth_rate computed once.  box [host] 3 or NULL: the two
 *                         new centres are wrapped into [0, L) as mhip_wrap_rigid does.  The arrays hold n + num_born
 *                         rows; rows beyond are never written.  Every other per-body field of the parent is the
 *                         caller's to copy: mhip_gather_rows(num_born, width, parent_of, src, src + n * width).
 *   mhip_aabb_moved       check_update_neighbor_list (:710-741): *flag [host] = 1 iff some body's min or max corner
 *                         moved since aabb_ref by d with dx*dx + dy*dy + dz*dz >= threshold^2 (left-to-right sum; NaN
 *                         does not fire).  Synchronises.  aabb_ref is the snapshot of the last build: the reference
 *                         accumulates per-step differences instead (:685-705), which is the same in exact arithmetic.
 * Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: dt, growth_rate or division_length negative or not
 * finite, threshold negative or not finite, num_born > n, a null pointer that would be dereferenced. */
int mhip_select_dividing(size_t n, const double* length, double division_length, int32_t* parent_of,
                         size_t* num_born /*[host]*/, mhip_stream_t stream);
int mhip_divide_grow_spherocylinders(size_t n, size_t num_born, const int32_t* parent_of, double dt,
                                     double growth_rate, const double* box /*[host] 3 or NULL*/, double* center,
                                     double* quat, double* radius, double* length, mhip_stream_t stream);
int mhip_aabb_moved(size_t n, const double* aabb, const double* aabb_ref, double threshold, int* flag /*[host]*/,
                    mhip_stream_t stream);

/* Bead-spring chains with thermal noise: the per-step kernels of the chromatin loop
 * (scrap/.../NgpHP1.cpp:3802-3990, SpringsUpdated.cpp, BrownianMotion.cpp) that the contact step lacks.
 *
 * Spring set (a handle, built once): m springs (i, j) = pairs[s] between n bodies, all of one type.
 *   MHIP_SPRING_HOOKEAN  r = rest length r0:  fm = k (L - r0) (1 / L)        (NgpHP1.cpp:1054-1069, its association)
 *   MHIP_SPRING_FENE     r = r_max:           fm = k / (1 - q q), q = L / r_max
 *     the force -grad U of U = -1/2 k r_max^2 ln(1 - (L / r_max)^2) (the potential HP1.cpp:3323-3333 weighs): attractive.
 *     NgpHP1.cpp:1105-1122 applies the opposite sign; this library does not.  A spring with L >= r_max
 *     (or L NaN) has no force: its term is NaN and it is counted in *overstretched.
 *   MHIP_SPRING_FENEWCA  r = r_max:           the Kremer-Grest bond; fm and its statistics: mundy_hip_bending.h
 *   with d = x_j - x_i, L = sqrt(d.d) (right fold), body i receives +fm d and body j -fm d.
 * k [m] / r [m] per spring [host], or NULL: then the scalar stands for every spring.  pairs [m][2] int32 [host].
 * create copies them, refuses (MHIP_ERR_INVALID_ARGUMENT, before any HIP call) an index outside [0, n), a spring from a
 * body to itself, k < 0, r0 < 0, r_max <= 0 and anything not finite, builds the body -> spring incidence on the device
 * and synchronises `stream`.
 * force: force [n][3] is written for every body (no atomics on forces): each body adds its spring terms in ascending
 * spring index from +0.0 (a body without springs gets +0.0 exactly); both ends of a spring evaluate d, L and fm d with
 * the same operations, so they receive exactly negated vectors.  *overstretched [device, 1 int] = number of FENE springs
 * without force; *max_length [device, 1 double] = the longest L (+0.0 without springs), order independent. */
#define MHIP_SPRING_HOOKEAN 0
#define MHIP_SPRING_FENE 1
#define MHIP_SPRING_FENEWCA 2
typedef struct mhip_springs* mhip_springs_t;
int mhip_springs_create(mhip_springs_t* handle, size_t n, size_t m, const int32_t* pairs /*[host] m x 2*/, int type,
                        const double* k /*[host] m or NULL*/, double k_scalar, const double* r /*[host] m or NULL*/,
                        double r_scalar, mhip_stream_t stream);
int mhip_springs_force(mhip_springs_t handle, const double* center, double* force, int* overstretched /*[device]*/,
                       double* max_length /*[device]*/, mhip_stream_t stream);
int mhip_springs_destroy(mhip_springs_t handle);
/* Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11; the generator family of the reference's openrand::Philox):
 * out[c] = the four 32-bit words of the bare generator at key (keys[c] lo32, hi32) and counter (counters[c] lo32,
 * counters[c] hi32, block, 0): ten rounds, multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 /
 * 0xBB67AE85.  Random123's known answers hold (counter 0, key 0 -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8).  openrand's
 * own stream (its key and counter layout) is not reproduced. */
int mhip_philox4x32_10(size_t count, const uint64_t* keys, const uint64_t* counters, uint32_t block,
                       uint32_t* out /*[count][4]*/, mhip_stream_t stream);
/* Brownian velocity, per body: blocks 0 and 1 of Philox at (keys[b], counters[b]) give four normals, of which the
 * first three are used; velocity[b][0..2] += sqrt(2 kt mob_trans[b] / dt) z (D = kT m_t, BrownianMotion.cpp:571,
 * SpringsUpdated.cpp:578; NgpHP1.cpp:2157-2181 writes sqrt(sqrt(6 pi mu) r / dt)); counters[b] += 1.
 * Uniform -> normal, per block of words (w0, w1, w2, w3):
 *   m = (w0 << 21) | (w1 >> 11), m' = (w2 << 21) | (w3 >> 11)   (53-bit integers)
 *   u1 = (m + 1) 2^-53 in (0, 1], u2 = m' 2^-53 in [0, 1)
 *   z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = sqrt(-2 ln u1) sin(2 pi u2), 2 pi = 6.283185307179586
 * Refused before any HIP call: kt negative or not finite, dt <= 0 or not finite. */
int mhip_brownian_velocity(size_t n, const uint64_t* keys, uint64_t* counters /*in/out*/, double kt, double dt,
                           const double* mob_trans, double* velocity /*[n][6]*/, mhip_stream_t stream);
/* Dry drag of a per-body force: velocity[b] = (mob_trans[b] F_b, 0, 0, 0); force [n][3] or NULL (F = 0).  The
 * U_ext = M F_ext of the chromatin step's resolve_collisions (NgpHP1.cpp:1488-1531). */
int mhip_drag_velocity(size_t n, const double* mob_trans, const double* force, double* velocity /*[n][6]*/,
                       mhip_stream_t stream);

/* N-body hydrodynamics as a velocity stage: u_t (+)= sum_s K(x_t - x_s, b_t, a_s) f_s, the long-range velocity the HP1
 * app adds to the dry velocity every step (scrap/.../HP1.cpp:3942-4059 compute_rpy_hydro, :4744-4803 the main loop;
 * kernels: scrap/.../periphery/Periphery.hpp:636-1085).  ns sources (centre [ns][3], radius a [ns], force [ns][3]), nt
 * targets (centre [nt][3], radius b [nt]); the two sets may be the same arrays (beads to beads) or different ones of
 * different sizes.  No self term is added (Periphery.hpp:946, HP1.cpp:4746): the dry drag stays the caller's.
 * With d = x_t - x_s, r2 = (dx dx + dy dy) + dz dz, f.d = (fx dx + fy dy) + fz dz, every product and sum associated
 * as the reference writes it (left to right), no contraction:
 *   MHIP_HYDRO_STOKES  (apply_stokes_kernel, Periphery.hpp:719-743)  scale = 1.0 / (8.0 * M_PI * viscosity) [host]
 *     rinv = r2 < 1e-12 ? 0 : quake_inv_sqrt(r2);  rinv3 = rinv rinv rinv
 *     u += (scale rinv3) (r2 f + d (f.d))                                       radii are not read (may be NULL)
 *   MHIP_HYDRO_RPY     (apply_rpy_kernel, :893-938)  the same scale and rinv; rinv5 = rinv rinv rinv3
 *     c = f rinv3 - (3 (f.d) rinv5) d;   v = scale (f rinv + d ((f.d) rinv3) + ((1/3) a a) c)
 *     u += v + ((1/6) b b) ((2 scale) c)
 *   MHIP_HYDRO_RPYC    (apply_rpyc_kernel, :1000-1081; the app's default, HP1.cpp:5241, and the accurate kind)
 *     r = sqrt(r2) (exact), r3 = r r2, rinv = r2 < 1e-12 ? 0 : 1.0 / r, h = d rinv, f.h = (fx hx + fy hy) + fz hz
 *     inv_pi = 1.0 / 3.14159265358979323846, inv_mu = 1.0 / viscosity
 *     a + b < r           far:  q = (a a + b b) rinv rinv,  s = (1/8) inv_pi inv_mu rinv
 *                               u += (s (1 + q (1/3))) f + (s (1 - q)) ((f.h) h)
 *     |a - b| < r, a > 1e-12 and b > 1e-12   overlapping:  s = (1/6) inv_pi inv_mu / (a b), e = (a - b)(a - b)
 *                               t1 = s (16 r3 (a + b) - (e + 3 r2)(e + 3 r2)) (1/32) rinv3
 *                               t2 = s 3 (e - r2) (e - r2) (1/32) rinv3;   u += t1 f + t2 ((f.h) h)
 *     otherwise           local drag: u += ((1/6) inv_pi inv_mu / max(a, b)) f, skipped when r2 < 1e-12
 *   quake_inv_sqrt (:71-82): i = 0x5fe6eb50c7b537a9 - (bits(x) >> 1) on the signed 64-bit pattern (arithmetic shift),
 *     y = double(i), result y (1.5 - ((x / 2) y y)): ONE Newton step, relative error up to 1.75e-3.  It is part of what
 *     STOKES and RPY are in the reference and is restated exactly; RPYC is the accurate kind.
 * Summation order, a function of ns alone (not of nt, of which targets share a workgroup, of the grid or the device):
 *   the sources are cut into consecutive chunks of MHIP_HYDRO_CHUNK; inside a chunk a target adds its terms in
 *   ascending source index from +0.0, per component; the chunk sums are added in ascending chunk index from +0.0; with
 *   accumulate != 0 that total is added to the old value last (otherwise it is stored).  One writer per target, no
 *   floating-point atomics: two calls give the same bits, and a target evaluated alone gives the bits it has in any
 *   larger target set.
 * velocity row t starts at velocity + t * velocity_stride; velocity_stride = 3, or 6 for the [n][6] rows
 * mhip_drag_velocity writes (the last three entries of a row are not touched).
 * The handle owns the grow-only buffer of the chunk sums ([chunk][target][3]) that a call uses when the target tiles
 * alone would not fill the chip; nothing is allocated once it is warm.  One call at a time per handle.
 * mhip_hydro_set_path (tests and timing): MHIP_HYDRO_PATH_IN_LANE (a lane walks all chunks), MHIP_HYDRO_PATH_PARTIAL
 * (chunk sums through the buffer, ordered second pass) instead of the launch rule's choice; the bits are the same.
 * mhip_hydro_last_path: the shape the last call took.
 * Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: an unknown kind, a viscosity that is not finite or <= 0,
 * a stride other than 3 or 6, a null array with a non-zero count (radii may be NULL for STOKES).  ns == 0 writes +0.0
 * (accumulate: leaves velocity alone); nt == 0 does nothing.
 * mhip_hydro_add_velocity: velocity[b][0..2] += u_hydro[b][0..2] (u_hydro [n][3]): a stored hydrodynamic velocity
 * into the rows of U_ext. */
#define MHIP_HYDRO_STOKES 0
#define MHIP_HYDRO_RPY 1
#define MHIP_HYDRO_RPYC 2
#define MHIP_HYDRO_CHUNK 1024
#define MHIP_HYDRO_PATH_AUTO 0
#define MHIP_HYDRO_PATH_IN_LANE 1
#define MHIP_HYDRO_PATH_PARTIAL 2
typedef struct mhip_hydro* mhip_hydro_t;
int mhip_hydro_create(mhip_hydro_t* handle);
int mhip_hydro_destroy(mhip_hydro_t handle);
int mhip_hydro_set_path(mhip_hydro_t handle, int path);
int mhip_hydro_last_path(mhip_hydro_t handle, int* path /*[host]*/);
int mhip_hydro_velocity(mhip_hydro_t handle, int kind, double viscosity, size_t ns, const double* source_center,
                        const double* source_radius, const double* source_force, size_t nt,
                        const double* target_center, const double* target_radius, double* velocity,
                        int velocity_stride, int accumulate, mhip_stream_t stream);
int mhip_hydro_add_velocity(size_t n, const double* u_hydro /*[n][3]*/, double* velocity, int velocity_stride,
                            mhip_stream_t stream);

/* Crosslinkers that bind and unbind: the kinetic Monte Carlo stage of the HP1 app (scrap/.../HP1.cpp:4728-4739 in the
 * step; :3264-3438 rates, :3440-3594 sampling, :3597-3748 state changes; NgpHP1.cpp:1830-2137 the same over a
 * per-crosslinker list of bind sites), which the reference runs serially on the host in an STK modification cycle.
 * m crosslinkers over n bodies.  Crosslinker c has a fixed left head at body left[c] and a right head at right[c];
 * right[c] == left[c] means singly bound (as the reference represents it).  Several crosslinkers may bind one site.
 * While doubly bound, c is the spring (left[c], right[c]) of mhip_springs_force, type / k / r as there (the library's
 * FENE sign).  DESIGN.md 5f states the model and its deviations.
 *   binding rate of a singly bound c to site s, d = |x_s - x_left| (right-fold norm), inv_kt = 1 / kt:
 *     HOOKEAN  A exp(-0.5 inv_kt k (d - r0) (d - r0))                      (HP1.cpp:3320, its association)
 *     FENE     d < r_max: A pow(1 - (d / r_max) (d / r_max), 0.5 inv_kt k r_max r_max), else 0   (:3332-3334)
 *     s == left[c] is skipped (:3298-3306); d > capture_radius has rate 0 exactly, whatever the candidate list holds
 *   one uniform per crosslinker and step: u = ((w0 << 21) | (w1 >> 11)) 2^-53 from block 0 of Philox at
 *     (keys[c], counters[c]); counters[c] += 1 whatever the state (:3487-3491, :3560-3565)
 *   singly bound: z_tot = sum of dt rate_s over the candidate row of left[c], left to right from +0.0; binds iff
 *     u < 1 - exp(-z_tot), to the first site whose running sum of (1 - exp(-z_tot)) dt / z_tot rate_s exceeds u
 *     (:3504-3527); z_tot == 0 never binds
 *   doubly bound: unbinds iff u < 1 - exp(-(dt k_off)) (what :3554-3573 reduces to); then right[c] = left[c]
 *   both populations are sampled from the state at the start of the step (:3757-3764).
 * create [host arrays; right NULL = all singly bound; is_site [n] bytes, NULL = every body is a bind site] refuses
 *   (MHIP_ERR_INVALID_ARGUMENT, before any HIP call) an index outside [0, n), a right head that is neither left[c] nor a
 *   bind site, an unknown type, k < 0, r0 < 0, r_max <= 0, bind_rate (A) < 0, unbind_rate (k_off) < 0, kt <= 0,
 *   capture_radius <= 0 and anything not finite; it builds both body -> crosslinker incidences on the device and
 *   synchronises `stream`.
 * set_candidates: the bind sites each body's crosslinkers may reach, as the CSR (row_ptr [n + 1], col [num_entries]) of a
 *   neighbour search that lists at least every site within capture_radius (mhip_broadphase_get_pairs); copied, and
 *   every row sorted by ids[col] (int64 [n]; NULL = by col) ONCE here: the order a crosslinker walks its candidates in
 *   (the reference walks its connected linkers, :3473, :3510).  With ids that survive a renumbering of the bodies, a
 *   step is bit-identical after it.
 * kmc_step: one step of the above at the positions `center`; events [device, 2 ints] = (binds, unbinds) of this step
 *   (the perform_state_change passes :3597-3748 without a modification cycle); the incidence of the right ends is
 *   rebuilt on the device.  z_total [m] (optional) receives z_tot of every singly bound crosslinker (0 for a doubly
 *   bound one): what a test compares the rates through.  MHIP_ERR_RUNTIME without candidates.  No synchronisation.
 * force: every doubly bound crosslinker as its spring; each body adds its terms in ascending crosslinker index from
 *   +0.0 (no atomics on forces; the two ends receive exactly negated vectors) and the sum is written to force [n][3]
 *   (accumulate = 0) or added to it (accumulate = 1).  *overstretched / *max_length [device] as mhip_springs_force.
 *   (compute_hookean_spring_forces / compute_fene_spring_forces over the doubly bound part, :4736-4739)
 * get_state / set_state: left and right [m] int32 device arrays out of / into the handle (get: NULL skips; set: left
 *   NULL = unchanged; indices are not checked), the incidences rebuilt.
 * renumber: the bodies were permuted; new_of_old [n] int32 = the new index of every old body.  Crosslinker indices do
 *   not change.  The candidates are dropped (set_candidates again). */
typedef struct mhip_crosslinkers* mhip_crosslinkers_t;
int mhip_crosslinkers_create(mhip_crosslinkers_t* handle, size_t n, size_t m, const int32_t* left /*[host] m*/,
                             const int32_t* right /*[host] m or NULL*/, const unsigned char* is_site /*[host] n or NULL*/,
                             int type, double k, double r, double bind_rate, double unbind_rate, double kt,
                             double capture_radius, mhip_stream_t stream);
int mhip_crosslinkers_set_candidates(mhip_crosslinkers_t handle, const int32_t* row_ptr, const int32_t* col,
                                     size_t num_entries, const int64_t* ids, mhip_stream_t stream);
int mhip_crosslinkers_kmc_step(mhip_crosslinkers_t handle, const double* center, double dt, const uint64_t* keys,
                               uint64_t* counters /*in/out*/, int* events /*[device] 2*/,
                               double* z_total /*[device] m or NULL*/, mhip_stream_t stream);
int mhip_crosslinkers_force(mhip_crosslinkers_t handle, const double* center, double* force, int accumulate,
                            int* overstretched /*[device]*/, double* max_length /*[device]*/, mhip_stream_t stream);
int mhip_crosslinkers_get_state(mhip_crosslinkers_t handle, int32_t* left, int32_t* right, mhip_stream_t stream);
int mhip_crosslinkers_set_state(mhip_crosslinkers_t handle, const int32_t* left, const int32_t* right,
                                mhip_stream_t stream);
int mhip_crosslinkers_renumber(mhip_crosslinkers_t handle, const int32_t* new_of_old, mhip_stream_t stream);
int mhip_crosslinkers_destroy(mhip_crosslinkers_t handle);

/* The nuclear periphery of the HP1 app: a wall that confines every bead in a sphere or an ellipsoid
 * (scrap/.../HP1.cpp:4063-4284; on the device NgpHP1.cpp:2409-2527).  One linear spring of constant k per bead that
 * touches the wall, along the wall's inward normal; in the reference's association:
 *   MHIP_PERIPHERY_SPHERE (HP1.cpp:4208-4238), R = radii[0], x = c - center:
 *     nrm = sqrt(x0 x0 + (x1 x1 + x2 x2)), ssd = R - nrm - r; where ssd < 0: inward = (-x) (1 / nrm) and
 *     F_k = F_k - (k inward_k) ssd.  With center = 0 this is the reference bit for bit.
 *   MHIP_PERIPHERY_ELLIPSOID (NgpHP1.cpp:2444-2527), semi-axes radii = (a, b, c), orientation quat (w, x, y, z):
 *     coarse filter: the level set (b0 b0 inv_a2 + b1 b1 inv_b2 + b2 b2 inv_c2) - 1, inv_a2 = 1 / (a a), at the eight
 *     corners c -/+ r of the bead's box in the body frame conjugate(q) (corner - center); all eight < 0: no force.
 *     Otherwise y = conjugate(q) (c - center) and the exact signed distance sd (negative inside), closest point and
 *     outward unit normal n of the S-E class of mhip_contact_mixed (closed form, csrc/segment_ellipsoid.hpp):
 *     ssd = -sd - r; where ssd < 0: pn = -(q n) and F_k = F_k - (k pn_k) ssd.  The reference calls a shared-normal
 *     distance that its tree does not define; its nearest existing routine (PointEllipsoid.hpp:94-135) is good to 1e-4.
 *     A bead that fails the filter must not sit on the ellipsoid's medial set (the closest point is not unique there);
 *     a bead radius below the smallest semi-axis keeps every such bead away from it.
 *   MHIP_PERIPHERY_ELLIPSOID_FAST (HP1.cpp:4148-4206), x = c - center, no orientation (quat must be the identity):
 *     g = (x0 x0 inv_a2 + x1 x1 inv_b2 + x2 x2 inv_c2) - 1 with inv_a2 = 1 / ((a - r) (a - r)); where g > 0:
 *     F_k = F_k - k (2 x_k inv_k2).
 *   The spherical "fast approximate" variant (HP1.cpp:4240-4264) moves positions and is not built.
 * Precondition on the caller, for every shape: each bead radius r is below the smallest periphery radius.  The bead
 * radii are device data and are not checked here (the stepper refuses them on the host).  Without it SPHERE divides by
 * nrm = 0 for a bead with r >= R at the exact centre, and ELLIPSOID_FAST by (a - r) = 0: the force is then not finite.
 * center [n][3], radius [n], force [n][3].  accumulate = 0: force is written, +0.0 for a body without wall contact (a
 * body with contact gets 0.0 - term); accumulate = 1: the term is subtracted from force, which stays untouched where
 * there is no contact.  No atomics on forces.  colliding [device, 1 int, or NULL] = number of bodies with contact;
 * max_overlap [device, 1 double, or NULL] = the largest -ssd (ELLIPSOID_FAST: the largest g), +0.0 without contact,
 * order independent.  Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: an unknown shape, radii <= 0 (SPHERE:
 * radii[0] only), k < 0, a quaternion that is not unit to 1e-12 (|q|^2 - 1), a non-identity quat with ELLIPSOID_FAST,
 * anything not finite. */
#define MHIP_PERIPHERY_SPHERE 0
#define MHIP_PERIPHERY_ELLIPSOID 1
#define MHIP_PERIPHERY_ELLIPSOID_FAST 2
typedef struct mhip_periphery {
  int shape;
  double center[3];
  double quat[4];
  double radii[3];
  double k;
} mhip_periphery;
int mhip_periphery_force(const mhip_periphery* periphery, size_t n, const double* center, const double* radius,
                         double* force, int accumulate, int* colliding /*[device] or NULL*/,
                         double* max_overlap /*[device] or NULL*/, mhip_stream_t stream);

/* Active euchromatin force dipoles of the HP1 app (scrap/.../HP1.cpp:2796-2826, :3770-3853, :4286-4354): m springs
 * (i, j) = pairs[s] between n bodies, each a two-state (0 inactive, 1 active) Poisson process with the rates kon
 * (0 -> 1) and koff (1 -> 0); an active spring pushes its beads apart with a force of magnitude sigma.
 *   uniform: u = (((w0 << 21) | (w1 >> 11)) + 1) 2^-53 in (0, 1] from block 0 of Philox at (keys[s], counter[s]): the
 *     library's own map (openrand's stream is not reproduced), so log(u) is finite
 *   create [host arrays; keys NULL = the spring's index, counters NULL = 0]: every spring inactive,
 *     next_time = -log(u) (1 / kon), counter + 1, elapsed = 0 (:2796-2826); builds the body -> spring incidence on the
 *     device and synchronises `stream`.  Refuses (MHIP_ERR_INVALID_ARGUMENT, before any HIP call) an index outside
 *     [0, n), a spring from a body to itself, kon <= 0, koff <= 0, a key or counter outside [0, 2^63), anything not
 *     finite.
 *   sample: a spring with elapsed >= next_time draws u, flips its state, sets next_time = -log(u) (1 / koff) when it
 *     switched on or -log(u) (1 / kon) when it switched off, elapsed = 0 and counter + 1 (:3798-3816).  A spring that
 *     does not switch draws nothing.  switches [device, 2 ints] = (switched on, switched off) of this call.
 *   force: for a spring in state 1, nvec = x_j - x_i, nsqr = n0 n0 + n1 n1 + n2 n2 (left to right),
 *     t_k = (sigma / sqrt(nsqr)) nvec_k; body i receives -t and body j +t (:4325-4347), the same operations at both
 *     ends, so exactly negated vectors.  Each body adds its terms in ascending spring index from +0.0 (no atomics on
 *     forces); the sum is written to force [n][3] (accumulate = 0: +0.0 for a body without an active spring) or added to
 *     it (accumulate = 1: untouched for such a body).
 *     active [device, 1 int, or NULL] = number of springs in state 1.
 *   advance: elapsed += dt for every spring (:3835-3853); dt < 0 or not finite is refused.
 *   get_state / set_state: state [m] int32, next_time [m], elapsed [m], counters [m] device arrays out of / into the
 *     handle; NULL skips.  Nothing is checked.
 *   renumber: the bodies were permuted; new_of_old [n] int32 = the new index of every old body.  Spring indices, states
 *     and timers do not change; the incidence is rebuilt. */
typedef struct mhip_active_springs* mhip_active_springs_t;
int mhip_active_springs_create(mhip_active_springs_t* handle, size_t n, size_t m, const int32_t* pairs /*[host] m x 2*/,
                               double sigma, double kon, double koff, const uint64_t* keys /*[host] m or NULL*/,
                               const uint64_t* counters /*[host] m or NULL*/, mhip_stream_t stream);
int mhip_active_springs_sample(mhip_active_springs_t handle, int* switches /*[device] 2*/, mhip_stream_t stream);
int mhip_active_springs_force(mhip_active_springs_t handle, const double* center, double* force, int accumulate,
                              int* active /*[device] or NULL*/, mhip_stream_t stream);
int mhip_active_springs_advance(mhip_active_springs_t handle, double dt, mhip_stream_t stream);
int mhip_active_springs_get_state(mhip_active_springs_t handle, int32_t* state, double* next_time, double* elapsed,
                                  uint64_t* counters, mhip_stream_t stream);
int mhip_active_springs_set_state(mhip_active_springs_t handle, const int32_t* state, const double* next_time,
                                  const double* elapsed, const uint64_t* counters, mhip_stream_t stream);
int mhip_active_springs_renumber(mhip_active_springs_t handle, const int32_t* new_of_old, mhip_stream_t stream);
int mhip_active_springs_destroy(mhip_active_springs_t handle);

/* Centerline-twist (discrete Kirchhoff rod) elastic filaments: the rod forces of the reference's sperm apps
 * (scrap/parameter_interface/alens/tests/performance_tests/CollidingOverdampedFrictionalSperm.cpp; the same text in
 * CollidingFrictionalSperm.cpp, CollidingSperm.cpp, NonInteractingSperm.cpp and scrap/Sperm.cpp).  DESIGN.md 5j.
 * F filaments; filament f owns the contiguous nodes node_ptr[f] .. node_ptr[f + 1] - 1 (at least 2), N nodes in all.
 * Edge e joins the nodes e and e + 1 of one filament and is indexed by its left node (the slot of a filament's last node
 * is unused and stays +0.0); element i is (i - 1, i, i + 1) around an interior node i.  All state lives in the handle:
 *   per node   center [N][3], twist [N], velocity [N][3], twist_velocity [N], force [N][3], twist_torque [N],
 *              radius [N], rest_curvature [N][3], arclength [N], curvature [N][3] (interior nodes; +0.0 elsewhere)
 *   per edge   tangent [N][3], orientation [N][4] (w, x, y, z), length [N], binormal [N][3], each kept twice: new and old
 *              (the reference's StateNP1 / StateN)
 *   per filament  phase [F] of the rest-curvature wave; the caller supplies it (the reference draws it from OpenRAND,
 *              :1132-1133, whose stream this library does not reproduce); NULL = 0
 * Arithmetic: dot(a, b) = a0 b0 + (a1 b1 + a2 b2), |a| = sqrt(dot(a, a)); v /= s divides componentwise and v / s
 * multiplies by 1 / s (mundy_math/impl/VectorImpl.hpp:240-267); quaternion product and q * v as everywhere in this
 * library (q (0, v) conjugate(q) / |q|^2); products and sums left to right as written; sin and cos are the library's
 * fixed IEEE sequence (the oracle's shared_sincos).
 *
 * create  [host arrays node_ptr [F + 1] int32, radius [N], rest_curvature [N][3], arclength [N], phase [F] or NULL]
 *   copies them and synchronises `stream`; every later call of the handle runs on that stream.  Refused with
 *   MHIP_ERR_INVALID_ARGUMENT before any HIP call: a null handle / params / node_ptr, node_ptr[0] != 0, a node_ptr that
 *   is not monotone, a filament of fewer than 2 nodes, rest_length <= 0, viscosity <= 0, poisson_ratio <= -1,
 *   youngs_modulus < 0, a radius <= 0, anything not finite.
 * set_state  [device arrays center [N][3], twist [N], edge_orientation [N][4]] copies them, computes every edge's
 *   tangent and length from the centres (t = (x[e+1] - x[e]) /= l, :1053-1055) and zeroes velocity, twist_velocity,
 *   force, twist_torque, curvature and binormal; old = new.  The initial triad of :1057-1068 is the caller's (the
 *   reference builds it on the host as well).
 * advance  the head of the time loop, :1999-2010, one kernel, per node in this order:
 *     disable_twist (:1832-1838): twist = twist_velocity = 0;  monolayer (:1840-1862): center[0] = velocity[0] = 0
 *     rotate_field_states (:1080-1083): the edge state's new and old copies change places (pointers)
 *     update_generalized_position (:1779-1811): center = center + dt velocity, twist = twist + dt twist_velocity
 *     zero_out_transient_node_fields (:1085-1093): velocity, force, twist_velocity, twist_torque = +0.0
 * force  at the reference's `time` = timestep_index * timestep_size; two kernels, edge_pass then node_pass, which are
 *   entry points of their own as well (the reference's compute_edge_information and its two node functions).
 *   edge pass, compute_edge_information (:1223-1240), per edge e with t_old, q_old its old tangent and orientation:
 *     d = x[e+1] - x[e], l = |d|, t = d /= l;  c = t_old x t, tt = dot(t_old, t)
 *     b = (2 c) / (1 + tt): the binormal of ONE edge at two times, as the reference has it
 *     r = [cos(twist[e] / 2), sin(twist[e] / 2) t_old];  p = [w, (0.5 c) / w], w = sqrt(0.5 (1 + tt))
 *       (quat_from_parallel_transport, mundy_math/Quaternion.hpp:1489-1506)
 *     q = (p r) q_old: the twist rotation is applied again every step and q is not renormalised, as in the reference
 *   node pass, per element i (:1315-1316, :1411-1423; :1166-1167 for the wave), r = radius[i]:
 *     g = conjugate(q[i-1]) q[i], kappa = 2 vec(g), curvature[i] = kappa
 *     rest = rest_curvature[i], with wave != 0 its component 0 replaced by
 *       wave_amplitude sin((wave_number arclength[i] + wave_frequency time) + phase[f])   (not written back)
 *     dk = kappa - rest, I = 0.25 pi r r r r, G = 0.5 E / (1 + nu), il = 1 / l0
 *     m = (-il E I dk0, -il E I dk1, -il 2 G I dk2);  m = q[i-1] * (g.w m + vec(g) x m)
 *     with (t, b, l) of edge i:      fr = (1 / l) ((m x t + (0.5 dot(t, m)) (dot(t, b) t)) - b)    (:1426-1430; the
 *       `- b` sits outside the 0.5 dot(t, m) factor in every one of these apps and is kept: DESIGN.md 5j)
 *     with (t, b, l) of edge i - 1:  fl = (1 / l) (m x t + (0.5 dot(t, m)) (dot(t, b) t - b))      (:1431-1435)
 *     node i + 1 receives +fr, node i -(fr + fl), node i - 1 +fl; twist_torque[i] += dot(t_i, m),
 *     twist_torque[i-1] -= dot(t_{i-1}, m)   (:1437-1458)
 *   per edge e (:1490-1504), r = radius[e+1]: k = E pi r r / l0, fs = (-k (l - l0)) t; node e + 1 receives +fs, node e -fs
 *   Every node gathers its terms, no atomics, from external_force[i] (or +0.0 for NULL) in this order: element i - 1
 *   (+fr), element i (-(fr + fl)), element i + 1 (+fl), edge i - 1 (+fs), edge i (-fs); the twist torque from +0.0:
 *   element i, then element i + 1.  The result does not depend on how nodes map to workgroups.
 *   external_force [device, N x 3, or NULL] is the seam for contact forces reduced to the nodes.
 *   stats [device, 2 doubles]: the largest |l - l0| / l0 over the edges and the largest component of |kappa - rest| over
 *   the elements (+0.0 without any), order independent: what a host chooses dt from.
 * velocity  compute_generalized_velocity (:1772-1775): velocity = ((1 / (6 pi eta)) (1 / r)) force,
 *   twist_velocity = ((1 / (8 pi eta)) ir ir ir) twist_torque, ir = 1 / r.
 * get  device pointers to every field; those of the edge state change places at every advance, so ask again after it.
 * force / edge_pass / node_pass / velocity / advance before set_state: MHIP_ERR_RUNTIME.  Contacts between filament segments:
 * mhip_filament_contacts_* below, whose node forces enter through external_force.  The inertial variants
 * (CollidingFrictionalSperm.cpp:1571-1675, CollidingSperm.cpp): mundy_hip_filament_inertial.h.  Not built: clamp_edge1
 * (:1813-1830), several GPUs. */
typedef struct mhip_filament_params {
  double youngs_modulus, poisson_ratio, rest_length, viscosity;
  double wave_amplitude, wave_number, wave_frequency; /* A, k = 2 pi / wavelength, omega = 2 pi / period (:1110-1111) */
  int wave, disable_twist, monolayer;
} mhip_filament_params;
typedef struct mhip_filament_fields {
  size_t num_nodes, num_filaments;
  double *center, *twist, *velocity, *twist_velocity, *force, *twist_torque;
  double *radius, *rest_curvature, *arclength, *curvature, *phase;
  double *edge_tangent, *edge_orientation, *edge_length, *edge_binormal;
  double *edge_tangent_old, *edge_orientation_old, *edge_length_old, *edge_binormal_old;
} mhip_filament_fields;
typedef struct mhip_filaments* mhip_filaments_t;
int mhip_filaments_create(mhip_filaments_t* handle, size_t num_filaments, const int32_t* node_ptr /*[host] F + 1*/,
                          const double* radius /*[host] N*/, const double* rest_curvature /*[host] N x 3*/,
                          const double* arclength /*[host] N*/, const double* phase /*[host] F or NULL*/,
                          const mhip_filament_params* params, mhip_stream_t stream);
int mhip_filaments_set_state(mhip_filaments_t handle, const double* center, const double* twist,
                             const double* edge_orientation);
int mhip_filaments_advance(mhip_filaments_t handle, double dt);
int mhip_filaments_force(mhip_filaments_t handle, double time, const double* external_force /*[device] N x 3 or NULL*/,
                         double* stats /*[device] 2*/);
int mhip_filaments_edge_pass(mhip_filaments_t handle);
int mhip_filaments_node_pass(mhip_filaments_t handle, double time, const double* external_force, double* stats);
int mhip_filaments_velocity(mhip_filaments_t handle);
int mhip_filaments_get(mhip_filaments_t handle, mhip_filament_fields* fields /*[host]*/);
int mhip_filaments_destroy(mhip_filaments_t handle);

/* Frictional Hertzian contacts between the segments of the filaments above: the contact half of the sperm apps' force
 * stage (compute_hertzian_contact_force_and_torque, CollidingOverdampedFrictionalSperm.cpp:1553-1731, run at :2013-2021
 * after the nodes have moved and before the centerline-twist forces).  DESIGN.md 5k.  FHC = .../evaluate_linker_potentials/
 * kernels/SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp, RED = .../linker_potential_force_reduction/
 * kernels/SpherocylinderSegment.cpp.  Segment i joins the nodes i and i + 1 and is indexed by its left node: every segment
 * array has N rows, the row of a filament's last node is the degenerate record (x_i, x_i, r_i, 0) with a finite box, kept out
 * of the search by its source / target sets.  Arithmetic as for the filaments (right-fold dot and norm).
 *
 * create  filaments: the handle whose nodes collide; it must outlive this one, and every call of this handle runs on
 *   `stream`, which must be the filaments' stream.  node_ptr [host, F + 1]: the filaments' own node_ptr once more (their
 *   handle does not give it back).  segment_radius [host, N] or NULL = the left node's radius.  Builds the source / target
 *   mask and the exclusion lists on the host (segments at most bonded_exclusion apart along one filament never pair:
 *   DestroyBoundNeighbors.cpp:150-170 with the reference's value 1), owns a mhip_broadphase_t, synchronises `stream`.
 *   The reference hard-codes E = 5e5, nu = 0.3, mu = 0.5, density 1, no damping and a history step of 1e-5 whatever dt is
 *   (FHC :406-417); here they are parameters, history_dt < 0 = the dt of the force call.  params->monolayer must be the
 *   filaments' flag.  Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: a null handle / filaments / params /
 *   node_ptr, a node_ptr that is not the filaments', mu, a damping, density or skin < 0, youngs_modulus <= 0,
 *   poisson_ratio outside (0, 1), bonded_exclusion < 1, a radius <= 0, anything not finite.
 * save_velocity  velocity_prev [N][3] = the filaments' velocity, with monolayer its component 0 = +0.0: the StateN
 *   velocities the force reads (FHC :388; apply_monolayer runs before rotate_field_states, :1999-2003).  To be called
 *   before mhip_filaments_advance, which zeroes the field.
 * update  the segment view: seg [N][8] = (x_i, x_{i+1}, r_i, 0) and the buffered boxes aabb [N][6] = (min - r - skin,
 *   max + r + skin) (.../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161).  On the first call, or when a box corner
 *   has moved since the last build by d with |d|^2 >= skin^2 / 4 (:1565-1607; mhip_aabb_moved against the snapshot of the
 *   last build, threshold 0.5 skin), the list is rebuilt (:1612-1717): MHIP_SEARCH_AABB on these boxes, buffer 0,
 *   symmetric = 0, the exclusions above; tang_disp is carried (mhip_contact_history_carry), the segment -> linker
 *   incidence is built, sep / force / share become +0.0.  *rebuilt [host] tells.  Synchronises.
 * force  per linker (i, j), one kernel: the centreline closest points cp_i, cp_j and their distance
 *   (distance_sq_between_line_segments, ...SpherocylinderSegmentSpherocylinderSegmentLinker.cpp:204-237), sep = distance -
 *   (r_i + r_j), n = (cp_j - cp_i) (1 / distance).  sep > 0: tang_disp, force and share rows are +0.0 (written only where
 *   they are not +0.0 already).  Otherwise, for each side with end nodes 0, 1 (FHC :357-380):
 *     rv = v1 - v0, lc = cp - x0, L = |x1 - x0|, iL = 1 / L, t = (x1 - x0) iL, v from velocity_prev
 *     v_cp = (v0 + (dot(lc, rv) t) iL) + (dot(lc, t) (rv - dot(t, rv) t)) iL
 *   rel = v_cp,j - v_cp,i and the law of mhip_hertz_friction_force (one device function) give tang_disp[c] and force[c],
 *   the force F on segment i.  share[c][side] (RED :206-212), with Fs = +F for side 0 (segment i) and -F for side 1:
 *     share = (dot(lc, t) (Fs + dot(t, Fs) t)) iL - (dot(t, Fs) lc) iL      (the `+` is the reference's and is kept)
 *   Reduction to the nodes (RED :213-221), a gather without atomics: for segment e, a0[e] = +0.0 + sum of (Fs - share) and
 *   a1[e] = +0.0 + sum of share over its linkers in ascending list order; node_force[i] = ((external_force[i] or +0.0) +
 *   a0[i]) + a1[i - 1], a term whose segment does not exist left out.  The twist torque of a contact is ignored, as in the
 *   reference (RED :199).  stats [device, 16 bytes] as for mhip_hertz_friction_force: a double max(0, -sep) over the
 *   contact branch, a uint64 count of capped contacts.  A pair index outside the segments gives NaN rows and is never
 *   dereferenced.  node_force is what mhip_filaments_force takes as external_force.
 *   segment_view (the first half of update), linker_pass and reduce (the two halves of force) are entry points of their
 *   own as well, as the filaments' edge_pass and node_pass are.
 * set_history  plants tang_disp rows: the given canonical list (pairs [c][2], tang_disp [c][3], device) is carried into the
 *   current list; before the first update it is kept and carried into the first list (a restart).
 * get  device pointers (they move at a rebuild: ask again after an update that rebuilt) and counts.
 * force before save_velocity or update: MHIP_ERR_RUNTIME, the message names the missing call.
 * The frictionless ...HertzianContact kernel: mhip_filament_contacts_set_law of mundy_hip_filament_inertial.h.
 * Not built: periodic cells, several GPUs, a renumbering of nodes, the WCA kernel. */
typedef struct mhip_filament_contact_params {
  double skin, youngs_modulus, poisson_ratio;
  double mu, normal_damping, tangential_damping, density;
  double history_dt;    /* < 0: the dt of the force call */
  int bonded_exclusion; /* >= 1; the reference's value is 1 */
  int monolayer;        /* the filaments' flag */
} mhip_filament_contact_params;
typedef struct mhip_filament_contact_fields {
  size_t num_nodes, num_pairs;
  int32_t* pairs;                       /* [num_pairs][2] */
  double *sep, *tang_disp, *force;      /* [num_pairs], [num_pairs][3], [num_pairs][3] */
  double* share;                        /* [num_pairs][2][3] */
  double *node_force, *seg, *aabb, *velocity_prev; /* [N][3], [N][8], [N][6], [N][3] */
} mhip_filament_contact_fields;
typedef struct mhip_filament_contacts* mhip_filament_contacts_t;
int mhip_filament_contacts_create(mhip_filament_contacts_t* handle, mhip_filaments_t filaments,
                                  const int32_t* node_ptr /*[host] F + 1*/,
                                  const double* segment_radius /*[host] N or NULL*/,
                                  const mhip_filament_contact_params* params, mhip_stream_t stream);
int mhip_filament_contacts_save_velocity(mhip_filament_contacts_t handle);
int mhip_filament_contacts_update(mhip_filament_contacts_t handle, int* rebuilt /*[host]*/);
int mhip_filament_contacts_force(mhip_filament_contacts_t handle, double dt,
                                 const double* external_force /*[device] N x 3 or NULL*/, void* stats /*[device]*/);
int mhip_filament_contacts_segment_view(mhip_filament_contacts_t handle);
int mhip_filament_contacts_linker_pass(mhip_filament_contacts_t handle, double dt, void* stats /*[device]*/);
int mhip_filament_contacts_reduce(mhip_filament_contacts_t handle, const double* external_force);
int mhip_filament_contacts_set_history(mhip_filament_contacts_t handle, size_t c, const int32_t* pairs,
                                       const double* tang_disp);
int mhip_filament_contacts_get(mhip_filament_contacts_t handle, mhip_filament_contact_fields* fields /*[host]*/);
int mhip_filament_contacts_destroy(mhip_filament_contacts_t handle);

/* Mixed shapes (BASELINE configs[4]): kind[n] = 0 sphere, 1 spherocylinder, 2 ellipsoid; shape[n][3] = (r,-,-) /
 * (r,L,-) / (r1,r2,r3); quat is ignored for spheres.  compute_aabb dispatches on kind (compute_aabb.hpp:72-127) and
 * also returns the bounding radii (compute_bounding_radius.hpp:61-93).  contact_mixed bins the pairs by shape class and
 * runs one distance routine per class: S-S, S-R (scrap/.../SphereSpherocylinderLinker.cpp:210-239), R-R, E-E as above;
 * S-E = distance(Point, Ellipsoid) - r (exact by default, see mhip_contact_mixed_set_sphere_ellipsoid_route) and R-E = closest approach of the rod's centreline to the ellipsoid (exact
 * signed point - ellipsoid distance minimised along the centreline, closed form: csrc/segment_ellipsoid.hpp) - r are
 * build extensions (the reference's SphereEllipsoid.hpp / LineSegmentEllipsoid.hpp are empty stubs): parity unpinned.
 * class_counts [host, 6] (optional) = pairs per class in the order SS, SR, SE, RR, RE, EE (synchronises if given). */
int mhip_compute_aabb_mixed(size_t n, const int32_t* kind, const double* center, const double* quat,
                            const double* shape, double* aabb, double* bounding_radius, mhip_stream_t stream);
/* BUILD EXTENSION (SURVEY a7's flagged option): the same with the TIGHT CONSERVATIVE box for the ellipsoids (half extent
 * along lab axis k = sqrt(sum_j (r_j (q e_j)[k])^2)).  The reference's box (centre -/+ q*radii, compute_aabb.hpp:82-103)
 * is exact only for axis-aligned orientations: for a general rotation an extent can collapse towards zero, and a
 * neighbour search on those boxes silently misses overlapping ellipsoid pairs.  Spheres and rods are unchanged. */
int mhip_compute_aabb_mixed_conservative(size_t n, const int32_t* kind, const double* center, const double* quat,
                                         const double* shape, double* aabb, double* bounding_radius,
                                         mhip_stream_t stream);
int mhip_contact_mixed(size_t c, const int32_t* pairs, const int32_t* kind, const double* center, const double* quat,
                       const double* shape, double* sep, double* normal, double* cp1, double* cp2, double* ra,
                       double* rb, size_t* class_counts /*[host]*/, mhip_stream_t stream);
/* BUILD OPTION, labelled wherever it is exposed: on = 1 makes the following mhip_contact_mixed* calls (any thread) run
 * the S-E and E-E minimisation classes from a build with floating-point contraction ON (fused multiply-adds):
 * their results then agree with the default build -- which is bit-identical to the CPU oracle -- only to the
 * reference's own tolerance for ellipsoid distances, 1e-4 (UnitTestEllipsoidEllipsoid.cpp:53), on >= 99.5 % of pairs
 * (tests/test_gpu_mixed.py).  The closed-form classes (S-S, S-R, R-R, R-E) are not affected.  Default 0. */
int mhip_contact_mixed_set_contraction(int on);
/* S-E (a build extension: the reference's SphereEllipsoid.hpp is an empty stub) = signed distance of the sphere's centre
 * to the ellipsoid, minus the radius.  route 0 (default): the exact distance in closed form (csrc/segment_ellipsoid.hpp);
 * route 1: distance(Point, Ellipsoid) as the reference computes it (PointEllipsoid.hpp:94-135, nine-start L-BFGS over
 * the surface normal).  ROUTE 1 IS THE REFERENCE-ROUTINE ROUTE, the one SURVEY 8f.4 prescribes for S-E; route 0 solves
 * the same problem (closest surface point in the Euclidean sense, signed by inside / outside) exactly and matches
 * route 1 to that routine's own 1e-4 wherever its minimiser reaches the global minimum.  Where the two differ by more
 * than 1e-4 (the nine starts stall in a local minimum: needles, flakes, points near a long axis; < 0.5 % of the pairs
 * of the mixed packing) the tests certify PAIR BY PAIR that route 0's foot point is the closer one and satisfies the
 * optimality conditions (tests/test_gpu_mixed.py, tests/test_oracle_ellipsoid_kat.py:
 * certify_sphere_ellipsoid_disagreements).  Applies to the following mhip_contact_mixed* calls of any thread. */
int mhip_contact_mixed_set_sphere_ellipsoid_route(int route);
/* objective evaluations the L-BFGS classes (S-E, E-E; the middle word was R-E's, closed-form since round 3: 0)
 * needed in the last mhip_contact_mixed* call of this host thread, and in the last mhip_distance_ellipsoid_* / mhip_contact_ellipsoids call: these kernels are fp64-vector bound
 * (about 2.3 * 10^3 fp64 instructions per evaluation), so evaluations x that / time is their roofline figure */
int mhip_contact_mixed_last_evaluations(unsigned long long evaluations[3] /*[host]*/, mhip_stream_t stream);
int mhip_ellipsoid_last_evaluations(unsigned long long* evaluations /*[host]*/, mhip_stream_t stream);
/* periodic box [host: 3 edge lengths]: body j at the nearest lattice image of its centre, c_j' = c_i + sep(c_i, c_j) */
int mhip_contact_mixed_periodic(size_t c, const int32_t* pairs, const int32_t* kind, const double* center,
                                const double* quat, const double* shape, const double* box /*[host] 3*/, double* sep,
                                double* normal, double* cp1, double* cp2, double* ra, double* rb,
                                size_t* class_counts /*[host]*/, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Broad phase (seam S3).
 * Replaces: stk::search::coarse_search(domain, range, MORTON_LBVH, comm, results, exec, symmetry) +
 *           SearchFilter::apply / filter_view compaction     mundy/mesh/src/mundy_mesh/GenNeighborLinkers.hpp:650-664,
 *           :141-183; the rebuild rule :603-615; scrap: ArborX BVH query scrap/lcp_spheres/NgpLcp.cpp:297-330.
 * Predicate (defined here; the reference's is third party): MHIP_SEARCH_SPHERES = bounding spheres
 * (centre, bounding_radius + buffer), closed test d^2 <= (Ri + Rj)^2; MHIP_SEARCH_AABB = aabb grown by buffer on every
 * face, closed interval test of geom::intersects (AABB.hpp:420-431).  Results are canonical: sorted by (i, j);
 * symmetric = 0 gives unique i < j pairs, 1 gives both orientations; i == j only with include_self.
 * Search method (GenNeighborLinks::set_search_method, :443-447; the reference's default is stk::search::MORTON_LBVH):
 * the uniform cell grid (cell edge = twice the largest reach; fastest when bodies are of similar size), a linear BVH over
 * 63-bit Morton keys (adapts to each body's size: size-disperse systems), or AUTO = LBVH when the largest reach exceeds
 * twice the mean reach.  Periodic systems: the tree holds every volume translated into the primary cell and is walked
 * once per image of the query that can meet it; a cell with an edge below four times the largest reach goes to the grid
 * whatever was asked for (mhip_broadphase_method_used tells).  Same lists either way.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { MHIP_SEARCH_SPHERES = 0, MHIP_SEARCH_AABB = 1 };
enum { MHIP_SEARCH_METHOD_AUTO = 0, MHIP_SEARCH_METHOD_GRID = 1, MHIP_SEARCH_METHOD_MORTON_LBVH = 2 };

typedef struct mhip_broadphase* mhip_broadphase_t;

typedef struct {
  int search_kind; /* MHIP_SEARCH_* */
  int symmetric;   /* 0: i<j ; 1: i!=j both orders */
  double buffer;   /* search buffer added to every volume */
  int periodic;    /* 0 free space, 1 orthorhombic periodic box [0,box), 2 triclinic unit cell `cell` */
  double box[3];
  int method;       /* MHIP_SEARCH_METHOD_* (0 = AUTO) */
  int include_self; /* 0 = ExcludeSelfInteractions (GenNeighborLinkers.hpp:185-200), 1 = (i, i) is a result */
  /* periodic == 2: the unit cell of PeriodicMetric (periodicity.hpp:233-332), row-major 3 x 3, lattice vectors as
   * COLUMNS.  A pair is tested at the image PeriodicMetric::sep picks for the centres / box midpoints (minimum image of
   * the fractional coordinates, :304-307).  Grid and tree work in scaled fractional coordinates (the cell becomes an
   * orthorhombic box of the three perpendicular widths of the cell); same lists as the brute-force statement. */
  double cell[9];
} mhip_broadphase_config;

int mhip_broadphase_create(mhip_broadphase_t* handle);
int mhip_broadphase_destroy(mhip_broadphase_t handle);
/* Builds the neighbour list of n bodies; *num_pairs [host] receives the pair count (synchronises, as filter_view's
 * deep_copy of the scan total does, GenNeighborLinkers.hpp:155-156).  Also snapshots the centres for
 * mhip_broadphase_needs_rebuild. */
int mhip_broadphase_build(mhip_broadphase_t handle, const mhip_broadphase_config* config /*[host]*/, size_t n,
                          const double* aabb, const double* center, const double* bounding_radius,
                          size_t* num_pairs /*[host]*/, mhip_stream_t stream);
/* Copies the pair list ([num_pairs][2] int32) and/or the CSR form (row_ptr[n+1], col[num_pairs]); NULL skips. */
int mhip_broadphase_get_pairs(mhip_broadphase_t handle, int32_t* pairs, int32_t* row_ptr, int32_t* col,
                              mhip_stream_t stream);
/* The rest of the seam: who may pair with whom, and results in the reference's vocabulary.
 *   set_sets        acts_on(source_selector, target_selector) (GenNeighborLinkers.hpp:486-507): is_source / is_target
 *                   [n] bytes (NULL = every body); a result (s, t) needs s in the sources and t in the targets -- with
 *                   symmetric = 0 additionally s < t.  The reference's domain and range views are two selections of one
 *                   entity population (specializations_, :626-629), which is what the two masks express.
 *   set_exclusions  search_filters::ExcludeConnectedEntities (:202-236) and the existing-link set kept when duplicate
 *                   links are not allowed (:91-113, :643-648): CSR (ex_ptr [n + 1], ex_idx) of partners a source must
 *                   not be paired with; the ordered pair (s, t) is dropped when t is in the list of s.
 *   set_identities  (stk::mesh::EntityId, owner rank) of every body (:575-584); NULL id = the local index, NULL owner = 0
 * All three copy their arrays into the handle; sets / exclusions invalidate the current list (the next needs_rebuild
 * says yes).  get_ident_pairs returns the list as IdentProcIntersection rows (domain id, domain proc, range id, range
 * proc), any output NULL to skip.  method_used: which structure the last build ran on (MHIP_SEARCH_METHOD_*). */
int mhip_broadphase_set_sets(mhip_broadphase_t handle, size_t n, const unsigned char* is_source,
                             const unsigned char* is_target, mhip_stream_t stream);
int mhip_broadphase_set_exclusions(mhip_broadphase_t handle, size_t n, const int32_t* ex_ptr, const int32_t* ex_idx,
                                   size_t num_entries, mhip_stream_t stream);
int mhip_broadphase_set_identities(mhip_broadphase_t handle, size_t n, const uint64_t* entity_id,
                                   const int32_t* owner_rank, mhip_stream_t stream);
int mhip_broadphase_get_ident_pairs(mhip_broadphase_t handle, uint64_t* source_id, int32_t* source_proc,
                                    uint64_t* target_id, int32_t* target_proc, mhip_stream_t stream);
int mhip_broadphase_method_used(mhip_broadphase_t handle, int* method /*[host]*/);
/* Periodic cells: the predicate tests a pair at the NEAREST image of its centres / box midpoints only -- the minimum
 * image of PeriodicScaledMetric::sep (periodicity.hpp:812-816), as every periodic distance of the reference does.  That
 * finds every overlap as long as the smallest cell edge exceeds four times the largest reach (half extent + buffer) of
 * the bodies; in a smaller cell two volumes can also meet through a second image, and such pairs are NOT reported.
 * *complete [host] = 1 when the last build's cell met the condition (always 1 in free space), 0 otherwise: a caller
 * that needs the multi-image list has to replicate the cell.  No synchronisation (the build has read the figure). */
int mhip_broadphase_minimum_image_complete(mhip_broadphase_t handle, int* complete /*[host]*/);
/* The list in MuNDy's link layout, so that it can be handed to LinkData without the host-serial
 * request_link loop of GenNeighborLinkers.hpp:714-738:
 *   export_coo  one row per link, as the fields LinkCOOData keeps per link entity (LinkMetaData.hpp:102-106): the link's
 *               own id first_link_id + k, MUNDY_LINKED_ENTITY_IDS [P][2] (source, target), MUNDY_LINKED_ENTITY_RANKS
 *               [P][2] (bytes); any output NULL to skip
 *   export_crs  entity -> connected links, as LinkCRSBucketConn keeps it per entity bucket (LinkCRSBucketConn.hpp:
 *               183-191): entities in index order cut into buckets of bucket_capacity (STK's default bucket: 512);
 *               num_connected_links [n]; sparse_connectivity_offsets [num_buckets][capacity + 1], bucket local;
 *               sparse_connectivity [2 P] link ids (a link is connected to both its entities), ascending per entity;
 *               bucket_begin [num_buckets + 1] = where each bucket's connectivity starts in sparse_connectivity */
int mhip_links_export_coo(mhip_broadphase_t handle, uint64_t first_link_id, int source_rank, int target_rank,
                          uint64_t* link_id, uint64_t* linked_entity_ids, unsigned char* linked_entity_ranks,
                          mhip_stream_t stream);
int mhip_links_export_crs(mhip_broadphase_t handle, uint64_t first_link_id, unsigned bucket_capacity,
                          unsigned* num_connected_links, unsigned* sparse_connectivity_offsets,
                          uint64_t* sparse_connectivity, uint64_t* bucket_begin, mhip_stream_t stream);
/* Rebuild rule: *flag [host] = 1 iff any centre moved more than 0.5*buffer since the last build (synchronises). */
int mhip_broadphase_needs_rebuild(mhip_broadphase_t handle, size_t n, const double* center, int* flag /*[host]*/,
                                  mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Convex solver backend (seam S1) -- the static interface of convex::KokkosBackend as a C ABI.
 * Replaces: mundy/math/src/mundy_math/convex.hpp:141-285 (deep_copy, apply/gemv, axpby, wrapped_axpbyz, diff_dot x2,
 *           reduce_max), residual policies :434-496, BBStepStrategy :498-516.  Functors cannot cross a C ABI, so the
 *           four convex spaces (:46-115) and the two residual policies are enums + scalars.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { MHIP_SPACE_UNCONSTRAINED = 0, MHIP_SPACE_LOWER_BOUND = 1, MHIP_SPACE_UPPER_BOUND = 2, MHIP_SPACE_BOUNDED = 3 };
enum { MHIP_RESIDUAL_PROJECTED_DIFF = 0, MHIP_RESIDUAL_PROJECTED_GRADIENT = 1 };

typedef struct {
  int kind; /* MHIP_SPACE_* */
  double lower_bound, upper_bound;
} mhip_space;

typedef struct {
  unsigned max_iters; /* PGDConfig::max_iters, default 1000 (convex.hpp:523) */
  double tol;         /* PGDConfig::tol, default 1e-8 (convex.hpp:524) */
  int residual_kind;  /* MHIP_RESIDUAL_*; default policy is PROJECTED_DIFF (convex.hpp:762-768) */
} mhip_pgd_config;

typedef struct {
  unsigned num_iters; /* completed non-terminal iterations (convex.hpp:664) */
  double residual;
  int converged; /* non-convergence is not an error (convex.hpp:673-675) */
} mhip_solve_result;

int mhip_deep_copy(size_t n, double* dst, const double* src, mhip_stream_t stream);
int mhip_fill(size_t n, double* dst, double value, mhip_stream_t stream);
int mhip_axpby(size_t n, double alpha, const double* x, double beta, double* y, mhip_stream_t stream);
int mhip_wrapped_axpbyz(size_t n, double alpha, const double* x, double beta, const double* y, double* z,
                        const mhip_space* space /*[host]*/, mhip_stream_t stream);
int mhip_diff_dot2(size_t n, const double* x, const double* y, double* result /*[host]*/, mhip_stream_t stream);
int mhip_diff_dot4(size_t n, const double* x1, const double* x2, const double* y1, const double* y2,
                   double* result /*[host]*/, mhip_stream_t stream);
int mhip_residual(size_t n, int residual_kind, const double* x, const double* grad, const mhip_space* space /*[host]*/,
                  double* result /*[host]*/, mhip_stream_t stream);
int mhip_bb_step(size_t n, const double* x_old, const double* g_old, const double* x, const double* g,
                 double* result /*[host]*/, mhip_stream_t stream);
/* y = A x, A row-major n x n (KokkosBlas::gemv "N", convex.hpp:168-174) */
int mhip_gemv(size_t n, const double* A, const double* x, double* y, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Matrix-free contact operator (seam S2):  y = dt * D^T M D x  over a neighbour list.
 * Replaces: sum_collision_force / compute_the_mobility_problem (dry) / compute_rate_of_change_of_sep,
 *           scrap/lcp_spheres/NgpLcp.cpp:442-530; rigid-body torque terms follow the dry local-drag mobility of
 *           scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:808-848 (U = F/(6 pi mu r),
 *           W = T/(8 pi mu r^3)), passed in as per-body scalars.
 * ra, rb, mob_rot may all be NULL (translation only, the sphere app).  The handle keeps views of the caller's
 * arrays (they must outlive it) and owns a body->constraint incidence index, so sums run in a fixed order (bitwise
 * reproducible, no atomics).  Both create calls synchronise `stream`: the pair list is validated on the device (an
 * index outside [0, num_bodies) or a self pair is MHIP_ERR_INVALID_ARGUMENT) and its form read back before the index
 * is laid out.  refresh and everything below up to the solvers is asynchronous.
 * priority [C] or NULL: a locality hint for that index only (never the result beyond summation-order rounding) -- each
 * body lists the contacts with priority < 0 first.  Pass the signed separations: the contacts that overlap at the
 * start of the step are the ones that will carry impulses, and the body sweep of the LCP solver only walks those.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mhip_contact_op* mhip_contact_op_t;

int mhip_contact_op_create(mhip_contact_op_t* handle, size_t num_constraints, size_t num_bodies, const int32_t* pairs,
                           const double* normal, const double* ra, const double* rb, const double* mob_trans,
                           const double* mob_rot, double dt, const double* priority, mhip_stream_t stream);
/* Spherocylinders: the same operator with rod-compressed kinematics.  A rod's contact point lies on its centreline,
 * cp = c + (s - 1/2)(p1 - p0), so each lever arm is one scalar; the sweeps stream (s, t) [16 B per contact] instead of
 * (ra, rb) [48 B] and 32-byte instead of 48-byte half-edge records (-18 % bytes per BBPGD iteration).  arc_s / arc_t
 * [C] and seg [N][8] are the outputs of mhip_contact_spherocylinders / mhip_spherocylinder_segments.  Same operator up
 * to rounding (the arm (s - 1/2) u replaces (p0 + s u) - c). */
int mhip_contact_op_create_rods(mhip_contact_op_t* handle, size_t num_constraints, size_t num_bodies,
                                const int32_t* pairs, const double* normal, const double* arc_s, const double* arc_t,
                                const double* seg, const double* mob_trans, const double* mob_rot, double dt,
                                const double* priority, mhip_stream_t stream);
/* Same pairs, new geometry (a step that reuses the neighbour list): keeps the incidence index and redoes only the
 * half-edge records / rod axes from the new arrays (which replace the ones given at create; mobilities and dt stay).
 * A quarter of the cost of building the operator again.  The order inside a body's list is the one fixed at create. */
int mhip_contact_op_refresh(mhip_contact_op_t handle, const double* normal, const double* ra, const double* rb,
                            mhip_stream_t stream);
int mhip_contact_op_refresh_rods(mhip_contact_op_t handle, const double* normal, const double* arc_s,
                                 const double* arc_t, const double* seg, mhip_stream_t stream);
int mhip_contact_op_destroy(mhip_contact_op_t handle);
/* A destroyed operator leaves its device workspaces in one process-wide spare set that the next create adopts (no
 * allocation in the steady state of a time loop); this frees that set. */
int mhip_release_cached_workspaces(void);
int mhip_contact_op_apply(mhip_contact_op_t handle, const double* x, double* y, mhip_stream_t stream);
/* The body sweep of apply without its constraint sweep: the velocity rows U = M D x of a caller-given x [C] (one
 * non-negative force magnitude per contact: body i receives -x_c n_c, body j +x_c n_c, at the operator's lever arms),
 * read with mhip_contact_op_body_velocity.  Same incidence index and fixed-order double-double sums as apply; a body
 * whose contacts all carry x = 0 gets a zero row.  The rods' angular rows are formed too.
 * Replaces: LinkerPotentialForceReduction (.../linker_potential_force_reduction/kernels/Spherocylinder.cpp:173-207 --
 *           force and torque (cp - x_body) x F summed per body) followed by compute_generalized_velocity
 *           (scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:806-848, dry drag). */
int mhip_contact_op_body_sweep(mhip_contact_op_t handle, const double* x, mhip_stream_t stream);
/* The same sweep for a vector force per contact, force [C][3]: U_b = m_t sum +/-F_c, W_b = m_r sum arm x (+/-F_c) with +
 * on side i and - on side j, over the operator's own incidence index and half-edge arms (spheres, vector arms, rod
 * arms), fixed-order double-double sums.  body_sweep_vector(-x_c n_c) gives the rows of body_sweep(x) bit for bit.  The
 * operator is left as mhip_contact_op_body_sweep leaves it (rod rows hold (U, W x u), omega is filled), so
 * mhip_contact_op_body_velocity reads the result.  Refused while a staged solve is in progress. */
int mhip_contact_op_body_sweep_vector(mhip_contact_op_t handle, const double* force, mhip_stream_t stream);
/* The transpose sweep alone: sep_dot [C] = D^T U of a caller-given velocity [N][6] (U, W) rows,
 *   sep_dot_c = n_c . [(U_j + W_j x rb) - (U_i + W_i x ra)]
 * with the operator's own kinematics (spheres, vector arms, rod arms).  It is apply's constraint sweep (X_APPLY) on the
 * caller's rows with no dt factor, same expressions and rounding: dt * constraint_rate(body_velocity after body_sweep(x))
 * == apply(x) bit for bit, and <x, D^T U> = <D x, U> to rounding.  Rod operators first form (U, W x u) rows in an
 * operator workspace.  Refused while a staged solve is in progress.
 * Replaces: sep += dt D^T U_ext of resolve_collisions (NgpHP1.cpp:1488-1531). */
int mhip_contact_op_constraint_rate(mhip_contact_op_t handle, const double* velocity, double* sep_dot,
                                    mhip_stream_t stream);
/* Per-kernel timing of the fused solver (measurement support, no effect on results): when enabled,
 * mhip_bbpgd_solve_contact brackets the k_body / k_constraint launches of every 8th iteration with HIP events on
 * `stream` and accumulates their device durations.  get_profile returns the totals in milliseconds and the number of timed iterations
 * (sampled launches of each kernel) since profiling was enabled.  All out pointers [host]. */
/* sizes the operator was created with (either pointer may be NULL) */
int mhip_contact_op_sizes(mhip_contact_op_t handle, size_t* num_constraints, size_t* num_bodies);
/* How the two sweeps are laid out on the chip -- time only, never results: every sum that reaches an iterate is a
 * double-double pair rounded once, so any mapping gives the same bits (tests/test_gpu_convex.py checks exactly that).
 *   xcd_tile        consecutive 256-item tiles handed to one XCD (8 XCDs with private L2s; 0 = identity mapping,
 *                   default 32); -1 keeps the current value
 *   lanes_per_body  lanes that share one body's contact list in the body sweep: 2, 4, 8 or 16 (default by mean
 *                   degree); -1 keeps the current value */
int mhip_contact_op_set_work_mapping(mhip_contact_op_t handle, int xcd_tile, int lanes_per_body);
/* Cold tier, TIME ONLY (the iterates are the same bits): where the body sweep of a tiered solve takes its drift bound
 * from -- 1: the difference of a body's new row and its row of the previous iterate (48 more bytes read per body: free
 * while both row tables sit in the Infinity Cache); 2: the change of the force accumulated in registers beside the
 * sums (no extra read; rods and spheres with the default lane layout only); 0 (default): by size -- rows up to
 * 1.75 * 10^6 bodies, registers beyond. */
int mhip_contact_op_set_drift_source(mhip_contact_op_t op, int source);
/* *source [host] = the form a tiered solve on this operator would take now (1 or 2) */
int mhip_contact_op_get_drift_source(mhip_contact_op_t op, int* source /*[host]*/);
/* Cold tier of mhip_bbpgd_solve_contact (time only, never results).  Two thirds of the contacts of a packing are inactive
 * (x = 0, g > 0) for most of a solve; such a contact adds exact zeros to every sum of an iteration, and how far its
 * gradient can have moved is bounded by its two bodies' accumulated velocity changes.  From the first convergence poll on
 * the solve therefore renumbers the contacts hot-first and leaves the cold tail alone (a body whose accumulated change
 * reaches the smallest bound of its sleeping contacts wakes those that have reached theirs; a woken contact is evaluated
 * like any other again).  Same
 * iterates, bit for bit, and the same iteration count as with tiering off (every sum is a double-double pair rounded
 * once, so the partition of the contacts does not reach the sums).  LCP solves (any of the three operator forms) with at
 * least 1.5 million contacts (below that the solve is launch-bound and the bookkeeping costs more than the shorter
 * sweep saves), in the fused solve and -- for the contacts between two bodies the rank owns -- in the staged /
 * distributed one; mode 0 = off, 1 = on (default), 2 = test hook: leave the tiers mid-solve, as the solve does before a BB
 * step outside [0, finite], 3 = test hook: no minimum size (2 has none either).
 * tier_stats: iterations that ran tiered, mean share of hot contacts over them, renumberings, contacts woken. */
int mhip_contact_op_set_tiering(mhip_contact_op_t handle, int mode);
int mhip_contact_op_tier_stats(mhip_contact_op_t handle, size_t* tiered_iterations, double* mean_hot_fraction,
                               size_t* renumberings, size_t* wakeups);
int mhip_contact_op_set_profiling(mhip_contact_op_t handle, int enable);
int mhip_contact_op_get_profile(mhip_contact_op_t handle, double* body_ms, double* constraint_ms, size_t* iterations);
/* body velocities [num_bodies][6] = (U xyz, W xyz) from the last apply / solve iterate (valid in stream order after
 * that call; for a partitioned operator only the owned rows are meaningful) */
int mhip_contact_op_body_velocity(mhip_contact_op_t handle, const double** velocity /*[host] out: device pointer*/);

/* ------------------------------------------------------------------------------------------------------------------
 * BBPGD drivers (seam S1): solve_cqpp / solve_lcp with PGDStrategy<BBStepStrategy, residual policy>.
 * Replaces: mundy/math/src/mundy_math/convex.hpp:592-681 (PGDStrategy::initialize/iterate/done/result), :789-845.
 * State vectors x, g, x_tmp, g_tmp are caller-owned (PGDState holds references, convex.hpp:551-585); on return they
 * hold what the reference leaves in them.  x is the initial guess.
 *   _dense   : A is a row-major n x n device matrix (the KokkosBlas::gemv path)
 *   _contact : A is a contact operator handle; the iteration is fused into 3 kernels per iteration with a
 *              device-resident step size and residual (no host round trip per reduction).
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_bbpgd_solve_dense(size_t n, const double* A, const double* q, const mhip_space* space /*[host]*/,
                           const mhip_pgd_config* config /*[host]*/, double* x, double* g, double* x_tmp,
                           double* g_tmp, mhip_solve_result* result /*[host]*/, mhip_stream_t stream);
int mhip_bbpgd_solve_contact(mhip_contact_op_t op, const double* q, const mhip_space* space /*[host]*/,
                             const mhip_pgd_config* config /*[host]*/, double* x, double* g, double* x_tmp,
                             double* g_tmp, mhip_solve_result* result /*[host]*/, mhip_stream_t stream);

/* BUILD EXTENSION, parity unpinned -- Coulomb friction (BASELINE configs[2] names a "frictional LCP"; the reference has
 * no frictional solver: SURVEY F2).  The same fused BBPGD iteration on the cone complementarity problem
 *   p_c in R^3 (world-frame contact impulse),  K_c = { |p - (p.n) n| <= mu (p.n) },
 *   g_c = dt [(U_j + W_j x rb) - (U_i + W_i x ra)] + sep_c n_c,   p in K, g in K*, p . g = 0
 * (the convex relaxation of Anitescu / Tasora used by APGD-type solvers; mu = 0 reduces to the frictionless LCP).
 * op must be the vector-arm operator (mhip_contact_op_create with ra, rb = centre -> CONTACT POINT ON THE SURFACE, and
 * mob_rot).  p [C][3] is the initial guess on entry (in K; zeros are fine) and the solution on return, g [C][3] its
 * gradient.  Residual: Linf projected difference over the 3C components (config->residual_kind must say so). */
int mhip_bbpgd_solve_contact_friction(mhip_contact_op_t op, const double* sep, double mu,
                                      const mhip_pgd_config* config /*[host]*/, double* p, double* g,
                                      mhip_solve_result* result /*[host]*/, mhip_stream_t stream);
/* The same problem, arguments, result and stopping rule by APGD -- Nesterov-accelerated projected gradient descent with
 * adaptive restart and a backtracked curvature estimate (Mazhar, Heyn, Negrut, Tasora 2015: the algorithm BASELINE's
 * north star names, and the paper mundy_math/convex.hpp:476 cites), arranged so that a sweep is ONE operator application
 * (the gradient at the extrapolated point is the same extrapolation of the two stored gradients).  num_iters counts
 * every sweep, refused steps included.  BUILD EXTENSION like the BBPGD form: the reference has no frictional solver. */
int mhip_apgd_solve_contact_friction(mhip_contact_op_t op, const double* sep, double mu,
                                      const mhip_pgd_config* config /*[host]*/, double* p, double* g,
                                      mhip_solve_result* result /*[host]*/, mhip_stream_t stream);
/* Staged form of the same fused iteration for domain-decomposed runs: the host interleaves the halo
 * exchange and the cross-rank reduction between the stages, all asynchronously on `stream`:
 *     begin;  body(init) -> [ghost velocity halo] -> constraint(init, local) -> [all-gather local] -> finalize(init)
 *     repeat: body -> [halo] -> constraint(local) -> [all-gather] -> finalize;   poll every k iterations;   end
 * mhip_contact_op_set_partition: bodies [first, first+count) of the local index space are owned (swept by the body
 * stage), the rest are ghosts whose rows of `velocity` ([num_bodies][6], caller owned so the halo can write it) are
 * filled by the exchange; counted_contacts[c] != 0 marks contacts this rank contributes to the reductions (NULL: all).
 * local / gathered are DEVICE arrays of reduction records of MHIP_BBPGD_REDUCTION_WIDTH doubles:
 *     (max residual term, sum dx^2 as a double-double pair hi, lo, sum dx dg as a double-double pair hi, lo).
 * The two Barzilai-Borwein sums travel unrounded (~106 bits) and finalize adds the `nparts` gathered records in order
 * and rounds once, so every rank derives bit-identical step sizes and the rank count does not reach the result (the
 * same holds inside a rank for the workgroup mapping and, in the body sweep, for the order of a body's contact list).
 * Replaces: stk::all_reduce_max / stk::all_reduce_sum x3 per iteration (scrap/lcp_spheres/NGPSpheresLCP.cpp:371,
 * :450-452) with one 5-double all-gather, and the ghost field refresh of :1057 (left "TODO" there). */
#define MHIP_BBPGD_REDUCTION_WIDTH 5
int mhip_contact_op_set_partition(mhip_contact_op_t handle, size_t body_first, size_t body_count,
                                  const unsigned char* counted_contacts, double* velocity);
int mhip_bbpgd_stage_begin(mhip_contact_op_t op, const double* q, const mhip_space* space /*[host]*/,
                           const mhip_pgd_config* config /*[host]*/, double* x, double* g, double* x_tmp,
                           double* g_tmp, mhip_stream_t stream);
int mhip_bbpgd_stage_body(mhip_contact_op_t op, int init, mhip_stream_t stream);
int mhip_bbpgd_stage_constraint(mhip_contact_op_t op, int init, double* local, mhip_stream_t stream);
/* the constraint stage in pieces: sweep a sub-range of the constraints (any number of disjoint ranges per iteration,
 * e.g. interior contacts before the halo has landed, boundary contacts after), then reduce every sweep's partials of
 * this iteration into local.  stage_constraint == constraint_range(0, C) + reduce. */
int mhip_bbpgd_stage_constraint_range(mhip_contact_op_t op, int init, size_t c_first, size_t c_count,
                                      mhip_stream_t stream);
int mhip_bbpgd_stage_reduce(mhip_contact_op_t op, int init, double* local, mhip_stream_t stream);
int mhip_bbpgd_stage_finalize(mhip_contact_op_t op, int init, const double* gathered, int nparts,
                              mhip_stream_t stream);
int mhip_bbpgd_stage_poll(mhip_contact_op_t op, mhip_solve_result* result /*[host]*/, int* done /*[host]*/,
                          mhip_stream_t stream); /* synchronises */
/* between two iterations (e.g. right after a poll): copies the entries the body sweep's activity masks flag, and their
 * records, into compact per-body lists which the next sweeps stream instead of picking them out of the full lists
 * (time only: the same terms are summed, and every sum is rounded once).  Optional; the fused and distributed drivers
 * call it at their polls. */
int mhip_bbpgd_stage_snapshot_active(mhip_contact_op_t op, mhip_stream_t stream);
int mhip_bbpgd_stage_end(mhip_contact_op_t op, mhip_solve_result* result /*[host]*/, mhip_stream_t stream);
/* In-kernel small problems: convex::MundyMathBackend<Scalar, N> (convex.hpp:288-350) runs the same solver
 * on fixed-size Vector/Matrix inside a kernel; here one thread solves one dense n x n problem (1 <= n <= 16) of a
 * batch: A [batch][n][n] row major, q [batch][n], x [batch][n] (initial guess in, solution out), grad [batch][n],
 * per-problem num_iters / residual / converged (all device arrays).  Right-fold dot products and no |alpha|,|beta|
 * fast paths, exactly as that backend evaluates them. */
int mhip_solve_small_cqpp_batch(size_t batch, int n, const double* A, const double* q,
                                const mhip_space* space /*[host]*/, const mhip_pgd_config* config /*[host]*/,
                                double* x, double* grad, unsigned* num_iters, double* residual, int* converged,
                                mhip_stream_t stream);
/* The scrap app's own solver variant: resolve_collisions, scrap/lcp_spheres/NgpLcp.cpp:558-759 --
 * Dai-Fletcher residual |min(g,0)| / |g| with the 1e-12 active-set test (:376-405), strict `< max_allowable_overlap`
 * convergence, first step 1/residual, BB1/BB2 alternating by the parity of ite_count with the `|b| < 1e-12` guard
 * (:716-731), ite_count counting started iterations.  lam is the initial guess (in) and the multipliers (out);
 * lam_tmp, g, g_tmp are work vectors [C] (g = sep + dt*sep_dot on return).  *max_speed [host] receives max|U| over
 * bodies (ComputeMaxVelocity :743-755; CollisionResult.max_displacement = max_speed * dt).  result->num_iters = ite_count,
 * result->residual = max_abs_projected_sep. */
int mhip_scrap_bbpgd_solve_contact(mhip_contact_op_t op, const double* sep, double max_allowable_overlap,
                                   unsigned max_iterations, double* lam, double* lam_tmp, double* g, double* g_tmp,
                                   mhip_solve_result* result /*[host]*/, double* max_speed /*[host]*/,
                                   mhip_stream_t stream);
/* Same algorithm driven kernel-by-kernel through the S1 vector entry points above (what the C++ adapter's
 * HipBackend does): the unfused reference structure, kept as an in-library cross-check of the fused path. */
int mhip_bbpgd_solve_contact_unfused(mhip_contact_op_t op, const double* q, const mhip_space* space /*[host]*/,
                                     const mhip_pgd_config* config /*[host]*/, double* x, double* g, double* x_tmp,
                                     double* g_tmp, mhip_solve_result* result /*[host]*/, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Stream compaction helpers (filter_view, mundy/mesh/src/mundy_mesh/GenNeighborLinkers.hpp:141-183: exclusive scan +
 * stable scatter; the total is read back on the host exactly as :155-156 does).
 *   filter_pairs_owned : keep pairs with at least one endpoint in [first, first+count) (drops ghost-ghost pairs);
 *                        counted_out[k] = 1 iff the kept pair's source (lower index) is owned.  pairs_out may alias
 *                        neither input.  *count_out [host].
 *   select_aabb_overlap: indices (ascending) of the boxes aabb[i] grown by `buffer` that intersect (closed test) the
 *                        box `box6` [host: min xyz, max xyz] -- the ghost candidates for a neighbouring rank.
 *   select_contacts    : BUILD OPTION (off by default: the reference's LCP app makes every neighbour pair a constraint,
 *                        scrap/lcp_spheres/NgpLcp.cpp:346-373).  kept_index [<= c] = ascending indices of the candidate
 *                        pairs whose signed separation is not above `cutoff` (NaN kept), by wavefront ballot + prefix
 *                        sum; *count_out [host].  The caller gathers pairs / normals / arms with mhip_gather_rows and
 *                        builds the operator on the kept contacts only: fewer constraints per sweep.  A dropped pair
 *                        is a constraint that must stay inactive: check g = sep + dt sdot >= 0 on the dropped pairs
 *                        afterwards (the steppers do, and fall back to the full list when it fails).
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_select_contacts(size_t c, const double* sep, double cutoff, int32_t* kept_index, size_t* count_out /*[host]*/,
                         mhip_stream_t stream);
int mhip_filter_pairs_owned(size_t c, const int32_t* pairs_in, size_t first, size_t count, int32_t* pairs_out,
                            unsigned char* counted_out, size_t* count_out /*[host]*/, mhip_stream_t stream);
/* Same selection, ordered for overlap: first the pairs with BOTH bodies owned (interior), then those with exactly one
 * (boundary), each block in input order.  interior_out = size of the first block, count_out = total.  The staged solver
 * sweeps [0, interior) while the ghost-velocity halo that the boundary block needs is still in flight. */
int mhip_partition_pairs_owned(size_t c, const int32_t* pairs_in, size_t first, size_t count, int32_t* pairs_out,
                               unsigned char* counted_out, size_t* interior_out /*[host]*/,
                               size_t* count_out /*[host]*/, mhip_stream_t stream);
int mhip_select_aabb_overlap(size_t n, const double* aabb, double buffer, const double* box6 /*[host]*/,
                             int32_t* idx_out, size_t* count_out /*[host]*/, mhip_stream_t stream);
/* A rank's region as several boxes: bodies [k * ceil(n / nchunks), ...) form chunk k (the owned bodies are in curve
 * order, so a chunk is a compact blob); boxes [device, (nchunks + 1)][6] receives the bounds of each chunk's boxes grown
 * by `buffer` and, last, their union.  select_aabb_overlap_any keeps the bodies whose grown box meets ANY of the first
 * nboxes boxes (boxes [device, (nboxes + 1)][6], the last one the union, used as a quick reject) -- the ghost
 * candidates for a rank described that way; ascending order.  No host round trip in chunk_bounds. */
int mhip_aabb_chunk_bounds(size_t n, const double* aabb, double buffer, int nchunks, double* boxes,
                           mhip_stream_t stream);
int mhip_select_aabb_overlap_any(size_t n, const double* aabb, double buffer, int nboxes, const double* boxes,
                                 int32_t* idx_out, size_t* count_out /*[host]*/, mhip_stream_t stream);
/* min / max corner over n boxes grown by `buffer`: out6 [host] (an empty set gives the inverted box) */
int mhip_aabb_bounds(size_t n, const double* aabb, double buffer, double* out6 /*[host]*/, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Time integration either side of the solve: x += dt * U (scrap/lcp_spheres/NgpLcp.cpp:898) and, for
 * rods, q <- rotate_quaternion(q, W, dt) (mundy/math/src/mundy_math/Quaternion.hpp:1366-1390).
 * velocity is [n][6] as produced by the contact operator.  quat may be NULL (spheres).
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_integrate_euler(size_t n, double dt, const double* velocity, double* center, double* quat,
                         mhip_stream_t stream);

/* Periodic box: PeriodicScaledMetric::sep (minimum-image separation p1 -> p2) and wrap_rigid of a
 * Sphere / Spherocylinder / Ellipsoid (the centre is wrapped into [0, box), orientation and size untouched).
 * Replaces: mundy/geom/src/mundy_geom/periodicity.hpp:812-823, :1088-1113, :1156-1160.  box [host] 3 doubles. */
int mhip_periodic_sep(size_t n, const double* box, const double* p1, const double* p2, double* out,
                      mhip_stream_t stream);
int mhip_wrap_rigid(size_t n, const double* box, double* center, mhip_stream_t stream);

/* Triclinic cell: PeriodicMetric (periodicity.hpp:233-332).  cell [host] = 3x3 unit-cell matrix, row
 * major, lattice vectors as COLUMNS; its inverse is math::inverse (Matrix.hpp:1596-1601: adjugate / determinant).
 *   mhip_unit_cell_inverse        host-only: that inverse, for callers that want fractional coordinates
 *   mhip_periodic_sep_triclinic   sep(p1, p2) = h * min_image(h_inv * (p2 - p1))          (:304-307)
 *   mhip_wrap_rigid_triclinic     centre <- h * safe_unit_mod1(h_inv * centre)             (:312-314, :1088-1113)
 *   mhip_shift_image_triclinic    p + h * images, images [n][3] int32                      (:323-327)
 *   mhip_contact_spheres_triclinic  mhip_contact_spheres with this metric's minimum image */
int mhip_unit_cell_inverse(const double* cell, double* cell_inv);
int mhip_periodic_sep_triclinic(size_t n, const double* cell, const double* p1, const double* p2, double* out,
                                mhip_stream_t stream);
int mhip_wrap_rigid_triclinic(size_t n, const double* cell, double* center, mhip_stream_t stream);
int mhip_shift_image_triclinic(size_t n, const double* cell, const double* p, const int32_t* images, double* out,
                               mhip_stream_t stream);
int mhip_contact_spheres_triclinic(size_t c, const int32_t* pairs, const double* center, const double* radius,
                                   const double* cell, double* sep, double* normal, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Body reordering: Z-order (Morton) permutation of bodies by centre, z most significant as
 * zorder_knn::Less (mundy/math/src/mundy_math/zmort.hpp:195-220) orders non-negative lattice coordinates.
 * perm[k] = index of the body that goes to position k.  Deterministic (ties broken by index).
 * The lattice has 2^b cells per axis, b = the largest of 4..8 with 8^b <= 8 n (the code space stays within 8 codes per
 * body: 128 cells per axis at 10^6 bodies); lattice coordinates floor((c - lo) / cell_size) are clamped to
 * [0, 2^b - 1], so bodies outside that cube share the boundary cells (a locality heuristic there, exact Z-order inside).
 * The clamp is applied to the floored double before the integer conversion: a coordinate below 0 or NaN gives cell 0,
 * one above 2^b - 1 or +inf gives 2^b - 1 (the same rule for mhip_curve_order / mhip_curve_keys).
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_morton_order(size_t n, const double* center, const double* lo /*[host] 3*/, double cell_size, int32_t* perm,
                      mhip_stream_t stream);
/* The same reordering along any lattice curve given as a table: key_table [device, (2^level)^3 int32, indexed
 * [ix][iy][iz]] = visiting index of the cell.  With the table of mundy::math::hilbert_3d (mundy/math/src/mundy_math/
 * Hilbert.hpp:48-83; mundy_amd.distributed.hilbert_key_table generates it with that recursion) this is the Hilbert
 * order used for the domain decomposition.  Cells: floor((c - lo) / (hi - lo) * 2^level) clamped to the lattice as
 * above (NaN -> 0); ties by index.  level <= 8. */
int mhip_curve_order(size_t n, const double* center, const double* lo /*[host] 3*/, const double* hi /*[host] 3*/,
                     int level, const int32_t* key_table, int32_t* perm, mhip_stream_t stream);
/* keys[i] = key_table entry of body i's cell (the value mhip_curve_order sorts by): the Hilbert position of the cell --
 * what the work-weighted domain decomposition cuts and what decides a body's owner when it migrates */
int mhip_curve_keys(size_t n, const double* center, const double* lo /*[host] 3*/, const double* hi /*[host] 3*/,
                    int level, const int32_t* key_table, uint32_t* keys, mhip_stream_t stream);
/* perm = the stable ascending order of n unsigned 64-bit keys (radix sort, 8 bits per pass): perm[k] = index of the
 * k-th key.  keys is not modified. */
int mhip_sort_by_key_u64(size_t n, const uint64_t* keys, int32_t* perm, mhip_stream_t stream);
/* dst[k][0..width) = src[perm[k]][0..width)  for rows of `width` doubles */
int mhip_gather_rows(size_t n, size_t width, const int32_t* perm, const double* src, double* dst, mhip_stream_t stream);
/* dst[k * dst_stride + c] = src[k * src_stride + c], c < width (strides in doubles): packs per-body fields into
 * interleaved records for the ghost exchange and unpacks them again */
int mhip_copy_strided(size_t n, size_t width, const double* src, size_t src_stride, double* dst, size_t dst_stride,
                      mhip_stream_t stream);


/* ----------------------------------------------------------------------------------------------------------------
 * Multi-GPU transport and the domain-decomposed solve driven from C++.
 *
 * Replaces, on the reference side: the MPI communicator handed to stk::search::coarse_search and change_ghosting
 * (mundy/mesh/src/mundy_mesh/GenNeighborLinkers.hpp:658, :687-711), and per BBPGD iteration stk::all_reduce_max +
 * 3 x stk::all_reduce_sum (scrap/lcp_spheres/NGPSpheresLCP.cpp:371, :450-452) and the ghost field refresh left as a
 * TODO at :1057.
 *
 * A communicator is one rank's end of a group of `world` ranks, one rank per GPU.  Two transports:
 *   - RCCL (mhip_comm_create_rccl): grouped ncclSend / ncclRecv over xGMI, issued on a stream the communicator owns
 *     and ordered against the caller's stream with events, so an exchange started after one kernel overlaps the
 *     kernels launched before mhip_comm_exchange_finish; ncclAllGather goes straight onto the caller's stream (it sits
 *     on the critical path of every solver iteration).  A message addressed to oneself is delivered as a local copy
 *     (the host transport rejects it).  librccl is looked up at run time (dlopen of
 *     the already loaded librccl.so.1 or the one on the library path): no link dependency.  The 128-byte unique id
 *     is made by rank 0 (mhip_comm_unique_id) and handed to the other ranks by the launcher (MPI_Bcast in an MPI
 *     host, the torch.distributed store in bench.py).
 *   - host callbacks (mhip_comm_create_host): the same calls forwarded to two functions of the host program after a
 *     stream synchronisation (device pointers are passed through).  For hosts that bring their own message layer and
 *     for tests where several ranks share one GPU, which RCCL refuses.
 * All buffers are DEVICE pointers to doubles; counts are in doubles.  Handles are not thread-safe.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct mhip_comm* mhip_comm_t;
#define MHIP_COMM_ID_BYTES 128
typedef int (*mhip_comm_exchange_fn)(void* user, int nsend, const int* send_peer, const double* const* send_buf,
                                     const size_t* send_count, int nrecv, const int* recv_peer, double* const* recv_buf,
                                     const size_t* recv_count); /* returns 0 when every message has landed */
typedef int (*mhip_comm_all_gather_fn)(void* user, const double* send, size_t count, double* recv /*[world][count]*/);

int mhip_comm_unique_id(unsigned char* id /*[host] MHIP_COMM_ID_BYTES*/);
int mhip_comm_create_rccl(mhip_comm_t* comm, const unsigned char* id /*[host]*/, int rank, int world);
int mhip_comm_create_host(mhip_comm_t* comm, int rank, int world, mhip_comm_exchange_fn exchange,
                          mhip_comm_all_gather_fn all_gather, void* user);
int mhip_comm_destroy(mhip_comm_t comm);
int mhip_comm_info(mhip_comm_t comm, int* rank, int* world, int* is_rccl);
/* Mailbox (ranks of ONE node): the 5-double reduction record every rank contributes to every BBPGD iteration
 * (NGPSpheresLCP.cpp:371, :450-452: 1 all_reduce_max + 3 all_reduce_sum there) travels through slots in the ranks'
 * device memory instead of a collective launch: every rank owns a box of fine-grained memory that all the others map
 * (hipIpc handles, exchanged through the communicator's own all-gather); a rank writes its record into its slot of
 * every box -- posted writes over xGMI -- and polls its own box, all inside the kernel that forms the record.  Every
 * 8-byte word carries 32 bits of data and the number of the exchange, so each store validates itself and the writes
 * may arrive in any order.  Collective call.  *opened = 1: every rank has mapped every box and two trial exchanges went
 * through everywhere (mhip_bbpgd_solve_contact_distributed then uses it); 0: somebody could not (another node, no peer
 * access) and everybody keeps the transport's all-gather.  A record that does not arrive within 20 s ends the solve in
 * MHIP_ERR_RUNTIME on the ranks that waited for it (bounded polling: no wave waits forever). */
int mhip_comm_mailbox_open(mhip_comm_t comm, int* opened /*[host]*/, mhip_stream_t stream);
int mhip_comm_mailbox_close(mhip_comm_t comm);
/* The per-iteration VELOCITY HALO of mhip_bbpgd_solve_contact_distributed without the collective library, for the
 * ranks of ONE node (same condition as the mailbox).  on = 1: from the next mhip_ghost_plan on (collective: every rank
 * must have made the same call) each rank keeps an inbox of fine-grained device memory, one slot per local body row,
 * IPC-mapped by all the others.  After its body sweep a rank writes the rows its peers hold as ghosts straight into
 * their inboxes (posted writes over xGMI; every 8-byte word carries 32 bits of data and the number of the exchange, so
 * each store validates itself); before its boundary sweep a rank collects its ghost rows from its own inbox into the
 * velocity table (bounded polling: a peer that never writes ends in MHIP_ERR_RUNTIME).  Replaces the gather kernel,
 * the grouped ncclSend / ncclRecv and two stream hand-overs per iteration by two launches on the solver's own stream.
 * Anything short of success on every rank (allocation, mapping, probing) leaves everybody on send / recv.  The solve
 * takes this path only for the halo of the communicator's current ghost plan; same rows, same bits.
 * Replaces: communicate_field_data (scrap/.../SpherocylinderSpherocylinderLinker.cpp:154-155) inside the iteration,
 * the ghost refresh the reference leaves as a TODO (NGPSpheresLCP.cpp:1057). */
int mhip_comm_halo_ipc_enable(mhip_comm_t comm, int on);
/* Bound of every wait on a peer's words (mailbox records, inbox rows) in seconds; default 20.  A wait that exceeds it
 * ends the solve with MHIP_ERR_RUNTIME on that rank -- no wave waits forever.  After ANY failed distributed solve the
 * ranks may disagree on the exchange numbers: the next mhip_ghost_plan (collective) re-agrees them (the maximum over the
 * ranks) and clears the sticky error flag, so the recovery is "rebuild, then solve again". */
int mhip_comm_set_exchange_timeout(mhip_comm_t comm, double seconds);
/* TEST HOOK: the next mhip_bbpgd_solve_contact_distributed on this communicator returns MHIP_ERR_RUNTIME at its
 * at_poll-th convergence poll (1 = the first), after the iterations enqueued until then; 0 = off.  One shot.  Exists so
 * that the tests can show a failed solve leaves the communicator usable (exchange numbers retired on every exit). */
int mhip_comm_inject_fault(mhip_comm_t comm, unsigned at_poll);
/* *active [host] = 1 when the current ghost plan's halo will travel through the inboxes */
int mhip_comm_halo_ipc_active(mhip_comm_t comm, int* active /*[host]*/);
/* recv[r][0..count) = rank r's send[0..count); later work on `stream` sees recv */
int mhip_comm_all_gather(mhip_comm_t comm, const double* send, size_t count, double* recv, mhip_stream_t stream);
/* One grouped point-to-point exchange: message k goes to send_peer[k] / comes from recv_peer[k]; empty messages are
 * skipped on both sides.  start: the transfers begin once the work already on `stream` is done; finish: later work on
 * `stream` waits for them.  The peer / pointer / count arrays are host arrays and are read during start only. */
int mhip_comm_exchange_start(mhip_comm_t comm, int nsend, const int* send_peer, const double* const* send_buf,
                             const size_t* send_count, int nrecv, const int* recv_peer, double* const* recv_buf,
                             const size_t* recv_count, mhip_stream_t stream);
int mhip_comm_exchange_finish(mhip_comm_t comm, mhip_stream_t stream);

/* Ghost-velocity halo of one rank, fixed between neighbour-list rebuilds.  velocity = the [num_local_bodies][6] array
 * given to mhip_contact_op_set_partition.  Rows send_index[...] (DEVICE, local body indices, peer after peer in the
 * order of send_peer, send_rows[k] of them for peer k) go out each iteration; rows [recv_first_row[k],
 * recv_first_row[k] + recv_rows[k]) are filled from recv_peer[k]. */
typedef struct mhip_velocity_halo {
  double* velocity;
  int num_send_peers;
  const int* send_peer;       /* [host] */
  const size_t* send_rows;    /* [host] */
  const int32_t* send_index;  /* [device] sum(send_rows) */
  int num_recv_peers;
  const int* recv_peer;            /* [host] */
  const size_t* recv_first_row;    /* [host] */
  const size_t* recv_rows;         /* [host] */
} mhip_velocity_halo;
/* Ghost bodies of one neighbour-list rebuild (replaces coarse_search(comm) + change_ghosting,
 * GenNeighborLinkers.hpp:658, :687-711).  Ranks own contiguous, increasing ranges of the global (curve-ordered) ids.
 *   plan:     all-gather of the rank regions (64 chunk boxes per rank, mhip_aabb_chunk_bounds), per peer the owned bodies
 *             whose grown box meets any of the peer's boxes (closed test, ascending order), all-gather of the count
 *             matrix.  The owned bodies should be in curve order (any order is correct, only looser).  Fills `layout`:
 *             local index order = ghosts of lower ranks (peer order), the n owned bodies, ghosts of higher ranks --
 *             also global-id order, so local pairs (i < j) keep their global orientation; and the velocity halo of
 *             this layout (lists owned by the communicator, valid until the next plan; halo.velocity is left NULL).
 *   exchange: moves rows of `width` doubles with that plan: local[num_ghost_lo + i] = records[i] for the owned rows,
 *             ghost rows filled from their owners.  Any number of record sets per plan. */
typedef struct mhip_ghost_layout {
  size_t num_ghost_lo, num_owned, num_ghost_hi;
  size_t num_sent; /* owned bodies that are ghosts somewhere, counted once per receiving rank */
  mhip_velocity_halo halo;
} mhip_ghost_layout;
/* The bookkeeping of the plan on its own (host arithmetic only, no device): counts[s * world + d] = bodies rank s sends
 * to rank d.  Peer lists are filled in ascending rank order, empty messages left out; the lists must hold `world`
 * entries.  recv_first_row = first local row of each peer's ghosts. */
int mhip_ghost_layout_from_counts(int world, int rank, size_t n_owned, const size_t* counts /*[host]*/,
                                  size_t* num_ghost_lo, size_t* num_ghost_hi, int* num_send, int* send_peer,
                                  size_t* send_rows, int* num_recv, int* recv_peer, size_t* recv_first_row,
                                  size_t* recv_rows);
int mhip_ghost_plan(mhip_comm_t comm, size_t n, const double* aabb, double buffer,
                    mhip_ghost_layout* layout /*[host] out*/, mhip_stream_t stream);
int mhip_ghost_exchange(mhip_comm_t comm, size_t width, const double* records /*[n][width]*/,
                        double* local /*[num_ghost_lo + n + num_ghost_hi][width]*/, mhip_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Ownership follows the bodies (replaces the RCB repartition of stk::balance::balanceStkMesh,
 * scrap/lcp_spheres/NGPSpheresLCP.cpp:956, which the bacteria app calls every load_balance_frequency steps,
 * scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:1076-1078).  Ranks own contiguous ranges of
 * the Hilbert curve over a fixed lattice: rank r owns the cells  splitters[r - 1] < key <= splitters[r].
 *   mhip_hilbert_key_table  [host] table[ix][iy][iz] = position of the cell along mundy::math::hilbert_3d
 *                           (mundy/math/src/mundy_math/Hilbert.hpp:48-83); (2^level)^3 entries, level <= 8; feed it to
 *                           mhip_curve_keys / mhip_curve_order
 *   mhip_curve_cut          cuts the curve at equal cumulative WORK: weight per body (null = 1; the steppers use
 *                           1 + contacts of the last step) histogrammed over the cells, all-gathered, summed in rank
 *                           order, cut where the running sum reaches r / world of the total.  Every rank computes the
 *                           same world - 1 splitters [host].  Collective.
 *   mhip_migrate_plan       destination rank of every owned body from its cell key; counts all-gathered.  n_new =
 *                           bodies this rank owns afterwards.  Collective.
 *   mhip_migrate_exchange   records [n][width] -> out [n_new][width]: the rows that stay (in their present order),
 *                           then the arrivals, peers in increasing rank; one grouped send / recv per peer.  Any number
 *                           of exchanges may follow one plan.  The caller then orders its rows as it likes (the
 *                           steppers: by cell key, ties by entity id -- the order a single rank would have).
 * Small helpers of that bookkeeping:
 *   mhip_body_work_weights  weights[k] = 1 + number of pairs that contain local body first + k, k < count
 *   mhip_compose_keys_u64   out[i] = major[i] << shift | (uint64) minor[i]  (cell key, then entity id).  Precondition,
 *                           not checked on the device: every minor[i] is an integer-valued double in [0, 2^shift);
 *                           another value overwrites key bits or is truncated.  The steppers use shift 40 and refuse
 *                           entity ids outside [0, 2^40) when they are given.
 *   mhip_fill_sequence      dst[i] = first + i
 * ---------------------------------------------------------------------------------------------------------------- */
int mhip_hilbert_key_table(int level, int32_t* table /*[host] (2^level)^3*/);
int mhip_body_work_weights(size_t c, const int32_t* pairs, size_t first, size_t count, double* weights /*[count]*/,
                           mhip_stream_t stream);
int mhip_compose_keys_u64(size_t n, const uint32_t* major, const double* minor, int shift, uint64_t* out,
                          mhip_stream_t stream);
int mhip_fill_sequence(size_t n, double first, double* dst, mhip_stream_t stream);
int mhip_curve_cut(mhip_comm_t comm, size_t n, const uint32_t* keys, const double* weights /*[n] or null*/, size_t ncell,
                   int64_t* splitters /*[host] world - 1*/, mhip_stream_t stream);
int mhip_migrate_plan(mhip_comm_t comm, size_t n, const uint32_t* keys, const int64_t* splitters /*[host] world - 1*/,
                      size_t* n_new, size_t* num_sent /*or null*/, size_t* num_received /*or null*/,
                      mhip_stream_t stream);
int mhip_migrate_exchange(mhip_comm_t comm, size_t width, const double* records /*[n][width]*/,
                          double* out /*[n_new][width]*/, mhip_stream_t stream);
typedef struct mhip_dist_profile { /* HIP-event times of sampled iterations that did work, summed over them */
  double body_ms;        /* body sweep */
  double constraint_ms;  /* interior + boundary constraint sweeps (the wait for the halo excluded) */
  double halo_wait_ms;   /* between the interior and the boundary sweep: collect from the inbox / finish of send-recv */
  size_t timed_iterations;
  double halo_post_ms;   /* after the body sweep: the push into the peers' inboxes / gather + start of send-recv */
  double record_ms;      /* after the boundary sweep: this rank's record, its exchange (the wait for the slowest rank
                            included) and the finalize */
  int halo_path;         /* what this solve ACTUALLY used: 0 no halo (one rank / no ghosts), 1 IPC-mapped inboxes,
                            2 grouped send / recv of the transport */
  int record_path;       /* 1 mailbox inside the fold-finalize launch, 2 mailbox in the record's launch (world > the
                            fused limit), 3 all-gather of the transport */
} mhip_dist_profile;
/* The domain-decomposed BBPGD solve, whole loop on the host side of this library (no interpreter between the stages):
 *   begin;  per iteration: body sweep of the owned bodies -> pack + start the velocity halo -> constraint sweep of the
 *   interior contacts [0, interior_contacts) while the halo is in flight -> finish halo -> sweep of the boundary
 *   contacts -> local (max, sum dx^2, sum dx dg) record -> all-gather -> every rank reduces the records in rank order
 *   (bit-identical steps) ;  convergence polled after stretches of 8, 16, 32, ... iterations, at most poll_every (0: 64) ;  end.
 * Same iterates as the mhip_bbpgd_stage_* sequence driven by hand.  op must carry mhip_contact_op_set_partition; the
 * four solver vectors are caller owned as in mhip_bbpgd_solve_contact.  profile may be NULL. */
int mhip_bbpgd_solve_contact_distributed(mhip_contact_op_t op, mhip_comm_t comm, const mhip_velocity_halo* halo,
                                         size_t interior_contacts, const double* q, const mhip_space* space /*[host]*/,
                                         const mhip_pgd_config* config /*[host]*/, double* x, double* g, double* x_tmp,
                                         double* g_tmp, unsigned poll_every, mhip_solve_result* result /*[host]*/,
                                         mhip_dist_profile* profile /*[host]*/, mhip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUNDY_HIP_H_ */
