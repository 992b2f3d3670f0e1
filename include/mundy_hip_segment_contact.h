/* mundy_hip_segment_contact.h -- frictionless contacts between backbone segments: the excluded volume of the HP1 app.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (SEGMENT_CONTACT_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives.  tests/test_segment_contact_host.py and
 * tests/test_gpu_segment_contacts_streams.py make over this header the checks that tests/test_capi_symbols.py and
 * tests/test_gpu_streams.py make over mundy_hip.h.  The contract is mundy_hip.h's: every entry point takes a
 * mhip_stream_t and is ordered on it; only update, which returns a host flag, synchronises (and create, whose host
 * arrays may go as soon as it returns).
 *
 * The reference (scrap/.../HP1.cpp:4356-4496, compute_hertzian_contact_forces, the first term of its force field,
 * :4737): the excluded volume of the chromatin acts between the spherocylinder segments that join consecutive beads.
 *   list        every pair of segments whose boxes meet and that share no node (:3053-3175,
 *               DestroyBoundNeighbors.cpp:150-170), rebuilt when a box corner has moved by skin / 2 (:3212-3262)
 *   distance    ...SpherocylinderSegmentSpherocylinderSegmentLinker.cpp:204-237
 *   law         ...SegmentHertzianContact.cpp:192-225 (HERTZ) or ...SegmentWCA.cpp:187-210 (WCA), no friction, no history
 *   reduction   linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221, then the end-segment
 *               correction of HP1.cpp:4375-4493
 *
 * Segments.  m segments over n bodies; segment e joins the bodies ends[e][0] and ends[e][1] (any connectivity: a body
 *   may carry any number of segments) and has the radius r_e.  seg[e] = (x_a, x_b, r_e, 0), one 64-byte row.
 * Boxes.  aabb[e] = compute_aabb(SpherocylinderSegment) of (x_a, x_b, reach_e), grown by skin; reach_e = r_e for HERTZ,
 *   max(r_e, cutoff / 2) for WCA.  (The reference uses r_e for both; the wider box makes the list a superset, so that no
 *   pair inside the cutoff is missing from it.)
 * List.  MHIP_SEARCH_AABB over these boxes, buffer 0, unique pairs i < j in ascending (i, j) order, without the pairs
 *   that share a node.  Rebuilt on the first update, when forced, or when mhip_aabb_moved(aabb, snapshot of the last
 *   build, 0.5 skin) fires.
 * Linker (i, j).  cp_i, cp_j, dist = distance(segment i, segment j); sep = dist - (r_i + r_j);
 *   n = (cp_j - cp_i) (1 / dist).  Force branch: HERTZ iff sep < 0, WCA iff dist < cutoff.
 *     HERTZ  Rs = r_i r_j / (r_i + r_j), Es = E E / (E - E nu nu + E - E nu nu),
 *            fm = (4.0 / 3.0) Es sqrt(Rs) pow(-sep, 1.5)
 *     WCA    d = sep + (r_i + r_j), rho2 = sigma sigma / (d d), rho6 = rho2 rho2 rho2, rho12 = rho6 rho6,
 *            fm = 24.0 epsilon (2.0 rho12 - rho6) / d
 *   force[c] = -fm n, on segment i (segment j receives the negative); share[c][side] = what the second end node of that
 *   side's segment receives of the force acting at its closest point (the first one receives the rest).  Outside the
 *   branch the force and share rows are +0.0.  dist == 0 gives NaN rows.  A pair index outside [0, m) gives NaN rows
 *   and is never dereferenced.
 * Segment sums.  From +0.0, over the segment's linkers in ascending list order: a0[e] = sum (Fs - share),
 *   a1[e] = sum share, Fs = +/- force[c] by side.  Where end_correction[e] is set (HP1.cpp:4395-4434, :4451-4490):
 *   L = sqrt((dx dx + dy dy) + dz dz), t = d / L per component, d = x_b - x_a;
 *     HERTZ  fm as above with sep = L - 2 r_e and Rs = r_e r_e / (r_e + r_e), iff sep < 0
 *            (pow(-sep, 1.5) there rounded once, not to the library pow's ulp: the value a host pow returns)
 *     WCA    fm as above with d = L, iff L < cutoff
 *   a0[e] -= fm t, a1[e] += fm t.
 * Node gather.  S_b = +0.0 + sum over the body's (segment, side) entries in ascending segment index of a_side[e];
 *   force[b] = S_b, or force[b] + S_b when accumulating (a body on no segment: +0.0, or left untouched).  No atomic on
 *   a force; nothing depends on the grid.
 * Statistics.  stats [device, 16 bytes]: stats[0] the bits of the double max(0, -sep) over the force branch, the
 *   corrected end segments included (sep = L - 2 r_e there, for both kinds); stats[1] a uint64 count of the linkers in
 *   the force branch.
 *
 * create     copies the host arrays, builds the exclusion rows on the host and the body -> (segment, side) incidence
 *            on the device, synchronises `stream`.  radius NULL: radius_scalar for every segment.  end_correction NULL:
 *            no segment is corrected.  m == 0 is valid.  Refused with MHIP_ERR_INVALID_ARGUMENT before any HIP call: a
 *            null handle, ends (m > 0) or params; an end outside [0, n); a segment from a body to itself; a radius <= 0;
 *            skin < 0; HERTZ: youngs_modulus <= 0, poisson_ratio outside (0, 1); WCA: epsilon < 0, sigma <= 0,
 *            cutoff <= 0; an unknown kind; anything not finite.
 * update     segment view and boxes at `center` [n][3]; rebuilds the list when due.  *rebuilt [host] tells.  Synchronises.
 * force      segment view at `center`, then linker_pass and reduce.  stats is zeroed first.  MHIP_ERR_RUNTIME before the
 *            first update, the message names the missing call.
 * linker_pass / reduce   the two halves of force over the segment view as it stands.  linker_pass zeroes stats;
 *            reduce only raises stats[0] (stats may be NULL there).
 * get        device pointers and counts.  destroy frees the handle.
 * Not built: periodic cells, several GPUs, friction or history, per-segment materials, the contact's twist torque (the
 * reference ignores it). */
#ifndef MUNDY_HIP_SEGMENT_CONTACT_H_
#define MUNDY_HIP_SEGMENT_CONTACT_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MHIP_SEGMENT_CONTACT_HERTZ 0
#define MHIP_SEGMENT_CONTACT_WCA 1

typedef struct mhip_segment_contact_params {
  int kind; /* MHIP_SEGMENT_CONTACT_* */
  double skin;
  double youngs_modulus, poisson_ratio; /* HERTZ */
  double epsilon, sigma, cutoff;        /* WCA */
} mhip_segment_contact_params;
typedef struct mhip_segment_contact_fields {
  size_t num_bodies, num_segments, num_pairs;
  int32_t* pairs;      /* [num_pairs][2] */
  double *sep, *force; /* [num_pairs], [num_pairs][3] */
  double* share;       /* [num_pairs][2][3] */
  double *seg, *aabb;  /* [num_segments][8], [num_segments][6] */
} mhip_segment_contact_fields;
typedef struct mhip_segment_contacts* mhip_segment_contacts_t;

int mhip_segment_contacts_create(mhip_segment_contacts_t* handle, size_t n, size_t m,
                                 const int32_t* ends /*[host] m x 2*/, const double* radius /*[host] m or NULL*/,
                                 double radius_scalar, const unsigned char* end_correction /*[host] m or NULL*/,
                                 const mhip_segment_contact_params* params, mhip_stream_t stream);
int mhip_segment_contacts_destroy(mhip_segment_contacts_t handle);
int mhip_segment_contacts_update(mhip_segment_contacts_t handle, const double* center, int force_rebuild,
                                 int* rebuilt /*[host]*/, mhip_stream_t stream);
int mhip_segment_contacts_force(mhip_segment_contacts_t handle, const double* center, double* force /*[n][3]*/,
                                int accumulate, void* stats /*[device] 16 bytes*/, mhip_stream_t stream);
int mhip_segment_contacts_linker_pass(mhip_segment_contacts_t handle, void* stats /*[device] 16 bytes*/,
                                      mhip_stream_t stream);
int mhip_segment_contacts_reduce(mhip_segment_contacts_t handle, double* force /*[n][3]*/, int accumulate,
                                 void* stats /*[device] 16 bytes or NULL*/, mhip_stream_t stream);
int mhip_segment_contacts_get(mhip_segment_contacts_t handle, mhip_segment_contact_fields* fields);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_SEGMENT_CONTACT_H_ */
