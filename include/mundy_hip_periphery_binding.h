/* mundy_hip_periphery_binding.h -- periphery bind sites: crosslinkers that tether chromatin to the nuclear envelope.
 *
 * A header of its own, which mundy_hip.h does not contain, and bound by a table of its own in capi.py
 * (PERIPHERY_BINDING_SIGNATURES), for the reason mundy_hip_hydro_periphery.h gives: tests/test_gpu_streams.py fails for
 * any stream-taking prototype of mundy_hip.h that its case table does not call, tests/test_capi_symbols.py for a binding
 * of SIGNATURES that mundy_hip.h does not declare, and the change that added these entry points could edit neither file.
 * tests/test_periphery_binding_host.py and tests/test_gpu_periphery_binding_streams.py make the same checks over this
 * header.  A later change that may edit those files folds this header back into mundy_hip.h.  The contract is
 * mundy_hip.h's: every entry point takes a mhip_stream_t and is ordered on it, none synchronises.
 *
 * The reference (scrap/.../HP1.cpp): the right head of an HP1 crosslinker binds to a chromatin bead or to one of a set
 * of immobile bind sites scattered over the nuclear envelope (enable_periphery_binding, on by default: :5220; 1000
 * random sites, A = 1, k = 1000, r0 = 1: :5287-5292).  The sites have rate constants of their own (:3340-3398) and take
 * part in the same draw (:3473-3529).  The extension of the crosslinker model of mundy_hip.h (mhip_crosslinkers_*):
 *
 * Sites and state.  P immobile sites y_s, s in [0, P).  left[c], right[c] as before: right == left singly bound,
 *   right >= 0 and != left bound to that bead, right == -(s + 1) bound to periphery site s.  Several crosslinkers may
 *   hold one site (no exclusivity in the reference).
 * Rate to a site.  d = |y_s - x_left| (the right-fold norm of the bead rate), rate = xl_rate<TYPE>(d) of the
 *   crosslinkers' spring type and 1 / kT with the periphery's own A_p (bind_rate), k_p, r_p (:3372-3394); FENE: d >= r_p
 *   gives 0; d > capture_radius_p gives 0 exactly.
 * Draw.  One uniform per crosslinker and step, u = ((w0 << 21) | (w1 >> 11)) 2^-53 of Philox block 0 at (key, counter);
 *   the counter advances whatever the state.  A singly bound c walks the bead row of left[c] in ascending original id,
 *   then the periphery row of left[c] in ascending site index.  z_tot is ONE running sum over both rows from +0.0,
 *   z_tot += dt rate.  It binds iff u < 1 - exp(-z_tot); the running sum of ((1 - exp(-z_tot)) dt / z_tot) rate goes on
 *   across the row boundary, and the first entry whose running sum exceeds u wins, bead or site.
 * Unbinding.  A periphery-bound crosslinker unbinds iff u < 1 - exp(-(dt k_off_p)); a bead-bound one with k_off.
 * Force.  A periphery-bound crosslinker is the spring between x_left and y_s of the crosslinkers' type / k / r (the
 *   reference runs one constraint forcing over every non-left-bound HP1, :4507-4514): d = y_s - x_left, the spring_term
 *   of mhip_crosslinkers_force, added to the left bead only, at the crosslinker's place in the ascending-index merge of
 *   that bead's lists.  The site receives nothing (nothing ever moves it: :4559, :4616).  Overstretched count and
 *   longest length include it, taken at the left end.
 * With no sites set every result of every mhip_crosslinkers_* call is bit-identical to what it was.
 *
 * Deviations from the reference:
 *   1. candidate order: beads, then sites.  The reference walks the STK connectivity of the left bead, bead and site
 *      linkers mixed in creation order, which cannot be pinned; the probabilities are the same, the chosen entry for a
 *      given u is not.
 *   2. the periphery's own capture radius: rate 0 exactly beyond it (the bead rows' deviation, with a radius of its own)
 *   3. the uniform's 53-bit map (as for the bead rows; the reference draws openrand's double)
 *   4. the optional second unbinding rate k_off_p (the reference uses one rate and asks for two: :3419-3420)
 *   5. the sites are generated on the host (mundy_amd.synth.periphery_bind_sites; the reference's RANDOM mode,
 *      :2907-2963, with numpy's generator: openrand's stream is not pinned)
 *
 * mhip_crosslinkers_set_periphery_sites copies the P sites into the handle and drops the periphery candidates.  It may
 *   be called again with the same P to move the sites.  Refused before any HIP call (MHIP_ERR_INVALID_ARGUMENT): P == 0
 *   or P >= 2^31, anything not finite, a negative bind_rate or unbind_rate, k < 0, r < 0, capture_radius <= 0, a null
 *   handle or site_center, r <= 0 for FENE crosslinkers (r_p is then an r_max), a P other than an earlier call's.
 * mhip_crosslinkers_set_periphery_candidates: the first n rows of a CSR whose columns are site index + col_offset (a
 *   neighbour search over the concatenation of beads and sites: col_offset = n).  The rows are copied, the offset is
 *   subtracted and every row is sorted ascending by site index.  MHIP_ERR_RUNTIME before sites are set.  A column
 *   outside [0, P) after the subtraction is never followed.
 * mhip_crosslinkers_kmc_step_periphery: the step above.  events[0] = all binds, events[1] = all unbinds (overwritten);
 *   the number of periphery-bound crosslinkers after the step is ADDED to periphery_bound[0] (NULL: not counted);
 *   z_total as in mhip_crosslinkers_kmc_step.  MHIP_ERR_RUNTIME if either candidate list is missing.
 * mhip_crosslinkers_kmc_step on a handle with sites is this call with a NULL periphery_bound.  Once sites are set,
 *   mhip_crosslinkers_force, _get_state, _set_state and _renumber honour negative right heads; _renumber drops both
 *   candidate lists.  mhip_crosslinkers_create is unchanged: a periphery-bound initial state arrives through
 *   mhip_crosslinkers_set_state after the sites are set. */
#ifndef MUNDY_HIP_PERIPHERY_BINDING_H_
#define MUNDY_HIP_PERIPHERY_BINDING_H_

#include "mundy_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int mhip_crosslinkers_set_periphery_sites(mhip_crosslinkers_t handle, size_t P,
                                          const double* site_center /*[device] P x 3*/, double bind_rate, double k,
                                          double r, double unbind_rate, double capture_radius, mhip_stream_t stream);
int mhip_crosslinkers_set_periphery_candidates(mhip_crosslinkers_t handle, const int32_t* row_ptr /*[device] n + 1*/,
                                               const int32_t* col /*[device] num_entries*/, size_t num_entries,
                                               int32_t col_offset, mhip_stream_t stream);
int mhip_crosslinkers_kmc_step_periphery(mhip_crosslinkers_t handle, const double* center, double dt,
                                         const uint64_t* keys, uint64_t* counters, int* events /*[device] 2*/,
                                         int* periphery_bound /*[device] 1, added to; NULL ok*/, double* z_total,
                                         mhip_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MUNDY_HIP_PERIPHERY_BINDING_H_ */
