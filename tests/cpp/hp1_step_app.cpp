// hp1_step_app.cpp -- the whole HP1 chromatin step (HP1.cpp:4728-4803) in one mech::SphereChainStepper
// (mundy_hip/stepper.hpp), every optional stage chosen by a letter, with no Python and no torch in the process; the
// case is tests/hp1_case.py's, which the Python stepper runs with the same letters:
//   X crosslinkers (set_crosslinkers)              Y periphery bind sites (set_periphery_sites; needs X)
//   P the nuclear wall, a sphere (set_periphery)   A active dipoles (set_active_springs)
//   U hydrodynamics, RPYC (set_hydrodynamics)      W the periphery's no-slip correction (set_hydro_periphery; needs U)
//   E an external force, added by this program     H the Hertz contact, its force the first term of the force field
// (H without U has no counterpart in pipeline.ContactStepper, whose first-term order is a key of hydrodynamics=.)
// Without E the step is step().  With E the stages run by hand, the way a host program adds a term of its own:
//   neighbors() -> [contact_forces()] -> forces() -> force() += external force -> external_velocity() -> resolve()
// Usage: hp1_step_app <input.bin> <steps> <letters or -> <dt> <search_buffer> <k> <r0> <kt>
//            <xl_k> <xl_r0> <bind_rate> <unbind_rate> <xl_kt> <capture_radius> <xl_skin>
//            <p_bind_rate> <p_k> <p_r0> <p_unbind_rate> <p_capture_radius> <wall_radius> <wall_k>
//            <sigma> <kon> <koff> <viscosity> <update_every> <youngs_modulus> <poisson_ratio>
//   input.bin: uint64 n, m (springs), mx (crosslinkers), P (periphery sites), ma (active springs), S (quadrature
//   nodes), 1; doubles center[3n] radius[n] mob_trans[n]; int32 pairs[2m]; then, in this order: int32 left[mx], bytes
//   sites[n], doubles site_center[3P], int32 active_pairs[2 ma], doubles points[3S] weights[S] normals[3S],
//   doubles external_force[3n].  Every array is in the file whatever the letters; they decide what is used.
// Every crosslinker starts singly bound; rng keys are the body / crosslinker / active spring indices, counters start
// at 0.  Prints one line per step with every integer and flag of StepStats and its four maxima (%.17g), then bit-level
// checksums of the final centres, right heads, active states and switching times, and of the last step's U_ext.
#include <cstring>

#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 30) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <letters of XYPAUWEH or -> <dt> <search_buffer> <k> <r0> <kt> <xl_k> "
                 "<xl_r0> <bind_rate> <unbind_rate> <xl_kt> <capture_radius> <xl_skin> <p_bind_rate> <p_k> <p_r0> "
                 "<p_unbind_rate> <p_capture_radius> <wall_radius> <wall_k> <sigma> <kon> <koff> <viscosity> "
                 "<update_every> <youngs_modulus> <poisson_ratio>\n",
                 argv[0]);
    return 1;
  }
  const char* letters = argv[3];
  if (std::strspn(letters, "XYPAUWEH-") != std::strlen(letters)) {
    std::fprintf(stderr, "stage letters: some of XYPAUWEH, or -\n");
    return 1;
  }
  const auto on = [letters](char c) { return std::strchr(letters, c) != nullptr; };
  if ((on('Y') && !on('X')) || (on('W') && !on('U'))) {
    std::fprintf(stderr, "stage letters: Y needs X, W needs U\n");
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1], 7);
  const size_t n = in.n, mx = in.counts[2], P = in.counts[3], ma = in.counts[4], S = in.counts[5];
  const auto left = read_array<int32_t>(in.file, mx);
  const auto sites = read_array<unsigned char>(in.file, n);
  const auto site_points = read_array<double>(in.file, 3 * P);
  const auto active_pairs = read_array<int32_t>(in.file, 2 * ma);
  const auto points = read_array<double>(in.file, 3 * S), weights = read_array<double>(in.file, S),
             normals = read_array<double>(in.file, 3 * S);
  const auto external = read_array<double>(in.file, 3 * n);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  double v[26];
  for (int k = 0; k < 26; ++k) v[k] = std::atof(argv[4 + k]);
  const double dt = v[0], buffer = v[1], k = v[2], r0 = v[3], kt = v[4], xl_k = v[5], xl_r0 = v[6], bind_rate = v[7],
               unbind_rate = v[8], xl_kt = v[9], cap = v[10], xl_skin = v[11], p_bind_rate = v[12], p_k = v[13],
               p_r0 = v[14], p_unbind_rate = v[15], p_cap = v[16], wall_radius = v[17], wall_k = v[18], sigma = v[19],
               kon = v[20], koff = v[21], viscosity = v[22], youngs_modulus = v[24], poisson_ratio = v[25];
  const int update_every = static_cast<int>(v[23]);

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, MHIP_SPRING_HOOKEAN, k, r0, kt);
  if (on('H')) st.set_hertz_contact(youngs_modulus, poisson_ratio, /*contact_forces_in_force_stage=*/true);
  if (on('X')) st.set_crosslinkers(left, sites, MHIP_SPRING_HOOKEAN, xl_k, xl_r0, bind_rate, unbind_rate, xl_kt, cap, xl_skin);
  if (on('Y')) st.set_periphery_sites(site_points, p_bind_rate, p_k, p_r0, p_unbind_rate, p_cap);
  if (on('P')) {
    mhip_periphery wall{};
    wall.shape = MHIP_PERIPHERY_SPHERE;
    wall.radii[0] = wall.radii[1] = wall.radii[2] = wall_radius;
    wall.k = wall_k;
    wall.quat[0] = 1.0;
    st.set_periphery(wall);
  }
  if (on('A')) st.set_active_springs(active_pairs, sigma, kon, koff);
  if (on('U')) st.set_hydrodynamics(MHIP_HYDRO_RPYC, viscosity, update_every);
  if (on('W')) {
    st.set_hydro_periphery(points, weights, normals, /*skip_same_index=*/true);
    std::printf("PERIPHERY nodes %zu min_pivot %.17g\n", S, st.min_pivot());
  }
  const DeviceVector ext(external);
  long long bound = 0;
  for (int s = 0; s < steps; ++s) {
    mech::StepStats r;
    if (on('E')) {
      st.neighbors();
      if (on('H')) st.contact_forces();
      st.forces();
      check(mhip_axpby(3 * n, 1.0, ext.data(), 1.0, st.force(), nullptr));
      st.external_velocity();
      r = st.resolve();
    } else {
      r = st.step();
    }
    bound += r.crosslinker_binds - r.crosslinker_unbinds;
    std::printf("STEP %d contacts %zu iterations %u converged %d rebuilt %d born %zu sliding %zu carried %zu "
                "springs_overstretched %d binds %d unbinds %d bound %lld periphery_bound %d crosslinkers_overstretched %d "
                "colliding %d active %d on %d off %d max_overlap %.17g max_spring_length %.17g max_crosslinker_length "
                "%.17g max_periphery_overlap %.17g\n",
                s, r.num_contacts, r.num_iters, r.converged ? 1 : 0, r.rebuilt ? 1 : 0, r.num_born, r.num_sliding,
                r.num_carried, r.springs_overstretched, r.crosslinker_binds, r.crosslinker_unbinds, bound,
                r.crosslinker_periphery_bound, r.crosslinkers_overstretched, r.periphery_colliding, r.active_springs,
                r.active_switches_on, r.active_switches_off, r.max_overlap, r.max_spring_length,
                r.max_crosslinker_length, r.max_periphery_overlap);
  }
  std::printf("CHECKSUM center %016llx\n", checksum(st.center().download()));
  if (on('X')) std::printf("CHECKSUM right %016llx\n", checksum(st.crosslinkers()->right_heads()));
  if (on('A'))
    std::printf("CHECKSUM state %016llx next_time %016llx\n", checksum(st.active_springs()->states()),
                checksum(st.active_springs()->next_times()));
  std::printf("CHECKSUM u_ext %016llx\n", checksum_device(st.u_ext(), 6 * n));
  return 0;
}
