// backbone_collision_step_app.cpp -- the chromatin step with the HP1 app's excluded volume: frictionless Hertzian or WCA
// contacts between the backbone segments that join consecutive beads (HP1.cpp:4356-4496), the first term of the force
// field (:4737).  On spheres, driven from a C++ host program through mech::SphereChainStepper (mundy_hip/stepper.hpp)
// and its set_backbone_collision, with no Python and no torch in the process:
//   segment list -> segment contacts -> += Hookean spring forces -> U_ext = M F + U_brown [+ u_hydro] -> the mode's
//   contact stage -> Euler
// Usage: backbone_collision_step_app <input.bin> <steps> <mode> <law> <dt> <search_buffer> <k> <r0> <kt> <viscosity>
//                                    <E> <nu> <segment_radius> <skin> <epsilon> <sigma> <cutoff>
//   mode: none   no sphere contact (set_sphere_contacts(false)): U = U_ext, the reference's configuration
//         first  Hertzian sphere contact as the first term of the force field, with RPYC hydrodynamics every step
//         lcp    the sphere LCP after U_ext
//   law: hertz | wca (E and nu are also the sphere contact's material in mode first)
//   input.bin: uint64 n, uint64 m, then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m]; the springs are
//   the segments, and the end correction marks every segment with an end node that belongs to no other segment
// rng keys are the body indices, counters start at 0.  Prints one line per step and bit-level checksums of the final
// centres and U_ext, so the test can compare the whole trajectory with the Python driver's.
#include <cstring>
#include <string>

#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 18) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <none|first|lcp> <hertz|wca> <dt> <search_buffer> <k> <r0> <kt> "
                 "<viscosity> <E> <nu> <segment_radius> <skin> <epsilon> <sigma> <cutoff>\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1]);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  const std::string mode = argv[3], law = argv[4];
  if ((mode != "none" && mode != "first" && mode != "lcp") || (law != "hertz" && law != "wca")) {
    std::fprintf(stderr, "mode must be none, first or lcp; law must be hertz or wca\n");
    return 1;
  }
  const double dt = std::atof(argv[5]), buffer = std::atof(argv[6]), k = std::atof(argv[7]), r0 = std::atof(argv[8]),
               kt = std::atof(argv[9]), viscosity = std::atof(argv[10]);
  mhip_segment_contact_params prm{};
  prm.kind = law == "hertz" ? MHIP_SEGMENT_CONTACT_HERTZ : MHIP_SEGMENT_CONTACT_WCA;
  prm.youngs_modulus = std::atof(argv[11]);
  prm.poisson_ratio = std::atof(argv[12]);
  const double segment_radius = std::atof(argv[13]);
  prm.skin = std::atof(argv[14]);
  prm.epsilon = std::atof(argv[15]);
  prm.sigma = std::atof(argv[16]);
  prm.cutoff = std::atof(argv[17]);

  // "first or last element in chain": an end node that no other segment touches
  std::vector<int> degree(in.n, 0);
  for (int32_t b : in.pairs) ++degree[static_cast<size_t>(b)];
  std::vector<unsigned char> end_correction(in.m, 0);
  for (size_t e = 0; e < in.m; ++e)
    end_correction[e] = degree[static_cast<size_t>(in.pairs[2 * e])] == 1 ||
                        degree[static_cast<size_t>(in.pairs[2 * e + 1])] == 1;

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, MHIP_SPRING_HOOKEAN, k, r0, kt);
  st.set_backbone_collision(prm, in.pairs, {}, segment_radius, end_correction);
  if (mode == "none") st.set_sphere_contacts(false);
  if (mode == "first") {
    st.set_hertz_contact(prm.youngs_modulus, prm.poisson_ratio, /*contact_forces_in_force_stage=*/true);
    st.set_hydrodynamics(MHIP_HYDRO_RPYC, viscosity, 1);
  }
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats r = st.step();
    std::printf("STEP %d contacts %zu iterations %u converged %d rebuilt %d max_overlap %.17g max_spring_length %.17g "
                "segment_pairs %zu segment_contacts %zu segment_list_rebuilt %d max_segment_overlap %.17g\n",
                s, r.num_contacts, r.num_iters, r.converged ? 1 : 0, r.rebuilt ? 1 : 0, r.max_overlap,
                r.max_spring_length, r.num_segment_pairs, r.segment_contacts, r.segment_list_rebuilt ? 1 : 0,
                r.max_segment_overlap);
    if (r.springs_overstretched != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  std::printf("CHECKSUM center %016llx u_ext %016llx\n", checksum(st.center().download()),
              checksum_device(st.u_ext(), 6 * in.n));
  return 0;
}
