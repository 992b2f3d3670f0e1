// bending_step_app.cpp -- the semiflexible chain step from a C++ host program through mech::SphereChainStepper
// (mundy_hip/stepper.hpp), with no Python and no torch in the process: the chain step of chain_step_app with angular
// springs (AngularSpringsKernel.cpp:107-197; mundy_hip_bending.h) and a choice of backbone bond.
//   neighbour list -> springs -> angular springs -> U_ext = M F + U_brown -> contacts, LCP -> Euler update
// Usage: bending_step_app <input.bin> <steps> <dt> <search_buffer> <spring_type> <k> <r> <kt> <k_angle> <rest_angle>
//                         [<wca_epsilon> <wca_sigma>]
//   input.bin: uint64 n, uint64 m, uint64 ma, then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m], then
//   int32 triplets[3 ma] = (end, end, centre)
//   spring_type: 0 Hookean (r = rest length), 2 FENE-WCA (r = r_max; epsilon and sigma default to 1)
// rng keys are the body indices, counters start at 0.  Prints one line per step and bit-level checksums of the final
// centres and of the last step's force, so the test can compare the whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

static int run(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <spring_type> <k> <r> <kt> <k_angle> <rest_angle> "
                 "[<wca_epsilon> <wca_sigma>]\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1], 3);
  const std::vector<int32_t> triplets = read_array<int32_t>(in.file, 3 * in.counts[2]);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]), type = std::atoi(argv[5]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[6]), r = std::atof(argv[7]),
               kt = std::atof(argv[8]), k_angle = std::atof(argv[9]), rest_angle = std::atof(argv[10]);

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, type, k, r, kt);
  if (argc >= 13) st.set_spring_wca(std::atof(argv[11]), std::atof(argv[12]));
  st.set_angular_springs(triplets, k_angle, rest_angle);
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats q = st.step();
    std::printf("STEP %d contacts %zu iterations %u max_spring_length %.17g springs_overstretched %d "
                "max_angle_deviation %.17g angular_degenerate %d rebuilt %d converged %d\n",
                s, q.num_contacts, q.num_iters, q.max_spring_length, q.springs_overstretched, q.max_angle_deviation,
                q.angular_degenerate, q.rebuilt ? 1 : 0, q.converged ? 1 : 0);
    if (q.angular_degenerate != 0 || (type != MHIP_SPRING_FENEWCA && q.springs_overstretched != 0)) {
      std::fprintf(stderr, "a spring without force\n");
      return 3;
    }
  }
  std::printf("CHECKSUM center %016llx force %016llx\n", checksum(st.center().download()),
              checksum_device(st.force(), 3 * st.num_bodies()));
  return 0;
}

/// a refusal of the library (std::invalid_argument from mundy_hip::check) ends the program with status 4 and its message
int main(int argc, char** argv) {
  try {
    return run(argc, argv);
  } catch (const std::invalid_argument& e) {
    std::fprintf(stderr, "REFUSED %s\n", e.what());
    return 4;
  }
}
