// nucleus_step_app.cpp -- the chromatin step of the reference's HP1 app inside its nucleus: bead-spring chains with
// thermal noise, confined by the periphery (HP1.cpp:4063-4284) and driven by the active euchromatin force dipoles
// (:3770-3853, :4286-4354), from a C++ host program through mech::SphereChainStepper (mundy_hip/stepper.hpp) and its
// set_periphery + set_active_springs, with no Python and no torch in the process.  The force stage in the
// reference's order (:4733-4741):
//   neighbour list -> active sampling -> Hookean backbone forces -> periphery force -> active force dipoles
//   -> U_ext = M F + U_brown -> contacts, q = sep + dt D^T U_ext -> BBPGD from lambda = 0 -> U = U_ext + M D lambda
//   -> Euler update -> the active springs' timers advance by dt
// Usage: nucleus_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <shape> <R0> <R1> <R2> <K>
//                         <cx> <cy> <cz> <qw> <qx> <qy> <qz> <sigma> <kon> <koff>
//   input.bin: uint64 n, uint64 m (springs), uint64 ma (active springs), then doubles center[3n] radius[n]
//   mob_trans[n], then int32 pairs[2m], int32 active_pairs[2ma]
// rng keys are the body / active spring indices, counters start at 0.  Prints one line per step and bit-level checksums
// of the final centres and of the active springs' state, so the test can compare the whole trajectory with the Python
// driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 23) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <shape> <R0> <R1> <R2> <K> <cx> <cy> "
                 "<cz> <qw> <qx> <qy> <qz> <sigma> <kon> <koff>\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1], 3);
  const auto active_pairs = read_array<int32_t>(in.file, 2 * in.counts[2]);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]);
  mhip_periphery wall{};
  wall.shape = std::atoi(argv[8]);
  for (int a = 0; a < 3; ++a) wall.radii[a] = std::atof(argv[9 + a]);
  wall.k = std::atof(argv[12]);
  for (int a = 0; a < 3; ++a) wall.center[a] = std::atof(argv[13 + a]);
  for (int a = 0; a < 4; ++a) wall.quat[a] = std::atof(argv[16 + a]);
  const double sigma = std::atof(argv[20]), kon = std::atof(argv[21]), koff = std::atof(argv[22]);

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, MHIP_SPRING_HOOKEAN, k, r0, kt);
  st.set_periphery(wall);
  st.set_active_springs(active_pairs, sigma, kon, koff);
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats r = st.step();
    std::printf("STEP %d contacts %zu iterations %u colliding %d active %d on %d off %d rebuilt %d converged %d\n", s,
                r.num_contacts, r.num_iters, r.periphery_colliding, r.active_springs, r.active_switches_on,
                r.active_switches_off, r.rebuilt ? 1 : 0, r.converged ? 1 : 0);
    if (r.springs_overstretched != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  std::printf("CHECKSUM center %016llx\n", checksum(st.center().download()));
  std::printf("CHECKSUM state %016llx\n", checksum(st.active_springs()->states()));
  std::printf("CHECKSUM next_time %016llx\n", checksum(st.active_springs()->next_times()));
  return 0;
}
