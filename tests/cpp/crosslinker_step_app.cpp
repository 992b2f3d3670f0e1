// crosslinker_step_app.cpp -- the chromatin step of the reference's HP1 app with its crosslinker kinetic Monte Carlo
// stage (HP1.cpp:4728-4739) on spheres, driven from a C++ host program through mech::SphereChainStepper
// (mundy_hip/stepper.hpp) and its set_crosslinkers, with no Python and no torch in the process:
//   neighbour list, and the candidate list of the crosslinkers (its own search: sources the beads that carry a
//   crosslinker, targets the bind sites) -> KMC at the positions of the start of the step -> Hookean backbone forces
//   + the doubly bound crosslinkers as springs -> U_ext = M F + U_brown -> contacts, q = sep + dt D^T U_ext -> BBPGD
//   from lambda = 0 -> U = U_ext + M D lambda -> Euler update
// Usage: crosslinker_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt>
//                             <xl_k> <xl_r0> <bind_rate> <unbind_rate> <xl_kt> <capture_radius> <xl_skin>
//   input.bin: uint64 n, uint64 m (springs), uint64 mx (crosslinkers), then doubles center[3n] radius[n] mob_trans[n],
//   then int32 pairs[2m], int32 left[mx], bytes sites[n]
// Every crosslinker starts singly bound; rng keys are the body / crosslinker indices, counters start at 0, ids are the
// body indices.  Prints one line per step and bit-level checksums of the final centres and right heads, so the test
// can compare the whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 15) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <xl_k> <xl_r0> <bind_rate> "
                 "<unbind_rate> <xl_kt> <capture_radius> <xl_skin>\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1], 3);
  const size_t mx = in.counts[2];
  const auto left = read_array<int32_t>(in.file, mx);
  const auto sites = read_array<unsigned char>(in.file, in.n);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), xl_k = std::atof(argv[8]), xl_r0 = std::atof(argv[9]),
               bind_rate = std::atof(argv[10]), unbind_rate = std::atof(argv[11]), xl_kt = std::atof(argv[12]),
               cap = std::atof(argv[13]), xl_skin = std::atof(argv[14]);

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, MHIP_SPRING_HOOKEAN, k, r0, kt);
  st.set_crosslinkers(left, sites, MHIP_SPRING_HOOKEAN, xl_k, xl_r0, bind_rate, unbind_rate, xl_kt, cap, xl_skin);
  long long bound = 0;
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats r = st.step();
    bound += r.crosslinker_binds - r.crosslinker_unbinds;
    std::printf("STEP %d contacts %zu iterations %u bound %lld binds %d unbinds %d rebuilt %d converged %d\n", s,
                r.num_contacts, r.num_iters, bound, r.crosslinker_binds, r.crosslinker_unbinds, r.rebuilt ? 1 : 0,
                r.converged ? 1 : 0);
    if (r.springs_overstretched != 0 || r.crosslinkers_overstretched != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  std::printf("CHECKSUM center %016llx\n", checksum(st.center().download()));
  std::printf("CHECKSUM right %016llx\n", checksum(st.crosslinkers()->right_heads()));
  return 0;
}
