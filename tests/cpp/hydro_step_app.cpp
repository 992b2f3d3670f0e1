// hydro_step_app.cpp -- the chromatin step with n-body hydrodynamics, as the reference's HP1 app runs it by default
// (HP1.cpp:4744-4803; compute_rpy_hydro :3942-4059), on spheres, driven from a C++ host program through
// mech::SphereChainStepper (mundy_hip/stepper.hpp) and its set_hydrodynamics, with no Python and no torch in the process:
//   neighbour list -> Hookean spring forces F -> U_ext = M F + U_brown -> every update_every-th step u_hydro = hydro(F)
//   -> U_ext += u_hydro -> contacts, q = sep + dt D^T U_ext -> BBPGD from lambda = 0 -> U = U_ext + M D lambda -> Euler
// Usage: hydro_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every>
//   kind: 0 stokes, 1 rpy, 2 rpyc (MHIP_HYDRO_*); the hydrodynamic radii are the beads' own
//   input.bin: uint64 n, uint64 m, then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m]
// rng keys are the body indices, counters start at 0.  Prints one line per step and a bit-level checksum of the final
// centres, so the test can compare the whole trajectory with the Python driver's.
#include <chrono>

#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every>\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1]);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), viscosity = std::atof(argv[8]);
  const int kind = std::atoi(argv[9]), update_every = std::atoi(argv[10]);
  if (update_every < 1) {
    std::fprintf(stderr, "update_every must be >= 1\n");
    return 1;
  }

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */,
                              in.pairs, MHIP_SPRING_HOOKEAN, k, r0, kt);
  st.set_hydrodynamics(kind, viscosity, update_every);
  for (int s = 0; s < steps; ++s) {
    const auto t0 = std::chrono::steady_clock::now();
    const mech::StepStats r = st.step();
    const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("STEP %d contacts %zu iterations %u max_spring_length %.17g rebuilt %d converged %d ms %.3f\n", s,
                r.num_contacts, r.num_iters, r.max_spring_length, r.rebuilt ? 1 : 0, r.converged ? 1 : 0, ms);
    if (r.springs_overstretched != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  std::printf("CHECKSUM center %016llx\n", checksum(st.center().download()));
  return 0;
}
