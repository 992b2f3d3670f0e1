// hydro_solve_step_app.cpp -- the chromatin step whose LCP is solved against the hydrodynamic mobility, as the reference's
// newer chromatin app resolves collisions (resolve_collisions over an ApplyMobilityOp, NgpHP1.cpp:1487-1645, with
// SphereRpyMobilityOp :677-701 or, inside a periphery, SphereConfinedRpyMobilityOp :703-766): the step of
// hydro_step_app.cpp / hydro_periphery_step_app.cpp with set_hydrodynamic_solve(true), driven from a C++ host program
// through mech::SphereChainStepper (mundy_hip/stepper.hpp), with no Python and no torch in the process:
//   neighbour list -> Hookean spring forces F -> U_ext = M F + U_brown -> every update_every-th step u_hydro = hydro(F)
//   (+ correction(F)) -> U_ext += u_hydro -> contacts -> q = sep + dt D^T U_ext -> BBPGD on dt D^T M_h D from lambda = 0,
//   M_h = m_t + hydro_kind (+ the periphery's correction) at the current positions -> U = U_ext + M_h D lambda -> Euler
// Usage: hydro_solve_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every>
//                             <in_solve> <max_iters> <tol> [<order>]
//   kind: 1 rpy, 2 rpyc (MHIP_HYDRO_*); the hydrodynamic radii are the beads' own; in_solve: 0 the dry solve, 1 this one
//   input.bin: uint64 n, uint64 m, then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m], then
//              uint64 S, uint64 skip_same_index, then doubles points[3S] weights[S] normals[3S] (S = 0: free space)
//   order (optional; the setter sequences the stepper refuses, for the tests): solve_first (set_hydrodynamic_solve before
//   set_hydrodynamics), after_hertz (after set_hertz_contact), hertz_later (set_hertz_contact afterwards), no_spheres
//   (set_sphere_contacts(false) afterwards), stokes_later (set_hydrodynamics with the Stokeslet afterwards).  A refusal
//   of the stepper is printed as "REFUSED <what>" on stderr and ends the program with status 2.
// rng keys are the body indices, counters start at 0.  Prints one line per step and a bit-level checksum of the final
// centres and of the last step's multipliers, so the test can compare the whole trajectory with the Python driver's.
#include <chrono>
#include <stdexcept>
#include <string>

#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 14) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every> "
                 "<in_solve> <max_iters> <tol> [<order>]\n",
                 argv[0]);
    return 1;
  }
  const ChainInput in = read_chain_input(argv[1]);
  const auto surf = read_array<std::uint64_t>(in.file, 2);
  const size_t S = surf[0];
  const bool skip_same_index = surf[1] != 0;
  const auto points = read_array<double>(in.file, 3 * S), weights = read_array<double>(in.file, S),
             normals = read_array<double>(in.file, 3 * S);
  std::fclose(in.file);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), viscosity = std::atof(argv[8]);
  const int kind = std::atoi(argv[9]), update_every = std::atoi(argv[10]), in_solve = std::atoi(argv[11]);
  const unsigned max_iters = static_cast<unsigned>(std::atoi(argv[12]));
  const double tol = std::atof(argv[13]);
  if (update_every < 1) {
    std::fprintf(stderr, "update_every must be >= 1\n");
    return 1;
  }

  mech::SphereChainStepper st(in.center, in.radius, in.mob_trans, dt, buffer, {max_iters, tol}, in.pairs,
                              MHIP_SPRING_HOOKEAN, k, r0, kt);
  const std::string order = argc > 14 ? argv[14] : "";
  try {
    if (order == "solve_first") st.set_hydrodynamic_solve(true);
    if (order == "after_hertz") st.set_hertz_contact(1000.0, 0.3, true);
    st.set_hydrodynamics(kind, viscosity, update_every);
    if (S > 0) {
      st.set_hydro_periphery(points, weights, normals, skip_same_index);
      std::printf("PERIPHERY nodes %zu min_pivot %.17g\n", S, st.min_pivot());
    }
    st.set_hydrodynamic_solve(in_solve != 0);
    if (order == "hertz_later") st.set_hertz_contact(1000.0, 0.3, true);
    if (order == "no_spheres") {
      const mhip_segment_contact_params params{MHIP_SEGMENT_CONTACT_HERTZ, 0.5, 1000.0, 0.3, 1.0, 1.0, 1.12246204831};
      st.set_backbone_collision(params, in.pairs, {}, 0.5, {});
      st.set_sphere_contacts(false);
    }
    if (order == "stokes_later") st.set_hydrodynamics(MHIP_HYDRO_STOKES, viscosity, update_every);
  } catch (const std::logic_error& e) {  // (std::invalid_argument is one)
    std::fprintf(stderr, "REFUSED %s\n", e.what());
    return 2;
  }
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
  std::vector<double> lambda = st.lambda().download();
  lambda.resize(st.num_lambda());
  std::printf("CHECKSUM center %016llx lambda %016llx\n", checksum(st.center().download()), checksum(lambda));
  return 0;
}
