// filament_inertial_app.cpp -- the inertial sperm apps' step (CollidingFrictionalSperm.cpp:1890-1948, CollidingSperm.cpp:
// the Newmark predictor / corrector around the centerline-twist forces, optionally the stiffness ramp of `equilibriate`
// before it and contacts between the segments inside it) from a C++ host program through the C ABI and
// mundy_hip/stepper.hpp, with no Python and no torch in the process:
//   [equilibrate] -> per step: [save velocity] -> predict -> [segment view, list, linker pass + reduction] -> edge pass +
//   node pass -> correct (+ kinetic energy)
// Usage: filament_inertial_app <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist>
//                              <monolayer> <density> <damping kind> <c_t> <c_r> <fixed filament, -1 = none>
//                              <relaxed E, 0 = no ramp> <threshold> <growth> <poll every>
//                              [<skin> <contact E> <contact nu> <mu> <normal damping> <tangential damping>
//                               <contact density> <history dt, negative = dt> <bonded exclusion> <law>]
//   input.bin: uint64 F, uint64 N, int32 node_ptr[F + 1], then doubles center[3N] twist[N] edge_orientation[4N]
//   radius[N] rest_curvature[3N] arclength[N] phase[F]
// Prints the steps per level of the ramp, the statistics of every step as hexadecimal floats and bit-level checksums of
// the final state, so the test can compare the whole trajectory with the Python stepper's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc != 23 && argc != 33) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist> "
                 "<monolayer> <density> <damping kind> <c_t> <c_r> <fixed filament> <relaxed E> <threshold> <growth> "
                 "<poll every> [<skin> <contact E> <contact nu> <mu> <normal damping> <tangential damping> "
                 "<contact density> <history dt> <bonded exclusion> <law>]\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const auto fn = read_array<std::uint64_t>(f, 2);
  const size_t F = fn[0], N = fn[1];
  const auto node_ptr = read_array<int32_t>(f, F + 1);
  const auto center = read_array<double>(f, 3 * N), twist = read_array<double>(f, N),
             orient = read_array<double>(f, 4 * N), radius = read_array<double>(f, N),
             rest = read_array<double>(f, 3 * N), arclength = read_array<double>(f, N), phase = read_array<double>(f, F);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]);
  mhip_filament_params prm{};
  prm.youngs_modulus = std::atof(argv[4]);
  prm.poisson_ratio = std::atof(argv[5]);
  prm.rest_length = std::atof(argv[6]);
  prm.viscosity = std::atof(argv[7]);
  prm.wave_amplitude = std::atof(argv[8]);
  prm.wave_number = std::atof(argv[9]);
  prm.wave_frequency = std::atof(argv[10]);
  prm.wave = std::atoi(argv[11]);
  prm.disable_twist = std::atoi(argv[12]);
  prm.monolayer = std::atoi(argv[13]);
  mhip_filament_inertial_params ip{};
  ip.density = std::atof(argv[14]);
  ip.damping_kind = std::atoi(argv[15]);
  ip.translational_damping = std::atof(argv[16]);
  ip.twist_damping = std::atof(argv[17]);
  const long fixed = std::atol(argv[18]);
  const double relaxed = std::atof(argv[19]), threshold = std::atof(argv[20]), growth = std::atof(argv[21]);
  const size_t poll_every = static_cast<size_t>(std::atol(argv[22]));

  try {
    mech::FilamentStepper stepper(node_ptr, center, twist, orient, radius, rest, arclength, phase, prm);
    std::vector<unsigned char> mask;
    if (fixed >= 0) {
      mask.assign(F, 0);
      mask.at(static_cast<size_t>(fixed)) = 1;
    }
    stepper.set_inertial(ip, mask);
    if (argc == 33) {
      mhip_filament_contact_params cp{};
      cp.skin = std::atof(argv[23]);
      cp.youngs_modulus = std::atof(argv[24]);
      cp.poisson_ratio = std::atof(argv[25]);
      cp.mu = std::atof(argv[26]);
      cp.normal_damping = std::atof(argv[27]);
      cp.tangential_damping = std::atof(argv[28]);
      cp.density = std::atof(argv[29]);
      cp.history_dt = std::atof(argv[30]);
      cp.bonded_exclusion = std::atoi(argv[31]);
      stepper.set_contacts(cp);
      stepper.set_contact_law(std::atoi(argv[32]));
    }
    if (relaxed > 0.0) {
      const std::vector<size_t> levels = stepper.equilibrate(dt, relaxed, threshold, growth, poll_every);
      for (size_t k = 0; k < levels.size(); ++k) std::printf("LEVEL %zu steps %zu\n", k, levels[k]);
    }
    for (int s = 0; s < steps; ++s) {
      const mech::StepStats st = stepper.step(dt);
      std::printf("STEP %d max_stretch %a max_curvature_deviation %a kinetic_energy %a num_pairs %zu max_overlap %a "
                  "num_sliding %zu rebuilt %d\n",
                  s, st.max_stretch, st.max_curvature_deviation, st.kinetic_energy, st.num_contacts, st.max_overlap,
                  st.num_sliding, st.rebuilt ? 1 : 0);
    }
    const mhip_filament_fields fl = stepper.fields();
    const mhip_filament_inertial_fields il = stepper.inertial_fields();
    std::printf("CHECKSUM center %016llx\n", checksum_device(fl.center, 3 * N));
    std::printf("CHECKSUM twist %016llx\n", checksum_device(fl.twist, N));
    std::printf("CHECKSUM velocity %016llx\n", checksum_device(fl.velocity, 3 * N));
    std::printf("CHECKSUM twist_velocity %016llx\n", checksum_device(fl.twist_velocity, N));
    std::printf("CHECKSUM acceleration %016llx\n", checksum_device(il.acceleration, 3 * N));
    std::printf("CHECKSUM twist_acceleration %016llx\n", checksum_device(il.twist_acceleration, N));
    std::printf("CHECKSUM edge_orientation %016llx\n", checksum_device(fl.edge_orientation, 4 * N));
    if (argc == 33) {
      const mhip_filament_contact_fields cf = stepper.contact_fields();
      std::printf("CHECKSUM node_force %016llx\n", checksum_device(cf.node_force, 3 * N));
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "filament_inertial_app: %s\n", e.what());
    return 3;
  }
  return 0;
}
