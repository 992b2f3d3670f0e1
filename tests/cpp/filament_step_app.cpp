// filament_step_app.cpp -- the elastic half of the reference's sperm apps (centerline-twist rod forces, node drag and
// the node update with its two constraints, CollidingOverdampedFrictionalSperm.cpp:1999-2027) from a C++ host program
// through the C ABI and mundy_hip/stepper.hpp, with no Python and no torch in the process:
//   advance (disable_twist, monolayer, old <-> new, x += dt v) -> edge pass + node pass -> node drag
// Usage: filament_step_app <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist>
//                          <monolayer>
//   input.bin: uint64 F, uint64 N, int32 node_ptr[F + 1], then doubles center[3N] twist[N] edge_orientation[4N]
//   radius[N] rest_curvature[3N] arclength[N] phase[F]
// Prints the two statistics of every step as hexadecimal floats and bit-level checksums of the final state, so the test
// can compare the whole trajectory with the Python stepper's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 14) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist> "
                 "<monolayer>\n",
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

  mech::FilamentStepper stepper(node_ptr, center, twist, orient, radius, rest, arclength, phase, prm);
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats st = stepper.step(dt);
    std::printf("STEP %d max_stretch %a max_curvature_deviation %a\n", s, st.max_stretch, st.max_curvature_deviation);
  }
  const mhip_filament_fields fl = stepper.fields();
  std::printf("CHECKSUM center %016llx\n", checksum_device(fl.center, 3 * N));
  std::printf("CHECKSUM twist %016llx\n", checksum_device(fl.twist, N));
  std::printf("CHECKSUM velocity %016llx\n", checksum_device(fl.velocity, 3 * N));
  std::printf("CHECKSUM twist_velocity %016llx\n", checksum_device(fl.twist_velocity, N));
  std::printf("CHECKSUM edge_orientation %016llx\n", checksum_device(fl.edge_orientation, 4 * N));
  return 0;
}
