// filament_contact_app.cpp -- the whole force stage of the reference's colliding sperm app (frictional Hertzian contacts
// between the filament segments, then the centerline-twist rod forces, CollidingOverdampedFrictionalSperm.cpp:1999-2027)
// from a C++ host program through the C ABI and mundy_hip/stepper.hpp, with no Python and no torch in the process:
//   save velocity -> advance -> segment view, list -> linker pass + reduction -> edge pass + node pass -> node drag
// Usage: filament_contact_app <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist>
//                             <monolayer> <skin> <contact E> <contact nu> <mu> <normal damping> <tangential damping>
//                             <density> <history dt, negative = dt> <bonded exclusion>
//   input.bin: uint64 F, uint64 N, int32 node_ptr[F + 1], then doubles center[3N] twist[N] edge_orientation[4N]
//   radius[N] rest_curvature[3N] arclength[N] phase[F]
// Prints the statistics of every step as hexadecimal floats and bit-level checksums of the final state, so the test
// can compare the whole trajectory with the Python stepper's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 23) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <E> <nu> <l0> <eta> <A> <k> <omega> <wave> <disable_twist> "
                 "<monolayer> <skin> <contact E> <contact nu> <mu> <normal damping> <tangential damping> <density> "
                 "<history dt> <bonded exclusion>\n",
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

  mhip_filament_contact_params cp{};
  cp.skin = std::atof(argv[14]);
  cp.youngs_modulus = std::atof(argv[15]);
  cp.poisson_ratio = std::atof(argv[16]);
  cp.mu = std::atof(argv[17]);
  cp.normal_damping = std::atof(argv[18]);
  cp.tangential_damping = std::atof(argv[19]);
  cp.density = std::atof(argv[20]);
  cp.history_dt = std::atof(argv[21]);
  cp.bonded_exclusion = std::atoi(argv[22]);

  mech::FilamentStepper stepper(node_ptr, center, twist, orient, radius, rest, arclength, phase, prm);
  stepper.set_contacts(cp);
  for (int s = 0; s < steps; ++s) {
    const mech::StepStats st = stepper.step(dt);
    std::printf("STEP %d max_stretch %a max_curvature_deviation %a num_pairs %zu max_overlap %a num_sliding %zu rebuilt %d\n",
                s, st.max_stretch, st.max_curvature_deviation, st.num_contacts, st.max_overlap, st.num_sliding,
                st.rebuilt ? 1 : 0);
  }
  const mhip_filament_fields fl = stepper.fields();
  std::printf("CHECKSUM center %016llx\n", checksum_device(fl.center, 3 * N));
  std::printf("CHECKSUM twist %016llx\n", checksum_device(fl.twist, N));
  std::printf("CHECKSUM velocity %016llx\n", checksum_device(fl.velocity, 3 * N));
  std::printf("CHECKSUM twist_velocity %016llx\n", checksum_device(fl.twist_velocity, N));
  std::printf("CHECKSUM edge_orientation %016llx\n", checksum_device(fl.edge_orientation, 4 * N));
  const mhip_filament_contact_fields cf = stepper.contact_fields();
  std::printf("CHECKSUM node_force %016llx\n", checksum_device(cf.node_force, 3 * N));
  if (cf.num_pairs) std::printf("CHECKSUM tang_disp %016llx\n", checksum_device(cf.tang_disp, 3 * cf.num_pairs));
  return 0;
}
