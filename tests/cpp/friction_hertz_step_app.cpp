// friction_hertz_step_app.cpp -- the frictional soft-contact step loop of the reference
// (CollidingOverdampedFrictionalSperm.cpp:1553-1777: neighbour list -> frictional Hertzian force per linker from the
// previous step's velocities and the linker's tangential history -> force / torque per body -> dry drag -> Euler update)
// on spherocylinders, driven from a C++ host program through mundy_hip/stepper.hpp (SpherocylinderStepper with
// set_hertz_contact + set_hertz_friction), with no Python and no torch in the process.
// Usage: friction_hertz_step_app <input.bin> <steps> <reorder_cell> <reorder_at_step> <dt> <youngs_modulus>
//                                <poisson_ratio> <mu> <gamma_n> <gamma_t> <density> <search_buffer>
//   input.bin: uint64 n, then doubles center[3n] quat[4n] radius[n] length[n] mob_trans[n] mob_rot[n]
//   reorder_cell <= 0: no Z-order reorder; otherwise one before step <reorder_at_step>
// Prints one line per step with bit-level checksums of the centres, the linker forces and the tangential displacements,
// so the test can compare the whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 13) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <reorder_cell> <reorder_at_step> <dt> <E> <nu> <mu> <gamma_n> <gamma_t> "
                 "<density> <search_buffer>\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  std::uint64_t n = 0;
  if (std::fread(&n, sizeof n, 1, f) != 1) return 2;
  const auto center = read_array<double>(f, 3 * n), quat = read_array<double>(f, 4 * n),
             radius = read_array<double>(f, n), length = read_array<double>(f, n), mob_t = read_array<double>(f, n),
             mob_r = read_array<double>(f, n);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double cell = std::atof(argv[3]);
  const int reorder_at = std::atoi(argv[4]);
  const double dt = std::atof(argv[5]), E = std::atof(argv[6]), nu = std::atof(argv[7]), mu = std::atof(argv[8]),
               gamma_n = std::atof(argv[9]), gamma_t = std::atof(argv[10]), density = std::atof(argv[11]),
               buffer = std::atof(argv[12]);

  mech::SpherocylinderStepper st(center, quat, radius, length, mob_t, mob_r, dt, buffer, convex::PGDConfig<double>{});
  try {
    st.set_hertz_friction(mu);  // the order of the calls is checked
    std::fprintf(stderr, "set_hertz_friction before set_hertz_contact was accepted\n");
    return 3;
  } catch (const std::logic_error&) {
  }
  st.set_hertz_contact(E, nu);
  st.set_hertz_friction(mu, gamma_n, gamma_t, density);
  for (int k = 0; k < steps; ++k) {
    if (cell > 0.0 && k == reorder_at) {
      const double lo[3] = {0.0, 0.0, 0.0};
      st.reorder_bodies(cell, lo);
    }
    const mech::StepStats s = st.step(true, false);
    const size_t C = s.num_contacts;
    std::printf("STEP %d contacts %zu max_overlap %.17g rebuilt %d sliding %zu carried %zu center %016llx force %016llx "
                "tang_disp %016llx\n",
                k, C, s.max_overlap, s.rebuilt ? 1 : 0, s.num_sliding, s.num_carried,
                checksum(st.center().download(), 3 * n), checksum(st.contact_force().download(), 3 * C),
                checksum(st.tang_disp().download(), 3 * C));
  }
  std::printf("CHECKSUM center %016llx quat %016llx\n", checksum(st.center().download(), 3 * n),
              checksum(st.quat().download(), 4 * n));
  return 0;
}
