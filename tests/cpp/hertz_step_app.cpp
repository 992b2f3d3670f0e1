// hertz_step_app.cpp -- the soft-contact step loop of the reference's production app (Bacteria.cpp:755-848,
// :1033-1080: neighbour list -> Hertz force per linker -> force / torque per body -> dry drag -> Euler update) on
// spherocylinders, driven from a C++ host program through mundy_hip/stepper.hpp (SpherocylinderStepper in Hertz
// mode), with no Python and no torch in the process.
// Usage: hertz_step_app <input.bin> <steps> <reorder_cell> <periodic_box_edge> <dt> <youngs_modulus> <poisson_ratio>
//   input.bin: uint64 n, then doubles center[3n] quat[4n] radius[n] length[n] mob_trans[n] mob_rot[n]
//   reorder_cell <= 0: no Z-order reorder; periodic_box_edge <= 0: free space
// Prints one line per step and a bit-level checksum of the final centres / orientations, so the test can compare the
// whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 8) {
    std::fprintf(stderr, "Usage: %s <input.bin> <steps> <reorder_cell> <periodic_box_edge> <dt> <E> <nu>\n", argv[0]);
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
  const double cell = std::atof(argv[3]), edge = std::atof(argv[4]), dt = std::atof(argv[5]);
  const double E = std::atof(argv[6]), nu = std::atof(argv[7]);

  const double box[3] = {edge, edge, edge};
  mech::SpherocylinderStepper st(center, quat, radius, length, mob_t, mob_r, dt, /*search_buffer=*/0.1,
                                 convex::PGDConfig<double>{}, edge > 0.0 ? box : nullptr);
  st.set_hertz_contact(E, nu);
  if (cell > 0.0) {
    const double lo[3] = {0.0, 0.0, 0.0};
    st.reorder_bodies(cell, lo);
  }
  for (int k = 0; k < steps; ++k) {
    const auto t0 = std::chrono::steady_clock::now();
    const mech::StepStats s = st.step(true, false);
    const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("STEP %d contacts %zu max_overlap %.17g rebuilt %d iterations %u converged %d ms %.3f\n", k,
                s.num_contacts, s.max_overlap, s.rebuilt ? 1 : 0, s.num_iters, s.converged ? 1 : 0, ms);
  }
  std::printf("CHECKSUM center %016llx quat %016llx\n", checksum(st.center().download()), checksum(st.quat().download()));
  return 0;
}
