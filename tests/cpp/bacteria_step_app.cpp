// bacteria_step_app.cpp -- the colony loop of the reference's production app (Bacteria.cpp:1033-1080: divide_bacteria
// -> grow_bacteria -> neighbour list with the corner rebuild rule -> Hertz force per linker -> force / torque per body
// -> dry drag -> Euler update) on spherocylinders, driven from a C++ host program through mundy_hip/stepper.hpp
// (SpherocylinderStepper with set_hertz_contact and set_growth), with no Python and no torch in the process.
// Usage: bacteria_step_app <input.bin> <steps> <reorder_cell> <periodic_box_edge> <dt> <youngs_modulus> <poisson_ratio>
//                          <growth_rate> <division_length> <search_buffer>
//   input.bin: uint64 n, then doubles center[3n] quat[4n] radius[n] length[n] mob_trans[n] mob_rot[n]
//   reorder_cell <= 0: no Z-order reorder; periodic_box_edge <= 0: free space
// Prints one line per step and a bit-level checksum of the final centres / orientations, so the test can compare the
// whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr, "Usage: %s <input.bin> <steps> <reorder_cell> <periodic_box_edge> <dt> <E> <nu> <rate> <D> "
                 "<buffer>\n", argv[0]);
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
  const double rate = std::atof(argv[8]), division = std::atof(argv[9]), buffer = std::atof(argv[10]);

  const double box[3] = {edge, edge, edge};
  mech::SpherocylinderStepper st(center, quat, radius, length, mob_t, mob_r, dt, buffer,
                                 convex::PGDConfig<double>{}, edge > 0.0 ? box : nullptr);
  st.set_hertz_contact(E, nu);
  st.set_growth(rate, division);
  if (cell > 0.0) {
    const double lo[3] = {0.0, 0.0, 0.0};
    st.reorder_bodies(cell, lo);
  }
  for (int k = 0; k < steps; ++k) {
    const auto t0 = std::chrono::steady_clock::now();
    const mech::StepStats s = st.step(true, false);
    const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("STEP %d bodies %zu born %zu contacts %zu max_overlap %.17g rebuilt %d ms %.3f\n", k, st.num_bodies(),
                s.num_born, s.num_contacts, s.max_overlap, s.rebuilt ? 1 : 0, ms);
  }
  // the live rows only (the buffers hold spare rows beyond num_bodies())
  auto live = [&](const DeviceVector& a, size_t w) {
    auto h = a.download();
    h.resize(w * st.num_bodies());
    return h;
  };
  std::printf("CHECKSUM center %016llx quat %016llx length %016llx\n", checksum(live(st.center(), 3)),
              checksum(live(st.quat(), 4)), checksum(live(st.length(), 1)));
  return 0;
}
