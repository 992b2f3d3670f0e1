// hydro_step_app.cpp -- the chromatin step with n-body hydrodynamics, as the reference's HP1 app runs it by default
// (HP1.cpp:4744-4803; compute_rpy_hydro :3942-4059), on spheres, driven from a C++ host program through the C ABI and
// mundy_hip/adapter.hpp, with no Python and no torch in the process:
//   neighbour list -> Hookean spring forces F -> U_ext = M F + U_brown -> every update_every-th step u_hydro = hydro(F)
//   -> U_ext += u_hydro -> contacts, q = sep + dt D^T U_ext -> BBPGD from lambda = 0 -> U = U_ext + M D lambda -> Euler
// Usage: hydro_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every>
//   kind: 0 stokes, 1 rpy, 2 rpyc (MHIP_HYDRO_*); the hydrodynamic radii are the beads' own
//   input.bin: uint64 n, uint64 m, then doubles center[3n] radius[n] mob_trans[n], then int32 pairs[2m]
// rng keys are the body indices, counters start at 0.  Prints one line per step and a bit-level checksum of the final
// centres, so the test can compare the whole trajectory with the Python driver's.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mundy_hip/adapter.hpp"

using namespace mundy_hip;

template <class T>
static std::vector<T> read_array(std::FILE* f, size_t count) {
  std::vector<T> v(count);
  if (std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
  return v;
}
static unsigned long long checksum(const std::vector<double>& v) {  // order-sensitive FNV-1a over the bit patterns
  unsigned long long h = 1469598103934665603ull;
  for (double d : v) {
    unsigned long long b;
    std::memcpy(&b, &d, sizeof b);
    h = (h ^ b) * 1099511628211ull;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <viscosity> <kind> <update_every>\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const auto nm = read_array<std::uint64_t>(f, 2);
  const size_t n = nm[0], m = nm[1];
  const auto center_h = read_array<double>(f, 3 * n), radius_h = read_array<double>(f, n),
             mob_h = read_array<double>(f, n);
  const auto pairs_h = read_array<int32_t>(f, 2 * m);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), viscosity = std::atof(argv[8]);
  const int kind = std::atoi(argv[9]), update_every = std::atoi(argv[10]);
  if (update_every < 1) {
    std::fprintf(stderr, "update_every must be >= 1\n");
    return 1;
  }

  DeviceVector center(center_h), radius(radius_h), mob_t(mob_h), aabb(6 * n), force(3 * n), u_ext(6 * n), u_hydro(3 * n);
  mhip_hydro_t hydro = nullptr;
  check(mhip_hydro_create(&hydro));
  std::vector<std::uint64_t> keys_h(n), zeros(n, 0);
  for (size_t i = 0; i < n; ++i) keys_h[i] = i;
  DeviceArray<std::uint64_t> keys(keys_h), counters(zeros);
  mech::Springs springs(n, pairs_h, MHIP_SPRING_HOOKEAN, {}, k, {}, r0);
  mesh::GenNeighborLinks links;
  links.set_search_buffer(buffer).set_search_kind(MHIP_SEARCH_AABB);
  links.concretize();
  DeviceArray<int32_t> pairs;
  std::unique_ptr<ContactOperator> op;
  DeviceVector sep, normal, q, x, g, xt, gt, vel;
  const mhip_space lcp{MHIP_SPACE_LOWER_BOUND, 0.0, 0.0};
  const mhip_pgd_config pc{10000, 1e-5, MHIP_RESIDUAL_PROJECTED_DIFF};  // NgpLcp.cpp:851-852
  auto grow = [](DeviceVector& v, size_t need) {
    if (v.size() < need || v.size() == 0) v = DeviceVector(need ? need : 1);
  };
  for (int s = 0; s < steps; ++s) {
    const auto t0 = std::chrono::steady_clock::now();
    check(mhip_compute_aabb_spheres(n, center.data(), radius.data(), aabb.data(), nullptr));
    const bool rebuilt = links.generate(n, aabb.data(), center.data(), radius.data(), nullptr, false);
    if (rebuilt) links.links_into(pairs);
    const size_t C = links.num_links();
    // U_ext = M F_spring + U_brown
    mech::compute_hookean_spring_forces(springs, center.data(), force.data());
    check(mhip_drag_velocity(n, mob_t.data(), force.data(), u_ext.data(), nullptr));
    mech::compute_brownian_velocity(n, keys.data(), counters.data(), kt, dt, mob_t.data(), u_ext.data());
    // the stored hydrodynamic velocity of F: recomputed every update_every-th step, added on every step
    if (s % update_every == 0)
      check(mhip_hydro_velocity(hydro, kind, viscosity, n, center.data(), radius.data(), force.data(), n, center.data(),
                                radius.data(), u_hydro.data(), 3, 0, nullptr));
    check(mhip_hydro_add_velocity(n, u_hydro.data(), u_ext.data(), 6, nullptr));
    grow(sep, C); grow(normal, 3 * C); grow(q, C); grow(x, C); grow(g, C); grow(xt, C); grow(gt, C);
    check(mhip_contact_spheres(C, pairs.data(), center.data(), radius.data(), nullptr, sep.data(), normal.data(),
                               nullptr));
    if (rebuilt || !op)
      op.reset(new ContactOperator(C, n, pairs.data(), normal.data(), nullptr, nullptr, mob_t.data(), nullptr, dt,
                                   nullptr, /*priority=*/sep.data()));
    else
      op->refresh(normal.data(), nullptr, nullptr);
    // q = sep + dt D^T U_ext (NgpHP1.cpp:1488-1531)
    check(mhip_contact_op_constraint_rate(op->handle(), u_ext.data(), q.data(), nullptr));
    check(mhip_axpby(C, 1.0, sep.data(), dt, q.data(), nullptr));
    check(mhip_fill(C, x.data(), 0.0, nullptr));
    mhip_solve_result res{};
    check(mhip_bbpgd_solve_contact(op->handle(), q.data(), &lcp, &pc, x.data(), g.data(), xt.data(), gt.data(), &res,
                                   nullptr));
    // U = U_ext + M D lambda, then x += dt U
    grow(vel, 6 * n);
    check(mhip_deep_copy(6 * n, vel.data(), op->compute_generalized_velocity(), nullptr));
    check(mhip_axpby(6 * n, 1.0, u_ext.data(), 1.0, vel.data(), nullptr));
    check(mhip_integrate_euler(n, dt, vel.data(), center.data(), nullptr, nullptr));
    check(mhip_stream_synchronize(nullptr));
    const double ms = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::printf("STEP %d contacts %zu iterations %u max_spring_length %.17g rebuilt %d converged %d ms %.3f\n", s, C,
                res.num_iters, springs.max_length(), rebuilt ? 1 : 0, res.converged ? 1 : 0, ms);
    if (springs.overstretched() != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  check(mhip_hydro_destroy(hydro));
  std::printf("CHECKSUM center %016llx\n", checksum(center.download()));
  return 0;
}
