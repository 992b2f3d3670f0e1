// nucleus_step_app.cpp -- the chromatin step of the reference's HP1 app inside its nucleus: bead-spring chains with
// thermal noise, confined by the periphery (HP1.cpp:4063-4284) and driven by the active euchromatin force dipoles
// (:3770-3853, :4286-4354), from a C++ host program through the C ABI and mundy_hip/adapter.hpp, with no Python and no
// torch in the process.  The force stage in the reference's order (:4733-4741):
//   neighbour list -> active sampling -> Hookean backbone forces -> periphery force -> active force dipoles
//   -> U_ext = M F + U_brown -> contacts, q = sep + dt D^T U_ext -> BBPGD from lambda = 0 -> U = U_ext + M D lambda
//   -> Euler update -> the active springs' timers advance by dt
// Usage: nucleus_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <shape> <R0> <R1> <R2> <K>
//                         <cx> <cy> <cz> <qw> <qx> <qy> <qz> <sigma> <kon> <koff>
//   input.bin: uint64 n, uint64 m (springs), uint64 ma (active springs), then doubles center[3n] radius[n]
//   mob_trans[n], then int32 pairs[2m], int32 active_pairs[2ma]
// rng keys are the body / active spring indices, counters start at 0.  Prints one line per step and bit-level checksums
// of the final centres and of the active springs' state, so the test can compare the whole trajectory with the Python
// driver's.
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
  if (count && std::fread(v.data(), sizeof(T), count, f) != count) {
    std::fprintf(stderr, "short read\n");
    std::exit(2);
  }
  return v;
}
template <class T>
static unsigned long long checksum(const std::vector<T>& v) {  // order-sensitive FNV-1a over the bit patterns
  unsigned long long h = 1469598103934665603ull;
  for (T d : v) {
    unsigned long long b = 0;
    std::memcpy(&b, &d, sizeof d);
    h = (h ^ b) * 1099511628211ull;
  }
  return h;
}

int main(int argc, char** argv) {
  if (argc < 23) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <shape> <R0> <R1> <R2> <K> <cx> <cy> "
                 "<cz> <qw> <qx> <qy> <qz> <sigma> <kon> <koff>\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const auto nm = read_array<std::uint64_t>(f, 3);
  const size_t n = nm[0], m = nm[1], ma = nm[2];
  const auto center_h = read_array<double>(f, 3 * n), radius_h = read_array<double>(f, n),
             mob_h = read_array<double>(f, n);
  const auto pairs_h = read_array<int32_t>(f, 2 * m);
  const auto active_h = read_array<int32_t>(f, 2 * ma);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]);
  mhip_periphery wall{};
  wall.shape = std::atoi(argv[8]);
  for (int a = 0; a < 3; ++a) wall.radii[a] = std::atof(argv[9 + a]);
  wall.k = std::atof(argv[12]);
  for (int a = 0; a < 3; ++a) wall.center[a] = std::atof(argv[13 + a]);
  for (int a = 0; a < 4; ++a) wall.quat[a] = std::atof(argv[16 + a]);
  const double sigma = std::atof(argv[20]), kon = std::atof(argv[21]), koff = std::atof(argv[22]);

  DeviceVector center(center_h), radius(radius_h), mob_t(mob_h), aabb(6 * n), force(3 * n), u_ext(6 * n);
  std::vector<std::uint64_t> keys_h(n), zeros(n, 0);
  for (size_t i = 0; i < n; ++i) keys_h[i] = i;
  DeviceArray<std::uint64_t> keys(keys_h), counters(zeros);
  mech::Springs springs(n, pairs_h, MHIP_SPRING_HOOKEAN, {}, k, {}, r0);
  mesh::GenNeighborLinks links;
  links.set_search_buffer(buffer).set_search_kind(MHIP_SEARCH_AABB);
  links.concretize();
  mhip_active_springs_t act = nullptr;
  check(mhip_active_springs_create(&act, n, ma, active_h.data(), sigma, kon, koff, nullptr, nullptr, nullptr));
  DeviceArray<int> switches(2), num_active(1), colliding(1);
  DeviceVector deepest(1);

  DeviceArray<int32_t> pairs;
  std::unique_ptr<ContactOperator> op;
  DeviceVector sep, normal, q, x, g, xt, gt, vel;
  const mhip_space lcp{MHIP_SPACE_LOWER_BOUND, 0.0, 0.0};
  const mhip_pgd_config pc{10000, 1e-5, MHIP_RESIDUAL_PROJECTED_DIFF};  // NgpLcp.cpp:851-852
  auto grow = [](DeviceVector& v, size_t need) {
    if (v.size() < need || v.size() == 0) v = DeviceVector(need ? need : 1);
  };
  for (int s = 0; s < steps; ++s) {
    check(mhip_compute_aabb_spheres(n, center.data(), radius.data(), aabb.data(), nullptr));
    const bool rebuilt = links.generate(n, aabb.data(), center.data(), radius.data(), nullptr, false);
    if (rebuilt) links.links_into(pairs);
    const size_t C = links.num_links();
    // F = F_spring + F_periphery + F_active, after the sampling (HP1.cpp:4733-4741)
    check(mhip_active_springs_sample(act, switches.data(), nullptr));
    mech::compute_hookean_spring_forces(springs, center.data(), force.data());
    check(mhip_periphery_force(&wall, n, center.data(), radius.data(), force.data(), 1, colliding.data(), deepest.data(),
                               nullptr));
    check(mhip_active_springs_force(act, center.data(), force.data(), 1, num_active.data(), nullptr));
    check(mhip_drag_velocity(n, mob_t.data(), force.data(), u_ext.data(), nullptr));
    mech::compute_brownian_velocity(n, keys.data(), counters.data(), kt, dt, mob_t.data(), u_ext.data());
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
    // U = U_ext + M D lambda, then x += dt U, then the timers
    grow(vel, 6 * n);
    check(mhip_deep_copy(6 * n, vel.data(), op->compute_generalized_velocity(), nullptr));
    check(mhip_axpby(6 * n, 1.0, u_ext.data(), 1.0, vel.data(), nullptr));
    check(mhip_integrate_euler(n, dt, vel.data(), center.data(), nullptr, nullptr));
    check(mhip_active_springs_advance(act, dt, nullptr));
    const auto sw = switches.download();
    std::printf("STEP %d contacts %zu iterations %u colliding %d active %d on %d off %d rebuilt %d converged %d\n", s, C,
                res.num_iters, colliding.download()[0], num_active.download()[0], sw[0], sw[1], rebuilt ? 1 : 0,
                res.converged ? 1 : 0);
    if (springs.overstretched() != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  DeviceArray<int32_t> state(ma ? ma : 1);
  DeviceVector next_time(ma ? ma : 1);
  check(mhip_active_springs_get_state(act, state.data(), next_time.data(), nullptr, nullptr, nullptr));
  auto state_h = state.download();
  auto next_h = next_time.download();
  state_h.resize(ma);
  next_h.resize(ma);
  std::printf("CHECKSUM center %016llx\n", checksum(center.download()));
  std::printf("CHECKSUM state %016llx\n", checksum(state_h));
  std::printf("CHECKSUM next_time %016llx\n", checksum(next_h));
  check(mhip_active_springs_destroy(act));
  return 0;
}
