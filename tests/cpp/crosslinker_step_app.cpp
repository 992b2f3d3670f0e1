// crosslinker_step_app.cpp -- the chromatin step of the reference's HP1 app with its crosslinker kinetic Monte Carlo
// stage (HP1.cpp:4728-4739) on spheres, driven from a C++ host program through the C ABI and mundy_hip/adapter.hpp,
// with no Python and no torch in the process:
//   neighbour list, and the candidate list of the crosslinkers (its own search: sources the beads that carry a
//   crosslinker, targets the bind sites) -> KMC at the positions of the start of the step -> Hookean backbone forces
//   + the doubly bound crosslinkers as springs -> U_ext = M F + U_brown -> contacts, q = sep + dt D^T U_ext -> BBPGD
//   from lambda = 0 -> U = U_ext + M D lambda -> Euler update
// Usage: crosslinker_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt>
//                             <xl_k> <xl_r0> <bind_rate> <unbind_rate> <xl_kt> <capture_radius> <xl_skin>
//   input.bin: uint64 n, uint64 m (springs), uint64 mx (crosslinkers), then doubles center[3n] radius[n] mob_trans[n],
//   then int32 pairs[2m], int32 left[mx], bytes sites[n]
// Every crosslinker starts singly bound; rng keys are the body / crosslinker indices, counters start at 0, ids are the
// body indices.  Prints one line per step and bit-level checksums of the final centres and right heads, so the test
// can compare the whole trajectory with the Python driver's.
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
  if (argc < 15) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <xl_k> <xl_r0> <bind_rate> "
                 "<unbind_rate> <xl_kt> <capture_radius> <xl_skin>\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const auto nm = read_array<std::uint64_t>(f, 3);
  const size_t n = nm[0], m = nm[1], mx = nm[2];
  const auto center_h = read_array<double>(f, 3 * n), radius_h = read_array<double>(f, n),
             mob_h = read_array<double>(f, n);
  const auto pairs_h = read_array<int32_t>(f, 2 * m);
  const auto left_h = read_array<int32_t>(f, mx);
  const auto sites_h = read_array<unsigned char>(f, n);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), xl_k = std::atof(argv[8]), xl_r0 = std::atof(argv[9]),
               bind_rate = std::atof(argv[10]), unbind_rate = std::atof(argv[11]), xl_kt = std::atof(argv[12]),
               cap = std::atof(argv[13]), xl_skin = std::atof(argv[14]);

  DeviceVector center(center_h), radius(radius_h), mob_t(mob_h), aabb(6 * n), force(3 * n), u_ext(6 * n);
  std::vector<std::uint64_t> keys_h(n), zeros(n, 0), xkeys_h(mx), xzeros(mx, 0);
  for (size_t i = 0; i < n; ++i) keys_h[i] = i;
  for (size_t c = 0; c < mx; ++c) xkeys_h[c] = c;
  DeviceArray<std::uint64_t> keys(keys_h), counters(zeros), xl_keys(xkeys_h), xl_counters(xzeros);
  mech::Springs springs(n, pairs_h, MHIP_SPRING_HOOKEAN, {}, k, {}, r0);
  mesh::GenNeighborLinks links;
  links.set_search_buffer(buffer).set_search_kind(MHIP_SEARCH_AABB);
  links.concretize();

  // crosslinkers: the handle, and the candidate search through the C ABI (its CSR form feeds set_candidates)
  mhip_crosslinkers_t xl = nullptr;
  check(mhip_crosslinkers_create(&xl, n, mx, left_h.data(), nullptr, sites_h.data(), MHIP_SPRING_HOOKEAN, xl_k, xl_r0,
                                 bind_rate, unbind_rate, xl_kt, cap, nullptr));
  std::vector<unsigned char> src_h(n, 0);
  for (int32_t l : left_h) src_h[l] = 1;
  std::vector<std::int64_t> ids_h(n);
  for (size_t i = 0; i < n; ++i) ids_h[i] = static_cast<std::int64_t>(i);
  DeviceArray<unsigned char> sources(src_h), sites(sites_h);
  DeviceArray<std::int64_t> ids(ids_h);
  DeviceVector reach(std::vector<double>(n, 0.5 * cap));
  mhip_broadphase_t xl_search = nullptr;
  check(mhip_broadphase_create(&xl_search));
  check(mhip_broadphase_set_sets(xl_search, n, sources.data(), sites.data(), nullptr));
  mhip_broadphase_config xl_cfg{};
  xl_cfg.search_kind = MHIP_SEARCH_SPHERES;
  xl_cfg.symmetric = 1;
  xl_cfg.buffer = xl_skin;
  bool xl_generated = false;
  DeviceArray<int32_t> xl_ptr(n + 1), xl_col;
  DeviceArray<int> events(2), xl_over(1);
  DeviceVector xl_longest(1);
  long long bound = 0;

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
    // candidate list by the displacement rule, rows sorted by id once per build; then the KMC step
    int stale = 1;
    if (xl_generated) check(mhip_broadphase_needs_rebuild(xl_search, n, center.data(), &stale, nullptr));
    if (stale) {
      size_t entries = 0;
      check(mhip_broadphase_build(xl_search, &xl_cfg, n, nullptr, center.data(), reach.data(), &entries, nullptr));
      if (xl_col.size() < entries || xl_col.size() == 0) xl_col = DeviceArray<int32_t>(entries + entries / 4 + 16);
      check(mhip_broadphase_get_pairs(xl_search, nullptr, xl_ptr.data(), xl_col.data(), nullptr));
      check(mhip_crosslinkers_set_candidates(xl, xl_ptr.data(), xl_col.data(), entries, ids.data(), nullptr));
      xl_generated = true;
    }
    check(mhip_crosslinkers_kmc_step(xl, center.data(), dt, xl_keys.data(), xl_counters.data(), events.data(), nullptr,
                                     nullptr));
    // U_ext = M (F_spring + F_crosslinker) + U_brown
    mech::compute_hookean_spring_forces(springs, center.data(), force.data());
    check(mhip_crosslinkers_force(xl, center.data(), force.data(), 1, xl_over.data(), xl_longest.data(), nullptr));
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
    // U = U_ext + M D lambda, then x += dt U
    grow(vel, 6 * n);
    check(mhip_deep_copy(6 * n, vel.data(), op->compute_generalized_velocity(), nullptr));
    check(mhip_axpby(6 * n, 1.0, u_ext.data(), 1.0, vel.data(), nullptr));
    check(mhip_integrate_euler(n, dt, vel.data(), center.data(), nullptr, nullptr));
    const auto ev = events.download();
    bound += ev[0] - ev[1];
    std::printf("STEP %d contacts %zu iterations %u bound %lld binds %d unbinds %d rebuilt %d converged %d\n", s, C,
                res.num_iters, bound, ev[0], ev[1], rebuilt ? 1 : 0, res.converged ? 1 : 0);
    if (springs.overstretched() != 0 || xl_over.download()[0] != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  DeviceArray<int32_t> right(mx ? mx : 1);
  check(mhip_crosslinkers_get_state(xl, nullptr, right.data(), nullptr));
  auto right_h = right.download();
  right_h.resize(mx);
  std::printf("CHECKSUM center %016llx\n", checksum(center.download()));
  std::printf("CHECKSUM right %016llx\n", checksum(right_h));
  check(mhip_crosslinkers_destroy(xl));
  check(mhip_broadphase_destroy(xl_search));
  return 0;
}
