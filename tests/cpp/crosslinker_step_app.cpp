// crosslinker_step_app.cpp -- the chromatin step of the reference's HP1 app with its crosslinker kinetic Monte Carlo
// stage (HP1.cpp:4728-4739) on spheres, driven from a C++ host program through the stages of mech::SphereChainStepper
// (mundy_hip/stepper.hpp) and the C ABI, with no Python and no torch in the process:
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
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"

using namespace mundy_hip;

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

  mech::SphereChainStepper st(center_h, radius_h, mob_h, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */, pairs_h,
                              MHIP_SPRING_HOOKEAN, k, r0, kt);
  const double* center = st.center().data();

  // crosslinkers: the handle, and the candidate search through the C ABI (its CSR form feeds set_candidates)
  std::vector<std::uint64_t> xkeys_h(mx), xzeros(mx, 0);
  for (size_t c = 0; c < mx; ++c) xkeys_h[c] = c;
  DeviceArray<std::uint64_t> xl_keys(xkeys_h), xl_counters(xzeros);
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

  for (int s = 0; s < steps; ++s) {
    st.neighbors();
    // candidate list by the displacement rule, rows sorted by id once per build; then the KMC step
    int stale = 1;
    if (xl_generated) check(mhip_broadphase_needs_rebuild(xl_search, n, center, &stale, nullptr));
    if (stale) {
      size_t entries = 0;
      check(mhip_broadphase_build(xl_search, &xl_cfg, n, nullptr, center, reach.data(), &entries, nullptr));
      if (xl_col.size() < entries || xl_col.size() == 0) xl_col = DeviceArray<int32_t>(entries + entries / 4 + 16);
      check(mhip_broadphase_get_pairs(xl_search, nullptr, xl_ptr.data(), xl_col.data(), nullptr));
      check(mhip_crosslinkers_set_candidates(xl, xl_ptr.data(), xl_col.data(), entries, ids.data(), nullptr));
      xl_generated = true;
    }
    check(mhip_crosslinkers_kmc_step(xl, center, dt, xl_keys.data(), xl_counters.data(), events.data(), nullptr,
                                     nullptr));
    // U_ext = M (F_spring + F_crosslinker) + U_brown
    check(mhip_crosslinkers_force(xl, center, st.forces(), 1, xl_over.data(), xl_longest.data(), nullptr));
    st.external_velocity();
    const mech::StepStats r = st.resolve();
    const auto ev = events.download();
    bound += ev[0] - ev[1];
    std::printf("STEP %d contacts %zu iterations %u bound %lld binds %d unbinds %d rebuilt %d converged %d\n", s,
                r.num_contacts, r.num_iters, bound, ev[0], ev[1], r.rebuilt ? 1 : 0, r.converged ? 1 : 0);
    if (r.springs_overstretched != 0 || xl_over.download()[0] != 0) {
      std::fprintf(stderr, "overstretched spring\n");
      return 3;
    }
  }
  DeviceArray<int32_t> right(mx ? mx : 1);
  check(mhip_crosslinkers_get_state(xl, nullptr, right.data(), nullptr));
  std::printf("CHECKSUM center %016llx\n", checksum(st.center().download()));
  std::printf("CHECKSUM right %016llx\n", checksum(right.download(), mx));
  check(mhip_crosslinkers_destroy(xl));
  check(mhip_broadphase_destroy(xl_search));
  return 0;
}
