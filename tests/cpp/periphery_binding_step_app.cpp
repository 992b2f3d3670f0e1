// periphery_binding_step_app.cpp -- crosslinker_step_app with the periphery's bind sites
// (include/mundy_hip_periphery_binding.h; HP1.cpp:3340-3398, :3473-3529): the chromatin step whose crosslinkers bind to
// chromatin beads and to immobile sites on the nuclear envelope, driven from a C++ host program through the stages of
// mech::SphereChainStepper (mundy_hip/stepper.hpp) and the C ABI, with no Python and no torch in the process:
//   neighbour list, the bead candidate list (sources the beads that carry a crosslinker, targets the bind sites) and the
//   periphery candidate list (the same sources, targets the periphery sites, over the beads followed by the sites)
//   -> KMC over both rows at the positions of the start of the step -> Hookean backbone forces + the doubly bound
//   crosslinkers as springs, the periphery-bound ones between their bead and their site -> U_ext = M F + U_brown
//   -> contacts, q = sep + dt D^T U_ext -> BBPGD from lambda = 0 -> U = U_ext + M D lambda -> Euler update
// Usage: periphery_binding_step_app <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt>
//            <xl_k> <xl_r0> <bind_rate> <unbind_rate> <xl_kt> <capture_radius> <xl_skin>
//            <p_bind_rate> <p_k> <p_r0> <p_unbind_rate> <p_capture_radius>
//   input.bin: uint64 n, uint64 m (springs), uint64 mx (crosslinkers), uint64 P (periphery sites), then doubles
//   center[3n] radius[n] mob_trans[n], then int32 pairs[2m], int32 left[mx], bytes sites[n], doubles site_center[3P]
// Every crosslinker starts singly bound; rng keys are the body / crosslinker indices, counters start at 0, ids are the
// body indices.  Prints one line per step and bit-level checksums of the final centres and right heads, so the test
// can compare the whole trajectory with the Python driver's.
#include "app_util.hpp"
#include "mundy_hip/stepper.hpp"
#include "mundy_hip_periphery_binding.h"

using namespace mundy_hip;

int main(int argc, char** argv) {
  if (argc < 20) {
    std::fprintf(stderr,
                 "Usage: %s <input.bin> <steps> <dt> <search_buffer> <k> <r0> <kt> <xl_k> <xl_r0> <bind_rate> "
                 "<unbind_rate> <xl_kt> <capture_radius> <xl_skin> <p_bind_rate> <p_k> <p_r0> <p_unbind_rate> "
                 "<p_capture_radius>\n",
                 argv[0]);
    return 1;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  const auto nm = read_array<std::uint64_t>(f, 4);
  const size_t n = nm[0], m = nm[1], mx = nm[2], P = nm[3];
  const auto center_h = read_array<double>(f, 3 * n), radius_h = read_array<double>(f, n),
             mob_h = read_array<double>(f, n);
  const auto pairs_h = read_array<int32_t>(f, 2 * m);
  const auto left_h = read_array<int32_t>(f, mx);
  const auto sites_h = read_array<unsigned char>(f, n);
  const auto points_h = read_array<double>(f, 3 * P);
  std::fclose(f);
  const int steps = std::atoi(argv[2]);
  const double dt = std::atof(argv[3]), buffer = std::atof(argv[4]), k = std::atof(argv[5]), r0 = std::atof(argv[6]),
               kt = std::atof(argv[7]), xl_k = std::atof(argv[8]), xl_r0 = std::atof(argv[9]),
               bind_rate = std::atof(argv[10]), unbind_rate = std::atof(argv[11]), xl_kt = std::atof(argv[12]),
               cap = std::atof(argv[13]), xl_skin = std::atof(argv[14]), p_bind_rate = std::atof(argv[15]),
               p_k = std::atof(argv[16]), p_r0 = std::atof(argv[17]), p_unbind_rate = std::atof(argv[18]),
               p_cap = std::atof(argv[19]);

  mech::SphereChainStepper st(center_h, radius_h, mob_h, dt, buffer, {10000, 1e-5} /* NgpLcp.cpp:851-852 */, pairs_h,
                              MHIP_SPRING_HOOKEAN, k, r0, kt);
  const double* center = st.center().data();

  // crosslinkers: the handle with its periphery sites, and the two candidate searches through the C ABI
  std::vector<std::uint64_t> xkeys_h(mx), xzeros(mx, 0);
  for (size_t c = 0; c < mx; ++c) xkeys_h[c] = c;
  DeviceArray<std::uint64_t> xl_keys(xkeys_h), xl_counters(xzeros);
  mhip_crosslinkers_t xl = nullptr;
  check(mhip_crosslinkers_create(&xl, n, mx, left_h.data(), nullptr, sites_h.data(), MHIP_SPRING_HOOKEAN, xl_k, xl_r0,
                                 bind_rate, unbind_rate, xl_kt, cap, nullptr));
  DeviceVector points(points_h);
  check(mhip_crosslinkers_set_periphery_sites(xl, P, points.data(), p_bind_rate, p_k, p_r0, p_unbind_rate, p_cap,
                                              nullptr));
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
  // the periphery's search: beads followed by sites, sources the same beads, targets the sites; the sites never move,
  // so the displacement rule rebuilds the list when a bead has moved
  std::vector<double> all_h(center_h);
  all_h.insert(all_h.end(), points_h.begin(), points_h.end());
  std::vector<unsigned char> psrc_h(src_h), ptgt_h(n, 0);
  psrc_h.resize(n + P, 0);
  ptgt_h.resize(n + P, 1);
  DeviceVector all(all_h), p_reach(std::vector<double>(n + P, 0.5 * p_cap));
  DeviceArray<unsigned char> p_sources(psrc_h), p_targets(ptgt_h);
  mhip_broadphase_t p_search = nullptr;
  check(mhip_broadphase_create(&p_search));
  check(mhip_broadphase_set_sets(p_search, n + P, p_sources.data(), p_targets.data(), nullptr));
  bool p_generated = false;
  DeviceArray<int32_t> p_ptr(n + P + 1), p_col;
  DeviceArray<int> events(2), xl_over(1), p_bound(std::vector<int>(1, 0));
  DeviceVector xl_longest(1);
  long long bound = 0;

  for (int s = 0; s < steps; ++s) {
    st.neighbors();
    // candidate lists by the displacement rule, rows sorted once per build; then the KMC step over both rows
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
    check(mhip_deep_copy(3 * n, all.data(), center, nullptr));
    stale = 1;
    if (p_generated) check(mhip_broadphase_needs_rebuild(p_search, n + P, all.data(), &stale, nullptr));
    if (stale) {
      size_t entries = 0;
      check(mhip_broadphase_build(p_search, &xl_cfg, n + P, nullptr, all.data(), p_reach.data(), &entries, nullptr));
      if (p_col.size() < entries || p_col.size() == 0) p_col = DeviceArray<int32_t>(entries + entries / 4 + 16);
      check(mhip_broadphase_get_pairs(p_search, nullptr, p_ptr.data(), p_col.data(), nullptr));
      check(mhip_crosslinkers_set_periphery_candidates(xl, p_ptr.data(), p_col.data(), entries,
                                                       static_cast<int32_t>(n), nullptr));
      p_generated = true;
    }
    p_bound.upload(std::vector<int>(1, 0));
    check(mhip_crosslinkers_kmc_step_periphery(xl, center, dt, xl_keys.data(), xl_counters.data(), events.data(),
                                               p_bound.data(), nullptr, nullptr));
    // U_ext = M (F_spring + F_crosslinker) + U_brown
    check(mhip_crosslinkers_force(xl, center, st.forces(), 1, xl_over.data(), xl_longest.data(), nullptr));
    st.external_velocity();
    const mech::StepStats r = st.resolve();
    const auto ev = events.download();
    bound += ev[0] - ev[1];
    std::printf("STEP %d contacts %zu iterations %u bound %lld binds %d unbinds %d periphery_bound %d rebuilt %d "
                "converged %d\n",
                s, r.num_contacts, r.num_iters, bound, ev[0], ev[1], p_bound.download()[0], r.rebuilt ? 1 : 0,
                r.converged ? 1 : 0);
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
  check(mhip_broadphase_destroy(p_search));
  return 0;
}
