// hydro.hip -- n-body hydrodynamics as a velocity stage: u_t (+)= sum_s K(x_t - x_s, b_t, a_s) f_s for the three pair
// kernels of the reference's periphery library (scrap/.../periphery/Periphery.hpp: apply_stokes_kernel :719-743,
// apply_rpy_kernel :893-938, apply_rpyc_kernel :1000-1081; quake_inv_sqrt :71-82), which the HP1 app adds to the dry
// velocity every step (HP1.cpp:3942-4059, :4744-4803).  All-pairs fp64: the one compute-bound stage of the chain step.
//   one target per lane (centre, radius in registers); the sources of a chunk pass through LDS in tiles of kBlock,
//   64 bytes each = four ds_read_b128 at one address for the whole wave (a broadcast: no bank conflicts, no global
//   loads in the inner loop); the loop over a tile takes four sources at a time so the sqrt / divide chains of
//   independent sources interleave (RPYC: the far field is formed without a branch, the few other pairs are redone).
// Summation contract (mundy_hip.h): chunks of MHIP_HYDRO_CHUNK consecutive sources, ascending source index inside a
// chunk from +0.0, chunk sums in ascending chunk index from +0.0, the old value last.  A target has one writer and there
// are no floating-point atomics.  Two launch shapes produce those same bits:
//   in-lane   grid = target tiles; a lane walks every chunk with a chunk accumulator and a running total
//   partial   grid = target tiles x chunk groups (fills the chip when the tiles alone do not); a workgroup writes the
//             chunk sums of its group to partial[chunk][target][3], k_hydro_reduce adds them in chunk order
// The Stokes double layer of surface nodes onto points (apply_stokes_double_layer_kernel, Periphery.hpp:1221-1313;
// mhip_hydro_double_layer of mundy_hip_hydro_periphery.h) is a fourth pair term on the same machinery, with a staged
// source record of its own (80 bytes) and the reference's `t == s` skip behind a flag.
#include "mhip_internal.hpp"
#include "../../include/mundy_hip_hydro_periphery.h"

namespace mhip {

constexpr int kHydroChunk = MHIP_HYDRO_CHUNK;
static_assert(kHydroChunk % kBlock == 0, "a chunk is a whole number of staged tiles");
// workgroups that give every CU four (256 CUs x 4 workgroups of 4 waves = 4 waves per SIMD): below it the grid also
// splits the chunks
constexpr size_t kHydroFillGroups = 1024;

struct __align__(16) HydroSource {  // 64 bytes: (x, y, z, a) (fx, fy, fz, -)
  double x, y, z, a, fx, fy, fz, pad;
};

// The Stokes double layer of surface nodes onto points (Periphery.hpp:1221-1313), one more pair term on this machinery
// (mhip_hydro_double_layer, mundy_hip_hydro_periphery.h): not a kind of mhip_hydro_velocity, which refuses it.
constexpr int kHydroDoubleLayer = 3;

// its staged source: the centre and the six symmetric combinations of s_ij = (n_i f_j) w, which depend on the source
// alone and are formed once when the tile is staged (the same bits as the reference's per-pair products); 80 bytes
struct __align__(16) HydroDlSource {
  double x, y, z, sxx, syy, szz, sxy, sxz, syz, pad;
};

template <int KIND>
struct HydroSourceOf {
  using type = HydroSource;
};
template <>
struct HydroSourceOf<kHydroDoubleLayer> {
  using type = HydroDlSource;
};

struct HydroConst {
  double scale;  // 1 / (8 pi mu), formed once on the host (STOKES, RPY); double layer: -(3 / (4 pi mu))
  double c8;     // (1/8) (1/pi) (1/mu), the product RPYC's far field starts from
  double c6;     // (1/6) (1/pi) (1/mu), overlapping and local drag
};

constexpr double kHydroZero = 1.0e-12;  // the reference's DOUBLE_ZERO
// sources a lane has in flight in the inner loop (A/B builds: -DMHIP_HYDRO_IN_FLIGHT=n; DESIGN.md 5l has the timings)
#ifndef MHIP_HYDRO_IN_FLIGHT
#define MHIP_HYDRO_IN_FLIGHT 4
#endif
constexpr int kHydroInFlight = MHIP_HYDRO_IN_FLIGHT;

// Periphery.hpp:71-82: the bit trick with ONE Newton step (relative error up to 1.75e-3): part of what STOKES and RPY are
__device__ inline double quake_inv_sqrt(double number) {
  const double x2 = number * 0.5;
  long long i = __double_as_longlong(number);
  i = 0x5fe6eb50c7b537a9ll - (i >> 1);
  const double y = __longlong_as_double(i);
  return y * (1.5 - (x2 * y * y));
}

// RPYC when a + b < r does not hold (a few pairs per bead): the overlapping form, the local drag or nothing
__device__ inline V3 rpyc_near_term(double dx, double dy, double dz, const HydroSource& s, double b,
                                          const HydroConst& k) {
  constexpr double one_over_32 = 1.0 / 32.0;
  const double fx = s.fx, fy = s.fy, fz = s.fz, a = s.a;
  const double r2 = dx * dx + dy * dy + dz * dz;
  const double r = sqrt(r2);
  if (fabs(a - b) < r && a > kHydroZero && b > kHydroZero) {  // overlapping, different radii
    const double r3 = r * r2;
    const double rinv = r2 < kHydroZero ? 0.0 : 1.0 / r;
    const double rinv2 = rinv * rinv;
    const double rinv3 = rinv2 * rinv;
    const double hx = dx * rinv, hy = dy * rinv, hz = dz * rinv;
    const double fdh = fx * hx + fy * hy + fz * hz;
    const double a_plus_b = a + b;
    const double a_minus_b = a - b;
    const double a_minus_b2 = a_minus_b * a_minus_b;
    const double tmp3 = a_minus_b2 + 3 * r2;
    const double tmp4 = a_minus_b2 - r2;
    const double so = k.c6 / (a * b);
    const double t1 = so * (16.0 * r3 * a_plus_b - tmp3 * tmp3) * one_over_32 * rinv3;
    const double t2 = so * 3.0 * tmp4 * tmp4 * one_over_32 * rinv3;
    return {t1 * fx + t2 * (fdh * hx), t1 * fy + t2 * (fdh * hy), t1 * fz + t2 * (fdh * hz)};
  }
  // one sphere inside the other: local drag; coincident centres are skipped (a +-0.0 term adds nothing)
  const double sl = r2 < kHydroZero ? 0.0 : k.c6 / (a < b ? b : a);
  return {sl * fx, sl * fy, sl * fz};
}

// One pair term.  RPYC: the far field, without a branch (so the sqrt / divide chains of the unrolled sources interleave);
// *near says that the pair is not in the far field and rpyc_near_term has to replace the value.
template <int KIND>
__device__ inline V3 hydro_term(double dx, double dy, double dz, const HydroSource& s, double b, const HydroConst& k,
                                bool* near) {
  const double fx = s.fx, fy = s.fy, fz = s.fz;
  const double r2 = dx * dx + dy * dy + dz * dz;
  *near = false;
  if (KIND == MHIP_HYDRO_STOKES) {
    const double rinv = r2 < kHydroZero ? 0.0 : quake_inv_sqrt(r2);
    const double rinv3 = rinv * rinv * rinv;
    const double fdr = fx * dx + fy * dy + fz * dz;
    const double sr3 = k.scale * rinv3;
    return {sr3 * (r2 * fx + dx * fdr), sr3 * (r2 * fy + dy * fdr), sr3 * (r2 * fz + dz * fdr)};
  } else if (KIND == MHIP_HYDRO_RPY) {
    constexpr double one_over_three = 1.0 / 3.0;
    constexpr double one_over_six = 1.0 / 6.0;
    const double a = s.a;
    const double a2_over_three = one_over_three * a * a;
    const double rinv = r2 < kHydroZero ? 0.0 : quake_inv_sqrt(r2);
    const double rinv3 = rinv * rinv * rinv;
    const double rinv5 = rinv * rinv * rinv3;
    const double fdr = fx * dx + fy * dy + fz * dz;
    const double three_fdr_rinv5 = 3.0 * fdr * rinv5;
    const double cx = fx * rinv3 - three_fdr_rinv5 * dx;
    const double cy = fy * rinv3 - three_fdr_rinv5 * dy;
    const double cz = fz * rinv3 - three_fdr_rinv5 * dz;
    const double fdr_rinv3 = fdr * rinv3;
    const double v0 = k.scale * (fx * rinv + dx * fdr_rinv3 + a2_over_three * cx);
    const double v1 = k.scale * (fy * rinv + dy * fdr_rinv3 + a2_over_three * cy);
    const double v2 = k.scale * (fz * rinv + dz * fdr_rinv3 + a2_over_three * cz);
    const double lap0 = 2.0 * k.scale * cx;
    const double lap1 = 2.0 * k.scale * cy;
    const double lap2 = 2.0 * k.scale * cz;
    const double lap_coeff = one_over_six * b * b;
    return {v0 + lap_coeff * lap0, v1 + lap_coeff * lap1, v2 + lap_coeff * lap2};
  } else {
    constexpr double one_over_three = 1.0 / 3.0;
    const double a = s.a;
    const double r = sqrt(r2);
    const double rinv = r2 < kHydroZero ? 0.0 : 1.0 / r;
    const double rinv2 = rinv * rinv;
    const double hx = dx * rinv, hy = dy * rinv, hz = dz * rinv;
    const double fdh = fx * hx + fy * hy + fz * hz;
    const double a2 = a * a;
    const double b2 = b * b;
    const double a2_plus_b2_rinv2 = (a2 + b2) * rinv2;
    const double sf = k.c8 * rinv;
    const double t1 = sf * (1. + a2_plus_b2_rinv2 * one_over_three);
    const double t2 = sf * (1. - a2_plus_b2_rinv2);
    *near = !(a + b < r);
    return {t1 * fx + t2 * (fdh * hx), t1 * fy + t2 * (fdh * hy), t1 * fz + t2 * (fdh * hz)};
  }
}

// Periphery.hpp:1279-1308 with the source's products staged: coeff and d coeff, associated as the reference's lines
__device__ inline V3 hydro_dl_term(double dx, double dy, double dz, const HydroDlSource& s, const HydroConst& k) {
  const double r2 = dx * dx + dy * dy + dz * dz;
  const double rinv = r2 < kHydroZero ? 0.0 : quake_inv_sqrt(r2);
  const double rinv2 = rinv * rinv;
  const double rinv5 = rinv * rinv2 * rinv2;
  double coeff = s.sxx * dx * dx + s.syy * dy * dy + s.szz * dz * dz;
  coeff += s.sxy * dx * dy;
  coeff += s.sxz * dx * dz;
  coeff += s.syz * dy * dz;
  coeff *= k.scale * rinv5;
  return {dx * coeff, dy * coeff, dz * coeff};
}

template <int KIND, class SRC>
__device__ inline V3 hydro_pair(double dx, double dy, double dz, const SRC& s, double b, const HydroConst& k,
                                bool* near) {
  if constexpr (KIND == kHydroDoubleLayer) {
    *near = false;
    return hydro_dl_term(dx, dy, dz, s, k);
  } else {
    return hydro_term<KIND>(dx, dy, dz, s, b, k, near);
  }
}

// the terms of the sources tile[0 .. cnt) added to acc in ascending order; kHydroInFlight sources in flight.
// skip_j (double layer only): the tile entry whose term is +0.0, the reference's `t == s` return; -1: none
template <int KIND, class SRC>
__device__ inline void hydro_add_tile(const SRC* tile, int cnt, double tx, double ty, double tz, double b,
                                      const HydroConst& k, int skip_j, V3& acc) {
  int j = 0;
  for (; j + kHydroInFlight <= cnt; j += kHydroInFlight) {
    V3 v[kHydroInFlight];
    bool near[kHydroInFlight];
    bool any_near = false;
#pragma unroll
    for (int u = 0; u < kHydroInFlight; ++u) {
      const SRC src = tile[j + u];
      v[u] = hydro_pair<KIND>(tx - src.x, ty - src.y, tz - src.z, src, b, k, &near[u]);
      if (KIND == kHydroDoubleLayer && j + u == skip_j) v[u] = V3{0.0, 0.0, 0.0};
      any_near |= near[u];
    }
    if constexpr (KIND == MHIP_HYDRO_RPYC) {  // (the only kind with a near field: the other records have no radius)
      if (any_near) {
#pragma unroll
        for (int u = 0; u < kHydroInFlight; ++u) {
          if (near[u]) {
            const HydroSource src = tile[j + u];
            v[u] = rpyc_near_term(tx - src.x, ty - src.y, tz - src.z, src, b, k);
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kHydroInFlight; ++u) {
      acc.x = acc.x + v[u].x;
      acc.y = acc.y + v[u].y;
      acc.z = acc.z + v[u].z;
    }
  }
  for (; j < cnt; ++j) {
    const SRC src = tile[j];
    bool near;
    V3 v = hydro_pair<KIND>(tx - src.x, ty - src.y, tz - src.z, src, b, k, &near);
    if constexpr (KIND == MHIP_HYDRO_RPYC) {
      if (near) v = rpyc_near_term(tx - src.x, ty - src.y, tz - src.z, src, b, k);
    }
    if (KIND == kHydroDoubleLayer && j == skip_j) v = V3{0.0, 0.0, 0.0};
    acc.x = acc.x + v.x;
    acc.y = acc.y + v.y;
    acc.z = acc.z + v.z;
  }
}

struct HydroArgs {
  size_t ns, nt, nchunks, chunks_per_group;
  const double *sc, *sa, *sf, *tc, *tb;
  const double *sn, *sw;  // double layer: the sources' normals [ns][3] and weights [ns] (sa and tb are not read)
  int skip_same;          // double layer: the term of source t onto target t is skipped
  double* out;       // in-lane: velocity (stride, accumulate); partial: partial[chunk][target][3]
  int stride, accumulate;
  HydroConst k;
  // (the hydrodynamic solve, mundy_hip_hydro_solve.h) a device word of the solver: non-zero = the solve is over and this
  // launch, enqueued behind its last iteration, leaves everything as it is.  null: no such word.
  const int* gate;
};

// source s as the kernel stages it in LDS
template <int KIND>
__device__ inline typename HydroSourceOf<KIND>::type hydro_stage(const HydroArgs& p, size_t s) {
  if constexpr (KIND == kHydroDoubleLayer) {
    const double n0 = p.sn[3 * s], n1 = p.sn[3 * s + 1], n2 = p.sn[3 * s + 2];
    const double f0 = p.sf[3 * s], f1 = p.sf[3 * s + 1], f2 = p.sf[3 * s + 2];
    const double w = p.sw[s];
    HydroDlSource src;
    src.x = p.sc[3 * s];
    src.y = p.sc[3 * s + 1];
    src.z = p.sc[3 * s + 2];
    src.sxx = n0 * f0 * w;
    src.syy = n1 * f1 * w;
    src.szz = n2 * f2 * w;
    src.sxy = n0 * f1 * w + n1 * f0 * w;
    src.sxz = n0 * f2 * w + n2 * f0 * w;
    src.syz = n1 * f2 * w + n2 * f1 * w;
    src.pad = 0.0;
    return src;
  } else {
    HydroSource src;
    src.x = p.sc[3 * s];
    src.y = p.sc[3 * s + 1];
    src.z = p.sc[3 * s + 2];
    src.a = (KIND != MHIP_HYDRO_STOKES) ? p.sa[s] : 0.0;
    src.fx = p.sf[3 * s];
    src.fy = p.sf[3 * s + 1];
    src.fz = p.sf[3 * s + 2];
    src.pad = 0.0;
    return src;
  }
}

// SPARSE (mhip_hydro_set_sparse_sources; never the double layer): a staged tile is compacted, in order, to the sources
// with a non-zero force component.  A source with f = (+-0, +-0, +-0) adds +-0.0 to every target (finite inputs), and a
// sum started from +0.0 is unchanged by +-0.0 terms: the same bits.  The count is uniform over the workgroup.
template <int KIND, bool PARTIAL, bool SPARSE>
__global__ void __launch_bounds__(kBlock) k_hydro(HydroArgs p) {
  __shared__ typename HydroSourceOf<KIND>::type tile[kBlock];
  __shared__ int kept[SPARSE ? kBlock / 64 : 1];  // per wave: sources of the tile that stay
  if (p.gate != nullptr && *p.gate != 0) return;
  const size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x;
  const bool valid = t < p.nt;
  double tx = 0.0, ty = 0.0, tz = 0.0, b = 0.0;
  if (valid) {
    tx = p.tc[3 * t];
    ty = p.tc[3 * t + 1];
    tz = p.tc[3 * t + 2];
    if (KIND != MHIP_HYDRO_STOKES && KIND != kHydroDoubleLayer) b = p.tb[t];
  }
  const size_t c0 = PARTIAL ? blockIdx.y * p.chunks_per_group : 0;
  size_t c1 = PARTIAL ? c0 + p.chunks_per_group : p.nchunks;
  if (c1 > p.nchunks) c1 = p.nchunks;
  V3 total{0.0, 0.0, 0.0};
  for (size_t c = c0; c < c1; ++c) {
    V3 acc{0.0, 0.0, 0.0};
    const size_t s_begin = c * (size_t)kHydroChunk;
    const size_t s_end = s_begin + kHydroChunk < p.ns ? s_begin + kHydroChunk : p.ns;
    for (size_t s0 = s_begin; s0 < s_end; s0 += kBlock) {
      __syncthreads();  // the previous tile has been read by every wave
      const size_t s = s0 + threadIdx.x;
      int cnt = s_end - s0 < (size_t)kBlock ? static_cast<int>(s_end - s0) : kBlock;
      if constexpr (SPARSE) {
        typename HydroSourceOf<KIND>::type src{};
        bool keep = false;
        if (s < s_end) {
          src = hydro_stage<KIND>(p, s);
          keep = src.fx != 0.0 || src.fy != 0.0 || src.fz != 0.0;  // (-0.0 != 0.0 is false; a NaN stays)
        }
        const unsigned long long votes = __ballot(keep);
        const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if (lane == 0) kept[wave] = __popcll(votes);
        __syncthreads();
        int slot = __popcll(votes & ((1ull << lane) - 1ull));  // kept sources before this one: in its wave ...
        cnt = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
          if (w < wave) slot += kept[w];  // ... and in the waves before it
          cnt += kept[w];
        }
        if (keep) tile[slot] = src;  // slot <= threadIdx.x < kBlock
      } else {
        if (s < s_end) tile[threadIdx.x] = hydro_stage<KIND>(p, s);
      }
      __syncthreads();
      int skip_j = -1;
      if (KIND == kHydroDoubleLayer && p.skip_same && t >= s0 && t - s0 < (size_t)cnt) skip_j = static_cast<int>(t - s0);
      hydro_add_tile<KIND>(tile, cnt, tx, ty, tz, b, p.k, skip_j, acc);
    }
    if (PARTIAL) {
      if (valid) store3(p.out, c * p.nt + t, acc);
    } else {
      total = total + acc;
    }
  }
  if (!PARTIAL && valid) {
    double* o = p.out + t * (size_t)p.stride;
    if (p.accumulate) {
      o[0] = o[0] + total.x;
      o[1] = o[1] + total.y;
      o[2] = o[2] + total.z;
    } else {
      o[0] = total.x;
      o[1] = total.y;
      o[2] = total.z;
    }
  }
}

// the ordered second pass of the partial shape: chunk sums in ascending chunk index from +0.0, the old value last
__global__ void __launch_bounds__(kBlock) k_hydro_reduce(size_t nt, size_t nchunks, const double* __restrict__ partial,
                                                        double* __restrict__ out, int stride, int accumulate,
                                                        const int* __restrict__ gate) {
  const size_t t = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (t >= nt) return;
  if (gate != nullptr && *gate != 0) return;
  V3 total{0.0, 0.0, 0.0};
  for (size_t c = 0; c < nchunks; ++c) total = total + load3(partial, c * nt + t);
  double* o = out + t * (size_t)stride;
  if (accumulate) {
    o[0] = o[0] + total.x;
    o[1] = o[1] + total.y;
    o[2] = o[2] + total.z;
  } else {
    o[0] = total.x;
    o[1] = total.y;
    o[2] = total.z;
  }
}

// velocity[b][0..2] += u[b][0..2]: the stored hydrodynamic velocity into the [n][6] (or [n][3]) rows of U_ext
__global__ void __launch_bounds__(kBlock) k_hydro_add(size_t n, const double* __restrict__ u, double* __restrict__ vel,
                                                     int stride) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    double* v = vel + i * (size_t)stride;
    v[0] = v[0] + u[3 * i];
    v[1] = v[1] + u[3 * i + 1];
    v[2] = v[2] + u[3 * i + 2];
  }
}

template <int KIND>
static void launch_hydro(bool partial, bool sparse, dim3 grid, const HydroArgs& a, hipStream_t s) {
  if constexpr (KIND != kHydroDoubleLayer) {  // (surface densities are dense: the double layer has no sparse form)
    if (sparse) {
      if (partial)
        k_hydro<KIND, true, true><<<grid, kBlock, 0, s>>>(a);
      else
        k_hydro<KIND, false, true><<<grid, kBlock, 0, s>>>(a);
      return;
    }
  }
  if (partial)
    k_hydro<KIND, true, false><<<grid, kBlock, 0, s>>>(a);
  else
    k_hydro<KIND, false, false><<<grid, kBlock, 0, s>>>(a);
}

}  // namespace mhip

using namespace mhip;

namespace mhip {
int hydro_launch(mhip_hydro* h, int kind, HydroArgs a, double* velocity, bool sparse, hipStream_t s);
}

struct mhip_hydro {
  HandleBuffer partial;  // grow-only: [chunk][target][3] of the largest partial-shape call so far
  int path = MHIP_HYDRO_PATH_AUTO;
  int last_path = MHIP_HYDRO_PATH_AUTO;
  bool sparse = false;  // mhip_hydro_set_sparse_sources
};

extern "C" {

int mhip_hydro_create(mhip_hydro_t* handle) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  *handle = new mhip_hydro();
  return MHIP_SUCCESS;
}

int mhip_hydro_destroy(mhip_hydro_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_hydro_set_path(mhip_hydro_t h, int path) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle is null");
  MHIP_REQUIRE(path == MHIP_HYDRO_PATH_AUTO || path == MHIP_HYDRO_PATH_IN_LANE || path == MHIP_HYDRO_PATH_PARTIAL,
               MHIP_ERR_INVALID_ARGUMENT, "unknown hydro launch path %d", path);
  h->path = path;
  return MHIP_SUCCESS;
}

int mhip_hydro_set_sparse_sources(mhip_hydro_t h, int on) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle is null");
  MHIP_REQUIRE(on == 0 || on == 1, MHIP_ERR_INVALID_ARGUMENT, "sparse sources must be 0 or 1, got %d", on);
  h->sparse = on != 0;
  return MHIP_SUCCESS;
}

int mhip_hydro_last_path(mhip_hydro_t h, int* path) {
  MHIP_REQUIRE(h != nullptr && path != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle / path is null");
  *path = h->last_path;
  return MHIP_SUCCESS;
}

int mhip_hydro_velocity(mhip_hydro_t h, int kind, double viscosity, size_t ns, const double* source_center,
                        const double* source_radius, const double* source_force, size_t nt,
                        const double* target_center, const double* target_radius, double* velocity,
                        int velocity_stride, int accumulate, mhip_stream_t stream) {
  return hydro_velocity(h, kind, viscosity, ns, source_center, source_radius, source_force, nt, target_center,
                        target_radius, velocity, velocity_stride, accumulate, nullptr, stream);
}

}  // extern "C"

int mhip::hydro_velocity(mhip_hydro* h, int kind, double viscosity, size_t ns, const double* source_center,
                         const double* source_radius, const double* source_force, size_t nt,
                         const double* target_center, const double* target_radius, double* velocity,
                         int velocity_stride, int accumulate, const HydroLaunchOptions* opt, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle is null");
  MHIP_REQUIRE(kind == MHIP_HYDRO_STOKES || kind == MHIP_HYDRO_RPY || kind == MHIP_HYDRO_RPYC,
               MHIP_ERR_INVALID_ARGUMENT, "unknown hydrodynamic kernel kind %d", kind);
  MHIP_REQUIRE(std::isfinite(viscosity) && viscosity > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "viscosity must be finite and > 0, got %g", viscosity);
  MHIP_REQUIRE(velocity_stride == 3 || velocity_stride == 6, MHIP_ERR_INVALID_ARGUMENT,
               "velocity_stride must be 3 or 6, got %d", velocity_stride);
  const bool radii = kind != MHIP_HYDRO_STOKES;
  MHIP_REQUIRE(ns == 0 || (source_center && source_force && (source_radius || !radii)), MHIP_ERR_INVALID_ARGUMENT,
               "source_center / source_radius / source_force is null");
  MHIP_REQUIRE(nt == 0 || (target_center && velocity && (target_radius || !radii)), MHIP_ERR_INVALID_ARGUMENT,
               "target_center / target_radius / velocity is null");
  MHIP_REQUIRE(ns < (1ull << 40) && nt < (1ull << 31) * (size_t)kBlock, MHIP_ERR_INVALID_ARGUMENT,
               "too many sources or targets");
  if (nt == 0) return MHIP_SUCCESS;
  if (ns == 0 && accumulate) return MHIP_SUCCESS;  // an empty sum: velocity stays as it is
  HydroArgs a{};
  a.ns = ns;
  a.nt = nt;
  a.sc = source_center;
  a.sa = source_radius;
  a.sf = source_force;
  a.tc = target_center;
  a.tb = target_radius;
  a.stride = velocity_stride;
  a.accumulate = accumulate ? 1 : 0;
  constexpr double one_over_eight = 1.0 / 8.0;
  constexpr double one_over_six = 1.0 / 6.0;
  constexpr double inv_pi = 1.0 / 3.14159265358979323846;
  const double inv_viscosity = 1.0 / viscosity;
  a.k.scale = 1.0 / (8.0 * M_PI * viscosity);
  a.k.c8 = one_over_eight * inv_pi * inv_viscosity;
  a.k.c6 = one_over_six * inv_pi * inv_viscosity;
  a.gate = opt ? opt->gate : nullptr;
  return hydro_launch(h, kind, a, velocity, opt ? opt->sparse : h->sparse, as_stream(stream));
}

// the launch both entry points share: the launch rule, the grow-only buffer and the ordered second pass
int mhip::hydro_launch(mhip_hydro* h, int kind, HydroArgs a, double* velocity, bool sparse, hipStream_t s) {
  const size_t nt = a.nt;
  const int velocity_stride = a.stride;
  a.nchunks = (a.ns + kHydroChunk - 1) / kHydroChunk;
  // launch rule: target tiles alone when they fill the chip (or there is one chunk at most), otherwise tiles x groups
  const size_t tiles = (nt + kBlock - 1) / kBlock;
  size_t groups = (kHydroFillGroups + tiles - 1) / tiles;
  if (groups > a.nchunks) groups = a.nchunks;  // (0 without sources: the in-lane shape writes the zeros)
  const bool partial = h->path == MHIP_HYDRO_PATH_AUTO ? groups > 1 : (h->path == MHIP_HYDRO_PATH_PARTIAL && groups > 0);
  h->last_path = partial ? MHIP_HYDRO_PATH_PARTIAL : MHIP_HYDRO_PATH_IN_LANE;
  dim3 grid(static_cast<unsigned>(tiles), 1, 1);
  if (partial) {
    a.chunks_per_group = (a.nchunks + groups - 1) / groups;
    groups = (a.nchunks + a.chunks_per_group - 1) / a.chunks_per_group;  // no empty group
    grid.y = static_cast<unsigned>(groups);
    if (int e = h->partial.reserve(a.nchunks * nt * 3 * sizeof(double))) return e;
    a.out = h->partial.as<double>();
  } else {
    a.chunks_per_group = a.nchunks;
    a.out = velocity;
  }
  switch (kind) {
    case MHIP_HYDRO_STOKES: launch_hydro<MHIP_HYDRO_STOKES>(partial, sparse, grid, a, s); break;
    case MHIP_HYDRO_RPY: launch_hydro<MHIP_HYDRO_RPY>(partial, sparse, grid, a, s); break;
    case MHIP_HYDRO_RPYC: launch_hydro<MHIP_HYDRO_RPYC>(partial, sparse, grid, a, s); break;
    default: launch_hydro<kHydroDoubleLayer>(partial, false, grid, a, s); break;
  }
  MHIP_LAUNCH_CHECK();
  if (partial) {
    k_hydro_reduce<<<grid_exact(nt), kBlock, 0, s>>>(nt, a.nchunks, h->partial.as<double>(), velocity, velocity_stride,
                                                     a.accumulate, a.gate);
    MHIP_LAUNCH_CHECK();
  }
  return MHIP_SUCCESS;
}

extern "C" {

int mhip_hydro_double_layer(mhip_hydro_t h, double viscosity, size_t ns, const double* center, const double* normal,
                            const double* weight, const double* force, size_t nt, const double* target_center,
                            double* velocity, int velocity_stride, int accumulate, int skip_same_index,
                            mhip_stream_t stream) {
  return hydro_double_layer(h, viscosity, ns, center, normal, weight, force, nt, target_center, velocity, velocity_stride,
                            accumulate, skip_same_index, nullptr, stream);
}

}  // extern "C"

int mhip::hydro_double_layer(mhip_hydro* h, double viscosity, size_t ns, const double* center, const double* normal,
                             const double* weight, const double* force, size_t nt, const double* target_center,
                             double* velocity, int velocity_stride, int accumulate, int skip_same_index,
                             const HydroLaunchOptions* opt, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle is null");
  MHIP_REQUIRE(std::isfinite(viscosity) && viscosity > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "viscosity must be finite and > 0, got %g", viscosity);
  MHIP_REQUIRE(velocity_stride == 3 || velocity_stride == 6, MHIP_ERR_INVALID_ARGUMENT,
               "velocity_stride must be 3 or 6, got %d", velocity_stride);
  MHIP_REQUIRE(ns == 0 || (center && normal && weight && force), MHIP_ERR_INVALID_ARGUMENT,
               "center / normal / weight / force is null");
  MHIP_REQUIRE(nt == 0 || (target_center && velocity), MHIP_ERR_INVALID_ARGUMENT, "target_center / velocity is null");
  MHIP_REQUIRE(ns < (1ull << 40) && nt < (1ull << 31) * (size_t)kBlock, MHIP_ERR_INVALID_ARGUMENT,
               "too many sources or targets");
  if (nt == 0) return MHIP_SUCCESS;
  if (ns == 0 && accumulate) return MHIP_SUCCESS;  // an empty sum: velocity stays as it is
  HydroArgs a{};
  a.ns = ns;
  a.nt = nt;
  a.sc = center;
  a.sn = normal;
  a.sw = weight;
  a.sf = force;
  a.tc = target_center;
  a.skip_same = skip_same_index ? 1 : 0;
  a.stride = velocity_stride;
  a.accumulate = accumulate ? 1 : 0;
  const double scale_dl = 3.0 / (4.0 * M_PI * viscosity);
  a.k.scale = -scale_dl;
  a.gate = opt ? opt->gate : nullptr;
  return hydro_launch(h, kHydroDoubleLayer, a, velocity, false, as_stream(stream));  // (surface densities are dense)
}

extern "C" {

int mhip_hydro_add_velocity(size_t n, const double* u_hydro, double* velocity, int velocity_stride,
                            mhip_stream_t stream) {
  MHIP_REQUIRE(velocity_stride == 3 || velocity_stride == 6, MHIP_ERR_INVALID_ARGUMENT,
               "velocity_stride must be 3 or 6, got %d", velocity_stride);
  MHIP_REQUIRE(n == 0 || (u_hydro && velocity), MHIP_ERR_INVALID_ARGUMENT, "u_hydro / velocity is null");
  if (n == 0) return MHIP_SUCCESS;
  k_hydro_add<<<grid_for(n), kBlock, 0, as_stream(stream)>>>(n, u_hydro, velocity, velocity_stride);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

}  // extern "C"
