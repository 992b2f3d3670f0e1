// force_device.hpp -- what the soft-force sources (hertz.hip, hertz_friction.hip, chain.hip, crosslink.hip, periphery.hip,
// active.hip) share: the statistic epilogues, the spring and Hertz pair terms, the counter-based generator every
// reference app draws from, the per-body force write, the body -> entry incidence build, the run-time flag -> template
// argument dispatch.  (The lifetime of a handle's buffers -- HandleBuffer -- lives in mhip_internal.hpp, next to the
// destructor-less DeviceBuffer of the process-lifetime scratch, so that every handle of the library shares one type.)
#pragma once
#include "mhip_internal.hpp"

#include <memory>
#include <type_traits>

namespace mhip {

// ---- host: flag dispatch (HandleBuffer, hip_status and upload live in mhip_internal.hpp) ----------------------------
// A run-time flag (a bool or a small enum) becomes a template argument: f(std::integral_constant<T, V>{}) for the first V
// of the list equal to v, for the last one when none is; inside f, decltype(arg)::value.  (convex.hip keeps its own
// pick<> of the same shape: that file is part of the solver stamp and is not edited for this.)
template <auto V, auto... Rest, class F>
void dispatch(decltype(V) v, F&& f) {
  if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<decltype(V), V>{});
  else if (v == V) f(std::integral_constant<decltype(V), V>{});
  else dispatch<Rest...>(v, f);
}
template <class F>
void dispatch_bools(bool a, bool b, F&& f) {  // f(std::bool_constant<a>{}, std::bool_constant<b>{})
  dispatch<true, false>(a, [&](auto ca) { dispatch<true, false>(b, [&](auto cb) { f(ca, cb); }); });
}

// ---- body -> entry incidence (chain.hip) -------------------------------------------------------------------------
// A source lists item i of m at bodies: src(i, f) calls f(body, entry) for each.  build_incidence: count -> exclusive
// scan -> fill -> per-body sort into ptr[0 .. n], ent, every body's list ascending (the fill order depends on atomic
// arrival).  deg: n + 1 ints of scratch; ws: scan_workspace_bytes(n).  m == 0: ptr all zero, no launches.
// Every source of the library is one of the four below, and chain.hip instantiates the build for each.
struct PairEnds {  // entry (s << 1) | side of pair s at body pairs[s][side]
  const int2* pairs;
  template <class F>
  __device__ void operator()(size_t s, F&& f) const {
    const int2 p = pairs[s];
    f(p.x, static_cast<int32_t>(s << 1));
    f(p.y, static_cast<int32_t>((s << 1) | 1));
  }
};
struct ListedAt {  // entry c at body at[c]; with `other`, only where at[c] != other[c]
  const int32_t* at;
  const int32_t* other;
  template <class F>
  __device__ void operator()(size_t c, F&& f) const {
    const int32_t b = at[c];
    if (!other || other[c] != b) f(b, static_cast<int32_t>(c));
  }
};
struct ListedAtBody {  // entry c at body at[c] where that is a body (>= 0: a negative head sits on none) and != other[c]
  const int32_t* at;
  const int32_t* other;
  template <class F>
  __device__ void operator()(size_t c, F&& f) const {
    const int32_t b = at[c];
    if (b >= 0 && other[c] != b) f(b, static_cast<int32_t>(c));
  }
};
// One angular spring: the two ends (roles 0 and 1) and the centre (role 2), the reference's BEAM_3 node order
// (AngularSpringsKernel.cpp:125-133), padded to one 16-byte load.
struct alignas(16) Triplet {
  int32_t a, b, c, pad;
};
struct TripletEnds {  // entry (t << 2) | role of triplet t at its end a (role 0), end b (1) and centre c (2)
  const Triplet* triplets;
  template <class F>
  __device__ void operator()(size_t t, F&& f) const {
    const Triplet q = triplets[t];
    f(q.a, static_cast<int32_t>(t << 2));
    f(q.b, static_cast<int32_t>((t << 2) | 1));
    f(q.c, static_cast<int32_t>((t << 2) | 2));
  }
};
template <class SRC>
int build_incidence(size_t n, size_t m, SRC src, int32_t* deg, int32_t* ptr, int32_t* ent, void* ws, hipStream_t s);

// ---- Philox4x32-10 -----------------------------------------------------------------------------------------------
// counter (c0, c1, c2, c3), key (k0, k1): ten rounds, the key bumped by the Weyl increments between rounds
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

__device__ inline uint4 philox4x32_10(uint4 c, uint2 k) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    if (r > 0) {
      k.x += kPhiloxW0;
      k.y += kPhiloxW1;
    }
    const uint64_t p0 = static_cast<uint64_t>(kPhiloxM0) * c.x;
    const uint64_t p1 = static_cast<uint64_t>(kPhiloxM1) * c.z;
    c = make_uint4(static_cast<uint32_t>(p1 >> 32) ^ c.y ^ k.x, static_cast<uint32_t>(p1),
                   static_cast<uint32_t>(p0 >> 32) ^ c.w ^ k.y, static_cast<uint32_t>(p0));
  }
  return c;
}
// key = (lo32, hi32) of the 64-bit key; counter = (lo32, hi32) of the 64-bit counter, then the block index, then 0
__device__ inline uint4 philox_draw(uint64_t key, uint64_t ctr, uint32_t block) {
  return philox4x32_10(make_uint4(static_cast<uint32_t>(ctr), static_cast<uint32_t>(ctr >> 32), block, 0u),
                       make_uint2(static_cast<uint32_t>(key), static_cast<uint32_t>(key >> 32)));
}
// the 53-bit integer m = (w0 << 21) | (w1 >> 11) of the first two words: m 2^-53 in [0, 1), (m + 1) 2^-53 in (0, 1]
__device__ inline uint64_t philox_u53(uint4 w) {
  return (static_cast<uint64_t>(w.x) << 21) | static_cast<uint64_t>(w.y >> 11);
}

// ---- statistic epilogues: every lane of the workgroup calls them, after its grid-stride loop ---------------------
// The largest v of the launch goes to one device double through an atomic max on its bit pattern: every candidate is a
// non-negative double, whose bits order like the value, so the result does not depend on the order in which workgroups
// arrive.  Wave max, then across the workgroup's waves, then one atomic per workgroup (the grid is capped at kMaxGrid),
// none for +0.0 or a null `bits`.  Once per kernel: the LDS slots are not fenced for a second use.
__device__ inline void block_stat_max(double v, unsigned long long* bits) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_xor(v, off, 64);
    v = o > v ? o : v;
  }
  __shared__ double wave_max[kBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_max[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0 && bits) {
    double m = wave_max[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) m = wave_max[w] > m ? wave_max[w] : m;
    if (m > 0.0) atomicMax(bits, static_cast<unsigned long long>(__double_as_longlong(m)));
  }
}
// a counter summed over the workgroup: one atomic per workgroup, none for 0 (once per kernel, as block_stat_max)
__device__ inline void block_stat_add(unsigned v, unsigned long long* dst) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  __shared__ unsigned wave_count[kBlock / 64];
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned k = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) k += wave_count[w];
    if (k > 0) atomicAdd(dst, static_cast<unsigned long long>(k));
  }
}
// a counter summed over the wave: one atomic per wave, none for 0 or a null dst
__device__ inline void wave_stat_add(int v, int* dst) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0 && v && dst) atomicAdd(dst, v);
}

// ---- force laws ---------------------------------------------------------------------------------------------------
// A spring of length L = |d| pulls with fm d.  Hookean (r = rest length): fm = k (L - r) (1 / L) (NgpHP1.cpp:1054-1069,
// its association).  FENE (r = r_max), -grad of U = -1/2 k r_max^2 ln(1 - (L / r_max)^2): attractive, and no force (NaN)
// at L >= r_max -- the caller counts that spring as overstretched where !(L < r).
// FENE-WCA (r = r_max), the Kremer-Grest bond in the reference's expressions and association
// (FENEWCASpringsKernel.cpp:147-176): the length is clamped to r_max - 1e-4 (its hard-coded epsilon_reg), so the bond
// never goes without force -- the caller counts it as overstretched where !(L < r - kFeneWcaClamp).  The WCA cutoff
// 2^(1/6) sigma is the handle's, computed once on the host: no pow here.
struct SpringTerm {
  double L, fm;
};
struct WcaParams {
  double epsilon = 1.0, sigma = 1.0, cutoff = 0.0;
};
constexpr double kFeneWcaClamp = 1e-4;
template <int TYPE>
__device__ inline SpringTerm spring_term(V3 d, double k, double r, WcaParams w = WcaParams{}) {
  const double L = sqrt(dot(d, d));
  if (TYPE == MHIP_SPRING_HOOKEAN) return {L, k * (L - r) * (1.0 / L)};
  if (TYPE == MHIP_SPRING_FENEWCA) {
    const double rm = r - kFeneWcaClamp;
    const double La = rm < L ? rm : L;  // std::min(L, rm): a NaN L stays NaN
    const double spring = k * La / (1.0 - (La / r) * (La / r));
    const double rho2 = w.sigma * w.sigma / (La * La);
    const double rho6 = rho2 * rho2 * rho2;
    const double rho12 = rho6 * rho6;
    const double lj = La < w.cutoff ? 6.0 * 4.0 * w.epsilon * (2.0 * rho12 - rho6) / La : 0.0;
    return {L, (spring - lj) * (1.0 / L)};
  }
  const double q = L / r;
  return {L, (L < r) ? k / (1.0 - q * q) : __builtin_nan("")};
}
// f -= fm d or f += fm d: the term is formed in the same operations at both ends of a spring, so the two ends receive
// exactly negated vectors
__device__ inline void add_term(V3& f, bool minus, double fm, V3 d) {
  const V3 t = fm * d;
  f = minus ? f - t : f + t;
}

// The (r, E, nu) of a pair's two bodies (scalar materials are kernel arguments: no per-body gather), its reduced radius
// and effective modulus E* in the reference's expressions and association
// (SpherocylinderSpherocylinderHertzianContact.cpp:205-219).
struct HertzPair {
  double ri, rj, Ei, Ej, vi, vj, Rs, Es;
};
template <bool E_ARRAY, bool NU_ARRAY>
__device__ inline HertzPair hertz_pair(int2 p, const double* __restrict__ radius, const double* __restrict__ E, double E0,
                                       const double* __restrict__ nu, double nu0) {
  HertzPair h;
  h.ri = radius[p.x], h.rj = radius[p.y];
  h.Ei = E_ARRAY ? E[p.x] : E0, h.Ej = E_ARRAY ? E[p.y] : E0;
  h.vi = NU_ARRAY ? nu[p.x] : nu0, h.vj = NU_ARRAY ? nu[p.y] : nu0;
  h.Rs = (h.ri * h.rj) / (h.ri + h.rj);
  h.Es = (h.Ei * h.Ej) / (h.Ej - h.Ej * h.vi * h.vi + h.Ei - h.Ei * h.vj * h.vj);
  return h;
}
// The Hertzian force magnitude of an overlap -s > 0 (...HertzianContact.cpp:217-219; HP1.cpp:4413-4415): the one
// expression hertz.hip and segment_contact.hip evaluate.
__device__ inline double hertz_force_magnitude(double Es, double Rs, double s) {
  return (4.0 / 3.0) * Es * sqrt(Rs) * pow(-s, 1.5);
}
// x^(3/2) for x > 0, rounded once: sqrt(x) = s + s_lo and x s = p + p_lo as unevaluated pairs (the residuals through
// explicit fma), so the sum p + (p_lo + x s_lo) carries ~100 bits before its one rounding.  The library's pow is good
// to an ulp, not to half of one; a host libm's pow is correctly rounded on all but a vanishing share of arguments, so
// where a force must agree with a host evaluation in bits and not to 1e-14 (the end-segment correction of
// segment_contact.hip), this is the pow to use.
__device__ inline double pow_three_halves(double x) {
  const double s = sqrt(x);
  const double s_lo = fma(-s, s, x) / (2.0 * s);
  const double p = x * s;
  const double p_lo = fma(x, s, -p) + x * s_lo;
  return p + p_lo;
}

// (hertz_friction.hip, and the row writers of segment_linkers.hpp)
__device__ inline bool row_is_pos_zero(const double* p, size_t c) {  // the three words of row c are all +0.0
  return (__double_as_longlong(p[3 * c]) | __double_as_longlong(p[3 * c + 1]) | __double_as_longlong(p[3 * c + 2])) == 0;
}
// The frictional Hertzian law of one contact (sep <= 0, or NaN), after the contact-point velocities
// (SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:468-511): rel = v_cp,j - v_cp,i, n the
// normal from i to j, td the pair's history row.  force is the one on body i; td the new history row.
// hertz_friction.hip (rigid rods) and filament_contact.hip (flexible segments) call this one text.
struct FrictionContact {
  V3 force, td;
  bool capped;
};
__device__ inline V3 vdiv(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
__device__ inline FrictionContact hertz_friction_law(V3 rel, V3 n, double s, const HertzPair& h,
                                                     const mhip_hertz_friction_params& prm, V3 td) {
  const V3 rel_n = dot(rel, n) * n;
  const V3 rel_t = rel - rel_n;
  td = td + rel_t * prm.dt;                                                         // :474
  td = td - dot(td, n) * n;                                                         // :475
  const double td_mag = norm(td);
  // the sphere mass of the rod radius, as written (:484-485)
  const double mi = 4.0 / 3.0 * M_PI * h.ri * h.ri * h.ri * prm.density;
  const double mj = 4.0 / 3.0 * M_PI * h.rj * h.rj * h.rj * prm.density;
  const double ms = (mi * mj) / (mi + mj);
  // k_n = 4/3 E* (hertz.hip's E*), k_t = 8 G*: for equal materials 4/3 G / (1 - nu) and 4 G / (2 - nu) (:409-411)
  const double Gi = 0.5 * h.Ei / (1.0 + h.vi), Gj = 0.5 * h.Ej / (1.0 + h.vj);
  const double Gs = (Gi * Gj) / (Gj * (2.0 - h.vi) + Gi * (2.0 - h.vj));
  const double kn = (4.0 / 3.0) * h.Es, kt = 8.0 * Gs;
  const double hp = sqrt(-h.Rs * s);                                                // :490
  const V3 damp_t = (ms * prm.tangential_damping) * rel_t;
  const V3 Fn = hp * ((kn * s) * n + (ms * prm.normal_damping) * rel_n);            // :491-493
  V3 Ft = hp * (kt * td + damp_t);                                                  // :494-495
  const double ft_mag = norm(Ft);
  const double cap = prm.mu * norm(Fn);
  const bool capped = ft_mag > cap;
  if (capped) {  // Coulomb: rescale history and force (:497-511)
    if (td_mag != 0.0) {
      const double ratio = cap / ft_mag;
      const V3 shift = vdiv(damp_t, kt);
      td = ratio * (td + shift) - shift;
      Ft = Ft * ratio;
    } else {
      Ft = V3{0.0, 0.0, 0.0};
    }
  }
  return {Fn + Ft, td, capped};  // on body i; body j receives the negative
}

// The row of body b: force + f or f.  A kernel that leaves the rows of untouched bodies alone in accumulate mode skips
// the call (force + 0.0 would turn a -0.0 into +0.0, and cost the traffic).
template <bool ACCUMULATE>
__device__ inline void write_force(double* __restrict__ force, size_t b, V3 f) {
  store3(force, b, ACCUMULATE ? load3(force, b) + f : f);
}

}  // namespace mhip
