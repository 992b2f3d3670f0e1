// hydro_periphery.hip -- the periphery's no-slip correction of the n-body hydrodynamics (mundy_hip_hydro_periphery.h):
// the second-kind boundary-integral matrix of the surface (fill_skfie_matrix, scrap/.../periphery/Periphery.hpp:1370-1597),
// its inverse (the reference: KokkosBlas::gesv against the identity, :175-210; here an in-place Gauss-Jordan elimination
// with partial pivoting whose every element operation is independent of the launch shape), f_surf = -(Minv u_surf)
// (:2125-2140) and the composite call of the steppers.  The double-layer sum itself is a pair term of hydro.hip.
//   fill      one thread per (t, s) 3x3 block; one wave per row for the row sums; one thread per block to finish
//   invert    per column: one workgroup finds the pivot and copies the column, one launch swaps / scales the pivot row,
//             one updates every other element; the pivot index and value stay on the device
//   matvec    one wave streams a row (row-major, once-read: non-temporal loads), lanes stride by 64, fixed halving tree
// fp64 throughout, -ffp-contract=off, one writer per output, no floating-point atomics.
#include <cmath>
#include <memory>

#include "../../include/mundy_hip_hydro_periphery.h"
#include "mhip_internal.hpp"

namespace mhip {

constexpr double kPeripheryZero = 1.0e-12;  // the reference's DOUBLE_ZERO
constexpr size_t kPeripheryMaxN = 65535;    // a grid dimension of the elimination is N

// Periphery.hpp:71-82 (as in hydro.hip)
__device__ inline double periphery_quake_inv_sqrt(double number) {
  const double x2 = number * 0.5;
  long long i = __double_as_longlong(number);
  i = 0x5fe6eb50c7b537a9ll - (i >> 1);
  const double y = __longlong_as_double(i);
  return y * (1.5 - (x2 * y * y));
}

// ROWSUM's second half: 64 lane sums -> p_0 on every lane (an addition is commutative: the butterfly gives lane 0 the
// bits of the halving tree)
__device__ inline double rowsum_tree(double v) {
  for (int h = 32; h > 0; h >>= 1) v = v + __shfl_xor(v, h, 64);
  return v;
}

// T[3t+i][3s+j] of Periphery.hpp:1416-1446, one thread per (t, s)
__global__ void __launch_bounds__(kBlock) k_periphery_fill(size_t S, const double* __restrict__ y,
                                                           const double* __restrict__ nrm, const double* __restrict__ w,
                                                           double scale, double* __restrict__ T) {
  const size_t s = blockIdx.x * (size_t)kBlock + threadIdx.x;
  const size_t t = blockIdx.y;
  if (s >= S) return;
  const size_t N = 3 * S;
  const double dx = y[3 * t] - y[3 * s];
  const double dy = y[3 * t + 1] - y[3 * s + 1];
  const double dz = y[3 * t + 2] - y[3 * s + 2];
  const double dr2 = dx * dx + dy * dy + dz * dz;
  const double rinv = dr2 < kPeripheryZero ? 0.0 : periphery_quake_inv_sqrt(dr2);
  const double rinv2 = rinv * rinv;
  const double rinv5 = rinv * rinv2 * rinv2;
  const double qw = w[s];
  const double sn0 = nrm[3 * s] * qw, sn1 = nrm[3 * s + 1] * qw, sn2 = nrm[3 * s + 2] * qw;
  const double rdn = dx * sn0 + dy * sn1 + dz * sn2;
  const double v0 = scale * rinv5 * rdn * dx;
  const double v1 = scale * rinv5 * rdn * dy;
  const double v2 = scale * rinv5 * rdn * dz;
  double* r0 = T + (3 * t) * N + 3 * s;
  double* r1 = r0 + N;
  double* r2 = r1 + N;
  r0[0] = dx * v0, r0[1] = dx * v1, r0[2] = dx * v2;
  r1[0] = dy * v0, r1[1] = dy * v1, r1[2] = dy * v2;
  r2[0] = dz * v0, r2[1] = dz * v1, r2[2] = dz * v2;
}

// W[row][c] = ROWSUM_s T[row][3s+c]: one wave per row
__global__ void __launch_bounds__(kBlock) k_periphery_rowsums(size_t S, const double* __restrict__ T,
                                                              double* __restrict__ W) {
  const size_t N = 3 * S;
  const size_t row = blockIdx.x * (size_t)(kBlock / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (row >= N) return;  // (a whole wave)
  const double* r = T + row * N;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0;
  for (size_t s = lane; s < S; s += 64) {
    a0 = a0 + r[3 * s];
    a1 = a1 + r[3 * s + 1];
    a2 = a2 + r[3 * s + 2];
  }
  a0 = rowsum_tree(a0);
  a1 = rowsum_tree(a1);
  a2 = rowsum_tree(a2);
  if (lane == 0) W[3 * row] = a0, W[3 * row + 1] = a1, W[3 * row + 2] = a2;
}

// the singularity subtraction into the diagonal blocks (Periphery.hpp:1515-1529), then the complementary matrix
// (:1570-1596), one thread per (t, s)
__global__ void __launch_bounds__(kBlock) k_periphery_finish(size_t S, const double* __restrict__ nrm,
                                                             const double* __restrict__ w, const double* __restrict__ W,
                                                             double* __restrict__ T) {
  const size_t s = blockIdx.x * (size_t)kBlock + threadIdx.x;
  const size_t t = blockIdx.y;
  if (s >= S) return;
  const size_t N = 3 * S;
  const double qw = w[s];
  const double wn[3] = {nrm[3 * s] * qw, nrm[3 * s + 1] * qw, nrm[3 * s + 2] * qw};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    double* r = T + (3 * t + i) * N + 3 * s;
    const double nt = nrm[3 * t + i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double v = r[j];
      if (t == s) v = v + W[3 * (3 * t + i) + j];
      r[j] = v + nt * wn[j];
    }
  }
}

// the state of an elimination on the device
struct GjState {
  double pivot;      // the pivot value of the current column
  double min_pivot;  // the smallest |pivot| so far
  int row;           // the pivot row of the current column
  int bad;           // a pivot was zero or not finite: every later launch returns at once
};

// column k: the pivot (largest |A[i][k]| of rows k .. N-1, the lowest index on a tie) and the column as it stands after
// the row swap, col[i] = A[i][k] (col[k] is not used).  One workgroup.
__global__ void __launch_bounds__(kBlock) k_gj_pivot(size_t N, size_t k, const double* __restrict__ A,
                                                     double* __restrict__ col, int* __restrict__ piv, GjState* st) {
  __shared__ double best_v[kBlock];
  __shared__ int best_i[kBlock];
  if (st->bad) return;
  double bv = -1.0;
  int bi = static_cast<int>(N);
  bool nan = false;
  for (size_t i = threadIdx.x; i < N; i += kBlock) {
    const double a = A[i * N + k];
    col[i] = a;
    if (i >= k) {
      const double m = fabs(a);
      nan |= !(m == m);
      if (m > bv) bv = m, bi = static_cast<int>(i);  // ascending i: the first of equal magnitudes stays
    }
  }
  if (nan) bv = __builtin_inf(), bi = -1;  // (refused below)
  best_v[threadIdx.x] = bv;
  best_i[threadIdx.x] = bi;
  __syncthreads();
  for (int h = kBlock / 2; h > 0; h >>= 1) {
    if (threadIdx.x < h) {
      const double ov = best_v[threadIdx.x + h];
      const int oi = best_i[threadIdx.x + h];
      if (ov > best_v[threadIdx.x] || (ov == best_v[threadIdx.x] && oi < best_i[threadIdx.x]))
        best_v[threadIdx.x] = ov, best_i[threadIdx.x] = oi;
    }
    __syncthreads();
  }
  const int p = best_i[0];
  const double m = best_v[0];
  if (p < 0 || p >= static_cast<int>(N) || !(m > 0.0) || !(m < __builtin_inf())) {
    if (threadIdx.x == 0) st->bad = 1;
    return;
  }
  __syncthreads();  // every col[i] is written
  if (threadIdx.x == 0) {
    const double pv = col[p];
    col[p] = col[k];  // the swap, as the column sees it
    piv[k] = p;
    st->row = p;
    st->pivot = pv;
    if (m < st->min_pivot) st->min_pivot = m;
  }
}

// rows k and p swap; row k: A[k][k] = 1.0, then A[k][j] / pv; rowk[j] keeps the new row k.  One thread per column j.
__global__ void __launch_bounds__(kBlock) k_gj_row(size_t N, size_t k, double* __restrict__ A, double* __restrict__ rowk,
                                                   const GjState* st) {
  if (st->bad) return;
  const size_t j = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (j >= N) return;
  const size_t p = static_cast<size_t>(st->row);
  const double pv = st->pivot;
  const double a = A[k * N + j];
  const double b = A[p * N + j];
  const double v = (j == k ? 1.0 : b) / pv;
  rowk[j] = v;
  A[k * N + j] = v;
  if (p != k) A[p * N + j] = a;
}

// every row i != k: A[i][j] = (j == k ? 0.0 : A[i][j]) - col[i] rowk[j], two roundings.  grid (columns / 256, rows)
__global__ void __launch_bounds__(kBlock) k_gj_update(size_t N, size_t k, double* __restrict__ A,
                                                      const double* __restrict__ col, const double* __restrict__ rowk,
                                                      const GjState* st) {
  if (st->bad) return;
  const size_t j = blockIdx.x * (size_t)kBlock + threadIdx.x;
  const size_t i = blockIdx.y;
  if (j >= N || i == k) return;
  const double f = col[i];
  double* a = A + i * N + j;
  const double old = j == k ? 0.0 : *a;
  *a = old - f * rowk[j];
}

// the column swaps undone, k = N-1 .. 0: one thread per row walks its own row
__global__ void __launch_bounds__(kBlock) k_gj_unswap(size_t N, double* __restrict__ A, const int* __restrict__ piv,
                                                      const GjState* st) {
  if (st->bad) return;
  const size_t i = blockIdx.x * (size_t)kBlock + threadIdx.x;
  if (i >= N) return;
  double* r = A + i * N;
  for (size_t k = N; k-- > 0;) {
    const size_t p = static_cast<size_t>(piv[k]);
    if (p != k) {
      const double a = r[k];
      r[k] = r[p];
      r[p] = a;
    }
  }
}

// f[r] = -(ROWSUM_j Minv[r][j] u[j]): one wave per row, the matrix read once
__global__ void __launch_bounds__(kBlock) k_periphery_matvec(size_t N, const double* __restrict__ Minv,
                                                             const double* __restrict__ u, double* __restrict__ f) {
  const size_t row = blockIdx.x * (size_t)(kBlock / 64) + threadIdx.x / 64;
  const int lane = threadIdx.x % 64;
  if (row >= N) return;  // (a whole wave)
  const double* r = Minv + row * N;
  double acc = 0.0;
  size_t j = lane;
  for (; j + 192 < N; j += 256) {  // four loads in flight; the sum stays in ascending j
    const double m0 = __builtin_nontemporal_load(r + j), m1 = __builtin_nontemporal_load(r + j + 64),
                 m2 = __builtin_nontemporal_load(r + j + 128), m3 = __builtin_nontemporal_load(r + j + 192);
    acc = acc + m0 * u[j];
    acc = acc + m1 * u[j + 64];
    acc = acc + m2 * u[j + 128];
    acc = acc + m3 * u[j + 192];
  }
  for (; j < N; j += 64) acc = acc + __builtin_nontemporal_load(r + j) * u[j];
  acc = rowsum_tree(acc);
  if (lane == 0) f[row] = -acc;
}

}  // namespace mhip

using namespace mhip;

namespace mhip {
int hydro_periphery_correct(mhip_hydro_periphery* h, mhip_hydro* ws, int kind, size_t n, const double* center,
                            const double* radius, const double* force, double* velocity, int velocity_stride,
                            int skip_same_index, const HydroLaunchOptions* opt, mhip_stream_t stream);
}

struct mhip_hydro_periphery {
  size_t S = 0;
  double viscosity = 0.0;
  int state = MHIP_HYDRO_PERIPHERY_EMPTY;
  HandleBuffer points, weights, normals;  // copies of the quadrature
  HandleBuffer matrix;                    // [N][N]: M after a fill, Minv after the inversion
  HandleBuffer zero_radius;               // [S] zeros: the nodes as targets of mhip_hydro_velocity
  HandleBuffer u_surf, f_surf;            // [N] each
  HandleBuffer col, rowk, rowsum, piv, gj;  // the elimination's column, row, pivots and state; the fill's W [N][3]
  size_t n() const { return 3 * S; }
};

static int periphery_load(mhip_hydro_periphery_t h, const double* src, int state, hipStream_t s) {
  const size_t bytes = h->n() * h->n() * sizeof(double);
  if (int e = h->matrix.reserve(bytes)) return e;
  MHIP_HIP(hipMemcpyAsync(h->matrix.ptr, src, bytes, hipMemcpyDeviceToDevice, s));
  h->state = state;
  return MHIP_SUCCESS;
}

static int periphery_surface_forces(mhip_hydro_periphery_t h, const double* u, double* f, hipStream_t s) {
  const size_t N = h->n();
  k_periphery_matvec<<<grid_exact(N, kBlock / 64), kBlock, 0, s>>>(N, h->matrix.as<double>(), u, f);
  MHIP_LAUNCH_CHECK();
  return MHIP_SUCCESS;
}

extern "C" {

int mhip_hydro_periphery_create(mhip_hydro_periphery_t* handle, size_t num_nodes, const double* points,
                                const double* weights, const double* normals, double viscosity, mhip_stream_t stream) {
  MHIP_REQUIRE(handle != nullptr, MHIP_ERR_INVALID_ARGUMENT, "handle is null");
  MHIP_REQUIRE(num_nodes > 0, MHIP_ERR_INVALID_ARGUMENT, "a periphery needs at least one surface node");
  MHIP_REQUIRE(3 * num_nodes <= kPeripheryMaxN, MHIP_ERR_INVALID_ARGUMENT, "too many surface nodes: 3 S = %zu > %zu",
               3 * num_nodes, kPeripheryMaxN);
  MHIP_REQUIRE(points && weights && normals, MHIP_ERR_INVALID_ARGUMENT, "points / weights / normals is null");
  MHIP_REQUIRE(std::isfinite(viscosity) && viscosity > 0.0, MHIP_ERR_INVALID_ARGUMENT,
               "viscosity must be finite and > 0, got %g", viscosity);
  hipStream_t s = as_stream(stream);
  auto h = std::make_unique<mhip_hydro_periphery>();
  h->S = num_nodes;
  h->viscosity = viscosity;
  const size_t S = num_nodes, N = 3 * S, d = sizeof(double);
  for (HandleBuffer* b : {&h->points, &h->normals, &h->u_surf, &h->f_surf})
    if (int e = b->reserve(N * d)) return e;
  for (HandleBuffer* b : {&h->weights, &h->zero_radius})
    if (int e = b->reserve(S * d)) return e;
  MHIP_HIP(hipMemcpyAsync(h->points.ptr, points, N * d, hipMemcpyDeviceToDevice, s));
  MHIP_HIP(hipMemcpyAsync(h->normals.ptr, normals, N * d, hipMemcpyDeviceToDevice, s));
  MHIP_HIP(hipMemcpyAsync(h->weights.ptr, weights, S * d, hipMemcpyDeviceToDevice, s));
  MHIP_HIP(hipMemsetAsync(h->zero_radius.ptr, 0, S * d, s));
  *handle = h.release();
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_destroy(mhip_hydro_periphery_t h) {
  delete h;
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_fill_double_layer(mhip_hydro_periphery_t h, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  const size_t S = h->S, N = h->n();
  if (int e = h->matrix.reserve(N * N * sizeof(double))) return e;
  const double scale = -3.0 / (4.0 * M_PI * h->viscosity);
  const dim3 grid(grid_exact(S), static_cast<unsigned>(S), 1);
  k_periphery_fill<<<grid, kBlock, 0, as_stream(stream)>>>(S, h->points.as<double>(), h->normals.as<double>(),
                                                           h->weights.as<double>(), scale, h->matrix.as<double>());
  MHIP_LAUNCH_CHECK();
  h->state = MHIP_HYDRO_PERIPHERY_DOUBLE_LAYER;
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_fill_matrix(mhip_hydro_periphery_t h, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  const size_t S = h->S, N = h->n();
  if (int e = h->rowsum.reserve(3 * N * sizeof(double))) return e;
  if (int e = mhip_hydro_periphery_fill_double_layer(h, stream)) return e;
  h->state = MHIP_HYDRO_PERIPHERY_EMPTY;
  hipStream_t s = as_stream(stream);
  k_periphery_rowsums<<<grid_exact(N, kBlock / 64), kBlock, 0, s>>>(S, h->matrix.as<double>(), h->rowsum.as<double>());
  MHIP_LAUNCH_CHECK();
  const dim3 grid(grid_exact(S), static_cast<unsigned>(S), 1);
  k_periphery_finish<<<grid, kBlock, 0, s>>>(S, h->normals.as<double>(), h->weights.as<double>(),
                                             h->rowsum.as<double>(), h->matrix.as<double>());
  MHIP_LAUNCH_CHECK();
  h->state = MHIP_HYDRO_PERIPHERY_MATRIX;
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_set_matrix(mhip_hydro_periphery_t h, const double* matrix, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  MHIP_REQUIRE(matrix != nullptr, MHIP_ERR_INVALID_ARGUMENT, "matrix is null");
  return periphery_load(h, matrix, MHIP_HYDRO_PERIPHERY_MATRIX, as_stream(stream));
}

int mhip_hydro_periphery_set_inverse(mhip_hydro_periphery_t h, const double* inverse, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  MHIP_REQUIRE(inverse != nullptr, MHIP_ERR_INVALID_ARGUMENT, "inverse is null");
  return periphery_load(h, inverse, MHIP_HYDRO_PERIPHERY_INVERSE, as_stream(stream));
}

int mhip_hydro_periphery_matrix(mhip_hydro_periphery_t h, const double** matrix, int* state) {
  MHIP_REQUIRE(h != nullptr && matrix != nullptr && state != nullptr, MHIP_ERR_INVALID_ARGUMENT,
               "periphery handle / matrix / state is null");
  *matrix = h->state == MHIP_HYDRO_PERIPHERY_EMPTY ? nullptr : h->matrix.as<double>();
  *state = h->state;
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_invert(mhip_hydro_periphery_t h, double* min_pivot, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  MHIP_REQUIRE(min_pivot != nullptr, MHIP_ERR_INVALID_ARGUMENT, "min_pivot is null");
  MHIP_REQUIRE(h->state == MHIP_HYDRO_PERIPHERY_MATRIX, MHIP_ERR_LOGIC,
               "invert needs a matrix: call fill_matrix or set_matrix first");
  const size_t N = h->n();
  hipStream_t s = as_stream(stream);
  for (HandleBuffer* b : {&h->col, &h->rowk})
    if (int e = b->reserve(N * sizeof(double))) return e;
  if (int e = h->piv.reserve(N * sizeof(int))) return e;
  if (int e = h->gj.reserve(sizeof(GjState))) return e;
  GjState st{};
  st.min_pivot = __builtin_inf();
  MHIP_HIP(hipMemcpyAsync(h->gj.ptr, &st, sizeof(st), hipMemcpyHostToDevice, s));
  MHIP_HIP(hipStreamSynchronize(s));  // (st is a local: pageable memory is staged before the copy returns, and this
                                      //  entry point synchronises anyway)
  double* A = h->matrix.as<double>();
  double *col = h->col.as<double>(), *rowk = h->rowk.as<double>();
  int* piv = h->piv.as<int>();
  GjState* dst = h->gj.as<GjState>();
  h->state = MHIP_HYDRO_PERIPHERY_EMPTY;
  const dim3 grid(grid_exact(N), static_cast<unsigned>(N), 1);
  for (size_t k = 0; k < N; ++k) {
    k_gj_pivot<<<1, kBlock, 0, s>>>(N, k, A, col, piv, dst);
    k_gj_row<<<grid_exact(N), kBlock, 0, s>>>(N, k, A, rowk, dst);
    k_gj_update<<<grid, kBlock, 0, s>>>(N, k, A, col, rowk, dst);
  }
  MHIP_LAUNCH_CHECK();
  k_gj_unswap<<<grid_exact(N), kBlock, 0, s>>>(N, A, piv, dst);
  MHIP_LAUNCH_CHECK();
  MHIP_HIP(hipMemcpyAsync(&st, dst, sizeof(st), hipMemcpyDeviceToHost, s));
  MHIP_HIP(hipStreamSynchronize(s));
  MHIP_REQUIRE(!st.bad, MHIP_ERR_RUNTIME, "the matrix is singular to working precision: a pivot is zero or not finite");
  *min_pivot = st.min_pivot;
  h->state = MHIP_HYDRO_PERIPHERY_INVERSE;
  return MHIP_SUCCESS;
}

int mhip_hydro_periphery_surface_forces(mhip_hydro_periphery_t h, const double* u_surf, double* f_surf,
                                        mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  MHIP_REQUIRE(u_surf && f_surf, MHIP_ERR_INVALID_ARGUMENT, "u_surf / f_surf is null");
  MHIP_REQUIRE(h->state == MHIP_HYDRO_PERIPHERY_INVERSE, MHIP_ERR_LOGIC,
               "surface_forces needs the inverse: call invert or set_inverse first");
  return periphery_surface_forces(h, u_surf, f_surf, as_stream(stream));
}

int mhip_hydro_periphery_correct(mhip_hydro_periphery_t h, mhip_hydro_t ws, int kind, size_t n, const double* center,
                                 const double* radius, const double* force, double* velocity, int velocity_stride,
                                 int skip_same_index, mhip_stream_t stream) {
  return hydro_periphery_correct(h, ws, kind, n, center, radius, force, velocity, velocity_stride, skip_same_index,
                                 nullptr, stream);
}

}  // extern "C"

// the composite call with the launch options of its two pair sums (mhip_internal.hpp; the hydrodynamic solve gates them)
int mhip::hydro_periphery_correct(mhip_hydro_periphery* h, mhip_hydro* ws, int kind, size_t n, const double* center,
                                  const double* radius, const double* force, double* velocity, int velocity_stride,
                                  int skip_same_index, const HydroLaunchOptions* opt, mhip_stream_t stream) {
  MHIP_REQUIRE(h != nullptr, MHIP_ERR_INVALID_ARGUMENT, "periphery handle is null");
  MHIP_REQUIRE(ws != nullptr, MHIP_ERR_INVALID_ARGUMENT, "hydro handle is null");
  MHIP_REQUIRE(kind == MHIP_HYDRO_STOKES || kind == MHIP_HYDRO_RPY || kind == MHIP_HYDRO_RPYC,
               MHIP_ERR_INVALID_ARGUMENT, "unknown hydrodynamic kernel kind %d", kind);
  MHIP_REQUIRE(velocity_stride == 3 || velocity_stride == 6, MHIP_ERR_INVALID_ARGUMENT,
               "velocity_stride must be 3 or 6, got %d", velocity_stride);
  MHIP_REQUIRE(n == 0 || (center && force && velocity && (radius || kind == MHIP_HYDRO_STOKES)),
               MHIP_ERR_INVALID_ARGUMENT, "center / radius / force / velocity is null");
  MHIP_REQUIRE(h->state == MHIP_HYDRO_PERIPHERY_INVERSE, MHIP_ERR_LOGIC,
               "correct needs the inverse: call invert or set_inverse first");
  if (n == 0) return MHIP_SUCCESS;
  const size_t S = h->S;
  double *u = h->u_surf.as<double>(), *f = h->f_surf.as<double>();
  const double* y = h->points.as<double>();
  if (int e = hydro_velocity(ws, kind, h->viscosity, n, center, radius, force, S, y, h->zero_radius.as<double>(), u, 3, 0,
                             opt, stream))
    return e;
  if (int e = periphery_surface_forces(h, u, f, as_stream(stream))) return e;
  return hydro_double_layer(ws, h->viscosity, S, y, h->normals.as<double>(), h->weights.as<double>(), f, n, center,
                            velocity, velocity_stride, 1, skip_same_index, opt, stream);
}
