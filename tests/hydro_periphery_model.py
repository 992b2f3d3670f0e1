"""numpy float64 restatement of the periphery's no-slip correction (include/mundy_hip_hydro_periphery.h), written from
the reference's text (scrap/.../periphery/Periphery.hpp: gen_sphere_quadrature :90-167, fill_skfie_matrix :1370-1597,
apply_stokes_double_layer_kernel :1221-1313, compute_surface_forces :2125-2140; HP1.cpp:4005-4037), every product and
sum in the reference's association (no `**`, no fused operations: numpy rounds every elementwise operation once), with
the orders of summation the header documents:
  ROWSUM (the fill's row sums, the matrix-vector product): 64 partial sums over the indices l, l + 64, ... in ascending
    order from +0.0, then the halvings p[:h] + p[h:2h], h = 32 .. 1;
  the double layer: hydro_model's chunked sums (chunks of CHUNK sources, ascending, chunk sums ascending, old value last).
The inverse is the header's in-place Gauss-Jordan elimination with partial pivoting, operation for operation."""
import math

import numpy as np

import hydro_model as hm

LANES = 64


def sphere_quadrature(order, radius, include_poles=False, invert=False):
    """gen_sphere_quadrature as its loops are written -> points [S, 3], weights [S], normals [S, 3]"""
    nodes_gl, weights_gl = np.polynomial.legendre.leggauss(order + 1)
    num = (order + 1) * (2 * order + 2) + (2 if include_poles else 0)
    points, weights, normals = np.zeros((num, 3)), np.zeros(num), np.zeros((num, 3))
    if include_poles:
        points[0] = (0.0, 0.0, 1.0)
    weightfactor = radius * radius * 2 * math.pi / (2 * order + 2)
    for j in range(order + 1):
        for k in range(2 * order + 2):
            cos_t = nodes_gl[order - j]
            phi = 2 * math.pi * k / (2 * order + 2)
            sin_t = math.sqrt(1 - cos_t * cos_t)
            index = j * (2 * order + 2) + k + (1 if include_poles else 0)
            points[index] = (sin_t * math.cos(phi), sin_t * math.sin(phi), cos_t)
            weights[index] = weightfactor * weights_gl[order - j]
    if include_poles:
        points[num - 1] = (0.0, 0.0, -1.0)
    normals[:] = (-1.0 if invert else 1.0) * points
    points *= radius
    return points, weights, normals


def rowsum(a):
    """ROWSUM over the last axis of a [rows, L]"""
    rows, L = a.shape
    K = (L + LANES - 1) // LANES
    pad = np.zeros((rows, K * LANES))  # (+0.0 added to a partial sum that started from +0.0 changes no bit)
    pad[:, :L] = a
    pad = pad.reshape(rows, K, LANES)
    p = np.zeros((rows, LANES))
    for k in range(K):
        p = p + pad[:, k, :]
    h = LANES // 2
    while h > 0:
        p = p[:, :h] + p[:, h:2 * h]
        h //= 2
    return p[:, 0]


def _rinv5(r2):
    with np.errstate(all="ignore"):
        rinv = np.where(r2 < hm.DOUBLE_ZERO, 0.0, hm.quake_inv_sqrt(r2).reshape(r2.shape))
    rinv2 = rinv * rinv
    return (rinv * rinv2) * rinv2


def double_layer_matrix(points, weights, normals, viscosity):
    """T [3S, 3S] of fill_stokes_double_layer_matrix"""
    S = points.shape[0]
    scale = np.float64(-3.0) / ((np.float64(4.0) * np.float64(math.pi)) * np.float64(viscosity))
    d = points[:, None, :] - points[None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    rinv5 = _rinv5((dx * dx + dy * dy) + dz * dz)
    sn = normals * weights[:, None]
    rdn = (dx * sn[None, :, 0] + dy * sn[None, :, 1]) + dz * sn[None, :, 2]
    pre = (scale * rinv5) * rdn
    T = np.zeros((S, 3, S, 3))
    for i in range(3):
        for j in range(3):
            T[:, i, :, j] = d[..., i] * (pre * d[..., j])
    return T.reshape(3 * S, 3 * S)


def fill_matrix(points, weights, normals, viscosity):
    """(T, M): the double-layer block, then singularity subtraction and the complementary matrix"""
    S = points.shape[0]
    T = double_layer_matrix(points, weights, normals, viscosity)
    W = np.stack([rowsum(np.ascontiguousarray(T[:, c::3])) for c in range(3)], axis=1)  # [3S, 3]
    M = T.copy().reshape(S, 3, S, 3)
    idx = np.arange(S)
    M[idx, :, idx, :] = M[idx, :, idx, :] + W.reshape(S, 3, 3)
    wn = normals * weights[:, None]
    M = M + normals[:, :, None, None] * wn[None, None, :, :]
    return T, M.reshape(3 * S, 3 * S)


class SingularMatrix(RuntimeError):
    pass


def gauss_jordan(A):
    """-> (inverse, min_pivot, number of row swaps) by the header's algorithm"""
    A = np.array(A, dtype=np.float64)
    N = A.shape[0]
    piv = np.zeros(N, dtype=np.int64)
    min_pivot, swaps = np.inf, 0
    with np.errstate(all="ignore"):
        for k in range(N):
            mag = np.abs(A[k:, k])
            if np.isnan(mag).any():
                raise SingularMatrix("column %d holds a NaN" % k)
            p = k + int(np.argmax(mag))  # the first of equal magnitudes
            m = mag[p - k]
            if not (m > 0.0 and m < np.inf):
                raise SingularMatrix("pivot %d is %r" % (k, m))
            piv[k] = p
            if p != k:
                A[[k, p]] = A[[p, k]]
                swaps += 1
            min_pivot = min(min_pivot, m)
            pv = A[k, k]
            A[k, k] = 1.0
            rowk = A[k] / pv
            f = A[:, k].copy()
            A[:, k] = 0.0
            A = A - f[:, None] * rowk[None, :]
            A[k] = rowk
        for k in range(N - 1, -1, -1):
            p = piv[k]
            if p != k:
                A[:, [k, p]] = A[:, [p, k]]
    return A, float(min_pivot), swaps


def surface_forces(Minv, u_surf, rows=None):
    """f = -(ROWSUM_j Minv[r][j] u[j]) for every row (or the rows listed)"""
    M = Minv if rows is None else Minv[rows]
    return -rowsum(M * u_surf.reshape(-1)[None, :])


def dl_terms(viscosity, tgt, center, normal, weight, force):
    """the pair terms [nt, ns, 3] of apply_stokes_double_layer_kernel (no skip)"""
    nscale = -(np.float64(3.0) / ((np.float64(4.0) * np.float64(math.pi)) * np.float64(viscosity)))
    n, f, w = normal, force, weight
    s = [[(n[:, i] * f[:, j]) * w for j in range(3)] for i in range(3)]
    sxy, sxz, syz = s[0][1] + s[1][0], s[0][2] + s[2][0], s[1][2] + s[2][1]
    d = tgt[:, None, :] - center[None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    rinv5 = _rinv5((dx * dx + dy * dy) + dz * dz)
    coeff = ((s[0][0][None] * dx) * dx + (s[1][1][None] * dy) * dy) + (s[2][2][None] * dz) * dz
    coeff = coeff + (sxy[None] * dx) * dy
    coeff = coeff + (sxz[None] * dx) * dz
    coeff = coeff + (syz[None] * dy) * dz
    coeff = coeff * (nscale * rinv5)
    return d * coeff[..., None]


def double_layer(viscosity, center, normal, weight, force, tgt, old=None, skip_same_index=True, targets=None,
                 chunk=hm.CHUNK, block=256):
    """u [nt, 3] in mhip_hydro_velocity's order; targets: the row indices of tgt in the full target array (default
    arange(nt)), which decide what skip_same_index skips"""
    ns, nt = center.shape[0], tgt.shape[0]
    tidx = np.arange(nt) if targets is None else np.asarray(targets)
    total = np.zeros((nt, 3))
    for c0 in range(0, ns, chunk):
        acc = np.zeros((nt, 3))
        for s0 in range(c0, min(c0 + chunk, ns), block):
            s1 = min(s0 + block, c0 + chunk, ns)
            terms = dl_terms(viscosity, tgt, center[s0:s1], normal[s0:s1], weight[s0:s1], force[s0:s1])
            if skip_same_index:
                same = tidx[:, None] == np.arange(s0, s1)[None, :]
                terms = np.where(same[..., None], 0.0, terms)
            acc = np.add.accumulate(np.concatenate([acc[:, None, :], terms], axis=1), axis=1)[:, -1, :]
        total = total + acc
    return total if old is None else old + total


def surface_velocity(kind, viscosity, center, radius, force, points):
    """u_surf [S, 3] = K(beads -> nodes) F with node radius 0"""
    return hm.velocity(kind, viscosity, center, radius, force, points, np.zeros(points.shape[0]))


def correct(kind, viscosity, points, weights, normals, Minv, center, radius, force, old=None, skip_same_index=True,
            targets=None, tgt=None):
    """the composite call: (u, u_surf, f_surf); tgt / targets: a sample of the beads as targets of the last step"""
    u_surf = surface_velocity(kind, viscosity, center, radius, force, points)
    f_surf = surface_forces(Minv, u_surf).reshape(-1, 3)
    u = double_layer(viscosity, points, normals, weights, f_surf, center if tgt is None else tgt, old=old,
                     skip_same_index=skip_same_index, targets=targets)
    return u, u_surf, f_surf


def stokeslet_in_sphere_correction(x, F, R, viscosity):
    """the image flow of a Stokeslet F at the centre of a no-slip sphere of radius R, at x [n, 3]:
    c [-3 F / R + (2 |x|^2 F - (F.x) x) / R^3], c = 1 / (8 pi mu)"""
    c = 1.0 / (8.0 * math.pi * viscosity)
    x2 = (x * x).sum(axis=1)[:, None]
    return c * (-3.0 * F[None, :] / R + (2.0 * x2 * F[None, :] - (x @ F)[:, None] * x) / R ** 3)


def centred_stokeslet_error(order, R=5.0, viscosity=1.0, ntargets=40, seed=0, skip_same_index=False, kind="rpyc",
                            lapack=False):
    """relative error (max norm over the targets / max norm of the closed form) of the correction a unit Stokeslet at
    the centre induces at ntargets seeded points with |x| <= 0.6 R; lapack: numpy.linalg.inv instead of gauss_jordan"""
    rng = np.random.default_rng(seed)
    F = np.array([0.3, -1.1, 0.5])
    v = rng.normal(size=(ntargets, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    x = v * (0.6 * R * rng.uniform(0.0, 1.0, ntargets) ** (1.0 / 3.0))[:, None]
    pts, w, nrm = sphere_quadrature(order, R, include_poles=False, invert=True)
    _, M = fill_matrix(pts, w, nrm, viscosity)
    Minv = np.linalg.inv(M) if lapack else gauss_jordan(M)[0]
    u_surf = surface_velocity(kind, viscosity, np.zeros((1, 3)), np.zeros(1), F[None, :], pts)
    f_surf = surface_forces(Minv, u_surf).reshape(-1, 3)
    got = double_layer(viscosity, pts, nrm, w, f_surf, x, skip_same_index=skip_same_index)
    want = stokeslet_in_sphere_correction(x, F, R, viscosity)
    return float(np.abs(got - want).max() / np.abs(want).max())
