"""numpy restatement of the colony step (Bacteria.cpp:905-966, :685-748) as the library defines it, operation by operation
in the device's association (fp64, no contraction), so that the GPU can be compared bit for bit.

  divide: body i (ascending) divides iff length[i] > D (strict; NaN never); the k-th divider gets child row n + k.
          t = qrot(q, zhat); cl = 0.5 L - r; s = r + 0.5 cl; off = t * s;
          child = (c + off, q, r, cl), parent = (c - off, q, r, cl); both centres wrapped into [0, L) when periodic
  grow:   every length (children included) += g, g = dt * rate computed once
  moved:  some corner's dx*dx + dy*dy + dz*dz >= threshold*threshold (left to right)
"""
import numpy as np


def qmul(q, o):
    """mhip_internal.hpp qmul, columns (w, x, y, z), left-to-right sums"""
    qw, qx, qy, qz = q
    ow, ox, oy, oz = o
    return (((qw * ow - qx * ox) - qy * oy) - qz * oz,
            ((qw * ox + qx * ow) + qy * oz) - qz * oy,
            ((qw * oy - qx * oz) + qy * ow) + qz * ox,
            ((qw * oz + qx * oy) - qy * ox) + qz * ow)


def qrot_z(quat):
    """qrot(q, (0, 0, 1)) of mhip_internal.hpp:114-120: q (0, v) q^-1 with q^-1 = conj(q) * (1 / |q|^2)"""
    q = np.asarray(quat, dtype=np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    inv = 1.0 / (((w * w + x * x) + y * y) + z * z)
    qi = (w * inv, -x * inv, -y * inv, -z * inv)
    zero, one = np.zeros_like(w), np.ones_like(w)
    r = qmul(qmul((w, x, y, z), (zero, zero, zero, one)), qi)
    return np.stack([r[1], r[2], r[3]], axis=1)


def unit_mod1(s):
    """impl::safe_unit_mod1 as geom_device.hpp unit_mod1"""
    k = np.floor(s).astype(np.int64).astype(np.float64)
    t = s - k
    return np.where(np.abs(t - 1.0) < 1e-15, 0.0, t)


def wrap(box, p):
    """PeriodicScaledMetric::wrap of centres [m, 3] (mhip_wrap_rigid)"""
    b = np.asarray(box, dtype=np.float64)
    inv = 1.0 / b
    return np.stack([b[a] * unit_mod1(inv[a] * p[:, a]) for a in range(3)], axis=1)


def select_dividing(length, division_length):
    """ascending indices with length > D (NaN compares false)"""
    with np.errstate(invalid="ignore"):
        return np.nonzero(np.asarray(length) > division_length)[0].astype(np.int32)


def divide_grow(center, quat, radius, length, parent_of, dt, growth_rate, box=None):
    """one divide + grow on n bodies: returns (center, quat, radius, length) of n + nb bodies (new arrays)"""
    n, nb = len(radius), len(parent_of)
    g = dt * growth_rate
    c = np.concatenate([center, np.zeros((nb, 3))])
    q = np.concatenate([quat, np.zeros((nb, 4))])
    r = np.concatenate([radius, np.zeros(nb)])
    L = np.concatenate([length, np.zeros(nb)])
    if nb:
        p = np.asarray(parent_of, dtype=np.int64)
        t = qrot_z(quat[p])
        cl = 0.5 * length[p] - radius[p]
        s = radius[p] + 0.5 * cl
        off = t * s[:, None]
        child, parent = center[p] + off, center[p] - off
        if box is not None:
            child, parent = wrap(box, child), wrap(box, parent)
        kids = n + np.arange(nb)
        c[p], c[kids] = parent, child
        q[kids] = quat[p]
        r[kids] = radius[p]
        L[p] = cl
        L[kids] = cl
    return c, q, r, L + g


def aabb_moved(aabb, ref, threshold):
    d = np.asarray(aabb) - np.asarray(ref)
    t2 = threshold * threshold
    lo = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    hi = (d[:, 3] * d[:, 3] + d[:, 4] * d[:, 4]) + d[:, 5] * d[:, 5]
    return bool(((lo >= t2) | (hi >= t2)).any())


def length_recursion(length, radius, division_length, dt, growth_rate, steps):
    """lengths alone (positions do not enter): per step, the body count and the sorted lengths after the step"""
    L, r = np.asarray(length, dtype=np.float64).copy(), np.asarray(radius, dtype=np.float64).copy()
    g = dt * growth_rate
    out = []
    for _ in range(steps):
        p = select_dividing(L, division_length)
        cl = 0.5 * L[p] - r[p]
        L[p] = cl
        L = np.concatenate([L, cl]) + g
        r = np.concatenate([r, r[p]])
        out.append((len(L), np.sort(L)))
    return out
