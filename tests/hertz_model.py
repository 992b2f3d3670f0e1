"""numpy restatement of the Hertzian soft-contact step (scrap/parameter_interface/alens/tests/performance_tests/
Bacteria.cpp:755-848 and the Hertzian contact kernels of evaluate_linker_potentials) -- the checker of the soft-contact
tests.  Same expressions and association as the reference:

    R* = r_i r_j / (r_i + r_j)        E* = E_i E_j / (E_j - E_j nu_i^2 + E_i - E_i nu_j^2)
    f  = (4/3) E* sqrt(R*) (-sep)^1.5  (sep < 0), else +0.0

body i receives -f n at its contact point, body j +f n; torque (cp - x_body) x F; dry drag U = m_t F, W = m_r T.
"""
import numpy as np


def per_body(v, n):
    """a number or an [n] array -> [n] float64 array"""
    a = np.asarray(v, dtype=np.float64)
    return np.full(n, float(a)) if a.ndim == 0 else a


def effective_radius(ri, rj):
    return (ri * rj) / (ri + rj)


def effective_modulus(Ei, Ej, vi, vj):
    return (Ei * Ej) / (Ej - Ej * vi * vi + Ei - Ei * vj * vj)


def hertz_force(pairs, sep, radius, youngs_modulus=1000.0, poisson_ratio=0.3):
    """per-linker force magnitude [C] (+0.0 where sep >= 0) and the largest overlap max(0, -sep)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    sep = np.asarray(sep, dtype=np.float64)
    n = len(radius)
    r, E, nu = (per_body(a, n) for a in (radius, youngs_modulus, poisson_ratio))
    i, j = pairs[:, 0], pairs[:, 1]
    Rs = effective_radius(r[i], r[j])
    Es = effective_modulus(E[i], E[j], nu[i], nu[j])
    over = sep < 0.0
    with np.errstate(invalid="ignore"):
        f = np.where(over, (4.0 / 3.0) * Es * np.sqrt(Rs) * np.power(np.where(over, -sep, 0.0), 1.5), 0.0)
    max_overlap = float(np.max(np.where(over, -sep, 0.0))) if len(sep) else 0.0
    return f, max_overlap


def elastic_energy(pairs, sep, radius, youngs_modulus=1000.0, poisson_ratio=0.3):
    """sum over overlapping linkers of (8/15) E* sqrt(R*) delta^(5/2): the potential whose gradient the force is"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(radius)
    r, E, nu = (per_body(a, n) for a in (radius, youngs_modulus, poisson_ratio))
    i, j = pairs[:, 0], pairs[:, 1]
    d = np.maximum(-np.asarray(sep, dtype=np.float64), 0.0)
    return float(np.sum((8.0 / 15.0) * effective_modulus(E[i], E[j], nu[i], nu[j]) * np.sqrt(effective_radius(r[i], r[j]))
                        * d ** 2.5))


def stiffness(pairs, sep, radius, youngs_modulus=1000.0, poisson_ratio=0.3):
    """df / d(delta) = 2 E* sqrt(R* delta) per linker (0 where sep >= 0)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    n = len(radius)
    r, E, nu = (per_body(a, n) for a in (radius, youngs_modulus, poisson_ratio))
    i, j = pairs[:, 0], pairs[:, 1]
    d = np.maximum(-np.asarray(sep, dtype=np.float64), 0.0)
    return 2.0 * effective_modulus(E[i], E[j], nu[i], nu[j]) * np.sqrt(effective_radius(r[i], r[j]) * d)


def body_force_torque(pairs, normal, f, n, arm_i=None, arm_j=None):
    """(F [n,3], T [n,3], sum |F| [n]) of the linker forces: -f n on body i at arm_i, +f n on body j at arm_j"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    Fc = f[:, None] * np.asarray(normal)
    F = np.zeros((n, 3))
    T = np.zeros((n, 3))
    scale = np.zeros(n)
    np.add.at(F, pairs[:, 0], -Fc)
    np.add.at(F, pairs[:, 1], Fc)
    mag = np.linalg.norm(Fc, axis=1)
    np.add.at(scale, pairs[:, 0], mag)
    np.add.at(scale, pairs[:, 1], mag)
    if arm_i is not None:
        np.add.at(T, pairs[:, 0], np.cross(arm_i, -Fc))
        np.add.at(T, pairs[:, 1], np.cross(arm_j, Fc))
    return F, T, scale


def rod_arms(pairs, s, t, seg):
    """the rod-compressed lever arms (s - 1/2)(p1 - p0) of the two closest points (centreline closest points)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    u = seg[:, 3:6] - seg[:, 0:3]
    return (s - 0.5)[:, None] * u[pairs[:, 0]], (t - 0.5)[:, None] * u[pairs[:, 1]]
