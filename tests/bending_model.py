"""numpy restatement of the semiflexible-chain force laws (include/mundy_hip_bending.h), written from the reference's
text: the FENE-WCA bond (FENEWCASpringsKernel.cpp:147-176) and the angular spring (AngularSpringsKernel.cpp:143-168), in
the operations, association and summation order the header documents.  The float expressions round like the device
code; the cosines of the rest angles are the handle's own (ops.AngularSprings.cos_rest), not recomputed here.

The potentials the laws are the gradients of, in mpmath (tests/potentials.py's conventions), are at the end."""
import math

import mpmath as mp
import numpy as np

import potentials as P

CLAMP = 1e-4   # the reference's hard-coded epsilon_reg


def wca_cutoff(sigma):
    """2^(1/6) sigma, as the library computes it once on the host (std::pow)"""
    return math.pow(2.0, 1.0 / 6.0) * sigma


def _dot(a, b):
    """the library's right fold"""
    return a[:, 0] * b[:, 0] + (a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2])


def fenewca_terms(pairs, k, r_max, center, epsilon=1.0, sigma=1.0):
    """per bond: (term [m, 3] that body i receives, L [m]); body j receives -term"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    m = p.shape[0]
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (m,))
    r = np.broadcast_to(np.asarray(r_max, dtype=np.float64), (m,))
    d = center[p[:, 1]] - center[p[:, 0]]
    L = np.sqrt(_dot(d, d))
    with np.errstate(divide="ignore", invalid="ignore"):
        rm = r - CLAMP
        La = np.where(rm < L, rm, L)   # std::min(L, rm)
        spring = k * La / (1.0 - (La / r) * (La / r))
        rho2 = sigma * sigma / (La * La)
        rho6 = rho2 * rho2 * rho2
        rho12 = rho6 * rho6
        lj = np.where(La < wca_cutoff(sigma), 6.0 * 4.0 * epsilon * (2.0 * rho12 - rho6) / La, 0.0)
        fm = (spring - lj) * (1.0 / L)
    return fm[:, None] * d, L


def fenewca_force(n, pairs, k, r_max, center, epsilon=1.0, sigma=1.0):
    """-> (force [n, 3], clamped, max_length): each body adds its terms in ascending bond index from +0.0; clamped = the
    bonds with !(L < r_max - 1e-4)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    term, L = fenewca_terms(p, k, r_max, center, epsilon, sigma)
    m = p.shape[0]
    f = np.zeros((n, 3))
    # bond by bond, +term at i and -term at j: every body meets its bonds in ascending index (np.add.at is unbuffered
    # and sequential)
    np.add.at(f, np.stack([p[:, 0], p[:, 1]], axis=1).reshape(-1), np.stack([term, -term], axis=1).reshape(-1, 3))
    r = np.broadcast_to(np.asarray(r_max, dtype=np.float64), (m,))
    over = int((~(L < r - CLAMP)).sum())
    mx = float(np.max(np.where(np.isnan(L), 0.0, L))) if m else 0.0
    return f, over, max(mx, 0.0)


def angular_rows(triplets, k, cos_rest, center):
    """per triplet (a, b, c): (F_a, F_b, F_c [m, 3], L1, L2 [m], |cos(theta) - cos_rest| [m])"""
    t = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
    m = t.shape[0]
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (m,))
    c0 = np.broadcast_to(np.asarray(cos_rest, dtype=np.float64), (m,))
    v1 = center[t[:, 0]] - center[t[:, 2]]
    v2 = center[t[:, 1]] - center[t[:, 2]]
    s1, s2 = _dot(v1, v1), _dot(v2, v2)
    L1, L2 = np.sqrt(s1), np.sqrt(s2)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = _dot(v1, v2) / (L1 * L2)
        tau = k * (c - c0)
        a11 = tau * c / s1
        a13 = -tau / (L1 * L2)
        a33 = tau * c / s2
        fa = a11[:, None] * v1 + a13[:, None] * v2
        fb = a33[:, None] * v2 + a13[:, None] * v1
        fc = -fa - fb
    return fa, fb, fc, L1, L2, np.abs(c - c0)


def angular_force(n, triplets, k, cos_rest, center, force=None):
    """-> (force [n, 3], degenerate, max_deviation): each body adds its rows in ascending triplet index from +0.0;
    force= an [n, 3] array: the accumulate form -- each body's sum is added to its row, a body on no triplet keeps its
    row as it is.  degenerate = the triplets with a zero arm; max_deviation ignores NaN"""
    t = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
    fa, fb, fc, L1, L2, dev = angular_rows(t, k, cos_rest, center)
    f = np.zeros((n, 3))
    np.add.at(f, t.reshape(-1), np.stack([fa, fb, fc], axis=1).reshape(-1, 3))
    if force is not None:
        on = np.zeros(n, bool)
        on[t.reshape(-1)] = True
        f = np.where(on[:, None], np.asarray(force) + f, np.asarray(force))
    deg = int(((L1 == 0.0) | (L2 == 0.0)).sum())
    mx = float(np.max(np.where(np.isnan(dev), 0.0, dev))) if t.shape[0] else 0.0
    return f, deg, mx


def angular_energy(triplets, k, cos_rest, center):
    """U = sum 1/2 k (cos(theta) - cos_rest)^2 in float64 (for trends, not for bits)"""
    t = np.asarray(triplets, dtype=np.int64).reshape(-1, 3)
    v1 = center[t[:, 0]] - center[t[:, 2]]
    v2 = center[t[:, 1]] - center[t[:, 2]]
    c = (v1 * v2).sum(axis=1) / np.sqrt((v1 * v1).sum(axis=1) * (v2 * v2).sum(axis=1))
    return float((0.5 * np.asarray(k) * (c - np.asarray(cos_rest)) ** 2).sum())


# ---- the potentials (mpmath; call inside `with P.hp():`) -----------------------------------------------------------------------
def fenewca_potential(L, k, r_max, epsilon, sigma):
    """U(L) = FENE + WCA for L below the clamp r_max - 1e-4 (the float64 difference, the number the law compares with);
    past it the straight line with the slope at the clamp: the clamped bond pulls with the constant force of
    L_adj = r_max - 1e-4"""
    rm = mp.mpf(float(np.float64(r_max) - CLAMP))
    k, r, e, s = (mp.mpf(float(v)) for v in (k, r_max, epsilon, sigma))
    cut = mp.mpf(float(wca_cutoff(float(sigma))))

    def u(x):
        return P.fene(x, k, r) + P.wca(x, e, s, cut)

    if L < rm:
        return u(L)
    rho6 = (s / rm) ** 6
    slope = k * rm / (1 - (rm / r) ** 2) - (24 * e * (2 * rho6 * rho6 - rho6) / rm if rm < cut else 0)
    return u(rm) + slope * (L - rm)


def fenewca_term(i, j, k, r_max, epsilon=1.0, sigma=1.0):
    return P.pair_term(i, j, lambda L: fenewca_potential(L, k, r_max, epsilon, sigma), "fenewca")


def angular_term(a, b, c, k, cos_rest):
    """U = 1/2 k (cos(theta) - cos_rest)^2 of the angle at c; cos_rest the float64 the handle stores, taken exactly"""
    k, c0 = mp.mpf(float(k)), mp.mpf(float(cos_rest))

    def energy(p):
        v1, v2 = P.sub(p[0], p[2]), P.sub(p[1], p[2])
        cs = P.dot(v1, v2) / (P.norm(v1) * P.norm(v2))
        return k * (cs - c0) ** 2 / 2

    return P.Term((a, b, c), energy, 1, "angular")
