"""The per-body contact force and torque of a contact operator (include/mundy_hip_contact_force.h) restated on the CPU:
the device's per-term expressions in numpy (the device is built with -ffp-contract=off), every per-body sum the
correctly rounded one (math.fsum), which is what a double-double pair rounded once gives while sum|terms| / |sum| stays
below 2^40.  Only the summation differs from the device, and its result does not depend on the order.

    scalar form  x [C] with normal [C, 3]:  f = -(x n) at the source body pairs[c, 0], +(x n) at the target pairs[c, 1]
    vector form  force [C, 3]:              f = +F at the source, -F at the target
    torque about the body centre: spheres +0.0; vector arms sum r x f (r = ra at the source, rb at the target);
    rods u x sum coef f with coef = clamp(arclength, 0, 1) - 1/2 and u = p1 - p0 of seg [N, 8]
    a contact with x == 0, or F == (0, 0, 0), is never added; accumulate: out = old + sum, one more rounding"""
import math

import numpy as np


def cross(a, b):
    """V3 cross of mhip_internal.hpp, component by component"""
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def exact(terms):
    """the correctly rounded sum (+0.0 for an empty or cancelling sum: the device's pair starts at +0.0)"""
    return math.fsum(terms) + 0.0


def body_force(N, pairs, *, x=None, normal=None, force=None, ra=None, rb=None, rod=None, stride=6, old=None,
               want_terms=False):
    """-> out [N, stride]; rod = (s, t, seg); old: the buffer accumulated onto (None: overwrite).  want_terms: also
    sum|f| per body [N, 3] (the conditioning of the force sums)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    if x is not None:
        x = np.asarray(x, dtype=np.float64)
        f = x[:, None] * np.asarray(normal, dtype=np.float64)
        live = np.flatnonzero(x != 0.0)
        sides = ((0, -f), (1, f))
    else:
        force = np.asarray(force, dtype=np.float64).reshape(-1, 3)
        live = np.flatnonzero((force != 0.0).any(axis=1))
        sides = ((0, force), (1, -force))
    tf = [[[] for _ in range(3)] for _ in range(N)]
    tt = [[[] for _ in range(3)] for _ in range(N)]
    for side, fs in sides:
        tq = None
        if rod is not None:
            coef = np.clip(rod[side], 0.0, 1.0) - 0.5
            tq = coef[:, None] * fs
        elif ra is not None:
            tq = cross(ra if side == 0 else rb, fs)
        for c in live:
            b = pairs[c, side]
            for k in range(3):
                tf[b][k].append(fs[c, k])
                if tq is not None:
                    tt[b][k].append(tq[c, k])
    F = np.array([[exact(tf[b][k]) for k in range(3)] for b in range(N)]).reshape(N, 3)
    T = np.array([[exact(tt[b][k]) for k in range(3)] for b in range(N)]).reshape(N, 3)
    if rod is not None:
        seg = rod[2]
        T = cross(seg[:, 3:6] - seg[:, 0:3], T)
    out = np.concatenate([F, T], axis=1)[:, :stride]
    if old is not None:
        out = np.asarray(old, dtype=np.float64) + out
    if want_terms:
        mag = np.array([[math.fsum(abs(v) for v in tf[b][k]) for k in range(3)] for b in range(N)]).reshape(N, 3)
        return out, mag
    return out
