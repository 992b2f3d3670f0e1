"""numpy restatement of the nucleus terms of the chain step (periphery.hip, active.hip), in the operations and order
include/mundy_hip.h documents: the wall force of a spherical or ellipsoidal periphery, the two-state (telegraph)
process of the active springs and their force dipoles.  The float expressions round like the device code; the exact
point - ellipsoid distance is a scalar translation of csrc/segment_ellipsoid.hpp (a test may pass another provider of
the distance and of the rotations, e.g. the oracle's, which restates the device's IEEE sequence)."""
import math

import numpy as np

import chain_model as cm


# ---- rotations (Quaternion.hpp: (q * (0, v)) * inverse(q), the oracle's association) ----------------------------------
def _qmul(q, o):
    return (q[0] * o[0] - q[1] * o[1] - q[2] * o[2] - q[3] * o[3],
            q[0] * o[1] + q[1] * o[0] + q[2] * o[3] - q[3] * o[2],
            q[0] * o[2] - q[1] * o[3] + q[2] * o[0] + q[3] * o[1],
            q[0] * o[3] + q[1] * o[2] - q[2] * o[1] + q[3] * o[0])


def quat_rotate(quat, v):
    """quat [4] (w, x, y, z) applied to v [n, 3]"""
    q = [np.float64(x) for x in quat]
    v = np.asarray(v, dtype=np.float64)
    inv = 1.0 / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qi = (q[0] * inv, -q[1] * inv, -q[2] * inv, -q[3] * inv)
    r = _qmul(_qmul(q, (np.zeros(len(v)), v[:, 0], v[:, 1], v[:, 2])), qi)
    return np.stack([r[1], r[2], r[3]], axis=1)


def conjugate(quat):
    return (quat[0], -quat[1], -quat[2], -quat[3])


# ---- exact signed point - ellipsoid distance (segment_ellipsoid.hpp, one point at a time) -----------------------------
_NEWTON_MAX, _TINY, _REL_TINY = 64, 1e-290, 1e-100


def _root3(r0, r1, m0, m1, z0, z1, z2):
    u = z2
    for _ in range(_NEWTON_MAX):
        d0, d1 = u + m0, u + m1
        q0, q1, q2 = r0 * z0 / d0, r1 * z1 / d1, z2 / u
        Q = q0 * q0 + q1 * q1 + q2 * q2
        if not Q > 1.0:
            break
        dg = q0 * q0 / d0 + q1 * q1 / d1 + q2 * q2 / u
        un = u + Q * (math.sqrt(Q) - 1.0) / dg
        if not un > u:
            break
        u = un
    return u


def _root2(r0, m0, z0, z1):
    u = z1
    for _ in range(_NEWTON_MAX):
        d0 = u + m0
        q0, q1 = r0 * z0 / d0, z1 / u
        Q = q0 * q0 + q1 * q1
        if not Q > 1.0:
            break
        dg = q0 * q0 / d0 + q1 * q1 / u
        un = u + Q * (math.sqrt(Q) - 1.0) / dg
        if not un > u:
            break
        u = un
    return u


def _ellipse2(e0, e1, y0, y1):
    """-> (distance, x0, x1): closest point of the ellipse with e0 >= e1 to (y0, y1) >= 0"""
    if y1 > 0.0:
        if y0 > 0.0:
            z0, z1 = y0 / e0, y1 / e1
            if z0 * z0 + z1 * z1 - 1.0 != 0.0:
                q = e0 / e1
                r0, m0 = q * q, (q - 1.0) * (q + 1.0)
                u = _root2(r0, m0, z0, z1)
                x0, x1 = r0 * y0 / (u + m0), y1 / u
                a, b = x0 - y0, x1 - y1
                return math.sqrt(a * a + b * b), x0, x1
            return 0.0, y0, y1
        return abs(y1 - e1), 0.0, e1
    numer0, denom0 = e0 * y0, e0 * e0 - e1 * e1
    if numer0 < denom0:
        xde0 = numer0 / denom0
        x0, x1 = e0 * xde0, e1 * math.sqrt(1.0 - xde0 * xde0)
        a = x0 - y0
        return math.sqrt(a * a + x1 * x1), x0, x1
    return abs(y0 - e0), e0, 0.0


def _ellipsoid3(e0, e1, e2, y0, y1, y2):
    """-> (distance, x0, x1, x2): closest point of the ellipsoid with e0 >= e1 >= e2 to y >= 0"""
    if y2 > 0.0:
        if y1 > 0.0:
            if y0 > 0.0:
                z0, z1, z2 = y0 / e0, y1 / e1, y2 / e2
                if z0 * z0 + z1 * z1 + z2 * z2 - 1.0 != 0.0:
                    q0, q1 = e0 / e2, e1 / e2
                    r0, r1 = q0 * q0, q1 * q1
                    m0, m1 = (q0 - 1.0) * (q0 + 1.0), (q1 - 1.0) * (q1 + 1.0)
                    u = _root3(r0, r1, m0, m1, z0, z1, z2)
                    x0, x1, x2 = r0 * y0 / (u + m0), r1 * y1 / (u + m1), y2 / u
                    a, b, c = x0 - y0, x1 - y1, x2 - y2
                    return math.sqrt(a * a + b * b + c * c), x0, x1, x2
                return 0.0, y0, y1, y2
            d, x1, x2 = _ellipse2(e1, e2, y1, y2)
            return d, 0.0, x1, x2
        if y0 > 0.0:
            d, x0, x2 = _ellipse2(e0, e2, y0, y2)
            return d, x0, 0.0, x2
        return abs(y2 - e2), 0.0, 0.0, e2
    denom0, denom1 = e0 * e0 - e2 * e2, e1 * e1 - e2 * e2
    numer0, numer1 = e0 * y0, e1 * y1
    if numer0 < denom0 and numer1 < denom1:
        xde0, xde1 = numer0 / denom0, numer1 / denom1
        discr = 1.0 - xde0 * xde0 - xde1 * xde1
        if discr > 0.0:
            x0, x1, x2 = e0 * xde0, e1 * xde1, e2 * math.sqrt(discr)
            a, b = x0 - y0, x1 - y1
            return math.sqrt(a * a + b * b + x2 * x2), x0, x1, x2
    d, x0, x1 = _ellipse2(e0, e1, y0, y1)
    return d, x0, x1, 0.0


def point_ellipsoid_body(y, e):
    """one point y [3] in the frame of the ellipsoid with semi-axes e [3] -> (signed distance (negative inside), closest
    surface point [3], outward unit normal there [3])"""
    y, e = [float(v) for v in y], [float(v) for v in e]
    sgn = [-1.0 if v < 0.0 else 1.0 for v in y]
    a = [s * v for s, v in zip(sgn, y)]
    floor = max(_REL_TINY * max(a), _TINY)
    a = [0.0 if v < floor else v for v in a]
    order = sorted(range(3), key=lambda k: -e[k])  # (stable: equal semi-axes keep their order, as the device's swaps)
    es, ys = [e[k] for k in order], [a[k] for k in order]
    res = _ellipsoid3(es[0], es[1], es[2], ys[0], ys[1], ys[2])
    dist, xs = res[0], res[1:]
    w = [ys[k] / es[k] for k in range(3)]
    inside = w[0] * w[0] + w[1] * w[1] + w[2] * w[2] < 1.0
    m = [xs[k] / (es[k] * es[k]) for k in range(3)]
    inv = 1.0 / math.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
    x, n = [0.0] * 3, [0.0] * 3
    for place, k in enumerate(order):
        x[k], n[k] = sgn[k] * xs[place], sgn[k] * (m[place] * inv)
    return (-dist if inside else dist), x, n


def exact_distance(points, pcenter, quat, radii, rotate=quat_rotate):
    """the periphery's exact route for lab points [n, 3] -> (sd [n], pn [n, 3]): signed distance to the ellipsoid
    (negative inside) and the wall's inward normal pn = -(q n) at the closest point"""
    y = rotate(conjugate(quat), np.asarray(points, dtype=np.float64) - np.asarray(pcenter, dtype=np.float64))
    sd, nb = np.empty(len(y)), np.empty((len(y), 3))
    for i in range(len(y)):
        sd[i], _, nb[i] = point_ellipsoid_body(y[i], radii)
    return sd, -rotate(quat, nb)


# ---- periphery forces -----------------------------------------------------------------------------------------------------
def _apply(force, hit, term, over, n):
    """hit beads: F - term (from 0.0 where force is None); the others untouched (+0.0 where force is None)"""
    f = np.zeros((n, 3)) if force is None else np.array(force, dtype=np.float64, copy=True)
    f[hit] = f[hit] - term[hit]
    mx = float(over[hit].max()) if hit.any() else 0.0
    return f, int(hit.sum()), mx


def sphere_force(center, radius, R, K, pcenter=(0.0, 0.0, 0.0), force=None):
    """HP1.cpp:4208-4238 -> (force [n, 3], colliding, max_overlap); force=None: written, else accumulated into a copy"""
    x = np.asarray(center, dtype=np.float64) - np.asarray(pcenter, dtype=np.float64)
    nrm = np.sqrt(x[:, 0] * x[:, 0] + (x[:, 1] * x[:, 1] + x[:, 2] * x[:, 2]))
    ssd = R - nrm - radius
    hit = ssd < 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inward = (-x) * (1.0 / nrm)[:, None]
        term = (K * inward) * ssd[:, None]
    return _apply(force, hit, term, -ssd, len(x))


def level_set(b, ia, ib, ic):
    return (b[:, 0] * b[:, 0] * ia + b[:, 1] * b[:, 1] * ib + b[:, 2] * b[:, 2] * ic) - 1.0


def ellipsoid_filter(center, radius, radii, pcenter, quat, rotate=quat_rotate):
    """the coarse filter of NgpHP1.cpp:2462-2500 -> mask of the beads whose eight box corners all lie inside"""
    c, r = np.asarray(center, dtype=np.float64), np.asarray(radius, dtype=np.float64)
    pc = np.asarray(pcenter, dtype=np.float64)
    ia, ib, ic = (1.0 / (np.float64(e) * np.float64(e)) for e in radii)
    inside = np.ones(len(c), dtype=bool)
    for k in range(8):
        corner = np.stack([c[:, 0] + r if k & 1 else c[:, 0] - r, c[:, 1] + r if k & 2 else c[:, 1] - r,
                           c[:, 2] + r if k & 4 else c[:, 2] - r], axis=1)
        inside &= level_set(rotate(conjugate(quat), corner - pc), ia, ib, ic) < 0.0
    return inside


def ellipsoid_force(center, radius, radii, K, pcenter=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), force=None,
                    distance=None, rotate=quat_rotate, use_filter=True):
    """NgpHP1.cpp:2444-2527 with the exact distance -> (force, colliding, max_overlap).  distance(points [k, 3]) ->
    (sd [k], pn [k, 3]) evaluates the beads that fail the filter (default: exact_distance of this module)"""
    c, r = np.asarray(center, dtype=np.float64), np.asarray(radius, dtype=np.float64)
    n = len(c)
    near = ~ellipsoid_filter(c, r, radii, pcenter, quat, rotate) if use_filter else np.ones(n, dtype=bool)
    if distance is None:
        distance = lambda pts: exact_distance(pts, pcenter, quat, radii, rotate)  # noqa: E731
    ssd, pn = np.zeros(n), np.zeros((n, 3))
    if near.any():
        sd, pn[near] = distance(c[near])
        ssd[near] = -sd - r[near]
    hit = near & (ssd < 0.0)
    term = (K * pn) * ssd[:, None]
    return _apply(force, hit, term, -ssd, n)


def ellipsoid_fast_force(center, radius, radii, K, pcenter=(0.0, 0.0, 0.0), force=None):
    """HP1.cpp:4148-4206 -> (force, colliding, largest level-set value)"""
    x = np.asarray(center, dtype=np.float64) - np.asarray(pcenter, dtype=np.float64)
    r = np.asarray(radius, dtype=np.float64)
    inv = [1.0 / ((np.float64(e) - r) * (np.float64(e) - r)) for e in radii]
    g = level_set(x, *inv)
    hit = g > 0.0
    term = np.stack([K * (2.0 * x[:, k] * inv[k]) for k in range(3)], axis=1)
    return _apply(force, hit, term, g, len(x))


def surface_points(rng, n, radii, lo, hi):
    """body-frame points at lo .. hi of the surface along random directions (uniform on the unit sphere, scaled by the
    semi-axes) -> [n, 3]"""
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d * np.asarray(radii, dtype=np.float64) * rng.uniform(lo, hi, n)[:, None]


# ---- active springs: a telegraph process per spring and its force dipole -------------------------------------------------
def uniform_open(keys, counters):
    """u = (((w0 << 21) | (w1 >> 11)) + 1) 2^-53 in (0, 1] from block 0 at (key, counter)"""
    w = cm.philox(keys, counters, 0).astype(np.uint64)
    m = (w[:, 0] << np.uint64(21)) | (w[:, 1] >> np.uint64(11))
    return (m + np.uint64(1)).astype(np.float64) * 2.0 ** -53


def active_init(keys, counters, kon):
    """HP1.cpp:2796-2826 -> dict(state, next_time, elapsed, counters)"""
    keys, counters = np.asarray(keys, dtype=np.uint64), np.asarray(counters, dtype=np.uint64)
    m = len(keys)
    return dict(state=np.zeros(m, np.int32), next_time=-np.log(uniform_open(keys, counters)) * (1.0 / kon),
                elapsed=np.zeros(m), counters=counters + np.uint64(1))


def active_sample(s, keys, kon, koff):
    """HP1.cpp:3798-3816 on a state dict -> (new dict, (switched on, switched off))"""
    keys = np.asarray(keys, dtype=np.uint64)
    fire = s["elapsed"] >= s["next_time"]
    u = uniform_open(keys, s["counters"])
    on, off = fire & (s["state"] == 0), fire & (s["state"] != 0)
    with np.errstate(divide="ignore"):
        nt = np.where(on, -np.log(u) * (1.0 / koff), np.where(off, -np.log(u) * (1.0 / kon), s["next_time"]))
    new = dict(state=np.where(on, 1, np.where(off, 0, s["state"])).astype(np.int32), next_time=nt,
               elapsed=np.where(fire, 0.0, s["elapsed"]), counters=s["counters"] + fire.astype(np.uint64))
    return new, (int(on.sum()), int(off.sum()))


def active_advance(s, dt):
    return dict(s, elapsed=s["elapsed"] + dt)


def active_force(n, pairs, state, sigma, center, force=None):
    """HP1.cpp:4325-4347 -> (force [n, 3], number of active springs): each body adds its terms in ascending spring index
    from +0.0 (body i: -t, body j: +t); force=None: written, else the sums are added into a copy (touched bodies only)"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)[np.asarray(state) == 1]
    m = p.shape[0]
    center = np.asarray(center, dtype=np.float64)
    nv = center[p[:, 1]] - center[p[:, 0]]
    nsqr = nv[:, 0] * nv[:, 0] + nv[:, 1] * nv[:, 1] + nv[:, 2] * nv[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        term = (sigma / np.sqrt(nsqr))[:, None] * nv
    body = np.concatenate([p[:, 0], p[:, 1]])
    sidx = np.concatenate([np.arange(m), np.arange(m)])
    plus = np.concatenate([np.zeros(m, bool), np.ones(m, bool)])
    order = np.lexsort((sidx, body))
    body, sidx, plus = body[order], sidx[order], plus[order]
    start = np.searchsorted(body, np.arange(n))
    rank = np.arange(body.shape[0]) - start[body]
    f = np.zeros((n, 3))
    for slot in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == slot
        t, b = term[sidx[sel]], body[sel]
        f[b] = np.where(plus[sel][:, None], f[b] + t, f[b] - t)
    if force is not None:
        out = np.array(force, dtype=np.float64, copy=True)
        touched = np.unique(body)
        out[touched] = out[touched] + f[touched]
        f = out
    return f, m
