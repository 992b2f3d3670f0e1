"""The small configurations of tests/test_potentials_host.py (calibration against the numpy models) and
tests/test_gpu_force_gradients.py (the device against -grad U): one Case per force term of the chain step, 16 to 64
bodies, coordinates O(1) shifted off the origin by SHIFT so that nothing cancels by symmetry.

A Case carries its inputs (x, `fixed`: what does not move with the bodies -- periphery sites, the wall's centre and
orientation), the energy terms of tests/potentials.py over them, the existing float64 numpy model of the term
(calibration only) and the call of the device entry point.  check() asserts the conditions the inputs were built to
meet: every member at least MARGIN from a branch boundary, members on both sides of it.

moved(case, quat, shift) is the same configuration rotated and translated in float64 -- what the device is given -- and
its exact pre-image in mpmath, x = Q^T (x' - t), fixed objects included: the energies are evaluated there, in the
original frame, and the device's forces at x' must be Q times those."""
import math

import mpmath as mp
import numpy as np

import potentials as P

SHIFT = np.array([0.75, -1.5, 2.25])
MARGIN = 1e-3
EPS = 2.0 ** -52


def M(v):
    return mp.mpf(float(v))


# ---- frames -----------------------------------------------------------------------------------------------------------------------
def quat_mul(p, q):
    return np.array([p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3],
                     p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
                     p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1],
                     p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]])


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


IDENTITY = np.array([1.0, 0.0, 0.0, 0.0])


def fixed_mp(fixed):
    """the fixed objects of the original frame as mpmath values"""
    out = {}
    if "sites" in fixed:
        out["sites"] = [P.vec(s) for s in fixed["sites"]]
    if "center" in fixed:
        out["center"] = P.vec(fixed["center"])
    if "quat" in fixed:
        out["rot"] = P.rotation(fixed["quat"])
    return out


def moved(case, quat, shift):
    """-> (x' [n, 3], fixed' (float64: the device's inputs), y: the exact pre-images of x' as mpf triples, fixed_y: the
    pre-images of fixed', Q: the rotation as 3 lists of mpf).  Call inside `with P.hp():`."""
    R = np.asarray(P.ld_rotation(quat), dtype=np.float64)
    shift = np.asarray(shift, dtype=np.float64)
    x2 = np.ascontiguousarray(case.x @ R.T + shift)
    f2 = {}
    if "sites" in case.fixed:
        f2["sites"] = np.ascontiguousarray(case.fixed["sites"] @ R.T + shift)
    if "center" in case.fixed:
        f2["center"] = R @ case.fixed["center"] + shift
    if "quat" in case.fixed:
        q = quat_mul(quat, case.fixed["quat"])
        f2["quat"] = q / np.linalg.norm(q)
    Q, t = P.rotation(quat), P.vec(shift)
    back = lambda p: P.apply(Q, P.sub(P.vec(p), t), transpose=True)  # noqa: E731
    y = [back(p) for p in x2]
    fy = {}
    if "sites" in f2:
        fy["sites"] = [back(s) for s in f2["sites"]]
    if "center" in f2:
        fy["center"] = back(f2["center"])
    if "quat" in f2:
        Rq = P.rotation(f2["quat"])
        fy["rot"] = [[sum(Q[k][i] * Rq[k][j] for k in range(3)) for j in range(3)] for i in range(3)]   # Q^T R(q')
    return x2, f2, y, fy, Q


class Case:
    pair_terms = False      # the momentum and angular-momentum invariants hold
    rotates = True          # False: the term has no orientation to rotate (the fast ellipsoid wall): translate only
    rows = "bodies"         # "linkers": the device returns one force per linker (the force on its first body)
    group = ""              # the row of the K table the case belongs to

    def __init__(self, name):
        self.name, self.fixed = name, {}

    def terms(self, fixed):
        raise NotImplementedError

    def model(self):
        raise NotImplementedError

    def device(self, ops, dev, host, x, fixed):
        raise NotImplementedError

    def check(self):
        pass

    def lever_positions(self, x):
        """positions whose cross product with the rows gives the angular momentum (rows == "bodies": x itself)"""
        return x

    def exact(self, x=None, fixed=None):
        """-> (F [rows, 3] float64 of the mpmath gradient, S [rows] float64, Fmp, Smp); the original frame by default.
        Call inside `with P.hp():`."""
        x = self.x if x is None else x
        fixed = fixed_mp(self.fixed) if fixed is None else fixed
        F, S, per = P.exact_forces(self.terms(fixed), x, n=self.n)
        if self.rows == "linkers":
            F, S = [g[0] for _, g in per], [m for m, _ in per]
        return F, S


def box_points(rng, n, edge):
    return rng.uniform(0.0, edge, (n, 3)) + SHIFT


def lengths(x, pairs):
    d = x[pairs[:, 1]] - x[pairs[:, 0]]
    return np.sqrt((d * d).sum(axis=1))


def random_pairs(rng, n, m):
    """a chain through all bodies, then random further pairs, no pair twice and no self pair"""
    seen, out = set(), []
    for i in range(n - 1):
        seen.add((i, i + 1))
        out.append((i, i + 1))
    while len(out) < m:
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if i != j and (min(i, j), max(i, j)) not in seen:
            seen.add((min(i, j), max(i, j)))
            out.append((i, j))
    return np.array(out, dtype=np.int32)


# ---- springs ------------------------------------------------------------------------------------------------------------------------
class SpringCase(Case):
    pair_terms = True
    group = "springs"

    def __init__(self, kind):
        super().__init__("springs_" + kind)
        rng = np.random.default_rng(101 if kind == "hookean" else 102)
        self.kind, self.n = kind, 24
        self.x = box_points(rng, self.n, 2.0)
        self.pairs = random_pairs(rng, self.n, 40)
        L = lengths(self.x, self.pairs)
        self.k = rng.uniform(1.0, 5.0, 40)
        # Hookean: rest lengths on both sides of L (stretched and compressed); FENE: r_max beyond every L
        self.r = L * (rng.uniform(0.5, 1.5, 40) if kind == "hookean" else rng.uniform(1.05, 2.0, 40))

    def check(self):
        L = lengths(self.x, self.pairs)
        if self.kind == "hookean":
            assert (np.abs(L - self.r) >= MARGIN).all() and (L > self.r).any() and (L < self.r).any()
        else:
            assert (L <= self.r - MARGIN).all()   # (past r_max the law has no value: there is no second side)

    def terms(self, fixed):
        law = P.hookean if self.kind == "hookean" else P.fene
        return [P.pair_term(i, j, (lambda L, k=M(k), r=M(r): law(L, k, r))) for (i, j), k, r in
                zip(self.pairs, self.k, self.r)]

    def model(self):
        import chain_model as cm
        return cm.spring_force(self.n, self.pairs, self.kind, self.k, self.r, self.x)[0]

    def device(self, ops, dev, host, x, fixed):
        sp = ops.Springs(self.n, self.pairs, self.kind, self.k, self.r)
        f = host(sp.force(dev(x))[0]).copy()
        sp.close()
        return f


# ---- crosslinkers -------------------------------------------------------------------------------------------------------------------
class CrosslinkerCase(Case):
    group = "crosslinkers"

    def __init__(self, kind, with_sites):
        super().__init__("crosslinkers_%s%s" % (kind, "_sites" if with_sites else ""))
        rng = np.random.default_rng({"hookean": 111, "fene": 112}[kind] + (10 if with_sites else 0))
        self.kind, self.n, self.m, self.with_sites = kind, 24, 40, with_sites
        self.pair_terms = not with_sites
        self.x = box_points(rng, self.n, 2.0)
        # bodies 20 .. 23 hold singly bound crosslinkers only: their rows must stay +0.0
        self.left = rng.integers(0, 20, self.m)
        self.left[:4] = np.arange(20, 24)
        self.right = self.left.copy()
        # after the first four: a third singly bound, a third bound to a bead, a third to a bead or (with sites) a site
        u = np.concatenate([np.zeros(4), (np.arange(self.m - 4) % 3) * 0.35])
        for c in np.flatnonzero(u > 0.3):
            j = int(rng.integers(0, 20))
            while j == self.left[c]:
                j = int(rng.integers(0, 20))
            self.right[c] = j
        if with_sites:
            self.fixed["sites"] = box_points(rng, 6, 2.0)
            tied = np.flatnonzero(u > 0.65)
            self.right[tied] = -(rng.integers(0, 6, tied.size) + 1)
        self.k = 3.5
        L = self._lengths()
        self.r = 0.8 if kind == "hookean" else float(1.2 * L.max())

    def _far(self, x, sites):
        bound = self.right != self.left
        pts = x if sites is None else np.concatenate([x, sites])
        far = np.where(self.right < 0, self.n - (self.right + 1), self.right)
        return bound, pts, far

    def _lengths(self):
        bound, pts, far = self._far(self.x, self.fixed.get("sites"))
        d = pts[far[bound]] - self.x[self.left[bound]]
        return np.sqrt((d * d).sum(axis=1))

    def check(self):
        L = self._lengths()
        bound = self.right != self.left
        assert bound.sum() >= 20 and (~bound).sum() >= 8 and (self.right[bound] >= 0).sum() >= 8
        if self.with_sites:
            assert (self.right < 0).sum() >= 8
        if self.kind == "hookean":
            assert (np.abs(L - self.r) >= MARGIN).all() and (L > self.r).any() and (L < self.r).any()
        else:
            assert (L <= self.r - MARGIN).all()
        touched = np.unique(np.concatenate([self.left[bound], self.right[bound & (self.right >= 0)]]))
        assert not np.isin(self.zero_rows(), touched).any()

    def zero_rows(self):
        return np.arange(20, 24)

    def terms(self, fixed):
        law = P.hookean if self.kind == "hookean" else P.fene
        k, r = M(self.k), M(self.r)
        f = lambda L: law(L, k, r)  # noqa: E731
        out = []
        for le, ri in zip(self.left, self.right):
            if ri == le:
                continue
            out.append(P.pair_term(le, ri, f) if ri >= 0 else P.tether_term(le, fixed["sites"][-(ri + 1)], f))
        return out

    def model(self):
        import periphery_binding_model as pm
        sites = self.fixed.get("sites", np.zeros((0, 3)))
        return pm.crosslinker_force(self.n, self.left, self.right, self.kind, self.k, self.r, self.x, sites)[0]

    def device(self, ops, dev, host, x, fixed):
        import torch
        start = np.where(self.right < 0, self.left, self.right)
        xl = ops.Crosslinkers(self.n, self.left, start, np.ones(self.n, np.uint8), self.kind, self.k, self.r, 1.0, 1.0,
                              1.0, 1.0)
        if self.with_sites:
            xl.set_periphery_sites(dev(fixed["sites"]), 1.0, 1.0, 2.0, None, 1.0)
        xl.set_state(None, dev(self.right.astype(np.int32)))
        f = host(xl.force(dev(x))[0]).copy()
        xl.close()
        del torch
        return f


# ---- active dipoles -------------------------------------------------------------------------------------------------------------------
class ActiveCase(Case):
    pair_terms = True
    group = "active"

    def __init__(self):
        super().__init__("active")
        rng = np.random.default_rng(121)
        self.n, self.sigma = 24, 2.5
        self.x = box_points(rng, self.n, 2.0)
        self.pairs = random_pairs(rng, 20, 30)
        # bodies 20 .. 23: springs that are off only
        self.pairs = np.concatenate([self.pairs, np.array([[20, 21], [22, 23], [21, 22]], np.int32)])
        self.state = (rng.random(len(self.pairs)) < 0.5).astype(np.int32)
        self.state[-3:] = 0

    def zero_rows(self):
        return np.arange(20, 24)

    def check(self):
        assert 8 <= self.state.sum() <= len(self.state) - 8 and (lengths(self.x, self.pairs) >= 0.1).all()

    def terms(self, fixed):
        s = M(self.sigma)
        return [P.pair_term(i, j, lambda L: P.active(L, s)) for (i, j), on in zip(self.pairs, self.state) if on]

    def model(self):
        import periphery_model as pm
        return pm.active_force(self.n, self.pairs, self.state, self.sigma, self.x)[0]

    def device(self, ops, dev, host, x, fixed):
        a = ops.ActiveSprings(self.n, self.pairs, self.sigma, 1.0, 1.0)
        a.set_state(state=dev(self.state))
        f = host(a.force(dev(x))[0]).copy()
        a.close()
        return f


# ---- the walls ------------------------------------------------------------------------------------------------------------------------
def _unit(rng, n):
    d = rng.normal(size=(n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _overlaps(rng, n, lo=0.02, hi=0.25):
    """overlaps delta on both sides of 0, at least MARGIN away: half colliding, half not"""
    d = rng.uniform(lo, hi, n)
    d[1::2] *= -1.0
    return d


class SphereWallCase(Case):
    group = "sphere wall"

    def __init__(self):
        super().__init__("wall_sphere")
        rng = np.random.default_rng(131)
        self.n, self.R, self.K = 32, 2.0, 50.0
        self.fixed["center"] = SHIFT + np.array([0.1, -0.2, 0.05])
        self.radius = rng.uniform(0.1, 0.3, self.n)
        self.x = self.fixed["center"] + _unit(rng, self.n) * (self.R - self.radius + _overlaps(rng, self.n))[:, None]

    def delta(self):
        return np.linalg.norm(self.x - self.fixed["center"], axis=1) + self.radius - self.R

    def zero_rows(self):
        return np.flatnonzero(self.delta() < 0)

    def check(self):
        d = self.delta()
        assert (np.abs(d) >= MARGIN).all() and (d > 0).sum() >= 8 and (d < 0).sum() >= 8

    def terms(self, fixed):
        R, K = M(self.R), M(self.K)
        return [P.Term((b,), (lambda p, r=M(r): P.sphere_wall(p[0], fixed["center"], r, R, K))) for b, r in
                enumerate(self.radius)]

    def spec(self, fixed):
        return dict(shape="sphere", radius=self.R, k=self.K, center=fixed["center"])

    def model(self):
        import periphery_model as pm
        return pm.sphere_force(self.x, self.radius, self.R, self.K, self.fixed["center"])[0]

    def device(self, ops, dev, host, x, fixed):
        return host(ops.periphery_force(self.spec(fixed), dev(x), dev(self.radius))[0]).copy()


class EllipsoidWallCase(Case):
    group = "ellipsoid wall"

    def __init__(self, name, radii, quat=None, seed=141):
        super().__init__("wall_ellipsoid_" + name)
        rng = np.random.default_rng(seed)
        self.n, self.K, self.radii = 32, 50.0, np.asarray(radii, dtype=np.float64)
        self.fixed["center"] = SHIFT + np.array([0.1, -0.2, 0.05])
        self.fixed["quat"] = IDENTITY if quat is None else np.asarray(quat, dtype=np.float64) / np.linalg.norm(quat)
        e = self.radii
        u = _unit(rng, self.n)
        # the first eight on principal planes and axes: one or two body-frame coordinates exactly zero
        zero = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (2,), (0,)]
        for b, z in enumerate(zero):
            u[b, list(z)] = 0.0
            u[b] /= np.linalg.norm(u[b])
        self.exact_zero = len(zero) if quat is None else 0
        surf = u * e   # a point of the surface and its outward normal
        nrm = surf / (e * e)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        # the overlap delta on both sides of 0 and the bead radius set the signed distance s = delta - r: within
        # 0.2 min(e) of the wall, inside; every fifth bead lies outside the wall instead (and so collides)
        self.radius = rng.uniform(0.05, 0.15, self.n)
        s = _overlaps(rng, self.n, 0.02, 0.05) - self.radius
        s[::5] = rng.uniform(0.01, 0.05, self.n)[::5]
        body = surf + nrm * s[:, None]
        Rm = np.asarray(P.ld_rotation(self.fixed["quat"]), dtype=np.float64)
        self.x = np.ascontiguousarray(body @ Rm.T + self.fixed["center"])

    def delta(self):
        body = (P._ld(self.x) - P._ld(self.fixed["center"])) @ P.ld_rotation(self.fixed["quat"])
        return np.asarray(self.radius + P.ld_point_ellipsoid(body, self.radii), dtype=np.float64)

    def zero_rows(self):
        return np.flatnonzero(self.delta() < 0)

    def check(self):
        d = self.delta()
        sd = d - self.radius
        assert (np.abs(d) >= MARGIN).all() and (d > 0).sum() >= 8 and (d < 0).sum() >= 8
        assert (np.abs(sd) <= 0.3 * self.radii.min()).all()
        if self.exact_zero:
            body = self.x - self.fixed["center"]
            nz = (body[:self.exact_zero] == 0.0).sum(axis=1)
            assert ((nz == 1) | (nz == 2)).all() and (nz == 2).sum() >= 2 and self.exact_zero >= 4
            assert (d[:self.exact_zero] > 0).sum() >= 3   # (colliding beads among them: the branch reaches the force)

    def terms(self, fixed):
        e, K = [M(v) for v in self.radii], M(self.K)
        return [P.Term((b,), (lambda p, r=M(r): P.ellipsoid_wall(p[0], fixed["center"], fixed["rot"], e, r, K)))
                for b, r in enumerate(self.radius)]

    def spec(self, fixed):
        return dict(shape="ellipsoid", radii=self.radii, k=self.K, center=fixed["center"], quat=fixed["quat"])

    def model(self):
        import periphery_model as pm
        return pm.ellipsoid_force(self.x, self.radius, self.radii, self.K, self.fixed["center"],
                                  tuple(self.fixed["quat"]))[0]

    def device(self, ops, dev, host, x, fixed):
        return host(ops.periphery_force(self.spec(fixed), dev(x), dev(self.radius))[0]).copy()


class FastWallCase(Case):
    group = "ellipsoid wall, fast"
    rotates = False

    def __init__(self):
        super().__init__("wall_ellipsoid_fast")
        rng = np.random.default_rng(151)
        self.n, self.K, self.radii = 32, 50.0, np.array([3.0, 2.0, 1.0])
        self.fixed["center"] = SHIFT + np.array([0.1, -0.2, 0.05])
        self.radius = rng.uniform(0.1, 0.3, self.n)
        g = _overlaps(rng, self.n, 0.01, 0.3)
        self.x = self.fixed["center"] + _unit(rng, self.n) * (self.radii - self.radius[:, None]) * np.sqrt(1.0 + g)[:, None]

    def g(self):
        return (((self.x - self.fixed["center"]) / (self.radii - self.radius[:, None])) ** 2).sum(axis=1) - 1.0

    def zero_rows(self):
        return np.flatnonzero(self.g() < 0)

    def check(self):
        g = self.g()
        assert (np.abs(g) >= MARGIN).all() and (g > 0).sum() >= 8 and (g < 0).sum() >= 8

    def terms(self, fixed):
        e, K = [M(v) for v in self.radii], M(self.K)
        return [P.Term((b,), (lambda p, r=M(r): P.ellipsoid_wall_fast(p[0], fixed["center"], e, r, K)))
                for b, r in enumerate(self.radius)]

    def model(self):
        import periphery_model as pm
        return pm.ellipsoid_fast_force(self.x, self.radius, self.radii, self.K, self.fixed["center"])[0]

    def device(self, ops, dev, host, x, fixed):
        spec = dict(shape="ellipsoid_fast", radii=self.radii, k=self.K, center=fixed["center"])
        return host(ops.periphery_force(spec, dev(x), dev(self.radius))[0]).copy()


# ---- sphere - sphere Hertz ------------------------------------------------------------------------------------------------------------
class SphereHertzCase(Case):
    pair_terms = True
    rows = "linkers"
    group = "sphere Hertz"

    def __init__(self):
        super().__init__("hertz_spheres")
        rng = np.random.default_rng(161)
        self.n = 32
        self.radius = rng.uniform(0.3, 0.6, self.n)
        self.E = rng.uniform(500.0, 1500.0, self.n)
        self.nu = rng.uniform(0.2, 0.4, self.n)
        self.x = box_points(rng, self.n, 3.0)
        i, j = np.triu_indices(self.n, 1)
        sep = np.linalg.norm(self.x[j] - self.x[i], axis=1) - (self.radius[i] + self.radius[j])
        keep = (sep < 0.3) & (np.abs(sep) >= MARGIN)
        self.pairs = np.stack([i[keep], j[keep]], axis=1).astype(np.int32)
        self.pairs[1::2] = self.pairs[1::2, ::-1].copy()   # the first body is not always the lower index

    def sep(self):
        p = self.pairs
        return lengths(self.x, p) - (self.radius[p[:, 0]] + self.radius[p[:, 1]])

    def zero_rows(self):
        return np.flatnonzero(self.sep() > 0)

    def check(self):
        s = self.sep()
        assert (np.abs(s) >= MARGIN).all() and (s < 0).sum() >= 16 and (s > 0).sum() >= 8 and len(s) <= 160

    def terms(self, fixed):
        out = []
        for i, j in self.pairs:
            Es = P.effective_modulus(M(self.E[i]), M(self.nu[i]), M(self.E[j]), M(self.nu[j]))
            Rs = P.effective_radius(M(self.radius[i]), M(self.radius[j]))
            rr = M(self.radius[i]) + M(self.radius[j])
            out.append(P.pair_term(i, j, (lambda L, Es=Es, Rs=Rs, rr=rr: P.hertz(rr - L, Es, Rs))))
        return out

    def lever_positions(self, x):
        return x[self.pairs[:, 0]] - x[self.pairs[:, 1]]   # F_i at x_i and -F_i at x_j

    def model(self):
        import hertz_model as hm
        import oracle
        oracle.build()
        sep, nrm = oracle.contact_spheres(self.pairs, self.x, self.radius)
        f, _ = hm.hertz_force(self.pairs, sep, self.radius, self.E, self.nu)
        return -f[:, None] * nrm

    def device(self, ops, dev, host, x, fixed):
        p, r = dev(self.pairs), dev(self.radius)
        sep, nrm = ops.contact_spheres(p, dev(x), r)
        f, _ = ops.hertz_contact_force(p, sep, r, dev(self.E), dev(self.nu))
        return 0.0 - host(f)[:, None] * host(nrm)   # (0.0 - x: a linker out of the branch gives +0.0, not -0.0)


# ---- backbone segments -------------------------------------------------------------------------------------------------------------------
WCA = dict(epsilon=1.0, sigma=1.0, cutoff=1.12246204831)
SEG_E, SEG_NU, SEG_SKIN = 1000.0, 0.3, 0.3
MIN_SIN, MIN_DIST, BOX = 0.2, 0.3, 3.2


def _seg_dist(x, ends, i, j):
    """float64 (dist, |sin|, number of closest points that are end nodes) of the segment pairs (i, j), by
    tests/potentials.py's longdouble enumeration"""
    a0, a1, b0, b1 = x[ends[i, 0]], x[ends[i, 1]], x[ends[j, 0]], x[ends[j, 1]]
    d, s, t = P.ld_segment_segment(a0, a1, b0, b1, want_parameters=True)
    u, v = a1 - a0, b1 - b0
    sin = np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v, axis=1))
    cls = ((s == 0) | (s == 1)).astype(int) + ((t == 0) | (t == 1)).astype(int)
    return np.asarray(d, dtype=np.float64), sin, cls


def _unshared_pairs(ends):
    i, j = np.triu_indices(len(ends), 1)
    share = (ends[i, 0] == ends[j, 0]) | (ends[i, 0] == ends[j, 1]) | (ends[i, 1] == ends[j, 0]) | (ends[i, 1] == ends[j, 1])
    return i[~share], j[~share]


def grow_segments(seed, kind, branch=True):
    """chains grown bead by bead in a box: a new segment is kept only if, against every earlier segment that shares no
    node with it, it stays min_dist apart (Hertz: MIN_DIST; WCA: 0.8 sigma) and MIN_SIN from parallel whenever it is
    within reach, and 2 MARGIN from the law's branch boundary.  Step lengths 0.85 .. 1.25 (on both sides of the WCA
    cutoff and of 2 r), per-segment radii 0.4 .. 0.55.  Five chains of four segments; a sixth of two starts from an
    inner node of the first (a node with three segments); then twelve single segments, each laid across an existing
    one so that both closest points are interior (second neighbours along a chain supply the end - end pairs).
    branch=False leaves the sixth chain out: every chain is then a run of consecutive nodes (a filament).
    -> (grown, x [n, 3], ends int32 [m, 2], radius [m])"""
    rng = np.random.default_rng(seed)
    x, ends, radius = [], [], []
    min_dist = MIN_DIST if kind == "hertz" else 0.8 * WCA["sigma"]

    def boundary(r_old, r_new):
        return (r_old + r_new) if kind == "hertz" else WCA["cutoff"]

    def ok(p, q, shared, r_new):
        if not ends:
            return True
        e = np.array(ends)
        keep = ~np.isin(e, list(shared)).any(axis=1)
        if not keep.any():
            return True
        e, r = e[keep], np.array(radius)[keep]
        X = np.array(x)
        a0, a1 = X[e[:, 0]], X[e[:, 1]]
        d = np.asarray(P.ld_segment_segment(a0, a1, np.broadcast_to(p, a0.shape), np.broadcast_to(q, a0.shape)),
                       dtype=np.float64)
        u, v = a1 - a0, q - p
        sin = np.linalg.norm(np.cross(u, v), axis=1) / (np.linalg.norm(u, axis=1) * np.linalg.norm(v))
        near = d < boundary(r, r_new) + 0.05
        return bool(((d[near] >= min_dist) & (sin[near] >= MIN_SIN)).all() and
                    (np.abs(d - boundary(r, r_new)) >= 2 * MARGIN).all())

    max_dot = 0.0 if kind == "hertz" else -0.45   # no folding back onto a segment of the same node
    slack = 0.3 if kind == "hertz" else 2.0        # (the straighter WCA chains need room past the box of the starts)

    def outgoing(node):
        return [(x[b if a == node else a] - x[node]) / np.linalg.norm(x[b] - x[a]) for a, b in ends if node in (a, b)]

    def add(p_index, q, r_new):
        x.append(q)
        ends.append((p_index, len(x) - 1))
        radius.append(r_new)

    def chain(start_index, beads, dot_limit):
        if start_index is None:
            x.append(rng.uniform(0.0, BOX, 3) + SHIFT)
            last = len(x) - 1
        else:
            last = start_index
        made = 0
        for _ in range(1500):
            if made == beads:
                break
            w = _unit(rng, 1)[0]
            step = w * rng.uniform(0.85, 1.25)
            q, r_new = x[last] + step, rng.uniform(0.4, 0.55)
            if np.any(q < SHIFT - slack) or np.any(q > SHIFT + BOX + slack) or any(w @ o > dot_limit for o in outgoing(last)):
                continue
            if abs(np.linalg.norm(step) - boundary(r_new, r_new)) < 2 * MARGIN:
                continue
            if ok(x[last], q, {last}, r_new):
                add(last, q, r_new)
                last = len(x) - 1
                made += 1
        return made == beads

    def crossing():
        """one more segment, of two new bodies, that crosses an existing one: both closest points interior"""
        lo, hi = (0.35, 0.75) if kind == "hertz" else (0.82, 1.08)
        for _ in range(300):
            a, b = ends[int(rng.integers(0, len(ends)))]
            u = (x[b] - x[a]) / np.linalg.norm(x[b] - x[a])
            p = x[a] + rng.uniform(0.25, 0.75) * (x[b] - x[a])
            n = np.cross(u, _unit(rng, 1)[0])
            if np.linalg.norm(n) < 0.3:
                continue
            n /= np.linalg.norm(n)
            ang = rng.uniform(0.6, np.pi - 0.6)
            w = np.cos(ang) * u + np.sin(ang) * np.cross(n, u)   # perpendicular to n, well away from parallel to u
            c, L, t, r_new = p + n * rng.uniform(lo, hi), rng.uniform(0.85, 1.25), rng.uniform(0.25, 0.75), rng.uniform(0.4, 0.55)
            p0, p1 = c - t * L * w, c + (1.0 - t) * L * w
            if abs(L - boundary(r_new, r_new)) < 2 * MARGIN or not ok(p0, p1, set(), r_new):
                continue
            x.append(p0)
            add(len(x) - 1, p1, r_new)
            return True
        return False

    good = all(chain(None, 4, max_dot) for _ in range(5)) and (not branch or chain(2, 2, 0.2))
    good = good and all(crossing() for _ in range(12))
    return good, np.array(x), np.array(ends, dtype=np.int32), np.array(radius)


class SegmentCase(Case):
    pair_terms = True

    def __init__(self, kind, correction):
        super().__init__("segments_%s%s" % (kind, "_end_correction" if correction else ""))
        self.kind, self.correction = kind, correction
        self.group = "segment " + ("Hertz" if kind == "hertz" else "WCA")
        good, self.x, self.ends, self.radius = grow_segments(segment_seed(kind), kind)
        assert good
        self.n, self.m = self.x.shape[0], self.ends.shape[0]
        deg = np.bincount(self.ends.reshape(-1), minlength=self.n)
        self.corr = (deg[self.ends] == 1).any(axis=1) if correction else np.zeros(self.m, bool)
        i, j = _unshared_pairs(self.ends)
        d, sin, cls = _seg_dist(self.x, self.ends, i, j)
        near = d < self.boundary(i, j) + 0.3
        self.pi, self.pj, self.d, self.sin, self.cls = i[near], j[near], d[near], sin[near], cls[near]

    def boundary(self, i, j):
        return (self.radius[i] + self.radius[j]) if self.kind == "hertz" else np.full(len(i), WCA["cutoff"])

    def in_branch(self):
        return self.d < self.boundary(self.pi, self.pj)

    def check(self):
        deg = np.bincount(self.ends.reshape(-1), minlength=self.n)
        assert 16 <= self.n <= 64 and deg.max() == 3 and np.ptp(self.radius) > 0.1
        inb = self.in_branch()
        assert (np.abs(self.d - self.boundary(self.pi, self.pj)) >= MARGIN).all() and inb.sum() >= 12 and (~inb).sum() >= 4
        assert (self.sin[inb] >= MIN_SIN).all() and (self.d[inb] >= MIN_DIST).all()
        if self.kind == "wca":
            assert (self.d[inb] >= 0.8 * WCA["sigma"]).all()
        cls = self.cls[inb]
        assert (cls == 0).sum() * 3 >= len(cls) and (cls == 2).sum() * 5 >= len(cls) and (cls == 1).any(), \
            np.bincount(cls, minlength=3)
        if self.correction:
            L = lengths(self.x, self.ends)[self.corr]
            b = 2.0 * self.radius[self.corr] if self.kind == "hertz" else WCA["cutoff"]
            assert (np.abs(L - b) >= MARGIN).all() and (L < b).sum() >= 3 and (L > b).sum() >= 2 and (L >= 0.8).all()

    def _law(self, ri, rj):
        if self.kind == "hertz":
            Es = P.effective_modulus(M(SEG_E), M(SEG_NU), M(SEG_E), M(SEG_NU))
            Rs, rr = P.effective_radius(M(ri), M(rj)), M(ri) + M(rj)
            return lambda d: P.hertz(rr - d, Es, Rs)
        eps, sig, cut = M(WCA["epsilon"]), M(WCA["sigma"]), M(WCA["cutoff"])
        return lambda d: P.wca(d, eps, sig, cut)

    def terms(self, fixed):
        out = [P.segment_pair_term(self.ends[i], self.ends[j], self._law(self.radius[i], self.radius[j]))
               for i, j in zip(self.pi, self.pj)]
        for s in np.flatnonzero(self.corr):
            out.append(P.pair_term(self.ends[s, 0], self.ends[s, 1], self._law(self.radius[s], self.radius[s])))
        return out

    def model(self):
        import segment_contact_model as scm
        mod = scm.SegmentContacts(self.n, self.ends, self.kind, self.radius, SEG_SKIN,
                                  end_correction=None if self.correction else False, youngs_modulus=SEG_E,
                                  poisson_ratio=SEG_NU, **WCA)
        mod.update(self.x)
        return mod.force_pass(self.x)[0]

    def device(self, ops, dev, host, x, fixed):
        sc = ops.SegmentContacts(self.n, kind=self.kind, radius=self.radius, skin=SEG_SKIN, segments=self.ends,
                                 end_correction=None if self.correction else False, youngs_modulus=SEG_E,
                                 poisson_ratio=SEG_NU, **WCA)
        xd = dev(x)
        sc.update(xd)
        f = host(sc.force(xd)[0]).copy()
        self.last_rows = (host(sc.field("pairs")).copy(), host(sc.field("sep")).copy(), host(sc.field("force")).copy())
        sc.close()
        return f


# the first seeds from 200 on whose configuration grows to the end and meets SegmentCase.check
SEGMENT_SEEDS = {"hertz": 203, "wca": 207}


def segment_seed(kind):
    return SEGMENT_SEEDS[kind]


# ---- the list ----------------------------------------------------------------------------------------------------------------------------
def _build():
    q = np.array([0.4, -0.3, 0.6, 0.5])
    cases = [SpringCase("hookean"), SpringCase("fene"),
             CrosslinkerCase("hookean", False), CrosslinkerCase("fene", False),
             CrosslinkerCase("hookean", True), CrosslinkerCase("fene", True),
             ActiveCase(), SphereWallCase(),
             EllipsoidWallCase("321", (3.0, 2.0, 1.0), seed=141), EllipsoidWallCase("411", (4.0, 1.0, 1.0), seed=142),
             EllipsoidWallCase("221", (2.0, 2.0, 1.0), seed=143), EllipsoidWallCase("111", (1.0, 1.0, 1.0), seed=144),
             EllipsoidWallCase("321_rotated", (3.0, 2.0, 1.0), quat=q, seed=145),
             FastWallCase(), SphereHertzCase(),
             SegmentCase("hertz", False), SegmentCase("hertz", True), SegmentCase("wca", False),
             SegmentCase("wca", True)]
    return {c.name: c for c in cases}


_CASES = {}


def cases():
    if not _CASES:
        _CASES.update(_build())
    return _CASES


NAMES = ("springs_hookean", "springs_fene", "crosslinkers_hookean", "crosslinkers_fene", "crosslinkers_hookean_sites",
         "crosslinkers_fene_sites", "active", "wall_sphere", "wall_ellipsoid_321", "wall_ellipsoid_411",
         "wall_ellipsoid_221", "wall_ellipsoid_111", "wall_ellipsoid_321_rotated", "wall_ellipsoid_fast", "hertz_spheres",
         "segments_hertz", "segments_hertz_end_correction", "segments_wca", "segments_wca_end_correction")


def deviation(F, Fexact, S):
    """per row: max_k |F[b, k] - Fexact[b, k]| in units of eps S_b (rows with S_b = 0 must agree exactly: inf otherwise)"""
    err = np.abs(np.asarray(F) - np.asarray(Fexact)).max(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(S > 0, err / (EPS * S), np.where(err == 0, 0.0, np.inf))


_EXACT = {}


def exact(name):
    """the mpmath forces of a case in its own frame, once -> (F float64 [rows, 3], S float64 [rows])"""
    if name not in _EXACT:
        with P.hp():
            F, S = cases()[name].exact()
            _EXACT[name] = (P.to_float(F), np.array([float(s) for s in S]))
    return _EXACT[name]


def fsum_rows(rows):
    return np.array([math.fsum(float(v) for v in rows[:, k]) for k in range(rows.shape[1])])


# ---- the mobility's cloud ------------------------------------------------------------------------------------------------------------------
VISCOSITY = 0.9


def mobility_cloud():
    """48 beads, radii uniform in 0.2 .. 1.2, in a box of 3: 1604 far, 622 overlapping and 30 nested ordered pairs, every
    pair at least 1e-3 from a branch boundary -> (center [48, 3], radius [48], branch [48, 48] of 'f' / 'o' / 'n' / '-')"""
    rng = np.random.default_rng(3)
    c = rng.uniform(0.0, 3.0, (48, 3)) + SHIFT
    a = rng.uniform(0.2, 1.2, 48)
    r = np.linalg.norm(c[:, None] - c[None], axis=2)
    s, m = a[:, None] + a[None], np.abs(a[:, None] - a[None])
    branch = np.where(r > s, "f", np.where(r > m, "o", "n"))
    branch[np.eye(48, dtype=bool)] = "-"
    off = branch != "-"
    assert min(np.abs(r - s)[off].min(), np.abs(r - m)[off].min()) >= MARGIN
    return c, a, branch


def far_cloud():
    """16 small beads far apart: every pair has r >= 3 (a + b), where RPY must approach RPYC's far branch"""
    rng = np.random.default_rng(4)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(2), np.arange(2), indexing="ij"), -1).reshape(-1, 3)
    c = g * 3.5 + rng.uniform(-0.25, 0.25, (16, 3)) + SHIFT
    a = rng.uniform(0.2, 0.5, 16)
    r = np.linalg.norm(c[:, None] - c[None], axis=2) + np.eye(16) * 1e9
    assert (r >= 3.0 * (a[:, None] + a[None])).all()
    return c, a


_RPYC = {}


def rpyc_blocks():
    """the mpmath mobility of mobility_cloud(), once -> (M [144, 144] float64 rounded from mpmath, off-diagonal blocks
    only; Mmp: the rows of mpf with the self term)"""
    if not _RPYC:
        c, a, _ = mobility_cloud()
        with P.hp():
            Mmp = P.rpyc_matrix(c, a, VISCOSITY, self_term=True)
            M64 = np.array([[float(v) for v in row] for row in Mmp])
        _RPYC["v"] = (M64, Mmp)
    return _RPYC["v"]


# ---- the longdouble forms over the same inputs -------------------------------------------------------------------------------------------
def ld_energies(case):
    """the energy of every term of case.terms(...) in the original frame, in the same order, by the vectorised
    numpy.longdouble forms -> [terms] longdouble"""
    x, f = P._ld(case.x), case.fixed
    if isinstance(case, SpringCase):
        L = P.ld_norm(x[case.pairs[:, 1]] - x[case.pairs[:, 0]])
        return (P.ld_hookean if case.kind == "hookean" else P.ld_fene)(L, case.k, case.r)
    if isinstance(case, CrosslinkerCase):
        bound, pts, far = case._far(case.x, f.get("sites"))
        L = P.ld_norm(P._ld(pts)[far[bound]] - x[case.left[bound]])
        return (P.ld_hookean if case.kind == "hookean" else P.ld_fene)(L, case.k, case.r)
    if isinstance(case, ActiveCase):
        p = case.pairs[case.state == 1]
        return P.ld_active(P.ld_norm(x[p[:, 1]] - x[p[:, 0]]), case.sigma)
    if isinstance(case, SphereWallCase):
        return P.ld_sphere_wall(x, f["center"], case.radius, case.R, case.K)
    if isinstance(case, EllipsoidWallCase):
        return P.ld_ellipsoid_wall(x, f["center"], f["quat"], case.radii, case.radius, case.K)
    if isinstance(case, FastWallCase):
        return P.ld_ellipsoid_wall_fast(x, f["center"], case.radii, case.radius, case.K)
    if isinstance(case, SphereHertzCase):
        i, j = case.pairs[:, 0], case.pairs[:, 1]
        delta = P._ld(case.radius[i]) + P._ld(case.radius[j]) - P.ld_norm(x[j] - x[i])
        return P.ld_hertz(delta, P.ld_effective_modulus(case.E[i], case.nu[i], case.E[j], case.nu[j]),
                          P.ld_effective_radius(case.radius[i], case.radius[j]))
    if isinstance(case, SegmentCase):
        e, r = case.ends, P._ld(case.radius)
        i, j = case.pi, case.pj
        d = P.ld_segment_segment(x[e[i, 0]], x[e[i, 1]], x[e[j, 0]], x[e[j, 1]])
        c = np.flatnonzero(case.corr)
        L = P.ld_norm(x[e[c, 1]] - x[e[c, 0]])
        if case.kind == "hertz":
            Es = P.ld_effective_modulus(SEG_E, SEG_NU, SEG_E, SEG_NU)
            return np.concatenate([P.ld_hertz(r[i] + r[j] - d, Es, P.ld_effective_radius(r[i], r[j])),
                                   P.ld_hertz(2 * r[c] - L, Es, P.ld_effective_radius(r[c], r[c]))])
        return np.concatenate([P.ld_wca(d, **WCA), P.ld_wca(L, **WCA)])
    raise TypeError(case)


def mp_energies(case):
    """the same by the mpmath forms -> a list of mpf.  Call inside `with P.hp():`."""
    X = [P.vec(p) for p in case.x]
    return [t.energy([X[b] for b in t.bodies]) for t in case.terms(fixed_mp(case.fixed))]


# ---- the tolerances (measured and asserted by tests/test_potentials_host.py, whose docstring holds the table) --------------------------
TOLERANCE_K = {"springs": 16.0, "crosslinkers": 16.0, "active": 4.0, "sphere wall": 64.0, "ellipsoid wall": 512.0,
               "ellipsoid wall, fast": 8.0, "sphere Hertz": 256.0, "segment Hertz": 32.0, "segment WCA": 256.0,
               "rpyc": 16.0, "filament force": 64.0, "filament force, wave": 128.0, "filament torque": 128.0,
               "filament Hertz": 16.0}
FAST_RSQRT_DELTA = 1.752e-3


# ---- the second frame of every case ------------------------------------------------------------------------------------------------------
def at(case, x, fixed):
    """the case with other positions and fixed objects (for its model(): a shallow copy)"""
    import copy
    c = copy.copy(case)
    c.x, c.fixed = x, fixed
    return c


_MOVED = {}


def moved_exact(name):
    """the case rotated by a random rotation Q (seeded by its name; the fast ellipsoid wall: not rotated) and translated
    -> (x' [n, 3], fixed', Q F [rows, 3] float64 with F the mpmath forces at the exact pre-image of x' in the original
    frame, S [rows]); once"""
    if name not in _MOVED:
        case = cases()[name]
        rng = np.random.default_rng(sum(map(ord, name)))
        quat = random_quat(rng) if case.rotates else IDENTITY
        shift = np.array([-1.25, 0.5, 2.0]) + rng.uniform(-0.5, 0.5, 3)
        with P.hp():
            x2, f2, y, fy, Q = moved(case, quat, shift)
            F, S = case.exact(x=y, fixed=fy)
            _MOVED[name] = (x2, f2, P.to_float([P.apply(Q, f) for f in F]), np.array([float(s) for s in S]))
    return _MOVED[name]
