"""The LCP against a hydrodynamic mobility (include/mundy_hip_hydro_solve.h) restated on the CPU: BBPGD as convex.hpp:592-681
states it, in the dry oracle's words (oracle/mundy_oracle.hpp: residual :1231-1247, bb_step :1249-1255, solve_cqpp
:1264-1292) with the BB sums as math.fsum (a double-double pair rounded once), over

    apply(x) = dt * D^T (M_h (D x))      F   = contact_force_model.body_force(x)           (stride 3)
                                         U   = chain_model.drag_velocity(m_t, F)
                                         U  += hydro_model.velocity(kind, F, old=U)
                                         U  += hydro_periphery_model.correct(F, old=U)      (with a periphery)
                                         y_c = dt * (((-n.x (Ui.x - Uj.x)) - n.y (Ui.y - Uj.y)) - n.z (Ui.z - Uj.z))

every product and sum in the device's association.  The inputs of the GPU tests are built here too, so that the host
test can assert the model's convergence on exactly those."""
import math

import numpy as np

import chain_model
import contact_force_model as cfm
import hydro_model as hm
import hydro_periphery_model as pm

SMALL_STEP = 1e-6
ZERO_TOL = 1e-15
LOWEST = -np.finfo(np.float64).max


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def contacts(center, radius, cutoff):
    """pairs i < j with |c_j - c_i| < cutoff, in ascending (i, j): (pairs int32 [C, 2], normal [C, 3] from i to j, sep [C])"""
    n = len(center)
    i, j = np.triu_indices(n, 1)
    d = center[j] - center[i]
    dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    keep = dist < cutoff
    i, j, d, dist = i[keep], j[keep], d[keep], dist[keep]
    pairs = np.ascontiguousarray(np.stack([i, j], axis=1), dtype=np.int32)
    return pairs, np.ascontiguousarray(d / dist[:, None]), dist - (radius[i] + radius[j])


def mobility_of(radius, viscosity):
    return 1.0 / (6.0 * math.pi * viscosity * radius)


def packing(n, side, seed=3, cutoff=1.5, dt=1e-2, viscosity=1.0, hydro_radius=None, lonely=False, centred=False):
    """the issue's case: n spheres of radius 0.5, centres uniform in a box of the given side, pairs closer than cutoff.
    lonely: the second half of the bodies is moved far away, one by one (no contact at all);
    hydro_radius "poly": polydisperse hydrodynamic radii different from the bead radii, and their mobilities;
    centred: the box is centred on the origin (inside a periphery)"""
    rng = np.random.default_rng(seed)
    center = rng.uniform(0.0, side, (n, 3))
    if centred:
        center = center - 0.5 * side
    if lonely:
        half = np.arange(n // 2, n)
        center[half] = np.array([3.0 * side, 0.0, 0.0]) + 5.0 * np.stack([half, 0 * half, 0 * half], axis=1)
    radius = np.full(n, 0.5)
    pairs, normal, sep = contacts(center, radius, cutoff)
    a = radius.copy()
    if hydro_radius == "poly":
        a = rng.uniform(0.2, 0.7, n)
    # (m_t belongs to the hydrodynamic radii: M_h = m_t + RPYC is positive semi-definite only with its own self term)
    return dict(n=n, center=center, radius=radius, hydro_radius=a, pairs=pairs, normal=normal, q=sep, dt=dt,
                viscosity=viscosity, mob_trans=mobility_of(a, viscosity))


def two_beads(r, a, bead_radius, delta, dt=1e-2, viscosity=1.0):
    """one contact, two equal beads a distance r apart along x, sep = -delta"""
    center = np.array([[0.0, 0.0, 0.0], [r, 0.0, 0.0]])
    radius = np.full(2, bead_radius)
    return dict(n=2, center=center, radius=radius, hydro_radius=np.full(2, a), pairs=np.array([[0, 1]], dtype=np.int32),
                normal=np.array([[1.0, 0.0, 0.0]]), q=np.array([-delta]), dt=dt, viscosity=viscosity,
                mob_trans=mobility_of(np.full(2, a), viscosity))


def trap_case(dt=1e-2, viscosity=1.0):
    """three far-apart groups: an overlapping pair (active), a touching pair with q > 0 (inactive), a lone bead"""
    center = np.array([[0.0, 0.0, 0.0], [0.9, 0.0, 0.0], [8.0, 0.0, 0.0], [8.0, 1.05, 0.0], [4.0, 7.0, 3.0]])
    radius = np.full(5, 0.5)
    pairs = np.array([[0, 1], [2, 3]], dtype=np.int32)
    normal = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    q = np.array([0.9 - 1.0, 1.05 - 1.0])
    return dict(n=5, center=center, radius=radius, hydro_radius=radius.copy(), pairs=pairs, normal=normal, q=q, dt=dt,
                viscosity=viscosity, mob_trans=mobility_of(radius, viscosity))


# the cases of tests/test_gpu_hydro_solve.py, by name: the issue's main case (two source chunks, 1024 + 76, five source
# tiles), the same at n = 300, a chunk of one source, two and three bodies, no contact at all, half the bodies without a
# contact, hydrodynamic radii of their own, the n = 300 case inside a periphery, the cold tier's trap
PACKINGS = {
    "main": dict(n=1100, side=14.0),
    "n300": dict(n=300, side=9.0),
    "n1025": dict(n=1025, side=13.7),
    "n3": dict(n=3, side=1.2),
    "lonely": dict(n=300, side=7.1, lonely=True),
    "poly": dict(n=300, side=9.0, hydro_radius="poly"),
    "centred": dict(n=300, side=9.0, centred=True),
    "c0": dict(n=40, side=30.0, cutoff=1e-3),
}
CASE_NAMES = tuple(PACKINGS) + ("n2", "trap")
_CASES = {}


def case_of(name):
    """the named case, built once and left unchanged"""
    if name not in _CASES:
        if name == "n2":
            _CASES[name] = two_beads(0.9, 0.5, 0.5, 0.1)
        elif name == "trap":
            _CASES[name] = trap_case()
        else:
            _CASES[name] = packing(**PACKINGS[name])
    return _CASES[name]


def closed_form_lambda(r, a, delta, dt, viscosity, branch):
    """lambda = delta / (2 dt (m - c)), c the pair mobility along the line of centres (the header's RPYC formulas)"""
    m = 1.0 / (6.0 * math.pi * viscosity * a)
    if branch == "overlap":  # equal radii: t1 + t2 of the overlapping form
        so = 1.0 / (6.0 * math.pi * viscosity) / (a * a)
        t1 = so * (16.0 * r ** 3 * (2.0 * a) - (3.0 * r * r) ** 2) / 32.0 / r ** 3
        t2 = so * 3.0 * (r * r) ** 2 / 32.0 / r ** 3
        c = t1 + t2
    else:
        s = 1.0 / (8.0 * math.pi * viscosity * r)
        qq = 2.0 * a * a / (r * r)
        c = s * (2.0 - 2.0 * qq / 3.0)
    return delta / (2.0 * dt * (m - c))


# ---- the operator ------------------------------------------------------------------------------------------------------------
class RpycGeometry:
    """hydro_model.pair_terms("rpyc") for beads onto beads with everything that depends on the geometry alone formed once
    (the same operations in the same association: test_hydro_solve_host.py compares it with hydro_model.velocity bit for
    bit), so that an iteration of the model costs a few array operations"""

    def __init__(self, viscosity, center, radius):
        _, c8, c6 = hm.constants(viscosity)
        one_over_three, one_over_32 = np.float64(1.0 / 3.0), np.float64(1.0 / 32.0)
        with np.errstate(all="ignore"):
            d = center[:, None, :] - center[None, :, :]  # [target, source]
            b, a = radius[:, None], radius[None, :]
            dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
            r2 = (dx * dx + dy * dy) + dz * dz
            r = np.sqrt(r2)
            r3 = r * r2
            rinv = np.where(r2 < hm.DOUBLE_ZERO, 0.0, 1.0 / r)
            rinv2 = rinv * rinv
            rinv3 = rinv2 * rinv
            self.h = (dx * rinv, dy * rinv, dz * rinv)
            q = (a * a + b * b) * rinv2
            sf = c8 * rinv
            t1f = sf * (1.0 + q * one_over_three)
            t2f = sf * (1.0 - q)
            e = (a - b) * (a - b)
            tmp3 = e + 3.0 * r2
            tmp4 = e - r2
            so = c6 / (a * b)
            t1o = ((so * ((16.0 * r3) * (a + b) - tmp3 * tmp3)) * one_over_32) * rinv3
            t2o = ((((so * 3.0) * tmp4) * tmp4) * one_over_32) * rinv3
            self.sl = np.broadcast_to(c6 / np.where(a < b, b, a), r2.shape)
            br = hm.rpyc_branch(d, a, b)
        self.t1 = np.where(br == hm.FAR, t1f, t1o)
        self.t2 = np.where(br == hm.FAR, t2f, t2o)
        self.two = br <= hm.OVERLAP
        self.local = br == hm.LOCAL
        self.n = len(center)

    def velocity(self, force, old=None, chunk=hm.CHUNK, block=256):
        n = self.n
        fx, fy, fz = force[None, :, 0], force[None, :, 1], force[None, :, 2]
        hx, hy, hz = self.h
        with np.errstate(all="ignore"):
            fdh = (fx * hx + fy * hy) + fz * hz
            terms = np.stack([np.where(self.two, self.t1 * f + self.t2 * (fdh * h), np.where(self.local, self.sl * f, 0.0))
                              for f, h in ((fx, hx), (fy, hy), (fz, hz))], axis=-1)
        total = np.zeros((n, 3))
        for c0 in range(0, n, chunk):
            acc = np.zeros((n, 3))
            for s0 in range(c0, min(c0 + chunk, n), block):
                s1 = min(s0 + block, c0 + chunk, n)
                acc = np.add.accumulate(np.concatenate([acc[:, None, :], terms[:, s0:s1]], axis=1), axis=1)[:, -1, :]
            total = total + acc
        return total if old is None else old + total


class Operator:
    """A = dt D^T M_h D of a case (packing / two_beads / trap_case).  kind None: the dry operator (M_h = m_t);
    periphery = dict(points, weights, normals, inverse, viscosity, skip_same_index); viscosity overrides the case's in
    the hydrodynamic part only (the dry limit)"""

    def __init__(self, case, kind="rpyc", periphery=None, viscosity=None):
        self.case, self.kind, self.periphery = case, kind, periphery
        self.viscosity = case["viscosity"] if viscosity is None else viscosity
        self.geometry = None
        if kind == "rpyc":
            self.geometry = RpycGeometry(self.viscosity, case["center"], case["hydro_radius"])

    def body_force(self, x):
        c = self.case
        return cfm.body_force(c["n"], c["pairs"], x=x, normal=c["normal"], stride=3)

    def rows(self, x):
        """M_h D x as [n, 6]"""
        c = self.case
        F = self.body_force(x)
        U = chain_model.drag_velocity(c["mob_trans"], F)
        if self.kind is not None:
            if self.geometry is not None:
                U[:, :3] = self.geometry.velocity(F, old=U[:, :3])
            else:
                U[:, :3] = hm.velocity(self.kind, self.viscosity, c["center"], c["hydro_radius"], F, old=U[:, :3])
            p = self.periphery
            if p is not None:
                U[:, :3] = pm.correct(self.kind, p["viscosity"], p["points"], p["weights"], p["normals"], p["inverse"],
                                      c["center"], c["hydro_radius"], F, old=U[:, :3],
                                      skip_same_index=p["skip_same_index"])[0]
        return U

    def constraint_rate(self, U):
        """the sphere form of mhip_contact_op_constraint_rate"""
        c = self.case
        n = c["normal"]
        vi, vj = U[c["pairs"][:, 0], :3], U[c["pairs"][:, 1], :3]
        return ((-n[:, 0]) * (vi[:, 0] - vj[:, 0]) - n[:, 1] * (vi[:, 1] - vj[:, 1])) - n[:, 2] * (vi[:, 2] - vj[:, 2])

    def apply(self, x, want_rows=False):
        U = self.rows(x)
        y = self.case["dt"] * self.constraint_rate(U)
        return (y, U) if want_rows else y


# ---- the solver ---------------------------------------------------------------------------------------------------------------
def project(v):
    return np.where(v < 0.0, 0.0, v)  # LowerBound{0}: (x < lo) ? lo : x


def residual(x, g):
    """projected-difference residual (convex.hpp:434-496); an empty max keeps Kokkos::Max's identity"""
    if len(x) == 0:
        with np.errstate(over="ignore"):
            return LOWEST / SMALL_STEP
    return float(np.max(np.abs(x - project(x - SMALL_STEP * g)))) / SMALL_STEP


def bb_step(x_old, g_old, x, g):
    dx = x - x_old
    num = math.fsum(dx * dx) + 0.0
    den = math.fsum(dx * (g - g_old)) + 0.0
    eps = ZERO_TOL * 10
    den += eps * (abs(den) < eps)
    with np.errstate(all="ignore"):
        return float(np.float64(num) / np.float64(den))


def solve(op, q, x0, max_iters=1000, tol=1e-8):
    """-> dict(x, g, x_tmp, g_tmp, rows, num_iters, residual, converged): solve_cqpp of the dry oracle over op.apply;
    rows = M_h D x of the returned x"""
    q = np.asarray(q, dtype=np.float64)
    x_tmp = np.array(x0, dtype=np.float64)
    y, rows = op.apply(x_tmp, want_rows=True)
    g_tmp = 1.0 * q + 1.0 * y
    res = residual(x_tmp, g_tmp)
    with np.errstate(all="ignore"):
        step = float(np.float64(1.0) / np.float64(res))
    it, converged = 0, res <= tol
    x, g = x_tmp.copy(), g_tmp.copy()
    while not (converged or it >= max_iters):
        with np.errstate(all="ignore"):
            v = 1.0 * x_tmp if abs(-step) < ZERO_TOL else 1.0 * x_tmp + (-step) * g_tmp
        x = project(v)
        y, rows = op.apply(x, want_rows=True)
        g = 1.0 * q + 1.0 * y
        res = residual(x, g)
        if res <= tol:
            converged = True
            break
        step = bb_step(x_tmp, g_tmp, x, g)
        x_tmp, g_tmp = x.copy(), g.copy()
        it += 1
    return dict(x=x, g=g, x_tmp=x_tmp, g_tmp=g_tmp, rows=rows, num_iters=it, residual=res, converged=bool(converged))
