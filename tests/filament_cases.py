"""The filament family's configurations for tests/test_potentials_host.py (calibration) and
tests/test_gpu_force_gradients.py (the device against the discrete rod energy): a sibling of tests/gradient_cases.py,
because a filament has twists beside positions and an energy that holds the last evaluation's tangents and frames
fixed, which the Case interface has no place for.

A State is what one evaluation of the force starts from -- centres x, twists theta, the old tangents T and old frames D
-- taken from a run of the numpy model (filament_model.py), never from the device, and the model's own output for
calibration.  exact(state) is, in mpmath and on the state's compared nodes,
        F = -dE/dx (+ R),   tau = -dE/dtheta,   S_F, S_tau
of the energy of tests/potentials.py ("the discrete rod"): per element i (the interior node i with the edges i - 1 and
i) and per edge, so that a node needs its <= 3 elements and 2 edges only.  S_F[b] is the sum of the magnitudes of the
five terms node b gathers, S_tau[b] = |dE_b/dtheta_b| + |dE_{b+1}/dtheta_b|.

The stray term.  The reference's force of element i on its right node has `- b_i` outside the factor 1/2 (t_i.m_i)
that multiplies it in the gradient.  With t_i.m_i = -dE_i/dtheta_i the law is
        F = -grad E + R,     R_i = -(1 / l_i) (1 + 1/2 dE_i/dtheta_i) b_i  on node i + 1,   -R_i on node i,
b_i = 2 T_i x t_i / (1 + T_i.t_i) the binormal of edge i between its old and its new tangent.  At the first evaluation
after set_state T = t and R vanishes; exact(stray=True) adds R, assembled from the mpmath dE_i/dtheta_i.

Layouts: "small", filaments of 2 (stretch only), 3 (one element), 4, 5, 20, 3, 2 and 4 nodes, 43 nodes; "border", one
filament of 259 nodes, whose nodes 256 .. 258 lie past the border of the node pass's 256-node tile, compared on its last
12 nodes only; "planar", the small layout in the plane x = 0 (the monolayer); radii 0.5 .. 1, rest curvatures +-0.1 per
component, twists +-0.3, edge lengths 0.85 .. 1.2, E = 10, nu = 0.3, l0 = 1, the triad of every edge d1 = (1, 0, 0),
d2 = t x d1 / |t x d1|, d3 = t through the reference's rotation_matrix_to_quaternion.
States: "first" (the first evaluation after set_state, at time 0.25), "wave" (the same with the rest-curvature wave on),
"moved" (first evaluation, velocity, advance(0.02), then the evaluation at time 0.5: T != t, the binormal acts).

ContactCase: filaments grown like gradient_cases.grow_segments grows its chains (five of five nodes, twelve of two laid
across them), every listed pair 2 MARGIN from the overlap boundary, MIN_SIN from parallel."""
import math

import mpmath as mp
import numpy as np

import filament_model as fm
import gradient_cases as gc
import potentials as P

EPS = gc.EPS
M = gc.M
E, NU, L0, ETA = 10.0, 0.3, 1.0, 1.0
WAVE = dict(amplitude=0.2, wave_number=0.7, frequency=1.3)
TIME_FIRST, TIME_MOVED, DT = 0.25, 0.5, 0.02
MIN_BINORMAL = 1e-3
COUNTS = {"small": (2, 3, 4, 5, 20, 3, 2, 4), "border": (259,), "planar": (2, 3, 4, 5, 20, 3, 2, 4)}
STATES = ("first", "wave", "moved")
NAMES = tuple("filaments_%s_%s" % (s, lay) for lay in ("small", "border") for s in STATES)


def params(wave=False, disable_twist=False, monolayer=False):
    return fm.Params(E=E, nu=NU, l0=L0, eta=ETA, A=WAVE["amplitude"] if wave else 0.0,
                     k=WAVE["wave_number"] if wave else 0.0, omega=WAVE["frequency"] if wave else 0.0, wave=wave,
                     disable_twist=disable_twist, monolayer=monolayer)


def device_kwargs(prm):
    return dict(youngs_modulus=prm.E, poisson_ratio=prm.nu, rest_length=prm.l0, viscosity=prm.eta,
                wave=WAVE if prm.wave else None, disable_twist=prm.disable_twist, monolayer=prm.monolayer)


_LAYOUTS = {}


def layout(name):
    """-> dict(node_ptr, center, twist, radius, rest_curvature, arclength, edge_orientation, phase, n, compared)"""
    if name in _LAYOUTS:
        return _LAYOUTS[name]
    counts = np.asarray(COUNTS[name])
    rng = np.random.default_rng({"small": 51, "border": 52, "planar": 53}[name])
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n, F = int(ptr[-1]), len(counts)
    last = np.zeros(n, bool)
    last[ptr[1:] - 1] = True
    fid = np.repeat(np.arange(F), counts)
    # tangents: a random walk on the sphere, restarted at every filament's first edge
    walk = np.cumsum(rng.normal(scale=0.15, size=(n, 3)), axis=0)
    t = np.array([0.1, 0.2, 1.0]) + walk - walk[ptr[:-1]][fid]
    if name == "planar":
        t[:, 0] = 0.0
    t /= np.sqrt((t * t).sum(axis=1))[:, None]
    step = t * rng.uniform(0.85, 1.2, (n, 1))
    step[last] = 0.0
    c = np.cumsum(np.concatenate([np.zeros((1, 3)), step[:-1]]), axis=0)
    c = c - c[ptr[:-1]][fid] + (rng.uniform(-3.0, 3.0, (F, 3)) + gc.SHIFT)[fid]
    if name == "planar":
        c[:, 0] = 0.0
    quat = np.array([fm.triad_orientation(tk) for tk in t])
    quat[last] = (1.0, 0.0, 0.0, 0.0)
    s = (np.arange(n) - ptr[:-1][fid]).astype(np.float64)
    compared = np.arange(n - 12, n) if name == "border" else np.arange(n)
    _LAYOUTS[name] = dict(node_ptr=ptr, center=np.ascontiguousarray(c), twist=rng.uniform(-0.3, 0.3, n),
                          radius=rng.uniform(0.5, 1.0, n), rest_curvature=rng.uniform(-0.1, 0.1, (n, 3)), arclength=s,
                          edge_orientation=quat, phase=rng.uniform(0.0, 2.0 * math.pi, F), n=n, compared=compared)
    return _LAYOUTS[name]


def rotated(lay, quat, shift):
    """the layout rotated by the unit quaternion `quat` and translated, in float64: x' = Q x + s, frames quat * q"""
    R = np.asarray(P.ld_rotation(quat), dtype=np.float64)
    out = dict(lay)
    out["center"] = np.ascontiguousarray(lay["center"] @ R.T + np.asarray(shift, dtype=np.float64))
    out["edge_orientation"] = np.array([gc.quat_mul(quat, q) for q in lay["edge_orientation"]])
    return out


def new_model(lay, prm):
    f = fm.Filaments(lay["node_ptr"], lay["radius"], lay["rest_curvature"], lay["arclength"], lay["phase"], prm)
    return f.set_state(lay["center"], lay["twist"], lay["edge_orientation"])


class State:
    """the inputs of one force evaluation and the numpy model's output there"""

    def __init__(self, lay, kind):
        self.layout, self.kind, self.wave = lay, kind, kind == "wave"
        self.prm = params(wave=self.wave)
        m = new_model(lay, self.prm)
        self.time = TIME_FIRST
        if kind == "moved":
            m.compute_force(TIME_FIRST)
            m.compute_velocity()
            m.advance(DT)
            self.time = TIME_MOVED
        self.x, self.theta = m.center.copy(), m.twist.copy()
        self.T, self.D = m.edge_tangent_old.copy(), m.edge_orientation_old.copy()
        self.stats = m.compute_force(self.time)
        self.model = m
        self.nodes = np.asarray(lay["compared"])
        self.has_l, self.has_r, self.interior = m.has_l, m.has_r, m.interior

    def check(self):
        m = self.model
        e = self.has_r
        assert (np.diff(self.layout["node_ptr"]) >= 2).all()
        tt = (self.T[e] * m.edge_tangent[e]).sum(axis=1)
        assert (1.0 + tt >= 1.0).all()   # no edge near the pole of the transport
        assert np.abs(self.theta[e]).max() > 0.1
        b = np.abs(m.edge_binormal[e]).max()
        if self.kind == "moved":
            assert b >= MIN_BINORMAL, b
        else:
            assert b == 0.0

    def model_rows(self):
        return self.model.force[self.nodes], self.model.twist_torque[self.nodes]


def exact(st, quat=None, shift=None, stray=False):
    """-> dict(F [rows, 3], tau [rows], S_F [rows], S_tau [rows], R [rows, 3]) as float64, rows = st.nodes.  With quat and
    shift the state is one that was run from a rotated layout: the energy is taken at its exact pre-image x = Q^T (x' -
    s), T = Q^T T', D = conj(quat) D', and F and R are returned turned back by Q.  Call inside `with P.hp():`."""
    lay = st.layout
    n = lay["n"]
    X, T = [P.vec(p) for p in st.x], [P.vec(p) for p in st.T]
    D = [[M(v) for v in q] for q in st.D]
    Q = None
    if quat is not None:
        Q, s = P.rotation(quat), P.vec(shift)
        qn = [M(v) for v in quat]
        nq = mp.sqrt(sum(v * v for v in qn))
        qc = P.qconj([v / nq for v in qn])
        X = [P.apply(Q, P.sub(p, s), transpose=True) for p in X]
        T = [P.apply(Q, p, transpose=True) for p in T]
        D = [P.qmul(qc, q) for q in D]
    th = [M(v) for v in st.theta]
    r = [M(v) for v in lay["radius"]]
    Em, num, l0 = M(E), M(NU), M(L0)
    fid = np.repeat(np.arange(len(lay["node_ptr"]) - 1), np.diff(lay["node_ptr"]))
    zero3 = [mp.mpf(0)] * 3
    F = {int(b): list(zero3) for b in st.nodes}
    Rn = {int(b): list(zero3) for b in st.nodes}
    SF = {int(b): mp.mpf(0) for b in st.nodes}
    tau = {int(b): mp.mpf(0) for b in st.nodes}
    St = {int(b): mp.mpf(0) for b in st.nodes}

    def gather(b, f, stray_part=None):
        if b in F:
            if stray_part is not None:
                Rn[b] = [Rn[b][k] + stray_part[k] for k in range(3)]
                f = [f[k] + stray_part[k] for k in range(3)]
            F[b] = [F[b][k] + f[k] for k in range(3)]
            SF[b] = SF[b] + P.norm(f)

    elements = sorted({i for b in st.nodes for i in (b - 1, b, b + 1) if 0 <= i < n and st.interior[i]})
    edges = sorted({e for b in st.nodes for e in (b - 1, b) if 0 <= e < n and st.has_r[e] and (e == b or st.has_l[b])})
    for i in elements:
        rest = P.vec(lay["rest_curvature"][i])
        if st.wave:
            rest = P.wave_rest_curvature(rest, M(WAVE["amplitude"]), M(WAVE["wave_number"]), M(lay["arclength"][i]),
                                         M(WAVE["frequency"]), M(st.time), M(lay["phase"][fid[i]]))

        def energy(p, t2, i=i, rest=rest):
            return P.rod_element(p, t2, (T[i - 1], T[i]), (D[i - 1], D[i]), rest, r[i], Em, num, l0)

        gx, gt = P.rod_gradient(energy, [X[i - 1], X[i], X[i + 1]], [th[i - 1], th[i]])
        R = None
        if stray:
            d = P.sub(X[i + 1], X[i])
            L = P.norm(d)
            t = [v / L for v in d]
            c = P.cross(T[i], t)
            w = 1 + P.dot(T[i], t)
            dE = -gt[1]   # dE_i / dtheta_i
            R = [-(1 + dE / 2) * (2 * v / w) / L for v in c]
        gather(i - 1, gx[0])
        gather(i, gx[1], None if R is None else [-v for v in R])
        gather(i + 1, gx[2], R)
        for b, g in ((i - 1, gt[0]), (i, gt[1])):
            if b in tau:
                tau[b], St[b] = tau[b] + g, St[b] + abs(g)
    for e in edges:
        gx, _ = P.rod_gradient(lambda p, _t, e=e: P.rod_edge(p, r[e + 1], Em, l0), [X[e], X[e + 1]], [])
        gather(e, gx[0])
        gather(e + 1, gx[1])
    rows = [int(b) for b in st.nodes]
    turn = (lambda v: P.apply(Q, v)) if Q is not None else (lambda v: v)
    return dict(F=P.to_float([turn(F[b]) for b in rows]), R=P.to_float([turn(Rn[b]) for b in rows]),
                tau=np.array([float(tau[b]) for b in rows]), S_F=np.array([float(SF[b]) for b in rows]),
                S_tau=np.array([float(St[b]) for b in rows]))


_STATES, _EXACT, _MOVED = {}, {}, {}


def split(name):
    _, kind, lay = name.split("_")
    return kind, lay


def state(name):
    if name not in _STATES:
        kind, lay = split(name)
        _STATES[name] = State(layout(lay), kind)
    return _STATES[name]


def exact_of(name):
    """the state's exact forces (with the stray term where it acts: "moved") and torques, once"""
    if name not in _EXACT:
        with P.hp():
            _EXACT[name] = exact(state(name), stray=split(name)[0] == "moved")
    return _EXACT[name]


def rigid_motion(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    return gc.random_quat(rng), np.array([-1.25, 0.5, 2.0]) + rng.uniform(-0.5, 0.5, 3)


def moved_exact(name):
    """the state reached from the layout rotated and translated (seeded by the name), with Q F, tau and S at its exact
    pre-image -> (the rotated layout, State, exact); once"""
    if name not in _MOVED:
        kind, lay = split(name)
        quat, shift = rigid_motion(name)
        lay2 = rotated(layout(lay), quat, shift)
        st = State(lay2, kind)
        with P.hp():
            _MOVED[name] = (lay2, st, exact(st, quat, shift, stray=kind == "moved"))
    return _MOVED[name]


def deviation(F, Fexact, S):
    F, Fexact = np.asarray(F), np.asarray(Fexact)
    return gc.deviation(F.reshape(len(S), -1), Fexact.reshape(len(S), -1), S)


# ---- the two forms over the same inputs ---------------------------------------------------------------------------------------------
def ld_energies(st):
    """the energy of every element and edge of the state, by the longdouble forms -> (elements [n], edges [n])"""
    lay, e = st.layout, np.flatnonzero(st.has_r)
    q = np.zeros((lay["n"], 4), dtype=P.LD)
    q[e] = P.ld_edge_frame(st.T[e], P.ld_unit_tangent(st.x[e], st.x[e + 1]), st.theta[e], st.D[e])
    rest = lay["rest_curvature"]
    if st.wave:
        fid = np.repeat(np.arange(len(lay["node_ptr"]) - 1), np.diff(lay["node_ptr"]))
        rest = P.ld_wave_rest_curvature(rest, WAVE["amplitude"], WAVE["wave_number"], lay["arclength"], WAVE["frequency"],
                                        st.time, lay["phase"][fid])
    return P.ld_rod_energy(lay["node_ptr"], st.x, q, lay["radius"], rest, E, NU, L0)


def mp_energies(st, nodes):
    """the same by the mpmath forms, for the elements and edges `nodes` index -> (elements, edges): lists of mpf (None
    where a node has no element or no edge).  Call inside `with P.hp():`."""
    lay = st.layout
    X, T = [P.vec(p) for p in st.x], [P.vec(p) for p in st.T]
    D = [[M(v) for v in q] for q in st.D]
    fid = np.repeat(np.arange(len(lay["node_ptr"]) - 1), np.diff(lay["node_ptr"]))
    el, ed = [], []
    for i in nodes:
        if st.interior[i]:
            rest = P.vec(lay["rest_curvature"][i])
            if st.wave:
                rest = P.wave_rest_curvature(rest, M(WAVE["amplitude"]), M(WAVE["wave_number"]), M(lay["arclength"][i]),
                                             M(WAVE["frequency"]), M(st.time), M(lay["phase"][fid[i]]))
            el.append(P.rod_element([X[i - 1], X[i], X[i + 1]], [M(st.theta[i - 1]), M(st.theta[i])], (T[i - 1], T[i]),
                                    (D[i - 1], D[i]), rest, M(lay["radius"][i]), M(E), M(NU), M(L0)))
        else:
            el.append(None)
        ed.append(P.rod_edge([X[i], X[i + 1]], M(lay["radius"][i + 1]), M(E), M(L0)) if st.has_r[i] else None)
    return el, ed


# ---- contacts between filament segments ---------------------------------------------------------------------------------------------
CONTACT_E, CONTACT_NU, CONTACT_SKIN = 200.0, 0.3, 0.3
CONTACT_SEED = 308   # the first seed from 300 on whose configuration grows to the end and meets ContactCase.check


class ContactCase:
    group = "filament Hertz"

    def __init__(self, seed=CONTACT_SEED):
        good, self.x, ends, rseg = gc.grow_segments(seed, "hertz", branch=False)
        self.good = good and bool((ends[:, 1] == ends[:, 0] + 1).all())
        self.n = n = self.x.shape[0]
        self.has_r = np.zeros(n, bool)
        self.has_r[ends[:, 0]] = True
        first = np.concatenate([[True], ~self.has_r[:-1]])
        self.node_ptr = np.concatenate([np.flatnonzero(first), [n]]).astype(np.int32)
        self.radius = np.zeros(n)
        self.radius[ends[:, 0]] = rseg
        self.radius[~self.has_r] = self.radius[np.flatnonzero(~self.has_r) - 1]   # a last node owns no segment
        self.ends = ends
        seg = ends[:, 0]
        i, j = gc._unshared_pairs(ends)
        d, sin, cls = gc._seg_dist(self.x, ends, i, j)
        near = d < self.radius[seg[i]] + self.radius[seg[j]] + 0.3
        self.pi, self.pj, self.d, self.sin, self.cls = seg[i[near]], seg[j[near]], d[near], sin[near], cls[near]
        fid = np.repeat(np.arange(len(self.node_ptr) - 1), np.diff(self.node_ptr))
        s = (np.arange(n) - self.node_ptr[:-1][fid]).astype(np.float64)
        self.layout = dict(node_ptr=self.node_ptr, center=self.x, twist=np.zeros(n), radius=self.radius,
                           rest_curvature=np.zeros((n, 3)), arclength=s,
                           edge_orientation=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), phase=np.zeros(len(self.node_ptr) - 1), n=n)

    def boundary(self):
        return self.radius[self.pi] + self.radius[self.pj]

    def in_branch(self):
        return self.d < self.boundary()

    def check(self, bonded_exclusion=1):
        assert self.good and 24 <= self.n <= 51 and np.ptp(self.radius) > 0.1
        inb = self.in_branch()
        assert (np.abs(self.d - self.boundary()) >= 2 * gc.MARGIN).all() and inb.sum() >= 16 and (~inb).sum() >= 8
        assert (self.sin[inb] >= gc.MIN_SIN).all() and (self.d[inb] >= gc.MIN_DIST).all()
        cls = self.cls[inb]
        assert (cls == 0).sum() * 3 >= len(cls) and (cls == 2).any() and (cls == 1).any(), np.bincount(cls, minlength=3)
        fid = np.repeat(np.arange(len(self.node_ptr) - 1), np.diff(self.node_ptr))
        assert not ((fid[self.pi] == fid[self.pj]) & (np.abs(self.pj - self.pi) <= bonded_exclusion)).any()
        # the closest-point map's branch changes: a parameter that is clamped stays clamped, an interior one interior
        # (the free minimiser of each parameter with the other held, s* = (b t - d) / a and t* = (b s + e) / c in
        # potentials.segment_segment's letters, is 2 MARGIN inside (0, 1) or 2 MARGIN outside [0, 1])
        _, s, t = (np.asarray(v, dtype=np.float64) for v in self.closest())
        x = self.x
        u, v, w = x[self.pi + 1] - x[self.pi], x[self.pj + 1] - x[self.pj], x[self.pi] - x[self.pj]
        dots = lambda p, q: (p * q).sum(axis=1)  # noqa: E731
        free = ((dots(u, v) * t - dots(u, w)) / dots(u, u), (dots(u, v) * s + dots(v, w)) / dots(v, v))
        for q, star in zip((s, t), free):
            inner = (q > 0) & (q < 1)
            assert (np.abs(star - q)[inner] <= 1e-12).all()
            assert (np.minimum(np.abs(star), np.abs(1 - star))[inb] >= 2 * gc.MARGIN).all()

    def closest(self):
        x = self.x
        return P.ld_segment_segment(x[self.pi], x[self.pi + 1], x[self.pj], x[self.pj + 1], want_parameters=True)

    def terms(self):
        Em, num = M(CONTACT_E), M(CONTACT_NU)
        return [P.Term((i, i + 1, j, j + 1),
                       (lambda p, ri=M(self.radius[i]), rj=M(self.radius[j]):
                        P.filament_pair_hertz(p[0], p[1], p[2], p[3], ri, rj, Em, num)), 2)
                for i, j in zip(self.pi, self.pj)]

    def ld_energies(self):
        x = self.x
        return P.ld_filament_pair_hertz(x[self.pi], x[self.pi + 1], x[self.pj], x[self.pj + 1], self.radius[self.pi],
                                        self.radius[self.pj], CONTACT_E, CONTACT_NU)

    def contact_kwargs(self, mu=0.0):
        return dict(skin=CONTACT_SKIN, youngs_modulus=CONTACT_E, poisson_ratio=CONTACT_NU, mu=mu)

    def model(self):
        import filament_contact_model as fcm
        c = fcm.Contacts(new_model(self.layout, params()), **self.contact_kwargs())
        c.update()
        c.force_pass(DT)
        return c.node_force


_CONTACT = {}


def contact_case():
    if "case" not in _CONTACT:
        _CONTACT["case"] = ContactCase()
    return _CONTACT["case"]


def contact_exact():
    """-> (F [n, 3], S [n]) of the frictionless Hertz energy of the listed pairs, once"""
    if "exact" not in _CONTACT:
        c = contact_case()
        with P.hp():
            F, S, _ = P.exact_forces(c.terms(), c.x, n=c.n)
            _CONTACT["exact"] = (P.to_float(F), np.array([float(s) for s in S]))
    return _CONTACT["exact"]


def planted(case, pairs):
    """saved node velocities and a tangential history for the listed pairs (seeded) -> (velocity [n, 3], tang_disp [c, 3])"""
    rng = np.random.default_rng(61)
    return rng.normal(size=(case.n, 3)), rng.normal(scale=2e-3, size=(len(pairs), 3))


def contact_balance(case, pairs, pair_force, node_force):
    """the momentum and the angular momentum of a contact stage's output, the sums by math.fsum: every pair force acts
    at the closest point cp1 of its first segment and its negative at cp2 of the second (both from the longdouble
    distance), and the barycentric share hands exactly that force and that moment to the segment's two nodes
    -> (|sum F| / (eps sum |F|), |sum x x F - sum (cp1 - cp2) x F_pair| / (eps sum |x| |F|))"""
    x = case.x
    i, j = pairs[:, 0], pairs[:, 1]
    _, s, t = P.ld_segment_segment(x[i], x[i + 1], x[j], x[j + 1], want_parameters=True)
    xl = P._ld(x)
    arm = np.asarray((xl[i] + s[:, None] * (xl[i + 1] - xl[i])) - (xl[j] + t[:, None] * (xl[j + 1] - xl[j])), dtype=np.float64)
    couple = gc.fsum_rows(np.concatenate([np.cross(x, node_force), -np.cross(arm, pair_force)]))
    total = gc.fsum_rows(node_force)
    sum_f = math.fsum(np.linalg.norm(node_force, axis=1))
    sum_xf = math.fsum(np.linalg.norm(x, axis=1) * np.linalg.norm(node_force, axis=1))
    return np.abs(total).max() / (EPS * sum_f), np.abs(couple).max() / (EPS * sum_xf)


# ---- the energy along a trajectory ----------------------------------------------------------------------------------------------------
DESCENT_STEPS, DESCENT_DT = 12, 0.01


def descent_ratios(lay, step, monolayer):
    """step() -> (F [n, 3], v [n, 3], x [n, 3], q [n, 4]) after one more step (advance by the last velocity, then force
    and velocity at the new centres); E in longdouble from the centres and the stepped frames -> per step (E before, E
    after, -dE / (dt F.v)), F and v those the advance to `after` used"""
    rows, prev = [], None
    for _ in range(DESCENT_STEPS + 1):
        F, v, x, q = step()
        bend, stretch = P.ld_rod_energy(lay["node_ptr"], x, q, lay["radius"], lay["rest_curvature"], E, NU, L0)
        U = bend.sum() + stretch.sum()
        if prev is not None:
            U0, F0, v0 = prev
            fv = np.sum(P._ld(F0) * P._ld(v0))
            rows.append((float(U0), float(U), float(-(U - U0) / (P.LD(DESCENT_DT) * fv))))
        v = np.array(v)
        if monolayer:
            v[:, 0] = 0.0   # advance() moves no node out of the plane
        prev = (U, np.array(F), v)
    return rows


def model_descent(name, monolayer):
    lay = layout(name)
    m = new_model(lay, params(disable_twist=True, monolayer=monolayer))
    k = [0]

    def step():
        m.step(DESCENT_DT, k[0] * DESCENT_DT)
        k[0] += 1
        return m.force, m.velocity, m.center, m.edge_orientation
    return descent_ratios(lay, step, monolayer)
