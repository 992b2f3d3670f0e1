"""The energies of the chain step's soft forces and the RPYC mobility, written from the physics and not from the kernels.

Every force term of the chain step, with its switching states held fixed, is the negative gradient of a scalar that fits
in one line (the table below).  This module states those scalars twice: a scalar form in mpmath at DPS = 50 digits, from
which a test takes -grad U by central differences (exact_forces), and a vectorised numpy.longdouble form, from which the
trajectory test takes U(x) of a whole configuration.  The geometry the energies need (segment - segment distance, signed
point - ellipsoid distance) is written here again, by routes other than the device's and the models': nothing is
imported from a *_model.py, from the oracle or from the package.

    L = |x_j - x_i|, delta = overlap > 0
    Hookean spring, crosslinker, periphery-site tether      1/2 k (L - r)^2
    FENE spring, crosslinker                               -1/2 k r_max^2 ln(1 - (L / r_max)^2),  L < r_max
    active dipole, state on                                -sigma L
    sphere wall                                             1/2 K delta^2,  delta = |x - c| + r - R
    ellipsoid wall, exact route                             1/2 K delta^2,  delta = r + signed distance (negative inside)
    ellipsoid wall, fast route                              K g,  g = sum x_k^2 / (e_k - r)^2 - 1 where g > 0
    sphere - sphere Hertz                                   (8/15) E* sqrt(R*) delta^(5/2)
    segment - segment Hertz                                 the same, delta = r_i + r_j - dist(seg_i, seg_j)
    segment - segment WCA                                   4 eps [(sigma / d)^12 - (sigma / d)^6] + const,  d < cutoff
    end-segment correction                                  the same two laws at d = L of the segment (Hertz: delta = 2 r - L)
    rod element (bend and twist), rod edge (stretch)        see "the discrete rod" below: frames carried by parallel transport
    filament segment - segment Hertz                        the segment Hertz law with the radii of the segments' left nodes

    1 / E* = (1 - nu_i^2) / E_i + (1 - nu_j^2) / E_j        1 / R* = 1 / r_i + 1 / r_j          (contact mechanics)

The mobility rpyc_tt(d, a, b, mu) is the translation - translation Rotne-Prager-Yamakawa tensor of two spheres of
different radii, positive definite for every configuration: Wajnryb, Mizerski, Zuk, Szymczak, J. Fluid Mech. 731, R3
(2013), which derives it, and Zuk, Wajnryb, Mizerski, Szymczak, J. Fluid Mech. 741, R5 (2014), which lists the three
branches of mu^tt_ij for r > a_i + a_j, a_> - a_< < r <= a_i + a_j and r <= a_> - a_<.  (PAPERS.md does not list the two
papers and no copy was at hand when this was written: the expressions below are the well-known ones, the equation
numbers are left for whoever has the papers open.)
    r > a + b              1 / (8 pi mu r) [(1 + (a^2 + b^2) / (3 r^2)) I + (1 - (a^2 + b^2) / r^2) rr]
    |a - b| < r <= a + b   1 / (6 pi mu a b) [(16 r^3 (a + b) - ((a - b)^2 + 3 r^2)^2) / (32 r^3) I
                                              + 3 ((a - b)^2 - r^2)^2 / (32 r^3) rr]
    r <= |a - b|           1 / (6 pi mu max(a, b)) I
    self                   1 / (6 pi mu a) I
with rr the dyad of the unit separation."""
import numpy as np
import mpmath as mp

DPS = 50
LD = np.longdouble


def hp():
    """the working precision of every mpmath form: `with hp(): ...`"""
    return mp.workdps(DPS)


def vec(x):
    """three numbers (float64 or mpf) -> a list of three mpf, exactly"""
    return [mp.mpf(float(v)) if isinstance(v, (float, np.floating, int)) else mp.mpf(v) for v in x]


def sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def norm(a):
    return mp.sqrt(dot(a, a))


# ---- the laws: scalars of one length ---------------------------------------------------------------------------------------
def hookean(L, k, r):
    return k * (L - r) ** 2 / 2


def fene(L, k, r_max):
    """defined for L < r_max only (the caller keeps its inputs inside)"""
    return -k * r_max * r_max * mp.log(1 - (L / r_max) ** 2) / 2


def active(L, sigma):
    return -sigma * L


def effective_modulus(Ei, nui, Ej, nuj):
    return 1 / ((1 - nui * nui) / Ei + (1 - nuj * nuj) / Ej)


def effective_radius(ri, rj):
    return 1 / (1 / ri + 1 / rj)


def hertz(delta, Es, Rs):
    """(8/15) E* sqrt(R*) delta^(5/2) for delta > 0, else 0"""
    if not delta > 0:
        return mp.mpf(0)
    return mp.mpf(8) / 15 * Es * mp.sqrt(Rs) * delta ** (mp.mpf(5) / 2)


def wca(d, epsilon, sigma, cutoff):
    """4 eps [(sigma / d)^12 - (sigma / d)^6] less its value at the cutoff for d < cutoff, else 0.  The constant has no
    gradient; it makes U continuous where a pair enters or leaves the cutoff, which the energy along a trajectory
    needs."""
    if not d < cutoff:
        return mp.mpf(0)
    q, qc = (sigma / d) ** 6, (sigma / cutoff) ** 6
    return 4 * epsilon * ((q * q - q) - (qc * qc - qc))


# ---- geometry -----------------------------------------------------------------------------------------------------------------
def segment_segment(a0, a1, b0, b1):
    """the distance between two segments -> (dist, s, t): the quadratic |a0 + s u - b0 - t v|^2 minimised over the unit
    square by enumerating its faces (the interior stationary point where there is one, then the four edges, each a
    clamped one-dimensional minimum)"""
    u, v, w = sub(a1, a0), sub(b1, b0), sub(a0, b0)
    a, b, c, d, e = dot(u, u), dot(u, v), dot(v, v), dot(u, w), dot(v, w)

    def clamp(q):
        return min(max(q, mp.mpf(0)), mp.mpf(1))

    def d2(s, t):
        p = [w[k] + s * u[k] - t * v[k] for k in range(3)]
        return dot(p, p)

    cand = [(mp.mpf(0), clamp(e / c)), (mp.mpf(1), clamp((e + b) / c)),
            (clamp(-d / a), mp.mpf(0)), (clamp((b - d) / a), mp.mpf(1))]
    det = a * c - b * b
    if det > 0:
        s, t = (b * e - c * d) / det, (a * e - b * d) / det
        if 0 <= s <= 1 and 0 <= t <= 1:
            cand.append((s, t))
    best = min(cand, key=lambda st: d2(*st))
    return mp.sqrt(d2(*best)), best[0], best[1]


def point_ellipsoid(y, e):
    """signed distance (negative inside) of the point y from the ellipsoid sum (x_i / e_i)^2 = 1 in its own frame.
    The closest point is x_i = e_i^2 y_i / (t + e_i^2) with t the largest root of sum (e_i y_i / (t + e_i^2))^2 = 1;
    the sum is convex and decreasing right of its last pole, so Newton from a point where it is >= 0 climbs to the
    root monotonically.  A coordinate y_j = 0 drops out of the sum; the root then holds only while t > -e_j^2, and
    otherwise (a point of a principal plane or axis deep inside) t = -e_j^2 of the shortest such axis and the closest
    point leaves the plane: x_j^2 = e_j^2 (1 - sum_{i != j} (x_i / e_i)^2)."""
    y, e = [abs(v) for v in y], list(e)
    nz = [i for i in range(3) if y[i] != 0]
    zero = [i for i in range(3) if y[i] == 0]
    t = None
    if nz:
        t = max(e[i] * y[i] - e[i] * e[i] for i in nz)   # each single term is >= 1 at its own such t
        hi = mp.sqrt(sum((e[i] * y[i]) ** 2 for i in nz)) - min(e[i] for i in nz) ** 2   # F(hi) <= 0: the bracket
        for _ in range(200):
            F = sum((e[i] * y[i] / (t + e[i] * e[i])) ** 2 for i in nz) - 1
            dF = -2 * sum((e[i] * y[i]) ** 2 / (t + e[i] * e[i]) ** 3 for i in nz)
            step = -F / dF
            t = min(t + step, hi)
            if abs(step) <= mp.mpf(10) ** (-DPS + 4) * (1 + abs(t)):
                break
    leave = [j for j in zero if t is None or t <= -e[j] * e[j]]
    if not leave:
        x = [e[i] * e[i] * y[i] / (t + e[i] * e[i]) if i in nz else mp.mpf(0) for i in range(3)]
        dist = norm(sub(x, y))
        return dist if t > 0 else -dist
    j = min(leave, key=lambda i: e[i])
    x = [mp.mpf(0)] * 3
    for i in nz:
        x[i] = e[i] * e[i] * y[i] / (e[i] * e[i] - e[j] * e[j])
    x[j] = e[j] * mp.sqrt(1 - sum((x[i] / e[i]) ** 2 for i in nz))
    return -norm(sub(x, y))


def rotation(quat):
    """the rotation matrix (3 lists of 3 mpf) of the quaternion (w, x, y, z), normalised here"""
    w, x, y, z = [mp.mpf(float(v)) for v in quat]
    n = mp.sqrt(w * w + x * x + y * y + z * z)
    w, x, y, z = w / n, x / n, y / n, z / n
    return [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
            [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
            [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]


def apply(R, v, transpose=False):
    if transpose:
        return [R[0][k] * v[0] + R[1][k] * v[1] + R[2][k] * v[2] for k in range(3)]
    return [R[k][0] * v[0] + R[k][1] * v[1] + R[k][2] * v[2] for k in range(3)]


def matmul(A, B, transpose_b=False):
    Bt = B if transpose_b else [[B[j][i] for j in range(3)] for i in range(3)]
    return [[dot(A[i], Bt[j]) for j in range(3)] for i in range(3)]


# ---- the walls ------------------------------------------------------------------------------------------------------------------
def sphere_wall(x, c, r, R, K):
    delta = norm(sub(x, c)) + r - R
    return K * delta * delta / 2 if delta > 0 else mp.mpf(0)


def ellipsoid_wall(x, c, rot, e, r, K):
    """rot: the wall's rotation matrix (body -> lab)"""
    delta = r + point_ellipsoid(apply(rot, sub(x, c), transpose=True), e)
    return K * delta * delta / 2 if delta > 0 else mp.mpf(0)


def level_set(x, c, e, r):
    return sum(((x[k] - c[k]) / (e[k] - r)) ** 2 for k in range(3)) - 1


def ellipsoid_wall_fast(x, c, e, r, K):
    g = level_set(x, c, e, r)
    return K * g if g > 0 else mp.mpf(0)


# ---- terms: (bodies, U of their positions, size of the first group) ----------------------------------------------------------
class Term:
    """one energy term: `bodies` (indices), U(list of their positions as mpf triples) -> mpf, and `group`: the term's
    magnitude is |sum of -grad U over the first `group` bodies| (a pair term: the force on its first body; a segment
    pair: the force on its first segment; a wall: the force on the bead)"""

    def __init__(self, bodies, energy, group=1, label=""):
        self.bodies, self.energy, self.group, self.label = tuple(int(b) for b in bodies), energy, group, label


def pair_term(i, j, law, label=""):
    """law(L) -> U"""
    return Term((i, j), lambda p: law(norm(sub(p[1], p[0]))), 1, label)


def tether_term(i, site, law, label=""):
    """a bead tied to a fixed point"""
    return Term((i,), lambda p: law(norm(sub(site, p[0]))), 1, label)


def segment_pair_term(nodes_i, nodes_j, law, label=""):
    """law(dist) -> U between the segments (x[nodes_i[0]], x[nodes_i[1]]) and (x[nodes_j[0]], x[nodes_j[1]])"""
    return Term(tuple(nodes_i) + tuple(nodes_j), lambda p: law(segment_segment(p[0], p[1], p[2], p[3])[0]), 2, label)


def gradient(term, pos, h=None):
    """-grad U of one term at pos (a list of mpf triples, one per body of the term) by central differences with h =
    1e-15 at DPS digits: the truncation error is h^2 U''' / 6 ~ 1e-30, the rounding error 1e-50 / h -> [len(bodies)]
    triples"""
    h = mp.mpf(10) ** -15 if h is None else h
    out = []
    for b in range(len(pos)):
        g = []
        for k in range(3):
            hi = [list(p) for p in pos]
            lo = [list(p) for p in pos]
            hi[b][k] = hi[b][k] + h
            lo[b][k] = lo[b][k] - h
            g.append(-(term.energy(hi) - term.energy(lo)) / (2 * h))
        out.append(g)
    return out


def exact_forces(terms, x, n=None):
    """x: positions (float64 rows or mpf triples) -> (F: n triples of mpf = the sum of -grad U over the terms, S: n mpf
    = for every body the sum of the magnitudes of the terms that act on it, per_term: [(magnitude, [force triples])]).
    Call inside `with hp():`."""
    X = [vec(p) for p in x]
    n = len(X) if n is None else n
    F = [[mp.mpf(0)] * 3 for _ in range(n)]
    S = [mp.mpf(0)] * n
    per_term = []
    for t in terms:
        g = gradient(t, [X[b] for b in t.bodies])
        first = [sum(g[b][k] for b in range(t.group)) for k in range(3)]
        mag = norm(first)
        for gb, b in zip(g, t.bodies):
            F[b] = [F[b][k] + gb[k] for k in range(3)]
        for b in set(t.bodies):
            S[b] = S[b] + mag
        per_term.append((mag, g))
    return F, S, per_term


def to_float(F):
    return np.array([[float(v) for v in row] for row in F], dtype=np.float64).reshape(len(F), -1)


# ---- the discrete rod: frames, curvature, energy ------------------------------------------------------------------------------
# An edge carries a frame as a unit quaternion q = (w, x, y, z), body -> lab.  Between two evaluations the frame follows the
# edge by parallel transport in time: with T and D the edge's tangent and frame at the last evaluation (held fixed), t(x)
# its tangent now and theta its twist,
#       q(x, theta) = PT(T -> t(x)) [cos theta/2, sin theta/2 T] D
# PT(T -> t) = [w, (T x t) / (2 w)], w = sqrt((1 + T.t) / 2), is the rotation about T x t that takes T to t.  The
# curvature of an interior node, in the frame of its left edge, is twice the vector part of conj(q_left) q_right (for a
# rotation by the angle phi about the body-frame axis n: 2 sin(phi / 2) n), and the energy of the element around a node
# of radius r
#       (1 / (2 l0)) dk^T diag(E I, E I, 2 G I) dk,    dk = kappa - rest,  I = pi r^4 / 4,  G = E / (2 (1 + nu))
# An edge of length l stores (1/2) (E pi r^2 / l0) (l - l0)^2 with r the radius of its right node.
def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(p, q):
    return [p[0] * q[0] - p[1] * q[1] - p[2] * q[2] - p[3] * q[3],
            p[0] * q[1] + p[1] * q[0] + p[2] * q[3] - p[3] * q[2],
            p[0] * q[2] - p[1] * q[3] + p[2] * q[0] + p[3] * q[1],
            p[0] * q[3] + p[1] * q[2] - p[2] * q[1] + p[3] * q[0]]


def qconj(q):
    return [q[0], -q[1], -q[2], -q[3]]


def unit_tangent(x0, x1):
    d = sub(x1, x0)
    L = norm(d)
    return [d[0] / L, d[1] / L, d[2] / L]


def transport(T, t):
    """the quaternion of the parallel transport of the unit vector T onto the unit vector t (T.t > -1)"""
    w = mp.sqrt((1 + dot(T, t)) / 2)
    c = cross(T, t)
    return [w, c[0] / (2 * w), c[1] / (2 * w), c[2] / (2 * w)]


def twist_rotation(theta, T):
    """the rotation by theta about the unit vector T"""
    s = mp.sin(theta / 2)
    return [mp.cos(theta / 2), s * T[0], s * T[1], s * T[2]]


def edge_frame(T, t, theta, D):
    return qmul(qmul(transport(T, t), twist_rotation(theta, T)), D)


def curvature(q_left, q_right):
    g = qmul(qconj(q_left), q_right)
    return [2 * g[1], 2 * g[2], 2 * g[3]]


def wave_rest_curvature(rest, amplitude, wave_number, s, frequency, time, phase):
    """the travelling wave replaces component 0 of the rest curvature of the node at arclength s"""
    return [amplitude * mp.sin(wave_number * s + frequency * time + phase), rest[1], rest[2]]


def rod_bend_twist(kappa, rest, r, E, nu, l0):
    I = mp.pi * r ** 4 / 4
    G = E / (2 * (1 + nu))
    dk = sub(kappa, rest)
    return (E * I * (dk[0] * dk[0] + dk[1] * dk[1]) + 2 * G * I * dk[2] * dk[2]) / (2 * l0)


def rod_stretch(L, r_right, E, l0):
    return E * mp.pi * r_right * r_right / l0 * (L - l0) ** 2 / 2


def rod_element(p, theta, T, D, rest, r, E, nu, l0):
    """the energy of the element around p[1]: p = its three nodes, theta, T, D = (left edge, right edge)"""
    ql = edge_frame(T[0], unit_tangent(p[0], p[1]), theta[0], D[0])
    qr = edge_frame(T[1], unit_tangent(p[1], p[2]), theta[1], D[1])
    return rod_bend_twist(curvature(ql, qr), rest, r, E, nu, l0)


def rod_edge(p, r_right, E, l0):
    return rod_stretch(norm(sub(p[1], p[0])), r_right, E, l0)


def rod_gradient(energy, pos, theta, h=None):
    """energy(pos, theta) -> U, pos a list of mpf triples and theta a list of mpf: -(dU/dpos [len(pos)] triples, dU/dtheta
    [len(theta)]) by central differences, as gradient() takes them"""
    h = mp.mpf(10) ** -15 if h is None else h
    gx, gt = [], []
    for b in range(len(pos)):
        g = []
        for k in range(3):
            hi, lo = [list(p) for p in pos], [list(p) for p in pos]
            hi[b][k], lo[b][k] = hi[b][k] + h, lo[b][k] - h
            g.append(-(energy(hi, theta) - energy(lo, theta)) / (2 * h))
        gx.append(g)
    for b in range(len(theta)):
        hi, lo = list(theta), list(theta)
        hi[b], lo[b] = hi[b] + h, lo[b] - h
        gt.append(-(energy(pos, hi) - energy(pos, lo)) / (2 * h))
    return gx, gt


def filament_pair_hertz(a0, a1, b0, b1, ri, rj, E, nu):
    """the frictionless Hertz energy of two filament segments of one material: delta = r_i + r_j less the distance of
    the centrelines; k_n = 4/3 E* of the frictional law is this energy's d^2 U / d delta^2 / sqrt(R* delta)"""
    return hertz(ri + rj - segment_segment(a0, a1, b0, b1)[0], effective_modulus(E, nu, E, nu), effective_radius(ri, rj))


# ---- the mobility ---------------------------------------------------------------------------------------------------------------
def rpyc_branch(r, a, b):
    return "far" if r > a + b else ("overlap" if r > abs(a - b) else "nested")


def rpyc_tt(d, a, b, mu):
    """the 3 x 3 translation - translation mobility (mp.matrix) of spheres of radii a and b at separation d"""
    d = vec(d)
    a, b, mu = mp.mpf(float(a)), mp.mpf(float(b)), mp.mpf(float(mu))
    r = norm(d)
    I = mp.eye(3)
    branch = rpyc_branch(r, a, b)
    if branch == "nested":
        return I / (6 * mp.pi * mu * max(a, b))
    h = mp.matrix([[d[i] * d[j] / (r * r) for j in range(3)] for i in range(3)])
    if branch == "far":
        s = (a * a + b * b) / (r * r)
        return (I * (1 + s / 3) + h * (1 - s)) / (8 * mp.pi * mu * r)
    m = (a - b) ** 2
    ci = (16 * r ** 3 * (a + b) - (m + 3 * r * r) ** 2) / (32 * r ** 3)
    ch = 3 * (m - r * r) ** 2 / (32 * r ** 3)
    return (I * ci + h * ch) / (6 * mp.pi * mu * a * b)


def rpyc_self(a, mu):
    return mp.eye(3) / (6 * mp.pi * mp.mpf(float(mu)) * mp.mpf(float(a)))


def rpyc_matrix(center, radius, mu, self_term=True):
    """the 3n x 3n mobility as rows of mpf (a list of lists)"""
    n = len(radius)
    M = [[mp.mpf(0)] * (3 * n) for _ in range(3 * n)]
    for t in range(n):
        for s in range(n):
            if s == t:
                blk = rpyc_self(radius[t], mu) if self_term else mp.zeros(3)
            else:
                blk = rpyc_tt([mp.mpf(float(center[t][k])) - mp.mpf(float(center[s][k])) for k in range(3)], radius[s],
                              radius[t], mu)
            for i in range(3):
                for j in range(3):
                    M[3 * t + i][3 * s + j] = blk[i, j]
    return M


# ---- numpy.longdouble forms, vectorised over the leading axis ----------------------------------------------------------------
def _ld(a):
    return np.asarray(a, dtype=LD)


def ld_norm(d):
    return np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])


def ld_hookean(L, k, r):
    return _ld(k) * (_ld(L) - _ld(r)) ** 2 / LD(2)


def ld_fene(L, k, r_max):
    L, k, r_max = _ld(L), _ld(k), _ld(r_max)
    return -k * r_max * r_max * np.log1p(-(L / r_max) ** 2) / LD(2)


def ld_active(L, sigma):
    return -_ld(sigma) * _ld(L)


def ld_effective_modulus(Ei, nui, Ej, nuj):
    Ei, nui, Ej, nuj = _ld(Ei), _ld(nui), _ld(Ej), _ld(nuj)
    return LD(1) / ((LD(1) - nui * nui) / Ei + (LD(1) - nuj * nuj) / Ej)


def ld_effective_radius(ri, rj):
    return LD(1) / (LD(1) / _ld(ri) + LD(1) / _ld(rj))


def ld_hertz(delta, Es, Rs):
    delta = _ld(delta)
    pos = np.where(delta > 0, delta, LD(0))
    return LD(8) / LD(15) * _ld(Es) * np.sqrt(_ld(Rs)) * (pos * pos * np.sqrt(pos))


def ld_wca(d, epsilon, sigma, cutoff):
    d = _ld(d)
    q, qc = (_ld(sigma) / d) ** 6, (_ld(sigma) / _ld(cutoff)) ** 6
    return np.where(d < _ld(cutoff), LD(4) * _ld(epsilon) * ((q * q - q) - (qc * qc - qc)), LD(0))


def ld_segment_segment(a0, a1, b0, b1, want_parameters=False):
    """distances [c] of segment pairs [c, 3] x 4: the same enumeration of the faces of the unit square; with
    want_parameters -> (dist, s, t)"""
    a0, a1, b0, b1 = _ld(a0), _ld(a1), _ld(b0), _ld(b1)
    u, v, w = a1 - a0, b1 - b0, a0 - b0
    vd = lambda p, q: p[..., 0] * q[..., 0] + p[..., 1] * q[..., 1] + p[..., 2] * q[..., 2]  # noqa: E731
    a, b, c, d, e = vd(u, u), vd(u, v), vd(v, v), vd(u, w), vd(v, w)
    clamp = lambda q: np.minimum(np.maximum(q, LD(0)), LD(1))  # noqa: E731

    def d2(s, t):
        p = w + s[..., None] * u - t[..., None] * v
        return vd(p, p)

    zero, one = np.zeros_like(a), np.ones_like(a)
    det = a * c - b * b
    with np.errstate(all="ignore"):
        s, t = (b * e - c * d) / det, (a * e - b * d) / det
        ok = (det > 0) & (s >= 0) & (s <= 1) & (t >= 0) & (t <= 1)
    cand = [(zero, clamp(e / c)), (one, clamp((e + b) / c)), (clamp(-d / a), zero), (clamp((b - d) / a), one),
            (np.where(ok, s, zero), np.where(ok, t, clamp(e / c)))]   # (no interior point: the first edge again)
    D = np.stack([d2(s_, t_) for s_, t_ in cand])
    pick = np.argmin(D, axis=0)[None]
    best = np.take_along_axis(D, pick, axis=0)[0]
    if want_parameters:
        S, T = np.stack([c_[0] for c_ in cand]), np.stack([c_[1] for c_ in cand])
        return np.sqrt(best), np.take_along_axis(S, pick, axis=0)[0], np.take_along_axis(T, pick, axis=0)[0]
    return np.sqrt(best)


def ld_point_ellipsoid(y, e):
    """signed distances [n] of body-frame points y [n, 3] from the ellipsoid with semi-axes e [3]; point_ellipsoid's
    route with a fixed number of Newton steps"""
    y, e = np.abs(_ld(y)), _ld(e)
    n = y.shape[0]
    e2 = e * e
    nzm = y != 0
    big = LD(-1e300)
    with np.errstate(all="ignore"):
        t = np.max(np.where(nzm, e * y - e2, big), axis=1)
        hi = np.sqrt(np.sum(np.where(nzm, (e * y) ** 2, LD(0)), axis=1)) - np.min(np.where(nzm, e2, LD(1e300)), axis=1)
        for _ in range(80):
            den = t[:, None] + e2
            F = np.sum(np.where(nzm, (e * y / den) ** 2, LD(0)), axis=1) - LD(1)
            dF = -LD(2) * np.sum(np.where(nzm, (e * y) ** 2 / den ** 3, LD(0)), axis=1)
            step = np.where(dF != 0, -F / dF, LD(0))
            t = np.where(np.isfinite(step), np.minimum(t + step, hi), t)
        has = nzm.any(axis=1)
        leave = ~nzm & (~has[:, None] | (t[:, None] <= -e2))
        out = np.empty(n, dtype=LD)
        x = np.where(nzm, e2 * y / (t[:, None] + e2), LD(0))
        dist = ld_norm(x - y)
        out[:] = np.where(t > 0, dist, -dist)
        for row in np.flatnonzero(leave.any(axis=1)):
            j = min(np.flatnonzero(leave[row]), key=lambda i: e[i])
            xr = np.where(nzm[row], e2 * y[row] / (e2 - e2[j]), LD(0))
            xr[j] = e[j] * np.sqrt(LD(1) - np.sum(np.where(nzm[row], (xr / e) ** 2, LD(0))))
            out[row] = -ld_norm(xr - y[row])
    return out


def ld_rotation(quat):
    q = _ld(quat)
    w, x, y, z = q / np.sqrt(np.sum(q * q))
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], dtype=LD)


def ld_sphere_wall(x, c, r, R, K):
    delta = ld_norm(_ld(x) - _ld(c)) + _ld(r) - _ld(R)
    return np.where(delta > 0, _ld(K) * delta * delta / LD(2), LD(0))


def ld_ellipsoid_wall(x, c, quat, e, r, K):
    body = (_ld(x) - _ld(c)) @ ld_rotation(quat)   # rows: R^T (x - c)
    delta = _ld(r) + ld_point_ellipsoid(body, e)
    return np.where(delta > 0, _ld(K) * delta * delta / LD(2), LD(0))


def ld_ellipsoid_wall_fast(x, c, e, r, K):
    g = np.sum(((_ld(x) - _ld(c)) / (_ld(e)[None, :] - _ld(r)[:, None])) ** 2, axis=1) - LD(1)
    return np.where(g > 0, _ld(K) * g, LD(0))


def ld_spring_energy(x, pairs, kind, k, r):
    x, p = _ld(x), np.asarray(pairs).reshape(-1, 2)
    L = ld_norm(x[p[:, 1]] - x[p[:, 0]])
    return (ld_hookean if kind == "hookean" else ld_fene)(L, k, r).sum()


def ld_sphere_hertz_energy(x, radius, E, nu, reach=0.0):
    """all pairs i < j of the spheres"""
    x, radius = _ld(x), _ld(radius)
    n = x.shape[0]
    i, j = np.triu_indices(n, 1)
    near = np.linalg.norm(np.asarray(x[i] - x[j], dtype=np.float64), axis=1) < np.asarray(radius[i] + radius[j],
                                                                                          dtype=np.float64) + 1e-6
    i, j = i[near], j[near]
    delta = radius[i] + radius[j] - ld_norm(x[j] - x[i])
    return ld_hertz(delta, ld_effective_modulus(E, nu, E, nu), ld_effective_radius(radius[i], radius[j])).sum()


def ld_backbone_energy(x, ends, kind, radius, end_correction, E=1000.0, nu=0.3, epsilon=1.0, sigma=1.0,
                       cutoff=1.12246204831):
    """every pair of segments that share no node, plus the end-segment correction of the segments flagged"""
    x, ends = _ld(x), np.asarray(ends).reshape(-1, 2)
    m = ends.shape[0]
    radius = np.broadcast_to(_ld(radius), (m,))
    i, j = np.triu_indices(m, 1)
    share = (ends[i, 0] == ends[j, 0]) | (ends[i, 0] == ends[j, 1]) | (ends[i, 1] == ends[j, 0]) | (ends[i, 1] == ends[j, 1])
    mid = np.asarray(x[ends[:, 0]] + x[ends[:, 1]], dtype=np.float64) * 0.5
    half = 0.5 * np.linalg.norm(np.asarray(x[ends[:, 1]] - x[ends[:, 0]], dtype=np.float64), axis=1)
    reach = (np.asarray(radius[i] + radius[j], dtype=np.float64) if kind == "hertz" else float(cutoff)) + 1e-6
    near = ~share & (np.linalg.norm(mid[i] - mid[j], axis=1) < half[i] + half[j] + reach)
    i, j = i[near], j[near]
    d = ld_segment_segment(x[ends[i, 0]], x[ends[i, 1]], x[ends[j, 0]], x[ends[j, 1]])
    Es = ld_effective_modulus(E, nu, E, nu)
    if kind == "hertz":
        U = ld_hertz(radius[i] + radius[j] - d, Es, ld_effective_radius(radius[i], radius[j])).sum()
    else:
        U = ld_wca(d, epsilon, sigma, cutoff).sum()
    c = np.flatnonzero(np.asarray(end_correction))
    if c.size:
        L = ld_norm(x[ends[c, 1]] - x[ends[c, 0]])
        if kind == "hertz":
            U = U + ld_hertz(LD(2) * radius[c] - L, Es, ld_effective_radius(radius[c], radius[c])).sum()
        else:
            U = U + ld_wca(L, epsilon, sigma, cutoff).sum()
    return U


# ---- the discrete rod in longdouble, one row per edge or element ----------------------------------------------------------------
def ld_cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def ld_dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def ld_qmul(p, q):
    return np.stack([p[..., 0] * q[..., 0] - p[..., 1] * q[..., 1] - p[..., 2] * q[..., 2] - p[..., 3] * q[..., 3],
                     p[..., 0] * q[..., 1] + p[..., 1] * q[..., 0] + p[..., 2] * q[..., 3] - p[..., 3] * q[..., 2],
                     p[..., 0] * q[..., 2] - p[..., 1] * q[..., 3] + p[..., 2] * q[..., 0] + p[..., 3] * q[..., 1],
                     p[..., 0] * q[..., 3] + p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1] + p[..., 3] * q[..., 0]], axis=-1)


def ld_qconj(q):
    return q * np.array([1, -1, -1, -1], dtype=LD)


def ld_unit_tangent(x0, x1):
    d = _ld(x1) - _ld(x0)
    return d / ld_norm(d)[..., None]


def ld_transport(T, t):
    T, t = _ld(T), _ld(t)
    w = np.sqrt((LD(1) + ld_dot(T, t)) / LD(2))
    return np.concatenate([w[..., None], ld_cross(T, t) / (LD(2) * w)[..., None]], axis=-1)


def ld_twist_rotation(theta, T):
    half = _ld(theta) / LD(2)
    return np.concatenate([np.cos(half)[..., None], np.sin(half)[..., None] * _ld(T)], axis=-1)


def ld_edge_frame(T, t, theta, D):
    return ld_qmul(ld_qmul(ld_transport(T, t), ld_twist_rotation(theta, T)), _ld(D))


def ld_curvature(q_left, q_right):
    return LD(2) * ld_qmul(ld_qconj(_ld(q_left)), _ld(q_right))[..., 1:]


def ld_wave_rest_curvature(rest, amplitude, wave_number, s, frequency, time, phase):
    out = _ld(rest).copy()
    out[..., 0] = _ld(amplitude) * np.sin(_ld(wave_number) * _ld(s) + _ld(frequency) * _ld(time) + _ld(phase))
    return out


def ld_rod_bend_twist(kappa, rest, r, E, nu, l0):
    r, E, nu, l0 = _ld(r), _ld(E), _ld(nu), _ld(l0)
    I = np.arctan(LD(1)) * r ** 4   # pi / 4 = atan(1), in longdouble
    G = E / (LD(2) * (LD(1) + nu))
    dk = _ld(kappa) - _ld(rest)
    return (E * I * (dk[..., 0] * dk[..., 0] + dk[..., 1] * dk[..., 1]) + LD(2) * G * I * dk[..., 2] * dk[..., 2]) / (LD(2) * l0)


def ld_rod_stretch(L, r_right, E, l0):
    r, l0 = _ld(r_right), _ld(l0)
    return _ld(E) * (LD(4) * np.arctan(LD(1))) * r * r / l0 * (_ld(L) - l0) ** 2 / LD(2)


def ld_filament_pair_hertz(a0, a1, b0, b1, ri, rj, E, nu):
    d = ld_segment_segment(a0, a1, b0, b1)
    return ld_hertz(_ld(ri) + _ld(rj) - d, ld_effective_modulus(E, nu, E, nu), ld_effective_radius(ri, rj))


def ld_rod_energy(node_ptr, x, q, radius, rest, E, nu, l0):
    """the energy of filaments from their centres x [n, 3] and edge frames q [n, 4] (row e: the edge e -> e + 1; the row
    of a filament's last node is not read) -> (per interior node [n], per edge [n]), zero in the rows that have neither"""
    node_ptr = np.asarray(node_ptr)
    n = int(node_ptr[-1])
    x, q = _ld(x), _ld(q)
    has_r, has_l = np.ones(n, bool), np.ones(n, bool)
    has_r[node_ptr[1:] - 1], has_l[node_ptr[:-1]] = False, False
    inner = np.flatnonzero(has_r & has_l)
    edge = np.flatnonzero(has_r)
    bend, stretch = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    bend[inner] = ld_rod_bend_twist(ld_curvature(q[inner - 1], q[inner]), _ld(rest)[inner], _ld(radius)[inner], E, nu, l0)
    stretch[edge] = ld_rod_stretch(ld_norm(x[edge + 1] - x[edge]), _ld(radius)[edge + 1], E, l0)
    return bend, stretch
