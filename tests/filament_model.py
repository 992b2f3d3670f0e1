"""numpy restatement of the centerline-twist filament step (filament.hip), written from the reference text
(CollidingOverdampedFrictionalSperm.cpp:1095-1509, :1733-1862, :1999-2010) in the operations and order
include/mundy_hip.h documents: every float expression below rounds like the device code (numpy never contracts a
product and a sum, the device build does not either), sine and cosine come from the oracle's shared_sincos (the device's
fixed IEEE sequence).  Vectors are kept as tuples of component arrays so that every sum's association is in the text:
dot(a, b) = a0 b0 + (a1 b1 + a2 b2), |a| = sqrt(x*x + (y*y + z*z))."""
import math
from dataclasses import dataclass

import numpy as np

PI = math.pi


@dataclass
class Params:
    E: float = 10.0
    nu: float = 0.3
    l0: float = 1.0
    eta: float = 1.0
    A: float = 0.0       # wave amplitude
    k: float = 0.0       # spatial frequency 2 pi / wavelength
    omega: float = 0.0   # temporal frequency 2 pi / period
    wave: bool = False
    disable_twist: bool = False
    monolayer: bool = False


def _sincos(x):
    import oracle
    oracle.build()
    return oracle.shared_sincos(x)


# ---- vectors and quaternions as tuples of component arrays (mhip_internal.hpp) ----------------------------------------
def _v(a):
    a = np.asarray(a, dtype=np.float64)
    return tuple(a[:, c].copy() for c in range(a.shape[1]))


def _arr(t):
    return np.stack(t, axis=1)


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _scale(s, a):
    return tuple(s * x for x in a)


def _dot(a, b):
    return a[0] * b[0] + (a[1] * b[1] + a[2] * b[2])


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _qmul(q, o):
    return (q[0] * o[0] - q[1] * o[1] - q[2] * o[2] - q[3] * o[3],
            q[0] * o[1] + q[1] * o[0] + q[2] * o[3] - q[3] * o[2],
            q[0] * o[2] - q[1] * o[3] + q[2] * o[0] + q[3] * o[1],
            q[0] * o[3] + q[1] * o[2] - q[2] * o[1] + q[3] * o[0])


def _qrot(q, v):
    inv = 1.0 / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    qi = (q[0] * inv, -q[1] * inv, -q[2] * inv, -q[3] * inv)
    r = _qmul(_qmul(q, (np.zeros_like(v[0]), v[0], v[1], v[2])), qi)
    return (r[1], r[2], r[3])


def _shift(t, by):
    """component arrays moved by `by` rows: out[i] = in[i - by] (the rows that fall off are never used)"""
    return tuple(np.roll(x, by) for x in t)


# ---- the state ---------------------------------------------------------------------------------------------------------
class Filaments:
    """F filaments over N nodes; the fields of mhip_filament_fields as numpy arrays"""

    def __init__(self, node_ptr, radius, rest_curvature, arclength, phase=None, params=None, sincos=None):
        self.prm = params or Params()
        self.node_ptr = np.asarray(node_ptr, dtype=np.int64)
        n = self.n = int(self.node_ptr[-1])
        self.num_filaments = len(self.node_ptr) - 1
        self.radius = np.array(radius, dtype=np.float64)
        self.rest_curvature = np.array(rest_curvature, dtype=np.float64).reshape(n, 3)
        self.arclength = np.array(arclength, dtype=np.float64)
        self.phase = np.zeros(self.num_filaments) if phase is None else np.array(phase, dtype=np.float64)
        self.sincos = sincos or _sincos
        count = np.diff(self.node_ptr)
        assert (count >= 2).all()
        self.fid = np.repeat(np.arange(self.num_filaments), count)
        first, last = np.zeros(n, bool), np.zeros(n, bool)
        first[self.node_ptr[:-1]] = True
        last[self.node_ptr[1:] - 1] = True
        self.has_l, self.has_r = ~first, ~last
        self.interior = self.has_l & self.has_r
        self.elem_l = self.has_l & np.roll(self.interior, 1)    # element i - 1 exists
        self.elem_r = self.has_r & np.roll(self.interior, -1)   # element i + 1 exists

    def set_state(self, center, twist, edge_orientation):
        n = self.n
        self.center = np.array(center, dtype=np.float64).reshape(n, 3)
        self.twist = np.array(twist, dtype=np.float64)
        self.velocity, self.force, self.curvature = (np.zeros((n, 3)) for _ in range(3))
        self.twist_velocity, self.twist_torque = np.zeros(n), np.zeros(n)
        e = self.has_r
        x = _v(self.center)
        with np.errstate(all="ignore"):
            d = _sub(_shift(x, -1), x)
            l = np.sqrt(_dot(d, d))
            t = _arr((d[0] / l, d[1] / l, d[2] / l))
        self.edge_tangent = np.where(e[:, None], t, 0.0)
        self.edge_length = np.where(e, l, 0.0)
        self.edge_orientation = np.array(edge_orientation, dtype=np.float64).reshape(n, 4)
        self.edge_binormal = np.zeros((n, 3))
        self.edge_tangent_old, self.edge_length_old = self.edge_tangent.copy(), self.edge_length.copy()
        self.edge_orientation_old, self.edge_binormal_old = self.edge_orientation.copy(), self.edge_binormal.copy()
        return self

    # ---- :1999-2010 ----------------------------------------------------------------------------------------------------
    def advance(self, dt):
        p = self.prm
        if p.disable_twist:
            self.twist[:] = 0.0
            self.twist_velocity[:] = 0.0
        if p.monolayer:
            self.center[:, 0] = 0.0
            self.velocity[:, 0] = 0.0
        for name in ("edge_tangent", "edge_orientation", "edge_length", "edge_binormal"):
            new, old = getattr(self, name), getattr(self, name + "_old")
            setattr(self, name, old)
            setattr(self, name + "_old", new)
        self.center = self.center + dt * self.velocity
        self.twist = self.twist + dt * self.twist_velocity
        self.velocity = np.zeros_like(self.velocity)
        self.force = np.zeros_like(self.force)
        self.twist_velocity = np.zeros_like(self.twist_velocity)
        self.twist_torque = np.zeros_like(self.twist_torque)

    # ---- compute_edge_information, :1223-1240 ----------------------------------------------------------------------------
    def edge_pass(self):
        e = self.has_r
        x = _v(self.center)
        to, qo = _v(self.edge_tangent_old), _v(self.edge_orientation_old)
        with np.errstate(all="ignore"):
            d = _sub(_shift(x, -1), x)
            l = np.sqrt(_dot(d, d))
            t = (d[0] / l, d[1] / l, d[2] / l)
            c = _cross(to, t)
            tt = _dot(to, t)
            ib = 1.0 / (1.0 + tt)
            b = tuple((2.0 * ck) * ib for ck in c)
            sh, ch = self.sincos(0.5 * self.twist)
            rot_twist = (ch, sh * to[0], sh * to[1], sh * to[2])
            w = np.sqrt(0.5 * (1.0 + tt))
            iw = 1.0 / w
            rot_pt = (w, (0.5 * c[0]) * iw, (0.5 * c[1]) * iw, (0.5 * c[2]) * iw)
            q = _qmul(_qmul(rot_pt, rot_twist), qo)
        # the slot of a filament's last node keeps what it held
        self.edge_tangent = np.where(e[:, None], _arr(t), self.edge_tangent)
        self.edge_binormal = np.where(e[:, None], _arr(b), self.edge_binormal)
        self.edge_length = np.where(e, l, self.edge_length)
        self.edge_orientation = np.where(e[:, None], _arr(q), self.edge_orientation)

    # ---- :1166-1167, :1315-1316, :1411-1458, :1490-1504 -------------------------------------------------------------------
    def node_pass(self, time, external_force=None):
        p = self.prm
        E, nu, l0 = np.float64(p.E), np.float64(p.nu), np.float64(p.l0)
        t, b, l, q = _v(self.edge_tangent), _v(self.edge_binormal), self.edge_length, _v(self.edge_orientation)
        tl, bl, ll, ql = _shift(t, 1), _shift(b, 1), np.roll(l, 1), _shift(q, 1)   # edge i - 1 at row i
        r = self.radius
        inner = self.interior
        with np.errstate(all="ignore"):
            rest = list(_v(self.rest_curvature))
            if p.wave:
                wt = np.float64(p.omega) * np.float64(time)
                sn, _ = self.sincos(np.float64(p.k) * self.arclength + wt + self.phase[self.fid])
                rest[0] = np.float64(p.A) * sn
            g = _qmul((ql[0], -ql[1], -ql[2], -ql[3]), q)
            kappa = (2.0 * g[1], 2.0 * g[2], 2.0 * g[3])
            dk = _sub(kappa, rest)
            inertia = 0.25 * PI * r * r * r * r
            shear = 0.5 * E / (1.0 + nu)
            il = 1.0 / l0
            bt = (-il * E * inertia * dk[0], -il * E * inertia * dk[1], -il * 2 * shear * inertia * dk[2])
            gv = (g[1], g[2], g[3])
            m = _qrot(ql, _add(_scale(g[0], bt), _cross(gv, bt)))
            # tmp_force_ip1 with the element's right edge (edge i), tmp_force_im1 with its left edge (edge i - 1)
            fr = _scale(1.0 / l, _sub(_add(_cross(m, t), _scale(0.5 * _dot(t, m), _scale(_dot(t, b), t))), b))
            fl = _scale(1.0 / ll, _add(_cross(m, tl), _scale(0.5 * _dot(tl, m), _sub(_scale(_dot(tl, bl), tl), bl))))
            tq_c = _dot(t, m)      # on node i from element i
            tq_l = _dot(tl, m)     # taken off node i - 1 by element i
            # stretch of edge e, radius of its right node
            ks = E * PI * np.roll(r, -1) * np.roll(r, -1) / l0
            fs = _scale(-ks * (l - l0), t)
            stretch = np.abs(l - l0) / l0
        n = self.n
        f = np.zeros((n, 3)) if external_force is None else np.array(external_force, dtype=np.float64).reshape(n, 3)
        fr, fl, fs = _arr(fr), _arr(fl), _arr(fs)
        k = self.elem_l
        f[k] = f[k] + np.roll(fr, 1, axis=0)[k]
        k = inner
        f[k] = f[k] - (fr[k] + fl[k])
        k = self.elem_r
        f[k] = f[k] + np.roll(fl, -1, axis=0)[k]
        k = self.has_l
        f[k] = f[k] + np.roll(fs, 1, axis=0)[k]
        k = self.has_r
        f[k] = f[k] - fs[k]
        tq = np.zeros(n)
        k = inner
        tq[k] = tq[k] + tq_c[k]
        k = self.elem_r
        tq[k] = tq[k] - np.roll(tq_l, -1)[k]
        self.force, self.twist_torque = f, tq
        self.terms = dict(fr=fr, fl=fl, fs=fs, m=_arr(m))   # per element (rows of interior nodes) and per edge
        self.curvature = np.where(inner[:, None], _arr(kappa), self.curvature)
        dev = np.abs(_arr(dk))[inner]
        max_stretch = float(stretch[self.has_r].max()) if self.has_r.any() else 0.0
        max_dk = float(dev.max()) if dev.size else 0.0
        return max_stretch, max_dk

    def compute_force(self, time, external_force=None):
        """-> (largest |l - l0| / l0, largest |kappa - rest| component)"""
        self.edge_pass()
        return self.node_pass(time, external_force)

    # ---- :1755-1775 --------------------------------------------------------------------------------------------------------
    def compute_velocity(self):
        eta = np.float64(self.prm.eta)
        c6, c8 = 1.0 / (6.0 * PI * eta), 1.0 / (8.0 * PI * eta)
        ir = 1.0 / self.radius
        ir3 = ir * ir * ir
        self.velocity = (c6 * ir)[:, None] * self.force
        self.twist_velocity = (c8 * ir3) * self.twist_torque

    def step(self, dt, time, external_force=None):
        """one pass of the reference's loop body: advance -> forces at x(t + dt) -> velocities"""
        self.advance(dt)
        stats = self.compute_force(time, external_force)
        self.compute_velocity()
        return stats


# ---- the initial triad (:1057-1068) ---------------------------------------------------------------------------------------
def triad_orientation(tangent, flip=False):
    """the quaternion (w, x, y, z) of the rotation matrix with the columns d1 = (+-1, 0, 0), d2 = d3 x d1 / |.|, d3 = t
    (rotation_matrix_to_quaternion, mundy_math/Quaternion.hpp:1410-1427)"""
    t = np.asarray(tangent, dtype=np.float64)
    d1 = np.array([-1.0 if flip else 1.0, 0.0, 0.0])
    d2 = np.cross(t, d1)
    d2 = d2 / math.sqrt(d2[0] * d2[0] + (d2[1] * d2[1] + d2[2] * d2[2]))
    D = np.stack([d1, d2, t], axis=1)
    half = lambda v: math.sqrt(max(0.0, v)) / 2.0  # noqa: E731
    return np.array([half(1.0 + D[0, 0] + D[1, 1] + D[2, 2]),
                     math.copysign(half(1.0 + D[0, 0] - D[1, 1] - D[2, 2]), D[2, 1] - D[1, 2]),
                     math.copysign(half(1.0 - D[0, 0] + D[1, 1] - D[2, 2]), D[0, 2] - D[2, 0]),
                     math.copysign(half(1.0 - D[0, 0] - D[1, 1] + D[2, 2]), D[1, 0] - D[0, 1])])
