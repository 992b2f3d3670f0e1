"""numpy restatement of the inertial filament step (k_filament_predict, k_filament_correct and the kinetic energy of
filament.hip; the frictionless law of filament_contact.hip), written from the reference text over
filament_model.Filaments and filament_contact_model.Contacts in the operations and order
include/mundy_hip_filament_inertial.h documents:
  predict        CollidingFrictionalSperm.cpp:1699-1706 (disable_twist), :1708-1737 (apply_monolayer), rotate_field_states,
                 :968-1018 (update_generalized_position), in the order of the loop :1902-1921
  correct        :1616-1672 (update_generalized_position_velocity_and_acceleration), CollidingSperm.cpp:1563-1595
  kinetic energy :1739-1779, per node; the total is math.fsum of the terms (the device's sum is correctly rounded)
  equilibrate    :1781-1865
  Hertz law      .../evaluate_linker_potentials/kernels/SpherocylinderSegmentSpherocylinderSegmentHertzianContact.cpp:208-225
Every float expression rounds like the device code: numpy never contracts, the device build does not either."""
import math

import numpy as np

import filament_contact_model as fcm
import filament_model as fm

PI = math.pi
BETA, GAMMA = 0.25, 0.5


class InertialFilaments(fm.Filaments):
    """fm.Filaments with mass: acceleration [N, 3] and twist_acceleration [N] beside its fields"""

    def set_inertial(self, density, damping="critical", fixed_filaments=None):
        self.density = np.float64(density)
        self.damping = damping
        self.fixed = np.zeros(self.n, bool)
        if fixed_filaments is not None:
            self.fixed = np.asarray(fixed_filaments, bool)[self.fid]
        return self

    def set_state(self, center, twist, edge_orientation):
        super().set_state(center, twist, edge_orientation)
        self.acceleration, self.twist_acceleration = np.zeros((self.n, 3)), np.zeros(self.n)
        return self

    def set_motion(self, velocity=None, twist_velocity=None, acceleration=None, twist_acceleration=None):
        n = self.n
        z3, z1 = np.zeros((n, 3)), np.zeros(n)
        self.velocity = z3.copy() if velocity is None else np.array(velocity, dtype=np.float64).reshape(n, 3)
        self.twist_velocity = z1.copy() if twist_velocity is None else np.array(twist_velocity, dtype=np.float64)
        self.acceleration = z3.copy() if acceleration is None else np.array(acceleration, dtype=np.float64).reshape(n, 3)
        self.twist_acceleration = (z1.copy() if twist_acceleration is None
                                   else np.array(twist_acceleration, dtype=np.float64))

    # ---- :1902-1921 ------------------------------------------------------------------------------------------------------
    def predict(self, dt):
        p = self.prm
        dt = np.float64(dt)
        if p.disable_twist:                                            # :1703-1705
            self.twist = np.zeros(self.n)
            self.twist_velocity = np.zeros(self.n)
            self.twist_acceleration = np.zeros(self.n)
        if p.monolayer:                                                # :1733-1735
            self.center[:, 0] = 0.0
            self.velocity[:, 0] = 0.0
            self.acceleration[:, 0] = 0.0
        for name in ("edge_tangent", "edge_orientation", "edge_length", "edge_binormal"):   # rotate_field_states
            new, old = getattr(self, name), getattr(self, name + "_old")
            setattr(self, name, old)
            setattr(self, name + "_old", new)
        coeff = 0.5 * dt * dt * (1.0 - 2.0 * BETA)                     # :1013
        self.center = (self.center + dt * self.velocity) + coeff * self.acceleration                  # :1014
        self.twist = (self.twist + dt * self.twist_velocity) + coeff * self.twist_acceleration       # :1015-1016

    def mass(self):
        """-> (m, I) per node, :1633-1636"""
        r = self.radius
        r2 = r * r
        r3 = r2 * r
        m = 4.0 / 3.0 * PI * r3 * self.density
        return m, 2.0 / 5.0 * m * r2

    # ---- :1616-1672 ------------------------------------------------------------------------------------------------------
    def correct(self, dt):
        """-> the kinetic energy of the velocities written (math.fsum of kinetic_terms())"""
        dt = np.float64(dt)
        m, I = self.mass()
        if isinstance(self.damping, str):                               # :1645-1646
            ct = np.sqrt(m * np.float64(self.prm.E))
            cr = ct
        else:                                                           # CollidingSperm.cpp:1576-1577
            ct = np.full(self.n, np.float64(self.damping[0]))
            cr = np.full(self.n, np.float64(self.damping[1]))
        v, a, tv, ta = self.velocity, self.acceleration, self.twist_velocity, self.twist_acceleration
        c1 = (1.0 - GAMMA) * dt                                         # :1647
        pv = v + c1 * a                                                 # :1648
        ptv = tv + c1 * ta                                              # :1649
        with np.errstate(all="ignore"):
            an = (1.0 / m)[:, None] * (self.force - ct[:, None] * v)    # :1658
            tan = 1.0 / I * (self.twist_torque - cr * tv)               # :1659-1660
            c2 = dt * dt * BETA                                         # :1665
            x = self.center + c2 * an                                   # :1666
            tw = self.twist + c2 * tan                                  # :1667
            c3 = dt * GAMMA                                             # :1669
            vn = pv + c3 * an                                           # :1670
            tvn = ptv + c3 * tan                                        # :1671
        fx = self.fixed                                                 # :1652-1656
        self.acceleration = np.where(fx[:, None], 0.0, an)
        self.twist_acceleration = np.where(fx, 0.0, tan)
        self.velocity = np.where(fx[:, None], 0.0, vn)
        self.twist_velocity = np.where(fx, 0.0, tvn)
        self.center = np.where(fx[:, None], self.center, x)
        self.twist = np.where(fx, self.twist, tw)
        return self.kinetic_energy()

    # ---- :1739-1779 ------------------------------------------------------------------------------------------------------
    def kinetic_terms(self):
        m, I = self.mass()
        v = fm._v(self.velocity)
        w = self.twist_velocity
        return 0.5 * m * fm._dot(v, v) + 0.5 * I * w * w                # :1767-1769

    def kinetic_energy(self):
        return math.fsum(self.kinetic_terms())

    def step(self, dt, time, external_force=None):
        """one pass of the loop body :1902-1947 -> (statistics of the force evaluation, kinetic energy)"""
        self.predict(dt)
        stats = self.compute_force(time, external_force)
        return stats, self.correct(dt)


def ramp_levels(relaxed, normal, growth=1.1):
    """the moduli the reference's loop visits (:1800-1863): repeated `*= growth` in floating point"""
    out, E = [], float(relaxed)
    while E < float(normal):
        out.append(E)
        E *= float(growth)
    return out


def equilibrate(model, dt, time, relaxed, threshold=1e-6, growth=1.1, poll_every=1, max_steps=1000000):
    """:1781-1865 on the model -> the steps per level; the model's modulus is its own again on return"""
    normal = model.prm.E
    levels, total = [], 0
    try:
        for E in ramp_levels(relaxed, normal, growth):
            model.prm.E = E
            count, energy = 0, float("inf")
            while energy > threshold:
                if total + poll_every > max_steps:
                    raise RuntimeError("equilibrate: max_steps")
                for _ in range(poll_every):
                    _, energy = model.step(dt, time)
                count += poll_every
                total += poll_every
            levels.append(count)
    finally:
        model.prm.E = normal
    return levels


# ---- the frictionless law over filament_contact_model.Contacts --------------------------------------------------------------
def reduce_rows(contacts, force, share, external_force=None):
    """the reduction of filament_contact_model.Contacts.force_pass over given rows -> node_force"""
    n, p = contacts.n, contacts.pairs
    A0, A1 = np.zeros((n, 3)), np.zeros((n, 3))
    Fs = np.stack([force, -force], axis=1)
    np.add.at(A0, p.reshape(-1), (Fs - share).reshape(-1, 3))
    np.add.at(A1, p.reshape(-1), share.reshape(-1, 3))
    f = np.zeros((n, 3)) if external_force is None else np.array(external_force, dtype=np.float64).reshape(n, 3)
    hr = contacts.f.has_r
    hl = np.concatenate([[False], hr[:-1]])
    f[hr] = f[hr] + A0[hr]
    f[hl] = f[hl] + np.roll(A1, 1, axis=0)[hl]
    return f


class HertzContacts(fcm.Contacts):
    """fcm.Contacts under the frictionless law: no velocity is read, tang_disp stays +0.0, nothing is counted"""

    def __init__(self, filaments, skin, youngs_modulus, poisson_ratio, mu=0.0, damping=(0.0, 0.0), density=1.0,
                 segment_radius=None, history_dt=None, bonded_exclusion=1, law="hertz"):
        assert law == "hertz"
        super().__init__(filaments, skin, youngs_modulus, poisson_ratio, mu, damping, density, segment_radius, history_dt,
                         bonded_exclusion)

    def save_velocity(self):
        pass

    def force_pass(self, dt, external_force=None):
        p, seg = self.pairs, self.seg
        c = p.shape[0]
        i, j = p[:, 0], p[:, 1]
        a0, a1, b0, b1 = seg[i, 0:3], seg[i, 3:6], seg[j, 0:3], seg[j, 3:6]
        force, sh = np.zeros((c, 3)), np.zeros((c, 2, 3))
        max_overlap = 0.0
        if c:
            dist, cp1, cp2, _, _, _ = fcm._oracle().distance_segment_segment(a0, a1, b0, b1)
            ri, rj = seg[i, 6], seg[j, 6]
            self.sep = dist - (ri + rj)
        else:
            self.sep = np.zeros(0)
        k = np.flatnonzero(self.sep < 0.0)
        if k.size:
            s = self.sep[k]
            nrm = (cp2[k] - cp1[k]) * (1.0 / dist[k])[:, None]
            Rs = (ri[k] * rj[k]) / (ri[k] + rj[k])                                               # :208
            E, nu = np.float64(self.E), np.float64(self.nu)
            Es = (E * E) / (E - E * nu * nu + E - E * nu * nu)                                   # :209-212
            mag = (4.0 / 3.0) * Es * np.sqrt(Rs) * np.power(-s, 1.5)                             # :217-219
            F = (-mag)[:, None] * nrm                                                            # :225
            force[k] = F
            sh[k, 0] = fcm.share(a0[k], a1[k], cp1[k], F)
            sh[k, 1] = fcm.share(b0[k], b1[k], cp2[k], -F)
            max_overlap = float((-s).max())
        self.force, self.share, self.tang_disp = force, sh, np.zeros((c, 3))
        self.node_force = reduce_rows(self, force, sh, external_force)
        self.stats = (max_overlap, 0)
        return self.stats


def contact_step(contacts, dt, time, external_force=None):
    """one inertial step with contacts, in the stepper's order: save_velocity (frictional law) -> predict -> update ->
    contact force -> forces -> correct -> (filament statistics, contact statistics, rebuilt, kinetic energy)"""
    f = contacts.f
    contacts.save_velocity()
    f.predict(dt)
    rebuilt = contacts.update()
    cstats = contacts.force_pass(dt, external_force)
    fstats = f.compute_force(time, contacts.node_force)
    return fstats, cstats, rebuilt, f.correct(dt)
