"""numpy restatement of the contact stage of the colliding filaments (filament_contact.hip), written from the reference
text in the operations and order include/mundy_hip.h documents:
  segment boxes     .../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161 (oracle.compute_aabb_segments, then the skin)
  rebuild rule      CollidingOverdampedFrictionalSperm.cpp:1565-1607 against the snapshot of the last build
  the list          :1612-1717 and DestroyBoundNeighbors.cpp:150-170: a brute-force search over the boxes
  distance          oracle.distance_segment_segment (distance_sq_between_line_segments)
  contact velocity  ...FrictionalHertzianContact.cpp:357-380;  the law :429-516 (friction_hertz_model's coefficients)
  reduction         .../linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221
Right-fold dot and norm, `* iL` where the reference multiplies.  Segment i joins the nodes i and i + 1 of one filament;
the row of a filament's last node is the degenerate record (x_i, x_i, r_i, 0), which never pairs."""
import math

import numpy as np

import friction_hertz_model as fh
from friction_hertz_model import dot, norm


def _oracle():
    import oracle
    oracle.build()
    return oracle


def point_velocity(x0, x1, v0, v1, cp):
    """get_contact_point_velocity (:357-380)"""
    rv, lc, lr = v1 - v0, cp - x0, x1 - x0
    iL = 1.0 / norm(lr)
    t = lr * iL[:, None]
    term1 = (dot(lc, rv)[:, None] * t) * iL[:, None]
    term2 = (dot(lc, t)[:, None] * (rv - dot(t, rv)[:, None] * t)) * iL[:, None]
    return (v0 + term1) + term2


def share(x0, x1, cp, Fs):
    """what the segment's right end node receives of Fs acting at cp (RED :206-212); the left one receives Fs - this"""
    lc, lr = cp - x0, x1 - x0
    iL = 1.0 / norm(lr)
    t = lr * iL[:, None]
    term1 = (dot(t, Fs)[:, None] * lc) * iL[:, None]
    term2 = (dot(lc, t)[:, None] * (Fs + dot(t, Fs)[:, None] * t)) * iL[:, None]
    return term2 - term1


def overlapping_pairs(aabb, has_r, node_ptr, bonded_exclusion=1):
    """every (i, j), i < j, of real segments whose boxes meet (closed intervals) and that are not at most
    bonded_exclusion apart along one filament; ascending (i, j) -> int32 [c, 2]"""
    n = aabb.shape[0]
    fid = np.repeat(np.arange(len(node_ptr) - 1), np.diff(node_ptr))
    out = []
    lo, hi = aabb[:, :3], aabb[:, 3:]
    for i in np.flatnonzero(has_r):
        j = np.arange(i + 1, n)
        ok = has_r[j] & (lo[i] <= hi[j]).all(axis=1) & (lo[j] <= hi[i]).all(axis=1)
        ok &= ~((fid[j] == fid[i]) & (j - i <= bonded_exclusion))
        jj = j[ok]
        out.append(np.stack([np.full(jj.size, i), jj], axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.int32).reshape(-1, 2)


class Contacts:
    """the contact stage over a filament_model.Filaments; the fields of mhip_filament_contact_fields as numpy arrays"""

    def __init__(self, filaments, skin, youngs_modulus, poisson_ratio, mu, damping=(0.0, 0.0), density=1.0,
                 segment_radius=None, history_dt=None, bonded_exclusion=1):
        self.f = filaments
        self.n = filaments.n
        self.skin, self.E, self.nu, self.mu = float(skin), float(youngs_modulus), float(poisson_ratio), float(mu)
        self.gn, self.gt, self.density = float(damping[0]), float(damping[1]), float(density)
        self.history_dt, self.bonded = history_dt, int(bonded_exclusion)
        self.radius = (filaments.radius if segment_radius is None else np.asarray(segment_radius, np.float64)).copy()
        self.velocity_prev = np.zeros((self.n, 3))
        self.node_force = np.zeros((self.n, 3))
        self.pairs = None
        self.tang_disp = np.zeros((0, 3))
        self.planted = None

    def save_velocity(self):
        v = self.f.velocity.copy()
        if self.f.prm.monolayer:
            v[:, 0] = 0.0
        self.velocity_prev = v

    def segment_view(self):
        x0 = self.f.center
        x1 = np.where(self.f.has_r[:, None], np.roll(x0, -1, axis=0), x0)
        self.seg = np.concatenate([x0, x1, self.radius[:, None], np.zeros((self.n, 1))], axis=1)
        box = _oracle().compute_aabb_segments(x0, x1, self.radius)
        self.aabb = np.concatenate([box[:, :3] - self.skin, box[:, 3:] + self.skin], axis=1)

    def moved(self):
        d = self.aabb - self.aabb_ref
        lo2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        hi2 = d[:, 3] * d[:, 3] + d[:, 4] * d[:, 4] + d[:, 5] * d[:, 5]
        thr = 0.5 * self.skin
        return bool(((lo2 >= thr * thr) | (hi2 >= thr * thr)).any())

    def set_history(self, pairs, tang_disp):
        pairs, tang_disp = np.asarray(pairs).reshape(-1, 2), np.asarray(tang_disp, np.float64).reshape(-1, 3)
        if self.pairs is None:
            self.planted = (pairs, tang_disp)
        else:
            self.tang_disp, _ = fh.carry_history(pairs, tang_disp, None, self.pairs)

    def update(self):
        """-> rebuilt"""
        self.segment_view()
        if self.pairs is not None and not self.moved():
            return False
        new = overlapping_pairs(self.aabb, self.f.has_r, self.f.node_ptr, self.bonded)
        old = (self.pairs, self.tang_disp) if self.pairs is not None else self.planted
        if old is None:
            self.tang_disp = np.zeros((new.shape[0], 3))
        else:
            self.tang_disp, _ = fh.carry_history(old[0], old[1], None, new)
        self.pairs = new
        c = new.shape[0]
        self.sep, self.force, self.share = np.zeros(c), np.zeros((c, 3)), np.zeros((c, 2, 3))
        self.aabb_ref = self.aabb.copy()
        return True

    def force_pass(self, dt, external_force=None):
        """linker pass and reduction -> (max_overlap, num_sliding)"""
        p, seg, n = self.pairs, self.seg, self.n
        c = p.shape[0]
        i, j = p[:, 0], p[:, 1]
        a0, a1, b0, b1 = seg[i, 0:3], seg[i, 3:6], seg[j, 0:3], seg[j, 3:6]
        force, sh, td = np.zeros((c, 3)), np.zeros((c, 2, 3)), np.zeros((c, 3))
        max_overlap, sliding = 0.0, 0
        if c:
            dist, cp1, cp2, _, _, _ = _oracle().distance_segment_segment(a0, a1, b0, b1)
            ri, rj = seg[i, 6], seg[j, 6]
            self.sep = dist - (ri + rj)
        else:
            self.sep = np.zeros(0)
        k = np.flatnonzero(~(self.sep > 0.0))
        if k.size:
            with np.errstate(all="ignore"):
                ik, jk, s = i[k], j[k], self.sep[k]
                nrm = (cp2[k] - cp1[k]) * (1.0 / dist[k])[:, None]
                v = self.velocity_prev
                vi = point_velocity(a0[k], a1[k], v[ik], v[ik + 1], cp1[k])
                vj = point_velocity(b0[k], b1[k], v[jk], v[jk + 1], cp2[k])
                F, tdk, capped = friction_law(vj - vi, nrm, s, ri[k], rj[k], self.E, self.nu, self.mu, self.gn, self.gt,
                                              self.density, dt if self.history_dt is None else self.history_dt,
                                              self.tang_disp[k])
                force[k], td[k] = F, tdk
                sh[k, 0] = share(a0[k], a1[k], cp1[k], F)
                sh[k, 1] = share(b0[k], b1[k], cp2[k], -F)
            ov = -s[-s > 0.0]
            max_overlap = float(ov.max()) if ov.size else 0.0
            sliding = int(capped.sum())
        self.force, self.share, self.tang_disp = force, sh, td
        # reduction: per segment from +0.0, its linkers in ascending order (side 0 then side 1 of one linker cannot be
        # the same segment); then the node adds (external + a0[i]) + a1[i - 1]
        A0, A1 = np.zeros((n, 3)), np.zeros((n, 3))
        Fs = np.stack([force, -force], axis=1)
        # ufunc.at is unbuffered: entry 2 c + side is added to its segment's sum in ascending order, one rounding each
        np.add.at(A0, p.reshape(-1), (Fs - sh).reshape(-1, 3))
        np.add.at(A1, p.reshape(-1), sh.reshape(-1, 3))
        f = np.zeros((n, 3)) if external_force is None else np.array(external_force, dtype=np.float64).reshape(n, 3)
        hr = self.f.has_r
        hl = np.concatenate([[False], hr[:-1]])
        f[hr] = f[hr] + A0[hr]
        f[hl] = f[hl] + np.roll(A1, 1, axis=0)[hl]
        self.node_force = f
        self.stats = (max_overlap, sliding)
        return self.stats


def friction_law(rel, nrm, s, ri, rj, E, nu, mu, gamma_n, gamma_t, density, dt, tang_disp):
    """the law of friction_hertz_model.friction_force after the contact-point velocities, branch for branch
    -> (force on segment i, new tang_disp, capped)"""
    rel_n = dot(rel, nrm)[:, None] * nrm
    rel_t = rel - rel_n
    td = tang_disp + rel_t * dt
    td = td - dot(td, nrm)[:, None] * nrm
    td_mag = norm(td)
    mi = 4.0 / 3.0 * math.pi * ri * ri * ri * density
    mj = 4.0 / 3.0 * math.pi * rj * rj * rj * density
    Rs = (ri * rj) / (ri + rj)
    ms = (mi * mj) / (mi + mj)
    Ev, nv = np.full(len(s), float(E)), np.full(len(s), float(nu))
    kn, kt = fh.spring_coefficients(Ev, Ev, nv, nv)
    hp = np.sqrt(-Rs * s)
    damp_t = (ms * gamma_t)[:, None] * rel_t
    Fn = hp[:, None] * ((kn * s)[:, None] * nrm + (ms * gamma_n)[:, None] * rel_n)
    Ft = hp[:, None] * (kt[:, None] * td + damp_t)
    ft_mag = norm(Ft)
    cap = mu * norm(Fn)
    capped = ft_mag > cap
    ratio = cap / ft_mag
    shift = damp_t / kt[:, None]
    rescale = capped & (td_mag != 0.0)
    td = np.where(rescale[:, None], ratio[:, None] * (td + shift) - shift, td)
    Ft = np.where(rescale[:, None], Ft * ratio[:, None], Ft)
    Ft = np.where((capped & ~rescale)[:, None], 0.0, Ft)
    return Fn + Ft, td, capped


def step(contacts, dt, time, external_force=None):
    """one pass of the loop with contacts: save_velocity -> advance -> update -> contact force -> forces -> velocities
    -> (filament statistics, contact statistics, rebuilt)"""
    f = contacts.f
    contacts.save_velocity()
    f.advance(dt)
    rebuilt = contacts.update()
    cstats = contacts.force_pass(dt, external_force)
    fstats = f.compute_force(time, contacts.node_force)
    f.compute_velocity()
    return fstats, cstats, rebuilt
