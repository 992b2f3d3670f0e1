"""numpy restatement of the frictional Hertzian rod contact (hertz_friction.hip) and of the history carry, in the
operations and association the library documents (include/mundy_hip.h).  Only + - * / sqrt occur and numpy rounds each
of them once, so the float expressions land on the device's bits.  The model is the definition the tests hold the
kernels to; it follows SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:384-518 branch for branch."""
import math

import numpy as np


def dot(a, b):
    """right fold a0 b0 + (a1 b1 + a2 b2) (mundy_math/impl/VectorImpl.hpp:339-344)"""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def norm(a):
    return np.sqrt(dot(a, a))


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _per_body(v, n):
    return np.full(n, float(v)) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)


def spring_coefficients(Ei, Ej, ni, nj):
    """(k_n, k_t) = (4/3 E*, 8 G*) in the kernel's association"""
    Es = (Ei * Ej) / (Ej - Ej * ni * ni + Ei - Ei * nj * nj)
    Gi, Gj = 0.5 * Ei / (1.0 + ni), 0.5 * Ej / (1.0 + nj)
    Gs = (Gi * Gj) / (Gj * (2.0 - ni) + Gi * (2.0 - nj))
    return (4.0 / 3.0) * Es, 8.0 * Gs


def reference_coefficients(E, nu):
    """the reference's two expressions for one material (:409-411)"""
    G = 0.5 * E / (1.0 + nu)
    return 4.0 / 3.0 * G / (1.0 - nu), 4.0 * G / (2.0 - nu)


def contact_point_velocity(vel, seg, b, arc):
    """U + W x ((s - 1/2)(p1 - p0)), the arclength clamped to [0, 1] (the rod-compressed operator's arm)"""
    axis = seg[b, 3:6] - seg[b, 0:3]
    coef = np.where(arc < 0.0, 0.0, np.where(arc > 1.0, 1.0, arc)) - 0.5
    arm = coef[:, None] * axis
    return vel[b, 0:3] + cross(vel[b, 3:6], arm)


def friction_force(pairs, sep, normal, arc_s, arc_t, seg, radius, E, nu, vel_prev, mu, gamma_n, gamma_t, density, dt,
                   tang_disp, parts=None):
    """-> (force [c, 3] on body i, new tang_disp [c, 3], max_overlap, num_sliding).  Rows with sep > 0 are +0.0.
    parts (a dict, optional) receives the two summands of the force, "Fn" and "Ft" [c, 3], as the kernel forms them."""
    pairs = np.asarray(pairs).reshape(-1, 2)
    c, n = pairs.shape[0], radius.shape[0]
    E, nu = _per_body(E, n), _per_body(nu, n)
    force = np.zeros((c, 3))
    td_out = np.zeros((c, 3))
    bad = ((pairs < 0) | (pairs >= n)).any(axis=1)
    force[bad] = np.nan
    td_out[bad] = np.nan
    k = np.nonzero(~bad & ~(sep > 0.0))[0]  # the contact branch: sep <= 0, or NaN
    if parts is not None:
        parts["Fn"], parts["Ft"] = np.zeros((c, 3)), np.zeros((c, 3))
    if k.size == 0:
        return force, td_out, 0.0, 0
    i, j = pairs[k, 0], pairs[k, 1]
    s, nrm = sep[k], normal[k]
    with np.errstate(invalid="ignore", divide="ignore"):
        vi = contact_point_velocity(vel_prev, seg, i, arc_s[k])
        vj = contact_point_velocity(vel_prev, seg, j, arc_t[k])
        rel = vj - vi
        rel_n = dot(rel, nrm)[:, None] * nrm
        rel_t = rel - rel_n
        td = tang_disp[k] + rel_t * dt
        td = td - dot(td, nrm)[:, None] * nrm
        td_mag = norm(td)
        ri, rj = radius[i], radius[j]
        mi = 4.0 / 3.0 * math.pi * ri * ri * ri * density
        mj = 4.0 / 3.0 * math.pi * rj * rj * rj * density
        Rs = (ri * rj) / (ri + rj)
        ms = (mi * mj) / (mi + mj)
        kn, kt = spring_coefficients(E[i], E[j], nu[i], nu[j])
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
        force[k] = Fn + Ft
        td_out[k] = td
        if parts is not None:
            parts["Fn"][k], parts["Ft"][k] = Fn, Ft
    ov = -s[-s > 0.0]
    return force, td_out, float(ov.max()) if ov.size else 0.0, int(capped.sum())


def carry_history(pairs_old, hist_old, new_of_old, pairs_new):
    """-> (hist_new [c_new, 3], carried).  A dict keyed by the unordered renumbered pair; the row changes sign when the
    orientation (which endpoint is listed first) differs between the renumbered old pair and the new pair."""
    table = {}
    for row, (a, b) in enumerate(np.asarray(pairs_old).reshape(-1, 2).tolist()):
        if new_of_old is not None:
            a, b = int(new_of_old[a]), int(new_of_old[b])
        if a < 0 or b < 0 or a == b:
            continue
        table[(min(a, b), max(a, b))] = (row, a > b)
    pairs_new = np.asarray(pairs_new).reshape(-1, 2)
    out = np.zeros((pairs_new.shape[0], 3))
    carried = 0
    for c, (i, j) in enumerate(pairs_new.tolist()):
        hit = table.get((min(i, j), max(i, j)))
        if hit is not None and i != j:
            row, flipped = hit
            out[c] = -hist_old[row] if flipped != (i > j) else hist_old[row]
            carried += 1
    return out, carried


# ---- the two-rod sled: a rod pressed onto a fixed rod across it and pulled along it ------------------------------------
SLED = dict(r=0.5, E=1000.0, nu=0.3, dt=1e-4, press=1.0, viscosity=1e-3, length_bottom=8.0, length_top=4.0)


def sled_constants():
    """(k_n, k_t, R*, equilibrium overlap, hp at that overlap, m_t of the top rod)"""
    kn, kt = spring_coefficients(SLED["E"], SLED["E"], SLED["nu"], SLED["nu"])
    Rs = SLED["r"] * SLED["r"] / (SLED["r"] + SLED["r"])
    delta = (SLED["press"] / (kn * math.sqrt(Rs))) ** (2.0 / 3.0)
    mt = 1.0 / (6.0 * math.pi * SLED["viscosity"] * 2.5)
    return kn, kt, Rs, delta, math.sqrt(Rs * delta), mt


def sled(pull, mu, steps):
    """Bottom rod (body 0) along x, fixed; top rod (body 1) along y, resting on it at the equilibrium overlap, pushed down
    by `press` and pulled along x by `pull`; explicit Euler with the dry drag m_t.  Returns per step (x, v_x, |tang_disp|,
    num_sliding) of the top rod, using friction_force for the one contact."""
    _, _, _, delta, _, mt = sled_constants()
    r, dt = SLED["r"], SLED["dt"]
    Lb, Lt = SLED["length_bottom"], SLED["length_top"]
    pos = np.array([0.0, 0.0, 2.0 * r - delta])
    vel = np.zeros((2, 6))
    td = np.zeros((1, 3))
    radius = np.array([r, r])
    pairs = np.array([[0, 1]])
    out = []
    for _ in range(steps):
        seg = np.zeros((2, 8))
        seg[0, 0:3], seg[0, 3:6] = (-0.5 * Lb, 0.0, 0.0), (0.5 * Lb, 0.0, 0.0)
        seg[1, 0:3], seg[1, 3:6] = pos + (0.0, -0.5 * Lt, 0.0), pos + (0.0, 0.5 * Lt, 0.0)
        sep = np.array([pos[2] - 2.0 * r])
        normal = np.array([[0.0, 0.0, 1.0]])
        s, t = np.array([0.5 + pos[0] / Lb]), np.array([0.5])
        f, td, _, sliding = friction_force(pairs, sep, normal, s, t, seg, radius, SLED["E"], SLED["nu"], vel, mu, 0.0,
                                           0.0, 1.0, dt, td)
        u = mt * (-f[0] + np.array([pull, 0.0, -SLED["press"]]))
        vel[1, 0:3] = u
        pos = pos + dt * u
        out.append((pos[0], u[0], float(norm(td[0])), sliding))
    return out
