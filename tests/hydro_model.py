"""numpy float64 restatement of the n-body hydrodynamic velocity stage (mhip_hydro_velocity), written from the
reference's text: the pair kernels of scrap/.../periphery/Periphery.hpp (apply_stokes_kernel :719-743, apply_rpy_kernel
:893-938, apply_rpyc_kernel :1000-1081, quake_inv_sqrt :71-82), every product and sum in the reference's association (no
`**`, no fused operations: numpy rounds every elementwise operation once), and the summation order mundy_hip.h
documents: chunks of CHUNK consecutive sources, ascending source index inside a chunk from +0.0, chunk sums in ascending
chunk index from +0.0, the old value last.  A pair term is vectorised over the targets; the sums are strictly
sequential (np.add.accumulate is a running sum)."""
import numpy as np

CHUNK = 1024  # MHIP_HYDRO_CHUNK
KINDS = ("stokes", "rpy", "rpyc")
DOUBLE_ZERO = 1.0e-12
FAR, OVERLAP, LOCAL, SKIPPED = 0, 1, 2, 3  # RPYC branches


def quake_inv_sqrt(x):
    """Periphery.hpp:71-82: magic constant minus the arithmetically shifted signed pattern, ONE Newton step"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    x2 = x * 0.5
    i = x.view(np.int64)
    i = np.int64(0x5fe6eb50c7b537a9) - (i >> np.int64(1))
    y = i.view(np.float64)
    return y * (1.5 - ((x2 * y) * y))


def constants(viscosity):
    """(scale, c8, c6): 1 / (8 pi mu) formed once, and the two products RPYC's branches start from"""
    mu = np.float64(viscosity)
    inv_pi = np.float64(1.0) / np.float64(3.14159265358979323846)
    inv_mu = np.float64(1.0) / mu
    scale = np.float64(1.0) / ((np.float64(8.0) * np.float64(np.pi)) * mu)
    c8 = (np.float64(1.0 / 8.0) * inv_pi) * inv_mu
    c6 = (np.float64(1.0 / 6.0) * inv_pi) * inv_mu
    return scale, c8, c6


def rpyc_branch(d, a, b):
    """which branch apply_rpyc_kernel takes for the separations d [..., 3] and radii a (source), b (target)"""
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    r = np.sqrt(r2)
    far = a + b < r
    over = ~far & (np.abs(a - b) < r) & (a > DOUBLE_ZERO) & (b > DOUBLE_ZERO)
    skipped = ~far & ~over & (r2 < DOUBLE_ZERO)
    return np.where(far, FAR, np.where(over, OVERLAP, np.where(skipped, SKIPPED, LOCAL)))


def pair_terms(kind, viscosity, tgt_center, tgt_radius, src_center, src_radius, src_force):
    """K(x_t - x_s, b_t, a_s) f_s for every target t [nt] against ONE source or one source per column: the arrays
    broadcast (targets [nt, 1, 3] against sources [1, ns, 3] gives [nt, ns, 3])"""
    scale, c8, c6 = constants(viscosity)
    with np.errstate(all="ignore"):
        d = tgt_center - src_center
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        fx, fy, fz = np.broadcast_arrays(src_force[..., 0], src_force[..., 1], src_force[..., 2])
        r2 = (dx * dx + dy * dy) + dz * dz
        if kind == "stokes":
            rinv = np.where(r2 < DOUBLE_ZERO, 0.0, quake_inv_sqrt(r2))
            rinv3 = (rinv * rinv) * rinv
            fdr = (fx * dx + fy * dy) + fz * dz
            sr3 = scale * rinv3
            out = [sr3 * (r2 * f + dd * fdr) for f, dd in ((fx, dx), (fy, dy), (fz, dz))]
        elif kind == "rpy":
            a, b = src_radius, tgt_radius
            a2_over_three = (np.float64(1.0 / 3.0) * a) * a
            rinv = np.where(r2 < DOUBLE_ZERO, 0.0, quake_inv_sqrt(r2))
            rinv3 = (rinv * rinv) * rinv
            rinv5 = (rinv * rinv) * rinv3
            fdr = (fx * dx + fy * dy) + fz * dz
            three_fdr_rinv5 = (3.0 * fdr) * rinv5
            fdr_rinv3 = fdr * rinv3
            lap_coeff = (np.float64(1.0 / 6.0) * b) * b
            out = []
            for f, dd in ((fx, dx), (fy, dy), (fz, dz)):
                c = f * rinv3 - three_fdr_rinv5 * dd
                v = scale * ((f * rinv + dd * fdr_rinv3) + a2_over_three * c)
                lap = (2.0 * scale) * c
                out.append(v + lap_coeff * lap)
        elif kind == "rpyc":
            a, b = src_radius, tgt_radius
            one_over_three, one_over_32 = np.float64(1.0 / 3.0), np.float64(1.0 / 32.0)
            r = np.sqrt(r2)
            r3 = r * r2
            rinv = np.where(r2 < DOUBLE_ZERO, 0.0, 1.0 / r)
            rinv2 = rinv * rinv
            rinv3 = rinv2 * rinv
            hx, hy, hz = dx * rinv, dy * rinv, dz * rinv
            fdh = (fx * hx + fy * hy) + fz * hz
            # far
            q = (a * a + b * b) * rinv2
            sf = c8 * rinv
            t1f = sf * (1.0 + q * one_over_three)
            t2f = sf * (1.0 - q)
            # overlapping
            a_plus_b = a + b
            a_minus_b = a - b
            e = a_minus_b * a_minus_b
            tmp3 = e + 3.0 * r2
            tmp4 = e - r2
            so = c6 / (a * b)
            t1o = ((so * ((16.0 * r3) * a_plus_b - tmp3 * tmp3)) * one_over_32) * rinv3
            t2o = ((((so * 3.0) * tmp4) * tmp4) * one_over_32) * rinv3
            # local drag
            sl = c6 / np.where(a < b, b, a)
            br = rpyc_branch(d, a, b)
            t1 = np.where(br == FAR, t1f, t1o)
            t2 = np.where(br == FAR, t2f, t2o)
            out = []
            for f, h in ((fx, hx), (fy, hy), (fz, hz)):
                two = t1 * f + t2 * (fdh * h)
                out.append(np.where(br <= OVERLAP, two, np.where(br == LOCAL, sl * f, 0.0)))
        else:
            raise ValueError("kind must be one of %s" % (KINDS,))
    return np.stack(np.broadcast_arrays(*out), axis=-1)


def velocity(kind, viscosity, src_center, src_radius, src_force, tgt_center=None, tgt_radius=None, old=None,
             want_abs=False, chunk=CHUNK, block=256):
    """u [nt, 3] in the documented order (old [nt, 3]: added last); want_abs: also A [nt, 3] = sum_s |term_ts| per
    component (any order: it only scales error bounds)"""
    if tgt_center is None:
        tgt_center, tgt_radius = src_center, src_radius
    ns, nt = src_center.shape[0], tgt_center.shape[0]
    if src_radius is None:
        src_radius = np.zeros(ns)
    if tgt_radius is None:
        tgt_radius = np.zeros(nt)
    total = np.zeros((nt, 3))
    A = np.zeros((nt, 3))
    tc, tb = tgt_center[:, None, :], tgt_radius[:, None]
    for c0 in range(0, ns, chunk):
        acc = np.zeros((nt, 3))
        for s0 in range(c0, min(c0 + chunk, ns), block):
            s1 = min(s0 + block, c0 + chunk, ns)
            terms = pair_terms(kind, viscosity, tc, tb, src_center[None, s0:s1], src_radius[None, s0:s1],
                               src_force[None, s0:s1])
            # a strictly sequential running sum that starts from acc
            acc = np.add.accumulate(np.concatenate([acc[:, None, :], terms], axis=1), axis=1)[:, -1, :]
            if want_abs:
                A += np.abs(terms).sum(axis=1)
        total = total + acc
    if old is not None:
        total = old + total
    return (total, A) if want_abs else total


def inputs(ns, nt=None, seed=0, density=0.35):
    """polydisperse spheres, radii 0.2 .. 1.2, in a box dense enough for all three RPYC branches, with a few exact
    duplicates of centres and some zero radii; nt=None: beads to beads (targets = sources)"""
    rng = np.random.default_rng(seed)

    def cloud(n, edge):
        c = rng.uniform(0.0, edge, (n, 3))
        r = rng.uniform(0.2, 1.2, n)
        r[rng.random(n) < 0.05] = 0.0
        return c, r

    n_all = ns + (nt or 0)
    edge = max(2.0, (n_all / density) ** (1.0 / 3.0))
    sc, sa = cloud(ns, edge)
    f = rng.normal(size=(ns, 3))
    if nt is None:
        if ns >= 8:  # exact duplicates of centres
            sc[ns // 2] = sc[1]
            sc[ns - 1] = sc[3]
        return dict(sc=sc, sa=sa, f=f, tc=sc, tb=sa)
    tc, tb = cloud(nt, edge)
    k = min(ns, nt)
    dup = np.arange(0, k, max(1, k // 7))  # targets on top of sources (coincident: skipped / zero rinv)
    tc[dup] = sc[dup]
    return dict(sc=sc, sa=sa, f=f, tc=tc, tb=tb)
