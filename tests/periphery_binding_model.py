"""numpy restatement of the crosslinker KMC step with periphery bind sites (crosslink.hip: k_xl_kmc_periphery,
k_xl_force_periphery), in the operations and order include/mundy_hip_periphery_binding.h documents.  It extends
crosslinker_model.py, which it imports and leaves as it is: the uniform, the distance and the rate are that module's.

State: right[c] == left[c] singly bound, right[c] >= 0 bound to that bead, right[c] == -(s + 1) bound to site s.
Parameters: par = the crosslinkers' dict(kind, k, r, A, k_off, kt, capture_radius); per = the periphery's dict(A, k, r,
k_off, capture_radius) (k_off None: the crosslinkers')."""
import numpy as np

import chain_model as cm
import crosslinker_model as xm


def from_ops(p):
    """the keywords of ops.Crosslinkers / crosslinker_model.decision_case's par -> this module's par"""
    return dict(kind=p["kind"], k=p["k"], r=p["r"], A=p["bind_rate"], k_off=p["unbind_rate"], kt=p["kt"],
                capture_radius=p["capture_radius"])


def site_rows(center, sources, sites, reach):
    """CSR (ptr [n + 1], col: site indices) over the beads: row b of a source holds every site s with
    |y_s - x_b| <= reach, ascending in s (the order a crosslinker walks them in)"""
    center, sites = np.asarray(center, dtype=np.float64), np.asarray(sites, dtype=np.float64)
    n, P = center.shape[0], sites.shape[0]
    allc = np.concatenate([center, sites])
    src = np.concatenate([np.asarray(sources).astype(bool), np.zeros(P, bool)])
    tgt = np.concatenate([np.zeros(n, bool), np.ones(P, bool)])
    ptr, col = xm.candidate_rows(allc, src, tgt, reach)
    return ptr[:n + 1], col - n


def sort_rows(ptr, col):
    """every row ascending in site index"""
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))
    return col[np.lexsort((col, row))]


def kmc_step(center, left, right, ptr, col, pptr, pcol, sites, par, per, dt, keys, counters):
    """one KMC step -> dict(right, counters, u, z_tot, margin, binds, unbinds, periphery_bound, z_beads)
    ptr / col: the bead rows by body, pptr / pcol: the site rows by body, both already in walking order.  z_beads is the
    running sum at the end of the bead row; margin as crosslinker_model.kmc_step's, over both rows."""
    center, sites = np.asarray(center, dtype=np.float64), np.asarray(sites, dtype=np.float64).reshape(-1, 3)
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    pptr, pcol = np.asarray(pptr, dtype=np.int64), np.asarray(pcol, dtype=np.int64)
    kind, kt = par["kind"], par["kt"]
    k_off_p = par["k_off"] if per.get("k_off") is None else per["k_off"]
    m = left.shape[0]
    u = xm.uniform(keys, counters)
    bound = right != left
    at_site = right < 0
    new_right = right.copy()
    margin = np.full(m, np.inf)
    # doubly bound: the rate constant goes by the sign of right
    p_off = np.where(at_site, 1.0 - np.exp(-(dt * k_off_p)), 1.0 - np.exp(-(dt * par["k_off"])))
    unbind = bound & (u < p_off)
    new_right[unbind] = left[unbind]
    margin[bound] = np.abs(u[bound] - p_off[bound])
    xl = center[left]

    def rows(rptr, rcol, pos, self_skip, cap, rate_par):
        lo, ln = rptr[left], rptr[left + 1] - rptr[left]
        ln = np.where(bound, 0, ln)
        width = int(ln.max()) if m else 0

        def slot(j):
            live = j < ln
            s = rcol[np.where(live, lo + j, 0)] if rcol.size else np.zeros(m, np.int64)
            d = xm.distance(pos[s], xl) if pos.shape[0] else np.zeros(m)
            ok = live & (d <= cap)
            if self_skip:
                ok &= s != left
            return ok, s, np.where(ok, xm.rate(kind, d, rate_par["k"], rate_par["r"], rate_par["A"], kt), 0.0)
        return width, slot

    bw, bslot = rows(ptr, col, center, True, par["capture_radius"], par)
    pw, pslot = rows(pptr, pcol, sites, False, per["capture_radius"], per)
    z_tot = np.zeros(m)
    for j in range(bw):
        ok, _, rt = bslot(j)
        z_tot = np.where(ok, z_tot + dt * rt, z_tot)
    z_beads = z_tot.copy()
    for j in range(pw):  # the same running sum goes on over the site row
        ok, _, rt = pslot(j)
        z_tot = np.where(ok, z_tot + dt * rt, z_tot)
    p_bind = 1.0 - np.exp(-z_tot)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = p_bind * dt / z_tot
    binds = ~bound & (u < p_bind)
    margin[~bound] = np.abs(u[~bound] - p_bind[~bound])
    cumsum = np.zeros(m)
    done = np.zeros(m, bool)
    for width, slot, encode in ((bw, bslot, lambda s: s), (pw, pslot, lambda s: -(s + 1))):
        for j in range(width):
            ok, s, rt = slot(j)
            with np.errstate(invalid="ignore"):
                near = ok & binds & ~done
                cumsum = np.where(near, cumsum + scale * rt, cumsum)
                hit = near & (u < cumsum)
                margin[near] = np.minimum(margin[near], np.abs(u[near] - cumsum[near]))
            new_right[hit] = encode(s[hit])
            done |= hit
    return dict(right=new_right, counters=np.asarray(counters).astype(np.uint64) + np.uint64(1), u=u, z_tot=z_tot,
                z_beads=z_beads, margin=margin, binds=int(done.sum()), unbinds=int(unbind.sum()),
                periphery_bound=int((new_right < 0).sum()))


def crosslinker_force(n, left, right, kind, k, r, center, sites):
    """-> (force [n, 3], overstretched, max_length, site_force [P, 3]): the doubly bound crosslinkers as springs in
    ascending crosslinker index; a periphery-bound one is the spring (left, site), whose term goes to the left bead
    only.  site_force is what the sites would receive (and do not): the sum over the beads is its negative, up to the
    rounding of that sum."""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    center, sites = np.asarray(center, dtype=np.float64), np.asarray(sites, dtype=np.float64).reshape(-1, 3)
    b = right != left
    far = np.where(right < 0, n - (right + 1), right)
    f, over, mx = cm.spring_force(n + sites.shape[0], np.stack([left[b], far[b]], axis=1), kind, k, r,
                                  np.concatenate([center, sites]))
    return f[:n], over, mx, f[n:]


def decision_case(kind, seed, n=20000, m=20000, P=300):
    """crosslinker_model.decision_case at reduced n, with P sites, most of them on a sphere cutting through the dense
    box; a third of the crosslinkers start bead-bound, a sixth periphery-bound"""
    d = xm.decision_case(kind, seed, n=n, m=m)
    rng = np.random.default_rng(seed + 1000)
    edge = 22.0 * (n / 1e5) ** (1.0 / 3.0)
    v = rng.normal(size=(P, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    # a sphere about the box's corner region: its surface passes through the dense box
    pts = 0.5 * edge + 0.45 * edge * v
    # ... and a fifth of the sites next to beads of the dilute halo that carry a crosslinker: rows with sites only
    c = d["center"]
    halo = np.flatnonzero(((c < -2.0) | (c > edge + 2.0)).any(axis=1) & np.isin(np.arange(n), d["left"]))
    at = halo[rng.permutation(halo.size)[:P // 5]]
    pts[:at.size] = c[at] + np.array([0.5, 0.0, 0.0])
    d["site_points"] = pts
    right = d["right"].copy()
    free = np.flatnonzero(right == d["left"])
    pick = free[rng.random(free.size) < 0.25]   # a quarter of the two thirds that are free: a sixth
    right[pick] = -(rng.integers(0, P, pick.size) + 1)
    d["right"] = right
    d["per"] = dict(A=3.0, k=4.0, r=0.4 if kind == "hookean" else 1.1, k_off=9.0, capture_radius=1.2)
    return d


DECISION_SEEDS = {"hookean": 11, "fene": 12}
