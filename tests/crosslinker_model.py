"""numpy restatement of the crosslinker kinetic Monte Carlo step (crosslink.hip), written from the reference text
(HP1.cpp:3264-3438 rates, :3440-3594 sampling, :3597-3748 state changes) in the operations and order include/mundy_hip.h
documents.  The uniform is chain_model.philox's; exp / pow are numpy's, so a device result may differ from these in the
last place -- every threshold a decision depends on is returned, so that a test can tell how close a draw came."""
import numpy as np

import chain_model as cm


def uniform(keys, counters):
    """u = ((w0 << 21) | (w1 >> 11)) 2^-53 from block 0 at (key, counter)"""
    w = cm.philox(keys, counters, 0).astype(np.uint64)
    return ((w[:, 0] << np.uint64(21)) | (w[:, 1] >> np.uint64(11))).astype(np.float64) * 2.0 ** -53


def distance(a, b):
    d = a - b
    return np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))


def rate(kind, d, k, r, A, kt):
    """binding rate to a site at distance d (HP1.cpp:3320, :3332-3334), their association"""
    inv_kt = 1.0 / kt
    d = np.asarray(d, dtype=np.float64)
    if kind == "hookean":
        return A * np.exp(-0.5 * inv_kt * k * (d - r) * (d - r))
    with np.errstate(invalid="ignore"):
        base = np.where(d < r, 1.0 - (d / r) * (d / r), 1.0)
        return np.where(d < r, A * np.power(base, 0.5 * inv_kt * k * r * r), 0.0)


def candidate_rows(center, sources, sites, reach):
    """CSR (ptr [n + 1], col) over the bodies: row s of a source holds every site t != s with |x_t - x_s| <= reach,
    ascending in t; other rows are empty.  A cell grid of edge `reach`, exact distances."""
    center = np.asarray(center, dtype=np.float64)
    n = center.shape[0]
    src = np.flatnonzero(np.asarray(sources))
    tgt = np.flatnonzero(np.asarray(sites))
    if src.size == 0 or tgt.size == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int64)
    lo = center.min(axis=0)
    cell = np.floor((center - lo) / reach).astype(np.int64) + 1
    dims = cell.max(axis=0) + 2
    key = lambda c: (c[:, 0] * dims[1] + c[:, 1]) * dims[2] + c[:, 2]  # noqa: E731
    tkey = key(cell[tgt])
    order = np.argsort(tkey, kind="stable")
    tgt, tkey = tgt[order], tkey[order]
    ss, tt = [], []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                k = key(cell[src] + np.array([dx, dy, dz]))
                a, b = np.searchsorted(tkey, k, "left"), np.searchsorted(tkey, k, "right")
                cnt = b - a
                s = np.repeat(src, cnt)
                off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
                t = tgt[np.repeat(a, cnt) + off]
                keep = (t != s) & (distance(center[t], center[s]) <= reach)
                ss.append(s[keep])
                tt.append(t[keep])
    s, t = np.concatenate(ss), np.concatenate(tt)
    order = np.lexsort((t, s))
    s, t = s[order], t[order]
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, s + 1, 1)
    return np.cumsum(ptr), t


def sort_rows_by_id(ptr, col, ids):
    """every row ascending in ids[col] (the order a crosslinker walks its candidates in)"""
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr))
    return col[np.lexsort((np.asarray(ids)[col], row))]


def kmc_step(center, left, right, ptr, col, kind, k, r, A, k_off, kt, capture_radius, dt, keys, counters):
    """one KMC step -> dict(right, counters, u, z_tot, margin, binds, unbinds)
    ptr / col: the candidate rows by body, already in walking order.  margin [m] = the distance of u from the nearest
    threshold the decision of that crosslinker compares it with (p_bind and every running sum of its row; p_unbind for
    a doubly bound one)."""
    center = np.asarray(center, dtype=np.float64)
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    ptr, col = np.asarray(ptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    m = left.shape[0]
    u = uniform(keys, counters)
    bound = right != left
    new_right = right.copy()
    margin = np.full(m, np.inf)
    # doubly bound: what HP1.cpp:3554-3573 reduces to
    p_off = 1.0 - np.exp(-(dt * k_off))
    unbind = bound & (u < p_off)
    new_right[unbind] = left[unbind]
    margin[bound] = np.abs(u[bound] - p_off)
    # singly bound: two passes over the row of the left bead
    lo, ln = ptr[left], ptr[left + 1] - ptr[left]
    ln = np.where(bound, 0, ln)
    xl = center[left]
    width = int(ln.max()) if m else 0

    def slot_rate(j):
        live = j < ln
        s = col[np.where(live, lo + j, 0)] if col.size else np.zeros(m, np.int64)
        d = distance(center[s], xl)
        ok = live & (s != left) & (d <= capture_radius)
        return ok, s, np.where(ok, rate(kind, d, k, r, A, kt), 0.0)

    z_tot = np.zeros(m)
    for j in range(width):
        ok, _, rt = slot_rate(j)
        z_tot = np.where(ok, z_tot + dt * rt, z_tot)
    p_bind = 1.0 - np.exp(-z_tot)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = p_bind * dt / z_tot
    binds = ~bound & (u < p_bind)
    margin[~bound] = np.abs(u[~bound] - p_bind[~bound])
    cumsum = np.zeros(m)
    site = np.full(m, -1, np.int64)
    for j in range(width):
        ok, s, rt = slot_rate(j)
        with np.errstate(invalid="ignore"):
            cumsum = np.where(ok, cumsum + scale * rt, cumsum)
            hit = ok & binds & (site < 0) & (u < cumsum)
            near = ok & binds & (site < 0)
            margin[near] = np.minimum(margin[near], np.abs(u[near] - cumsum[near]))
        site[hit] = s[hit]
    chosen = site >= 0
    new_right[chosen] = site[chosen]
    return dict(right=new_right, counters=np.asarray(counters).astype(np.uint64) + np.uint64(1), u=u, z_tot=z_tot,
                margin=margin, binds=int(chosen.sum()), unbinds=int(unbind.sum()))


def crosslinker_force(n, left, right, kind, k, r, center):
    """the doubly bound crosslinkers as the springs (left, right) in ascending crosslinker index"""
    left, right = np.asarray(left, dtype=np.int64), np.asarray(right, dtype=np.int64)
    b = right != left
    return cm.spring_force(n, np.stack([left[b], right[b]], axis=1), kind, k, r, np.asarray(center, dtype=np.float64))


def decision_case(kind, seed, n=100000, m=100000):
    """the system of the rates-and-decisions test: random beads (a dense box and a dilute halo, so that rows hold 0 to
    about 40 candidates), half of them bind sites, crosslinkers on random beads (several on some, none on others), a
    third doubly bound; ids a random permutation, keys and counters spread over their ranges"""
    rng = np.random.default_rng(seed)
    nd = (9 * n) // 10
    center = np.concatenate([rng.uniform(0.0, 22.0 * (n / 1e5) ** (1.0 / 3.0), (nd, 3)),
                             rng.uniform(-40.0, 64.0, (n - nd, 3))])
    center = center[rng.permutation(n)]
    sites = (rng.random(n) < 0.5).astype(np.uint8)
    left = rng.integers(0, n, m)
    right = left.copy()
    pick = rng.random(m) < 1.0 / 3.0
    site_idx = np.flatnonzero(sites)
    right[pick] = site_idx[rng.integers(0, site_idx.size, int(pick.sum()))]
    par = dict(kind=kind, k=5.0, r=0.5 if kind == "hookean" else 0.9, bind_rate=2.0, unbind_rate=6.0, kt=1.0,
               capture_radius=1.0)
    return dict(center=center, sites=sites, left=left, right=right, ids=rng.permutation(n).astype(np.int64),
                keys=rng.integers(0, 2 ** 63, m, dtype=np.int64), counter=rng.integers(0, 2 ** 40, m, dtype=np.int64),
                dt=0.05, par=par)


DECISION_SEEDS = {"hookean": 11, "fene": 12}
DECISION_MARGIN = 1e-12  # times max(1, z_tot)


def left_out(res):
    """crosslinkers whose draw came too close to a threshold for a device with another exp / pow to be held to it"""
    return res["margin"] <= DECISION_MARGIN * np.maximum(1.0, res["z_tot"])
