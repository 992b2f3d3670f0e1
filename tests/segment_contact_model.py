"""numpy restatement of the backbone segment contacts (segment_contact.hip), written from the reference text in the
operations and order include/mundy_hip_segment_contact.h documents:
  segment boxes   .../compute_aabb/kernels/SpherocylinderSegment.cpp:156-161 (oracle.compute_aabb_segments, then the skin)
  rebuild rule    HP1.cpp:3212-3262 against the snapshot of the last build
  the list        HP1.cpp:3053-3175 and DestroyBoundNeighbors.cpp:150-170: a brute-force search over the boxes, without
                  the pairs that share a node
  distance        oracle.distance_segment_segment
  the laws        ...SegmentHertzianContact.cpp:192-225, ...SegmentWCA.cpp:187-210
  reduction       .../linker_potential_force_reduction/kernels/SpherocylinderSegment.cpp:193-221, then the end-segment
                  correction of HP1.cpp:4375-4493
Right-fold dot and norm, `* iL` where the reference multiplies.  Segment e joins the bodies ends[e][0] and ends[e][1].

The three cases of the tests (case(name)) are regenerated from their seeds; nothing here touches the device."""
import numpy as np

from filament_contact_model import share
from friction_hertz_model import dot, norm  # noqa: F401

DEFAULTS = dict(youngs_modulus=1000.0, poisson_ratio=0.3, epsilon=1.0, sigma=1.0, cutoff=1.12246204831)
COLINEAR_D = 3.162277660168379e-08   # sqrt(1e-15): LineSegmentLineSegment.hpp:215


def _oracle():
    import oracle
    oracle.build()
    return oracle


def chain_end_segments(n, ends):
    """segments with an end node that belongs to no other segment ("first or last element in chain")"""
    ends = np.asarray(ends).reshape(-1, 2)
    deg = np.bincount(ends.reshape(-1), minlength=n)
    return (deg[ends] == 1).any(axis=1) if ends.size else np.zeros(0, bool)


def overlapping_pairs(aabb, ends):
    """every (i, j), i < j, of segments whose boxes meet (closed intervals) and that share no node; ascending (i, j)
    -> int32 [c, 2]"""
    m = aabb.shape[0]
    lo, hi = aabb[:, :3], aabb[:, 3:]
    out = []
    for i in range(m):
        j = np.arange(i + 1, m)
        ok = (lo[i] <= hi[j]).all(axis=1) & (lo[j] <= hi[i]).all(axis=1)
        ok &= ~((ends[j] == ends[i, 0]) | (ends[j] == ends[i, 1])).any(axis=1)
        jj = j[ok]
        out.append(np.stack([np.full(jj.size, i), jj], axis=1))
    return (np.concatenate(out) if out else np.zeros((0, 2))).astype(np.int32).reshape(-1, 2)


def hertz_magnitude(E, nu, ri, rj, s):
    Rs = (ri * rj) / (ri + rj)
    Es = (E * E) / (E - E * nu * nu + E - E * nu * nu)
    return (4.0 / 3.0) * Es * np.sqrt(Rs) * np.power(-s, 1.5)


def wca_magnitude(epsilon, sigma, d):
    rho2 = sigma * sigma / (d * d)
    rho6 = rho2 * rho2 * rho2
    rho12 = rho6 * rho6
    return 24.0 * epsilon * (2.0 * rho12 - rho6) / d


class SegmentContacts:
    """the term over n bodies; the fields of mhip_segment_contact_fields as numpy arrays"""

    def __init__(self, n, ends, kind, radius, skin, end_correction=None, **law):
        self.n, self.kind, self.skin = int(n), kind, float(skin)
        self.ends = np.asarray(ends, dtype=np.int64).reshape(-1, 2)
        self.m = self.ends.shape[0]
        self.radius = np.broadcast_to(np.asarray(radius, dtype=np.float64), (self.m,)).copy()
        p = dict(DEFAULTS, **law)
        self.E, self.nu = float(p["youngs_modulus"]), float(p["poisson_ratio"])
        self.epsilon, self.sigma, self.cutoff = float(p["epsilon"]), float(p["sigma"]), float(p["cutoff"])
        if end_correction is None:
            self.corr = chain_end_segments(self.n, self.ends)
        elif end_correction is False:
            self.corr = np.zeros(self.m, bool)
        else:
            self.corr = np.asarray(end_correction) != 0
        self.pairs = None

    def segment_view(self, x):
        x0, x1 = x[self.ends[:, 0]], x[self.ends[:, 1]]
        self.seg = np.concatenate([x0, x1, self.radius[:, None], np.zeros((self.m, 1))], axis=1)
        reach = self.radius if self.kind == "hertz" else np.maximum(self.radius, 0.5 * self.cutoff)
        box = _oracle().compute_aabb_segments(x0, x1, reach) if self.m else np.zeros((0, 6))
        self.aabb = np.concatenate([box[:, :3] - self.skin, box[:, 3:] + self.skin], axis=1)

    def moved(self):
        d = self.aabb - self.aabb_ref
        lo2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        hi2 = d[:, 3] * d[:, 3] + d[:, 4] * d[:, 4] + d[:, 5] * d[:, 5]
        thr = 0.5 * self.skin
        return bool(((lo2 >= thr * thr) | (hi2 >= thr * thr)).any())

    def update(self, x, force_rebuild=False):
        """-> rebuilt"""
        self.segment_view(x)
        if self.pairs is not None and not force_rebuild and not self.moved():
            return False
        self.pairs = overlapping_pairs(self.aabb, self.ends)
        self.aabb_ref = self.aabb.copy()
        return True

    def linker_pass(self):
        """sep, force, share, in_branch, dist and the closest-point parameters of every linker -> (max_overlap, count)"""
        p, seg = self.pairs, self.seg
        c = p.shape[0]
        i, j = p[:, 0], p[:, 1]
        a0, a1, b0, b1 = seg[i, 0:3], seg[i, 3:6], seg[j, 0:3], seg[j, 3:6]
        self.force, self.share = np.zeros((c, 3)), np.zeros((c, 2, 3))
        if c:
            self.dist, cp1, cp2, self.s, self.t, _ = _oracle().distance_segment_segment(a0, a1, b0, b1)
            ri, rj = seg[i, 6], seg[j, 6]
            self.sep = self.dist - (ri + rj)
        else:
            self.dist = self.sep = self.s = self.t = np.zeros(0)
        self.in_branch = (self.sep < 0.0) if self.kind == "hertz" else (self.dist < self.cutoff)
        k = np.flatnonzero(self.in_branch)
        if k.size:
            with np.errstate(all="ignore"):
                nrm = (cp2[k] - cp1[k]) * (1.0 / self.dist[k])[:, None]
                if self.kind == "hertz":
                    fm = hertz_magnitude(self.E, self.nu, ri[k], rj[k], self.sep[k])
                else:
                    fm = wca_magnitude(self.epsilon, self.sigma, self.sep[k] + (ri[k] + rj[k]))
                F = (-fm)[:, None] * nrm
                self.force[k] = F
                self.share[k, 0] = share(a0[k], a1[k], cp1[k], F)
                self.share[k, 1] = share(b0[k], b1[k], cp2[k], -F)
        ov = -self.sep[k]
        self.stats = (float(ov.max()) if k.size and ov.max() > 0.0 else 0.0, int(k.size))
        return self.stats

    def end_terms(self):
        """the correction of every segment -> (fm t [m, 3], in the branch [m], L - 2 r [m]); all-zero rows where no
        correction is set or the branch is not taken"""
        d = self.seg[:, 3:6] - self.seg[:, 0:3]
        with np.errstate(all="ignore"):
            L = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
            t = d / L[:, None]
            gap = L - 2.0 * self.radius
            if self.kind == "hertz":
                on = self.corr & (gap < 0.0)
                fm = hertz_magnitude(self.E, self.nu, self.radius, self.radius, np.where(on, gap, -1.0))
            else:
                on = self.corr & (L < self.cutoff)
                fm = wca_magnitude(self.epsilon, self.sigma, L)
            ft = np.where(on[:, None], fm[:, None] * t, 0.0)
        return ft, on, gap

    def reduce(self, force=None, share_rows=None, external=None):
        """the segment sums and the node gather over the linker rows given (default: the model's own) -> node force
        [n, 3] = external + S, a body on no segment keeping its external row (or +0.0).  Also raises stats[0] by the
        corrected end segments."""
        force = self.force if force is None else np.asarray(force).reshape(-1, 3)
        sh = self.share if share_rows is None else np.asarray(share_rows).reshape(-1, 2, 3)
        m, n, p = self.m, self.n, self.pairs
        A = np.zeros((m, 2, 3))
        Fs = np.stack([force, -force], axis=1)
        # ufunc.at is unbuffered: entry 2 c + side is added to its segment's sum in ascending order, one rounding each
        # (side 0 and side 1 of one linker are never the same segment)
        np.add.at(A[:, 0], p.reshape(-1), (Fs - sh).reshape(-1, 3))
        np.add.at(A[:, 1], p.reshape(-1), sh.reshape(-1, 3))
        ft, on, gap = self.end_terms()
        A[on, 0] = A[on, 0] - ft[on]
        A[on, 1] = A[on, 1] + ft[on]
        self.sums = A
        # node gather: ascending (segment, side)
        S = np.zeros((n, 3))
        np.add.at(S, self.ends.reshape(-1), A.reshape(-1, 3))
        touched = np.zeros(n, bool)
        touched[self.ends.reshape(-1)] = True
        if external is None:
            out = S
        else:
            out = np.array(external, dtype=np.float64).reshape(n, 3)
            out[touched] = out[touched] + S[touched]
        ov = -gap[on]
        mx = max(self.stats[0], float(ov.max())) if on.any() and ov.max() > 0.0 else self.stats[0]
        self.stats = (mx, self.stats[1])
        return out

    def force_pass(self, x, external=None):
        """segment view at x, linker pass, reduction -> (node force, (max_overlap, count))"""
        self.segment_view(x)
        self.linker_pass()
        f = self.reduce(external=external)
        return f, self.stats

    def forms(self):
        """per linker: both closest points interior / an end node involved / the colinear branch (boolean arrays)"""
        seg, p = self.seg, self.pairs
        u = seg[p[:, 0], 3:6] - seg[p[:, 0], 0:3]
        v = seg[p[:, 1], 3:6] - seg[p[:, 1], 0:3]
        a, b, c = dot(u, u), dot(u, v), dot(v, v)
        colinear = (a * c - b * b) < COLINEAR_D
        inner = lambda q: (q > 0.0) & (q < 1.0)  # noqa: E731
        interior = ~colinear & inner(self.s) & inner(self.t)
        return interior, ~colinear & ~interior, colinear


# ---- the three cases -----------------------------------------------------------------------------------------------------
RADIUS, SKIN = 0.5, 0.3
CASES = ("jittered_lattice", "exact_lattice", "random_walks")


def backbone_segments(node_ptr):
    node_ptr = np.asarray(node_ptr, dtype=np.int64)
    out = [np.stack([np.arange(a, b - 1), np.arange(a + 1, b)], axis=1) for a, b in zip(node_ptr[:-1], node_ptr[1:])]
    return np.concatenate(out).astype(np.int32) if out else np.zeros((0, 2), np.int32)


def lattice(side, beads, pitch, spacing, jitter, seed):
    """side x side straight chains of `beads` beads along x (hp1_case's layout)"""
    g = np.stack(np.meshgrid(np.arange(beads) * pitch, np.arange(side) * spacing, np.arange(side) * spacing,
                             indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3))
    if jitter:
        c = c + np.random.default_rng(seed).normal(size=c.shape) * jitter
    return np.ascontiguousarray(c), np.arange(side * side + 1) * beads


def random_walks(chains, beads, box, seed):
    """`chains` walks of unit steps in uniformly random directions from uniformly random starts in [0, box)^3"""
    rng = np.random.default_rng(seed)
    start = rng.uniform(0.0, box, size=(chains, 1, 3))
    step = rng.normal(size=(chains, beads - 1, 3))
    step /= np.linalg.norm(step, axis=2, keepdims=True)
    c = np.concatenate([start, start + np.cumsum(step, axis=1)], axis=1)
    return np.ascontiguousarray(c.reshape(-1, 3)), np.arange(chains + 1) * beads


_CASES = {}


def case(name):
    """-> dict(center [n, 3], ends int32 [m, 2], n, m); built once"""
    if name not in _CASES:
        if name == "jittered_lattice":
            c, ptr = lattice(4, 40, 0.9, 0.9, 0.03, 5)
        elif name == "exact_lattice":
            c, ptr = lattice(3, 30, 0.9, 0.9, 0.0, None)
        elif name == "random_walks":
            c, ptr = random_walks(24, 30, 6.0, 7)
        else:
            raise ValueError(name)
        ends = backbone_segments(ptr)
        _CASES[name] = dict(center=c, ends=ends, n=c.shape[0], m=ends.shape[0])
    return _CASES[name]


_MODELS = {}


def evaluated(name, kind, end_correction=None):
    """the model of a case after update and force_pass at its centres (shared, read-only)"""
    key = (name, kind, end_correction)
    if key not in _MODELS:
        cs = case(name)
        mod = SegmentContacts(cs["n"], cs["ends"], kind, RADIUS, SKIN, end_correction=end_correction)
        mod.update(cs["center"])
        mod.node_force, _ = mod.force_pass(cs["center"])
        _MODELS[key] = mod
    return _MODELS[key]
