"""Synthetic inputs for the contact hot path (numpy, host side).

The reference draws inputs from OpenRAND Philox keyed (seed, body index) (scrap/lcp_spheres/NgpLcp.cpp:810-833,
mundy_geom/randomize.hpp:56-300).  OpenRAND is not available, so this is an own counter-based generator with the same
keying: every value is a pure function of (seed, body index, stream), hence identical on every rank and for every
partition of the bodies.  Input streams are therefore not reproducible against OpenRAND (harmless: the same arrays
feed the CPU oracle and the GPU path).
"""
import numpy as np

_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    """splitmix64 finaliser on uint64 arrays"""
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & _M64
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return z ^ (z >> np.uint64(31))


def uniform01(seed, index, stream):
    """U[0,1) doubles, a pure function of (seed, index, stream); index is an integer array"""
    idx = np.asarray(index, dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = _mix(np.uint64(seed) * np.uint64(0xD1342543DE82EF95) + np.uint64(stream))
        z = _mix(_mix(idx ^ key) + np.uint64(stream) * np.uint64(0x2545F4914F6CDD1D))
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def box_edge(n, body_volume, volume_fraction):
    return float((n * body_volume / volume_fraction) ** (1.0 / 3.0))


def spheres(n, radius=1.0, volume_fraction=0.40, seed=1234, first=0):
    """n spheres, centres uniform in [0, L)^3 (generate_random_point, randomize.hpp:57-64); monodisperse r as
    NgpLcp.cpp:849.  Returns dict(center [n,3], radius [n], box L)."""
    idx = np.arange(first, first + n)
    L = box_edge(n, 4.0 / 3.0 * np.pi * radius ** 3, volume_fraction)
    c = np.stack([uniform01(seed, idx, s) * L for s in (0, 1, 2)], axis=1)
    return dict(center=np.ascontiguousarray(c), radius=np.full(n, float(radius)), box=L)


def spherocylinder_centers(indices, n_total, radius=0.5, length=2.0, volume_fraction=0.40, seed=1234):
    """centres only, for explicit global indices (used to order a large system before a rank materialises its slice)"""
    idx = np.asarray(indices)
    vol = np.pi * radius ** 2 * length + 4.0 / 3.0 * np.pi * radius ** 3
    L = box_edge(n_total, vol, volume_fraction)
    return np.ascontiguousarray(np.stack([uniform01(seed, idx, s) * L for s in (0, 1, 2)], axis=1)), L


def spherocylinders(n, radius=0.5, length=2.0, volume_fraction=0.40, seed=1234, first=0, n_total=None, indices=None):
    """n spherocylinders (centre, unit quaternion, radius, length).  Orientation: axis u uniform on the sphere,
    q = quat_from_parallel_transport(zhat, u) (randomize.hpp:79-84, Quaternion.hpp:1489-1505).  Body volume
    pi r^2 L + 4/3 pi r^3; the box edge comes from n_total (default n) so shards of one system share a box."""
    idx = np.arange(first, first + n) if indices is None else np.asarray(indices)
    n = len(idx)
    vol = np.pi * radius ** 2 * length + 4.0 / 3.0 * np.pi * radius ** 3
    L = box_edge(n if n_total is None else n_total, vol, volume_fraction)
    c = np.stack([uniform01(seed, idx, s) * L for s in (0, 1, 2)], axis=1)
    z = 2.0 * uniform01(seed, idx, 3) - 1.0
    phi = 2.0 * np.pi * uniform01(seed, idx, 4)
    z = np.clip(z, -1.0 + 1e-9, 1.0)  # u = -zhat makes the parallel-transport quaternion singular
    st = np.sqrt(1.0 - z * z)
    u = np.stack([st * np.cos(phi), st * np.sin(phi), z], axis=1)
    # quat_from_parallel_transport(zhat, u): w = sqrt((1 + z.u)/2), xyz = 0.5 (zhat x u) / w
    w = np.sqrt(0.5 * (1.0 + u[:, 2]))
    q = np.stack([w, 0.5 * (-u[:, 1]) / w, 0.5 * (u[:, 0]) / w, np.zeros(n)], axis=1)
    return dict(center=np.ascontiguousarray(c), quat=np.ascontiguousarray(q), radius=np.full(n, float(radius)),
                length=np.full(n, float(length)), box=L)


def aligned_spherocylinders(n, radius=0.5, length=2.0, volume_fraction=0.40, seed=1234, axis=(0.0, 0.0, 1.0)):
    """n PARALLEL spherocylinders (a nematic packing: every pair takes the colinear branch of the segment-segment
    distance, LineSegmentLineSegment.hpp:215-265 -- end-to-end pairs with an unclamped parameter, side-by-side pairs
    with overlapping projections).  Centres uniform in the box of the requested volume fraction; one common axis."""
    b = spherocylinders(n, radius, length, volume_fraction, seed)
    u = np.asarray(axis, dtype=np.float64)
    u = u / np.linalg.norm(u)
    # quat_from_parallel_transport(zhat, u)  (Quaternion.hpp:1489-1505)
    w = np.sqrt(0.5 * (1.0 + u[2]))
    q = np.array([w, 0.5 * (-u[1]) / w, 0.5 * u[0] / w, 0.0])
    b["quat"] = np.ascontiguousarray(np.tile(q, (n, 1)))
    return b


def mixed_bodies(n, volume_fraction=0.40, seed=1234, sphere_radius=0.5, rod=(0.5, 2.0), ellipsoid=(0.8, 0.5, 0.4)):
    """BASELINE configs[4]: n bodies, kind = index mod 3 (0 sphere, 1 spherocylinder, 2 ellipsoid), centres uniform
    in the box that gives the requested volume fraction, orientations uniform (unit quaternions from 4 normal
    deviates via Box-Muller on the counter-based stream).  shape rows: (r,0,0) / (r,L,0) / (r1,r2,r3)."""
    idx = np.arange(n)
    kind = (idx % 3).astype(np.int32)
    vols = np.array([4.0 / 3.0 * np.pi * sphere_radius ** 3,
                     np.pi * rod[0] ** 2 * rod[1] + 4.0 / 3.0 * np.pi * rod[0] ** 3,
                     4.0 / 3.0 * np.pi * ellipsoid[0] * ellipsoid[1] * ellipsoid[2]])
    L = float((vols[kind].sum() / volume_fraction) ** (1.0 / 3.0))
    c = np.stack([uniform01(seed, idx, s) * L for s in (0, 1, 2)], axis=1)
    u = [np.maximum(uniform01(seed, idx, 10 + s), 1e-300) for s in range(4)]
    g = np.stack([np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
                  np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])],
                 axis=1)
    q = g / np.linalg.norm(g, axis=1, keepdims=True)
    shape = np.zeros((n, 3))
    shape[kind == 0] = [sphere_radius, 0.0, 0.0]
    shape[kind == 1] = [rod[0], rod[1], 0.0]
    shape[kind == 2] = list(ellipsoid)
    return dict(kind=kind, center=np.ascontiguousarray(c), quat=np.ascontiguousarray(q), shape=shape, box=L)


def dry_mobility(radius, viscosity=1e-3, bounding_radius=None):
    """dry local drag (NgpLcp.cpp:484-486; Bacteria.cpp:810-848): U = F / (6 pi mu r), W = T / (8 pi mu r^3).
    For rods the effective radius is the bounding radius when given."""
    r = np.asarray(radius if bounding_radius is None else bounding_radius, dtype=np.float64)
    return 1.0 / (6.0 * np.pi * viscosity * r), 1.0 / (8.0 * np.pi * viscosity * r ** 3)


def chains(num_chains, beads_per_chain, r0=1.0, radius=0.5, seed=1234, cell=None):
    """Random-walk bead-spring chains (the chromatin model of NgpHP1.cpp with the numbers of its ngp_hp1.yaml: r = 0.5,
    r0 = 1, k = 3, kT = 0.1, mu = 1, dt = 1e-3, skin 1.0).  Chain c walks inside its own cubic cell of a lattice (edge
    `cell`, default ~ 2.5 radii of gyration + 2 r), bead to bead at distance exactly r0 in uniformly drawn directions,
    redrawing any step that would leave the cell's interior shrunk by r: beads of different chains never overlap (beads
    of one chain may).  Returns dict(center [n, 3], radius [n], pairs int32 [n - num_chains, 2] (bead b -> b + 1 along
    each chain), chain [n] int32, plus the app's parameters k, kt, viscosity, dt, skin, r0)."""
    rng = np.random.default_rng(seed)
    B, M = int(beads_per_chain), int(num_chains)
    if cell is None:
        cell = 2.0 * radius + max(2.0 * r0, 2.5 * r0 * np.sqrt(max(B, 1) / 6.0) * 2.0)
    side = int(np.ceil(M ** (1.0 / 3.0))) if M else 0
    idx = np.arange(M)
    lo = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1).astype(np.float64) * cell \
        if M else np.zeros((0, 3))
    inner_lo, inner_hi = lo + radius, lo + cell - radius
    pos = np.empty((M, B, 3))
    if B:
        pos[:, 0] = lo + 0.5 * cell
    for b in range(1, B):
        prev = pos[:, b - 1]
        nxt = np.empty_like(prev)
        todo = np.ones(M, dtype=bool)
        while todo.any():
            k = int(todo.sum())
            u = rng.normal(size=(k, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            cand = prev[todo] + r0 * u
            ok = ((cand >= inner_lo[todo]) & (cand <= inner_hi[todo])).all(axis=1)
            sel = np.flatnonzero(todo)[ok]
            nxt[sel] = cand[ok]
            todo[sel] = False
        pos[:, b] = nxt
    center = np.ascontiguousarray(pos.reshape(-1, 3))
    first = np.arange(M)[:, None] * B + np.arange(B - 1)[None, :] if B > 1 else np.zeros((M, 0), dtype=np.int64)
    pairs = np.ascontiguousarray(np.stack([first.reshape(-1), first.reshape(-1) + 1], axis=1).astype(np.int32))
    return dict(center=center, radius=np.full(M * B, float(radius)), pairs=pairs,
                chain=np.repeat(np.arange(M, dtype=np.int32), B), k=3.0, kt=0.1, viscosity=1.0, dt=1e-3, skin=1.0,
                r0=float(r0))


def triad_quaternion(d1, d2, d3):
    """rotation_matrix_to_quaternion (mundy_math/Quaternion.hpp:1410-1427) of the matrix with the columns d1, d2, d3
    [m, 3] each -> (w, x, y, z) [m, 4]"""
    D00, D11, D22 = d1[:, 0], d2[:, 1], d3[:, 2]
    half = lambda v: np.sqrt(np.maximum(0.0, v)) / 2.0  # noqa: E731
    w = half(1.0 + D00 + D11 + D22)
    x = np.copysign(half(1.0 + D00 - D11 - D22), d2[:, 2] - d3[:, 1])   # D21 - D12
    y = np.copysign(half(1.0 - D00 + D11 - D22), d3[:, 0] - d1[:, 2])   # D02 - D20
    z = np.copysign(half(1.0 - D00 - D11 + D22), d1[:, 1] - d2[:, 0])   # D10 - D01
    return np.stack([w, x, y, z], axis=1)


def filaments(num_filaments, nodes, radius=0.5, segment_length=1.0, rest_curvature=(0.0, 0.0, 0.0), seed=None):
    """Straight filaments laid out as the sperm apps' declare_and_initialize_sperm does
    (CollidingOverdampedFrictionalSperm.cpp:688-1072): filament j in the plane x = 0 at y = 2 j (2 radius), along +z from
    z = 0, the even-numbered ones flipped (from z = segment_length (nodes - 1) along -z); node i at tail + axis i
    segment_length with arclength i segment_length; every edge's orientation from the triad d1 = (+-1, 0, 0) (-1 for a
    flipped filament), d3 = the tangent, d2 = d3 x d1 / |d3 x d1| (:1057-1068).  seed: the phase of filament j is
    2 pi uniform01(seed, j, 0) (the reference draws 2 pi rng.rand() from OpenRAND); None = no phases.
    Returns dict(node_ptr int32 [F + 1], center [N, 3], twist [N], radius [N], rest_curvature [N, 3], arclength [N],
    edge_orientation [N, 4] (w, x, y, z; the slot of a filament's last node holds the identity), phase [F] or None)."""
    F, B = int(num_filaments), int(nodes)
    if B < 2:
        raise ValueError("a filament has at least 2 nodes, got %d" % B)
    j = np.arange(F, dtype=np.float64)
    flip = (np.arange(F) % 2 == 0)
    i = np.arange(B, dtype=np.float64)
    tail = np.stack([np.zeros(F), 2.0 * j * (2.0 * radius), np.where(flip, segment_length * (B - 1), 0.0)], axis=1)
    axis = np.stack([np.zeros(F), np.zeros(F), np.where(flip, -1.0, 1.0)], axis=1)
    center = tail[:, None, :] + axis[:, None, :] * i[None, :, None] * segment_length
    d = center[:, 1:] - center[:, :-1]
    t = d / np.sqrt(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))[..., None]
    d1 = np.broadcast_to(np.stack([np.where(flip, -1.0, 1.0), np.zeros(F), np.zeros(F)], axis=1)[:, None, :], t.shape)
    d2 = np.cross(t, d1)
    d2 = d2 / np.sqrt(d2[..., 0] * d2[..., 0] + (d2[..., 1] * d2[..., 1] + d2[..., 2] * d2[..., 2]))[..., None]
    quat = np.zeros((F, B, 4))
    quat[..., 0] = 1.0
    quat[:, :-1] = triad_quaternion(d1.reshape(-1, 3), d2.reshape(-1, 3), t.reshape(-1, 3)).reshape(F, B - 1, 4)
    N = F * B
    phase = None if seed is None else 2.0 * np.pi * uniform01(seed, np.arange(F), 0)
    return dict(node_ptr=(np.arange(F + 1) * B).astype(np.int32), center=np.ascontiguousarray(center.reshape(N, 3)),
                twist=np.zeros(N), radius=np.full(N, float(radius)),
                rest_curvature=np.ascontiguousarray(np.broadcast_to(np.asarray(rest_curvature, dtype=np.float64), (N, 3))),
                arclength=np.tile(i * segment_length, F), edge_orientation=np.ascontiguousarray(quat.reshape(N, 4)),
                phase=phase)


def crossed_filaments(num_filaments, nodes, radius=0.5, segment_length=1.0, angle=0.5 * np.pi, overlap=0.125, pitch=None,
                      offset=None, seed=None):
    """Two layers of `num_filaments` straight filaments each, laid at an angle: the colliding filaments' test bed.
    Layer 0 lies in the plane x = 0: filament j at y = j pitch, along +z from z = 0 (pitch defaults to 4 radius + 2
    segment_length / nodes: parallel neighbours never touch).  Layer 1 is layer 0 turned by `angle` about the x axis
    through the centre of the patch and moved by `offset` (default (2 radius - overlap, 0, 0): every crossing is a
    contact of depth `overlap`).  Fields as synth.filaments returns them; layer 0 comes first."""
    F, B = int(num_filaments), int(nodes)
    if B < 2:
        raise ValueError("a filament has at least 2 nodes, got %d" % B)
    r, l0 = float(radius), float(segment_length)
    pitch = 4.0 * r + 2.0 * l0 / B if pitch is None else float(pitch)
    offset = np.array([2.0 * r - overlap, 0.0, 0.0] if offset is None else offset, dtype=np.float64)
    i = np.arange(B, dtype=np.float64)
    base = np.zeros((F, B, 3))
    base[:, :, 1] = (np.arange(F, dtype=np.float64) * pitch)[:, None]
    base[:, :, 2] = (i * l0)[None, :]
    mid = np.array([0.0, 0.5 * (F - 1) * pitch, 0.5 * (B - 1) * l0])
    ca, sa = np.cos(angle), np.sin(angle)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, ca, sa], [0.0, -sa, ca]])   # +z -> (0, sin a, cos a)
    top = (base - mid) @ rot.T + mid + offset
    center = np.concatenate([base, top]).reshape(2 * F * B, 3)
    tangent = np.repeat(np.stack([[0.0, 0.0, 1.0], rot @ np.array([0.0, 0.0, 1.0])]), F * B, axis=0)
    d1 = np.tile([1.0, 0.0, 0.0], (2 * F * B, 1))
    d2 = np.cross(tangent, d1)
    d2 = d2 / np.sqrt(d2[:, 0] * d2[:, 0] + (d2[:, 1] * d2[:, 1] + d2[:, 2] * d2[:, 2]))[:, None]
    quat = triad_quaternion(d1, d2, tangent).reshape(2 * F, B, 4)
    quat[:, -1] = (1.0, 0.0, 0.0, 0.0)
    N = 2 * F * B
    phase = None if seed is None else 2.0 * np.pi * uniform01(seed, np.arange(2 * F), 0)
    return dict(node_ptr=(np.arange(2 * F + 1) * B).astype(np.int32), center=np.ascontiguousarray(center),
                twist=np.zeros(N), radius=np.full(N, r), rest_curvature=np.zeros((N, 3)),
                arclength=np.tile(i * l0, 2 * F), edge_orientation=np.ascontiguousarray(quat.reshape(N, 4)), phase=phase)


def sphere_quadrature(order, radius, include_poles=False, invert=False):
    """gen_sphere_quadrature (periphery/Periphery.hpp:90-167) -> (points [S, 3], weights [S], normals [S, 3]): the
    Gauss-Legendre rule of order + 1 nodes in cos(theta) times 2 order + 2 equispaced azimuths, ring j from the north
    pole down (cos theta_j = nodes_gl[order - j]), k around (phi_k = 2 pi k / (2 order + 2)); weights
    radius^2 2 pi / (2 order + 2) weights_gl[order - j]; normals = +-points of the unit sphere (invert: inward); the
    points are scaled by the radius last.  include_poles adds the two poles with weight 0 (first and last).  The
    Gauss-Legendre rule is numpy.polynomial.legendre.leggauss (ascending nodes, as the reference's)."""
    order = int(order)
    if order < 0:
        raise ValueError("order must be non-negative, got %d" % order)
    if not (radius > 0):
        raise ValueError("radius must be positive, got %r" % (radius,))
    nodes_gl, weights_gl = np.polynomial.legendre.leggauss(order + 1)
    nphi = 2 * order + 2
    j = np.repeat(np.arange(order + 1), nphi)
    k = np.tile(np.arange(nphi), order + 1)
    cos_t = nodes_gl[order - j]
    phi = 2 * np.pi * k / nphi
    sin_t = np.sqrt(1 - cos_t * cos_t)
    points = np.stack([sin_t * np.cos(phi), sin_t * np.sin(phi), cos_t], axis=1)
    weights = (radius * radius * 2 * np.pi / nphi) * weights_gl[order - j]
    if include_poles:
        points = np.concatenate([[[0.0, 0.0, 1.0]], points, [[0.0, 0.0, -1.0]]])
        weights = np.concatenate([[0.0], weights, [0.0]])
    normals = (-1.0 if invert else 1.0) * points
    points = points * radius
    return np.ascontiguousarray(points), np.ascontiguousarray(weights), np.ascontiguousarray(normals)


def periphery_bind_sites(shape, radii, count, seed=1234):
    """The reference's RANDOM periphery bind sites (HP1.cpp:2907-2963), generated on the host once -> points
    [count, 3] on the surface, about the origin in the periphery's own frame.  shape "sphere" (radii: the radius, or
    three equal ones) or "ellipsoid" (radii: the semi-axes a, b, c).  Sphere: theta = 2 pi u1, phi = acos(2 u2 - 1),
    R (sin phi cos theta, sin phi sin theta, cos phi): uniform in area.  Ellipsoid: the same point of the unit sphere
    is kept iff sqrt((b c x)^2 + (a c y)^2 + (a b z)^2) / max(b c, a c, a b) > u3 (the area element of the push
    forward, so that the kept points are uniform in the ellipsoid's area) and then scaled by (a, b, c); a rejected
    attempt draws three new uniforms.  The uniforms are numpy's default_rng(seed), three per attempt (the sphere uses
    the first two): the reference's openrand stream is not pinned."""
    count = int(count)
    if count <= 0:
        raise ValueError("count must be > 0, got %r" % (count,))
    if shape not in ("sphere", "ellipsoid"):
        raise ValueError("shape must be 'sphere' or 'ellipsoid', got %r" % (shape,))
    r = np.atleast_1d(np.asarray(radii, dtype=np.float64))
    if shape == "sphere":
        if r.shape not in ((1,), (3,)) or not (r == r[0]).all():
            raise ValueError("a sphere takes one radius, got %r" % (radii,))
        r = np.full(3, r[0])
    if r.shape != (3,) or not (np.isfinite(r) & (r > 0.0)).all():
        raise ValueError("radii must be finite and > 0, got %r" % (radii,))
    a, b, c = (float(v) for v in r)
    rng = np.random.default_rng(seed)
    inv_mu_max = 1.0 / max(b * c, a * c, a * b)
    kept, have = [], 0
    while have < count:
        u = rng.random((count - have, 3))
        theta = 2.0 * np.pi * u[:, 0]
        phi = np.arccos(2.0 * u[:, 1] - 1.0)
        x, y, z = np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)
        if shape == "sphere":
            keep = np.ones(x.shape[0], bool)
        else:
            mu = np.sqrt((b * c * x) * (b * c * x) + (a * c * y) * (a * c * y) + (a * b * z) * (a * b * z))
            keep = inv_mu_max * mu > u[:, 2]
        kept.append(np.stack([a * x[keep], b * y[keep], c * z[keep]], axis=1))
        have += int(keep.sum())
    return np.ascontiguousarray(np.concatenate(kept)[:count])


def backbone_segments(node_ptr):
    """the backbone segments of contiguous chains: chain c holds the beads node_ptr[c] .. node_ptr[c + 1] - 1, and a
    segment joins every two consecutive beads of a chain -> ends int32 [m, 2], in bead order"""
    ptr = np.asarray(node_ptr, dtype=np.int64)
    if ptr.ndim != 1 or ptr.size < 1 or (np.diff(ptr) < 0).any():
        raise ValueError("node_ptr must be a non-decreasing 1-d array, got %r" % (node_ptr,))
    first = np.concatenate([np.arange(a, b - 1) for a, b in zip(ptr[:-1], ptr[1:])] or [np.zeros(0, np.int64)])
    return np.ascontiguousarray(np.stack([first, first + 1], axis=1).astype(np.int32))


def chain_triplets(node_ptr):
    """the angular springs of contiguous chains (ChainOfSprings.cpp:436-467): one for every interior bead i + 1 of a
    chain, in the reference's BEAM_3 node order, ends first and centre last -> triplets int32 [m, 3] = (i, i + 2, i + 1),
    in bead order"""
    ptr = np.asarray(node_ptr, dtype=np.int64)
    if ptr.ndim != 1 or ptr.size < 1 or (np.diff(ptr) < 0).any():
        raise ValueError("node_ptr must be a non-decreasing 1-d array, got %r" % (node_ptr,))
    first = np.concatenate([np.arange(a, b - 2) for a, b in zip(ptr[:-1], ptr[1:])] or [np.zeros(0, np.int64)])
    return np.ascontiguousarray(np.stack([first, first + 2, first + 1], axis=1).astype(np.int32))
