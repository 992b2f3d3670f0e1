"""numpy restatement of the chain step's kernels (chain.hip): Philox4x32-10, the uniform -> normal map, the Brownian
velocity, the drag velocity and the Hookean / FENE spring forces, in the operations and order the library documents
(include/mundy_hip.h).  Integer arithmetic is exact; the float expressions round like the device code."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
_M32 = np.uint64(0xFFFFFFFF)
TWO_PI = 6.283185307179586

# Random123 kat_vectors (philox4x32_10): (counter words, key words, result words); confirmed against an independent
# implementation of the generator
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


def philox_words(c, k):
    """c [n, 4], k [n, 2] uint32 words (any int dtype) -> [n, 4] uint32: ten rounds, key bumped between rounds"""
    c = [np.asarray(c)[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = (np.asarray(k)[:, i].astype(np.uint64) for i in range(2))
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k0) & _M32, p1 & _M32, ((p0 >> np.uint64(32)) ^ c[3] ^ k1) & _M32,
             p0 & _M32]
    return np.stack(c, axis=1).astype(np.uint32)


def philox(keys, counters, block):
    """the library's keying: key (lo32, hi32), counter (lo32, hi32, block, 0); keys / counters uint64 [n]"""
    k = np.asarray(keys).astype(np.uint64)
    c = np.asarray(counters).astype(np.uint64)
    n = k.shape[0]
    cw = np.stack([c & _M32, c >> np.uint64(32), np.full(n, block, np.uint64), np.zeros(n, np.uint64)], axis=1)
    kw = np.stack([k & _M32, k >> np.uint64(32)], axis=1)
    return philox_words(cw, kw)


def box_muller(w):
    """[n, 4] uint32 words -> two normals per row (z0, z1)"""
    w = w.astype(np.uint64)
    m = (w[:, 0] << np.uint64(21)) | (w[:, 1] >> np.uint64(11))
    mp = (w[:, 2] << np.uint64(21)) | (w[:, 3] >> np.uint64(11))
    u1 = (m + np.uint64(1)).astype(np.float64) * 2.0 ** -53
    u2 = mp.astype(np.float64) * 2.0 ** -53
    rad = np.sqrt(-2.0 * np.log(u1))
    th = TWO_PI * u2
    return rad * np.cos(th), rad * np.sin(th)


def normals(keys, counters):
    """the three normals a body draws at (key, counter): blocks 0 and 1, first three of four"""
    z0, z1 = box_muller(philox(keys, counters, 0))
    z2, _ = box_muller(philox(keys, counters, 1))
    return np.stack([z0, z1, z2], axis=1)


def brownian_velocity(keys, counters, kt, dt, mob_trans, velocity):
    """-> (velocity with rows 0..2 += sqrt(2 kt m_t / dt) z, counters + 1)"""
    v = np.array(velocity, dtype=np.float64, copy=True)
    coef = np.sqrt(2.0 * kt * np.asarray(mob_trans) / dt)
    z = normals(keys, counters)
    v[:, :3] = v[:, :3] + coef[:, None] * z
    return v, (np.asarray(counters).astype(np.uint64) + np.uint64(1))


def drag_velocity(mob_trans, force):
    v = np.zeros((len(mob_trans), 6))
    if force is not None:
        v[:, :3] = np.asarray(mob_trans)[:, None] * force
    return v


def spring_terms(pairs, kind, k, r, center):
    """per spring: (term [m, 3] that body i receives, L [m]); body j receives -term"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    m = p.shape[0]
    k = np.broadcast_to(np.asarray(k, dtype=np.float64), (m,))
    r = np.broadcast_to(np.asarray(r, dtype=np.float64), (m,))
    d = center[p[:, 1]] - center[p[:, 0]]
    L = np.sqrt(d[:, 0] * d[:, 0] + (d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == "hookean":
            fm = k * (L - r) * (1.0 / L)
        else:
            q = L / r
            fm = np.where(L < r, k / (1.0 - q * q), np.nan)
    return fm[:, None] * d, L


def spring_force(n, pairs, kind, k, r, center):
    """-> (force [n, 3], overstretched, max_length): each body adds its terms in ascending spring index from +0.0"""
    p = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    term, L = spring_terms(p, kind, k, r, center)
    m = p.shape[0]
    body = np.concatenate([p[:, 0], p[:, 1]])
    sidx = np.concatenate([np.arange(m), np.arange(m)])
    sign = np.concatenate([np.ones(m, bool), np.zeros(m, bool)])
    order = np.lexsort((sidx, body))
    body, sidx, sign = body[order], sidx[order], sign[order]
    start = np.searchsorted(body, np.arange(n))
    rank = np.arange(body.shape[0]) - start[body]
    f = np.zeros((n, 3))
    for slot in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == slot
        t = term[sidx[sel]]
        b = body[sel]
        s = sign[sel][:, None]
        f[b] = np.where(s, f[b] + t, f[b] - t)
    over = int((~(L < np.asarray(r))).sum()) if kind == "fene" else 0
    mx = float(np.max(np.where(np.isnan(L), 0.0, L))) if m else 0.0
    return f, over, max(mx, 0.0)


def fene_energy(L, k, r_max):
    """U = -1/2 k r_max^2 ln(1 - (L / r_max)^2)"""
    return -0.5 * k * r_max * r_max * np.log(1.0 - (L / r_max) ** 2)
