"""The double-double sums of the solve against math.fsum, bit for bit.

Every sum that feeds an iterate is claimed to be a double-double pair rounded once (mhip_internal.hpp): the correctly
rounded exact sum while sum|terms| / |sum| <= 2^40.  Here that claim is pinned on ill-conditioned data for the S1
reductions behind diff_dot, bb_step and residual (n at the wave, block and grid-stride edges) and for the per-body force
and torque sums of the body sweep (spheres, vector arms, rods; hub bodies at the activity-mask and general-incidence
edges; every work mapping).  The terms are computed with numpy by the device's per-term expressions (the device is built
with -ffp-contract=off), so only the summation is under test.  An overflowing or NaN sum is reported as the plain sum
would be."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_GRID = 2048 * 256      # kMaxGrid workgroups of kBlock threads: the S1 reductions go grid-stride beyond
S1_SIZES = [1, 63, 64, 65, 256, 257, MAX_GRID - 1, MAX_GRID, MAX_GRID + 1, 3_000_000]


@pytest.fixture(scope="module")
def ops():
    from mundy_amd import ops as o
    return o


def _bits(v):
    return np.float64(v).view(np.uint64)


def _exact(terms):
    """the correctly rounded sum (+0.0 for an empty or cancelling sum: the device's pair starts at +0.0)"""
    return math.fsum(terms) + 0.0


def _s1_vectors(rng, n, max_log2_cond=40):
    """x1, x2, y1, y2 whose products (x1 - x2)(y1 - y2) spread over 10^-15 .. 10^3, with pairs of large products of
    opposite sign at random positions on top (as _conditioned_system in test_gpu_primitives.py builds them): the sum
    cancels to sum|t| / |sum t| in [2^30, 2^40] once n allows pairs"""
    x2, y2 = rng.normal(size=n), rng.normal(size=n)
    sgn = lambda: rng.choice([-1.0, 1.0], n)  # noqa: E731
    x1 = x2 + sgn() * 10.0 ** rng.uniform(-7.5, 1.5, n)
    y1 = y2 + sgn() * 10.0 ** rng.uniform(-7.5, 1.5, n)
    if n < 3:
        return x1, x2, y1, y2
    npairs = min(32, n // 3)
    idx = rng.choice(n, 2 * npairs, replace=False)
    base = math.fsum((x1 - x2) * (y1 - y2))
    d2 = y1 - y2
    for a, b in zip(idx[::2], idx[1::2]):
        m = 2.0 ** rng.uniform(30, 44) * abs(base) / (2 * npairs) * rng.uniform(0.5, 1.0)
        x1[a] = x2[a] + m / d2[a]
        x1[b] = x2[b] - m / d2[b]                      # cancels the product at a up to the roundings
    while True:
        t = (x1 - x2) * (y1 - y2)
        s = math.fsum(t)
        if s != 0.0 and np.abs(t).sum() <= 2.0 ** max_log2_cond * abs(s):
            break
        x1[idx] = x2[idx] + 0.5 * (x1[idx] - x2[idx])
    return x1, x2, y1, y2


@pytest.mark.parametrize("n", S1_SIZES)
def test_s1_reductions_are_the_correctly_rounded_sum(ops, oracle, n):
    from gpu_util import dev
    rng = np.random.default_rng(4000 + n % 1000)
    x1, x2, y1, y2 = _s1_vectors(rng, n)
    d1, d2 = x1 - x2, y1 - y2
    t = d1 * d2
    cond = np.abs(t).sum() / abs(math.fsum(t))
    assert cond <= 2.0 ** 40 and (n < 63 or cond >= 2.0 ** 30), cond
    assert np.abs(t).max() / np.abs(t).min() > 1e15 or n < 63          # the terms do spread
    dot4 = _exact(t)
    dot2 = _exact(d1 * d1)
    bb_eps = 1e-15 * 10                                               # kBBEps: bb_step's guard of a tiny den
    den = dot4 + bb_eps * (1.0 if abs(dot4) < bb_eps else 0.0)
    perm = rng.permutation(n)
    for name, (a, b, c, d) in (("as built", (x1, x2, y1, y2)), ("permuted", (x1[perm], x2[perm], y1[perm], y2[perm]))):
        A, B, Cc, D = dev(a), dev(b), dev(c), dev(d)
        assert _bits(ops.diff_dot(A, B, Cc, D)) == _bits(dot4), (name, ops.diff_dot(A, B, Cc, D), dot4)
        assert _bits(ops.diff_dot(A, B)) == _bits(dot2), (name, ops.diff_dot(A, B), dot2)
        # bb_step(x_old, g_old, x, g) = sum (x - x_old)^2 / sum (x - x_old)(g - g_old), each sum rounded once
        assert _bits(ops.bb_step(B, D, A, Cc)) == _bits(dot2 / den), (name, ops.bb_step(B, D, A, Cc), dot2 / den)
        for kind in (0, 1):
            # a max is exact in any order
            assert _bits(ops.residual(kind, A, Cc, (1, 0.0, 0.0))) == _bits(oracle.residual(kind, a, c, (1, 0.0, 0.0)))


def test_s1_overflow_and_nan_are_reported_as_the_plain_sum(ops):
    # dd_value: a sum whose pair overflowed or met NaN is the plain sum's value (the lo word is NaN there)
    from gpu_util import dev
    inf = float("inf")
    n = 1000
    z = np.zeros(n)
    one = np.ones(n)
    for where in (0, 517, n - 1):
        x = np.ones(n)
        x[where] = inf
        assert ops.diff_dot(dev(x), dev(z), dev(one), dev(z)) == inf            # one term +inf
        assert ops.diff_dot(dev(-x), dev(z), dev(one), dev(z)) == -inf          # one term -inf
        assert ops.diff_dot(dev(x), dev(z)) == inf
        x2 = x.copy()
        x2[(where + 300) % n] = -inf
        assert math.isnan(ops.diff_dot(dev(x2), dev(z), dev(one), dev(z)))     # +inf and -inf
    big = np.zeros(n)
    big[[3, 700]] = 1.3e154                                                   # squares 1.69e308: finite, their sum not
    assert ops.diff_dot(dev(big), dev(z)) == inf


# ---- the body sweep's per-body sums ------------------------------------------------------------------------------------
HUB_DEGREES = (1, 64, 65, 150, 2500)    # one contact; the 64-slot activity mask and one past it; > kArrangeMaxList = 1024


def _hub_system(rng, kin):
    """hubs of the degrees above, each touched by leaves of degree 1 (either side of the pair); x >= 0 with exact
    zeros; normals in +-n pairs on every hub so that its force cancels to 2^-30 .. 2^-40 of sum|terms|"""
    H = len(HUB_DEGREES)
    pairs, nrm, x = [], [], []
    leaf = H
    for h, deg in enumerate(HUB_DEGREES):
        src = rng.random(deg) < 0.5                  # hub as the source (force -x n) or the target (+x n)
        sign = np.where(src, -1.0, 1.0)
        xs = 10.0 ** rng.uniform(-3, 3, deg)
        ns = rng.normal(size=(deg, 3))
        ns /= np.linalg.norm(ns, axis=1, keepdims=True)
        for k in range(0, deg - 1, 2):
            # the hub's share of contact k+1 is minus that of contact k, up to 2^-e
            ns[k + 1] = -sign[k] * sign[k + 1] * ns[k]
            xs[k + 1] = xs[k] * (1.0 + 2.0 ** -rng.uniform(30, 40))
            if rng.random() < 0.1:
                xs[k] = xs[k + 1] = 0.0              # inactive: exact zeros, skipped
        if deg % 2 and deg > 1:
            xs[-1] *= 2.0 ** -40                      # the odd one out, small
        for k in range(deg):
            pairs.append((h, leaf) if src[k] else (leaf, h))
            leaf += 1
        nrm.append(ns)
        x.append(xs)
    pairs = np.array(pairs, dtype=np.int32)
    perm = rng.permutation(len(pairs))              # contacts in no particular order
    pairs, nrm, x = pairs[perm], np.concatenate(nrm)[perm], np.concatenate(x)[perm]
    N = leaf
    C = len(pairs)
    S = dict(N=N, pairs=np.ascontiguousarray(pairs), normal=np.ascontiguousarray(nrm), x=x,
             mt=rng.uniform(0.5, 2.0, N), mr=rng.uniform(0.5, 2.0, N))
    if kin == "rigid":
        S["ra"], S["rb"] = rng.normal(size=(C, 3)), rng.normal(size=(C, 3))
    if kin == "rod":
        p0 = rng.normal(size=(N, 3)) * 10
        seg = np.concatenate([p0, p0 + rng.normal(size=(N, 3)), rng.uniform(0.2, 0.5, (N, 2))], axis=1)
        # arclengths, some outside [0, 1] (clamped by the operator)
        S.update(seg=np.ascontiguousarray(seg), s=rng.uniform(-0.1, 1.1, C), t=rng.uniform(-0.1, 1.1, C))
    return S


def _cross(a, b):
    # V3 cross of mhip_internal.hpp, component by component
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _rows_reference(S, kin):
    """(U, W) per body from the per-term expressions of k_body: f = +-(x n) (source -, target +); spheres U = m_t
    fsum(f); vector arms W = m_r fsum(r x f) with r = ra at the source, rb at the target; rods S = fsum(coef f) with
    coef = clamp(arclength, 0, 1) - 1/2, then w = m_r (u x S), u = p1 - p0"""
    pairs, x, n = S["pairs"], S["x"], S["normal"]
    N = S["N"]
    out = np.zeros((N, 6))
    f = x[:, None] * n
    sides = []
    for side, sgn in ((0, -1.0), (1, 1.0)):
        sl = dict(body=pairs[:, side], f=sgn * f)
        if kin == "rigid":
            sl["tq"] = _cross(S["ra"] if side == 0 else S["rb"], sl["f"])
        if kin == "rod":
            coef = np.clip(S["s"] if side == 0 else S["t"], 0.0, 1.0) - 0.5
            sl["tq"] = coef[:, None] * sl["f"]
        sides.append(sl)
    terms_f = [[[] for _ in range(3)] for _ in range(N)]
    terms_t = [[[] for _ in range(3)] for _ in range(N)]
    for sl in sides:
        for c in range(len(pairs)):
            if x[c] == 0.0:
                continue                              # an inactive contact is never added
            b = sl["body"][c]
            for k in range(3):
                terms_f[b][k].append(sl["f"][c, k])
                if kin != "trans":
                    terms_t[b][k].append(sl["tq"][c, k])
    F = np.array([[_exact(terms_f[b][k]) for k in range(3)] for b in range(N)])
    out[:, :3] = S["mt"][:, None] * F
    if kin != "trans":
        T = np.array([[_exact(terms_t[b][k]) for k in range(3)] for b in range(N)])
        if kin == "rod":
            u = S["seg"][:, 3:6] - S["seg"][:, 0:3]
            T = _cross(u, T)
        out[:, 3:] = S["mr"][:, None] * T
    return out, F


def _hub_op(ops, S, kin):
    from gpu_util import dev
    if kin == "trans":
        return ops.ContactOperator(dev(S["pairs"]), dev(S["normal"]), dev(S["mt"]), 1.0)
    if kin == "rigid":
        return ops.ContactOperator(dev(S["pairs"]), dev(S["normal"]), dev(S["mt"]), 1.0, ra=dev(S["ra"]),
                                   rb=dev(S["rb"]), mob_rot=dev(S["mr"]))
    return ops.ContactOperator(dev(S["pairs"]), dev(S["normal"]), dev(S["mt"]), 1.0, mob_rot=dev(S["mr"]),
                               rod=(dev(S["s"]), dev(S["t"]), dev(S["seg"])))


@pytest.mark.parametrize("kin", ["trans", "rigid", "rod"])
def test_body_rows_are_the_correctly_rounded_sums(ops, kin):
    from gpu_util import assert_bits_equal, dev, host
    rng = np.random.default_rng({"trans": 71, "rigid": 72, "rod": 73}[kin])
    S = _hub_system(rng, kin)
    ref, F = _rows_reference(S, kin)
    H = len(HUB_DEGREES)
    deg = np.bincount(S["pairs"].ravel(), minlength=S["N"])
    assert tuple(deg[:H]) == HUB_DEGREES and (deg[H:] == 1).all()
    # the hubs' forces cancel: sum|terms| / |sum| between 2^30 and 2^40+ (degree > 1, odd degrees a little less)
    f = S["x"][:, None] * S["normal"]
    for h in range(1, H):
        mask = (S["pairs"] == h).any(axis=1)
        ratio = np.abs(f[mask]).sum() / np.abs(F[h]).max()
        assert ratio >= 2.0 ** 25, (HUB_DEGREES[h], ratio)
    op = _hub_op(ops, S, kin)
    x = dev(S["x"])
    for xcd_tile, lanes in ((0, 2), (32, 4), (5, 8), (8, 16), (-1, -1)):
        op.set_work_mapping(xcd_tile, lanes)
        got = host(op.body_velocity_of(x))
        cols = slice(0, 3) if kin == "trans" else slice(0, 6)
        assert_bits_equal(got[:, cols], ref[:, cols], "%s rows under mapping %s" % (kin, (xcd_tile, lanes)))
    op.close()


@pytest.mark.parametrize("kin", ["trans", "rigid"])
def test_body_row_overflow_and_nan_are_reported_as_the_plain_sum(ops, kin):
    from gpu_util import dev, host
    rng = np.random.default_rng(5)
    S = _hub_system(rng, kin)
    op = _hub_op(ops, S, kin)
    pairs, n = S["pairs"], S["normal"]
    hub = 3                                             # degree 150
    at_hub = np.flatnonzero((pairs == hub).any(axis=1))
    assert (np.abs(n[at_hub]) > 0).all()                # (no inf * 0 terms)
    inf = float("inf")
    x = S["x"].copy()
    x[at_hub[0]] = inf
    sgn = -1.0 if pairs[at_hub[0], 0] == hub else 1.0
    got = host(op.body_velocity_of(dev(x)))
    np.testing.assert_array_equal(got[hub, :3], S["mt"][hub] * sgn * np.sign(n[at_hub[0]]) * inf)
    # a second contact of the hub pushing the other way with an infinite multiplier: +inf + -inf, NaN
    sgn2 = -1.0 if pairs[at_hub[1], 0] == hub else 1.0
    x[at_hub[1]] = inf
    nn = n.copy()
    nn[at_hub[1]] = -sgn * sgn2 * n[at_hub[0]]
    S2 = dict(S, normal=nn)
    op2 = _hub_op(ops, S2, kin)
    got = host(op2.body_velocity_of(dev(x)))
    assert np.isnan(got[hub, :3]).all()
    op.close()
    op2.close()
