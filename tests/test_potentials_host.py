"""tests/potentials.py on the host: its two forms against each other, its geometry against cases worked by hand, and the
calibration of the tolerances of tests/test_gpu_force_gradients.py and tests/test_gpu_mobility_properties.py.

Calibration.  For every case of tests/gradient_cases.py, in its own frame and in the rotated and translated frame of the
equivariance test, -grad U by central differences in mpmath (h = 1e-15 at 50 digits) against the existing float64 numpy
model of the term; a body's deviation in units of eps S_b, S_b the sum of the
magnitudes of the terms that act on body b (mpmath's); for the mobility, a 3 x 3 block of hydro_model.pair_terms against
rpyc_tt in units of eps |block| (Frobenius).  K = four times the worst deviation of the term, rounded up to a power of
two: the factor leaves room for a device pow and sqrt that are good to an ulp where libm rounds correctly.  K is measured
here, from the model and the exact gradient, never from the device.  test_calibration prints this table again and asserts
that the model stays under K / 4.

    term                     worst deviation [eps S_b]     K
    springs                          3.33                  16
    crosslinkers                     3.69                  16
    active                           0.80                   4
    sphere wall                     13.6                   64
    ellipsoid wall                 108                    512
    ellipsoid wall, fast             1.24                   8
    sphere Hertz                    48.8                  256
    segment Hertz                    5.94                  32
    segment WCA                     35.7                  256
    rpyc (per block)                 2.88                  16

    delta = 1.752e-3 (measured 1.75118e-3): the largest relative error of the one-step fast inverse square root over
    the r^2 of far_cloud(), against 1 / sqrt in longdouble

(The walls' and the sphere Hertz deviations are those of the overlap, a difference of O(1) numbers, over overlaps down
to 0.02 and 0.005.)"""
import math

import mpmath as mp
import numpy as np
import pytest

import gradient_cases as gc
import potentials as P

EPS = gc.EPS


# ---- the two forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gc.NAMES)
def test_mpmath_and_longdouble_forms_agree(name):
    """every term's energy on the inputs of the device tests, to 1e-15 relative (of the larger of |U| and, for WCA, of
    its two powers, which cancel at d = sigma)"""
    case = gc.cases()[name]
    ld = gc.ld_energies(case)
    with P.hp():
        exact = gc.mp_energies(case)
        assert len(exact) == len(ld) > 0
        worst = 0.0
        for u, v in zip(exact, ld):
            scale = abs(u)
            if name.startswith("segments_wca") and u != 0:
                scale = max(scale, mp.mpf(1))   # 4 eps (sigma / d)^12 is O(1) on d in 0.8 .. 1.12
            if u == 0:
                assert v == 0
                continue
            worst = max(worst, float(abs(mp.mpf(float(v)) + mp.mpf(float(v - np.longdouble(float(v)))) - u) / scale))
    print("%s: worst relative difference %.3g" % (name, worst))
    assert worst <= 1e-15
    assert any(u != 0 for u in exact)


def test_inputs_meet_their_conditions():
    for case in gc.cases().values():
        case.check()


# ---- geometry -------------------------------------------------------------------------------------------------------------------
def _seg_both(a0, a1, b0, b1):
    with P.hp():
        d, s, t = P.segment_segment(P.vec(a0), P.vec(a1), P.vec(b0), P.vec(b1))
        d, s, t = float(d), float(s), float(t)
    dl, sl, tl = P.ld_segment_segment(np.array([a0]), np.array([a1]), np.array([b0]), np.array([b1]), True)
    assert abs(float(dl[0]) - d) <= 1e-15 * max(d, 1.0) and abs(float(sl[0]) - s) <= 1e-15 and abs(float(tl[0]) - t) <= 1e-15
    return d, s, t


def test_segment_distance_by_hand():
    # crossed perpendicular segments, 0.7 apart: both closest points interior
    d, s, t = _seg_both([-1.0, 0, 0], [1.0, 0, 0], [0.5, -1.0, 0.7], [0.5, 3.0, 0.7])
    assert abs(d - 0.7) <= 1e-15 and abs(s - 0.75) <= 1e-15 and abs(t - 0.25) <= 1e-15
    # end to end on one line, a gap of 0.5
    d, s, t = _seg_both([0.0, 0, 0], [1.0, 0, 0], [1.5, 0, 0], [3.0, 0, 0])
    assert abs(d - 0.5) <= 1e-15 and (s, t) == (1.0, 0.0)
    # an end against an interior: the foot of the perpendicular
    d, s, t = _seg_both([0.0, 0, 0], [2.0, 0, 0], [0.5, 0.3, 0.4], [0.5, 2.0, 3.0])
    assert abs(d - 0.5) <= 1e-15 and abs(s - 0.25) <= 1e-15 and t == 0.0
    # two ends, neither on a foot: a 3-4-5 triangle
    d, s, t = _seg_both([0.0, 0, 0], [1.0, 0, 0], [4.0, 4.0, 0], [6.0, 5.0, 0])
    assert abs(d - 5.0) <= 1e-15 and (s, t) == (1.0, 0.0)


def _sd_both(y, e):
    with P.hp():
        d = float(P.point_ellipsoid(P.vec(y), P.vec(e)))
    dl = float(P.ld_point_ellipsoid(np.array([y]), np.array(e))[0])
    assert abs(dl - d) <= 1e-15 * max(abs(d), 1.0), (y, e, d, dl)
    return d


def test_point_ellipsoid_distance_by_hand():
    e = (3.0, 2.0, 1.0)
    # a point on each axis, outside and (near the wall) inside: the closest point is the axis' own pole
    for axis, pole in enumerate(e):
        for offset in (0.5, -0.125):
            y = [0.0, 0.0, 0.0]
            y[axis] = pole + offset
            assert abs(_sd_both(y, e) - offset) <= 1e-15, (axis, offset)
            y[axis] = -y[axis]
            assert abs(_sd_both(y, e) - offset) <= 1e-15
    # deep inside on the long axis the closest point leaves the axis: at (2, 0, 0) it is (2.25, 0, +-sqrt(7)/4), at
    # distance sqrt(1/16 + 7/16)
    assert abs(_sd_both([2.0, 0.0, 0.0], e) + math.sqrt(0.5)) <= 1e-15
    # the centre: the shortest semi-axis
    assert abs(_sd_both([0.0, 0.0, 0.0], e) + 1.0) <= 1e-15
    # in the plane z = 0, outside: the ellipse (3, 2) and its normal at (3 cos, 2 sin): offset 0.25 along the normal
    c, s = math.cos(0.7), math.sin(0.7)
    n = np.array([c / 3.0, s / 2.0]) / math.hypot(c / 3.0, s / 2.0)
    assert abs(_sd_both([3.0 * c + 0.25 * n[0], 2.0 * s + 0.25 * n[1], 0.0], e) - 0.25) <= 4e-15
    # a sphere passed as an ellipsoid: |y| - R, general points and points with zero coordinates
    for y in ([0.3, -0.4, 1.2], [0.0, 0.6, 0.0], [0.1, 0.0, -0.2], [2.0, -1.0, 0.5], [0.0, 0.0, 0.0]):
        want = math.sqrt(sum(v * v for v in y)) - 1.5
        assert abs(_sd_both(y, (1.5, 1.5, 1.5)) - want) <= 2e-15
    # a general point of (3, 2, 1): the closest point x satisfies y - x = d n(x) with n the unit normal at x
    x = np.array([3.0 * 0.5, 2.0 * 0.5, 1.0 * math.sqrt(0.5)])
    n = x / np.array(e) ** 2
    n /= np.linalg.norm(n)
    for d in (0.2, -0.15):
        assert abs(_sd_both(list(x + d * n), e) - d) <= 4e-15


# ---- calibration ----------------------------------------------------------------------------------------------------------------
def _pow2_at_least(v):
    return 2.0 ** math.ceil(math.log2(v))


def test_calibration():
    worst = {}
    for name in gc.NAMES:
        case = gc.cases()[name]
        F, S = gc.exact(name)
        dev = gc.deviation(case.model(), F, S)
        x2, f2, QF, S2 = gc.moved_exact(name)   # the rotated and translated frame of the equivariance test
        dev2 = gc.deviation(gc.at(case, x2, f2).model(), QF, S2)
        assert np.isfinite(dev).all() and np.isfinite(dev2).all(), name
        worst[case.group] = max(worst.get(case.group, 0.0), float(dev.max()), float(dev2.max()))
        print("%-34s worst deviation of the model %8.3g eps S_b, rotated %8.3g" % (name, dev.max(), dev2.max()))
    worst["rpyc"] = _rpyc_model_deviation()
    print("\n    %-26s %-28s %s   (4 x worst, rounded up)" % ("term", "worst deviation [eps S_b]", "K"))
    for group, k in gc.TOLERANCE_K.items():
        print("    %-26s %-28.3g %-5g %g" % (group, worst[group], k, _pow2_at_least(4.0 * worst[group])))
    assert set(worst) == set(gc.TOLERANCE_K)
    for group, k in gc.TOLERANCE_K.items():
        assert worst[group] <= k / 4.0, (group, worst[group], k)
        assert k == 2.0 ** round(math.log2(k))


def _rpyc_model_deviation():
    """hydro_model.pair_terms on unit forces against rpyc_tt: the worst max |block - exact| / (eps |exact|_F) over the
    off-diagonal blocks of the cloud"""
    import hydro_model as hm
    c, a, _ = gc.mobility_cloud()
    M64, _ = gc.rpyc_blocks()
    n = len(a)
    worst = 0.0
    cols = [hm.pair_terms("rpyc", gc.VISCOSITY, c[:, None, :], a[:, None], c[None], a[None],
                          np.broadcast_to(np.eye(3)[j], (1, n, 3))) for j in range(3)]   # [t, s, i] per column j
    for t in range(n):
        for s in range(n):
            if s != t:
                blk = np.stack([cols[j][t, s] for j in range(3)], axis=1)
                ref = M64[3 * t:3 * t + 3, 3 * s:3 * s + 3]
                worst = max(worst, np.abs(blk - ref).max() / (EPS * np.linalg.norm(ref)))
    return float(worst)


def fast_rsqrt_delta():
    """the largest relative error of the one-step fast inverse square root over the r^2 of far_cloud(): a dense
    logarithmic sample of the range and the values themselves, against 1 / sqrt in longdouble"""
    import hydro_model as hm
    c, _ = gc.far_cloud()
    d = c[:, None] - c[None]
    r2 = (d * d).sum(axis=2)[~np.eye(len(c), dtype=bool)]
    x = np.concatenate([r2, np.exp(np.linspace(np.log(r2.min()), np.log(r2.max()), 400001))])
    exact = 1.0 / np.sqrt(x.astype(np.longdouble))
    return float(np.max(np.abs(hm.quake_inv_sqrt(x).astype(np.longdouble) - exact) / exact))


def test_fast_inverse_square_root_delta():
    delta = fast_rsqrt_delta()
    print("delta = %.6g" % delta)
    assert delta <= gc.FAST_RSQRT_DELTA and delta >= 0.5 * gc.FAST_RSQRT_DELTA


# ---- the mobility's own properties, in mpmath -------------------------------------------------------------------------------------
def test_rpyc_is_symmetric_positive_definite_and_continuous():
    M64, Mmp = gc.rpyc_blocks()
    _, _, branch = gc.mobility_cloud()
    assert (branch == "f").sum() >= 20 and (branch == "o").sum() >= 20 and (branch == "n").sum() >= 20
    with P.hp():
        n = len(Mmp)
        assert all(Mmp[i][j] == Mmp[j][i] for i in range(n) for j in range(i)) or \
            max(abs(Mmp[i][j] - Mmp[j][i]) for i in range(n) for j in range(i)) < mp.mpf(10) ** -45
    w = np.linalg.eigvalsh(M64)
    print("smallest eigenvalue %.6g" % w[0])
    assert w[0] > 1e-3
    np.linalg.cholesky(M64)
    # continuity across r = a + b (C^1) and r = |a - b| (C^0)
    with P.hp():
        u = [mp.mpf(2) / 7, mp.mpf(-3) / 7, mp.mpf(6) / 7]
        for a, b in ((1.0, 1.0), (0.5, 0.9), (1.2, 0.3), (0.7, 0.2), (0.4, 1.1)):
            for r0 in (a + b, abs(a - b)):
                if r0 == 0.0:
                    continue
                h = mp.mpf(10) ** -20
                lo = P.rpyc_tt([v * r0 * (1 - h) for v in u], a, b, 0.9)
                hi = P.rpyc_tt([v * r0 * (1 + h) for v in u], a, b, 0.9)
                assert mp.norm(hi - lo) <= mp.mpf(10) ** -18 * mp.norm(lo), (a, b, r0)
