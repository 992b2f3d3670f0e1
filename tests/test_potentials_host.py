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
    filament force                  13.9                   64
    filament force, wave            30.9                  128
    filament torque                 26.6                  128
    filament Hertz                   2.63                  16

    delta = 1.752e-3 (measured 1.75118e-3): the largest relative error of the one-step fast inverse square root over
    the r^2 of far_cloud(), against 1 / sqrt in longdouble

(The walls' and the sphere Hertz deviations are those of the overlap, a difference of O(1) numbers, over overlaps down
to 0.02 and 0.005.)

The filament rows are tests/filament_cases.py's: filament_model.py against the gradient of the discrete rod energy, plus
the stray term R where the binormal acts (the "moved" states), over every state in its own frame and run from a rotated
and translated layout; the torque row in units of eps S_tau.  The wave has a row of its own: its phase k s + omega t +
phi is rounded at |phase| up to 190 on the 259-node filament, which costs A eps |phase|.  filament Hertz is
filament_contact_model.py without friction against the pair Hertz energy."""
import math

import mpmath as mp
import numpy as np
import pytest

import filament_cases as fc
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
    for name in fc.NAMES:
        fc.state(name).check()
        fc.moved_exact(name)[1].check()
    fc.contact_case().check()


def _ld_minus_mp(v, u):
    """the longdouble v less the mpf u, exactly"""
    return mp.mpf(float(v)) + mp.mpf(float(v - np.longdouble(float(v)))) - u


@pytest.mark.parametrize("name", fc.NAMES)
def test_filament_forms_agree(name):
    """every element's and every edge's energy on the inputs of the device tests, to 1e-15 of itself"""
    st = fc.state(name)
    el, ed = fc.ld_energies(st)
    worst, count = 0.0, 0
    with P.hp():
        mel, med = fc.mp_energies(st, st.nodes)
        for b, u_el, u_ed in zip(st.nodes, mel, med):
            for u, v in ((u_el, el[b]), (u_ed, ed[b])):
                if u is None:
                    assert v == 0
                    continue
                assert u > 0
                worst, count = max(worst, float(abs(_ld_minus_mp(v, u)) / u)), count + 1
    print("%s: worst relative difference %.3g over %d terms" % (name, worst, count))
    assert worst <= 1e-15 and count >= 20


def test_filament_contact_forms_agree():
    case = fc.contact_case()
    ld = case.ld_energies()
    with P.hp():
        X = [P.vec(p) for p in case.x]
        exact = [t.energy([X[b] for b in t.bodies]) for t in case.terms()]
        worst = 0.0
        for u, v in zip(exact, ld):
            if u == 0:
                assert v == 0
            else:
                worst = max(worst, float(abs(_ld_minus_mp(v, u)) / u))
    print("worst relative difference %.3g" % worst)
    assert worst <= 1e-15 and sum(u != 0 for u in exact) >= 16 and sum(u == 0 for u in exact) >= 8


# ---- the discrete rod by hand -----------------------------------------------------------------------------------------------
def _frames_both(T, x, theta, D):
    """the frames of the edges of the polyline x from old tangents T, twists and old frames, in both forms -> ([edges, 4]
    float64 from mpmath, [edges, 4] longdouble)"""
    x = np.asarray(x, dtype=np.float64)
    with P.hp():
        q = [P.edge_frame(P.vec(T[e]), P.unit_tangent(P.vec(x[e]), P.vec(x[e + 1])), gc.M(theta[e]),
                          [gc.M(v) for v in D[e]]) for e in range(len(x) - 1)]
        q = np.array([[float(v) for v in row] for row in q])
    ql = P.ld_edge_frame(np.asarray(T), P.ld_unit_tangent(x[:-1], x[1:]), np.asarray(theta), np.asarray(D))
    assert np.abs(np.asarray(ql, dtype=np.float64) - q).max() <= 2e-16
    return q, ql


def _curvature_both(q, ql):
    with P.hp():
        k = np.array([[float(v) for v in P.curvature([gc.M(v) for v in q[i]], [gc.M(v) for v in q[i + 1]])]
                      for i in range(len(q) - 1)])
    kl = np.asarray(P.ld_curvature(ql[:-1], ql[1:]), dtype=np.float64)
    assert np.abs(kl - k).max() <= 4e-16
    return k


IDENTITY4 = (1.0, 0.0, 0.0, 0.0)


def test_rod_by_hand():
    z = (0.0, 0.0, 1.0)
    n = 6
    straight = np.stack([np.zeros(n), np.zeros(n), np.arange(n) * 1.0], axis=1)
    # a straight rod at rest, dyadic inputs: every frame the identity, E = 0 exactly, in both forms
    q, ql = _frames_both([z] * (n - 1), straight, [0.0] * (n - 1), [IDENTITY4] * (n - 1))
    assert (q == np.array(IDENTITY4)).all() and (ql == np.array(IDENTITY4, dtype=P.LD)).all()
    ptr = np.array([0, n])
    qn = np.concatenate([ql, [IDENTITY4]])
    bend, stretch = P.ld_rod_energy(ptr, straight, qn, np.full(n, 0.75), np.zeros((n, 3)), 10.0, 0.3, 1.0)
    assert (bend == 0).all() and (stretch == 0).all()
    with P.hp():
        X = [P.vec(p) for p in straight]
        for i in range(1, n - 1):
            assert P.rod_element(X[i - 1:i + 2], [mp.mpf(0)] * 2, [P.vec(z)] * 2, [P.vec(IDENTITY4)] * 2, [mp.mpf(0)] * 3,
                                 gc.M(0.75), gc.M(10.0), gc.M(0.3), gc.M(1.0)) == 0
            assert P.rod_edge(X[i:i + 2], gc.M(0.75), gc.M(10.0), gc.M(1.0)) == 0
    # a planar polygonal arc, turning angle phi per node, reached from the straight rod by transport alone: the curvature
    # is 2 sin(phi / 2) about the normal of the plane, here -x (z turns towards +y)
    phi = 0.3
    a = np.arange(n - 1) * phi
    arc = np.concatenate([np.zeros((1, 3)), np.cumsum(np.stack([np.zeros(n - 1), np.sin(a), np.cos(a)], axis=1) * 1.1, axis=0)])
    q, ql = _frames_both([z] * (n - 1), arc, [0.0] * (n - 1), [IDENTITY4] * (n - 1))
    k = _curvature_both(q, ql)
    assert np.abs(k[1:] - np.array([-2.0 * math.sin(phi / 2.0), 0.0, 0.0])).max() <= 1e-15
    assert np.abs(k[0] - np.array([-2.0 * math.sin(phi / 2.0), 0.0, 0.0])).max() <= 1e-15
    # its element energy by hand: (1 / (2 l0)) E (pi r^4 / 4) (2 sin(phi / 2) - rest_0)^2
    r, E, l0, rest0 = 0.75, 10.0, 0.8, -0.1
    want = 0.5 / l0 * E * (math.pi * r ** 4 / 4.0) * (-2.0 * math.sin(phi / 2.0) - rest0) ** 2
    qn = np.concatenate([ql, [IDENTITY4]])
    bend, _ = P.ld_rod_energy(ptr, arc, qn, np.full(n, r), np.tile([rest0, 0.0, 0.0], (n, 1)), E, 0.3, l0)
    assert np.abs(np.asarray(bend[1:-1], dtype=np.float64) - want).max() <= 1e-14 * want and bend[0] == 0 and bend[-1] == 0
    # a straight rod with the twist difference dtheta between neighbouring edges: kappa_3 = 2 sin(dtheta / 2)
    dth = 0.4
    q, ql = _frames_both([z] * (n - 1), straight, np.arange(n - 1) * dth, [IDENTITY4] * (n - 1))
    k = _curvature_both(q, ql)
    assert np.abs(k - np.array([0.0, 0.0, 2.0 * math.sin(dth / 2.0)])).max() <= 1e-15
    # ... stored with 2 G I = E I / (1 + nu): the twist energy by hand
    nu = 0.25
    want = 0.5 / l0 * (E / (1.0 + nu)) * (math.pi * r ** 4 / 4.0) * (2.0 * math.sin(dth / 2.0)) ** 2
    qn = np.concatenate([ql, [IDENTITY4]])
    bend, _ = P.ld_rod_energy(ptr, straight, qn, np.full(n, r), np.zeros((n, 3)), E, nu, l0)
    assert np.abs(np.asarray(bend[1:-1], dtype=np.float64) - want).max() <= 1e-14 * want
    # one edge stretched by 0.5 (the third), the right node's radius 0.5 among radii of 1: 1/2 (E pi r^2 / l0) 0.25
    long = straight.copy()
    long[3:, 2] += 0.5
    radius = np.ones(n)
    radius[3] = 0.5
    _, stretch = P.ld_rod_energy(ptr, long, np.tile(IDENTITY4, (n, 1)), radius, np.zeros((n, 3)), 8.0, 0.3, 1.0)
    want = 0.5 * 8.0 * math.pi * 0.25 * 0.25
    assert abs(float(stretch[2]) - want) <= 1e-15 * want and stretch[2] == stretch.sum()
    with P.hp():
        assert abs(P.rod_edge([P.vec(long[2]), P.vec(long[3])], gc.M(0.5), gc.M(8.0), gc.M(1.0)) - mp.pi / 4) <= mp.mpf(10) ** -45


def test_wave_rest_curvature_by_hand():
    rest = np.array([[0.05, -0.02, 0.07]])
    with P.hp():
        got = P.wave_rest_curvature(P.vec(rest[0]), gc.M(0.2), gc.M(0.5), gc.M(3.0), gc.M(2.0), gc.M(0.25), gc.M(-2.0))
        assert got[0] == 0 and got[1:] == P.vec(rest[0])[1:]   # A sin(1.5 + 0.5 - 2)
        got = P.wave_rest_curvature(P.vec(rest[0]), gc.M(0.2), gc.M(0.5), gc.M(3.0), gc.M(2.0), gc.M(0.25), gc.M(0.0))
        assert abs(got[0] - mp.mpf("0.2") * mp.sin(2)) <= mp.mpf(10) ** -16
    ld = P.ld_wave_rest_curvature(rest, 0.2, 0.5, 3.0, 2.0, 0.25, 0.0)
    assert abs(float(ld[0, 0]) - 0.2 * math.sin(2.0)) <= 1e-16 and (ld[0, 1:] == rest[0, 1:]).all()


def test_the_stray_term_is_the_whole_departure_from_the_gradient():
    """On the "moved" states filament_model.py is -grad E + R within K (test_calibration); without R it is not, by the
    size of R, which is at least 100 K eps S_F on some node: the device test cannot pass with R dropped."""
    K = gc.TOLERANCE_K["filament force"]
    for name in fc.NAMES:
        if fc.split(name)[0] != "moved":
            continue
        st, ex = fc.state(name), fc.exact_of(name)
        Fm, _ = st.model_rows()
        with_r = fc.deviation(Fm, ex["F"], ex["S_F"])
        without = fc.deviation(Fm, ex["F"] - ex["R"], ex["S_F"])
        size = np.abs(ex["R"]).max(axis=1) / (EPS * ex["S_F"])
        print("%s: max |R| = %.3g = %.3g eps S_F; model - exact: %.3g with R, %.3g without" % (
            name, np.abs(ex["R"]).max(), size.max(), with_r.max(), without.max()))
        assert with_r.max() <= K / 4.0 and size.max() >= 100.0 * K and without.max() >= 100.0 * K


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
    worst.update(_filament_model_deviation())
    print("\n    %-26s %-28s %s   (4 x worst, rounded up)" % ("term", "worst deviation [eps S_b]", "K"))
    for group, k in gc.TOLERANCE_K.items():
        print("    %-26s %-28.3g %-5g %g" % (group, worst[group], k, _pow2_at_least(4.0 * worst[group])))
    assert set(worst) == set(gc.TOLERANCE_K)
    for group, k in gc.TOLERANCE_K.items():
        assert worst[group] <= k / 4.0, (group, worst[group], k)
        assert k == 2.0 ** round(math.log2(k))


def _filament_model_deviation():
    """filament_model.py against -grad E (+ R) and -dE/dtheta, every state in its own frame and run from the rotated
    layout; filament_contact_model.py without friction against the pair Hertz energy"""
    worst = {"filament force": 0.0, "filament force, wave": 0.0, "filament torque": 0.0}
    for name in fc.NAMES:
        group = "filament force, wave" if fc.split(name)[0] == "wave" else "filament force"
        for tag, st, ex in (("", fc.state(name), fc.exact_of(name)), (", rotated",) + fc.moved_exact(name)[1:]):
            Fm, Tm = st.model_rows()
            dF, dT = fc.deviation(Fm, ex["F"], ex["S_F"]), fc.deviation(Tm, ex["tau"], ex["S_tau"])
            assert np.isfinite(dF).all() and np.isfinite(dT).all(), name
            print("%-34s worst deviation of the model: force %8.3g eps S_F, torque %8.3g eps S_tau" % (
                name + tag, dF.max(), dT.max()))
            worst[group] = max(worst[group], float(dF.max()))
            worst["filament torque"] = max(worst["filament torque"], float(dT.max()))
    case = fc.contact_case()
    F, S = fc.contact_exact()
    d = gc.deviation(case.model(), F, S)
    assert np.isfinite(d).all()
    print("%-34s worst deviation of the model %8.3g eps S_b" % ("filament contacts", d.max()))
    worst["filament Hertz"] = float(d.max())
    return worst


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
