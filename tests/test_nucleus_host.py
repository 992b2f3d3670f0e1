"""CPU-side checks of the nucleus terms of the chain step: known answers of the numpy model (periphery_model.py), its
exact distance against the reference routine, the telegraph process of the active springs, and the refusals of the
stepper, of ops and of the library (before any HIP call); the new entry points exported and bound."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import periphery_model as pm

RADII = (3.0, 2.0, 1.5)


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


# ---- 1. known answers of the periphery model ---------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_sphere_bead_beyond_contact_along_an_axis(axis, sign):
    R, r, K, delta = 5.0, 0.25, 7.0, 2.0 ** -6   # (every figure a dyadic rational: the answer is exact)
    c = np.zeros((1, 3))
    c[0, axis] = sign * (R - r + delta)
    f, col, mx = pm.sphere_force(c, np.array([r]), R, K)
    want = np.zeros(3)
    want[axis] = -sign * K * delta
    assert col == 1 and mx == delta and (f[0] == want).all()
    # added into an existing force, and untouched for a bead without contact
    base = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    f2, col2, _ = pm.sphere_force(np.vstack([c, np.zeros((1, 3))]), np.array([r, r]), R, K, force=base)
    assert col2 == 1 and (f2[0] == base[0] + want).all() and (f2[1] == base[1]).all()


def test_sphere_touching_and_centre_beads_get_no_force():
    R, r = 5.0, 0.25
    c = np.array([[R - r, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, -(R - r), 0.0]])
    f, col, mx = pm.sphere_force(c, np.full(3, r), R, 3.0)
    assert col == 0 and mx == 0.0 and not f.any() and not np.signbit(f).any()


def test_sphere_shifted_centre_is_the_same_answer():
    rng = np.random.default_rng(0)
    c = rng.normal(size=(500, 3)) * 3.0
    r = rng.uniform(0.1, 0.3, 500)
    f0, col0, mx0 = pm.sphere_force(c, r, 5.0, 2.0)
    # (c + shift) - shift is not c: each sum rounds at magnitudes below 32, so a coordinate moves by at most
    # 2 ulp(32) / 2 = 7.2e-15 and a bead by 1.3e-14.  ssd moves by as much; the force, K = 2, by K (1 + |ssd| / |x|)
    # times that, and |ssd| < |x|: below 5.2e-14.  The bound for all three is 1e-13.
    shift = np.array([8.0, -16.0, 4.0])
    f1, col1, mx1 = pm.sphere_force(c + shift, r, 5.0, 2.0, pcenter=shift)
    ssd = 5.0 - np.linalg.norm(c, axis=1) - r
    assert np.abs(c + shift).max() < 32.0 and np.abs(ssd).min() > 1e-12   # no bead that 1.3e-14 could carry across
    assert col0 > 50 and col1 == col0 and abs(mx1 - mx0) < 1e-13
    assert np.abs(f0 - f1).max() < 1e-13


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_ellipsoid_bead_beyond_contact_along_a_principal_axis(axis):
    r, K, delta = 0.25, 7.0, 2.0 ** -6
    for sign in (1.0, -1.0):
        c = np.zeros((1, 3))
        c[0, axis] = sign * (RADII[axis] - r + delta)
        f, col, mx = pm.ellipsoid_force(c, np.array([r]), RADII, K)
        want = np.zeros(3)
        want[axis] = -sign * K * delta
        assert col == 1 and abs(mx - delta) < 1e-15 and np.abs(f[0] - want).max() < 1e-14
    # touching, and at the centre (filtered: the medial set is never evaluated)
    c = np.zeros((2, 3))
    c[0, axis] = RADII[axis] - r - 1e-12
    f, col, mx = pm.ellipsoid_force(c, np.full(2, r), RADII, K)
    assert col == 0 and mx == 0.0 and not f.any()
    assert pm.ellipsoid_filter(c, np.full(2, r), RADII, (0, 0, 0), (1, 0, 0, 0)).tolist() == [False, True]


def test_ellipsoid_with_equal_radii_is_the_sphere():
    rng = np.random.default_rng(1)
    R, K = 4.0, 3.0
    c = pm.surface_points(rng, 2000, (R, R, R), 0.75, 1.1)
    r = rng.uniform(0.05, 0.3, 2000)
    q = _unit([0.7, -0.2, 0.5, 0.4])
    pc = np.array([0.5, -1.0, 2.0])
    fs, cols, mxs = pm.sphere_force(c + pc, r, R, K, pcenter=pc)
    fe, cole, mxe = pm.ellipsoid_force(c + pc, r, (R, R, R), K, pcenter=pc, quat=q)
    assert cols > 500
    err = np.abs(fs - fe).max()
    print("sphere vs equal-radii ellipsoid: max |dF| = %.3g, colliding %d / %d" % (err, cols, cole))
    assert err < 1e-13 and abs(mxs - mxe) < 1e-13


def test_filter_passes_only_beads_whose_box_is_inside():
    rng = np.random.default_rng(2)
    q, pc = _unit([0.9, 0.1, -0.3, 0.2]), np.array([0.3, -0.2, 0.5])
    y = pm.surface_points(rng, 3000, RADII, 0.0, 1.1)
    c = pm.quat_rotate(q, y) + pc
    r = rng.uniform(0.05, 0.2, 3000)
    inside = pm.ellipsoid_filter(c, r, RADII, pc, q)
    sd, _ = pm.exact_distance(c, pc, q, RADII)
    # a filtered bead cannot touch the wall: its box, which holds the bead, is inside the (convex) ellipsoid
    assert inside.sum() > 500 and (-sd[inside] - r[inside] > 0).all()
    # with and without the filter the force is the same
    f0 = pm.ellipsoid_force(c, r, RADII, 2.0, pc, q)
    f1 = pm.ellipsoid_force(c, r, RADII, 2.0, pc, q, use_filter=False)
    assert (f0[0] == f1[0]).all() and f0[1:] == f1[1:]


def test_fast_ellipsoid_known_answers():
    r, K = 0.25, 3.0
    c = np.array([[RADII[0] - r + 0.125, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, RADII[1] - r, 0.0], [0.0, 0.0, -1.5]])
    f, col, mx = pm.ellipsoid_fast_force(c, np.full(4, r), RADII, K)
    a = RADII[0] - r
    assert col == 2 and (f[1] == 0).all() and (f[2] == 0).all()     # centre and touching (g = 0): no force
    assert f[0, 0] == -(K * (2.0 * c[0, 0] * (1.0 / (a * a)))) and f[0, 1] == 0 and f[0, 2] == 0
    assert f[3, 2] > 0 and mx == max((c[0, 0] / a) ** 2 - 1, (1.5 / 1.25) ** 2 - 1)


def test_exact_distance_agrees_with_the_reference_routine_at_its_own_margin(oracle):
    # distance(SharedNormalSigned, Point, Ellipsoid) (PointEllipsoid.hpp:94-135): nine-start L-BFGS good to 1e-4
    # (UnitTestEllipsoidEllipsoid.cpp:52-53).  The margin is that routine's own; no tighter bound is pinned.
    rng = np.random.default_rng(3)
    n = 500
    q, pc = _unit([0.9, 0.1, -0.3, 0.2]), np.array([0.3, -0.2, 0.5])
    c = pm.quat_rotate(q, pm.surface_points(rng, n, RADII, 0.75, 1.1)) + pc
    sd, pn = pm.exact_distance(c, pc, q, RADII)
    d, cp, nrm = oracle.distance_point_ellipsoid(c, np.tile(pc, (n, 1)), np.tile(q, (n, 1)), np.tile(RADII, (n, 1)))
    print("exact vs reference routine: max |d - sd| = %.3g, max |n + pn| = %.3g, inside %.0f %%"
          % (np.abs(d - sd).max(), np.abs(nrm + pn).max(), 100 * (sd < 0).mean()))
    assert not np.isnan(sd).any() and 0.5 < (sd < 0).mean() < 0.9
    assert np.abs(d - sd).max() <= 1e-4
    # the closest points lie on the surface, and c - closest is along the normal
    y = pm.quat_rotate(pm.conjugate(q), c - pc)
    x = np.array([pm.point_ellipsoid_body(p, RADII)[1] for p in y])
    assert np.abs(((x / np.asarray(RADII)) ** 2).sum(axis=1) - 1.0).max() < 1e-14


# ---- 2. the telegraph process -------------------------------------------------------------------------------------------
def test_uniform_is_the_open_53_bit_map_of_block_0():
    import chain_model as cm
    keys, ctr = np.array([0, 5, 2 ** 62], np.uint64), np.array([0, 7, 2 ** 40], np.uint64)
    w = cm.philox(keys, ctr, 0).astype(np.uint64)
    u = pm.uniform_open(keys, ctr)
    m = (w[:, 0] * np.uint64(2 ** 21)) + (w[:, 1] >> np.uint64(11))
    assert (u == (m + np.uint64(1)).astype(np.float64) / 2.0 ** 53).all()
    assert ((u > 0) & (u <= 1)).all() and np.isfinite(np.log(u)).all()


def test_dwell_count_is_ceil_of_time_over_dt():
    m, dt = 4000, 2.0 ** -4   # (a dyadic dt: the timers are exact sums)
    keys = np.arange(m, dtype=np.uint64)
    s = pm.active_init(keys, np.zeros(m, np.uint64), kon=1.5)
    assert (s["state"] == 0).all() and (s["elapsed"] == 0).all() and (s["counters"] == 1).all()
    t_on = s["next_time"].copy()
    switched_at = np.full(m, -1)
    for rnd in range(200):
        s, (on, off) = pm.active_sample(s, keys, 1.5, 4.0)
        first = (switched_at < 0) & (s["state"] == 1)
        switched_at[first] = rnd
        assert off == 0 or rnd > 0
        s = pm.active_advance(s, dt)
    done = switched_at >= 0
    assert done.mean() > 0.99
    # a spring drawn T waits ceil(T / dt) rounds: it is sampled at the start of each round, and elapsed = rounds dt
    assert (switched_at[done] == np.ceil(t_on[done] / dt)).all()
    # a spring that does not switch draws nothing: its counter counts its switches only
    assert (s["counters"] >= 2)[done].all() and (s["counters"][~done] == 1).all()


def test_active_force_is_a_dipole_of_magnitude_sigma():
    rng = np.random.default_rng(4)
    n = 200
    center = rng.normal(size=(n, 3))
    pairs = np.stack([np.arange(0, n, 2), np.arange(1, n, 2)], axis=1)   # a matching
    state = (np.arange(n // 2) % 3 == 0).astype(np.int32)
    f, act = pm.active_force(n, pairs, state, 2.5, center)
    assert act == state.sum()
    on = pairs[state == 1]
    assert (f[on[:, 0]] == -f[on[:, 1]]).all() and np.abs(np.linalg.norm(f[on[:, 0]], axis=1) - 2.5).max() < 1e-14
    off = pairs[state == 0]
    assert not f[off].any() and not np.signbit(f[off]).any()
    # body i is pushed away from body j
    assert (((center[on[:, 1]] - center[on[:, 0]]) * f[on[:, 0]]).sum(axis=1) < 0).all()
    base = rng.normal(size=(n, 3))
    f2, _ = pm.active_force(n, pairs, state, 2.5, center, force=base)
    assert (f2[off.ravel()] == base[off.ravel()]).all() and (f2[on[:, 0]] == base[on[:, 0]] + f[on[:, 0]]).all()


# ---- 3. refusals before any device work ---------------------------------------------------------------------------------
def test_step_stats_gain_the_nucleus_counts_with_default_zero():
    from mundy_amd import pipeline
    s = pipeline.StepStats()
    assert (s.periphery_colliding, s.max_periphery_overlap, s.active_springs, s.active_switches) == (0, 0.0, 0, (0, 0))


def _per(**kw):
    d = dict(shape="ellipsoid", radii=(3.0, 2.0, 1.5), k=10.0)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not ...}


def _act(**kw):
    d = dict(springs=[0, 2], sigma=1.0, kon=2.0, koff=3.0)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not ...}


SPRINGS = (np.array([[0, 1], [1, 2], [2, 3]]), "hookean", 10.0, 1.0)


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.full((n,), 0.5, dtype=torch.float64)
    kind = kw.pop("kind", "sphere")
    extra = {}
    if kind != "sphere":
        extra = dict(quat=torch.zeros((n, 4), dtype=torch.float64), length=torch.ones(n, dtype=torch.float64))
    if kind == "mixed":
        extra = dict(quat=extra["quat"], kinds=torch.zeros(n, dtype=torch.int32),
                     shape=torch.ones((n, 3), dtype=torch.float64))
    return pipeline.ContactStepper(kind, c, r, **extra, **kw)


@pytest.mark.parametrize("kw,match", [
    (dict(kind="spherocylinder", periphery=_per()), "spheres only"),
    (dict(kind="mixed", periphery=_per()), "spheres only"),
    (dict(kind="spherocylinder", active_forces=_act(), springs=SPRINGS), "spheres only"),
    (dict(periphery=_per(), growth_rate=0.1, division_length=2.0), "growth"),
    (dict(periphery=_per(), contact_model="hertz", hertz_friction=0.3), "hertz_friction"),
    (dict(periphery=_per(), friction=0.3), "friction"),
    (dict(periphery=_per(), contact_cutoff=0.1), "contact_cutoff"),
    (dict(periphery=_per(), periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(active_forces=_act(), springs=SPRINGS, periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(periphery=[1, 2]), "dict"),
    (dict(periphery=_per(colour=1)), "unknown key"),
    (dict(periphery=_per(k=...)), "missing key"),
    (dict(periphery=_per(shape=...)), "missing key"),
    (dict(periphery=_per(radii=...)), "missing key"),
    (dict(periphery=_per(shape="sphere")), "missing key"),
    (dict(periphery=_per(radius=3.0)), "takes radii"),
    (dict(periphery=_per(shape="sphere", radius=3.0)), "takes radius"),
    (dict(periphery=_per(shape="cube")), "shape must be"),
    (dict(periphery=_per(radii=(3.0, 2.0))), "3 numbers"),
    (dict(periphery=_per(radii=(3.0, 0.0, 1.5))), "> 0"),
    (dict(periphery=_per(radii=(3.0, -2.0, 1.5))), "> 0"),
    (dict(periphery=_per(radii=(3.0, math.inf, 1.5))), "finite"),
    (dict(periphery=_per(shape="sphere", radii=..., radius=math.nan)), "finite"),
    (dict(periphery=_per(shape="sphere", radii=..., radius=0.0)), "> 0"),
    (dict(periphery=_per(k=-1.0)), ">= 0"),
    (dict(periphery=_per(k=math.nan)), "finite"),
    (dict(periphery=_per(center=(0.0, math.inf, 0.0))), "finite"),
    (dict(periphery=_per(center=(0.0, 0.0))), "3 numbers"),
    (dict(periphery=_per(quat=(1.0, 0.0, 0.0))), "4 numbers"),
    (dict(periphery=_per(quat=(1.0, 1e-5, 0.0, 0.0))), "unit quaternion"),
    (dict(periphery=_per(quat=(0.0, 0.0, 0.0, 0.0))), "unit quaternion"),
    (dict(periphery=_per(quat=(math.nan, 0.0, 0.0, 0.0))), "finite"),
    (dict(periphery=_per(shape="ellipsoid_fast", quat=(0.0, 1.0, 0.0, 0.0))), "no orientation"),
    (dict(periphery=_per(radii=(3.0, 2.0, 0.5))), "bead radius"),
    (dict(periphery=_per(shape="sphere", radii=..., radius=0.4)), "bead radius"),
    (dict(active_forces=_act()), "needs springs"),
    (dict(active_forces=[0, 1], springs=SPRINGS), "dict"),
    (dict(active_forces=_act(colour=1), springs=SPRINGS), "unknown key"),
    (dict(active_forces=_act(sigma=...), springs=SPRINGS), "missing key"),
    (dict(active_forces=_act(springs=...), springs=SPRINGS), "missing key"),
    (dict(active_forces=_act(springs=[0, 3]), springs=SPRINGS), "outside"),
    (dict(active_forces=_act(springs=[-1]), springs=SPRINGS), "outside"),
    (dict(active_forces=_act(springs=[1, 1]), springs=SPRINGS), "more than once"),
    (dict(active_forces=_act(springs=[0.0, 1.0]), springs=SPRINGS), "integers"),
    (dict(active_forces=_act(springs=[[0, 1]]), springs=SPRINGS), "integers of shape"),
    (dict(active_forces=_act(sigma=math.nan), springs=SPRINGS), "sigma"),
    (dict(active_forces=_act(kon=0.0), springs=SPRINGS), "kon"),
    (dict(active_forces=_act(kon=math.inf), springs=SPRINGS), "kon"),
    (dict(active_forces=_act(koff=-1.0), springs=SPRINGS), "koff"),
    (dict(active_forces=_act(koff=math.nan), springs=SPRINGS), "koff"),
    (dict(active_forces=_act(keys=[0, -1]), springs=SPRINGS), r"2\^63"),
    (dict(active_forces=_act(keys=[0, 1, 2]), springs=SPRINGS), "keys"),
    (dict(active_forces=_act(counter=[0.5, 1.0]), springs=SPRINGS), "counter")])
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_ops_checks_mirror_the_library_without_loading_it(monkeypatch):
    from mundy_amd import capi, ops

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    c, r = torch.zeros((2, 3), dtype=torch.float64), torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="unit quaternion"):
        ops.periphery_force(_per(quat=(2.0, 0.0, 0.0, 0.0)), c, r)
    with pytest.raises(ValueError, match="itself"):
        ops.ActiveSprings(3, [[0, 1], [2, 2]], 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="outside"):
        ops.ActiveSprings(3, [[0, 3]], 1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="kon"):
        ops.ActiveSprings(3, [[0, 1]], 1.0, -1.0, 1.0)
    assert ops.check_periphery(_per(shape="sphere", radii=..., radius=2.0))[1] == [2.0, 2.0, 2.0]


# ---- 4. the library's own refusals (before any HIP call) ---------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    names = ["mhip_periphery_force"] + ["mhip_active_springs_" + s for s in
                                        ("create", "sample", "force", "advance", "get_state", "set_state", "renumber",
                                         "destroy")]
    for name in names:
        assert hasattr(lib, name) and name in capi.SIGNATURES


def _periphery(shape=1, center=(0.0, 0.0, 0.0), quat=(1.0, 0.0, 0.0, 0.0), radii=(3.0, 2.0, 1.5), k=1.0):
    from mundy_amd import capi
    return capi.Periphery(shape, (C.c_double * 3)(*center), (C.c_double * 4)(*quat), (C.c_double * 3)(*radii), k)


@pytest.mark.parametrize("kw,match", [
    (dict(shape=3), "unknown periphery shape"), (dict(shape=-1), "unknown periphery shape"),
    (dict(radii=(3.0, 0.0, 1.5)), "radii"), (dict(radii=(3.0, 2.0, -1.5)), "radii"),
    (dict(radii=(math.nan, 2.0, 1.5)), "radii"), (dict(shape=0, radii=(0.0, 2.0, 1.5)), "radii"),
    (dict(shape=2, radii=(3.0, math.inf, 1.5)), "radii"), (dict(k=-1.0), "constant k"), (dict(k=math.nan), "constant k"),
    (dict(k=math.inf), "constant k"), (dict(center=(0.0, math.nan, 0.0)), "center"),
    (dict(quat=(1.0, 1e-5, 0.0, 0.0)), "unit quaternion"), (dict(quat=(0.0, 0.0, 0.0, 0.0)), "unit quaternion"),
    (dict(quat=(math.inf, 0.0, 0.0, 0.0)), "quat"), (dict(shape=2, quat=(0.0, 0.0, 1.0, 0.0)), "no orientation")])
def test_periphery_force_refuses_bad_arguments_before_any_hip_call(lib, kw, match):
    from mundy_amd import capi
    cfg = _periphery(**kw)
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_periphery_force(C.byref(cfg), 0, None, None, None, 0, None, None, None))


def test_periphery_force_accepts_what_it_should_and_refuses_null(lib):
    from mundy_amd import capi
    # a sphere reads radii[0] only; n = 0 without statistics makes no HIP call
    capi.check(lib.mhip_periphery_force(C.byref(_periphery(shape=0, radii=(3.0, -1.0, math.nan))), 0, None, None, None, 0,
                                        None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_periphery_force(None, 0, None, None, None, 0, None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_periphery_force(C.byref(_periphery()), 4, None, None, None, 0, None, None, None))


def _create(lib, n=4, pairs=((0, 1), (2, 3)), sigma=1.0, kon=2.0, koff=3.0, keys=None, counters=None):
    p = np.ascontiguousarray(pairs, dtype=np.int32)
    ks = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    cs = None if counters is None else np.ascontiguousarray(counters, dtype=np.uint64)
    cp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p(12345)
    st = lib.mhip_active_springs_create(C.byref(h), n, p.shape[0], cp(p), sigma, kon, koff, cp(ks), cp(cs), None)
    return st, h


@pytest.mark.parametrize("kw,match", [
    (dict(pairs=((0, 4),)), "outside"), (dict(pairs=((-1, 2),)), "outside"), (dict(pairs=((0, 1), (2, 2))), "itself"),
    (dict(sigma=math.nan), "sigma"), (dict(sigma=math.inf), "sigma"), (dict(kon=0.0), "kon"), (dict(kon=-1.0), "kon"),
    (dict(kon=math.nan), "kon"), (dict(koff=0.0), "koff"), (dict(koff=math.inf), "koff"),
    (dict(keys=(0, 2 ** 63)), "key outside"), (dict(counters=(2 ** 63, 0)), "counter outside")])
def test_active_create_refuses_bad_arguments_before_any_hip_call(lib, kw, match):
    from mundy_amd import capi
    st, h = _create(lib, **kw)
    with pytest.raises(ValueError, match=match):
        capi.check(st)
    assert h.value is None  # nothing was created


def test_active_null_handles_and_bad_dt_are_refused(lib):
    from mundy_amd import capi
    P = lambda v: C.c_void_p(16 * v)  # noqa: E731  (fake device pointers, never dereferenced)
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_create(None, 4, 0, None, 1.0, 1.0, 1.0, None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_sample(None, P(1), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_force(None, P(1), P(2), 0, P(3), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_advance(None, 1e-3, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_get_state(None, P(1), None, None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_set_state(None, P(1), None, None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_active_springs_renumber(None, P(1), None))
    capi.check(lib.mhip_active_springs_destroy(None))


def test_nucleus_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("nucleus_step_app")
    assert os.path.exists(exe)
