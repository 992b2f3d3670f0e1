"""Semiflexible chains on the device (include/mundy_hip_bending.h): the angular springs and the FENE-WCA
bond bit for bit against tests/bending_model.py (the cosines of the rest angles are the handle's own), their statistics
wherever they sit, renumbering, both held to the gradients of their potentials at the K of tests/bending_cases.py, the
Python stepper against the composed models over 20 steps, a relaxation, and the C++ stepper against the Python one."""
import math
import subprocess

import numpy as np
import pytest

import bending_cases as bc
import bending_model as bm
import chain_model as chm
import gradient_cases as gc
import hp1_case as hp1
import hydro_model
from gpu_util import (PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host, renumberings,
                      star_and_random_graph)
from test_gpu_chain import _graph

pytestmark = pytest.mark.gpu


def _same_double(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


# ---- the angular springs, bit for bit ---------------------------------------------------------------------------------------------
def _star_and_random_triplets(rng):
    """gpu_util's star and random graph as triplets: body 0 is the centre of 100 triplets over consecutive spokes, every
    random edge (i, j) gets a third body as its centre; the 20 bodies behind the star stay on no triplet"""
    n, pairs = star_and_random_graph(rng)
    n0 = 121
    spokes = np.arange(1, 101)
    star = np.stack([spokes, np.roll(spokes, -1), np.zeros(100, np.int64)], axis=1)
    g = pairs[100:].astype(np.int64)
    c = rng.integers(n0, n, len(g))
    keep = (c != g[:, 0]) & (c != g[:, 1])
    return n, np.concatenate([star, np.column_stack([g[keep], c[keep]])]).astype(np.int32)


def _angular_case(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "one triplet":
        return 3, np.array([[0, 2, 1]], np.int32), rng.normal(size=(3, 3))
    if name == "star and random":
        n, t = _star_and_random_triplets(rng)
        return n, t, rng.uniform(0.0, 6.0, (n, 3))
    from mundy_amd import synth
    n = PAST_FULL_GRID   # one chain: the grid-stride loop's second pass
    steps = rng.normal(size=(n, 3))
    steps *= (rng.uniform(0.6, 1.3, n) / np.linalg.norm(steps, axis=1))[:, None]
    return n, synth.chain_triplets([0, n]), np.cumsum(steps, axis=0)


@pytest.mark.parametrize("per_triplet", [False, True])
@pytest.mark.parametrize("name", ["one triplet", "star and random", "long chain"])
def test_angular_forces_bit_for_bit(name, per_triplet):
    from mundy_amd import ops
    n, t, c = _angular_case(name)
    rng = np.random.default_rng(17)
    m = len(t)
    k = rng.uniform(0.5, 9.0, m) if per_triplet else 3.0
    a = rng.uniform(0.0, math.pi, m) if per_triplet else 2.5
    if per_triplet:
        a[::5], a[1::7] = math.pi, 0.0   # the ends of the range, where the cosine is exact
    h = ops.AngularSprings(n, t, k, a)
    cr = h.cos_rest
    assert cr.shape == (m,) and (h.triplets == t).all() and (h.k == k).all()
    assert np.abs(cr - np.cos(a)).max() <= 2e-16   # (the handle's std::cos; the model takes these, not numpy's)
    want, wdeg, wmx = bm.angular_force(n, t, k, cr, c)
    f, deg, mx = h.force(dev(c))
    assert_bits_equal(host(f), want, "%s, written" % name)
    assert int(deg.item()) == wdeg == 0 and _same_double(mx.item(), wmx) and wmx > 0
    old = rng.normal(size=(n, 3))
    old[::3] = -0.0   # accumulate leaves the rows of untouched bodies alone: a -0.0 stays
    want2, _, _ = bm.angular_force(n, t, k, cr, c, force=old)
    acc = dev(old)
    _, deg2, mx2 = h.force(dev(c), out=acc, accumulate=True)
    assert_bits_equal(host(acc), want2, "%s, accumulated" % name)
    assert int(deg2.item()) == 0 and _same_double(mx2.item(), wmx)
    on = np.zeros(n, bool)
    on[t.reshape(-1)] = True
    if name == "star and random":
        assert np.bincount(t[:, 2])[0] == 100 and (~on).sum() >= 20
        assert all_pos_zero(host(f)[~on])
        assert_bits_equal(host(acc)[~on], old[~on], "bodies on no triplet")
    if name == "one triplet":   # the three rows of a triplet: the centre's is the negated sum of the other two, exactly
        fh = host(f)
        assert (fh[1] == -fh[0] - fh[2]).all()
    h.close()


def test_angular_incidence_without_triplets():
    from mundy_amd import ops
    for n in (5, 1):
        h = ops.AngularSprings(n, np.zeros((0, 3), np.int32), 1.0, math.pi)
        x = dev(np.random.default_rng(n).normal(size=(n, 3)))
        f, deg, mx = h.force(x)
        assert all_pos_zero(host(f)) and int(deg.item()) == 0 and all_pos_zero(host(mx))
        old = dev(np.full((n, 3), -0.0))
        h.force(x, out=old, accumulate=True)
        assert_bits_equal(host(old), np.full((n, 3), -0.0), "untouched")
        assert h.cos_rest.shape == (0,) and h.triplets.shape == (0, 3)
        h.close()


# ---- the FENE-WCA bond, bit for bit --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wca", [None, (0.7, 0.9)])
@pytest.mark.parametrize("per_spring", [False, True])
@pytest.mark.parametrize("graph", ["chain", "random8", "matching"])
def test_fenewca_forces_bit_for_bit(graph, per_spring, wca):
    """the graphs of tests/test_gpu_chain.py's spring test; bond lengths from 0.6 (inside the cutoff) to past r_max
    (clamped)"""
    from mundy_amd import ops
    rng = np.random.default_rng(sum(map(ord, graph)) + 2 * per_spring)
    n = 3001 if graph != "matching" else 3000
    pairs = _graph(rng, graph, n).astype(np.int32)
    m = pairs.shape[0]
    if graph == "chain":
        steps = rng.normal(size=(n, 3))
        steps *= (rng.uniform(0.6, 1.6, n) / np.linalg.norm(steps, axis=1))[:, None]
        c = np.cumsum(steps, axis=0)
    else:
        c = rng.uniform(0, 1.6, (n, 3))
    k = rng.uniform(0.5, 30.0, m) if per_spring else 30.0
    r = rng.uniform(1.2, 2.0, m) if per_spring else 1.5
    s = ops.Springs(n, pairs, "fenewca", k, r)
    eps, sig = (1.0, 1.0) if wca is None else wca
    if wca is not None:
        s.set_wca(*wca)
    assert s.wca == (eps, sig)
    f, over, mx = s.force(dev(c))
    want, wover, wmx = bm.fenewca_force(n, pairs, k, r, c, eps, sig)
    assert_bits_equal(host(f), want, "%s %s %s" % (graph, per_spring, wca))
    L = np.linalg.norm(c[pairs[:, 1]] - c[pairs[:, 0]], axis=1)
    assert int(over.item()) == wover > 0 and _same_double(mx.item(), wmx) and np.isfinite(want).all()
    assert (L < bm.wca_cutoff(sig)).sum() > 10 and (L > bm.wca_cutoff(sig)).sum() > 10
    if graph == "matching":
        fh = host(f)
        assert (fh[pairs[:, 1]] == -fh[pairs[:, 0]]).all()
    s.close()


def test_set_wca_is_refused_for_the_other_types():
    from mundy_amd import capi, ops
    for kind in ("hookean", "fene"):
        s = ops.Springs(3, [[0, 1]], kind, 3.0, 1.5)
        with pytest.raises(ValueError, match="belong to 'fenewca'"):
            s.set_wca(1.0, 1.0)
        with pytest.raises(ValueError, match="MHIP_SPRING_FENEWCA"):   # and by the library itself
            capi.check(capi.load().mhip_springs_set_wca(s._h, 1.0, 1.0))
        s.close()
    s = ops.Springs(3, [[0, 1]], "fenewca", 3.0, 1.5)
    for eps, sig in ((0.0, 1.0), (1.0, math.inf)):
        with pytest.raises(ValueError, match="must be finite and > 0"):
            capi.check(capi.load().mhip_springs_set_wca(s._h, eps, sig))
    s.close()


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def _straight_chain_triplets(n):
    """the triplets (i, i + 2, i + 1) of a straight chain of n beads with unit spacing (cos(theta) = -1 exactly); the
    last one is listed as (n - 1, n - 3, n - 2), so that body n - 1 is a role-0 end too"""
    first = np.arange(n - 2)
    t = np.stack([first, first + 2, first + 1], axis=1).astype(np.int32)
    t[n - 3] = (n - 1, n - 3, n - 2)
    c = np.zeros((n, 3))
    c[:, 0] = np.arange(n)
    return c, t


@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_angular_statistics_are_found_wherever_they_sit(pos):
    """every triplet straight and at rest but the one whose role-0 end is body pos: its rest angle is pi / 2 (deviation
    |-1 - cos(pi / 2)|); then, in a second set, that triplet's centre sits on its first end (one arm of zero length)"""
    from mundy_amd import ops
    n = PAST_FULL_GRID
    c, t = _straight_chain_triplets(n)
    which = pos if pos < n - 2 else n - 3
    assert t[which, 0] == pos
    a = np.full(n - 2, math.pi)
    a[which] = 0.5 * math.pi
    h = ops.AngularSprings(n, t, 2.0, a)
    cr = h.cos_rest
    f, deg, mx = h.force(dev(c))
    want, wdeg, wmx = bm.angular_force(n, t, 2.0, cr, c)
    assert wdeg == 0 and wmx == abs(-1.0 - cr[which]) and 0.99 < wmx < 1.01
    assert int(deg.item()) == 0 and _same_double(mx.item(), wmx)
    assert_bits_equal(host(f), want, "one triplet off its rest angle, first end at %d" % pos)
    h.close()
    # a lone triplet list: only the degenerate one and two sound ones far from it
    far = (which + 1000) % (n - 2)
    t2 = np.stack([t[which], t[far], t[(far + 7) % (n - 2)]])
    c2 = c.copy()
    c2[t2[0, 2]] = c2[t2[0, 0]]
    h = ops.AngularSprings(n, t2, 2.0, 2.0)
    f, deg, mx = h.force(dev(c2))
    want, wdeg, wmx = bm.angular_force(n, t2, 2.0, h.cos_rest, c2)
    assert int(deg.item()) == wdeg == 1 and _same_double(mx.item(), wmx) and wmx > 0
    fh = host(f)
    assert np.isnan(fh[t2[0]]).all() and np.isfinite(fh[t2[1:].reshape(-1)]).all()
    h.close()


def test_degenerate_triplets_are_counted_once_each_and_the_stepper_raises():
    from mundy_amd import ops, pipeline
    c = np.array([[0.0, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [2.0, 0.5, 0], [3.0, 0, 0], [4.0, 1.0, 0]])
    t = np.array([[0, 2, 1], [1, 3, 2], [2, 4, 3], [3, 5, 4]], np.int32)   # beads 1 and 2 coincide: the first two
    h = ops.AngularSprings(6, t, 2.0, math.pi)
    f, deg, mx = h.force(dev(c))
    want, wdeg, wmx = bm.angular_force(6, t, 2.0, h.cos_rest, c)
    assert int(deg.item()) == wdeg == 2 and _same_double(mx.item(), wmx)
    # (a NaN is a NaN: its sign and payload are the hardware's; every other row in bits)
    fh = host(f)
    assert (np.isnan(fh) == np.isnan(want)).all() and np.isnan(fh[:4]).all() and np.isfinite(fh[4:]).all()
    assert_bits_equal(fh[4:], want[4:], "the rows no degenerate triplet touches")
    h.close()
    # (the Hertz contact: the two coincident beads touch, and a solve is not what this is about)
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(6, 0.1)), contact_model="hertz",
                                 angular_springs=(t, 2.0, math.pi))
    with pytest.raises(RuntimeError, match="angular spring"):
        st.step()


def test_clamped_fenewca_bonds_are_counted_and_the_stepper_reports_them():
    from mundy_amd import ops, pipeline
    c = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.6, 0, 0], [10.0, 0, 0]])
    pairs = np.array([[0, 1], [1, 2], [2, 3]])
    s = ops.Springs(4, pairs, "fenewca", 3.0, 1.5)
    f, over, mx = s.force(dev(c))
    want, wover, wmx = bm.fenewca_force(4, pairs, 3.0, 1.5, c)
    assert int(over.item()) == wover == 2 and float(mx.item()) == wmx == 7.4
    assert_bits_equal(host(f), want, "clamped bonds")
    assert np.isfinite(host(f)).all() and host(f)[3, 0] < -1e4   # pulled back with the clamped force
    s.close()
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(4, 0.3)), springs=(pairs, "fenewca", 3.0, 1.5), dt=1e-9)
    assert st.step().springs_overstretched == 2


# ---- renumbering ---------------------------------------------------------------------------------------------------------------------
def test_renumbered_triplets_give_the_same_rows_permuted():
    from mundy_amd import ops
    rng = np.random.default_rng(23)
    n, t = _star_and_random_triplets(rng)
    c = rng.uniform(0.0, 6.0, (n, 3))
    k, a = rng.uniform(0.5, 9.0, len(t)), rng.uniform(0.0, math.pi, len(t))
    ref = ops.AngularSprings(n, t, k, a)
    f0 = host(ref.force(dev(c))[0])
    ref.close()
    for name, new_of_old in renumberings(rng, n).items():
        h = ops.AngularSprings(n, t, k, a)
        h.renumber(dev(new_of_old))
        assert (h.triplets == new_of_old[t]).all()
        x = np.empty_like(c)
        x[new_of_old] = c
        f, deg, mx = h.force(dev(x))
        assert_bits_equal(host(f)[new_of_old], f0, name)
        assert int(deg.item()) == 0
        h.close()


# ---- the device against the gradient of the potential ------------------------------------------------------------------------------
@pytest.mark.parametrize("moved", [False, True], ids=["own frame", "rotated"])
@pytest.mark.parametrize("name", bc.NAMES)
def test_device_forces_are_the_gradient_of_the_potential(name, moved):
    """held to -grad U from mpmath at the K measured on the host from the numpy model (bending_cases.TOLERANCE_K)"""
    from mundy_amd import ops
    case = bc.cases()[name]
    x = case.moved() if moved else case.x
    if case.kind == "fenewca":
        h = ops.Springs(case.n, case.pairs, "fenewca", case.k, case.r_max)
        h.set_wca(*case.wca)
        f = host(h.force(dev(x))[0])
        F, S = bc.exact(name, moved)
    else:
        h = ops.AngularSprings(case.n, case.triplets, case.k, case.rest_angle)
        f = host(h.force(dev(x))[0])
        F, S = bc.exact(name, moved, cos_rest=h.cos_rest)
    h.close()
    d = gc.deviation(f, F, S)
    print("%s: worst deviation of the device %.3g eps S_b (K = %g)" % (name, d.max(), bc.TOLERANCE_K[case.group]))
    assert np.isfinite(d).all() and d.max() <= bc.TOLERANCE_K[case.group]


# ---- the stepper against the composed models -----------------------------------------------------------------------------------------
K_ANGLE, REST_ANGLE = 4.0, 2.8


def _bending_stepper(case, bond, **kw):
    from mundy_amd import pipeline, synth
    n = case["n"]
    trip = synth.chain_triplets(np.arange(0, n + 1, hp1.BEADS))
    springs = ((case["pairs"], "hookean", case["spring_k"], case["spring_r"]) if bond == "hookean" else
               (case["pairs"], "fenewca", 30.0, 1.5))
    opts = dict(dt=case["dt"], viscosity=case["viscosity"], search_buffer=case["search_buffer"], contact_model="hertz",
                youngs_modulus=case["youngs_modulus"], poisson_ratio=case["poisson_ratio"], brownian_kt=case["kt"],
                springs=springs, angular_springs=(trip, K_ANGLE, REST_ANGLE))
    if bond == "fenewca":
        opts["spring_wca"] = (0.8, 0.95)
    opts.update(kw)
    return pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), **opts), trip


@pytest.mark.parametrize("bond,hydro", [("hookean", False), ("fenewca", False), ("hookean", True)])
def test_step_is_the_composed_models(bond, hydro):
    """20 steps of springs, angular springs, noise and Hertz contacts (hp1_case's chains), each from the stepper's own
    state at its start: the force field, U_ext and the velocity bit for bit.  reorder_bodies before step 7 (the models
    then take the handle's renumbered triplets and the stepper's renumbered pairs); step 12 is run, restored and run
    again.  hydro: the Hertz force is the first term of the field and u_hydro of the whole field is added to U_ext."""
    from mundy_amd import ops
    case = hp1.build("UH" if hydro else "H")
    n, radius = case["n"], case["radius"]
    kw = dict(hydrodynamics=dict(kind="rpyc", update_every=1, contact_forces=True)) if hydro else {}
    st, trip = _bending_stepper(case, bond, **kw)
    cr = st.angular.cos_rest
    assert cr.shape == (len(trip),) and abs(cr[0] - math.cos(REST_ANGLE)) <= 2e-16
    mt = host(st.mob_trans)
    acted = 0
    for step in range(20):
        if step == 7:
            perm = host(st.reorder_bodies()).astype(np.int64)
            inv = np.empty_like(perm)
            inv[perm] = np.arange(n)
            assert (st.angular.triplets == inv[trip]).all() and (st.angular.triplets != trip).any()
            assert_bits_equal(st.angular.cos_rest, cr, "the cosines stay")
        snap = st.snapshot() if step == 12 else None
        x0 = host(st.center).copy()
        keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
        s = st.step()
        if snap is not None:
            first = {k: host(getattr(st, k)).copy() for k in ("center", "spring_force", "u_ext", "velocity")}
            st.restore(snap)
            s2 = st.step()
            for k, v in first.items():
                assert_bits_equal(host(getattr(st, k)), v, "step 12 again after restore: %s" % k)
            assert (s2.max_angle_deviation, s2.max_spring_length) == (s.max_angle_deviation, s.max_spring_length)
        pairs_now, trip_now = st._spring_spec[0], st.angular.triplets
        if bond == "hookean":
            F, over, wlen = chm.spring_force(n, pairs_now, "hookean", case["spring_k"], case["spring_r"], x0)
        else:
            F, over, wlen = bm.fenewca_force(n, pairs_now, 30.0, 1.5, x0, 0.8, 0.95)
        if hydro:   # F = (D f + F_spring) + F_angular
            F = hp1.contact_force(case, host(st.links.pairs), host(st.lam), host(st.contacts["normal"])) + F
        F, wdeg, wdev = bm.angular_force(n, trip_now, K_ANGLE, cr, x0, force=F)
        assert_bits_equal(host(st.spring_force), F, "step %d: the force field" % step)
        assert s.angular_degenerate == wdeg == 0 and _same_double(s.max_angle_deviation, wdev) and wdev > 0
        assert s.springs_overstretched == over == 0 and _same_double(s.max_spring_length, wlen)
        only_angular = bm.angular_force(n, trip_now, K_ANGLE, cr, x0)[0]
        acted += int(np.abs(only_angular).max() > 0.0)
        u_hydro = 0.0
        if hydro:
            u_hydro = host(st.u_hydro)
            # (the stepper sums the hydrodynamics in the constructor's numbering, whatever reorder_bodies did since)
            rows = np.arange(n) if st._hydro_rows is None else host(st._hydro_rows).astype(np.int64)
            numbers = np.arange(n) if st._hydro_numbers is None else host(st._hydro_numbers).astype(np.int64)
            want_h = hydro_model.velocity("rpyc", case["viscosity"], x0[rows], radius[rows], F[rows])[numbers]
            assert_bits_equal(u_hydro, want_h, "step %d: u_hydro of the whole force field" % step)
        base = host(ops.brownian_velocity(keys, ctr, case["kt"], case["dt"], st.mob_trans,
                                          ops.drag_velocity(st.mob_trans, dev(F))))
        u_ext = host(st.u_ext)
        assert_bits_equal(u_ext[:, :3], base[:, :3] + u_hydro, "step %d: U_ext" % step)
        vel = host(st.velocity)
        if hydro:
            assert_bits_equal(vel, u_ext, "step %d: U = U_ext" % step)
        else:
            assert_bits_equal(vel, u_ext + host(st.op.body_velocity_of(st.lam)), "step %d: U = U_ext + M D f" % step)
        assert s.num_contacts > 0 and s.max_overlap > 0
        assert_bits_equal(host(st.center), x0 + st.dt * vel[:, :3], "step %d: Euler" % step)
    assert acted == 20 and mt.shape == (n,)


def test_without_the_new_options_the_step_is_what_it_was():
    """angular_springs=None and spring_wca=None are the stepper without the keywords: no handle, no statistics array, the
    same bits (the untouched options against the C++ stepper: tests/test_gpu_chain.py::test_chain_step_app_matches_python,
    as before)"""
    from mundy_amd import pipeline
    case = hp1.build("H")
    kw = hp1.stepper_kwargs(case)
    a = pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), **kw)
    b = pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), angular_springs=None, spring_wca=None,
                                **kw)
    assert b.angular is None and not hasattr(b, "_bending_stats") and "bending" not in b._modes
    for _ in range(3):
        sa, sb = a.step(), b.step()
        assert_bits_equal(host(a.center), host(b.center), "explicit defaults")
        assert sa.max_spring_length == sb.max_spring_length and sb.max_angle_deviation == 0.0


# ---- physics ---------------------------------------------------------------------------------------------------------------------------
def test_a_bent_three_bead_chain_relaxes_monotonically_to_straight():
    """theta0 = pi, no noise, no contacts, no bonds: U = 1/2 k (1 + cos(theta))^2 never rises, and ends below 1e-12 (k = 1:
    the bar in units of k, the bar of the closed-form relaxations of DESIGN.md 5g).  About theta = pi the potential is
    quartic in the bend phi = pi - theta, U ~ k phi^4 / 8, so the relaxation is algebraic, phi' = phi (1 - 3 a phi^2) per
    step with a = dt m_t k / L^2, not exponential: the bar U = 1e-12 is phi = 1.7e-3, reached after ~1 / (6 a phi^2) steps.
    A step of a = 32 is monotone for a bend of 0.07 (3 a phi^2 = 0.47 < 1) and needs ~1850 steps (the numpy model: 1833);
    2400 are run.  U is read from the step's own statistic: max_angle_deviation = |cos(theta) - cos(theta0)|."""
    from mundy_amd import pipeline
    phi = 0.07
    x = np.array([[-math.cos(phi / 2), math.sin(phi / 2), 0.0], [math.cos(phi / 2), math.sin(phi / 2), 0.0], [0.0, 0.0, 0.0]])
    x[:, 2] += np.array([0.01, -0.02, 0.0])
    st = pipeline.ContactStepper("sphere", dev(x), dev(np.full(3, 0.05)), dt=32.0, mob_trans=dev(np.ones(3)),
                                 angular_springs=([[0, 1, 2]], 1.0, math.pi))
    assert st.angular.cos_rest[0] == -1.0
    U = []
    for _ in range(2400):
        s = st.step()
        assert s.num_contacts == 0
        U.append(0.5 * s.max_angle_deviation ** 2)
    U = np.array(U)
    print("U: %.3g -> %.3g, first below 1e-12 at step %d" % (U[0], U[-1], int(np.argmax(U <= 1e-12))))
    assert U[0] > 3e-6 and (np.diff(U) <= 0).all()
    assert U[-1] <= 1e-12
    xf = host(st.center)
    v1, v2 = xf[0] - xf[2], xf[1] - xf[2]
    assert 1.0 + v1 @ v2 / math.sqrt((v1 @ v1) * (v2 @ v2)) <= math.sqrt(2e-12) * 1.001


# ---- the C++ stepper ------------------------------------------------------------------------------------------------------------------
def _app_input(case, trip, path):
    with open(path, "wb") as f:
        np.array([case["n"], case["pairs"].shape[0], trip.shape[0]], dtype=np.uint64).tofile(f)
        for a in (case["center"], case["radius"], case["mob_trans"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        case["pairs"].astype(np.int32).tofile(f)
        trip.astype(np.int32).tofile(f)


@pytest.mark.parametrize("bond", ["hookean", "fenewca"])
def test_bending_step_app_matches_python(bond, tmp_path):
    """mech::SphereChainStepper with set_angular_springs (and MHIP_SPRING_FENEWCA + set_spring_wca) against the Python
    stepper over 20 steps of the LCP step: STEP lines and the checksums of the centres and of the last force field"""
    from cpp_apps import build_app, checksums, fnv1a_bits
    case = hp1.build("")
    st, trip = _bending_stepper(case, bond, contact_model="lcp")
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d max_spring_length %.17g springs_overstretched %d "
                     "max_angle_deviation %.17g angular_degenerate %d" % (
                         k, s.num_contacts, s.num_iters, s.max_spring_length, s.springs_overstretched,
                         s.max_angle_deviation, s.angular_degenerate))
    exe = build_app("bending_step_app")
    path = str(tmp_path / "in.bin")
    _app_input(case, trip, path)
    spring = ["0", repr(case["spring_k"]), repr(case["spring_r"])] if bond == "hookean" else ["2", "30.0", "1.5"]
    args = [exe, path, "20", repr(case["dt"]), repr(case["search_buffer"])] + spring + [
        repr(case["kt"]), repr(K_ANGLE), repr(REST_ANGLE)] + (["0.8", "0.95"] if bond == "fenewca" else [])
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:14]) for g in got] == lines
    cs = checksums(out.stdout)
    assert cs["center"] == fnv1a_bits(host(st.center)) and cs["force"] == fnv1a_bits(host(st.spring_force))
    # and the stepper's refusals, which are the library's: a rest angle past pi, a WCA sigma of zero, set_wca on Hookean
    bad = list(args)
    bad[10] = "3.5"
    refusals = [(bad, "rest angle")]
    if bond == "fenewca":
        refusals.append((args[:11] + ["0.8", "0.0"], "sigma"))
    else:
        refusals.append((args + ["0.8", "0.95"], "MHIP_SPRING_FENEWCA"))
    for a, match in refusals:
        r = subprocess.run(a, capture_output=True, text=True, timeout=120)
        assert r.returncode == 4 and "REFUSED" in r.stderr and match in r.stderr, (r.returncode, r.stderr)
