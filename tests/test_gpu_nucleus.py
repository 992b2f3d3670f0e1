"""The nucleus terms of the chain step on the device (periphery.hip, active.hip) against the numpy model
(periphery_model.py, with the oracle's distance and rotations: the device's IEEE sequence), the closed-form relaxation
at a wall, the telegraph process of the active springs, the stepper's carry of their state, the C++ driver and the
full-size step."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import chain_model as cm
import crosslinker_model as xm
import periphery_model as pm
from gpu_util import (PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host, line_with_one_long_bond,
                      renumberings, star_and_random_graph, star_graph)

pytestmark = pytest.mark.gpu
PAST_GRID_CAP = 2048 * 256 + 77   # grid_for caps the grid at 2048 workgroups of 256: lanes take a second body here
SIZES = (1, 63, 257, 20001)


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return q / np.linalg.norm(q)


def _rotate(oracle):
    """the oracle's quaternion rotate in the model's signature"""
    return lambda quat, v: oracle.quat_rotate(np.tile(np.asarray(quat, dtype=np.float64), (len(v), 1)), v)


def _oracle_distance(oracle, pc, quat, radii):
    """(sd, pn) of the device's S-E class: oracle.contact_mixed on (bead as a sphere of radius 0, periphery as the
    ellipsoid), route 0, returns sep = sd - 0.0 and normal = -n in the lab frame"""
    def distance(points):
        k = len(points)
        kind = np.array([0] * k + [2], np.int32)
        center = np.vstack([points, np.asarray(pc, dtype=np.float64)])
        q = np.vstack([np.tile([1.0, 0.0, 0.0, 0.0], (k, 1)), np.asarray(quat, dtype=np.float64)])
        shape = np.vstack([np.zeros((k, 3)), np.asarray(radii, dtype=np.float64)])
        pairs = np.stack([np.arange(k), np.full(k, k)], axis=1).astype(np.int32)
        out = oracle.contact_mixed(pairs, kind, center, q, shape)
        return out["sep"], out["normal"]
    return distance


def _beads(rng, n, radii, pc, quat, special=True):
    """n beads at 0.5 .. 1.1 of the surface (the medial set is never evaluated): deep inside, within one radius of the
    wall, touching, outside; with `special`, beads on every symmetry plane and axis (exact-zero body coordinates; only
    an unrotated periphery at the origin keeps them exact)"""
    e = np.asarray(radii, dtype=np.float64)
    scale = np.where(rng.random(n) < 0.4, rng.uniform(0.5, 0.85, n), rng.uniform(0.9, 1.1, n))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    y = d * e * scale[:, None]
    r = rng.uniform(0.05, 0.15, n)
    if special and n >= 63:
        k = 0
        for zero in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2)):       # planes, then axes
            for s in (0.6, 0.93, 0.99, 1.0, 1.06):
                y[k, list(zero)] = 0.0
                y[k] *= s / math.sqrt(((y[k] / e) ** 2).sum())
                k += 1
        for a in range(3):                                            # touching along each axis, to the last bit and next
            for off in (0.0, 1e-15, -1e-15):
                y[k] = 0.0
                y[k, a] = e[a] - r[k] + off
                k += 1
        y[k] = 0.0                                                    # the periphery's centre: filtered
    c = pm.quat_rotate(quat, y) + np.asarray(pc, dtype=np.float64)
    return np.ascontiguousarray(c), r


def _device(spec, c, r, base):
    from mundy_amd import ops
    out = None if base is None else dev(base.copy())
    f, col, mx = ops.periphery_force(spec, dev(c), dev(r), out=out, accumulate=base is not None)
    return host(f), int(host(col)[0]), float(host(mx)[0])


def _compare(got, want, what):
    assert_bits_equal(got[0], want[0], what + ": force")
    assert got[1] == want[1], (what, "colliding", got[1], want[1])
    assert np.float64(got[2]).view(np.uint64) == np.float64(want[2]).view(np.uint64), (what, "max_overlap", got[2], want[2])


# ---- 1. periphery, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", [(0.0, 0.0, 0.0), (0.75, -1.5, 2.25)])
def test_sphere_periphery_bit_for_bit(pc):
    rng = np.random.default_rng(11)
    R, K = 2.5, 7.0
    hits = 0
    for n in SIZES + ((PAST_GRID_CAP,) if pc[0] else ()):
        c, r = _beads(rng, n, (R, R, R), pc, (1.0, 0.0, 0.0, 0.0))
        spec = dict(shape="sphere", radius=R, k=K, center=pc)
        want = pm.sphere_force(c, r, R, K, pcenter=pc)
        _compare(_device(spec, c, r, None), want, "sphere n = %d" % n)
        base = rng.normal(size=(n, 3))
        _compare(_device(spec, c, r, base), pm.sphere_force(c, r, R, K, pcenter=pc, force=base), "sphere, added, n = %d" % n)
        hits += want[1]
        if n >= 257:
            assert 0.1 * n < want[1] < 0.6 * n and want[2] > 0.1
    assert hits > 0


@pytest.mark.parametrize("radii,pc,quat,big", [
    ((3.0, 2.0, 1.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), False),     # all different; exact-zero body coordinates
    ((2.0, 3.0, 3.0), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), False),     # two equal
    ((2.5, 2.5, 2.5), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), False),     # all equal
    ((1.5, 3.0, 2.0), (0.75, -1.5, 2.25), (0.9, 0.1, -0.3, 0.2), True),  # shifted and rotated
    ((2.0, 2.0, 3.0), (-4.0, 0.5, 0.0), (0.2, -0.7, 0.1, 0.6), False)])
def test_ellipsoid_periphery_bit_for_bit(oracle, radii, pc, quat, big):
    rng = np.random.default_rng(12)
    quat = tuple(_unit(quat)) if quat[0] != 1.0 else quat
    K = 7.0
    rot, dist = _rotate(oracle), _oracle_distance(oracle, pc, quat, radii)
    spec = dict(shape="ellipsoid", radii=radii, k=K, center=pc, quat=quat)
    for n in SIZES + ((PAST_GRID_CAP,) if big else ()):
        c, r = _beads(rng, n, radii, pc, quat)
        want = pm.ellipsoid_force(c, r, radii, K, pc, quat, distance=dist, rotate=rot)
        _compare(_device(spec, c, r, None), want, "ellipsoid n = %d" % n)
        base = rng.normal(size=(n, 3))
        _compare(_device(spec, c, r, base),
                 pm.ellipsoid_force(c, r, radii, K, pc, quat, force=base, distance=dist, rotate=rot),
                 "ellipsoid, added, n = %d" % n)
        if n >= 257:
            filtered = pm.ellipsoid_filter(c, r, radii, pc, quat, rot)
            assert 0.1 * n < filtered.sum() < 0.6 * n and 0.1 * n < want[1] < 0.6 * n and want[2] > 0.1
            untouched = np.abs(want[0]).sum(axis=1) == 0
            assert untouched[filtered].all() and not np.signbit(want[0][untouched]).any()


def test_fast_ellipsoid_periphery_bit_for_bit():
    rng = np.random.default_rng(13)
    radii, pc, K = (3.0, 2.0, 1.5), (0.75, -1.5, 2.25), 7.0
    spec = dict(shape="ellipsoid_fast", radii=radii, k=K, center=pc)
    for n in SIZES + (PAST_GRID_CAP,):
        c, r = _beads(rng, n, radii, pc, (1.0, 0.0, 0.0, 0.0))
        want = pm.ellipsoid_fast_force(c, r, radii, K, pcenter=pc)
        _compare(_device(spec, c, r, None), want, "fast n = %d" % n)
        base = rng.normal(size=(n, 3))
        _compare(_device(spec, c, r, base), pm.ellipsoid_fast_force(c, r, radii, K, pcenter=pc, force=base),
                 "fast, added, n = %d" % n)
        if n >= 257:
            assert 0.1 * n < want[1] < 0.7 * n


def _beads_on_the_axes(pos, n=PAST_FULL_GRID, R=2.0):
    """beads of radius 0.5 on the coordinate axes of a sphere of radius R: at distance 1.75 (overlap 0.25), every third
    one at 1.0 (inside, untouched), bead pos at 2.0 (overlap 0.5); all exact"""
    dist = np.full(n, R - 0.25)
    dist[1::3] = 1.0
    dist[pos] = R
    c = np.zeros((n, 3))
    c[np.arange(n), (np.arange(n) // 3) % 3] = dist
    return c, np.full(n, 0.5)


@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_periphery_statistics_are_found_wherever_they_sit(pos):
    c, r = _beads_on_the_axes(pos)
    want = pm.sphere_force(c, r, 2.0, 7.0)
    assert want[2] == 0.5 and want[1] == len(c) - len(c[1::3]) + (pos % 3 == 1)
    _compare(_device(dict(shape="sphere", radius=2.0, k=7.0), c, r, None), want, "axes, deep bead at %d" % pos)


def test_periphery_accumulate_leaves_untouched_rows_untouched():
    """a bead the wall does not touch keeps its row, -0.0 included (force + 0.0 would make it +0.0)"""
    rng = np.random.default_rng(15)
    c, r = _beads_on_the_axes(0, n=20001)
    inside = np.zeros(len(c), bool)
    inside[1::3] = True
    base = rng.normal(size=c.shape)
    base[inside] = -0.0
    for spec, model in ((dict(shape="sphere", radius=2.0, k=7.0), lambda: pm.sphere_force(c, r, 2.0, 7.0, force=base)),
                        (dict(shape="ellipsoid_fast", radii=(2.0, 2.0, 2.0), k=7.0),
                         lambda: pm.ellipsoid_fast_force(c, r, (2.0, 2.0, 2.0), 7.0, force=base)),
                        (dict(shape="ellipsoid", radii=(2.0, 2.0, 2.0), k=7.0), None)):
        got = _device(spec, c, r, base)
        assert got[1] == int((~inside).sum()) and (got[0][inside].view(np.uint64) == 1 << 63).all(), spec["shape"]
        assert (got[0][~inside] != base[~inside]).any(axis=1).all()
        if model is not None:
            _compare(got, model(), spec["shape"] + ", added into -0.0 rows")


def test_ellipsoid_periphery_against_the_reference_routine(oracle):
    """The reference's existing routine, distance(SharedNormalSigned, Point, Ellipsoid), is a nine-start L-BFGS good to
    eps = 1e-4 in the distance (UnitTestEllipsoidEllipsoid.cpp:52-53).  Force = K pn ssd, so a distance error eps moves
    it by K eps.  The normal: measured on the CPU model (periphery_model.exact_distance against the routine's normal),
    max |n_ref - n| = 6.4e-7 on the 500 points of this test and 1.1e-7 .. 7.9e-7 on five other draws of 500 from the
    same shell; the allowance is theta = 4e-6, five times the largest of the six.  (The routine's eps alone would allow
    theta <= sqrt(4 eps d) / rho_min = 0.0146 at d = 0.3, rho_min = c^2 / a = 0.75: it converges far closer than its
    own margin, and the allowance follows the measurement, not that worst case.)  So |dF| <= K (eps + |ssd| theta)."""
    rng = np.random.default_rng(14)
    n, K = 500, 7.0
    radii, pc, quat = (3.0, 2.0, 1.5), (0.3, -0.2, 0.5), tuple(_unit((0.9, 0.1, -0.3, 0.2)))
    y = pm.surface_points(rng, n, radii, 0.93, 1.1)
    c, r = pm.quat_rotate(quat, y) + np.asarray(pc), rng.uniform(0.05, 0.15, n)
    got = _device(dict(shape="ellipsoid", radii=radii, k=K, center=pc, quat=quat), c, r, None)

    def reference(points):
        k = len(points)
        d, _, nrm = oracle.distance_point_ellipsoid(points, np.tile(pc, (k, 1)), np.tile(quat, (k, 1)),
                                                    np.tile(radii, (k, 1)))
        return d, -nrm
    ref = pm.ellipsoid_force(c, r, radii, K, pc, quat, distance=reference, rotate=_rotate(oracle))
    sd, pn = pm.exact_distance(c, pc, quat, radii)
    ssd = -sd - r
    assert np.abs(sd).max() <= 0.3 + 1e-9 and got[1] > 100
    eps, theta = 1e-4, 4e-6
    d_ref, pn_ref = reference(c)
    turn = np.linalg.norm(pn_ref - pn, axis=1)
    err = np.linalg.norm(got[0] - ref[0], axis=1)
    print("against the reference routine: max |dF| = %.3g (K eps = %.3g), max |d_ref - sd| = %.3g, max |n_ref - n| = %.3g, "
          "colliding %d vs %d" % (err.max(), K * eps, np.abs(d_ref - sd).max(), turn.max(), got[1], ref[1]))
    assert (turn <= theta).all()
    assert (err <= K * (eps + np.abs(ssd) * theta)).all()
    assert (np.abs(np.linalg.norm(got[0], axis=1) - np.linalg.norm(ref[0], axis=1)) <= K * 1e-4).all()


# ---- 2. closed form: a bead relaxing at the wall ----------------------------------------------------------------------
def _two_beads(per, x0, y0, r=0.5):
    """two beads outside the wall along +x and +y, neighbours in the list but far from touching; no noise"""
    from mundy_amd import pipeline
    c = np.array([[x0, 0.0, 0.0], [0.0, y0, 0.0]])
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(2, r)), dt=1e-3, viscosity=1.0, search_buffer=4.0,
                                   periphery=per)


@pytest.mark.parametrize("shape", ["sphere", "ellipsoid"])
def test_overlap_decays_geometrically_at_the_wall(shape):
    r, K, d0, steps = 0.5, 40.0, 0.25, 50
    radii = (2.0, 2.0, 2.0) if shape == "sphere" else (2.0, 3.0, 4.0)
    per = dict(shape="sphere", radius=2.0, k=K) if shape == "sphere" else dict(shape="ellipsoid", radii=radii, k=K)
    st = _two_beads(per, radii[0] - r + d0, radii[1] - r + 2 * d0)
    mt = float(host(st.mob_trans)[0])
    rate = 1.0 - st.dt * mt * K
    for s in range(steps):
        stat = st.step()
        assert stat.num_contacts == 1 and stat.periphery_colliding == 2 and float(st.contacts["sep"].min()) > 0.5
        want = 2 * d0 * rate ** s
        assert abs(stat.max_periphery_overlap - want) <= 1e-12 * want
    c = host(st.center)
    for got, start in ((c[0, 0] - (radii[0] - r), d0), (c[1, 1] - (radii[1] - r), 2 * d0)):
        want = start * rate ** steps
        print("%s: overlap after %d steps %.15g, closed form %.15g" % (shape, steps, got, want))
        assert abs(got - want) <= 1e-12 * want
    assert c[0, 1] == 0 and c[0, 2] == 0 and c[1, 0] == 0 and c[1, 2] == 0
    # the compression run: the wall shrinks between steps, the overlap is what the new radius implies
    st.scale_periphery(0.9)
    stat = st.step()
    assert abs(stat.max_periphery_overlap - (c[1, 1] - (0.9 * radii[1] - r))) <= 1e-13
    with pytest.raises(ValueError, match="bead radius"):
        st.scale_periphery(0.2)
    snap = st.snapshot()
    st.scale_periphery(1.5)
    assert st.step().periphery_colliding == 0
    st.restore(snap)
    assert st.periphery["radii"] == [0.9 * v for v in radii]


# ---- 3. active springs -----------------------------------------------------------------------------------------------------
def _state(act):
    st, nt, el, ct = act.state()
    return dict(state=host(st), next_time=host(nt), elapsed=host(el), counters=host(ct).view(np.uint64))


def test_active_sampling_follows_the_model_round_by_round():
    from mundy_amd import ops
    m, dt, kon, koff = 10 ** 5, 0.05, 10.0, 9.0
    rng = np.random.default_rng(21)
    keys = rng.permutation(2 ** 40 + np.arange(m)).astype(np.int64)
    ctr0 = rng.integers(0, 2 ** 62, m)
    pairs = np.stack([np.arange(m), np.arange(m) + 1], axis=1)
    act = ops.ActiveSprings(m + 1, pairs, 1.0, kon, koff, keys=keys, counter=ctr0)
    ku = keys.view(np.uint64)
    dv = _state(act)
    want = pm.active_init(ku, ctr0.astype(np.uint64), kon)
    assert (dv["state"] == 0).all() and (dv["elapsed"] == 0).all() and (dv["counters"] == want["counters"]).all()
    worst = float(np.abs(dv["next_time"] / want["next_time"] - 1.0).max())
    total_on = total_off = 0
    for rnd in range(30):
        sw = host(act.sample())
        # the model decides each spring from the device's previous (elapsed, next_time): the same doubles on both sides
        want, (on, off) = pm.active_sample(dv, ku, kon, koff)
        dv = _state(act)
        assert (int(sw[0]), int(sw[1])) == (on, off)
        assert (dv["state"] == want["state"]).all() and (dv["counters"] == want["counters"]).all()
        assert_bits_equal(dv["elapsed"], want["elapsed"], "elapsed after sampling")
        rel = np.abs(dv["next_time"] - want["next_time"]) / want["next_time"]
        worst = max(worst, float(rel.max()))
        total_on, total_off = total_on + on, total_off + off
        act.advance(dt)
        adv = host(act.state()[2])
        assert_bits_equal(adv, dv["elapsed"] + dt, "elapsed after advance")
        dv["elapsed"] = adv
    print("30 rounds: %d switched on, %d off; next_time: max relative error %.3g" % (total_on, total_off, worst))
    assert total_on > 3 * m and total_off > 3 * m and worst <= 1e-13
    # a spring that did not switch drew nothing
    assert (dv["counters"] - ctr0.astype(np.uint64) - np.uint64(1)).sum() == total_on + total_off
    act.close()


def _graphs():
    rng = np.random.default_rng(22)
    n = 3001
    chain = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    m = 4 * n
    g = rng.integers(0, n, (3 * m, 2))
    g = g[g[:, 0] != g[:, 1]]
    deg = np.zeros(n, int)
    keep = []
    for i, j in g:                      # degree <= 8
        if deg[i] < 8 and deg[j] < 8:
            deg[i] += 1
            deg[j] += 1
            keep.append((i, j))
    perm = rng.permutation(n - 1)
    matching = np.stack([perm[0::2][:(n - 1) // 2], perm[1::2][:(n - 1) // 2]], axis=1)
    return n, dict(chain=chain, graph=np.array(keep), matching=matching)


@pytest.mark.parametrize("which", ["chain", "graph", "matching"])
def test_active_forces_bit_for_bit(which):
    from mundy_amd import ops
    n, graphs = _graphs()
    pairs = graphs[which]
    m = pairs.shape[0]
    rng = np.random.default_rng(23)
    center = rng.normal(size=(n, 3)) * 3.0
    state = (rng.random(m) < 0.4).astype(np.int32)
    sigma = 2.5
    act = ops.ActiveSprings(n, pairs, sigma, 1.0, 1.0)
    act.set_state(state=dev(state))
    f, na = act.force(dev(center))
    want, count = pm.active_force(n, pairs, state, sigma, center)
    assert_bits_equal(host(f), want, which)
    assert int(host(na)[0]) == count == int(state.sum())
    base = rng.normal(size=(n, 3))
    f2, na2 = act.force(dev(center), out=dev(base.copy()), accumulate=True)
    assert_bits_equal(host(f2), pm.active_force(n, pairs, state, sigma, center, force=base)[0], which + ", added")
    assert int(host(na2)[0]) == count
    got = host(f)
    if which == "matching":
        on = pairs[state == 1]
        assert_bits_equal(got[on[:, 0]], -got[on[:, 1]], "the two ends")
        idle = np.ones(n, bool)
        idle[on.ravel()] = False
        assert idle.sum() > n // 2 and not got[idle].any() and not np.signbit(got[idle]).any()
        assert_bits_equal(host(f2)[idle], base[idle], "untouched rows")
        assert all(math.fsum(got[:, k]) == 0.0 for k in range(3))   # (fsum: the exact sum)
    else:
        assert np.abs(got.sum(axis=0)).max() < 1e-9
    # a renumbering of the bodies: the same forces in the new rows
    perm = rng.permutation(n)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    act.renumber(dev(inv.astype(np.int32)))
    f3, _ = act.force(dev(center[perm]))
    assert_bits_equal(host(f3), want[perm], which + ", renumbered")
    act.close()


def test_active_count_past_a_full_grid():
    from mundy_amd import ops
    n = PAST_FULL_GRID
    center, pairs = line_with_one_long_bond(0)
    state = (np.random.default_rng(24).random(n - 1) < 0.4).astype(np.int32)
    act = ops.ActiveSprings(n, pairs, 2.5, 1.0, 1.0)
    act.set_state(state=dev(state))
    f, na = act.force(dev(center))
    want, count = pm.active_force(n, pairs, state, 2.5, center)
    assert int(host(na)[0]) == count == int(state.sum()) > 0
    assert_bits_equal(host(f), want, "line")
    act.close()


@pytest.mark.parametrize("case", ["no springs", "one body", "star"])
def test_active_incidence_empty_and_star(case):
    from mundy_amd import ops
    rng = np.random.default_rng(25)
    n, pairs = {"no springs": (5, np.zeros((0, 2), np.int32)), "one body": (1, np.zeros((0, 2), np.int32)),
                "star": star_graph()}[case]
    m = pairs.shape[0]
    center = rng.normal(size=(n, 3))
    state = (rng.random(m) < 0.7).astype(np.int32)
    act = ops.ActiveSprings(n, pairs, 2.5, 1.0, 1.0)
    if m:
        act.set_state(state=dev(state))
    assert not host(act.sample()).any()   # (nothing has elapsed: no spring switches, whatever m)
    f, na = act.force(dev(center))
    want, count = pm.active_force(n, pairs, state, 2.5, center)
    assert_bits_equal(host(f), want, case)
    assert int(host(na)[0]) == count == int(state.sum())
    if case == "star":
        assert count > 50 and all_pos_zero(host(f)[101:])
    else:
        assert all_pos_zero(host(f))
    act.close()


def test_active_accumulate_leaves_untouched_rows_untouched():
    """a body without an active spring keeps its row, -0.0 included"""
    from mundy_amd import ops
    rng = np.random.default_rng(26)
    n, pairs = star_and_random_graph(rng)
    state = (rng.random(pairs.shape[0]) < 0.2).astype(np.int32)
    state[:100] = 0                                # the hub's springs are all off: listed, yet untouched
    center = rng.normal(size=(n, 3)) * 3.0
    idle = np.ones(n, bool)
    idle[pairs[state == 1].ravel()] = False
    base = rng.normal(size=(n, 3))
    base[idle] = -0.0
    act = ops.ActiveSprings(n, pairs, 2.5, 1.0, 1.0)
    act.set_state(state=dev(state))
    f, _ = act.force(dev(center), out=dev(base.copy()), accumulate=True)
    got = host(f)
    assert idle[:121].all() and idle.sum() > 200 and (got[idle].view(np.uint64) == 1 << 63).all()
    assert_bits_equal(got, pm.active_force(n, pairs, state, 2.5, center, force=base)[0], "added into -0.0 rows")
    act.close()


@pytest.mark.parametrize("which", ["reversed", "random"])
def test_renumbered_active_springs_equal_a_fresh_handle(which):
    from mundy_amd import ops
    rng = np.random.default_rng(27)
    n, pairs = star_and_random_graph(rng)
    new_of_old = renumberings(rng, n)[which]
    state = (rng.random(pairs.shape[0]) < 0.5).astype(np.int32)
    center_old = rng.normal(size=(n, 3)) * 3.0
    center = np.empty_like(center_old)
    center[new_of_old] = center_old
    act = ops.ActiveSprings(n, pairs, 2.5, 1.0, 1.0)
    act.set_state(state=dev(state))
    act.renumber(dev(new_of_old))
    fresh = ops.ActiveSprings(n, new_of_old[pairs], 2.5, 1.0, 1.0)
    fresh.set_state(state=dev(state))
    (f, na), (g, nb) = act.force(dev(center)), fresh.force(dev(center))
    assert_bits_equal(host(f), host(g), "fresh handle")
    assert int(host(na)[0]) == int(host(nb)[0]) == int(state.sum())
    assert_bits_equal(host(f)[new_of_old], pm.active_force(n, pairs, state, 2.5, center_old)[0],
                      "model in the old numbering")
    act.close()
    fresh.close()


def test_active_fraction_reaches_the_stationary_value():
    from mundy_amd import ops
    M, dt, kon, koff, rounds = 10 ** 6, 0.05, 8.0, 12.0, 50
    assert (kon + koff) * rounds * dt >= 40
    pairs = np.stack([np.arange(M), np.arange(M) + 1], axis=1)
    act = ops.ActiveSprings(M + 1, pairs, 1.0, kon, koff)
    for _ in range(rounds):
        act.sample()
        act.advance(dt)
    frac = float(host(act.state()[0]).mean())
    # dwell times in rounds are ceil(T / dt), T exponential: geometric, mean 1 / (1 - exp(-k dt)); on ends at koff
    e_on, e_off = 1.0 / (1.0 - math.exp(-koff * dt)), 1.0 / (1.0 - math.exp(-kon * dt))
    p = e_on / (e_on + e_off)
    sigma = math.sqrt(p * (1.0 - p) / M)
    print("active fraction %.5f, stationary %.5f, sigma %.2g" % (frac, p, sigma))
    assert abs(frac - p) < 5.0 * sigma
    act.close()


# ---- 4. the stepper ----------------------------------------------------------------------------------------------------------
def _chains(seed=5, side=5, beads=80):
    """side x side straight chains along x (spacing 1, beads of radius 0.3: no contacts) 1.2 apart, jittered"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(beads) * 1.0, np.arange(side) * 1.2, np.arange(side) * 1.2, indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3)) + rng.normal(size=(side * side * beads, 3)) * 0.03
    n = c.shape[0]
    first = (np.arange(side * side)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    pairs = np.stack([first, first + 1], axis=1).astype(np.int32)
    return c, pairs, np.arange(0, n, 2), rng.permutation(2 ** 20)[:n].astype(np.int64)


WALL = dict(shape="ellipsoid", radii=(41.0, 4.0, 3.5), k=10.0, center=(39.5, 2.4, 2.4),
            quat=tuple(_unit((0.9995, 0.0, 0.01, 0.02))))


def _nucleus_stepper(model="lcp", nucleus=True, periphery=WALL, kon=300.0, crosslinkers=True):
    from mundy_amd import pipeline
    c, pairs, left, keys = _chains()
    n = c.shape[0]
    kw = dict(dt=1e-3, viscosity=1.0, search_buffer=0.4, contact_model=model, springs=(pairs, "hookean", 3.0, 1.0),
              brownian_kt=0.1)
    if crosslinkers:
        kw["crosslinkers"] = dict(left=left, sites=np.ones(n, np.uint8), kind="hookean", k=3.0, r=1.0, bind_rate=300.0,
                                  unbind_rate=150.0, kt=0.1, capture_radius=1.5, skin=0.3, keys=keys[:left.shape[0]])
    if nucleus:
        idx = np.arange(0, pairs.shape[0], 3)
        kw["periphery"] = periphery
        kw["active_forces"] = dict(springs=idx, sigma=2.0, kon=kon, koff=200.0, keys=keys[:idx.shape[0]] + 7)
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.3)), **kw)


def _final(st):
    order = np.argsort(host(st.ids))
    s, nt, el, ct = (host(t) for t in st.active_state())
    return host(st.center)[order], s, nt, el, ct


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_stepper_trajectory_is_invariant_under_reorder_and_restore(model):
    steps = 20
    a = _nucleus_stepper(model)
    assert a.center.shape[0] == 2000
    on = off = hits = 0
    for _ in range(steps):
        s = a.step()
        on, off, hits = on + s.active_switches[0], off + s.active_switches[1], hits + s.periphery_colliding
        # (no contact is active: the trajectories below do not hang on the sum order of a solve)
        assert float(a.contacts["sep"].min()) > 0.0
    fa = _final(a)
    assert on > 100 and off > 20 and hits > 20 * steps and s.max_periphery_overlap > 0 and s.crosslinker_bound > 0
    assert s.active_springs == int(fa[1].sum()) == on - off
    b = _nucleus_stepper(model)
    for _ in range(steps // 2):
        b.step()
    perm = b.reorder_bodies(curve="morton", cell_size=2.0)
    assert (host(perm) != np.arange(perm.shape[0])).any()
    for _ in range(steps - steps // 2):
        sb = b.step()
    fb = _final(b)
    assert_bits_equal(fb[0], fa[0], "centres after reorder_bodies")
    assert (fb[1] == fa[1]).all() and (fb[4] == fa[4]).all()
    assert_bits_equal(fb[2], fa[2], "next_time after reorder_bodies")
    assert_bits_equal(fb[3], fa[3], "elapsed after reorder_bodies")
    assert (sb.active_springs, sb.periphery_colliding, sb.max_periphery_overlap) == \
        (s.active_springs, s.periphery_colliding, s.max_periphery_overlap)
    c = _nucleus_stepper(model)
    for _ in range(8):
        c.step()
    snap = c.snapshot()
    for _ in range(5):
        c.step()
    c.scale_periphery(0.97)
    c.step()
    c.restore(snap)
    for _ in range(steps - 8):
        sc = c.step()
    fc = _final(c)
    assert_bits_equal(fc[0], fa[0], "centres after restore")
    assert (fc[1] == fa[1]).all() and (fc[4] == fa[4]).all()
    assert_bits_equal(fc[2], fa[2], "next_time after restore")
    assert sc.active_springs == s.active_springs and sc.max_periphery_overlap == s.max_periphery_overlap


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_idle_nucleus_is_the_stepper_without_the_keywords(model):
    plain = _nucleus_stepper(model, nucleus=False)
    far = dict(shape="sphere", radius=1e3, k=10.0)
    idle = _nucleus_stepper(model, periphery=far, kon=1e-300)   # first switching time ~ 1e300: never
    assert plain.periphery is None and plain.active is None and plain._chain_stats.shape[0] == 6
    for _ in range(5):
        sp = plain.step()
        si = idle.step()
        assert_bits_equal(host(idle.center), host(plain.center), "idle nucleus")
        assert (si.periphery_colliding, si.max_periphery_overlap, si.active_springs, si.active_switches) == (0, 0.0, 0,
                                                                                                            (0, 0))
        assert si.crosslinker_bound == sp.crosslinker_bound and si.max_spring_length == sp.max_spring_length
    assert (host(idle.active_state()[3]) == 1).all()   # the draw of create, nothing since


def test_step_force_is_the_models_sum_in_the_reference_order(oracle):
    st = _nucleus_stepper(crosslinkers=False)
    c0, pairs, _, _ = _chains()
    n = c0.shape[0]
    x0 = c0.copy()
    idx = np.arange(0, pairs.shape[0], 3)
    ext = np.random.default_rng(31).normal(size=(n, 3))
    for _ in range(3):
        st.step(external_force=dev(ext))
        state = host(st.active_state()[0])
        F, _, _ = cm.spring_force(n, pairs, "hookean", 3.0, 1.0, x0)
        F, col, mx = pm.ellipsoid_force(x0, np.full(n, 0.3), WALL["radii"], WALL["k"], WALL["center"], WALL["quat"],
                                        force=F, rotate=_rotate(oracle),
                                        distance=_oracle_distance(oracle, WALL["center"], WALL["quat"], WALL["radii"]))
        F, _ = pm.active_force(n, pairs[idx], state, 2.0, x0, force=F)
        assert_bits_equal(host(st.spring_force), F + ext, "springs, periphery, active dipoles, external force")
        x0 = host(st.center).copy()
    assert col > 0


# every valid choice of force terms: the active dipoles act on springs, so they need them (8 + 16 = 24 cases)
TERM_SUBSETS = [t for t in ((s, x, p, a, e) for s in (0, 1) for x in (0, 1) for p in (0, 1) for a in (0, 1)
                            for e in (0, 1)) if t[0] or not t[3]]
ROUND_WALL = dict(shape="sphere", radius=39.0, k=10.0, center=(39.5, 2.4, 2.4))   # the chains' end beads reach 39.5


@pytest.mark.parametrize("terms", TERM_SUBSETS, ids=lambda t: "".join(c for c, on in zip("SXPAE", t) if on) or "none")
def test_force_stage_is_the_models_sum_for_every_choice_of_terms(terms):
    """springs, crosslinker springs, periphery, active dipoles, external force: whichever of them are switched on, the
    stepper's force is the numpy models summed in the reference's order, bit for bit, over three steps, from the
    stepper's own crosslinker heads (after its KMC) and active states (after its sampling); every term that is on
    acts on some bead in at least one of the steps"""
    from mundy_amd import pipeline
    has_s, has_x, has_p, has_a, has_e = terms
    assert len(TERM_SUBSETS) == 24
    c0, pairs, left, keys = _chains()
    n, radius = c0.shape[0], np.full(c0.shape[0], 0.3)
    idx = np.arange(0, pairs.shape[0], 3)
    kw = dict(dt=1e-3, viscosity=1.0, search_buffer=0.4)
    if has_s:
        kw["springs"] = (pairs, "hookean", 3.0, 1.0)
    if has_x:  # every fourth crosslinker doubly bound from the start, to the next bead of its chain (left is even)
        right = left.copy()
        right[::4] += 1
        kw["crosslinkers"] = dict(left=left, right=right, sites=np.ones(n, np.uint8), kind="hookean", k=3.0, r=1.0,
                                  bind_rate=300.0, unbind_rate=150.0, kt=0.1, capture_radius=1.5, skin=0.3,
                                  keys=keys[:left.shape[0]])
    if has_p:
        kw["periphery"] = ROUND_WALL
    if has_a:
        kw["active_forces"] = dict(springs=idx, sigma=2.0, kon=300.0, koff=200.0, keys=keys[:idx.shape[0]] + 7)
    if not (has_s or has_x or has_p):
        kw["brownian_kt"] = 0.0   # no noise: the keyword switches the chain step on
    st = pipeline.ContactStepper("sphere", dev(c0), dev(radius), **kw)
    ext = np.random.default_rng(31).normal(size=(n, 3)) if has_e else None
    x0 = c0.copy()
    acted = dict(x=0, p=0, a=0)
    for _ in range(3):
        s = st.step(external_force=None if ext is None else dev(ext))
        F = None
        if has_s:
            F = cm.spring_force(n, pairs, "hookean", 3.0, 1.0, x0)[0]
        if has_x:
            le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
            X = xm.crosslinker_force(n, le, ri, "hookean", 3.0, 1.0, x0)[0]
            F = X if F is None else F + X
            acted["x"] += int((ri != le).sum() > 0 and np.abs(X).max() > 0.0)
            assert s.crosslinker_bound == int((ri != le).sum())
        if has_p:
            F, col, mx = pm.sphere_force(x0, radius, ROUND_WALL["radius"], ROUND_WALL["k"], ROUND_WALL["center"], force=F)
            acted["p"] += int(col > 0)
            assert (s.periphery_colliding, s.max_periphery_overlap) == (col, mx)
        if has_a:
            state = host(st.active_state()[0])
            F, count = pm.active_force(n, pairs[idx], state, 2.0, x0, force=F)
            acted["a"] += int(count > 0)
            assert s.active_springs == count
        if F is not None:
            assert_bits_equal(host(st.spring_force), F if ext is None else F + ext, "the force stage's sum")
        elif has_e:   # the caller's force goes to the drag as it is
            assert_bits_equal(host(st.u_ext), cm.drag_velocity(host(st.mob_trans), ext), "U_ext of the external force")
            assert not host(st.spring_force).any()
        else:
            assert not host(st.u_ext).any() and not host(st.spring_force).any()
        x0 = host(st.center).copy()
    # a bound crosslinker under tension, a bead at the wall, an active spring: in some step, for every term that is on
    assert all(acted[k] > 0 for k, on in (("x", has_x), ("p", has_p), ("a", has_a)) if on), acted


# ---- 5. the C++ driver ----------------------------------------------------------------------------------------------------
def test_nucleus_step_app_matches_python():
    from cpp_apps import build_app, checksums, fnv1a as fnv
    from mundy_amd import capi, pipeline, synth
    d = synth.chains(2, 1000, seed=8)
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    lo, hi = d["center"].min(axis=0), d["center"].max(axis=0)
    pc = [float(v) for v in 0.5 * (lo + hi)]
    radii = [float(v) for v in 0.7 * 0.5 * (hi - lo)]
    quat = [float(v) for v in _unit((0.9, 0.1, -0.3, 0.2))]
    idx = np.arange(0, d["pairs"].shape[0], 2)
    ap = dict(sigma=2.0, kon=150.0, koff=100.0)
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"], periphery=dict(shape="ellipsoid", radii=radii, k=5.0, center=pc,
                                                                     quat=quat),
                                 active_forces=dict(springs=idx, **ap))
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d colliding %d active %d on %d off %d" % (
            k, s.num_contacts, s.num_iters, s.periphery_colliding, s.active_springs, s.active_switches[0],
            s.active_switches[1]))
    assert s.periphery_colliding > 0 and s.active_springs > 0
    import tempfile
    exe = build_app("nucleus_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0], idx.shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            d["pairs"][idx].astype(np.int32).tofile(f)
        args = [d["dt"], d["skin"], d["k"], d["r0"], d["kt"]]
        tail = radii + [5.0] + pc + quat + [ap["sigma"], ap["kon"], ap["koff"]]
        out = subprocess.run([exe, path, "20"] + [repr(float(a)) for a in args] + [str(capi.PERIPHERY_ELLIPSOID)] +
                             [repr(float(a)) for a in tail], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:14]) for g in got] == lines
    cs = checksums(out.stdout)
    state, next_time = (host(t) for t in st.active_state()[:2])
    assert cs["center"] == fnv(host(st.center).reshape(-1).view(np.uint64).tolist())
    assert cs["state"] == fnv(state.astype(np.int64).tolist())
    assert cs["next_time"] == fnv(next_time.view(np.uint64).tolist())


# ---- 6. full size ------------------------------------------------------------------------------------------------------------
def test_one_step_at_full_size():
    from mundy_amd import pipeline, synth
    d = synth.chains(1000, 1000, seed=3)
    n = d["center"].shape[0]
    lo, hi = d["center"].min(axis=0), d["center"].max(axis=0)
    half = 0.5 * (hi - lo)
    idx = np.arange(0, d["pairs"].shape[0], 2)
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"],
                                 periphery=dict(shape="ellipsoid", radii=[float(v) for v in 1.2 * half], k=1.0,
                                                center=[float(v) for v in 0.5 * (lo + hi)],
                                                quat=[float(v) for v in _unit((0.9, 0.1, -0.3, 0.2))]),
                                 active_forces=dict(springs=idx, sigma=1.0, kon=1e3, koff=1e3))
    assert n == 10 ** 6
    t0 = host(st.active_state()[1])
    st.active.advance(1e-3)              # as if a step had passed: the springs drawn T <= 1e-3 switch on now
    s = st.step()
    assert s.num_bodies == n and s.converged
    assert 0 < s.periphery_colliding < n // 2 and s.max_periphery_overlap > 0 and math.isfinite(s.max_periphery_overlap)
    assert s.active_switches == (int((t0 <= 1e-3).sum()), 0) and s.active_springs == s.active_switches[0] > 10 ** 5
    assert not bool(torch.isnan(st.center).any()) and not bool(torch.isnan(st.spring_force).any())
    el = host(st.active_state()[2])
    assert ((el == 1e-3) | (el == 2e-3)).all()
