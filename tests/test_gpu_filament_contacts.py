"""The colliding filaments' contact stage on the device (filament_contact.hip) against the numpy model
(filament_contact_model.py), bit for bit: the segment view, the pair list, the linker pass with both statistics, the
reduction to the nodes, rebuild and carry, the stepper over 50 steps, and the overlap two pressed filaments come to rest
at."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import filament_contact_model as fcm
import filament_model as fm
import friction_hertz_model as fh
from gpu_util import PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host
from test_gpu_filaments import BORDER_COUNTS, COMPARED, STATE, device_kwargs, make_case, new_device, new_model, params

pytestmark = pytest.mark.gpu

MATERIAL = dict(youngs_modulus=200.0, poisson_ratio=0.3)
LINKER_FIELDS = ("sep", "tang_disp", "force", "share")


def new_contacts(case, prm, **kw):
    """(device filaments, device contacts, model filaments, model contacts) of one case"""
    from mundy_amd import ops
    d, m = new_device(case, prm), new_model(case, prm)
    return d, ops.FilamentContacts(d, **kw), m, fcm.Contacts(m, **kw)


def stats_of(t):
    h = host(t)
    return float(h[0]), int(h.view(np.int64)[1])


def assert_linkers(dc, mc, what):
    assert_bits_equal(host(dc.field("sep")), mc.sep, what + ": sep")
    for name in ("tang_disp", "force", "share"):
        assert_bits_equal(host(dc.field(name)), getattr(mc, name), "%s: %s" % (what, name))


def force_both(dc, mc, dt, ext=None, what=""):
    got = stats_of(dc.force(dt, None if ext is None else dev(ext)))
    want = mc.force_pass(dt, ext)
    assert_linkers(dc, mc, what)
    assert_bits_equal(host(dc.field("node_force")), mc.node_force, what + ": node_force")
    assert_bits_equal(np.array([got[0]]), np.array([want[0]]), what + ": max_overlap")
    assert got[1] == want[1], (what, got, want)
    return want


# ---- 1. the segment view ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("monolayer", [False, True])
def test_segment_view_and_saved_velocity(oracle, monolayer):
    case = make_case(31, BORDER_COUNTS)
    d, dc, m, mc = new_contacts(case, params(monolayer=monolayer), skin=0.25, mu=0.5, **MATERIAL)
    d.force(0.25)
    d.velocity()
    m.compute_force(0.25)
    m.compute_velocity()
    assert np.abs(m.velocity[:, 0]).max() > 1e-4
    dc.save_velocity()
    mc.save_velocity()
    assert_bits_equal(host(dc.field("velocity_prev")), mc.velocity_prev, "velocity_prev")
    assert all_pos_zero(mc.velocity_prev[:, 0]) == monolayer
    assert dc.update() and mc.update()
    assert_bits_equal(host(dc.field("seg")), mc.seg, "seg")
    assert_bits_equal(host(dc.field("aabb")), mc.aabb, "aabb")
    last = case["node_ptr"][1:] - 1
    assert np.array_equal(mc.seg[last, 0:3], mc.seg[last, 3:6]) and np.isfinite(mc.aabb).all()
    assert np.array_equal(host(dc.field("pairs")), mc.pairs)
    dc.close()
    d.close()


# ---- 2. the pair list ---------------------------------------------------------------------------------------------------
def straight_case(d):
    return dict(d, n=len(d["radius"]), phase=np.zeros(len(d["node_ptr"]) - 1) if d["phase"] is None else d["phase"])


def coil(nodes=60, turns=3.0, coil_radius=2.0, rise=0.9):
    """one filament wound into a helix whose turns lie 0.9 apart: it touches itself"""
    a = np.linspace(0.0, 2.0 * math.pi * turns, nodes)
    c = np.stack([coil_radius * np.cos(a), coil_radius * np.sin(a), rise * a / (2.0 * math.pi)], axis=1)
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (nodes, 1))
    return dict(node_ptr=np.array([0, nodes], dtype=np.int32), center=c, twist=np.zeros(nodes), radius=np.full(nodes, 0.5),
                rest_curvature=np.zeros((nodes, 3)), arclength=np.arange(nodes) * 1.0, edge_orientation=quat,
                phase=np.zeros(1), n=nodes)


@pytest.mark.parametrize("which", ["crossed", "coil", "two_nodes"])
def test_pair_list_equals_the_brute_force_list(oracle, which):
    from mundy_amd import synth
    case = {"crossed": lambda: straight_case(synth.crossed_filaments(6, 9, angle=1.0)), "coil": coil,
            "two_nodes": lambda: straight_case(synth.crossed_filaments(8, 2, pitch=1.5))}[which]()
    for bonded in (1, 3):
        d, dc, m, mc = new_contacts(case, params(), skin=0.5, mu=0.5, bonded_exclusion=bonded, **MATERIAL)
        assert dc.update() and mc.update()
        got = host(dc.field("pairs"))
        assert np.array_equal(got, mc.pairs) and dc.num_pairs == len(mc.pairs) > 0
        assert not np.isin(got, case["node_ptr"][1:] - 1).any()
        if which == "coil":   # the filament's own turns, never its neighbours along the centreline
            assert (np.diff(got, axis=1) > bonded).all() and len(got) > 20
        dc.close()
        d.close()


# ---- 3. the linker pass -------------------------------------------------------------------------------------------------
def grid_patches(count):
    """(a, b) patches with sum a b == count: in a patch, a segments along z cross b segments along y"""
    out = []
    while count > 0:
        a = max(1, int(math.isqrt(count)))
        b = count // a
        out.append((a, b))
        count -= a * b
    return out


def crossing_grid(count, rng, shift=None, base=None):
    """2-node filaments in patches (grid_patches): every segment along z of a patch lies under every segment along y of
    it, so the list has exactly `count` linkers; radii in [0.4, 0.6], the layers' distance per filament such that about
    half of the crossings touch (base=None) or none does (base = the distance); shift [filament] moves a filament
    towards the other layer.  -> case"""
    pitch, skin = 2.0, 0.25   # parallel neighbours: 2.0 > 2 * 0.6 + 2 * skin
    centers, y0 = [], 0.0
    for a, b in grid_patches(count):
        la, lb = (a - 1) * pitch + 2.0, (b - 1) * pitch + 2.0   # the lengths span the other layer
        xa = rng.uniform(0.0, 0.15, a) if base is None else np.zeros(a)
        xb = rng.uniform(0.7, 1.15, b) if base is None else np.full(b, base)
        for j in range(a):     # along z, at y = y0 + j pitch
            centers += [[xa[j], y0 + j * pitch, -1.0], [xa[j], y0 + j * pitch, lb - 1.0]]
        for k in range(b):     # along y, at z = k pitch
            centers += [[xb[k], y0 - 1.0, k * pitch], [xb[k], y0 + la - 1.0, k * pitch]]
        y0 += la + 4.0
    c = np.array(centers)
    n = len(c)
    if shift is not None:
        c[:, 0] += np.repeat(shift, 2)
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))   # (the filaments' own forces are never evaluated on these cases)
    radius = np.repeat(rng.uniform(0.4, 0.6, n // 2) if base is None else np.full(n // 2, 0.5), 2)
    return dict(node_ptr=(np.arange(n // 2 + 1) * 2).astype(np.int32), center=c, twist=np.zeros(n), radius=radius,
                rest_curvature=np.zeros((n, 3)), arclength=np.tile([0.0, 1.0], n // 2), edge_orientation=quat,
                phase=np.zeros(n // 2), n=n, skin=skin)


def plant(dc, mc, rng, velocity=True, history=True):
    n, c = mc.n, len(mc.pairs)
    if velocity:
        v = rng.normal(size=(n, 3))
        dc.set_field("velocity_prev", dev(v))
        mc.velocity_prev = v
    if history:
        td = rng.normal(scale=2e-3, size=(c, 3))
        dc.set_history(dev(mc.pairs), dev(td))   # the list itself: the carry is the identity
        mc.tang_disp = td.copy()
        assert_bits_equal(host(dc.field("tang_disp")), mc.tang_disp, "planted history")


@pytest.mark.parametrize("count", [1, 255, 256, 257, PAST_FULL_GRID])
def test_linker_pass_matches_the_model(oracle, count):
    rng = np.random.default_rng(40 + count % 7)
    case = crossing_grid(count, rng)
    d, dc, m, mc = new_contacts(case, params(), skin=case["skin"], mu=0.35, damping=(0.4, 0.2), density=1.5, **MATERIAL)
    dc.save_velocity()
    assert dc.update() and mc.update()
    assert len(mc.pairs) == count and np.array_equal(host(dc.field("pairs")), mc.pairs)
    plant(dc, mc, rng)
    ext = rng.normal(size=(case["n"], 3))
    overlap, sliding = force_both(dc, mc, 0.01, ext, "first call")
    touching = int((mc.sep <= 0.0).sum())
    if count >= 255:   # both branches of the Coulomb cap, and separated pairs
        assert 0 < sliding < touching < count and overlap > 0.0
    apart = np.flatnonzero(mc.sep > 0.0)
    for name in ("tang_disp", "force", "share"):
        assert all_pos_zero(getattr(mc, name)[apart])
    if apart.size:
        # a separated pair's rows are written only where they are not +0.0: a planted -0.0 is replaced ...
        f = host(dc.field("force"))
        f[apart[0]] = -0.0
        dc.set_field("force", dev(f))
        assert not all_pos_zero(host(dc.field("force"))[apart[0]])
    force_both(dc, mc, 0.01, None, "second call")   # ... and without one the second call gives the model's rows
    assert all_pos_zero(host(dc.field("force"))[apart])
    dc.close()
    d.close()


def test_capped_contact_without_history_has_no_tangential_force(oracle):
    rng = np.random.default_rng(47)
    case = crossing_grid(256, rng)
    # history_dt = 0 keeps the history at zero; mu = 0 caps every contact: F_t = 0, the force lies along the normal
    d, dc, m, mc = new_contacts(case, params(), skin=case["skin"], mu=0.0, damping=(0.4, 0.2), history_dt=0.0, **MATERIAL)
    dc.save_velocity()
    assert dc.update() and mc.update()
    plant(dc, mc, rng, history=False)
    overlap, sliding = force_both(dc, mc, 0.01, None, "capped")
    hit = mc.sep <= 0.0
    assert sliding == hit.sum() > 20 and all_pos_zero(mc.tang_disp)
    i, j = mc.pairs[hit, 0], mc.pairs[hit, 1]
    _, cp1, cp2, _, _, _ = oracle.distance_segment_segment(mc.seg[i, 0:3], mc.seg[i, 3:6], mc.seg[j, 0:3], mc.seg[j, 3:6])
    nrm = cp2 - cp1
    assert np.abs(np.cross(mc.force[hit], nrm)).max() <= 1e-12 * np.abs(mc.force[hit]).max()
    dc.close()
    d.close()


def test_statistics_at_every_position(oracle):
    # the full-grid list with the layers 1.4 apart (radii 0.5): nothing touches until the two filaments of the linker
    # at `pos` are moved 0.25 towards each other: that pair alone is 0.9 apart
    rng = np.random.default_rng(48)
    settings = dict(mu=0.0, damping=(0.0, 0.3), **MATERIAL)
    case = crossing_grid(PAST_FULL_GRID, rng, base=1.4)
    nfil = len(case["node_ptr"]) - 1
    d, dc, m, mc = new_contacts(case, params(), skin=case["skin"], **settings)
    dc.save_velocity()
    assert dc.update() and mc.update()
    pairs = mc.pairs   # the list once, from the model; it does not depend on the shifts below
    assert len(pairs) == PAST_FULL_GRID and np.array_equal(host(dc.field("pairs")), pairs)
    assert stats_of(dc.force(0.01)) == (0.0, 0) and all_pos_zero(host(dc.field("node_force")))
    dc.close()
    d.close()
    for pos in STAT_POSITIONS:
        shift = np.zeros(nfil)
        shift[pairs[pos, 0] // 2], shift[pairs[pos, 1] // 2] = 0.25, -0.25
        case = crossing_grid(PAST_FULL_GRID, rng, shift=shift, base=1.4)
        from mundy_amd import ops
        d = new_device(case, params())
        dc = ops.FilamentContacts(d, skin=case["skin"], **settings)
        dc.save_velocity()
        assert dc.update() and dc.num_pairs == PAST_FULL_GRID
        v = np.zeros((case["n"], 3))
        v[pairs[pos, 0], 1] = 1.0   # a tangential velocity: the one contact is capped (mu = 0)
        dc.set_field("velocity_prev", dev(v))
        overlap, sliding = stats_of(dc.force(0.01))
        sep = host(dc.field("sep"))
        assert sliding == 1 and overlap == -sep[pos] and abs(overlap - 0.1) < 1e-12, pos
        assert (np.delete(sep, pos) > 0.0).all()
        dc.close()
        d.close()


# ---- 4. the reduction ---------------------------------------------------------------------------------------------------
def comb(order=None):
    """long straight filaments of BORDER_COUNTS nodes along z, side by side, each crossed over its first and its last
    segment by a short 2-node filament along y; then one long segment crossed by 100 short ones, and 20 isolated
    2-node filaments.  order: a permutation of the filaments (the same case laid out differently)."""
    fil = []
    for f, count in enumerate(BORDER_COUNTS):   # first, so that they end on, one before and one after a tile border
        fil.append(np.stack([np.zeros(count), np.full(count, 4.0 * f), np.arange(count) * 1.0], axis=1))
    for f, count in enumerate(BORDER_COUNTS):
        for zc in sorted({0.5, count - 1.5}):
            fil.append(np.array([[0.9, 4.0 * f - 1.0, zc], [0.9, 4.0 * f + 1.0, zc]]))
    y = 4.0 * len(BORDER_COUNTS) + 4.0
    fil.append(np.array([[0.0, y, -2.0], [0.0, y, 162.0]]))                       # the hub
    for s in range(100):
        fil.append(np.array([[0.85 + 0.001 * s, y - 1.0, 1.6 * s], [0.85 + 0.001 * s, y + 1.0, 1.6 * s]]))
    for s in range(20):
        fil.append(np.array([[10.0, 3.0 * s, -5.0], [10.0, 3.0 * s, -4.0]]))
    order = np.arange(len(fil)) if order is None else order
    fil = [fil[k] for k in order]
    counts = np.array([len(x) for x in fil])
    c = np.concatenate(fil)
    n = len(c)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(node_ptr=ptr, center=c, twist=np.zeros(n), radius=np.full(n, 0.5), rest_curvature=np.zeros((n, 3)),
                arclength=np.zeros(n), edge_orientation=np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)),
                phase=np.zeros(len(fil)), n=n)


@pytest.mark.parametrize("layout", ["as_built", "shuffled"])
def test_reduction_across_tile_borders_and_a_long_row(oracle, layout):
    rng = np.random.default_rng(50)
    nfil = len(comb()["node_ptr"]) - 1
    case = comb(None if layout == "as_built" else rng.permutation(nfil))
    if layout == "as_built":
        assert case["node_ptr"][1:4].tolist() == [256, 511, 513]
    d, dc, m, mc = new_contacts(case, params(), skin=0.25, mu=0.4, damping=(0.2, 0.1), **MATERIAL)
    dc.save_velocity()
    assert dc.update() and mc.update()
    assert np.array_equal(host(dc.field("pairs")), mc.pairs)
    plant(dc, mc, rng)
    ext = rng.normal(size=(case["n"], 3))
    force_both(dc, mc, 0.01, ext, "with an external force")
    force_both(dc, mc, 0.01, None, "without")
    rows = np.bincount(mc.pairs.reshape(-1), minlength=case["n"])
    assert rows.max() >= 100 and (rows == 0).sum() > 20
    touched = np.flatnonzero(np.abs(mc.node_force).max(axis=1) > 0.0)
    ptr = case["node_ptr"]
    long_ones = [f for f in range(nfil) if ptr[f + 1] - ptr[f] in BORDER_COUNTS and ptr[f + 1] - ptr[f] > 2]
    for f in long_ones:   # first and last segment of every long filament carry a contact
        assert ptr[f] in touched and ptr[f + 1] - 1 in touched
    # NULL and an array of +0.0: the same bits
    force_both(dc, mc, 0.01, np.zeros((case["n"], 3)), "zero external force")
    dc.close()
    d.close()


# ---- 5. rebuild and carry, 6. the stepper ---------------------------------------------------------------------------------
WAVE_CASE = dict(eta=0.04, skin=0.06, mu=0.6, dt=0.01, overlap=0.02)


def stepper_case(monolayer):
    from mundy_amd import synth
    ov = WAVE_CASE["overlap"]
    if monolayer:   # everything in the plane x = 0: layer 1 lies across, beyond the tips of layer 0
        d = synth.crossed_filaments(3, 6, overlap=ov, seed=7, pitch=2.5, offset=(0.0, 0.0, 5.0 + 1.0 - ov))
    else:
        d = synth.crossed_filaments(3, 6, overlap=ov, seed=7, angle=1.2)
    return straight_case(d)


def new_steppers(case, prm, contacts):
    from mundy_amd import pipeline
    st = pipeline.FilamentStepper(case["node_ptr"], case["center"], case["radius"], case["edge_orientation"],
                                  case["arclength"], twist=case["twist"], rest_curvature=case["rest_curvature"],
                                  phase=case["phase"], contacts=contacts, **device_kwargs(prm))
    m = new_model(case, prm)
    return st, m, (None if contacts is None else fcm.Contacts(m, **contacts))


def step_both(st, m, mc, dt, k, ext=None):
    """one step of the stepper and of the model, everything compared -> (contact statistics, rebuilt, contacts touching)"""
    got = st.step(dt, None if ext is None else dev(ext))
    fstats, cstats, rebuilt = fcm.step(mc, dt, k * dt, ext)
    what = "step %d" % k
    assert got.rebuilt == rebuilt and got.num_pairs == len(mc.pairs), what
    assert_bits_equal(np.array([got.max_stretch, got.max_curvature_deviation, got.max_overlap]),
                      np.array([fstats[0], fstats[1], cstats[0]]), what)
    assert got.num_sliding == cstats[1], what
    assert np.array_equal(host(st.contacts.field("pairs")), mc.pairs), what
    assert_bits_equal(host(st.contacts.field("tang_disp")), mc.tang_disp, what + ": tang_disp")
    assert_bits_equal(host(st.contacts.field("node_force")), mc.node_force, what + ": node_force")
    return cstats, rebuilt, int((mc.sep <= 0.0).sum())


@pytest.mark.parametrize("monolayer", [False, True])
def test_fifty_steps_with_contacts_match_the_model(oracle, monolayer):
    case = stepper_case(monolayer)
    base = params(wave=True, disable_twist=monolayer, monolayer=monolayer)
    prm = fm.Params(**dict(base.__dict__, eta=WAVE_CASE["eta"]))
    contacts = dict(skin=WAVE_CASE["skin"], mu=WAVE_CASE["mu"], damping=(0.1, 0.05), **MATERIAL)
    st, m, mc = new_steppers(case, prm, contacts)
    rebuilds = sliding = sticking = 0
    for k in range(50):
        cstats, rebuilt, touching = step_both(st, m, mc, WAVE_CASE["dt"], k)
        rebuilds += int(rebuilt and k > 0)
        sliding += cstats[1]
        sticking += (touching - cstats[1]) if k > 0 else 0
    for name in STATE:
        assert_bits_equal(host(st.field(name)), getattr(m, name), "after 50 steps: " + name)
    # the case was chosen on the CPU so that the model alone shows all three: it cannot pass on an empty list
    assert rebuilds >= 1 and sliding >= 1 and sticking >= 1, (rebuilds, sliding, sticking)
    assert np.isfinite(m.center).all()
    if monolayer:
        assert all_pos_zero(m.center[:, 0])
    st.close()


def test_without_contacts_the_stepper_is_the_parents(oracle):
    case = stepper_case(False)
    prm = fm.Params(**dict(params(wave=True).__dict__, eta=WAVE_CASE["eta"]))
    st, m, _ = new_steppers(case, prm, None)
    assert st.contacts is None
    for k in range(50):
        got = st.step(WAVE_CASE["dt"])
        want = m.step(WAVE_CASE["dt"], k * WAVE_CASE["dt"])
        assert_bits_equal(np.array([got.max_stretch, got.max_curvature_deviation]), np.array(want), "step %d" % k)
        assert got.num_pairs == 0 and got.max_overlap == 0.0 and not got.rebuilt
    for name in STATE:
        assert_bits_equal(host(st.field(name)), getattr(m, name), name)
    st.close()


def two_crossed(gap):
    """two 2-node filaments of length 2 and radius 0.5 crossing at their midpoints, the centrelines `gap` apart along x"""
    c = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [gap, -1.0, 0.0], [gap, 1.0, 0.0]])
    q = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1))
    q[2] = fm.triad_orientation([0.0, 1.0, 0.0])
    return dict(node_ptr=np.array([0, 2, 4], dtype=np.int32), center=c, twist=np.zeros(4), radius=np.full(4, 0.5),
                rest_curvature=np.zeros((4, 3)), arclength=np.array([0.0, 2.0, 0.0, 2.0]), edge_orientation=q,
                phase=np.zeros(2), n=4)


def test_no_rebuild_until_a_node_moves_past_half_the_skin(oracle):
    # the crossed layers at rest but for their contacts: small steps, no rebuild; then one node is pushed so hard that
    # it moves past skin / 2 in a single step, and the list is rebuilt at the model's step with the histories carried
    case = stepper_case(False)
    prm = fm.Params(**dict(params().__dict__, eta=1.0))
    contacts = dict(skin=0.5, mu=0.6, **MATERIAL)
    st, m, mc = new_steppers(case, prm, contacts)
    push = np.zeros((case["n"], 3))
    push[5, 2] = 0.3 / (1e-3 * (1.0 / (6.0 * math.pi * 1.0 * 0.5)))   # dt v = 0.3 > skin / 2
    flags = []
    for k in range(12):
        _, rebuilt, touching = step_both(st, m, mc, 1e-3, k, push if k == 8 else None)
        flags.append(rebuilt)
        if k == 9:
            before = (mc.pairs.copy(), mc.tang_disp.copy())
    # the push of step 8 becomes a velocity at its end and a displacement in step 9
    assert flags == [True] + [False] * 8 + [True, False, False] and touching > 0
    assert np.abs(before[1]).max() > 0.0   # rows that the rebuild of step 9 carried over
    st.close()


def test_a_pair_that_leaves_the_list_starts_again_from_zero(oracle):
    case = two_crossed(0.98)
    prm = fm.Params(E=10.0, nu=0.3, l0=2.0, eta=1.0)
    contacts = dict(skin=0.125, mu=0.5, youngs_modulus=1000.0, poisson_ratio=0.3)
    st, m, mc = new_steppers(case, prm, contacts)
    per_step = 1.0 / (0.01 * (1.0 / (6.0 * math.pi * 0.5)))   # the force that moves a node by 1 in one step
    slide, away = np.zeros((4, 3)), np.zeros((4, 3))
    slide[2:, 2] = 0.1 * per_step    # the top filament slides along the bottom one: a history builds up
    away[2:, 0] = 0.5 * per_step     # it moves 0.5 a step along the normal: beyond the boxes after one step
    plan = {0: slide, 1: slide, 2: away, 3: away, 4: -away, 5: -away}   # a force acts on the positions one step later
    sizes, history, carried = [], [], []
    f, c = st.filaments, st.contacts
    for k in range(8):   # the stepper's sequence by hand, to look at the history between the carry and the force
        ext = plan.get(k)
        c.save_velocity()
        mc.save_velocity()
        f.advance(0.01)
        m.advance(0.01)
        assert c.update() == mc.update(), k
        assert np.array_equal(host(c.field("pairs")), mc.pairs), k
        assert_bits_equal(host(c.field("tang_disp")), mc.tang_disp, "step %d: carried history" % k)
        carried.append(all_pos_zero(mc.tang_disp))
        force_both(c, mc, 0.01, ext, "step %d" % k)
        f.force(k * 0.01, c.node_force_ptr())
        m.compute_force(k * 0.01, mc.node_force)
        f.velocity()
        m.compute_velocity()
        sizes.append(len(mc.pairs))
        history.append(float(np.abs(mc.tang_disp).max()) if len(mc.pairs) else -1.0)
    assert_bits_equal(host(f.field("center")), m.center, "center")
    # in the list while it slides, gone beyond the boxes, back again: the history the pair had is not carried
    assert sizes == [1, 1, 1, 0, 0, 0, 1, 1], sizes
    assert min(history[1:3]) > 1e-4 and not carried[2] and carried[6] and not carried[7], (history, carried)
    st.close()


# ---- 7. two filaments pressed together come to rest where the Hertz force carries the load ------------------------------
def test_pressed_filaments_rest_at_the_hertz_overlap():
    from mundy_amd import pipeline
    case = two_crossed(0.99)
    E, nu, load = 1000.0, 0.3, 1.0
    st = pipeline.FilamentStepper(case["node_ptr"], case["center"], case["radius"], case["edge_orientation"],
                                  case["arclength"], youngs_modulus=10.0, poisson_ratio=0.3, rest_length=2.0,
                                  viscosity=1.0, contacts=dict(skin=0.5, youngs_modulus=E, poisson_ratio=nu, mu=0.5))
    ext = np.zeros((4, 3))
    ext[:2, 0], ext[2:, 0] = 0.5 * load, -0.5 * load
    ext = dev(ext)
    for _ in range(150):
        st.step(0.05, ext, read_stats=False)
    got = st.step(0.05, ext)
    kn, _ = fh.spring_coefficients(E, E, nu, nu)
    delta = (load / (kn * math.sqrt(0.25))) ** (2.0 / 3.0)   # load = sqrt(R* delta) k_n delta, R* = 1/4
    print("overlap", got.max_overlap, "deviation", got.max_overlap - delta, "velocity", float(st.field("velocity").abs().max()))
    # the model reaches 2.4e-17 on the CPU after 150 steps; the bound is the arc test's of 5j
    assert abs(got.max_overlap - delta) < 1e-12 and got.num_pairs == 1 and got.num_sliding == 0
    assert float(st.field("velocity").abs().max()) < 1e-12
    st.close()


# ---- 8. the C++ driver ----------------------------------------------------------------------------------------------------
def test_filament_contact_app_matches_python():
    from cpp_apps import build_app, checksums, fnv1a as fnv
    case = stepper_case(False)
    prm = fm.Params(**dict(params(wave=True).__dict__, eta=WAVE_CASE["eta"]))
    contacts = dict(skin=WAVE_CASE["skin"], mu=WAVE_CASE["mu"], damping=(0.1, 0.05), **MATERIAL)
    st, _, _ = new_steppers(case, prm, contacts)
    dt, steps = WAVE_CASE["dt"], 20
    lines = [st.step(dt) for _ in range(steps)]
    assert sum(s.num_sliding for s in lines) > 0 and sum(s.rebuilt for s in lines) >= 2
    exe = build_app("filament_contact_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([len(case["node_ptr"]) - 1, case["n"]], dtype=np.uint64).tofile(f)
            case["node_ptr"].astype(np.int32).tofile(f)
            for name in ("center", "twist", "edge_orientation", "radius", "rest_curvature", "arclength", "phase"):
                case[name].astype(np.float64).tofile(f)
        args = [dt, prm.E, prm.nu, prm.l0, prm.eta, prm.A, prm.k, prm.omega]
        cargs = [contacts["skin"], MATERIAL["youngs_modulus"], MATERIAL["poisson_ratio"], contacts["mu"], 0.1, 0.05, 1.0, -1.0]
        out = subprocess.run([exe, path, str(steps)] + [repr(float(a)) for a in args] + ["1", "0", "0"]
                             + [repr(float(a)) for a in cargs] + ["1"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert len(got) == steps
    for k, (w, s) in enumerate(zip(got, lines)):
        assert_bits_equal(np.array([float.fromhex(w[3]), float.fromhex(w[5]), float.fromhex(w[9])]),
                          np.array([s.max_stretch, s.max_curvature_deviation, s.max_overlap]), "step %d" % k)
        assert (int(w[7]), int(w[11]), int(w[13])) == (s.num_pairs, s.num_sliding, int(s.rebuilt)), k

    sums = checksums(out.stdout)
    for name in ("center", "twist", "velocity", "twist_velocity", "edge_orientation"):
        assert sums[name] == fnv(np.ascontiguousarray(host(st.field(name))).reshape(-1).view(np.uint64)), name
    for name in ("node_force", "tang_disp"):
        assert sums[name] == fnv(np.ascontiguousarray(host(st.contacts.field(name))).reshape(-1).view(np.uint64)), name
    st.close()
