"""The backbone segment contacts on the device (segment_contact.hip, ops.SegmentContacts) against the numpy model
(segment_contact_model.py), both laws, on the three cases of tests/test_segment_contact_host.py.
  A  the list and every row against the model
  B  the reduction order: the model's reduction of the device's own rows, bit for bit
  C  the forces do not depend on the age of the list
  D  the chain step with the term (tests/backbone_case.py) against the composed models; reorder, restore, crossed strands
  E  tests/cpp/backbone_collision_step_app.cpp against the Python stepper
Tolerances: WCA uses only + - * /, so everything is bit for bit.  The Hertz force goes through pow: 1e-14 |f| per linker,
the project's bar for that expression (tests/test_gpu_hertz.py); the share map is linear in F with norm <= 3 + 1, so the
Hertz shares get the same bound times 4."""
import numpy as np
import pytest
import torch

import segment_contact_model as scm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

gpu = pytest.mark.gpu
KINDS = ("hertz", "wca")


def O():
    from mundy_amd import ops
    return ops


def make(name, kind, end_correction=None, **kw):
    cs = scm.case(name)
    spec = dict(kind=kind, radius=scm.RADIUS, skin=scm.SKIN, segments=cs["ends"], end_correction=end_correction)
    spec.update(kw)
    return O().SegmentContacts(cs["n"], **spec), dev(cs["center"])


def stats_of(t):
    return O().SegmentContacts.read_stats(t)


# ---- A. list and rows ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", scm.CASES)
def test_list_and_rows_against_the_model(name, kind):
    mod = scm.evaluated(name, kind)
    sc, x = make(name, kind)
    with pytest.raises(RuntimeError, match="before mhip_segment_contacts_update"):
        sc.force(x)
    assert sc.update(x) and not sc.update(x) and sc.update(x, force_rebuild=True)
    pairs = host(sc.field("pairs"))
    assert pairs.shape == mod.pairs.shape and (pairs == mod.pairs).all()
    assert_bits_equal(host(sc.field("seg")), mod.seg, "seg")
    assert_bits_equal(host(sc.field("aabb")), mod.aabb, "aabb")
    f, stats = sc.force(x)
    assert_bits_equal(host(sc.field("sep")), mod.sep, "sep")
    force, share = host(sc.field("force")), host(sc.field("share"))
    out = ~mod.in_branch
    assert all_pos_zero(force[out]) and all_pos_zero(share[out]), "rows outside the force branch are not +0.0"
    if kind == "wca":
        assert_bits_equal(force, mod.force, "force")
        assert_bits_equal(share, mod.share, "share")
    else:
        fn = np.sqrt((mod.force * mod.force).sum(axis=1))
        err_f = np.abs(force - mod.force).max(axis=1)
        err_s = np.abs(share - mod.share).max(axis=(1, 2))
        print(name, "hertz: max |df| / |f| = %.3g, max |dshare| / |f| = %.3g" % (
            (err_f[mod.in_branch] / fn[mod.in_branch]).max(), (err_s[mod.in_branch] / fn[mod.in_branch]).max()))
        assert (err_f <= 1e-14 * fn).all() and (err_s <= 4e-14 * fn).all()
    mx, count = stats_of(stats)
    assert count == mod.stats[1] == int(mod.in_branch.sum())
    assert_bits_equal([mx], [mod.stats[0]], "max overlap")
    # the linker pass alone leaves out the end segments' overlaps; the reduction only raises the maximum
    lp = scm.SegmentContacts(mod.n, mod.ends, kind, scm.RADIUS, scm.SKIN)
    lp.update(host(x))
    lp.linker_pass()
    st = torch.full((2,), 77, dtype=torch.int64, device="cuda")
    mx1, count1 = stats_of(sc.linker_pass(st))
    assert count1 == count
    assert_bits_equal([mx1], [lp.stats[0]], "max overlap of the linker pass")
    sc.close()


# ---- B. the reduction ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("correction", [None, False], ids=["end_correction", "no_correction"])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", scm.CASES)
def test_reduction_order_is_the_models(name, kind, correction):
    """The model's reduction of the device's own force and share rows against the device's node forces, bit for bit.
    With the end correction in Hertz mode the model's own pow (numpy's) enters the comparison: the device evaluates that
    term's x^(3/2) with one rounding (pow_three_halves), which is what a host pow returns on these inputs."""
    mod = scm.SegmentContacts(scm.case(name)["n"], scm.case(name)["ends"], kind, scm.RADIUS, scm.SKIN,
                              end_correction=correction)
    sc, x = make(name, kind, end_correction=correction)
    mod.update(host(x))
    mod.segment_view(host(x))
    mod.linker_pass()
    sc.update(x)
    f, _ = sc.force(x)
    force, share = host(sc.field("force")), host(sc.field("share"))
    want = mod.reduce(force=force, share_rows=share)
    assert_bits_equal(host(f), want, "node force")
    old = np.random.default_rng(3).normal(size=want.shape)
    acc = dev(old)
    sc.force(x, out=acc, accumulate=True)
    assert_bits_equal(host(acc), mod.reduce(force=force, share_rows=share, external=old), "accumulated node force")
    again = sc.reduce()
    assert_bits_equal(host(again), want, "reduce() alone")
    total = np.abs(force).sum()
    assert np.isfinite(total) and total > 0.0
    # sum_b node_force < 1e-12 sum |F_c| (tests/test_gpu_hertz.py); with the end correction, whose two terms cancel
    # exactly, the bar is the same
    assert np.abs(host(f).sum(axis=0)).max() < 1e-12 * (total + np.abs(mod.end_terms()[0]).sum())
    sc.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_y_connectivity_and_bodies_on_no_segment(kind):
    # node 0 carries three segments; bodies 6 and 7 carry none; segments 3 and 4 cross all three arms
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [-0.5, 0.8, 0], [-0.5, -0.8, 0], [0.2, 0.1, 0.4], [0.9, 0.2, 0.5],
                  [5.0, 5, 5], [0.3, 0.3, 0.3], [-0.4, 0.2, 0.45], [-0.3, -0.6, 0.5]])
    ends = np.array([[0, 1], [0, 2], [0, 3], [4, 5], [8, 9]], dtype=np.int32)
    n = x.shape[0]
    mod = scm.SegmentContacts(n, ends, kind, 0.5, 0.3)
    mod.update(x)
    want, mstats = mod.force_pass(x)
    assert mod.pairs.tolist() == [[0, 3], [0, 4], [1, 3], [1, 4], [2, 3], [2, 4], [3, 4]] and mod.in_branch.sum() >= 4
    sc = O().SegmentContacts(n, kind=kind, radius=0.5, skin=0.3, segments=ends)
    xd = dev(x)
    assert sc.update(xd) and (host(sc.field("pairs")) == mod.pairs).all()
    f, stats = sc.force(xd)
    force, share = host(sc.field("force")), host(sc.field("share"))
    assert_bits_equal(host(f), mod.reduce(force=force, share_rows=share), "node force")
    np.testing.assert_allclose(host(f), want, rtol=1e-13, atol=1e-13 * np.abs(want).max())
    assert all_pos_zero(host(f)[[6, 7]])
    old = np.random.default_rng(4).normal(size=(n, 3))
    old[7] = -0.0   # an untouched row keeps even the sign of a zero
    acc = dev(old)
    sc.force(xd, out=acc, accumulate=True)
    assert_bits_equal(host(acc)[[6, 7]], old[[6, 7]], "rows of bodies on no segment")
    assert stats_of(stats)[1] == mstats[1]
    sc.close()


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_no_segments(kind):
    n = 300
    x = dev(np.random.default_rng(1).normal(size=(n, 3)))
    sc = O().SegmentContacts(n, kind=kind, radius=0.5, skin=0.3, segments=np.zeros((0, 2), np.int32))
    assert sc.update(x) and sc.num_pairs == 0
    f, stats = sc.force(x, out=dev(np.ones((n, 3))))
    assert all_pos_zero(host(f)) and stats_of(stats) == (0.0, 0)
    keep = dev(np.full((n, 3), -0.0))
    sc.force(x, out=keep, accumulate=True)
    assert_bits_equal(host(keep), np.full((n, 3), -0.0), "accumulate with no segments")
    sc.close()


@gpu
def test_per_segment_radii_reach_the_law():
    cs = scm.case("random_walks")
    r = np.random.default_rng(2).uniform(0.3, 0.6, cs["m"])
    mod = scm.SegmentContacts(cs["n"], cs["ends"], "wca", r, scm.SKIN)
    mod.update(cs["center"])
    want, mstats = mod.force_pass(cs["center"])
    sc, x = make("random_walks", "wca", radius=r)
    sc.update(x)
    f, stats = sc.force(x)
    assert_bits_equal(host(sc.field("force")), mod.force, "force")
    assert_bits_equal(host(f), want, "node force")
    assert stats_of(stats)[1] == mstats[1]
    sc.close()


# ---- C. the forces do not depend on the age of the list -----------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_forces_do_not_depend_on_the_age_of_the_list(kind):
    cs = scm.case("jittered_lattice")
    rng = np.random.default_rng(11)
    x = cs["center"].copy()
    mod = scm.SegmentContacts(cs["n"], cs["ends"], kind, scm.RADIUS, scm.SKIN)
    sc, _ = make("jittered_lattice", kind)
    flags = []
    for step in range(20):
        xd = dev(x)
        rebuilt = sc.update(xd)
        assert rebuilt == mod.update(x), "rebuild flag at step %d" % step
        flags.append(rebuilt)
        f, stats = sc.force(xd)
        fresh, _ = make("jittered_lattice", kind)
        assert fresh.update(xd)
        g, gstats = fresh.force(xd)
        assert_bits_equal(host(f), host(g), "node force at step %d (list %s)" % (step, "new" if rebuilt else "kept"))
        assert stats_of(stats) == stats_of(gstats)
        fresh.close()
        x = x + rng.normal(size=x.shape) * 0.02
    assert flags[0] and sum(flags[1:]) >= 2 and flags.count(False) >= 5, flags
    sc.close()


# ---- D. the step ------------------------------------------------------------------------------------------------------------------
import backbone_case as bc  # noqa: E402

STEPS = 10


def _stepper(case, kwargs=None):
    from mundy_amd import pipeline
    kw = bc.stepper_kwargs(case) if kwargs is None else kwargs
    return pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), **kw)


def _same_double(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


@gpu
@pytest.mark.parametrize("mode", bc.MODES)
@pytest.mark.parametrize("kind", KINDS)
def test_step_is_the_composed_models(kind, mode):
    """F, U_ext, U and the new statistics of STEPS steps, each from the stepper's own state at its start.  WCA: bit for
    bit.  Hertz: F within 1e-13 sum |F_c| per node (the sum over the linkers of the node's segments, the end terms
    included), and everything downstream of the device's own F bit for bit."""
    from mundy_amd import ops
    case = bc.build(kind, mode)
    st, model = _stepper(case), bc.segment_model(case)
    mt = host(st.mob_trans)
    rebuilds = 0
    for step in range(STEPS):
        x0 = host(st.center).copy()
        keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
        s = st.step()
        Dlam = None
        if mode == "none":
            assert s.num_contacts == 0 and s.converged and s.num_iters == 0 and s.max_overlap == 0.0 and st.op is None
            with pytest.raises(RuntimeError, match="no contacts"):
                st.body_contact_force()
        else:
            pairs, lam, normal = host(st.links.pairs), host(st.lam), host(st.contacts["normal"])
            assert s.num_contacts == len(pairs) > 0 and s.converged
            if mode == "first":
                Dlam = bc.contact_force(case, pairs, lam, normal)
                assert np.abs(Dlam).max() > 0.0
        F, info = bc.force_field(case, model, x0, Dlam)
        got_F = host(st.spring_force)
        assert np.abs(info["backbone"] - (0.0 if Dlam is None else Dlam)).max() > 0.0
        if kind == "wca":
            assert_bits_equal(got_F, F, "step %d: the force field" % step)
            assert _same_double(s.max_segment_overlap, info["max_segment_overlap"])
        else:
            err = np.abs(got_F - F).max(axis=1)
            print("step %d: max |dF| / sum |F_c| = %.3g" % (step, (err / np.maximum(info["scale"], 1e-300)).max()))
            assert (err <= 1e-13 * info["scale"]).all()
            assert abs(s.max_segment_overlap - info["max_segment_overlap"]) <= 1e-15
        assert (s.segment_contacts, s.num_segment_pairs, s.segment_list_rebuilt) == (
            info["segment_contacts"], info["num_segment_pairs"], info["rebuilt"])
        assert _same_double(s.max_spring_length, info["max_spring_length"])
        rebuilds += int(info["rebuilt"])
        # -- U_ext = (m_t F + U_brown) + u_hydro from the device's own F: the noise of the device's own kernel in bits
        u_hydro = 0.0
        if mode == "first":
            u_hydro = host(st.u_hydro)
            assert_bits_equal(u_hydro, bc.hydro_velocity(case, x0, got_F), "step %d: u_hydro of the whole field" % step)
        u_ext = host(st.u_ext)
        base = host(ops.brownian_velocity(keys, ctr, case["kt"], case["dt"], st.mob_trans,
                                          ops.drag_velocity(st.mob_trans, dev(got_F))))
        assert_bits_equal(u_ext[:, :3], base[:, :3] + u_hydro, "step %d: U_ext" % step)
        assert all_pos_zero(u_ext[:, 3:])
        vel = host(st.velocity)
        if mode == "lcp":
            sweep = host(st.op.body_velocity_of(st.lam))
            assert_bits_equal(vel, u_ext + sweep, "step %d: U = U_ext + M D lam" % step)
        else:
            assert_bits_equal(vel, u_ext, "step %d: U = U_ext" % step)
        assert_bits_equal(host(st.center), x0 + case["dt"] * vel[:, :3], "step %d: the Euler update" % step)
    assert rebuilds >= 2, "the list was built %d time(s) in %d steps" % (rebuilds, STEPS)
    assert mt.shape == (case["n"],)


def _run(case, steps, st=None):
    st = _stepper(case) if st is None else st
    for _ in range(steps):
        assert st.step().segment_contacts > 0
    return st


_STRAIGHT = {}


def _straight(kind, mode):
    """the undisturbed run of 2 STEPS steps -> the final centres; computed once"""
    if (kind, mode) not in _STRAIGHT:
        _STRAIGHT[kind, mode] = host(_run(bc.build(kind, mode), 2 * STEPS).center).copy()
    return _STRAIGHT[kind, mode]


@gpu
@pytest.mark.parametrize("mode", ["none", "first"])
@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_is_invariant_under_reorder_bodies(kind, mode):
    """reorder_bodies at step STEPS of 2 STEPS: every later row equals the unreordered run's, permuted, bit for bit (the
    segment numbering never changes, and a node sums its segments in ascending segment index)"""
    case = bc.build(kind, mode)
    want = _straight(kind, mode)
    st = _run(case, STEPS)
    keys0 = host(st.rng_keys).copy()
    perm = host(st.reorder_bodies(curve="morton", cell_size=2.0))
    assert (perm != np.arange(case["n"])).any() and (host(st.rng_keys) == keys0[perm]).all()
    _run(case, STEPS, st)
    order = np.argsort(host(st.rng_keys))   # the keys are the original numbers
    assert_bits_equal(host(st.center)[order], want, "centres after reorder_bodies")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_trajectory_is_invariant_under_snapshot_and_restore(kind):
    case = bc.build(kind, "none")
    want = _straight(kind, "none")
    st = _run(case, 7)
    snap = st.snapshot()
    _run(case, 3, st)
    st.restore(snap)
    s = st.step()
    assert s.segment_list_rebuilt, "restore marks the list stale"
    _run(case, 2 * STEPS - 8, st)
    assert_bits_equal(host(st.center), want, "centres after restore")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_crossed_strands_do_not_pass_through_each_other(kind):
    case = bc.crossed_strands(kind)
    # without an excluded volume the two strands, driven at m_t F each, would have crossed well within the run
    assert 2.0 * case["steps"] * case["dt"] * case["mob_trans"][0] * 10.0 > 2.0 * 0.9
    st = _stepper(case, bc.crossed_kwargs(case))
    ext = dev(case["ext"])
    low = bc.crossed_gap(case, case["center"])
    for _ in range(case["steps"]):
        s = st.step(external_force=ext)
        low = min(low, bc.crossed_gap(case, host(st.center)))
    x_model, low_model = bc.crossed_model_run(case)
    print("crossed strands, %s: smallest gap %.4f (model %.4f), final %.4f (model %.4f)" % (
        kind, low, low_model, bc.crossed_gap(case, host(st.center)), bc.crossed_gap(case, x_model)))
    assert low > 0.5 and low_model > 0.5 and s.segment_contacts > 0
    np.testing.assert_allclose(host(st.center), x_model, rtol=0, atol=1e-9)


# ---- E. the C++ stepper against the Python stepper -------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,mode", [("hertz", "none"), ("wca", "none"), ("hertz", "first"), ("wca", "lcp")])
def test_backbone_collision_step_app_matches_python(kind, mode):
    import os
    import subprocess
    import tempfile

    from cpp_apps import build_app, checksums, fnv1a_bits
    case = bc.build(kind, mode)
    st = _stepper(case)
    lines = []
    for k in range(2 * STEPS):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d converged %d rebuilt %d max_overlap %.17g max_spring_length %.17g "
                     "segment_pairs %d segment_contacts %d segment_list_rebuilt %d max_segment_overlap %.17g" % (
                         k, s.num_contacts, s.num_iters, s.converged, s.rebuilt, s.max_overlap, s.max_spring_length,
                         s.num_segment_pairs, s.segment_contacts, s.segment_list_rebuilt, s.max_segment_overlap))
    exe = build_app("backbone_collision_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        bc.write_app_input(case, path)
        out = subprocess.run([exe, path] + bc.app_arguments(case, 2 * STEPS), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert got == lines
    cs = checksums(out.stdout)
    assert cs["center"] == fnv1a_bits(host(st.center)) and cs["u_ext"] == fnv1a_bits(host(st.u_ext))
    assert sum("segment_list_rebuilt 1" in ln for ln in lines) >= 2
