"""The full HP1 step -- every stage on in one stepper (tests/hp1_case.py) -- on the device.

1. pipeline.ContactStepper against the composed numpy models, three steps, bit for bit: the force field in the
   reference's association, u_hydro of that whole field on update steps and carried on the stale one, U_ext, the
   velocity, and every statistic of StepStats (none of a term that is off moves from zero).
2. The all-on trajectory under snapshot / restore across a stale-u_hydro step, and under reorder_bodies.
3. tests/cpp/hp1_step_app (mech::SphereChainStepper with the same stages) against the Python stepper over 20 steps.

Tolerances: none of this file's own.  The noise of the numpy model is compared at the 1e-13 of
tests/test_gpu_chain.py::test_hertz_chain_velocity_is_external_plus_contact (its log and cos are numpy's), next to the
bit comparison against the device's own noise kernel; a KMC decision is compared with the model's outside the 1e-12
margin of tests/test_gpu_crosslinkers.py (exp is numpy's), next to the exact event counts from the device's heads; the
active springs' next_time at the 1e-13 of tests/test_gpu_nucleus.py."""
import os
import subprocess

import numpy as np
import pytest

import chain_model as chm
import hertz_model
import hp1_case as hp1
import periphery_model as pm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

CASE_IDS = [hp1.case_id(c) for c in hp1.CASES]


def _stepper(case):
    from mundy_amd import pipeline
    return pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), **hp1.stepper_kwargs(case))


def _heads(st):
    return tuple(host(t).astype(np.int64) for t in st.crosslinker_state())


def _active(st):
    s, nt, el, ct = st.active_state()
    return dict(state=host(s), next_time=host(nt), elapsed=host(el), counters=host(ct).view(np.uint64))


def _same_double(a, b):
    return np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


# ---- 1. the Python stepper against the composed models ----------------------------------------------------------------------
@pytest.mark.parametrize("letters", hp1.CASES, ids=CASE_IDS)
def test_step_is_the_composed_models(oracle, letters):
    """Each of three steps from the stepper's own state at its start (centres, heads, active state, keys and counters)
    and, where it has to be, read after it (heads after the KMC, states after the sampling, the device's multipliers and
    normals).  update_every = 2: step 1 adds a stale u_hydro, step 2 recomputes it."""
    from mundy_amd import ops
    case = hp1.build(letters)
    on, n, radius = case["letters"], case["n"], case["radius"]
    st = _stepper(case)
    mt = host(st.mob_trans)
    assert_bits_equal(mt, case["mob_trans"], "the mobility the C++ input carries")
    if "W" in on:
        assert st.hydro["periphery_min_pivot"] == hp1.periphery_inverse(case)[1]
    ext = dev(case["ext"]) if "E" in on else None
    acted = {c: 0 for c in "XYPAUWEH" if c in on}
    acted["contacts"] = 0   # (either contact model: some multiplier is positive)
    bound = 0
    for step in range(3):
        x0 = host(st.center).copy()
        keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
        if "X" in on:
            le0, ri0 = _heads(st)
            xc0 = host(st.xl_counter).copy()
        if "A" in on:
            a0 = _active(st)
        if "U" in on:
            u_prev, update = host(st.u_hydro).copy(), st.hydro_step % case["hydro"]["update_every"] == 0
            assert update == (step != 1)
        s = st.step(external_force=ext)
        # -- contacts: the oracle's separations, the device's multipliers
        pairs, lam, normal = host(st.links.pairs), host(st.lam), host(st.contacts["normal"])
        sep, _ = oracle.contact_spheres(pairs, x0, radius)
        assert_bits_equal(host(st.contacts["sep"]), sep, "separations")
        assert s.num_contacts == len(pairs) == len(lam) and s.converged
        acted["contacts"] += int(lam.max() > 0.0)
        Dlam = None
        if "H" in on:
            assert ((lam > 0) == (sep < 0)).all() and s.num_iters == 0
            assert _same_double(s.max_overlap, hertz_model.hertz_force(pairs, sep, radius)[1]) and s.max_overlap > 0
            if case["first_term"]:
                Dlam = hp1.contact_force(case, pairs, lam, normal)
                acted["H"] += int(np.abs(Dlam).max() > 0.0)
            else:
                acted["H"] += int(lam.max() > 0.0)
        else:
            assert (lam >= 0).all() and s.max_overlap == 0.0
        # -- crosslinker KMC: events counted from the device's own heads; decisions against the model outside its margin
        heads = None
        if "X" in on:
            heads = le, ri = _heads(st)
            assert (le == le0).all() and (host(st.xl_counter) == xc0 + 1).all()
            binds, unbinds = int(((ri0 == le0) & (ri != le)).sum()), int(((ri0 != le0) & (ri == le)).sum())
            assert (((ri0 != le0) & (ri != le)) <= (ri == ri0)).all()   # a bound head stays where it is or lets go
            bound += binds - unbinds
            assert (s.crosslinker_binds, s.crosslinker_unbinds, s.crosslinker_bound) == (binds, unbinds, bound)
            k = hp1.kmc(case, x0, le0, ri0, xc0)
            safe = k["margin"] > 1e-12
            print("step %d: binds %d unbinds %d; %d of %d decisions outside the margin" % (step, binds, unbinds,
                                                                                          safe.sum(), len(le)))
            # (a uniform falls within 1e-12 of one of a row's few thresholds with probability ~1e-11: all but never)
            assert safe.sum() >= len(le) - 2 and (ri[safe] == k["right"][safe]).all()
            if safe.all():
                assert (binds, unbinds) == (k["binds"], k["unbinds"])
        else:
            assert (s.crosslinker_binds, s.crosslinker_unbinds, s.crosslinker_bound, s.crosslinker_periphery_bound,
                    s.max_crosslinker_length) == (0, 0, 0, 0, 0.0)
        # -- active sampling: the model decides from the device's previous (elapsed, next_time)
        state = None
        if "A" in on:
            ku = np.arange(len(a0["state"]), dtype=np.uint64)
            want, switches = pm.active_sample(a0, ku, case["active"]["kon"], case["active"]["koff"])
            a1 = _active(st)
            state = a1["state"]
            assert (state == want["state"]).all() and (a1["counters"] == want["counters"]).all()
            assert s.active_switches == switches
            assert_bits_equal(a1["elapsed"], want["elapsed"] + case["dt"], "elapsed after the step")
            assert (np.abs(a1["next_time"] - want["next_time"]) <= 1e-13 * want["next_time"]).all()
        else:
            assert (s.active_springs, s.active_switches) == (0, (0, 0))
        # -- the force field
        F, info = hp1.force_field(case, x0, heads, state, Dlam)
        assert_bits_equal(host(st.spring_force), F, "step %d: the force field" % step)
        for c, did in info["acted"].items():
            acted[c] += int(did)
        assert _same_double(s.max_spring_length, info["max_spring_length"])
        if "X" in on:
            assert s.crosslinker_bound == info["crosslinker_bound"]
            assert s.crosslinker_periphery_bound == info["crosslinker_periphery_bound"]
            assert _same_double(s.max_crosslinker_length, info["max_crosslinker_length"])
            if "Y" not in on:
                assert s.crosslinker_periphery_bound == 0 and (ri >= 0).all()
        if "P" in on:
            assert s.periphery_colliding == info["periphery_colliding"]
            assert _same_double(s.max_periphery_overlap, info["max_periphery_overlap"])
        else:
            assert (s.periphery_colliding, s.max_periphery_overlap) == (0, 0.0)
        if "A" in on:
            assert s.active_springs == info["active_springs"] == int(state.sum())
        # -- u_hydro: of the whole field on an update step, the previous one on the stale step
        u_hydro = 0.0
        if "U" in on:
            u_hydro = host(st.u_hydro)
            if update:
                plain = hp1.hydro_velocity(case, x0, F, correction=False)
                want_h = hp1.hydro_velocity(case, x0, F)
                assert_bits_equal(u_hydro, want_h, "step %d: u_hydro of the whole force field" % step)
                springs_only = hp1.hydro_velocity(case, x0, info["spring_force"])
                assert (want_h.view(np.uint64) != springs_only.view(np.uint64)).any(axis=1).sum() >= n // 2
                acted["U"] += int(np.abs(plain).max() > 0.0)
                if "W" in on:
                    acted["W"] += int((want_h.view(np.uint64) != plain.view(np.uint64)).any())
            else:
                assert_bits_equal(u_hydro, u_prev, "step %d: the stale u_hydro" % step)
                assert np.abs(u_hydro).max() > 0.0
        # -- U_ext = (m_t F + U_brown) + u_hydro: the noise of the device's own kernel in bits, the model's at 1e-13
        u_ext = host(st.u_ext)
        keys_h, ctr_h = host(keys).view(np.uint64).copy(), host(ctr).view(np.uint64).copy()   # (the kernel advances ctr)
        base = host(ops.brownian_velocity(keys, ctr, case["kt"], case["dt"], st.mob_trans,
                                          ops.drag_velocity(st.mob_trans, dev(F))))
        assert_bits_equal(u_ext[:, :3], base[:, :3] + u_hydro, "step %d: U_ext" % step)
        assert all_pos_zero(u_ext[:, 3:])
        model, ctr1 = chm.brownian_velocity(keys_h, ctr_h, case["kt"], case["dt"], mt, chm.drag_velocity(mt, F))
        worst = float(np.abs(u_ext[:, :3] - (model[:, :3] + u_hydro)).max())
        print("step %d: max |U_ext - model| = %.3g" % (step, worst))
        assert worst <= 1e-13 and (host(st.rng_counter).view(np.uint64) == ctr1).all()
        # -- the velocity
        vel = host(st.velocity)
        if case["first_term"]:
            assert_bits_equal(vel, u_ext, "step %d: U = U_ext" % step)
        else:   # U = U_ext + M D lam: the body sweep of the device's multipliers
            sweep = host(st.op.body_velocity_of(st.lam))
            assert_bits_equal(sweep[:, :3], mt[:, None] * hp1.contact_force(case, pairs, lam, normal), "M D lam")
            assert_bits_equal(vel, u_ext + sweep, "step %d: U = U_ext + M D lam" % step)
    # every term that is on acted on some bead in at least one of the steps
    assert all(v > 0 for v in acted.values()), acted


# ---- 2. the all-on trajectory under restore and reorder -----------------------------------------------------------------------
STEPS = 20
_STRAIGHT = {}


def _run(case, steps, st=None):
    st = _stepper(case) if st is None else st
    for _ in range(steps):
        s = st.step(external_force=dev(case["ext"][host(st.ids)]))   # the force follows its bead
        assert s.converged and s.max_overlap > 0.0
    return st


def _final(st):
    """(centres, right heads as ids or -(s + 1), active state, next_time) in the order of the original ids"""
    ids = host(st.ids)
    order = np.argsort(ids)
    le, ri = _heads(st)
    a = _active(st)
    return host(st.center)[order], np.where(ri < 0, ri, ids[np.maximum(ri, 0)]), a["state"], a["next_time"]


def _straight(case):
    """the undisturbed run of a case; computed once"""
    key = hp1.case_id(case["letters"])
    if key not in _STRAIGHT:
        _STRAIGHT[key] = _final(_run(case, STEPS))
    return _STRAIGHT[key]


def _assert_same_trajectory(got, want, what):
    assert_bits_equal(got[0], want[0], "centres " + what)
    assert (got[1] == want[1]).all(), "right heads " + what
    assert (got[2] == want[2]).all(), "active states " + what
    assert_bits_equal(got[3], want[3], "next_time " + what)


def test_all_on_trajectory_is_invariant_under_snapshot_and_restore():
    """snapshot() at step 7 -- odd, so the u_hydro it saves is a stale one --, three more steps, restore()"""
    case = hp1.build(hp1.ALL)
    want = _straight(case)
    st = _run(case, 7)
    assert st.hydro_step == 7
    snap = st.snapshot()
    _run(case, 3, st)
    st.restore(snap)
    assert st.hydro_step == 7
    _assert_same_trajectory(_final(_run(case, STEPS - 7, st)), want, "after restore")
    assert (want[1] < 0).any() and (want[1] >= 0).any() and want[2].any()   # tethers, bead bonds and active springs


@pytest.mark.parametrize("letters", [hp1.ALL - set("UW"), hp1.ALL], ids=lambda c: hp1.case_id(c))
def test_trajectory_is_invariant_under_reorder_bodies(letters):
    """reorder_bodies(curve="morton") at step 10 of 20, the external force following its bead.

    Crosslinkers, periphery sites, wall, active dipoles, external force and Hertz contact round every sum once or take
    it in an order the numbering does not reach.  The hydrodynamics do neither: the all-pairs sums of u_hydro and of the
    correction walk the sources in index order, and skip_same_index, the reference's quirk,
    drops the term of surface node i onto bead i.  The stepper therefore evaluates them in the constructor's numbering
    whatever the rows' order.  Before it did, this test measured on the all-on case (640 beads, 1920 coordinates; right
    heads and active states equal in every variant) max |dx| = 0.1 with all 1920 coordinates different in bits, 7.1e-15
    (109) with skip_same_index=False, 1.8e-15 (32) without W, and 0 without U and W."""
    case = hp1.build(letters)
    want = _straight(case)
    st = _run(case, STEPS // 2)
    perm = host(st.reorder_bodies(curve="morton", cell_size=2.0))
    assert (perm != np.arange(case["n"])).any()
    got = _final(_run(case, STEPS - STEPS // 2, st))
    print("%s after reorder_bodies: max |centre difference| = %.3g, %d of %d coordinates differ in bits, %d of %d right "
          "heads differ" % (hp1.case_id(letters), np.abs(got[0] - want[0]).max(),
                            int((got[0].view(np.uint64) != want[0].view(np.uint64)).sum()), want[0].size,
                            int((got[1] != want[1]).sum()), len(want[1])))
    _assert_same_trajectory(got, want, "after reorder_bodies")


# ---- 3. the C++ stepper against the Python stepper -------------------------------------------------------------------------------
def _app_letters(letters):
    """mech::SphereChainStepper has the Hertz contact with its force as the first term only, pipeline.ContactStepper has
    that order as a key of hydrodynamics= only: the case without U runs in both with the LCP"""
    return letters if "U" in letters else letters - {"H"}


@pytest.mark.parametrize("letters", hp1.CASES, ids=CASE_IDS)
def test_hp1_step_app_matches_python(letters):
    import tempfile

    from cpp_apps import build_app, checksums, fnv1a, fnv1a_bits
    case = hp1.build(_app_letters(letters))
    on = case["letters"]
    st = _stepper(case)
    ext = dev(case["ext"]) if "E" in on else None
    lines = []
    for k in range(STEPS):
        s = st.step(external_force=ext)
        lines.append("STEP %d contacts %d iterations %d converged %d rebuilt %d born %d sliding %d carried 0 "
                     "springs_overstretched 0 binds %d unbinds %d bound %d periphery_bound %d crosslinkers_overstretched 0 "
                     "colliding %d active %d on %d off %d max_overlap %.17g max_spring_length %.17g "
                     "max_crosslinker_length %.17g max_periphery_overlap %.17g" % (
                         k, s.num_contacts, s.num_iters, s.converged, s.rebuilt, s.num_born, s.num_sliding,
                         s.crosslinker_binds, s.crosslinker_unbinds, s.crosslinker_bound, s.crosslinker_periphery_bound,
                         s.periphery_colliding, s.active_springs, s.active_switches[0], s.active_switches[1],
                         s.max_overlap, s.max_spring_length, s.max_crosslinker_length, s.max_periphery_overlap))
    exe = build_app("hp1_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        hp1.write_app_input(case, path)
        out = subprocess.run([exe, path] + hp1.app_arguments(case, STEPS), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert got == lines
    cs = checksums(out.stdout)
    bits32 = lambda a: fnv1a(np.ascontiguousarray(a, dtype=np.int32).view(np.uint32).tolist())  # noqa: E731
    assert cs["center"] == fnv1a_bits(host(st.center))
    assert cs["u_ext"] == fnv1a_bits(host(st.u_ext))
    assert ("right" in cs) == ("X" in on) and ("state" in cs) == ("A" in on)
    if "X" in on:
        assert cs["right"] == bits32(host(st.crosslinker_state()[1]))
    if "A" in on:
        a = _active(st)
        assert cs["state"] == bits32(a["state"]) and cs["next_time"] == fnv1a_bits(a["next_time"])
    if "W" in on:
        pivot = [ln for ln in out.stdout.splitlines() if ln.startswith("PERIPHERY")][0].split()[-1]
        assert pivot == "%.17g" % st.hydro["periphery_min_pivot"]
