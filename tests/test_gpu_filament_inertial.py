"""The inertial filament step on the device (k_filament_predict, k_filament_correct and the kinetic energy of
filament.hip; the frictionless law of filament_contact.hip; include/mundy_hip_filament_inertial.h) against the numpy
model (filament_inertial_model.py), bit for bit unless said otherwise: every field after two full steps across tile
borders and the grid-stride loop's second pass, the kinetic energy against math.fsum, the stepper over 50 steps, the
frictionless law's rows (at the pow bar) and their reduction (bit for bit), inertial steps with contacts, the stiffness
ramp, the C++ driver, and the overdamped path of a handle that has been made inertial."""
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import filament_contact_model as fcm
import filament_inertial_model as fim
import filament_model as fm
from gpu_util import PAST_FULL_GRID, all_pos_zero, assert_bits_equal, dev, host
from test_gpu_filaments import BORDER_COUNTS, STATE, device_kwargs, make_case, new_device, new_model, params

pytestmark = pytest.mark.gpu

MOTION = ("velocity", "twist_velocity", "acceleration", "twist_acceleration")
ALL = STATE + ("acceleration", "twist_acceleration")
DT = 0.02
CRITICAL = dict(density=1.5, damping="critical")
CONSTANT = dict(density=1.5, damping=(0.3, 0.2))
POW_BAR = 1e-14   # the Hertz rows: device pow against numpy's


def new_inertial_model(case, prm, dynamics):
    f = fim.InertialFilaments(case["node_ptr"], case["radius"], case["rest_curvature"], case["arclength"], case["phase"],
                              prm)
    f.set_inertial(**dynamics)
    return f.set_state(case["center"], case["twist"], case["edge_orientation"])


def new_inertial_device(case, prm, dynamics, inertial_first=True):
    from mundy_amd import ops
    f = ops.Filaments(case["node_ptr"], case["radius"], case["rest_curvature"], case["arclength"], case["phase"],
                      **device_kwargs(prm))
    if inertial_first:
        f.set_inertial(**dynamics)
    f.set_state(dev(case["center"]), dev(case["twist"]), dev(case["edge_orientation"]))
    if not inertial_first:   # the fields are allocated, and zero, whichever call comes first
        f.set_inertial(**dynamics)
    return f


def assert_same(d, m, names, what):
    for name in names:
        assert_bits_equal(host(d.field(name)), getattr(m, name), "%s: %s" % (what, name))


def bits(x):
    return np.array([x], dtype=np.float64).view(np.uint64)[0]


def two_steps(case, prm, dynamics, external=None, energy=True, inertial_first=True):
    """two full steps: after the first a != 0 and v != 0, in the second t_old != t, so the binormal acts; every field
    after every kernel, the kinetic energy after every corrector -> (device, model)"""
    d, m = new_inertial_device(case, prm, dynamics, inertial_first), new_inertial_model(case, prm, dynamics)
    assert_same(d, m, ALL, "initial state")
    ext = None if external is None else dev(external)
    ke = torch.full((1,), -1.0, dtype=torch.float64, device="cuda")
    for k, time in enumerate((0.25, 0.5)):
        d.predict(DT)
        m.predict(DT)
        assert_same(d, m, ALL, "step %d: after predict" % k)
        stats = d.force(time, ext).tolist()
        want = m.compute_force(time, external)
        assert_bits_equal(np.array(stats), np.array(want), "step %d: statistics" % k)
        d.correct(DT, ke if energy else None)
        want_ke = m.correct(DT)
        assert_same(d, m, ALL, "step %d: after correct" % k)
        if energy:
            assert bits(float(ke[0])) == bits(want_ke), (k, float(ke[0]), want_ke)
            assert want_ke > 0.0
    assert np.abs(m.edge_binormal).max() > 1e-4 and np.abs(m.acceleration).max() > 1e-4
    assert np.abs(m.twist_acceleration).max() > 1e-6
    return d, m


# ---- 1. predict and correct, every field -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dynamics", [CRITICAL, CONSTANT], ids=["critical", "constant"])
@pytest.mark.parametrize("constrained", [False, True])
def test_two_steps_across_tile_borders_match_the_model(oracle, dynamics, constrained):
    assert np.cumsum(BORDER_COUNTS)[:3].tolist() == [256, 511, 513]
    case = make_case(41, BORDER_COUNTS)
    assert np.ptp(case["radius"]) > 0.3   # non-uniform radii: every node its own mass
    prm = params(wave=True, disable_twist=constrained, monolayer=constrained)
    d, m = two_steps(case, prm, dynamics, inertial_first=not constrained)
    if constrained:
        # the corrector runs after the constraints and writes all components; the head of the next step erases them
        assert np.abs(m.center[:, 0]).max() > 0.0 and np.abs(m.twist).max() > 0.0
        d.predict(DT)
        m.predict(DT)
        assert_same(d, m, ALL, "the third predict")
        assert all_pos_zero(m.center[:, 0]) and all_pos_zero(m.twist) and all_pos_zero(m.twist_acceleration)
        assert all_pos_zero(m.velocity[:, 0]) and all_pos_zero(m.acceleration[:, 0]) and all_pos_zero(m.twist_velocity)
    d.close()


@pytest.mark.parametrize("fixed", [(3,), (6,), (0, 3, 6)], ids=["middle", "end", "first_middle_end"])
def test_fixed_filaments_stay_where_they_are(oracle, fixed):
    case = make_case(42, BORDER_COUNTS)
    mask = np.zeros(len(BORDER_COUNTS), bool)
    mask[list(fixed)] = True
    ext = np.random.default_rng(6).normal(size=(case["n"], 3))
    d, m = two_steps(case, params(), dict(CRITICAL, fixed_filaments=mask), external=ext)
    rows = m.fixed
    assert rows.sum() == sum(BORDER_COUNTS[f] for f in fixed)
    assert_bits_equal(m.center[rows], case["center"][rows], "fixed nodes: center")
    assert_bits_equal(m.twist[rows], case["twist"][rows], "fixed nodes: twist")
    for name in MOTION:
        assert all_pos_zero(getattr(m, name)[rows]), name
        assert np.abs(getattr(m, name)[~rows]).max() > 0.0, name
    d.close()


def test_one_filament_of_three_nodes(oracle):
    d, _ = two_steps(make_case(43, (3,)), params(wave=True), CONSTANT)
    d.close()


def past_full_grid_case(seed):
    counts = [301] * (PAST_FULL_GRID // 301) + [PAST_FULL_GRID % 301]
    case = make_case(seed, counts)
    assert case["n"] == PAST_FULL_GRID and counts[-1] >= 3
    return case, len(counts)


def test_second_pass_of_the_grid_stride_loop(oracle):
    # 2048 workgroups of 256 lanes: node 2048 * 256 is the second pass of lane 0, and the 2048 block partials of the
    # kinetic energy are more than the 256 one pass of k_filament_energy_fold takes (this is the size that crosses it:
    # the border layout has 7 partials, the 3-node filament 1)
    case, F = past_full_grid_case(44)
    mask = np.zeros(F, bool)
    mask[-1] = True   # the filament the second pass works on
    d, _ = two_steps(case, params(wave=True), dict(CRITICAL, fixed_filaments=mask))
    d.close()


# ---- 2. the kinetic energy ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["three_nodes", "border", "past_full_grid"])
def test_kinetic_energy_is_the_exact_sum(oracle, which):
    case = {"three_nodes": lambda: make_case(45, (3,)), "border": lambda: make_case(46, BORDER_COUNTS),
            "past_full_grid": lambda: past_full_grid_case(47)[0]}[which]()
    n = case["n"]
    assert (n + 255) // 256 > 256 if which == "past_full_grid" else (n + 255) // 256 <= 256   # the fold's width
    prm = params()
    d, m = new_inertial_device(case, prm, CONSTANT), new_inertial_model(case, prm, CONSTANT)
    # zero velocities: exactly +0.0
    assert bits(float(d.kinetic_energy()[0])) == bits(0.0)
    rng = np.random.default_rng(8)
    # magnitudes over twelve binades: a sum that a plain double accumulation does not get right
    v = rng.normal(size=(n, 3)) * 2.0 ** rng.integers(-6, 6, (n, 1))
    w = rng.normal(size=n) * 2.0 ** rng.integers(-6, 6, n)
    d.set_motion(dev(v), dev(w))
    m.set_motion(v, w)
    assert_same(d, m, MOTION, "planted motion")
    terms = m.kinetic_terms()
    want = math.fsum(terms)
    got = float(d.kinetic_energy()[0])
    assert bits(got) == bits(want), (got, want)
    # the sum fused into the corrector: the same bits as the stand-alone entry point on the velocities it wrote
    ke = torch.empty(1, dtype=torch.float64, device="cuda")
    d.force(0.0)
    m.compute_force(0.0)
    d.correct(DT, ke)
    want = m.correct(DT)
    assert_same(d, m, MOTION, "after correct")
    assert bits(float(ke[0])) == bits(want) == bits(float(d.kinetic_energy()[0]))
    d.close()


def test_null_energy_pointer_changes_no_other_output(oracle):
    case = make_case(48, BORDER_COUNTS)
    a, _ = two_steps(case, params(wave=True), CRITICAL, energy=True)
    b, _ = two_steps(case, params(wave=True), CRITICAL, energy=False)
    for name in ALL:
        assert_bits_equal(host(a.field(name)), host(b.field(name)), name)
    a.close()
    b.close()


# ---- 3. the stepper ----------------------------------------------------------------------------------------------------------
def new_stepper(case, prm, dynamics, contacts=None):
    from mundy_amd import pipeline
    return pipeline.FilamentStepper(case["node_ptr"], case["center"], case["radius"], case["edge_orientation"],
                                    case["arclength"], twist=case["twist"], rest_curvature=case["rest_curvature"],
                                    phase=case["phase"], dynamics=dynamics, contacts=contacts, **device_kwargs(prm))


@pytest.mark.parametrize("constrained", [False, True])
def test_fifty_steps_match_the_model(oracle, constrained):
    case = make_case(49, BORDER_COUNTS)
    prm = params(wave=True, disable_twist=constrained, monolayer=constrained)
    st, m = new_stepper(case, prm, CRITICAL), new_inertial_model(case, prm, CRITICAL)
    dt = 0.01
    for k in range(50):
        got = st.step(dt)
        want, ke = m.step(dt, k * dt)
        assert_bits_equal(np.array([got.max_stretch, got.max_curvature_deviation, got.kinetic_energy]),
                          np.array([want[0], want[1], ke]), "step %d" % k)
    assert_same(st, m, ALL, "after 50 steps")
    assert np.isfinite(m.center).all() and np.abs(m.center - case["center"]).max() > 1e-3
    st.close()


# ---- 4. the frictionless law -------------------------------------------------------------------------------------------------
MATERIAL = dict(youngs_modulus=200.0, poisson_ratio=0.3)


def crossed_case(overlap=0.125, **kw):
    from mundy_amd import synth
    d = synth.crossed_filaments(6, 5, overlap=overlap, **kw)   # a dozen filaments of five nodes
    return dict(d, n=len(d["radius"]), phase=np.zeros(len(d["node_ptr"]) - 1) if d["phase"] is None else d["phase"])


def close_rows(got, want, what):
    """the pow bar: |got - want| <= POW_BAR * the largest magnitude of the row set"""
    scale = max(float(np.abs(want).max()), 1e-300)
    err = float(np.abs(got - want).max())
    assert err <= POW_BAR * scale, "%s: %.3e of %.3e" % (what, err, scale)


def test_frictionless_rows_and_their_reduction(oracle):
    from mundy_amd import ops
    case = crossed_case(angle=1.0)
    prm = params()
    d, m = new_device(case, prm), new_model(case, prm)
    spec = dict(skin=0.25, mu=0.5, **MATERIAL)
    dc, mc = ops.FilamentContacts(d, law="hertz", **spec), fim.HertzContacts(m, **spec)
    assert dc.update() and mc.update()
    assert np.array_equal(host(dc.field("pairs")), mc.pairs)
    ext = np.random.default_rng(9).normal(size=(case["n"], 3))
    stats = host(dc.force(DT, dev(ext)))   # no save_velocity
    want = mc.force_pass(DT, ext)
    touching = mc.sep < 0.0
    assert touching.sum() >= 8 and (~touching).sum() >= 1
    assert_bits_equal(host(dc.field("sep")), mc.sep, "sep")
    force, share = host(dc.field("force")), host(dc.field("share"))
    close_rows(force, mc.force, "force")
    close_rows(share, mc.share, "share")
    close_rows(host(dc.field("node_force")), mc.node_force, "node_force")
    assert all_pos_zero(force[~touching]) and all_pos_zero(share[~touching])
    assert all_pos_zero(host(dc.field("tang_disp")))
    assert float(stats[0]) == want[0] > 0.0 and int(stats.view(np.int64)[1]) == 0
    # the reduction of the device's own rows: bit for bit
    assert_bits_equal(host(dc.field("node_force")), fim.reduce_rows(mc, force, share, ext), "node_force of the device's rows")
    # the normal force alone: F is along -n, so the left segment is pushed away from the right one
    k = np.flatnonzero(touching)[0]
    i, j = mc.pairs[k]
    mid = lambda s: 0.5 * (mc.seg[s, 0:3] + mc.seg[s, 3:6])  # noqa: E731
    assert np.dot(force[k], mid(i) - mid(j)) > 0.0
    # back to law 0: the frictional rows of a handle that never left it
    d2 = new_device(case, prm)
    dc2 = ops.FilamentContacts(d2, **spec)
    dc.set_law("frictional")
    v = dev(np.random.default_rng(10).normal(size=(case["n"], 3)))
    for h, f in ((dc, d), (dc2, d2)):
        f.set_inertial(**CONSTANT)
        f.set_motion(v)
        h.save_velocity()
        h.update()
        h.force(DT, dev(ext))
    for name in ("sep", "tang_disp", "force", "share", "node_force"):
        assert_bits_equal(host(dc.field(name)), host(dc2.field(name)), "law 0 again: " + name)
    assert np.abs(host(dc.field("tang_disp"))).max() > 0.0
    for h in (dc, dc2, d, d2):
        h.close()


def test_refusals_on_a_live_handle():
    from mundy_amd import capi, ops
    case = crossed_case()
    d = new_device(case, params())
    dc = ops.FilamentContacts(d, skin=0.25, mu=0.5, **MATERIAL)
    with pytest.raises(ValueError, match="law"):
        dc.set_law("wca")
    with pytest.raises(ValueError, match="unknown filament contact law"):
        capi.check(capi.load().mhip_filament_contacts_set_law(dc._h, 2))
    dc.update()
    with pytest.raises(RuntimeError, match="save_velocity"):
        dc.force(DT)   # the frictional law still asks for it
    dc.set_law("hertz")
    dc.force(DT)
    # and the filaments' own
    with pytest.raises(RuntimeError, match="before mhip_filaments_set_inertial"):
        d.predict(DT)
    with pytest.raises(RuntimeError, match="before mhip_filaments_set_inertial"):
        d.correct(DT)
    with pytest.raises(RuntimeError, match="before mhip_filaments_set_inertial"):
        d.kinetic_energy()
    with pytest.raises(ValueError, match="density"):
        capi.check(capi.load().mhip_filaments_set_inertial(d._h, capi.FilamentInertialParams(0.0, 1, 0.0, 0.0), None))
    d.set_inertial(**CRITICAL)
    for call in (lambda: d.predict(-1.0), lambda: d.correct(float("nan"))):
        with pytest.raises(ValueError, match="dt must be finite"):
            call()
    dc.close()
    d.close()
    f = ops.Filaments(case["node_ptr"], case["radius"], case["rest_curvature"], case["arclength"], **device_kwargs(params()))
    f.set_inertial(**CRITICAL)
    for call in (lambda: f.predict(DT), lambda: f.correct(DT), lambda: f.kinetic_energy()):
        with pytest.raises(RuntimeError, match="before mhip_filaments_set_state"):
            call()
    f.close()


# ---- 5. inertial steps with contacts -----------------------------------------------------------------------------------------
STEP_CASE = dict(eta=0.04, mu=0.6, dt=0.01, overlap=0.02)


def contact_run(case, prm, law, skin, steps=20, lockstep_model=True):
    """`steps` inertial steps of the stepper with contacts, against the composed models when asked -> the final fields.
    Frictional law: everything bit for bit.  Frictionless law: the device's pow and numpy's may differ in the last
    place, so every step checks the model's own rows against the device's at the pow bar and then continues from the
    device's rows, which keeps everything downstream of the rows bit for bit."""
    contacts = dict(skin=skin, mu=STEP_CASE["mu"], damping=(0.1, 0.05), law=law, **MATERIAL)
    st = new_stepper(case, prm, CRITICAL, contacts)
    m = new_inertial_model(case, prm, CRITICAL)
    mc = (fim.HertzContacts if law == "hertz" else fcm.Contacts)(m, **{k: v for k, v in contacts.items()
                                                                    if law == "hertz" or k != "law"})
    dt = STEP_CASE["dt"]
    touched = 0
    for k in range(steps):
        got = st.step(dt)
        if not lockstep_model:
            continue
        what = "%s, step %d" % (law, k)
        mc.save_velocity()
        m.predict(dt)
        rebuilt = mc.update()
        cstats = mc.force_pass(dt)
        assert got.rebuilt == rebuilt and got.num_pairs == len(mc.pairs), what
        assert np.array_equal(host(st.contacts.field("pairs")), mc.pairs), what
        assert_bits_equal(host(st.contacts.field("sep")), mc.sep, what + ": sep")
        touched += int((mc.sep < 0.0).sum())
        if law == "hertz":
            force, share = host(st.contacts.field("force")), host(st.contacts.field("share"))
            if len(mc.pairs):
                close_rows(force, mc.force, what + ": force")
                close_rows(share, mc.share, what + ": share")
            mc.node_force = fim.reduce_rows(mc, force, share)
            assert all_pos_zero(host(st.contacts.field("tang_disp"))), what
        else:
            for name in ("tang_disp", "force", "share"):
                assert_bits_equal(host(st.contacts.field(name)), getattr(mc, name), "%s: %s" % (what, name))
            assert got.num_sliding == cstats[1], what
        assert_bits_equal(host(st.contacts.field("node_force")), mc.node_force, what + ": node_force")
        fstats = m.compute_force(k * dt, mc.node_force)
        ke = m.correct(dt)
        assert_bits_equal(np.array([got.max_stretch, got.max_curvature_deviation, got.max_overlap, got.kinetic_energy]),
                          np.array([fstats[0], fstats[1], cstats[0], ke]), what)
    out = {name: host(st.field(name)) for name in ALL}
    if lockstep_model:
        for name in ALL:
            assert_bits_equal(out[name], getattr(m, name), "%s, after %d steps: %s" % (law, steps, name))
        assert touched >= steps, touched   # it cannot pass on an empty list
    st.close()
    return out


@pytest.mark.parametrize("law", ["frictional", "hertz"])
def test_twenty_inertial_steps_with_contacts(oracle, law):
    case = crossed_case(overlap=STEP_CASE["overlap"], seed=7, angle=1.2)
    prm = fm.Params(**dict(params(wave=True).__dict__, eta=STEP_CASE["eta"]))
    small = contact_run(case, prm, law, skin=0.06)
    # the list's age does not reach the forces: a skin under which the list is rebuilt rarely or never
    large = contact_run(case, prm, law, skin=0.5, lockstep_model=False)
    for name in ALL:
        assert_bits_equal(small[name], large[name], "%s: skin 0.06 against 0.5: %s" % (law, name))


# ---- 6. the stiffness ramp ---------------------------------------------------------------------------------------------------
RAMP = dict(dt=0.1, relaxed=2.0, threshold=1e-5, growth=1.5)   # the model: [795, 87, 73, 62] steps, polled by 4: [796, 88, 72, 64]


def ramp_case():
    """three short straight filaments with a rest curvature: they bend into arcs at every level of the ramp"""
    case = make_case(50, (6, 5, 7))
    n = case["n"]
    fid = np.repeat(np.arange(3), (6, 5, 7))
    s = case["arclength"]
    case["center"] = np.stack([np.zeros(n), 4.0 * fid, s], axis=1)
    case["twist"] = np.zeros(n)
    case["edge_orientation"] = np.tile(fm.triad_orientation([0.0, 0.0, 1.0]), (n, 1))
    case["rest_curvature"] = np.tile([0.3, 0.0, 0.0], (n, 1))
    case["radius"] = np.full(n, 0.5)
    return case


@pytest.mark.parametrize("poll_every", [1, 4])
def test_equilibrate_matches_the_model(oracle, poll_every):
    case = ramp_case()
    prm = params(disable_twist=True, monolayer=True)
    dyn = dict(density=1.0, damping="critical")
    m = new_inertial_model(case, prm, dyn)
    want = fim.equilibrate(m, RAMP["dt"], 0.0, RAMP["relaxed"], RAMP["threshold"], RAMP["growth"])
    assert len(want) == len(fim.ramp_levels(RAMP["relaxed"], prm.E, RAMP["growth"])) >= 3 and min(want) >= 1
    assert max(want) > 4 and any(w % 4 for w in want)
    st = new_stepper(case, prm, dyn)
    got = st.equilibrate(RAMP["dt"], RAMP["relaxed"], threshold=RAMP["threshold"], growth=RAMP["growth"],
                         poll_every=poll_every)
    assert st.step_index == 0 and st.filaments.params.youngs_modulus == prm.E
    if poll_every == 1:
        assert got == want
        assert_same(st, m, ALL, "after the ramp")
    else:
        # a level ends at the first poll at or past the model's count, unless the energy has risen above the threshold
        # again by then -- the model with the same polling says which
        m4 = new_inertial_model(case, prm, dyn)
        want4 = fim.equilibrate(m4, RAMP["dt"], 0.0, RAMP["relaxed"], RAMP["threshold"], RAMP["growth"], poll_every=4)
        assert got == want4
        assert got[0] == -(-want[0] // 4) * 4 and all(g % 4 == 0 for g in got)
        assert_same(st, m4, ALL, "after the polled ramp")
    with pytest.raises(RuntimeError, match="max_steps"):
        st.equilibrate(RAMP["dt"], RAMP["relaxed"], threshold=0.0, growth=RAMP["growth"], max_steps=10)
    assert st.filaments.params.youngs_modulus == prm.E   # restored after the refusal too
    st.close()


# ---- 7. the overdamped path of an inertial handle ----------------------------------------------------------------------------
def test_the_overdamped_path_is_untouched(oracle):
    case = make_case(51, BORDER_COUNTS)
    prm = params(wave=True)
    a, b, m = new_device(case, prm), new_inertial_device(case, prm, CRITICAL), new_model(case, prm)
    for k in range(3):
        for d in (a, b):
            d.advance(DT)
            d.force(k * DT)
            d.velocity()
        m.step(DT, k * DT)
    for name in STATE:
        assert_bits_equal(host(a.field(name)), host(b.field(name)), name)
        assert_bits_equal(host(b.field(name)), getattr(m, name), "against the model: " + name)
    assert all_pos_zero(host(b.field("acceleration"))) and all_pos_zero(host(b.field("twist_acceleration")))
    a.close()
    b.close()


# ---- 8. the C++ driver -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_contacts", [False, True], ids=["filaments", "contacts"])
def test_filament_inertial_app_matches_python(with_contacts):
    from cpp_apps import build_app, checksums, fnv1a_bits
    if with_contacts:
        case = crossed_case(overlap=STEP_CASE["overlap"], seed=7, angle=1.2)
        prm = fm.Params(**dict(params(wave=True).__dict__, eta=STEP_CASE["eta"]))
        contacts = dict(skin=0.06, mu=STEP_CASE["mu"], damping=(0.1, 0.05), law="hertz", **MATERIAL)
        dynamics, fixed, ramp = dict(density=1.5, damping=(0.3, 0.2)), -1, None
    else:
        case, prm, contacts = ramp_case(), params(disable_twist=True, monolayer=True), None
        dynamics, fixed, ramp = dict(density=1.0, damping="critical", fixed_filaments=[False, True, False]), 1, RAMP
    st = new_stepper(case, prm, dynamics, contacts)
    dt, steps = 0.01, 20
    levels = []
    if ramp:
        dt = ramp["dt"]
        levels = st.equilibrate(dt, ramp["relaxed"], threshold=ramp["threshold"], growth=ramp["growth"], poll_every=2)
        assert len(levels) >= 3 and max(levels) > 2
    lines = [st.step(dt) for _ in range(steps)]
    assert all(s.kinetic_energy > 0.0 for s in lines)
    exe = build_app("filament_inertial_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([len(case["node_ptr"]) - 1, case["n"]], dtype=np.uint64).tofile(f)
            case["node_ptr"].astype(np.int32).tofile(f)
            for name in ("center", "twist", "edge_orientation", "radius", "rest_curvature", "arclength", "phase"):
                case[name].astype(np.float64).tofile(f)
        args = [dt, prm.E, prm.nu, prm.l0, prm.eta, prm.A, prm.k, prm.omega]
        flags = [str(int(prm.wave)), str(int(prm.disable_twist)), str(int(prm.monolayer))]
        critical = dynamics["damping"] == "critical"
        iargs = [repr(float(dynamics["density"])), "1" if critical else "0"] + \
            [repr(float(c)) for c in ((0.0, 0.0) if critical else dynamics["damping"])] + [str(fixed)]
        rargs = [repr(float(ramp["relaxed"])), repr(float(ramp["threshold"])), repr(float(ramp["growth"])), "2"] if ramp \
            else ["0", "0", "1.1", "1"]
        cargs = []
        if with_contacts:
            cargs = [repr(float(a)) for a in (contacts["skin"], MATERIAL["youngs_modulus"], MATERIAL["poisson_ratio"],
                                              contacts["mu"], 0.1, 0.05, 1.0, -1.0)] + ["1", "1"]
        out = subprocess.run([exe, path, str(steps)] + [repr(float(a)) for a in args] + flags + iargs + rargs + cargs,
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got_levels = [int(ln.split()[3]) for ln in out.stdout.splitlines() if ln.startswith("LEVEL")]
    assert got_levels == levels
    got = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert len(got) == steps
    for k, (w, s) in enumerate(zip(got, lines)):
        assert_bits_equal(np.array([float.fromhex(w[3]), float.fromhex(w[5]), float.fromhex(w[7]), float.fromhex(w[11])]),
                          np.array([s.max_stretch, s.max_curvature_deviation, s.kinetic_energy, s.max_overlap]),
                          "step %d" % k)
        assert (int(w[9]), int(w[13]), int(w[15])) == (s.num_pairs, s.num_sliding, int(s.rebuilt)), k
    sums = checksums(out.stdout)
    for name in ("center", "twist", "velocity", "twist_velocity", "acceleration", "twist_acceleration", "edge_orientation"):
        assert sums[name] == fnv1a_bits(host(st.field(name))), name
    if with_contacts:
        assert sums["node_force"] == fnv1a_bits(host(st.contacts.field("node_force")))
        assert sum(s.num_pairs for s in lines) > 0 and max(s.max_overlap for s in lines) > 0.0
    st.close()
