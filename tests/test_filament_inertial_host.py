"""CPU-side checks of the inertial filaments (include/mundy_hip_filament_inertial.h): known answers of the numpy model
(filament_inertial_model.py) in dyadic inputs, its recurrence against the closed form in mpmath, its fixed point (the
overdamped one), the stiffness ramp on the model, the frictionless law's known answer, every refusal of the library
(before any HIP call), of ops and of the stepper, and the header against the binding table and the library.

Calibration (test_recurrence_against_its_closed_form prints the figures again).  With E = 0, constant damping and a
constant force every component of a node follows one affine map of (x, v, a); the two-node filament along its axis, under
its stretch term alone, one of (z0, z1, v0, v1, a0, a1).  The map is taken to the K-th power in mpmath (potentials.DPS
digits), K = 64, and the numpy model's state after K steps is compared in units of eps times the largest magnitude the
trajectory of that quantity reaches.  Measured here: RECURRENCE_MEASURED; the bound is four times that."""
import ctypes as C
import math
import os
import re

import mpmath as mp
import numpy as np
import pytest

import filament_inertial_model as fim
import filament_model as fm
import potentials as P
from gpu_util import all_pos_zero

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_filament_inertial.h")
NAMES = ("mhip_filaments_set_inertial", "mhip_filaments_set_motion", "mhip_filaments_predict", "mhip_filaments_correct",
         "mhip_filaments_kinetic_energy", "mhip_filaments_set_youngs_modulus", "mhip_filaments_get_inertial",
         "mhip_filament_contacts_set_law")
EPS = 2.0 ** -52
K_STEPS = 64
# worst deviation of the numpy model from the mpmath closed form after K_STEPS steps, in eps of the trajectory's magnitude
RECURRENCE_MEASURED = {"free_node": 3.81, "two_nodes": 22.8}   # 3.80355, 22.7139
RECURRENCE_BOUND = {k: 4.0 * v for k, v in RECURRENCE_MEASURED.items()}
# the arc: what the model reaches after ARC_STEPS steps (test_the_fixed_point_is_the_overdamped_one prints it)
# measured: angle 5.3e-15, length 3.6e-15, kinetic energy 3.5e-29 (the rounding floor); the bound is the existing 1e-12, and
# 1e-24 is the kinetic energy of velocities of that size
ARC_STEPS, ARC_BOUND, ARC_ENERGY = 2000, 1e-12, 1e-24


def straight(n, spacing=1.0, radius=1.0, rest=(0.0, 0.0, 0.0), counts=None, **prm):
    counts = [n] if counts is None else counts
    ptr = np.concatenate([[0], np.cumsum(counts)])
    n = int(ptr[-1])
    fid = np.repeat(np.arange(len(counts)), counts)
    s = (np.arange(n) - ptr[:-1][fid]) * spacing
    c = np.stack([np.zeros(n), 4.0 * fid, s], axis=1)
    q = np.tile(fm.triad_orientation([0.0, 0.0, 1.0]), (n, 1))
    f = fim.InertialFilaments(ptr, np.full(n, radius), np.tile(np.asarray(rest, dtype=np.float64), (n, 1)), s,
                              params=fm.Params(**prm))
    return f, c, q


def dyadic_density(radius, mass):
    """a density at which the model's node mass is exactly `mass`"""
    r3 = (radius * radius) * radius
    rho = mass / (4.0 / 3.0 * math.pi * r3)
    for cand in (rho, np.nextafter(rho, 0.0), np.nextafter(rho, np.inf)):
        if 4.0 / 3.0 * math.pi * r3 * cand == mass:
            return float(cand)
    raise AssertionError("no density gives the mass %r at radius %r" % (mass, radius))


# ---- 1. known answers ------------------------------------------------------------------------------------------------------
def test_a_constant_force_on_a_free_node_in_dyadic_inputs(oracle):
    rho = dyadic_density(0.5, 2.0)
    f, c, q = straight(0, radius=0.5, counts=[2, 2], E=0.0, l0=1.0)
    f.set_inertial(rho, (0.0, 0.0), fixed_filaments=[False, True])
    f.set_state(c, np.zeros(4), q)
    m, _ = f.mass()
    assert np.array_equal(m, np.full(4, 2.0))
    F = np.array([[0.5, -1.0, 0.25], [0.0, 0.0, 0.0], [3.0, 3.0, 3.0], [1.0, 0.0, 0.0]])
    dt = 0.25
    _, ke = f.step(dt, 0.0, F)
    a = F[0] / 2.0
    assert np.array_equal(f.acceleration[0], a)
    assert np.array_equal(f.velocity[0], (dt / 2.0) * a)
    assert np.array_equal(f.center[0], c[0] + (dt * dt / 4.0) * a)
    # the second node of the free filament feels nothing: E = 0
    assert all_pos_zero(f.acceleration[1]) and all_pos_zero(f.velocity[1]) and np.array_equal(f.center[1], c[1])
    # the fixed filament stays where it is, all four fields +0.0, whatever pulls on it
    for name in ("velocity", "acceleration", "twist_velocity", "twist_acceleration"):
        assert all_pos_zero(getattr(f, name)[2:]), name
    assert np.array_equal(f.center[2:], c[2:]) and all_pos_zero(f.twist)
    # kinetic energy: 0.5 m v.v of the one moving node, every factor dyadic
    v = (dt / 2.0) * a
    assert ke == 0.5 * 2.0 * (v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])) > 0.0
    # a second step: x = x + dt v + (dt dt / 4) a, then a again F / m (no damping), x += (dt dt / 4) a, v += dt a
    f.step(dt, dt, F)
    assert np.array_equal(f.acceleration[0], a) and np.array_equal(f.velocity[0], (1.5 * dt) * a)
    # (the start from a(0) = 0 costs the first step half of its displacement: 1.25 dt dt a, not 2 dt dt a)
    assert np.array_equal(f.center[0], c[0] + (1.25 * dt * dt) * a)


def test_the_twist_follows_the_same_law(oracle):
    # a torque cannot be applied from outside; the map of the twist is checked through set_motion: with E = 0 the torque
    # is 0 and twist_acceleration = -(c_r / I) twist_velocity
    rho = dyadic_density(0.5, 2.0)
    f, c, q = straight(3, radius=0.5, E=0.0, l0=1.0)
    f.set_inertial(rho, (0.0, 0.125)).set_state(c, np.zeros(3), q)
    _, I = f.mass()
    assert np.array_equal(I, np.full(3, 0.4 * 2.0 * 0.25))
    w = np.array([1.0, -2.0, 0.5])
    f.set_motion(twist_velocity=w)
    dt = 0.5
    f.step(dt, 0.0)
    ta = 1.0 / I * (0.0 - 0.125 * w)
    assert np.array_equal(f.twist_acceleration, ta)
    assert np.array_equal(f.twist_velocity, w + (dt * 0.5) * ta)
    assert np.array_equal(f.twist, (0.0 + dt * w) + (dt * dt * 0.25) * ta)


# ---- 2. the recurrence against its closed form ---------------------------------------------------------------------------------
def mp_power(A, k):
    R = mp.eye(A.rows)
    for _ in range(k):
        R = A * R
    return R


def free_node_map(dt, m, c, F):
    """(x, v, a, 1) -> one step, exactly: predict x' = x + dt v + (dt dt / 4) a; a' = (F - c v) / m;
    x'' = x' + (dt dt / 4) a'; v' = v + (dt / 2) a + (dt / 2) a'"""
    dt, m, c, F = (mp.mpf(float(x)) for x in (dt, m, c, F))
    q, h = dt * dt / 4, dt / 2
    an = [0, -c / m, 0, F / m]
    x = [1 + q * an[0], dt + q * an[1], q + q * an[2], q * an[3]]
    v = [h * an[0], 1 + h * an[1], h + h * an[2], h * an[3]]
    return mp.matrix([x, v, an, [0, 0, 0, 1]])


def two_node_map(dt, m, c, k, l0):
    """(z0, z1, v0, v1, a0, a1, 1) -> one step of the two-node filament along z under its stretch force: after the
    predictor, F1 = -k ((z1' - z0') - l0) on the right node and -F1 on the left one"""
    dt, m, c, k, l0 = (mp.mpf(float(x)) for x in (dt, m, c, k, l0))
    q, h = dt * dt / 4, dt / 2
    unit = lambda i: [1 if j == i else 0 for j in range(7)]  # noqa: E731
    add = lambda *rows: [sum(col) for col in zip(*rows)]  # noqa: E731
    mul = lambda s, row: [s * x for x in row]  # noqa: E731
    z0p = add(unit(0), mul(dt, unit(2)), mul(q, unit(4)))
    z1p = add(unit(1), mul(dt, unit(3)), mul(q, unit(5)))
    F1 = add(mul(-k, add(z1p, mul(-1, z0p))), mul(k * l0, unit(6)))
    a0 = mul(1 / m, add(mul(-1, F1), mul(-c, unit(2))))
    a1 = mul(1 / m, add(F1, mul(-c, unit(3))))
    z0 = add(z0p, mul(q, a0))
    z1 = add(z1p, mul(q, a1))
    v0 = add(unit(2), mul(h, unit(4)), mul(h, a0))
    v1 = add(unit(3), mul(h, unit(5)), mul(h, a1))
    return mp.matrix([z0, z1, v0, v1, a0, a1, unit(6)])


def measure_free_node():
    r, rho, c_t, dt = 0.75, 1.3, 0.4, 0.1
    F = np.array([0.7, -1.1, 0.3])
    f, c, q = straight(2, radius=r, E=0.0, l0=1.0)
    f.set_inertial(rho, (c_t, 0.0)).set_state(c, np.zeros(2), q)
    ext = np.zeros((2, 3))
    ext[0] = F
    track = np.zeros((3, 3))
    for k in range(K_STEPS):
        f.step(dt, k * dt, ext)
        track = np.maximum(track, np.abs(np.stack([f.center[0] - c[0], f.velocity[0], f.acceleration[0]])))
    m = f.mass()[0][0]
    worst = 0.0
    with P.hp():
        for comp in range(3):
            A = mp_power(free_node_map(dt, m, c_t, F[comp]), K_STEPS)
            want = A * mp.matrix([0, 0, 0, 1])
            got = (f.center[0, comp] - c[0, comp], f.velocity[0, comp], f.acceleration[0, comp])
            for j in range(3):
                worst = max(worst, float(abs(mp.mpf(float(got[j])) - want[j]) / (EPS * track[j, comp])))
    return worst


def measure_two_nodes():
    r, rho, c_t, dt, E, l0 = 0.5, 1.1, 0.3, 0.05, 6.0, 1.0
    f, c, q = straight(2, spacing=1.25, radius=r, E=E, l0=l0, disable_twist=True)
    f.set_inertial(rho, (c_t, 0.0)).set_state(c, np.zeros(2), q)
    z_start = c[:, 2].copy()
    track = np.zeros(6)
    for k in range(K_STEPS):
        f.step(dt, k * dt)
        state = np.concatenate([f.center[:, 2], f.velocity[:, 2], f.acceleration[:, 2]])
        track = np.maximum(track, np.abs(state))
    assert all_pos_zero(f.center[:, 0]) and np.array_equal(f.center[:, 1], c[:, 1])
    assert np.abs(f.velocity[:, 2]).max() > 1e-3 and track[2] > 0.05
    m = f.mass()[0][0]
    k_spring = E * math.pi * r * r / l0
    with P.hp():
        A = mp_power(two_node_map(dt, m, c_t, k_spring, l0), K_STEPS)
        want = A * mp.matrix([mp.mpf(float(z_start[0])), mp.mpf(float(z_start[1])), 0, 0, 0, 0, 1])
        worst = max(float(abs(mp.mpf(float(state[j])) - want[j]) / (EPS * track[j])) for j in range(6))
    return worst


def test_recurrence_against_its_closed_form(oracle):
    got = {"free_node": measure_free_node(), "two_nodes": measure_two_nodes()}
    print("recurrence: deviation in eps of the trajectory's magnitude", got, "bound", RECURRENCE_BOUND)
    for name, value in got.items():
        assert value <= RECURRENCE_BOUND[name], (name, value)


# ---- 3. the fixed point is the overdamped one -------------------------------------------------------------------------------
def test_the_fixed_point_is_the_overdamped_one(oracle):
    from test_filament_host import turning_angles
    # the filament of test_filament_host.py::test_relaxation_to_an_arc with mass, under critical damping
    f, c, q = straight(6, rest=(0.3, 0.0, 0.0), E=10.0, nu=0.3, l0=1.0, eta=1.0, disable_twist=True, monolayer=True)
    f.set_inertial(1.0, "critical").set_state(c, np.zeros(6), q)
    for s in range(ARC_STEPS):
        _, ke = f.step(0.1, s * 0.1)
    angle, length = turning_angles(f.center)
    print("angle error", np.abs(angle - 2.0 * math.asin(0.15)).max(), "length error", np.abs(length - 1.0).max(),
          "kinetic energy", ke)
    assert np.abs(angle - 2.0 * math.asin(0.15)).max() < ARC_BOUND
    assert np.abs(length - 1.0).max() < ARC_BOUND
    assert 0.0 <= ke < ARC_ENERGY
    # The corrector runs after the constraints: the reference's force has a component along the binormal of the old and
    # the new tangent, which is normal to the plane, and the monolayer removes what it does at
    # the head of the next step.  At rest the binormal vanishes.
    assert np.abs(f.center[:, 0]).max() < ARC_BOUND and all_pos_zero(f.twist)
    f.predict(0.1)
    assert all_pos_zero(f.center[:, 0]) and all_pos_zero(f.velocity[:, 0]) and all_pos_zero(f.acceleration[:, 0])


# ---- 4. equilibrate on the model -----------------------------------------------------------------------------------------------
def test_equilibrate_on_the_model(oracle):
    f, c, q = straight(6, rest=(0.3, 0.0, 0.0), E=10.0, nu=0.3, l0=1.0, disable_twist=True, monolayer=True)
    f.set_inertial(1.0, "critical").set_state(c, np.zeros(6), q)
    # the reference's own loop (:1800-1863), by repeated *= 1.1 in floating point
    E, levels = 1.0, 0
    while E < 10.0:
        levels += 1
        E *= 1.1
    assert levels == 25 == len(fim.ramp_levels(1.0, 10.0))
    steps = fim.equilibrate(f, 0.1, 0.0, 1.0, threshold=1e-7)
    assert len(steps) == levels and min(steps) >= 1 and max(steps) > 1
    assert f.prm.E == 10.0
    assert f.kinetic_energy() <= 1e-7
    with pytest.raises(RuntimeError, match="max_steps"):
        fim.equilibrate(f, 0.1, 0.0, 1.0, threshold=0.0, max_steps=30)
    assert f.prm.E == 10.0
    # a ramp that starts at or above the modulus has no level
    assert fim.equilibrate(f, 0.1, 0.0, 10.0) == []


# ---- 5. the frictionless law's known answer -------------------------------------------------------------------------------------
def test_two_crossed_segments_under_the_frictionless_law(oracle):
    # two 2-node filaments of radius 0.5 crossing at their midpoints, the centrelines 0.75 apart: sep = -0.25, R* = 0.25
    c = np.array([[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.75, -1.0, 0.0], [0.75, 1.0, 0.0]])
    q = np.tile([1.0, 0.0, 0.0, 0.0], (4, 1))
    f = fm.Filaments([0, 2, 4], np.full(4, 0.5), np.zeros((4, 3)), [0.0, 2.0, 0.0, 2.0], params=fm.Params(E=10.0, l0=2.0))
    f.set_state(c, np.zeros(4), q)
    E, nu = 1000.0, 0.25
    hc = fim.HertzContacts(f, skin=0.25, youngs_modulus=E, poisson_ratio=nu)
    assert hc.update() and hc.pairs.tolist() == [[0, 2]]
    stats = hc.force_pass(0.01)
    Es = (E * E) / (E - E * nu * nu + E - E * nu * nu)
    F = (4.0 / 3.0) * Es * math.sqrt(0.25) * 0.25 ** 1.5
    assert np.array_equal(hc.sep, [-0.25]) and stats == (0.25, 0)
    assert np.array_equal(hc.force, [[-F, 0.0, 0.0]])
    assert all_pos_zero(hc.tang_disp)
    # the contact points are the midpoints: each end node takes half
    assert np.array_equal(hc.node_force[:, 0], [-0.5 * F, -0.5 * F, 0.5 * F, 0.5 * F])
    assert all_pos_zero(np.abs(hc.node_force[:, 1:]))
    # apart: nothing, and +0.0
    f.center = c + np.array([[0.0, 0, 0], [0.0, 0, 0], [0.5, 0, 0], [0.5, 0, 0]])
    hc.update()
    assert hc.force_pass(0.01) == (0.0, 0) and all_pos_zero(hc.force) and all_pos_zero(hc.node_force)


# ---- 6. the library: header, table, refusals before any HIP call --------------------------------------------------------------
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_header_symbols_are_exported_and_bound_and_the_table_names_nothing_else(lib):
    from mundy_amd import capi
    protos = header_prototypes()
    assert set(protos) == set(NAMES) == set(capi.FILAMENT_INERTIAL_SIGNATURES)
    for other in (capi.SIGNATURES, capi.PERIPHERY_SIGNATURES, capi.CONTACT_FORCE_SIGNATURES,
                  capi.PERIPHERY_BINDING_SIGNATURES, capi.SEGMENT_CONTACT_SIGNATURES, capi.HYDRO_SOLVE_SIGNATURES):
        assert not set(capi.FILAMENT_INERTIAL_SIGNATURES) & set(other)
    inc = os.path.join(ROOT, "include")
    others = [open(os.path.join(inc, h)).read() for h in sorted(os.listdir(inc))
              if h.endswith(".h") and h != "mundy_hip_filament_inertial.h"]
    assert len(others) >= 6
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.FILAMENT_INERTIAL_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
        assert "mhip_stream_t" not in args   # every call runs on the stream of its handle
    text = open(HEADER).read()
    for macro, value in (("MHIP_FILAMENT_DAMPING_CONSTANT", capi.FILAMENT_DAMPING_CONSTANT),
                         ("MHIP_FILAMENT_DAMPING_CRITICAL", capi.FILAMENT_DAMPING_CRITICAL),
                         ("MHIP_FILAMENT_CONTACT_FRICTIONAL", capi.FILAMENT_CONTACT_FRICTIONAL),
                         ("MHIP_FILAMENT_CONTACT_HERTZ", capi.FILAMENT_CONTACT_HERTZ)):
        assert value == int(re.search(r"#define %s (\d+)" % macro, text).group(1))
    # the structs as the header lays them out
    body = re.search(r"typedef struct mhip_filament_inertial_params \{(.*?)\} mhip_filament_inertial_params;",
                     re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = [w.strip().split()[-1] for part in body.split(";") if part.strip()
              for w in re.sub(r"^\s*(double|int)\s+", "", part.strip()).split(",")]
    assert fields == [f[0] for f in capi.FilamentInertialParams._fields_]
    assert C.sizeof(capi.FilamentInertialParams) == 32 and C.sizeof(capi.FilamentInertialFields) == 16
    # mundy_hip.h no longer calls any of it "not built"
    main = open(os.path.join(inc, "mundy_hip.h")).read()
    assert "mundy_hip_filament_inertial.h" in main and "the\n * inertial variants" not in main


def test_library_refuses_before_any_hip_call(lib):
    from mundy_amd import capi
    prm = lambda rho=1.0, kind=1, ct=0.0, cr=0.0: C.byref(capi.FilamentInertialParams(rho, kind, ct, cr))  # noqa: E731
    nan, inf = float("nan"), float("inf")
    # set_inertial checks what needs no handle first: every refusal can be had without a device
    for args, match in (((None, None, None), "params is null"), ((None, prm(rho=0.0), None), "density"),
                        ((None, prm(rho=-1.0), None), "density"), ((None, prm(rho=nan), None), "density"),
                        ((None, prm(rho=inf), None), "density"), ((None, prm(kind=2), None), "unknown damping kind 2"),
                        ((None, prm(kind=-1), None), "unknown damping kind"),
                        ((None, prm(kind=0, ct=-0.5), None), "damping coefficients"),
                        ((None, prm(kind=0, cr=-0.5), None), "damping coefficients"),
                        ((None, prm(kind=0, ct=nan), None), "damping coefficients"),
                        ((None, prm(kind=0, cr=inf), None), "damping coefficients"),
                        ((None, prm(), None), "handle is null"), ((None, prm(kind=0, ct=1.0, cr=2.0), None), "handle is null")):
        with pytest.raises(ValueError, match=match):
            capi.check(lib.mhip_filaments_set_inertial(*args))
    # the critical kind does not read the two numbers
    with pytest.raises(ValueError, match="handle is null"):
        capi.check(lib.mhip_filaments_set_inertial(None, prm(kind=1, ct=-1.0, cr=nan), None))
    for E in (-1.0, nan, inf):
        with pytest.raises(ValueError, match="youngs_modulus"):
            capi.check(lib.mhip_filaments_set_youngs_modulus(None, E))
    for law in (-1, 2):
        with pytest.raises(ValueError, match="unknown filament contact law"):
            capi.check(lib.mhip_filament_contacts_set_law(None, law))
    fields = capi.FilamentInertialFields()
    one = (C.c_double * 1)()
    for call in (lambda: lib.mhip_filaments_set_motion(None, None, None, None, None),
                 lambda: lib.mhip_filaments_predict(None, 0.1), lambda: lib.mhip_filaments_correct(None, 0.1, None),
                 lambda: lib.mhip_filaments_kinetic_energy(None, C.cast(one, C.c_void_p)),
                 lambda: lib.mhip_filaments_set_youngs_modulus(None, 1.0),
                 lambda: lib.mhip_filaments_get_inertial(None, C.byref(fields)),
                 lambda: lib.mhip_filament_contacts_set_law(None, 1)):
        with pytest.raises(ValueError, match="handle is null"):
            capi.check(call())


def test_ops_and_stepper_refuse_bad_dynamics():
    from mundy_amd import ops, pipeline
    good = dict(density=1.0, damping="critical", fixed_filaments=None)
    for change, match in ((dict(density=0.0), "density"), (dict(density=float("nan")), "density"),
                          (dict(damping="viscous"), "damping"), (dict(damping=(1.0,)), "damping"),
                          (dict(damping=(-1.0, 0.0)), r"damping\[0\]"), (dict(damping=(0.0, float("inf"))), r"damping\[1\]"),
                          (dict(fixed_filaments=np.zeros(3, bool)), "fixed_filaments"),
                          (dict(fixed_filaments=np.zeros(1)), "fixed_filaments")):
        spec = dict(good, **change)
        with pytest.raises(ValueError, match=match):
            ops.check_filament_inertial(1, **spec)
        with pytest.raises(ValueError, match=match):
            pipeline.FilamentStepper([0, 4], np.zeros((4, 3)), np.ones(4), np.zeros((4, 4)), np.arange(4.0),
                                     youngs_modulus=10.0, rest_length=1.0, viscosity=1.0, dynamics=spec)
    with pytest.raises(ValueError, match="unknown key"):
        pipeline.FilamentStepper([0, 4], np.zeros((4, 3)), np.ones(4), np.zeros((4, 4)), np.arange(4.0),
                                 youngs_modulus=10.0, rest_length=1.0, viscosity=1.0, dynamics=dict(density=1.0, mass=2.0))
    with pytest.raises(ValueError, match="missing key"):
        pipeline.FilamentStepper([0, 4], np.zeros((4, 3)), np.ones(4), np.zeros((4, 4)), np.arange(4.0),
                                 youngs_modulus=10.0, rest_length=1.0, viscosity=1.0, dynamics=dict(damping="critical"))
    prm, fixed = ops.check_filament_inertial(2, 1.5, (0.25, 0.5), [True, False])
    assert (prm.density, prm.damping_kind, prm.translational_damping, prm.twist_damping) == (1.5, 0, 0.25, 0.5)
    assert fixed.dtype == np.uint8 and fixed.tolist() == [1, 0]
    assert ops.check_filament_inertial(2, 1.5)[0].damping_kind == 1
    # the contacts' law
    spec = dict(skin=0.1, youngs_modulus=10.0, poisson_ratio=0.3, mu=0.5)
    with pytest.raises(ValueError, match="law"):
        ops.check_filament_contacts(4, law="wca", **spec)
    with pytest.raises(ValueError, match="law"):
        pipeline.FilamentStepper([0, 4], np.zeros((4, 3)), np.ones(4), np.zeros((4, 4)), np.arange(4.0),
                                 youngs_modulus=10.0, rest_length=1.0, viscosity=1.0, contacts=dict(spec, law="wca"))
    ops.check_filament_contacts(4, law="hertz", **spec)
