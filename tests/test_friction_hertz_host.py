"""Frictional Hertzian rod contact, host side: the numpy model (tests/friction_hertz_model.py) gives the known answers of
stick, slide and reset, its spring coefficients are the reference's, the carry model keeps, drops, zeroes and flips, the
two-rod sled reaches its closed-form steady states; the new entry points are exported and bound, and every refusal
happens before any HIP call (no GPU needed)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import friction_hertz_model as fm


def _one_contact(sep, vel_j, td, mu=0.5, dt=1e-3, gn=0.0, gt=0.0):
    """rods 0 (along x) and 1 (along y) of radius 0.5 crossing at their centres, n = +z; rod 1 moves with vel_j"""
    seg = np.array([[-2.0, 0, 0, 2.0, 0, 0, 0, 0], [0, -2.0, 1.0 + sep, 0, 2.0, 1.0 + sep, 0, 0]])
    vel = np.zeros((2, 6))
    vel[1, :3] = vel_j
    return fm.friction_force(np.array([[0, 1]]), np.array([sep]), np.array([[0.0, 0.0, 1.0]]), np.array([0.5]),
                             np.array([0.5]), seg, np.array([0.5, 0.5]), 1000.0, 0.3, vel, mu, gn, gt, 1.0, dt, td)


def test_stick_then_slide_known_answers():
    # constant tangential velocity v: |F_t| = hp k_t v dt k grows linearly until it reaches mu |F_n|, then stays there
    # and the history stays at mu |F_n| / (hp k_t)
    sep, v, dt, mu = -0.02, 0.05, 1e-3, 0.5
    kn, kt = fm.spring_coefficients(1000.0, 1000.0, 0.3, 0.3)
    hp = math.sqrt(0.25 * 0.02)
    fn = hp * kn * 0.02
    k_slide = int(math.ceil(mu * fn / (hp * kt * v * dt)))
    assert 10 < k_slide < 400
    td = np.zeros((1, 3))
    for k in range(1, k_slide + 50):
        f, td, mx, sliding = _one_contact(sep, (v, 0.0, 0.0), td, mu=mu, dt=dt)
        ft = math.hypot(f[0, 0], f[0, 1])
        assert f[0, 2] == pytest.approx(-fn, rel=1e-14) and mx == 0.02
        if k < k_slide:
            assert sliding == 0 and ft == pytest.approx(hp * kt * v * dt * k, rel=1e-12)
            assert f[0, 0] > 0.0  # on body i, along the motion of j relative to i
        else:
            assert sliding == 1 and ft == pytest.approx(mu * fn, rel=1e-14)
            assert fm.norm(td[0]) == pytest.approx(mu * fn / (hp * kt), rel=1e-14)


def test_history_resets_where_the_pair_separates():
    td = np.array([[0.01, -0.02, 0.0]])
    f, td, mx, sliding = _one_contact(1e-6, (0.1, 0.0, 0.0), td)
    assert f.tolist() == [[0.0, 0.0, 0.0]] and td.tolist() == [[0.0, 0.0, 0.0]]
    assert not np.signbit(f).any() and not np.signbit(td).any() and mx == 0.0 and sliding == 0


def test_capped_force_without_history_is_zero():
    # mu = 0 and tangential damping only: |F_t| > 0 = mu |F_n| with tang_disp == 0 exactly (dt = 0) -> F_t = 0 (:508-510)
    f, td, _, sliding = _one_contact(-0.02, (0.05, 0.0, 0.0), np.zeros((1, 3)), mu=0.0, dt=0.0, gt=2.0)
    assert sliding == 1 and f[0, 0] == 0.0 and f[0, 1] == 0.0 and f[0, 2] < 0.0 and td.tolist() == [[0.0, 0.0, 0.0]]


def test_normal_damping_opposes_approach():
    f0, _, _, _ = _one_contact(-0.02, (0.0, 0.0, -0.1), np.zeros((1, 3)))
    f1, _, _, _ = _one_contact(-0.02, (0.0, 0.0, -0.1), np.zeros((1, 3)), gn=50.0)
    assert f1[0, 2] < f0[0, 2] < 0.0  # body i is pushed away harder while j approaches


def test_spring_coefficients_are_the_references():
    kn, kt = fm.spring_coefficients(5.0e5, 5.0e5, 0.3, 0.3)
    rn, rt = fm.reference_coefficients(5.0e5, 0.3)
    assert abs(kn - rn) <= 1e-14 * rn and abs(kt - rt) <= 1e-14 * rt


def test_carry_model_keeps_drops_zeroes_and_flips():
    old = np.array([[0, 1], [0, 2], [1, 3], [2, 3]])
    hist = np.arange(1.0, 13.0).reshape(4, 3)
    # same numbering: (0, 2) dropped, (1, 2) new
    new = np.array([[0, 1], [1, 2], [1, 3], [2, 3]])
    out, carried = fm.carry_history(old, hist, None, new)
    assert carried == 3 and out.tolist() == [hist[0].tolist(), [0.0] * 3, hist[2].tolist(), hist[3].tolist()]
    # renumbering 0 -> 3, 1 -> 1, 2 -> 0, 3 -> 2: old (0, 1) becomes (3, 1) -- listed as (1, 3), flipped
    ren = np.array([3, 1, 0, 2])
    new = np.array([[0, 2], [0, 3], [1, 2], [1, 3]])
    out, carried = fm.carry_history(old, hist, ren, new)
    # old (2, 3) -> (0, 2) kept; old (0, 2) -> (3, 0) flipped; old (1, 3) -> (1, 2) kept; old (0, 1) -> (3, 1) flipped
    assert carried == 4
    assert out.tolist() == [hist[3].tolist(), (-hist[1]).tolist(), hist[2].tolist(), (-hist[0]).tolist()]
    # a body that is gone carries nothing
    out, carried = fm.carry_history(old, hist, np.array([0, -1, 1, 2]), np.array([[0, 1], [1, 2]]))
    assert carried == 2 and out.tolist() == [hist[1].tolist(), hist[3].tolist()]
    out, carried = fm.carry_history(np.zeros((0, 2), int), np.zeros((0, 3)), None, np.array([[0, 1]]))
    assert carried == 0 and out.tolist() == [[0.0, 0.0, 0.0]]


def test_sled_sticks_below_the_coulomb_bound():
    _, kt, _, delta, hp, _ = fm.sled_constants()
    assert delta == pytest.approx(0.0195333, rel=1e-5)
    run = fm.sled(0.3, 0.5, 300)
    x, v, td, _ = run[-1]
    assert not any(r[3] for r in run)
    assert x == pytest.approx(0.3 / (hp * kt), rel=1e-12) and x == pytest.approx(4.7437957e-3, rel=1e-7)
    assert abs(v) < 1e-12 and td == pytest.approx(x, rel=1e-12)


def test_sled_slides_above_it_at_the_closed_form_speed():
    _, kt, _, _, hp, mt = fm.sled_constants()
    run = fm.sled(0.8, 0.5, 300)
    _, v, td, sliding = run[-1]
    assert sliding == 1
    assert v == pytest.approx(mt * (0.8 - 0.5 * 1.0), rel=1e-13) and v == pytest.approx(6.366197723, rel=1e-9)
    assert td == pytest.approx(0.5 * 1.0 / (hp * kt), rel=1e-13) and td == pytest.approx(7.90633e-3, rel=1e-5)


# ---- the library: exports and refusals before any HIP call -------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    for name in ("mhip_hertz_friction_force", "mhip_contact_op_body_sweep_vector", "mhip_contact_history_carry"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


_ARGS = ("pairs", "sep", "normal", "arc_s", "arc_t", "seg", "radius", "vel", "params", "tang_disp", "force", "stats")


def _friction(lib, prm=(0.5, 0.0, 0.0, 1.0, 1e-3), E0=1000.0, nu0=0.3, missing=()):
    from mundy_amd import capi
    p = {k: (None if k in missing else C.c_void_p(16)) for k in _ARGS}  # (never dereferenced)
    params = capi.HertzFrictionParams(*prm)
    return lib.mhip_hertz_friction_force(1, 2, p["pairs"], p["sep"], p["normal"], p["arc_s"], p["arc_t"], p["seg"],
                                         p["radius"], None, E0, None, nu0, p["vel"],
                                         None if "params" in missing else C.byref(params), p["tang_disp"], p["force"],
                                         p["stats"], None)


@pytest.mark.parametrize("prm,match", [((-0.1, 0, 0, 1, 1e-3), "mu"), ((float("nan"), 0, 0, 1, 1e-3), "mu"),
                                       ((float("inf"), 0, 0, 1, 1e-3), "mu"), ((0.5, -1.0, 0, 1, 1e-3), "damping"),
                                       ((0.5, 0, float("nan"), 1, 1e-3), "damping"),
                                       ((0.5, 0, float("inf"), 1, 1e-3), "damping"), ((0.5, 0, 0, -1.0, 1e-3), "density"),
                                       ((0.5, 0, 0, float("inf"), 1e-3), "density"), ((0.5, 0, 0, 1, -1e-3), "dt"),
                                       ((0.5, 0, 0, 1, float("nan")), "dt")])
def test_bad_parameters_are_refused_before_any_hip_call(lib, prm, match):
    from mundy_amd import capi
    with pytest.raises(ValueError, match=match):
        capi.check(_friction(lib, prm=prm))


@pytest.mark.parametrize("E0,nu0", [(0.0, 0.3), (float("nan"), 0.3), (1000.0, 0.0), (1000.0, 1.0)])
def test_bad_scalar_materials_are_refused_before_any_hip_call(lib, E0, nu0):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="youngs_modulus|poisson_ratio"):
        capi.check(_friction(lib, E0=E0, nu0=nu0))


@pytest.mark.parametrize("missing", _ARGS)
def test_null_pointers_are_refused_before_any_hip_call(lib, missing):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(_friction(lib, missing=(missing,)))


def test_sweep_and_carry_refuse_null_arguments(lib):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_contact_op_body_sweep_vector(None, None, None))
    p = C.c_void_p(16)
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_contact_history_carry(1, None, p, None, 0, 1, p, p, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_contact_history_carry(1, p, p, None, 0, 1, p, None, None, None))
    with pytest.raises(ValueError, match="in place"):
        capi.check(lib.mhip_contact_history_carry(1, p, p, None, 0, 1, p, p, None, None))


def test_python_checks_come_first():
    from mundy_amd import ops
    f64 = dict(dtype=torch.float64)
    pairs = torch.zeros((1, 2), dtype=torch.int32)
    a = dict(pairs=pairs, sep=torch.zeros(1, **f64), normal=torch.zeros((1, 3), **f64), arc_s=torch.zeros(1, **f64),
             arc_t=torch.zeros(1, **f64), seg=torch.zeros((2, 8), **f64), radius=torch.ones(2, **f64),
             velocity_prev=torch.zeros((2, 6), **f64), tang_disp=torch.zeros((1, 3), **f64))
    with pytest.raises(ValueError, match="mu"):
        ops.hertz_friction_force(mu=-1.0, dt=1e-3, **a)
    with pytest.raises(ValueError, match="damping"):
        ops.hertz_friction_force(mu=0.5, dt=1e-3, damping=(0.0, float("nan")), **a)
    with pytest.raises(ValueError, match="density"):
        ops.hertz_friction_force(mu=0.5, dt=1e-3, density=-1.0, **a)
    with pytest.raises(ValueError, match="dt"):
        ops.hertz_friction_force(mu=0.5, dt=float("inf"), **a)
    with pytest.raises(ValueError, match="poisson_ratio"):
        ops.hertz_friction_force(mu=0.5, dt=1e-3, poisson_ratio=1.0, **a)
    with pytest.raises(ValueError, match="tang_disp"):
        ops.hertz_friction_force(mu=0.5, dt=1e-3, **dict(a, tang_disp=torch.zeros((2, 3), **f64)))
    with pytest.raises(ValueError, match="velocity_prev"):
        ops.hertz_friction_force(mu=0.5, dt=1e-3, **dict(a, velocity_prev=torch.zeros((2, 3), **f64)))
    with pytest.raises(ValueError, match="hist_old"):
        ops.carry_contact_history(pairs, torch.zeros((2, 3), **f64), pairs)


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.ones(n, dtype=torch.float64)
    q = torch.zeros((n, 4), dtype=torch.float64)
    kind = kw.pop("kind", "spherocylinder")
    args = dict(contact_model="hertz", hertz_friction=0.5)
    args.update(kw)
    if kind == "sphere":
        return pipeline.ContactStepper("sphere", c, r, **args)
    if kind == "mixed":
        return pipeline.ContactStepper("mixed", c, None, q, kinds=torch.tensor([0, 1, 1, 1], dtype=torch.int32),
                                       shape=torch.ones((n, 3), dtype=torch.float64), **args)
    return pipeline.ContactStepper(kind, c, r, q, length=4.0 * r, **args)


@pytest.mark.parametrize("kw,match", [
    (dict(contact_model="lcp"), "contact_model='hertz'"), (dict(kind="sphere"), "spherocylinder"),
    (dict(kind="mixed"), "spherocylinder"), (dict(rod_kinematics=False), "rod_kinematics"),
    (dict(growth_rate=0.1, division_length=8.0), "growth"),
    (dict(springs=(np.array([[0, 1]], dtype=np.int32), "hookean", 1.0, 1.0)), "springs"),
    (dict(brownian_kt=0.0), "springs or brownian_kt"), (dict(friction=0.3), "friction"),
    (dict(hertz_friction=-0.5), "hertz_friction"), (dict(hertz_friction=float("nan")), "hertz_friction"),
    (dict(hertz_damping=(-1.0, 0.0)), "hertz_damping"), (dict(hertz_damping=(0.0, float("inf"))), "hertz_damping"),
    (dict(hertz_damping=1.0), "hertz_damping"), (dict(hertz_density=-1.0), "hertz_density"),
    (dict(periodic_box=torch.eye(3, dtype=torch.float64)), "orthorhombic"),
    (dict(hertz_friction=None, hertz_damping=(1.0, 0.5)), "pass hertz_friction"),
    (dict(hertz_friction=None, hertz_damping=1.0), "pass hertz_friction"),
    (dict(hertz_friction=None, hertz_density=2.0), "pass hertz_friction")])
def test_stepper_refusals_before_any_device_work(kw, match):
    # all refused in the constructor before anything reaches the device (these tensors are on the CPU)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_the_lcp_friction_keyword_stays_refused_under_hertz_as_before():
    with pytest.raises(ValueError, match="takes no friction"):
        _stepper(friction=0.3)


def test_step_stats_gain_num_sliding_with_default_zero():
    from mundy_amd import pipeline
    assert pipeline.StepStats().num_sliding == 0


def test_friction_hertz_step_app_compiles_and_links():
    # the C++ frictional stepper (include/mundy_hip/stepper.hpp, set_hertz_friction) and its driver build on the CPU box
    import os
    from cpp_apps import build_app
    exe = build_app("friction_hertz_step_app")
    assert os.path.exists(exe)
