"""Hertzian soft contact, host side: the numpy restatement reproduces the known answers of the model, the new entry
points are exported and bound, and bad arguments are refused before any HIP call (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

from hertz_model import effective_modulus, effective_radius, hertz_force


def test_known_answer_equal_materials():
    # spheres r = 1, 2; E = 1000, nu = 0.3 for both; centre distance 2.9 (sep = 2.9 - 3)
    radius = np.array([1.0, 2.0])
    assert effective_modulus(1000.0, 1000.0, 0.3, 0.3) == 549.4505494505495
    assert effective_radius(1.0, 2.0) == 0.6666666666666666
    f, mx = hertz_force(np.array([[0, 1]]), np.array([2.9 - 3.0]), radius, 1000.0, 0.3)
    assert f[0] == pytest.approx(18.915669578546606, rel=1e-14)
    assert mx == pytest.approx(0.1, rel=1e-14)


def test_known_answer_unequal_materials():
    # E = 1000 / 250, nu = 0.3 / 0.45, r = 0.5 / 0.5, delta = 0.02
    E = np.array([1000.0, 250.0])
    nu = np.array([0.3, 0.45])
    assert effective_modulus(E[0], E[1], nu[0], nu[1]) == 243.90243902439025
    f, mx = hertz_force(np.array([[0, 1]]), np.array([-0.02]), np.array([0.5, 0.5]), E, nu)
    assert f[0] == pytest.approx(0.459906849552226, rel=1e-14)
    assert mx == 0.02


def test_touching_and_separated_pairs_carry_exactly_plus_zero():
    f, mx = hertz_force(np.array([[0, 1], [1, 2]]), np.array([0.0, 0.5]), np.ones(3))
    assert f.tolist() == [0.0, 0.0] and not np.signbit(f).any() and mx == 0.0


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    for name in ("mhip_hertz_contact_force", "mhip_contact_op_body_sweep"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


def _hertz(lib, E=None, E0=1000.0, nu=None, nu0=0.3, c=1, pairs=1, sep=1, radius=1, force=1, mx=1):
    p = lambda v: None if v is None or v == 0 else C.c_void_p(16 * int(v))  # noqa: E731  (never dereferenced)
    return lib.mhip_hertz_contact_force(c, 2, p(pairs), p(sep), p(radius), p(E), E0, p(nu), nu0, p(force), p(mx), None)


@pytest.mark.parametrize("E0,nu0", [(0.0, 0.3), (-1.0, 0.3), (float("nan"), 0.3), (float("inf"), 0.3),
                                    (1000.0, 0.0), (1000.0, 1.0), (1000.0, -0.2), (1000.0, 1.5), (1000.0, float("nan"))])
def test_bad_scalar_materials_are_refused_before_any_hip_call(lib, E0, nu0):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="youngs_modulus|poisson_ratio"):
        capi.check(_hertz(lib, E0=E0, nu0=nu0))


@pytest.mark.parametrize("missing", ["pairs", "sep", "radius", "force", "mx"])
def test_null_pointers_are_refused_before_any_hip_call(lib, missing):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(_hertz(lib, **{missing: 0}))


def test_body_sweep_refuses_a_null_handle(lib):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_contact_op_body_sweep(None, None, None))


def test_python_material_checks_come_first():
    from mundy_amd import ops
    pairs = torch.zeros((1, 2), dtype=torch.int32)
    sep = torch.zeros(1, dtype=torch.float64)
    r = torch.ones(2, dtype=torch.float64)
    with pytest.raises(ValueError, match="youngs_modulus"):
        ops.hertz_contact_force(pairs, sep, r, youngs_modulus=0.0)
    with pytest.raises(ValueError, match="poisson_ratio"):
        ops.hertz_contact_force(pairs, sep, r, poisson_ratio=1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.hertz_contact_force(pairs, sep, r, youngs_modulus=torch.ones(3, dtype=torch.float64))


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.ones(n, dtype=torch.float64)
    q = torch.zeros((n, 4), dtype=torch.float64)
    kind = kw.pop("kind", "spherocylinder")
    extra = dict(kinds=torch.tensor([0, 1, 2, 1], dtype=torch.int32), shape=torch.ones((n, 3), dtype=torch.float64)) \
        if kind == "mixed" else dict(length=r)
    return pipeline.ContactStepper(kind, c, r, q, contact_model="hertz", **extra, **kw)


@pytest.mark.parametrize("kw,match", [(dict(friction=0.3), "friction"), (dict(contact_cutoff=0.1), "contact_cutoff"),
                                      (dict(warm_start=True), "warm-start"), (dict(kind="mixed"), "ellipsoid"),
                                      (dict(youngs_modulus=-5.0), "youngs_modulus"),
                                      (dict(poisson_ratio=0.0), "poisson_ratio")])
def test_stepper_refuses_what_hertz_mode_does_not_have(kw, match):
    # all refused in the constructor before anything reaches the device (these tensors are on the CPU)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_stepper_refuses_an_unknown_contact_model():
    from mundy_amd import pipeline
    with pytest.raises(ValueError, match="contact_model"):
        pipeline.ContactStepper("sphere", torch.zeros((1, 3), dtype=torch.float64), torch.ones(1, dtype=torch.float64),
                                contact_model="dem")


def test_step_stats_gain_max_overlap_with_default_zero():
    from mundy_amd import pipeline
    assert pipeline.StepStats().max_overlap == 0.0


def test_hertz_step_app_compiles_and_links():
    # the C++ Hertz stepper (include/mundy_hip/stepper.hpp, set_hertz_contact) and its driver build on the CPU box
    import os
    from cpp_apps import build_app
    exe = build_app("hertz_step_app")
    assert os.path.exists(exe)
