"""CPU-side checks of the hydrodynamic velocity stage: the numpy model (tests/hydro_model.py) against closed forms,
Wilson's three spheres and its own symmetry; every refusal of mhip_hydro_velocity, ops.hydro_velocity and the stepper's
hydrodynamics= keyword, all of which happen before any HIP call."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import hydro_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. the model ------------------------------------------------------------------------------------------------------
def test_quake_inv_sqrt_has_the_error_of_one_newton_step():
    x = np.exp(np.linspace(math.log(1e-3), math.log(1e6), 20000))
    rel = np.abs(hm.quake_inv_sqrt(x) * np.sqrt(x) - 1.0)
    assert rel.max() < 1.8e-3
    assert rel.max() > 1e-3  # ONE step: a second one would bring it to ~5e-6
    # the bit trick itself, on one argument by hand
    i = np.float64(2.0).view(np.int64)
    y = (np.int64(0x5fe6eb50c7b537a9) - (i >> 1)).view(np.float64)
    assert hm.quake_inv_sqrt(np.array([2.0]))[0] == y * (1.5 - ((1.0 * y) * y))


def _one(kind, mu, d, a, b, f):
    return hm.pair_terms(kind, mu, np.asarray(d, dtype=np.float64)[None], np.array([b]), np.zeros((1, 3)),
                         np.array([a]), np.asarray(f, dtype=np.float64)[None])[0]


def test_rpyc_branch_selection_and_values():
    mu, f = 0.7, np.array([0.3, -1.1, 0.5])
    c6 = 1.0 / (6.0 * math.pi * mu)
    # far, both radii zero: the Stokeslet
    d = np.array([1.0, 2.0, -2.0])
    assert hm.rpyc_branch(d, 0.0, 0.0) == hm.FAR
    r = 3.0
    h = d / r
    want = (f + h * (f @ h)) / (8.0 * math.pi * mu * r)
    np.testing.assert_allclose(_one("rpyc", mu, d, 0.0, 0.0, f), want, rtol=1e-14)
    # far with radii: 1 + (a^2 + b^2) / (3 r^2), 1 - (a^2 + b^2) / r^2
    a, b = 0.9, 0.4
    assert hm.rpyc_branch(d, a, b) == hm.FAR
    q = (a * a + b * b) / (r * r)
    want = ((1.0 + q / 3.0) * f + (1.0 - q) * h * (f @ h)) / (8.0 * math.pi * mu * r)
    np.testing.assert_allclose(_one("rpyc", mu, d, a, b, f), want, rtol=1e-14)
    # overlapping with a != b (Zuk et al. 2014)
    d = np.array([0.0, 0.6, 0.8])
    a, b, r = 0.9, 0.4, 1.0
    assert hm.rpyc_branch(d, a, b) == hm.OVERLAP
    h = d / r
    t1 = (16.0 * r ** 3 * (a + b) - ((a - b) ** 2 + 3.0 * r * r) ** 2) / (32.0 * r ** 3)
    t2 = 3.0 * ((a - b) ** 2 - r * r) ** 2 / (32.0 * r ** 3)
    want = c6 / (a * b) * (t1 * f + t2 * h * (f @ h))
    np.testing.assert_allclose(_one("rpyc", mu, d, a, b, f), want, rtol=1e-13)
    # at touching the overlapping form continues the far field
    far = _one("rpyc", mu, d * (1.3 + 1e-9), a, b, f)
    over = _one("rpyc", mu, d * (1.3 - 1e-9), a, b, f)
    assert hm.rpyc_branch(d * (1.3 + 1e-9), a, b) == hm.FAR and hm.rpyc_branch(d * (1.3 - 1e-9), a, b) == hm.OVERLAP
    np.testing.assert_allclose(far, over, rtol=1e-7)
    # one sphere inside the other: r < |a - b|, local drag of the larger
    d = np.array([0.1, 0.0, 0.2])
    assert hm.rpyc_branch(d, 1.2, 0.3) == hm.LOCAL
    np.testing.assert_allclose(_one("rpyc", mu, d, 1.2, 0.3, f), c6 / 1.2 * f, rtol=1e-15)
    np.testing.assert_allclose(_one("rpyc", mu, d, 0.3, 1.2, f), c6 / 1.2 * f, rtol=1e-15)
    # coincident centres: skipped, whatever the radii
    for a, b in ((0.5, 0.5), (1.2, 0.3), (0.0, 0.0), (0.0, 0.7)):
        assert hm.rpyc_branch(np.zeros(3), a, b) == hm.SKIPPED
        assert np.all(_one("rpyc", mu, np.zeros(3), a, b, f) == 0.0)
    # a zero-radius target inside a source: not "overlapping" (needs both radii > 1e-12) but local drag
    d = np.array([0.3, 0.1, 0.0])
    assert hm.rpyc_branch(d, 0.8, 0.0) == hm.LOCAL
    np.testing.assert_allclose(_one("rpyc", mu, d, 0.8, 0.0, f), c6 / 0.8 * f, rtol=1e-15)


def test_rpy_and_stokes_agree_with_their_closed_forms_at_quake_accuracy():
    mu, f, d, a, b = 1.3, np.array([0.3, -1.1, 0.5]), np.array([2.0, -1.0, 2.5]), 0.6, 0.9
    r = math.sqrt(d @ d)
    h = d / r
    stokes = (f + h * (f @ h)) / (8.0 * math.pi * mu * r)
    np.testing.assert_allclose(_one("stokes", mu, d, a, b, f), stokes, rtol=6e-3)  # rinv^3 r^2: three quake factors
    q = (a * a + b * b) / (r * r)
    rpy = ((1.0 + q / 3.0) * f + (1.0 - q) * h * (f @ h)) / (8.0 * math.pi * mu * r)
    np.testing.assert_allclose(_one("rpy", mu, d, a, b, f), rpy, rtol=0, atol=1e-2 * np.abs(rpy).max())
    # coincident centres: rinv = 0, no contribution
    assert np.all(_one("stokes", mu, np.zeros(3), a, b, f) == 0.0) and np.all(_one("rpy", mu, np.zeros(3), a, b, f) == 0.0)


def _three_spheres(kind, s):
    """UnitTestPeriphery.cpp:671-774 (the reference only prints the result): returns (U2, U3) as it defines them"""
    R, mu = 12.34, 1.0
    x = np.array([[0.0, 0.0, 0.0], [-s * R / 2.0, -math.sqrt(3.0) * s * R / 2.0, 0.0],
                  [s * R / 2.0, -math.sqrt(3.0) * s * R / 2.0, 0.0]])
    f = np.zeros((3, 3))
    f[0, 1] = -6.0 * math.pi * R
    rad = np.full(3, R)
    u = hm.velocity(kind, mu, x, rad, f) + f / (6.0 * math.pi * R * mu)
    return u[1, 1], u[2, 0]


def test_wilson_three_spheres():
    u2, u3 = _three_spheres("rpyc", 6.0)
    print("s = 6: |U2 + 0.21586| = %.3g, |U3 - 0.05078| = %.3g" % (abs(u2 + 0.21586), abs(u3 - 0.05078)))
    assert abs(u2 + 0.21586) <= 2e-5
    assert abs(u3 - 0.05078) <= 5e-4
    # RPY is a far-field closure: near touching it is off by far more, so the agreement above is no accident
    u2, u3 = _three_spheres("rpyc", 2.01)
    print("s = 2.01: |U2 + 0.63461| = %.3g, |U3 - 0.00498| = %.3g" % (abs(u2 + 0.63461), abs(u3 - 0.00498)))
    assert abs(u2 + 0.63461) > 5e-2
    assert abs(u3 - 0.00498) > 5e-2


@pytest.mark.parametrize("kind", ["rpyc", "rpy"])
def test_model_mobility_is_symmetric(kind):
    n = 150
    d = hm.inputs(n, seed=3, density=0.6)
    assert (d["sa"] == 0.0).any()
    br = hm.rpyc_branch(d["sc"][:, None] - d["sc"][None], d["sa"][None], d["sa"][:, None])
    assert (br == hm.OVERLAP).sum() > 0 and (br == hm.FAR).sum() > 0
    rng = np.random.default_rng(5)
    f, g = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    mf = hm.velocity(kind, 0.8, d["sc"], d["sa"], f)
    mg, ag = hm.velocity(kind, 0.8, d["sc"], d["sa"], g, want_abs=True)
    bound = 4.0 * (n + 16) * 2.0 ** -53 * float((np.abs(f) * ag).sum())
    diff = abs(float((f * mg).sum()) - float((g * mf).sum()))
    print(kind, "asymmetry", diff, "bound", bound)
    assert diff <= bound


def test_chunked_sum_is_the_documented_order():
    d = hm.inputs(2 * hm.CHUNK + 77, 5, seed=1)
    u = hm.velocity("rpyc", 1.0, d["sc"], d["sa"], d["f"], d["tc"], d["tb"])
    # by hand: a python loop, one source at a time
    total = np.zeros((5, 3))
    for c0 in range(0, d["sc"].shape[0], hm.CHUNK):
        acc = np.zeros((5, 3))
        for s in range(c0, min(c0 + hm.CHUNK, d["sc"].shape[0])):
            acc = acc + hm.pair_terms("rpyc", 1.0, d["tc"], d["tb"], d["sc"][s], d["sa"][s], d["f"][s])
        total = total + acc
    assert np.array_equal(u.view(np.int64), total.view(np.int64))
    from mundy_amd import capi
    assert hm.CHUNK == capi.HYDRO_CHUNK
    text = open(os.path.join(ROOT, "include", "mundy_hip.h")).read()
    assert "#define MHIP_HYDRO_CHUNK %d\n" % hm.CHUNK in text


# ---- 2. the stepper's refusals (before the library is loaded) -------------------------------------------------------------
SPRINGS = (np.array([[0, 1], [1, 2], [2, 3]]), "hookean", 10.0, 1.0)


def _hy(**kw):
    d = dict(kind="rpyc")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not ...}


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
    (dict(hydrodynamics=_hy()), "belongs to the chain step"),
    (dict(kind="spherocylinder", hydrodynamics=_hy()), "belongs to the chain step"),
    (dict(kind="spherocylinder", hydrodynamics=_hy(), springs=SPRINGS), "spheres only"),
    (dict(kind="mixed", hydrodynamics=_hy(), brownian_kt=0.0), "spheres only"),
    (dict(kind="spherocylinder", hydrodynamics=_hy(), brownian_kt=0.0, growth_rate=0.1, division_length=2.0),
     "spheres only"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, growth_rate=0.1, division_length=2.0), "growth"),
    (dict(hydrodynamics=_hy(), brownian_kt=0.0, periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, friction=0.3), "friction"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, contact_cutoff=0.1), "contact_cutoff"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, contact_model="hertz", hertz_friction=0.3), "hertz_friction"),
    (dict(hydrodynamics="rpyc", springs=SPRINGS), "dict"),
    (dict(hydrodynamics=_hy(kind=...), springs=SPRINGS), "missing key"),
    (dict(hydrodynamics=_hy(colour=1), springs=SPRINGS), "unknown key"),
    (dict(hydrodynamics=_hy(kind="oseen"), springs=SPRINGS), "kind must be"),
    (dict(hydrodynamics=_hy(kind=2), springs=SPRINGS), "kind must be"),
    (dict(hydrodynamics=_hy(radius=-0.1), springs=SPRINGS), "radius must be finite"),
    (dict(hydrodynamics=_hy(radius=math.nan), springs=SPRINGS), "radius must be finite"),
    (dict(hydrodynamics=_hy(radius=[0.5, 0.5, math.inf, 0.5]), springs=SPRINGS), "radius must be finite"),
    (dict(hydrodynamics=_hy(radius=[0.5, 0.5, -1.0, 0.5]), springs=SPRINGS), "radius must be finite"),
    (dict(hydrodynamics=_hy(radius=[0.5, 0.5]), springs=SPRINGS), "shape"),
    (dict(hydrodynamics=_hy(update_every=0), springs=SPRINGS), "update_every"),
    (dict(hydrodynamics=_hy(update_every=-2), springs=SPRINGS), "update_every"),
    (dict(hydrodynamics=_hy(update_every=1.5), springs=SPRINGS), "update_every")])
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_check_hydrodynamics_accepts_what_it_should():
    from mundy_amd import ops
    assert ops.check_hydrodynamics(dict(kind="stokes"), 4) == ("stokes", None, 1)
    kind, radius, every = ops.check_hydrodynamics(dict(kind="rpy", radius=0.0, update_every=3), 4)
    assert (kind, every) == ("rpy", 3) and np.array_equal(radius, np.zeros(4))
    assert np.array_equal(ops.check_hydrodynamics(dict(kind="rpyc", radius=[1.0, 2.0, 0.0, 0.5]), 4)[1],
                          [1.0, 2.0, 0.0, 0.5])


def test_step_stats_and_wrapper_refusals(monkeypatch):
    from mundy_amd import capi, ops

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    c, r, f = (torch.zeros((2, 3), dtype=torch.float64), torch.ones(2, dtype=torch.float64),
               torch.zeros((2, 3), dtype=torch.float64))
    with pytest.raises(ValueError, match="kind must be"):
        ops.hydro_velocity("oseen", 1.0, c, r, f)
    for mu in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="viscosity"):
            ops.hydro_velocity("rpyc", mu, c, r, f)
    with pytest.raises(ValueError, match="src_radius must not be None"):
        ops.hydro_velocity("rpy", 1.0, c, None, f)
    with pytest.raises(ValueError, match="src_force must have shape"):
        ops.hydro_velocity("rpyc", 1.0, c, r, f[:1])
    with pytest.raises(ValueError, match="out must have shape"):
        ops.hydro_velocity("rpyc", 1.0, c, r, f, out=torch.zeros((2, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="accumulate needs out"):
        ops.hydro_velocity("rpyc", 1.0, c, r, f, accumulate=True)


# ---- 3. the library's own refusals (before any HIP call) -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


@pytest.fixture()
def handle(lib):
    from mundy_amd import capi
    h = C.c_void_p()
    capi.check(lib.mhip_hydro_create(C.byref(h)))
    yield h
    capi.check(lib.mhip_hydro_destroy(h))


P = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


def _call(lib, h, kind=2, mu=1.0, ns=3, sc=P, sa=P, sf=P, nt=2, tc=P, tb=P, vel=P, stride=3, acc=0):
    from mundy_amd import capi
    capi.check(lib.mhip_hydro_velocity(h, kind, mu, ns, sc, sa, sf, nt, tc, tb, vel, stride, acc, None))


@pytest.mark.parametrize("kw,match", [
    (dict(kind=3), "unknown hydrodynamic kernel kind"), (dict(kind=-1), "unknown hydrodynamic kernel kind"),
    (dict(mu=0.0), "viscosity"), (dict(mu=-1.0), "viscosity"), (dict(mu=math.nan), "viscosity"),
    (dict(mu=math.inf), "viscosity"),
    (dict(stride=4), "velocity_stride"), (dict(stride=0), "velocity_stride"), (dict(stride=-3), "velocity_stride"),
    (dict(sc=None), "null"), (dict(sf=None), "null"), (dict(sa=None), "null"), (dict(kind=1, sa=None), "null"),
    (dict(tc=None), "null"), (dict(vel=None), "null"), (dict(tb=None), "null"), (dict(kind=1, tb=None), "null"),
    (dict(kind=0, sc=None, sa=None, tb=None), "null")])
def test_hydro_velocity_refuses_before_any_hip_call(lib, handle, kw, match):
    with pytest.raises(ValueError, match=match):
        _call(lib, handle, **kw)


def test_hydro_velocity_null_handle_empty_calls_and_paths(lib, handle):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="handle is null"):
        _call(lib, None)
    with pytest.raises(ValueError, match="handle is null"):
        capi.check(lib.mhip_hydro_create(None))
    # nt == 0 does nothing, with or without arrays; ns == 0 with accumulate leaves velocity alone: no HIP call
    _call(lib, handle, nt=0, tc=None, tb=None, vel=None)
    _call(lib, handle, ns=0, sc=None, sa=None, sf=None, acc=1)
    with pytest.raises(ValueError, match="unknown hydro launch path"):
        capi.check(lib.mhip_hydro_set_path(handle, 3))
    capi.check(lib.mhip_hydro_set_path(handle, capi.HYDRO_PATH_PARTIAL))
    capi.check(lib.mhip_hydro_set_path(handle, capi.HYDRO_PATH_AUTO))
    with pytest.raises(ValueError, match="velocity_stride"):
        capi.check(lib.mhip_hydro_add_velocity(1, P, P, 5, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_hydro_add_velocity(1, None, P, 6, None))
    capi.check(lib.mhip_hydro_add_velocity(0, None, None, 6, None))


def test_step_stats_timings_name():
    # the stage mark the stepper adds after springs_brownian (timed=True) is called "hydrodynamics"
    import inspect

    from mundy_amd import pipeline
    src = inspect.getsource(pipeline.ContactStepper.external_velocity)
    assert src.index('mark("springs_brownian")') < src.index('mark("hydrodynamics")')


def test_hydro_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("hydro_step_app")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 1 and "Usage" in out.stderr
