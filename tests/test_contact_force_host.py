"""CPU-side checks of the per-body contact force (include/mundy_hip_contact_force.h): the new header against the library
and its binding table; every refusal the library makes from its arguments alone, through ctypes, before any HIP call
(the refusals that need an operator handle -- null x / out, a staged solve, a partitioned operator -- need device memory:
tests/test_gpu_contact_force.py); the wrappers' and the stepper's refusals with the loader disabled; the model
(tests/contact_force_model.py) against hand-computed cases; the new C++ app compiles and links."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import contact_force_model as cm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_contact_force.h")
NAMES = ("mhip_contact_op_body_force", "mhip_contact_op_body_force_vector")


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


# ---- 1. the header, the library and the binding table -------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_header_symbols_are_exported_and_bound_and_the_table_names_nothing_else(lib):
    from mundy_amd import capi
    protos = header_prototypes()
    assert set(protos) == set(NAMES) == set(capi.CONTACT_FORCE_SIGNATURES)
    assert not set(capi.CONTACT_FORCE_SIGNATURES) & set(capi.SIGNATURES)
    assert not set(capi.CONTACT_FORCE_SIGNATURES) & set(capi.PERIPHERY_SIGNATURES)
    others = [open(os.path.join(ROOT, "include", h)).read() for h in ("mundy_hip.h", "mundy_hip_hydro_periphery.h")]
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)  # exported
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.CONTACT_FORCE_SIGNATURES[name]) == 6
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
        assert "mhip_stream_t" in args
    text = open(HEADER).read()
    first = text[:text.index("*/")]
    for why in ("test_gpu_streams.py", "test_capi_symbols.py", "test_hydro_periphery_host.py",
                "test_gpu_hydro_periphery_streams.py"):
        assert why in first, "the first comment does not say why the header is its own: %s" % why


# ---- 2. the library's refusals (before any HIP call) ---------------------------------------------------------------------
P = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("kw,match", [
    (dict(h=None), "handle is null"), (dict(h=None, stride=6, acc=1), "handle is null"),
    (dict(stride=4), "stride must be 3 or 6"), (dict(stride=0), "stride must be 3 or 6"),
    (dict(stride=-3), "stride must be 3 or 6"), (dict(stride=9), "stride must be 3 or 6"),
    (dict(acc=2), "accumulate must be 0 or 1"), (dict(acc=-1), "accumulate must be 0 or 1"),
    # what the arguments alone decide is refused with or without a handle
    (dict(h=None, stride=5), "stride must be 3 or 6"), (dict(h=None, acc=7), "accumulate must be 0 or 1")])
def test_library_refuses_before_any_hip_call(lib, name, kw, match):
    from mundy_amd import capi
    a = dict(h=None, stride=3, acc=0)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        capi.check(getattr(lib, name)(a["h"], P, P, a["stride"], a["acc"], None))


# ---- 3. the wrappers' and the stepper's refusals (before the library is loaded) ------------------------------------------
SPRINGS = (np.array([[0, 1], [1, 2], [2, 3]]), "hookean", 10.0, 1.0)


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.full((n,), 0.5, dtype=torch.float64)
    return pipeline.ContactStepper("sphere", c, r, **kw)


def _hy(**kw):
    d = dict(kind="rpyc")
    d.update(kw)
    return d


@pytest.mark.parametrize("kw,match", [
    # the LCP's multipliers do not exist when U_ext is formed
    (dict(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS, contact_model="lcp"), "needs contact_model='hertz'"),
    (dict(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS), "needs contact_model='hertz'"),
    (dict(hydrodynamics=_hy(contact_forces=True), brownian_kt=0.0), "needs contact_model='hertz'"),
    # a bool, nothing else
    (dict(hydrodynamics=_hy(contact_forces=1), springs=SPRINGS, contact_model="hertz"), "contact_forces must be a bool"),
    (dict(hydrodynamics=_hy(contact_forces="yes"), springs=SPRINGS, contact_model="hertz"),
     "contact_forces must be a bool"),
    (dict(hydrodynamics=_hy(contact_forces=None), springs=SPRINGS, contact_model="hertz"),
     "contact_forces must be a bool"),
    (dict(hydrodynamics=_hy(contact_forces=np.bool_(True)), springs=SPRINGS, contact_model="hertz"),
     "contact_forces must be a bool"),
    # not without the chain step, and whatever refuses hydrodynamics refuses it with the key inside
    (dict(hydrodynamics=_hy(contact_forces=True), contact_model="hertz"), "belongs to the chain step"),
    (dict(hydrodynamics=_hy(contact_forces=False), contact_model="hertz"), "belongs to the chain step"),
    (dict(hydrodynamics=_hy(contact_forces=True), contact_model="hertz", brownian_kt=0.0,
          periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(hydrodynamics=_hy(contact_force=True), springs=SPRINGS, contact_model="hertz"), "unknown key")])
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_check_hydrodynamics_learns_the_key_and_returns_what_it_returned():
    from mundy_amd import ops
    assert ops.check_hydrodynamics(dict(kind="rpyc", contact_forces=True), 4) == ("rpyc", None, 1)
    assert ops.check_hydrodynamics(dict(kind="stokes", contact_forces=False, update_every=2), 4) == ("stokes", None, 2)
    with pytest.raises(ValueError, match="contact_forces must be a bool"):
        ops.check_hydrodynamics(dict(kind="rpyc", contact_forces=0), 4)


def test_the_default_is_off_and_the_stage_names_are_in_the_reference_order():
    import inspect

    from mundy_amd import pipeline
    sig = inspect.signature(pipeline.ContactStepper.__init__)
    assert sig.parameters["hydrodynamics"].default is None
    src = inspect.getsource(pipeline.ContactStepper.contact_forces)
    assert src.index('mark("hertz_force")') < src.index('mark("operator")') < src.index('mark("body_force")')
    step = inspect.getsource(pipeline.ContactStepper.step)
    on = step.index("if self.hydro_contact_forces:")
    assert (on < step.index('mark("narrowphase")', on) < step.index("self.contact_forces(", on) <
            step.index("self.external_velocity(", on))


# ---- 4. the model against hand-computed cases ------------------------------------------------------------------------------
def test_model_two_overlapping_spheres():
    pairs = np.array([[0, 1]], dtype=np.int32)
    n = np.array([[1.0, 0.0, 0.0]])
    out = cm.body_force(3, pairs, x=np.array([2.0]), normal=n)
    assert out.shape == (3, 6)
    np.testing.assert_array_equal(out[:, :3], [[-2.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    assert not out[:, 3:].view(np.uint64).any() and not out[2].view(np.uint64).any()  # +0.0, bit for bit
    # the vector form of the same contact: F_c = -(x n) on the source
    vec = cm.body_force(3, pairs, force=-2.0 * n)
    assert np.array_equal(vec.view(np.uint64), out.view(np.uint64))
    # stride 3, accumulate, and a zero multiplier that adds nothing (not even -0.0 onto a -0.0)
    old = np.array([[1.0, -0.0, 3.0], [0.5, 0.5, 0.5], [-0.0, -0.0, -0.0]])
    acc = cm.body_force(3, pairs, x=np.array([2.0]), normal=n, stride=3, old=old)
    np.testing.assert_array_equal(acc, [[-1.0, 0.0, 3.0], [2.5, 0.5, 0.5], [0.0, 0.0, 0.0]])
    none = cm.body_force(3, pairs, x=np.array([0.0]), normal=n, stride=3)
    assert not none.view(np.uint64).any()


def test_model_one_rod_pair_with_a_known_arm():
    # rod 0 along x from (0,0,0) to (2,0,0), touched at its far end (s = 1: arm = (1/2) u = (1,0,0)) by rod 1 at its
    # middle (t = 1/2: no arm); n = +y, x = 3: rod 0 is pushed down at its tip, torque (1,0,0) x (0,-3,0) = (0,0,-3)
    seg = np.array([[0.0, 0.0, 0.0, 2.0, 0.0, 0.0, 0.3, 0.3], [1.0, 1.0, -1.0, 1.0, 1.0, 1.0, 0.3, 0.3]])
    pairs = np.array([[0, 1]], dtype=np.int32)
    n = np.array([[0.0, 1.0, 0.0]])
    out = cm.body_force(2, pairs, x=np.array([3.0]), normal=n, rod=(np.array([1.0]), np.array([0.5]), seg))
    np.testing.assert_array_equal(out[0], [0.0, -3.0, 0.0, 0.0, 0.0, -3.0])
    np.testing.assert_array_equal(out[1], [0.0, 3.0, 0.0, 0.0, 0.0, 0.0])
    # an arclength past the end is clamped to it: the same arm
    out2 = cm.body_force(2, pairs, x=np.array([3.0]), normal=n, rod=(np.array([1.2]), np.array([0.5]), seg))
    np.testing.assert_array_equal(out2, out)
    # the vector-arm form of the same contact: r = (1, 0, 0) on rod 0, 0 on rod 1
    arms = cm.body_force(2, pairs, x=np.array([3.0]), normal=n, ra=np.array([[1.0, 0.0, 0.0]]), rb=np.zeros((1, 3)))
    np.testing.assert_array_equal(arms, out)


def test_model_a_hub_whose_forces_cancel():
    # the hub (body 0, the target of every pair) receives +1e16, +1, -1e16 along x in this order: a plain running sum
    # loses the 1, the correctly rounded sum is exactly 1
    pairs = np.array([[1, 0], [2, 0], [3, 0]], dtype=np.int32)
    n = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]])
    x = np.array([1e16, 1.0, 1e16])
    assert (1e16 + 1.0) - 1e16 == 0.0
    out, mag = cm.body_force(4, pairs, x=x, normal=n, stride=3, want_terms=True)
    np.testing.assert_array_equal(out[0], [1.0, 0.0, 0.0])
    assert mag[0, 0] == 2e16 and mag[0, 0] / abs(out[0, 0]) >= 2.0 ** 25
    np.testing.assert_array_equal(out[1:, 0], [-1e16, -1.0, 1e16])
    # forces that cancel exactly leave +0.0
    out = cm.body_force(4, pairs[[0, 2]], x=x[[0, 2]], normal=n[[0, 2]], stride=3)
    assert not out[0].view(np.uint64).any()


# ---- 5. the C++ side ---------------------------------------------------------------------------------------------------------
def test_hydro_contact_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("hydro_contact_step_app")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 1 and "Usage" in out.stderr and "<E> <nu>" in out.stderr
