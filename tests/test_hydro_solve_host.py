"""CPU-side checks of the LCP against a hydrodynamic mobility (include/mundy_hip_hydro_solve.h): the new header against
the library and its binding table; every refusal the library makes from its arguments alone, through ctypes, before any
HIP call (the refusals that need an operator handle -- lever arms, a body count, a space -- need device memory:
tests/test_gpu_hydro_solve.py, with those of a staged solve in progress and of a partitioned operator, and the C++
stepper's through tests/cpp/hydro_solve_step_app); the wrappers' and the stepper's refusals with the loader disabled; the model
(tests/hydro_solve_model.py) against hydro_model, against the two closed forms, and its convergence on exactly the inputs
the GPU tests use."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hydro_model as hm
import hydro_solve_model as hsm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_hydro_solve.h")
NAMES = ("mhip_hydro_set_sparse_sources", "mhip_contact_op_apply_hydro", "mhip_bbpgd_solve_contact_hydro")


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
    assert set(protos) == set(NAMES) == set(capi.HYDRO_SOLVE_SIGNATURES)
    tables = (capi.SIGNATURES, capi.PERIPHERY_SIGNATURES, capi.CONTACT_FORCE_SIGNATURES,
              capi.PERIPHERY_BINDING_SIGNATURES, capi.SEGMENT_CONTACT_SIGNATURES)
    for other in tables:
        assert not set(capi.HYDRO_SOLVE_SIGNATURES) & set(other)
    inc = os.path.join(ROOT, "include")
    others = [open(os.path.join(inc, h)).read() for h in sorted(os.listdir(inc))
              if h.endswith(".h") and h != "mundy_hip_hydro_solve.h"]
    assert len(others) >= 5
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)  # exported
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.HYDRO_SOLVE_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
    assert sorted(n for n, a in protos.items() if "mhip_stream_t" in a) == sorted(NAMES[1:])
    text = open(HEADER).read()
    first = text[:text.index("*/")]
    for cite in ("NgpHP1.cpp:1487-1645", ":677-701", ":833-925", ":703-766", ":927-1023", "convex.hpp:592-681",
                 "test_gpu_streams.py", "test_capi_symbols.py"):
        assert cite in first, "the header's comment does not cite %s" % cite


def test_the_struct_has_the_headers_fields_in_the_headers_order():
    from mundy_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct mhip_hydro_mobility \{(.*?)\} mhip_hydro_mobility;", text, flags=re.S).group(1)
    fields = [re.split(r"[\s*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
    assert fields == [f[0] for f in capi.HydroMobility._fields_]
    assert fields == ["workspace", "kind", "viscosity", "n", "center", "radius", "periphery", "skip_same_index"]
    assert C.sizeof(capi.HydroMobility) == 64   # pointer, int + pad, double, size_t, three pointers, int + pad


# ---- 2. the library's refusals (before any HIP call) ---------------------------------------------------------------------
P = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


def _mob(**kw):
    from mundy_amd import capi
    m = capi.HydroMobility(64, capi.HYDRO_RPYC, 1.0, 4, 64, 64, None, 1)
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def _call(lib, name, op, mob):
    from mundy_amd import capi
    mp = None if mob is None else C.byref(mob)
    if name == "mhip_contact_op_apply_hydro":
        return lib.mhip_contact_op_apply_hydro(op, mp, P, P, None)
    res, sp, pc = capi.SolveResult(), capi.Space(capi.SPACE_LOWER_BOUND, 0.0, 0.0), capi.PgdConfig(10, 1e-8, 0)
    return lib.mhip_bbpgd_solve_contact_hydro(op, mp, P, C.byref(sp), C.byref(pc), P, P, P, P, C.byref(res), None)


@pytest.mark.parametrize("name", NAMES[1:])
def test_library_refuses_null_handles_and_structs_before_any_hip_call(lib, name):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="operator handle is null"):
        capi.check(_call(lib, name, None, _mob()))
    with pytest.raises(ValueError, match="operator handle is null"):
        capi.check(_call(lib, name, None, None))
    with pytest.raises(ValueError, match="operator handle is null"):
        capi.check(_call(lib, name, None, _mob(kind=capi.HYDRO_STOKES, viscosity=-1.0)))


def test_solve_refuses_a_null_result_and_sparse_sources_a_null_handle(lib):
    from mundy_amd import capi
    sp, pc = capi.Space(capi.SPACE_LOWER_BOUND, 0.0, 0.0), capi.PgdConfig(10, 1e-8, 0)
    with pytest.raises(ValueError, match="result"):
        capi.check(lib.mhip_bbpgd_solve_contact_hydro(None, C.byref(_mob()), P, C.byref(sp), C.byref(pc), P, P, P, P,
                                                      None, None))
    with pytest.raises(ValueError, match="hydro handle is null"):
        capi.check(lib.mhip_hydro_set_sparse_sources(None, 1))
    h = C.c_void_p()
    capi.check(lib.mhip_hydro_create(C.byref(h)))
    try:
        for bad in (2, -1):
            with pytest.raises(ValueError, match="must be 0 or 1"):
                capi.check(lib.mhip_hydro_set_sparse_sources(h, bad))
        capi.check(lib.mhip_hydro_set_sparse_sources(h, 1))
        capi.check(lib.mhip_hydro_set_sparse_sources(h, 0))
    finally:
        capi.check(lib.mhip_hydro_destroy(h))


# ---- 3. the wrappers' and the stepper's refusals (before the library is loaded) ------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)


def _cpu(n=4):
    return torch.zeros((n, 3), dtype=torch.float64), torch.full((n,), 0.5, dtype=torch.float64)


@pytest.mark.parametrize("kw,match", [
    (dict(kind="stokes"), "Stokeslet"), (dict(kind="oseen"), "kind must be"),
    (dict(viscosity=0.0), "viscosity"), (dict(viscosity=-1.0), "viscosity"), (dict(viscosity=float("inf")), "viscosity"),
    (dict(viscosity=float("nan")), "viscosity"),
    (dict(center=torch.zeros((4, 2), dtype=torch.float64)), "center must have shape"),
    (dict(radius=torch.zeros(5, dtype=torch.float64)), "radius must have shape"),
    (dict(periphery="sphere"), "HydroPeriphery"), (dict(skip_same_index=1), "skip_same_index must be a bool"),
    (dict(workspace=7), "HydroWorkspace"),
    (dict(), "must live on the GPU")])   # (what is left for a host tensor once everything else is in order)
def test_hydro_mobility_refuses_without_loading_the_library(no_library, kw, match):
    from mundy_amd import ops
    center, radius = _cpu()
    a = dict(kind="rpyc", viscosity=1.0, center=center, radius=radius)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        ops.HydroMobility(**a)


def test_hydro_mobility_refuses_a_periphery_of_another_viscosity(no_library):
    from mundy_amd import ops
    center, radius = _cpu()
    P = object.__new__(ops.HydroPeriphery)   # (no device: only its viscosity is read before the refusal)
    P.viscosity = 2.0
    with pytest.raises(ValueError, match="built with viscosity 2.0, the mobility has 1.0"):
        ops.HydroMobility("rpyc", 1.0, center, radius, periphery=P)
    P.viscosity = 1.0
    with pytest.raises(ValueError, match="must live on the GPU"):
        ops.HydroMobility("rpyc", 1.0, center, radius, periphery=P)


def test_solvers_refuse_what_is_not_a_mobility_or_not_an_lcp(no_library):
    from mundy_amd import ops
    q = torch.zeros(3, dtype=torch.float64)
    mob = object.__new__(ops.HydroMobility)   # (no device: the checks under test come before its fields are read)
    with pytest.raises(ValueError, match="must be a HydroMobility"):
        ops.solve_lcp(None, q, q, mobility="rpyc")
    with pytest.raises(ValueError, match="needs a ContactOperator"):
        ops.solve_lcp(torch.zeros((3, 3), dtype=torch.float64), q, q, mobility=mob)
    op = object.__new__(ops.ContactOperator)
    with pytest.raises(ValueError, match="fused driver only"):
        ops.solve_lcp(op, q, q, mobility=mob, fused=False)
    for space in ((ops.SPACE_UNCONSTRAINED, 0.0, 0.0), (ops.SPACE_LOWER_BOUND, 1.0, 0.0), (ops.SPACE_BOUNDED, 0.0, 1.0)):
        with pytest.raises(ValueError, match="LowerBound"):
            ops.solve_cqpp(op, q, space, q, mobility=mob)
    # the pair (operator, mobility)
    op.num_bodies, mob.num_bodies = 4, 4
    for keep in ((None, None, q, None, None, None, None, None), (None, None, None, None, None, q, None, None),
                 (None, None, None, None, None, None, (q, q, q), None)):
        op._keep = keep
        with pytest.raises(ValueError, match="sphere operator"):
            ops.solve_lcp(op, q, q, mobility=mob)
        with pytest.raises(ValueError, match="sphere operator"):
            mob.check_operator(op)
    op._keep, mob.num_bodies = (None,) * 8, 5
    op.num_constraints = 3
    with pytest.raises(ValueError, match="5 bodies, the operator 4"):
        ops.ContactOperator.apply_hydro(op, mob, q)
    with pytest.raises(ValueError, match="must be a HydroMobility"):
        ops.ContactOperator.apply_hydro(op, None, q)
    with pytest.raises(ValueError, match="on must be a bool"):
        ops.HydroWorkspace.set_sparse_sources(object.__new__(ops.HydroWorkspace), 1)


SPRINGS = (np.array([[0, 1], [1, 2], [2, 3]]), "hookean", 10.0, 1.0)


def _stepper(**kw):
    from mundy_amd import pipeline
    center, radius = _cpu()
    return pipeline.ContactStepper("sphere", center, radius, **kw)


def _hy(**kw):
    d = dict(kind="rpyc", in_solve=True)
    d.update(kw)
    return d


@pytest.mark.parametrize("kw,match", [
    (dict(hydrodynamics=_hy(in_solve=1), springs=SPRINGS), "in_solve must be a bool"),
    (dict(hydrodynamics=_hy(in_solve="yes"), springs=SPRINGS), "in_solve must be a bool"),
    (dict(hydrodynamics=_hy(in_solve=None), springs=SPRINGS), "in_solve must be a bool"),
    (dict(hydrodynamics=_hy(in_solve=np.bool_(True)), springs=SPRINGS), "in_solve must be a bool"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, contact_model="hertz"), "in_solve needs contact_model='lcp'"),
    (dict(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS, contact_model="hertz"),
     "in_solve needs contact_model='lcp'"),
    # (the existing refusal and its message come first, exactly as they are)
    (dict(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS), "needs contact_model='hertz'"),
    (dict(hydrodynamics=_hy(kind="stokes"), springs=SPRINGS), "in_solve needs kind 'rpyc' or 'rpy'"),
    # refusals that hydrodynamics= had before the key existed and that stand in front of it: they pass without the key
    # too, and are here to show that the key does not open a way round them
    (dict(hydrodynamics=_hy(), springs=SPRINGS, friction=0.3), "friction"),
    (dict(hydrodynamics=_hy(), springs=SPRINGS, contact_cutoff=0.1), "contact_cutoff"),
    (dict(hydrodynamics=_hy()), "belongs to the chain step"),
    (dict(hydrodynamics=_hy(in_solves=True), springs=SPRINGS), "unknown key")])
def test_stepper_refuses_without_loading_the_library(no_library, kw, match):
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_in_solve_with_contact_forces_is_refused_whatever_the_contact_model(no_library):
    # with "lcp" the older refusal of contact_forces fires, message unchanged; with "hertz" the new one of the contact
    # model: no third check is needed, and there is none
    with pytest.raises(ValueError, match="contact_forces needs contact_model='hertz': the LCP's multipliers do not"):
        _stepper(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS, contact_model="lcp")
    with pytest.raises(ValueError, match="in_solve needs contact_model='lcp'"):
        _stepper(hydrodynamics=_hy(contact_forces=True), springs=SPRINGS, contact_model="hertz")


def test_check_hydrodynamics_learns_the_key_and_returns_what_it_returned():
    from mundy_amd import ops
    assert ops.check_hydrodynamics(dict(kind="rpyc", in_solve=True), 4) == ("rpyc", None, 1)
    assert ops.check_hydrodynamics(dict(kind="rpy", in_solve=False, update_every=2), 4) == ("rpy", None, 2)
    assert ops.check_hydrodynamics(dict(kind="stokes", in_solve=True, contact_forces=False), 4) == ("stokes", None, 1)
    with pytest.raises(ValueError, match="in_solve must be a bool"):
        ops.check_hydrodynamics(dict(kind="rpyc", in_solve=0), 4)
    with pytest.raises(ValueError, match="contact_forces must be a bool"):
        ops.check_hydrodynamics(dict(kind="rpyc", contact_forces=0), 4)


# ---- 4. the model ------------------------------------------------------------------------------------------------------------
def test_cached_pair_geometry_is_hydro_models_velocity_bit_for_bit():
    for name in ("n300", "poly", "n3", "n2"):
        c = hsm.case_of(name)
        rng = np.random.default_rng(2)
        F = rng.normal(size=(c["n"], 3))
        F[rng.random(c["n"]) < 0.4] = 0.0
        old = rng.normal(size=(c["n"], 3))
        got = hsm.RpycGeometry(c["viscosity"], c["center"], c["hydro_radius"]).velocity(F, old=old)
        want = hm.velocity("rpyc", c["viscosity"], c["center"], c["hydro_radius"], F, old=old)
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), name
    # a polydisperse cloud with every RPYC branch, coincident centres among them
    d = hm.inputs(300, seed=4)
    br = hm.rpyc_branch(d["sc"][:, None, :] - d["sc"][None, :, :], d["sa"][None, :], d["sa"][:, None])
    assert all((br == k).any() for k in (hm.FAR, hm.OVERLAP, hm.LOCAL, hm.SKIPPED))
    got = hsm.RpycGeometry(1.3, d["sc"], d["sa"]).velocity(d["f"])
    want = hm.velocity("rpyc", 1.3, d["sc"], d["sa"], d["f"])
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("name", hsm.CASE_NAMES)
def test_model_converges_on_the_inputs_of_the_gpu_tests(name):
    c = hsm.case_of(name)
    nc = len(c["q"])
    s = hsm.solve(hsm.Operator(c), c["q"], np.zeros(nc), max_iters=1000, tol=1e-8)
    print("%s: n = %d, %d contacts (%d overlapping), %d iterations, residual %.3g" % (
        name, c["n"], nc, int((c["q"] < 0).sum()), s["num_iters"], s["residual"]))
    assert s["converged"] and s["num_iters"] < 1000
    assert (s["x"] >= 0.0).all()
    if name == "main":
        assert c["n"] == 1100 and nc == 2758 and 850 <= int((c["q"] < 0).sum()) <= 910
        assert 40 <= s["num_iters"] <= 150   # (a dense-matrix BBPGD: 74)
    if name == "c0":
        assert nc == 0 and s["num_iters"] == 0
    if name == "lonely":
        touched = np.zeros(c["n"], dtype=bool)
        touched[c["pairs"].reshape(-1)] = True
        assert not touched[c["n"] // 2:].any() and touched[:c["n"] // 2].any()
    if name == "poly":
        assert np.abs(c["hydro_radius"] - c["radius"]).min() > 0.0


def test_model_dry_limit_is_the_dry_operator():
    c = hsm.case_of("n300")
    x = np.random.default_rng(1).uniform(0.0, 1.0, len(c["q"]))
    wet = hsm.Operator(c, viscosity=1e200).apply(x)
    dry = hsm.Operator(c, kind=None).apply(x)
    assert np.array_equal(wet.view(np.uint64), dry.view(np.uint64))


@pytest.mark.parametrize("branch,r,a,bead", (("overlap", 0.9, 0.5, 0.5), ("far", 1.2, 0.5, 0.65)))
def test_model_has_the_closed_form_multiplier_of_two_equal_beads(branch, r, a, bead):
    c = hsm.two_beads(r, a, bead, 0.1)
    assert abs(c["q"][0] + 0.1) < 1e-15
    want = hsm.closed_form_lambda(r, a, 0.1, c["dt"], c["viscosity"], branch)
    wet = hsm.solve(hsm.Operator(c), c["q"], np.zeros(1), tol=1e-10)
    dry = hsm.solve(hsm.Operator(c, kind=None), c["q"], np.zeros(1), tol=1e-10)
    assert wet["converged"] and dry["converged"]
    assert abs(wet["x"][0] - want) <= 1e-12 * want
    assert wet["x"][0] > dry["x"][0]
    assert abs(dry["x"][0] - 47.1238898038469) < 1e-9
    if branch == "overlap":
        assert abs(want - 139.626) < 1e-3


def test_model_trap_an_inactive_contact_and_a_lone_bead_feel_the_active_pair():
    c = hsm.case_of("trap")
    wet = hsm.solve(hsm.Operator(c), c["q"], np.zeros(2))
    dry = hsm.solve(hsm.Operator(c, kind=None), c["q"], np.zeros(2))
    assert wet["x"][1] == 0.0 and dry["x"][1] == 0.0 and wet["x"][0] > dry["x"][0] > 0.0
    assert dry["g"][1] == c["q"][1] and not dry["rows"][4].any()
    assert wet["g"][1] != c["q"][1] and wet["g"][1] > 0.0 and np.abs(wet["rows"][4, :3]).max() > 0.0


# ---- 5. the C++ side ---------------------------------------------------------------------------------------------------------
def test_hydro_solve_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("hydro_solve_step_app")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 1 and "Usage" in out.stderr and "<in_solve> <max_iters> <tol>" in out.stderr
