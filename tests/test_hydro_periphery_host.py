"""CPU-side checks of the periphery's no-slip correction (include/mundy_hip_hydro_periphery.h): the numpy model
(tests/hydro_periphery_model.py) against quadrature identities, rigid motions, the closed form of a Stokeslet at the
centre of a no-slip sphere and LAPACK's inverse; the new header against the library and its binding table; every
refusal that happens before a HIP call, of the library through ctypes and of the stepper before the library loads.
(The refusals that need a handle -- surface_forces before an inverse, invert without a matrix -- need device memory:
tests/test_gpu_hydro_periphery.py.)"""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import hydro_periphery_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_hydro_periphery.h")
R = 5.0


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
    assert len(protos) == 11
    assert set(protos) == set(capi.PERIPHERY_SIGNATURES)
    assert not set(capi.PERIPHERY_SIGNATURES) & set(capi.SIGNATURES)
    main = open(os.path.join(ROOT, "include", "mundy_hip.h")).read()
    for name, args in protos.items():
        assert name not in main, "%s is declared in mundy_hip.h too" % name
        fn = getattr(lib, name)  # exported
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.PERIPHERY_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
    text = open(HEADER).read()
    assert "test_gpu_streams.py" in text[:1200] and "test_capi_symbols.py" in text[:1200]  # the first comment says why
    for k, v in (("EMPTY", 0), ("MATRIX", 1), ("INVERSE", 2), ("DOUBLE_LAYER", 3)):
        assert "#define MHIP_HYDRO_PERIPHERY_%s %d" % (k, v) in text
        assert getattr(capi, "HYDRO_PERIPHERY_" + k) == v


# ---- 2. the library's refusals (before any HIP call) ---------------------------------------------------------------------
P = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


@pytest.mark.parametrize("kw,match", [
    (dict(out=False), "handle is null"), (dict(S=0), "at least one surface node"), (dict(S=21846), "too many"),
    (dict(pts=None), "null"), (dict(w=None), "null"), (dict(nrm=None), "null"),
    (dict(mu=0.0), "viscosity"), (dict(mu=-1.0), "viscosity"), (dict(mu=math.nan), "viscosity"),
    (dict(mu=math.inf), "viscosity")])
def test_create_refuses_before_any_hip_call(lib, kw, match):
    from mundy_amd import capi
    a = dict(out=True, S=18, pts=P, w=P, nrm=P, mu=1.0)
    a.update(kw)
    h = C.c_void_p()
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_hydro_periphery_create(C.byref(h) if a["out"] else None, a["S"], a["pts"], a["w"], a["nrm"],
                                                   a["mu"], None))
    assert not h.value


def test_null_handles_are_refused(lib):
    from mundy_amd import capi
    x = C.c_double()
    for call in (lambda: lib.mhip_hydro_periphery_fill_matrix(None, None),
                 lambda: lib.mhip_hydro_periphery_fill_double_layer(None, None),
                 lambda: lib.mhip_hydro_periphery_set_matrix(None, P, None),
                 lambda: lib.mhip_hydro_periphery_set_inverse(None, P, None),
                 lambda: lib.mhip_hydro_periphery_invert(None, C.byref(x), None),
                 lambda: lib.mhip_hydro_periphery_matrix(None, None, None),
                 lambda: lib.mhip_hydro_periphery_surface_forces(None, P, P, None),
                 lambda: lib.mhip_hydro_periphery_correct(None, P, 2, 3, P, P, P, P, 3, 1, None)):
        with pytest.raises(ValueError, match="handle"):
            capi.check(call())
    capi.check(lib.mhip_hydro_periphery_destroy(None))  # like delete


@pytest.fixture()
def ws(lib):
    from mundy_amd import capi
    h = C.c_void_p()
    capi.check(lib.mhip_hydro_create(C.byref(h)))
    yield h
    capi.check(lib.mhip_hydro_destroy(h))


def _dl(lib, h, mu=1.0, ns=3, c=P, n=P, w=P, f=P, nt=2, tc=P, vel=P, stride=3, acc=0, skip=1):
    from mundy_amd import capi
    capi.check(lib.mhip_hydro_double_layer(h, mu, ns, c, n, w, f, nt, tc, vel, stride, acc, skip, None))


@pytest.mark.parametrize("kw,match", [
    (dict(mu=0.0), "viscosity"), (dict(mu=-2.0), "viscosity"), (dict(mu=math.nan), "viscosity"),
    (dict(mu=math.inf), "viscosity"), (dict(stride=4), "velocity_stride"), (dict(stride=0), "velocity_stride"),
    (dict(c=None), "null"), (dict(n=None), "null"), (dict(w=None), "null"), (dict(f=None), "null"),
    (dict(tc=None), "null"), (dict(vel=None), "null")])
def test_double_layer_refuses_before_any_hip_call(lib, ws, kw, match):
    with pytest.raises(ValueError, match=match):
        _dl(lib, ws, **kw)


def test_double_layer_null_handle_and_empty_calls(lib, ws):
    with pytest.raises(ValueError, match="handle is null"):
        _dl(lib, None)
    _dl(lib, ws, nt=0, tc=None, vel=None)  # nothing to do: no HIP call
    _dl(lib, ws, ns=0, c=None, n=None, w=None, f=None, acc=1)


# ---- 3. the wrappers' and the stepper's refusals (before the library is loaded) ------------------------------------------
SPRINGS = (np.array([[0, 1], [1, 2], [2, 3]]), "hookean", 10.0, 1.0)
QUAD = pm.sphere_quadrature(2, R, invert=True)


def _pe(**kw):
    d = dict(shape="sphere", radius=R, spectral_order=2)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not ...}


def _arrays(**kw):
    d = dict(points=QUAD[0], weights=QUAD[1], normals=QUAD[2])
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
    return pipeline.ContactStepper(kind, c, r, **extra, **kw)


def _hy(periphery, **kw):
    d = dict(kind="rpyc", periphery=periphery)
    d.update(kw)
    return d


@pytest.mark.parametrize("kw,match", [
    # whatever refuses hydrodynamics refuses it with a periphery inside
    (dict(hydrodynamics=_hy(_pe())), "belongs to the chain step"),
    (dict(kind="spherocylinder", hydrodynamics=_hy(_pe()), springs=SPRINGS), "spheres only"),
    (dict(hydrodynamics=_hy(_pe()), springs=SPRINGS, growth_rate=0.1, division_length=2.0), "growth"),
    (dict(hydrodynamics=_hy(_pe()), brownian_kt=0.0, periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(hydrodynamics=_hy(_pe()), springs=SPRINGS, friction=0.3), "friction"),
    (dict(hydrodynamics=_hy(_pe()), springs=SPRINGS, contact_cutoff=0.1), "contact_cutoff"),
    (dict(hydrodynamics=_hy(_pe(), kind="oseen"), springs=SPRINGS), "kind must be"),
    (dict(hydrodynamics=_hy(_pe(), update_every=0), springs=SPRINGS), "update_every"),
    # the key itself
    (dict(hydrodynamics=_hy("sphere"), springs=SPRINGS), "dict"),
    (dict(hydrodynamics=_hy(_pe(colour=1)), springs=SPRINGS), "unknown key"),
    (dict(hydrodynamics=_hy(_pe(shape="ellipsoid")), springs=SPRINGS), "shape must be 'sphere'"),
    (dict(hydrodynamics=_hy(_pe(radius=...)), springs=SPRINGS), "missing key"),
    (dict(hydrodynamics=_hy(_pe(spectral_order=...)), springs=SPRINGS), "missing key"),
    (dict(hydrodynamics=_hy(_pe(radius=0.0)), springs=SPRINGS), "radius must be finite and > 0"),
    (dict(hydrodynamics=_hy(_pe(radius=-5.0)), springs=SPRINGS), "radius must be finite and > 0"),
    (dict(hydrodynamics=_hy(_pe(radius=math.inf)), springs=SPRINGS), "radius must be finite and > 0"),
    (dict(hydrodynamics=_hy(_pe(radius=math.nan)), springs=SPRINGS), "radius must be finite and > 0"),
    (dict(hydrodynamics=_hy(_pe(spectral_order=0)), springs=SPRINGS), "spectral_order"),
    (dict(hydrodynamics=_hy(_pe(spectral_order=-3)), springs=SPRINGS), "spectral_order"),
    (dict(hydrodynamics=_hy(_pe(spectral_order=2.5)), springs=SPRINGS), "spectral_order"),
    (dict(hydrodynamics=_hy(_pe(spectral_order=200)), springs=SPRINGS), "too many surface nodes"),
    (dict(hydrodynamics=_hy(_pe(points=QUAD[0])), springs=SPRINGS), "not both"),
    (dict(hydrodynamics=_hy(_arrays(weights=...)), springs=SPRINGS), "missing key"),
    (dict(hydrodynamics=_hy(_arrays(radius=R)), springs=SPRINGS), "belongs to shape"),
    (dict(hydrodynamics=_hy(_arrays(points=QUAD[0][:, :2])), springs=SPRINGS), "points must have shape"),
    (dict(hydrodynamics=_hy(_arrays(weights=QUAD[1][:-1])), springs=SPRINGS), "weights / normals must have shapes"),
    (dict(hydrodynamics=_hy(_arrays(normals=QUAD[2][:-1])), springs=SPRINGS), "weights / normals must have shapes"),
    (dict(hydrodynamics=_hy(_arrays(normals=np.full_like(QUAD[2], math.nan))), springs=SPRINGS), "must be finite"),
    (dict(hydrodynamics=_hy(_pe(inverse=np.zeros((5, 5)))), springs=SPRINGS), "inverse must have shape"),
    (dict(hydrodynamics=_hy(_pe(skip_same_index=1)), springs=SPRINGS), "skip_same_index")])
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_check_hydrodynamics_accepts_the_key():
    from mundy_amd import ops
    assert ops.check_hydrodynamics(dict(kind="rpyc", periphery=_pe()), 4) == ("rpyc", None, 1)
    assert ops.check_hydrodynamics(dict(kind="rpyc", periphery=None), 4) == ("rpyc", None, 1)
    got = ops.check_hydro_periphery(_pe(spectral_order=4))
    want = pm.sphere_quadrature(4, R, include_poles=False, invert=True)  # the app's call: no poles, inward normals
    for k, w in zip(("points", "weights", "normals"), want):
        assert np.array_equal(got[k], w)
    assert got["inverse"] is None and got["skip_same_index"] is True
    got = ops.check_hydro_periphery(_arrays(skip_same_index=False, inverse=np.eye(54)))
    assert got["skip_same_index"] is False and got["inverse"].shape == (54, 54)
    assert np.array_equal(got["points"], QUAD[0])


def test_wrapper_refusals(monkeypatch):
    from mundy_amd import capi, ops

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    z3, z1 = torch.zeros((4, 3), dtype=torch.float64), torch.zeros(4, dtype=torch.float64)
    for mu in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="viscosity"):
            ops.hydro_double_layer(mu, z3, z3, z1, z3, z3)
        with pytest.raises(ValueError, match="viscosity"):
            ops.HydroPeriphery(z3, z1, z3, mu)
    with pytest.raises(ValueError, match="normal must have shape"):
        ops.hydro_double_layer(1.0, z3, z3[:2], z1, z3, z3)
    with pytest.raises(ValueError, match="weight must have shape"):
        ops.hydro_double_layer(1.0, z3, z3, z1[:2], z3, z3)
    with pytest.raises(ValueError, match="out must have shape"):
        ops.hydro_double_layer(1.0, z3, z3, z1, z3, z3, out=torch.zeros((4, 4), dtype=torch.float64))
    with pytest.raises(ValueError, match="accumulate needs out"):
        ops.hydro_double_layer(1.0, z3, z3, z1, z3, z3, accumulate=True)
    with pytest.raises(ValueError, match="points must have shape"):
        ops.HydroPeriphery(z3[:0], z1[:0], z3[:0], 1.0)
    with pytest.raises(ValueError, match="weights / normals"):
        ops.HydroPeriphery(z3, z1[:2], z3, 1.0)


# ---- 4. the quadrature ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2, 4, 7, 12, 32])
def test_quadrature(order):
    from mundy_amd import synth
    radius = 2.5
    p, w, n = synth.sphere_quadrature(order, radius, include_poles=False, invert=True)
    S = (order + 1) * (2 * order + 2)
    assert p.shape == (S, 3) and w.shape == (S,) and n.shape == (S, 3)
    for got, want in zip((p, w, n), pm.sphere_quadrature(order, radius, include_poles=False, invert=True)):
        assert np.array_equal(got, want)  # the restatement as the reference's loops are written
    area = 4.0 * math.pi * radius * radius
    assert abs(w.sum() - area) <= 1e-13 * area
    np.testing.assert_allclose((n * n).sum(axis=1), 1.0, rtol=0, atol=4e-16)
    assert ((n * p).sum(axis=1) < 0).all()  # inward
    assert np.array_equal(n * radius, -p) or np.allclose(n * radius, -p, rtol=0, atol=1e-15)
    if order >= 4:  # exact for polynomials of degree <= 2 order + 1 in cos(theta), <= 2 order + 1 in phi
        x, y, z = (p / radius).T
        for f, exact in ((z * z, 4.0 * math.pi / 3.0), (z ** 4, 4.0 * math.pi / 5.0),
                         (x * x * y * y, 4.0 * math.pi / 15.0)):
            got = float((w * f).sum()) / (radius * radius)
            assert abs(got - exact) <= 1e-12 * exact, (order, got, exact)
    # the point order of Periphery.hpp:86-89: rings from the north pole down, 2 order + 2 points around each
    nphi = 2 * order + 2
    rings = p.reshape(order + 1, nphi, 3)
    assert (np.diff(rings[:, 0, 2]) < 0).all() and rings[0, 0, 2] > 0 > rings[-1, 0, 2]
    assert np.ptp(rings[:, :, 2], axis=1).max() == 0.0
    assert (rings[:, 0, 1] == 0.0).all() and (rings[:, 0, 0] > 0).all()  # phi_0 = 0
    phi = np.arctan2(rings[0, :, 1], rings[0, :, 0]) % (2 * math.pi)
    np.testing.assert_allclose(phi, 2 * math.pi * np.arange(nphi) / nphi, rtol=0, atol=1e-14)
    # with the poles: first and last, weight 0, outward normals when not inverted
    pp, wp, npl = synth.sphere_quadrature(order, radius, include_poles=True, invert=False)
    assert pp.shape == (S + 2, 3) and wp[0] == 0.0 and wp[-1] == 0.0
    assert np.array_equal(pp[0], [0.0, 0.0, radius]) and np.array_equal(pp[-1], [0.0, 0.0, -radius])
    assert np.array_equal(pp[1:-1], p) and np.array_equal(npl[1:-1], -n) and np.array_equal(wp[1:-1], w)


# ---- 5. the model's matrix and inverse ---------------------------------------------------------------------------------------
def test_rowsum_is_the_documented_order():
    rng = np.random.default_rng(0)
    for L in (1, 63, 64, 65, 200):
        a = rng.normal(size=(3, L))
        lanes = [np.float64(0.0)] * 64
        for j in range(L):
            lanes[j % 64] = lanes[j % 64] + a[1, j]
        h = 32
        while h:
            lanes = [lanes[i] + lanes[i + h] for i in range(h)]
            h //= 2
        assert pm.rowsum(a)[1] == lanes[0]


def test_fill_is_the_reference_sequence_on_a_small_surface():
    """T, the singularity subtraction and the complementary matrix by scalar loops over the reference's lines"""
    p, w, n = pm.sphere_quadrature(1, R, invert=True)
    S, mu = p.shape[0], 0.8
    T, M = pm.fill_matrix(p, w, n, mu)
    scale = -3.0 / (4.0 * math.pi * mu)
    want = np.zeros((3 * S, 3 * S))
    for t in range(S):
        for s in range(S):
            d = p[t] - p[s]
            r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
            rinv = 0.0 if r2 < 1e-12 else float(pm.hm.quake_inv_sqrt(np.array([r2]))[0])
            rinv5 = rinv * (rinv * rinv) * (rinv * rinv)
            sn = n[s] * w[s]
            rdn = d[0] * sn[0] + d[1] * sn[1] + d[2] * sn[2]
            for i in range(3):
                for j in range(3):
                    want[3 * t + i, 3 * s + j] = d[i] * (scale * rinv5 * rdn * d[j])
    assert np.array_equal(T, want)
    assert (T[np.arange(3 * S), np.arange(3 * S)] == 0.0).all()  # rinv = 0 on the diagonal blocks
    W = np.stack([pm.rowsum(np.ascontiguousarray(want[:, c::3])) for c in range(3)], axis=1)
    for t in range(S):
        want[3 * t:3 * t + 3, 3 * t:3 * t + 3] += W[3 * t:3 * t + 3]
    for t in range(S):
        for s in range(S):
            want[3 * t:3 * t + 3, 3 * s:3 * s + 3] += np.outer(n[t], n[s] * w[s])
    assert np.array_equal(M, want)


RIGID_MEASURED = {"translation": {4: 0.378, 8: 0.178, 12: 0.116}, "rotation": {4: 0.230, 8: 0.112, 12: 0.0741}}


def test_rigid_motions_are_cancelled_inside():
    """u_surf = U or Omega x y on the surface: the correction DL(-(Minv u_surf)) is -(U) or -(Omega x x) inside, to the
    discretisation error of the order.  The singularity-subtracted rule is first order in the mesh width ~ 1 / (p + 1),
    and that is what the model shows (largest component of the error over the largest of the flow on the surface, 40
    seeded targets with |x| <= 0.6 R):
        translation  order 4: 0.378   8: 0.178   12: 0.116          rotation  order 4: 0.230   8: 0.112   12: 0.0741
    Asserted: at least first-order decrease between the orders, and each figure within 1.5 x of the measured one (the
    margin is for the seed).  (The Stokeslet of the next test is cancelled far better at the same order: its surface
    velocity is small where the rule is worst.)"""
    rng = np.random.default_rng(1)
    v = rng.normal(size=(40, 3))
    x = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.6 * R * rng.uniform(0, 1, 40) ** (1 / 3))[:, None]
    U, Om = np.array([0.4, -0.2, 0.9]), np.array([-0.3, 0.5, 0.1])
    flows = {"translation": lambda y: np.tile(U, (y.shape[0], 1)), "rotation": lambda y: np.cross(Om, y)}
    errs = {name: {} for name in flows}
    for order in (4, 8, 12):
        p, w, n = pm.sphere_quadrature(order, R, invert=True)
        Minv = np.linalg.inv(pm.fill_matrix(p, w, n, 1.0)[1])
        for name, flow in flows.items():
            f = pm.surface_forces(Minv, flow(p)).reshape(-1, 3)
            got = pm.double_layer(1.0, p, n, w, f, x, skip_same_index=False)
            errs[name][order] = float(np.abs(got + flow(x)).max() / np.abs(flow(p)).max())
            print(name, "order", order, "relative error %.4f" % errs[name][order])
    for name, e in errs.items():
        assert e[8] <= e[4] * 5.0 / 9.0 and e[12] <= e[8] * 9.0 / 13.0, (name, e)
        for order in e:
            assert e[order] <= 1.5 * RIGID_MEASURED[name][order], (name, order, e[order])


STOKESLET_MEASURED = {8: 0.0340, 12: 0.0177, 16: 0.0135}


def test_centred_stokeslet_closed_form():
    """The correction of a Stokeslet F at the centre of a no-slip sphere, c [-3 F / R + (2 |x|^2 F - (F.x) x) / R^3]
    with c = 1 / (8 pi mu), at 40 seeded targets with |x| <= 0.6 R, the algorithm as coded (RPYC with zero radii onto
    the nodes, skip_same_index on).  Measured with this model, relative to the largest closed-form component:
        order 8: 0.03403   order 12: 0.01767   order 16: 0.01345     (skip_same_index off: 0.02734, 0.01790, 0.01333;
        order 4: 0.179 with the skip, 0.0599 without)
    Each must stay below 1.5 x that figure (the margin is for the seed: the model is deterministic), and the error must
    decrease with the order.  The inverse is numpy.linalg.inv here (the elimination of the model in numpy takes 15 s at
    order 16; the two inverses differ by 1e-13, test_gauss_jordan_against_lapack)."""
    errs = {}
    for order in (8, 12, 16):
        errs[order] = pm.centred_stokeslet_error(order, R=R, skip_same_index=True, lapack=True)
        print("order %d: relative error %.5f (measured %.4f)" % (order, errs[order], STOKESLET_MEASURED[order]))
    assert errs[8] > errs[12] > errs[16]
    for order, e in errs.items():
        assert e <= 1.5 * STOKESLET_MEASURED[order], (order, e)


def test_model_elimination_carries_the_closed_form_at_order_8():
    """the same figure through the model's own Gauss-Jordan inverse (what the device reproduces bit for bit)"""
    e = pm.centred_stokeslet_error(8, R=R, skip_same_index=True, lapack=False)
    print("order 8, Gauss-Jordan inverse: %.5f" % e)
    assert e <= 1.5 * STOKESLET_MEASURED[8]


@pytest.mark.parametrize("order", [2, 4, 7])
def test_gauss_jordan_against_lapack(order):
    p, w, n = pm.sphere_quadrature(order, R, invert=True)
    _, M = pm.fill_matrix(p, w, n, 1.0)
    N = M.shape[0]
    inv, min_pivot, _ = pm.gauss_jordan(M)
    ref = np.linalg.inv(M)
    I = np.eye(N)
    res, res_ref = np.abs(M @ inv - I).max(), np.abs(M @ ref - I).max()
    print("order %d (N = %d): cond %.0f, max|M Minv - I| %.3g (LAPACK %.3g), min pivot %.3g" % (
        order, N, np.linalg.cond(M), res, res_ref, min_pivot))
    assert res <= 10.0 * res_ref
    assert min_pivot > 0.0


def test_gauss_jordan_pivots():
    rng = np.random.default_rng(7)
    A = rng.normal(size=(66, 66))
    np.fill_diagonal(A, 0.0)
    inv, min_pivot, swaps = pm.gauss_jordan(A)
    print("66 x 66, zero diagonal: %d row swaps" % swaps)
    assert swaps >= 1
    ref = np.linalg.inv(A)
    I = np.eye(66)
    assert np.abs(A @ inv - I).max() <= 10.0 * np.abs(A @ ref - I).max()
    # a tie takes the lowest row; a permutation comes back exactly
    Pm = np.eye(5)[[2, 0, 3, 1, 4]]
    got, mp, sw = pm.gauss_jordan(Pm)
    assert np.array_equal(got, Pm.T) and mp == 1.0 and sw > 0
    tie = np.array([[1.0, 2.0], [-1.0, 1.0]])
    assert np.allclose(pm.gauss_jordan(tie)[0], np.linalg.inv(tie), rtol=1e-15) and pm.gauss_jordan(tie)[2] == 0
    with pytest.raises(pm.SingularMatrix):
        pm.gauss_jordan(np.array([[1.0, 2.0], [2.0, 4.0]]))
    with pytest.raises(pm.SingularMatrix):
        pm.gauss_jordan(np.array([[1.0, math.nan], [2.0, 4.0]]))


# ---- 6. the C++ driver ----------------------------------------------------------------------------------------------------------
def test_hydro_periphery_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("hydro_periphery_step_app")
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 1 and "Usage" in out.stderr
