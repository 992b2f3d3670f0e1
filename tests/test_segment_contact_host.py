"""CPU-side checks of the backbone segment contacts (include/mundy_hip_segment_contact.h): the numpy model
(segment_contact_model.py) against closed forms, the conditions of the three GPU cases from the model alone, the header
against the binding table and the library, every refusal with the library loader disabled and the library's own before
any HIP call, the stepper's refusals, the C++ app.

The three cases (r = 0.5, skin = 0.3, the default WCA parameters), as segment_contact_model.case builds them:
  case               nodes / segments   linkers Hertz / WCA   in the force branch Hertz / WCA
  jittered_lattice   640 / 624          8530 / 9426           3332 / 3352     22 interior-interior in the branch
  exact_lattice      270 / 261          3023 / 3023           1263 / 1263     every linker colinear
  random_walks       720 / 696          21964 / 25386         4573 / 5840     623 / 698 interior-interior in the branch
"""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import segment_contact_model as scm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_segment_contact.h")
NAMES = ("mhip_segment_contacts_create", "mhip_segment_contacts_destroy", "mhip_segment_contacts_update",
         "mhip_segment_contacts_force", "mhip_segment_contacts_linker_pass", "mhip_segment_contacts_reduce",
         "mhip_segment_contacts_get")
K_BLOCK = 256
E, NU = 1000.0, 0.3


def hertz_spheres(r, L):
    """the Hertz force of two spheres of radius r whose centres are L apart"""
    Es = (E * E) / (E - E * NU * NU + E - E * NU * NU)
    return (4.0 / 3.0) * Es * math.sqrt(r * r / (r + r)) * (2.0 * r - L) ** 1.5


# ---- 1. the model against closed forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hertz", "wca"])
def test_two_crossed_segments(kind):
    d, r = 0.8, 0.5
    x = np.array([[-1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.3, -1.0, d], [0.3, 2.0, d]])
    mod = scm.SegmentContacts(4, [[0, 1], [2, 3]], kind, r, 0.3, end_correction=False)
    assert mod.update(x) and mod.pairs.tolist() == [[0, 1]]
    f, stats = mod.force_pass(x)
    want = hertz_spheres(r, d) if kind == "hertz" else 24.0 * (2.0 / d ** 12 - 1.0 / d ** 6) / d
    assert mod.dist[0] == d and abs(mod.sep[0] - (d - 1.0)) < 1e-16
    np.testing.assert_allclose(mod.force[0], [0.0, 0.0, -want], rtol=1e-14, atol=1e-14 * want)
    assert stats == (1.0 - mod.dist[0], 1)
    # the two end nodes of a segment share its force: the shares sum to Fs, by the lever rule of the closest point
    np.testing.assert_allclose(f[0] + f[1], mod.force[0], rtol=1e-14)
    np.testing.assert_allclose(f[2] + f[3], -mod.force[0], rtol=1e-14)
    np.testing.assert_allclose(f[1, 2] / (f[0, 2] + f[1, 2]), 1.3 / 2.0, rtol=1e-14)   # cp at x = 0.3 of [-1, 1]
    np.testing.assert_allclose(f[3, 2] / (f[2, 2] + f[3, 2]), 1.0 / 3.0, rtol=1e-14)   # cp at y = 0 of [-1, 2]
    assert np.abs(f.sum(axis=0)).max() <= 1e-14 * want


def test_shrinking_middle_segment_and_the_end_correction():
    # three segments in a row (HP1.cpp:4369-4372): the outer two share no node and collide through the middle one when
    # it shrinks below 2 r; a chain's first and last segment lack that neighbour on one side, and the correction is
    # the Hertz force of two spheres at the segment's own length
    r, L = 0.5, 0.9
    x = np.array([[0.0, 0, 0], [L, 0, 0], [2 * L, 0, 0], [3 * L, 0, 0]])
    ends = [[0, 1], [1, 2], [2, 3]]
    plain = scm.SegmentContacts(4, ends, "hertz", r, 0.3, end_correction=False)
    plain.update(x)
    f0, _ = plain.force_pass(x)
    assert plain.pairs.tolist() == [[0, 2]]
    fm = hertz_spheres(r, L)
    np.testing.assert_allclose(f0[:, 0], [0.0, -fm, fm, 0.0], rtol=1e-13, atol=1e-13 * fm)
    corr = scm.SegmentContacts(4, ends, "hertz", r, 0.3)
    assert corr.corr.tolist() == [True, False, True]
    corr.update(x)
    f1, stats = corr.force_pass(x)
    np.testing.assert_allclose((f1 - f0)[:, 0], [-fm, fm, -fm, fm], rtol=1e-13, atol=1e-13 * fm)
    assert (f1[:, 1:] == 0.0).all() and abs(stats[0] - (2 * r - L)) < 1e-15 and stats[1] == 1
    # a segment longer than 2 r is not corrected
    far = scm.SegmentContacts(4, ends, "hertz", r, 0.3)
    far.update(x * 1.2)
    assert (far.force_pass(x * 1.2)[0] == 0.0).all()


def test_wca_vanishes_at_its_minimum():
    sigma, eps = 1.0, 1.0
    d = 2.0 ** (1.0 / 6.0) * sigma
    assert abs(scm.wca_magnitude(eps, sigma, np.array([d]))[0]) <= 1e-15 * 24.0 * eps / sigma
    assert scm.wca_magnitude(eps, sigma, np.array([0.99 * d]))[0] > 0.0


def test_y_connectivity_excludes_every_pair_that_shares_the_node():
    x = np.array([[0.0, 0, 0], [1.0, 0, 0], [-0.5, 0.8, 0], [-0.5, -0.8, 0], [0.2, 0.1, 0.4], [0.9, 0.2, 0.5]])
    ends = np.array([[0, 1], [0, 2], [0, 3], [4, 5]])
    mod = scm.SegmentContacts(6, ends, "hertz", 0.5, 0.3)
    mod.update(x)
    assert mod.pairs.tolist() == [[0, 3], [1, 3], [2, 3]]
    assert mod.corr.tolist() == [True, True, True, True]


# ---- 2. the three cases meet the conditions the GPU tests rely on ---------------------------------------------------------
@pytest.mark.parametrize("kind", ["hertz", "wca"])
def test_cases_meet_their_conditions(kind):
    seen = np.zeros(3, bool)
    for name in scm.CASES:
        cs, mod = scm.case(name), scm.evaluated(name, kind)
        forms = mod.forms()
        print(name, kind, cs["n"], cs["m"], mod.pairs.shape[0], int(mod.in_branch.sum()),
              [int((f & mod.in_branch).sum()) for f in forms], mod.dist.min())
        assert mod.pairs.shape[0] > K_BLOCK and cs["n"] > K_BLOCK and mod.in_branch.sum() > K_BLOCK
        assert (mod.dist > 0.0).all()
        assert (np.diff(mod.pairs[:, 0].astype(np.int64) * cs["m"] + mod.pairs[:, 1]) > 0).all()
        seen |= [bool((f & mod.in_branch).any()) for f in forms]
    assert seen.all(), "interior-interior, end-node, colinear: %s" % seen
    assert scm.evaluated("exact_lattice", kind).forms()[2].all()


# ---- 3. the library: header, table, refusals before any HIP call ----------------------------------------------------------
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
    assert set(protos) == set(NAMES) == set(capi.SEGMENT_CONTACT_SIGNATURES)
    for other in (capi.SIGNATURES, capi.PERIPHERY_SIGNATURES, capi.CONTACT_FORCE_SIGNATURES,
                  capi.PERIPHERY_BINDING_SIGNATURES):
        assert not set(capi.SEGMENT_CONTACT_SIGNATURES) & set(other)
    others = [open(os.path.join(ROOT, "include", h)).read()
              for h in ("mundy_hip.h", "mundy_hip_hydro_periphery.h", "mundy_hip_contact_force.h",
                        "mundy_hip_periphery_binding.h")]
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.SEGMENT_CONTACT_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
        assert ("mhip_stream_t" in args) == (name not in ("mhip_segment_contacts_destroy", "mhip_segment_contacts_get"))
    text = open(HEADER).read()
    assert capi.SEGMENT_CONTACT_HERTZ == int(re.search(r"#define MHIP_SEGMENT_CONTACT_HERTZ (\d+)", text).group(1))
    assert capi.SEGMENT_CONTACT_WCA == int(re.search(r"#define MHIP_SEGMENT_CONTACT_WCA (\d+)", text).group(1))
    assert C.sizeof(capi.SegmentContactParams) == 56 and C.sizeof(capi.SegmentContactFields) == 72


Q = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


def _create(lib, n=4, ends=((0, 1), (2, 3)), radius=None, r0=0.5, corr=None, null_params=False, null_handle=False,
            null_ends=False, **prm):
    from mundy_amd import capi
    p = dict(kind=0, skin=0.3, youngs_modulus=E, poisson_ratio=NU, epsilon=1.0, sigma=1.0, cutoff=1.12)
    p.update(prm)
    params = capi.SegmentContactParams(*[p[k] for k in ("kind", "skin", "youngs_modulus", "poisson_ratio", "epsilon",
                                                         "sigma", "cutoff")])
    e = np.ascontiguousarray(ends, dtype=np.int32).reshape(-1, 2)
    ra = None if radius is None else np.ascontiguousarray(radius, dtype=np.float64)
    h = C.c_void_p()
    capi.check(lib.mhip_segment_contacts_create(
        None if null_handle else C.byref(h), n, e.shape[0], None if null_ends else e.ctypes.data_as(C.c_void_p),
        None if ra is None else ra.ctypes.data_as(C.c_void_p), r0, None, None if null_params else C.byref(params), None))
    return h


REFUSED = [
    (dict(null_handle=True), "handle is null"), (dict(null_ends=True), "ends is null"),
    (dict(null_params=True), "params is null"),
    (dict(ends=((0, 4), (2, 3))), "outside"), (dict(ends=((0, 1), (-1, 3))), "outside"),
    (dict(ends=((0, 1), (2, 2))), "to itself"),
    (dict(r0=0.0), "radius"), (dict(r0=-1.0), "radius"), (dict(r0=math.nan), "radius"), (dict(r0=math.inf), "radius"),
    (dict(radius=[0.5, 0.0]), "radius"), (dict(radius=[math.nan, 0.5]), "radius"),
    (dict(skin=-0.1), "skin"), (dict(skin=math.nan), "skin"), (dict(skin=math.inf), "skin"),
    (dict(youngs_modulus=0.0), "youngs_modulus"), (dict(youngs_modulus=math.inf), "youngs_modulus"),
    (dict(youngs_modulus=math.nan), "youngs_modulus"),
    (dict(poisson_ratio=0.0), "poisson_ratio"), (dict(poisson_ratio=1.0), "poisson_ratio"),
    (dict(poisson_ratio=math.nan), "poisson_ratio"),
    (dict(kind=1, epsilon=-1.0), "epsilon"), (dict(kind=1, epsilon=math.nan), "epsilon"),
    (dict(kind=1, sigma=0.0), "sigma"), (dict(kind=1, sigma=math.inf), "sigma"),
    (dict(kind=1, cutoff=0.0), "cutoff"), (dict(kind=1, cutoff=math.nan), "cutoff"),
    (dict(kind=2), "unknown segment contact kind"), (dict(kind=-1), "unknown segment contact kind"),
]


@pytest.mark.parametrize("kw,match", REFUSED)
def test_create_refuses_before_any_hip_call(lib, kw, match):
    # (this machine may have no device: a refusal that came after a HIP call would be a MhipError, not a ValueError)
    with pytest.raises(ValueError, match=match):
        _create(lib, **kw)


def test_null_handles_are_refused(lib):
    from mundy_amd import capi
    flag = C.c_int(0)
    fields = capi.SegmentContactFields()
    for call in (lambda: lib.mhip_segment_contacts_update(None, Q, 0, C.byref(flag), None),
                 lambda: lib.mhip_segment_contacts_force(None, Q, Q, 0, Q, None),
                 lambda: lib.mhip_segment_contacts_linker_pass(None, Q, None),
                 lambda: lib.mhip_segment_contacts_reduce(None, Q, 0, Q, None),
                 lambda: lib.mhip_segment_contacts_get(None, C.byref(fields))):
        with pytest.raises(ValueError, match="null"):
            capi.check(call())
    assert lib.mhip_segment_contacts_destroy(None) == 0


def _spec(**kw):
    s = dict(kind="hertz", radius=0.5, skin=0.3, segments=np.array([[0, 1], [2, 3]]))
    s.update(kw)
    return s


OPS_REFUSED = [
    (_spec(kind="lj"), "kind"), (_spec(segments=None), "segments"), (_spec(segments=[[0, 4], [2, 3]]), "outside"),
    (_spec(segments=[[0, 1], [2, 2]]), "to itself"), (_spec(segments=[[0.5, 1.0]]), "integers"),
    (_spec(radius=0.0), "radius"), (_spec(radius=[0.5, math.nan]), "radius"), (_spec(radius=[0.5]), "shape"),
    (_spec(skin=-1.0), "skin"), (_spec(skin=math.nan), "skin"),
    (_spec(youngs_modulus=0.0), "youngs_modulus"), (_spec(poisson_ratio=1.0), "poisson_ratio"),
    (_spec(kind="wca", epsilon=-1.0), "epsilon"), (_spec(kind="wca", sigma=0.0), "sigma"),
    (_spec(kind="wca", cutoff=math.inf), "cutoff"), (_spec(end_correction=[1, 0, 1]), "end_correction"),
    (_spec(friction=0.5), "unknown key"), ({k: v for k, v in _spec().items() if k != "skin"}, "missing"),
]


@pytest.mark.parametrize("spec,match", OPS_REFUSED)
def test_check_segment_contacts_refuses_without_loading_the_library(monkeypatch, spec, match):
    from mundy_amd import capi, ops

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        ops.check_segment_contacts(4, spec)
    with pytest.raises(ValueError, match=match):
        ops.SegmentContacts(4, **spec)


def test_check_segment_contacts_returns_the_defaults_and_the_chain_ends():
    from mundy_amd import capi, ops, synth
    ends = synth.backbone_segments([0, 4, 6, 7])
    assert ends.tolist() == [[0, 1], [1, 2], [2, 3], [4, 5]] == scm.backbone_segments([0, 4, 6, 7]).tolist()
    e, ra, r0, corr, prm = ops.check_segment_contacts(7, dict(kind="wca", radius=0.5, skin=0.3, segments=ends))
    assert e.dtype == np.int32 and ra is None and r0 == 0.5 and corr.tolist() == [1, 0, 1, 1]
    assert corr.tolist() == scm.chain_end_segments(7, ends).astype(int).tolist()
    assert (prm.kind, prm.skin, prm.epsilon, prm.sigma, prm.cutoff) == (capi.SEGMENT_CONTACT_WCA, 0.3, 1.0, 1.0,
                                                                       1.12246204831)
    assert (prm.youngs_modulus, prm.poisson_ratio) == (1000.0, 0.3)
    assert ops.check_segment_contacts(7, _spec(segments=ends, end_correction=False))[3].tolist() == [0, 0, 0, 0]
    assert ops.check_segment_contacts(7, _spec(segments=ends, end_correction=[0, 1, 0, 0]))[3].tolist() == [0, 1, 0, 0]
    assert ops.check_segment_contacts(7, _spec(segments=ends, radius=[0.5, 0.4, 0.3, 0.2]))[1].tolist() == [0.5, 0.4, 0.3,
                                                                                                         0.2]


# ---- 4. the stepper's refusals, before the library is loaded ----------------------------------------------------------------
def _bb(**kw):
    d = dict(kind="hertz", radius=0.5, skin=0.3, segments=np.array([[0, 1], [2, 3]]))
    d.update(kw)
    return d


STEPPER_REFUSED = [
    (dict(contact_model="none"), "needs backbone_collision"),
    (dict(contact_model="soft", backbone_collision=_bb()), "contact_model must be"),
    (dict(backbone_collision=_bb(), periodic_box=[9.0, 9.0, 9.0]), "periodic_box"),
    (dict(backbone_collision=_bb(), kind="spherocylinder"), "spheres only"),
    (dict(backbone_collision=_bb(), growth_rate=0.1), "spheres only|growth"),
    (dict(backbone_collision=_bb(segments=None)), "segments= or springs="),
    (dict(backbone_collision=_bb(kind="lj")), "kind"),
    (dict(backbone_collision=_bb(skin=-1.0)), "skin"),
    (dict(backbone_collision=_bb(friction=1.0)), "unknown key"),
    (dict(backbone_collision=[0.5, 0.3]), "must be a dict"),
    (dict(contact_model="none", backbone_collision=_bb(segments=[[0, 1], [3, 3]])), "to itself"),
]


@pytest.mark.parametrize("kw,match", STEPPER_REFUSED)
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi, pipeline

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    kw = dict(kw)
    kind = kw.pop("kind", "sphere")
    n = 4
    extra = {}
    if kind == "spherocylinder":
        extra = dict(quat=torch.tensor([[1.0, 0, 0, 0]] * n, dtype=torch.float64),
                     length=torch.ones(n, dtype=torch.float64))
    with pytest.raises(ValueError, match=match):
        pipeline.ContactStepper(kind, torch.zeros((n, 3), dtype=torch.float64),
                                torch.full((n,), 0.5, dtype=torch.float64), **extra, **kw)


def test_new_step_statistics_default_to_zero_and_the_pinned_layout_is_unchanged():
    from mundy_amd import pipeline
    s = pipeline.StepStats()
    assert (s.max_segment_overlap, s.segment_contacts, s.num_segment_pairs, s.segment_list_rebuilt) == (0.0, 0, 0, False)
    assert pipeline.STATS_LENGTH == {"chain": 3, "crosslinkers": 6, "nucleus": 9} and len(pipeline.STATS) == 13


# ---- 5. the C++ app ------------------------------------------------------------------------------------------------------------
def test_backbone_collision_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("backbone_collision_step_app")
    assert os.path.exists(exe)
