"""CPU-side checks of the periphery bind sites (include/mundy_hip_periphery_binding.h): known answers of the numpy model
(periphery_binding_model.py), the seeds of the GPU decision test, every refusal with the library loader disabled and the
library's own before any HIP call, the site generator, the statistics slot, the header against the binding table, the
C++ app."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import crosslinker_model as xm
import periphery_binding_model as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_periphery_binding.h")
NAMES = ("mhip_crosslinkers_set_periphery_sites", "mhip_crosslinkers_set_periphery_candidates",
         "mhip_crosslinkers_kmc_step_periphery")
PAR = dict(kind="hookean", k=5.0, r=0.5, A=2.0, k_off=3.0, kt=1.0, capture_radius=1.0)
PER = dict(A=3.0, k=4.0, r=0.4, k_off=None, capture_radius=1.2)
DT = 0.05


def _lattice(m, d_bead, d_site):
    """m independent groups far from each other: left bead 2c, a bead site 2c + 1 at d_bead along x (None: the bead
    row is empty), periphery site c at d_site along y (None: the site row is empty)"""
    center = np.zeros((2 * m, 3))
    center[:, 2] = 10.0 * (np.arange(2 * m) // 2)
    center[1::2, 0] = 5.0 if d_bead is None else d_bead
    left = 2 * np.arange(m)
    cnt = np.zeros(2 * m, np.int64)
    ptr, col = np.zeros(2 * m + 1, np.int64), np.zeros(0, np.int64)
    if d_bead is not None:
        cnt[left] = 1
        ptr, col = np.concatenate([[0], np.cumsum(cnt)]), left + 1
    sites = center[0::2].copy()
    sites[:, 1] = 5.0 if d_site is None else d_site
    pptr, pcol = np.zeros(2 * m + 1, np.int64), np.zeros(0, np.int64)
    if d_site is not None:
        cnt[:] = 0
        cnt[left] = 1
        pptr, pcol = np.concatenate([[0], np.cumsum(cnt)]), np.arange(m)
    return center, left, ptr, col, pptr, pcol, sites


def _step(case, right=None, par=PAR, per=PER, keys=None):
    center, left, ptr, col, pptr, pcol, sites = case
    m = left.shape[0]
    keys = np.arange(m, dtype=np.uint64) if keys is None else keys
    return pm.kmc_step(center, left, left.copy() if right is None else right, ptr, col, pptr, pcol, sites, par, per, DT,
                       keys, np.zeros(m, np.uint64))


def _rate(d, p, kind="hookean", kt=1.0):
    return float(xm.rate(kind, d, p["k"], p["r"], p["A"], kt))


# ---- 1. known answers of the model -------------------------------------------------------------------------------------
def test_only_periphery_candidates_in_reach():
    m, d = 20000, 0.7
    case = _lattice(m, None, d)
    res = _step(case)
    z = DT * _rate(d, PER)
    want = res["u"] < 1.0 - math.exp(-z)
    assert (res["z_tot"] == z).all() and (res["z_beads"] == 0).all()
    assert 0 < want.sum() < m and res["binds"] == want.sum() == res["periphery_bound"]
    assert (res["right"][want] == -(np.arange(m)[want] + 1)).all() and (res["right"][~want] == case[1][~want]).all()
    assert (res["counters"] == 1).all()


def test_z_tot_is_the_bead_row_sum_continued_over_the_site_row():
    m = 5000
    case = _lattice(m, 0.8, 0.6)
    center, left, ptr, col = case[:4]
    res = _step(case)
    beads = xm.kmc_step(center, left, left.copy(), ptr, col, "hookean", PAR["k"], PAR["r"], PAR["A"], PAR["k_off"], 1.0,
                        PAR["capture_radius"], DT, np.arange(m, dtype=np.uint64), np.zeros(m, np.uint64))
    assert (res["z_beads"].view(np.uint64) == beads["z_tot"].view(np.uint64)).all()
    zb = 0.0 + DT * _rate(0.8, PAR)
    assert (res["z_beads"] == zb).all() and (res["z_tot"] == zb + DT * _rate(0.6, PER)).all()   # one sum, left to right


def test_a_draw_between_the_two_rows_binds_the_site():
    m = 40000
    case = _lattice(m, 0.8, 0.6)
    left = case[1]
    res = _step(case)
    z = 0.0 + DT * _rate(0.8, PAR) + DT * _rate(0.6, PER)
    p_bind = 1.0 - math.exp(-z)
    scale = p_bind * DT / z
    c1 = 0.0 + scale * _rate(0.8, PAR)
    c2 = c1 + scale * _rate(0.6, PER)
    u = res["u"]
    bead, site, none = u < c1, (u >= c1) & (u < min(c2, p_bind)), u >= p_bind
    assert bead.sum() > 100 and site.sum() > 100 and none.sum() > 100
    assert (res["right"][bead] == left[bead] + 1).all()
    assert (res["right"][site] == -(np.arange(m)[site] + 1)).all()     # past the bead row's last sum, below the site's
    assert (res["right"][none] == left[none]).all()
    assert res["binds"] == bead.sum() + site.sum() and res["periphery_bound"] == site.sum()
    # the margin sees the thresholds of both rows
    i = int(np.argmin(np.abs(u - c1)))
    assert res["margin"][i] == abs(u[i] - c1)


def test_capture_cut_is_exact_at_the_peripherys_own_radius():
    m = 500
    cap = PER["capture_radius"]
    assert cap != PAR["capture_radius"]
    for d, binds in ((cap, True), (np.nextafter(cap, 2.0), False), (np.nextafter(cap, 0.0), True),
                     (PAR["capture_radius"], True)):
        case = _lattice(m, None, d)
        assert (xm.distance(case[6], case[0][case[1]]) == d).all()
        res = _step(case, per=dict(PER, A=1e9))
        assert ((res["right"] < 0) == binds).all(), d
        assert ((res["z_tot"] > 0) == binds).all()


def test_fene_guard_at_the_peripherys_r_max():
    m = 500
    par = dict(PAR, kind="fene", r=0.9)
    per = dict(PER, A=1e9, r=1.1, capture_radius=2.0)
    for d, live in ((1.1, False), (np.nextafter(1.1, 2.0), False), (1.5, False), (np.nextafter(1.1, 0.0), True),
                    (0.5, True)):
        res = _step(_lattice(m, None, d), par=par, per=per)
        assert ((res["z_tot"] > 0) == live).all() and not np.isnan(res["margin"]).any(), d
    assert (_step(_lattice(m, None, 0.5), par=par, per=per)["right"] < 0).all()
    assert (_step(_lattice(m, None, 0.95), par=par, per=per)["right"] < 0).all()   # beyond the crosslinkers' own r_max


def test_unbinding_rate_goes_by_the_sign_of_right():
    m = 40000
    case = _lattice(m, 0.8, 0.6)
    left = case[1]
    right = left + 1
    right[m // 2:] = -(np.arange(m)[m // 2:] + 1)
    res = _step(case, right=right, per=dict(PER, k_off=11.0))
    p_bead, p_site = 1.0 - math.exp(-(DT * PAR["k_off"])), 1.0 - math.exp(-(DT * 11.0))
    want = np.where(right < 0, res["u"] < p_site, res["u"] < p_bead)
    assert ((res["right"] == left) == want).all() and (res["right"][~want] == right[~want]).all()
    assert res["unbinds"] == want.sum() and res["binds"] == 0 and (res["z_tot"] == 0).all()
    assert res["periphery_bound"] == int((~want[m // 2:]).sum())
    between = (res["u"] >= p_bead) & (res["u"] < p_site)
    assert between[:m // 2].sum() > 100 and (res["right"][:m // 2][between[:m // 2]] != left[:m // 2][between[:m // 2]]).all()
    # the default: the crosslinkers' own rate
    res = _step(case, right=right)
    assert ((res["right"] == left) == (res["u"] < p_bead)).all()


def test_sites_out_of_reach_give_the_crosslinker_models_result_bit_for_bit():
    d = xm.decision_case("hookean", 5, n=3000, m=4000)
    p = d["par"]
    src = np.zeros(3000, np.uint8)
    src[d["left"]] = 1
    ptr, col = xm.candidate_rows(d["center"], src, d["sites"], p["capture_radius"])
    col = xm.sort_rows_by_id(ptr, col, d["ids"])
    keys, ctr = d["keys"].view(np.uint64), d["counter"].view(np.uint64)
    want = xm.kmc_step(d["center"], d["left"], d["right"], ptr, col, "hookean", p["k"], p["r"], p["bind_rate"],
                       p["unbind_rate"], p["kt"], p["capture_radius"], d["dt"], keys, ctr)
    sites = np.random.default_rng(1).uniform(500.0, 510.0, (37, 3))
    # listed but beyond the capture radius, and not listed at all
    listed = (np.concatenate([[0], np.cumsum(src.astype(np.int64) * 2)]), np.tile([3, 30], int(src.sum())))
    for pptr, pcol in (listed, (np.zeros(3001, np.int64), np.zeros(0, np.int64))):
        got = pm.kmc_step(d["center"], d["left"], d["right"], ptr, col, pptr, pcol, sites, pm.from_ops(p), PER, d["dt"],
                          keys, ctr)
        assert (got["right"] == want["right"]).all() and (got["counters"] == want["counters"]).all()
        for k in ("z_tot", "margin", "u"):
            assert (got[k].view(np.uint64) == want[k].view(np.uint64)).all(), k
        assert (got["binds"], got["unbinds"], got["periphery_bound"]) == (want["binds"], want["unbinds"], 0)


def test_force_model_adds_the_site_term_to_the_left_bead_only():
    c = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    sites = np.array([[0.0, 0.0, 3.0], [9.0, 9.0, 9.0]])
    left, right = np.array([0, 0, 2, 1]), np.array([1, -1, 2, -1])
    f, over, mx, fs = pm.crosslinker_force(3, left, right, "hookean", 2.0, 0.5, c, sites)
    t01 = 2.0 * (1.0 - 0.5) * (1.0 / 1.0) * np.array([1.0, 0.0, 0.0])
    t0s = 2.0 * (3.0 - 0.5) * (1.0 / 3.0) * np.array([0.0, 0.0, 3.0])
    d1s = sites[0] - c[1]
    L = math.sqrt(d1s[0] * d1s[0] + d1s[1] * d1s[1] + d1s[2] * d1s[2])
    t1s = 2.0 * (L - 0.5) * (1.0 / L) * d1s
    assert (f[0] == (0.0 + t01) + t0s).all() and (f[1] == (0.0 - t01) + t1s).all() and (f[2] == 0).all()
    assert (fs[0] == (0.0 - t0s) - t1s).all() and (fs[1] == 0).all() and over == 0 and mx == L


@pytest.mark.parametrize("kind", ["hookean", "fene"])
def test_decision_case_seeds_leave_no_crosslinker_out_in_the_model(kind):
    d = pm.decision_case(kind, pm.DECISION_SEEDS[kind])
    p, per = d["par"], d["per"]
    n, m = d["center"].shape[0], d["left"].shape[0]
    src = np.zeros(n, np.uint8)
    src[d["left"]] = 1
    ptr, col = xm.candidate_rows(d["center"], src, d["sites"], p["capture_radius"])
    col = xm.sort_rows_by_id(ptr, col, d["ids"])
    pptr, pcol = pm.site_rows(d["center"], src, d["site_points"], per["capture_radius"])
    res = pm.kmc_step(d["center"], d["left"], d["right"], ptr, col, pptr, pcol, d["site_points"], pm.from_ops(p), per,
                      d["dt"], d["keys"].view(np.uint64), d["counter"].view(np.uint64))
    assert int(xm.left_out(res).sum()) == 0
    at_site, at_bead = d["right"] < 0, (d["right"] >= 0) & (d["right"] != d["left"])
    assert abs(at_site.mean() - 1.0 / 6.0) < 0.02 and abs(at_bead.mean() - 1.0 / 3.0) < 0.02
    rows, prows = np.diff(ptr)[d["left"]], np.diff(pptr)[d["left"]]
    free = d["right"] == d["left"]
    for a in (False, True):   # the four kinds of row among the singly bound
        for b in (False, True):
            assert (free & ((rows > 0) == a) & ((prows > 0) == b)).sum() > 10, (a, b)
    new = res["right"] != d["right"]
    assert (new & (res["right"] < 0)).sum() > 20 and (new & (res["right"] >= 0) & free).sum() > 500
    assert (at_site & (res["right"] == d["left"])).sum() > 200 and res["unbinds"] > 1000
    assert (res["z_tot"] > res["z_beads"]).sum() > 200


# ---- 2. refusals with the loader disabled ------------------------------------------------------------------------------
PTS = [[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]


def _per(**kw):
    d = dict(points=PTS, bind_rate=1.0, k=1000.0, r=1.0)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not ...}


def _xl(**kw):
    d = dict(left=[0, 1], sites=[1, 1, 1, 1], kind="hookean", k=5.0, r=0.5, bind_rate=2.0, unbind_rate=3.0, kt=1.0,
             capture_radius=1.0, skin=0.25, periphery_sites=_per())
    d.update(kw)
    return d


REFUSED = [
    (_xl(periphery_sites=[1, 2]), "dict"),
    (_xl(periphery_sites=_per(colour=1)), "unknown key"),
    (_xl(periphery_sites=_per(points=...)), "missing key"),
    (_xl(periphery_sites=_per(k=...)), "missing key"),
    (_xl(periphery_sites=_per(points=np.zeros((0, 3)))), "P must be > 0"),
    (_xl(periphery_sites=_per(points=[[0.0, 1.0]])), r"shape \[P, 3\]"),
    (_xl(periphery_sites=_per(points=[0.0, 1.0, 2.0])), r"shape \[P, 3\]"),
    (_xl(periphery_sites=_per(points=[[0.0, math.nan, 1.0]])), "finite"),
    (_xl(periphery_sites=_per(points=[[0.0, math.inf, 1.0]])), "finite"),
    (_xl(periphery_sites=_per(bind_rate=-1.0)), "bind_rate"),
    (_xl(periphery_sites=_per(bind_rate=math.inf)), "bind_rate"),
    (_xl(periphery_sites=_per(unbind_rate=-1.0)), "unbind_rate"),
    (_xl(periphery_sites=_per(unbind_rate=math.nan)), "unbind_rate"),
    (_xl(periphery_sites=_per(k=-1.0)), "constant k"),
    (_xl(periphery_sites=_per(k=math.nan)), "constant k"),
    (_xl(periphery_sites=_per(r=-0.5)), "rest length"),
    (_xl(periphery_sites=_per(r=math.inf)), "rest length"),
    (_xl(kind="fene", periphery_sites=_per(r=0.0)), "r_max"),
    (_xl(kind="fene", periphery_sites=_per(r=-1.0)), "r_max"),
    (_xl(periphery_sites=_per(capture_radius=0.0)), "capture_radius"),
    (_xl(periphery_sites=_per(capture_radius=-2.0)), "capture_radius"),
    (_xl(periphery_sites=_per(capture_radius=math.inf)), "capture_radius"),
    (_xl(right=[0, -4]), "no periphery site"),
    (_xl(right=[0, 4]), "outside"),
    (dict(_xl(right=[0, -1]), periphery_sites=None), "outside"),
]


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    return pipeline.ContactStepper("sphere", torch.zeros((n, 3), dtype=torch.float64),
                                   torch.full((n,), 0.5, dtype=torch.float64), **kw)


@pytest.mark.parametrize("spec,match", REFUSED)
def test_stepper_refuses_without_loading_the_library(monkeypatch, spec, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(crosslinkers=spec)


def test_check_periphery_sites_returns_the_defaults(monkeypatch):
    from mundy_amd import capi, ops
    monkeypatch.setattr(capi, "load", lambda: (_ for _ in ()).throw(AssertionError("loaded")))
    pts, a, k, r, off, cap = ops.check_periphery_sites(_per(), "hookean", 3.0, 1.5)
    assert pts.shape == (3, 3) and pts.dtype == np.float64 and (a, k, r, off, cap) == (1.0, 1000.0, 1.0, 3.0, 1.5)
    _, _, _, _, off, cap = ops.check_periphery_sites(_per(unbind_rate=7.0, capture_radius=2.0), "fene", 3.0, 1.5)
    assert (off, cap) == (7.0, 2.0)
    # a right head at a periphery site passes the crosslinker check only with the count of sites
    le, ri = ops.check_crosslinkers(4, [0, 1], [-3, 1], [1, 1, 1, 1], "hookean", 5.0, 0.5, 2.0, 3.0, 1.0, 1.0,
                                    num_periphery_sites=3)[:2]
    assert ri.tolist() == [-3, 1] and ri.dtype == np.int32
    with pytest.raises(ValueError, match="outside"):
        ops.check_crosslinkers(4, [0, 1], [-3, 1], [1, 1, 1, 1], "hookean", 5.0, 0.5, 2.0, 3.0, 1.0, 1.0)


# ---- 3. the library: header, table, refusals before any HIP call ------------------------------------------------------
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
    assert set(protos) == set(NAMES) == set(capi.PERIPHERY_BINDING_SIGNATURES)
    for other in (capi.SIGNATURES, capi.PERIPHERY_SIGNATURES, capi.CONTACT_FORCE_SIGNATURES):
        assert not set(capi.PERIPHERY_BINDING_SIGNATURES) & set(other)
    others = [open(os.path.join(ROOT, "include", h)).read()
              for h in ("mundy_hip.h", "mundy_hip_hydro_periphery.h", "mundy_hip_contact_force.h")]
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.PERIPHERY_BINDING_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
        assert "mhip_stream_t" in args
    first = open(HEADER).read()
    first = first[:first.index("*/")]
    for why in ("test_gpu_streams.py", "test_capi_symbols.py", "test_periphery_binding_host.py",
                "test_gpu_periphery_binding_streams.py"):
        assert why in first, "the first comment does not say why the header is its own: %s" % why
    for word in ("beads, then sites", "capture radius", "53-bit", "k_off_p", "generated on the host"):
        assert word in first, "the header does not list the deviation: %s" % word


Q = C.c_void_p(64)  # a non-null pointer that no refused call dereferences


@pytest.mark.parametrize("kw,match", [
    (dict(P=0), "P must be > 0"), (dict(P=2 ** 31), "too many"),
    (dict(a=-1.0), "bind_rate"), (dict(a=math.nan), "bind_rate"), (dict(a=math.inf), "bind_rate"),
    (dict(off=-1.0), "unbind_rate"), (dict(off=math.nan), "unbind_rate"),
    (dict(k=-1.0), "constant k"), (dict(k=math.inf), "constant k"),
    (dict(r=-0.1), "rest length"), (dict(r=math.nan), "rest length"),
    (dict(cap=0.0), "capture_radius"), (dict(cap=-1.0), "capture_radius"), (dict(cap=math.inf), "capture_radius"),
    (dict(), "handle is null")])
def test_set_periphery_sites_refuses_before_any_hip_call(lib, kw, match):
    # (what the arguments alone decide is refused with or without a handle; the refusals that need one -- another P,
    #  r_max <= 0 for FENE crosslinkers, a null site_center -- need a device: tests/test_gpu_periphery_binding.py)
    from mundy_amd import capi
    a = dict(P=3, a=1.0, k=1000.0, r=1.0, off=3.0, cap=1.0)
    a.update(kw)
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_crosslinkers_set_periphery_sites(None, a["P"], Q, a["a"], a["k"], a["r"], a["off"], a["cap"],
                                                             None))


def test_null_handles_are_refused(lib):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_set_periphery_candidates(None, Q, Q, 4, 0, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_kmc_step_periphery(None, Q, 1e-3, Q, Q, Q, None, None, None))


# ---- 4. the site generator -----------------------------------------------------------------------------------------------
def test_sphere_sites_lie_on_the_sphere_and_are_uniform_in_area():
    from mundy_amd import synth
    N, R = 200000, 2.5
    p = synth.periphery_bind_sites("sphere", R, N, seed=3)
    assert p.shape == (N, 3) and p.dtype == np.float64
    assert np.abs((p * p).sum(axis=1) / (R * R) - 1.0).max() <= 1e-14
    z = p[:, 2] / R   # uniform on [-1, 1]: mean 0, variance 1/3, fourth moment 1/5
    assert abs(z.mean()) < 5.0 * math.sqrt(1.0 / 3.0 / N)
    assert abs(z.var() - 1.0 / 3.0) < 5.0 * math.sqrt((1.0 / 5.0 - 1.0 / 9.0) / N)
    assert (synth.periphery_bind_sites("sphere", R, 100, seed=3) == p[:100]).all()   # a prefix: one stream
    assert (synth.periphery_bind_sites("sphere", (R, R, R), 10, seed=3) == p[:10]).all()
    assert (synth.periphery_bind_sites("sphere", R, 100, seed=4) != p[:100]).any()


def test_ellipsoid_sites_lie_on_the_ellipsoid_and_are_uniform_in_area():
    from mundy_amd import synth
    N, (a, b, c) = 200000, (3.0, 2.0, 1.0)
    p = synth.periphery_bind_sites("ellipsoid", (a, b, c), N, seed=5)
    assert p.shape == (N, 3)
    assert np.abs((p[:, 0] / a) ** 2 + (p[:, 1] / b) ** 2 + (p[:, 2] / c) ** 2 - 1.0).max() <= 1e-14
    # the area fraction above z = c / 2 by quadrature over the unit sphere's (t = cos phi, theta): dA = mu dt dtheta
    t, wt = np.polynomial.legendre.leggauss(200)
    th = 2.0 * np.pi * (np.arange(400) + 0.5) / 400

    def area(t0, t1):
        tt = 0.5 * (t1 - t0) * t + 0.5 * (t1 + t0)
        s = np.sqrt(1.0 - tt * tt)[:, None]
        x, y, z = s * np.cos(th)[None, :], s * np.sin(th)[None, :], tt[:, None]
        mu = np.sqrt((b * c * x) ** 2 + (a * c * y) ** 2 + (a * b * z) ** 2)
        return 0.5 * (t1 - t0) * (wt[:, None] * mu).sum() * (2.0 * np.pi / 400)
    frac = area(0.5, 1.0) / area(-1.0, 1.0)
    assert abs(area(-1.0, 1.0) / (4.0 * np.pi) - 1.0) > 0.1 and abs(area(0.0, 1.0) / area(-1.0, 0.0) - 1.0) < 1e-12
    got = float((p[:, 2] > 0.5 * c).mean())
    print("fraction above c/2: %.5f, area fraction %.5f" % (got, frac))
    assert abs(got - frac) < 5.0 * math.sqrt(frac * (1.0 - frac) / N)
    assert abs(frac - 0.25) > 0.02   # (not the sphere's fraction: the rejection step matters)


@pytest.mark.parametrize("args,match", [
    (("cube", 1.0, 10), "shape"), (("sphere", 1.0, 0), "count"), (("sphere", (1.0, 2.0, 3.0), 5), "one radius"),
    (("ellipsoid", (1.0, 2.0), 5), "radii"), (("ellipsoid", (1.0, -2.0, 1.0), 5), "radii"),
    (("sphere", math.inf, 5), "radii")])
def test_site_generator_refuses(args, match):
    from mundy_amd import synth
    with pytest.raises(ValueError, match=match):
        synth.periphery_bind_sites(*args)


# ---- 5. statistics ------------------------------------------------------------------------------------------------------
def test_the_new_statistic_sits_in_slot_5_lane_1_and_is_read():
    from mundy_amd import pipeline
    assert list(pipeline.STATS)[-1] == "crosslinker_periphery_bound"
    assert pipeline.STATS["crosslinker_periphery_bound"] == ("crosslinkers", 5, 1)
    taken = [(slot, lane) for _, slot, lane in pipeline.STATS.values()]
    assert len(set(taken)) == len(taken)
    buf = torch.zeros(pipeline.STATS_LENGTH["crosslinkers"], dtype=torch.float64)
    v = pipeline.stat(buf, "crosslinker_periphery_bound")
    assert v.dtype == torch.int32 and tuple(v.shape) == (1,)
    v += 41
    pipeline.stat(buf, "crosslinkers_overstretched")[0] = 7
    got = pipeline.read_stats(buf)
    assert got["crosslinker_periphery_bound"] == 41 and got["crosslinkers_overstretched"] == 7
    assert "crosslinker_periphery_bound" not in pipeline.read_stats(torch.zeros(3, dtype=torch.float64))
    assert pipeline.StepStats().crosslinker_periphery_bound == 0


# ---- 6. the C++ app -----------------------------------------------------------------------------------------------------
def test_periphery_binding_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("periphery_binding_step_app")
    assert os.path.exists(exe)
