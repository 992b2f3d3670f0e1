"""CPU-side checks of the crosslinker KMC step: known answers of the numpy model (crosslinker_model.py), the refusals of
the stepper and of mhip_crosslinkers_create (before any HIP call), the new entry points exported and bound."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import crosslinker_model as xm

PAR = dict(kind="hookean", k=5.0, r=0.5, A=2.0, k_off=3.0, kt=1.0, capture_radius=1.0, dt=0.05)


def _step(center, left, right, ptr, col, keys=None, counters=None, **kw):
    p = dict(PAR, **kw)
    m = len(left)
    keys = np.arange(m, dtype=np.uint64) if keys is None else keys
    counters = np.zeros(m, dtype=np.uint64) if counters is None else counters
    return xm.kmc_step(np.asarray(center, dtype=np.float64), left, right, ptr, col, p["kind"], p["k"], p["r"], p["A"],
                       p["k_off"], p["kt"], p["capture_radius"], p["dt"], keys, counters)


def _pairs(m, d):
    """m independent (left bead 2c, site 2c + 1) pairs at distance d along x, far from each other"""
    center = np.zeros((2 * m, 3))
    center[:, 1] = 10.0 * (np.arange(2 * m) // 2)
    center[1::2, 0] = d
    left = 2 * np.arange(m)
    ptr = np.zeros(2 * m + 1, np.int64)
    ptr[1::2] = np.arange(1, m + 1)
    ptr[2::2] = np.arange(1, m + 1)
    return center, left, ptr, left + 1


def test_uniform_is_the_53_bit_map_of_block_0():
    import chain_model as cm
    keys, ctr = np.array([0, 5, 2 ** 62], np.uint64), np.array([0, 7, 2 ** 40], np.uint64)
    w = cm.philox(keys, ctr, 0).astype(np.uint64)
    u = xm.uniform(keys, ctr)
    assert (u == ((w[:, 0] * np.uint64(2 ** 21)) + (w[:, 1] >> np.uint64(11))).astype(np.float64) / 2.0 ** 53).all()
    assert ((u >= 0) & (u < 1)).all()


def test_no_candidates_never_binds_and_still_advances_the_counter():
    m = 5000
    left = np.arange(m)
    ctr = np.arange(m, dtype=np.uint64) * np.uint64(3)
    res = _step(np.zeros((m, 3)), left, left.copy(), np.zeros(m + 1, np.int64), np.zeros(0, np.int64), counters=ctr)
    assert (res["right"] == left).all() and res["binds"] == 0 and res["unbinds"] == 0
    assert (res["counters"] == ctr + np.uint64(1)).all()
    assert (res["z_tot"] == 0).all() and not np.isnan(res["margin"]).any()


@pytest.mark.parametrize("kw", [dict(A=0.0), dict(kind="fene", r=0.4)])
def test_zero_total_rate_never_binds_and_makes_no_nan(kw):
    m = 20000
    center, left, ptr, col = _pairs(m, 0.5)   # FENE: d = 0.5 >= r_max = 0.4
    with np.errstate(all="raise", divide="ignore", invalid="ignore"):
        res = _step(center, left, left.copy(), ptr, col, **kw)
    assert (res["z_tot"] == 0).all()
    assert (res["right"] == left).all() and res["binds"] == 0
    assert res["u"].min() < 1e-3 and not np.isnan(res["margin"]).any()   # even the smallest draw does not bind


def test_single_candidate_binds_iff_u_below_one_minus_exp():
    m = 20000
    d = 0.8
    center, left, ptr, col = _pairs(m, d)
    res = _step(center, left, left.copy(), ptr, col)
    rate = PAR["A"] * math.exp(-0.5 * (1.0 / PAR["kt"]) * PAR["k"] * (d - PAR["r"]) * (d - PAR["r"]))
    p = 1.0 - math.exp(-PAR["dt"] * rate)
    want = res["u"] < p
    assert (np.abs(res["z_tot"] - PAR["dt"] * rate) <= 1e-15).all()
    assert ((res["right"] != left) == want).all() and (res["right"][want] == col[want]).all()
    assert 0 < want.sum() < m and res["binds"] == want.sum()


def test_capture_cutoff_is_exact_at_the_radius_and_at_the_next_double():
    m = 2000
    cap = PAR["capture_radius"]
    for d, binds in ((cap, True), (np.nextafter(cap, 2.0), False), (np.nextafter(cap, 0.0), True)):
        center, left, ptr, col = _pairs(m, d)
        assert (xm.distance(center[col], center[left]) == d).all()
        res = _step(center, left, left.copy(), ptr, col, A=1e9)   # within reach, binding is certain
        assert ((res["right"] != left) == binds).all(), d
        assert ((res["z_tot"] > 0) == binds).all()


def test_fene_guard_at_and_beyond_r_max():
    r = 0.9
    d = np.array([0.0, 0.5, np.nextafter(r, 0.0), r, np.nextafter(r, 1.0), 0.95, 5.0])
    z = xm.rate("fene", d, 5.0, r, 2.0, 1.0)
    assert (z[3:] == 0).all() and (z[:3] >= 0).all() and np.isfinite(z).all()
    assert z[0] == 2.0 and z[1] == 2.0 * (1.0 - (0.5 / r) * (0.5 / r)) ** (0.5 * 1.0 * 5.0 * r * r)
    assert xm.rate("hookean", np.array([0.5]), 5.0, 0.5, 2.0, 1.0)[0] == 2.0


def test_self_site_is_skipped():
    m = 1000
    center, left, _, _ = _pairs(m, 0.5)
    # every left bead lists itself and its partner; with the partner out of reach only the self site is left
    ptr = np.zeros(2 * m + 1, np.int64)
    ptr[1::2] = 2 * np.arange(1, m + 1)
    ptr[2::2] = 2 * np.arange(1, m + 1)
    col = np.stack([left, left + 1], axis=1).reshape(-1)
    res = _step(center, left, left.copy(), ptr, col, A=1e9)
    assert (res["right"] == left + 1).all()
    center[1::2, 0] = 3.0
    res = _step(center, left, left.copy(), ptr, col, A=1e9)
    assert (res["right"] == left).all() and (res["z_tot"] == 0).all()


def test_doubly_bound_unbinds_at_the_constant_rate_and_ignores_its_row():
    m = 20000
    center, left, ptr, col = _pairs(m, 0.5)
    res = _step(center, left, left + 1, ptr, col)
    p = 1.0 - math.exp(-(PAR["dt"] * PAR["k_off"]))
    want = res["u"] < p
    assert ((res["right"] == left) == want).all() and (res["right"][~want] == left[~want] + 1).all()
    assert res["unbinds"] == want.sum() and res["binds"] == 0
    assert (res["counters"] == 1).all()


def test_two_state_chain_reaches_its_stationary_bound_fraction():
    m, d, steps = 200000, 0.7, 40
    center, left, ptr, col = _pairs(m, d)
    kw = dict(A=8.0, k_off=6.0)
    p_on = 1.0 - math.exp(-PAR["dt"] * float(xm.rate("hookean", d, PAR["k"], PAR["r"], kw["A"], PAR["kt"])))
    p_off = 1.0 - math.exp(-PAR["dt"] * kw["k_off"])
    assert (1.0 - p_on - p_off) ** steps < 1e-9   # mixed
    right, ctr = left.copy(), np.zeros(m, np.uint64)
    keys = np.random.default_rng(5).integers(0, 2 ** 63, m).astype(np.uint64)
    for _ in range(steps):
        res = _step(center, left, right, ptr, col, keys=keys, counters=ctr, **kw)
        right, ctr = res["right"], res["counters"]
    pi = p_on / (p_on + p_off)
    frac = float((right != left).mean())
    assert abs(frac - pi) < 5.0 * math.sqrt(pi * (1.0 - pi) / m), (frac, pi)


def test_candidate_rows_are_the_brute_force_lists():
    rng = np.random.default_rng(2)
    n = 600
    c = rng.uniform(0, 6, (n, 3))
    src, tgt = rng.random(n) < 0.6, rng.random(n) < 0.5
    ptr, col = xm.candidate_rows(c, src, tgt, 1.0)
    d = xm.distance(c[:, None, :], c[None, :, :])
    want = (d <= 1.0) & src[:, None] & tgt[None, :] & ~np.eye(n, dtype=bool)
    for s in range(n):
        assert (col[ptr[s]:ptr[s + 1]] == np.flatnonzero(want[s])).all()
    ids = rng.permutation(n)
    by_id = xm.sort_rows_by_id(ptr, col, ids)
    for s in range(0, n, 7):
        row = by_id[ptr[s]:ptr[s + 1]]
        assert sorted(row) == sorted(col[ptr[s]:ptr[s + 1]]) and (np.diff(ids[row]) > 0).all()


@pytest.mark.parametrize("kind", ["hookean", "fene"])
def test_decision_case_seeds_leave_no_crosslinker_out_in_the_model(kind):
    # the seeds of tests/test_gpu_crosslinkers.py: with a 53-bit uniform about 10^-10 of the draws fall within the margin
    d = xm.decision_case(kind, xm.DECISION_SEEDS[kind])
    p = d["par"]
    src = np.zeros(d["sites"].shape[0], np.uint8)
    src[d["left"]] = 1
    ptr, col = xm.candidate_rows(d["center"], src, d["sites"], p["capture_radius"])
    col = xm.sort_rows_by_id(ptr, col, d["ids"])
    rows = np.diff(ptr)[d["left"]]
    assert rows.min() == 0 and 30 <= rows.max() <= 60
    res = xm.kmc_step(d["center"], d["left"], d["right"], ptr, col, kind, p["k"], p["r"], p["bind_rate"],
                      p["unbind_rate"], p["kt"], p["capture_radius"], d["dt"], d["keys"].view(np.uint64),
                      d["counter"].view(np.uint64))
    assert int(xm.left_out(res).sum()) == 0
    assert res["binds"] > 5000 and res["unbinds"] > 5000 and (res["counters"] == d["counter"].view(np.uint64) + 1).all()


def test_step_stats_gain_the_crosslinker_counts_with_default_zero():
    from mundy_amd import pipeline
    s = pipeline.StepStats()
    assert (s.crosslinker_bound, s.crosslinker_binds, s.crosslinker_unbinds) == (0, 0, 0)


# ---- refusals -----------------------------------------------------------------------------------------------------------
def _xl(**kw):
    d = dict(left=[0, 1], sites=[1, 1, 1, 1], kind="hookean", k=5.0, r=0.5, bind_rate=2.0, unbind_rate=3.0, kt=1.0,
             capture_radius=1.0, skin=0.25)
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
    (dict(kind="spherocylinder", crosslinkers=_xl()), "spheres only"),
    (dict(kind="mixed", crosslinkers=_xl()), "spheres only"),
    (dict(kind="spherocylinder", crosslinkers=_xl(), growth_rate=0.1, division_length=2.0), "spheres only"),
    (dict(crosslinkers=_xl(), growth_rate=0.1, division_length=2.0), "growth"),
    (dict(crosslinkers=_xl(), contact_model="hertz", hertz_friction=0.3), "hertz_friction"),
    (dict(crosslinkers=_xl(), friction=0.3), "friction"),
    (dict(crosslinkers=_xl(), contact_cutoff=0.1), "contact_cutoff"),
    (dict(crosslinkers=_xl(), periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(crosslinkers=[0, 1]), "dict"),
    (dict(crosslinkers=_xl(colour=1)), "unknown key"),
    (dict(crosslinkers=_xl(skin=...)), "missing key"),
    (dict(crosslinkers=_xl(sites=[1, 1, 1])), "mask"),
    (dict(crosslinkers=_xl(sites=[1, 2, 0, 1])), "0 / 1"),
    (dict(crosslinkers=_xl(sites=[0.5, 1.0, 0.0, 1.0])), "mask"),
    (dict(crosslinkers=_xl(left=[0, 4])), "outside"),
    (dict(crosslinkers=_xl(left=[[0, 1]])), r"shape \[m\]"),
    (dict(crosslinkers=_xl(right=[0, 7])), "outside"),
    (dict(crosslinkers=_xl(right=[0])), "right must be"),
    (dict(crosslinkers=_xl(sites=[1, 1, 0, 1], right=[2, 1])), "not a bind site"),
    (dict(crosslinkers=_xl(kind="harmonic")), "spring type"),
    (dict(crosslinkers=_xl(k=-1.0)), "constant k"),
    (dict(crosslinkers=_xl(r=-0.5)), "rest length"),
    (dict(crosslinkers=_xl(kind="fene", r=0.0)), "r_max"),
    (dict(crosslinkers=_xl(bind_rate=-2.0)), "bind_rate"),
    (dict(crosslinkers=_xl(bind_rate=math.inf)), "bind_rate"),
    (dict(crosslinkers=_xl(unbind_rate=math.nan)), "unbind_rate"),
    (dict(crosslinkers=_xl(kt=0.0)), "kt"),
    (dict(crosslinkers=_xl(capture_radius=0.0)), "capture_radius"),
    (dict(crosslinkers=_xl(skin=-0.1)), "skin"),
    (dict(crosslinkers=_xl(keys=[0, -1])), r"2\^63"),
    (dict(crosslinkers=_xl(keys=[0, 1, 2])), "keys"),
    (dict(crosslinkers=_xl(counter=[0.5, 1.0])), "counter")])
def test_stepper_refuses_without_loading_the_library(monkeypatch, kw, match):
    from mundy_amd import capi

    def no_load():
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(capi, "load", no_load)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    for name in ("create", "set_candidates", "kmc_step", "force", "get_state", "set_state", "renumber", "destroy"):
        assert hasattr(lib, "mhip_crosslinkers_" + name) and "mhip_crosslinkers_" + name in capi.SIGNATURES


def _create(lib, n=4, left=(0, 1), right=None, sites=(1, 1, 1, 1), kind=0, k=5.0, r=0.5, a=2.0, off=3.0, kt=1.0, cap=1.0):
    le = np.ascontiguousarray(left, dtype=np.int32)
    ri = None if right is None else np.ascontiguousarray(right, dtype=np.int32)
    si = None if sites is None else np.ascontiguousarray(sites, dtype=np.uint8)
    cp = lambda x: None if x is None else x.ctypes.data_as(C.c_void_p)  # noqa: E731
    h = C.c_void_p(12345)
    st = lib.mhip_crosslinkers_create(C.byref(h), n, le.shape[0], cp(le), cp(ri), cp(si), kind, k, r, a, off, kt, cap,
                                      None)
    return st, h


@pytest.mark.parametrize("kw,match", [
    (dict(left=(0, 4)), "outside"), (dict(left=(-1, 2)), "outside"), (dict(right=(0, 9)), "outside"),
    (dict(sites=(1, 1, 0, 1), right=(2, 1)), "not a bind site"), (dict(kind=7), "spring type"),
    (dict(k=-1.0), "k must"), (dict(k=math.nan), "k must"), (dict(r=-0.1), "rest length"), (dict(kind=1, r=0.0), "r_max"),
    (dict(kind=1, r=math.inf), "r_max"), (dict(a=-1.0), "bind_rate"), (dict(a=math.inf), "bind_rate"),
    (dict(off=-1.0), "unbind_rate"), (dict(off=math.nan), "unbind_rate"), (dict(kt=0.0), "kt"), (dict(kt=-1.0), "kt"),
    (dict(kt=math.inf), "kt"), (dict(cap=0.0), "capture_radius"), (dict(cap=math.nan), "capture_radius")])
def test_create_refuses_bad_arguments_before_any_hip_call(lib, kw, match):
    from mundy_amd import capi
    st, h = _create(lib, **kw)
    with pytest.raises(ValueError, match=match):
        capi.check(st)
    assert h.value is None  # nothing was created


def test_null_handles_and_pointers_are_refused(lib):
    from mundy_amd import capi
    P = lambda v: C.c_void_p(16 * v)  # noqa: E731  (fake device pointers, never dereferenced)
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_create(None, 4, 0, None, None, None, 0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_kmc_step(None, P(1), 1e-3, P(2), P(3), P(4), None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_force(None, P(1), P(2), 0, P(3), P(4), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_set_candidates(None, P(1), P(2), 4, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_crosslinkers_renumber(None, P(1), None))
    capi.check(lib.mhip_crosslinkers_destroy(None))


def test_crosslinker_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("crosslinker_step_app")
    assert os.path.exists(exe)
