"""Growth and division, host side: the numpy restatement gives the known answers of the model, the new entry points are
exported and bound, and bad arguments are refused before any HIP call (no GPU needed)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import growth_model as gm
from mundy_amd.ops import aabb_moved, divide_grow_spherocylinders, select_dividing


def test_known_answer_axis_aligned_rod():
    # identity quaternion: the rod axis is zhat; r = 0.5, L = 2.5 -> cl = 0.75, s = 0.875
    c = np.array([[1.0, 2.0, 3.0]])
    q = np.array([[1.0, 0.0, 0.0, 0.0]])
    r, L = np.array([0.5]), np.array([2.5])
    assert gm.qrot_z(q).tolist() == [[0.0, 0.0, 1.0]]
    p = gm.select_dividing(L, 2.0)
    assert p.tolist() == [0]
    c2, q2, r2, L2 = gm.divide_grow(c, q, r, L, p, dt=0.0, growth_rate=0.1)
    assert L2.tolist() == [0.75, 0.75] and r2.tolist() == [0.5, 0.5]
    assert c2.tolist() == [[1.0, 2.0, 3.0 - 0.875], [1.0, 2.0, 3.0 + 0.875]]
    assert np.array_equal(q2, np.vstack([q, q]))
    # segments [c - L/2, c + L/2] along zhat: parent [-1.25, -0.5], child [0.5, 1.25] relative to the old centre
    parent_hi = c2[0, 2] + 0.5 * L2[0]
    child_lo = c2[1, 2] - 0.5 * L2[1]
    assert child_lo - parent_hi == 2 * r[0]
    assert c2[0, 2] - 0.5 * L2[0] == 3.0 - 1.25 and c2[1, 2] + 0.5 * L2[1] == 3.0 + 1.25


def test_growth_adds_dt_times_rate_once():
    L = np.array([1.0, 1.5])
    *_, L2 = gm.divide_grow(np.zeros((2, 3)), np.tile([1.0, 0, 0, 0], (2, 1)), np.full(2, 0.5), L,
                            gm.select_dividing(L, 2.0), dt=1e-3, growth_rate=0.1)
    g = 1e-3 * 0.1
    assert L2.tolist() == [1.0 + g, 1.5 + g]


def test_equal_length_and_nan_do_not_divide():
    assert gm.select_dividing(np.array([2.0, np.nan, np.nextafter(2.0, 3.0), np.inf]), 2.0).tolist() == [2, 3]


def test_children_are_ranked_in_index_order():
    L = np.array([3.0, 1.0, 3.0, 3.0, 1.0])
    p = gm.select_dividing(L, 2.0)
    assert p.tolist() == [0, 2, 3]
    c = np.arange(15, dtype=np.float64).reshape(5, 3)
    c2, *_ = gm.divide_grow(c, np.tile([1.0, 0, 0, 0], (5, 1)), np.full(5, 0.5), L, p, 0.0, 0.0)
    for k, i in enumerate(p):  # child n + k sits above its parent i along zhat
        assert c2[5 + k, 2] > c2[i, 2] and c2[5 + k, 0] == c[i, 0]


def test_periodic_wrap_of_a_child_across_a_face():
    c = np.array([[0.5, 0.5, 9.9]])
    c2, *_ = gm.divide_grow(c, np.array([[1.0, 0, 0, 0]]), np.array([0.5]), np.array([2.5]), np.array([0]), 0.0, 0.0,
                            box=(10.0, 10.0, 10.0))
    assert 0.0 <= c2[1, 2] < 10.0 and c2[1, 2] == pytest.approx(9.9 + 0.875 - 10.0, abs=1e-12)


def test_length_recursion_doubles_a_single_rod():
    # r = 0.5, D = 2: a rod starting at 2.0 divides every time its length passes 2
    hist = gm.length_recursion([2.0], [0.5], 2.0, dt=0.1, growth_rate=1.0, steps=30)
    counts = [nb for nb, _ in hist]
    assert counts[0] == 1 and counts[-1] > 1 and counts == sorted(counts)


def test_aabb_moved_threshold():
    ref = np.zeros((1, 6))
    at = ref.copy()
    at[0, 0] = 0.5
    below = ref.copy()
    below[0, 3] = np.nextafter(0.5, 0.0)
    assert gm.aabb_moved(at, ref, 0.5) and not gm.aabb_moved(below, ref, 0.5)


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    for name in ("mhip_select_dividing", "mhip_divide_grow_spherocylinders", "mhip_aabb_moved"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


P = lambda v: None if not v else C.c_void_p(16 * int(v))  # noqa: E731  (fake device pointers, never dereferenced)


@pytest.mark.parametrize("D", [-1.0, float("nan"), float("inf"), -float("inf")])
def test_select_refuses_bad_division_length(lib, D):
    from mundy_amd import capi
    cnt = C.c_size_t(7)
    with pytest.raises(ValueError, match="division_length"):
        capi.check(lib.mhip_select_dividing(4, P(1), D, P(2), C.byref(cnt), None))
    assert cnt.value == 0


@pytest.mark.parametrize("missing", ["length", "parent_of", "num_born"])
def test_select_refuses_null_pointers(lib, missing):
    from mundy_amd import capi
    cnt = C.c_size_t(0)
    args = dict(length=P(1), parent_of=P(2), num_born=C.byref(cnt))
    args[missing] = None
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_select_dividing(4, args["length"], 2.0, args["parent_of"], args["num_born"], None))


def _dg(lib, n=4, nb=1, parent=1, dt=1e-3, rate=0.1, box=None, center=2, quat=3, radius=4, length=5):
    b = None if box is None else (C.c_double * 3)(*box)
    return lib.mhip_divide_grow_spherocylinders(n, nb, P(parent), dt, rate, b, P(center), P(quat), P(radius),
                                                P(length), None)


@pytest.mark.parametrize("kw,match", [(dict(dt=-1e-3), "dt"), (dict(dt=float("nan")), "dt"),
                                      (dict(dt=float("inf")), "dt"), (dict(rate=-0.1), "growth_rate"),
                                      (dict(rate=float("nan")), "growth_rate"), (dict(rate=float("inf")), "growth_rate"),
                                      (dict(nb=5), "num_born"), (dict(parent=0), "null"), (dict(length=0), "null"),
                                      (dict(center=0), "null"), (dict(quat=0), "null"), (dict(radius=0), "null"),
                                      (dict(box=(1.0, 0.0, 1.0)), "box"), (dict(box=(1.0, float("inf"), 1.0)), "box")])
def test_divide_grow_refuses_bad_arguments(lib, kw, match):
    from mundy_amd import capi
    with pytest.raises(ValueError, match=match):
        capi.check(_dg(lib, **kw))


@pytest.mark.parametrize("thr,aabb,ref,match", [(-0.1, 1, 2, "threshold"), (float("nan"), 1, 2, "threshold"),
                                                (float("inf"), 1, 2, "threshold"), (0.1, 0, 2, "null"),
                                                (0.1, 1, 0, "null")])
def test_aabb_moved_refuses_bad_arguments(lib, thr, aabb, ref, match):
    from mundy_amd import capi
    flag = C.c_int(5)
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_aabb_moved(3, P(aabb), P(ref), thr, C.byref(flag), None))
    assert flag.value == 0


def test_aabb_moved_refuses_a_null_flag(lib):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="flag"):
        capi.check(lib.mhip_aabb_moved(3, P(1), P(2), 0.1, None, None))


def test_python_wrappers_check_numbers_first():
    L = torch.ones(3, dtype=torch.float64)
    with pytest.raises(ValueError, match="division_length"):
        select_dividing(L, -1.0)
    with pytest.raises(ValueError, match="threshold"):
        aabb_moved(torch.zeros((3, 6), dtype=torch.float64), torch.zeros((3, 6), dtype=torch.float64), -1.0)
    c, q = torch.zeros((3, 3), dtype=torch.float64), torch.zeros((3, 4), dtype=torch.float64)
    p = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="growth_rate"):
        divide_grow_spherocylinders(3, p, 1e-3, math.nan, c, q, L, L)
    with pytest.raises(ValueError, match="rows"):  # 3 rows cannot hold 3 bodies + 1 child
        divide_grow_spherocylinders(3, p, 1e-3, 0.1, c, q, L, L)


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.full((n,), 0.5, dtype=torch.float64)
    q = torch.zeros((n, 4), dtype=torch.float64)
    kind = kw.pop("kind", "spherocylinder")
    args = dict(growth_rate=0.1, division_length=2.0, contact_model="hertz")
    args.update(kw)
    if kind == "mixed":
        extra = dict(kinds=torch.tensor([0, 1, 1, 1], dtype=torch.int32), shape=torch.ones((n, 3), dtype=torch.float64))
    else:
        extra = dict(length=torch.ones(n, dtype=torch.float64))
    return pipeline.ContactStepper(kind, c, r, q, **extra, **args)


@pytest.mark.parametrize("kw,match", [
    (dict(kind="sphere"), "spherocylinders"), (dict(kind="mixed"), "spherocylinders"),
    (dict(search_kind=0), "SEARCH_AABB"), (dict(friction=0.3, contact_model="lcp"), "friction"),
    (dict(contact_cutoff=0.1, contact_model="lcp"), "contact_cutoff"), (dict(warm_start=True, contact_model="lcp"), "warm"),
    (dict(division_length=0.99), "division_length"), (dict(division_length=None), "division_length"),
    (dict(division_length=float("nan")), "division_length"), (dict(growth_rate=-0.1), "growth_rate"),
    (dict(growth_rate=float("inf")), "growth_rate"), (dict(periodic_box=np.eye(3) * 10.0), "orthorhombic"),
    (dict(ids=torch.arange(3)), "ids"), (dict(capacity=-1), "capacity")])
def test_stepper_refuses_what_growth_mode_does_not_have(kw, match):
    # refused in the constructor before anything reaches the device (these tensors are on the CPU)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


@pytest.mark.parametrize("kw", [dict(division_length=2.0), dict(capacity=10), dict(ids=torch.arange(4))])
def test_growth_keywords_need_growth_rate(kw):
    from mundy_amd import pipeline
    n = 4
    with pytest.raises(ValueError, match="growth_rate"):
        pipeline.ContactStepper("spherocylinder", torch.zeros((n, 3), dtype=torch.float64),
                                torch.full((n,), 0.5, dtype=torch.float64), torch.zeros((n, 4), dtype=torch.float64),
                                torch.ones(n, dtype=torch.float64), **kw)


def test_step_stats_gain_num_born_with_default_zero():
    from mundy_amd import pipeline
    assert pipeline.StepStats().num_born == 0


def test_bacteria_step_app_compiles_and_links():
    # the C++ growth stepper (SpherocylinderStepper::set_growth) and its driver build on the CPU box
    import os
    from cpp_apps import build_app
    exe = build_app("bacteria_step_app")
    assert os.path.exists(exe)
