"""The conditions of the all-on HP1 case (tests/hp1_case.py), checked without a GPU: by the numpy models alone every
term of the step acts at step 0 from the initial state, in both contact modes.  The case's rates, capture radii and
seeds are chosen against this file, not against the device.  And the C++ driver of the case compiles and links.

The active dipoles are the one term that cannot act at step 0: a spring switches when elapsed >= next_time, the first
sampling sees elapsed = 0 and next_time = -log(u) / kon > 0, and neither stepper can be handed another initial state.
Their condition is therefore the earliest one that can hold: none is on at step 0, some are at step 1."""
import os

import numpy as np
import pytest

import hertz_model
import hp1_case as hp1
import hydro_model as hm
import hydro_periphery_model as hpm
import periphery_model as pm


def test_the_case_list():
    ids = [hp1.case_id(c) for c in hp1.CASES]
    assert ids == ["XYPAUWEH", "XYPAUWE", "PAUWEH", "XPAUWEH", "XYAUWEH", "XYPUWEH", "XYPAUEH", "XYPAEH", "XYPAUWH"]
    for c in hp1.CASES:
        assert hp1.check_letters(c) == c
    for bad in ("Y", "W", "XYZ"):
        with pytest.raises(ValueError):
            hp1.check_letters(bad)


def test_stepper_keywords_follow_the_letters():
    kw = hp1.stepper_kwargs(hp1.build(hp1.ALL))
    assert kw["contact_model"] == "hertz" and kw["hydrodynamics"]["contact_forces"] is True
    assert set(kw["hydrodynamics"]["periphery"]) == {"points", "weights", "normals"}
    assert kw["hydrodynamics"]["update_every"] == 2 and kw["hydrodynamics"]["kind"] == "rpyc"
    assert "right" not in kw["crosslinkers"] and "keys" not in kw["crosslinkers"] and "keys" not in kw["active_forces"]
    assert kw["crosslinkers"]["periphery_sites"]["points"].shape == (2000, 3)
    kw = hp1.stepper_kwargs(hp1.build("E"))
    assert kw["contact_model"] == "lcp"
    assert not any(k in kw for k in ("crosslinkers", "periphery", "active_forces", "hydrodynamics"))
    case = hp1.build(hp1.ALL - set("UW"))
    assert not case["first_term"] and "hydrodynamics" not in hp1.stepper_kwargs(case)
    assert hp1.build(hp1.ALL)["n"] <= 2000


@pytest.mark.parametrize("mode", ["lcp", "hertz"])
def test_every_term_acts_at_step_0(oracle, mode):
    case = hp1.build(hp1.ALL if mode == "hertz" else hp1.ALL - {"H"})
    n, x, r = case["n"], case["center"], case["radius"]
    left = case["xl"]["left"]
    # the geometry the terms hang on: every bead inside the no-slip surface, the end beads through the wall
    assert np.linalg.norm(x, axis=1).max() + r.max() < hp1.HYDRO_RADIUS - 1.0
    assert (left[1:] - left[:-1] == 2).all() and len(left) == n // 2
    # crosslinker KMC: a bind to a bead and a bind to a periphery site
    k = hp1.kmc(case, x, left, left, np.zeros(len(left), np.uint64))
    site_binds = k["periphery_bound"]
    print("%s: step 0 binds %d, of them %d to a site" % (mode, k["binds"], site_binds))
    assert k["binds"] - site_binds >= 1 and site_binds >= 1 and k["unbinds"] == 0
    # active dipoles: none at step 0 (see the module's text), some at step 1
    keys = np.arange(case["active_pairs"].shape[0], dtype=np.uint64)
    a0 = pm.active_init(keys, np.zeros(len(keys), np.uint64), case["active"]["kon"])
    a0, (on0, off0) = pm.active_sample(a0, keys, case["active"]["kon"], case["active"]["koff"])
    assert (a0["next_time"] > 0.0).all() and (on0, off0) == (0, 0)
    a1, (on1, _) = pm.active_sample(pm.active_advance(a0, case["dt"]), keys, case["active"]["kon"], case["active"]["koff"])
    assert on1 >= 1 and int(a1["state"].sum()) == on1
    Fa, count = pm.active_force(n, case["active_pairs"], a1["state"], case["active"]["sigma"], x)
    assert count == on1 and np.abs(Fa).max() > 0.0
    # Hertz mode: most beads are in an overlap, so the first term D f is non-zero on most
    Dlam = None
    if mode == "hertz":
        lo, hi, R = oracle.grow(oracle.compute_aabb_spheres(x, r), r, case["search_buffer"])
        pairs = oracle.search(oracle.SEARCH_AABB, lo, hi, x, R).reshape(-1, 2)
        sep, nrm = oracle.contact_spheres(pairs, x, r)
        touched = np.zeros(n, bool)
        touched[pairs[sep < 0.0].ravel()] = True
        print("hertz: %d of %d pairs overlap, %d of %d beads are in an overlap" % ((sep < 0).sum(), len(pairs),
                                                                                   touched.sum(), n))
        assert touched.sum() >= n // 2
        lam, _ = hertz_model.hertz_force(pairs, sep, r, case["youngs_modulus"], case["poisson_ratio"])
        Dlam = hp1.contact_force(case, pairs, lam, nrm)
        assert case["first_term"] and (np.abs(Dlam).max(axis=1) > 0).sum() >= n // 2
    # the force field of step 0: crosslinker, site-bound, wall and external terms all act
    F, info = hp1.force_field(case, x, (left, k["right"]), a0["state"], Dlam)
    assert info["acted"] == dict(X=True, Y=True, P=True, A=False, E=True), info["acted"]
    assert info["periphery_colliding"] > 0 and info["max_periphery_overlap"] > 0.0
    assert info["crosslinker_bound"] == k["binds"] and info["crosslinker_periphery_bound"] == site_binds
    # the hydrodynamic terms see that whole field: not the velocity of the spring force alone, and a correction
    u_full = hm.velocity("rpyc", case["viscosity"], x, r, F)
    u_springs = hm.velocity("rpyc", case["viscosity"], x, r, info["spring_force"])
    assert (u_full.view(np.uint64) != u_springs.view(np.uint64)).any(axis=1).sum() >= n // 2
    qp, qw, qn = case["quadrature"]
    corr = hpm.correct("rpyc", case["viscosity"], qp, qw, qn, hp1.periphery_inverse(case)[0], x, r, F)[0]
    assert np.isfinite(corr).all() and np.abs(corr).max() > 0.0
    assert (hp1.hydro_velocity(case, x, F).view(np.uint64) != u_full.view(np.uint64)).any(axis=1).sum() >= n // 2


def test_hp1_step_app_compiles_and_links():
    from cpp_apps import build_app
    exe = build_app("hp1_step_app")
    assert os.path.exists(exe)
