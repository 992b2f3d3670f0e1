"""Periphery bind sites on the device (crosslink.hip: k_xl_kmc_periphery, k_xl_force_periphery, the right-end incidence
that leaves periphery-bound heads out) against the numpy model (periphery_binding_model.py), the stepper's carry of the
negative encoding, the C++ driver and the statistics of the two-row draw."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import chain_model as cm
import crosslinker_model as xm
import periphery_binding_model as pm
from gpu_util import assert_bits_equal, dev, host, renumberings

pytestmark = pytest.mark.gpu


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else
                            np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _search(center, left, sites, cap, skin):
    """the stepper's bead search on its own"""
    from mundy_amd import ops
    n = center.shape[0]
    src = np.zeros(n, np.uint8)
    src[left] = 1
    links = (ops.GenNeighborLinks().set_search_buffer(skin).set_search_kind(ops.SEARCH_SPHERES)
             .set_enforce_source_target_symmetry(True).acts_on(dev(src), dev(np.asarray(sites, np.uint8))).concretize())
    assert links.generate(None, center, torch.full((n,), 0.5 * cap, dtype=torch.float64, device=center.device))
    return links, src


def _site_search(center, src, points, cap, skin):
    """the stepper's site search on its own: beads followed by sites, sources the beads with a crosslinker, targets the
    sites -> (links, first n + 1 entries of row_ptr and the columns as site indices, on the host)"""
    from mundy_amd import ops
    n, P = center.shape[0], points.shape[0]
    allc = torch.cat([center, points])
    s = dev(np.concatenate([src, np.zeros(P, np.uint8)]))
    t = dev(np.concatenate([np.zeros(n, np.uint8), np.ones(P, np.uint8)]))
    links = (ops.GenNeighborLinks().set_search_buffer(skin).set_search_kind(ops.SEARCH_SPHERES)
             .set_enforce_source_target_symmetry(True).acts_on(s, t).concretize())
    assert links.generate(None, allc, torch.full((n + P,), 0.5 * cap, dtype=torch.float64, device=center.device))
    ptr, col = host(links.row_ptr).astype(np.int64), host(links.col).astype(np.int64)
    assert ptr[n] == ptr[-1] == col.shape[0] and (col >= n).all()   # the sites' own rows are empty
    return links, ptr[:n + 1], col - n


def _handle(n, left, right, sites, p, points, per):
    """a handle with sites; a periphery-bound initial state arrives through set_state"""
    from mundy_amd import ops
    right = np.asarray(left if right is None else right)
    xl = ops.Crosslinkers(n, left, np.where(right < 0, left, right), sites, p["kind"], p["k"], p["r"], p["bind_rate"],
                          p["unbind_rate"], p["kt"], p["capture_radius"])
    xl.set_periphery_sites(points if isinstance(points, torch.Tensor) else dev(points), per["A"], per["k"], per["r"],
                           per.get("k_off"), per["capture_radius"])
    if (right < 0).any():
        xl.set_state(None, dev(right.astype(np.int32)))
    return xl


def _state(xl):
    return tuple(host(t).astype(np.int64) for t in xl.state("cuda"))


# ---- 1. smallest shapes ------------------------------------------------------------------------------------------------
SMALL_P = dict(kind="hookean", k=5.0, r=0.5, bind_rate=8.0, unbind_rate=6.0, kt=1.0, capture_radius=1.0)
SMALL_PER = dict(A=6.0, k=4.0, r=0.4, k_off=9.0, capture_radius=1.2)


def small_case(m, P, seed=0):
    """crosslinker c on its own left bead c, with a partner bead m + c; c % 4 decides its rows: bit 0 a bead site within
    reach (the partner), bit 1 a periphery site within reach (site (c // 4) % P).  Beads with a site row sit next to
    their site on its +x side (no partner near) or its -x side (partner behind them); the others on a far lattice."""
    rng = np.random.default_rng(100 * m + P + seed)
    c = np.arange(m)
    kind = c % 4
    pts = np.stack([40.0 + 8.0 * np.arange(P), np.zeros(P), np.zeros(P)], axis=1)
    center = np.zeros((2 * m, 3))
    far = np.stack([-20.0 - 12.0 * (c // 16), 12.0 * ((c // 4) % 4), 12.0 * (c % 4) + 0.0 * c], axis=1).astype(np.float64)
    jit = rng.uniform(-0.1, 0.1, (m, 3))
    s = (c // 4) % P
    near = pts[s] + np.where(kind[:, None] == 2, 1.0, -1.0) * np.array([0.9, 0.0, 0.0]) + jit
    center[:m] = np.where((kind >= 2)[:, None], near, far + jit)
    partner = center[:m] - np.array([0.6, 0.0, 0.0])
    partner[kind % 2 == 0] = np.stack([-20.0 - 12.0 * (c // 16), 12.0 * ((c // 4) % 4) + 6.0, 12.0 * (c % 4)],
                                      axis=1)[kind % 2 == 0] + 300.0
    center[m:] = partner
    sites = np.concatenate([np.zeros(m, np.uint8), (kind % 2 == 1).astype(np.uint8)])
    if not sites.any():
        sites[m] = 1   # (a mask without a site is a valid input, but the bead search then has no target set)
    left = c.copy()
    right = left.copy()
    bead_bound = (c % 5 == 1) & (kind % 2 == 1)
    right[bead_bound] = m + c[bead_bound]
    site_bound = c % 7 == 3
    right[site_bound] = -((c[site_bound] % P) + 1)
    return dict(center=center, left=left, right=right, sites=sites, points=pts, kind=kind,
                keys=rng.integers(0, 2 ** 63, m, dtype=np.int64), counter=rng.integers(0, 2 ** 40, m, dtype=np.int64),
                dt=0.05)


def _model(d, p, per, ptr, col, pptr, pcol, right=None, ids=None):
    n = d["center"].shape[0]
    ids = np.arange(n) if ids is None else ids
    return pm.kmc_step(d["center"], d["left"], d["right"] if right is None else right, ptr,
                       xm.sort_rows_by_id(ptr, col, ids), pptr, pm.sort_rows(pptr, pcol), d["points"], pm.from_ops(p), per,
                       d["dt"], d["keys"].view(np.uint64), d["counter"].view(np.uint64))


@pytest.mark.parametrize("P", [1, 37])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_smallest_shapes_equal_the_model(m, P):
    d = small_case(m, P)
    n = 2 * m
    center, points = dev(d["center"]), dev(d["points"])
    links, src = _search(center, d["left"], d["sites"], SMALL_P["capture_radius"], 0.2)
    plinks, pptr, pcol = _site_search(center, src, points, SMALL_PER["capture_radius"], 0.2)
    ptr, col = host(links.row_ptr).astype(np.int64), host(links.col).astype(np.int64)
    res = _model(d, SMALL_P, SMALL_PER, ptr, col, pptr, pcol)
    assert not xm.left_out(res).any()
    if m >= 63:   # the four kinds of row, by what the model's sums saw
        free = d["right"] == d["left"]
        for a in (False, True):
            for b in (False, True):
                sel = free & ((res["z_beads"] > 0) == a) & ((res["z_tot"] > res["z_beads"]) == b)
                assert sel.sum() >= 3 and (d["kind"][sel] == a + 2 * b).all(), (a, b)
    xl = _handle(n, d["left"], d["right"], d["sites"], SMALL_P, points, SMALL_PER)
    xl.set_candidates(links.row_ptr, links.col, None)
    xl.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=n)
    keys, ctr = _i64(d["keys"]), _i64(d["counter"])
    z = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    pb = torch.full((1,), 1000, dtype=torch.int32, device="cuda")
    ev = host(xl.kmc_step(center, d["dt"], keys, ctr, z_total=z, periphery_bound=pb))
    le, ri = _state(xl)
    assert (le == d["left"]).all() and (ri == res["right"]).all()
    assert (int(ev[0]), int(ev[1])) == (res["binds"], res["unbinds"])
    assert int(pb.item()) == 1000 + res["periphery_bound"]   # added to
    assert (np.abs(host(z) - res["z_tot"]) <= 1e-13 * res["z_tot"]).all()
    assert (host(ctr) == d["counter"] + 1).all()
    f, over, mx = xl.force(center)
    want, wover, wmx, _ = pm.crosslinker_force(n, le, ri, "hookean", SMALL_P["k"], SMALL_P["r"], d["center"], d["points"])
    assert_bits_equal(host(f), want, "force after the step")
    assert int(over.item()) == wover and float(mx.item()) == wmx
    xl.close()


# ---- 2. rates and decisions ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hookean", "fene"])
def test_rates_and_decisions_against_the_model(kind):
    d = pm.decision_case(kind, pm.DECISION_SEEDS[kind])
    d["points"] = d["site_points"]
    p, per, n, m = d["par"], d["per"], d["center"].shape[0], d["left"].shape[0]
    center, points = dev(d["center"]), dev(d["points"])
    links, src = _search(center, d["left"], d["sites"], p["capture_radius"], 0.2)
    plinks, pptr, pcol = _site_search(center, src, points, per["capture_radius"], 0.2)
    ptr, col = host(links.row_ptr).astype(np.int64), host(links.col).astype(np.int64)
    # the site list: sources' rows only, every site within the periphery's capture radius, and more (the buffer)
    mptr, mcol = pm.site_rows(d["center"], src, d["points"], per["capture_radius"])
    row, mrow = np.repeat(np.arange(n), np.diff(pptr)), np.repeat(np.arange(n), np.diff(mptr))
    P = d["points"].shape[0]
    assert src[row].all() and np.isin(mrow * P + mcol, row * P + pcol).all() and pcol.shape[0] > mcol.shape[0] > 500
    xl = _handle(n, d["left"], d["right"], d["sites"], p, points, per)
    xl.set_candidates(links.row_ptr, links.col, dev(d["ids"]))
    xl.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=n)
    keys, ctr = _i64(d["keys"]), _i64(d["counter"])
    z = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    pb = torch.zeros(1, dtype=torch.int32, device="cuda")
    ev = host(xl.kmc_step(center, d["dt"], keys, ctr, z_total=z, periphery_bound=pb))
    res = _model(d, p, per, ptr, col, pptr, pcol, ids=d["ids"])
    exact = pm.kmc_step(d["center"], d["left"], d["right"], ptr, xm.sort_rows_by_id(ptr, col, d["ids"]), mptr, mcol,
                        d["points"], pm.from_ops(p), per, d["dt"], d["keys"].view(np.uint64), d["counter"].view(np.uint64))
    assert_bits_equal(res["z_tot"], exact["z_tot"], "model z_tot, buffered vs exact site list")
    assert (res["right"] == exact["right"]).all()
    zt = host(z)
    err = np.abs(zt - res["z_tot"])
    print("z_tot: max relative error %.3g" % float((err / np.maximum(res["z_tot"], 1e-300)).max()))
    assert (err <= 1e-13 * res["z_tot"]).all()
    assert not xm.left_out(res).any()   # the seeds were chosen so (tests/test_periphery_binding_host.py)
    le, ri = _state(xl)
    assert (le == d["left"]).all() and (ri == res["right"]).all()
    new = ri != d["right"]
    print("binds: %d to beads, %d to sites; unbinds %d; periphery-bound %d" % (
        int((new & (ri >= 0) & (ri != le)).sum()), int((new & (ri < 0)).sum()), res["unbinds"], res["periphery_bound"]))
    assert (new & (ri < 0)).sum() > 20
    assert (int(ev[0]), int(ev[1])) == (res["binds"], res["unbinds"])
    assert int(pb.item()) == res["periphery_bound"] == int((ri < 0).sum())
    assert (host(ctr) == d["counter"] + 1).all() and (host(keys) == d["keys"]).all()
    # the old entry point on a handle with sites is this call without the count
    xl.set_state(None, dev(d["right"].astype(np.int32)))
    ctr2 = _i64(d["counter"])
    ev2 = host(xl.kmc_step(center, d["dt"], keys, ctr2))
    assert (ev2 == ev).all() and (_state(xl)[1] == ri).all()
    xl.close()


# ---- 3. forces -------------------------------------------------------------------------------------------------------
def _sum_bound(n, left, right, kind, k, r, c, pts):
    """the rounding a sum over all rows of the force can carry: every bead adds at most deg terms, the sum over the beads
    and over the sites adds rows in some order; every partial sum is below the sum T of the terms' magnitudes"""
    b = right != left
    far = np.where(right < 0, n - (right + 1), right)
    term, _ = cm.spring_terms(np.stack([left[b], far[b]], axis=1), kind, k, r, np.concatenate([c, pts]))
    T = np.abs(term).sum(axis=0)
    deg = np.bincount(np.concatenate([left[b], far[b]])).max()
    return np.finfo(np.float64).eps * (2.0 * deg + 2.0 * (n + pts.shape[0])) * T


def test_forces_with_beads_and_sites_on_one_bead_bit_for_bit():
    rng = np.random.default_rng(51)
    n, m, P = 3000, 6000, 37
    c = rng.uniform(0, 9.0, (n, 3))
    pts = rng.uniform(-1.0, 10.0, (P, 3))
    left = rng.integers(0, n // 2, m)
    right = left.copy()
    u = rng.random(m)
    right[u < 0.4] = rng.integers(0, (3 * n) // 4, int((u < 0.4).sum()))
    right[u > 0.7] = -(rng.integers(0, P, int((u > 0.7).sum())) + 1)
    p = dict(kind="hookean", k=3.5, r=0.7, bind_rate=1.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    per = dict(A=1.0, k=2.0, r=0.3, capture_radius=1.0)
    xl = _handle(n, left, right, np.ones(n, np.uint8), p, pts, per)
    f, over, mx = xl.force(dev(c))
    want, wover, wmx, fs = pm.crosslinker_force(n, left, right, "hookean", p["k"], p["r"], c, pts)
    assert_bits_equal(host(f), want, "force")
    assert int(over.item()) == wover == 0 and float(mx.item()) == wmx
    both = np.intersect1d(left[(right >= 0) & (right != left)], left[right < 0])
    assert both.size > 100   # beads that hold bead-bound and site-bound crosslinkers alike
    # the sum over the beads is no longer zero: it is the negated sum of what the sites would have received
    total, lost = host(f).sum(axis=0), fs.sum(axis=0)
    assert (np.abs(total) > 1.0).all()
    assert (np.abs(total + lost) <= _sum_bound(n, left, right, "hookean", p["k"], p["r"], c, pts)).all()
    base = rng.normal(size=(n, 3))
    acc = dev(base)
    xl.force(dev(c), out=acc, accumulate=True)
    assert_bits_equal(host(acc), base + want, "accumulate")
    xl.close()


def test_a_bead_whose_only_crosslinker_is_site_bound():
    c = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0], [5.0, 5.0, 5.0], [7.0, 7.0, 7.0]])
    pts = np.array([[0.0, 0.0, 3.0], [9.0, 9.0, 9.0]])
    left, right = np.array([0, 3, 1]), np.array([1, -1, 1])
    p = dict(kind="hookean", k=2.0, r=0.5, bind_rate=1.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    xl = _handle(5, left, right, np.ones(5, np.uint8), p, pts, dict(A=1.0, k=1.0, r=0.3, capture_radius=1.0))
    f, over, mx = xl.force(dev(c))
    want, _, wmx, fs = pm.crosslinker_force(5, left, right, "hookean", 2.0, 0.5, c, pts)
    assert_bits_equal(host(f), want, "force")
    d = pts[0] - c[3]
    L = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    assert (host(f)[3] == 0.0 + 2.0 * (L - 0.5) * (1.0 / L) * d).all() and float(mx.item()) == wmx == L
    assert (host(f)[[2, 4]].view(np.uint64) == 0).all()   # +0.0: no crosslinker at all
    assert (host(f).sum(axis=0) == -fs.sum(axis=0)).all() and (fs[1] == 0).all()
    xl.close()


def test_fene_overstretch_of_site_bound_crosslinkers_is_counted():
    rng = np.random.default_rng(52)
    m, P = 3000, 37
    pts = rng.uniform(0.0, 30.0, (P, 3))
    s = rng.integers(0, P, m)
    c = pts[s] + rng.normal(size=(m, 3)) * 0.6
    left, right = np.arange(m), -(s + 1)
    right[::3] = left[::3]   # a third singly bound
    p = dict(kind="fene", k=2.0, r=1.2, bind_rate=1.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    xl = _handle(m, left, right, np.ones(m, np.uint8), p, pts, dict(A=1.0, k=1.0, r=2.0, capture_radius=1.0))
    f, over, mx = xl.force(dev(c))
    f = host(f)
    want, wover, wmx, _ = pm.crosslinker_force(m, left, right, "fene", 2.0, 1.2, c, pts)
    L = xm.distance(pts[s], c)
    bound = right < 0
    bad = bound & ~(L < 1.2)
    assert 0 < bad.sum() < bound.sum() and int(over.item()) == wover == int(bad.sum())
    assert float(mx.item()) == wmx == L[bound].max()
    assert np.isnan(f[bad]).all() and (np.isnan(want) == np.isnan(f)).all()
    assert_bits_equal(f[~bad], want[~bad], "fene")
    xl.close()


# ---- 4. incidence after events, and renumbering --------------------------------------------------------------------
def test_force_after_six_steps_with_events_equals_a_fresh_handle():
    d = pm.decision_case("hookean", 31, n=8000, m=12000, P=200)
    p, per, n = d["par"], d["per"], d["center"].shape[0]
    center, points = dev(d["center"]), dev(d["site_points"])
    links, src = _search(center, d["left"], d["sites"], p["capture_radius"], 0.1)
    plinks, _, _ = _site_search(center, src, points, per["capture_radius"], 0.1)
    xl = _handle(n, d["left"], d["right"], d["sites"], p, points, per)
    xl.set_candidates(links.row_ptr, links.col, dev(d["ids"]))
    xl.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=n)
    keys, ctr = _i64(d["keys"]), _i64(d["counter"])
    total = np.zeros(2, np.int64)
    to_site = 0
    prev = d["right"]
    for _ in range(6):
        pb = torch.zeros(1, dtype=torch.int32, device="cuda")
        ev = host(xl.kmc_step(center, d["dt"], keys, ctr, periphery_bound=pb))
        assert ev[0] > 0 and ev[1] > 0
        total += ev
        le, ri = _state(xl)
        assert (le == d["left"]).all() and int(pb.item()) == int((ri < 0).sum())
        to_site += int(((ri < 0) & (ri != prev)).sum())
        prev = ri
        fresh = _handle(n, le, ri, d["sites"], p, points, per)
        f = host(xl.force(center)[0])
        assert_bits_equal(f, host(fresh.force(center)[0]), "fresh handle")
        assert_bits_equal(f, pm.crosslinker_force(n, le, ri, "hookean", p["k"], p["r"], d["center"], d["site_points"])[0],
                          "model")
        fresh.close()
    assert to_site > 20
    assert int((ri != le).sum()) == int((d["right"] != d["left"]).sum()) + total[0] - total[1]
    xl.close()


@pytest.mark.parametrize("which", ["reversed", "random"])
def test_every_crosslinker_site_bound_then_renumber(which):
    rng = np.random.default_rng(53)
    n, m, P = 3000, 5000, 37
    c = rng.uniform(0.0, 8.0, (n, 3))
    pts = rng.uniform(0.0, 8.0, (P, 3))
    left = rng.integers(0, n, m)
    right = -(rng.integers(0, P, m) + 1)
    new_of_old = renumberings(rng, n)[which]
    p = dict(kind="hookean", k=5.0, r=0.5, bind_rate=2.0, unbind_rate=6.0, kt=1.0, capture_radius=1.0)
    per = dict(A=3.0, k=4.0, r=0.4, capture_radius=1.2)
    xl = _handle(n, left, right, np.ones(n, np.uint8), p, pts, per)
    before = host(xl.force(dev(c))[0])
    assert_bits_equal(before, pm.crosslinker_force(n, left, right, "hookean", 5.0, 0.5, c, pts)[0], "model")
    xl.renumber(dev(new_of_old))
    le, ri = _state(xl)
    assert (le == new_of_old[left]).all() and (ri == right).all()   # the heads at the sites keep their values
    c2 = np.empty_like(c)
    c2[new_of_old] = c
    after, over, mx = xl.force(dev(c2))
    assert_bits_equal(host(after)[new_of_old], before, "force after renumber")
    assert int(over.item()) == 0 and float(mx.item()) > 0
    # both candidate lists were dropped with the numbering
    keys, ctr = _i64(np.arange(m)), torch.zeros(m, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="set_candidates"):
        xl.kmc_step(dev(c2), 0.05, keys, ctr)
    links, src = _search(dev(c2), le, np.ones(n, np.uint8), 1.0, 0.1)
    xl.set_candidates(links.row_ptr, links.col, None)
    with pytest.raises(RuntimeError, match="set_periphery_candidates"):
        xl.kmc_step(dev(c2), 0.05, keys, ctr)
    plinks, pptr, pcol = _site_search(dev(c2), src, dev(pts), 1.2, 0.1)
    xl.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=n)
    ev = host(xl.kmc_step(dev(c2), 0.05, keys, ctr))
    ptr, col = host(links.row_ptr).astype(np.int64), host(links.col).astype(np.int64)
    res = pm.kmc_step(c2, le, ri, ptr, xm.sort_rows_by_id(ptr, col, np.arange(n)), pptr, pm.sort_rows(pptr, pcol), pts,
                      pm.from_ops(p), per, 0.05, np.arange(m, dtype=np.uint64), np.zeros(m, np.uint64))
    assert not xm.left_out(res).any() and (_state(xl)[1] == res["right"]).all()
    assert (int(ev[0]), int(ev[1])) == (0, res["unbinds"]) and res["unbinds"] > 500
    xl.close()


def _shared_right_case(m, n=130):
    """every second crosslinker doubly bound, to one of 11 beads that none has as its left: the right lists hold many
    crosslinkers each, so the per-body sort after the fill decides their order"""
    rng = np.random.default_rng(54 + m)
    c = np.arange(m)
    left = (c * 7) % 97
    right = np.where(c % 2 == 0, 100 + (c * 37) % 11, left)
    return rng.uniform(0.0, 4.0, (n, 3)), rng.uniform(0.0, 4.0, (37, 3)), left, right


# neither kind of site is ever bound to and nothing unbinds: a KMC step changes no head and rebuilds the right lists
QUIET_P = dict(kind="hookean", k=5.0, r=0.5, bind_rate=0.0, unbind_rate=0.0, kt=1.0, capture_radius=1.0)
QUIET_PER = dict(A=0.0, k=4.0, r=0.4, capture_radius=1.2)


@pytest.mark.parametrize("m", [1, 65, 257])
def test_right_incidence_is_the_same_with_and_without_sites(m):
    from mundy_amd import ops
    n = 130
    c, pts, left, right = _shared_right_case(m, n)
    if m > 1:
        assert np.bincount(right[right != left]).max() >= 3
    ones, p = np.ones(n, np.uint8), QUIET_P
    center = dev(c)
    with_sites = _handle(n, left, None, ones, p, pts, QUIET_PER)
    without = ops.Crosslinkers(n, left, left, ones, p["kind"], p["k"], p["r"], p["bind_rate"], p["unbind_rate"], p["kt"],
                               p["capture_radius"])

    def same(what, heads, pos):
        for xl in (with_sites, without):
            le, ri = _state(xl)
            assert (le == heads[0]).all() and (ri == heads[1]).all(), what
        fa, fb = with_sites.force(pos), without.force(pos)
        assert_bits_equal(host(fa[0]), host(fb[0]), what)
        assert int(fa[1].item()) == int(fb[1].item()) and float(fa[2].item()) == float(fb[2].item()), what
        return host(fa[0])

    for xl in (with_sites, without):
        xl.set_state(None, dev(right.astype(np.int32)))
    f0 = same("after set_state", (left, right), center)
    assert_bits_equal(f0, pm.crosslinker_force(n, left, right, "hookean", p["k"], p["r"], c, pts)[0], "model")
    links, src = _search(center, left, ones, p["capture_radius"], 0.1)
    plinks, _, _ = _site_search(center, src, dev(pts), QUIET_PER["capture_radius"], 0.1)
    with_sites.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=n)
    for xl in (with_sites, without):
        xl.set_candidates(links.row_ptr, links.col, None)
        ev = host(xl.kmc_step(center, 0.05, _i64(np.arange(m)), torch.zeros(m, dtype=torch.int64, device="cuda")))
        assert (ev == 0).all()
    assert_bits_equal(same("after a KMC step", (left, right), center), f0, "the step moved no head")
    new_of_old = renumberings(np.random.default_rng(0), n)["reversed"]
    for xl in (with_sites, without):
        xl.renumber(dev(new_of_old))
    c2 = np.empty_like(c)
    c2[new_of_old] = c
    f2 = same("after renumber", (new_of_old[left], new_of_old[right]), dev(c2))
    assert_bits_equal(f2[new_of_old], f0, "force after renumber")
    with_sites.close()
    without.close()


@pytest.mark.parametrize("m", [1, 65, 257])
def test_right_incidence_leaves_out_the_periphery_bound_among_the_bead_bound(m):
    n = 130
    c, pts, left, right = _shared_right_case(m, n)
    bound = np.flatnonzero(right != left)
    right[bound[::2]] = -((bound[::2] % pts.shape[0]) + 1)   # every second doubly bound one sits on a site instead
    xl = _handle(n, left, right, np.ones(n, np.uint8), QUIET_P, pts, QUIET_PER)
    le, ri = _state(xl)
    assert (le == left).all() and (ri == right).all() and (ri < 0).any()
    f, over, mx = xl.force(dev(c))
    want, wover, wmx, _ = pm.crosslinker_force(n, left, right, "hookean", QUIET_P["k"], QUIET_P["r"], c, pts)
    assert_bits_equal(host(f), want, "force")
    assert int(over.item()) == wover and float(mx.item()) == wmx
    xl.close()


def test_refusals_that_need_a_handle():
    from mundy_amd import ops
    n = 8
    c = dev(np.arange(3.0 * n).reshape(n, 3))
    pts = dev(np.zeros((3, 3)))
    xl = ops.Crosslinkers(n, [0, 1], None, np.ones(n, np.uint8), "fene", 5.0, 0.9, 2.0, 3.0, 1.0, 1.0)
    row_ptr = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    col = torch.zeros(0, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="set_periphery_sites"):
        xl.set_periphery_candidates(row_ptr, col)
    xl.set_candidates(row_ptr, col, None)
    keys, ctr = _i64(np.arange(2)), torch.zeros(2, dtype=torch.int64, device="cuda")
    pb = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="set_periphery_candidates"):
        xl.kmc_step(c, 0.05, keys, ctr, periphery_bound=pb)
    with pytest.raises(ValueError, match="r_max"):
        xl.set_periphery_sites(pts, 1.0, 1.0, 0.0)
    xl.set_periphery_sites(pts, 1.0, 1.0, 1.1)
    xl.set_periphery_sites(pts + 1.0, 1.0, 1.0, 1.1)   # the same P again: the sites move
    with pytest.raises(ValueError, match="earlier call"):
        xl.set_periphery_sites(dev(np.zeros((4, 3))), 1.0, 1.0, 1.1)
    xl.close()


# ---- 5. the stepper ------------------------------------------------------------------------------------------------------
def _chains(seed=5, side=6, beads=40):
    """side x side straight chains along x (spacing 1, beads of radius 0.3: no contacts) 1.2 apart, jittered, centred on
    the origin; backbone springs, a crosslinker on every second bead, every bead a bind site"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(beads) * 1.0, np.arange(side) * 1.2, np.arange(side) * 1.2, indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3)) + rng.normal(size=(side * side * beads, 3)) * 0.03
    c -= c.mean(axis=0)
    n = c.shape[0]
    first = (np.arange(side * side)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    pairs = np.stack([first, first + 1], axis=1).astype(np.int32)
    left = np.arange(0, n, 2)
    keys = rng.permutation(2 ** 20)[:left.shape[0]].astype(np.int64)
    return c, pairs, left, keys


RADIUS = 20.5   # the nucleus: the chains' ends (|x| <= 19.6, the corner chains at |c| < 20) are within reach of the wall


def _sites(count=2000, radius=RADIUS, seed=9):
    from mundy_amd import synth
    return synth.periphery_bind_sites("sphere", radius, count, seed=seed)


def _stepper(skin=0.3, sites="on", model="lcp", right=None, **extra):
    from mundy_amd import pipeline
    c, pairs, left, keys = _chains()
    n = c.shape[0]
    xl = dict(left=left, sites=np.ones(n, np.uint8), kind="hookean", k=3.0, r=1.0, bind_rate=300.0, unbind_rate=150.0,
              kt=0.1, capture_radius=1.5, skin=skin, keys=keys, **extra)
    if right is not None:
        xl["right"] = right
    if sites == "on":
        xl["periphery_sites"] = dict(points=_sites(), bind_rate=2000.0, k=0.5, r=0.8, unbind_rate=100.0, capture_radius=1.8)
    elif sites == "far":
        xl["periphery_sites"] = dict(points=_sites(radius=80.0), bind_rate=400.0, k=3.0, r=0.8)
    elif sites == "none":
        xl["periphery_sites"] = None
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.3)), dt=1e-3, viscosity=1.0, search_buffer=0.4,
                                   contact_model=model, springs=(pairs, "hookean", 3.0, 1.0), brownian_kt=0.1,
                                   periphery=dict(shape="sphere", radius=RADIUS, k=50.0), crosslinkers=xl)


def _by_id(st):
    """(centres, right heads as ids or -(s + 1), left heads as ids) in the order of the original ids"""
    ids = host(st.ids)
    order = np.argsort(ids)
    le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
    return host(st.center)[order], np.where(ri < 0, ri, ids[np.maximum(ri, 0)]), ids[le]


def test_stepper_trajectory_is_invariant_under_reorder_restore_and_skin():
    steps = 24
    c0, _, left, _ = _chains()
    # a periphery-bound initial state: every fourth of the 40 crosslinkers nearest to a site, each at its nearest site
    d2 = ((c0[left][:, None, :] - _sites()[None, :, :]) ** 2).sum(axis=2)
    first = np.argsort(d2.min(axis=1))[:40:4]
    right = left.copy()
    right[first] = -(d2.argmin(axis=1)[first] + 1)
    started = np.zeros(left.shape[0], bool)
    started[first] = True
    a = _stepper(right=right)
    assert a.crosslinker_bound == 10
    binds = unbinds = 0
    seen = 0
    for _ in range(steps):
        s = a.step()
        binds, unbinds = binds + s.crosslinker_binds, unbinds + s.crosslinker_unbinds
        seen = max(seen, s.crosslinker_periphery_bound)
        assert float(a.contacts["sep"].min()) > 0.0   # (no active contact: no solve's sum order in the trajectory)
    ca, ra, la = _by_id(a)
    assert binds > 200 and unbinds > 50 and s.crosslinker_bound == 10 + binds - unbinds == int((ra != la).sum())
    # (the last KMC step precedes the last state read by nothing: the count after it is the state's)
    assert s.crosslinker_periphery_bound == int((ra < 0).sum()) > 0 and seen >= s.crosslinker_periphery_bound
    assert int(((ra < 0) & ~started).sum()) > 0   # new tethers, not only the initial ones
    b = _stepper(right=right)
    for _ in range(steps // 2):
        b.step()
    perm = b.reorder_bodies(curve="morton", cell_size=2.0)
    assert (host(perm) != np.arange(perm.shape[0])).any()
    for _ in range(steps - steps // 2):
        sb = b.step()
    cb, rb, lb = _by_id(b)
    assert_bits_equal(cb, ca, "centres after reorder_bodies")
    assert (rb == ra).all() and (lb == la).all()
    assert (sb.crosslinker_bound, sb.crosslinker_periphery_bound) == (s.crosslinker_bound, s.crosslinker_periphery_bound)
    c = _stepper(right=right)
    for _ in range(8):
        c.step()
    snap = c.snapshot()
    assert (snap["_crosslinkers"][1] < 0).any()   # the snapshot carries the negative encoding
    for _ in range(5):
        c.step()
    c.restore(snap)
    for _ in range(steps - 8):
        sc = c.step()
    cc, rc, _ = _by_id(c)
    assert_bits_equal(cc, ca, "centres after restore")
    assert (rc == ra).all() and sc.crosslinker_bound == s.crosslinker_bound
    e = _stepper(skin=0.04, right=right)
    for _ in range(steps):
        e.step()
    ce, re_, _ = _by_id(e)
    print("site candidate list builds: skin 0.3 -> %d, skin 0.04 -> %d" % (a.crosslinker_site_rebuilds,
                                                                         e.crosslinker_site_rebuilds))
    assert e.crosslinker_site_rebuilds > a.crosslinker_site_rebuilds
    assert_bits_equal(ce, ca, "centres with another skin")
    assert (re_ == ra).all()
    # scale_periphery moves the wall, not the sites
    before = host(a.xl_site_points).copy()
    a.scale_periphery(0.99)
    a.step()
    assert_bits_equal(host(a.xl_site_points), before, "sites after scale_periphery")


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_without_sites_the_stepper_is_todays(model):
    plain, none, far = (_stepper(sites=s, model=model) for s in ("absent", "none", "far"))
    assert plain.xl_site_links is None and none.xl_site_links is None and far.xl_site_links is not None
    for _ in range(6):
        sp = plain.step()
        none.step()
        sf = far.step()
        assert_bits_equal(host(none.center), host(plain.center), "periphery_sites=None")
        assert_bits_equal(host(far.center), host(plain.center), "sites all out of reach")
        assert (host(far.crosslinker_state()[1]) == host(plain.crosslinker_state()[1])).all()
        assert (host(none.crosslinker_state()[1]) == host(plain.crosslinker_state()[1])).all()
        assert (sf.crosslinker_binds, sf.crosslinker_unbinds, sf.crosslinker_bound) == (
            sp.crosslinker_binds, sp.crosslinker_unbinds, sp.crosslinker_bound)
        assert sf.crosslinker_periphery_bound == sp.crosslinker_periphery_bound == 0
        assert sf.max_crosslinker_length == sp.max_crosslinker_length
    assert sp.crosslinker_bound > 0


# ---- 6. the C++ driver ---------------------------------------------------------------------------------------------------
def test_periphery_binding_step_app_matches_python():
    from cpp_apps import build_app, checksums, fnv1a as fnv
    from mundy_amd import pipeline, synth
    d = synth.chains(2, 1000, seed=8)
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    left = np.arange(0, n, 2)
    sites = (np.arange(n) % 3 != 0).astype(np.uint8)
    xp = dict(k=3.0, r=1.0, bind_rate=200.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5, skin=0.5)
    # sites next to every 20th bead: tethers form from the first step on
    pts = np.ascontiguousarray(d["center"][::20] + np.array([0.0, 0.0, 0.7]))
    pp = dict(bind_rate=300.0, k=3.0, r=0.8, unbind_rate=80.0, capture_radius=1.6)
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"],
                                 crosslinkers=dict(left=left, sites=sites, kind="hookean",
                                                   periphery_sites=dict(points=pts, **pp), **xp))
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d bound %d binds %d unbinds %d periphery_bound %d" % (
            k, s.num_contacts, s.num_iters, s.crosslinker_bound, s.crosslinker_binds, s.crosslinker_unbinds,
            s.crosslinker_periphery_bound))
    assert s.crosslinker_periphery_bound > 0 and s.crosslinker_bound > s.crosslinker_periphery_bound
    import tempfile
    exe = build_app("periphery_binding_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0], left.shape[0], pts.shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            left.astype(np.int32).tofile(f)
            sites.tofile(f)
            pts.astype(np.float64).tofile(f)
        args = [d["dt"], d["skin"], d["k"], d["r0"], d["kt"], xp["k"], xp["r"], xp["bind_rate"], xp["unbind_rate"],
                xp["kt"], xp["capture_radius"], xp["skin"], pp["bind_rate"], pp["k"], pp["r"], pp["unbind_rate"],
                pp["capture_radius"]]
        out = subprocess.run([exe, path, "20"] + [repr(float(a)) for a in args], capture_output=True, text=True,
                             timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:14]) for g in got] == lines
    cs = checksums(out.stdout)
    assert cs["center"] == fnv(host(st.center).reshape(-1).view(np.uint64).tolist())
    # (the app's checksum runs over the 32-bit patterns, zero-extended: a head at a site is a negative int32)
    assert cs["right"] == fnv(host(st.crosslinker_state()[1]).astype(np.int32).view(np.uint32).tolist())


# ---- 7. statistics on 10^5 immobile beads ------------------------------------------------------------------------------
def _lattice(m, offsets, spacing=4.0):
    side = int(math.ceil(m ** (1.0 / 3.0)))
    idx = np.arange(m)
    base = (np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1) * spacing).astype(np.float64)
    return base, [base + np.asarray(o, dtype=np.float64) for o in offsets]


def test_stationary_periphery_bound_fraction_on_immobile_beads_1e5():
    from mundy_amd import pipeline
    m, dsep, steps, dt = 10 ** 5, 0.75, 40, 0.05
    c, (pts,) = _lattice(m, [(dsep, 0.0, 0.0)])
    p = dict(kind="hookean", k=5.0, r=0.5, bind_rate=8.0, unbind_rate=3.0, kt=1.0, capture_radius=1.0)
    per = dict(bind_rate=8.0, k=4.0, r=0.45, unbind_rate=6.0, capture_radius=1.1)
    rng = np.random.default_rng(61)
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(m, 0.25)), dt=dt, search_buffer=0.5, brownian_kt=0.1,
                                 mob_trans=torch.zeros(m, dtype=torch.float64, device="cuda"),
                                 crosslinkers=dict(left=np.arange(m), sites=np.zeros(m, np.uint8), skin=0.25,
                                                   keys=rng.integers(0, 2 ** 63, m, dtype=np.int64),
                                                   periphery_sites=dict(points=pts, **per), **p))
    for _ in range(steps):
        s = st.step()
    assert_bits_equal(host(st.center), c, "immobile")
    d = xm.distance(pts, c)
    assert (d == d[0]).all()
    p_on = 1.0 - math.exp(-dt * float(xm.rate("hookean", d[0], per["k"], per["r"], per["bind_rate"], p["kt"])))
    p_off = 1.0 - math.exp(-dt * per["unbind_rate"])   # the periphery's own rate, not the crosslinkers' 3.0
    assert (1.0 - p_on - p_off) ** steps < 1e-9   # mixed
    pi = p_on / (p_on + p_off)
    le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
    frac = float((ri < 0).mean())
    print("periphery-bound fraction %.6f, expected %.6f, sigma %.2g" % (frac, pi, math.sqrt(pi * (1 - pi) / m)))
    assert abs(frac - pi) < 5.0 * math.sqrt(pi * (1.0 - pi) / m)
    assert ((ri == le) | (ri == -(np.arange(m) + 1))).all()
    assert s.crosslinker_periphery_bound == s.crosslinker_bound == int((ri < 0).sum())
    assert (host(st.xl_counter) == steps).all()


def test_bead_and_site_are_chosen_in_the_ratio_of_their_rates_1e5():
    m, dt = 10 ** 5, 0.05
    base, (partner, pts) = _lattice(m, [(0.55, 0.0, 0.0), (0.0, 0.8, 0.0)])
    c = np.concatenate([base, partner])
    sites = np.concatenate([np.zeros(m, np.uint8), np.ones(m, np.uint8)])
    p = dict(kind="hookean", k=5.0, r=0.5, bind_rate=6.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    per = dict(A=18.0, k=3.0, r=0.4, capture_radius=1.0)   # (rates 5.96 to the bead, 14.2 to the site)
    center, points = dev(c), dev(pts)
    left = np.arange(m)
    links, src = _search(center, left, sites, 1.0, 0.1)
    plinks, _, _ = _site_search(center, src, points, 1.0, 0.1)
    xl = _handle(2 * m, left, None, sites, p, points, per)
    xl.set_candidates(links.row_ptr, links.col, None)
    xl.set_periphery_candidates(plinks.row_ptr, plinks.col, col_offset=2 * m)
    keys = _i64(np.random.default_rng(62).integers(0, 2 ** 63, m, dtype=np.int64))
    ctr = torch.zeros(m, dtype=torch.int64, device="cuda")
    pb = torch.zeros(1, dtype=torch.int32, device="cuda")
    ev = host(xl.kmc_step(center, dt, keys, ctr, periphery_bound=pb))
    ri = _state(xl)[1]
    rb = float(xm.rate("hookean", xm.distance(partner[0], base[0]), p["k"], p["r"], p["bind_rate"], p["kt"]))
    rs = float(xm.rate("hookean", xm.distance(pts[0], base[0]), per["k"], per["r"], per["A"], p["kt"]))
    to_bead, to_site = int((ri == left + m).sum()), int((ri == -(left + 1)).sum())
    nb = to_bead + to_site
    p_bind = 1.0 - math.exp(-dt * (rb + rs))
    assert ev[0] == nb and ev[1] == 0 and int(pb.item()) == to_site and int((ri != left).sum()) == nb
    assert abs(nb - m * p_bind) < 5.0 * math.sqrt(m * p_bind * (1.0 - p_bind))
    q = rs / (rb + rs)   # the ratio of chosen frequencies is the ratio of rates: the site's share of the binds
    print("binds %d: %d to the bead, %d to the site; site share %.5f, expected %.5f" % (nb, to_bead, to_site,
                                                                                     to_site / nb, q))
    assert abs(rb / rs - 1.0) > 0.2
    assert abs(to_site - nb * q) < 5.0 * math.sqrt(nb * q * (1.0 - q))
    xl.close()
