"""Crosslinkers that bind and unbind on the device (crosslink.hip) against the numpy model (crosslinker_model.py), the
stepper's carry of their state, the C++ driver and the full-size step."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import chain_model as cm
import crosslinker_model as xm
from gpu_util import (PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host, line_with_one_long_bond,
                      renumberings, star_and_random_graph, star_graph)

pytestmark = pytest.mark.gpu


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else
                            np.ascontiguousarray(a, dtype=np.int64)).cuda()


def _search(center, left, sites, cap, skin):
    """the stepper's candidate search on its own -> (links, CSR on the host)"""
    from mundy_amd import ops
    n = center.shape[0]
    src = np.zeros(n, np.uint8)
    src[left] = 1
    links = (ops.GenNeighborLinks().set_search_buffer(skin).set_search_kind(ops.SEARCH_SPHERES)
             .set_enforce_source_target_symmetry(True).acts_on(dev(src), dev(np.asarray(sites, np.uint8))).concretize())
    assert links.generate(None, center, torch.full((n,), 0.5 * cap, dtype=torch.float64, device=center.device))
    return links, src


def _handle(n, left, right, sites, p):
    from mundy_amd import ops
    return ops.Crosslinkers(n, left, right, sites, p["kind"], p["k"], p["r"], p["bind_rate"], p["unbind_rate"], p["kt"],
                            p["capture_radius"])


def _model_step(center, left, right, ptr, col, p, dt, keys, ctr):
    return xm.kmc_step(center, left, right, ptr, col, p["kind"], p["k"], p["r"], p["bind_rate"], p["unbind_rate"],
                       p["kt"], p["capture_radius"], dt, keys, ctr)


# ---- 1. rates and decisions --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hookean", "fene"])
def test_rates_and_decisions_against_the_model(kind):
    d = xm.decision_case(kind, xm.DECISION_SEEDS[kind])
    p, n, m = d["par"], d["center"].shape[0], d["left"].shape[0]
    center = dev(d["center"])
    links, src = _search(center, d["left"], d["sites"], p["capture_radius"], 0.2)
    ptr, col = host(links.row_ptr).astype(np.int64), host(links.col).astype(np.int64)
    row = np.repeat(np.arange(n), np.diff(ptr))
    # the list: sources' rows only, bind sites only, and every site within the capture radius
    assert src[row].all() and d["sites"][col].all() and (row != col).all()
    mptr, mcol = xm.candidate_rows(d["center"], src, d["sites"], p["capture_radius"])
    mrow = np.repeat(np.arange(n), np.diff(mptr))
    assert np.isin(mrow * n + mcol, row * n + col).all()
    assert col.shape[0] > mcol.shape[0]   # the buffer lists more: the kernel's own cut-off is at work
    xl = _handle(n, d["left"], d["right"], d["sites"], p)
    xl.set_candidates(links.row_ptr, links.col, dev(d["ids"]))
    keys, ctr = _i64(d["keys"]), _i64(d["counter"])
    z = torch.full((m,), -1.0, dtype=torch.float64, device="cuda")
    ev = host(xl.kmc_step(center, d["dt"], keys, ctr, z_total=z))
    res = _model_step(d["center"], d["left"], d["right"], ptr, xm.sort_rows_by_id(ptr, col, d["ids"]), p, d["dt"],
                      d["keys"].view(np.uint64), d["counter"].view(np.uint64))
    # the wider list changes nothing: the model on the exact lists gives the same sums
    exact = _model_step(d["center"], d["left"], d["right"], mptr, xm.sort_rows_by_id(mptr, mcol, d["ids"]), p, d["dt"],
                        d["keys"].view(np.uint64), d["counter"].view(np.uint64))
    assert_bits_equal(res["z_tot"], exact["z_tot"], "model z_tot, buffered vs exact list")
    assert (res["right"] == exact["right"]).all()
    zt = host(z)
    err = np.abs(zt - res["z_tot"])
    print("z_tot: max relative error %.3g" % float((err / np.maximum(res["z_tot"], 1e-300)).max()))
    assert (err <= 1e-13 * res["z_tot"]).all()
    out = xm.left_out(res)
    print("left out: %d of %d" % (int(out.sum()), m))
    assert out.sum() <= m // 10000
    _, right = xl.state("cuda")
    right = host(right).astype(np.int64)
    assert (right[~out] == res["right"][~out]).all()
    if not out.any():
        assert (int(ev[0]), int(ev[1])) == (res["binds"], res["unbinds"])
    assert (host(ctr) == d["counter"] + 1).all()
    assert (host(keys) == d["keys"]).all()


# ---- 2. forces ---------------------------------------------------------------------------------------------------------
def _force_case(rng, n=6000, m=9000):
    c = rng.uniform(0, 12.0, (n, 3))
    left = rng.integers(0, n // 2, m)           # several crosslinkers on one bead, the upper half of the beads anchors none
    right = left.copy()
    pick = rng.random(m) < 0.6
    right[pick] = rng.integers(0, (3 * n) // 4, int(pick.sum()))   # the last quarter has no crosslinker at all
    return c, left, right


@pytest.mark.parametrize("kind,r", [("hookean", 0.7), ("fene", 40.0)])
def test_crosslinker_forces_bit_for_bit(kind, r):
    rng = np.random.default_rng(21)
    c, left, right = _force_case(rng)
    n = c.shape[0]
    p = dict(kind=kind, k=3.5, r=r, bind_rate=1.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    xl = _handle(n, left, right, np.ones(n, np.uint8), p)
    f, over, mx = xl.force(dev(c))
    want, wover, wmx = xm.crosslinker_force(n, left, right, kind, p["k"], r, c)
    assert_bits_equal(host(f), want, "crosslinker force")
    assert int(over.item()) == wover == 0 and float(mx.item()) == wmx
    used = np.zeros(n, bool)
    used[left[right != left]] = True
    used[right[right != left]] = True
    assert (~used).sum() > n // 8 and (host(f)[~used].view(np.uint64) == 0).all()   # +0.0 exactly
    deg = np.bincount(np.concatenate([left[right != left], right[right != left]]), minlength=n)
    assert deg.max() >= 4
    # added into a backbone force
    base = rng.normal(size=(n, 3))
    acc = dev(base)
    xl.force(dev(c), out=acc, accumulate=True)
    assert_bits_equal(host(acc), base + want, "accumulate")


def test_matching_gets_exactly_negated_vectors_and_fene_overstretch_is_counted():
    rng = np.random.default_rng(22)
    m = 5000
    c = rng.uniform(0, 30.0, (2 * m, 3))
    c[1::2] = c[0::2] + rng.normal(size=(m, 3)) * 0.4
    left, right = 2 * np.arange(m), 2 * np.arange(m) + 1
    L = xm.distance(c[right], c[left])
    p = dict(kind="fene", k=2.0, r=1.2, bind_rate=1.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    xl = _handle(2 * m, left, right, np.ones(2 * m, np.uint8), p)
    f, over, mx = xl.force(dev(c))
    f = host(f)
    ok = L < p["r"]
    assert 0 < (~ok).sum() < m and int(over.item()) == int((~ok).sum()) and float(mx.item()) == L.max()
    assert_bits_equal(f[left][ok], -f[right][ok], "negation")
    assert np.isnan(f[left][~ok]).all() and np.isnan(f[right][~ok]).all()
    want, _, _ = xm.crosslinker_force(2 * m, left, right, "fene", p["k"], p["r"], c)
    # (a NaN has no bits to pin: whether 0 - NaN keeps or flips the sign of the payload is the adder's business, and the
    #  host's and the device's differ; the overstretched rows are NaN in both, every other row agrees bit for bit)
    assert (np.isnan(want) == np.isnan(f)).all()
    assert_bits_equal(f[np.repeat(ok, 2)], want[np.repeat(ok, 2)], "fene matching")


# ---- 3. incidence after events -----------------------------------------------------------------------------------------
def test_force_after_events_equals_a_fresh_handle():
    d = xm.decision_case("hookean", 31, n=20000, m=30000)
    p, n = d["par"], d["center"].shape[0]
    center = dev(d["center"])
    links, _ = _search(center, d["left"], d["sites"], p["capture_radius"], 0.1)
    xl = _handle(n, d["left"], d["right"], d["sites"], p)
    xl.set_candidates(links.row_ptr, links.col, dev(d["ids"]))
    keys, ctr = _i64(d["keys"]), _i64(d["counter"])
    total = np.zeros(2, np.int64)
    for _ in range(6):
        ev = host(xl.kmc_step(center, d["dt"], keys, ctr))
        assert ev[0] > 0 and ev[1] > 0
        total += ev
        le, ri = (host(t).astype(np.int64) for t in xl.state("cuda"))
        assert (le == d["left"]).all()
        fresh = _handle(n, le, ri, d["sites"], p)
        f = host(xl.force(center)[0])
        assert_bits_equal(f, host(fresh.force(center)[0]), "fresh handle")
        assert_bits_equal(f, xm.crosslinker_force(n, le, ri, "hookean", p["k"], p["r"], d["center"])[0], "model")
        fresh.close()
    assert int((ri != le).sum()) == int((d["right"] != d["left"]).sum()) + total[0] - total[1]


# ---- 3b. the helpers shared with the other force kernels: statistic epilogue, incidence build ------------------------
PAR = dict(kind="hookean", k=5.0, r=0.5, bind_rate=2.0, unbind_rate=6.0, kt=1.0, capture_radius=1.0)


@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_crosslinker_max_length_is_found_wherever_it_sits(pos):
    n = PAST_FULL_GRID
    c, pairs = line_with_one_long_bond(pos)   # the left ends take the statistics
    xl = _handle(n, pairs[:, 0], pairs[:, 1], np.ones(n, np.uint8), PAR)
    f, over, mx = xl.force(dev(c))
    want, wover, wmx = xm.crosslinker_force(n, pairs[:, 0], pairs[:, 1], "hookean", PAR["k"], PAR["r"], c)
    assert wmx == 1.5 and float(mx.item()) == wmx and int(over.item()) == wover == 0
    assert_bits_equal(host(f), want, "line, long crosslinker at %d" % pos)
    xl.close()


@pytest.mark.parametrize("case", ["no crosslinkers", "one body", "star", "all singly bound"])
def test_crosslinker_incidence_empty_and_star(case):
    rng = np.random.default_rng(32)
    none = np.zeros(0, np.int64)
    if case == "star":
        n, pairs = star_graph()
        left, right = pairs[:, 0], pairs[:, 1]
    elif case == "all singly bound":   # the right incidence is empty, the left one is not
        n = 121
        left = rng.integers(0, 100, 300)
        right = left.copy()
    else:
        n, left, right = (5 if case == "no crosslinkers" else 1), none, none
    c = rng.normal(size=(n, 3))
    xl = _handle(n, left, right, np.ones(n, np.uint8), PAR)
    f, over, mx = xl.force(dev(c))
    want, wover, wmx = xm.crosslinker_force(n, left, right, "hookean", PAR["k"], PAR["r"], c)
    assert_bits_equal(host(f), want, case)
    assert int(over.item()) == wover == 0
    assert np.float64(mx.item()).view(np.uint64) == np.float64(wmx).view(np.uint64)
    if case == "star":
        assert all_pos_zero(host(f)[101:]) and wmx > 0
        base = -np.zeros((n, 3))
        base[:101] = rng.normal(size=(101, 3))
        acc = dev(base)
        xl.force(dev(c), out=acc, accumulate=True)
        assert_bits_equal(host(acc)[:101], (base + want)[:101], "accumulate")
    else:
        assert all_pos_zero(host(f)) and all_pos_zero(host(mx))
    xl.close()


@pytest.fixture(scope="module")
def renumber_case():
    """the star and a random graph of 3000 bodies as doubly bound crosslinkers, 2000 singly bound ones, in a box dense
    enough for tens of candidates per row"""
    rng = np.random.default_rng(33)
    n, pairs = star_and_random_graph(rng)
    single = rng.integers(0, n, 2000)
    left = np.concatenate([pairs[:, 0], single]).astype(np.int64)
    right = np.concatenate([pairs[:, 1], single]).astype(np.int64)
    m = left.shape[0]
    return dict(n=n, left=left, right=right, center=rng.uniform(0.0, 8.0, (n, 3)), perms=renumberings(rng, n),
                ids=rng.permutation(n).astype(np.int64), keys=rng.integers(0, 2 ** 63, m, dtype=np.int64),
                counter=rng.integers(0, 2 ** 40, m, dtype=np.int64))


@pytest.mark.parametrize("which", ["reversed", "random"])
def test_renumbered_crosslinkers_equal_a_fresh_handle(renumber_case, which):
    d = renumber_case
    n, new_of_old = d["n"], d["perms"][which]
    sites = np.ones(n, np.uint8)
    xl = _handle(n, d["left"], d["right"], sites, PAR)
    xl.renumber(dev(new_of_old))
    left, right = new_of_old[d["left"]].astype(np.int64), new_of_old[d["right"]].astype(np.int64)
    le, ri = (host(t).astype(np.int64) for t in xl.state("cuda"))
    assert (le == left).all() and (ri == right).all()
    fresh = _handle(n, left, right, sites, PAR)
    c = np.empty_like(d["center"])
    c[new_of_old] = d["center"]
    center = dev(c)
    f = host(xl.force(center)[0])
    assert_bits_equal(f, host(fresh.force(center)[0]), "fresh handle")
    want = xm.crosslinker_force(n, d["left"], d["right"], "hookean", PAR["k"], PAR["r"], d["center"])[0]
    assert_bits_equal(f[new_of_old], want, "model in the old numbering")
    # one KMC step on the same candidates and streams: the same events, the same state, the same force afterwards
    links, _ = _search(center, left, sites, PAR["capture_radius"], 0.1)
    out = []
    for h in (xl, fresh):
        h.set_candidates(links.row_ptr, links.col, dev(d["ids"]))
        keys, ctr = _i64(d["keys"]), _i64(d["counter"])
        ev = host(h.kmc_step(center, 0.05, keys, ctr))
        out.append((ev, host(h.state("cuda")[1]), host(h.force(center)[0])))
    assert out[0][0][0] > 0 and out[0][0][1] > 0
    assert (out[0][0] == out[1][0]).all() and (out[0][1] == out[1][1]).all()
    assert_bits_equal(out[0][2], out[1][2], "force after the step")
    xl.close()
    fresh.close()


# ---- 4. statistics -----------------------------------------------------------------------------------------------------
def _pair_lattice(m, offsets, spacing=4.0):
    """m groups of (left bead, sites at left + offsets[k]) on a cubic lattice, far from each other"""
    g = 1 + len(offsets)
    side = int(math.ceil(m ** (1.0 / 3.0)))
    idx = np.arange(m)
    base = np.stack([idx % side, (idx // side) % side, idx // (side * side)], axis=1) * spacing
    c = np.repeat(base, g, axis=0).astype(np.float64)
    for k, o in enumerate(offsets):
        c[1 + k::g] += np.asarray(o, dtype=np.float64)
    return c, g * idx


def test_stationary_bound_fraction_on_immobile_pairs_1e6():
    from mundy_amd import pipeline
    m, dsep, steps = 10 ** 6, 0.75, 40
    c, left = _pair_lattice(m, [(dsep, 0.0, 0.0)])
    n = c.shape[0]
    sites = np.zeros(n, np.uint8)
    sites[1::2] = 1
    p = dict(kind="hookean", k=5.0, r=0.5, bind_rate=8.0, unbind_rate=6.0, kt=1.0, capture_radius=1.0)
    dt = 0.05
    rng = np.random.default_rng(41)
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.25)), dt=dt, search_buffer=0.5, brownian_kt=0.1,
                                 mob_trans=torch.zeros(n, dtype=torch.float64, device="cuda"),
                                 crosslinkers=dict(left=left, sites=sites, skin=0.25,
                                                   keys=rng.integers(0, 2 ** 63, m, dtype=np.int64), **p))
    for _ in range(steps):
        s = st.step()
    assert_bits_equal(host(st.center), c, "immobile")
    d = xm.distance(c[1::2], c[0::2])
    assert (d == d[0]).all()
    p_on = 1.0 - math.exp(-dt * float(xm.rate("hookean", d[0], p["k"], p["r"], p["bind_rate"], p["kt"])))
    p_off = 1.0 - math.exp(-dt * p["unbind_rate"])
    assert (1.0 - p_on - p_off) ** steps < 1e-9   # mixed
    pi = p_on / (p_on + p_off)
    le, ri = (host(t) for t in st.crosslinker_state())
    frac = float((ri != le).mean())
    print("bound fraction %.6f, expected %.6f, sigma %.2g" % (frac, pi, math.sqrt(pi * (1 - pi) / m)))
    assert abs(frac - pi) < 5.0 * math.sqrt(pi * (1.0 - pi) / m)
    assert s.crosslinker_bound == int((ri != le).sum()) and (ri[ri != le] == le[ri != le] + 1).all()
    assert (host(st.xl_counter) == steps).all()


def test_chosen_site_frequencies_follow_the_rates_1e6():
    m = 10 ** 6
    offs = [(0.55, 0.0, 0.0), (0.0, 0.8, 0.0), (0.0, 0.0, -0.95)]
    c, left = _pair_lattice(m, offs)
    n = c.shape[0]
    sites = np.ones(n, np.uint8)
    sites[0::4] = 0
    p = dict(kind="hookean", k=5.0, r=0.5, bind_rate=6.0, unbind_rate=1.0, kt=1.0, capture_radius=1.0)
    dt = 0.05
    center = dev(c)
    links, _ = _search(center, left, sites, p["capture_radius"], 0.1)
    xl = _handle(n, left, None, sites, p)
    xl.set_candidates(links.row_ptr, links.col, None)
    keys = _i64(np.random.default_rng(42).integers(0, 2 ** 63, m, dtype=np.int64))
    ctr = torch.zeros(m, dtype=torch.int64, device="cuda")
    ev = host(xl.kmc_step(center, dt, keys, ctr))
    ri = host(xl.state("cuda")[1]).astype(np.int64)
    which = ri - left
    rates = np.array([float(xm.rate("hookean", xm.distance(c[1 + k], c[0]), p["k"], p["r"], p["bind_rate"], p["kt"]))
                      for k in range(3)])
    z = dt * rates.sum()
    nb = int((which > 0).sum())
    p_bind = 1.0 - math.exp(-z)
    assert ev[0] == nb and ev[1] == 0
    assert abs(nb - m * p_bind) < 5.0 * math.sqrt(m * p_bind * (1.0 - p_bind))
    for k in range(3):
        q = rates[k] / rates.sum()
        got = int((which == 1 + k).sum())
        print("site %d: %d of %d bound, expected share %.6f, got %.6f" % (k, got, nb, q, got / nb))
        assert abs(got - nb * q) < 5.0 * math.sqrt(nb * q * (1.0 - q))


def test_small_dt_occupancy_ratio_is_the_boltzmann_ratio_1e6():
    m, steps = 10 ** 6, 4500
    d1, d2 = 0.6, 0.9
    c, left = _pair_lattice(m, [(d1, 0.0, 0.0)])
    c[1::2][m // 2:, 0] += d2 - d1
    n = c.shape[0]
    sites = np.zeros(n, np.uint8)
    sites[1::2] = 1
    kt = 0.5
    p = dict(kind="hookean", k=4.0, r=0.5, bind_rate=1.3, unbind_rate=1.0, kt=kt, capture_radius=1.0)
    dt = 0.003
    center = dev(c)
    links, _ = _search(center, left, sites, p["capture_radius"], 0.1)
    xl = _handle(n, left, None, sites, p)
    xl.set_candidates(links.row_ptr, links.col, None)
    keys = _i64(np.random.default_rng(43).integers(0, 2 ** 63, m, dtype=np.int64))
    ctr = torch.zeros(m, dtype=torch.int64, device="cuda")
    ev = torch.zeros(2, dtype=torch.int32, device="cuda")
    for _ in range(steps):
        xl.kmc_step(center, dt, keys, ctr, events=ev)
    le, ri = (host(t) for t in xl.state("cuda"))
    bound = ri != le
    dd = xm.distance(c[1::2], c[0::2])
    a, b = dd < 0.75, dd > 0.75
    assert a.sum() == b.sum() == m // 2
    odds = [bound[s].sum() / (~bound[s]).sum() for s in (a, b)]
    var = sum(1.0 / (s.sum() * bound[s].mean() * (1.0 - bound[s].mean())) for s in (a, b))
    u = lambda d: 0.5 * p["k"] * (d - p["r"]) ** 2  # noqa: E731
    want = math.exp(-(u(dd[a][0]) - u(dd[b][0])) / kt)
    # finite dt: the odds are (1 - exp(-dt r_on)) / (1 - exp(-dt k_off)), whose ratio differs from r_1 / r_2 by the
    # factor 1 - dt (r_1 - r_2) / 2 + O(dt^2) < 0.3 sigma here; mixing: (1 - p_on - p_off)^steps < 1e-9
    r1, r2 = (float(xm.rate("hookean", dd[s][0], p["k"], p["r"], p["bind_rate"], kt)) for s in (a, b))
    assert dt * abs(r1 - r2) / 2.0 < 0.3 * math.sqrt(var)
    assert (1.0 - dt * (min(r1, r2) + p["unbind_rate"]) * 0.99) ** steps < 1e-9
    got = odds[0] / odds[1]
    print("odds ratio %.5f, Boltzmann %.5f, sigma (relative) %.2g" % (got, want, math.sqrt(var)))
    assert abs(got / want - 1.0) < 5.0 * math.sqrt(var)


# ---- 5. the stepper ----------------------------------------------------------------------------------------------------
def _chains(seed=5, side=6, beads=60):
    """side x side straight chains along x (spacing 1, beads of radius 0.3: no contacts) 1.2 apart, jittered; backbone
    springs, a crosslinker on every second bead, every bead a bind site"""
    rng = np.random.default_rng(seed)
    g = np.stack(np.meshgrid(np.arange(beads) * 1.0, np.arange(side) * 1.2, np.arange(side) * 1.2, indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3)) + rng.normal(size=(side * side * beads, 3)) * 0.03
    n = c.shape[0]
    first = (np.arange(side * side)[:, None] * beads + np.arange(beads - 1)[None, :]).reshape(-1)
    pairs = np.stack([first, first + 1], axis=1).astype(np.int32)
    left = np.arange(0, n, 2)
    keys = rng.permutation(2 ** 20)[:left.shape[0]].astype(np.int64)
    return c, pairs, left, keys


def _xl_stepper(skin=0.3, crosslinkers=True, bind_rate=300.0, model="lcp", **extra):
    from mundy_amd import pipeline
    c, pairs, left, keys = _chains()
    n = c.shape[0]
    kw = dict(dt=1e-3, viscosity=1.0, search_buffer=0.4, contact_model=model, springs=(pairs, "hookean", 3.0, 1.0),
              brownian_kt=0.1)
    if crosslinkers:
        kw["crosslinkers"] = dict(left=left, sites=np.ones(n, np.uint8), kind="hookean", k=3.0, r=1.0,
                                  bind_rate=bind_rate, unbind_rate=150.0, kt=0.1, capture_radius=1.5, skin=skin,
                                  keys=keys, **extra)
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.3)), **kw)


def _by_id(st):
    """(centres, right heads as ids, left heads as ids) in the order of the original ids"""
    ids = host(st.ids)
    order = np.argsort(ids)
    le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
    return host(st.center)[order], ids[ri], ids[le]


def test_stepper_trajectory_is_invariant_under_reorder_restore_and_skin():
    steps = 30
    a = _xl_stepper()
    binds = unbinds = 0
    for _ in range(steps):
        s = a.step()
        binds, unbinds = binds + s.crosslinker_binds, unbinds + s.crosslinker_unbinds
        # (no contact is active: the trajectories below do not hang on the sum order of a solve)
        assert float(a.contacts["sep"].min()) > 0.0
    ca, ra, la = _by_id(a)
    assert binds > 200 and unbinds > 50 and s.crosslinker_bound == binds - unbinds == int((ra != la).sum())
    assert s.max_crosslinker_length > 0
    # a reorder in the middle
    b = _xl_stepper()
    for _ in range(steps // 2):
        b.step()
    perm = b.reorder_bodies(curve="morton", cell_size=2.0)
    assert (host(perm) != np.arange(perm.shape[0])).any()
    for _ in range(steps - steps // 2):
        sb = b.step()
    cb, rb, lb = _by_id(b)
    assert_bits_equal(cb, ca, "centres after reorder_bodies")
    assert (rb == ra).all() and (lb == la).all() and sb.crosslinker_bound == s.crosslinker_bound
    assert (host(b.xl_counter) == steps).all()
    # through snapshot / restore
    c = _xl_stepper()
    for _ in range(10):
        c.step()
    snap = c.snapshot()
    for _ in range(7):
        c.step()
    c.restore(snap)
    for _ in range(steps - 10):
        sc = c.step()
    cc, rc, _ = _by_id(c)
    assert_bits_equal(cc, ca, "centres after restore")
    assert (rc == ra).all() and sc.crosslinker_bound == s.crosslinker_bound
    # another skin: the candidate list is rebuilt in other steps, the result is the same
    e = _xl_stepper(skin=0.04)
    for _ in range(steps):
        e.step()
    ce, re_, _ = _by_id(e)
    print("candidate list builds: skin 0.3 -> %d, skin 0.04 -> %d" % (a.crosslinker_rebuilds, e.crosslinker_rebuilds))
    assert e.crosslinker_rebuilds > a.crosslinker_rebuilds
    assert_bits_equal(ce, ca, "centres with another skin")
    assert (re_ == ra).all()


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_without_crosslinkers_the_stepper_is_todays(model):
    plain = _xl_stepper(crosslinkers=False, model=model)
    none = _xl_stepper(crosslinkers=False, model=model)
    none2 = type(plain)("sphere", plain.center.clone(), plain.radius.clone(), dt=1e-3, viscosity=1.0, search_buffer=0.4,
                        contact_model=model, springs=(_chains()[1], "hookean", 3.0, 1.0), brownian_kt=0.1,
                        crosslinkers=None)
    idle = _xl_stepper(bind_rate=0.0, model=model)   # crosslinkers that never bind: +0.0 added to every force
    assert plain.crosslinkers is None and plain._chain_stats.shape[0] == 3 and plain.ids is None
    for _ in range(5):
        sp = plain.step()
        none.step()
        none2.step()
        si = idle.step()
        assert_bits_equal(host(none.center), host(plain.center), "no keyword")
        assert_bits_equal(host(none2.center), host(plain.center), "crosslinkers=None")
        assert_bits_equal(host(idle.center), host(plain.center), "idle crosslinkers")
        assert si.crosslinker_binds == si.crosslinker_bound == 0 and sp.crosslinker_bound == 0
        assert si.max_spring_length == sp.max_spring_length
    assert (host(idle.xl_counter) == 5).all()


def test_crosslinkers_alone_make_a_chain_step():
    from mundy_amd import pipeline
    c, _, left, keys = _chains()
    n = c.shape[0]
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.3)), dt=1e-3, viscosity=1.0, search_buffer=0.4,
                                 crosslinkers=dict(left=left, sites=np.ones(n, np.uint8), kind="fene", k=0.1, r=2.5,
                                                   bind_rate=300.0, unbind_rate=150.0, kt=0.1, capture_radius=1.5,
                                                   skin=0.3, keys=keys))
    # (FENE weight (1 - (d / r_max)^2)^(k r_max^2 / 2 kT): exponent 3.1 here, so sites at d ~ 1 bind at a rate of ~170)
    x0 = c.copy()
    for _ in range(3):
        s = st.step()
        le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
        F, _, _ = xm.crosslinker_force(n, le, ri, "fene", 0.1, 2.5, x0)
        assert_bits_equal(host(st.spring_force), F, "force of the doubly bound set at the start of the step")
        x0 = host(st.center).copy()
    assert s.crosslinker_bound > 0 and st.rng_keys is not None


# ---- 6. the C++ driver -------------------------------------------------------------------------------------------------
def test_crosslinker_step_app_matches_python():
    from cpp_apps import build_app, checksums, fnv1a as fnv
    from mundy_amd import pipeline, synth
    d = synth.chains(2, 1000, seed=8)
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    left = np.arange(0, n, 2)
    sites = (np.arange(n) % 3 != 0).astype(np.uint8)
    xp = dict(k=3.0, r=1.0, bind_rate=200.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5, skin=0.5)
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"], crosslinkers=dict(left=left, sites=sites, kind="hookean", **xp))
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d bound %d binds %d unbinds %d" % (
            k, s.num_contacts, s.num_iters, s.crosslinker_bound, s.crosslinker_binds, s.crosslinker_unbinds))
    assert s.crosslinker_bound > 0 and sum(int(ln.split()[-1]) for ln in lines) > 0
    import tempfile
    exe = build_app("crosslinker_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0], left.shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            left.astype(np.int32).tofile(f)
            sites.tofile(f)
        args = [d["dt"], d["skin"], d["k"], d["r0"], d["kt"], xp["k"], xp["r"], xp["bind_rate"], xp["unbind_rate"],
                xp["kt"], xp["capture_radius"], xp["skin"]]
        out = subprocess.run([exe, path, "20"] + [repr(float(a)) for a in args], capture_output=True, text=True,
                             timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:12]) for g in got] == lines
    cs = checksums(out.stdout)
    assert cs["center"] == fnv(host(st.center).reshape(-1).view(np.uint64).tolist())
    assert cs["right"] == fnv(host(st.crosslinker_state()[1]).astype(np.int64).tolist())


# ---- 7. full size ------------------------------------------------------------------------------------------------------
def test_one_step_at_full_size():
    from mundy_amd import pipeline, synth
    d = synth.chains(1000, 1000, seed=3)
    n = d["center"].shape[0]
    left = np.arange(0, n, 2)
    m = left.shape[0]
    rng = np.random.default_rng(7)
    sites = (rng.random(n) < 0.7).astype(np.uint8)
    cap = 1.5
    # a tenth starts doubly bound, to the next bead along the chain where that is a site
    right = left.copy()
    pick = (rng.random(m) < 0.1) & (sites[np.minimum(left + 1, n - 1)] == 1) & ((left + 1) % 1000 != 0)
    right[pick] = left[pick] + 1
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"],
                                 crosslinkers=dict(left=left, right=right, sites=sites, kind="hookean", k=3.0, r=1.0,
                                                   bind_rate=100.0, unbind_rate=100.0, kt=0.1, capture_radius=cap,
                                                   skin=0.5))
    bound0 = int(pick.sum())
    assert n == 10 ** 6 and m == 5 * 10 ** 5 and st.crosslinker_bound == bound0
    s = st.step()
    assert s.num_bodies == n and s.converged
    le, ri = (host(t).astype(np.int64) for t in st.crosslinker_state())
    assert (le == left).all()
    b = ri != le
    assert s.crosslinker_binds > 1000 and s.crosslinker_unbinds > 1000
    assert s.crosslinker_bound == int(b.sum())
    assert s.crosslinker_binds - s.crosslinker_unbinds == int(b.sum()) - bound0
    new = b & (ri != right)
    assert int(new.sum()) == s.crosslinker_binds
    assert sites[ri[b]].all()
    assert (xm.distance(d["center"][ri[new]], d["center"][le[new]]) <= cap).all()   # at bind time: the step's start
    assert (host(st.xl_counter) == 1).all()
    # the force of the step: backbone + the doubly bound set after the KMC, at the positions of the start
    F, _, _ = cm.spring_force(n, d["pairs"], "hookean", d["k"], d["r0"], d["center"])
    X, _, mx = xm.crosslinker_force(n, le, ri, "hookean", 3.0, 1.0, d["center"])
    assert_bits_equal(host(st.spring_force), F + X, "spring + crosslinker force")
    assert s.max_crosslinker_length == mx
