"""Bead-spring chains with Brownian motion on the GPU: the spring, Philox, Brownian and drag kernels against the numpy
restatement in tests/chain_model.py, the transpose sweep of the contact operator, and the chain step of the stepper
(spring closure, LCP with external velocities, Hertz, statistics of the noise, reorder / snapshot invariance, the C++
driver and one step at full size)."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import chain_model as cm
import friction_hertz_model as fm
import hertz_model as hm
from gpu_util import (PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host, line_with_one_long_bond,
                      star_graph)

pytestmark = pytest.mark.gpu

MASK63 = (1 << 63) - 1


def _u64_as_i64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


# ---- spring forces ---------------------------------------------------------------------------------------------------
def _graph(rng, name, n):
    if name == "chain":
        return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    if name == "random8":  # random graph, degree <= 8, a few isolated bodies
        deg = np.zeros(n, int)
        out = []
        for _ in range(3 * n):
            i, j = rng.integers(0, n - 5, 2)
            if i != j and deg[i] < 8 and deg[j] < 8:
                out.append((i, j))
                deg[i] += 1
                deg[j] += 1
        return np.array(out)
    if name == "matching":  # disjoint springs: each body one term, so the two ends are exact negatives
        p = rng.permutation(n)
        return np.stack([p[0::2], p[1::2]], axis=1)
    raise KeyError(name)


@pytest.mark.parametrize("kind", ["hookean", "fene"])
@pytest.mark.parametrize("per_spring", [False, True])
@pytest.mark.parametrize("graph", ["chain", "random8", "matching"])
def test_spring_forces_bit_for_bit(kind, per_spring, graph):
    from mundy_amd import ops
    rng = np.random.default_rng(hash((kind, per_spring, graph)) % 2 ** 32)
    n = 3001 if graph != "matching" else 3000
    pairs = _graph(rng, graph, n).astype(np.int32)
    m = pairs.shape[0]
    if graph == "chain":  # a random walk with bond lengths around 1
        steps = rng.normal(size=(n, 3))
        steps *= (rng.uniform(0.6, 1.3, n) / np.linalg.norm(steps, axis=1))[:, None]
        c = np.cumsum(steps, axis=0)
    else:
        c = rng.uniform(0, 4.0, (n, 3))
    if kind == "hookean":
        k = rng.uniform(0.5, 5.0, m) if per_spring else 3.0
        r = rng.uniform(0.0, 1.5, m) if per_spring else 1.0
    else:  # r_max above every spring's length
        L = np.linalg.norm(c[pairs[:, 1]] - c[pairs[:, 0]], axis=1)
        k = rng.uniform(0.5, 5.0, m) if per_spring else 3.0
        r = L * rng.uniform(1.05, 2.0, m) if per_spring else 1.01 * float(L.max())
    s = ops.Springs(n, pairs, kind, k, r)
    f, over, mx = s.force(dev(c))
    want, wover, wmx = cm.spring_force(n, pairs, kind, k, r, c)
    assert_bits_equal(host(f), want, "%s %s %s" % (kind, per_spring, graph))
    assert int(over.item()) == wover == 0 and float(mx.item()) == wmx
    if graph == "random8":
        iso = np.setdiff1d(np.arange(n), pairs.reshape(-1))
        assert iso.size and (host(f)[iso].view(np.uint64) == 0).all()  # exactly +0.0
    if graph == "matching":
        fh = host(f)
        assert (fh[pairs[:, 1]] == -fh[pairs[:, 0]]).all()


def test_fene_overstretched_counted_and_stepper_raises():
    from mundy_amd import ops, pipeline
    c = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.6, 0, 0], [10.0, 0, 0]])
    pairs = np.array([[0, 1], [1, 2], [2, 3]])
    s = ops.Springs(4, pairs, "fene", 3.0, 1.5)
    f, over, mx = s.force(dev(c))
    assert int(over.item()) == 2 and float(mx.item()) == 7.4
    fh = host(f)
    assert np.isfinite(fh[0]).all() and np.isnan(fh[1:]).all()
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.full(4, 0.3)), springs=(pairs, "fene", 3.0, 1.5))
    with pytest.raises(RuntimeError, match="FENE"):
        st.step()


# ---- the statistic epilogue the force kernels share: the maximum is found wherever it sits ------------------------------
@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_spring_max_length_is_found_wherever_it_sits(pos):
    from mundy_amd import ops
    n = PAST_FULL_GRID
    c, pairs = line_with_one_long_bond(pos)
    s = ops.Springs(n, pairs, "hookean", 3.0, 0.75)
    f, over, mx = s.force(dev(c))
    want, wover, wmx = cm.spring_force(n, pairs, "hookean", 3.0, 0.75, c)
    assert wmx == 1.5 and float(mx.item()) == wmx and int(over.item()) == wover == 0
    assert_bits_equal(host(f), want, "line, long bond at %d" % pos)
    s.close()


def _contacts_with_one_deep_overlap(pos, bodies):
    """PAST_FULL_GRID contacts dealt round robin to `bodies` disjoint body pairs (2 k, 2 k + 1): overlap 0.25, every
    third one apart, contact pos overlapping by 0.5"""
    c = PAST_FULL_GRID
    k = np.arange(c) % bodies
    pairs = np.stack([2 * k, 2 * k + 1], axis=1).astype(np.int32)
    sep = np.full(c, -0.25)
    sep[1::3] = 0.125
    sep[pos] = -0.5
    return pairs, sep


@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_hertz_max_overlap_is_found_wherever_it_sits(pos):
    from mundy_amd import ops
    pairs, sep = _contacts_with_one_deep_overlap(pos, 1024)
    radius = np.full(2048, 0.5)
    _, mx = ops.hertz_contact_force(dev(pairs), dev(sep), dev(radius))
    _, wmx = hm.hertz_force(pairs, sep, radius)
    assert wmx == 0.5 and float(mx.item()) == wmx


@pytest.mark.parametrize("pos", STAT_POSITIONS)
def test_friction_hertz_statistics_are_found_wherever_they_sit(pos):
    """every odd body pair slides sideways at speed 1 with mu = 1e-4: F_t = h k_t dt = 0.23 against mu F_n = 0.005, capped
    by a wide margin; the even pairs are at rest, F_t = 0: not capped whatever the rounding"""
    from mundy_amd import ops
    nb = 1024
    pairs, sep = _contacts_with_one_deep_overlap(pos, nb)
    c = pairs.shape[0]
    seg = np.tile([-1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], (2 * nb, 1))
    radius = np.full(2 * nb, 0.5)
    vel = np.zeros((2 * nb, 6))
    vel[3::4, 0] = 1.0
    normal, arc, td0 = np.tile([0.0, 0.0, 1.0], (c, 1)), np.full(c, 0.5), np.zeros((c, 3))
    mu, dt = 1e-4, 1e-3
    td = dev(td0)
    f, stats = ops.hertz_friction_force(dev(pairs), dev(sep), dev(normal), dev(arc), dev(arc), dev(seg), dev(radius),
                                        dev(vel), td, mu, dt)
    wf, wtd, wmx, wcapped = fm.friction_force(pairs, sep, normal, arc, arc, seg, radius, 1000.0, 0.3, vel, mu, 0.0, 0.0,
                                              1.0, dt, td0)
    h = stats.cpu()
    assert wmx == 0.5 and float(h[0]) == wmx
    assert int(h.view(torch.int64)[1]) == wcapped == int(((pairs[:, 0] % 4 == 2) & (sep < 0)).sum())
    assert_bits_equal(host(f), wf, "force")
    assert_bits_equal(host(td), wtd, "history")


# ---- the incidence build the handles share: empty and degenerate lists ---------------------------------------------
@pytest.mark.parametrize("case", ["no springs", "one body", "star"])
def test_spring_incidence_empty_and_star(case):
    from mundy_amd import ops
    rng = np.random.default_rng(31)
    n, pairs = {"no springs": (5, np.zeros((0, 2), np.int32)), "one body": (1, np.zeros((0, 2), np.int32)),
                "star": star_graph()}[case]
    c = rng.normal(size=(n, 3))
    s = ops.Springs(n, pairs, "hookean", 3.0, 0.5)
    f, over, mx = s.force(dev(c))
    want, wover, wmx = cm.spring_force(n, pairs, "hookean", 3.0, 0.5, c)
    assert_bits_equal(host(f), want, case)
    assert int(over.item()) == wover == 0
    assert np.float64(mx.item()).view(np.uint64) == np.float64(wmx).view(np.uint64)
    if case == "star":
        assert np.bincount(pairs.ravel())[0] == 100 and all_pos_zero(host(f)[101:]) and wmx > 0
    else:
        assert all_pos_zero(host(f)) and all_pos_zero(host(mx))
    s.close()


# ---- generator -------------------------------------------------------------------------------------------------------
def test_philox_known_answers_on_the_device():
    from mundy_amd import ops
    for ctr, key, want in cm.KAT:
        if ctr[3] != 0:
            continue  # the library's counter word 3 is always 0
        k = _u64_as_i64([key[0] | (key[1] << 32)])
        c = _u64_as_i64([ctr[0] | (ctr[1] << 32)])
        out = host(ops.philox4x32_10(k, c, block=ctr[2])).view(np.uint32)
        assert out[0].tolist() == list(want)


@pytest.mark.parametrize("block", [0, 1, 0xFFFFFFFF])
def test_philox_bit_for_bit_with_high_bits(block):
    from mundy_amd import ops
    rng = np.random.default_rng(block & 0xFFFF)
    n = 100003
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64) | (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    ctrs = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    keys[:4] = [0, 2 ** 64 - 1, 2 ** 32, 2 ** 32 - 1]
    ctrs[:4] = [2 ** 64 - 1, 0, 2 ** 32 - 1, 2 ** 32]
    out = host(ops.philox4x32_10(_u64_as_i64(keys), _u64_as_i64(ctrs), block=block)).view(np.uint32)
    assert (out == cm.philox(keys, ctrs, block)).all()


def test_brownian_increments_match_model_and_counters_advance():
    from mundy_amd import ops
    rng = np.random.default_rng(11)
    n = 200001
    keys = rng.integers(0, 2 ** 63, n, dtype=np.uint64)
    ctrs = rng.integers(0, 2 ** 62, n, dtype=np.uint64)
    mt = rng.uniform(0.05, 0.5, n)
    v0 = rng.normal(size=(n, 6))
    kd, cd, vd = _u64_as_i64(keys), _u64_as_i64(ctrs), dev(v0)
    ops.brownian_velocity(kd, cd, 0.1, 1e-3, dev(mt), vd)
    want, wc = cm.brownian_velocity(keys, ctrs, 0.1, 1e-3, mt, v0)
    got = host(vd)
    assert np.abs(got - want).max() <= 1e-13
    assert (got[:, 3:] == v0[:, 3:]).all()
    assert (host(cd).view(np.uint64) == wc).all()


def test_drag_velocity_bit_for_bit():
    from mundy_amd import ops
    rng = np.random.default_rng(5)
    n = 5001
    mt, F = rng.uniform(0.1, 1.0, n), rng.normal(size=(n, 3))
    assert_bits_equal(host(ops.drag_velocity(dev(mt), dev(F))), cm.drag_velocity(mt, F))
    assert (host(ops.drag_velocity(dev(mt))).view(np.uint64) == 0).all()


# ---- the transpose sweep ---------------------------------------------------------------------------------------------
def _operator(kind, rod_kinematics=True, n=3000, seed=2):
    from gpu_util import random_rods
    from mundy_amd import pipeline
    rng = np.random.default_rng(seed)
    if kind == "sphere":
        c = rng.uniform(0, 14.0, (n, 3))
        st = pipeline.ContactStepper("sphere", dev(c), dev(rng.uniform(0.4, 0.8, n)))
    else:
        c, q, r, ln = random_rods(rng, n, 20.0)
        st = pipeline.ContactStepper("spherocylinder", dev(c), dev(r), dev(q), dev(ln), rod_kinematics=rod_kinematics)
    st.step(integrate=False)
    assert st.op.num_constraints > 1000
    return st


@pytest.mark.parametrize("kind,rodk", [("sphere", True), ("spherocylinder", False), ("spherocylinder", True)])
def test_constraint_rate_is_the_adjoint_of_the_body_sweep(kind, rodk):
    from mundy_amd import ops
    st = _operator(kind, rodk)
    op = st.op
    rng = np.random.default_rng(7)
    x = dev(rng.normal(size=op.num_constraints))
    # dt * D^T (M D x) == apply(x), bit for bit
    vel = op.body_velocity_of(x)
    rate = op.constraint_rate(vel)
    assert_bits_equal(host(st.dt * rate), host(op.apply(x)), "dt D^T M D x")
    # <x, D^T U> = <D x, U>: D x is the body sweep with unit mobilities
    c = st.contacts
    kw = dict(ra=c.get("ra"), rb=c.get("rb"))
    n = st.center.shape[0]
    ones = torch.ones(n, dtype=torch.float64, device="cuda")
    if kind == "sphere":
        unit = ops.ContactOperator(st.contact_pairs, c["normal"], ones, st.dt, priority=c["sep"])
    elif rodk:
        unit = ops.ContactOperator(st.contact_pairs, c["normal"], ones, st.dt, mob_rot=ones,
                                   rod=(c["s"], c["t"], st.seg), priority=c["sep"])
    else:
        unit = ops.ContactOperator(st.contact_pairs, c["normal"], ones, st.dt, mob_rot=ones, priority=c["sep"], **kw)
    U = dev(rng.normal(size=(n, 6)))
    if kind == "sphere":
        U[:, 3:] = 0.0
    Dx = host(unit.body_velocity_of(x))
    lhs = math.fsum(host(x) * host(unit.constraint_rate(U)))
    rhs = math.fsum((Dx * host(U)).reshape(-1))
    scale = math.fsum(np.abs(host(x)) * np.abs(host(unit.constraint_rate(U.abs()))))
    assert abs(lhs - rhs) <= 1e-12 * scale
    unit.close()


def test_constraint_rate_by_hand_for_spheres():
    st = _operator("sphere")
    rng = np.random.default_rng(9)
    U = rng.normal(size=(st.center.shape[0], 6))
    got = host(st.op.constraint_rate(dev(U)))
    p, nrm = host(st.contact_pairs).astype(int), host(st.contacts["normal"])
    d = U[p[:, 1], :3] - U[p[:, 0], :3]
    assert np.allclose(got, (nrm * d).sum(axis=1), rtol=0, atol=1e-13)


# ---- the stepper -----------------------------------------------------------------------------------------------------
def _lattice(side, spacing):
    g = np.arange(side, dtype=np.float64) * spacing
    return np.ascontiguousarray(np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3))


def _free(n_side=100, kt=0.1, **kw):
    from mundy_amd import pipeline
    c = _lattice(n_side, 4.0)  # boxes of half-width r + buffer = 1.5 never touch: no contacts
    n = c.shape[0]
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(n, 0.5)), dt=1e-3, viscosity=1.0, search_buffer=1.0,
                                   brownian_kt=kt, **kw)


def test_free_brownian_step_statistics_1e6():
    st = _free(100)
    n = st.center.shape[0]
    D = 0.1 * float(st.mob_trans[0])
    var = 2.0 * D * 1e-3
    x0 = host(st.center).copy()
    st.step()
    x1 = host(st.center).copy()
    st.step()
    d1, d2 = x1 - x0, host(st.center) - x1
    assert st.contact_pairs.shape[0] == 0
    for d in (d1, d2):
        assert np.all(np.abs(d.mean(axis=0)) < 5.0 * math.sqrt(var / n))
        assert np.all(np.abs(d.var(axis=0) - var) < 5.0 * var * math.sqrt(2.0 / n))
    corr = lambda a, b: float(np.mean((a - a.mean()) * (b - b.mean())) / (a.std() * b.std()))  # noqa: E731
    for a, b in ((d1[:, 0], d1[:, 1]), (d1[:, 1], d1[:, 2]), (d1[:, 0], d1[:, 2]), (d1[:, 0], d2[:, 0]),
                 (d1[:, 1], d2[:, 1]), (d1[:, 2], d2[:, 2])):
        assert abs(corr(a, b)) < 5.0 / math.sqrt(n)
    assert (host(st.rng_counter) == 2).all()


def test_free_brownian_msd_over_100_steps():
    st = _free(40)
    n = st.center.shape[0]
    D = 0.1 * float(st.mob_trans[0])
    x0 = host(st.center).copy()
    for _ in range(100):
        st.step()
    msd = ((host(st.center) - x0) ** 2).sum(axis=1)
    t = 100 * 1e-3
    want = 6.0 * D * t
    # |dx|^2 = (2 D t) chi^2_3: variance 6 (2 D t)^2
    assert abs(msd.mean() - want) < 5.0 * math.sqrt(6.0) * 2.0 * D * t / math.sqrt(n)


def test_free_step_invariant_under_reorder_and_restore():
    rng = np.random.default_rng(4)
    st = _free(20, rng_keys=torch.from_numpy(rng.permutation(8000).astype(np.int64)),
               rng_counter=torch.from_numpy(rng.integers(0, 2 ** 40, 8000)))
    snap = st.snapshot()
    st.step()
    ref = dict(zip(host(st.rng_keys).tolist(), host(st.center)))
    ref_c = host(st.rng_counter).copy()
    st.restore(snap)
    st.step()
    assert_bits_equal(host(st.center), np.array([ref[k] for k in host(st.rng_keys).tolist()]), "after restore")
    assert (host(st.rng_counter) == ref_c).all()
    st.restore(snap)
    st.reorder_bodies(curve="morton", cell_size=5.0)
    st.step()
    got = np.array([ref[k] for k in host(st.rng_keys).tolist()])
    assert_bits_equal(host(st.center), got, "after reorder_bodies")


def _packed(seed=1, n=4000, box=18.0, r=0.5):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, box, (n, 3)), np.full(n, r)


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_defaults_unchanged_and_zero_noise_is_the_plain_step(model):
    from mundy_amd import pipeline
    c, r = _packed()
    kw = dict(contact_model=model, dt=1e-3, viscosity=1.0)
    a = pipeline.ContactStepper("sphere", dev(c), dev(r), **kw)
    b = pipeline.ContactStepper("sphere", dev(c), dev(r), springs=None, brownian_kt=None, rng_keys=None,
                                rng_counter=None, **kw)
    z = pipeline.ContactStepper("sphere", dev(c), dev(r), brownian_kt=0.0, **kw)
    for _ in range(3):
        sa, sb, sz = a.step(), b.step(), z.step()
        assert sa.num_contacts > 0 and sa.num_contacts == sb.num_contacts == sz.num_contacts
        assert_bits_equal(host(a.center), host(b.center), "explicit defaults")
        assert_bits_equal(host(a.center), host(z.center), "kT = 0, no springs")
        assert sa.num_iters == sz.num_iters and sa.max_overlap == sz.max_overlap
    assert not a.chain and a.springs is None and a.rng_keys is None


def test_two_bead_hookean_closure():
    from mundy_amd import pipeline
    k, r0, dt = 3.0, 1.0, 1e-3
    c = np.array([[0.0, 0.0, 0.0], [1.9, 0.0, 0.0]])
    st = pipeline.ContactStepper("sphere", dev(c), dev(np.array([0.5, 0.3])), dt=dt, viscosity=1.0,
                                 springs=([[0, 1]], "hookean", k, r0))
    m = host(st.mob_trans)
    fac = 1.0 - k * (m[0] + m[1]) * dt
    ext = 1.9 - r0
    for _ in range(20):
        s = st.step()
        ext *= fac
        x = host(st.center)
        assert (x[1, 0] - x[0, 0] - r0) == pytest.approx(ext, rel=1e-12)
        assert (x[:, 1:] == 0).all()
    assert s.max_spring_length == pytest.approx(r0 + ext / fac, rel=1e-12)


def _compressing_chain(model, n_beads=400, spacing=1.0):
    from mundy_amd import pipeline, ops
    # beads touching along a line, springs with rest length 0.5 pull them into each other: only U_ext drives contact
    c = np.zeros((n_beads, 3))
    c[:, 0] = np.arange(n_beads) * spacing
    c[:, 1] = 0.01 * np.sin(np.arange(n_beads))
    pairs = np.stack([np.arange(n_beads - 1), np.arange(1, n_beads)], axis=1)
    return pipeline.ContactStepper("sphere", dev(c), dev(np.full(n_beads, 0.5)), dt=1e-3, viscosity=1.0,
                                   search_buffer=1.0, contact_model=model,
                                   cfg=ops.PGDConfig(max_iters=100000, tol=1e-12),
                                   springs=(pairs, "hookean", 30.0, 0.5), brownian_kt=0.1)


def test_compressed_chain_lcp_sees_the_external_velocity():
    from mundy_amd import ops
    st = _compressing_chain("lcp")
    st.step()
    lam = host(st.lam)
    sep = host(st.contacts["sep"])
    g = sep + st.dt * host(st.op.constraint_rate(st.velocity))
    assert (lam >= 0).all() and lam.max() > 0
    assert g.min() >= -1e-8
    assert np.abs(lam * g).max() <= 1e-8 * max(1.0, lam.max())
    # a solve that ignores U_ext: q = sep, then U = U_ext + M D lambda -> the contacts overlap by dt |D^T U_ext|
    lam0, _, _ = ops.solve_lcp(st.op, st.contacts["sep"], torch.zeros_like(st.lam), st.cfg)
    u0 = st.op.body_velocity_of(lam0)
    u0 += st.u_ext
    g0 = sep + st.dt * host(st.op.constraint_rate(u0))
    assert g0.min() < -1e-5


def test_hertz_chain_velocity_is_external_plus_contact():
    st = _compressing_chain("hertz", spacing=0.97)
    x0 = host(st.center).copy()
    keys, ctr0 = host(st.rng_keys).copy(), host(st.rng_counter).copy()
    st.step()
    n = x0.shape[0]
    p = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1)
    F, _, _ = cm.spring_force(n, p, "hookean", 30.0, 0.5, x0)
    mt = host(st.mob_trans)
    uext, _ = cm.brownian_velocity(keys.view(np.uint64), ctr0.view(np.uint64), 0.1, st.dt, mt, cm.drag_velocity(mt, F))
    assert np.abs(host(st.u_ext) - uext).max() <= 1e-13
    ucon = host(st.op.body_velocity_of(st.lam))
    assert np.abs(host(st.velocity) - (uext + ucon)).max() <= 1e-12
    assert_bits_equal(host(st.center), x0 + st.dt * host(st.velocity)[:, :3], "Euler")


def test_chain_step_app_matches_python():
    from cpp_apps import build_app, fnv1a
    from mundy_amd import pipeline, synth
    d = synth.chains(2, 1000, seed=8)
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"])
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d max_spring_length %.17g" % (k, s.num_contacts, s.num_iters,
                                                                                     s.max_spring_length))
    import tempfile
    exe = build_app("chain_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
        out = subprocess.run([exe, path, "20", repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]),
                              repr(d["kt"])], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:8]) for g in got] == lines
    cs = [ln for ln in out.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert cs[2] == fnv1a(host(st.center).reshape(-1).view(np.uint64).tolist())


def test_one_step_at_full_size():
    from mundy_amd import pipeline, synth
    d = synth.chains(1000, 1000, seed=3)
    n = d["center"].shape[0]
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"])
    s = st.step()
    assert s.num_bodies == n == 10 ** 6 and s.num_contacts > 0 and s.converged
    F, _, mx = cm.spring_force(n, d["pairs"], "hookean", d["k"], d["r0"], d["center"])
    assert_bits_equal(host(st.spring_force), F, "spring force")
    assert s.max_spring_length == mx
    rng = np.random.default_rng(0)
    sample = rng.choice(n, 20000, replace=False)
    mt = host(st.mob_trans)[sample]
    uext, _ = cm.brownian_velocity(sample.astype(np.uint64), np.zeros(sample.size, np.uint64), d["kt"], d["dt"], mt,
                                   cm.drag_velocity(mt, F[sample]))
    assert np.abs(host(st.u_ext)[sample] - uext).max() <= 1e-13
    lam = host(st.lam)
    g = host(st.contacts["sep"]) + st.dt * host(st.op.constraint_rate(st.velocity))
    assert (lam >= 0).all() and g.min() >= -10 * st.cfg.tol
    assert (host(st.rng_counter) == 1).all()
