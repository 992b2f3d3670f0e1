"""The periphery's no-slip correction on the GPU (include/mundy_hip_hydro_periphery.h), device against the numpy model
of tests/hydro_periphery_model.py, bit for bit unless said otherwise: the matrix fill, the Gauss-Jordan inverse, the
matrix-vector product, the double-layer sum on the machinery of mhip_hydro_velocity, the composite call, the stepper's
hydrodynamics=dict(periphery=...) stage, the C++ driver and one call at the app's size (order 32, 2 178 nodes)."""
import ctypes as C_
import os
import subprocess

import numpy as np
import pytest
import torch

import hydro_model as hm
import hydro_periphery_model as pm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

C = hm.CHUNK
MU = 0.7
R = 5.0
SIZES = (1, 2, 63, 64, 65, 257, C - 1, C, C + 1, 2 * C + 77)
BIG = 3 * C + 5


def _surface(order, mu=MU):
    from mundy_amd import ops
    p, w, n = pm.sphere_quadrature(order, R, include_poles=False, invert=True)
    return dict(p=p, w=w, n=n, h=ops.HydroPeriphery(dev(p), dev(w), dev(n), mu))


def _seeded_matrix(N, seed=0):
    A = np.random.default_rng(1000 + N + seed).normal(size=(N, N))
    np.fill_diagonal(A, 0.0)  # no elimination step finds its pivot on the diagonal by default
    return A


# ---- 1. the fill ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [2, 4, 7, 11])
def test_fill_bit_for_bit(order):
    s = _surface(order)
    assert s["p"].shape[0] == {2: 18, 4: 50, 7: 128, 11: 288}[order]  # across the 256-wide tile
    assert s["h"].state == "empty"
    T, M = pm.fill_matrix(s["p"], s["w"], s["n"], MU)
    s["h"].fill_double_layer()
    assert s["h"].state == "double_layer"
    assert_bits_equal(host(s["h"].matrix()), T, "T, order %d" % order)
    s["h"].fill_matrix()
    assert s["h"].state == "matrix"
    assert_bits_equal(host(s["h"].matrix()), M, "M, order %d" % order)
    s["h"].fill_matrix()
    assert_bits_equal(host(s["h"].matrix()), M, "M again")
    s["h"].close()


# ---- 2. the inverse ---------------------------------------------------------------------------------------------------------
def _handle(N):
    from mundy_amd import ops
    assert N % 3 == 0
    z = torch.zeros((N // 3, 3), dtype=torch.float64, device="cuda")
    return ops.HydroPeriphery(z, z[:, 0].contiguous(), z, 1.0)


@pytest.mark.parametrize("N", [3, 63, 66, 129, 258, 384])
def test_invert_seeded_matrices_bit_for_bit(N):
    A = _seeded_matrix(N)
    want, min_pivot, swaps = pm.gauss_jordan(A)
    assert swaps >= 1
    h = _handle(N)
    got_pivot = h.set_matrix(dev(A)).invert()
    assert h.state == "inverse"
    first = host(h.matrix())
    assert_bits_equal(first, want, "inverse, N = %d" % N)
    assert got_pivot == min_pivot
    assert h.set_matrix(dev(A)).invert() == min_pivot
    assert_bits_equal(host(h.matrix()), first, "twice")
    assert np.abs(A @ first - np.eye(N)).max() < 1e-9
    h.close()


def test_invert_refuses_a_singular_matrix_and_the_state_refusals():
    from mundy_amd import ops
    h = _handle(66)
    u = torch.zeros(66, dtype=torch.float64, device="cuda")
    with pytest.raises(AssertionError, match="invert needs a matrix"):
        h.invert()
    with pytest.raises(AssertionError, match="needs the inverse"):
        h.surface_forces(u)
    z3 = torch.zeros((4, 3), dtype=torch.float64, device="cuda")
    with pytest.raises(AssertionError, match="needs the inverse"):
        h.correct("rpyc", z3, z3[:, 0].contiguous(), z3, z3.clone())
    A = _seeded_matrix(66)
    A[:, 40] = 0.0  # exactly singular, and exactly so in floating point: the column stays +-0.0 until its own step
    with pytest.raises(pm.SingularMatrix):
        pm.gauss_jordan(A)
    with pytest.raises(RuntimeError, match="singular"):
        h.set_matrix(dev(A)).invert()
    assert h.state == "empty"
    with pytest.raises(AssertionError, match="needs the inverse"):
        h.surface_forces(u)
    A[40, 3] = np.nan
    with pytest.raises(RuntimeError, match="singular"):
        h.set_matrix(dev(A)).invert()
    with pytest.raises(AssertionError, match="invert needs a matrix"):  # an inverse is not inverted again
        h.set_inverse(dev(_seeded_matrix(66))).invert()
    with pytest.raises(ValueError, match="kind"):
        from mundy_amd import capi
        P = C_.c_void_p(64)
        ws = ops.HydroWorkspace()
        capi.check(capi.load().mhip_hydro_periphery_correct(h._h, ws._h, 3, 3, P, P, P, P, 3, 1, None))
    ws.close()
    h.close()


@pytest.mark.parametrize("order", [2, 4, 7])
def test_invert_the_filled_matrix(order):
    s = _surface(order)
    _, M = pm.fill_matrix(s["p"], s["w"], s["n"], MU)
    want, min_pivot, _ = pm.gauss_jordan(M)
    assert s["h"].fill_matrix().invert() == min_pivot
    assert_bits_equal(host(s["h"].matrix()), want, "Minv, order %d" % order)
    s["h"].close()


# ---- 3. the matrix-vector product ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 189, 192, 195, 771, 3072, 3075, 3 * 1058])
def test_surface_forces_bit_for_bit(N):
    rng = np.random.default_rng(N)
    Minv, u = rng.normal(size=(N, N)), rng.normal(size=N)
    h = _handle(N)
    h.set_inverse(dev(Minv))
    got = host(h.surface_forces(dev(u)))
    assert_bits_equal(got, pm.surface_forces(Minv, u), "f_surf, N = %d" % N)
    assert_bits_equal(host(h.surface_forces(dev(u))), got, "twice")
    # one row alone (by hand: 64 strided partial sums, the halving tree) has the bits it has in the full product
    r = N // 2
    lanes = [np.float64(0.0)] * 64
    for j in range(N):
        lanes[j % 64] = lanes[j % 64] + Minv[r, j] * u[j]
    k = 32
    while k:
        lanes = [lanes[i] + lanes[i + k] for i in range(k)]
        k //= 2
    assert got[r] == -lanes[0]
    assert_bits_equal(pm.surface_forces(Minv, u, rows=[r]), got[r:r + 1], "row %d alone" % r)
    h.close()


# ---- 4. the double layer ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cloud():
    """BIG surface nodes (points on a sphere, unit normals, positive weights, a density) and BIG targets inside, a few
    targets exactly on nodes (the rinv = 0 branch)"""
    rng = np.random.default_rng(12)
    v = rng.normal(size=(BIG, 3))
    n = -v / np.linalg.norm(v, axis=1, keepdims=True)
    d = dict(c=-R * n, n=n, w=rng.uniform(0.01, 0.05, BIG), f=rng.normal(size=(BIG, 3)))
    t = rng.normal(size=(BIG, 3))
    d["t"] = t / np.linalg.norm(t, axis=1, keepdims=True) * rng.uniform(0.0, 0.95 * R, (BIG, 1))
    dup = np.arange(0, BIG, 97)
    d["t"][dup] = d["c"][(dup * 3 + 1) % BIG]  # on another node ...
    d["t"][5] = d["c"][5]                      # ... and on the node of the same index
    d["dev"] = {k: dev(v) for k, v in d.items()}
    return d


def _gpu_dl(d, ns, nt, **kw):
    from mundy_amd import ops
    g = d["dev"]
    return ops.hydro_double_layer(MU, g["c"][:ns], g["n"][:ns], g["w"][:ns], g["f"][:ns], g["t"][:nt], **kw)


def _model_dl(d, ns, nt, **kw):
    return pm.double_layer(MU, d["c"][:ns], d["n"][:ns], d["w"][:ns], d["f"][:ns], d["t"][:nt], **kw)


def _size_pairs():
    """the (ns, nt) set of tests/test_gpu_hydro.py: every ns of SIZES with two nt each, 24 of the 100, + the extremes"""
    k = len(SIZES)
    out = []
    for i, ns in enumerate(SIZES):
        out += [(ns, SIZES[(3 * i + 1) % k]), (ns, SIZES[(7 * i + 4) % k])]
    out += [(1, 1), (2 * C + 77, C + 1), (BIG, 1), (1, BIG)]
    return sorted(set(out))


@pytest.mark.parametrize("ns,nt", _size_pairs())
def test_double_layer_sums_bit_for_bit(cloud, ns, nt):
    from mundy_amd import ops
    rng = np.random.default_rng(ns * 7919 + nt)
    old = rng.normal(size=(nt, 6))
    ws = ops.HydroWorkspace()
    for skip in (True, False):
        want = _model_dl(cloud, ns, nt, skip_same_index=skip)
        assert np.isfinite(want).all()
        assert_bits_equal(host(_gpu_dl(cloud, ns, nt, skip_same_index=skip)), want, "(%d, %d) skip %s" % (ns, nt, skip))
        buf = dev(old)
        _gpu_dl(cloud, ns, nt, out=buf, accumulate=True, skip_same_index=skip, workspace=ws)
        assert_bits_equal(host(buf)[:, :3], old[:, :3] + want, "(%d, %d), stride 6 accumulate" % (ns, nt))
        assert_bits_equal(host(buf)[:, 3:], old[:, 3:], "untouched columns")
        for path in ("in_lane", "partial"):
            ws.set_path(path)
            buf3 = dev(old[:, :3].copy())
            _gpu_dl(cloud, ns, nt, out=buf3, accumulate=True, skip_same_index=skip, workspace=ws)
            assert ws.last_path() == path
            assert_bits_equal(host(buf3), old[:, :3] + want, "(%d, %d), %s" % (ns, nt, path))
            buf6 = dev(old)
            _gpu_dl(cloud, ns, nt, out=buf6, skip_same_index=skip, workspace=ws)
            assert_bits_equal(host(buf6)[:, :3], want, "(%d, %d), %s, stride 6 store" % (ns, nt, path))
        ws.set_path("auto")
    ws.close()


def test_double_layer_skip_and_coincident_targets(cloud):
    ns, nt = 300, 200
    on, off = host(_gpu_dl(cloud, ns, nt, skip_same_index=True)), host(_gpu_dl(cloud, ns, nt, skip_same_index=False))
    terms = pm.dl_terms(MU, cloud["t"][:nt], cloud["c"][:ns], cloud["n"][:ns], cloud["w"][:ns], cloud["f"][:ns])
    same = terms[np.arange(nt), np.arange(nt)]
    differs = (on.view(np.uint64) != off.view(np.uint64)).any(axis=1)
    assert differs.sum() >= nt - 2 and not differs[5]  # target 5 lies ON node 5: rinv = 0, the term is +-0.0 anyway
    assert all_pos_zero(np.abs(same[5])) and np.isfinite(terms).all()
    assert np.abs(off - on - same).max() <= 1e-12 * np.abs(terms).max()
    # ns != nt on both sides: the index that is skipped is the row index of the arrays
    for a, b in ((64, 300), (300, 64)):
        want = _model_dl(cloud, a, b, skip_same_index=True)
        assert_bits_equal(host(_gpu_dl(cloud, a, b, skip_same_index=True)), want, "skip, (%d, %d)" % (a, b))
        assert (want.view(np.uint64) != _model_dl(cloud, a, b, skip_same_index=False).view(np.uint64)).any()
    # a target evaluated alone: index 0 of its own array, so the skip moves with it -- without the skip, the same bits
    alone = host(_gpu_dl(dict(dev={k: (v[7:8] if k == "t" else v) for k, v in cloud["dev"].items()}), ns, 1,
                         skip_same_index=False))
    assert_bits_equal(alone, off[7:8], "a target alone")
    assert_bits_equal(host(_gpu_dl(cloud, ns, nt, skip_same_index=True)), on, "two calls")


def test_double_layer_empty_sets(cloud):
    from mundy_amd import ops
    g = cloud["dev"]
    z, z1 = torch.empty((0, 3), dtype=torch.float64, device="cuda"), torch.empty((0,), dtype=torch.float64, device="cuda")
    out = dev(np.full((5, 3), 7.0))
    ops.hydro_double_layer(MU, z, z, z1, z, g["t"][:5], out=out)
    assert all_pos_zero(host(out))
    assert ops.hydro_double_layer(MU, g["c"][:9], g["n"][:9], g["w"][:9], g["f"][:9], z).shape == (0, 3)


# ---- 5. the composite call ----------------------------------------------------------------------------------------------------
def _beads(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    x = v / np.linalg.norm(v, axis=1, keepdims=True) * (0.8 * R * rng.uniform(0, 1, n) ** (1 / 3))[:, None]
    return x, rng.uniform(0.05, 0.3, n), rng.normal(size=(n, 3))


@pytest.mark.parametrize("kind,skip", [("rpyc", True), ("rpyc", False), ("rpy", True), ("stokes", True)])
def test_correct_is_the_three_calls_and_the_model(kind, skip):
    from mundy_amd import ops
    s = _surface(4)
    hp = s["h"]
    hp.fill_matrix().invert()
    Minv = host(hp.matrix())
    x, a, F = _beads(333, 3)
    old = np.random.default_rng(4).normal(size=(333, 6))
    got = dev(old)
    ws = ops.HydroWorkspace()
    hp.correct(kind, dev(x), dev(a), dev(F), got, skip_same_index=skip, workspace=ws)
    # by hand
    S = s["p"].shape[0]
    u_surf = ops.hydro_velocity(kind, MU, dev(x), dev(a), dev(F), dev(s["p"]), torch.zeros(S, dtype=torch.float64,
                                                                                          device="cuda"))
    f_surf = hp.surface_forces(u_surf)
    hand = dev(old)
    ops.hydro_double_layer(MU, dev(s["p"]), dev(s["n"]), dev(s["w"]), f_surf, dev(x), out=hand, accumulate=True,
                           skip_same_index=skip)
    assert_bits_equal(host(got), host(hand), "the three calls by hand")
    want, mu_surf, mf_surf = pm.correct(kind, MU, s["p"], s["w"], s["n"], Minv, x, a, F, old=old[:, :3],
                                        skip_same_index=skip)
    assert_bits_equal(host(u_surf), mu_surf, "u_surf")
    assert_bits_equal(host(f_surf), mf_surf, "f_surf")
    assert_bits_equal(host(got)[:, :3], want, "the model")
    assert_bits_equal(host(got)[:, 3:], old[:, 3:], "untouched columns")
    ws.close()
    hp.close()


def test_device_inherits_the_closed_form_bound_at_order_8():
    """the device's correction of a centred Stokeslet IS the model's (bit for bit), so it is within the bound
    tests/test_hydro_periphery_host.py measures for the model: 1.5 x 0.0340 at order 8"""
    from mundy_amd import ops
    s = _surface(8, mu=1.0)
    s["h"].fill_matrix().invert()
    rng = np.random.default_rng(0)
    F = np.array([[0.3, -1.1, 0.5]])
    v = rng.normal(size=(40, 3))
    v /= np.sqrt((v * v).sum(axis=1))[:, None]
    x = v * (0.6 * R * rng.uniform(0.0, 1.0, 40) ** (1.0 / 3.0))[:, None]
    S = s["p"].shape[0]
    u_surf = ops.hydro_velocity("rpyc", 1.0, dev(np.zeros((1, 3))), dev(np.zeros(1)), dev(F), dev(s["p"]),
                                torch.zeros(S, dtype=torch.float64, device="cuda"))
    f_surf = s["h"].surface_forces(u_surf)
    got = host(ops.hydro_double_layer(1.0, dev(s["p"]), dev(s["n"]), dev(s["w"]), f_surf, dev(x), skip_same_index=True))
    _, M = pm.fill_matrix(s["p"], s["w"], s["n"], 1.0)
    mu_surf = pm.surface_velocity("rpyc", 1.0, np.zeros((1, 3)), np.zeros(1), F, s["p"])
    mf = pm.surface_forces(pm.gauss_jordan(M)[0], mu_surf).reshape(-1, 3)
    assert_bits_equal(got, pm.double_layer(1.0, s["p"], s["n"], s["w"], mf, x, skip_same_index=True), "the model")
    want = pm.stokeslet_in_sphere_correction(x, F[0], R, 1.0)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("device, order 8: relative error of the correction %.5f" % err)
    assert err <= 1.5 * 0.0340
    assert err == pm.centred_stokeslet_error(8, R=R, skip_same_index=True)
    s["h"].close()


# ---- 6. the stepper -----------------------------------------------------------------------------------------------------------
ORDER = 4


def _chains(seed=8, jitter=0.05):
    from mundy_amd import synth
    d = synth.chains(4, 50, seed=seed, cell=2.4)
    d["center"] = d["center"] - np.array([2.4, 2.4, 1.2])  # inside the sphere of radius 5
    d["center"] = d["center"] + jitter * np.random.default_rng(seed).normal(size=d["center"].shape)
    assert np.linalg.norm(d["center"], axis=1).max() < R - 0.5
    return d


def _pe(**kw):
    return dict(shape="sphere", radius=R, spectral_order=ORDER, **kw)


def _stepper(d, hydro=..., **kw):
    from mundy_amd import pipeline
    args = dict(dt=d["dt"], viscosity=d["viscosity"], search_buffer=d["skin"],
                springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"])
    if hydro is not ...:
        args["hydrodynamics"] = hydro
    args.update(kw)
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), **args)


@pytest.fixture(scope="module")
def surface4():
    p, w, n = pm.sphere_quadrature(ORDER, R, invert=True)
    _, M = pm.fill_matrix(p, w, n, 1.0)
    Minv, min_pivot, _ = pm.gauss_jordan(M)
    return dict(p=p, w=w, n=n, Minv=Minv, min_pivot=min_pivot)


@pytest.mark.parametrize("skip", [True, False])
def test_stepper_external_velocity_is_dry_plus_noise_plus_hydro_plus_correction(surface4, skip):
    from mundy_amd import ops
    d = _chains()
    s4 = surface4
    st = _stepper(d, dict(kind="rpyc", periphery=_pe(skip_same_index=skip)))
    assert st.hydro["periphery_min_pivot"] == s4["min_pivot"] and st.hydro_periphery.state == "inverse"
    assert_bits_equal(host(st.hydro_periphery.matrix()), s4["Minv"], "the inverse built at construction")
    keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
    x0 = host(st.center).copy()
    st.compute_aabb()
    st.generate_neighbor_links()
    st.external_velocity()
    F = host(st.spring_force)
    assert np.abs(F).max() > 1e-3
    base = ops.brownian_velocity(keys, ctr, d["kt"], d["dt"], st.mob_trans, ops.drag_velocity(st.mob_trans, dev(F)))
    want_h = hm.velocity("rpyc", d["viscosity"], x0, d["radius"], F)
    want, _, _ = pm.correct("rpyc", d["viscosity"], s4["p"], s4["w"], s4["n"], s4["Minv"], x0, d["radius"], F,
                            old=want_h, skip_same_index=skip)
    assert (want.view(np.uint64) != want_h.view(np.uint64)).any(axis=1).all()
    assert_bits_equal(host(st.u_hydro), want, "u_hydro")
    assert_bits_equal(host(st.u_ext)[:, :3], host(base)[:, :3] + want, "u_ext")
    assert all_pos_zero(host(st.u_ext)[:, 3:])
    assert st.hydro_step == 1


def test_stepper_update_every_and_timings():
    d = _chains()
    st = _stepper(d, dict(kind="rpyc", update_every=3, periphery=_pe()))
    plain = _stepper(d, dict(kind="rpyc", update_every=3))
    seen = []
    for k in range(7):
        before = host(st.u_hydro).copy()
        s = st.step(timed=(k == 0))
        if k == 0:
            assert list(s.timings_ms) == list(plain.step(timed=True).timings_ms)  # part of the hydrodynamics mark
        seen.append(not np.array_equal(before.view(np.uint64), host(st.u_hydro).view(np.uint64)))
        assert st.hydro_step == k + 1
    assert seen == [True, False, False, True, False, False, True]


def test_stepper_without_forces_and_without_the_key():
    d = _chains(jitter=0.0)
    kw = dict(springs=(d["pairs"], "hookean", 0.0, d["r0"]), brownian_kt=0.0)
    a, b = _stepper(d, **kw), _stepper(d, dict(kind="rpyc", periphery=_pe()), **kw)
    for _ in range(3):
        a.step()
        b.step()
        assert_bits_equal(host(b.center), host(a.center), "zero forces")
    assert all_pos_zero(host(b.u_hydro))
    # the key absent (or None): today's trajectory
    d = _chains()
    a, b = _stepper(d, dict(kind="rpyc", update_every=2)), _stepper(d, dict(kind="rpyc", update_every=2, periphery=None))
    c = _stepper(d, dict(kind="rpyc", update_every=2, periphery=_pe()))
    assert a.hydro_periphery is None and b.hydro_periphery is None
    for _ in range(4):
        a.step()
        b.step()
        c.step()
    assert_bits_equal(host(b.center), host(a.center), "periphery=None")
    assert_bits_equal(host(b.u_hydro), host(a.u_hydro), "periphery=None")
    assert (host(c.u_hydro).view(np.uint64) != host(a.u_hydro).view(np.uint64)).any()


def test_stepper_snapshot_restore_across_an_update_boundary():
    d = _chains()
    st = _stepper(d, dict(kind="rpyc", update_every=2, periphery=_pe()))
    st.step()
    snap = st.snapshot()
    for _ in range(3):
        st.step()
    first = (host(st.center).copy(), host(st.u_hydro).copy(), st.hydro_step)
    st.restore(snap)
    assert st.hydro_step == 1
    for _ in range(3):
        st.step()
    assert_bits_equal(host(st.center), first[0], "centres after restore")
    assert_bits_equal(host(st.u_hydro), first[1], "u_hydro after restore")
    assert st.hydro_step == first[2] == 4


def _dl_abs(mu, x, p, n, w, g):
    """sum_s |DL_ts| g_s per component: an upper bound of what a change of at most g [S, 3] in the surface density moves
    in the double layer at x (exact r^-5 with 1 % for the quake estimate of it)"""
    d = np.abs(x[:, None, :] - p[None, :, :])
    r2 = (d * d).sum(axis=2)
    c = 1.01 * 3.0 / (4.0 * np.pi * mu) * r2 ** -2.5
    coeff = c * w[None, :] * (d * np.abs(n)[None]).sum(axis=2) * (d * g[None]).sum(axis=2)
    return (d * coeff[..., None]).sum(axis=1)


def test_stepper_reorder_bodies(surface4):
    """skip_same_index=False: the correction of a bead does not depend on its row; a renumbering changes the order of
    the sums over the BEADS alone (the beads-to-beads sum and u_surf).  Section 5l's bound for such a sum is 2 n eps A, A
    the sum of the magnitudes of its terms; carried through the two linear steps behind u_surf, with their own rounding
    on changed inputs:
        |d u_surf| <= 2 n eps A_surf
        |d f|      <= |Minv| |d u_surf| + 2 (N / 64 + 8) eps |Minv| |u_surf|
        |d u|      <= 2 n eps A + DLabs(|d f|) + 2 (S + 8) eps DLabs(|f|)"""
    d = _chains()
    n = d["center"].shape[0]
    hy = dict(kind="rpyc", periphery=_pe(skip_same_index=False))
    a, b = _stepper(d, hy), _stepper(d, hy)
    a.step()
    b.step()
    perm = host(b.reorder_bodies()).astype(np.int64)
    assert not np.array_equal(perm, np.arange(n))
    assert_bits_equal(host(b.u_hydro), host(a.u_hydro)[perm], "the stored velocity moves with its rows")
    for s in (a, b):
        s.compute_aabb()
        s.generate_neighbor_links()
        s.external_velocity()
    assert_bits_equal(host(b.center), host(a.center)[perm], "centres")
    Fa, xa = host(a.spring_force), host(a.center)
    assert_bits_equal(host(b.spring_force), Fa[perm], "forces")
    s4, mu, eps = surface4, d["viscosity"], 2.0 ** -53
    S = s4["p"].shape[0]
    N = 3 * S
    _, A = hm.velocity("rpyc", mu, xa, d["radius"], Fa, want_abs=True)
    u_surf, A_surf = hm.velocity("rpyc", mu, xa, d["radius"], Fa, s4["p"], np.zeros(S), want_abs=True)
    absM = np.abs(s4["Minv"])
    f = pm.surface_forces(s4["Minv"], u_surf).reshape(S, 3)
    df = (absM @ (2.0 * n * eps * A_surf.reshape(-1)) +
          2.0 * (N / 64 + 8) * eps * (absM @ np.abs(u_surf).reshape(-1))).reshape(S, 3)
    bound = (2.0 * n * eps * A + _dl_abs(mu, xa, s4["p"], s4["n"], s4["w"], df) +
             2.0 * (S + 8) * eps * _dl_abs(mu, xa, s4["p"], s4["n"], s4["w"], np.abs(f)))[perm]
    ua, ub = host(a.u_hydro)[perm], host(b.u_hydro)
    print("reorder: max |du| %.3g, smallest bound %.3g" % (np.abs(ub - ua).max(), bound.min()))
    assert (np.abs(ub - ua) <= bound).all()
    # the stepper evaluates the sums in the constructor's numbering: the bound holds with nothing to spare
    assert np.abs(ub).max() > 0.0
    assert_bits_equal(ub, ua, "u_hydro of every bead, whatever its row")


def test_stepper_reorder_bodies_keeps_the_skipped_pairs():
    """skip_same_index=True (the default) drops the term of surface node i onto bead i of the constructor's numbering,
    before and after reorder_bodies: the corrected u_hydro of every bead keeps its bits"""
    d = _chains()
    n = d["center"].shape[0]
    hy = dict(kind="rpyc", periphery=_pe())
    a, b, c = _stepper(d, hy), _stepper(d, hy), _stepper(d, dict(kind="rpyc", periphery=_pe(skip_same_index=False)))
    assert a.hydro["skip_same_index"] and not c.hydro["skip_same_index"]
    for s in (a, b, c):
        s.step()
    # the skip acts: from the same centres it changes the first S beads and no other
    S = a.hydro_periphery.num_nodes
    differ = (host(a.u_hydro).view(np.uint64) != host(c.u_hydro).view(np.uint64)).any(axis=1)
    assert S < n and differ[:S].any() and not differ[S:].any()
    perm = host(b.reorder_bodies()).astype(np.int64)
    assert (perm[:S] >= S).any() and (perm[S:] < S).any()   # beads cross the boundary between the two kinds of row
    for s in (a, b):
        s.compute_aabb()
        s.generate_neighbor_links()
        s.external_velocity()
    assert_bits_equal(host(b.center), host(a.center)[perm], "centres")
    ua = host(a.u_hydro)
    assert np.abs(ua).max() > 0.0
    assert_bits_equal(host(b.u_hydro), ua[perm], "u_hydro of every bead, whatever its row")


def test_stepper_precomputed_inverse(surface4):
    d = _chains()
    p, w, n = surface4["p"], surface4["w"], surface4["n"]
    a = _stepper(d, dict(kind="rpyc", periphery=_pe()))
    b = _stepper(d, dict(kind="rpyc", periphery=dict(points=p, weights=w, normals=n, inverse=surface4["Minv"])))
    c = _stepper(d, dict(kind="rpyc", periphery=_pe(inverse=a.hydro_periphery.matrix())))
    for _ in range(3):
        for s in (a, b, c):
            s.step()
    assert_bits_equal(host(b.u_hydro), host(a.u_hydro), "inverse= as a host array, the quadrature as arrays")
    assert_bits_equal(host(c.u_hydro), host(a.u_hydro), "inverse= as a device tensor")
    assert_bits_equal(host(b.center), host(a.center), "centres")


# ---- 7. the C++ driver ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [True, False])
def test_hydro_periphery_step_app_matches_python(surface4, skip):
    import tempfile

    from cpp_apps import build_app, fnv1a
    from mundy_amd import capi, synth
    d = _chains()
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    st = _stepper(d, dict(kind="rpyc", update_every=2, periphery=_pe(skip_same_index=skip)))
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d max_spring_length %.17g" % (k, s.num_contacts, s.num_iters,
                                                                                     s.max_spring_length))
    exe = build_app("hydro_periphery_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            np.array([surface4["p"].shape[0], 1 if skip else 0], dtype=np.uint64).tofile(f)
            for k in ("p", "w", "n"):
                surface4[k].astype(np.float64).tofile(f)
        out = subprocess.run([exe, path, "20", repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]),
                              repr(d["kt"]), repr(d["viscosity"]), str(capi.HYDRO_RPYC), "2"], capture_output=True,
                             text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:8]) for g in got] == lines
    assert "min_pivot %.17g" % surface4["min_pivot"] in out.stdout
    cs = [ln for ln in out.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert cs[2] == fnv1a(host(st.center).reshape(-1).view(np.uint64).tolist())


# ---- 8. the app's size ----------------------------------------------------------------------------------------------------------
def test_order_32_and_twenty_thousand_beads():
    """order 32: S = 2 178 nodes, N = 6 534 (a 341 MB matrix), 2 x 10^4 beads.  A 64-bead sample of the composite call
    against the model's sums over the device's f_surf, and max|M Minv - I| on 64 seeded rows against 10 x what
    numpy.linalg.inv leaves on the order-7 matrix (N = 384), scaled by N / 384.  Recorded on an MI355X: see DESIGN.md 5o."""
    from mundy_amd import ops
    s = _surface(32)
    hp = s["h"]
    S = s["p"].shape[0]
    N = 3 * S
    assert S == 2178
    hp.fill_matrix()
    rows = np.sort(np.random.default_rng(6).choice(N, 64, replace=False))
    M_rows = hp.matrix()[torch.from_numpy(rows).cuda()]
    min_pivot = hp.invert()
    Minv = hp.matrix()
    res = float((M_rows @ Minv - torch.eye(N, dtype=torch.float64, device="cuda")[torch.from_numpy(rows).cuda()])
                .abs().max())
    p7, w7, n7 = pm.sphere_quadrature(7, R, invert=True)
    M7 = pm.fill_matrix(p7, w7, n7, MU)[1]
    ref = float(np.abs(M7 @ np.linalg.inv(M7) - np.eye(384)).max())
    print("order 32: min pivot %.4g, max|M Minv - I| on 64 rows %.3g (bound %.3g)" % (min_pivot, res,
                                                                                      10.0 * ref * N / 384.0))
    assert min_pivot > 0.0 and res <= 10.0 * ref * N / 384.0
    del M_rows, Minv
    n = 20000
    x, a, F = _beads(n, 9)
    smp = np.sort(np.concatenate([[0, 1, S - 1, S, n - 1], np.random.default_rng(4).choice(n, 59, replace=False)]))
    old = np.random.default_rng(5).normal(size=(n, 3))
    got = dev(old)
    ws = ops.HydroWorkspace()
    hp.correct("rpyc", dev(x), dev(a), dev(F), got, workspace=ws)
    u_surf = ops.hydro_velocity("rpyc", MU, dev(x), dev(a), dev(F), dev(s["p"]),
                                torch.zeros(S, dtype=torch.float64, device="cuda"), workspace=ws)
    f_surf = host(hp.surface_forces(u_surf))
    assert np.isfinite(f_surf).all()
    want = pm.double_layer(MU, s["p"], s["n"], s["w"], f_surf, x[smp], old=old[smp], skip_same_index=True, targets=smp)
    assert_bits_equal(host(got)[smp], want, "order 32, 64 beads")
    ws.close()
    hp.close()
