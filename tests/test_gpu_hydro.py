"""N-body hydrodynamics on the GPU (mhip_hydro_velocity): pair terms and ordered sums bit for bit against the numpy
restatement in tests/hydro_model.py, independence of a target's bits from the target set and from the launch shape,
determinism, symmetry of the mobility, the stepper's hydrodynamics= stage, the C++ driver and one call at 10^5 beads."""
import os
import subprocess

import numpy as np
import pytest
import torch

import hydro_model as hm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

C = hm.CHUNK
MU = 0.7
SIZES = (1, 2, 63, 64, 65, 257, C - 1, C, C + 1, 2 * C + 77)
BIG = 3 * C + 5


def _branch_counts(d, ns=None, nt=None):
    sc, sa, tc, tb = d["sc"][:ns], d["sa"][:ns], d["tc"][:nt], d["tb"][:nt]
    br = hm.rpyc_branch(tc[:, None] - sc[None], sa[None], tb[:, None])
    return [int((br == k).sum()) for k in (hm.FAR, hm.OVERLAP, hm.LOCAL, hm.SKIPPED)]


@pytest.fixture(scope="module")
def cloud():
    """BIG sources and BIG targets (different arrays) of polydisperse spheres, radii 0.2 .. 1.2 and some zero, a few
    targets exactly on sources, dense enough for every RPYC branch; the tests take leading slices"""
    d = hm.inputs(BIG, BIG, seed=11)
    assert (d["sa"] == 0.0).any() and (d["tb"] == 0.0).any()
    assert min(_branch_counts(d, 2 * C + 77, 2 * C + 77)) > 0
    d["dev"] = {k: dev(v) for k, v in d.items()}
    return d


def _gpu(kind, d, ns, nt, **kw):
    from mundy_amd import ops
    g = d["dev"]
    return ops.hydro_velocity(kind, MU, g["sc"][:ns], g["sa"][:ns], g["f"][:ns], g["tc"][:nt], g["tb"][:nt], **kw)


def _model(kind, d, ns, nt, **kw):
    return hm.velocity(kind, MU, d["sc"][:ns], d["sa"][:ns], d["f"][:ns], d["tc"][:nt], d["tb"][:nt], **kw)


# ---- 1. pair terms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [1, 63, 257, 20001])
def test_pair_terms_bit_for_bit(nt):
    """ns = 1: every target's result is one term added to +0.0"""
    from mundy_amd import ops
    rng = np.random.default_rng(100 + nt)
    sc, sa, f = rng.uniform(-1.0, 1.0, (1, 3)), np.array([0.9]), rng.normal(size=(1, 3))
    u = rng.normal(size=(nt, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    tc = sc + u * rng.uniform(0.0, 4.0, (nt, 1))
    tb = rng.uniform(0.2, 1.2, nt)
    tb[rng.random(nt) < 0.1] = 0.0
    tc[16::17] = sc  # exact duplicates of the source's centre
    if nt >= 63:
        assert min(_branch_counts(dict(sc=sc, sa=sa, tc=tc, tb=tb))) > 0
    for kind in hm.KINDS:
        got = host(ops.hydro_velocity(kind, MU, dev(sc), dev(sa), dev(f), dev(tc), dev(tb)))
        want = hm.pair_terms(kind, MU, tc, tb, sc[0], sa[0], f[0]) + 0.0
        assert np.isfinite(want).all()
        assert_bits_equal(got, want, "%s pair terms, nt = %d" % (kind, nt))
    # radii are not read by the Stokeslet
    got = host(ops.hydro_velocity("stokes", MU, dev(sc), None, dev(f), dev(tc), None))
    assert_bits_equal(got, hm.pair_terms("stokes", MU, tc, tb, sc[0], sa[0], f[0]) + 0.0, "stokes without radii")


# ---- 2. sums -------------------------------------------------------------------------------------------------------------
def _size_pairs():
    """every ns of SIZES with two nt each, the diagonal's ends, and the rectangular extremes: 24 of the 100 + 2"""
    k = len(SIZES)
    out = []
    for i, ns in enumerate(SIZES):
        out += [(ns, SIZES[(3 * i + 1) % k]), (ns, SIZES[(7 * i + 4) % k])]
    out += [(1, 1), (2 * C + 77, C + 1), (BIG, 1), (1, BIG)]
    return sorted(set(out))


@pytest.mark.parametrize("ns,nt", _size_pairs())
def test_sums_bit_for_bit(cloud, ns, nt):
    from mundy_amd import ops
    rng = np.random.default_rng(ns * 7919 + nt)
    old = rng.normal(size=(nt, 6))
    ws = ops.HydroWorkspace()
    for kind in hm.KINDS:
        want = _model(kind, cloud, ns, nt)
        assert np.isfinite(want).all()
        assert_bits_equal(host(_gpu(kind, cloud, ns, nt)), want, "%s (%d, %d), stride 3" % (kind, ns, nt))
        # stride 6, added last to what the rows hold; the angular half of a row is not touched
        buf = dev(old)
        _gpu(kind, cloud, ns, nt, out=buf, accumulate=True, workspace=ws)
        assert_bits_equal(host(buf)[:, :3], old[:, :3] + want, "%s (%d, %d), stride 6 accumulate" % (kind, ns, nt))
        assert_bits_equal(host(buf)[:, 3:], old[:, 3:], "untouched columns")
        # the other launch shape: the same bits
        for path in ("in_lane", "partial"):
            ws.set_path(path)
            buf3 = dev(old[:, :3].copy())
            _gpu(kind, cloud, ns, nt, out=buf3, accumulate=True, workspace=ws)
            assert ws.last_path() == path
            assert_bits_equal(host(buf3), old[:, :3] + want, "%s (%d, %d), %s" % (kind, ns, nt, path))
            buf6 = dev(old)
            _gpu(kind, cloud, ns, nt, out=buf6, workspace=ws)
            assert_bits_equal(host(buf6)[:, :3], want, "%s (%d, %d), %s, stride 6 store" % (kind, ns, nt, path))
        ws.set_path("auto")
    ws.close()


def test_empty_sets(cloud):
    from mundy_amd import ops
    g = cloud["dev"]
    z = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    z1 = torch.empty((0,), dtype=torch.float64, device="cuda")
    out = dev(np.full((5, 3), 7.0))
    ops.hydro_velocity("rpyc", MU, z, z1, z, g["tc"][:5], g["tb"][:5], out=out)
    assert all_pos_zero(host(out))  # no sources: +0.0
    out = dev(np.full((5, 6), -0.0))
    ops.hydro_velocity("rpyc", MU, z, z1, z, g["tc"][:5], g["tb"][:5], out=out, accumulate=True)
    assert_bits_equal(host(out), np.full((5, 6), -0.0), "accumulate without sources leaves the rows alone")
    assert ops.hydro_velocity("rpy", MU, g["sc"][:9], g["sa"][:9], g["f"][:9], z, z1).shape == (0, 3)


# ---- 3. independence from the target set and the launch shape, 4. determinism ---------------------------------------------
@pytest.fixture(scope="module")
def beads():
    d = hm.inputs(20001, seed=21)
    assert min(_branch_counts(d, None, 300)[:3]) > 0
    d["sample"] = np.sort(np.random.default_rng(2).choice(20001, 64, replace=False))
    d["dev"] = {k: dev(v) for k, v in d.items()}
    return d


@pytest.mark.parametrize("kind", hm.KINDS)
def test_a_targets_bits_do_not_depend_on_the_target_set_or_the_path(beads, kind):
    from mundy_amd import ops
    g, smp = beads["dev"], beads["sample"]
    ws = ops.HydroWorkspace()
    full = host(ops.hydro_velocity(kind, MU, g["sc"], g["sa"], g["f"], workspace=ws))
    auto_path = ws.last_path()
    again = host(ops.hydro_velocity(kind, MU, g["sc"], g["sa"], g["f"], workspace=ws))
    assert_bits_equal(again, full, "two calls")
    idx = torch.from_numpy(smp).cuda()
    tc, tb = g["sc"][idx].contiguous(), g["sa"][idx].contiguous()
    alone = host(ops.hydro_velocity(kind, MU, g["sc"], g["sa"], g["f"], tc, tb, workspace=ws))
    assert_bits_equal(alone, full[smp], "64 targets alone")
    want = hm.velocity(kind, MU, beads["sc"], beads["sa"], beads["f"], beads["sc"][smp], beads["sa"][smp])
    assert_bits_equal(full[smp], want, "the model, for those 64")
    seen = {auto_path}
    for path in ("in_lane", "partial"):
        ws.set_path(path)
        forced = host(ops.hydro_velocity(kind, MU, g["sc"], g["sa"], g["f"], workspace=ws))
        assert ws.last_path() == path
        seen.add(path)
        assert_bits_equal(forced, full, path)
    assert seen == {"in_lane", "partial"}
    ws.close()


def test_launch_rule_takes_both_paths_by_size(cloud):
    """enough target tiles to fill the chip: a lane walks the chunks itself; fewer: chunk groups and the second pass"""
    from mundy_amd import ops
    ns, nt = C + 1, 1024 * 256 + 1
    rng = np.random.default_rng(9)
    sc, sa, f = cloud["sc"][:ns], cloud["sa"][:ns], cloud["f"][:ns]
    lo, hi = sc.min(axis=0), sc.max(axis=0)
    tc, tb = rng.uniform(lo, hi, (nt, 3)), rng.uniform(0.2, 1.2, nt)
    smp = np.concatenate([[0, nt - 1], rng.choice(nt, 62, replace=False)])
    ws = ops.HydroWorkspace()
    got = host(ops.hydro_velocity("rpyc", MU, dev(sc), dev(sa), dev(f), dev(tc), dev(tb), workspace=ws))
    assert ws.last_path() == "in_lane"
    assert_bits_equal(got[smp], hm.velocity("rpyc", MU, sc, sa, f, tc[smp], tb[smp]), "many tiles")
    few = 1024 * 256 - 256  # one tile short of the rule
    ops.hydro_velocity("rpyc", MU, dev(sc), dev(sa), dev(f), dev(tc[:few]), dev(tb[:few]), workspace=ws)
    assert ws.last_path() == "partial"
    _gpu("rpyc", cloud, C, 5, workspace=ws)  # one chunk: nothing to split
    assert ws.last_path() == "in_lane"
    ws.close()


# ---- 5. symmetry ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rpyc", "rpy"])
def test_device_mobility_is_symmetric(cloud, kind):
    from mundy_amd import ops
    n = 2 * C + 77
    x, a = cloud["sc"][:n], cloud["sa"][:n]
    rng = np.random.default_rng(17)
    f, g = rng.normal(size=(n, 3)), rng.normal(size=(n, 3))
    mf = host(ops.hydro_velocity(kind, MU, dev(x), dev(a), dev(f)))
    mg = host(ops.hydro_velocity(kind, MU, dev(x), dev(a), dev(g)))
    _, ag = hm.velocity(kind, MU, x, a, g, want_abs=True)
    bound = 4.0 * (n + 16) * 2.0 ** -53 * float((np.abs(f) * ag).sum())
    diff = abs(float((f * mg).sum()) - float((g * mf).sum()))
    print(kind, "asymmetry", diff, "bound", bound)
    assert diff <= bound


# ---- 6. the stepper ------------------------------------------------------------------------------------------------------
def _chains(seed=8, jitter=0.05):
    from mundy_amd import synth
    d = synth.chains(2, 1000, seed=seed)
    d["center"] = d["center"] + jitter * np.random.default_rng(seed).normal(size=d["center"].shape)  # stretched springs
    return d


def _stepper(d, hydro=..., **kw):
    from mundy_amd import pipeline
    args = dict(dt=d["dt"], viscosity=d["viscosity"], search_buffer=d["skin"],
                springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"])
    if hydro is not ...:
        args["hydrodynamics"] = hydro
    args.update(kw)
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), **args)


def test_stepper_external_velocity_is_dry_plus_noise_plus_hydro():
    from mundy_amd import ops
    d = _chains()
    st = _stepper(d, dict(kind="rpyc"))
    keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
    x0 = host(st.center).copy()
    st.compute_aabb()
    st.generate_neighbor_links()
    st.external_velocity()
    F = host(st.spring_force)
    assert np.abs(F).max() > 1e-3
    # (m_t F) + U_brown: the two existing kernels at the same keys and counters
    base = ops.brownian_velocity(keys, ctr, d["kt"], d["dt"], st.mob_trans, ops.drag_velocity(st.mob_trans, dev(F)))
    want_h = hm.velocity("rpyc", d["viscosity"], x0, d["radius"], F)
    assert_bits_equal(host(st.u_hydro), want_h, "u_hydro")
    assert_bits_equal(host(st.u_ext)[:, :3], host(base)[:, :3] + want_h, "u_ext")
    assert all_pos_zero(host(st.u_ext)[:, 3:])
    assert (host(st.rng_counter) == host(ctr)).all() and st.hydro_step == 1


def test_stepper_hydrodynamic_radius_and_kinds():
    d = _chains()
    n = d["center"].shape[0]
    rad = np.random.default_rng(3).uniform(0.0, 0.8, n)
    for kind, radius, want_r in (("rpy", 0.25, np.full(n, 0.25)), ("stokes", None, d["radius"]), ("rpyc", rad, rad)):
        st = _stepper(d, dict(kind=kind, radius=radius))
        st.compute_aabb()
        st.generate_neighbor_links()
        st.external_velocity()
        smp = np.arange(0, n, 41)
        want = hm.velocity(kind, d["viscosity"], d["center"], want_r, host(st.spring_force), d["center"][smp],
                           want_r[smp])
        assert_bits_equal(host(st.u_hydro)[smp], want, kind)


def test_stepper_update_every():
    d = _chains()
    st = _stepper(d, dict(kind="rpyc", update_every=3))
    seen = []
    for k in range(7):
        before = host(st.u_hydro).copy()
        s = st.step(timed=(k == 0))
        if k == 0:
            names = list(s.timings_ms)
            assert names.index("hydrodynamics") == names.index("springs_brownian") + 1
        changed = not np.array_equal(before.view(np.uint64), host(st.u_hydro).view(np.uint64))
        seen.append(changed)
        assert st.hydro_step == k + 1
    assert seen == [True, False, False, True, False, False, True]


def test_stepper_stale_velocity_is_added_every_step():
    from mundy_amd import ops
    d = _chains()
    st = _stepper(d, dict(kind="rpyc", update_every=3), brownian_kt=0.0)
    st.step()
    stored = host(st.u_hydro).copy()
    assert np.abs(stored).max() > 0
    st.compute_aabb()
    st.generate_neighbor_links()
    st.external_velocity()  # step 1: no update
    assert_bits_equal(host(st.u_hydro), stored, "kept")
    dry = host(ops.drag_velocity(st.mob_trans, st.spring_force))[:, :3]
    assert_bits_equal(host(st.u_ext)[:, :3], dry + stored, "stale u_hydro added")


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_stepper_without_forces_is_the_run_without_the_keyword(model):
    d = _chains(jitter=0.0)
    kw = dict(springs=(d["pairs"], "hookean", 0.0, d["r0"]), brownian_kt=0.0, contact_model=model)
    a, b = _stepper(d, **kw), _stepper(d, dict(kind="rpyc"), **kw)
    for _ in range(3):
        sa, sb = a.step(), b.step()
        assert sa.num_contacts == sb.num_contacts and sa.num_contacts > 0
        assert_bits_equal(host(b.center), host(a.center), "zero forces")
    moved = not np.array_equal(host(a.center), d["center"])
    assert moved  # the contacts of overlapping beads did move something
    assert all_pos_zero(host(b.u_hydro))


def test_stepper_snapshot_restore_across_an_update_boundary():
    d = _chains()
    st = _stepper(d, dict(kind="rpyc", update_every=2))
    st.step()  # the counter is odd now: the three steps below update at their second
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


def test_stepper_reorder_bodies():
    d = _chains()
    n = d["center"].shape[0]
    rad = np.random.default_rng(5).uniform(0.1, 0.8, n)
    a = _stepper(d, dict(kind="rpyc", radius=rad))
    b = _stepper(d, dict(kind="rpyc", radius=rad))
    a.step()
    b.step()
    perm = host(b.reorder_bodies()).astype(np.int64)
    assert not np.array_equal(perm, np.arange(n))
    assert_bits_equal(host(b.u_hydro), host(a.u_hydro)[perm], "the stored velocity moves with its rows")
    assert_bits_equal(host(b.hydro_radius), rad[perm], "and the radii")
    for s in (a, b):  # the next evaluation: the rows in another order, the sums in the constructor's numbering
        s.compute_aabb()
        s.generate_neighbor_links()
        s.external_velocity()
    assert_bits_equal(host(b.center), host(a.center)[perm], "centres")
    Fa = host(a.spring_force)
    assert_bits_equal(host(b.spring_force), Fa[perm], "forces")
    _, A = hm.velocity("rpyc", d["viscosity"], host(a.center), rad, Fa, want_abs=True)
    ua, ub = host(a.u_hydro)[perm], host(b.u_hydro)
    bound = 2.0 * n * 2.0 ** -53 * A[perm]
    assert (np.abs(ub - ua) <= bound).all()
    assert np.abs(ub).max() > 0.0
    assert_bits_equal(ub, ua, "u_hydro of every bead, whatever its row")  # (the sum keeps the constructor's order)


@pytest.mark.parametrize("model", ["lcp", "hertz"])
def test_stepper_runs_with_both_contact_models(model):
    d = _chains()
    st = _stepper(d, dict(kind="rpyc"), contact_model=model)
    for _ in range(20):
        s = st.step()
        assert s.converged
    assert np.isfinite(host(st.center)).all() and np.abs(host(st.u_hydro)).max() > 0


# ---- 7. the C++ driver ---------------------------------------------------------------------------------------------------
def test_hydro_step_app_matches_python():
    import tempfile

    from cpp_apps import build_app, fnv1a
    from mundy_amd import capi, synth
    d = _chains()
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    st = _stepper(d, dict(kind="rpyc", update_every=2))
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d iterations %d max_spring_length %.17g" % (k, s.num_contacts, s.num_iters,
                                                                                     s.max_spring_length))
    exe = build_app("hydro_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
        out = subprocess.run([exe, path, "20", repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]),
                              repr(d["kt"]), repr(d["viscosity"]), str(capi.HYDRO_RPYC), "2"], capture_output=True,
                             text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:8]) for g in got] == lines
    cs = [ln for ln in out.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert cs[2] == fnv1a(host(st.center).reshape(-1).view(np.uint64).tolist())


# ---- 8. one larger call --------------------------------------------------------------------------------------------------
def test_hundred_thousand_beads():
    """10^5 x 10^5 RPYC: 98 chunks, a partial buffer of 98 x 10^5 x 24 bytes; 64 targets against the model"""
    from mundy_amd import ops
    n = 100000
    d = hm.inputs(n, seed=31)
    smp = np.sort(np.concatenate([[0, n - 1], np.random.default_rng(4).choice(n, 62, replace=False)]))
    ws = ops.HydroWorkspace()
    got = host(ops.hydro_velocity("rpyc", MU, dev(d["sc"]), dev(d["sa"]), dev(d["f"]), workspace=ws))
    assert ws.last_path() == "partial"
    ws.close()
    assert np.isfinite(got).all()
    want = hm.velocity("rpyc", MU, d["sc"], d["sa"], d["f"], d["sc"][smp], d["sa"][smp])
    assert_bits_equal(got[smp], want, "10^5 beads, 64 targets")
