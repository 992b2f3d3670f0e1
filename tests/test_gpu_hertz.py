"""Hertzian soft contact on the GPU (contact_model="hertz"): the per-linker force kernel and the operator's body sweep
against the numpy restatement in tests/hertz_model.py, conservation, order independence, the dynamics of the step, the
periodic box, the C++ stepper against the Python one, and one step at full size."""
import subprocess

import numpy as np
import pytest

from hertz_model import body_force_torque, elastic_energy, hertz_force, rod_arms, stiffness

pytestmark = pytest.mark.gpu


def _spheres(rng, n, box):
    c = rng.uniform(0, box, (n, 3))
    return dict(kind="sphere", center=c, radius=rng.uniform(0.4, 0.8, n))


def _rods(rng, n, box):
    from gpu_util import random_rods
    c, q, r, ln = random_rods(rng, n, box)
    return dict(kind="spherocylinder", center=c, quat=q, radius=r, length=ln)


def _mixed(rng, n, box):
    from gpu_util import random_rods
    c, q, r, ln = random_rods(rng, n, box)
    kinds = (np.arange(n) % 2).astype(np.int32)   # 0 sphere, 1 spherocylinder
    shape = np.stack([r, np.where(kinds == 1, ln, 0.0), np.zeros(n)], axis=1)
    return dict(kind="mixed", center=c, quat=q, kinds=kinds, shape=shape, radius=r)


MAKERS = {"sphere": _spheres, "spherocylinder": _rods, "mixed": _mixed}


def _materials(rng, n, per_body):
    if not per_body:
        return 1000.0, 0.3
    return rng.uniform(200.0, 2000.0, n), rng.uniform(0.1, 0.49, n)


def _stepper(b, E, nu, box=None, **kw):
    from gpu_util import dev
    from mundy_amd import pipeline
    tens = lambda v: dev(v) if isinstance(v, np.ndarray) else v  # noqa: E731
    args = dict(contact_model="hertz", youngs_modulus=tens(E), poisson_ratio=tens(nu), periodic_box=box, **kw)
    if b["kind"] == "sphere":
        return pipeline.ContactStepper("sphere", dev(b["center"]), dev(b["radius"]), **args)
    if b["kind"] == "spherocylinder":
        return pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                       dev(b["length"]), **args)
    return pipeline.ContactStepper("mixed", dev(b["center"]), None, dev(b["quat"]), kinds=dev(b["kinds"]),
                                   shape=dev(b["shape"]), **args)


def _contacts(st):
    st.compute_aabb()
    st.generate_neighbor_links(force=True)
    return st.compute_contacts()


def _arms(st, b):
    """the lever arms the operator uses: none (spheres), rod-compressed (rods), the contact routine's (mixed)"""
    from gpu_util import host
    c, pairs = st.contacts, host(st.links.pairs)
    if b["kind"] == "sphere":
        return None, None
    if b["kind"] == "spherocylinder":
        return rod_arms(pairs, host(c["s"]), host(c["t"]), host(st.seg))
    return host(c["ra"]), host(c["rb"])


CASES = [(k, pb) for k in ("sphere", "spherocylinder", "mixed") for pb in (False, True)]


@pytest.mark.parametrize("kind,per_body", CASES)
def test_per_linker_force_matches_the_model(kind, per_body):
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    rng = np.random.default_rng(11)
    n = 3000
    b = MAKERS[kind](rng, n, 18.0)
    E, nu = _materials(rng, n, per_body)
    st = _stepper(b, E, nu)
    c = _contacts(st)
    pairs, sep = host(st.links.pairs), host(c["sep"])
    assert (sep < 0).sum() > 100 and (sep >= 0).sum() > 100
    f, mx = ops.hertz_contact_force(st.links.pairs, c["sep"], dev(b["radius"]),
                                    dev(E) if per_body else E, dev(nu) if per_body else nu)
    f, mx = host(f), float(host(mx)[0])
    f_ref, mx_ref = hertz_force(pairs, sep, b["radius"], E, nu)
    over = sep < 0
    assert np.all(np.abs(f[over] - f_ref[over]) <= 1e-14 * np.abs(f_ref[over]))
    assert_bits_equal(f[~over], np.zeros(int((~over).sum())), "force of the pairs that do not overlap")
    assert mx == mx_ref


def test_per_body_materials_follow_their_bodies():
    """reorder_bodies, snapshot and restore carry per-body youngs_modulus / poisson_ratio tensors like every other
    per-body array (outside growth mode they used to stay behind: the bodies moved, their materials did not)"""
    from gpu_util import assert_bits_equal, host
    rng = np.random.default_rng(11)
    n = 3000
    b = _spheres(rng, n, 18.0)
    E, nu = _materials(rng, n, True)
    st = _stepper(b, E, nu)
    snap = st.snapshot()
    perm = host(st.reorder_bodies()).astype(np.int64)
    assert (perm != np.arange(n)).any() and (np.sort(perm) == np.arange(n)).all()
    assert_bits_equal(host(st.youngs_modulus), E[perm], "youngs_modulus after reorder_bodies")
    assert_bits_equal(host(st.poisson_ratio), nu[perm], "poisson_ratio after reorder_bodies")
    assert_bits_equal(host(st.center), b["center"][perm], "center after reorder_bodies")
    st.step()
    pairs, sep = host(st.links.pairs), host(st.contacts["sep"])
    over = sep < 0
    assert over.sum() > 100
    f, f_ref = host(st.lam), hertz_force(pairs, sep, b["radius"][perm], E[perm], nu[perm])[0]
    assert np.all(np.abs(f[over] - f_ref[over]) <= 1e-14 * np.abs(f_ref[over]))
    st.restore(snap)
    for name, want in (("youngs_modulus", E), ("poisson_ratio", nu), ("center", b["center"]), ("radius", b["radius"])):
        assert_bits_equal(host(getattr(st, name)), want, name + " after restore")


def _check_rows(vel, F, T, scale, mt, mr, arm_max):
    U_ref, W_ref = mt[:, None] * F, (mr[:, None] * T if mr is not None else np.zeros_like(T))
    tol_u = 1e-12 * mt * scale
    assert np.all(np.abs(vel[:, :3] - U_ref) <= tol_u[:, None] + 1e-300)
    if mr is not None:
        tol_w = 1e-12 * mr * scale * arm_max
        assert np.all(np.abs(vel[:, 3:] - W_ref) <= tol_w[:, None] + 1e-300)
    idle = scale == 0.0
    assert not np.any(vel[idle])  # bodies whose linkers all have sep >= 0: zero rows
    return idle


@pytest.mark.parametrize("kind,per_body", CASES)
def test_body_velocities_match_the_reduction_and_conserve(kind, per_body):
    from gpu_util import host
    rng = np.random.default_rng(12)
    n = 3000
    b = MAKERS[kind](rng, n, 18.0)
    E, nu = _materials(rng, n, per_body)
    st = _stepper(b, E, nu)
    s = st.step(integrate=False)
    assert s.num_iters == 0 and s.converged and s.max_overlap > 0.0
    pairs, c = host(st.links.pairs), st.contacts
    f = host(st.lam)
    ai, aj = _arms(st, b)
    F, T, scale = body_force_torque(pairs, host(c["normal"]), f, n, ai, aj)
    vel = host(st.op.body_velocity())
    mt = host(st.mob_trans)
    mr = host(st.mob_rot) if st.mob_rot is not None else None
    arm_max = 0.0 if ai is None else float(max(np.abs(ai).max(), np.abs(aj).max()))
    assert _check_rows(vel, F, T, scale, mt, mr, arm_max).any()
    # conservation: sum F = 0 and sum (x x F + T) = 0, from the velocities and the mobilities
    Fb = vel[:, :3] / mt[:, None]
    Tb = vel[:, 3:] / mr[:, None] if mr is not None else np.zeros_like(Fb)
    tot = scale.sum()
    assert np.all(np.abs(Fb.sum(axis=0)) <= 1e-12 * tot)
    x = b["center"]
    L = np.abs(x).max() + 1.0
    assert np.all(np.abs((np.cross(x, Fb) + Tb).sum(axis=0)) <= 1e-11 * tot * L)


def test_velocities_do_not_depend_on_contact_order():
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    rng = np.random.default_rng(13)
    n = 4000
    b = _rods(rng, n, 19.0)
    st = _stepper(b, 1000.0, 0.3)
    c = _contacts(st)
    mt, mr = st.mob_trans, st.mob_rot
    f, _ = ops.hertz_contact_force(st.links.pairs, c["sep"], dev(b["radius"]))
    op = ops.ContactOperator(st.links.pairs, c["normal"], mt, st.dt, mob_rot=mr, rod=(c["s"], c["t"], st.seg),
                             priority=c["sep"])
    ref = host(op.body_velocity_of(f))
    op.close()
    C = st.links.pairs.shape[0]
    perm = dev(rng.permutation(C)).long()
    P = {k: c[k][perm].contiguous() for k in ("sep", "normal", "s", "t")}
    pairs = st.links.pairs[perm].contiguous()
    fp, _ = ops.hertz_contact_force(pairs, P["sep"], dev(b["radius"]))
    assert_bits_equal(host(fp), host(f)[host(perm)], "forces of the permuted list")
    op = ops.ContactOperator(pairs, P["normal"], mt, st.dt, mob_rot=mr, rod=(P["s"], P["t"], st.seg),
                             priority=P["sep"])
    assert_bits_equal(host(op.body_velocity_of(fp)), ref, "velocity rows with the contacts shuffled")
    op.close()


def test_two_spheres_close_their_overlap_by_dt_m_f():
    from gpu_util import host
    b = dict(kind="sphere", center=np.array([[5.0, 5.0, 5.0], [7.9, 5.0, 5.0]]), radius=np.array([1.0, 2.0]))
    dt = 1e-5
    st = _stepper(b, 1000.0, 0.3, dt=dt)
    s = st.step()
    f = host(st.lam)
    assert s.num_contacts == 1 and f[0] == pytest.approx(18.915669578546606, rel=1e-13)
    assert s.max_overlap == pytest.approx(0.1, rel=1e-13)
    mt = host(st.mob_trans)
    x0, x = b["center"], host(st.center)
    closed = (np.linalg.norm(x[1] - x[0]) - 3.0) - (np.linalg.norm(x0[1] - x0[0]) - 3.0)
    assert closed == pytest.approx(dt * (mt[0] + mt[1]) * f[0], rel=1e-9)


def test_relaxed_rods_lose_elastic_energy_and_overlap():
    from gpu_util import dev, host
    from mundy_amd import ops, pipeline, synth
    n = 10_000
    b = synth.spherocylinders(n, seed=5)
    lcp = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                  dev(b["length"]), search_buffer=0.1, cfg=ops.PGDConfig(max_iters=10000, tol=1e-5))
    for _ in range(2):   # relaxed packing: two steps of the LCP path
        lcp.step(force_rebuild=True)
    r = b["radius"]
    st = pipeline.ContactStepper("spherocylinder", lcp.center.clone(), dev(r), lcp.quat.clone(), dev(b["length"]),
                                 search_buffer=0.1, contact_model="hertz")
    c = _contacts(st)
    pairs, sep = host(st.links.pairs), host(c["sep"])
    mt = host(st.mob_trans)
    k = stiffness(pairs, sep, r)
    assert (k > 0).sum() > 100
    st.dt = 0.1 * 2.0 / float(np.max((mt[pairs[:, 0]] + mt[pairs[:, 1]]) * k))  # a tenth of the explicit limit
    energy, overlap = [], []
    for _ in range(50):
        s = st.step()
        energy.append(elastic_energy(host(st.links.pairs), host(st.contacts["sep"]), r))
        overlap.append(s.max_overlap)
    assert energy[0] > 0.0
    assert all(e1 <= e0 * (1.0 + 1e-12) for e0, e1 in zip(energy, energy[1:])), energy
    assert overlap[-1] < overlap[0], overlap


@pytest.mark.parametrize("kind", ["sphere", "spherocylinder"])
def test_lattice_translation_leaves_velocities_unchanged(kind):
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    rng = np.random.default_rng(14)
    n, L = 2000, 16.0   # a power-of-two box, centres on a 2^-30 grid: a lattice translation is exact
    b = MAKERS[kind](rng, n, L)
    b["center"] = np.round(b["center"] * 2.0 ** 30) / 2.0 ** 30
    box = [L, L, L]
    st = _stepper(b, 1000.0, 0.3, box=box)
    st.step(integrate=False)
    ref = host(st.op.body_velocity())
    assert np.any(ref)
    moved = b["center"].copy()
    moved[0] += [L, 0.0, 0.0]
    moved[7] -= [0.0, L, L]
    pairs = st.links.pairs
    if kind == "sphere":
        sep, normal = ops.contact_spheres(pairs, dev(moved), dev(b["radius"]), box=box)
        f, _ = ops.hertz_contact_force(pairs, sep, dev(b["radius"]))
        op = ops.ContactOperator(pairs, normal, st.mob_trans, st.dt, priority=sep)
        assert_bits_equal(host(op.body_velocity_of(f)), ref, "velocity rows after a lattice translation")
    else:
        cm = dev(moved)
        seg = ops.spherocylinder_segments(cm, st.quat, st.radius, st.length)
        c = ops.contact_spherocylinders(pairs, seg, cm, want_points=False, arms="arclength", box=box)
        f, _ = ops.hertz_contact_force(pairs, c["sep"], dev(b["radius"]))
        op = ops.ContactOperator(pairs, c["normal"], st.mob_trans, st.dt, mob_rot=st.mob_rot,
                                 rod=(c["s"], c["t"], seg), priority=c["sep"])
        vel = host(op.body_velocity_of(f))
        # the segment of a translated rod is recomputed from its new centre: equal to rounding
        scale = np.abs(ref).max()
        assert np.all(np.abs(vel - ref) <= 1e-10 * scale)
    op.close()


@pytest.mark.parametrize("periodic", [False, True])
def test_cpp_hertz_stepper_reproduces_the_python_driver(tmp_path, periodic):
    import torch
    from cpp_apps import build_app, fnv1a_bits as _checksum
    from gpu_util import dev
    from mundy_amd import pipeline, synth
    n = 30_000
    b = synth.spherocylinders(n, seed=43)
    mt, mr = synth.dry_mobility(0.5 * b["length"] + b["radius"])
    inp = tmp_path / "rods.bin"
    with open(inp, "wb") as f:
        f.write(np.uint64(n).tobytes())
        for a in (b["center"], b["quat"], b["radius"], b["length"], mt, mr):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    exe = build_app("hertz_step_app")
    dt, E, nu = 1e-7, 1000.0, 0.3
    box = [float(b["box"])] * 3 if periodic else None
    p = subprocess.run([exe, str(inp), "3", "3.0", "%.17g" % (b["box"] if periodic else 0.0), repr(dt), repr(E), repr(nu)],
                       capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    steps = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("STEP")]
    assert len(steps) == 3
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]), dev(b["length"]),
                                 dt=dt, search_buffer=0.1, mob_trans=dev(mt), mob_rot=dev(mr), periodic_box=box,
                                 contact_model="hertz", youngs_modulus=E, poisson_ratio=nu)
    st.reorder_bodies(cell_size=3.0, lo=[0.0, 0.0, 0.0])
    rebuilt = []
    for k in range(3):
        s = st.step()
        rebuilt.append(s.rebuilt)
        assert int(steps[k][3]) == s.num_contacts and float(steps[k][5]) == s.max_overlap
        assert int(steps[k][7]) == int(s.rebuilt)
    assert rebuilt[0]
    if not periodic:
        assert not all(rebuilt)   # both the build and the refresh of the operator are exercised
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    torch.cuda.synchronize()
    assert line[2] == _checksum(st.center.cpu().numpy()) and line[4] == _checksum(st.quat.cpu().numpy())


def test_full_size_step_holds_the_per_body_checks_on_a_sample():
    from gpu_util import dev, host
    from mundy_amd import pipeline, synth
    n = 1_000_000
    b = synth.spherocylinders(n)
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                 dev(b["length"]), search_buffer=0.1, contact_model="hertz")
    s = st.step(integrate=False)
    assert s.num_contacts > 5_000_000 and s.max_overlap > 0.0
    pairs, c = host(st.links.pairs), st.contacts
    sample = np.sort(np.random.default_rng(15).choice(n, 10_000, replace=False))
    mine = np.isin(pairs[:, 0], sample) | np.isin(pairs[:, 1], sample)
    sub = pairs[mine]
    ai, aj = rod_arms(sub, host(c["s"])[mine], host(c["t"])[mine], host(st.seg))
    F, T, scale = body_force_torque(sub, host(c["normal"])[mine], host(st.lam)[mine], n, ai, aj)
    vel = host(st.op.body_velocity())
    mt, mr = host(st.mob_trans), host(st.mob_rot)
    arm_max = float(max(np.abs(ai).max(), np.abs(aj).max()))
    _check_rows(vel[sample], F[sample], T[sample], scale[sample], mt[sample], mr[sample], arm_max)
