"""GPU parity of the per-body contact force (include/mundy_hip_contact_force.h) and of what the stepper builds on it.

1. The primitive, bit for bit against tests/contact_force_model.py (the device's per-term expressions, every sum the
   correctly rounded one): spheres, vector arms and rods at the wave and workgroup edges of the body count, both strides,
   both entry points, accumulate, exact zeros, no contact at all, every work mapping, and hubs whose forces cancel to
   sum|terms| / |sum| >= 2^25 (an uncompensated sum would fail there).
2. Its bit relations to the two body sweeps, and that it leaves the operator alone.
3. pipeline.ContactStepper: body_contact_force() of every contact model, and hydrodynamics=dict(contact_forces=True) --
   the Hertz force as the first term of the force field -- stage by stage against the models, with the physics the
   mode exists for: a bead that touches nothing feels a distant pair's contact forces through the hydrodynamics."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import chain_model as chm
import contact_force_model as cm
import hydro_model as hm
import hydro_periphery_model as pm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

DT = 5e-3
BODY_COUNTS = (1, 31, 33, 127, 129, 1000)   # the wave and workgroup edges of tests/test_gpu_body_layout.py
KINDS = ("spheres", "arms", "rods")
MAPPINGS = ((0, 2), (32, 4), (5, 8), (8, 16))


@pytest.fixture(scope="module")
def ops():
    import torch
    assert torch.cuda.is_available()
    from mundy_amd import ops as o
    return o


# ---- systems ----------------------------------------------------------------------------------------------------------------
_PROBLEMS = {}


def _problem(oracle, kind, n):
    """a packing of n bodies with its neighbour pairs and contact geometry from the oracle, multipliers with exact zeros
    and a force vector per contact with zero rows; computed once per (kind, n)"""
    if (kind, n) in _PROBLEMS:
        return _PROBLEMS[kind, n]
    from mundy_amd import synth
    if kind == "spheres":
        s = synth.spheres(n, volume_fraction=0.35, seed=78)
        c, r = s["center"], s["radius"]
        lo, hi, R = oracle.grow(oracle.compute_aabb_spheres(c, r), r, 0.3)
        pairs = oracle.search(oracle.SEARCH_SPHERES, lo, hi, c, R).reshape(-1, 2)
        sep, nrm = oracle.contact_spheres(pairs, c, r)
        mt, _ = synth.dry_mobility(r)
        P = dict(N=n, pairs=pairs, sep=sep, normal=nrm, mt=mt, mr=None)
    else:
        b = synth.spherocylinders(n, seed=77)
        c = b["center"]
        aabb = oracle.compute_aabb_spherocylinders(c, b["quat"], b["radius"], b["length"])
        brad = oracle.bounding_radius_spherocylinders(b["radius"], b["length"])
        lo, hi, R = oracle.grow(aabb, brad, 0.1)
        pairs = oracle.search(oracle.SEARCH_AABB, lo, hi, c, R).reshape(-1, 2)
        seg = oracle.spherocylinder_segments(c, b["quat"], b["radius"], b["length"])
        out = oracle.contact_spherocylinders(pairs, seg, c)
        mt, mr = synth.dry_mobility(b["radius"], bounding_radius=brad)
        P = dict(N=n, pairs=pairs, sep=out["sep"], normal=out["normal"], ra=out["ra"], rb=out["rb"], s=out["s"],
                 t=out["t"], seg=seg, mt=mt, mr=mr)
    nc = len(P["pairs"])
    rng = np.random.default_rng(1000 * KINDS.index(kind) + n)
    x = rng.uniform(0.1, 2.0, nc)
    x[rng.random(nc) < 0.3] = 0.0                       # inactive contacts: exact zeros
    fv = rng.normal(size=(nc, 3))
    fv[rng.random(nc) < 0.3] = 0.0
    P.update(kind=kind, pairs=np.ascontiguousarray(P["pairs"], dtype=np.int32), x=x, fv=fv)
    _PROBLEMS[kind, n] = P
    return P


def _geometry(P):
    """the operator's kinematics as the model takes them"""
    if len(P["pairs"]) == 0 or P["kind"] == "spheres":
        return {}
    if P["kind"] == "rods":
        return dict(rod=(P["s"], P["t"], P["seg"]))
    return dict(ra=P["ra"], rb=P["rb"])


def _gpu_op(ops, P):
    if P["kind"] == "rods":
        return ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT, mob_rot=dev(P["mr"]),
                                   rod=(dev(P["s"]), dev(P["t"]), dev(P["seg"])))
    if P["kind"] == "arms" and len(P["pairs"]) > 0:
        # (an operator without a contact has no arms to be told from spheres by: it is built as the sphere operator)
        return ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT, ra=dev(P["ra"]),
                                   rb=dev(P["rb"]), mob_rot=dev(P["mr"]))
    return ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT)


# ---- 1. the primitive against the model -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", BODY_COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_body_force_is_the_model_bit_for_bit(ops, oracle, kind, n):
    P = _problem(oracle, kind, n)
    N, pairs, geo = P["N"], P["pairs"], _geometry(P)
    nc = len(pairs)
    if n > 1:
        assert nc > 0 and (P["x"] == 0.0).any() and (P["x"] != 0.0).any()
    op = _gpu_op(ops, P)
    x, fv = dev(P["x"]), dev(P["fv"])
    rng = np.random.default_rng(5)
    for stride in (3, 6):
        want_x = cm.body_force(N, pairs, x=P["x"], normal=P["normal"], stride=stride, **geo)
        want_v = cm.body_force(N, pairs, force=P["fv"], stride=stride, **geo)
        got = op.body_force(x, stride=stride)
        assert tuple(got.shape) == (N, stride)
        assert_bits_equal(host(got), want_x, "%s n=%d body_force stride %d" % (kind, n, stride))
        assert_bits_equal(host(op.body_force_vector(fv, stride=stride)), want_v,
                          "%s n=%d body_force_vector stride %d" % (kind, n, stride))
        assert_bits_equal(host(op.body_force(x, stride=stride)), want_x, "a second call")
        # accumulate onto a buffer that is not zero: out = old + sum, one more rounding
        old = rng.normal(size=(N, stride)) * 3.0
        buf = dev(old.copy())
        assert op.body_force(x, out=buf, stride=stride, accumulate=True) is buf
        assert_bits_equal(host(buf), cm.body_force(N, pairs, x=P["x"], normal=P["normal"], stride=stride, old=old, **geo),
                          "%s n=%d accumulate stride %d" % (kind, n, stride))
        buf = dev(old.copy())
        op.body_force_vector(fv, out=buf, stride=stride, accumulate=True)
        assert_bits_equal(host(buf), cm.body_force(N, pairs, force=P["fv"], stride=stride, old=old, **geo),
                          "%s n=%d vector accumulate stride %d" % (kind, n, stride))
        # the overwriting call does not read what it overwrites
        buf = dev(np.full((N, stride), np.nan))
        op.body_force(x, out=buf, stride=stride)
        assert_bits_equal(host(buf), want_x, "overwrite of NaN")
    if kind == "spheres" or nc == 0:
        assert all_pos_zero(want_x[:, 3:])               # the torque of a sphere: +0.0
    else:
        assert np.abs(want_x[:, 3:]).max() > 0
    # every work mapping: the result does not depend on it
    want = cm.body_force(N, pairs, x=P["x"], normal=P["normal"], **geo)
    for xcd_tile, lanes in MAPPINGS:
        op.set_work_mapping(xcd_tile, lanes)
        assert_bits_equal(host(op.body_force(x)), want, "%s n=%d mapping %s" % (kind, n, (xcd_tile, lanes)))
        assert_bits_equal(host(op.body_force_vector(fv)), want_v, "%s n=%d vector, mapping %s" % (kind, n, (xcd_tile, lanes)))
    op.close()


@pytest.mark.parametrize("kind", KINDS)
def test_no_multiplier_and_no_contact(ops, oracle, kind):
    import torch
    P = _problem(oracle, kind, 129)
    N, nc = P["N"], len(P["pairs"])
    op = _gpu_op(ops, P)
    old = np.random.default_rng(8).normal(size=(N, 6))
    for stride in (3, 6):
        # every x an exact zero (of either sign), every force row zero: nothing is added.  The forces are +0.0, and the
        # torques of spheres and vector arms; a rod's torque is u x (+0.0), whose components may be -0.0 (the model's)
        z = np.zeros(nc)
        z[::2] = -0.0
        want = cm.body_force(N, P["pairs"], x=z, normal=P["normal"], stride=stride, **_geometry(P))
        assert all_pos_zero(want[:, :3]) and (kind == "rods" or all_pos_zero(want)) and not want.any()
        assert_bits_equal(host(op.body_force(dev(z), stride=stride)), want, "x of zeros")
        assert_bits_equal(host(op.body_force_vector(dev(np.zeros((nc, 3))), stride=stride)), want, "forces of zeros")
        buf = dev(old[:, :stride].copy())
        op.body_force(dev(z), out=buf, stride=stride, accumulate=True)
        assert_bits_equal(host(buf), old[:, :stride], "accumulate of nothing")
    op.close()
    # C = 0: +0.0 rows, or out left alone with accumulate
    none = torch.empty((0, 2), dtype=torch.int32, device="cuda")
    op = ops.ContactOperator(none, torch.empty((0, 3), dtype=torch.float64, device="cuda"), dev(P["mt"]), DT)
    for stride in (3, 6):
        e1, e3 = torch.empty(0, dtype=torch.float64, device="cuda"), torch.empty((0, 3), dtype=torch.float64, device="cuda")
        buf = dev(np.full((N, stride), np.nan))
        op.body_force(e1, out=buf, stride=stride)
        assert all_pos_zero(host(buf))
        assert all_pos_zero(host(op.body_force_vector(e3, stride=stride)))
        keep = np.where(old[:, :stride] > 0, -0.0, old[:, :stride])   # with some -0.0: not even + 0.0 touches them
        buf = dev(keep.copy())
        op.body_force(e1, out=buf, stride=stride, accumulate=True)
        op.body_force_vector(e3, out=buf, stride=stride, accumulate=True)
        assert_bits_equal(host(buf), keep, "C = 0 with accumulate")
    op.close()


# ---- hubs whose forces cancel ------------------------------------------------------------------------------------------------
HUB_DEGREES = (1, 64, 65, 150, 700)


def _hub_system(rng, kind):
    """hubs of the degrees above, each touched by leaves of degree 1 (either side of the pair); x >= 0 with exact
    zeros; normals in +-n pairs on every hub so that its force cancels to 2^-30 .. 2^-40 of sum|terms|"""
    pairs, nrm, x = [], [], []
    leaf = len(HUB_DEGREES)
    for h, deg in enumerate(HUB_DEGREES):
        src = rng.random(deg) < 0.5                  # hub as the source (force -x n) or the target (+x n)
        sign = np.where(src, -1.0, 1.0)
        xs = 10.0 ** rng.uniform(-3, 3, deg)
        ns = rng.normal(size=(deg, 3))
        ns /= np.linalg.norm(ns, axis=1, keepdims=True)
        for k in range(0, deg - 1, 2):
            ns[k + 1] = -sign[k] * sign[k + 1] * ns[k]    # the hub's share of contact k+1 is minus that of contact k ...
            xs[k + 1] = xs[k] * (1.0 + 2.0 ** -rng.uniform(30, 40))  # ... up to 2^-e
            if rng.random() < 0.1:
                xs[k] = xs[k + 1] = 0.0              # inactive: exact zeros, skipped
        if deg % 2 and deg > 1:
            xs[-1] *= 2.0 ** -40                      # the odd one out, small
        for k in range(deg):
            pairs.append((h, leaf) if src[k] else (leaf, h))
            leaf += 1
        nrm.append(ns)
        x.append(xs)
    pairs = np.array(pairs, dtype=np.int32)
    perm = rng.permutation(len(pairs))              # contacts in no particular order
    pairs, nrm, x = pairs[perm], np.concatenate(nrm)[perm], np.concatenate(x)[perm]
    N, nc = leaf, len(pairs)
    S = dict(kind=kind, N=N, pairs=np.ascontiguousarray(pairs), normal=np.ascontiguousarray(nrm), x=x,
             mt=rng.uniform(0.5, 2.0, N), mr=rng.uniform(0.5, 2.0, N))
    if kind == "arms":
        S["ra"], S["rb"] = rng.normal(size=(nc, 3)), rng.normal(size=(nc, 3))
    if kind == "rods":
        p0 = rng.normal(size=(N, 3)) * 10
        seg = np.concatenate([p0, p0 + rng.normal(size=(N, 3)), rng.uniform(0.2, 0.5, (N, 2))], axis=1)
        # arclengths, some outside [0, 1] (clamped by the operator)
        S.update(seg=np.ascontiguousarray(seg), s=rng.uniform(-0.1, 1.1, nc), t=rng.uniform(-0.1, 1.1, nc))
    return S


@pytest.mark.parametrize("kind", KINDS)
def test_hub_forces_that_cancel_are_the_correctly_rounded_sums(ops, kind):
    rng = np.random.default_rng({"spheres": 81, "arms": 82, "rods": 83}[kind])
    S = _hub_system(rng, kind)
    geo = _geometry(S)
    H = len(HUB_DEGREES)
    deg = np.bincount(S["pairs"].ravel(), minlength=S["N"])
    assert tuple(deg[:H]) == HUB_DEGREES and (deg[H:] == 1).all() and max(HUB_DEGREES) >= 500
    want, mag = cm.body_force(S["N"], S["pairs"], x=S["x"], normal=S["normal"], want_terms=True, **geo)
    # the hubs' forces cancel: an uncompensated sum of these terms is wrong in the leading digits
    for h in range(1, H):
        ratio = mag[h].sum() / np.abs(want[h, :3]).max()
        print("hub of degree %d: sum|terms| / |sum| = 2^%.1f" % (HUB_DEGREES[h], np.log2(ratio)))
        assert ratio >= 2.0 ** 25, (HUB_DEGREES[h], ratio)
    # the same force as a vector per contact: -(x n) on the source
    fvec = -(S["x"][:, None] * S["normal"])
    op = _gpu_op(ops, S)
    for xcd_tile, lanes in MAPPINGS + ((-1, -1),):
        op.set_work_mapping(xcd_tile, lanes)
        assert_bits_equal(host(op.body_force(dev(S["x"]))), want, "%s hubs, mapping %s" % (kind, (xcd_tile, lanes)))
        assert_bits_equal(host(op.body_force_vector(dev(fvec))), want, "%s hubs, vector form" % kind)
    old = rng.normal(size=(S["N"], 3))
    buf = dev(old.copy())
    op.body_force(dev(S["x"]), out=buf, stride=3, accumulate=True)
    assert_bits_equal(host(buf), old + want[:, :3], "hubs, accumulate")
    op.close()


# ---- 2. bit relations to the parent's code ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (33, 1000))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_relations_to_the_body_sweeps(ops, oracle, kind, n):
    P = _problem(oracle, kind, n)
    op = _gpu_op(ops, P)
    x, fv = dev(P["x"]), dev(P["fv"])
    FT = host(op.body_force(x))
    # U = m_t F, and W = m_r T for vector arms and rods: the sweep's rows of the same x
    rows = host(op.body_velocity_of(x))
    assert np.abs(rows[:, :3]).max() > 0
    assert_bits_equal(rows[:, :3], P["mt"][:, None] * FT[:, :3], "U = m_t F")
    if kind != "spheres":
        assert np.abs(rows[:, 3:]).max() > 0
        assert_bits_equal(rows[:, 3:], P["mr"][:, None] * FT[:, 3:], "W = m_r T")
    # ... and of the same force vectors
    FTv = host(op.body_force_vector(fv))
    op.body_sweep_vector(fv)
    rows_v = host(op.body_velocity())
    assert_bits_equal(rows_v[:, :3], P["mt"][:, None] * FTv[:, :3], "vector form: U = m_t F")
    if kind != "spheres":
        assert_bits_equal(rows_v[:, 3:], P["mr"][:, None] * FTv[:, 3:], "vector form: W = m_r T")
    # the scalar form is the vector form of -(x n)
    minus_xn = dev(-(P["x"][:, None] * P["normal"]))
    assert_bits_equal(host(op.body_force_vector(minus_xn)), FT, "body_force_vector(-x n) == body_force(x)")
    # two calls give the same bits, and none of them moved the rows the last sweep wrote
    assert_bits_equal(host(op.body_force(x)), FT, "a second call")
    assert_bits_equal(host(op.body_velocity()), rows_v, "the operator's rows after the force calls")
    op.close()


@pytest.mark.parametrize("kind", KINDS)
def test_a_call_after_a_solve_leaves_the_velocities_valid(ops, oracle, kind):
    P = _problem(oracle, kind, 1000)
    nc = len(P["pairs"])
    op = _gpu_op(ops, P)
    lam, g, res = ops.solve_lcp(op, dev(P["sep"]), dev(np.zeros(nc)), ops.PGDConfig(max_iters=20000, tol=1e-7))
    assert res.converged and res.num_iters > 1 and float(lam.max()) > 0
    before = host(op.body_velocity())
    FT = op.body_force(lam)
    assert_bits_equal(host(op.body_velocity()), before, "body_velocity() after body_force")
    assert_bits_equal(host(FT), cm.body_force(P["N"], P["pairs"], x=host(lam), normal=P["normal"], **_geometry(P)),
                      "the force of the solve's multipliers")
    op.close()


def test_refusals_that_need_a_handle(ops, oracle):
    import torch
    from mundy_amd import capi
    lib = capi.load()
    P = _problem(oracle, "rods", 129)
    N, nc = P["N"], len(P["pairs"])
    op = _gpu_op(ops, P)
    x, out = dev(P["x"]), torch.zeros((N, 6), dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    for name, what in (("mhip_contact_op_body_force", "x"), ("mhip_contact_op_body_force_vector", "force")):
        fn = getattr(lib, name)
        with pytest.raises(ValueError, match="%s must not be null" % what):
            capi.check(fn(op._h, None, p(out), 6, 0, None))
        with pytest.raises(ValueError, match="out must not be null"):
            capi.check(fn(op._h, p(x), None, 6, 0, None))
        with pytest.raises(ValueError, match="stride must be 3 or 6"):
            capi.check(fn(op._h, p(x), p(out), 4, 0, None))
        with pytest.raises(ValueError, match="accumulate must be 0 or 1"):
            capi.check(fn(op._h, p(x), p(out), 6, 2, None))
    for bad in (dict(stride=4), dict(accumulate=1), dict(out=out[:, :3])):
        with pytest.raises(ValueError):
            op.body_force(x, **bad)
    with pytest.raises(ValueError, match="x must have shape"):
        op.body_force(x[:-1])
    with pytest.raises(ValueError, match="force must have shape"):
        op.body_force_vector(x)
    # a staged solve in progress, as the sweeps refuse it
    sep = dev(P["sep"])
    v = [torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(4)]
    sp, pc = capi.Space(ops.SPACE_LOWER_BOUND, 0.0, 0.0), capi.PgdConfig(10, 1e-5, ops.RESIDUAL_PROJECTED_DIFF)
    capi.check(lib.mhip_bbpgd_stage_begin(op._h, p(sep), C.byref(sp), C.byref(pc), *(p(t) for t in v), None))
    with pytest.raises(RuntimeError, match="staged solve is in progress"):
        op.body_force(x)
    with pytest.raises(RuntimeError, match="staged solve is in progress"):
        op.body_force_vector(dev(P["fv"]))
    res = capi.SolveResult()
    capi.check(lib.mhip_bbpgd_stage_end(op._h, C.byref(res), None))
    # a partitioned operator: distributed force output is out of scope
    capi.check(lib.mhip_contact_op_set_partition(op._h, 1, N - 1, None, None))
    with pytest.raises(AssertionError, match="partitioned"):
        op.body_force(x)
    with pytest.raises(AssertionError, match="partitioned"):
        op.body_force_vector(dev(P["fv"]))
    capi.check(lib.mhip_contact_op_set_partition(op._h, 0, N, None, None))
    assert all_pos_zero(host(out))                       # no refused call wrote anything
    assert_bits_equal(host(op.body_force(x)), cm.body_force(N, P["pairs"], x=P["x"], normal=P["normal"], **_geometry(P)),
                      "after the refusals")
    op.close()


# ---- 3. the stepper ---------------------------------------------------------------------------------------------------------
def _chains(seed=8, jitter=0.05):
    """the input of tests/test_gpu_hydro.py: two chains of 1000 beads whose beads overlap along the chain"""
    from mundy_amd import synth
    d = synth.chains(2, 1000, seed=seed)
    d["center"] = d["center"] + jitter * np.random.default_rng(seed).normal(size=d["center"].shape)
    return d


def _stepper(d, hydro=..., **kw):
    from mundy_amd import pipeline
    args = dict(dt=d["dt"], viscosity=d["viscosity"], search_buffer=d["skin"], contact_model="hertz",
                springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"])
    if hydro is not ...:
        args["hydrodynamics"] = hydro
    args.update(kw)
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), **args)


def _stages(st):
    """one step of the new mode through the public stages, without the Euler update"""
    st.compute_aabb()
    rebuilt = st.generate_neighbor_links()
    st.compute_contacts()
    st.contact_forces(rebuilt)
    st.external_velocity()
    return st.resolve_collisions(rebuilt)


ON = dict(kind="rpyc", contact_forces=True)


def test_stepper_force_field_holds_the_contact_forces(oracle):
    from mundy_amd import ops
    d = _chains()
    n = d["center"].shape[0]
    st = _stepper(d, ON)
    keys, ctr = st.rng_keys.clone(), st.rng_counter.clone()
    x0 = host(st.center).copy()
    res = _stages(st)
    assert res.converged and res.num_iters == 0
    pairs = host(st.links.pairs)
    # from the oracle's separations: most beads are in an overlap, so most carry a contact force
    sep, nrm = oracle.contact_spheres(pairs, x0, d["radius"])
    touched = np.zeros(n, bool)
    touched[pairs[sep < 0.0].ravel()] = True
    print("%d of %d pairs overlap, %d of %d beads are in an overlap" % ((sep < 0).sum(), len(pairs), touched.sum(), n))
    assert touched.sum() >= n // 2
    lam = host(st.lam)
    assert ((lam > 0) == (sep < 0)).all() and st.contact_pairs is st.links.pairs and st.lam.shape[0] == len(pairs)
    # F = (D lam) + F_spring: the model's contact force of the device's own multipliers, then the springs' term
    Fc = cm.body_force(n, pairs, x=lam, normal=host(st.contacts["normal"]), stride=3)
    assert (np.abs(Fc).max(axis=1) > 0).sum() >= n // 2
    Fs, _, _ = chm.spring_force(n, d["pairs"], "hookean", d["k"], d["r0"], x0)
    assert np.abs(Fs).max() > 1e-3
    F = host(st.spring_force)
    assert_bits_equal(F, Fc + Fs, "F = D lam + F_spring")
    # u_hydro = hydro(F), and U_ext = (m_t F + U_brown) + u_hydro with the existing kernels for the first two terms
    want_h = hm.velocity("rpyc", d["viscosity"], x0, d["radius"], F)
    assert_bits_equal(host(st.u_hydro), want_h, "u_hydro")
    base = ops.brownian_velocity(keys, ctr, d["kt"], d["dt"], st.mob_trans, ops.drag_velocity(st.mob_trans, dev(F)))
    assert_bits_equal(host(st.u_ext)[:, :3], host(base)[:, :3] + want_h, "u_ext")
    assert all_pos_zero(host(st.u_ext)[:, 3:])
    assert st.hydro_step == 1
    # the hydrodynamics of the default mode's force field is another one: the spring force alone
    off = _stepper(d, dict(kind="rpyc"))
    off.compute_aabb()
    off.generate_neighbor_links()
    off.external_velocity()
    assert_bits_equal(host(off.spring_force), Fs, "the default's force field")
    assert (host(off.u_hydro).view(np.uint64) != want_h.view(np.uint64)).any(axis=1).sum() >= n // 2
    # U = U_ext, and body_contact_force() is the model's (F, T = +0.0)
    st.integrate()
    assert_bits_equal(host(st.velocity), host(st.u_ext), "U = U_ext")
    assert np.abs(host(st.center) - (x0 + d["dt"] * host(st.u_ext)[:, :3])).max() <= 2.0 ** -50 * np.abs(x0).max()
    bcf = host(st.body_contact_force())
    assert_bits_equal(bcf[:, :3], Fc, "body_contact_force")
    assert all_pos_zero(bcf[:, 3:])


def test_stepper_max_overlap_statistics_and_timings():
    d = _chains()
    on, off = _stepper(d, ON), _stepper(d, dict(kind="rpyc"))
    a, b = on.step(timed=True), off.step()
    assert a.max_overlap == b.max_overlap > 0 and float(on.max_overlap) == a.max_overlap
    assert a.max_spring_length == b.max_spring_length > 0
    assert a.num_contacts == b.num_contacts == on.contact_pairs.shape[0] == on.lam.shape[0] and a.converged
    assert_bits_equal(host(on.lam), host(off.lam), "the Hertz forces of the first step")
    names = [k for k in a.timings_ms if k not in ("aabb", "broadphase")]
    assert names == ["narrowphase", "hertz_force", "operator", "body_force", "springs_brownian", "hydrodynamics",
                     "integrate"], names


def test_stepper_update_every():
    d = _chains()
    st = _stepper(d, dict(ON, update_every=3))
    seen = []
    for k in range(7):
        before = host(st.u_hydro).copy()
        st.step()
        seen.append(not np.array_equal(before.view(np.uint64), host(st.u_hydro).view(np.uint64)))
        assert st.hydro_step == k + 1
    assert seen == [True, False, False, True, False, False, True]   # recomputed on steps 0, 3, 6


def test_stepper_stale_velocity_is_added_every_step():
    from mundy_amd import ops
    d = _chains()
    st = _stepper(d, dict(ON, update_every=3), brownian_kt=0.0)
    st.step()
    stored = host(st.u_hydro).copy()
    assert np.abs(stored).max() > 0
    _stages(st)  # step 1: no update
    assert_bits_equal(host(st.u_hydro), stored, "kept")
    dry = host(ops.drag_velocity(st.mob_trans, st.spring_force))[:, :3]
    assert_bits_equal(host(st.u_ext)[:, :3], dry + stored, "stale u_hydro added")


def test_stepper_snapshot_restore_across_an_update_boundary():
    d = _chains()
    st = _stepper(d, dict(ON, update_every=2))
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
    a, b = _stepper(d, ON), _stepper(d, ON)
    a.step()
    b.step()
    perm = host(b.reorder_bodies()).astype(np.int64)
    assert not np.array_equal(perm, np.arange(n))
    assert_bits_equal(host(b.u_hydro), host(a.u_hydro)[perm], "the stored velocity moves with its rows")
    with pytest.raises(RuntimeError, match="needs a step"):
        b.body_contact_force()                      # the multipliers are in the old numbering
    for s in (a, b):  # the next evaluation: the rows in another order, the sums in the constructor's numbering
        _stages(s)
    assert_bits_equal(host(b.center), host(a.center)[perm], "centres")
    # every sum of the force stage is rounded once or taken in an order the numbering does not reach
    Fa = host(a.spring_force)
    assert_bits_equal(host(b.spring_force), Fa[perm], "forces")
    assert_bits_equal(host(b.body_contact_force()), host(a.body_contact_force())[perm], "contact forces")
    _, A = hm.velocity("rpyc", d["viscosity"], host(a.center), d["radius"], Fa, want_abs=True)
    ua, ub = host(a.u_hydro)[perm], host(b.u_hydro)
    bound = 2.0 * n * 2.0 ** -53 * A[perm]           # 2 ns 2^-53 sum|term|
    assert (np.abs(ub - ua) <= bound).all()
    assert np.abs(ub).max() > 0.0
    assert_bits_equal(ub, ua, "u_hydro of every bead, whatever its row")  # (the sum keeps the constructor's order)


def test_stepper_with_the_periphery_correction():
    """4 chains of 50 beads inside R = 5 at order 4 (DESIGN 5o's case): the correction is the model's of the same F"""
    from mundy_amd import synth
    R = 5.0
    d = synth.chains(4, 50, seed=8, cell=2.4)
    d["center"] = d["center"] - np.array([2.4, 2.4, 1.2])
    d["center"] = d["center"] + 0.05 * np.random.default_rng(8).normal(size=d["center"].shape)
    assert np.linalg.norm(d["center"], axis=1).max() < R - 0.5
    n = d["center"].shape[0]
    p, w, nn = pm.sphere_quadrature(4, R, invert=True)
    _, M = pm.fill_matrix(p, w, nn, d["viscosity"])
    Minv, min_pivot, _ = pm.gauss_jordan(M)
    st = _stepper(d, dict(ON, periphery=dict(shape="sphere", radius=R, spectral_order=4)))
    assert st.hydro["periphery_min_pivot"] == min_pivot
    x0 = host(st.center).copy()
    _stages(st)
    pairs, lam = host(st.links.pairs), host(st.lam)
    assert (lam > 0).sum() > n // 4
    Fc = cm.body_force(n, pairs, x=lam, normal=host(st.contacts["normal"]), stride=3)
    Fs, _, _ = chm.spring_force(n, d["pairs"], "hookean", d["k"], d["r0"], x0)
    F = host(st.spring_force)
    assert_bits_equal(F, Fc + Fs, "F")
    want_h = hm.velocity("rpyc", d["viscosity"], x0, d["radius"], F)
    want, _, _ = pm.correct("rpyc", d["viscosity"], p, w, nn, Minv, x0, d["radius"], F, old=want_h)
    assert (want.view(np.uint64) != want_h.view(np.uint64)).any(axis=1).all()
    assert_bits_equal(host(st.u_hydro), want, "u_hydro with the correction of the same F")


def test_stepper_without_overlaps_is_the_default_mode():
    """every separation positive (radii scaled down): no contact force, the two orders compute the same numbers; a zero
    may differ in sign"""
    d = _chains()
    c = d["center"]
    d2 = ((c[:, None, :] - c[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(d2, np.inf)
    dmin = float(np.sqrt(d2.min()))      # (beads of one chain may come close: the walk crosses itself)
    d["radius"] = np.full_like(d["radius"], 0.25 * dmin)
    # no noise and a tenth of the time step: five steps of the spring and hydrodynamic velocities (a few units) move a
    # bead by ~1e-3, the gap between the closest two is dmin / 2 = 0.023
    kw = dict(brownian_kt=0.0, dt=0.1 * d["dt"])
    on, off = _stepper(d, ON, **kw), _stepper(d, dict(kind="rpyc"), **kw)
    for _ in range(5):
        a, b = on.step(), off.step()
        assert a.max_overlap == b.max_overlap == 0.0 and a.num_contacts == b.num_contacts > 0
        assert float(on.lam.max()) == 0.0
        ca, cb = host(on.center), host(off.center)
        assert np.array_equal(ca, cb)
        assert np.array_equal(host(on.velocity), host(off.velocity))
        assert np.array_equal(host(on.u_hydro), host(off.u_hydro))
    assert not np.array_equal(ca, d["center"])


def test_body_contact_force_of_every_contact_model(oracle):
    import torch
    from mundy_amd import pipeline, synth
    # before a first step
    s = synth.spheres(300, volume_fraction=0.35, seed=5)
    st = pipeline.ContactStepper("sphere", dev(s["center"]), dev(s["radius"]))
    with pytest.raises(RuntimeError, match="needs a step"):
        st.body_contact_force()
    # LCP spheres: from the multipliers
    st.step()
    lam = host(st.lam)
    assert (lam > 0).any()
    want = cm.body_force(300, host(st.contact_pairs), x=lam, normal=host(st.contacts["normal"]))
    before = host(st.op.body_velocity())
    assert_bits_equal(host(st.body_contact_force()), want, "LCP spheres")
    assert_bits_equal(host(st.op.body_velocity()), before, "the step's velocities")
    # Hertz rods: from the Hertz forces, torques from the arclengths
    b = synth.spherocylinders(300, seed=6)
    mk = lambda **kw: pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]),  # noqa: E731
                                              quat=dev(b["quat"]), length=dev(b["length"]), contact_model="hertz",
                                              dt=1e-5, **kw)
    st = mk()
    with pytest.raises(RuntimeError, match="needs a step"):
        st.body_contact_force()
    st.step(integrate=False)
    c = st.contacts
    lam = host(st.lam)
    assert (lam > 0).any()
    rod = (host(c["s"]), host(c["t"]), host(st.seg))
    want = cm.body_force(300, host(st.contact_pairs), x=lam, normal=host(c["normal"]), rod=rod)
    assert np.abs(want[:, 3:]).max() > 0
    assert_bits_equal(host(st.body_contact_force()), want, "Hertz rods")
    # frictional Hertz rods: from the linker force vectors
    st = mk(hertz_friction=0.5)
    with pytest.raises(RuntimeError, match="needs a step"):
        st.body_contact_force()
    st.step(integrate=False)
    c = st.contacts
    fv = host(st.contact_force)
    assert (np.abs(fv).max(axis=1) > 0).any()
    rod = (host(c["s"]), host(c["t"]), host(st.seg))
    want = cm.body_force(300, host(st.contact_pairs), force=fv, rod=rod)
    assert_bits_equal(host(st.body_contact_force()), want, "frictional Hertz rods")
    # cone friction: from -p, at the surface lever arms of its operator
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), quat=dev(b["quat"]),
                                 length=dev(b["length"]), friction=0.3, cfg=None)
    st.step(integrate=False)
    got = host(st.body_contact_force())
    p = host(st.impulse)
    pairs = host(st.contact_pairs)
    assert (np.abs(p).max(axis=1) > 0).any()
    # (the force alone: the operator's surface arms stay on the device) F_b = sum -p at the source, +p at the target
    want = cm.body_force(300, pairs, force=-p, stride=3)
    assert_bits_equal(got[:, :3], want, "cone friction")
    assert np.abs(got[:, 3:]).max() > 0 and torch.isfinite(st.body_contact_force()).all()


# ---- the physics the feature exists for ---------------------------------------------------------------------------------------
def test_a_distant_bead_feels_the_contact_forces_of_a_pair():
    """no springs, no noise: two overlapping beads and a third at distance 10 that touches nothing"""
    from mundy_amd import pipeline
    c = np.array([[0.0, 0.0, 0.0], [0.8, 0.0, 0.0], [3.0, 10.0, 1.0]])
    r = np.full(3, 0.5)
    mu = 1.0
    mk = lambda hydro: pipeline.ContactStepper("sphere", dev(c), dev(r), dt=1e-4, viscosity=mu, contact_model="hertz",  # noqa: E731
                                               brownian_kt=0.0, hydrodynamics=hydro)
    on, off = mk(dict(kind="rpyc", contact_forces=True)), mk(dict(kind="rpyc"))
    a, b = on.step(integrate=False), off.step(integrate=False)
    assert a.num_contacts == b.num_contacts and abs(a.max_overlap - 0.2) < 1e-15 and a.max_overlap == b.max_overlap
    pairs, lam = host(on.contact_pairs), host(on.lam)
    assert (lam > 0).sum() == 1
    Fc = cm.body_force(3, pairs, x=lam, normal=host(on.contacts["normal"]), stride=3)
    np.testing.assert_array_equal(Fc[2], 0.0)                 # the third bead carries no contact force
    assert Fc[0, 0] < 0 < Fc[1, 0] and Fc[0, 0] == -Fc[1, 0]  # the pair is pushed apart
    assert_bits_equal(host(on.spring_force), Fc, "F is the contact force alone")
    want, A = hm.velocity("rpyc", mu, c, r, Fc, want_abs=True)
    assert_bits_equal(host(on.u_hydro), want, "u_hydro = hydro(F)")
    # the two forces cancel at the third bead only in their leading order: what is left is the force dipole's field.  The
    # model's own lower bound: it is far above the rounding of the two terms it is the difference of (2 terms of size
    # A, each good to a few ulp)
    floor = 64 * 2.0 ** -53 * np.max(A[2])
    assert np.abs(want[2]).max() > 1e3 * floor > 0, (want[2], floor)
    vel_on, vel_off = host(on.u_ext), host(off.u_ext)
    assert_bits_equal(vel_on[2, :3], want[2], "the third bead moves with the hydrodynamic velocity of the contact forces")
    assert np.abs(vel_on[2]).max() > 1e3 * floor
    # the default: the third bead does not move at all -- the force field the hydrodynamics saw held no contact force
    off.integrate()
    assert all_pos_zero(vel_off) and all_pos_zero(host(off.u_hydro))
    assert all_pos_zero(host(off.velocity)[2])
    assert np.abs(host(off.velocity)[:2, 0]).min() > 0        # while the pair itself is pushed apart in both modes
    on.integrate()
    assert np.abs(host(on.velocity)[:2, 0]).min() > 0


# ---- the C++ driver ---------------------------------------------------------------------------------------------------------------
def test_hydro_contact_step_app_matches_python():
    import tempfile

    from cpp_apps import build_app, fnv1a
    from mundy_amd import capi, synth
    d = _chains()
    n = d["center"].shape[0]
    E, nu = 1000.0, 0.3
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    st = _stepper(d, dict(ON, update_every=2), youngs_modulus=E, poisson_ratio=nu)
    lines = []
    for k in range(20):
        s = st.step()
        lines.append("STEP %d contacts %d max_overlap %.17g max_spring_length %.17g" % (k, s.num_contacts, s.max_overlap,
                                                                                      s.max_spring_length))
    exe = build_app("hydro_contact_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
        out = subprocess.run([exe, path, "20", repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]),
                              repr(d["kt"]), repr(d["viscosity"]), str(capi.HYDRO_RPYC), "2", repr(E), repr(nu)],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert [" ".join(g.split()[:8]) for g in got] == lines
    cs = [ln for ln in out.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert cs[2] == fnv1a(host(st.center).reshape(-1).view(np.uint64).tolist())
