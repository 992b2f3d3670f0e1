"""Frictional Hertzian rod contact on the GPU (contact_model="hertz", hertz_friction=mu): the per-linker kernel, the
vector body sweep and the history carry against the numpy model in tests/friction_hertz_model.py, the stepper's
trajectory with rebuilds, a reorder and a restore, the two-rod sled's closed-form steady states, the unchanged
frictionless step, the C++ stepper against the Python one, and one step at full size."""
import subprocess

import numpy as np
import pytest

import friction_hertz_model as fm
from hertz_model import hertz_force, rod_arms, stiffness

pytestmark = pytest.mark.gpu


def _rods(rng, n, box):
    from gpu_util import random_rods
    c, q, r, ln = random_rods(rng, n, box)
    return dict(center=c, quat=q, radius=r, length=ln)


def _stepper(b, **kw):
    from gpu_util import dev
    from mundy_amd import pipeline
    tens = lambda v: dev(v) if isinstance(v, np.ndarray) else v  # noqa: E731
    kw = {k: tens(v) for k, v in kw.items()}
    kw.setdefault("contact_model", "hertz")
    return pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                   dev(b["length"]), **kw)


def _contacts(st):
    st.compute_aabb()
    st.generate_neighbor_links(force=True)
    return st.compute_contacts()


def _random_contact_problem(seed, per_body):
    """>= 10^4 rod contacts of a random packing with random previous velocities and histories"""
    from gpu_util import host
    rng = np.random.default_rng(seed)
    n = 4000
    b = _rods(rng, n, 19.0)
    E, nu = (rng.uniform(200.0, 2000.0, n), rng.uniform(0.1, 0.49, n)) if per_body else (1000.0, 0.3)
    st = _stepper(b)
    c = _contacts(st)
    C = st.links.pairs.shape[0]
    sep = host(c["sep"])
    assert C >= 10_000 and (sep <= 0).sum() > 100 and (sep > 0).sum() > 100
    vel = rng.normal(size=(n, 6))
    hist = rng.normal(scale=0.02, size=(C, 3)) * (rng.uniform(size=(C, 1)) < 0.7)  # some rows without history
    return st, b, c, E, nu, vel, hist


def _device_force(st, b, c, E, nu, vel, hist, mu, damping, dt=1e-3, density=1.3):
    from gpu_util import dev, host
    from mundy_amd import ops
    import torch
    tens = lambda v: dev(v) if isinstance(v, np.ndarray) else v  # noqa: E731
    td = dev(hist)
    out = torch.full((hist.shape[0], 3), 7.0, dtype=torch.float64, device=td.device)  # stale rows must not survive
    f, stats = ops.hertz_friction_force(st.links.pairs, c["sep"], c["normal"], c["s"], c["t"], st.seg, dev(b["radius"]),
                                        dev(vel), td, mu, dt, damping=damping, density=density, youngs_modulus=tens(E),
                                        poisson_ratio=tens(nu), out=out)
    h = stats.cpu()
    return host(f), host(td), float(h[0]), int(h.view(torch.int64)[1])


def _model_force(st, b, c, E, nu, vel, hist, mu, damping, dt=1e-3, density=1.3, parts=None):
    from gpu_util import host
    return fm.friction_force(host(st.links.pairs), host(c["sep"]), host(c["normal"]), host(c["s"]), host(c["t"]),
                             host(st.seg), b["radius"], E, nu, vel, mu, damping[0], damping[1], density, dt, hist,
                             parts=parts)


def _assert_coulomb(parts, mu):
    """|F_t| <= mu |F_n| (1 + 1e-14) on every contact, for the two summands of the force as the kernel forms them (the
    model's, once the force is the model's bit for bit).  Splitting the SUM along the contact normal instead is
    ill-conditioned with normal damping: where the damping term nearly cancels the spring term, |F_n| is a difference of
    two numbers 10^4 times larger and the rounded F_n is parallel to n only to ~1e-12 of its own length."""
    ft, fn = np.linalg.norm(parts["Ft"], axis=1), np.linalg.norm(parts["Fn"], axis=1)
    assert np.any(ft > 0.0) and np.all(ft <= mu * fn * (1.0 + 1e-14))


# ---- 1, 4: per-linker parity and the Coulomb bound ---------------------------------------------------------------------
@pytest.mark.parametrize("per_body", [False, True])
@pytest.mark.parametrize("damping", [(0.0, 0.0), (40.0, 15.0)])
def test_per_linker_force_and_history_are_the_model_bit_for_bit(per_body, damping):
    from gpu_util import assert_bits_equal, host
    prob = _random_contact_problem(21, per_body)
    mu = 0.5
    f, td, mx, sliding = _device_force(*prob, mu, damping)
    parts = {}
    f_ref, td_ref, mx_ref, sliding_ref = _model_force(*prob, mu, damping, parts=parts)
    assert_bits_equal(f, f_ref, "linker forces")
    assert_bits_equal(td, td_ref, "tangential displacements")
    sep = host(prob[2]["sep"])
    away = sep > 0
    assert_bits_equal(f[away], np.zeros((int(away.sum()), 3)), "force rows of separated pairs")
    assert_bits_equal(td[away], np.zeros((int(away.sum()), 3)), "history rows of separated pairs")
    assert mx == mx_ref and mx > 0.0
    assert sliding == sliding_ref and 0 < sliding < int((~away).sum())
    _assert_coulomb(parts, mu)
    if damping == (0.0, 0.0):
        # without damping nothing cancels in F_n: the DEVICE force itself, split along the contact normal, holds the bound
        n = host(prob[2]["normal"])
        fn = (f * n).sum(axis=1)[:, None] * n
        assert np.all(np.linalg.norm(f - fn, axis=1) <= mu * np.linalg.norm(fn, axis=1) * (1.0 + 1e-14))


def test_a_pair_outside_the_bodies_gives_nan_and_is_never_dereferenced():
    from gpu_util import dev, host
    from mundy_amd import ops
    import torch
    f64 = dict(dtype=torch.float64, device="cuda")
    pairs = torch.tensor([[0, 1], [0, 2], [-1, 1]], dtype=torch.int32, device="cuda")
    seg = dev(np.array([[-1.0, 0, 0, 1.0, 0, 0, 0, 0], [0, -1.0, 0.9, 0, 1.0, 0.9, 0, 0]]))
    td = torch.zeros((3, 3), **f64)
    f, _ = ops.hertz_friction_force(pairs, torch.full((3,), -0.1, **f64),
                                    dev(np.tile([0.0, 0.0, 1.0], (3, 1))), torch.full((3,), 0.5, **f64),
                                    torch.full((3,), 0.5, **f64), seg, torch.full((2,), 0.5, **f64),
                                    torch.zeros((2, 6), **f64), td, 0.5, 1e-3)
    f = host(f)
    assert np.isfinite(f[0]).all() and f[0, 2] < 0.0 and np.isnan(f[1:]).all() and np.isnan(host(td)[1:]).all()


# ---- 2: the frictionless limit -----------------------------------------------------------------------------------------
def test_without_friction_and_damping_the_force_is_the_hertz_force_along_the_normal():
    from gpu_util import dev, host
    from mundy_amd import ops
    prob = _random_contact_problem(22, True)
    st, b, c, E, nu = prob[:5]
    f, td, _, _ = _device_force(*prob, 0.0, (0.0, 0.0))
    fh, _ = ops.hertz_contact_force(st.links.pairs, c["sep"], dev(b["radius"]), dev(E), dev(nu))
    fh, n = host(fh), host(c["normal"])
    assert (fh > 0).sum() > 100
    # (test_gpu_hertz's per-linker bar: sqrt(R* delta) delta against sqrt(R*) pow(delta, 1.5))
    assert np.all(np.abs(f + fh[:, None] * n) <= 1e-14 * fh[:, None])
    assert not np.any(td)  # mu = 0: the history is rescaled to nothing


# ---- 3: the vector body sweep ------------------------------------------------------------------------------------------
def _operator(kind, st, c, pairs=None, sel=None):
    from mundy_amd import ops
    g = (lambda v: v) if sel is None else (lambda v: v[sel].contiguous())
    pairs = st.links.pairs if pairs is None else pairs
    if kind == "sphere":
        return ops.ContactOperator(pairs, g(c["normal"]), st.mob_trans, st.dt, priority=g(c["sep"]))
    if kind == "vector":
        return ops.ContactOperator(pairs, g(c["normal"]), st.mob_trans, st.dt, ra=g(c["ra"]), rb=g(c["rb"]),
                                   mob_rot=st.mob_rot, priority=g(c["sep"]))
    return ops.ContactOperator(pairs, g(c["normal"]), st.mob_trans, st.dt, mob_rot=st.mob_rot,
                               rod=(g(c["s"]), g(c["t"]), st.seg), priority=g(c["sep"]))


@pytest.mark.parametrize("kind", ["sphere", "vector", "rod"])
def test_vector_sweep_equals_the_scalar_sweep_and_the_numpy_reduction(kind):
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    rng = np.random.default_rng(23)
    n = 4000
    b = _rods(rng, n, 19.0)
    st = _stepper(b, rod_kinematics=(kind == "rod"))
    c = _contacts(st)
    pairs = host(st.links.pairs)
    C = pairs.shape[0]
    x, _ = ops.hertz_contact_force(st.links.pairs, c["sep"], dev(b["radius"]))
    nrm, xh = host(c["normal"]), host(x)
    assert (xh > 0).sum() > 100
    op = _operator(kind, st, c)
    ref = host(op.body_velocity_of(x))
    # the same terms: -(x n) on side i, +(x n) on side j
    op.body_sweep_vector(dev(-xh[:, None] * nrm))
    assert_bits_equal(host(op.body_velocity()), ref, "rows of body_sweep_vector(-x n) against body_sweep(x)")
    # a force with a tangential part, on the loaded contacts only
    F = -xh[:, None] * nrm + 0.4 * xh[:, None] * rng.normal(size=(C, 3))
    op.body_sweep_vector(dev(F))
    rows = host(op.body_velocity())
    op.close()
    perm = rng.permutation(C)
    pd = dev(perm).long()
    op = _operator(kind, st, c, pairs=st.links.pairs[pd].contiguous(), sel=pd)
    op.body_sweep_vector(dev(F[perm]))
    assert_bits_equal(host(op.body_velocity()), rows, "rows with the contacts shuffled")
    op.close()
    # numpy reduction at 1e-12 of each body's sum |F|
    if kind == "sphere":
        ai = aj = None
    elif kind == "vector":
        ai, aj = host(c["ra"]), host(c["rb"])
    else:
        ai, aj = rod_arms(pairs, host(c["s"]), host(c["t"]), host(st.seg))
    Fb, Tb, scale = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    np.add.at(Fb, pairs[:, 0], F)
    np.add.at(Fb, pairs[:, 1], -F)
    mag = np.linalg.norm(F, axis=1)
    np.add.at(scale, pairs[:, 0], mag)
    np.add.at(scale, pairs[:, 1], mag)
    mt, mr = host(st.mob_trans), host(st.mob_rot)
    assert np.all(np.abs(rows[:, :3] - mt[:, None] * Fb) <= (1e-12 * mt * scale)[:, None] + 1e-300)
    if ai is not None:
        np.add.at(Tb, pairs[:, 0], np.cross(ai, F))
        np.add.at(Tb, pairs[:, 1], np.cross(aj, -F))
        arm_max = float(max(np.abs(ai).max(), np.abs(aj).max()))
        assert np.all(np.abs(rows[:, 3:] - mr[:, None] * Tb) <= (1e-12 * mr * scale * arm_max)[:, None] + 1e-300)
        assert np.any(rows[:, 3:])
    else:
        assert not np.any(rows[:, 3:])
    idle = scale == 0.0
    assert idle.any() and not np.any(rows[idle])  # unloaded bodies: zero rows
    # sum_b F_b = 0 (the couple dist * n x F_t of forces at two centreline points is the reference's: not asserted)
    assert np.all(np.abs((rows[:, :3] / mt[:, None]).sum(axis=0)) <= 1e-12 * scale.sum())


def test_vector_sweep_is_refused_while_a_staged_solve_is_in_progress():
    import ctypes as C
    import torch
    from mundy_amd import capi, ops
    rng = np.random.default_rng(26)
    st = _stepper(_rods(rng, 500, 9.0))
    c = _contacts(st)
    op = _operator("rod", st, c)
    nc = op.num_constraints
    x, g, xt, gt = (torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(4))
    force = torch.zeros((nc, 3), dtype=torch.float64, device="cuda")
    sp = capi.Space(ops.SPACE_LOWER_BOUND, 0.0, 0.0)
    pc = capi.PgdConfig(10, 1e-5, ops.RESIDUAL_PROJECTED_DIFF)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    lib = capi.load()
    capi.check(lib.mhip_bbpgd_stage_begin(op._h, p(c["sep"]), C.byref(sp), C.byref(pc), p(x), p(g), p(xt), p(gt), None))
    res, done = capi.SolveResult(), C.c_int(0)
    local = torch.empty(5, dtype=torch.float64, device="cuda")  # MHIP_BBPGD_REDUCTION_WIDTH
    try:
        capi.check(lib.mhip_bbpgd_stage_body(op._h, 1, None))  # the first iteration of a one-rank staged solve
        capi.check(lib.mhip_bbpgd_stage_constraint(op._h, 1, p(local), None))
        capi.check(lib.mhip_bbpgd_stage_finalize(op._h, 1, p(local), 1, None))
        capi.check(lib.mhip_bbpgd_stage_poll(op._h, C.byref(res), C.byref(done), None))
        with pytest.raises(RuntimeError, match="staged solve is in progress"):
            op.body_sweep_vector(force)
    finally:
        capi.check(lib.mhip_bbpgd_stage_end(op._h, C.byref(res), None))
    op.body_sweep_vector(force)  # accepted again
    op.close()


# ---- 5: the history carry ----------------------------------------------------------------------------------------------
def _canonical(pairs):
    pairs = np.sort(pairs, axis=1)
    pairs = np.unique(pairs[pairs[:, 0] != pairs[:, 1]], axis=0)  # unique sorts by (i, j)
    return np.ascontiguousarray(pairs.astype(np.int32))


@pytest.mark.parametrize("renumber", [True, False])
def test_history_carry_is_the_model_bit_for_bit(renumber):
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    rng = np.random.default_rng(24)
    n = 40_000
    old = _canonical(rng.integers(0, n, size=(101_000, 2)))[:100_000]
    assert old.shape[0] == 100_000
    hist = rng.normal(size=(old.shape[0], 3))
    hist[rng.uniform(size=old.shape[0]) < 0.2] = 0.0
    new_of_old = rng.permutation(n).astype(np.int32) if renumber else None
    mapped = old if new_of_old is None else new_of_old[old]
    keep = mapped[rng.uniform(size=old.shape[0]) < 0.5]
    fresh = rng.integers(0, n, size=(keep.shape[0], 2))
    new = _canonical(np.concatenate([keep, fresh]))
    ref, carried_ref = fm.carry_history(old, hist, new_of_old, new)
    out, carried = ops.carry_contact_history(dev(old), dev(hist), dev(new),
                                             new_of_old=None if new_of_old is None else dev(new_of_old),
                                             want_count=True)
    assert carried == carried_ref and 40_000 < carried < 60_000
    assert_bits_equal(host(out), ref, "carried history")
    if renumber:  # the sign flips are really exercised
        flipped = (new_of_old[old[:, 0]] > new_of_old[old[:, 1]]).mean()
        assert 0.3 < flipped < 0.7


def test_history_carry_of_empty_and_single_lists():
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    empty_p, empty_h = dev(np.zeros((0, 2), dtype=np.int32)), dev(np.zeros((0, 3)))
    one_p, one_h = dev(np.array([[2, 5]], dtype=np.int32)), dev(np.array([[1.0, -2.0, 3.0]]))
    out, k = ops.carry_contact_history(empty_p, empty_h, empty_p, want_count=True)
    assert tuple(out.shape) == (0, 3) and k == 0
    out, k = ops.carry_contact_history(empty_p, empty_h, one_p, want_count=True)
    assert_bits_equal(host(out), np.zeros((1, 3)), "a new pair without an old list")
    assert k == 0
    out, k = ops.carry_contact_history(one_p, one_h, empty_p, want_count=True)
    assert tuple(out.shape) == (0, 3) and k == 0
    out, k = ops.carry_contact_history(one_p, one_h, one_p, want_count=True)
    assert k == 1 and host(out).tolist() == [[1.0, -2.0, 3.0]]
    ren = dev(np.array([0, 1, 7, 3, 4, 6, 5, 2], dtype=np.int32))  # 2 -> 7, 5 -> 6: listed as (6, 7), flipped
    out, k = ops.carry_contact_history(one_p, one_h, dev(np.array([[6, 7]], dtype=np.int32)), new_of_old=ren,
                                       want_count=True)
    assert k == 1 and host(out).tolist() == [[-1.0, 2.0, -3.0]]
    out, k = ops.carry_contact_history(one_p, one_h, dev(np.array([[2, 6]], dtype=np.int32)), want_count=True)
    assert k == 0 and host(out).tolist() == [[0.0, 0.0, 0.0]]


@pytest.mark.parametrize("old", [[[1, 3], [0, 2]], [[0, 2], [0, 2]], [[0, 1], [3, 2]], [[0, 1], [-1, 2]]])
def test_history_carry_refuses_an_unrenumbered_list_that_is_not_canonical(old):
    from gpu_util import dev
    from mundy_amd import ops
    pairs = dev(np.array(old, dtype=np.int32))
    hist = dev(np.ones((2, 3)))
    new = dev(np.array([[0, 2]], dtype=np.int32))
    with pytest.raises(ValueError, match="not canonical"):
        ops.carry_contact_history(pairs, hist, new)
    # a renumbering sorts: the same list is then accepted ((3, 2) is the pair {2, 3}, a negative index carries nothing)
    ident = dev(np.arange(4, dtype=np.int32))
    if min(map(min, old)) >= 0:
        out = ops.carry_contact_history(pairs, hist, new, new_of_old=ident)
        assert tuple(out.shape) == (1, 3)


# ---- 6: the stepper's trajectory ---------------------------------------------------------------------------------------
def _relaxed_rods(n, seed=5):
    """rods of synth's packing after two steps of the LCP path (host arrays)"""
    from gpu_util import dev, host
    from mundy_amd import ops, pipeline, synth
    b = synth.spherocylinders(n, seed=seed)
    lcp = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                  dev(b["length"]), search_buffer=0.1, cfg=ops.PGDConfig(max_iters=10000, tol=1e-5))
    for _ in range(2):
        lcp.step(force_rebuild=True)
    return dict(center=host(lcp.center).copy(), quat=host(lcp.quat).copy(), radius=b["radius"], length=b["length"])


def _explicit_dt(b):
    """a tenth of the explicit limit 2 / max (m_i + m_j) k_c of the packing's stiffest contact"""
    from gpu_util import host
    st = _stepper(b, search_buffer=0.1)
    c = _contacts(st)
    pairs, mt = host(st.links.pairs), host(st.mob_trans)
    k = stiffness(pairs, host(c["sep"]), b["radius"])
    assert (k > 0).sum() > 100
    return 0.1 * 2.0 / float(np.max((mt[pairs[:, 0]] + mt[pairs[:, 1]]) * k))


MU, DAMPING, STEPS = 0.5, (30.0, 10.0), 50


def _buffer_for_rebuilds(b, dt):
    """a search buffer the run outgrows at least twice more: the list is rebuilt when a centre has moved half the buffer
    since the last build, and over the run the farthest body moves D, so with buffer / 2 = D / 6 at least
    D / (D / 6 + one step) - 1 >= 3 rebuilds follow the first"""
    from gpu_util import host
    st = _stepper(b, dt=dt, search_buffer=1.0, hertz_friction=MU, hertz_damping=DAMPING)
    x0 = b["center"]
    for _ in range(STEPS):
        st.step()
    return float(np.linalg.norm(host(st.center) - x0, axis=1).max()) / 3.0


def _run_and_check_against_the_model(b, dt, buffer, reorder_at=None, restore_at=None):
    """steps the frictional stepper; at every step the model, fed with the stepper's own contacts, previous velocity
    and its OWN history (a dict keyed by the pair in the original numbering, oriented low id -> high id), must give the
    stepper's force and history bit for bit.  Returns per step {pair: (force, history)} in the original numbering."""
    from gpu_util import assert_bits_equal, host
    st = _stepper(b, dt=dt, search_buffer=buffer, hertz_friction=MU, hertz_damping=DAMPING)
    n = b["radius"].shape[0]
    ids = np.arange(n)       # original id of the body in each row
    history = {}             # (id_lo, id_hi) -> tang_disp of "hi relative to lo"
    rebuilds, records, stats = [], [], []
    for k in range(STEPS):
        if k == reorder_at:
            perm = host(st.reorder_bodies()).astype(np.int64)
            ids = ids[perm]
        if k == restore_at:  # a step taken and thrown away: the restored state must step as if it had not been
            snap = st.snapshot()
            st.step(force_rebuild=True)
            st.restore(snap)
        prev = host(st.prev_velocity).copy()
        s = st.step()
        pairs, c = host(st.links.pairs), st.contacts
        gi, gj = ids[pairs[:, 0]], ids[pairs[:, 1]]
        sign = np.where(gi < gj, 1.0, -1.0)
        keys = list(zip(np.minimum(gi, gj).tolist(), np.maximum(gi, gj).tolist()))
        zero = np.zeros(3)
        hist = np.array([history.get(key, zero) for key in keys]).reshape(-1, 3) * sign[:, None]
        if s.rebuilt and k > 0:
            rebuilds.append(k)
            assert np.any(hist, axis=1).sum() >= 1 and st.last_carried >= 1  # a non-zero row is carried
        f_ref, td_ref, mx_ref, sliding_ref = fm.friction_force(
            pairs, host(c["sep"]), host(c["normal"]), host(c["s"]), host(c["t"]), host(st.seg), b["radius"], 1000.0, 0.3,
            prev, MU, DAMPING[0], DAMPING[1], 1.0, dt, hist)
        f, td = host(st.contact_force), host(st.tang_disp)
        assert_bits_equal(f, f_ref, "linker forces at step %d" % k)
        assert_bits_equal(td, td_ref, "tangential displacements at step %d" % k)
        assert s.max_overlap == mx_ref and s.num_sliding == sliding_ref
        live = np.flatnonzero(np.any(td_ref, axis=1) | np.any(f_ref, axis=1))
        history = {keys[r]: td_ref[r] * sign[r] for r in live.tolist()}
        records.append({keys[r]: (f_ref[r] * sign[r], td_ref[r] * sign[r]) for r in live.tolist()})
        stats.append((s.num_contacts, s.num_sliding))
    return st, ids, rebuilds, records, stats


@pytest.fixture(scope="module")
def trajectory_setup():
    b = _relaxed_rods(2000)
    dt = _explicit_dt(b)
    return b, dt, _buffer_for_rebuilds(b, dt)


def test_stepper_trajectory_is_the_model_step_by_step_with_rebuilds(trajectory_setup):
    b, dt, buffer = trajectory_setup
    st, _, rebuilds, records, stats = _run_and_check_against_the_model(b, dt, buffer)
    assert len(rebuilds) >= 2, rebuilds
    assert any(k for _, k in stats) and any(len(r) > 100 for r in records)  # friction acts, some contacts slide


def _assert_same_records(a, b):
    for k, (ra, rb) in enumerate(zip(a, b)):
        assert ra.keys() == rb.keys(), "contact sets differ at step %d" % k
        for key, (f, td) in ra.items():
            assert f.tobytes() == rb[key][0].tobytes() and td.tobytes() == rb[key][1].tobytes(), (k, key)


def test_a_reorder_leaves_per_pair_histories_and_forces_unchanged(trajectory_setup):
    from gpu_util import assert_bits_equal, host
    b, dt, buffer = trajectory_setup
    st0, _, _, rec0, _ = _run_and_check_against_the_model(b, dt, buffer)
    st1, ids, _, rec1, _ = _run_and_check_against_the_model(b, dt, buffer, reorder_at=20)
    assert not np.array_equal(ids, np.arange(ids.shape[0]))
    # per pair in the original numbering, oriented low id -> high id: bit for bit (the sign is the orientation's)
    _assert_same_records(rec0, rec1)


def test_snapshot_restore_then_step_gives_the_same_bits(trajectory_setup):
    from gpu_util import assert_bits_equal, host
    b, dt, buffer = trajectory_setup
    st0, _, _, rec0, _ = _run_and_check_against_the_model(b, dt, buffer)
    st1, _, _, rec1, _ = _run_and_check_against_the_model(b, dt, buffer, restore_at=25)
    _assert_same_records(rec0, rec1)
    assert_bits_equal(host(st1.center), host(st0.center), "centres after a restore in mid run")
    assert_bits_equal(host(st1.quat), host(st0.quat), "orientations after a restore in mid run")


# ---- 7: the two-rod sled -----------------------------------------------------------------------------------------------
def _sled(pull, mu, steps=1000):
    from gpu_util import dev, host
    from mundy_amd import pipeline
    _, _, _, delta, _, mt = fm.sled_constants()
    S = fm.SLED
    h = np.sqrt(0.5)
    # the library's rod axis is q * zhat: a quarter turn about y puts it along x, one about -x along y
    b = dict(center=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0 * S["r"] - delta]]),
             quat=np.array([[h, 0.0, h, 0.0], [h, -h, 0.0, 0.0]]), radius=np.array([S["r"], S["r"]]),
             length=np.array([S["length_bottom"], S["length_top"]]))
    st = _stepper(b, dt=S["dt"], youngs_modulus=S["E"], poisson_ratio=S["nu"], hertz_friction=mu,
                  mob_trans=np.array([0.0, mt]), mob_rot=np.array([0.0, 1.0]))
    ext = dev(np.array([[0.0, 0.0, 0.0], [pull, 0.0, -S["press"]]]))
    sliding = []
    for _ in range(steps):
        s = st.step(external_force=ext)
        assert s.num_contacts == 1
        sliding.append(s.num_sliding)
    assert np.array_equal(host(st.center)[0], [0.0, 0.0, 0.0])
    return st, sliding


def test_sled_sticks_below_the_coulomb_bound():
    from gpu_util import host
    _, kt, _, _, hp, _ = fm.sled_constants()
    st, sliding = _sled(0.3, 0.5)
    assert not any(sliding)
    x = host(st.center)[1, 0]
    assert abs(x - 0.3 / (hp * kt)) <= 1e-9 * 0.3 / (hp * kt) and abs(x - 4.7437957e-3) < 1e-9
    assert np.all(np.abs(host(st.velocity)[1]) < 1e-12)


def test_sled_slides_above_it_at_the_closed_form_speed():
    from gpu_util import host
    _, kt, _, _, hp, mt = fm.sled_constants()
    st, sliding = _sled(0.8, 0.5)
    assert all(k == 1 for k in sliding[-100:])
    v = host(st.velocity)[1]
    v_ref = mt * (0.8 - 0.5 * fm.SLED["press"])
    assert abs(v[0] - v_ref) <= 1e-9 * v_ref and abs(v_ref - 6.366197723) < 1e-8
    td = float(np.linalg.norm(host(st.tang_disp)[0]))
    td_ref = 0.5 * fm.SLED["press"] / (hp * kt)
    assert abs(td - td_ref) <= 1e-9 * td_ref and abs(td_ref - 7.90633e-3) < 1e-7


def test_external_force_stays_refused_without_the_new_mode():
    rng = np.random.default_rng(27)
    b = _rods(rng, 50, 6.0)
    st = _stepper(b)
    from gpu_util import dev
    with pytest.raises(ValueError, match="external_force belongs to the chain step"):
        st.step(external_force=dev(np.zeros((50, 3))))
    fr = _stepper(b, hertz_friction=0.5)
    with pytest.raises(ValueError, match="shape"):
        fr.step(external_force=dev(np.zeros((49, 3))))


# ---- 8: the keyword off ------------------------------------------------------------------------------------------------
def test_hertz_step_without_the_keyword_is_the_step_through_the_old_entry_points():
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops
    b = _relaxed_rods(2000, seed=6)
    dt = _explicit_dt(b)
    st = _stepper(b, dt=dt, search_buffer=0.05)
    # the frictionless step as it was, entry point by entry point
    center, quat = dev(b["center"]), dev(b["quat"])
    radius, length = dev(b["radius"]), dev(b["length"])
    links = ops.GenNeighborLinks().set_search_buffer(0.05).set_search_kind(ops.SEARCH_AABB).concretize()
    brad = ops.bounding_radius_spherocylinders(radius, length)
    mt, mr = st.mob_trans.clone(), st.mob_rot.clone()
    op, rebuilds = None, 0
    for k in range(12):
        s = st.step()
        assert s.num_sliding == 0
        aabb = ops.compute_aabb_spherocylinders(center, quat, radius, length)
        rebuilt = links.generate(aabb, center, brad)
        rebuilds += int(rebuilt)
        assert rebuilt == s.rebuilt
        seg = ops.spherocylinder_segments(center, quat, radius, length)
        c = ops.contact_spherocylinders(links.pairs, seg, center, want_points=False, arms="arclength")
        f, mx = ops.hertz_contact_force(links.pairs, c["sep"], radius, 1000.0, 0.3)
        if rebuilt or op is None:
            if op is not None:
                op.close()
            op = ops.ContactOperator(links.pairs, c["normal"], mt, dt, mob_rot=mr, rod=(c["s"], c["t"], seg),
                                     priority=c["sep"])
        else:
            op.refresh(c["normal"], rod=(c["s"], c["t"], seg))
        op.body_sweep(f)
        ops.integrate_euler(dt, op.body_velocity(), center, quat)
        assert float(mx.item()) == s.max_overlap
        assert_bits_equal(host(st.center), host(center), "centres at step %d" % k)
        assert_bits_equal(host(st.quat), host(quat), "orientations at step %d" % k)
    assert 1 <= rebuilds < 12   # both the build and the refresh of the operator


# ---- 9: the C++ stepper -------------------------------------------------------------------------------------------------
def test_cpp_frictional_stepper_reproduces_the_python_driver(tmp_path, trajectory_setup):
    from cpp_apps import build_app, fnv1a_bits as _checksum
    from gpu_util import host
    from mundy_amd import synth
    b, dt, buffer = trajectory_setup
    n = b["radius"].shape[0]
    mt, mr = synth.dry_mobility(0.5 * b["length"] + b["radius"])
    inp = tmp_path / "rods.bin"
    with open(inp, "wb") as f:
        f.write(np.uint64(n).tobytes())
        for a in (b["center"], b["quat"], b["radius"], b["length"], mt, mr):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    exe = build_app("friction_hertz_step_app")
    steps, reorder_at = 30, 12
    p = subprocess.run([exe, str(inp), str(steps), "3.0", str(reorder_at), repr(dt), "1000.0", "0.3", repr(MU),
                        repr(DAMPING[0]), repr(DAMPING[1]), "1.0", repr(buffer)], capture_output=True, text=True,
                       timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("STEP")]
    assert len(lines) == steps
    st = _stepper(b, dt=dt, search_buffer=buffer, hertz_friction=MU, hertz_damping=DAMPING, mob_trans=mt, mob_rot=mr)
    rebuilds = 0
    for k in range(steps):
        if k == reorder_at:
            st.reorder_bodies(cell_size=3.0, lo=[0.0, 0.0, 0.0])
        s = st.step()
        w = dict(zip(lines[k][2::2], lines[k][3::2]))
        assert int(w["contacts"]) == s.num_contacts and float(w["max_overlap"]) == s.max_overlap, k
        assert int(w["rebuilt"]) == int(s.rebuilt) and int(w["sliding"]) == s.num_sliding, k
        if s.rebuilt and k > 0:
            rebuilds += 1
            assert int(w["carried"]) == st.last_carried > 0, k
        assert w["center"] == _checksum(host(st.center)), k
        assert w["force"] == _checksum(host(st.contact_force)), k
        assert w["tang_disp"] == _checksum(host(st.tang_disp)), k
    assert rebuilds >= 2   # the reorder's and at least one of the buffer's
    last = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert last[2] == _checksum(host(st.center)) and last[4] == _checksum(host(st.quat))


# ---- 10: full size ------------------------------------------------------------------------------------------------------
def test_full_size_step_holds_the_sweep_and_coulomb_checks_on_a_sample():
    import torch
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import pipeline, synth
    n = 1_000_000
    b = synth.spherocylinders(n)
    mu = 0.5
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                 dev(b["length"]), search_buffer=0.1, contact_model="hertz", hertz_friction=mu)
    # previous velocities that make the contacts shear (before the first step they are zero: no tangential force)
    gen = torch.Generator(device="cuda").manual_seed(28)
    st.prev_velocity.copy_(torch.randn((n, 6), dtype=torch.float64, device="cuda", generator=gen) * 50.0)
    prev = host(st.prev_velocity).copy()
    s = st.step(integrate=False)
    assert s.num_contacts > 5_000_000 and s.max_overlap > 0.0 and s.num_sliding > 0
    rng = np.random.default_rng(29)
    pairs, c = host(st.links.pairs), st.contacts
    # 10^4 sampled contacts of the contact branch: the model's force bit for bit, and the Coulomb bound on its summands
    F = host(st.contact_force)
    live = np.flatnonzero(host(c["sep"]) <= 0)
    pick = np.sort(rng.choice(live, 10_000, replace=False))
    parts = {}
    f_ref, td_ref, _, _ = fm.friction_force(
        pairs[pick], host(c["sep"])[pick], host(c["normal"])[pick], host(c["s"])[pick], host(c["t"])[pick],
        host(st.seg), b["radius"], 1000.0, 0.3, prev, mu, 0.0, 0.0, 1.0, st.dt, np.zeros((pick.shape[0], 3)),
        parts=parts)
    assert_bits_equal(F[pick], f_ref, "sampled linker forces")
    assert_bits_equal(host(st.tang_disp)[pick], td_ref, "sampled tangential displacements")
    _assert_coulomb(parts, mu)
    # the vector sweep against the numpy reduction on 10^4 sampled bodies
    sample = np.sort(rng.choice(n, 10_000, replace=False))
    mine = np.isin(pairs[:, 0], sample) | np.isin(pairs[:, 1], sample)
    sub, Fs = pairs[mine], F[mine]
    ai, aj = rod_arms(sub, host(c["s"])[mine], host(c["t"])[mine], host(st.seg))
    Fb, Tb, scale = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n)
    np.add.at(Fb, sub[:, 0], Fs)
    np.add.at(Fb, sub[:, 1], -Fs)
    np.add.at(Tb, sub[:, 0], np.cross(ai, Fs))
    np.add.at(Tb, sub[:, 1], np.cross(aj, -Fs))
    mag = np.linalg.norm(Fs, axis=1)
    np.add.at(scale, sub[:, 0], mag)
    np.add.at(scale, sub[:, 1], mag)
    vel = host(st.op.body_velocity())[sample]
    mt, mr = host(st.mob_trans)[sample], host(st.mob_rot)[sample]
    arm_max = float(max(np.abs(ai).max(), np.abs(aj).max()))
    assert np.all(np.abs(vel[:, :3] - mt[:, None] * Fb[sample]) <= (1e-12 * mt * scale[sample])[:, None] + 1e-300)
    assert np.all(np.abs(vel[:, 3:] - mr[:, None] * Tb[sample])
                  <= (1e-12 * mr * scale[sample] * arm_max)[:, None] + 1e-300)
    idle = scale[sample] == 0.0
    assert not np.any(vel[idle])
