"""GPU parity of the LCP against a hydrodynamic mobility (include/mundy_hip_hydro_solve.h).

1. apply_hydro, y and the body rows, bit for bit against the composition of the public calls the header names.
2. The solve against tests/hydro_solve_model.py: the four vectors, the count and the residual bit for bit after 1, 2 and 5
   iterations and at convergence.
3. The dry limit without a model: a mobility of viscosity 1e200 gives the bits of mhip_bbpgd_solve_contact.
4. One contact between two equal beads against the closed-form multiplier, both RPYC branches.
5. The cold tier's trap: an inactive contact's gradient and a lone bead's row move with forces far away, and the
   operator's tiering mode does not reach the hydrodynamic solve.
6. The LCP's conditions and the header's bit relations at convergence on the main case.
7. Sparse sources: hydro_velocity with the switch on against off, bit for bit, in both launch shapes.
The inputs are hydro_solve_model's; tests/test_hydro_solve_host.py asserts the model's convergence on them, so no test
here can pass with converged == False."""
import numpy as np
import pytest

import chain_model as chm
import hydro_model as hm
import hydro_periphery_model as pm
import hydro_solve_model as hsm
from gpu_util import all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

PERIPHERY = dict(order=9, radius=12.0)  # 200 nodes
_SOLVED = {}
case_of = hsm.case_of


def model_solution(name, max_iters=1000, tol=1e-8, periphery=None):
    """the model's solve from x0 = 0, computed once per (case, max_iters, tol) and left unchanged"""
    key = (name, max_iters, tol, periphery is not None)
    if key not in _SOLVED:
        c = case_of(name)
        _SOLVED[key] = hsm.solve(hsm.Operator(c, "rpyc", periphery), c["q"], np.zeros(len(c["q"])), max_iters, tol)
    return _SOLVED[key]


@pytest.fixture(scope="module")
def ops():
    import torch
    assert torch.cuda.is_available()
    from mundy_amd import ops as o
    return o


@pytest.fixture(scope="module")
def periphery(ops):
    """the sphere of radius 12 at spectral order 9 (200 nodes), inverted on the device; its inverse for the model"""
    pts, w, nrm = pm.sphere_quadrature(PERIPHERY["order"], PERIPHERY["radius"], include_poles=False, invert=True)
    P = ops.HydroPeriphery(dev(pts), dev(w), dev(nrm), 1.0)
    P.fill_matrix()
    assert P.invert() > 0.0
    return P, dict(points=pts, weights=w, normals=nrm, inverse=host(P.matrix()), viscosity=1.0,
                   skip_same_index=True)


class Gpu:
    """a case on the device: the sphere operator, the mobility and a workspace of its own"""

    def __init__(self, ops, c, kind="rpyc", periphery=None, skip=True, viscosity=None):
        self.ops, self.c, self.kind, self.P, self.skip = ops, c, kind, periphery, skip
        self.mu = c["viscosity"] if viscosity is None else viscosity
        self.ws = ops.HydroWorkspace()
        self.center, self.a = dev(c["center"]), dev(c["hydro_radius"])
        self.op = ops.ContactOperator(dev(c["pairs"].reshape(-1, 2)), dev(c["normal"].reshape(-1, 3)), dev(c["mob_trans"]),
                                      c["dt"])
        self.mob = ops.HydroMobility(kind, self.mu, self.center, self.a, periphery=periphery, skip_same_index=skip,
                                     workspace=self.ws)
        self.q = dev(c["q"])

    def composed(self, x):
        """(y, rows) of the header's composition of public calls"""
        ops, op = self.ops, self.op
        F = op.body_force(x, stride=3)
        op.body_sweep(x)
        U = op.body_velocity()
        ops.hydro_velocity(self.kind, self.mu, self.center, self.a, F, out=U, accumulate=True, workspace=self.ws)
        if self.P is not None:
            self.P.correct(self.kind, self.center, self.a, F, U, skip_same_index=self.skip, workspace=self.ws)
        return self.c["dt"] * op.constraint_rate(U), U

    def solve(self, x0=None, max_iters=1000, tol=1e-8, mobility=True):
        import torch
        x = torch.zeros_like(self.q) if x0 is None else dev(x0)
        state = (x, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x))
        cfg = self.ops.PGDConfig(max_iters=max_iters, tol=tol)
        _, _, res = self.ops.solve_lcp(self.op, self.q, x, cfg, state=state, mobility=self.mob if mobility else None)
        out = dict(zip(("x", "g", "x_tmp", "g_tmp"), (host(t) for t in state)))
        out.update(rows=host(self.op.body_velocity()), num_iters=res.num_iters, residual=res.residual,
                   converged=res.converged)
        return out


def assert_same_solution(got, want, what, keys=("x", "g", "x_tmp", "g_tmp", "rows")):
    print("%s: %d iterations, residual %.17g (want %d, %.17g)" % (what, got["num_iters"], got["residual"],
                                                                   want["num_iters"], want["residual"]))
    assert got["num_iters"] == want["num_iters"] and got["converged"] == want["converged"], what
    assert_bits_equal(np.array([got["residual"]]), np.array([want["residual"]]), what + " residual")
    for k in keys:
        assert_bits_equal(got[k], want[k], "%s %s" % (what, k))


# ---- 1. apply_hydro against the composition -----------------------------------------------------------------------------------
def _xs(nc):
    rng = np.random.default_rng(11)
    x = rng.uniform(0.0, 2.0, nc)
    x[rng.random(nc) < 0.4] = 0.0
    one = np.zeros(nc)
    if nc:
        one[nc // 2] = 1.5
    return dict(random=x, zero=np.zeros(nc), one=one)


# (skip_same_index is the periphery correction's argument: without a periphery it has nothing to change)
@pytest.mark.parametrize("with_periphery,skip", ((False, True), (True, True), (True, False)))
@pytest.mark.parametrize("kind", ("rpyc", "rpy"))
def test_apply_hydro_is_the_composition_of_the_public_calls(ops, periphery, kind, with_periphery, skip):
    names = ("centred", ) if with_periphery else ("main", "n1025", "poly", "lonely", "n3", "n2")
    for name in names:
        c = case_of(name)
        G = Gpu(ops, c, kind, periphery[0] if with_periphery else None, skip)
        for label, x in _xs(len(c["q"])).items():
            xd = dev(x)
            want_y, want_rows = G.composed(xd)
            y = G.op.apply_hydro(G.mob, xd)
            rows = G.op.body_velocity()
            what = "%s %s x=%s" % (name, kind, label)
            assert_bits_equal(host(y), host(want_y), what + " y")
            assert_bits_equal(host(rows), host(want_rows), what + " rows")
            if label == "one" and name == "lonely":  # every body moves, those without a contact too
                assert (np.abs(host(rows)[:, :3]).max(axis=1) > 0.0).all()
            if label == "zero":
                assert all_pos_zero(host(rows))


def test_no_contact_at_all_gives_zero_rows_and_converges_at_once(ops):
    assert len(case_of("c0")["q"]) == 0
    G = Gpu(ops, case_of("c0"))
    import torch
    e = torch.empty(0, dtype=torch.float64, device="cuda")
    assert tuple(G.op.apply_hydro(G.mob, e).shape) == (0,)
    assert all_pos_zero(host(G.op.body_velocity()))
    s = G.solve()
    assert s["num_iters"] == 0 and s["converged"] and all_pos_zero(s["rows"])
    dry = G.solve(mobility=False)
    assert s["residual"] == dry["residual"]


# ---- 2. against the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iters", (1, 2, 5))
@pytest.mark.parametrize("name", ("main", "n300", "n1025", "n2", "n3", "lonely", "poly"))
def test_first_iterations_are_the_model_bit_for_bit(ops, name, max_iters):
    want = model_solution(name, max_iters=max_iters)
    got = Gpu(ops, case_of(name)).solve(max_iters=max_iters)
    assert_same_solution(got, want, "%s max_iters=%d" % (name, max_iters))


def test_first_iterations_with_the_periphery_are_the_model_bit_for_bit(ops, periphery):
    want = model_solution("centred", max_iters=2, periphery=periphery[1])
    got = Gpu(ops, case_of("centred"), periphery=periphery[0]).solve(max_iters=2)
    assert_same_solution(got, want, "centred with the periphery, max_iters=2")


@pytest.mark.parametrize("name", ("n300", "lonely", "poly", "n3"))
def test_converged_solve_is_the_model_bit_for_bit(ops, name):
    want = model_solution(name)
    assert want["converged"]
    assert_same_solution(Gpu(ops, case_of(name)).solve(), want, "%s at convergence" % name)


def test_main_case_converges_in_the_models_count_to_the_models_bits(ops):
    want = model_solution("main")
    assert want["converged"]
    assert_same_solution(Gpu(ops, case_of("main")).solve(), want, "main at convergence", keys=("x", "g"))


# ---- 3. the dry limit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("main", "n300", "lonely"))
def test_a_vanishing_hydrodynamic_part_gives_the_dry_solve_bit_for_bit(ops, name):
    G = Gpu(ops, case_of(name), viscosity=1e200)
    wet, dry = G.solve(), G.solve(mobility=False)
    assert dry["converged"] and dry["num_iters"] > 10
    assert_same_solution(wet, dry, "%s, viscosity 1e200 against the dry solve" % name, keys=("x", "g"))


# ---- 4. closed forms -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("branch,r,a,bead", (("overlap", 0.9, 0.5, 0.5), ("far", 1.2, 0.5, 0.65)))
def test_one_contact_between_two_equal_beads_has_the_closed_form_multiplier(ops, branch, r, a, bead):
    c = hsm.two_beads(r, a, bead, 0.1)
    G = Gpu(ops, c)
    wet, dry = G.solve(tol=1e-10), G.solve(tol=1e-10, mobility=False)
    want = hsm.closed_form_lambda(r, a, 0.1, c["dt"], c["viscosity"], branch)
    print("%s: lambda %.15g, closed form %.15g, dry %.15g" % (branch, wet["x"][0], want, dry["x"][0]))
    assert wet["converged"] and dry["converged"]
    assert abs(wet["x"][0] - want) <= 1e-12 * want
    assert abs(dry["x"][0] - 0.1 / (2 * c["dt"] * c["mob_trans"][0])) <= 1e-12 * dry["x"][0]
    assert wet["x"][0] > dry["x"][0]
    if branch == "overlap":
        assert abs(want - 139.626) < 1e-3 and abs(dry["x"][0] - 47.124) < 1e-3


# ---- 5. the trap ------------------------------------------------------------------------------------------------------------------------
def test_inactive_contacts_and_lone_beads_feel_forces_far_away_whatever_the_tiering(ops):
    c = case_of("trap")
    G = Gpu(ops, c)
    wet, dry = G.solve(), G.solve(mobility=False)
    assert wet["converged"] and dry["converged"]
    assert wet["x"][0] > 0.0 and wet["x"][1] == 0.0 and dry["x"][1] == 0.0
    assert dry["g"][1] == c["q"][1] and all_pos_zero(dry["rows"][4])
    assert wet["g"][1] != c["q"][1] and wet["g"][1] > 0.0
    assert np.abs(wet["rows"][4, :3]).max() > 0.0
    assert_same_solution(wet, model_solution("trap"), "trap")
    G.op.set_tiering(2)
    assert_same_solution(G.solve(), wet, "trap with the operator's tiering forced to mode 2")
    G.op.set_tiering(0)
    assert_same_solution(G.solve(), wet, "trap with the operator's tiering off")


# ---- 6. at convergence ---------------------------------------------------------------------------------------------------------------------
def test_converged_main_case_satisfies_the_lcp_and_the_headers_bit_relations(ops):
    G = Gpu(ops, case_of("main"))
    s = G.solve()
    assert s["converged"] and 0 < s["num_iters"] < 1000
    assert (s["x"] >= 0.0).all() and (s["x"] > 0.0).any()
    x, g = dev(s["x"]), dev(s["g"])
    assert ops.residual(ops.RESIDUAL_PROJECTED_DIFF, x, g, ops.LCP_SPACE) <= 1e-8
    rows = G.op.body_velocity()
    assert_bits_equal(s["g"], host(G.q + G.c["dt"] * G.op.constraint_rate(rows)), "g = q + dt D^T rows")
    want_y, want_rows = G.composed(x)
    assert_bits_equal(s["rows"], host(want_rows), "rows = M_h D x of the returned x")
    zero_share = float((np.abs(host(G.op.body_force(x, stride=3))).max(axis=1) == 0.0).mean())
    print("main: %d iterations, %.1f %% of the bodies carry no force at the solution" % (s["num_iters"], 100 * zero_share))


# ---- 7. sparse sources ------------------------------------------------------------------------------------------------------------------------
def _force_fields(ns):
    rng = np.random.default_rng(5)
    f = rng.normal(size=(ns, 3))
    one = np.zeros((ns, 3))
    one[700, 1] = -2.0
    last = np.zeros((ns, 3))
    last[1024 + 3:] = f[1024 + 3:]  # every tile of the first chunk is empty, and the start of the last tile
    neg = f.copy()
    neg[rng.random(ns) < 0.5] = -0.0
    seventy = f.copy()
    seventy[rng.random(ns) < 0.7] = 0.0
    return dict(zero=np.zeros((ns, 3)), one=one, last_tile=last, negative_zero=neg, seventy=seventy, dense=f)


@pytest.mark.parametrize("path", ("in_lane", "partial"))
@pytest.mark.parametrize("nt", (1100, 37))
@pytest.mark.parametrize("kind", ("rpyc", "rpy"))
def test_sparse_sources_give_the_bits_of_the_dense_walk(ops, kind, nt, path):
    c = case_of("main")
    ns = c["n"]
    rng = np.random.default_rng(9)
    sc, sa = dev(c["center"]), dev(rng.uniform(0.2, 0.7, ns))
    tc, tb = (sc, sa) if nt == ns else (dev(rng.uniform(0.0, 14.0, (nt, 3))), dev(rng.uniform(0.2, 0.7, nt)))
    ws = ops.HydroWorkspace()
    ws.set_path(path)
    old = dev(rng.normal(size=(nt, 6)))
    for label, f in _force_fields(ns).items():
        fd = dev(f)
        out = {}
        for on in (False, True):
            ws.set_sparse_sources(on)
            fresh = ops.hydro_velocity(kind, 1.0, sc, sa, fd, tc, tb, workspace=ws)
            assert ws.last_path() == path
            acc = ops.hydro_velocity(kind, 1.0, sc, sa, fd, tc, tb, out=old.clone(), accumulate=True, workspace=ws)
            out[on] = (host(fresh), host(acc))
        what = "%s nt=%d %s %s" % (kind, nt, path, label)
        assert_bits_equal(out[True][0], out[False][0], what)
        assert_bits_equal(out[True][1], out[False][1], what + " accumulated")
        if label == "zero":
            assert all_pos_zero(out[True][0])
        else:
            assert np.abs(out[True][0]).max() > 0.0


def test_the_solve_does_not_depend_on_the_workspaces_switch_and_leaves_the_workspace_usable(ops):
    G = Gpu(ops, case_of("n300"))
    off = G.solve()
    G.ws.set_sparse_sources(True)
    on = G.solve()
    assert_same_solution(on, off, "n300 with the workspace's sparse sources on")
    assert_same_solution(off, model_solution("n300"), "n300")
    # the converged solve's stop word does not stay with the workspace: its next call computes
    f = dev(np.random.default_rng(6).normal(size=(G.c["n"], 3)))
    after = ops.hydro_velocity("rpyc", G.mu, G.center, G.a, f, workspace=G.ws)
    fresh = ops.hydro_velocity("rpyc", G.mu, G.center, G.a, f, workspace=ops.HydroWorkspace())
    assert np.abs(host(after)).min() > 0.0
    assert_bits_equal(host(after), host(fresh), "hydro_velocity on the solve's workspace afterwards")


# ---- 8. the stepper -------------------------------------------------------------------------------------------------------------------------------
CFG = dict(max_iters=1000, tol=1e-8)


def _stepper(ops, c, hydro, **kw):
    from mundy_amd import pipeline
    args = dict(dt=c["dt"], viscosity=c["viscosity"], search_buffer=0.3, brownian_kt=0.0, cfg=ops.PGDConfig(**CFG))
    if hydro is not None:
        args["hydrodynamics"] = hydro
    args.update(kw)
    return pipeline.ContactStepper("sphere", dev(c["center"]), dev(c["radius"]), **args)


def _external_force(n):
    return np.random.default_rng(21).normal(size=(n, 3))


@pytest.mark.parametrize("with_periphery", (False, True))
def test_stepper_in_solve_is_the_composed_models_over_three_steps(ops, with_periphery):
    c = case_of("centred")
    n, mu, dt = c["n"], c["viscosity"], c["dt"]
    hydro = dict(kind="rpyc", in_solve=True)
    nodes = None
    if with_periphery:
        pts, w, nrm = pm.sphere_quadrature(PERIPHERY["order"], PERIPHERY["radius"], include_poles=False, invert=True)
        hydro["periphery"] = dict(points=pts, weights=w, normals=nrm)
    st = _stepper(ops, c, hydro, warm_start=True)
    if with_periphery:
        nodes = dict(points=pts, weights=w, normals=nrm, inverse=host(st.hydro_periphery.matrix()), viscosity=mu,
                     skip_same_index=True)
    F = _external_force(n)
    mt = host(st.mob_trans)
    lam_prev, warm = None, 0
    for step in range(3):
        x0 = host(st.center).copy()
        stats = st.step(external_force=dev(F))
        assert stats.converged and stats.num_contacts > 0
        # U_ext = m_t F + hydro(F) (+ the periphery's correction of F), unchanged by in_solve
        u_ext = chm.drag_velocity(mt, F)
        u_ext[:, :3] = u_ext[:, :3] + pm_or_free(nodes, mu, x0, c["radius"], F)
        assert_bits_equal(host(st.u_ext), u_ext, "step %d U_ext" % step)
        # the step's own contact list; q = sep + dt D^T U_ext
        con = dict(n=n, center=x0, radius=c["radius"], hydro_radius=c["radius"], pairs=host(st.contact_pairs),
                   normal=host(st.contacts["normal"]), q=None, dt=dt, viscosity=mu, mob_trans=mt)
        op = hsm.Operator(con, "rpyc", nodes)
        q = 1.0 * host(st.contacts["sep"]) + dt * op.constraint_rate(u_ext)
        assert_bits_equal(host(st.q), q, "step %d q" % step)
        reuse = lam_prev is not None and not stats.rebuilt and len(lam_prev) == len(q)
        warm += int(reuse)
        want = hsm.solve(op, q, lam_prev if reuse else np.zeros(len(q)), **CFG)
        assert want["converged"] and want["num_iters"] == stats.num_iters
        assert_bits_equal(host(st.lam), want["x"], "step %d lambda" % step)
        lam_prev = want["x"]
        U = 1.0 * u_ext + 1.0 * want["rows"]
        assert_bits_equal(host(st.velocity), U, "step %d U" % step)
        assert_bits_equal(host(st.center), x0 + dt * U[:, :3], "step %d positions" % step)
        assert_bits_equal(host(st.body_contact_force())[:, :3], op.body_force(want["x"]), "step %d D lambda" % step)
    assert warm > 0, "no step reused the multipliers: warm_start was not exercised"


def pm_or_free(nodes, mu, x, radius, F):
    u = hm.velocity("rpyc", mu, x, radius, F)
    if nodes is not None:
        u = pm.correct("rpyc", mu, nodes["points"], nodes["weights"], nodes["normals"], nodes["inverse"], x, radius, F,
                       old=u, skip_same_index=True)[0]
    return u


def test_stepper_without_in_solve_is_todays_step_and_a_distant_bead_tells_the_two_apart(ops):
    c = case_of("lonely")   # the second half of the beads touches nothing
    F = dev(_external_force(c["n"]))
    runs = {}
    for label, hydro in (("absent", dict(kind="rpyc")), ("false", dict(kind="rpyc", in_solve=False)),
                         ("true", dict(kind="rpyc", in_solve=True))):
        st = _stepper(ops, c, hydro)
        for _ in range(2):
            stats = st.step(external_force=F)
            assert stats.converged
        runs[label] = (host(st.velocity), host(st.center), host(st.lam), host(st.u_ext))
    for a, b in zip(runs["absent"], runs["false"]):
        assert_bits_equal(a, b, "in_solve=False against the absent key")
    far = c["n"] - 1
    dU = runs["true"][0][far, :3] - runs["absent"][0][far, :3]
    print("the last bead's velocity differs by", dU)
    assert np.abs(dU).max() > 0.0
    # dry, that bead moves with U_ext alone; with the mobility inside the solve it feels the contacts
    assert_bits_equal(runs["absent"][0][far], runs["absent"][3][far], "the dry solve leaves a lone bead at U_ext")


def test_stepper_in_solve_refuses_reorder_bodies(ops):
    st = _stepper(ops, case_of("n300"), dict(kind="rpyc", in_solve=True))
    with pytest.raises(ValueError, match="in_solve"):
        st.reorder_bodies()


# ---- the refusals that need an operator handle --------------------------------------------------------------------------------------------------
def test_library_refuses_operators_mobilities_and_spaces_it_does_not_cover(ops):
    import ctypes as C

    import torch
    from mundy_amd import capi
    c = case_of("n300")
    G = Gpu(ops, c)
    nc = len(c["q"])
    lib = capi.load()
    x = torch.zeros(nc, dtype=torch.float64, device="cuda")
    vec = [torch.zeros_like(x) for _ in range(4)]

    def solve(op, mob, space=ops.LCP_SPACE):
        res, sp, pc = capi.SolveResult(), capi.Space(*space), capi.PgdConfig(10, 1e-8, 0)
        return lib.mhip_bbpgd_solve_contact_hydro(op._h, C.byref(mob), G.q.data_ptr(), C.byref(sp), C.byref(pc),
                                                  *[v.data_ptr() for v in vec], C.byref(res), None)

    def apply(op, mob):
        return lib.mhip_contact_op_apply_hydro(op._h, C.byref(mob), x.data_ptr(), vec[0].data_ptr(), None)

    def mob(**kw):
        m = capi.HydroMobility(G.ws._h, capi.HYDRO_RPYC, 1.0, c["n"], G.center.data_ptr(), G.a.data_ptr(), None, 1)
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    arms = dev(np.zeros((nc, 3)))
    rigid = ops.ContactOperator(dev(c["pairs"]), dev(c["normal"]), dev(c["mob_trans"]), c["dt"], ra=arms, rb=arms,
                                mob_rot=dev(c["mob_trans"]))
    for call in (solve, apply):
        for op, m, match in ((rigid, mob(), "sphere operator"), (G.op, mob(n=c["n"] - 1), "bodies"),
                             (G.op, mob(kind=capi.HYDRO_STOKES), "Stokeslet"), (G.op, mob(kind=7), "unknown"),
                             (G.op, mob(viscosity=0.0), "viscosity"), (G.op, mob(viscosity=float("inf")), "viscosity"),
                             (G.op, mob(workspace=None), "hydro handle is null"), (G.op, mob(center=None), "center")):
            with pytest.raises(ValueError, match=match):
                capi.check(call(op, m))
    for space in ((ops.SPACE_UNCONSTRAINED, 0.0, 0.0), (ops.SPACE_LOWER_BOUND, 0.5, 0.0), (ops.SPACE_BOUNDED, 0.0, 1.0)):
        with pytest.raises(ValueError, match="LowerBound"):
            capi.check(solve(G.op, mob(), space))
    # a periphery without its inverse
    pts, w, nrm = pm.sphere_quadrature(2, 12.0, include_poles=False, invert=True)
    P = ops.HydroPeriphery(dev(pts), dev(w), dev(nrm), 1.0)
    with pytest.raises(AssertionError, match="inverse"):
        capi.check(apply(G.op, mob(periphery=P._h)))
    # nothing was written by a refused call
    assert all_pos_zero(host(vec[0]))
    # a staged solve in progress, then a partitioned operator (an operator of its own: the partition stays with it).
    # The vectors hold a pattern and the rows those of an accepted call: a refused call leaves both as they are.
    other = ops.ContactOperator(dev(c["pairs"]), dev(c["normal"]), dev(c["mob_trans"]), c["dt"])
    xr = dev(np.random.default_rng(4).uniform(0.0, 1.0, nc))
    capi.check(lib.mhip_contact_op_apply_hydro(other._h, C.byref(mob()), xr.data_ptr(), vec[0].data_ptr(), None))
    rows = host(other.body_velocity())
    assert np.abs(rows[:, :3]).min() > 0.0
    pattern = [np.full(nc, 1.25 + k) for k in range(4)]

    def refused(kind, match):
        for v, p in zip(vec, pattern):
            v.copy_(dev(p))
        for call in (solve, apply):
            with pytest.raises(kind, match=match):
                capi.check(call(other, mob()))
            for v, p in zip(vec, pattern):
                assert_bits_equal(host(v), p, "a vector after the refused call (%s)" % match)
            assert_bits_equal(host(other.body_velocity()), rows, "the rows after the refused call (%s)" % match)

    res, sp, pc = capi.SolveResult(), capi.Space(*ops.LCP_SPACE), capi.PgdConfig(10, 1e-8, 0)
    work = [torch.zeros_like(x) for _ in range(4)]
    capi.check(lib.mhip_bbpgd_stage_begin(other._h, G.q.data_ptr(), C.byref(sp), C.byref(pc),
                                          *[v.data_ptr() for v in work], None))
    refused(RuntimeError, "staged solve is in progress")          # MHIP_ERR_RUNTIME
    capi.check(lib.mhip_bbpgd_stage_end(other._h, C.byref(res), None))
    capi.check(apply(other, mob()))   # (accepted again once the staged solve has ended; x = 0: +0.0 rows)
    rows = host(other.body_velocity())
    capi.check(lib.mhip_contact_op_set_partition(other._h, 0, c["n"] - 7, None, None))
    refused(AssertionError, "partitioned operator")                # MHIP_ERR_LOGIC: a sub-range of the bodies
    counted = torch.ones(nc, dtype=torch.uint8, device="cuda")
    capi.check(lib.mhip_contact_op_set_partition(other._h, 0, c["n"], counted.data_ptr(), None))
    refused(AssertionError, "partitioned operator")                # every body, but a `counted` array
    capi.check(lib.mhip_contact_op_set_partition(other._h, 0, c["n"], None, None))
    capi.check(apply(other, mob()))   # (the whole operator again)


ORDERS = (("", 0, "needs MHIP_HYDRO_RPYC or MHIP_HYDRO_RPY"), ("solve_first", 2, "needs set_hydrodynamics first"),
          ("after_hertz", 2, "needs the LCP contact model"), ("hertz_later", 2, "no Hertz contact with it"),
          ("no_spheres", 2, "needs the sphere contacts"), ("stokes_later", 2, "needs MHIP_HYDRO_RPYC or MHIP_HYDRO_RPY"))


def test_cpp_stepper_refuses_what_the_python_stepper_refuses():
    import os
    import subprocess
    import tempfile

    from cpp_apps import build_app
    from mundy_amd import synth
    d = _chains()
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    exe = build_app("hydro_solve_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([d["center"].shape[0], d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            for a in (d["center"], d["radius"], mt):
                a.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            np.array([0, 1], dtype=np.uint64).tofile(f)

        def run(kind, in_solve, order):
            args = [exe, path, "1", repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]), repr(d["kt"]),
                    repr(d["viscosity"]), str(kind), "1", str(in_solve), "10000", "1e-5"] + ([order] if order else [])
            return subprocess.run(args, capture_output=True, text=True, timeout=600)
        for order, kind, match in ORDERS:
            out = run(kind, 1, order)
            assert out.returncode == 2 and "STEP" not in out.stdout, (order, out.returncode, out.stderr)
            assert out.stderr.startswith("REFUSED SphereChainStepper:") and match in out.stderr, (order, out.stderr)
        # the same sequences without the hydrodynamic solve are the stepper's ordinary configurations
        for order in ("hertz_later", "stokes_later"):
            out = run(2, 0, order)
            assert out.returncode == 0 and "STEP 0" in out.stdout, (order, out.stderr)


# ---- the C++ driver ---------------------------------------------------------------------------------------------------------------------------------
def _chains(seed=8, jitter=0.05):
    from mundy_amd import synth
    d = synth.chains(4, 50, seed=seed, cell=2.4)
    d["center"] = d["center"] - np.array([2.4, 2.4, 1.2])  # inside the sphere of radius 5
    d["center"] = d["center"] + jitter * np.random.default_rng(seed).normal(size=d["center"].shape)
    assert np.linalg.norm(d["center"], axis=1).max() < 5.0 - 0.5
    return d


@pytest.mark.parametrize("confined", (False, True))
def test_hydro_solve_step_app_matches_python(ops, confined):
    import os
    import subprocess
    import tempfile

    from cpp_apps import build_app, fnv1a
    from mundy_amd import capi, pipeline, synth
    d = _chains()
    n = d["center"].shape[0]
    mt, _ = synth.dry_mobility(d["radius"], viscosity=d["viscosity"])
    pts, w, nrm = pm.sphere_quadrature(4, 5.0, include_poles=False, invert=True)
    steps, cfg = 8, dict(max_iters=10000, tol=1e-5)
    runs = {}
    for in_solve in (True, False):
        hydro = dict(kind="rpyc", update_every=2, in_solve=in_solve)
        if confined:
            hydro["periphery"] = dict(points=pts, weights=w, normals=nrm)
        st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                     search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                     brownian_kt=d["kt"], cfg=ops.PGDConfig(**cfg), hydrodynamics=hydro)
        lines, contacts = [], 0
        for k in range(steps):
            s = st.step()
            assert s.converged
            contacts += s.num_contacts
            lines.append("STEP %d contacts %d iterations %d max_spring_length %.17g" % (k, s.num_contacts, s.num_iters,
                                                                                         s.max_spring_length))
        assert contacts > 0
        runs[in_solve] = (lines, fnv1a(host(st.center).reshape(-1).view(np.uint64).tolist()),
                          fnv1a(host(st.lam).reshape(-1).view(np.uint64).tolist()))
    assert runs[True][1] != runs[False][1], "the hydrodynamic solve moved the beads as the dry one does"
    exe = build_app("hydro_solve_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([n, d["pairs"].shape[0]], dtype=np.uint64).tofile(f)
            d["center"].astype(np.float64).tofile(f)
            d["radius"].astype(np.float64).tofile(f)
            mt.astype(np.float64).tofile(f)
            d["pairs"].astype(np.int32).tofile(f)
            np.array([pts.shape[0] if confined else 0, 1], dtype=np.uint64).tofile(f)
            if confined:
                for a in (pts, w, nrm):
                    a.astype(np.float64).tofile(f)
        for in_solve in (True, False):
            out = subprocess.run([exe, path, str(steps), repr(d["dt"]), repr(d["skin"]), repr(d["k"]), repr(d["r0"]),
                                  repr(d["kt"]), repr(d["viscosity"]), str(capi.HYDRO_RPYC), "2", "1" if in_solve else "0",
                                  str(cfg["max_iters"]), repr(cfg["tol"])], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0, out.stderr
            got = [ln for ln in out.stdout.splitlines() if ln.startswith("STEP")]
            lines, center, lam = runs[in_solve]
            assert [" ".join(g.split()[:8]) for g in got] == lines
            cs = [ln for ln in out.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
            assert cs[2] == center and cs[4] == lam, "in_solve=%s" % in_solve
