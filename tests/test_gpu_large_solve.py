"""GPU parity past the size gates of the contact solve, bit for bit against the oracle at K iterations.

Several paths of convex.hip switch on only above a size: the one-launch fold + finalize with its ticket hand-off (more
than MHIP_FOLD_ABOVE = 4096 constraint tiles, C > 1 048 576), the fold + 1024-thread final pass of the init iteration,
the staged reduce and the cone-BBPGD / APGD / unfused drivers (same threshold), the grid-stride constraint sweep (more
than kMaxConstraintGrid = 32768 tiles, C > 8 388 608), the cold tier on by default (C >= 1.5e6) and the drift source
chosen by size (more than 1.75e6 bodies).  A solve to convergence at these sizes is too slow for the serial oracle, so
every case runs K iterations on both sides -- the device and oracle.solve_cqpp_contact (or the scrap / friction
statement) in compensated mode, which defines every sum as the device does -- and requires the final x, g, the previous
iterate (x_tmp, g_tmp), the iteration count and the residual to be the same bits.  Each case also asserts that its gate
fired.  Problems are built with the oracle's broad phase and contact kernels, so nothing here depends on the device's.
(`apply` itself, and with it the unfused driver, launches at most kMaxGrid = 2048 workgroups: its constraint sweep goes
grid-stride from 524 288 contacts on, so the fold-size unfused case covers that loop too.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FOLD_TILES = 4096          # MHIP_FOLD_ABOVE (convex.hip)
GRID_CAP_TILES = 32768     # kMaxConstraintGrid (convex.hip)
TILE = 256                 # constraints per tile (kBlock)
TIER_MIN_CONTACTS = 1_500_000    # kTierMinContacts (convex.hip)
ROW_DRIFT_MAX_BODIES = 1_750_000  # kRowDriftMaxBodies (convex.hip)
DT = 5e-3

K_FOLD = 30      # spheres past the fold gate (fused, unfused, staged)
K_TIER = 80      # rods in the default tier: polls at 8, 24, 56 iterations; the tiers must have been built by 80
K_RIGID = 20     # the same rods with vector arms
K_GRID = 4       # spheres past the grid-stride gate
K_OTHER = 12     # scrap BB1/BB2, cone-BBPGD, APGD


@pytest.fixture(scope="module")
def ops():
    import torch
    assert torch.cuda.is_available()
    from mundy_amd import ops as o
    return o


def _spheres(oracle, n, phi=0.4, buffer=0.25):
    from mundy_amd import synth
    s = synth.spheres(n, volume_fraction=phi)
    c, r = s["center"], s["radius"]
    lo, hi, R = oracle.grow(oracle.compute_aabb_spheres(c, r), r, buffer)
    pairs = oracle.search(oracle.SEARCH_SPHERES, lo, hi, c, R)
    sep, nrm = oracle.contact_spheres(pairs, c, r)
    mt, mr = synth.dry_mobility(r)
    return dict(N=n, pairs=pairs, sep=sep, normal=nrm, mt=mt, mr=mr, radius=r)


def _rods(oracle, n, buffer=0.1):
    from mundy_amd import synth
    b = synth.spherocylinders(n)
    c = b["center"]
    aabb = oracle.compute_aabb_spherocylinders(c, b["quat"], b["radius"], b["length"])
    brad = oracle.bounding_radius_spherocylinders(b["radius"], b["length"])
    lo, hi, R = oracle.grow(aabb, brad, buffer)
    pairs = oracle.search(oracle.SEARCH_AABB, lo, hi, c, R)
    seg = oracle.spherocylinder_segments(c, b["quat"], b["radius"], b["length"])
    out = oracle.contact_spherocylinders(pairs, seg, c)
    mt, mr = synth.dry_mobility(b["radius"], bounding_radius=brad)
    return dict(N=n, pairs=pairs, sep=out["sep"], normal=out["normal"], ra=out["ra"], rb=out["rb"], s=out["s"],
                t=out["t"], seg=seg, mt=mt, mr=mr)


@pytest.fixture(scope="module")
def fold_spheres(oracle):
    P = _spheres(oracle, 360_000)
    C = len(P["pairs"])
    assert FOLD_TILES * TILE < C < TIER_MIN_CONTACTS, C     # past the fold gate, below the default tier
    with oracle.compensated_sums():
        P["oracle"] = oracle.solve_cqpp_contact(P["pairs"], P["normal"], None, None, P["mt"], None, DT, P["sep"],
                                                np.zeros(C), max_iters=K_FOLD, tol=1e-12, threads=False,
                                                previous=True)
    return P


@pytest.fixture(scope="module")
def tier_rods(oracle):
    P = _rods(oracle, 210_000)
    C = len(P["pairs"])
    assert TIER_MIN_CONTACTS <= C < GRID_CAP_TILES * TILE and P["N"] <= ROW_DRIFT_MAX_BODIES, C
    return P


@pytest.fixture(scope="module")
def grid_spheres(oracle):
    P = _spheres(oracle, 2_800_000)
    assert len(P["pairs"]) > GRID_CAP_TILES * TILE and P["N"] > ROW_DRIFT_MAX_BODIES, len(P["pairs"])
    return P


def _state(C):
    from gpu_util import dev
    return tuple(dev(np.zeros(C)) for _ in range(4))


def _assert_same_solve(st, res, ref, what):
    """st = device (x, g, x_tmp, g_tmp), res its SolveResult; ref = the oracle's (x, g, result, (x_tmp, g_tmp))"""
    from gpu_util import assert_bits_equal, host
    xo, go, ro, (xto, gto) = ref
    assert (res.num_iters, res.converged) == (ro["num_iters"], ro["converged"]), (what, res, ro)
    assert res.residual == ro["residual"], (what, res.residual, ro["residual"])
    assert_bits_equal(host(st[0]), xo, what + ": x")
    assert_bits_equal(host(st[1]), go, what + ": g")
    assert_bits_equal(host(st[2]), xto, what + ": x_tmp (previous iterate)")
    assert_bits_equal(host(st[3]), gto, what + ": g_tmp")


def _sphere_op(ops, P, arms=False):
    from gpu_util import dev
    if not arms:
        return ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT)
    return ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT, ra=dev(P["ras"]), rb=dev(P["rbs"]),
                               mob_rot=dev(P["mr"]))


# ---- fold + finalize (more than 4096 tiles) ----------------------------------------------------------------------------
def test_fold_finalize_spheres_fused_and_unfused(ops, oracle, fold_spheres):
    # fused: k_fold_finalize<X_SOLVE> every iteration, fold_partials + k_finalize (1024 threads) at the init iteration;
    # unfused: the separate apply / reductions of the driver, the same sums
    from gpu_util import dev
    P = fold_spheres
    C = len(P["pairs"])
    q = dev(P["sep"])
    for fused in (True, False):
        op = _sphere_op(ops, P)
        op.set_tiering(0)
        st = _state(C)
        _, _, res = ops.solve_lcp(op, q, None, ops.PGDConfig(max_iters=K_FOLD, tol=1e-12), state=st, fused=fused)
        assert op.tier_stats()["tiered_iterations"] == 0
        _assert_same_solve(st, res, P["oracle"], "fused" if fused else "unfused")
        assert res.num_iters == K_FOLD
        op.close()


def _staged_solve(ops, op, q, cfg, split=None):
    """the staged entry points on one rank: the whole-range wrapper, or (split = c1) the constraint stage as two range
    sweeps [0, c1) and [c1, C) and one reduce, as the distributed driver calls them"""
    import ctypes as C
    import torch
    from mundy_amd import capi
    lib = capi.load()
    nc = op.num_constraints
    x, g, xt, gt = (torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(4))
    local = torch.empty(5, dtype=torch.float64, device="cuda")  # MHIP_BBPGD_REDUCTION_WIDTH
    sp = capi.Space(ops.SPACE_LOWER_BOUND, 0.0, 0.0)
    pc = capi.PgdConfig(cfg.max_iters, cfg.tol, cfg.residual_kind)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    capi.check(lib.mhip_bbpgd_stage_begin(op._h, p(q), C.byref(sp), C.byref(pc), p(x), p(g), p(xt), p(gt), None))
    res, done = capi.SolveResult(), C.c_int(0)
    for it in range(cfg.max_iters + 1):
        init = 1 if it == 0 else 0
        capi.check(lib.mhip_bbpgd_stage_body(op._h, init, None))
        if split is None:
            capi.check(lib.mhip_bbpgd_stage_constraint(op._h, init, p(local), None))
        else:
            capi.check(lib.mhip_bbpgd_stage_constraint_range(op._h, init, 0, split, None))
            capi.check(lib.mhip_bbpgd_stage_constraint_range(op._h, init, split, nc - split, None))
            capi.check(lib.mhip_bbpgd_stage_reduce(op._h, init, p(local), None))
        capi.check(lib.mhip_bbpgd_stage_finalize(op._h, init, p(local), 1, None))   # one rank: its own record
        capi.check(lib.mhip_bbpgd_stage_poll(op._h, C.byref(res), C.byref(done), None))
        if done.value:
            break
    capi.check(lib.mhip_bbpgd_stage_end(op._h, C.byref(res), None))
    return (x, g, xt, gt), res


@pytest.mark.parametrize("split", [None, "halves"])
def test_fold_staged_driver_equals_fused_solve(ops, oracle, fold_spheres, split):
    # the staged reduce past 4096 partials (fold_partials + k_reduce_local at 1024 threads), the finalize of the one
    # gathered record; once through mhip_bbpgd_stage_constraint, once as two ranges + mhip_bbpgd_stage_reduce (each range
    # below the fold gate on its own, together above it)
    import torch
    from gpu_util import dev
    P = fold_spheres
    C = len(P["pairs"])
    cfg = ops.PGDConfig(max_iters=K_FOLD, tol=1e-12)
    q = dev(P["sep"])
    op = _sphere_op(ops, P)
    c1 = None if split is None else (C // 2 // TILE) * TILE + 77    # (a boundary inside a tile)
    if c1 is not None:
        assert -(-c1 // TILE) <= FOLD_TILES and -(-(C - c1) // TILE) <= FOLD_TILES
        assert -(-c1 // TILE) + -(-(C - c1) // TILE) > FOLD_TILES
    st, res = _staged_solve(ops, op, q, cfg, split=c1)
    assert (res.num_iters, bool(res.converged)) == (K_FOLD, False)
    ref = _state(C)
    op_f = _sphere_op(ops, P)
    _, _, rf = ops.solve_lcp(op_f, q, None, cfg, state=ref)
    assert res.residual == rf.residual
    for a, b in zip(st, ref):
        assert torch.equal(a, b)
    _assert_same_solve(st, rf, P["oracle"], "staged" + ("" if c1 is None else " in two ranges"))
    op.close()
    op_f.close()


# ---- the other drivers on the partials machinery ---------------------------------------------------------------------
def test_fold_scrap_variant(ops, oracle, fold_spheres):
    from gpu_util import assert_bits_equal, dev, host
    P = fold_spheres
    C = len(P["pairs"])
    op = _sphere_op(ops, P)
    lam, g, res = ops.resolve_collisions(op, dev(P["sep"]), dev(np.zeros(C)), DT, max_allowable_overlap=1e-12,
                                         max_col_iterations=K_OTHER)
    with oracle.compensated_sums():
        lo, go, ro = oracle.scrap_resolve_collisions(P["pairs"], P["normal"], None, None, P["mt"], None, DT, P["sep"],
                                                     np.zeros(C), max_allowable_overlap=1e-12, max_iters=K_OTHER)
    assert res.ite_count == ro["ite_count"] == K_OTHER
    assert res.max_abs_projected_sep == ro["max_abs_projected_sep"]
    assert res.max_displacement == ro["max_speed"] * DT
    assert_bits_equal(host(lam), lo, "scrap lambda")
    assert_bits_equal(host(g), go, "scrap g")
    op.close()


@pytest.mark.parametrize("method", ["bbpgd", "apgd"])
def test_fold_friction_drivers(ops, oracle, fold_spheres, method):
    # cone-BBPGD and APGD (their partial records go through fold_partials + k_finalize every iteration) on the vector-arm
    # operator with lever arms to the surface contact points, mu = 0.3
    from gpu_util import assert_bits_equal, dev, host
    P = dict(fold_spheres)
    pr, r = P["pairs"], P["radius"]
    # ops.surface_lever_arms with zero centreline arms: ra + r_i n, rb - r_j n
    P["ras"] = np.zeros((len(pr), 3)) + r[pr[:, 0]][:, None] * P["normal"]
    P["rbs"] = np.zeros((len(pr), 3)) - r[pr[:, 1]][:, None] * P["normal"]
    op = _sphere_op(ops, P, arms=True)
    mu = 0.3
    p, g, res = ops.solve_friction_contact(op, dev(P["sep"]), mu, cfg=ops.PGDConfig(max_iters=K_OTHER, tol=1e-12),
                                           method=method)
    with oracle.compensated_sums():
        po, go, ro = oracle.solve_friction_contact(pr, P["normal"], P["ras"], P["rbs"], P["mt"], P["mr"], DT, P["sep"],
                                                   mu, max_iters=K_OTHER, tol=1e-12, method=method)
    assert (res.num_iters, res.converged) == (ro["num_iters"], ro["converged"]) == (K_OTHER, False)
    assert res.residual == ro["residual"]
    assert_bits_equal(host(p), po, method + " impulses")
    assert_bits_equal(host(g), go, method + " g")
    op.close()


# ---- the cold tier on by default (C >= 1.5e6), both drift sources ----------------------------------------------------
def test_default_tier_rods_both_drift_sources(ops, oracle, tier_rods):
    from gpu_util import dev
    P = tier_rods
    C = len(P["pairs"])
    rod = (P["s"], P["t"], P["seg"])
    with oracle.compensated_sums():
        ref = oracle.solve_cqpp_contact(P["pairs"], P["normal"], None, None, P["mt"], P["mr"], DT, P["sep"],
                                        np.zeros(C), max_iters=K_TIER, tol=1e-12, threads=False, rod=rod, previous=True)
    q = dev(P["sep"])
    for source in (1, 2):
        op = ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT, mob_rot=dev(P["mr"]),
                                 rod=tuple(dev(a) for a in rod))
        assert op.drift_source() == 1          # by size: the row form up to 1.75e6 bodies
        op.set_drift_source(source)            # (tiering left at its default)
        assert op.drift_source() == source
        st = _state(C)
        _, _, res = ops.solve_lcp(op, q, None, ops.PGDConfig(max_iters=K_TIER, tol=1e-12), state=st)
        stats = op.tier_stats()
        print("rods, drift source %d: %s" % (source, stats))
        assert stats["renumberings"] >= 1 and stats["tiered_iterations"] > 0, stats
        _assert_same_solve(st, res, ref, "tiered rods, drift source %d" % source)
        op.close()


def test_default_size_vector_arm_rods(ops, oracle, tier_rods):
    # the KIN_RIGID sweeps (ra, rb, mob_rot) at the same size, fold + finalize every iteration
    from gpu_util import dev
    P = tier_rods
    C = len(P["pairs"])
    with oracle.compensated_sums():
        ref = oracle.solve_cqpp_contact(P["pairs"], P["normal"], P["ra"], P["rb"], P["mt"], P["mr"], DT, P["sep"],
                                        np.zeros(C), max_iters=K_RIGID, tol=1e-12, threads=False, previous=True)
    op = ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), DT, ra=dev(P["ra"]), rb=dev(P["rb"]),
                             mob_rot=dev(P["mr"]))
    st = _state(C)
    _, _, res = ops.solve_lcp(op, dev(P["sep"]), None, ops.PGDConfig(max_iters=K_RIGID, tol=1e-12), state=st)
    _assert_same_solve(st, res, ref, "vector-arm rods")
    op.close()


# ---- the grid-stride constraint sweep (more than 32768 tiles) --------------------------------------------------------
def test_grid_stride_sweep_apply_identity_and_solve(ops, oracle, grid_spheres):
    from gpu_util import assert_bits_equal, dev, host
    P = grid_spheres
    C = len(P["pairs"])
    op = _sphere_op(ops, P)
    assert op.drift_source() == 2              # by size: more than 1.75e6 bodies take the register form
    x = np.random.default_rng(3).uniform(0.0, 1.0, C)
    x[::7] = 0.0                               # (inactive contacts: exact zeros the body sweep skips)
    dx = dev(x)
    y = op.apply(dx)
    with oracle.compensated_sums():
        yo = oracle.contact_op_apply(P["pairs"], P["normal"], None, None, P["mt"], None, DT, x, P["N"])
    assert_bits_equal(host(y), yo, "A x past the grid cap")
    assert_bits_equal(host(DT * op.constraint_rate(op.body_velocity_of(dx))), host(y), "dt D^T M D x")
    with oracle.compensated_sums():
        ref = oracle.solve_cqpp_contact(P["pairs"], P["normal"], None, None, P["mt"], None, DT, P["sep"], np.zeros(C),
                                        max_iters=K_GRID, tol=1e-12, threads=False, previous=True)
    st = _state(C)
    _, _, res = ops.solve_lcp(op, dev(P["sep"]), None, ops.PGDConfig(max_iters=K_GRID, tol=1e-12), state=st)
    _assert_same_solve(st, res, ref, "fused solve past the grid cap")
    op.close()
