"""GPU parity at the benchmark's size, stage by stage, bit for bit against the exact oracle.

bench.py times 10^6 spherocylinders (BASELINE configs[2]) and, with --mixed, 10^6 spheres / rods / ellipsoids
(configs[4]).  Several gates of the device path are crossed only there or only along the stepper's own path: the cell
capacity max(n, 4096) of the grid, the two-level LBVH refit (more than 4096 leaves) and its single-workgroup top pass,
rows longer than kShortSegment = 32 (workgroup radix sort), the Morton reorder at 10^6 bodies, the incidence build on
the stepper's 7.6 * 10^6-contact list, the cold tier and the row drift source that are on by default at this size,
and integrate_euler over 10^6 rows.  Here the stepper runs the benchmark's set-up one stage at a time, and every stage
is compared with the oracle (liboracle.so, never the fast build) in the ORIGINAL body numbering: the stepper's
permutation is undone as bench.py's dump_outputs undoes it, and pair lists are put in a canonical order.  The
contact operator and the BBPGD iterations run through the oracle's body-parallel forms (parallel=True), whose bits are
those of the serial forms (tests/test_oracle_parallel_rod.py).

A third case, size-disperse spheres, takes the LBVH through AUTO with hub rows of hundreds of partners.  Every case
asserts that its gates fired, so a change to a generator cannot make a test vacuous; each prints its gate evidence and
the oracle and device time of every stage (pytest -s)."""
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 1_000_000
DT = 5e-3
BUFFER = 0.1                  # bench.py --buffer
CELL = 3.0                    # bench.py --reorder-cell
MIXED_PHI = 0.40              # bench.py MIXED_PHI_DEFAULT
ROD_CONTACTS = 7_621_833      # the headline's contact count
K_ROD = 72                    # the rods' solve: past the first renumbering of the cold tier (polls at 8, 24, 56)
K_MIXED = 6                   # the mixed solve (vector arms)
SHORT_SEGMENT = 32            # kShortSegment (mhip_internal.hpp): longer rows take the workgroup radix sort
REFIT_CHUNK = 4096            # broadphase.hip: a tree of more leaves is refit in two chunked passes, then the top
TIER_MIN_CONTACTS = 1_500_000  # kTierMinContacts (convex.hip): the cold tier is on by default from here
POLY_N = 500_000              # size-disperse spheres (the oracle's cell search takes seconds here, minutes at sigma 0.8)
POLY_SIGMA = 0.5
EE_SAMPLE = 10_000            # ellipsoid-ellipsoid contacts checked (the oracle's L-BFGS is too slow for all of them)


@pytest.fixture(scope="module")
def ops():
    import torch
    assert torch.cuda.is_available()
    from mundy_amd import ops as o
    return o


class _Clock:
    """oracle and device seconds per stage, printed with the gate evidence at the end of a fixture"""

    def __init__(self, case):
        self.case, self.rows, self.notes = case, {}, []

    def _run(self, stage, col, fn, sync):
        import torch
        if sync:
            torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        if sync:
            torch.cuda.synchronize()
        self.rows.setdefault(stage, [0.0, 0.0])[col] += time.perf_counter() - t
        return out

    def oracle(self, stage, fn):
        return self._run(stage, 0, fn, False)

    def device(self, stage, fn):
        return self._run(stage, 1, fn, True)

    def note(self, text):
        self.notes.append(text)

    def report(self):
        print("\n[%s]" % self.case)
        for text in self.notes:
            print("  gate: " + text)
        for stage, (o, d) in self.rows.items():
            print("  %-28s oracle %7.2f s   device %7.3f s" % (stage, o, d))
        print("  %-28s oracle %7.2f s   device %7.3f s" % ("total", sum(r[0] for r in self.rows.values()),
                                                            sum(r[1] for r in self.rows.values())))


def _bits(a, b, what):
    from gpu_util import assert_bits_equal
    assert_bits_equal(a, b, what)


def _original(pairs, perm):
    """a device list in the stepper's numbering -> the same rows, same orientation and order, in the original numbering"""
    return np.ascontiguousarray(perm[pairs.astype(np.int64)].astype(np.int32))


def _unique_keys(pairs, n):
    """canonical order of an unordered pair list: (lower, higher) as one int64 key, ascending"""
    p = pairs.astype(np.int64)
    return np.sort(np.minimum(p[:, 0], p[:, 1]) * n + np.maximum(p[:, 0], p[:, 1]))


def _ordered_keys(pairs, n):
    p = pairs.astype(np.int64)
    return np.sort(p[:, 0] * n + p[:, 1])


def _assert_same_list(got, exp_unique, n, what, symmetric=False):
    """got: a device list in the original numbering; exp_unique: the oracle's unique list (i < j, sorted).  Equal as
    sets -- nothing missing, nothing extra -- and, for a unique list, every pair once.  A symmetric list must hold both
    orientations of every oracle pair."""
    e = exp_unique.astype(np.int64)
    if symmetric:
        exp = np.sort(np.concatenate([e[:, 0] * n + e[:, 1], e[:, 1] * n + e[:, 0]]))
        key = _ordered_keys(got, n)
    else:
        exp = e[:, 0] * n + e[:, 1]
        assert np.all(exp[1:] > exp[:-1]) and np.all(e[:, 0] < e[:, 1])
        key = _unique_keys(got, n)
    if len(key) == len(exp) and np.array_equal(key, exp):
        return
    missing = np.setdiff1d(exp, key, assume_unique=True).size
    extra = len(key) - len(exp) + missing
    raise AssertionError("%s: %d pairs on the device, %d in the oracle: %d missing, %d extra" % (
        what, len(key), len(exp), missing, extra))


def _morton_perm(c, n):
    """the Z-order permutation of mhip_morton_order as tests/test_gpu_reorder_integrate.py states it: lattice cells of
    edge CELL from the origin, z-most-significant bit interleave, ties by index"""
    bits = 4
    while bits < 8 and (1 << (3 * (bits + 1))) <= 8 * n:
        bits += 1
    cells = np.clip(np.floor(c * (1.0 / CELL)).astype(np.int64), 0, (1 << bits) - 1)
    key = np.zeros(n, dtype=np.int64)
    for bit in range(bits):
        for axis in range(3):
            key |= ((cells[:, axis] >> bit) & 1) << (3 * bit + axis)
    return np.argsort(key, kind="stable"), cells, bits


def _state(C):
    import torch
    return tuple(torch.zeros(C, dtype=torch.float64, device="cuda") for _ in range(4))


def _assert_same_solve(dev_out, ref, what):
    """dev_out = (x, g, SolveResult) of the stepper's solve + (x, g, x_tmp, g_tmp) of the same solve with caller-owned
    state; ref = the oracle's (x, g, result, (x_tmp, g_tmp))"""
    (x, g, res, state) = dev_out
    xo, go, ro, (xto, gto) = ref
    assert (res.num_iters, res.converged) == (ro["num_iters"], ro["converged"]), (what, res, ro)
    assert res.residual == ro["residual"], (what, res.residual, ro["residual"])
    _bits(x, xo, what + ": x")
    _bits(g, go, what + ": g")
    _bits(state[0], xo, what + ": x (caller-owned state)")
    _bits(state[1], go, what + ": g (caller-owned state)")
    _bits(state[2], xto, what + ": x_tmp (previous iterate)")
    _bits(state[3], gto, what + ": g_tmp")


# ---- rods: bench.py's headline, configs[2] ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rods(ops, oracle):
    from gpu_util import dev, host
    from mundy_amd import pipeline, synth
    T = _Clock("10^6 rods, configs[2]")
    b = synth.spherocylinders(N, seed=1234)
    c, q, r, L = b["center"], b["quat"], b["radius"], b["length"]
    box = np.full(3, b["box"])
    st = pipeline.ContactStepper("spherocylinder", dev(c), dev(r), dev(q), dev(L), dt=DT, viscosity=1e-3,
                                 search_buffer=BUFFER, search_kind=ops.SEARCH_AABB,
                                 cfg=ops.PGDConfig(max_iters=K_ROD, tol=1e-12))
    R = dict(b=b)
    perm = T.device("reorder", lambda: st.reorder_bodies(cell_size=CELL, lo=[0.0, 0.0, 0.0]))
    R["perm"] = p = host(perm).astype(np.int64)
    R["perm_o"] = T.oracle("reorder", lambda: _morton_perm(c, N))
    R["reordered"] = {k: host(getattr(st, k)).copy() for k in ("center", "quat", "radius", "length")}

    T.device("aabb", st.compute_aabb)
    R["aabb"], R["brad"] = host(st.aabb), host(st.bounding_radius)
    R["aabb_o"] = T.oracle("aabb", lambda: oracle.compute_aabb_spherocylinders(c, q, r, L))
    R["brad_o"] = oracle.bounding_radius_spherocylinders(r, L)

    T.device("neighbour list", lambda: st.generate_neighbor_links(force=True))
    R["pairs"], R["method"] = host(st.links.pairs), st.links.method_used()
    R["rows"] = int(np.diff(host(st.links.row_ptr)).max())
    lo, hi, reach = oracle.grow(R["aabb_o"], R["brad_o"], BUFFER)
    R["pairs_o"] = T.oracle("neighbour list", lambda: oracle.search(oracle.SEARCH_AABB, lo, hi, c, reach))
    R["pairs_o_periodic"] = T.oracle("periodic list", lambda: oracle.search(oracle.SEARCH_AABB, lo, hi, c, reach,
                                                                           box=box))
    # the same volumes through each structure, unique and symmetric, free and in the periodic box of synth
    R["lists"] = {}
    for name, method, sym, bx in (("grid", ops.SEARCH_METHOD_GRID, False, None),
                                  ("lbvh", ops.SEARCH_METHOD_MORTON_LBVH, False, None),
                                  ("grid symmetric", ops.SEARCH_METHOD_GRID, True, None),
                                  ("lbvh symmetric", ops.SEARCH_METHOD_MORTON_LBVH, True, None),
                                  ("grid periodic", ops.SEARCH_METHOD_GRID, False, box),
                                  ("lbvh periodic", ops.SEARCH_METHOD_MORTON_LBVH, False, box)):
        g = (ops.GenNeighborLinks().set_search_kind(ops.SEARCH_AABB).set_search_buffer(BUFFER)
             .set_search_method(method).set_enforce_source_target_symmetry(sym).set_periodic_box(bx).concretize())
        T.device("periodic list" if bx is not None else "neighbour list",
                 lambda: g.generate(st.aabb, st.center, st.bounding_radius))
        R["lists"][name] = (_original(host(g.pairs), p), g.method_used(), int(np.diff(host(g.row_ptr)).max()), method)
        g.close()

    T.device("contacts", st.compute_contacts)
    R["con"] = {k: host(st.contacts[k]) for k in ("sep", "normal", "s", "t")}
    R["seg"] = host(st.seg)
    po = _original(R["pairs"], p)         # the device's list in the original numbering, its orientation and order
    seg_o = oracle.spherocylinder_segments(c, q, r, L)
    R["seg_o"] = seg_o
    R["con_o"] = con_o = T.oracle("contacts", lambda: oracle.contact_spherocylinders(po, seg_o, c))
    C = len(po)

    # the stepper's own solve: its operator, default tiering, K iterations
    res = T.device("operator + solve", lambda: st.resolve_collisions(True))
    R["lam"], R["grad"], R["res"] = host(st.lam), host(st.grad), res
    R["vel"] = host(st.op.body_velocity())
    R["tier"], R["drift"] = st.op.tier_stats(), st.op.drift_source()
    R["mob"] = host(st.mob_trans), host(st.mob_rot)
    T.device("integrate", st.integrate)
    R["center1"], R["quat1"] = host(st.center), host(st.quat)
    # the same solve again on the stepper's operator, with the state owned here: the previous iterate
    state = _state(C)
    _, _, res2 = ops.solve_lcp(st.op, st.contacts["sep"], None, st.cfg, state=state)
    R["res2"], R["state"] = res2, [host(a) for a in state]
    # apply of a seeded non-negative x, and the body rows it leaves
    x = np.random.default_rng(2024).random(C)
    x[::5] = 0.0
    R["x"] = x
    R["y"] = T.device("apply", lambda: host(st.op.apply(dev(x))))
    R["xvel"] = host(st.op.body_velocity_of(dev(x)))

    mt, mr = synth.dry_mobility(r, bounding_radius=R["brad_o"])
    R["mob_o"] = mt, mr
    rod = (con_o["s"], con_o["t"], seg_o)
    with oracle.compensated_sums():
        R["y_o"], R["xvel_o"] = T.oracle("apply", lambda: oracle.contact_op_apply(
            po, con_o["normal"], None, None, mt, mr, DT, x, N, rod=rod, body_velocity=True, parallel=True))
        R["solve_o"] = T.oracle("operator + solve", lambda: oracle.solve_cqpp_contact(
            po, con_o["normal"], None, None, mt, mr, DT, con_o["sep"], np.zeros(C), max_iters=K_ROD, tol=1e-12,
            rod=rod, previous=True, parallel=True))
        R["vel_o"] = T.oracle("integrate", lambda: oracle.contact_op_apply(
            po, con_o["normal"], None, None, mt, mr, DT, R["lam"], N, rod=rod, body_velocity=True, parallel=True)[1])
    vel = np.empty_like(R["vel"])
    vel[p] = R["vel"]                      # the device's velocity rows, original numbering
    with oracle.shared_trig():             # rotate_quaternion with the device's sin / cos
        R["center1_o"], R["quat1_o"] = T.oracle("integrate", lambda: oracle.integrate_euler(DT, vel, c, q))

    T.note("contacts %d; stepper's list: method %d, longest row %d" % (C, R["method"], R["rows"]))
    for name, (_, used, rows, _) in R["lists"].items():
        T.note("%s: method %d, longest row %d" % (name, used, rows))
    T.note("solve: %d iterations, tier %s, drift source %d" % (res.num_iters, R["tier"], R["drift"]))
    T.report()
    yield R
    st.op.close()
    st.links.close()


def test_rods_reorder_is_the_z_order(rods):
    expected, cells, bits = rods["perm_o"]
    assert bits == 7 and cells.max() < (1 << bits) - 1          # no body clamped into the border cells
    np.testing.assert_array_equal(rods["perm"], expected)
    b, p = rods["b"], rods["perm"]
    for k in ("center", "quat", "radius", "length"):
        _bits(rods["reordered"][k], b[k][p], "reordered " + k)


def test_rods_aabb_and_bounding_radius(rods):
    p = rods["perm"]
    _bits(rods["aabb"], rods["aabb_o"][p], "AABBs")
    _bits(rods["brad"], rods["brad_o"][p], "bounding radii")


def test_rods_neighbour_lists_equal_the_oracle(ops, rods):
    p, uniq = rods["perm"], rods["pairs_o"]
    assert len(uniq) == ROD_CONTACTS
    _assert_same_list(_original(rods["pairs"], p), uniq, N, "the stepper's list")
    assert rods["method"] == ops.SEARCH_METHOD_GRID                 # AUTO on equal rods
    assert rods["rows"] > SHORT_SEGMENT                             # a long row on the stepper's own path
    for name, (got, used, rows, method) in rods["lists"].items():
        assert used == method, (name, used)                         # 4 x reach << box edge: no hand-over to the grid
        exp = rods["pairs_o_periodic"] if "periodic" in name else uniq
        _assert_same_list(got, exp, N, name, symmetric="symmetric" in name)
        if "symmetric" in name:
            assert rows > SHORT_SEGMENT, (name, rows)               # long rows took the workgroup sort
    assert N > REFIT_CHUNK                                           # the LBVH cases took the two-level refit
    assert len(rods["pairs_o_periodic"]) > len(uniq)                 # the box's faces do add pairs


def test_rods_contacts_bit_exact(rods):
    con, con_o = rods["con"], rods["con_o"]
    _bits(rods["seg"], rods["seg_o"][rods["perm"]], "segment records")
    for k in ("sep", "normal", "s", "t"):
        _bits(con[k], con_o[k], "rod contacts: " + k)
    assert (con["sep"] < 0).sum() > 100_000                          # overlapping rods: a solve with work to do


def test_rods_operator_bit_exact(rods):
    p = rods["perm"]
    mt, mr = rods["mob_o"]
    _bits(rods["mob"][0], mt[p], "translational mobility")
    _bits(rods["mob"][1], mr[p], "rotational mobility")
    _bits(rods["y"], rods["y_o"], "apply of the stepper's operator")
    _bits(rods["xvel"], rods["xvel_o"][p], "body velocity rows (U, W) of x")


def test_rods_solve_bit_exact(rods):
    tier = rods["tier"]
    assert len(rods["pairs"]) >= TIER_MIN_CONTACTS
    assert tier["renumberings"] >= 1 and tier["tiered_iterations"] > 0, tier
    assert rods["drift"] == 1                                        # by size: the row form at 10^6 rods
    assert rods["res"].num_iters == K_ROD
    _assert_same_solve((rods["lam"], rods["grad"], rods["res"], rods["state"]), rods["solve_o"], "10^6 rods, K = %d"
                       % K_ROD)
    assert (rods["res2"].num_iters, rods["res2"].residual) == (rods["res"].num_iters, rods["res"].residual)


def test_rods_integrate_bit_exact(rods):
    p = rods["perm"]
    _bits(rods["vel"], rods["vel_o"][p], "velocity rows of the solve's multipliers")
    _bits(rods["center1"], rods["center1_o"][p], "centres after integrate")
    _bits(rods["quat1"], rods["quat1_o"][p], "quaternions after integrate")
    assert np.abs(rods["vel"][:, 3:]).max() > 0                     # the rods turn


# ---- mixed bodies: bench.py --mixed, configs[4] -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ops, oracle):
    from gpu_util import dev, host
    from mundy_amd import pipeline, synth
    T = _Clock("10^6 mixed bodies, configs[4]")
    b = synth.mixed_bodies(N, volume_fraction=MIXED_PHI, seed=1234)
    kind, c, q, shape = b["kind"], b["center"], b["quat"], b["shape"]
    st = pipeline.ContactStepper("mixed", dev(c), None, dev(q), search_buffer=BUFFER,
                                 cfg=ops.PGDConfig(max_iters=K_MIXED, tol=1e-12), kinds=dev(kind), shape=dev(shape))
    R = dict(b=b)
    R["perm"] = p = host(T.device("reorder", lambda: st.reorder_bodies(cell_size=CELL, lo=[0.0, 0.0, 0.0]))).astype(
        np.int64)
    T.device("aabb", st.compute_aabb)
    cons, cons_brad = T.device("aabb", lambda: ops.compute_aabb_mixed(st.kinds, st.center, st.quat, st.shape,
                                                                      conservative_ellipsoids=True))
    R["aabb"], R["brad"], R["aabb_c"], R["brad_c"] = host(st.aabb), host(st.bounding_radius), host(cons), host(cons_brad)
    aabb_o, brad_o = T.oracle("aabb", lambda: oracle.aabb_mixed(kind, c, q, shape))
    ell = kind == 2
    cons_o = aabb_o.copy()
    cons_o[ell] = oracle.compute_aabb_ellipsoids_conservative(c[ell], q[ell], shape[ell])
    R["aabb_o"], R["brad_o"], R["aabb_c_o"] = aabb_o, brad_o, cons_o

    T.device("neighbour list", lambda: st.generate_neighbor_links(force=True))
    R["pairs"], R["method"] = host(st.links.pairs), st.links.method_used()
    g = ops.GenNeighborLinks().set_search_kind(ops.SEARCH_AABB).set_search_buffer(BUFFER).concretize()
    T.device("neighbour list", lambda: g.generate(cons, st.center, cons_brad))
    R["pairs_c"] = _original(host(g.pairs), p)
    g.close()
    for key, box in (("pairs_o", aabb_o), ("pairs_c_o", cons_o)):
        lo, hi, reach = oracle.grow(box, brad_o, BUFFER)
        R[key] = T.oracle("neighbour list", lambda: oracle.search(oracle.SEARCH_AABB, lo, hi, c, reach))

    T.device("contacts", st.compute_contacts)
    con = R["con"] = {k: host(st.contacts[k]) for k in ("sep", "normal", "ra", "rb")}
    po = _original(R["pairs"], p)
    ka, kb = kind[po[:, 0]], kind[po[:, 1]]
    R["cls"] = cls = np.minimum(ka, kb) * 3 + np.maximum(ka, kb)
    R["con_o"] = {}
    with oracle.shared_trig():
        for name, code in (("SS", 0), ("SR", 1), ("RR", 4), ("SE", 2), ("RE", 5), ("EE", 8)):
            idx = np.nonzero(cls == code)[0]
            if name == "EE":
                idx = np.sort(np.random.default_rng(5).choice(idx, EE_SAMPLE, replace=False))
            sub = np.ascontiguousarray(po[idx])
            R["con_o"][name] = (idx, T.oracle("contacts", lambda: oracle.contact_mixed(sub, kind, c, q, shape)))

    C = len(po)
    res = T.device("operator + solve", lambda: st.resolve_collisions(True))
    R["lam"], R["grad"], R["res"] = host(st.lam), host(st.grad), res
    state = _state(C)
    _, _, R["res2"] = ops.solve_lcp(st.op, st.contacts["sep"], None, st.cfg, state=state)
    R["state"] = [host(a) for a in state]
    x = np.random.default_rng(2025).random(C)
    x[::3] = 0.0
    R["y"] = T.device("apply", lambda: host(st.op.apply(dev(x))))
    R["mob"] = host(st.mob_trans), host(st.mob_rot)
    # the operator of the device's own contacts: all of E-E is out of the oracle's reach, the other classes are pinned
    # by test_mixed_contacts_bit_exact
    mt, mr = synth.dry_mobility(brad_o)
    R["mob_o"] = mt, mr
    with oracle.compensated_sums():
        R["y_o"] = T.oracle("apply", lambda: oracle.contact_op_apply(po, con["normal"], con["ra"], con["rb"], mt, mr,
                                                                     DT, x, N, parallel=True))
        R["solve_o"] = T.oracle("operator + solve", lambda: oracle.solve_cqpp_contact(
            po, con["normal"], con["ra"], con["rb"], mt, mr, DT, con["sep"], np.zeros(C), max_iters=K_MIXED,
            tol=1e-12, previous=True, parallel=True))
    T.note("contacts %d (conservative box %d); method %d; classes %s" % (
        C, len(R["pairs_c"]), R["method"], {n: int((cls == k).sum()) for n, k in
                                            (("SS", 0), ("SR", 1), ("RR", 4), ("SE", 2), ("RE", 5), ("EE", 8))}))
    T.report()
    yield R
    st.op.close()
    st.links.close()


def test_mixed_aabbs_bit_exact(mixed):
    p = mixed["perm"]
    _bits(mixed["aabb"], mixed["aabb_o"][p], "mixed AABBs, the reference's ellipsoid box")
    _bits(mixed["aabb_c"], mixed["aabb_c_o"][p], "mixed AABBs, the conservative ellipsoid box")
    _bits(mixed["brad"], mixed["brad_o"][p], "bounding radii")
    _bits(mixed["brad_c"], mixed["brad_o"][p], "bounding radii (conservative box)")
    ell = mixed["b"]["kind"][p] == 2
    assert (mixed["aabb_c"][ell] != mixed["aabb"][ell]).any()        # the two boxes are different boxes


def test_mixed_neighbour_lists_equal_the_oracle(mixed):
    p = mixed["perm"]
    _assert_same_list(_original(mixed["pairs"], p), mixed["pairs_o"], N, "mixed list, reference box")
    _assert_same_list(mixed["pairs_c"], mixed["pairs_c_o"], N, "mixed list, conservative box")
    assert min(len(mixed["pairs_c_o"]), len(mixed["pairs_o"])) > 3_000_000


def test_mixed_contacts_bit_exact(mixed):
    con = mixed["con"]
    for name, (idx, exp) in mixed["con_o"].items():
        assert len(idx) >= (EE_SAMPLE if name == "EE" else 100_000), (name, len(idx))
        for k in ("sep", "normal", "ra", "rb"):
            _bits(con[k][idx], exp[k], "mixed contacts %s: %s" % (name, k))
    covered = sum(len(idx) for name, (idx, _) in mixed["con_o"].items() if name != "EE")
    assert covered + (mixed["cls"] == 8).sum() == len(mixed["cls"])     # every contact is in one class


def test_mixed_operator_and_solve_bit_exact(mixed):
    p = mixed["perm"]
    mt, mr = mixed["mob_o"]
    _bits(mixed["mob"][0], mt[p], "translational mobility")
    _bits(mixed["mob"][1], mr[p], "rotational mobility")
    _bits(mixed["y"], mixed["y_o"], "apply of the stepper's operator")
    assert mixed["res"].num_iters == K_MIXED
    _assert_same_solve((mixed["lam"], mixed["grad"], mixed["res"], mixed["state"]), mixed["solve_o"],
                       "10^6 mixed bodies, K = %d" % K_MIXED)


# ---- size-disperse spheres: the LBVH through AUTO, hub rows -----------------------------------------------------------
@pytest.fixture(scope="module")
def poly(ops, oracle):
    from gpu_util import dev, host
    from test_gpu_broadphase import _polydisperse
    T = _Clock("%d size-disperse spheres" % POLY_N)
    c, r = _polydisperse(np.random.default_rng(11), POLY_N, sigma=POLY_SIGMA)
    R = dict(r=r)
    dc, dr = dev(c), dev(r)
    aabb = ops.compute_aabb_spheres(dc, dr)
    R["lists"] = {}
    for sym in (False, True):
        g = (ops.GenNeighborLinks().set_search_kind(ops.SEARCH_SPHERES).set_search_buffer(BUFFER)
             .set_search_method(ops.SEARCH_METHOD_AUTO).set_enforce_source_target_symmetry(sym).concretize())
        T.device("neighbour list", lambda: g.generate(aabb, dc, dr))
        R["lists"][sym] = (host(g.pairs), g.method_used(), int(np.diff(host(g.row_ptr)).max()),
                           int((np.diff(host(g.row_ptr)) > SHORT_SEGMENT).sum()))
        g.close()
    lo, hi, reach = oracle.grow(oracle.compute_aabb_spheres(c, r), r, BUFFER)
    R["pairs_o"] = T.oracle("neighbour list", lambda: oracle.search(oracle.SEARCH_SPHERES, lo, hi, c, reach))
    for sym, (pairs, used, rows, nlong) in R["lists"].items():
        T.note("symmetric %s: %d pairs, method %d, longest row %d, %d rows > %d" % (sym, len(pairs), used, rows, nlong,
                                                                                 SHORT_SEGMENT))
    T.report()
    return R


def test_size_disperse_lists_equal_the_oracle(ops, poly):
    r = poly["r"]
    assert r.max() > 8.0 * np.median(r)
    for sym, (pairs, used, rows, nlong) in poly["lists"].items():
        assert used == ops.SEARCH_METHOD_MORTON_LBVH, used           # the LBVH through AUTO
        assert POLY_N > REFIT_CHUNK                                  # its two-level refit and top pass
        assert rows > 4 * SHORT_SEGMENT and nlong >= 50, (rows, nlong)    # hub rows: the workgroup sort
        _assert_same_list(pairs, poly["pairs_o"], POLY_N, "size-disperse spheres, symmetric %s" % sym, symmetric=sym)
