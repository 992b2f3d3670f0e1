"""The body-parallel forms of the oracle's contact operator and BBPGD solve (contact_op_apply / solve_cqpp_contact with
parallel=True) against the serial forms, bit for bit.  They are the checker of the full-size GPU tests
(tests/test_gpu_full_size_parity.py), where the serial rod-form solve would take seconds per iteration; they are only
useful if they reproduce the serial bits at every thread count: each body sums its contacts in ascending contact order,
exactly the order of the serial scatter."""
import numpy as np
import pytest

DT = 5e-3
N_RODS = 20_000
K = 100


@pytest.fixture(scope="module")
def rods(oracle):
    from mundy_amd import synth
    b = synth.spherocylinders(N_RODS, seed=77)
    c = b["center"]
    aabb = oracle.compute_aabb_spherocylinders(c, b["quat"], b["radius"], b["length"])
    brad = oracle.bounding_radius_spherocylinders(b["radius"], b["length"])
    lo, hi, R = oracle.grow(aabb, brad, 0.1)
    pairs = oracle.search(oracle.SEARCH_AABB, lo, hi, c, R)
    pairs = pairs[(pairs != 0).all(axis=1)]              # body 0 without a contact: an empty row of the incidence
    # contacts in no particular order, some pairs listed (j, i): a body's terms come from both slots of a pair and in
    # an order that is not that of its partners -- what the device's list looks like in another numbering
    rng = np.random.default_rng(5)
    pairs = pairs[rng.permutation(len(pairs))]
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    pairs = np.ascontiguousarray(pairs)
    seg = oracle.spherocylinder_segments(c, b["quat"], b["radius"], b["length"])
    out = oracle.contact_spherocylinders(pairs, seg, c)
    mt, mr = synth.dry_mobility(b["radius"], bounding_radius=brad)
    deg = np.bincount(pairs.ravel(), minlength=N_RODS)
    assert len(pairs) > 4 * N_RODS and deg.max() >= 12 and (deg == 0).any()   # hubs, and bodies with no contact
    return dict(pairs=pairs, out=out, seg=seg, mt=mt, mr=mr)


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, what
    bad = a.view(np.uint64) != b.view(np.uint64)
    assert not bad.any(), "%s: %d of %d elements differ" % (what, int(bad.sum()), a.size)


def _solve(oracle, P, parallel, max_iters, tol, rod=True):
    o = P["out"]
    C = len(P["pairs"])
    kw = dict(rod=(o["s"], o["t"], P["seg"])) if rod else {}
    ra, rb = (None, None) if rod else (o["ra"], o["rb"])
    return oracle.solve_cqpp_contact(P["pairs"], o["normal"], ra, rb, P["mt"], P["mr"], DT, o["sep"], np.zeros(C),
                                     max_iters=max_iters, tol=tol, previous=True, parallel=parallel, **kw)


def _same_solve(a, b, what):
    (xa, ga, ra, (xta, gta)), (xb, gb, rb, (xtb, gtb)) = a, b
    assert ra["num_iters"] == rb["num_iters"] and ra["converged"] == rb["converged"], (what, ra, rb)
    assert np.float64(ra["residual"]).view(np.uint64) == np.float64(rb["residual"]).view(np.uint64), (what, ra, rb)
    for name, u, v in (("x", xa, xb), ("g", ga, gb), ("x_tmp", xta, xtb), ("g_tmp", gta, gtb)):
        _bits(u, v, "%s: %s" % (what, name))


@pytest.fixture(scope="module")
def serial(oracle, rods):
    """the serial solves, compensated sums: K iterations and a run to convergence"""
    with oracle.compensated_sums():
        k = _solve(oracle, rods, False, K, 1e-12)
        conv = _solve(oracle, rods, False, 20_000, 1e-5)
    assert k[2]["num_iters"] == K and not k[2]["converged"]
    assert conv[2]["converged"] and conv[2]["num_iters"] > K, conv[2]
    return dict(k=k, conv=conv)


@pytest.fixture(params=[1, 3, 8])
def threads(request, oracle):
    kept = oracle.num_threads(fast=False)
    oracle.set_num_threads(request.param, fast=False)
    assert oracle.num_threads(fast=False) == request.param
    yield request.param
    oracle.set_num_threads(kept, fast=False)


def test_parallel_rod_apply_and_body_rows_bit_exact(oracle, rods, threads):
    P, o = rods, rods["out"]
    C, N = len(P["pairs"]), N_RODS
    rod = (o["s"], o["t"], P["seg"])
    x = np.random.default_rng(threads).random(C)
    x[::7] = 0.0
    for mode in ("compensated", "serial"):
        with (oracle.compensated_sums() if mode == "compensated" else _nothing()):
            ys, vs = oracle.contact_op_apply(P["pairs"], o["normal"], None, None, P["mt"], P["mr"], DT, x, N, rod=rod,
                                             body_velocity=True)
            yp, vp = oracle.contact_op_apply(P["pairs"], o["normal"], None, None, P["mt"], P["mr"], DT, x, N, rod=rod,
                                             body_velocity=True, parallel=True)
        _bits(yp, ys, "rod apply, %s sums, %d threads" % (mode, threads))
        _bits(vp, vs, "rod body rows, %s sums, %d threads" % (mode, threads))
        assert np.abs(vs).max() > 0 and not np.isnan(ys).any()


def test_parallel_vector_arm_apply_bit_exact(oracle, rods, threads):
    P, o = rods, rods["out"]
    C, N = len(P["pairs"]), N_RODS
    x = np.random.default_rng(10 + threads).random(C)
    with oracle.compensated_sums():
        for ra, rb, mr in ((o["ra"], o["rb"], P["mr"]), (None, None, None)):   # rigid bodies, and translation only
            ys = oracle.contact_op_apply(P["pairs"], o["normal"], ra, rb, P["mt"], mr, DT, x, N)
            yp = oracle.contact_op_apply(P["pairs"], o["normal"], ra, rb, P["mt"], mr, DT, x, N, parallel=True)
            _bits(yp, ys, "vector-arm apply (arms %s), %d threads" % (ra is not None, threads))


def test_parallel_rod_solve_bit_exact_k_iterations(oracle, rods, serial, threads):
    with oracle.compensated_sums():
        par = _solve(oracle, rods, True, K, 1e-12)
    _same_solve(par, serial["k"], "rod solve, K = %d, %d threads" % (K, threads))


def test_parallel_rod_solve_bit_exact_to_convergence(oracle, rods, serial, threads):
    with oracle.compensated_sums():
        par = _solve(oracle, rods, True, 20_000, 1e-5)
    _same_solve(par, serial["conv"], "rod solve to convergence, %d threads" % threads)


def test_parallel_vector_arm_solve_bit_exact(oracle, rods):
    kept = oracle.num_threads(fast=False)
    try:
        with oracle.compensated_sums():
            ref = _solve(oracle, rods, False, 30, 1e-12, rod=False)
            for th in (1, 3, 8):
                oracle.set_num_threads(th, fast=False)
                _same_solve(_solve(oracle, rods, True, 30, 1e-12, rod=False), ref,
                            "vector-arm solve, %d threads" % th)
    finally:
        oracle.set_num_threads(kept, fast=False)


class _nothing:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False
