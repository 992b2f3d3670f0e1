"""Every entry point of include/mundy_hip.h on a stream that is not the null stream (INTEGRATION.md binds the library to
Kokkos::HIP().hip_stream()), bit for bit against the same call on the null stream -- whose results the rest of the suite
pins to the oracle and the models.  tests/stream_util.py is the instrument: the real inputs reach the live buffers
through a producer that sleeps on the side stream, so a launch, memset or copy of the library that lands on any other
stream reads the decoy that lies there meanwhile, and an entry point that blocks although the header calls it
asynchronous finds the stream still busy when it returns.

The table CASES drives one parametrised test; test_every_stream_entry_point_was_called (last) parses the header and fails
for a prototype with a mhip_stream_t that no case called and EXEMPT does not list.  test_scratch_hand_over checks the
ordering of the thread-local scratch between two streams (csrc/scratch_owner.hpp).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip.h")

# ---- the entry points that block the host (mundy_hip.h: "entry points that return host scalars synchronise") -----------
HOST_SCALAR = "returns a host scalar"
SYNCHRONISES = {
    "mhip_memcpy_h2d": "pageable source: reusable on return",
    "mhip_memcpy_d2h": "the data is on the host on return",
    "mhip_stream_synchronize": "what it is for",
    "mhip_contact_history_carry": "when carried is given or new_of_old is NULL (the canonical-order check)",
    "mhip_select_dividing": HOST_SCALAR,
    "mhip_aabb_moved": HOST_SCALAR,
    "mhip_springs_create": "host arrays uploaded before return",
    "mhip_crosslinkers_create": "host arrays uploaded before return",
    "mhip_active_springs_create": "host arrays uploaded before return",
    "mhip_filaments_create": "host arrays uploaded before return",
    "mhip_filament_contacts_create": "host arrays uploaded before return",
    "mhip_filament_contacts_update": HOST_SCALAR,
    "mhip_contact_mixed": "when class_counts is given",
    "mhip_contact_mixed_periodic": "when class_counts is given",
    "mhip_contact_mixed_last_evaluations": HOST_SCALAR,
    "mhip_ellipsoid_last_evaluations": HOST_SCALAR,
    "mhip_broadphase_build": HOST_SCALAR,
    "mhip_broadphase_needs_rebuild": HOST_SCALAR,
    "mhip_contact_op_create": "the pair list is validated on the device and the verdict read on the host",
    "mhip_contact_op_create_rods": "the pair list is validated on the device and the verdict read on the host",
    "mhip_diff_dot2": HOST_SCALAR,
    "mhip_diff_dot4": HOST_SCALAR,
    "mhip_residual": HOST_SCALAR,
    "mhip_bb_step": HOST_SCALAR,
    "mhip_bbpgd_solve_dense": HOST_SCALAR,
    "mhip_bbpgd_solve_contact": HOST_SCALAR,
    "mhip_bbpgd_solve_contact_unfused": HOST_SCALAR,
    "mhip_bbpgd_solve_contact_friction": HOST_SCALAR,
    "mhip_apgd_solve_contact_friction": HOST_SCALAR,
    "mhip_scrap_bbpgd_solve_contact": HOST_SCALAR,
    "mhip_bbpgd_stage_poll": HOST_SCALAR,
    "mhip_bbpgd_stage_end": HOST_SCALAR,
    "mhip_select_contacts": HOST_SCALAR,
    "mhip_filter_pairs_owned": HOST_SCALAR,
    "mhip_partition_pairs_owned": HOST_SCALAR,
    "mhip_select_aabb_overlap": HOST_SCALAR,
    "mhip_select_aabb_overlap_any": HOST_SCALAR,
    "mhip_aabb_bounds": HOST_SCALAR,
}

# ---- stream-taking entry points no case of this file calls: only those that need a communicator --------------------
NEEDS_COMM = "takes a mhip_comm_t: its own communication stream, several processes (tests/test_gpu_distributed.py)"
EXEMPT = {name: NEEDS_COMM for name in (
    "mhip_comm_mailbox_open", "mhip_comm_all_gather", "mhip_comm_exchange_start", "mhip_comm_exchange_finish",
    "mhip_ghost_plan", "mhip_ghost_exchange", "mhip_curve_cut", "mhip_migrate_plan", "mhip_migrate_exchange",
    "mhip_bbpgd_solve_contact_distributed")}


def header_prototypes():
    """{name: argument text} of every `int mhip_*(...)` declaration of the header (comments removed)"""
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def stream_prototypes():
    return {n: a for n, a in header_prototypes().items() if "mhip_stream_t" in a}


# ---- CPU checks of the tables -------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) >= 130, len(streamed)
    for name in SYNCHRONISES:
        assert name in protos, "%s (SYNCHRONISES) is not declared in mundy_hip.h" % name
    for name in EXEMPT:
        assert name in streamed, "%s (EXEMPT) takes no stream" % name
        assert "mhip_comm_t" in streamed[name], "%s is exempt but takes no communicator" % name
    for case in CASES:
        for fn in case.fns:
            assert fn in protos, "%s: %s is not declared in mundy_hip.h" % (case.name, fn)
        if case.blocks is False:
            assert all(SYNCHRONISES[f].startswith("when ") for f in case.fns if f in SYNCHRONISES), case.name
    assert len({c.name for c in CASES}) == len(CASES)


def test_python_layers_reach_the_library_through_capi_load():
    # the coverage count replaces capi.load by a recorder: that sees every call only if no layer opens the library itself,
    # imports load() by name or keeps what it returned at module level
    for mod in ("ops", "pipeline", "distributed"):
        src = open(os.path.join(ROOT, "mundy_amd", mod + ".py")).read()
        assert "CDLL" not in src and "LIB_PATH" not in src and "capi._lib" not in src, mod
        assert not re.search(r"^from\s+\S*capi\s+import\s[^\n]*\bload\b", src, flags=re.M), mod
        assert not re.search(r"^\S[^\n]*capi\.load\(", src, flags=re.M), "%s keeps the library at module level" % mod
    assert "capi.load()" in open(os.path.join(ROOT, "mundy_amd", "ops.py")).read()


# ---- inputs ---------------------------------------------------------------------------------------------------------------
N = 3001            # bodies: eleven full workgroups of 256 and a partial one
NKEYS = 5000
BOX = 25.0
CELL = np.array([[25.0, 3.0, 1.0], [0.0, 24.0, 2.0], [0.0, 0.0, 26.0]])  # lattice vectors as columns
_cache = {}


def _oracle():
    import oracle
    oracle.build()
    return oracle


def _rng(seed, salt):
    return np.random.default_rng(7919 * salt + seed)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def D(**arrays):
    return {k: dev(v) for k, v in arrays.items()}


def p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def lib():
    from mundy_amd import capi
    return capi.load()


def O():
    from mundy_amd import ops
    return ops


def check(status):
    from mundy_amd import capi
    capi.check(status)


def stream():
    from mundy_amd import ops
    return ops._stream()


def _unit(a):
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def _pairs(rng, n, c):
    """c index pairs (i, j), i != j, int32"""
    pr = rng.integers(0, n, (c, 2))
    same = pr[:, 0] == pr[:, 1]
    pr[same, 1] = (pr[same, 0] + 1) % n
    return pr.astype(np.int32)


def _canonical_pairs(rng, n, c):
    """c distinct pairs i < j in ascending (i, j) order"""
    pr = np.sort(_pairs(rng, n, c + c // 2), axis=1)
    pr = np.unique(pr, axis=0)
    assert len(pr) >= c
    pr = pr[np.sort(rng.permutation(len(pr))[:c])]
    return np.ascontiguousarray(pr.astype(np.int32))


def m_rods(seed):
    from gpu_util import random_rods
    c, q, r, l = random_rods(_rng(seed, 1), N, BOX)
    return dict(center=c, quat=q, radius=r, length=l)


def m_rods_seg(seed):
    b = m_rods(seed)
    b["seg"] = _oracle().spherocylinder_segments(b["center"], b["quat"], b["radius"], b["length"])
    return b


def m_ellipsoids(seed, n=N, edge=BOX, salt=2):
    rng = _rng(seed, salt)
    return dict(center=rng.uniform(0, edge, (n, 3)), quat=_unit(rng.normal(size=(n, 4))),
                radii=rng.uniform(0.4, 1.0, (n, 3)))


def m_points(seed, names, salt=3):
    rng = _rng(seed, salt)
    return {k: rng.uniform(0, BOX, (N, 3)) for k in names}


def m_mixed(seed):
    from mundy_amd import synth
    b = synth.mixed_bodies(N, seed=4321 + seed)
    return dict(kind=b["kind"], center=b["center"], quat=b["quat"], shape=b["shape"]), b["box"]


def problem(maker, seed=3, n=N):
    """the solver problems of the suite's own makers at N bodies, checked as scripts/dump_secondary_solves.py checks its
    inputs: more than one 256-contact tile, a partial last tile, a body with at most one incidence entry and (cone
    paths) one with more entries than one pass of the sweep's 8 lanes x 2 entries covers"""
    key = (maker, seed, n)
    if key not in _cache:
        import test_gpu_convex as tc
        import test_oracle_friction_ext as tf
        fn = {"sphere": tc._sphere_problem, "rod": tc._rod_problem, "rod_arclength": tc._rod_problem_arclength,
              "cone": tf._rod_system}[maker]
        P = fn(_oracle(), n, seed=seed)
        nc = len(P["pairs"])
        deg = np.bincount(np.asarray(P["pairs"]).ravel(), minlength=n)
        assert nc > 256 and nc % 256 != 0 and deg.min() <= 1 and (maker != "cone" or deg.max() > 16), (maker, nc, deg.max())
        _cache[key] = P
    return _cache[key]


def new_op(P, live=None, cone=False):
    """the contact operator of a problem; `live` supplies the device arrays a create case delays"""
    from mundy_amd import ops
    g = (lambda k: live[k]) if live is not None else (lambda k: None if P[k] is None else dev(P[k]))
    if P.get("rod"):
        return ops.ContactOperator(g("pairs"), g("normal"), g("mt"), 5e-3, mob_rot=g("mr"), rod=(g("s"), g("t"), g("seg")))
    if cone:
        return ops.ContactOperator(g("pairs"), g("normal"), g("mt"), 5e-3, ra=g("ras"), rb=g("rbs"), mob_rot=g("mr"))
    ra, rb, mr = (None if P[k] is None else g(k) for k in ("ra", "rb", "mr"))
    return ops.ContactOperator(g("pairs"), g("normal"), g("mt"), 5e-3, ra=ra, rb=rb, mob_rot=mr)


def shuffled(a, seed, salt=9):
    """the rows of `a` in another order: a valid input of the same shape and range (the decoy of a fixed problem)"""
    return a if seed == 0 else np.ascontiguousarray(a[_rng(seed, salt).permutation(len(a))])


CASES = []


def may_block(c):
    """a case blocks the host when an entry point it calls is in SYNCHRONISES; blocks=False marks the non-blocking form
    of one the table lists with a condition ("when ...")"""
    return any(f in SYNCHRONISES for f in c.fns) if c.blocks is None else c.blocks


def case(name, make, call, fns, **kw):
    CASES.append(Case(name, make, call, tuple(fns), **kw))


def ops_call(fn, *names, **kw):
    """call(live, ctx) = ops.<fn>(live[names...], **kw)"""
    def call(live, ctx):
        from mundy_amd import ops
        return getattr(ops, fn)(*[live[k] for k in names], **kw)
    return call


# ---- geometry ---------------------------------------------------------------------------------------------------------------
case("aabb_spheres", lambda s: D(**{k: m_rods(s)[k] for k in ("center", "radius")}),
     ops_call("compute_aabb_spheres", "center", "radius"), ["mhip_compute_aabb_spheres"])
case("aabb_spherocylinders", lambda s: D(**m_rods(s)),
     ops_call("compute_aabb_spherocylinders", "center", "quat", "radius", "length"), ["mhip_compute_aabb_spherocylinders"])
case("aabb_ellipsoids", lambda s: D(**m_ellipsoids(s)), ops_call("compute_aabb_ellipsoids", "center", "quat", "radii"),
     ["mhip_compute_aabb_ellipsoids"])
case("aabb_ellipsoids_conservative", lambda s: D(**m_ellipsoids(s)),
     ops_call("compute_aabb_ellipsoids_conservative", "center", "quat", "radii"),
     ["mhip_compute_aabb_ellipsoids_conservative"])
case("aabb_segments", lambda s: D(seg=m_rods_seg(s)["seg"]), ops_call("compute_aabb_segments", "seg"),
     ["mhip_compute_aabb_segments"])
case("bounding_radius_spherocylinders", lambda s: D(**{k: m_rods(s)[k] for k in ("radius", "length")}),
     ops_call("bounding_radius_spherocylinders", "radius", "length"), ["mhip_bounding_radius_spherocylinders"])
case("bounding_radius_ellipsoids", lambda s: D(radii=m_ellipsoids(s)["radii"]),
     ops_call("bounding_radius_ellipsoids", "radii"), ["mhip_bounding_radius_ellipsoids"])
case("spherocylinder_segments", lambda s: D(**m_rods(s)),
     ops_call("spherocylinder_segments", "center", "quat", "radius", "length"), ["mhip_spherocylinder_segments"])


def m_two_spheres(s):
    rng = _rng(s, 4)
    return D(c1=rng.uniform(0, BOX, (N, 3)), r1=rng.uniform(0.3, 0.6, N), c2=rng.uniform(0, BOX, (N, 3)),
             r2=rng.uniform(0.3, 0.6, N))


case("distance_sphere_sphere", m_two_spheres, ops_call("distance_sphere_sphere", "c1", "r1", "c2", "r2"),
     ["mhip_distance_sphere_sphere"])
case("distance_point_segment", lambda s: D(**m_points(s, ("p", "a0", "a1"))),
     ops_call("distance_point_segment", "p", "a0", "a1"), ["mhip_distance_point_segment"])
case("distance_point_sphere", lambda s: D(r=_rng(s, 5).uniform(0.3, 0.6, N), **m_points(s, ("p", "c"))),
     ops_call("distance_point_sphere", "p", "c", "r"), ["mhip_distance_point_sphere"])
case("distance_segment_sphere", lambda s: D(r=_rng(s, 5).uniform(0.3, 0.6, N), **m_points(s, ("a0", "a1", "c"))),
     ops_call("distance_segment_sphere", "a0", "a1", "c", "r"), ["mhip_distance_segment_sphere"])
case("distance_segment_segment", lambda s: D(**m_points(s, ("a0", "a1", "b0", "b1"))),
     ops_call("distance_segment_segment", "a0", "a1", "b0", "b1"), ["mhip_distance_segment_segment"])

NPAIRS = 10007  # 39 tiles of 256 contacts and a partial one


def m_sphere_pairs(s):
    b = m_rods(s)
    return D(pairs=_pairs(_rng(s, 6), N, NPAIRS), center=b["center"], radius=b["radius"])


def m_rod_pairs(s):
    b = m_rods_seg(s)
    return D(pairs=_pairs(_rng(s, 6), N, NPAIRS), seg=b["seg"], center=b["center"])


case("contact_spheres", m_sphere_pairs, ops_call("contact_spheres", "pairs", "center", "radius"), ["mhip_contact_spheres"])
case("contact_spheres_periodic", m_sphere_pairs, ops_call("contact_spheres", "pairs", "center", "radius", box=[BOX] * 3),
     ["mhip_contact_spheres"])
case("contact_spheres_triclinic", m_sphere_pairs, ops_call("contact_spheres", "pairs", "center", "radius", box=CELL),
     ["mhip_contact_spheres_triclinic"])
case("contact_spherocylinders", m_rod_pairs, ops_call("contact_spherocylinders", "pairs", "seg", "center"),
     ["mhip_contact_spherocylinders"])
case("contact_spherocylinders_arclength", m_rod_pairs,
     ops_call("contact_spherocylinders", "pairs", "seg", "center", want_points=False, arms="arclength"),
     ["mhip_contact_spherocylinders"])
case("contact_spherocylinders_periodic", m_rod_pairs,
     ops_call("contact_spherocylinders", "pairs", "seg", "center", box=[BOX] * 3), ["mhip_contact_spherocylinders_periodic"])


# ---- ellipsoids ---------------------------------------------------------------------------------------------------------------
def m_ee(n):
    def make(s):
        a, b = m_ellipsoids(s, n, 4.0, 11), m_ellipsoids(s, n, 4.0, 12)
        return D(c1=a["center"], q1=a["quat"], r1=a["radii"], c2=b["center"], q2=b["quat"], r2=b["radii"])
    return make


def call_ee_evaluations(live, ctx):
    from mundy_amd import ops
    out = ops.distance_ellipsoid_ellipsoid(*[live[k] for k in ("c1", "q1", "r1", "c2", "q2", "r2")])
    return out, ops.ellipsoid_last_evaluations()


for n_ee in (65, 5000):
    case("distance_ellipsoid_ellipsoid_%d" % n_ee, m_ee(n_ee),
         ops_call("distance_ellipsoid_ellipsoid", "c1", "q1", "r1", "c2", "q2", "r2"), ["mhip_distance_ellipsoid_ellipsoid"])
    case("distance_point_ellipsoid_%d" % n_ee, m_ee(n_ee), ops_call("distance_point_ellipsoid", "c2", "c1", "q1", "r1"),
         ["mhip_distance_point_ellipsoid"])
    case("contact_ellipsoids_%d" % n_ee,
         lambda s, n=n_ee: D(pairs=_pairs(_rng(s, 13), 600, n), **m_ellipsoids(s, 600, 9.0, 14)),
         ops_call("contact_ellipsoids", "pairs", "center", "quat", "radii"), ["mhip_contact_ellipsoids"])
case("ellipsoid_last_evaluations", m_ee(5000), call_ee_evaluations,
     ["mhip_distance_ellipsoid_ellipsoid", "mhip_ellipsoid_last_evaluations"])


# ---- mixed shapes -------------------------------------------------------------------------------------------------------------
def m_mixed_pairs(s):
    b, _ = m_mixed(s)
    return D(pairs=_pairs(_rng(s, 15), N, 5003), **b)


def call_mixed(route=False, last=False, **kw):
    def call(live, ctx):
        from mundy_amd import ops
        ops.contact_mixed_set_sphere_ellipsoid_route(route)
        try:
            out = ops.contact_mixed(live["pairs"], live["kind"], live["center"], live["quat"], live["shape"], **kw)
            return (out, ops.contact_mixed_last_evaluations()) if last else out
        finally:
            ops.contact_mixed_set_sphere_ellipsoid_route(False)
    return call


case("aabb_mixed", lambda s: D(**m_mixed(s)[0]), ops_call("compute_aabb_mixed", "kind", "center", "quat", "shape"),
     ["mhip_compute_aabb_mixed"])
case("aabb_mixed_conservative", lambda s: D(**m_mixed(s)[0]),
     ops_call("compute_aabb_mixed", "kind", "center", "quat", "shape", conservative_ellipsoids=True),
     ["mhip_compute_aabb_mixed_conservative"])
case("contact_mixed", m_mixed_pairs, call_mixed(), ["mhip_contact_mixed"], blocks=False)
case("contact_mixed_minimiser_route", m_mixed_pairs, call_mixed(route=True), ["mhip_contact_mixed"], blocks=False)
case("contact_mixed_counts", m_mixed_pairs, call_mixed(want_counts=True), ["mhip_contact_mixed"])
case("contact_mixed_periodic", m_mixed_pairs, call_mixed(box=[m_mixed(0)[1]] * 3), ["mhip_contact_mixed_periodic"],
     blocks=False)
case("contact_mixed_periodic_counts", m_mixed_pairs, call_mixed(box=[m_mixed(0)[1]] * 3, want_counts=True),
     ["mhip_contact_mixed_periodic"])
case("contact_mixed_last_evaluations", m_mixed_pairs, call_mixed(route=True, last=True),
     ["mhip_contact_mixed_last_evaluations"])


# ---- reorder ----------------------------------------------------------------------------------------------------------------
def key_table(level=4):
    if ("table", level) not in _cache:
        from mundy_amd import ops
        _cache["table", level] = dev(ops.hilbert_key_table(level).astype(np.int32))
    return _cache["table", level]


def m_centres(s):
    return D(center=_rng(s, 20).uniform(0, BOX, (N, 3)))


LO, HI = [0.0] * 3, [BOX] * 3
case("morton_order", m_centres, lambda live, ctx: O().morton_order(live["center"], LO, 1.7),
     ["mhip_morton_order"])
case("curve_order", m_centres,
     lambda live, ctx: O().curve_order(live["center"], LO, HI, 4, key_table()),
     ["mhip_curve_order"])
case("curve_keys", m_centres,
     lambda live, ctx: O().curve_keys(live["center"], LO, HI, 4, key_table()),
     ["mhip_curve_keys"])


def m_keys(s):
    k = _rng(s, 21).integers(0, 1 << 62, NKEYS, dtype=np.int64)
    k[::7] = k[3]  # ties: the sort is stable
    return D(keys=k)


case("sort_by_key_u64", m_keys, ops_call("sort_by_key", "keys"), ["mhip_sort_by_key_u64"])
case("gather_rows", lambda s: D(perm=_rng(s, 22).integers(0, N, N).astype(np.int32), src=_rng(s, 23).normal(size=(N, 7))),
     ops_call("gather_rows", "perm", "src"), ["mhip_gather_rows"])


def call_copy_strided(live, ctx):
    dst = live["dst"]
    check(lib().mhip_copy_strided(N, 5, p(live["src"]), 7, p(dst), 6, stream()))
    return dst


case("copy_strided", lambda s: D(src=_rng(s, 24).normal(size=(N, 7)), dst=_rng(s, 25).normal(size=(N, 6))),
     call_copy_strided, ["mhip_copy_strided"])
case("periodic_sep", lambda s: D(**m_points(s, ("p1", "p2"))),
     lambda live, ctx: O().periodic_sep([BOX] * 3, live["p1"], live["p2"]), ["mhip_periodic_sep"])
case("periodic_sep_triclinic", lambda s: D(**m_points(s, ("p1", "p2"))),
     lambda live, ctx: O().periodic_sep(CELL, live["p1"], live["p2"]), ["mhip_periodic_sep_triclinic"])
case("wrap_rigid", lambda s: D(center=_rng(s, 26).uniform(-2 * BOX, 3 * BOX, (N, 3))),
     lambda live, ctx: O().wrap_rigid([BOX] * 3, live["center"]), ["mhip_wrap_rigid"])
case("wrap_rigid_triclinic", lambda s: D(center=_rng(s, 26).uniform(-2 * BOX, 3 * BOX, (N, 3))),
     lambda live, ctx: O().wrap_rigid(CELL, live["center"]), ["mhip_wrap_rigid_triclinic"])
case("shift_image_triclinic",
     lambda s: D(p=_rng(s, 27).uniform(0, BOX, (N, 3)), images=_rng(s, 28).integers(-2, 3, (N, 3)).astype(np.int32)),
     lambda live, ctx: O().shift_image(CELL, live["p"], live["images"]),
     ["mhip_shift_image_triclinic"])


def m_euler(s):
    b = m_rods(s)
    return D(velocity=_rng(s, 29).normal(size=(N, 6)), center=b["center"], quat=b["quat"])


def call_euler(live, ctx):
    from mundy_amd import ops
    ops.integrate_euler(5e-3, live["velocity"], live["center"], live["quat"])
    return live["center"], live["quat"]


case("integrate_euler", m_euler, call_euler, ["mhip_integrate_euler"])


def call_compose(live, ctx):
    out = torch.empty(NKEYS, dtype=torch.int64, device="cuda")
    check(lib().mhip_compose_keys_u64(NKEYS, p(live["major"]), p(live["minor"]), 24, p(out), stream()))
    return out


case("compose_keys_u64",
     lambda s: D(major=_rng(s, 30).integers(0, 1 << 31, NKEYS).astype(np.int32),
                 minor=_rng(s, 31).integers(0, 1 << 24, NKEYS).astype(np.float64)), call_compose, ["mhip_compose_keys_u64"])


def call_fill_sequence(live, ctx):
    # (no device input: the buffer written is a live one, and its first element stays what the producer delivered)
    out = live["out"]
    check(lib().mhip_fill_sequence(N - 1, 17.0, p(out[1:]), stream()))
    return out


case("fill_sequence", lambda s: D(out=_rng(s, 32).normal(size=N)), call_fill_sequence, ["mhip_fill_sequence"])


def call_work_weights(live, ctx):
    w = torch.empty(1025, dtype=torch.float64, device="cuda")
    check(lib().mhip_body_work_weights(NPAIRS, p(live["pairs"]), 1000, 1025, p(w), stream()))
    return w


case("body_work_weights", lambda s: D(pairs=_pairs(_rng(s, 33), N, NPAIRS)), call_work_weights, ["mhip_body_work_weights"])


# ---- halo: ballot compactions and box reductions ----------------------------------------------------------------------------
def m_aabb(s):
    lo = _rng(s, 40).uniform(0, 20, (N, 3))
    lo = lo[np.argsort(lo[:, 0])]
    return D(aabb=np.concatenate([lo, lo + _rng(s, 41).uniform(0.1, 1.0, (N, 3))], axis=1))


def call_owned(which):
    def call(live, ctx):
        out = torch.empty((NPAIRS, 2), dtype=torch.int32, device="cuda")
        counted = torch.empty(NPAIRS, dtype=torch.uint8, device="cuda")
        cnt, n_int = C.c_size_t(0), C.c_size_t(0)
        if which == "filter":
            check(lib().mhip_filter_pairs_owned(NPAIRS, p(live["pairs"]), 700, 1500, p(out), p(counted), C.byref(cnt),
                                                stream()))
        else:
            check(lib().mhip_partition_pairs_owned(NPAIRS, p(live["pairs"]), 700, 1500, p(out), p(counted),
                                                   C.byref(n_int), C.byref(cnt), stream()))
        return out[:cnt.value], counted[:cnt.value], int(cnt.value), int(n_int.value)
    return call


case("filter_pairs_owned", lambda s: D(pairs=np.sort(_pairs(_rng(s, 42), N, NPAIRS), axis=1)), call_owned("filter"),
     ["mhip_filter_pairs_owned"])
case("partition_pairs_owned", lambda s: D(pairs=np.sort(_pairs(_rng(s, 42), N, NPAIRS), axis=1)), call_owned("partition"),
     ["mhip_partition_pairs_owned"])


def call_select_overlap(live, ctx):
    idx = torch.empty(N, dtype=torch.int32, device="cuda")
    cnt = C.c_size_t(0)
    check(lib().mhip_select_aabb_overlap(N, p(live["aabb"]), 0.25, (C.c_double * 6)(2.0, 2, 2, 9, 9, 9), p(idx),
                                         C.byref(cnt), stream()))
    return idx[:cnt.value], int(cnt.value)


def call_chunk_bounds(live, ctx):
    boxes = torch.empty((8, 6), dtype=torch.float64, device="cuda")
    check(lib().mhip_aabb_chunk_bounds(N, p(live["aabb"]), 0.15, 7, p(boxes), stream()))
    return boxes


def call_overlap_any(live, ctx):
    boxes = call_chunk_bounds(live, ctx)
    idx = torch.empty(N, dtype=torch.int32, device="cuda")
    cnt = C.c_size_t(0)
    check(lib().mhip_select_aabb_overlap_any(N, p(live["query"]), 0.15, 3, p(boxes), p(idx), C.byref(cnt), stream()))
    return idx[:cnt.value], int(cnt.value)


def call_aabb_bounds(live, ctx):
    out6 = (C.c_double * 6)()
    check(lib().mhip_aabb_bounds(N, p(live["aabb"]), 0.3, out6, stream()))
    return [float(v) for v in out6]


def call_select_contacts(live, ctx):
    from mundy_amd import ops
    kept = ops.select_contacts(live["sep"], 0.05)
    return kept, int(kept.shape[0])


case("select_contacts", lambda s: D(sep=_rng(s, 43).uniform(-0.1, 0.3, NPAIRS)), call_select_contacts,
     ["mhip_select_contacts"])
case("select_aabb_overlap", m_aabb, call_select_overlap, ["mhip_select_aabb_overlap"])
case("aabb_chunk_bounds", m_aabb, call_chunk_bounds, ["mhip_aabb_chunk_bounds"])
case("select_aabb_overlap_any", lambda s: dict(m_aabb(s), query=m_aabb(s + 2)["aabb"]), call_overlap_any,
     ["mhip_aabb_chunk_bounds", "mhip_select_aabb_overlap_any"])
case("aabb_bounds", m_aabb, call_aabb_bounds, ["mhip_aabb_bounds"])


# ---- forces -------------------------------------------------------------------------------------------------------------------
def m_hertz(s):
    rng = _rng(s, 50)
    return D(pairs=_pairs(rng, N, NPAIRS), sep=rng.uniform(-0.1, 0.1, NPAIRS), radius=rng.uniform(0.3, 0.6, N))


def m_hertz_friction(s):
    rng = _rng(s, 51)
    b = m_rods_seg(s)
    return D(pairs=_pairs(rng, N, NPAIRS), sep=rng.uniform(-0.1, 0.1, NPAIRS), normal=_unit(rng.normal(size=(NPAIRS, 3))),
             arc_s=rng.uniform(0, 1, NPAIRS), arc_t=rng.uniform(0, 1, NPAIRS), seg=b["seg"], radius=b["radius"],
             velocity_prev=rng.normal(size=(N, 6)), tang_disp=0.01 * rng.normal(size=(NPAIRS, 3)))


def call_hertz_friction(live, ctx):
    from mundy_amd import ops
    f, st = ops.hertz_friction_force(*[live[k] for k in ("pairs", "sep", "normal", "arc_s", "arc_t", "seg", "radius",
                                                         "velocity_prev", "tang_disp")], 0.3, 1e-3, damping=(0.1, 0.05))
    return f, st, live["tang_disp"]


case("hertz_contact_force", m_hertz, ops_call("hertz_contact_force", "pairs", "sep", "radius"), ["mhip_hertz_contact_force"])
case("hertz_friction_force", m_hertz_friction, call_hertz_friction, ["mhip_hertz_friction_force"])


def m_carry(s):
    rng = _rng(s, 52)
    return D(pairs_old=_canonical_pairs(rng, N, NPAIRS), hist_old=rng.normal(size=(NPAIRS, 3)),
             pairs_new=_canonical_pairs(rng, N, NPAIRS - 200), new_of_old=rng.permutation(N).astype(np.int32))


def call_carry(renumber, count):
    def call(live, ctx):
        from mundy_amd import ops
        return ops.carry_contact_history(live["pairs_old"], live["hist_old"], live["pairs_new"],
                                         new_of_old=live["new_of_old"] if renumber else None, want_count=count)
    return call


case("contact_history_carry_renumbered", m_carry, call_carry(True, False), ["mhip_contact_history_carry"],
     blocks=False)
case("contact_history_carry_counted", m_carry, call_carry(True, True), ["mhip_contact_history_carry"])
case("contact_history_carry_canonical", m_carry, call_carry(False, False), ["mhip_contact_history_carry"])


def chain(seed=8):
    if ("chain", seed) not in _cache:
        from mundy_amd import synth
        d = synth.chains(3, 1000, seed=seed)
        d["center0"] = d["center"]
        _cache["chain", seed] = d
    return _cache["chain", seed]


def m_chain_centres(s):
    d = chain()
    return D(center=d["center0"] + 0.05 * _rng(s, 53).normal(size=d["center0"].shape))


def open_springs(live):
    from mundy_amd import ops
    d = chain()
    return ops.Springs(d["center0"].shape[0], d["pairs"], "hookean", d["k"], d["r0"])


def call_springs_lifecycle(live, ctx):
    h = open_springs(live)
    try:
        return h.force(live["center"])
    finally:
        h.close()


case("springs_force", m_chain_centres, lambda live, h: h.force(live["center"]), ["mhip_springs_force"], open=open_springs,
     close=lambda h: h.close())
case("springs_lifecycle", m_chain_centres, call_springs_lifecycle, ["mhip_springs_create", "mhip_springs_force"])


def m_philox(s):
    rng = _rng(s, 54)
    return D(keys=rng.integers(0, 1 << 62, N, dtype=np.int64), counters=rng.integers(0, 1 << 40, N, dtype=np.int64),
             mob_trans=rng.uniform(0.5, 2.0, N), velocity=rng.normal(size=(N, 6)), force=rng.normal(size=(N, 3)))


def call_brownian(live, ctx):
    from mundy_amd import ops
    ops.brownian_velocity(live["keys"], live["counters"], 0.1, 1e-3, live["mob_trans"], live["velocity"])
    return live["velocity"], live["counters"]


case("philox4x32_10", m_philox, ops_call("philox4x32_10", "keys", "counters", block=1), ["mhip_philox4x32_10"])
case("brownian_velocity", m_philox, call_brownian, ["mhip_brownian_velocity"])
case("drag_velocity", m_philox, ops_call("drag_velocity", "mob_trans", "force"), ["mhip_drag_velocity"])


def m_periphery(radii):
    def make(s):
        rng = _rng(s, 55)
        c = _unit(rng.normal(size=(N, 3))) * rng.uniform(0.0, 0.97, (N, 1)) * np.asarray(radii)
        return D(center=c, radius=np.full(N, 0.5), out=rng.normal(size=(N, 3)))
    return make


def call_periphery(spec):
    def call(live, ctx):
        from mundy_amd import ops
        return ops.periphery_force(spec, live["center"], live["radius"], out=live["out"], accumulate=True)
    return call


case("periphery_force_sphere", m_periphery([10.0] * 3), call_periphery(dict(shape="sphere", radius=10.0, k=3.0)),
     ["mhip_periphery_force"])
case("periphery_force_ellipsoid", m_periphery([10.0, 8.0, 6.0]),
     call_periphery(dict(shape="ellipsoid", radii=(10.0, 8.0, 6.0), k=3.0, quat=(0.9, 0.1, 0.3, 0.3))), ["mhip_periphery_force"])
case("periphery_force_ellipsoid_fast", m_periphery([10.0, 8.0, 6.0]),
     call_periphery(dict(shape="ellipsoid_fast", radii=(10.0, 8.0, 6.0), k=3.0)), ["mhip_periphery_force"])


# active springs: the state itself is an input (set_state), so the switching clock arrives through the delayed producer
def _active_handle(keys_seed=0):
    from mundy_amd import ops
    d = chain()
    m = d["pairs"].shape[0]
    sel = np.arange(0, m, 2)
    return ops.ActiveSprings(d["center0"].shape[0], d["pairs"][sel], 2.0, 40.0, 60.0,
                             keys=_rng(keys_seed, 56).integers(0, 1 << 62, len(sel), dtype=np.int64))


def m_active(s):
    h = _active_handle(s)
    for _ in range(3 + s):  # a valid state of its own: some springs on, clocks part-way
        h.sample()
        h.advance(5e-3)
    st, nt, el, ct = h.state()
    torch.cuda.synchronize()
    h.close()
    n = chain()["center0"].shape[0]
    return dict(state=st, next_time=nt, elapsed=el, counter=ct, new_of_old=dev(_rng(s, 57).permutation(n).astype(np.int32)),
                **m_chain_centres(s))


def call_active(live, h, renumber=False):
    h.set_state(live["state"], live["next_time"], live["elapsed"], live["counter"])
    sw = h.sample()
    f, active = h.force(live["center"])
    h.advance(5e-3)
    out = [sw, f, active, h.state()]
    if renumber:  # (not undone: only where the handle lives for one call)
        h.renumber(live["new_of_old"])
        out += [h.force(live["center"], out=f.clone(), accumulate=True)[0], h.state()]
    return out


def call_active_lifecycle(live, ctx):
    h = _active_handle()
    try:
        return call_active(live, h, renumber=True)
    finally:
        h.close()


ACTIVE_FNS = ["mhip_active_springs_set_state", "mhip_active_springs_sample", "mhip_active_springs_force",
              "mhip_active_springs_advance", "mhip_active_springs_get_state"]
case("active_springs", m_active, call_active, ACTIVE_FNS, open=lambda live: _active_handle(), close=lambda h: h.close())
case("active_springs_lifecycle", m_active, call_active_lifecycle,
     ["mhip_active_springs_create", "mhip_active_springs_renumber"] + ACTIVE_FNS)


# crosslinkers: heads, candidate list, keys and counters are inputs
XL = dict(kind="hookean", k=3.0, r=1.0, bind_rate=200.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5)


def _xl_handle():
    from mundy_amd import ops
    d = chain()
    n = d["center0"].shape[0]
    left = np.arange(0, n, 2)
    sites = (np.arange(n) % 3 != 0).astype(np.uint8)
    return ops.Crosslinkers(n, left, None, sites, XL["kind"], XL["k"], XL["r"], XL["bind_rate"], XL["unbind_rate"],
                            XL["kt"], XL["capture_radius"])


def _xl_candidates():
    """CSR of the bodies within the capture radius (+ skin) of each other at the chain's own positions"""
    if "xl_csr" not in _cache:
        from mundy_amd import ops
        d = chain()
        n = d["center0"].shape[0]
        c = dev(d["center0"])
        links = (ops.GenNeighborLinks().set_search_buffer(0.5).set_search_kind(ops.SEARCH_SPHERES)
                 .set_enforce_source_target_symmetry(True).concretize())
        links.generate(None, c, torch.full((n,), 0.75, dtype=torch.float64, device="cuda"))
        _cache["xl_csr"] = (links.row_ptr.cpu().numpy(), links.col.cpu().numpy())
        links.close()
    return _cache["xl_csr"]


def m_crosslinkers(s):
    d = chain()
    n = d["center0"].shape[0]
    rng = _rng(s, 58)
    left = np.arange(0, n, 2)
    m = len(left)
    row_ptr, col = _xl_candidates()
    right = left.copy()  # a third bound to a site among the left head's candidates
    for i in rng.permutation(m)[: m // 3]:
        cand = col[row_ptr[left[i]]:row_ptr[left[i] + 1]]
        cand = cand[cand % 3 != 0]
        if len(cand):
            right[i] = cand[rng.integers(0, len(cand))]
    # the same candidates in another order inside every row is the same list to the library only after its own sort:
    # the decoy takes the rows as they are and differs in heads, keys, counters and positions
    return dict(right=dev(right.astype(np.int32)), row_ptr=dev(row_ptr.astype(np.int32)), col=dev(col.astype(np.int32)),
                ids=dev(np.arange(n, dtype=np.int64)), keys=dev(rng.integers(0, 1 << 62, m, dtype=np.int64)),
                counters=dev(rng.integers(0, 1 << 40, m, dtype=np.int64)),
                new_of_old=dev(rng.permutation(n).astype(np.int32)), **m_chain_centres(s))


def call_crosslinkers(live, h, renumber=False):
    m = live["right"].shape[0]
    h.set_state(None, live["right"])
    h.set_candidates(live["row_ptr"], live["col"], live["ids"])
    z = torch.zeros(m, dtype=torch.float64, device="cuda")
    ev = h.kmc_step(live["center"], 1e-3, live["keys"], live["counters"], z_total=z)
    out = [ev, z, h.force(live["center"]), h.state("cuda"), live["counters"]]
    if renumber:  # (not undone: only where the handle lives for one call)
        h.renumber(live["new_of_old"])
        out.append(h.state("cuda"))
    return out


def call_crosslinkers_lifecycle(live, ctx):
    h = _xl_handle()
    try:
        return call_crosslinkers(live, h, renumber=True)
    finally:
        h.close()


XL_FNS = ["mhip_crosslinkers_set_state", "mhip_crosslinkers_set_candidates", "mhip_crosslinkers_kmc_step",
          "mhip_crosslinkers_force", "mhip_crosslinkers_get_state"]
case("crosslinkers", m_crosslinkers, call_crosslinkers, XL_FNS, open=lambda live: _xl_handle(), close=lambda h: h.close())
case("crosslinkers_lifecycle", m_crosslinkers, call_crosslinkers_lifecycle,
     ["mhip_crosslinkers_create", "mhip_crosslinkers_renumber"] + XL_FNS)


# hydrodynamics: ns = 2 chunks + 77 sources, 300 targets, both workspace paths
def m_hydro(s):
    import hydro_model as hm
    d = hm.inputs(2 * hm.CHUNK + 77, 300, seed=60 + s)
    return D(sc=d["sc"], sa=d["sa"], f=d["f"], tc=d["tc"], tb=d["tb"], out=_rng(s, 61).normal(size=(300, 6)))


def open_hydro(path):
    def open_(live):
        from mundy_amd import ops
        ws = ops.HydroWorkspace()
        ws.set_path(path)
        return ws
    return open_


def call_hydro(kind, accumulate=False):
    def call(live, ws):
        from mundy_amd import ops
        if accumulate:
            return ops.hydro_velocity(kind, 0.7, live["sc"], live["sa"], live["f"], live["tc"], live["tb"], out=live["out"],
                                      accumulate=True, workspace=ws)
        return ops.hydro_velocity(kind, 0.7, live["sc"], live["sa"], live["f"], live["tc"], live["tb"], workspace=ws)
    return call


for path in ("in_lane", "partial"):
    for kind in ("rpyc", "rpy", "stokes"):
        case("hydro_velocity_%s_%s" % (kind, path), m_hydro, call_hydro(kind), ["mhip_hydro_velocity"],
             open=open_hydro(path), close=lambda ws: ws.close())
    case("hydro_velocity_accumulate_%s" % path, m_hydro, call_hydro("rpyc", True), ["mhip_hydro_velocity"],
         open=open_hydro(path), close=lambda ws: ws.close())
case("hydro_add_velocity", lambda s: D(u=_rng(s, 62).normal(size=(N, 3)), velocity=_rng(s, 63).normal(size=(N, 6))),
     ops_call("hydro_add_velocity", "u", "velocity"), ["mhip_hydro_add_velocity"])


# filaments and their contacts: the handle runs on the stream current at its creation, so a case is a whole life
def _filament_case(s):
    key = ("filaments", s)
    if key not in _cache:
        from test_gpu_filaments import BORDER_COUNTS, make_case
        _cache[key] = make_case(26 + s, BORDER_COUNTS)
    return _cache[key]


def m_filaments(s):
    c = _filament_case(s)
    return D(center=c["center"], twist=c["twist"], edge_orientation=c["edge_orientation"],
             ext=0.1 * _rng(s, 64).normal(size=(c["n"], 3)))


FILAMENT_OUT = ("center", "twist", "edge_tangent", "edge_length", "edge_binormal", "edge_orientation", "curvature", "force",
                "twist_torque", "velocity", "twist_velocity", "edge_tangent_old", "edge_orientation_old")


def call_filaments(live, ctx):
    from mundy_amd import ops
    from test_gpu_filaments import device_kwargs, params
    c = _filament_case(0)
    f = ops.Filaments(c["node_ptr"], c["radius"], c["rest_curvature"], c["arclength"], c["phase"],
                      **device_kwargs(params(wave=True)))
    try:
        f.set_state(live["center"], live["twist"], live["edge_orientation"])
        stats = [f.force(0.0, live["ext"])]
        f.velocity()
        f.advance(1e-3)
        f.edge_pass()
        stats.append(f.node_pass(1e-3, live["ext"]))
        f.velocity()
        return stats, {k: f.field(k) for k in FILAMENT_OUT}
    finally:
        f.close()


case("filaments_lifecycle", m_filaments, call_filaments,
     ["mhip_filaments_create", "mhip_filaments_set_state", "mhip_filaments_advance", "mhip_filaments_force",
      "mhip_filaments_edge_pass", "mhip_filaments_node_pass", "mhip_filaments_velocity", "mhip_filaments_get"])


def _crossed(s):
    key = ("crossed", s)
    if key not in _cache:
        from mundy_amd import synth
        _cache[key] = synth.crossed_filaments(24, 12, angle=1.0 + 0.07 * s, overlap=0.125 + 0.02 * s, seed=7)
    return _cache[key]


def m_filament_contacts(s):
    c = _crossed(s)
    n = c["center"].shape[0]
    return D(center=c["center"], twist=c["twist"], edge_orientation=c["edge_orientation"],
             velocity_prev=_rng(s, 65).normal(size=(n, 3)))


def call_filament_contacts(live, ctx):
    from mundy_amd import ops
    from test_gpu_filaments import device_kwargs, params
    c = _crossed(0)
    f = ops.Filaments(c["node_ptr"], c["radius"], c["rest_curvature"], c["arclength"], c["phase"],
                      **device_kwargs(params()))
    fc = None
    try:
        f.set_state(live["center"], live["twist"], live["edge_orientation"])
        fc = ops.FilamentContacts(f, skin=0.5, mu=0.5, youngs_modulus=200.0, poisson_ratio=0.3, damping=(0.1, 0.05))
        f.force(0.0)
        f.velocity()
        fc.save_velocity()
        rebuilt = fc.update()
        fc.set_field("velocity_prev", live["velocity_prev"])
        out = {"rebuilt": rebuilt, "num_pairs": fc.num_pairs, "stats": fc.force(1e-3).clone()}
        out.update({k: fc.field(k) for k in ("pairs", "sep", "tang_disp", "force", "share", "node_force", "seg", "aabb")})
        # the same in its halves, on a history planted by hand
        pairs = fc.field("pairs")
        fc.set_history(pairs, out["tang_disp"] * 0.5)
        fc.segment_view()
        out["stats2"] = fc.linker_pass(1e-3, stats=torch.zeros(2, dtype=torch.float64, device="cuda"))
        fc.reduce()
        out.update({k + "2": fc.field(k) for k in ("tang_disp", "force", "node_force")})
        f.force(1e-3, fc.node_force_ptr())
        out["filament_force"] = f.field("force")
        return out
    finally:
        if fc is not None:
            fc.close()
        f.close()


case("filament_contacts_lifecycle", m_filament_contacts, call_filament_contacts,
     ["mhip_filaments_create", "mhip_filament_contacts_create", "mhip_filament_contacts_save_velocity",
      "mhip_filament_contacts_update", "mhip_filament_contacts_force", "mhip_filament_contacts_segment_view",
      "mhip_filament_contacts_linker_pass", "mhip_filament_contacts_reduce", "mhip_filament_contacts_set_history",
      "mhip_filament_contacts_get"])


# growth
def m_growth(s):
    b = m_rods(s)
    cap = N + N // 2
    pad = lambda a: np.concatenate([a, np.zeros((cap - N,) + a.shape[1:])])  # noqa: E731
    return D(center=pad(b["center"]), quat=pad(b["quat"]), radius=pad(b["radius"]), length=pad(b["length"]))


def call_select_dividing(live, ctx):
    from mundy_amd import ops
    parent_of, nb = ops.select_dividing(live["length"][:N], 1.9)
    return parent_of, nb


def call_divide_grow(live, ctx):
    # parent_of: every seventh body (a host-side choice, so that the call under test is the only library call)
    from mundy_amd import ops
    ops.divide_grow_spherocylinders(N, live["parent_of"], 0.01, 0.5, live["center"], live["quat"], live["radius"],
                                    live["length"], box=[BOX] * 3)
    return live["center"], live["quat"], live["radius"], live["length"]


def m_divide_grow(s):
    d = m_growth(s)
    parents = np.arange(s, N, 7 + s)[:370]                                   # ascending, as select_dividing lists them
    d["length"][torch.from_numpy(parents).cuda()] = dev(_rng(s, 66).uniform(2.0, 2.5, len(parents)))
    d["parent_of"] = dev(parents.astype(np.int32))
    return d


def m_aabb_pair(s):
    a = m_aabb(s)["aabb"]
    ref = a.clone()
    ref[(5 + 100 * s)::(900 + s), 4] += 0.3 * (1 - s)  # the real problem moved a corner, the decoy did not
    return dict(aabb=a, aabb_ref=ref)


case("select_dividing", m_growth, call_select_dividing, ["mhip_select_dividing"])
case("divide_grow_spherocylinders", m_divide_grow, call_divide_grow, ["mhip_divide_grow_spherocylinders"])
case("aabb_moved", m_aabb_pair, lambda live, ctx: O().aabb_moved(live["aabb"], live["aabb_ref"], 0.2), ["mhip_aabb_moved"])


# ---- broad phase --------------------------------------------------------------------------------------------------------------
def m_broadphase(s):
    o = _oracle()
    b = m_rods(s)
    rng = _rng(s, 70)
    aabb = o.compute_aabb_spherocylinders(b["center"], b["quat"], b["radius"], b["length"])
    brad = o.bounding_radius_spherocylinders(b["radius"], b["length"])
    moved = b["center"] + rng.normal(size=(N, 3)) * (0.001 + 0.2 * (1 - s))   # the real centres moved far, the decoy's not
    return D(aabb=aabb, center=b["center"], bounding_radius=brad, moved=moved, src=(rng.random(N) < 0.7).astype(np.uint8),
             tgt=(rng.random(N) < 0.7).astype(np.uint8), ex_ptr=np.arange(N + 1, dtype=np.int32),  # one excluded partner each
             ex_idx=rng.integers(0, N, N).astype(np.int32), ids=rng.permutation(N).astype(np.int64) + 10 ** 12,
             ranks=rng.integers(0, 4, N).astype(np.int32))


def call_broadphase(method, kind, periodic=None):
    def call(live, ctx):
        from mundy_amd import ops
        links = (ops.GenNeighborLinks().set_search_buffer(0.2).set_search_kind(kind).set_search_method(method)
                 .set_enforce_source_target_symmetry(True).set_periodic_box(periodic)
                 .acts_on(live["src"], live["tgt"]).concretize())
        try:
            links.set_excluded_partners(live["ex_ptr"], live["ex_idx"])
            links.set_identities(live["ids"], live["ranks"])
            links.generate(live["aabb"] if kind == ops.SEARCH_AABB else None, live["center"], live["bounding_radius"])
            out = dict(pairs=links.pairs, row_ptr=links.row_ptr, col=links.col, num_pairs=links.num_pairs,
                       method=links.method_used(), ident=links.ident_pairs(), coo=links.export_coo(first_link_id=5),
                       crs=links.export_crs(first_link_id=5, bucket_capacity=512),
                       rebuild=links.needs_rebuild(live["moved"]))
            return out
        finally:
            links.close()
    return call


BP_FNS = ["mhip_broadphase_set_sets", "mhip_broadphase_set_exclusions", "mhip_broadphase_set_identities",
          "mhip_broadphase_build", "mhip_broadphase_get_pairs", "mhip_broadphase_get_ident_pairs", "mhip_links_export_coo",
          "mhip_links_export_crs", "mhip_broadphase_needs_rebuild"]
for bp_name, bp_method in (("auto", 0), ("grid", 1), ("morton_lbvh", 2)):
    for bp_kind_name, bp_kind in (("spheres", 0), ("aabb", 1)):
        case("broadphase_%s_%s" % (bp_name, bp_kind_name), m_broadphase, call_broadphase(bp_method, bp_kind), BP_FNS)


def open_links(live):
    from mundy_amd import ops
    links = ops.GenNeighborLinks().set_search_buffer(0.2).set_search_kind(ops.SEARCH_AABB).concretize()
    links.generate(live["aabb"], live["center"], live["bounding_radius"])
    return links


def call_broadphase_reads(live, links):
    """what follows a build without a host scalar: the identities in, the lists and both exports out"""
    links.set_identities(live["ids"], live["ranks"])
    pairs = torch.empty((links.num_pairs, 2), dtype=torch.int32, device="cuda")
    row_ptr = torch.empty(N + 1, dtype=torch.int32, device="cuda")
    col = torch.empty(links.num_pairs, dtype=torch.int32, device="cuda")
    check(lib().mhip_broadphase_get_pairs(links._h, p(pairs), p(row_ptr), p(col), stream()))
    return pairs, row_ptr, col, links.ident_pairs(), links.export_coo(first_link_id=5), links.export_crs(first_link_id=5)


case("broadphase_reads", m_broadphase, call_broadphase_reads,
     ["mhip_broadphase_set_identities", "mhip_broadphase_get_pairs", "mhip_broadphase_get_ident_pairs",
      "mhip_links_export_coo", "mhip_links_export_crs"], open=open_links, close=lambda links: links.close())
case("broadphase_needs_rebuild", m_broadphase, lambda live, links: links.needs_rebuild(live["moved"]),
     ["mhip_broadphase_needs_rebuild"], open=open_links, close=lambda links: links.close())
case("broadphase_grid_periodic", m_broadphase, call_broadphase(1, 1, [BOX] * 3), BP_FNS)
case("broadphase_lbvh_triclinic", m_broadphase, call_broadphase(2, 0, CELL), BP_FNS)


# ---- solver vector primitives -------------------------------------------------------------------------------------------------
NV = 10007


def m_vectors(s):
    rng = _rng(s, 80)
    return D(x=rng.normal(size=NV), y=rng.normal(size=NV), x2=rng.normal(size=NV), y2=rng.normal(size=NV))


def call_deep_copy(live, ctx):
    check(lib().mhip_deep_copy(NV - 1, p(live["y"][1:]), p(live["x"][1:]), stream()))
    return live["y"]


def call_fill(live, ctx):
    check(lib().mhip_fill(NV - 2, p(live["y"][1:]), 2.5, stream()))
    return live["y"]


def call_axpby(live, ctx):
    from mundy_amd import ops
    ops.axpby(1.5, live["x"], -0.5, live["y"])
    ops.axpby(0.75, live["x2"][1:], 1e-17, live["y2"][1:])   # the 8-byte aligned path and a beta fast path
    return live["y"], live["y2"]


def call_wrapped(live, ctx):
    from mundy_amd import ops
    z = torch.empty_like(live["x"])
    ops.wrapped_axpbyz(1.0, live["x"], -0.5, live["y"], z, (3, -0.3, 0.3))
    return z


def call_sum(which):
    """one scalar reduction per case: the case blocks because of that entry point alone"""
    def call(live, ctx):
        from mundy_amd import ops
        x, y, x2, y2 = (live[k] for k in ("x", "y", "x2", "y2"))
        return {"diff_dot2": lambda: ops.diff_dot(x, y), "diff_dot4": lambda: ops.diff_dot(x, x2, y, y2),
                "residual_diff": lambda: ops.residual(0, x, y, (1, 0.0, 0.0)),
                "residual_gradient": lambda: ops.residual(1, x, y, (3, -0.5, 0.5)),
                "bb_step": lambda: ops.bb_step(x, y, x2, y2)}[which]()
    return call


case("deep_copy", m_vectors, call_deep_copy, ["mhip_deep_copy"])
case("fill", m_vectors, call_fill, ["mhip_fill"])
case("axpby", m_vectors, call_axpby, ["mhip_axpby"])
case("wrapped_axpbyz", m_vectors, call_wrapped, ["mhip_wrapped_axpbyz"])
for sum_name, sum_fn in (("diff_dot2", "mhip_diff_dot2"), ("diff_dot4", "mhip_diff_dot4"), ("residual_diff", "mhip_residual"),
                         ("residual_gradient", "mhip_residual"), ("bb_step", "mhip_bb_step")):
    case(sum_name, m_vectors, call_sum(sum_name), [sum_fn])


def m_dense(s):
    from test_oracle_convex_kat import random_lcp
    A, q, _ = random_lcp(200, seed=200 + s)
    return D(A=A, q=q, x0=np.full(200, 99.99))


def call_dense(cfg):
    def call(live, ctx):
        from mundy_amd import ops
        return ops.solve_lcp(live["A"], live["q"], live["x0"], ops.PGDConfig(**cfg))
    return call


case("gemv", m_dense, ops_call("gemv", "A", "q"), ["mhip_gemv"])
case("bbpgd_solve_dense_9", m_dense, call_dense(dict(max_iters=9, tol=1e-12)), ["mhip_bbpgd_solve_dense"])
case("bbpgd_solve_dense_tol", m_dense, call_dense(dict(max_iters=1000, tol=1e-6)), ["mhip_bbpgd_solve_dense"])


def m_small_batch(s):
    rng = _rng(s, 81)
    B = rng.uniform(-1, 1, (N, 4, 4))
    A = B @ B.transpose(0, 2, 1) + 4.0 * np.eye(4)
    return D(A=A, q=rng.normal(size=(N, 4)), x0=rng.uniform(0, 1, (N, 4)))


def call_small_batch(live, ctx):
    from mundy_amd import ops
    return ops.solve_small_cqpp_batch(live["A"], live["q"], (1, 0.0, 0.0), live["x0"], ops.PGDConfig(max_iters=200, tol=1e-8))


case("solve_small_cqpp_batch", m_small_batch, call_small_batch, ["mhip_solve_small_cqpp_batch"])


# ---- contact operator -----------------------------------------------------------------------------------------------------------
OP_ARRAYS = {"sphere": ("pairs", "normal", "mt"), "rod": ("pairs", "normal", "mt", "mr", "ra", "rb"),
             "rod_arclength": ("pairs", "normal", "mt", "mr", "s", "t", "seg")}


def m_op_arrays(maker):
    def make(s):
        P = problem(maker)
        # the decoy: the same pair list (its indices must stay in range and the incidence is what it is) with the rows of
        # every geometry array in another order, a valid operator of its own
        d = {k: (P[k] if k == "pairs" else shuffled(P[k], s, 90 + i)) for i, k in enumerate(OP_ARRAYS[maker])}
        d["x"] = _rng(s, 91).uniform(0, 1, len(P["pairs"]))
        return D(**d)
    return make


def call_op_create(maker):
    def call(live, ctx):
        op = new_op(problem(maker), live)
        try:
            return op.apply(live["x"]), op.body_velocity()
        finally:
            op.close()
    return call


def call_op_refresh(maker):
    def call(live, op):
        if maker == "rod_arclength":
            op.refresh(live["normal"], rod=(live["s"], live["t"], live["seg"]))
        else:
            op.refresh(live["normal"], ra=live.get("ra"), rb=live.get("rb"))
        return op.apply(live["x"])
    return call


for maker in ("sphere", "rod", "rod_arclength"):
    create = "mhip_contact_op_create_rods" if maker == "rod_arclength" else "mhip_contact_op_create"
    refresh = "mhip_contact_op_refresh_rods" if maker == "rod_arclength" else "mhip_contact_op_refresh"
    case("contact_op_create_%s" % maker, m_op_arrays(maker), call_op_create(maker), [create, "mhip_contact_op_apply"])
    case("contact_op_refresh_%s" % maker, m_op_arrays(maker), call_op_refresh(maker), [refresh, "mhip_contact_op_apply"],
         open=lambda live, maker=maker: new_op(problem(maker), live), close=lambda op: op.close())


def m_op_vectors(maker):
    def make(s):
        P = problem(maker)
        nc = len(P["pairs"])
        rng = _rng(s, 92)
        force = rng.normal(size=(nc, 3))
        force[::3] = 0.0
        return D(x=rng.uniform(0, 1, nc), force=force, velocity=rng.normal(size=(P["N"], 6)))
    return make


def call_op_sweeps(live, op):
    y = op.apply(live["x"])
    v_apply = op.body_velocity()
    op.body_sweep(live["x"])
    v_sweep = op.body_velocity()
    op.body_sweep_vector(live["force"])
    v_vector = op.body_velocity()
    return y, v_apply, v_sweep, v_vector, op.constraint_rate(live["velocity"])


for maker in ("sphere", "rod", "rod_arclength"):
    case("contact_op_sweeps_%s" % maker, m_op_vectors(maker), call_op_sweeps,
         ["mhip_contact_op_apply", "mhip_contact_op_body_sweep", "mhip_contact_op_body_sweep_vector",
          "mhip_contact_op_constraint_rate", "mhip_contact_op_body_velocity", "mhip_deep_copy"],
         open=lambda live, maker=maker: new_op(problem(maker)), close=lambda op: op.close())


# ---- solves -----------------------------------------------------------------------------------------------------------------------
CAPPED, TO_TOL = dict(max_iters=9, tol=1e-12), dict(max_iters=20000, tol=1e-6)


def m_sep(maker):
    def make(s):
        P = problem(maker)
        nc = len(P["pairs"])
        return D(sep=shuffled(P["sep"], s, 93), lam0=np.abs(np.sin(np.arange(nc) + s)) * 0.01)
    return make


def open_solver_op(maker, tiering=None, drift=None):
    def open_(live):
        op = new_op(problem(maker), cone=(maker == "cone"))
        if tiering is not None:
            op.set_tiering(tiering)
        if drift is not None:
            op.set_drift_source(drift)
        return op
    return open_


def call_solve(cfg, fused=True):
    def call(live, op):
        from mundy_amd import ops
        x, g, res = ops.solve_lcp(op, live["sep"], torch.zeros_like(live["sep"]), ops.PGDConfig(**cfg), fused=fused)
        return x, g, res, op.body_velocity(), (op.tier_stats()["tiered_iterations"] > 0 if fused else False)
    return call


for maker in ("sphere", "rod_arclength"):
    for tier, drift in ((3, 1), (3, 2), (0, 1)):
        for label, cfg in (("9", CAPPED), ("tol", TO_TOL)):
            case("bbpgd_solve_contact_%s_tier%d_drift%d_%s" % (maker, tier, drift, label), m_sep(maker), call_solve(cfg),
                 ["mhip_bbpgd_solve_contact"], open=open_solver_op(maker, tier, drift), close=lambda op: op.close())
for label, cfg in (("9", CAPPED), ("tol", TO_TOL)):
    case("bbpgd_solve_contact_rod_vector_%s" % label, m_sep("rod"), call_solve(cfg), ["mhip_bbpgd_solve_contact"],
         open=open_solver_op("rod"), close=lambda op: op.close())
    case("bbpgd_solve_contact_unfused_%s" % label, m_sep("sphere"), call_solve(cfg, fused=False),
         ["mhip_bbpgd_solve_contact_unfused"], open=open_solver_op("sphere"), close=lambda op: op.close())


def call_staged(cfg, pieces):
    """the staged entry points driven by hand on one rank (tests/test_gpu_convex.py); pieces: the constraint stage as two
    ranges and a reduce, with a snapshot of the active lists after every poll"""
    def call(live, op):
        from mundy_amd import capi, ops
        nc = live["sep"].shape[0]
        x, g, xt, gt = (torch.zeros(nc, dtype=torch.float64, device="cuda") for _ in range(4))
        local = torch.empty(5, dtype=torch.float64, device="cuda")
        sp, pc = capi.Space(ops.SPACE_LOWER_BOUND, 0.0, 0.0), capi.PgdConfig(cfg["max_iters"], cfg["tol"], 0)
        s = stream()
        check(lib().mhip_bbpgd_stage_begin(op._h, p(live["sep"]), C.byref(sp), C.byref(pc), p(x), p(g), p(xt), p(gt), s))
        res, done = capi.SolveResult(), C.c_int(0)
        it = 0
        while not done.value:
            for _ in range(8):  # a stretch of iterations between two polls
                init = 1 if it == 0 else 0
                check(lib().mhip_bbpgd_stage_body(op._h, init, s))
                if pieces:
                    half = nc // 2 + 3
                    check(lib().mhip_bbpgd_stage_constraint_range(op._h, init, 0, half, s))
                    check(lib().mhip_bbpgd_stage_constraint_range(op._h, init, half, nc - half, s))
                    check(lib().mhip_bbpgd_stage_reduce(op._h, init, p(local), s))
                else:
                    check(lib().mhip_bbpgd_stage_constraint(op._h, init, p(local), s))
                check(lib().mhip_bbpgd_stage_finalize(op._h, init, p(local), 1, s))
                it += 1
            check(lib().mhip_bbpgd_stage_poll(op._h, C.byref(res), C.byref(done), s))
            if pieces and not done.value:
                check(lib().mhip_bbpgd_stage_snapshot_active(op._h, s))
        check(lib().mhip_bbpgd_stage_end(op._h, C.byref(res), s))
        return x, g, int(res.num_iters), float(res.residual), bool(res.converged), op.body_velocity()
    return call


STAGE_FNS = ["mhip_bbpgd_stage_begin", "mhip_bbpgd_stage_body", "mhip_bbpgd_stage_constraint", "mhip_bbpgd_stage_finalize",
             "mhip_bbpgd_stage_poll", "mhip_bbpgd_stage_end"]
for label, cfg in (("9", CAPPED), ("tol", TO_TOL)):
    case("bbpgd_staged_%s" % label, m_sep("rod_arclength"), call_staged(cfg, False), STAGE_FNS,
         open=open_solver_op("rod_arclength"), close=lambda op: op.close())
    case("bbpgd_staged_pieces_%s" % label, m_sep("rod_arclength"), call_staged(cfg, True),
         STAGE_FNS + ["mhip_bbpgd_stage_constraint_range", "mhip_bbpgd_stage_reduce", "mhip_bbpgd_stage_snapshot_active"],
         open=open_solver_op("rod_arclength"), close=lambda op: op.close())


def call_friction(method, mu, cfg):
    def call(live, op):
        from mundy_amd import ops
        return ops.solve_friction_contact(op, live["sep"], mu, cfg=ops.PGDConfig(**cfg), method=method)
    return call


for method in ("bbpgd", "apgd"):
    for mu in (0.0, 0.3):
        for label, cfg in (("9", CAPPED), ("tol", dict(max_iters=50000, tol=1e-6))):
            case("%s_solve_contact_friction_mu%g_%s" % (method, mu, label), m_sep("cone"), call_friction(method, mu, cfg),
                 ["mhip_%s_solve_contact_friction" % method], open=open_solver_op("cone"), close=lambda op: op.close())


def call_scrap(cap):
    def call(live, op):
        from mundy_amd import ops
        lam, g, r = ops.resolve_collisions(op, live["sep"], live["lam0"], 1.0, max_allowable_overlap=1e-5,
                                           max_col_iterations=cap)
        return lam, g, r
    return call


for maker in ("sphere", "rod", "rod_arclength"):
    for label, cap in (("9", 9), ("tol", 10000)):
        case("scrap_bbpgd_solve_contact_%s_%s" % (maker, label), m_sep(maker), call_scrap(cap),
             ["mhip_scrap_bbpgd_solve_contact"], open=open_solver_op(maker), close=lambda op: op.close())


# ---- runtime: the copies and the synchronisation -------------------------------------------------------------------------------
def call_memcpy_h2d(live, ctx):
    """a host array into all of a live buffer but its first element, which stays what the producer delivered"""
    y = live["y"]
    host_in = np.arange(NV - 1, dtype=np.float64) * 0.5
    check(lib().mhip_memcpy_h2d(p(y[1:]), host_in.ctypes.data_as(C.c_void_p), 8 * (NV - 1), stream()))
    return y


def call_memcpy_d2h(live, ctx):
    """a d2h behind the delayed producer returns the real data, not the decoy"""
    back = np.empty(NV)
    check(lib().mhip_memcpy_d2h(back.ctypes.data_as(C.c_void_p), p(live["x"]), 8 * NV, stream()))
    return torch.from_numpy(back)


def call_stream_synchronize(live, ctx):
    """an asynchronous library kernel, then the synchronisation: the stream has drained when it returns"""
    s = stream()
    check(lib().mhip_axpby(NV, 1.0, p(live["x"]), 2.0, p(live["y"]), s))
    check(lib().mhip_stream_synchronize(s))
    return bool(torch.cuda.current_stream().query()), live["y"]


case("memcpy_h2d", m_vectors, call_memcpy_h2d, ["mhip_memcpy_h2d"])
case("memcpy_d2h", m_vectors, call_memcpy_d2h, ["mhip_memcpy_d2h"])
case("stream_synchronize", m_vectors, call_stream_synchronize, ["mhip_axpby", "mhip_stream_synchronize"])


# ---- the parametrised test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    """the side stream, its calibrated delay, and the recorder in front of the library"""
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    su.CALLED.clear()
    su.REPORT["cases"].clear()
    su.recording_library(mp)
    side = torch.cuda.Stream()
    cycles_per_ms = su.calibrate(side)
    ran = set()
    try:
        yield dict(side=side, cycles_per_ms=cycles_per_ms, ran=ran)
    finally:
        mp.undo()
        print("\nstream harness: %.0f sleep cycles per ms, longest delay %.0f ms, %d cases, %d entry points called" % (
            cycles_per_ms, su.REPORT["longest_delay_ms"], len(ran), len(su.CALLED)))


@gpu
def test_canary_a_side_stream_does_not_wait_for_the_null_stream_and_back(rig):
    # the instrument itself: real -> x behind a sleep on the side stream, a clone of x on the null stream meanwhile.  The
    # clone must hold the decoy; if it holds the real data, side streams block against the null stream on this runtime
    # and every other test of this file is blind.
    side = rig["side"]
    real, decoy = dev(np.arange(4096, dtype=np.float64)), dev(-np.arange(4096, dtype=np.float64) - 1.0)
    x = decoy.clone()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        torch.cuda._sleep(int(su.MIN_DELAY_MS * rig["cycles_per_ms"]))
        x.copy_(real)
    y = x.clone()  # the null stream
    early = not side.query()
    torch.cuda.current_stream().synchronize()
    side.synchronize()
    assert early, "the sleep had ended before the null stream's clone was issued: the delay is too short to tell"
    assert torch.equal(y, decoy), "the null stream waited for the side stream: this runtime serialises them"
    assert torch.equal(x, real)
    rig["canary"] = True


@gpu
@pytest.mark.parametrize("case_", CASES, ids=[c.name for c in CASES])
def test_entry_point_on_a_side_stream(rig, case_):
    assert rig.get("canary"), "the canary did not pass (or did not run): the side stream is not proven non-blocking"
    with su.stop_on_device_fault():
        su.run_on_side_stream(case_, rig["side"], rig["cycles_per_ms"], synchronises=may_block(case_))
    rig["ran"].add(case_.name)


# ---- ContactStepper: construct and step entirely on the side stream ---------------------------------------------------------------
def stepper_sphere_lcp():
    from mundy_amd import ops, pipeline, synth
    b = synth.spheres(N, volume_fraction=0.3, seed=11)
    return pipeline.ContactStepper("sphere", dev(b["center"]), dev(b["radius"]), search_buffer=0.3,
                                   cfg=ops.PGDConfig(max_iters=2000, tol=1e-6))


def stepper_rods_friction():
    from mundy_amd import pipeline, synth
    b = synth.spherocylinders(2000, seed=12)
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]), dev(b["length"]),
                                 search_buffer=0.1, contact_model="hertz", hertz_friction=0.3, dt=1e-4)
    return st


def stepper_chain():
    from mundy_amd import pipeline
    d = chain()
    n = d["center0"].shape[0]
    xp = dict(k=3.0, r=1.0, bind_rate=200.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5, skin=0.5)
    return pipeline.ContactStepper("sphere", dev(d["center0"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                   search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                   brownian_kt=d["kt"], hydrodynamics=dict(kind="rpyc", update_every=2),
                                   crosslinkers=dict(left=np.arange(0, n, 2), sites=(np.arange(n) % 3 != 0).astype(np.uint8),
                                                     kind="hookean", **xp))


def stepper_mixed():
    from mundy_amd import ops, pipeline, synth
    b = synth.mixed_bodies(2001, seed=13)
    return pipeline.ContactStepper("mixed", dev(b["center"]), None, dev(b["quat"]), search_buffer=0.1,
                                   cfg=ops.PGDConfig(max_iters=2000, tol=1e-6), kinds=dev(b["kind"]), shape=dev(b["shape"]))


def _stepper_outputs(st, s):
    out = dict(center=st.center, aabb=st.aabb, pairs=st.contact_pairs, lam=st.lam, num_iters=int(s.num_iters),
               num_contacts=int(s.num_contacts), residual=float(s.residual), converged=bool(s.converged),
               rebuilt=bool(s.rebuilt), max_overlap=float(s.max_overlap), velocity=st.op.body_velocity())
    if st.quat is not None:
        out["quat"] = st.quat
    for k in ("sep", "normal", "ra", "rb", "s", "t"):
        if st.contacts.get(k) is not None:
            out["contact_" + k] = st.contacts[k]
    for k in ("u_ext", "spring_force", "u_hydro", "tang_disp", "contact_force", "prev_velocity", "grad", "q"):
        if isinstance(getattr(st, k, None), torch.Tensor):
            out[k] = getattr(st, k)
    if getattr(st, "crosslinkers", None) is not None:
        out["crosslinker_state"] = st.crosslinker_state()
        out["crosslinker_counts"] = (int(s.crosslinker_bound), int(s.crosslinker_binds), int(s.crosslinker_unbinds))
    return su._flatten(out)


STEPS = 5


@gpu
@pytest.mark.parametrize("make", [stepper_sphere_lcp, stepper_rods_friction, stepper_chain, stepper_mixed],
                         ids=["sphere_lcp", "rods_frictional_hertz", "chain_springs_noise_rpyc_crosslinkers", "mixed"])
def test_contact_stepper_on_a_side_stream(rig, make):
    # the stepper built and stepped five times under the side stream against a null-stream run.  In front of every step:
    # the state of ANOTHER step in the per-body arrays (a valid decoy), then a sleep and the restoration of this step's
    # state from the null-stream run's snapshot, on the side stream.
    assert rig.get("canary"), "the canary did not pass (or did not run): the side stream is not proven non-blocking"
    with su.stop_on_device_fault():
        _stepper_on_a_side_stream(rig, make)


def _stepper_on_a_side_stream(rig, make):
    side, cycles = rig["side"], int(su.MIN_DELAY_MS * rig["cycles_per_ms"])
    st = make()
    snaps, ref = [], []
    for k in range(STEPS):
        snaps.append(st.snapshot())
        st.restore(snaps[k])
        s = st.step()
        ref.append(su.freeze(_stepper_outputs(st, s)))
    torch.cuda.synchronize()
    assert su.differing(ref[0], ref[1]), "the steps do not differ: a stale state would pass"
    with su.recorded(), torch.cuda.stream(side):
        st2 = make()
        for k in range(STEPS):
            decoy = snaps[(k + 2) % STEPS]
            for name in ("center", "quat"):
                if isinstance(getattr(st2, name, None), torch.Tensor):
                    getattr(st2, name).copy_(decoy[name])
            side.synchronize()
            torch.cuda._sleep(cycles)
            st2.restore(snaps[k])
            s = st2.step()
            got = su._clone(_stepper_outputs(st2, s))
            side.synchronize()
            su.assert_same(su.freeze(got), ref[k], "%s, step %d" % (make.__name__, k))
        side.synchronize()


# ---- the scratch of the handle-free entry points between two streams ----------------------------------------------------------------
HAND_OVER = ["morton_order", "curve_order", "curve_keys", "sort_by_key_u64", "distance_ellipsoid_ellipsoid_5000",
             "distance_point_ellipsoid_5000", "contact_ellipsoids_5000", "contact_mixed", "contact_mixed_periodic",
             "contact_history_carry_renumbered"]


@gpu
@pytest.mark.parametrize("name", HAND_OVER)
def test_scratch_hand_over(rig, name):
    # X on stream A behind a sleep, then X with other inputs on stream B from the same host thread.  Both use the same
    # thread-local scratch (csrc/scratch_owner.hpp): B's call must wait for A's, so when B has drained A has too, and
    # both results are the null-stream ones.  (With the claim removed B would run at once, on A's histogram / keys /
    # counters / board: the order of completion shows it without letting the kernels collide on purpose -- the test is
    # only ever run with the claim in place.)
    assert rig.get("canary"), "the canary did not pass (or did not run): the side stream is not proven non-blocking"
    with su.stop_on_device_fault():
        _scratch_hand_over(rig, name)


def _scratch_hand_over(rig, name):
    import time
    case_ = {c.name: c for c in CASES}[name]
    assert case_.open is None
    a_in, b_in = case_.make(0), case_.make(1)
    torch.cuda.synchronize()
    ref_a, ref_b = su._run(case_, a_in), su._run(case_, b_in)
    A, B = rig["side"], torch.cuda.Stream()
    for s_, inputs in ((A, a_in), (B, b_in)):  # warm both streams' allocator pools; the scratch has its size already
        with torch.cuda.stream(s_):
            case_.call({k: v.clone() for k, v in inputs.items()}, None)
            s_.synchronize()
    la, lb = ({k: v.clone() for k, v in d.items()} for d in (a_in, b_in))
    torch.cuda.synchronize()
    with torch.cuda.stream(A):
        torch.cuda._sleep(int(su.MIN_DELAY_MS * rig["cycles_per_ms"]))
        out_a = case_.call(la, None)
        a_busy = not A.query()
        got_a = su._clone(su._flatten(out_a))
    with torch.cuda.stream(B):
        out_b = case_.call(lb, None)
        got_b = su._clone(su._flatten(out_b))
    assert not may_block(case_), "a call that blocks has drained stream A before B's call is made: the case is blind"
    assert a_busy, "stream A had drained before B's call was made: the delay is too short to tell"
    deadline = time.perf_counter() + 20.0
    while not B.query():
        assert time.perf_counter() < deadline, "stream B never drained"
    a_done_when_b_done = A.query()
    A.synchronize()
    B.synchronize()
    assert a_done_when_b_done, "%s on stream B finished while the same thread's call on stream A was still running" % name
    su.assert_same(su.freeze(got_a), ref_a, name + " on stream A")
    su.assert_same(su.freeze(got_b), ref_b, name + " on stream B")


def _ellipsoid_writer(live):
    O().distance_ellipsoid_ellipsoid(*[live[k] for k in ("c1", "q1", "r1", "c2", "q2", "r2")])


def _mixed_writer(live):
    call_mixed(route=True)(live, None)


READERS = {"ellipsoid_last_evaluations": (m_ee(5000), _ellipsoid_writer, lambda: O().ellipsoid_last_evaluations()),
           "contact_mixed_last_evaluations": (m_mixed_pairs, _mixed_writer, lambda: O().contact_mixed_last_evaluations())}


@gpu
@pytest.mark.parametrize("name", sorted(READERS))
def test_scratch_hand_over_to_a_reader(rig, name):
    # the *_last_evaluations readers block, so the test above cannot see their claim.  Here the scratch holds the
    # DECOY's counters; the asynchronous call on the real inputs goes on stream A behind a sleep; the reader is called on
    # stream B from the same thread.  It must wait for A -- A has drained when it returns -- and return the count of the
    # real inputs.  Without the reader's claim it returns at once with the decoy's count.
    assert rig.get("canary"), "the canary did not pass (or did not run): the side stream is not proven non-blocking"
    with su.stop_on_device_fault():
        make, write, read = READERS[name]
        real, decoy = make(0), make(1)
        torch.cuda.synchronize()
        write(real)
        want = read()
        write(decoy)
        other = read()
        assert want != other, "the decoy needs as many evaluations as the real problem: the case is blind"
        A, B = rig["side"], torch.cuda.Stream()
        with torch.cuda.stream(A):  # (also the warm call of A's allocator pool)
            write(decoy)
            A.synchronize()
        with torch.cuda.stream(A):
            torch.cuda._sleep(int(su.MIN_DELAY_MS * rig["cycles_per_ms"]))
            write(real)
            a_busy = not A.query()
        with torch.cuda.stream(B):
            got = read()
            a_done = A.query()
        A.synchronize()
        B.synchronize()
        assert a_busy, "stream A had drained before the reader was called: the delay is too short to tell"
        assert a_done, "%s on stream B returned while the call it reads from was still running on stream A" % name
        assert got == want, (got, want, other)


# ---- coverage: measured, not declared ------------------------------------------------------------------------------------------------
@gpu
def test_every_stream_entry_point_was_called(rig):
    assert len(rig["ran"]) == len(CASES), "only %d of %d cases ran in this session: the count needs the whole module" % (
        len(rig["ran"]), len(CASES))
    missing = sorted(n for n in stream_prototypes() if n not in su.CALLED and n not in EXEMPT)
    assert not missing, "stream-taking entry points no case called and EXEMPT does not list: %s" % missing
    listed = sorted(f for c in CASES for f in c.fns if f not in su.CALLED)
    assert not listed, "entry points a case lists but did not call: %s" % listed
