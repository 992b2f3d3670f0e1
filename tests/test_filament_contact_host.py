"""CPU-side checks of the colliding filaments' contact stage: known answers of the numpy model
(filament_contact_model.py) in dyadic inputs, the contact-point velocity, the balance of the node forces, who pairs with
whom, the refusals of ops, of the stepper and of the library (before any HIP call), and the new entry points."""
import ctypes as C
import math

import numpy as np
import pytest

import filament_contact_model as fcm
import filament_model as fm
import friction_hertz_model as fh
from gpu_util import all_pos_zero

U = 2.0 ** -53   # unit roundoff
MATERIAL = dict(youngs_modulus=1024.0, poisson_ratio=0.25, mu=0.5)


def filaments(node_ptr, center, radius, **prm):
    n = len(center)
    f = fm.Filaments(node_ptr, np.broadcast_to(np.asarray(radius, np.float64), (n,)).copy(), np.zeros((n, 3)),
                     np.zeros(n), params=fm.Params(**prm))
    q = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    return f.set_state(np.asarray(center, np.float64), np.zeros(n), q)


def crossing(z_top, y_first):
    """filament 0 along z through (0, 0, -1), (0, 0, 1), (0, 0, 3); filament 1 along y at x = 1, z = z_top, its first node
    at y = y_first; both of radius 5/8 and segment length 2: segments 0 and 3 touch with an overlap of 1/4, the normal
    is (1, 0, 0) exactly and nothing else touches"""
    c = [[0.0, 0.0, -1.0], [0.0, 0.0, 1.0], [0.0, 0.0, 3.0],
         [1.0, y_first, z_top], [1.0, y_first + 2.0, z_top], [1.0, y_first + 4.0, z_top]]
    f = filaments([0, 3, 6], c, 0.625)
    k = fcm.Contacts(f, skin=0.5, **MATERIAL)
    assert k.update()
    return k


def hertz_force(r=0.625, overlap=0.25):
    kn, _ = fh.spring_coefficients(*(np.float64(v) for v in (1024.0, 1024.0, 0.25, 0.25)))
    Rs = (r * r) / (r + r)
    return math.sqrt(Rs * overlap) * (kn * overlap)   # sqrt(R* delta) k_n delta


# ---- known answers ------------------------------------------------------------------------------------------------------
def test_midpoint_over_midpoint_splits_the_hertz_force_in_halves(oracle):
    k = crossing(z_top=0.0, y_first=-1.0)
    assert k.pairs.tolist() == [[0, 3], [0, 4], [1, 3], [1, 4]]
    stats = k.force_pass(0.01)
    F = hertz_force()
    assert stats == (0.25, 0) and F > 0.0
    assert k.sep[0] == -0.25 and (k.sep[1:] > 0.125).all()   # the others: sqrt(2) - 5/4 twice, sqrt(3) - 5/4
    assert np.array_equal(k.force[0], [-F, 0.0, 0.0]) and all_pos_zero(k.force[1:]) and all_pos_zero(k.tang_disp)
    # the left segment is pushed along -n, the right one along +n; each end node takes exactly half
    want = np.zeros((6, 3))
    want[[0, 1], 0] = -(F / 2.0)
    want[[3, 4], 0] = F / 2.0
    assert np.array_equal(k.node_force, want)
    assert all_pos_zero(k.node_force[[2, 5]])


def test_quarter_point_shares_three_quarters_and_one_quarter(oracle):
    k = crossing(z_top=-0.5, y_first=-0.5)
    k.force_pass(0.01)
    F = hertz_force()
    assert np.array_equal(k.sep[:1], [-0.25]) and (k.sep[1:] > 0.0).all()
    assert np.array_equal(k.share[0], [[-(0.25 * F), 0.0, 0.0], [0.25 * F, 0.0, 0.0]])
    want = np.zeros((6, 3))
    want[0, 0], want[1, 0] = -(F - 0.25 * F), -(0.25 * F)
    want[3, 0], want[4, 0] = F - 0.25 * F, 0.25 * F
    assert np.array_equal(k.node_force, want)
    assert F - 0.25 * F == 0.75 * F
    # an external force comes first: (external + a0[i]) + a1[i - 1]
    ext = np.full((6, 3), 0.5)
    k.force_pass(0.01, ext)
    assert np.array_equal(k.node_force, ext + want)


def test_contact_point_velocity(oracle):
    rng = np.random.default_rng(3)
    x0, x1 = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    v0, v1 = rng.normal(size=(50, 3)), rng.normal(size=(50, 3))
    # at the left end node lc = 0: exactly that node's velocity
    assert np.array_equal(fcm.point_velocity(x0, x1, v0, v1, x0), v0)
    # at the right end node: v1 up to the roundings of the two terms (each a few u |v1 - v0|)
    got = fcm.point_velocity(x0, x1, v0, v1, x1)
    assert np.abs(got - v1).max() <= 16.0 * U * np.abs(v1 - v0).max()
    # a rigidly translating segment: rv = 0, both terms vanish, at the midpoint and anywhere else
    mid = 0.5 * (x0 + x1)
    assert np.array_equal(fcm.point_velocity(x0, x1, v0, v0, mid), v0)
    # a segment turning about its left end with angular velocity w: v_cp = w x lc for a point on the centreline
    w = rng.normal(size=(50, 3))
    s = rng.uniform(0.0, 1.0, (50, 1))
    cp = x0 + s * (x1 - x0)
    got = fcm.point_velocity(x0, x1, np.zeros((50, 3)), np.cross(w, x1 - x0), cp)
    assert np.abs(got - np.cross(w, cp - x0)).max() < 1e-13


def random_case(rng, moving):
    from mundy_amd import synth
    d = synth.crossed_filaments(5, 7, radius=0.5, segment_length=1.0, angle=1.1, overlap=0.2)
    n = len(d["radius"])
    center = d["center"] + rng.uniform(-0.05, 0.05, (n, 3))
    f = filaments(d["node_ptr"], center, rng.uniform(0.45, 0.55, n))
    if moving:
        f.velocity = rng.normal(size=(n, 3))
    k = fcm.Contacts(f, skin=0.5, damping=(0.3, 0.2), **MATERIAL)
    k.save_velocity()
    k.update()
    if moving:
        k.set_history(k.pairs, rng.normal(scale=1e-3, size=(len(k.pairs), 3)))
    k.force_pass(0.01)
    return f, k


def _entry_totals(k):
    """sum over the list's entries of |Fs - share| + |share| per component, and the longest incidence row"""
    Fs = np.stack([k.force, -k.force], axis=1)
    total = (np.abs(Fs - k.share) + np.abs(k.share)).sum(axis=(0, 1))
    return total, int(np.bincount(k.pairs.reshape(-1)).max())


def test_node_forces_sum_to_zero(oracle):
    f, k = random_case(np.random.default_rng(17), moving=True)
    assert (k.sep <= 0.0).sum() >= 10 and k.stats[1] > 0 and np.abs(k.tang_disp).max() > 0.0
    # A linker puts Fs - share and share on one segment's end nodes and the same with -F on the other's.  (Fs - share) +
    # share differs from Fs by the one rounding of the subtraction; a segment with K entries adds each of its two sums in
    # K roundings, and a node adds its two sums in 2 more: K + 3 roundings, each below u (1 + (K + 3) u) times the sum of
    # the magnitudes entering.  With T = sum over all entries of |Fs - share| + |share|: |sum F| <= (K + 3) u (1 + ..) T.
    total, K = _entry_totals(k)
    bound = (K + 3) * U * (1.0 + (K + 3) * U) * total
    got = np.array([math.fsum(k.node_force[:, c]) for c in range(3)])
    assert (np.abs(got) <= bound).all() and (total > 0.0).all(), (got, bound)


def test_node_forces_have_no_net_torque_without_friction(oracle):
    # Zero velocities and zero history: rel = 0 exactly, F = F_n along n.  (With a tangential force the pair has the
    # torque (cp_i - cp_j) x F_t: the reference applies it at the two centreline points, which are a distance apart.)
    f, k = random_case(np.random.default_rng(18), moving=False)
    hit = k.sep <= 0.0
    assert hit.sum() >= 10 and k.stats[1] == 0
    x, F = f.center, k.node_force
    tor = np.array([math.fsum(x[:, 1] * F[:, 2]) - math.fsum(x[:, 2] * F[:, 1]),
                    math.fsum(x[:, 2] * F[:, 0]) - math.fsum(x[:, 0] * F[:, 2]),
                    math.fsum(x[:, 0] * F[:, 1]) - math.fsum(x[:, 1] * F[:, 0])])
    # In exact arithmetic a side's two node forces have the torque cp x Fs (for cp on the centreline the two tangential
    # pieces of `share` cancel and share = (a / L) Fs), and cp_i x F - cp_j x F = (cp_i - cp_j) x F = 0 for F along the
    # normal.  In doubles: the contact points (3 roundings a component), lc, t, the two dots, the terms of share (10),
    # the normal (2), Fs - share, the segment sums (K) and the node sum (2) -- fewer than 32 + K roundings per side, each
    # moving a force of size |F| by at most u |F| at a lever below R = max |x| + the segment length.
    _, K = _entry_totals(k)
    R = np.abs(x).max() * math.sqrt(3.0) + 1.2
    bound = 2.0 * (32 + K) * U * R * np.sqrt((k.force[hit] ** 2).sum(axis=1)).sum()
    assert (np.abs(tor) <= bound).all(), (tor, bound)
    assert np.abs(F).max() > 1.0


# ---- who pairs with whom ------------------------------------------------------------------------------------------------
def test_neighbours_never_pair_and_second_neighbours_do(oracle):
    c = np.zeros((5, 3))
    c[:, 2] = np.arange(5)
    f = filaments([0, 5], c, 0.5)
    k = fcm.Contacts(f, skin=0.25, **MATERIAL)
    k.update()
    # boxes of segments two apart meet (z: [i - 0.75, i + 1.75]), three apart do not
    assert k.pairs.tolist() == [[0, 2], [1, 3]]
    k2 = fcm.Contacts(f, skin=0.25, bonded_exclusion=2, **MATERIAL)
    k2.update()
    assert k2.pairs.shape == (0, 2)
    k2.force_pass(0.01)
    assert all_pos_zero(k2.node_force) and k2.stats == (0.0, 0)


def test_the_last_nodes_segment_never_pairs(oracle):
    # two 2-node filaments side by side: rows 1 and 3 are degenerate records inside the other filament's box
    c = [[0.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.75, 0.0, 0.0], [0.75, 0.0, 1.0]]
    f = filaments([0, 2, 4], c, 0.5)
    k = fcm.Contacts(f, skin=0.5, **MATERIAL)
    k.update()
    assert k.pairs.tolist() == [[0, 2]]
    assert np.array_equal(k.seg[1], [0.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.5, 0.0])
    assert np.array_equal(k.aabb[1], [-1.0, -1.0, 0.0, 1.0, 1.0, 2.0])
    from mundy_amd import synth
    d = synth.crossed_filaments(3, 4, overlap=0.125)
    g = filaments(d["node_ptr"], d["center"], d["radius"])
    kk = fcm.Contacts(g, skin=1.0, **MATERIAL)
    kk.update()
    last = d["node_ptr"][1:] - 1
    assert len(kk.pairs) > 9 and not np.isin(kk.pairs, last).any()
    fid = np.repeat(np.arange(6), 4)
    same = fid[kk.pairs[:, 0]] == fid[kk.pairs[:, 1]]
    assert (np.diff(kk.pairs[same], axis=1) > 1).all()


def test_monolayer_zeroes_the_saved_velocity_component(oracle):
    c = np.zeros((3, 3))
    c[:, 2] = np.arange(3)
    for mono in (False, True):
        f = filaments([0, 3], c, 0.5, monolayer=mono)
        f.velocity = np.full((3, 3), -2.0)
        k = fcm.Contacts(f, skin=0.25, **MATERIAL)
        k.save_velocity()
        assert np.array_equal(k.velocity_prev[:, 1:], np.full((3, 2), -2.0))
        assert all_pos_zero(k.velocity_prev[:, 0]) if mono else np.array_equal(k.velocity_prev[:, 0], [-2.0] * 3)


# ---- refusals, before any HIP call --------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


GOOD = dict(skin=0.5, youngs_modulus=1000.0, poisson_ratio=0.3, mu=0.5)
BAD = [(dict(skin=-1.0), "skin"), (dict(skin=float("nan")), "skin"), (dict(youngs_modulus=0.0), "youngs_modulus"),
       (dict(poisson_ratio=1.0), "poisson_ratio"), (dict(poisson_ratio=0.0), "poisson_ratio"), (dict(mu=-0.5), "mu"),
       (dict(mu=float("inf")), "mu"), (dict(damping=(-1.0, 0.0)), "damping"), (dict(damping=(0.0, float("nan"))), "damping"),
       (dict(density=-1.0), "density"), (dict(bonded_exclusion=0), "bonded_exclusion")]


@pytest.mark.parametrize("change, match", BAD + [
    (dict(history_dt=float("inf")), "history_dt"), (dict(damping=0.5), "damping"),
    (dict(segment_radius=np.array([1.0, 0.0, 1.0, 1.0])), "radius"), (dict(segment_radius=np.ones(3)), "shape"),
    (dict(bonded_exclusion=1.5), "bonded_exclusion")])
def test_ops_and_stepper_refuse_bad_contacts(change, match):
    from mundy_amd import ops, pipeline
    args = dict(GOOD)
    args.update(change)
    with pytest.raises(ValueError, match=match):
        ops.check_filament_contacts(4, **args)
    c = np.zeros((4, 3))
    c[:, 2] = np.arange(4)
    with pytest.raises(ValueError, match=match):   # before the filaments are built: no library call
        pipeline.FilamentStepper([0, 4], c, np.ones(4), np.zeros((4, 4)), np.arange(4) * 1.0, youngs_modulus=10.0,
                                 rest_length=1.0, viscosity=1.0, contacts=args)
    prm, r = ops.check_filament_contacts(4, **GOOD)
    assert prm.history_dt == -1.0 and prm.bonded_exclusion == 1 and r is None


def test_stepper_refuses_a_malformed_contacts_dict():
    from mundy_amd import pipeline
    c = np.zeros((4, 3))
    for spec, match in ((dict(skin=0.5), "missing key"), (dict(GOOD, friction=1.0), "unknown key"), (3.0, "must be a dict")):
        with pytest.raises(ValueError, match=match):
            pipeline.FilamentStepper([0, 4], c, np.ones(4), np.zeros((4, 4)), np.arange(4) * 1.0, youngs_modulus=10.0,
                                     rest_length=1.0, viscosity=1.0, contacts=spec)


def test_library_refuses_before_any_hip_call(lib):
    from mundy_amd import capi
    ptr = np.array([0, 4], dtype=np.int32)

    def create(handle=True, params=True, **over):
        v = dict(skin=0.5, E=1000.0, nu=0.3, mu=0.5, gn=0.0, gt=0.0, rho=1.0, hdt=-1.0, bonded=1)
        v.update(over)
        prm = capi.FilamentContactParams(v["skin"], v["E"], v["nu"], v["mu"], v["gn"], v["gt"], v["rho"], v["hdt"],
                                         v["bonded"], 0)
        h = C.c_void_p()
        # no filaments handle: every refusal below comes before it is looked at
        capi.check(lib.mhip_filament_contacts_create(C.byref(h) if handle else None, None, ptr.ctypes.data_as(C.c_void_p),
                                                     None, C.byref(prm) if params else None, None))

    for kwargs, match in ((dict(handle=False), "handle is null"), (dict(params=False), "params is null"),
                          (dict(skin=-0.5), "skin"), (dict(E=0.0), "youngs_modulus"), (dict(nu=1.5), "poisson_ratio"),
                          (dict(mu=-1.0), "mu"), (dict(gn=-1.0), "damping"), (dict(gt=float("nan")), "damping"),
                          (dict(rho=-1.0), "density"), (dict(hdt=float("nan")), "history_dt"),
                          (dict(bonded=0), "bonded_exclusion"), (dict(), "filaments handle is null")):
        with pytest.raises(ValueError, match=match):
            create(**kwargs)
    fields, flag = capi.FilamentContactFields(), C.c_int(0)
    for call in (lambda: lib.mhip_filament_contacts_save_velocity(None),
                 lambda: lib.mhip_filament_contacts_update(None, C.byref(flag)),
                 lambda: lib.mhip_filament_contacts_force(None, 0.1, None, None),
                 lambda: lib.mhip_filament_contacts_segment_view(None),
                 lambda: lib.mhip_filament_contacts_linker_pass(None, 0.1, None),
                 lambda: lib.mhip_filament_contacts_reduce(None, None),
                 lambda: lib.mhip_filament_contacts_set_history(None, 0, None, None),
                 lambda: lib.mhip_filament_contacts_get(None, C.byref(fields))):
        with pytest.raises(ValueError, match="handle is null"):
            capi.check(call())
    assert lib.mhip_filament_contacts_destroy(None) == 0


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    names = ["mhip_filament_contacts_" + s for s in ("create", "save_velocity", "update", "force", "segment_view",
                                                       "linker_pass", "reduce", "set_history", "get", "destroy")]
    header = open(capi.LIB_PATH.replace("mundy_amd/lib/libmundy_hip.so", "include/mundy_hip.h")).read()
    for name in names:
        assert hasattr(lib, name) and name in capi.SIGNATURES and name + "(" in header
    assert C.sizeof(capi.FilamentContactParams) == 8 * 8 + 2 * 4
    assert C.sizeof(capi.FilamentContactFields) == 2 * 8 + len(capi.FILAMENT_CONTACT_FIELDS) * 8
    assert list(capi.FILAMENT_CONTACT_FIELDS) == ["pairs", "sep", "tang_disp", "force", "share", "node_force", "seg",
                                                  "aabb", "velocity_prev"]
