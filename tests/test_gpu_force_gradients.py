"""Every soft-force kernel of the chain step against the negative gradient of its energy (tests/potentials.py), and the
composed step against the energy it must lower.

The parity tests hold each kernel to a numpy model that was written from the same text as the kernel.  These hold it to
the physics: for every body b and component k
        |F_dev[b, k] - (-dU/dx_bk)| <= K eps S_b
with -grad U from mpmath (central differences at 50 digits), S_b the sum of the magnitudes of the terms acting on b and K
the term's entry of the table in tests/test_potentials_host.py, which that module measures from the model and the exact
gradient and never from the device.  The configurations are tests/gradient_cases.py's: 24 to 51 bodies, every member
1e-3 or more from a branch boundary, members on both sides, and an out-of-branch member contributes exactly zero.
  A  force = -grad U, term by term
  B  momentum and angular momentum of the pair terms
  C  rigid-motion equivariance: the configuration rotated and translated, wall included, gives Q F
  D  the composed step lowers U by dt F.v, to the first order of the explicit Euler step
The filament family (filament.hip, filament_contact.hip) against the discrete rod energy, on tests/filament_cases.py:
  E  first evaluation, wave off and on: F = -grad E and tau = -dE/dtheta
  F  after the nodes moved: tau = -dE/dtheta, F = -grad E + R, R the reference's stray binormal term and nothing else
  G  momentum per filament        H  rigid-motion equivariance through set_state, force, velocity, advance, force
  I  FilamentStepper with the twist off lowers E by dt F.v
  J  segment contacts: frictionless = -grad of the pair Hertz energy; with friction, momentum and the contact couple"""
import math

import numpy as np
import pytest

import gradient_cases as gc
import potentials as P
from gpu_util import all_pos_zero, dev, host

gpu = pytest.mark.gpu
EPS = gc.EPS
PAIR_NAMES = tuple(n for n in gc.NAMES if n.startswith(("springs", "active", "hertz", "segments")) or
                   n in ("crosslinkers_hookean", "crosslinkers_fene"))


def O():
    from mundy_amd import ops
    return ops


def _device(case, x=None, fixed=None):
    return case.device(O(), dev, host, case.x if x is None else x, case.fixed if fixed is None else fixed)


# ---- A. force = -grad U ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", gc.NAMES)
def test_force_is_minus_the_gradient_of_the_energy(name):
    case = gc.cases()[name]
    case.check()
    F = _device(case)
    exact, S = gc.exact(name)
    d = gc.deviation(F, exact, S)
    K = gc.TOLERANCE_K[case.group]
    print("%s: worst deviation %.3g eps S_b (K = %g)" % (name, d.max(), K))
    assert (d <= K).all(), (name, int(np.argmax(d)), float(d.max()))
    assert (S > 0).sum() >= 8
    # an out-of-branch member contributes exactly zero
    if hasattr(case, "zero_rows"):
        rows = case.zero_rows()
        assert len(rows) >= 4 and (S[rows] == 0).all() and all_pos_zero(F[rows]), name
    if isinstance(case, gc.SegmentCase):
        pairs, sep, force = case.last_rows
        listed = {(int(i), int(j)): k for k, (i, j) in enumerate(pairs)}
        inb = case.in_branch()
        mine = {(int(i), int(j)) for i, j in zip(case.pi[inb], case.pj[inb])}
        assert mine <= set(listed), "a pair in the force branch is missing from the device's list"
        out = np.array([p not in mine for p in listed])
        assert out.sum() >= 4 and all_pos_zero(force[out]) and (np.abs(force[~out]).max(axis=1) > 0).all()


# ---- B. momentum and angular momentum ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", PAIR_NAMES)
def test_pair_terms_conserve_momentum_and_angular_momentum(name):
    """|sum_b F_b| <= 8 eps sum |F| and |sum_b x_b x F_b| <= 8 eps sum |x| |F| on the device's output, the sums by
    math.fsum: the barycentric share and the central direction make both exact up to rounding"""
    case = gc.cases()[name]
    assert case.pair_terms
    F = _device(case)
    if case.rows == "linkers":   # the linker's force on its first body; the second receives its negative
        lever, total = case.lever_positions(case.x), np.zeros(3)
        norms = 2.0 * np.linalg.norm(F, axis=1)
    else:
        lever, total = case.x, gc.fsum_rows(F)
        norms = np.linalg.norm(F, axis=1)
    torque = gc.fsum_rows(np.cross(lever, F))
    sum_f = math.fsum(norms)
    sum_xf = math.fsum(np.linalg.norm(lever, axis=1) * np.linalg.norm(F, axis=1))
    print("%s: |sum F| = %.3g eps sum |F|, |sum x x F| = %.3g eps sum |x| |F|" % (
        name, np.abs(total).max() / (EPS * sum_f), np.abs(torque).max() / (EPS * sum_xf)))
    assert sum_f > 0.0
    assert np.abs(total).max() <= 8.0 * EPS * sum_f
    assert np.abs(torque).max() <= 8.0 * EPS * sum_xf


# ---- C. rigid motions ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", gc.NAMES)
def test_forces_turn_with_the_configuration(name):
    """The configuration rotated by a random Q and translated, in float64; the energies at its exact pre-image, in the
    original frame: the device's forces are Q F to K eps S_b.  (The fast ellipsoid wall has no orientation: it is
    translated only.)"""
    case = gc.cases()[name]
    x2, f2, want, S = gc.moved_exact(name)
    assert np.abs(x2 - case.x).max() > 0.5
    got = _device(case, x2, f2)
    d = gc.deviation(got, want, S)
    K = gc.TOLERANCE_K[case.group]
    print("%s: worst deviation from Q F %.3g eps S_b (K = %g)" % (name, d.max(), K))
    assert (d <= K).all(), (name, int(np.argmax(d)), float(d.max()))


# ---- D. descent along the composed step ------------------------------------------------------------------------------------------------
import backbone_case as bc  # noqa: E402

DESCENT_STEPS = 12


def chain_energy(case, x, sphere_hertz):
    """U(x) of the backbone case in longdouble: springs, backbone segments with the end correction, and (mode "first")
    the Hertz contacts of the bead spheres"""
    ends = np.asarray(case["pairs"])
    deg = np.bincount(ends.reshape(-1), minlength=case["n"])
    U = P.ld_spring_energy(x, ends, "hookean", case["spring_k"], case["spring_r"])
    U = U + P.ld_backbone_energy(x, ends, case["kind"], bc.SEGMENT_RADIUS, (deg[ends] == 1).any(axis=1),
                                 E=case["youngs_modulus"], nu=case["poisson_ratio"])
    if sphere_hertz:
        U = U + P.ld_sphere_hertz_energy(x, case["radius"], case["youngs_modulus"], case["poisson_ratio"])
    return U


def descent_ratios(case, step, steps=DESCENT_STEPS):
    """step(x) -> (F [n, 3], v [n, 3], the new x): -> per step (U before, U after, -dU / (dt F.v))"""
    out = []
    x = case["center"].copy()
    first = case["mode"] == "first"
    U0 = chain_energy(case, x, first)
    for _ in range(steps):
        F, v, x = step(x)
        U1 = chain_energy(case, x, first)
        fv = np.sum(np.asarray(F, dtype=np.longdouble) * np.asarray(v, dtype=np.longdouble))
        out.append((float(U0), float(U1), float(-(U1 - U0) / (np.longdouble(case["dt"]) * fv))))
        U0 = U1
    return out


DESCENT = [(kind, mode, hydro) for kind in ("hertz", "wca") for mode, hydro in
           (("none", False), ("first", True), ("none", True))]


@gpu
@pytest.mark.parametrize("kind,mode,hydro", DESCENT, ids=["%s-%s%s" % (k, m, "-rpyc" if h and m == "none" else "")
                                                          for k, m, h in DESCENT])
def test_step_descends_the_energy(kind, mode, hydro):
    """Without noise the step is explicit Euler along v = M F with M positive definite: U falls at every step, and
    -dU / (dt F.v) is 1 less the second-order term of the step -- within 0.5 .. 1 + 1e-9 (the composed numpy models give
    0.816 .. 0.994 on these cases).  A stage added with the wrong sign, a mobility applied twice or a hydrodynamic
    velocity taken from another force field leaves the band."""
    from mundy_amd import pipeline
    case = bc.build(kind, mode)
    kw = bc.stepper_kwargs(case)
    kw["brownian_kt"] = None
    if hydro and mode == "none":
        kw["hydrodynamics"] = dict(case["hydro"])
    assert (mode == "first") == bool(kw.get("hydrodynamics", {}).get("contact_forces", False))
    st = pipeline.ContactStepper("sphere", dev(case["center"]), dev(case["radius"]), **kw)

    def step(x):
        s = st.step()
        assert s.segment_contacts > 0
        if mode == "first":
            assert s.num_contacts > 0
        return host(st.spring_force).copy(), host(st.velocity)[:, :3].copy(), host(st.center).copy()

    rows = descent_ratios(case, step)
    for k, (U0, U1, ratio) in enumerate(rows):
        print("%s %s%s step %2d: U %.9g -> %.9g, -dU / (dt F.v) = %.6f" % (kind, mode, " rpyc" if hydro else "", k, U0,
                                                                         U1, ratio))
    assert all(U1 < U0 for U0, U1, _ in rows)
    assert all(0.5 <= r <= 1.0 + 1e-9 for _, _, r in rows), [r for _, _, r in rows]


# ---- E .. J. the filament family against the discrete rod energy ---------------------------------------------------------------------
import filament_cases as fc  # noqa: E402

K_FORCE = {"first": "filament force", "wave": "filament force, wave", "moved": "filament force"}


def _filaments(lay, prm):
    f = O().Filaments(lay["node_ptr"], lay["radius"], lay["rest_curvature"], lay["arclength"], lay["phase"],
                      **fc.device_kwargs(prm))
    f.set_state(dev(lay["center"]), dev(lay["twist"]), dev(lay["edge_orientation"]))
    return f


_EVALUATED = {}


def filament_evaluation(lay, kind, key=None):
    """the device over the layout: set_state, force [, velocity, advance, force] -> (F [n, 3], tau [n], statistics [2])
    of the last evaluation; kept per key (the output is a function of the inputs alone)"""
    if key is not None and key in _EVALUATED:
        return _EVALUATED[key]
    f = _filaments(lay, fc.params(wave=kind == "wave"))
    stats = f.force(fc.TIME_FIRST)
    if kind == "moved":
        f.velocity()
        f.advance(fc.DT)
        stats = f.force(fc.TIME_MOVED)
    out = (host(f.field("force")).copy(), host(f.field("twist_torque")).copy(), host(stats).copy())
    f.close()
    if key is not None:
        _EVALUATED[key] = out
    return out


def _assert_filament_rows(name, st, ex, F, tau):
    kind = fc.split(name)[0]
    Kf, Kt = gc.TOLERANCE_K[K_FORCE[kind]], gc.TOLERANCE_K["filament torque"]
    dF = fc.deviation(F[st.nodes], ex["F"], ex["S_F"])
    dT = fc.deviation(tau[st.nodes], ex["tau"], ex["S_tau"])
    print("%s: worst deviation: force %.3g eps S_F (K = %g), torque %.3g eps S_tau (K = %g)" % (name, dF.max(), Kf,
                                                                                              dT.max(), Kt))
    assert (dF <= Kf).all(), (name, int(np.argmax(dF)), float(dF.max()))
    assert (dT <= Kt).all(), (name, int(np.argmax(dT)), float(dT.max()))
    assert (ex["S_F"] > 0).all() and (ex["S_tau"] > 0).sum() >= 8
    return Kf


@gpu
@pytest.mark.parametrize("name", fc.NAMES)
def test_filament_force_is_minus_the_gradient_plus_the_stray_term(name):
    """E (conservative where it should be) and F (departs only by the stray term).  At the first evaluation after
    set_state, wave off or on, F = -grad E and tau = -dE/dtheta on every node.  After the nodes have moved tau =
    -dE/dtheta still, and F = -grad E + R with R of tests/filament_cases.py, which is at least 100 K eps S_F on some
    node: the test cannot pass with R dropped, nor with anything beside R added."""
    kind, lay_name = fc.split(name)
    st = fc.state(name)
    st.check()
    F, tau, _ = filament_evaluation(st.layout, kind, name)
    ex = fc.exact_of(name)
    K = _assert_filament_rows(name, st, ex, F, tau)
    size = np.abs(ex["R"]).max(axis=1) / (EPS * ex["S_F"])
    if kind == "moved":
        print("%s: max |R| = %.3g, %.3g eps S_F" % (name, np.abs(ex["R"]).max(), size.max()))
        assert size.max() >= 100.0 * K
    else:
        assert not ex["R"].any()
    # a filament of two nodes has no element: torques of exactly +0.0 (and so has every filament's last node)
    ptr = st.layout["node_ptr"]
    two = np.flatnonzero(np.diff(ptr) == 2)
    assert lay_name != "small" or len(two) == 2
    for f in two:
        assert all_pos_zero(tau[ptr[f]:ptr[f + 1]])
    assert all_pos_zero(tau[ptr[1:] - 1])


@gpu
@pytest.mark.parametrize("name", fc.NAMES)
def test_filaments_conserve_momentum(name):
    """G.  Per filament |sum F| <= 8 eps sum |F|, the sums by math.fsum, in all three states: every element and edge
    term is handed out with the sum zero, the stray term as +R and -R.  No angular momentum is asserted: the twist is
    not a full rotational degree of freedom, and sum x x F of the model is 0.08 on the small layout."""
    kind, _ = fc.split(name)
    st = fc.state(name)
    F, _, _ = filament_evaluation(st.layout, kind, name)
    ptr = st.layout["node_ptr"]
    worst = 0.0
    for a, b in zip(ptr[:-1], ptr[1:]):
        sum_f = math.fsum(np.linalg.norm(F[a:b], axis=1))
        assert sum_f > 0.0
        worst = max(worst, np.abs(gc.fsum_rows(F[a:b])).max() / (EPS * sum_f))
    print("%s: worst |sum F| = %.3g eps sum |F| over %d filaments" % (name, worst, len(ptr) - 1))
    assert worst <= 8.0


@gpu
@pytest.mark.parametrize("name", fc.NAMES)
def test_filament_forces_turn_with_the_configuration(name):
    """H.  The layout rotated by a random Q and translated, frames q_Q q, then set_state, force [, velocity, advance,
    force]: the evaluation gives Q F (and Q R) and the same tau, to K against the exact values at the pre-image, whose
    old tangents and frames are those of the model's run from the rotated layout; and the same two statistics as the
    run that was not rotated.  (The rotated layout is Q x + s to 4 eps max |x| per coordinate, so an edge's length
    differs by at most 8 eps max |x| and, with l near 1, its tangent and the curvature by as much again: 32 eps max
    |x| bounds both statistics.)"""
    kind, _ = fc.split(name)
    lay2, st2, ex2 = fc.moved_exact(name)
    lay = fc.state(name).layout
    assert np.abs(lay2["center"] - lay["center"]).max() > 0.5
    st2.check()
    F, tau, stats = filament_evaluation(lay2, kind)
    _assert_filament_rows(name + ", rotated", st2, ex2, F, tau)
    _, _, stats0 = filament_evaluation(lay, kind, name)
    bound = 32.0 * EPS * max(np.abs(lay["center"]).max(), np.abs(lay2["center"]).max())
    print("%s: statistics %r, not rotated %r" % (name, stats.tolist(), stats0.tolist()))
    assert (stats0 > 0.0).all() and (np.abs(stats - stats0) <= bound).all()


@gpu
@pytest.mark.parametrize("layout,monolayer", [("small", False), ("planar", True)], ids=["3d", "monolayer"])
def test_filament_step_descends_the_energy(layout, monolayer):
    """I.  FilamentStepper with disable_twist, no wave, 12 steps of dt = 0.01: with the twist held at zero the frames
    follow the edges by transport alone, E (longdouble, from the centres and the stepped frames) is a function of the
    stepped state, and the step is explicit Euler along v = F / (6 pi eta r): E falls at every step and -dE / (dt F.v)
    is 1 less the step's second-order term, within 0.5 .. 1 + 1e-9.  filament_model.py gives 0.9823 .. 0.9849 in 3-D
    and 0.9838 .. 0.9858 in the monolayer on these layouts (printed beside the device's).  The stray term R does
    no harm here: it is of the order |b| / l = dt |v| / l against |F|.
    With the twist on nothing is asserted: the twist rotation is applied to the carried frame again at every step
    (DESIGN.md 5j, quirk 1), so the twist enters as a rate, E is not a function of (x, theta), and along the model's
    trajectory on the small layout it rises (7.8 -> 70 over 30 steps)."""
    from mundy_amd import pipeline
    lay = fc.layout(layout)
    prm = fc.params(disable_twist=True, monolayer=monolayer)
    st = pipeline.FilamentStepper(lay["node_ptr"], lay["center"], lay["radius"], lay["edge_orientation"], lay["arclength"],
                                  twist=lay["twist"], rest_curvature=lay["rest_curvature"], phase=lay["phase"],
                                  **fc.device_kwargs(prm))

    def step():
        st.step(fc.DESCENT_DT)
        return (host(st.field("force")), host(st.field("velocity")), host(st.field("center")),
                host(st.field("edge_orientation")))

    rows = fc.descent_ratios(lay, step, monolayer)
    st.close()
    model = fc.model_descent(layout, monolayer)
    for k, ((U0, U1, ratio), (_, _, want)) in enumerate(zip(rows, model)):
        print("%s step %2d: E %.9g -> %.9g, -dE / (dt F.v) = %.6f (model %.6f)" % (layout, k, U0, U1, ratio, want))
    assert len(rows) == fc.DESCENT_STEPS
    assert all(U1 < U0 for U0, U1, _ in rows)
    assert all(0.5 <= r <= 1.0 + 1e-9 for _, _, r in rows), [r for _, _, r in rows]
    assert all(0.5 <= r <= 1.0 + 1e-9 for _, _, r in model)


def _contact_stage(case, mu):
    f = _filaments(case.layout, fc.params())
    c = O().FilamentContacts(f, **case.contact_kwargs(mu))
    c.save_velocity()
    assert c.update()
    return f, c


@gpu
def test_frictionless_filament_contacts_are_minus_the_gradient_of_the_hertz_energy():
    """J.  mu = 0, no damping, nothing saved: the node forces are -grad of the sum of the pair energies (8/15) E* sqrt(R*)
    delta^(5/2) within K, the barycentric share included; a listed pair out of overlap contributes exactly +0.0."""
    case = fc.contact_case()
    case.check()
    f, c = _contact_stage(case, 0.0)
    c.force(fc.DT)
    F = host(c.field("node_force")).copy()
    pairs, force = host(c.field("pairs")).copy(), host(c.field("force")).copy()
    c.close()
    f.close()
    exact, S = fc.contact_exact()
    d = gc.deviation(F, exact, S)
    K = gc.TOLERANCE_K[case.group]
    print("filament contacts: worst deviation %.3g eps S_b (K = %g)" % (d.max(), K))
    assert (d <= K).all(), (int(np.argmax(d)), float(d.max()))
    assert (S > 0).sum() >= 16
    listed = {(int(i), int(j)) for i, j in pairs}
    inb = case.in_branch()
    mine = {(int(i), int(j)) for i, j in zip(case.pi[inb], case.pj[inb])}
    assert mine <= listed, "a pair in overlap is missing from the device's list"
    out = np.array([(int(i), int(j)) not in mine for i, j in pairs])
    assert out.sum() >= 8 and all_pos_zero(force[out]) and (np.abs(force[~out]).max(axis=1) > 0).all()


@gpu
def test_frictional_filament_contacts_conserve_momentum_and_leave_the_contact_couple():
    """J.  mu = 0.5 with a planted tangential history and saved velocities: |sum F| <= 8 eps sum |F| over the nodes, and
    sum x x F = sum over the pairs of (cp1 - cp2) x F_pair to 8 eps sum |x| |F|: friction acts at the closest points
    of the centrelines, so exactly this couple is left, and the barycentric share hands each segment's force and moment
    to its two nodes.  The closest points are the longdouble distance's, not the device's."""
    case = fc.contact_case()
    f, c = _contact_stage(case, 0.5)
    pairs = host(c.field("pairs")).copy()
    velocity, history = fc.planted(case, pairs)
    c.set_field("velocity_prev", dev(velocity))
    c.set_history(dev(pairs), dev(history))
    stats = host(c.force(fc.DT)).copy()
    F, force, sep = host(c.field("node_force")).copy(), host(c.field("force")).copy(), host(c.field("sep")).copy()
    c.close()
    f.close()
    touching, sliding = int((sep <= 0.0).sum()), int(stats.view(np.int64)[1])
    x = case.x
    _, s, t = P.ld_segment_segment(x[pairs[:, 0]], x[pairs[:, 0] + 1], x[pairs[:, 1]], x[pairs[:, 1] + 1], True)
    arm = np.asarray((x[pairs[:, 0]] + s[:, None] * (x[pairs[:, 0] + 1] - x[pairs[:, 0]])) -
                     (x[pairs[:, 1]] + t[:, None] * (x[pairs[:, 1] + 1] - x[pairs[:, 1]])), dtype=np.float64)
    hit = sep <= 0.0
    unit = arm[hit] / np.linalg.norm(arm[hit], axis=1)[:, None]
    tangential = force[hit] - (force[hit] * unit).sum(axis=1)[:, None] * unit
    assert touching >= 16 and 0 < sliding < touching
    assert (np.linalg.norm(tangential, axis=1) > 1e-3 * np.linalg.norm(force[hit], axis=1)).sum() >= 8
    mom, ang = fc.contact_balance(case, pairs, force, F)
    print("frictional filament contacts: %d touching, %d sliding; |sum F| = %.3g eps sum |F|, couple off by %.3g eps sum "
          "|x| |F|" % (touching, sliding, mom, ang))
    assert mom <= 8.0 and ang <= 8.0
