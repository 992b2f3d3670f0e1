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
  D  the composed step lowers U by dt F.v, to the first order of the explicit Euler step"""
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
