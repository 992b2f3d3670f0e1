"""One test case, "the nucleus with everything on": every stage of the HP1 chromatin step in one stepper, for
tests/test_hp1_step_host.py (the numpy models alone) and tests/test_gpu_hp1_step.py (pipeline.ContactStepper and the C++
mech::SphereChainStepper).  numpy only: nothing here touches the device.

The stage letters:  X crosslinkers,  Y periphery bind sites (needs X),  P the nuclear wall,  A active dipoles,
U hydrodynamics,  W the periphery's no-slip correction (needs U),  E an external force,  H the Hertz contact with its
force as the first term of the force field (without H: the LCP).  The backbone springs and the noise are always on.

H without U: pipeline.ContactStepper hangs contact_forces=True on hydrodynamics=, so without hydrodynamics the Hertz
contact runs in the stepper's other order (a body sweep after U_ext, no first term); mech::SphereChainStepper has the
first-term order only and cannot run that case (`first_term` below tells the two apart).

build(letters) -> a dict of plain arrays and numbers (what the models and the C++ input file take); stepper_kwargs(case)
-> the keyword arguments of pipeline.ContactStepper after (kind, center, radius).  The composed models of one step:
kmc(), force_field(), hydro_velocity()."""
import numpy as np

import chain_model as chm
import contact_force_model as cfm
import crosslinker_model as xm
import hydro_model as hm
import hydro_periphery_model as hpm
import periphery_binding_model as pbm
import periphery_model as pm

LETTERS = "XYPAUWEH"
ALL = frozenset(LETTERS)
# all on in both contact modes; from all-on in Hertz mode one stage left out at a time (with what needs it)
CASES = [ALL, ALL - {"H"}] + [ALL - set(s) for s in ("XY", "Y", "P", "A", "W", "UW", "E")]


def case_id(letters):
    return "".join(c for c in LETTERS if c in letters)


def check_letters(letters):
    letters = frozenset(letters)
    if not letters <= ALL or ("Y" in letters and "X" not in letters) or ("W" in letters and "U" not in letters):
        raise ValueError("stage letters %r: a subset of %s, Y with X, W with U" % (case_id(letters), LETTERS))
    return letters


SIDE, BEADS = 4, 40
WALL_RADIUS = 19.9    # the chains' end beads sit at |x| = 19.5 +- 0.03: every one of them overlaps the wall
HYDRO_RADIUS = 22.0   # the no-slip surface: every bead is well inside
QUADRATURE_ORDER = 4


def build(letters):
    """SIDE x SIDE straight chains of BEADS beads along x (spacing 1, 1.2 apart, jittered by 0.03, centred on the
    origin).  Hertz mode: radius 0.52, so neighbours along a chain overlap by 0.04 +- 0.04.  LCP: radius 0.5, so half
    of them overlap and the first solve pushes the chains apart.  A crosslinker on every other bead, every bead a bind
    site, and a candidate skin of 0.02, a few steps of noise: both candidate lists are rebuilt from moved beads several
    times in 20 steps, and a list kept from the initial centres misses sites that have come within reach.  An active
    dipole on every third spring; 2000 periphery sites on the wall."""
    from mundy_amd import synth
    letters = check_letters(letters)
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(BEADS) * 1.0, np.arange(SIDE) * 1.2, np.arange(SIDE) * 1.2, indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3)) + rng.normal(size=(SIDE * SIDE * BEADS, 3)) * 0.03
    c = np.ascontiguousarray(c - c.mean(axis=0))
    n = c.shape[0]
    first = (np.arange(SIDE * SIDE)[:, None] * BEADS + np.arange(BEADS - 1)[None, :]).reshape(-1)
    pairs = np.ascontiguousarray(np.stack([first, first + 1], axis=1).astype(np.int32))
    radius = np.full(n, 0.52 if "H" in letters else 0.5)
    viscosity = 1.0
    idx = np.arange(0, pairs.shape[0], 3)
    qp, qw, qn = hpm.sphere_quadrature(QUADRATURE_ORDER, HYDRO_RADIUS, invert=True)
    return dict(
        letters=letters, first_term="H" in letters and "U" in letters, n=n, center=c, radius=radius, pairs=pairs,
        mob_trans=synth.dry_mobility(radius, viscosity=viscosity)[0],
        dt=1e-3, viscosity=viscosity, search_buffer=0.4, kt=0.1, spring_k=3.0, spring_r=1.0,
        youngs_modulus=1000.0, poisson_ratio=0.3,
        xl=dict(left=np.arange(0, n, 2), sites=np.ones(n, np.uint8), kind="hookean", k=3.0, r=1.0, bind_rate=300.0,
                unbind_rate=150.0, kt=0.1, capture_radius=1.5, skin=0.02),
        site_points=synth.periphery_bind_sites("sphere", WALL_RADIUS, 2000, seed=9),
        per=dict(bind_rate=2000.0, k=0.5, r=0.8, unbind_rate=100.0, capture_radius=1.8),
        wall=dict(shape="sphere", radius=WALL_RADIUS, k=50.0),
        active=dict(springs=idx, sigma=2.0, kon=300.0, koff=200.0), active_pairs=np.ascontiguousarray(pairs[idx]),
        hydro=dict(kind="rpyc", update_every=2), quadrature=(qp, qw, qn),
        ext=np.random.default_rng(31).normal(size=(n, 3)))


def stepper_kwargs(case):
    """the keyword arguments of pipeline.ContactStepper("sphere", center, radius, **kw) for the case"""
    on = case["letters"]
    kw = dict(dt=case["dt"], viscosity=case["viscosity"], search_buffer=case["search_buffer"],
              contact_model="hertz" if "H" in on else "lcp", youngs_modulus=case["youngs_modulus"],
              poisson_ratio=case["poisson_ratio"], brownian_kt=case["kt"],
              springs=(case["pairs"], "hookean", case["spring_k"], case["spring_r"]))
    if "X" in on:
        kw["crosslinkers"] = dict(case["xl"])
        if "Y" in on:
            kw["crosslinkers"]["periphery_sites"] = dict(points=case["site_points"], **case["per"])
    if "P" in on:
        kw["periphery"] = dict(case["wall"])
    if "A" in on:
        kw["active_forces"] = dict(case["active"])
    if "U" in on:
        kw["hydrodynamics"] = dict(case["hydro"])
        if "H" in on:
            kw["hydrodynamics"]["contact_forces"] = True
        if "W" in on:
            qp, qw, qn = case["quadrature"]
            kw["hydrodynamics"]["periphery"] = dict(points=qp, weights=qw, normals=qn)
    return kw


# ---- the composed models of one step ----------------------------------------------------------------------------------------
def _per(case):
    p = case["per"]
    return dict(A=p["bind_rate"], k=p["k"], r=p["r"], k_off=p["unbind_rate"], capture_radius=p["capture_radius"])


def kmc(case, x, left, right, counters):
    """one KMC step of the crosslinkers at the centres x from the heads and counters given (keys: the crosslinker
    indices; candidate rows: exact, by ascending body / site index) -> periphery_binding_model.kmc_step's dict, or
    crosslinker_model.kmc_step's without Y"""
    p, n = case["xl"], case["n"]
    src = np.zeros(n, bool)
    src[np.asarray(left)] = True
    keys = np.arange(len(left), dtype=np.uint64)
    counters = np.asarray(counters).astype(np.uint64)
    ptr, col = xm.candidate_rows(x, src, p["sites"], p["capture_radius"])
    if "Y" not in case["letters"]:
        return xm.kmc_step(x, left, right, ptr, col, p["kind"], p["k"], p["r"], p["bind_rate"], p["unbind_rate"], p["kt"],
                           p["capture_radius"], case["dt"], keys, counters)
    pptr, pcol = pbm.site_rows(x, src, case["site_points"], case["per"]["capture_radius"])
    return pbm.kmc_step(x, left, right, ptr, col, pptr, pcol, case["site_points"], pbm.from_ops(p), _per(case),
                        case["dt"], keys, counters)


def force_field(case, x, heads=None, active_state=None, contact_force=None):
    """F = ((((D lam + F_spring) + F_crosslinker) + F_wall) + F_active) + F_ext at the centres x, the terms that are
    off left out; heads = (left, right) after the step's KMC, active_state after its sampling, contact_force = D lam
    [n, 3] (the first term: given only where the step has one).  -> (F, info): info holds each model's statistics and,
    per term, whether it acted on some bead"""
    on, n = case["letters"], case["n"]
    info = dict(acted={})
    F, _, info["max_spring_length"] = chm.spring_force(n, case["pairs"], "hookean", case["spring_k"], case["spring_r"], x)
    info["spring_force"] = F
    if contact_force is not None:
        F = contact_force + F
    if "X" in on:
        le, ri = (np.asarray(h, dtype=np.int64) for h in heads)
        p = case["xl"]
        if "Y" in on:
            X, _, mx, _ = pbm.crosslinker_force(n, le, ri, p["kind"], p["k"], p["r"], x, case["site_points"])
            only = pbm.crosslinker_force(n, le, np.where(ri < 0, ri, le), p["kind"], p["k"], p["r"], x,
                                         case["site_points"])[0]
            info["acted"]["Y"] = bool(np.abs(only).max() > 0.0)
        else:
            X, _, mx = xm.crosslinker_force(n, le, ri, p["kind"], p["k"], p["r"], x)
        F = F + X
        info.update(crosslinker_bound=int((ri != le).sum()), crosslinker_periphery_bound=int((ri < 0).sum()),
                    max_crosslinker_length=mx, crosslinker_force=X)
        info["acted"]["X"] = bool(np.abs(X).max() > 0.0)
    if "P" in on:
        w = case["wall"]
        F, info["periphery_colliding"], info["max_periphery_overlap"] = pm.sphere_force(x, case["radius"], w["radius"],
                                                                                        w["k"], force=F)
        info["acted"]["P"] = info["periphery_colliding"] > 0
    if "A" in on:
        F, info["active_springs"] = pm.active_force(n, case["active_pairs"], active_state, case["active"]["sigma"], x,
                                                    force=F)
        info["acted"]["A"] = info["active_springs"] > 0
    if "E" in on:
        F = F + case["ext"]
        info["acted"]["E"] = bool(np.abs(case["ext"]).max() > 0.0)
    return F, info


def contact_force(case, pairs, lam, normal):
    """D lam [n, 3]: the contact force of every body from per-contact force magnitudes"""
    return cfm.body_force(case["n"], pairs, x=lam, normal=normal, stride=3)


_INVERSE = {}


def periphery_inverse(case):
    """(Minv, min_pivot) of the case's no-slip surface by the model's own fill and Gauss-Jordan; computed once"""
    key = (QUADRATURE_ORDER, HYDRO_RADIUS, case["viscosity"])
    if key not in _INVERSE:
        qp, qw, qn = case["quadrature"]
        Minv, min_pivot, _ = hpm.gauss_jordan(hpm.fill_matrix(qp, qw, qn, case["viscosity"])[1])
        _INVERSE[key] = (Minv, min_pivot)
    return _INVERSE[key]


def hydro_velocity(case, x, F, correction=None):
    """u_hydro [n, 3] of the force field F at the centres x: hydro_model.velocity, and with W (or correction=True) the
    periphery's correction of the same F added to it"""
    u = hm.velocity(case["hydro"]["kind"], case["viscosity"], x, case["radius"], F)
    if ("W" in case["letters"]) if correction is None else correction:
        qp, qw, qn = case["quadrature"]
        u = hpm.correct(case["hydro"]["kind"], case["viscosity"], qp, qw, qn, periphery_inverse(case)[0], x, case["radius"],
                        F, old=u)[0]
    return u


# ---- the input of tests/cpp/hp1_step_app -------------------------------------------------------------------------------------
def write_app_input(case, path):
    """read_chain_input's header (n, springs, crosslinkers, periphery sites, active springs, quadrature nodes, 1 with an
    external force else 0) and arrays, then: crosslinker left (int32), site mask (bytes [n]), periphery site points,
    active pairs (int32), quadrature points, weights, normals, external force [n][3]; a stage that is off writes its
    arrays all the same, the app's stage letters decide what is used"""
    qp, qw, qn = case["quadrature"]
    left = case["xl"]["left"]
    with open(path, "wb") as f:
        np.array([case["n"], case["pairs"].shape[0], left.shape[0], case["site_points"].shape[0],
                  case["active_pairs"].shape[0], qp.shape[0], 1], dtype=np.uint64).tofile(f)
        for a in (case["center"], case["radius"], case["mob_trans"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        case["pairs"].astype(np.int32).tofile(f)
        left.astype(np.int32).tofile(f)
        case["xl"]["sites"].astype(np.uint8).tofile(f)
        np.ascontiguousarray(case["site_points"], dtype=np.float64).tofile(f)
        case["active_pairs"].astype(np.int32).tofile(f)
        for a in (qp, qw, qn, case["ext"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)


def app_arguments(case, steps):
    """the command line of hp1_step_app after the input file: steps, the stage letters, then every number in the
    order of the app's usage line"""
    x, p, w, a = case["xl"], case["per"], case["wall"], case["active"]
    nums = [case["dt"], case["search_buffer"], case["spring_k"], case["spring_r"], case["kt"],
            x["k"], x["r"], x["bind_rate"], x["unbind_rate"], x["kt"], x["capture_radius"], x["skin"],
            p["bind_rate"], p["k"], p["r"], p["unbind_rate"], p["capture_radius"],
            w["radius"], w["k"], a["sigma"], a["kon"], a["koff"], case["viscosity"], case["hydro"]["update_every"],
            case["youngs_modulus"], case["poisson_ratio"]]
    return [str(int(steps)), case_id(case["letters"]) or "-"] + [repr(float(v)) for v in nums]
