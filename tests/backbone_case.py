"""The chain step with the backbone segment contacts: tests/hp1_case.py's lattice (SIDE x SIDE straight chains of BEADS
beads along x, spacing 1, 1.2 apart, jittered by 0.03, centred on the origin) with springs, noise and the segment term,
for tests/test_gpu_segment_contacts.py (pipeline.ContactStepper and the C++ mech::SphereChainStepper).  numpy only.

Modes:  "none"   contact_model="none": the reference's configuration, U = U_ext
        "first"  contact_model="hertz" + hydrodynamics contact_forces: F = (D f + F_backbone) + F_spring, U = U_ext
        "lcp"    contact_model="lcp": the segment term is one more force, U = U_ext + M D lam

Segments of radius 0.55 on a pitch of 1: a segment and its second neighbour along the chain overlap by 0.1 +- 0.04 (Hertz)
and lie inside the WCA cutoff; neighbouring chains, 1.2 apart, come within the cutoff here and there.  The skin of 0.05
makes the 10 steps of noise rebuild the list a few times."""
import numpy as np

import chain_model as chm
import contact_force_model as cfm
import hydro_model as hm
import segment_contact_model as scm

SIDE, BEADS = 4, 40
MODES = ("none", "first", "lcp")
SEGMENT_RADIUS, SKIN = 0.55, 0.05


def build(kind, mode):
    from mundy_amd import synth
    assert kind in ("hertz", "wca") and mode in MODES
    rng = np.random.default_rng(5)
    g = np.stack(np.meshgrid(np.arange(BEADS) * 1.0, np.arange(SIDE) * 1.2, np.arange(SIDE) * 1.2, indexing="ij"), -1)
    c = np.ascontiguousarray(g.transpose(1, 2, 0, 3).reshape(-1, 3)) + rng.normal(size=(SIDE * SIDE * BEADS, 3)) * 0.03
    c = np.ascontiguousarray(c - c.mean(axis=0))
    n = c.shape[0]
    pairs = synth.backbone_segments(np.arange(SIDE * SIDE + 1) * BEADS)
    radius = np.full(n, 0.52 if mode == "first" else 0.5)
    viscosity = 1.0
    return dict(kind=kind, mode=mode, n=n, center=c, radius=radius, pairs=pairs,
                mob_trans=synth.dry_mobility(radius, viscosity=viscosity)[0], dt=1e-3, viscosity=viscosity,
                search_buffer=0.4, kt=0.1, spring_k=3.0, spring_r=1.0, youngs_modulus=1000.0, poisson_ratio=0.3,
                backbone=dict(kind=kind, radius=SEGMENT_RADIUS, skin=SKIN), hydro=dict(kind="rpyc", update_every=1))


def stepper_kwargs(case):
    """the keyword arguments of pipeline.ContactStepper("sphere", center, radius, **kw) for the case"""
    kw = dict(dt=case["dt"], viscosity=case["viscosity"], search_buffer=case["search_buffer"],
              contact_model={"none": "none", "first": "hertz", "lcp": "lcp"}[case["mode"]],
              youngs_modulus=case["youngs_modulus"], poisson_ratio=case["poisson_ratio"], brownian_kt=case["kt"],
              springs=(case["pairs"], "hookean", case["spring_k"], case["spring_r"]),
              backbone_collision=dict(case["backbone"]))
    if case["mode"] == "first":
        kw["hydrodynamics"] = dict(case["hydro"], contact_forces=True)
    return kw


def segment_model(case):
    return scm.SegmentContacts(case["n"], case["pairs"], case["kind"], SEGMENT_RADIUS, SKIN)


def force_field(case, model, x, contact_force=None):
    """F = ((D f +) F_backbone) + F_spring at the centres x; `model` (segment_model) carries the list from step to step
    -> (F, info: rebuilt, the segment statistics, the two terms, sum |F_c| per node)"""
    rebuilt = model.update(x)
    S, stats = model.force_pass(x, external=contact_force)
    Fs, _, mx = chm.spring_force(case["n"], case["pairs"], "hookean", case["spring_k"], case["spring_r"], x)
    # sum over the linkers of the node's segments of |F_c|: what the Hertz bound of the force is taken from
    per_seg = np.zeros(model.m)
    mag = np.sqrt((model.force * model.force).sum(axis=1))
    np.add.at(per_seg, model.pairs.reshape(-1), np.repeat(mag, 2))
    per_seg += np.sqrt((model.end_terms()[0] ** 2).sum(axis=1))
    per_node = np.zeros(case["n"])
    np.add.at(per_node, model.ends.reshape(-1), np.repeat(per_seg, 2))
    return S + Fs, dict(rebuilt=rebuilt, max_segment_overlap=stats[0], segment_contacts=stats[1],
                        num_segment_pairs=model.pairs.shape[0], backbone=S, spring=Fs, max_spring_length=mx,
                        scale=per_node)


def contact_force(case, pairs, lam, normal):
    return cfm.body_force(case["n"], pairs, x=lam, normal=normal, stride=3)


def hydro_velocity(case, x, F):
    return hm.velocity(case["hydro"]["kind"], case["viscosity"], x, case["radius"], F)


# ---- two crossed strands ----------------------------------------------------------------------------------------------------
def crossed_strands(kind):
    """strand A along x through the origin, strand B along y, 0.9 above it; a constant force presses B down and A up.
    Without an excluded volume between the segments B would be below A after ~50 of the 120 steps."""
    from mundy_amd import synth
    b = 9
    t = (np.arange(b) - 0.5 * (b - 1)) * 1.0 + 0.13   # (off the lattice: the crossing is interior to both segments)
    A = np.stack([t, np.zeros(b), np.zeros(b)], axis=1)
    B = np.stack([np.full(b, 0.07), t, np.full(b, 0.9)], axis=1)
    c = np.ascontiguousarray(np.concatenate([A, B]))
    ext = np.zeros_like(c)
    ext[:b, 2], ext[b:, 2] = 10.0, -10.0
    radius = np.full(2 * b, 0.5)
    return dict(kind=kind, n=2 * b, beads=b, center=c, radius=radius, pairs=synth.backbone_segments([0, b, 2 * b]),
                ext=ext, mob_trans=synth.dry_mobility(radius, viscosity=1.0)[0], dt=1e-2, viscosity=1.0, spring_k=100.0,
                spring_r=1.0, steps=120, backbone=dict(kind=kind, radius=0.5, skin=0.3))


def crossed_kwargs(case):
    return dict(dt=case["dt"], viscosity=case["viscosity"], contact_model="none",
                springs=(case["pairs"], "hookean", case["spring_k"], case["spring_r"]),
                backbone_collision=dict(case["backbone"]))


def crossed_gap(case, x):
    """z of strand B's middle bead above strand A's"""
    b = case["beads"]
    return float(x[b + b // 2, 2] - x[b // 2, 2])


def crossed_model_run(case):
    """the numpy step of the crossed strands, no noise: x += dt m_t (F_backbone + F_spring + F_ext) -> (centres, the
    smallest gap of the run)"""
    x = case["center"].copy()
    model = scm.SegmentContacts(case["n"], case["pairs"], case["kind"], 0.5, 0.3)
    low = crossed_gap(case, x)
    for _ in range(case["steps"]):
        model.update(x)
        S, _ = model.force_pass(x)
        Fs = chm.spring_force(case["n"], case["pairs"], "hookean", case["spring_k"], case["spring_r"], x)[0]
        F = (S + Fs) + case["ext"]
        x = x + case["dt"] * (case["mob_trans"][:, None] * F)
        low = min(low, crossed_gap(case, x))
    return x, low


# ---- the input of tests/cpp/backbone_collision_step_app ------------------------------------------------------------------------
def write_app_input(case, path):
    """read_chain_input's file: uint64 n, m, then center, radius, mob_trans (float64), then the pairs (int32)"""
    with open(path, "wb") as f:
        np.array([case["n"], case["pairs"].shape[0]], dtype=np.uint64).tofile(f)
        for a in (case["center"], case["radius"], case["mob_trans"]):
            np.ascontiguousarray(a, dtype=np.float64).tofile(f)
        case["pairs"].astype(np.int32).tofile(f)


def app_arguments(case, steps):
    """the command line of backbone_collision_step_app after the input file"""
    law = dict(scm.DEFAULTS, youngs_modulus=case["youngs_modulus"], poisson_ratio=case["poisson_ratio"])
    nums = [case["dt"], case["search_buffer"], case["spring_k"], case["spring_r"], case["kt"], case["viscosity"],
            law["youngs_modulus"], law["poisson_ratio"], SEGMENT_RADIUS, SKIN, law["epsilon"], law["sigma"], law["cutoff"]]
    return [str(int(steps)), case["mode"], case["kind"]] + [repr(float(v)) for v in nums]
