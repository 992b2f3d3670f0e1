"""The timestep composition of the hot path -- what the reference's step loops call, in their order
(scrap/lcp_spheres/NgpLcp.cpp:835-920; operator pipeline of
scrap/parameter_interface/alens/tests/performance_tests/Bacteria.cpp:755-805):

    compute_aabb -> GenNeighborLinks.generate (rebuild only when the search buffer is violated)
                 -> signed separation + contact normal (+ lever arms) per link
                 -> resolve_collisions: BBPGD on the LCP  0 <= dt D^T M D lambda + sep  _|_  lambda >= 0
                 -> Euler update x += dt U (and q <- rotate(q, W dt) for rods)

contact_model="hertz" replaces the solve by the reference's Hertzian soft-contact force (the same app's contact stage,
Bacteria.cpp:755-848; scrap/lcp_spheres/NGPSpheres2.cpp:192-240):

    ... -> signed separation + contact normal -> Hertz force per linker (EvaluateLinkerPotentials)
        -> force / torque summed per body and dry drag U = M D f (LinkerPotentialForceReduction +
           compute_generalized_velocity: the contact operator's body sweep, no solve) -> Euler update

growth_rate= adds the colony step of the same app (Bacteria.cpp:1033-1080) in front of the AABBs:

    divide_bacteria (rods longer than division_length split in two, children appended as rows n + k)
        -> grow_bacteria (every length += dt * growth_rate) -> ... contact step as above
    with the rebuild rule of growing bodies: births, or some AABB corner moved by >= the search buffer since the last
    build (check_update_neighbor_list, :685-748) -- the centre rule is not consulted.

springs= / brownian_kt= add the bead-spring chain step of the chromatin app (spheres only; NgpHP1.cpp:3802-3990):

    ... -> broad phase -> spring forces F (+ external_force) -> U_ext = M F + U_brown
        -> contacts, q = sep + dt D^T U_ext (ContactOperator.constraint_rate) -> solve (or Hertz f)
        -> U = U_ext + M D lambda -> Euler update

crosslinkers= adds the kinetic Monte Carlo stage of the HP1 app to the chain step (HP1.cpp:4728-4739):

    ... -> broad phase, and the candidate list of the crosslinkers (its own search and rebuild rule)
        -> KMC at the positions of the start of the step: right heads bind and unbind
        -> spring forces + the doubly bound crosslinkers as springs (+ external_force) -> the chain step as above

periphery= / active_forces= add the last two force terms of that app's step (HP1.cpp:4733-4741, :4839-4842): the wall
of the nucleus and the active euchromatin force dipoles, in the reference's order:

    ... -> crosslinker KMC -> active sampling (springs whose time has come switch on or off)
        -> spring forces -> crosslinker springs -> periphery force -> active force dipoles (+ external_force)
        -> the chain step as above -> Euler update -> the active springs' timers advance by dt

hydrodynamics= adds the long-range hydrodynamic velocity of the same app's default configuration to the chain step
(HP1.cpp:4744-4803; compute_rpy_hydro :3942-4059), a velocity stage outside the solver:

    ... -> forces F -> U_ext = M F -> += U_brown -> every update_every-th step u_hydro = sum_s K(x_t - x_s) F_s
        (RPYC, RPY or Stokeslet, all pairs) -> += u_hydro (every step) -> contacts -> the chain step as above

hydrodynamics=dict(..., contact_forces=True) with contact_model="hertz" is that step in the reference's own order
(HP1.cpp:4728-4803): the Hertz force is the first term of the force field, so the dry velocity, the hydrodynamic
velocity and the periphery's no-slip correction all see it, and no body sweep follows:

    ... -> broad phase -> contacts -> Hertz force per linker -> operator -> F = D f (ContactOperator.body_force)
        -> += springs, crosslinkers, periphery, active, external force -> U_ext = M F + U_brown
        -> every update_every-th step u_hydro = hydro(F) (+ the periphery's correction of F) -> U_ext += u_hydro
        -> U = U_ext -> Euler update

hydrodynamics=dict(..., in_solve=True) with contact_model="lcp" solves the LCP against the hydrodynamic mobility, as the
reference's newer chromatin app does (resolve_collisions over an ApplyMobilityOp, NgpHP1.cpp:1487-1645: every BBPGD
iteration is F = D lambda -> U = M F -> sdot = D^T U with M = RPY + local drag, :833-925, or with the no-slip periphery as
well, :927-1023): the force stage, U_ext and q = sep + dt D^T U_ext are the step's above, and

    ... -> solve 0 <= lambda _|_ dt D^T M_h D lambda + q >= 0, M_h = m_t + hydro_kind (+ the periphery's correction) at
        the current positions (ops.solve_lcp(mobility=)) -> U = U_ext + M_h D lambda -> Euler update

backbone_collision= adds the excluded volume of that app, which acts between the backbone segments that join consecutive
beads, not between the bead spheres (compute_hertzian_contact_forces, HP1.cpp:4356-4496: the first term of its force
field, :4737); contact_model="none" then leaves the sphere contact out altogether, the reference's own configuration:

    ... -> segment list (rebuilt when a segment box has moved by skin / 2) -> crosslinker KMC -> active sampling
        -> backbone segment contacts (Hertz or WCA; after D f, where that is the first term) -> spring forces -> ...
        -> U_ext as above [-> contacts -> solve or Hertz sweep, unless contact_model="none": U = U_ext] -> Euler update

hertz_friction= replaces the frictionless Hertz force by the reference's frictional rod contact with a per-pair
tangential history (SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:384-518, run every step by
CollidingOverdampedFrictionalSperm.cpp:1553-1731):

    ... -> broad phase (on a rebuild: the history is carried to the new list) -> contacts
        -> frictional force per linker from the previous step's body velocities (a vector per contact)
        -> operator build / refresh -> body_sweep_vector -> U = M D F (+ U_ext = M F_ext) -> Euler update

FilamentStepper is the other half of that app's step, the centerline-twist rod forces that make chained nodes a filament
(CollidingOverdampedFrictionalSperm.cpp:1999-2027):

    advance (disable_twist, monolayer, old <-> new edge state, x += dt v, transient fields zeroed)
        -> edge pass + node pass: elastic forces and twist torques at x(t + dt) (+ external_force)
        -> node drag: the velocities the next advance uses

Everything is device resident; host logic here only sequences library calls.
"""
import math

from dataclasses import dataclass, field

import numpy as np
import torch

from . import ops, synth

# The chain step's statistics array, read once per step (layout: DESIGN.md 5h, shared with the C++ step apps):
# name -> (first mode that writes it, float64 slot, int32 lane of that slot or None for the float64 itself)
STATS = {
    "max_overlap": ("chain", 0, None), "max_spring_length": ("chain", 1, None),
    "springs_overstretched": ("chain", 2, 0),
    "crosslinker_binds": ("crosslinkers", 3, 0), "crosslinker_unbinds": ("crosslinkers", 3, 1),
    "max_crosslinker_length": ("crosslinkers", 4, None), "crosslinkers_overstretched": ("crosslinkers", 5, 0),
    "max_periphery_overlap": ("nucleus", 6, None), "periphery_colliding": ("nucleus", 7, 0),
    "active_springs": ("nucleus", 7, 1), "active_switches_on": ("nucleus", 8, 0),
    "active_switches_off": ("nucleus", 8, 1),
    "crosslinker_periphery_bound": ("crosslinkers", 5, 1)}
STATS_LENGTH = {"chain": 3, "crosslinkers": 6, "nucleus": 9}  # float64 slots of the array, by the last mode switched on
# two-int records that one kernel writes at once: name -> its entries, lanes 0 and 1 of one slot
STAT_PAIRS = {"crosslinker_events": ("crosslinker_binds", "crosslinker_unbinds"),
              "active_switches": ("active_switches_on", "active_switches_off")}


def stat(buf, name):
    """the entry `name` of a statistics array, for a kernel to write: a float64 [1] view, an int32 [1] view, or the
    int32 [2] view of a pair of STAT_PAIRS"""
    first, second = STAT_PAIRS.get(name, (name, None))
    _, slot, lane = STATS[first]
    if lane is None:
        return buf[slot:slot + 1]
    return buf.view(torch.int32)[2 * slot + lane:2 * slot + lane + (1 if second is None else 2)]


def read_stats(buf):
    """one copy of a statistics array to the host -> {name: value} of the entries the array is long enough to hold"""
    h = buf.cpu()
    f, i = h.tolist(), h.view(torch.int32).tolist()
    return {name: f[slot] if lane is None else i[2 * slot + lane]
            for name, (_, slot, lane) in STATS.items() if slot < len(f)}


@dataclass
class StepStats:
    num_bodies: int = 0
    num_contacts: int = 0
    rebuilt: bool = False
    num_iters: int = 0
    residual: float = 0.0
    converged: bool = False
    timings_ms: dict = field(default_factory=dict)
    max_overlap: float = 0.0  # contact_model="hertz": max(0, -sep) over the step's contacts (what dt is chosen from)
    num_born: int = 0  # growth mode: bodies that divided this step (their children are rows n_before + k)
    max_spring_length: float = 0.0  # springs=: the longest spring at the start of the step
    springs_overstretched: int = 0  # ... "fenewca": the bonds clamped at r_max - 1e-4 (the other FENE kind raises)
    angular_degenerate: int = 0        # angular_springs=: triplets with an arm of zero length (the step raises)
    max_angle_deviation: float = 0.0   # ... the largest |cos(theta) - cos(rest_angle)| at this step's force evaluation
    num_sliding: int = 0  # hertz_friction=: contacts whose tangential force was capped at mu |F_n| this step
    crosslinker_bound: int = 0    # crosslinkers=: doubly bound crosslinkers after this step's KMC
    crosslinker_binds: int = 0    # ... right heads that bound this step
    crosslinker_unbinds: int = 0  # ... and that unbound
    max_crosslinker_length: float = 0.0  # ... the longest doubly bound crosslinker at this step's force evaluation
    crosslinker_periphery_bound: int = 0  # ... periphery_sites=: of crosslinker_bound, those bound to a periphery site
    periphery_colliding: int = 0         # periphery=: beads in contact with the wall at this step's force evaluation
    max_periphery_overlap: float = 0.0   # ... the deepest of them (ellipsoid_fast: the largest level-set value)
    active_springs: int = 0              # active_forces=: springs in the active state at this step's force evaluation
    active_switches: tuple = (0, 0)      # ... springs that switched (on, off) this step
    max_stretch: float = 0.0               # FilamentStepper: the largest |l - l0| / l0 over the edges at the force evaluation
    max_curvature_deviation: float = 0.0   # ... the largest component of |kappa - kappa_rest| over the elements
    kinetic_energy: float = 0.0            # ... dynamics=: the kinetic energy of the velocities the corrector wrote
    num_pairs: int = 0  # FilamentStepper(contacts=): segment pairs in the neighbour list (max_overlap, num_sliding, rebuilt too)
    max_segment_overlap: float = 0.0   # backbone_collision=: max(0, -sep) over the force branch, corrected end segments included
    segment_contacts: int = 0          # ... segment pairs in the force branch at this step's force evaluation
    num_segment_pairs: int = 0         # ... segment pairs in the neighbour list
    segment_list_rebuilt: bool = False  # ... whether this step rebuilt that list


class ContactStepper:
    """One rank's bodies (spheres, spherocylinders, or a mix with ellipsoids) and the per-timestep contact resolution."""

    def __init__(self, kind, center, radius, quat=None, length=None, *, dt=5e-3, viscosity=1e-3, search_buffer=0.25,
                 search_kind=ops.SEARCH_AABB, periodic_box=None, cfg=None, warm_start=False, mob_trans=None,
                 mob_rot=None, rod_kinematics=True, kinds=None, shape=None, friction=None, contact_cutoff=None,
                 conservative_ellipsoid_box=False, friction_method="apgd", contact_model="lcp", youngs_modulus=1000.0,
                 poisson_ratio=0.3, growth_rate=None, division_length=None, capacity=None, ids=None, springs=None,
                 brownian_kt=None, rng_keys=None, rng_counter=None, hertz_friction=None, hertz_damping=(0.0, 0.0),
                 hertz_density=1.0, crosslinkers=None, periphery=None, active_forces=None, hydrodynamics=None,
                 backbone_collision=None, angular_springs=None, spring_wca=None):
        """kind = "sphere" | "spherocylinder" | "mixed".  Mixed systems (BASELINE configs[4]) pass kinds [n] int32
        (0 sphere, 1 spherocylinder, 2 ellipsoid) and shape [n, 3] = (r,-,-) / (r,L,-) / (r1,r2,r3) instead of
        radius / length.
        contact_model = "lcp" (default: hard contact, BBPGD) | "hertz" (soft contact, no solve; spheres and rods only).
        youngs_modulus (E > 0) and poisson_ratio (0 < nu < 1): numbers or per-body tensors [n], Hertz mode only
        (defaults: Bacteria.cpp:1213-1214).
        growth_rate (None = off): the bacterial colony step (spherocylinders, SEARCH_AABB, either contact model, no
        friction / cutoff / warm start).  Rods with length > division_length divide, every rod grows by dt *
        growth_rate per step.  The stepper then owns grow-only storage of `capacity` rows (default n + n/8 + 16, grown
        with headroom) of which center, quat, radius, length, bounding_radius, mob_*, per-body E / nu and ids (int64,
        default arange(n)) are views of the first n rows; the caller's tensors are copied, not updated.  Default
        mobilities use the rod radius (Bacteria.cpp:807-848), which growth does not change.
        springs = (pairs [m, 2], "hookean" | "fene", k, r) and / or brownian_kt (kT >= 0): the chain step (spheres, no
        growth, friction or cutoff; springs take no periodic box).  r is the rest length (Hookean) or r_max (FENE); k and
        r numbers or per-spring arrays.  rng_keys (integers in [0, 2^63), default arange(n)) and rng_counter (default
        0) key the Philox stream of each body; the counters advance by one per step.  step(external_force=) adds a
        per-step [n, 3] force to the spring force.
        hertz_friction = mu >= 0 (None = off): the reference's frictional Hertzian rod contact with a tangential history
        per pair; needs contact_model="hertz", kind="spherocylinder" and rod_kinematics=True (free space or an
        orthorhombic box; no growth, springs or noise).  hertz_damping = (normal, tangential) >= 0 and hertz_density >= 0
        (the sphere mass of the rod radius weighs the damping) default to the reference's values.  The stepper then
        owns prev_velocity [n, 6] (zero before the first step) and tang_disp [C, 3] with the pair list it belongs to;
        step(external_force=) adds U_ext = (m_t F, 0) to the contact velocity.
        crosslinkers = dict(left=, right=None, sites=, kind=, k=, r=, bind_rate=, unbind_rate=, kt=, capture_radius=,
        skin=, keys=None, counter=None): m crosslinkers with fixed left heads at the bodies left [m] and right heads
        that bind to the bodies of the byte mask sites [n] and unbind (right [m], default = left: all singly bound); the
        chain step (spheres, free space, either contact model, with or without springs / brownian_kt).  kind / k / r:
        the spring a doubly bound crosslinker is; bind_rate (A) and unbind_rate (k_off) >= 0, kt > 0 (the Boltzmann
        weight of binding), capture_radius > 0 (no binding beyond it), skin >= 0 (buffer of the candidate search).  keys
        (integers in [0, 2^63), default arange(m)) and counter (default 0) key each crosslinker's Philox stream.  The
        stepper then owns ids [n] (int64, arange(n): the order candidates are walked in, kept by reorder_bodies).  Its
        optional key periphery_sites = dict(points= [P, 3], bind_rate=, k=, r=, unbind_rate=None, capture_radius=None)
        adds P immobile bind sites on the nuclear envelope (HP1.cpp:3340-3398) with rate constants of
        their own (unbind_rate and capture_radius default to the crosslinkers'): right may then hold -(s + 1), bound to
        site s, and a periphery-bound crosslinker is a spring between its bead and the site.  scale_periphery does not
        move the sites.
        periphery = dict(shape="sphere" | "ellipsoid" | "ellipsoid_fast", radius= (sphere) or radii= (3 semi-axes), k=,
        center=(0, 0, 0), quat=(1, 0, 0, 0)): the wall of the nucleus, a linear spring of constant k >= 0 on every bead
        that touches it ("ellipsoid": exact distance; "ellipsoid_fast": the reference's level-set force, no quat); the
        chain step (spheres, free space, either contact model).  Every bead radius must be below the smallest periphery
        radius.  scale_periphery(factor) shrinks or grows it between steps.
        active_forces = dict(springs=, sigma=, kon=, koff=, keys=None, counter=None): the springs= pairs listed in
        springs [ma] (indices, no repeats) switch on at the rate kon and off at the rate koff (> 0) and push their
        beads apart with a force of magnitude sigma while on; keys (integers in [0, 2^63), default arange(ma)) and
        counter (default 0) key each one's Philox stream.  Needs springs=.  The timers advance by dt at the end of every
        step that integrates.
        hydrodynamics = dict(kind="rpyc" | "rpy" | "stokes", radius=None, update_every=1): the long-range hydrodynamic
        velocity of the force stage's forces, added to U_ext after the noise (HP1.cpp:4744-4803); the chain step (spheres,
        free space, either contact model).  radius: the hydrodynamic radii, None (the beads' own), a number or [n]
        numbers >= 0; update_every k >= 1: recomputed on the steps 0, k, 2k, ... of this stepper and added on every
        step.  The stepper then owns u_hydro [n, 3].  "rpyc" is the accurate kind.  Its optional key
        periphery = dict(shape="sphere", radius=, spectral_order=) or dict(points=, weights=, normals=) (+ inverse=,
        skip_same_index=True) adds the no-slip correction of a confining surface to u_hydro on the same steps
        (HP1.cpp:4005-4037): the surface's boundary-integral matrix is filled and inverted at
        construction (or inverse=, a precomputed [3S, 3S] one, is loaded).  Its optional key contact_forces=True
        (contact_model="hertz" only; default False: the step above, unchanged) makes the Hertz contact force the first
        term of F, as the reference has it: contacts are evaluated before the forces, F = D f + springs + ..., the
        hydrodynamics and the periphery's correction see the contact forces, and U = U_ext with no body sweep (DESIGN.md
        5p).  With "lcp" it is refused: the multipliers do not exist when U_ext is formed.  Its optional key
        in_solve=True (contact_model="lcp" only, kind "rpyc" or "rpy", not with contact_forces; default False: the step
        above, unchanged) solves the LCP against M_h = m_t + hydro_kind (+ the periphery's correction) at the current
        positions instead of the dry m_t, so U = U_ext + M_h D lambda and every bead feels every contact;
        body_contact_force() stays D lambda, warm_start works as before, reorder_bodies is refused.
        backbone_collision = dict(kind="hertz" | "wca", radius=, skin=, youngs_modulus=1000.0, poisson_ratio=0.3,
        epsilon=1.0, sigma=1.0, cutoff=1.12246204831, segments=None, end_correction=None): frictionless contacts between
        the backbone segments (ops.SegmentContacts), a force term after the crosslinker KMC and the active
        sampling and before the springs; the chain step (spheres, free space).  segments [m, 2] defaults to the springs=
        pairs; radius a number or [m]; skin >= 0 the buffer of the segment list; end_correction None marks every segment
        with an end node that belongs to no other segment (the reference's "first or last element in chain"), a byte mask
        [m] or False overrides it.  contact_model = "none" (only with backbone_collision): no sphere list, narrow phase,
        solve or sweep; U = U_ext, num_contacts = 0 and body_contact_force() raises -- the reference's configuration.
        With "lcp" and "hertz" the segment term is one more force of the force stage.
        springs of kind "fenewca" are the Kremer-Grest bond (FENE + WCA; mundy_hip_bending.h): r is r_max,
        spring_wca = (epsilon, sigma), both > 0, default (1, 1) as the reference hard-codes them.  Such a bond never goes
        without force: a step reports the clamped ones in springs_overstretched and does not raise.
        angular_springs = (triplets [m, 3], k, rest_angle): the three-body bending term U = 1/2 k (cos(theta) -
        cos(rest_angle))^2 of the reference's AngularSpringsKernel (ops.AngularSprings; synth.chain_triplets lists a
        chain's triplets: end, end, centre); k >= 0 and rest_angle in [0, pi] numbers or per-triplet arrays.  A force term
        after the springs and before the crosslinker springs; the chain step (spheres, free space), with or without
        springs=.  A triplet with a zero arm has no force: the step raises."""
        if kind not in ("sphere", "spherocylinder", "mixed"):
            raise ValueError("kind must be 'sphere', 'spherocylinder' or 'mixed'")
        if contact_model not in ("lcp", "hertz", "none"):
            raise ValueError("contact_model must be 'lcp', 'hertz' or 'none'")
        if contact_model == "none" and backbone_collision is None:
            raise ValueError("contact_model='none' leaves no excluded volume: it needs backbone_collision=")
        self.contact_model = contact_model
        if contact_model == "hertz":  # (checked before anything reaches the device)
            for what, v in (("friction", friction), ("contact_cutoff", contact_cutoff)):
                if v is not None:
                    raise ValueError("contact_model='hertz' takes no %s (the LCP path's options)" % what)
            if warm_start:
                raise ValueError("contact_model='hertz' has no solve to warm-start")
            if kind == "mixed" and kinds is not None and bool((kinds == 2).any()):
                raise ValueError("contact_model='hertz' has no ellipsoid contact (the reference has no such kernel)")
            ops._material(youngs_modulus, center.shape[0], "youngs_modulus", 0.0, float("inf"))
            ops._material(poisson_ratio, center.shape[0], "poisson_ratio", 0.0, 1.0)
        self.youngs_modulus, self.poisson_ratio = youngs_modulus, poisson_ratio
        chain_only = (kind, growth_rate, hertz_friction, friction, contact_cutoff, periodic_box)
        xl_spec = None
        if crosslinkers is not None:  # (checked before anything reaches the device)
            xl_spec = self._check_crosslinkers(chain_only, center.shape[0], crosslinkers)
        nucleus_spec = None
        if periphery is not None or active_forces is not None:  # (checked before anything reaches the device)
            nucleus_spec = self._check_nucleus(chain_only, center.shape[0], radius, springs, periphery, active_forces)
        backbone_spec = None
        if backbone_collision is not None:  # (checked before anything reaches the device)
            backbone_spec = self._check_backbone(chain_only, center.shape[0], springs, backbone_collision)
        bending_spec = None
        if angular_springs is not None:  # (checked before anything reaches the device)
            bending_spec = self._check_bending(chain_only, center.shape[0], angular_springs)
        wca_spec = None
        if spring_wca is not None:  # (checked before anything reaches the device)
            if not isinstance(spring_wca, (tuple, list)) or len(spring_wca) != 2:
                raise ValueError("spring_wca must be (epsilon, sigma)")
            if springs is None or not isinstance(springs, (tuple, list)) or len(springs) != 4:
                raise ValueError("spring_wca needs springs=(pairs, 'fenewca', k, r_max)")
            wca_spec = ops.check_wca(springs[1], *spring_wca)
        hydro_spec = None
        if hydrodynamics is not None:  # (checked before anything reaches the device)
            if (springs is None and brownian_kt is None and crosslinkers is None and periphery is None and
                    active_forces is None and backbone_collision is None and angular_springs is None):
                raise ValueError("hydrodynamics belongs to the chain step: pass springs= or brownian_kt= (0.0: no noise)")
            self._check_chain_only("hydrodynamics", "the kernels are free-space", *chain_only)
            hydro_spec = ops.check_hydrodynamics(hydrodynamics, center.shape[0])
            if hydrodynamics.get("contact_forces", False) and contact_model != "hertz":
                raise ValueError("hydrodynamics contact_forces needs contact_model='hertz': the LCP's multipliers do not "
                                 "exist when U_ext is formed")
            if hydrodynamics.get("in_solve", False):
                # (with contact_forces=True as well: refused above under "lcp", here under any other model)
                if contact_model != "lcp":
                    raise ValueError("hydrodynamics in_solve needs contact_model='lcp': it is the mobility of the LCP")
                if hydro_spec[0] == "stokes":
                    raise ValueError("hydrodynamics in_solve needs kind 'rpyc' or 'rpy': the Stokeslet is not positive "
                                     "semi-definite at bead separations")
            if hydrodynamics.get("periphery") is not None:
                hydro_spec += (ops.check_hydro_periphery(hydrodynamics["periphery"]),)
        # the Hertz force as the first term of the chain step's force field (HP1.cpp:4737-4741) instead of a body sweep
        # after U_ext
        self.hydro_contact_forces = hydrodynamics is not None and bool(hydrodynamics.get("contact_forces", False))
        # the LCP solved against the hydrodynamic mobility (NgpHP1.cpp:1487-1645; mundy_hip_hydro_solve.h), not the dry one
        self.hydro_in_solve = hydrodynamics is not None and bool(hydrodynamics.get("in_solve", False))
        self.hertz_friction = None
        if hertz_friction is not None:  # (checked before anything reaches the device)
            self._check_hertz_friction(contact_model, kind, rod_kinematics, growth_rate, springs, brownian_kt,
                                       periodic_box, hertz_friction, hertz_damping, hertz_density)
            self.hertz_friction = float(hertz_friction)
            self.hertz_damping = (float(hertz_damping[0]), float(hertz_damping[1]))
            self.hertz_density = float(hertz_density)
        elif hertz_damping not in ((0.0, 0.0), [0.0, 0.0]) or hertz_density != 1.0:
            raise ValueError("hertz_damping and hertz_density belong to the frictional Hertz contact: pass hertz_friction")
        self.growth = growth_rate is not None
        if self.growth:  # (checked before anything reaches the device)
            self._check_growth(kind, search_kind, friction, contact_cutoff, warm_start, growth_rate, division_length,
                               radius, quat, length, periodic_box, capacity, ids)
        elif division_length is not None or capacity is not None or ids is not None:
            raise ValueError("division_length, capacity and ids belong to growth mode: pass growth_rate")
        self.chain = (springs is not None or brownian_kt is not None or crosslinkers is not None or
                      nucleus_spec is not None or backbone_spec is not None or bending_spec is not None)
        if self.chain:  # (checked before anything reaches the device)
            chain_spec = self._check_chain(kind, center.shape[0], periodic_box, friction, contact_cutoff, springs,
                                           brownian_kt, rng_keys, rng_counter)
        elif rng_keys is not None or rng_counter is not None:
            raise ValueError("rng_keys and rng_counter key the Brownian noise: pass brownian_kt")
        if kind == "spherocylinder" and (quat is None or length is None):
            raise ValueError("spherocylinders need quat and length")
        if kind == "mixed" and (quat is None or kinds is None or shape is None):
            raise ValueError("mixed systems need quat, kinds and shape")
        if friction is not None and kind != "spherocylinder":
            raise ValueError("the friction extension is wired for spherocylinders")
        self.kind = kind
        # BUILD EXTENSION, mixed systems: the tight conservative ellipsoid box in the neighbour search instead of the
        # reference's (compute_aabb.hpp:82-103), which can miss overlapping ellipsoids of general orientation
        self.conservative_ellipsoid_box = bool(conservative_ellipsoid_box)
        # BUILD EXTENSION (parity unpinned: the reference has no frictional solver): Coulomb coefficient, None = the
        # reference's frictionless LCP
        self.friction = None if friction is None else float(friction)
        # "apgd" (Mazhar et al. 2015; 10^6 rods at mu = 0.3: 2 189 sweeps from the raw packing, 318 from the relaxed one)
        # or "bbpgd" (the reference's iteration with a cone projection: 23 227 / 754)
        self.friction_method = friction_method
        self.center, self.radius, self.quat, self.length = center, radius, quat, length
        self.kinds, self.shape = kinds, shape
        self.dt, self.viscosity = float(dt), float(viscosity)
        self.box = periodic_box
        self.cfg = cfg or ops.PGDConfig(max_iters=10000, tol=1e-5)  # NgpLcp.cpp:851-852
        self.warm_start = warm_start
        # spherocylinders: lever arms as one arclength per contact (mhip_contact_op_create_rods) -- same operator up to
        # rounding, 18 % fewer bytes per solver iteration; False selects the (ra, rb) vector form
        self.rod_kinematics = bool(rod_kinematics)
        self.links = (ops.GenNeighborLinks().set_search_buffer(search_buffer).set_search_kind(search_kind)
                      .set_periodic_box(periodic_box).concretize())
        n = center.shape[0]
        # dry local drag U = F/(6 pi mu r), W = T/(8 pi mu r^3) (NgpLcp.cpp:484-486, Bacteria.cpp:810-848); the
        # per-body coefficients are set-up data computed once on the host (same numbers feed the CPU oracle)
        if kind == "sphere":
            self.bounding_radius = radius.clone()
            eff = radius
        elif kind == "mixed":
            self.bounding_radius = ops.compute_aabb_mixed(kinds, center, quat, shape)[1]
            eff = self.bounding_radius
        else:
            self.bounding_radius = ops.bounding_radius_spherocylinders(radius, length)
            # growth mode: the rod radius, constant while a rod grows (Bacteria.cpp:807-848)
            eff = radius if self.growth else self.bounding_radius
            self.seg = torch.empty((n, 8), dtype=torch.float64, device=center.device)
        if mob_trans is None:
            mt, mr = synth.dry_mobility(eff.cpu().numpy(), viscosity=self.viscosity)
            mob_trans = torch.from_numpy(mt).to(center.device)
            mob_rot = torch.from_numpy(mr).to(center.device) if kind != "sphere" else None
        self.mob_trans, self.mob_rot = mob_trans, (mob_rot if kind != "sphere" else None)
        self.op = None
        self.lam = None
        self.contacts = None
        self.work_mapping = None  # (xcd_tile, lanes_per_body) for ContactOperator.set_work_mapping: time only
        self.tiering = None       # ContactOperator.set_tiering mode (None: the library default): time only
        self.profile_next = False  # per-kernel timing of the next solve (ContactOperator.set_profiling): time only
        # BUILD OPTION (None = off, the reference's behaviour: every neighbour pair is a constraint, NgpLcp.cpp:346-373):
        # only pairs within contact_cutoff of touching become constraints of this step (ballot compaction of the
        # candidate list); the dropped pairs are checked afterwards (they must satisfy g >= 0, i.e. stay inactive) and
        # the step is redone on the full list if one does not.
        self.contact_cutoff = None if contact_cutoff is None else float(contact_cutoff)
        self.cutoff_fallbacks = 0
        self.ids = self.springs = self.rng_keys = self.rng_counter = self.crosslinkers = None
        self.xl_sources = self.xl_sites = self.periphery = self.active = self.hydro = self.backbone = None
        self.angular = None
        self._spring_wca = wca_spec
        if self.growth:
            self._init_growth(growth_rate, division_length, capacity, ids, search_buffer)
        if self.chain:
            self._init_chain(*chain_spec)
        if self.hertz_friction is not None:
            self._init_hertz_friction()
        if xl_spec is not None:
            self._init_crosslinkers(xl_spec)
        if nucleus_spec is not None:
            self._init_nucleus(*nucleus_spec)
        if hydro_spec is not None:
            self._init_hydro(*hydro_spec)
        if backbone_spec is not None:
            self._init_backbone(backbone_spec)
        if bending_spec is not None:
            self._init_bending(bending_spec)
        # the springs' own term, added to F = D f or to the segment contacts' force (the spring kernel overwrites)
        if (self.hydro_contact_forces or self.backbone is not None) and self.springs is not None:
            self._spring_term = torch.zeros((n, 3), dtype=torch.float64, device=center.device)
        # the optional modes that carry state of their own: snapshot, restore and reorder_bodies call their
        # _snapshot_<mode>() / _restore_<mode>(saved) / _renumber_<mode>(perm, inv) hooks in this order
        on = dict(growth=self.growth, friction=self.hertz_friction is not None, springs=self.springs is not None,
                  crosslinkers=self.crosslinkers is not None, periphery=self.periphery is not None,
                  active=self.active is not None, hydro=self.hydro is not None, backbone=self.backbone is not None,
                  bending=self.angular is not None)
        self._modes = [m for m, v in on.items() if v]

    @staticmethod
    def _check_chain_only(what, why_no_box, kind, growth_rate, hertz_friction, friction, contact_cutoff, box):
        """`what` (a plural) belongs to the chain step: spheres in free space, no growth, no friction of either kind"""
        if kind != "sphere":
            raise ValueError("%s are wired for spheres only (the chain step), not %r" % (what, kind))
        if growth_rate is not None:
            raise ValueError("%s do not run in growth mode" % what)
        if hertz_friction is not None:
            raise ValueError("%s take no hertz_friction (the rod contact)" % what)
        if friction is not None or contact_cutoff is not None:
            raise ValueError("%s take no friction or contact_cutoff" % what)
        if box is not None:
            raise ValueError("%s take no periodic_box (%s)" % (what, why_no_box))

    @staticmethod
    def _check_orthorhombic(what, box):
        if box is not None and np.asarray(box.cpu() if isinstance(box, torch.Tensor) else box).size != 3:
            raise ValueError("%s takes an orthorhombic periodic box (3 edge lengths)" % what)

    # -- frictional Hertz contact (FrictionalHertzianContact.cpp:384-518) -------------------------------------------------
    @staticmethod
    def _check_hertz_friction(contact_model, kind, rod_kinematics, growth_rate, springs, kt, box, mu, damping, density):
        if contact_model != "hertz":
            raise ValueError("hertz_friction needs contact_model='hertz'")
        if kind != "spherocylinder":
            raise ValueError("hertz_friction is the reference's rod-rod kernel: kind must be 'spherocylinder', not %r"
                             % kind)
        if not rod_kinematics:
            raise ValueError("hertz_friction needs rod_kinematics=True (the arclength form of the contact points)")
        if growth_rate is not None:
            raise ValueError("hertz_friction does not run in growth mode")
        if springs is not None or kt is not None:
            raise ValueError("hertz_friction takes no springs or brownian_kt")
        ContactStepper._check_orthorhombic("hertz_friction", box)
        if not isinstance(damping, (tuple, list)) or len(damping) != 2:
            raise ValueError("hertz_damping must be (normal, tangential)")
        for name, v in (("hertz_friction", mu), ("hertz_damping[0]", damping[0]), ("hertz_damping[1]", damping[1]),
                        ("hertz_density", density)):
            ops._finite_nonneg(float(v), name)

    def _init_hertz_friction(self):
        n, dev = self.center.shape[0], self.center.device
        self.prev_velocity = torch.zeros((n, 6), dtype=torch.float64, device=dev)  # the reference's StateN field
        self.tang_disp = None      # [C, 3], "j relative to i", rows of hist_pairs
        self.hist_pairs = None     # the pair list tang_disp belongs to
        self.contact_force = None  # [C, 3], on body i
        self._renumber = None      # reorder_bodies since the last carry: new index of every old body (int32)
        self._fr_stats = torch.zeros(2, dtype=torch.float64, device=dev)  # (max_overlap, num_sliding as int64 bits)
        self._fr_u_ext = None
        self._fr_has_ext = False
        self.last_carried = 0      # new pairs that found their old history row at the last carry
        self.velocity = None

    def _snapshot_friction(self):
        """the history, the list it belongs to and the previous velocities"""
        return (self.prev_velocity.clone(), None if self.tang_disp is None else self.tang_disp.clone(),
                self.hist_pairs, self._renumber)

    def _restore_friction(self, saved):
        prev, disp, pairs, renumber = saved
        self.prev_velocity.copy_(prev)
        # (a clone: the stepper updates its history in place, and the next step carries it to the list in use)
        self.tang_disp = None if disp is None else disp.clone()
        self.hist_pairs, self._renumber = (None if disp is None else pairs.clone()), renumber

    def _renumber_friction(self, perm, inv):
        """previous velocities move with their rows, the history through the inverse at the next carry"""
        self.prev_velocity = ops.gather_rows(perm, self.prev_velocity)
        self._renumber = inv if self._renumber is None else inv[self._renumber.long()].contiguous()

    def _carry_history(self):
        """tang_disp follows the neighbour list: after a rebuild, a renumbering or a restore every pair of the new list
        receives the row of the same pair of the old one, every other pair +0.0"""
        pairs = self.links.pairs
        if self.hist_pairs is pairs and self._renumber is None:
            return
        dev = self.center.device
        if self.tang_disp is None:
            self.tang_disp = torch.zeros((pairs.shape[0], 3), dtype=torch.float64, device=dev)
            self.last_carried = 0
        else:
            self.tang_disp, self.last_carried = ops.carry_contact_history(self.hist_pairs, self.tang_disp, pairs,
                                                                          new_of_old=self._renumber, want_count=True)
        self._renumber = None
        self.hist_pairs = pairs
        self.contact_force = torch.zeros((pairs.shape[0], 3), dtype=torch.float64, device=dev)

    def _hertz_friction(self, rebuilt, mark):
        """frictional soft contact: per-linker force vector from the previous step's velocities and the history, then the
        operator's vector body sweep -- U = M D F (no solve)"""
        self._carry_history()
        mark("history_carry")
        c, pairs = self.contacts, self.links.pairs
        ops.hertz_friction_force(pairs, c["sep"], c["normal"], c["s"], c["t"], self.seg, self.radius, self.prev_velocity,
                                 self.tang_disp, self.hertz_friction, self.dt, damping=self.hertz_damping,
                                 density=self.hertz_density, youngs_modulus=self.youngs_modulus,
                                 poisson_ratio=self.poisson_ratio, out=self.contact_force, stats=self._fr_stats)
        mark("hertz_force")
        self._operator(rebuilt, pairs)
        mark("operator")
        self.op.body_sweep_vector(self.contact_force)
        mark("body_sweep")
        return ops.SolveResult(num_iters=0, residual=0.0, converged=True)

    # -- bead-spring chains with thermal noise (NgpHP1.cpp:3802-3990) ----------------------------------------------------
    @staticmethod
    def _check_chain(kind, n, box, friction, contact_cutoff, springs, kt, keys, counter):
        if kind != "sphere":
            raise ValueError("springs and Brownian noise are wired for spheres only, not %r" % kind)
        if friction is not None or contact_cutoff is not None:
            raise ValueError("springs / brownian_kt take no friction or contact_cutoff")
        if springs is not None and box is not None:
            raise ValueError("springs take no periodic_box (the chains are unbounded; no minimum-image springs)")
        spec = None
        if springs is not None:
            if not isinstance(springs, (tuple, list)) or len(springs) != 4:
                raise ValueError("springs must be (pairs, 'hookean' | 'fene', k, r)")
            pairs, skind, k, r = springs
            p, _, ka, k0, ra, r0 = ops.check_springs(pairs, skind, k, r, n)
            spec = (p, skind, ka if ka is not None else k0, ra if ra is not None else r0)
        if kt is not None:
            kt = ops._finite_nonneg(float(kt), "brownian_kt")
        elif keys is not None or counter is not None:
            raise ValueError("rng_keys and rng_counter key the Brownian noise: pass brownian_kt")
        return (spec, kt, ops.check_philox_ints(keys, n, "rng_keys"),
                ops.check_philox_ints(counter, n, "rng_counter"))

    def _init_chain(self, spec, kt, keys, counter):
        n, dev = self.center.shape[0], self.center.device
        self._spring_spec = spec
        self.springs = self._new_springs() if spec is not None else None
        self.brownian_kt = kt
        self.rng_keys = (torch.arange(n, dtype=torch.int64, device=dev) if keys is None else
                         torch.from_numpy(keys).to(dev))
        self.rng_counter = (torch.zeros(n, dtype=torch.int64, device=dev) if counter is None else
                            torch.from_numpy(counter).to(dev))
        self._chain_stats = torch.zeros(STATS_LENGTH["chain"], dtype=torch.float64, device=dev)  # one read per step
        self.spring_force = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        self.u_ext = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        self.velocity = None

    def _new_springs(self):
        sp = ops.Springs(self.center.shape[0], *self._spring_spec)
        if self._spring_wca is not None:
            sp.set_wca(*self._spring_wca)
        return sp

    def _snapshot_springs(self):
        return None  # (the set is fixed: nothing to save)

    def _restore_springs(self, saved):
        pass

    def _renumber_springs(self, perm, inv):
        """spring endpoints through the inverse permutation (spring order kept): a new handle from the host copy of
        the pairs, the library has no renumbering of a spring set"""
        p, skind, k, r = self._spring_spec
        self._spring_spec = (np.ascontiguousarray(inv.cpu().numpy()[p], dtype=np.int32), skind, k, r)
        self.springs.close()
        self.springs = self._new_springs()

    # -- angular springs (AngularSpringsKernel.cpp:107-197; SpringsUpdated.cpp:1843-1862) ------------------------------------
    @staticmethod
    def _check_bending(chain_only, n, spec):
        ContactStepper._check_chain_only("angular_springs", "no minimum-image angles", *chain_only)
        if not isinstance(spec, (tuple, list)) or len(spec) != 3:
            raise ValueError("angular_springs must be (triplets, k, rest_angle)")
        t, ka, k0, aa, a0 = ops.check_angular_springs(n, *spec)
        return t, (ka if ka is not None else k0), (aa if aa is not None else a0)

    def _init_bending(self, spec):
        self.angular = ops.AngularSprings(self.center.shape[0], *spec)
        # (max_angle_deviation, angular_degenerate in the low int32 of the second word): an array of its own, read with
        # the chain step's -- the layout of that one is shared with the C++ apps and stays as it is
        self._bending_stats = torch.zeros(2, dtype=torch.float64, device=self.center.device)

    def _snapshot_bending(self):
        return None  # (the set is fixed: nothing to save)

    def _restore_bending(self, saved):
        pass

    def _renumber_bending(self, perm, inv):
        self.angular.renumber(inv)  # the three indices of every triplet; order, k and rest angles stay

    # -- crosslinkers that bind and unbind (HP1.cpp:3264-3748, :4728-4739) ------------------------------------------------
    _XL_KEYS = ("left", "right", "sites", "kind", "k", "r", "bind_rate", "unbind_rate", "kt", "capture_radius", "skin",
                "keys", "counter", "periphery_sites")

    @staticmethod
    def _check_crosslinkers(chain_only, n, spec):
        ContactStepper._check_chain_only("crosslinkers", "no minimum-image crosslinkers", *chain_only)
        ops.check_dict_spec(spec, "crosslinkers", ContactStepper._XL_KEYS,
                            optional=("right", "keys", "counter", "periphery_sites"))
        per = None
        if spec.get("periphery_sites") is not None:
            per = ops.check_periphery_sites(spec["periphery_sites"], spec["kind"], spec["unbind_rate"],
                                            spec["capture_radius"])
        checked = ops.check_crosslinkers(n, spec["left"], spec.get("right"), spec["sites"], spec["kind"], spec["k"],
                                         spec["r"], spec["bind_rate"], spec["unbind_rate"], spec["kt"],
                                         spec["capture_radius"], num_periphery_sites=0 if per is None else per[0].shape[0])
        skin = ops._finite_nonneg(spec["skin"], "crosslinker skin")
        m = checked[0].shape[0]
        return (checked, spec["kind"], skin, ops.check_philox_ints(spec.get("keys"), m, "crosslinker keys"),
                ops.check_philox_ints(spec.get("counter"), m, "crosslinker counter"), per)

    def _init_crosslinkers(self, xl_spec):
        (le, ri, si, _, k, r, a, off, kt, cap), skind, skin, keys, counter, per = xl_spec
        n, dev = self.center.shape[0], self.center.device
        m = le.shape[0]
        self.xl_site_links = self.xl_site_points = None
        if per is None:
            self.crosslinkers = ops.Crosslinkers(n, le, ri, si, skind, k, r, a, off, kt, cap)
        else:  # a periphery-bound initial state arrives through set_state, after the sites are set
            pts, pa, pk, pr, poff, pcap = per
            self.crosslinkers = ops.Crosslinkers(n, le, np.where(ri < 0, le, ri), si, skind, k, r, a, off, kt, cap)
            self.xl_site_points = torch.from_numpy(pts).to(dev)
            self.crosslinkers.set_periphery_sites(self.xl_site_points, pa, pk, pr, poff, pcap)
            if (ri < 0).any():
                self.crosslinkers.set_state(None, torch.from_numpy(ri).to(dev))
            # the candidate search over beads followed by sites: the beads' rows are copied in every step, the sites
            # never move, so the displacement rule rebuilds the list when a bead has moved
            P = pts.shape[0]
            self._xl_site_all = torch.cat([self.center, self.xl_site_points])
            self._xl_site_reach = torch.full((n + P,), 0.5 * pcap, dtype=torch.float64, device=dev)
            self._xl_site_targets = torch.cat([torch.zeros(n, dtype=torch.uint8, device=dev),
                                               torch.ones(P, dtype=torch.uint8, device=dev)])
        self.crosslinker_skin = skin
        self.xl_keys = torch.arange(m, dtype=torch.int64, device=dev) if keys is None else torch.from_numpy(keys).to(dev)
        self.xl_counter = (torch.zeros(m, dtype=torch.int64, device=dev) if counter is None else
                           torch.from_numpy(counter).to(dev))
        self.crosslinker_bound = int((ri != le).sum())
        # per-body arrays of the candidate search: who carries a crosslinker, who is a bind site, every body's reach
        src = np.zeros(n, dtype=np.uint8)
        src[le] = 1
        self.xl_sources, self.xl_sites = torch.from_numpy(src).to(dev), torch.from_numpy(si).to(dev)
        self.xl_reach = torch.full((n,), 0.5 * cap, dtype=torch.float64, device=dev)
        self.ids = torch.arange(n, dtype=torch.int64, device=dev)
        self._chain_stats = torch.zeros(STATS_LENGTH["crosslinkers"], dtype=torch.float64, device=dev)
        self.xl_links = None
        self.crosslinker_rebuilds = 0  # candidate lists built so far
        self.crosslinker_site_rebuilds = 0  # ... and periphery candidate lists
        self._new_crosslinker_search()

    def _new_crosslinker_search(self):
        """the candidate search: bounding spheres of radius capture_radius / 2 (+ skin), sources the beads that carry a
        crosslinker, targets the bind sites; a fresh builder, since the masks follow the body numbering"""
        def search(old, sources, targets):
            if old is not None:
                old.close()
            return (ops.GenNeighborLinks().set_search_buffer(self.crosslinker_skin).set_search_kind(ops.SEARCH_SPHERES)
                    .set_enforce_source_target_symmetry(True).acts_on(sources, targets).concretize())
        self.xl_links = search(self.xl_links, self.xl_sources, self.xl_sites)
        if self.xl_site_points is not None:  # periphery_sites=: sources the same beads, targets the sites
            src = torch.cat([self.xl_sources, torch.zeros_like(self._xl_site_targets[self.xl_sources.shape[0]:])])
            self.xl_site_links = search(self.xl_site_links, src, self._xl_site_targets)

    def crosslinker_kmc(self):
        """candidate list (rebuilt by the displacement rule, rows sorted by id once per build) -> one KMC step at the
        current positions; the event counts stay on the device (self._chain_stats)"""
        if self.xl_links.generate(None, self.center, self.xl_reach):
            self.crosslinker_rebuilds += 1
            self.crosslinkers.set_candidates(self.xl_links.row_ptr, self.xl_links.col, self.ids)
        if self.xl_site_links is None:
            self.crosslinkers.kmc_step(self.center, self.dt, self.xl_keys, self.xl_counter,
                                       events=stat(self._chain_stats, "crosslinker_events"))
            return
        n = self.center.shape[0]
        self._xl_site_all[:n].copy_(self.center)
        if self.xl_site_links.generate(None, self._xl_site_all, self._xl_site_reach):
            self.crosslinker_site_rebuilds += 1
            self.crosslinkers.set_periphery_candidates(self.xl_site_links.row_ptr, self.xl_site_links.col, col_offset=n)
        self.crosslinkers.kmc_step(self.center, self.dt, self.xl_keys, self.xl_counter,
                                   events=stat(self._chain_stats, "crosslinker_events"),
                                   periphery_bound=stat(self._chain_stats, "crosslinker_periphery_bound"))

    def crosslinker_state(self):
        """-> (left, right) int32 [m] device tensors in the current body numbering; right == left: singly bound,
        right == -(s + 1): bound to periphery site s"""
        return self.crosslinkers.state(self.center.device)

    def _snapshot_crosslinkers(self):
        """both heads (in the numbering of the snapshot), keys, counters, bound count"""
        return self.crosslinker_state() + (self.xl_keys.clone(), self.xl_counter.clone(), self.crosslinker_bound)

    def _restore_crosslinkers(self, saved):
        left, right, keys, counter, self.crosslinker_bound = saved
        self.crosslinkers.set_state(left, right)
        self.xl_keys.copy_(keys)
        self.xl_counter.copy_(counter)

    def _renumber_crosslinkers(self, perm, inv):
        """heads through the inverse permutation, and a new search"""
        self.crosslinkers.renumber(inv)
        self._new_crosslinker_search()

    # -- the nuclear periphery and the active force dipoles (HP1.cpp:4063-4354) -------------------------------------------
    _ACTIVE_KEYS = ("springs", "sigma", "kon", "koff", "keys", "counter")

    @staticmethod
    def _check_nucleus(chain_only, n, radius, springs, periphery, active):
        ContactStepper._check_chain_only("periphery / active_forces", "the nucleus is a closed wall", *chain_only)
        per = act = None
        if periphery is not None:
            per = ops.check_periphery(periphery)
        if active is not None:
            ops.check_dict_spec(active, "active_forces", ContactStepper._ACTIVE_KEYS, optional=("keys", "counter"))
            if springs is None:
                raise ValueError("active_forces needs springs=: its springs are indices into those pairs")
            if not isinstance(springs, (tuple, list)) or len(springs) != 4:
                raise ValueError("springs must be (pairs, 'hookean' | 'fene', k, r)")
            pairs = springs[0]
            p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
            p = p.reshape(-1, 2)
            idx = active["springs"]
            idx = idx.detach().cpu().numpy() if isinstance(idx, torch.Tensor) else np.asarray(idx)
            if idx.ndim != 1 or not (idx.dtype.kind in "iu" or idx.size == 0):
                raise ValueError("active_forces springs must be integers of shape [ma], got %s %s" % (idx.dtype, idx.shape))
            idx = idx.astype(np.int64)
            if idx.size and (idx.min() < 0 or idx.max() >= p.shape[0]):
                raise ValueError("active_forces springs: an index outside [0, %d)" % p.shape[0])
            if np.unique(idx).size != idx.size:
                raise ValueError("active_forces springs: a spring is listed more than once")
            act = ops.check_active_springs(n, p[idx], active["sigma"], active["kon"], active["koff"],
                                           active.get("keys"), active.get("counter"))
        # the one read of the beads (a reduction and a readback for a device tensor): after both dicts have passed
        rmax = float(radius.max()) if radius.shape[0] else 0.0
        if per is not None and rmax >= min(per[1]):
            raise ValueError("periphery: a bead radius %g >= the smallest periphery radius %g" % (rmax, min(per[1])))
        return per, act, rmax

    def _init_nucleus(self, per, act, rmax):
        dev = self.center.device
        self._max_bead_radius = rmax
        if per is not None:
            self.periphery = dict(shape=per[0], radii=list(per[1]), k=per[2], center=list(per[3]), quat=list(per[4]))
        if act is not None:
            self.active = ops.ActiveSprings(self.center.shape[0], *act)
        self._chain_stats = torch.zeros(STATS_LENGTH["nucleus"], dtype=torch.float64, device=dev)

    def _periphery_spec(self):
        p = self.periphery
        return p["shape"], p["radii"], p["k"], p["center"], p["quat"]

    def scale_periphery(self, factor):
        """the compression run (HP1.cpp:4715-4726): every periphery radius *= factor, between steps"""
        if self.periphery is None:
            raise ValueError("scale_periphery needs periphery=")
        factor = float(factor)
        if not (factor > 0.0 and factor < math.inf):
            raise ValueError("scale_periphery: factor must be finite and > 0, got %r" % factor)
        radii = [r * factor for r in self.periphery["radii"]]
        if not all(r < math.inf for r in radii) or self._max_bead_radius >= min(radii):
            raise ValueError("scale_periphery: a bead radius %g >= the smallest periphery radius %g"
                             % (self._max_bead_radius, min(radii)))
        self.periphery["radii"] = radii

    def _snapshot_periphery(self):
        return list(self.periphery["radii"])  # its size (scale_periphery)

    def _restore_periphery(self, saved):
        self.periphery["radii"] = list(saved)

    def _renumber_periphery(self, perm, inv):
        pass

    def active_state(self):
        """-> (state int32, next_time, elapsed, counter int64) [ma] device tensors of the active springs (copies)"""
        return self.active.state(self.center.device)

    def _snapshot_active(self):
        return self.active_state()  # states, timers and counters

    def _restore_active(self, saved):
        self.active.set_state(*saved)

    def _renumber_active(self, perm, inv):
        self.active.renumber(inv)  # endpoints; states and timers stay

    # -- contacts between backbone segments (HP1.cpp:4356-4496) -------------------------------------------------------------
    @staticmethod
    def _check_backbone(chain_only, n, springs, spec):
        ContactStepper._check_chain_only("backbone_collision segments", "no minimum-image segments", *chain_only)
        ops.check_dict_spec(spec, "backbone_collision", ops.SEGMENT_CONTACT_KEYS,
                            optional=tuple(ops.SEGMENT_CONTACT_DEFAULTS))
        spec = dict(spec)
        if spec.get("segments") is None:
            if springs is None:
                raise ValueError("backbone_collision needs segments= or springs=: its segments default to the spring pairs")
            if not isinstance(springs, (tuple, list)) or len(springs) != 4:
                raise ValueError("springs must be (pairs, 'hookean' | 'fene', k, r)")
            spec["segments"] = springs[0]
        ends, ra, r0, corr, _ = ops.check_segment_contacts(n, spec)
        # host copies: what _renumber_backbone makes the next handle from
        spec.update(segments=ends, radius=ra if ra is not None else r0, end_correction=corr)
        return spec

    def _init_backbone(self, spec):
        self._backbone_spec = spec
        self.backbone = ops.SegmentContacts(self.center.shape[0], **spec)
        # (bits of the double max overlap, linkers in the force branch): read once, at the end of the step
        self._backbone_stats = torch.zeros(2, dtype=torch.int64, device=self.center.device)
        self._backbone_stale = False   # restore(): the next update rebuilds the list whatever has moved
        self._backbone_rebuilt = False

    def _snapshot_backbone(self):
        return None  # (the forces do not depend on when the list was built: nothing to save)

    def _restore_backbone(self, saved):
        self._backbone_stale = True

    def _renumber_backbone(self, perm, inv):
        """segment ends through the inverse permutation (segment order kept): a new handle from the host copy of the
        ends, whose first update builds its list"""
        spec = self._backbone_spec
        spec["segments"] = np.ascontiguousarray(inv.cpu().numpy()[spec["segments"]], dtype=np.int32)
        self.backbone.close()
        self.backbone = ops.SegmentContacts(self.center.shape[0], **spec)

    # -- n-body hydrodynamics as a velocity stage (HP1.cpp:3942-4059, :4744-4803) -----------------------------------------
    def _init_hydro(self, kind, radius, every, periphery=None):
        n, dev = self.center.shape[0], self.center.device
        self.hydro = dict(kind=kind, update_every=every)
        self.hydro_radius = None if radius is None else torch.from_numpy(radius).to(dev)  # None: the beads' own
        self.u_hydro = torch.zeros((n, 3), dtype=torch.float64, device=dev)  # the stored velocity, added every step
        self.hydro_step = 0  # the reference's timestep_index_ of `% hydro_update_frequency_ == 0`
        self._hydro_ws = ops.HydroWorkspace()
        # after reorder_bodies: (the row of every bead of the constructor's numbering, that number of every row), int32.
        # The hydrodynamics are evaluated in the constructor's numbering (_hydro_velocity)
        self._hydro_rows = self._hydro_numbers = None
        self.hydro_periphery = None
        if periphery is not None:  # the surface, its matrix and the inverse: built once, here
            to = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)  # noqa: E731
            hp = ops.HydroPeriphery(to(periphery["points"]), to(periphery["weights"]), to(periphery["normals"]),
                                    self.viscosity)
            inverse = periphery["inverse"]
            if inverse is None:
                hp.fill_matrix()
                self.hydro["periphery_min_pivot"] = hp.invert()
            else:
                if not isinstance(inverse, torch.Tensor):
                    inverse = torch.from_numpy(np.ascontiguousarray(inverse, dtype=np.float64))
                hp.set_inverse(inverse.to(device=dev, dtype=torch.float64).contiguous())
            self.hydro_periphery = hp
            self.hydro["skip_same_index"] = periphery["skip_same_index"]

    def _snapshot_hydro(self):
        """the stored velocity, the step counter, the hydrodynamic radii and the numbering the rows are in"""
        return (self.u_hydro.clone(), self.hydro_step, None if self.hydro_radius is None else self.hydro_radius.clone(),
                self._hydro_rows, self._hydro_numbers)  # (the two maps are replaced, never written: no copies)

    def _restore_hydro(self, saved):
        u, self.hydro_step, radius, self._hydro_rows, self._hydro_numbers = saved
        self.u_hydro.copy_(u)
        if radius is not None:
            self.hydro_radius.copy_(radius)

    def _renumber_hydro(self, perm, inv):
        """the stored velocity and the radii move with their rows; the two maps to and from the constructor's numbering
        compose with the permutation"""
        self.u_hydro = ops.gather_rows(perm, self.u_hydro)
        if self.hydro_radius is not None:
            self.hydro_radius = ops.gather_rows(perm, self.hydro_radius)
        if self._hydro_rows is None:
            self._hydro_rows, self._hydro_numbers = inv, perm
        else:
            self._hydro_rows = inv[self._hydro_rows.long()]
            self._hydro_numbers = self._hydro_numbers[perm.long()]

    def _hydro_velocity(self, force):
        """every update_every-th step u_hydro = hydro(F) of the force stage's F; every step u_ext[:, :3] += u_hydro.

        hydro(F) is evaluated in the constructor's numbering, whatever reorder_bodies has done since: the all-pairs sums
        walk the sources in index order and skip_same_index pairs surface node i with bead i (as the reference does, which
        never renumbers), so u_hydro of a bead is the same in bits in any order of the rows.  After a reorder this costs
        three row gathers before and one after the O(n^2) sums; before one, nothing."""
        if self.hydro_step % self.hydro["update_every"] == 0:
            if force is None:
                self.u_hydro.zero_()
            else:
                center, radius = self.center, self.radius if self.hydro_radius is None else self.hydro_radius
                rows, u = self._hydro_rows, self.u_hydro
                if rows is not None:
                    center, radius, force = (ops.gather_rows(rows, t) for t in (center, radius, force))
                    u = torch.empty_like(self.u_hydro)
                ops.hydro_velocity(self.hydro["kind"], self.viscosity, center, radius, force, out=u,
                                   workspace=self._hydro_ws)
                if self.hydro_periphery is not None:  # the no-slip correction of the periphery, into the same u_hydro
                    self.hydro_periphery.correct(self.hydro["kind"], center, radius, force, u,
                                                 skip_same_index=self.hydro["skip_same_index"],
                                                 workspace=self._hydro_ws)
                if rows is not None:
                    self.u_hydro = ops.gather_rows(self._hydro_numbers, u)
        self.hydro_step += 1
        ops.hydro_add_velocity(self.u_hydro, self.u_ext)

    def _force_stage(self, external_force):
        """the force stage in the reference's order (HP1.cpp:4733-4741): crosslinker KMC, active sampling, backbone
        segment contacts, springs, angular springs, crosslinker springs, periphery, active force dipoles, external force;
        every term after the first that writes is added into self.spring_force.  The segment list is brought up to date first, on the
        positions of the start of the step.  With no such term the caller's external_force (or None: no force at all) is
        returned as it is, not copied.  With hydrodynamics contact_forces the buffer already holds the contact force
        F = D f (contact_forces()), the first term as in the reference, and every term here is added to it:
        F = ((((((D f + F_backbone) + F_spring) + F_angular) + F_crosslinker) + F_periphery) + F_active) + F_ext, each + one
        rounding, a term that is off left out."""
        st, force, written = self._chain_stats, self.spring_force, self.hydro_contact_forces
        if self.backbone is not None:
            self._backbone_rebuilt = self.backbone.update(self.center, force_rebuild=self._backbone_stale)
            self._backbone_stale = False
        if self.crosslinkers is not None:
            self.crosslinker_kmc()
        if self.active is not None:
            self.active.sample(switches=stat(st, "active_switches"))
        if self.backbone is not None:
            self.backbone.force(self.center, out=force, accumulate=written, stats=self._backbone_stats)
            written = True
        if self.springs is not None and written:  # (the spring kernel overwrites: its term goes through a buffer of its own)
            self.springs.force(self.center, out=self._spring_term,
                               stats=(stat(st, "springs_overstretched"), stat(st, "max_spring_length")))
            ops.axpby(1.0, self._spring_term.view(-1), 1.0, force.view(-1))
        elif self.springs is not None:
            self.springs.force(self.center, out=force,
                               stats=(stat(st, "springs_overstretched"), stat(st, "max_spring_length")))
            written = True
        if self.angular is not None:  # (SpringsUpdated.cpp:1844: one execute over both spring parts)
            bs = self._bending_stats
            self.angular.force(self.center, out=force, accumulate=written,
                               stats=(bs.view(torch.int32)[2:3], bs[0:1]))
            written = True
        if self.crosslinkers is not None:
            self.crosslinkers.force(self.center, out=force, accumulate=written,
                                    stats=(stat(st, "crosslinkers_overstretched"), stat(st, "max_crosslinker_length")))
            written = True
        if self.periphery is not None:
            ops.periphery_force(self._periphery_spec(), self.center, self.radius, out=force, accumulate=written,
                                stats=(stat(st, "periphery_colliding"), stat(st, "max_periphery_overlap")))
            written = True
        if self.active is not None:
            self.active.force(self.center, out=force, accumulate=written, active=stat(st, "active_springs"))
            written = True
        if not written:
            return external_force
        if external_force is not None:
            ops.axpby(1.0, external_force.reshape(-1), 1.0, force.view(-1))
        return force

    def external_velocity(self, external_force=None, mark=lambda name: None):
        """U_ext = M (F_spring + F_crosslinker + F_periphery + F_active + F_ext) + U_brown (+ u_hydro) into self.u_ext
        (the rng counters advance; with crosslinkers, their KMC step runs first, then the active springs' sampling);
        mark(name) is told the stages (springs_brownian[, hydrodynamics]) as they are issued.  With hydrodynamics
        contact_forces, contact_forces() comes first: it has zeroed the statistics and written max_overlap and F = D f"""
        if not self.hydro_contact_forces:
            self._chain_stats.zero_()
        force = self._force_stage(external_force)
        ops.drag_velocity(self.mob_trans, force, out=self.u_ext)
        if self.brownian_kt is not None:
            ops.brownian_velocity(self.rng_keys, self.rng_counter, self.brownian_kt, self.dt, self.mob_trans,
                                  self.u_ext)
        mark("springs_brownian")
        if self.hydro is not None:
            self._hydro_velocity(force)
            mark("hydrodynamics")
        return self.u_ext

    # -- growth mode (Bacteria.cpp:905-966, :685-748) ---------------------------------------------------------------
    @staticmethod
    def _check_growth(kind, search_kind, friction, contact_cutoff, warm_start, growth_rate, division_length, radius,
                      quat, length, box, capacity, ids):
        if kind != "spherocylinder":
            raise ValueError("growth mode grows and divides spherocylinders only, not %r" % kind)
        if search_kind != ops.SEARCH_AABB:
            raise ValueError("growth mode needs search_kind=SEARCH_AABB (the corner rebuild rule bounds box gaps)")
        if friction is not None or contact_cutoff is not None:
            raise ValueError("growth mode takes no friction or contact_cutoff")
        if warm_start:
            raise ValueError("growth mode has no warm start: the constraint set changes with every birth")
        if quat is None or length is None:
            raise ValueError("spherocylinders need quat and length")
        ops._finite_nonneg(growth_rate, "growth_rate")
        if division_length is None:
            raise ValueError("growth mode needs division_length")
        D = ops._finite_nonneg(division_length, "division_length")
        rmax = float(radius.max()) if radius.shape[0] else 0.0
        if D < 2.0 * rmax:
            raise ValueError("division_length %g < 2 * max(radius) = %g: a child's length 0.5 L - r would not be "
                             "positive" % (D, 2.0 * rmax))
        ContactStepper._check_orthorhombic("growth mode", box)
        if capacity is not None and int(capacity) < 0:
            raise ValueError("capacity must be >= 0")
        if ids is not None and (ids.dtype != torch.int64 or tuple(ids.shape) != (radius.shape[0],)):
            raise ValueError("ids must be int64 of shape [n]")

    def _init_growth(self, growth_rate, division_length, capacity, ids, search_buffer):
        self.growth_rate, self.division_length = float(growth_rate), float(division_length)
        self.search_buffer = float(search_buffer)
        n = self.center.shape[0]
        dev = self.center.device
        if ids is None:
            ids = torch.arange(n, dtype=torch.int64, device=dev)
        self.ids = ids
        self.next_id = int(ids.max()) + 1 if n else 0
        self.n = n
        self._cap = 0
        self._store = {}
        self._ensure_capacity(max(int(capacity or 0), n + n // 8 + 16), fresh=True)
        self._aabb_ref = None  # the AABBs of the last build (corner rebuild rule)
        self.last_parent_of = torch.empty(0, dtype=torch.int32, device=dev)

    def _ensure_capacity(self, need, fresh=False):
        """grow-only storage: a step whose births fit allocates nothing; otherwise new buffers with headroom, the live
        rows copied over (the old ones stay alive as long as an operator still points into them)"""
        if need <= self._cap:
            return
        cap = need if fresh else need + need // 8 + 16
        n = self.n
        for name in self._body_arrays() + ["seg"]:
            old = getattr(self, name)
            buf = torch.empty((cap,) + tuple(old.shape[1:]), dtype=old.dtype, device=self.center.device)
            if name != "seg":
                buf[:n].copy_(old[:n])
            self._store[name] = buf
        self._cap = cap
        self._view()

    def _view(self):
        for name, buf in self._store.items():
            setattr(self, name, buf[:self.n])

    def _snapshot_growth(self):
        return self.n, self.next_id

    def _restore_growth(self, saved):
        """the views take the saved body count (restore then fills them); every list is in another numbering"""
        self._ensure_capacity(saved[0])
        self.n, self.next_id = saved
        self._view()
        self._aabb_ref = None
        self._forget_numbering()

    def _renumber_growth(self, perm, inv):
        self._aabb_ref = None  # the corner rebuild rule starts over

    def grow_and_divide(self):
        """divide_bacteria -> grow_bacteria (Bacteria.cpp:926-966, :905-920) on the device: returns the birth count.
        Children are rows n + k with parent last_parent_of[k] and id next_id + k; the new bounding radii follow."""
        n = self.n
        parent_of, nb = ops.select_dividing(self.length, self.division_length)
        if nb:
            self._ensure_capacity(n + nb)
        s = self._store
        ops.divide_grow_spherocylinders(n, parent_of, self.dt, self.growth_rate, s["center"], s["quat"], s["radius"],
                                        s["length"], box=self.box)
        if nb:
            for name in self._body_arrays():
                if name not in ("center", "quat", "radius", "length", "bounding_radius", "ids"):
                    ops.copy_parent_rows(parent_of, n, s[name])
            s["ids"][n:n + nb] = torch.arange(self.next_id, self.next_id + nb, dtype=torch.int64,
                                              device=self.center.device)
            self.next_id += nb
            self.n = n + nb
            self._view()
        # lengths changed: every bounding radius changes too
        ops.bounding_radius_spherocylinders(self.radius, self.length, out=self.bounding_radius)
        self.last_parent_of = parent_of
        return nb

    def _growth_links(self, births, force):
        """the reference's rebuild rule of growing bodies: births, force, or an AABB corner moved by >= buffer since
        the last build (check_update_neighbor_list, Bacteria.cpp:685-748)"""
        rebuild = (force or births > 0 or self._aabb_ref is None or not self.links.generated or
                   ops.aabb_moved(self.aabb, self._aabb_ref, self.search_buffer))
        if rebuild:
            self.links.generate(self.aabb, self.center, self.bounding_radius, force=True)
            self._aabb_ref = self.aabb  # compute_aabb returns a fresh tensor each step: this is a snapshot
        return rebuild

    # -- stages -----------------------------------------------------------------------------------------------------
    def _body_arrays(self):
        """the names of the tensors this stepper carries per body, in any mode: what snapshot / restore save, what
        reorder_bodies permutes, what growth mode stores with headroom and a child copies from its parent"""
        names = ("center", "radius", "quat", "length", "bounding_radius", "mob_trans", "mob_rot", "shape", "kinds", "ids",
                 "rng_keys", "rng_counter", "xl_sources", "xl_sites")
        if self.contact_model == "hertz":  # (the LCP ignores the materials, and does not check them)
            names += ("youngs_modulus", "poisson_ratio")
        return [k for k in names if isinstance(getattr(self, k), torch.Tensor)]

    def snapshot(self):
        """device copies of every per-body array (to restart a step from the same input) under its name, and what each
        mode saves of its own under "_<mode>" (growth mode: the body count)"""
        snap = {k: getattr(self, k).clone() for k in self._body_arrays()}
        for m in self._modes:
            snap["_" + m] = getattr(self, "_snapshot_" + m)()
        return snap

    def restore(self, snap):
        for m in self._modes:
            getattr(self, "_restore_" + m)(snap["_" + m])
        for k in self._body_arrays():
            getattr(self, k).copy_(snap[k])

    def _forget_numbering(self):
        """the neighbour list, the operator's incidence index and the multipliers are in an old numbering"""
        self.links.invalidate()
        if self.op is not None:
            self.op.close()
            self.op = None
        self.lam = None

    def reorder_bodies(self, cell_size=None, lo=None, curve="morton", hi=None, level=7):
        """Space-filling-curve permutation of all per-body arrays by centre (what the reference's zmorton /
        Hilbert helpers are advertised for): neighbours in space become neighbours in memory, so every gather of the
        contact sweeps hits nearby lines.  curve = "morton" (lattice of edge cell_size anchored at lo) or "hilbert"
        (the hilbert_3d order of a (2^level)^3 lattice over [lo, hi]; both give the same sweep times).  Every per-body
        tensor is permuted in place, the caller's center and radius and, in the Hertz model where they are tensors, its
        youngs_modulus and poisson_ratio among them.  Returns the permutation (new position k holds old body perm[k]).
        Refused with hydrodynamics in_solve: a renumbering changes the association of the solve's all-pairs sums."""
        if self.hydro_in_solve:
            raise ValueError("reorder_bodies is not supported with hydrodynamics in_solve: the all-pairs sums inside the "
                             "solve are taken in the rows' order")
        if lo is None:
            lo = self.center.min(dim=0).values.tolist() if self.box is None else [0.0, 0.0, 0.0]
        if curve == "hilbert":
            from . import distributed
            if hi is None:
                hi = self.center.max(dim=0).values.tolist() if self.box is None else list(self.box)
            table = torch.from_numpy(distributed.hilbert_key_table(level).astype("int32")).to(self.center.device)
            perm = ops.curve_order(self.center, lo, hi, level, table)
        elif curve == "morton":
            if cell_size is None:
                cell_size = 2.0 * float(self.bounding_radius.max())
            perm = ops.morton_order(self.center, lo, cell_size)
        else:
            raise ValueError("curve must be 'morton' or 'hilbert'")
        for name in self._body_arrays():
            t = getattr(self, name)
            t.copy_(ops.gather_rows(perm, t) if t.dtype == torch.float64 else t[perm.long()])
        if self._modes:  # every mode renumbers its own state through the one inverse: the new index of every old body
            inv = torch.empty_like(perm)
            inv[perm.long()] = torch.arange(perm.shape[0], dtype=perm.dtype, device=perm.device)
            for m in self._modes:
                getattr(self, "_renumber_" + m)(perm, inv)
        # the neighbour list, the operator's incidence index and the multipliers are in the old numbering: a reused list
        # would pair the wrong bodies unless the displacement test happened to fire, so force the rebuild
        self._forget_numbering()
        return perm

    def compute_aabb(self):
        if self.kind == "sphere":
            self.aabb = ops.compute_aabb_spheres(self.center, self.radius)
        elif self.kind == "mixed":
            self.aabb = ops.compute_aabb_mixed(self.kinds, self.center, self.quat, self.shape,
                                               conservative_ellipsoids=self.conservative_ellipsoid_box)[0]
        else:
            self.aabb = ops.compute_aabb_spherocylinders(self.center, self.quat, self.radius, self.length)
        return self.aabb

    def generate_neighbor_links(self, force=False):
        return self.links.generate(self.aabb, self.center, self.bounding_radius, force=force)

    def compute_contacts(self):
        pairs = self.links.pairs
        if self.kind == "sphere":
            sep, normal = ops.contact_spheres(pairs, self.center, self.radius, box=self.box)
            self.contacts = dict(sep=sep, normal=normal, ra=None, rb=None)
        elif self.kind == "mixed":  # pairs binned by shape class, one distance routine per class
            self.contacts = ops.contact_mixed(pairs, self.kinds, self.center, self.quat, self.shape, box=self.box)
        else:
            ops.spherocylinder_segments(self.center, self.quat, self.radius, self.length, out=self.seg)
            rodk = self.rod_kinematics and self.friction is None
            self.contacts = ops.contact_spherocylinders(pairs, self.seg, self.center, want_points=False,
                                                        arms="arclength" if rodk else "vector", box=self.box)
        return self.contacts

    def _compact_contacts(self):
        """contacts within the cutoff -> (pairs, contact arrays) of this step's constraints, the rest kept aside"""
        c = self.contacts
        kept = ops.select_contacts(c["sep"], self.contact_cutoff)
        keep_mask = torch.zeros(c["sep"].shape[0], dtype=torch.bool, device=kept.device)
        keep_mask[kept.long()] = True
        pairs64 = self.links.pairs.view(torch.float64).reshape(-1)       # one (i, j) row = 8 bytes
        out = {k: (ops.gather_rows(kept, v) if isinstance(v, torch.Tensor) and v.shape[0] == keep_mask.shape[0] else v)
               for k, v in c.items()}
        pairs = ops.gather_rows(kept, pairs64).view(torch.int32).reshape(-1, 2)
        return pairs, out, ~keep_mask

    def _dropped_pairs_stay_inactive(self, dropped):
        """g = sep + dt * sdot >= 0 on the pairs left out of the solve, from the body velocities it produced"""
        if not bool(dropped.any()):
            return True
        c, p = self.full_contacts, self.links.pairs[dropped].long()
        vel = self.op.body_velocity()
        n = c["normal"][dropped]
        vi, vj = vel[p[:, 0], :3].clone(), vel[p[:, 1], :3].clone()
        if self.kind != "sphere":
            if c.get("ra") is not None:
                ra, rb = c["ra"][dropped], c["rb"][dropped]
            else:  # arclength form: arm = (s - 1/2) (p1 - p0)
                u = self.seg[:, 3:6] - self.seg[:, 0:3]
                ra = (c["s"][dropped] - 0.5).unsqueeze(1) * u[p[:, 0]]
                rb = (c["t"][dropped] - 0.5).unsqueeze(1) * u[p[:, 1]]
            vi += torch.cross(vel[p[:, 0], 3:], ra, dim=1)
            vj += torch.cross(vel[p[:, 1], 3:], rb, dim=1)
        g = c["sep"][dropped] - self.dt * ((vi - vj) * n).sum(dim=1)
        return bool((g >= -self.cfg.tol).all())

    def resolve_collisions(self, rebuilt, mark=lambda name: None):
        """the contact stage of either model; mark(name) is told the Hertz stages ([history_carry,] hertz_force,
        operator, body_sweep) as they are issued"""
        if self.hydro_contact_forces:  # contact_forces() was the contact stage; U = U_ext, nothing to sweep
            self.contact_pairs = self.links.pairs
            return ops.SolveResult(num_iters=0, residual=0.0, converged=True)
        if self.contact_model == "hertz":
            self.contact_pairs = self.links.pairs
            return (self._hertz if self.hertz_friction is None else self._hertz_friction)(rebuilt, mark)
        if self.contact_cutoff is not None and self.friction is None:
            self.full_contacts = self.contacts
            pairs, self.contacts, dropped = self._compact_contacts()
            res = self._resolve(True, pairs)       # the constraint set changes from step to step: new operator
            if self._dropped_pairs_stay_inactive(dropped):
                self.contact_pairs = pairs
                return res
            self.cutoff_fallbacks += 1             # a dropped pair would have carried an impulse: the full list decides
            self.contacts = self.full_contacts
            self.contact_pairs = self.links.pairs
            return self._resolve(True, self.links.pairs)
        self.contact_pairs = self.links.pairs
        return self._resolve(rebuilt, self.links.pairs)

    def _operator(self, rebuilt, pairs, lcp=False):
        """the operator follows the constraint list: built when the list is new, its geometry refreshed (the incidence
        index kept) on a step that reuses it; the LCP path reuses only a live handle"""
        c = self.contacts
        reuse = not rebuilt and self.op is not None and self.op.num_constraints == pairs.shape[0]
        if lcp:
            reuse = reuse and bool(self.op._h)
        if self.op is not None and not reuse:
            self.op.close()
        if self.kind == "spherocylinder" and self.rod_kinematics:
            if reuse:
                self.op.refresh(c["normal"], rod=(c["s"], c["t"], self.seg))
            else:
                self.op = ops.ContactOperator(pairs, c["normal"], self.mob_trans, self.dt, mob_rot=self.mob_rot,
                                              rod=(c["s"], c["t"], self.seg), priority=c["sep"])
        elif reuse:
            self.op.refresh(c["normal"], ra=c.get("ra"), rb=c.get("rb"))
        else:
            self.op = ops.ContactOperator(pairs, c["normal"], self.mob_trans, self.dt, ra=c.get("ra"), rb=c.get("rb"),
                                          mob_rot=self.mob_rot, priority=c["sep"])

    def _resolve(self, rebuilt, pairs):
        c = self.contacts
        if self.friction is not None:  # a new operator at the surface lever arms, every step
            if self.op is not None:
                self.op.close()
            ra, rb = ops.surface_lever_arms(pairs, c["normal"], c["ra"], c["rb"], self.radius)
            self.op = ops.ContactOperator(pairs, c["normal"], self.mob_trans, self.dt, ra=ra, rb=rb,
                                          mob_rot=self.mob_rot)
            p, g, res = ops.solve_friction_contact(self.op, c["sep"], self.friction, cfg=self.cfg,
                                                   method=self.friction_method)
            self.impulse, self.lam = p, (p * c["normal"]).sum(dim=1)
            return res
        self._operator(rebuilt, pairs, lcp=True)
        if self.work_mapping is not None:
            self.op.set_work_mapping(*self.work_mapping)
        if self.tiering is not None:
            self.op.set_tiering(self.tiering)
        if self.profile_next:
            self.op.set_profiling(True)  # per-kernel HIP-event timing of the fused iteration (bench.py roofline)
        nc = pairs.shape[0]
        if rebuilt or self.lam is None or not self.warm_start or self.lam.shape[0] != nc:
            self.lam = torch.zeros(nc, dtype=torch.float64, device=self.center.device)  # NgpLcp.cpp:890-891
        q = c["sep"]
        if self.chain:  # q = sep + dt D^T U_ext (NgpHP1.cpp:1488-1531)
            q = self.op.constraint_rate(self.u_ext)
            ops.axpby(1.0, c["sep"], self.dt, q)
            self.q = q
        x, g, res = ops.solve_lcp(self.op, q, self.lam, self.cfg, mobility=self._hydro_mobility())
        self.lam, self.grad = x, g
        return res

    def _hydro_mobility(self):
        """hydrodynamics in_solve: M_h at the current positions (the rows then hold M_h D lambda); otherwise None"""
        if not self.hydro_in_solve:
            return None
        radius = self.radius if self.hydro_radius is None else self.hydro_radius
        return ops.HydroMobility(self.hydro["kind"], self.viscosity, self.center, radius, periphery=self.hydro_periphery,
                                 skip_same_index=self.hydro.get("skip_same_index", True), workspace=self._hydro_ws)

    def _contact_radius(self):
        """the radius the Hertz model takes: the sphere / rod radius, not the bounding radius"""
        return self.shape[:, 0].contiguous() if self.kind == "mixed" else self.radius

    def _hertz(self, rebuilt, mark):
        """soft contact: per-linker Hertz force, then the operator's body sweep on it -- U = M D f (no solve)"""
        c, pairs = self.contacts, self.links.pairs
        self.lam, self.max_overlap = ops.hertz_contact_force(pairs, c["sep"], self._contact_radius(),
                                                             self.youngs_modulus, self.poisson_ratio,
                                                             max_overlap=(stat(self._chain_stats, "max_overlap")
                                                                          if self.chain else None))
        mark("hertz_force")
        self._operator(rebuilt, pairs)
        mark("operator")
        self.op.body_sweep(self.lam)
        mark("body_sweep")
        return ops.SolveResult(num_iters=0, residual=0.0, converged=True)

    def contact_forces(self, rebuilt, mark=lambda name: None):
        """hydrodynamics contact_forces: the stage between compute_contacts() and external_velocity() (HP1.cpp:4737):
        Hertz force per linker, operator build / refresh, then the contact force of every body F = D f into the force
        buffer, which the force stage adds to.  The step's statistics start here; mark(name) is told hertz_force,
        operator, body_force."""
        if not self.hydro_contact_forces:
            raise ValueError("contact_forces() is the stage of hydrodynamics=dict(..., contact_forces=True)")
        self._chain_stats.zero_()
        c, pairs = self.contacts, self.links.pairs
        self.contact_pairs = pairs
        self.lam, self.max_overlap = ops.hertz_contact_force(pairs, c["sep"], self._contact_radius(),
                                                             self.youngs_modulus, self.poisson_ratio,
                                                             max_overlap=stat(self._chain_stats, "max_overlap"))
        mark("hertz_force")
        self._operator(rebuilt, pairs)
        mark("operator")
        self.op.body_force(self.lam, out=self.spring_force, stride=3)
        mark("body_force")
        return self.spring_force

    def body_contact_force(self):
        """[n, 6] (F, T): the force and the torque about its centre that the last step's contacts put on every body
        (ContactOperator.body_force[_vector]; the mobility is not applied) -- from the multipliers (LCP), the Hertz
        forces, the frictional Hertz force vectors or the cone solver's impulses -p.  Raises before a first step, and
        after reorder_bodies until the next one."""
        if self.op is None or not self.op._h or self.lam is None and self.hertz_friction is None:
            raise RuntimeError("body_contact_force needs a step: there are no contacts yet")
        if self.hertz_friction is not None:
            return self.op.body_force_vector(self.contact_force)
        if self.friction is not None:
            return self.op.body_force_vector(-self.impulse)
        return self.op.body_force(self.lam)

    def integrate(self):
        if self.hydro_contact_forces or self.contact_model == "none":  # U = U_ext: every contact force is inside it
            vel = self.velocity = self.u_ext.clone()
            ops.integrate_euler(self.dt, vel, self.center, self.quat)
            return
        vel = self.op.body_velocity()
        if self.chain:  # U = U_ext + U_contact
            ops.axpby(1.0, self.u_ext.view(-1), 1.0, vel.view(-1))
            self.velocity = vel
        if self.hertz_friction is not None:  # U = U_contact (+ U_ext); the next step's previous velocity
            if self._fr_has_ext:  # the U_ext of this step(external_force=) only: consumed here
                ops.axpby(1.0, self._fr_u_ext.view(-1), 1.0, vel.view(-1))
                self._fr_has_ext = False
            self.prev_velocity = self.velocity = vel
        ops.integrate_euler(self.dt, vel, self.center, self.quat)
        if self.box is not None:
            # wrap_rigid_inplace of a Sphere / Spherocylinder / Ellipsoid: the centre goes back into the box,
            # orientation and size are untouched (periodicity.hpp:1088-1113, :1156-1160)
            ops.wrap_rigid(self.box, self.center)

    # -- one timestep -------------------------------------------------------------------------------------------------
    def step(self, integrate=True, force_rebuild=False, timed=False, external_force=None):
        if external_force is not None:
            if not self.chain and self.hertz_friction is None:
                raise ValueError("external_force belongs to the chain step: pass springs= or brownian_kt= (0.0: no noise)")
            if tuple(external_force.shape) != (self.center.shape[0], 3):
                raise ValueError("external_force must have shape [%d, 3], got %s" % (self.center.shape[0],
                                                                                    tuple(external_force.shape)))
        st = StepStats(num_bodies=self.center.shape[0])
        ev = []

        def mark(name):
            if timed:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                ev.append((name, e))

        mark("start")
        if self.contact_model == "none":  # no sphere contact at all: the force stage, then U = U_ext
            self.external_velocity(external_force, mark)
            if integrate:
                self.integrate()
                if self.active is not None:
                    self.active.advance(self.dt)
            mark("integrate")
            st.converged = True  # (as the Hertz path reports: nothing to solve)
            self._read_chain_stats(st)
            return self._timings(st, ev, timed)
        if self.growth:
            st.num_born = self.grow_and_divide()
            st.num_bodies = self.n
            mark("grow_divide")
        self.compute_aabb()
        mark("aabb")
        if self.growth:
            st.rebuilt = self._growth_links(st.num_born, force_rebuild)
        else:
            st.rebuilt = self.generate_neighbor_links(force=force_rebuild)
        mark("broadphase")
        if self.hydro_contact_forces:  # the reference's order: contacts first, their force the first term of F
            self.compute_contacts()
            mark("narrowphase")
            self.contact_forces(st.rebuilt, mark)
            self.external_velocity(external_force, mark)
        elif self.chain:
            self.external_velocity(external_force, mark)
        elif self.hertz_friction is not None:
            self._fr_has_ext = external_force is not None
            if self._fr_has_ext:  # U_ext = (m_t F, 0)
                self._fr_u_ext = ops.drag_velocity(self.mob_trans, external_force, out=self._fr_u_ext)
        if not self.hydro_contact_forces:
            self.compute_contacts()
            mark("narrowphase")
        res = self.resolve_collisions(st.rebuilt, mark)
        if self.contact_model == "lcp":
            mark("solve")
        if integrate:
            self.integrate()
            if self.chain and self.active is not None:  # update_euchromatin_state_time (HP1.cpp:4839-4842)
                self.active.advance(self.dt)
        mark("integrate")
        st.num_contacts = self.contact_pairs.shape[0]
        st.num_iters, st.residual, st.converged = res.num_iters, res.residual, res.converged
        if self.chain:
            self._read_chain_stats(st)
        elif self.hertz_friction is not None:  # the one read of the step: (max_overlap, num_sliding)
            h = self._fr_stats.cpu()
            st.max_overlap, st.num_sliding = float(h[0]), int(h.view(torch.int64)[1])
        elif self.contact_model == "hertz":
            st.max_overlap = float(self.max_overlap.item())
        return self._timings(st, ev, timed)

    @staticmethod
    def _timings(st, ev, timed):
        if timed:
            torch.cuda.synchronize()
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                st.timings_ms[name] = a.elapsed_time(b)
        return st

    def _read_chain_stats(self, st):
        """the chain step's statistics into st: one read of the statistics array, and one of the segment contacts' own"""
        got = read_stats(self._chain_stats)  # the one read of the step
        st.max_overlap, st.max_spring_length = got["max_overlap"], got["max_spring_length"]
        st.springs_overstretched = got["springs_overstretched"]
        # (a FENE-WCA bond is clamped, never without force: its count is reported)
        if got["springs_overstretched"] and self.springs.kind != "fenewca":
            raise RuntimeError("%d FENE spring(s) stretched to L >= r_max: no force (reduce dt)"
                               % got["springs_overstretched"])
        if self.angular is not None:
            h = self._bending_stats.cpu()
            st.max_angle_deviation, st.angular_degenerate = float(h[0]), int(h.view(torch.int32)[2])
            if st.angular_degenerate:
                raise RuntimeError("%d angular spring(s) with an arm of zero length: no force" % st.angular_degenerate)
        if self.crosslinkers is not None:
            st.crosslinker_binds, st.crosslinker_unbinds = got["crosslinker_binds"], got["crosslinker_unbinds"]
            self.crosslinker_bound += st.crosslinker_binds - st.crosslinker_unbinds
            st.crosslinker_bound = self.crosslinker_bound
            st.max_crosslinker_length = got["max_crosslinker_length"]
            st.crosslinker_periphery_bound = got["crosslinker_periphery_bound"]
            if got["crosslinkers_overstretched"]:
                raise RuntimeError("%d FENE crosslinker(s) stretched to L >= r_max: no force (reduce dt)"
                                   % got["crosslinkers_overstretched"])
        if self.periphery is not None or self.active is not None:
            st.periphery_colliding, st.max_periphery_overlap = got["periphery_colliding"], got["max_periphery_overlap"]
            st.active_springs = got["active_springs"]
            st.active_switches = (got["active_switches_on"], got["active_switches_off"])
        if self.backbone is not None:
            st.max_segment_overlap, st.segment_contacts = ops.SegmentContacts.read_stats(self._backbone_stats)
            st.num_segment_pairs, st.segment_list_rebuilt = self.backbone.num_pairs, self._backbone_rebuilt


class FilamentStepper:
    """Centerline-twist elastic filaments (ops.Filaments) stepped as the reference's sperm apps step them
    (CollidingOverdampedFrictionalSperm.cpp:1999-2027).  node_ptr [F + 1], center [N, 3], radius [N], edge_orientation
    [N, 4] (w, x, y, z; by left node: synth.filaments builds the reference's initial triad), arclength [N]; twist and
    rest_curvature default to 0; wave = dict(amplitude, wave_number, frequency) with phase [F].  Host arrays or tensors.
    contacts = None, or dict(skin, youngs_modulus, poisson_ratio, mu, damping=(0, 0), density=1.0, segment_radius=None,
    history_dt=None, bonded_exclusion=1, law="frictional"): Hertzian contacts between the segments (ops.FilamentContacts),
    frictional or, with law="hertz", frictionless, whose node forces, added to the caller's external_force, enter the
    filament forces.
    dynamics = None: the overdamped step.  dynamics = dict(density, damping="critical" | (c_t, c_r), fixed_filaments=None):
    nodes with mass, stepped by the Newmark predictor / corrector of CollidingFrictionalSperm.cpp:1890-1948 and
    CollidingSperm.cpp (ops.Filaments.set_inertial); equilibrate() is then the stiffness ramp of the former.  Frictional
    contacts are accepted with dynamics: the seam (node_force as external_force) and the field the law reads (v(t), saved
    before the predictor) are those of the overdamped app; the reference has that call commented out in its inertial
    loop (CollidingFrictionalSperm.cpp:1927), so there is no reference run of that combination.
    Left out: clamp_edge1 (commented out in every loop of the reference), the two-component rest curvature of
    CollidingFrictionalSperm.cpp:1072-1082 (the wave is the library's), periodic cells, several GPUs."""

    def __init__(self, node_ptr, center, radius, edge_orientation, arclength, *, twist=None, rest_curvature=None,
                 phase=None, youngs_modulus, poisson_ratio=0.3, rest_length, viscosity, wave=None, disable_twist=False,
                 monolayer=False, contacts=None, dynamics=None):
        n = int(np.asarray(node_ptr.cpu() if isinstance(node_ptr, torch.Tensor) else node_ptr)[-1])
        if rest_curvature is None:
            rest_curvature = np.zeros((n, 3))
        if contacts is not None:  # refused before anything is built
            ops.check_dict_spec(contacts, "contacts", ("skin", "youngs_modulus", "poisson_ratio", "mu", "damping", "density",
                                                       "segment_radius", "history_dt", "bonded_exclusion", "law"),
                                optional=("damping", "density", "segment_radius", "history_dt", "bonded_exclusion", "law"))
            ops.check_filament_contacts(n, **contacts)
        if dynamics is not None:
            ops.check_dict_spec(dynamics, "dynamics", ("density", "damping", "fixed_filaments"),
                                optional=("damping", "fixed_filaments"))
            num_filaments = len(node_ptr) - 1
            ops.check_filament_inertial(num_filaments, **dynamics)
        self.filaments = ops.Filaments(node_ptr, radius, rest_curvature, arclength, phase, youngs_modulus=youngs_modulus,
                                       poisson_ratio=poisson_ratio, rest_length=rest_length, viscosity=viscosity,
                                       wave=wave, disable_twist=disable_twist, monolayer=monolayer)
        dev = lambda a: (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(  # noqa: E731
            a, dtype=np.float64))).to(device="cuda", dtype=torch.float64).contiguous()
        self.n = n
        self.youngs_modulus = float(youngs_modulus)
        self.dynamics = dynamics
        if dynamics is not None:
            self.filaments.set_inertial(**dynamics)
        self.filaments.set_state(dev(center), dev(np.zeros(n) if twist is None else twist), dev(edge_orientation))
        self.step_index = 0
        # (max_stretch, max_curvature_deviation, max_overlap, num_sliding as int64 bits, kinetic_energy): one host read
        # per step
        self._stats = torch.zeros(5, dtype=torch.float64, device="cuda")
        self.contacts = None if contacts is None else ops.FilamentContacts(self.filaments, **contacts)

    def close(self):
        if self.contacts is not None:
            self.contacts.close()
        self.filaments.close()

    def field(self, name):
        return self.filaments.field(name)

    def step(self, dt, external_force=None, read_stats=True):
        """advance -> forces at x(t + dt), time = step_index * dt as the reference counts it -> velocities.  With
        contacts: save_velocity -> advance -> update -> contact force (with external_force) -> forces -> velocities.
        With dynamics: save_velocity (frictional contacts only) -> predict -> update -> contact force -> forces ->
        correct, which also sums the kinetic energy.
        read_stats=False skips the one host read of the step (the statistics then stay at their defaults)."""
        f, c = self.filaments, self.contacts
        inertial = self.dynamics is not None
        st = StepStats(num_bodies=self.n)
        if c is not None and c.law == "frictional":
            c.save_velocity()
        if inertial:
            f.predict(dt)
        else:
            f.advance(dt)
        if c is not None:
            st.rebuilt = c.update()
            c.force(dt, external_force, self._stats[2:4])
            external_force = c.node_force_ptr()
        f.force(self.step_index * float(dt), external_force, self._stats[:2])
        if inertial:
            f.correct(dt, self._stats[4:])
        else:
            f.velocity()
        self.step_index += 1
        if read_stats:
            got = self._stats.cpu()
            st.max_stretch, st.max_curvature_deviation = float(got[0]), float(got[1])
            if inertial:
                st.kinetic_energy = float(got[4])
            if c is not None:
                st.max_overlap, st.num_sliding = float(got[2]), int(got.view(torch.int64)[3])
                st.num_pairs = st.num_contacts = c.num_pairs
        return st

    def equilibrate(self, dt, relaxed_youngs_modulus, threshold=1e-6, growth=1.1, poll_every=1, max_steps=1000000):
        """The stiffness ramp of CollidingFrictionalSperm.cpp:1781-1865 (`equilibriate`): E = relaxed_youngs_modulus;
        while E < the stepper's modulus: inertial steps without contacts until the kinetic energy is <= threshold (at
        least one step per level), then E *= growth.  step_index is not advanced, so a wave stays frozen at its current
        time (the reference does not propagate it there).  On return the modulus is the stepper's own again.
        poll_every: the one liberty taken -- the kinetic energy (8 bytes) is read once per poll_every steps, so a level
        ends at the first multiple of poll_every at which it is <= threshold; 1 is the reference's loop.  max_steps: the
        most steps of the whole ramp; one more raises RuntimeError (the reference would spin).  -> the steps per level."""
        if self.dynamics is None:
            raise RuntimeError("equilibrate needs dynamics=")
        E = float(relaxed_youngs_modulus)
        if not (math.isfinite(E) and E > 0.0):
            raise ValueError("relaxed_youngs_modulus must be finite and > 0, got %r" % (relaxed_youngs_modulus,))
        if not (math.isfinite(float(growth)) and float(growth) > 1.0):
            raise ValueError("growth must be finite and > 1, got %r" % (growth,))
        if isinstance(poll_every, bool) or not isinstance(poll_every, (int, np.integer)) or poll_every < 1:
            raise ValueError("poll_every must be an integer >= 1, got %r" % (poll_every,))
        if isinstance(max_steps, bool) or not isinstance(max_steps, (int, np.integer)) or max_steps < 1:
            raise ValueError("max_steps must be an integer >= 1, got %r" % (max_steps,))
        f = self.filaments
        time = self.step_index * float(dt)
        levels, total = [], 0
        try:
            while E < self.youngs_modulus:
                f.set_youngs_modulus(E)
                count = 0
                energy = float("inf")
                while energy > float(threshold):
                    if total + poll_every > max_steps:
                        raise RuntimeError("equilibrate: the kinetic energy is %r > %r after %d steps (max_steps) at "
                                           "E = %r" % (energy, threshold, total, E))
                    for _ in range(int(poll_every)):
                        f.predict(dt)
                        f.force(time, None, self._stats[:2])
                        f.correct(dt, self._stats[4:])
                    count += int(poll_every)
                    total += int(poll_every)
                    energy = float(self._stats[4:].cpu()[0])
                levels.append(count)
                E *= float(growth)
        finally:
            f.set_youngs_modulus(self.youngs_modulus)
        return levels
