"""The centerline-twist filaments on the device (filament.hip) against the numpy model (filament_model.py, with the
oracle's sine and cosine: the device's IEEE sequence), bit for bit: the edge state, curvature, forces, twist torques,
velocities and both statistics, across tile borders and the grid-stride loop's second pass; the stepper against the
model over 50 steps, the relaxation to the arc of the rest curvature, and the C++ driver."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch

import filament_model as fm
from gpu_util import PAST_FULL_GRID, STAT_POSITIONS, all_pos_zero, assert_bits_equal, dev, host

pytestmark = pytest.mark.gpu

# filament ends on (256), one before (511) and one after (513) a border of the 256-node tiles; then short ones, and two
# that span whole tiles
BORDER_COUNTS = (256, 255, 2, 3, 4, 257, 513)
WAVE = dict(amplitude=0.2, wave_number=0.7, frequency=1.3)
COMPARED = ("edge_tangent", "edge_length", "edge_binormal", "edge_orientation", "curvature", "force", "twist_torque",
            "velocity", "twist_velocity")
STATE = ("center", "twist") + COMPARED + ("edge_tangent_old", "edge_length_old", "edge_binormal_old",
                                         "edge_orientation_old")


def make_case(seed, counts):
    """filaments bent out of plane and stretched, with twist, non-uniform radii and rest curvatures, a phase each"""
    from mundy_amd import synth
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    n, F = int(ptr[-1]), len(counts)
    last = np.zeros(n, bool)
    last[ptr[1:] - 1] = True
    first = np.zeros(n, bool)
    first[ptr[:-1]] = True
    fid = np.repeat(np.arange(F), counts)
    # tangents: a random walk on the sphere, restarted (by subtracting the walk's value at the filament's first edge)
    walk = np.cumsum(rng.normal(scale=0.15, size=(n, 3)), axis=0)
    t = np.array([0.1, 0.2, 1.0]) + walk - walk[ptr[:-1]][fid]
    t /= np.sqrt((t * t).sum(axis=1))[:, None]
    step = t * rng.uniform(0.85, 1.2, (n, 1))
    step[last] = 0.0
    c = np.cumsum(np.concatenate([np.zeros((1, 3)), step[:-1]]), axis=0)
    c = c - c[ptr[:-1]][fid] + rng.uniform(-3.0, 3.0, (F, 3))[fid]
    d1 = np.tile([1.0, 0.0, 0.0], (n, 1))
    d2 = np.cross(t, d1)
    d2 /= np.sqrt((d2 * d2).sum(axis=1))[:, None]
    quat = synth.triad_quaternion(d1, d2, t)
    quat[last] = (1.0, 0.0, 0.0, 0.0)
    s = np.arange(n) - ptr[:-1][fid]
    return dict(node_ptr=ptr, center=np.ascontiguousarray(c), twist=rng.uniform(-0.3, 0.3, n),
                radius=rng.uniform(0.5, 1.0, n), rest_curvature=rng.uniform(-0.1, 0.1, (n, 3)),
                arclength=s.astype(np.float64), edge_orientation=quat, phase=rng.uniform(0.0, 2.0 * math.pi, F), n=n)


def params(wave=False, disable_twist=False, monolayer=False):
    return fm.Params(E=10.0, nu=0.3, l0=1.0, eta=1.0, A=WAVE["amplitude"] if wave else 0.0,
                     k=WAVE["wave_number"] if wave else 0.0, omega=WAVE["frequency"] if wave else 0.0, wave=wave,
                     disable_twist=disable_twist, monolayer=monolayer)


def new_model(case, prm):
    f = fm.Filaments(case["node_ptr"], case["radius"], case["rest_curvature"], case["arclength"], case["phase"], prm)
    return f.set_state(case["center"], case["twist"], case["edge_orientation"])


def device_kwargs(prm):
    return dict(youngs_modulus=prm.E, poisson_ratio=prm.nu, rest_length=prm.l0, viscosity=prm.eta,
                wave=WAVE if prm.wave else None, disable_twist=prm.disable_twist, monolayer=prm.monolayer)


def new_device(case, prm):
    from mundy_amd import ops
    f = ops.Filaments(case["node_ptr"], case["radius"], case["rest_curvature"], case["arclength"], case["phase"],
                      **device_kwargs(prm))
    f.set_state(dev(case["center"]), dev(case["twist"]), dev(case["edge_orientation"]))
    return f


def assert_same(d, m, names, what):
    for name in names:
        assert_bits_equal(host(d.field(name)), getattr(m, name), "%s: %s" % (what, name))


def two_evaluations(case, prm, external=None, dt=0.02):
    """set_state -> force, velocity (t_old = t: no binormal yet) -> advance -> force, velocity (the nodes have moved and
    twisted: binormal, parallel transport and the twist rotation all act), device against model after each"""
    d, m = new_device(case, prm), new_model(case, prm)
    assert_same(d, m, STATE, "initial state")
    ext = None if external is None else dev(external)
    for k, time in enumerate((0.25, 0.5)):
        if k:
            d.advance(dt)
            m.advance(dt)
            assert_same(d, m, STATE, "after advance")
        stats = d.force(time, ext).tolist()
        want = m.compute_force(time, external)
        d.velocity()
        m.compute_velocity()
        assert_same(d, m, COMPARED, "evaluation %d" % k)
        assert_bits_equal(np.array(stats), np.array(want), "evaluation %d: statistics" % k)
        assert want[0] > 0.0 and want[1] > 0.0
    assert np.abs(m.edge_binormal).max() > 1e-4 and np.abs(m.twist_torque).max() > 1e-4
    d.close()
    return m


# ---- 1. every field, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wave", [False, True])
def test_fields_across_tile_borders_match_the_model(oracle, wave):
    assert np.cumsum(BORDER_COUNTS)[:3].tolist() == [256, 511, 513]
    two_evaluations(make_case(21, BORDER_COUNTS), params(wave=wave))


def test_one_filament_of_three_nodes(oracle):
    two_evaluations(make_case(22, (3,)), params(wave=True))


def test_second_pass_of_the_grid_stride_loop(oracle):
    counts = [301] * (PAST_FULL_GRID // 301) + [PAST_FULL_GRID % 301]
    case = make_case(23, counts)
    assert case["n"] == PAST_FULL_GRID and counts[-1] >= 3
    two_evaluations(case, params(wave=True))


def test_external_force_is_added_first_and_null_is_zero(oracle):
    case = make_case(24, BORDER_COUNTS)
    ext = np.random.default_rng(5).normal(size=(case["n"], 3))
    with_ext = two_evaluations(case, params(), external=ext)
    without = two_evaluations(case, params())
    assert not np.array_equal(with_ext.force, without.force)
    # NULL and an array of +0.0: the same bits
    a, b = new_device(case, params()), new_device(case, params())
    a.force(0.0)
    b.force(0.0, torch.zeros((case["n"], 3), dtype=torch.float64, device="cuda"))
    for name in ("force", "twist_torque"):
        assert_bits_equal(host(a.field(name)), host(b.field(name)), name)
    a.close()
    b.close()


# ---- 2. the statistics, wherever the largest value sits ------------------------------------------------------------------
def test_statistics_at_every_position():
    from mundy_amd import ops, synth
    # straight filaments at rest along z, all in one row of nodes: nothing stretched, nothing bent
    counts = [301] * (PAST_FULL_GRID // 301) + [PAST_FULL_GRID % 301]
    n = PAST_FULL_GRID
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    fid = np.repeat(np.arange(len(counts)), counts)
    s = (np.arange(n) - ptr[:-1][fid]).astype(np.float64)
    center = np.stack([np.zeros(n), 4.0 * fid, s], axis=1)
    quat = np.tile([1.0, 0.0, 0.0, 0.0], (n, 1))
    for pos in STAT_POSITIONS:
        edge, node = min(pos, n - 2), min(max(pos, 1), n - 2)   # the nearest edge and interior node
        assert edge + 1 < ptr[fid[edge] + 1] and ptr[fid[node]] < node < ptr[fid[node] + 1] - 1
        c = center.copy()
        c[edge + 1:ptr[fid[edge] + 1], 2] += 0.5      # edge `edge` is 1.5 long
        rest = np.zeros((n, 3))
        rest[node, 1] = 0.25                          # element `node` is 0.25 away from its rest curvature
        f = ops.Filaments(ptr, np.ones(n), rest, s, youngs_modulus=8.0, poisson_ratio=0.25, rest_length=1.0,
                          viscosity=1.0)
        f.set_state(dev(c), dev(np.zeros(n)), dev(quat))
        assert f.force(0.0).tolist() == [0.5, 0.25], pos
        f.close()
    # and nothing at all
    f = ops.Filaments(ptr, np.ones(n), np.zeros((n, 3)), s, youngs_modulus=8.0, poisson_ratio=0.25, rest_length=1.0,
                      viscosity=1.0)
    f.set_state(dev(center), dev(np.zeros(n)), dev(quat))
    stats = f.force(0.0)
    assert all_pos_zero(host(stats)) and all_pos_zero(host(f.field("force"))) and all_pos_zero(host(f.field("twist_torque")))
    f.close()
    assert synth.filaments(2, 3)["node_ptr"].tolist() == [0, 3, 6]


# ---- 3. the stepper ---------------------------------------------------------------------------------------------------------
def new_stepper(case, prm):
    from mundy_amd import pipeline
    return pipeline.FilamentStepper(case["node_ptr"], case["center"], case["radius"], case["edge_orientation"],
                                    case["arclength"], twist=case["twist"], rest_curvature=case["rest_curvature"],
                                    phase=case["phase"], **device_kwargs(prm))


@pytest.mark.parametrize("constrained", [False, True])
def test_fifty_steps_match_the_model(oracle, constrained):
    case = make_case(25, BORDER_COUNTS)
    prm = params(wave=True, disable_twist=constrained, monolayer=constrained)
    st, m = new_stepper(case, prm), new_model(case, prm)
    dt = 0.01
    for k in range(50):
        got = st.step(dt)
        want = m.step(dt, k * dt)
        assert_bits_equal(np.array([got.max_stretch, got.max_curvature_deviation]), np.array(want), "step %d" % k)
    assert_same(st, m, STATE, "after 50 steps")
    assert np.isfinite(m.center).all() and np.abs(m.center - case["center"]).max() > 1e-3
    if constrained:
        assert all_pos_zero(m.center[:, 0]) and all_pos_zero(m.twist)
    st.close()


def test_relaxation_to_an_arc_on_the_device():
    from mundy_amd import pipeline, synth
    # the case of test_filament_host.py::test_relaxation_to_an_arc, under the same bound
    n = 6
    center = np.zeros((n, 3))
    center[:, 2] = np.arange(n)
    quat = np.tile(fm.triad_orientation([0.0, 0.0, 1.0]), (n, 1))
    st = pipeline.FilamentStepper([0, n], center, np.ones(n), quat, np.arange(n) * 1.0,
                                  rest_curvature=np.tile([0.3, 0.0, 0.0], (n, 1)), youngs_modulus=10.0, poisson_ratio=0.3,
                                  rest_length=1.0, viscosity=1.0, disable_twist=True, monolayer=True)
    for _ in range(4000):
        st.step(0.1, read_stats=False)
    c = host(st.field("center"))
    d = np.diff(c, axis=0)
    cr = np.cross(d[:-1], d[1:])
    angle = np.arctan2(np.sqrt((cr * cr).sum(axis=1)), (d[:-1] * d[1:]).sum(axis=1))
    length = np.sqrt((d * d).sum(axis=1))
    print("angle error", np.abs(angle - 2.0 * math.asin(0.15)).max(), "length error", np.abs(length - 1.0).max())
    assert np.abs(angle - 2.0 * math.asin(0.15)).max() < 1e-12
    assert np.abs(length - 1.0).max() < 1e-12
    st.close()
    assert synth.filaments(1, n)["center"][:, 2].tolist() == [5.0, 4.0, 3.0, 2.0, 1.0, 0.0]   # filament 0 is flipped


# ---- 4. the C++ driver ------------------------------------------------------------------------------------------------------
def test_filament_step_app_matches_python():
    from cpp_apps import build_app, checksums, fnv1a as fnv
    case = make_case(26, BORDER_COUNTS)
    prm = params(wave=True)
    st = new_stepper(case, prm)
    dt, steps = 0.01, 20
    lines = [st.step(dt) for _ in range(steps)]
    import tempfile
    exe = build_app("filament_step_app")
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "in.bin")
        with open(path, "wb") as f:
            np.array([len(case["node_ptr"]) - 1, case["n"]], dtype=np.uint64).tofile(f)
            case["node_ptr"].astype(np.int32).tofile(f)
            for name in ("center", "twist", "edge_orientation", "radius", "rest_curvature", "arclength", "phase"):
                case[name].astype(np.float64).tofile(f)
        args = [dt, prm.E, prm.nu, prm.l0, prm.eta, prm.A, prm.k, prm.omega]
        out = subprocess.run([exe, path, str(steps)] + [repr(float(a)) for a in args] + ["1", "0", "0"],
                             capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    got = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("STEP")]
    assert len(got) == steps
    for k, (words, s) in enumerate(zip(got, lines)):
        assert_bits_equal(np.array([float.fromhex(words[3]), float.fromhex(words[5])]),
                          np.array([s.max_stretch, s.max_curvature_deviation]), "step %d" % k)

    sums = checksums(out.stdout)
    for name in ("center", "twist", "velocity", "twist_velocity", "edge_orientation"):
        words = np.ascontiguousarray(host(st.field(name))).reshape(-1).view(np.uint64)
        assert sums[name] == fnv(words), name
    st.close()
