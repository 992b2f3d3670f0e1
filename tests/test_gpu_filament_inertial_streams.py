"""Every entry point of include/mundy_hip_filament_inertial.h on a stream that is not the null stream, bit for bit
against the same calls on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py,
imported, not modified).  None of these entry points takes a stream: each runs on the stream of its handle, which is the
stream current when the handle was created, so a case is a whole life -- create, make inertial, plant the state, step --
as the filament cases of tests/test_gpu_streams.py are.  The real inputs reach the live buffers through a producer that
sleeps on the side stream, so a launch, memset or copy that lands on another stream reads the decoy.  The last test
parses the header and fails for a prototype that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_filament_inertial.h")

# creation waits for its uploads (the host arrays may go when it returns), and so does set_inertial with a mask
SYNCHRONISES = {"mhip_filaments_create": "synchronises the stream before it returns",
                "mhip_filament_contacts_create": "synchronises the stream before it returns",
                "mhip_filaments_set_inertial": "uploads the per-node flag of the fixed filaments and waits for it"}
OUT = ("center", "twist", "velocity", "twist_velocity", "acceleration", "twist_acceleration", "force", "twist_torque",
       "edge_orientation", "edge_tangent_old")


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_cache = {}


def _case(s):
    if ("border", s) not in _cache:
        from test_gpu_filaments import BORDER_COUNTS, make_case
        _cache[("border", s)] = make_case(60 + s, BORDER_COUNTS)
    return _cache[("border", s)]


def _crossed(s):
    if ("crossed", s) not in _cache:
        from mundy_amd import synth
        _cache[("crossed", s)] = synth.crossed_filaments(6, 5, angle=1.0 + 0.07 * s, overlap=0.125 + 0.02 * s, seed=7)
    return _cache[("crossed", s)]


def m_inertial(s):
    c = _case(s)
    rng = np.random.default_rng(70 + s)
    n = c["n"]
    return dict(center=dev(c["center"]), twist=dev(c["twist"]), edge_orientation=dev(c["edge_orientation"]),
                velocity=dev(0.1 * rng.normal(size=(n, 3))), twist_velocity=dev(0.1 * rng.normal(size=n)),
                acceleration=dev(0.1 * rng.normal(size=(n, 3))), twist_acceleration=dev(0.1 * rng.normal(size=n)),
                ext=dev(0.1 * rng.normal(size=(n, 3))))


def call_inertial(damping, fixed):
    def call(live, ctx):
        from mundy_amd import ops
        from test_gpu_filaments import device_kwargs, params
        c = _case(0)
        f = ops.Filaments(c["node_ptr"], c["radius"], c["rest_curvature"], c["arclength"], c["phase"],
                          **device_kwargs(params(wave=True)))
        try:
            mask = None
            if fixed:
                mask = np.zeros(len(c["node_ptr"]) - 1, bool)
                mask[3] = True
            f.set_inertial(1.5, damping, mask)
            f.set_state(live["center"], live["twist"], live["edge_orientation"])
            f.set_motion(live["velocity"], live["twist_velocity"], live["acceleration"], live["twist_acceleration"])
            before = f.kinetic_energy().clone()
            ke = torch.zeros(2, dtype=torch.float64, device="cuda")
            f.predict(0.01)
            f.force(0.0, live["ext"])
            f.correct(0.01, ke[:1])
            f.set_youngs_modulus(7.0)
            f.predict(0.01)
            f.force(0.01, live["ext"])
            f.correct(0.01)          # without the sum
            f.kinetic_energy(ke[1:])
            return before, ke, {k: f.field(k) for k in OUT}
        finally:
            f.close()
    return call


def m_contacts(s):
    c = _crossed(s)
    return dict(center=dev(c["center"]), twist=dev(c["twist"]), edge_orientation=dev(c["edge_orientation"]))


def call_contacts(live, ctx):
    from mundy_amd import ops
    from test_gpu_filaments import device_kwargs, params
    c = _crossed(0)
    f = ops.Filaments(c["node_ptr"], c["radius"], c["rest_curvature"], c["arclength"], c["phase"],
                      **device_kwargs(params()))
    fc = None
    try:
        f.set_state(live["center"], live["twist"], live["edge_orientation"])
        fc = ops.FilamentContacts(f, skin=0.5, mu=0.5, youngs_modulus=200.0, poisson_ratio=0.3, law="hertz")
        rebuilt = fc.update()
        out = {"rebuilt": rebuilt, "num_pairs": fc.num_pairs, "stats": fc.force(1e-3).clone()}
        out.update({k: fc.field(k) for k in ("pairs", "sep", "tang_disp", "force", "share", "node_force")})
        return out
    finally:
        if fc is not None:
            fc.close()
        f.close()


LIFE = ("mhip_filaments_create", "mhip_filaments_set_inertial", "mhip_filaments_set_motion", "mhip_filaments_predict",
        "mhip_filaments_correct", "mhip_filaments_kinetic_energy", "mhip_filaments_set_youngs_modulus",
        "mhip_filaments_get_inertial")
CASES = [Case("inertial_critical_fixed", m_inertial, call_inertial("critical", True), LIFE),
         Case("inertial_constant", m_inertial, call_inertial((0.3, 0.2), False), LIFE),
         Case("contacts_frictionless", m_contacts, call_contacts,
              ("mhip_filaments_create", "mhip_filament_contacts_create", "mhip_filament_contacts_set_law"))]


def may_block(c):
    return any(f in SYNCHRONISES for f in c.fns)


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos = header_prototypes()
    assert len(protos) == 8 and not any("mhip_stream_t" in a for a in protos.values())
    assert len({c.name for c in CASES}) == len(CASES)
    assert set(protos) <= {f for c in CASES for f in c.fns}


# ---- the parametrised test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    su.recording_library(mp)
    # a stream of the high-priority pool: the runtime shares a few hardware queues among the streams of one priority, so
    # a further normal-priority stream here would move every stream a later module creates onto another queue, and the
    # canary of tests/test_gpu_streams.py, which runs after this module, depends on which queue its side stream shares
    # (see the note in tests/test_gpu_streams_body_clean_waves.py).  The high-priority pool has queues of its own, which
    # the null stream never shares; for the ordering these tests check, the priority is immaterial.
    side = torch.cuda.Stream(priority=-1)
    cycles_per_ms = su.calibrate(side)
    try:
        yield dict(side=side, cycles_per_ms=cycles_per_ms, ran=set())
    finally:
        mp.undo()


@gpu
def test_canary_a_side_stream_does_not_wait_for_the_null_stream(rig):
    # the instrument itself (as in tests/test_gpu_streams.py): if the null stream's clone holds the real data, side
    # streams block against the null stream on this runtime and every other test of this file is blind
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


# ---- coverage: measured, not declared ---------------------------------------------------------------------------------------------
@gpu
def test_every_entry_point_of_the_header_was_called(rig):
    assert len(rig["ran"]) == len(CASES), "only %d of %d cases ran in this session: the count needs the whole module" % (
        len(rig["ran"]), len(CASES))
    missing = sorted(n for n in header_prototypes() if n not in su.CALLED)
    assert not missing, "entry points of the header no case called: %s" % missing
    listed = sorted(f for c in CASES for f in c.fns if f not in su.CALLED)
    assert not listed, "entry points a case lists but did not call: %s" % listed
