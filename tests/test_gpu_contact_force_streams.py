"""Both entry points of include/mundy_hip_contact_force.h on a stream that is not the null stream, bit for bit against
the same call on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py, imported, not
modified): the real inputs reach the live buffers through a producer that sleeps on the side stream, so a launch or memset
that lands on another stream reads the decoy, and an entry point that blocks although the header calls it asynchronous
finds the stream still busy when it returns.  The last test parses the header and fails for a prototype with a
mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_contact_force.h")
DT = 5e-3
N = 3001   # bodies: with four lanes each, 46 full workgroups and a partial one

SYNCHRONISES = {}   # neither entry point returns a host scalar


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def stream_prototypes():
    return {n: a for n, a in header_prototypes().items() if "mhip_stream_t" in a}


def may_block(c):
    return any(f in SYNCHRONISES for f in c.fns)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def O():
    from mundy_amd import ops
    return ops


# ---- the operators: a random contact graph on N bodies, of each kinematics (fixed: the inputs under test are x, force, out) ---
def _graph():
    rng = np.random.default_rng(7)
    nc = 4 * N
    pairs = rng.integers(0, N, (nc, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]].astype(np.int32)
    nrm = rng.normal(size=(len(pairs), 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return rng, np.ascontiguousarray(pairs), nrm


def NC():
    return len(_graph()[1])


def open_op(kind):
    def open_(live):
        ops = O()
        rng, pairs, nrm = _graph()
        nc = len(pairs)
        mt, mr = dev(rng.uniform(0.5, 2.0, N)), dev(rng.uniform(0.5, 2.0, N))
        if kind == "spheres":
            return ops.ContactOperator(dev(pairs), dev(nrm), mt, DT)
        if kind == "arms":
            return ops.ContactOperator(dev(pairs), dev(nrm), mt, DT, ra=dev(rng.normal(size=(nc, 3))),
                                       rb=dev(rng.normal(size=(nc, 3))), mob_rot=mr)
        p0 = rng.normal(size=(N, 3)) * 10
        seg = np.concatenate([p0, p0 + rng.normal(size=(N, 3)), rng.uniform(0.2, 0.5, (N, 2))], axis=1)
        return ops.ContactOperator(dev(pairs), dev(nrm), mt, DT, mob_rot=mr,
                                   rod=(dev(rng.uniform(0, 1, nc)), dev(rng.uniform(0, 1, nc)), dev(seg)))
    return open_


def open_empty(live):
    z = torch.empty
    return O().ContactOperator(z((0, 2), dtype=torch.int32, device="cuda"), z((0, 3), dtype=torch.float64, device="cuda"),
                               dev(np.ones(N)), DT)


def close_op(op):
    op.close()


# ---- inputs: seed 0 the real problem, seed 1 the decoy (same shapes, a valid problem of its own) ----------------------------
def m_inputs(s):
    rng = np.random.default_rng(30 + s)
    nc = NC()
    x = rng.uniform(0.1, 2.0, nc)
    x[rng.random(nc) < 0.3] = 0.0
    force = rng.normal(size=(nc, 3))
    force[rng.random(nc) < 0.3] = 0.0
    return dict(x=dev(x), force=dev(force), out3=dev(rng.normal(size=(N, 3))), out6=dev(rng.normal(size=(N, 6))))


def m_empty(s):
    # (C = 0: the only input is the buffer that the overwriting call clears and the accumulating call leaves alone)
    rng = np.random.default_rng(40 + s)
    return dict(out6=dev(rng.normal(size=(N, 6))), keep=dev(rng.normal(size=(N, 3))))


def call_scalar(live, op):
    fresh3, fresh6 = op.body_force(live["x"], stride=3), op.body_force(live["x"], stride=6)
    op.body_force(live["x"], out=live["out3"], stride=3, accumulate=True)
    op.body_force(live["x"], out=live["out6"], stride=6, accumulate=True)
    return fresh3, fresh6, live["out3"], live["out6"]


def call_vector(live, op):
    fresh3, fresh6 = op.body_force_vector(live["force"], stride=3), op.body_force_vector(live["force"], stride=6)
    op.body_force_vector(live["force"], out=live["out3"], stride=3, accumulate=True)
    op.body_force_vector(live["force"], out=live["out6"], stride=6, accumulate=True)
    return fresh3, fresh6, live["out3"], live["out6"]


def call_empty(live, op):
    e1 = torch.empty(0, dtype=torch.float64, device="cuda")
    e3 = torch.empty((0, 3), dtype=torch.float64, device="cuda")
    # the accumulating calls leave `keep` as the producer delivered it; the overwriting ones clear a copy of out6 -- a
    # memset on another stream would be overwritten by the delayed copy
    op.body_force(e1, out=live["keep"], stride=3, accumulate=True)
    op.body_force_vector(e3, out=live["keep"], stride=3, accumulate=True)
    op.body_force(e1, out=live["out6"], stride=6)
    cleared = live["out6"].clone()
    live["out6"].copy_(live["keep"].repeat(1, 2))
    op.body_force_vector(e3, out=live["out6"], stride=6)
    return live["keep"], cleared, live["out6"], live["keep"] + live["out6"][:, :3]


CASES = []


def case(name, make, call, fns, **kw):
    CASES.append(Case(name, make, call, tuple(fns), **kw))


for kind in ("spheres", "arms", "rods"):
    case("body_force_%s" % kind, m_inputs, call_scalar, ["mhip_contact_op_body_force"], open=open_op(kind),
         close=close_op)
    case("body_force_vector_%s" % kind, m_inputs, call_vector, ["mhip_contact_op_body_force_vector"],
         open=open_op(kind), close=close_op)
case("body_force_no_contact", m_empty, call_empty, ["mhip_contact_op_body_force", "mhip_contact_op_body_force_vector"],
     open=open_empty, close=close_op)


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) == 2 and len(protos) == 2
    for name in SYNCHRONISES:
        assert name in streamed
    for c in CASES:
        for fn in c.fns:
            assert fn in protos, "%s: %s is not declared in the header" % (c.name, fn)
    assert len({c.name for c in CASES}) == len(CASES)


# ---- the parametrised test ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    su.recording_library(mp)
    side = torch.cuda.Stream()
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
def test_every_stream_entry_point_of_the_header_was_called(rig):
    assert len(rig["ran"]) == len(CASES), "only %d of %d cases ran in this session: the count needs the whole module" % (
        len(rig["ran"]), len(CASES))
    missing = sorted(n for n in stream_prototypes() if n not in su.CALLED)
    assert not missing, "stream-taking entry points no case called: %s" % missing
    listed = sorted(f for c in CASES for f in c.fns if f not in su.CALLED)
    assert not listed, "entry points a case lists but did not call: %s" % listed
