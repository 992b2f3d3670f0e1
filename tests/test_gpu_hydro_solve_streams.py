"""Both stream-taking entry points of include/mundy_hip_hydro_solve.h on a stream that is not the null stream, bit for bit
against the same call on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py,
imported, not modified): the real inputs reach the live buffers through a producer that sleeps on the side stream, so a
launch, memset or copy that lands on another stream reads the decoy, and an entry point that blocks although the header
calls it asynchronous finds the stream still busy when it returns.  The solve polls its stream and so belongs to
SYNCHRONISES.  The last test parses the header and fails for a prototype with a mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import hydro_periphery_model as pm
import hydro_solve_model as hsm
import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_hydro_solve.h")

SYNCHRONISES = {"mhip_bbpgd_solve_contact_hydro": "returns the iteration count and the residual: polls its stream"}


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


def CASE():
    return hsm.case_of("centred")   # 300 beads inside the periphery's sphere, 756 contacts


# ---- the handles: the case's sphere operator, a workspace, and (the confined cases) a periphery with its inverse -----------
def open_handles(confined):
    def open_(live):
        ops, c = O(), CASE()
        op = ops.ContactOperator(dev(c["pairs"]), dev(c["normal"]), dev(c["mob_trans"]), c["dt"])
        P = None
        if confined:
            pts, w, nrm = pm.sphere_quadrature(4, 12.0, include_poles=False, invert=True)
            P = ops.HydroPeriphery(dev(pts), dev(w), dev(nrm), c["viscosity"])
            P.fill_matrix()
            P.invert()
        return dict(op=op, ws=ops.HydroWorkspace(), periphery=P)
    return open_


def close_handles(ctx):
    ctx["op"].close()
    ctx["ws"].close()
    if ctx["periphery"] is not None:
        ctx["periphery"].close()


def mobility(live, ctx, kind):
    # (built per call: the struct points at the live centres and radii, which the delayed producer delivers)
    return O().HydroMobility(kind, CASE()["viscosity"], live["center"], live["radius"], periphery=ctx["periphery"],
                             workspace=ctx["ws"])


# ---- inputs: seed 0 the real problem, seed 1 the decoy (same shapes, a valid problem of its own) ----------------------------
def m_inputs(s):
    c = CASE()
    rng = np.random.default_rng(50 + s)
    nc = len(c["q"])
    x = rng.uniform(0.1, 2.0, nc)
    x[rng.random(nc) < 0.4] = 0.0
    return dict(x=dev(x), q=dev(c["q"] + 0.02 * s * rng.uniform(0.0, 1.0, nc)), x0=dev(0.1 * s * rng.uniform(0.0, 1.0, nc)),
                center=dev(c["center"] + 1e-3 * s * rng.normal(size=c["center"].shape)),
                radius=dev(c["hydro_radius"] * (1.0 + 0.05 * s)))   # (larger: m_t + RPYC stays positive semi-definite)


def call_apply(kind):
    def call(live, ctx):
        y = ctx["op"].apply_hydro(mobility(live, ctx, kind), live["x"])
        return y, ctx["op"].body_velocity()
    return call


def call_solve(live, ctx):
    ops = O()
    x = live["x0"].clone()
    state = (x, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x))
    _, _, res = ops.solve_lcp(ctx["op"], live["q"], x, ops.PGDConfig(max_iters=1000, tol=1e-8), state=state,
                              mobility=mobility(live, ctx, "rpyc"))
    assert res.converged
    return state, res, ctx["op"].body_velocity()


CASES = []


def case(name, make, call, fns, **kw):
    CASES.append(Case(name, make, call, tuple(fns), **kw))


for confined in (False, True):
    tag = "confined" if confined else "free"
    for kind in ("rpyc", "rpy"):
        case("apply_hydro_%s_%s" % (kind, tag), m_inputs, call_apply(kind), ["mhip_contact_op_apply_hydro"],
             open=open_handles(confined), close=close_handles)
    case("solve_contact_hydro_%s" % tag, m_inputs, call_solve, ["mhip_bbpgd_solve_contact_hydro"],
         open=open_handles(confined), close=close_handles)


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) == 2 and len(protos) == 3
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
