"""Every stream-taking entry point of include/mundy_hip_hydro_periphery.h on a stream that is not the null stream, bit for
bit against the same call on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py,
imported, not modified): the real inputs reach the live buffers through a producer that sleeps on the side stream, so a
launch, memset or copy that lands on another stream reads the decoy, and an entry point that blocks although the header
calls it asynchronous finds the stream still busy when it returns.  The last test parses the header and fails for a
prototype with a mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import hydro_periphery_model as pm
import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_hydro_periphery.h")
MU = 0.7

SYNCHRONISES = {"mhip_hydro_periphery_invert": "returns a host scalar"}


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def stream_prototypes():
    return {n: a for n, a in header_prototypes().items() if "mhip_stream_t" in a}


def may_block(c):
    return any(f in SYNCHRONISES for f in c.fns)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def D(**kw):
    return {k: dev(v) for k, v in kw.items()}


def O():
    from mundy_amd import ops
    return ops


# ---- inputs: seed 0 the real problem, seed 1 the decoy (same shapes, a valid problem of its own) -----------------------------
ORDER = 7  # 128 nodes, N = 384
NB = 3001  # beads: eleven full workgroups and a partial one


def m_surface(s):
    p, w, n = pm.sphere_quadrature(ORDER, 5.0 if s == 0 else 4.0, invert=True)
    if s:  # the decoy: the same sphere turned and squeezed
        p, n = p[:, [1, 2, 0]] * np.array([1.0, 0.9, 1.1]), n[:, [1, 2, 0]]
    return D(p=p, w=w, n=n)


def m_matrix(s):
    A = np.random.default_rng(40 + s).normal(size=(258, 258))
    np.fill_diagonal(A, 0.0)
    return D(A=A)


def m_matvec(s):
    rng = np.random.default_rng(50 + s)
    return D(Minv=rng.normal(size=(384, 384)), u=rng.normal(size=384))


def _beads(rng, n):
    v = rng.normal(size=(n, 3))
    x = v / np.linalg.norm(v, axis=1, keepdims=True) * (4.0 * rng.uniform(0, 1, n) ** (1 / 3))[:, None]
    return x, rng.uniform(0.05, 0.3, n), rng.normal(size=(n, 3))


def m_double_layer(s):
    rng = np.random.default_rng(60 + s)
    ns = 2 * 1024 + 77
    v = rng.normal(size=(ns, 3))
    n = -v / np.linalg.norm(v, axis=1, keepdims=True)
    x, _, _ = _beads(rng, 300)
    return D(c=-5.0 * n, n=n, w=rng.uniform(0.01, 0.05, ns), f=rng.normal(size=(ns, 3)), t=x, out=rng.normal(size=(300, 6)))


def m_correct(s):
    rng = np.random.default_rng(70 + s)
    x, a, F = _beads(rng, NB)
    return D(Minv=rng.normal(size=(384, 384)) / 20.0, x=x, a=a, F=F, vel=rng.normal(size=(NB, 6)))


# ---- calls --------------------------------------------------------------------------------------------------------------------
def open_list(live):
    return dict(handles=[])


def close_list(ctx):
    for h in ctx["handles"]:
        h.close()
    if ctx.get("ws") is not None:
        ctx["ws"].close()


def call_create(fill):
    def call(live, ctx):
        # (the handle is kept until close: releasing its buffers would wait for the stream)
        h = O().HydroPeriphery(live["p"], live["w"], live["n"], MU)
        ctx["handles"].append(h)
        getattr(h, fill)()
        return h.matrix()
    return call


def open_handle(n_nodes, surface=False, path=None):
    def open_(live):
        ops = O()
        if surface:
            s = m_surface(0)
            h = ops.HydroPeriphery(s["p"], s["w"], s["n"], MU)
        else:
            z = torch.zeros((n_nodes, 3), dtype=torch.float64, device="cuda")
            h = ops.HydroPeriphery(z, z[:, 0].contiguous(), z, MU)
        ws = ops.HydroWorkspace()
        if path is not None:
            ws.set_path(path)
        return dict(handles=[h], ws=ws)
    return open_


def call_set_matrix(live, ctx):
    return ctx["handles"][0].set_matrix(live["A"]).matrix()


def call_invert(live, ctx):
    h = ctx["handles"][0]
    min_pivot = h.set_matrix(live["A"]).invert()
    return dict(inverse=h.matrix(), min_pivot=min_pivot)


def call_surface_forces(live, ctx):
    h = ctx["handles"][0]
    return dict(f=h.set_inverse(live["Minv"]).surface_forces(live["u"]), inverse=h.matrix())


def call_double_layer(accumulate, skip):
    def call(live, ctx):
        if accumulate:
            return O().hydro_double_layer(MU, live["c"], live["n"], live["w"], live["f"], live["t"], out=live["out"],
                                          accumulate=True, skip_same_index=skip, workspace=ctx["ws"])
        return O().hydro_double_layer(MU, live["c"], live["n"], live["w"], live["f"], live["t"], skip_same_index=skip,
                                      workspace=ctx["ws"])
    return call


def call_correct(kind):
    def call(live, ctx):
        h = ctx["handles"][0]
        h.set_inverse(live["Minv"])
        return h.correct(kind, live["x"], live["a"], live["F"], live["vel"], workspace=ctx["ws"])
    return call


CASES = []


def case(name, make, call, fns, **kw):
    CASES.append(Case(name, make, call, tuple(fns), **kw))


case("create_fill_matrix", m_surface, call_create("fill_matrix"),
     ["mhip_hydro_periphery_create", "mhip_hydro_periphery_fill_matrix"], open=open_list, close=close_list)
case("create_fill_double_layer", m_surface, call_create("fill_double_layer"),
     ["mhip_hydro_periphery_create", "mhip_hydro_periphery_fill_double_layer"], open=open_list, close=close_list)
case("set_matrix", m_matrix, call_set_matrix, ["mhip_hydro_periphery_set_matrix"], open=open_handle(86),
     close=close_list)
case("set_matrix_invert", m_matrix, call_invert, ["mhip_hydro_periphery_set_matrix", "mhip_hydro_periphery_invert"],
     open=open_handle(86), close=close_list)
case("set_inverse_surface_forces", m_matvec, call_surface_forces,
     ["mhip_hydro_periphery_set_inverse", "mhip_hydro_periphery_surface_forces"], open=open_handle(128),
     close=close_list)
for path in ("in_lane", "partial"):
    case("double_layer_%s" % path, m_double_layer, call_double_layer(False, True), ["mhip_hydro_double_layer"],
         open=open_handle(1, path=path), close=close_list)
    case("double_layer_accumulate_%s" % path, m_double_layer, call_double_layer(True, False),
         ["mhip_hydro_double_layer"], open=open_handle(1, path=path), close=close_list)
for kind in ("rpyc", "stokes"):
    case("correct_%s" % kind, m_correct, call_correct(kind),
         ["mhip_hydro_periphery_set_inverse", "mhip_hydro_periphery_correct"], open=open_handle(128, surface=True),
         close=close_list)


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) == 9 and len(protos) == 11
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
