"""Every entry point of include/mundy_hip_bending.h on a stream that is not the null stream, whole lives (create, force,
renumber, force, destroy on the side stream), bit for bit against the same calls on the null stream, with the
instrument of tests/test_gpu_streams.py (tests/stream_util.py, imported, not modified): the real inputs reach the live
buffers through a producer that sleeps on the side stream, so a launch, copy or memset that lands on another stream
reads the decoy, and an entry point that blocks although the header calls it asynchronous finds the stream still busy
when it returns.  The last test parses the header and fails for a prototype with a mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_bending.h")
N = 3001   # no multiple of a wave or a workgroup

# create uploads the caller's host arrays and waits for the stream before it returns (the header says so)
SYNCHRONISES = {"mhip_angular_springs_create": "frees the caller's host arrays on return: waits for its uploads"}


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def stream_prototypes():
    return {n: a for n, a in header_prototypes().items() if "mhip_stream_t" in a}


def may_block(c):
    return any(f in SYNCHRONISES for f in c.fns)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _triplets():
    from mundy_amd import synth
    t = synth.chain_triplets(np.arange(0, N + 1, 50).tolist() + [N])   # chains of 50 beads and one of 1
    extra = np.array([[0, 100, 7], [9, 1500, 7], [2999, 3, 7]], np.int32)   # body 7 is the centre of four
    return np.concatenate([t, extra])


def m_inputs(s):
    rng = np.random.default_rng(90 + s)
    steps = rng.normal(size=(N, 3))
    steps *= (rng.uniform(0.7, 1.2, N) / np.linalg.norm(steps, axis=1))[:, None]
    return dict(center=dev(np.cumsum(steps, axis=0)), old=dev(rng.normal(size=(N, 3))),
                new_of_old=dev(rng.permutation(N).astype(np.int32)))


def _open(live):
    from mundy_amd import ops
    t = _triplets()
    rng = np.random.default_rng(5)
    return ops.AngularSprings(N, t, rng.uniform(1.0, 9.0, len(t)), rng.uniform(0.0, np.pi, len(t)))


def call_force(live, h):
    """both forms of the force on an open handle, the statistics with them"""
    f, deg, mx = h.force(live["center"])
    acc = live["old"].clone()
    _, deg2, mx2 = h.force(live["center"], out=acc, accumulate=True)
    return [f, deg, mx, acc, deg2, mx2]


def call_renumber(live, h):
    """renumber an open handle by the live permutation and back through the force: the handle's indices are state of
    the handle, so every call starts by putting them back (a renumbering by the inverse)"""
    h.renumber(live["new_of_old"])
    x = torch.empty_like(live["center"])
    x[live["new_of_old"].long()] = live["center"]
    out = h.force(x)
    inv = torch.empty_like(live["new_of_old"])
    inv[live["new_of_old"].long()] = torch.arange(N, dtype=torch.int32, device="cuda")
    h.renumber(inv)
    return list(out) + list(h.force(live["center"]))


def call_whole_life(live, _):
    """create, force, renumber, force, destroy: the handle's whole life on the current stream"""
    h = _open(live)
    try:
        return call_force(live, h) + call_renumber(live, h)
    finally:
        h.close()


CASES = [Case("angular_force", m_inputs, call_force, ("mhip_angular_springs_force",), open=_open,
              close=lambda h: h.close()),
         Case("angular_renumber", m_inputs, call_renumber, ("mhip_angular_springs_renumber", "mhip_angular_springs_force"),
              open=_open, close=lambda h: h.close()),
         Case("angular_whole_life", m_inputs, call_whole_life,
              ("mhip_angular_springs_create", "mhip_angular_springs_force", "mhip_angular_springs_renumber"))]


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(protos) == 6 and len(streamed) == 3   # set_wca, get and destroy are host calls
    for c in CASES:
        for fn in c.fns:
            assert fn in protos, "%s: %s is not declared in the header" % (c.name, fn)
    assert sorted({f for c in CASES for f in c.fns}) == sorted(streamed)
    assert set(SYNCHRONISES) <= set(streamed)


# ---- the parametrised test --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    su.recording_library(mp)
    # a stream of the high-priority pool: the runtime shares a few hardware queues among the streams of one priority, so
    # a further normal-priority stream here would move every stream a later module creates onto another queue, and the
    # canary of tests/test_gpu_streams.py, which runs after this module, depends on which queue its side stream shares
    # (DESIGN.md 5v).  The high-priority pool has queues of its own, which the null stream never shares; for the ordering
    # these tests check, the priority is immaterial.
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


# ---- coverage: measured, not declared -----------------------------------------------------------------------------------------
@gpu
def test_every_stream_entry_point_of_the_header_was_called(rig):
    assert len(rig["ran"]) == len(CASES), "only %d of %d cases ran in this session: the count needs the whole module" % (
        len(rig["ran"]), len(CASES))
    missing = sorted(n for n in stream_prototypes() if n not in su.CALLED)
    assert not missing, "stream-taking entry points no case called: %s" % missing
    listed = sorted(f for c in CASES for f in c.fns if f not in su.CALLED)
    assert not listed, "entry points a case lists but did not call: %s" % listed
