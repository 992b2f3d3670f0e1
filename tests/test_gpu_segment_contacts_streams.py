"""Every entry point of include/mundy_hip_segment_contact.h on a stream that is not the null stream, bit for bit against
the same call on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py, imported, not
modified): the real inputs reach the live buffers through a producer that sleeps on the side stream, so a launch, memset
or copy that lands on another stream reads the decoy, and an entry point that blocks although the header calls it
asynchronous finds the stream still busy when it returns.  The last test parses the header and fails for a prototype with
a mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import segment_contact_model as scm
import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_segment_contact.h")

# create waits for its uploads (its host arrays may go when it returns); update returns the host flag `rebuilt`
SYNCHRONISES = {"mhip_segment_contacts_create": "synchronises the stream before it returns",
                "mhip_segment_contacts_update": "returns a host flag"}


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


def _ends():
    return scm.case("jittered_lattice")["ends"]


def m_inputs(s):
    """seed 0: the jittered lattice of the other tests; seed 1: the same lattice with another jitter"""
    c = scm.case("jittered_lattice")["center"] if s == 0 else scm.lattice(4, 40, 0.9, 0.9, 0.05, 77)[0]
    return dict(center=dev(c), acc=dev(np.random.default_rng(50 + s).normal(size=c.shape)))


def _new(kind):
    return O().SegmentContacts(scm.case("jittered_lattice")["n"], kind=kind, radius=scm.RADIUS, skin=scm.SKIN,
                               segments=_ends())


def open_updated(kind):
    def open_(live):
        sc = _new(kind)
        sc.update(live["center"])
        return sc
    return open_


def open_bin(live):
    return []   # the handles a call creates, closed with the case


def close_bin(handles):
    for h in handles:
        h.close()


def call_create(kind):
    def call(live, handles):
        sc = _new(kind)
        handles.append(sc)
        rebuilt = sc.update(live["center"])
        f, stats = sc.force(live["center"])
        return rebuilt, sc.field("pairs"), f, stats.clone()
    return call


def call_update(live, sc):
    # the list's age is state of the handle: every call starts from a forced rebuild, then asks the moved test
    first = sc.update(live["center"], force_rebuild=True)
    second = sc.update(live["center"])
    return first, second, sc.field("pairs"), sc.field("aabb"), sc.field("seg")


def call_force(live, sc):
    f, stats = sc.force(live["center"])
    stats = stats.clone()
    sc.force(live["center"], out=live["acc"], accumulate=True)
    return f, stats, live["acc"], sc.field("sep"), sc.field("force"), sc.field("share")


def call_halves(live, sc):
    # force() lays the segment view of the live centres; the halves then run over it
    sc.force(live["center"])
    stats = torch.empty(2, dtype=torch.int64, device="cuda")
    sc.linker_pass(stats)
    after_pass = stats.clone()
    f = sc.reduce(stats=stats)
    sc.reduce(out=live["acc"], accumulate=True)
    return after_pass, stats, f, live["acc"], sc.field("force")


def close_handle(sc):
    sc.close()


CASES = []
for kind_ in ("hertz", "wca"):
    CASES.append(Case("create_%s" % kind_, m_inputs, call_create(kind_),
                      ("mhip_segment_contacts_create", "mhip_segment_contacts_update", "mhip_segment_contacts_force"),
                      open=open_bin, close=close_bin))
    CASES.append(Case("update_%s" % kind_, m_inputs, call_update, ("mhip_segment_contacts_update",),
                      open=open_updated(kind_), close=close_handle))
    CASES.append(Case("force_%s" % kind_, m_inputs, call_force, ("mhip_segment_contacts_force",),
                      open=open_updated(kind_), close=close_handle))
    CASES.append(Case("halves_%s" % kind_, m_inputs, call_halves,
                      ("mhip_segment_contacts_force", "mhip_segment_contacts_linker_pass",
                       "mhip_segment_contacts_reduce"), open=open_updated(kind_), close=close_handle))


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) == 5 and len(protos) == 7
    for name in SYNCHRONISES:
        assert name in streamed
    for c in CASES:
        for fn in c.fns:
            assert fn in protos, "%s: %s is not declared in the header" % (c.name, fn)
    assert len({c.name for c in CASES}) == len(CASES)
    assert {f for c in CASES for f in c.fns} == set(streamed)


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
