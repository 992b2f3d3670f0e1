"""Every entry point of include/mundy_hip_periphery_binding.h on a stream that is not the null stream, bit for bit against
the same call on the null stream, with the instrument of tests/test_gpu_streams.py (tests/stream_util.py, imported, not
modified): the real inputs reach the live buffers through a producer that sleeps on the side stream, so a launch, copy or
memset that lands on another stream reads the decoy, and an entry point that blocks although the header calls it
asynchronous finds the stream still busy when it returns.  The last test parses the header and fails for a prototype
with a mhip_stream_t that no case called."""
import os
import re

import numpy as np
import pytest
import torch

import stream_util as su
from stream_util import Case

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_periphery_binding.h")
N, M, P = 3001, 2001, 203   # beads, crosslinkers, sites: no multiple of a wave or a workgroup
XL = dict(kind="hookean", k=3.0, r=1.0, bind_rate=40.0, unbind_rate=10.0, kt=0.5, capture_radius=1.5)
PER = dict(bind_rate=60.0, k=2.0, r=0.8, unbind_rate=15.0, capture_radius=1.7)

SYNCHRONISES = {}   # no entry point of the header returns a host scalar


def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return dict(re.findall(r"\bint\s+(mhip_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S))


def stream_prototypes():
    return {n: a for n, a in header_prototypes().items() if "mhip_stream_t" in a}


def may_block(c):
    return any(f in SYNCHRONISES for f in c.fns)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


_cache = {}


def _system():
    """beads in a box dense enough for a few candidates per row, sites scattered through it; the two CSR lists at these
    positions (fixed: what differs between the real problem and the decoy is every array the calls take)"""
    if "sys" not in _cache:
        from mundy_amd import ops
        rng = np.random.default_rng(70)
        c = rng.uniform(0.0, 11.0, (N, 3))
        left = rng.permutation(N)[:M]
        src = np.zeros(N, np.uint8)
        src[left] = 1
        sites = (np.arange(N) % 3 != 0).astype(np.uint8)
        csr = []
        for n, s, t, reach in ((N, src, sites, 0.5 * XL["capture_radius"] + 0.4),
                               (N + P, np.concatenate([src, np.zeros(P, np.uint8)]),
                                np.concatenate([np.zeros(N, np.uint8), np.ones(P, np.uint8)]),
                                0.5 * PER["capture_radius"] + 0.4)):
            pos = c if n == N else np.concatenate([c, rng.uniform(0.0, 11.0, (P, 3))])
            links = (ops.GenNeighborLinks().set_search_buffer(0.0).set_search_kind(ops.SEARCH_SPHERES)
                     .set_enforce_source_target_symmetry(True).acts_on(dev(s), dev(t)).concretize())
            links.generate(None, dev(pos), torch.full((n,), reach, dtype=torch.float64, device="cuda"))
            csr.append((links.row_ptr.cpu().numpy(), links.col.cpu().numpy(), pos))
            links.close()
        _cache["sys"] = dict(center=c, left=left, sites=sites, bead_csr=csr[0][:2], site_csr=csr[1][:2],
                             points=csr[1][2][N:])
    return _cache["sys"]


def _handle():
    from mundy_amd import ops
    d = _system()
    return ops.Crosslinkers(N, d["left"], None, d["sites"], XL["kind"], XL["k"], XL["r"], XL["bind_rate"],
                            XL["unbind_rate"], XL["kt"], XL["capture_radius"])


def m_inputs(s):
    d = _system()
    rng = np.random.default_rng(71 + s)
    left = d["left"]
    right = left.copy()
    u = rng.random(M)
    right[u < 0.3] = -(rng.integers(0, P, int((u < 0.3).sum())) + 1)
    site_idx = np.flatnonzero(d["sites"])
    right[u > 0.7] = site_idx[rng.integers(0, site_idx.size, int((u > 0.7).sum()))]
    row_ptr, col = d["bead_csr"]
    p_ptr, p_col = d["site_csr"]
    # (the lists are those of the fixed positions, wide enough for the jitter: the decoy differs in positions, sites,
    #  heads, keys, counters and the running count)
    return dict(center=dev(d["center"] + rng.normal(size=(N, 3)) * 0.05),
                points=dev(d["points"] + rng.normal(size=(P, 3)) * 0.05), right=dev(right.astype(np.int32)),
                row_ptr=dev(row_ptr.astype(np.int32)), col=dev(col.astype(np.int32)),
                p_ptr=dev(p_ptr.astype(np.int32)), p_col=dev(p_col.astype(np.int32)),
                keys=dev(rng.integers(0, 1 << 62, M, dtype=np.int64)),
                counters=dev(rng.integers(0, 1 << 40, M, dtype=np.int64)),
                count=dev(rng.integers(0, 1000, 1).astype(np.int32)))


def call_periphery(live, h):
    h.set_periphery_sites(live["points"], PER["bind_rate"], PER["k"], PER["r"], PER["unbind_rate"], PER["capture_radius"])
    h.set_state(None, live["right"])
    h.set_candidates(live["row_ptr"], live["col"], None)
    h.set_periphery_candidates(live["p_ptr"], live["p_col"], col_offset=N)
    z = torch.zeros(M, dtype=torch.float64, device="cuda")
    ev = h.kmc_step(live["center"], 0.01, live["keys"], live["counters"], z_total=z, periphery_bound=live["count"])
    out = [ev, z, h.force(live["center"]), h.state("cuda"), live["counters"], live["count"]]
    # the old entry point on the handle with sites: the same kernel, no count
    ev2 = h.kmc_step(live["center"], 0.01, live["keys"], live["counters"])
    out += [ev2, h.state("cuda"), h.force(live["center"])]
    return out


FNS = ["mhip_crosslinkers_set_periphery_sites", "mhip_crosslinkers_set_periphery_candidates",
       "mhip_crosslinkers_kmc_step_periphery"]
CASES = [Case("periphery_binding", m_inputs, call_periphery, tuple(FNS), open=lambda live: _handle(),
              close=lambda h: h.close())]


# ---- CPU check of the tables ----------------------------------------------------------------------------------------------
def test_tables_name_entry_points_of_the_header():
    protos, streamed = header_prototypes(), stream_prototypes()
    assert len(streamed) == 3 and len(protos) == 3   # every entry point takes a stream
    for c in CASES:
        for fn in c.fns:
            assert fn in protos, "%s: %s is not declared in the header" % (c.name, fn)
    assert sorted(f for c in CASES for f in c.fns) == sorted(streamed)


# ---- the parametrised test --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rig():
    assert torch.cuda.is_available()
    mp = pytest.MonkeyPatch()
    su.recording_library(mp)
    side = torch.cuda.Stream()
    cycles_per_ms = su.calibrate(side)
    _system()
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
