"""What a closed handle leaves behind: nothing.  Every handle of the library is made of owning members (csrc/
mhip_internal.hpp: HandleBuffer, PinnedBlock), a destroyed operator's workspaces move as one struct into the spare set,
and mhip_memory_stats counts the bytes those types hold.  Each case builds its objects, uses them so that the lazily
reserved buffers exist, closes them, releases the spare set and compares the counters with their values at the start of
the case -- zero when nothing else in the process holds a handle.  The equalities are exact: these are counts."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import torch
    assert torch.cuda.is_available()
    from mundy_amd import ops as o
    return o


def settled(ops):
    """(handle_bytes, pinned_bytes) once dropped wrappers are collected and the spare set is released"""
    from mundy_amd import capi
    gc.collect()
    capi.check(capi.load().mhip_release_cached_workspaces())
    m = ops.memory_stats()
    return m["handle_bytes"], m["pinned_bytes"]


def held(ops):
    m = ops.memory_stats()
    return m["handle_bytes"], m["pinned_bytes"]


def test_broadphase_grid_and_lbvh(ops):
    import torch
    from gpu_util import dev
    from mundy_amd import synth
    start = settled(ops)
    s = synth.spheres(512)
    n = 512
    c, r = dev(s["center"]), dev(s["radius"])
    src = torch.ones(n, dtype=torch.uint8, device="cuda")
    tgt = torch.ones(n, dtype=torch.uint8, device="cuda")
    tgt[::7] = 0
    ex_ptr = dev(np.arange(n + 1, dtype=np.int32))            # every body excludes its successor
    ex_idx = dev(((np.arange(n) + 1) % n).astype(np.int32))
    ids = dev(np.arange(n, dtype=np.int64) + 1000)
    ranks = dev(np.zeros(n, dtype=np.int32))
    for method in (ops.SEARCH_METHOD_GRID, ops.SEARCH_METHOD_MORTON_LBVH):
        g = (ops.GenNeighborLinks().set_search_buffer(0.3).set_search_kind(ops.SEARCH_SPHERES).set_search_method(method)
             .acts_on(src, tgt).concretize())
        g.set_excluded_partners(ex_ptr, ex_idx)
        g.set_identities(ids, ranks)
        assert g.generate(None, c, r) and g.num_pairs > 0
        assert g.method_used() == method
        lid, _, _ = g.export_coo()
        assert lid.shape[0] == g.num_pairs
        g.export_crs()
        now = held(ops)
        assert now[0] > start[0] and now[1] > start[1], (start, now)   # device buffers and the two pinned blocks
        g.close()
    assert settled(ops) == start


def _use_operator(ops, P, profile):
    import torch
    from gpu_util import dev
    from test_gpu_convex import _gpu_op
    C, N = len(P["pairs"]), P["N"]
    op = _gpu_op(ops, P)
    if profile:
        op.set_profiling(True)
    _, _, res = ops.solve_lcp(op, dev(P["sep"]), dev(np.zeros(C)), ops.PGDConfig(max_iters=300, tol=1e-6))
    assert res.num_iters > 0
    if profile:
        assert op.get_profile()[2] > 0                       # the events exist
    if P["ra"] is not None:                                  # the rod forms
        op.constraint_rate(torch.ones((N, 6), dtype=torch.float64, device="cuda"))
        op.body_sweep_vector(torch.ones((C, 3), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    op.close()


@pytest.mark.parametrize("form", ["spheres", "rods_vector_arms", "rods_arclength_arms"])
def test_operator_three_kinematics(ops, oracle, form):
    from test_gpu_convex import _rod_problem, _rod_problem_arclength, _sphere_problem
    maker = {"spheres": _sphere_problem, "rods_vector_arms": _rod_problem, "rods_arclength_arms": _rod_problem_arclength}[form]
    P = maker(oracle, 512, seed=3)
    assert len(P["pairs"]) > 0
    start = settled(ops)
    allocations = []
    for _ in range(4):
        _use_operator(ops, P, profile=(form == "rods_arclength_arms"))
        allocations.append(ops.memory_stats()["allocations"])
        assert held(ops)[0] > start[0]                       # the spare set holds the closed operator's workspaces
    print("allocations after each of four operators:", allocations)
    assert allocations[2] == allocations[1] and allocations[3] == allocations[1], allocations
    assert settled(ops) == start


def test_operator_with_tiers(ops, oracle):
    from gpu_util import dev
    from test_gpu_convex import _gpu_op, _rod_problem_arclength
    P = _rod_problem_arclength(oracle, 12000, seed=41)
    C = len(P["pairs"])
    assert C >= 65536, C
    start = settled(ops)
    op = _gpu_op(ops, P)
    op.set_tiering(3)
    ops.solve_lcp(op, dev(P["sep"]), dev(np.zeros(C)), ops.PGDConfig(max_iters=10000, tol=1e-6))
    stats = op.tier_stats()
    assert stats["tiered_iterations"] > 0, stats             # the nine tier buffers existed
    op.close()
    assert settled(ops) == start


def test_failed_create(ops):
    import torch
    from gpu_util import dev
    z = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")  # noqa: E731
    bad = dev(np.array([[0, 9]], dtype=np.int32))
    normal, mob = z(1, 3), z(5)
    start = settled(ops)
    with pytest.raises(ValueError, match="outside"):
        ops.ContactOperator(bad, normal, mob, 1e-3)
    assert held(ops)[0] > start[0]                           # what the refused operator had reserved: now the spare set
    assert settled(ops) == start


def test_second_operator_while_the_spare_is_held(ops, oracle):
    from gpu_util import dev
    from test_gpu_convex import _gpu_op, _sphere_problem
    P = _sphere_problem(oracle, 512, seed=3)
    start = settled(ops)
    a, b = _gpu_op(ops, P), _gpu_op(ops, P)
    for op in (a, b):
        op.apply(dev(np.ones(len(P["pairs"]))))
    import torch
    torch.cuda.synchronize()
    two = held(ops)
    a.close()
    assert held(ops) == two                                  # moved into the spare set, nothing freed
    b.close()                                                # the spare is held: this set is freed
    one = held(ops)
    assert one[0] - start[0] == (two[0] - start[0]) // 2 > 0 and one[1] - start[1] == (two[1] - start[1]) // 2 > 0
    assert settled(ops) == start


def test_hydro_workspace(ops):
    import hydro_model as hm
    from gpu_util import dev
    start = settled(ops)
    d = hm.inputs(1500, 64, seed=60)                          # two chunks of sources: `partial` is reserved
    assert 1500 > hm.CHUNK
    ws = ops.HydroWorkspace()
    ws.set_path("partial")
    ops.hydro_velocity("rpyc", 0.7, dev(d["sc"]), dev(d["sa"]), dev(d["f"]), dev(d["tc"]), dev(d["tb"]), workspace=ws)
    assert held(ops)[0] > start[0]
    ws.close()
    assert settled(ops) == start


@pytest.mark.parametrize("what", ["springs", "crosslinkers", "active_springs", "filaments", "filament_contacts"])
def test_force_handles(ops, what):
    # one create, one use, one close each, as the whole-life cases of test_gpu_streams.py run them
    import test_gpu_streams as ts
    make, life = {"springs": (ts.m_chain_centres, ts.call_springs_lifecycle),
                  "crosslinkers": (ts.m_crosslinkers, ts.call_crosslinkers_lifecycle),
                  "active_springs": (ts.m_active, ts.call_active_lifecycle),
                  "filaments": (ts.m_filaments, ts.call_filaments),
                  "filament_contacts": (ts.m_filament_contacts, ts.call_filament_contacts)}[what]
    live = make(0)
    start = settled(ops)
    before = ops.memory_stats()["allocations"]
    life(live, None)
    assert ops.memory_stats()["allocations"] > before        # the handle did reserve counted buffers
    assert settled(ops) == start


def test_scratch_is_steady(ops):
    import torch
    from gpu_util import dev
    from mundy_amd import pipeline, synth
    b = synth.spherocylinders(512)
    start = settled(ops)
    st = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]), dev(b["length"]),
                                 search_buffer=0.1, cfg=ops.PGDConfig(max_iters=2000, tol=1e-5))
    readings = []
    for _ in range(2):
        for _ in range(3):
            st.step(force_rebuild=True)
        torch.cuda.synchronize()
        m = ops.memory_stats()
        readings.append((m["allocations"], m["scratch_bytes"]))
    print("(allocations, scratch_bytes) after three and after six rebuilt steps:", readings)
    assert readings[1] == readings[0], readings
    st.op.close()
    st.links.close()
    del st
    assert settled(ops) == start
