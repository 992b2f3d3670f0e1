"""Bead-spring chains, host side: the numpy restatement passes the generator's known answers and the FENE force is
-grad U, the new entry points are exported and bound, and bad arguments are refused before any HIP call (no GPU)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import chain_model as cm


@pytest.mark.parametrize("ctr,key,want", cm.KAT)
def test_philox_model_known_answers(ctr, key, want):
    got = cm.philox_words(np.array([ctr], dtype=np.uint64), np.array([key], dtype=np.uint64))
    assert got[0].tolist() == list(want)


def test_philox_keying_of_the_library():
    # key (lo32, hi32), counter (lo32, hi32, block, 0): counter 0 / key 0 / block 0 is the first known answer
    assert cm.philox(np.array([0], np.uint64), np.array([0], np.uint64), 0)[0].tolist() == list(cm.KAT[0][2])
    k = np.array([0x299F31D0A4093822], dtype=np.uint64)
    c = np.array([0x85A308D3243F6A88], dtype=np.uint64)
    direct = cm.philox_words(np.array([[0x243F6A88, 0x85A308D3, 7, 0]], np.uint64),
                             np.array([[0xA4093822, 0x299F31D0]], np.uint64))
    assert cm.philox(k, c, 7).tolist() == direct.tolist()


def test_uniform_to_normal_map_ends():
    # all-zero words: u1 = 2^-53 (never 0), u2 = 0; all-one words: u1 = 1, so the radius is 0
    z0, z1 = cm.box_muller(np.zeros((1, 4), np.uint32))
    assert z0[0] == math.sqrt(-2.0 * math.log(2.0 ** -53)) and z1[0] == 0.0
    z0, z1 = cm.box_muller(np.full((1, 4), 0xFFFFFFFF, np.uint32))
    assert abs(z0[0]) == 0.0 and abs(z1[0]) == 0.0


def test_normals_are_standard():
    n = 200000
    z = cm.normals(np.arange(n, dtype=np.uint64), np.zeros(n, np.uint64))
    assert np.all(np.abs(z.mean(axis=0)) < 5.0 / math.sqrt(n))
    assert np.all(np.abs(z.var(axis=0) - 1.0) < 5.0 * math.sqrt(2.0 / n))


@pytest.mark.parametrize("L", [0.1, 0.7, 1.2, 1.45])
def test_fene_force_is_minus_grad_of_its_potential(L):
    k, rmax = 3.0, 1.5
    rng = np.random.default_rng(3)
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    xi = np.array([0.3, -0.2, 1.0])
    c = np.stack([xi, xi + L * u])
    f, over, mx = cm.spring_force(2, [[0, 1]], "fene", k, rmax, c)
    assert over == 0 and mx == pytest.approx(L, rel=1e-15)
    h = 1e-6
    for a in range(3):
        cp, cmn = c.copy(), c.copy()
        cp[0, a] += h
        cmn[0, a] -= h
        Lp, Lm = np.linalg.norm(cp[1] - cp[0]), np.linalg.norm(cmn[1] - cmn[0])
        fd = -(cm.fene_energy(Lp, k, rmax) - cm.fene_energy(Lm, k, rmax)) / (2 * h)
        assert f[0, a] == pytest.approx(fd, rel=1e-7, abs=1e-7 * np.abs(f[0]).max())
    assert np.dot(f[0], c[1] - c[0]) > 0.0  # attractive: body i is pulled towards j
    assert (f[1] == -f[0]).all()


def test_fene_overstretched_has_no_force():
    c = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [3.5, 0, 0]])
    f, over, mx = cm.spring_force(3, [[0, 1], [1, 2]], "fene", 3.0, 1.5, c)
    assert over == 2 and np.isnan(f).all() and mx == 2.0


def test_hookean_two_bead_closure():
    # m_i = m_j = m: L - r0 shrinks by 1 - 2 k m dt per Euler step
    k, r0, m, dt = 3.0, 1.0, 0.1, 1e-3
    c = np.array([[0.0, 0.0, 0.0], [1.7, 0.0, 0.0]])
    f, _, _ = cm.spring_force(2, [[0, 1]], "hookean", k, r0, c)
    c2 = c + dt * m * f
    assert (c2[1, 0] - c2[0, 0] - r0) == pytest.approx(0.7 * (1 - 2 * k * m * dt), rel=1e-14)


def test_isolated_bodies_get_plus_zero():
    f, _, _ = cm.spring_force(4, [[1, 2]], "hookean", 1.0, 0.5, np.arange(12, dtype=float).reshape(4, 3))
    assert (f[[0, 3]].view(np.uint64) == 0).all()


def test_chain_generator_spacing_and_no_overlap_between_chains():
    from mundy_amd import synth
    d = synth.chains(8, 40, seed=5)
    c, p, ch = d["center"], d["pairs"], d["chain"]
    assert c.shape == (320, 3) and p.shape == (8 * 39, 2)
    L = np.linalg.norm(c[p[:, 1]] - c[p[:, 0]], axis=1)
    assert np.allclose(L, 1.0, rtol=1e-12)
    diff = np.linalg.norm(c[:, None] - c[None], axis=2)
    other = ch[:, None] != ch[None]
    assert (diff[other] >= 2 * 0.5).all()
    assert (d["k"], d["kt"], d["viscosity"], d["dt"], d["skin"]) == (3.0, 0.1, 1.0, 1e-3, 1.0)


def test_step_stats_gain_max_spring_length_with_default_zero():
    from mundy_amd import pipeline
    assert pipeline.StepStats().max_spring_length == 0.0


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def test_new_entry_points_are_exported_and_bound(lib):
    from mundy_amd import capi
    for name in ("mhip_springs_create", "mhip_springs_force", "mhip_springs_destroy", "mhip_philox4x32_10",
                 "mhip_brownian_velocity", "mhip_drag_velocity", "mhip_contact_op_constraint_rate"):
        assert hasattr(lib, name) and name in capi.SIGNATURES


def _create(lib, n=4, pairs=((0, 1), (1, 2)), kind=0, k=None, k0=3.0, r=None, r0=1.0):
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    arr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    ka, ra = arr(k), arr(r)
    h = C.c_void_p(12345)
    st = lib.mhip_springs_create(C.byref(h), n, p.shape[0], p.ctypes.data_as(C.c_void_p), kind,
                                 None if ka is None else ka.ctypes.data_as(C.c_void_p), k0,
                                 None if ra is None else ra.ctypes.data_as(C.c_void_p), r0, None)
    return st, h


@pytest.mark.parametrize("kw,match", [
    (dict(pairs=((0, 4),)), "outside"), (dict(pairs=((-1, 2),)), "outside"), (dict(pairs=((2, 2),)), "itself"),
    (dict(k0=-1.0), "k must"), (dict(k0=math.nan), "k must"), (dict(k0=math.inf), "k must"),
    (dict(k=[3.0, -0.5]), "k must"), (dict(k=[3.0, math.nan]), "k must"), (dict(r0=-0.1), "rest length"),
    (dict(r=[1.0, math.inf]), "rest length"), (dict(kind=1, r0=0.0), "r_max"), (dict(kind=1, r=[1.0, -1.0]), "r_max"),
    (dict(kind=1, r0=math.nan), "r_max"), (dict(kind=7), "spring type")])
def test_springs_create_refuses_bad_arguments(lib, kw, match):
    from mundy_amd import capi
    st, h = _create(lib, **kw)
    with pytest.raises(ValueError, match=match):
        capi.check(st)
    assert h.value is None  # nothing was created


P = lambda v: None if not v else C.c_void_p(16 * int(v))  # noqa: E731  (fake device pointers, never dereferenced)


@pytest.mark.parametrize("kt,dt,match", [(-0.1, 1e-3, "kt"), (math.nan, 1e-3, "kt"), (math.inf, 1e-3, "kt"),
                                         (0.1, 0.0, "dt"), (0.1, -1e-3, "dt"), (0.1, math.inf, "dt")])
def test_brownian_refuses_bad_numbers(lib, kt, dt, match):
    from mundy_amd import capi
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_brownian_velocity(4, P(1), P(2), kt, dt, P(3), P(4), None))


def test_null_pointers_are_refused(lib):
    from mundy_amd import capi
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_brownian_velocity(4, P(1), None, 0.1, 1e-3, P(3), P(4), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_philox4x32_10(4, P(1), P(2), 0, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_springs_force(None, P(1), P(2), P(3), P(4), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_contact_op_constraint_rate(None, P(1), P(2), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_drag_velocity(4, None, None, P(1), None))


def test_python_wrappers_check_first():
    from mundy_amd import ops
    with pytest.raises(ValueError, match="kt"):
        ops.brownian_velocity(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), -1.0, 1e-3,
                              torch.ones(2, dtype=torch.float64), torch.zeros((2, 6), dtype=torch.float64))
    with pytest.raises(ValueError, match="block"):
        ops.philox4x32_10(torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), block=2 ** 32)
    with pytest.raises(ValueError, match="itself"):
        ops.Springs(3, [[0, 0]], "hookean", 1.0, 1.0)
    with pytest.raises(ValueError, match="spring type"):
        ops.Springs(3, [[0, 1]], "harmonic", 1.0, 1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.Springs(3, [[0, 1], [1, 2]], "fene", [1.0], 1.5)


def _stepper(**kw):
    from mundy_amd import pipeline
    n = 4
    c = torch.zeros((n, 3), dtype=torch.float64)
    r = torch.full((n,), 0.5, dtype=torch.float64)
    kind = kw.pop("kind", "sphere")
    extra = {}
    if kind == "spherocylinder":
        extra = dict(quat=torch.zeros((n, 4), dtype=torch.float64), length=torch.ones(n, dtype=torch.float64))
    return pipeline.ContactStepper(kind, c, r, **extra, **kw)


SPR = ([[0, 1], [1, 2], [2, 3]], "hookean", 3.0, 1.0)


@pytest.mark.parametrize("kw,match", [
    (dict(kind="spherocylinder", springs=SPR), "spheres only"),
    (dict(kind="spherocylinder", brownian_kt=0.1), "spheres only"),
    (dict(kind="spherocylinder", brownian_kt=0.1, growth_rate=0.1, division_length=2.0), "spheres only"),
    (dict(springs=SPR, periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(brownian_kt=0.1, friction=0.3), "friction"), (dict(springs=SPR, contact_cutoff=0.1), "contact_cutoff"),
    (dict(brownian_kt=-0.1), "brownian_kt"), (dict(brownian_kt=math.nan), "brownian_kt"),
    (dict(brownian_kt=math.inf), "brownian_kt"),
    (dict(springs=([[0, 4]], "hookean", 3.0, 1.0)), "outside"), (dict(springs=([[0, 1]], "fene", 3.0, 0.0)), "r_max"),
    (dict(springs=([[0, 1]], "hookean", -3.0, 1.0)), "k must"), (dict(springs=([[0, 1]], "hookean", 3.0)), "springs"),
    (dict(brownian_kt=0.1, rng_keys=torch.tensor([0, 1, 2, -1])), r"2\^63"),
    (dict(brownian_kt=0.1, rng_keys=torch.arange(3)), "rng_keys"),
    (dict(brownian_kt=0.1, rng_keys=torch.ones(4, dtype=torch.float64)), "rng_keys"),
    (dict(brownian_kt=0.1, rng_counter=torch.tensor([0, 1, 2, -5])), r"2\^63"),
    (dict(rng_keys=torch.arange(4)), "brownian_kt"), (dict(springs=SPR, rng_counter=torch.arange(4)), "brownian_kt")])
def test_stepper_refuses_what_the_chain_step_does_not_have(kw, match):
    # refused in the constructor before anything reaches the device (these tensors are on the CPU)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


def test_chain_step_app_compiles_and_links():
    import os
    from cpp_apps import build_app
    exe = build_app("chain_step_app")
    assert os.path.exists(exe)


def test_statistics_table_is_sound():
    """every entry of the chain step's statistics array has a place of its own, and lies inside the array of the first
    mode that writes it (no library, no device: the layout is DESIGN.md 5h)"""
    from mundy_amd import pipeline
    table, length = pipeline.STATS, pipeline.STATS_LENGTH
    assert length == dict(chain=3, crosslinkers=6, nucleus=9)
    places = [(slot, lane) for _, slot, lane in table.values()]
    assert len(set(places)) == len(places)
    float_slots = {slot for slot, lane in places if lane is None}
    int_slots = {slot for slot, lane in places if lane is not None}
    assert not float_slots & int_slots
    assert all(lane in (None, 0, 1) for _, lane in places)
    for name, (mode, slot, lane) in table.items():
        assert 0 <= slot < length[mode], name
    assert float_slots | int_slots == set(range(9))
    # the accessor returns views of the buffer at those places, for the device array and its host copy alike
    buf = torch.zeros(9, dtype=torch.float64)
    for k, name in enumerate(table):
        pipeline.stat(buf, name)[0] = k + 1
    assert buf.tolist()[:2] == [1.0, 2.0] and buf.view(torch.int32).tolist()[4:6] == [3, 0]
    for k, (name, (_, slot, lane)) in enumerate(table.items()):
        got = buf[slot] if lane is None else buf.view(torch.int32)[2 * slot + lane]
        assert got == k + 1, name
    # a pair is two entries in lanes 0 and 1 of one slot, and its view holds both
    for pair, (first, second) in pipeline.STAT_PAIRS.items():
        assert pair not in table and table[first][1:] == (table[second][1], 0) and table[second][2] == 1
        assert table[first][0] == table[second][0]
    assert pipeline.stat(buf, "crosslinker_events").tolist() == [4, 5]
    assert pipeline.stat(buf, "active_switches").tolist() == [11, 12]
    # and the decode of the step's one readback gives every name its value, or leaves out what a shorter array lacks
    assert pipeline.read_stats(buf) == {name: k + 1 for k, name in enumerate(table)}
    for mode, count in length.items():
        assert set(pipeline.read_stats(buf[:count])) == {name for name, (m, slot, _) in table.items() if slot < count}
        assert {name for name, (m, _, _) in table.items() if m == mode} <= set(pipeline.read_stats(buf[:count]))
