"""Growth and division on the GPU: the three kernels bit for bit against tests/growth_model.py, and the growth-mode
stepper -- lengths and counts against the length recursion, the corner rebuild rule (no missed contact), no stale state
after births, determinism and reordering, the periodic box, the C++ stepper against the Python one, one step at full
size."""
import subprocess

import numpy as np
import pytest

import growth_model as gm

pytestmark = pytest.mark.gpu

SENTINEL = np.array([0x7FF4DEADBEEF0123], dtype=np.uint64).view(np.float64)[0]  # a signalling-NaN pattern


def _lengths(rng, n, mode, D):
    if mode == "none":
        return rng.uniform(1.2, D, n)
    if mode == "all":
        return rng.uniform(D + 1e-9, 2 * D, n)
    L = rng.uniform(1.2, D, n)
    if mode == "first" and n:
        L[0] = D + 0.5
    elif mode == "last" and n:
        L[-1] = D + 0.5
    elif mode == "mixed":
        L = rng.uniform(1.2, 2 * D, n)
        L[rng.random(n) < 0.1] = D           # exactly the threshold: does not divide
        L[rng.random(n) < 0.05] = np.nan      # NaN: does not divide
    return L


def _run_kernels(c, q, r, L, D, dt, rate, box, spare=5):
    import torch
    from gpu_util import dev, host
    from mundy_amd import ops
    n = len(r)
    rows = 2 * n + spare  # room for every body to divide, and rows nobody may touch

    def pad(a, w):
        out = np.full((rows, w) if w > 1 else rows, SENTINEL)
        out[:n] = a
        return dev(out)
    dc, dq, dr, dL = pad(c, 3), pad(q, 4), pad(r, 1), pad(L, 1)
    parent_of, nb = ops.select_dividing(dL[:n], D)
    ops.divide_grow_spherocylinders(n, parent_of, dt, rate, dc, dq, dr, dL, box=box)
    torch.cuda.synchronize()
    return host(parent_of), nb, host(dc), host(dq), host(dr), host(dL)


def _assert_rows(got, want, n_live, what):
    from gpu_util import assert_bits_equal
    g, w = got[:n_live], want
    nan_g, nan_w = np.isnan(g), np.isnan(w)
    assert np.array_equal(nan_g, nan_w), what + ": NaN positions differ"
    assert_bits_equal(np.where(nan_g, 0.0, g), np.where(nan_w, 0.0, w), what)
    tail = got[n_live:]
    assert (np.ascontiguousarray(tail).view(np.uint64) == SENTINEL.view(np.uint64)).all(), what + ": spare rows written"


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000, 100_003])
@pytest.mark.parametrize("mode", ["none", "all", "first", "last", "mixed"])
def test_divide_grow_matches_the_model_bit_for_bit(n, mode):
    from gpu_util import random_rods
    rng = np.random.default_rng(n * 7 + len(mode))
    D, dt, rate = 2.5, 1e-3, 0.1
    box = 10.0 + 3.0 * (n % 2)
    c, q, r, _ = random_rods(rng, n, box, rmin=0.3, rmax=0.6)  # per-body radii
    q = q * rng.uniform(0.5, 2.0, (n, 1))                      # not unit: qrot divides by |q|^2
    L = _lengths(rng, n, mode, D)
    for periodic in (False, True):
        b = (box, box + 1.0, box + 2.0) if periodic else None
        parent_of, nb, gc, gq, gr, gL = _run_kernels(c, q, r, L, D, dt, rate, b)
        want_p = gm.select_dividing(L, D)
        assert nb == len(want_p) and parent_of.tolist() == want_p.tolist()
        wc, wq, wr, wL = gm.divide_grow(c, q, r, L, want_p, dt, rate, box=b)
        m = n + nb
        _assert_rows(gc, wc, m, "center")
        _assert_rows(gq, wq, m, "quat")
        _assert_rows(gr, wr, m, "radius")
        _assert_rows(gL, wL, m, "length")
        if mode == "all":
            assert nb == n
        if mode in ("first", "last") and n:
            assert parent_of.tolist() == [0 if mode == "first" else n - 1]
        if periodic and nb:
            assert (wc[:m] >= 0).all() and (wc[:m] < np.array(b)).all()


def test_children_crossing_a_face_are_wrapped():
    rng = np.random.default_rng(5)
    n, box = 200, (6.0, 6.0, 6.0)
    c = rng.uniform(0, 6.0, (n, 3))
    c[:, 0] = rng.choice([0.05, 5.95], n)   # next to the x faces, axis along x: one child of each crosses
    q = np.tile([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0], (n, 1))  # zhat -> xhat
    r, L = np.full(n, 0.5), np.full(n, 3.0)
    parent_of, nb, gc, gq, gr, gL = _run_kernels(c, q, r, L, 2.0, 0.0, 0.0, box)
    assert nb == n
    wc, wq, wr, wL = gm.divide_grow(c, q, r, L, parent_of, 0.0, 0.0, box=box)
    _assert_rows(gc, wc, 2 * n, "center")
    assert (gc[:2 * n] >= 0).all() and (gc[:2 * n] < 6.0).all()


def test_aabb_moved_matches_numpy_at_the_threshold():
    from gpu_util import dev
    from mundy_amd import ops
    rng = np.random.default_rng(3)
    for n in (1, 64, 65, 10_001):
        ref = rng.uniform(-5, 5, (n, 6))
        small = ref + rng.uniform(-0.1, 0.1, (n, 6))
        assert ops.aabb_moved(dev(small), dev(ref), 0.5) is gm.aabb_moved(small, ref, 0.5) is False
        for corner in (0, 3):
            k = n // 2
            at = ref.copy()
            at[k, corner] = 0.0
            at[k, corner + 1] = 0.0
            base = at.copy()
            at[k, corner + 2] = 0.5
            base[k, corner + 2] = 0.0
            below = at.copy()
            below[k, corner + 2] = np.nextafter(0.5, 0.0)
            ref_k = base
            assert ops.aabb_moved(dev(at), dev(ref_k), 0.5) and gm.aabb_moved(at, ref_k, 0.5)
            assert not ops.aabb_moved(dev(below), dev(ref_k), 0.5) and not gm.aabb_moved(below, ref_k, 0.5)
    empty = dev(np.zeros((0, 6)))
    assert ops.aabb_moved(empty, empty, 0.1) is False


def _colony(seed, n, D=2.0, r=0.5):
    """n rods (synth.spherocylinders, box edge b["box"]) with lengths uniform in (cl_min, D], cl_min = 0.5 D - r: a
    fresh child's length"""
    from mundy_amd import synth
    b = synth.spherocylinders(n, radius=r, seed=seed)
    cl_min = 0.5 * D - r
    b["length"] = cl_min + (D - cl_min) * (1.0 - synth.uniform01(seed, np.arange(n), 9))
    return b


def _stepper(b, box=None, **kw):
    from gpu_util import dev
    from mundy_amd import pipeline
    args = dict(dt=1e-3, viscosity=1.0, search_buffer=0.5, contact_model="hertz", growth_rate=5.0,
                division_length=2.0, periodic_box=box)
    args.update(kw)
    return pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]),
                                   dev(b["length"]), **args)


def test_colony_from_one_rod_follows_the_length_recursion():
    from gpu_util import host
    from mundy_amd import ops
    # a fast-growing line of rods: hard contact (the LCP) keeps it free of interpenetration whatever the growth speed
    L0, r, D, dt, rate = 2.0, 0.5, 2.0, 1e-3, 50.0
    b = dict(center=np.array([[0.1, 6.0, 6.0]]), quat=np.array([[np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0]]),
             radius=np.array([r]), length=np.array([L0]))
    st = _stepper(b, dt=dt, growth_rate=rate, division_length=D, search_buffer=0.5, contact_model="lcp",
                  cfg=ops.PGDConfig(max_iters=2000, tol=1e-5))
    steps = 0
    want = gm.length_recursion([L0], [r], D, dt, rate, 400)
    parent_id = {}
    while st.n < 128:
        ids_before = host(st.ids).copy()
        s = st.step()
        n_now, L_want = want[steps]
        assert s.num_bodies == st.n == n_now, steps
        assert np.array_equal(np.sort(host(st.length)), L_want), steps
        ids = host(st.ids)
        assert len(set(ids.tolist())) == st.n
        if s.num_born:
            p = host(st.last_parent_of)
            for k, child in enumerate(ids[st.n - s.num_born:]):
                parent_id[int(child)] = int(ids_before[p[k]])
            assert s.rebuilt
        assert np.isfinite(host(st.center)).all(), steps
        steps += 1
        assert steps < 400
    assert st.n == 128
    # every id but the root has one parent with a smaller id; following parents always ends at id 0
    assert sorted(parent_id) == list(range(1, 128))
    for child in parent_id:
        x = child
        while x != 0:
            assert parent_id[x] < x
            x = parent_id[x]


def test_centres_stay_in_the_periodic_box_after_births():
    from gpu_util import host
    b = _colony(61, 300)
    box = float(b["box"])
    b["center"][:20, 0] = 0.02            # next to a face: children of the dividing ones cross it
    b["length"][:20] = 2.0 + 1e-12 * np.arange(1, 21)
    st = _stepper(b, box=(box, box, box))
    born = 0
    for k in range(30):
        s = st.step()
        born += s.num_born
        c = host(st.center)
        assert (c >= 0).all() and (c < box).all(), k
    assert born >= 20


def test_growing_rods_enter_the_list_before_they_overlap():
    from gpu_util import dev, host
    from mundy_amd import pipeline
    buffer, eps, g = 0.25, 0.01, 0.004
    r, L = 0.5, 2.0
    gap = 2 * buffer + eps  # between the tips
    c = np.array([[0.0, 0.0, 0.0], [L + 2 * r + gap, 0.0, 0.0]])
    q = np.tile([np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0], (2, 1))  # both along x, tip to tip
    st = pipeline.ContactStepper("spherocylinder", dev(c), dev(np.full(2, r)), dev(q), dev(np.full(2, L)), dt=1e-3,
                                 search_buffer=buffer, contact_model="hertz", growth_rate=g / 1e-3, division_length=100.0,
                                 mob_trans=dev(np.zeros(2)), mob_rot=dev(np.zeros(2)))  # the rods only grow
    entered = None
    for k in range(140):
        s = st.step()
        true_sep = gap - (k + 1) * g            # the tips advance g / 2 each per step
        listed = s.num_contacts > 0
        if listed and entered is None:
            entered = k
        if true_sep < 1e-9:
            assert listed, "step %d: overlapping rods (sep %g) are not in the neighbour list" % (k, true_sep)
            assert host(st.contacts["sep"])[0] < 1e-9
    assert entered is not None and gap - (entered + 1) * g > 0, "the pair must be listed before the rods touch"


def test_no_contact_is_missed_over_a_colony_trajectory():
    import oracle
    from gpu_util import host
    b = _colony(11, 500)
    st = _stepper(b)
    births = 0
    for k in range(40):
        s = st.step()
        births += s.num_born
        n = st.n
        seg = host(st.seg)   # the segments of this step's contact stage (before the Euler update)
        i, j = np.triu_indices(n, 1)
        pairs = np.stack([i, j], axis=1).astype(np.int32)
        sep = oracle.contact_spherocylinders(pairs, seg, seg[:, :3])["sep"]
        overl = {tuple(p) for p in pairs[sep < 0].tolist()}
        listed = {tuple(sorted(p)) for p in host(st.links.pairs).tolist()}
        missing = overl - listed
        assert not missing, "step %d: %d overlapping pairs missing from the list" % (k, len(missing))
    assert births > 0


@pytest.mark.parametrize("model", ["hertz", "lcp"])
def test_a_step_with_births_equals_a_fresh_stepper(model):
    import torch
    from gpu_util import assert_bits_equal, dev, host
    from mundy_amd import ops, pipeline
    b = _colony(21, 400)
    kw = dict(contact_model=model, cfg=ops.PGDConfig(max_iters=2000, tol=1e-6))
    st = _stepper(b, **kw)
    seen_births = checked = 0
    for k in range(60):
        snap = {name: host(getattr(st, name)).copy() for name in ("center", "quat", "radius", "length", "mob_trans",
                                                                   "mob_rot", "ids")}
        s = st.step()
        if seen_births and s.num_born:
            fresh = pipeline.ContactStepper(
                "spherocylinder", dev(snap["center"]), dev(snap["radius"]), dev(snap["quat"]), dev(snap["length"]),
                dt=1e-3, viscosity=1.0, search_buffer=0.5, growth_rate=5.0, division_length=2.0,
                mob_trans=dev(snap["mob_trans"]), mob_rot=dev(snap["mob_rot"]), ids=dev(snap["ids"]), **kw)
            f = fresh.step()
            torch.cuda.synchronize()
            assert f.num_born == s.num_born and f.rebuilt and s.rebuilt
            assert f.num_contacts == s.num_contacts
            assert np.array_equal(host(fresh.links.pairs), host(st.links.pairs))
            for name in ("center", "quat", "length"):
                assert_bits_equal(host(getattr(fresh, name)), host(getattr(st, name)), name)
            assert np.array_equal(host(fresh.ids), host(st.ids))
            checked += 1
            if checked == 2:
                break
        seen_births += s.num_born
    assert checked == 2


def _match_by_position(ca, cb):
    d = ((ca[:, None, :] - cb[None, :, :]) ** 2).sum(axis=2)
    m = d.argmin(axis=1)
    assert len(set(m.tolist())) == len(m), "position matching is not one to one"
    return m


def test_runs_are_deterministic_and_reordering_changes_nothing_but_numbering():
    from gpu_util import assert_bits_equal, host
    b = _colony(31, 400)
    runs = []
    for reorder in (False, False, True):
        st = _stepper(b)
        counts = []
        for k in range(30):
            if reorder and k % 10 == 0:
                st.reorder_bodies()
            counts.append(st.step().num_bodies)
        runs.append((counts, host(st.center), host(st.length), host(st.ids), host(st.quat)))
    (c0, x0, l0, i0, q0), (c1, x1, l1, i1, q1), (c2, x2, l2, i2, q2) = runs
    assert c0 == c1
    assert_bits_equal(x0, x1, "center")
    assert_bits_equal(q0, q1, "quat")
    assert_bits_equal(l0, l1, "length")
    assert np.array_equal(i0, i1)
    assert c2 == c0 and len(x2) == len(x0) and c0[-1] > c0[0]
    # bodies present from the start keep their ids; children are numbered in birth (index) order, which a
    # reorder changes, so bodies are matched by position
    n0 = 400
    pos0 = {int(i): k for k, i in enumerate(i0)}
    for k, i in enumerate(i2):
        if i < n0:
            a = pos0[int(i)]
            assert np.all(np.abs(x2[k] - x0[a]) <= 1e-12 * np.abs(x0[a]).max())
    m = _match_by_position(x2, x0)
    assert np.all(np.abs(x2 - x0[m]) <= 1e-12 * np.abs(x0).max())
    assert np.array_equal(l2, l0[m])


def _cpp_against_python(tmp_path, b, box, steps, viscosity=1.0, rate=5.0):
    """runs bacteria_step_app and the Python stepper on the same rods: per step the body count, births, contacts, the
    largest overlap and the rebuild flag must agree, and the final checksums of the live rows.  Returns the Python
    stepper and the total births."""
    from cpp_apps import build_app, fnv1a_bits as _checksum
    from gpu_util import dev, host
    from mundy_amd import synth
    n = len(b["radius"])
    mt, mr = synth.dry_mobility(b["radius"], viscosity=viscosity)
    inp = tmp_path / "rods.bin"
    with open(inp, "wb") as f:
        f.write(np.uint64(n).tobytes())
        for a in (b["center"], b["quat"], b["radius"], b["length"], mt, mr):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
    exe = build_app("bacteria_step_app")
    dt, E, nu, D, buf = 1e-3, 1000.0, 0.3, 2.0, 0.5
    p = subprocess.run([exe, str(inp), str(steps), "0", repr(box or 0.0), repr(dt), repr(E), repr(nu), repr(rate),
                        repr(D), repr(buf)], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:], p.stderr[-2000:])
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("STEP")]
    assert len(lines) == steps
    st = _stepper(b, box=(box, box, box) if box else None, dt=dt, viscosity=viscosity, growth_rate=rate,
                  division_length=D, search_buffer=buf, youngs_modulus=E, poisson_ratio=nu, mob_trans=dev(mt),
                  mob_rot=dev(mr))
    born = 0
    for k in range(steps):
        s = st.step()
        born += s.num_born
        ln = lines[k]
        assert int(ln[3]) == s.num_bodies and int(ln[5]) == s.num_born and int(ln[7]) == s.num_contacts, k
        assert float(ln[9]) == s.max_overlap and int(ln[11]) == int(s.rebuilt), k
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("CHECKSUM")][0].split()
    assert line[2] == _checksum(host(st.center)) and line[4] == _checksum(host(st.quat))
    assert line[6] == _checksum(host(st.length))
    return st, born


def test_cpp_growth_stepper_reproduces_the_python_driver(tmp_path):
    b = _colony(41, 3000)
    st, born = _cpp_against_python(tmp_path, b, float(b["box"]), 20)
    assert born > 0


def test_cpp_growth_stepper_follows_a_colony_well_past_its_first_capacity(tmp_path):
    # 8 well separated rods grow into lines of several generations: the C++ stepper's buffers (n + n/8 + 16 rows at
    # first) are regrown several times, in steps that have births
    from mundy_amd import synth
    n0 = 8
    b = synth.spherocylinders(n0, radius=0.5, seed=71)
    g = np.stack(np.meshgrid([0.0, 25.0], [0.0, 25.0], [0.0, 25.0], indexing="ij"), axis=-1).reshape(n0, 3)
    b["center"] = np.ascontiguousarray(g)
    b["length"] = 0.5 + 1.5 * (1.0 - synth.uniform01(71, np.arange(n0), 9))
    # mobility 2 at dt = 1e-3: contacts relax faster than the rods grow (no interpenetration along the lines)
    st, born = _cpp_against_python(tmp_path, b, None, 1000, viscosity=1.0 / (6.0 * np.pi * 0.5 * 2.0))
    assert st.n == n0 + born and st.n >= 6 * n0, st.n


def test_one_step_at_a_million_rods():
    from gpu_util import host
    n = 1_000_000
    b = _colony(51, n)
    dt, rate = 1e-3, 0.1  # Bacteria.cpp's defaults: tens of births per step at this size
    st = _stepper(b, dt=dt, growth_rate=rate)
    s0 = st.step()        # lengths in (cl_min, D]: nobody divides before growing once
    assert s0.num_born == 0 and s0.rebuilt
    predicted = int(((b["length"] + dt * rate) > 2.0).sum())
    s = st.step()
    assert s.num_born == predicted and predicted > 0
    assert st.n == n + predicted and s.rebuilt and s.num_contacts > 0
    assert np.isfinite(host(st.center)).all()
