"""The small entry points the rebalance, ghost and dense paths are built from, through the C ABI (or the thin `ops`
wrapper), each against a numpy / math.fsum statement of the same operation, bit for bit: the 64-bit radix sort, key
composition, curve keys and orders, work weights, sequences, strided copies, row gathers, contact selection, the
double-double gemv rows and the AABB bounds.  Sizes cover the wave (64), workgroup (256) and sort-tile (1024) edges."""
import ctypes as C
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097, 200_003]


@pytest.fixture(scope="module")
def ops():
    from mundy_amd import ops as o
    return o


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _lib():
    from mundy_amd import capi
    return capi.load()


def _check(status):
    from mundy_amd import capi
    capi.check(status)


def _stream():
    from mundy_amd import ops
    return ops._stream()


def _u64(keys):
    """uint64 keys as the int64 tensor the library reads (same bits)"""
    from gpu_util import dev
    return dev(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))


def _stable(keys):
    return np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable")


def _lattice(f, maxc):
    """the library's lattice coordinate of a floored position (mundy_hip.h): clamped in double first, NaN -> 0"""
    with np.errstate(invalid="ignore"):
        return np.where(~(f > 0.0), 0.0, np.minimum(f, float(maxc))).astype(np.int64)


def _curve_keys_ref(c, lo, hi, level, table):
    """table[clip(floor((c - lo) / span * 2^level), 0, 2^level - 1)] in that order of evaluation"""
    span = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor((c - np.asarray(lo, dtype=np.float64)) / span * float(1 << level))
    cell = _lattice(f, (1 << level) - 1)
    return table[cell[:, 0], cell[:, 1], cell[:, 2]]


# ---- mhip_sort_by_key_u64 -------------------------------------------------------------------------------------------
def _key_families(rng, n):
    yield "uniform", rng.integers(0, 1 << 64, n, dtype=np.uint64)          # the top bit is set in half of them
    yield "equal", np.full(n, 0x8000_0000_dead_beef, dtype=np.uint64)
    step = np.uint64(((1 << 64) - 1) // max(n, 1))                          # strictly descending over all 64 bits
    yield "descending", np.uint64((1 << 64) - 1) - np.arange(n, dtype=np.uint64) * step
    few = np.array([0, 1, 1 << 63, (1 << 64) - 1, 0x00ff_0000_0000_ff00], dtype=np.uint64)
    yield "few distinct", few[rng.integers(0, len(few), n)]
    base = int(rng.integers(0, 1 << 64, dtype=np.uint64))
    for b in range(8):                                                       # every radix pass on its own
        digit = rng.integers(0, 256, n, dtype=np.uint64)
        keys = (np.uint64(base) & ~np.uint64(0xff << (8 * b))) | (digit << np.uint64(8 * b))
        yield "byte %d" % b, keys


def _check_sort(ops, keys, what):
    from gpu_util import host
    import torch
    dk = _u64(keys)
    before = dk.clone()
    perm = host(ops.sort_by_key(dk)).astype(np.int64)
    assert torch.equal(dk, before), "%s: the keys were modified" % what
    ref = _stable(keys)
    bad = np.nonzero(perm != ref)[0]
    assert bad.size == 0, "%s (n = %d): %d positions differ, first at %d" % (what, len(keys), bad.size, bad[0])


@pytest.mark.parametrize("n", SIZES)
def test_sort_by_key_u64_is_the_stable_unsigned_argsort(ops, n):
    rng = np.random.default_rng(n)
    for what, keys in _key_families(rng, n):
        _check_sort(ops, keys, what)


def test_sort_by_key_u64_on_composed_curve_keys(ops):
    # the keys the rebalances sort: level-8 Hilbert key << 40 | entity id (all 64 bits in use, negative as int64)
    from mundy_amd import distributed as D
    rng = np.random.default_rng(8)
    table = D.hilbert_key_table(8)
    for n in (1025, 4097, 200_003):
        cells = rng.integers(0, 256, (n, 3))
        cells[: n // 4] = cells[0]                                          # one crowded cell: ties on the major key
        ids = rng.integers(0, 1 << 40, n, dtype=np.uint64)
        ids[-3:] = [(1 << 40) - 1, (1 << 40) - 2, 0]
        keys = (table[cells[:, 0], cells[:, 1], cells[:, 2]].astype(np.uint64) << np.uint64(40)) | ids
        assert (keys >= np.uint64(1 << 63)).any()
        _check_sort(ops, keys, "composed curve keys")


def test_sort_by_key_u64_empty_and_scratch_reuse(ops):
    # n = 0 succeeds without touching perm; the thread_local scratch grows and is reused, never shrunk
    import torch
    e = torch.empty(0, dtype=torch.int64, device="cuda")
    assert ops.sort_by_key(e).shape == (0,)
    _check(_lib().mhip_sort_by_key_u64(0, None, None, _stream()))
    rng = np.random.default_rng(11)
    for n in (300_007, 65, 1025, 300_007, 2):
        _check_sort(ops, rng.integers(0, 1 << 64, n, dtype=np.uint64), "scratch reuse")


# ---- mhip_compose_keys_u64 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1, 24, 40])
def test_compose_keys_u64(shift):
    from gpu_util import dev, host
    import torch
    rng = np.random.default_rng(shift)
    major_max = min((1 << 32) - 1, (1 << (64 - shift)) - 1)
    for n in SIZES:
        major = rng.integers(0, major_max + 1, n, dtype=np.uint64)
        minor = rng.integers(0, 1 << shift, n, dtype=np.uint64)
        major[0], minor[0] = major_max, (1 << shift) - 1                     # the largest of both
        if n > 1:
            major[1], minor[1] = 0, 0
        out = torch.empty(n, dtype=torch.int64, device="cuda")
        dmaj = dev(major.astype(np.uint32).view(np.int32))
        dmin = dev(minor.astype(np.float64))
        _check(_lib().mhip_compose_keys_u64(n, _p(dmaj), _p(dmin), shift, _p(out), _stream()))
        ref = (major << np.uint64(shift)) | minor
        assert np.array_equal(host(out).view(np.uint64), ref), (shift, n)
    with pytest.raises(ValueError, match="shift"):
        _check(_lib().mhip_compose_keys_u64(1, _p(dmaj), _p(dmin), 41, _p(out), _stream()))


# ---- mhip_curve_keys / mhip_curve_order / mhip_morton_order on the whole real line ----------------------------------
def _hard_centres(rng, n, lo, hi, level):
    lo, hi = np.asarray(lo), np.asarray(hi)
    c = rng.uniform(lo, hi, (n, 3))
    k = min(n, 4096)
    kind = rng.integers(0, 8, k)
    faces = lo + (hi - lo) * rng.integers(0, (1 << level) + 1, (k, 3)) / float(1 << level)   # on cell faces
    out = rng.choice([-1.0, 1.0], (k, 3)) * 10.0 ** rng.uniform(0, 300, (k, 3))             # up to 1e300 outside
    special = np.array([np.nan, np.inf, -np.inf, lo[0], hi[0], -0.0, 0.0])
    pick = [faces, lo + out, hi + out, np.broadcast_to(lo, (k, 3)), np.broadcast_to(hi, (k, 3)),
            special[rng.integers(0, len(special), (k, 3))], faces, c[:k]]
    for j in range(8):
        sel = kind == j
        c[:k][sel] = pick[j][sel]
    # single coordinates off: one axis NaN / inf and the others ordinary
    m = min(n, 64)
    c[:m, rng.integers(0, 3)] = rng.choice([np.nan, np.inf, -np.inf, 1e300, -1e300], m)
    rng.shuffle(c)
    return c


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5, 6, 7, 8])
def test_curve_keys_and_order_match_the_numpy_statement(ops, level):
    from gpu_util import dev, host
    from mundy_amd import distributed as D
    rng = np.random.default_rng(100 + level)
    lo, hi = np.array([-3.0, 0.5, 2.0]), np.array([40.0, 61.5, 33.0])
    table = D.hilbert_key_table(level)
    dtab = dev(table.astype(np.int32))
    for n in (1, 63, 65, 1025, 4097, 200_003):
        c = _hard_centres(rng, n, lo, hi, level)
        ref = _curve_keys_ref(c, lo, hi, level, table)
        keys = host(ops.curve_keys(dev(c), lo, hi, level, dtab)).astype(np.int64)
        bad = np.nonzero(keys != ref)[0]
        assert bad.size == 0, (level, n, bad.size, c[bad[:3]], keys[bad[:3]], ref[bad[:3]])
        if n > 512 * 8 ** level:     # ties are ordered per cell by one thread (insertion sort): keep cells small
            continue
        perm = host(ops.curve_order(dev(c), lo, hi, level, dtab)).astype(np.int64)
        assert np.array_equal(perm, np.argsort(ref, kind="stable")), (level, n)


def test_morton_order_on_out_of_range_infinite_and_nan_centres(ops):
    from gpu_util import dev, host
    from test_gpu_reorder_integrate import _morton_key
    rng = np.random.default_rng(21)
    lo = np.array([1.0, -2.0, 0.5])
    for n, cell in ((65, 7.0), (4097, 1.7), (200_003, 0.9)):
        bits = 4                                   # the lattice resolution rule of mhip_morton_order (mundy_hip.h)
        while bits < 8 and (1 << (3 * (bits + 1))) <= 8 * n:
            bits += 1
        hi = lo + cell * (1 << bits)
        c = _hard_centres(rng, n, lo, hi, bits)
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.floor((c - lo) * (1.0 / cell))
        key = _morton_key(_lattice(f, (1 << bits) - 1))
        perm = host(ops.morton_order(dev(c), lo, cell)).astype(np.int64)
        ref = np.argsort(key.astype(np.uint64), kind="stable")
        assert np.array_equal(perm, ref), (n, int((perm != ref).sum()))


# ---- mhip_body_work_weights -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [0, 1, 63, 64, 65, 100_000])
def test_body_work_weights_is_one_plus_the_pair_count(c):
    from gpu_util import dev, host
    import torch
    rng = np.random.default_rng(c)
    for first, count in ((0, 1), (0, 257), (1000, 1025), (5, 4097)):
        pairs = rng.integers(0, first + count + 600, (c, 2)).astype(np.int32)  # below first, inside, past the end
        if c:
            pairs[0] = [max(first - 1, 0), first + count]
        w = torch.full((count,), -7.0, dtype=torch.float64, device="cuda")
        dp = dev(pairs) if c else torch.empty((0, 2), dtype=torch.int32, device="cuda")
        _check(_lib().mhip_body_work_weights(c, _p(dp), first, count, _p(w), _stream()))
        ref = 1.0 + np.bincount(pairs.ravel(), minlength=first + count + 600)[first:first + count]
        assert np.array_equal(host(w), ref), (c, first, count)


# ---- mhip_fill_sequence, mhip_copy_strided, mhip_gather_rows --------------------------------------------------------
def test_fill_sequence():
    from gpu_util import assert_bits_equal, host
    import torch
    for n in SIZES:
        for first in (0.0, float(1 << 31), float((1 << 53) - n)):
            out = torch.full((n,), np.nan, dtype=torch.float64, device="cuda")
            _check(_lib().mhip_fill_sequence(n, first, _p(out), _stream()))
            assert_bits_equal(host(out), first + np.arange(n, dtype=np.float64), "fill_sequence %d from %r" % (n, first))


def test_copy_strided():
    from gpu_util import assert_bits_equal, dev, host
    rng = np.random.default_rng(4)
    for n in (1, 64, 65, 1025, 4097):
        for width in range(1, 17):
            ss, ds = width + int(rng.integers(1, 5)), width + int(rng.integers(1, 5))
            src = rng.normal(size=(n, ss))
            dst0 = rng.normal(size=(n, ds))
            dsrc, ddst = dev(src), dev(dst0)
            _check(_lib().mhip_copy_strided(n, width, _p(dsrc), ss, _p(ddst), ds, _stream()))
            ref = dst0.copy()
            ref[:, :width] = src[:, :width]
            assert_bits_equal(host(ddst), ref, "copy_strided n=%d width=%d strides %d/%d" % (n, width, ss, ds))
    # the offset columns the rebalance unpacks (record column 12 of 13 into a packed vector)
    rec = rng.normal(size=(257, 13))
    drec, out = dev(rec), dev(np.zeros(257))
    _check(_lib().mhip_copy_strided(257, 1, C.c_void_p(drec.data_ptr() + 12 * 8), 13, _p(out), 1, _stream()))
    assert_bits_equal(host(out), rec[:, 12], "copy_strided column 12")


def test_gather_rows_repeated_and_reversed(ops):
    from gpu_util import assert_bits_equal, dev, host
    rng = np.random.default_rng(6)
    for n in (1, 63, 65, 1025, 4097):
        src_n = max(n // 3, 1)
        perms = {"reversed": np.arange(src_n)[::-1], "repeated": rng.integers(0, src_n, n),
                 "one row": np.full(n, src_n - 1)}
        for width in range(1, 17):
            src = rng.normal(size=(src_n, width))
            src.ravel()[::7] = -0.0
            for what, perm in perms.items():
                perm = np.ascontiguousarray(perm, dtype=np.int32)
                assert_bits_equal(host(ops.gather_rows(dev(perm), dev(src))), src[perm],
                                  "gather_rows %s n=%d width=%d" % (what, n, width))


# ---- mhip_select_contacts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [-np.inf, 0.0, np.inf, 0.25])
def test_select_contacts_keeps_not_above_cutoff(ops, cutoff):
    from gpu_util import dev, host
    rng = np.random.default_rng(7)
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 0.25, -0.25, np.nextafter(0.25, 1), 1e-300, -1e-300])
    for n in SIZES:
        sep = rng.normal(scale=0.5, size=n)
        sel = rng.random(n) < 0.3
        sep[sel] = special[rng.integers(0, len(special), int(sel.sum()))]
        sep[rng.random(n) < 0.1] = cutoff                                    # sep == cutoff is kept
        kept = host(ops.select_contacts(dev(sep), cutoff)).astype(np.int64)
        with np.errstate(invalid="ignore"):
            ref = np.nonzero(~(sep > cutoff))[0]
        assert np.array_equal(kept, ref), (cutoff, n, kept.size, ref.size)


# ---- mhip_gemv: the double-double row sum, rounded once -------------------------------------------------------------
def _conditioned_system(rng, n, max_log2_cond=40):
    """A, x whose row sums cancel: every row carries pairs of large terms of opposite sign on top of O(1) terms, sized
    for a condition number sum|terms| / |sum| spread up to 2^max_log2_cond (and kept at or below it)"""
    x = rng.uniform(0.5, 2.0, n) * rng.choice([-1.0, 1.0], n)
    A = rng.normal(size=(n, n))
    if n < 3:
        return A, x
    npairs = max(1, min(8, n // 3))
    for i in range(n):
        e = rng.uniform(0, max_log2_cond)
        big = 2.0 ** e * math.sqrt(n) / (2 * npairs)
        cols = rng.choice(n, 2 * npairs, replace=False)
        for a, b in zip(cols[::2], cols[1::2]):
            m = big * rng.uniform(0.5, 1.0)
            A[i, a] = m / x[a]
            A[i, b] = -m / x[b]                                   # cancels A[i, a] x[a] up to the roundings
        while True:
            t = A[i] * x
            s = math.fsum(t)
            if s != 0.0 and np.abs(t).sum() <= 2.0 ** max_log2_cond * abs(s):
                break
            A[i, cols] *= 0.5
    return A, x


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 1000])
def test_gemv_rows_are_the_correctly_rounded_sum(ops, n):
    # device build -ffp-contract=off: the products are numpy's; the double-double accumulator rounds once, correctly
    # while sum|terms| / |sum| <= 2^40, so every row equals math.fsum of its products
    from gpu_util import assert_bits_equal, dev, host
    rng = np.random.default_rng(1000 + n)
    A, x = _conditioned_system(rng, n)
    t = A * x
    cond = np.abs(t).sum(axis=1) / np.abs([math.fsum(r) for r in t])
    assert cond.max() <= 2.0 ** 40 and (n < 3 or cond.max() >= 2.0 ** 30), cond.max()
    ref = np.array([math.fsum(r) for r in t])
    y = host(ops.gemv(dev(A), dev(x)))
    assert_bits_equal(y, ref, "gemv n=%d" % n)
    # the same sums in another column order: the same bits
    p = rng.permutation(n)
    assert_bits_equal(host(ops.gemv(dev(np.ascontiguousarray(A[:, p])), dev(x[p]))), y, "gemv n=%d, permuted" % n)


# ---- mhip_aabb_bounds -----------------------------------------------------------------------------------------------
def test_aabb_bounds():
    from gpu_util import dev
    rng = np.random.default_rng(9)
    for n in SIZES:
        c = rng.uniform(-1e3, 1e3, (n, 3))
        h = rng.uniform(0.0, 5.0, (n, 3))
        aabb = np.concatenate([c - h, c + h], axis=1)
        for buffer in (0.0, 0.1, 3.7):
            out = (C.c_double * 6)()
            _check(_lib().mhip_aabb_bounds(n, _p(dev(aabb)), buffer, out, _stream()))
            ref = np.concatenate([(aabb[:, :3] - buffer).min(axis=0), (aabb[:, 3:] + buffer).max(axis=0)])
            assert np.array_equal(np.array(out[:]).view(np.uint64), ref.view(np.uint64)), (n, buffer)
    out = (C.c_double * 6)(*([0.0] * 6))
    _check(_lib().mhip_aabb_bounds(0, None, 0.5, out, _stream()))       # the empty set: the inverted box
    big = np.finfo(np.float64).max
    assert list(out) == [big, big, big, -big, -big, -big]


# ---- entity ids at the top of their range survive a rebalance in (cell, id) order -----------------------------------
def test_rebalance_orders_ids_near_the_bound(ops):
    from gpu_util import dev, host
    from mundy_amd import distributed as D, synth
    b = synth.spherocylinders(3000, seed=5)
    rng = np.random.default_rng(12)
    ids = ((1 << 40) - 1 - rng.permutation(3000)).astype(np.float64)       # 2^40 - 3000 .. 2^40 - 1, shuffled
    st = D.DistributedContactStepper(dev(b["center"]), dev(b["quat"]), dev(b["radius"]), dev(b["length"]), 0,
                                     entity_id=dev(ids), domain=(0.0, float(b["box"])), curve_level=5)
    st.rebalance()
    e = host(st.entity_id)
    assert np.array_equal(np.sort(e), np.sort(ids))                         # every id kept, none rounded
    cells = _curve_keys_ref(host(st.center), [0.0] * 3, [float(b["box"])] * 3, 5, D.hilbert_key_table(5))
    order = np.lexsort((e, cells))
    assert np.array_equal(order, np.arange(3000)), "owned set not in (cell, entity id) order"
    with pytest.raises(ValueError, match=r"\[0, 2\^40\)"):
        D.DistributedContactStepper(dev(b["center"]), dev(b["quat"]), dev(b["radius"]), dev(b["length"]), 0,
                                    entity_id=dev(ids + 3000.0), domain=(0.0, float(b["box"])))
