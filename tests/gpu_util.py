import numpy as np
import torch


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.detach().cpu().numpy()


def random_rods(rng, n, box, rmin=0.3, rmax=0.6, lmin=0.5, lmax=2.5):
    c = rng.uniform(0, box, (n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return c, q, rng.uniform(rmin, rmax, n), rng.uniform(lmin, lmax, n)


def assert_bits_equal(a, b, what=""):
    """bit-for-bit equality of float64 arrays (NaN == NaN when the payloads match)"""
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = a.view(np.uint64) != b.view(np.uint64)
    # +0.0 vs -0.0 would show up here too, deliberately
    assert not bad.any(), "%s: %d of %d elements differ; max |diff| = %g" % (
        what, int(bad.sum()), a.size, float(np.nanmax(np.abs(a - b)[bad])) if bad.any() else 0.0)


# ---- inputs for the helpers the force kernels share (statistic epilogues, incidence build) ---------------------------
PAST_FULL_GRID = 2048 * 256 + 3   # one item more than a full grid of kMaxGrid workgroups: the grid-stride loop's second pass
# first and last lane of a wave, a wave boundary, a workgroup boundary, the second pass
STAT_POSITIONS = (0, 63, 64, 255, 256, PAST_FULL_GRID - 1)


def line_with_one_long_bond(pos, n=PAST_FULL_GRID):
    """n bodies on the x axis joined in a line by bonds of length 1, the one whose FIRST end is body pos of length 1.5
    (all coordinates and lengths exact) -> (center [n, 3], pairs int32 [n - 1, 2]).  Bond s is (s, s + 1), but the last
    one is listed as (n - 1, n - 2): body n - 1 is a first end too, and only body n - 2 is none."""
    assert pos != n - 2
    length = np.ones(n - 1)
    length[min(pos, n - 2)] = 1.5
    c = np.zeros((n, 3))
    c[1:, 0] = np.cumsum(length)
    pairs = np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)
    pairs[n - 2] = (n - 1, n - 2)
    return c, pairs


def star_graph(spokes=100, isolated=20):
    """body 0 joined to bodies 1 .. spokes (a list far longer than the per-body insertion sort usually sees), then
    `isolated` bodies nothing touches -> (n, pairs int32 [spokes, 2])"""
    pairs = np.stack([np.zeros(spokes, np.int64), np.arange(1, spokes + 1)], axis=1).astype(np.int32)
    pairs[1::2] = pairs[1::2, ::-1]   # the hub is the first end of every other spoke only
    return 1 + spokes + isolated, pairs


def star_and_random_graph(rng, bodies=3000, edges=6000):
    """the star followed by a random graph on `bodies` further bodies -> (n, pairs int32 [m, 2])"""
    n0, star = star_graph()
    g = rng.integers(0, bodies, (edges, 2))
    g = g[g[:, 0] != g[:, 1]] + n0
    return n0 + bodies, np.concatenate([star, g]).astype(np.int32)


def renumberings(rng, n):
    """new_of_old int32 [n]: the reversal and a random permutation"""
    return {"reversed": np.arange(n - 1, -1, -1).astype(np.int32), "random": rng.permutation(n).astype(np.int32)}


def all_pos_zero(a):
    """every element exactly +0.0"""
    return not np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).any()
