"""The device's RPYC mobility against the published closed form and its properties (tests/potentials.py: rpyc_tt).

The hydrodynamics' parity tests hold the kernel to hydro_model.py, a transcription of the same text.  Here the 144 x 144
matrix of the 48-bead cloud of tests/gradient_cases.py (1604 far, 622 overlapping, 30 nested ordered pairs) is built on
the device column by column, from unit forces, once per path of HydroWorkspace.set_path, and held to what needs no
transcription: every off-diagonal block is rpyc_tt to K eps |block| (K from tests/test_potentials_host.py), the matrix
is symmetric, with the self term it is positive definite with mpmath's smallest eigenvalue, and it is continuous across
both branch boundaries.  "rpy" goes through the reference's one-step fast inverse square root and is approximate by
design: it is only held to the far branch within 5 delta at r >= 3 (a + b), delta that root's worst relative error
(measured on the host, tests/test_potentials_host.py)."""
import math

import mpmath as mp
import numpy as np
import pytest

import gradient_cases as gc
import potentials as P
from gpu_util import dev, host

pytestmark = pytest.mark.gpu
EPS = gc.EPS
MU = gc.VISCOSITY
PATHS = ("auto", "in_lane", "partial")


def device_matrix(kind, center, radius, path="auto"):
    """column 3 s + j = the velocities of all beads under the unit force e_j on bead s -> [3 n, 3 n]"""
    from mundy_amd import ops
    n = len(radius)
    ws = ops.HydroWorkspace()
    ws.set_path(path)
    c, a = dev(center), dev(radius)
    M = np.empty((3 * n, 3 * n))
    f = np.zeros((n, 3))
    for s in range(n):
        for j in range(3):
            f[s, j] = 1.0
            M[:, 3 * s + j] = host(ops.hydro_velocity(kind, MU, c, a, dev(f), workspace=ws)).reshape(-1)
            f[s, j] = 0.0
    if path != "auto":
        assert ws.last_path() == path
    ws.close()
    return M


_MATRIX = {}


@pytest.fixture(params=PATHS)
def matrix(request):
    if request.param not in _MATRIX:
        c, a, _ = gc.mobility_cloud()
        _MATRIX[request.param] = device_matrix("rpyc", c, a, request.param)
    return _MATRIX[request.param]


def blocks(M, n):
    return M.reshape(n, 3, n, 3).transpose(0, 2, 1, 3)   # [t, s, i, j]


def test_every_branch_is_populated():
    _, _, branch = gc.mobility_cloud()
    counts = {k: int((branch == k).sum()) for k in "fon"}
    print(counts)
    assert min(counts.values()) >= 20


def test_blocks_are_the_closed_form(matrix):
    ref, _ = gc.rpyc_blocks()
    _, a, branch = gc.mobility_cloud()
    n = len(a)
    B, R = blocks(matrix, n), blocks(ref, n)
    K = gc.TOLERANCE_K["rpyc"]
    off = ~np.eye(n, dtype=bool)
    err = np.abs(B - R).max(axis=(2, 3))
    scale = np.sqrt((R * R).sum(axis=(2, 3)))
    for k, what in (("f", "far"), ("o", "overlapping"), ("n", "nested")):
        sel = branch == k
        print("%-12s worst |block - rpyc_tt| = %.3g eps |block| (K = %g)" % (what, (err[sel] / (EPS * scale[sel])).max(), K))
    assert (err[off] <= K * EPS * scale[off]).all()
    # no self term: the diagonal blocks are exactly zero
    assert (B[np.arange(n), np.arange(n)] == 0.0).all()


def test_matrix_is_symmetric_positive_definite(matrix):
    ref, Mmp = gc.rpyc_blocks()
    _, a, _ = gc.mobility_cloud()
    n = len(a)
    asym = np.abs(matrix - matrix.T)
    print("largest |M - M^T| / |M| = %.3g" % (asym / np.maximum(np.abs(matrix), 1e-300)).max())
    # (the exchange d -> -d and a <-> b may change a bit: the per-term allowance of tests/test_gpu_hydro.py's symmetry test)
    assert (asym <= 4.0 * 2.0 ** -53 * np.abs(matrix)).all()
    full = matrix + np.diag(np.repeat(1.0 / (6.0 * math.pi * MU * a), 3))
    np.linalg.cholesky(full)   # raises LinAlgError unless positive definite
    lam = np.linalg.eigvalsh(0.5 * (full + full.T))[0]
    # mpmath's smallest eigenvalue: the Rayleigh quotient, at 50 digits, of the float64 eigenvector of the rounded matrix
    # (its error is second order in the eigenvector's)
    w, V = np.linalg.eigh(ref)
    with P.hp():
        v = [mp.mpf(float(t)) for t in V[:, 0]]
        Mv = [sum(Mmp[i][j] * v[j] for j in range(3 * n)) for i in range(3 * n)]
        exact = float(sum(v[i] * Mv[i] for i in range(3 * n)) / sum(t * t for t in v))
    print("smallest eigenvalue: device %.15g, mpmath %.15g" % (lam, exact))
    assert exact > 1e-3 and abs(lam - exact) <= 1e-10 * exact


RADIUS_PAIRS = ((1.0, 1.0), (0.8, 0.2), (0.5, 0.9), (1.2, 0.3), (0.4, 1.1))   # a = b and a = 4 b among them


@pytest.mark.parametrize("a,b", RADIUS_PAIRS)
def test_mobility_is_continuous_across_its_branch_boundaries(a, b):
    """one source of radius a, targets of radius b at r = (a + b)(1 -+ 1e-9) and r = |a - b|(1 -+ 1e-9): the two sides
    differ by at most 1e-7 |block| (the published form is C^1 across r = a + b: the jump is O(1e-9); a coefficient in
    error in either branch gives O(1))"""
    from mundy_amd import ops
    u = np.array([2.0, -3.0, 6.0]) / 7.0
    src = gc.SHIFT[None].copy()
    radii = [(a + b) * (1.0 - 1e-9), (a + b) * (1.0 + 1e-9)]
    if a != b:
        radii += [abs(a - b) * (1.0 - 1e-9), abs(a - b) * (1.0 + 1e-9)]
    tgt = src + np.array(radii)[:, None] * u
    r = np.linalg.norm(tgt - src, axis=1)
    assert r[0] < a + b < r[1] and (a == b or r[2] < abs(a - b) < r[3])
    blk = np.empty((len(radii), 3, 3))
    for j in range(3):
        blk[:, :, j] = host(ops.hydro_velocity("rpyc", MU, dev(src), dev(np.array([a])), dev(np.eye(3)[j][None]),
                                               tgt_center=dev(tgt), tgt_radius=dev(np.full(len(radii), b))))
    for k in range(0, len(radii), 2):
        jump = np.linalg.norm(blk[k + 1] - blk[k]) / np.linalg.norm(blk[k])
        print("a = %g, b = %g, r = %.3g: jump %.3g |block|" % (a, b, radii[k], jump))
        assert np.linalg.norm(blk[k]) > 0.0 and jump <= 1e-7


def test_rpy_approaches_the_far_branch():
    c, a = gc.far_cloud()
    n = len(a)
    B = blocks(device_matrix("rpy", c, a), n)
    delta = gc.FAST_RSQRT_DELTA
    worst = 0.0
    with P.hp():
        for t in range(n):
            for s in range(n):
                if s == t:
                    continue
                d = [mp.mpf(float(c[t][k])) - mp.mpf(float(c[s][k])) for k in range(3)]
                assert P.rpyc_branch(P.norm(d), a[s], a[t]) == "far" and P.norm(d) >= 3 * (a[s] + a[t])
                ref = P.rpyc_tt(d, a[s], a[t], MU)
                ref = np.array([[float(ref[i, j]) for j in range(3)] for i in range(3)])
                worst = max(worst, np.linalg.norm(B[t, s] - ref) / np.linalg.norm(ref))
    print("rpy against the far branch: worst %.3g |block| (5 delta = %.3g)" % (worst, 5.0 * delta))
    assert 0.0 < worst <= 5.0 * delta
