"""The inputs on which the semiflexible-chain laws are held to the gradients of their potentials, for
tests/test_bending_host.py (the numpy model, where the tolerances are measured) and tests/test_gpu_bending.py (the
device, held to them).  numpy and mpmath only: nothing here touches the device.

Every case is a chain of beads laid out as a random walk with prescribed bond lengths, in its own frame and in a rotated
and translated one.  TOLERANCE_K: a body's deviation from -grad U (central differences in mpmath at 50 digits,
tests/potentials.py) in units of eps S_b, S_b the sum of the magnitudes of the terms that act on body b; four times the
worst deviation of the numpy model (tests/bending_model.py), rounded up to a power of two -- measured from the model
and the exact gradient by tests/test_bending_host.py::test_calibration, never from the device:

    group                    worst deviation [eps S_b]      K
    fenewca                         15.1                   64
    fenewca near the clamp        1068                   8192
    angular                          2.68                  16

"fenewca near the clamp" are bonds within 2e-3 of r_max - 1e-4 and past it: 1 - (L_adj / r_max)^2 is then a difference
of two numbers that agree to three or four digits, and the rounding of L_adj / r_max alone costs a thousand eps and more
of the force.  That is
the law as the reference writes it, not a defect of its evaluation."""
import math

import numpy as np

import bending_model as bm
import gradient_cases as gc
import potentials as P

EPS = gc.EPS
TOLERANCE_K = {"fenewca": 64.0, "fenewca near the clamp": 8192.0, "angular": 16.0}
R_MAX = 1.5
CUTOFF = bm.wca_cutoff(1.0)


def _walk(rng, lengths):
    """len(lengths) + 1 beads: a random walk whose steps have the given lengths (to rounding)"""
    steps = rng.normal(size=(len(lengths), 3))
    steps *= (np.asarray(lengths) / np.linalg.norm(steps, axis=1))[:, None]
    return np.concatenate([np.zeros((1, 3)), np.cumsum(steps, axis=0)])


def _chain_pairs(n):
    return np.stack([np.arange(n - 1), np.arange(1, n)], axis=1).astype(np.int32)


class Case:
    """kind "fenewca": pairs, k [m], r_max, wca = (epsilon, sigma); kind "angular": triplets, k [m], rest_angle [m]"""

    def __init__(self, group, kind, x, **kw):
        self.group, self.kind, self.x = group, kind, np.ascontiguousarray(x)
        self.__dict__.update(kw)
        self.n = self.x.shape[0]

    def cos_rest(self):
        """what std::cos gives on this machine's libm; the device tests take the handle's own"""
        return np.array([math.cos(a) for a in self.rest_angle])

    def model(self, x=None, cos_rest=None):
        x = self.x if x is None else x
        if self.kind == "fenewca":
            return bm.fenewca_force(self.n, self.pairs, self.k, self.r_max, x, *self.wca)[0]
        return bm.angular_force(self.n, self.triplets, self.k, self.cos_rest() if cos_rest is None else cos_rest, x)[0]

    def terms(self, cos_rest=None):
        if self.kind == "fenewca":
            return [bm.fenewca_term(i, j, k, self.r_max, *self.wca) for (i, j), k in zip(self.pairs, self.k)]
        cr = self.cos_rest() if cos_rest is None else cos_rest
        return [bm.angular_term(a, b, c, k, c0) for (a, b, c), k, c0 in zip(self.triplets, self.k, cr)]

    def moved(self):
        """the case's positions rotated and translated (float64: the new input, not an exact image)"""
        rng = np.random.default_rng(77)
        q = gc.random_quat(rng)
        w, a, b, c = q
        R = np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                      [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                      [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]])
        return np.ascontiguousarray(self.x @ R.T + np.array([3.25, -1.5, 0.75]))

    def check(self):
        """the conditions the case was built for"""
        assert self.n >= 24
        if self.kind == "fenewca":
            p = np.asarray(self.pairs)
            for x in (self.x, self.moved()):
                L = np.linalg.norm(x[p[:, 1]] - x[p[:, 0]], axis=1)
                cut, clamp = bm.wca_cutoff(self.wca[1]), self.r_max - bm.CLAMP
                assert (np.abs(L - cut) >= 1e-3).all() and (np.abs(L - clamp) >= 1e-3).all()
                assert (L < cut).sum() >= 3 and (L > cut).sum() >= 3
                if self.group == "fenewca":
                    assert (L < clamp - 2e-3).all()
                else:
                    assert (L < clamp).sum() >= 3 and (L > clamp).sum() >= 3
        else:
            assert len(set(np.round(self.rest_angle, 6))) >= 4


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    # both sides of the WCA cutoff 1.1225 sigma, well below the clamp
    lengths = [0.85, 0.9, 0.95, 1.0, 1.05, 1.1, CUTOFF - 1.5e-3, CUTOFF + 1.5e-3, 1.13, 1.15, 1.2, 1.25, 1.3, 1.35,
               1.4, 0.87, 0.97, 1.07, 1.17, 1.27, 1.37, 1.02, 1.22]
    x = _walk(rng, lengths)
    out["fenewca"] = Case("fenewca", "fenewca", x, pairs=_chain_pairs(24), k=rng.uniform(5.0, 30.0, 23), r_max=R_MAX,
                          wca=(1.0, 1.0))
    # epsilon and sigma of its own: cutoff 1.0102
    cut = bm.wca_cutoff(0.9)
    lengths = [0.8, 0.85, 0.9, 0.95, 1.0, cut - 1.5e-3, cut + 1.5e-3, 1.05, 1.1, 1.15, 1.2, 1.25, 1.3, 1.35, 1.4, 0.82,
               0.92, 0.98, 1.03, 1.12, 1.22, 1.32, 1.38]
    x = _walk(rng, lengths)
    out["fenewca, epsilon 0.7 sigma 0.9"] = Case("fenewca", "fenewca", x, pairs=_chain_pairs(24),
                                                 k=rng.uniform(5.0, 30.0, 23), r_max=R_MAX, wca=(0.7, 0.9))
    # both sides of the clamp r_max - 1e-4 = 1.4999 (and of the cutoff)
    clamp = R_MAX - bm.CLAMP
    lengths = [clamp - 1.5e-3, clamp + 1.5e-3, 1.6, 2.0, 1.497, 1.51, 0.9, 1.0, 1.1, 1.2, 1.3, 1.4, 1.498, 1.502, 1.55,
               1.75, 2.5, 1.495, 1.05, 0.95, 1.45, 1.48, 1.53]
    x = _walk(rng, lengths)
    out["fenewca, clamped"] = Case("fenewca near the clamp", "fenewca", x, pairs=_chain_pairs(24),
                                   k=rng.uniform(5.0, 30.0, 23), r_max=R_MAX, wca=(1.0, 1.0))
    # a chain's own triplets at several rest angles, and a few triplets that share a centre
    x = _walk(rng, rng.uniform(0.8, 1.2, 25))
    first = np.arange(24)
    trip = np.stack([first, first + 2, first + 1], axis=1)
    trip = np.concatenate([trip, [[0, 9, 5], [3, 20, 5], [25, 12, 5], [7, 2, 18]]]).astype(np.int32)
    angles = np.array([math.pi, 2.5, 2.0, 0.5 * math.pi, 1.0, 0.0, 3.0])
    out["angular"] = Case("angular", "angular", x, triplets=trip, k=rng.uniform(1.0, 20.0, len(trip)),
                          rest_angle=angles[np.arange(len(trip)) % len(angles)])
    return out


NAMES = tuple(cases())
_EXACT = {}


def exact(name, moved=False, cos_rest=None):
    """the mpmath forces of a case, once per (name, frame) -> (F float64 [n, 3], S float64 [n]).  cos_rest: the handle's
    cosines where they are not this machine's (they then key the cache too)"""
    key = (name, moved, None if cos_rest is None else np.asarray(cos_rest).tobytes())
    if key not in _EXACT:
        case = cases()[name]
        with P.hp():
            F, S, _ = P.exact_forces(case.terms(cos_rest), case.moved() if moved else case.x)
            _EXACT[key] = (P.to_float(F), np.array([float(s) for s in S]))
    return _EXACT[key]
