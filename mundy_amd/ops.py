"""Host-side mirror of the reference's hot-path interface over libmundy_hip.so, on torch CUDA(HIP) tensors.

Names follow the reference: compute_aabb / distance / GenNeighborLinks (mundy_mesh/GenNeighborLinkers.hpp) /
solve_cqpp, solve_lcp, PGDConfig, SolveResult (mundy_math/convex.hpp).  torch is plumbing (device memory + the
current stream); all arithmetic runs in the HIP library.  float64 everywhere; pairs are int32 [C, 2].
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import capi
from .capi import (RESIDUAL_PROJECTED_DIFF, RESIDUAL_PROJECTED_GRADIENT, SEARCH_AABB, SEARCH_METHOD_AUTO,  # noqa: F401
                   SEARCH_METHOD_GRID, SEARCH_METHOD_MORTON_LBVH, SEARCH_SPHERES, SPACE_BOUNDED, SPACE_LOWER_BOUND, SPACE_UNCONSTRAINED, SPACE_UPPER_BOUND)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t, dtype=torch.float64, cols=None, name="tensor", allow_none=False):
    if t is None:
        if allow_none:
            return None
        raise ValueError("%s must not be None" % name)
    if not t.is_cuda:
        raise ValueError("%s must live on the GPU (mundy_amd has no CPU path)" % name)
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise ValueError("%s must have shape [n, %d], got %s" % (name, cols, tuple(t.shape)))
    return C.c_void_p(t.data_ptr())


def _new(ref, *shape, dtype=torch.float64):
    return torch.empty(shape, dtype=dtype, device=ref.device)


class _Handle:
    """owner of one library handle self._h; _destroy names the C function that frees it.  close() is idempotent and safe
    on an object whose constructor raised before the handle existed"""
    _h = None
    _destroy = None

    def close(self):
        if self._h:
            getattr(capi.load(), self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host-side validation shared by the wrappers and the stepper (no library call) -----------------------------------
def _finite_nonneg(value, name):
    v = float(value)
    if not (v >= 0.0 and v < float("inf")):
        raise ValueError("%s must be finite and >= 0, got %r" % (name, value))
    return v


def _finite(value, name, ok, what):
    v = float(value)
    if not (math.isfinite(v) and ok(v)):
        raise ValueError("%s must be finite and %s, got %r" % (name, what, v))
    return v


def _read_field(ptr, rows, width, name=None):
    """a copy of `rows` rows of `width` 8-byte words at the library pointer `ptr` as a new device tensor: float64
    [rows, width] ([rows] for width 1), "share" viewed as [rows, 2, 3]; "pairs": int32 [rows, 2], one word per pair"""
    if name == "pairs":
        out, words = torch.empty((rows, 2), dtype=torch.int32, device="cuda"), rows
    else:
        shape = (rows, width) if width > 1 else (rows,)
        out, words = torch.empty(shape, dtype=torch.float64, device="cuda"), rows * width
    if words:
        capi.check(capi.load().mhip_deep_copy(words, C.c_void_p(out.data_ptr()), C.c_void_p(ptr), _stream()))
    return out.view(rows, 2, 3) if name == "share" else out


def _write_field(ptr, rows, width, value, name):
    """the inverse of _read_field for a float64 field: `value` (a device tensor of the field's size) over the library's"""
    if name == "pairs" or value.numel() != rows * width:
        raise ValueError("%s: expected %d float64 values" % (name, rows * width))
    if rows:
        capi.check(capi.load().mhip_deep_copy(rows * width, C.c_void_p(ptr), _ptr(value, name=name), _stream()))


def check_dict_spec(spec, what, keys, optional=()):
    """a keyword given as a dict: it is one, holds no key outside `keys`, and every key not in `optional`"""
    if not isinstance(spec, dict):
        raise ValueError("%s must be a dict with the keys %s" % (what, ", ".join(keys)))
    unknown = sorted(set(spec) - set(keys))
    if unknown:
        raise ValueError("%s: unknown key(s) %s" % (what, ", ".join(unknown)))
    missing = [k for k in keys if k not in spec and k not in optional]
    if missing:
        raise ValueError("%s: missing key(s) %s" % (what, ", ".join(missing)))


def check_philox_ints(t, count, name, dtype=np.int64):
    """Philox keys / counters: integers of shape [count] in [0, 2^63) -> contiguous host array of dtype (None stays None)"""
    if t is None:
        return None
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    if a.dtype.kind not in "iu" or a.shape != (count,):
        raise ValueError("%s must be integers of shape [%d], got %s %s" % (name, count, a.dtype, a.shape))
    if a.size and (int(a.min()) < 0 or int(a.max()) >= 2 ** 63):
        raise ValueError("%s must lie in [0, 2^63)" % name)
    return np.ascontiguousarray(a, dtype=dtype)


def device_info():
    n = C.c_int(0)
    name = C.create_string_buffer(256)
    capi.check(capi.load().mhip_device_info(C.byref(n), name, 256))
    return n.value, name.value.decode()


def memory_stats():
    """What the library holds in this process (mhip_memory_stats; no HIP call): device bytes owned by live handles and
    the spare workspace set, device bytes of the process-lifetime scratch, pinned host bytes, allocation calls so far."""
    names = ("handle_bytes", "scratch_bytes", "pinned_bytes", "allocations")
    vals = [C.c_size_t(0) for _ in names]
    capi.check(capi.load().mhip_memory_stats(*[C.byref(v) for v in vals]))
    return {k: v.value for k, v in zip(names, vals)}


# ---- per-body geometry (compute_aabb.hpp / compute_bounding_radius.hpp) --------------------------------------------
def compute_aabb_spheres(center, radius):
    n = radius.shape[0]
    out = _new(center, n, 6)
    capi.check(capi.load().mhip_compute_aabb_spheres(n, _ptr(center, cols=3), _ptr(radius), _ptr(out), _stream()))
    return out


def compute_aabb_spherocylinders(center, quat, radius, length):
    n = radius.shape[0]
    out = _new(center, n, 6)
    capi.check(capi.load().mhip_compute_aabb_spherocylinders(n, _ptr(center, cols=3), _ptr(quat, cols=4),
                                                             _ptr(radius), _ptr(length), _ptr(out), _stream()))
    return out


def compute_aabb_ellipsoids(center, quat, radii):
    n = center.shape[0]
    out = _new(center, n, 6)
    capi.check(capi.load().mhip_compute_aabb_ellipsoids(n, _ptr(center, cols=3), _ptr(quat, cols=4),
                                                        _ptr(radii, cols=3), _ptr(out), _stream()))
    return out


def compute_aabb_ellipsoids_conservative(center, quat, radii):
    """build extension: tight box of the rotated ellipsoid (the reference's box is not conservative)"""
    n = center.shape[0]
    out = _new(center, n, 6)
    capi.check(capi.load().mhip_compute_aabb_ellipsoids_conservative(n, _ptr(center, cols=3), _ptr(quat, cols=4),
                                                                     _ptr(radii, cols=3), _ptr(out), _stream()))
    return out


def compute_aabb_segments(seg):
    n = seg.shape[0]
    out = _new(seg, n, 6)
    capi.check(capi.load().mhip_compute_aabb_segments(n, _ptr(seg, cols=8), _ptr(out), _stream()))
    return out


def bounding_radius_spherocylinders(radius, length, out=None):
    out = torch.empty_like(radius) if out is None else out
    capi.check(capi.load().mhip_bounding_radius_spherocylinders(radius.shape[0], _ptr(radius), _ptr(length),
                                                                _ptr(out), _stream()))
    return out


def bounding_radius_ellipsoids(radii):
    out = _new(radii, radii.shape[0])
    capi.check(capi.load().mhip_bounding_radius_ellipsoids(radii.shape[0], _ptr(radii, cols=3), _ptr(out), _stream()))
    return out


def spherocylinder_segments(center, quat, radius, length, out=None):
    n = radius.shape[0]
    seg = _new(center, n, 8) if out is None else out
    capi.check(capi.load().mhip_spherocylinder_segments(n, _ptr(center, cols=3), _ptr(quat, cols=4), _ptr(radius),
                                                        _ptr(length), _ptr(seg, cols=8), _stream()))
    return seg


# ---- distances (mundy_geom/distance/*.hpp) ----------------------------------------------------------------------------
def distance_sphere_sphere(c1, r1, c2, r2):
    n = r1.shape[0]
    dist, sep = _new(c1, n), _new(c1, n, 3)
    capi.check(capi.load().mhip_distance_sphere_sphere(n, _ptr(c1, cols=3), _ptr(r1), _ptr(c2, cols=3), _ptr(r2),
                                                       _ptr(dist), _ptr(sep), _stream()))
    return dist, sep


def distance_point_segment(p, a0, a1):
    n = p.shape[0]
    dist, cp, t, sep = _new(p, n), _new(p, n, 3), _new(p, n), _new(p, n, 3)
    capi.check(capi.load().mhip_distance_point_segment(n, _ptr(p, cols=3), _ptr(a0, cols=3), _ptr(a1, cols=3),
                                                       _ptr(dist), _ptr(cp), _ptr(t), _ptr(sep), _stream()))
    return dist, cp, t, sep


def distance_point_sphere(p, c, r):
    """distance(Point, Sphere, sep) (PointSphere.hpp:69-79)."""
    n = p.shape[0]
    dist, sep = _new(p, n), _new(p, n, 3)
    capi.check(capi.load().mhip_distance_point_sphere(n, _ptr(p, cols=3), _ptr(c, cols=3), _ptr(r), _ptr(dist),
                                                      _ptr(sep), _stream()))
    return dist, sep


def distance_segment_sphere(a0, a1, c, r):
    """distance(LineSegment, Sphere, closest_point, arch_length, sep) (LineSegmentSphere.hpp:88-100)."""
    n = a0.shape[0]
    dist, cp, t, sep = _new(a0, n), _new(a0, n, 3), _new(a0, n), _new(a0, n, 3)
    capi.check(capi.load().mhip_distance_segment_sphere(n, _ptr(a0, cols=3), _ptr(a1, cols=3), _ptr(c, cols=3), _ptr(r),
                                                        _ptr(dist), _ptr(cp), _ptr(t), _ptr(sep), _stream()))
    return dist, cp, t, sep


def distance_segment_segment(a0, a1, b0, b1):
    n = a0.shape[0]
    dist, cp1, cp2 = _new(a0, n), _new(a0, n, 3), _new(a0, n, 3)
    s, t, sep = _new(a0, n), _new(a0, n), _new(a0, n, 3)
    capi.check(capi.load().mhip_distance_segment_segment(n, _ptr(a0, cols=3), _ptr(a1, cols=3), _ptr(b0, cols=3),
                                                         _ptr(b1, cols=3), _ptr(dist), _ptr(cp1), _ptr(cp2), _ptr(s),
                                                         _ptr(t), _ptr(sep), _stream()))
    return dist, cp1, cp2, s, t, sep


def distance_ellipsoid_ellipsoid(c1, q1, r1, c2, q2, r2):
    n = c1.shape[0]
    out = dict(dist=_new(c1, n), cp1=_new(c1, n, 3), cp2=_new(c1, n, 3), n1=_new(c1, n, 3), n2=_new(c1, n, 3))
    capi.check(capi.load().mhip_distance_ellipsoid_ellipsoid(
        n, _ptr(c1, cols=3), _ptr(q1, cols=4), _ptr(r1, cols=3), _ptr(c2, cols=3), _ptr(q2, cols=4), _ptr(r2, cols=3),
        _ptr(out["dist"]), _ptr(out["cp1"]), _ptr(out["cp2"]), _ptr(out["n1"]), _ptr(out["n2"]), _stream()))
    return out


def distance_point_ellipsoid(p, c, q, r):
    n = p.shape[0]
    dist, cp, nrm = _new(p, n), _new(p, n, 3), _new(p, n, 3)
    capi.check(capi.load().mhip_distance_point_ellipsoid(n, _ptr(p, cols=3), _ptr(c, cols=3), _ptr(q, cols=4),
                                                         _ptr(r, cols=3), _ptr(dist), _ptr(cp), _ptr(nrm), _stream()))
    return dist, cp, nrm


def contact_ellipsoids(pairs, center, quat, radii):
    c = pairs.shape[0]
    out = dict(sep=_new(center, c), normal=_new(center, c, 3), cp1=_new(center, c, 3), cp2=_new(center, c, 3),
               ra=_new(center, c, 3), rb=_new(center, c, 3))
    capi.check(capi.load().mhip_contact_ellipsoids(
        c, _ptr(pairs, torch.int32, 2), _ptr(center, cols=3), _ptr(quat, cols=4), _ptr(radii, cols=3),
        _ptr(out["sep"]), _ptr(out["normal"]), _ptr(out["cp1"]), _ptr(out["cp2"]), _ptr(out["ra"]), _ptr(out["rb"]),
        _stream()))
    return out


KIND_SPHERE, KIND_ROD, KIND_ELLIPSOID = 0, 1, 2


def compute_aabb_mixed(kind, center, quat, shape, conservative_ellipsoids=False):
    """conservative_ellipsoids=True: BUILD EXTENSION, the tight conservative ellipsoid box instead of the reference's
    (compute_aabb.hpp:82-103, which is not conservative for general orientations)"""
    n = kind.shape[0]
    aabb, brad = _new(center, n, 6), _new(center, n)
    fn = capi.load().mhip_compute_aabb_mixed_conservative if conservative_ellipsoids else capi.load().mhip_compute_aabb_mixed
    capi.check(fn(n, _ptr(kind, torch.int32), _ptr(center, cols=3), _ptr(quat, cols=4), _ptr(shape, cols=3),
                  _ptr(aabb), _ptr(brad), _stream()))
    return aabb, brad


def contact_mixed(pairs, kind, center, quat, shape, want_counts=False, box=None):
    """box: 3 edge lengths of an orthorhombic periodic box (body j at the nearest image of its centre)"""
    c = pairs.shape[0]
    out = dict(sep=_new(center, c), normal=_new(center, c, 3), cp1=_new(center, c, 3), cp2=_new(center, c, 3),
               ra=_new(center, c, 3), rb=_new(center, c, 3))
    counts = (C.c_size_t * 6)() if want_counts else None
    if box is not None:
        capi.check(capi.load().mhip_contact_mixed_periodic(
            c, _ptr(pairs, torch.int32, 2), _ptr(kind, torch.int32), _ptr(center, cols=3), _ptr(quat, cols=4),
            _ptr(shape, cols=3), (C.c_double * 3)(*[float(b) for b in box]), _ptr(out["sep"]), _ptr(out["normal"]),
            _ptr(out["cp1"]), _ptr(out["cp2"]), _ptr(out["ra"]), _ptr(out["rb"]), counts, _stream()))
    else:
        capi.check(capi.load().mhip_contact_mixed(
            c, _ptr(pairs, torch.int32, 2), _ptr(kind, torch.int32), _ptr(center, cols=3), _ptr(quat, cols=4),
            _ptr(shape, cols=3), _ptr(out["sep"]), _ptr(out["normal"]), _ptr(out["cp1"]), _ptr(out["cp2"]),
            _ptr(out["ra"]), _ptr(out["rb"]), counts, _stream()))
    if want_counts:
        out["class_counts"] = dict(zip(("SS", "SR", "SE", "RR", "RE", "EE"), [int(v) for v in counts]))
    return out


def contact_mixed_set_sphere_ellipsoid_route(reference_minimiser):
    """S-E of contact_mixed: False (default) = the exact point - ellipsoid distance in closed form, True = the reference's
    own point - ellipsoid routine (nine-start L-BFGS, PointEllipsoid.hpp:94-135), which the closed form matches to 1e-4"""
    capi.check(capi.load().mhip_contact_mixed_set_sphere_ellipsoid_route(1 if reference_minimiser else 0))


def contact_mixed_set_contraction(on):
    """BUILD OPTION (labelled): the S-E / E-E minimisation classes of contact_mixed from the build with fused
    multiply-adds -- results at the reference's 1e-4 instead of bit parity with the oracle.  Default off."""
    capi.check(capi.load().mhip_contact_mixed_set_contraction(1 if on else 0))


def contact_mixed_last_evaluations():
    """objective evaluations of the (S-E, R-E, E-E) classes in the last contact_mixed call (R-E is closed-form: 0)"""
    ev = (C.c_ulonglong * 3)()
    capi.check(capi.load().mhip_contact_mixed_last_evaluations(ev, _stream()))
    return dict(SE=int(ev[0]), RE=int(ev[1]), EE=int(ev[2]))


def ellipsoid_last_evaluations():
    ev = C.c_ulonglong(0)
    capi.check(capi.load().mhip_ellipsoid_last_evaluations(C.byref(ev), _stream()))
    return int(ev.value)


def _cell(box):
    """periodic cell argument: 3 edge lengths (PeriodicScaledMetric) or a 3x3 unit-cell matrix with the lattice vectors
    as columns (PeriodicMetric).  Returns (is_triclinic, ctypes array)."""
    import numpy as _np
    a = _np.asarray(box.detach().cpu() if isinstance(box, torch.Tensor) else box, dtype=_np.float64)
    if a.size == 3:
        return False, (C.c_double * 3)(*a.reshape(3).tolist())
    if a.size == 9:
        return True, (C.c_double * 9)(*a.reshape(9).tolist())
    raise ValueError("periodic cell must be 3 edge lengths or a 3x3 unit-cell matrix, got shape %s" % (a.shape,))


def contact_spheres(pairs, center, radius, box=None, out=None):
    c = pairs.shape[0]
    sep, normal = (_new(center, c), _new(center, c, 3)) if out is None else out
    tri, boxp = (False, None) if box is None else _cell(box)
    fn = capi.load().mhip_contact_spheres_triclinic if tri else capi.load().mhip_contact_spheres
    capi.check(fn(c, _ptr(pairs, torch.int32, 2), _ptr(center, cols=3), _ptr(radius), boxp, _ptr(sep), _ptr(normal),
                  _stream()))
    return sep, normal


def contact_spherocylinders(pairs, seg, center, want_points=True, out=None, arms="vector", box=None):
    """arms="vector": lever arms ra / rb [C,3]; arms="arclength": only (s, t), for ContactOperator(rod=...).
    box: 3 edge lengths of an orthorhombic periodic box (rod j at the nearest image of its centre)."""
    c = pairs.shape[0]
    if out is None:
        out = dict(sep=_new(seg, c), normal=_new(seg, c, 3))
        if arms == "vector":
            out.update(ra=_new(seg, c, 3), rb=_new(seg, c, 3))
        if want_points or arms == "arclength":
            out.update(s=_new(seg, c), t=_new(seg, c))
        if want_points:
            out.update(cp1=_new(seg, c, 3), cp2=_new(seg, c, 3))
    g = lambda k: _ptr(out.get(k), allow_none=True, name=k)  # noqa: E731
    if box is not None:
        capi.check(capi.load().mhip_contact_spherocylinders_periodic(
            c, _ptr(pairs, torch.int32, 2), _ptr(seg, cols=8), _ptr(center, cols=3),
            (C.c_double * 3)(*[float(b) for b in box]), g("sep"), g("normal"), g("cp1"), g("cp2"), g("ra"), g("rb"),
            g("s"), g("t"), _stream()))
        return out
    capi.check(capi.load().mhip_contact_spherocylinders(c, _ptr(pairs, torch.int32, 2), _ptr(seg, cols=8),
                                                        _ptr(center, cols=3), g("sep"), g("normal"), g("cp1"),
                                                        g("cp2"), g("ra"), g("rb"), g("s"), g("t"), _stream()))
    return out


def _material(value, n, name, lo, hi):
    """a per-body material parameter: a number (checked here, on the host) -> (None, value); a tensor [n] -> (tensor, 0)"""
    if isinstance(value, torch.Tensor):
        if value.dim() != 1 or value.shape[0] != n:
            raise ValueError("%s must be a number or a tensor of shape [%d], got %s" % (name, n, tuple(value.shape)))
        return value, 0.0
    v = float(value)
    if not (lo < v < hi):
        raise ValueError("%s must lie in (%g, %g), got %r" % (name, lo, hi, value))
    return None, v


def hertz_contact_force(pairs, sep, radius, youngs_modulus=1000.0, poisson_ratio=0.3, out=None, max_overlap=None):
    """Hertzian soft contact per linker (EvaluateLinkerPotentials, Bacteria.cpp:755-804; mhip_hertz_contact_force):
    f_c = (4/3) E* sqrt(R*) (-sep_c)^1.5 for sep_c < 0, else +0.0.  radius [n] = sphere / rod radius (not the bounding
    radius); youngs_modulus (E > 0) and poisson_ratio (0 < nu < 1) are numbers or per-body tensors [n] (defaults:
    Bacteria.cpp:1213-1214).  Returns (f [C], max_overlap [1] device tensor = max(0, -sep))."""
    c, n = pairs.shape[0], radius.shape[0]
    E, E0 = _material(youngs_modulus, n, "youngs_modulus", 0.0, float("inf"))
    nu, nu0 = _material(poisson_ratio, n, "poisson_ratio", 0.0, 1.0)
    f = _new(sep, c) if out is None else out
    mx = _new(sep, 1) if max_overlap is None else max_overlap
    capi.check(capi.load().mhip_hertz_contact_force(c, n, _ptr(pairs, torch.int32, 2, name="pairs"), _ptr(sep, name="sep"),
                                                    _ptr(radius, name="radius"),
                                                    _ptr(E, allow_none=True, name="youngs_modulus"), E0,
                                                    _ptr(nu, allow_none=True, name="poisson_ratio"), nu0,
                                                    _ptr(f, name="out"), _ptr(mx, name="max_overlap"), _stream()))
    return f, mx


def hertz_friction_force(pairs, sep, normal, arc_s, arc_t, seg, radius, velocity_prev, tang_disp, mu, dt,
                         damping=(0.0, 0.0), density=1.0, youngs_modulus=1000.0, poisson_ratio=0.3, out=None,
                         stats=None):
    """Frictional Hertzian rod contact per linker with a tangential history (mhip_hertz_friction_force; the reference's
    SpherocylinderSegmentSpherocylinderSegmentFrictionalHertzianContact.cpp:384-518).  velocity_prev [n, 6] = the
    previous step's (U, W) rows; tang_disp [C, 3] is updated in place ("j relative to i"); damping = (normal,
    tangential).  Returns (force [C, 3] on body i -- body j receives its negative, ContactOperator.body_sweep_vector --,
    stats [2] float64 device tensor: max(0, -sep), and the number of capped contacts as int64 bits: stats.view(int64)[1])."""
    c, n = pairs.shape[0], radius.shape[0]
    E, E0 = _material(youngs_modulus, n, "youngs_modulus", 0.0, float("inf"))
    nu, nu0 = _material(poisson_ratio, n, "poisson_ratio", 0.0, 1.0)
    prm = capi.HertzFrictionParams(_finite_nonneg(mu, "mu"), _finite_nonneg(damping[0], "normal damping"),
                                   _finite_nonneg(damping[1], "tangential damping"),
                                   _finite_nonneg(density, "density"), _finite_nonneg(dt, "dt"))
    if tuple(tang_disp.shape) != (c, 3):
        raise ValueError("tang_disp must have shape [%d, 3], got %s" % (c, tuple(tang_disp.shape)))
    if tuple(velocity_prev.shape) != (n, 6):
        raise ValueError("velocity_prev must have shape [%d, 6], got %s" % (n, tuple(velocity_prev.shape)))
    for name, t in (("sep", sep), ("arc_s", arc_s), ("arc_t", arc_t)):
        if tuple(t.shape) != (c,):
            raise ValueError("%s must have shape [%d], got %s" % (name, c, tuple(t.shape)))
    if tuple(normal.shape) != (c, 3) or tuple(seg.shape) != (n, 8):
        raise ValueError("normal must have shape [%d, 3] and seg [%d, 8]" % (c, n))
    f = _new(sep, c, 3) if out is None else out
    if tuple(f.shape) != (c, 3):
        raise ValueError("out must have shape [%d, 3], got %s" % (c, tuple(f.shape)))
    if out is None:
        f.zero_()  # (rows out of contact are written only where they are not +0.0 already)
    st = _new(sep, 2) if stats is None else stats
    capi.check(capi.load().mhip_hertz_friction_force(
        c, n, _ptr(pairs, torch.int32, 2, name="pairs"), _ptr(sep, name="sep"), _ptr(normal, cols=3, name="normal"),
        _ptr(arc_s, name="arc_s"), _ptr(arc_t, name="arc_t"), _ptr(seg, cols=8, name="seg"), _ptr(radius, name="radius"),
        _ptr(E, allow_none=True, name="youngs_modulus"), E0, _ptr(nu, allow_none=True, name="poisson_ratio"), nu0,
        _ptr(velocity_prev, cols=6, name="velocity_prev"), C.byref(prm), _ptr(tang_disp, cols=3, name="tang_disp"),
        _ptr(f, cols=3, name="out"), _ptr(st, name="stats"), _stream()))
    return f, st


def carry_contact_history(pairs_old, hist_old, pairs_new, new_of_old=None, want_count=False):
    """history rows [C_old, 3] of the pairs of one contact list -> rows [C_new, 3] of the next: a new pair (i, j) receives
    the row of the old pair whose endpoints, renumbered through new_of_old [n_old] int32 (None: unchanged numbering, and
    the old list must be the broad phase's canonical sorted one), are {i, j}, negated if the orientation came out
    swapped; every other new pair +0.0 (mhip_contact_history_carry).  want_count: returns (rows, carried).  Synchronises
    when want_count or new_of_old is None; an unrenumbered old list that does not ascend strictly raises ValueError."""
    c_old, c_new = pairs_old.shape[0], pairs_new.shape[0]
    if tuple(hist_old.shape) != (c_old, 3):
        raise ValueError("hist_old must have shape [%d, 3], got %s" % (c_old, tuple(hist_old.shape)))
    out = _new(hist_old, c_new, 3)
    n_old = 0 if new_of_old is None else new_of_old.shape[0]
    k = C.c_size_t(0)
    capi.check(capi.load().mhip_contact_history_carry(
        c_old, _ptr(pairs_old, torch.int32, 2, name="pairs_old"), _ptr(hist_old, cols=3, name="hist_old"),
        _ptr(new_of_old, torch.int32, allow_none=True, name="new_of_old"), n_old, c_new,
        _ptr(pairs_new, torch.int32, 2, name="pairs_new"), _ptr(out, cols=3, name="hist_new"),
        C.byref(k) if want_count else None, _stream()))
    return (out, int(k.value)) if want_count else out


# ---- broad phase (GenNeighborLinks, mundy_mesh/GenNeighborLinkers.hpp:294-866) ---------------------------------------
class GenNeighborLinks(_Handle):
    """Builder-style mirror of mundy::mesh::GenNeighborLinks: set_* -> concretize() -> generate().

    generate(aabb, center, bounding_radius) returns True when a search was performed (first call, or some centre moved
    more than half the search buffer, :510-543, :603-615); the links are then available as .pairs ([P, 2] int32,
    sorted by (source, target)), .row_ptr / .col (CSR).
    """
    _destroy = "mhip_broadphase_destroy"

    def __init__(self):
        h = C.c_void_p()
        capi.check(capi.load().mhip_broadphase_create(C.byref(h)))
        self._h = h
        self._cfg = capi.BroadphaseConfig(SEARCH_SPHERES, 0, 0.0, 0, (C.c_double * 3)(0, 0, 0), 0, 0)
        self._concretized = False
        self._generated = False
        self.pairs = self.row_ptr = self.col = None
        self.num_pairs = 0

    def _setter_guard(self, what):
        if self._concretized:
            raise RuntimeError("Cannot set %s after concretization." % what)  # :402-462

    def set_search_buffer(self, search_buffer):
        self._setter_guard("search buffer")
        self._cfg.buffer = float(search_buffer)
        return self

    def set_search_kind(self, kind):
        self._setter_guard("search kind")
        self._cfg.search_kind = int(kind)
        return self

    def set_enforce_source_target_symmetry(self, value):
        self._setter_guard("enforce source-target symmetry")
        self._cfg.symmetric = 1 if value else 0
        return self

    def set_periodic_box(self, box):
        self._setter_guard("periodic box")
        if box is None:
            self._cfg.periodic = 0
        else:
            a = np.asarray(box, dtype=np.float64)
            if a.shape == (3,):
                self._cfg.periodic = 1
                self._cfg.box = (C.c_double * 3)(*[float(b) for b in a])
            elif a.shape == (3, 3):   # the unit cell of PeriodicMetric: lattice vectors as columns (periodicity.hpp:233-332)
                self._cfg.periodic = 2
                self._cfg.cell = (C.c_double * 9)(*[float(b) for b in a.reshape(9)])
            else:
                raise ValueError("periodic cell must be 3 edge lengths or a 3x3 unit-cell matrix, got shape %s" % (a.shape,))
        return self

    def set_search_method(self, method):
        """stk::search::SearchMethod of the reference (:443-447; its default is MORTON_LBVH): SEARCH_METHOD_AUTO,
        SEARCH_METHOD_GRID or SEARCH_METHOD_MORTON_LBVH -- same lists, different structure"""
        self._setter_guard("search method")
        self._cfg.method = int(method)
        return self

    def set_exclude_self_interactions(self, value=True):
        """search_filters::ExcludeSelfInteractions (:185-200); the default.  False lets (i, i) be a result."""
        self._setter_guard("search filter")
        self._cfg.include_self = 0 if value else 1
        return self

    def acts_on(self, source_mask=None, target_mask=None):
        """acts_on(source_selector, target_selector, ...) (:486-507): uint8 masks [n] over the bodies (None = all); a
        result (s, t) needs s among the sources and t among the targets"""
        self._setter_guard("source/targets")
        self._sets = (source_mask, target_mask)
        n = (source_mask if source_mask is not None else target_mask)
        capi.check(capi.load().mhip_broadphase_set_sets(
            self._h, 0 if n is None else n.shape[0], _ptr(source_mask, torch.uint8, allow_none=True, name="source_mask"),
            _ptr(target_mask, torch.uint8, allow_none=True, name="target_mask"), _stream()))
        return self

    def set_excluded_partners(self, ex_ptr, ex_idx):
        """search_filters::ExcludeConnectedEntities (:202-236) / the already-linked neighbours when duplicate links
        are not allowed (:91-113): CSR (int32 ex_ptr [n + 1], ex_idx) of partners each source must not be paired with.
        May be called again between generates (the connectivity of a mesh changes); it invalidates the list."""
        if ex_ptr is None:
            capi.check(capi.load().mhip_broadphase_set_exclusions(self._h, 0, None, None, 0, _stream()))
        else:
            capi.check(capi.load().mhip_broadphase_set_exclusions(
                self._h, ex_ptr.shape[0] - 1, _ptr(ex_ptr, torch.int32, name="ex_ptr"),
                _ptr(ex_idx, torch.int32, name="ex_idx"), ex_idx.shape[0], _stream()))
        self._generated = False
        return self

    def set_identities(self, entity_id=None, owner_rank=None, n=None):
        """(stk::mesh::EntityId, owner rank) of every body (:575-584): int64 ids (bit pattern of the u64), int32 ranks"""
        n = n if n is not None else (entity_id if entity_id is not None else owner_rank).shape[0]
        capi.check(capi.load().mhip_broadphase_set_identities(
            self._h, n, _ptr(entity_id, torch.int64, allow_none=True, name="entity_id"),
            _ptr(owner_rank, torch.int32, allow_none=True, name="owner_rank"), _stream()))
        return self

    def ident_pairs(self):
        """the links as stk::search IdentProcIntersection rows: (source id, source proc, target id, target proc)"""
        dev = self.pairs.device
        sid, tid = (torch.empty(self.num_pairs, dtype=torch.int64, device=dev) for _ in range(2))
        sp, tp = (torch.empty(self.num_pairs, dtype=torch.int32, device=dev) for _ in range(2))
        capi.check(capi.load().mhip_broadphase_get_ident_pairs(self._h, _ptr(sid, torch.int64), _ptr(sp, torch.int32),
                                                               _ptr(tid, torch.int64), _ptr(tp, torch.int32), _stream()))
        return sid, sp, tid, tp

    def method_used(self):
        m = C.c_int(0)
        capi.check(capi.load().mhip_broadphase_method_used(self._h, C.byref(m)))
        return m.value

    def minimum_image_complete(self):
        """False when the last build's periodic cell was so small (an edge <= 4 x the largest reach) that volumes can
        also meet through a second image -- pairs the minimum-image predicate does not report"""
        m = C.c_int(0)
        capi.check(capi.load().mhip_broadphase_minimum_image_complete(self._h, C.byref(m)))
        return bool(m.value)

    def export_coo(self, first_link_id=0, source_rank=3, target_rank=3):
        """MuNDy's LinkCOOData rows (LinkMetaData.hpp:102-106): (link ids [P], linked entity ids [P, 2], linked entity
        ranks [P, 2] uint8; 3 = stk::topology::ELEM_RANK)"""
        dev = self.pairs.device
        lid = torch.empty(self.num_pairs, dtype=torch.int64, device=dev)
        ids = torch.empty((self.num_pairs, 2), dtype=torch.int64, device=dev)
        ranks = torch.empty((self.num_pairs, 2), dtype=torch.uint8, device=dev)
        capi.check(capi.load().mhip_links_export_coo(self._h, int(first_link_id), int(source_rank), int(target_rank),
                                                     _ptr(lid, torch.int64), _ptr(ids, torch.int64),
                                                     _ptr(ranks, torch.uint8), _stream()))
        return lid, ids, ranks

    def export_crs(self, first_link_id=0, bucket_capacity=512):
        """entity -> connected links in LinkCRSBucketConn's layout (LinkCRSBucketConn.hpp:183-191), entities in index
        order cut into buckets of bucket_capacity: (num_connected_links [n], sparse_connectivity_offsets [nb, cap + 1],
        sparse_connectivity [2 P], bucket_begin [nb + 1])"""
        dev = self.pairs.device
        n = self.row_ptr.shape[0] - 1
        nb = (n + bucket_capacity - 1) // bucket_capacity
        num = torch.empty(n, dtype=torch.int32, device=dev)
        offs = torch.empty((nb, bucket_capacity + 1), dtype=torch.int32, device=dev)
        conn = torch.empty(2 * self.num_pairs, dtype=torch.int64, device=dev)
        begin = torch.empty(nb + 1, dtype=torch.int64, device=dev)
        capi.check(capi.load().mhip_links_export_crs(self._h, int(first_link_id), int(bucket_capacity),
                                                     _ptr(num, torch.int32), _ptr(offs, torch.int32),
                                                     _ptr(conn, torch.int64), _ptr(begin, torch.int64), _stream()))
        return num, offs, conn, begin

    def concretize(self):
        if self._concretized:
            raise RuntimeError("Cannot concretize more than once.")  # :494
        self._concretized = True
        return self

    def needs_rebuild(self, center):
        flag = C.c_int(0)
        capi.check(capi.load().mhip_broadphase_needs_rebuild(self._h, center.shape[0], _ptr(center, cols=3),
                                                             C.byref(flag), _stream()))
        return bool(flag.value)

    def invalidate(self):
        """the body numbering changed (reordering, migration): the next generate() rebuilds whatever the rebuild rule says"""
        self._generated = False

    @property
    def generated(self):
        """True once generate() has built a list that invalidate() has not discarded since"""
        return self._generated

    def generate(self, aabb, center, bounding_radius, force=False):
        if not self._concretized:
            raise RuntimeError("Cannot generate links before concretization.")  # :511
        if self._generated and not force and not self.needs_rebuild(center):
            return False
        n = center.shape[0]
        cnt = C.c_size_t(0)
        capi.check(capi.load().mhip_broadphase_build(
            self._h, C.byref(self._cfg), n, _ptr(aabb, cols=6, allow_none=True, name="aabb"), _ptr(center, cols=3),
            _ptr(bounding_radius, allow_none=True, name="bounding_radius"), C.byref(cnt), _stream()))
        self.num_pairs = int(cnt.value)
        self.pairs = torch.empty((self.num_pairs, 2), dtype=torch.int32, device=center.device)
        self.row_ptr = torch.empty(n + 1, dtype=torch.int32, device=center.device)
        self.col = torch.empty(self.num_pairs, dtype=torch.int32, device=center.device)
        capi.check(capi.load().mhip_broadphase_get_pairs(self._h, _ptr(self.pairs, torch.int32),
                                                         _ptr(self.row_ptr, torch.int32), _ptr(self.col, torch.int32),
                                                         _stream()))
        self._generated = True
        return True


# ---- convex (mundy_math/convex.hpp) ----------------------------------------------------------------------------------
@dataclass
class PGDConfig:  # convex.hpp:519-525
    max_iters: int = 1000
    tol: float = 1e-8
    residual_kind: int = RESIDUAL_PROJECTED_DIFF


@dataclass
class SolveResult:  # convex.hpp:527-541
    num_iters: int = 0
    residual: float = 0.0
    converged: bool = False


def _space(space):
    kind, lo, hi = space
    return capi.Space(int(kind), float(lo), float(hi))


def _cfg(cfg):
    return capi.PgdConfig(int(cfg.max_iters), float(cfg.tol), int(cfg.residual_kind))


LCP_SPACE = (SPACE_LOWER_BOUND, 0.0, 0.0)  # to_cqpp: LowerBound{0} (convex.hpp:424-428)


def axpby(alpha, x, beta, y):
    capi.check(capi.load().mhip_axpby(x.shape[0], alpha, _ptr(x), beta, _ptr(y), _stream()))


def wrapped_axpbyz(alpha, x, beta, y, z, space):
    sp = _space(space)
    capi.check(capi.load().mhip_wrapped_axpbyz(x.shape[0], alpha, _ptr(x), beta, _ptr(y), _ptr(z), C.byref(sp),
                                               _stream()))


def diff_dot(x, y, x2=None, y2=None):
    r = C.c_double()
    if x2 is None:
        capi.check(capi.load().mhip_diff_dot2(x.shape[0], _ptr(x), _ptr(y), C.byref(r), _stream()))
    else:  # diff_dot(x1, x2, y1, y2) = sum (x1-x2)(y1-y2)
        capi.check(capi.load().mhip_diff_dot4(x.shape[0], _ptr(x), _ptr(y), _ptr(x2), _ptr(y2), C.byref(r), _stream()))
    return r.value


def residual(kind, x, grad, space):
    r = C.c_double()
    sp = _space(space)
    capi.check(capi.load().mhip_residual(x.shape[0], kind, _ptr(x), _ptr(grad), C.byref(sp), C.byref(r), _stream()))
    return r.value


def bb_step(x_old, g_old, x, g):
    r = C.c_double()
    capi.check(capi.load().mhip_bb_step(x.shape[0], _ptr(x_old), _ptr(g_old), _ptr(x), _ptr(g), C.byref(r), _stream()))
    return r.value


def gemv(A, x):
    y = torch.empty_like(x)
    capi.check(capi.load().mhip_gemv(x.shape[0], _ptr(A), _ptr(x), _ptr(y), _stream()))
    return y


class ContactOperator(_Handle):
    """Matrix-free A = dt D^T M D over a neighbour list (the LinearOp of seam S2; apply(x, y) as convex.hpp:133-136)."""
    _destroy = "mhip_contact_op_destroy"

    def __init__(self, pairs, normal, mob_trans, dt, ra=None, rb=None, mob_rot=None, rod=None, priority=None):
        """rod = (arc_s, arc_t, seg): spherocylinders with rod-compressed lever arms (mhip_contact_op_create_rods).
        priority [C] (optional, e.g. the signed separations): locality hint -- each body lists the contacts with
        priority < 0 first; changes nothing but the summation order."""
        self.num_constraints = pairs.shape[0]
        self.num_bodies = mob_trans.shape[0]
        self._keep = (pairs, normal, ra, rb, mob_trans, mob_rot, rod, priority)  # the handle holds views of these
        prio = _ptr(priority, allow_none=True, name="priority")
        h = C.c_void_p()
        if rod is not None:
            arc_s, arc_t, seg = rod
            capi.check(capi.load().mhip_contact_op_create_rods(
                C.byref(h), self.num_constraints, self.num_bodies, _ptr(pairs, torch.int32, 2), _ptr(normal, cols=3),
                _ptr(arc_s), _ptr(arc_t), _ptr(seg, cols=8), _ptr(mob_trans), _ptr(mob_rot), float(dt), prio, _stream()))
        else:
            capi.check(capi.load().mhip_contact_op_create(
                C.byref(h), self.num_constraints, self.num_bodies, _ptr(pairs, torch.int32, 2), _ptr(normal, cols=3),
                _ptr(ra, allow_none=True, name="ra"), _ptr(rb, allow_none=True, name="rb"), _ptr(mob_trans),
                _ptr(mob_rot, allow_none=True, name="mob_rot"), float(dt), prio, _stream()))
        self._h = h
        self._device = normal.device

    def refresh(self, normal, ra=None, rb=None, rod=None):
        """same pairs, new geometry (a step that reuses the neighbour list): keeps the incidence index, redoes the
        half-edge records from the new arrays (mhip_contact_op_refresh[_rods])"""
        pairs, _, _, _, mob_trans, mob_rot, old_rod, priority = self._keep
        if (rod is None) != (old_rod is None):
            raise ValueError("refresh must keep the operator's kinematics")
        if rod is not None:
            arc_s, arc_t, seg = rod
            capi.check(capi.load().mhip_contact_op_refresh_rods(self._h, _ptr(normal, cols=3), _ptr(arc_s), _ptr(arc_t),
                                                                _ptr(seg, cols=8), _stream()))
        else:
            capi.check(capi.load().mhip_contact_op_refresh(self._h, _ptr(normal, cols=3),
                                                           _ptr(ra, allow_none=True, name="ra"),
                                                           _ptr(rb, allow_none=True, name="rb"), _stream()))
        self._keep = (pairs, normal, ra, rb, mob_trans, mob_rot, rod, priority)

    def apply(self, x, y=None):
        y = torch.empty_like(x) if y is None else y
        capi.check(capi.load().mhip_contact_op_apply(self._h, _ptr(x), _ptr(y), _stream()))
        return y

    def apply_hydro(self, mobility, x, y=None):
        """y = dt D^T M_h D x with the hydrodynamic mobility M_h = m_t + hydro_kind (+ the periphery's correction) of a
        HydroMobility (mhip_contact_op_apply_hydro; include/mundy_hip_hydro_solve.h); body_velocity() then reads the
        rows M_h D x.  Bit for bit the composition body_force -> m_t F -> hydro_velocity -> correct -> dt constraint_rate."""
        if not isinstance(mobility, HydroMobility):
            raise ValueError("mobility must be a HydroMobility, got %r" % (mobility,))
        if tuple(x.shape) != (self.num_constraints,):
            raise ValueError("x must have shape [%d], got %s" % (self.num_constraints, tuple(x.shape)))
        mobility.check_operator(self)
        y = torch.empty_like(x) if y is None else y
        if tuple(y.shape) != (self.num_constraints,):
            raise ValueError("y must have shape [%d], got %s" % (self.num_constraints, tuple(y.shape)))
        capi.check(capi.load().mhip_contact_op_apply_hydro(self._h, C.byref(mobility.struct), _ptr(x, name="x"),
                                                           _ptr(y, name="y"), _stream()))
        return y

    def body_sweep(self, x):
        """the velocity rows (U, W) = M D x of per-contact force magnitudes x [C] (body i gets -x n, body j +x n): the
        body sweep alone, no constraint sweep (LinkerPotentialForceReduction + compute_generalized_velocity,
        mhip_contact_op_body_sweep); body_velocity() reads them"""
        if tuple(x.shape) != (self.num_constraints,):
            raise ValueError("x must have shape [%d], got %s" % (self.num_constraints, tuple(x.shape)))
        capi.check(capi.load().mhip_contact_op_body_sweep(self._h, _ptr(x, name="x"), _stream()))

    def body_sweep_vector(self, force):
        """the velocity rows (U, W) of a vector force per contact, force [C, 3]: body i gets +F_c, body j -F_c, at the
        operator's lever arms (mhip_contact_op_body_sweep_vector); body_velocity() reads them.
        body_sweep_vector(-x[:, None] * n) gives the rows of body_sweep(x) bit for bit."""
        if tuple(force.shape) != (self.num_constraints, 3):
            raise ValueError("force must have shape [%d, 3], got %s" % (self.num_constraints, tuple(force.shape)))
        capi.check(capi.load().mhip_contact_op_body_sweep_vector(self._h, _ptr(force, name="force"), _stream()))

    def _body_force(self, fn, arr, name, out, stride, accumulate):
        if stride not in (3, 6):
            raise ValueError("stride must be 3 or 6, got %r" % (stride,))
        if not isinstance(accumulate, (bool, np.bool_)):
            raise ValueError("accumulate must be a bool, got %r" % (accumulate,))
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs out")
            out = torch.empty((self.num_bodies, stride), dtype=torch.float64, device=self._device)
        elif tuple(out.shape) != (self.num_bodies, stride):
            raise ValueError("out must have shape [%d, %d], got %s" % (self.num_bodies, stride, tuple(out.shape)))
        capi.check(getattr(capi.load(), fn)(self._h, _ptr(arr, name=name), _ptr(out, name="out"), int(stride),
                                            1 if accumulate else 0, _stream()))
        return out

    def body_force(self, x, out=None, stride=6, accumulate=False):
        """the per-body contact force (and, stride 6, torque about the centre) D x of per-contact multipliers x [C]:
        F_b = sum -/+ x_c n_c (source / target), T_b from the operator's lever arms, the mobility never applied
        (mhip_contact_op_body_force; include/mundy_hip_contact_force.h).  out [N, stride] (default: a new one);
        accumulate adds the rounded sums to what out holds.  body_velocity() is left as it is.
        body_velocity_of(x)[:, :3] == mob_trans[:, None] * body_force(x)[:, :3] bit for bit."""
        if tuple(x.shape) != (self.num_constraints,):
            raise ValueError("x must have shape [%d], got %s" % (self.num_constraints, tuple(x.shape)))
        return self._body_force("mhip_contact_op_body_force", x, "x", out, stride, accumulate)

    def body_force_vector(self, force, out=None, stride=6, accumulate=False):
        """the same sums of a vector force per contact, force [C, 3]: body i gets +F_c, body j -F_c
        (mhip_contact_op_body_force_vector).  body_force_vector(-x[:, None] * n) equals body_force(x) bit for bit."""
        if tuple(force.shape) != (self.num_constraints, 3):
            raise ValueError("force must have shape [%d, 3], got %s" % (self.num_constraints, tuple(force.shape)))
        return self._body_force("mhip_contact_op_body_force_vector", force, "force", out, stride, accumulate)

    def constraint_rate(self, velocity, out=None):
        """sep_dot [C] = D^T U of a velocity [N, 6] (U, W): n_c . [(U_j + W_j x rb) - (U_i + W_i x ra)] with this
        operator's kinematics -- the adjoint of body_sweep, without apply's dt (mhip_contact_op_constraint_rate)"""
        if tuple(velocity.shape) != (self.num_bodies, 6):
            raise ValueError("velocity must have shape [%d, 6], got %s" % (self.num_bodies, tuple(velocity.shape)))
        y = torch.empty(self.num_constraints, dtype=torch.float64, device=self._device) if out is None else out
        capi.check(capi.load().mhip_contact_op_constraint_rate(self._h, _ptr(velocity, cols=6, name="velocity"),
                                                               _ptr(y, name="out"), _stream()))
        return y

    def body_velocity_of(self, x):
        """[N, 6] (U, W) = M D x (body_sweep, then a copy of the rows)"""
        self.body_sweep(x)
        return self.body_velocity()

    def body_velocity(self):
        """[N, 6] (U, W) of the last evaluated iterate -- a view of handle-owned memory; clone to keep."""
        p = C.c_void_p()
        capi.check(capi.load().mhip_contact_op_body_velocity(self._h, C.byref(p)))
        n = self.num_bodies
        if n == 0:
            return torch.empty((0, 6), dtype=torch.float64, device=self._device)
        out = torch.empty((n, 6), dtype=torch.float64, device=self._device)
        capi.check(capi.load().mhip_deep_copy(6 * n, _ptr(out), p, _stream()))
        return out

    def set_work_mapping(self, xcd_tile=-1, lanes_per_body=-1):
        """layout of the sweeps on the chip (time only; results do not depend on it)"""
        capi.check(capi.load().mhip_contact_op_set_work_mapping(self._h, int(xcd_tile), int(lanes_per_body)))

    def set_tiering(self, mode=1):
        """cold tier of the fused solve: 0 off, 1 on (default), 2 test hook (time only; results do not depend on it)"""
        capi.check(capi.load().mhip_contact_op_set_tiering(self._h, int(mode)))

    def set_drift_source(self, source=0):
        """tiered solves, time only: 0 by size, 1 drift from the difference of the two body rows, 2 from the change of
        the force kept in registers (mhip_contact_op_set_drift_source)"""
        capi.check(capi.load().mhip_contact_op_set_drift_source(self._h, int(source)))

    def drift_source(self):
        """the form a tiered solve on this operator takes: 1 rows, 2 registers"""
        v = C.c_int(0)
        capi.check(capi.load().mhip_contact_op_get_drift_source(self._h, C.byref(v)))
        return int(v.value)

    def tier_stats(self):
        """(tiered iterations, mean hot share, renumberings, wake-ups) of the last solve_lcp on this operator"""
        it, rn, wk, hot = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_double(0.0)
        capi.check(capi.load().mhip_contact_op_tier_stats(self._h, C.byref(it), C.byref(hot), C.byref(rn), C.byref(wk)))
        return dict(tiered_iterations=it.value, mean_hot_fraction=hot.value, renumberings=rn.value, wakeups=wk.value)

    def set_profiling(self, enable=True):
        capi.check(capi.load().mhip_contact_op_set_profiling(self._h, 1 if enable else 0))

    def get_profile(self):
        """(k_body ms, k_constraint ms, timed iterations) accumulated by the fused solver since set_profiling"""
        a, b, n = C.c_double(), C.c_double(), C.c_size_t()
        capi.check(capi.load().mhip_contact_op_get_profile(self._h, C.byref(a), C.byref(b), C.byref(n)))
        return a.value, b.value, int(n.value)


def _state(x0, state):
    if state is not None:
        return state
    x = x0.clone()
    return x, torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)


def solve_cqpp(A, q, space, x0, cfg=None, state=None, fused=True, mobility=None):
    """solve_cqpp (convex.hpp:789-797).  A is a ContactOperator (matrix free) or a dense [n, n] tensor.
    Returns (x, grad, SolveResult); `state` = caller-owned (x, grad, x_tmp, grad_tmp) as PGDState holds them.
    mobility: a HydroMobility -- the LCP of a sphere ContactOperator against A = dt D^T M_h D
    (mhip_bbpgd_solve_contact_hydro; A.body_velocity() then holds M_h D x); None: the dry mobility of the operator."""
    cfg = cfg or PGDConfig()
    if mobility is not None:
        if not isinstance(mobility, HydroMobility):
            raise ValueError("mobility must be a HydroMobility, got %r" % (mobility,))
        if not isinstance(A, ContactOperator):
            raise ValueError("a hydrodynamic mobility needs a ContactOperator, not a dense matrix")
        if not fused:
            raise ValueError("a hydrodynamic mobility has the fused driver only")
        if int(space[0]) != SPACE_LOWER_BOUND or float(space[1]) != 0.0:
            raise ValueError("the hydrodynamic solve is an LCP: the space must be LowerBound{0}, got %r" % (space,))
        mobility.check_operator(A)
        x, g, x_tmp, g_tmp = _state(x0, state)
        res, sp, pc = capi.SolveResult(), _space(space), _cfg(cfg)
        capi.check(capi.load().mhip_bbpgd_solve_contact_hydro(
            A._h, C.byref(mobility.struct), _ptr(q), C.byref(sp), C.byref(pc), _ptr(x), _ptr(g), _ptr(x_tmp),
            _ptr(g_tmp), C.byref(res), _stream()))
        return x, g, SolveResult(int(res.num_iters), float(res.residual), bool(res.converged))
    x, g, x_tmp, g_tmp = _state(x0, state)
    res, sp, pc = capi.SolveResult(), _space(space), _cfg(cfg)
    lib = capi.load()
    if isinstance(A, ContactOperator):
        fn = lib.mhip_bbpgd_solve_contact if fused else lib.mhip_bbpgd_solve_contact_unfused
        capi.check(fn(A._h, _ptr(q), C.byref(sp), C.byref(pc), _ptr(x), _ptr(g), _ptr(x_tmp), _ptr(g_tmp),
                      C.byref(res), _stream()))
    else:
        n = q.shape[0]
        if A.dim() != 2 or A.shape[0] != n or A.shape[1] != n:
            raise ValueError("gemv: dimension mismatch A vs x")  # convex.hpp:171-172
        capi.check(lib.mhip_bbpgd_solve_dense(n, _ptr(A), _ptr(q), C.byref(sp), C.byref(pc), _ptr(x), _ptr(g),
                                              _ptr(x_tmp), _ptr(g_tmp), C.byref(res), _stream()))
    return x, g, SolveResult(int(res.num_iters), float(res.residual), bool(res.converged))


def solve_friction_contact(A, sep, mu, p0=None, cfg=None, method="bbpgd"):
    """BUILD EXTENSION, parity unpinned (the reference has no frictional solver): Coulomb friction as a
    cone complementarity problem on the vector-arm ContactOperator A (lever arms to the contact points ON THE
    SURFACES), solved by the fused BBPGD iteration with a per-contact cone projection.  Returns (p [C,3] world-frame
    impulses, g [C,3], SolveResult); mu = 0 reproduces the frictionless LCP (p = lambda n)."""
    cfg = cfg or PGDConfig()
    c = sep.shape[0]
    p = torch.zeros((c, 3), dtype=torch.float64, device=sep.device) if p0 is None else p0.clone()
    g = torch.empty_like(p)
    res, pc = capi.SolveResult(), _cfg(cfg)
    if method not in ("bbpgd", "apgd"):   # "apgd": Mazhar et al. 2015, one operator application per sweep
        raise ValueError("method must be 'bbpgd' or 'apgd'")
    fn = capi.load().mhip_bbpgd_solve_contact_friction if method == "bbpgd" else capi.load().mhip_apgd_solve_contact_friction
    capi.check(fn(A._h, _ptr(sep), float(mu), C.byref(pc), _ptr(p, cols=3), _ptr(g, cols=3), C.byref(res), _stream()))
    return p, g, SolveResult(int(res.num_iters), float(res.residual), bool(res.converged))


def surface_lever_arms(pairs, normal, ra, rb, radius):
    """lever arms to the contact points on the surfaces of two round-capped bodies (spheres, spherocylinders) from
    the centreline arms: ra + r_i n, rb - r_j n.  Friction acts there; for a frictionless contact the difference is
    parallel to the force and drops out of the torque."""
    ri = radius[pairs[:, 0].long()][:, None]
    rj = radius[pairs[:, 1].long()][:, None]
    return (ra + ri * normal).contiguous(), (rb - rj * normal).contiguous()


def solve_small_cqpp_batch(A, q, space, x0, cfg=None):
    """make_mundy_math_cqpp + solve_cqpp on a batch of small dense problems, one thread each (convex.hpp:288-350,
    :722-733).  A [b, n, n], q [b, n], x0 [b, n]; returns (x, grad, num_iters, residual, converged) device tensors."""
    cfg = cfg or PGDConfig()
    b, n = q.shape
    if A.shape != (b, n, n):
        raise ValueError("A must be [batch, n, n]")
    x = x0.clone()
    g = torch.empty_like(x)
    it = torch.empty(b, dtype=torch.int32, device=q.device)
    res = torch.empty(b, dtype=torch.float64, device=q.device)
    conv = torch.empty(b, dtype=torch.int32, device=q.device)
    sp, pc = _space(space), _cfg(cfg)
    capi.check(capi.load().mhip_solve_small_cqpp_batch(b, n, _ptr(A), _ptr(q), C.byref(sp), C.byref(pc), _ptr(x),
                                                       _ptr(g), _ptr(it, torch.int32), _ptr(res),
                                                       _ptr(conv, torch.int32), _stream()))
    return x, g, it, res, conv.bool()


@dataclass
class CollisionResult:  # scrap/lcp_spheres/NgpLcp.cpp:550-554
    max_abs_projected_sep: float = 0.0
    ite_count: int = 0
    max_displacement: float = 0.0


def resolve_collisions(op, sep, lam, dt, max_allowable_overlap=1e-5, max_col_iterations=10000):
    """The scrap app's own BBPGD (resolve_collisions, NgpLcp.cpp:558-759) on a ContactOperator.  `lam` is the initial
    guess and receives the multipliers.  Returns (lam, g = sep + dt*sep_dot, CollisionResult)."""
    lam_tmp, g, g_tmp = torch.empty_like(lam), torch.empty_like(lam), torch.empty_like(lam)
    res, spd = capi.SolveResult(), C.c_double(0.0)
    capi.check(capi.load().mhip_scrap_bbpgd_solve_contact(
        op._h, _ptr(sep), float(max_allowable_overlap), int(max_col_iterations), _ptr(lam), _ptr(lam_tmp), _ptr(g),
        _ptr(g_tmp), C.byref(res), C.byref(spd), _stream()))
    return lam, g, CollisionResult(float(res.residual), int(res.num_iters), float(spd.value) * float(dt))


def solve_lcp(A, q, x0, cfg=None, state=None, fused=True, mobility=None):
    """solve_lcp (convex.hpp:839-845): 0 <= A x + q  _|_  x >= 0.  mobility: see solve_cqpp."""
    return solve_cqpp(A, q, LCP_SPACE, x0, cfg, state, fused, mobility)


# ---- reordering / integration -----------------------------------------------------------------------------------------
def morton_order(center, lo, cell_size):
    n = center.shape[0]
    perm = torch.empty(n, dtype=torch.int32, device=center.device)
    lop = (C.c_double * 3)(*[float(v) for v in lo])
    capi.check(capi.load().mhip_morton_order(n, _ptr(center, cols=3), lop, float(cell_size), _ptr(perm, torch.int32),
                                             _stream()))
    return perm


def curve_order(center, lo, hi, level, key_table):
    """permutation along a lattice curve given by key_table [2^level]^3 (device int32), e.g. the Hilbert table of
    mundy_amd.distributed.hilbert_key_table; ties by index"""
    n = center.shape[0]
    perm = torch.empty(n, dtype=torch.int32, device=center.device)
    lop = (C.c_double * 3)(*[float(v) for v in lo])
    hip = (C.c_double * 3)(*[float(v) for v in hi])
    capi.check(capi.load().mhip_curve_order(n, _ptr(center, cols=3), lop, hip, int(level),
                                            _ptr(key_table.reshape(-1), torch.int32), _ptr(perm, torch.int32), _stream()))
    return perm


def curve_keys(center, lo, hi, level, key_table):
    """key_table entry of every body's cell (int32 tensor): what curve_order sorts by"""
    n = center.shape[0]
    keys = torch.empty(n, dtype=torch.int32, device=center.device)
    lop = (C.c_double * 3)(*[float(v) for v in lo])
    hip = (C.c_double * 3)(*[float(v) for v in hi])
    capi.check(capi.load().mhip_curve_keys(n, _ptr(center, cols=3), lop, hip, int(level),
                                           _ptr(key_table.reshape(-1), torch.int32), _ptr(keys, torch.int32), _stream()))
    return keys


def hilbert_key_table(level):
    """table[ix, iy, iz] = position of the lattice cell along mundy::math::hilbert_3d (Hilbert.hpp:48-83): the library's
    own generator (host code, needs no GPU); numpy int32 array of shape (2^level,) * 3"""
    n = 1 << int(level)
    table = np.empty((n, n, n), dtype=np.int32)
    capi.check(capi.load().mhip_hilbert_key_table(int(level), C.c_void_p(table.ctypes.data)))
    return table


def sort_by_key(keys):
    """stable ascending order of unsigned 64-bit keys (int64 bit pattern: a negative int64 sorts after every
    non-negative one): int32 permutation (library radix sort)"""
    perm = torch.empty(keys.shape[0], dtype=torch.int32, device=keys.device)
    capi.check(capi.load().mhip_sort_by_key_u64(keys.shape[0], _ptr(keys, torch.int64), _ptr(perm, torch.int32), _stream()))
    return perm


def select_contacts(sep, cutoff):
    """BUILD OPTION: ascending indices (int32) of the candidate pairs whose signed separation is not above `cutoff`
    (NaN kept) -- wavefront ballot / prefix-sum compaction (mhip_select_contacts)"""
    kept = torch.empty(sep.shape[0], dtype=torch.int32, device=sep.device)
    cnt = C.c_size_t(0)
    capi.check(capi.load().mhip_select_contacts(sep.shape[0], _ptr(sep), float(cutoff), _ptr(kept, torch.int32),
                                                C.byref(cnt), _stream()))
    return kept[:int(cnt.value)]


# ---- growth and division of spherocylinders (Bacteria.cpp:905-966, :685-748) -------------------------------------------
def select_dividing(length, division_length):
    """divide_bacteria's mark + partial_sum (mhip_select_dividing): (parent_of, num_born) -- int32 ascending indices of
    the bodies with length > division_length (strict; NaN never divides); birth k becomes row n + k"""
    D = _finite_nonneg(division_length, "division_length")
    parent_of = torch.empty(length.shape[0], dtype=torch.int32, device=length.device)
    cnt = C.c_size_t(0)
    capi.check(capi.load().mhip_select_dividing(length.shape[0], _ptr(length, name="length"), D,
                                                _ptr(parent_of, torch.int32), C.byref(cnt), _stream()))
    nb = int(cnt.value)
    return parent_of[:nb], nb


def divide_grow_spherocylinders(n, parent_of, dt, growth_rate, center, quat, radius, length, box=None):
    """subdivide_spherocylinders + grow_bacteria in place (mhip_divide_grow_spherocylinders): the first n rows are the
    bodies before the step, parent_of [nb] the ascending list of select_dividing; rows [n, n + nb) receive the children.
    Every array must hold at least n + nb rows; rows beyond are untouched.  box: 3 edge lengths of [0, L) or None."""
    dt = _finite_nonneg(dt, "dt")
    rate = _finite_nonneg(growth_rate, "growth_rate")
    n, nb = int(n), int(parent_of.shape[0])
    for name, t in (("center", center), ("quat", quat), ("radius", radius), ("length", length)):
        if t.shape[0] < n + nb:
            raise ValueError("%s holds %d rows, the step needs n + births = %d" % (name, t.shape[0], n + nb))
    b = None
    if box is not None:
        tri, b = _cell(box)
        if tri:
            raise ValueError("growth takes an orthorhombic box (3 edge lengths)")
    capi.check(capi.load().mhip_divide_grow_spherocylinders(
        n, nb, _ptr(parent_of, torch.int32, name="parent_of"), dt, rate, b, _ptr(center, cols=3, name="center"),
        _ptr(quat, cols=4, name="quat"), _ptr(radius, name="radius"), _ptr(length, name="length"), _stream()))


def copy_parent_rows(parent_of, n, buf):
    """rows [n, n + nb) of buf = rows parent_of of buf: every per-body field the parent hands to its child
    (mhip_gather_rows on the same float64 storage, bits copied)"""
    nb = int(parent_of.shape[0])
    if nb == 0:
        return buf
    if buf.shape[0] < n + nb:
        raise ValueError("buf holds %d rows, the step needs n + births = %d" % (buf.shape[0], n + nb))
    width = buf[0].numel()
    capi.check(capi.load().mhip_gather_rows(nb, width, _ptr(parent_of, torch.int32, name="parent_of"),
                                            _ptr(buf, name="buf"), _ptr(buf[n:], name="buf"), _stream()))
    return buf


def aabb_moved(aabb, aabb_ref, threshold):
    """check_update_neighbor_list (mhip_aabb_moved): True iff some min or max corner moved by |d|^2 >= threshold^2"""
    thr = _finite_nonneg(threshold, "threshold")
    if tuple(aabb_ref.shape) != tuple(aabb.shape):
        raise ValueError("aabb_ref must have the shape of aabb %s, got %s" % (tuple(aabb.shape), tuple(aabb_ref.shape)))
    flag = C.c_int(0)
    capi.check(capi.load().mhip_aabb_moved(aabb.shape[0], _ptr(aabb, cols=6, name="aabb"),
                                           _ptr(aabb_ref, cols=6, name="aabb_ref"), thr, C.byref(flag), _stream()))
    return bool(flag.value)


def gather_rows(perm, src):
    src2 = src if src.dim() == 2 else src.unsqueeze(1)
    dst = torch.empty((perm.shape[0], src2.shape[1]), dtype=src2.dtype, device=src2.device)
    capi.check(capi.load().mhip_gather_rows(perm.shape[0], src2.shape[1], _ptr(perm, torch.int32), _ptr(src2),
                                            _ptr(dst), _stream()))
    return dst if src.dim() == 2 else dst.squeeze(1)


def periodic_sep(box, p1, p2):
    """metric.sep(p1, p2): PeriodicScaledMetric for 3 edge lengths, PeriodicMetric for a 3x3 unit cell"""
    out = torch.empty_like(p1)
    tri, b = _cell(box)
    fn = capi.load().mhip_periodic_sep_triclinic if tri else capi.load().mhip_periodic_sep
    capi.check(fn(p1.shape[0], b, _ptr(p1, cols=3), _ptr(p2, cols=3), _ptr(out), _stream()))
    return out


def wrap_rigid(box, center):
    """wrap_rigid_inplace of spheres / spherocylinders / ellipsoids: their centres are wrapped into the unit cell"""
    tri, b = _cell(box)
    fn = capi.load().mhip_wrap_rigid_triclinic if tri else capi.load().mhip_wrap_rigid
    capi.check(fn(center.shape[0], b, _ptr(center, cols=3), _stream()))
    return center


def shift_image(cell, p, images):
    """PeriodicMetric::shift_image: p + h * images (images [n, 3] int32)"""
    out = torch.empty_like(p)
    a = _cell(cell)[1] if _cell(cell)[0] else None
    if a is None:  # edge lengths -> diagonal unit cell (periodic_metric_from_unit_cell, periodicity.hpp:848-855)
        e = _cell(cell)[1]
        a = (C.c_double * 9)(e[0], 0, 0, 0, e[1], 0, 0, 0, e[2])
    capi.check(capi.load().mhip_shift_image_triclinic(p.shape[0], a, _ptr(p, cols=3), _ptr(images, torch.int32, 3),
                                                      _ptr(out), _stream()))
    return out


def unit_cell_inverse(cell):
    import numpy as _np
    a = (C.c_double * 9)(*_np.asarray(cell, dtype=_np.float64).reshape(9).tolist())
    out = (C.c_double * 9)()
    capi.check(capi.load().mhip_unit_cell_inverse(a, out))
    return _np.array(list(out)).reshape(3, 3)


def integrate_euler(dt, velocity, center, quat=None):
    capi.check(capi.load().mhip_integrate_euler(center.shape[0], float(dt), _ptr(velocity, cols=6),
                                                _ptr(center, cols=3), _ptr(quat, cols=4, allow_none=True), _stream()))


# ---- bead-spring chains with thermal noise (NgpHP1.cpp:3802-3990, BrownianMotion.cpp, SpringsUpdated.cpp) ------------
SPRING_TYPES = {"hookean": capi.SPRING_HOOKEAN, "fene": capi.SPRING_FENE}
# (the crosslinkers' kinds, which their checks read; a backbone spring set has the Kremer-Grest bond as well)
BACKBONE_SPRING_TYPES = dict(SPRING_TYPES, fenewca=capi.SPRING_FENEWCA)


def _spring_param(value, m, name, positive):
    """a per-spring parameter: a number -> (None, value); an array / tensor [m] -> (host float64 array, 0.0); checked
    here on the host, as the library checks it again before any HIP call"""
    if isinstance(value, (torch.Tensor, np.ndarray, list, tuple)):
        a = np.ascontiguousarray((value.detach().cpu().numpy() if isinstance(value, torch.Tensor) else
                                  np.asarray(value)), dtype=np.float64)
        if a.shape != (m,):
            raise ValueError("%s must be a number or an array of shape [%d], got %s" % (name, m, a.shape))
        vals = a
    else:
        a, vals = None, np.array([float(value)])
    ok = np.isfinite(vals) & ((vals > 0.0) if positive else (vals >= 0.0))
    if not ok.all():
        raise ValueError("%s must be finite and %s 0, got %r" % (name, ">" if positive else ">=",
                                                                 float(vals[~ok][0])))
    return (a, 0.0) if a is not None else (None, float(vals[0]))


def check_springs(pairs, kind, k, r, n):
    """host-side validation of a spring set -> (pairs int32 [m, 2] host, type, k array / None, k0, r array / None, r0)"""
    if kind not in BACKBONE_SPRING_TYPES:
        raise ValueError("spring type must be 'hookean', 'fene' or 'fenewca', got %r" % (kind,))
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2 or not (p.dtype.kind in "iu" or p.size == 0):
        raise ValueError("spring pairs must be integers of shape [m, 2], got %s %s" % (p.dtype, p.shape))
    if p.size and (p.min() < 0 or p.max() >= n):
        raise ValueError("spring pairs: an index outside [0, %d)" % n)
    if p.size and (p[:, 0] == p[:, 1]).any():
        raise ValueError("spring pairs: a spring from a body to itself (spring %d)" % int(np.argmax(p[:, 0] == p[:, 1])))
    m = p.shape[0]
    ka, k0 = _spring_param(k, m, "spring constant k", False)
    fene = kind != "hookean"
    ra, r0 = _spring_param(r, m, "r_max" if fene else "rest length r0", fene)
    return np.ascontiguousarray(p, dtype=np.int32), BACKBONE_SPRING_TYPES[kind], ka, k0, ra, r0


def check_wca(kind, epsilon, sigma):
    """host-side validation of the WCA parameters of a "fenewca" spring set -> (epsilon, sigma)"""
    if kind != "fenewca":
        raise ValueError("WCA epsilon and sigma belong to 'fenewca' springs, not %r" % (kind,))
    _, eps = _spring_param(float(epsilon), 1, "WCA epsilon", True)
    _, sig = _spring_param(float(sigma), 1, "WCA sigma", True)
    return eps, sig


class Springs(_Handle):
    """A spring set between n bodies (mhip_springs_*): kind "hookean" (r = rest length), "fene" or "fenewca" (r = r_max;
    the latter the Kremer-Grest bond of mundy_hip_bending.h, epsilon = sigma = 1 until set_wca); k and r numbers or
    per-spring arrays.  force(center) -> (force [n, 3], overstretched [1] int32, max_length [1] float64), the
    two statistics left on the device.  Every body sums its terms in ascending spring index from +0.0."""
    _destroy = "mhip_springs_destroy"

    def __init__(self, n, pairs, kind, k, r):
        p, t, ka, k0, ra, r0 = check_springs(pairs, kind, k, r, n)
        self.n, self.num_springs, self.kind = int(n), p.shape[0], kind
        self.pairs, self.k, self.r = p, (ka if ka is not None else k0), (ra if ra is not None else r0)
        h = C.c_void_p()
        cp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_springs_create(C.byref(h), self.n, p.shape[0], cp(p), t, cp(ka), k0, cp(ra), r0,
                                                   _stream()))
        self._h = h
        self.wca = (1.0, 1.0) if kind == "fenewca" else None

    def set_wca(self, epsilon, sigma):
        """the WCA part of a "fenewca" set (mhip_springs_set_wca): epsilon, sigma finite and > 0, for every later force"""
        eps, sig = check_wca(self.kind, epsilon, sigma)
        capi.check(capi.load().mhip_springs_set_wca(self._h, eps, sig))
        self.wca = (eps, sig)

    def force(self, center, out=None, stats=None):
        """stats: an optional int32 [1] / float64 [1] pair (overstretched, max_length) to write into"""
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        f = torch.empty((self.n, 3), dtype=torch.float64, device=center.device) if out is None else out
        if stats is None:
            stats = (torch.empty(1, dtype=torch.int32, device=center.device),
                     torch.empty(1, dtype=torch.float64, device=center.device))
        over, mx = stats
        capi.check(capi.load().mhip_springs_force(self._h, _ptr(center, cols=3, name="center"), _ptr(f, name="out"),
                                                  C.c_void_p(over.data_ptr()), C.c_void_p(mx.data_ptr()), _stream()))
        return f, over, mx


def check_angular_springs(n, triplets, k, rest_angle):
    """host-side validation of an angular spring set (no library call) -> (triplets int32 [m, 3] host: end a, end b,
    centre c; k array / None, k0, rest_angle array / None, rest_angle0)"""
    t = triplets.detach().cpu().numpy() if isinstance(triplets, torch.Tensor) else np.asarray(triplets)
    if t.size == 0:
        t = t.reshape(0, 3)
    if t.ndim != 2 or t.shape[1] != 3 or not (t.dtype.kind in "iu" or t.size == 0):
        raise ValueError("angular spring triplets must be integers of shape [m, 3], got %s %s" % (t.dtype, t.shape))
    if t.size and (t.min() < 0 or t.max() >= n):
        raise ValueError("angular spring triplets: an index outside [0, %d)" % n)
    same = (t[:, 0] == t[:, 1]) | (t[:, 0] == t[:, 2]) | (t[:, 1] == t[:, 2])
    if same.any():
        raise ValueError("angular spring triplets: the three bodies of triplet %d are not distinct" % int(np.argmax(same)))
    m = t.shape[0]
    if m >= 2 ** 29:
        raise ValueError("angular spring triplets: %d triplets, the incidence entries hold fewer than 2^29" % m)
    ka, k0 = _spring_param(k, m, "angular spring constant k", False)
    aa, a0 = _spring_param(rest_angle, m, "rest angle", False)
    vals = aa if aa is not None else np.array([a0])
    if (vals > math.pi).any():
        raise ValueError("rest angle must lie in [0, pi], got %r" % float(vals[vals > math.pi][0]))
    return np.ascontiguousarray(t, dtype=np.int32), ka, k0, aa, a0


class AngularSprings(_Handle):
    """m angular springs between n bodies (mhip_angular_springs_*, mundy_hip_bending.h): triplets [m, 3] = (end a, end b,
    centre c), U = 1/2 k (cos(theta) - cos(rest_angle))^2 with theta the angle at c; k and rest_angle numbers or
    per-triplet arrays.  force(center) -> (force [n, 3], degenerate [1] int32, max_deviation [1] float64), the two
    statistics left on the device.  Every body sums its rows in ascending triplet index from +0.0."""
    _destroy = "mhip_angular_springs_destroy"

    def __init__(self, n, triplets, k, rest_angle):
        t, ka, k0, aa, a0 = check_angular_springs(n, triplets, k, rest_angle)
        self.n, self.num_triplets = int(n), t.shape[0]
        h = C.c_void_p()
        cp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_angular_springs_create(C.byref(h), self.n, t.shape[0], cp(t), cp(ka), k0, cp(aa), a0,
                                                           _stream()))
        self._h = h

    def _get(self, what):
        m = self.num_triplets
        out = np.empty((m, 3), dtype=np.int32) if what == 0 else np.empty(m, dtype=np.float64)
        args = [None, None, None]
        args[what] = out.ctypes.data_as(C.c_void_p)
        capi.check(capi.load().mhip_angular_springs_get(self._h, *args))
        return out

    @property
    def triplets(self):
        """int32 [m, 3] host: the triplets as the handle holds them (after any renumbering)"""
        return self._get(0)

    @property
    def k(self):
        return self._get(1)

    @property
    def cos_rest(self):
        """float64 [m] host: the cosines of the rest angles the kernel uses, to the bit"""
        return self._get(2)

    def force(self, center, out=None, accumulate=False, stats=None):
        """written to (or, accumulate=True, added into) out [n, 3]; stats: an optional int32 [1] / float64 [1] pair
        (degenerate, max_deviation) to write into"""
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out")
            out = torch.empty((self.n, 3), dtype=torch.float64, device=center.device)
        if stats is None:
            stats = (torch.empty(1, dtype=torch.int32, device=center.device),
                     torch.empty(1, dtype=torch.float64, device=center.device))
        deg, dev = stats
        capi.check(capi.load().mhip_angular_springs_force(
            self._h, _ptr(center, cols=3, name="center"), _ptr(out, cols=3, name="out"), 1 if accumulate else 0,
            _ptr(deg, torch.int32, name="degenerate"), _ptr(dev, name="max_deviation"), _stream()))
        return out, deg, dev

    def renumber(self, new_of_old):
        """the bodies were permuted: new_of_old int32 [n]"""
        if tuple(new_of_old.shape) != (self.n,):
            raise ValueError("new_of_old must have shape [%d], got %s" % (self.n, tuple(new_of_old.shape)))
        capi.check(capi.load().mhip_angular_springs_renumber(self._h, _ptr(new_of_old, torch.int32, name="new_of_old"),
                                                             _stream()))


def _u64(t, name):
    """int64 tensors carry the u64 keys / counters of the generator (bit patterns)"""
    return _ptr(t, torch.int64, name=name)


def philox4x32_10(keys, counters, block=0):
    """the bare Philox4x32-10 (mhip_philox4x32_10): [count, 4] int32 holding the uint32 words at key (keys lo, hi) and
    counter (counters lo, hi, block, 0); keys / counters are int64 tensors read as u64 bit patterns"""
    b = int(block)
    if not (0 <= b < 2 ** 32):
        raise ValueError("block must be a uint32, got %r" % (block,))
    if keys.shape != counters.shape or keys.dim() != 1:
        raise ValueError("keys and counters must be 1-D of one shape")
    out = torch.empty((keys.shape[0], 4), dtype=torch.int32, device=keys.device)
    capi.check(capi.load().mhip_philox4x32_10(keys.shape[0], _u64(keys, "keys"), _u64(counters, "counters"), b,
                                              _ptr(out, torch.int32), _stream()))
    return out


def brownian_velocity(keys, counters, kt, dt, mob_trans, velocity):
    """velocity[:, :3] += sqrt(2 kt m_t / dt) z with z from Philox blocks 0 and 1 at (key, counter); counters += 1
    (mhip_brownian_velocity).  keys / counters int64 [n] (counters updated in place), velocity [n, 6] in place."""
    kt, dt = float(kt), float(dt)
    if not (kt >= 0.0 and kt < float("inf")):
        raise ValueError("kt must be finite and >= 0, got %r" % kt)
    if not (dt > 0.0 and dt < float("inf")):
        raise ValueError("dt must be finite and > 0, got %r" % dt)
    n = keys.shape[0]
    for name, t in (("counters", counters), ("mob_trans", mob_trans), ("velocity", velocity)):
        if t.shape[0] != n:
            raise ValueError("%s holds %d rows, keys %d" % (name, t.shape[0], n))
    capi.check(capi.load().mhip_brownian_velocity(n, _u64(keys, "keys"), _u64(counters, "counters"), kt, dt,
                                                  _ptr(mob_trans, name="mob_trans"),
                                                  _ptr(velocity, cols=6, name="velocity"), _stream()))
    return velocity


def drag_velocity(mob_trans, force=None, out=None):
    """[n, 6] (m_t F, 0) of a per-body force [n, 3] (None: F = 0) (mhip_drag_velocity)"""
    n = mob_trans.shape[0]
    v = torch.empty((n, 6), dtype=torch.float64, device=mob_trans.device) if out is None else out
    capi.check(capi.load().mhip_drag_velocity(n, _ptr(mob_trans, name="mob_trans"),
                                              _ptr(force, cols=3, allow_none=True, name="force"),
                                              _ptr(v, cols=6, name="out"), _stream()))
    return v


# ---- n-body hydrodynamics as a velocity stage (Periphery.hpp:636-1085; HP1.cpp:3942-4059) ----------------------------
HYDRO_KINDS = {"stokes": capi.HYDRO_STOKES, "rpy": capi.HYDRO_RPY, "rpyc": capi.HYDRO_RPYC}
HYDRO_PATHS = {"auto": capi.HYDRO_PATH_AUTO, "in_lane": capi.HYDRO_PATH_IN_LANE, "partial": capi.HYDRO_PATH_PARTIAL}


def _hydro_kind(kind):
    if kind not in HYDRO_KINDS:
        raise ValueError("hydrodynamics kind must be 'rpyc', 'rpy' or 'stokes', got %r" % (kind,))
    return HYDRO_KINDS[kind]


def check_hydrodynamics(spec, n):
    """hydrodynamics=dict(kind=, radius=None, update_every=1, periphery=None, contact_forces=False, in_solve=False) of
    the stepper -> (kind, radius, update_every); radius None (the beads' own), a number or [n] numbers, finite and >= 0
    -> None or a host array [n]; periphery: checked by check_hydro_periphery; contact_forces and in_solve: bools, which
    the stepper reads"""
    check_dict_spec(spec, "hydrodynamics", ("kind", "radius", "update_every", "periphery", "contact_forces", "in_solve"),
                    optional=("radius", "update_every", "periphery", "contact_forces", "in_solve"))
    for key in ("contact_forces", "in_solve"):
        if not isinstance(spec.get(key, False), bool):
            raise ValueError("hydrodynamics %s must be a bool, got %r" % (key, spec[key]))
    _hydro_kind(spec["kind"])
    if spec.get("periphery") is not None:  # (the stepper takes its checked form from check_hydro_periphery)
        check_hydro_periphery(spec["periphery"])
    radius = spec.get("radius")
    if radius is not None:
        a = radius.detach().cpu().numpy() if isinstance(radius, torch.Tensor) else np.asarray(radius, dtype=np.float64)
        if a.ndim == 0:
            a = np.full(n, float(a))
        if a.shape != (n,):
            raise ValueError("hydrodynamics radius must be a number or have shape [%d], got %s" % (n, a.shape))
        if a.size and not bool(np.all(np.isfinite(a) & (a >= 0.0))):
            raise ValueError("hydrodynamics radius must be finite and >= 0")
        radius = np.ascontiguousarray(a, dtype=np.float64)
    every = spec.get("update_every", 1)
    if isinstance(every, bool) or not isinstance(every, (int, np.integer)) or every < 1:
        raise ValueError("hydrodynamics update_every must be an integer >= 1, got %r" % (every,))
    return spec["kind"], radius, int(every)


class HydroWorkspace(_Handle):
    """mhip_hydro_t: the grow-only buffer of chunk sums a call of hydro_velocity may use; one call at a time"""
    _destroy = "mhip_hydro_destroy"

    def __init__(self):
        h = C.c_void_p()
        capi.check(capi.load().mhip_hydro_create(C.byref(h)))
        self._h = h

    def set_path(self, path="auto"):
        """tests and timing: "in_lane" / "partial" instead of the launch rule's choice ("auto"); the bits are the same"""
        if path not in HYDRO_PATHS:
            raise ValueError("path must be 'auto', 'in_lane' or 'partial'")
        capi.check(capi.load().mhip_hydro_set_path(self._h, HYDRO_PATHS[path]))

    def last_path(self):
        p = C.c_int()
        capi.check(capi.load().mhip_hydro_last_path(self._h, C.byref(p)))
        return {v: k for k, v in HYDRO_PATHS.items()}[p.value]

    def set_sparse_sources(self, on=True):
        """hydro_velocity on this workspace skips the sources whose force is (+-0, +-0, +-0) inside every staged tile
        (mhip_hydro_set_sparse_sources): time only, the bits are the same.  Off by default; the hydrodynamic solve's
        own launches use it whatever this switch says, and leave it alone."""
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError("on must be a bool, got %r" % (on,))
        capi.check(capi.load().mhip_hydro_set_sparse_sources(self._h, 1 if on else 0))


_hydro_default = None


def hydro_velocity(kind, viscosity, src_center, src_radius, src_force, tgt_center=None, tgt_radius=None, out=None,
                   accumulate=False, workspace=None):
    """u_t (+)= sum_s K(x_t - x_s, b_t, a_s) f_s (mhip_hydro_velocity): kind "rpyc" (the accurate one) | "rpy" |
    "stokes"; targets default to the sources (beads to beads; no self term).  out [nt, 3] or [nt, 6] (the first three
    columns are written), default a new [nt, 3]; accumulate adds to what out holds.  Radii may be None for "stokes".
    The sums are taken in the fixed order mundy_hip.h documents (a function of the source count alone)."""
    global _hydro_default
    k = _hydro_kind(kind)
    mu = float(viscosity)
    if not (mu > 0.0 and mu < float("inf")):
        raise ValueError("viscosity must be finite and > 0, got %r" % (viscosity,))
    if tgt_center is None:
        tgt_center, tgt_radius = src_center, src_radius
    ns, nt = src_center.shape[0], tgt_center.shape[0]
    need_r = k != capi.HYDRO_STOKES
    for name, t, rows, cols in (("src_force", src_force, ns, 3), ("src_center", src_center, ns, 3),
                                ("tgt_center", tgt_center, nt, 3)):
        if t.dim() != 2 or tuple(t.shape) != (rows, cols):
            raise ValueError("%s must have shape [%d, %d], got %s" % (name, rows, cols, tuple(t.shape)))
    for name, t, rows in (("src_radius", src_radius, ns), ("tgt_radius", tgt_radius, nt)):
        if t is None and need_r:
            raise ValueError("%s must not be None for kind %r" % (name, kind))
        if t is not None and tuple(t.shape) != (rows,):
            raise ValueError("%s must have shape [%d], got %s" % (name, rows, tuple(t.shape)))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty((nt, 3), dtype=torch.float64, device=src_center.device)
    if out.dim() != 2 or out.shape[0] != nt or out.shape[1] not in (3, 6):
        raise ValueError("out must have shape [%d, 3] or [%d, 6], got %s" % (nt, nt, tuple(out.shape)))
    if workspace is None:
        if _hydro_default is None:
            _hydro_default = HydroWorkspace()
        workspace = _hydro_default
    capi.check(capi.load().mhip_hydro_velocity(
        workspace._h, k, mu, ns, _ptr(src_center, name="src_center"),
        _ptr(src_radius, name="src_radius", allow_none=True), _ptr(src_force, name="src_force"), nt,
        _ptr(tgt_center, name="tgt_center"), _ptr(tgt_radius, name="tgt_radius", allow_none=True),
        _ptr(out, name="out"), int(out.shape[1]), 1 if accumulate else 0, _stream()))
    return out


def hydro_add_velocity(u_hydro, velocity):
    """velocity[:, :3] += u_hydro (mhip_hydro_add_velocity): u_hydro [n, 3], velocity [n, 3] or [n, 6], in place"""
    n = u_hydro.shape[0]
    if velocity.dim() != 2 or velocity.shape[0] != n or velocity.shape[1] not in (3, 6):
        raise ValueError("velocity must have shape [%d, 3] or [%d, 6], got %s" % (n, n, tuple(velocity.shape)))
    capi.check(capi.load().mhip_hydro_add_velocity(n, _ptr(u_hydro, cols=3, name="u_hydro"),
                                                   _ptr(velocity, name="velocity"), int(velocity.shape[1]), _stream()))
    return velocity


# ---- the periphery's no-slip correction of the hydrodynamics (mundy_hip_hydro_periphery.h; HP1.cpp:4005-4037) -----------
HYDRO_PERIPHERY_STATES = {capi.HYDRO_PERIPHERY_EMPTY: "empty", capi.HYDRO_PERIPHERY_MATRIX: "matrix",
                          capi.HYDRO_PERIPHERY_INVERSE: "inverse", capi.HYDRO_PERIPHERY_DOUBLE_LAYER: "double_layer"}
_HYDRO_PERIPHERY_KEYS = ("shape", "radius", "spectral_order", "points", "weights", "normals", "inverse",
                         "skip_same_index")


def _host_f64(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a, dtype=np.float64)


def check_hydro_periphery(spec):
    """periphery= of hydrodynamics=: dict(shape="sphere", radius=, spectral_order=) or dict(points=, weights=, normals=),
    with optional inverse= ([3S, 3S], a precomputed Minv) and skip_same_index=True (the reference's quirk)
    -> dict(points [S, 3], weights [S], normals [S, 3], inverse or None, skip_same_index), host arrays; no library call"""
    check_dict_spec(spec, "hydrodynamics periphery", _HYDRO_PERIPHERY_KEYS, optional=_HYDRO_PERIPHERY_KEYS)
    if "shape" in spec:
        if spec["shape"] != "sphere":
            raise ValueError("hydrodynamics periphery shape must be 'sphere' (or pass points, weights, normals), got %r"
                             % (spec["shape"],))
        for k in ("points", "weights", "normals"):
            if k in spec:
                raise ValueError("hydrodynamics periphery takes shape= or points=, weights=, normals=, not both")
        for k in ("radius", "spectral_order"):
            if k not in spec:
                raise ValueError("hydrodynamics periphery shape='sphere' is missing key %r" % k)
        radius, order = spec["radius"], spec["spectral_order"]
        if isinstance(radius, bool) or not isinstance(radius, (int, float, np.integer, np.floating)) or \
                not (float(radius) > 0.0 and float(radius) < float("inf")):
            raise ValueError("hydrodynamics periphery radius must be finite and > 0, got %r" % (radius,))
        if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or order < 1:
            raise ValueError("hydrodynamics periphery spectral_order must be an integer >= 1, got %r" % (order,))
        from . import synth
        points, weights, normals = synth.sphere_quadrature(int(order), float(radius), include_poles=False, invert=True)
    else:
        for k in ("points", "weights", "normals"):
            if k not in spec:
                raise ValueError("hydrodynamics periphery is missing key %r (or pass shape='sphere')" % k)
        for k in ("radius", "spectral_order"):
            if k in spec:
                raise ValueError("hydrodynamics periphery %s belongs to shape='sphere'" % k)
        points, weights, normals = (_host_f64(spec[k]) for k in ("points", "weights", "normals"))
        S = points.shape[0]
        if points.ndim != 2 or points.shape[1] != 3 or S == 0:
            raise ValueError("hydrodynamics periphery points must have shape [S, 3] with S >= 1, got %s" % (points.shape,))
        if weights.shape != (S,) or normals.shape != (S, 3):
            raise ValueError("hydrodynamics periphery weights / normals must have shapes [%d] / [%d, 3], got %s / %s"
                             % (S, S, weights.shape, normals.shape))
        if not bool(np.all(np.isfinite(points)) and np.all(np.isfinite(weights)) and np.all(np.isfinite(normals))):
            raise ValueError("hydrodynamics periphery points, weights and normals must be finite")
    S = points.shape[0]
    if 3 * S > 65535:
        raise ValueError("hydrodynamics periphery has too many surface nodes: 3 S = %d > 65535" % (3 * S))
    inverse = spec.get("inverse")
    if inverse is not None:
        shape = tuple(inverse.shape) if hasattr(inverse, "shape") else np.shape(inverse)
        if shape != (3 * S, 3 * S):
            raise ValueError("hydrodynamics periphery inverse must have shape [%d, %d], got %s" % (3 * S, 3 * S, shape))
    skip = spec.get("skip_same_index", True)
    if not isinstance(skip, (bool, np.bool_)):
        raise ValueError("hydrodynamics periphery skip_same_index must be True or False, got %r" % (skip,))
    return dict(points=points, weights=weights, normals=normals, inverse=inverse, skip_same_index=bool(skip))


class HydroPeriphery(_Handle):
    """mhip_hydro_periphery_t: the surface (points [S, 3], weights [S], inward normals [S, 3]; device tensors, copied),
    its boundary-integral matrix M and the inverse, in ONE [3S, 3S] buffer (`state`: which of the two it holds), and the
    surface velocity and density of the correction.  fill_matrix() / set_matrix(M) -> invert() (returns the smallest
    pivot magnitude; synchronises) or set_inverse(Minv) -> surface_forces(u) / correct(...)."""
    _destroy = "mhip_hydro_periphery_destroy"

    def __init__(self, points, weights, normals, viscosity):
        S = points.shape[0]
        if points.dim() != 2 or points.shape[1] != 3 or S == 0:
            raise ValueError("points must have shape [S, 3] with S >= 1, got %s" % (tuple(points.shape),))
        if tuple(weights.shape) != (S,) or tuple(normals.shape) != (S, 3):
            raise ValueError("weights / normals must have shapes [%d] / [%d, 3]" % (S, S))
        mu = float(viscosity)
        if not (mu > 0.0 and mu < float("inf")):
            raise ValueError("viscosity must be finite and > 0, got %r" % (viscosity,))
        self.num_nodes, self.n, self.viscosity, self.device = S, 3 * S, mu, points.device
        h = C.c_void_p()
        capi.check(capi.load().mhip_hydro_periphery_create(C.byref(h), S, _ptr(points, name="points"),
                                                           _ptr(weights, name="weights"),
                                                           _ptr(normals, name="normals"), mu, _stream()))
        self._h = h

    def fill_double_layer(self):
        """tests: the double-layer block T alone (state "double_layer")"""
        capi.check(capi.load().mhip_hydro_periphery_fill_double_layer(self._h, _stream()))
        return self

    def fill_matrix(self):
        capi.check(capi.load().mhip_hydro_periphery_fill_matrix(self._h, _stream()))
        return self

    def _square(self, m, name):
        if tuple(m.shape) != (self.n, self.n):
            raise ValueError("%s must have shape [%d, %d], got %s" % (name, self.n, self.n, tuple(m.shape)))
        return _ptr(m, name=name)

    def set_matrix(self, matrix):
        capi.check(capi.load().mhip_hydro_periphery_set_matrix(self._h, self._square(matrix, "matrix"), _stream()))
        return self

    def set_inverse(self, inverse):
        capi.check(capi.load().mhip_hydro_periphery_set_inverse(self._h, self._square(inverse, "inverse"), _stream()))
        return self

    def invert(self):
        """M -> Minv in place; -> the smallest pivot magnitude (a host number: synchronises)"""
        m = C.c_double()
        capi.check(capi.load().mhip_hydro_periphery_invert(self._h, C.byref(m), _stream()))
        return m.value

    @property
    def state(self):
        return self._matrix()[1]

    def _matrix(self):
        p, st = C.c_void_p(), C.c_int()
        capi.check(capi.load().mhip_hydro_periphery_matrix(self._h, C.byref(p), C.byref(st)))
        return p.value, HYDRO_PERIPHERY_STATES[st.value]

    def matrix(self):
        """a copy [3S, 3S] of what the buffer holds (M, Minv or T), made on the current stream"""
        p, st = self._matrix()
        if st == "empty":
            raise AssertionError("the periphery holds no matrix")
        out = torch.empty((self.n, self.n), dtype=torch.float64, device=self.device)
        capi.check(capi.load().mhip_deep_copy(self.n * self.n, _ptr(out), C.c_void_p(p), _stream()))
        return out

    def surface_forces(self, u_surf, out=None):
        """f_surf = -(Minv u_surf), [3S] or [S, 3]"""
        if u_surf.numel() != self.n:
            raise ValueError("u_surf must hold %d numbers, got %d" % (self.n, u_surf.numel()))
        if out is None:
            out = torch.empty_like(u_surf)
        if out.numel() != self.n:
            raise ValueError("out must hold %d numbers, got %d" % (self.n, out.numel()))
        capi.check(capi.load().mhip_hydro_periphery_surface_forces(self._h, _ptr(u_surf, name="u_surf"),
                                                                   _ptr(out, name="out"), _stream()))
        return out

    def correct(self, kind, center, radius, force, velocity, skip_same_index=True, workspace=None):
        """velocity[:, :3] += DL(nodes -> beads)(-(Minv K(beads -> nodes) force)) (mhip_hydro_periphery_correct)"""
        global _hydro_default
        k = _hydro_kind(kind)
        n = center.shape[0]
        for name, t in (("center", center), ("force", force)):
            if t.dim() != 2 or tuple(t.shape) != (n, 3):
                raise ValueError("%s must have shape [%d, 3], got %s" % (name, n, tuple(t.shape)))
        if radius is None and k != capi.HYDRO_STOKES:
            raise ValueError("radius must not be None for kind %r" % (kind,))
        if radius is not None and tuple(radius.shape) != (n,):
            raise ValueError("radius must have shape [%d], got %s" % (n, tuple(radius.shape)))
        if velocity.dim() != 2 or velocity.shape[0] != n or velocity.shape[1] not in (3, 6):
            raise ValueError("velocity must have shape [%d, 3] or [%d, 6], got %s" % (n, n, tuple(velocity.shape)))
        if workspace is None:
            if _hydro_default is None:
                _hydro_default = HydroWorkspace()
            workspace = _hydro_default
        capi.check(capi.load().mhip_hydro_periphery_correct(
            self._h, workspace._h, k, n, _ptr(center, name="center"), _ptr(radius, name="radius", allow_none=True),
            _ptr(force, name="force"), _ptr(velocity, name="velocity"), int(velocity.shape[1]),
            1 if skip_same_index else 0, _stream()))
        return velocity


class HydroMobility:
    """mhip_hydro_mobility (include/mundy_hip_hydro_solve.h): the long-range part of M_h = m_t + hydro_kind (+ the
    periphery's no-slip correction) for ContactOperator.apply_hydro and solve_lcp(..., mobility=).  kind "rpyc" | "rpy"
    (the Stokeslet is not positive semi-definite at bead separations); center [n, 3] and the hydrodynamic radius [n] are
    device tensors this object keeps alive and the library reads at every call (update them in place, or build a new
    one); periphery: a HydroPeriphery holding its inverse, built with the same viscosity; workspace: a HydroWorkspace
    (default: the module's; one call at a time, as for hydro_velocity)."""

    def __init__(self, kind, viscosity, center, radius, periphery=None, skip_same_index=True, workspace=None):
        global _hydro_default
        k = _hydro_kind(kind)
        if k == capi.HYDRO_STOKES:
            raise ValueError("the Stokeslet is not positive semi-definite at bead separations: kind must be 'rpyc' or "
                             "'rpy'")
        mu = float(viscosity)
        if not (mu > 0.0 and mu < float("inf")):
            raise ValueError("viscosity must be finite and > 0, got %r" % (viscosity,))
        if center.dim() != 2 or center.shape[1] != 3:
            raise ValueError("center must have shape [n, 3], got %s" % (tuple(center.shape),))
        n = center.shape[0]
        if tuple(radius.shape) != (n,):
            raise ValueError("radius must have shape [%d], got %s" % (n, tuple(radius.shape)))
        if periphery is not None and not isinstance(periphery, HydroPeriphery):
            raise ValueError("periphery must be a HydroPeriphery, got %r" % (periphery,))
        if periphery is not None and periphery.viscosity != mu:  # (its correction uses the handle's own)
            raise ValueError("the periphery was built with viscosity %r, the mobility has %r" % (periphery.viscosity, mu))
        if not isinstance(skip_same_index, (bool, np.bool_)):
            raise ValueError("skip_same_index must be a bool, got %r" % (skip_same_index,))
        if workspace is not None and not isinstance(workspace, HydroWorkspace):
            raise ValueError("workspace must be a HydroWorkspace, got %r" % (workspace,))
        cp, rp = _ptr(center, name="center"), _ptr(radius, name="radius")
        if workspace is None:
            if _hydro_default is None:
                _hydro_default = HydroWorkspace()
            workspace = _hydro_default
        self.kind, self.viscosity, self.num_bodies = kind, mu, n
        self.center, self.radius, self.periphery, self.workspace = center, radius, periphery, workspace
        self.skip_same_index = bool(skip_same_index)
        self.struct = capi.HydroMobility(workspace._h, k, mu, n, cp, rp, periphery._h if periphery is not None else None,
                                         1 if skip_same_index else 0)

    def check_operator(self, op):
        """what the library refuses of the pair (operator, mobility), refused here before it is called"""
        _, _, ra, rb, _, mob_rot, rod, _ = op._keep
        if ra is not None or rb is not None or mob_rot is not None or rod is not None:
            raise ValueError("the hydrodynamic mobility needs a sphere operator: no lever arms, rods or mob_rot")
        if op.num_bodies != self.num_bodies:
            raise ValueError("the mobility has %d bodies, the operator %d" % (self.num_bodies, op.num_bodies))


def hydro_double_layer(viscosity, center, normal, weight, force, tgt_center, out=None, accumulate=False,
                       skip_same_index=True, workspace=None):
    """u_t (+)= sum_s DL(x_t - y_s; n_s, w_s, f_s) (mhip_hydro_double_layer): the Stokes double layer of the surface
    nodes (center, normal [ns, 3], weight [ns], force [ns, 3]) at the targets [nt, 3]; out [nt, 3] or [nt, 6], default
    a new [nt, 3].  skip_same_index (the reference's quirk): the term of source t onto target t is skipped.  The sums
    are those of hydro_velocity."""
    global _hydro_default
    mu = float(viscosity)
    if not (mu > 0.0 and mu < float("inf")):
        raise ValueError("viscosity must be finite and > 0, got %r" % (viscosity,))
    ns, nt = center.shape[0], tgt_center.shape[0]
    for name, t, rows in (("center", center, ns), ("normal", normal, ns), ("force", force, ns),
                          ("tgt_center", tgt_center, nt)):
        if t.dim() != 2 or tuple(t.shape) != (rows, 3):
            raise ValueError("%s must have shape [%d, 3], got %s" % (name, rows, tuple(t.shape)))
    if tuple(weight.shape) != (ns,):
        raise ValueError("weight must have shape [%d], got %s" % (ns, tuple(weight.shape)))
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs out")
        out = torch.empty((nt, 3), dtype=torch.float64, device=center.device)
    if out.dim() != 2 or out.shape[0] != nt or out.shape[1] not in (3, 6):
        raise ValueError("out must have shape [%d, 3] or [%d, 6], got %s" % (nt, nt, tuple(out.shape)))
    if workspace is None:
        if _hydro_default is None:
            _hydro_default = HydroWorkspace()
        workspace = _hydro_default
    capi.check(capi.load().mhip_hydro_double_layer(
        workspace._h, mu, ns, _ptr(center, name="center"), _ptr(normal, name="normal"), _ptr(weight, name="weight"),
        _ptr(force, name="force"), nt, _ptr(tgt_center, name="tgt_center"), _ptr(out, name="out"), int(out.shape[1]),
        1 if accumulate else 0, 1 if skip_same_index else 0, _stream()))
    return out


# ---- crosslinkers that bind and unbind (HP1.cpp:3264-3748, :4728-4739) ------------------------------------------------
def check_crosslinkers(n, left, right, sites, kind, k, r, bind_rate, unbind_rate, kt, capture_radius,
                       num_periphery_sites=0):
    """host-side validation of a crosslinker set (no library call) -> (left int32 [m], right int32 [m], sites uint8
    [n], type, k, r, bind_rate, unbind_rate, kt, capture_radius).  num_periphery_sites = P > 0: right may also hold
    -(s + 1), s in [0, P): bound to periphery site s"""

    def host(a):
        return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)

    if kind == "fenewca":
        raise ValueError("crosslinkers take no 'fenewca' springs: the reference's binding rates have no FENE-WCA branch")
    if kind not in SPRING_TYPES:
        raise ValueError("crosslinker spring type must be 'hookean' or 'fene', got %r" % (kind,))
    if left is None:
        raise ValueError("crosslinkers need left: the body of every fixed left head")
    le = host(left)
    if le.ndim != 1 or not (le.dtype.kind in "iu" or le.size == 0):
        raise ValueError("crosslinker left must be integers of shape [m], got %s %s" % (le.dtype, le.shape))
    m = le.shape[0]
    if le.size and (le.min() < 0 or le.max() >= n):
        raise ValueError("crosslinker left: an index outside [0, %d)" % n)
    if sites is None:
        raise ValueError("crosslinkers need sites: a byte mask [n] of the bodies a right head may bind to")
    si = host(sites)
    if si.shape != (n,) or si.dtype.kind not in "biu":
        raise ValueError("crosslinker sites must be a bool / integer mask of shape [%d], got %s %s" % (n, si.dtype,
                                                                                                    si.shape))
    if si.size and (si.min() < 0 or si.max() > 1):
        raise ValueError("crosslinker sites must hold 0 / 1 only")
    si = np.ascontiguousarray(si, dtype=np.uint8)
    if right is None:
        ri = le.copy()
    else:
        ri = host(right)
        if ri.shape != (m,) or not (ri.dtype.kind in "iu" or ri.size == 0):
            raise ValueError("crosslinker right must be integers of shape [%d], got %s %s" % (m, ri.dtype, ri.shape))
        if ri.size and (ri.min() < -int(num_periphery_sites) or ri.max() >= n):
            raise ValueError("crosslinker right: an index outside [0, %d)" % n if not num_periphery_sites else
                             "crosslinker right: an index outside [0, %d) and no periphery site -(s + 1), s in [0, %d)"
                             % (n, num_periphery_sites))
        bad = (ri != le) & (ri >= 0) & (si[np.maximum(ri, 0)] == 0)
        if bad.any():
            c = int(np.argmax(bad))
            raise ValueError("crosslinker %d: right head at body %d, which is not a bind site" % (c, int(ri[c])))
    fene = kind == "fene"
    _, k0 = _spring_param(float(k), m, "crosslinker spring constant k", False)
    _, r0 = _spring_param(float(r), m, "crosslinker r_max" if fene else "crosslinker rest length r0", fene)
    _, a0 = _spring_param(float(bind_rate), m, "bind_rate", False)
    _, off = _spring_param(float(unbind_rate), m, "unbind_rate", False)
    _, kt0 = _spring_param(float(kt), m, "crosslinker kt", True)
    _, cap = _spring_param(float(capture_radius), m, "capture_radius", True)
    return (np.ascontiguousarray(le, dtype=np.int32), np.ascontiguousarray(ri, dtype=np.int32), si, SPRING_TYPES[kind],
            k0, r0, a0, off, kt0, cap)


_PERIPHERY_SITE_KEYS = ("points", "bind_rate", "k", "r", "unbind_rate", "capture_radius")


def check_periphery_sites(spec, kind, unbind_rate, capture_radius):
    """host-side validation of periphery bind sites dict(points= [P, 3], bind_rate=, k=, r=, unbind_rate=None,
    capture_radius=None) for crosslinkers of spring type `kind` (no library call) -> (points float64 [P, 3] host,
    bind_rate, k, r, unbind_rate, capture_radius); unbind_rate and capture_radius default to the crosslinkers' own"""
    check_dict_spec(spec, "periphery_sites", _PERIPHERY_SITE_KEYS, optional=("unbind_rate", "capture_radius"))
    if kind == "fenewca":
        raise ValueError("crosslinkers take no 'fenewca' springs: the reference's binding rates have no FENE-WCA branch")
    if kind not in SPRING_TYPES:
        raise ValueError("crosslinker spring type must be 'hookean' or 'fene', got %r" % (kind,))
    pts = spec["points"]
    pts = pts.detach().cpu().numpy() if isinstance(pts, torch.Tensor) else np.asarray(pts)
    if pts.ndim != 2 or pts.shape[1] != 3 or pts.dtype.kind not in "fiu":
        raise ValueError("periphery_sites points must be numbers of shape [P, 3], got %s %s" % (pts.dtype, pts.shape))
    if pts.shape[0] == 0:
        raise ValueError("periphery_sites points: P must be > 0")
    if pts.shape[0] >= 2 ** 31:
        raise ValueError("periphery_sites points: too many sites for a 32-bit right head")
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    if not np.isfinite(pts).all():
        raise ValueError("periphery_sites points must be finite")
    fene = kind == "fene"
    _, a0 = _spring_param(float(spec["bind_rate"]), 1, "periphery_sites bind_rate", False)
    _, k0 = _spring_param(float(spec["k"]), 1, "periphery_sites spring constant k", False)
    _, r0 = _spring_param(float(spec["r"]), 1, "periphery_sites r_max" if fene else "periphery_sites rest length r0",
                          fene)
    off = spec.get("unbind_rate")
    _, off = _spring_param(float(unbind_rate if off is None else off), 1, "periphery_sites unbind_rate", False)
    cap = spec.get("capture_radius")
    _, cap = _spring_param(float(capture_radius if cap is None else cap), 1, "periphery_sites capture_radius", True)
    return pts, a0, k0, r0, off, cap


class Crosslinkers(_Handle):
    """m crosslinkers over n bodies (mhip_crosslinkers_*): fixed left heads, right heads that bind to the bodies of the
    `sites` mask and unbind (right == left: singly bound); a doubly bound one is a spring of `kind` / k / r.
    set_candidates(row_ptr, col, ids) -> kmc_step(center, dt, keys, counters) -> force(center)."""
    _destroy = "mhip_crosslinkers_destroy"

    def __init__(self, n, left, right, sites, kind, k, r, bind_rate, unbind_rate, kt, capture_radius):
        le, ri, si, t, k0, r0, a0, off, kt0, cap = check_crosslinkers(n, left, right, sites, kind, k, r, bind_rate,
                                                                       unbind_rate, kt, capture_radius)
        self.n, self.num_crosslinkers, self.kind = int(n), le.shape[0], kind
        self.k, self.r, self.capture_radius, self.unbind_rate = k0, r0, cap, off
        self.num_periphery_sites = 0
        h = C.c_void_p()
        cp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_crosslinkers_create(C.byref(h), self.n, le.shape[0], cp(le), cp(ri), cp(si), t, k0,
                                                        r0, a0, off, kt0, cap, _stream()))
        self._h = h

    def set_candidates(self, row_ptr, col, ids=None):
        """the CSR of a neighbour search over the bodies; every row is sorted by ids[col] (int64 [n]) here, once"""
        if tuple(row_ptr.shape) != (self.n + 1,):
            raise ValueError("row_ptr must have shape [%d], got %s" % (self.n + 1, tuple(row_ptr.shape)))
        if ids is not None and tuple(ids.shape) != (self.n,):
            raise ValueError("ids must have shape [%d], got %s" % (self.n, tuple(ids.shape)))
        capi.check(capi.load().mhip_crosslinkers_set_candidates(
            self._h, _ptr(row_ptr, torch.int32, name="row_ptr"), _ptr(col, torch.int32, name="col"), col.shape[0],
            _ptr(ids, torch.int64, allow_none=True, name="ids"), _stream()))

    def set_periphery_sites(self, points, bind_rate, k, r, unbind_rate=None, capture_radius=None):
        """P immobile bind sites of the periphery (mhip_crosslinkers_set_periphery_sites): points float64 [P, 3] on the
        device, copied; their own bind_rate, k, r, unbind_rate (default: the crosslinkers'), capture_radius (default:
        the crosslinkers').  right == -(s + 1) then means bound to site s.  Again with the same P: the sites move.  The
        periphery candidates are dropped."""
        if points.dim() != 2 or points.shape[1] != 3:
            raise ValueError("points must have shape [P, 3], got %s" % (tuple(points.shape),))
        _, a0, k0, r0, off, cap = check_periphery_sites(
            dict(points=np.zeros((max(points.shape[0], 0), 3)), bind_rate=bind_rate, k=k, r=r, unbind_rate=unbind_rate,
                 capture_radius=capture_radius), self.kind, self.unbind_rate, self.capture_radius)
        if self.num_periphery_sites and points.shape[0] != self.num_periphery_sites:
            raise ValueError("periphery sites: P = %d, but an earlier call set %d sites" % (points.shape[0],
                                                                                         self.num_periphery_sites))
        capi.check(capi.load().mhip_crosslinkers_set_periphery_sites(
            self._h, points.shape[0], _ptr(points, cols=3, name="points"), a0, k0, r0, off, cap, _stream()))
        self.num_periphery_sites = points.shape[0]
        self.periphery_capture_radius = cap

    def set_periphery_candidates(self, row_ptr, col, col_offset=0):
        """the first n rows of a CSR whose columns are site index + col_offset (a neighbour search over beads followed
        by sites: col_offset = n; row_ptr may be longer than n + 1); every row is sorted by site index here, once"""
        if row_ptr.dim() != 1 or row_ptr.shape[0] < self.n + 1:
            raise ValueError("row_ptr must hold at least %d entries, got %s" % (self.n + 1, tuple(row_ptr.shape)))
        off = int(col_offset)
        if not (0 <= off < 2 ** 31):
            raise ValueError("col_offset must be in [0, 2^31), got %r" % (col_offset,))
        capi.check(capi.load().mhip_crosslinkers_set_periphery_candidates(
            self._h, _ptr(row_ptr, torch.int32, name="row_ptr"), _ptr(col, torch.int32, name="col"), col.shape[0], off,
            _stream()))

    def kmc_step(self, center, dt, keys, counters, events=None, z_total=None, periphery_bound=None):
        """one KMC step at `center`; counters += 1; -> events int32 [2] = (binds, unbinds), left on the device;
        z_total (optional float64 [m]) receives every singly bound crosslinker's total rate x dt; periphery_bound
        (optional int32 [1], needs periphery sites): the number of periphery-bound crosslinkers after the step is added
        to it"""
        m = self.num_crosslinkers
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        if tuple(keys.shape) != (m,) or tuple(counters.shape) != (m,):
            raise ValueError("keys and counters must have shape [%d]" % m)
        if z_total is not None and tuple(z_total.shape) != (m,):
            raise ValueError("z_total must have shape [%d]" % m)
        ev = torch.empty(2, dtype=torch.int32, device=center.device) if events is None else events
        if periphery_bound is not None:
            if tuple(periphery_bound.shape) != (1,):
                raise ValueError("periphery_bound must have shape [1]")
            capi.check(capi.load().mhip_crosslinkers_kmc_step_periphery(
                self._h, _ptr(center, cols=3, name="center"), float(dt), _u64(keys, "keys"), _u64(counters, "counters"),
                _ptr(ev, torch.int32, name="events"), _ptr(periphery_bound, torch.int32, name="periphery_bound"),
                _ptr(z_total, allow_none=True, name="z_total"), _stream()))
            return ev
        capi.check(capi.load().mhip_crosslinkers_kmc_step(self._h, _ptr(center, cols=3, name="center"), float(dt),
                                                          _u64(keys, "keys"), _u64(counters, "counters"),
                                                          _ptr(ev, torch.int32, name="events"),
                                                          _ptr(z_total, allow_none=True, name="z_total"), _stream()))
        return ev

    def force(self, center, out=None, accumulate=False, stats=None):
        """the doubly bound crosslinkers as springs: written to (or, accumulate=True, added into) out [n, 3];
        stats as Springs.force"""
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out")
            out = torch.empty((self.n, 3), dtype=torch.float64, device=center.device)
        if stats is None:
            stats = (torch.empty(1, dtype=torch.int32, device=center.device),
                     torch.empty(1, dtype=torch.float64, device=center.device))
        over, mx = stats
        capi.check(capi.load().mhip_crosslinkers_force(self._h, _ptr(center, cols=3, name="center"),
                                                       _ptr(out, cols=3, name="out"), 1 if accumulate else 0,
                                                       C.c_void_p(over.data_ptr()), C.c_void_p(mx.data_ptr()),
                                                       _stream()))
        return out, over, mx

    def state(self, device):
        """-> (left, right) int32 [m] device tensors (copies)"""
        le, ri = (torch.empty(self.num_crosslinkers, dtype=torch.int32, device=device) for _ in range(2))
        capi.check(capi.load().mhip_crosslinkers_get_state(self._h, _ptr(le, torch.int32), _ptr(ri, torch.int32),
                                                           _stream()))
        return le, ri

    def set_state(self, left, right):
        """left (None = unchanged) and right int32 [m] device tensors into the handle; indices are not checked"""
        m = self.num_crosslinkers
        for name, t in (("left", left), ("right", right)):
            if t is not None and tuple(t.shape) != (m,):
                raise ValueError("%s must have shape [%d], got %s" % (name, m, tuple(t.shape)))
        capi.check(capi.load().mhip_crosslinkers_set_state(self._h, _ptr(left, torch.int32, allow_none=True, name="left"),
                                                           _ptr(right, torch.int32, name="right"), _stream()))

    def renumber(self, new_of_old):
        """the bodies were permuted: new_of_old int32 [n]; the candidates are dropped"""
        if tuple(new_of_old.shape) != (self.n,):
            raise ValueError("new_of_old must have shape [%d], got %s" % (self.n, tuple(new_of_old.shape)))
        capi.check(capi.load().mhip_crosslinkers_renumber(self._h, _ptr(new_of_old, torch.int32, name="new_of_old"),
                                                          _stream()))


# ---- the nuclear periphery (HP1.cpp:4063-4284, NgpHP1.cpp:2409-2527) ---------------------------------------------------
PERIPHERY_SHAPES = {"sphere": capi.PERIPHERY_SPHERE, "ellipsoid": capi.PERIPHERY_ELLIPSOID,
                    "ellipsoid_fast": capi.PERIPHERY_ELLIPSOID_FAST}
_PERIPHERY_KEYS = ("shape", "radius", "radii", "k", "center", "quat")


def check_periphery(spec):
    """host-side validation of a periphery dict(shape=, radius= or radii=, k=, center=(0, 0, 0), quat=(1, 0, 0, 0)) (no
    library call) -> (shape name, radii (3 floats; a sphere's radius three times), k, center, quat)"""
    check_dict_spec(spec, "periphery", _PERIPHERY_KEYS, optional=("radius", "radii", "center", "quat"))
    shape = spec["shape"]
    if shape not in PERIPHERY_SHAPES:
        raise ValueError("periphery shape must be 'sphere', 'ellipsoid' or 'ellipsoid_fast', got %r" % (shape,))
    want, other = ("radius", "radii") if shape == "sphere" else ("radii", "radius")
    if want not in spec:
        raise ValueError("periphery: missing key(s) %s" % want)
    if other in spec:
        raise ValueError("periphery: shape %r takes %s, not %s" % (shape, want, other))

    def floats(v, count, name):
        try:
            a = [float(x) for x in (v.tolist() if hasattr(v, "tolist") else v)]
        except TypeError:
            a = None
        if a is None or len(a) != count:
            raise ValueError("periphery %s must be %d numbers, got %r" % (name, count, v))
        if not all(math.isfinite(x) for x in a):
            raise ValueError("periphery %s must be finite, got %r" % (name, a))
        return a
    radii = floats([spec["radius"]] * 3, 3, "radius") if shape == "sphere" else floats(spec["radii"], 3, "radii")
    if not all(x > 0.0 for x in radii):
        raise ValueError("periphery %s must be finite and > 0, got %r" % (want, radii if want == "radii" else radii[0]))
    k = floats([spec["k"]], 1, "k")[0]
    if not k >= 0.0:
        raise ValueError("periphery k must be finite and >= 0, got %r" % k)
    center = floats(spec.get("center", (0.0, 0.0, 0.0)), 3, "center")
    quat = floats(spec.get("quat", (1.0, 0.0, 0.0, 0.0)), 4, "quat")
    q2 = quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]
    if not abs(q2 - 1.0) <= 1e-12:
        raise ValueError("periphery quat must be a unit quaternion to 1e-12, |q|^2 - 1 = %g" % (q2 - 1.0))
    if shape == "ellipsoid_fast" and quat != [1.0, 0.0, 0.0, 0.0]:
        raise ValueError("periphery shape 'ellipsoid_fast' has no orientation (HP1.cpp:4155-4159): quat must be "
                         "(1, 0, 0, 0)")
    return shape, radii, k, center, quat


def periphery_force(periphery, center, radius, out=None, accumulate=False, stats=None):
    """the wall force of a periphery dict (check_periphery) on every bead (mhip_periphery_force): written to (or,
    accumulate=True, added into) out [n, 3] -> (out, colliding [1] int32, max_overlap [1] float64), the two statistics
    left on the device; stats: an optional (int32 [1], float64 [1]) pair to write them into"""
    shape, radii, k, c, q = periphery if isinstance(periphery, tuple) else check_periphery(periphery)
    n = center.shape[0]
    if tuple(center.shape) != (n, 3) or tuple(radius.shape) != (n,):
        raise ValueError("center must have shape [n, 3] and radius [n], got %s and %s" % (tuple(center.shape),
                                                                                          tuple(radius.shape)))
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs out")
        out = torch.empty((n, 3), dtype=torch.float64, device=center.device)
    if stats is None:
        stats = (torch.empty(1, dtype=torch.int32, device=center.device),
                 torch.empty(1, dtype=torch.float64, device=center.device))
    col, mx = stats
    cfg = capi.Periphery(PERIPHERY_SHAPES[shape], (C.c_double * 3)(*c), (C.c_double * 4)(*q), (C.c_double * 3)(*radii), k)
    capi.check(capi.load().mhip_periphery_force(C.byref(cfg), n, _ptr(center, cols=3, name="center"),
                                                _ptr(radius, name="radius"), _ptr(out, cols=3, name="out"),
                                                1 if accumulate else 0, C.c_void_p(col.data_ptr()),
                                                C.c_void_p(mx.data_ptr()), _stream()))
    return out, col, mx


# ---- active euchromatin force dipoles (HP1.cpp:2796-2826, :3770-3853, :4286-4354) --------------------------------------
def check_active_springs(n, pairs, sigma, kon, koff, keys=None, counter=None):
    """host-side validation of an active spring set (no library call) -> (pairs int32 [m, 2] host, sigma, kon, koff, keys
    uint64 [m] / None, counter uint64 [m] / None)"""
    p = pairs.detach().cpu().numpy() if isinstance(pairs, torch.Tensor) else np.asarray(pairs)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2 or not (p.dtype.kind in "iu" or p.size == 0):
        raise ValueError("active spring pairs must be integers of shape [m, 2], got %s %s" % (p.dtype, p.shape))
    if p.size and (p.min() < 0 or p.max() >= n):
        raise ValueError("active spring pairs: an index outside [0, %d)" % n)
    if p.size and (p[:, 0] == p[:, 1]).any():
        raise ValueError("active spring pairs: a spring from a body to itself (spring %d)"
                         % int(np.argmax(p[:, 0] == p[:, 1])))
    m = p.shape[0]
    sigma, kon, koff = float(sigma), float(kon), float(koff)
    if not math.isfinite(sigma):
        raise ValueError("active sigma must be finite, got %r" % sigma)
    for name, v in (("kon", kon), ("koff", koff)):
        if not (v > 0.0 and math.isfinite(v)):
            raise ValueError("active %s must be finite and > 0, got %r" % (name, v))
    return (np.ascontiguousarray(p, dtype=np.int32), sigma, kon, koff, check_philox_ints(keys, m, "active keys", np.uint64),
            check_philox_ints(counter, m, "active counter", np.uint64))


class ActiveSprings(_Handle):
    """m springs over n bodies that switch on and off as two-state Poisson processes and push their beads apart while on
    (mhip_active_springs_*): sample() -> force(center) -> ... -> advance(dt).  keys (default: the spring's index) and
    counter (default 0) key each spring's Philox stream."""
    _destroy = "mhip_active_springs_destroy"

    def __init__(self, n, pairs, sigma, kon, koff, keys=None, counter=None):
        p, sigma, kon, koff, ks, cs = check_active_springs(n, pairs, sigma, kon, koff, keys, counter)
        self.n, self.num_springs = int(n), p.shape[0]
        self.pairs, self.sigma, self.kon, self.koff = p, sigma, kon, koff
        h = C.c_void_p()
        cp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_active_springs_create(C.byref(h), self.n, p.shape[0], cp(p), sigma, kon, koff,
                                                          cp(ks), cp(cs), _stream()))
        self._h = h

    def sample(self, switches=None):
        """springs whose time has come switch; -> switches int32 [2] = (on, off) of this call, left on the device"""
        sw = torch.empty(2, dtype=torch.int32, device="cuda") if switches is None else switches
        capi.check(capi.load().mhip_active_springs_sample(self._h, _ptr(sw, torch.int32, name="switches"), _stream()))
        return sw

    def force(self, center, out=None, accumulate=False, active=None):
        """the force dipoles of the springs in state 1: written to (or, accumulate=True, added into) out [n, 3]
        -> (out, active int32 [1] = their number, left on the device)"""
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        if out is None:
            if accumulate:
                raise ValueError("accumulate=True needs out")
            out = torch.empty((self.n, 3), dtype=torch.float64, device=center.device)
        if active is None:
            active = torch.empty(1, dtype=torch.int32, device=center.device)
        capi.check(capi.load().mhip_active_springs_force(self._h, _ptr(center, cols=3, name="center"),
                                                         _ptr(out, cols=3, name="out"), 1 if accumulate else 0,
                                                         _ptr(active, torch.int32, name="active"), _stream()))
        return out, active

    def advance(self, dt):
        dt = float(dt)
        if not (dt >= 0.0 and dt < float("inf")):
            raise ValueError("dt must be finite and >= 0, got %r" % dt)
        capi.check(capi.load().mhip_active_springs_advance(self._h, dt, _stream()))

    def state(self, device="cuda"):
        """-> (state int32 [m], next_time [m], elapsed [m], counter int64 [m]) device tensors (copies)"""
        m = self.num_springs
        st = torch.empty(m, dtype=torch.int32, device=device)
        nt, el = (torch.empty(m, dtype=torch.float64, device=device) for _ in range(2))
        ct = torch.empty(m, dtype=torch.int64, device=device)
        capi.check(capi.load().mhip_active_springs_get_state(self._h, _ptr(st, torch.int32), _ptr(nt), _ptr(el),
                                                             _u64(ct, "counter"), _stream()))
        return st, nt, el, ct

    def set_state(self, state=None, next_time=None, elapsed=None, counter=None):
        """device tensors of the shapes state() returns into the handle; None = unchanged; values are not checked"""
        m = self.num_springs
        for name, t in (("state", state), ("next_time", next_time), ("elapsed", elapsed), ("counter", counter)):
            if t is not None and tuple(t.shape) != (m,):
                raise ValueError("%s must have shape [%d], got %s" % (name, m, tuple(t.shape)))
        capi.check(capi.load().mhip_active_springs_set_state(
            self._h, _ptr(state, torch.int32, allow_none=True, name="state"),
            _ptr(next_time, allow_none=True, name="next_time"), _ptr(elapsed, allow_none=True, name="elapsed"),
            _ptr(counter, torch.int64, allow_none=True, name="counter"), _stream()))

    def renumber(self, new_of_old):
        """the bodies were permuted: new_of_old int32 [n]"""
        if tuple(new_of_old.shape) != (self.n,):
            raise ValueError("new_of_old must have shape [%d], got %s" % (self.n, tuple(new_of_old.shape)))
        capi.check(capi.load().mhip_active_springs_renumber(self._h, _ptr(new_of_old, torch.int32, name="new_of_old"),
                                                            _stream()))


# ---- centerline-twist elastic filaments (mhip_filaments_*) ------------------------------------------------------------
def check_filaments(node_ptr, radius, rest_curvature, arclength, phase, youngs_modulus, poisson_ratio, rest_length,
                    viscosity, wave):
    """host-side validation of a filament set (no library call) -> (node_ptr int32 [F + 1], radius [N],
    rest_curvature [N, 3], arclength [N], phase [F] / None, capi.FilamentParams without the two constraint flags)"""
    host = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    ptr = host(node_ptr)
    if ptr.ndim != 1 or ptr.size < 1 or ptr.dtype.kind not in "iu":
        raise ValueError("node_ptr must be integers of shape [F + 1], got %s %s" % (ptr.dtype, ptr.shape))
    if int(ptr[0]) != 0:
        raise ValueError("node_ptr[0] must be 0, got %d" % int(ptr[0]))
    count = np.diff(ptr.astype(np.int64))
    if (count < 0).any():
        raise ValueError("node_ptr is not monotone at filament %d" % int(np.argmax(count < 0)))
    if (count < 2).any():
        f = int(np.argmax(count < 2))
        raise ValueError("filament %d has %d node(s): a filament has at least 2" % (f, int(count[f])))
    n, F = int(ptr[-1]), ptr.size - 1
    if n >= 2 ** 31:
        raise ValueError("too many nodes for 32-bit indices")
    r = np.ascontiguousarray(host(radius), dtype=np.float64)
    kr = np.ascontiguousarray(host(rest_curvature), dtype=np.float64)
    s = np.ascontiguousarray(host(arclength), dtype=np.float64)
    if r.shape != (n,) or kr.shape != (n, 3) or s.shape != (n,):
        raise ValueError("radius / rest_curvature / arclength must have the shapes [%d], [%d, 3], [%d], got %s, %s, %s"
                         % (n, n, n, r.shape, kr.shape, s.shape))
    if not (np.isfinite(r) & (r > 0.0)).all():
        raise ValueError("node %d: radius must be finite and > 0" % int(np.argmin(np.isfinite(r) & (r > 0.0))))
    if not (np.isfinite(kr).all() and np.isfinite(s).all()):
        raise ValueError("rest_curvature / arclength must be finite")
    ph = None
    if phase is not None:
        ph = np.ascontiguousarray(host(phase), dtype=np.float64)
        if ph.shape != (F,) or not np.isfinite(ph).all():
            raise ValueError("phase must be finite and of shape [%d], got %s" % (F, ph.shape))
    E, nu, l0, eta = float(youngs_modulus), float(poisson_ratio), float(rest_length), float(viscosity)
    if not (E >= 0.0 and math.isfinite(E)):
        raise ValueError("youngs_modulus must be finite and >= 0, got %r" % E)
    if not (nu > -1.0 and math.isfinite(nu)):
        raise ValueError("poisson_ratio must be finite and > -1, got %r" % nu)
    if not (l0 > 0.0 and math.isfinite(l0)):
        raise ValueError("rest_length must be finite and > 0, got %r" % l0)
    if not (eta > 0.0 and math.isfinite(eta)):
        raise ValueError("viscosity must be finite and > 0, got %r" % eta)
    A = k = w = 0.0
    if wave is not None:
        check_dict_spec(wave, "wave", ("amplitude", "wave_number", "frequency"))
        A, k, w = float(wave["amplitude"]), float(wave["wave_number"]), float(wave["frequency"])
        if not (math.isfinite(A) and math.isfinite(k) and math.isfinite(w)):
            raise ValueError("wave: amplitude, wave_number and frequency must be finite")
    prm = capi.FilamentParams(E, nu, l0, eta, A, k, w, 1 if wave is not None else 0, 0, 0)
    return np.ascontiguousarray(ptr, dtype=np.int32), r, kr, s, ph, prm


def check_filament_inertial(num_filaments, density, damping="critical", fixed_filaments=None):
    """host-side validation of Filaments.set_inertial (no library call) -> (capi.FilamentInertialParams, the mask as
    uint8 [F] / None)"""
    rho = float(density)
    if not (math.isfinite(rho) and rho > 0.0):
        raise ValueError("density must be finite and > 0, got %r" % (density,))
    if isinstance(damping, str):
        if damping != "critical":
            raise ValueError('damping must be "critical" or (translational, twist), got %r' % (damping,))
        prm = capi.FilamentInertialParams(rho, capi.FILAMENT_DAMPING_CRITICAL, 0.0, 0.0)
    else:
        if not (isinstance(damping, (tuple, list)) and len(damping) == 2):
            raise ValueError('damping must be "critical" or (translational, twist), got %r' % (damping,))
        ct, cr = _finite_nonneg(damping[0], "damping[0]"), _finite_nonneg(damping[1], "damping[1]")
        prm = capi.FilamentInertialParams(rho, capi.FILAMENT_DAMPING_CONSTANT, ct, cr)
    fixed = None
    if fixed_filaments is not None:
        fixed = fixed_filaments.detach().cpu().numpy() if isinstance(fixed_filaments, torch.Tensor) else fixed_filaments
        fixed = np.asarray(fixed)
        if fixed.shape != (num_filaments,) or fixed.dtype.kind not in "biu":
            raise ValueError("fixed_filaments must be a mask of shape [%d], got %s %s"
                             % (num_filaments, fixed.dtype, fixed.shape))
        fixed = np.ascontiguousarray(fixed != 0, dtype=np.uint8)
    return prm, fixed


class Filaments(_Handle):
    """F centerline-twist filaments over N nodes (mhip_filaments_*): the state lives in the handle.  wave: None, or
    dict(amplitude, wave_number, frequency) of the travelling rest-curvature wave (phase [F] keys it per filament).
    set_state -> [advance -> force -> velocity] per step; field(name) copies a field of capi.FILAMENT_FIELDS out."""
    _destroy = "mhip_filaments_destroy"
    _WIDTH = {"center": 3, "velocity": 3, "force": 3, "rest_curvature": 3, "curvature": 3, "edge_tangent": 3,
              "edge_binormal": 3, "edge_tangent_old": 3, "edge_binormal_old": 3, "edge_orientation": 4,
              "edge_orientation_old": 4}

    def __init__(self, node_ptr, radius, rest_curvature, arclength, phase=None, *, youngs_modulus, poisson_ratio,
                 rest_length, viscosity, wave=None, disable_twist=False, monolayer=False):
        ptr, r, kr, s, ph, prm = check_filaments(node_ptr, radius, rest_curvature, arclength, phase, youngs_modulus,
                                                 poisson_ratio, rest_length, viscosity, wave)
        prm.disable_twist, prm.monolayer = int(bool(disable_twist)), int(bool(monolayer))
        self.node_ptr, self.params = ptr, prm
        self.n, self.num_filaments = int(ptr[-1]), ptr.size - 1
        h = C.c_void_p()
        cp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_filaments_create(C.byref(h), self.num_filaments, cp(ptr), cp(r), cp(kr), cp(s), cp(ph),
                                                     C.byref(prm), _stream()))
        self._h = h

    def set_state(self, center, twist, edge_orientation):
        """device tensors center [N, 3], twist [N], edge_orientation [N, 4] (w, x, y, z; indexed by the left node)"""
        n = self.n
        for name, t, shape in (("center", center, (n, 3)), ("twist", twist, (n,)),
                               ("edge_orientation", edge_orientation, (n, 4))):
            if tuple(t.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, list(shape), tuple(t.shape)))
        capi.check(capi.load().mhip_filaments_set_state(self._h, _ptr(center, name="center"), _ptr(twist, name="twist"),
                                                        _ptr(edge_orientation, name="edge_orientation")))

    def advance(self, dt):
        capi.check(capi.load().mhip_filaments_advance(self._h, float(dt)))

    def force(self, time, external_force=None, stats=None):
        """edge pass + node pass at `time`; -> stats float64 [2] = (largest |l - l0| / l0, largest |kappa - rest|
        component), left on the device"""
        ext = self._external(external_force)
        if stats is None:
            stats = torch.empty(2, dtype=torch.float64, device="cuda")
        capi.check(capi.load().mhip_filaments_force(self._h, float(time), ext, _ptr(stats, name="stats")))
        return stats

    def _external(self, external_force):
        """a tensor [N, 3], None, or the pointer of a [N, 3] buffer the library owns (FilamentContacts.node_force_ptr)"""
        if isinstance(external_force, C.c_void_p):
            return external_force
        if external_force is not None and tuple(external_force.shape) != (self.n, 3):
            raise ValueError("external_force must have shape [%d, 3], got %s" % (self.n, tuple(external_force.shape)))
        return _ptr(external_force, allow_none=True, name="external_force")

    def edge_pass(self):
        """the first half of force(): every edge's tangent, length, binormal and orientation"""
        capi.check(capi.load().mhip_filaments_edge_pass(self._h))

    def node_pass(self, time, external_force=None, stats=None):
        """the second half of force(): curvature, forces and twist torques from the edge state as it stands"""
        if stats is None:
            stats = torch.empty(2, dtype=torch.float64, device="cuda")
        capi.check(capi.load().mhip_filaments_node_pass(self._h, float(time), self._external(external_force),
                                                        _ptr(stats, name="stats")))
        return stats

    def velocity(self):
        capi.check(capi.load().mhip_filaments_velocity(self._h))

    # ---- inertial nodes (include/mundy_hip_filament_inertial.h) -------------------------------------------------------
    def set_inertial(self, density, damping="critical", fixed_filaments=None):
        """nodes with mass: per step predict(dt) -> force(time, external) -> correct(dt).  damping: "critical"
        (c_t = c_r = sqrt(m E), CollidingFrictionalSperm.cpp) or the constants (c_t, c_r) (CollidingSperm.cpp);
        fixed_filaments: None or a mask [F] of the filaments that do not move"""
        prm, fixed = check_filament_inertial(self.num_filaments, density, damping, fixed_filaments)
        capi.check(capi.load().mhip_filaments_set_inertial(
            self._h, C.byref(prm), None if fixed is None else fixed.ctypes.data_as(C.c_void_p)))
        self.inertial = prm

    def set_motion(self, velocity=None, twist_velocity=None, acceleration=None, twist_acceleration=None):
        """device tensors [N, 3], [N], [N, 3], [N]; None: zeros"""
        n = self.n
        for name, t, shape in (("velocity", velocity, (n, 3)), ("twist_velocity", twist_velocity, (n,)),
                               ("acceleration", acceleration, (n, 3)), ("twist_acceleration", twist_acceleration, (n,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError("%s must have shape %s, got %s" % (name, list(shape), tuple(t.shape)))
        capi.check(capi.load().mhip_filaments_set_motion(
            self._h, _ptr(velocity, allow_none=True, name="velocity"),
            _ptr(twist_velocity, allow_none=True, name="twist_velocity"),
            _ptr(acceleration, allow_none=True, name="acceleration"),
            _ptr(twist_acceleration, allow_none=True, name="twist_acceleration")))

    def predict(self, dt):
        capi.check(capi.load().mhip_filaments_predict(self._h, float(dt)))

    def correct(self, dt, kinetic_energy=None):
        """kinetic_energy: None, or a float64 device tensor whose first element receives the sum"""
        capi.check(capi.load().mhip_filaments_correct(self._h, float(dt), _ptr(kinetic_energy, allow_none=True,
                                                                               name="kinetic_energy")))

    def kinetic_energy(self, out=None):
        """the kinetic energy of the current velocities -> float64 [1] on the device"""
        if out is None:
            out = torch.empty(1, dtype=torch.float64, device="cuda")
        capi.check(capi.load().mhip_filaments_kinetic_energy(self._h, _ptr(out, name="out")))
        return out

    def set_youngs_modulus(self, youngs_modulus):
        capi.check(capi.load().mhip_filaments_set_youngs_modulus(self._h, float(youngs_modulus)))
        self.params.youngs_modulus = float(youngs_modulus)

    def field(self, name):
        """a copy of one field (capi.FILAMENT_FIELDS, "acceleration", "twist_acceleration") as a device tensor"""
        if name in ("acceleration", "twist_acceleration"):
            got = capi.FilamentInertialFields()
            capi.check(capi.load().mhip_filaments_get_inertial(self._h, C.byref(got)))
            if not getattr(got, name):
                raise RuntimeError("%s before set_inertial" % name)
            return _read_field(getattr(got, name), self.n, 3 if name == "acceleration" else 1)
        if name not in capi.FILAMENT_FIELDS:
            raise ValueError("unknown filament field %r" % (name,))
        fields = capi.FilamentFields()
        capi.check(capi.load().mhip_filaments_get(self._h, C.byref(fields)))
        rows = self.num_filaments if name == "phase" else self.n
        return _read_field(getattr(fields, name), rows, self._WIDTH.get(name, 1))


# ---- frictional Hertzian contacts between filament segments (mhip_filament_contacts_*) ---------------------------------
FILAMENT_CONTACT_LAWS = {"frictional": capi.FILAMENT_CONTACT_FRICTIONAL, "hertz": capi.FILAMENT_CONTACT_HERTZ}


def check_filament_contacts(n, skin, youngs_modulus, poisson_ratio, mu, damping=(0.0, 0.0), density=1.0,
                            segment_radius=None, history_dt=None, bonded_exclusion=1, law="frictional"):
    """host-side validation of a contact stage over n nodes (no library call) -> (capi.FilamentContactParams without the
    monolayer flag, segment_radius [n] / None).  law: "frictional", or "hertz", the frictionless law
    (mundy_hip_filament_inertial.h), which reads neither mu nor the dampings"""
    if law not in FILAMENT_CONTACT_LAWS:
        raise ValueError("law must be one of %s, got %r" % (", ".join(sorted(FILAMENT_CONTACT_LAWS)), law))
    skin = _finite(skin, "skin", lambda v: v >= 0.0, ">= 0")
    E = _finite(youngs_modulus, "youngs_modulus", lambda v: v > 0.0, "> 0")
    nu = _finite(poisson_ratio, "poisson_ratio", lambda v: 0.0 < v < 1.0, "in (0, 1)")
    mu = _finite(mu, "mu", lambda v: v >= 0.0, ">= 0")
    if not (isinstance(damping, (tuple, list)) and len(damping) == 2):
        raise ValueError("damping must be (normal, tangential), got %r" % (damping,))
    gn = _finite(damping[0], "damping[0]", lambda v: v >= 0.0, ">= 0")
    gt = _finite(damping[1], "damping[1]", lambda v: v >= 0.0, ">= 0")
    rho = _finite(density, "density", lambda v: v >= 0.0, ">= 0")
    hdt = -1.0 if history_dt is None else _finite(history_dt, "history_dt", lambda v: v >= 0.0, ">= 0")
    if isinstance(bonded_exclusion, bool) or not isinstance(bonded_exclusion, (int, np.integer)) or bonded_exclusion < 1:
        raise ValueError("bonded_exclusion must be an integer >= 1, got %r" % (bonded_exclusion,))
    r = None
    if segment_radius is not None:
        r = segment_radius.detach().cpu().numpy() if isinstance(segment_radius, torch.Tensor) else segment_radius
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.shape != (n,):
            raise ValueError("segment_radius must have shape [%d], got %s" % (n, r.shape))
        if not (np.isfinite(r) & (r > 0.0)).all():
            raise ValueError("segment %d: radius must be finite and > 0" % int(np.argmin(np.isfinite(r) & (r > 0.0))))
    return capi.FilamentContactParams(skin, E, nu, mu, gn, gt, rho, hdt, int(bonded_exclusion), 0), r


class FilamentContacts(_Handle):
    """Frictional Hertzian contacts between the segments of an ops.Filaments (mhip_filament_contacts_*); segment i joins
    the nodes i and i + 1.  Per step: save_velocity -> filaments.advance -> update -> force -> filaments.force(time,
    node_force).  The filaments must outlive this object; all calls run on the stream current at construction."""
    _destroy = "mhip_filament_contacts_destroy"

    def __init__(self, filaments, **params):
        prm, r = check_filament_contacts(filaments.n, **params)
        prm.monolayer = int(filaments.params.monolayer)
        self.filaments, self.params, self.n = filaments, prm, filaments.n
        h = C.c_void_p()
        capi.check(capi.load().mhip_filament_contacts_create(
            C.byref(h), filaments._h, filaments.node_ptr.ctypes.data_as(C.c_void_p),
            None if r is None else r.ctypes.data_as(C.c_void_p), C.byref(prm), _stream()))
        self._h = h
        self.stats = torch.zeros(2, dtype=torch.float64, device="cuda")
        self.law = "frictional"
        if params.get("law", "frictional") != "frictional":
            self.set_law(params["law"])

    def set_law(self, law):
        """"frictional" (the default) or "hertz": the frictionless law, which needs no save_velocity"""
        if law not in FILAMENT_CONTACT_LAWS:
            raise ValueError("law must be one of %s, got %r" % (", ".join(sorted(FILAMENT_CONTACT_LAWS)), law))
        capi.check(capi.load().mhip_filament_contacts_set_law(self._h, FILAMENT_CONTACT_LAWS[law]))
        self.law = law

    def save_velocity(self):
        capi.check(capi.load().mhip_filament_contacts_save_velocity(self._h))

    def update(self):
        """the segment view and, when a box corner has moved by skin / 2 (or on the first call), the list -> rebuilt"""
        rebuilt = C.c_int(0)
        capi.check(capi.load().mhip_filament_contacts_update(self._h, C.byref(rebuilt)))
        return bool(rebuilt.value)

    def force(self, dt, external_force=None, stats=None):
        """linker pass + reduction -> stats [2] float64 on the device: (max overlap, the bits of the int64 count of
        capped contacts); the node forces are field("node_force") / node_force_ptr()"""
        if external_force is not None and tuple(external_force.shape) != (self.n, 3):
            raise ValueError("external_force must have shape [%d, 3], got %s" % (self.n, tuple(external_force.shape)))
        stats = self.stats if stats is None else stats
        capi.check(capi.load().mhip_filament_contacts_force(self._h, float(dt),
                                                            _ptr(external_force, allow_none=True, name="external_force"),
                                                            _ptr(stats, name="stats")))
        return stats

    def segment_view(self):
        """the first half of update(): seg and aabb from the nodes as they stand"""
        capi.check(capi.load().mhip_filament_contacts_segment_view(self._h))

    def linker_pass(self, dt, stats=None):
        """the first half of force(): sep, tang_disp, force and share of every linker, and the statistics"""
        stats = self.stats if stats is None else stats
        capi.check(capi.load().mhip_filament_contacts_linker_pass(self._h, float(dt), _ptr(stats, name="stats")))
        return stats

    def reduce(self, external_force=None):
        """the second half of force(): node_force from the linker rows as they stand"""
        capi.check(capi.load().mhip_filament_contacts_reduce(self._h, _ptr(external_force, allow_none=True,
                                                                           name="external_force")))

    def set_history(self, pairs, tang_disp):
        """plants tang_disp [c, 3] for the canonical list pairs int32 [c, 2] (device tensors)"""
        c = int(pairs.shape[0])
        if tuple(tang_disp.shape) != (c, 3):
            raise ValueError("tang_disp must have shape [%d, 3], got %s" % (c, tuple(tang_disp.shape)))
        capi.check(capi.load().mhip_filament_contacts_set_history(
            self._h, c, _ptr(pairs, dtype=torch.int32, cols=2, name="pairs") if c else None,
            _ptr(tang_disp, name="tang_disp") if c else None))

    def fields(self):
        f = capi.FilamentContactFields()
        capi.check(capi.load().mhip_filament_contacts_get(self._h, C.byref(f)))
        return f

    @property
    def num_pairs(self):
        return int(self.fields().num_pairs)

    def node_force_ptr(self):
        """the device pointer of node_force [N, 3]: what Filaments.force takes as external_force without a copy"""
        return C.c_void_p(self.fields().node_force)

    def _span(self, name):
        if name not in capi.FILAMENT_CONTACT_FIELDS:
            raise ValueError("unknown filament contact field %r" % (name,))
        f = self.fields()
        rows = int(f.num_pairs) if name in ("pairs", "sep", "tang_disp", "force", "share") else self.n
        return getattr(f, name), rows, capi.FILAMENT_CONTACT_FIELDS[name]

    def field(self, name):
        """a copy of one field (capi.FILAMENT_CONTACT_FIELDS) as a device tensor; pairs int32 [c, 2], share [c, 2, 3]"""
        return _read_field(*self._span(name), name)

    def set_field(self, name, value):
        """overwrites one float64 field of the handle with `value` (a device tensor of the field's size): a restart"""
        _write_field(*self._span(name), value, name)


# ---- frictionless contacts between backbone segments (mhip_segment_contacts_*, include/mundy_hip_segment_contact.h) -----
SEGMENT_CONTACT_KINDS = {"hertz": capi.SEGMENT_CONTACT_HERTZ, "wca": capi.SEGMENT_CONTACT_WCA}
SEGMENT_CONTACT_KEYS = ("kind", "radius", "skin", "youngs_modulus", "poisson_ratio", "epsilon", "sigma", "cutoff",
                        "segments", "end_correction")
SEGMENT_CONTACT_DEFAULTS = dict(youngs_modulus=1000.0, poisson_ratio=0.3, epsilon=1.0, sigma=1.0, cutoff=1.12246204831,
                                segments=None, end_correction=None)


def chain_end_segments(n, ends):
    """the reference's "first or last element in chain": segments with an end node that belongs to no other segment ->
    uint8 [m]"""
    ends = np.asarray(ends).reshape(-1, 2)
    deg = np.bincount(ends.reshape(-1), minlength=n)
    return (deg[ends] == 1).any(axis=1).astype(np.uint8) if ends.size else np.zeros(0, np.uint8)


def check_segment_contacts(n, spec):
    """host-side validation of a segment contact term over n bodies (no library call): the refusals of
    mhip_segment_contacts_create.  spec: kind, radius, skin, segments ([m, 2] ends) and optionally the material / WCA
    parameters and end_correction (None: chain_end_segments; False: none; or a mask [m])
    -> (ends int32 [m, 2], radius array [m] / None, radius scalar, end_correction uint8 [m], capi.SegmentContactParams)"""
    check_dict_spec(spec, "segment contacts", SEGMENT_CONTACT_KEYS, optional=tuple(SEGMENT_CONTACT_DEFAULTS))
    spec = dict(SEGMENT_CONTACT_DEFAULTS, **spec)
    if spec["kind"] not in SEGMENT_CONTACT_KINDS:
        raise ValueError("segment contact kind must be 'hertz' or 'wca', got %r" % (spec["kind"],))
    if spec["segments"] is None:
        raise ValueError("segment contacts: segments is missing")
    seg = spec["segments"]
    p = seg.detach().cpu().numpy() if isinstance(seg, torch.Tensor) else np.asarray(seg)
    if p.size == 0:
        p = p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2 or not (p.dtype.kind in "iu" or p.size == 0):
        raise ValueError("segments must be integers of shape [m, 2], got %s %s" % (p.dtype, p.shape))
    if p.size and (p.min() < 0 or p.max() >= n):
        raise ValueError("segments: an index outside [0, %d)" % n)
    if p.size and (p[:, 0] == p[:, 1]).any():
        raise ValueError("segments: a segment from a body to itself (segment %d)" % int(np.argmax(p[:, 0] == p[:, 1])))
    m = p.shape[0]
    ra, r0 = _spring_param(spec["radius"], m, "segment radius", True)

    def number(name, ok, what):
        return _finite(spec[name], name, ok, what)
    skin = number("skin", lambda v: v >= 0.0, ">= 0")
    hertz = spec["kind"] == "hertz"
    # (the parameters of the other law are carried, not checked: the library reads only its own kind's)
    E = number("youngs_modulus", lambda v: v > 0.0, "> 0") if hertz else float(spec["youngs_modulus"])
    nu = number("poisson_ratio", lambda v: 0.0 < v < 1.0, "in (0, 1)") if hertz else float(spec["poisson_ratio"])
    eps = float(spec["epsilon"]) if hertz else number("epsilon", lambda v: v >= 0.0, ">= 0")
    sigma = float(spec["sigma"]) if hertz else number("sigma", lambda v: v > 0.0, "> 0")
    cutoff = float(spec["cutoff"]) if hertz else number("cutoff", lambda v: v > 0.0, "> 0")
    ec = spec["end_correction"]
    if ec is None:
        corr = chain_end_segments(n, p)
    elif ec is False:
        corr = np.zeros(m, np.uint8)
    else:
        corr = ec.detach().cpu().numpy() if isinstance(ec, torch.Tensor) else np.asarray(ec)
        if corr.shape != (m,) or corr.dtype.kind not in "biu":
            raise ValueError("end_correction must be None, False or a mask of shape [%d], got %s %s" %
                             (m, corr.dtype, corr.shape))
        corr = (corr != 0).astype(np.uint8)
    prm = capi.SegmentContactParams(SEGMENT_CONTACT_KINDS[spec["kind"]], skin, E, nu, eps, sigma, cutoff)
    return np.ascontiguousarray(p, dtype=np.int32), ra, r0, np.ascontiguousarray(corr), prm


class SegmentContacts(_Handle):
    """Frictionless Hertzian or WCA contacts between the segments `segments` [m, 2] over n bodies
    (mhip_segment_contacts_*): the backbone excluded volume of the HP1 app.  Per step: update(center) ->
    force(center, out, accumulate).  spec: the dict of check_segment_contacts."""
    _destroy = "mhip_segment_contacts_destroy"

    def __init__(self, n, **spec):
        ends, ra, r0, corr, prm = check_segment_contacts(n, spec)
        self.n, self.num_segments, self.kind = int(n), ends.shape[0], spec["kind"]
        self.ends, self.radius, self.end_correction, self.params = ends, (ra if ra is not None else r0), corr, prm
        h = C.c_void_p()
        cp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
        capi.check(capi.load().mhip_segment_contacts_create(C.byref(h), self.n, ends.shape[0], cp(ends), cp(ra), r0,
                                                            cp(corr), C.byref(prm), _stream()))
        self._h = h
        self.stats = torch.zeros(2, dtype=torch.int64, device="cuda")

    def _center(self, center):
        if tuple(center.shape) != (self.n, 3):
            raise ValueError("center must have shape [%d, 3], got %s" % (self.n, tuple(center.shape)))
        return _ptr(center, cols=3, name="center")

    def update(self, center, force_rebuild=False):
        """the segment view and boxes at `center` and, on the first call, when forced or when a box corner has moved by
        skin / 2, the list -> rebuilt"""
        rebuilt = C.c_int(0)
        capi.check(capi.load().mhip_segment_contacts_update(self._h, self._center(center), int(bool(force_rebuild)),
                                                            C.byref(rebuilt), _stream()))
        return bool(rebuilt.value)

    def _out(self, out, accumulate):
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs an `out` to add to")
            out = torch.empty((self.n, 3), dtype=torch.float64, device="cuda")
        if tuple(out.shape) != (self.n, 3):
            raise ValueError("out must have shape [%d, 3], got %s" % (self.n, tuple(out.shape)))
        return out

    def force(self, center, out=None, accumulate=False, stats=None):
        """segment view at `center`, linker pass, reduction -> (force [n, 3], stats int64 [2] on the device: the bits of
        the double max overlap, the number of linkers in the force branch)"""
        out = self._out(out, accumulate)
        stats = self.stats if stats is None else stats
        capi.check(capi.load().mhip_segment_contacts_force(self._h, self._center(center), _ptr(out, name="out"),
                                                           int(bool(accumulate)),
                                                           _ptr(stats, dtype=torch.int64, name="stats"), _stream()))
        return out, stats

    def linker_pass(self, stats=None):
        """the first half of force() over the segment view as it stands: sep, force, share of every linker"""
        stats = self.stats if stats is None else stats
        capi.check(capi.load().mhip_segment_contacts_linker_pass(self._h, _ptr(stats, dtype=torch.int64, name="stats"),
                                                                 _stream()))
        return stats

    def reduce(self, out=None, accumulate=False, stats=None):
        """the second half of force(): the node forces from the linker rows as they stand; stats[0] is only raised"""
        out = self._out(out, accumulate)
        capi.check(capi.load().mhip_segment_contacts_reduce(
            self._h, _ptr(out, name="out"), int(bool(accumulate)),
            _ptr(stats, dtype=torch.int64, name="stats", allow_none=True), _stream()))
        return out

    @staticmethod
    def read_stats(stats):
        """stats tensor -> (max overlap, linkers in the force branch); synchronises"""
        s = stats.cpu().numpy()
        return float(s[:1].view(np.float64)[0]), int(s[1])

    def fields(self):
        f = capi.SegmentContactFields()
        capi.check(capi.load().mhip_segment_contacts_get(self._h, C.byref(f)))
        return f

    @property
    def num_pairs(self):
        return int(self.fields().num_pairs)

    def field(self, name):
        """a copy of one field (capi.SEGMENT_CONTACT_FIELDS) as a device tensor; pairs int32 [c, 2], share [c, 2, 3]"""
        if name not in capi.SEGMENT_CONTACT_FIELDS:
            raise ValueError("unknown segment contact field %r" % (name,))
        f = self.fields()
        rows = self.num_segments if name in ("seg", "aabb") else int(f.num_pairs)
        return _read_field(getattr(f, name), rows, capi.SEGMENT_CONTACT_FIELDS[name], name)
