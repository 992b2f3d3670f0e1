"""The semiflexible-chain laws on the host (include/mundy_hip_bending.h): the numpy restatement
tests/bending_model.py against known answers and against the gradients of its potentials (where the tolerances of
tests/test_gpu_bending.py are measured), conservation and the clamp, every refusal that happens before a HIP call, and
the header against its binding table and the built library.  No compute entry point runs here."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import bending_cases as bc
import bending_model as bm
import gradient_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mundy_hip_bending.h")
NAMES = ("mhip_springs_set_wca", "mhip_angular_springs_create", "mhip_angular_springs_force",
         "mhip_angular_springs_renumber", "mhip_angular_springs_get", "mhip_angular_springs_destroy")


@pytest.fixture(scope="module")
def lib():
    from mundy_amd import build, capi
    build.build()
    return capi.load()


def _ulps(a, b):
    return abs(int(np.float64(a).view(np.int64)) - int(np.float64(b).view(np.int64)))


# ---- known answers ---------------------------------------------------------------------------------------------------------------
def test_the_reference_fenewca_answer():
    """UnitTestSprings.cpp:273-318: k = 3, r_max = 2.5, beads at the origin and at (0, 0, 1): magnitude 24 - 3 / 0.84,
    repulsive, at both ends, within the four ulps of EXPECT_DOUBLE_EQ"""
    x = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    f, over, mx = bm.fenewca_force(2, [[0, 1]], 3.0, 2.5, x)
    want = 24.0 - 3.0 / 0.84
    assert want > 0 and over == 0 and mx == 1.0
    assert (f[:, :2] == 0).all()
    assert f[0, 2] < 0 < f[1, 2]   # pushed apart
    assert _ulps(-f[0, 2], want) <= 4 and _ulps(f[1, 2], want) <= 4


def test_a_right_angle_by_hand():
    """unit arms, theta0 = pi (cos = -1 exactly): c = 0, tau = k, F_a = -k v2, F_b = -k v1, F_c = k (v1 + v2)"""
    k = 2.5
    x = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]])
    f, deg, dev = bm.angular_force(3, [[0, 1, 2]], k, -1.0, x)
    v1, v2 = x[0] - x[2], x[1] - x[2]
    assert deg == 0 and dev == 1.0
    assert (f[0] == -k * v2).all() and (f[1] == -k * v1).all() and (f[2] == k * (v1 + v2)).all()


def test_a_straight_triplet_at_pi_has_no_force():
    x = np.array([[-1.0, 0.0, 0.0], [1.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    f, deg, dev = bm.angular_force(3, [[0, 1, 2]], 7.0, -1.0, x)
    assert deg == 0 and dev == 0.0 and (f == 0.0).all()


def test_chain_triplets_are_the_references():
    """ChainOfSprings.cpp:456-462: (i, i + 2, i + 1) for every interior bead, chain by chain"""
    from mundy_amd import synth
    t = synth.chain_triplets([0, 4, 6, 7, 10])   # chains of 4, 2, 1 and 3 beads
    assert t.dtype == np.int32 and t.tolist() == [[0, 2, 1], [1, 3, 2], [7, 9, 8]]
    assert synth.chain_triplets([0]).shape == (0, 3)
    with pytest.raises(ValueError, match="non-decreasing"):
        synth.chain_triplets([0, 3, 2])


# ---- the gradient of the potential: where the device's tolerances are measured -----------------------------------------------
def test_inputs_meet_their_conditions():
    for case in bc.cases().values():
        case.check()


def test_calibration():
    """the model against -grad U (mpmath central differences at 50 digits), every case in its own frame and in the
    rotated and translated one; K of bending_cases.TOLERANCE_K is four times the worst, rounded up to a power of two"""
    worst = {}
    for name in bc.NAMES:
        case = bc.cases()[name]
        for moved in (False, True):
            F, S = bc.exact(name, moved)
            dev = gc.deviation(case.model(case.moved() if moved else None), F, S)
            assert np.isfinite(dev).all() and (S > 0).all(), name
            worst[case.group] = max(worst.get(case.group, 0.0), float(dev.max()))
            print("%-34s %-8s worst deviation of the model %8.3g eps S_b" % (name, "rotated" if moved else "", dev.max()))
    print("\n    %-26s %-28s %s   (4 x worst, rounded up)" % ("group", "worst deviation [eps S_b]", "K"))
    for group, k in bc.TOLERANCE_K.items():
        print("    %-26s %-28.3g %-5g %g" % (group, worst[group], k, 2.0 ** math.ceil(math.log2(4.0 * worst[group]))))
    assert set(worst) == set(bc.TOLERANCE_K)
    for group, k in bc.TOLERANCE_K.items():
        assert worst[group] <= k / 4.0, (group, worst[group], k)
        assert k == 2.0 ** round(math.log2(k))


# ---- conservation and the clamp ---------------------------------------------------------------------------------------------------
def test_momentum_and_angular_momentum_of_every_term():
    for name, case in bc.cases().items():
        x = case.x
        if case.kind == "fenewca":
            term, _ = bm.fenewca_terms(case.pairs, case.k, case.r_max, x, *case.wca)
            i, j = np.asarray(case.pairs).T
            rows, bodies = np.stack([term, -term], axis=1), np.stack([i, j], axis=1)
            assert (rows.sum(axis=1) == 0.0).all()   # exactly negated
        else:
            fa, fb, fc, _, _, _ = bm.angular_rows(case.triplets, case.k, case.cos_rest(), x)
            rows, bodies = np.stack([fa, fb, fc], axis=1), np.asarray(case.triplets)
            assert ((-fa - fb) == fc).all()          # the centre's row is the negated sum, exactly
        scale = np.abs(rows).max(axis=(1, 2))
        arm = np.abs(x[bodies]).max(axis=(1, 2))
        torque = np.cross(x[bodies], rows).sum(axis=1)
        assert (np.abs(rows.sum(axis=1)).max(axis=1) <= 4 * gc.EPS * scale).all(), name
        assert (np.abs(torque).max(axis=1) <= 16 * gc.EPS * scale * arm).all(), name


def test_a_bond_past_r_max_pulls_with_the_clamped_force_and_is_counted():
    k, r = 3.0, 1.5
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [2.6, 0.0, 0.0], [10.0, 0.0, 0.0], [10.0, 1.4999, 0.0]])
    pairs = [[0, 1], [1, 2], [2, 3], [3, 4]]
    term, L = bm.fenewca_terms(pairs, k, r, x)
    f, over, mx = bm.fenewca_force(5, pairs, k, r, x)
    assert over == 3 and mx == 7.4 and np.isfinite(f).all()   # 1.6, 7.4 and the bond AT the clamp; L = 1 is not
    la = r - 1e-4
    want = k * la / (1.0 - (la / r) * (la / r))   # past the cutoff: no WCA part
    assert want > 1e4
    for s in (1, 2):   # the same finite magnitude, towards the other bead
        assert _ulps(np.linalg.norm(term[s]), want) <= 2 and term[s][0] > 0
    assert _ulps(np.linalg.norm(term[3]), want) <= 2 and term[3][1] > 0


# ---- refusals, before any HIP call --------------------------------------------------------------------------------------------------
def P(k=1):
    return C.c_void_p(k * 64)   # a non-null pointer nothing dereferences: every refusal below comes first


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.mark.parametrize("trip,k,ks,a,as_,match", [
    ([[0, 1, 4]], None, 1.0, None, 3.0, "outside"), ([[0, -1, 2]], None, 1.0, None, 3.0, "outside"),
    ([[0, 0, 2]], None, 1.0, None, 3.0, "distinct"), ([[0, 1, 0]], None, 1.0, None, 3.0, "distinct"),
    ([[0, 2, 2]], None, 1.0, None, 3.0, "distinct"),
    ([[0, 1, 2]], None, -1.0, None, 3.0, "k must"), ([[0, 1, 2]], [-1.0], 0.0, None, 3.0, "k must"),
    ([[0, 1, 2]], None, math.nan, None, 3.0, "k must"), ([[0, 1, 2]], [math.inf], 0.0, None, 3.0, "k must"),
    ([[0, 1, 2]], None, 1.0, None, -0.1, "rest angle"), ([[0, 1, 2]], None, 1.0, None, 3.2, "rest angle"),
    ([[0, 1, 2]], None, 1.0, [math.nan], 0.0, "rest angle"), ([[0, 1, 2]], None, 1.0, [4.0], 0.0, "rest angle")])
def test_angular_create_refusals(lib, trip, k, ks, a, as_, match):
    from mundy_amd import capi
    h = C.c_void_p(1)
    t = _i32(trip)
    ka, aa = (None if v is None else _f64(v) for v in (k, a))
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_angular_springs_create(C.byref(h), 4, len(trip), _ptr(t), _ptr(ka), ks, _ptr(aa), as_, None))
    assert h.value is None


def test_angular_entry_points_refuse_nulls_and_too_many(lib):
    from mundy_amd import capi
    h = C.c_void_p()
    with pytest.raises(ValueError, match="too many triplets"):
        capi.check(lib.mhip_angular_springs_create(C.byref(h), 4, 2 ** 29, P(), None, 1.0, None, 3.0, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_angular_springs_create(None, 4, 0, None, None, 1.0, None, 3.0, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_angular_springs_create(C.byref(h), 4, 1, None, None, 1.0, None, 3.0, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_angular_springs_force(None, P(1), P(2), 0, P(3), P(4), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_angular_springs_renumber(None, P(1), None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_angular_springs_get(None, None, None, None))
    with pytest.raises(ValueError, match="null"):
        capi.check(lib.mhip_springs_set_wca(None, 1.0, 1.0))
    assert lib.mhip_angular_springs_destroy(None) == 0


@pytest.mark.parametrize("r,match", [(0.0, "r_max"), (-1.0, "r_max"), (math.nan, "r_max")])
def test_fenewca_create_refusals(lib, r, match):
    from mundy_amd import capi
    h = C.c_void_p(1)
    p = _i32([[0, 1]])
    with pytest.raises(ValueError, match=match):
        capi.check(lib.mhip_springs_create(C.byref(h), 2, 1, _ptr(p), capi.SPRING_FENEWCA, None, 1.0, None, r, None))
    with pytest.raises(ValueError, match="k must"):
        capi.check(lib.mhip_springs_create(C.byref(h), 2, 1, _ptr(p), capi.SPRING_FENEWCA, None, -1.0, None, 1.5, None))
    with pytest.raises(ValueError, match="unknown spring type"):
        capi.check(lib.mhip_springs_create(C.byref(h), 2, 1, _ptr(p), 3, None, 1.0, None, 1.5, None))


def test_fenewca_crosslinkers_are_refused(lib):
    from mundy_amd import capi, ops
    h = C.c_void_p(1)
    left = _i32([0])
    with pytest.raises(ValueError, match="FENE-WCA"):
        capi.check(lib.mhip_crosslinkers_create(C.byref(h), 2, 1, _ptr(left), None, None, capi.SPRING_FENEWCA, 1.0, 1.5,
                                                1.0, 1.0, 1.0, 1.0, None))
    assert h.value is None
    spec = dict(left=[0], sites=np.ones(2, np.uint8), kind="fenewca", k=1.0, r=1.5, bind_rate=1.0, unbind_rate=1.0,
                kt=1.0, capture_radius=1.0)
    with pytest.raises(ValueError, match="no 'fenewca' springs"):
        ops.check_crosslinkers(2, right=None, **spec)
    with pytest.raises(ValueError, match="no 'fenewca' springs"):
        ops.check_periphery_sites(dict(points=np.zeros((1, 3)), bind_rate=1.0, k=1.0, r=1.0), "fenewca", 1.0, 1.0)
    with pytest.raises(ValueError, match="no 'fenewca' springs"):
        _stepper(brownian_kt=0.0, crosslinkers=dict(spec, skin=0.1))


def test_ops_check_first():
    from mundy_amd import ops
    p, t, ka, k0, ra, r0 = ops.check_springs([[0, 1]], "fenewca", 3.0, 1.5, 2)
    assert t == 2 and (ka, k0, ra, r0) == (None, 3.0, None, 1.5)
    with pytest.raises(ValueError, match="r_max"):
        ops.check_springs([[0, 1]], "fenewca", 3.0, 0.0, 2)
    with pytest.raises(ValueError, match="belong to 'fenewca'"):
        ops.check_wca("fene", 1.0, 1.0)
    for eps, sig, match in ((0.0, 1.0, "epsilon"), (1.0, -1.0, "sigma"), (math.nan, 1.0, "epsilon"),
                            (1.0, math.inf, "sigma")):
        with pytest.raises(ValueError, match=match):
            ops.check_wca("fenewca", eps, sig)
    assert ops.check_wca("fenewca", 0.7, 0.9) == (0.7, 0.9)
    ok = ops.check_angular_springs(4, [[0, 2, 1]], [2.0], math.pi)
    assert ok[0].dtype == np.int32 and ok[1].tolist() == [2.0] and ok[3] is None and ok[4] == math.pi
    for args, match in ((([[0, 1, 4]], 1.0, 3.0), "outside"), (([[0, 1, 1]], 1.0, 3.0), "distinct"),
                        (([[0, 1]], 1.0, 3.0), "shape"), (([[0.5, 1, 2]], 1.0, 3.0), "integers"),
                        (([[0, 1, 2]], -1.0, 3.0), "k must"), (([[0, 1, 2]], [1.0, 2.0], 3.0), "shape"),
                        (([[0, 1, 2]], 1.0, 3.2), "rest angle"), (([[0, 1, 2]], 1.0, -0.5), "rest angle"),
                        (([[0, 1, 2]], 1.0, [math.nan]), "rest angle")):
        with pytest.raises(ValueError, match=match):
            ops.check_angular_springs(4, *args)
    with pytest.raises(ValueError, match="distinct"):   # the class checks before it reaches the library
        ops.AngularSprings(4, [[0, 1, 1]], 1.0, 3.0)


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


ANG = ([[0, 2, 1], [1, 3, 2]], 2.0, math.pi)
WCA_SPR = ([[0, 1], [1, 2], [2, 3]], "fenewca", 30.0, 1.5)


@pytest.mark.parametrize("kw,match", [
    (dict(kind="spherocylinder", angular_springs=ANG), "spheres only"),
    (dict(angular_springs=ANG, periodic_box=[10.0, 10.0, 10.0]), "periodic_box"),
    (dict(angular_springs=ANG, friction=0.3), "friction"), (dict(angular_springs=ANG, contact_cutoff=0.1), "contact_cutoff"),
    (dict(kind="spherocylinder", angular_springs=ANG, growth_rate=0.1, division_length=2.0), "spheres only"),
    (dict(kind="spherocylinder", angular_springs=ANG, contact_model="hertz", hertz_friction=0.3), "spheres only"),
    (dict(angular_springs=ANG[:2]), "angular_springs must be"),
    (dict(angular_springs=([[0, 2, 4]], 2.0, 3.0)), "outside"), (dict(angular_springs=([[0, 2, 2]], 2.0, 3.0)), "distinct"),
    (dict(angular_springs=([[0, 2, 1]], -2.0, 3.0)), "k must"), (dict(angular_springs=([[0, 2, 1]], 2.0, 3.5)), "rest angle"),
    (dict(springs=WCA_SPR, spring_wca=(0.0, 1.0)), "epsilon"), (dict(springs=WCA_SPR, spring_wca=(1.0, math.nan)), "sigma"),
    (dict(springs=WCA_SPR, spring_wca=(1.0,)), "spring_wca must be"),
    (dict(springs=(WCA_SPR[0], "fene", 30.0, 1.5), spring_wca=(1.0, 1.0)), "belong to 'fenewca'"),
    (dict(brownian_kt=0.1, spring_wca=(1.0, 1.0)), "spring_wca needs springs"),
    (dict(springs=(WCA_SPR[0], "fenewca", 30.0, 0.0)), "r_max"),
    (dict(springs=WCA_SPR, periodic_box=[10.0, 10.0, 10.0]), "periodic_box")])
def test_stepper_refusals(kw, match):
    # refused in the constructor before anything reaches the device (these tensors are on the CPU)
    with pytest.raises(ValueError, match=match):
        _stepper(**kw)


CPP_REFUSALS = r"""
#include <cmath>
#include <cstdio>
#include "mundy_hip/stepper.hpp"
using namespace mundy_hip;
template <class F>
static int refused(const char* what, F&& f) {
  try {
    f();
  } catch (const std::invalid_argument& e) {
    std::printf("REFUSED %s: %s\n", what, e.what());
    return 0;
  }
  std::printf("ACCEPTED %s\n", what);
  return 1;
}
int main() {
  int bad = 0;
  bad += refused("index", [] { mech::AngularSprings a(4, {0, 1, 4}, {}, 1.0, {}, 3.0); });
  bad += refused("distinct", [] { mech::AngularSprings a(4, {0, 1, 1}, {}, 1.0, {}, 3.0); });
  bad += refused("k", [] { mech::AngularSprings a(4, {0, 1, 2}, {}, -1.0, {}, 3.0); });
  bad += refused("k array", [] { mech::AngularSprings a(4, {0, 1, 2}, {std::nan("")}, 0.0, {}, 3.0); });
  bad += refused("angle", [] { mech::AngularSprings a(4, {0, 1, 2}, {}, 1.0, {}, 3.2); });
  bad += refused("angle array", [] { mech::AngularSprings a(4, {0, 1, 2}, {}, 1.0, {-0.5}, 0.0); });
  return bad;
}
"""


def test_cpp_classes_refuse_without_a_device_and_the_app_links(tmp_path):
    """mech::AngularSprings throws std::invalid_argument from the library's own checks, before any HIP call;
    mech::SphereChainStepper::set_angular_springs constructs exactly that class (the stepper itself needs a device:
    tests/test_gpu_bending.py runs its refusals through the app)"""
    from cpp_apps import build_app, compile_cpp
    assert os.path.exists(build_app("bending_step_app"))
    src = tmp_path / "refusals.cpp"
    src.write_text(CPP_REFUSALS)
    out = subprocess.run([compile_cpp(src, tmp_path / "refusals")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.count("REFUSED") == 6 and "ACCEPTED" not in out.stdout


# ---- the header and the table --------------------------------------------------------------------------------------------------------
def header_prototypes():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(mhip_[a-z0-9_]+)\s*\(([^;]*)\)\s*;", text)}


def test_header_symbols_are_exported_and_bound_and_the_table_names_nothing_else(lib):
    from mundy_amd import capi
    protos = header_prototypes()
    assert set(protos) == set(NAMES) == set(capi.BENDING_SIGNATURES)
    for other in (capi.SIGNATURES, capi.PERIPHERY_SIGNATURES, capi.CONTACT_FORCE_SIGNATURES,
                  capi.PERIPHERY_BINDING_SIGNATURES, capi.SEGMENT_CONTACT_SIGNATURES, capi.HYDRO_SOLVE_SIGNATURES,
                  capi.FILAMENT_INERTIAL_SIGNATURES):
        assert not set(capi.BENDING_SIGNATURES) & set(other)
    inc = os.path.join(ROOT, "include")
    others = [open(os.path.join(inc, h)).read() for h in sorted(os.listdir(inc))
              if h.endswith(".h") and h != "mundy_hip_bending.h"]
    assert len(others) >= 7
    for name, args in protos.items():
        for text in others:
            assert not re.search(r"\b%s\s*\(" % name, text), "%s is declared in another header too" % name
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(capi.BENDING_SIGNATURES[name])
        assert len(fn.argtypes) == len([a for a in args.split(",") if a.strip()]), name
    # the entry points that take a stream, and those that by design do not
    with_stream = {n for n, a in protos.items() if "mhip_stream_t" in a}
    assert with_stream == {"mhip_angular_springs_create", "mhip_angular_springs_force", "mhip_angular_springs_renumber"}
    main = open(os.path.join(inc, "mundy_hip.h")).read()
    assert re.search(r"#define\s+MHIP_SPRING_FENEWCA\s+2\b", main) and capi.SPRING_FENEWCA == 2
    from mundy_amd import ops
    assert ops.BACKBONE_SPRING_TYPES == dict(hookean=0, fene=1, fenewca=2) and "fenewca" not in ops.SPRING_TYPES
