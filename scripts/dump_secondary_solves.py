"""Every output array of the solver's secondary sweeps on small fixed inputs, as .npy files -- run on two trees and
compare the directories byte for byte (cmp / sha256sum) to show that a change of convex.hip left their bits alone.

    python scripts/dump_secondary_solves.py OUTDIR

Paths: the cone BBPGD and APGD friction solves, the scrap BBPGD variant on the three kinematics, and the vector-force
body sweep.  Inputs come from the makers of the test suite at 800 bodies; each must have more than one 256-contact
tile, a partial last tile, a body with at most one incidence entry and (cone paths) a body with more entries than
one pass of the sweep's 8 lanes x 2 entries covers, or the script refuses it."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle  # noqa: E402
from gpu_util import dev, host  # noqa: E402
from mundy_amd import ops  # noqa: E402
from test_gpu_convex import _gpu_op, _rod_problem, _rod_problem_arclength, _sphere_problem  # noqa: E402
from test_oracle_friction_ext import _rod_system  # noqa: E402

out = sys.argv[1]
os.makedirs(out, exist_ok=True)
oracle.build()


def save(name, a):
    np.save(os.path.join(out, name + ".npy"), np.ascontiguousarray(a))


def check_input(name, P, cone):
    C = len(P["pairs"])
    deg = np.bincount(np.asarray(P["pairs"]).ravel(), minlength=P["N"] if "N" in P else len(P["mt"]))
    ok = C > 256 and C % 256 != 0 and deg.min() <= 1 and (not cone or deg.max() > 16)
    print("%s: %d contacts (%d tiles + %d), degrees %d ... %d" % (name, C, C // 256, C % 256, deg.min(), deg.max()))
    if not ok:
        sys.exit("%s does not reach every path of the sweeps" % name)


# cone BBPGD and APGD
P = _rod_system(oracle, 800, seed=2)
check_input("cone", P, True)
op = ops.ContactOperator(dev(P["pairs"]), dev(P["normal"]), dev(P["mt"]), 5e-3, ra=dev(P["ras"]), rb=dev(P["rbs"]),
                         mob_rot=dev(P["mr"]))
for method in ("bbpgd", "apgd"):
    for mu in (0.0, 0.3):
        for label, cfg in [("it%d" % k, ops.PGDConfig(max_iters=k, tol=1e-12)) for k in (0, 1, 3, 9)] + \
                          [("tol", ops.PGDConfig(max_iters=50000, tol=1e-6))]:
            p, g, r = ops.solve_friction_contact(op, dev(P["sep"]), mu, cfg=cfg, method=method)
            tag = "cone_%s_mu%g_%s" % (method, mu, label)
            save(tag + "_p", host(p))
            save(tag + "_g", host(g))
            save(tag + "_result", np.array([r.num_iters, r.residual, float(r.converged)]))
op.close()

# the scrap variant and the vector body sweep on the three kinematics
for maker in (_sphere_problem, _rod_problem, _rod_problem_arclength):
    name = maker.__name__.strip("_")
    P = maker(oracle, 800, seed=3)
    check_input(name, P, False)
    C = len(P["pairs"])
    op = _gpu_op(ops, P)
    lam0 = np.abs(np.sin(np.arange(C))) * 0.01  # a nonzero guess: the first step's quirk takes part
    for label, cap in (("it1", 1), ("it2", 2), ("it7", 7), ("tol", 10000)):
        lam, g, r = ops.resolve_collisions(op, dev(P["sep"]), dev(lam0), 1.0, max_allowable_overlap=1e-5,
                                           max_col_iterations=cap)
        tag = "scrap_%s_%s" % (name, label)
        save(tag + "_lam", host(lam))
        save(tag + "_g", host(g))
        save(tag + "_result", np.array([r.ite_count, r.max_abs_projected_sep, r.max_displacement]))  # dt = 1: max speed
    force = np.random.default_rng(5).normal(size=(C, 3))
    force[::3] = 0.0
    op.body_sweep_vector(dev(force))
    torch.cuda.synchronize()
    save("vector_%s_body_velocity" % name, host(op.body_velocity()))
    op.close()
print("%d files in %s" % (len(os.listdir(out)), out))
