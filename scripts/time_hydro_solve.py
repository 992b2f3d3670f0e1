"""The LCP against the hydrodynamic mobility (mhip_bbpgd_solve_contact_hydro, include/mundy_hip_hydro_solve.h) on
chromatin chains (synth.chains, ngp_hp1.yaml's numbers): the contact list of the chains as they are drawn, q = sep, RPYC.

    python scripts/time_hydro_solve.py [--sizes 10000 30000] [--iters 16 48] [--rounds 9] [--reps 10] [--warmup 2]
                                       [--zero-shares 0.5 0.7 0.9 0.99] [--json PATH]
        per size, device-event medians of
          hydro iteration   (solve of --iters[1] iterations - solve of --iters[0]) / their difference, tol = 0 so that no
                            solve converges, from lambda = 0; the same for the dry fused solve (dry iteration)
          mobility stage    one accumulating mhip_hydro_velocity onto [n][6] rows with the force field F = D lambda of the
                            iterate after --iters[1] iterations, sparse sources on and off in alternating rounds of one
                            session (median of the rounds' medians, and their spread)
          stand-alone call  the same entry point with seeded normal forces on every bead (0 % zero rows), sparse sources
                            on and off alike: the dense regime; and with 50, 70, 90 and 99 % of those rows set to zero
                            at random (--zero-shares): how the sparse shape scales with the share of force-carrying beads
        and the share of bodies without a contact force at that iterate.  One JSON object per line to --json
        (profiles/hydro_solve_timing.jsonl is written from it).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def device_ms(fn, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t))


def system(n):
    """the chains, their sphere contact list and operator on the device"""
    import torch
    from mundy_amd import ops, pipeline, synth
    d = synth.chains(max(1, n // 1000), 1000 if n >= 1000 else n, seed=1234)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], brownian_kt=0.0)
    st.compute_aabb()
    st.generate_neighbor_links()
    st.compute_contacts()
    pairs, c = st.links.pairs, st.contacts
    op = ops.ContactOperator(pairs, c["normal"], st.mob_trans, d["dt"])
    return dict(d=d, st=st, op=op, q=c["sep"].clone(), center=st.center, radius=st.radius, n=int(st.center.shape[0]),
                contacts=int(pairs.shape[0]), overlapping=int((c["sep"] < 0).sum()))


def measure(n, iters, rounds, reps, warmup, zero_shares):
    import numpy as np
    import torch
    from mundy_amd import ops
    s = system(n)
    op, q, c, r, mu = s["op"], s["q"], s["center"], s["radius"], s["d"]["viscosity"]
    ws = ops.HydroWorkspace()
    mob = ops.HydroMobility("rpyc", mu, c, r, workspace=ws)
    state = tuple(torch.empty_like(q) for _ in range(4))

    def solve(k, mobility):
        state[0].zero_()
        return ops.solve_lcp(op, q, state[0], ops.PGDConfig(max_iters=k, tol=0.0), state=state, mobility=mobility)

    k0, k1 = iters
    per_iter = {}
    for label, m in (("hydro", mob), ("dry", None)):
        t0 = device_ms(lambda: solve(k0, m), reps, warmup)
        t1 = device_ms(lambda: solve(k1, m), reps, warmup)
        per_iter[label] = (t1 - t0) / (k1 - k0)
    # the force field of the iterate the hydrodynamic solve has reached after k1 iterations
    x, _, res = solve(k1, mob)
    F = op.body_force(x, stride=3)
    zero_share = float((F.abs().amax(dim=1) == 0.0).double().mean())
    dense = torch.from_numpy(np.random.default_rng(7).normal(size=(s["n"], 3))).cuda()
    rows = torch.zeros((s["n"], 6), dtype=torch.float64, device="cuda")
    fields = [("solve", F), ("dense", dense)]
    rng = np.random.default_rng(8)
    for share in zero_shares:  # the dense field with that share of its rows set to zero at random
        f = dense.clone()
        f[torch.from_numpy(rng.random(s["n"]) < share).cuda()] = 0.0
        fields.append(("zero_%g" % share, f))
    stage = {(what, on): [] for what, _ in fields for on in (True, False)}
    for _ in range(rounds):  # alternating rounds in one session
        for on in (True, False):
            ws.set_sparse_sources(on)
            for what, f in fields:
                stage[what, on].append(device_ms(
                    lambda: ops.hydro_velocity("rpyc", mu, c, r, f, out=rows, accumulate=True, workspace=ws), reps, warmup))
    ws.set_sparse_sources(False)

    def summary(v):
        return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))

    out = dict(what="hydro_solve", n=s["n"], contacts=s["contacts"], overlapping=s["overlapping"], iters=list(iters),
               iterations_run=res.num_iters, zero_force_share=zero_share, hydro_iteration_ms=per_iter["hydro"],
               dry_iteration_ms=per_iter["dry"],
               mobility_stage_ms=dict(sparse=summary(stage["solve", True]), dense_walk=summary(stage["solve", False])),
               standalone_dense_field_ms=dict(sparse=summary(stage["dense", True]),
                                              dense_walk=summary(stage["dense", False])),
               zero_rows_ms={what: dict(zero_share=float((f.abs().amax(dim=1) == 0.0).double().mean()),
                                        sparse=summary(stage[what, True]), dense_walk=summary(stage[what, False]))
                             for what, f in fields[2:]},
               path=ws.last_path(), rounds=rounds, reps=reps, warmup=warmup)
    out["dry_plus_stage_ms"] = out["dry_iteration_ms"] + out["mobility_stage_ms"]["sparse"]["median"]
    ws.close()
    op.close()
    return out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 30000])
    ap.add_argument("--iters", type=int, nargs=2, default=[16, 48])
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--zero-shares", type=float, nargs="*", default=[0.5, 0.7, 0.9, 0.99])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = [dict(what="setup", device=torch.cuda.get_device_name(), kind="rpyc")]
    for n in args.sizes:
        out.append(measure(n, args.iters, args.rounds, args.reps, args.warmup, args.zero_shares))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
