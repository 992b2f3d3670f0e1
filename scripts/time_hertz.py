"""Soft-contact (Hertz) step on the BASELINE configs[2] geometry: 10^6 spherocylinders r = 0.5, L = 2 at 40 % volume
fraction, Z-ordered, relaxed by two steps of the LCP path (as `bench.py --full` relaxes its packing), then Hertz steps at
a dt of a tenth of the explicit limit 2 / max_c (m_i + m_j) k_c of the initial stiffness k_c = 2 E* sqrt(R* delta_c).

    python scripts/time_hertz.py [--n N] [--steps K] [--warmup W] [--json PATH]
        ms per step with and without a list rebuild (host clock around synchronised steps), split by stage with device
        events (step(timed=True)); one JSON object per line to --json.
    python scripts/time_hertz.py --profile-steps K --sizes PATH
        only Hertz steps (no LCP relaxation in the process when --load-relaxed is given): the run rocprofv3
        --kernel-trace --stats is pointed at; writes the sizes the byte counts need.
    python scripts/time_hertz.py --summarize STATS_CSV --sizes PATH
        the Hertz kernel and the body-only sweep from a rocprofv3 kernel_stats.csv: time per launch, algorithmic bytes,
        share of the 8 TB/s HBM peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12  # B/s, MI355X spec (DESIGN.md section 4 uses the same peak)
E, NU = 1000.0, 0.3  # the reference's defaults (Bacteria.cpp:1213-1214)


def relaxed_system(n, relax_steps, load=None, save=None):
    import torch
    from mundy_amd import ops, pipeline, synth
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    b = synth.spherocylinders(n)
    if load:
        z = np.load(load)
        return dict(center=dev(z["center"]), quat=dev(z["quat"]), radius=dev(b["radius"]), length=dev(b["length"]))
    lcp = pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]), dev(b["length"]),
                                  search_buffer=0.1, cfg=ops.PGDConfig(max_iters=10000, tol=1e-5))
    lcp.reorder_bodies(cell_size=3.0, lo=[0.0, 0.0, 0.0])
    for _ in range(relax_steps):
        lcp.step(integrate=True, force_rebuild=True)
    out = dict(center=lcp.center.clone(), quat=lcp.quat.clone(), radius=lcp.radius.clone(), length=lcp.length.clone())
    if lcp.op is not None:
        lcp.op.close()
    if save:
        np.savez(save, center=out["center"].cpu().numpy(), quat=out["quat"].cpu().numpy())
    return out


def hertz_stepper(sysd):
    from mundy_amd import pipeline
    from hertz_model import stiffness
    st = pipeline.ContactStepper("spherocylinder", sysd["center"], sysd["radius"], sysd["quat"], sysd["length"],
                                 search_buffer=0.1, contact_model="hertz", youngs_modulus=E, poisson_ratio=NU)
    st.compute_aabb()
    st.generate_neighbor_links(force=True)
    c = st.compute_contacts()
    pairs, sep = st.links.pairs.cpu().numpy(), c["sep"].cpu().numpy()
    mt = st.mob_trans.cpu().numpy()
    k = stiffness(pairs, sep, sysd["radius"].cpu().numpy(), E, NU)
    st.dt = 0.1 * 2.0 / float(np.max((mt[pairs[:, 0]] + mt[pairs[:, 1]]) * k))
    return st, dict(num_contacts=int(len(pairs)), overlapping=int((sep < 0).sum()), dt=st.dt,
                    max_overlap_initial=float(max(0.0, -sep.min())))


def timing(args):
    import torch
    sysd = relaxed_system(args.n, args.relax_steps, save=args.save_relaxed)
    st, info = hertz_stepper(sysd)
    lines = [dict(what="setup", n=args.n, relax_steps=args.relax_steps, youngs_modulus=E, poisson_ratio=NU, **info)]
    for rebuild in (True, False):
        for _ in range(args.warmup):
            st.step(force_rebuild=rebuild)
        torch.cuda.synchronize()
        wall, stages, rebuilt, ov = [], {}, [], []
        for _ in range(args.steps):   # host clock around synchronised steps (the max_overlap read synchronises)
            t0 = time.perf_counter()
            s = st.step(force_rebuild=rebuild)
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            rebuilt.append(s.rebuilt)
            ov.append(s.max_overlap)
        for _ in range(args.steps):   # device events per stage, separate steps (the events add host work)
            s = st.step(force_rebuild=rebuild, timed=True)
            for k, v in s.timings_ms.items():
                stages.setdefault(k, []).append(v)
        lines.append(dict(what="hertz step, %s" % ("list rebuilt every step" if rebuild else "list reused (rebuild rule)"),
                          steps=args.steps, ms_per_step_median=round(float(np.median(wall)), 4),
                          ms_per_step_min=round(float(np.min(wall)), 4), rebuilt_steps=int(sum(rebuilt)),
                          num_contacts=s.num_contacts, max_overlap_last=ov[-1],
                          stage_ms_median={k: round(float(np.median(v)), 4) for k, v in stages.items()}))
    return lines


def profile(args):
    import torch
    sysd = relaxed_system(args.n, args.relax_steps, load=args.load_relaxed)
    st, info = hertz_stepper(sysd)
    for k in range(args.profile_steps):
        st.step(force_rebuild=(k == 0))
    torch.cuda.synchronize()
    s = st.step(integrate=False)
    f = st.lam.cpu().numpy()
    sizes = dict(info, n=args.n, num_contacts=s.num_contacts, loaded_contacts=int((f > 0).sum()),
                 steps=args.profile_steps + 1)
    with open(args.sizes, "w") as fh:
        json.dump(sizes, fh)
    return [dict(what="profiled run", **sizes)]


def algorithmic_bytes(sz):
    C, N, A = sz["num_contacts"], sz["n"], sz["loaded_contacts"]
    return {
        # pair 8 + sep 8 read, force 8 written per contact; the rod radius once per body (scalar E, nu: no gather)
        "k_hertz_force": 24 * C + 8 * N,
        # body sweep (X_APPLY, rod kinematics): incidence entry 4 per half edge, the 32-byte half-edge record of each
        # half edge whose force is not zero, the force 8 per contact (gathered by both half edges, counted once);
        # per body row pointer 4 + mobilities 16 + axis 24 + (U, Z) row 48 + angular velocity 24
        "k_body": 4 * 2 * C + 32 * 2 * A + 8 * C + 116 * N,
    }


def summarize(args):
    import csv
    sz = json.load(open(args.sizes))
    rows = list(csv.DictReader(open(args.summarize)))
    want = algorithmic_bytes(sz)
    out = []
    # (the profiled process runs no solve: every k_body launch in it is a body-only sweep)
    for name_key, label in (("k_hertz_force", "Hertz force (k_hertz_force)"),
                            ("k_body", "body-only sweep (k_body in X_APPLY mode, rod kinematics)")):
        hit = [r for r in rows if name_key in r["Name"]]
        if not hit:
            out.append(dict(what=label, error="not in the trace"))
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        total_ns = sum(float(r["TotalDurationNs"]) for r in hit)
        avg_ms = total_ns / calls / 1e6
        b = want[name_key]
        out.append(dict(what=label, kernels=[r["Name"] for r in hit], calls=calls, ms_per_launch=round(avg_ms, 5),
                        algorithmic_bytes=b, achieved_TBps=round(b / (avg_ms * 1e-3) / 1e12, 3),
                        share_of_hbm_peak=round(b / (avg_ms * 1e-3) / HBM_PEAK, 3)))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--relax-steps", type=int, default=2)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--json", default=None)
    p.add_argument("--save-relaxed", default=None)
    p.add_argument("--load-relaxed", default=None)
    p.add_argument("--profile-steps", type=int, default=0)
    p.add_argument("--sizes", default=None)
    p.add_argument("--summarize", default=None)
    args = p.parse_args()
    if args.summarize:
        lines = summarize(args)
    elif args.profile_steps:
        lines = profile(args)
    else:
        lines = timing(args)
    for ln in lines:
        print(json.dumps(ln))
    if args.json:
        with open(args.json, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
