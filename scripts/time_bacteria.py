"""The bacterial colony step (Bacteria.cpp:1033-1080) at full size: 10^6 spherocylinders r = 0.5 from
synth.spherocylinders, lengths uniform in (cl_min, D] (cl_min = 0.5 D - r, a fresh child's length) so that births come
at a steady rate, Hertz contact with Bacteria's E, nu and viscosity, its dt = 1e-3 and growth rate 0.1 (:1205-1225).

    python scripts/time_bacteria.py [--n N] [--steps K] [--warmup W] [--json PATH]
        ms per step (host clock around synchronised steps), births and list rebuilds per step, with and without a
        Morton reorder every 10 steps (the reference load-balances every 10, :1076); the stages of separate steps
        from device events (step(timed=True)), grow_divide among them.  One JSON object per line to --json.
    python scripts/time_bacteria.py --profile-steps K [--quiet-steps Q] --sizes PATH
        K growth steps, then Q steps in which nobody divides (the division length raised out of reach), so that each of
        them runs the corner test against the AABBs of its last build: the run rocprofv3 --kernel-trace --stats is
        pointed at; writes the sizes the byte counts need.
    python scripts/time_bacteria.py --summarize STATS_CSV --sizes PATH
        the growth kernels from a rocprofv3 kernel_stats.csv: time per launch, algorithmic bytes, share of the
        8 TB/s HBM peak.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12  # B/s, MI355X spec (as scripts/time_hertz.py)
R, D, E, NU, VISC, DT, RATE = 0.5, 2.0, 1000.0, 0.3, 1.0, 1e-3, 0.1  # Bacteria.cpp:1205-1225
BUFFER = 0.5  # buffer_distance_ = bacteria_radius_


def colony(n, seed=1234):
    import torch
    from mundy_amd import pipeline, synth
    b = synth.spherocylinders(n, radius=R, seed=seed)
    cl_min = 0.5 * D - R
    length = cl_min + (D - cl_min) * (1.0 - synth.uniform01(seed, np.arange(n), 9))
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    return pipeline.ContactStepper("spherocylinder", dev(b["center"]), dev(b["radius"]), dev(b["quat"]), dev(length),
                                   dt=DT, viscosity=VISC, search_buffer=BUFFER, contact_model="hertz",
                                   youngs_modulus=E, poisson_ratio=NU, growth_rate=RATE, division_length=D)


def timing(args):
    import torch
    lines = [dict(what="setup", n=args.n, radius=R, division_length=D, youngs_modulus=E, poisson_ratio=NU,
                  viscosity=VISC, dt=DT, growth_rate=RATE, search_buffer=BUFFER, steps=args.steps, warmup=args.warmup)]
    for reorder_every in (0, 10):
        st = colony(args.n)
        for _ in range(args.warmup):
            st.step()
        torch.cuda.synchronize()
        wall, born, rebuilt, contacts, stages = [], [], [], [], {}
        for k in range(args.steps):  # host clock around synchronised steps (the birth count read synchronises)
            t0 = time.perf_counter()
            if reorder_every and k % reorder_every == 0:
                st.reorder_bodies()
            s = st.step()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            born.append(s.num_born)
            rebuilt.append(s.rebuilt)
            contacts.append(s.num_contacts)
        for _ in range(args.steps):  # device events per stage, separate steps (the events add host work)
            s = st.step(timed=True)
            for key, v in s.timings_ms.items():
                stages.setdefault(key, []).append(v)
        wall, born, rebuilt = np.array(wall), np.array(born), np.array(rebuilt)
        lines.append(dict(what="growth step, %s" % ("Morton reorder every %d steps" % reorder_every if reorder_every
                                                    else "no reorder"),
                          steps=args.steps, bodies_final=int(st.n), births_per_step_mean=round(float(born.mean()), 2),
                          steps_with_births=int((born > 0).sum()), rebuilds=int(rebuilt.sum()),
                          num_contacts_median=int(np.median(contacts)),
                          ms_per_step_median=round(float(np.median(wall)), 4),
                          ms_per_step_median_with_births=round(float(np.median(wall[born > 0])), 4) if (born > 0).any()
                          else None,
                          ms_per_step_median_without_births=round(float(np.median(wall[born == 0])), 4)
                          if (born == 0).any() else None,
                          stage_ms_median={key: round(float(np.median(v)), 4) for key, v in stages.items()}))
        if st.op is not None:
            st.op.close()
    return lines


def profile(args):
    import torch
    st = colony(args.n)
    born = rebuilt_quiet = 0
    for _ in range(args.profile_steps):
        born += st.step().num_born
    # at Bacteria's rate every step has births, and a step with births rebuilds without the corner test; these steps
    # have none, so each runs k_aabb_moved on this step's AABBs against the snapshot of the last build, as in a colony
    # that grows without dividing
    st.division_length = 1e300
    for _ in range(args.quiet_steps):
        s = st.step()
        assert s.num_born == 0
        rebuilt_quiet += int(s.rebuilt)
    torch.cuda.synchronize()
    sizes = dict(n=int(st.n), steps=args.profile_steps + args.quiet_steps, growth_steps=args.profile_steps,
                 quiet_steps=args.quiet_steps, quiet_steps_rebuilt=rebuilt_quiet, births=born)
    with open(args.sizes, "w") as fh:
        json.dump(sizes, fh)
    return [dict(what="profiled run", **sizes)]


def algorithmic_bytes(sz):
    n, nb = sz["n"], max(1, round(sz["births"] / max(1, sz["steps"])))
    return {
        # two passes read the length; per 1024-body tile a count and a base; parent_of written
        "k_divide_count": 8 * n + 4 * (n // 1024 + 1),
        "k_divide_emit": 8 * n + 4 * (n // 1024 + 1) + 4 * nb,
        # every length read and written; per birth the parent's centre, quat, radius read, two rows written
        "k_divide_grow": 16 * n + nb * (24 + 32 + 8 + 2 * (24 + 8) + 32 + 8),
        # both AABBs read (this step's and the snapshot of the last build)
        "k_aabb_moved": 96 * n,
    }


def summarize(args):
    import csv
    sz = json.load(open(args.sizes))
    rows = list(csv.DictReader(open(args.summarize)))
    want = algorithmic_bytes(sz)
    out = []
    for name_key in ("k_divide_count", "k_divide_emit", "k_divide_grow", "k_aabb_moved"):
        hit = [r for r in rows if name_key in r["Name"]]
        if not hit:
            out.append(dict(what=name_key, error="not in the trace"))
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        total_ns = sum(float(r["TotalDurationNs"]) for r in hit)
        avg_ms = total_ns / calls / 1e6
        b = want[name_key]
        out.append(dict(what=name_key, kernels=[r["Name"] for r in hit], calls=calls, ms_per_launch=round(avg_ms, 5),
                        algorithmic_bytes=b, achieved_TBps=round(b / (avg_ms * 1e-3) / 1e12, 3),
                        share_of_hbm_peak=round(b / (avg_ms * 1e-3) / HBM_PEAK, 3)))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--json", default=None)
    p.add_argument("--profile-steps", type=int, default=0)
    p.add_argument("--quiet-steps", type=int, default=10)
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
