"""Frictional Hertz step (hertz_friction=mu) against the frictionless one on the packing and by the method of
scripts/time_hertz.py: 10^6 spherocylinders of BASELINE configs[2], Z-ordered, relaxed by two LCP steps, dt a tenth of the
explicit limit.  The two steppers are timed alternately in one process (frictionless, frictional, frictionless, ...).

    python scripts/time_friction_hertz.py [--n N] [--steps K] [--warmup W] [--rounds R] [--json PATH]
        ms per step with a reused and with a rebuilt list (host clock around synchronised steps), split by stage with
        device events; the frictionless figures of the R rounds give the spread the comparison has to be read against.
    python scripts/time_friction_hertz.py --profile-steps K --sizes PATH [--load-relaxed NPZ]
        only frictional steps, every fifth with a rebuilt list: the run rocprofv3 --kernel-trace --stats is pointed at.
    python scripts/time_friction_hertz.py --summarize STATS_CSV --sizes PATH
        the three new kernels from a rocprofv3 kernel_stats.csv: time per launch, algorithmic bytes, share of the
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import time_hertz as th  # noqa: E402

MU = 0.5  # the reference's friction coefficient (FrictionalHertzianContact.cpp:413); no damping, density 1


def frictional_stepper(sysd, dt):
    from mundy_amd import pipeline
    return pipeline.ContactStepper("spherocylinder", sysd["center"].clone(), sysd["radius"], sysd["quat"].clone(),
                                   sysd["length"], dt=dt, search_buffer=0.1, contact_model="hertz",
                                   youngs_modulus=th.E, poisson_ratio=th.NU, hertz_friction=MU)


def time_steps(st, rebuild, steps, warmup):
    import torch
    for _ in range(warmup):
        st.step(force_rebuild=rebuild)
    torch.cuda.synchronize()
    wall, stages, sliding = [], {}, []
    for _ in range(steps):   # host clock around synchronised steps (the read of the step's statistics synchronises)
        t0 = time.perf_counter()
        s = st.step(force_rebuild=rebuild)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        sliding.append(s.num_sliding)
    for _ in range(steps):   # device events per stage, separate steps
        s = st.step(force_rebuild=rebuild, timed=True)
        for k, v in s.timings_ms.items():
            stages.setdefault(k, []).append(v)
    return dict(ms_per_step_median=round(float(np.median(wall)), 4), ms_per_step_min=round(float(np.min(wall)), 4),
                num_contacts=s.num_contacts, max_overlap_last=s.max_overlap, num_sliding_last=sliding[-1],
                stage_ms_median={k: round(float(np.median(v)), 4) for k, v in stages.items()})


def timing(args):
    sysd = th.relaxed_system(args.n, args.relax_steps, load=args.load_relaxed, save=args.save_relaxed)
    plain, info = th.hertz_stepper(dict(sysd, center=sysd["center"].clone(), quat=sysd["quat"].clone()))
    fr = frictional_stepper(sysd, plain.dt)
    lines = [dict(what="setup", n=args.n, relax_steps=args.relax_steps, youngs_modulus=th.E, poisson_ratio=th.NU, mu=MU,
                  **info)]
    for r in range(args.rounds):
        for name, st in (("frictionless", plain), ("frictional", fr)):
            for rebuild in (False, True):
                lines.append(dict(what="%s step, %s" % (name, "list rebuilt every step" if rebuild else "list reused"),
                                  round=r, steps=args.steps, **time_steps(st, rebuild, args.steps, args.warmup)))
    for rebuild in ("list reused", "list rebuilt every step"):
        a = [ln["ms_per_step_median"] for ln in lines if ln["what"] == "frictionless step, " + rebuild]
        b = [ln["ms_per_step_median"] for ln in lines if ln["what"] == "frictional step, " + rebuild]
        lines.append(dict(what="summary, " + rebuild, frictionless_ms=a, frictionless_spread_ms=round(max(a) - min(a), 4),
                          frictional_ms=b, frictional_over_frictionless=round(float(np.median(b) / np.median(a)), 3)))
    return lines


def profile(args):
    import torch
    sysd = th.relaxed_system(args.n, args.relax_steps, load=args.load_relaxed)
    plain, info = th.hertz_stepper(dict(sysd, center=sysd["center"].clone(), quat=sysd["quat"].clone()))
    fr = frictional_stepper(sysd, plain.dt)
    rebuilds = 0
    for k in range(args.profile_steps):
        s = fr.step(force_rebuild=(k % 5 == 0))
        rebuilds += int(s.rebuilt)
    torch.cuda.synchronize()
    s = fr.step(integrate=False)
    sep = fr.contacts["sep"].cpu().numpy()
    f = fr.contact_force.cpu().numpy()
    sizes = dict(info, n=args.n, num_contacts=s.num_contacts, contact_branch=int((~(sep > 0)).sum()),
                 loaded_contacts=int(np.any(f, axis=1).sum()), num_sliding=s.num_sliding,
                 steps=args.profile_steps + 1, carries=max(rebuilds - 1, 0))
    with open(args.sizes, "w") as fh:
        json.dump(sizes, fh)
    return [dict(what="profiled run", **sizes)]


def algorithmic_bytes(sz):
    C, N, A, B = sz["num_contacts"], sz["n"], sz["loaded_contacts"], sz["contact_branch"]
    return {
        # per contact: pair 8 + sep 8 read.  Out of contact: the history and force rows are READ (48) and written only
        # where they are not +0.0 (counted as never).  Contact branch: normal 24 + arclengths 16, history 24 read + 24
        # written, force 24 written.  Per body (gathered, cache resident across its contacts, counted once): previous
        # velocity row 48 + segment record 64 + radius 8 (scalar materials: no gather)
        "k_hertz_friction_force": 16 * C + 48 * (C - B) + 112 * B + 120 * N,
        # entry 4 per half edge and the 24-byte force row per contact (gathered by both half edges, counted once); the
        # 32-byte half-edge record of the half edges whose force is not zero; per body row pointer 4 + mobilities 16 +
        # axis 24 + (U, Z) row 48 + angular velocity 24
        "k_body_vector": 4 * 2 * C + 24 * C + 32 * 2 * A + 116 * N,
        # keys: an old pair 8 read, key 8 + value 4 written.  carry: a new pair 8 read, ~log2(C) probes of the sorted
        # keys that hit cache lines shared with the neighbouring lanes (the lists are sorted alike: counted as one
        # stream of keys and values, 12), the old row 24 read, the new row 24 written
        "k_history_keys": 20 * C,
        "k_history_carry": (8 + 12 + 24 + 24) * C,
    }


def summarize(args):
    import csv
    sz = json.load(open(args.sizes))
    rows = list(csv.DictReader(open(args.summarize)))
    out = []
    for key, b in algorithmic_bytes(sz).items():
        hit = [r for r in rows if key in r["Name"]]
        if not hit:
            out.append(dict(what=key, error="not in the trace"))
            continue
        calls = sum(int(r["Calls"]) for r in hit)
        avg_ms = sum(float(r["TotalDurationNs"]) for r in hit) / calls / 1e6
        out.append(dict(what=key, calls=calls, ms_per_launch=round(avg_ms, 5), algorithmic_bytes=b,
                        achieved_TBps=round(b / (avg_ms * 1e-3) / 1e12, 3),
                        share_of_hbm_peak=round(b / (avg_ms * 1e-3) / th.HBM_PEAK, 3)))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--relax-steps", type=int, default=2)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--rounds", type=int, default=2)
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
