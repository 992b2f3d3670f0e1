"""The n-body hydrodynamic velocity stage (mhip_hydro_velocity) on chromatin chains (synth.chains, ngp_hp1.yaml's numbers,
seeded normal forces on every bead).

    python scripts/time_hydro.py [--sizes 10000 30000 100000] [--kinds stokes rpy rpyc] [--reps 20] [--warmup 3]
                                 [--step-size 100000] [--steps 10] [--json PATH]
        beads-to-beads calls for every kind and size: device events around single calls, median / min / max over --reps
        after --warmup calls, for the launch rule's shape and for each forced shape (in_lane, partial); pair terms per
        second, counted flops per pair (below) and the share of the fp64 vector peak bench.py uses.  Then the chain step
        (LCP) at --step-size beads with and without hydrodynamics=: ms per step (host clock around synchronised steps) and
        the medians of the stage marks.  One JSON object per line to --json (profiles/hydro_timing.jsonl is written from
        it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_hydro.py --sizes 100000 --kinds rpyc --steps 0
        per-kernel times of the same calls: k_hydro against k_hydro_reduce is the share of the ordered second pass.

Counted flops per pair term (each + - * / sqrt once, as written in hydro.hip, the three adds into the sum included; the
integer operations of quake_inv_sqrt and the comparisons are not counted):
    stokes 36   3 d, 5 r2, 5 quake, 2 rinv3, 5 f.d, 1 scale rinv3, 12 the three components, 3 sum
    rpy    71   3 d, 2 a^2/3, 5 r2, 5 quake, 4 rinv3 rinv5, 5 f.d, 2 3(f.d)rinv5, 9 c, 1 (f.d)rinv3, 18 v, 6 lap, 2 b^2/6,
                6 v + lap, 3 sum
    rpyc   47   the far branch, which all but a few pairs per bead take: 3 d, 5 r2, 1 sqrt, 1 r3, 1 divide, 2 rinv2
                rinv3, 3 h, 5 f.h, 2 a^2 b^2, 2 q, 1 s, 5 t1 t2, 1 a + b, 12 the three components, 3 sum
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOPS_PER_PAIR = dict(stokes=36, rpy=71, rpyc=47)
PEAK_FP64_VECTOR = 78.6e12  # bench.py's figure for the MI355X


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
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def system(n):
    import numpy as np
    from mundy_amd import synth
    d = synth.chains(max(1, n // 1000), 1000 if n >= 1000 else n, seed=1234)
    d["force"] = np.random.default_rng(7).normal(size=d["center"].shape)
    return d


def calls(d, kinds, reps, warmup):
    import torch
    from mundy_amd import ops
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    c, r, f = dev(d["center"]), dev(d["radius"]), dev(d["force"])
    n = int(c.shape[0])
    out = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    ws = ops.HydroWorkspace()
    lines = []
    for kind in kinds:
        for path in ("auto", "in_lane", "partial"):
            ws.set_path(path)
            ms = device_ms(lambda: ops.hydro_velocity(kind, d["viscosity"], c, r, f, out=out, workspace=ws), reps,
                           warmup)
            pairs_per_s = n * n / (ms["median"] * 1e-3)
            flops = FLOPS_PER_PAIR[kind] * pairs_per_s
            lines.append(dict(what="call", kind=kind, n=n, path=path, path_taken=ws.last_path(), ms=ms,
                              pair_terms_per_s=pairs_per_s, flops_per_pair=FLOPS_PER_PAIR[kind], flop_per_s=flops,
                              share_of_fp64_vector_peak=flops / PEAK_FP64_VECTOR, reps=reps, warmup=warmup))
    ws.close()
    return lines


def steps(d, hydro, nsteps, warmup):
    import numpy as np
    import torch
    from mundy_amd import pipeline
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    kw = {} if hydro is None else dict(hydrodynamics=hydro)
    st = pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"], **kw)
    for _ in range(warmup):
        st.step()
    torch.cuda.synchronize()
    wall, marks = [], {}
    for _ in range(nsteps):
        t0 = time.perf_counter()
        s = st.step(timed=True)
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        for k, v in s.timings_ms.items():
            marks.setdefault(k, []).append(v)
    return dict(what="step", n=int(d["center"].shape[0]), hydrodynamics=hydro, steps=nsteps, warmup=warmup,
                ms_per_step_median=float(np.median(wall)), ms_per_step_min=float(np.min(wall)),
                ms_per_step_max=float(np.max(wall)), stage_ms_median={k: float(np.median(v)) for k, v in marks.items()})


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[10000, 30000, 100000])
    ap.add_argument("--kinds", nargs="*", default=["stokes", "rpy", "rpyc"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-size", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = [dict(what="setup", device=torch.cuda.get_device_name(), peak_fp64_vector=PEAK_FP64_VECTOR,
                flops_per_pair=FLOPS_PER_PAIR)]
    for n in args.sizes:
        out += calls(system(n), args.kinds, args.reps, args.warmup)
    by = {(ln["kind"], ln["n"]): ln["pair_terms_per_s"] for ln in out if ln["what"] == "call" and ln["path"] == "auto"}
    if args.sizes:
        lo, hi = min(args.sizes), max(args.sizes)
        for kind in args.kinds:
            out.append(dict(what="ratio", kind=kind, n_small=lo, n_large=hi,
                            pair_rate_small_over_large=by[(kind, lo)] / by[(kind, hi)]))
    if args.steps > 0:
        d = system(args.step_size)
        out.append(steps(d, None, args.steps, args.warmup))
        out.append(steps(d, dict(kind="rpyc"), args.steps, args.warmup))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
