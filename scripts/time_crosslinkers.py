"""The chromatin chain step with its crosslinker KMC stage (HP1.cpp:4728-4739) at full size: the 10^6-bead system of
scripts/time_chromatin.py (synth.chains, ngp_hp1.yaml's numbers) with one crosslinker on every second bead, every bead
a bind site.

    python scripts/time_crosslinkers.py [--chains M] [--beads B] [--steps K] [--warmup W] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then for the LCP and the Hertz step: ms per
        step with crosslinkers off and on (host clock around synchronised steps: medians, min / max), and device-event
        medians of the four crosslinker stages on the state the run has reached -- candidate sort (set_candidates on
        the current list), KMC kernel + incidence rebuild (kmc_step), the rebuild on its own (set_state) and the force.
        One JSON object per line to --json (default profiles/crosslinker_timing.jsonl is written by hand from it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_crosslinkers.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

XL = dict(kind="hookean", k=3.0, r=1.0, bind_rate=100.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5, skin=0.5)


def stepper(d, model, crosslinkers):
    import numpy as np
    import torch
    from mundy_amd import pipeline
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    n = d["center"].shape[0]
    kw = {}
    if crosslinkers:
        kw["crosslinkers"] = dict(left=np.arange(0, n, 2), sites=np.ones(n, np.uint8), **XL)
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                   search_buffer=d["skin"], contact_model=model,
                                   springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"], **kw)


def device_us(fn, reps):
    """median / min / max device time of fn() in microseconds, from events around single calls"""
    import numpy as np
    import torch
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(1e3 * a.elapsed_time(b))
    return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))


def copy_rate(nbytes=1 << 30, reps=10):
    """GB/s (read + write) of a device-to-device copy: the ceiling the kernels' compulsory bytes are set against"""
    import torch
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    dst.copy_(src)
    us = device_us(lambda: dst.copy_(src), reps)
    gbps = lambda t: 2.0 * nbytes / (t * 1e-6) / 1e9  # noqa: E731
    return dict(median=gbps(us["median"]), min=gbps(us["max"]), max=gbps(us["min"]))


def main():
    import numpy as np
    import torch
    from mundy_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    d = synth.chains(args.chains, args.beads, seed=1234)
    n = int(d["center"].shape[0])
    rate = copy_rate()
    out = [dict(what="setup", n=n, crosslinkers=(n + 1) // 2, chains=args.chains, beads=args.beads, steps=args.steps,
                warmup=args.warmup, device=torch.cuda.get_device_name(), copy_GBps=rate, **XL)]
    for model in ("lcp", "hertz"):
        for on in (False, True):
            st = stepper(d, model, on)
            for _ in range(args.warmup):
                st.step()
            torch.cuda.synchronize()
            wall, binds, bound = [], [], 0
            for _ in range(args.steps):
                t0 = time.perf_counter()
                s = st.step()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                binds.append(s.crosslinker_binds + s.crosslinker_unbinds)
                bound = s.crosslinker_bound
            line = dict(what="step", model=model, crosslinkers=on, ms_per_step_median=float(np.median(wall)),
                        ms_per_step_min=float(np.min(wall)), ms_per_step_max=float(np.max(wall)),
                        events_per_step_mean=float(np.mean(binds)), bound=bound)
            if on:
                xl, reps = st.crosslinkers, max(5, args.steps)
                ctr = st.xl_counter.clone()
                le, ri = st.crosslinker_state()
                ev = torch.zeros(2, dtype=torch.int32, device="cuda")
                force = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
                stats = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
                line["candidates"] = int(st.xl_links.col.shape[0])
                line["candidate_builds"] = st.crosslinker_rebuilds
                line["us"] = dict(
                    candidate_sort=device_us(lambda: xl.set_candidates(st.xl_links.row_ptr, st.xl_links.col, st.ids), reps),
                    kmc_step=device_us(lambda: xl.kmc_step(st.center, st.dt, st.xl_keys, ctr, events=ev), reps),
                    incidence_rebuild=device_us(lambda: xl.set_state(None, ri), reps),
                    force=device_us(lambda: xl.force(st.center, out=force, stats=stats), reps),
                    spring_force=device_us(lambda: st.springs.force(st.center, out=force), reps))
            out.append(line)
            del st
            torch.cuda.empty_cache()
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
