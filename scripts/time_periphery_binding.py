"""The chromatin chain step with crosslinkers that also bind to periphery sites (HP1.cpp:3340-3398, :3473-3529; DESIGN.md
5q) at full size: the system of scripts/time_crosslinkers.py (10^6 beads, one crosslinker on every second bead, every
bead a bind site) confined in a sphere about its centroid, with P random bind sites on that sphere.

    python scripts/time_periphery_binding.py [--chains M] [--beads B] [--steps K] [--warmup W] [--sites P [P ...]]
                                             [--root TREE] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then for the LCP and the Hertz step and for
        every P of --sites (default 0 1000 100000; 0: no periphery_sites keyword, the path of before): ms per step (host
        clock around synchronised steps: medians, min / max), and device-event medians per call on the state the run has
        reached -- kmc_step, force and, with sites, the periphery candidate build (the search over beads + sites, forced,
        and set_periphery_candidates).  One JSON object per line to --json.
        --root TREE times the mundy_amd of another checkout (built there): with --sites 0 the script uses nothing that
        the commit before the periphery sites lacks, which gives the A/B of the off path in one session.
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_periphery_binding.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

XL = dict(kind="hookean", k=3.0, r=1.0, bind_rate=100.0, unbind_rate=100.0, kt=0.1, capture_radius=1.5, skin=0.5)
# the reference's defaults for the sites (HP1.cpp:5287-5292): A = 1, k = 1000, r0 = 1; the crosslinkers' k_off and reach
PER = dict(bind_rate=1.0, k=1000.0, r=1.0)


def stepper(d, model, num_sites, wall):
    import numpy as np
    import torch
    from mundy_amd import pipeline, synth
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    n = d["center"].shape[0]
    xl = dict(left=np.arange(0, n, 2), sites=np.ones(n, np.uint8), **XL)
    if num_sites:
        pts = synth.periphery_bind_sites("sphere", wall["radius"], num_sites, seed=1234) + np.asarray(wall["center"])
        xl["periphery_sites"] = dict(points=np.ascontiguousarray(pts), **PER)
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                   search_buffer=d["skin"], contact_model=model,
                                   springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"],
                                   periphery=dict(shape="sphere", k=10.0, **wall), crosslinkers=xl)


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
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sites", type=int, nargs="+", default=[0, 1000, 100000])
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    from mundy_amd import synth
    d = synth.chains(args.chains, args.beads, seed=1234)
    n = int(d["center"].shape[0])
    mid = 0.5 * (d["center"].min(axis=0) + d["center"].max(axis=0))
    wall = dict(center=[float(v) for v in mid],
                radius=float(np.sqrt(((d["center"] - mid) ** 2).sum(axis=1)).max() + 2.0 * d["radius"].max()))
    rate = copy_rate()
    out = [dict(what="setup", n=n, crosslinkers=(n + 1) // 2, chains=args.chains, beads=args.beads, steps=args.steps,
                warmup=args.warmup, device=torch.cuda.get_device_name(), copy_GBps=rate, root=os.path.abspath(args.root),
                wall_radius=wall["radius"], crosslinker=XL, periphery_sites=PER)]
    for model in ("lcp", "hertz"):
        for num_sites in args.sites:
            st = stepper(d, model, num_sites, wall)
            for _ in range(args.warmup):
                st.step()
            torch.cuda.synchronize()
            wall_ms, events = [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                s = st.step()
                torch.cuda.synchronize()
                wall_ms.append(1e3 * (time.perf_counter() - t0))
                events.append(s.crosslinker_binds + s.crosslinker_unbinds)
            line = dict(what="step", model=model, sites=num_sites, ms_per_step_median=float(np.median(wall_ms)),
                        ms_per_step_min=float(np.min(wall_ms)), ms_per_step_max=float(np.max(wall_ms)),
                        events_per_step_mean=float(np.mean(events)), bound=s.crosslinker_bound,
                        periphery_bound=getattr(s, "crosslinker_periphery_bound", 0))
            xl, reps = st.crosslinkers, max(5, args.steps)
            ctr = st.xl_counter.clone()
            ev = torch.zeros(2, dtype=torch.int32, device="cuda")
            force = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
            stats = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
            line["candidates"] = int(st.xl_links.col.shape[0])
            us = dict(kmc_step=device_us(lambda: xl.kmc_step(st.center, st.dt, st.xl_keys, ctr, events=ev), reps),
                      force=device_us(lambda: xl.force(st.center, out=force, stats=stats), reps))
            if num_sites:
                links = st.xl_site_links

                def build():
                    links.generate(None, st._xl_site_all, st._xl_site_reach, force=True)
                    xl.set_periphery_candidates(links.row_ptr, links.col, col_offset=n)
                us["periphery_candidate_build"] = device_us(build, reps)
                us["periphery_candidate_sort"] = device_us(
                    lambda: xl.set_periphery_candidates(links.row_ptr, links.col, col_offset=n), reps)
                line["periphery_candidates"] = int(links.col.shape[0])
                line["periphery_candidate_builds"] = st.crosslinker_site_rebuilds
            line["us"] = us
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
