"""The centerline-twist filament step at full size: 10^6 nodes in filaments of 301 nodes (synth.filaments, the sperm apps'
layout), with the travelling rest-curvature wave on.

    python scripts/time_filaments.py [--nodes N] [--per-filament B] [--steps K] [--warmup W] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then over K real steps of the stepper's loop
        device-event medians (min / max) of each of its four kernels -- advance, edge pass, node pass, node drag -- and
        the host clock around whole synchronised steps; k_spring_force over the same nodes chained as Hookean springs,
        in the same run.  Each kernel's compulsory bytes (stated in BYTES below) over its median time gives its achieved
        GB/s, next to k_spring_force's and the copy rate.  One JSON object per line to --json
        (profiles/filament_timing.jsonl is written from it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_filaments.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARAMS = dict(youngs_modulus=10.0, poisson_ratio=0.3, rest_length=1.0, viscosity=1.0)
WAVE = dict(amplitude=0.1, wave_number=0.2, frequency=1.0)
DT = 0.01

# Compulsory bytes per node: every array a kernel must read or write once.  A neighbour's row (x[i + 1], radius[i + 1],
# the tile's three halo edges, phase[f]) is an adjacent row that the same or the next wave fetches anyway: a cache hit.
BYTES = {
    # read center 24, velocity 24, twist 8, twist velocity 8; write center 24, twist 8 and the four zeroed fields
    # velocity 24, force 24, twist velocity 8, twist torque 8
    "advance": 64 + 96,
    # read flag 1, center 24, twist 8, old tangent 24, old orientation 32; write tangent 24, binormal 24, length 8,
    # orientation 32
    "edge_pass": 89 + 88,
    # read flag 1, filament 4, radius 8, rest curvature 24, arclength 8, the edge record 88; write force 24, twist torque
    # 8, curvature 24
    "node_pass": 133 + 56,
    # read radius 8, force 24, twist torque 8; write velocity 24, twist velocity 8
    "velocity": 40 + 32,
    # ptr 4 + two entries 8 + two pairs 16 + own centre 24 + force 24 (scripts/time_nucleus.py)
    "spring_force": 76,
}


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
    from mundy_amd import ops, pipeline, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1000000)
    ap.add_argument("--per-filament", type=int, default=301)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    F = max(1, round(args.nodes / args.per_filament))
    d = synth.filaments(F, args.per_filament, radius=0.5, segment_length=1.0, seed=1234)
    n = int(d["center"].shape[0])
    rate = copy_rate()
    out = [dict(what="setup", n=n, filaments=F, nodes_per_filament=args.per_filament, steps=args.steps,
                warmup=args.warmup, dt=DT, device=torch.cuda.get_device_name(), copy_GBps=rate, wave=WAVE, **PARAMS)]
    st = pipeline.FilamentStepper(d["node_ptr"], d["center"], d["radius"], d["edge_orientation"], d["arclength"],
                                  phase=d["phase"], wave=WAVE, monolayer=True, **PARAMS)
    for _ in range(args.warmup):
        st.step(DT, read_stats=False)
    torch.cuda.synchronize()
    f = st.filaments
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    calls = (("advance", lambda k: f.advance(DT)), ("edge_pass", lambda k: f.edge_pass()),
             ("node_pass", lambda k: f.node_pass(k * DT, None, stats)), ("velocity", lambda k: f.velocity()))
    times = {name: [] for name, _ in calls}
    wall = []
    for k in range(args.warmup, args.warmup + args.steps):   # the stepper's own loop, an event pair around each call
        t0 = time.perf_counter()
        ev = []
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k)
            b.record()
            ev.append((name, a, b))
        torch.cuda.synchronize()
        wall.append(1e3 * (time.perf_counter() - t0))
        for name, a, b in ev:
            times[name].append(1e3 * a.elapsed_time(b))
    worst = stats.tolist()
    kernels = {}
    for name, t in times.items():
        med = float(np.median(t))
        kernels[name] = dict(us=dict(median=med, min=float(np.min(t)), max=float(np.max(t))), bytes=BYTES[name] * n,
                             GBps=BYTES[name] * n / (med * 1e-6) / 1e9)
    # the spring force of the chain step over the same nodes, chained node to node along every filament
    first = np.arange(n).reshape(F, args.per_filament)[:, :-1].reshape(-1)
    springs = ops.Springs(n, np.stack([first, first + 1], axis=1), "hookean", 3.0, 1.0)
    center = f.field("center")
    force = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    springs.force(center, out=force)
    us = device_us(lambda: springs.force(center, out=force), args.steps)
    kernels["spring_force"] = dict(us=us, bytes=BYTES["spring_force"] * n,
                                   GBps=BYTES["spring_force"] * n / (us["median"] * 1e-6) / 1e9)
    for k in kernels.values():
        k["fraction_of_copy_rate"] = k["GBps"] / rate["median"]
    out.append(dict(what="step", ms_per_step_median=float(np.median(wall)), ms_per_step_min=float(np.min(wall)),
                    ms_per_step_max=float(np.max(wall)), max_stretch=worst[0], max_curvature_deviation=worst[1],
                    kernels=kernels))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as fh:
            for line in out:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
