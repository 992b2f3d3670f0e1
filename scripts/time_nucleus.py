"""The chromatin chain step inside its nucleus at full size: the 10^6-bead system of scripts/time_chromatin.py
(synth.chains, ngp_hp1.yaml's numbers) inside a sphere and inside a 3 : 2 : 1.5 ellipsoid of the same volume, sized so
that a few per cent of the beads touch the wall, with active force dipoles on every second backbone spring.

    python scripts/time_nucleus.py [--chains M] [--beads B] [--steps K] [--warmup W] [--touching F] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then for the LCP and the Hertz step: ms per
        step with the keywords off and on (host clock around synchronised steps: medians, min / max), and device-event
        medians of single calls on the state the run has reached: the three periphery kernels, the active springs'
        sample / force / advance, and the backbone spring force.  Each kernel's compulsory bytes (stated below) over its
        median time gives its achieved GB/s, next to k_spring_force's and the copy rate of the same run.
        One JSON object per line to --json (profiles/nucleus_timing.jsonl is written from it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_nucleus.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACTIVE = dict(sigma=1.0, kon=100.0, koff=100.0)
K_WALL = 10.0


def walls(d, touching):
    """a sphere that the outermost `touching` of the beads reach, and the 3 : 2 : 1.5 ellipsoid of its volume"""
    import numpy as np
    pc = 0.5 * (d["center"].min(axis=0) + d["center"].max(axis=0))
    reach = np.linalg.norm(d["center"] - pc, axis=1) + d["radius"]
    R = float(np.quantile(reach, 1.0 - touching))
    s = R / (3.0 * 2.0 * 1.5) ** (1.0 / 3.0)
    pc = [float(v) for v in pc]
    return dict(sphere=dict(shape="sphere", radius=R, k=K_WALL, center=pc),
                ellipsoid=dict(shape="ellipsoid", radii=(3.0 * s, 2.0 * s, 1.5 * s), k=K_WALL, center=pc),
                ellipsoid_fast=dict(shape="ellipsoid_fast", radii=(3.0 * s, 2.0 * s, 1.5 * s), k=K_WALL, center=pc))


def stepper(d, model, periphery=None, active=False):
    import numpy as np
    import torch
    from mundy_amd import pipeline
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    kw = {}
    if periphery is not None:
        kw["periphery"] = periphery
    if active:
        kw["active_forces"] = dict(springs=np.arange(0, d["pairs"].shape[0], 2), **ACTIVE)
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


def kernels(st, wall_specs, reps):
    """single calls on the stepper's current state -> {name: dict(us=, bytes=, GBps=)}.  Compulsory bytes:
    periphery     centre 24 + radius 8 per body, + force read and write 48 per colliding body (accumulate = 1)
    spring force  ptr 4 + two entries 8 + two pairs 16 + own centre 24 + force 24 per body (the neighbours' centres are
                  the adjacent rows: cache hits)
    sample        elapsed 8 + next_time 8 per spring, + key 8, counter 16, state 8, next_time 8, elapsed 8 per switch
    active force  ptr 4 per body, + entry 4 and state 4 per incidence, + pair 8 and two centres 48 per active incidence,
                  + force 48 per touched body (accumulate = 1; an upper bound: a body's rows are shared by its springs)
    advance       elapsed read and write 16 per spring"""
    import torch
    from mundy_amd import ops
    n = st.center.shape[0]
    force = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    stats = (torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.float64, device="cuda"))
    out = {}

    def add(name, fn, nbytes, **extra):
        us = device_us(fn, reps)
        out[name] = dict(us=us, bytes=int(nbytes), GBps=nbytes / (us["median"] * 1e-6) / 1e9, **extra)
    for name, spec in wall_specs.items():
        checked = ops.check_periphery(spec)
        ops.periphery_force(checked, st.center, st.radius, out=force, accumulate=True, stats=stats)
        hit = int(stats[0].item())
        add("periphery_" + name, lambda: ops.periphery_force(checked, st.center, st.radius, out=force, accumulate=True,
                                                            stats=stats), 32 * n + 48 * hit, colliding=hit)
    add("spring_force", lambda: st.springs.force(st.center, out=force), 76 * n)
    act = st.active
    m = act.num_springs
    state, nt, el, ct = act.state()
    sw = torch.zeros(2, dtype=torch.int32, device="cuda")
    na = torch.zeros(1, dtype=torch.int32, device="cuda")
    on = int(state.sum().item())
    add("active_force", lambda: act.force(st.center, out=force, accumulate=True, active=na),
        4 * n + 8 * 2 * m + 56 * 2 * on + 48 * min(n, 2 * on), active=on)
    add("active_advance", lambda: act.advance(0.0), 16 * m)
    # sampling changes the state: every timed call starts from the same one (the reset is outside the events)
    t, switches = [], 0
    for _ in range(reps):
        act.set_state(state, nt, el, ct)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        act.sample(switches=sw)
        b.record()
        torch.cuda.synchronize()
        t.append(1e3 * a.elapsed_time(b))
        switches = int(sw.sum().item())
    act.set_state(state, nt, el, ct)
    t.sort()
    nbytes = 16 * m + 48 * switches
    out["active_sample"] = dict(us=dict(median=t[len(t) // 2], min=t[0], max=t[-1]), bytes=nbytes,
                                GBps=nbytes / (t[len(t) // 2] * 1e-6) / 1e9, switches=switches)
    return out


def main():
    import numpy as np
    import torch
    from mundy_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--touching", type=float, default=0.03)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    d = synth.chains(args.chains, args.beads, seed=1234)
    n = int(d["center"].shape[0])
    w = walls(d, args.touching)
    rate = copy_rate()
    out = [dict(what="setup", n=n, active_springs=(d["pairs"].shape[0] + 1) // 2, chains=args.chains, beads=args.beads,
                steps=args.steps, warmup=args.warmup, device=torch.cuda.get_device_name(), copy_GBps=rate,
                k_wall=K_WALL, sphere_radius=w["sphere"]["radius"], ellipsoid_radii=w["ellipsoid"]["radii"], **ACTIVE)]
    configs = (("off", None, False), ("sphere", w["sphere"], False), ("ellipsoid", w["ellipsoid"], False),
               ("ellipsoid_fast", w["ellipsoid_fast"], False), ("active", None, True),
               ("ellipsoid+active", w["ellipsoid"], True))
    for model in ("lcp", "hertz"):
        for name, per, active in configs:
            st = stepper(d, model, per, active)
            for _ in range(args.warmup):
                st.step()
            torch.cuda.synchronize()
            wall, hit, on = [], [], []
            for _ in range(args.steps):
                t0 = time.perf_counter()
                s = st.step()
                torch.cuda.synchronize()
                wall.append(1e3 * (time.perf_counter() - t0))
                hit.append(s.periphery_colliding)
                on.append(s.active_springs)
            line = dict(what="step", model=model, config=name, ms_per_step_median=float(np.median(wall)),
                        ms_per_step_min=float(np.min(wall)), ms_per_step_max=float(np.max(wall)),
                        colliding_mean=float(np.mean(hit)), active_mean=float(np.mean(on)))
            if per is not None and active and model == "lcp":
                line["kernels"] = kernels(st, w, max(5, args.steps))
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
