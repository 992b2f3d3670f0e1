"""The inertial filament step at full size, at the configuration of scripts/time_filaments.py: 999 922
nodes in 3 322 filaments of 301 (synth.filaments), wave and monolayer on.

    python scripts/time_filament_inertial.py [--nodes N] [--per-filament B] [--steps K] [--warmup W] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then device-event medians (min / max) over K
        real steps each of: the inertial loop with the kinetic energy (predict, edge pass + node pass, correct + fold),
        the inertial loop without it (correct alone), and the overdamped loop of the same filaments (advance, force,
        velocity); the host clock around whole synchronised steps of the inertial and of the overdamped stepper.  Each
        element-wise kernel's compulsory bytes (BYTES below) over its median time gives its achieved GB/s and its
        fraction of the copy rate.  One JSON object per line, appended to --json
        (profiles/filament_inertial_timing.jsonl).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_filaments import BYTES as OVERDAMPED_BYTES, DT, PARAMS, WAVE, copy_rate  # noqa: E402

DYNAMICS = dict(density=1.0, damping="critical")
# Compulsory bytes per node with monolayer on and twist on: every array a kernel must read or write once.
BYTES = {
    # read center 24, velocity 24, acceleration 24, twist 8, twist velocity 8, twist acceleration 8; write center 24,
    # twist 8 and, for the monolayer, component 0 of velocity and acceleration 8 + 8 (128 without the monolayer)
    "predict": 96 + 48,
    # read radius 8, force 24, twist torque 8, velocity 24, acceleration 24, twist velocity 8, twist acceleration 8,
    # center 24, twist 8; write center 24, twist 8, velocity 24, acceleration 24, twist velocity 8, twist acceleration 8.
    # The kinetic energy adds 16 bytes per workgroup of 256 nodes and a fold over at most 2048 pairs: nothing per node.
    "correct": 136 + 96,
    "correct_with_energy": 136 + 96,
    "advance": OVERDAMPED_BYTES["advance"],
    "velocity": OVERDAMPED_BYTES["velocity"],
}


def timed_steps(calls, first, steps):
    """`steps` real steps of a loop given as (name, fn(k)) calls, an event pair around each call -> ({name: [us]},
    [host ms per synchronised step])"""
    import torch
    times, wall = {name: [] for name, _ in calls}, []
    for k in range(first, first + steps):
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
    return times, wall


def main():
    import numpy as np
    import torch
    from mundy_amd import pipeline, synth
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
                warmup=args.warmup, dt=DT, device=torch.cuda.get_device_name(), copy_GBps=rate, wave=WAVE,
                dynamics=DYNAMICS, **PARAMS)]

    def stepper(dynamics):
        return pipeline.FilamentStepper(d["node_ptr"], d["center"], d["radius"], d["edge_orientation"], d["arclength"],
                                        phase=d["phase"], wave=WAVE, monolayer=True, dynamics=dynamics, **PARAMS)

    def summary(times, wall):
        kernels = {}
        for name, t in times.items():
            med = float(np.median(t))
            k = dict(us=dict(median=med, min=float(np.min(t)), max=float(np.max(t))))
            if name in BYTES:
                k.update(bytes=BYTES[name] * n, GBps=BYTES[name] * n / (med * 1e-6) / 1e9)
                k["fraction_of_copy_rate"] = k["GBps"] / rate["median"]
            kernels[name] = k
        return dict(ms_per_step_median=float(np.median(wall)), ms_per_step_min=float(np.min(wall)),
                    ms_per_step_max=float(np.max(wall)), kernels=kernels)

    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    energy = torch.zeros(1, dtype=torch.float64, device="cuda")
    # the inertial loop, with the kinetic energy and then without it
    st = stepper(DYNAMICS)
    for _ in range(args.warmup):
        st.step(DT, read_stats=False)
    torch.cuda.synchronize()
    f = st.filaments
    force = ("force", lambda k: f.force(k * DT, None, stats))
    times, wall = timed_steps((("predict", lambda k: f.predict(DT)), force,
                               ("correct_with_energy", lambda k: f.correct(DT, energy))), args.warmup, args.steps)
    out.append(dict(what="inertial_step_with_energy", kinetic_energy=float(energy[0]), **summary(times, wall)))
    times, wall = timed_steps((("predict", lambda k: f.predict(DT)), force, ("correct", lambda k: f.correct(DT))),
                              args.warmup + args.steps, args.steps)
    out.append(dict(what="inertial_step", max_stretch=stats.tolist()[0], **summary(times, wall)))
    st.close()
    # the overdamped loop of the same filaments, in the same run
    st = stepper(None)
    for _ in range(args.warmup):
        st.step(DT, read_stats=False)
    torch.cuda.synchronize()
    f = st.filaments
    times, wall = timed_steps((("advance", lambda k: f.advance(DT)), ("force", lambda k: f.force(k * DT, None, stats)),
                               ("velocity", lambda k: f.velocity())), args.warmup, args.steps)
    out.append(dict(what="overdamped_step", max_stretch=stats.tolist()[0], **summary(times, wall)))
    st.close()
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "a") as fh:
            for line in out:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
