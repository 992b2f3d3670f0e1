"""The per-body contact force (mundy_hip_contact_force.h) against the vector body sweep of the same build, and the Hertz
chain step with the contact forces inside the hydrodynamic force field against the default order.

    python scripts/time_contact_force.py [--beads 1000000] [--rods 1000000] [--reps 20] [--warmup 3]
                                         [--step-size 100000] [--steps 10] [--copy-gib 1.0] [--json PATH]
        On the Hertz contacts of a chain system of --beads beads (synth.chains, DESIGN 5d's system) and of the bench
        packing of --rods spherocylinders (0 skips either): device events around single calls, median / min / max over
        --reps after --warmup calls, of
          mhip_contact_op_body_force at stride 3 and 6, mhip_contact_op_body_force_vector at stride 6 (of -(x n), the same
          forces), and the yardsticks on the same operator and input: mhip_contact_op_body_sweep_vector (the same index
          and records, 48 bytes written per body) and mhip_contact_op_body_sweep (k_body's X_APPLY sweep);
        algorithmic bytes per call (below) and bytes per second next to a device-to-device copy of --copy-gib GiB timed
        the same way in the same process.  Then the Hertz chain step at --step-size beads with
        hydrodynamics=dict(kind="rpyc") with and without contact_forces=True: ms per step (host clock around synchronised
        steps) and the medians of the stage marks.  One JSON object per line to --json
        (profiles/contact_force_timing.jsonl is written from it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_contact_force.py --rods 0 --steps 0
        per-kernel times of the same calls (k_body_force against k_body_vector).

Algorithmic bytes of one call, C contacts of which A carry a force, N bodies, R = 24 / 48 / 32 bytes of a half-edge record
(spheres / vector arms / rods), g = 8 (scalar) or 24 (vector) bytes gathered per entry:
    2 C (4 + g) + 2 A R + N (8 + 8 stride [+ 24 for a rod's axis])        body force
    2 C (4 + 24) + 2 A R + N (8 + 16 + 48 [+ 24 + 24 for a rod's axis and omega])   vector sweep (mobilities, one row)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_hydro import device_ms  # noqa: E402


def _dev(a):
    import torch
    return torch.from_numpy(a).cuda()


def hertz_operator(kind, n):
    """the stepper's own operator and Hertz forces of the first step of an n-body system -> (stepper, record bytes)"""
    from mundy_amd import pipeline, synth
    if kind == "beads":
        d = synth.chains(max(1, n // 1000), 1000 if n >= 1000 else n, seed=1234)
        st = pipeline.ContactStepper("sphere", _dev(d["center"]), _dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                     search_buffer=d["skin"], contact_model="hertz")
        rec = 24
    else:
        b = synth.spherocylinders(n)
        st = pipeline.ContactStepper("spherocylinder", _dev(b["center"]), _dev(b["radius"]), quat=_dev(b["quat"]),
                                     length=_dev(b["length"]), contact_model="hertz")
        rec = 32
    st.step(integrate=False)
    return st, rec


def call_lines(kind, n, reps, warmup, copy):
    import torch
    st, rec = hertz_operator(kind, n)
    op, lam = st.op, st.lam
    N, C = op.num_bodies, op.num_constraints
    A = int((lam != 0).sum())
    fvec = (-(lam[:, None] * st.contacts["normal"])).contiguous()
    out3 = torch.empty((N, 3), dtype=torch.float64, device="cuda")
    out6 = torch.empty((N, 6), dtype=torch.float64, device="cuda")
    rod = 24 if kind == "rods" else 0
    force_bytes = lambda g, stride: 2 * C * (4 + g) + 2 * A * rec + N * (8 + 8 * stride + rod)  # noqa: E731
    sweep_bytes = 2 * C * (4 + 24) + 2 * A * rec + N * (8 + 16 + 48 + 2 * rod)
    calls = (("body_force_stride3", lambda: op.body_force(lam, out=out3, stride=3), force_bytes(8, 3)),
             ("body_force_stride6", lambda: op.body_force(lam, out=out6, stride=6), force_bytes(8, 6)),
             ("body_force_vector_stride6", lambda: op.body_force_vector(fvec, out=out6, stride=6), force_bytes(24, 6)),
             ("body_sweep_vector", lambda: op.body_sweep_vector(fvec), sweep_bytes),
             ("body_sweep", lambda: op.body_sweep(lam), None))
    lines = [dict(what="system", kind=kind, bodies=N, contacts=C, contacts_with_force=A, record_bytes=rec)]
    for name, fn, nbytes in calls:
        ms = device_ms(fn, reps, warmup)
        line = dict(what=name, kind=kind, bodies=N, us=dict((k, 1e3 * v) for k, v in ms.items()), reps=reps,
                    warmup=warmup)
        if nbytes is not None:
            line.update(algorithmic_bytes=nbytes, gb_per_s=nbytes / (ms["median"] * 1e-3) / 1e9,
                        share_of_copy=nbytes / (ms["median"] * 1e-3) / 1e9 / copy)
        lines.append(line)
    by = {ln["what"]: ln["us"] for ln in lines if "us" in ln}
    y = by["body_sweep_vector"]
    for name in ("body_force_stride3", "body_force_stride6", "body_force_vector_stride6"):
        lines.append(dict(what="ratio", kind=kind, call=name, median_over_body_sweep_vector=by[name]["median"] / y["median"],
                          ranges_overlap=by[name]["min"] <= y["max"] and y["min"] <= by[name]["max"]))
    return lines


def steps(d, hydro, nsteps, warmup):
    import numpy as np
    import torch
    from mundy_amd import pipeline
    st = pipeline.ContactStepper("sphere", _dev(d["center"]), _dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                 search_buffer=d["skin"], springs=(d["pairs"], "hookean", d["k"], d["r0"]),
                                 brownian_kt=d["kt"], contact_model="hertz", hydrodynamics=hydro)
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
    return dict(what="step", n=int(d["center"].shape[0]), contact_model="hertz", hydrodynamics=hydro, steps=nsteps,
                warmup=warmup, ms_per_step_median=float(np.median(wall)), ms_per_step_min=float(np.min(wall)),
                ms_per_step_max=float(np.max(wall)), stage_ms_median={k: float(np.median(v)) for k, v in marks.items()})


def main():
    import torch
    from mundy_amd import synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--beads", type=int, default=1000000)
    ap.add_argument("--rods", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step-size", type=int, default=100000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--copy-gib", type=float, default=1.0)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    words = int(args.copy_gib * 2 ** 30) // 8
    a, b = torch.empty(words, dtype=torch.float64, device="cuda"), torch.empty(words, dtype=torch.float64, device="cuda")
    cp = device_ms(lambda: b.copy_(a), args.reps, args.warmup)
    del a, b
    copy = 2 * 8 * words / (cp["median"] * 1e-3) / 1e9
    out = [dict(what="setup", device=torch.cuda.get_device_name(), copy_gib=args.copy_gib, copy_ms=cp,
                copy_gb_per_s_read_plus_write=copy)]
    for kind, n in (("beads", args.beads), ("rods", args.rods)):
        if n > 0:
            out += call_lines(kind, n, args.reps, args.warmup, copy)
            torch.cuda.empty_cache()
    if args.steps > 0:
        n = args.step_size
        d = synth.chains(max(1, n // 1000), 1000 if n >= 1000 else n, seed=1234)
        out.append(steps(d, dict(kind="rpyc"), args.steps, args.warmup))
        out.append(steps(d, dict(kind="rpyc", contact_forces=True), args.steps, args.warmup))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
