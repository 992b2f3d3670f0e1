"""The chromatin chain step (NgpHP1.cpp:3802-3990) at full size: 10^6 beads in 10^3 random-walk chains of 10^3
(synth.chains, ngp_hp1.yaml's r = 0.5, r0 = 1, k = 3, kT = 0.1, mu = 1, dt = 1e-3, skin 1.0), Hookean springs and
Brownian noise, with the LCP and with Hertz contact.

    python scripts/time_chromatin.py [--chains M] [--beads B] [--steps K] [--warmup W] [--json PATH]
        ms per step (host clock around synchronised steps), contacts and solver iterations, then the stages of
        separate steps from device events (step(timed=True)); springs_brownian is the three new kernels (spring force,
        drag velocity, Brownian velocity).  One JSON object per line to --json.
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_chromatin.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stepper(d, model):
    import torch
    from mundy_amd import pipeline
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                   search_buffer=d["skin"], contact_model=model,
                                   springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"])


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
    out = [dict(what="setup", n=int(d["center"].shape[0]), chains=args.chains, beads=args.beads, k=d["k"],
                kt=d["kt"], viscosity=d["viscosity"], dt=d["dt"], skin=d["skin"], steps=args.steps,
                warmup=args.warmup, device=torch.cuda.get_device_name())]
    for model in ("lcp", "hertz"):
        st = stepper(d, model)
        for _ in range(args.warmup):
            st.step()
        torch.cuda.synchronize()
        wall, contacts, iters, rebuilt = [], [], [], []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            s = st.step()
            torch.cuda.synchronize()
            wall.append(1e3 * (time.perf_counter() - t0))
            contacts.append(s.num_contacts)
            iters.append(s.num_iters)
            rebuilt.append(s.rebuilt)
        stages = {}
        for _ in range(max(3, args.steps // 4)):
            s = st.step(timed=True)
            for k, v in s.timings_ms.items():
                stages.setdefault(k, []).append(v)
        med = {k: float(np.median(v)) for k, v in stages.items()}
        tot = sum(med.values())
        out.append(dict(what="step", model=model, ms_per_step_median=float(np.median(wall)),
                        ms_per_step_mean=float(np.mean(wall)), contacts_mean=float(np.mean(contacts)),
                        iterations_mean=float(np.mean(iters)), rebuilds=int(sum(rebuilt)),
                        stages_ms_median=med, springs_brownian_share=med.get("springs_brownian", 0.0) / tot if tot else 0.0))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
