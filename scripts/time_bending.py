"""The bonded force kernels of the semiflexible chain step at full size: the 10^6 beads in 10^3
random-walk chains of 10^3 of scripts/time_chromatin.py (synth.chains), their bonds as Hookean and as FENE-WCA springs
(k_spring_force) and one angular spring per interior bead (k_angular_force, synth.chain_triplets), each timed alone with
device events, next to the device copy rate of the same run.

    python scripts/time_bending.py [--chains M] [--beads B] [--reps K] [--warmup W] [--json PATH]
        median ms per launch, and the GB/s of each kernel's compulsory bytes beside the GB/s of a device
        copy of 3 n doubles in the same run.  One JSON object per line, appended to --json (default
        profiles/bending_timing.jsonl).
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median_ms(fn, reps, warmup):
    import numpy as np
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    import torch
    from mundy_amd import ops, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "bending_timing.jsonl"))
    args = ap.parse_args()
    d = synth.chains(args.chains, args.beads, seed=1234)
    n = int(d["center"].shape[0])
    x = torch.from_numpy(d["center"]).cuda()
    pairs = d["pairs"]
    trip = synth.chain_triplets([c * args.beads for c in range(args.chains + 1)])
    m, ma = int(pairs.shape[0]), int(trip.shape[0])
    force = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    src = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    out = [dict(what="setup", n=n, chains=args.chains, beads=args.beads, springs=m, triplets=ma, reps=args.reps,
                warmup=args.warmup, device=torch.cuda.get_device_name())]
    copy_ms = median_ms(lambda: force.copy_(src), args.reps, args.warmup)
    copy_bytes = 2 * 24 * n
    out.append(dict(what="device copy", ms_median=copy_ms, bytes=copy_bytes, gb_per_s=copy_bytes / copy_ms * 1e-6))
    # compulsory bytes per launch: every body reads its row pointer pair (8), its entries (4 each) and writes its row
    # (24); every entry reads its record (8 a pair, 16 a triplet) and the rows of the record's bodies once per launch at
    # best (24 per body, counted once: neighbours in memory share them through the caches)
    spring_bytes = n * (8 + 24 + 24) + 2 * m * 4 + m * 8
    angular_bytes = n * (8 + 24 + 24) + 3 * ma * 4 + ma * 16
    stats_i = torch.zeros(1, dtype=torch.int32, device="cuda")
    stats_d = torch.zeros(1, dtype=torch.float64, device="cuda")
    for kind, k, r in (("hookean", d["k"], d["r0"]), ("fenewca", 30.0, 1.5)):
        s = ops.Springs(n, pairs, kind, k, r)
        ms = median_ms(lambda: s.force(x, out=force, stats=(stats_i, stats_d)), args.reps, args.warmup)
        out.append(dict(what="k_spring_force", kind=kind, ms_median=ms, compulsory_bytes=spring_bytes,
                        gb_per_s=spring_bytes / ms * 1e-6, of_copy_rate=spring_bytes / ms / (copy_bytes / copy_ms),
                        clamped=int(stats_i.item())))
        s.close()
    a = ops.AngularSprings(n, trip, 4.0, math.pi)
    for accumulate in (False, True):
        ms = median_ms(lambda: a.force(x, out=force, accumulate=accumulate, stats=(stats_i, stats_d)), args.reps,
                       args.warmup)
        nbytes = angular_bytes + (24 * n if accumulate else 0)
        out.append(dict(what="k_angular_force", accumulate=accumulate, ms_median=ms, compulsory_bytes=nbytes,
                        gb_per_s=nbytes / ms * 1e-6, of_copy_rate=nbytes / ms / (copy_bytes / copy_ms),
                        degenerate=int(stats_i.item())))
    a.close()
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "a") as f:
            for line in out:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
