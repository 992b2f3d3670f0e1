"""The backbone segment contacts (segment_contact.hip) at full size: the chain system of scripts/time_chromatin.py (10^6
beads in 10^3 random-walk chains of 10^3, r = 0.5, r0 = 1, k = 3, kT = 0.1, mu = 1, dt = 1e-3), segment radius 0.5, skin
0.3, both laws.

    python scripts/time_backbone_collision.py [--chains M] [--beads B] [--steps K] [--warmup W] [--json PATH]
        per law: device-event medians (min / max) of update (a forced rebuild, and the moved test alone), the linker pass
        and the reduction over K calls at the start positions, each pass's compulsory bytes (bytes_of below) over its
        median as GB/s next to the box's copy rate; then the host clock around whole synchronised steps of the chain step
        with contact_model="none", without the Euler update (see wall_ms).  Beside them the same beads under the
        sphere-Hertz chain step without the term (contact_model="hertz": the step as it was before this term existed,
        which it leaves unchanged).
        One JSON object per line, appended to --json (profiles/backbone_collision_timing.jsonl is written from it).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_filaments import copy_rate  # noqa: E402

RADIUS, SKIN = 0.5, 0.3


def bytes_of(n, m, c, active):
    """Compulsory bytes: every array read or written once.  The two 64-byte segment rows of a linker are gathered rows of
    a per-segment array: counted once per segment."""
    return {
        # per segment: ends 8, two centres 48 (gathered: once per body, 24 n), radius 8; the row 64 and the box 48 written
        "segment_view": m * (8 + 8 + 112) + n * 24,
        # per linker: pair 8, sep 8 and the flag 1 written, the rows force 24 + share 48 read (outside the branch: checked
        # for +0.0) or written (inside); per segment: the row 64
        "linker_pass": c * (8 + 8 + 1 + 72) + m * 64,
        # per segment: ptr 4, correction flag 1, sums 48 written (and the row 64 of a corrected one: ends only, not
        # counted); per entry (two per linker): entry 4, flag 1, and of a linker in the branch force 24, share 24;
        # per body: ptr 4, two entries of 4 and sums rows of 24, the force 24 written
        "reduce": m * 53 + 2 * c * 5 + 2 * active * 48 + n * (4 + 2 * 28 + 24),
    }


def main():
    import numpy as np
    import torch
    from mundy_amd import ops, pipeline, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=1000)
    ap.add_argument("--beads", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    d = synth.chains(args.chains, args.beads, seed=1234)
    n = int(d["center"].shape[0])
    ends = synth.backbone_segments(np.arange(args.chains + 1) * args.beads)
    dev = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rate = copy_rate()
    out = [dict(what="setup", n=n, segments=int(ends.shape[0]), chains=args.chains, beads=args.beads, radius=RADIUS,
                skin=SKIN, k=d["k"], kt=d["kt"], viscosity=d["viscosity"], dt=d["dt"], steps=args.steps,
                warmup=args.warmup, device=torch.cuda.get_device_name(), copy_GBps=rate)]

    def timed(fn, reps):
        t = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t.append(a.elapsed_time(b))
        return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))

    def wall_ms(st):
        # (integrate=False: the random walks start with segments 10^-3 apart, where one WCA step would throw beads out
        #  of any box; every step then evaluates the same positions and neither list is rebuilt after the first)
        for _ in range(args.warmup):
            st.step(integrate=False)
        torch.cuda.synchronize()
        t, stats = [], None
        for _ in range(args.steps):
            t0 = time.perf_counter()
            stats = st.step(integrate=False)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t))), stats

    def stepper(model, backbone):
        return pipeline.ContactStepper("sphere", dev(d["center"]), dev(d["radius"]), dt=d["dt"], viscosity=d["viscosity"],
                                       search_buffer=d["skin"], contact_model=model,
                                       springs=(d["pairs"], "hookean", d["k"], d["r0"]), brownian_kt=d["kt"],
                                       backbone_collision=backbone)

    x = dev(d["center"])
    for kind in ("hertz", "wca"):
        sc = ops.SegmentContacts(n, kind=kind, radius=RADIUS, skin=SKIN, segments=ends)
        f = torch.empty((n, 3), dtype=torch.float64, device="cuda")
        sc.update(x)
        sc.force(x, out=f)
        torch.cuda.synchronize()
        c = sc.num_pairs
        active = sc.read_stats(sc.stats)[1]
        want = bytes_of(n, ends.shape[0], c, active)
        stages = dict(update_rebuild=timed(lambda: sc.update(x, force_rebuild=True), max(3, args.steps // 2)),
                      update_kept=timed(lambda: sc.update(x), args.steps),
                      linker_pass=timed(lambda: sc.linker_pass(), args.steps),
                      reduce=timed(lambda: sc.reduce(out=f), args.steps),
                      force=timed(lambda: sc.force(x, out=f), args.steps))
        gbps = {k: want[k] / stages[k]["median"] / 1e6 for k in ("linker_pass", "reduce")}
        out.append(dict(what="stages", kind=kind, linkers=c, in_force_branch=active, stages_ms=stages, bytes=want,
                        achieved_GBps=gbps))
        sc.close()
        st = stepper("none", dict(kind=kind, radius=RADIUS, skin=SKIN))
        wall, s = wall_ms(st)
        out.append(dict(what="step", contact_model="none", backbone=kind, ms_per_step=wall,
                        num_segment_pairs=s.num_segment_pairs, segment_contacts=s.segment_contacts,
                        max_segment_overlap=s.max_segment_overlap))
        del st
        torch.cuda.empty_cache()
    st = stepper("hertz", None)
    wall, s = wall_ms(st)
    out.append(dict(what="step", contact_model="hertz", backbone=None, ms_per_step=wall, num_contacts=s.num_contacts,
                    max_overlap=s.max_overlap))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "a") as fh:
            for line in out:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
