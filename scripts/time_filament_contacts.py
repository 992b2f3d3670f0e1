"""The colliding filaments' step at full size: about 10^6 nodes in two crossed layers (synth.crossed_filaments) with a skin
of 2 r, the travelling rest-curvature wave on.

    python scripts/time_filament_contacts.py [--per-filament B] [--steps K] [--warmup W] [--json PATH]
        the box's copy rate in this run (device-to-device, read + write), then over K real steps of the stepper's loop
        device-event medians (min / max) of each contact kernel -- velocity copy, segment view, linker pass, reduction --
        next to the four filament kernels, the host clock around whole synchronised steps with the contacts, and the same
        for a second stepper over the same filaments without them.  Each kernel's compulsory bytes (stated in bytes_of
        below) over its median time gives its achieved GB/s, next to the copy rate.  One JSON object per line to --json
        (profiles/filament_contact_timing.jsonl is written from it).
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/time_filament_contacts.py --steps 5 --warmup 1
        per-kernel times of the same run.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from time_filaments import BYTES as FILAMENT_BYTES, DT, PARAMS, WAVE, copy_rate  # noqa: E402

CONTACTS = dict(skin=1.0, youngs_modulus=200.0, poisson_ratio=0.3, mu=0.5)


def bytes_of(n, c, touching):
    """Compulsory bytes of the contact kernels: every array read or written once.  The two 64-byte segment records of a
    linker and the velocities of a contact's four nodes are gathered rows of per-node arrays: counted once per node."""
    return {
        "save_velocity": n * (24 + 24),
        # read flag 1, centre 24, radius 8; write the record 64 and the box 48
        "segment_view": n * (33 + 112),
        # per linker: pair 8, sep 8 written, and the rows tang_disp 24 + force 24 + share 48 read (separated: checked for
        # +0.0) or written (touching: tang_disp also read); per node: the record 64, once
        "linker_pass": c * (16 + 96) + touching * 24 + n * 64,
        # per node: flag 1, ptr 4, node_force 24 written; per entry (two per linker): entry 4, sep 8, and of a touching
        # linker force 24, share 24
        "reduce": n * 29 + 2 * c * 12 + 2 * touching * 48,
    }


def main():
    import numpy as np
    import torch
    from mundy_amd import pipeline, synth
    ap = argparse.ArgumentParser()
    ap.add_argument("--per-filament", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    B = args.per_filament
    F = B // 2   # the layers' pitch is about two segment lengths: a square patch, every filament crosses every other
    d = synth.crossed_filaments(F, B, radius=0.5, segment_length=1.0, overlap=0.02, seed=1234)
    n = int(d["center"].shape[0])
    rate = copy_rate()
    out = [dict(what="setup", n=n, filaments=2 * F, nodes_per_filament=B, steps=args.steps, warmup=args.warmup, dt=DT,
                device=torch.cuda.get_device_name(), copy_GBps=rate, wave=WAVE, contacts=CONTACTS, **PARAMS)]

    def stepper(contacts):
        return pipeline.FilamentStepper(d["node_ptr"], d["center"], d["radius"], d["edge_orientation"], d["arclength"],
                                        phase=d["phase"], wave=WAVE, contacts=contacts, **PARAMS)

    def wall_ms(st):
        for _ in range(args.warmup):
            st.step(DT, read_stats=False)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            st.step(DT, read_stats=False)
            torch.cuda.synchronize()
            t.append(1e3 * (time.perf_counter() - t0))
        return dict(median=float(np.median(t)), min=float(np.min(t)), max=float(np.max(t)))

    plain = stepper(None)
    without = wall_ms(plain)
    plain.close()
    st = stepper(CONTACTS)
    with_contacts = wall_ms(st)
    f, c = st.filaments, st.contacts
    fstats = torch.zeros(2, dtype=torch.float64, device="cuda")
    cstats = torch.zeros(2, dtype=torch.float64, device="cuda")
    rebuilds = []
    # the stepper's own loop, an event pair around each call; update = segment view, the moved check and its read
    calls = (("save_velocity", lambda k: c.save_velocity()), ("advance", lambda k: f.advance(DT)),
             ("segment_view", lambda k: c.segment_view()), ("update", lambda k: rebuilds.append(c.update())),
             ("linker_pass", lambda k: c.linker_pass(DT, cstats)), ("reduce", lambda k: c.reduce()),
             ("edge_pass", lambda k: f.edge_pass()),
             ("node_pass", lambda k: f.node_pass(k * DT, c.node_force_ptr(), fstats)),
             ("velocity", lambda k: f.velocity()))
    times = {name: [] for name, _ in calls}
    first = st.step_index
    for k in range(first, first + args.steps):
        ev = []
        for name, fn in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(k)
            b.record()
            ev.append((name, a, b))
        torch.cuda.synchronize()
        for name, a, b in ev:
            times[name].append(1e3 * a.elapsed_time(b))
    pairs = c.num_pairs
    touching = int((c.field("sep") <= 0.0).sum().item())
    h = cstats.cpu()
    nbytes = dict(bytes_of(n, pairs, touching), **{k: v * n for k, v in FILAMENT_BYTES.items()})
    kernels = {}
    for name, t in times.items():
        med = float(np.median(t))
        kernels[name] = dict(us=dict(median=med, min=float(np.min(t)), max=float(np.max(t))))
        if name in nbytes:
            kernels[name].update(bytes=nbytes[name], GBps=nbytes[name] / (med * 1e-6) / 1e9,
                                 fraction_of_copy_rate=nbytes[name] / (med * 1e-6) / 1e9 / rate["median"])
    out.append(dict(what="step", ms_per_step_with_contacts=with_contacts, ms_per_step_without_contacts=without,
                    num_pairs=pairs, touching=touching, rebuilds_in_timed_steps=int(sum(rebuilds)),
                    max_overlap=float(h[0]), num_sliding=int(h.view(torch.int64)[1]), kernels=kernels))
    for line in out:
        print(json.dumps(line))
    if args.json:
        with open(args.json, "w") as fh:
            for line in out:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
