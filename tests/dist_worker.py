"""Worker of tests/test_gpu_distributed.py: `python -m torch.distributed.run --nproc-per-node W tests/dist_worker.py`.
All ranks share cuda:0 (gloo carries the halo through the host), each owns a Hilbert range of one global rod system;
rank 0 also solves the whole system on one rank and checks the distributed result against it."""
import gc
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    n_total = int(os.environ.get("DIST_BODIES", "12000"))
    tol = 1e-5
    dist.init_process_group(backend="gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    torch.cuda.set_device(0)
    from mundy_amd import capi, distributed as D, ops, pipeline, synth

    mixed = os.environ.get("DIST_MIXED", "0") == "1"   # BASELINE configs[4]: spheres + rods + ellipsoids
    phi, buf = float(os.environ.get("DIST_PHI", "0.4")), float(os.environ.get("DIST_BUFFER", "0.1"))
    seed = int(os.environ.get("DIST_SEED", "7"))     # 1234 at 10^6 bodies = the bench system (configs[3])
    b = synth.mixed_bodies(n_total, volume_fraction=0.25, seed=seed) if mixed else \
        synth.spherocylinders(n_total, seed=seed, volume_fraction=phi)
    order = D.hilbert_order(b["center"], 0.0, b["box"], level=5 if n_total < 200_000 else 7)
    starts = D.partition_ranges(n_total, world)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    g_center, g_quat = b["center"][order], b["quat"][order]
    a, e = int(starts[rank]), int(starts[rank + 1])
    cfg = ops.PGDConfig(max_iters=20000, tol=tol)
    D.Comm().self_check()

    def make_comm():   # DIST_NO_MAILBOX: the reduction records through the transport's all-gather, as on several nodes
        # DIST_NO_HALO_IPC: the velocity halo of the iteration through the transport's send / recv instead of the inboxes
        comm = D.Comm(mailbox=not os.environ.get("DIST_NO_MAILBOX"), halo_ipc=not os.environ.get("DIST_NO_HALO_IPC"))
        assert not (comm.mailbox and os.environ.get("DIST_NO_MAILBOX"))
        assert not (comm.halo_ipc and os.environ.get("DIST_NO_HALO_IPC"))
        # (a box that refuses fine-grained IPC memory leaves everybody on the all-gather: the solve must not care;
        # test_mailbox_opens_between_the_ranks_of_the_test_box is the one that insists)
        print("MAILBOX rank %d opened %d" % (rank, int(comm.mailbox)), flush=True)
        return comm
    if mixed:
        g_kind, g_shape = b["kind"][order], b["shape"][order]
        st = D.DistributedContactStepper(dev(g_center[a:e]), dev(g_quat[a:e]), None, None, a, comm=make_comm(),
                                         search_buffer=buf, cfg=cfg, poll_every=8, kind=dev(g_kind[a:e]),
                                         shape=dev(g_shape[a:e]))
    else:
        g_radius, g_length = b["radius"][order], b["length"][order]
        st = D.DistributedContactStepper(dev(g_center[a:e]), dev(g_quat[a:e]), dev(g_radius[a:e]), dev(g_length[a:e]),
                                         a, comm=make_comm(), search_buffer=buf, cfg=cfg,
                                         poll_every=int(os.environ.get("DIST_POLL", "8")),
                                         domain=(0.0, b["box"]), curve_level=4, recut_every=3)
    # DIST_TIER: cold tier mode of every rank's operator (3 = tier whatever the size, 2 = and leave the tiers mid-solve)
    if os.environ.get("DIST_TIER"):
        st.tiering = int(os.environ["DIST_TIER"])
    # DIST_FAULT: the first solve ends in an injected error (mhip_comm_inject_fault), the checked one comes after it.
    #   sym   every rank fails at its second poll (8 iterations enqueued everywhere); the next solve reuses the ghost plan
    #         and the inboxes as they are: the exchange numbers of the failed solve were retired on every rank
    #   asym  only the last rank fails; the others run on, time out waiting for its words (bound set to 3 s) and fail one
    #         poll later with MORE iterations enqueued: the ranks now disagree on the numbers, and the next ghost plan
    #         (a rebuild) re-agrees them
    fault = os.environ.get("DIST_FAULT")
    if fault:
        st.comm.set_exchange_timeout(3.0)
        if fault == "sym" or rank == world - 1:
            st.comm.inject_fault(2)
        try:
            st.step(integrate=False)
            failed = False
        except RuntimeError as e:
            failed = True
            print("FAULT rank %d: %s" % (rank, str(e)[:160]), flush=True)
        assert failed, "the injected fault did not end the solve on rank %d" % rank
        stats = st.step(integrate=False, force_rebuild=(fault != "sym"))
        assert stats["rebuilt"] == (fault != "sym")
    else:
        stats = st.step(integrate=False)
    print("HALO_IPC rank %d active %d" % (rank, int(st.comm.halo_ipc_active())), flush=True)
    tier_stats = st.op.tier_stats() if st.op is not None else {}
    gid = st.local["gid"].cpu().numpy().astype(np.int64)
    pairs = st.pairs.cpu().numpy()
    out = dict(stats=stats, gpairs=gid[pairs], counted=st.counted.cpu().numpy().astype(bool),
               g=st.grad.cpu().numpy(), x=st.lam.cpu().numpy(),
               vel=st.op.body_velocity()[st.n_lo:st.n_lo + st.n].cpu().numpy(), first=a, tier=tier_stats)
    gathered = [None] * world if rank == 0 else None
    dist.gather_object(out, gathered, dst=0)
    ok = True
    if rank == 0:
        if mixed:
            ref = pipeline.ContactStepper("mixed", dev(g_center), None, dev(g_quat), search_buffer=buf, cfg=cfg,
                                          kinds=dev(g_kind), shape=dev(g_shape))
        else:
            ref = pipeline.ContactStepper("spherocylinder", dev(g_center), dev(g_radius), dev(g_quat), dev(g_length),
                                          search_buffer=buf, cfg=cfg)
        rs = ref.step(integrate=False)
        rp = ref.links.pairs.cpu().numpy().astype(np.int64)
        rg = (ref.op.apply(ref.lam) + ref.contacts["sep"]).cpu().numpy()
        rvel = ref.op.body_velocity().cpu().numpy()
        key = lambda p: p[:, 0] * n_total + p[:, 1]  # noqa: E731
        allp = np.concatenate([o["gpairs"][o["counted"]] for o in gathered])
        allg = np.concatenate([o["g"][o["counted"]] for o in gathered])
        allx = np.concatenate([o["x"][o["counted"]] for o in gathered])
        srt = np.argsort(key(allp))
        checks = {}
        checks["pair set == single-rank neighbour list"] = np.array_equal(allp[srt], rp)
        if os.environ.get("DIST_TIER"):   # the staged solve of every rank did renumber its contacts hot-first
            checks["cold tier active on every rank: renumberings %s" % [o["tier"].get("renumberings") for o in gathered]] = \
                all(o["tier"].get("renumberings", 0) >= 1 for o in gathered)
        checks["all ranks converged"] = all(o["stats"]["converged"] for o in gathered) and rs.converged
        iters = [o["stats"]["num_iters"] for o in gathered]
        checks["same iteration count on every rank"] = len(set(iters)) == 1
        # every sum that feeds the BB step is a double-double pair rounded once (body sums on the owner, the two dot
        # products as pairs through the all-gather): the partition does not reach the iterates
        checks["iterations equal to single rank within 2 (%d vs %d)" % (iters[0], rs.num_iters)] = \
            abs(iters[0] - rs.num_iters) <= 2
        dilute = len(rp) == 0   # no contact anywhere: every rank solves an empty problem and still joins the collectives
        if checks["pair set == single-rank neighbour list"] and not dilute:
            dg = np.abs(allg[srt] - rg).max()
            checks["gradient vs single rank (max diff %.3g)" % dg] = dg <= 20 * tol
            checks["LCP conditions"] = allx.min() >= 0 and allg.min() >= -10 * tol and \
                np.abs(np.minimum(allx, allg)).max() <= 10 * tol
        vel = np.concatenate([o["vel"] for o in gathered])
        dv = np.abs(vel - rvel).max() / max(1e-30, np.abs(rvel).max())
        checks["owned velocities vs single rank (rel %.3g)" % dv] = dv <= 1e-3
        # duplicated (cross-rank) contacts carry bit-identical (x, g) on both ranks
        n_dup = 0
        if world > 1:
            kk = np.concatenate([key(o["gpairs"]) for o in gathered])
            xx = np.concatenate([o["x"] for o in gathered]).view(np.int64)
            gg = np.concatenate([o["g"] for o in gathered]).view(np.int64)
            o_ = np.argsort(kk, kind="stable")
            kk, xx, gg = kk[o_], xx[o_], gg[o_]
            same_key = kk[1:] == kk[:-1]
            n_dup = int(same_key.sum())
            differ = same_key & ((xx[1:] != xx[:-1]) | (gg[1:] != gg[:-1]))
            if differ.any():
                checks["%d duplicated contacts differ in (x, g)" % int(differ.sum())] = False
        checks["%d duplicated cross-rank contacts found" % n_dup] = (n_dup > 0) or world == 1 or dilute
        if os.environ.get("DIST_EXACT") and checks["pair set == single-rank neighbour list"]:
            # the partitioned solve IS the fused single-rank solve: same iteration count, same multipliers, bit for bit
            checks["iteration count equals the fused solve's (%d vs %d)" % (iters[0], rs.num_iters)] = iters[0] == rs.num_iters
            checks["multipliers bit-identical to the fused solve"] = np.array_equal(allx[srt], ref.lam.cpu().numpy())
            if os.environ.get("DIST_EXPECT_ITERS"):
                checks["iterations == %s" % os.environ["DIST_EXPECT_ITERS"]] = iters[0] == int(os.environ["DIST_EXPECT_ITERS"])
        # (a rank that owns nothing -- fewer bodies than ranks -- holds no ghosts either, but takes part in every collective)
        checks["ghosts exchanged"] = world == 1 or dilute or \
            all(o["stats"]["ghosts"] > 0 for o in gathered if len(o["vel"]) > 0)
        for k, v in checks.items():
            print(("ok   " if v else "FAIL ") + k)
            ok = ok and bool(v)
        print("DIST_RESULT", "PASS" if ok else "FAIL", "mixed" if mixed else "rods", "world", world, "contacts", len(rp), "iters", iters,
              "single", rs.num_iters)
    # a short trajectory: the owned bodies of every rank, advanced by three more full steps (ghost plan, list, solve and
    # Euler update each step), track the single-rank trajectory of the same system
    steps = int(os.environ.get("DIST_STEPS", "0"))
    reuse = os.environ.get("DIST_REUSE", "0") == "1"   # the rebuild rule across ranks instead of a rebuild every step
    migrate = os.environ.get("DIST_MIGRATE", "0") == "1"  # bodies change owner; the curve is re-cut by work
    if steps and not mixed:
        rebuilt, moved_out, imbalance = [], 0, []
        for _ in range(steps):
            stats = st.step(integrate=True, force_rebuild=not reuse, migrate=migrate)
            rebuilt.append(bool(stats["rebuilt"]))
            moved_out += stats.get("migrated_out", 0) if migrate else 0
            imbalance.append(stats["owned_contacts"])
        ent = st.entity_id.cpu().numpy().astype(np.int64)
        mine = dict(c=st.center.cpu().numpy(), q=st.quat.cpu().numpy(), conv=stats["converged"], ent=ent,
                    moved_out=moved_out, owned_contacts=imbalance, n=st.n)
        allc = [None] * world if rank == 0 else None
        dist.gather_object(mine, allc, dst=0)
        if rank == 0:
            ref_rebuilt = []
            for _ in range(steps):
                rs = ref.step(integrate=True, force_rebuild=not reuse)
                ref_rebuilt.append(bool(rs.rebuilt))
            c_ref, q_ref = ref.center.cpu().numpy(), ref.quat.cpu().numpy()
            ent_all = np.concatenate([o["ent"] for o in allc])
            order_e = np.argsort(ent_all)
            good_ids = np.array_equal(ent_all[order_e], np.arange(n_total))      # every body exactly once
            c_all = np.concatenate([o["c"] for o in allc])[order_e]
            q_all = np.concatenate([o["q"] for o in allc])[order_e]
            dc = np.abs(c_all - c_ref).max()
            dq = np.abs(np.abs(np.sum(q_all * q_ref, axis=1)) - 1.0).max()
            moved = np.abs(c_ref - g_center).max()
            # every sum that reaches an iterate is rounded once (double-double), so neither the partition nor a change of
            # owner reaches the trajectory: far below the 1e-4 this test used to allow
            good = all(o["conv"] for o in allc) and rs.converged and good_ids and dc <= 1e-11 and dq <= 1e-12
            if migrate:
                total_moved = sum(o["moved_out"] for o in allc)
                per_rank = np.array([o["owned_contacts"] for o in allc], dtype=np.float64)   # [rank][step]
                imb = per_rank.max(axis=0) * world / np.maximum(1.0, per_rank.sum(axis=0))
                # (a handful of bodies may never leave their cells: DIST_MIGRATE_ANY=1 only runs the machinery)
                owners_changed = total_moved > 0 or os.environ.get("DIST_MIGRATE_ANY", "0") == "1"
                print(("ok   " if owners_changed else "FAIL ") + "%d bodies changed owner over %d steps; owned bodies now %s; "
                      "contact imbalance (max / mean) first step %.3f, after the re-cuts %.3f"
                      % (total_moved, steps, [o["n"] for o in allc], imb[0], imb[-1]))
                good = good and owners_changed and (imb[-1] <= max(1.15, imb[0]) or os.environ.get("DIST_MIGRATE_ANY", "0") == "1")
            print(("ok   " if good else "FAIL ") + "%d-step trajectory vs single rank: max |dc| %.3g (bodies moved up to %.3g), "
                  "quaternion defect %.3g" % (steps, dc, moved, dq))
            if reuse:
                # every rank takes the same decision (it is all-gathered), and it is the single-rank one
                same = rebuilt == ref_rebuilt and (False in rebuilt) and (True in rebuilt)
                print(("ok   " if same else "FAIL ") + "rebuild decisions %s (single rank %s)" % (rebuilt, ref_rebuilt))
                good = good and same
            ok = ok and good
            print("DIST_TRAJECTORY", "PASS" if good else "FAIL")
    # everything closed, the spare set released: the library holds no device or pinned memory of its own (the
    # communicator's destructor; where the inboxes opened, the trial exchange's table too)
    handles = [st.op, st.links, st.comm] + ([ref.op, ref.links] if rank == 0 else [])
    st = ref = None
    for h in handles:
        if h is not None:
            h.close()
    gc.collect()
    capi.check(capi.load().mhip_release_cached_workspaces())
    m = ops.memory_stats()
    left = [None] * world if rank == 0 else None
    dist.gather_object((m["handle_bytes"], m["pinned_bytes"]), left, dst=0)
    if rank == 0:
        checks["handle bytes 0 after close"] = all(v == (0, 0) for v in left)
        print(("ok   " if checks["handle bytes 0 after close"] else "FAIL ") +
              "handle bytes 0 after close: (handle, pinned) per rank %s" % left)
        ok = ok and checks["handle bytes 0 after close"]
    flag = torch.tensor([1 if ok else 0])
    dist.broadcast(flag, src=0)
    dist.destroy_process_group()
    sys.exit(0 if flag.item() else 1)


if __name__ == "__main__":
    main()
