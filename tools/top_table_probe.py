#!/usr/bin/env python3
"""The lean one-launch kernel's interior record fetches on the bench step (crown, 8 spp, sample set 0 of bench.py):
per ray class alone and for the four-batch step, the launch time with the top table on and off (option "top_table")
and, under a statistics build (NNBVH_LIB=libnnbvh_hip_stats.so, python -c "from nn_bvh_amd import build;
build.build_stats()"), the interior lane-steps per launch and how many of them read their record from the LDS table.
Records per second = interior lane-steps (statistics build) over the launch time (product build): run it once with
each library and put the two beside tools/record_load_probe's figure of the same session.
Then the four-batch step at every top_burst of BURSTS (option "top_burst": the tagged lanes that make a wave take a
table step) and every refill_weight of REFILLS.
Usage: [NNBVH_LIB=...] python tools/top_table_probe.py [reps [BURSTS [REFILLS]]]   (7, 65,48,32,24,16,8,1 and 8)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    bursts = [int(v) for v in (sys.argv[2] if len(sys.argv) > 2 else "65,48,32,24,16,8,1").split(",")]
    refills = [int(v) for v in (sys.argv[3] if len(sys.argv) > 3 else "8").split(",")]
    import torch
    from nn_bvh_amd import BVHAggregate, build_tree, make_prims, raygen, scene
    cdev = torch.device("cuda", 0)
    verts, tris, _ = scene.load_scene("crown")
    tree = build_tree(make_prims(tris), verts)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    stream = torch.cuda.current_stream().cuda_stream
    # sample set 0 of bench.py (one GPU, tile order, 8 samples per pixel)
    xres = scene.CAMERAS["crown"][4]
    _, px, py = scene.camera_rays("crown", seed=1, sample=0, return_pixels=True)
    mine = np.lexsort((px, py, px // 4, py // 4))
    ds = raygen.DeviceScene(verts, tris, cdev)
    d_px, d_py = (torch.from_numpy(a[mine].astype(np.float64)).to(cdev) for a in (px, py))
    primary = torch.stack([ds.camera_rays("crown", d_px, d_py, seed=1, sample=s) for s in range(8)], 1).reshape(-1, 8).contiguous()

    def closest(rays_t):
        out = torch.empty(len(rays_t) * 32, dtype=torch.uint8, device=cdev)
        agg.intersect_device(rays_t.view(torch.uint8).reshape(-1).data_ptr(), out.data_ptr(), len(rays_t), stream)
        torch.cuda.synchronize()
        return out
    hits = closest(primary)
    bounce, _ = ds.bounce_rays(primary, hits, seed=[2, 0, 0])
    bounce2, _ = ds.bounce_rays(bounce, closest(bounce), seed=[4, 0, 0])
    shadow, _ = ds.shadow_rays(primary, hits, seed=[3, 0, 0], quads=scene.CROWN_LIGHT_QUADS)
    classes = {"shadow": ("any", shadow), "bounce2": ("closest", bounce2), "bounce": ("closest", bounce),
               "primary": ("closest", primary)}
    outs = {k: torch.empty(len(r) * 32, dtype=torch.uint8, device=cdev) for k, (_, r) in classes.items()}

    def batch(k):
        kind, r = classes[k]
        return (kind, r.view(torch.uint8).reshape(-1).data_ptr(), len(r), outs[k].data_ptr())
    work = [(k, [batch(k)], len(classes[k][1])) for k in classes]
    work.append(("step", [batch(k) for k in classes], sum(len(r) for _, r in classes.values())))  # bench.py's order
    agg.sched_stats(reset=True)
    try:  # a library from before the table (the parent's, for the comparison) has no such option
        agg.set_option("top_table", 1)
        has_option = True
    except Exception:
        has_option = False
    print(f"interior records {agg.info['interior_records']}, depth {agg.info['depth']}, library "
          f"{os.environ.get('NNBVH_LIB', 'libnnbvh_hip.so')}, {reps} launches each", flush=True)
    for name, batches, n in work:
        line = f"{name:8s} {n / 1e6:6.2f} M rays"
        for table in (1, 0) if has_option else ("-",):
            if has_option:
                agg.set_option("top_table", table)
            agg.trace_batches_device(batches, stream)  # warm-up
            torch.cuda.synchronize()
            agg.sched_stats(reset=True)
            ts = []
            for _ in range(reps):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                agg.trace_batches_device(batches, stream)
                b.record()
                torch.cuda.synchronize()
                ts.append(a.elapsed_time(b))
            st = agg.sched_stats(reset=True)
            ms = float(np.median(ts))
            line += f" | table {table}: {ms:7.3f} ms ({min(ts):.3f} .. {max(ts):.3f})"
            if st["int_step_lanes"]:
                lanes, top = st["int_step_lanes"] / reps, st["int_top_lanes"] / reps
                line += (f", interior lane-steps {lanes / 1e6:8.1f} M = {lanes / n:5.1f} per ray, from LDS {top / 1e6:7.1f} M"
                         f" = {top / max(lanes, 1):.4f}, {lanes / ms / 1e6:6.1f} G records/s at this build's time")
        print(line, flush=True)
    if has_option:
        agg.set_option("top_table", 1)
        sweep(agg, work[-1], stream, reps, bursts, refills)
    agg.close()


def sweep(agg, step, stream, reps, bursts, refills):
    """The four-batch step at every (top_burst, refill_weight) setting: `reps` launches each, the settings interleaved
    (one launch of each per round), median and range; under a statistics build the trips, lanes and shader cycles of the
    table (T), interior (I), primitive (P) and refill (R) trips per launch."""
    import torch
    _, batches, n = step
    try:
        agg.set_option("top_burst", 65)
    except Exception:  # a library from before the table steps
        print("no top_burst option in this library", flush=True)
        return
    settings = [(b, w) for w in refills for b in bursts]
    ts = {s: [] for s in settings}
    stats = {}

    def launch(s, timed):
        agg.set_option("top_burst", s[0])
        agg.set_option("refill_weight", s[1])
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        agg.trace_batches_device(batches, stream)
        b.record()
        torch.cuda.synchronize()
        if timed:
            ts[s].append(a.elapsed_time(b))
    for s in settings:
        launch(s, False)  # warm-up
    for _ in range(reps):
        for s in settings:
            launch(s, True)
    for s in settings:  # one more launch each for the counters
        agg.sched_stats(reset=True)
        launch(s, False)
        stats[s] = agg.sched_stats(reset=True)
    print(f"four-batch step, {reps} launches per setting, interleaved", flush=True)
    for s in settings:
        t, st = ts[s], stats[s]
        line = f"top_burst {s[0]:2d} refill_weight {s[1]:2d}: {float(np.median(t)):7.3f} ms ({min(t):.3f} .. {max(t):.3f})"
        if st["int_step_lanes"]:
            for k, name in (("T", "table"), ("I", "int"), ("P", "prim"), ("R", "refill")):
                trips, lanes, cyc = st[name + "_trips"], st[name + "_lanes"], st[name + "_cycles"]
                line += (f" | {k} {trips / 1e6:6.2f} M trips, {lanes / max(trips, 1):4.1f} lanes, "
                         f"{cyc / max(trips, 1):6.0f} cycles")
            line += (f" | interior lane-steps {(st['int_step_lanes'] + st['table_lanes']) / n:5.1f} per ray, in ordinary "
                     f"steps from LDS {st['int_top_lanes'] / n:5.1f}, in table steps {st['table_lanes'] / n:5.1f}")
        print(line, flush=True)


if __name__ == "__main__":
    main()
