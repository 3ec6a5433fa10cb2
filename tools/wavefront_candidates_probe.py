#!/usr/bin/env python3
"""One wavefront step (closest-hit queue + shadow queue) with host candidates: the one-launch call
(nnbvh_wavefront_intersect_closest_and_shadow_items_candidates) against the two-launch form (the shadow call, then
the closest call: gather + one candidate launch each, which is also all the single-batch candidate calls allow),
same scene, same device-resident queues, same enqueue / record passes; plus the trace kernels alone on
pre-gathered records (nnbvh_intersect_*_candidates_device twice against nnbvh_trace_batches_candidates_device).
Scene: a triangle soup with every 7th triangle declared host-only by its bounds (tests/test_host_candidates.py
flat_host_scene at scale).  Prints one JSON line; times are medians of --reps runs after 3 warm-up runs, with the
spread (min, max) next to them.
Usage: python tools/wavefront_candidates_probe.py [--tris 1000000] [--rays 4194304] [--reps 15] [--out DIR]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    from nn_bvh_amd import BVHAggregate, build_tree, make_prims, scene
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import HostCandidateArrays, RayQueue, WavefrontAggregate, WorkQueue
    n_tris, n, reps, K = arg("--tris", 1_000_000), arg("--rays", 1 << 22), arg("--reps", 15), 16
    rng = np.random.default_rng(0)
    extent = 10.0 * (n_tris / 1500) ** (1 / 3)  # the density of the test scene
    c = rng.uniform(-extent, extent, size=(n_tris, 1, 3))
    verts = (c + rng.uniform(-0.6, 0.6, size=(n_tris, 3, 3))).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n_tris, dtype=np.int32).reshape(n_tris, 3)
    prims = make_prims(tris)
    prims["kind"][np.arange(n_tris) % 7 == 3] = 3
    tv = verts[tris]
    bounds = np.concatenate([tv.min(1), tv.max(1)], 1).astype(np.float32)
    tree = build_tree(prims, verts, prim_bounds=bounds)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    mesh = ShadingMesh(verts, tris)
    dev = torch.device("cuda", 0)
    lo, hi = verts.min(0), verts.max(0)
    rays = scene.random_rays(n, lo, hi, 3)
    srays = scene.random_rays(n, lo, hi, 4, tmax=np.float32(1 - 1e-4))
    rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(srays, dev, shadow=True)
    wf = WavefrontAggregate(agg)
    queues = {k: WorkQueue(n, dev) for k in ("escaped", "basic_eval_material")}
    nh = WorkQueue(n, dev)
    hits = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    cc, sc = HostCandidateArrays(n, K, dev), HostCandidateArrays(n, K, dev)
    f4 = lambda: torch.rand((n, 4), dtype=torch.float32, device=dev) + 0.1  # noqa: E731
    Ld, r_u, r_l = f4(), f4(), f4()
    px = torch.randperm(n, device=dev).to(torch.int32)
    L = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 32).copy()).to(dev)
    d_srays = torch.from_numpy(srays.view(np.uint8).reshape(n, 32).copy()).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def reset():
        for q in list(queues.values()) + [nh]:
            q.Reset()

    def one_launch():
        wf.IntersectClosestAndShadowItemsWithCandidates(n, rq, mesh, cc, hits, n, sq, Ld, r_u, r_l, px, L, occ, sc,
                                                        needs_host=nh, **queues)

    def two_launches():
        wf.IntersectShadowWithCandidates(n, sq, Ld, r_u, r_l, px, L, occ, sc)
        wf.IntersectClosestItemsWithCandidates(n, rq, mesh, cc, hits, needs_host=nh, **queues)

    def trace_fused():
        agg.trace_batches_candidates_device(
            [("closest", d_rays.data_ptr(), n, hits.data_ptr()), ("any", d_srays.data_ptr(), n, occ.data_ptr())],
            [(K, cc.count.data_ptr(), cc.before.data_ptr(), cc.prim.data_ptr(), cc.instance.data_ptr()),
             (K, sc.count.data_ptr(), None, sc.prim.data_ptr(), sc.instance.data_ptr())], stream)

    def trace_two():
        agg.intersect_p_candidates_device(d_srays.data_ptr(), occ.data_ptr(), n, K, sc.count.data_ptr(),
                                          sc.prim.data_ptr(), sc.instance.data_ptr(), stream)
        agg.intersect_candidates_device(d_rays.data_ptr(), hits.data_ptr(), n, K, cc.count.data_ptr(),
                                        cc.before.data_ptr(), cc.prim.data_ptr(), cc.instance.data_ptr(), stream)

    def timed(fn):
        ms = []
        for i in range(reps + 3):
            reset()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(a.elapsed_time(b))
        return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}

    # interleaved order A B A B so that clock or thermal drift does not favour one form
    res = {"one_launch": timed(one_launch), "two_launches": timed(two_launches),
           "one_launch_again": timed(one_launch), "two_launches_again": timed(two_launches),
           "trace_fused": timed(trace_fused), "trace_two": timed(trace_two)}
    one_launch()
    torch.cuda.synchronize()
    cnt, scnt = cc.count.cpu().numpy(), sc.count.cpu().numpy()
    res.update({"tris": n_tris, "rays_per_queue": n, "capacity": K,
                "closest_share_with_candidates": round(float((cnt != 0).mean()), 4),
                "closest_share_void": round(float((cnt < 0).mean()), 5),
                "shadow_share_for_the_caller": round(float((occ.cpu().numpy() == 2).mean()), 4),
                "shadow_share_void": round(float((scnt < 0).mean()), 5),
                "grid_blocks": agg.info["grid_blocks"]})
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        os.makedirs(arg("--out", ""), exist_ok=True)
        with open(os.path.join(arg("--out", ""), "wavefront_candidates_probe.json"), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
