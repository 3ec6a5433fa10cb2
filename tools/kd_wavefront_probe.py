#!/usr/bin/env python3
"""Timing of the kd-tree batch-mode kernel against today's flat launches, forms alternated A B A B in ONE process:
  1. the bench step's four ray sets (nn_bvh_amd/raygen.py) as four nnbvh_kd_intersect_*_device launches against one
     nnbvh_kd_trace_batches_device call, shadow batch first and primary batch first;
  2. the dependent form through the queue calls: closest_and_shadow in one launch against the two calls, and the
     SOA-reading instances against gather + records (scene options "pair_one_launch" / "read_soa" 0);
  3. one batch through the batch-mode instance against the MODE 0 instance on the same rays.
Medians of --runs runs after --warmup warm-ups, min and max beside each.
Usage: timeout -k 10 600 python tools/kd_wavefront_probe.py [--scene crown] [--runs 15] [--warmup 3] [--spp 4]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="crown")
    ap.add_argument("--runs", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--spp", type=int, default=4)
    args = ap.parse_args()
    import torch
    from nn_bvh_amd import make_prims, raygen, scene
    from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    dev = torch.device("cuda", 0)
    verts, tris, source = scene.load_scene(args.scene)
    prims = make_prims(tris)
    kd = build_kd_tree(prims, verts, where="gpu")

    def scene_with(**options):
        a = KdTreeAggregate.from_tree(kd.nodes, kd.prim_indices, prims, verts, kd.bounds)
        for k, v in options.items():
            a.set_option(k, v)
        return a

    agg = scene_with(read_soa=1, pair_one_launch=1)
    agg_two = scene_with(read_soa=1, pair_one_launch=0)     # closest_and_shadow as the two calls
    agg_gather = scene_with(read_soa=0, pair_one_launch=1)  # SOA queues gathered into records
    stream = torch.cuda.current_stream(dev).cuda_stream
    # the bench step's four ray sets
    ds = raygen.DeviceScene(verts, tris, dev)
    _, px, py = scene.camera_rays(args.scene, seed=1, sample=0, return_pixels=True)
    tiles = np.lexsort((px, py, px // 4, py // 4))
    d_px = torch.from_numpy(px[tiles].astype(np.float64)).to(dev)
    d_py = torch.from_numpy(py[tiles].astype(np.float64)).to(dev)
    primary = torch.stack([ds.camera_rays(args.scene, d_px, d_py, seed=1, sample=s) for s in range(args.spp)], 1)
    primary = primary.reshape(-1, 8).contiguous()

    def trace(rays_t):
        out = torch.empty(len(rays_t) * 32, dtype=torch.uint8, device=dev)
        agg.intersect_device(rays_t.data_ptr(), out.data_ptr(), len(rays_t), stream)
        torch.cuda.synchronize()
        return out

    hits = trace(primary)
    bounce, _ = ds.bounce_rays(primary, hits, seed=[2, 0, 0])
    bounce2, _ = ds.bounce_rays(bounce, trace(bounce), seed=[4, 0, 0])
    if args.scene == "crown":
        shadow, _ = ds.shadow_rays(primary, hits, seed=[3, 0, 0], quads=scene.CROWN_LIGHT_QUADS)
    else:
        lo, hi = verts.min(0), verts.max(0)
        shadow, _ = ds.shadow_rays(primary, hits, seed=[3, 0, 0],
                                   box=(lo + (hi - lo) * [0.3, 0.9, 0.3], lo + (hi - lo) * [0.7, 1.0, 0.7]))
    sets = [("closest", primary), ("closest", bounce), ("closest", bounce2), ("any", shadow)]
    outs = [torch.empty(len(t) * (32 if k == "closest" else 1), dtype=torch.uint8, device=dev) for k, t in sets]
    n_step = sum(len(t) for _, t in sets)

    def four_launches():
        for (k, t), o in zip(sets, outs):
            if k == "closest":
                agg.intersect_device(t.data_ptr(), o.data_ptr(), len(t), stream)
            else:
                agg.intersect_p_device(t.data_ptr(), o.data_ptr(), len(t), stream=stream)

    def batches(order):
        tup = [(sets[i][0], sets[i][1].data_ptr(), len(sets[i][1]), outs[i].data_ptr()) for i in order]
        return lambda: agg.trace_batches_device(tup, stream)

    # the dependent form: the shadow queue of one depth and the ray queue of the next
    def queue(t, shadow_q):
        return RayQueue(t[:, 0:3].T.contiguous(), t[:, 4:7].T.contiguous(), tmax=t[:, 3].contiguous() if shadow_q else None)

    rq, sq = queue(bounce, False), queue(shadow, True)
    ns = len(shadow)
    gen = torch.Generator(device=dev).manual_seed(5)
    Ld = torch.rand((ns, 4), generator=gen, device=dev)
    ru, rl = torch.rand((ns, 4), generator=gen, device=dev) + 0.5, torch.rand((ns, 4), generator=gen, device=dev) + 0.5
    pix = torch.arange(ns, dtype=torch.int32, device=dev)
    L = torch.zeros((ns, 4), dtype=torch.float32, device=dev)
    q_hits = torch.empty((len(bounce), 32), dtype=torch.uint8, device=dev)
    q_occ = torch.empty(ns, dtype=torch.uint8, device=dev)

    def pair(a):
        wf = WavefrontAggregate(a)
        return lambda: wf.IntersectClosestAndShadow(len(bounce), rq, ns, sq, Ld, ru, rl, pix, L, hits=q_hits, occluded=q_occ)

    def one_batch():
        agg.trace_batches_device([("closest", bounce.data_ptr(), len(bounce), outs[1].data_ptr())], stream)

    def mode0():
        agg.intersect_device(bounce.data_ptr(), outs[1].data_ptr(), len(bounce), stream)

    n_pair = len(bounce) + ns
    groups = [
        ("1. bench step, %d rays" % n_step, n_step,
         [("four kd_intersect_*_device launches (the parent's path)", four_launches),
          ("one kd_trace_batches_device, primary first", batches([0, 1, 2, 3])),
          ("one kd_trace_batches_device, shadow first", batches([3, 0, 1, 2]))]),
        ("2. queue calls, %d rays (bounce-1 queue + shadow queue)" % n_pair, n_pair,
         [("closest_and_shadow as two calls, SOA read", pair(agg_two)),
          ("closest_and_shadow in one launch, SOA read", pair(agg)),
          ("closest_and_shadow in one launch, gather + records", pair(agg_gather))]),
        ("3. one batch, %d rays (bounce 1)" % len(bounce), len(bounce),
         [("MODE 0 instance (kd_intersect_closest_device)", mode0),
          ("batch-mode instance, one batch", one_batch)]),
    ]
    print(f"# {source}; kd tree built on the device, depth {kd.depth}; medians of {args.runs} runs after {args.warmup} "
          f"warm-ups, forms alternated in one process")
    for title, n, forms in groups:
        times = {name: [] for name, _ in forms}
        for rnd in range(args.warmup + args.runs):
            for name, fn in forms:
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if rnd >= args.warmup:
                    times[name].append(a.elapsed_time(b))
        print(title)
        for name, _ in forms:
            t = np.array(times[name])
            print(f"  {name:58s} median {np.median(t):8.3f} ms  min {t.min():8.3f}  max {t.max():8.3f}  "
                  f"({n / np.median(t) / 1e3:7.1f} Mray/s)", flush=True)
    for a in (agg, agg_two, agg_gather):
        a.close()


if __name__ == "__main__":
    main()
