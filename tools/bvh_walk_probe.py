#!/usr/bin/env python3
"""First measurements of the BVH walk calls (nnbvh_wavefront_walk_shadow_tr / _one_random) on the
crown BVH, device-built, with the workload and the tables of tools/kd_walk_probe.py so that the two trees can be read
side by side:
  1. IntersectShadowTr over 2^20 bounce shadow rays (the bench step's shadow set), with 0 %, 10 % and 50 % of the
     primitives marked interface (seeded);
  2. IntersectOneRandom over 2^20 segments between seeded points inside the scene bounds.
Forms per workload, as tools/wavefront_bounded_probe.py has them: the floor (one nnbvh_wavefront_intersect_closest on
the same first-segment rays), the unbounded call, the bounded call at the passes the batch needs and at 8, and the walk
call at --cap.  Per form: the median of --runs timed calls after --warmup warm-ups (device events, forms alternated in
one process), min and max; per workload the items left unfinished at --cap and the histogram of Intersect calls per
item.  The histogram comes from the calls themselves: a run with max_surfaces = c counts the items that need more than
c calls.
Usage: timeout -k 10 900 python tools/bvh_walk_probe.py [--runs 20] [--warmup 3] [--cap 64] > profiles/bvh_walk.txt"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="crown")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=64)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--label", default="an unversioned tree", help="the revision measured, for the header line")
    args = ap.parse_args()
    import torch
    from nn_bvh_amd import BVHAggregate, make_prims, raygen, scene
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    if not torch.cuda.is_available():
        raise SystemExit("bvh_walk_probe: no GPU (this probe measures; it has no CPU form)")
    dev = torch.device("cuda", 0)
    verts, tris, source = scene.load_scene(args.scene)
    prims = make_prims(tris)
    agg = BVHAggregate.build_on_device(prims, verts)
    mesh = ShadingMesh(verts, tris)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = args.n

    # ---- the shadow set of the bench step: shadow rays of the primary hits towards the light quads
    ds = raygen.DeviceScene(verts, tris, dev)
    _, px, py = scene.camera_rays(args.scene, seed=1, sample=0, return_pixels=True)
    spp = -(-5 * n // (2 * len(px)))  # (not every primary ray hits, and not every hit sends a shadow ray)
    d_px = torch.from_numpy(px.astype(np.float64)).to(dev)
    d_py = torch.from_numpy(py.astype(np.float64)).to(dev)
    primary = torch.stack([ds.camera_rays(args.scene, d_px, d_py, seed=1, sample=s) for s in range(spp)], 1)
    primary = primary.reshape(-1, 8).contiguous()
    hits = torch.empty(len(primary) * 32, dtype=torch.uint8, device=dev)
    agg.intersect_device(primary.data_ptr(), hits.data_ptr(), len(primary), stream)
    torch.cuda.synchronize()
    if args.scene == "crown":
        shadow, _ = ds.shadow_rays(primary, hits, seed=[3, 0, 0], quads=scene.CROWN_LIGHT_QUADS)
    else:
        lo, hi = verts.min(0), verts.max(0)
        shadow, _ = ds.shadow_rays(primary, hits, seed=[3, 0, 0],
                                   box=(lo + (hi - lo) * [0.3, 0.9, 0.3], lo + (hi - lo) * [0.7, 1.0, 0.7]))
    if len(shadow) < n:
        raise SystemExit(f"bvh_walk_probe: only {len(shadow)} shadow rays")
    shadow = shadow[:n].contiguous()
    sq = RayQueue(shadow[:, 0:3].T.contiguous(), shadow[:, 4:7].T.contiguous(), tmax=shadow[:, 3].contiguous())
    sq.time = shadow[:, 7].contiguous()
    zero_dir = int((shadow[:, 4:7] == 0).all(1).sum().item())
    gen = torch.Generator(device=dev).manual_seed(5)
    Ld = torch.rand((n, 4), generator=gen, device=dev)
    ru, rl = torch.rand((n, 4), generator=gen, device=dev) + 0.5, torch.rand((n, 4), generator=gen, device=dev) + 0.5
    pix = torch.arange(n, dtype=torch.int32, device=dev)
    L = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    state = torch.empty(n, dtype=torch.uint8, device=dev)
    unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
    floor_hits = torch.empty((n, 32), dtype=torch.uint8, device=dev)

    # ---- one-random segments between seeded points inside the bounds
    rng = np.random.default_rng(11)
    lo, hi = verts.min(0), verts.max(0)
    p0 = torch.from_numpy(rng.uniform(lo, hi, (n, 3)).astype(np.float32)).to(dev)
    p1 = torch.from_numpy(rng.uniform(lo, hi, (n, 3)).astype(np.float32)).to(dev)
    material = torch.zeros(n, dtype=torch.int32, device=dev)
    seg = torch.cat([p0, torch.ones((n, 1), device=dev), p1 - p0, torch.zeros((n, 1), device=dev)], 1)
    oq = RayQueue(seg[:, 0:3].T.contiguous(), seg[:, 4:7].T.contiguous(), tmax=seg[:, 3].contiguous())

    wf0 = WavefrontAggregate(agg)

    def floor(q):
        return lambda: wf0.IntersectClosest(n, q, hits=floor_hits)

    def shadow_call(wf):
        def call(cap=None, passes=None):
            wf.IntersectShadowTr(n, sq, mesh, Ld, ru, rl, pix, L, state, max_surfaces=cap, max_passes=passes,
                                 unfinished=None if cap is None and passes is None else unfinished)
        return call

    def one_random(cap=None, passes=None):
        wf0.IntersectOneRandom(n, p0, p1, material, mesh, None, max_surfaces=cap, max_passes=passes,
                               unfinished=None if cap is None and passes is None else unfinished)

    def left(call, cap):
        call(cap=cap)
        torch.cuda.synchronize()
        return int(unfinished.item())

    def histogram(call, started):
        """Intersect calls per item, from the unfinished counts at max_surfaces = 1, 2, ...: more[c] items need more
        than c calls (more[0] = the items that make a call at all)."""
        more = [started]
        while more[-1] > 0 and len(more) <= 4096:
            more.append(left(call, len(more)))
        return [n - more[0]] + [more[c - 1] - more[c] for c in range(1, len(more))]

    workloads = []  # (title, floor queue, call, items that start a walk)
    for share in (0.0, 0.1, 0.5):
        cls = (np.random.default_rng(7).random(len(prims)) < share).astype(np.uint8) * 2
        workloads.append((f"IntersectShadowTr, {share:4.0%} interface", sq, shadow_call(WavefrontAggregate(agg, cls)),
                          n - zero_dir))
    workloads.append(("IntersectOneRandom", oq, one_random, n))

    print(f"# bvh walk probe at {args.label}: {source}; BVH built on the device; {n} items per call, max_surfaces "
          f"{args.cap}; medians of {args.runs} calls after {args.warmup} warm-ups, forms alternated in one process")
    for title, q, call, started in workloads:
        hist = histogram(call, started)
        need = len(hist) - 1  # the longest walk's Intersect calls = the passes the batch needs
        forms = [("floor: one intersect_closest", floor(q)), ("unbounded", lambda call=call: call())]
        if 1 <= need <= 64:
            forms.append((f"bounded at {need} (needed)", lambda call=call, need=need: call(passes=need)))
        if need <= 8:
            forms.append(("bounded at 8", lambda call=call: call(passes=8)))
        forms.append((f"walk, max_surfaces {args.cap}", lambda call=call: call(cap=args.cap)))
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
        print(f"{title}: unfinished at {args.cap}: {left(call, args.cap)} of {n}; calls per item 0, 1, 2, ...: {hist}")
        for name, _ in forms:
            t = np.array(times[name])
            print(f"    {name:32s} median {np.median(t):8.3f} ms  min {t.min():8.3f}  max {t.max():8.3f}  "
                  f"({n / np.median(t) / 1e3:7.1f} Mitem/s)", flush=True)
    agg.close()
    mesh.close()


if __name__ == "__main__":
    main()
