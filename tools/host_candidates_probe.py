#!/usr/bin/env python3
"""Cost of listing host-only primitives as candidates (nnbvh_intersect_*_candidates_device) against the plain
calls that void such rays, on one scene with host-only primitives and the same device-resident rays: kernel
time of closest hit and occlusion-only any hit, with and without candidates (K = 8), and how many rays are void
today (instance -1 / occluded 2) against still void with candidates (count < 0) at K = 4, 8, 16.
Scene: the procedural triangle soup with every 31st triangle declared host-only (a textured-alpha stand-in, its
triangle's bounds) plus 32 large host-only boxes (light spheres).
Usage: python tools/host_candidates_probe.py [--tris 1000000] [--rays 2000000] [--reps 20] [--out DIR]"""
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
    n_tris, n_rays, reps = arg("--tris", 1_000_000), arg("--rays", 2_000_000), arg("--reps", 20)
    verts, tris = scene.procedural_scene(n_tris)
    prims = make_prims(tris)
    host = np.arange(len(prims)) % 31 == 5
    prims["kind"][host] = 3
    tv = verts[tris]
    bounds = np.concatenate([tv.min(1), tv.max(1)], 1).astype(np.float32)
    lo, hi = verts.min(0), verts.max(0)
    rng = np.random.default_rng(1)
    n_sph = 32
    c = lo + rng.random((n_sph, 3)) * (hi - lo)
    r = (0.02 * (hi - lo).max() * rng.uniform(0.5, 1.5, n_sph))[:, None]
    sph = np.zeros(n_sph, prims.dtype)
    sph["kind"], sph["id"] = 3, len(prims) + np.arange(n_sph)
    prims = np.concatenate([prims, sph])
    bounds = np.concatenate([bounds, np.concatenate([c - r, c + r], 1).astype(np.float32)])
    tree = build_tree(prims, verts, prim_bounds=bounds)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    rays = scene.random_rays(n_rays, lo, hi, 2)
    n = len(rays)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    d_hits = torch.empty(n * 32, dtype=torch.uint8, device=dev)
    d_occ = torch.empty(n, dtype=torch.uint8, device=dev)
    d_cnt = torch.empty(n, dtype=torch.int32, device=dev)
    d_bef = torch.empty(n, dtype=torch.int32, device=dev)
    d_prim = torch.empty(n * 16, dtype=torch.int32, device=dev)
    d_inst = torch.empty(n * 16, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    p = lambda t: t.data_ptr()  # noqa: E731
    calls = {
        "closest": lambda: agg.intersect_device(p(d_rays), p(d_hits), n, stream),
        "closest+candidates": lambda: agg.intersect_candidates_device(p(d_rays), p(d_hits), n, 8, p(d_cnt), p(d_bef),
                                                                      p(d_prim), p(d_inst), stream),
        "any": lambda: agg.intersect_p_device(p(d_rays), p(d_occ), n, stream=stream),
        "any+candidates": lambda: agg.intersect_p_candidates_device(p(d_rays), p(d_occ), n, 8, p(d_cnt), p(d_prim),
                                                                    p(d_inst), stream),
    }
    res = {"scene": {"triangles": int(n_tris), "host_triangles": int(host.sum()), "host_boxes": n_sph,
                     "rays": int(n)}, "ms": {}, "void": {}}
    for name, f in calls.items():
        for _ in range(3):
            f()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(reps):  # interleaving would mix the kinds' caches; each is timed on its own, warm
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ts.append(a.elapsed_time(b))
        ts = np.array(ts)
        res["ms"][name] = {"median": float(np.median(ts)), "min": float(ts.min()), "max": float(ts.max())}
        print(f"{name:20s} median {np.median(ts):8.3f} ms  min {ts.min():8.3f}  max {ts.max():8.3f}  ({reps} reps)")
    plain = agg.Intersect(rays)
    occ = agg.IntersectP(rays)
    res["void"]["closest_today"] = int((plain["instance"] == -1).sum())
    res["void"]["any_today"] = int((occ == 2).sum())
    print(f"void today: closest {res['void']['closest_today']} of {n}, any hit {res['void']['any_today']}")
    for k in (4, 8, 16):
        h, cands = agg.intersect_with_host_candidates(rays, capacity=k)
        o, acands = agg.intersect_p_with_host_candidates(rays, capacity=k)
        assert np.array_equal(o, occ)
        res["void"][f"closest_K{k}"] = int((cands["count"] < 0).sum())
        res["void"][f"any_K{k}"] = int(((o == 2) & (acands["count"] < 0)).sum())
        print(f"K = {k:2d}: still void: closest {res['void'][f'closest_K{k}']}, any hit {res['void'][f'any_K{k}']}; "
              f"rays with candidates {int((cands['count'] > 0).sum())}, mean count there "
              f"{cands['count'][cands['count'] > 0].mean():.2f}")
    agg.close()
    out = arg("--out", "")
    if out:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "probe.json"), "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
