#!/usr/bin/env python3
"""FIRST FIGURES, gating nothing: the fork's SAH and EPO scores (nn_bvh_amd.tree_quality) of the trees
of the five builders (sah, hlbvh, middle, equal: build_tree; nn: nn_tree.greedy_sah_tree, 4 levels) over a scene, the
phase times of the scoring call, and beside them the mean nodes_visited per ray of one seeded batch of incoherent
closest-hit rays (scene.random_rays between points of the scene's bounds) through BVHAggregate.Intersect on the same
tree.  No correlation between the scores and the visits is claimed or tested.
Scenes: those of --scenes whose blob exists under data/ (crown, bathroom, ... where the build made them), and killeroos
from the copy kept under tests/golden/.
Usage: timeout -k 10 600 python tools/tree_quality.py [--scenes killeroos,bathroom,crown] [--rays 262144] \\
           > profiles/tree_quality.txt"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BUILDERS = ("sah", "hlbvh", "middle", "equal", "nn")


def load(name):
    from nn_bvh_amd import scene
    if os.path.exists(scene.blob_path(name)):
        return scene.load_blob(name)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    if os.path.exists(path):
        with np.load(path) as z:
            return z["verts"], z["tris"]
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="killeroos,bathroom,crown")
    ap.add_argument("--rays", type=int, default=1 << 18)
    ap.add_argument("--leaf", type=int, default=4)
    ap.add_argument("--label", default="an unversioned tree", help="the revision measured, for the header line")
    args = ap.parse_args()
    from nn_bvh_amd import BVHAggregate, build_tree, lib, make_prims, nn_tree, scene, tree_quality
    if lib().nnbvh_device_count() < 1:
        raise SystemExit("tree_quality: no GPU (the scores are computed on the device; there is no CPU form)")
    print(f"# tree quality, first figures ({args.label}): they gate nothing and promise no correlation")
    print(f"# leaf size {args.leaf}; {args.rays} incoherent closest-hit rays (scene.random_rays, seed 5); "
          "times in ms, one call each, not a benchmark")
    for name in args.scenes.split(","):
        blob = load(name)
        if blob is None:
            print(f"# {name}: no blob, left out")
            continue
        verts, tris = blob
        prims = make_prims(tris)
        rays = scene.random_rays(args.rays, verts.min(0), verts.max(0), seed=5)
        print(f"\n{name}: {len(tris)} triangles")
        print(f"{'builder':8s} {'nodes':>8s} {'depth':>5s} {'sah':>10s} {'epo':>10s} {'ext pairs':>11s} "
              f"{'prepare':>8s} {'walk':>8s} {'reduce':>8s} {'total':>8s} {'visits/ray':>10s} {'build s':>8s}")
        for b in BUILDERS:
            t0 = time.time()
            if b == "nn":
                nodes, ordered = nn_tree.greedy_sah_tree(verts, tris, levels=4, max_prims_in_node=args.leaf)[0]
            else:
                t = build_tree(prims, verts, args.leaf, b)
                nodes, ordered = t.nodes, t.ordered_prims
            build_s = time.time() - t0
            tree_quality(nodes, ordered, verts)  # warm-up: the first call loads the code object
            q = tree_quality(nodes, ordered, verts)
            agg = BVHAggregate.from_tree(nodes, ordered, verts, device=0)
            visits = float(agg.Intersect(rays)["nodes_visited"].mean())
            agg.close()
            ms = q.gpu_ms
            print(f"{b:8s} {len(nodes):8d} {q.depth:5d} {q.sah:10.4f} {q.epo:10.4f} "
                  f"{q.ext_pairs_inner + q.ext_pairs_leaf:11d} {ms['prepare']:8.3f} {ms['walk']:8.3f} "
                  f"{ms['reduce']:8.3f} {ms['total']:8.3f} {visits:10.2f} {build_s:8.2f}")


if __name__ == "__main__":
    main()
