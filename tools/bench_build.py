#!/usr/bin/env python3
"""Build-time comparison on the GPU box: host SAH (threaded), host HLBVH and GPU HLBVH
(nnbvh_build_create_gpu) per scene blob; the GPU tree is checked byte-for-byte against the host
HLBVH.  Prints one JSON object.  usage: tools/bench_build.py [scene ...]

kd section (--kd: both sections, --kd-only: this one alone; scenes default to bathroom and crown; --kd-out=PATH
writes the table, default profiles/kd_device_scene.txt): creating a kd-tree scene, in one process alternated
A B A B ..., medians with min..max:
  A  build_kd_tree(where="gpu") + KdTreeAggregate.from_tree   the tree downloaded, validated, uploaded again and baked
  B  KdTreeAggregate.build_on_device                          bounds, tree and records made and kept on the device
  C  build_kd_tree(where="host") + from_tree, once, for the record
and the peak of the device memory in use during one B (sampled from a second thread) beside what the scene keeps.

two-level section (--two-level: with the other sections, --two-level-only: alone; --two-level-out=PATH, default
profiles/two_level_device_scene.txt): creating a two-level (instanced) scene, the same way:
  A0 instancing.assemble_two_level + BVHAggregate.from_tree   every tree from the host builder, uploaded and baked
  A  the same with the child and top trees from build_tree_gpu (built on the device, downloaded, uploaded and baked)
  B  BVHAggregate.build_two_level_on_device                    every tree built, numbered and baked on the device, the
                                                               object trees in ONE forest pass
  L  the same with NNBVH_TWO_LEVEL_LOOP=1                      ... the object trees one after another (B before the
                                                               forest build existed)
on (i) the 400 placements of the 33 K-triangle killeroo of tools/bench_instances.py and (ii) 2 000 objects of 64
triangles with 20 000 placements, where the per-object cost of building one tree after another shows; with the
phases of one forest build of the objects alone (build_forest_gpu) and B's peak device memory.
--split=hlbvh runs the four routes with HLBVH trees (phases of one build_hlbvh_forest_gpu; default output
profiles/two_level_device_scene_hlbvh.txt); --split=sah is the default.  With single-tree scenes named as well, their
JSON lines follow as usual (gpu_hlbvh_ms_end_to_end is the single HLBVH build's figure).

Scenes come from scene.load_scene: the blob data/<name>.npz, or the procedural stand-in of its size where it is absent.

--hlbvh-only: of the single-tree section only build_tree_gpu(prims, verts, 4) (HLBVH), end to end and by phase, 5 rounds
after a warm-up as median (min .. max); scenes default to killeroos and crown; --hlbvh-out=PATH also writes the table
(how profiles/hlbvh_one_pipeline.txt was measured, one process per commit)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from nn_bvh_amd import (BVHAggregate, build_forest_gpu, build_hlbvh_forest_gpu, build_tree, build_tree_gpu, make_prims,  # noqa: E402
                        scene)


def kd_section(names, out_path, rounds=5):
    import threading

    import torch

    from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree
    lines, result = [], {}

    def stats(ms):
        return f"{np.median(ms):9.1f} ms  ({min(ms):.1f} .. {max(ms):.1f})"

    for name in names:
        verts, tris, source = scene.load_scene(name)
        prims = make_prims(tris)

        def route_a():
            t = build_kd_tree(prims, verts, where="gpu")
            return KdTreeAggregate.from_tree(t.nodes, t.prim_indices, prims, verts, t.bounds), t.build_ms

        def route_b():
            return KdTreeAggregate.build_on_device(prims, verts), None

        for fn in (route_a, route_b):  # first-call costs (module load, allocator) outside the timing
            fn()[0].close()
        a_ms, b_ms, a_dev = [], [], []
        for _ in range(rounds):
            for fn, ms in ((route_a, a_ms), (route_b, b_ms)):
                t0 = time.perf_counter()
                agg, build_ms = fn()
                ms.append((time.perf_counter() - t0) * 1e3)
                if build_ms:
                    a_dev.append(build_ms)
                info = agg.info()
                agg.close()
        # peak device memory of one B: bytes in use on the device, sampled while the call runs
        torch.cuda.synchronize()
        base = torch.cuda.mem_get_info()[0]
        low, stop = [base], threading.Event()

        def sample():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                time.sleep(0.0005)

        th = threading.Thread(target=sample)
        th.start()
        agg, _ = route_b()
        stop.set()
        th.join()
        kept = base - torch.cuda.mem_get_info()[0]
        agg.close()
        t0 = time.perf_counter()
        t = build_kd_tree(prims, verts, where="host")
        c_build = (time.perf_counter() - t0) * 1e3
        KdTreeAggregate.from_tree(t.nodes, t.prim_indices, prims, verts, t.bounds).close()
        c_ms = (time.perf_counter() - t0) * 1e3
        gain = np.median(a_ms) - np.median(b_ms)
        spread = max(max(a_ms) - min(a_ms), max(b_ms) - min(b_ms))
        verdict = ("B ahead of A by more than either spread" if gain > spread else
                   "B behind A by more than either spread" if -gain > spread else "B and A within the spread")
        lines += [f"{name}: {source}",
                  f"  {len(tris)} triangles, {info['n_nodes']} nodes, {info['n_indices']} indices, depth {info['depth']}",
                  f"  A  device build, down, up again + bake   {stats(a_ms)}",
                  f"     of which the builder itself           {stats([m[0] for m in a_dev])} on the device, "
                  f"{np.median([m[1] for m in a_dev]):.1f} ms with the download",
                  f"  B  build_on_device                       {stats(b_ms)}",
                  f"  C  host build + upload + bake (once)     {c_ms:9.1f} ms  (build {c_build:.1f})",
                  f"  median A - median B = {gain:.1f} ms, larger spread {spread:.1f} ms: {verdict}",
                  f"  B device memory: peak {(base - low[0]) / 2**20:.0f} MiB in use during the call (sampled), "
                  f"{kept / 2**20:.0f} MiB kept (scene arrays {info['device_bytes'] / 2**20:.0f} MiB)", ""]
        result[name] = {"a_ms": a_ms, "b_ms": b_ms, "c_ms": c_ms, "peak_bytes": int(base - low[0]),
                        "scene_bytes": info["device_bytes"], "verdict": verdict}
    text = "\n".join([f"kd scene creation, {rounds} alternated rounds per scene, one process; {torch.cuda.get_device_name(0)}",
                      ""] + lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return result


def two_level_scenes():
    """name -> (top_prims, verts, objects, placements)"""
    out = {}
    rng = np.random.default_rng(1)

    def place(k, M):
        return (k, M[:3].astype(np.float32).reshape(12), np.linalg.inv(M)[:3].astype(np.float32).reshape(12))

    if os.path.exists(os.path.join(ROOT, "data", "killeroos.npz")):  # tools/bench_instances.py's scene
        side = 20
        verts, tris = scene.load_blob("killeroos")
        used, inv = np.unique(tris[4:4 + 33264], return_inverse=True)
        kv = verts[used]
        ext = kv.max(0) - kv.min(0)
        ground = (np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], np.float32) * side * ext.max()
                  + [0, 0, kv[:, 2].min()])
        top = make_prims(np.array([[0, 1, 2], [2, 3, 0]], np.int32) + len(kv))
        top["id"] += 10_000_000
        placements = []
        for i in range(side):
            for j in range(side):
                a, s = rng.uniform(0, 2 * np.pi), rng.uniform(0.6, 1.2)
                M = np.eye(4)
                M[:3, :3] = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]]) * s
                M[:3, 3] = [(i - side / 2) * ext[0] * 1.3, (j - side / 2) * ext[1] * 1.3, 0]
                placements.append(place(0, M))
        out["400 placements of one 33 264-triangle killeroo + a ground quad"] = (
            top, np.concatenate([kv, ground]).astype(np.float32), [make_prims(inv.reshape(-1, 3).astype(np.int32))],
            placements)
    n_obj, n_tri, n_place = 2000, 64, 20000
    c = rng.uniform(-1, 1, (n_obj * n_tri, 1, 3))
    verts = (c + rng.uniform(-0.2, 0.2, (n_obj * n_tri, 3, 3))).reshape(-1, 3).astype(np.float32)
    prims = make_prims(np.arange(3 * n_obj * n_tri, dtype=np.int32).reshape(-1, 3))
    placements = []
    for j in range(n_place):
        M = np.eye(4)
        M[:3, :3] *= rng.uniform(0.5, 2.0)
        M[:3, 3] = rng.uniform(-200, 200, 3)
        placements.append(place(j % n_obj, M))
    out[f"{n_obj} objects of {n_tri} triangles, {n_place} placements"] = (
        prims[:0], verts, [prims[k * n_tri:(k + 1) * n_tri] for k in range(n_obj)], placements)
    return out


def assemble_with(builder, top_prims, verts, objects, placements):
    """instancing.assemble_two_level with the trees from `builder`"""
    from nn_bvh_amd import instancing
    from nn_bvh_amd._lib import INSTANCE_DTYPE, PRIM_DTYPE
    children = [builder(o, verts) for o in objects]
    entries, n_top, _ = BVHAggregate.two_level_entries(top_prims, objects, placements)
    bounds = np.zeros((n_top, 6), np.float32)
    for j, (k, m, _) in enumerate(placements):
        root = children[k].nodes[0]
        bounds[len(top_prims) + j] = instancing.transform_bounds(m, np.concatenate([root["pmin"], root["pmax"]]))
    top = builder(entries[:n_top], verts, prim_bounds=bounds)
    nodes, prims, node_base = [top.nodes], [top.ordered_prims], []
    nb, pb = len(top.nodes), len(top.ordered_prims)
    for c in children:
        node_base.append(nb)
        cn = c.nodes.copy()
        interior = cn["nprims"] == 0
        cn["offset"][interior] += nb
        cn["offset"][~interior] += pb
        nodes.append(cn)
        prims.append(c.ordered_prims)
        nb += len(cn)
        pb += len(c.ordered_prims)
    instances = np.zeros(len(placements), INSTANCE_DTYPE)
    instances["render_from_prim"] = [p[1] for p in placements]
    instances["prim_from_render"] = [p[2] for p in placements]
    instances["root"] = [node_base[p[0]] for p in placements]
    instances["n_nodes"] = [len(children[p[0]].nodes) for p in placements]
    return np.concatenate(nodes), np.concatenate(prims).astype(PRIM_DTYPE), instances, len(top.nodes)


def two_level_section(out_path, rounds=5, split="sah"):
    import threading

    import torch

    from nn_bvh_amd import instancing
    lines, result = [], {}

    def stats(ms):
        return f"{np.median(ms):9.1f} ms  ({min(ms):.1f} .. {max(ms):.1f})"

    def phases(forest):
        m = forest.gpu_ms
        if split == "sah":
            return (f"  one forest build of the objects alone: upload {m[0]:.2f}, big nodes {m[1]:.2f}, subtrees {m[2]:.2f}, "
                    f"layout + bounds {m[3]:.2f}, download {m[4]:.2f} ms; {forest.n_levels} breadth-first passes, "
                    f"{forest.n_subtrees} subtrees")
        return (f"  one forest build of the objects alone: upload {m[0]:.2f}, sort + treelets {m[1]:.2f}, upper SAH "
                f"{m[2]:.2f}, emit {m[3]:.2f}, download {m[4]:.2f} ms; {forest.n_subtrees} treelets")

    for name, (top, verts, objects, placements) in two_level_scenes().items():
        def from_arrays(nodes, prims, instances, n_top):
            return BVHAggregate.from_tree(nodes, prims, verts, instances=instances, n_top_nodes=n_top)

        def route_a0():
            return from_arrays(*instancing.assemble_two_level(top, verts, objects, placements, 4, split))

        def route_a():
            gpu = lambda p, v, prim_bounds=None: build_tree_gpu(p, v, 4, prim_bounds, split_method=split)  # noqa: E731
            return from_arrays(*assemble_with(gpu, top, verts, objects, placements))

        def route_b():
            return BVHAggregate.build_two_level_on_device(top, verts, objects, placements, 4, split)

        def route_loop():
            os.environ["NNBVH_TWO_LEVEL_LOOP"] = "1"  # read once per call
            try:
                return route_b()
            finally:
                del os.environ["NNBVH_TWO_LEVEL_LOOP"]

        routes = (route_a0, route_a, route_loop, route_b)
        ref = None
        for fn in routes:  # first-call costs outside the timing; and the four scenes are one scene
            agg = fn()
            arrays = (agg.read(0).tobytes(), agg.read(1).tobytes(), agg.info)
            assert ref is None or arrays == ref, f"{fn.__name__} bakes other arrays"
            ref = arrays
            info = agg.info
            agg.close()
        ms = {fn.__name__: [] for fn in routes}
        for _ in range(rounds):
            for fn in routes:
                t0 = time.perf_counter()
                agg = fn()
                ms[fn.__name__].append((time.perf_counter() - t0) * 1e3)
                agg.close()
        torch.cuda.synchronize()
        base = torch.cuda.mem_get_info()[0]
        low, stop = [base], threading.Event()

        def sample():
            while not stop.is_set():
                low[0] = min(low[0], torch.cuda.mem_get_info()[0])
                time.sleep(0.0005)

        th = threading.Thread(target=sample)
        th.start()
        agg = route_b()
        stop.set()
        th.join()
        kept = base - torch.cuda.mem_get_info()[0]
        agg.close()
        forest = (build_forest_gpu if split == "sah" else build_hlbvh_forest_gpu)(objects, verts)
        a_ms, b_ms, l_ms, a0_ms = ms["route_a"], ms["route_b"], ms["route_loop"], ms["route_a0"]
        gain_l = np.median(l_ms) - np.median(b_ms)
        spread_l = max(max(l_ms) - min(l_ms), max(b_ms) - min(b_ms))
        verdict_l = ("B ahead of L by more than either spread" if gain_l > spread_l else
                     "B behind L by more than either spread" if -gain_l > spread_l else "B and L within the spread")
        gain = np.median(a_ms) - np.median(b_ms)
        spread = max(max(a_ms) - min(a_ms), max(b_ms) - min(b_ms))
        verdict = ("B ahead of A by more than either spread" if gain > spread else
                   "B behind A by more than either spread" if -gain > spread else "B and A within the spread")
        lines += [f"{name}",
                  f"  {sum(len(o) for o in objects)} object + {len(top)} top-level primitives, {len(objects)} objects, "
                  f"{len(placements)} placements; {info['interior_records']} interior records, "
                  f"{info['prim_slots']} slots, depth {info['depth']}",
                  f"  A0 host trees, uploaded + baked           {stats(ms['route_a0'])}",
                  f"  A  device trees, down, up again + baked   {stats(a_ms)}",
                  f"  L  build_two_level_on_device, object loop {stats(l_ms)}",
                  f"  B  build_two_level_on_device, forest      {stats(b_ms)}",
                  f"  median A - median B = {gain:.1f} ms, larger spread {spread:.1f} ms: {verdict}",
                  f"  median L - median B = {gain_l:.1f} ms, larger spread {spread_l:.1f} ms: {verdict_l}",
                  f"  median B - median A0 = {np.median(b_ms) - np.median(a0_ms):.1f} ms",
                  phases(forest),
                  f"  B device memory: peak {(base - low[0]) / 2**20:.0f} MiB in use during the call (sampled), "
                  f"{kept / 2**20:.0f} MiB kept (scene arrays {info['device_bytes'] / 2**20:.0f} MiB)", ""]
        result[name] = {"a0_ms": a0_ms, "a_ms": a_ms, "loop_ms": l_ms, "b_ms": b_ms, "peak_bytes": int(base - low[0]),
                        "scene_bytes": info["device_bytes"], "verdict": verdict, "verdict_loop": verdict_l,
                        "forest_phases_ms": forest.gpu_ms}
    text = "\n".join([f"two-level scene creation, {split} trees, {rounds} alternated rounds per scene, one process; "
                      f"{torch.cuda.get_device_name(0)}", ""] + lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)
    return result


def hlbvh_section(names, out_path, rounds=5):
    lines, result = [], {}

    def stats(ms):
        return f"{np.median(ms):9.2f} ms  ({min(ms):.2f} .. {max(ms):.2f})"

    for name in names:
        verts, tris, source = scene.load_scene(name)
        prims = make_prims(tris)
        build_tree_gpu(prims, verts, 4)  # warm-up: module load, allocator
        total, phases = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            tree = build_tree_gpu(prims, verts, 4)
            total.append((time.perf_counter() - t0) * 1e3)
            phases.append(tree.gpu_ms)
        lines += [f"{source}: {len(tris)} triangles, {len(tree.nodes)} nodes",
                  f"  build_tree_gpu, end to end   {stats(total)}"]
        lines += [f"    {what:26s} {stats([p[k] for p in phases])}"
                  for k, what in enumerate(("upload", "device sort + tree", "upper SAH", "emit", "download"))]
        lines.append("")
        result[name] = {"end_to_end_ms": total, "phases_ms": phases}
    text = "\n".join([f"single HLBVH build on the device, {rounds} rounds after a warm-up, median (min .. max)", ""] + lines)
    print(text)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write(text)
    return result


flags = [a for a in sys.argv[1:] if a.startswith("--")]
args = [a for a in sys.argv[1:] if not a.startswith("--")]
kd_out = os.path.join(ROOT, "profiles", "kd_device_scene.txt")
for f in flags:
    if f.startswith("--kd-out="):
        kd_out = f.split("=", 1)[1]
split = "sah"
for f in flags:
    if f.startswith("--split="):
        split = f.split("=", 1)[1]
if split not in ("sah", "hlbvh"):
    sys.exit("--split=sah or --split=hlbvh")
two_level_out = os.path.join(ROOT, "profiles", "two_level_device_scene" + ("" if split == "sah" else "_hlbvh") + ".txt")
for f in flags:
    if f.startswith("--two-level-out="):
        two_level_out = f.split("=", 1)[1]
names = args or ["killeroos", "coffee_maker", "bathroom", "crown"]
out = {}
if "--two-level" in flags or "--two-level-only" in flags:
    out["two_level_scene_create"] = two_level_section(two_level_out, split=split)
if "--kd" in flags or "--kd-only" in flags:
    out["kd_scene_create"] = kd_section(args or ["bathroom", "crown"], kd_out)
if "--hlbvh-only" in flags:
    hlbvh_out = [f.split("=", 1)[1] for f in flags if f.startswith("--hlbvh-out=")]
    out["single_hlbvh_build"] = hlbvh_section(args or ["killeroos", "crown"], hlbvh_out[0] if hlbvh_out else None)
for name in ([] if "--kd-only" in flags or "--two-level-only" in flags or "--hlbvh-only" in flags else names):
    verts, tris, _ = scene.load_scene(name)
    prims = make_prims(tris)

    def timed(fn, reps):
        best, res = 1e30, None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = fn()
            best = min(best, time.perf_counter() - t0)
        return best * 1e3, res

    ms_hl, host = timed(lambda: build_tree(prims, verts, 4, "hlbvh"), 3)
    ms_sah, host_sah = timed(lambda: build_tree(prims, verts, 4, "sah"), 2)
    build_tree_gpu(prims, verts, 4)  # warm-up: module load, allocator
    ms_gpu, dev = timed(lambda: build_tree_gpu(prims, verts, 4), 5)
    build_tree_gpu(prims, verts, 4, split_method="sah")
    ms_gpu_sah, dev_sah = timed(lambda: build_tree_gpu(prims, verts, 4, split_method="sah"), 5)

    def same(a, b):
        return bool(a.nodes.tobytes() == b.nodes.tobytes() and
                    a.ordered_prims.tobytes() == b.ordered_prims.tobytes() and a.depth == b.depth)
    def scene_host():
        t = build_tree(prims, verts, 4, "sah")
        BVHAggregate.from_tree(t.nodes, t.ordered_prims, verts).close()

    def scene_device():
        BVHAggregate.build_on_device(prims, verts, 4, "sah").close()

    ms_scene_host, _ = timed(scene_host, 2)
    scene_device()
    ms_scene_dev, _ = timed(scene_device, 5)
    out[name] = {"triangles": int(len(tris)), "sah_nodes": int(len(host_sah.nodes)),
                 "scene_create_ms_host_build_and_bake_sah": round(ms_scene_host, 1),
                 "scene_create_ms_device_build_and_bake_sah": round(ms_scene_dev, 1),
                 "hlbvh_nodes": int(len(host.nodes)),
                 "host_sah_ms": round(ms_sah, 1), "host_hlbvh_ms": round(ms_hl, 1),
                 "gpu_sah_ms_end_to_end": round(ms_gpu_sah, 1),
                 "gpu_sah_phases_ms (upload, big nodes, subtrees, layout+bounds, download)":
                     [round(v, 2) for v in dev_sah.gpu_ms],
                 "gpu_sah_identical_to_host": same(dev_sah, host_sah),
                 "gpu_hlbvh_ms_end_to_end": round(ms_gpu, 1),
                 "gpu_hlbvh_phases_ms (upload, device tree, host upper, emit, download)":
                     [round(v, 2) for v in dev.gpu_ms],
                 "gpu_hlbvh_identical_to_host": same(dev, host)}
print(json.dumps(out))
