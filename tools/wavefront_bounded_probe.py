#!/usr/bin/env python3
"""IntersectShadowTr / IntersectOneRandom: the host-driven loop against the bounded, capturable form.
Forms, each on the same scene and the same device-resident queue:
  A    the unbounded call (a 4-byte count read back and a stream synchronise once or twice per pass)
  B    bounded at the number of passes the batch needs (the smallest max_passes that leaves nothing unfinished)
  B8   bounded at 8 passes: (B8 - B) / (8 - needed) is the cost of one pass over an empty list
  G8   B8 replayed from a captured graph
Shadow batches run twice: with about 5 % interface surfaces and with none (the common shadow batch: one pass).
Scene: a triangle soup at the density of the test scenes, built on the device.  One process; times are medians of
--reps runs after 3 warm-up runs with the spread (min, max) next to them, device time between two events; the forms
are run alternated (A B B8 G8 A B B8 G8), each twice.  host_ms: the time the call itself holds the host thread
(no synchronise after it), median of the same runs.  Prints one JSON line.
Usage: python tools/wavefront_bounded_probe.py [--tris 1000000] [--rays 4194304] [--items 1048576] [--reps 15] [--out DIR]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    import torch
    from nn_bvh_amd import BVHAggregate, make_prims, scene
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    n_tris, n, m, reps = arg("--tris", 1_000_000), arg("--rays", 1 << 22), arg("--items", 1 << 20), arg("--reps", 15)
    rng = np.random.default_rng(0)
    extent = 10.0 * (n_tris / 1500) ** (1 / 3)
    c = rng.uniform(-extent, extent, size=(n_tris, 1, 3))
    verts = (c + rng.uniform(-0.6, 0.6, size=(n_tris, 3, 3))).reshape(-1, 3).astype(np.float32)
    tris = np.arange(3 * n_tris, dtype=np.int32).reshape(n_tris, 3)
    agg = BVHAggregate.build_on_device(make_prims(tris), verts)
    mesh = ShadingMesh(verts, tris)
    dev = torch.device("cuda", 0)
    lo, hi = verts.min(0), verts.max(0)
    # segments a few surfaces long: shadow rays towards lights nearby, not across the whole soup
    rays = scene.random_rays(n, lo, hi, 4, tmax=np.float32(1 - 1e-4))
    rays["d"] *= np.float32(40.0 / (2 * extent))
    q = RayQueue.from_records(rays, dev, shadow=True)
    f4 = lambda: torch.rand((n, 4), dtype=torch.float32, device=dev) + 0.1  # noqa: E731
    Ld, r_u, r_l = f4(), f4(), f4()
    px = torch.randperm(n, device=dev).to(torch.int32)
    L = torch.zeros((n, 4), dtype=torch.float32, device=dev)
    state = torch.zeros(n, dtype=torch.uint8, device=dev)
    unfinished = torch.zeros(1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream(dev)

    def timed(fn, graph=None):
        ms, host = [], []
        with torch.cuda.stream(side):
            for i in range(reps + 3):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                t0 = time.perf_counter()
                if graph is not None:
                    graph.replay()
                else:
                    fn()
                t1 = time.perf_counter()
                b.record()
                torch.cuda.synchronize()
                if i >= 3:
                    ms.append(a.elapsed_time(b))
                    host.append((t1 - t0) * 1e3)
        return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                "host_ms": round(float(np.median(host)), 4)}

    def capture(fn):
        with torch.cuda.stream(side):
            fn()  # the stream's workspace gets its size
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            fn()
        torch.cuda.synchronize()
        return g

    def needed_passes(call):
        for p in range(1, 65):
            with torch.cuda.stream(side):
                call(p)
            torch.cuda.synchronize()
            if int(unfinished.item()) == 0:
                return p
        raise SystemExit("a walk longer than 64 surfaces: the bounded form does not cover this batch")

    def compare(call):
        """A / B / B8 / G8 alternated, each twice."""
        need = needed_passes(call)
        forms = {"A": lambda: call(None), "B": lambda: call(need), "B8": lambda: call(max(need, 8))}
        graph = capture(forms["B8"])
        res = {"passes_needed": need, "passes_B8": max(need, 8)}
        for again in ("", "_again"):
            for k, fn in forms.items():
                res[k + again] = timed(fn)
            res["G8" + again] = timed(None, graph)
        extra = max(need, 8) - need
        if extra:
            res["empty_pass_ms"] = round((min(res["B8"]["median_ms"], res["B8_again"]["median_ms"]) -
                                          min(res["B"]["median_ms"], res["B_again"]["median_ms"])) / extra, 4)
        del graph
        return res

    out = {"tris": n_tris, "shadow_rays": n, "items": m, "reps": reps, "grid_blocks": agg.info["grid_blocks"]}
    for label, share in (("shadow_5pct_interface", 0.05), ("shadow_no_interface", 0.0)):
        cls = np.where(rng.random(n_tris) < share, 2, 0).astype(np.uint8)
        wf = WavefrontAggregate(agg, cls)

        def shadow(max_passes, wf=wf):
            wf.IntersectShadowTr(n, q, mesh, Ld, r_u, r_l, px, L, state, max_passes=max_passes,
                                 unfinished=None if max_passes is None else unfinished)
        out[label] = compare(shadow)
        torch.cuda.synchronize()
        st = state.cpu().numpy()
        out[label]["share_arrived"] = round(float((st == 0).mean()), 4)
        out[label]["share_for_the_caller"] = round(float((st == 2).mean()), 6)

    # one-random walks: segments of the same length through the same soup, three materials
    seg = scene.random_rays(m, lo, hi, 6)
    p0 = torch.from_numpy(np.ascontiguousarray(seg["o"])).to(dev)
    p1 = torch.from_numpy((seg["o"] + seg["d"] * np.float32(40.0 / (2 * extent))).astype(np.float32)).to(dev)
    material = torch.from_numpy(rng.integers(0, 3, m).astype(np.int32)).to(dev)
    prim_material = torch.from_numpy(rng.integers(0, 3, n_tris).astype(np.int32)).to(dev)
    wf = WavefrontAggregate(agg)
    keep = []

    def one_random(max_passes):
        keep[:] = [wf.IntersectOneRandom(m, p0, p1, material, mesh, prim_material, max_passes=max_passes,
                                         unfinished=None if max_passes is None else unfinished)]
    out["one_random"] = compare(one_random)
    torch.cuda.synchronize()
    out["one_random"]["share_with_a_sample"] = round(float((keep[0][2] > 0).float().mean().item()), 4)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        os.makedirs(arg("--out", ""), exist_ok=True)
        with open(os.path.join(arg("--out", ""), "wavefront_bounded_probe.json"), "w") as f:
            f.write(line + "\n")
    agg.close()
    mesh.close()


if __name__ == "__main__":
    main()
