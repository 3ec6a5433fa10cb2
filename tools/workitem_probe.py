#!/usr/bin/env python3
"""Work items in the enqueue vs the interaction post-pass, on the crown dependent step.

The step is bench.py's dependent form (primary closest-hit; bounce-1 closest-hit with the shadow rays of
depth 0 in one launch; bounce-2 closest-hit), batches generated as bench.py generates them (one sample set).
Two forms, timed alternately in one process with device events after warm-up:
  (a) IntersectClosest / IntersectClosestAndShadow + ShadingMesh.interactions_device per closest queue
      (bench.py's step_wavefront_intr: 192-B nnbvh_interaction per ray, misses included);
  (b) IntersectClosestItems / IntersectClosestAndShadowItems with the fields the reference's work items carry
      (MaterialEvalWorkItem / HitAreaLightWorkItem / MediumSampleWorkItem / the next ray).
Checks on a seeded sample that (b)'s basic_eval_material slices equal (a)'s records, and prints one JSON
line: ms per step of both forms and the algorithmic byte counts of the two kernels (for achieved bytes/s
next to a `rocprofv3 --kernel-trace --stats` run of this script).

    python tools/workitem_probe.py [--spp 8] [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nn_bvh_amd import BVHAggregate, _lib, make_prims, raygen, scene  # noqa: E402
from nn_bvh_amd.interaction import ShadingMesh  # noqa: E402
from nn_bvh_amd.wavefront import ItemSlices, RayQueue, WavefrontAggregate, WorkQueue  # noqa: E402


def soa_queue(rays_t, dev, shadow=False):
    """RayQueue from the device ray records (8 floats: o, tmax, d, time) raygen produces."""
    r = rays_t.view(-1, 8)
    o, d = r[:, 0:3].t().contiguous(), r[:, 4:7].t().contiguous()
    return RayQueue(o, d, tmax=r[:, 3].contiguous() if shadow else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spp", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200000, help="items compared between the two forms")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    verts, tris, _ = scene.load_scene("crown")
    prims = make_prims(tris)
    agg = BVHAggregate.build_on_device(prims, verts, 4, "sah")
    xres, yres = scene.CAMERAS["crown"][4], scene.CAMERAS["crown"][5]
    _, px, py = scene.camera_rays("crown", seed=1, sample=0, return_pixels=True)
    ds = raygen.DeviceScene(verts, tris, dev)
    d_px = torch.from_numpy(px.astype(np.float64)).to(dev)
    d_py = torch.from_numpy(py.astype(np.float64)).to(dev)
    primary_t = torch.stack([ds.camera_rays("crown", d_px, d_py, seed=1, sample=s) for s in range(args.spp)],
                            1).reshape(-1, 8).contiguous()
    stream = torch.cuda.current_stream(dev).cuda_stream
    n_primary = len(primary_t)
    hits0 = torch.empty((n_primary, 32), dtype=torch.uint8, device=dev)
    agg.intersect_device(primary_t.data_ptr(), hits0.data_ptr(), n_primary, stream)
    bounce_t, _ = ds.bounce_rays(primary_t, hits0.view(-1), seed=[2, 0, 0])
    bhits0 = torch.empty((len(bounce_t), 32), dtype=torch.uint8, device=dev)
    agg.intersect_device(bounce_t.data_ptr(), bhits0.data_ptr(), len(bounce_t), stream)
    bounce2_t, _ = ds.bounce_rays(bounce_t, bhits0.view(-1), seed=[4, 0, 0])
    shadow_t, _ = ds.shadow_rays(primary_t, hits0.view(-1), seed=[3, 0, 0], quads=scene.CROWN_LIGHT_QUADS)
    n_bounce, n_bounce2, n_shadow = len(bounce_t), len(bounce2_t), len(shadow_t)
    del bhits0
    q_primary, q_bounce, q_bounce2 = soa_queue(primary_t, dev), soa_queue(bounce_t, dev), soa_queue(bounce2_t, dev)
    q_shadow = soa_queue(shadow_t, dev, shadow=True)
    gen = torch.Generator(device=dev).manual_seed(100)
    Ld = torch.rand((n_shadow, 4), generator=gen, device=dev) * 2.0
    ru = torch.rand((n_shadow, 4), generator=gen, device=dev) + 0.5
    rl = torch.rand((n_shadow, 4), generator=gen, device=dev) + 0.5
    pix = torch.arange(n_shadow, dtype=torch.int32, device=dev)
    Lw = torch.zeros((n_shadow, 4), dtype=torch.float32, device=dev)

    wf = WavefrontAggregate(agg, np.zeros(len(tris), np.uint8))
    smesh = ShadingMesh(verts, tris)
    outq = {k: WorkQueue(n_primary, dev) for k in _lib.CLOSEST_QUEUES}
    items = {k: ItemSlices(n_primary, _lib.ITEM_QUEUE_FIELDS[k], dev) for k in _lib.ITEM_QUEUES}
    hits = [torch.empty((n, 32), dtype=torch.uint8, device=dev) for n in (n_primary, n_bounce, n_bounce2)]
    d_intr = torch.empty(n_primary * 192, dtype=torch.uint8, device=dev)

    def reset():
        for q in outq.values():
            q.Reset()

    def step_a():
        reset()
        wf.IntersectClosest(n_primary, q_primary, hits=hits[0], **outq)
        reset()
        wf.IntersectClosestAndShadow(n_bounce, q_bounce, n_shadow, q_shadow, Ld, ru, rl, pix, Lw, hits=hits[1], **outq)
        reset()
        wf.IntersectClosest(n_bounce2, q_bounce2, hits=hits[2], **outq)
        for h, n, q in zip(hits, (n_primary, n_bounce, n_bounce2), (q_primary, q_bounce, q_bounce2)):
            smesh.interactions_device(h.data_ptr(), n, d_intr.data_ptr(), ray_queue=q, stream=stream)

    def step_b():
        reset()
        wf.IntersectClosestItems(n_primary, q_primary, smesh, items=items, hits=hits[0], **outq)
        reset()
        wf.IntersectClosestAndShadowItems(n_bounce, q_bounce, smesh, n_shadow, q_shadow, Ld, ru, rl, pix, Lw,
                                          items=items, hits=hits[1], **outq)
        reset()
        wf.IntersectClosestItems(n_bounce2, q_bounce2, smesh, items=items, hits=hits[2], **outq)

    # ---- (b)'s slices against (a)'s records on the primary queue, seeded sample
    reset()
    wf.IntersectClosest(n_primary, q_primary, hits=hits[0], **outq)
    smesh.interactions_device(hits[0].data_ptr(), n_primary, d_intr.data_ptr(), ray_queue=q_primary, stream=stream)
    reset()
    wf.IntersectClosestItems(n_primary, q_primary, smesh, items=items, hits=hits[0], **outq)
    torch.cuda.synchronize()
    q = outq["basic_eval_material"]
    size = q.Size()
    rng = np.random.default_rng(7)
    pick = torch.from_numpy(rng.choice(size, min(args.sample, size), replace=False)).to(dev)
    idx = q.items[pick].long()
    rec = d_intr.view(-1, 192)[idx].cpu().numpy().view(_lib.INTERACTION_DTYPE).reshape(-1)
    sl = items["basic_eval_material"]
    mismatch = {}
    pi = np.stack([rec["pi_lo"][:, 0], rec["pi_hi"][:, 0], rec["pi_lo"][:, 1], rec["pi_hi"][:, 1], rec["pi_lo"][:, 2],
                   rec["pi_hi"][:, 2]])
    for f in _lib.ITEM_QUEUE_FIELDS["basic_eval_material"]:
        got = sl[f][..., pick].cpu().numpy()
        exp = {"prim": rec["prim"], "pi": pi}.get(f)
        if exp is None:
            exp = rec[f] if rec[f].ndim == 1 else rec[f].T
        mismatch[f] = int((np.ascontiguousarray(got).view(np.uint32) !=
                           np.ascontiguousarray(exp).view(np.uint32)).reshape(-1, len(pick)).any(0).sum())
    n_hit = [int(size)]
    for n, qq, h in ((n_bounce, q_bounce, hits[1]), (n_bounce2, q_bounce2, hits[2])):
        reset()
        wf.IntersectClosest(n, qq, hits=h, **outq)
        torch.cuda.synchronize()
        n_hit.append(outq["basic_eval_material"].Size())

    # ---- timing, the two forms alternately
    for _ in range(args.warmup):
        step_a()
        step_b()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ms_a, ms_b = [], []
    for _ in range(args.reps):
        ev[0].record()
        step_a()
        ev[1].record()
        step_b()
        ev[2].record()
        torch.cuda.synchronize()
        ms_a.append(ev[0].elapsed_time(ev[1]))
        ms_b.append(ev[1].elapsed_time(ev[2]))

    # ---- algorithmic bytes of the two kernels per step (mesh gathers counted once per hit: 3 indices + 3 vertices)
    n_all = n_primary + n_bounce + n_bounce2
    hits_total = sum(n_hit)
    gather = 12 + 36
    material_slices = sum(_lib.ITEM_FIELDS[f] for f in _lib.ITEM_QUEUE_FIELDS["basic_eval_material"])
    bytes_postpass = n_all * (32 + 16) + hits_total * (12 + gather + 192 - 16)  # miss: 16-B tail store
    bytes_items = n_all * 32 + hits_total * (12 + gather + 4 + 4 * material_slices) + (n_all - hits_total) * 4
    print(json.dumps({
        "probe": "workitem_probe", "scene": "crown", "spp": args.spp,
        "rays": {"primary": n_primary, "bounce": n_bounce, "bounce2": n_bounce2, "shadow": n_shadow},
        "hits_basic_material": n_hit,
        "ms_per_step_a_postpass": round(float(np.median(ms_a)), 4),
        "ms_per_step_b_items": round(float(np.median(ms_b)), 4),
        "ms_a_all": [round(x, 4) for x in ms_a], "ms_b_all": [round(x, 4) for x in ms_b],
        "algorithmic_bytes_per_step": {"k_triangle_interactions": bytes_postpass,
                                       "wf_enqueue_closest_items": bytes_items},
        "sample_compared": int(len(pick)), "sample_mismatches": mismatch,
    }))
    bad = {k: v for k, v in mismatch.items() if v}
    agg.close()
    smesh.close()
    if bad:
        raise SystemExit(f"form (b) differs from form (a) on {bad}")


if __name__ == "__main__":
    main()
