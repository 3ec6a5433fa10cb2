"""One process = one build: times the two-level alpha scene of
test_device_alpha_patches_and_smooth_triangles_inside_instances (static form) on device-resident rays.
usage: PYTHONPATH=<root of the build to time> python tools/two_level_alpha_probe.py TAG [--textured]
(TAG names the build in the JSON line; --textured: the scene's alpha-tested triangles, kinds 4 .. 7, turned into kinds
16 .. 19 over the three textures of tests/alpha_texture_oracle.py.  The package is the first nn_bvh_amd on PYTHONPATH,
so a checkout of another commit with its own library can be timed by the same file.)"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(1, os.path.join(os.path.dirname(HERE), "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import nn_bvh_amd  # noqa: E402
from nn_bvh_amd import BVHAggregate, instancing, scene  # noqa: E402

import test_alpha as ta  # noqa: E402
from test_oracle_vs_reference_live import random_affine  # noqa: E402

tag = sys.argv[1]
textured = "--textured" in sys.argv
N = 4_000_000

verts, prims, normals, alpha, kinds = ta.alpha_patch_scene(41, 500, 700)
rng = np.random.default_rng(3)
prims = prims.copy()
tri_alpha = (kinds == 4) | (kinds == 5)
smooth = tri_alpha & (rng.random(len(prims)) < 0.5)
prims["kind"] = np.where(smooth, kinds + 2, kinds)
uvs = ta.patch_uvs(verts)
n_place = 6
M, _ = random_affine(rng, n_place)
M[:, :3, 3] = rng.uniform(-15, 15, size=(n_place, 3))
Mi = np.linalg.inv(M.astype(np.float64)).astype(np.float32)
placements = [(0, M[j, :3].reshape(12), Mi[j, :3].reshape(12)) for j in range(n_place)]
kw = {}
if textured:
    import alpha_texture_oracle as ato
    t = (prims["kind"] >= 4) & (prims["kind"] <= 7)
    prims["kind"][t] += 12
    prims["v"][t, 3] = np.arange(t.sum()) % 3
    kw["alpha_textures"] = ato.scene_textures(0)
nodes, aprims, instances, n_top = instancing.assemble_two_level(prims[:0], verts, [prims], placements)
obj = aprims["kind"] != 2
a_ord = np.zeros(len(aprims), np.float32)
a_ord[obj] = alpha[aprims["id"][obj]]
agg = BVHAggregate.from_tree(nodes, aprims, verts, instances=instances, n_top_nodes=n_top, normals=normals, uvs=uvs,
                             prim_alpha=a_ord, **kw)
rays = scene.random_rays(N, [-25, -25, -25], [25, 25, 25], 13)
dev = torch.device("cuda", 0)
d_rays = torch.from_numpy(rays.view(np.uint8).reshape(N, 32)).to(dev)
d_hits = torch.zeros((N, 32), dtype=torch.uint8, device=dev)
d_occ = torch.zeros((N,), dtype=torch.uint8, device=dev)


def timed(batch, reps=7):
    out = []
    for k in range(reps + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        agg.trace_batches_device([batch])
        torch.cuda.synchronize()
        if k >= 2:
            out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


res = {"tag": tag, "textured": textured, "package": os.path.dirname(nn_bvh_amd.__file__), "rays": N,
       "closest_ms": timed(("closest", d_rays.data_ptr(), N, d_hits.data_ptr())),
       "any_ms": timed(("any", d_rays.data_ptr(), N, d_occ.data_ptr()))}
hits = d_hits.cpu().numpy().view(nn_bvh_amd._lib.HIT_DTYPE).reshape(-1)
res["hits_inside"] = int((hits["instance"] > 0).sum())
res["occluded"] = int((d_occ.cpu().numpy() == 1).sum())
import zlib  # noqa: E402
res["hits_crc"] = zlib.crc32(hits.tobytes())
agg.close()
print(json.dumps(res), flush=True)
