"""IntersectClosest with the work items themselves (include/nnbvh.h: nnbvh_wavefront_*_items; reference:
wavefront/intersect.h:16-156, wavefront/workitems.soa).

CPU part: exports, C layout of the new structs against the Python dtypes, argument checks that fail before
any device work.  GPU part: the index queues equal nnbvh_wavefront_intersect_closest's, every slice is
bit-equal to the matching field of nnbvh_triangle_interactions_device on the same hits (the post-pass pinned
to the compiled reference), ray_o equals the oracle's OffsetRayOrigin, and the needs_host / capacity /
nullable-slice rules hold."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, _lib, build_tree, scene
from test_interaction import check_hits_against_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUEUES = _lib.CLOSEST_QUEUES
NEW_SYMBOLS = ("nnbvh_wavefront_enqueue_closest_items_device", "nnbvh_wavefront_intersect_closest_items",
               "nnbvh_wavefront_intersect_closest_and_shadow_items")


# ---------------------------------------------------------------------------------------------- CPU
def test_new_symbols_are_exported(nnbvh_lib):
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.EXPORTS, name


def test_header_structs_compile_as_c11_and_match_the_dtypes(nnbvh_lib):
    fields = []
    for k, c in _lib.ITEM_FIELDS.items():
        fields.append(f'printf("s {k} %zu\\n", offsetof(nnbvh_item_slices, {k}));')
    for k in _lib.ITEM_QUEUES + ("needs_host",):
        fields.append(f'printf("q {k} %zu\\n", offsetof(nnbvh_closest_items, {k}));')
    src = ("#include <stddef.h>\n#include <stdio.h>\n#include \"nnbvh.h\"\nint main(void) {\n"
           'printf("size %zu %zu\\n", sizeof(nnbvh_item_slices), sizeof(nnbvh_closest_items));\n'
           + "\n".join(fields) + "\nreturn 0;\n}\n")
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "layout.c"), os.path.join(td, "layout")
        open(c, "w").write(src)
        subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), c,
                        "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    sizes = out[0].split()
    assert int(sizes[1]) == _lib.ITEM_SLICES_DTYPE.itemsize and int(sizes[2]) == _lib.CLOSEST_ITEMS_DTYPE.itemsize
    for line in out[1:]:
        if not line:
            continue
        kind, name, off = line.split()
        dt = _lib.ITEM_SLICES_DTYPE if kind == "s" else _lib.CLOSEST_ITEMS_DTYPE
        assert dt.fields[name][1] == int(off), name


def _call_enqueue(mesh_handle, queues_rec, items_rec, max_rays=16):
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k in ("ox", "oy", "oz", "dx", "dy", "dz"):
        soa[k] = 0x1000  # never dereferenced: the call must fail before any device work
    return _lib.lib().nnbvh_wavefront_enqueue_closest_items_device(
        mesh_handle, max_rays, _lib.ptr(soa), None, ctypes.c_void_p(0x1000), None, 0, _lib.ptr(queues_rec),
        _lib.ptr(items_rec), None)


def test_bad_arguments_fail_before_device_work(nnbvh_lib):
    fake_mesh = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))
    q = np.zeros(1, _lib.CLOSEST_QUEUES_DTYPE)
    it = np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
    assert _call_enqueue(None, q, it) == 1, "NULL mesh"
    for queue, allowed in _lib.ITEM_QUEUE_FIELDS.items():
        for field in _lib.ITEM_FIELDS:
            if field in allowed:
                continue
            bad = np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
            if _lib.ITEM_FIELDS[field] == 1:
                bad[queue][field] = 0x2000
            else:
                bad[queue][field][0, -1] = 0x2000
            assert _call_enqueue(fake_mesh, q, bad) == 1, (queue, field)
            assert queue in _lib.last_error()
    for name in QUEUES:
        neg = np.zeros(1, _lib.CLOSEST_QUEUES_DTYPE)
        neg[name]["size"], neg[name]["items"], neg[name]["capacity"] = 0x3000, 0x3000, -1
        assert _call_enqueue(fake_mesh, neg, it) == 1, name
    neg = np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
    neg["needs_host"]["size"], neg["needs_host"]["capacity"] = 0x3000, -5
    assert _call_enqueue(fake_mesh, q, neg) == 1
    assert _call_enqueue(fake_mesh, q, it, max_rays=-1) == 1
    # the scene-level calls: NULL scene / NULL mesh
    L = _lib.lib()
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    assert L.nnbvh_wavefront_intersect_closest_items(None, fake_mesh, 4, _lib.ptr(soa), None, None, 0, None,
                                                      _lib.ptr(q), _lib.ptr(it), None) == 1
    assert L.nnbvh_wavefront_intersect_closest_and_shadow_items(
        None, None, 4, _lib.ptr(soa), None, None, 0, None, _lib.ptr(q), _lib.ptr(it), 4, _lib.ptr(soa), None, None,
        None, None, None, None, 0, None, None) == 1


# ---------------------------------------------------------------------------------------------- GPU
ALL_FIELDS = {k: v for k, v in _lib.ITEM_QUEUE_FIELDS.items()}


def soup_setup(seed, n_rays, n_tris=2500, host_prims=0):
    """Random soup, its shading mesh, a BVH over it (+ host-only primitives), rays with times."""
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    verts, prims = ss.random_soup(n_tris, 0, seed)
    tri_vertices = prims["v"][:, :3].copy()
    rng = np.random.default_rng(seed + 7)
    normals = rng.normal(size=(len(verts), 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = rng.random((len(verts), 2)).astype(np.float32)
    faces = rng.integers(0, 1000, len(prims)).astype(np.int32)
    mesh = ShadingMesh(verts, tri_vertices, normals=normals, uvs=uvs, face_indices=faces)
    allp, pb = prims, None
    if host_prims:
        extra = np.zeros(host_prims, prims.dtype)
        extra["kind"] = 3
        extra["id"] = len(prims) + np.arange(host_prims)
        allp = np.concatenate([prims, extra])
        lo = rng.uniform(-8, 8, (len(allp), 3)).astype(np.float32)
        pb = np.concatenate([lo, lo + rng.uniform(0.5, 2, (len(allp), 3)).astype(np.float32)], 1)
    tree = build_tree(allp, verts, prim_bounds=pb)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    rays = scene.random_rays(n_rays, verts.min(0) - 3, verts.max(0) + 3, seed + 1)
    rays["time"] = rng.random(n_rays).astype(np.float32)
    return verts, allp, mesh, agg, rays


def ray_queue(rays, dev, has_medium=None):
    import torch
    from nn_bvh_amd.wavefront import RayQueue
    rq = RayQueue.from_records(rays, dev)
    rq.time = torch.from_numpy(np.ascontiguousarray(rays["time"])).to(dev)
    if has_medium is not None:
        rq.has_medium = torch.from_numpy(has_medium).to(dev)
    return rq


def full_items(capacity, dev, fields=None):
    from nn_bvh_amd.wavefront import ItemSlices
    return {k: ItemSlices(capacity, (fields or ALL_FIELDS)[k], dev) for k in _lib.ITEM_QUEUES}


def reference_records(mesh, hits_t, rq, n, dev):
    """nnbvh_triangle_interactions_device on the same hits: the post-pass the slices must equal."""
    import torch
    out = torch.zeros(n * 192, dtype=torch.uint8, device=dev)
    mesh.interactions_device(hits_t.data_ptr(), n, out.data_ptr(), ray_queue=rq,
                             stream=torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(_lib.INTERACTION_DTYPE)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def expected_field(field, queue, rows, intr, hits, d):
    """What slot k of `field` holds for item rows[k] of `queue` (float32 / int32 arrays [k] or [c, k])."""
    r = intr[rows]
    hit = hits["prim"][rows] >= 0
    if field == "prim":
        return np.where(hit, hits["prim"][rows], -1).astype(np.int32)
    if field == "t_max":
        return np.where(hit, hits["t"][rows], np.float32(np.inf)).astype(np.float32)
    if field == "pi":
        return np.stack([r["pi_lo"][:, 0], r["pi_hi"][:, 0], r["pi_lo"][:, 1], r["pi_hi"][:, 1], r["pi_lo"][:, 2],
                         r["pi_hi"][:, 2]])
    if field == "p":
        return ((r["pi_lo"] + r["pi_hi"]) / np.float32(2)).astype(np.float32).T
    if field == "wo":
        return (-d[rows]).T if queue == "medium_sample" else r["wo"].T
    if field == "ray_d":
        return d[rows].T
    if field == "ray_o":
        in12 = np.concatenate([r["pi_lo"], r["pi_hi"], r["n"], d[rows]], 1)
        return ob.offset_batch(in12)[:, 0:3].T
    if field in ("face_index", "time"):
        return r[field]
    return r[field].T


def check_slices(name, q, sl, intr, hits, d, expect_idx=None, nan_equal=False):
    """Queue `name`'s index set and every requested slice against the post-pass records.  nan_equal (opt-in, for
    inputs that produce NaNs): a word that is a NaN on both sides counts as equal."""
    size = q.Size()
    k = min(size, q.capacity)
    idx = q.items[:k].cpu().numpy()
    if expect_idx is not None:
        assert size == len(expect_idx) and np.array_equal(np.sort(idx), expect_idx), name
    order = np.argsort(idx)
    rows = idx[order]
    hit = hits["prim"][rows] >= 0
    for field, t in sl.fields.items():
        got = t.cpu().numpy()[..., :k][..., order]
        exp = expected_field(field, name, rows, intr, hits, d)
        if field in ("prim", "t_max"):
            assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(exp).view(np.uint32)), (name, field)
            continue
        # a miss inside a medium carries prim and t_max only
        if not hit.any():
            continue
        g, e = got[..., hit], np.asarray(exp)[..., hit]
        if field == "face_index":
            assert np.array_equal(g, e), (name, field)
        else:
            diff = (bits(g) != bits(e)) & ~(nan_equal & np.isnan(g) & np.isnan(e))
            bad = np.nonzero(diff.reshape(-1, hit.sum()).any(0))[0]
            assert len(bad) == 0, f"{name}.{field} differs on {len(bad)} of {hit.sum()} items, first {rows[hit][bad[:5]]}"
    return rows


def run_items(wf, mesh, max_rays, rq, dev, hits_t, fields=None, capacity=None, needs_host=True, **kw):
    from nn_bvh_amd.wavefront import WorkQueue
    cap = max_rays if capacity is None else capacity
    queues = {k: WorkQueue(cap, dev) for k in QUEUES}
    items = full_items(cap, dev, fields)
    nh = WorkQueue(cap, dev) if needs_host else None
    wf.IntersectClosestItems(max_rays, rq, mesh, items=items, needs_host=nh, hits=hits_t, **queues, **kw)
    return queues, items, nh


@pytest.mark.gpu
@pytest.mark.parametrize("device_size", [None, 5000, 0])
def test_gpu_items_equal_index_queues_and_post_pass(device_size):
    import torch
    from nn_bvh_amd.wavefront import WavefrontAggregate, WorkQueue
    max_rays = 7001
    verts, prims, mesh, agg, rays = soup_setup(21, max_rays)
    n = max_rays if device_size is None else device_size
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    has_medium = (rng.random(max_rays) < 0.15).astype(np.uint8)
    dev = torch.device("cuda", 0)
    rq = ray_queue(rays, dev, has_medium)
    if device_size is not None:
        rq.size.fill_(device_size)
    wf = WavefrontAggregate(agg, prim_class)
    old = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    hits_old = torch.zeros((max_rays, 32), dtype=torch.uint8, device=dev)
    wf.IntersectClosest(max_rays, rq, hits=hits_old, **old)
    hits_t = torch.zeros((max_rays, 32), dtype=torch.uint8, device=dev)
    queues, items, nh = run_items(wf, mesh, max_rays, rq, dev, hits_t)
    torch.cuda.synchronize()
    assert torch.equal(hits_t, hits_old)
    assert nh.Size() == 0
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    intr = reference_records(mesh, hits_t, rq, max(n, 1), dev)
    d = np.ascontiguousarray(rays["d"])
    for k in QUEUES:
        exp = np.sort(old[k].indices().cpu().numpy())
        got = np.sort(queues[k].indices().cpu().numpy())
        assert queues[k].Size() == old[k].Size() and np.array_equal(got, exp), k
        if k in items:
            check_slices(k, queues[k], items[k], intr, hits, d, exp)
    if n:
        med = queues["medium_sample"].indices().cpu().numpy()
        assert (hits["prim"][med] >= 0).any() and (hits["prim"][med] < 0).any()
        for k in _lib.ITEM_QUEUES:
            assert queues[k].Size() > 0, k
    agg.close()
    mesh.close()


@pytest.mark.gpu
def test_gpu_items_full_path_patches_uvs_instances():
    """The FULL instance: smooth normals, uvs, bilinear patches (with and without uv), static instances."""
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import WavefrontAggregate
    from test_instancing import two_level_scene
    verts, nodes, prims, instances, n_top, _ = two_level_scene(3, 50)
    prims = prims.copy()
    prims["id"] = np.arange(len(prims))
    tri_vertices = np.full((len(prims), 3), -1, np.int32)
    patch_vertices = np.full((len(prims), 4), -1, np.int32)
    tri_vertices[prims["kind"] == 0] = prims["v"][prims["kind"] == 0][:, :3]
    patch_vertices[prims["kind"] == 1] = prims["v"][prims["kind"] == 1]
    rng = np.random.default_rng(8)
    normals = rng.normal(size=(len(verts), 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = rng.random((len(verts), 2)).astype(np.float32)
    flags = np.full(len(prims), _lib.TRI_HAS_N, np.uint8)
    flags[::2] |= _lib.TRI_HAS_UV  # kinds with and without uv
    mesh = ShadingMesh(verts, tri_vertices, normals=normals, uvs=uvs, patch_vertices=patch_vertices, tri_flags=flags)
    mesh.set_instances(instances)
    agg = BVHAggregate.from_tree(nodes, prims, verts, instances=instances, n_top_nodes=n_top)
    n = 40000
    rays = scene.random_rays(n, [-30, -30, -30], [30, 30, 30], 9)
    rays["time"] = rng.random(n).astype(np.float32)
    dev = torch.device("cuda", 0)
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    rq = ray_queue(rays, dev, has_medium)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    wf = WavefrontAggregate(agg, prim_class)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    queues, items, nh = run_items(wf, mesh, n, rq, dev, hits_t)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    assert nh.Size() == 0
    intr = reference_records(mesh, hits_t, rq, n, dev)
    exp = dict(zip(QUEUES, ob.wavefront_enqueue_closest(hits, has_medium, prim_class)))
    inside = patches = 0
    held = []
    for k in _lib.ITEM_QUEUES:
        rows = check_slices(k, queues[k], items[k], intr, hits, np.ascontiguousarray(rays["d"]), exp[k])
        inside += (hits["instance"][rows] > 0).sum()
        patches += (intr["status"][rows] == 3).sum()
        held.append(rows[hits["prim"][rows] >= 0])
    assert inside > 500 and patches > 20
    # ... and the post-pass records the slices equal are themselves the composed oracle's, on the same hits
    held = np.unique(np.concatenate(held))
    inst = instances[np.maximum(hits["instance"][held] - 1, 0)]
    golden_flags = 2 + (np.arange(len(prims)) % 2 == 0)  # normals everywhere, uv on the even ids
    counts = check_hits_against_oracle(intr, held, rays, hits, verts, tri_vertices, patch_vertices, golden_flags,
                                       inst["render_from_prim"].reshape(-1, 3, 4),
                                       inst["prim_from_render"].reshape(-1, 3, 4), normals=normals, uvs=uvs,
                                       what="records of the item queues")
    assert counts[0, True] + counts[1, True] == (hits["instance"][held] > 0).sum() > 500
    assert counts[1, False] + counts[1, True] == (intr["status"][held] == 3).sum() > 20
    for kind in (0, 1):  # triangles and patches inside instances, each with and without uv
        sel = held[(hits["instance"][held] > 0) & (intr["status"][held] == (1, 3)[kind])]
        for uv in (0, 1):
            assert ((golden_flags[hits["prim"][sel]] & 1) == uv).any(), (kind, uv)
    agg.close()
    mesh.close()


@pytest.mark.gpu
def test_gpu_items_animated_instances():
    import torch
    import test_animated as ta
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import WavefrontAggregate
    verts, prims, _, _, _, _, anims, oa, placements = ta.animated_scene(4, 36)
    nodes, aprims, instances, n_top = ta.rebuild_with_motion_bounds(verts, prims, placements, anims, oa)
    obj = aprims["kind"] != 2
    n_ids = int(aprims["id"][obj].max()) + 1
    tri_vertices = np.full((n_ids, 3), -1, np.int32)
    tri_vertices[aprims["id"][obj]] = aprims["v"][obj][:, :3]
    mesh = ShadingMesh(verts, tri_vertices)
    mesh.set_instances(instances, animated=anims)
    agg = BVHAggregate.from_tree(nodes, aprims, verts, instances=instances, n_top_nodes=n_top, animated=anims)
    n = 30000
    rays = scene.random_rays(n, [-25, -25, -25], [25, 25, 25], 5)
    rays["time"] = np.random.default_rng(6).uniform(-0.2, 1.2, n).astype(np.float32)
    dev = torch.device("cuda", 0)
    rq = ray_queue(rays, dev)
    wf = WavefrontAggregate(agg)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    queues, items, nh = run_items(wf, mesh, n, rq, dev, hits_t)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    intr = reference_records(mesh, hits_t, rq, n, dev)
    rows = check_slices("basic_eval_material", queues["basic_eval_material"], items["basic_eval_material"], intr,
                        hits, np.ascontiguousarray(rays["d"]), np.nonzero(hits["prim"] >= 0)[0])
    assert (hits["instance"][rows] > 0).sum() > 1000
    # ... and the post-pass records the slices equal are themselves the composed oracle's (Interpolate with the
    # device's sine, the path's documented exception)
    k = np.maximum(hits["instance"][rows] - 1, 0)
    try:
        ob.set_sin_mode(1)
        mm = ob.anim_interpolate(oa[k], rays["time"][rows])
    finally:
        ob.set_sin_mode(0)
    counts = check_hits_against_oracle(intr, rows, rays, hits, verts, tri_vertices, None,
                                       np.zeros(len(tri_vertices), np.int32), mm[:, :16].reshape(-1, 4, 4)[:, :3, :],
                                       mm[:, 16:].reshape(-1, 4, 4)[:, :3, :], what="records of the item queue")
    assert counts[0, True] == (hits["instance"][rows] > 0).sum()
    moving = (anims["actually_animated"][k] != 0) & (rays["time"][rows] > 0) & (rays["time"][rows] < 1)
    assert moving.sum() > 500
    agg.close()
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("with_size", [True, False])
def test_gpu_needs_host_routing(with_size):
    """Voided records (host-only primitives on the ray) and hits on primitives the mesh has no vertices for go
    to needs_host only; with needs_host.size NULL they are dropped."""
    import torch
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import WavefrontAggregate, WorkQueue
    n = 15000
    verts, prims, mesh, agg, rays = soup_setup(31, n, n_tris=3000, host_prims=25)
    # a second mesh that lacks the vertices of every fifth triangle
    tv = prims["v"][:, :3].copy()
    tv[prims["kind"] == 3] = -1
    tv[::5] = -1
    partial = ShadingMesh(verts, tv)
    rng = np.random.default_rng(3)
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    dev = torch.device("cuda", 0)
    rq = ray_queue(rays, dev, has_medium)
    wf = WavefrontAggregate(agg)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    queues = {k: WorkQueue(n, dev) for k in QUEUES}
    items = full_items(n, dev)
    nh = WorkQueue(n, dev)

    class NoSize:  # a needs_host queue without a size counter: pushes dropped
        def _wire(self, rec):
            rec["items"], rec["size"], rec["capacity"] = nh.items.data_ptr(), 0, n
    wf.IntersectClosestItems(n, rq, partial, items=items, needs_host=nh if with_size else NoSize(), hits=hits_t,
                             **queues)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    voided = hits["instance"] == -1
    no_verts = (hits["prim"] >= 0) & ~voided & (tv[np.maximum(hits["prim"], 0), 0] < 0)
    assert voided.sum() > 10 and no_verts.sum() > 100
    host = np.nonzero(voided | no_verts)[0]
    if with_size:
        assert nh.Size() == len(host)
        assert np.array_equal(np.sort(nh.indices().cpu().numpy()), host)
    pushed = np.concatenate([queues[k].indices().cpu().numpy() for k in QUEUES])
    assert not np.isin(pushed, host).any(), "a needs_host item landed in another queue"
    # everything else is routed as before
    rest = np.setdiff1d(np.arange(n), host)
    exp = dict(zip(QUEUES, ob.wavefront_enqueue_closest(hits, has_medium, None)))
    intr = reference_records(partial, hits_t, rq, n, dev)
    for k in QUEUES:
        e = np.intersect1d(exp[k], rest)
        assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), e), k
        if k in items:
            check_slices(k, queues[k], items[k], intr, hits, np.ascontiguousarray(rays["d"]), e)
    agg.close()
    mesh.close()
    partial.close()


@pytest.mark.gpu
def test_gpu_capacity_guards_and_nullable_slices():
    """A queue smaller than its pushes counts all of them and stores nothing past its capacity (guard words
    after every slice stay untouched); a subset of the fields gives the same values and leaves the
    unrequested buffers as they were."""
    import torch
    from nn_bvh_amd.wavefront import ItemSlices, WavefrontAggregate, WorkQueue
    n = 6000
    verts, prims, mesh, agg, rays = soup_setup(41, n)
    rng = np.random.default_rng(9)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    dev = torch.device("cuda", 0)
    rq = ray_queue(rays, dev, has_medium)
    wf = WavefrontAggregate(agg, prim_class)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    full_q, full_i, _ = run_items(wf, mesh, n, rq, dev, hits_t)
    torch.cuda.synchronize()
    # capacity: 100 slots of every queue, guard words behind them
    cap, guard = 100, 64
    small_q = {k: WorkQueue(cap + guard, dev) for k in QUEUES}
    for q in small_q.values():
        q.capacity = cap
        q.items.fill_(-7)
    small_i = full_items(cap + guard, dev)
    for sl in small_i.values():
        for t in sl.fields.values():
            t.view(torch.int32).fill_(0x7F7F7F7F)
    wf.IntersectClosestItems(n, rq, mesh, items=small_i, hits=hits_t, **small_q)
    torch.cuda.synchronize()
    for k in QUEUES:
        assert small_q[k].Size() == full_q[k].Size(), k
        assert (small_q[k].items[cap:].cpu().numpy() == -7).all(), k
        if full_q[k].Size() >= cap:
            assert np.isin(small_q[k].items[:cap].cpu().numpy(), full_q[k].indices().cpu().numpy()).all(), k
    for k, sl in small_i.items():
        for f, t in sl.fields.items():
            assert (t[..., cap:].contiguous().view(torch.int32).cpu().numpy() == 0x7F7F7F7F).all(), (k, f)
    # nullable slices: a subset, unrequested buffers poisoned and untouched
    subset = {k: v[::2] for k, v in ALL_FIELDS.items()}
    poisoned = {k: ItemSlices(n, [f for f in ALL_FIELDS[k] if f not in subset[k]], dev) for k in _lib.ITEM_QUEUES}
    for sl in poisoned.values():
        for t in sl.fields.values():
            t.view(torch.int32).fill_(0x5A5A5A5A)
    sub_q = {k: WorkQueue(n, dev) for k in QUEUES}
    sub_i = full_items(n, dev, subset)
    wf.IntersectClosestItems(n, rq, mesh, items=sub_i, hits=hits_t, **sub_q)
    torch.cuda.synchronize()
    for k in _lib.ITEM_QUEUES:
        order_full = np.argsort(full_q[k].indices().cpu().numpy())
        order_sub = np.argsort(sub_q[k].indices().cpu().numpy())
        m = full_q[k].Size()
        hit = full_i[k]["prim"].cpu().numpy()[:m][order_full] >= 0  # a miss in a medium: prim and t_max only
        for f in subset[k]:
            a = full_i[k][f].cpu().numpy()[..., :m][..., order_full]
            b = sub_i[k][f].cpu().numpy()[..., :m][..., order_sub]
            if f not in ("prim", "t_max"):
                a, b = a[..., hit], b[..., hit]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (k, f)
        for f, t in poisoned[k].fields.items():
            assert (t.view(torch.int32).cpu().numpy() == 0x5A5A5A5A).all(), (k, f)
    agg.close()
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("alpha", [False, True])
def test_gpu_closest_and_shadow_items(alpha):
    """The one-launch form (and, for a scene with alpha-tested triangles, its two-call fallback): shadow
    radiance bit-equal to nnbvh_wavefront_intersect_shadow, closest side as IntersectClosestItems."""
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    from test_wavefront import shadow_inputs
    n, ns, n_pixels = 7001, 6000, 9000
    verts, prims, mesh, agg, rays = soup_setup(51, n)
    if alpha:
        agg.close()
        aprims = prims.copy()
        aprims["kind"][::3] = 4  # alpha-tested triangles (constant alpha 0.5): the fallback path
        aprims["v"][::3, 3] = np.float32(0.5).view(np.int32)
        tree = build_tree(aprims, verts)
        agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    srays = scene.random_rays(ns, verts.min(0) - 3, verts.max(0) + 3, 77)
    srays["tmax"] = np.float32(1 - 1e-4)
    srays["d"] *= np.float32(12.0)
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    Ld, r_u, r_l, px, L = shadow_inputs(ns, n_pixels, 7)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    rq = ray_queue(rays, dev, has_medium)
    sq = RayQueue.from_records(srays, dev, shadow=True)
    wf = WavefrontAggregate(agg, prim_class)
    L_ref = t(L)
    wf.IntersectShadow(ns, sq, t(Ld), t(r_u), t(r_l), t(px), L_ref)
    ref_q = {k: WorkQueue(n, dev) for k in QUEUES}
    hits_ref = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    wf.IntersectClosest(n, rq, hits=hits_ref, **ref_q)
    L_t = t(L)
    queues = {k: WorkQueue(n, dev) for k in QUEUES}
    items = full_items(n, dev)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    wf.IntersectClosestAndShadowItems(n, rq, mesh, ns, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, items=items,
                                      hits=hits_t, **queues)
    torch.cuda.synchronize()
    assert np.array_equal(L_t.cpu().numpy().view(np.uint32), L_ref.cpu().numpy().view(np.uint32))
    assert torch.equal(hits_t, hits_ref)
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    intr = reference_records(mesh, hits_t, rq, n, dev)
    voided = np.nonzero(hits["instance"] == -1)[0]  # needs_host (not requested here) instead
    for k in QUEUES:
        exp = np.setdiff1d(ref_q[k].indices().cpu().numpy(), voided)
        assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), exp), k
        if k in items:
            check_slices(k, queues[k], items[k], intr, hits, np.ascontiguousarray(rays["d"]), exp)
    agg.close()
    mesh.close()


@pytest.mark.gpu
def test_gpu_items_from_kd_hits():
    """Hit records of a kd-tree through nnbvh_wavefront_enqueue_closest_items_device."""
    import torch
    from nn_bvh_amd.kdtree import KdTreeAggregate
    from nn_bvh_amd.wavefront import WorkQueue, enqueue_closest_items
    n = 8000
    verts, prims, mesh, agg, rays = soup_setup(61, n)
    agg.close()
    kd = KdTreeAggregate.build(prims, verts)
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(-1, 32).copy()).to(dev)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    kd.intersect_device(d_rays.data_ptr(), hits_t.data_ptr(), n, torch.cuda.current_stream(dev).cuda_stream)
    rng = np.random.default_rng(2)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    rq = ray_queue(rays, dev, has_medium)
    queues = {k: WorkQueue(n, dev) for k in QUEUES}
    items = full_items(n, dev)
    enqueue_closest_items(mesh, n, rq, hits_t, prim_class=torch.from_numpy(prim_class).to(dev), items=items,
                          **queues)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    assert (hits["prim"] >= 0).sum() > 500
    intr = reference_records(mesh, hits_t, rq, n, dev)
    exp = dict(zip(QUEUES, ob.wavefront_enqueue_closest(hits, has_medium, prim_class)))
    for k in QUEUES:
        assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), exp[k]), k
        if k in items:
            check_slices(k, queues[k], items[k], intr, hits, np.ascontiguousarray(rays["d"]), exp[k])
    kd.close()
    mesh.close()
