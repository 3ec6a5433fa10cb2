"""One-launch batches and wavefront queue calls on kd-tree scenes (nnbvh_kd_trace_batches_device,
nnbvh_kd_wavefront_*): argument checks without a device; on the device, batches against the flat kd calls and the
oracle's KdTreeAggregate, the queue calls against the enqueue rules and RecordShadowRayResult in numpy, the work items
against the scene-free enqueue call, graph capture, and a cross-check with the BVH calls."""
import ctypes

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, NNBVHError, _lib, build_tree, scene
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree, kd_from_planes

QUEUES = _lib.CLOSEST_QUEUES
KD_CALLS = ("nnbvh_kd_trace_batches_device", "nnbvh_kd_wavefront_intersect_closest",
            "nnbvh_kd_wavefront_intersect_shadow", "nnbvh_kd_wavefront_intersect_closest_and_shadow",
            "nnbvh_kd_wavefront_intersect_closest_items", "nnbvh_kd_wavefront_intersect_closest_and_shadow_items")
ERR_ARG = 1


# ---------------------------------------------------------------------------------------------- CPU
def test_kd_entry_points_are_exported_with_prototypes():
    L = _lib.lib()
    for name in KD_CALLS:
        assert name in _lib.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int, name
    for name in KD_CALLS[1:]:
        assert getattr(L, name).argtypes == getattr(L, name.replace("nnbvh_kd_", "nnbvh_")).argtypes, name
    header = open(_lib.LIB_PATH.rsplit("nn_bvh_amd", 1)[0] + "include/nnbvh.h").read()
    for name in KD_CALLS:
        assert name + "(" in header, name


def _soa(n=16):
    """A ray_soa record over host memory: the calls below must fail before anything reads it."""
    buf = np.zeros((6, n), np.float32)
    rec = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k, name in enumerate(("ox", "oy", "oz", "dx", "dy", "dz")):
        rec[name] = buf[k].ctypes.data
    return rec, buf


def _queue_calls(L, scene_handle, max_rays, max_shadow):
    """The five queue calls with well-formed arguments apart from the scene / the two sizes."""
    rec, buf = _soa()
    qrec = np.zeros(1, _lib.CLOSEST_QUEUES_DTYPE)
    irec = np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
    f = np.zeros((16, 4), np.float32)
    px = np.zeros(16, np.int32)
    hits = np.zeros(16, HIT_DTYPE)
    p = _lib.ptr
    mesh = ctypes.c_void_p(1)  # never dereferenced: the scene / size checks come first
    shadow = (max_shadow, p(rec), None, p(f), p(f), p(f), p(px), p(f), 16, None, None)
    keep = (rec, buf, qrec, irec, f, px, hits)
    return keep, [
        ("closest", lambda: L.nnbvh_kd_wavefront_intersect_closest(scene_handle, max_rays, p(rec), None, None, 0, p(hits), p(qrec), None)),
        ("shadow", lambda: L.nnbvh_kd_wavefront_intersect_shadow(scene_handle, *shadow)),
        ("pair", lambda: L.nnbvh_kd_wavefront_intersect_closest_and_shadow(scene_handle, max_rays, p(rec), None, None, 0, p(hits), p(qrec), *shadow)),
        ("items", lambda: L.nnbvh_kd_wavefront_intersect_closest_items(scene_handle, mesh, max_rays, p(rec), None, None, 0, p(hits), p(qrec), p(irec), None)),
        ("pair_items", lambda: L.nnbvh_kd_wavefront_intersect_closest_and_shadow_items(scene_handle, mesh, max_rays, p(rec), None, None, 0, p(hits), p(qrec), p(irec), *shadow)),
    ]


def test_kd_calls_reject_bad_arguments_before_any_device_work():
    L = _lib.lib()
    fake = ctypes.c_void_p(8)  # a non-NULL "scene" that must never be dereferenced: the checks below come first
    batch = np.zeros(4, _lib.BATCH_DTYPE)
    batch["n"] = 8
    batch["d_rays"] = batch["d_out"] = 64
    # NULL scene
    assert L.nnbvh_kd_trace_batches_device(None, _lib.ptr(batch), 2, None) == ERR_ARG
    assert "kd_trace_batches_device" in _lib.last_error()
    keep, calls = _queue_calls(L, None, 8, 8)
    for name, call in calls:
        assert call() == ERR_ARG, name
        assert "kd_wavefront_intersect_" in _lib.last_error(), name
    assert L.nnbvh_kd_scene_set_option(None, b"read_soa", 0) == ERR_ARG
    # n_batches outside 1..4
    for nb in (0, 5, -1):
        assert L.nnbvh_kd_trace_batches_device(fake, _lib.ptr(batch), nb, None) == ERR_ARG, nb
    # a batch of 2^28 rays or more, a negative one, an unknown kind
    for field, value in (("n", 1 << 28), ("n", -1), ("kind", 2)):
        bad = batch.copy()
        bad[field][1] = value
        assert L.nnbvh_kd_trace_batches_device(fake, _lib.ptr(bad), 2, None) == ERR_ARG, (field, value)
    # negative max_rays / queues of 2^28 rays or more
    for mr, ms in ((-1, 8), (8, -1), (1 << 28, 8), (8, 1 << 28)):
        keep, calls = _queue_calls(L, fake, mr, ms)
        for name, call in calls:
            if (name in ("closest", "items") and ms != 8) or (name == "shadow" and mr != 8):
                continue  # the call has no such argument
            assert call() == ERR_ARG, (name, mr, ms)


def test_wavefront_aggregate_over_a_kd_handle_refuses_the_unsupported_methods():
    torch = pytest.importorskip("torch")
    from nn_bvh_amd.wavefront import WavefrontAggregate
    kd = KdTreeAggregate(None, np.zeros(6, np.float32))
    wf = WavefrontAggregate(kd)
    assert wf._name("intersect_closest") == "nnbvh_kd_wavefront_intersect_closest"
    with pytest.raises(NNBVHError, match="kd-tree"):
        wf.IntersectShadowTr(0, None, None, None, None, None, None, None)
    with pytest.raises(NNBVHError, match="kd-tree"):
        wf.IntersectOneRandom(0, None, None, None, None)
    del torch


def test_oracle_kd_and_bvh_agree_on_a_soup_without_duplicates():
    """The premise of the GPU cross-check: on this soup no ray has to be left out for a prim tie at equal t."""
    verts, prims, rays = _cross_scene()
    t = build_kd_tree(prims, verts)
    bt = build_tree(prims, verts)
    hk = ob.kd_closest(t.nodes, t.prim_indices, prims, verts, t.bounds, rays, 4)
    hb = ob.closest(bt.nodes, bt.ordered_prims, verts, rays, nthreads=4)
    assert np.array_equal(hk["t"].view(np.uint32), hb["t"].view(np.uint32))
    assert (hk["prim"] != hb["prim"]).sum() == 0
    assert (hk["prim"] >= 0).mean() > 0.2


def _cross_scene():
    verts, prims = ss.random_soup(3000, 0, 71)
    tri = verts[prims["v"][:, :3]].reshape(len(prims), 9)
    assert len(np.unique(tri, axis=0)) == len(prims), "duplicated triangles in the soup"
    rays = scene.random_rays(9000, verts.min(0) - 3, verts.max(0) + 3, 72)
    return verts, prims, rays[(rays["d"] != 0).all(1)]


# ---------------------------------------------------------------------------------------------- GPU
def _dev():
    import torch
    return torch.device("cuda", 0)


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


class Batches:
    """Device buffers of up to four batches (kind, rays) and the nnbvh_batch records over them."""

    def __init__(self, spec, counts=True):
        import torch
        self.spec = spec
        self.rays = [_to_dev(r) if len(r) else torch.zeros(32, dtype=torch.uint8, device=_dev()) for _, r in spec]
        self.out, self.vis, self.tst = [], [], []
        for kind, r in spec:
            n = max(len(r), 1)
            self.out.append(torch.full((n * (32 if kind == "closest" else 1),), 0xAB, dtype=torch.uint8, device=_dev()))
            self.vis.append(torch.full((n,), -7, dtype=torch.int32, device=_dev()) if counts and kind == "any" else None)
            self.tst.append(torch.full((n,), -7, dtype=torch.int32, device=_dev()) if counts and kind == "any" else None)

    def tuples(self):
        return [(kind, self.rays[k].data_ptr(), len(r), self.out[k].data_ptr(),
                 self.vis[k].data_ptr() if self.vis[k] is not None else None,
                 self.tst[k].data_ptr() if self.tst[k] is not None else None)
                for k, (kind, r) in enumerate(self.spec)]

    def results(self):
        import torch
        torch.cuda.synchronize()
        res = []
        for k, (kind, r) in enumerate(self.spec):
            o = self.out[k].cpu().numpy()
            if kind == "closest":
                res.append(o.view(HIT_DTYPE)[:len(r)])
            else:
                res.append((o[:len(r)], None if self.vis[k] is None else self.vis[k].cpu().numpy()[:len(r)],
                            None if self.tst[k] is None else self.tst[k].cpu().numpy()[:len(r)]))
        return res


def _flat(agg, kind, rays):
    """The flat device calls on the same rays."""
    import torch
    n = len(rays)
    d = _to_dev(rays)
    if kind == "closest":
        out = torch.zeros(n * 32, dtype=torch.uint8, device=_dev())
        agg.intersect_device(d.data_ptr(), out.data_ptr(), n, _stream())
        torch.cuda.synchronize()
        return out.cpu().numpy().view(HIT_DTYPE)
    out = torch.zeros(n, dtype=torch.uint8, device=_dev())
    vis = torch.zeros(n, dtype=torch.int32, device=_dev())
    tst = torch.zeros(n, dtype=torch.int32, device=_dev())
    agg.intersect_p_device(d.data_ptr(), out.data_ptr(), n, vis.data_ptr(), tst.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu().numpy(), vis.cpu().numpy(), tst.cpu().numpy()


def _check_batches(agg, tree, prims, verts, spec, oracle=True):
    """Up to four batches in one launch = the flat calls = the oracle, with and without the any-hit counts.  (nnbvh_batch
    carries host sizes only; device-resident sizes are the queue calls', see
    test_gpu_kd_device_size_above_the_bound_and_negative and the device_size / sizes parameters below.)"""
    b = Batches(spec)
    agg.trace_batches_device(b.tuples(), _stream())
    for (kind, rays), got in zip(spec, b.results()):
        if len(rays) == 0:
            continue
        flat = _flat(agg, kind, rays)
        if kind == "closest":
            assert got.tobytes() == flat.tobytes(), "batch records differ from nnbvh_kd_intersect_closest_device"
            if oracle:
                exp = ob.kd_closest(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)
                for f in ("prim", "t", "b0", "b1", "b2", "nodes_visited", "prim_tests"):
                    assert np.array_equal(got[f].view(np.uint32), exp[f].view(np.uint32)), f
        else:
            for g, f in zip(got, flat):
                assert np.array_equal(g, f), "any-hit batch differs from nnbvh_kd_intersect_any_device"
            if oracle:
                eo, ev, et = ob.kd_any_hit(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)
                assert np.array_equal(got[0], eo) and np.array_equal(got[1], ev) and np.array_equal(got[2], et)
    # without the counts
    b2 = Batches(spec, counts=False)
    agg.trace_batches_device(b2.tuples(), _stream())
    for (kind, rays), g1, g2 in zip(spec, b.results(), b2.results()):
        if kind == "any":
            assert np.array_equal(g1[0], g2[0])
        else:
            assert g1.tobytes() == g2.tobytes()
    return b.results()


def _soup_rays(verts, prims, seeds, n=40000):
    return np.concatenate([scene.random_rays(n, verts.min(0) - 2, verts.max(0) + 2, seeds[0]),
                           scene.random_rays(n // 4, verts.min(0), verts.max(0), seeds[1], tmax=0.5),
                           ss.edge_case_rays(verts, prims, seeds[2])])  # zero, -0 and denormal components among them (no NaN / inf)


def _four(rays, shadow_rays):
    """closest, any, closest, any with sizes ~60 k, 1, 0 and a few thousand."""
    return [("closest", rays[:60000]), ("any", shadow_rays[:1]), ("closest", rays[:0]), ("any", shadow_rays[:7001])]


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_gpu_kd_batches_equal_single_calls_and_oracle_on_soups_with_patches(max_prims):
    verts, prims = ss.random_soup(6000, 800, 11)
    tree = build_kd_tree(prims, verts, max_prims=max_prims)
    rays = _soup_rays(verts, prims, (12, 13, 14), 50000)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)
    res = _check_batches(agg, tree, prims, verts, _four(rays, rays[::-1].copy()))
    assert (res[0]["prim"] >= 0).mean() > 0.2 and res[0]["nodes_visited"].max() > 20
    # another order of kinds and sizes: any first, a single closest ray
    _check_batches(agg, tree, prims, verts, [("any", rays[:30000]), ("closest", rays[5:6]), ("any", rays[:0]),
                                             ("closest", rays[100:9000])], oracle=False)
    agg.close()


@pytest.mark.gpu
def test_gpu_kd_batches_lean_mesh_host_prims_deep_stack_and_nss_tree():
    # lean instance: connected mesh, ties
    verts, prims = ss.grid_mesh(64, 3)
    tree = build_kd_tree(prims, verts)
    rays = np.concatenate([scene.random_rays(60000, verts.min(0) - 1, verts.max(0) + 1, 15),
                           ss.edge_case_rays(verts, prims, 16)])
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)
    _check_batches(agg, tree, prims, verts, _four(rays, rays[::-1].copy()))
    agg.close()
    # an nss-style tree over the same mesh
    planes = np.zeros((15, 5), np.float32)
    for lvl in range(4):
        for k in range(2 ** lvl):
            planes[2 ** lvl - 1 + k, lvl % 3] = 1
            planes[2 ** lvl - 1 + k, 4] = (k + 0.5) / 2 ** lvl if lvl % 3 == 0 else 0.5
    nss = kd_from_planes(planes, prims, verts)
    agg = KdTreeAggregate.from_tree(nss.nodes, nss.prim_indices, prims, verts, nss.bounds)
    _check_batches(agg, nss, prims, verts, _four(rays[::8].copy(), rays[::-8].copy()))
    agg.close()
    # host-only primitives void the rays that reach them, as in the flat calls
    verts, prims = ss.random_soup(2000, 0, 17)
    extra = np.zeros(15, prims.dtype)
    extra["kind"], extra["id"] = 3, len(prims) + np.arange(15)
    allp = np.concatenate([prims, extra])
    rng = np.random.default_rng(18)
    lo = rng.uniform(-8, 8, (len(allp), 3)).astype(np.float32)
    pb = np.concatenate([lo, lo + rng.uniform(0.5, 2, (len(allp), 3)).astype(np.float32)], 1)
    tree = build_kd_tree(allp, verts, prim_bounds=pb)
    rays = scene.random_rays(20000, verts.min(0) - 2, verts.max(0) + 2, 19)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, allp, verts, tree.bounds)
    res = _check_batches(agg, tree, allp, verts, _four(rays, rays[::-1].copy()))
    assert (res[0]["instance"] == -1).any() and (res[3][0] == 2).any()
    agg.close()
    # deep tree: to-visit lists beyond the LDS window (HBM spill path)
    verts, prims = ss.random_soup(4000, 0, 20, extent=0.5, size=0.4)
    verts = verts * np.array([400, 1, 1], np.float32)
    tree = build_kd_tree(prims, verts, max_prims=1, max_depth=40)
    o = np.zeros(8000, _lib.RAY_DTYPE)
    rng = np.random.default_rng(21)
    o["o"] = np.stack([np.full(8000, -250.0), rng.uniform(-.5, .5, 8000), rng.uniform(-.5, .5, 8000)], 1)
    o["d"] = np.stack([np.ones(8000), rng.uniform(-.002, .002, 8000), rng.uniform(-.002, .002, 8000)], 1)
    o["tmax"] = np.inf
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)
    res = _check_batches(agg, tree, prims, verts, _four(o, o[::-1].copy()))
    assert res[0]["nodes_visited"].max() > 60
    agg.close()


@pytest.mark.gpu
def test_gpu_kd_batches_with_attribute_reading_alpha_kinds():
    from test_alpha import alpha_patch_scene, patch_uvs
    verts, prims, normals, alpha, kinds = alpha_patch_scene(43, 1500, 2500)
    rng = np.random.default_rng(4)
    prims = prims.copy()
    smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
    prims["kind"] = np.where(smooth, kinds + 2, kinds)
    uvs = patch_uvs(verts)
    tree = build_kd_tree(prims, verts, max_prims=2)
    rays = np.concatenate([scene.random_rays(40000, verts.min(0) - 1, verts.max(0) + 1, 21),
                           scene.random_rays(8000, verts.min(0), verts.max(0), 22, tmax=0.6)])
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, normals=normals, uvs=uvs,
                                    prim_alpha=alpha)
    try:
        ob.set_vertex_normals(normals)
        ob.set_vertex_uvs(uvs)
        ob.set_prim_alpha(alpha)
        res = _check_batches(agg, tree, prims, verts, _four(rays, rays[::-1].copy()))
    finally:
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
    hit_kind = prims["kind"][np.maximum(res[0]["prim"], 0)]
    for k in (6, 7, 8, 9, 10, 11, 12, 13, 14, 15):
        assert ((hit_kind == k) & (res[0]["prim"] >= 0)).sum() > 50, k
    agg.close()
    # alpha-tested triangles with a constant alpha (kinds 4 / 5): the PATCH instance without attributes
    from test_alpha import alpha_scene
    verts, prims, alpha, kinds = alpha_scene(6, 2500)
    tree = build_kd_tree(prims, verts, max_prims=2)
    rays = scene.random_rays(30000, verts.min(0) - 1, verts.max(0) + 1, 21)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)
    _check_batches(agg, tree, prims, verts, _four(rays, rays[::-1].copy()))
    agg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False])
def test_gpu_kd_scheduling_never_shows(lean):
    """Permuting the rays inside a batch, reordering the batches and splitting one batch into two give every ray the
    same record."""
    verts, prims = ss.grid_mesh(48, 5) if lean else ss.random_soup(4000, 500, 31)
    tree = build_kd_tree(prims, verts, max_prims=2)
    rays = np.concatenate([scene.random_rays(30000, verts.min(0) - 1, verts.max(0) + 1, 32),
                           ss.edge_case_rays(verts, prims, 33)])
    srays = scene.random_rays(9000, verts.min(0), verts.max(0), 34, tmax=0.7)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)

    def run(spec):
        b = Batches(spec)
        agg.trace_batches_device(b.tuples(), _stream())
        return b.results()

    base = run([("closest", rays), ("any", srays)])
    perm, sperm = np.random.default_rng(1).permutation(len(rays)), np.random.default_rng(2).permutation(len(srays))
    got = run([("closest", rays[perm]), ("any", srays[sperm])])
    assert got[0].tobytes() == base[0][perm].tobytes()
    for g, e in zip(got[1], base[1]):
        assert np.array_equal(g, e[sperm])
    got = run([("any", srays), ("closest", rays)])
    assert got[1].tobytes() == base[0].tobytes()
    for g, e in zip(got[0], base[1]):
        assert np.array_equal(g, e)
    cut, scut = 12345, 4000
    got = run([("closest", rays[:cut]), ("closest", rays[cut:]), ("any", srays[:scut]), ("any", srays[scut:])])
    assert got[0].tobytes() + got[1].tobytes() == base[0].tobytes()
    for k in range(3):
        assert np.array_equal(np.concatenate([got[2][k], got[3][k]]), base[1][k])
    agg.close()


# ---- the queue calls --------------------------------------------------------------------------------------------
def _kd_setup(seed, n_rays, n_patches=400):
    from nn_bvh_amd.wavefront import WavefrontAggregate
    verts, prims = ss.random_soup(2500, n_patches, seed)
    tree = build_kd_tree(prims, verts, max_prims=2)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds)
    # the forms under test, whatever the library's measured defaults are: the pair in ONE launch, SOA queues of a lean
    # scene read by the kernel (the other forms: test_gpu_kd_device_size_above_the_bound_and_negative and the SOA test)
    agg.set_option("pair_one_launch", 1)
    agg.set_option("read_soa", 1)
    rays = scene.random_rays(n_rays, verts.min(0) - 3, verts.max(0) + 3, seed + 1)
    return verts, prims, tree, agg, rays, WavefrontAggregate


def _shadow_rays(verts, n, seed):
    srays = scene.random_rays(n, verts.min(0) - 3, verts.max(0) + 3, seed)
    srays["tmax"] = np.float32(1 - 1e-4)
    srays["d"] *= np.float32(12.0)
    return srays


def _record_shadow_numpy(occ, Ld, r_u, r_l, px, L):
    s = r_u + r_l
    avg = (((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]) / np.float32(4)
    exp = L.copy()
    vis = occ == 0
    exp[px[vis]] = L[px[vis]] + Ld[vis] / avg[vis, None]
    return exp


def _kd_closest(tree, prims, verts, rays):
    return ob.kd_closest(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)


def _kd_any(tree, prims, verts, rays):
    return ob.kd_any_hit(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("device_size", [None, 5000, 0])
def test_gpu_kd_intersect_closest_queues(device_size, lean):
    import torch
    from test_wavefront import rules_numpy
    from nn_bvh_amd.wavefront import RayQueue, WorkQueue
    max_rays = 7001
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(21, max_rays, 0 if lean else 400)
    n = max_rays if device_size is None else device_size
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 0, 0, 1, 2, 4, 5], np.uint8), len(prims))
    has_medium = (rng.random(max_rays) < 0.1).astype(np.uint8)
    dev = _dev()
    rq = RayQueue.from_records(rays, dev)
    rq.has_medium = torch.from_numpy(has_medium).to(dev)
    if device_size is not None:
        rq.size.fill_(device_size)
    wf = WavefrontAggregate(agg, prim_class)
    queues = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    hits_t = torch.full((max_rays, 32), 0xAB, dtype=torch.uint8, device=dev)
    wf.IntersectClosest(max_rays, rq, hits=hits_t, **queues)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    # the queue carries no tmax (Infinity) and no time (0)
    qrays = rays[:n].copy()
    qrays["tmax"], qrays["time"] = np.inf, 0
    exp = _kd_closest(tree, prims, verts, qrays)
    assert hits[:n].tobytes() == exp.tobytes()
    assert (hits_t[n:].cpu().numpy() == 0xAB).all(), "records beyond the queue size were written"
    expq = rules_numpy(exp["prim"], has_medium[:n], prim_class)
    for k in QUEUES:
        assert queues[k].Size() == len(expq[k]), k
        assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), expq[k]), k
    if n:
        assert len(expq["escaped"]) and len(expq["next_ray"]) and len(expq["hit_area_light"])
    agg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("device_size", ["above", "negative"])
def test_gpu_kd_device_size_above_the_bound_and_negative(device_size, lean):
    """The batch holds min(max_rays, max(*d_size, 0)) rays: a device size above the bound gives the max_rays results and
    touches nothing beyond max_rays, a negative one gives the results of size 0 — for the two single calls and the pair
    call, on a lean scene (the kernel reads the SOA slices) and on one with patches (gather + records).  Every buffer
    holds 2000 more entries than max_rays and the size stays inside them, so a missing clamp shows in the sentinels."""
    import torch
    from test_wavefront import rules_numpy, shadow_inputs
    from nn_bvh_amd.wavefront import RayQueue, WorkQueue
    max_rays, max_shadow, extra, n_pixels = 6001, 5003, 2000, 9000
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(91, max_rays + extra, 0 if lean else 400)
    srays = _shadow_rays(verts, max_shadow + extra, 92)
    size_c = max_rays + 777 if device_size == "above" else -5
    size_s = max_shadow + 1234 if device_size == "above" else -(1 << 31)
    nc, ns = (max_rays, max_shadow) if device_size == "above" else (0, 0)
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 0, 0, 1, 2, 4, 5], np.uint8), len(prims))
    has_medium = (rng.random(max_rays + extra) < 0.1).astype(np.uint8)
    Ld, r_u, r_l, px, L = shadow_inputs(max_shadow + extra, n_pixels, 7)
    dev = _dev()
    rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(srays, dev, shadow=True)
    rq.has_medium = torch.from_numpy(has_medium).to(dev)
    rq.size.fill_(size_c)
    sq.size.fill_(size_s)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    wf = WavefrontAggregate(agg, prim_class)
    qrays = rays[:nc].copy()
    qrays["tmax"] = np.inf
    exp = _kd_closest(tree, prims, verts, qrays) if nc else np.zeros(0, HIT_DTYPE)
    expq = rules_numpy(exp["prim"], has_medium[:nc], prim_class)
    eocc = _kd_any(tree, prims, verts, srays[:ns]) if ns else np.zeros(0, np.uint8)
    expL = _record_shadow_numpy(eocc, Ld[:ns], r_u[:ns], r_l[:ns], px[:ns], L)

    def check_closest(hits_t, queues, what):
        hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
        assert hits[:nc].tobytes() == exp.tobytes(), what
        assert (hits_t[nc:].cpu().numpy() == 0xAB).all(), what + ": hit records beyond the batch were written"
        for k in QUEUES:
            assert queues[k].Size() == len(expq[k]), (what, k)
            assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), expq[k]), (what, k)
            assert (queues[k].items[len(expq[k]):].cpu().numpy() == -7).all(), (what, k)

    def check_shadow(occ_t, L_t, what):
        assert np.array_equal(occ_t.cpu().numpy()[:ns], eocc), what
        assert (occ_t.cpu().numpy()[ns:] == 9).all(), what + ": occlusion flags beyond the batch were written"
        assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32)), what

    def outputs():
        queues = {k: WorkQueue(max_rays + extra, dev) for k in QUEUES}
        for q in queues.values():
            q.items.fill_(-7)
        return (queues, torch.full((max_rays + extra, 32), 0xAB, dtype=torch.uint8, device=dev), t(L),
                torch.full((max_shadow + extra,), 9, dtype=torch.uint8, device=dev))

    queues, hits_t, L_t, occ_t = outputs()
    wf.IntersectClosest(max_rays, rq, hits=hits_t, **queues)
    wf.IntersectShadow(max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, occluded=occ_t)
    torch.cuda.synchronize()
    check_closest(hits_t, queues, "IntersectClosest")
    check_shadow(occ_t, L_t, "IntersectShadow")
    for one_launch in (1, 0):
        agg.set_option("pair_one_launch", one_launch)
        queues, hits_t, L_t, occ_t = outputs()
        wf.IntersectClosestAndShadow(max_rays, rq, max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, hits=hits_t,
                                     occluded=occ_t, **queues)
        torch.cuda.synchronize()
        check_closest(hits_t, queues, f"IntersectClosestAndShadow (one launch {one_launch})")
        check_shadow(occ_t, L_t, f"IntersectClosestAndShadow (one launch {one_launch})")
    if lean:  # ... and the lean scene's queues gathered into records
        agg.set_option("read_soa", 0)
        queues, hits_t, L_t, occ_t = outputs()
        wf.IntersectClosest(max_rays, rq, hits=hits_t, **queues)
        wf.IntersectShadow(max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, occluded=occ_t)
        torch.cuda.synchronize()
        check_closest(hits_t, queues, "IntersectClosest (gathered)")
        check_shadow(occ_t, L_t, "IntersectShadow (gathered)")
    if nc:
        assert len(expq["escaped"]) and len(expq["next_ray"]) and 0.1 < eocc.mean() < 0.9
    agg.close()


@pytest.mark.gpu
def test_gpu_kd_soa_form_equals_gathered_records():
    """A lean scene reads the queue's SOA slices itself; the same rays as nnbvh_ray records through
    nnbvh_kd_trace_batches_device give identical outputs, with time / tmax NULL and non-NULL."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue
    n = 20000
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(81, n, 0)
    rays["time"] = np.random.default_rng(3).random(n).astype(np.float32)
    rays["tmax"] = np.where(np.arange(n) % 3 == 0, np.float32(4.0), np.float32(np.inf))
    dev = _dev()
    wf = WavefrontAggregate(agg)
    for with_optional in (False, True):
        rq = RayQueue.from_records(rays, dev, shadow=with_optional)
        if with_optional:
            rq.time = torch.from_numpy(np.ascontiguousarray(rays["time"])).to(dev)
        rec = rays.copy()
        if not with_optional:
            rec["tmax"], rec["time"] = np.inf, 0
        hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        wf.IntersectClosest(n, rq, hits=hits_t)
        b = Batches([("closest", rec), ("any", rec)])
        agg.trace_batches_device(b.tuples(), _stream())
        got = b.results()
        assert hits_t.cpu().numpy().tobytes() == got[0].tobytes()
        agg.set_option("read_soa", 0)  # the same queue gathered into records by the library
        hits_g = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        wf.IntersectClosest(n, rq, hits=hits_g)
        agg.set_option("read_soa", 1)
        torch.cuda.synchronize()
        assert torch.equal(hits_g, hits_t)
        if with_optional:
            f = lambda m: torch.zeros((m, 4), dtype=torch.float32, device=dev)  # noqa: E731
            occ_t = torch.zeros(n, dtype=torch.uint8, device=dev)
            wf.IntersectShadow(n, rq, f(n), f(n) + 1, f(n) + 1, torch.arange(n, dtype=torch.int32, device=dev), f(n),
                               occluded=occ_t)
            torch.cuda.synchronize()
            assert np.array_equal(occ_t.cpu().numpy(), got[1][0])
    agg.close()


@pytest.mark.gpu
def test_gpu_kd_queue_overflow_and_unwanted_queues():
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WorkQueue
    n = 4096
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(31, n)
    dev = _dev()
    wf = WavefrontAggregate(agg)
    small = WorkQueue(100, dev)
    small.items.fill_(-7)
    esc = WorkQueue(n, dev)
    wf.IntersectClosest(n, RayQueue.from_records(rays, dev), escaped=esc, basic_eval_material=small)
    torch.cuda.synchronize()
    qrays = rays.copy()
    qrays["tmax"] = np.inf
    exp = _kd_closest(tree, prims, verts, qrays)
    hit_idx = np.nonzero(exp["prim"] >= 0)[0]
    assert len(hit_idx) > 100
    assert small.Size() == len(hit_idx)
    stored = small.items.cpu().numpy()
    assert len(stored) == 100 and np.isin(stored, hit_idx).all() and len(np.unique(stored)) == 100
    assert np.array_equal(np.sort(esc.indices().cpu().numpy()), np.nonzero(exp["prim"] < 0)[0])
    agg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_size", [None, 3000])
def test_gpu_kd_intersect_shadow_records_radiance(device_size):
    import torch
    from test_wavefront import shadow_inputs
    from nn_bvh_amd.wavefront import RayQueue
    max_rays, n_pixels = 6000, 9000
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(41, max_rays)
    rays = _shadow_rays(verts, max_rays, 42)
    n = max_rays if device_size is None else device_size
    Ld, r_u, r_l, px, L = shadow_inputs(max_rays, n_pixels, 7)
    dev = _dev()
    sq = RayQueue.from_records(rays, dev, shadow=True)
    if device_size is not None:
        sq.size.fill_(device_size)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    L_t, occ_t = t(L), torch.full((max_rays,), 9, dtype=torch.uint8, device=dev)
    wf = WavefrontAggregate(agg)
    wf.IntersectShadow(max_rays, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, occluded=occ_t)
    torch.cuda.synchronize()
    srec = rays[:n].copy()
    srec["time"] = 0
    eocc = _kd_any(tree, prims, verts, srec)
    assert 0.1 < eocc.mean() < 0.9
    assert np.array_equal(occ_t.cpu().numpy()[:n], eocc)
    assert (occ_t.cpu().numpy()[n:] == 9).all()
    exp = _record_shadow_numpy(eocc, Ld[:n], r_u[:n], r_l[:n], px[:n], L)
    assert np.array_equal(L_t.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    L2 = t(L)
    wf.IntersectShadow(max_rays, sq, t(Ld), t(r_u), t(r_l), t(px), L2)
    torch.cuda.synchronize()
    assert np.array_equal(L2.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    agg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [True, False])
@pytest.mark.parametrize("sizes", [(None, None), (5000, 3000), (0, 4000), (7001, 0)])
def test_gpu_kd_closest_and_shadow_in_one_launch(sizes, lean):
    """The pair call gives the hits, queues, flags and L of the oracle and of the two separate calls, and writes nothing
    beyond the queue sizes."""
    import torch
    from test_wavefront import rules_numpy, shadow_inputs
    from nn_bvh_amd.wavefront import RayQueue, WorkQueue
    max_rays, max_shadow, n_pixels = 7001, 6000, 9000
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(51, max_rays, 0 if lean else 400)
    srays = _shadow_rays(verts, max_shadow, 77)
    nc = max_rays if sizes[0] is None else sizes[0]
    ns = max_shadow if sizes[1] is None else sizes[1]
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 0, 0, 1, 2, 4, 5], np.uint8), len(prims))
    has_medium = (rng.random(max_rays) < 0.1).astype(np.uint8)
    Ld, r_u, r_l, px, L = shadow_inputs(max_shadow, n_pixels, 7)
    dev = _dev()
    rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(srays, dev, shadow=True)
    rq.has_medium = torch.from_numpy(has_medium).to(dev)
    if sizes[0] is not None:
        rq.size.fill_(sizes[0])
    if sizes[1] is not None:
        sq.size.fill_(sizes[1])
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    wf = WavefrontAggregate(agg, prim_class)
    queues = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    hits_t = torch.full((max_rays, 32), 0xAB, dtype=torch.uint8, device=dev)
    L_t, occ_t = t(L), torch.full((max_shadow,), 9, dtype=torch.uint8, device=dev)
    wf.IntersectClosestAndShadow(max_rays, rq, max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, hits=hits_t,
                                 occluded=occ_t, **queues)
    torch.cuda.synchronize()
    hits = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
    qrays = rays[:nc].copy()
    qrays["tmax"] = np.inf
    exp = _kd_closest(tree, prims, verts, qrays)
    assert hits[:nc].tobytes() == exp.tobytes()
    assert (hits_t[nc:].cpu().numpy() == 0xAB).all(), "hit records beyond the queue size were written"
    expq = rules_numpy(exp["prim"], has_medium[:nc], prim_class)
    for k in QUEUES:
        assert queues[k].Size() == len(expq[k]), k
        assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), expq[k]), k
    eocc = _kd_any(tree, prims, verts, srays[:ns])
    assert np.array_equal(occ_t.cpu().numpy()[:ns], eocc)
    assert (occ_t.cpu().numpy()[ns:] == 9).all(), "occlusion flags beyond the queue size were written"
    expL = _record_shadow_numpy(eocc, Ld[:ns], r_u[:ns], r_l[:ns], px[:ns], L)
    assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32))
    # ... and the two calls
    queues2 = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    hits2 = torch.full((max_rays, 32), 0xAB, dtype=torch.uint8, device=dev)
    L2, occ2 = t(L), torch.full((max_shadow,), 9, dtype=torch.uint8, device=dev)
    wf.IntersectShadow(max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L2, occluded=occ2)
    wf.IntersectClosest(max_rays, rq, hits=hits2, **queues2)
    torch.cuda.synchronize()
    assert torch.equal(hits2, hits_t) and torch.equal(occ2, occ_t) and torch.equal(L2, L_t)
    for k in QUEUES:
        assert queues2[k].Size() == queues[k].Size(), k
        assert np.array_equal(np.sort(queues2[k].indices().cpu().numpy()), np.sort(queues[k].indices().cpu().numpy())), k
    agg.close()


def _items_by_index(queue, slices):
    """field -> values ordered by the pushed item index (the push order itself is the scheduler's)."""
    idx = queue.indices().cpu().numpy()
    order = np.argsort(idx, kind="stable")
    out = {"index": idx[order]}
    for name, t in slices.fields.items():
        a = t.cpu().numpy()
        out[name] = (a[:len(idx)] if a.ndim == 1 else a[:, :len(idx)])[..., order]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("pair", [False, True])
def test_gpu_kd_items_equal_the_scene_free_enqueue_on_the_flat_hits(pair):
    import torch
    from test_wavefront import shadow_inputs
    from test_wavefront_items import full_items, ray_queue, soup_setup
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue, enqueue_closest_items
    n, max_shadow, n_pixels = 8000, 5000, 7000
    verts, prims, mesh, bvh, rays = soup_setup(61, n, host_prims=12)
    bvh.close()
    rng = np.random.default_rng(2)
    lo = rng.uniform(-8, 8, (len(prims), 3)).astype(np.float32)
    pb = np.concatenate([lo, lo + rng.uniform(0.5, 2, (len(prims), 3)).astype(np.float32)], 1)
    tri = prims["kind"] == 0
    from nn_bvh_amd.kdtree import prim_bounds_of
    tlo, thi = prim_bounds_of(prims[tri], verts)
    pb[tri] = np.concatenate([tlo, thi], 1)
    kd = KdTreeAggregate.build(prims, verts, prim_bounds=pb)
    kd.set_option("pair_one_launch", 1)
    dev = _dev()
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(prims))
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    rq = ray_queue(rays, dev, has_medium)
    wf = WavefrontAggregate(kd, prim_class)
    queues = {k: WorkQueue(n, dev) for k in QUEUES}
    items, nh = full_items(n, dev), WorkQueue(n, dev)
    hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
    if pair:
        srays = _shadow_rays(verts, max_shadow, 9)
        Ld, r_u, r_l, px, L = shadow_inputs(max_shadow, n_pixels, 7)
        t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        sq = RayQueue.from_records(srays, dev, shadow=True)
        L_t, occ_t = t(L), torch.zeros(max_shadow, dtype=torch.uint8, device=dev)
        wf.IntersectClosestAndShadowItems(n, rq, mesh, max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, items=items,
                                          needs_host=nh, hits=hits_t, occluded=occ_t, **queues)
        torch.cuda.synchronize()
        srec = srays.copy()
        srec["time"] = 0
        flat_occ = _flat(kd, "any", srec)[0]
        assert np.array_equal(occ_t.cpu().numpy(), flat_occ) and (flat_occ == 2).any()
        expL = _record_shadow_numpy(flat_occ, Ld, r_u, r_l, px, L)
        assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32))
    else:
        wf.IntersectClosestItems(n, rq, mesh, items=items, needs_host=nh, hits=hits_t, **queues)
    torch.cuda.synchronize()
    qrays = rays.copy()
    qrays["tmax"] = np.inf
    flat = _flat(kd, "closest", qrays)
    assert hits_t.cpu().numpy().tobytes() == flat.tobytes(), "kd queue call and flat call disagree"
    assert (flat["prim"] >= 0).sum() > 500 and (flat["instance"] == -1).any()
    # the kd hit's prim is the caller's primitive id: the scene-free enqueue on the flat hits gives the same items
    queues2 = {k: WorkQueue(n, dev) for k in QUEUES}
    items2, nh2 = full_items(n, dev), WorkQueue(n, dev)
    enqueue_closest_items(mesh, n, rq, _to_dev(flat).reshape(n, 32), prim_class=wf.prim_class, items=items2,
                          needs_host=nh2, **queues2)
    torch.cuda.synchronize()
    assert np.array_equal(np.sort(nh.indices().cpu().numpy()), np.sort(nh2.indices().cpu().numpy())) and nh.Size() > 0
    for k in QUEUES:
        assert queues[k].Size() == queues2[k].Size(), k
        if k in items:
            a, b = _items_by_index(queues[k], items[k]), _items_by_index(queues2[k], items2[k])
            assert np.array_equal(a["index"], b["index"]), k
            # a medium_sample item of a ray that hit nothing (or was voided) carries no surface: those rows stay unwritten
            surf = (flat["prim"][a["index"]] >= 0) & (flat["instance"][a["index"]] != -1)
            assert surf.sum() > 20, k
            for f in a:
                assert a[f][..., surf].tobytes() == b[f][..., surf].tobytes(), (k, f)
        else:
            assert np.array_equal(np.sort(queues[k].indices().cpu().numpy()), np.sort(queues2[k].indices().cpu().numpy()))
    kd.close()
    mesh.close()


@pytest.mark.gpu
def test_gpu_kd_wavefront_iteration_is_hip_graph_capturable():
    """One kd wavefront iteration — queue resets, IntersectClosest, then the shadow queue and the next ray queue in one
    launch — captured in a hipGraph on one stream and replayed to the same outputs."""
    import torch
    from test_wavefront import shadow_inputs
    from nn_bvh_amd.wavefront import RayQueue, WorkQueue
    max_rays, max_shadow, n_pixels = 6000, 5000, 8000
    verts, prims, tree, agg, rays, WavefrontAggregate = _kd_setup(61, max_rays, 0)
    srays = _shadow_rays(verts, max_shadow, 78)
    Ld, r_u, r_l, px, L = shadow_inputs(max_shadow, n_pixels, 9)
    dev = _dev()
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(srays, dev, shadow=True)
    rq2 = RayQueue.from_records(rays[::-1].copy(), dev)
    wf = WavefrontAggregate(agg)
    queues = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    queues2 = {k: WorkQueue(max_rays, dev) for k in QUEUES}
    first_t = torch.zeros((max_rays, 32), dtype=torch.uint8, device=dev)
    hits_t = torch.zeros((max_rays, 32), dtype=torch.uint8, device=dev)
    Ld_t, ru_t, rl_t, px_t, L_t = t(Ld), t(r_u), t(r_l), t(px), t(L)
    L0 = L_t.clone()
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()

    def iteration():
        for q in list(queues.values()) + list(queues2.values()):
            q.Reset()
        wf.IntersectClosest(max_rays, rq2, hits=first_t, **queues2)
        wf.IntersectClosestAndShadow(max_rays, rq, max_shadow, sq, Ld_t, ru_t, rl_t, px_t, L_t, hits=hits_t, **queues)

    with torch.cuda.stream(side):
        iteration()  # warm-up: creates this stream's workspace (allocation is not capturable)
    torch.cuda.synchronize()
    eager = (first_t.clone(), hits_t.clone(), L_t.clone())
    eager_sizes = {k: (queues[k].Size(), queues2[k].Size()) for k in QUEUES}
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        iteration()
    for _ in range(2):
        first_t.zero_()
        hits_t.zero_()
        L_t.copy_(L0)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(first_t, eager[0]) and torch.equal(hits_t, eager[1]) and torch.equal(L_t, eager[2])
        assert {k: (queues[k].Size(), queues2[k].Size()) for k in QUEUES} == eager_sizes
    qrays = rays.copy()
    qrays["tmax"] = np.inf
    exp = _kd_closest(tree, prims, verts, qrays)
    assert hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1).tobytes() == exp.tobytes()
    agg.close()


@pytest.mark.gpu
def test_gpu_kd_and_bvh_wavefront_aggregates_agree():
    """The same triangles through the BVH WavefrontAggregate and the kd one: the same escaped set and the same t per
    hit ray; a ray may be left out only where prim differs at equal t, which the CPU test above shows to be no ray."""
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    verts, prims, rays = _cross_scene()
    n = len(rays)
    dev = _dev()
    bt = build_tree(prims, verts)
    bvh = BVHAggregate.from_tree(bt.nodes, bt.ordered_prims, verts)
    kd = KdTreeAggregate.build(prims, verts, where="gpu")
    out = {}
    for name, agg in (("bvh", bvh), ("kd", kd)):
        wf = WavefrontAggregate(agg)
        esc = WorkQueue(n, dev)
        hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        wf.IntersectClosest(n, RayQueue.from_records(rays, dev), escaped=esc, hits=hits_t)
        torch.cuda.synchronize()
        out[name] = (np.sort(esc.indices().cpu().numpy()), hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1))
        agg.close()
    hb, hk = out["bvh"][1], out["kd"][1]
    left_out = (hb["prim"] != hk["prim"]) & (hb["t"].view(np.uint32) == hk["t"].view(np.uint32))
    assert left_out.sum() == 0
    assert np.array_equal(out["bvh"][0], out["kd"][0]) and len(out["kd"][0]) > 100
    assert np.array_equal(hb["t"].view(np.uint32), hk["t"].view(np.uint32))
    assert np.array_equal(hb["prim"], hk["prim"])
