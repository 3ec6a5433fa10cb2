"""kd-tree scenes created entirely on the device (nnbvh_kd_scene_create_gpu_build[_with_attributes],
KdTreeAggregate.build_on_device) and the read side of a kd scene (nnbvh_kd_scene_bounds / _info / _read).

The contract: the scene is the one nnbvh_kd_build_create_stable + nnbvh_kd_scene_create_with_attributes make from the
same arguments — the four device arrays byte for byte, bounds (the sign of a zero included), depth, flags, and every
result traced through it.  CPU: exports, prototypes and what is refused before any device work.  GPU: every decision
path of the builder (test_kd_build_gpu.PATH_CASES), the sign of zero in the union, the degenerate flag, every
primitive kind with and without its attribute arrays, tiny inputs, bad primitive lists, the caller's device, and a
wavefront iteration."""
import ctypes
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, PRIM_DTYPE, NNBVHError, _lib, scene
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree
from test_kd_build_gpu import PATH_CASES, TRACED, host_tree, path_scene

NEW_CALLS = ("nnbvh_kd_scene_create_gpu_build", "nnbvh_kd_scene_create_gpu_build_with_attributes",
             "nnbvh_kd_scene_bounds", "nnbvh_kd_scene_info", "nnbvh_kd_scene_read")
ERR_ARG = 1
K_DEGENERATE, K_HOST = 4, 16  # kPrimDegenerate, kPrimHost (csrc/nnbvh_internal.h)


# ---------------------------------------------------------------------------------------------- CPU
def test_device_scene_entry_points_are_exported_with_prototypes():
    L = _lib.lib()
    header = open(_lib.LIB_PATH.rsplit("nn_bvh_amd", 1)[0] + "include/nnbvh.h").read()
    for name in NEW_CALLS:
        assert name in _lib.EXPORTS, name
        fn = getattr(L, name)
        assert fn.argtypes is not None, name
        assert fn.restype is (ctypes.c_void_p if "create" in name else ctypes.c_int), name
        assert name + "(" in header, name
    assert len(L.nnbvh_kd_scene_create_gpu_build.argtypes) == 11
    assert len(L.nnbvh_kd_scene_create_gpu_build_with_attributes.argtypes) == 14


def _create(prims, n_prims, verts, n_verts, max_depth=-1, device=0):
    p = _lib.ptr
    return _lib.lib().nnbvh_kd_scene_create_gpu_build(
        None if prims is None else p(prims), n_prims, None if verts is None else p(verts), n_verts, None, 5, 1,
        ctypes.c_float(0.5), 1, max_depth, device)


def test_device_scene_calls_refuse_bad_arguments_before_any_device_work():
    """NULL or empty arrays, max_depth 65 and a negative device: NULL plus a message, whatever the machine holds."""
    L = _lib.lib()
    verts, prims, _ = path_scene("soup7")
    prims, verts = np.ascontiguousarray(prims), np.ascontiguousarray(verts)
    for args in ((None, 7, verts, 21), (prims, 7, None, 21), (prims, 0, verts, 21), (prims, 7, verts, 0),
                 (prims, -1, verts, 21)):
        assert _create(*args) is None, args[1::2]
        assert "empty primitive or vertex array" in _lib.last_error()
    assert _create(prims, 7, verts, 21, max_depth=65) is None
    assert "max_depth above the traversal stack" in _lib.last_error()
    assert _create(prims, 7, verts, 21, max_depth=64, device=-1) is None
    assert "no usable HIP device" in _lib.last_error()
    with pytest.raises(NNBVHError, match="max_depth above the traversal stack"):
        KdTreeAggregate.build_on_device(prims, verts, max_depth=65)
    with pytest.raises(NNBVHError, match="no usable HIP device"):
        KdTreeAggregate.build_on_device(prims, verts, device=-1)
    with pytest.raises(NNBVHError, match="empty primitive or vertex array"):
        KdTreeAggregate.build_on_device(prims[:0], verts)
    # NULL scenes
    out = np.zeros(8, np.int64)
    assert L.nnbvh_kd_scene_bounds(None, _lib.ptr(out)) == ERR_ARG and "nnbvh_kd_scene_bounds" in _lib.last_error()
    assert L.nnbvh_kd_scene_info(None, _lib.ptr(out)) == ERR_ARG and "nnbvh_kd_scene_info" in _lib.last_error()
    assert L.nnbvh_kd_scene_read(None, 0, _lib.ptr(out), 64) == ERR_ARG and "nnbvh_kd_scene_read" in _lib.last_error()


def test_build_on_device_without_a_usable_device_raises():
    """No CPU fallback: on a machine without a GPU device 0 is not there; with GPUs the first number past them is not."""
    verts, prims, _ = path_scene("soup7")
    with pytest.raises(NNBVHError, match="no usable HIP device"):
        KdTreeAggregate.build_on_device(prims, verts, device=max(_lib.lib().nnbvh_device_count(), 0))


# ---------------------------------------------------------------------------------------------- GPU
def _host_route(prims, verts, pb=None, tree=None, **kw):
    """The reference scene: the stable host builder's tree through from_tree."""
    attrs = {k: kw.pop(k) for k in ("normals", "uvs", "prim_alpha") if k in kw}
    t = tree if tree is not None else build_kd_tree(prims, verts, prim_bounds=pb, where="host_stable", **kw)
    return t, KdTreeAggregate.from_tree(t.nodes, t.prim_indices, prims, verts, t.bounds, **attrs)


def _assert_same_scene(dev, host, what, arrays=(0, 1, 2, 3)):
    assert dev.info() == host.info(), f"{what}: info {dev.info()} against {host.info()}"
    for k in arrays:
        d, h = dev.read(k), host.read(k)
        assert d.shape == h.shape and d.tobytes() == h.tobytes(), f"{what}: device array {k} differs"
    assert np.concatenate(dev.Bounds()).tobytes() == np.concatenate(host.Bounds()).tobytes(), \
        f"{what}: bounds {dev.Bounds()} against {host.Bounds()}"


def _rays(verts, prims):
    lo, hi = verts.min(0), verts.max(0)
    pad = 0.1 * (hi - lo) + 1
    return np.concatenate([scene.random_rays(3000, lo - pad, hi + pad, 51), scene.random_rays(1000, lo, hi, 52, tmax=0.5),
                           ss.edge_case_rays(verts, prims, 53, n=1024)])


def _assert_traces_like_the_oracle(dev, tree, prims, verts, what):
    rays = _rays(verts, prims)
    got = dev.Intersect(rays)
    occ, vis, tst = dev.IntersectP(rays, counts=True)
    exp = ob.kd_closest(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)
    eo, ev, et = ob.kd_any_hit(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays, 4)
    assert got.tobytes() == exp.tobytes(), f"{what}: closest-hit records differ from the oracle on the host-built tree"
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et), f"{what}: any-hit differs"


@pytest.mark.gpu
@pytest.mark.parametrize("family,name,kw,premise", PATH_CASES)
def test_device_scene_equals_the_host_route_on_every_builder_path(family, name, kw, premise):
    verts, prims, pb = path_scene(name)
    what = f"{name} {kw}"
    tree, host = _host_route(prims, verts, tree=host_tree(name, tuple(sorted(kw.items()))))
    dev = KdTreeAggregate.build_on_device(prims, verts, prim_bounds=pb, **kw)
    dev2 = KdTreeAggregate.build_on_device(prims, verts, prim_bounds=pb, **kw)
    try:
        _assert_same_scene(dev, host, what, arrays=(0, 1, 2))
        assert dev.info()["depth"] == tree.depth and dev.info()["n_nodes"] == len(tree.nodes)
        assert dev.read(0).tobytes() == tree.nodes.tobytes() and dev.read(1).tobytes() == tree.prim_indices.tobytes()
        assert np.concatenate(dev.Bounds()).tobytes() == tree.bounds.tobytes()
        _assert_same_scene(dev2, dev, what + " (two device creations)", arrays=(0, 1, 2))
        if family in TRACED:
            _assert_traces_like_the_oracle(dev, tree, prims, verts, what)
    finally:
        for a in (dev, dev2, host):
            a.close()


def _zero_boxes(first, second):
    """16 primitives = 8 boxes as triangle pairs, in x > 0 and y < 0 apart from four edges at zero: the minimum on x
    is reached by primitives 2 and 5 (lo.x = `first`, `second`), the maximum on y by primitives 3 and 6 (hi.y)."""
    lo = np.zeros((16, 3), np.float32)
    hi = np.zeros((16, 3), np.float32)
    for i in range(16):
        b = i // 2
        lo[i] = (1 + b, -9 + b * 0.5, b - 4)
        hi[i] = (2.5 + b, -8.25 + b * 0.5, b - 2.5)
    lo[2, 0], lo[5, 0] = first, second
    hi[3, 1], hi[6, 1] = first, second
    return ss.box_tris(lo, hi)


@pytest.mark.gpu
@pytest.mark.parametrize("first,second", [(0.0, -0.0), (-0.0, 0.0)], ids=["plus_first", "minus_first"])
def test_device_scene_bounds_keep_the_sign_of_zero_of_the_first_primitive(first, second):
    """The host's sequential union keeps the first of equals: the zero of the LOWEST-indexed primitive that reaches
    the extreme.  A float min / max over ordered bits would always answer -0 for a minimum and +0 for a maximum."""
    verts, prims = _zero_boxes(np.float32(first), np.float32(second))
    _, host = _host_route(prims, verts)
    dev = KdTreeAggregate.build_on_device(prims, verts)
    try:
        lo, hi = dev.Bounds()
        assert lo[0] == 0 and hi[1] == 0
        assert np.signbit(lo[0]) == np.signbit(np.float32(first)), f"min x: {lo[0]!r}, expected the zero of primitive 2"
        assert np.signbit(hi[1]) == np.signbit(np.float32(first)), f"max y: {hi[1]!r}, expected the zero of primitive 3"
        _assert_same_scene(dev, host, f"zeros {first} {second}", arrays=(0, 1, 2))
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_device_scene_on_signed_zero_edges(max_prims):
    verts, prims, _ = path_scene("signed_zeros")
    tree, host = _host_route(prims, verts, max_prims=max_prims)
    dev = KdTreeAggregate.build_on_device(prims, verts, max_prims=max_prims)
    try:
        _assert_same_scene(dev, host, "signed_zeros", arrays=(0, 1, 2))
        _assert_traces_like_the_oracle(dev, tree, prims, verts, "signed_zeros")
    finally:
        dev.close()
        host.close()


def _degenerate_triangles():
    """64 triangles: 8 with a repeated vertex, 8 collinear, 24 slivers (one edge of 0.5 .. 3, the other of 1e-18 ..
    1e-24 along another axis, from the origin: the cross product is their product, its square underflows to 0 below
    about 1e-22.5), 24 ordinary ones.  Returns (verts, prims, the slivers' indices)."""
    rng = np.random.default_rng(61)
    tris = []
    for i in range(8):
        a, b = rng.uniform(-3, 3, (2, 3))
        tris.append([(a, a, b), (a, b, a), (a, b, b), (a, a, a)][i % 4])
    for i in range(8):
        a, d = rng.uniform(-3, 3, 3), np.eye(3)[i % 3] * (1 + i)
        tris.append((a, a + d, a + 2 * d) if i < 4 else (a + d, a, a + 2 * d))
    slivers = range(len(tris), len(tris) + 24)
    for i in range(24):
        e = np.float32(10.0) ** np.float32(-18 - 6 * i / 23)
        long_axis, short_axis = i % 3, (i + 1 + i // 12) % 3
        p1, p2 = np.zeros(3), np.zeros(3)
        p1[long_axis] = (0.5, 1.0, 2.0, 3.0)[i % 4]
        p2[short_axis if short_axis != long_axis else (long_axis + 1) % 3] = e
        tris.append((np.zeros(3), p1, p2) if i % 2 else (np.zeros(3), p2, p1))
    v, p = ss.random_soup(24, 0, 62)
    verts = np.concatenate([np.asarray(tris, np.float32).reshape(-1, 3), v])
    prims = np.zeros(64, PRIM_DTYPE)
    prims["id"] = np.arange(64)
    prims["v"][:40, :3] = np.arange(120).reshape(40, 3)
    prims["v"][40:, :3] = p["v"][:, :3] + 120
    return verts, prims, np.array(slivers)


@pytest.mark.gpu
def test_device_scene_degenerate_flag_has_the_host_bits():
    verts, prims, slivers = _degenerate_triangles()
    _, host = _host_route(prims, verts)
    dev = KdTreeAggregate.build_on_device(prims, verts)
    try:
        flags = host.read(2).view(np.uint32)[:, 7]
        # the premise: among the slivers the squared cross product underflows for some and not for others
        assert 0 < ((flags[slivers] & K_DEGENERATE) != 0).sum() < len(slivers), flags[slivers]
        assert ((flags[:16] & K_DEGENERATE) != 0).all() and ((flags[40:] & K_DEGENERATE) == 0).all()
        _assert_same_scene(dev, host, "degenerate triangles", arrays=(0, 1, 2))
    finally:
        dev.close()
        host.close()


def _kind_scenes():
    """name -> (verts, prims, prim_bounds, attribute arrays); built once."""
    from test_alpha import alpha_patch_scene, alpha_scene, patch_uvs
    out = {}
    v, p = ss.random_soup(1500, 300, 6)
    out["soup+patches"] = (v, p, None, {})
    rng = np.random.default_rng(7)
    c = rng.uniform(-4, 4, (40, 3)).astype(np.float32)
    out["host_boxes"] = ss.host_boxes(c - 0.4, c + 0.4) + ({},)
    # host-only boxes among triangles: caller bounds for them, vertex bounds for the rest
    v, p = ss.random_soup(600, 60, 8)
    p = p.copy()
    pb = np.zeros((len(p), 6), np.float32)
    for i in range(0, len(p), 13):
        ctr = rng.uniform(-3, 3, 3).astype(np.float32)
        pb[i] = np.concatenate([ctr - 0.3, ctr + 0.3])
        p["kind"][i] = 3
    out["host_among_triangles"] = (v, p, pb, {})
    v, p, alpha, kinds = alpha_scene(6, 800)
    out["alpha_triangles"] = (v, p, None, {})
    v, p, normals, alpha, kinds = alpha_patch_scene(43, 500, 800)
    p = p.copy()
    smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(p)) < 0.5)
    p["kind"] = np.where(smooth, kinds + 2, kinds)
    assert set(range(4, 16)) <= set(p["kind"].tolist())
    full = dict(normals=normals, uvs=patch_uvs(v), prim_alpha=alpha)
    out["attributes_all"] = (v, p, None, full)
    for missing in ("normals", "uvs", "prim_alpha"):
        out["attributes_without_" + missing] = (v, p, None, {k: a for k, a in full.items() if k != missing})
    out["attributes_none"] = (v, p, None, {})
    return out


KIND_SCENES = ("soup+patches", "host_boxes", "host_among_triangles", "alpha_triangles", "attributes_all",
               "attributes_without_normals", "attributes_without_uvs", "attributes_without_prim_alpha",
               "attributes_none")
_kind_scenes = functools.lru_cache(maxsize=None)(_kind_scenes)


@pytest.mark.gpu
@pytest.mark.parametrize("name", KIND_SCENES)
def test_device_scene_every_primitive_kind_with_and_without_its_arrays(name):
    verts, prims, pb, attrs = _kind_scenes()[name]
    tree, host = _host_route(prims, verts, pb, max_prims=2, **attrs)
    dev = KdTreeAggregate.build_on_device(prims, verts, prim_bounds=pb, max_prims=2, **attrs)
    try:
        _assert_same_scene(dev, host, name)
        i = dev.info()
        kinds = prims["kind"]
        on_device = {"attributes_all": kinds >= 6, "attributes_without_normals": np.isin(kinds, (8, 9, 12, 13)),
                     "attributes_without_uvs": np.isin(kinds, (6, 7, 8, 9, 10, 11)),
                     "attributes_without_prim_alpha": np.isin(kinds, (6, 7))}.get(name)
        if on_device is not None:
            # a kind whose array is missing is host-only, in both routes (the records are equal: read from one)
            host_only = (dev.read(2).view(np.uint32)[:, 7] & K_HOST) != 0
            assert np.array_equal(host_only, (kinds >= 6) & ~on_device), name
            assert i["has_attribute_slots"] == 1 and dev.read(3).shape == (len(prims), 24) and dev.read(3).any()
        else:
            assert i["has_attribute_slots"] == 0 and dev.read(3).shape == (0, 24)
        rays = scene.random_rays(6000, verts.min(0) - 1, verts.max(0) + 1, 21)
        assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes(), name
        for d, h in zip(dev.IntersectP(rays, counts=True), host.IntersectP(rays, counts=True)):
            assert np.array_equal(d, h), name
        if i["has_host_prims"]:
            dh, dc = dev.intersect_with_host_candidates(rays)
            hh, hc = host.intersect_with_host_candidates(rays)
            assert dh.tobytes() == hh.tobytes() and all(np.array_equal(dc[k], hc[k]) for k in dc.dtype.names), name
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
def test_device_scene_of_one_primitive_is_a_root_leaf():
    verts, prims, _ = path_scene("soup1")
    _, host = _host_route(prims, verts)
    dev = KdTreeAggregate.build_on_device(prims, verts)
    try:
        i = dev.info()
        assert (i["n_nodes"], i["n_indices"], i["n_prims"], i["depth"]) == (1, 0, 1, 0)
        assert dev.read(1).shape == (0,) and int(dev.read(0)["flags"][0]) == (3 | 1 << 2)
        _assert_same_scene(dev, host, "one primitive", arrays=(0, 1, 2))
        rays = scene.random_rays(2000, verts.min(0) - 1, verts.max(0) + 1, 5)
        assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    finally:
        dev.close()
        host.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [7, 8])
def test_device_scene_of_seven_primitives_in_one_leaf(max_prims):
    verts, prims, _ = path_scene("soup7")
    _, host = _host_route(prims, verts, max_prims=max_prims)
    dev = KdTreeAggregate.build_on_device(prims, verts, max_prims=max_prims)
    try:
        assert (dev.info()["n_nodes"], dev.info()["n_indices"]) == (1, 7)
        _assert_same_scene(dev, host, f"seven primitives, max_prims {max_prims}", arrays=(0, 1, 2))
    finally:
        dev.close()
        host.close()


def _bad_lists():
    """name -> (verts, prims, the builders' message): the fault sits in the LAST of 3 000 primitives."""
    verts, prims = ss.random_soup(3000, 0, 5)
    out = {}
    for name, index in (("index_n_verts", len(verts)), ("index_minus_one", -1)):
        p = prims.copy()
        p["v"][-1, 2] = index
        out[name] = (verts, p, "vertex index out of range")
    v = verts.copy()
    v[prims["v"][-1, 0], 1] = np.nan
    out["nan_vertex"] = (v, prims, "non-finite vertex or primitive bounds")
    p = prims.copy()
    p["kind"][-1] = 99
    out["kind_99"] = (verts, p, "unsupported primitive kind")
    p = prims.copy()
    p["kind"][-1] = 3
    out["host_without_bounds"] = (verts, p, "host primitives need prim_bounds")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["index_n_verts", "index_minus_one", "nan_vertex", "kind_99", "host_without_bounds"])
def test_device_scene_refuses_a_bad_primitive_list_in_the_host_builders_words(name):
    """The device checks kind and vertex indices before it reads anything through them, and reports the lowest failing
    primitive's fault as kd_prepare words it; the library is as usable afterwards as before."""
    verts, prims, message = _bad_lists()[name]
    with pytest.raises(NNBVHError, match=message) as host_error:
        build_kd_tree(prims, verts, where="host_stable")
    with pytest.raises(NNBVHError, match=message) as dev_error:
        KdTreeAggregate.build_on_device(prims, verts)
    assert str(dev_error.value).split(": ", 1)[1] == str(host_error.value).split(": ", 1)[1]
    good_verts, good_prims = ss.random_soup(3000, 0, 5)
    tree = build_kd_tree(good_prims, good_verts, where="host_stable")
    dev = KdTreeAggregate.build_on_device(good_prims, good_verts)
    try:
        assert dev.read(0).tobytes() == tree.nodes.tobytes()
        _assert_traces_like_the_oracle(dev, tree, good_prims, good_verts, f"after {name}")
    finally:
        dev.close()


@pytest.mark.gpu
def test_device_routes_leave_the_callers_device_current():
    import torch
    verts, prims = ss.random_soup(500, 0, 3)
    before = torch.cuda.current_device()
    KdTreeAggregate.build_on_device(prims, verts).close()
    assert torch.cuda.current_device() == before
    build_kd_tree(prims, verts, where="gpu")
    assert torch.cuda.current_device() == before
    with pytest.raises(NNBVHError):  # ... on a failing call too
        bad = prims.copy()
        bad["kind"][0] = 99
        KdTreeAggregate.build_on_device(bad, verts)
    assert torch.cuda.current_device() == before
    if torch.cuda.device_count() < 2:
        return  # one device: nothing else to be current (the rest needs a second one)
    torch.cuda.set_device(0)
    tree = build_kd_tree(prims, verts, where="gpu", device=1)
    assert torch.cuda.current_device() == 0
    dev = KdTreeAggregate.build_on_device(prims, verts, device=1)
    assert torch.cuda.current_device() == 0
    assert dev.read(0).tobytes() == tree.nodes.tobytes()
    _assert_traces_like_the_oracle(dev, build_kd_tree(prims, verts, where="host_stable"), prims, verts, "device 1")
    assert torch.cuda.current_device() == 0
    dev.close()


@pytest.mark.gpu
def test_wavefront_queue_calls_on_a_device_created_scene():
    """One IntersectClosest + IntersectShadow of a WavefrontAggregate: queues, hit records, flags and radiance are
    those of the same calls on the host-route scene."""
    import torch
    from test_wavefront import shadow_inputs
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    max_rays, n_pixels = 5000, 7000
    verts, prims = ss.random_soup(2500, 400, 11)
    _, host = _host_route(prims, verts, max_prims=2)
    dev = KdTreeAggregate.build_on_device(prims, verts, max_prims=2)
    rays = scene.random_rays(max_rays, verts.min(0) - 3, verts.max(0) + 3, 12)
    srays = scene.random_rays(max_rays, verts.min(0) - 3, verts.max(0) + 3, 13)
    srays["tmax"] = np.float32(1 - 1e-4)
    srays["d"] *= np.float32(12.0)
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 0, 0, 1, 2, 4, 5], np.uint8), len(prims))
    has_medium = (rng.random(max_rays) < 0.1).astype(np.uint8)
    Ld, r_u, r_l, px, L = shadow_inputs(max_rays, n_pixels, 7)
    device = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    results = []
    for agg in (dev, host):
        rq, sq = RayQueue.from_records(rays, device), RayQueue.from_records(srays, device, shadow=True)
        rq.has_medium = t(has_medium)
        wf = WavefrontAggregate(agg, prim_class)
        queues = {k: WorkQueue(max_rays, device) for k in _lib.CLOSEST_QUEUES}
        hits = torch.full((max_rays, 32), 0xAB, dtype=torch.uint8, device=device)
        L_t, occ = t(L), torch.full((max_rays,), 9, dtype=torch.uint8, device=device)
        wf.IntersectClosest(max_rays, rq, hits=hits, **queues)
        wf.IntersectShadow(max_rays, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, occluded=occ)
        torch.cuda.synchronize()
        results.append((hits.cpu().numpy(), occ.cpu().numpy(), L_t.cpu().numpy(),
                        {k: np.sort(q.indices().cpu().numpy()) for k, q in queues.items()}))
    (dh, docc, dL, dq), (hh, hocc, hL, hq) = results
    assert dh.tobytes() == hh.tobytes() and np.array_equal(docc, hocc) and dL.tobytes() == hL.tobytes()
    for k in _lib.CLOSEST_QUEUES:
        assert np.array_equal(dq[k], hq[k]), k
    hit = dh.view(HIT_DTYPE).reshape(-1)["prim"] >= 0
    assert 0.1 < hit.mean() < 0.95 and 0.05 < (docc == 1).mean() < 0.95 and len(dq["escaped"]) and len(dq["next_ray"])
    dev.close()
    host.close()
