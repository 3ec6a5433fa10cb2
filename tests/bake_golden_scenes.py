"""The scenes of tests/golden/host_route_bake.npz, for tools/record_bake_golden.py (which wrote the fixture once, from
the commit that still baked host-built two-level and kd-tree scenes on the host) and tests/test_bake_golden.py (which
bakes them again through the same host-tree calls).  Every scene comes from a builder another test file already has;
none has more than about a thousand primitives.

scenes(): name -> a function that returns (family, aggregate, kinds), family "bvh" or "kd", kinds = the primitive
kinds in the order the scene bakes them (the ordered primitives of a BVH, the caller's order of a kd scene).
snapshot(family, aggregate): array name -> numpy array, "info" among them."""
import numpy as np

import scenes_small as ss
from nn_bvh_amd import BVHAggregate, _lib, build_tree

BVH_ARRAYS = {"records": 0, "stream": 1, "animation": 2}
KD_ARRAYS = {"nodes": 0, "indices": 1, "records": 2, "extras": 3}


def snapshot(family, agg):
    out = {}
    for name, what in (BVH_ARRAYS if family == "bvh" else KD_ARRAYS).items():
        a = agg.read(what)
        out[name] = np.zeros(0, np.uint8) if a is None else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    info = agg.info if family == "bvh" else agg.info()
    out["info"] = np.array(list(info.values()), np.int64)
    return out


def stream_slots(kinds):
    """16-byte slots per entry of a BVH scene's primitive stream (nnbvh_internal.h)"""
    k = np.asarray(kinds)
    smooth_patch, uv_patch = (k >= 8) & (k < 16) & (((k - 8) & 2) != 0), (k >= 12) & (k < 16)
    return np.select([k == 1, k == 2, (k == 6) | (k == 7), (k >= 8) & (k < 16), (k == 16) | (k == 17), k >= 18],
                     [4, 6, 6, 4 + 4 * smooth_patch + 2 * uv_patch, 5, 8], 3)


def _flat():
    verts, prims = ss.random_soup(60, 10, 4)
    t = build_tree(prims, verts, 4)
    return "bvh", BVHAggregate.from_tree(t.nodes, t.ordered_prims, verts), t.ordered_prims["kind"]


def _two_level_alpha(name):
    import test_two_level_alpha_texture as t2
    import two_level_alpha_oracle as tlo
    s = t2.static_scene() if name == "static" else t2.animated_scene()
    return "bvh", t2.make_aggregate(s, "host_tree"), tlo.shared_form(s)[1]["kind"]


def _edge_shape(name):
    import test_two_level_device as td
    pt, verts, objects, pl, kw = td.edge_shape(name)
    h = td.host_route(pt, verts, objects, pl, 4, "sah", None, kw.get("prim_bounds"))
    return "bvh", td.host_aggregate(h), h["prims"]["kind"]


def _animated_attributes():
    """the first scene of test_animated_placements_and_attributes_equal_the_host_route_and_the_oracle: 36 placements
    of a grid, two thirds animated, and one static placement of an object of alpha-tested patches (kinds 8, 10, 12)
    and smooth alpha-tested triangles (kind 6); normals, uvs and a per-primitive alpha"""
    import oracle_binding as ob
    import test_two_level_device as td
    from nn_bvh_amd import instancing
    from test_animated import animated_scene
    verts, prims, _, _, _, _, anims, oa, placements = animated_scene(4, 36)
    child = build_tree(prims, verts)
    root = np.concatenate([child.nodes[0]["pmin"], child.nodes[0]["pmax"]])
    motion = np.zeros((len(placements), 6), np.float32)
    for j in range(len(placements)):
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for t in (np.linspace(0, 1, 33) if anims[j]["actually_animated"] else [0.0]):
            m = ob.anim_interpolate(oa[j:j + 1], [t])[0, :16].reshape(4, 4)
            b = instancing.transform_bounds(m[:3].reshape(12), root)
            lo, hi = np.minimum(lo, b[:3]), np.maximum(hi, b[3:])
        pad = 0.05 * (hi - lo) + 1e-3
        motion[j] = np.concatenate([lo - pad, hi + pad])
    vb, pb = ss.random_soup(40, 30, 9, extent=1.0, size=0.3)
    pb = pb.copy()
    pb["v"] += len(verts)
    pb["id"] += 5000
    quads = np.nonzero(pb["kind"] == 1)[0]
    pb["kind"][quads] = np.array([8, 10, 12])[np.arange(len(quads)) % 3]
    tri = np.nonzero(pb["kind"] == 0)[0]
    pb["kind"][tri[::2]] = 6
    pb["v"][tri[::2], 3] = np.float32(0.5).view(np.int32)
    pb["v"][tri[1::2], 3] = 0
    all_verts = np.concatenate([verts, vb]).astype(np.float32)
    rng = np.random.default_rng(3)
    normals = rng.standard_normal((len(all_verts), 3)).astype(np.float32)
    uvs = rng.uniform(0, 1, (len(all_verts), 2)).astype(np.float32)
    pl = list(placements) + [td.placement(1, [[3, 0, 0, 5], [0, 3, 0, -8], [0, 0, 3, 2.0]])]
    anims2 = np.concatenate([anims, np.zeros(1, _lib.ANIMATED_DTYPE)])
    anims2[-1] = anims[0]
    anims2[-1]["actually_animated"] = 0
    entries, _, _ = BVHAggregate.two_level_entries(prims[:0], [prims, pb], pl)
    bounds = np.zeros((len(entries), 6), np.float32)
    bounds[:len(placements)] = motion
    alpha = rng.uniform(0.2, 1.0, len(entries)).astype(np.float32)
    h = td.host_route(prims[:0], all_verts, [prims, pb], pl, 4, "sah", anims2["actually_animated"] != 0, bounds, alpha)
    return "bvh", td.host_aggregate(h, anims2, normals, uvs), h["prims"]["kind"]


def _kd_alpha_texture(name, max_prims, with_uvs):
    import test_kd_alpha_texture as tk
    from nn_bvh_amd.kdtree import KdTreeAggregate
    s, t = tk.scene_of(name), tk.tree_of(name, max_prims, "host")
    agg = KdTreeAggregate.from_tree(t.nodes, t.prim_indices, s.prims, s.verts, t.bounds, normals=s.normals,
                                    uvs=s.uvs if with_uvs else None, alpha_textures=s.textures)
    return "kd", agg, s.prims["kind"]


def _kd_kinds(name):
    """host_among_triangles: host-only primitives; attributes_without_normals: the smooth alpha kinds given without
    normals (the host's record)"""
    import test_kd_device_scene as tk
    verts, prims, pb, attrs = tk._kind_scenes()[name]
    _, agg = tk._host_route(prims, verts, pb, max_prims=2, **attrs)
    return "kd", agg, prims["kind"]


def scenes():
    import test_two_level_device as td
    out = {"flat": _flat}
    for name in ("static", "animated"):
        out["two_level_alpha_texture/" + name] = lambda name=name: _two_level_alpha(name)
    for name in td.EDGE_SHAPES:
        out["edge_shape/" + name] = lambda name=name: _edge_shape(name)
    out["animated_attributes"] = _animated_attributes
    for name in ("soup", "grid"):
        for max_prims in (1, 4):
            for with_uvs in (True, False):
                out[f"kd_alpha_texture/{name}/{max_prims}/{'uvs' if with_uvs else 'no_uvs'}"] = (
                    lambda a=name, b=max_prims, c=with_uvs: _kd_alpha_texture(a, b, c))
    for name in ("host_among_triangles", "attributes_without_normals"):
        out["kd_kinds/" + name] = lambda name=name: _kd_kinds(name)
    return out
