"""Two-level scenes created entirely on the device (nnbvh_scene_create_instanced_gpu_build,
BVHAggregate.build_two_level_on_device) against today's route: trees from the host builder, assembled by
instancing.assemble_two_level's rules, baked by nnbvh_scene_create_instanced_with_attributes.  The device arrays
(nnbvh_scene_read) must be byte for byte the host route's, hence every traversal result too.

CPU: the argument faults (checked before a device is looked at), the generated instance entries, the depths of the
64 / 65 pair.  GPU: byte identity, parity with the oracle, edge shapes, the instance bounds against the reference's
Transform::operator()(Bounds3f) vectors, animated placements and attributes, refusals, invariants."""
import functools
import os

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import BVHAggregate, _lib, build_tree, instancing, make_prims, scene
from nn_bvh_amd._lib import INSTANCE_DTYPE, NNBVHError, PLACEMENT_DTYPE, PRIM_DTYPE, ptr

HERE = os.path.dirname(os.path.abspath(__file__))
SPLITS = {"sah": 0, "hlbvh": 1}


# ---- today's route, generalised to everything the new call takes -------------------------------------------------
def host_route(top_prims, verts, objects, placements, max_prims=4, split="sah", anim_flags=None, prim_bounds=None,
               prim_alpha=None):
    """assemble_two_level with the per-entry arrays of the device call: prim_bounds / prim_alpha are per entry of
    BVHAggregate.two_level_entries(...)[0].  Static instances get nnbvh_transform_bounds of the child root box;
    host-only entries and the instances of animated placements the caller's bounds.  Returns a dict."""
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    entries, n_top, first = BVHAggregate.two_level_entries(top_prims, objects, placements)
    caller_ids = entries["id"].copy()
    tagged = entries.copy()
    tagged["id"] = np.arange(len(entries))  # positions: carried through the builds, as the device call does
    pb = None if prim_bounds is None else np.asarray(prim_bounds, np.float32).reshape(len(entries), 6)
    children = []
    for k in range(len(objects)):
        sl = slice(first[k], first[k + 1])
        children.append(build_tree(tagged[sl], verts, max_prims, split, prim_bounds=None if pb is None else pb[sl]))
    bounds = np.zeros((n_top, 6), np.float32) if pb is None else pb[:n_top].copy()
    for i in range(n_top):
        if tagged["kind"][i] != 2:
            continue
        j = int(tagged["v"][i, 0])
        if anim_flags is not None and anim_flags[j]:
            continue
        root = children[placements[j][0]].nodes[0]
        bounds[i] = instancing.transform_bounds(placements[j][1], np.concatenate([root["pmin"], root["pmax"]]))
    top = build_tree(tagged[:n_top], verts, max_prims, split, prim_bounds=bounds)
    nodes, prims, node_base = [top.nodes], [top.ordered_prims], []
    nb, pbase = len(top.nodes), len(top.ordered_prims)
    for c in children:
        node_base.append(nb)
        cn = c.nodes.copy()
        interior = cn["nprims"] == 0
        cn["offset"][interior] += nb
        cn["offset"][~interior] += pbase
        nodes.append(cn)
        prims.append(c.ordered_prims)
        nb += len(cn)
        pbase += len(c.ordered_prims)
    prims = np.concatenate(prims).astype(PRIM_DTYPE)
    src = prims["id"].copy()
    prims["id"] = caller_ids[src]
    instances = np.zeros(len(placements), INSTANCE_DTYPE)
    for j, (k, m, mi) in enumerate(placements):
        instances[j]["render_from_prim"] = np.asarray(m, np.float32).reshape(12)
        instances[j]["prim_from_render"] = np.asarray(mi, np.float32).reshape(12)
        instances[j]["root"] = node_base[k]
        instances[j]["n_nodes"] = len(children[k].nodes)
    return {"nodes": np.concatenate(nodes), "prims": prims, "instances": instances, "n_top": len(top.nodes),
            "alpha": None if prim_alpha is None else np.asarray(prim_alpha, np.float32)[src],
            "top_depth": top.depth, "child_depths": [c.depth for c in children], "top": top, "verts": verts,
            # create_scene walks only the trees a placement names: the others add nothing to the scene's depth
            "child_depth": max(children[k].depth for k in {p[0] for p in placements})}


def host_aggregate(h, animated=None, normals=None, uvs=None):
    return BVHAggregate.from_tree(h["nodes"], h["prims"], h["verts"], instances=h["instances"], n_top_nodes=h["n_top"],
                                  animated=animated, normals=normals, prim_alpha=h["alpha"], uvs=uvs)


def assert_same_scene(dev, host, what=""):
    for k in (0, 1):
        a, b = dev.read(k), host.read(k)
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: array {k} differs from the host route's"
    assert dev.info == host.info, (what, dev.info, host.info)
    assert np.concatenate(dev.Bounds()).tobytes() == np.concatenate(host.Bounds()).tobytes(), what


def both_routes(top, verts, objects, placements, max_prims=4, split="sah", **kw):
    """(device-built aggregate, host-route aggregate, host-route arrays); kw: prim_bounds, prim_alpha, normals, uvs,
    animated."""
    animated = kw.get("animated")
    flags = None if animated is None else animated["actually_animated"] != 0
    h = host_route(top, verts, objects, placements, max_prims, split, flags, kw.get("prim_bounds"), kw.get("prim_alpha"))
    host = host_aggregate(h, animated, kw.get("normals"), kw.get("uvs"))
    dev = BVHAggregate.build_two_level_on_device(top, verts, objects, placements, max_prims, split, **kw)
    return dev, host, h


# ---- ingredients -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ingredients(seed=0, n_place=60):
    """test_instancing.two_level_scene's: a 12 x 12 grid mesh, a soup of 150 triangles and 30 patches, 40 top-level
    triangles, n_place random affine placements."""
    from test_oracle_vs_reference_live import random_affine
    rng = np.random.default_rng(seed)
    va, pa = ss.grid_mesh(12, seed)
    vb, pb = ss.random_soup(150, 30, seed + 1, extent=1.0, size=0.2)
    vt, pt = ss.random_soup(40, 0, seed + 2, extent=30.0, size=2.0)
    pb = pb.copy()
    pb["v"] += len(va)
    pb["v"][pb["kind"] == 0, 3] = 0
    pt = pt.copy()
    pt["v"][:, :3] += len(va) + len(vb)
    verts = np.concatenate([va, vb, vt]).astype(np.float32)
    M, Mi = random_affine(rng, n_place)
    M[:, :3, 3] = rng.uniform(-25, 25, size=(n_place, 3))
    M[:, :3, :3] *= (0.3 / np.abs(M[:, :3, :3]).max((1, 2)))[:, None, None] * rng.uniform(1, 6, (n_place, 1, 1))
    Mi = np.linalg.inv(M.astype(np.float64)).astype(np.float32)
    placements = [(int(rng.integers(0, 2)), M[j, :3].reshape(12).copy(), Mi[j, :3].reshape(12).copy())
                  for j in range(n_place)]
    return verts, pa, pb, pt, placements


def placement(k, m3x4):
    m = np.eye(4)
    m[:3] = np.asarray(m3x4, np.float64).reshape(3, 4)
    return (k, m[:3].astype(np.float32).reshape(12), np.linalg.inv(m)[:3].astype(np.float32).reshape(12))


def chain(n, e0=-60):
    """n tiny triangles with centroids at 2^i along x: the SAH builder peels a few off per level."""
    c = (2.0 ** (e0 + np.arange(n))).astype(np.float32)
    v = np.zeros((n, 3, 3), np.float32)
    v[:, :, 0] = c[:, None]
    v[:, 1, 0] *= np.float32(1 + 2.0 ** -20)
    v[:, 2, 1] = c * np.float32(2.0 ** -20)
    return v.reshape(-1, 3), make_prims(np.arange(3 * n, dtype=np.int32).reshape(n, 3))


# top list of N_TOP_64 / N_TOP_65 chain triangles + one instance of an N_OBJ-triangle chain, max_prims 1, sah:
# the host builder's depths a (top) and b (child) give a + b + 1 = 64 and 65
N_OBJ, N_TOP_64, N_TOP_65 = 80, 69, 70


def deep_scene(n_top):
    vo, po = chain(N_OBJ)
    vt, pt = chain(n_top)
    pt = pt.copy()
    pt["v"][:, :3] += len(vo)
    pt["id"] += 1000
    m = np.array([[1, 0, 0, 0], [0, 1, 0, 50.0], [0, 0, 1, 0]], np.float64)
    return pt, np.concatenate([vo, vt]), [po], [placement(0, m)]


def deep_scene_with_a_deeper_unnamed_object(n_top):
    """deep_scene plus an object no placement names whose tree is deeper than the named one's: the host route takes
    the scene's depth from the named trees alone."""
    top, verts, objects, placements = deep_scene(n_top)
    vu, pu = chain(126)
    pu = pu.copy()
    pu["v"][:, :3] += len(verts)
    pu["id"] += 5000
    return top, np.concatenate([verts, vu]), objects + [pu], placements


def deep_rays(top, verts, objects, n=4000, seed=1):
    """Rays aimed at the centroids of the chains' triangles (the object's chain stands at y = 50), from origins a few
    triangle sizes off their plane, and rays along the chains through every level."""
    from nn_bvh_amd import make_rays
    rng = np.random.default_rng(seed)
    tris = np.concatenate([verts[top["v"][:, :3]].astype(np.float64),
                           verts[objects[0]["v"][:, :3]].astype(np.float64) + [0, 50.0, 0]])
    pick = rng.integers(0, len(tris), n)
    c = tris[pick].mean(1)
    size = tris[pick][:, 0, 0:1] * 2.0 ** -20
    d = np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), rng.choice([-1.0, 1.0], (n, 1))], 1) * size * 8
    aimed = make_rays((c - d).astype(np.float32), (2 * d).astype(np.float32))
    o = np.stack([rng.uniform(0, 2.0 ** 20, n), rng.choice([0.0, 50.0], n), rng.uniform(-1e-9, 1e-9, n)], 1)
    t = np.stack([np.zeros(n), o[:, 1], np.zeros(n)], 1)
    along = make_rays(o.astype(np.float32), (t - o).astype(np.float32))
    return np.concatenate([aimed, along])


# ---- CPU -------------------------------------------------------------------------------------------------------
def raw_call(L, prims, n_top, first, verts, placements_table, normals=None, uvs=None, alpha=None, bounds=None,
             animated=None, max_prims=4, split=0, device=0, n_objects=None):
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    return L.nnbvh_scene_create_instanced_gpu_build(
        opt(prims), 0 if prims is None else len(prims), n_top, opt(first),
        (len(first) - 1 if first is not None else 0) if n_objects is None else n_objects, opt(verts),
        0 if verts is None else len(verts), opt(normals), opt(uvs), opt(alpha), opt(bounds), opt(placements_table),
        0 if placements_table is None else len(placements_table), opt(animated), max_prims, split, device)


def small_inputs():
    verts, pa, pb, pt, placements = ingredients(5, 6)
    prims, n_top, first = BVHAggregate.two_level_entries(pt, [pa, pb], placements)
    table = np.zeros(len(placements), PLACEMENT_DTYPE)
    for j, (k, m, mi) in enumerate(placements):
        table[j]["render_from_prim"], table[j]["prim_from_render"], table[j]["object"] = m, mi, k
    return prims, n_top, first, verts, table


def test_argument_faults_are_reported_before_any_device_call(nnbvh_lib):
    L = nnbvh_lib
    prims, n_top, first, verts, table = small_inputs()

    def refused(words, **kw):
        a = dict(prims=prims, n_top=n_top, first=first, verts=verts, placements_table=table)
        a.update(kw)
        assert not raw_call(L, **a), words
        assert words in _lib.last_error(), (words, _lib.last_error())

    # a well-formed call gets as far as the device check (an index no machine has)
    refused("no usable HIP device", device=1 << 20)
    refused("null or empty", prims=None)
    refused("null or empty", verts=None)
    refused("null or empty", first=None, n_objects=2)
    refused("null or empty", placements_table=None)
    refused("null or empty", placements_table=table[:0])
    refused("null or empty", n_top=0)
    for bad in (first + 1, first[[0, 2, 1]], np.array([first[0], first[1], first[1], first[2]], np.int32),
                np.array([first[0], first[2] + 1], np.int32)):
        refused("malformed object_first", first=np.ascontiguousarray(bad, np.int32))
    t = table.copy()
    t["object"][3] = 2
    refused("placement object out of range", placements_table=t)
    t["object"][3] = -1
    refused("placement object out of range", placements_table=t)
    inst_rows = np.nonzero(prims["kind"] == 2)[0]
    for v0 in (-1, len(table)):
        p = prims.copy()
        p["v"][inst_rows[0], 0] = v0
        refused("instance index out of range", prims=p)
    p = prims.copy()
    p["kind"][first[1] - 1] = 2
    p["v"][first[1] - 1, 0] = 0
    refused("nested instances are not supported", prims=p)
    for row, v in ((0, len(verts)), (first[0] + 3, -1), (first[1] + 2, 1 << 30)):
        p = prims.copy()
        p["v"][row, 1] = v
        refused("vertex index out of range", prims=p)
    p = prims.copy()
    p["kind"][first[0] + 1] = 99
    refused("unknown primitive kind", prims=p)
    for row in (2, first[1] + 5):  # host-only entries in the top list and inside an object
        p = prims.copy()
        p["kind"][row] = 3
        refused("need prim_bounds", prims=p)
    p = prims.copy()
    p["kind"][first[0] + 2] = 6  # smooth alpha triangle
    refused("need the vertex normals", prims=p)
    quad = np.nonzero(prims["kind"] == 1)[0][0]
    nrm, uv = np.zeros((len(verts), 3), np.float32), np.zeros((len(verts), 2), np.float32)
    alpha = np.ones(len(prims), np.float32)
    for kind, have in ((8, {}), (10, {"alpha": alpha}), (12, {"alpha": alpha, "normals": nrm}),
                       (14, {"alpha": alpha, "uvs": uv})):
        p = prims.copy()
        p["kind"][quad] = kind
        refused("NNBVH_PRIM_ALPHA_PATCH primitives need", prims=p, **have)
    anim = np.zeros(len(table), _lib.ANIMATED_DTYPE)
    anim["actually_animated"][2] = 1
    anim["start_time"], anim["end_time"] = 1.0, 1.0
    refused("empty time range", animated=anim, bounds=np.zeros((len(prims), 6), np.float32))
    anim["end_time"] = 2.0
    refused("need prim_bounds", animated=anim)  # MotionBounds stay the caller's
    refused("only the sah and hlbvh", split=2)
    refused("only the sah and hlbvh", split=3)


def test_host_tree_call_refuses_a_malformed_node_outside_every_instances_tree(nnbvh_lib):
    """The nodes of an object no instance names are not walked by the tree validation, yet the bake makes a record of
    each and looks up each leaf's slot: what they index with is range-checked before anything goes to a device
    (device = an index no machine has; the well-formed scene gets as far as the device check)."""
    pt, verts, objects, pl, _ = edge_shape("unnamed object")
    h = host_route(pt, verts, objects, pl)
    named = np.zeros(len(h["nodes"]), bool)
    named[:h["n_top"]] = True
    for inst in h["instances"]:
        named[inst["root"]:inst["root"] + inst["n_nodes"]] = True
    unnamed = np.nonzero(~named)[0]
    interior = unnamed[h["nodes"]["nprims"][unnamed] == 0]
    leaves = unnamed[h["nodes"]["nprims"][unnamed] != 0]
    assert len(interior) > 2 and len(leaves) > 2

    def create(nodes):
        return nnbvh_lib.nnbvh_scene_create_instanced(ptr(nodes), len(nodes), h["n_top"], ptr(h["prims"]), len(h["prims"]),
                                                     ptr(verts), len(verts), ptr(h["instances"]), len(h["instances"]),
                                                     1 << 20)

    assert not create(h["nodes"]) and "no usable HIP device" in _lib.last_error()
    bad = [(interior[1], "offset", len(h["nodes"])), (interior[1], "offset", 1 << 30), (interior[0], "offset", -1),
           (interior[2], "offset", interior[2] + 1), (interior[0], "axis", 3),
           (leaves[0], "offset", len(h["prims"])), (leaves[1], "offset", -1), (leaves[-1], "nprims", 60000)]
    for node, field, value in bad:
        nodes = h["nodes"].copy()
        nodes[field][node] = value
        assert not create(nodes), (node, field, value)
        assert "scene_create: malformed node outside every instance's tree" in _lib.last_error(), (node, field, value)
    # the same damage inside a named tree is the tree validation's to report, as before
    nodes = h["nodes"].copy()
    nodes["offset"][h["instances"]["root"][0]] = len(nodes)
    assert not create(nodes) and "outside the node's subtree range" in _lib.last_error()


def test_scene_read_refuses_a_null_scene(nnbvh_lib):
    out = np.zeros(16, np.uint32)
    assert nnbvh_lib.nnbvh_scene_read(None, 0, ptr(out), out.nbytes) == 1  # NNBVH_ERR_ARG
    assert "null" in _lib.last_error()


def test_generated_instance_entries_equal_assemble_two_levels(nnbvh_lib):
    verts, pa, pb, pt, placements = ingredients(5, 6)
    prims, n_top, first = BVHAggregate.two_level_entries(pt, [pa, pb], placements)
    _, aprims, _, n_top_nodes = instancing.assemble_two_level(pt, verts, [pa, pb], placements)
    assert n_top == len(pt) + len(placements) and list(first) == [n_top, n_top + len(pa), n_top + len(pa) + len(pb)]
    mine = prims[len(pt):n_top]
    theirs = aprims[:n_top][aprims[:n_top]["kind"] == 2]
    theirs = theirs[np.argsort(theirs["v"][:, 0])]
    assert mine.tobytes() == theirs.tobytes()
    assert prims[:len(pt)].tobytes() == pt.tobytes() and prims[n_top:].tobytes() == np.concatenate([pa, pb]).tobytes()
    # and the generalised host route of this file is assemble_two_level where both apply
    h = host_route(pt, verts, [pa, pb], placements)
    nodes, aprims, instances, n_top_nodes = instancing.assemble_two_level(pt, verts, [pa, pb], placements)
    assert h["nodes"].tobytes() == nodes.tobytes() and h["prims"].tobytes() == aprims.tobytes()
    assert h["instances"].tobytes() == instances.tobytes() and h["n_top"] == n_top_nodes


def test_depths_of_the_64_and_65_pair(nnbvh_lib):
    for n_top, total in ((N_TOP_64, 64), (N_TOP_65, 65)):
        top, verts, objects, placements = deep_scene(n_top)
        h = host_route(top, verts, objects, placements, 1, "sah")
        assert h["top_depth"] + h["child_depth"] + 1 == total, (n_top, h["top_depth"], h["child_depth"])
    # an object nobody places, deeper than the named one, changes neither sum
    for n_top, total in ((N_TOP_64, 64), (N_TOP_65, 65)):
        top, verts, objects, placements = deep_scene_with_a_deeper_unnamed_object(n_top)
        h = host_route(top, verts, objects, placements, 1, "sah")
        assert h["child_depths"][1] > h["child_depths"][0] == h["child_depth"]
        assert h["top_depth"] + h["child_depth"] + 1 == total and h["top_depth"] + h["child_depths"][1] + 1 > 64
    # the rays of the GPU test reach both levels of the accepted scene, and deep into them
    top, verts, objects, placements = deep_scene(N_TOP_64)
    h = host_route(top, verts, objects, placements, 1, "sah")
    exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], deep_rays(top, verts, objects), 8)
    assert (exp["instance"] > 0).sum() > 100 and (exp["prim"] >= 1000).sum() > 100 and exp["nodes_visited"].max() > 64


# ---- GPU -------------------------------------------------------------------------------------------------------
def trace_rays(verts, prims, seed):
    lo = np.array([-30, -30, -30.0])
    return np.concatenate([scene.random_rays(20000, lo, -lo, seed + 20),
                           ss.edge_case_rays(verts, prims[prims["kind"] != 2], seed, 2048)])


@pytest.mark.gpu
@pytest.mark.parametrize("split,max_prims", [("sah", 1), ("sah", 4), ("hlbvh", 1), ("hlbvh", 4)])
def test_device_built_two_level_scene_is_the_host_routes(split, max_prims):
    from test_gpu_parity import assert_hits_equal
    verts, pa, pb, pt, placements = ingredients(0, 60)
    dev, host, h = both_routes(pt, verts, [pa, pb], placements, max_prims, split)
    assert dev.nodes is None and dev.ordered_prims is None
    assert_same_scene(dev, host, f"{split} {max_prims}")
    rays = trace_rays(verts, h["prims"], 0)
    got, ref = dev.Intersect(rays), host.Intersect(rays)
    assert got.tobytes() == ref.tobytes()
    exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 16)
    assert (exp["instance"] > 0).sum() > 500
    assert_hits_equal(got, exp, "device-built two-level closest")
    assert (got["instance"] == exp["instance"]).all()
    eocc, evis, etst = ob.any_hit_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 16)
    occ, vis, tst = dev.IntersectP(rays, counts=True)
    hocc, hvis, htst = host.IntersectP(rays, counts=True)
    assert occ.tobytes() == hocc.tobytes() and vis.tobytes() == hvis.tobytes() and tst.tobytes() == htst.tobytes()
    assert (occ == eocc).all() and (vis == evis).all() and (tst == etst).all()
    assert (dev.IntersectP(rays) == eocc).all()
    dev.close()
    host.close()


def zero_edge_case(order):
    """Two placements of a box x in [0, 1], y, z in [-1, 1] whose transformed bounds end at a zero: with the
    row (-1, 0, -0, -0) the corners give -0 and +0 by turns (first of equals decides), with (-1, -0, -0, -0) ... ;
    listed in both orders."""
    v = np.array([[0, -1, -1], [1, 1, -1], [0, 1, 1], [1, -1, 1], [0.5, 0, 0], [1, 1, 1]], np.float32)
    obj = make_prims(np.array([[0, 1, 2], [3, 4, 5], [0, 3, 5], [1, 2, 4], [2, 3, 1]], np.int32))
    inv = np.array([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    a = (0, np.array([-1, 0.0, -0.0, -0.0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), inv)
    b = (0, np.array([-1, -0.0, 0.0, 0.0, 0, 1, 0, -0.0, 0, 0, 1, 0.0], np.float32), inv)
    c = placement(0, [[1, 0, 0, 3], [0, 1, 0, 0], [0, 0, 1, 0]])
    return obj[:0], v, [obj], [a, b, c] if order == 0 else [b, a, c]


def edge_shape(name):
    verts, pa, pb, pt, placements = ingredients(1, 12)
    kw = {}
    if name == "one-primitive object":
        objects, pl = [pa[:1], pb], placements
    elif name == "object of exactly max_prims":
        objects, pl = [pa[:4], pb], placements
    elif name == "instances only":
        pt, objects, pl = pt[:0], [pa, pb], placements
    elif name == "one placement":
        pt, objects, pl = pt[:0], [pa, pb], placements[:1]
    elif name == "one placement of a one-primitive object":
        pt, objects, pl = pt[:0], [pb[:1]], [(0,) + placements[0][1:]]
    elif name == "unnamed object":
        objects, pl = [pa, pb[:100], pb[100:]], [(min(k, 1) * 2, m, mi) for k, m, mi in placements]
    elif name == "unnamed object is the deepest":
        vu, pu = chain(120)
        pu = pu.copy()
        pu["v"][:, :3] += len(verts)
        pu["id"] += 5000
        verts, objects, pl = np.concatenate([verts, vu]), [pa, pu, pb], [(k * 2, m, mi) for k, m, mi in placements]
    elif name == "identical matrices":
        objects, pl = [pa, pb], placements[:5] + [placements[2], placements[2]] + placements[5:]
    elif name == "mirrored":
        mirror = np.array([[-1.5, 0, 0, 4], [0.2, 1, 0, -3], [0, 0, 2, 7.0]])
        assert np.linalg.det(mirror[:, :3]) < 0
        objects, pl = [pa, pb], placements + [placement(1, mirror), placement(0, mirror * [[1], [-1], [-1]])]
    elif name in ("zero extremes", "zero extremes, other order"):
        pt, verts, objects, pl = zero_edge_case(0 if name == "zero extremes" else 1)
    elif name == "host-only entries":
        pt, pa = pt.copy(), pa.copy()
        pt["kind"][::5] = 3
        pa["kind"][3::7] = 3
        objects, pl = [pa, pb], placements
        entries, _, _ = BVHAggregate.two_level_entries(pt, objects, pl)
        tri = verts[np.where(entries["kind"][:, None] == 2, 0, entries["v"][:, :3])]
        kw["prim_bounds"] = np.concatenate([tri.min(1), tri.max(1)], 1).astype(np.float32)
    else:
        raise KeyError(name)
    return pt, verts, objects, pl, kw


EDGE_SHAPES = ["one-primitive object", "object of exactly max_prims", "instances only", "one placement",
               "one placement of a one-primitive object", "unnamed object", "unnamed object is the deepest",
               "identical matrices", "mirrored",
               "zero extremes", "zero extremes, other order", "host-only entries"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", EDGE_SHAPES)
def test_edge_shapes_bake_to_the_host_routes_bytes(name):
    pt, verts, objects, pl, kw = edge_shape(name)
    for split in ("sah", "hlbvh"):
        dev, host, h = both_routes(pt, verts, objects, pl, 4, split, **kw)
        assert_same_scene(dev, host, f"{name} {split}")
        if name == "one placement of a one-primitive object":
            stream = dev.read(1)
            assert dev.info["interior_records"] == 0 and stream[5, 0] == np.uint32(~6 & 0xffffffff)  # child root = a leaf
        if name == "unnamed object is the deepest" and split == "sah":  # (hlbvh keeps the chain as shallow as the rest)
            # ... and the scene's depth is still the named trees'
            assert h["child_depths"][1] > max(h["child_depths"][0], h["child_depths"][2]) == h["child_depth"]
            assert dev.info["depth"] == h["top_depth"] + h["child_depth"] + 1
        if name.startswith("zero extremes"):
            # both signs of zero reach the baked child boxes' x maxima, so the comparison above has looked at them
            box_hi = h["top"].nodes["pmax"][:, 0]
            assert (box_hi == 0).any()
        rays = scene.random_rays(3000, [-30, -30, -30], [30, 30, 30], 3)
        assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes(), name
        dev.close()
        host.close()


@pytest.mark.gpu
def test_instance_bounds_equal_the_reference_vectors():
    """Transform::operator()(Bounds3f) of the reference binary (tests/golden/leaf_xfbounds.npz): one single-triangle
    object per record whose box is the record's, one placement each, max_prims 1: the child box stored in the interior
    record that refers to each instance's leaf is the golden output, bit for bit.  The records used are the first 256
    that are finite (matrix, box and output) AND whose box has pmin <= pmax on every axis: only then is the box of
    the triangle (pmin, pmax, (pmin.x, pmax.y, pmin.z)) the record's box."""
    g = np.load(os.path.join(HERE, "golden", "leaf_xfbounds.npz"))
    r, bits = g["inputs"], g["out_bits"]
    fine = np.isfinite(r[:, 0:12]).all(1) & np.isfinite(r[:, 16:22]).all(1) & np.isfinite(bits.view(np.float32)).all(1)
    fine &= (r[:, 16:19] <= r[:, 19:22]).all(1)
    pick = np.nonzero(fine)[0][:256]
    assert len(pick) == 256
    lo, hi = r[pick, 16:19], r[pick, 19:22]
    verts = np.stack([lo, hi, np.stack([lo[:, 0], hi[:, 1], lo[:, 2]], 1)], 1).reshape(-1, 3).astype(np.float32)
    tris = make_prims(np.arange(3 * 256, dtype=np.int32).reshape(256, 3))
    ident = np.eye(4, dtype=np.float32)[:3].reshape(12)
    placements = [(j, r[pick[j], 0:12].astype(np.float32), ident) for j in range(256)]
    dev = BVHAggregate.build_two_level_on_device(tris[:0], verts, [tris[j:j + 1] for j in range(256)], placements, 1, "sah")
    wide, stream = dev.read(0), dev.read(1)
    found = 0
    for which, at in ((12, 0), (13, 6)):  # ref0 with its box q[0:6], ref1 with q[6:12]
        ref = wide[:, which].view(np.int32)
        rows = np.nonzero(ref < 0)[0]
        slot = ~ref[rows]
        inst = (stream[slot + 1, 3] & 8) != 0  # kPrimInstance
        rows, slot = rows[inst], slot[inst]
        j = stream[slot, 3].view(np.int32)  # the placement index
        assert ((stream[slot + 1, 3] & 1) != 0).all()  # the leaf's last (only) primitive
        assert (wide[rows, at:at + 6] == bits[pick[j]]).all()
        found += len(rows)
    assert found == 256
    dev.close()


@pytest.mark.gpu
def test_animated_placements_and_attributes_equal_the_host_route_and_the_oracle():
    from test_animated import animated_scene, rebuild_with_motion_bounds
    verts, prims, _, _, _, _, anims, oa, placements = animated_scene(4, 36)
    # its motion bounds (the padded boxes of the instances' top-level entries), handed over as prim_bounds
    nodes_m, aprims_m, _, n_top_m = rebuild_with_motion_bounds(verts, prims, placements, anims, oa)
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
    # a second object: alpha patches (kinds 8, 10, 12) and smooth alpha triangles (kind 6)
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
    pl = list(placements) + [placement(1, [[3, 0, 0, 5], [0, 3, 0, -8], [0, 0, 3, 2.0]])]
    anims2 = np.concatenate([anims, np.zeros(1, _lib.ANIMATED_DTYPE)])
    anims2[-1] = anims[0]
    anims2[-1]["actually_animated"] = 0
    entries, n_top, first = BVHAggregate.two_level_entries(prims[:0], [prims, pb], pl)
    bounds = np.zeros((len(entries), 6), np.float32)
    bounds[:len(placements)] = motion
    bounds[len(placements)] = np.nan  # a static placement's: ignored
    alpha = rng.uniform(0.2, 1.0, len(entries)).astype(np.float32)
    dev, host, h = both_routes(prims[:0], all_verts, [prims, pb], pl, 4, "sah", animated=anims2,
                               prim_bounds=bounds, prim_alpha=alpha, normals=normals, uvs=uvs)
    assert_same_scene(dev, host, "animated + attributes")
    assert dev.read(2).tobytes() == host.read(2).tobytes() and dev.read(2).shape == (len(pl), 76)
    assert dev.info["interior_records"] > 0
    n = 30000
    rays = scene.random_rays(n, [-25, -25, -25], [25, 25, 25], 5)
    rays["time"] = np.random.default_rng(6).uniform(-0.2, 1.2, n).astype(np.float32)
    got = dev.Intersect(rays)
    occ, vis, tst = dev.IntersectP(rays, counts=True)
    assert got.tobytes() == host.Intersect(rays).tobytes()
    hocc = host.IntersectP(rays, counts=True)
    assert occ.tobytes() == hocc[0].tobytes() and vis.tobytes() == hocc[1].tobytes() and tst.tobytes() == hocc[2].tobytes()
    dev.close()
    host.close()
    # the oracle, as test_device_animated_instances_equal_the_oracle compares: the animated object alone (the oracle
    # has no alpha test), bit-equal with the device's sine
    dev, host, h = both_routes(prims[:0], verts, [prims], placements, 4, "sah", animated=anims,
                               prim_bounds=np.concatenate([motion, np.zeros((len(prims), 6), np.float32)]))
    assert_same_scene(dev, host, "animated")
    assert dev.read(2).tobytes() == host.read(2).tobytes()
    got = dev.Intersect(rays)
    occ, vis, tst = dev.IntersectP(rays, counts=True)
    try:
        ob.set_sin_mode(1)
        exp = ob.closest_anim(h["nodes"], h["prims"], verts, h["instances"], oa, rays, 4)
        eo, ev, et = ob.any_hit_anim(h["nodes"], h["prims"], verts, h["instances"], oa, rays, 4)
    finally:
        ob.set_sin_mode(0)
    assert got.tobytes() == exp.tobytes(), "device differs from the oracle with the device's sine"
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
    assert (exp["instance"] > 0).mean() > 0.1
    dev.close()
    host.close()


@pytest.mark.gpu
def test_malformed_geometry_is_refused_with_the_builders_messages():
    """A non-finite vertex is found by the device builder (k_prim_bounds) while it builds the object.  A vertex index
    out of range never gets that far through this call: the host-side argument check, which runs first, reports it
    in the builder's words (the builders' own index check is exercised by tests/test_gpu_build.py's callers of
    build_on_device / build_tree_gpu).  The flat build_on_device goes on refusing an instance entry."""
    verts, pa, pb, pt, placements = ingredients(1, 12)
    bad = verts.copy()
    bad[pb["v"][7, 1]] = np.inf
    with pytest.raises(NNBVHError, match="non-finite vertex"):
        BVHAggregate.build_two_level_on_device(pt, bad, [pa, pb], placements)
    badp = pb.copy()
    badp["v"][11, 2] = len(verts)
    with pytest.raises(NNBVHError, match="vertex index out of range"):
        BVHAggregate.build_two_level_on_device(pt, verts, [pa, badp], placements)
    flat = np.concatenate([pt, BVHAggregate.two_level_entries(pt, [pa], placements[:1])[0][len(pt):len(pt) + 1]])
    with pytest.raises(NNBVHError, match="instance"):
        BVHAggregate.build_on_device(flat, verts, prim_bounds=np.zeros((len(flat), 6), np.float32))


@pytest.mark.gpu
def test_depth_64_is_accepted_and_65_refused():
    from test_gpu_parity import assert_hits_equal
    top, verts, objects, placements = deep_scene(N_TOP_64)
    dev, host, h = both_routes(top, verts, objects, placements, 1, "sah")
    assert dev.info["depth"] == 64 == h["top_depth"] + h["child_depth"] + 1
    assert_same_scene(dev, host, "depth 64")
    rays = deep_rays(top, verts, objects)
    got = dev.Intersect(rays)
    exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 8)
    assert_hits_equal(got, exp, "depth 64")
    assert (got["instance"] == exp["instance"]).all()
    assert (exp["instance"] > 0).sum() > 100 and (exp["prim"] >= 1000).sum() > 100 and exp["nodes_visited"].max() > 64
    dev.close()
    host.close()
    top, verts, objects, placements = deep_scene(N_TOP_65)
    with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
        BVHAggregate.build_two_level_on_device(top, verts, objects, placements, 1, "sah")
    # an object nobody places, deeper than the named one, does not count: accepted at 64 as the host route accepts
    # it, with the host route's info (depth, hence the spill sizing) and arrays; refused at 65 like the host route
    top, verts, objects, placements = deep_scene_with_a_deeper_unnamed_object(N_TOP_64)
    dev, host, h = both_routes(top, verts, objects, placements, 1, "sah")
    assert dev.info["depth"] == 64 and h["top_depth"] + h["child_depths"][1] + 1 > 64
    assert_same_scene(dev, host, "depth 64 beside a deeper unnamed object")
    got = dev.Intersect(rays)
    assert_hits_equal(got, exp, "depth 64 beside a deeper unnamed object")
    assert (got["instance"] == exp["instance"]).all()
    dev.close()
    host.close()
    top, verts, objects, placements = deep_scene_with_a_deeper_unnamed_object(N_TOP_65)
    with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
        BVHAggregate.build_two_level_on_device(top, verts, objects, placements, 1, "sah")
    with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
        host_aggregate(host_route(top, verts, objects, placements, 1, "sah"))


@pytest.mark.gpu
def test_device_unchanged_and_two_scenes_alive():
    import torch
    from test_gpu_parity import assert_hits_equal
    verts, pa, pb, pt, placements = ingredients(2, 20)
    before = torch.cuda.current_device()
    first = BVHAggregate.build_two_level_on_device(pt, verts, [pa, pb], placements)
    assert torch.cuda.current_device() == before
    second, host2, h2 = both_routes(pt[:10], verts, [pb, pa], placements[:7], 2, "hlbvh")
    h1 = host_route(pt, verts, [pa, pb], placements)
    rays = scene.random_rays(8000, [-30, -30, -30], [30, 30, 30], 4)
    for agg, h in ((first, h1), (second, h2), (first, h1)):
        exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 8)
        got = agg.Intersect(rays)
        assert_hits_equal(got, exp, "two scenes alive")
        assert (got["instance"] == exp["instance"]).all() and (exp["instance"] > 0).sum() > 100
    for a in (first, second, host2):
        a.close()
