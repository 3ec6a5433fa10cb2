"""The HLBVH trees of many objects built in ONE device pass (nnbvh_build_forest_create_gpu_hlbvh,
build_hlbvh_forest_gpu) and the two-level scene call that uses it (nnbvh_scene_create_instanced_gpu_build with
NNBVH_SPLIT_HLBVH).

The yardstick for the bytes is the host builder on each object alone (build_tree(obj, verts, max_prims, "hlbvh")), byte
for byte (-0 is not +0); for the refusals, what the single device build of that object (build_tree_gpu) raises; for
scenes, the host route of test_two_level_device.  NNBVH_TWO_LEVEL_LOOP=1 keeps the object-by-object loop reachable, so
the forest route, the loop route and the host route are held side by side.

CPU: the argument faults, refused before a device is looked at.  GPU: every decision path of the HLBVH builder inside
one forest (a one-leaf object beside one of 4096 treelets), small and big neighbours sharing one sort, one radix tree
and one treelet table in both orders, two-level scenes on all three routes, and the refusals a loop over the objects
would have stopped at."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import (BVHAggregate, NNBVHError, _lib, build_hlbvh_forest_gpu, build_tree, build_tree_gpu, scene)
from nn_bvh_amd._lib import PRIM_DTYPE, ptr
from test_bvh_build_paths import PATH_CASES, morton_codes, path_scene
from test_bvh_forest import assert_forest_is_the_host_trees, join, shifted  # noqa: F401 (shifted: join's own helper)
from test_two_level_device import assert_same_scene, both_routes, ingredients, placement, trace_rays

LOOP = "NNBVH_TWO_LEVEL_LOOP"
HLBVH_SCENES = tuple(dict.fromkeys(p.values[1] for p in PATH_CASES if p.values[2] == "hlbvh"))


def treelets_of(boxes):
    """Groups of equal top-12 Morton bits (census_hlbvh's own count), from the primitives' boxes."""
    return len(np.unique(morton_codes(np.asarray(boxes, np.float32).reshape(-1, 6)) >> 18))


# ---- CPU -------------------------------------------------------------------------------------------------------
def raw_forest(L, prims, first, verts, bounds=None, max_prims=4, device=0, n_objects=None):
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    return L.nnbvh_build_forest_create_gpu_hlbvh(
        opt(prims), 0 if prims is None else len(prims), opt(first),
        (len(first) - 1 if first is not None else 0) if n_objects is None else n_objects, opt(verts),
        0 if verts is None else len(verts), opt(bounds), max_prims, device)


def test_hlbvh_forest_argument_faults_are_reported_before_any_device_call(nnbvh_lib):
    L = nnbvh_lib
    verts, objects = join([ss.random_soup(20, 6, 1), ss.random_soup(9, 0, 2), ss.random_soup(33, 3, 3)])
    prims = np.ascontiguousarray(np.concatenate(objects), PRIM_DTYPE)
    first = np.array([0, 26, 35, 71], np.int32)

    def refused(words, **kw):
        a = dict(prims=prims, first=first, verts=verts)
        a.update(kw)
        assert not raw_forest(L, **a), words
        assert words in _lib.last_error(), (words, _lib.last_error())

    # a well-formed call gets as far as the device check (an index no machine has)
    refused("no usable HIP device", device=1 << 20)
    refused("null or empty", prims=None)
    refused("null or empty", verts=None)
    refused("null or empty", first=None, n_objects=3)
    refused("null or empty", n_objects=0)
    for bad in (first + 1, first[[0, 2, 1, 3]], np.array([0, 26, 26, 71], np.int32), np.array([0, 26, 35, 72], np.int32),
                np.array([0, 26, 35, 70], np.int32)):
        refused("malformed object_first", first=np.ascontiguousarray(bad, np.int32))
    for row, col, v in ((0, 1, len(verts)), (30, 0, -1), (70, 2, 1 << 30)):
        p = prims.copy()
        p["v"][row, col] = v
        refused("vertex index out of range", prims=p)
    quad = np.nonzero(prims["kind"] == 1)[0][0]
    p = prims.copy()
    p["v"][quad, 3] = len(verts)
    refused("vertex index out of range", prims=p)
    p = prims.copy()
    p["kind"][40] = 99
    refused("unknown primitive kind", prims=p)
    p = prims.copy()
    p["kind"][27] = 2
    p["v"][27, 0] = 0
    refused("instance entries are not built in a forest", prims=p)
    refused("instance entries are not built in a forest", prims=p, bounds=np.zeros((len(prims), 6), np.float32))
    p = prims.copy()
    p["kind"][5] = 3
    refused("need prim_bounds", prims=p)
    refused("no usable HIP device", prims=p, bounds=np.zeros((len(prims), 6), np.float32), device=1 << 20)
    # a tree reads no vertex attributes: the alpha kinds are fine without normals / alpha / uvs
    p = prims.copy()
    p["kind"][3], p["kind"][quad] = 6, 14
    refused("no usable HIP device", prims=p, device=1 << 20)
    # NULL handles are argument errors, not crashes
    assert L.nnbvh_forest_nodes(None, None) is None and L.nnbvh_forest_n_levels(None) == -1
    assert L.nnbvh_forest_n_subtrees(None) == -1
    assert L.nnbvh_forest_gpu_timing(None, None) == 1
    L.nnbvh_forest_destroy(None)


# ---- GPU 1: every decision path, inside a forest -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_forest():
    verts, objects = join([path_scene(name)[:2] for name in HLBVH_SCENES])
    return verts, objects, sum(treelets_of(path_scene(name)[2]) for name in HLBVH_SCENES)


@functools.lru_cache(maxsize=None)
def path_forest_hosts(max_prims):
    verts, objects, _ = path_forest()
    return [build_tree(o, verts, max_prims, "hlbvh") for o in objects]


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 2, 4, 255])
def test_every_hlbvh_decision_path_inside_one_forest(max_prims):
    assert set(HLBVH_SCENES) == {"coincident", "soup1", "cluster_and_outlier", "sparse_soup", "all_cells", "code_runs",
                                 "dense_cell", "signed_zeros", "leaf_rules", "huge_soup"}
    verts, objects, n_treelets = path_forest()
    forest = build_hlbvh_forest_gpu(objects, verts, max_prims)
    assert_forest_is_the_host_trees(forest, path_forest_hosts(max_prims), f"max_prims {max_prims}")
    assert len(forest.gpu_ms) == 5 and forest.n_levels == 0
    assert forest.n_subtrees == n_treelets > 4096  # all_cells alone has 4096: the forest's tables go past one object's


# ---- GPU 2: neighbours do not leak -------------------------------------------------------------------------------
SIZES = (1, 2, 3, 64, 65, 256, 257)


def coplanar_centroids(n, seed):
    """A soup whose bounds centroids all lie in the plane z = 0.5: one axis of the object's centroid bounds is flat."""
    v, p = ss.random_soup(n, 0, seed, extent=2.0, size=0.25)
    v = v.reshape(n, 3, 3).copy()
    h = np.abs(v[:, :, 2]).max(1) / np.float32(4) + np.float32(0.125)
    h = (np.round(h * 64) / 64).astype(np.float32)            # multiples of 1/64: .5 (c - h) + .5 (c + h) == c exactly
    v[:, 0, 2], v[:, 1, 2], v[:, 2, 2] = 0.5 - h, 0.5 + h, 0.5
    return v.reshape(-1, 3).astype(np.float32), p


@functools.lru_cache(maxsize=None)
def neighbours():
    """test_bvh_forest.neighbours()'s construction (sizes cycling through SIZES, 3 soups per size, every geometry at
    several places of the list and translated every second time, one object of 2049 and one of 4097 in the middle),
    plus an object with coplanar centroids and one of 300 coincident centroids that stands directly before and directly
    after a one-triangle object."""
    parts, soups = [], {}
    for j in range(299):
        n, variant = SIZES[j % 7], (j // 7) % 3
        if (n, variant) not in soups:
            soups[n, variant] = ss.random_soup(n, 0, 1000 + 10 * n + variant, extent=3.0, size=0.4)
        v, p = soups[n, variant]
        if (j // 21) % 2:
            v = (v + np.float32([0.37 * j, -1.5, 0.001 * j])).astype(np.float32)
        parts.append((v, p))
    parts[150:150] = [ss.random_soup(2049, 0, 77), ss.random_soup(4097, 0, 78)]
    one, lump = ss.random_soup(1, 0, 79), ss.coincident_centroids(300, 5)
    parts[40:40] = [coplanar_centroids(90, 80)]
    parts[200:200] = [lump, one, lump]
    verts, objects = join(parts)
    cen = [(verts[o["v"][:, :3]].min(1) + verts[o["v"][:, :3]].max(1)) / 2 for o in (objects[40], objects[200])]
    assert np.ptp(cen[0][:, 2]) == 0 and np.ptp(cen[0][:, 0]) > 0 and not np.ptp(cen[1], axis=0).any()
    assert [len(objects[k]) for k in (200, 201, 202)] == [300, 1, 300]
    return verts, objects


@functools.lru_cache(maxsize=None)
def neighbour_hosts(max_prims):
    verts, objects = neighbours()
    return [build_tree(o, verts, max_prims, "hlbvh") for o in objects]


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_hlbvh_neighbours_do_not_leak_in_either_order(max_prims):
    verts, objects = neighbours()
    hosts = neighbour_hosts(max_prims)
    assert len(objects) == 305 and sorted({len(o) for o in objects}) == sorted(SIZES + (90, 300, 2049, 4097))
    forest = build_hlbvh_forest_gpu(objects, verts, max_prims)
    assert_forest_is_the_host_trees(forest, hosts, "in order")
    assert len(forest[200].nodes) == 1 == len(forest[201].nodes)  # one code, one big leaf, beside a one-leaf object
    back = build_hlbvh_forest_gpu(objects[::-1], verts, max_prims)
    assert_forest_is_the_host_trees(back, hosts[::-1], "reversed")
    # the same geometry, wherever it stands in the list, gives the same tree
    seen = {}
    for o, t in zip(objects, forest):
        key = (len(o), verts[o["v"][:, :3]].tobytes())
        assert seen.setdefault(key, t.nodes.tobytes()) == t.nodes.tobytes()
    assert len(seen) < len(objects)
    keep = [k for k, o in enumerate(objects) if len(o) <= 256]
    small = build_hlbvh_forest_gpu([objects[k] for k in keep], verts, max_prims)
    assert_forest_is_the_host_trees(small, [hosts[k] for k in keep], "small objects only")
    assert len(keep) > 250 and small.n_levels == 0 and small.n_subtrees >= len(keep)
    # the two key widths: one object alone sorts its 32-bit codes, beside a one-triangle neighbour (before it or
    # after it) 64-bit keys.  66 of its 70 triangles share a centroid: a leaf folded by a wavefront beside ordinary ones
    (v, lump), (w, rest) = ss.coincident_centroids(66, 7), ss.random_soup(4, 0, 81, extent=3.0, size=0.4)
    x = np.concatenate([lump, shifted(rest, len(v))])
    verts, (x, one) = join([(np.concatenate([v, w]), x), ss.random_soup(1, 0, 79)])
    host = build_tree(x, verts, max_prims, "hlbvh")
    leaves = host.nodes["nprims"][host.nodes["nprims"] > 0]
    assert len(x) == 70 and leaves.max() == 66 and len(leaves) > 1
    alone = build_tree_gpu(x, verts, max_prims, split_method="hlbvh")
    first, second = build_hlbvh_forest_gpu([x, one], verts, max_prims)[0], build_hlbvh_forest_gpu([one, x], verts, max_prims)[1]
    for t, what in ((alone, "alone"), (first, "object 0 of 2"), (second, "object 1 of 2")):
        assert t.nodes.tobytes() == host.nodes.tobytes(), f"{what}: nodes differ"
        assert t.ordered_prims.tobytes() == host.ordered_prims.tobytes(), f"{what}: ordered primitives differ"
        assert t.depth == host.depth, f"{what}: depth {t.depth} vs {host.depth}"


# ---- GPU 3: two-level scenes on the forest route, the loop route and the host route --------------------------------
def three_routes(monkeypatch, top, verts, objects, placements, max_prims, **kw):
    """(forest-route aggregate, loop-route aggregate, host-route aggregate, host-route arrays), compared."""
    monkeypatch.delenv(LOOP, raising=False)
    dev, host, h = both_routes(top, verts, objects, placements, max_prims, "hlbvh", **kw)
    monkeypatch.setenv(LOOP, "1")
    loop = BVHAggregate.build_two_level_on_device(top, verts, objects, placements, max_prims, "hlbvh", **kw)
    monkeypatch.delenv(LOOP)
    what = f"max_prims {max_prims}"
    assert_same_scene(dev, host, what + " forest route")
    assert_same_scene(loop, host, what + " loop route")
    assert_same_scene(dev, loop, what + " forest against loop")
    return dev, loop, host, h


def close(*aggs):
    for a in aggs:
        a.close()


@functools.lru_cache(maxsize=None)
def many_small_objects():
    """200 objects of 1 .. 70 triangles, 400 placements (every object named at least once), 10 top-level triangles."""
    rng = np.random.default_rng(11)
    sizes = np.concatenate([[1, 2, 3, 4, 5, 64, 65, 70], rng.integers(1, 71, 192)])
    parts = [ss.random_soup(int(n), 0, 300 + k, extent=1.0, size=0.3) for k, n in enumerate(sizes)]
    parts.append(ss.random_soup(10, 0, 299, extent=30.0, size=2.0))
    verts, objects = join(parts)
    top = objects.pop()
    top["id"] += 100000
    pl = []
    for j in range(400):
        s = rng.uniform(0.5, 3.0)
        m = np.concatenate([np.eye(3) * s * rng.choice([-1.0, 1.0]), rng.uniform(-25, 25, (3, 1))], 1)
        pl.append(placement(j % 200 if j < 200 else int(rng.integers(0, 200)), m))
    return top, verts, objects, pl


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_two_level_hlbvh_forest_loop_and_host_routes_are_the_same_bytes(max_prims, monkeypatch):
    from test_gpu_parity import assert_hits_equal
    verts, pa, pb, pt, placements = ingredients(0, 60)
    dev, loop, host, h = three_routes(monkeypatch, pt, verts, [pa, pb], placements, max_prims)
    rays = trace_rays(verts, h["prims"], 0)[::3]
    got = dev.Intersect(rays)
    exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 16)
    assert (exp["instance"] > 0).sum() > 500
    assert_hits_equal(got, exp, "forest-built two-level closest (hlbvh)")
    assert (got["instance"] == exp["instance"]).all()
    assert got.tobytes() == loop.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    close(dev, loop, host)
    top, verts, objects, pl = many_small_objects()
    dev, loop, host, h = three_routes(monkeypatch, top, verts, objects, pl, max_prims)
    rays = scene.random_rays(4000, [-30, -30, -30], [30, 30, 30], 8)
    assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    close(dev, loop, host)


@pytest.mark.gpu
def test_two_level_hlbvh_animated_placements_and_attributes_on_all_three_routes(monkeypatch):
    """test_bvh_forest's scene of the same name (animated placements with the caller's motion bounds, a second object of
    alpha patches and smooth alpha triangles, normals, uvs and a per-primitive alpha array) with "hlbvh"."""
    from test_animated import animated_scene
    verts, prims, _, _, _, _, anims, oa, placements = animated_scene(4, 36)
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
    lo, hi = all_verts.min(0) - 40, all_verts.max(0) + 40  # generous motion bounds: any finite box serves the comparison
    bounds = np.zeros((len(entries), 6), np.float32)
    bounds[:len(placements)] = np.concatenate([lo, hi])
    alpha = rng.uniform(0.2, 1.0, len(entries)).astype(np.float32)
    dev, loop, host, h = three_routes(monkeypatch, prims[:0], all_verts, [prims, pb], pl, 4, animated=anims2,
                                      prim_bounds=bounds, prim_alpha=alpha, normals=normals, uvs=uvs)
    assert dev.read(2).tobytes() == loop.read(2).tobytes() == host.read(2).tobytes()
    rays = scene.random_rays(5000, [-25, -25, -25], [25, 25, 25], 5)
    rays["time"] = np.random.default_rng(6).uniform(-0.2, 1.2, len(rays)).astype(np.float32)
    assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    close(dev, loop, host)


# ---- GPU 4: refusals are the loop's ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def faulty_objects(nonfinite_at, lump_at):
    """Five objects over one vertex array; object `nonfinite_at` has a non-finite vertex, object `lump_at` is 65 536
    triangles that share one centroid, so one Morton code: a leaf larger than a node's 16-bit count."""
    parts = [ss.random_soup(n, 0, seed) for n, seed in ((40, 500), (500, 3), (7, 502), (500, 3), (90, 504))]
    v, p = parts[nonfinite_at]
    v = v.copy()
    v[p["v"][len(p) // 2, 1]] = np.inf
    parts[nonfinite_at] = (v, p)
    parts[lump_at] = ss.coincident_centroids(65536, 6)
    return join(parts)


def single_build_refusal(objects, verts):
    """(index, message) of the first object the single device build refuses, the message without the call's name."""
    for k, o in enumerate(objects):
        try:
            build_tree_gpu(o, verts, 4, split_method="hlbvh")
        except NNBVHError as e:
            return k, str(e).split(": ", 1)[1]
    pytest.fail("the single device build refuses none of the objects")


def good_builds():
    verts, objects = join([ss.random_soup(n, 0, 600 + n) for n in (3, 300, 65)])
    forest = build_hlbvh_forest_gpu(objects, verts)
    assert_forest_is_the_host_trees(forest, [build_tree(o, verts, 4, "hlbvh") for o in objects], "after a refusal")
    verts, pa, pb, pt, placements = ingredients(2, 20)
    dev, host, _ = both_routes(pt, verts, [pa, pb], placements, 4, "hlbvh")
    assert_same_scene(dev, host, "after a refusal")
    close(dev, host)


@pytest.mark.gpu
@pytest.mark.parametrize("nonfinite_at,lump_at,words", [(1, 3, "non-finite vertex"), (3, 1, "share one Morton code")])
def test_hlbvh_refusals_are_the_loops(nonfinite_at, lump_at, words, monkeypatch):
    verts, objects = faulty_objects(nonfinite_at, lump_at)
    k, text = single_build_refusal(objects, verts)
    assert k == 1 and words in text and "internal error" not in text
    with pytest.raises(NNBVHError) as e:
        build_hlbvh_forest_gpu(objects, verts)
    assert text in str(e.value) and "internal error" not in str(e.value)
    m = [[1, 0, 0, 2.0], [0, 1, 0, 0], [0, 0, 1, 0]]
    pl = [placement(j, m) for j in (0, 2, 4, 0)]
    for env in (None, "1"):
        if env is None:
            monkeypatch.delenv(LOOP, raising=False)
        else:
            monkeypatch.setenv(LOOP, env)
        with pytest.raises(NNBVHError) as e:
            BVHAggregate.build_two_level_on_device(objects[0][:0], verts, objects, pl, 4, "hlbvh")
        assert text in str(e.value) and "internal error" not in str(e.value), (env, str(e.value))
    monkeypatch.delenv(LOOP)
    good_builds()


@pytest.mark.gpu
def test_two_kinds_of_fault_in_one_object_are_reported_in_one_order(monkeypatch):
    """A bad vertex index and an unknown kind in one object: the single build, a forest of one and the loop route all
    name the vertex index, the first in the builders' fixed order of faults."""
    verts, prims = ss.random_soup(20, 0, 90)
    prims = prims.copy()
    prims["v"][3, 1] = len(verts)
    prims["kind"][11] = 99
    monkeypatch.setenv(LOOP, "1")
    for build in (lambda: build_tree_gpu(prims, verts, 4, split_method="hlbvh"),
                  lambda: build_hlbvh_forest_gpu([prims], verts),
                  lambda: BVHAggregate.build_two_level_on_device(prims[:0], verts, [prims], [placement(0, np.eye(4)[:3])],
                                                                 4, "hlbvh")):
        with pytest.raises(NNBVHError) as e:
            build()
        assert "vertex index out of range" in str(e.value) and "unknown primitive kind" not in str(e.value)
    monkeypatch.delenv(LOOP)
