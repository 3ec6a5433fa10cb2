"""The SAH trees of many objects built in ONE device pass (nnbvh_build_forest_create_gpu, build_forest_gpu) and the
two-level scene call that uses it (nnbvh_scene_create_instanced_gpu_build with NNBVH_SPLIT_SAH).

The yardstick is the host builder on each object alone (build_tree(obj, verts, max_prims, "sah")), byte for byte
(-0 is not +0), and for scenes the host route of test_two_level_device.  NNBVH_TWO_LEVEL_LOOP=1 keeps the
object-by-object loop reachable, so the forest route, the loop route and the host route are held side by side.

CPU: the argument faults, refused before a device is looked at.  GPU: every decision path of the SAH builder inside
one forest at every hand-over threshold, small and big neighbours sharing levels, tiles and scan ranges in both
orders, two-level scenes on all three routes, and the refusals a loop over the objects would have stopped at."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import BVHAggregate, NNBVHError, _lib, build_forest_gpu, build_tree, scene
from nn_bvh_amd._lib import PRIM_DTYPE, ptr
from test_bvh_build_paths import COSTS_TEXT, KNOB, PATH_CASES, path_scene
from test_two_level_device import (N_TOP_64, N_TOP_65, assert_same_scene, both_routes, deep_rays, deep_scene,
                                   deep_scene_with_a_deeper_unnamed_object, ingredients, placement, trace_rays)

LOOP = "NNBVH_TWO_LEVEL_LOOP"
SAH_SCENES = tuple(dict.fromkeys(p.values[1] for p in PATH_CASES if p.values[2] == "sah"))


# ---- forests over one vertex array ------------------------------------------------------------------------------
def shifted(prims, by):
    """prims with their vertex indices moved by `by` (the columns the kind reads: 4 for patches, else 3)."""
    out = prims.copy()
    out["v"][:, :3] += by
    quad = (out["kind"] == 1) | (out["kind"] >= 8)
    out["v"][quad, 3] += by
    return out


def join(parts):
    """[(verts, prims), ...] -> (one vertex array, [prims with shifted indices, ...])."""
    verts, objects, at = [], [], 0
    for v, p in parts:
        verts.append(np.asarray(v, np.float32))
        objects.append(shifted(p, at))
        at += len(v)
    return np.ascontiguousarray(np.concatenate(verts), np.float32), objects


def assert_forest_is_the_host_trees(forest, hosts, what):
    assert len(forest) == len(hosts), what
    counts = [len(h.nodes) for h in hosts]
    assert np.array_equal(forest.node_first, np.concatenate([[0], np.cumsum(counts)])), f"{what}: node_first"
    for k, (t, h) in enumerate(zip(forest, hosts)):
        w = f"{what}: object {k} ({len(h.ordered_prims)} primitives)"
        assert len(t.nodes) == len(h.nodes), f"{w}: {len(t.nodes)} vs {len(h.nodes)} nodes"
        assert t.ordered_prims.tobytes() == h.ordered_prims.tobytes(), f"{w}: ordered primitives differ"
        assert t.nodes.tobytes() == h.nodes.tobytes(), f"{w}: nodes differ"
        assert t.depth == h.depth, f"{w}: depth {t.depth} vs {h.depth}"


@functools.lru_cache(maxsize=None)
def path_forest():
    return join([path_scene(name)[:2] for name in SAH_SCENES])


@functools.lru_cache(maxsize=None)
def path_forest_hosts(max_prims):
    verts, objects = path_forest()
    return [build_tree(o, verts, max_prims, "sah") for o in objects]


SIZES = (1, 2, 3, 64, 65, 256, 257)


@functools.lru_cache(maxsize=None)
def neighbours():
    """301 objects: sizes cycling through SIZES (small and big ones side by side), one of 2049 and one of 4097 in the
    middle.  Only 3 soups per size: every geometry appears many times, at other places of the list and, every second
    time, moved to another position in space (a copy of its vertices, translated)."""
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
    return join(parts)


@functools.lru_cache(maxsize=None)
def neighbour_hosts(max_prims):
    verts, objects = neighbours()
    return [build_tree(o, verts, max_prims, "sah") for o in objects]


# ---- CPU -------------------------------------------------------------------------------------------------------
def raw_forest(L, prims, first, verts, bounds=None, max_prims=4, split=0, device=0, n_objects=None):
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    return L.nnbvh_build_forest_create_gpu(
        opt(prims), 0 if prims is None else len(prims), opt(first),
        (len(first) - 1 if first is not None else 0) if n_objects is None else n_objects, opt(verts),
        0 if verts is None else len(verts), opt(bounds), max_prims, split, device)


def test_forest_argument_faults_are_reported_before_any_device_call(nnbvh_lib):
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
    for split in (1, 2, 3, 7):
        refused("the forest build is SAH only", split=split)
    # NULL handles are argument errors, not crashes
    assert L.nnbvh_forest_nodes(None, None) is None and L.nnbvh_forest_n_levels(None) == -1
    assert L.nnbvh_forest_gpu_timing(None, None) == 1
    L.nnbvh_forest_destroy(None)


def test_build_forest_gpu_refuses_hlbvh_by_having_no_such_argument():
    import inspect
    assert "split_method" not in inspect.signature(build_forest_gpu).parameters


# ---- GPU 1: every decision path, inside a forest -----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, 2, 64, 1 << 30])
@pytest.mark.parametrize("max_prims", [1, 4, 255])
def test_every_decision_path_inside_one_forest(max_prims, knob, monkeypatch):
    verts, objects = path_forest()
    hosts = path_forest_hosts(max_prims)
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(knob))
    forest = build_forest_gpu(objects, verts, max_prims)
    assert_forest_is_the_host_trees(forest, hosts, f"max_prims {max_prims} {KNOB}={knob}")
    assert len(forest.gpu_ms) == 5 and forest.n_subtrees >= len(objects)
    if knob == 1 << 30:
        assert forest.n_levels == 0 and forest.n_subtrees == len(objects)
    if knob == 2:
        assert forest.n_levels > 0


# ---- GPU 2: neighbours do not leak -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_neighbours_do_not_leak_in_either_order(max_prims, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    verts, objects = neighbours()
    hosts = neighbour_hosts(max_prims)
    assert len(objects) == 301 and sorted({len(o) for o in objects}) == sorted(SIZES + (2049, 4097))
    forest = build_forest_gpu(objects, verts, max_prims)
    assert_forest_is_the_host_trees(forest, hosts, "in order")
    assert forest.n_levels >= 3  # 4097 -> ... -> 256: the big objects' levels are shared with the 257s' single one
    back = build_forest_gpu(objects[::-1], verts, max_prims)
    assert_forest_is_the_host_trees(back, hosts[::-1], "reversed")
    # the same geometry, wherever it stands in the list, gives the same tree
    seen = {}
    for o, t in zip(objects, forest):
        key = (len(o), verts[o["v"][:, :3]].tobytes())
        assert seen.setdefault(key, t.nodes.tobytes()) == t.nodes.tobytes()
    assert len(seen) < len(objects)
    # nothing above the hand-over: no breadth-first pass at all, one wavefront per object
    keep = [k for k, o in enumerate(objects) if len(o) <= 256]
    small = build_forest_gpu([objects[k] for k in keep], verts, max_prims)
    assert_forest_is_the_host_trees(small, [hosts[k] for k in keep], "small objects only")
    assert small.n_levels == 0 and small.n_subtrees == len(keep) > 250


# ---- GPU 3: two-level scenes on the forest route, the loop route and the host route --------------------------------
def three_routes(monkeypatch, top, verts, objects, placements, max_prims, **kw):
    """(forest-route aggregate, loop-route aggregate, host-route aggregate, host-route arrays), compared."""
    monkeypatch.delenv(LOOP, raising=False)
    dev, host, h = both_routes(top, verts, objects, placements, max_prims, "sah", **kw)
    monkeypatch.setenv(LOOP, "1")
    loop = BVHAggregate.build_two_level_on_device(top, verts, objects, placements, max_prims, "sah", **kw)
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
def test_two_level_forest_loop_and_host_routes_are_the_same_bytes(max_prims, monkeypatch):
    from test_gpu_parity import assert_hits_equal
    verts, pa, pb, pt, placements = ingredients(0, 60)
    dev, loop, host, h = three_routes(monkeypatch, pt, verts, [pa, pb], placements, max_prims)
    rays = trace_rays(verts, h["prims"], 0)
    got = dev.Intersect(rays)
    exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 16)
    assert (exp["instance"] > 0).sum() > 500
    assert_hits_equal(got, exp, "forest-built two-level closest")
    assert (got["instance"] == exp["instance"]).all()
    assert got.tobytes() == loop.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    close(dev, loop, host)
    top, verts, objects, pl = many_small_objects()
    dev, loop, host, h = three_routes(monkeypatch, top, verts, objects, pl, max_prims)
    rays = scene.random_rays(4000, [-30, -30, -30], [30, 30, 30], 8)
    assert dev.Intersect(rays).tobytes() == host.Intersect(rays).tobytes()
    close(dev, loop, host)


@pytest.mark.gpu
def test_two_level_depth_64_is_accepted_and_65_refused_on_both_device_routes(monkeypatch):
    from test_gpu_parity import assert_hits_equal
    for make in (deep_scene, deep_scene_with_a_deeper_unnamed_object):
        top, verts, objects, placements = make(N_TOP_64)
        dev, loop, host, h = three_routes(monkeypatch, top, verts, objects, placements, 1)
        assert dev.info["depth"] == 64 == h["top_depth"] + h["child_depth"] + 1
        rays = deep_rays(top, verts, objects)
        exp = ob.closest_inst(h["nodes"], h["prims"], verts, h["instances"], rays, 8)
        assert_hits_equal(dev.Intersect(rays), exp, "depth 64, forest route")
        close(dev, loop, host)
        top, verts, objects, placements = make(N_TOP_65)
        for env in (None, "1"):
            if env is None:
                monkeypatch.delenv(LOOP, raising=False)
            else:
                monkeypatch.setenv(LOOP, env)
            with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
                BVHAggregate.build_two_level_on_device(top, verts, objects, placements, 1, "sah")
        monkeypatch.delenv(LOOP)


@pytest.mark.gpu
def test_two_level_animated_placements_and_attributes_on_all_three_routes(monkeypatch):
    """The scene of test_two_level_device's animated test: animated placements with the caller's motion bounds, a
    second object of alpha patches and smooth alpha triangles, normals, uvs and a per-primitive alpha array."""
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
def faulty_objects(nonfinite_at, huge_at):
    """Five soups over one vertex array; object `nonfinite_at` has a non-finite vertex, object `huge_at` coordinates
    for which every SAH cost is infinite."""
    parts = [ss.random_soup(n, 0, seed) for n, seed in ((40, 500), (500, 3), (7, 502), (500, 3), (90, 504))]
    v, p = parts[nonfinite_at]
    v = v.copy()
    v[p["v"][len(p) // 2, 1]] = np.inf
    parts[nonfinite_at] = (v, p)
    v, p = parts[huge_at]
    parts[huge_at] = ((v * np.float32(1e17)).astype(np.float32), p)
    return join(parts)


def good_forest_builds():
    verts, objects = join([ss.random_soup(n, 0, 600 + n) for n in (3, 300, 65)])
    forest = build_forest_gpu(objects, verts)
    assert_forest_is_the_host_trees(forest, [build_tree(o, verts, 4, "sah") for o in objects], "after a refusal")


@pytest.mark.gpu
@pytest.mark.parametrize("knob", [None, 2, 1 << 30])
def test_a_forest_reports_the_lowest_numbered_failing_object(knob, monkeypatch):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, str(knob))
    for nonfinite_at, huge_at, words in ((1, 3, "non-finite vertex"), (3, 1, COSTS_TEXT)):
        verts, objects = faulty_objects(nonfinite_at, huge_at)
        # what the loop of single builds stops at
        for k, o in enumerate(objects):
            try:
                build_tree(o, verts, 4, "sah")
            except NNBVHError as e:
                assert k == 1 and words in str(e)
                break
        else:
            pytest.fail("the host builder refuses none of the objects")
        with pytest.raises(NNBVHError, match=words) as e:
            build_forest_gpu(objects, verts)
        assert "internal error" not in str(e.value)
        good_forest_builds()


@pytest.mark.gpu
def test_a_two_level_scene_reports_the_lowest_numbered_failing_object(monkeypatch):
    m = [[1, 0, 0, 2.0], [0, 1, 0, 0], [0, 0, 1, 0]]
    for nonfinite_at, huge_at, words in ((1, 3, "non-finite vertex"), (3, 1, COSTS_TEXT)):
        verts, objects = faulty_objects(nonfinite_at, huge_at)
        pl = [placement(k, m) for k in (0, 2, 4, 0)]
        for env in (None, "1"):
            if env is None:
                monkeypatch.delenv(LOOP, raising=False)
            else:
                monkeypatch.setenv(LOOP, env)
            with pytest.raises(NNBVHError, match=words):
                BVHAggregate.build_two_level_on_device(objects[0][:0], verts, objects, pl, 4, "sah")
        monkeypatch.delenv(LOOP)
        good_forest_builds()
        verts, pa, pb, pt, placements = ingredients(2, 20)
        dev, host, _ = both_routes(pt, verts, [pa, pb], placements, 4, "sah")
        assert_same_scene(dev, host, "after a refusal")
        close(dev, host)
