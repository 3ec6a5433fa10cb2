"""KdTreeAggregate construction (cpu/aggregates.cpp:798-971): what the order of EQUAL (t, type) edges can and
cannot change (CPU: the host builder with libstdc++'s std::sort against the same builder with
std::stable_sort), and the device builder against the host one byte for byte (GPU).

Every decision path of buildTree has a scene of its own (PATH_CASES).  A census of the HOST-built tree (census(),
pure numpy) proves on the CPU that the scene reaches its path; the GPU tests then compare the device builder with
the host one byte for byte on exactly those cases, and trace rays through some of the device-built trees."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import NNBVHError, scene
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree, prim_bounds_of


def leaves_of(tree):
    """[(node index, sorted primitive ids)] of every leaf, in node order."""
    nodes, idx = tree.nodes, tree.prim_indices
    out = []
    for i in np.nonzero((nodes["flags"] & 3) == 3)[0]:
        n = int(nodes["flags"][i] >> 2)
        v = int(nodes["split_or_index"][i])
        out.append((int(i), sorted([v] if n == 1 else idx[v:v + n].tolist() if n else [])))
    return out


def scenes():
    yield "soup", ss.random_soup(3000, 0, 5)
    yield "soup+patches", ss.random_soup(1500, 300, 6)
    v, p = ss.grid_mesh(40, 7, bump=0.3)          # a connected mesh: shared vertices = many equal edges
    yield "mesh", (v, p)
    v, p = ss.coincident_centroids(120, 8)        # many identical bounds: leaves the depth limit closes
    yield "coincident", (v, p)
    vs = np.round(ss.random_soup(2500, 0, 9, extent=4.0, size=0.8)[0] * 4) / 4   # snapped to a grid
    yield "snapped", (vs.astype(np.float32), ss.random_soup(2500, 0, 9, extent=4.0, size=0.8)[1])


@pytest.mark.parametrize("max_prims", [1, 4])
def test_tie_order_changes_nothing_but_the_order_inside_leaves(max_prims):
    """aggregates.cpp:899-903 sorts with std::sort: the order among equal edges is the standard library's.
    Whatever it is, the node array (split planes, child links, leaf sizes, primitiveIndices offsets) and the
    SET of primitives of every leaf are the same."""
    some_differ = False
    for name, (verts, prims) in scenes():
        a = build_kd_tree(prims, verts, max_prims=max_prims)
        b = build_kd_tree(prims, verts, max_prims=max_prims, where="host_stable")
        leaf = (a.nodes["flags"] & 3) == 3
        multi = leaf & ((a.nodes["flags"] >> 2) > 1)
        assert a.nodes["flags"].tobytes() == b.nodes["flags"].tobytes(), name
        # split planes: equal as floats (a tie between a -0 and a +0 edge may hand either zero to the node);
        # multi-primitive leaves: the same primitiveIndices offsets; one-primitive leaves: compared as sets below
        assert np.array_equal(a.nodes["split_or_index"][~leaf].view(np.float32), b.nodes["split_or_index"][~leaf].view(np.float32)), name
        assert a.nodes["split_or_index"][multi].tobytes() == b.nodes["split_or_index"][multi].tobytes(), name
        assert len(a.prim_indices) == len(b.prim_indices) and a.depth == b.depth
        assert leaves_of(a) == leaves_of(b), name
        some_differ |= a.prim_indices.tobytes() != b.prim_indices.tobytes()
    assert some_differ or max_prims == 1  # the two orders do differ somewhere (else this test shows nothing)


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims,max_depth", [(1, -1), (4, -1), (1, 6), (2, 3)])
def test_device_kd_build_equals_the_host_builder(max_prims, max_depth):
    import torch
    # the build runs on the last device: on a machine with several, not the one that is current
    device, before = torch.cuda.device_count() - 1, torch.cuda.current_device()
    for name, (verts, prims) in scenes():
        h = build_kd_tree(prims, verts, max_prims=max_prims, max_depth=max_depth, where="host_stable")
        g = build_kd_tree(prims, verts, max_prims=max_prims, max_depth=max_depth, where="gpu", device=device)
        assert torch.cuda.current_device() == before, f"{name}: the build left device {torch.cuda.current_device()} current"
        assert g.nodes.tobytes() == h.nodes.tobytes(), f"{name}: node arrays differ"
        assert g.prim_indices.tobytes() == h.prim_indices.tobytes(), f"{name}: primitiveIndices differ"
        assert g.depth == h.depth and np.array_equal(g.bounds, h.bounds)


@pytest.mark.gpu
def test_device_kd_build_other_costs_and_host_primitives():
    verts, prims = ss.random_soup(2000, 100, 21)
    pb = np.zeros((len(prims), 6), np.float32)
    prims = prims.copy()
    host = np.arange(0, len(prims), 37)
    for i in host:   # a few host-only primitives with caller bounds
        c = np.random.default_rng(int(i)).uniform(-3, 3, 3).astype(np.float32)
        pb[i] = np.concatenate([c - 0.3, c + 0.3])
        prims["kind"][i] = 3
    for kw in (dict(isect_cost=80, traversal_cost=1, empty_bonus=0.2), dict(isect_cost=1, traversal_cost=4, empty_bonus=0.0),
               dict(max_prims=8)):
        h = build_kd_tree(prims, verts, prim_bounds=pb, where="host_stable", **kw)
        g = build_kd_tree(prims, verts, prim_bounds=pb, where="gpu", **kw)
        assert g.nodes.tobytes() == h.nodes.tobytes() and g.prim_indices.tobytes() == h.prim_indices.tobytes(), kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["killeroos", "bathroom"])
def test_device_kd_build_on_scene_blobs(name):
    blob = ss.scene_blob(name)
    if blob is None:
        pytest.skip(f"data/{name}.npz not present")
    verts, tris = blob
    prims = ss.make_prims(tris)
    h = build_kd_tree(prims, verts, where="host_stable")
    g = build_kd_tree(prims, verts, where="gpu")
    assert g.nodes.tobytes() == h.nodes.tobytes() and g.prim_indices.tobytes() == h.prim_indices.tobytes()
    print(f"{name}: {len(g.nodes)} nodes, {len(g.prim_indices)} indices, depth {g.depth}; device build "
          f"{g.build_ms[0]:.1f} ms (+ download {g.build_ms[1] - g.build_ms[0]:.1f} ms)")


# ---- a census of the tree: which decisions of buildTree (aggregates.cpp:852-971) it holds ---------------------------
CENSUS_KEYS = ("interior", "attempt0", "attempt1", "attempt2", "levels_with_all_attempts", "zero_splits",
               "zero_splits_signed", "leaves", "empty_leaves", "levels_of_empty_leaves_only", "depth_closed",
               "no_valid_edge", "nan_cost", "refused_16_or_more", "refused_below_16", "zero_area_leaves",
               "zero_area_over_max_prims", "multi_prim_leaves", "interior_between_multi_prim_leaves", "depth")


def census(nodes, prim_indices, bounds, max_prims, max_depth, prim_bounds):
    """Walk the node array depth first (below child at i + 1, above child at flags >> 2) with every node's float32
    box (child boxes: pMax[axis] / pMin[axis] = the split, :963-964) and depth, and count

    attempt0 / 1 / 2   interior nodes whose axis is MaxDimension(box), that + 1 mod 3, that + 2 mod 3 (:883, :937-941)
    levels_with_all_attempts   depths that hold interior nodes of all three kinds
    zero_splits (_signed)      interior nodes whose split is +-0 (with the sign bit)
    empty_leaves               leaves of no primitive; levels_of_empty_leaves_only: depths holding nothing else
    depth_closed               leaves of more than max_prims primitives at depth == max_depth (:872)
    leaves of more than max_prims primitives ABOVE the depth limit, by the rule of :944-950 that closed them:
      no_valid_edge            no bound edge of its primitives lies strictly inside its box on any axis (bestAxis == -1)
      nan_cost                 an edge does, but the box has no surface area: every cost is 0 * inf = NaN and never wins
      refused_16_or_more       an edge does, area > 0, n >= 16: only badRefines == 3 closes such a leaf
      refused_below_16         the same with n < 16: badRefines == 3 or bestCost > 4 leafCost
    zero_area_leaves (_over_max_prims), multi_prim_leaves, and interior nodes BOTH of whose sub-trees hold a
    multi-primitive leaf (the primitiveIndices offset of the above sub-tree is then a sum over the below one).
    prim_bounds: (n, 6) float32, min xyz max xyz.  max_depth <= 0: the reference's default, :808-809."""
    f32 = np.float32
    pb = np.asarray(prim_bounds, f32).reshape(-1, 6)
    if max_depth <= 0:
        max_depth = int(np.round(8 + f32(1.3) * f32(int(np.log2(len(pb))))))
    flags, word = nodes["flags"], nodes["split_or_index"]
    c = dict.fromkeys(CENSUS_KEYS, 0)
    kinds_at, all_empty_at, has_multi = {}, {}, {}
    stack = [(0, np.asarray(bounds, f32).copy(), 0)]
    order = []
    while stack:
        i, box, depth = stack.pop()
        order.append(i)
        c["depth"] = max(c["depth"], depth)
        fl = int(flags[i])
        d = box[3:] - box[:3]
        area = f32(2) * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2])
        if fl & 3 != 3:
            split = word[i:i + 1].view(f32)[0]
            axis = fl & 3
            longest = 0 if (d[0] > d[1] and d[0] > d[2]) else (1 if d[1] > d[2] else 2)
            k = (axis - longest) % 3
            c["interior"] += 1
            c[f"attempt{k}"] += 1
            kinds_at.setdefault(depth, set()).add(k)
            all_empty_at[depth] = False
            if split == 0:
                c["zero_splits"] += 1
                c["zero_splits_signed"] += int(np.signbit(split))
            assert box[axis] < split < box[3 + axis], f"node {i}: split {split} not strictly inside its box"
            lo_box, hi_box = box.copy(), box.copy()
            lo_box[3 + axis] = split
            hi_box[axis] = split
            stack.append((fl >> 2, hi_box, depth + 1))
            stack.append((i + 1, lo_box, depth + 1))
            continue
        n = fl >> 2
        c["leaves"] += 1
        c["empty_leaves"] += n == 0
        all_empty_at[depth] = all_empty_at.get(depth, True) and n == 0
        c["multi_prim_leaves"] += n > 1
        has_multi[i] = n > 1
        c["zero_area_leaves"] += area == 0
        if n <= max_prims:
            continue
        c["zero_area_over_max_prims"] += area == 0
        if depth == max_depth:
            c["depth_closed"] += 1
            continue
        assert depth < max_depth, f"leaf {i} below the depth limit"
        v = int(word[i])
        e = pb[prim_indices[v:v + n] if n > 1 else [v]]
        edges = np.concatenate([e[:, :3], e[:, 3:]])
        if not ((edges > box[:3]) & (edges < box[3:])).any():
            c["no_valid_edge"] += 1
        elif area == 0:
            c["nan_cost"] += 1
        else:
            c["refused_16_or_more" if n >= 16 else "refused_below_16"] += 1
    c["levels_with_all_attempts"] = sum(k == {0, 1, 2} for k in kinds_at.values())
    c["levels_of_empty_leaves_only"] = sum(bool(v) for v in all_empty_at.values())
    for i in reversed(order):  # depth-first pre-order reversed: children before their parent
        if int(flags[i]) & 3 != 3:
            below, above = has_multi[i + 1], has_multi[int(flags[i]) >> 2]
            c["interior_between_multi_prim_leaves"] += below and above
            has_multi[i] = below or above
    assert len(order) == len(nodes)
    return {k: int(v) for k, v in c.items()}


# ---- the cases: scene, builder parameters, the census lines that must not be zero ------------------------------------
@functools.lru_cache(maxsize=None)
def path_scene(name):
    """(verts, prims, caller bounds or None) of a scene, built once per session and never modified."""
    made = {
        "sticks": lambda: ss.kd_sticks(31),
        "signed_zeros": lambda: ss.kd_signed_zeros(32),
        "lattice": lambda: ss.kd_lattice(256, 3, 2),
        "cluster_lattice": lambda: ss.kd_cluster_lattice(33),
        "overlap24": lambda: ss.kd_overlap_clusters(34, 6, 24),
        "overlap8_alone": lambda: ss.kd_overlap_clusters(35, 1, 8),
        "overlap16_alone": lambda: ss.kd_overlap_clusters(35, 1, 16),
        "identical_boxes": lambda: ss.kd_identical_boxes(36),
        "flat": lambda: ss.kd_flat(800, 37),
        "line": lambda: ss.kd_line(60, 38),
        "point": lambda: ss.kd_line(60, 39, point=True),
        "flat_mix": lambda: ss.kd_flat_mix(40),
        "two_clusters": lambda: ss.kd_two_clusters(41),
        "soup1": lambda: ss.random_soup(1, 0, 21),
        "soup2": lambda: ss.random_soup(2, 0, 22),
        "soup3": lambda: ss.random_soup(3, 0, 23),
        "soup5": lambda: ss.random_soup(5, 0, 25),
        "soup7": lambda: ss.random_soup(7, 0, 27),
        "soup600": lambda: ss.random_soup(600, 0, 28),
        "chain64": lambda: (lambda ch: (ch.verts, ch.prims))(ss.kd_chain(64, 1)),
    }[name]()
    for a in made:
        a.setflags(write=False)
    return made if len(made) == 3 else made + (None,)


def _case(family, scene_name, premise, max_prims=(1, 4), **kw):
    return [pytest.param(family, scene_name, dict(kw, max_prims=m), premise,
                         id="-".join([scene_name] + [f"{k}={v}" for k, v in dict(kw, max_prims=m).items()]))
            for m in max_prims]


# premise: census keys that must be > 0 (a "=N" suffix: must equal N).  The premises are the issue's; parameters and
# generators were tuned until they hold, never the other way round.
PATH_CASES = (
    # retries on the other axes: children of attempt 1 / 2 segments land behind those of attempt 0 on the same level
    _case("sticks", "sticks", ("attempt0", "attempt1", "attempt2", "levels_with_all_attempts"))
    # -0 / +0 edges: the chosen edge's own sign goes into the node and both child boxes
    + _case("signed_zeros", "signed_zeros", ("zero_splits", "zero_splits_signed", "zero_splits_unsigned"))
    # equal costs: the first minimum wins, inside a wavefront, across wavefronts, in segments that share one
    + _case("equal_costs", "lattice", ("interior",))
    + _case("equal_costs", "lattice", ("interior",), isect_cost=0)
    + _case("equal_costs", "lattice", ("interior",), isect_cost=0, traversal_cost=0)
    + _case("equal_costs", "cluster_lattice", ("interior",))
    + _case("equal_costs", "cluster_lattice", ("interior",), isect_cost=0)
    + _case("equal_costs", "cluster_lattice", ("interior",), isect_cost=0, traversal_cost=0)
    # refusals: (a) badRefines == 3, (b) the root refused by bestCost > 4 leafCost with n < 16 (and not with n = 16),
    # (c) no valid edge above the depth limit
    + _case("refusals", "overlap24", ("refused_16_or_more",), max_prims=(1,))
    + _case("refusals", "overlap24", ("interior",), max_prims=(4,))
    + _case("refusals", "overlap8_alone", ("refused_below_16=1", "interior=0"), isect_cost=1, traversal_cost=64)
    + _case("refusals", "overlap16_alone", ("interior",), isect_cost=1, traversal_cost=64)
    + _case("refusals", "identical_boxes", ("no_valid_edge",))
    # flat and degenerate: one zero extent (finite costs); no surface area (NaN costs never win, or no edge at all)
    + _case("flat", "flat", ("interior", "zero_area_leaves=0"))
    + _case("flat", "line", ("nan_cost=1", "zero_area_over_max_prims=1", "interior=0"))
    + _case("flat", "point", ("no_valid_edge=1", "zero_area_over_max_prims=1", "interior=0"))
    + _case("flat", "flat_mix", ("interior", "multi_prim_leaves"))
    # empty space: zero-count segments with and without the bonus that favours them
    + _case("empty_space", "two_clusters", ("empty_leaves",), empty_bonus=0.5)
    + _case("empty_space", "two_clusters", ("interior",), empty_bonus=0.0)
    # tiny inputs, the root as a multi-primitive leaf, depth limits
    + _case("tiny", "soup1", ("interior=0", "leaves=1"))
    + _case("tiny", "soup2", ("leaves",))
    + _case("tiny", "soup3", ("leaves",))
    + _case("tiny", "soup5", ("leaves",))
    + _case("tiny", "soup7", ("interior=0", "multi_prim_leaves=1"), max_prims=(7, 8))
    + _case("tiny", "soup600", ("depth=1", "depth_closed"), max_depth=1)
    + _case("tiny", "chain64", ("depth=64", "depth_closed", "empty_leaves"), max_depth=64, isect_cost=0, traversal_cost=0)
    + _case("tiny", "chain64", ("interior",), max_depth=64)
    # the layout pass: multi-primitive leaves on both sides of many interior nodes
    + _case("layout", "soup600", ("interior_between_multi_prim_leaves",), max_prims=(4, 8))
)
FAMILIES = sorted({p.values[0] for p in PATH_CASES})
TRACED = ("sticks", "refusals", "flat")


def bounds_of(name):
    verts, prims, pb = path_scene(name)
    return pb if pb is not None else np.concatenate(prim_bounds_of(prims, verts), 1)


@functools.lru_cache(maxsize=None)
def host_tree(name, kw_items):
    verts, prims, pb = path_scene(name)
    return build_kd_tree(prims, verts, prim_bounds=pb, where="host_stable", **dict(kw_items))


def census_of(name, kw):
    t = host_tree(name, tuple(sorted(kw.items())))
    c = census(t.nodes, t.prim_indices, t.bounds, kw["max_prims"], kw.get("max_depth", -1), bounds_of(name))
    c["zero_splits_unsigned"] = c["zero_splits"] - c["zero_splits_signed"]
    assert c["depth"] == t.depth, f"{name}: the builder reports depth {t.depth}, the walk finds {c['depth']}"
    return t, c


@pytest.mark.parametrize("family", FAMILIES)
def test_census_every_scene_reaches_the_path_it_is_named_for(family):
    """The host builder's tree of every case of the family holds what the case is there for (no GPU)."""
    for p in PATH_CASES:
        fam, name, kw, premise = p.values
        if fam != family:
            continue
        _, c = census_of(name, kw)
        print(f"{p.id}: " + " ".join(f"{k}={v}" for k, v in c.items() if v))
        for want in premise:
            key, _, exact = want.partition("=")
            assert (c[key] == int(exact)) if exact else (c[key] > 0), f"{p.id}: census {want} does not hold: {c}"


def test_census_counts_a_hand_made_tree():
    """The census itself on a tree small enough to count by hand.  The root splits x at 2: attempt 0 of the box
    [0, 4] x [0, 1] x [0, 1].  Below it a leaf of two primitives whose box holds one of their edges (x = 1): refused,
    n < 16.  Above it a split of z at 0.5, attempt 2 of [2, 4] x [0, 1] x [0, 1] where x is the longest axis, into an
    empty leaf and a one-primitive leaf."""
    from nn_bvh_amd._lib import KD_NODE_DTYPE
    nodes = np.zeros(5, KD_NODE_DTYPE)
    f = lambda x: np.array([x], np.float32).view(np.uint32)[0]  # noqa: E731
    nodes[0] = (f(2.0), 0 | (2 << 2))
    nodes[1] = (0, 3 | (2 << 2))          # primitives idx[0:2] = 0, 1
    nodes[2] = (f(0.5), 2 | (4 << 2))
    nodes[3] = (0, 3 | (0 << 2))
    nodes[4] = (2, 3 | (1 << 2))
    pb = np.array([[0, 0, 0, 1, 1, 1], [1, 0, 0, 2, 1, 1], [2, 0, 0.5, 4, 1, 1]], np.float32)
    c = census(nodes, np.array([0, 1], np.int32), np.array([0, 0, 0, 4, 1, 1], np.float32), 1, 8, pb)
    want = dict.fromkeys(CENSUS_KEYS, 0)
    want.update(interior=2, attempt0=1, attempt2=1, leaves=3, empty_leaves=1, refused_below_16=1, multi_prim_leaves=1,
                depth=2)
    assert c == want


def test_max_depth_65_is_refused_by_both_builders():
    verts, prims, _ = path_scene("soup7")
    for where in ("host", "host_stable", "gpu"):
        with pytest.raises(NNBVHError, match="max_depth above the traversal stack"):
            build_kd_tree(prims, verts, max_depth=65, where=where)


# ---- GPU: the device builder on every case ---------------------------------------------------------------------------
def first_difference(g, h):
    """Where two trees first differ, for a failure message."""
    if len(g.nodes) != len(h.nodes):
        return f"{len(g.nodes)} nodes against {len(h.nodes)}"
    bad = np.nonzero((g.nodes["flags"] != h.nodes["flags"]) | (g.nodes["split_or_index"] != h.nodes["split_or_index"]))[0]
    if len(bad):
        i = int(bad[0])
        return (f"first differing node {i}: device (word {int(g.nodes['split_or_index'][i]):#010x}, flags "
                f"{int(g.nodes['flags'][i]):#x}) host (word {int(h.nodes['split_or_index'][i]):#010x}, flags "
                f"{int(h.nodes['flags'][i]):#x})")
    if len(g.prim_indices) != len(h.prim_indices):
        return f"{len(g.prim_indices)} primitiveIndices against {len(h.prim_indices)}"
    bad = np.nonzero(g.prim_indices != h.prim_indices)[0]
    return f"first differing primitiveIndices entry {int(bad[0])}" if len(bad) else "no difference"


@pytest.mark.gpu
@pytest.mark.parametrize("family,name,kw,premise", PATH_CASES)
def test_device_kd_build_equals_the_host_builder_on_every_path(family, name, kw, premise):
    """Byte for byte (split planes included: -0 is not +0 here), twice (the atomics and the three-attempt loop are
    deterministic); for sticks, refusals and flat scenes the device-built tree also carries rays to the oracle's
    answers."""
    verts, prims, pb = path_scene(name)
    h = host_tree(name, tuple(sorted(kw.items())))
    g = build_kd_tree(prims, verts, prim_bounds=pb, where="gpu", **kw)
    g2 = build_kd_tree(prims, verts, prim_bounds=pb, where="gpu", **kw)
    what = f"{name} {kw}"
    assert g.nodes.tobytes() == h.nodes.tobytes(), f"{what}: node arrays differ, {first_difference(g, h)}"
    assert g.prim_indices.tobytes() == h.prim_indices.tobytes(), f"{what}: primitiveIndices differ, {first_difference(g, h)}"
    assert g.depth == h.depth, f"{what}: depth {g.depth} against {h.depth}"
    assert g.bounds.tobytes() == h.bounds.tobytes(), f"{what}: bounds differ"
    assert g2.nodes.tobytes() == g.nodes.tobytes() and g2.prim_indices.tobytes() == g.prim_indices.tobytes() \
        and g2.depth == g.depth, f"{what}: two device builds differ, {first_difference(g2, g)}"
    if family not in TRACED:
        return
    lo, hi = verts.min(0), verts.max(0)
    pad = 0.1 * (hi - lo) + 1
    rays = np.concatenate([scene.random_rays(3000, lo - pad, hi + pad, 51), scene.random_rays(1000, lo, hi, 52, tmax=0.5),
                           ss.edge_case_rays(verts, prims, 53, n=1024)])
    agg = KdTreeAggregate.from_tree(g.nodes, g.prim_indices, prims, verts, g.bounds)
    try:
        got = agg.Intersect(rays)
        occ, vis, tst = agg.IntersectP(rays, counts=True)
    finally:
        agg.close()
    exp = ob.kd_closest(h.nodes, h.prim_indices, prims, verts, h.bounds, rays, 4)
    eo, ev, et = ob.kd_any_hit(h.nodes, h.prim_indices, prims, verts, h.bounds, rays, 4)
    assert got.tobytes() == exp.tobytes(), f"{what}: closest-hit records differ from the oracle on the host-built tree"
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et), f"{what}: any-hit differs"
