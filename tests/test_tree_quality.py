"""GPU tests of nnbvh_tree_quality_create against the brute-force oracle (tests/tree_quality_oracle.py).
In every case the per-primitive counts, the per-node counts and the two pair totals are compared as exact integers, the
eight doubles within the derived tolerance (2 n + 16) 2^-53 (n: primitives for the EPO sums, nodes for the SAH sums; NaN
and inf by class), and a second call must return identical bytes."""
import numpy as np
import pytest

import scenes_small as ss
import tree_quality_oracle as tq
from nn_bvh_amd import NNBVHError, build_tree, build_tree_gpu, make_prims, nn_tree, tree_quality

pytestmark = pytest.mark.gpu

BUILDERS = ("sah", "hlbvh", "middle", "equal", "nn")


def _tree(prims, verts, builder, leaf=4):
    if builder == "nn":
        return nn_tree.greedy_sah_tree(verts, prims["v"][:, :3], levels=4, max_prims_in_node=leaf)[0]
    t = build_tree(prims, verts, leaf, builder)
    return t.nodes, t.ordered_prims


def _check(nodes, ordered, verts, oracle=None, **constants):
    o = oracle if oracle is not None else tq.tree_quality(nodes, ordered, verts, **constants)
    q = tree_quality(nodes, ordered, verts, per_primitive=True, per_node=True, **constants)
    again = tree_quality(nodes, ordered, verts, per_primitive=True, per_node=True, **constants)
    assert (q.prim_ext_inner == o["prim_ext_inner"]).all()
    assert (q.prim_ext_leaf == o["prim_ext_leaf"]).all()
    assert (q.node_external == o["node_external"]).all()
    for k in ("ext_pairs_inner", "ext_pairs_leaf", "n_inner", "n_leaves", "depth"):
        assert getattr(q, k) == o[k], k
    bad = tq.mismatched_doubles(q, o, len(nodes), len(ordered))
    assert not bad, bad
    assert q.raw == again.raw
    assert q.prim_ext_inner.tobytes() == again.prim_ext_inner.tobytes()
    assert q.prim_ext_leaf.tobytes() == again.prim_ext_leaf.tobytes()
    assert q.node_external.tobytes() == again.node_external.tobytes()
    return q, o


# 1. lane and wave edges
@pytest.mark.parametrize("leaf", (1, 4, 255))
@pytest.mark.parametrize("n", (1, 2, 3, 63, 64, 65, 257, 1025))
def test_lane_and_wave_edges(n, leaf):
    verts, prims = ss.random_soup(n, seed=n, extent=3.0)
    nodes, ordered = _tree(prims, verts, "sah", leaf)
    q, o = _check(nodes, ordered, verts)
    if n == 1 or leaf == 255 and n <= 255:
        assert len(nodes) > 1 or (q.epo == 0.0 and q.n_leaves == 1 and q.n_inner == 0 and q.depth == 0)
    if n == 1:  # the root is a leaf: sah = c_leaf * nprims * A / A, no externals
        assert len(nodes) == 1 and q.sah == 1.0


def test_outputs_are_optional():
    verts, prims = ss.random_soup(65, seed=2, extent=3.0)
    nodes, ordered = _tree(prims, verts, "sah")
    q = tree_quality(nodes, ordered, verts)
    full = tree_quality(nodes, ordered, verts, per_primitive=True, per_node=True)
    assert q.prim_ext_inner is None and q.node_external is None and q.raw == full.raw
    assert set(q.gpu_ms) == {"prepare", "walk", "reduce", "total"} and all(v >= 0 for v in q.gpu_ms.values())


# 2. all five builders, and the device builders' byte-identical trees
@pytest.fixture(scope="module", params=("soup", "grid"))
def builder_scene(request):
    return ss.random_soup(1500) if request.param == "soup" else ss.grid_mesh(24)


@pytest.mark.parametrize("builder", BUILDERS)
def test_every_builder(builder_scene, builder):
    verts, prims = builder_scene
    nodes, ordered = _tree(prims, verts, builder)
    q, o = _check(nodes, ordered, verts)
    assert o["ext_pairs_inner"] > 0 and o["ext_pairs_leaf"] > 0


@pytest.mark.parametrize("method", ("sah", "hlbvh"))
def test_device_built_tree_scores_identically(builder_scene, method):
    verts, prims = builder_scene
    host = build_tree(prims, verts, 4, method)
    dev = build_tree_gpu(prims, verts, 4, split_method=method)
    assert dev.nodes.tobytes() == host.nodes.tobytes() and dev.ordered_prims.tobytes() == host.ordered_prims.tobytes()
    q, _ = _check(dev.nodes, dev.ordered_prims, verts)
    assert q.raw == tree_quality(host.nodes, host.ordered_prims, verts).raw


# 3. closed intervals and zeros
ZERO_SCENES = {"grid": lambda: ss.grid_mesh(16), "zero_cluster": lambda: ss.bvh_signed_zero_cluster(300),
               "zero_row": ss.bvh_signed_zero_row,
               # the row's unit boxes at half their pitch: neighbours overlap, and whether a vertex at +-0 lies in a
               # neighbour's box that starts at -+0 is decided by 0 == -0 alone (the row as it is has no externals)
               "zero_row_overlapping": lambda: ss.bvh_signed_zero_row(96, pitch=0.5)}


@pytest.mark.parametrize("scene", sorted(ZERO_SCENES))
def test_closed_intervals_and_signed_zeros(scene):
    verts, prims = ZERO_SCENES[scene]()
    nodes, ordered = _tree(prims, verts, "sah", 2)
    q, o = _check(nodes, ordered, verts)
    if scene in ("grid", "zero_row_overlapping"):
        # the case is about equality: > / < would change the counts the device was just held to
        strict = tq.tree_quality(nodes, ordered, verts, strict=True)
        assert o["ext_pairs_inner"] > 0 and o["ext_pairs_leaf"] > 0
        assert strict["ext_pairs_inner"] < o["ext_pairs_inner"] and strict["ext_pairs_leaf"] < o["ext_pairs_leaf"]
    if scene != "grid":  # a box corner of -0 holds a vertex at +0 and the reverse: both signs meet in these scenes
        z = verts[verts == 0]
        assert np.signbit(z).any() and not np.signbit(z).all()


# 4. one big leaf and total overlap
def test_one_big_leaf():
    verts, prims = ss.coincident_centroids(400)
    nodes, ordered = _tree(prims, verts, "sah")
    assert nodes["nprims"].max() > 4
    _check(nodes, ordered, verts)


@pytest.mark.parametrize("builder", ("sah", "equal"))
def test_total_overlap(builder):
    verts, prims = ss.bvh_overlapping(300, (1, 2, 3), 4)
    nodes, ordered = _tree(prims, verts, builder, 4)
    q, o = _check(nodes, ordered, verts)
    # nearly every primitive is external to the nodes off its own path: many adds land on one address
    assert len(nodes) > 1 and o["node_external"].max() > 0.9 * len(prims)
    assert o["ext_pairs_inner"] + o["ext_pairs_leaf"] > 100 * len(prims)


# 5. depth
@pytest.mark.parametrize("lean", ("right", "left"))
def test_chains_at_the_depth_limit(lean):
    lo, hi = tq.chain_boxes(65, seed=3)
    verts, prims = ss.box_tris(lo, hi)
    nodes = ss.chain_nodes(lo, hi) if lean == "right" else tq.left_chain_nodes(lo, hi)
    q, o = _check(nodes, prims, verts)
    assert q.depth == 64 and o["ext_pairs_inner"] > 0 and o["ext_pairs_leaf"] > 0
    lo, hi = tq.chain_boxes(66, seed=3)
    verts, prims = ss.box_tris(lo, hi)
    nodes = ss.chain_nodes(lo, hi) if lean == "right" else tq.left_chain_nodes(lo, hi)
    with pytest.raises(NNBVHError, match="tree depth 65 over 64"):
        tree_quality(nodes, prims, verts)


# 6. degenerate area
@pytest.mark.parametrize("point", (False, True))
def test_zero_area_gives_the_formulas_nan(point):
    verts, prims = ss.kd_line(60, point=point)
    nodes, ordered = _tree(prims, verts, "sah")
    q, o = _check(nodes, ordered, verts)
    assert q.prim_area == 0.0 and q.root_area == 0.0
    assert np.isnan(q.epo) and np.isnan(o["epo"]) and np.isnan(q.sah) == np.isnan(o["sah"])


# 7. contention at size
@pytest.mark.parametrize("size, most", ((2.0, 900), (3.0, 1000)))
def test_contention_at_size(size, most):
    """random_soup(6000, size=2.0) with leaf size 4 is the case as it was asked for, together with the condition that
    some node receives more than 1 000 externals.  On that scene none of the five builders gives a node that many: the
    busiest node, a child of the root, gets 965 (sah, middle), 964 (hlbvh), 942 (equal) and 923 (nn) — the triangles
    of the other half that reach into a slab about one triangle size wide, a tenth of the scene.  So that scene runs
    with the floor it can meet, and the same soup with size=3.0 carries the condition of more than 1 000."""
    verts, prims = ss.random_soup(6000, size=size)
    nodes, ordered = _tree(prims, verts, "sah", 4)
    o = tq.tree_quality(nodes, ordered, verts)
    print("busiest node:", int(o["node_external"].max()), "externals")
    assert o["node_external"].max() > most
    q, _ = _check(nodes, ordered, verts, oracle=o)
    print(f"6000-triangle soup, size {size}:", len(nodes), "nodes,", o["ext_pairs_inner"] + o["ext_pairs_leaf"],
          "pairs, gpu_ms", q.gpu_ms)


# 8. non-default constants
@pytest.mark.parametrize("c_inner, c_leaf", ((0.0, 0.0), (0.0, 1.0), (1.2, 0.0), (1e-300, 7.0 / 3.0), (3.7e5, 1e-9)))
def test_constants(c_inner, c_leaf):
    verts, prims = ss.random_soup(500, seed=9, extent=4.0)
    nodes, ordered = _tree(prims, verts, "sah")
    q, _ = _check(nodes, ordered, verts, c_inner=c_inner, c_leaf=c_leaf)
    base = tree_quality(nodes, ordered, verts)
    for k in ("inner_area", "leaf_area_weighted", "root_area", "prim_area", "ext_area_inner", "ext_area_leaf",
              "ext_pairs_inner", "ext_pairs_leaf"):
        assert getattr(q, k) == getattr(base, k), k
    assert q.sah == (c_inner * q.inner_area + c_leaf * q.leaf_area_weighted) / q.root_area
    assert q.epo == (c_inner * q.ext_area_inner + c_leaf * q.ext_area_leaf) / q.prim_area


# 9. the killeroos blob
def test_killeroos_sample():
    blob = ss.scene_blob("killeroos")
    if blob is None:
        pytest.skip("no killeroos blob")
    verts, tris = blob
    t = build_tree(make_prims(tris), verts, 4, "sah")
    pos = np.sort(np.random.default_rng(7).choice(len(t.ordered_prims), 4000, replace=False))
    o = tq.tree_quality(t.nodes, t.ordered_prims, verts, positions=pos)
    q = tree_quality(t.nodes, t.ordered_prims, verts, per_primitive=True, per_node=True)
    again = tree_quality(t.nodes, t.ordered_prims, verts, per_primitive=True, per_node=True)
    assert (q.prim_ext_inner[pos] == o["prim_ext_inner"]).all()
    assert (q.prim_ext_leaf[pos] == o["prim_ext_leaf"]).all()
    assert (q.node_external >= o["node_external"]).all()  # the sample's share of every node's count
    assert q.ext_pairs_inner == int(q.prim_ext_inner.astype(np.int64).sum())
    assert q.ext_pairs_leaf == int(q.prim_ext_leaf.astype(np.int64).sum())
    assert int(q.node_external.astype(np.int64).sum()) == q.ext_pairs_inner + q.ext_pairs_leaf
    assert q.raw == again.raw and q.node_external.tobytes() == again.node_external.tobytes()
    print("killeroos:", len(t.nodes), "nodes, sah", q.sah, "epo", q.epo, "gpu_ms", q.gpu_ms)
