"""CPU tests of the tree-quality scores: the numpy oracle (tests/tree_quality_oracle.py) against what
the fork's own SAH / EPO functions returned (tests/golden/tree_quality_reference.npz, recorded by
tests/golden/make_tree_quality_golden.py), the properties of the oracle that the GPU tests rely on, and every refusal
of nnbvh_tree_quality_create, none of which needs a device."""
import ctypes
import os

import numpy as np
import pytest

import scenes_small as ss
import tree_quality_oracle as tq
from nn_bvh_amd import NODE_DTYPE, PRIM_DTYPE, build_tree
from nn_bvh_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tree_quality_reference.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _golden_tree(g, key):
    scene = key.split("_")[0]
    return g[f"{key}_nodes"].view(NODE_DTYPE).reshape(-1), g[f"{key}_ordered_prims"].view(PRIM_DTYPE).reshape(-1), \
        g[f"{scene}_verts"]


def test_recorded_trees_cover_five_builders_on_two_scenes(golden):
    assert sorted(golden["trees"]) == sorted(f"{s}_{t}" for s in ("soup", "field")
                                             for t in ("sah", "hlbvh", "middle", "equal", "nn"))
    assert len(golden["soup_tris"]) <= 200 and len(golden["field_tris"]) <= 200
    assert float(golden["c_inner"]) == tq.C_INNER and float(golden["c_leaf"]) == tq.C_LEAF


@pytest.mark.parametrize("key", [f"{s}_{t}" for s in ("soup", "field") for t in ("sah", "hlbvh", "middle", "equal", "nn")])
def test_oracle_matches_the_forks_functions(golden, key):
    nodes, prims, verts = _golden_tree(golden, key)
    o = tq.tree_quality(nodes, prims, verts)
    # the pruned search of the fork finds the set the definition names, node by node
    assert (o["node_external"] == golden[f"{key}_node_external"]).all()
    assert o["node_external"][0] == 0
    assert o["ext_pairs_inner"] + o["ext_pairs_leaf"] == int(golden[f"{key}_node_external"].sum())
    print(key, "sah", o["sah"], float(golden[f"{key}_sah"]), "epo", o["epo"], float(golden[f"{key}_epo"]))
    assert tq.same_class_or_close(o["sah"], golden[f"{key}_sah"], len(nodes))
    assert tq.same_class_or_close(o["epo"], golden[f"{key}_epo"], len(prims))


@pytest.fixture(scope="module")
def field_tree():
    verts, prims = ss.grid_mesh(12)  # 288 triangles on shared vertices
    t = build_tree(prims, verts, 2, "sah")
    return t.nodes, t.ordered_prims, verts


def test_closed_intervals_decide_most_pairs_of_a_height_field(field_tree):
    closed = tq.tree_quality(*field_tree)
    strict = tq.tree_quality(*field_tree, strict=True)
    changed = int((closed["node_external"] != strict["node_external"]).sum())
    lost = (closed["ext_pairs_inner"] + closed["ext_pairs_leaf"]) - (strict["ext_pairs_inner"] + strict["ext_pairs_leaf"])
    print("pairs", closed["ext_pairs_inner"] + closed["ext_pairs_leaf"], "lost under > / <", lost, "nodes changed", changed)
    assert lost >= 1000


def test_any_vertex_is_neither_box_overlap_nor_centroid(field_tree):
    pairs = {}
    for rule in ("vertex", "overlap", "centroid"):
        o = tq.tree_quality(*field_tree, rule=rule)
        pairs[rule] = o["ext_pairs_inner"] + o["ext_pairs_leaf"]
    print(pairs)
    assert pairs["vertex"] != pairs["overlap"] and pairs["vertex"] != pairs["centroid"]
    assert pairs["centroid"] < pairs["vertex"] < pairs["overlap"]


def test_leaf_externals_and_primitives_without_any_exist():
    verts, prims = ss.random_soup(300, seed=3)
    t = build_tree(prims, verts, 4, "sah")
    o = tq.tree_quality(t.nodes, t.ordered_prims, verts)
    assert (o["prim_ext_leaf"] != 0).any()
    assert ((o["prim_ext_inner"] + o["prim_ext_leaf"]) == 0).any()


def test_left_chain_is_the_mirror_of_the_right_chain():
    lo, hi = tq.chain_boxes(9, seed=1)
    verts, prims = ss.box_tris(lo, hi)
    right = tq.tree_quality(ss.chain_nodes(lo, hi), prims, verts)
    left = tq.tree_quality(tq.left_chain_nodes(lo[::-1], hi[::-1]), *ss.box_tris(lo[::-1], hi[::-1])[::-1])
    assert right["depth"] == left["depth"] == 8
    assert right["ext_pairs_inner"] == left["ext_pairs_inner"] and right["ext_pairs_leaf"] == left["ext_pairs_leaf"]
    assert right["ext_pairs_inner"] + right["ext_pairs_leaf"] > 0


# ---- the refusals of nnbvh_tree_quality_create: host-side, before any device is looked at ---------------------------
def _base():
    verts, prims = ss.random_soup(40, seed=11)
    t = build_tree(prims, verts, 2, "sah")
    return t.nodes.copy(), t.ordered_prims.copy(), np.ascontiguousarray(verts, np.float32).copy()


def _call(nnbvh_lib, nodes, prims, verts, c_inner=1.2, c_leaf=1.0, n_nodes=None, n_prims=None, n_verts=None,
          with_out=True):
    """(status, message, out bytes changed?, arrays changed?)"""
    raw = _lib.TreeQuality()
    ctypes.memset(ctypes.byref(raw), 0xAB, ctypes.sizeof(raw))
    before = bytes(raw)
    k_inner = np.full(max(len(prims) if prims is not None else 1, 1), -7, np.int32)
    k_leaf, node_ext = k_inner.copy(), np.full(max(len(nodes) if nodes is not None else 1, 1), -7, np.int32)
    p = lambda a: _lib.ptr(a) if a is not None else None  # noqa: E731
    rc = nnbvh_lib.nnbvh_tree_quality_create(
        p(nodes), len(nodes) if n_nodes is None else n_nodes, p(prims), len(prims) if n_prims is None else n_prims,
        p(verts), len(verts) if n_verts is None else n_verts, c_inner, c_leaf, 0,
        ctypes.byref(raw) if with_out else None, p(k_inner), p(k_leaf), p(node_ext))
    touched = bytes(raw) != before or (k_inner != -7).any() or (k_leaf != -7).any() or (node_ext != -7).any()
    return rc, _lib.last_error(), touched


def _first_interior_with_leaf_children(nodes):
    for i in range(len(nodes)):
        if nodes["nprims"][i] == 0 and nodes["nprims"][i + 1] and nodes["nprims"][nodes["offset"][i]]:
            return i
    raise AssertionError("no such node")


def _fault_cases():
    def null_nodes(n, p, v):
        return dict(nodes=None, n_nodes=len(n))

    def empty_nodes(n, p, v):
        return dict(n_nodes=0)

    def null_prims(n, p, v):
        return dict(prims=None, n_prims=len(p))

    def empty_verts(n, p, v):
        return dict(n_verts=0)

    def null_out(n, p, v):
        return dict(with_out=False)

    def nan_c_inner(n, p, v):
        return dict(c_inner=float("nan"))

    def inf_c_leaf(n, p, v):
        return dict(c_leaf=float("inf"))

    def vertex_index(n, p, v):
        p["v"][5, 1] = len(v)

    def negative_vertex_index(n, p, v):
        p["v"][0, 2] = -1

    def nan_vertex(n, p, v):
        v[7, 1] = np.nan

    def inf_box_corner(n, p, v):
        n["pmax"][3, 2] = np.inf

    def offset_is_first_child(n, p, v):
        i = _first_interior_with_leaf_children(n)
        n["offset"][i] = i + 1

    def offset_past_the_end(n, p, v):
        n["offset"][0] = len(n)

    def offset_inside_first_subtree(n, p, v):
        n["offset"][0] = 2 if n["offset"][0] != 2 else 3

    def leaf_range(n, p, v):
        i = int(np.flatnonzero(n["nprims"])[-1])
        n["offset"][i] = len(p) - int(n["nprims"][i]) + 1

    def negative_leaf_range(n, p, v):
        n["offset"][int(np.flatnonzero(n["nprims"])[0])] = -1

    def covered_twice(n, p, v):
        leaves = np.flatnonzero(n["nprims"])
        n["offset"][leaves[1]] = n["offset"][leaves[0]]

    def covered_never(n, p, v):
        return dict(prims=np.concatenate([p, p[:1]]))

    def node_count(n, p, v):
        extra = n[-1:].copy()
        extra["offset"], extra["nprims"] = len(p), 1
        return dict(nodes=np.concatenate([n, extra]), prims=np.concatenate([p, p[-1:]]))

    def child_box(n, p, v):
        n["pmax"][1, 0] = n["pmax"][0, 0] + np.float32(1.0)

    def vertex_outside_leaf(n, p, v):
        v[p["v"][4, 0], 0] += np.float32(50.0)

    def patch(n, p, v):
        p["kind"][3] = 1

    def host_only(n, p, v):
        p["kind"][0] = 3

    return [(null_nodes, "null or empty"), (empty_nodes, "null or empty"), (null_prims, "null or empty"),
            (empty_verts, "null or empty"), (null_out, "null or empty"), (nan_c_inner, "must be finite"),
            (inf_c_leaf, "must be finite"), (vertex_index, "ordered primitive 5: vertex index"),
            (negative_vertex_index, "ordered primitive 0: vertex index -1"), (nan_vertex, "vertex 7 is not finite"),
            (inf_box_corner, "node 3: a box corner is not finite"), (offset_is_first_child, "second-child offset"),
            (offset_past_the_end, "node 0: second-child offset"),
            (offset_inside_first_subtree, "is not where its first child's subtree ends"),
            (leaf_range, "leaf range"), (negative_leaf_range, "leaf range [-1"), (covered_twice, "is covered by two leaves"),
            (covered_never, "is covered by no leaf"), (node_count, "is not 2 * leaves - 1"),
            (child_box, "node 1: box not inside the box of its parent, node 0"),
            (vertex_outside_leaf, "ordered primitive 4: vertex 0 outside the box of its leaf"),
            (patch, "ordered primitive 3 has kind 1: the fork defines both scores on triangles only"),
            (host_only, "the fork defines both scores on triangles only")]


@pytest.mark.parametrize("case", _fault_cases(), ids=lambda c: c[0].__name__)
def test_malformed_input_is_refused_on_the_host(nnbvh_lib, case):
    mutate, message = case
    nodes, prims, verts = _base()
    kw = dict(nodes=nodes, prims=prims, verts=verts)
    kw.update(mutate(nodes, prims, verts) or {})
    rc, text, touched = _call(nnbvh_lib, **kw)
    assert rc == 1, (rc, text)  # NNBVH_ERR_ARG
    assert "nnbvh_tree_quality_create" in text and message in text, text
    assert not touched


def test_chain_of_65_edges_is_refused_and_of_64_is_not(nnbvh_lib):
    for n_leaves, refused in ((66, True), (65, False)):
        lo, hi = tq.chain_boxes(n_leaves)
        verts, prims = ss.box_tris(lo, hi)
        for nodes in (ss.chain_nodes(lo, hi), tq.left_chain_nodes(lo, hi)):
            rc, text, touched = _call(nnbvh_lib, nodes, prims, verts)
            if refused:
                assert rc == 1 and "tree depth 65 over 64" in text and not touched, (rc, text)
            else:  # accepted by the host checks: scored where there is a device, NNBVH_ERR_DEVICE where there is none
                assert rc in (0, 2), (rc, text)
                assert rc == 0 or "no usable HIP device" in text


def test_python_wrapper_raises_with_the_message():
    from nn_bvh_amd import NNBVHError, tree_quality
    nodes, prims, verts = _base()
    prims["kind"][2] = 1
    with pytest.raises(NNBVHError, match="triangles only"):
        tree_quality(nodes, prims, verts)
