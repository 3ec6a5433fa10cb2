"""The fork's two tree scores, SAH(head_node) and EPO(head_node) (machine_learning/nn_loss.py:165-192, 119-135), of a
baked tree, computed on the device (nnbvh_tree_quality_create, include/nnbvh.h).  Any flat tree in the
layout build_tree / build_tree_gpu / nn_tree.bake produce can be scored; there is no CPU fallback."""
import ctypes

import numpy as np

from ._lib import NODE_DTYPE, PRIM_DTYPE, TreeQuality as _TreeQuality, check, lib, ptr

C_INNER, C_LEAF = 1.2, 1.0  # nn_loss.py:113-117

_DOUBLES = ("sah", "epo", "inner_area", "leaf_area_weighted", "root_area", "prim_area", "ext_area_inner",
            "ext_area_leaf")
_INTS = ("ext_pairs_inner", "ext_pairs_leaf", "n_inner", "n_leaves", "depth")


class TreeQuality:
    """Result of tree_quality(): the fields of nnbvh_tree_quality as attributes (sah, epo, the sums before the
    constants, the external-pair totals, n_inner, n_leaves, depth), gpu_ms = {"prepare", "walk", "reduce", "total"},
    and where asked for prim_ext_inner / prim_ext_leaf (int32 per ORDERED position) and node_external (int32 per
    node); None otherwise."""

    def __init__(self, raw, prim_ext_inner, prim_ext_leaf, node_external):
        for k in _DOUBLES:
            setattr(self, k, float(getattr(raw, k)))
        for k in _INTS:
            setattr(self, k, int(getattr(raw, k)))
        self.gpu_ms = dict(zip(("prepare", "walk", "reduce", "total"), (float(x) for x in raw.gpu_ms)))
        self.prim_ext_inner, self.prim_ext_leaf, self.node_external = prim_ext_inner, prim_ext_leaf, node_external
        self.raw = bytes(raw)[:ctypes.sizeof(_TreeQuality) - 16]  # everything but the times: equal on equal input

    def __repr__(self):
        return (f"TreeQuality(sah={self.sah:.6g}, epo={self.epo:.6g}, n_inner={self.n_inner}, "
                f"n_leaves={self.n_leaves}, depth={self.depth})")


def tree_quality(nodes, ordered_prims, verts, c_inner=C_INNER, c_leaf=C_LEAF, device=0, per_primitive=False,
                 per_node=False):
    """SAH and EPO of the tree (nodes, ordered_prims) over verts, with the fork's constants unless given.  Triangles
    only, as in the fork.  A malformed tree, or one that breaks the two nesting rules the scores rest on (a child box
    inside its parent's, a primitive inside its leaf's box), raises NNBVHError naming the first offender."""
    nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
    prims = np.ascontiguousarray(ordered_prims, PRIM_DTYPE)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    raw = _TreeQuality()
    k_inner = np.zeros(len(prims), np.int32) if per_primitive else None
    k_leaf = np.zeros(len(prims), np.int32) if per_primitive else None
    node_ext = np.zeros(len(nodes), np.int32) if per_node else None
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    check(lib().nnbvh_tree_quality_create(ptr(nodes), len(nodes), ptr(prims), len(prims), ptr(verts), len(verts),
                                          float(c_inner), float(c_leaf), int(device), ctypes.byref(raw),
                                          opt(k_inner), opt(k_leaf), opt(node_ext)), "nnbvh_tree_quality_create")
    return TreeQuality(raw, k_inner, k_leaf, node_ext)
