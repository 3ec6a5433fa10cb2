"""Brute-force numpy oracle of the fork's SAH and EPO scores (machine_learning/nn_loss.py:119-135, 165-192) by their
SET definition: for every (primitive, node) pair, is the primitive outside the node's subtree and does one of its
vertices lie in the node's closed box.  float32 comparisons for containment, float64 for areas and sums.  No tree walk
and no pruning by the tree: what tests/test_tree_quality.py holds the device to, and what tests/test_tree_quality_oracle.py holds to the
fork's own functions (tests/golden/tree_quality_reference.npz)."""
import numpy as np

C_INNER, C_LEAF = 1.2, 1.0  # nn_loss.py:113-117
DOUBLES = ("sah", "epo", "inner_area", "leaf_area_weighted", "root_area", "prim_area", "ext_area_inner",
           "ext_area_leaf")
# number of terms behind each double: "nodes" for the SAH sums, "prims" for the EPO sums (tolerance())
TERMS = {"sah": "nodes", "inner_area": "nodes", "leaf_area_weighted": "nodes", "root_area": "nodes",
         "epo": "prims", "prim_area": "prims", "ext_area_inner": "prims", "ext_area_leaf": "prims"}


def subtree_ends(nodes):
    """end[i] = the first node after node i's subtree in depth-first order"""
    n = len(nodes)
    end = np.zeros(n, np.int64)
    for i in range(n - 1, -1, -1):
        end[i] = i + 1 if nodes["nprims"][i] else end[nodes["offset"][i]]
    return end


def leaf_of_positions(nodes, n_prims):
    leaf_of = np.full(n_prims, -1, np.int64)
    for i in np.flatnonzero(nodes["nprims"]):
        o = int(nodes["offset"][i])
        leaf_of[o:o + int(nodes["nprims"][i])] = i
    return leaf_of


def tree_depth(nodes):
    """edges from the root to the deepest leaf"""
    level = np.zeros(len(nodes), np.int64)
    for i in range(len(nodes)):
        if nodes["nprims"][i] == 0:
            level[i + 1] = level[nodes["offset"][i]] = level[i] + 1
    return int(level.max())


def triangle_areas(verts, prims):
    P = np.asarray(verts, np.float32).reshape(-1, 3)[prims["v"][:, :3]].astype(np.float64)
    u = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    return 0.5 * np.sqrt((u * u).sum(1))


def box_areas(nodes):
    e = nodes["pmax"].astype(np.float64) - nodes["pmin"].astype(np.float64)
    return 2.0 * (e[:, 0] * e[:, 1] + e[:, 0] * e[:, 2] + e[:, 1] * e[:, 2])


def external_matrix(nodes, prims, verts, positions=None, strict=False, rule="vertex", chunk=None):
    """Yields (positions of the chunk, node indices `cols`, bool [chunk, len(cols)]): primitive at ordered position j is
    external to node cols[i]; to every node not in cols it is not.  rule "vertex": at least one vertex inside the box
    (the fork's); "overlap": the primitive's box overlaps the node's; "centroid": the centroid of the three vertices is
    inside.  strict: > / < instead of >= / <=.
    Brute force over (primitive, node) but for one exact shortcut that knows nothing of the tree: a node whose box
    does not meet the box around ALL vertices of the chunk can hold none of them under any of the rules, so its column
    is left out.  (Positions are in leaf order, so a chunk is compact in space; on 130 000 nodes this is the
    difference between seconds and a minute.)"""
    verts = np.asarray(verts, np.float32).reshape(-1, 3)
    n_nodes = len(nodes)
    positions = np.arange(len(prims)) if positions is None else np.asarray(positions)
    end = subtree_ends(nodes)
    own = leaf_of_positions(nodes, len(prims))
    lo, hi = nodes["pmin"], nodes["pmax"]  # float32 [n_nodes, 3]
    ge, le = (np.greater, np.less) if strict else (np.greater_equal, np.less_equal)
    chunk = chunk or max(1, (1 << 22) // max(n_nodes, 1))
    for c0 in range(0, len(positions), chunk):
        pos = positions[c0:c0 + chunk]
        P = verts[prims["v"][pos, :3]]  # float32 [c, 3, 3]
        vmin, vmax = P.reshape(-1, 3).min(0), P.reshape(-1, 3).max(0)
        cols = np.flatnonzero(((lo <= vmax) & (hi >= vmin)).all(1))
        clo, chi = lo[cols], hi[cols]
        if rule == "vertex":
            inside = np.ones((len(pos), 3, len(cols)), bool)
            for k in range(3):
                x = P[:, :, k, None]
                inside &= ge(x, clo[None, None, :, k]) & le(x, chi[None, None, :, k])
            inside = inside.any(1)
        elif rule == "overlap":
            mn, mx = P.min(1), P.max(1)
            inside = np.ones((len(pos), len(cols)), bool)
            for k in range(3):
                inside &= le(mn[:, k, None], chi[None, :, k]) & ge(mx[:, k, None], clo[None, :, k])
        elif rule == "centroid":
            c = (P.astype(np.float64).sum(1) / 3.0).astype(np.float32)
            inside = np.ones((len(pos), len(cols)), bool)
            for k in range(3):
                inside &= ge(c[:, k, None], clo[None, :, k]) & le(c[:, k, None], chi[None, :, k])
        else:
            raise ValueError(rule)
        o = own[pos][:, None]
        in_subtree = (cols[None, :] <= o) & (o < end[cols][None, :])
        yield pos, cols, inside & ~in_subtree


def tree_quality(nodes, prims, verts, c_inner=C_INNER, c_leaf=C_LEAF, positions=None, strict=False, rule="vertex"):
    """The fields of nnbvh_tree_quality plus prim_ext_inner / prim_ext_leaf (per ordered position; with `positions`:
    per sampled position, and node_external then counts the sample only) and node_external."""
    nodes, prims = np.asarray(nodes), np.asarray(prims)
    n_nodes = len(nodes)
    is_leaf = nodes["nprims"] != 0
    n_out = len(prims) if positions is None else len(positions)
    k_inner, k_leaf = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    node_external = np.zeros(n_nodes, np.int64)
    at = 0
    for pos, cols, ext in external_matrix(nodes, prims, verts, positions, strict, rule):
        leaf_cols = is_leaf[cols]
        k_inner[at:at + len(pos)] = ext[:, ~leaf_cols].sum(1)
        k_leaf[at:at + len(pos)] = ext[:, leaf_cols].sum(1)
        node_external[cols] += ext.sum(0)
        at += len(pos)
    sel = prims if positions is None else prims[np.asarray(positions)]
    area = triangle_areas(verts, sel)
    A = box_areas(nodes)
    out = {"inner_area": A[~is_leaf].sum() if (~is_leaf).any() else np.float64(0.0),
           "leaf_area_weighted": (A[is_leaf] * nodes["nprims"][is_leaf].astype(np.float64)).sum(),
           "root_area": A[0], "prim_area": area.sum(), "ext_area_inner": (area * k_inner).sum(),
           "ext_area_leaf": (area * k_leaf).sum()}
    c_inner, c_leaf = np.float64(c_inner), np.float64(c_leaf)
    with np.errstate(all="ignore"):
        out["sah"] = (c_inner * out["inner_area"] + c_leaf * out["leaf_area_weighted"]) / out["root_area"]
        out["epo"] = (c_inner * out["ext_area_inner"] + c_leaf * out["ext_area_leaf"]) / out["prim_area"]
    out = {k: float(v) for k, v in out.items()}
    out.update(ext_pairs_inner=int(k_inner.astype(np.int64).sum()), ext_pairs_leaf=int(k_leaf.astype(np.int64).sum()),
               n_inner=int((~is_leaf).sum()), n_leaves=int(is_leaf.sum()), depth=tree_depth(nodes),
               prim_ext_inner=k_inner, prim_ext_leaf=k_leaf, node_external=node_external.astype(np.int32))
    return out


def tolerance(n_terms):
    """Relative bound between two evaluations of a sum of n non-negative terms (or a ratio of two): recursive summation
    in any order is within (n - 1) 2^-53 of the exact sum on each side, and each term differs by a few ulps (the
    order of the three-term dot under the square root): (2 n + 16) 2^-53."""
    return (2 * n_terms + 16) * 2.0 ** -53


def same_class_or_close(got, exp, n_terms):
    """NaN and inf by class (and sign); finite values within tolerance(n_terms) relative to the expected value."""
    got, exp = float(got), float(exp)
    if np.isnan(exp) or np.isnan(got):
        return bool(np.isnan(exp) and np.isnan(got))
    if np.isinf(exp) or np.isinf(got):
        return got == exp
    return abs(got - exp) <= tolerance(n_terms) * abs(exp)


def mismatched_doubles(got, exp, n_nodes, n_prims):
    """[(field, got, expected, relative error, bound)] of the eight doubles outside the tolerance; got: an object with
    the fields as attributes or a dict, exp: tree_quality()'s dict"""
    bad = []
    for k in DOUBLES:
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        n = n_nodes if TERMS[k] == "nodes" else n_prims
        if not same_class_or_close(g, exp[k], n):
            rel = abs(g - exp[k]) / abs(exp[k]) if exp[k] else float("inf")
            bad.append((k, g, exp[k], rel, tolerance(n)))
    return bad


def left_chain_nodes(lo, hi):
    """The mirror image of scenes_small.chain_nodes: a maximally skewed tree over leaves with the boxes lo[k] / hi[k] (one
    primitive each, ordered position k) whose interior nodes have the interior child FIRST and a leaf second.  Nodes
    0 .. L - 2 are the interior ones, node L - 1 the deepest leaf (position 0); interior i's second child is the leaf at
    2 L - 2 - i (position L - 1 - i)."""
    from nn_bvh_amd import NODE_DTYPE
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    n_leaves = len(lo)
    nodes = np.zeros(2 * n_leaves - 1, NODE_DTYPE)
    for i in range(n_leaves - 1):
        nodes[i]["pmin"], nodes[i]["pmax"] = lo[:n_leaves - i].min(0), hi[:n_leaves - i].max(0)
        nodes[i]["offset"], nodes[i]["nprims"] = 2 * n_leaves - 2 - i, 0
    for k in range(n_leaves):
        leaf = nodes[n_leaves - 1 + k]
        leaf["pmin"], leaf["pmax"], leaf["offset"], leaf["nprims"] = lo[k], hi[k], k, 1
    return nodes


def chain_boxes(n_leaves, seed=0):
    """overlapping leaf boxes along x for the hand-made chains: neighbours share space, so externals exist"""
    rng = np.random.default_rng(seed)
    lo = np.stack([np.arange(n_leaves) * 0.5, rng.uniform(-1, 0, n_leaves), rng.uniform(-1, 0, n_leaves)], 1)
    hi = lo + np.stack([rng.uniform(0.6, 2.0, n_leaves), rng.uniform(1, 2, n_leaves), rng.uniform(1, 2, n_leaves)], 1)
    return lo.astype(np.float32), hi.astype(np.float32)
