"""BVHAggregate construction (cpu/aggregates.cpp:192-387 buildRecursive's SAH branch, :389-503 and :626-723 HLBVH; the
host builder nn_bvh_amd/csrc/bvh_build.cpp) and its device twins (bvh_build_gpu.hip, bvh_bake.hip).

Every decision path of the two builders has a scene of its own (PATH_CASES).  A census of the HOST-built tree
(census_sah / census_hlbvh, pure numpy: the builder's decisions recomputed in float32 in its own expression order)
proves on the CPU that the scene reaches its path; the GPU tests then compare the device builders with the host one
byte for byte on exactly those cases, for SAH at every hand-over threshold between the breadth-first and the
one-wavefront implementation, and trace rays through some of the device-built scenes.

Paths of the host code that no input reaches (and so have no case):
  * a leaf of more than 256 primitives closed by the cost rule: that rule needs n <= maxPrims <= 255 (:142).
  * bvh_build.cpp:324 (the reference's CHECK_NE, aggregates.cpp:650: all treelet centroids coincide in the chosen
    dimension).  upper() is entered with two or more treelets, each the primitives of ONE cell of the 16^3 grid over
    the centroid bounds, and two different cells means an axis on which the centroid bounds have an extent, on
    which both the cell at offset 0 and a cell further up are occupied.  Treelet BOUNDS centroids can still
    coincide (large boxes around small ones), which is why the host builder reports it instead of asserting; a
    finite input that does it was not found and none is claimed.
  * bvh_build.cpp:367 (CHECK_GT / CHECK_LT, :715-716): the partition puts every treelet on one side only when all
    of them share a bucket <= best or none does; bucket 0 and bucket 11 both hold a treelet whenever the centroid
    extent is non-zero and the costs are comparable.  With NaN costs (hlbvh_range below) best stays 0 and bucket 0
    is never empty, so the split is still proper.
  * one treelet holding an emitLBVH split: a single treelet means no axis has a centroid extent (else offsets 0 and
    1 both occur on it and fall into cells 0 and 15), so all codes are equal and the treelet is one leaf.  The
    one-treelet case is therefore a single leaf; splits inside a treelet are covered by every other HLBVH case."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import BVHAggregate, NNBVHError, build_tree, build_tree_gpu, scene
from nn_bvh_amd._lib import NODE_DTYPE
from test_gpu_build import same_tree

f32 = np.float32
FLT_MAX = np.finfo(np.float32).max
TILE = 2048          # bvh_build_gpu.hip kTile: primitives of one big node per block of the breadth-first kernels
LEAF_CLASSES = ("2", "3_64", "65_256", "gt256")
INTERIOR_CLASSES = ("2", "3_64", "65_256", "257_2048", "gt2048")


# ---- what both censuses share -----------------------------------------------------------------------------------
def prim_boxes(prims, verts):
    """(n, 6) float32: Triangle::Bounds / BilinearPatch::Bounds as the builders fold them, vertex by vertex, the first
    of equal values kept (the sign of a zero is the first vertex's that has it)."""
    verts = np.asarray(verts, np.float32)
    out = np.zeros((len(prims), 6), np.float32)
    for nv, sel in ((3, prims["kind"] != 1), (4, prims["kind"] == 1)):
        if sel.any():
            p = verts[prims["v"][sel][:, :nv]]
            out[sel, :3] = np.take_along_axis(p, p.argmin(1)[:, None, :], 1)[:, 0]
            out[sel, 3:] = np.take_along_axis(p, p.argmax(1)[:, None, :], 1)[:, 0]
    return out


def fold_first(boxes):
    """Box::add over the rows in order: (6,) float32, the first of equal values kept."""
    k = np.arange(3)
    return np.concatenate([boxes[boxes[:, :3].argmin(0), k], boxes[boxes[:, 3:].argmax(0), 3 + k]])


def area_of(mn, mx):
    """Bounds3::SurfaceArea (util/vecmath.h:1293-1296) over the last axis, float32, the builder's order."""
    d = mx - mn
    return f32(2) * (d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2] + d[..., 1] * d[..., 2])


def max_dimension(e):
    """Bounds3::MaxDimension (util/vecmath.h:1305-1313) of extents e (..., 3)."""
    return np.where((e[..., 0] > e[..., 1]) & (e[..., 0] > e[..., 2]), 0, np.where(e[..., 1] > e[..., 2], 1, 2))


def tree_shape(nodes):
    """Per node of a flattened LinearBVHNode array: first slot and number of its primitives in the ordered table,
    whether they are one contiguous slice, depth, parent, length of the left spine below it, and `pending`: the
    number of its ancestors whose second child is still to come when a depth-first build reaches it (those it lies
    in the first sub-tree of)."""
    n = len(nodes)
    off, npr = nodes["offset"].astype(np.int64), nodes["nprims"].astype(np.int64)
    start, cnt, size = np.zeros(n, np.int64), np.zeros(n, np.int64), np.ones(n, np.int64)
    depth, parent, spine = np.zeros(n, np.int64), np.full(n, -1, np.int64), np.zeros(n + 1, np.int64)
    pending = np.zeros(n, np.int64)
    contig = np.ones(n, bool)
    for i in range(n - 1, -1, -1):
        if npr[i]:
            start[i], cnt[i] = off[i], npr[i]
            continue
        lf, rt = i + 1, int(off[i])
        assert lf < rt < n and rt == lf + size[lf], f"node {i}: second child {rt} does not follow the first sub-tree"
        size[i] = 1 + size[lf] + size[rt]
        start[i], cnt[i] = min(start[lf], start[rt]), cnt[lf] + cnt[rt]
        contig[i] = contig[lf] and contig[rt] and start[rt] == start[lf] + cnt[lf]
        spine[i] = 1 + spine[lf]
    assert size[0] == n
    for i in range(n):
        if not npr[i]:
            depth[i + 1] = depth[off[i]] = depth[i] + 1
            parent[i + 1] = parent[off[i]] = i
            pending[i + 1], pending[off[i]] = pending[i] + 1, pending[i]
    return start, cnt, contig, depth, parent, spine[:n], pending


def check_interior_bounds(nodes, c):
    """Every interior node's stored box is Union(child 0, child 1) with the first of equal values kept (:371-373,
    :495-498); counts the nodes where both children supply a zero and the signs differ."""
    ii = np.nonzero(nodes["nprims"] == 0)[0]
    a, b = nodes[ii + 1], nodes[nodes["offset"][ii]]
    lo = np.where(b["pmin"] < a["pmin"], b["pmin"], a["pmin"])
    hi = np.where(a["pmax"] < b["pmax"], b["pmax"], a["pmax"])
    assert lo.tobytes() == nodes["pmin"][ii].tobytes() and hi.tobytes() == nodes["pmax"][ii].tobytes(), \
        "an interior node's bounds are not the in-order union of its children's"
    av, bv = np.concatenate([a["pmin"], a["pmax"]], 1), np.concatenate([b["pmin"], b["pmax"]], 1)
    c["mixed_zero_interior"] = int(((av == 0) & (bv == 0) & (np.signbit(av) != np.signbit(bv))).any(1).sum())


def check_leaf_bounds(nodes, i, boxes, c):
    """A leaf's stored box is the in-order fold over its primitives' boxes.  Counts it, and returns True, if the box
    holds a zero that its primitives supply with both signs."""
    got = np.concatenate([nodes["pmin"][i], nodes["pmax"][i]])
    assert got.tobytes() == fold_first(boxes).tobytes(), f"leaf {i}: bounds are not the in-order fold of its primitives'"
    for k in np.nonzero(got == 0)[0]:
        z = boxes[:, k][boxes[:, k] == 0]
        if np.signbit(z).any() and not np.signbit(z).all():
            c["mixed_zero_leaves"] += 1
            return True
    return False


def leaf_class(n):
    return "2" if n == 2 else "3_64" if n <= 64 else "65_256" if n <= 256 else "gt256"


def interior_class(n):
    return "2" if n == 2 else "3_64" if n <= 64 else "65_256" if n <= 256 else "257_2048" if n <= 2048 else "gt2048"


# ---- SAH: buildRecursive (aggregates.cpp:192-387; bvh_build.cpp Builder::build) replayed level by level ------------
SAH_KEYS = (("nodes", "leaves", "leaf_single") + tuple(f"leaf_{r}_{k}" for r in ("flat", "coincident", "cost") for k in LEAF_CLASSES)
            + tuple(f"interior_{k}" for k in INTERIOR_CLASSES) + ("interior_n256", "interior_n257", "interior_n2048", "interior_n2049")
            + ("split_forced", "split_cheaper", "split_both", "axis0", "axis1", "axis2", "maxdim_ties", "tied_min_cost",
               "empty_middle_bucket", "no_swap", "swaps_gt64", "swaps_across_tile", "mixed_zero_leaves")
            + tuple(f"mixed_zero_leaves_{k}" for k in LEAF_CLASSES)
            + ("mixed_zero_interior", "depth", "left_spine", "second_child_interior_pending_ge64"))


def census_sah(nodes, ordered_prims, prim_bounds, max_prims):
    """Replays the SAH build top-down on the primitive order the builder itself starts from (0 .. n - 1): for every
    node the bounds, the centroid bounds, MaxDimension, the 12 buckets, the 11 costs and the verdict, then libstdc++'s
    std::partition (the k-th offender of the left part from the left trades places with the k-th offender of the right
    part from the right) or the nth_element of two.  ASSERTS that the tree holds exactly these verdicts (leaf or
    interior, axis, size of the first child, every stored box, the final primitive order) and counts

    leaf_single                     leaves of one primitive (:221)
    leaf_flat_K                     bounds without surface area with n > 1 (:221), K the size class 2 / 3_64 / 65_256 / gt256
    leaf_coincident_K               centroid bounds degenerate in the chosen dimension (:243)
    leaf_cost_K                     n <= maxPrims and no split cheaper than the leaf (:337)
    interior_K, interior_nN         interior nodes by size class (2: the nth_element of two) and of exactly N primitives
    split_forced / _cheaper / _both n > maxPrims although the leaf is cheaper / n <= maxPrims, split cheaper / both hold
    axis0 / 1 / 2, maxdim_ties      split axes; interior nodes where the largest centroid extent is shared by two axes
    tied_min_cost                   split nodes whose minimum cost several splits share (the first must win)
    empty_middle_bucket             split nodes with an empty bucket among 1 .. 10
    no_swap, swaps_gt64             split nodes whose slice was already partitioned / with more than 64 swaps
    swaps_across_tile               split nodes of more than TILE primitives with a tile boundary that has swapped
                                    positions on both sides of it
    mixed_zero_leaves(_K) / _interior   nodes whose box holds a zero that their primitives (by leaf size class) / two
                                    children supply with both signs
    depth, left_spine               tree depth; interior nodes on the longest chain of first children
    second_child_interior_pending_ge64   interior nodes that are a second child reached with 64 or more second
                                    children still pending: a depth-first build pops a stack entry beyond the 64th
                                    and then pushes again."""
    pb = np.asarray(prim_bounds, np.float32).reshape(-1, 6)
    max_prims = min(255, max_prims)                                   # aggregates.cpp:142
    start, cnt, contig, depth, _, spine, pending = tree_shape(nodes)
    assert contig.all() and cnt[0] == len(pb) == len(ordered_prims)
    c = dict.fromkeys(SAH_KEYS, 0)
    c.update(nodes=len(nodes), leaves=int((nodes["nprims"] > 0).sum()), depth=int(depth.max()), left_spine=int(spine.max()))
    perm = np.arange(len(pb))
    is_leaf = nodes["nprims"] > 0
    second = np.zeros(len(nodes), bool)
    second[nodes["offset"][~is_leaf]] = True
    c["second_child_interior_pending_ge64"] = int((second & ~is_leaf & (pending >= 64)).sum())
    with np.errstate(all="ignore"):
        for d in range(int(depth.max()) + 1):
            idx = np.nonzero(depth == d)[0]                           # preorder: ascending slice starts
            S, C, K = start[idx], cnt[idx], len(idx)
            off = np.cumsum(C) - C
            seg = np.repeat(np.arange(K), C)
            j = np.arange(int(C.sum())) - off[seg]                    # position inside the node
            pos = S[seg] + j
            B = pb[perm[pos]]
            mn, mx = np.minimum.reduceat(B[:, :3], off), np.maximum.reduceat(B[:, 3:], off)
            cen = f32(.5) * B[:, :3] + f32(.5) * B[:, 3:]             # BVHPrimitive::Centroid
            cmn, cmx = np.minimum.reduceat(cen, off), np.maximum.reduceat(cen, off)
            area = area_of(mn, mx)
            ext = cmx - cmn
            dim = max_dimension(ext)
            ar = np.arange(K)
            lo_, hi_ = cmn[ar, dim], cmx[ar, dim]
            single = C == 1
            flat = ~single & (area == 0)
            coincide = ~single & ~flat & (hi_ == lo_)
            two = ~single & ~flat & ~coincide & (C == 2)
            sah = ~single & ~flat & ~coincide & (C > 2)
            # buckets (:305-318; Bounds3::Offset vecmath.h:1322-1331)
            cd = cen[np.arange(len(seg)), dim[seg]]
            o = cd - lo_[seg]
            o = np.where(hi_[seg] > lo_[seg], o / (hi_[seg] - lo_[seg]), o)
            bk = np.minimum((f32(12) * o).astype(np.int64), 11)
            bk = np.where(sah[seg], bk, 0)
            flatk = seg * 12 + bk
            counts = np.bincount(flatk, minlength=K * 12).reshape(K, 12)
            bmn, bmx = np.full((K * 12, 3), FLT_MAX, f32), np.full((K * 12, 3), -FLT_MAX, f32)
            np.minimum.at(bmn, flatk, B[:, :3])
            np.maximum.at(bmx, flatk, B[:, 3:])
            bmn, bmx = bmn.reshape(K, 12, 3), bmx.reshape(K, 12, 3)
            below, above = np.cumsum(counts, 1), np.cumsum(counts[:, ::-1], 1)[:, ::-1]
            cost = (f32(0) + below[:, :11].astype(f32) * area_of(np.minimum.accumulate(bmn, 1)[:, :11], np.maximum.accumulate(bmx, 1)[:, :11]))
            cost = cost + above[:, 1:].astype(f32) * area_of(np.minimum.accumulate(bmn[:, ::-1], 1)[:, ::-1][:, 1:],
                                                            np.maximum.accumulate(bmx[:, ::-1], 1)[:, ::-1][:, 1:])
            assert cost.dtype == np.float32
            cc = np.where(np.isnan(cost), np.inf, cost)               # a NaN never wins `cost < minCost`
            best = cc.argmin(1)                                       # the first minimum
            minc = cc[ar, best]
            assert not (sah & (minc == np.inf)).any(), "a node without a finite split cost: the builder must refuse it"
            tied = (cc == minc[:, None]).sum(1) > 1
            cheaper = (f32(.5) + minc / area) < C.astype(f32)
            over = C > max_prims
            split = sah & (over | cheaper)
            mid = np.where(sah, below[ar, best], C // 2)
            interior = two | split
            assert np.array_equal(interior, ~is_leaf[idx]), \
                f"level {d}: nodes {idx[interior != ~is_leaf[idx]][:5]} are leaves / interior against the replayed verdict"
            ii = idx[interior]
            assert np.array_equal(nodes["axis"][ii], dim[interior]), f"level {d}: split axes differ from MaxDimension"
            assert np.array_equal(cnt[ii + 1], mid[interior]), f"level {d}: first children differ in size from the replayed split"
            # std::partition(bucket <= best) of the split nodes, nth_element of the two-primitive ones
            act = split[seg]
            pred = bk <= best[seg]
            left = j < mid[seg]
            lf, rt = np.nonzero(act & left & ~pred)[0], np.nonzero(act & ~left & pred)[0]
            nsw = np.bincount(seg[lf], minlength=K)
            assert np.array_equal(nsw, np.bincount(seg[rt], minlength=K))
            rt = rt[np.lexsort((-rt, seg[rt]))]                       # per node from the right end
            pa, pb_ = pos[lf], pos[rt]
            perm[pa], perm[pb_] = perm[pb_].copy(), perm[pa].copy()
            t2 = np.nonzero(two)[0]
            sw = t2[cd[off[t2] + 1] < cd[off[t2]]]
            perm[S[sw]], perm[S[sw] + 1] = perm[S[sw] + 1].copy(), perm[S[sw]].copy()
            # the counts
            for k in np.nonzero(interior)[0]:
                n = int(C[k])
                c[f"interior_{interior_class(n)}"] += 1
                if n in (256, 257, 2048, 2049):
                    c[f"interior_n{n}"] += 1
                c[f"axis{int(dim[k])}"] += 1
                c["maxdim_ties"] += int((ext[k] == ext[k].max()).sum() > 1)
                if not split[k]:
                    continue
                c["split_both" if over[k] and cheaper[k] else "split_forced" if over[k] else "split_cheaper"] += 1
                c["tied_min_cost"] += int(tied[k])
                c["empty_middle_bucket"] += int((counts[k, 1:11] == 0).any())
                c["no_swap"] += int(nsw[k] == 0)
                c["swaps_gt64"] += int(nsw[k] > 64)
                if n > TILE and nsw[k]:
                    swapped = np.concatenate([j[lf[seg[lf] == k]], j[rt[seg[rt] == k]]])
                    c["swaps_across_tile"] += int(any((swapped < b).any() and (swapped >= b).any() for b in range(TILE, n, TILE)))
            one = idx[single]
            got = np.concatenate([nodes["pmin"][one], nodes["pmax"][one]], 1)
            assert got.tobytes() == B[off[single]].tobytes(), f"level {d}: a one-primitive leaf's bounds are not its primitive's"
            c["leaf_single"] += len(one)
            for k in np.nonzero(~interior & ~single)[0]:
                n = int(C[k])
                rule = "flat" if flat[k] else "coincident" if coincide[k] else "cost"
                c[f"leaf_{rule}_{leaf_class(n)}"] += 1
                if check_leaf_bounds(nodes, int(idx[k]), B[off[k]:off[k] + n], c):
                    c[f"mixed_zero_leaves_{leaf_class(n)}"] += 1
    assert np.array_equal(perm, ordered_prims["id"]), "the replayed partitions end in another primitive order"
    check_interior_bounds(nodes, c)
    return {k: int(v) for k, v in c.items()}


# ---- HLBVH: buildHLBVH / emitLBVH / buildUpperSAH (aggregates.cpp:389-503, 626-723) ----------------------------------
HLBVH_KEYS = (("nodes", "leaves", "treelets", "single_leaf_treelets", "leaf_small", "leaf_identical_codes", "leaf_le64",
               "leaf_n64", "leaf_n65", "leaf_gt65", "identical_inside_treelet", "skipped_bits")
              + tuple(f"split_bit_{b}" for b in range(17, -1, -1)) + ("axis0", "axis1", "axis2", "upper_nodes",
                                                                       "upper_tied_costs", "upper_nan_costs",
                                                                       "mixed_zero_leaves", "mixed_zero_interior", "depth"))


def left_shift3(x):
    x = np.where(x == (1 << 10), x - 1, x).astype(np.uint32)          # util/math.h:99-112
    x = (x | (x << 16)) & np.uint32(0b00000011000000000000000011111111)
    x = (x | (x << 8)) & np.uint32(0b00000011000000001111000000001111)
    x = (x | (x << 4)) & np.uint32(0b00000011000011000011000011000011)
    x = (x | (x << 2)) & np.uint32(0b00001001001001001001001001001001)
    return x


def morton_codes(pb):
    """:391-408: 30-bit codes of the bounds centroids' offsets in the centroid bounds, scaled by 2^10."""
    with np.errstate(all="ignore"):
        cen = f32(.5) * pb[:, :3] + f32(.5) * pb[:, 3:]
        cmn, cmx = cen.min(0), cen.max(0)
        o = cen - cmn
        o = np.where(cmx > cmn, o / (cmx - cmn), o)
        q = (o * f32(1024)).astype(np.uint32)
    return (left_shift3(q[:, 2]) << 2) | (left_shift3(q[:, 1]) << 1) | left_shift3(q[:, 0])


def census_hlbvh(nodes, ordered_prims, prim_bounds, max_prims):
    """Recomputes the Morton codes as the builder does, ASSERTS that the ordered table is their stable sort, that every
    node inside a treelet splits at the highest bit in which its first and last code differ, at the first primitive
    whose bit differs, with axis = bit % 3, that leaves obey emitLBVH's rule, that every upper node is the
    minimum-cost split of buildUpperSAH over its treelets' boxes, and every stored box, and counts

    treelets, single_leaf_treelets   groups of equal top-12 code bits; those that are one leaf
    leaf_small / leaf_identical_codes   leaves closed by n < maxPrims / by bitIndex == -1 with n >= maxPrims
    leaf_le64, leaf_n64, leaf_n65, leaf_gt65   leaf sizes around the device's wavefront-fold threshold (kBigLeaf = 64)
    identical_inside_treelet         identical-code leaves (n >= maxPrims) that are not their treelet's root
    split_bit_B, axis0 / 1 / 2       interior nodes of treelets by split bit; by axis
    skipped_bits                     such nodes that passed over one or more bits in which their codes agree
    upper_nodes, upper_tied_costs, upper_nan_costs   buildUpperSAH nodes; with the minimum shared; with cost[0] NaN
    mixed_zero_leaves / _interior, depth."""
    pb = np.asarray(prim_bounds, np.float32).reshape(-1, 6)
    max_prims = min(255, max_prims)
    codes = morton_codes(pb)
    order = np.argsort(codes, kind="stable")
    assert np.array_equal(ordered_prims["id"], order), "the ordered table is not the stable sort by Morton code"
    sc = codes[order].astype(np.int64)
    B = pb[order]
    start, cnt, contig, depth, parent, _, _ = tree_shape(nodes)
    c = dict.fromkeys(HLBVH_KEYS, 0)
    c.update(nodes=len(nodes), leaves=int((nodes["nprims"] > 0).sum()), depth=int(depth.max()),
             treelets=len(np.unique(sc >> 18)))
    last = start + cnt - 1
    inside = contig & ((sc[start] >> 18) == (sc[last] >> 18))
    bit_of = np.full(len(nodes), -1)
    roots_under = [None] * len(nodes)
    for i in range(len(nodes)):
        n, leaf = int(cnt[i]), nodes["nprims"][i] > 0
        if not inside[i]:
            assert not leaf
            continue
        root = i == 0 or not inside[parent[i]]
        lo, hi = int(sc[start[i]]), int(sc[last[i]])
        if leaf:
            c["single_leaf_treelets"] += root
            if n < max_prims:
                c["leaf_small"] += 1
            else:
                assert lo == hi, f"leaf {i}: {n} >= maxPrims primitives with different codes"
                c["leaf_identical_codes"] += 1
                c["identical_inside_treelet"] += not root
            c["leaf_le64"] += n <= 64
            c["leaf_n64"] += n == 64
            c["leaf_n65"] += n == 65
            c["leaf_gt65"] += n > 65
            check_leaf_bounds(nodes, i, B[start[i]:start[i] + n], c)
            continue
        assert n >= max_prims and lo != hi, f"node {i}: interior against emitLBVH's leaf rule"
        bit = (lo ^ hi).bit_length() - 1
        assert bit < 18 and nodes["axis"][i] == bit % 3
        first_bit = (sc[start[i]:start[i] + n] >> bit) & 1
        assert cnt[i + 1] == int((first_bit == first_bit[0]).sum()), f"node {i}: not split where bit {bit} flips"
        bit_of[i] = bit
        c[f"split_bit_{bit}"] += 1
        c[f"axis{bit % 3}"] += 1
        c["skipped_bits"] += bit < (17 if root else bit_of[parent[i]] - 1)
    assert int((inside & np.concatenate([[True], ~inside[parent[1:]]])).sum()) == c["treelets"]
    # buildUpperSAH over the treelet roots (their stored boxes), bottom-up for the sets
    with np.errstate(all="ignore"):
        for i in range(len(nodes) - 1, -1, -1):
            if inside[i]:
                roots_under[i] = [i] if (i == 0 or not inside[parent[i]]) else None
                continue
            lf, rt = roots_under[i + 1], roots_under[int(nodes["offset"][i])]
            mine = roots_under[i] = lf + rt
            rmn, rmx = nodes["pmin"][mine], nodes["pmax"][mine]
            cen = (rmn + rmx) * f32(.5)
            cmn, cmx = cen.min(0), cen.max(0)
            dim = int(max_dimension(cmx - cmn))
            assert cmx[dim] != cmn[dim] and nodes["axis"][i] == dim
            bk = np.minimum((f32(12) * ((cen[:, dim] - cmn[dim]) / (cmx[dim] - cmn[dim]))).astype(np.int64), 11)
            total = area_of(rmn.min(0), rmx.max(0))
            cost = np.zeros(11, f32)
            for s in range(11):
                a, b = bk <= s, bk > s
                a0 = area_of(rmn[a].min(0), rmx[a].max(0)) if a.any() else area_of(np.full(3, FLT_MAX, f32), np.full(3, -FLT_MAX, f32))
                a1 = area_of(rmn[b].min(0), rmx[b].max(0)) if b.any() else area_of(np.full(3, FLT_MAX, f32), np.full(3, -FLT_MAX, f32))
                cost[s] = f32(.125) + (f32(int(a.sum())) * a0 + f32(int(b.sum())) * a1) / total
            best, min_cost = 0, cost[0]
            for s in range(1, 11):
                if cost[s] < min_cost:
                    best, min_cost = s, cost[s]
            assert sorted(lf) == sorted(k for k, q in zip(mine, bk) if q <= best), f"upper node {i}: not the minimum-cost split"
            c["upper_nodes"] += 1
            c["upper_tied_costs"] += int((cost == min_cost).sum() > 1)
            c["upper_nan_costs"] += int(np.isnan(cost[0]))
    if (nodes["nprims"] == 0).any():
        check_interior_bounds(nodes, c)
    return {k: int(v) for k, v in c.items()}


def census(nodes, ordered_prims, verts, prim_bounds, max_prims, method):
    """The census of a host-built tree: census_sah or census_hlbvh by the split method.  prim_bounds: (n, 6) per
    primitive id, or None for triangles and patches, whose boxes are then folded from verts."""
    if prim_bounds is None:
        prim_bounds = np.zeros((len(ordered_prims), 6), np.float32)
        prim_bounds[ordered_prims["id"]] = prim_boxes(ordered_prims, verts)
    return {"sah": census_sah, "hlbvh": census_hlbvh}[method](nodes, ordered_prims, prim_bounds, max_prims)


# ---- the cases: scene, builder parameters, the census lines that must not be zero ------------------------------------
def _soup_with(extra, seed):
    v, p = ss.random_soup(4000, 0, seed)
    return ss.merge(extra, (v, p))


@functools.lru_cache(maxsize=None)
def path_scene(name):
    """(verts, prims, primitive boxes) of a scene, built once per session and never modified."""
    if name.startswith("soup") and name[4:].isdigit():
        made = ss.random_soup(int(name[4:]), 0, 100 + int(name[4:]))
    elif name.startswith("spine_pairs"):
        made = ss.bvh_spine(int(name[11:]), k0=-35, pairs=True)
    elif name.startswith("spine"):
        made = ss.bvh_spine(int(name[5:]), k0=-35)
    else:
        made = {
            "leaf_rules": lambda: ss.bvh_leaf_rules(50),
            "lattice": lambda: ss.bvh_lattice(16),
            "tiny_soup": lambda: (lambda v, p: ((v * f32(1e-25)).astype(f32), p))(*ss.random_soup(500, 0, 3)),
            "huge_soup": lambda: (lambda v, p: ((v * f32(1e19)).astype(f32), p))(*ss.random_soup(500, 0, 3)),
            "coincident": lambda: ss.coincident_centroids(300, 5),
            "cluster_and_outlier": lambda: ss.bvh_cluster_and_outlier(61),
            "sparse_soup": lambda: ss.random_soup(7500, 0, 41, extent=400.0, size=0.01),
            "all_cells": lambda: ss.bvh_all_cells(62),
            "code_runs": lambda: ss.bvh_code_runs(63),
            "dense_cell": lambda: ss.bvh_dense_cell(64),
            "signed_zeros": lambda: _soup_with(ss.merge(ss.bvh_signed_zero_cluster(700, 12), ss.bvh_signed_zero_row(96, 14)), 13),
        }[name]()
    verts, prims = made
    assert np.array_equal(prims["id"], np.arange(len(prims)))         # the censuses read ids as positions
    out = (np.ascontiguousarray(verts, np.float32), prims, prim_boxes(prims, verts))
    for a in out:
        a.setflags(write=False)
    return out


def _case(family, scene_name, method, premise, max_prims=(4,)):
    return [pytest.param(family, scene_name, method, m, premise, id=f"{scene_name}-{method}-max_prims={m}") for m in max_prims]


# premise: census keys that must be > 0 (a "=N" suffix: must equal N).  The premises are the issue's; generators and
# parameters were tuned until they hold, never the other way round.  What each family is there for on the device:
PATH_CASES = (
    # k_sah_subtrees' three leaf folds (registers, n <= 64; 64 chunks, n > 64) under each of the three leaf rules, big
    # nodes that do not split (phase A's "delegated" node) inside a tree, the first-of-equals rule of both leaf
    # folds and of k_sah_level_bounds, interior nodes of every size class of the breadth-first phase
    _case("sah_leaf_rules", "leaf_rules", "sah",
          ("leaf_flat_3_64", "leaf_flat_65_256", "leaf_flat_gt256", "leaf_coincident_3_64", "leaf_coincident_65_256",
           "leaf_coincident_gt256", "mixed_zero_leaves_3_64", "mixed_zero_leaves_65_256", "mixed_zero_leaves_gt256",
           "mixed_zero_interior", "interior_2", "interior_3_64",
           "interior_65_256", "interior_257_2048", "interior_gt2048", "split_forced", "split_both", "swaps_gt64",
           "no_swap", "axis0", "axis1", "axis2"), max_prims=(1,))
    + _case("sah_leaf_rules", "leaf_rules", "sah",
            ("leaf_cost_3_64", "leaf_flat_65_256", "leaf_coincident_gt256", "split_cheaper", "split_forced", "split_both",
             "mixed_zero_leaves_3_64", "mixed_zero_leaves_65_256", "mixed_zero_leaves_gt256", "mixed_zero_interior"), max_prims=(4,))
    + _case("sah_leaf_rules", "leaf_rules", "sah",
            ("leaf_cost_3_64", "leaf_cost_65_256", "leaf_flat_gt256", "leaf_coincident_65_256", "split_cheaper",
             "mixed_zero_leaves_3_64", "mixed_zero_leaves_65_256", "mixed_zero_leaves_gt256", "mixed_zero_interior"), max_prims=(255,))
    # the root on each side of every threshold of the device code: 1 / 2 / 3 (leaf, nth_element of two, buckets), 64 | 65
    # (registers | loops over the range), 256 | 257 (wavefront | breadth-first), 2048 | 2049 (one tile | two)
    + _case("sah_sizes", "soup1", "sah", ("nodes=1", "leaf_single=1"))
    + _case("sah_sizes", "soup2", "sah", ("interior_2=1", "nodes=3"))
    + _case("sah_sizes", "soup3", "sah", ("interior_3_64", "interior_2=1"))
    + _case("sah_sizes", "soup64", "sah", ("interior_3_64",))
    + _case("sah_sizes", "soup65", "sah", ("interior_65_256",))
    + _case("sah_sizes", "soup256", "sah", ("interior_n256=1",))
    + _case("sah_sizes", "soup257", "sah", ("interior_n257=1",))
    + _case("sah_sizes", "soup2048", "sah", ("interior_n2048=1",))
    + _case("sah_sizes", "soup2049", "sah", ("interior_n2049=1",))
    + _case("sah_sizes", "soup4097", "sah", ("interior_gt2048", "swaps_across_tile", "swaps_gt64"), max_prims=(1, 4))
    # equal costs, equal extents: the first minimum and MaxDimension's fall-through, slices that need no swap
    + _case("sah_ties", "lattice", "sah", ("tied_min_cost", "maxdim_ties", "no_swap", "interior_gt2048"), max_prims=(1, 4))
    # the pending-second-child stack of k_sah_subtrees: exactly full, one beyond, the longest chain of normal floats
    + _case("sah_spine", "spine65", "sah", ("left_spine=64", "depth=64", "tied_min_cost", "empty_middle_bucket"), max_prims=(1,))
    + _case("sah_spine", "spine66", "sah", ("left_spine=65", "depth=65"), max_prims=(1,))
    + _case("sah_spine", "spine71", "sah", ("left_spine=70", "depth=70"), max_prims=(1,))
    # ... and 70 pairs coming off the chain (69 splits and the last pair: a left spine of 70): an entry popped from
    # beyond the 64th is an interior node that pushes again (the pairs behind 64 .. 68 pending second children)
    + _case("sah_spine", "spine_pairs70", "sah", ("second_child_interior_pending_ge64=5", "left_spine=70", "depth=70"), max_prims=(1,))
    # every surface area underflows to 0: the root is a flat leaf of 500
    + _case("sah_range", "tiny_soup", "sah", ("nodes=1", "leaf_flat_gt256=1"))
    # HLBVH: k_classify's leaf rule, k_leaf_bounds | k_big_leaf_bounds on both sides of 64, k_karras / k_emit on every
    # split bit, k_interior_bounds' first-of-equals rule, the host's upper SAH with one .. 4096 treelets
    + _case("hlbvh_treelets", "coincident", "hlbvh", ("treelets=1", "nodes=1", "leaf_identical_codes=1", "leaf_gt65=1"))
    + _case("hlbvh_treelets", "soup1", "hlbvh", ("treelets=1", "nodes=1", "leaf_small=1"))
    + _case("hlbvh_treelets", "cluster_and_outlier", "hlbvh", ("treelets=2", "upper_nodes=1", "single_leaf_treelets=1", "split_bit_17"))
    + _case("hlbvh_treelets", "sparse_soup", "hlbvh", ("single_leaf_treelets", "upper_nodes", "upper_tied_costs"))
    + _case("hlbvh_treelets", "all_cells", "hlbvh", ("treelets=4096", "upper_nodes=4095", "upper_tied_costs"))
    + _case("hlbvh_leaves", "code_runs", "hlbvh", ("leaf_n64", "leaf_n65", "leaf_gt65", "leaf_le64", "identical_inside_treelet",
                                                   "leaf_identical_codes"), max_prims=(1, 2))
    # (with max_prims 255 the runs of 64 and 65 end up in larger n < maxPrims leaves; the run of 700 stays)
    + _case("hlbvh_leaves", "code_runs", "hlbvh", ("leaf_small", "leaf_gt65", "leaf_identical_codes=1", "identical_inside_treelet=1"),
            max_prims=(255,))
    + _case("hlbvh_bits", "dense_cell", "hlbvh", tuple(f"split_bit_{b}" for b in range(18)) + ("skipped_bits", "axis0", "axis1", "axis2"),
            max_prims=(1,))
    + _case("hlbvh_bits", "dense_cell", "hlbvh", ("skipped_bits", "leaf_small", "split_bit_17", "split_bit_3"), max_prims=(4,))
    + _case("hlbvh_zeros", "signed_zeros", "hlbvh", ("mixed_zero_leaves", "mixed_zero_interior", "leaf_gt65"))
    + _case("hlbvh_zeros", "leaf_rules", "hlbvh", ("mixed_zero_leaves", "mixed_zero_interior", "leaf_gt65", "leaf_identical_codes"))
    # the upper SAH's costs are inf / inf = NaN: best stays 0, the build still ends
    + _case("hlbvh_range", "huge_soup", "hlbvh", ("upper_nan_costs", "upper_nodes"))
)
FAMILIES = sorted({p.values[0] for p in PATH_CASES})
TRACED = ("sah_leaf_rules", "sah_ties", "hlbvh_leaves")
KNOB = "NNBVH_SAH_SMALL"   # where the breadth-first phase hands over to one wavefront per subtree: speed only


@functools.lru_cache(maxsize=None)
def host_tree(name, method, max_prims):
    verts, prims, _ = path_scene(name)
    t = build_tree(prims, verts, max_prims, method)
    for a in (t.nodes, t.ordered_prims):
        a.setflags(write=False)
    return t


def census_of(name, method, max_prims):
    t = host_tree(name, method, max_prims)
    verts, _, boxes = path_scene(name)
    c = census(t.nodes, t.ordered_prims, verts, boxes, max_prims, method)
    assert c["depth"] == t.depth, f"{name}: the builder reports depth {t.depth}, the walk finds {c['depth']}"
    return t, c


@pytest.mark.parametrize("family", FAMILIES)
def test_census_every_scene_reaches_the_path_it_is_named_for(family):
    """The host builder's tree of every case of the family holds what the case is there for (no GPU)."""
    for p in PATH_CASES:
        fam, name, method, max_prims, premise = p.values
        if fam != family:
            continue
        _, c = census_of(name, method, max_prims)
        print(f"{p.id}: " + " ".join(f"{k}={v}" for k, v in c.items() if v))
        for want in premise:
            key, _, exact = want.partition("=")
            assert (c[key] == int(exact)) if exact else (c[key] > 0), f"{p.id}: census {want} does not hold: {c}"


def _node(lo, hi, offset, nprims, axis):
    n = np.zeros(1, NODE_DTYPE)
    n["pmin"], n["pmax"], n["offset"], n["nprims"], n["axis"] = lo, hi, offset, nprims, axis
    return n


def test_census_counts_a_hand_made_sah_tree():
    """The SAH census on a tree small enough to count by hand, max_prims 1.  Unit cubes at x = 0, 1 and 10: centroid
    offsets 0, 0.1 and 1 fall into buckets 0, 1 and 11.  Split 0 costs 1 * 6 + 2 * 42 = 90, splits 1 .. 10 all cost
    2 * 10 + 1 * 6 = 26 (buckets 2 .. 10 are empty): the first of the tied minima, split 1, puts two primitives on the
    left without a swap; 1/2 + 26 / 46 < 3 and 3 > max_prims, so both reasons to split hold.  The left child is the
    nth_element of two, already in order.  Cube 0 starts at y = +0 and cube 1 at y = -0: their parent keeps the first
    child's +0 (one interior node with a zero of both signs); the root gets +0 from both sides."""
    lo = np.array([[0, 0.0, 0], [1, -0.0, 0], [10, 0.0, 0]], f32)
    hi = lo + f32(1)
    pb = np.concatenate([lo, hi], 1)
    nodes = np.concatenate([_node(lo[0], [11, 1, 1], 4, 0, 0), _node(lo[0], hi[1], 3, 0, 0), _node(lo[0], hi[0], 0, 1, 0),
                            _node(lo[1], hi[1], 1, 1, 0), _node(lo[2], hi[2], 2, 1, 0)])
    ordered = np.zeros(3, [("id", "<i4")])
    ordered["id"] = [0, 1, 2]
    c = census_sah(nodes, ordered, pb, 1)
    want = dict.fromkeys(SAH_KEYS, 0)
    want.update(nodes=5, leaves=3, leaf_single=3, interior_2=1, interior_3_64=1, split_both=1, axis0=2, tied_min_cost=1,
                empty_middle_bucket=1, no_swap=1, mixed_zero_interior=1, depth=2, left_spine=2)
    assert c == want
    # ... and it refuses a tree that is not the builder's: the same nodes with the split one bucket early
    wrong = np.concatenate([_node(lo[0], [11, 1, 1], 2, 0, 0), _node(lo[0], hi[0], 0, 1, 0), _node(lo[1], hi[2], 4, 0, 0),
                            _node(lo[1], hi[1], 1, 1, 0), _node(lo[2], hi[2], 2, 1, 0)])
    with pytest.raises(AssertionError, match="first children differ in size"):
        census_sah(wrong, ordered, pb, 1)


def test_census_counts_a_hand_made_hlbvh_tree():
    """The HLBVH census on four unit cubes at x = 0, 1, 14 and 15 (y and z shared: offsets and code bits 0 there),
    max_prims 1.  Centroid offsets 0, 1/15, 14/15, 1 scale to 0, 68, 955 and 1024 -> 1023: x cells 0, 1, 14 and 15 of
    the treelet grid, so four treelets of one leaf each (n = 1 is not < max_prims: closed by identical codes) under
    three upper nodes.  The upper root sees centroids 0.5, 1.5, 14.5, 15.5: buckets 0, 0, 11, 11, every split costs
    the same (tied), the first wins and halves the set; each half holds two treelets in buckets 0 and 11, tied again."""
    lo = np.array([[0, 0, 0], [1, 0, 0], [14, 0, 0], [15, 0, 0]], f32)
    hi = lo + f32(1)
    pb = np.concatenate([lo, hi], 1)
    nodes = np.concatenate([_node(lo[0], hi[3], 4, 0, 0), _node(lo[0], hi[1], 3, 0, 0), _node(lo[0], hi[0], 0, 1, 0),
                            _node(lo[1], hi[1], 1, 1, 0), _node(lo[2], hi[3], 6, 0, 0), _node(lo[2], hi[2], 2, 1, 0),
                            _node(lo[3], hi[3], 3, 1, 0)])
    ordered = np.zeros(4, [("id", "<i4")])
    ordered["id"] = [0, 1, 2, 3]
    c = census_hlbvh(nodes, ordered, pb, 1)
    want = dict.fromkeys(HLBVH_KEYS, 0)
    want.update(nodes=7, leaves=4, treelets=4, single_leaf_treelets=4, leaf_identical_codes=4, leaf_le64=4, upper_nodes=3,
                upper_tied_costs=3, depth=2)
    assert c == want


# ---- non-finite SAH costs: refused by both builders in the same words ---------------------------------------------
COSTS_TEXT = "coordinates too large for the SAH costs"


def huge(scale):
    verts, prims = ss.random_soup(500, 0, 3)
    return (verts * f32(scale)).astype(f32), prims


def refusal_of(fn, *args, **kw):
    with pytest.raises(NNBVHError, match=COSTS_TEXT) as e:
        fn(*args, **kw)
    assert "internal error" not in str(e.value)
    return str(e.value).split(": ", 1)[1]     # without the entry point's own name


@pytest.mark.parametrize("scale", [1e17, 1e25])
def test_host_sah_refuses_coordinates_whose_costs_are_all_infinite(scale):
    """count * surface area is +inf for every split: no cost is below the initial minimum, the reference's
    minCostSplitBucket stays -1, its partition puts nothing on the left and buildRecursive never ends.  The host
    builder says so (it used to overflow the stack); the other split methods build the input."""
    verts, prims = huge(scale)
    for max_prims in (1, 4, 255):
        text = refusal_of(build_tree, prims, verts, max_prims, "sah")
        assert "the reference does not terminate" in text
    for method in ("middle", "equal", "hlbvh"):
        assert build_tree(prims, verts, 4, method).nodes["nprims"].sum() == len(prims)


# ---- GPU: the device builders on every case ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family,name,method,max_prims,premise", PATH_CASES)
def test_device_build_equals_the_host_builder_on_every_path(family, name, method, max_prims, premise, monkeypatch):
    """Byte for byte (-0 is not +0), depth included, twice; SAH additionally with everything breadth-first (2), with
    the hand-over at 64, with the whole tree in one wavefront (2^30) and at the default: the threshold is speed only.
    For three families the device-built AND device-baked scene also carries rays to the oracle's answers on the
    host-built tree: the order inside multi-primitive leaves decides ties and prim_tests."""
    verts, prims, _ = path_scene(name)
    host = host_tree(name, method, max_prims)
    what = f"{name} max_prims {max_prims}"
    monkeypatch.delenv(KNOB, raising=False)
    _, dev = same_tree(prims, verts, max_prims, what=what, method=method, host=host)
    same_tree(prims, verts, max_prims, what=what + " built twice", method=method, host=dev)
    if method == "sah":
        for knob in (2, 64, 1 << 30):
            monkeypatch.setenv(KNOB, str(knob))
            same_tree(prims, verts, max_prims, what=f"{what} {KNOB}={knob}", method=method, host=host)
        monkeypatch.delenv(KNOB)
    if family not in TRACED:
        return
    lo, hi = verts.min(0), verts.max(0)
    pad = 0.1 * (hi - lo) + 1
    rays = np.concatenate([scene.random_rays(3000, lo - pad, hi + pad, 51), scene.random_rays(1000, lo, hi, 52, tmax=0.5),
                           ss.edge_case_rays(verts, prims, 53, n=1024)])
    agg = BVHAggregate.build_on_device(prims, verts, max_prims, method)
    try:
        got = agg.Intersect(rays)
        occ, vis, tst = agg.IntersectP(rays, counts=True)
    finally:
        agg.close()
    exp = ob.closest(host.nodes, host.ordered_prims, verts, rays)
    eo, ev, et = ob.any_hit(host.nodes, host.ordered_prims, verts, rays)
    assert got.tobytes() == exp.tobytes(), f"{what}: closest-hit records differ from the oracle on the host-built tree"
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et), f"{what}: any-hit differs"


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1e17, 1e25])
def test_device_sah_refuses_what_the_host_builder_refuses_in_the_same_words(scale, monkeypatch):
    verts, prims = huge(scale)
    want = refusal_of(build_tree, prims, verts, 4, "sah")
    for knob in (None, 2, 1 << 30):
        if knob is None:
            monkeypatch.delenv(KNOB, raising=False)
        else:
            monkeypatch.setenv(KNOB, str(knob))
        assert refusal_of(build_tree_gpu, prims, verts, 4, split_method="sah") == want
        assert refusal_of(BVHAggregate.build_on_device, prims, verts, 4, "sah") == want
    monkeypatch.delenv(KNOB)
    same_tree(prims, verts, what=f"soup x {scale}", method="hlbvh")     # HLBVH builds it on both sides


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["spine66", "spine71"])
def test_a_tree_deeper_than_the_traversal_stack_is_built_but_not_baked(name):
    """The builders return the chain's tree (the path cases above compare it); scene creation keeps refusing a tree
    deeper than 64 on the host-tree route and on the device route."""
    verts, prims, _ = path_scene(name)
    host = host_tree(name, "sah", 1)
    assert host.depth > 64
    with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
        BVHAggregate.from_tree(host.nodes, host.ordered_prims, verts)
    with pytest.raises(NNBVHError, match="tree deeper than the 64-entry traversal stack"):
        BVHAggregate.build_on_device(prims, verts, 1, "sah")
    v65, p65, _ = path_scene("spine65")                                  # depth 64: exactly the stack, accepted
    BVHAggregate.build_on_device(p65, v65, 1, "sah").close()
