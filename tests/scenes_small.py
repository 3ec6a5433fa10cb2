"""Small seeded scenes shared by the parity tests (inputs only)."""
import collections
import os

import numpy as np

from nn_bvh_amd import make_prims, scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def scene_blob(name):
    """(verts, tris) of a reference scene: data/<name>.npz where the build made it, else the copy kept under
    tests/golden/ (killeroos only, tools/make_killeroos.py's output: the larger scenes are not kept in the
    repository); None if neither exists."""
    if os.path.exists(scene.blob_path(name)):
        return scene.load_blob(name)
    path = os.path.join(GOLDEN, name + ".npz")
    if not os.path.exists(path):
        return None
    with np.load(path) as z:
        return z["verts"], z["tris"]


def random_soup(n_tris=2000, n_patches=0, seed=0, extent=10.0, size=0.6):
    """Random triangle (+ bilinear patch) soup in a box."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-extent, extent, size=(n_tris, 1, 3))
    tv = (c + rng.uniform(-size, size, size=(n_tris, 3, 3))).reshape(-1, 3)
    tri = np.arange(3 * n_tris, dtype=np.int32).reshape(n_tris, 3)
    verts = [tv]
    patch = None
    if n_patches:
        c = rng.uniform(-extent, extent, size=(n_patches, 1, 3))
        eu = rng.uniform(-size, size, size=(n_patches, 1, 3))
        ev = rng.uniform(-size, size, size=(n_patches, 1, 3))
        tw = rng.uniform(-0.3 * size, 0.3 * size, size=(n_patches, 1, 3))
        pv = np.concatenate([c, c + eu, c + ev, c + eu + ev + tw], 1).reshape(-1, 3)
        patch = (np.arange(4 * n_patches, dtype=np.int32) + 3 * n_tris).reshape(n_patches, 4)
        verts.append(pv)
    verts = np.concatenate(verts).astype(np.float32)
    return verts, make_prims(tri, patch)


def grid_mesh(n=48, seed=0, bump=0.4):
    """Connected height-field mesh: shared vertices/edges, so rays graze edges and hit
    shared vertices (the watertightness / tie-breaking cases)."""
    rng = np.random.default_rng(seed)
    x, z = np.meshgrid(np.linspace(-5, 5, n + 1), np.linspace(-5, 5, n + 1), indexing="ij")
    y = bump * rng.standard_normal(x.shape)
    verts = np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    a = (i * (n + 1) + j).ravel()
    tri = np.stack([a, a + n + 1, a + n + 2, a, a + n + 2, a + 1], 1).reshape(-1, 3)
    return verts, make_prims(tri.astype(np.int32))


def coincident_centroids(n=200, seed=0):
    """Many primitives with the same centroid -> one big leaf (> maxnodeprims), the
    coffee_maker 64-prim-leaf situation (aggregates.cpp:225-233)."""
    rng = np.random.default_rng(seed)
    # the builder's centroid is the BOUNDS centroid (aggregates.cpp:92): give every triangle the
    # box [c - h, c + h] (h a multiple of 1/64, so .5*min + .5*max == c exactly)
    h = (rng.integers(1, 64, size=(n, 3)) / 64.0).astype(np.float32)
    w = (rng.integers(-63, 64, size=(n, 3)) / 64.0).astype(np.float32) * h
    c = np.array([1.0, 2.0, 3.0], np.float32)
    verts = np.stack([c - h, c + h, c + w], 1).reshape(-1, 3).astype(np.float32)
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    return verts, make_prims(tri)


def edge_case_rays(verts, prims, seed=0, n=2048):
    """Rays built to sit on the comparison boundaries: axis-aligned (two zero components),
    one zero component, aimed exactly at shared vertices / edge midpoints, origins inside the
    scene box, shadow-style un-normalised d with tMax = 1 - 1e-4, tiny and huge tMax."""
    from nn_bvh_amd import make_rays
    rng = np.random.default_rng(seed)
    lo, hi = verts.min(0), verts.max(0)
    ext = hi - lo
    k = n // 8
    parts = []
    # axis-aligned through random vertices
    tgt = verts[rng.integers(0, len(verts), k)]
    ax = rng.integers(0, 3, k)
    d = np.zeros((k, 3), np.float32)
    d[np.arange(k), ax] = rng.choice([-1.0, 1.0], k)
    parts.append(make_rays(tgt - d * (ext.max() * 2), d))
    # one zero component
    o = lo + rng.random((k, 3)) * ext + ext * np.array([0, 2, 0])
    d = rng.normal(size=(k, 3)).astype(np.float32)
    d[np.arange(k), rng.integers(0, 3, k)] = 0
    d[:, 1] = -np.abs(d[:, 1]) - 0.1
    parts.append(make_rays(o, d))
    # exactly at vertices from outside
    o = (lo + rng.random((k, 3)) * ext + ext * 1.5).astype(np.float32)
    tgt = verts[rng.integers(0, len(verts), k)]
    parts.append(make_rays(o, tgt - o))
    # at edge midpoints of primitives
    p = prims[rng.integers(0, len(prims), k)]
    mid = (verts[p["v"][:, 0]] + verts[p["v"][:, 1]]) * np.float32(0.5)
    parts.append(make_rays(o, mid - o))
    # origins inside the box, random directions
    o2 = (lo + rng.random((k, 3)) * ext).astype(np.float32)
    parts.append(make_rays(o2, rng.normal(size=(k, 3))))
    # shadow style
    a = (lo + rng.random((k, 3)) * ext).astype(np.float32)
    b = (lo + rng.random((k, 3)) * ext).astype(np.float32)
    parts.append(make_rays(a, b - a, tmax=np.float32(1 - 1e-4)))
    # short tMax
    parts.append(make_rays(o2, rng.normal(size=(k, 3)), tmax=rng.uniform(0.01, 2.0, k)))
    # negative zero and denormal direction components
    d = rng.normal(size=(k, 3)).astype(np.float32)
    d[::2, 0] = -0.0
    d[1::2, 2] = 1e-42
    parts.append(make_rays(o2, d))
    return np.concatenate(parts)


# ---- skewed chains: scenes whose rays provably keep up to 64 nodes pending -------------------------------------
# (tests/test_stack_limits.py; the CPU tests there prove the depths with the oracle's pending-depth output)
Chain = collections.namedtuple("Chain", "verts prims nodes normals uvs prim_alpha leaf_lo leaf_hi")
TwoLevelChain = collections.namedtuple("TwoLevelChain", "verts prims nodes instances n_top a b outer_lo outer_hi "
                                                        "child_lo child_hi")
KdChain = collections.namedtuple("KdChain", "verts prims nodes prim_indices bounds normals uvs prim_alpha splits")

TRI_KINDS = (0, 4, 5, 6, 7)
PATCH_KINDS = (1, 8, 9, 10, 11, 12, 13, 14, 15)
ALPHAS = np.array([0.0, 0.25, 0.5, 0.9, 1.0, 1.5], np.float32)
LEAF_MIXES = {  # kind of leaf k = mix[k % len(mix)]
    "tri": (0,),
    "patch": (0, 1, 1),
    "alpha_tri": (4, 0, 5, 4, 6, 7),
    "alpha_patch": (8, 0, 9, 1, 10, 11, 4, 12, 13, 14, 15),
    "host": (0, 0, 3, 0, 1, 0, 0),
    "host_tri": (0, 0, 3, 0, 0),  # kind 3 leaves that keep their triangle (the same scene as triangles: the oracle's)
}


def chain_nodes(lo, hi, node_base=0, prim_base=0):
    """LinearBVHNode array of a maximally skewed tree over leaves with the boxes lo[k] / hi[k], one primitive each:
    node 2k = interior k (first child: leaf k at 2k + 1, second child: interior k + 1 at 2k + 2), the last node =
    the last leaf; every interior splits along x.  node_base / prim_base: where the tree sits in shared arrays."""
    from nn_bvh_amd import NODE_DTYPE
    n_leaves = len(lo)
    nodes = np.zeros(2 * n_leaves - 1, NODE_DTYPE)
    for k in range(n_leaves - 1):
        nodes[2 * k]["pmin"], nodes[2 * k]["pmax"] = lo[k:].min(0), hi[k:].max(0)
        nodes[2 * k]["offset"], nodes[2 * k]["nprims"], nodes[2 * k]["axis"] = node_base + 2 * k + 2, 0, 0
        nodes[2 * k + 1]["pmin"], nodes[2 * k + 1]["pmax"] = lo[k], hi[k]
        nodes[2 * k + 1]["offset"], nodes[2 * k + 1]["nprims"] = prim_base + k, 1
    nodes[-1]["pmin"], nodes[-1]["pmax"] = lo[-1], hi[-1]
    nodes[-1]["offset"], nodes[-1]["nprims"] = prim_base + n_leaves - 1, 1
    return nodes


def _tube_leaf(rng, x, n_verts):
    """Vertices of a triangle (3) or bilinear patch (4) at x inside the tube [-1, 1]^2 around the x axis.  Two kinds
    of leaf, drawn per leaf: with probability 0.85 a WALL primitive: its vertices are random points of the square's
    perimeter squeezed into the strip of width 0.5 along one wall (|y| or |z| in [0.5, 1]), which a ray within 0.45 of
    the axis cannot meet; else (0.15) an AXIS primitive: its vertices are random points of [-0.7, 0.7]^2 around the
    axis, which some of those rays meet and others miss.  A chain ray therefore misses most leaves' primitives and
    has a fair chance to hit each of the few axis ones: over 65 leaves most rays hit something, at a depth that
    varies from ray to ray.  The x coordinates are jittered by up to 0.3 (a patch is twisted: the ray spawned off its
    surface after a rejected alpha hit can meet it again)."""
    out = []
    side, off = rng.integers(0, 4), rng.random() < 0.85
    for _ in range(n_verts):
        s, t = rng.integers(0, 4), rng.uniform(-1.0, 1.0)
        y, z = ((t, -1.0), (t, 1.0), (-1.0, t), (1.0, t))[s]
        if off:  # squeezed into the half-width strip along wall `side`
            y, z = ((y, 0.25 * z - 0.75), (y, 0.25 * z + 0.75), (0.25 * y - 0.75, z), (0.25 * y + 0.75, z))[side]
        else:  # a small shape somewhere around the axis: some of the rays meet it
            y, z = rng.uniform(-0.7, 0.7, 2)
        out.append((x + rng.uniform(-0.3, 0.3), y, z))
    return out


def chain_tree(depth, rng, tube=False, leaves="tri", extras=False, x0=0.0):
    """A maximally skewed tree: every interior node has one leaf child (first) and one interior child (second),
    `depth` edges deep, built by hand in the LinearBVHNode layout; leaf k sits at x = x0 + 2 k.  A ray with d.x < 0
    enters the interior child first and keeps one leaf pending per level: `depth` entries at the deepest leaf.

    tube: every leaf's box is the cross-section [-1, 1]^2 around the x axis times the primitive's x extent, and the
    primitive lies inside it with its vertices on the tube's walls (see _tube_leaf; the boxes are conservative, as a
    caller's may be), so that a ray that stays within 0.45 of the axis crosses EVERY leaf box by a margin, whatever
    its tMax, and still misses most primitives.
    leaves: a key of LEAF_MIXES or a sequence of primitive kinds, cycled over the leaves: 0 triangle, 1 bilinear patch,
    3 host-only (its bounds are the caller's: the tube's cross-section around its x; in the "host_tri" mix it keeps a
    triangle's vertices in v, which the device never reads, so the same arrays with kind 0 are the oracle's scene), 4 .. 7 alpha-tested triangles
    (the alpha in v[3]; 6 / 7 read the normals), 8 .. 15 alpha-tested patches (prim_alpha; normals, uvs).
    extras: return a Chain (normals / uvs / prim_alpha per vertex / vertex / primitive, the leaf boxes) instead of
    (verts, prims, nodes)."""
    from nn_bvh_amd import PRIM_DTYPE, make_prims
    n_leaves = depth + 1
    x = x0 + np.arange(n_leaves, dtype=np.float32) * 2.0
    if not tube and leaves == "tri":  # the form test_gpu_parity's depth tests have always used
        c = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)[:, None, :]
        verts = (c + rng.uniform(-0.7, 0.7, size=(n_leaves, 3, 3))).reshape(-1, 3).astype(np.float32)
        prims = make_prims(np.arange(3 * n_leaves, dtype=np.int32).reshape(n_leaves, 3))
        lo = verts.reshape(n_leaves, 3, 3).min(1)
        hi = verts.reshape(n_leaves, 3, 3).max(1)
        nodes = chain_nodes(lo, hi)
        if extras:
            return Chain(verts, prims, nodes, None, None, None, lo, hi)
        return verts, prims, nodes
    assert tube, "leaf kinds other than triangles come in the tube form"
    mix = LEAF_MIXES[leaves] if isinstance(leaves, str) else tuple(leaves)
    verts, lo, hi = [], np.zeros((n_leaves, 3), np.float32), np.zeros((n_leaves, 3), np.float32)
    prims = np.zeros(n_leaves, PRIM_DTYPE)
    prims["id"] = np.arange(n_leaves)
    alpha = np.ones(n_leaves, np.float32)
    for k in range(n_leaves):
        kind = mix[k % len(mix)]
        prims[k]["kind"] = kind
        if kind == 3 and leaves != "host_tri":
            lo[k], hi[k] = (x[k] - 0.3, -1, -1), (x[k] + 0.3, 1, 1)
            continue
        nv = 3 if kind in TRI_KINDS or kind == 3 else 4
        v = np.array(_tube_leaf(rng, float(x[k]), nv), np.float32)
        prims[k]["v"][:nv] = len(verts) + np.arange(nv)
        verts.extend(v)
        lo[k], hi[k] = (v[:, 0].min(), -1, -1), (v[:, 0].max(), 1, 1)
        if kind >= 4:
            alpha[k] = ALPHAS[rng.integers(0, len(ALPHAS))]
            if kind <= 7:
                prims[k]["v"][3] = alpha[k:k + 1].view(np.int32)[0]
    verts = np.array(verts, np.float32).reshape(-1, 3)
    nodes = chain_nodes(lo, hi)
    if not extras:
        return verts, prims, nodes
    normals = rng.normal(size=(len(verts), 3)).astype(np.float32)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = rng.random((len(verts), 2)).astype(np.float32)
    return Chain(verts, prims, nodes, normals, uvs, alpha, lo, hi)


def chain_rays(x_far, n, seed, tmax_share=0.25):
    """n rays down a tube chain from beyond its far end (x_far = the largest x of the scene): origins within 0.3 of
    the axis, slopes up to 1e-3, so over a chain up to 150 long they stay within 0.45 of the axis.  d.x < 0: the
    interior child is the near one at every level.  A share has a finite tMax that ends inside the chain."""
    from nn_bvh_amd import make_rays
    rng = np.random.default_rng(seed)
    o = np.stack([np.full(n, x_far + 12.0), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([-np.ones(n), rng.uniform(-1e-3, 1e-3, n), rng.uniform(-1e-3, 1e-3, n)], 1)
    rays = make_rays(o, d)
    short = rng.random(n) < tmax_share
    rays["tmax"][short] = rng.uniform(20.0, x_far, short.sum()).astype(np.float32)
    return rays


def line_box_margin(rays, lo, hi, m_inv=None):
    """float64: the smallest distance by which the LINES of `rays` stay inside the y / z extent of the boxes lo / hi
    while they cross the boxes' x extent (negative: a line leaves a box sideways), per ray.  m_inv (3x4): the rays are
    taken into that space first."""
    o, d = rays["o"].astype(np.float64), rays["d"].astype(np.float64)
    if m_inv is not None:
        m = np.asarray(m_inv, np.float64).reshape(3, 4)
        o, d = o @ m[:, :3].T + m[:, 3], d @ m[:, :3].T
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    margin = np.full(len(rays), np.inf)
    for xs in (lo[:, 0], hi[:, 0]):
        t = (xs[None, :] - o[:, :1]) / d[:, :1]
        for ax in (1, 2):
            p = o[:, ax:ax + 1] + t * d[:, ax:ax + 1]
            margin = np.minimum(margin, np.minimum(p - lo[None, :, ax], hi[None, :, ax] - p).min(1))
    return margin


def rot_x(theta, tx):
    """Rigid transform: rotation by theta about the x axis, then translation by tx along it -> (m, m_inv) 3x4."""
    c, s = np.cos(theta), np.sin(theta)
    r = np.array([[1, 0, 0], [0, c, -s], [0, s, c]], np.float64)
    m = np.concatenate([r, [[tx], [0], [0]]], 1)
    mi = np.concatenate([r.T, -r.T @ [[tx], [0], [0]]], 1)
    return m.astype(np.float32).reshape(12), mi.astype(np.float32).reshape(12)


def two_level_chain(a, b, seed, instance_levels=None, moving=False):
    """Outer tube chain of depth a whose leaves at `instance_levels` (default: 3, a // 2 and the deepest, a) hold
    instance primitives of ONE child: a tube chain of depth b.  Placements rotate about the chain axis and shift along
    it, so a ray near the axis stays near the child's axis too, with d.x < 0 in both spaces: `a` outer entries are
    pending when the deepest instance is entered and b more inside it.  The library bounds a + (b + 1) by 64.
    moving: the instance boxes cover the motion of animated_two_level_chain (every second placement turns on about the
    axis and slides along it): the x extent of both end placements, and [-1.5, 1.5]^2 across (the child's
    cross-section [-1, 1]^2 at any angle lies within radius sqrt(2))."""
    from nn_bvh_amd import PRIM_DTYPE, instancing
    from nn_bvh_amd._lib import INSTANCE_DTYPE
    rng = np.random.default_rng(seed)
    levels = sorted(set(instance_levels if instance_levels is not None else (3, a // 2, a)))
    child = chain_tree(b, rng, tube=True, leaves="patch", extras=True)
    outer = chain_tree(a, rng, tube=True, leaves="tri", extras=True)
    n_top_nodes, n_top_prims = len(outer.nodes), len(outer.prims)
    verts = np.concatenate([outer.verts, child.verts])
    cprims = child.prims.copy()
    for k in range(len(cprims)):
        nv = 3 if cprims[k]["kind"] in TRI_KINDS else 4
        cprims[k]["v"][:nv] += len(outer.verts)
    cprims["id"] += n_top_prims
    oprims, lo, hi = outer.prims.copy(), outer.leaf_lo.copy(), outer.leaf_hi.copy()
    instances = np.zeros(len(levels), INSTANCE_DTYPE)
    croot = np.concatenate([child.nodes[0]["pmin"], child.nodes[0]["pmax"]])
    for j, k in enumerate(levels):
        m, mi = rot_x(0.4 + 0.9 * j, 2.0 * k)
        instances[j]["render_from_prim"], instances[j]["prim_from_render"] = m, mi
        instances[j]["root"], instances[j]["n_nodes"] = n_top_nodes, len(child.nodes)
        oprims[k] = np.zeros(1, PRIM_DTYPE)[0]
        oprims[k]["kind"], oprims[k]["id"], oprims[k]["v"][0] = 2, k, j
        box = instancing.transform_bounds(m, croot)
        lo[k], hi[k] = box[:3], box[3:]
        if moving:
            end = instancing.transform_bounds(rot_x(*end_placement(j, k))[0], croot)
            lo[k] = (min(box[0], end[0]) - 0.05, -1.5, -1.5)
            hi[k] = (max(box[3], end[3]) + 0.05, 1.5, 1.5)
    nodes = np.concatenate([chain_nodes(lo, hi), chain_nodes(child.leaf_lo, child.leaf_hi, n_top_nodes, n_top_prims)])
    return TwoLevelChain(verts, np.concatenate([oprims, cprims]), nodes, instances, n_top_nodes, a, b, lo, hi,
                         child.leaf_lo, child.leaf_hi)


def end_placement(j, k):
    """(angle, shift) of instance j (at outer leaf k) at the end of its motion; its start: (0.4 + 0.9 j, 2 k)."""
    return 0.4 + 0.9 * j + 0.7, 2.0 * k + 1.5


def animated_two_level_chain(a, b, seed):
    """two_level_chain with AnimatedTransforms: -> (TwoLevelChain, device records, oracle records).  Every second
    instance, the deepest one included, is actually animated over the time range [0, 1]: it turns by 0.7 rad about the
    chain axis and slides 1.5 along it, so that at EVERY ray time a ray near the axis stays near the child's axis and
    the depth argument of two_level_chain holds.  That is why the transforms are written here and not drawn from
    tests/golden/anim_interpolate.npz as tests/test_animated.py does: those are arbitrary affine maps, which take the
    ray off the child's axis.  The records are what the reference's AnimatedTransform holds for such a motion: T = the
    shifts, R = the unit quaternions (sin(angle / 2), 0, 0, cos(angle / 2)), S = identity, and the start / end
    matrices are Interpolate's own products Translate(T) * Rotate(R) * S, taken from the oracle so that they are
    bit-equal to what it gives an instant inside the range.  Instance boxes cover the motion (moving=True)."""
    import oracle_binding as ob
    from nn_bvh_amd import _lib
    t = two_level_chain(a, b, seed, moving=True)
    n = len(t.instances)
    levels = sorted({3, a // 2, a})
    oa = np.zeros(n, ob.ANIM_DTYPE)
    oa["start_time"], oa["end_time"] = 0.0, 1.0
    oa["S"] = np.eye(4, dtype=np.float32).reshape(16)
    ends = np.zeros((n, 2, 2))
    for j, k in enumerate(levels):
        ends[j] = (0.4 + 0.9 * j, 2.0 * k), end_placement(j, k)
        oa["actually_animated"][j] = int((n - 1 - j) % 2 == 0)
    for e, (fm, fi) in enumerate((("start_m", "start_minv"), ("end_m", "end_minv"))):
        oa["T"][:, e, 0] = ends[:, e, 1]
        oa["R"][:, e, 0], oa["R"][:, e, 3] = np.sin(ends[:, e, 0] / 2), np.cos(ends[:, e, 0] / 2)
    for e, (fm, fi) in enumerate((("start_m", "start_minv"), ("end_m", "end_minv"))):
        still = oa.copy()  # a motion that rests at this end: Interpolate inside the range composes its matrices
        still["T"][:, 1 - e], still["R"][:, 1 - e] = still["T"][:, e], still["R"][:, e]
        still["actually_animated"] = 1
        mm = ob.anim_interpolate(still, np.full(n, 0.5, np.float32))
        oa[fm], oa[fi] = mm[:, :16], mm[:, 16:]
    anims = np.zeros(n, _lib.ANIMATED_DTYPE)
    for f_o, f_p in (("start_m", "start_from"), ("start_minv", "start_inv"), ("end_m", "end_from"), ("end_minv", "end_inv")):
        anims[f_p] = oa[f_o]
    for f in ("T", "R", "S", "start_time", "end_time", "actually_animated"):
        anims[f] = oa[f]
    inst = t.instances.copy()  # the static placement = the start transform, as the oracle's walk and the device use it
    inst["render_from_prim"], inst["prim_from_render"] = oa["start_m"][:, :12], oa["start_minv"][:, :12]
    return t._replace(instances=inst), anims, oa


def kd_chain(depth, seed, form="lean"):
    """A maximally skewed kd-tree in KdTreeNode layout (8 B: interior {split, axis | above << 2}, leaf {index,
    3 | n << 2}; the below child follows its parent): interior k (node k) splits x at 2 (depth - k); its below child is
    interior k + 1, its above child the leaf of the slab [2 (depth - k), 2 (depth - k + 1)].  A ray along +x from
    x < 0 has o < split at every level and crosses every split plane inside the tree's bounds: one entry pushed per
    level, `depth` pending at the deepest leaf.  Leaves hold one tube primitive each (every fifth also its
    neighbour's, through primitiveIndices).  form: "lean" triangles, "patch" with bilinear patches, "attr" with the
    attribute-reading alpha kinds (6 .. 15)."""
    from nn_bvh_amd._lib import KD_NODE_DTYPE
    rng = np.random.default_rng(seed)
    mix = {"lean": "tri", "patch": "patch", "attr": "alpha_patch"}[form]
    # leaf slab j (j = 0 .. depth) covers x in [2 j, 2 j + 2]: its primitive at x = 2 j + 1
    ch = chain_tree(depth, rng, tube=True, leaves=mix, extras=True, x0=1.0)
    n_leaves = depth + 1
    nodes = np.zeros(2 * depth + 1, KD_NODE_DTYPE)
    splits = np.zeros(depth, np.float32)
    idx = []

    def leaf(node, j):
        if j % 5 == 2:
            nodes[node]["split_or_index"], nodes[node]["flags"] = len(idx), 3 | (2 << 2)
            idx.extend([j, (j + 1) % n_leaves])
        else:
            nodes[node]["split_or_index"], nodes[node]["flags"] = j, 3 | (1 << 2)

    for k in range(depth):
        splits[k] = 2.0 * (depth - k)
        above = 2 * depth - k  # node index of the above leaf: the leaves follow the interiors, deepest first
        nodes[k]["split_or_index"] = splits[k:k + 1].view(np.uint32)[0]
        nodes[k]["flags"] = 0 | (above << 2)
        leaf(above, depth - k)
    leaf(depth, 0)
    bounds = np.array([0.5, -1, -1, 2 * depth + 1.5, 1, 1], np.float32)
    return KdChain(ch.verts, ch.prims, nodes, np.array(idx, np.int32), bounds, ch.normals, ch.uvs, ch.prim_alpha, splits)


def kd_chain_rays(n, seed, tmax_share=0.25):
    """Rays up a kd chain from x = -5 (see chain_rays: within 0.45 of the axis throughout)."""
    from nn_bvh_amd import make_rays
    rng = np.random.default_rng(seed)
    o = np.stack([np.full(n, -5.0), rng.uniform(-0.3, 0.3, n), rng.uniform(-0.3, 0.3, n)], 1)
    d = np.stack([np.ones(n), rng.uniform(-1e-3, 1e-3, n), rng.uniform(-1e-3, 1e-3, n)], 1)
    rays = make_rays(o, d)
    short = rng.random(n) < tmax_share
    rays["tmax"][short] = rng.uniform(20.0, 120.0, short.sum()).astype(np.float32)
    return rays


# ---- kd-tree builder scenes: one per decision path of buildTree (tests/test_kd_build_gpu.py) -------------------
# Every generator returns (verts, prims) or, for host-only primitives, (verts, prims, prim_bounds).  The CPU tests
# there prove with a census of the host-built tree that each scene reaches the path it is named for.
def box_tris(lo, hi):
    """One triangle per box [lo, hi] whose Bounds() is exactly that box: (lo.x lo.y lo.z), (hi.x hi.y lo.z),
    (lo.x hi.y hi.z).  The coordinates are copied, never computed: signed zeros survive."""
    lo, hi = np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)
    v = np.stack([lo, np.stack([hi[:, 0], hi[:, 1], lo[:, 2]], 1), np.stack([lo[:, 0], hi[:, 1], hi[:, 2]], 1)], 1)
    return v.reshape(-1, 3).copy(), make_prims(np.arange(3 * len(lo), dtype=np.int32).reshape(-1, 3))


def merge(*parts):
    """Concatenate (verts, prims) scenes of triangles / patches: vertex indices and ids shifted."""
    verts, prims, nv, n = [], [], 0, 0
    for v, p in parts:
        p = p.copy()
        p["v"] = np.where(np.arange(4)[None, :] < np.where(p["kind"] == 1, 4, 3)[:, None], p["v"] + nv, p["v"])
        p["id"] = n + np.arange(len(p))
        verts.append(np.asarray(v, np.float32))
        prims.append(p)
        nv, n = nv + len(v), n + len(p)
    return np.concatenate(verts), np.concatenate(prims)


def host_boxes(lo, hi):
    """Host-only primitives (kind 3) with the caller's bounds: (verts, prims, prim_bounds)."""
    from nn_bvh_amd import PRIM_DTYPE
    pb = np.concatenate([np.asarray(lo, np.float32).reshape(-1, 3), np.asarray(hi, np.float32).reshape(-1, 3)], 1)
    prims = np.zeros(len(pb), PRIM_DTYPE)
    prims["kind"], prims["id"] = 3, np.arange(len(pb))
    return np.zeros((1, 3), np.float32), prims, np.ascontiguousarray(pb)


def kd_sticks(seed=0, n_bundles=9, n_soup=500):
    """Retries on the other axes.  A bundle = 6 .. 14 disjoint slabs that all span the bundle's whole extent on its
    longest axis a: no edge lies strictly inside a node that holds only the bundle, so attempt 0 fails.  Family 1
    differs on both other axes (attempt 1, axis a + 1, splits it); family 2 ("plates") also spans axis a + 1 and is
    stacked along a + 2 (attempt 2).  Bundles sit on a ring far outside an ordinary soup and far from each other, so
    that empty-space cuts isolate them at various depths while soup nodes of the same levels split on attempt 0."""
    rng = np.random.default_rng(seed)
    los, his = [], []
    for b in range(2 * n_bundles):
        a = b % 3
        u, w = (a + 1) % 3, (a + 2) % 3
        ang = 2 * np.pi * b / (2 * n_bundles)
        c = np.array([40 * np.cos(ang), 40 * np.sin(ang), 12.0 * (b % 5) - 24], np.float32)
        m = int(rng.integers(6, 15))
        lo, hi = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
        lo[:, a], hi[:, a] = c[a] - 4, c[a] + 4                       # every slab: the whole long extent
        if b < n_bundles:                                             # family 1: a grid of rods across u and w
            ku, kw = np.arange(m) % 3, np.arange(m) // 3
            lo[:, u], hi[:, u] = c[u] + 0.5 * ku, c[u] + 0.5 * ku + 0.25
            lo[:, w], hi[:, w] = c[w] + 0.5 * kw, c[w] + 0.5 * kw + 0.25
        else:                                                         # family 2: plates spanning a and u, stacked on w
            lo[:, u], hi[:, u] = c[u] - 1.5, c[u] + 1.5
            lo[:, w], hi[:, w] = c[w] + 0.25 * np.arange(m), c[w] + 0.25 * np.arange(m) + 0.125
        los.append(lo)
        his.append(hi)
    return merge(box_tris(np.concatenate(los), np.concatenate(his)), random_soup(n_soup, 0, seed + 1, extent=8.0))


def kd_signed_zeros(seed=0, n=600, n_soup=600):
    """Many bound edges at exactly 0 on every axis, -0 and +0 mixed per primitive and axis in list order, inside a
    soup that straddles the origin.  Per axis k a primitive lies on the negative side (its box ENDS at +-0) or on the
    positive side (its box STARTS at +-0, or a little inside: a clean cut at the run of End edges), so the plane 0 is
    a cheap split and the chosen edge's own sign goes into the node."""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0).astype(np.float32)
    side = rng.random((n, 3)) < 0.5
    size = rng.uniform(0.2, 3.0, (n, 3)).astype(np.float32)
    gap = np.where(rng.random((n, 3)) < 0.5, z, np.float32(0.03125)).astype(np.float32)   # start AT zero or past it
    lo = np.where(side, -size, gap).astype(np.float32)
    hi = np.where(side, z, size).astype(np.float32)
    return merge(box_tris(lo, hi), random_soup(n_soup, 0, seed + 1, extent=3.0, size=0.3))


def kd_lattice(nx=256, ny=3, nz=2):
    """Equal costs: a regular lattice of identical disjoint boxes (host-only primitives, the caller's bounds), pitch 1
    and size 0.5, all coordinates small dyadic numbers: symmetric edges cost the same and the FIRST must win.  A run
    of nx >= 200 boxes per x row: one segment's edges span several wavefronts."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    lo = g.astype(np.float32)
    return host_boxes(lo, lo + np.float32(0.5))


def kd_cluster_lattice(seed=0, n_clusters=150):
    """Equal costs in SMALL segments: clusters of 3 .. 20 identical boxes in a row, the clusters on a coarse regular
    grid far apart: after a few levels many segments of a handful of edges share each wavefront."""
    rng = np.random.default_rng(seed)
    los = []
    for c in range(n_clusters):
        k = int(rng.integers(3, 21))
        base = np.array([64.0 * (c % 6), 64.0 * ((c // 6) % 5), 64.0 * (c // 30)], np.float32)
        row = np.zeros((k, 3), np.float32)
        row[:, c % 3] = np.arange(k)
        los.append(base + row)
    lo = np.concatenate(los)
    return host_boxes(lo, lo + np.float32(0.5))


def kd_overlap_clusters(seed=0, n_clusters=6, n_per=24, spacing=30.0):
    """Refusals: clusters of boxes that all contain a common core [-1, 1]^3 and reach 0 .. 1 beyond it on every side:
    every split leaves nearly all primitives on both sides, cost > leafCost three times along a path (bad == 3)."""
    rng = np.random.default_rng(seed)
    c = (np.arange(n_clusters)[:, None] * np.array([spacing, 0.37 * spacing, -0.21 * spacing])).astype(np.float32)
    c = np.repeat(c, n_per, 0)
    lo = c - 1 - rng.random((len(c), 3)).astype(np.float32)
    hi = c + 1 + rng.random((len(c), 3)).astype(np.float32)
    return box_tris(lo, hi)


def kd_identical_boxes(seed=0, n_stacks=5, n_per=12, n_soup=400):
    """No valid edge: stacks of IDENTICAL boxes next to a soup: a node that holds only one stack is cut down to the
    stack's box, and then no edge lies strictly inside it on any axis."""
    rng = np.random.default_rng(seed)
    c = rng.uniform(-20, 20, (n_stacks, 3)).astype(np.float32)
    h = rng.uniform(0.5, 1.5, (n_stacks, 3)).astype(np.float32)
    lo, hi = np.repeat(c - h, n_per, 0), np.repeat(c + h, n_per, 0)
    return merge(box_tris(lo, hi), random_soup(n_soup, 0, seed + 1, extent=6.0))


def kd_flat(n=800, seed=0):
    """All triangles in the plane z = 0 (written as +0 and -0): one zero extent, costs stay finite."""
    rng = np.random.default_rng(seed)
    verts, prims = random_soup(n, 0, seed, extent=6.0)
    verts = verts.copy()
    verts[:, 2] = np.where(rng.random(len(verts)) < 0.5, 0.0, -0.0)
    return verts, prims


def kd_line(n=60, seed=0, point=False):
    """Degenerate triangles with every vertex on one line (the x axis shifted to y = 1, z = 2) or, point=True, at one
    point: the root's box has no surface area, 1 / 0 = inf, 0 * inf = NaN: no cost ever wins."""
    rng = np.random.default_rng(seed)
    verts = np.zeros((3 * n, 3), np.float32)
    verts[:, 0] = 0.5 if point else rng.uniform(-5, 5, 3 * n)
    verts[:, 1], verts[:, 2] = 1.0, 2.0
    return verts, make_prims(np.arange(3 * n, dtype=np.int32).reshape(n, 3))


def kd_flat_mix(seed=0):
    """A plane, a line and a point of degenerate geometry inside an ordinary soup."""
    return merge(kd_flat(300, seed), kd_line(40, seed + 1), kd_line(20, seed + 2, point=True),
                 random_soup(500, 0, seed + 3, extent=6.0))


def kd_two_clusters(seed=0, n=400):
    """Empty space: two dense clusters far apart (and off each other's axes): cutting empty space away pays."""
    v1, p1 = random_soup(n, 0, seed, extent=1.0, size=0.2)
    v2, p2 = random_soup(n, 0, seed + 1, extent=1.5, size=0.2)
    return merge((v1, p1), (v2 + np.array([60, 25, -40], np.float32), p2))


# ---- BVH builder scenes: one per decision path of the SAH / HLBVH builders (tests/test_bvh_build_paths.py) --------
# Every generator returns (verts, prims) with ids = positions.  The CPU tests there prove with a census of the
# host-built tree that each scene reaches the path it is named for.
def shifted(scene_, by):
    """A (verts, prims) scene translated by a vector of small integers (exact for the dyadic coordinates used here)."""
    v, p = scene_
    return (np.asarray(v, np.float32) + np.asarray(by, np.float32)).astype(np.float32), p


def bvh_overlapping(n, centre, seed, jitter=0.02):
    """n triangles whose boxes all nearly fill the cube centre +- 1 (each face moved out by up to `jitter`): distinct
    centroids, but no split separates anything, so every SAH split costs about n + 1/2 against a leaf's n."""
    rng = np.random.default_rng(seed)
    c = np.asarray(centre, np.float32)
    lo = c - 1 - jitter * rng.random((n, 3)).astype(np.float32)
    hi = c + 1 + jitter * rng.random((n, 3)).astype(np.float32)
    return box_tris(lo, hi)


def bvh_signed_zero_cluster(n=700, seed=12, x0=0.0):
    """n triangles with the box [+-0, 1]^3 (one centroid): their minimum corner mixes +0 and -0 per axis.  x0 != 0
    moves the cluster along x: its box starts at x0 there and keeps the mixed zeros on y and z."""
    rng = np.random.default_rng(seed)
    z = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0).astype(np.float32)
    v = np.zeros((n, 3, 3), np.float32)
    v[:, 0] = z
    v[:, 1] = [1, 1, 0]
    v[:, 2] = [1, 0, 1]
    v[:, 1, 2] = z[:, 2]
    v[:, 2, 1] = z[:, 1]
    if x0:
        v[:, :, 0] += np.float32(x0)
    return v.reshape(-1, 3), make_prims(np.arange(3 * n, dtype=np.int32).reshape(n, 3))


def bvh_signed_zero_row(n=96, seed=0, x0=14.0, pitch=1.5):
    """A row of unit boxes along x whose y and z start at +-0, signs mixed: every interior node above them joins two
    children that both supply the zero, often with different signs."""
    rng = np.random.default_rng(seed)
    lo = np.where(rng.random((n, 3)) < 0.5, 0.0, -0.0).astype(np.float32)
    lo[:, 0] = x0 + pitch * np.arange(n)
    hi = np.ones((n, 3), np.float32)
    hi[:, 0] = lo[:, 0] + 1
    return box_tris(lo, hi)


def bvh_leaf_rules(seed=0):
    """A 3 000-triangle soup around the origin with, placed around and inside it: overlapping cubes (the cost rule),
    coincident centroids, degenerate triangles on an x-parallel segment (no surface area) and signed zeros (clusters
    of 700 inside the soup, of 40 and 150 beside it, and a row of boxes)."""
    return merge(
        random_soup(3000, 0, seed, extent=10.0),
        bvh_overlapping(40, (40, 5, -7), seed + 1), bvh_overlapping(200, (-35, 20, 9), seed + 2),
        shifted(coincident_centroids(40, seed + 3), (10, -40, 5)), shifted(coincident_centroids(200, seed + 4), (-20, -30, -15)),
        shifted(coincident_centroids(700, seed + 5), (25, 35, 20)),
        shifted(kd_line(30, seed + 6), (-40, -10, 20)), shifted(kd_line(150, seed + 7), (30, -25, -30)),
        shifted(kd_line(600, seed + 8), (-15, 40, -25)),
        bvh_signed_zero_cluster(700, seed + 9), bvh_signed_zero_row(96, seed + 10),
        bvh_signed_zero_cluster(40, seed + 11, x0=-14.0), bvh_signed_zero_cluster(150, seed + 12, x0=-18.0))


def bvh_lattice(n=16):
    """n^3 identical boxes on a regular lattice: equal centroid spacings and equal extents on the three axes."""
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 3)
    lo = g.astype(np.float32)
    return box_tris(lo, lo + np.float32(0.5))


def bvh_spine(n, ratio=12.1, k0=-32, pairs=False):
    """n tiny triangles in planes x = ratio^(k0 + k), 2^-10 wide in y and z: with 12 SAH buckets the largest centroid
    is alone in the last bucket and every other one falls into the first, at every level: a left spine of n - 1.
    pairs: a second triangle at x (1 + 2^-10) beside each, so that what comes off per level is a pair, i.e. an
    interior node (the nth_element of two) as the second child."""
    x = (np.float64(ratio) ** (k0 + np.arange(n))).astype(np.float32)
    if pairs:
        x = np.stack([x, x * np.float32(1 + 2.0 ** -10)], 1).reshape(-1).astype(np.float32)
        n = 2 * n
    lo = np.zeros((n, 3), np.float32)
    lo[:, 0] = x
    hi = np.full((n, 3), 2.0 ** -10, np.float32)
    hi[:, 0] = x
    return box_tris(lo, hi)


def bvh_cluster_and_outlier(seed=0, n=1500, far=40.0):
    """A unit-extent soup and one triangle far away on the diagonal: the soup falls into ONE cell of the 16^3 treelet
    grid, the outlier into the opposite one."""
    v, p = random_soup(1, 0, seed + 1, extent=0.0, size=0.5)
    return merge(random_soup(n, 0, seed, extent=1.0, size=0.2), (v + np.float32(far), p))


def bvh_all_cells(seed=0, n_soup=2000):
    """A 16^3 lattice of small triangles (one per cell of the treelet grid) inside a soup of the same extent."""
    return merge(bvh_lattice(16), shifted(random_soup(n_soup, 0, seed, extent=7.0, size=0.3), (7.5, 7.5, 7.5)))


def bvh_code_runs(seed=0):
    """Runs of identical Morton codes of 64, 65 and 700 primitives (coincident centroids), each with a few dozen
    small triangles close by, inside a soup."""
    parts = [random_soup(3000, 0, seed, extent=10.0)]
    for k, (n, at) in enumerate(((64, (4, -6, 2)), (65, (-7, 3, -5)), (700, (1, 8, 6)))):
        parts.append(shifted(coincident_centroids(n, seed + 1 + k), at))
        parts.append(shifted(random_soup(40, 0, seed + 5 + k, extent=0.25, size=0.05), np.array(at) + [1, 2, 3]))
    return merge(*parts)


def bvh_dense_cell(seed=0):
    """3 000 triangles spread over about one cell of the treelet grid of a sparse 2 000-triangle soup: the cell's
    treelet splits on every one of the 18 bits."""
    return merge(random_soup(3000, 0, seed, extent=3.0, size=0.1), random_soup(2000, 0, seed + 1, extent=50.0))
