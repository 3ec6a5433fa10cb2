"""Host-side mirror of the reference's aggregate interface for the accelerated path.

`BVHAggregate` here has the reference's method names and argument meaning
(/root/reference/src/pbrt/cpu/aggregates.h:28-70: Create / Bounds / Intersect / IntersectP),
batched the way the wavefront caller batches them (wavefront/aggregate.cpp:34-68).  All
arithmetic happens in libnnbvh_hip.so on the GPU; numpy/torch only carry buffers.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import HIT_DTYPE, NODE_DTYPE, PRIM_DTYPE, RAY_DTYPE, NNBVHError, check, ptr

SPLIT_METHODS = {"sah": 0, "hlbvh": 1, "middle": 2, "equal": 3}


def make_prims(tri_indices=None, patch_indices=None):
    """Primitive table in creation order: triangles first, then bilinear patches.
    ids are the running primitive index (the reference's position in `prims`)."""
    nt = 0 if tri_indices is None else len(tri_indices)
    npch = 0 if patch_indices is None else len(patch_indices)
    prims = np.zeros(nt + npch, PRIM_DTYPE)
    prims["id"] = np.arange(nt + npch, dtype=np.int32)
    if nt:
        prims["kind"][:nt] = 0
        prims["v"][:nt, :3] = np.asarray(tri_indices, np.int32).reshape(nt, 3)
    if npch:
        prims["kind"][nt:] = 1
        prims["v"][nt:] = np.asarray(patch_indices, np.int32).reshape(npch, 4)
    return prims


def make_rays(o, d, tmax=np.inf, time=0.0):
    o = np.asarray(o, np.float32).reshape(-1, 3)
    rays = np.zeros(len(o), RAY_DTYPE)
    rays["o"] = o
    rays["d"] = np.asarray(d, np.float32).reshape(-1, 3)
    rays["tmax"] = tmax
    rays["time"] = time
    return rays


class BuiltTree:
    """Output of the host builder (BVHAggregate ctor + flattenBVH, aggregates.cpp:140-522)."""

    def __init__(self, nodes, ordered_prims, depth):
        self.nodes = nodes
        self.ordered_prims = ordered_prims
        self.depth = depth


def _take_build(L, h, what):
    if not h:
        raise NNBVHError(what + ": " + _lib.last_error())
    try:
        n = ctypes.c_int(0)
        pn = L.nnbvh_build_nodes(h, ctypes.byref(n))
        nodes = np.frombuffer((ctypes.c_char * (n.value * 32)).from_address(pn),
                              NODE_DTYPE).copy()
        pp = L.nnbvh_build_ordered_prims(h, ctypes.byref(n))
        ordered = np.frombuffer((ctypes.c_char * (n.value * 24)).from_address(pp),
                                PRIM_DTYPE).copy()
        tree = BuiltTree(nodes, ordered, L.nnbvh_build_depth(h))
        ms = np.zeros(5, np.float64)
        L.nnbvh_build_gpu_timing(h, ptr(ms))
        tree.gpu_ms = [float(x) for x in ms]  # phases: see nnbvh_build_gpu_timing
        tree.n_upper = L.nnbvh_build_n_upper(h)  # see nnbvh_forest_n_upper; both 0 for host builds
        tree.n_upper_passes = L.nnbvh_build_n_upper_passes(h)
    finally:
        L.nnbvh_build_destroy(h)
    return tree


def build_tree(prims, verts, max_prims_in_node=4, split_method="sah", prim_bounds=None):
    """SAH / HLBVH / middle / equal-counts build on the host (no GPU needed).  prim_bounds
    ([n, 6] float32) is required when the list contains instance primitives (kind 2)."""
    L = _lib.lib()
    prims = np.ascontiguousarray(prims, PRIM_DTYPE)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    if split_method not in SPLIT_METHODS:
        # aggregates.cpp:735-738 warns and falls back to sah; we report instead
        raise NNBVHError(f'BVH split method "{split_method}" unknown')
    if prim_bounds is not None:
        prim_bounds = np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
        h = L.nnbvh_build_create_with_bounds(ptr(prims), len(prims), ptr(verts), len(verts),
                                             ptr(prim_bounds), int(max_prims_in_node),
                                             SPLIT_METHODS[split_method])
    else:
        h = L.nnbvh_build_create(ptr(prims), len(prims), ptr(verts), len(verts),
                                 int(max_prims_in_node), SPLIT_METHODS[split_method])
    return _take_build(L, h, "nnbvh_build_create")


def build_tree_gpu(prims, verts, max_prims_in_node=4, prim_bounds=None, device=0, split_method="hlbvh"):
    """SAH or HLBVH tree built on the GPU: byte-identical to build_tree(..., split_method)."""
    if split_method not in ("sah", "hlbvh"):
        raise NNBVHError(f'GPU build supports "sah" and "hlbvh", not "{split_method}"')
    L = _lib.lib()
    prims = np.ascontiguousarray(prims, PRIM_DTYPE)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    pb = None
    if prim_bounds is not None:
        pb = np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
    h = L.nnbvh_build_create_gpu(ptr(prims), len(prims), ptr(verts), len(verts),
                                 ptr(pb) if pb is not None else None, int(max_prims_in_node),
                                 SPLIT_METHODS[split_method], int(device))
    return _take_build(L, h, "nnbvh_build_create_gpu")


class BuiltForest(list):
    """build_forest_gpu's / build_hlbvh_forest_gpu's result: a list of BuiltTree, one per object, with the pass's own
    figures as attributes: gpu_ms (the five phases of nnbvh_forest_gpu_timing), n_levels (SAH: breadth-first passes
    run; HLBVH: 0), n_subtrees (SAH: subtrees built by one wavefront each; HLBVH: treelets in the forest), n_upper
    (SAH: nodes built breadth-first; HLBVH: upper nodes, treelets less objects), n_upper_passes (HLBVH: device passes of
    the upper SAH build, 0 when no object has two treelets; SAH: 0) and node_first (where each tree starts in the
    forest's node array)."""


def _forest(name, objects, verts, max_prims_in_node, prim_bounds, tail):
    L = _lib.lib()
    objects = [np.ascontiguousarray(o, PRIM_DTYPE) for o in objects]
    prims = np.ascontiguousarray(np.concatenate(objects), PRIM_DTYPE) if objects else np.zeros(0, PRIM_DTYPE)
    first = np.ascontiguousarray(np.concatenate([[0], np.cumsum([len(o) for o in objects])]), np.int32)
    verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    pb = None
    if prim_bounds is not None:
        pb = np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
    h = getattr(L, name)(ptr(prims), len(prims), ptr(first), len(objects), ptr(verts), len(verts),
                         ptr(pb) if pb is not None else None, int(max_prims_in_node), *tail)
    if not h:
        raise NNBVHError(name + ": " + _lib.last_error())
    try:
        def array(fn, dtype, extra=0):  # a copy of what an accessor points at: its count + extra elements
            n = ctypes.c_int(0)
            p = fn(h, ctypes.byref(n))
            nbytes = (n.value + extra) * np.dtype(dtype).itemsize
            return np.frombuffer((ctypes.c_char * nbytes).from_address(p), dtype).copy()

        nodes = array(L.nnbvh_forest_nodes, NODE_DTYPE)
        ordered = array(L.nnbvh_forest_ordered_prims, PRIM_DTYPE)
        node_first = array(L.nnbvh_forest_node_first, np.int32, 1)
        depths = array(L.nnbvh_forest_depths, np.int32)
        forest = BuiltForest(BuiltTree(nodes[node_first[k]:node_first[k + 1]].copy(),
                                       ordered[first[k]:first[k + 1]].copy(), int(depths[k]))
                             for k in range(len(objects)))
        ms = np.zeros(5, np.float64)
        L.nnbvh_forest_gpu_timing(h, ptr(ms))
        forest.gpu_ms = [float(x) for x in ms]
        forest.n_levels = L.nnbvh_forest_n_levels(h)
        forest.n_subtrees = L.nnbvh_forest_n_subtrees(h)
        forest.n_upper = L.nnbvh_forest_n_upper(h)
        forest.n_upper_passes = L.nnbvh_forest_n_upper_passes(h)
        forest.node_first = node_first
    finally:
        L.nnbvh_forest_destroy(h)
    return forest


def build_forest_gpu(objects, verts, max_prims_in_node=4, prim_bounds=None, device=0):
    """The SAH trees of `objects` (a list of PRIM_DTYPE arrays over ONE vertex array) built in one pass on the GPU
    (nnbvh_build_forest_create_gpu): tree k is byte for byte build_tree(objects[k], verts, max_prims_in_node, "sah").
    prim_bounds ([total primitives, 6] float32, the objects' rows one after another) is read for host-only primitives.
    Returns a BuiltForest."""
    return _forest("nnbvh_build_forest_create_gpu", objects, verts, max_prims_in_node, prim_bounds,
                   (SPLIT_METHODS["sah"], int(device)))


def build_hlbvh_forest_gpu(objects, verts, max_prims_in_node=4, prim_bounds=None, device=0):
    """build_forest_gpu for HLBVH trees (nnbvh_build_forest_create_gpu_hlbvh): tree k is byte for byte
    build_tree(objects[k], verts, max_prims_in_node, "hlbvh").  Of the BuiltForest, gpu_ms are build_tree_gpu's HLBVH
    phases, n_levels is 0 and n_subtrees counts the treelets of the whole forest."""
    return _forest("nnbvh_build_forest_create_gpu_hlbvh", objects, verts, max_prims_in_node, prim_bounds,
                   (int(device),))


class BVHAggregate:
    """GPU-resident aggregate.  Construct from primitives (builds the tree on the host like
    BVHAggregate::Create, aggregates.cpp:725-744: splitmethod "sah", maxnodeprims 4) or from
    an already flattened tree via `from_tree`."""

    def __init__(self, prims, verts, max_prims_in_node=4, split_method="sah", device=0):
        tree = build_tree(prims, verts, max_prims_in_node, split_method)
        self._init(tree.nodes, tree.ordered_prims, verts, device, tree.depth)

    @classmethod
    def from_tree(cls, nodes, ordered_prims, verts, device=0, instances=None, n_top_nodes=None, animated=None,
                  normals=None, prim_alpha=None, uvs=None, alpha_textures=None):
        """instances (INSTANCE_DTYPE) + n_top_nodes make a two-level scene: nodes[:n_top_nodes] is
        the top-level tree, the child trees follow (see nn_bvh_amd.instancing).  animated
        (ANIMATED_DTYPE, one per instance) turns instances into AnimatedPrimitives.  normals: per-vertex
        shading normals, needed by alpha-tested triangles / patches of smooth meshes (prim kinds 6 / 7, 10 / 11);
        prim_alpha: one constant alpha per entry of ordered_prims, read for alpha-tested patches (kinds 8 .. 15);
        uvs: per-vertex (u, v), read for the alpha-tested patches of meshes with uv (kinds 12 .. 15) and the
        triangles with an image-textured alpha (kinds 16 .. 19; None: the default corners);
        alpha_textures: a sequence of AlphaTexture, the table kinds 16 .. 19 index with v[3]; with instances the
        scene is two-level (nnbvh_scene_create_instanced_with_alpha_textures) and a textured triangle inside an object
        is evaluated on the instance-space ray."""
        self = cls.__new__(cls)
        self._init(nodes, ordered_prims, verts, device, None, instances, n_top_nodes, animated, normals, prim_alpha, uvs,
                   alpha_textures)
        return self

    @classmethod
    def build_on_device(cls, prims, verts, max_prims_in_node=4, split_method="sah", prim_bounds=None,
                        device=0, normals=None, prim_alpha=None, uvs=None, alpha_textures=None):
        """Tree built AND baked on the GPU (nnbvh_scene_create_gpu_build): the tree never visits the
        host.  Same traversal results as the host-built aggregate; `nodes` / `ordered_prims` are
        not available on this object.  normals (per vertex) / prim_alpha (per entry of `prims`, the caller's order):
        what the smooth alpha-tested kinds and the alpha-tested patches read.  alpha_textures: a sequence of
        AlphaTexture, the table the kinds 16 .. 19 index with v[3]; uvs gives them their (u, v)."""
        if split_method not in ("sah", "hlbvh"):
            raise NNBVHError(f'GPU build supports "sah" and "hlbvh", not "{split_method}"')
        self = cls.__new__(cls)
        L = _lib.lib()
        prims = np.ascontiguousarray(prims, PRIM_DTYPE)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        pb = None
        if prim_bounds is not None:
            pb = np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
        self.nodes = self.ordered_prims = None
        self.verts = verts
        self.device = int(device)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(len(verts), 3)
        pa = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(len(prims))
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(len(verts), 2)
        if alpha_textures is not None:
            self.alpha_textures, n_tex = _lib.alpha_texture_table(alpha_textures)
            self._h = L.nnbvh_scene_create_gpu_build_with_alpha_textures(
                ptr(prims), len(prims), ptr(verts), len(verts), ptr(pb) if pb is not None else None,
                ptr(nrm) if nrm is not None else None, ptr(uv) if uv is not None else None,
                ptr(pa) if pa is not None else None, int(max_prims_in_node), SPLIT_METHODS[split_method], self.device,
                self.alpha_textures, n_tex)
        else:
            self._h = L.nnbvh_scene_create_gpu_build_with_attributes(
                ptr(prims), len(prims), ptr(verts), len(verts), ptr(pb) if pb is not None else None,
                ptr(nrm) if nrm is not None else None, ptr(uv) if uv is not None else None,
                ptr(pa) if pa is not None else None,
                int(max_prims_in_node), SPLIT_METHODS[split_method], self.device)
        if not self._h:
            raise NNBVHError("nnbvh_scene_create_gpu_build: " + _lib.last_error())
        self._read_info()
        return self

    @staticmethod
    def two_level_entries(top_prims, objects, placements):
        """The primitive list nnbvh_scene_create_instanced_gpu_build takes, made of assemble_two_level's inputs:
        the top-level primitives, the instance entries assemble_two_level generates (kind 2, v[0] = j,
        id = n_top + j), then the objects one after another.  Returns (prims, n_top_prims, object_first)."""
        top_prims = np.asarray(top_prims, PRIM_DTYPE).reshape(-1)
        n_top = len(top_prims)
        inst_prims = np.zeros(len(placements), PRIM_DTYPE)
        inst_prims["kind"] = 2
        inst_prims["v"][:, 0] = np.arange(len(placements))
        inst_prims["id"] = n_top + np.arange(len(placements))
        objects = [np.asarray(o, PRIM_DTYPE).reshape(-1) for o in objects]
        prims = np.ascontiguousarray(np.concatenate([top_prims, inst_prims] + objects), PRIM_DTYPE)
        first = n_top + len(placements) + np.concatenate([[0], np.cumsum([len(o) for o in objects])])
        return prims, n_top + len(placements), np.ascontiguousarray(first, np.int32)

    @classmethod
    def build_two_level_on_device(cls, top_prims, verts, objects, placements, max_prims_in_node=4, split_method="sah",
                                  animated=None, prim_bounds=None, normals=None, prim_alpha=None, uvs=None, device=0,
                                  alpha_textures=None):
        """A two-level scene (instancing.assemble_two_level's inputs: top-level primitives, object definitions,
        placements (object index, render_from_prim 3x4, prim_from_render 3x4)) with every tree built AND baked on
        the GPU (nnbvh_scene_create_instanced_gpu_build); byte-identical device arrays and the same results as
        assemble_two_level + from_tree.  prim_bounds / prim_alpha: per entry of two_level_entries(...)[0] (the top
        list, the generated instance entries, then the objects); prim_bounds is read for host-only primitives and
        the instances of animated placements only.  animated: ANIMATED_DTYPE, one per placement.  `nodes` /
        `ordered_prims` are not available on this object; `instances` is the placement table in the form
        ShadingMesh.set_instances takes (root / n_nodes zero: the trees live on the device).  alpha_textures: a
        sequence of AlphaTexture, the table the kinds 16 .. 19 index with v[3], in objects and in the top-level list
        (nnbvh_scene_create_instanced_gpu_build_with_alpha_textures); uvs gives them their (u, v)."""
        if split_method not in ("sah", "hlbvh"):
            raise NNBVHError(f'GPU build supports "sah" and "hlbvh", not "{split_method}"')
        self = cls.__new__(cls)
        L = _lib.lib()
        prims, n_top, first = cls.two_level_entries(top_prims, objects, placements)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        table = np.zeros(len(placements), _lib.PLACEMENT_DTYPE)
        self.instances = np.zeros(len(placements), _lib.INSTANCE_DTYPE)
        for j, (k, m, mi) in enumerate(placements):
            table[j]["render_from_prim"] = np.asarray(m, np.float32).reshape(12)
            table[j]["prim_from_render"] = np.asarray(mi, np.float32).reshape(12)
            table[j]["object"] = int(k)
        self.instances["render_from_prim"] = table["render_from_prim"]
        self.instances["prim_from_render"] = table["prim_from_render"]
        self.nodes = self.ordered_prims = None
        self.verts = verts
        self.device = int(device)
        self.animated = None if animated is None else np.ascontiguousarray(animated, _lib.ANIMATED_DTYPE)
        if self.animated is not None and len(self.animated) != len(placements):
            raise NNBVHError(f"animated has {len(self.animated)} entries for {len(placements)} placements")
        if alpha_textures is not None:  # (the length faults as NNBVHError, not as reshape's ValueError)
            for name, a, n, w in (("normals", normals, len(verts), 3), ("uvs", uvs, len(verts), 2),
                                  ("prim_alpha", prim_alpha, len(prims), 1)):
                if a is not None and np.asarray(a).size != n * w:
                    raise NNBVHError(f"{name} has {np.asarray(a).size // w} entries where the scene has {n}")
        pb = None if prim_bounds is None else np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(len(verts), 3)
        pa = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(len(prims))
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(len(verts), 2)
        opt = lambda a: ptr(a) if a is not None and len(a) else None  # noqa: E731
        args = (opt(prims), len(prims), n_top, ptr(first), len(objects), opt(verts), len(verts), opt(nrm), opt(uv), opt(pa),
                opt(pb), opt(table), len(table), opt(self.animated), int(max_prims_in_node), SPLIT_METHODS[split_method],
                self.device)
        if alpha_textures is not None:
            self.alpha_textures, n_tex = _lib.alpha_texture_table(alpha_textures)
            self._h = L.nnbvh_scene_create_instanced_gpu_build_with_alpha_textures(*args, self.alpha_textures, n_tex)
        else:
            self._h = L.nnbvh_scene_create_instanced_gpu_build(*args)
        if not self._h:
            raise NNBVHError("nnbvh_scene_create_instanced_gpu_build: " + _lib.last_error())
        self._read_info()
        return self

    def read(self, what):
        """The baked device arrays (nnbvh_scene_read) as bytes-exact numpy arrays: 0 = interior records
        (uint32 [n, 16]), 1 = primitive stream (uint32 [slots, 4]), 2 = animation table (float32 [instances, 76];
        None for scenes without one), 3 = alpha-texture descriptor table (uint32 [textures, 12]), 4 = alpha texel pool
        (float32 [texels]; both None for scenes without alpha textures)."""
        if what not in (0, 1, 2, 3, 4):
            raise NNBVHError(f"read: unknown array {what!r} (0 interior records, 1 primitive stream, 2 animation table, "
                             "3 alpha-texture table, 4 alpha texel pool)")
        if what in (3, 4):
            table = getattr(self, "alpha_textures", None)
            if table is None:
                return None
            out = (np.zeros((len(table), 12), np.uint32) if what == 3
                   else np.zeros(sum(t.width * t.height for t in table), np.float32))
        elif what == 2:
            n = 0 if getattr(self, "animated", None) is None else len(self.animated)
            if n == 0:
                return None
            out = np.zeros((n, 76), np.float32)
        elif what == 0:
            out = np.zeros((self.info["interior_records"], 16), np.uint32)
        else:
            out = np.zeros((self.info["prim_slots"], 4), np.uint32)
        if out.nbytes:
            check(_lib.lib().nnbvh_scene_read(self._h, int(what), ptr(out), out.nbytes), "nnbvh_scene_read")
        return out

    def _read_info(self):
        info = np.zeros(6, np.int64)
        check(_lib.lib().nnbvh_scene_info(self._h, ptr(info)), "nnbvh_scene_info")
        self.info = {"interior_records": int(info[0]), "prim_slots": int(info[1]),
                     "depth": int(info[2]), "device_bytes": int(info[3]),
                     "grid_blocks": int(info[4]), "stack_window": int(info[5])}

    def _init(self, nodes, ordered_prims, verts, device, depth, instances=None, n_top_nodes=None, animated=None,
              normals=None, prim_alpha=None, uvs=None, alpha_textures=None):
        L = _lib.lib()
        self.nodes = np.ascontiguousarray(nodes, NODE_DTYPE)
        self.ordered_prims = np.ascontiguousarray(ordered_prims, PRIM_DTYPE)
        self.verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        self.device = int(device)
        if alpha_textures is not None and instances is not None and len(instances):
            self.instances = np.ascontiguousarray(instances, _lib.INSTANCE_DTYPE)
            f32 = lambda a, w: None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, w)  # noqa: E731
            self.normals, self.uvs = f32(normals, 3), f32(uvs, 2)
            self.prim_alpha = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(-1)
            self.animated = None if animated is None else np.ascontiguousarray(animated, _lib.ANIMATED_DTYPE)
            for name, a, n in (("normals", self.normals, len(self.verts)), ("uvs", self.uvs, len(self.verts)),
                               ("prim_alpha", self.prim_alpha, len(self.ordered_prims)),
                               ("animated", self.animated, len(self.instances))):
                if a is not None and len(a) != n:
                    raise NNBVHError(f"{name} has {len(a)} entries where the scene has {n}")
            self.alpha_textures, n_tex = _lib.alpha_texture_table(alpha_textures)
            opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
            self._h = L.nnbvh_scene_create_instanced_with_alpha_textures(
                ptr(self.nodes), len(self.nodes), int(n_top_nodes), ptr(self.ordered_prims), len(self.ordered_prims),
                ptr(self.verts), len(self.verts), ptr(self.instances), len(self.instances), opt(self.animated),
                opt(self.normals), opt(self.uvs), opt(self.prim_alpha), self.device, self.alpha_textures, n_tex)
        elif alpha_textures is not None:
            self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            self.prim_alpha = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(-1)
            self.uvs = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
            assert self.prim_alpha is None or len(self.prim_alpha) == len(self.ordered_prims)
            assert self.normals is None or len(self.normals) == len(self.verts)
            assert self.uvs is None or len(self.uvs) == len(self.verts)
            self.alpha_textures, n_tex = _lib.alpha_texture_table(alpha_textures)
            opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
            self._h = L.nnbvh_scene_create_with_alpha_textures(
                ptr(self.nodes), len(self.nodes), ptr(self.ordered_prims), len(self.ordered_prims), ptr(self.verts),
                opt(self.normals), opt(self.uvs), opt(self.prim_alpha), len(self.verts), self.device,
                self.alpha_textures, n_tex)
        elif instances is not None and len(instances):
            self.instances = np.ascontiguousarray(instances, _lib.INSTANCE_DTYPE)
            if normals is not None or prim_alpha is not None or uvs is not None:
                f32 = lambda a, w: None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, w)  # noqa: E731
                self.normals, self.uvs = f32(normals, 3), f32(uvs, 2)
                self.prim_alpha = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(-1)
                self.animated = None if animated is None else np.ascontiguousarray(animated, _lib.ANIMATED_DTYPE)
                opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
                self._h = L.nnbvh_scene_create_instanced_with_attributes(
                    ptr(self.nodes), len(self.nodes), int(n_top_nodes), ptr(self.ordered_prims),
                    len(self.ordered_prims), ptr(self.verts), len(self.verts), ptr(self.instances),
                    len(self.instances), opt(self.animated), opt(self.normals), opt(self.uvs), opt(self.prim_alpha),
                    self.device)
            elif animated is not None:
                self.animated = np.ascontiguousarray(animated, _lib.ANIMATED_DTYPE)
                assert len(self.animated) == len(self.instances)
                self._h = L.nnbvh_scene_create_instanced_animated(
                    ptr(self.nodes), len(self.nodes), int(n_top_nodes), ptr(self.ordered_prims),
                    len(self.ordered_prims), ptr(self.verts), len(self.verts), ptr(self.instances),
                    len(self.instances), ptr(self.animated), self.device)
            else:
                self._h = L.nnbvh_scene_create_instanced(
                    ptr(self.nodes), len(self.nodes), int(n_top_nodes), ptr(self.ordered_prims),
                    len(self.ordered_prims), ptr(self.verts), len(self.verts), ptr(self.instances),
                    len(self.instances), self.device)
        elif prim_alpha is not None:
            self.normals = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            self.prim_alpha = np.ascontiguousarray(prim_alpha, np.float32).reshape(-1)
            self.uvs = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(-1, 2)
            assert len(self.prim_alpha) == len(self.ordered_prims)
            assert self.normals is None or len(self.normals) == len(self.verts)
            assert self.uvs is None or len(self.uvs) == len(self.verts)
            self._h = L.nnbvh_scene_create_with_attributes(
                ptr(self.nodes), len(self.nodes), ptr(self.ordered_prims), len(self.ordered_prims), ptr(self.verts),
                ptr(self.normals) if self.normals is not None else None,
                ptr(self.uvs) if self.uvs is not None else None, ptr(self.prim_alpha), len(self.verts), self.device)
        elif normals is not None:
            self.normals = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
            assert len(self.normals) == len(self.verts)
            self._h = L.nnbvh_scene_create_with_normals(ptr(self.nodes), len(self.nodes), ptr(self.ordered_prims),
                                                        len(self.ordered_prims), ptr(self.verts), ptr(self.normals),
                                                        len(self.verts), self.device)
        else:
            self._h = L.nnbvh_scene_create(ptr(self.nodes), len(self.nodes), ptr(self.ordered_prims),
                                           len(self.ordered_prims), ptr(self.verts), len(self.verts),
                                           self.device)
        if not self._h:
            raise NNBVHError("nnbvh_scene_create: " + _lib.last_error())
        self._read_info()

    def close(self):
        if getattr(self, "_h", None):
            _lib.lib().nnbvh_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, key, value):
        """nnbvh_scene_set_option (include/nnbvh.h lists the keys): speed only, never results.  "offsets32" 0 makes the
        scene behave as if it did not fit 32-bit offsets (never the lean instances, no LDS top table: the general
        instances, correct for every scene); 1 restores what the scene's sizes say."""
        check(_lib.lib().nnbvh_scene_set_option(self._h, key.encode(), int(value)),
              f"set_option({key})")

    def sched_stats(self, reset=True):
        """Diagnostics (NNBVH_STATS builds): trips and lanes per step kind."""
        out = np.zeros(20, np.uint64)
        check(_lib.lib().nnbvh_scene_sched_stats(self._h, ptr(out), int(reset)), "sched_stats")
        return dict(zip(("int_trips", "int_lanes", "prim_trips", "prim_lanes", "refill_trips",
                         "refill_lanes", "i_nint", "i_nprim", "i_nidle", "spare0", "int_cycles",
                         "prim_cycles", "refill_cycles", "int_top_lanes", "int_steps", "int_step_lanes",
                         "table_trips", "table_lanes", "table_cycles", "spare1"),
                        (int(x) for x in out)))

    # -- reference interface ----------------------------------------------------------
    def Bounds(self):
        out = np.zeros(6, np.float32)
        check(_lib.lib().nnbvh_scene_bounds(self._h, ptr(out)), "nnbvh_scene_bounds")
        return out[:3].copy(), out[3:].copy()

    def Intersect(self, rays, out=None):
        """Closest hit for a host ray batch (RAY_DTYPE) -> HIT_DTYPE array (`out`: write into this array,
        e.g. one the caller has pinned)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE) if out is None else out
        assert hits.dtype == HIT_DTYPE and len(hits) == len(rays) and hits.flags.c_contiguous
        check(_lib.lib().nnbvh_intersect_closest(self._h, ptr(rays), len(rays), ptr(hits)),
              "nnbvh_intersect_closest")
        return hits

    def IntersectP(self, rays, counts=False):
        """Any hit -> uint8 occluded[, nodes_visited, prim_tests]."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        occ = np.zeros(len(rays), np.uint8)
        if counts:
            vis = np.zeros(len(rays), np.int32)
            tst = np.zeros(len(rays), np.int32)
            check(_lib.lib().nnbvh_intersect_any(self._h, ptr(rays), len(rays), ptr(occ),
                                                 ptr(vis), ptr(tst)), "nnbvh_intersect_any")
            return occ, vis, tst
        check(_lib.lib().nnbvh_intersect_any(self._h, ptr(rays), len(rays), ptr(occ), None, None),
              "nnbvh_intersect_any")
        return occ

    # -- device-resident batches (torch tensors are only buffers + the current stream) ----
    def intersect_device(self, d_rays, d_hits, n, stream=0):
        check(_lib.lib().nnbvh_intersect_closest_device(self._h, d_rays, n, d_hits, stream),
              "nnbvh_intersect_closest_device")

    def trace_batches_device(self, batches, stream=0):
        """batches: iterable of (kind, d_rays, n, d_out[, d_nodes_visited, d_prim_tests]) with kind
        "closest" or "any"; all traced concurrently, ordered as one operation on `stream`."""
        arr = np.zeros(len(batches), _lib.BATCH_DTYPE)
        for i, b in enumerate(batches):
            arr[i]["kind"] = {"closest": 0, "any": 1}[b[0]]
            arr[i]["d_rays"], arr[i]["n"], arr[i]["d_out"] = b[1], b[2], b[3]
            if len(b) > 4:
                arr[i]["d_nodes_visited"], arr[i]["d_prim_tests"] = b[4] or 0, b[5] or 0
        check(_lib.lib().nnbvh_trace_batches_device(self._h, ptr(arr), len(arr), stream),
              "nnbvh_trace_batches_device")

    def trace_batches_candidates_device(self, batches, candidates, stream=0):
        """trace_batches_device with host candidates per batch (nnbvh_trace_batches_candidates_device).
        candidates[b]: None for a plain batch, else (capacity, d_count, d_before, d_prim, d_instance) device
        pointers (d_before None for an "any" batch), filled as by intersect[_p]_candidates_device."""
        assert len(candidates) == len(batches)
        arr = np.zeros(len(batches), _lib.BATCH_DTYPE)
        for i, b in enumerate(batches):
            arr[i]["kind"] = {"closest": 0, "any": 1}[b[0]]
            arr[i]["d_rays"], arr[i]["n"], arr[i]["d_out"] = b[1], b[2], b[3]
            if len(b) > 4:
                arr[i]["d_nodes_visited"], arr[i]["d_prim_tests"] = b[4] or 0, b[5] or 0
        cs = (_lib.HostCandidates * max(len(batches), 1))()
        for i, c in enumerate(candidates):
            if c is not None:
                cs[i] = _lib.HostCandidates(int(c[0]), c[1], c[2], c[3], c[4])
        check(_lib.lib().nnbvh_trace_batches_candidates_device(self._h, ptr(arr), len(arr), cs, stream),
              "nnbvh_trace_batches_candidates_device")

    def intersect_p_device(self, d_rays, d_occ, n, d_visited=None, d_tests=None, stream=0):
        check(_lib.lib().nnbvh_intersect_any_device(self._h, d_rays, n, d_occ, d_visited, d_tests,
                                                    stream), "nnbvh_intersect_any_device")

    # -- host-only primitives as candidates (include/nnbvh.h nnbvh_host_candidates) -----------
    def intersect_with_host_candidates(self, rays, capacity=8):
        """Closest hit that lists the host-only primitives each ray reached instead of voiding it.
        Returns (hits, cands): hits as Intersect (the closest DEVICE hit, its real instance unless
        cands["count"] < 0), cands a candidates_dtype(capacity) array; merge with resolve_host_candidates."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        cnt, before, prim, inst = _candidate_arrays(len(rays), capacity)
        c = _lib.HostCandidates(int(capacity), cnt.ctypes.data, before.ctypes.data, prim.ctypes.data, inst.ctypes.data)
        check(_lib.lib().nnbvh_intersect_closest_candidates(self._h, ptr(rays), len(rays), ptr(hits), ctypes.byref(c)),
              "nnbvh_intersect_closest_candidates")
        return hits, _pack_candidates(cnt, before, prim, inst)

    def intersect_p_with_host_candidates(self, rays, capacity=8):
        """Occlusion-only any hit with candidates -> (occluded uint8, cands); cands["before"] is 0.
        occluded 2 with count > 0: test the candidates (resolve_host_candidates_any)."""
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        occ = np.zeros(len(rays), np.uint8)
        cnt, before, prim, inst = _candidate_arrays(len(rays), capacity)
        c = _lib.HostCandidates(int(capacity), cnt.ctypes.data, None, prim.ctypes.data, inst.ctypes.data)
        check(_lib.lib().nnbvh_intersect_any_candidates(self._h, ptr(rays), len(rays), ptr(occ), ctypes.byref(c)),
              "nnbvh_intersect_any_candidates")
        return occ, _pack_candidates(cnt, before, prim, inst)

    def intersect_candidates_device(self, d_rays, d_hits, n, capacity, d_count, d_before, d_prim, d_instance,
                                    stream=0):
        """intersect_device with candidates: device pointers int32[n] count / before, int32[n * capacity]
        prim / instance (nnbvh_intersect_closest_candidates_device)."""
        c = _lib.HostCandidates(int(capacity), d_count, d_before, d_prim, d_instance)
        check(_lib.lib().nnbvh_intersect_closest_candidates_device(self._h, d_rays, n, d_hits, ctypes.byref(c), stream),
              "nnbvh_intersect_closest_candidates_device")

    def intersect_p_candidates_device(self, d_rays, d_occ, n, capacity, d_count, d_prim, d_instance, stream=0):
        c = _lib.HostCandidates(int(capacity), d_count, None, d_prim, d_instance)
        check(_lib.lib().nnbvh_intersect_any_candidates_device(self._h, d_rays, n, d_occ, ctypes.byref(c), stream),
              "nnbvh_intersect_any_candidates_device")


def candidates_dtype(capacity):
    """Per-ray host candidates: count (0..K; -1 more than K; -2 alpha re-trace: void), before (closest hit:
    candidates met before the device hit), prim[K] (nnbvh_prim.id), instance[K] (0 top level, k + 1 instance k)."""
    return np.dtype([("count", "<i4"), ("before", "<i4"), ("prim", "<i4", capacity), ("instance", "<i4", capacity)])


def _candidate_arrays(n, capacity):
    if not 1 <= int(capacity) <= 16:
        raise NNBVHError(f"host candidates: capacity must be 1..16, not {capacity}")
    k = int(capacity)
    return (np.zeros(n, np.int32), np.zeros(n, np.int32), np.full((n, k), -1, np.int32),
            np.full((n, k), -1, np.int32))


def _pack_candidates(cnt, before, prim, inst):
    out = np.zeros(len(cnt), candidates_dtype(prim.shape[1]))
    out["count"], out["before"], out["prim"], out["instance"] = cnt, before, prim, inst
    return out


def _test_candidates(rays, res, tmax, cands, host_intersect, lo, hi):
    """Test candidate columns j with lo[i] <= j < hi[i] in order; a hit replaces the result and sets tMax.
    Returns which rays accepted a candidate."""
    took = np.zeros(len(rays), bool)
    for j in range(cands["prim"].shape[1]):
        idx = np.nonzero((lo <= j) & (j < hi))[0]
        if len(idx) == 0:
            continue
        prim, inst = cands["prim"][idx, j], cands["instance"][idx, j]
        hit, t, b0, b1, b2 = (np.asarray(x) for x in host_intersect(idx, prim, inst, tmax[idx].copy()))
        w = idx[hit.astype(bool)]
        h = hit.astype(bool)
        res["prim"][w], res["instance"][w] = prim[h], inst[h]
        res["t"][w], res["b0"][w], res["b1"][w], res["b2"][w] = t[h], b0[h], b1[h], b2[h]
        tmax[w] = t[h]
        took[w] = True
    return took


def resolve_host_candidates(rays, hits, cands, host_intersect, kind=None, device_intersect=None):
    """Merge the device hit with the caller's tests of the host candidates (the rule of include/nnbvh.h):
    candidates 0 .. before-1, then the device hit, then candidates before .. count-1, each accepted against the
    running tMax and replacing the result.

    host_intersect(ray_idx, prim, instance, tmax) -> (hit, t, b0, b1, b2): vectorised over one candidate column
    (arrays of the same length); the ray is rays[ray_idx] in render space, transforming it into an instance's
    space is the callback's job (as TransformedPrimitive's).
    kind: array indexed by nnbvh_prim.id (the device primitives' kinds, NNBVH_PRIM_*); a device hit after an
    accepted candidate stands iff t <= tMax (triangle kinds) or t < tMax (bilinear patch kinds).  None = every
    device primitive is a triangle.
    device_intersect: optional callback like host_intersect for the DEVICE primitives; when given, a device hit
    after an accepted candidate is re-tested with it at the reduced tMax instead of being compared on t — the
    reference's own test, exact also where t lies within an ulp of tMax.
    Rays with count < 0 stay void (instance -1).  nodes_visited / prim_tests are the device walk's."""
    rays = np.asarray(rays)
    res = hits.copy()
    cnt, before = cands["count"], cands["before"]
    ok = cnt >= 0
    tmax = rays["tmax"].astype(np.float32).copy()
    first = np.where(ok, before, 0)
    # the running result starts as a miss; the device hit is inserted between the two candidate runs
    res["prim"][ok], res["t"][ok], res["instance"][ok] = -1, tmax[ok], 0
    res["b0"][ok] = res["b1"][ok] = res["b2"][ok] = 0
    took = _test_candidates(rays, res, tmax, cands, host_intersect, np.zeros_like(first), first)
    dev = ok & (hits["prim"] >= 0)
    accept = dev & ~took
    ask = np.nonzero(dev & took)[0]
    if len(ask):
        t = hits["t"][ask]
        if device_intersect is not None:
            acc = np.asarray(device_intersect(ask, hits["prim"][ask], hits["instance"][ask], tmax[ask].copy())[0])
            acc = acc.astype(bool)
        else:
            patch = np.zeros(len(ask), bool)
            if kind is not None:
                k = np.asarray(kind)[hits["prim"][ask]]
                patch = (k == 1) | ((k >= 8) & (k <= 15))
            acc = np.where(patch, t < tmax[ask], t <= tmax[ask])
        accept[ask[acc]] = True
    w = np.nonzero(accept)[0]
    for f in ("prim", "t", "b0", "b1", "b2", "instance"):
        res[f][w] = hits[f][w]
    tmax[w] = hits["t"][w]
    _test_candidates(rays, res, tmax, cands, host_intersect, first, np.where(ok, cnt, 0))
    return res


def resolve_host_candidates_any(rays, occluded, cands, host_intersect):
    """Any hit: occluded = device occluded or some candidate hits with ray.tmax (host_intersect as in
    resolve_host_candidates).  Rays with occluded 2 and count < 0 stay 2 (void)."""
    rays = np.asarray(rays)
    res = np.asarray(occluded).copy()
    cnt = cands["count"]
    todo = (res == 2) & (cnt > 0)
    res[todo] = 0
    for j in range(cands["prim"].shape[1]):
        idx = np.nonzero(todo & (j < cnt) & (res == 0))[0]
        if len(idx) == 0:
            continue
        hit = np.asarray(host_intersect(idx, cands["prim"][idx, j], cands["instance"][idx, j],
                                        rays["tmax"][idx].astype(np.float32))[0]).astype(bool)
        res[idx[hit]] = 1
    return res
