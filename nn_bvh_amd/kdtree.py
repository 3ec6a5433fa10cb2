"""Host-side mirror of the KdTreeAggregate entry points (include/nnbvh.h, nnbvh_kd_*): pbrt's
kd-tree accelerator (/root/reference/src/pbrt/cpu/aggregates.cpp:746-1161) and an importer for the
plane arrays the nss learned kd-trees are exported as (machine_learning/nss_kd_tree.py:204-240)."""
import collections
import ctypes

import numpy as np

from . import _lib
from ._lib import HIT_DTYPE, KD_NODE_DTYPE, PRIM_DTYPE, RAY_DTYPE, check, ptr

KdBuilt = collections.namedtuple("KdBuilt", "nodes prim_indices bounds depth build_ms", defaults=((0.0, 0.0),))


def build_kd_tree(prims, verts, prim_bounds=None, isect_cost=5, traversal_cost=1, empty_bonus=0.5, max_prims=1,
                  max_depth=-1, where="host", device=0):
    """KdTreeAggregate's constructor (aggregates.cpp:798-971); defaults are those of KdTreeAggregate::Create
    (aggregates.cpp:1152-1161).  where: "host" (libstdc++'s std::sort order inside multi-primitive leaves),
    "host_stable" (std::stable_sort order) or "gpu" (the device builder: the same arrays as "host_stable")."""
    L = _lib.lib()
    prims = np.ascontiguousarray(prims, PRIM_DTYPE)
    verts = np.ascontiguousarray(verts, np.float32)
    pb = None if prim_bounds is None else np.ascontiguousarray(prim_bounds, np.float32)
    args = (ptr(prims), len(prims), ptr(verts), len(verts), None if pb is None else ptr(pb),
            isect_cost, traversal_cost, ctypes.c_float(empty_bonus), max_prims, max_depth)
    if where == "gpu":
        h = L.nnbvh_kd_build_create_gpu(*args, device)
    elif where == "host_stable":
        h = L.nnbvh_kd_build_create_stable(*args)
    else:
        h = L.nnbvh_kd_build_create(*args)
    if not h:
        raise _lib.NNBVHError(f"nnbvh_kd_build_create ({where}) failed: {_lib.last_error()}")
    try:
        n = ctypes.c_int()
        p = L.nnbvh_kd_build_nodes(h, ctypes.byref(n))
        nodes = np.frombuffer((ctypes.c_char * (n.value * 8)).from_address(p), KD_NODE_DTYPE).copy()
        p = L.nnbvh_kd_build_prim_indices(h, ctypes.byref(n))
        idx = (np.frombuffer((ctypes.c_char * (n.value * 4)).from_address(p), np.int32).copy()
               if n.value else np.zeros(0, np.int32))
        bounds = np.zeros(6, np.float32)
        check(L.nnbvh_kd_build_bounds(h, ptr(bounds)), "nnbvh_kd_build_bounds")
        depth = L.nnbvh_kd_build_depth(h)
        ms = np.zeros(2, np.float64)
        check(L.nnbvh_kd_build_timing(h, ptr(ms)), "nnbvh_kd_build_timing")
    finally:
        L.nnbvh_kd_build_destroy(h)
    return KdBuilt(nodes, idx, bounds, depth, (float(ms[0]), float(ms[1])))


class KdTreeAggregate:
    """KdTreeAggregate (cpu/aggregates.h:75-105) resident on the device."""

    def __init__(self, handle, bounds, device=0):
        self._h = handle
        self.bounds = bounds
        self.device = device
        self.alpha_textures = None  # the ctypes table of a scene with image-textured alpha

    @classmethod
    def from_tree(cls, nodes, prim_indices, prims, verts, bounds, device=0, normals=None, uvs=None, prim_alpha=None,
                  alpha_textures=None):
        """normals / uvs (per vertex) and prim_alpha (per entry of prims): what the alpha-tested kinds of smooth meshes
        and the alpha-tested patches read; without them such primitives are the host's (void records).
        alpha_textures: a sequence of AlphaTexture, the table the kinds 16 .. 19 index with v[3]
        (nnbvh_kd_scene_create_with_alpha_textures); uvs gives them their (u, v) (None: the default corners)."""
        nodes = np.ascontiguousarray(nodes, KD_NODE_DTYPE)
        idx = np.ascontiguousarray(prim_indices, np.int32)
        prims = np.ascontiguousarray(prims, PRIM_DTYPE)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        bounds = np.ascontiguousarray(bounds, np.float32)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(len(verts), 3)
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(len(verts), 2)
        pa = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(len(prims))
        opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
        args = (ptr(nodes), len(nodes), ptr(idx) if len(idx) else None, len(idx), ptr(prims), len(prims), ptr(verts),
                len(verts), ptr(bounds), opt(nrm), opt(uv), opt(pa), device)
        if alpha_textures is not None:
            table, n_tex = _lib.alpha_texture_table(alpha_textures)
            h = _lib.lib().nnbvh_kd_scene_create_with_alpha_textures(*args, table, n_tex)
        else:
            table = None
            h = _lib.lib().nnbvh_kd_scene_create_with_attributes(*args)
        if not h:
            raise _lib.NNBVHError(f"nnbvh_kd_scene_create failed: {_lib.last_error()}")
        self = cls(h, bounds, device)
        self.alpha_textures = table  # kept alive with the scene, as BVHAggregate keeps its own
        return self

    @classmethod
    def build(cls, prims, verts, device=0, normals=None, uvs=None, prim_alpha=None, alpha_textures=None, **kw):
        t = build_kd_tree(prims, verts, **kw)
        return cls.from_tree(t.nodes, t.prim_indices, prims, verts, t.bounds, device, normals, uvs, prim_alpha,
                             alpha_textures)

    @classmethod
    def build_on_device(cls, prims, verts, device=0, normals=None, uvs=None, prim_alpha=None, prim_bounds=None,
                        isect_cost=5, traversal_cost=1, empty_bonus=0.5, max_prims=1, max_depth=-1, alpha_textures=None):
        """nnbvh_kd_scene_create_gpu_build_with_attributes (with alpha_textures, a sequence of AlphaTexture:
        nnbvh_kd_scene_create_gpu_build_with_alpha_textures): primitive bounds, the tree and the primitive records are
        made on the device and stay there.  The scene of build_kd_tree(where="host_stable") + from_tree, byte for byte:
        inside multi-primitive leaves the primitives stand in std::stable_sort order, not in the libstdc++ std::sort
        order of build() (the leaf-order note of build_kd_tree).  prim_bounds: read for host-only primitives only."""
        prims = np.ascontiguousarray(prims, PRIM_DTYPE)
        verts = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
        nrm = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(len(verts), 3)
        uv = None if uvs is None else np.ascontiguousarray(uvs, np.float32).reshape(len(verts), 2)
        pa = None if prim_alpha is None else np.ascontiguousarray(prim_alpha, np.float32).reshape(len(prims))
        pb = None if prim_bounds is None else np.ascontiguousarray(prim_bounds, np.float32).reshape(len(prims), 6)
        opt = lambda a: ptr(a) if a is not None and a.size else None  # noqa: E731
        L = _lib.lib()
        args = (opt(prims), len(prims), opt(verts), len(verts), opt(pb), opt(nrm), opt(uv), opt(pa), isect_cost,
                traversal_cost, ctypes.c_float(empty_bonus), max_prims, max_depth, device)
        if alpha_textures is not None:
            table, n_tex = _lib.alpha_texture_table(alpha_textures)
            h = L.nnbvh_kd_scene_create_gpu_build_with_alpha_textures(*args, table, n_tex)
        else:
            table = None
            h = L.nnbvh_kd_scene_create_gpu_build_with_attributes(*args)
        if not h:
            raise _lib.NNBVHError(f"nnbvh_kd_scene_create_gpu_build failed: {_lib.last_error()}")
        bounds = np.zeros(6, np.float32)
        agg = cls(h, bounds, device)
        agg.alpha_textures = table
        check(L.nnbvh_kd_scene_bounds(h, ptr(bounds)), "nnbvh_kd_scene_bounds")
        return agg

    INFO_KEYS = ("n_nodes", "n_indices", "n_prims", "depth", "device_bytes", "has_host_prims", "has_patches",
                 "has_attribute_slots")

    def info(self):
        """nnbvh_kd_scene_info as a dict (INFO_KEYS)."""
        out = np.zeros(8, np.int64)
        check(_lib.lib().nnbvh_kd_scene_info(self._h, ptr(out)), "nnbvh_kd_scene_info")
        return dict(zip(self.INFO_KEYS, (int(v) for v in out)))

    def read(self, what):
        """nnbvh_kd_scene_read: the scene's device arrays as numpy arrays.  what: 0 / "nodes" (KD_NODE_DTYPE), 1 /
        "prim_indices" (int32), 2 / "prims" (float32 [n, 16]: the 64-B records), 3 / "attributes" (float32 [n, 24]:
        the 96-B slots; empty in scenes without them), 4 / "alpha_textures" (uint32 [n, 12]: the 48-B descriptors), 5 /
        "alpha_texels" (float32: the texel pool; both empty in scenes without an alpha-texture table)."""
        what = {"nodes": 0, "prim_indices": 1, "prims": 2, "attributes": 3, "alpha_textures": 4,
                "alpha_texels": 5}.get(what, what)
        i = self.info()
        table = self.alpha_textures if self.alpha_textures is not None else ()
        rows, dtype, width = [(i["n_nodes"], KD_NODE_DTYPE, 1), (i["n_indices"], np.int32, 1),
                              (i["n_prims"], np.float32, 16),
                              (i["n_prims"] if i["has_attribute_slots"] else 0, np.float32, 24),
                              (len(table), np.uint32, 12),
                              (sum(t.width * t.height for t in table), np.float32, 1)][what]
        out = np.zeros(rows * width, dtype)
        check(_lib.lib().nnbvh_kd_scene_read(self._h, what, ptr(out) if out.size else None, out.nbytes),
              "nnbvh_kd_scene_read")
        return out if width == 1 else out.reshape(-1, width)

    def close(self):
        if self._h:
            _lib.lib().nnbvh_kd_scene_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def Bounds(self):
        return self.bounds[:3].copy(), self.bounds[3:].copy()

    def Intersect(self, rays):
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        check(_lib.lib().nnbvh_kd_intersect_closest(self._h, ptr(rays), len(rays), ptr(hits)),
              "nnbvh_kd_intersect_closest")
        return hits

    def IntersectP(self, rays, counts=False):
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        occ = np.zeros(len(rays), np.uint8)
        vis = np.zeros(len(rays), np.int32) if counts else None
        tst = np.zeros(len(rays), np.int32) if counts else None
        check(_lib.lib().nnbvh_kd_intersect_any(self._h, ptr(rays), len(rays), ptr(occ),
                                                ptr(vis) if counts else None, ptr(tst) if counts else None),
              "nnbvh_kd_intersect_any")
        return (occ, vis, tst) if counts else occ

    def intersect_device(self, d_rays, d_hits, n, stream=0):
        check(_lib.lib().nnbvh_kd_intersect_closest_device(self._h, ctypes.c_void_p(d_rays), n,
                                                           ctypes.c_void_p(d_hits), ctypes.c_void_p(stream)),
              "nnbvh_kd_intersect_closest_device")

    def intersect_p_device(self, d_rays, d_occ, n, d_visited=None, d_tests=None, stream=0):
        check(_lib.lib().nnbvh_kd_intersect_any_device(self._h, ctypes.c_void_p(d_rays), n, ctypes.c_void_p(d_occ),
                                                       ctypes.c_void_p(d_visited) if d_visited else None,
                                                       ctypes.c_void_p(d_tests) if d_tests else None,
                                                       ctypes.c_void_p(stream)),
              "nnbvh_kd_intersect_any_device")

    def set_option(self, key, value):
        """nnbvh_kd_scene_set_option: "read_soa", "pair_one_launch", "offsets32" (speed only, never results).
        "offsets32" 0 runs the kernel instances with 64-bit addressing (those of scenes beyond 4 GiB, correct for every
        scene) although this scene fits 32-bit offsets; 1 restores the width computed from the scene's sizes."""
        check(_lib.lib().nnbvh_kd_scene_set_option(self._h, key.encode(), int(value)), f"kd set_option({key})")

    def trace_batches_device(self, batches, stream=0):
        """nnbvh_kd_trace_batches_device: 1..4 independent batches, closest-hit and any-hit mixed, in ONE kernel launch
        on `stream`.  batches: iterable of (kind, d_rays, n, d_out[, d_visited, d_tests]) with kind "closest"
        (d_out: HIT_DTYPE records) or "any" (d_out: uint8 flags; the optional int32 arrays get the exact counts);
        device pointers."""
        rec = np.zeros(len(batches), _lib.BATCH_DTYPE)
        for k, b in enumerate(batches):
            kind, d_rays, n, d_out = b[:4]
            rec[k]["kind"] = {"closest": 0, "any": 1}[kind]
            rec[k]["d_rays"], rec[k]["n"], rec[k]["d_out"] = d_rays or 0, n, d_out or 0
            rec[k]["d_nodes_visited"] = (b[4] or 0) if len(b) > 4 else 0
            rec[k]["d_prim_tests"] = (b[5] or 0) if len(b) > 5 else 0
        check(_lib.lib().nnbvh_kd_trace_batches_device(self._h, ptr(rec) if len(rec) else None, len(rec),
                                                       ctypes.c_void_p(stream)),
              "nnbvh_kd_trace_batches_device")

    # -- host-only primitives as candidates (include/nnbvh.h nnbvh_host_candidates; the BVHAggregate methods of the
    # same names, with instance 0 in every entry and a primitive listed once however many leaves hold it) ----------
    def intersect_with_host_candidates(self, rays, capacity=8):
        """Closest hit that lists the host-only primitives each ray reached instead of voiding it.  Returns
        (hits, cands) as BVHAggregate.intersect_with_host_candidates; merge with resolve_host_candidates."""
        from .aggregate import _candidate_arrays, _pack_candidates
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        hits = np.zeros(len(rays), HIT_DTYPE)
        cnt, before, prim, inst = _candidate_arrays(len(rays), capacity)
        c = _lib.HostCandidates(int(capacity), cnt.ctypes.data, before.ctypes.data, prim.ctypes.data, inst.ctypes.data)
        check(_lib.lib().nnbvh_kd_intersect_closest_candidates(self._h, ptr(rays), len(rays), ptr(hits),
                                                               ctypes.byref(c)),
              "nnbvh_kd_intersect_closest_candidates")
        return hits, _pack_candidates(cnt, before, prim, inst)

    def intersect_p_with_host_candidates(self, rays, capacity=8):
        """Any hit with candidates -> (occluded uint8, cands); cands["before"] is 0.  occluded 2 with count > 0: test
        the candidates (resolve_host_candidates_any)."""
        from .aggregate import _candidate_arrays, _pack_candidates
        rays = np.ascontiguousarray(rays, RAY_DTYPE)
        occ = np.zeros(len(rays), np.uint8)
        cnt, before, prim, inst = _candidate_arrays(len(rays), capacity)
        c = _lib.HostCandidates(int(capacity), cnt.ctypes.data, None, prim.ctypes.data, inst.ctypes.data)
        check(_lib.lib().nnbvh_kd_intersect_any_candidates(self._h, ptr(rays), len(rays), ptr(occ), ctypes.byref(c)),
              "nnbvh_kd_intersect_any_candidates")
        return occ, _pack_candidates(cnt, before, prim, inst)

    def intersect_candidates_device(self, d_rays, d_hits, n, capacity, d_count, d_before, d_prim, d_instance,
                                    stream=0):
        """intersect_device with candidates: device pointers int32[n] count / before, int32[n * capacity] prim /
        instance (nnbvh_kd_intersect_closest_candidates_device)."""
        c = _lib.HostCandidates(int(capacity), d_count, d_before, d_prim, d_instance)
        check(_lib.lib().nnbvh_kd_intersect_closest_candidates_device(self._h, d_rays, n, d_hits, ctypes.byref(c),
                                                                      stream),
              "nnbvh_kd_intersect_closest_candidates_device")

    def intersect_p_candidates_device(self, d_rays, d_occ, n, capacity, d_count, d_prim, d_instance, stream=0):
        c = _lib.HostCandidates(int(capacity), d_count, None, d_prim, d_instance)
        check(_lib.lib().nnbvh_kd_intersect_any_candidates_device(self._h, d_rays, n, d_occ, ctypes.byref(c), stream),
              "nnbvh_kd_intersect_any_candidates_device")

    def trace_batches_candidates_device(self, batches, candidates, stream=0):
        """trace_batches_device with host candidates per batch (nnbvh_kd_trace_batches_candidates_device), ONE launch.
        candidates[b]: None for a plain batch, else (capacity, d_count, d_before, d_prim, d_instance) device pointers
        (d_before None for an "any" batch), filled as by intersect[_p]_candidates_device."""
        assert len(candidates) == len(batches)
        rec = np.zeros(len(batches), _lib.BATCH_DTYPE)
        for k, b in enumerate(batches):
            kind, d_rays, n, d_out = b[:4]
            rec[k]["kind"] = {"closest": 0, "any": 1}[kind]
            rec[k]["d_rays"], rec[k]["n"], rec[k]["d_out"] = d_rays or 0, n, d_out or 0
            rec[k]["d_nodes_visited"] = (b[4] or 0) if len(b) > 4 else 0
            rec[k]["d_prim_tests"] = (b[5] or 0) if len(b) > 5 else 0
        cs = (_lib.HostCandidates * max(len(batches), 1))()
        for k, c in enumerate(candidates):
            if c is not None:
                cs[k] = _lib.HostCandidates(int(c[0]), c[1], c[2], c[3], c[4])
        check(_lib.lib().nnbvh_kd_trace_batches_candidates_device(self._h, ptr(rec) if len(rec) else None, len(rec),
                                                                  cs, ctypes.c_void_p(stream)),
              "nnbvh_kd_trace_batches_candidates_device")


# ---- nss learned kd-trees ---------------------------------------------------------------------
def prim_bounds_of(prims, verts):
    """Per-primitive bounds (Triangle::Bounds / BilinearPatch::Bounds: min / max over the vertices)."""
    prims = np.asarray(prims)
    # triangles, alpha-tested triangles and triangles with an image-textured alpha: v[3] is no vertex index there (the
    # bits of an alpha, a texture number) and is not followed
    is_tri = np.isin(prims["kind"], (0, 4, 5, 6, 7, 16, 17, 18, 19))
    v = np.asarray(verts, np.float32)[np.where(is_tri[:, None], prims["v"][:, [0, 1, 2, 0]], prims["v"])]
    tri = is_tri[:, None, None]
    lo = np.where(tri, v[:, :3].min(1, keepdims=True), v.min(1, keepdims=True))[:, 0]
    hi = np.where(tri, v[:, :3].max(1, keepdims=True), v.max(1, keepdims=True))[:, 0]
    return lo.astype(np.float32), hi.astype(np.float32)


def kd_from_planes(planes, prims, verts, scale=None, translate=0.0):
    """KdTreeNode array from an nss plane array.

    `planes` is what kdTree.exportTree_structure / getPlaneArray write (machine_learning/
    nss_kd_tree.py:204-216, 239-240; np.savez key 'b'): float32 [n, 5] in LEVEL order, level l holding
    2**l rows, row = (one-hot split axis x y z, unused, offset - pc_translation) in the NORMALISED
    point-cloud frame.  scale / translate map a normalised offset back to scene space: split =
    offset * scale[axis] + translate[axis] (None: the scene's bounding box, i.e. the
    getAABBox / applyNormalization frame of nss_common).  A row whose axis is all-zero ends the tree on
    that branch (leaf).  Primitives are distributed as KdTreeAggregate::buildTree does (a primitive
    overlapping the plane goes to both sides: below if its min <= split... see classify below), and the
    nodes are laid out in the reference's order (below child at index + 1), so the result feeds
    nnbvh_kd_scene_create.  The nss exporter has no counterpart for leaves; the last plane level's
    children are leaves holding the primitives that reach them.

    Parity: unpinned — the reference ships no exported tree; tests/test_kdtree.py holds a
    synthetic known answer."""
    planes = np.asarray(planes, np.float32).reshape(-1, 5)
    prims = np.ascontiguousarray(prims, PRIM_DTYPE)
    lo, hi = prim_bounds_of(prims, verts)
    bmin, bmax = lo.min(0), hi.max(0)
    if scale is None:
        scale = (bmax - bmin).astype(np.float32)
        translate = bmin.astype(np.float32)
    scale = np.broadcast_to(np.asarray(scale, np.float32), (3,))
    translate = np.broadcast_to(np.asarray(translate, np.float32), (3,))
    n_levels = int(np.log2(len(planes) + 1))
    if 2 ** n_levels - 1 != len(planes):
        raise ValueError("plane array must hold a complete level-order tree (2**levels - 1 rows)")
    nodes, indices = [], []

    def emit(level, slot, ids):
        me = len(nodes)
        nodes.append([0, 0])
        row = planes[2 ** level - 1 + slot] if level < n_levels else None
        axis = -1 if row is None or not row[:3].any() else int(np.argmax(row[:3]))
        if axis < 0 or len(ids) == 0:
            n = len(ids)
            if n == 1:
                nodes[me] = [int(ids[0]), 3 | (1 << 2)]
            else:
                nodes[me] = [len(indices) if n else 0, 3 | (n << 2)]
                indices.extend(int(i) for i in ids)
            return
        split = np.float32(row[4] * scale[axis] + translate[axis])
        # buildTree's classification at an edge t = split (aggregates.cpp:954-960): below gets every
        # primitive that starts before the split plane, above every primitive that ends after it;
        # a primitive lying IN the plane (min == max == split) goes below
        below = ids[(lo[ids, axis] < split) | ((lo[ids, axis] == split) & (hi[ids, axis] == split))]
        above = ids[hi[ids, axis] > split]
        emit(level + 1, 2 * slot, below)
        nodes[me] = [int(split.view(np.uint32)), axis | (len(nodes) << 2)]
        emit(level + 1, 2 * slot + 1, above)

    emit(0, 0, np.arange(len(prims)))
    out = np.zeros(len(nodes), KD_NODE_DTYPE)
    out["split_or_index"] = np.array([n[0] for n in nodes], np.int64).astype(np.uint32)
    out["flags"] = np.array([n[1] for n in nodes], np.uint32)
    bounds = np.concatenate([bmin, bmax]).astype(np.float32)
    depth = n_levels
    return KdBuilt(out, np.array(indices, np.int32), bounds, depth)
