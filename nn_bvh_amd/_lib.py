"""ctypes binding of libnnbvh_hip.so (include/nnbvh.h).  Loading fails loudly: there is no
Python or CPU fallback for the traversal path."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NNBVH_LIB selects a diagnostic build (e.g. libnnbvh_hip_stats.so); default is the product
LIB_PATH = os.path.join(_HERE, os.environ.get("NNBVH_LIB", "libnnbvh_hip.so"))

# numpy views of the wire structs (byte-identical to include/nnbvh.h)
NODE_DTYPE = np.dtype([("pmin", "<f4", 3), ("pmax", "<f4", 3), ("offset", "<i4"),
                       ("nprims", "<u2"), ("axis", "u1"), ("pad", "u1")])
PRIM_DTYPE = np.dtype([("kind", "<i4"), ("id", "<i4"), ("v", "<i4", 4)])
RAY_DTYPE = np.dtype([("o", "<f4", 3), ("tmax", "<f4"), ("d", "<f4", 3), ("time", "<f4")])
INSTANCE_DTYPE = np.dtype([("render_from_prim", "<f4", 12), ("prim_from_render", "<f4", 12),
                           ("root", "<i4"), ("n_nodes", "<i4")])
PLACEMENT_DTYPE = np.dtype([("render_from_prim", "<f4", 12), ("prim_from_render", "<f4", 12),
                            ("object", "<i4"), ("pad", "<i4")])
ANIMATED_DTYPE = np.dtype([("start_from", "<f4", 16), ("start_inv", "<f4", 16), ("end_from", "<f4", 16),
                           ("end_inv", "<f4", 16), ("T", "<f4", (2, 3)), ("R", "<f4", (2, 4)), ("S", "<f4", (2, 16)),
                           ("start_time", "<f4"), ("end_time", "<f4"), ("actually_animated", "<i4"), ("pad", "<i4")])
BATCH_DTYPE = np.dtype([("kind", "<i4"), ("pad", "<i4"), ("d_rays", "<u8"), ("n", "<i8"),
                        ("d_out", "<u8"), ("d_nodes_visited", "<u8"), ("d_prim_tests", "<u8")])
HIT_DTYPE = np.dtype([("prim", "<i4"), ("t", "<f4"), ("b0", "<f4"), ("b1", "<f4"), ("b2", "<f4"),
                      ("nodes_visited", "<i4"), ("prim_tests", "<i4"), ("instance", "<i4")])
KD_NODE_DTYPE = np.dtype([("split_or_index", "<u4"), ("flags", "<u4")])
RAY_SOA_DTYPE = np.dtype([(k, "<u8") for k in ("ox", "oy", "oz", "dx", "dy", "dz", "time", "tmax",
                                                "has_medium")])
WORK_QUEUE_DTYPE = np.dtype([("items", "<u8"), ("size", "<u8"), ("capacity", "<i4"), ("pad", "<i4")])
CLOSEST_QUEUES = ("escaped", "hit_area_light", "basic_eval_material", "universal_eval_material",
                  "medium_sample", "next_ray")
CLOSEST_QUEUES_DTYPE = np.dtype([(k, WORK_QUEUE_DTYPE) for k in CLOSEST_QUEUES])
CLASS_BASIC, CLASS_UNIVERSAL, CLASS_INTERFACE, CLASS_AREA_LIGHT = 0, 1, 2, 4
INTERACTION_DTYPE = np.dtype([("pi_lo", "<f4", 3), ("pi_hi", "<f4", 3), ("uv", "<f4", 2), ("wo", "<f4", 3),
                              ("time", "<f4"), ("n", "<f4", 3), ("face_index", "<i4"), ("dpdu", "<f4", 3),
                              ("dpdv", "<f4", 3), ("ns", "<f4", 3), ("dpdus", "<f4", 3), ("dpdvs", "<f4", 3),
                              ("dndus", "<f4", 3), ("dndvs", "<f4", 3), ("dndu", "<f4", 3), ("dndv", "<f4", 3),
                              ("pad0", "<f4"), ("prim", "<i4"), ("status", "<i4"), ("pad1", "<i4", 2)])
TRI_FLIP_NORMAL, TRI_HAS_UV, TRI_HAS_N, TRI_HAS_S = 1, 2, 4, 8
# nnbvh_item_slices: one device pointer per slice (0 = not wanted), field name -> number of components
ITEM_FIELDS = {"prim": 1, "pi": 6, "p": 3, "n": 3, "ns": 3, "dpdu": 3, "dpdv": 3, "dpdus": 3, "dpdvs": 3,
               "dndus": 3, "dndvs": 3, "wo": 3, "uv": 2, "face_index": 1, "time": 1, "t_max": 1, "ray_o": 3,
               "ray_d": 3}
ITEM_SLICES_DTYPE = np.dtype([(k, "<u8") if c == 1 else (k, "<u8", c) for k, c in ITEM_FIELDS.items()])
ITEM_QUEUES = ("hit_area_light", "basic_eval_material", "universal_eval_material", "medium_sample", "next_ray")
CLOSEST_ITEMS_DTYPE = np.dtype([(k, ITEM_SLICES_DTYPE) for k in ITEM_QUEUES] + [("needs_host", WORK_QUEUE_DTYPE)])
# the fields each queue's Push stores (wavefront/intersect.h): any other slice is an NNBVH_ERR_ARG
_MATERIAL_FIELDS = ("prim", "pi", "n", "ns", "dpdu", "dpdv", "dpdus", "dpdvs", "dndus", "dndvs", "wo", "uv",
                    "face_index", "time")
ITEM_QUEUE_FIELDS = {"hit_area_light": ("prim", "p", "n", "uv", "wo"),
                     "basic_eval_material": _MATERIAL_FIELDS, "universal_eval_material": _MATERIAL_FIELDS,
                     "medium_sample": _MATERIAL_FIELDS + ("t_max",),
                     "next_ray": ("prim", "ray_o", "ray_d", "time")}
assert INTERACTION_DTYPE.itemsize == 192
assert NODE_DTYPE.itemsize == 32 and PRIM_DTYPE.itemsize == 24
assert RAY_SOA_DTYPE.itemsize == 72 and CLOSEST_QUEUES_DTYPE.itemsize == 6 * 24
assert RAY_DTYPE.itemsize == 32 and HIT_DTYPE.itemsize == 32
assert ITEM_SLICES_DTYPE.itemsize == 48 * 8 and CLOSEST_ITEMS_DTYPE.itemsize == 5 * 48 * 8 + 24

EXPORTS = [
    "nnbvh_last_error", "nnbvh_device_count", "nnbvh_build_create", "nnbvh_build_nodes",
    "nnbvh_build_ordered_prims", "nnbvh_build_depth", "nnbvh_build_destroy",
    "nnbvh_scene_create", "nnbvh_scene_create_with_normals", "nnbvh_scene_create_with_attributes", "nnbvh_scene_create_gpu_build_with_attributes", "nnbvh_scene_create_instanced_with_attributes", "nnbvh_scene_destroy", "nnbvh_scene_bounds", "nnbvh_scene_info",
    "nnbvh_intersect_closest", "nnbvh_intersect_any", "nnbvh_intersect_closest_device",
    "nnbvh_intersect_any_device", "nnbvh_scene_set_option", "nnbvh_scene_sched_stats",
    "nnbvh_trace_batches_device", "nnbvh_scene_create_instanced", "nnbvh_transform_bounds",
    "nnbvh_build_create_with_bounds", "nnbvh_wavefront_intersect_closest",
    "nnbvh_wavefront_intersect_shadow", "nnbvh_wavefront_intersect_closest_and_shadow", "nnbvh_build_create_gpu", "nnbvh_build_gpu_timing",
    "nnbvh_shading_mesh_create", "nnbvh_shading_mesh_destroy", "nnbvh_triangle_interactions_device",
    "nnbvh_triangle_interactions", "nnbvh_scene_create_gpu_build",
    "nnbvh_shading_mesh_set_instances", "nnbvh_shading_mesh_set_instances_animated", "nnbvh_host_register",
    "nnbvh_host_unregister", "nnbvh_wavefront_record_shadow_device",
    "nnbvh_film_create", "nnbvh_film_destroy", "nnbvh_film_clear", "nnbvh_film_add_samples_device",
    "nnbvh_film_pixels_device", "nnbvh_film_read", "nnbvh_film_pack_pixels_device",
    "nnbvh_film_unpack_pixels_device", "nnbvh_kd_build_create", "nnbvh_kd_build_create_gpu",
    "nnbvh_kd_build_create_stable", "nnbvh_kd_build_timing", "nnbvh_kd_build_nodes",
    "nnbvh_kd_build_prim_indices", "nnbvh_kd_build_bounds", "nnbvh_kd_build_depth", "nnbvh_kd_build_destroy",
    "nnbvh_kd_scene_create", "nnbvh_kd_scene_create_with_attributes", "nnbvh_kd_scene_destroy", "nnbvh_kd_intersect_closest", "nnbvh_kd_intersect_any",
    "nnbvh_kd_intersect_closest_device", "nnbvh_kd_intersect_any_device",
    "nnbvh_wavefront_intersect_shadow_tr", "nnbvh_wavefront_intersect_one_random",
    "nnbvh_wavefront_intersect_shadow_tr_bounded", "nnbvh_wavefront_intersect_one_random_bounded",
    "nnbvh_kd_wavefront_walk_shadow_tr", "nnbvh_kd_wavefront_walk_one_random",
    "nnbvh_wavefront_walk_shadow_tr", "nnbvh_wavefront_walk_one_random",
    "nnbvh_scene_create_instanced_animated", "nnbvh_wavefront_enqueue_closest_items_device",
    "nnbvh_wavefront_intersect_closest_items", "nnbvh_wavefront_intersect_closest_and_shadow_items",
    "nnbvh_intersect_closest_candidates", "nnbvh_intersect_any_candidates",
    "nnbvh_intersect_closest_candidates_device", "nnbvh_intersect_any_candidates_device",
    "nnbvh_trace_batches_candidates_device", "nnbvh_wavefront_intersect_closest_items_candidates",
    "nnbvh_wavefront_enqueue_closest_items_indexed_device", "nnbvh_wavefront_intersect_shadow_candidates",
    "nnbvh_wavefront_intersect_closest_and_shadow_items_candidates",
    "nnbvh_kd_trace_batches_device", "nnbvh_kd_wavefront_intersect_closest", "nnbvh_kd_wavefront_intersect_shadow",
    "nnbvh_kd_wavefront_intersect_closest_and_shadow", "nnbvh_kd_wavefront_intersect_closest_items",
    "nnbvh_kd_wavefront_intersect_closest_and_shadow_items", "nnbvh_kd_scene_set_option",
    "nnbvh_kd_intersect_closest_candidates", "nnbvh_kd_intersect_any_candidates",
    "nnbvh_kd_intersect_closest_candidates_device", "nnbvh_kd_intersect_any_candidates_device",
    "nnbvh_kd_trace_batches_candidates_device", "nnbvh_kd_wavefront_intersect_closest_items_candidates",
    "nnbvh_kd_wavefront_intersect_shadow_candidates",
    "nnbvh_kd_wavefront_intersect_closest_and_shadow_items_candidates",
    "nnbvh_kd_scene_create_gpu_build", "nnbvh_kd_scene_create_gpu_build_with_attributes", "nnbvh_kd_scene_bounds",
    "nnbvh_kd_scene_info", "nnbvh_kd_scene_read", "nnbvh_scene_create_instanced_gpu_build", "nnbvh_scene_read",
    "nnbvh_build_forest_create_gpu", "nnbvh_forest_nodes", "nnbvh_forest_node_first", "nnbvh_forest_depths",
    "nnbvh_forest_ordered_prims", "nnbvh_forest_gpu_timing", "nnbvh_forest_n_levels", "nnbvh_forest_n_subtrees",
    "nnbvh_forest_destroy", "nnbvh_build_forest_create_gpu_hlbvh",
    "nnbvh_scene_create_with_alpha_textures", "nnbvh_scene_create_gpu_build_with_alpha_textures",
    "nnbvh_kd_scene_create_with_alpha_textures", "nnbvh_kd_scene_create_gpu_build_with_alpha_textures",
    "nnbvh_instance_launches",
    "nnbvh_scene_create_instanced_with_alpha_textures", "nnbvh_scene_create_instanced_gpu_build_with_alpha_textures",
    "nnbvh_tree_quality_create",
    "nnbvh_forest_n_upper", "nnbvh_forest_n_upper_passes", "nnbvh_build_n_upper", "nnbvh_build_n_upper_passes",
]


class HostCandidates(ctypes.Structure):
    """nnbvh_host_candidates (include/nnbvh.h): host or device pointers, as the entry point expects."""
    _fields_ = [("capacity", ctypes.c_int32), ("count", ctypes.c_void_p), ("before", ctypes.c_void_p),
                ("prim", ctypes.c_void_p), ("instance", ctypes.c_void_p)]


assert ctypes.sizeof(HostCandidates) == 40


class TreeQuality(ctypes.Structure):
    """nnbvh_tree_quality (include/nnbvh.h): the fork's SAH and EPO of a baked tree and the sums behind them."""
    _fields_ = [("sah", ctypes.c_double), ("epo", ctypes.c_double), ("inner_area", ctypes.c_double),
                ("leaf_area_weighted", ctypes.c_double), ("root_area", ctypes.c_double),
                ("prim_area", ctypes.c_double), ("ext_area_inner", ctypes.c_double),
                ("ext_area_leaf", ctypes.c_double), ("ext_pairs_inner", ctypes.c_int64),
                ("ext_pairs_leaf", ctypes.c_int64), ("n_inner", ctypes.c_int32), ("n_leaves", ctypes.c_int32),
                ("depth", ctypes.c_int32), ("pad", ctypes.c_int32), ("gpu_ms", ctypes.c_float * 4)]


assert ctypes.sizeof(TreeQuality) == 112

WRAP_MODES = {"repeat": 0, "clamp": 1, "black": 2}


class AlphaTexture(ctypes.Structure):
    """nnbvh_alpha_texture (include/nnbvh.h): one FloatImageTexture as the alpha test of a GeometricPrimitive sees
    it — level 0 of the image (float32 [height, width], row 0 = the image's first row, already decoded to linear), the
    wrap mode, the filter, the UVMapping, scale and invert.  Primitive kinds 16 .. 19 name one by v[3]."""
    _fields_ = [("texels", ctypes.c_void_p), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("wrap", ctypes.c_int32), ("point_filter", ctypes.c_int32), ("su", ctypes.c_float),
                ("sv", ctypes.c_float), ("du", ctypes.c_float), ("dv", ctypes.c_float), ("scale", ctypes.c_float),
                ("invert", ctypes.c_int32)]

    def __init__(self, texels, wrap="repeat", point_filter=False, su=1.0, sv=1.0, du=0.0, dv=0.0, scale=1.0,
                 invert=False):
        self.image = np.ascontiguousarray(texels, np.float32)  # kept alive with the descriptor
        if self.image.ndim != 2:
            raise NNBVHError(f"AlphaTexture: texels must be [height, width], not {self.image.shape}")
        super().__init__(self.image.ctypes.data if self.image.size else None, self.image.shape[1], self.image.shape[0],
                         WRAP_MODES[wrap] if isinstance(wrap, str) else int(wrap), int(bool(point_filter)), su, sv,
                         du, dv, scale, int(bool(invert)))


assert ctypes.sizeof(AlphaTexture) == 48


def alpha_texture_table(alpha_textures):
    """(ctypes array or None, count) of a sequence of AlphaTexture"""
    textures = list(alpha_textures)
    if not all(isinstance(t, AlphaTexture) for t in textures):
        raise NNBVHError("alpha_textures: a sequence of nn_bvh_amd.AlphaTexture")
    return ((AlphaTexture * len(textures))(*textures) if textures else None), len(textures)


_lib = None


class NNBVHError(RuntimeError):
    pass


def lib():
    """The loaded shared library (built by nn_bvh_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NNBVHError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(the traversal path has no fallback)")
    # A process must hold ONE HIP runtime.  PyTorch (used for device buffers by the callers of the
    # *_device entry points) ships its own libamdhip64; if this library pulled in the system copy
    # first, torch.cuda would later find no device.  Loading torch first makes both share torch's.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    L.nnbvh_last_error.restype = ctypes.c_char_p
    L.nnbvh_device_count.restype = i32
    L.nnbvh_build_create.restype = vp
    L.nnbvh_build_create.argtypes = [vp, i32, vp, i32, i32, i32]
    L.nnbvh_build_nodes.restype = vp
    L.nnbvh_build_nodes.argtypes = [vp, ctypes.POINTER(i32)]
    L.nnbvh_build_ordered_prims.restype = vp
    L.nnbvh_build_ordered_prims.argtypes = [vp, ctypes.POINTER(i32)]
    L.nnbvh_build_depth.restype = i32
    L.nnbvh_build_depth.argtypes = [vp]
    for fn in (L.nnbvh_build_n_upper, L.nnbvh_build_n_upper_passes, L.nnbvh_forest_n_upper, L.nnbvh_forest_n_upper_passes):
        fn.restype = i32
        fn.argtypes = [vp]
    L.nnbvh_build_destroy.restype = None
    L.nnbvh_build_destroy.argtypes = [vp]
    L.nnbvh_scene_create.restype = vp
    L.nnbvh_scene_create.argtypes = [vp, i32, vp, i32, vp, i32, i32]
    L.nnbvh_scene_create_with_normals.restype = vp
    L.nnbvh_scene_create_with_normals.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32]
    L.nnbvh_scene_create_instanced_with_attributes.restype = vp
    L.nnbvh_scene_create_instanced_with_attributes.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32]
    L.nnbvh_scene_create_with_attributes.restype = vp
    L.nnbvh_scene_create_with_attributes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32]
    L.nnbvh_scene_destroy.restype = None
    L.nnbvh_scene_destroy.argtypes = [vp]
    L.nnbvh_scene_bounds.restype = i32
    L.nnbvh_scene_bounds.argtypes = [vp, vp]
    L.nnbvh_scene_info.restype = i32
    L.nnbvh_scene_info.argtypes = [vp, vp]
    L.nnbvh_intersect_closest.restype = i32
    L.nnbvh_intersect_closest.argtypes = [vp, vp, i64, vp]
    L.nnbvh_intersect_any.restype = i32
    L.nnbvh_intersect_any.argtypes = [vp, vp, i64, vp, vp, vp]
    L.nnbvh_intersect_closest_device.restype = i32
    L.nnbvh_intersect_closest_device.argtypes = [vp, vp, i64, vp, vp]
    L.nnbvh_intersect_any_device.restype = i32
    L.nnbvh_intersect_any_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.nnbvh_scene_set_option.restype = i32
    L.nnbvh_scene_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    L.nnbvh_scene_create_instanced.restype = vp
    L.nnbvh_scene_create_instanced.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, i32]
    L.nnbvh_scene_create_instanced_animated.restype = vp
    L.nnbvh_scene_create_instanced_animated.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, i32, vp, i32]
    L.nnbvh_transform_bounds.restype = None
    L.nnbvh_transform_bounds.argtypes = [vp, vp, vp]
    L.nnbvh_build_create_with_bounds.restype = vp
    L.nnbvh_build_create_with_bounds.argtypes = [vp, i32, vp, i32, vp, i32, i32]
    L.nnbvh_trace_batches_device.restype = i32
    L.nnbvh_trace_batches_device.argtypes = [vp, vp, i32, vp]
    L.nnbvh_scene_create_gpu_build.restype = vp
    L.nnbvh_scene_create_gpu_build.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32]
    L.nnbvh_scene_create_gpu_build_with_attributes.restype = vp
    L.nnbvh_scene_create_gpu_build_with_attributes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, i32]
    L.nnbvh_scene_create_with_alpha_textures.restype = vp
    L.nnbvh_scene_create_with_alpha_textures.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, vp, i32]
    L.nnbvh_scene_create_gpu_build_with_alpha_textures.restype = vp
    L.nnbvh_scene_create_gpu_build_with_alpha_textures.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, i32]
    L.nnbvh_build_create_gpu.restype = vp
    L.nnbvh_build_create_gpu.argtypes = [vp, i32, vp, i32, vp, i32, i32, i32]
    L.nnbvh_build_gpu_timing.restype = i32
    L.nnbvh_build_gpu_timing.argtypes = [vp, vp]
    L.nnbvh_shading_mesh_create.restype = vp
    L.nnbvh_shading_mesh_create.argtypes = [vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, i32]
    L.nnbvh_shading_mesh_set_instances.restype = i32
    L.nnbvh_shading_mesh_set_instances.argtypes = [vp, vp, i32]
    L.nnbvh_host_register.restype = i32
    L.nnbvh_host_register.argtypes = [vp, ctypes.c_size_t]
    L.nnbvh_host_unregister.restype = i32
    L.nnbvh_host_unregister.argtypes = [vp]
    L.nnbvh_shading_mesh_set_instances_animated.restype = i32
    L.nnbvh_shading_mesh_set_instances_animated.argtypes = [vp, vp, vp, i32]
    L.nnbvh_shading_mesh_destroy.restype = None
    L.nnbvh_shading_mesh_destroy.argtypes = [vp]
    L.nnbvh_triangle_interactions.restype = i32
    L.nnbvh_triangle_interactions.argtypes = [vp, vp, vp, i32, vp]
    L.nnbvh_triangle_interactions_device.restype = i32
    L.nnbvh_triangle_interactions_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp]
    L.nnbvh_wavefront_intersect_closest.restype = i32
    L.nnbvh_wavefront_intersect_closest.argtypes = [vp, i32, vp, vp, vp, i64, vp, vp, vp]
    L.nnbvh_wavefront_intersect_shadow.restype = i32
    L.nnbvh_wavefront_intersect_shadow.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.nnbvh_wavefront_intersect_closest_and_shadow.restype = i32
    L.nnbvh_wavefront_intersect_closest_and_shadow.argtypes = [vp, i32, vp, vp, vp, i64, vp, vp,
                                                               i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, vp]
    L.nnbvh_wavefront_enqueue_closest_items_device.restype = i32
    L.nnbvh_wavefront_enqueue_closest_items_device.argtypes = [vp, i32, vp, vp, vp, vp, i64, vp, vp, vp]
    L.nnbvh_wavefront_intersect_closest_items.restype = i32
    L.nnbvh_wavefront_intersect_closest_items.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp]
    L.nnbvh_wavefront_intersect_closest_and_shadow_items.restype = i32
    L.nnbvh_wavefront_intersect_closest_and_shadow_items.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, i32, vp,
                                                                     vp, vp, vp, vp, vp, vp, i64, vp, vp]
    # kd-tree scenes: the BVH calls' argument lists behind a nnbvh_kd_scene *
    L.nnbvh_kd_scene_set_option.restype = i32
    L.nnbvh_kd_scene_set_option.argtypes = [vp, ctypes.c_char_p, i32]
    L.nnbvh_kd_trace_batches_device.restype = i32
    L.nnbvh_kd_trace_batches_device.argtypes = L.nnbvh_trace_batches_device.argtypes
    for name in ("intersect_closest", "intersect_shadow", "intersect_closest_and_shadow", "intersect_closest_items",
                 "intersect_closest_and_shadow_items"):
        kd = getattr(L, "nnbvh_kd_wavefront_" + name)
        kd.restype = i32
        kd.argtypes = getattr(L, "nnbvh_wavefront_" + name).argtypes
    L.nnbvh_wavefront_record_shadow_device.restype = i32
    L.nnbvh_wavefront_record_shadow_device.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i64, i32, vp]
    L.nnbvh_film_create.restype = vp
    L.nnbvh_film_create.argtypes = [i32, i32, i32, i32, ctypes.c_float, i32]
    L.nnbvh_film_destroy.restype = None
    L.nnbvh_film_destroy.argtypes = [vp]
    L.nnbvh_film_clear.restype = i32
    L.nnbvh_film_clear.argtypes = [vp, vp]
    L.nnbvh_film_add_samples_device.restype = i32
    L.nnbvh_film_add_samples_device.argtypes = [vp, vp, vp, vp, i32, vp, i32, i32, vp, vp]
    L.nnbvh_film_pixels_device.restype = i32
    L.nnbvh_film_pixels_device.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(i64)]
    L.nnbvh_film_read.restype = i32
    L.nnbvh_film_read.argtypes = [vp, vp]
    L.nnbvh_film_pack_pixels_device.restype = i32
    L.nnbvh_film_pack_pixels_device.argtypes = [vp, vp, i64, vp, vp]
    L.nnbvh_film_unpack_pixels_device.restype = i32
    L.nnbvh_film_unpack_pixels_device.argtypes = [vp, vp, i64, vp, vp]
    L.nnbvh_kd_build_create.restype = vp
    L.nnbvh_kd_build_create.argtypes = [vp, i32, vp, i32, vp, i32, i32, ctypes.c_float, i32, i32]
    L.nnbvh_kd_build_create_stable.restype = vp
    L.nnbvh_kd_build_create_stable.argtypes = [vp, i32, vp, i32, vp, i32, i32, ctypes.c_float, i32, i32]
    L.nnbvh_kd_build_create_gpu.restype = vp
    L.nnbvh_kd_build_create_gpu.argtypes = [vp, i32, vp, i32, vp, i32, i32, ctypes.c_float, i32, i32, i32]
    L.nnbvh_kd_build_timing.argtypes = [vp, vp]
    L.nnbvh_kd_build_nodes.restype = vp
    L.nnbvh_kd_build_nodes.argtypes = [vp, ctypes.POINTER(i32)]
    L.nnbvh_kd_build_prim_indices.restype = vp
    L.nnbvh_kd_build_prim_indices.argtypes = [vp, ctypes.POINTER(i32)]
    L.nnbvh_kd_build_bounds.restype = i32
    L.nnbvh_kd_build_bounds.argtypes = [vp, vp]
    L.nnbvh_kd_build_depth.restype = i32
    L.nnbvh_kd_build_depth.argtypes = [vp]
    L.nnbvh_kd_build_destroy.restype = None
    L.nnbvh_kd_build_destroy.argtypes = [vp]
    L.nnbvh_kd_scene_create.restype = vp
    L.nnbvh_kd_scene_create.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp, i32]
    L.nnbvh_kd_scene_create_with_attributes.restype = vp
    L.nnbvh_kd_scene_create_with_attributes.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, i32]
    L.nnbvh_kd_scene_create_gpu_build.restype = vp
    L.nnbvh_kd_scene_create_gpu_build.argtypes = [vp, i32, vp, i32, vp, i32, i32, ctypes.c_float, i32, i32, i32]
    L.nnbvh_kd_scene_create_gpu_build_with_attributes.restype = vp
    L.nnbvh_kd_scene_create_gpu_build_with_attributes.argtypes = [vp, i32, vp, i32, vp, vp, vp, vp, i32, i32,
                                                                  ctypes.c_float, i32, i32, i32]
    # ... and with the alpha-texture table of the kinds 16 .. 19 behind the same arguments
    L.nnbvh_kd_scene_create_with_alpha_textures.restype = vp
    L.nnbvh_kd_scene_create_with_alpha_textures.argtypes = (
        list(L.nnbvh_kd_scene_create_with_attributes.argtypes) + [vp, i32])
    L.nnbvh_kd_scene_create_gpu_build_with_alpha_textures.restype = vp
    L.nnbvh_kd_scene_create_gpu_build_with_alpha_textures.argtypes = (
        list(L.nnbvh_kd_scene_create_gpu_build_with_attributes.argtypes) + [vp, i32])
    L.nnbvh_kd_scene_bounds.restype = i32
    L.nnbvh_kd_scene_bounds.argtypes = [vp, vp]
    L.nnbvh_kd_scene_info.restype = i32
    L.nnbvh_kd_scene_info.argtypes = [vp, vp]
    L.nnbvh_scene_create_instanced_gpu_build.restype = vp
    L.nnbvh_scene_create_instanced_gpu_build.argtypes = [vp, i32, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, i32, vp,
                                                         i32, i32, i32]
    L.nnbvh_scene_read.restype = i32
    L.nnbvh_scene_read.argtypes = [vp, i32, vp, ctypes.c_size_t]
    # ... and the two-level calls with the alpha-texture table behind the same arguments
    L.nnbvh_scene_create_instanced_with_alpha_textures.restype = vp
    L.nnbvh_scene_create_instanced_with_alpha_textures.argtypes = (
        list(L.nnbvh_scene_create_instanced_with_attributes.argtypes) + [vp, i32])
    L.nnbvh_scene_create_instanced_gpu_build_with_alpha_textures.restype = vp
    L.nnbvh_scene_create_instanced_gpu_build_with_alpha_textures.argtypes = (
        list(L.nnbvh_scene_create_instanced_gpu_build.argtypes) + [vp, i32])
    L.nnbvh_build_forest_create_gpu.restype = vp
    L.nnbvh_build_forest_create_gpu.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i32, i32]
    L.nnbvh_build_forest_create_gpu_hlbvh.restype = vp
    L.nnbvh_build_forest_create_gpu_hlbvh.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, i32]
    for name in ("nodes", "node_first", "depths", "ordered_prims"):
        getattr(L, "nnbvh_forest_" + name).restype = vp
        getattr(L, "nnbvh_forest_" + name).argtypes = [vp, vp]
    L.nnbvh_forest_gpu_timing.restype = i32
    L.nnbvh_forest_gpu_timing.argtypes = [vp, vp]
    L.nnbvh_forest_n_levels.restype = i32
    L.nnbvh_forest_n_levels.argtypes = [vp]
    L.nnbvh_forest_n_subtrees.restype = i32
    L.nnbvh_forest_n_subtrees.argtypes = [vp]
    L.nnbvh_forest_destroy.restype = None
    L.nnbvh_forest_destroy.argtypes = [vp]
    L.nnbvh_kd_scene_read.restype = i32
    L.nnbvh_kd_scene_read.argtypes = [vp, i32, vp, ctypes.c_size_t]
    L.nnbvh_kd_scene_destroy.restype = None
    L.nnbvh_kd_scene_destroy.argtypes = [vp]
    L.nnbvh_kd_intersect_closest.restype = i32
    L.nnbvh_kd_intersect_closest.argtypes = [vp, vp, i64, vp]
    L.nnbvh_kd_intersect_any.restype = i32
    L.nnbvh_kd_intersect_any.argtypes = [vp, vp, i64, vp, vp, vp]
    L.nnbvh_kd_intersect_closest_device.restype = i32
    L.nnbvh_kd_intersect_closest_device.argtypes = [vp, vp, i64, vp, vp]
    L.nnbvh_kd_intersect_any_device.restype = i32
    L.nnbvh_kd_intersect_any_device.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    L.nnbvh_wavefront_intersect_shadow_tr.restype = i32
    L.nnbvh_wavefront_intersect_shadow_tr.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp]
    L.nnbvh_wavefront_intersect_one_random.restype = i32
    L.nnbvh_wavefront_intersect_one_random.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp, vp]
    L.nnbvh_wavefront_intersect_shadow_tr_bounded.restype = i32
    L.nnbvh_wavefront_intersect_shadow_tr_bounded.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, vp, i64, vp,
                                                              i32, vp, vp]
    L.nnbvh_wavefront_intersect_one_random_bounded.restype = i32
    L.nnbvh_wavefront_intersect_one_random_bounded.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i64, vp, vp, vp, vp,
                                                               i32, vp, vp]
    # the walk calls of a kd scene: the bounded calls' argument lists, max_surfaces for max_passes
    L.nnbvh_kd_wavefront_walk_shadow_tr.restype = i32
    L.nnbvh_kd_wavefront_walk_shadow_tr.argtypes = list(L.nnbvh_wavefront_intersect_shadow_tr_bounded.argtypes)
    L.nnbvh_kd_wavefront_walk_one_random.restype = i32
    L.nnbvh_kd_wavefront_walk_one_random.argtypes = list(L.nnbvh_wavefront_intersect_one_random_bounded.argtypes)
    L.nnbvh_wavefront_walk_shadow_tr.restype = i32
    L.nnbvh_wavefront_walk_shadow_tr.argtypes = list(L.nnbvh_wavefront_intersect_shadow_tr_bounded.argtypes)
    L.nnbvh_wavefront_walk_one_random.restype = i32
    L.nnbvh_wavefront_walk_one_random.argtypes = list(L.nnbvh_wavefront_intersect_one_random_bounded.argtypes)
    hc = ctypes.POINTER(HostCandidates)
    L.nnbvh_intersect_closest_candidates.restype = i32
    L.nnbvh_intersect_closest_candidates.argtypes = [vp, vp, i64, vp, hc]
    L.nnbvh_intersect_any_candidates.restype = i32
    L.nnbvh_intersect_any_candidates.argtypes = [vp, vp, i64, vp, hc]
    L.nnbvh_intersect_closest_candidates_device.restype = i32
    L.nnbvh_intersect_closest_candidates_device.argtypes = [vp, vp, i64, vp, hc, vp]
    L.nnbvh_intersect_any_candidates_device.restype = i32
    L.nnbvh_intersect_any_candidates_device.argtypes = [vp, vp, i64, vp, hc, vp]
    L.nnbvh_trace_batches_candidates_device.restype = i32
    L.nnbvh_trace_batches_candidates_device.argtypes = [vp, vp, i32, hc, vp]
    L.nnbvh_wavefront_intersect_closest_items_candidates.restype = i32
    L.nnbvh_wavefront_intersect_closest_items_candidates.argtypes = [vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, hc, vp]
    L.nnbvh_wavefront_enqueue_closest_items_indexed_device.restype = i32
    L.nnbvh_wavefront_enqueue_closest_items_indexed_device.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, i64, vp, vp, vp]
    L.nnbvh_wavefront_intersect_shadow_candidates.restype = i32
    L.nnbvh_wavefront_intersect_shadow_candidates.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, hc, vp]
    L.nnbvh_wavefront_intersect_closest_and_shadow_items_candidates.restype = i32
    L.nnbvh_wavefront_intersect_closest_and_shadow_items_candidates.argtypes = [
        vp, vp, i32, vp, vp, vp, i64, vp, vp, vp, hc, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, hc, vp]
    # ... and their kd forms
    for name in ("intersect_closest_candidates", "intersect_any_candidates", "intersect_closest_candidates_device",
                 "intersect_any_candidates_device", "trace_batches_candidates_device",
                 "wavefront_intersect_closest_items_candidates", "wavefront_intersect_shadow_candidates",
                 "wavefront_intersect_closest_and_shadow_items_candidates"):
        kd = getattr(L, "nnbvh_kd_" + name)
        kd.restype = i32
        kd.argtypes = getattr(L, "nnbvh_" + name).argtypes
    L.nnbvh_scene_sched_stats.restype = i32
    L.nnbvh_scene_sched_stats.argtypes = [vp, vp, i32]
    L.nnbvh_instance_launches.restype = i32
    L.nnbvh_instance_launches.argtypes = [i32, vp, vp, i32, i32]
    L.nnbvh_tree_quality_create.restype = i32
    L.nnbvh_tree_quality_create.argtypes = [vp, i32, vp, i32, vp, i32, ctypes.c_double, ctypes.c_double, i32,
                                            ctypes.POINTER(TreeQuality), vp, vp, vp]
    _lib = L
    return L


FAMILY_BVH, FAMILY_KD = 0, 1  # nnbvh_instance_launches


def instance_launches(family, reset=False):
    """The launch ledger of one kernel family -> {instance tuple: launches so far in this process}.  family FAMILY_BVH:
    (mode, window, inst, patch, alpha, soa, hostc) of trace_kernel; FAMILY_KD: (mode, patch, o32, attr, hostc) of
    kd_trace_kernel.  Needs no device."""
    L = lib()
    n = L.nnbvh_instance_launches(family, None, None, 0, 0)
    if n < 0:
        raise NNBVHError(f"nnbvh_instance_launches failed (status {-n}): {last_error()}")
    desc, counts = np.zeros((n, 7), np.int32), np.zeros(n, np.uint64)
    L.nnbvh_instance_launches(family, ptr(desc), ptr(counts), n, int(bool(reset)))
    width = 7 if family == FAMILY_BVH else 5
    return {tuple(int(x) for x in row[:width]): int(c) for row, c in zip(desc, counts)}


class LaunchLedger:
    """`with LaunchLedger(family) as led:` ... led.launched is then {instance tuple: launches made inside the block},
    the instances with none left out."""

    def __init__(self, family):
        self.family = family
        self.launched = {}

    def __enter__(self):
        self._before = instance_launches(self.family)
        return self

    def __exit__(self, *exc):
        after = instance_launches(self.family)
        self.launched = {k: v - self._before[k] for k, v in after.items() if v != self._before[k]}
        return False


def last_error():
    return lib().nnbvh_last_error().decode("utf-8", "replace")


def check(rc, what):
    if rc != 0:
        raise NNBVHError(f"{what} failed (status {rc}): {last_error()}")


def ptr(a):
    return ctypes.c_void_p(a.ctypes.data)
