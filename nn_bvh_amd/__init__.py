"""nn_bvh_amd — MI355X-native (gfx950) BVH traversal + ray-primitive intersection for pbrt's
BVHAggregate hot path.  The product is libnnbvh_hip.so behind include/nnbvh.h; this package
is its Python host-side mirror (buffers and launch only) plus input generators."""
from ._lib import (HIT_DTYPE, NODE_DTYPE, PRIM_DTYPE, RAY_DTYPE, AlphaTexture, NNBVHError, lib)  # noqa: F401
from .aggregate import BVHAggregate, build_forest_gpu, build_hlbvh_forest_gpu, build_tree, build_tree_gpu, make_prims, make_rays  # noqa: F401
from .aggregate import candidates_dtype, resolve_host_candidates, resolve_host_candidates_any  # noqa: F401
from .quality import TreeQuality, tree_quality  # noqa: F401
