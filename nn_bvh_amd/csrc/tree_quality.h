// tree_quality.h — launch interface of the SAH / EPO scoring passes over a baked tree (tree_quality.hip,
// DESIGN.md §5.16).  The caller (capi_quality.cpp) has validated the tree on the host: every index the kernels follow is
// in range, the nodes are in depth-first order and no path is longer than kQualityMaxDepth edges.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nnbvh.h"

namespace nnbvh {

constexpr int kQualityMaxDepth = 64;  // edges from the root to the deepest leaf: the end[] chase is at most this long
constexpr int kQualityBlock = 256;    // threads per block of every pass; one block partial per kQualityBlock elements

// scoring record of one node, 32 B: {pmin.xyz, pmax.x} {pmax.y, pmax.z, end, nprims} (the last two as int32 bits);
// end = the first node after the node's subtree in depth-first order
struct QualityBuffers {
    const nnbvh_linear_node *nodes = nullptr;  // [n_nodes]
    const nnbvh_prim *prims = nullptr;         // [n_prims], leaf order
    const float *verts = nullptr;              // [3 * n_verts]
    int n_nodes = 0, n_prims = 0;
    float4 *rec = nullptr;           // [2 * n_nodes]
    int32_t *leaf_of = nullptr;      // [n_prims]: the leaf that holds ordered position j
    int32_t *k_inner = nullptr;      // [n_prims]: inner nodes that hold position j's primitive as an external
    int32_t *k_leaf = nullptr;       // [n_prims]: ... leaves
    int32_t *node_external = nullptr;  // [n_nodes]: externals of node i
    double *partials = nullptr;      // [5 * quality_blocks(max(n_nodes, n_prims))] block partials of the double sums
    long long *ipartials = nullptr;  // [2 * quality_blocks(n_prims)] block partials of the pair counts
    double *sums = nullptr;          // [5]: inner_area, leaf_area_weighted, prim_area, ext_area_inner, ext_area_leaf
    long long *isums = nullptr;      // [2]: ext_pairs_inner, ext_pairs_leaf
};

inline int quality_blocks(int n) { return (n + kQualityBlock - 1) / kQualityBlock; }

// the three phases, each enqueued on `stream`; nothing synchronises
hipError_t launch_quality_prepare(const QualityBuffers &b, hipStream_t stream);  // rec, leaf_of; node_external = 0
hipError_t launch_quality_walk(const QualityBuffers &b, hipStream_t stream);     // k_inner, k_leaf, node_external
hipError_t launch_quality_reduce(const QualityBuffers &b, hipStream_t stream);   // sums, isums

}  // namespace nnbvh
