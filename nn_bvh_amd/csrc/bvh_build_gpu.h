// bvh_build_gpu.h — interface between the host code of the C ABI (bvh_build.cpp, bvh_capi.cpp, capi_two_level.cpp)
// and the device builders (bvh_build_gpu.hip) and the device baker of every BVH scene (bvh_bake.hip).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/nnbvh.h"

namespace nnbvh {

// Upper levels of an HLBVH (buildUpperSAH, cpu/aggregates.cpp:626-723) over treelet roots given
// by bounds (6 floats each) and subtree node counts, laid out in flattenBVH's DFS order
// (aggregates.cpp:505-522): where every treelet's nodes start, how deep its root sits, and the
// upper interior nodes themselves.
struct UpperLayout {
    std::vector<int> base;    // [nTreelets] flat index of the treelet's root
    std::vector<int> depth;   // [nTreelets] depth of the treelet's root
    std::vector<int> upper_index;                 // flat indices of the upper interior nodes
    std::vector<nnbvh_linear_node> upper_nodes;   // ... and their contents
    int total_nodes = 0;
};
bool hlbvh_upper_layout(const float *treelet_bounds, const int *treelet_sizes, int n_treelets,
                        UpperLayout *out, std::string *error);
// The words for a treelet table the device's upper build refused (bvh_build_gpu.hip, step 8b): the host's checks of the
// table in the host's order, then hlbvh_upper_layout, whose first failure in its left-first recursion is the message.
// false: the host builder refuses nothing here.
bool hlbvh_upper_refusal(const float *treelet_bounds, const int *treelet_sizes, int n_treelets, std::string *text);

struct GpuBuildResult {
    std::vector<nnbvh_linear_node> nodes;
    std::vector<nnbvh_prim> ordered;
    int depth = 0;
    // milliseconds: host->device copies, device pipeline up to the treelet table, device upper trees,
    // device emit, device->host copies
    double ms[5] = {0, 0, 0, 0, 0};
    int n_treelets = 0, n_unique_codes = 0;
    int n_upper = 0, n_upper_passes = 0;  // as ForestBuildResult's
    // keep_on_device (in): do not download; hand the device arrays to the caller instead (who frees
    // them with hipFree): LinearBVHNode[total_nodes], leaf-ordered nnbvh_prim[n_prims], float3 verts
    bool keep_on_device = false;
    void *d_nodes = nullptr, *d_ordered = nullptr, *d_verts = nullptr;
    int total_nodes = 0;
};
// prim_bounds may be NULL when every primitive is a triangle or a bilinear patch.
bool gpu_hlbvh(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
               const float *prim_bounds, int max_prims_in_node, int device, GpuBuildResult *out,
               std::string *error);

// A SAH node none of whose 11 split costs is below +inf (count * surface area overflows for every split): the
// reference's minCostSplitBucket stays -1 there (aggregates.cpp:343-353), its std::partition puts nothing on the
// left and buildRecursive recurses on the same range for ever.  The host and the device builder evaluate the same
// floats, refuse the same nodes and say so in the same words.
constexpr const char *kSahCostsErrorText =
    "nnbvh_build_create: coordinates too large for the SAH costs (count * surface area is not finite for any "
    "split; the reference does not terminate on this input)";

// SAH (buildRecursive's default branch) on the device; same tree and leaf order as the host builder.
// ms: upload, big nodes breadth-first, subtrees (one wavefront each), layout + bounds, download;
// n_treelets = subtrees built by wavefronts, n_unique_codes = nodes built breadth-first.
bool gpu_sah(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts, const float *prim_bounds,
             int max_prims_in_node, int device, GpuBuildResult *out, std::string *error);

// Device memory handed from one build to the next: a block a build gives back serves the next request it is
// large enough for (the smallest such block), so a sequence of builds on ONE stream allocates for its largest
// member only.  clear() frees everything.
struct ScratchPool {
    struct Block {
        void *p;
        size_t bytes;
        bool used;
    };
    std::vector<Block> blocks;
    void *take(size_t bytes);  // null: hipMalloc failed
    void give(void *p);
    void clear();
    ~ScratchPool() { clear(); }
};

// The builders' cores: input that is already on the device (the current one), output left there.  gpu_hlbvh /
// gpu_sah are an upload (and, without keep_on_device, a download) around them.  out: d_nodes, d_ordered,
// total_nodes, depth, ms[1..3] and the counts.
struct DeviceBuildInput {
    const nnbvh_prim *d_prims = nullptr;
    int n_prims = 0;
    const float *d_verts = nullptr;
    int n_verts = 0;
    const float *d_prim_bounds = nullptr;  // 6 floats per primitive, or null (as prim_bounds above)
    int max_prims_in_node = 4;
    void *stream = nullptr;  // hipStream_t (this header is also read by host-only builds)
    ScratchPool *pool = nullptr;               // nullable: scratch comes from and goes back to it
    nnbvh_linear_node *d_nodes_out = nullptr;  // nullable: room for 2 * n_prims - 1 nodes; else hipMalloc'ed, the caller's
    nnbvh_prim *d_ordered_out = nullptr;       // nullable: room for n_prims primitives; else likewise
};
bool gpu_hlbvh_device(const DeviceBuildInput &in, GpuBuildResult *out, std::string *error);
bool gpu_sah_device(const DeviceBuildInput &in, GpuBuildResult *out, std::string *error);

// SAH trees of many objects in ONE pass (gpu_sah_device is its one-object case).  in.d_prims holds the objects'
// primitives one after another, object k at [object_first[k], object_first[k + 1]) (host array, object_first[0] = 0,
// strictly increasing, object_first[n_objects] = in.n_prims); in.d_prim_bounds is indexed like in.d_prims.  Every tree is
// byte for byte gpu_sah_device's of that object alone: its second-child offsets count from its own root, its leaves'
// first primitives from the object's first primitive.  in.d_nodes_out, when given, has room for
// 2 * n_prims - n_objects nodes.  A malformed input fails with the message a loop of gpu_sah_device calls over the
// objects would have stopped at: the lowest-numbered failing object's.
struct ForestBuildResult {
    void *d_nodes = nullptr, *d_ordered = nullptr;  // [tree 0, tree 1, ...]; object k's primitives at object_first[k]
    int total_nodes = 0;
    std::vector<int> node_first;  // [n_objects + 1] tree k is d_nodes[node_first[k] .. node_first[k + 1])
    std::vector<int> depth;       // [n_objects]
    double ms[5] = {0, 0, 0, 0, 0};  // as gpu_sah's ([0] and [4] are the wrappers')
    int n_levels = 0;                // breadth-first passes run (each works on every object's big nodes of one level)
    int n_subtrees = 0, n_upper = 0;  // subtrees built by wavefronts, nodes built breadth-first
    int n_upper_passes = 0;           // HLBVH only: launches of the upper build's pass kernel (0: no object has two treelets)
    int n_codes = 0;                  // HLBVH only: distinct (object, Morton code) keys in the forest
};
bool gpu_sah_forest_device(const DeviceBuildInput &in, const int *object_first, int n_objects, ForestBuildResult *out,
                           std::string *error);
// The same for HLBVH trees (gpu_hlbvh_device is its one-object case): tree k is byte for byte that of object k alone,
// from a fixed number of launches and synchronisations whatever n_objects is (one radix sort over the key
// (object << 30) | Morton code, 64 bits wide, or the 32-bit code alone when n_objects is 1) plus the passes of the upper
// SAH, which runs on the device over one table of every object's treelets: one pass when no object has more than 64
// treelets, a few more for larger ones.  No tree data visits the host.  Of the result, ms has the meaning of
// gpu_hlbvh's ([1] device pipeline up to the treelet table, [2] device upper trees, [3] device emit), n_levels = 0,
// n_subtrees = treelets in the forest, n_upper = upper nodes, n_upper_passes = those passes, n_codes = distinct keys.  A malformed input fails with the message a loop of
// gpu_hlbvh_device calls over the objects would have stopped at; an object with several kinds of fault reports the
// first of: vertex index, missing bounds, non-finite, unknown kind, leaf size, treelet checks.
bool gpu_hlbvh_forest_device(const DeviceBuildInput &in, const int *object_first, int n_objects, ForestBuildResult *out,
                             std::string *error);

// The baking of every BVH scene (bvh_bake.hip): the 64-B "both children" records and the 16-B-slot primitive
// stream from a device-resident tree, the device builders' output or the caller's validated tree uploaded by
// bvh_capi.cpp.  Every primitive kind; instance entries with an InstanceBake (two-level scenes).
struct BakedScene {
    void *d_wide = nullptr, *d_prims = nullptr;  // float4 arrays, owned by the caller afterwards
    int n_interior = 0;
    long n_slots = 0;
    int root_ref = 0;
    float bounds[6] = {0, 0, 0, 0, 0, 0};
    int has_host_prims = 0;
    int has_patches = 0;
    int has_alpha = 0;
};
// d_normals: per-vertex shading normals (3 floats, indexed like the vertices) or null; read for
// NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH primitives only
// instances: null refuses NNBVH_PRIM_INSTANCE entries (flat scenes); else the instance-aware form for two-level
// scenes, d_nodes = [top tree, child trees] in one numbering.  stream: a hipStream_t, null = the default stream.
struct InstanceBake {
    const nnbvh_placement *d_placements = nullptr;  // v[0] of an instance entry indexes this (the caller has checked it)
    const int *d_object_root = nullptr;             // [n_objects] node index of each object's root (placement.object indexes it)
    const unsigned char *d_animated = nullptr;      // nullable, [n_placements]: 1 = kPrimAnimated
    // [n_nodes]: 1 = a node of an object no placement names.  Only the trees that placements name are validated and
    // walked, so only their leaves mark a last primitive; such an object is baked, and never reached
    const unsigned char *d_node_unnamed = nullptr;
};
bool bake_on_device(const void *d_nodes, int n_nodes, const void *d_ordered_prims, int n_prims, const void *d_verts,
                    int device, BakedScene *out, std::string *error, const void *d_normals = nullptr,
                    const void *d_prim_alpha = nullptr, const void *d_uvs = nullptr,
                    const InstanceBake *instances = nullptr, void *stream = nullptr);

// Two-level scenes on the device (bvh_bake.hip).  instance_bounds: d_bounds[6 i .. 6 i + 5] of every top-level entry i
// that is an instance of a static placement becomes Transform::operator()(Bounds3f) of its child's root box
// (d_child_nodes[d_child_base[object]]).  rebase_children: the child trees copied behind the n_top_nodes nodes of
// d_nodes_out with their offsets moved into the scene's numbering; d_object_root[k] = n_top_nodes + d_child_base[k];
// d_node_unnamed[i] (one per node of d_nodes_out) = 1 for the nodes of objects with d_object_named[k] == 0.
bool instance_bounds_on_device(const void *d_top_prims, int n_top, const nnbvh_placement *d_placements,
                               const unsigned char *d_animated, const void *d_child_nodes, const int *d_child_base,
                               float *d_bounds, void *stream, std::string *error);
bool rebase_children_on_device(const void *d_child_nodes, int n_child_nodes, const int *d_child_base,
                               const int *d_object_first, int n_objects, int n_top_nodes, void *d_nodes_out,
                               int *d_object_root, const unsigned char *d_object_named, unsigned char *d_node_unnamed,
                               void *stream, std::string *error);

// d_ordered: leaf-ordered nnbvh_prim[n_prims] of a build that ran with ids = positions in the caller's array;
// gathers prim_alpha into that order (*d_alpha_out, hipMalloc'ed, the caller's to free) and restores caller_ids
bool gather_prim_alpha_on_device(void *d_ordered, int n_prims, const float *prim_alpha, const int32_t *caller_ids,
                                 void **d_alpha_out, std::string *error);

}  // namespace nnbvh
