// kd_trace.h — kd-tree scenes between the kernel (kd_trace.hip), their C ABI (capi_kd.cpp), the wavefront queue calls
// (capi_wavefront.cpp) and the device-side creation (kd_bake.hip): the kernel's arguments and launcher, the scene
// object, its per-stream workspaces and the batch-mode and walk launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <map>
#include <mutex>

#include "../../include/nnbvh.h"
#include "kd_instance.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kKdBlock = 256;
constexpr int kKdW = 8;              // LDS window of the to-visit stack, entries per lane (patch instances)
constexpr int kKdWLean = 4;          // ... of the lean instances: 18 KiB of LDS per block, 8 blocks per CU (measured
                                     // against 8 entries / 5 blocks: crown +8 %, bathroom +11 %)
constexpr int kKdQueues = 8;         // one ray queue per XCD
constexpr int kKdQueueStride = 32;   // words: every queue head on its own 128-B line
constexpr int kKdMaxBatches = 4;   // batches one batch-mode launch may cover
constexpr int kKdIndexBits = 28;   // a lane's ray tag = batch << 28 | index: batches below 2^28 rays

struct KdParams {
    const uint2 *nodes;           // KdTreeNode[], {split | index, flags}
    const int32_t *primIndices;   // KdTreeAggregate::primitiveIndices
    const float4 *prims;          // 4 slots of 16 B per primitive, in the caller's primitive order:
                                  // {p0, id} {p1, flags} {p2, 0} {p3 (patch), 0}
    float bmin[3], bmax[3];       // KdTreeAggregate::bounds
    const nnbvh_ray *rays;
    nnbvh_hit *hits;              // MODE 0
    uint8_t *occluded;            // MODE 1
    int32_t *visitedOut, *testsOut;  // MODE 1, nullable
    long n;
    unsigned *queue;
    int nQueues;
    int primWeight, refillWeight, nodeRepeat;
    int hasHostPrims;
    float4 *spill;                // [kMaxStack][grid threads] overflow of the LDS window
    const float4 *extras;         // ATTR instances: 6 slots per primitive {n0} {n1} {n2} {n3} {uv00, uv10} {uv01, uv11}
                                  // (per-vertex normals / uvs of the alpha-tested kinds that read them), else null
    // batch mode (MODE 2 / 3: one launch over several batches, closest-hit and any-hit mixed).  Appended, so that the
    // fields above keep their kernel-argument offsets.  Batch b's queue heads sit at
    // queue[(b * nQueues + q) * kKdQueueStride]; bit b of anyMask = batch b is any-hit (bOut = uint8 occluded[]),
    // else closest (bOut = nnbvh_hit[])
    int nBatches;
    unsigned anyMask;
    const nnbvh_ray *bRays[kKdMaxBatches];   // MODE 2
    nnbvh_ray_soa bSoa[kKdMaxBatches];       // MODE 3: SOA<Ray> slices (tmax == nullptr: Infinity, time == nullptr: 0)
    void *bOut[kKdMaxBatches];
    int32_t *bVisited[kKdMaxBatches], *bTests[kKdMaxBatches];  // any-hit batches, nullable
    long bN[kKdMaxBatches];
    const int32_t *bNDev[kKdMaxBatches];     // nullable: device-resident size of batch b, clamped to [0, bN[b]]
    // candidate mode (the HOSTC instances of MODE 2, scenes with host-only primitives), appended
    // again: per batch the arrays of its nnbvh_host_candidates.  bHcCap[b] == 0: batch b is a plain batch, a
    // host-only primitive voids its ray as in the plain instances
    int bHcCap[kKdMaxBatches];
    int32_t *bHcCount[kKdMaxBatches];
    int32_t *bHcBefore[kKdMaxBatches];       // closest batches only
    int32_t *bHcPrim[kKdMaxBatches];
    int32_t *bHcInst[kKdMaxBatches];
    // walk mode (the WALK instances), appended again: the shading mesh the hit's pi / n come from and
    // the per-item arrays of the walk (walk_math.h).  One batch; a lane's ray tag is its work item
    MeshView wMesh;
    WalkParams walk;
    // image-textured alpha (the ATTR = 2 instances), appended again: the scene's descriptor table (three 16-B slots per
    // texture, AlphaTexDesc of alpha_texture_math.h) and its texel pool.  A kPrimAlphaTex triangle keeps the texture
    // index in slot 2's w and its (u, v) pairs in slots 4 / 5 of its extras: {u0, v0, u1, v1} {u2, v2, 0, 0}
    const float4 *alphaTex;
    const float *alphaTexels;
};

// One instance of kd_trace_kernel (KdInstance; kKdInstances of kd_instance.h lists those the library holds).
// occupancy != nullptr: do not launch, report resident blocks per CU of that instance.  hipErrorInvalidValue for an
// instance the library does not hold
hipError_t launch_kd_trace(const KdInstance &is, const KdParams &p, int blocks, hipStream_t stream, int *occupancy);
// The launch ledger (nnbvh_instance_launches, family 1): how often launch_kd_trace has enqueued each instance in this
// process (occupancy queries do not count).  Up to `capacity` rows: desc gets 7 ints per instance (the KdInstance, zero-
// padded), counts its count; either may be null.  reset: the counts are zeroed after they are read.  Returns the
// number of instances.  Host code only; no device is touched.
int kd_instance_launches(int32_t *desc, uint64_t *counts, int capacity, int reset);

struct KdWorkspace {
    unsigned *queue = nullptr;  // kKdMaxBatches x kKdQueues heads
    float4 *spill = nullptr;
    void *d_in = nullptr, *d_out = nullptr, *d_aux0 = nullptr, *d_aux1 = nullptr;
    size_t in_bytes = 0, out_bytes = 0, aux_bytes = 0;
    void *d_hits = nullptr;  // hit records of the queue calls made without d_hits
    size_t hits_bytes = 0;
    // grow-only arrays of the walk calls (nnbvh_kd_wavefront_walk_*): ray records and per-item state.  Per stream like
    // the queue heads: the calls are asynchronous on their stream
    static constexpr int kWalk = 6;
    void *walk[kWalk] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    size_t walk_bytes[kWalk] = {0, 0, 0, 0, 0, 0};
};

// One batch of a batch-mode launch: nnbvh_ray records, or with rays == nullptr the SOA<Ray> slices of a wavefront
// queue.  The batch holds min(n, max(*d_n, 0)) rays (d_n nullable).
struct KdBatch {
    int any = 0;                         // 0: closest hit, out = nnbvh_hit[n]; 1: any hit, out = uint8[n]
    const void *rays = nullptr;
    const nnbvh_ray_soa *soa = nullptr;
    int64_t n = 0;
    const int32_t *d_n = nullptr;
    void *out = nullptr;
    void *visited = nullptr, *tests = nullptr;  // any hit, nullable: exact counts
    // nullable; capacity > 0: the batch's host candidates (device pointers, arrays of n entries; the caller has checked
    // them).  count / before are zeroed by kernel nodes ahead of the launch
    const nnbvh_host_candidates *hc = nullptr;
};

}  // namespace nnbvh

struct nnbvh_kd_scene {
    int device = 0;
    int n_cus = 0;
    int depth = 0;
    int has_host_prims = 0;
    int has_patches = 0;
    int fits32 = 0;  // kd_fits32 of the scene's sizes
    int offsets32 = 1;  // option "offsets32" (speed only): 0 = run the O32 = 0 instances although the scene fits
    int n_nodes = 0, n_indices = 0, n_prims = 0;  // what nnbvh_kd_scene_info / _read report (d_indices holds max(n_indices, 1))
    float bounds[6];
    uint2 *d_nodes = nullptr;
    int32_t *d_indices = nullptr;
    float4 *d_prims = nullptr;
    float4 *d_extras = nullptr;  // 6 slots per primitive, scenes with attribute-reading alpha kinds only
    int blocks_per_cu[nnbvh::kKdInstanceCount] = {};  // resident blocks per CU, by row of kKdInstances (0: not asked yet)
    // tuning (speed only, never results; nnbvh_kd_scene_set_option "read_soa" / "pair_one_launch"; DESIGN.md §5.7
    // holds the measurement behind the defaults)
    // both 0 until a recorded probe run shows the new form ahead by more than the spread of either form
    int read_soa = 0;         // 1: lean scenes, the kernel reads a queue's SOA slices itself (0: gather + records)
    int pair_one_launch = 0;  // 1: closest_and_shadow as ONE batch-mode launch over both queues (0: the two calls)
    std::mutex mu;
    std::map<hipStream_t, nnbvh::KdWorkspace> workspaces;
    // image-textured alpha (kinds 16 .. 19): descriptor table (AlphaTexDesc, alpha_texture_math.h) and texel pool, or
    // null: the caller's table, attached whenever one was given.  has_alpha_tex: a kPrimAlphaTex record was baked —
    // such a scene has attribute slots (d_extras), a table and no alpha-tested patch, and runs the ATTR = 2 instances.
    // A scene with a table but no textured triangle runs the instances it would run without the table
    void *d_alpha_tex = nullptr;
    float *d_alpha_texels = nullptr;
    int n_alpha_tex = 0;
    int64_t n_alpha_texels = 0;
    int has_alpha_tex = 0;
};

namespace nnbvh {

// nodes (8 B), primitive records (64 B) and indices (4 B) each below 4 GiB: the O32 instances reach them.
// The O32 = 1 instances form `(unsigned)index * sizeof(element)` and add it to a scalar base, so they are correct as
// long as that product does not wrap: 2^32 / 8 = 2^29 nodes, 2^32 / 4 = 2^30 indices, 2^32 / 64 = 2^26 primitive
// records.  The primitive bound keeps two records of slack below 2^26: a primitive step reads slots 0 .. 3 of a record
// through the one offset, and with the slack the END of the last record (not only its start) stays below 2^32.
// The O32 = 0 instances index with 64-bit arithmetic throughout (`at` widens before it scales; the attribute slots
// are reached through `6 * (long)index`), so they are correct for every count the C ABI can express: n_nodes,
// n_indices and n_prims are `int`, at most 2^31 - 1 each.  (Before the scale moved into `at`, the wide path formed
// 4 * index in int and was wrong from 2^29 primitive records on.)
inline int kd_fits32(int64_t n_nodes, int64_t n_prims, int64_t n_indices) {
    return (n_nodes < (1 << 29) && n_prims < (1 << 26) - 1 && n_indices < (1 << 30)) ? 1 : 0;
}
// what the choice of an instance reads from a scene (the pickers of kd_instance.h)
inline KdTraits kd_scene_traits(const nnbvh_kd_scene *s) {
    return {s->has_patches, s->d_extras != nullptr, s->has_alpha_tex, s->d_alpha_tex != nullptr, s->has_host_prims,
            s->fits32, s->offsets32, s->read_soa};
}

// A new scene object with everything filled in but its device arrays, which either creation route (the caller's tree:
// capi_kd.cpp; the device's own: kd_bake.hip) attaches.
inline nnbvh_kd_scene *kd_new_scene(int device, int n_cus, int depth, bool has_host_prims, bool has_patches, int n_nodes,
                                    int n_indices, int n_prims, const float bounds[6]) {
    auto *s = new nnbvh_kd_scene;
    s->device = device;
    s->n_cus = n_cus;
    s->depth = depth;
    s->has_host_prims = has_host_prims ? 1 : 0;
    s->has_patches = has_patches ? 1 : 0;
    s->n_nodes = n_nodes;
    s->n_indices = n_indices;
    s->n_prims = n_prims;
    s->fits32 = kd_fits32(n_nodes, n_prims, n_indices);
    std::memcpy(s->bounds, bounds, 24);
    return s;
}

// One workspace per stream, as for the BVH scenes.  The caller holds s->mu.
KdWorkspace *kd_workspace_for(nnbvh_kd_scene *s, hipStream_t stream);

// ONE batch-mode launch (behind the one queue-reset node) over 1..kKdMaxBatches batches.  Batches given as SOA
// slices are read by the kernel itself where the scene's instance has a SOA form (lean scenes, every batch of the
// launch SOA); else they are gathered into workspace records first.  Where a batch has host candidates the launch
// runs the kernel's candidate-mode instances (record form only) if the scene holds host-only primitives, else the
// plain ones over the zeroed counts.  The caller has checked the arguments, made the scene's device current and holds
// s->mu.
int kd_launch_batches(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const KdBatch *batches, int n_batches);

// The queue-head reset node and ONE launch of a walk instance.  The caller has checked the arguments
// (a scene without attribute arrays, a mesh without an instance table), made the scene's device current and holds s->mu.
int launch_walk(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const WalkJob &walk);

// The descriptor table and texel pool of a checked alpha-texture table (n_textures > 0) uploaded and attached to a
// scene either creation route has made (capi_kd.cpp).  false: the scene is destroyed, the error text says why.
bool kd_attach_alpha_textures(nnbvh_kd_scene *s, const nnbvh_alpha_texture *textures, int n_textures);
// slot 0..KdWorkspace::kWalk-1 of the workspace's walk arrays, grown to `bytes`
bool kd_walk_scratch(KdWorkspace *w, int slot, size_t bytes, void **out);

}  // namespace nnbvh
