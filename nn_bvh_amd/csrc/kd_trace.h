// kd_trace.h — what the wavefront queue calls (capi_wavefront.cpp) need of a kd-tree scene: the scene object, its
// per-stream workspaces and the batch-mode launcher of kd_trace.hip.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <map>
#include <mutex>

#include "../../include/nnbvh.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kKdMaxBatches = 4;   // batches one batch-mode launch may cover
constexpr int kKdIndexBits = 28;   // a lane's ray tag = batch << 28 | index: batches below 2^28 rays

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
    int fits32 = 0;  // nodes (8 B), primitive records (64 B) and indices (4 B) each below 4 GiB
    int n_nodes = 0, n_indices = 0, n_prims = 0;  // what nnbvh_kd_scene_info / _read report (d_indices holds max(n_indices, 1))
    float bounds[6];
    uint2 *d_nodes = nullptr;
    int32_t *d_indices = nullptr;
    float4 *d_prims = nullptr;
    float4 *d_extras = nullptr;  // 6 slots per primitive, scenes with attribute-reading alpha kinds only
    // closest, any, batches of records, batches of SOA slices, batches with host candidates, then the walk instances:
    // shadow-tr lean / full, one-random lean / full
    int blocks_per_cu[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // tuning (speed only, never results; nnbvh_kd_scene_set_option "read_soa" / "pair_one_launch"; DESIGN.md §5.7
    // holds the measurement behind the defaults)
    // both 0 until a recorded probe run shows the new form ahead by more than the spread of either form
    int read_soa = 0;         // 1: lean scenes, the kernel reads a queue's SOA slices itself (0: gather + records)
    int pair_one_launch = 0;  // 1: closest_and_shadow as ONE batch-mode launch over both queues (0: the two calls)
    std::mutex mu;
    std::map<hipStream_t, nnbvh::KdWorkspace> workspaces;
};

namespace nnbvh {

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
// slot 0..KdWorkspace::kWalk-1 of the workspace's walk arrays, grown to `bytes`
bool kd_walk_scratch(KdWorkspace *w, int slot, size_t bytes, void **out);

}  // namespace nnbvh
