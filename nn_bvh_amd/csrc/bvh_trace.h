// bvh_trace.h — launch interface between the C ABI of BVH scenes (capi_trace.cpp, capi_wavefront.cpp) and the kernels
// of bvh_trace.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nnbvh.h"
#include "nnbvh_internal.h"
#include "trace_instance.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kBlockThreads = 256;   // 4 wavefronts (the two lean one-launch instances: trace_block_threads)
constexpr int kMaxQueues = 8;        // one ray queue per XCD
constexpr int kQueueStrideWords = 32;  // each queue head on its own 128-B line
constexpr int kMaxFusedBatches = 4;    // batches one mode-3 launch may cover
constexpr int kSchedStatWords = 20;   // NNBVH_STATS builds: counters per scene (nnbvh_scene_sched_stats)
constexpr int kFusedIndexBits = 28;    // a lane's ray tag = batch << 28 | index: batches below 2^28 rays

struct TraceParams {
    const float4 *wide;   // interior records, 4 x float4 each
    const float4 *prims;  // prim stream, 16-B slots
    float rootMin[3], rootMax[3];
    int rootRef;
    const nnbvh_ray *rays;
    nnbvh_hit *hits;        // MODE 0
    uint8_t *occluded;      // MODE 1/2
    int32_t *visitedOut;    // MODE 1, nullable
    int32_t *testsOut;      // MODE 1, nullable
    long n;
    const int32_t *nDev;    // nullable: device-resident batch size, clamped to [0, n]
    unsigned *queue;        // nQueues heads, kQueueStrideWords apart, zeroed before launch
    int nQueues;
    int primWeight;         // scheduling weight of a lane waiting on a primitive (interior = 16)
    int refillWeight;       // scheduling weight of an idle lane (interior = 16)
    int hasHostPrims;       // scene contains NNBVH_PRIM_HOST primitives
    int intRepeat;          // interior steps per scheduling decision (>= 1)
    int primRepeat;         // primitive steps per scheduling decision (>= 1)
    int fits32;             // wide[] and prims[] are both below 4 GiB: the lean instances' 32-bit offsets reach them
    unsigned long long *stats;  // NNBVH_STATS builds: trips/lanes per step kind; else unused
    uint2 *spill;           // [kMaxStack][grid threads] overflow of the LDS stack window
    const float *anim;      // two-level scenes: kAnimStride floats per instance (anim_math.h), or null
    // mode 3 (one launch over several batches, closest-hit and occlusion-only any-hit mixed): batch
    // b's rays / results / size, queue heads at queue[(b * nQueues + q) * kQueueStrideWords]; bit b
    // of anyMask = batch b is any-hit (bOut = uint8 occluded[]), else closest (bOut = nnbvh_hit[])
    int nBatches;
    unsigned anyMask;
    const nnbvh_ray *bRays[kMaxFusedBatches];
    void *bOut[kMaxFusedBatches];
    long bN[kMaxFusedBatches];
    const int32_t *bNDev[kMaxFusedBatches];  // nullable: device-resident size of batch b, clamped to [0, bN[b]]
    // rays == nullptr (bRays[b] == nullptr): the batch is a wavefront queue, read as the SOA<Ray> slices it is
    // (tmax == nullptr: Infinity, time == nullptr: 0) — no gather pass into nnbvh_ray records
    nnbvh_ray_soa soa;
    nnbvh_ray_soa bSoa[kMaxFusedBatches];
    // candidate mode (hcCap > 0: the HOSTC instances of modes 0 / 2, scenes with host-only primitives): the host-only
    // primitives a ray meets are listed instead of voiding its record (nnbvh_host_candidates, include/nnbvh.h)
    int hcCap;              // K, list entries per ray; 0 = off
    int32_t *hcCount;       // [n]: 0..K; -1 more than K; -2 an alpha re-trace voided the ray
    int32_t *hcBefore;      // [n], mode 0: candidates met before the device hit that stands (zeroed before launch)
    int32_t *hcPrim;        // [n * K]: nnbvh_prim.id of each candidate, traversal order
    int32_t *hcInst;        // [n * K]: 0 = top level, k + 1 = inside instance k
    // ... of mode 3 (its HOSTC instances; hcCap > 0 only selects them): the same five per batch, picked by the lane's
    // batch tag.  bHcCap[b] == 0: batch b is a plain batch, a host-only primitive voids its ray as in the plain instances
    int bHcCap[kMaxFusedBatches];
    int32_t *bHcCount[kMaxFusedBatches];
    int32_t *bHcBefore[kMaxFusedBatches];  // closest batches only
    int32_t *bHcPrim[kMaxFusedBatches];
    int32_t *bHcInst[kMaxFusedBatches];
    // walk mode (the WALK instances, modes 4 / 5), appended again so that the fields above keep their
    // kernel-argument offsets: the shading mesh the hit's pi / n come from and the per-item arrays of the walk
    // (walk_math.h).  The batch is rays / n / nDev; a lane's ray index is its work item
    ShadingMeshDevice wMesh;
    WalkParams walk;
    // image-textured alpha (the ALPHA = 3 instances), appended for the same reason: the scene's descriptor table (three
    // 16-B slots per texture, AlphaTexDesc of alpha_texture_math.h) and its texel pool
    const float4 *alphaTex;
    const float *alphaTexels;
    // the scene's top table (top_table.h; the lean mode-3 instances copy it into LDS), appended likewise: nTop records
    // of four float4 each, at most kTopRecords.  With nTop > 0 rootRef is the tagged root, kTopTag | 0
    const float4 *top;
    int nTop;
    int topBurst;  // tagged interior lanes that make the wave take a table step (1..64; above 64: never)
};

hipError_t launch_zero_queue(unsigned *queue, int words, hipStream_t stream);
// ... and the same for a per-ray int32 array (candidate counts, `before`): a kernel node, not a memset
hipError_t launch_zero_words(int32_t *words, long n, int maxBlocks, hipStream_t stream);

// Threads per block of the instance `is`: kBlockThreads but for the two lean one-launch instances, whose larger blocks
// share one LDS top table among more waves (bvh_trace.hip block_threads).  Grid sizes on the host side (grid_blocks,
// the `blocks_per_cu` option, max_grid_threads) stay in units of kBlockThreads lanes; run_instance converts.
int trace_block_threads(const TraceInstance &is);

// One launch of the instance `is` (trace_instance.h; hipErrorInvalidValue for one the library does not hold) on
// `blocks` blocks of trace_block_threads(is) threads.
// occupancy != nullptr: do not launch, report resident blocks per CU of that instance.
hipError_t launch_trace(const TraceInstance &is, const TraceParams &p, int blocks, hipStream_t stream, int *occupancy);
// The launch ledger (nnbvh_instance_launches, family 0): how often launch_trace has enqueued each instance in this
// process (occupancy queries do not count).  Up to `capacity` rows: desc gets the 7 ints of each TraceInstance, counts
// its count; either may be null.  reset: the counts are zeroed after they are read.  Returns the number of instances.
// Host code only; no device is touched.
int trace_instance_launches(int32_t *desc, uint64_t *counts, int capacity, int reset);

// Tests only (nnbvh_debug_top_table of bvh_capi.cpp): the prologue of the lean one-launch instances alone.  Every one
// of `blocks` blocks copies the table it built in LDS to out + block * top_debug_capacity() records and its record
// count to nOut[block].
int top_debug_capacity();
hipError_t launch_top_table_debug(const float4 *top, int nTop, const float4 *wide, int blocks, float4 *out, int *nOut,
                                  hipStream_t stream);

}  // namespace nnbvh
