// bvh_trace.h — launch interface between the C ABI (bvh_capi.cpp) and the kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nnbvh.h"
#include "nnbvh_internal.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kBlockThreads = 256;   // 4 wavefronts
constexpr int kMaxQueues = 8;        // one ray queue per XCD
constexpr int kQueueStrideWords = 32;  // each queue head on its own 128-B line
constexpr int kMaxFusedBatches = 4;    // batches one mode-3 launch may cover
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
};

hipError_t launch_zero_queue(unsigned *queue, int words, hipStream_t stream);
// ... and the same for a per-ray int32 array (candidate counts, `before`): a kernel node, not a memset
hipError_t launch_zero_words(int32_t *words, long n, int maxBlocks, hipStream_t stream);

// occupancy != nullptr: do not launch, report resident blocks per CU of that kernel instance
// patches: bit 0 = the scene holds bilinear patches (0: kernel instances without the parked ray direction),
// bit 1 = it holds alpha-tested triangles (the ALPHA = 1 kernel instances), bit 2 = alpha-tested bilinear patches
// too (the ALPHA = 2 instances), bit 3 = triangles with an image-textured alpha (the ALPHA = 3 instances: flat scenes,
// window 8)
hipError_t launch_trace(int mode, const TraceParams &p, int window, int instanced, int patches, int blocks,
                        hipStream_t stream, int *occupancy);

// The walk instances (modes 4 / 5 of the kernel, always at window 8: `stack_window` is a speed-only option and is
// ignored here).  kind 1: IntersectShadowTr's walk, 2: IntersectOneRandom's.  form 0: lean (FULL = false; neither scene
// nor mesh holds patches, no instance table, no host-only primitives, fits32), 1: general (FULL = true), 2: static
// two-level scene (FULL = true).  occupancy as for launch_trace.
hipError_t launch_trace_walk(int kind, int form, const TraceParams &p, int blocks, hipStream_t stream, int *occupancy);

}  // namespace nnbvh
