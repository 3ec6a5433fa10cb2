// kd_trace.hip — KdTreeAggregate::Intersect / IntersectP on gfx950, plus their C ABI.
//
// What is computed (reference: /root/reference/src/pbrt/cpu/aggregates.cpp):
//   closest hit   KdTreeAggregate::Intersect    :973-1067
//   any hit       KdTreeAggregate::IntersectP   :1069-1150
//   root interval Bounds3::IntersectP(o, d, tMax, &t0, &t1)   util/vecmath.h:1547-1571
//   leaves        the same Triangle / BilinearPatch tests as the BVH kernels (trace_math.h)
// Results (hit primitive, t, barycentrics, kdNodesVisited and nTriTests per ray) are bit-identical
// to that code.  HOW it runs is the BVH kernels' scheme: persistent 64-lane
// wavefronts over XCD-aware ray queues, a per-lane state machine whose step kind (node step /
// primitive step / refill) the wave picks from ballots, and the KdNodeToVisit{node, tMin, tMax}
// stack (aggregates.cpp:747-750) as a ring window in LDS that spills its oldest entry to a
// coalesced HBM array.  A node step reads ONE 8-B KdTreeNode; there is no box test below the root
// (a kd-tree clips the ray interval against split planes instead), so node steps are ~4x cheaper
// than a BVH interior step and the kernel is bound by the dependent 8-B loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/nnbvh.h"
#include "nnbvh_internal.h"
#include "trace_math.h"
#include "spawn_math.h"
#include "bvh_trace.h"
#include "kd_trace.h"
#include "wavefront.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kKdBlock = 256;
constexpr int kKdW = 8;              // LDS window of the to-visit stack, entries per lane (patch instances)
constexpr int kKdWLean = 4;          // ... of the lean instances: 18 KiB of LDS per block, 8 blocks per CU (measured
                                     // against 8 entries / 5 blocks: crown +8 %, bathroom +11 %)
constexpr int kKdQueues = 8;         // one ray queue per XCD
constexpr int kKdQueueStride = 32;   // words: every queue head on its own 128-B line
constexpr int kKdDone = -1;          // lane carries no ray
constexpr int kKdLeaf = -2;          // lane is walking the primitives of a leaf

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
};

// A lane takes up the ray {R0, R1} = {o, tMax} {d, time}: the reciprocals (aggregates.cpp:980), the shear, the
// `ray.d[axis] <= 0` bits of aggregates.cpp:1002-1003, cold hit slots, zeroed counts and the root interval (:975-977:
// rays that miss the tree's bounds return before anything is counted).  Used at a refill and, in the walk instances,
// when an item's walk goes on with its spawned ray.  A macro and not a lambda or a function: the refill path of the
// existing instances then compiles to the code it compiled to before the walk instances shared it.
#define KD_BEGIN_RAY(R0, R1)                                                                                          \
    do {                                                                                                              \
        r.o = {(R0).x, (R0).y, (R0).z};                                                                               \
        rayTMax = (R0).w;                                                                                             \
        const V3 dir = {(R1).x, (R1).y, (R1).z};                                                                      \
        if (PATCH) d = dir;                                                                                           \
        r.inv = {1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z};                                                           \
        ray_shear(r, dir);                                                                                            \
        r.kz |= (dir.x <= 0.0f ? 16 : 0) | (dir.y <= 0.0f ? 32 : 0) | (dir.z <= 0.0f ? 64 : 0);                       \
        if constexpr (BATCH) r.kz |= ((p.anyMask >> curBatch) & 1u) ? kAnyLane : 0;                                   \
        if (MODE != 1) {                                                                                              \
            cold[kColdHit][lane] = __int_as_float(-1);                                                                \
            cold[kColdHit + 1][lane] = 0.0f;                                                                          \
            cold[kColdHit + 2][lane] = 0.0f;                                                                          \
            cold[kColdHit + 3][lane] = 0.0f;                                                                          \
        }                                                                                                             \
        if (HOSTC || p.hasHostPrims) cold[kColdHost][lane] = 0.0f;                                                    \
        if constexpr (WALK != 0) {                                                                                    \
            cold[kColdDir][lane] = (R1).x;                                                                            \
            cold[kColdDir + 1][lane] = (R1).y;                                                                        \
            cold[kColdDir + 2][lane] = (R1).z;                                                                        \
            cold[kColdTime][lane] = (R1).w;                                                                           \
            cold[kColdTMax][lane] = (R0).w;                                                                           \
        }                                                                                                             \
        visited = 0;                                                                                                  \
        tests = 0;                                                                                                    \
        found = false;                                                                                                \
        sp = base = 0;                                                                                                \
        cur = kd_root_interval(p.bmin, p.bmax, r.o, r.inv, rayTMax, tMin, tMax) ? 0 : kKdDone;                        \
    } while (0)

// MODE 0: closest hit; MODE 1: any hit (counts written when asked for).
// MODE 2 / 3: batch mode.  One launch drains up to kKdMaxBatches independent batches in list order, each closest-hit
// or any-hit, each with its own eight queue heads and a size that may live on the device (the kernel reads it).  The
// lane's ray tag (cold ray index) carries its batch in the bits above kKdIndexBits; whether the lane's ray is an
// any-hit ray rides as bit 7 of r.kz, and the three places where the two walks differ (the rayTMax < tMin exit, an
// accepted hit, what is retired) are chosen per lane from it.  MODE 2 reads nnbvh_ray records; MODE 3 (lean form
// only) reads every batch as the SOA<Ray> slices of a wavefront queue, its own instance so that the record form does
// not carry the second fetch path.
// PATCH = 0: the scene holds no bilinear patches — nothing reads the ray direction after the ray is
// fetched except `ray.d[axis] <= 0` at interior nodes, which rides as three bits beside the shear's
// kz; the patch test, the largest register consumer, is not compiled in.
// W: entries per lane of the LDS window of the to-visit stack.
// O32: nodes, primitive records and primitiveIndices are each below 4 GiB and are fetched through 32-bit
// byte offsets from a scalar base (no 64-bit shift / add per fetch).
// ATTR = 1 (with PATCH = 1): the scene holds alpha-tested triangles of smooth meshes or alpha-tested bilinear patches,
// whose re-trace reads per-vertex attributes from p.extras (bvh_trace.hip's ALPHA = 1 smooth / ALPHA = 2 code)
// HOSTC = 1 (MODE 2 only, scenes with host-only primitives): candidate mode.  A host-only primitive does not void the
// ray: its id goes to the ray's list (p.bHcPrim / p.bHcInst of the lane's batch at ray * K, traversal order, the count
// in the kColdHost slot) unless it stands there already — a kd-tree holds a primitive in every leaf its box overlaps
// — and the walk goes on as if the primitive were absent.  An accepted closest hit on a lane with candidates stores
// how many came before it (p.bHcBefore).  At retire the count goes to p.bHcCount: 0..K, -1 = more than K (record
// void), -2 = an alpha re-trace voided the ray.  A batch with bHcCap[b] == 0 is a plain batch: its first host-only
// primitive "overflows" a list of none.
// MODE 4 / 5 = MODE 2 with WALK = 1 / 2 (one closest-hit batch, no ATTR, no HOSTC): the walk instances.  A lane does not retire
// its ray when the closest-hit walk is finished: it runs one step of IntersectShadowTr (1) or IntersectOneRandom (2)
// for its work item (walk_math.h: the verdicts and arithmetic of the fused pass steps of wavefront2.hip) and, where
// the item's walk goes on, re-enters the tree with the spawned ray.  Nothing is written to bOut.  PATCH = 1 instances
// compute the interaction with the patch-capable code (FULL), the lean ones with the triangle-only code.
// (WALK rides in MODE — MODE 4 = MODE 2 with WALK 1, MODE 5 = MODE 2 with WALK 2 — and not as a seventh template
// parameter: that would rename every existing instance.)
template <int MODE, int PATCH, int W, int O32, int ATTR = 0, int HOSTC = 0>
__global__ __launch_bounds__(kKdBlock, PATCH ? 1 : 2) void kd_trace_kernel(KdParams p) {
    constexpr int WALK = MODE >= 4 ? MODE - 3 : 0;
    static_assert(!HOSTC || MODE == 2, "candidate mode: the record-reading batch instances only");
    static_assert(!WALK || (!ATTR && !HOSTC), "walk instances: the plain record-reading batch form only");
    auto pick_batch = [](const auto &arr, int b) {  // arr[b] of a kernel-argument array
        return b == 0 ? arr[0] : (b == 1 ? arr[1] : (b == 2 ? arr[2] : arr[3]));
    };
    auto at = [](const auto *base, int index) {  // &base[index]
        using T = decltype(base);
        return O32 ? reinterpret_cast<T>(reinterpret_cast<const char *>(base) + (unsigned)index * (unsigned)sizeof(*base))
                   : base + (long)index;
    };
    // KdNodeToVisit {node, tMin, tMax}: the three words of an entry 64 dwords apart
    __shared__ float s_stack[kKdBlock / 64][W][3][64];
    // cold per-ray state ([field][lane]): ray index, best hit (closest), reached-a-host-primitive flag
    constexpr bool BATCH = MODE >= 2, SOA = MODE == 3;
    static_assert(MODE >= 0 && MODE <= 5 && (!SOA || (!PATCH && !ATTR)), "SOA instances: the lean form only");
    constexpr int kAnyLane = 128;  // BATCH: bit 7 of r.kz
    // WALK: six more slots — the direction, time and tMax of the item's current ray (the step needs them for wo, the
    // selected segment ray and the next ray) and the number of Intersect calls made for the item
    constexpr int kColdRi = 0, kColdHit = 1, kColdHost = (MODE != 1) ? 5 : 1, kColdWalk = kColdHost + 1;
    constexpr int kColdDir = kColdWalk, kColdTime = kColdWalk + 3, kColdTMax = kColdWalk + 4, kColdCalls = kColdWalk + 5;
    constexpr int kColdFields = kColdWalk + (WALK ? 6 : 0);
    __shared__ float s_cold[kKdBlock / 64][kColdFields][64];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * kKdBlock + threadIdx.x;
    float(*stk)[3][64] = s_stack[wave];
    float(*cold)[64] = s_cold[wave];
    cold[kColdRi][lane] = __int_as_float(-1);
    const long spillStride = (long)gridDim.x * kKdBlock;

    int q = 0;
    if (p.nQueues > 1) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        q = (int)(xcc & 0xf) % p.nQueues;
    }
    int queuesTried = 0;
    const long nRays = p.n;
    int curBatch = 0;  // BATCH: the batch this wave draws from

    RayState r;          // o, 1/d, shear; r.kz also carries bit 4 + k = (d[k] <= 0), see the refill
    V3 d = {0, 0, 0};    // PATCH only: the patch test reads the direction
    float rayTMax = 0.0f, tMin = 0.0f, tMax = 0.0f;
    int visited = 0, tests = 0;
    int cur = kKdDone, sp = 0, base = 0;
    // a lane inside a leaf (cur == kKdLeaf): leafIdx = the primitive to test next, leafPos = where the
    // index after it sits in primitiveIndices, leafLeft = primitives still to test including leafIdx
    int leafIdx = 0, leafPos = 0, leafLeft = 0;
    bool found = false, exhausted = false;

    // aggregates.cpp:1053-1060 / :1098-1105: next entry of the to-visit list, or the ray is finished
    auto pop_or_done = [&]() {
        if (sp > 0) {
            --sp;
            float node = stk[sp & (W - 1)][0][lane];
            float a = stk[sp & (W - 1)][1][lane], b = stk[sp & (W - 1)][2][lane];
            asm volatile("" : "+v"(node), "+v"(a), "+v"(b));
            if (sp < base) {  // rare: the entry lives in the HBM spill array
                const float4 e = p.spill[(long)sp * spillStride + gtid];
                base = sp;
                node = e.x;
                a = e.y;
                b = e.z;
                asm volatile("" : "+v"(node), "+v"(a), "+v"(b));
            }
            cur = __float_as_int(node);
            tMin = a;
            tMax = b;
        } else {
            cur = kKdDone;
        }
    };

    for (;;) {
        const bool isNode = cur >= 0;
        const bool isIdle = cur == kKdDone;
        const int nNode = __popcll(__ballot(isNode));
        const unsigned long long idleMask = __ballot(isIdle);
        const int nIdle = __popcll(idleMask);
        const int nPrim = 64 - nNode - nIdle;
        const int sI = nNode * 16, sP = nPrim * p.primWeight;
        const int sR = exhausted ? 0 : nIdle * p.refillWeight;

        if (nIdle == 64 || (sR > sI && sR > sP)) {
            // ---- retire finished rays, refill idle lanes ------------------------------------
            const int ri = isIdle ? __float_as_int(cold[kColdRi][lane]) : -1;
            // WALK: the lane's item walks on from nextO in direction nextD / would start call walk.maxSurfaces + 1
            [[maybe_unused]] bool goOn = false, capped = false;
            [[maybe_unused]] V3 nextO = {0.0f, 0.0f, 0.0f}, nextD = {0.0f, 0.0f, 0.0f};
            [[maybe_unused]] float nextTMax = 1.0f, nextTime = 0.0f;  // aggregate.Intersect(r, 1), time 0: WALK 2
            if (ri >= 0) {
                const bool needHost = p.hasHostPrims && cold[kColdHost][lane] != 0.0f;
                if constexpr (WALK != 0) {
                    // one step of the walk for item ri (the tag of the one batch is the index), on the hit record a
                    // MODE 2 closest lane would retire
                    const float4 r0 = {r.o.x, r.o.y, r.o.z, cold[kColdTMax][lane]};
                    const float4 r1 = {cold[kColdDir][lane], cold[kColdDir + 1][lane], cold[kColdDir + 2][lane],
                                       cold[kColdTime][lane]};
                    const float4 h0 = {cold[kColdHit][lane], rayTMax, cold[kColdHit + 1][lane], cold[kColdHit + 2][lane]};
                    const float4 h1 = {cold[kColdHit + 3][lane], __int_as_float(visited), __int_as_float(tests),
                                       needHost ? __int_as_float(-1) : 0.0f};
                    if constexpr (WALK == 1) {
                        goOn = w2_str_item<PATCH != 0>(p.wMesh, r0, r1, h0, h1, ri, p.walk.primClass, p.walk.nPrimClass,
                                                       p.walk.pLight, p.walk.state, nextO, nextD);
                        nextTMax = r0.w;  // tMax is the work item's, unchanged (intersect.h:175, :187)
                        nextTime = r1.w;
                        // the spawned ray has a zero direction: the walk ends, the ray arrives (state stays 0)
                        if (goOn && nextD.x == 0.0f && nextD.y == 0.0f && nextD.z == 0.0f) goOn = false;
                    } else {
                        goOn = w2_or_item<PATCH != 0>(p.wMesh, r0, r1, h0, h1, ri, p.walk.p1, p.walk.material,
                                                      p.walk.primMaterial, p.walk.nPrimMaterial, p.walk.st,
                                                      p.walk.selHits, p.walk.selRays, nextO, nextD);
                    }
                    if (goOn) {
                        const int calls = __float_as_int(cold[kColdCalls][lane]);
                        if (calls >= p.walk.maxSurfaces) {  // the caller's to finish, as w2_mark_unfinished marks it
                            goOn = false;
                            capped = true;
                            if constexpr (WALK == 1) p.walk.state[ri] = 2;
                            else p.walk.selHits[2 * (long)ri + 1].w = __int_as_float(-1);
                        } else {
                            cold[kColdCalls][lane] = __int_as_float(calls + 1);
                        }
                    }
                } else if constexpr (HOSTC) {
                    // candidate mode, a block of its own so that the plain instances' retire below stays as it is:
                    // the count goes to the batch's array; an any-hit ray is the caller's (2) when it met a host-only
                    // primitive, a closest-hit record is void only for count < 0
                    const int b = ri >> kKdIndexBits;
                    const long idx = ri & ((1 << kKdIndexBits) - 1);
                    void *outp = pick_batch(p.bOut, b);
                    const int c = __float_as_int(cold[kColdHost][lane]);
                    if (pick_batch(p.bHcCap, b) > 0) pick_batch(p.bHcCount, b)[idx] = c;
                    if (r.kz & kAnyLane) {
                        int32_t *vis = pick_batch(p.bVisited, b), *tst = pick_batch(p.bTests, b);
                        reinterpret_cast<uint8_t *>(outp)[idx] = found ? 1 : (c != 0 ? 2 : 0);
                        if (vis) vis[idx] = visited;
                        if (tst) tst[idx] = tests;
                    } else {
                        float4 h0, h1;
                        h0.x = cold[kColdHit][lane];
                        h0.y = rayTMax;
                        h0.z = cold[kColdHit + 1][lane];
                        h0.w = cold[kColdHit + 2][lane];
                        h1.x = cold[kColdHit + 3][lane];
                        h1.y = __int_as_float(visited);
                        h1.z = __int_as_float(tests);
                        h1.w = c < 0 ? __int_as_float(-1) : 0.0f;
                        float4 *out = reinterpret_cast<float4 *>(outp) + 2 * idx;
                        out[0] = h0;
                        out[1] = h1;
                    }
                } else if constexpr (BATCH) {  // the lane's batch has its own arrays
                    const int b = ri >> kKdIndexBits;
                    const long idx = ri & ((1 << kKdIndexBits) - 1);
                    void *outp = b == 0 ? p.bOut[0] : (b == 1 ? p.bOut[1] : (b == 2 ? p.bOut[2] : p.bOut[3]));
                    if (r.kz & kAnyLane) {
                        int32_t *vis = b == 0 ? p.bVisited[0] : (b == 1 ? p.bVisited[1] : (b == 2 ? p.bVisited[2] : p.bVisited[3]));
                        int32_t *tst = b == 0 ? p.bTests[0] : (b == 1 ? p.bTests[1] : (b == 2 ? p.bTests[2] : p.bTests[3]));
                        reinterpret_cast<uint8_t *>(outp)[idx] = found ? 1 : (needHost ? 2 : 0);
                        if (vis) vis[idx] = visited;
                        if (tst) tst[idx] = tests;
                    } else {
                        float4 h0, h1;
                        h0.x = cold[kColdHit][lane];
                        h0.y = rayTMax;
                        h0.z = cold[kColdHit + 1][lane];
                        h0.w = cold[kColdHit + 2][lane];
                        h1.x = cold[kColdHit + 3][lane];
                        h1.y = __int_as_float(visited);
                        h1.z = __int_as_float(tests);
                        h1.w = needHost ? __int_as_float(-1) : 0.0f;
                        float4 *out = reinterpret_cast<float4 *>(outp) + 2 * idx;
                        out[0] = h0;
                        out[1] = h1;
                    }
                } else if (MODE == 0) {
                    float4 h0, h1;
                    h0.x = cold[kColdHit][lane];
                    h0.y = rayTMax;
                    h0.z = cold[kColdHit + 1][lane];
                    h0.w = cold[kColdHit + 2][lane];
                    h1.x = cold[kColdHit + 3][lane];
                    h1.y = __int_as_float(visited);
                    h1.z = __int_as_float(tests);
                    h1.w = needHost ? __int_as_float(-1) : 0.0f;
                    float4 *out = reinterpret_cast<float4 *>(p.hits) + 2 * (long)ri;
                    out[0] = h0;
                    out[1] = h1;
                } else {
                    p.occluded[ri] = found ? 1 : (needHost ? 2 : 0);
                    if (p.visitedOut) p.visitedOut[ri] = visited;
                    if (p.testsOut) p.testsOut[ri] = tests;
                }
            }
            int newRi = -1;
            // the lanes that take a new ray, their number and mask: the idle ones, less (WALK) those that walk on
            bool takes = isIdle;
            unsigned long long takeMask = idleMask;
            int nTake = nIdle;
            if constexpr (WALK != 0) {
                const unsigned long long cm = __ballot(capped);
                if (p.walk.unfinished && cm != 0ull && lane == __ffsll((long long)cm) - 1)
                    atomicAdd(p.walk.unfinished, __popcll(cm));
                if (goOn) {  // same item, same lane: cold[kColdRi] stays
                    const float4 a = {nextO.x, nextO.y, nextO.z, nextTMax}, b = {nextD.x, nextD.y, nextD.z, nextTime};
                    KD_BEGIN_RAY(a, b);
                }
                takes = isIdle && !goOn;
                takeMask = __ballot(takes);
                nTake = __popcll(takeMask);
                if (exhausted) {  // every lane was idle: the wave ends when none of them walks on
                    if (nTake == 64) break;
                    if (takes) cold[kColdRi][lane] = __int_as_float(-1);  // retired: the step must not run on it again
                    continue;
                }
            } else {
                if (exhausted) break;  // only reached with every lane idle
            }
            for (;;) {
                if constexpr (WALK != 0) {
                    if (nTake == 0) break;
                }
                static_assert(kKdQueues == 8, "queue ranges are computed with a shift by 3");
                const int qShift = p.nQueues > 1 ? 3 : 0;  // nQueues is 1 or 8: a shift, not a 64-bit division
                long nQ = nRays;
                if constexpr (BATCH) {
                    nQ = p.bN[curBatch];
                    if (const int32_t *nd = p.bNDev[curBatch]) {  // wavefront queues: the size lives on the device
                        const long v = *nd;
                        nQ = v < 0 ? 0 : (v < nQ ? v : nQ);
                    }
                }
                const long qBegin = (nQ * q) >> qShift, qEnd = (nQ * (q + 1)) >> qShift;
                unsigned got = 0;
                if (lane == 0) got = atomicAdd(&p.queue[((BATCH ? curBatch * p.nQueues : 0) + q) * kKdQueueStride], (unsigned)nTake);
                got = __builtin_amdgcn_readfirstlane(got);
                const long start = qBegin + (long)got;
                if (start < qEnd) {
                    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(takeMask >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((unsigned)takeMask, 0u));
                    if (takes && start + rank < qEnd) newRi = (int)(start + rank);
                    break;
                }
                if (++queuesTried >= p.nQueues) {
                    if constexpr (BATCH) {
                        if (curBatch + 1 < p.nBatches) {  // this batch is handed out (or empty): on to the next
                            ++curBatch;
                            queuesTried = 0;
                            continue;
                        }
                    }
                    exhausted = true;
                    break;
                }
                q = (q + 1 == p.nQueues) ? 0 : q + 1;
            }
            if (takes) cold[kColdRi][lane] = __int_as_float((BATCH && newRi >= 0) ? (newRi | (curBatch << kKdIndexBits)) : newRi);
            if (newRi >= 0) {
                float4 r0, r1;
                if constexpr (SOA) {  // a wavefront queue: SOA<Ray> slices (wavefront/workitems.soa:40-50)
                    const nnbvh_ray_soa &s = p.bSoa[curBatch];
                    r0 = {s.ox[newRi], s.oy[newRi], s.oz[newRi], s.tmax ? s.tmax[newRi] : __builtin_inff()};
                    r1 = {s.dx[newRi], s.dy[newRi], s.dz[newRi], s.time ? s.time[newRi] : 0.0f};
                } else {
                    const float4 *in = reinterpret_cast<const float4 *>(BATCH ? p.bRays[curBatch] : p.rays) + 2 * (long)newRi;
                    r0 = in[0];
                    r1 = in[1];
                }
                if constexpr (WALK != 0) {
                    // `while (ray.d != Vector3f(0, 0, 0))`, intersect.h:183 / aggregate.cpp:100: a zero direction makes
                    // no Intersect call — the item is finished as the init kernel left it, the lane stays idle
                    if (r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f) {
                        cold[kColdRi][lane] = __int_as_float(-1);
                    } else {
                        cold[kColdCalls][lane] = __int_as_float(1);
                        KD_BEGIN_RAY(r0, r1);
                    }
                } else {
                    KD_BEGIN_RAY(r0, r1);
                }
            }
            continue;
        }

        if (sP > sI || nNode == 0) {
            // ---- primitive step: lanes inside a leaf test ONE primitive ------------------------
            if (cur == kKdLeaf) {
                // one trip to memory: the primitive's three slots and — if the leaf goes on — the index of
                // the primitive after it, all issued before anything is looked at
                const float4 *rec = at(p.prims, 4 * leafIdx);
                float4 s0 = rec[0], s1 = rec[1], s2 = rec[2];
                int nextIdx = 0;
                if (leafLeft > 1) nextIdx = *at(p.primIndices, leafPos);
                asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s0.z), "+v"(s0.w), "+v"(s1.x), "+v"(s1.y),
                                  "+v"(s1.z), "+v"(s1.w), "+v"(s2.x), "+v"(s2.y), "+v"(s2.z), "+v"(s2.w), "+v"(nextIdx));
                const unsigned flags = __float_as_uint(s1.w);
                if (flags & kPrimHost) {
                    if constexpr (HOSTC) {
                        // the caller tests this primitive itself: list it (rare path: the entries go straight to
                        // global memory) and walk on as if it were absent
                        const int c = __float_as_int(cold[kColdHost][lane]);
                        if (c >= 0) {  // -1 (overflow) and -2 (alpha re-trace) stay
                            const int tag = __float_as_int(cold[kColdRi][lane]);
                            const int b = tag >> kKdIndexBits;
                            const int cap = pick_batch(p.bHcCap, b);
                            const long first = (long)(tag & ((1 << kKdIndexBits) - 1)) * cap;
                            int32_t *hcPrim = pick_batch(p.bHcPrim, b);
                            const int id = __float_as_int(s0.w);
                            // the repeat rule: the primitive sits in every leaf its box overlaps; only its first
                            // position in traversal order is listed (c <= cap entries of this lane's own)
                            bool listed = false;
                            for (int j = 0; j < c; ++j) listed = listed || hcPrim[first + j] == id;
                            if (!listed) {
                                if (c < cap) {
                                    hcPrim[first + c] = id;
                                    pick_batch(p.bHcInst, b)[first + c] = 0;  // kd scenes have one level
                                }
                                cold[kColdHost][lane] = __int_as_float(c < cap ? c + 1 : -1);
                            }
                        }
                    } else {
                        cold[kColdHost][lane] = 1.0f;
                    }
                } else {
                    tests += 1;
                    bool hit;
                    float x0, x1, x2, th;
                    if (!PATCH || !(flags & kPrimPatch)) {
                        hit = triangle_test(r, rayTMax, (flags & kPrimDegenerate) != 0, {s0.x, s0.y, s0.z},
                                            {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z}, x0, x1, x2, th);
                        if (PATCH && hit && (flags & kPrimAlpha)) {
                            // GeometricPrimitive::Intersect / IntersectP with a constant alpha (cpu/primitive.cpp:
                            // 57-70, 79-81), as in the BVH kernels; scenes with such primitives run the PATCH
                            // instances, which keep the ray direction
                            const float a = s2.w;
                            if (a < 1) {
                                const float u = (a <= 0) ? 1.f : hash_float_6f(r.o, d);
                                if (u > a) {
                                    hit = false;
                                    RayState rn = r;
                                    if (ATTR && (flags & kPrimSmooth)) {  // FaceForward(n, ns): shapes.h:939-951
                                        const float4 *ex = p.extras + 6 * (long)leafIdx;
                                        const float4 m0 = ex[0], m1 = ex[1], m2 = ex[2];
                                        rn.o = alpha_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                                                    x0, x1, x2, (flags & kPrimFlipN) != 0, d, true,
                                                                    {m0.x, m0.y, m0.z}, {m1.x, m1.y, m1.z}, {m2.x, m2.y, m2.z});
                                    } else {
                                        rn.o = alpha_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                                                    x0, x1, x2, (flags & kPrimFlipN) != 0, d);
                                    }
                                    tests += 1;  // Triangle::Intersect counts the re-test too
                                    float y0, y1, y2, tn;
                                    if (triangle_test(rn, rayTMax - th, (flags & kPrimDegenerate) != 0, {s0.x, s0.y, s0.z},
                                                      {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z}, y0, y1, y2, tn))
                                        cold[kColdHost][lane] = HOSTC ? __int_as_float(-2) : 1.0f;  // the ray is the caller's (see bvh_trace.hip)
                                }
                            }
                        }
                    } else {
                        const float4 s3 = rec[3];
                        x2 = 0.0f;
                        if constexpr (ATTR != 0) {
                            // GeometricPrimitive::Intersect around a BilinearPatch: the recursion of cpu/primitive.cpp:
                            // 63-69 followed for up to three re-traces, as in bvh_trace.hip (ALPHA = 2)
                            constexpr int kAlphaPatchDepth = 3;
                            const float a = (flags & kPrimAlpha) ? s2.w : 1.0f;
                            RayState rn = r;
                            float tm = rayTMax, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                            int k = 0;
                            for (;;) {
                                hit = patch_test(rn, d, tm, {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                                 {s3.x, s3.y, s3.z}, x0, x1, th);
                                if (!hit || !(a < 1)) break;
                                const float u = (a <= 0) ? 1.f : hash_float_6f(rn.o, d);
                                if (!(u > a)) break;
                                if (k == kAlphaPatchDepth) {
                                    hit = false;
                                    cold[kColdHost][lane] = HOSTC ? __int_as_float(-2) : 1.0f;
                                    break;
                                }
                                if (k == 0) t0 = th;
                                else if (k == 1) t1 = th;
                                else t2 = th;
                                ++k;
                                rn.o = patch_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                                            {s3.x, s3.y, s3.z}, x0, x1, (flags & kPrimFlipN) != 0, d,
                                                            (flags & kPrimSmooth) != 0, (flags & kPrimUV) != 0,
                                                            p.extras + 6 * (long)leafIdx, 4);
                                tm = tm - th;
                                tests += 1;
                            }
                            if (hit && k > 0) {
                                if (k == 3) th = th + t2;
                                if (k >= 2) th = th + t1;
                                th = th + t0;
                            }
                        } else {
                            hit = patch_test(r, d, rayTMax, {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z},
                                             {s2.x, s2.y, s2.z}, {s3.x, s3.y, s3.z}, x0, x1, th);
                        }
                    }
                    if (hit) {
                        if (MODE == 0 || (BATCH && !(r.kz & kAnyLane))) {
                            cold[kColdHit][lane] = s0.w;
                            cold[kColdHit + 1][lane] = x0;
                            cold[kColdHit + 2][lane] = x1;
                            cold[kColdHit + 3][lane] = x2;
                            rayTMax = th;  // :1035-1036, :1046-1047
                            if constexpr (HOSTC) {  // the candidates met before this hit (the last store wins);
                                                    // c > 0 only in a batch with candidate arrays
                                const int c = __float_as_int(cold[kColdHost][lane]);
                                if (c > 0) {
                                    const int tag = __float_as_int(cold[kColdRi][lane]);
                                    pick_batch(p.bHcBefore, tag >> kKdIndexBits)[tag & ((1 << kKdIndexBits) - 1)] = c;
                                }
                            }
                        } else {
                            found = true;
                        }
                    }
                }
                leafLeft -= 1;
                leafIdx = nextIdx;
                leafPos += 1;
                if ((MODE == 1 || BATCH) && found) cur = kKdDone;  // :1091-1094, :1101-1104 (only any-hit lanes set it)
                else if (leafLeft == 0) pop_or_done();
            }
        } else {
            // ---- node step(s): up to p.nodeRepeat in a row before the next scheduling decision ------
            int rep = 0;
            do {
                if (cur >= 0) {
                    if ((MODE == 0 || (BATCH && !(r.kz & kAnyLane))) && rayTMax < tMin) {  // :989-991 a hit closer than this node: finished
                        cur = kKdDone;
                    } else {
                        visited += 1;
                        const uint2 nd = *at(p.nodes, cur);
                        const unsigned flags = nd.y;
                        if ((flags & 3u) != 3u) {
                            // interior (:993-1023 / :1110-1144)
                            const int axis = (int)(flags & 3u);
                            const float split = __uint_as_float(nd.x);
                            const float oa = axis == 0 ? r.o.x : (axis == 1 ? r.o.y : r.o.z);
                            const float ia = axis == 0 ? r.inv.x : (axis == 1 ? r.inv.y : r.inv.z);
                            const bool dLe0 = ((r.kz >> (4 + axis)) & 1) != 0;  // ray.d[axis] <= 0
                            const float tSplit = (split - oa) * ia;
                            const bool belowFirst = (oa < split) || (oa == split && dLe0);
                            const int above = (int)(flags >> 2);
                            const int firstChild = belowFirst ? cur + 1 : above;
                            const int secondChild = belowFirst ? above : cur + 1;
                            if (tSplit > tMax || tSplit <= 0.0f) {
                                cur = firstChild;
                            } else if (tSplit < tMin) {
                                cur = secondChild;
                            } else {
                                if (sp - base == W) {  // window full: its oldest entry goes to HBM
                                    float4 e;
                                    e.x = stk[base & (W - 1)][0][lane];
                                    e.y = stk[base & (W - 1)][1][lane];
                                    e.z = stk[base & (W - 1)][2][lane];
                                    e.w = 0.0f;
                                    p.spill[(long)base * spillStride + gtid] = e;
                                    ++base;
                                }
                                stk[sp & (W - 1)][0][lane] = __int_as_float(secondChild);
                                stk[sp & (W - 1)][1][lane] = tSplit;
                                stk[sp & (W - 1)][2][lane] = tMax;
                                ++sp;
                                cur = firstChild;
                                tMax = tSplit;
                            }
                        } else {
                            // leaf (:1025-1061 / :1084-1107): one primitive index lives in the node itself,
                            // several sit in primitiveIndices — the first of them is fetched here, so that
                            // every primitive step is ONE trip to memory
                            const int nPrimitives = (int)(flags >> 2);
                            if (nPrimitives == 0) {
                                pop_or_done();
                            } else {
                                leafLeft = nPrimitives;
                                leafPos = (int)nd.x + 1;
                                leafIdx = nPrimitives == 1 ? (int)nd.x : *at(p.primIndices, (int)nd.x);
                                cur = kKdLeaf;
                            }
                        }
                    }
                }
            } while (++rep < p.nodeRepeat && __ballot(cur >= 0) != 0ull);
        }
    }
}

#undef KD_BEGIN_RAY

__global__ void kd_zero_queue_kernel(unsigned *queue, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) queue[i] = 0u;
}

static bool kd_hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

struct KdDeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit KdDeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = kd_hip_ok(hipSetDevice(dev), "hipSetDevice");
    }
    ~KdDeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

static bool kd_grow(void **ptr, size_t *have, size_t need, const char *what) {
    if (*have >= need) return true;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *have = 0;
    if (!kd_hip_ok(hipMalloc(ptr, need), what)) return false;
    *have = need;
    return true;
}

}  // namespace nnbvh

using namespace nnbvh;

KdWorkspace *nnbvh::kd_workspace_for(nnbvh_kd_scene *s, hipStream_t stream) {
    auto it = s->workspaces.find(stream);
    if (it != s->workspaces.end()) return &it->second;
    KdWorkspace w;
    // an entry is spilled only when W newer ones sit above it: levels 0 .. depth - W of a lane's list, at the
    // smallest window any instance runs with
    const size_t spill_levels = (size_t)std::max(s->depth + 1 - std::min(kKdW, kKdWLean), 1);
    const size_t spill_bytes = spill_levels * (size_t)s->n_cus * 8 * kKdBlock * sizeof(float4);
    if (!kd_hip_ok(hipMalloc((void **)&w.queue, kKdMaxBatches * kKdQueues * kKdQueueStride * sizeof(unsigned)), "hipMalloc(queue)"))
        return nullptr;
    if (!kd_hip_ok(hipMalloc((void **)&w.spill, spill_bytes), "hipMalloc(spill)")) {
        (void)hipFree(w.queue);
        return nullptr;
    }
    return &(s->workspaces[stream] = w);
}

static void kd_fill_scene(const nnbvh_kd_scene *s, const KdWorkspace *w, KdParams &p) {
    p.nodes = s->d_nodes;
    p.primIndices = s->d_indices;
    p.prims = s->d_prims;
    std::memcpy(p.bmin, s->bounds, 12);
    std::memcpy(p.bmax, s->bounds + 3, 12);
    p.queue = w->queue;
    p.nQueues = kKdQueues;
    p.primWeight = 12;  // swept on bathroom: 12 / 8 / 4 is the best of 4 x 2 x 3 (+1.5 % over 24 / 8 / 4)
    p.refillWeight = 8;
    p.nodeRepeat = 4;
    p.hasHostPrims = s->has_host_prims;
    p.spill = w->spill;
    p.extras = s->d_extras;
}

// lean scenes (no patches, no attributes): their batch-mode instance has a form that reads SOA slices itself
static bool kd_scene_reads_soa(const nnbvh_kd_scene *s) { return s->read_soa && !s->has_patches && !s->d_extras; }

static int kd_launch(nnbvh_kd_scene *s, int mode, const void *d_rays, int64_t n, void *d_hits, void *d_occ,
                     void *d_vis, void *d_tests, hipStream_t stream, KdWorkspace *w) {
    KdParams p{};
    kd_fill_scene(s, w, p);
    p.rays = (const nnbvh_ray *)d_rays;
    p.hits = (nnbvh_hit *)d_hits;
    p.occluded = (uint8_t *)d_occ;
    p.visitedOut = (int32_t *)d_vis;
    p.testsOut = (int32_t *)d_tests;
    p.n = (long)n;
    // the four instances: closest / any hit x scenes with / without bilinear patches
    void (*const kernels[8])(KdParams) = {
        kd_trace_kernel<0, 0, kKdWLean, 0>, kd_trace_kernel<1, 0, kKdWLean, 0>, kd_trace_kernel<0, 1, kKdW, 0>,
        kd_trace_kernel<1, 1, kKdW, 0>,     kd_trace_kernel<0, 0, kKdWLean, 1>, kd_trace_kernel<1, 0, kKdWLean, 1>,
        kd_trace_kernel<0, 1, kKdW, 1>,     kd_trace_kernel<1, 1, kKdW, 1>};
    // ... and the attribute-reading forms of the PATCH instances
    void (*const attr_kernels[4])(KdParams) = {kd_trace_kernel<0, 1, kKdW, 0, 1>, kd_trace_kernel<1, 1, kKdW, 0, 1>,
                                               kd_trace_kernel<0, 1, kKdW, 1, 1>, kd_trace_kernel<1, 1, kKdW, 1, 1>};
    void (*const kernel)(KdParams) = s->d_extras ? attr_kernels[mode + 2 * s->fits32]
                                                 : kernels[mode + 2 * s->has_patches + 4 * s->fits32];
    if (s->blocks_per_cu[mode] == 0) {
        int occ = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kKdBlock, 0);
        s->blocks_per_cu[mode] = (e == hipSuccess && occ > 0) ? std::min(occ, 8) : 4;
    }
    int blocks = s->n_cus * s->blocks_per_cu[mode];
    const int64_t need = (n + kKdBlock - 1) / kKdBlock;
    if (need < blocks) blocks = (int)std::max<int64_t>(need, 1);
    hipLaunchKernelGGL(kd_zero_queue_kernel, dim3(1), dim3(256), 0, stream, w->queue, kKdQueues * kKdQueueStride);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kKdBlock), 0, stream, p);
    return kd_hip_ok(hipGetLastError(), "kd trace kernel launch") ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

int nnbvh::kd_launch_batches(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const KdBatch *batches, int n_batches) {
    KdParams p{};
    kd_fill_scene(s, w, p);
    bool all_soa = true, candidates = false;
    int64_t total = 0, soa_rays = 0;
    for (int b = 0; b < n_batches; ++b) {
        all_soa = all_soa && !batches[b].rays;
        if (!batches[b].rays) soa_rays += batches[b].n;
        total += batches[b].n;
        candidates = candidates || (batches[b].hc && batches[b].hc->capacity > 0);
    }
    // a candidate call always goes through the record form ("read_soa" has no effect on it)
    const bool read_soa = !candidates && all_soa && kd_scene_reads_soa(s);
    const bool hostc = candidates && s->has_host_prims;  // else: the plain instances over zeroed counts
    if (!read_soa && soa_rays > 0 &&
        !kd_grow(&w->d_in, &w->in_bytes, (size_t)soa_rays * sizeof(nnbvh_ray), "hipMalloc(wavefront rays)"))
        return NNBVH_ERR_DEVICE;
    char *gathered = (char *)w->d_in;
    p.nBatches = n_batches;
    p.anyMask = 0;
    for (int b = 0; b < n_batches; ++b) {
        const KdBatch &k = batches[b];
        p.anyMask |= k.any ? 1u << b : 0u;
        p.bOut[b] = k.out;
        p.bVisited[b] = k.any ? (int32_t *)k.visited : nullptr;
        p.bTests[b] = k.any ? (int32_t *)k.tests : nullptr;
        p.bN[b] = (long)k.n;
        p.bNDev[b] = k.d_n;
        if (k.hc && k.hc->capacity > 0 && k.n > 0) {
            const int zero_blocks = s->n_cus * 8;
            if (!kd_hip_ok(launch_zero_words(k.hc->count, (long)k.n, zero_blocks, stream), "candidate count reset launch") ||
                (!k.any && !kd_hip_ok(launch_zero_words(k.hc->before, (long)k.n, zero_blocks, stream),
                                      "candidate before reset launch")))
                return NNBVH_ERR_DEVICE;
            if (hostc) {
                p.bHcCap[b] = k.hc->capacity;
                p.bHcCount[b] = k.hc->count;
                p.bHcBefore[b] = k.any ? nullptr : k.hc->before;
                p.bHcPrim[b] = k.hc->prim;
                p.bHcInst[b] = k.hc->instance;
            }
        }
        if (read_soa) {
            if (k.soa) p.bSoa[b] = *k.soa;  // (an empty batch may come without slices)
        } else if (!k.rays && k.n > 0) {
            if (!kd_hip_ok(launch_wf_gather(*k.soa, WavefrontCount{(int)k.n, k.d_n}, gathered, s->n_cus * 8, stream),
                           "gather kernel launch"))
                return NNBVH_ERR_DEVICE;
            p.bRays[b] = (const nnbvh_ray *)gathered;
            gathered += (size_t)k.n * sizeof(nnbvh_ray);
        } else {
            p.bRays[b] = (const nnbvh_ray *)k.rays;
        }
    }
    // record form: lean / patches / attributes, each with and without 32-bit offsets; SOA form: lean only
    void (*const kernels[8])(KdParams) = {
        kd_trace_kernel<2, 0, kKdWLean, 0>, kd_trace_kernel<2, 1, kKdW, 0>, kd_trace_kernel<2, 1, kKdW, 0, 1>,
        kd_trace_kernel<3, 0, kKdWLean, 0>, kd_trace_kernel<2, 0, kKdWLean, 1>, kd_trace_kernel<2, 1, kKdW, 1>,
        kd_trace_kernel<2, 1, kKdW, 1, 1>,  kd_trace_kernel<3, 0, kKdWLean, 1>};
    // ... and the candidate-mode twins of the record form
    void (*const hostc_kernels[6])(KdParams) = {
        kd_trace_kernel<2, 0, kKdWLean, 0, 0, 1>, kd_trace_kernel<2, 1, kKdW, 0, 0, 1>, kd_trace_kernel<2, 1, kKdW, 0, 1, 1>,
        kd_trace_kernel<2, 0, kKdWLean, 1, 0, 1>, kd_trace_kernel<2, 1, kKdW, 1, 0, 1>, kd_trace_kernel<2, 1, kKdW, 1, 1, 1>};
    const int form = read_soa ? 3 : (s->d_extras ? 2 : (s->has_patches ? 1 : 0));
    void (*const kernel)(KdParams) = hostc ? hostc_kernels[form + 3 * s->fits32] : kernels[form + 4 * s->fits32];
    const int slot = hostc ? 4 : (read_soa ? 3 : 2);
    if (s->blocks_per_cu[slot] == 0) {
        int occ = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kKdBlock, 0);
        s->blocks_per_cu[slot] = (e == hipSuccess && occ > 0) ? std::min(occ, 8) : 4;
    }
    int blocks = s->n_cus * s->blocks_per_cu[slot];
    const int64_t need = (total + kKdBlock - 1) / kKdBlock;
    if (need < blocks) blocks = (int)std::max<int64_t>(need, 1);
    hipLaunchKernelGGL(kd_zero_queue_kernel, dim3(1), dim3(256), 0, stream, w->queue,
                       n_batches * kKdQueues * kKdQueueStride);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kKdBlock), 0, stream, p);
    return kd_hip_ok(hipGetLastError(), "kd batch trace kernel launch") ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

extern "C" {

nnbvh_kd_scene *nnbvh_kd_scene_create(const nnbvh_kd_node *nodes, int n_nodes, const int32_t *prim_indices,
                                      int n_indices, const nnbvh_prim *prims, int n_prims, const float *verts,
                                      int n_verts, const float bounds_min_max[6], int device) {
    return nnbvh_kd_scene_create_with_attributes(nodes, n_nodes, prim_indices, n_indices, prims, n_prims, verts, n_verts,
                                                 bounds_min_max, nullptr, nullptr, nullptr, device);
}

nnbvh_kd_scene *nnbvh_kd_scene_create_with_attributes(const nnbvh_kd_node *nodes, int n_nodes,
                                                      const int32_t *prim_indices, int n_indices,
                                                      const nnbvh_prim *prims, int n_prims, const float *verts,
                                                      int n_verts, const float bounds_min_max[6], const float *normals,
                                                      const float *uvs, const float *prim_alpha, int device) {
    if (!nodes || n_nodes <= 0 || n_indices < 0 || (n_indices > 0 && !prim_indices) || !prims || n_prims <= 0 ||
        !verts || n_verts <= 0 || !bounds_min_max) {
        set_error("kd_scene_create: null or empty argument");
        return nullptr;
    }
    for (int k = 0; k < n_prims; ++k)
        if (is_alphatex_kind(prims[k].kind)) {
            set_error(std::string("kd_scene_create: ") + kAlphaTexElsewhere);
            return nullptr;
        }
    // ---- validate everything the kernel indexes with ---------------------------------------------
    for (int i = 0; i < n_indices; ++i)
        if (prim_indices[i] < 0 || prim_indices[i] >= n_prims) {
            set_error("kd_scene_create: primitive index out of range in primitiveIndices");
            return nullptr;
        }
    struct Frame {
        int node, end, depth;
    };
    std::vector<Frame> st;
    st.push_back({0, n_nodes, 0});
    int visited = 0, max_depth = 0;
    while (!st.empty()) {
        const Frame f = st.back();
        st.pop_back();
        ++visited;
        if (f.node < 0 || f.node >= f.end) {
            set_error("kd_scene_create: node index outside its subtree range");
            return nullptr;
        }
        max_depth = std::max(max_depth, f.depth);
        const nnbvh_kd_node &nd = nodes[f.node];
        if ((nd.flags & 3u) == 3u) {
            if (f.node + 1 != f.end) {
                set_error("kd_scene_create: leaf does not close its subtree range (not the reference's layout)");
                return nullptr;
            }
            const uint32_t np = nd.flags >> 2;
            const int32_t v = (int32_t)nd.split_or_index;
            if (np == 1 && (v < 0 || v >= n_prims)) {
                set_error("kd_scene_create: leaf primitive index out of range");
                return nullptr;
            }
            if (np > 1 && (v < 0 || (int64_t)v + np > n_indices)) {
                set_error("kd_scene_create: leaf primitive range out of bounds");
                return nullptr;
            }
        } else {
            const int64_t above = nd.flags >> 2;
            if (above <= f.node + 1 || above >= f.end) {
                set_error("kd_scene_create: above-child link outside its subtree range");
                return nullptr;
            }
            float split;
            std::memcpy(&split, &nd.split_or_index, 4);
            if (std::isnan(split)) {
                set_error("kd_scene_create: NaN split position");
                return nullptr;
            }
            st.push_back({(int)above, f.end, f.depth + 1});
            st.push_back({f.node + 1, (int)above, f.depth + 1});
        }
    }
    if (visited != n_nodes) {
        set_error("kd_scene_create: unreachable nodes in the array");
        return nullptr;
    }
    if (max_depth > kMaxStack) {
        set_error("kd_scene_create: tree deeper than the traversal stack (64 entries, aggregates.cpp:982)");
        return nullptr;
    }
    // ---- primitive records: 4 slots per primitive in the caller's order --------------------------
    std::vector<float> rec((size_t)n_prims * 16, 0.0f);
    bool has_host = false, has_patch = false;
    // the alpha-tested kinds that read per-vertex attributes: on the device when the caller gave what they read
    // (6 more slots per primitive in a second array), else the host's as before
    auto on_device = [&](int kind) {
        if (is_smooth_alpha_kind(kind)) return normals != nullptr;
        if (is_alpha_patch_kind(kind))
            return prim_alpha && (!is_smooth_alpha_patch_kind(kind) || normals) && (!is_uv_alpha_patch_kind(kind) || uvs);
        return false;
    };
    bool any_attr = false;
    for (int k = 0; k < n_prims && !any_attr; ++k) any_attr = on_device(prims[k].kind);
    std::vector<float> extras(any_attr ? (size_t)n_prims * 24 : 0, 0.0f);
    for (int k = 0; k < n_prims; ++k) {
        const nnbvh_prim &pr = prims[k];
        float *s = &rec[(size_t)k * 16];
        uint32_t flags = 0;
        std::memcpy(&s[3], &pr.id, 4);
        const bool attr = on_device(pr.kind);
        if (pr.kind == NNBVH_PRIM_HOST || ((is_smooth_alpha_kind(pr.kind) || is_alpha_patch_kind(pr.kind)) && !attr)) {
            // (alpha-tested triangles of smooth meshes and alpha-tested patches without the arrays they read: the host's)
            flags |= kPrimHost;
            has_host = true;
        } else if (is_triangle_kind(pr.kind) || pr.kind == NNBVH_PRIM_BILINEAR_PATCH || is_alpha_patch_kind(pr.kind)) {
            const int nv = is_triangle_kind(pr.kind) ? 3 : 4;
            if (attr) {
                float *ex = &extras[(size_t)k * 24];
                const bool smooth = is_smooth_alpha_kind(pr.kind) || is_smooth_alpha_patch_kind(pr.kind);
                for (int j = 0; j < nv && smooth; ++j)
                    if (pr.v[j] >= 0 && pr.v[j] < n_verts) std::memcpy(&ex[4 * j], normals + 3 * (size_t)pr.v[j], 12);
                for (int j = 0; j < 4 && is_uv_alpha_patch_kind(pr.kind); ++j)
                    if (pr.v[j] >= 0 && pr.v[j] < n_verts) std::memcpy(&ex[16 + 2 * j], uvs + 2 * (size_t)pr.v[j], 8);
                flags |= kPrimAlpha | (smooth ? kPrimSmooth : 0u) | (is_uv_alpha_patch_kind(pr.kind) ? kPrimUV : 0u);
                if (pr.kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED || is_flipped_alpha_patch_kind(pr.kind)) flags |= kPrimFlipN;
                has_host = true;   // a re-trace chain that does not end voids the ray
                has_patch = true;  // the alpha test hashes the ray direction
            }
            if (pr.kind == NNBVH_PRIM_ALPHA_TRIANGLE || pr.kind == NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED) {
                // the alpha value rides in v[3] (bit pattern) and goes to slot 2's w, as in the BVH scenes;
                // a re-trace that hits voids the ray like a host primitive, and the test needs the ray
                // direction: such scenes run the PATCH instances
                flags |= kPrimAlpha | (pr.kind == NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED ? kPrimFlipN : 0u);
                has_host = true;
                has_patch = true;
            }
            for (int j = 0; j < nv; ++j) {
                if (pr.v[j] < 0 || pr.v[j] >= n_verts) {
                    set_error("kd_scene_create: vertex index out of range");
                    return nullptr;
                }
                std::memcpy(&s[4 * j], verts + 3 * (size_t)pr.v[j], 12);
            }
            std::memcpy(&s[3], &pr.id, 4);
            if (flags & kPrimAlpha) {
                if (is_alpha_patch_kind(pr.kind)) s[11] = prim_alpha[k];  // a patch needs all four v[]
                else std::memcpy(&s[11], &pr.v[3], 4);
            }
            if (nv == 4) {
                flags |= kPrimPatch;
                has_patch = true;
            }
            else if (kd_triangle_is_degenerate(&s[0], &s[4], &s[8])) flags |= kPrimDegenerate;
        } else {
            set_error("kd_scene_create: unsupported primitive kind (triangles, alpha-tested triangles, patches, host primitives)");
            return nullptr;
        }
        std::memcpy(&s[7], &flags, 4);
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        set_error("kd_scene_create: no usable HIP device");
        return nullptr;
    }
    KdDeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    hipDeviceProp_t prop;
    if (!kd_hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return nullptr;
    auto *s = new nnbvh_kd_scene;
    s->device = device;
    s->n_cus = prop.multiProcessorCount;
    s->depth = max_depth;
    s->has_host_prims = has_host ? 1 : 0;
    s->has_patches = has_patch ? 1 : 0;
    s->n_nodes = n_nodes;
    s->n_indices = n_indices;
    s->n_prims = n_prims;
    s->fits32 = (n_nodes < (1 << 29) && n_prims < (1 << 26) - 1 && n_indices < (1 << 30)) ? 1 : 0;
    std::memcpy(s->bounds, bounds_min_max, 24);
    const size_t ni = (size_t)std::max(n_indices, 1);
    bool ok = kd_hip_ok(hipMalloc((void **)&s->d_nodes, (size_t)n_nodes * 8), "hipMalloc(kd nodes)") &&
              kd_hip_ok(hipMalloc((void **)&s->d_indices, ni * 4), "hipMalloc(kd indices)") &&
              kd_hip_ok(hipMalloc((void **)&s->d_prims, rec.size() * 4), "hipMalloc(kd prims)") &&
              kd_hip_ok(hipMemcpy(s->d_nodes, nodes, (size_t)n_nodes * 8, hipMemcpyHostToDevice), "upload kd nodes") &&
              kd_hip_ok(hipMemcpy(s->d_prims, rec.data(), rec.size() * 4, hipMemcpyHostToDevice), "upload kd prims");
    if (ok && n_indices > 0)
        ok = kd_hip_ok(hipMemcpy(s->d_indices, prim_indices, (size_t)n_indices * 4, hipMemcpyHostToDevice),
                       "upload kd indices");
    if (ok && any_attr)
        ok = kd_hip_ok(hipMalloc((void **)&s->d_extras, extras.size() * 4), "hipMalloc(kd attributes)") &&
             kd_hip_ok(hipMemcpy(s->d_extras, extras.data(), extras.size() * 4, hipMemcpyHostToDevice), "upload kd attributes");
    if (!ok) {
        nnbvh_kd_scene_destroy(s);
        return nullptr;
    }
    return s;
}

void nnbvh_kd_scene_destroy(nnbvh_kd_scene *s) {
    if (!s) return;
    KdDeviceGuard guard(s->device);
    for (auto &kv : s->workspaces) {
        KdWorkspace &w = kv.second;
        for (void *ptr : {(void *)w.queue, (void *)w.spill, w.d_in, w.d_out, w.d_aux0, w.d_aux1, w.d_hits})
            if (ptr) (void)hipFree(ptr);
        for (void *ptr : w.walk)
            if (ptr) (void)hipFree(ptr);
    }
    if (s->d_nodes) (void)hipFree(s->d_nodes);
    if (s->d_indices) (void)hipFree(s->d_indices);
    if (s->d_prims) (void)hipFree(s->d_prims);
    if (s->d_extras) (void)hipFree(s->d_extras);
    delete s;
}

int nnbvh_kd_intersect_closest_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                      void *stream) {
    if (!s || n < 0 || n >= 0x7fffffffLL || (n > 0 && (!d_rays || !d_hits))) {
        set_error("kd_intersect_closest_device: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, (hipStream_t)stream);
    if (!w) return NNBVH_ERR_DEVICE;
    return kd_launch(s, 0, d_rays, n, d_hits, nullptr, nullptr, nullptr, (hipStream_t)stream, w);
}

int nnbvh_kd_intersect_any_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                  void *d_nodes_visited, void *d_prim_tests, void *stream) {
    if (!s || n < 0 || n >= 0x7fffffffLL || (n > 0 && (!d_rays || !d_occluded))) {
        set_error("kd_intersect_any_device: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, (hipStream_t)stream);
    if (!w) return NNBVH_ERR_DEVICE;
    return kd_launch(s, 1, d_rays, n, nullptr, d_occluded, d_nodes_visited, d_prim_tests, (hipStream_t)stream, w);
}

int nnbvh_kd_scene_set_option(nnbvh_kd_scene *s, const char *key, int value) {
    if (!s || !key) {
        set_error("kd_scene_set_option: null argument");
        return NNBVH_ERR_ARG;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    const std::string k(key);
    if (k == "read_soa") s->read_soa = value != 0;
    else if (k == "pair_one_launch") s->pair_one_launch = value != 0;
    else {
        set_error("kd_scene_set_option: unknown key " + k);
        return NNBVH_ERR_ARG;
    }
    return NNBVH_OK;
}

}  // extern "C"

// nnbvh_kd_trace_batches_device and its candidates form (cands nullable; cands[b] belongs to batches[b], capacity 0 =
// a plain batch).  Everything is checked before the scene is looked at.
static int kd_trace_batches(const char *fn, nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches,
                            const nnbvh_host_candidates *cands, bool with_candidates, void *stream) {
    if (!s || !batches || n_batches < 1 || n_batches > kKdMaxBatches || (with_candidates && !cands)) {
        set_error(std::string(fn) + (with_candidates ? ": bad argument (a scene, 1..4 batches and their candidates)"
                                                     : ": bad argument (a scene and 1..4 batches)"));
        return NNBVH_ERR_ARG;
    }
    KdBatch jobs[kKdMaxBatches];
    int64_t total = 0;
    for (int b = 0; b < n_batches; ++b) {
        const nnbvh_batch &k = batches[b];
        if ((k.kind != NNBVH_BATCH_CLOSEST && k.kind != NNBVH_BATCH_ANY) || k.n < 0 || k.n >= (1LL << kKdIndexBits) ||
            (k.n > 0 && (!k.d_rays || !k.d_out))) {
            set_error(std::string(fn) + ": bad batch (kind, 0 <= n < 2^28, rays and output)");
            return NNBVH_ERR_ARG;
        }
        if (cands && cands[b].capacity != 0) {
            const char *why = candidates_fault(&cands[b], k.kind == NNBVH_BATCH_CLOSEST);
            if (!why && k.kind == NNBVH_BATCH_ANY && (k.d_nodes_visited || k.d_prim_tests))
                why = "an any-hit batch has exact counts or candidates, not both";
            if (why) {
                set_error(std::string(fn) + ": batch candidates: " + why);
                return NNBVH_ERR_ARG;
            }
            jobs[b].hc = &cands[b];
        }
        jobs[b].any = k.kind == NNBVH_BATCH_ANY;
        jobs[b].rays = k.d_rays;
        jobs[b].n = k.n;
        jobs[b].out = k.d_out;
        jobs[b].visited = k.d_nodes_visited;
        jobs[b].tests = k.d_prim_tests;
        total += k.n;
    }
    if (total == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, (hipStream_t)stream);
    if (!w) return NNBVH_ERR_DEVICE;
    return kd_launch_batches(s, w, (hipStream_t)stream, jobs, n_batches);
}

// the arguments of a single-batch candidate call (a one-batch launch: fewer than 2^28 rays)
static bool kd_candidate_args_ok(const char *fn, const nnbvh_kd_scene *s, int64_t n, const void *rays, const void *out,
                                 const nnbvh_host_candidates *c, bool closest) {
    const char *why = nullptr;
    if (!s || n < 0 || (n > 0 && (!rays || !out))) why = "bad argument";
    else if ((why = candidates_fault(c, closest)) != nullptr) {}
    else if (n >= (1LL << kKdIndexBits)) why = "a batch of 2^28 rays or more";
    if (why) set_error(std::string(fn) + ": " + why);
    return !why;
}

static int kd_candidates_device(const char *fn, nnbvh_kd_scene *s, bool any, const void *d_rays, int64_t n, void *d_out,
                                const nnbvh_host_candidates *c, void *stream) {
    if (!kd_candidate_args_ok(fn, s, n, d_rays, d_out, c, !any)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, (hipStream_t)stream);
    if (!w) return NNBVH_ERR_DEVICE;
    KdBatch batch;
    batch.any = any, batch.rays = d_rays, batch.n = n, batch.out = d_out, batch.hc = c;
    return kd_launch_batches(s, w, (hipStream_t)stream, &batch, 1);
}

// host buffers: one staged copy in, one launch on the null stream, copies out (synchronous)
static int kd_candidates_host(const char *fn, nnbvh_kd_scene *s, bool any, const nnbvh_ray *rays, int64_t n, void *out,
                              const nnbvh_host_candidates *c) {
    if (!kd_candidate_args_ok(fn, s, n, rays, out, c, !any)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    const size_t k = (size_t)c->capacity, out_elem = any ? 1 : sizeof(nnbvh_hit);
    void *d_rays = nullptr, *d_out = nullptr;
    nnbvh_host_candidates d{};
    d.capacity = c->capacity;
    bool ok = kd_hip_ok(hipMalloc(&d_rays, (size_t)n * sizeof(nnbvh_ray)), "hipMalloc(rays)") &&
              kd_hip_ok(hipMalloc(&d_out, (size_t)n * out_elem), "hipMalloc(results)") &&
              kd_hip_ok(hipMalloc((void **)&d.count, (size_t)n * 4), "hipMalloc(count)") &&
              (any || kd_hip_ok(hipMalloc((void **)&d.before, (size_t)n * 4), "hipMalloc(before)")) &&
              kd_hip_ok(hipMalloc((void **)&d.prim, (size_t)n * k * 4), "hipMalloc(prim)") &&
              kd_hip_ok(hipMalloc((void **)&d.instance, (size_t)n * k * 4), "hipMalloc(instance)") &&
              kd_hip_ok(hipMemcpy(d_rays, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays") &&
              // the caller's entries beyond count stay as they were: start from them
              kd_hip_ok(hipMemcpy(d.prim, c->prim, (size_t)n * k * 4, hipMemcpyHostToDevice), "copy prim") &&
              kd_hip_ok(hipMemcpy(d.instance, c->instance, (size_t)n * k * 4, hipMemcpyHostToDevice), "copy instance");
    KdWorkspace *w = ok ? kd_workspace_for(s, nullptr) : nullptr;
    int rc = w ? NNBVH_OK : NNBVH_ERR_DEVICE;
    if (rc == NNBVH_OK) {
        KdBatch batch;
        batch.any = any, batch.rays = d_rays, batch.n = n, batch.out = d_out, batch.hc = &d;
        rc = kd_launch_batches(s, w, nullptr, &batch, 1);
    }
    if (rc == NNBVH_OK &&
        !(kd_hip_ok(hipStreamSynchronize(nullptr), "kd trace") &&
          kd_hip_ok(hipMemcpy(out, d_out, (size_t)n * out_elem, hipMemcpyDeviceToHost), "copy results") &&
          kd_hip_ok(hipMemcpy(c->count, d.count, (size_t)n * 4, hipMemcpyDeviceToHost), "copy count") &&
          (any || kd_hip_ok(hipMemcpy(c->before, d.before, (size_t)n * 4, hipMemcpyDeviceToHost), "copy before")) &&
          kd_hip_ok(hipMemcpy(c->prim, d.prim, (size_t)n * k * 4, hipMemcpyDeviceToHost), "copy prim") &&
          kd_hip_ok(hipMemcpy(c->instance, d.instance, (size_t)n * k * 4, hipMemcpyDeviceToHost), "copy instance")))
        rc = NNBVH_ERR_DEVICE;
    for (void *q : {d_rays, d_out, (void *)d.count, (void *)d.before, (void *)d.prim, (void *)d.instance})
        if (q) (void)hipFree(q);
    return rc;
}

extern "C" {

int nnbvh_kd_trace_batches_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches, void *stream) {
    return kd_trace_batches("kd_trace_batches_device", s, batches, n_batches, nullptr, false, stream);
}

int nnbvh_kd_trace_batches_candidates_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches,
                                             const nnbvh_host_candidates *cands, void *stream) {
    return kd_trace_batches("kd_trace_batches_candidates_device", s, batches, n_batches, cands, true, stream);
}

int nnbvh_kd_intersect_closest_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                                 const nnbvh_host_candidates *c, void *stream) {
    return kd_candidates_device("kd_intersect_closest_candidates_device", s, false, d_rays, n, d_hits, c, stream);
}

int nnbvh_kd_intersect_any_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                             const nnbvh_host_candidates *c, void *stream) {
    return kd_candidates_device("kd_intersect_any_candidates_device", s, true, d_rays, n, d_occluded, c, stream);
}

int nnbvh_kd_intersect_closest_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits,
                                          const nnbvh_host_candidates *c) {
    return kd_candidates_host("kd_intersect_closest_candidates", s, false, rays, n, hits, c);
}

int nnbvh_kd_intersect_any_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                                      const nnbvh_host_candidates *c) {
    return kd_candidates_host("kd_intersect_any_candidates", s, true, rays, n, occluded, c);
}

int nnbvh_kd_intersect_closest(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits) {
    if (!s || n < 0 || n >= 0x7fffffffLL || (n > 0 && (!rays || !hits))) {
        set_error("kd_intersect_closest: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, nullptr);
    if (!w) return NNBVH_ERR_DEVICE;
    if (!kd_grow(&w->d_in, &w->in_bytes, (size_t)n * sizeof(nnbvh_ray), "hipMalloc(rays)") ||
        !kd_grow(&w->d_out, &w->out_bytes, (size_t)n * sizeof(nnbvh_hit), "hipMalloc(hits)"))
        return NNBVH_ERR_DEVICE;
    if (!kd_hip_ok(hipMemcpy(w->d_in, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays"))
        return NNBVH_ERR_DEVICE;
    const int rc = kd_launch(s, 0, w->d_in, n, w->d_out, nullptr, nullptr, nullptr, nullptr, w);
    if (rc != NNBVH_OK) return rc;
    if (!kd_hip_ok(hipStreamSynchronize(nullptr), "kd trace") ||
        !kd_hip_ok(hipMemcpy(hits, w->d_out, (size_t)n * sizeof(nnbvh_hit), hipMemcpyDeviceToHost), "copy hits"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

int nnbvh_kd_intersect_any(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                           int32_t *nodes_visited, int32_t *prim_tests) {
    if (!s || n < 0 || n >= 0x7fffffffLL || (n > 0 && (!rays || !occluded))) {
        set_error("kd_intersect_any: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    KdDeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::lock_guard<std::mutex> lock(s->mu);
    KdWorkspace *w = kd_workspace_for(s, nullptr);
    if (!w) return NNBVH_ERR_DEVICE;
    if (!kd_grow(&w->d_in, &w->in_bytes, (size_t)n * sizeof(nnbvh_ray), "hipMalloc(rays)") ||
        !kd_grow(&w->d_out, &w->out_bytes, (size_t)n, "hipMalloc(occluded)") ||
        !kd_grow(&w->d_aux0, &w->aux_bytes, (size_t)n * 8, "hipMalloc(counts)"))
        return NNBVH_ERR_DEVICE;
    int32_t *d_vis = (int32_t *)w->d_aux0, *d_tst = d_vis + n;
    if (!kd_hip_ok(hipMemcpy(w->d_in, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays"))
        return NNBVH_ERR_DEVICE;
    const int rc = kd_launch(s, 1, w->d_in, n, nullptr, w->d_out, nodes_visited ? d_vis : nullptr,
                             prim_tests ? d_tst : nullptr, nullptr, w);
    if (rc != NNBVH_OK) return rc;
    if (!kd_hip_ok(hipStreamSynchronize(nullptr), "kd trace") ||
        !kd_hip_ok(hipMemcpy(occluded, w->d_out, (size_t)n, hipMemcpyDeviceToHost), "copy occluded"))
        return NNBVH_ERR_DEVICE;
    if (nodes_visited && !kd_hip_ok(hipMemcpy(nodes_visited, d_vis, (size_t)n * 4, hipMemcpyDeviceToHost), "copy counts"))
        return NNBVH_ERR_DEVICE;
    if (prim_tests && !kd_hip_ok(hipMemcpy(prim_tests, d_tst, (size_t)n * 4, hipMemcpyDeviceToHost), "copy counts"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

}  // extern "C"

// ---- the walk calls' launchers (capi_wavefront.cpp: nnbvh_kd_wavefront_walk_*) ------------------------------------
bool nnbvh::kd_walk_scratch(KdWorkspace *w, int slot, size_t bytes, void **out) {
    if (!kd_grow(&w->walk[slot], &w->walk_bytes[slot], std::max<size_t>(bytes, 16), "hipMalloc(walk workspace)"))
        return false;
    *out = w->walk[slot];
    return true;
}

int nnbvh::launch_walk(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const WalkJob &k) {
    KdParams p{};
    kd_fill_scene(s, w, p);
    p.nBatches = 1;
    p.anyMask = 0;
    p.bRays[0] = (const nnbvh_ray *)k.rays;
    p.bN[0] = (long)k.n;
    p.bNDev[0] = k.d_n;
    const ShadingMeshDevice &m = *k.mesh;
    p.wMesh = {m.verts, m.triVerts, m.patchVerts, m.normals, m.uvs, m.tangents, m.faceIndices, m.triFlags, m.nTris,
               m.defaultFlags, nullptr, 0, nullptr, nullptr};  // kd scenes have one level
    p.walk = k.a;
    // the lean instance with the triangle-only interaction where neither the scene nor the mesh holds patches, else the
    // PATCH = 1 instance with the patch-capable one (launch_str_step's choice of FULL); each with both offset widths
    void (*const kernels[8])(KdParams) = {
        kd_trace_kernel<4, 0, kKdWLean, 0>, kd_trace_kernel<4, 1, kKdW, 0>, kd_trace_kernel<4, 0, kKdWLean, 1>,
        kd_trace_kernel<4, 1, kKdW, 1>,     kd_trace_kernel<5, 0, kKdWLean, 0>, kd_trace_kernel<5, 1, kKdW, 0>,
        kd_trace_kernel<5, 0, kKdWLean, 1>, kd_trace_kernel<5, 1, kKdW, 1>};
    const int full = (s->has_patches || m.patchVerts) ? 1 : 0;
    void (*const kernel)(KdParams) = kernels[4 * (k.kind - 1) + 2 * s->fits32 + full];
    const int slot = 5 + 2 * (k.kind - 1) + full;
    if (s->blocks_per_cu[slot] == 0) {
        int occ = 0;
        const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kKdBlock, 0);
        s->blocks_per_cu[slot] = (e == hipSuccess && occ > 0) ? std::min(occ, 8) : 4;
    }
    int blocks = s->n_cus * s->blocks_per_cu[slot];
    const int64_t need = (k.n + kKdBlock - 1) / kKdBlock;
    if (need < blocks) blocks = (int)std::max<int64_t>(need, 1);
    hipLaunchKernelGGL(kd_zero_queue_kernel, dim3(1), dim3(256), 0, stream, w->queue, kKdQueues * kKdQueueStride);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(kKdBlock), 0, stream, p);
    return kd_hip_ok(hipGetLastError(), "kd walk kernel launch") ? NNBVH_OK : NNBVH_ERR_DEVICE;
}
