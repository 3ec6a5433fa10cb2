// kd_trace.hip — KdTreeAggregate::Intersect / IntersectP on gfx950: the kernel and its launcher (kd_trace.h; the C ABI
// of kd-tree scenes is capi_kd.cpp).
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

#include <array>
#include <utility>

#include "../../include/nnbvh.h"
#include "nnbvh_internal.h"
#include "trace_math.h"
#include "alpha_texture_math.h"
#include "spawn_math.h"
#include "kd_trace.h"
#include "launch_ledger.h"
#include "walk_math.h"

namespace nnbvh {

constexpr int kKdDone = -1;          // lane carries no ray
constexpr int kKdLeaf = -2;          // lane is walking the primitives of a leaf

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
// ATTR = 2 (with PATCH = 1): the scene holds triangles whose alpha is an image texture (kPrimAlphaTex records; the
// creation calls refuse alpha-tested patches beside them, so the patch recursion is not compiled in; a scene that has
// a table but no such triangle runs the ATTR = 0 / 1 instances).  The ATTR = 1 triangle path
// with, for such a triangle, alpha = FloatImageTexture::Evaluate at the hit's (u, v) (alpha_texture_math.h: the (u, v)
// pairs from slots 4 / 5 of the primitive's extras, the descriptor from p.alphaTex, the texels from p.alphaTexels)
// instead of the constant in slot 2 (bvh_trace.hip's ALPHA = 3 code)
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
    auto at = [](const auto *base, int index, int scale = 1) {  // &base[index * scale]; the wide form widens first
        using T = decltype(base);
        return O32 ? reinterpret_cast<T>(reinterpret_cast<const char *>(base) +
                                         (unsigned)(scale * index) * (unsigned)sizeof(*base))
                   : base + (long)index * scale;
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
                const float4 *rec = at(p.prims, leafIdx, 4);
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
                            [[maybe_unused]] float aTex = 0.0f;
                            if constexpr (ATTR == 2) {
                                // alpha.Evaluate(si->intr) of a FloatImageTexture: the (u, v) slots, the descriptor and
                                // the texels are read here, on a hit only, and are dead before the normals are fetched
                                // below
                                if (flags & kPrimAlphaTex) {
                                    const float4 *uvp = p.extras + 6 * (long)leafIdx + 4;
                                    const float4 uva = uvp[0], uvb = uvp[1];
                                    const float4 *dp = p.alphaTex + 3 * (long)__float_as_int(s2.w);
                                    const float4 d0 = dp[0], d1 = dp[1], d2 = dp[2];
                                    const AlphaTexDesc desc = {__float_as_uint(d0.x), __float_as_uint(d0.y),
                                                               __float_as_int(d0.z), __float_as_int(d0.w),
                                                               __float_as_int(d1.x), __float_as_int(d1.y), d1.z, d1.w,
                                                               d2.x, d2.y, d2.z, __float_as_int(d2.w)};
                                    aTex = alpha_texture_eval(x0, x1, x2, uva.x, uva.y, uva.z, uva.w, uvb.x, uvb.y, desc,
                                                              p.alphaTexels);
                                }
                            }
                            const float a = (ATTR == 2 && (flags & kPrimAlphaTex)) ? aTex : s2.w;
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
                        if constexpr (ATTR == 1) {
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

// ---- the instances: one kernel per entry of kKdInstances (kd_instance.h), in its order and under its row number ------
template <size_t I>
constexpr auto kd_kernel() {  // the window follows from patch
    constexpr KdInstance k = kKdInstances[I];
    return kd_trace_kernel<k.mode, k.patch, k.patch ? kKdW : kKdWLean, k.o32, k.attr, k.hostc>;
}
template <size_t... I>
constexpr std::array<void (*)(KdParams), sizeof...(I)> kd_kernels(std::index_sequence<I...>) {
    return {{kd_kernel<I>()...}};
}
static const auto kKdKernels = kd_kernels(std::make_index_sequence<kKdInstanceCount>());

// the launch ledger: one count per entry of kKdInstances, in its order
static LaunchLedger<kKdInstanceCount> g_kd_ledger;

hipError_t launch_kd_trace(const KdInstance &is, const KdParams &p, int blocks, hipStream_t stream, int *occupancy) {
    const int row = kd_instance_index(is);
    if (row < 0) return hipErrorInvalidValue;
    if (occupancy) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occupancy, kKdKernels[row], kKdBlock, 0);
    hipLaunchKernelGGL(kKdKernels[row], dim3((unsigned)blocks), dim3(kKdBlock), 0, stream, p);
    g_kd_ledger.count(row);
    return hipGetLastError();
}

int kd_instance_launches(int32_t *desc, uint64_t *counts, int capacity, int reset) {
    return g_kd_ledger.read(desc, counts, capacity, reset, [](int i) {
        const KdInstance &k = kKdInstances[i];
        return std::array<int32_t, 7>{{k.mode, k.patch, k.o32, k.attr, k.hostc}};
    });
}

}  // namespace nnbvh
