// bvh_trace.hip — hand-written gfx950 traversal kernels for the nnbvh C ABI.
//
// What is computed (reference: /root/reference/src/pbrt):
//   closest hit   BVHAggregate::Intersect   cpu/aggregates.cpp:529-579
//   any hit       BVHAggregate::IntersectP  cpu/aggregates.cpp:581-624
//   slab test     Bounds3::IntersectP       util/vecmath.h:1573-1608
//   triangle      IntersectTriangle         shapes.cpp:172-273
//   patch         IntersectBilinearPatch    shapes.h:1279-1347 (+ util/math.h:614-637, 1420-1426)
// Results (hit primitive, t, barycentrics, node-visit and primitive-test counts) are
// bit-identical to that code; HOW it is computed is CDNA4-specific:
//   * persistent 64-lane wavefronts pull rays from a global queue; lanes whose ray has
//     terminated are refilled in place (ballot + mbcnt compaction of the idle lanes), so
//     SIMD slots stay occupied although rays visit 1..400 nodes each;
//   * one 64-B "both children" record per interior node (nnbvh_internal.h) halves the
//     length of the dependent-load chain of the reference's 32-B node walk; a child box's
//     whole slab test is carried by ONE float, its entry distance or +inf (trace_math.h
//     slab_entry_key), and the far child is pushed WITH it, so the deferred box test the
//     reference performs when it pops the node (`tMin < tMax` with the then-current tMax)
//     needs no memory access at all and still gives the identical boolean;
//   * the per-lane traversal stack is a short ring window in LDS ([entry][word][lane], bank-
//     conflict-free) that spills its oldest entry to a coalesced HBM scratch array only
//     when a ray's pending-node list outgrows the window;
//   * fp32 arithmetic is emitted with -ffp-contract=off; __builtin_fmaf appears exactly
//     where the reference calls FMA(); division and sqrt are IEEE (hipcc default).
// No MFMA: this is pointer chasing + branchy fp32, bounded by cache/HBM request rate.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <array>
#include <cstring>
#include <iterator>
#include <utility>

#include "bvh_trace.h"
#include "alpha_texture_math.h"
#include "anim_math.h"
#include "launch_ledger.h"
#include "spawn_math.h"
#include "stream_access.h"
#include "top_extend.h"
#include "trace_math.h"
#include "walk_math.h"

namespace nnbvh {

// ------------------------------------------------------------------------------------
constexpr int kDone = (int)0x80000000;    // never a leaf ref: ~slot with slot = 0x7fffffff
constexpr int kReturn = (int)0x80000001;  // an instance's child traversal is exhausted (slot 0x7ffffffe)
constexpr int kEnter = (int)0x80000002;   // INST = 2: the lane waits to enter an AnimatedPrimitive (slot 0x7ffffffd)

// trace_kernel<MODE, W, INST, PATCH, ALPHA, SOA, HOSTC>: every ray of every entry point runs through one instance
// of this template (trace_instance.h lists the instances and picks one from the scene and the call).
//
// MODE 0: closest hit (counts always)
// MODE 1: any hit with exact node-visit / prim-test counts (pushes every far child)
// MODE 2: any hit, occlusion flag only
// MODE 3: several batches in ONE launch, each closest hit (as MODE 0) or occlusion-only any hit (as
//         MODE 2): the batches of one wavefront iteration share a single ramp-up and a single drain
//         (DESIGN.md §5.1).  A lane's ray tag carries its batch; what differs per lane is only what a
//         hit does and what is written at retire.
//
// W: entries per lane of the LDS stack window (4, 8 or 16; every instance but the general single-level one has 8).
//
// Every lane is a small state machine over `cur`:
//     cur >= 0            an interior record to process        (interior step)
//     cur <  0, != kDone  ~cur = prim-stream slot to test next (primitive step)
//     cur == kReturn      INST: the child tree is exhausted    (primitive step: back to the outer leaf)
//     cur == kEnter       INST = 2: waits at an AnimatedPrimitive (enter step)
//     cur == kDone        no ray (refill trip: retire the finished one, fetch the next)
// Each trip of the scheduling loop the WAVE picks one kind of step (wave-uniform, from
// ballots) and the lanes in that state execute it; the others idle for that trip.  A ray's
// own sequence of steps is exactly the reference's, so results cannot depend on the policy.
// These step kinds (refill, enter, primitive, interior and, in the lean one-launch instances, table) are all there are.
// A table step is an interior step for the lanes whose record is in the block's LDS top table only: no global load, so
// it does not last a global round trip.  An interior trip begins with table steps while at least p.topBurst lanes wait at
// a tagged record; the check sits there and not at the head of the loop, where it cost every trip 1.5 % in all.
//
// INST = 1: the scene is two-level (TransformedPrimitive leaves, cpu/primitive.cpp:112-131).  An
// instance primitive saves the lane's ray state in LDS, transforms the ray with the reference's
// interval arithmetic, traverses the child tree ABOVE the current stack level (`floor`) and
// returns to the outer leaf when the child is exhausted.  Compiled separately so that
// single-level scenes pay nothing for it.
//
// INST = 2: ... with AnimatedPrimitives among the instances (the interpolation of the transform costs 60
// VGPRs; scenes whose instances are all static run INST = 1).
//
// PATCH = 0 ("lean"): the scene holds no bilinear patches, no instances and no host-only primitives, so
// nothing ever reads the ray direction after the ray is fetched: no patch test, no direction / ray
// index / host flag in LDS (20 KiB per block = 8 blocks per CU), <= 64 VGPRs = 8 wavefronts per SIMD,
// records and slots through 32-bit offsets from a scalar base, and the ray-invariant select predicates
// (direction signs, kz) kept as wave-level masks in SGPRs (trace_math.h RayMasks) instead of being
// recomputed per lane in every step.
// ALPHA = 1: the scene holds alpha-tested triangles (kPrimAlpha, cpu/primitive.cpp:57-70); compiled
// separately so that other scenes pay nothing for the hash and the re-trace.
// ALPHA = 2: ... and alpha-tested bilinear patches (the patch's interaction point and normal incl. the (s, t)
// reparametrisation, the re-trace loop).
// ALPHA = 3: the scene holds triangles whose alpha is an image texture (kPrimAlphaTex; flat scenes, no alpha-tested
// patches): the ALPHA = 1 path where, for such a triangle, alpha is FloatImageTexture::Evaluate at the hit's (u, v)
// (alpha_texture_math.h) instead of the constant in slot 2.  Constant-alpha triangles run as in ALPHA = 1.
// Two-level scenes have no ALPHA = 3 instances: a two-level scene with a textured triangle reports has_alpha = 2 and
// runs the INST = 1 / 2 x ALPHA = 2 instances, which carry the same branch (kAlphaTex below) beside the patches' one.
// There the barycentrics and the hash are those of the instance-space ray (the top-level list: the ray as given),
// and textured triangles and alpha-tested patches may share a scene.  The flat ALPHA = 2 instances do not have it.
// SOA = 1 (lean instances of modes 0, 2, 3 only): a batch without nnbvh_ray records (rays == nullptr) is read as the
// SOA<Ray> slices of a wavefront queue — no gather pass.  Its own instances: the mere presence of the second fetch
// path in the refill trip cost the one-launch step 1.3 % (9.31 -> 9.44 ms).
// HOSTC = 1 (general instances of modes 0, 2 and 3, window 8, scenes with host-only primitives): candidate mode.  A
// host-only primitive no longer voids the ray: its id and the current instance are appended to the ray's list
// (p.hcPrim / p.hcInst at ray * K, traversal order, the count in the kColdHost slot), and the walk goes on as
// the walk that skips it, which is what the plain instances do already.  Closest hit: an accepted hit on a ray
// with candidates stores how many came before it (p.hcBefore).  At retire the count goes to p.hcCount and the
// record keeps its real instance unless the list overflowed (-1) or an alpha re-trace voided the ray (-2).
// Instances of their own, so that the other instances' code is not touched.
// MODE 3 (no ALPHA instances): every batch has its own five arrays (p.bHc*), picked by the lane's batch tag at the same
// three sites; a batch with bHcCap[b] == 0 is a plain batch (its first host-only primitive "overflows" a list of
// zero entries, so the record is void as in the plain instances, and nothing is written to candidate arrays).
//
// Cache policy: the rays a refill trip fetches and the records, flags and counts a retire writes are used once per
// launch and go past the caches' default policy (stream_access.h: the `nt` forms of global_load / global_store), so
// that they do not evict the tree's records: crown step 9.21 -> 8.96 ms (-2.7 %).  Interior records,
// primitive slots and the stack spill stay on plain accesses: streamed, slots cost +17.6 % and spills +2.5 %.
//
// Tuning constants (each with its measurement; -D overrides are for A/B builds only).
// waves/SIMD the register allocator must leave room for (measured in steady state: closest
// hit 5 -> 6 waves is +9 %; beyond that the spills cost more than the extra waves hide)
#ifndef NNBVH_MINW_CLOSEST
#define NNBVH_MINW_CLOSEST 6
#endif
#ifndef NNBVH_MINW_ANY
#define NNBVH_MINW_ANY 6
#endif
// ... and the waves/SIMD the lean instances (<= 64 VGPRs) run on top of that
#ifndef NNBVH_LEAN_EXTRA_WAVES
#define NNBVH_LEAN_EXTRA_WAVES 2
#endif
// the ALPHA instances (hash + re-trace in the primitive step): at 6 waves they spill 8-18 registers, at 5 none —
// a 1 M-triangle soup with 70 % alpha-tested triangles: closest 6.26 -> 4.95 ms, any 5.38 -> 4.52 ms
#ifndef NNBVH_MINW_ALPHA
#define NNBVH_MINW_ALPHA 5
#endif
// ALPHA = 2: 158-162 VGPRs = 3 waves without spills; 2 waves measured 30 % slower, 4 waves (22-27 spilled
// registers) no faster
#ifndef NNBVH_MINW_ALPHA_PATCH
#define NNBVH_MINW_ALPHA_PATCH 3
#endif
// ALPHA = 3 (tools/isa_regs.py, profiles/alpha_texture.txt): at 5 waves the closest-hit instances spill 2-6 registers,
// at 4 none (93-102 VGPRs)
#ifndef NNBVH_MINW_ALPHA_TEX
#define NNBVH_MINW_ALPHA_TEX 4
#endif
// the walk instances (MODE 4 / 5, DESIGN.md §5.5.1: the interaction, the spawn and the reservoir update at retire):
// bounds chosen from tools/isa_regs.py as the most waves at which no instance spills
#ifndef NNBVH_MINW_WALK_LEAN
#define NNBVH_MINW_WALK_LEAN 4
#endif
#ifndef NNBVH_MINW_WALK
#define NNBVH_MINW_WALK 4
#endif
// ... of the instance trace_kernel<modew, W, inst, patch, alpha, SOA, HOSTC>
constexpr int min_waves(int modew, int inst, int patch, int alpha) {
    if (inst) return 1;  // two-level scenes: no bound (98-116 VGPRs, 160-177 with the interpolation of INST = 2)
    if (modew >= 4) return patch ? NNBVH_MINW_WALK : NNBVH_MINW_WALK_LEAN;
    if (alpha == 2) return NNBVH_MINW_ALPHA_PATCH;  // alpha-tested patches
    if (alpha == 3) return NNBVH_MINW_ALPHA_TEX;    // image-textured alpha
    if (alpha) return NNBVH_MINW_ALPHA;             // alpha-tested triangles
    return ((modew == 0 || modew == 3) ? NNBVH_MINW_CLOSEST : NNBVH_MINW_ANY) + (patch ? 0 : NNBVH_LEAN_EXTRA_WAVES);
}
// Threads per block of that instance.  The two lean one-launch instances (kTop below) run the CU's 32 waves as two
// blocks of 1024 threads instead of eight of 256: two copies of the LDS top table per CU instead of eight leave each
// room for top_lds_records() = 255 records instead of 63 (512: 127 records, A/B builds only).
#ifndef NNBVH_TOP_BLOCK
#define NNBVH_TOP_BLOCK 1024
#endif
constexpr int block_threads(int modew, int inst, int patch) {
    return (modew == 3 && !inst && !patch) ? NNBVH_TOP_BLOCK : kBlockThreads;
}
int trace_block_threads(const TraceInstance &is) { return block_threads(is.mode, is.inst, is.patch); }

// The prologue of the lean one-launch instances, for a block of BT threads: the scene's nTop records copied into s_top,
// then the extension of top_extend.h from `wide` up to top_lds_records(BT) records, two barriers per generation (every
// wave scans every group of pairs itself, so no ballot goes through LDS; nobody patches a word before all have
// scanned).  Every thread of the block calls it.  Returns the records in the table.
template <int BT>
__device__ __forceinline__ int load_top_table(float4 *s_top, const float4 *top, int nTop, const float4 *wide) {
    constexpr int kCap = top_lds_records(BT);
    static_assert(kCap >= kTopRecords && kTopRecords * 4 <= BT, "one float4 per thread copies the scene's table");
    static_assert(2 * kCap <= BT, "one (slot, child) pair per thread in a generation");
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < nTop * 4) s_top[t] = top[t];
    __syncthreads();  // every thread of every block, whatever the launch has to do
    int next = nTop;
    if constexpr (kCap > kTopRecords) {
        float *words = reinterpret_cast<float *>(s_top);
        int begin = 0;
        while (next < kCap && begin < next) {  // (block-uniform; nTop == 0: no table, no extension)
            const int end = next, nPairs = 2 * (end - begin), nGroups = (nPairs + 63) >> 6;
            TopGroupScan scan;
            int ref = -1;  // the reference of this thread's pair, number t
            for (int g = 0; g < nGroups; ++g) {
                const int pair = 64 * g + lane;
                int r = -1;
                if (pair < nPairs) r = __float_as_int(words[(begin + (pair >> 1)) * 16 + 12 + (pair & 1)]);
                scan.add(g, wave, __ballot(top_is_candidate(r)));
                ref = g == wave ? r : ref;
            }
            const int slot = top_is_candidate(ref) ? scan.slot(lane, next, kCap) : -1;
            __syncthreads();
            if (slot >= 0) {
                const float4 *rec = wide + 4 * (long)ref;
                const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2], q3 = rec[3];
                s_top[4 * slot] = q0;
                s_top[4 * slot + 1] = q1;
                s_top[4 * slot + 2] = q2;
                s_top[4 * slot + 3] = q3;
                words[(begin + (t >> 1)) * 16 + 12 + (t & 1)] = __int_as_float(kTopTag | slot);
            }
            __syncthreads();
            begin = end;
            next = next + scan.total < kCap ? next + scan.total : kCap;
        }
    }
    return next;
}
// ... alone, for tests: block b writes its table to out + b * top_lds_records(BT) * 4 and its record count to nOut[b]
template <int BT>
__global__ __launch_bounds__(BT) void top_table_debug_kernel(const float4 *top, int nTop, const float4 *wide,
                                                             float4 *out, int *nOut) {
    constexpr int kCap = top_lds_records(BT);
    __shared__ float4 s_top[kCap * 4];
    const int n = load_top_table<BT>(s_top, top, nTop, wide);
    for (int k = threadIdx.x; k < n * 4; k += BT) out[(long)blockIdx.x * kCap * 4 + k] = s_top[k];
    if (threadIdx.x == 0) nOut[blockIdx.x] = n;
}
int top_debug_capacity() { return top_lds_records(NNBVH_TOP_BLOCK); }
hipError_t launch_top_table_debug(const float4 *top, int nTop, const float4 *wide, int blocks, float4 *out, int *nOut,
                                  hipStream_t stream) {
    hipLaunchKernelGGL(top_table_debug_kernel<NNBVH_TOP_BLOCK>, dim3((unsigned)blocks), dim3(NNBVH_TOP_BLOCK), 0,
                       stream, top, nTop, wide, out, nOut);
    return hipGetLastError();
}

// INST = 2: weight of a lane waiting to enter an AnimatedPrimitive in the step selection (interior = 16); 0 = enter
// at once inside the primitive step (the round-2 form: 11 of 64 lanes active in the interpolation)
#ifndef NNBVH_ANIM_ENTER_WEIGHT
#define NNBVH_ANIM_ENTER_WEIGHT 8
#endif
// entry b of a per-batch table of the kernel arguments (scalar loads and selects: no indexed access into the argument)
template <typename T>
__device__ __forceinline__ T pick_batch(const T (&a)[kMaxFusedBatches], int b) {
    static_assert(kMaxFusedBatches == 4, "written out for four batches");
    return b == 0 ? a[0] : (b == 1 ? a[1] : (b == 2 ? a[2] : a[3]));
}

// A lane takes up the ray {R0, R1} = {o, tMax} {d, time}: the reciprocals and the shear (aggregates.cpp:534-535), cold
// hit slots, the INST fields, the host flag, the counts (the root is visited), an empty stack and the root slab test.
// Used at a refill and, in the walk instances, when an item's walk goes on with its spawned ray.  A macro and not a
// lambda or a function, as KD_BEGIN_RAY (kd_trace.hip): the refill path of the existing instances then compiles to the
// code it compiled to before the walk instances shared it.
#define BVH_BEGIN_RAY(R0, R1)                                                                                         \
    do {                                                                                                              \
        r.o = {(R0).x, (R0).y, (R0).z};                                                                               \
        tMax = (R0).w;                                                                                                \
        const V3 d = {(R1).x, (R1).y, (R1).z};                                                                        \
        if (PATCH) {                                                                                                  \
            cold[kColdD][lane] = d.x;                                                                                 \
            cold[kColdD + 1][lane] = d.y;                                                                             \
            cold[kColdD + 2][lane] = d.z;                                                                             \
        }                                                                                                             \
        /* aggregates.cpp:534-535 */                                                                                  \
        r.inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};                                                                 \
        ray_shear(r, d);                                                                                              \
        if constexpr (kTop) {                                                                                         \
            hit0 = __int_as_float(-1);                                                                                \
            hit1 = hit2 = hit3 = 0.0f;                                                                                \
        } else if (MODE == 0 || MODE == 3) {                                                                          \
            cold[kColdHit][lane] = __int_as_float(-1);                                                                \
            cold[kColdHit + 1][lane] = 0.0f;                                                                          \
            cold[kColdHit + 2][lane] = 0.0f;                                                                          \
            cold[kColdHit + 3][lane] = 0.0f;                                                                          \
        }                                                                                                             \
        if (INST) {                                                                                                   \
            cold[kHitInst][lane] = 0.0f;                                                                              \
            cold[kCurInst][lane] = 0.0f;                                                                              \
            cold[kColdTime][lane] = (R1).w; /* ray.time: read by animated instances */                                \
            floor = -1;                                                                                               \
        }                                                                                                             \
        if (!kLean && (HOSTC || p.hasHostPrims)) cold[kColdHost][lane] = 0.0f; /* candidate mode: count 0 */          \
        if constexpr (WALK != 0) {                                                                                    \
            cold[kWalkD][lane] = (R1).x;                                                                              \
            cold[kWalkD + 1][lane] = (R1).y;                                                                          \
            cold[kWalkD + 2][lane] = (R1).z;                                                                          \
            cold[kWalkTime][lane] = (R1).w;                                                                           \
            cold[kWalkTMax][lane] = (R0).w;                                                                           \
        }                                                                                                             \
        visited = 1; /* the root */                                                                                   \
        tests = 0;                                                                                                    \
        found = false;                                                                                                \
        sp = base = 0;                                                                                                \
        float tEntry;                                                                                                 \
        const bool rootHit = slab_partial(p.rootMin[0], p.rootMin[1], p.rootMin[2], p.rootMax[0], p.rootMax[1],       \
                                          p.rootMax[2], r, tEntry) &&                                                 \
                             (tEntry < tMax);                                                                         \
        cur = rootHit ? p.rootRef : kDone;                                                                            \
    } while (0)

// MODEW = MODE, or 4 / 5 for the walk instances: MODE 0 (record-reading, one-batch closest hit) with WALK = 1
// (IntersectShadowTr) / WALK = 2 (IntersectOneRandom); DESIGN.md §5.5.1.  A lane does not retire its ray when the
// closest-hit walk is finished: it runs one step of the walk for its work item (walk_math.h: the verdicts and arithmetic
// of the fused pass steps of wavefront2.hip) on the hit record a MODE 0 lane would store and, where the item's walk goes
// on, re-enters the tree at the root with the spawned ray.  Nothing is written to p.hits.  The ray index a lane fetched
// is its item.  PATCH = 1 instances compute the interaction with the patch- and instance-capable code (FULL), the lean
// one with the triangle-only code.  Window 8 only; no ALPHA, SOA, HOSTC or INST = 2 forms.  (WALK rides in the first
// template argument and not as an eighth one: that would rename every existing instance.)
template <int MODEW, int W, int INST, int PATCH, int ALPHA = 0, int SOA = 0, int HOSTC = 0>
__global__ __launch_bounds__(block_threads(MODEW, INST, PATCH), min_waves(MODEW, INST, PATCH, ALPHA))
void trace_kernel(TraceParams p) {
    constexpr int WALK = MODEW >= 4 ? MODEW - 3 : 0;
    constexpr int MODE = WALK ? 0 : MODEW;
    static_assert(!WALK || (MODEW <= 5 && W == 8 && INST != 2 && !ALPHA && !SOA && !HOSTC),
                  "walk instances: the plain record-reading closest-hit form at window 8");
    static_assert(PATCH || !INST, "two-level scenes need the ray direction");
    static_assert(PATCH || !ALPHA, "the alpha test hashes the ray direction");
    static_assert(ALPHA != 3 || (INST == 0 && W == 8 && MODE != 3), "textured alpha: flat scenes, window 8, modes 0 / 1 / 2");
    static_assert(!HOSTC || (PATCH && (MODE == 0 || MODE == 2 || (MODE == 3 && !ALPHA && W == 8)) && !SOA),
                  "candidate mode: general instances of modes 0 / 2 / 3");
    // the instance evaluates image-textured alpha (kPrimAlphaTex): the flat ALPHA = 3 instances, and the ALPHA = 2
    // instances of two-level scenes, which are the ones such a scene gets when it holds a textured triangle
    constexpr bool kAlphaTex = ALPHA == 3 || (ALPHA == 2 && INST != 0);
    constexpr int BT = block_threads(MODEW, INST, PATCH);
    // the stack window: entry k of a lane = (child reference, entry distance), the two words 64 dwords
    // apart so that one ds_read2st64 / ds_write2st64 with one address moves both
    __shared__ float s_stack[BT / 64][W][2][64];
    // Cold per-ray state parked in LDS ([field][lane], conflict-free) instead of VGPRs: the
    // ray index (read when the ray retires), the direction (read by the patch test only; the
    // triangle test uses the precomputed shear) and, closest hit, the current best hit
    // (written on an accepted hit, read at retire).  Frees 4 / 8 registers per lane.
    // The lean instances (PATCH = 0: no patches, no instances, and — the launcher sees to it — no
    // host-only primitives) keep the ray index in a VGPR and have no host flag: the closest-hit kernel's
    // cold state is then the four hit words, 20 KiB of LDS per block with the stack window, which is
    // what lets an EIGHTH block share the CU's 160 KiB (its 61 VGPRs allow 8 wavefronts per SIMD).
    constexpr bool kLean = !PATCH && !INST;
    constexpr int kColdRi = 0, kColdD = 1, kColdHit = kLean ? 0 : (PATCH ? 4 : 1),
                  kColdHost = kColdHit + ((MODE == 0 || MODE == 3) ? 4 : 0);
    constexpr int kColdBase = kColdHost + (kLean ? 0 : 1);  // kColdHost: the ray reached a host-only primitive
    // two-level scenes: the outer ray saved while a child tree is traversed
    constexpr int kSaveO = kColdBase, kSaveInv = kColdBase + 3, kSaveShear = kColdBase + 6,
                  kSaveKz = kColdBase + 9, kSaveTmax = kColdBase + 10, kSaveD = kColdBase + 11,
                  kResume = kColdBase + 14, kCurInst = kColdBase + 15, kHitInst = kColdBase + 16,
                  kInnerHit = kColdBase + 17, kColdTime = kColdBase + 18, kPendSlot = kColdBase + 19;
    // WALK: six more slots — the direction, time and tMax of the item's current ray (the step needs them for wo, the
    // selected segment ray and the next ray; the lean instance parks no direction, and an instance overwrites kColdD
    // while a child tree is traversed) and the number of Intersect calls made for the item
    constexpr int kColdWalk = kColdBase + (INST ? 20 : 0);
    [[maybe_unused]] constexpr int kWalkD = kColdWalk, kWalkTime = kColdWalk + 3, kWalkTMax = kColdWalk + 4,
                                   kWalkCalls = kColdWalk + 5;
    constexpr int kColdFields = kColdWalk + (WALK ? 6 : 0);
    // The lean one-launch instances keep the four hit words in VGPRs (hit0 .. hit3) and have no cold state at all: the
    // LDS beside the stack windows goes to the block's top table: the scene's table (nnbvh_internal.h
    // kTopRecords), extended by the block itself from p.wide to top_lds_records(BT) records (load_top_table above).  A
    // lane whose `cur` carries kTopTag reads its record from there instead of from p.wide — the same bytes.  Tagged
    // references only come out of table records and the tagged root, and pass through the stack and its spill unchanged.
    constexpr bool kTop = kLean && MODEW == 3;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int gtid = blockIdx.x * BT + threadIdx.x;
    float(*stk)[2][64] = s_stack[wave];
    float(*cold)[64] = nullptr;
    [[maybe_unused]] const float4 *top = nullptr;
    if constexpr (kTop) {
        // (the alignment puts the table first in the block's LDS, ahead of the 64 KiB of stack windows: a record's four
        // ds_read_b128 then take the lane's byte offset as it is, with immediate offsets 0 .. 48)
        __shared__ __attribute__((aligned(1024))) float4 s_top[top_lds_records(BT) * 4];
        load_top_table<BT>(s_top, p.top, p.nTop, p.wide);
        top = s_top;
    } else {
        __shared__ float s_cold[BT / 64][kColdFields > 0 ? kColdFields : 1][64];
        cold = s_cold[wave];
    }
    [[maybe_unused]] float hit0 = 0.0f, hit1 = 0.0f, hit2 = 0.0f, hit3 = 0.0f;  // kTop: the current best hit
    int riReg = -1;  // lean instances: the ray this lane carries, -1 = none
    if (!kLean) cold[kColdRi][lane] = __int_as_float(-1);
    const long spillStride = (long)gridDim.x * BT;

    // which queue this wave drains first: its XCD's share of the batch (speed only)
    int q = 0;
    if (p.nQueues > 1) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        q = (int)(xcc & 0xf) % p.nQueues;
    }
    int queuesTried = 0;
    int curBatch = 0;  // MODE 3: the batch this wave is drawing rays from (wave-uniform)
    // batch size: the host's bound, or a device-resident queue size below it (wavefront callers)
    long nRays = p.n;
    if (p.nDev) {
        const long nd = (long)*p.nDev;
        nRays = nd < 0 ? 0 : (nd < nRays ? nd : nRays);
    }

#ifdef NNBVH_STATS
    // trips/lanes per kind (I, P, R); [6..8] = sum nInt,nPrim,nIdle over I trips; [10..12] = shader
    // cycles (s_memtime) spent in I / P / R trips incl. their scheduling decision; [14], [15] =
    // interior steps executed and the lanes that took part in them; [13] = those of the lanes whose record came from
    // the LDS top table (lean one-launch instances); [16], [17], [18] = table trips, the lanes that took part in them,
    // their shader cycles (not part of [13] .. [15])
    unsigned long long st[kSchedStatWords] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    unsigned long long stPrev = __builtin_amdgcn_s_memtime();
    int stKind = 2;
#endif
    RayState r;
    RayMasks masks = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull};  // lean instances: rebuilt after every refill trip
    float tMax = 0.0f;
    int visited = 0, tests = 0;
    int cur = kDone, sp = 0, base = 0;
    int floor = -1;      // INST: stack level the current child traversal must not pop below
    bool found = false;  // MODE 1/2
    bool exhausted = false;
    // kTop: the table-step threshold, read once and made opaque: left to itself the compiler re-reads p.topBurst from the
    // kernel arguments wherever it is compared (the SGPRs are full), and the wait for that scalar load is also a wait
    // for the LDS stack writes in flight
    [[maybe_unused]] int topBurst = 65;
    if constexpr (kTop) {
        topBurst = p.topBurst;
        asm volatile("" : "+s"(topBurst));
    }

    // pop entries until one whose deferred box test passes with the current tMax
    auto pop_entry = [&](int &ref, float &key) {
        --sp;
        ref = __float_as_int(stk[sp & (W - 1)][0][lane]);  // always an LDS read (stale if spilled)
        key = stk[sp & (W - 1)][1][lane];
        asm volatile("" : "+v"(ref), "+v"(key));  // keeps the two reads ds_read (no flat select)
        if (sp < base) {                     // rare: the entry lives in the HBM spill array
            const uint2 e = p.spill[(long)sp * spillStride + gtid];
            base = sp;
            ref = (int)e.x;
            key = __uint_as_float(e.y);
            // complete the load inside this rare branch, so that the common path's join
            // needs no vmcnt wait
            asm volatile("" : "+v"(ref), "+v"(key));
        }
        if (MODE != 2) visited += 1;
    };
    auto pop_next = [&]() -> int {
        const int lowest = (INST && floor > 0) ? floor : 0;
        const int none = (INST && floor >= 0) ? kReturn : kDone;
        if (sp <= lowest) return none;
        // the first entry is usually the one (only a tMax that shrank since the push rejects it)
        int ref;
        float key;
        pop_entry(ref, key);
        if (key < tMax) return ref;
        while (sp > lowest) {
            pop_entry(ref, key);
            if (key < tMax) return ref;
        }
        return none;
    };

    // TransformedPrimitive::Intersect / IntersectP (cpu/primitive.cpp:112-131): park the outer ray
    // in LDS, transform it into the instance's space, count and test the child root.
    auto enter_instance = [&](int slot, unsigned flags, float4 s0, float4 s1, float4 s2) {
        const float4 s3 = p.prims[slot + 3], s4 = p.prims[slot + 4], s5 = p.prims[slot + 5];
        const V3 dOuter = {cold[kColdD][lane], cold[kColdD + 1][lane], cold[kColdD + 2][lane]};
        cold[kSaveO][lane] = r.o.x;
        cold[kSaveO + 1][lane] = r.o.y;
        cold[kSaveO + 2][lane] = r.o.z;
        cold[kSaveInv][lane] = r.inv.x;
        cold[kSaveInv + 1][lane] = r.inv.y;
        cold[kSaveInv + 2][lane] = r.inv.z;
        cold[kSaveShear][lane] = r.sx;
        cold[kSaveShear + 1][lane] = r.sy;
        cold[kSaveShear + 2][lane] = r.sz;
        cold[kSaveKz][lane] = __int_as_float(r.kz);
        cold[kSaveTmax][lane] = tMax;
        cold[kSaveD][lane] = dOuter.x;
        cold[kSaveD + 1][lane] = dOuter.y;
        cold[kSaveD + 2][lane] = dOuter.z;
        cold[kResume][lane] = __int_as_float((flags & kPrimLast) ? kDone : ~(slot + 6));
        cold[kCurInst][lane] = __int_as_float(__float_as_int(s0.w) + 1);
        cold[kInnerHit][lane] = 0.0f;
        V3 oIn, dIn;
        float4 m0 = s2, m1 = s3, m2 = s4;
        if (INST == 2 && (flags & kPrimAnimated) && p.anim)  // AnimatedPrimitive: Interpolate(r.time), primitive.cpp:143-144
            anim_inverse_rows(p.anim + (long)kAnimStride * __float_as_int(s0.w), cold[kColdTime][lane], m0, m1, m2);
        apply_inverse_ray(m0, m1, m2, r.o, dOuter, tMax, oIn, dIn);
        r.o = oIn;
        cold[kColdD][lane] = dIn.x;
        cold[kColdD + 1][lane] = dIn.y;
        cold[kColdD + 2][lane] = dIn.z;
        r.inv = {1.0f / dIn.x, 1.0f / dIn.y, 1.0f / dIn.z};
        ray_shear(r, dIn);
        floor = sp;
        if (MODE != 2) visited += 1;  // the child aggregate's root
        float tEntry;
        const bool rootHit =
            slab_partial(s0.x, s0.y, s0.z, s1.x, s1.y, s1.z, r, tEntry) && (tEntry < tMax);
        cur = rootHit ? __float_as_int(s5.x) : kReturn;
    };

    // the child tree is exhausted: restore the outer ray; the inner tHit becomes the outer tMax
    // iff a hit was accepted inside (`si = primSi; tMax = si->tHit`), then resume the outer leaf
    auto leave_instance = [&]() {
        const bool innerHit = cold[kInnerHit][lane] != 0.0f;
        r.o = {cold[kSaveO][lane], cold[kSaveO + 1][lane], cold[kSaveO + 2][lane]};
        r.inv = {cold[kSaveInv][lane], cold[kSaveInv + 1][lane], cold[kSaveInv + 2][lane]};
        r.sx = cold[kSaveShear][lane];
        r.sy = cold[kSaveShear + 1][lane];
        r.sz = cold[kSaveShear + 2][lane];
        r.kz = __float_as_int(cold[kSaveKz][lane]);
        cold[kColdD][lane] = cold[kSaveD][lane];
        cold[kColdD + 1][lane] = cold[kSaveD + 1][lane];
        cold[kColdD + 2][lane] = cold[kSaveD + 2][lane];
        if (!innerHit) tMax = cold[kSaveTmax][lane];
        cold[kCurInst][lane] = 0.0f;
        floor = -1;
        const int resume = __float_as_int(cold[kResume][lane]);
        cur = (resume == kDone) ? pop_next() : resume;
    };

    // one primitive of the lane's leaf, its three slots s0..s2 in hand: the Primitive tag dispatch
    // (cpu/primitive.h), the leaf test, what a hit does, and where the lane goes next
    auto prim_math = [&](const int slot, const float4 s0, const float4 s1, const float4 s2) {
        const unsigned flags = __float_as_uint(s1.w);
        if (INST && (flags & kPrimInstance)) {
            if (INST == 2 && NNBVH_ANIM_ENTER_WEIGHT > 0 && (flags & kPrimAnimated) && p.anim) {
                // Interpolate(ray.time) costs ~600 instructions: the lane waits in the kEnter state until the
                // wave runs an ENTER step for all lanes that have reached an AnimatedPrimitive by then
                cold[kPendSlot][lane] = __int_as_float(slot);
                cur = kEnter;
            } else {
                enter_instance(slot, flags, s0, s1, s2);
            }
        } else if (!kLean && (flags & kPrimHost)) {
            // a primitive only the host can intersect (quadric, curve, alpha-tested
            // ...): this ray's result is void and the caller re-traces it on the CPU
            if constexpr (HOSTC) {
                // ... or, in candidate mode, the caller tests this primitive itself: list it (rare path: the
                // entries go straight to global memory) and walk on as if it were absent
                const int c = __float_as_int(cold[kColdHost][lane]);
                if (c >= 0) {  // -1 (overflow) and -2 (alpha re-trace) stay
                    long ray = __float_as_int(cold[kColdRi][lane]);
                    int cap = p.hcCap;
                    int32_t *hcPrim = p.hcPrim, *hcInst = p.hcInst;
                    if constexpr (MODE == 3) {  // the lane's batch has its own arrays
                        const int b = (int)(ray >> kFusedIndexBits);
                        ray &= (1 << kFusedIndexBits) - 1;
                        cap = pick_batch(p.bHcCap, b);
                        hcPrim = pick_batch(p.bHcPrim, b);
                        hcInst = pick_batch(p.bHcInst, b);
                    }
                    if (c < cap) {
                        const long at = ray * cap + c;
                        hcPrim[at] = __float_as_int(s0.w);
                        hcInst[at] = INST ? __float_as_int(cold[kCurInst][lane]) : 0;
                    }
                    cold[kColdHost][lane] = __int_as_float(c < cap ? c + 1 : -1);
                }
            } else {
                cold[kColdHost][lane] = 1.0f;
            }
            cur = (flags & kPrimLast) ? pop_next() : ~(slot + 3);
        } else {
            tests += 1;
            bool hit;
            float x0, x1, x2, th;
            int next;
            if (!PATCH || !(flags & kPrimPatch)) {
                hit = triangle_test(r, tMax, (flags & kPrimDegenerate) != 0,
                                    {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z},
                                    {s2.x, s2.y, s2.z}, x0, x1, x2, th, kLean ? &masks : nullptr);
                next = slot + ((ALPHA && (flags & kPrimSmooth)) ? 6 : 3);
                if constexpr (kAlphaTex) next += (flags & kPrimAlphaTex) ? 2 : 0;  // the (u, v) slots
                if (ALPHA && hit && (flags & kPrimAlpha)) {
                    // GeometricPrimitive::Intersect, cpu/primitive.cpp:57-70 (IntersectP takes
                    // the same route, :79-81): stochastic alpha test on the ray as given
                    [[maybe_unused]] float aTex = 0.0f;
                    if constexpr (kAlphaTex) {
                        // alpha.Evaluate(si->intr) of a FloatImageTexture: the (u, v) slots, the descriptor and the
                        // texels are read here, on a hit only, and are dead before the normals are fetched below
                        if (flags & kPrimAlphaTex) {
                            const float4 *uvp = p.prims + slot + ((flags & kPrimSmooth) ? 6 : 3);
                            const float4 uva = uvp[0], uvb = uvp[1];
                            const float4 *dp = p.alphaTex + 3 * (long)__float_as_int(s2.w);
                            const float4 d0 = dp[0], d1 = dp[1], d2 = dp[2];
                            const AlphaTexDesc desc = {__float_as_uint(d0.x), __float_as_uint(d0.y), __float_as_int(d0.z),
                                                       __float_as_int(d0.w), __float_as_int(d1.x), __float_as_int(d1.y),
                                                       d1.z, d1.w, d2.x, d2.y, d2.z, __float_as_int(d2.w)};
                            aTex = alpha_texture_eval(x0, x1, x2, uva.x, uva.y, uva.z, uva.w, uvb.x, uvb.y, desc,
                                                      p.alphaTexels);
                        }
                    }
                    const float a = (kAlphaTex && (flags & kPrimAlphaTex)) ? aTex : s2.w;
                    if (a < 1) {
                        const V3 rd = {cold[kColdD][lane], cold[kColdD + 1][lane],
                                       cold[kColdD + 2][lane]};
                        const float u = (a <= 0) ? 1.f : hash_float_6f(r.o, rd);
                        if (u > a) {
                            // ignored; the reference re-traces from the hit point against this
                            // shape alone: rNext = si->intr.SpawnRay(r.d), Intersect(rNext, tMax - tHit)
                            hit = false;
                            RayState rn = r;  // same direction: same reciprocals and shear
                            if (flags & kPrimSmooth) {  // a mesh with shading normals: offset along FaceForward(n, ns)
                                const float4 m0 = p.prims[slot + 3], m1 = p.prims[slot + 4], m2 = p.prims[slot + 5];
                                rn.o = alpha_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z}, x0,
                                                            x1, x2, (flags & kPrimFlipN) != 0, rd, true, {m0.x, m0.y, m0.z},
                                                            {m1.x, m1.y, m1.z}, {m2.x, m2.y, m2.z});
                            } else {
                                rn.o = alpha_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z},
                                                            {s2.x, s2.y, s2.z}, x0, x1, x2,
                                                            (flags & kPrimFlipN) != 0, rd);
                            }
                            tests += 1;  // Triangle::Intersect counts the re-test too
                            float y0, y1, y2, tn;
                            if (triangle_test(rn, tMax - th, (flags & kPrimDegenerate) != 0,
                                              {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z},
                                              {s2.x, s2.y, s2.z}, y0, y1, y2, tn))
                                cold[kColdHost][lane] = HOSTC ? __int_as_float(-2) : 1.0f;  // never for a planar
                                                               // triangle; if it happens the ray is the caller's
                        }
                    }
                }
            } else {
                const float4 s3 = p.prims[slot + 3];
                x2 = 0.0f;
                const V3 rd = {cold[PATCH ? kColdD : 0][lane], cold[PATCH ? kColdD + 1 : 0][lane],
                               cold[PATCH ? kColdD + 2 : 0][lane]};
                next = slot + 4 + ((ALPHA == 2 && (flags & kPrimSmooth)) ? 4 : 0) + ((ALPHA == 2 && (flags & kPrimUV)) ? 2 : 0);
                if constexpr (ALPHA == 2) {
                    // GeometricPrimitive::Intersect around a BilinearPatch (cpu/primitive.cpp:50-70).  A non-planar
                    // patch can be met again by the ray spawned off its own surface, so the recursion of :63-69 is
                    // followed: level k tests the ray of level k (its origin goes into the hash), up to
                    // kAlphaPatchDepth re-traces, beyond which the record is void (the caller re-traces the ray)
                    constexpr int kAlphaPatchDepth = 3;
                    const float a = (flags & kPrimAlpha) ? s2.w : 1.0f;
                    RayState rn = r;  // patch_test reads the origin only
                    float tm = tMax, t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                    int k = 0;
                    for (;;) {
                        hit = patch_test(rn, rd, tm, {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                         {s3.x, s3.y, s3.z}, x0, x1, th);
                        if (!hit || !(a < 1)) break;  // :52-54 / :58
                        const float u = (a <= 0) ? 1.f : hash_float_6f(rn.o, rd);
                        if (!(u > a)) break;  // accepted: (x0, x1, th) are this level's
                        if (k == kAlphaPatchDepth) {
                            hit = false;
                            cold[kColdHost][lane] = HOSTC ? __int_as_float(-2) : 1.0f;
                            break;
                        }
                        if (k == 0) t0 = th;
                        else if (k == 1) t1 = th;
                        else t2 = th;
                        ++k;
                        // rNext = si->intr.SpawnRay(r.d); Intersect(rNext, tMax - si->tHit)
                        rn.o = patch_retrace_origin({s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z}, {s2.x, s2.y, s2.z},
                                                    {s3.x, s3.y, s3.z}, x0, x1, (flags & kPrimFlipN) != 0, rd,
                                                    (flags & kPrimSmooth) != 0, (flags & kPrimUV) != 0,
                                                    p.prims + slot + 4);
                        tm = tm - th;
                        tests += 1;
                    }
                    if (hit && k > 0) {  // siNext->tHit += si->tHit (:67-68), unwinding from the deepest level
                        if (k == 3) th = th + t2;
                        if (k >= 2) th = th + t1;
                        th = th + t0;
                    }
                } else {
                    hit = patch_test(r, rd, tMax, {s0.x, s0.y, s0.z}, {s1.x, s1.y, s1.z},
                                     {s2.x, s2.y, s2.z}, {s3.x, s3.y, s3.z}, x0, x1, th);
                }
            }
            bool closestLane = MODE == 0;
            if (MODE == 3 && hit)
                closestLane = !((p.anyMask >> ((kLean ? riReg : __float_as_int(cold[kColdRi][lane])) >> kFusedIndexBits)) & 1u);
            if (hit) {
                if (closestLane) {
                    if constexpr (kTop) {
                        hit0 = s0.w;
                        hit1 = x0;
                        hit2 = x1;
                        hit3 = x2;
                    } else {
                        cold[kColdHit][lane] = s0.w;  // primitive id bits
                        cold[kColdHit + 1][lane] = x0;
                        cold[kColdHit + 2][lane] = x1;
                        cold[kColdHit + 3][lane] = x2;
                    }
                    tMax = th;
                    if (INST) {
                        cold[kHitInst][lane] = cold[kCurInst][lane];
                        cold[kInnerHit][lane] = 1.0f;
                    }
                    if constexpr (HOSTC && MODE == 0) {  // the candidates met before this hit (the last store wins)
                        const int c = __float_as_int(cold[kColdHost][lane]);
                        if (c > 0) p.hcBefore[__float_as_int(cold[kColdRi][lane])] = c;
                    }
                    if constexpr (HOSTC && MODE == 3) {  // c > 0 only in a batch with candidate arrays
                        const int c = __float_as_int(cold[kColdHost][lane]);
                        if (c > 0) {
                            const int tag = __float_as_int(cold[kColdRi][lane]);
                            pick_batch(p.bHcBefore, tag >> kFusedIndexBits)[tag & ((1 << kFusedIndexBits) - 1)] = c;
                        }
                    }
                } else {
                    found = true;
                }
            }
            if (MODE != 0 && found) cur = kDone;           // aggregates.cpp:597-602
            else if (flags & kPrimLast) cur = pop_next();  // leaf finished
            else cur = ~next;
        }
    };

    // one interior record q0..q3 in hand: both children's slab keys, the far child pushed with its key,
    // the near child entered (aggregates.cpp:556-574)
    auto interior_math = [&](const float4 q0, const float4 q1, const float4 q2, const float4 q3) {
        const int ref0 = __float_as_int(q3.x), ref1 = __float_as_int(q3.y);
        const int axis = __float_as_int(q3.z);
        // aggregates.cpp:562-568: near child = second child iff dirIsNeg[axis]
        const bool swap = ((r.kz >> axis) & 1) != 0;  // dirIsNeg[axis], packed by ray_shear
        // one float per child: its entry distance, +inf if the box is missed whatever tMax is
        // (slab_entry_key) — the verdicts are then two compares against tMax
        const float k0 = kLean ? slab_entry_key(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r, masks)
                               : slab_entry_key(q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, r);
        const float k1 = kLean ? slab_entry_key(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r, masks)
                               : slab_entry_key(q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, r);
        const int nearRef = swap ? ref1 : ref0, farRef = swap ? ref0 : ref1;
        const float nearT = swap ? k1 : k0, farT = swap ? k0 : k1;
        visited += 1;  // the near child is entered now
        // A far child whose tMax-independent tests failed (key +inf) can never be entered: it is
        // counted now and not pushed.  One that merely fails against TODAY's tMax must be pushed:
        // tMax is not monotone — a hit accepted with tScaled <= tMax * det can round to a t one ulp
        // ABOVE the old tMax (shapes.cpp:239-244; rays that meet a shared vertex at exactly tMax do
        // it), and the reference tests the far child against that later value.  MODE 1 pushes every
        // far child (exact counts up to the first hit).
        const bool doPush = (MODE == 1) || (farT < __builtin_inff());
        if (doPush && sp - base == W - 1) {  // the window is full: its oldest entry goes to the HBM spill array
            uint2 e;
            e.x = __float_as_uint(stk[base & (W - 1)][0][lane]);
            e.y = __float_as_uint(stk[base & (W - 1)][1][lane]);
            p.spill[(long)base * spillStride + gtid] = e;
            ++base;
        }
        stk[sp & (W - 1)][0][lane] = __int_as_float(farRef);
        stk[sp & (W - 1)][1][lane] = farT;
        sp += doPush ? 1 : 0;
        if (MODE == 0 || MODE == 3) visited += doPush ? 0 : 1;
        cur = nearT < tMax ? nearRef : pop_next();
    };
    auto interior_step = [&]() {
#ifdef NNBVH_STATS
        st[14] += 1;
        st[15] += __popcll(__ballot(cur >= 0));
        if (kTop) st[13] += __popcll(__ballot(cur >= 0 && (cur & kTopTag) != 0));  // ... of them, served from the top table
#endif
        if constexpr (kTop) {
            // a tagged lane reads the byte copy of its record from the block's table (slot = cur without the tag: the
            // shift drops bit 30), the others load from p.wide; both join before the arithmetic.  One asm block holds
            // both load groups, each under its lanes' exec mask, and one wait for both: the two sources write the same
            // sixteen VGPRs in disjoint lanes, and written as two branches the compiler orders them, so that every
            // mixed wave-step paid an LDS round trip (s_waitcnt lgkmcnt(0)) before its global loads were issued
            // (profiles/top_table_255.txt).  The word with the references and the axis is asked for first, as before.
            // (top's LDS address is the low half of its flat one)
            if (cur >= 0) {
                typedef float v4f __attribute__((ext_vector_type(4)));
                const unsigned at = (unsigned)cur << 6;
                v4f q0, q1, q2, q3;
                const unsigned long long tagged = __ballot((cur & kTopTag) != 0);
                const unsigned ldsAt = at + (unsigned)reinterpret_cast<uintptr_t>(top);
                unsigned long long active;
                asm volatile(
                    "s_mov_b64 %[act], exec\n\t"
                    "s_andn2_b64 exec, exec, %[tag]\n\t"
                    "s_cbranch_execz 1f\n\t"
                    "global_load_dwordx4 %[q3], %[at], %[wide] offset:48\n\t"
                    "global_load_dwordx4 %[q0], %[at], %[wide]\n\t"
                    "global_load_dwordx4 %[q1], %[at], %[wide] offset:16\n\t"
                    "global_load_dwordx4 %[q2], %[at], %[wide] offset:32\n"
                    "1:\n\t"
                    "s_and_b64 exec, %[act], %[tag]\n\t"
                    "s_cbranch_execz 2f\n\t"
                    "ds_read_b128 %[q3], %[lds] offset:48\n\t"
                    "ds_read_b128 %[q0], %[lds]\n\t"
                    "ds_read_b128 %[q1], %[lds] offset:16\n\t"
                    "ds_read_b128 %[q2], %[lds] offset:32\n"
                    "2:\n\t"
                    "s_mov_b64 exec, %[act]\n\t"
                    "s_waitcnt vmcnt(0) lgkmcnt(0)"
                    : [q0] "=&v"(q0), [q1] "=&v"(q1), [q2] "=&v"(q2), [q3] "=&v"(q3), [act] "=&s"(active)
                    : [at] "v"(at), [lds] "v"(ldsAt), [wide] "s"(p.wide), [tag] "s"(tagged)
                    : "scc");
                interior_math({q0.x, q0.y, q0.z, q0.w}, {q1.x, q1.y, q1.z, q1.w}, {q2.x, q2.y, q2.z, q2.w},
                              {q3.x, q3.y, q3.z, q3.w});
            }
        } else if (cur >= 0) {
            // lean instances address records and slots with a 32-bit byte offset from a scalar base (one
            // 32-bit shift instead of a 64-bit shift and a 64-bit add per fetch); the launcher only picks
            // them when both arrays are below 4 GiB (p.fits32)
            const float4 *rec = kLean ? reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(p.wide) + ((unsigned)cur << 6))
                                      : p.wide + 4 * (long)cur;
            const float4 q3 = rec[3];
            const float4 q0 = rec[0], q1 = rec[1], q2 = rec[2];
            interior_math(q0, q1, q2, q3);
        }
    };
    // the table step (kTop): the LDS block of interior_step alone, for the lanes at a tagged record.  No global load is
    // issued and none is waited for (the spill store of a full window and the spill re-load of a pop complete inside
    // their own branches)
    [[maybe_unused]] auto table_step = [&]() {
        if (((unsigned)cur >> 30) == 1u) {  // cur >= 0 && (cur & kTopTag)
            typedef float v4f __attribute__((ext_vector_type(4)));
            const v4f *rec = reinterpret_cast<const v4f *>(reinterpret_cast<const char *>(top) + ((unsigned)cur << 6));
            const v4f q3 = rec[3];
            const v4f q0 = rec[0], q1 = rec[1], q2 = rec[2];
            interior_math({q0.x, q0.y, q0.z, q0.w}, {q1.x, q1.y, q1.z, q1.w}, {q2.x, q2.y, q2.z, q2.w},
                          {q3.x, q3.y, q3.z, q3.w});
        }
    };

    for (;;) {
#ifdef NNBVH_STATS
        {
            const unsigned long long now = __builtin_amdgcn_s_memtime();
            st[10 + stKind] += now - stPrev;
            stPrev = now;
        }
#endif
        const bool isInt = cur >= 0;
        const bool isIdle = cur == kDone;
        const int nInt = __popcll(__ballot(isInt));
        const unsigned long long idleMask = __ballot(isIdle);
        const int nIdle = __popcll(idleMask);
        const int nEnter = (INST == 2 && NNBVH_ANIM_ENTER_WEIGHT > 0) ? __popcll(__ballot(cur == kEnter)) : 0;
        const int nPrim = 64 - nInt - nIdle - nEnter;

        // Wave-uniform choice of this trip's step kind: the one that advances the most lanes
        // per instruction issued.  A lane's weight says how cheap its step is relative to an
        // interior step (weight 16): primitive tests and refills are longer, so they must
        // gather more lanes before they are worth a trip.  All-idle always refills/retires.
        const int sI = nInt * 16, sP = nPrim * p.primWeight;
        const int sR = exhausted ? 0 : nIdle * p.refillWeight;
#ifdef NNBVH_STATS
        unsigned long long &stTrips = (nIdle == 64 || (sR > sI && sR > sP)) ? st[4]
                                      : ((sP > sI || nInt == 0) ? st[2] : st[0]);
        (&stTrips)[0] += 1;
        (&stTrips)[1] += (nIdle == 64 || (sR > sI && sR > sP)) ? nIdle
                         : ((sP > sI || nInt == 0) ? nPrim : nInt);
        stKind = (&stTrips == &st[4]) ? 2 : ((&stTrips == &st[2]) ? 1 : 0);
        if (&stTrips == &st[0]) {
            st[6] += nInt;
            st[7] += nPrim;
            st[8] += nIdle;
        }
#endif
        if (nIdle == 64 || (sR > sI && sR > sP)) {
            // ---- retire finished rays, refill idle lanes -------------------------------
            const int ri = isIdle ? (kLean ? riReg : __float_as_int(cold[kColdRi][lane])) : -1;
            // WALK: the lane's item walks on from nextO in direction nextD / would start call walk.maxSurfaces + 1
            [[maybe_unused]] bool goOn = false, capped = false;
            [[maybe_unused]] V3 nextO = {0.0f, 0.0f, 0.0f}, nextD = {0.0f, 0.0f, 0.0f};
            [[maybe_unused]] float nextTMax = 1.0f, nextTime = 0.0f;  // aggregate.Intersect(r, 1), time 0: WALK 2
            if constexpr (WALK != 0) {
                if (ri >= 0) {
                    // one step of the walk for item ri, on the hit record a MODE 0 lane would store (counters, instance
                    // word and the "void" rule for host-only primitives included) and the record of the lane's ray
                    const float4 r0 = {r.o.x, r.o.y, r.o.z, cold[kWalkTMax][lane]};
                    const float4 r1 = {cold[kWalkD][lane], cold[kWalkD + 1][lane], cold[kWalkD + 2][lane],
                                       cold[kWalkTime][lane]};
                    const float4 h0 = {cold[kColdHit][lane], tMax, cold[kColdHit + 1][lane], cold[kColdHit + 2][lane]};
                    float4 h1 = {cold[kColdHit + 3][lane], __int_as_float(visited), __int_as_float(tests),
                                 INST ? cold[kHitInst][lane] : 0.0f};
                    if (!kLean && p.hasHostPrims && cold[kColdHost][lane] != 0.0f) h1.w = __int_as_float(-1);
                    const ShadingMeshDevice &sm = p.wMesh;
                    const MeshView wm = {sm.verts, sm.triVerts, sm.patchVerts, sm.normals, sm.uvs, sm.tangents,
                                         sm.faceIndices, sm.triFlags, sm.nTris, sm.defaultFlags, sm.instances,
                                         sm.nInstances, sm.anim, sm.animFwd};
                    if constexpr (WALK == 1) {
                        goOn = w2_str_item<PATCH != 0>(wm, r0, r1, h0, h1, ri, p.walk.primClass, p.walk.nPrimClass,
                                                       p.walk.pLight, p.walk.state, nextO, nextD);
                        nextTMax = r0.w;  // tMax is the work item's, unchanged (intersect.h:175, :187)
                        nextTime = r1.w;
                        // the spawned ray has a zero direction: the walk ends, the ray arrives (state stays 0)
                        if (goOn && nextD.x == 0.0f && nextD.y == 0.0f && nextD.z == 0.0f) goOn = false;
                    } else {
                        goOn = w2_or_item<PATCH != 0>(wm, r0, r1, h0, h1, ri, p.walk.p1, p.walk.material,
                                                      p.walk.primMaterial, p.walk.nPrimMaterial, p.walk.st,
                                                      p.walk.selHits, p.walk.selRays, nextO, nextD);
                    }
                    if (goOn) {
                        const int calls = __float_as_int(cold[kWalkCalls][lane]);
                        if (calls >= p.walk.maxSurfaces) {  // the caller's to finish, as w2_mark_unfinished marks it
                            goOn = false;
                            capped = true;
                            if constexpr (WALK == 1) p.walk.state[ri] = 2;
                            else p.walk.selHits[2 * (long)ri + 1].w = __int_as_float(-1);
                        } else {
                            cold[kWalkCalls][lane] = __int_as_float(calls + 1);
                        }
                    }
                }
            } else if constexpr (MODE == 3 && HOSTC) {
                // candidate mode of the one-launch kernel, a block of its own so that the plain instances' retire
                // below stays as it is: the count goes to the batch's array; an any-hit ray is the caller's (2) when
                // it met a host-only primitive, a closest-hit record is void only for count < 0
                if (ri >= 0) {
                    const int b = ri >> kFusedIndexBits;
                    const long idx = ri & ((1 << kFusedIndexBits) - 1);
                    void *outp = pick_batch(p.bOut, b);
                    const int c = __float_as_int(cold[kColdHost][lane]);
                    if (pick_batch(p.bHcCap, b) > 0) pick_batch(p.bHcCount, b)[idx] = c;
                    if ((p.anyMask >> b) & 1u) {
                        store_stream(reinterpret_cast<uint8_t *>(outp) + idx, (uint8_t)(found ? 1 : (c != 0 ? 2 : 0)));
                    } else {
                        float4 h0, h1;
                        h0.x = cold[kColdHit][lane];
                        h0.y = tMax;
                        h0.z = cold[kColdHit + 1][lane];
                        h0.w = cold[kColdHit + 2][lane];
                        h1.x = cold[kColdHit + 3][lane];
                        h1.y = __int_as_float(visited);
                        h1.z = __int_as_float(tests);
                        h1.w = INST ? cold[kHitInst][lane] : 0.0f;
                        if (c < 0) h1.w = __int_as_float(-1);
                        float4 *out = reinterpret_cast<float4 *>(outp) + 2 * idx;
                        store_stream(out, h0);
                        store_stream(out + 1, h1);
                    }
                }
            } else if (MODE == 3 && ri >= 0) {
                const int b = ri >> kFusedIndexBits;
                const long idx = ri & ((1 << kFusedIndexBits) - 1);
                void *outp = b == 0 ? p.bOut[0] : (b == 1 ? p.bOut[1] : (b == 2 ? p.bOut[2] : p.bOut[3]));
                const bool needHost = !kLean && p.hasHostPrims && cold[kColdHost][lane] != 0.0f;
                if ((p.anyMask >> b) & 1u) {
                    store_stream(reinterpret_cast<uint8_t *>(outp) + idx, (uint8_t)(found ? 1 : (needHost ? 2 : 0)));
                } else {
                    float4 h0, h1;
                    h0.x = kTop ? hit0 : cold[kColdHit][lane];
                    h0.y = tMax;
                    h0.z = kTop ? hit1 : cold[kColdHit + 1][lane];
                    h0.w = kTop ? hit2 : cold[kColdHit + 2][lane];
                    h1.x = kTop ? hit3 : cold[kColdHit + 3][lane];
                    h1.y = __int_as_float(visited);
                    h1.z = __int_as_float(tests);
                    h1.w = INST ? cold[kHitInst][lane] : 0.0f;
                    if (needHost) h1.w = __int_as_float(-1);
                    float4 *out = reinterpret_cast<float4 *>(outp) + 2 * idx;
                    store_stream(out, h0);
                    store_stream(out + 1, h1);
                }
            } else if (ri >= 0) {
                if (MODE == 0) {
                    float4 h0, h1;
                    h0.x = cold[kColdHit][lane];  // hit primitive id (bit pattern)
                    h0.y = tMax;
                    h0.z = cold[kColdHit + 1][lane];
                    h0.w = cold[kColdHit + 2][lane];
                    h1.x = cold[kColdHit + 3][lane];
                    h1.y = __int_as_float(visited);
                    h1.z = __int_as_float(tests);
                    h1.w = INST ? cold[kHitInst][lane] : 0.0f;  // 0 / instance index + 1 (bit pattern)
                    if constexpr (HOSTC) {
                        const int c = __float_as_int(cold[kColdHost][lane]);
                        if (c < 0) h1.w = __int_as_float(-1);
                        p.hcCount[ri] = c;
                    } else if (!kLean && p.hasHostPrims && cold[kColdHost][lane] != 0.0f) {
                        h1.w = __int_as_float(-1);
                    }
                    float4 *out = reinterpret_cast<float4 *>(p.hits) + 2 * (long)ri;
                    store_stream(out, h0);
                    store_stream(out + 1, h1);
                } else {
                    bool needHost;
                    if constexpr (HOSTC) {
                        const int c = __float_as_int(cold[kColdHost][lane]);
                        needHost = c != 0;
                        p.hcCount[ri] = c;
                    } else {
                        needHost = !kLean && p.hasHostPrims && cold[kColdHost][lane] != 0.0f;
                    }
                    store_stream(&p.occluded[ri], (uint8_t)(found ? 1 : (needHost ? 2 : 0)));
                    if (MODE == 1) {
                        if (p.visitedOut) store_stream(&p.visitedOut[ri], (int32_t)visited);
                        if (p.testsOut) store_stream(&p.testsOut[ri], (int32_t)tests);
                    }
                }
            }
            int newRi = -1;  // n < 2^31 is enforced by the ABI
            // the lanes that take a new ray, their number and mask: the idle ones, less (WALK) those that walk on
            bool takes = isIdle;
            unsigned long long takeMask = idleMask;
            int nTake = nIdle;
            if constexpr (WALK != 0) {
                const unsigned long long cm = __ballot(capped);
                if (p.walk.unfinished && cm != 0ull && lane == __ffsll((long long)cm) - 1)
                    atomicAdd(p.walk.unfinished, __popcll(cm));
                if (goOn) {  // same item, same lane: the ray index stays
                    const float4 a = {nextO.x, nextO.y, nextO.z, nextTMax}, b = {nextD.x, nextD.y, nextD.z, nextTime};
                    BVH_BEGIN_RAY(a, b);
                }
                takes = isIdle && !goOn;
                takeMask = __ballot(takes);
                nTake = __popcll(takeMask);
                if (exhausted) {  // every lane was idle: the wave ends when none of them walks on
                    if (nTake == 64) break;
                    if (takes) {  // retired: the step must not run on it again
                        if (kLean) riReg = -1;
                        else cold[kColdRi][lane] = __int_as_float(-1);
                    }
                    if (kLean) masks = ray_masks(r);  // some lanes carry new rays
                    continue;
                }
            } else {
                if (exhausted) break;  // only reached with every lane idle (sR == 0 otherwise)
            }
            long start = 0;
            for (;;) {  // find a queue with work left (own XCD's first, then steal)
                if constexpr (WALK != 0) {
                    if (nTake == 0) break;  // every idle lane walks on: nothing is drawn
                }
                if (MODE == 3) {
                    nRays = p.bN[curBatch];
                    if (const int32_t *nd = p.bNDev[curBatch]) {  // wavefront queues: the size lives on the device
                        const long v = *nd;
                        nRays = v < 0 ? 0 : (v < nRays ? v : nRays);
                    }
                }
                // p.nQueues is 1 or kMaxQueues = 8: the division of a long is a shift (the scalar unit has
                // no 64-bit divide; the compiler's expansion was ~250 instructions per refill)
                static_assert(kMaxQueues == 8, "queue ranges are computed with a shift by 3");
                const int qShift = p.nQueues > 1 ? 3 : 0;
                const long qBegin = (nRays * q) >> qShift, qEnd = (nRays * (q + 1)) >> qShift;
                unsigned got = 0;
                if (lane == 0)
                    got = atomicAdd(&p.queue[((MODE == 3 ? curBatch * p.nQueues : 0) + q) * kQueueStrideWords],
                                    (unsigned)nTake);
                got = __builtin_amdgcn_readfirstlane(got);
                start = qBegin + (long)got;
                if (start < qEnd) {
                    const int rank = __builtin_amdgcn_mbcnt_hi(
                        (unsigned)(takeMask >> 32),
                        __builtin_amdgcn_mbcnt_lo((unsigned)takeMask, 0u));
                    if (takes && start + rank < qEnd) newRi = (int)(start + rank);
                    break;
                }
                if (++queuesTried >= p.nQueues) {
                    if (MODE == 3 && curBatch + 1 < p.nBatches) {  // this batch is handed out: on to the next
                        ++curBatch;
                        queuesTried = 0;
                        continue;
                    }
                    exhausted = true;
                    break;
                }
                q = (q + 1 == p.nQueues) ? 0 : q + 1;
            }
            if (takes) {
                const int tag = (MODE == 3 && newRi >= 0) ? (newRi | (curBatch << kFusedIndexBits)) : newRi;
                if (kLean) riReg = tag;
                else cold[kColdRi][lane] = __int_as_float(tag);
            }
            if (newRi >= 0) {
                const nnbvh_ray *batchRays = MODE == 3 ? p.bRays[curBatch] : p.rays;
                float4 r0, r1;
                if (!SOA || batchRays) {
                    const float4 *in = reinterpret_cast<const float4 *>(batchRays) + 2 * (long)newRi;
                    r0 = load_stream(in);
                    r1 = load_stream(in + 1);
                } else {  // a wavefront queue: SOA<Ray> slices (wavefront/workitems.soa:40-50)
                    const nnbvh_ray_soa &q = MODE == 3 ? p.bSoa[curBatch] : p.soa;
                    auto ld = [&](const float *a) { return load_stream(a + newRi); };
                    r0 = {ld(q.ox), ld(q.oy), ld(q.oz), q.tmax ? ld(q.tmax) : __builtin_inff()};
                    r1 = {ld(q.dx), ld(q.dy), ld(q.dz), q.time ? ld(q.time) : 0.0f};
                }
                if constexpr (WALK != 0) {
                    // `while (ray.d != Vector3f(0, 0, 0))`, intersect.h:183 / aggregate.cpp:100: a zero direction makes
                    // no Intersect call — the item is finished as the init kernel left it, the lane stays idle
                    if (r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f) {
                        if (kLean) riReg = -1;
                        else cold[kColdRi][lane] = __int_as_float(-1);
                    } else {
                        cold[kWalkCalls][lane] = __int_as_float(1);
                        BVH_BEGIN_RAY(r0, r1);
                    }
                } else {
                    BVH_BEGIN_RAY(r0, r1);
                }
            }
            if (kLean) masks = ray_masks(r);  // some lanes carry new rays
            continue;
        }

        if (INST == 2 && NNBVH_ANIM_ENTER_WEIGHT > 0 && nEnter > 0 &&
            ((nInt == 0 && nPrim == 0) || (nEnter * NNBVH_ANIM_ENTER_WEIGHT > sI && nEnter * NNBVH_ANIM_ENTER_WEIGHT > sP))) {
            // ---- enter step: every lane waiting at an AnimatedPrimitive enters it now -------------------
            if (cur == kEnter) {
                const int slot = __float_as_int(cold[kPendSlot][lane]);
                const float4 s0 = p.prims[slot], s1 = p.prims[slot + 1], s2 = p.prims[slot + 2];
                enter_instance(slot, __float_as_uint(s1.w), s0, s1, s2);
            }
            continue;
        }

        if (sP > sI || nInt == 0) {
            // ---- primitive step: lanes with a pending leaf test ONE primitive -----------
            // (up to p.primRepeat of them per scheduling decision: lanes whose leaf is finished sit the
            // rest out, lanes still inside theirs go on without another round of ballots)
            // (the one-launch kernel keeps ONE: compiled in, the loop costs it 6 registers — spills at 8
            // wavefronts per SIMD — and 2.6 % of its rate)
            const int nPrep = (MODE == 3) ? 1 : p.primRepeat;
            int prep = 0;
            do {
            if (cur < 0 && cur != kDone) {
                if (INST && cur == kReturn) leave_instance();
                if (cur < 0 && cur != kDone && cur != kReturn && (INST != 2 || cur != kEnter)) {
                    const int slot = ~cur;
                    const float4 *pr = kLean ? reinterpret_cast<const float4 *>(reinterpret_cast<const char *>(p.prims) + ((unsigned)slot << 4))
                                             : p.prims + slot;
                    float4 s0 = pr[0], s1 = pr[1], s2 = pr[2];
                    // all three slots are fetched before anything looks at the flags: left alone the compiler
                    // loads the flag word first and the vertices only inside the not-degenerate branch, two
                    // dependent trips to memory per primitive
                    asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s0.z), "+v"(s0.w), "+v"(s1.x), "+v"(s1.y),
                                      "+v"(s1.z), "+v"(s1.w), "+v"(s2.x), "+v"(s2.y), "+v"(s2.z), "+v"(s2.w));
                    prim_math(slot, s0, s1, s2);
                }
            }
            } while (++prep < nPrep && __ballot(cur < 0 && cur != kDone) != 0ull);
        } else {
            // ---- interior step(s): up to p.intRepeat in a row before the next scheduling
            // decision (lanes that leave the interior state sit the remaining ones out) -------
            if (MODE == 3) {
                if constexpr (kTop) {
                    // ---- table step(s): an interior trip of a wave with at least p.topBurst lanes at a record of the
                    // LDS table begins with steps for those lanes alone, on one ballot each, until fewer are left (they
                    // ride along in the ordinary steps below).  After a refill the new rays so walk down the top levels
                    // at the refill's lane count and without a global round trip.  (p.topBurst > 64: never)
#ifdef NNBVH_STATS
                    unsigned long long stT0 = 0;  // (read only when a table step runs: s_memtime is not free)
                    bool stTable = false;
#endif
                    for (;;) {
                        const int nTag = __popcll(__ballot(((unsigned)cur >> 30) == 1u));
                        if (nTag < topBurst) break;
#ifdef NNBVH_STATS
                        if (!stTable) stT0 = __builtin_amdgcn_s_memtime();
                        stTable = true;
                        st[16] += 1;
                        st[17] += nTag;
#endif
                        table_step();
                    }
#ifdef NNBVH_STATS
                    if (stTable) {
                        const unsigned long long stT1 = __builtin_amdgcn_s_memtime();
                        st[18] += stT1 - stT0;
                        stPrev += stT1 - stT0;  // ... which are not the interior trip's
                    }
#endif
                }
                // the one-launch kernel: the first three steps (the default int_repeat) written out, no trip
                // counter to maintain (+0.8 %; the separate-launch kernels lose 1.8 % with it and keep the loop)
                interior_step();
                if (p.intRepeat > 1 && __ballot(cur >= 0) != 0ull) {
                    interior_step();
                    if (p.intRepeat > 2 && __ballot(cur >= 0) != 0ull) {
                        interior_step();
                        for (int rep = 3; rep < p.intRepeat && __ballot(cur >= 0) != 0ull; ++rep) interior_step();
                    }
                }
            } else {
            int rep = 0;
            do {
                interior_step();
            } while (++rep < p.intRepeat && __ballot(cur >= 0) != 0ull);
            }
        }
    }
#ifdef NNBVH_STATS
    if (lane == 0 && p.stats)
        for (int k = 0; k < kSchedStatWords; ++k) atomicAdd(&p.stats[k], st[k]);
#endif
}
#undef BVH_BEGIN_RAY

// The queue heads are cleared by a (tiny) kernel rather than hipMemsetAsync: as a kernel node the
// clear keeps its place between the launches of a captured hipGraph.
__global__ void zero_queue_kernel(unsigned *queue, int words) {
    for (int i = threadIdx.x; i < words; i += blockDim.x) queue[i] = 0u;
}
hipError_t launch_zero_queue(unsigned *queue, int words, hipStream_t stream) {
    hipLaunchKernelGGL(zero_queue_kernel, dim3(1), dim3(256), 0, stream, queue, words);
    return hipGetLastError();
}

__global__ void zero_words_kernel(int32_t *words, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) words[i] = 0;
}
hipError_t launch_zero_words(int32_t *words, long n, int maxBlocks, hipStream_t stream) {
    long blocks = (n + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks < maxBlocks ? blocks : maxBlocks);
    hipLaunchKernelGGL(zero_words_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, words, n);
    return hipGetLastError();
}

// ---- the instances: one kernel per entry of kTraceInstances (trace_instance.h), in its order -----------------------
struct TraceEntry {
    TraceInstance is;
    void (*kernel)(TraceParams);
};
template <size_t I>
constexpr TraceEntry trace_entry() {
    constexpr TraceInstance t = kTraceInstances[I];
    return {t, trace_kernel<t.mode, t.window, t.inst, t.patch, t.alpha, t.soa, t.hostc>};
}
template <size_t... I>
constexpr std::array<TraceEntry, sizeof...(I)> trace_table(std::index_sequence<I...>) {
    return {{trace_entry<I>()...}};
}
static const auto kTraceTable = trace_table(std::make_index_sequence<std::size(kTraceInstances)>());

// the launch ledger: one count per entry of kTraceInstances, in its order
static LaunchLedger<(int)std::size(kTraceInstances)> g_trace_ledger;

hipError_t launch_trace(const TraceInstance &is, const TraceParams &p, int blocks, hipStream_t stream, int *occupancy) {
    for (size_t i = 0; i < kTraceTable.size(); ++i) {
        const TraceEntry &e = kTraceTable[i];
        if (std::memcmp(&e.is, &is, sizeof is) != 0) continue;
        const int threads = trace_block_threads(is);
        if (occupancy) return hipOccupancyMaxActiveBlocksPerMultiprocessor(occupancy, e.kernel, threads, 0);
        hipLaunchKernelGGL(e.kernel, dim3((unsigned)blocks), dim3(threads), 0, stream, p);
        g_trace_ledger.count((int)i);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

int trace_instance_launches(int32_t *desc, uint64_t *counts, int capacity, int reset) {
    return g_trace_ledger.read(desc, counts, capacity, reset, [](int i) {
        const TraceInstance &t = kTraceInstances[i];
        return std::array<int32_t, 7>{{t.mode, t.window, t.inst, t.patch, t.alpha, t.soa, t.hostc}};
    });
}

}  // namespace nnbvh
