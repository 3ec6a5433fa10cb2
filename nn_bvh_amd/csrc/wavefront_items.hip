// wavefront_items.hip — WavefrontAggregate::IntersectClosest's enqueue with the work items themselves
// (/root/reference/src/pbrt/wavefront/intersect.h:16-156): for every item the reference's routing, and
// for every item bound to a queue that carries geometry the SurfaceInteraction (interaction_math.h, the
// same bits as the post-pass of interaction.hip), stored as SOA slices at the item's pushed slot
// (MaterialEvalWorkItem, HitAreaLightWorkItem, MediumSampleWorkItem, the spawned ray of an interface
// surface: wavefront/workitems.soa:63-75, 118-141, 156-174).
//
// Structure of wf_enqueue_closest (wavefront.hip): a block classifies a chunk of items, reserves each
// destination range with ONE atomicAdd per queue and chunk, then pushes.  The chunk is 256 threads x 4
// items (not x 16): the interaction needs its ~100 registers for ONE item at a time, so the chunk's hit
// records are parked in LDS (32 KB per block) between the classify and the push pass instead of in
// registers, and the push pass loops over them without unrolling the interaction four times.  Each hit
// record is read from memory once; the interaction runs only for the items whose queue stores geometry.
#include <hip/hip_runtime.h>

#include "interaction_math.h"
#include "spawn_math.h"
#include "wavefront_items.h"

namespace nnbvh {

static constexpr int kItBlock = 256;
static constexpr int kItItems = 4;                    // items per thread and chunk
static constexpr int kItChunk = kItBlock * kItItems;  // 1024 items per block iteration
static constexpr int kItQueues = 7;                   // the six of nnbvh_closest_queues + needs_host
static constexpr int kItBits = 7;                     // destination bits per item, kItItems of them in one word
enum : unsigned {
    kIEscaped = 1, kIAreaLight = 2, kIBasic = 4, kIUniversal = 8, kIMedium = 16, kINext = 32, kIHost = 64
};

struct ItemsParams {
    MeshView m;
    const float4 *hits;
    WavefrontCount cnt;
    nnbvh_ray_soa soa;
    const uint8_t *primClass;
    long nPrimClass;
    nnbvh_closest_queues out;
    nnbvh_closest_items items;
    // the EXT instances only (at the end: the other instances read nothing behind `items`)
    const int32_t *hcCount;  // nullable, per ray: != 0 = the ray has host candidates (or is void): needs_host only
    const int32_t *index;    // nullable: the items are rays index[0 .. n) instead of 0 .. n (cnt counts the list)
    int maxRays;             // rays the hit records / the ray queue hold: list entries outside [0, maxRays) are skipped
};

// intersect.h:19-29 (miss) and :56-128 (hit), plus the two cases the device cannot finish: a voided
// record (a host-only primitive lies on the ray) and a hit whose interaction the mesh cannot compute
template <bool FULL>
__device__ __forceinline__ unsigned item_destinations(const MeshView &m, int prim, int inst, bool medium,
                                                      unsigned cls) {
    if (inst == -1) return kIHost;
    if (prim >= 0 && imath::interaction_status<FULL>(m, prim, inst) == NNBVH_INTERACTION_HOST) return kIHost;
    if (medium) return kIMedium;
    if (prim < 0) return kIEscaped;
    if (cls & NNBVH_CLASS_INTERFACE) return kINext;
    return ((cls & NNBVH_CLASS_AREA_LIGHT) ? kIAreaLight : 0u) |
           ((cls & NNBVH_CLASS_UNIVERSAL) ? kIUniversal : kIBasic);
}

// The five slice tables hold 255 pointers.  Left alone, the compiler hoists their loads out of the loops
// and spills a thousand SGPRs.  So the tables are read through the kernel-argument segment itself, and the
// table's address is laundered where a group of fields is stored: each pointer is loaded (a scalar load,
// scalar cache) next to its store.  (Taking the address of the by-value kernel argument instead would copy
// it to scratch.)
#define KARG __attribute__((address_space(4)))
typedef const KARG nnbvh_item_slices *SliceTable;
__device__ __forceinline__ SliceTable fresh(SliceTable t) {
    __asm__ volatile("" : "+s"(t)::"memory");
    return t;
}

__device__ __forceinline__ void put1(float *p, int at, float v) {
    if (p) p[at] = v;
}
#define PUT3(field, v)                     \
    do {                                   \
        const SliceTable t_ = fresh(table); \
        put1(t_->field[0], at, (v)[0]);     \
        put1(t_->field[1], at, (v)[1]);     \
        put1(t_->field[2], at, (v)[2]);     \
    } while (0)

// one item's slices at slot `at`.  Which pointers may be non-null for which queue is checked by the
// entry points (include/nnbvh.h), so the values that differ between queues come in as arguments.
__device__ __forceinline__ void store_item(SliceTable table, int at, int prim, bool geometry,
                                           const nnbvh_interaction &r, const float *wo, float tMax,
                                           const float *rayO, const float *rayD) {
    if (int32_t *q = fresh(table)->prim) q[at] = prim;
    put1(fresh(table)->t_max, at, tMax);
    if (!geometry) return;
    {
        const SliceTable t = fresh(table);
#pragma unroll
        for (int k = 0; k < 3; ++k) {  // Point3fi: x.low x.high y.low y.high z.low z.high
            put1(t->pi[2 * k], at, r.pi_lo[k]);
            put1(t->pi[2 * k + 1], at, r.pi_hi[k]);
        }
    }
    {
        const SliceTable t = fresh(table);
#pragma unroll
        for (int k = 0; k < 3; ++k) put1(t->p[k], at, (r.pi_lo[k] + r.pi_hi[k]) / 2);  // Interval::Midpoint (util/math.h:851)
    }
    PUT3(n, r.n);
    PUT3(ns, r.ns);
    PUT3(dpdu, r.dpdu);
    PUT3(dpdv, r.dpdv);
    PUT3(dpdus, r.dpdus);
    PUT3(dpdvs, r.dpdvs);
    PUT3(dndus, r.dndus);
    PUT3(dndvs, r.dndvs);
    PUT3(wo, wo);
    {
        const SliceTable t = fresh(table);
        put1(t->uv[0], at, r.uv[0]);
        put1(t->uv[1], at, r.uv[1]);
        if (int32_t *q = t->face_index) q[at] = r.face_index;
        put1(t->time, at, r.time);
    }
    PUT3(ray_o, rayO);
    PUT3(ray_d, rayD);
}
#undef PUT3

#ifndef NNBVH_ITEMS_LEAN_WAVES
#define NNBVH_ITEMS_LEAN_WAVES 4
#endif
// EXT = 1: the forms that go with host candidates (include/nnbvh.h): a per-ray candidate count that sends a ray to
// needs_host whatever its record says, and / or an index list of the rays to enqueue (the second pass over the
// rays the caller has resolved).  Instances of their own: the plain ones stay as they are.
template <bool FULL, bool EXT = false>
__global__ __launch_bounds__(kItBlock, FULL ? 1 : NNBVH_ITEMS_LEAN_WAVES) void wf_enqueue_closest_items(
    ItemsParams p) {
    __shared__ float4 hitLds[kItItems][2][kItBlock];  // the chunk's hit records, 32 KB
    __shared__ int waveCount[kItBlock / 64][kItQueues];
    __shared__ int waveBase[kItBlock / 64][kItQueues];
    const nnbvh_work_queue *queues = &p.out.escaped;        // six consecutive members, in bit order ...
    // ... the slice tables of queues 1..5, read from the kernel-argument segment (p is the only argument)
    const SliceTable slices = &((const KARG ItemsParams *)__builtin_amdgcn_kernarg_segment_ptr())->items.hit_area_light;
    const int n = wf_count_items(p.cnt);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long chunk = (long)blockIdx.x * kItChunk; chunk < n; chunk += (long)gridDim.x * kItChunk) {
        unsigned dest = 0;  // kItBits per item
        int count[kItQueues] = {0, 0, 0, 0, 0, 0, 0};  // wave-uniform
#pragma unroll
        for (int k = 0; k < kItItems; ++k) {
            long i = chunk + k * kItBlock + threadIdx.x;
            unsigned d = 0;
            bool live = i < n;
            if (EXT && live && p.index) {
                i = p.index[i];
                live = i >= 0 && i < p.maxRays;
            }
            if (live) {
                const float4 h0 = p.hits[2 * i], h1 = p.hits[2 * i + 1];
                hitLds[k][0][threadIdx.x] = h0;
                hitLds[k][1][threadIdx.x] = h1;
                const int prim = __float_as_int(h0.x);
                const bool medium = p.soa.has_medium && p.soa.has_medium[i] != 0;
                unsigned cls = NNBVH_CLASS_BASIC;
                if (prim >= 0 && p.primClass && (long)prim < p.nPrimClass) cls = p.primClass[prim];
                d = item_destinations<FULL>(p.m, prim, __float_as_int(h1.w), medium, cls);
                if (EXT && p.hcCount && p.hcCount[i] != 0) d = kIHost;
            }
            dest |= d << (kItBits * k);
#pragma unroll
            for (int q = 0; q < kItQueues; ++q) count[q] += __popcll(__ballot((d >> q) & 1u));
        }
        if (lane == 0)
#pragma unroll
            for (int q = 0; q < kItQueues; ++q) waveCount[wave][q] = count[q];
        __syncthreads();
        if (threadIdx.x < kItQueues) {
            const int q = threadIdx.x;
            const nnbvh_work_queue &queue = q < 6 ? queues[q] : p.items.needs_host;
            int total = 0;
            for (int w = 0; w < kItBlock / 64; ++w) total += waveCount[w][q];
            int base = 0;
            if (total > 0 && queue.size) base = atomicAdd(queue.size, total);
            for (int w = 0; w < kItBlock / 64; ++w) {
                waveBase[w][q] = base;
                base += waveCount[w][q];
            }
        }
        __syncthreads();
        int run[kItQueues];
#pragma unroll
        for (int q = 0; q < kItQueues; ++q) run[q] = __builtin_amdgcn_readfirstlane(waveBase[wave][q]);  // SGPRs
#pragma unroll 1
        for (int k = 0; k < kItItems; ++k) {
            int i = (int)(chunk + k * kItBlock + threadIdx.x);
            const unsigned d = (dest >> (kItBits * k)) & ((1u << kItBits) - 1);
            if (EXT && d != 0 && p.index) i = p.index[i];  // d != 0: the slot is inside the list and its ray in range
            // an item is pushed to one queue, or to hit_area_light + one material queue: two slots
            int atLight = 0, at = 0;
#pragma unroll
            for (int q = 0; q < kItQueues; ++q) {
                const unsigned long long mask = __ballot((d >> q) & 1u);
                const int pos = run[q] + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32),
                                                                        __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
                if ((d >> q) & 1u) {
                    if (q == 1) atLight = pos;
                    else at = pos;
                }
                run[q] += __popcll(mask);
            }
            if (d == 0) continue;
#pragma unroll
            for (int q = 0; q < kItQueues; ++q) {
                const nnbvh_work_queue &queue = q < 6 ? queues[q] : p.items.needs_host;
                const int slot = q == 1 ? atLight : at;
                if (((d >> q) & 1u) && queue.size && slot < queue.capacity) queue.items[slot] = i;
            }
            if (d & (kIEscaped | kIHost)) continue;  // index only
            const float4 h0 = hitLds[k][0][threadIdx.x], h1 = hitLds[k][1][threadIdx.x];
            const int prim = __float_as_int(h0.x);
            const bool geometry = prim >= 0;  // everything left but a miss inside a medium
            nnbvh_interaction r;
            __builtin_memset(&r, 0, sizeof r);
            float rd[3] = {0, 0, 0};
            if (geometry) {
                rd[0] = p.soa.dx[i], rd[1] = p.soa.dy[i], rd[2] = p.soa.dz[i];
                const float time = p.soa.time ? p.soa.time[i] : 0.0f;
                const int status = imath::interaction_status<FULL>(p.m, prim, __float_as_int(h1.w));
                // a triangle with a zero geometric normal (never reported as hit) leaves r zero
                imath::surface_interaction<FULL>(p.m, status, prim, h0, h1, imath::F3{-rd[0], -rd[1], -rd[2]}, time,
                                                 r, [](int) {});
            }
            float ro[3] = {0, 0, 0};
            if (d & kINext) {  // Interaction::SpawnRay(ray.d): OffsetRayOrigin(pi, n, d) (interaction.h:98-100)
                const V3 o = offset_ray_origin(V3{r.pi_lo[0], r.pi_lo[1], r.pi_lo[2]},
                                               V3{r.pi_hi[0], r.pi_hi[1], r.pi_hi[2]}, V3{r.n[0], r.n[1], r.n[2]},
                                               V3{rd[0], rd[1], rd[2]});
                ro[0] = o.x, ro[1] = o.y, ro[2] = o.z;
            }
#pragma unroll
            for (int q = 1; q <= 5; ++q) {
                const nnbvh_work_queue &queue = queues[q];
                const int slot = q == 1 ? atLight : at;
                if (!((d >> q) & 1u) || !queue.size || slot >= queue.capacity) continue;
                // MediumSampleWorkItem::wo is -ray.d as it is (intersect.h:76); the others carry intr.wo
                const bool med = q == 4;
                const float wo[3] = {med ? -rd[0] : r.wo[0], med ? -rd[1] : r.wo[1], med ? -rd[2] : r.wo[2]};
                store_item(slices + (q - 1), slot, med && !geometry ? -1 : prim, geometry, r, wo,
                           geometry ? h0.y : __builtin_inff(), ro, rd);
            }
        }
        __syncthreads();  // the next chunk reuses the LDS records and counters
    }
}

hipError_t launch_wf_enqueue_closest_items(const ShadingMeshDevice &m, const void *hits, WavefrontCount cnt,
                                           const nnbvh_ray_soa &soa, const uint8_t *primClass, long nPrimClass,
                                           const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                           int maxBlocks, hipStream_t stream, const int32_t *hcCount,
                                           const int32_t *index, int maxRays) {
    ItemsParams p;
    p.hcCount = hcCount;
    p.index = index;
    p.maxRays = maxRays;
    p.m = MeshView{m.verts, m.triVerts, m.patchVerts, m.normals, m.uvs, m.tangents, m.faceIndices, m.triFlags,
                   m.nTris, m.defaultFlags, m.instances, m.nInstances, m.anim, m.animFwd};
    p.hits = (const float4 *)hits;
    p.cnt = cnt;
    p.soa = soa;
    p.primClass = primClass;
    p.nPrimClass = nPrimClass;
    p.out = out;
    p.items = items;
    int blocks = (cnt.n + kItChunk - 1) / kItChunk;
    blocks = blocks < 1 ? 1 : (blocks < maxBlocks ? blocks : maxBlocks);
    if (hcCount || index) {
        if (items_kernel_full(m))
            hipLaunchKernelGGL((wf_enqueue_closest_items<true, true>), dim3(blocks), dim3(kItBlock), 0, stream, p);
        else
            hipLaunchKernelGGL((wf_enqueue_closest_items<false, true>), dim3(blocks), dim3(kItBlock), 0, stream, p);
    } else if (items_kernel_full(m))
        hipLaunchKernelGGL(wf_enqueue_closest_items<true>, dim3(blocks), dim3(kItBlock), 0, stream, p);
    else
        hipLaunchKernelGGL(wf_enqueue_closest_items<false>, dim3(blocks), dim3(kItBlock), 0, stream, p);
    return hipGetLastError();
}

}  // namespace nnbvh
