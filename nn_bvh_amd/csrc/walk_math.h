// walk_math.h — the IntersectShadowTr / IntersectOneRandom walks (wavefront/intersect.h:183-256,
// wavefront/aggregate.cpp:100-108) as the walk instances of both trace kernels run them (bvh_trace.hip modes 4 / 5,
// kd_trace.hip modes 4 / 5), inside the lane that has just finished the closest-hit walk: the per-item
// arrays (WalkParams, one member of either kernel's arguments), the launch job both launchers take (WalkJob) and the
// per-item bodies of the retire step.  w2_str_item / w2_or_item are the walks' rules, written once: the fused pass
// steps of the BVH pass calls, bounded and unbounded (wavefront2.hip: str_step, or_step_fused), are the list
// bookkeeping around the same two bodies.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "interaction_math.h"
#include "spawn_math.h"
#include "wavefront2.h"

namespace nnbvh {

// The per-item arrays of a walk: the last member of TraceParams and of KdParams, behind the kernel's shading mesh.
struct WalkParams {
    const uint8_t *primClass;       // WALK 1: class per primitive id, nullable
    long nPrimClass;
    const float4 *pLight;           // WALK 1: the light point of each item
    uint8_t *state;                 // WALK 1: 0 at launch; 1 blocked, 2 the caller's to finish
    const float *p1;                // WALK 2: the segment's end point of each item
    const int32_t *material;        // WALK 2: the material each item looks for
    const int32_t *primMaterial;    // WALK 2: material per primitive id, nullable
    long nPrimMaterial;
    OneRandomState st;              // WALK 2: PCG32 state and reservoir weights per item
    float4 *selHits, *selRays;      // WALK 2: selected hit record and its segment ray per item
    int maxSurfaces;                // Intersect calls an item may make
    int32_t *unfinished;            // nullable: counts the items that would start one more
};

// One launch of a walk instance of a trace kernel behind its queue reset node (launch_walk: capi_trace.cpp for BVH
// scenes, capi_kd.cpp for kd-tree scenes), over the items whose first rays are the records `rays`: item i is ray i,
// and the batch holds min(n, max(*d_n, 0)) of them (d_n nullable).  The caller has checked the arguments, the type's
// refusals among them, and holds the scene's lock.
struct WalkJob {
    int kind = 1;  // 1: IntersectShadowTr's walk, 2: IntersectOneRandom's
    const ShadingMeshDevice *mesh = nullptr;
    const void *rays = nullptr;
    int64_t n = 0;
    const int32_t *d_n = nullptr;
    // kind 1: state[] is 0 and pLight[] set for every item (str_init); kind 2: the arrays launch_or_init_all
    // (wavefront2.h) has set; unfinished (nullable) is zero before the launch
    WalkParams a{};
};

// pi low / high and n of the SurfaceInteraction of hit {h0, h1} of the ray whose second half is r1;
// false: a hit the device cannot finish (the post-pass's status is neither TRIANGLE nor PATCH)
template <bool FULL>
__device__ __forceinline__ bool w2_hit_pi_n(const MeshView &m, float4 h0, float4 h1, float4 r1, V3 &lo, V3 &hi,
                                            V3 &n) {
    const int prim = __float_as_int(h0.x);
    const int status = imath::interaction_status<FULL>(m, prim, __float_as_int(h1.w));
    if (status != NNBVH_INTERACTION_TRIANGLE && status != NNBVH_INTERACTION_PATCH) return false;
    nnbvh_interaction r;
    __builtin_memset(&r, 0, sizeof r);
    bool ok = false;
    imath::surface_interaction<FULL>(m, status, prim, h0, h1, imath::F3{-r1.x, -r1.y, -r1.z}, r1.w, r,
                                     [&](int final_status) { ok = final_status != NNBVH_INTERACTION_HOST; });
    lo = {r.pi_lo[0], r.pi_lo[1], r.pi_lo[2]};
    hi = {r.pi_hi[0], r.pi_hi[1], r.pi_hi[2]};
    n = {r.n[0], r.n[1], r.n[2]};
    return ok;
}

// Shadow ray {r0, r1} of work item `item` with the closest hit {h0, h1}: one turn of TraceTransmittance's loop
// (intersect.h:183-256).  true: the walk goes on from o in direction d, tMax and time kept (a zero direction is the
// caller's to catch: the next step's first verdict); false: the walk has ended, state[item] holds 1 or 2 where the ray
// does not arrive.
template <bool FULL>
__device__ __forceinline__ bool w2_str_item(const MeshView &m, float4 r0, float4 r1, float4 h0, float4 h1, int item,
                                            const uint8_t *primClass, long nPrimClass, const float4 *pLight,
                                            uint8_t *state, V3 &o, V3 &d) {
    o = d = {0.0f, 0.0f, 0.0f};
    const bool zeroDir = r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f;
    const int prim = __float_as_int(h0.x);
    if (zeroDir) {  // while (ray.d != Vector3f(0, 0, 0)), :183: a zero direction ends the walk, T stays 1
    } else if (__float_as_int(h1.w) == -1) {
        state[item] = 2;  // a host-only primitive lies on the way
    } else if (prim >= 0) {
        unsigned cls = NNBVH_CLASS_BASIC;
        if (primClass && (long)prim < nPrimClass) cls = primClass[prim];
        if (!(cls & NNBVH_CLASS_INTERFACE)) {
            state[item] = 1;  // :190-195 hit opaque surface
        } else {  // result.hit && !result.material
            V3 lo, hi, nn;
            if (!w2_hit_pi_n<FULL>(m, h0, h1, r1, lo, hi, nn)) {
                state[item] = 2;
            } else {
                const float4 pl = pLight[item];
                spawn_ray_to(lo, hi, nn, {pl.x, pl.y, pl.z}, o, d);  // ray = spawnTo(pLight), :255
                return true;
            }
        }
    }
    return false;
}

// Segment ray {r0, r1} of one-random item `item` with the closest hit {h0, h1}: one turn of IntersectOneRandom's loop
// (aggregate.cpp:100-108).  true: the walk goes on from o in direction d (never zero), tMax = 1, time = 0.
template <bool FULL>
__device__ __forceinline__ bool w2_or_item(const MeshView &m, float4 r0, float4 r1, float4 h0, float4 h1, int item,
                                           const float *p1, const int32_t *material, const int32_t *primMaterial,
                                           long nPrimMaterial, OneRandomState st, float4 *selHits, float4 *selRays,
                                           V3 &o, V3 &d) {
    o = d = {0.0f, 0.0f, 0.0f};
    const int prim = __float_as_int(h0.x);
    V3 lo, hi, nn;
    if (prim < 0 && __float_as_int(h1.w) != -1) {
        // :103-104 no further surface on the segment: the walk ends
    } else if (__float_as_int(h1.w) == -1 || !w2_hit_pi_n<FULL>(m, h0, h1, r1, lo, hi, nn)) {
        selHits[2 * (long)item + 1].w = __int_as_float(-1);  // the item is the caller's
    } else {  // base = si->intr, :105
        const int mat = (primMaterial && (long)prim < nPrimMaterial) ? primMaterial[prim] : 0;
        if (mat == material[item]) {  // :106-107 wrs.Add(SubsurfaceInteraction(si->intr), 1.f)
            Pcg32 g = {st.rng[2 * (long)item], st.rng[2 * (long)item + 1]};
            float weightSum = st.weights[2 * (long)item];
            const float weight = 1.0f;
            weightSum += weight;
            const float p = weight / weightSum;
            if (pcg32_float(g) < p) {  // util/sampling.h:535-546
                selHits[2 * (long)item] = h0;
                selHits[2 * (long)item + 1] = h1;
                selRays[2 * (long)item] = r0;
                selRays[2 * (long)item + 1] = r1;
                st.weights[2 * (long)item + 1] = weight;
            }
            st.weights[2 * (long)item] = weightSum;
            st.rng[2 * (long)item] = g.state;
        }
        const V3 a1 = {p1[3 * (long)item], p1[3 * (long)item + 1], p1[3 * (long)item + 2]};
        spawn_ray_to(lo, hi, nn, a1, o, d);
        if (!(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f)) return true;
    }
    return false;
}

}  // namespace nnbvh
