// wavefront2.hip — the bookkeeping kernels of WavefrontAggregate::IntersectShadowTr and
// ::IntersectOneRandom (/root/reference/src/pbrt/wavefront/aggregate.cpp:70-116) for scenes
// without participating media.
//
// Both reference functions are loops of closest-hit traces per work item:
//   IntersectShadowTr -> TraceTransmittance (wavefront/intersect.h:164-274): trace; an opaque hit
//       ends the ray with T = 0; a hit on an interface surface (no material) continues from the hit
//       point towards the light point with SpawnRayTo; without media T_ray, r_u, r_l stay 1, and a
//       ray that arrives adds Ld * (1 / (sr.r_u * 1 + sr.r_l * 1).Average()) to its pixel sample;
//   IntersectOneRandom (aggregate.cpp:90-116): walk the segment p0 -> p1 surface by surface and
//       reservoir-sample one hit whose material matches, WeightedReservoirSampler seeded with
//       Hash(p0, p1).
// On the device one loop iteration is one pass over the still-active items, two kernels: the trace
// kernel (bvh_trace.hip) and a step kernel here, which gives each item its verdict (walk_math.h: the
// hit's interaction stays in registers), updates the per-item state and writes the next segment's
// rays compacted (one atomic per wavefront).  Every kernel is a streaming pass, HBM-bound.
#include <hip/hip_runtime.h>

#include "interaction_math.h"
#include "spawn_math.h"
#include "walk_math.h"
#include "wavefront2.h"

namespace nnbvh {

static constexpr int kW2Block = 256;

__device__ __forceinline__ int w2_count(WavefrontCount c) {
    int n = c.n;
    if (c.nDev) {
        const int nd = *c.nDev;
        n = nd < 0 ? 0 : (nd < n ? nd : n);
    }
    return n;
}

// wave-aggregated append: returns this lane's slot in the list `counter` counts, or -1
__device__ __forceinline__ int w2_append(bool want, int32_t *counter) {
    const unsigned long long mask = __ballot(want);
    if (mask == 0ull) return -1;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)mask) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(counter, __popcll(mask));
    base = __shfl(base, leader);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
    return want ? base + rank : -1;
}

static int w2_grid(int n, int maxBlocks) {
    int blocks = (n + kW2Block - 1) / kW2Block;
    if (blocks < 1) blocks = 1;
    return blocks < maxBlocks ? blocks : maxBlocks;
}

// ---- IntersectShadowTr ------------------------------------------------------------------------
// state: 0 = arrives (T_ray = 1), 1 = blocked by an opaque surface, 2 = a host-only primitive or an
// interaction the device cannot finish lies on the way: the caller's to finish
__global__ __launch_bounds__(kW2Block) void str_init(nnbvh_ray_soa q, WavefrontCount cnt, float4 *rays,
                                                     int32_t *orig, float4 *pLight, uint8_t *state) {
    const int n = w2_count(cnt);
    for (int i = blockIdx.x * kW2Block + threadIdx.x; i < n; i += gridDim.x * kW2Block) {
        float4 a, b;
        a.x = q.ox[i];
        a.y = q.oy[i];
        a.z = q.oz[i];
        a.w = q.tmax ? q.tmax[i] : __builtin_inff();
        b.x = q.dx[i];
        b.y = q.dy[i];
        b.z = q.dz[i];
        b.w = q.time ? q.time[i] : 0.0f;
        rays[2 * (long)i] = a;
        rays[2 * (long)i + 1] = b;
        orig[i] = i;
        // Point3f pLight = ray(tMax) = o + d * t (ray.h:33, intersect.h:177)
        pLight[i] = make_float4(a.x + b.x * a.w, a.y + b.y * a.w, a.z + b.z * a.w, 0.0f);
        state[i] = 0;
    }
}

// intersect.h:258-273 with T_ray = r_u = r_l = SampledSpectrum(1.f)
__global__ __launch_bounds__(kW2Block) void str_record(const uint8_t *state, WavefrontCount cnt, const float4 *Ld,
                                                       const float4 *ru, const float4 *rl,
                                                       const int32_t *pixelIndex, float *L, long nPixels,
                                                       uint8_t *visibleOut) {
    const int n = w2_count(cnt);
    for (int i = blockIdx.x * kW2Block + threadIdx.x; i < n; i += gridDim.x * kW2Block) {
        const uint8_t st = state[i];
        if (visibleOut) visibleOut[i] = st;
        if (st != 0) continue;
        const float4 ld = Ld[i], u = ru[i], l = rl[i];
        // (sr.r_u * r_u + sr.r_l * r_l).Average(), r_u = r_l = 1
        const float s0 = u.x * 1.0f + l.x * 1.0f, s1 = u.y * 1.0f + l.y * 1.0f, s2 = u.z * 1.0f + l.z * 1.0f,
                    s3 = u.w * 1.0f + l.w * 1.0f;
        float sum = s0;
        sum += s1;
        sum += s2;
        sum += s3;
        const float avg = sum / 4.0f;
        const float k = 1.0f / avg;  // T_ray / Average(): SampledSpectrum / Float, component by component
        const long px = pixelIndex[i];
        if (px < 0 || px >= nPixels) continue;
        float4 *dst = reinterpret_cast<float4 *>(L) + px;
        float4 v = *dst;
        v.x = v.x + ld.x * k;  // Ld *= T_ray / ...; L = Lpixel + Ld
        v.y = v.y + ld.y * k;
        v.z = v.z + ld.z * k;
        v.w = v.w + ld.w * k;
        *dst = v;
    }
}

// ---- IntersectOneRandom -----------------------------------------------------------------------
// Item i before its walk: the seeded reservoir, cleared outputs and the first segment ray {a, b} (its direction may
// be zero)
__device__ __forceinline__ void or_init_item(const float *p0, const float *p1, int i, OneRandomState st,
                                             float4 *selHits, float4 *selRays, float4 &a, float4 &b) {
    const V3 a0 = {p0[3 * (long)i], p0[3 * (long)i + 1], p0[3 * (long)i + 2]};
    const V3 a1 = {p1[3 * (long)i], p1[3 * (long)i + 1], p1[3 * (long)i + 2]};
    Pcg32 g;  // WeightedReservoirSampler wrs(Hash(w.p0, w.p1)), aggregate.cpp:94-96
    pcg32_set_sequence(g, hash_6f(a0, a1));
    st.rng[2 * (long)i] = g.state;
    st.rng[2 * (long)i + 1] = g.inc;
    st.weights[2 * (long)i] = 0.0f;
    st.weights[2 * (long)i + 1] = 0.0f;
    selHits[2 * (long)i] = make_float4(__int_as_float(-1), 0.0f, 0.0f, 0.0f);
    selHits[2 * (long)i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    selRays[2 * (long)i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    selRays[2 * (long)i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    V3 o, d;
    // Interaction base(w.p0, 0, Medium()): exact point, n = (0, 0, 0); r = base.SpawnRayTo(w.p1), :97-99
    spawn_ray_to(a0, a0, {0.0f, 0.0f, 0.0f}, a1, o, d);
    a = make_float4(o.x, o.y, o.z, 1.0f);  // aggregate.Intersect(r, 1), :102
    b = make_float4(d.x, d.y, d.z, 0.0f);
}

__global__ __launch_bounds__(kW2Block) void or_init(const float *p0, const float *p1, WavefrontCount cnt,
                                                    OneRandomState st, float4 *raysOut, int32_t *origOut,
                                                    int32_t *counter, float4 *selHits, float4 *selRays) {
    const int n = w2_count(cnt);
    const int nPad = (n + 63) & ~63;
    for (int i = blockIdx.x * kW2Block + threadIdx.x; i < nPad; i += gridDim.x * kW2Block) {
        bool goOn = false;
        float4 a, b;
        if (i < n) {
            or_init_item(p0, p1, i, st, selHits, selRays, a, b);
            goOn = !(b.x == 0.0f && b.y == 0.0f && b.z == 0.0f);  // :100-101
        }
        const int at = w2_append(goOn, counter);
        if (at >= 0) {
            raysOut[2 * (long)at] = a;
            raysOut[2 * (long)at + 1] = b;
            origOut[at] = i;
        }
    }
}

__global__ __launch_bounds__(kW2Block) void or_finish(WavefrontCount cnt, OneRandomState st, float *pdf,
                                                      float *weightSumOut) {
    const int n = w2_count(cnt);
    for (int i = blockIdx.x * kW2Block + threadIdx.x; i < n; i += gridDim.x * kW2Block) {
        const float weightSum = st.weights[2 * (long)i], reservoirWeight = st.weights[2 * (long)i + 1];
        // :110-114: HasSample() ? SampleProbability() = reservoirWeight / weightSum : 0
        pdf[i] = weightSum > 0 ? reservoirWeight / weightSum : 0.0f;
        if (weightSumOut) weightSumOut[i] = weightSum;
    }
}

// ---- one fused step per pass ------------------------------------------------------------------------
// A pass of either walk is two kernels: the trace and one of the steps below, the list bookkeeping around the per-item
// bodies of walk_math.h (w2_str_item / w2_or_item, the bodies the walk instances of the trace kernels call).  The
// hit's interaction is computed in registers: only pi and n are used, so the other fields' arithmetic is dead code
// and no 192-byte record is written or read back.  The bounded calls enqueue their passes up front, sized for the
// queue; the unbounded calls launch them one by one, sized by the count the host has read back.
template <bool FULL>
__global__ __launch_bounds__(kW2Block) void str_step(MeshView m, const float4 *raysCur, const float4 *hitsCur,
                                                     const int32_t *origCur, WavefrontCount cur,
                                                     const uint8_t *primClass, long nPrimClass, const float4 *pLight,
                                                     uint8_t *state, float4 *raysNext, int32_t *origNext,
                                                     int32_t *counter) {
    const int n = w2_count(cur);
    const int nPad = (n + 63) & ~63;  // whole wavefronts take part in the ballots
    for (int j = blockIdx.x * kW2Block + threadIdx.x; j < nPad; j += gridDim.x * kW2Block) {
        bool goOn = false;
        float4 a, b;
        int item = 0;
        if (j < n) {
            const float4 r0 = raysCur[2 * (long)j], r1 = raysCur[2 * (long)j + 1];
            const float4 h0 = hitsCur[2 * (long)j], h1 = hitsCur[2 * (long)j + 1];
            item = origCur[j];
            V3 o, d;
            goOn = w2_str_item<FULL>(m, r0, r1, h0, h1, item, primClass, nPrimClass, pLight, state, o, d);
            a = make_float4(o.x, o.y, o.z, r0.w);  // tMax and time are the work item's, unchanged (:175, :187)
            b = make_float4(d.x, d.y, d.z, r1.w);
        }
        const int at = w2_append(goOn, counter);
        if (at >= 0) {
            raysNext[2 * (long)at] = a;
            raysNext[2 * (long)at + 1] = b;
            origNext[at] = item;
        }
    }
}

template <bool FULL>
__global__ __launch_bounds__(kW2Block) void or_step_fused(MeshView m, const float4 *raysCur, const float4 *hitsCur,
                                                          const int32_t *origCur, WavefrontCount cur, const float *p1,
                                                          const int32_t *material, const int32_t *primMaterial,
                                                          long nPrimMaterial, OneRandomState st, float4 *raysNext,
                                                          int32_t *origNext, int32_t *counter, float4 *selHits,
                                                          float4 *selRays) {
    const int n = w2_count(cur);
    const int nPad = (n + 63) & ~63;
    for (int j = blockIdx.x * kW2Block + threadIdx.x; j < nPad; j += gridDim.x * kW2Block) {
        bool goOn = false;
        float4 a, b;
        int item = 0;
        if (j < n) {
            item = origCur[j];
            const float4 r0 = raysCur[2 * (long)j], r1 = raysCur[2 * (long)j + 1];
            const float4 h0 = hitsCur[2 * (long)j], h1 = hitsCur[2 * (long)j + 1];
            V3 o, d;
            goOn = w2_or_item<FULL>(m, r0, r1, h0, h1, item, p1, material, primMaterial, nPrimMaterial, st, selHits,
                                    selRays, o, d);
            a = make_float4(o.x, o.y, o.z, 1.0f);  // aggregate.Intersect(r, 1), :102
            b = make_float4(d.x, d.y, d.z, 0.0f);
        }
        const int at = w2_append(goOn, counter);
        if (at >= 0) {
            raysNext[2 * (long)at] = a;
            raysNext[2 * (long)at + 1] = b;
            origNext[at] = item;
        }
    }
}

__global__ __launch_bounds__(kW2Block) void w2_mark_unfinished(const float4 *raysLeft, const int32_t *origLeft,
                                                               WavefrontCount left, uint8_t *state, float4 *selHits,
                                                               int32_t *unfinished) {
    const int n = w2_count(left);
    const int nPad = (n + 63) & ~63;
    for (int j = blockIdx.x * kW2Block + threadIdx.x; j < nPad; j += gridDim.x * kW2Block) {
        bool mark = false;
        if (j < n) {
            const int item = origLeft[j];
            if (state) {  // while (ray.d != Vector3f(0, 0, 0)): a zero direction has ended the walk, the ray arrives
                const float4 r1 = raysLeft[2 * (long)j + 1];
                mark = !(r1.x == 0.0f && r1.y == 0.0f && r1.z == 0.0f);
                if (mark) state[item] = 2;
            } else {
                mark = true;
                selHits[2 * (long)item + 1].w = __int_as_float(-1);
            }
        }
        const unsigned long long mask = __ballot(mark);
        if (unfinished && mask != 0ull && (threadIdx.x & 63) == __ffsll((long long)mask) - 1)
            atomicAdd(unfinished, __popcll(mask));
    }
}

// or_init for the walk instances of the trace kernels (both trees): EVERY item's first segment ray goes to rays[i], a
// zero direction included (the walk kernel ends such an item at its fetch), so there is no list to compact and nothing
// to count.  (A template, so that it is emitted behind the kernels above.)
template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void or_init_all(const float *p0, const float *p1, WavefrontCount cnt,
                                                   OneRandomState st, float4 *rays, float4 *selHits,
                                                   float4 *selRays) {
    int n = cnt.n;
    if (cnt.nDev) {
        const int nd = *cnt.nDev;
        n = nd < 0 ? 0 : (nd < n ? nd : n);
    }
    for (int i = blockIdx.x * BLOCK + threadIdx.x; i < n; i += gridDim.x * BLOCK) {
        float4 a, b;
        or_init_item(p0, p1, i, st, selHits, selRays, a, b);
        rays[2 * (long)i] = a;
        rays[2 * (long)i + 1] = b;
    }
}

// ---- launchers ----------------------------------------------------------------------------------
hipError_t launch_str_init(const nnbvh_ray_soa &q, WavefrontCount cnt, void *rays, int32_t *orig, float4 *pLight,
                           uint8_t *state, int maxBlocks, hipStream_t stream) {
    hipLaunchKernelGGL(str_init, dim3(w2_grid(cnt.n, maxBlocks)), dim3(kW2Block), 0, stream, q, cnt, (float4 *)rays,
                       orig, pLight, state);
    return hipGetLastError();
}
hipError_t launch_str_record(const uint8_t *state, WavefrontCount cnt, const float *Ld, const float *ru,
                             const float *rl, const int32_t *pixelIndex, float *L, long nPixels,
                             uint8_t *visibleOut, int maxBlocks, hipStream_t stream) {
    hipLaunchKernelGGL(str_record, dim3(w2_grid(cnt.n, maxBlocks)), dim3(kW2Block), 0, stream, state, cnt,
                       (const float4 *)Ld, (const float4 *)ru, (const float4 *)rl, pixelIndex, L, nPixels,
                       visibleOut);
    return hipGetLastError();
}
hipError_t launch_or_init(const float *p0, const float *p1, WavefrontCount cnt, OneRandomState st, void *raysOut,
                          int32_t *origOut, int32_t *counter, void *selHits, void *selRays, int maxBlocks,
                          hipStream_t stream) {
    hipLaunchKernelGGL(or_init, dim3(w2_grid(cnt.n, maxBlocks)), dim3(kW2Block), 0, stream, p0, p1, cnt, st,
                       (float4 *)raysOut, origOut, counter, (float4 *)selHits, (float4 *)selRays);
    return hipGetLastError();
}
hipError_t launch_or_finish(WavefrontCount cnt, OneRandomState st, float *pdf, float *weightSum, int maxBlocks,
                            hipStream_t stream) {
    hipLaunchKernelGGL(or_finish, dim3(w2_grid(cnt.n, maxBlocks)), dim3(kW2Block), 0, stream, cnt, st, pdf,
                       weightSum);
    return hipGetLastError();
}

static MeshView w2_mesh_view(const ShadingMeshDevice &m) {
    return {m.verts, m.triVerts, m.patchVerts, m.normals, m.uvs, m.tangents, m.faceIndices, m.triFlags, m.nTris,
            m.defaultFlags, m.instances, m.nInstances, m.anim, m.animFwd};
}
// FULL as launch_triangle_interactions chooses it: the mesh has patches or an instance table
hipError_t launch_str_step(const ShadingMeshDevice &m, const void *raysCur, const void *hitsCur,
                           const int32_t *origCur, WavefrontCount cur, const uint8_t *primClass, long nPrimClass,
                           const float4 *pLight, uint8_t *state, void *raysNext, int32_t *origNext, int32_t *counter,
                           int maxBlocks, hipStream_t stream) {
    const dim3 grid(w2_grid(cur.n, maxBlocks)), block(kW2Block);
    if (m.patchVerts || m.instances)
        hipLaunchKernelGGL(str_step<true>, grid, block, 0, stream, w2_mesh_view(m), (const float4 *)raysCur,
                           (const float4 *)hitsCur, origCur, cur, primClass, nPrimClass, pLight, state,
                           (float4 *)raysNext, origNext, counter);
    else
        hipLaunchKernelGGL(str_step<false>, grid, block, 0, stream, w2_mesh_view(m), (const float4 *)raysCur,
                           (const float4 *)hitsCur, origCur, cur, primClass, nPrimClass, pLight, state,
                           (float4 *)raysNext, origNext, counter);
    return hipGetLastError();
}
hipError_t launch_or_step_fused(const ShadingMeshDevice &m, const void *raysCur, const void *hitsCur,
                                const int32_t *origCur, WavefrontCount cur, const float *p1, const int32_t *material,
                                const int32_t *primMaterial, long nPrimMaterial, OneRandomState st, void *raysNext,
                                int32_t *origNext, int32_t *counter, void *selHits, void *selRays, int maxBlocks,
                                hipStream_t stream) {
    const dim3 grid(w2_grid(cur.n, maxBlocks)), block(kW2Block);
    if (m.patchVerts || m.instances)
        hipLaunchKernelGGL(or_step_fused<true>, grid, block, 0, stream, w2_mesh_view(m), (const float4 *)raysCur,
                           (const float4 *)hitsCur, origCur, cur, p1, material, primMaterial, nPrimMaterial, st,
                           (float4 *)raysNext, origNext, counter, (float4 *)selHits, (float4 *)selRays);
    else
        hipLaunchKernelGGL(or_step_fused<false>, grid, block, 0, stream, w2_mesh_view(m), (const float4 *)raysCur,
                           (const float4 *)hitsCur, origCur, cur, p1, material, primMaterial, nPrimMaterial, st,
                           (float4 *)raysNext, origNext, counter, (float4 *)selHits, (float4 *)selRays);
    return hipGetLastError();
}
hipError_t launch_w2_mark_unfinished(const void *raysLeft, const int32_t *origLeft, WavefrontCount left,
                                     uint8_t *state, void *selHits, int32_t *unfinished, int maxBlocks,
                                     hipStream_t stream) {
    hipLaunchKernelGGL(w2_mark_unfinished, dim3(w2_grid(left.n, maxBlocks)), dim3(kW2Block), 0, stream,
                       (const float4 *)raysLeft, origLeft, left, state, (float4 *)selHits, unfinished);
    return hipGetLastError();
}
// (last: or_init_all is then emitted behind the kernels above)
hipError_t launch_or_init_all(const float *p0, const float *p1, WavefrontCount cnt, OneRandomState st, void *rays,
                              void *selHits, void *selRays, int maxBlocks, hipStream_t stream) {
    hipLaunchKernelGGL(or_init_all<kW2Block>, dim3(w2_grid(cnt.n, maxBlocks)), dim3(kW2Block), 0, stream, p0, p1, cnt,
                       st, (float4 *)rays, (float4 *)selHits, (float4 *)selRays);
    return hipGetLastError();
}

}  // namespace nnbvh
