// interaction.hip — Triangle:: and BilinearPatch::InteractionFromIntersection on the device
// (/root/reference/src/pbrt/shapes.h:884-1010, 1396-1489, with the SurfaceInteraction constructor
// and SetShadingGeometry they run: interaction.h:32-33, 164-214).
//
// The traversal kernels return what TriangleIntersection carries (primitive, b0 b1 b2, t);
// Triangle::Intersect (shapes.cpp:302-334) then builds the SurfaceInteraction every later stage of
// the reference reads (wavefront/intersect.h:49-156 copies pi, n, dpdu, dpdv, uv, shading.* and
// faceIndex into its work items).  This is that post-pass for a whole batch of hit records: one
// thread per item, ~250 flops, 80-190 B gathered (hit, ray direction + time, 3 vertex indices,
// 3 positions, optional uv / normal / tangent triples) and 192 B written — a streaming, HBM-bound
// pass a few percent of the trace it follows.  The per-hit arithmetic lives in interaction_math.h
// (shared with the work-item enqueue of wavefront_items.hip); tests/test_interaction.py checks it
// bit for bit against vectors produced by the compiled reference function.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "interaction.h"
#include "interaction_math.h"

namespace nnbvh {

// FULL = false: the mesh has neither bilinear patches nor an instance table — the patch interaction, the
// instance / AnimatedPrimitive transforms and their registers are compiled out (crown: 1.00 -> see DESIGN.md §5.6)
#ifndef NNBVH_INTR_LEAN_WAVES
#define NNBVH_INTR_LEAN_WAVES 4
#endif
template <bool FULL>
__global__ __launch_bounds__(256, FULL ? 1 : NNBVH_INTR_LEAN_WAVES) void k_triangle_interactions(
    MeshView m, const float4 *__restrict__ rays, nnbvh_ray_soa soa, const float4 *__restrict__ hits, int n,
    const int32_t *nDev, nnbvh_interaction *__restrict__ out) {
    if (nDev) {
        const int nd = *nDev;
        n = nd < 0 ? 0 : (nd < n ? nd : n);
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const float4 h0 = hits[2 * (long)i], h1 = hits[2 * (long)i + 1];
        const int prim = __float_as_int(h0.x);
        nnbvh_interaction r;
        __builtin_memset(&r, 0, sizeof r);
        r.prim = prim;
        int status = imath::interaction_status<FULL>(m, prim, __float_as_int(h1.w));
        r.status = status;
        if (status != NNBVH_INTERACTION_TRIANGLE && status != NNBVH_INTERACTION_PATCH) {
            // only prim / status are meaningful: store the record's last 16 B {prim, status, 0, 0}
            reinterpret_cast<float4 *>(out + i)[11] =
                make_float4(__int_as_float(prim), __int_as_float(status), 0.0f, 0.0f);
            continue;
        }
        imath::F3 wo;
        float time;
        if (rays) {
            const float4 r1 = rays[2 * (long)i + 1];
            wo = {-r1.x, -r1.y, -r1.z};  // Triangle::Intersect passes -ray.d (shapes.cpp:331)
            time = r1.w;
        } else {
            wo = {-soa.dx[i], -soa.dy[i], -soa.dz[i]};
            time = soa.time ? soa.time[i] : 0.0f;
        }
        imath::surface_interaction<FULL>(m, status, prim, h0, h1, wo, time, r, [&](int final_status) {
            if (final_status == NNBVH_INTERACTION_HOST) {
                reinterpret_cast<float4 *>(out + i)[11] =
                    make_float4(__int_as_float(prim), __int_as_float(NNBVH_INTERACTION_HOST), 0.0f, 0.0f);
                return;
            }
            out[i] = r;
        });
    }
}

hipError_t launch_triangle_interactions(const ShadingMeshDevice &m, const void *rays, const nnbvh_ray_soa *soa,
                                        const void *hits, int n, const int32_t *nDev, void *out, int maxBlocks,
                                        hipStream_t stream) {
    MeshView v{m.verts, m.triVerts, m.patchVerts, m.normals, m.uvs, m.tangents, m.faceIndices, m.triFlags, m.nTris, m.defaultFlags,
               m.instances, m.nInstances, m.anim, m.animFwd};
    nnbvh_ray_soa s;
    __builtin_memset(&s, 0, sizeof s);
    if (soa) s = *soa;
    int blocks = (n + 255) / 256;
    blocks = blocks < 1 ? 1 : (blocks < maxBlocks ? blocks : maxBlocks);
    if (m.patchVerts || m.instances)
        hipLaunchKernelGGL(k_triangle_interactions<true>, dim3(blocks), dim3(256), 0, stream, v, (const float4 *)rays, s,
                           (const float4 *)hits, n, nDev, (nnbvh_interaction *)out);
    else
        hipLaunchKernelGGL(k_triangle_interactions<false>, dim3(blocks), dim3(256), 0, stream, v, (const float4 *)rays, s,
                           (const float4 *)hits, n, nDev, (nnbvh_interaction *)out);
    return hipGetLastError();
}

}  // namespace nnbvh
