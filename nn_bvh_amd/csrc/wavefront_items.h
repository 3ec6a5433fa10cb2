// wavefront_items.h — launch interface of the work-item enqueue (wavefront_items.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nnbvh.h"
#include "interaction.h"
#include "wavefront.h"

namespace nnbvh {

__device__ __forceinline__ int wf_count_items(const WavefrontCount &c) {
    int n = c.n;
    if (c.nDev) {
        const int nd = *c.nDev;
        n = nd < 0 ? 0 : (nd < n ? nd : n);
    }
    return n;
}

// the FULL kernel instance (patch interaction, instance transforms) only where the mesh needs it
inline bool items_kernel_full(const ShadingMeshDevice &m) { return m.patchVerts || m.instances; }

// soa: the ray queue the hits belong to (dx dy dz read; time and has_medium optional)
// hcCount (nullable, per ray): rays with a non-zero host-candidate count go to needs_host only.  index (nullable):
// enqueue rays index[0 .. n) with n from cnt; entries outside [0, maxRays) are skipped.  Either one selects the
// kernel's EXT instances; without them the plain instances run.
hipError_t launch_wf_enqueue_closest_items(const ShadingMeshDevice &m, const void *hits, WavefrontCount cnt,
                                           const nnbvh_ray_soa &soa, const uint8_t *primClass, long nPrimClass,
                                           const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                           int maxBlocks, hipStream_t stream, const int32_t *hcCount = nullptr,
                                           const int32_t *index = nullptr, int maxRays = 0);

}  // namespace nnbvh
