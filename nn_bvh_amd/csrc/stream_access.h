// stream_access.h — loads and stores for data that a launch touches exactly once (ray records and queue slices in,
// hit records, occlusion bytes and counts out): they carry the non-temporal hint (the `nt` bit of global_load /
// global_store on gfx950), so that they do not compete with the tree's records for cache lines.  What is computed
// cannot depend on them: the hint says where bytes are cached, not what they are.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nnbvh {

typedef float stream_f4 __attribute__((ext_vector_type(4)));

static __device__ __forceinline__ float4 load_stream(const float4 *p) {
    const stream_f4 v = __builtin_nontemporal_load(reinterpret_cast<const stream_f4 *>(p));
    return make_float4(v.x, v.y, v.z, v.w);
}
static __device__ __forceinline__ void store_stream(float4 *p, float4 v) {
    const stream_f4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<stream_f4 *>(p));
}
static __device__ __forceinline__ float load_stream(const float *p) { return __builtin_nontemporal_load(p); }
static __device__ __forceinline__ void store_stream(uint8_t *p, uint8_t v) { __builtin_nontemporal_store(v, p); }
static __device__ __forceinline__ void store_stream(int32_t *p, int32_t v) { __builtin_nontemporal_store(v, p); }

}  // namespace nnbvh
