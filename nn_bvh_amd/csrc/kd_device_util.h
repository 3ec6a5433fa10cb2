// kd_device_util.h — device helpers shared by the kd-tree builder (kd_build_gpu.hip) and the device-side scene
// creation (kd_bake.hip): both reduce (value, index) pairs to "the first of equals" through 64-bit minima.
#pragma once
#include <hip/hip_runtime.h>

namespace nnbvh {

__device__ __forceinline__ unsigned kd_ordered_bits(float f) {  // monotone float -> unsigned; -0 and +0 compare equal
    unsigned u = __float_as_uint(f);
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ unsigned long long kd_wave_min_u64(unsigned long long v) {
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned lo = __shfl_xor((unsigned)v, off), hi = __shfl_xor((unsigned)(v >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

}  // namespace nnbvh
