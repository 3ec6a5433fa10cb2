// tree_quality.hip — SAH and EPO of a baked tree as the fork's machine_learning/nn_loss.py defines them (DESIGN.md
// §5.16), for gfx950.
//
// EPO by its set definition: a primitive p is external to node n when p is not in n's subtree and at least one of its
// vertices lies in n's closed box.  Swapping the sums, epo needs per primitive only the NUMBERS of inner nodes and of
// leaves that hold it as an external: one stackless point-in-box walk over the depth-first node array per primitive,
// exact integers out.  The double sums go through a reduction of fixed shape (block partials in index order, one block
// over the partials): no floating-point atomics, the same 64 bits on every call.
#include <hip/hip_runtime.h>

#include "tree_quality.h"

namespace nnbvh {

#ifndef NNBVH_QUALITY_FOLD
#define NNBVH_QUALITY_FOLD 2  // how the lanes of a wave that sit on the same node add to it
#endif

// ---- preparation ---------------------------------------------------------------------------------------------------
// One thread per node: end[n] by chasing second children to the subtree's rightmost leaf (the host has refused trees
// deeper than kQualityMaxDepth, so the chase is bounded; the bound is kept here so that no input can make it long),
// the packed record, and for a leaf the leaf_of[] entries of its positions.
__global__ __launch_bounds__(kQualityBlock) void quality_prepare_kernel(const nnbvh_linear_node *__restrict__ nodes,
                                                                         int n_nodes, int n_prims,
                                                                         float4 *__restrict__ rec,
                                                                         int32_t *__restrict__ leaf_of,
                                                                         int32_t *__restrict__ node_external) {
    const int n = blockIdx.x * kQualityBlock + threadIdx.x;
    if (n >= n_nodes) return;
    const nnbvh_linear_node me = nodes[n];
    int k = n;
    for (int step = 0; step < kQualityMaxDepth; ++step) {
        if (nodes[k].nprims != 0) break;
        const int next = nodes[k].offset;
        if (next <= k || next >= n_nodes) break;  // never on a validated tree
        k = next;
    }
    const int end = k + 1;
    rec[2 * (size_t)n] = make_float4(me.pmin[0], me.pmin[1], me.pmin[2], me.pmax[0]);
    rec[2 * (size_t)n + 1] = make_float4(me.pmax[1], me.pmax[2], __int_as_float(end), __int_as_float((int)me.nprims));
    node_external[n] = 0;
    for (int j = 0; j < (int)me.nprims; ++j) {
        const long long pos = (long long)me.offset + j;
        if (pos >= 0 && pos < n_prims) leaf_of[pos] = n;
    }
}

// ---- the walk ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool in_box(float x, float y, float z, const float4 &a, const float4 &b) {
    return x >= a.x && x <= a.w && y >= a.y && y <= b.x && z >= a.z && z <= b.y;
}

// One lane per ordered position: neighbouring lanes hold the primitives of one leaf or of neighbouring leaves and walk
// alike.  i rises strictly, so a lane leaves the loop after at most n_nodes trips.  No stack, no LDS.
__global__ __launch_bounds__(kQualityBlock) void quality_walk_kernel(const float4 *__restrict__ rec, int n_nodes,
                                                                      const nnbvh_prim *__restrict__ prims,
                                                                      const float *__restrict__ verts,
                                                                      const int32_t *__restrict__ leaf_of, int n_prims,
                                                                      int32_t *__restrict__ k_inner,
                                                                      int32_t *__restrict__ k_leaf,
                                                                      int32_t *__restrict__ node_external) {
    const int j = blockIdx.x * kQualityBlock + threadIdx.x;
    if (j >= n_prims) return;
    const nnbvh_prim p = prims[j];
    const float *v0 = verts + 3 * (size_t)p.v[0], *v1 = verts + 3 * (size_t)p.v[1], *v2 = verts + 3 * (size_t)p.v[2];
    const float x0 = v0[0], y0 = v0[1], z0 = v0[2];
    const float x1 = v1[0], y1 = v1[1], z1 = v1[2];
    const float x2 = v2[0], y2 = v2[1], z2 = v2[2];
    const int own = leaf_of[j];
    int ki = 0, kl = 0;
    int i = 0;
    while (i < n_nodes) {
        const float4 a = rec[2 * (size_t)i], b = rec[2 * (size_t)i + 1];
        const int end = __float_as_int(b.z), nprims = __float_as_int(b.w);
        const bool inside = in_box(x0, y0, z0, a, b) || in_box(x1, y1, z1, a, b) || in_box(x2, y2, z2, a, b);
        const bool external = inside && !(i <= own && own < end);
        if (external) {
            ki += nprims == 0;
            kl += nprims != 0;
        }
#if NNBVH_QUALITY_FOLD == 2
        // the externals of this trip that sit on the node of the first of them add once, the others one by one: near
        // the root a wave walks in step and a node takes thousands, further down the lanes are on nodes of their own
        if (external) {
            const int node = __builtin_amdgcn_readfirstlane(i);
            const unsigned long long same = __ballot(i == node);
            if (i != node)
                atomicAdd(&node_external[i], 1);
            else if ((int)(threadIdx.x & 63) == __ffsll((long long)same) - 1)
                atomicAdd(&node_external[node], (int)__popcll(same));
        }
#elif NNBVH_QUALITY_FOLD == 1
        // every group of externals of this trip that sit on one node adds once
        unsigned long long pending = __ballot(external);
        while (pending) {
            const int leader = __ffsll((long long)pending) - 1;
            const int node = __shfl(i, leader);
            const unsigned long long same = __ballot(external && i == node);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(&node_external[node], (int)__popcll(same));
            pending &= ~same;
        }
#else
        if (external) atomicAdd(&node_external[i], 1);
#endif
        i = inside ? i + 1 : max(end, i + 1);
    }
    k_inner[j] = ki;
    k_leaf[j] = kl;
}

// ---- the sums ------------------------------------------------------------------------------------------------------
// fixed shape: thread t's term at s[t], halving tree, the block's sum at s[0]
template <class T>
__device__ __forceinline__ T block_sum(T v, T *s) {
    const int t = threadIdx.x;
    __syncthreads();
    s[t] = v;
    __syncthreads();
    for (int stride = kQualityBlock / 2; stride > 0; stride >>= 1) {
        if (t < stride) s[t] = s[t] + s[t + stride];
        __syncthreads();
    }
    return s[0];
}

// 2 (xy + xz + yz) of a node's box, in double from its float32 corners
__device__ __forceinline__ double box_area(const float4 &a, const float4 &b) {
    const double x = (double)a.w - (double)a.x, y = (double)b.x - (double)a.y, z = (double)b.y - (double)a.z;
    return 2.0 * (x * y + x * z + y * z);
}

// block partials of the SAH sums: partials[0][blk] = sum of inner box areas, partials[1][blk] = sum of leaf box area
// times nprims, over the block's nodes in index order
__global__ __launch_bounds__(kQualityBlock) void quality_node_partials_kernel(const float4 *__restrict__ rec, int n_nodes,
                                                                               double *__restrict__ partials,
                                                                               int n_blocks) {
    __shared__ double s[kQualityBlock];
    const int n = blockIdx.x * kQualityBlock + threadIdx.x;
    double inner = 0.0, leaf = 0.0;
    if (n < n_nodes) {
        const float4 a = rec[2 * (size_t)n], b = rec[2 * (size_t)n + 1];
        const int nprims = __float_as_int(b.w);
        const double area = box_area(a, b);
        if (nprims == 0)
            inner = area;
        else
            leaf = area * (double)nprims;
    }
    inner = block_sum(inner, s);
    leaf = block_sum(leaf, s);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = inner;
        partials[(size_t)n_blocks + blockIdx.x] = leaf;
    }
}

// block partials of the EPO sums: area, area * k_inner, area * k_leaf (double) and k_inner, k_leaf (int64)
__global__ __launch_bounds__(kQualityBlock) void quality_prim_partials_kernel(const nnbvh_prim *__restrict__ prims,
                                                                               const float *__restrict__ verts,
                                                                               const int32_t *__restrict__ k_inner,
                                                                               const int32_t *__restrict__ k_leaf,
                                                                               int n_prims, double *__restrict__ partials,
                                                                               long long *__restrict__ ipartials,
                                                                               int n_blocks) {
    __shared__ double s[kQualityBlock];
    __shared__ long long si[kQualityBlock];
    const int j = blockIdx.x * kQualityBlock + threadIdx.x;
    double area = 0.0, a_inner = 0.0, a_leaf = 0.0;
    long long ki = 0, kl = 0;
    if (j < n_prims) {
        const nnbvh_prim p = prims[j];
        const float *v0 = verts + 3 * (size_t)p.v[0], *v1 = verts + 3 * (size_t)p.v[1], *v2 = verts + 3 * (size_t)p.v[2];
        const double bx = (double)v1[0] - (double)v0[0], by = (double)v1[1] - (double)v0[1], bz = (double)v1[2] - (double)v0[2];
        const double cx = (double)v2[0] - (double)v0[0], cy = (double)v2[1] - (double)v0[1], cz = (double)v2[2] - (double)v0[2];
        const double ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;
        area = 0.5 * sqrt(ux * ux + uy * uy + uz * uz);
        ki = k_inner[j];
        kl = k_leaf[j];
        a_inner = area * (double)ki;
        a_leaf = area * (double)kl;
    }
    area = block_sum(area, s);
    a_inner = block_sum(a_inner, s);
    a_leaf = block_sum(a_leaf, s);
    ki = block_sum(ki, si);
    kl = block_sum(kl, si);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = area;
        partials[(size_t)n_blocks + blockIdx.x] = a_inner;
        partials[2 * (size_t)n_blocks + blockIdx.x] = a_leaf;
        ipartials[blockIdx.x] = ki;
        ipartials[(size_t)n_blocks + blockIdx.x] = kl;
    }
}

// one block over the partials of `channels` sums: thread t adds partials t, t + 256, ... in that order, then the tree
template <class T>
__global__ __launch_bounds__(kQualityBlock) void quality_final_kernel(const T *__restrict__ partials, int n_blocks,
                                                                       int channels, T *__restrict__ out) {
    __shared__ T s[kQualityBlock];
    for (int c = 0; c < channels; ++c) {
        T v = 0;
        for (int b = threadIdx.x; b < n_blocks; b += kQualityBlock) v = v + partials[(size_t)c * n_blocks + b];
        v = block_sum(v, s);
        if (threadIdx.x == 0) out[c] = v;
    }
}

// ---- launchers -----------------------------------------------------------------------------------------------------
hipError_t launch_quality_prepare(const QualityBuffers &b, hipStream_t stream) {
    hipLaunchKernelGGL(quality_prepare_kernel, dim3(quality_blocks(b.n_nodes)), dim3(kQualityBlock), 0, stream, b.nodes,
                       b.n_nodes, b.n_prims, b.rec, b.leaf_of, b.node_external);
    return hipGetLastError();
}

hipError_t launch_quality_walk(const QualityBuffers &b, hipStream_t stream) {
    hipLaunchKernelGGL(quality_walk_kernel, dim3(quality_blocks(b.n_prims)), dim3(kQualityBlock), 0, stream, b.rec,
                       b.n_nodes, b.prims, b.verts, b.leaf_of, b.n_prims, b.k_inner, b.k_leaf, b.node_external);
    return hipGetLastError();
}

hipError_t launch_quality_reduce(const QualityBuffers &b, hipStream_t stream) {
    const int nb_nodes = quality_blocks(b.n_nodes), nb_prims = quality_blocks(b.n_prims);
    hipLaunchKernelGGL(quality_node_partials_kernel, dim3(nb_nodes), dim3(kQualityBlock), 0, stream, b.rec, b.n_nodes,
                       b.partials, nb_nodes);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(quality_final_kernel<double>, dim3(1), dim3(kQualityBlock), 0, stream, b.partials, nb_nodes, 2,
                       b.sums);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // the partials array is reused: the launches of one stream are ordered
    hipLaunchKernelGGL(quality_prim_partials_kernel, dim3(nb_prims), dim3(kQualityBlock), 0, stream, b.prims, b.verts,
                       b.k_inner, b.k_leaf, b.n_prims, b.partials, b.ipartials, nb_prims);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(quality_final_kernel<double>, dim3(1), dim3(kQualityBlock), 0, stream, b.partials, nb_prims, 3,
                       b.sums + 2);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(quality_final_kernel<long long>, dim3(1), dim3(kQualityBlock), 0, stream, b.ipartials, nb_prims, 2,
                       b.isums);
    return hipGetLastError();
}

}  // namespace nnbvh
