// kd_bake.hip — the primitive records and attribute slots of every kd-tree scene (kd_bake_records: the ONE writer of
// that layout, for the caller's tree uploaded by capi_kd.cpp and for the device-built one; tests/test_bake_golden.py
// holds its bytes to a recording), and a kd-tree scene created entirely on the device
// (nnbvh_kd_scene_create_gpu_build): the primitive bounds kd_prepare (kd_build.cpp) computes on the host, their union,
// the device builder (kd_build_gpu.hip) with its result left where it is, and the records — bit for bit the scene of
// nnbvh_kd_build_create_stable + nnbvh_kd_scene_create_with_attributes, without the tree's round trip through host
// memory.
//
//   k_kd_prim_bounds   one lane per primitive: kind and vertex indices are checked BEFORE anything is gathered with
//                      them (the list is the caller's, unvalidated); Triangle::Bounds / BilinearPatch::Bounds in the
//                      host's operand order; the lowest failing primitive and its reason, the six extremes of the
//                      union and five scene flags reduced per wave, per block, then one atomic each
//   k_kd_host_bounds   scenes with NNBVH_PRIM_HOST entries only: their rows of the caller's prim_bounds
//   k_kd_union_pick    the union's six floats are the winners' own bit patterns (the sign of a zero is that of the
//                      lowest-indexed primitive that reaches the extreme, as in the host's sequential union)
//   k_kd_bake          one lane per primitive: its 64-B record and, in scenes that have them, its 96-B attribute slots
// All four are streaming passes; nothing here runs while rays are traced.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <limits>
#include <string>

#include "kd_build_gpu.h"
#include "kd_device_util.h"
#include "kd_trace.h"
#include "nnbvh_internal.h"

namespace nnbvh {
namespace {

constexpr int kBb = 256;
constexpr unsigned kFlagHostKind = 1u;  // an NNBVH_PRIM_HOST entry: the caller's prim_bounds rows are needed
constexpr unsigned kFlagAnyAttr = 2u;   // a kind that reads the 96-B attribute slots
constexpr unsigned kFlagHasHost = 4u;   // nnbvh_kd_scene::has_host_prims
constexpr unsigned kFlagHasPatch = 8u;  // nnbvh_kd_scene::has_patches
constexpr unsigned kFlagAlphaTex = 16u;  // nnbvh_kd_scene::has_alpha_tex: a textured triangle (kPrimAlphaTex record)

// what the bounds passes reduce into; uploaded as {~0, {~0 x 6}, 0, ...}
struct KdPrep {
    unsigned long long fault;   // primitive << 8 | KdPrimFault of the lowest failing primitive
    unsigned long long key[6];  // per extreme: value (-0 and +0 equal) << 32 | primitive, smallest wins
    unsigned flags;
    unsigned pad;
    float bounds[6];
};

struct KdHave {  // which optional arrays the caller gave; alphaTex: an alpha-texture table (kinds 16 .. 19 are known)
    int primBounds, normals, uvs, primAlpha, alphaTex;
};

// std::min / std::max as kd_build.cpp's KBox code uses them: the FIRST of equals (and of a NaN pair) is kept
__device__ __forceinline__ float first_min(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float first_max(float a, float b) { return a < b ? b : a; }

// 0: not a kind with vertices.  A textured triangle (kinds 16 .. 19, scenes with an alpha-texture table) has three:
// its v[3] is the texture index, which the host has checked
__device__ __forceinline__ int kd_vertex_count(int kind, bool alphaTex) {
    return (is_triangle_kind(kind) || (alphaTex && is_alphatex_kind(kind))) ? 3
           : (kind == NNBVH_PRIM_BILINEAR_PATCH || is_alpha_patch_kind(kind)) ? 4 : 0;
}

// block-wide minimum of the seven 64-bit words of a lane, then one atomicMin per word and block
__device__ __forceinline__ void block_min_to(unsigned long long fault, const unsigned long long key[6], unsigned flags,
                                             KdPrep *out) {
    __shared__ unsigned long long part[kBb / 64][7];
    __shared__ unsigned flagPart[kBb / 64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long w[7];
    w[0] = kd_wave_min_u64(fault);
#pragma unroll
    for (int k = 0; k < 6; ++k) w[1 + k] = kd_wave_min_u64(key[k]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) flags |= __shfl_xor(flags, off);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 7; ++k) part[wave][k] = w[k];
        flagPart[wave] = flags;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        unsigned long long m = part[0][threadIdx.x];
        for (int q = 1; q < kBb / 64; ++q) m = part[q][threadIdx.x] < m ? part[q][threadIdx.x] : m;
        if (m != ~0ull) atomicMin(threadIdx.x == 0 ? &out->fault : &out->key[threadIdx.x - 1], m);
    } else if (threadIdx.x == 7) {
        unsigned f = 0;
        for (int q = 0; q < kBb / 64; ++q) f |= flagPart[q];
        if (f) atomicOr(&out->flags, f);
    }
}

// the six keys of a finite box: minima as they are, maxima inverted, so that the smallest key is the extreme of the
// lowest-indexed primitive
__device__ __forceinline__ void box_keys(const float b[6], int i, unsigned long long key[6]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        key[k] = ((unsigned long long)kd_ordered_bits(b[k]) << 32) | (unsigned)i;
        key[3 + k] = ((unsigned long long)(~kd_ordered_bits(b[3 + k])) << 32) | (unsigned)i;
    }
}
__device__ __forceinline__ bool box_finite(const float b[6]) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 6; ++k) ok = ok && __builtin_isfinite(b[k]);
    return ok;
}

__global__ __launch_bounds__(kBb) void k_kd_prim_bounds(const nnbvh_prim *__restrict__ prims, int n,
                                                       const float *__restrict__ verts, int nVerts, KdHave have,
                                                       float *__restrict__ pb, KdPrep *out) {
    const int i = blockIdx.x * kBb + threadIdx.x;
    unsigned long long fault = ~0ull, key[6] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    unsigned flags = 0;
    if (i < n) {
        const nnbvh_prim p = prims[i];
        const int nv = kd_vertex_count(p.kind, have.alphaTex != 0);
        int why = kKdPrimOk;
        if (p.kind == NNBVH_PRIM_HOST) {
            // its box comes from the caller's row, in k_kd_host_bounds once that array is on the device
            if (!have.primBounds) why = kKdHostNeedsBounds;
            flags |= kFlagHostKind | kFlagHasHost;
        } else if (!nv) {
            why = kKdBadKind;
        } else {
            for (int k = 0; k < nv; ++k)
                if (p.v[k] < 0 || p.v[k] >= nVerts) why = kKdBadVertexIndex;
            if (why == kKdPrimOk) {  // only now is anything read through the indices
                float v[4][3];
                for (int k = 0; k < nv; ++k)
                    for (int c = 0; c < 3; ++c) v[k][c] = verts[3 * (long)p.v[k] + c];
                float b[6];
                for (int c = 0; c < 3; ++c) {
                    if (nv == 3) {  // Union(Bounds3f(p0, p1), p2), shapes.cpp:294-300
                        b[c] = first_min(first_min(v[0][c], v[1][c]), v[2][c]);
                        b[3 + c] = first_max(first_max(v[0][c], v[1][c]), v[2][c]);
                    } else {        // Union(Bounds3f(p00, p01), Bounds3f(p10, p11)), shapes.cpp:1073-1080
                        b[c] = first_min(first_min(v[0][c], v[2][c]), first_min(v[1][c], v[3][c]));
                        b[3 + c] = first_max(first_max(v[0][c], v[2][c]), first_max(v[1][c], v[3][c]));
                    }
                }
                for (int c = 0; c < 6; ++c) pb[6 * (long)i + c] = b[c];
                if (box_finite(b)) box_keys(b, i, key);
                else why = kKdNonFinite;
            }
            // the scene flags, as capi_kd.cpp computes them for a caller's tree
            const bool attr = kd_attr_on_device(p.kind, have.normals, have.uvs, have.primAlpha);
            if (is_alphatex_kind(p.kind)) flags |= kFlagHasHost | kFlagHasPatch | kFlagAnyAttr | kFlagAlphaTex;
            else if ((is_smooth_alpha_kind(p.kind) || is_alpha_patch_kind(p.kind)) && !attr) flags |= kFlagHasHost;
            else if (attr || is_flat_alpha_kind(p.kind)) flags |= kFlagHasHost | kFlagHasPatch | (attr ? kFlagAnyAttr : 0u);
            else if (nv == 4) flags |= kFlagHasPatch;
        }
        if (why != kKdPrimOk) fault = ((unsigned long long)(unsigned)i << 8) | (unsigned)why;
    }
    block_min_to(fault, key, flags, out);
}

__global__ __launch_bounds__(kBb) void k_kd_host_bounds(const nnbvh_prim *__restrict__ prims, int n,
                                                       const float *__restrict__ primBounds, float *__restrict__ pb,
                                                       KdPrep *out) {
    const int i = blockIdx.x * kBb + threadIdx.x;
    unsigned long long fault = ~0ull, key[6] = {~0ull, ~0ull, ~0ull, ~0ull, ~0ull, ~0ull};
    if (i < n && prims[i].kind == NNBVH_PRIM_HOST) {
        float b[6];
        for (int c = 0; c < 6; ++c) pb[6 * (long)i + c] = b[c] = primBounds[6 * (long)i + c];
        if (box_finite(b)) box_keys(b, i, key);
        else fault = ((unsigned long long)(unsigned)i << 8) | (unsigned)kKdNonFinite;
    }
    block_min_to(fault, key, 0u, out);
}

__global__ void k_kd_union_pick(const float *__restrict__ pb, KdPrep *out) {
    const int k = threadIdx.x;
    if (k < 6 && out->key[k] != ~0ull) out->bounds[k] = pb[6 * (long)(unsigned)out->key[k] + k];
}

__global__ __launch_bounds__(kBb) void k_kd_bake(const nnbvh_prim *__restrict__ prims, int n,
                                                const float *__restrict__ verts, const float *__restrict__ normals,
                                                const float *__restrict__ uvs, const float *__restrict__ primAlpha,
                                                float4 *__restrict__ rec, float4 *__restrict__ extras) {
    const int i = blockIdx.x * kBb + threadIdx.x;
    if (i >= n) return;
    const nnbvh_prim p = prims[i];
    const bool attr = kd_attr_on_device(p.kind, normals != nullptr, uvs != nullptr, primAlpha != nullptr);
    const bool tex = is_alphatex_kind(p.kind);  // (only scenes with an alpha-texture table get this far with one)
    const int nv = (is_triangle_kind(p.kind) || tex) ? 3 : 4;
    float s[16], ex[24];
    for (int k = 0; k < 16; ++k) s[k] = 0.0f;
    for (int k = 0; k < 24; ++k) ex[k] = 0.0f;
    unsigned flags = 0;
    if (p.kind == NNBVH_PRIM_HOST || ((is_smooth_alpha_kind(p.kind) || is_alpha_patch_kind(p.kind)) && !attr)) {
        flags = kPrimHost;  // no geometry: the host's
    } else {
        if (attr) {
            const bool smooth = is_smooth_alpha_kind(p.kind) || is_smooth_alpha_patch_kind(p.kind);
            for (int j = 0; j < nv && smooth; ++j)
                for (int c = 0; c < 3; ++c) ex[4 * j + c] = normals[3 * (long)p.v[j] + c];
            for (int j = 0; j < 4 && is_uv_alpha_patch_kind(p.kind); ++j)
                for (int c = 0; c < 2; ++c) ex[16 + 2 * j + c] = uvs[2 * (long)p.v[j] + c];
            flags |= kPrimAlpha | (smooth ? kPrimSmooth : 0u) | (is_uv_alpha_patch_kind(p.kind) ? kPrimUV : 0u);
            if (p.kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED || is_flipped_alpha_patch_kind(p.kind)) flags |= kPrimFlipN;
        }
        if (tex) {
            // normals in slots 0 .. 2 (smooth kinds), the three (u, v) pairs — the mesh's or
            // the default corners (0,0), (1,0), (1,1) — in slots 4 / 5, the texture index (v[3]) in slot 2's w below
            const bool smooth = is_smooth_alphatex_kind(p.kind);
            for (int j = 0; j < 3 && smooth; ++j)
                for (int c = 0; c < 3; ++c) ex[4 * j + c] = normals[3 * (long)p.v[j] + c];
            for (int j = 0; j < 3; ++j) {
                ex[16 + 2 * j] = uvs ? uvs[2 * (long)p.v[j]] : (j == 0 ? 0.0f : 1.0f);
                ex[16 + 2 * j + 1] = uvs ? uvs[2 * (long)p.v[j] + 1] : (j == 2 ? 1.0f : 0.0f);
            }
            flags |= kPrimAlpha | kPrimAlphaTex | (smooth ? kPrimSmooth : 0u) | (is_flipped_alphatex_kind(p.kind) ? kPrimFlipN : 0u);
        }
        if (is_flat_alpha_kind(p.kind)) flags |= kPrimAlpha | (p.kind == NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED ? kPrimFlipN : 0u);
        for (int j = 0; j < nv; ++j)
            for (int c = 0; c < 3; ++c) s[4 * j + c] = verts[3 * (long)p.v[j] + c];
        if (flags & kPrimAlpha) s[11] = is_alpha_patch_kind(p.kind) ? primAlpha[i] : __int_as_float(p.v[3]);
        if (nv == 4) flags |= kPrimPatch;
        else if (kd_triangle_is_degenerate(&s[0], &s[4], &s[8])) flags |= kPrimDegenerate;
    }
    s[3] = __int_as_float(p.id);
    s[7] = __uint_as_float(flags);
    float4 *r = rec + 4 * (long)i;
    for (int q = 0; q < 4; ++q) r[q] = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
    if (extras) {
        float4 *e = extras + 6 * (long)i;
        for (int q = 0; q < 6; ++q) e[q] = make_float4(ex[4 * q], ex[4 * q + 1], ex[4 * q + 2], ex[4 * q + 3]);
    }
}

struct DevMem {  // device allocations of one call, freed on every way out unless taken
    void *ptrs[12] = {};
    int n = 0;
    void *get(size_t bytes) {
        void *p = nullptr;
        if (n >= 12 || hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        return ptrs[n++] = p;
    }
    void free_one(void *p) {
        for (int k = 0; k < n; ++k)
            if (ptrs[k] == p && p) {
                (void)hipFree(p);
                ptrs[k] = nullptr;
            }
    }
    void *take(void *p) {  // no longer this holder's
        for (int k = 0; k < n; ++k)
            if (ptrs[k] == p) ptrs[k] = nullptr;
        return p;
    }
    ~DevMem() {
        for (int k = 0; k < n; ++k)
            if (ptrs[k]) (void)hipFree(ptrs[k]);
    }
};

struct OwnStream {
    hipStream_t s = nullptr;
    ~OwnStream() {
        if (s) (void)hipStreamDestroy(s);
    }
};

inline int grid_of(long n) { return (int)((n + kBb - 1) / kBb); }

}  // namespace

#define KB_CHECK(expr, what)                                                                 \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            *error = std::string("device kd scene: ") + what + ": " + hipGetErrorString(e_); \
            return nullptr;                                                                  \
        }                                                                                    \
    } while (0)

bool kd_bake_records(const nnbvh_prim *d_prims, int n_prims, const float *d_verts, const float *d_normals,
                     const float *d_uvs, const float *d_prim_alpha, bool any_attr, hipStream_t stream, void **d_rec,
                     void **d_extras, std::string *error) {
    DevMem mem;
    auto *dRec = (float4 *)mem.get((size_t)n_prims * 64);
    auto *dExtras = any_attr ? (float4 *)mem.get((size_t)n_prims * 96) : nullptr;
    if (!dRec || (any_attr && !dExtras)) {
        *error = "device kd scene: hipMalloc(primitive records) failed";
        return false;
    }
    hipLaunchKernelGGL(k_kd_bake, dim3(grid_of(n_prims)), dim3(kBb), 0, stream, d_prims, n_prims, d_verts, d_normals, d_uvs,
                       d_prim_alpha, dRec, dExtras);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        *error = std::string("device kd scene: bake kernel: ") + hipGetErrorString(e);
        return false;
    }
    *d_rec = mem.take(dRec);
    *d_extras = mem.take(dExtras);
    return true;
}

nnbvh_kd_scene *kd_scene_create_on_device(const KdSceneInputs &in, KdPrimFault *fault, std::string *error) {
    *fault = kKdPrimOk;
    const int n = in.n_prims;
    ScopedDevice guard(in.device);  // the caller's current device comes back on every return below
    KB_CHECK(guard.status, "hipSetDevice");
    hipDeviceProp_t prop;
    KB_CHECK(hipGetDeviceProperties(&prop, in.device), "hipGetDeviceProperties");
    OwnStream own;
    KB_CHECK(hipStreamCreateWithFlags(&own.s, hipStreamNonBlocking), "hipStreamCreate");
    hipStream_t stream = own.s;

    // ---- the caller's arrays, once --------------------------------------------------------------------------
    DevMem mem;
    auto upload = [&](const void *src, size_t bytes) -> void * {
        void *d = mem.get(bytes);
        if (d && hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, stream) != hipSuccess) return nullptr;
        return d;
    };
    const size_t nv = (size_t)in.n_verts;
    auto *dPrims = (nnbvh_prim *)upload(in.prims, (size_t)n * sizeof(nnbvh_prim));
    auto *dVerts = (float *)upload(in.verts, nv * 12);
    auto *dNormals = in.normals ? (float *)upload(in.normals, nv * 12) : nullptr;
    auto *dUVs = in.uvs ? (float *)upload(in.uvs, nv * 8) : nullptr;
    auto *dAlpha = in.prim_alpha ? (float *)upload(in.prim_alpha, (size_t)n * 4) : nullptr;
    auto *dPB = (float *)mem.get((size_t)n * 24);
    KdPrep prep;
    std::memset(&prep, 0xff, sizeof prep.fault + sizeof prep.key);
    prep.flags = prep.pad = 0;
    // Bounds3f() of the host's sequential union, for the extremes no primitive reaches (none: every box is finite)
    for (int k = 0; k < 3; ++k) prep.bounds[k] = std::numeric_limits<float>::max(), prep.bounds[3 + k] = std::numeric_limits<float>::lowest();
    auto *dPrep = (KdPrep *)upload(&prep, sizeof prep);
    if (!dPrims || !dVerts || (in.normals && !dNormals) || (in.uvs && !dUVs) || (in.prim_alpha && !dAlpha) || !dPB || !dPrep) {
        *error = "device kd scene: hipMalloc or upload failed";
        return nullptr;
    }

    // ---- bounds, validation, union ---------------------------------------------------------------------------
    const KdHave have{in.prim_bounds != nullptr, in.normals != nullptr, in.uvs != nullptr, in.prim_alpha != nullptr,
                      in.textures != nullptr && in.n_textures > 0};
    hipLaunchKernelGGL(k_kd_prim_bounds, dim3(grid_of(n)), dim3(kBb), 0, stream, dPrims, n, dVerts, in.n_verts, have, dPB, dPrep);
    hipLaunchKernelGGL(k_kd_union_pick, dim3(1), dim3(64), 0, stream, dPB, dPrep);
    KB_CHECK(hipGetLastError(), "bounds kernels");
    KB_CHECK(hipMemcpyAsync(&prep, dPrep, sizeof prep, hipMemcpyDeviceToHost, stream), "read bounds result");
    KB_CHECK(hipStreamSynchronize(stream), "bounds kernels");
    if ((prep.flags & kFlagHostKind) && in.prim_bounds) {
        // only these rows are ever read, so only such scenes upload the array
        auto *dCaller = (float *)upload(in.prim_bounds, (size_t)n * 24);
        if (!dCaller) {
            *error = "device kd scene: hipMalloc or upload failed";
            return nullptr;
        }
        hipLaunchKernelGGL(k_kd_host_bounds, dim3(grid_of(n)), dim3(kBb), 0, stream, dPrims, n, dCaller, dPB, dPrep);
        hipLaunchKernelGGL(k_kd_union_pick, dim3(1), dim3(64), 0, stream, dPB, dPrep);
        KB_CHECK(hipGetLastError(), "host-primitive bounds kernels");
        KB_CHECK(hipMemcpyAsync(&prep, dPrep, sizeof prep, hipMemcpyDeviceToHost, stream), "read bounds result");
        KB_CHECK(hipStreamSynchronize(stream), "host-primitive bounds kernels");
        mem.free_one(dCaller);
    }
    if (prep.fault != ~0ull) {
        *fault = (KdPrimFault)(prep.fault & 0xffu);
        return nullptr;
    }

    // ---- the tree, left on the device ------------------------------------------------------------------------
    KdGpuTree tree;
    if (!gpu_kd_build_device(dPB, n, prep.bounds, in.isect_cost, in.traversal_cost, in.empty_bonus, in.max_prims,
                             in.max_depth, stream, &tree, error))
        return nullptr;
    mem.free_one(dPB);  // with the builder's scratch gone too, the bake allocates into the room they left
    mem.free_one(dPrep);

    // ---- primitive records -------------------------------------------------------------------------------------
    void *dRec = nullptr, *dExtras = nullptr;
    if (!kd_bake_records(dPrims, n, dVerts, dNormals, dUVs, dAlpha, (prep.flags & kFlagAnyAttr) != 0, stream, &dRec, &dExtras,
                         error))
        return nullptr;

    // (depth <= max_depth <= 64 by the caller's check: the tree is the library's own, nothing to validate)
    nnbvh_kd_scene *s = kd_new_scene(in.device, prop.multiProcessorCount, tree.depth, (prep.flags & kFlagHasHost) != 0,
                                     (prep.flags & kFlagHasPatch) != 0, tree.n_nodes, tree.n_indices, n, prep.bounds);
    s->d_nodes = (uint2 *)tree.d_nodes;
    s->d_indices = tree.d_indices;
    tree.release();
    s->d_prims = (float4 *)dRec;
    s->d_extras = (float4 *)dExtras;
    s->has_alpha_tex = (prep.flags & kFlagAlphaTex) ? 1 : 0;
    // the descriptor table and the texel pool are the only arrays of such a scene that come from the host
    if (have.alphaTex && !kd_attach_alpha_textures(s, in.textures, in.n_textures)) {
        *error = nnbvh_last_error();
        return nullptr;
    }
    return s;
}

}  // namespace nnbvh
