// kd_build_gpu.h — interface between the kd-tree C ABI (kd_build.cpp), the device builder (kd_build_gpu.hip) and the
// device-side scene creation (kd_bake.hip).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/nnbvh.h"

namespace nnbvh {

// Makes `device` current for a scope and puts the caller's device back on every way out of it.
struct ScopedDevice {
    int prev = -1;
    hipError_t status = hipSuccess;
    explicit ScopedDevice(int device) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        status = hipSetDevice(device);
    }
    ~ScopedDevice() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    ScopedDevice(const ScopedDevice &) = delete;
    ScopedDevice &operator=(const ScopedDevice &) = delete;
};

// The builder's two output arrays, resident on the device.  The holder owns them until release().
struct KdGpuTree {
    nnbvh_kd_node *d_nodes = nullptr;
    int32_t *d_indices = nullptr;  // max(n_indices, 1) entries
    int n_nodes = 0, n_indices = 0;
    int depth = 0;   // edges root -> deepest node
    int levels = 0;
    KdGpuTree() = default;
    KdGpuTree(const KdGpuTree &) = delete;
    KdGpuTree &operator=(const KdGpuTree &) = delete;
    ~KdGpuTree() {
        if (d_nodes) (void)hipFree(d_nodes);
        if (d_indices) (void)hipFree(d_indices);
    }
    void release() { d_nodes = nullptr, d_indices = nullptr; }
};

struct KdGpuResult {
    std::vector<nnbvh_kd_node> nodes;
    std::vector<int32_t> prim_indices;
    int depth = 0;
    int levels = 0;
    double device_ms = 0;  // upload of the primitive bounds .. the two output arrays written on the device
    double total_ms = 0;   // ... and downloaded
};

// The device builder proper.  d_prim_bounds: 6 floats (min, max) per primitive ON THE DEVICE, finite (the caller
// validated them); bounds = their union.  The caller has made the device current; everything runs on `stream` (the
// builder's read-backs synchronise it), all scratch is freed on return, and on success the stream is idle and *out
// owns the two arrays.  Same node array as the host builder; primitives inside multi-primitive leaves in
// std::stable_sort order (see the note at the top of kd_build_gpu.hip).
bool gpu_kd_build_device(const float *d_prim_bounds, int n_prims, const float bounds[6], int isect_cost,
                         int traversal_cost, float empty_bonus, int max_prims, int max_depth, hipStream_t stream,
                         KdGpuTree *out, std::string *error);

// ... from host bounds to host arrays (nnbvh_kd_build_create_gpu): upload, gpu_kd_build_device, download, on a stream
// of its own with the caller's current device restored.
bool gpu_kd_build(const float *prim_bounds, int n_prims, const float bounds[6], int isect_cost, int traversal_cost,
                  float empty_bonus, int max_prims, int max_depth, int device, KdGpuResult *out, std::string *error);

// What the device found wrong with the primitive list of nnbvh_kd_scene_create_gpu_build (kd_bake.hip), in the order
// kd_prepare (kd_build.cpp) checks one primitive; the C ABI turns it into kd_prepare's message.
enum KdPrimFault { kKdPrimOk = 0, kKdHostNeedsBounds = 1, kKdBadKind = 2, kKdBadVertexIndex = 3, kKdNonFinite = 4 };

struct KdSceneInputs {
    const nnbvh_prim *prims;
    int n_prims;
    const float *verts;
    int n_verts;
    const float *prim_bounds, *normals, *uvs, *prim_alpha;  // nullable
    int isect_cost, traversal_cost, max_prims, max_depth;   // max_depth resolved and checked by the caller
    float empty_bonus;
    int device;                                             // checked by the caller
    // the alpha-texture table the kinds 16 .. 19 index with v[3], checked by the caller (check_alpha_textures); null:
    // the caller has refused those kinds
    const nnbvh_alpha_texture *textures;
    int n_textures;
};

// The 64-B primitive records of a kd scene, in the order of d_prims, and with any_attr its 96-B attribute slots (else
// *d_extras = nullptr), baked from device arrays on `stream` (kd_bake.hip; the device is current, the list and what its
// kinds read have been checked).  Both results are hipMalloc'ed and the caller's; the stream is idle on return.
bool kd_bake_records(const nnbvh_prim *d_prims, int n_prims, const float *d_verts, const float *d_normals,
                     const float *d_uvs, const float *d_prim_alpha, bool any_attr, hipStream_t stream, void **d_rec,
                     void **d_extras, std::string *error);

// Triangles in, traceable kd scene out; the tree never visits the host (kd_bake.hip).  nullptr with *fault set for a
// bad primitive list, else nullptr with *error set.
nnbvh_kd_scene *kd_scene_create_on_device(const KdSceneInputs &in, KdPrimFault *fault, std::string *error);

}  // namespace nnbvh
