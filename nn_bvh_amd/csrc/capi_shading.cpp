// capi_shading.cpp — the C ABI of include/nnbvh.h, shading part: shading meshes and the
// Triangle::InteractionFromIntersection post-pass (shapes.h:884-1010).  Host code only.
#include <cstring>
#include <vector>

#include "capi_internal.h"

using namespace nnbvh;

static_assert(sizeof(nnbvh_interaction) == 192, "nnbvh_interaction must be 192 bytes");

template <typename T>
static bool upload(T **dst, const T *src, size_t count, const char *what) {
    *dst = nullptr;
    if (!src || count == 0) return true;
    return hip_ok(hipMalloc((void **)dst, count * sizeof(T)), what) &&
           hip_ok(hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice), what);
}

extern "C" {

nnbvh_shading_mesh *nnbvh_shading_mesh_create(const float *verts, int n_verts,
                                              const int32_t *tri_vertices,
                                              const int32_t *patch_vertices, int n_tris,
                                              const float *normals, const float *uvs,
                                              const float *tangents, const int32_t *face_indices,
                                              const uint8_t *tri_flags, int device) {
    if (!verts || !tri_vertices || n_verts <= 0 || n_tris <= 0) {
        set_error("shading_mesh_create: empty vertex or triangle array");
        return nullptr;
    }
    for (long i = 0; i < 3L * n_tris; ++i) {
        const int v = tri_vertices[i];
        const bool not_a_triangle = tri_vertices[i - i % 3] < 0;
        if (!not_a_triangle && (v < 0 || v >= n_verts)) {
            set_error("shading_mesh_create: vertex index out of range");
            return nullptr;
        }
    }
    for (long i = 0; patch_vertices && i < 4L * n_tris; ++i) {
        const int v = patch_vertices[i];
        const bool not_a_patch = patch_vertices[i - i % 4] < 0;
        if (!not_a_patch && (v < 0 || v >= n_verts)) {
            set_error("shading_mesh_create: patch vertex index out of range");
            return nullptr;
        }
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    auto *m = new nnbvh_shading_mesh;
    m->device = device;
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) {
        delete m;
        return nullptr;
    }
    m->n_cus = prop.multiProcessorCount;
    m->d.nTris = n_tris;
    m->d.nVerts = n_verts;
    m->d.defaultFlags = (uvs ? NNBVH_TRI_HAS_UV : 0) | (normals ? NNBVH_TRI_HAS_N : 0) |
                        (tangents ? NNBVH_TRI_HAS_S : 0);
    const bool ok = upload(&m->d.verts, verts, 3 * (size_t)n_verts, "shading mesh: vertices") &&
                    upload(&m->d.triVerts, tri_vertices, 3 * (size_t)n_tris, "shading mesh: indices") &&
                    upload(&m->d.patchVerts, patch_vertices, 4 * (size_t)n_tris, "shading mesh: patch indices") &&
                    upload(&m->d.normals, normals, 3 * (size_t)n_verts, "shading mesh: normals") &&
                    upload(&m->d.uvs, uvs, 2 * (size_t)n_verts, "shading mesh: uvs") &&
                    upload(&m->d.tangents, tangents, 3 * (size_t)n_verts, "shading mesh: tangents") &&
                    upload(&m->d.faceIndices, face_indices, (size_t)n_tris, "shading mesh: face indices") &&
                    upload(&m->d.triFlags, tri_flags, (size_t)n_tris, "shading mesh: flags");
    if (!ok) {
        nnbvh_shading_mesh_destroy(m);
        return nullptr;
    }
    return m;
}

int nnbvh_shading_mesh_set_instances(nnbvh_shading_mesh *m, const nnbvh_instance *instances, int n_instances) {
    if (!m || n_instances < 0 || (n_instances > 0 && !instances)) {
        set_error("shading_mesh_set_instances: bad argument");
        return NNBVH_ERR_ARG;
    }
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    if (m->d.instances) (void)hipFree(m->d.instances);
    m->d.instances = nullptr;
    m->d.nInstances = 0;
    // the animation tables describe the table they came with: a new instance table starts without them
    // (surface_interaction indexes m.anim by the instance of the NEW table)
    for (float **p : {&m->d.anim, &m->d.animFwd}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (n_instances == 0) return NNBVH_OK;
    if (!upload(&m->d.instances, instances, (size_t)n_instances, "shading mesh: instances")) return NNBVH_ERR_DEVICE;
    m->d.nInstances = n_instances;
    return NNBVH_OK;
}

int nnbvh_shading_mesh_set_instances_animated(nnbvh_shading_mesh *m, const nnbvh_instance *instances,
                                              const nnbvh_animated_transform *animated, int n_instances) {
    int rc = nnbvh_shading_mesh_set_instances(m, instances, n_instances);
    if (rc != NNBVH_OK) return rc;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    for (float **p : {&m->d.anim, &m->d.animFwd}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    if (!animated || n_instances == 0) return NNBVH_OK;
    std::vector<float> table((size_t)n_instances * kAnimStride, 0.0f), fwd((size_t)n_instances * 24);
    for (int k = 0; k < n_instances; ++k) {
        fill_anim_entry(animated[k], &table[(size_t)k * kAnimStride]);
        std::memcpy(&fwd[(size_t)k * 24], animated[k].start_from, 48);       // rows 0..2 of startTransform.m
        std::memcpy(&fwd[(size_t)k * 24 + 12], animated[k].end_from, 48);    // ... of endTransform.m
    }
    if (!upload(&m->d.anim, table.data(), table.size(), "shading mesh: animation table") ||
        !upload(&m->d.animFwd, fwd.data(), fwd.size(), "shading mesh: animation table"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

void nnbvh_shading_mesh_destroy(nnbvh_shading_mesh *m) {
    if (!m) return;
    DeviceGuard guard(m->device);
    if (m->d.instances) (void)hipFree(m->d.instances);
    if (m->d.anim) (void)hipFree(m->d.anim);
    if (m->d.animFwd) (void)hipFree(m->d.animFwd);
    void *ptrs[] = {m->d.verts, m->d.triVerts, m->d.patchVerts, m->d.normals, m->d.uvs, m->d.tangents, m->d.faceIndices, m->d.triFlags};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

int nnbvh_triangle_interactions_device(const nnbvh_shading_mesh *m, const void *d_rays,
                                       const nnbvh_ray_soa *ray_soa, const void *d_hits,
                                       int32_t max_items, const int32_t *d_size, void *d_out,
                                       void *stream) {
    const bool soa_given = ray_soa && ray_soa->dx && ray_soa->dy && ray_soa->dz;
    if (!m || max_items < 0 || (max_items > 0 && (!d_hits || !d_out || (!d_rays && !soa_given)))) {
        set_error("triangle_interactions_device: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (max_items == 0) return NNBVH_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    if (!hip_ok(launch_triangle_interactions(m->d, d_rays, d_rays ? nullptr : ray_soa, d_hits, max_items, d_size,
                                             d_out, m->n_cus * 8, (hipStream_t)stream),
                "interaction kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

int nnbvh_triangle_interactions(const nnbvh_shading_mesh *m, const nnbvh_ray *rays, const nnbvh_hit *hits,
                                int32_t n, nnbvh_interaction *out) {
    if (!m || n < 0 || (n > 0 && (!rays || !hits || !out))) {
        set_error("triangle_interactions: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    void *d_rays = nullptr, *d_hits = nullptr, *d_out = nullptr;
    int rc = NNBVH_ERR_DEVICE;
    if (hip_ok(hipMalloc(&d_rays, (size_t)n * sizeof(nnbvh_ray)), "hipMalloc(rays)") &&
        hip_ok(hipMalloc(&d_hits, (size_t)n * sizeof(nnbvh_hit)), "hipMalloc(hits)") &&
        hip_ok(hipMalloc(&d_out, (size_t)n * sizeof(nnbvh_interaction)), "hipMalloc(interactions)") &&
        hip_ok(hipMemcpy(d_rays, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays") &&
        hip_ok(hipMemcpy(d_hits, hits, (size_t)n * sizeof(nnbvh_hit), hipMemcpyHostToDevice), "copy hits") &&
        hip_ok(launch_triangle_interactions(m->d, d_rays, nullptr, d_hits, n, nullptr, d_out, m->n_cus * 8, nullptr),
               "interaction kernel launch") &&
        hip_ok(hipMemcpy(out, d_out, (size_t)n * sizeof(nnbvh_interaction), hipMemcpyDeviceToHost), "copy interactions"))
        rc = NNBVH_OK;
    for (void *p : {d_rays, d_hits, d_out})
        if (p) (void)hipFree(p);
    return rc;
}

}  // extern "C"
