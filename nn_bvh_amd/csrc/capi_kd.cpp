// capi_kd.cpp — the C ABI of include/nnbvh.h, kd-tree scenes: creation from the caller's tree (its validation, the
// upload, and the primitive records baked by kd_bake.hip as for a device-built tree), the read-side calls, the launchers of kd_trace.hip's instances and the ray-batch
// calls on device and host buffers.  (The queue calls: capi_wavefront.cpp; the builders: kd_build.cpp.)  Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"
#include "kd_build_gpu.h"
#include "wavefront.h"

using namespace nnbvh;

KdWorkspace *nnbvh::kd_workspace_for(nnbvh_kd_scene *s, hipStream_t stream) {
    auto it = s->workspaces.find(stream);
    if (it != s->workspaces.end()) return &it->second;
    KdWorkspace w;
    // an entry is spilled only when W newer ones sit above it: levels 0 .. depth - W of a lane's list, at the
    // smallest window any instance runs with
    const size_t spill_levels = (size_t)std::max(s->depth + 1 - std::min(kKdW, kKdWLean), 1);
    const size_t spill_bytes = spill_levels * (size_t)s->n_cus * 8 * kKdBlock * sizeof(float4);
    if (!hip_ok(hipMalloc((void **)&w.queue, kKdMaxBatches * kKdQueues * kKdQueueStride * sizeof(unsigned)), "hipMalloc(queue)"))
        return nullptr;
    if (!hip_ok(hipMalloc((void **)&w.spill, spill_bytes), "hipMalloc(spill)")) {
        (void)hipFree(w.queue);
        return nullptr;
    }
    return &(s->workspaces[stream] = w);
}

// the scene and workspace part of a launch's parameters; the launchers add the rays and the outputs
static KdParams scene_params(const nnbvh_kd_scene *s, const KdWorkspace *w) {
    KdParams p{};
    p.nodes = s->d_nodes;
    p.primIndices = s->d_indices;
    p.prims = s->d_prims;
    std::memcpy(p.bmin, s->bounds, 12);
    std::memcpy(p.bmax, s->bounds + 3, 12);
    p.queue = w->queue;
    p.nQueues = kKdQueues;
    p.primWeight = 12;  // swept on bathroom: 12 / 8 / 4 is the best of 4 x 2 x 3 (+1.5 % over 24 / 8 / 4)
    p.refillWeight = 8;
    p.nodeRepeat = 4;
    p.hasHostPrims = s->has_host_prims;
    p.spill = w->spill;
    p.extras = s->d_extras;
    p.alphaTex = (const float4 *)s->d_alpha_tex;
    p.alphaTexels = s->d_alpha_texels;
    return p;
}

// The queue heads zeroed, then the instance over total_rays rays in all.  Persistent grid = what is resident at once,
// asked from the runtime for the exact instance (once: s->blocks_per_cu keeps it by the instance's row of kKdInstances)
// and capped at the 8 blocks per CU the spill array is sized for; never more threads than rays to start with.
static int kd_run(nnbvh_kd_scene *s, const KdWorkspace *w, hipStream_t stream, const KdInstance &is, const KdParams &p,
                  int64_t total_rays, int queue_words, const char *what) {
    const int row = kd_instance_index(is);
    if (row < 0) return hip_ok(hipErrorInvalidValue, what) ? NNBVH_OK : NNBVH_ERR_DEVICE;  // the library does not hold it
    int &per_cu = s->blocks_per_cu[row];
    if (per_cu == 0) {
        int occ = 0;
        const hipError_t e = launch_kd_trace(is, p, 0, nullptr, &occ);
        per_cu = (e == hipSuccess && occ > 0) ? std::min(occ, 8) : 4;
    }
    int blocks = s->n_cus * per_cu;
    const int64_t need = (total_rays + kKdBlock - 1) / kKdBlock;
    if (need < blocks) blocks = (int)std::max<int64_t>(need, 1);
    hipError_t e = launch_zero_queue(w->queue, queue_words, stream);  // (bvh_trace.h: a kernel node)
    if (e == hipSuccess) e = launch_kd_trace(is, p, blocks, stream, nullptr);
    return hip_ok(e, what) ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

// one batch of records, mode 0: closest hit (out = nnbvh_hit[n]), mode 1: any hit (out = uint8[n], counts nullable)
static int kd_launch(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, int mode, const void *d_rays, int64_t n,
                     void *d_out, void *d_vis, void *d_tests) {
    KdParams p = scene_params(s, w);
    p.rays = (const nnbvh_ray *)d_rays;
    if (mode == 0) p.hits = (nnbvh_hit *)d_out;
    else p.occluded = (uint8_t *)d_out;
    p.visitedOut = (int32_t *)d_vis;
    p.testsOut = (int32_t *)d_tests;
    p.n = (long)n;
    return kd_run(s, w, stream, pick_kd_instance(kd_scene_traits(s), mode), p, n, kKdQueues * kKdQueueStride,
                  "kd trace kernel launch");
}

int nnbvh::kd_launch_batches(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const KdBatch *batches, int n_batches) {
    KdParams p = scene_params(s, w);
    bool all_soa = true, candidates = false;
    int64_t total = 0, soa_rays = 0;
    for (int b = 0; b < n_batches; ++b) {
        all_soa = all_soa && !batches[b].rays;
        if (!batches[b].rays) soa_rays += batches[b].n;
        total += batches[b].n;
        candidates = candidates || (batches[b].hc && batches[b].hc->capacity > 0);
    }
    // record form (mode 2): the scene's instance or its candidate-mode twin; SOA form (mode 3): lean only
    bool read_soa = false;
    const KdInstance is = pick_kd_batch_instance(kd_scene_traits(s), all_soa, candidates, &read_soa);
    if (!read_soa && soa_rays > 0 &&
        !grow(&w->d_in, &w->in_bytes, (size_t)soa_rays * sizeof(nnbvh_ray), "hipMalloc(wavefront rays)"))
        return NNBVH_ERR_DEVICE;
    char *gathered = (char *)w->d_in;
    p.nBatches = n_batches;
    p.anyMask = 0;
    for (int b = 0; b < n_batches; ++b) {
        const KdBatch &k = batches[b];
        p.anyMask |= k.any ? 1u << b : 0u;
        p.bOut[b] = k.out;
        p.bVisited[b] = k.any ? (int32_t *)k.visited : nullptr;
        p.bTests[b] = k.any ? (int32_t *)k.tests : nullptr;
        p.bN[b] = (long)k.n;
        p.bNDev[b] = k.d_n;
        if (k.hc && k.hc->capacity > 0 && k.n > 0) {
            if (!zero_candidates(s->n_cus, k.hc, k.n, !k.any, stream)) return NNBVH_ERR_DEVICE;
            if (is.hostc) {  // else: the plain instance over the zeroed counts
                p.bHcCap[b] = k.hc->capacity;
                p.bHcCount[b] = k.hc->count;
                p.bHcBefore[b] = k.any ? nullptr : k.hc->before;
                p.bHcPrim[b] = k.hc->prim;
                p.bHcInst[b] = k.hc->instance;
            }
        }
        if (read_soa) {
            if (k.soa) p.bSoa[b] = *k.soa;  // (an empty batch may come without slices)
        } else if (!k.rays && k.n > 0) {
            if (!hip_ok(launch_wf_gather(*k.soa, WavefrontCount{(int)k.n, k.d_n}, gathered, s->n_cus * 8, stream),
                        "gather kernel launch"))
                return NNBVH_ERR_DEVICE;
            p.bRays[b] = (const nnbvh_ray *)gathered;
            gathered += (size_t)k.n * sizeof(nnbvh_ray);
        } else {
            p.bRays[b] = (const nnbvh_ray *)k.rays;
        }
    }
    return kd_run(s, w, stream, is, p, total, n_batches * kKdQueues * kKdQueueStride, "kd batch trace kernel launch");
}

// ---- the walk calls' launchers (capi_wavefront.cpp: nnbvh_kd_wavefront_walk_*) ------------------------------------
bool nnbvh::kd_walk_scratch(KdWorkspace *w, int slot, size_t bytes, void **out) {
    if (!grow(&w->walk[slot], &w->walk_bytes[slot], std::max<size_t>(bytes, 16), "hipMalloc(walk workspace)"))
        return false;
    *out = w->walk[slot];
    return true;
}

int nnbvh::launch_walk(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, const WalkJob &k) {
    KdParams p = scene_params(s, w);
    p.nBatches = 1;
    p.anyMask = 0;
    p.bRays[0] = (const nnbvh_ray *)k.rays;
    p.bN[0] = (long)k.n;
    p.bNDev[0] = k.d_n;
    const ShadingMeshDevice &m = *k.mesh;
    p.wMesh = {m.verts, m.triVerts, m.patchVerts, m.normals, m.uvs, m.tangents, m.faceIndices, m.triFlags, m.nTris,
               m.defaultFlags, nullptr, 0, nullptr, nullptr};  // kd scenes have one level
    p.walk = k.a;
    return kd_run(s, w, stream, pick_kd_walk_instance(kd_scene_traits(s), k.kind, m.patchVerts != nullptr), p, k.n,
                  kKdQueues * kKdQueueStride, "kd walk kernel launch");
}

bool nnbvh::kd_attach_alpha_textures(nnbvh_kd_scene *s, const nnbvh_alpha_texture *textures, int n_textures) {
    if (upload_alpha_textures(s->device, textures, n_textures, &s->d_alpha_tex, &s->d_alpha_texels, &s->n_alpha_texels)) {
        s->n_alpha_tex = n_textures;
        return true;
    }
    const std::string why = nnbvh_last_error();
    nnbvh_kd_scene_destroy(s);
    set_error(why);
    return false;
}

// nnbvh_kd_scene_create_with_attributes (textures == nullptr: kinds 16 .. 19 are refused) and
// nnbvh_kd_scene_create_with_alpha_textures (the caller has checked the table with check_alpha_textures)
static nnbvh_kd_scene *kd_scene_create(const nnbvh_kd_node *nodes, int n_nodes, const int32_t *prim_indices, int n_indices,
                                       const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                       const float bounds_min_max[6], const float *normals, const float *uvs,
                                       const float *prim_alpha, int device, const nnbvh_alpha_texture *textures,
                                       int n_textures);

extern "C" {

nnbvh_kd_scene *nnbvh_kd_scene_create(const nnbvh_kd_node *nodes, int n_nodes, const int32_t *prim_indices,
                                      int n_indices, const nnbvh_prim *prims, int n_prims, const float *verts,
                                      int n_verts, const float bounds_min_max[6], int device) {
    return nnbvh_kd_scene_create_with_attributes(nodes, n_nodes, prim_indices, n_indices, prims, n_prims, verts, n_verts,
                                                 bounds_min_max, nullptr, nullptr, nullptr, device);
}

nnbvh_kd_scene *nnbvh_kd_scene_create_with_attributes(const nnbvh_kd_node *nodes, int n_nodes,
                                                      const int32_t *prim_indices, int n_indices,
                                                      const nnbvh_prim *prims, int n_prims, const float *verts,
                                                      int n_verts, const float bounds_min_max[6], const float *normals,
                                                      const float *uvs, const float *prim_alpha, int device) {
    return kd_scene_create(nodes, n_nodes, prim_indices, n_indices, prims, n_prims, verts, n_verts, bounds_min_max, normals,
                           uvs, prim_alpha, device, nullptr, 0);
}

nnbvh_kd_scene *nnbvh_kd_scene_create_with_alpha_textures(const nnbvh_kd_node *nodes, int n_nodes,
                                                          const int32_t *prim_indices, int n_indices,
                                                          const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const float bounds_min_max[6],
                                                          const float *normals, const float *uvs, const float *prim_alpha,
                                                          int device, const nnbvh_alpha_texture *textures,
                                                          int n_textures) {
    if (!check_alpha_textures("nnbvh_kd_scene_create_with_alpha_textures", prims, n_prims, normals, textures, n_textures))
        return nullptr;
    return kd_scene_create(nodes, n_nodes, prim_indices, n_indices, prims, n_prims, verts, n_verts, bounds_min_max, normals,
                           uvs, prim_alpha, device, textures, n_textures);
}

}  // extern "C"

static nnbvh_kd_scene *kd_scene_create(const nnbvh_kd_node *nodes, int n_nodes, const int32_t *prim_indices, int n_indices,
                                       const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                       const float bounds_min_max[6], const float *normals, const float *uvs,
                                       const float *prim_alpha, int device, const nnbvh_alpha_texture *textures,
                                       int n_textures) {
    if (!nodes || n_nodes <= 0 || n_indices < 0 || (n_indices > 0 && !prim_indices) || !prims || n_prims <= 0 ||
        !verts || n_verts <= 0 || !bounds_min_max) {
        set_error("kd_scene_create: null or empty argument");
        return nullptr;
    }
    const bool alpha_textures = textures && n_textures > 0;  // (else check_alpha_textures has found no kind 16 .. 19)
    for (int k = 0; k < n_prims && !alpha_textures; ++k)
        if (is_alphatex_kind(prims[k].kind)) {
            set_error(std::string("kd_scene_create: ") + kAlphaTexElsewhere);
            return nullptr;
        }
    // ---- validate everything the kernel indexes with ---------------------------------------------
    for (int i = 0; i < n_indices; ++i)
        if (prim_indices[i] < 0 || prim_indices[i] >= n_prims) {
            set_error("kd_scene_create: primitive index out of range in primitiveIndices");
            return nullptr;
        }
    struct Frame {
        int node, end, depth;
    };
    std::vector<Frame> st;
    st.push_back({0, n_nodes, 0});
    int visited = 0, max_depth = 0;
    while (!st.empty()) {
        const Frame f = st.back();
        st.pop_back();
        ++visited;
        if (f.node < 0 || f.node >= f.end) {
            set_error("kd_scene_create: node index outside its subtree range");
            return nullptr;
        }
        max_depth = std::max(max_depth, f.depth);
        const nnbvh_kd_node &nd = nodes[f.node];
        if ((nd.flags & 3u) == 3u) {
            if (f.node + 1 != f.end) {
                set_error("kd_scene_create: leaf does not close its subtree range (not the reference's layout)");
                return nullptr;
            }
            const uint32_t np = nd.flags >> 2;
            const int32_t v = (int32_t)nd.split_or_index;
            if (np == 1 && (v < 0 || v >= n_prims)) {
                set_error("kd_scene_create: leaf primitive index out of range");
                return nullptr;
            }
            if (np > 1 && (v < 0 || (int64_t)v + np > n_indices)) {
                set_error("kd_scene_create: leaf primitive range out of bounds");
                return nullptr;
            }
        } else {
            const int64_t above = nd.flags >> 2;
            if (above <= f.node + 1 || above >= f.end) {
                set_error("kd_scene_create: above-child link outside its subtree range");
                return nullptr;
            }
            float split;
            std::memcpy(&split, &nd.split_or_index, 4);
            if (std::isnan(split)) {
                set_error("kd_scene_create: NaN split position");
                return nullptr;
            }
            st.push_back({(int)above, f.end, f.depth + 1});
            st.push_back({f.node + 1, (int)above, f.depth + 1});
        }
    }
    if (visited != n_nodes) {
        set_error("kd_scene_create: unreachable nodes in the array");
        return nullptr;
    }
    if (max_depth > kMaxStack) {
        set_error("kd_scene_create: tree deeper than the traversal stack (64 entries, aggregates.cpp:982)");
        return nullptr;
    }
    // ---- the primitive list: kinds and vertex indices, and the scene's flags --------------------------
    bool has_host = false, has_patch = false, any_attr = false, any_alpha_tex = false;
    for (int k = 0; k < n_prims; ++k) {
        const nnbvh_prim &pr = prims[k];
        // a kind with attribute slots: the textured triangles ((u, v) pairs, and the normals check_alpha_textures asked
        // for) and the alpha-tested kinds whose arrays the caller gave
        const bool tex = is_alphatex_kind(pr.kind);
        const bool attr = tex || kd_attr_on_device(pr.kind, normals != nullptr, uvs != nullptr, prim_alpha != nullptr);
        if (pr.kind == NNBVH_PRIM_HOST || ((is_smooth_alpha_kind(pr.kind) || is_alpha_patch_kind(pr.kind)) && !attr)) {
            has_host = true;  // (... without the arrays they read: the host's, a record without geometry)
            continue;
        }
        const int nv = (is_triangle_kind(pr.kind) || tex) ? 3
                       : (pr.kind == NNBVH_PRIM_BILINEAR_PATCH || is_alpha_patch_kind(pr.kind)) ? 4 : 0;
        if (!nv) {
            set_error("kd_scene_create: unsupported primitive kind (triangles, alpha-tested triangles, patches, host primitives)");
            return nullptr;
        }
        for (int j = 0; j < nv; ++j)
            if (pr.v[j] < 0 || pr.v[j] >= n_verts) {
                set_error("kd_scene_create: vertex index out of range");
                return nullptr;
            }
        any_attr = any_attr || attr;
        any_alpha_tex = any_alpha_tex || tex;
        // an alpha re-trace chain that does not end voids the ray like a host primitive, and the alpha test hashes the
        // ray direction: such scenes run the PATCH instances
        if (attr || is_flat_alpha_kind(pr.kind)) has_host = has_patch = true;
        if (nv == 4) has_patch = true;
    }
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) {
        set_error("kd_scene_create: no usable HIP device");
        return nullptr;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) return nullptr;
    nnbvh_kd_scene *s = kd_new_scene(device, prop.multiProcessorCount, max_depth, has_host, has_patch, n_nodes, n_indices,
                                     n_prims, bounds_min_max);
    const size_t ni = (size_t)std::max(n_indices, 1);
    bool ok = hip_ok(hipMalloc((void **)&s->d_nodes, (size_t)n_nodes * 8), "hipMalloc(kd nodes)") &&
              hip_ok(hipMalloc((void **)&s->d_indices, ni * 4), "hipMalloc(kd indices)") &&
              hip_ok(hipMemcpy(s->d_nodes, nodes, (size_t)n_nodes * 8, hipMemcpyHostToDevice), "upload kd nodes");
    if (ok && n_indices > 0)
        ok = hip_ok(hipMemcpy(s->d_indices, prim_indices, (size_t)n_indices * 4, hipMemcpyHostToDevice),
                    "upload kd indices");
    // ---- primitive records and attribute slots: baked on the device from the caller's arrays (kd_bake.hip) ----
    if (ok) {
        Uploads up;
        const auto *d_prims = (const nnbvh_prim *)up.put(prims, (size_t)n_prims * sizeof(nnbvh_prim), "kd primitives");
        const auto *d_verts = (const float *)up.put(verts, (size_t)n_verts * 12, "kd vertices");
        const auto *d_normals = (const float *)up.put(normals, (size_t)n_verts * 12, "kd normals");
        const auto *d_uvs = (const float *)up.put(uvs, (size_t)n_verts * 8, "kd uvs");
        const auto *d_alpha = (const float *)up.put(prim_alpha, (size_t)n_prims * 4, "kd primitive alpha");
        std::string err;
        ok = up.ok;
        if (ok && !kd_bake_records(d_prims, n_prims, d_verts, d_normals, d_uvs, d_alpha, any_attr, nullptr,
                                   (void **)&s->d_prims, (void **)&s->d_extras, &err)) {
            set_error(err);
            ok = false;
        }
    }
    if (!ok) {
        const std::string why = nnbvh_last_error();
        nnbvh_kd_scene_destroy(s);
        set_error(why);
        return nullptr;
    }
    s->has_alpha_tex = any_alpha_tex ? 1 : 0;
    if (alpha_textures && !kd_attach_alpha_textures(s, textures, n_textures)) return nullptr;
    return s;
}

extern "C" {

void nnbvh_kd_scene_destroy(nnbvh_kd_scene *s) {
    if (!s) return;
    DeviceGuard guard(s->device);
    for (auto &kv : s->workspaces) {
        KdWorkspace &w = kv.second;
        for (void *ptr : {(void *)w.queue, (void *)w.spill, w.d_in, w.d_out, w.d_aux0, w.d_aux1, w.d_hits})
            if (ptr) (void)hipFree(ptr);
        for (void *ptr : w.walk)
            if (ptr) (void)hipFree(ptr);
    }
    if (s->d_nodes) (void)hipFree(s->d_nodes);
    if (s->d_indices) (void)hipFree(s->d_indices);
    if (s->d_prims) (void)hipFree(s->d_prims);
    if (s->d_extras) (void)hipFree(s->d_extras);
    if (s->d_alpha_tex) (void)hipFree(s->d_alpha_tex);
    if (s->d_alpha_texels) (void)hipFree(s->d_alpha_texels);
    delete s;
}

int nnbvh_kd_scene_set_option(nnbvh_kd_scene *s, const char *key, int value) {
    // (checked before the scene is looked at: a bad value is refused whatever the scene is)
    if (key && std::string(key) == "offsets32" && value != 0 && value != 1) {
        set_error("kd_scene_set_option: offsets32 must be 0 or 1");
        return NNBVH_ERR_ARG;
    }
    if (!s || !key) {
        set_error("kd_scene_set_option: null argument");
        return NNBVH_ERR_ARG;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    const std::string k(key);
    if (k == "read_soa") s->read_soa = value != 0;
    else if (k == "pair_one_launch") s->pair_one_launch = value != 0;
    else if (k == "offsets32") {
        // 0: the O32 = 0 instances although the scene fits; 1: what kd_fits32 says of its sizes.  The resident blocks
        // per CU are dropped with the width (the cache is per instance: this only asks again)
        if (s->offsets32 != value)
            for (int &b : s->blocks_per_cu) b = 0;
        s->offsets32 = value;
    } else {
        set_error("kd_scene_set_option: unknown key " + k);
        return NNBVH_ERR_ARG;
    }
    return NNBVH_OK;
}

int nnbvh_kd_scene_bounds(const nnbvh_kd_scene *s, float out_min_max[6]) {
    if (!s || !out_min_max) {
        set_error("nnbvh_kd_scene_bounds: null argument");
        return NNBVH_ERR_ARG;
    }
    std::memcpy(out_min_max, s->bounds, 24);
    return NNBVH_OK;
}

static size_t kd_array_bytes(const nnbvh_kd_scene *s, int what) {
    switch (what) {
    case 0: return (size_t)s->n_nodes * 8;
    case 1: return (size_t)s->n_indices * 4;
    case 2: return (size_t)s->n_prims * 64;
    case 3: return s->d_extras ? (size_t)s->n_prims * 96 : 0;
    case 4: return (size_t)s->n_alpha_tex * 48;
    default: return (size_t)s->n_alpha_texels * 4;
    }
}

int nnbvh_kd_scene_info(const nnbvh_kd_scene *s, int64_t out[8]) {
    if (!s || !out) {
        set_error("nnbvh_kd_scene_info: null argument");
        return NNBVH_ERR_ARG;
    }
    out[0] = s->n_nodes;
    out[1] = s->n_indices;
    out[2] = s->n_prims;
    out[3] = s->depth;
    // (the index array is never empty on the device: one entry stands in for none)
    out[4] = (int64_t)(kd_array_bytes(s, 0) + std::max<size_t>(kd_array_bytes(s, 1), 4) + kd_array_bytes(s, 2) + kd_array_bytes(s, 3) +
                       kd_array_bytes(s, 4) + kd_array_bytes(s, 5));
    out[5] = s->has_host_prims;
    out[6] = s->has_patches;
    out[7] = s->d_extras ? 1 : 0;
    return NNBVH_OK;
}

int nnbvh_kd_scene_read(const nnbvh_kd_scene *s, int what, void *out, size_t bytes) {
    if (!s || what < 0 || what > 5) {
        set_error("nnbvh_kd_scene_read: null scene or unknown array (0 nodes, 1 primitiveIndices, 2 primitive records, 3 "
                  "attribute slots, 4 alpha-texture table, 5 alpha texel pool)");
        return NNBVH_ERR_ARG;
    }
    const size_t have = kd_array_bytes(s, what);
    if (bytes != have || (have > 0 && !out)) {
        set_error("nnbvh_kd_scene_read: the buffer is not the array's exact size (" + std::to_string(have) + " bytes)");
        return NNBVH_ERR_ARG;
    }
    if (have == 0) return NNBVH_OK;
    const void *src = what == 0 ? (const void *)s->d_nodes : what == 1 ? (const void *)s->d_indices
                    : what == 2 ? (const void *)s->d_prims : what == 3 ? (const void *)s->d_extras
                    : what == 4 ? (const void *)s->d_alpha_tex : (const void *)s->d_alpha_texels;
    ScopedDevice guard(s->device);
    hipError_t e = guard.status;
    if (e == hipSuccess) e = hipMemcpy(out, src, have, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        set_error(std::string("nnbvh_kd_scene_read: ") + hipGetErrorString(e));
        return NNBVH_ERR_DEVICE;
    }
    return NNBVH_OK;
}

}  // extern "C"

// the arguments of a plain single-batch call, device or host buffers
static bool kd_batch_args_ok(const char *fn, const nnbvh_kd_scene *s, int64_t n, const void *rays, const void *out) {
    if (s && n >= 0 && n < 0x7fffffffLL && (n == 0 || (rays && out))) return true;
    set_error(std::string(fn) + ": bad argument");
    return false;
}

// nnbvh_kd_intersect_closest_device (mode 0) and _any_device (mode 1): one batch of records on the caller's stream
static int kd_device_call(const char *fn, nnbvh_kd_scene *s, int mode, const void *d_rays, int64_t n, void *d_out,
                          void *d_vis, void *d_tests, void *stream) {
    if (!kd_batch_args_ok(fn, s, n, d_rays, d_out)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return kd_launch(s, call.w, (hipStream_t)stream, mode, d_rays, n, d_out, d_vis, d_tests);
}

// nnbvh_kd_trace_batches_device and its candidates form (cands nullable; cands[b] belongs to batches[b], capacity 0 =
// a plain batch).  Everything is checked before the scene is looked at.
static int kd_trace_batches(const char *fn, nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches,
                            const nnbvh_host_candidates *cands, bool with_candidates, void *stream) {
    if (!s || !batches || n_batches < 1 || n_batches > kKdMaxBatches || (with_candidates && !cands)) {
        set_error(std::string(fn) + (with_candidates ? ": bad argument (a scene, 1..4 batches and their candidates)"
                                                     : ": bad argument (a scene and 1..4 batches)"));
        return NNBVH_ERR_ARG;
    }
    KdBatch jobs[kKdMaxBatches];
    int64_t total = 0;
    for (int b = 0; b < n_batches; ++b) {
        const nnbvh_batch &k = batches[b];
        if ((k.kind != NNBVH_BATCH_CLOSEST && k.kind != NNBVH_BATCH_ANY) || k.n < 0 || k.n >= (1LL << kKdIndexBits) ||
            (k.n > 0 && (!k.d_rays || !k.d_out))) {
            set_error(std::string(fn) + ": bad batch (kind, 0 <= n < 2^28, rays and output)");
            return NNBVH_ERR_ARG;
        }
        if (cands && cands[b].capacity != 0) {
            const char *why = candidates_fault(&cands[b], k.kind == NNBVH_BATCH_CLOSEST);
            if (!why && k.kind == NNBVH_BATCH_ANY && (k.d_nodes_visited || k.d_prim_tests))
                why = "an any-hit batch has exact counts or candidates, not both";
            if (why) {
                set_error(std::string(fn) + ": batch candidates: " + why);
                return NNBVH_ERR_ARG;
            }
            jobs[b].hc = &cands[b];
        }
        jobs[b].any = k.kind == NNBVH_BATCH_ANY;
        jobs[b].rays = k.d_rays;
        jobs[b].n = k.n;
        jobs[b].out = k.d_out;
        jobs[b].visited = k.d_nodes_visited;
        jobs[b].tests = k.d_prim_tests;
        total += k.n;
    }
    if (total == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return kd_launch_batches(s, call.w, (hipStream_t)stream, jobs, n_batches);
}

// the arguments of a single-batch candidate call (a one-batch launch: fewer than 2^28 rays)
static bool kd_candidate_args_ok(const char *fn, const nnbvh_kd_scene *s, int64_t n, const void *rays, const void *out,
                                 const nnbvh_host_candidates *c, bool closest) {
    const char *why = nullptr;
    if (!s || n < 0 || (n > 0 && (!rays || !out))) why = "bad argument";
    else if ((why = candidates_fault(c, closest)) != nullptr) {}
    else if (n >= (1LL << kKdIndexBits)) why = "a batch of 2^28 rays or more";
    if (why) set_error(std::string(fn) + ": " + why);
    return !why;
}

static int kd_candidates_device(const char *fn, nnbvh_kd_scene *s, bool any, const void *d_rays, int64_t n, void *d_out,
                                const nnbvh_host_candidates *c, void *stream) {
    if (!kd_candidate_args_ok(fn, s, n, d_rays, d_out, c, !any)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    KdBatch batch;
    batch.any = any, batch.rays = d_rays, batch.n = n, batch.out = d_out, batch.hc = c;
    return kd_launch_batches(s, call.w, (hipStream_t)stream, &batch, 1);
}

// host buffers (candidates_host of capi_internal.h stages them): the one launch is a one-batch launch, waited for
static int kd_candidates_host(const char *fn, nnbvh_kd_scene *s, bool any, const nnbvh_ray *rays, int64_t n, void *out,
                              const nnbvh_host_candidates *c) {
    if (!kd_candidate_args_ok(fn, s, n, rays, out, c, !any)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    return candidates_host(s, !any, rays, n, out, c,
                           [&](KdWorkspace *w, void *d_rays, void *d_out, const nnbvh_host_candidates &d) {
                               KdBatch batch;
                               batch.any = any, batch.rays = d_rays, batch.n = n, batch.out = d_out, batch.hc = &d;
                               const int rc = kd_launch_batches(s, w, nullptr, &batch, 1);
                               if (rc != NNBVH_OK) return rc;
                               return hip_ok(hipStreamSynchronize(nullptr), "kd trace") ? NNBVH_OK : NNBVH_ERR_DEVICE;
                           });
}

// one per-ray output array of a plain host-buffer call (host == nullptr: not asked for) and what its errors call it
struct KdHostArray {
    void *host;
    size_t elem;  // bytes per ray
    const char *alloc, *copy;
};

// nnbvh_kd_intersect_closest (mode 0, outs = {hits}) and _any (mode 1, outs = {occluded, nodes_visited?, prim_tests?}):
// everything staged in the null stream's workspace — outs[0] in d_out, the counts side by side in d_aux0 —, one launch,
// copies out (synchronous)
static int kd_host_call(const char *fn, nnbvh_kd_scene *s, int mode, const nnbvh_ray *rays, int64_t n,
                        const KdHostArray *outs, int n_outs) {
    if (!kd_batch_args_ok(fn, s, n, rays, outs[0].host)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, nullptr);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    KdWorkspace *w = call.w;
    if (!grow(&w->d_in, &w->in_bytes, (size_t)n * sizeof(nnbvh_ray), "hipMalloc(rays)") ||
        !grow(&w->d_out, &w->out_bytes, (size_t)n * outs[0].elem, outs[0].alloc) ||
        (n_outs > 1 && !grow(&w->d_aux0, &w->aux_bytes, (size_t)n * 4 * (size_t)(n_outs - 1), outs[1].alloc)))
        return NNBVH_ERR_DEVICE;
    void *dev[3] = {w->d_out, nullptr, nullptr};
    for (int k = 1; k < n_outs; ++k)
        if (outs[k].host) dev[k] = (int32_t *)w->d_aux0 + (k - 1) * n;  // (a count not asked for is not written)
    if (!hip_ok(hipMemcpy(w->d_in, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays"))
        return NNBVH_ERR_DEVICE;
    const int rc = kd_launch(s, w, nullptr, mode, w->d_in, n, dev[0], dev[1], dev[2]);
    if (rc != NNBVH_OK) return rc;
    if (!hip_ok(hipStreamSynchronize(nullptr), "kd trace")) return NNBVH_ERR_DEVICE;
    for (int k = 0; k < n_outs; ++k)
        if (dev[k] && !hip_ok(hipMemcpy(outs[k].host, dev[k], (size_t)n * outs[k].elem, hipMemcpyDeviceToHost), outs[k].copy))
            return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

extern "C" {

int nnbvh_kd_intersect_closest_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                      void *stream) {
    return kd_device_call("kd_intersect_closest_device", s, 0, d_rays, n, d_hits, nullptr, nullptr, stream);
}

int nnbvh_kd_intersect_any_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                  void *d_nodes_visited, void *d_prim_tests, void *stream) {
    return kd_device_call("kd_intersect_any_device", s, 1, d_rays, n, d_occluded, d_nodes_visited, d_prim_tests, stream);
}

int nnbvh_kd_trace_batches_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches, void *stream) {
    return kd_trace_batches("kd_trace_batches_device", s, batches, n_batches, nullptr, false, stream);
}

int nnbvh_kd_trace_batches_candidates_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches,
                                             const nnbvh_host_candidates *cands, void *stream) {
    return kd_trace_batches("kd_trace_batches_candidates_device", s, batches, n_batches, cands, true, stream);
}

int nnbvh_kd_intersect_closest_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                                 const nnbvh_host_candidates *c, void *stream) {
    return kd_candidates_device("kd_intersect_closest_candidates_device", s, false, d_rays, n, d_hits, c, stream);
}

int nnbvh_kd_intersect_any_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                             const nnbvh_host_candidates *c, void *stream) {
    return kd_candidates_device("kd_intersect_any_candidates_device", s, true, d_rays, n, d_occluded, c, stream);
}

int nnbvh_kd_intersect_closest_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits,
                                          const nnbvh_host_candidates *c) {
    return kd_candidates_host("kd_intersect_closest_candidates", s, false, rays, n, hits, c);
}

int nnbvh_kd_intersect_any_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                                      const nnbvh_host_candidates *c) {
    return kd_candidates_host("kd_intersect_any_candidates", s, true, rays, n, occluded, c);
}

int nnbvh_kd_intersect_closest(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits) {
    const KdHostArray outs[1] = {{hits, sizeof(nnbvh_hit), "hipMalloc(hits)", "copy hits"}};
    return kd_host_call("kd_intersect_closest", s, 0, rays, n, outs, 1);
}

int nnbvh_kd_intersect_any(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                           int32_t *nodes_visited, int32_t *prim_tests) {
    const KdHostArray outs[3] = {{occluded, 1, "hipMalloc(occluded)", "copy occluded"},
                                 {nodes_visited, 4, "hipMalloc(counts)", "copy counts"},
                                 {prim_tests, 4, "hipMalloc(counts)", "copy counts"}};
    return kd_host_call("kd_intersect_any", s, 1, rays, n, outs, 3);
}

}  // extern "C"
