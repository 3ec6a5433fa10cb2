// capi_two_level.cpp — nnbvh_scene_create_instanced_gpu_build: a two-level scene (object instances as pbrt builds
// them, scene.cpp:1521-1577) from the caller's primitive lists to traceable without a tree visiting the host.  Every
// object definition's tree (all of them in one forest pass, SAH or HLBVH), then the top-level tree
// over the instances' transformed bounds, come from the device builders' cores (bvh_build_gpu.hip); the trees are put
// into one numbering and baked by bvh_bake.hip.  nnbvh_build_forest_create_gpu[_hlbvh], at the end, is that forest pass alone.  The device
// arrays are byte for byte those of nn_bvh_amd.instancing.assemble_two_level + nnbvh_scene_create_instanced_with_attributes.
// create_instanced_gpu_build is the body of that call and of its twin with an alpha-texture table (bvh_capi.cpp).
// Host code only.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "bvh_build_gpu.h"
#include "capi_internal.h"

using namespace nnbvh;

namespace {

const char *kFn = "scene_create_instanced_gpu_build: ";

bool fault(const std::string &msg) {
    set_error(msg);
    return false;
}

// The per-primitive part of the checks below, for the scene call and the forest call alike: kinds, vertex indices,
// the arrays a kind needs.  A scene's list is [n_top_prims top-level entries, the objects' primitives]; a forest's
// has objects only (n_top_prims = 0, no placements) and builds trees, which read no vertex attributes.
struct PrimListCheck {
    int n_top_prims = 0, n_placements = 0;
    const nnbvh_animated_transform *animated = nullptr;
    const float *prim_bounds = nullptr, *normals = nullptr, *uvs = nullptr, *prim_alpha = nullptr;
    bool scene = true;  // false: a forest of trees: attributes are not asked for, instance entries have no place
    bool alpha_textures = false;  // the scene call with an alpha-texture table: check_alpha_textures has seen kinds 16 .. 19
    const char *fn = "";  // (forests) the call's name in front of its own message
};
bool check_prims(const nnbvh_prim *prims, int n_prims, int n_verts, const PrimListCheck &c) {
    for (int i = 0; i < n_prims; ++i) {
        const nnbvh_prim &p = prims[i];
        int nv = 0;
        if (p.kind == NNBVH_PRIM_INSTANCE) {
            if (!c.scene) return fault(std::string(c.fn) + "instance entries are not built in a forest");
            if (i >= c.n_top_prims) return fault("scene_create: nested instances are not supported");
            if (p.v[0] < 0 || p.v[0] >= c.n_placements) return fault("scene_create: instance index out of range");
            if (c.animated && c.animated[p.v[0]].actually_animated && !c.prim_bounds)
                return fault("nnbvh_build_create: instance / host primitives need prim_bounds");
        } else if (p.kind == NNBVH_PRIM_HOST) {
            if (!c.prim_bounds) return fault("nnbvh_build_create: instance / host primitives need prim_bounds");
        } else if (is_smooth_alpha_kind(p.kind)) {
            nv = 3;
            if (c.scene && !c.normals)
                return fault("scene_create: NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH primitives need the vertex normals "
                             "(nnbvh_scene_create_with_normals)");
        } else if (is_alpha_patch_kind(p.kind)) {
            nv = 4;
            if (c.scene && (!c.prim_alpha || (is_smooth_alpha_patch_kind(p.kind) && !c.normals) ||
                            (is_uv_alpha_patch_kind(p.kind) && !c.uvs)))
                return fault("scene_create: NNBVH_PRIM_ALPHA_PATCH primitives need the per-primitive alpha array, the "
                             "smooth ones the vertex normals, the _UV ones the vertex uvs too "
                             "(nnbvh_scene_create_with_attributes)");
        } else if (is_triangle_kind(p.kind)) nv = 3;
        else if (p.kind == NNBVH_PRIM_BILINEAR_PATCH) nv = 4;
        else if (is_alphatex_kind(p.kind)) {  // a triangle for a tree; a scene needs the call with an alpha-texture table
            if (c.scene && !c.alpha_textures) return fault(std::string("scene_create: ") + kAlphaTexElsewhere);
            nv = 3;
        } else return fault("scene_create: unknown primitive kind");
        for (int j = 0; j < nv; ++j)
            if (p.v[j] < 0 || p.v[j] >= n_verts) return fault("nnbvh_build_create: vertex index out of range");
    }
    return true;
}

// Everything a kernel indexes with, checked on the host arrays before a device is looked at.
bool check_arguments(const nnbvh_prim *prims, int n_prims, int n_top_prims, const int32_t *object_first, int n_objects,
                     const float *verts, int n_verts, const float *normals, const float *uvs, const float *prim_alpha,
                     const float *prim_bounds, const nnbvh_placement *placements, int n_placements,
                     const nnbvh_animated_transform *animated, int split_method, bool alpha_textures) {
    if (!prims || !verts || !object_first || !placements || n_prims <= 0 || n_verts <= 0 || n_top_prims <= 0 ||
        n_objects <= 0 || n_placements <= 0)
        return fault(std::string(kFn) + "null or empty input array");
    if (object_first[0] != n_top_prims || object_first[n_objects] != n_prims)
        return fault(std::string(kFn) + "malformed object_first (it starts at n_top_prims and ends at n_prims)");
    for (int k = 0; k < n_objects; ++k)
        if (object_first[k + 1] <= object_first[k])
            return fault(std::string(kFn) + "malformed object_first (an object is empty or the entries decrease)");
    if (split_method != NNBVH_SPLIT_SAH && split_method != NNBVH_SPLIT_HLBVH)
        return fault(std::string(kFn) + "only the sah and hlbvh split methods are built on the device");
    for (int j = 0; j < n_placements; ++j) {
        if (placements[j].object < 0 || placements[j].object >= n_objects)
            return fault(std::string(kFn) + "placement object out of range");
        if (animated && animated[j].actually_animated && !(animated[j].end_time > animated[j].start_time))
            return fault("scene_create: animated instance with an empty time range");
    }
    PrimListCheck c;
    c.n_top_prims = n_top_prims;
    c.n_placements = n_placements;
    c.animated = animated;
    c.prim_bounds = prim_bounds;
    c.normals = normals;
    c.uvs = uvs;
    c.prim_alpha = prim_alpha;
    c.alpha_textures = alpha_textures;
    return check_prims(prims, n_prims, n_verts, c);
}

// The forest call's: the same faults in the same words where the two calls share them.
bool check_forest_arguments(const nnbvh_prim *prims, int n_prims, const int32_t *object_first, int n_objects,
                            const float *verts, int n_verts, const float *prim_bounds, int split_method, bool hlbvh) {
    const char *fn = hlbvh ? "nnbvh_build_forest_create_gpu_hlbvh: " : "nnbvh_build_forest_create_gpu: ";
    if (!prims || !verts || !object_first || n_prims <= 0 || n_verts <= 0 || n_objects <= 0)
        return fault(std::string(fn) + "null or empty input array");
    if (object_first[0] != 0 || object_first[n_objects] != n_prims)
        return fault(std::string(fn) + "malformed object_first (it starts at 0 and ends at n_prims)");
    for (int k = 0; k < n_objects; ++k)
        if (object_first[k + 1] <= object_first[k])
            return fault(std::string(fn) + "malformed object_first (an object is empty or the entries decrease)");
    if (!hlbvh && split_method != NNBVH_SPLIT_SAH)
        return fault(std::string(fn) + "the forest build is SAH only (split_method NNBVH_SPLIT_SAH; HLBVH forests: "
                                       "nnbvh_build_forest_create_gpu_hlbvh)");
    PrimListCheck c;
    c.prim_bounds = prim_bounds;
    c.scene = false;
    c.fn = fn;
    return check_prims(prims, n_prims, n_verts, c);
}

// the call's device memory and stream: freed on every way out
struct Held {
    std::vector<void *> ptrs;
    hipStream_t stream = nullptr;
    ScratchPool pool;
    template <typename T>
    T *get(size_t count, const char *what) {
        void *p = nullptr;
        if (!hip_ok(hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)), what)) return nullptr;
        ptrs.push_back(p);
        return (T *)p;
    }
    void drop(const void *p) {
        for (void *&q : ptrs)
            if (q && q == p) {
                (void)hipFree(q);
                q = nullptr;
            }
    }
    ~Held() {
        pool.clear();
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

template <typename T>
bool put(T *dst, const T *src, size_t count, hipStream_t stream, const char *what) {
    return hip_ok(hipMemcpyAsync(dst, src, count * sizeof(T), hipMemcpyHostToDevice, stream), what);
}

}  // namespace

extern "C" nnbvh_scene *nnbvh_scene_create_instanced_gpu_build(
    const nnbvh_prim *prims, int n_prims, int n_top_prims, const int32_t *object_first, int n_objects,
    const float *verts, int n_verts, const float *normals, const float *uvs, const float *prim_alpha,
    const float *prim_bounds, const nnbvh_placement *placements, int n_placements,
    const nnbvh_animated_transform *animated, int max_prims_in_node, int split_method, int device) {
    return create_instanced_gpu_build(prims, n_prims, n_top_prims, object_first, n_objects, verts, n_verts, normals, uvs,
                                      prim_alpha, prim_bounds, placements, n_placements, animated, max_prims_in_node,
                                      split_method, device, false);
}

// (nnbvh_scene_create_instanced_gpu_build_with_alpha_textures is beside the other calls with a table, bvh_capi.cpp)
nnbvh_scene *nnbvh::create_instanced_gpu_build(
    const nnbvh_prim *prims_in, int n_prims, int n_top_prims, const int32_t *object_first, int n_objects,
    const float *verts, int n_verts, const float *normals, const float *uvs, const float *prim_alpha,
    const float *prim_bounds, const nnbvh_placement *placements, int n_placements,
    const nnbvh_animated_transform *animated, int max_prims_in_node, int split_method, int device,
    bool alpha_textures) {
    if (!check_arguments(prims_in, n_prims, n_top_prims, object_first, n_objects, verts, n_verts, normals, uvs,
                         prim_alpha, prim_bounds, placements, n_placements, animated, split_method, alpha_textures))
        return nullptr;
    const int n_dev = nnbvh_device_count();
    if (n_dev <= 0 || device < 0 || device >= n_dev) {
        set_error(std::string(kFn) + "no usable HIP device (this library has no CPU fallback)");
        return nullptr;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    const auto t_start = std::chrono::steady_clock::now();

    // with a per-primitive array to carry along, the builds run with ids = positions in the caller's array; the
    // gather pass puts the caller's ids back (bvh_bake.hip), as nnbvh_scene_create_gpu_build_with_attributes does
    const nnbvh_prim *prims = prims_in;
    std::vector<nnbvh_prim> tagged;
    std::vector<int32_t> caller_ids;
    if (prim_alpha) {
        tagged.assign(prims_in, prims_in + n_prims);
        caller_ids.resize((size_t)n_prims);
        for (int i = 0; i < n_prims; ++i) {
            caller_ids[(size_t)i] = tagged[(size_t)i].id;
            tagged[(size_t)i].id = i;
        }
        prims = tagged.data();
    }
    std::vector<unsigned char> anim_flag;
    if (animated) {
        anim_flag.resize((size_t)n_placements);
        for (int j = 0; j < n_placements; ++j) anim_flag[(size_t)j] = animated[j].actually_animated ? 1 : 0;
    }

    std::vector<unsigned char> named((size_t)n_objects, 0);
    for (int j = 0; j < n_placements; ++j) named[(size_t)placements[j].object] = 1;

    Held h;
    if (!hip_ok(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking), "hipStreamCreate")) return nullptr;
    hipStream_t stream = h.stream;
    const int n_obj_prims = n_prims - n_top_prims;
    const size_t child_cap = 2 * (size_t)n_obj_prims - (size_t)n_objects;  // sum of 2 n - 1
    const size_t top_cap = 2 * (size_t)n_top_prims - 1;
    // the vertices, the primitives and the caller's bounds go up once; every build reads its part of them
    nnbvh_prim *d_prims = h.get<nnbvh_prim>((size_t)n_prims, "hipMalloc(primitives)");
    float *d_verts = h.get<float>(3 * (size_t)n_verts, "hipMalloc(vertices)");
    float *d_bounds = h.get<float>(6 * (size_t)(prim_bounds ? n_prims : n_top_prims), "hipMalloc(bounds)");
    nnbvh_placement *d_placements = h.get<nnbvh_placement>((size_t)n_placements, "hipMalloc(placements)");
    unsigned char *d_anim_flag = animated ? h.get<unsigned char>((size_t)n_placements, "hipMalloc(placements)") : nullptr;
    int *d_object_first = h.get<int>((size_t)n_objects, "hipMalloc(objects)");
    int *d_child_base = h.get<int>((size_t)n_objects, "hipMalloc(objects)");
    int *d_object_root = h.get<int>((size_t)n_objects, "hipMalloc(objects)");
    unsigned char *d_named = h.get<unsigned char>((size_t)n_objects, "hipMalloc(objects)");
    nnbvh_prim *d_ordered = h.get<nnbvh_prim>((size_t)n_prims, "hipMalloc(ordered primitives)");
    nnbvh_linear_node *d_child_nodes = h.get<nnbvh_linear_node>(child_cap, "hipMalloc(child trees)");
    if (!d_prims || !d_verts || !d_bounds || !d_placements || (animated && !d_anim_flag) || !d_object_first ||
        !d_child_base || !d_object_root || !d_named || !d_ordered || !d_child_nodes)
        return nullptr;
    bool ok = put(d_prims, prims, (size_t)n_prims, stream, "hipMemcpy(primitives)") &&
              put(d_verts, verts, 3 * (size_t)n_verts, stream, "hipMemcpy(vertices)") &&
              put(d_placements, placements, (size_t)n_placements, stream, "hipMemcpy(placements)") &&
              put(d_object_first, (const int *)object_first, (size_t)n_objects, stream, "hipMemcpy(objects)") &&
              put(d_named, named.data(), (size_t)n_objects, stream, "hipMemcpy(objects)");
    if (ok && prim_bounds) ok = put(d_bounds, prim_bounds, 6 * (size_t)n_prims, stream, "hipMemcpy(bounds)");
    if (ok && !prim_bounds) ok = hip_ok(hipMemsetAsync(d_bounds, 0, 24 * (size_t)n_top_prims, stream), "hipMemset(bounds)");
    if (ok && animated) ok = put(d_anim_flag, anim_flag.data(), (size_t)n_placements, stream, "hipMemcpy(placements)");
    if (!ok || !hip_ok(hipStreamSynchronize(stream), "upload")) return nullptr;

    // the children first: tree k into d_child_nodes at child_base[k], its leaf order into the scene's primitive array
    // at the object's own place (the scene's order is [top, object 0, object 1, ...], as the caller's list is)
    std::string err;
    std::vector<int> child_base((size_t)n_objects);
    int child_total = 0, child_depth = 0;
    auto build = [&](DeviceBuildInput &in, GpuBuildResult *r) {
        in.d_verts = d_verts;
        in.n_verts = n_verts;
        in.max_prims_in_node = max_prims_in_node;
        in.stream = stream;
        in.pool = &h.pool;
        const bool built = split_method == NNBVH_SPLIT_SAH ? gpu_sah_device(in, r, &err) : gpu_hlbvh_device(in, r, &err);
        if (!built) set_error(err);
        return built;
    };
    // All objects in one forest pass, SAH or HLBVH.  NNBVH_TWO_LEVEL_LOOP=1 keeps the object-by-object loop reachable
    // for both (speed only, like NNBVH_SAH_SMALL: the same bytes either way)
    const char *loop_env = std::getenv("NNBVH_TWO_LEVEL_LOOP");
    const bool forest = !(loop_env && std::atoi(loop_env) != 0);
    if (forest) {
        std::vector<int> local_first((size_t)n_objects + 1);
        for (int k = 0; k <= n_objects; ++k) local_first[(size_t)k] = object_first[k] - n_top_prims;
        DeviceBuildInput in;
        in.d_prims = d_prims + n_top_prims;
        in.n_prims = n_obj_prims;
        in.d_prim_bounds = prim_bounds ? d_bounds + 6 * (size_t)n_top_prims : nullptr;
        in.d_nodes_out = d_child_nodes;
        in.d_ordered_out = d_ordered + n_top_prims;
        in.d_verts = d_verts;
        in.n_verts = n_verts;
        in.max_prims_in_node = max_prims_in_node;
        in.stream = stream;
        in.pool = &h.pool;
        ForestBuildResult f;
        if (!(split_method == NNBVH_SPLIT_SAH ? gpu_sah_forest_device : gpu_hlbvh_forest_device)(in, local_first.data(), n_objects, &f, &err)) {
            set_error(err);
            return nullptr;
        }
        child_total = f.total_nodes;
        for (int k = 0; k < n_objects; ++k) {
            child_base[(size_t)k] = f.node_first[(size_t)k];
            if (named[(size_t)k]) child_depth = std::max(child_depth, f.depth[(size_t)k] + 1);
        }
    }
    for (int k = 0; k < n_objects && !forest; ++k) {
        const int first = object_first[k], count = object_first[k + 1] - first;
        DeviceBuildInput in;
        in.d_prims = d_prims + first;
        in.n_prims = count;
        in.d_prim_bounds = prim_bounds ? d_bounds + 6 * (size_t)first : nullptr;
        in.d_nodes_out = d_child_nodes + child_total;
        in.d_ordered_out = d_ordered + first;
        GpuBuildResult r;
        if (!build(in, &r)) return nullptr;
        child_base[(size_t)k] = child_total;
        child_total += r.total_nodes;
        // (only the trees a placement names are ever walked: an object nobody places adds nothing to the depth)
        if (named[(size_t)k]) child_depth = std::max(child_depth, r.depth + 1);
    }
    // the top tree over the instances' bounds, straight into the front of the scene's node array
    nnbvh_linear_node *d_nodes = h.get<nnbvh_linear_node>(top_cap + (size_t)child_total, "hipMalloc(tree)");
    unsigned char *d_node_unnamed = h.get<unsigned char>(top_cap + (size_t)child_total, "hipMalloc(tree)");
    if (!d_nodes || !d_node_unnamed) return nullptr;
    if (!put(d_child_base, child_base.data(), (size_t)n_objects, stream, "hipMemcpy(objects)")) return nullptr;
    if (!instance_bounds_on_device(d_prims, n_top_prims, d_placements, d_anim_flag, d_child_nodes, d_child_base, d_bounds,
                                   stream, &err)) {
        set_error(err);
        return nullptr;
    }
    GpuBuildResult top;
    {
        DeviceBuildInput in;
        in.d_prims = d_prims;
        in.n_prims = n_top_prims;
        in.d_prim_bounds = d_bounds;
        in.d_nodes_out = d_nodes;
        in.d_ordered_out = d_ordered;
        if (!build(in, &top)) return nullptr;
    }
    const int depth = top.depth + child_depth;  // pending entries of the outer walk + those of the child walk
    if (depth > kMaxStack) {
        set_error("scene_create: tree deeper than the 64-entry traversal stack");
        return nullptr;
    }
    const int n_nodes = top.total_nodes + child_total;
    if (!rebase_children_on_device(d_child_nodes, child_total, d_child_base, d_object_first, n_objects, top.total_nodes,
                                   d_nodes, d_object_root, d_named, d_node_unnamed, stream, &err)) {
        set_error(err);
        return nullptr;
    }
    if (!hip_ok(hipStreamSynchronize(stream), "two-level build")) return nullptr;
    // all builder scratch goes before the bake allocates
    h.pool.clear();
    h.drop(d_prims);
    h.drop(d_bounds);
    h.drop(d_child_nodes);
    h.drop(d_child_base);
    h.drop(d_object_first);
    h.drop(d_named);

    float *d_alpha = nullptr, *d_normals = nullptr, *d_uvs = nullptr;
    if (prim_alpha) {
        // the gather works on the DEFAULT stream with blocking copies and ends with hipDeviceSynchronize: it sees the
        // builds' output only because the private stream was synchronised above, and the bake below (private stream
        // again) sees its output only because of that device-wide wait.  Keep both
        void *p = nullptr;
        if (!gather_prim_alpha_on_device(d_ordered, n_prims, prim_alpha, caller_ids.data(), &p, &err)) {
            set_error(err);
            return nullptr;
        }
        h.ptrs.push_back(p);
        d_alpha = (float *)p;
    }
    if (normals) {
        d_normals = h.get<float>(3 * (size_t)n_verts, "hipMalloc(normals)");
        if (!d_normals || !put(d_normals, normals, 3 * (size_t)n_verts, stream, "hipMemcpy(normals)")) return nullptr;
    }
    if (uvs) {
        d_uvs = h.get<float>(2 * (size_t)n_verts, "hipMalloc(uvs)");
        if (!d_uvs || !put(d_uvs, uvs, 2 * (size_t)n_verts, stream, "hipMemcpy(uvs)")) return nullptr;
    }
    InstanceBake inst;
    inst.d_placements = d_placements;
    inst.d_object_root = d_object_root;
    inst.d_animated = d_anim_flag;
    inst.d_node_unnamed = d_node_unnamed;
    BakedScene b;
    if (!bake_on_device(d_nodes, n_nodes, d_ordered, n_prims, d_verts, device, &b, &err, d_normals, d_alpha, d_uvs, &inst,
                        stream)) {
        set_error(err);
        return nullptr;
    }

    nnbvh_scene *s = scene_from_baked(b, depth, device, true);
    if (!s || (animated && !upload_anim_table(s, animated, n_placements))) return nullptr;
    s->build_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return s;
}

// ---- nnbvh_build_forest_create_gpu: the object trees alone, downloaded ------------------------------------------------
// (here and not beside nnbvh_build_create_gpu: bvh_build.cpp is also built on its own, without the device code, and
// this call shares its argument checks with the scene call above)
struct nnbvh_forest {
    std::vector<nnbvh_linear_node> nodes;
    std::vector<nnbvh_prim> ordered;
    std::vector<int32_t> node_first, depths;
    double ms[5] = {0, 0, 0, 0, 0};
    int n_levels = 0, n_subtrees = 0, n_upper = 0, n_upper_passes = 0;
};

namespace {

nnbvh_forest *forest_create(const nnbvh_prim *prims, int n_prims, const int32_t *object_first, int n_objects,
                            const float *verts, int n_verts, const float *prim_bounds, int max_prims_in_node,
                            int split_method, int device, bool hlbvh) {
    if (!check_forest_arguments(prims, n_prims, object_first, n_objects, verts, n_verts, prim_bounds, split_method, hlbvh))
        return nullptr;
    const int n_dev = nnbvh_device_count();
    if (n_dev <= 0 || device < 0 || device >= n_dev) {
        set_error(std::string(hlbvh ? "nnbvh_build_forest_create_gpu_hlbvh" : "nnbvh_build_forest_create_gpu") +
                  ": no usable HIP device (this library has no CPU fallback)");
        return nullptr;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    auto since = [](std::chrono::steady_clock::time_point t) {
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    };
    Held h;
    if (!hip_ok(hipStreamCreateWithFlags(&h.stream, hipStreamNonBlocking), "hipStreamCreate")) return nullptr;
    auto t0 = std::chrono::steady_clock::now();
    nnbvh_prim *d_prims = h.get<nnbvh_prim>((size_t)n_prims, "hipMalloc(primitives)");
    float *d_verts = h.get<float>(3 * (size_t)n_verts, "hipMalloc(vertices)");
    float *d_bounds = prim_bounds ? h.get<float>(6 * (size_t)n_prims, "hipMalloc(bounds)") : nullptr;
    if (!d_prims || !d_verts || (prim_bounds && !d_bounds)) return nullptr;
    bool ok = put(d_prims, prims, (size_t)n_prims, h.stream, "hipMemcpy(primitives)") &&
              put(d_verts, verts, 3 * (size_t)n_verts, h.stream, "hipMemcpy(vertices)");
    if (ok && prim_bounds) ok = put(d_bounds, prim_bounds, 6 * (size_t)n_prims, h.stream, "hipMemcpy(bounds)");
    if (!ok || !hip_ok(hipStreamSynchronize(h.stream), "upload")) return nullptr;
    auto out = std::make_unique<nnbvh_forest>();
    out->ms[0] = since(t0);

    DeviceBuildInput in;
    in.d_prims = d_prims;
    in.n_prims = n_prims;
    in.d_verts = d_verts;
    in.n_verts = n_verts;
    in.d_prim_bounds = d_bounds;
    in.max_prims_in_node = max_prims_in_node;
    in.stream = h.stream;
    in.pool = &h.pool;
    ForestBuildResult f;
    std::string err;
    if (!(hlbvh ? gpu_hlbvh_forest_device : gpu_sah_forest_device)(in, (const int *)object_first, n_objects, &f, &err)) {
        set_error(err);
        return nullptr;
    }
    h.ptrs.push_back(f.d_nodes);
    h.ptrs.push_back(f.d_ordered);
    t0 = std::chrono::steady_clock::now();
    out->nodes.resize((size_t)f.total_nodes);
    out->ordered.resize((size_t)n_prims);
    if (!hip_ok(hipMemcpyAsync(out->nodes.data(), f.d_nodes, out->nodes.size() * sizeof(nnbvh_linear_node),
                               hipMemcpyDeviceToHost, h.stream), "hipMemcpy(nodes)") ||
        !hip_ok(hipMemcpyAsync(out->ordered.data(), f.d_ordered, out->ordered.size() * sizeof(nnbvh_prim),
                               hipMemcpyDeviceToHost, h.stream), "hipMemcpy(ordered primitives)") ||
        !hip_ok(hipStreamSynchronize(h.stream), "download"))
        return nullptr;
    out->ms[4] = since(t0);
    for (int k = 1; k <= 3; ++k) out->ms[k] = f.ms[k];
    out->node_first.assign(f.node_first.begin(), f.node_first.end());
    out->depths.assign(f.depth.begin(), f.depth.end());
    out->n_levels = f.n_levels;
    out->n_subtrees = f.n_subtrees;
    out->n_upper = f.n_upper;
    out->n_upper_passes = f.n_upper_passes;
    return out.release();
}

}  // namespace

extern "C" nnbvh_forest *nnbvh_build_forest_create_gpu(const nnbvh_prim *prims, int n_prims, const int32_t *object_first,
                                                       int n_objects, const float *verts, int n_verts,
                                                       const float *prim_bounds, int max_prims_in_node, int split_method,
                                                       int device) {
    return forest_create(prims, n_prims, object_first, n_objects, verts, n_verts, prim_bounds, max_prims_in_node,
                         split_method, device, false);
}

extern "C" nnbvh_forest *nnbvh_build_forest_create_gpu_hlbvh(const nnbvh_prim *prims, int n_prims,
                                                             const int32_t *object_first, int n_objects,
                                                             const float *verts, int n_verts, const float *prim_bounds,
                                                             int max_prims_in_node, int device) {
    return forest_create(prims, n_prims, object_first, n_objects, verts, n_verts, prim_bounds, max_prims_in_node,
                         NNBVH_SPLIT_HLBVH, device, true);
}

extern "C" const nnbvh_linear_node *nnbvh_forest_nodes(const nnbvh_forest *f, int *n_nodes) {
    if (!f) return nullptr;
    if (n_nodes) *n_nodes = (int)f->nodes.size();
    return f->nodes.data();
}
extern "C" const int32_t *nnbvh_forest_node_first(const nnbvh_forest *f, int *n_objects) {
    if (!f) return nullptr;
    if (n_objects) *n_objects = (int)f->depths.size();
    return f->node_first.data();
}
extern "C" const int32_t *nnbvh_forest_depths(const nnbvh_forest *f, int *n_objects) {
    if (!f) return nullptr;
    if (n_objects) *n_objects = (int)f->depths.size();
    return f->depths.data();
}
extern "C" const nnbvh_prim *nnbvh_forest_ordered_prims(const nnbvh_forest *f, int *n_prims) {
    if (!f) return nullptr;
    if (n_prims) *n_prims = (int)f->ordered.size();
    return f->ordered.data();
}
extern "C" int nnbvh_forest_gpu_timing(const nnbvh_forest *f, double out_ms[5]) {
    if (!f || !out_ms) return NNBVH_ERR_ARG;
    std::memcpy(out_ms, f->ms, sizeof f->ms);
    return NNBVH_OK;
}
extern "C" int nnbvh_forest_n_levels(const nnbvh_forest *f) { return f ? f->n_levels : -1; }
extern "C" int nnbvh_forest_n_subtrees(const nnbvh_forest *f) { return f ? f->n_subtrees : -1; }
extern "C" int nnbvh_forest_n_upper(const nnbvh_forest *f) { return f ? f->n_upper : -1; }
extern "C" int nnbvh_forest_n_upper_passes(const nnbvh_forest *f) { return f ? f->n_upper_passes : -1; }
extern "C" void nnbvh_forest_destroy(nnbvh_forest *f) { delete f; }
