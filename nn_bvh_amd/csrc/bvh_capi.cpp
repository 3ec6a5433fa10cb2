// bvh_capi.cpp — the C ABI of include/nnbvh.h, scene part: validation of the caller's trees and primitives, their
// upload to the device baker (bvh_bake.hip: the one writer of the device layout, for flat and two-level scenes, host-
// and device-built trees alike), the scene object around what it made, scene queries and options, workspaces.  The
// calls that launch kernels are in capi_trace.cpp
// (ray batches), capi_wavefront.cpp (queues) and capi_shading.cpp (shading meshes).  Host code only
// (compiled with hipcc for the HIP runtime API).  There is deliberately no CPU traversal in this
// library: if no HIP device is usable the intersect entry points fail with NNBVH_ERR_DEVICE.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "alpha_texture_math.h"
#include "bvh_build_gpu.h"
#include "capi_internal.h"
#include "top_extend.h"
#include "top_table.h"

namespace nnbvh {

static thread_local std::string g_error;
void set_error(const std::string &msg) { g_error = msg; }

}  // namespace nnbvh

using namespace nnbvh;

// -------------------------------------------------------------------------------------
// Tree validation: everything the kernels index with is range-checked here once, so a
// malformed tree is an NNBVH_ERR_ARG at create time, never a device fault.
// Validates the DFS-laid-out tree occupying nodes[root, root + n_tree).  `covered`
// is shared by all trees of a scene (top level + instanced children).
static bool validate_tree(const nnbvh_linear_node *nodes, int root, int n_tree, const nnbvh_prim *prims,
                          int n_prims, bool allow_instances, std::vector<uint8_t> &covered, int *depth_out) {
    if (n_tree < 1) {
        set_error("scene_create: tree has no nodes");
        return false;
    }
    const int n_nodes = root + n_tree;
    // iterative DFS; each frame = (node, end bound of its subtree range, depth)
    struct Frame {
        int node, end, depth;
    };
    std::vector<Frame> st;
    st.push_back({root, n_nodes, 0});
    int visited = 0, max_depth = 0;
    while (!st.empty()) {
        Frame f = st.back();
        st.pop_back();
        ++visited;
        if (f.node < 0 || f.node >= f.end) {
            set_error("scene_create: node index outside its subtree range");
            return false;
        }
        max_depth = std::max(max_depth, f.depth);
        const nnbvh_linear_node &nd = nodes[f.node];
        // Bounds3f with min <= max on every axis (and no NaN): what every builder emits, and what the
        // interior step's form of the slab test (trace_math.h slab_entry_key) is equal to the
        // reference's for
        for (int k = 0; k < 3; ++k)
            if (!(nd.pmin[k] <= nd.pmax[k])) {
                set_error("scene_create: node bounds with min > max (or NaN)");
                return false;
            }
        if (nd.nprims > 0) {
            if (f.node + 1 != f.end) {
                set_error("scene_create: leaf does not close its subtree range (not a DFS layout)");
                return false;
            }
            if (nd.offset < 0 || (int64_t)nd.offset + nd.nprims > n_prims) {
                set_error("scene_create: leaf primitive range out of bounds");
                return false;
            }
            for (int i = 0; i < nd.nprims; ++i) {
                if (covered[(size_t)nd.offset + i]) {
                    set_error("scene_create: primitive referenced by two leaves");
                    return false;
                }
                covered[(size_t)nd.offset + i] = 1;
                if (!allow_instances && prims[(size_t)nd.offset + i].kind == NNBVH_PRIM_INSTANCE) {
                    set_error("scene_create: nested instances are not supported");
                    return false;
                }
            }
        } else {
            if (nd.axis > 2) {
                set_error("scene_create: interior node axis > 2");
                return false;
            }
            const int c0 = f.node + 1, c1 = nd.offset;
            if (c1 <= c0 || c1 >= f.end) {
                set_error("scene_create: secondChildOffset outside the node's subtree range");
                return false;
            }
            st.push_back({c1, f.end, f.depth + 1});
            st.push_back({c0, c1, f.depth + 1});
        }
    }
    if (visited != n_tree) {
        set_error("scene_create: unreachable nodes in the array");
        return false;
    }
    *depth_out = max_depth;
    return true;
}

// AngleBetween(Quaternion, Quaternion) (util/vecmath.h:1138-1143) and SinXOverX (util/math.h:340-344) with
// the host's libm, as the reference's Slerp evaluates them; they depend on the transform only
static float quat_dot_host(const float a[4], const float b[4]) {
    return (a[0] * b[0] + a[1] * b[1] + a[2] * b[2]) + a[3] * b[3];
}
static float quat_angle_between_host(const float q1[4], const float q2[4]) {
    float t[4];
    const bool neg = quat_dot_host(q1, q2) < 0;
    for (int k = 0; k < 4; ++k) t[k] = neg ? q1[k] + q2[k] : q2[k] - q1[k];
    float x = std::sqrt(quat_dot_host(t, t)) / 2;
    x = x < -1 ? -1 : (x > 1 ? 1 : x);
    return neg ? 3.14159265358979323846f - 2 * std::asin(x) : 2 * std::asin(x);
}

static float sin_x_over_x_host(float x) {
    if (1 - x * x == 1) return 1;
    return std::sin(x) / x;
}

// one entry of the device's animation table (layout: anim_math.h)
void nnbvh::fill_anim_entry(const nnbvh_animated_transform &a, float *t) {
    std::memcpy(t, a.T, 24);
    std::memcpy(t + 6, a.R, 32);
    std::memcpy(t + 14, a.S, 128);
    t[46] = a.start_time;
    t[47] = a.end_time;
    t[48] = quat_angle_between_host(a.R[0], a.R[1]);
    t[49] = sin_x_over_x_host(t[48]);
    std::memcpy(t + 50, a.start_inv, 48);
    std::memcpy(t + 62, a.end_inv, 48);
    t[74] = a.actually_animated ? 1.0f : 0.0f;
}

// ---- image-textured alpha (kinds 16 .. 19) ---------------------------------------------------------------------
// Everything the kernel indexes a texture with, checked on the host before a device is looked at; `fn` names the call.
bool nnbvh::check_alpha_textures(const char *fn, const nnbvh_prim *prims, int n_prims, const float *normals,
                                 const nnbvh_alpha_texture *textures, int n_textures, bool with_patches) {
    auto fault = [&](const std::string &what) {
        set_error(std::string(fn) + ": " + what);
        return false;
    };
    if (n_textures < 0 || (n_textures > 0 && !textures)) return fault("null alpha-texture table");
    static_assert(NNBVH_WRAP_REPEAT == kWrapRepeat && NNBVH_WRAP_CLAMP == kWrapClamp && NNBVH_WRAP_BLACK == kWrapBlack,
                  "alpha_texture_math.h restates the wrap modes");
    for (int k = 0; k < n_textures; ++k) {
        const nnbvh_alpha_texture &t = textures[k];
        const std::string which = "alpha texture " + std::to_string(k);
        if (!t.texels) return fault(which + " has null texels");
        if (t.width < 1 || t.width > kMaxAlphaTexSize || t.height < 1 || t.height > kMaxAlphaTexSize)
            return fault(which + ": width and height must be 1 .. 2^24");
        if (t.wrap != NNBVH_WRAP_REPEAT && t.wrap != NNBVH_WRAP_CLAMP && t.wrap != NNBVH_WRAP_BLACK)
            return fault(which + ": unknown wrap mode (NNBVH_WRAP_REPEAT, _CLAMP or _BLACK; OctahedralSphere is not supported)");
    }
    bool textured = false, patches = false;
    for (int i = 0; prims && i < n_prims; ++i) {
        const nnbvh_prim &p = prims[i];
        patches = patches || is_alpha_patch_kind(p.kind);
        if (!is_alphatex_kind(p.kind)) continue;
        textured = true;
        if (n_textures == 0) return fault("NNBVH_PRIM_ALPHATEX_TRIANGLE primitives need the alpha-texture table");
        if (p.v[3] < 0 || p.v[3] >= n_textures) return fault("alpha-texture index out of range");
        if (is_smooth_alphatex_kind(p.kind) && !normals)
            return fault("NNBVH_PRIM_ALPHATEX_TRIANGLE_SMOOTH primitives need the vertex normals");
    }
    if (textured && patches && !with_patches)  // (two-level scenes run both through their ALPHA = 2 instances)
        return fault("image-textured alpha on triangles and alpha-tested patches (kinds 8 .. 15) in one scene are not "
                     "supported");
    return true;
}

// A descriptor table and texel pool (alpha_texture_math.h) made from the caller's textures and uploaded to `device`: the
// descriptors in order, the images one after another.  false: the error text is set, and what was allocated stays in
// the two pointers for the caller to free (they belong to a scene that is then destroyed).  Shared with the kd scenes.
bool nnbvh::upload_alpha_textures(int device, const nnbvh_alpha_texture *textures, int n_textures, void **d_table,
                                  float **d_texels, int64_t *n_texels) {
    std::vector<AlphaTexDesc> table((size_t)n_textures);
    uint64_t total = 0;
    for (int k = 0; k < n_textures; ++k) {
        const nnbvh_alpha_texture &t = textures[k];
        AlphaTexDesc &d = table[(size_t)k];
        d.texelLo = (uint32_t)total;
        d.texelHi = (uint32_t)(total >> 32);
        d.width = t.width;
        d.height = t.height;
        d.wrap = t.wrap;
        d.pointFilter = t.point_filter ? 1 : 0;
        d.su = t.su, d.sv = t.sv, d.du = t.du, d.dv = t.dv;
        d.scale = t.scale;
        d.invert = t.invert ? 1 : 0;
        total += (uint64_t)t.width * (uint64_t)t.height;
    }
    DeviceGuard guard(device);
    bool ok = guard.ok && hip_ok(hipMalloc(d_table, table.size() * sizeof(AlphaTexDesc)), "hipMalloc(alpha textures)") &&
              hip_ok(hipMalloc((void **)d_texels, (size_t)total * 4), "hipMalloc(alpha texels)") &&
              hip_ok(hipMemcpy(*d_table, table.data(), table.size() * sizeof(AlphaTexDesc), hipMemcpyHostToDevice),
                     "hipMemcpy(alpha textures)");
    uint64_t at = 0;
    for (int k = 0; ok && k < n_textures; ++k) {
        const uint64_t n = (uint64_t)textures[k].width * (uint64_t)textures[k].height;
        ok = hip_ok(hipMemcpy(*d_texels + at, textures[k].texels, (size_t)n * 4, hipMemcpyHostToDevice),
                    "hipMemcpy(alpha texels)");
        at += n;
    }
    *n_texels = (int64_t)total;
    return ok;
}

// the scene's descriptor table and texel pool, uploaded once; false: the scene is destroyed
bool nnbvh::attach_alpha_textures(nnbvh_scene *s, const nnbvh_alpha_texture *textures, int n_textures) {
    if (!s || n_textures <= 0) return s != nullptr;
    int64_t total = 0;
    if (!upload_alpha_textures(s->device, textures, n_textures, &s->d_alpha_tex, &s->d_alpha_texels, &total)) {
        const std::string why = nnbvh_last_error();
        nnbvh_scene_destroy(s);
        set_error(why);
        return false;
    }
    s->n_alpha_tex = n_textures;
    s->n_alpha_texels = total;
    s->device_bytes += (size_t)n_textures * sizeof(AlphaTexDesc) + (size_t)total * 4;
    return true;
}

// The top table of a flat scene that runs the lean instances (top_table.h): the first kTopRecords records breadth-first
// from the root, read back from the baked array one by one (which is only read) and uploaded as an array of the
// scene's own.  Other scenes, and a scene whose root is a leaf, have none.  false: a device call failed.
static bool attach_top_table(nnbvh_scene *s) {
    if (!scene_runs_lean(s)) return true;
    std::vector<WideNode> table;
    std::vector<int32_t> order;
    const auto fetch = [&](int32_t record, WideNode *out) {
        return hip_ok(hipMemcpy(out, s->d_wide + 4 * (size_t)record, sizeof(WideNode), hipMemcpyDeviceToHost),
                      "hipMemcpy(top record)");
    };
    if (!build_top_table(fetch, s->root_ref, s->n_interior, kTopRecords, &table, &order)) return false;
    if (table.empty()) return true;
    const size_t bytes = table.size() * sizeof(WideNode);
    if (!hip_ok(hipMalloc((void **)&s->d_top, bytes), "hipMalloc(top table)") ||
        !hip_ok(hipMemcpy(s->d_top, table.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy(top table)"))
        return false;
    s->n_top = (int)table.size();
    s->device_bytes += bytes;
    return true;
}

// A scene object around arrays baked on the device (bvh_bake.hip): every creation route ends here, with the scene's
// device current.  instanced: a two-level scene, which always runs the general kernels (so it has no top table) and
// counts its one allocation as it was made, records 256-B aligned and the stream's 64 B of padding; a flat scene counts
// the two arrays.  nullptr: the error text is set, the arrays are freed.
nnbvh_scene *nnbvh::scene_from_baked(const BakedScene &b, int depth, int device, bool instanced) {
    hipDeviceProp_t prop;
    if (!hip_ok(hipGetDeviceProperties(&prop, device), "hipGetDeviceProperties")) {
        (void)hipFree(b.d_wide);  // one allocation: d_prims points into it
        return nullptr;
    }
    auto *s = new nnbvh_scene;
    s->device = device;
    s->n_cus = prop.multiProcessorCount;
    s->n_interior = b.n_interior;
    s->n_slots = b.n_slots;
    s->depth = depth;
    std::memcpy(s->bounds, b.bounds, sizeof b.bounds);
    s->root_ref = b.root_ref;
    s->instanced = instanced ? 1 : 0;
    s->has_host_prims = (b.has_host_prims || b.has_alpha) ? 1 : 0;  // an alpha re-trace that hits voids the ray like a host primitive
    // (the alpha test hashes the ray direction, parked with the patches' one)
    s->has_patches = (instanced || b.has_patches || b.has_alpha) ? 1 : 0;
    s->has_alpha = b.has_alpha;
    s->max_grid_threads = s->n_cus * 8 * kBlockThreads;
    s->d_wide = (float4 *)b.d_wide;
    s->d_prims = (float4 *)b.d_prims;
    const size_t records = (size_t)std::max(b.n_interior, 1) * sizeof(WideNode),
                 slots = std::max<size_t>((size_t)b.n_slots, 1) * 16;
    s->device_bytes = instanced ? ((records + 255) & ~(size_t)255) + slots + 64 : records + slots;
    if (hipMalloc((void **)&s->d_stats, nnbvh::kSchedStatWords * sizeof(unsigned long long)) == hipSuccess)
        (void)hipMemset(s->d_stats, 0, nnbvh::kSchedStatWords * sizeof(unsigned long long));
    if (!instanced && !attach_top_table(s)) {
        const std::string why = nnbvh_last_error();
        nnbvh_scene_destroy(s);
        set_error(why);
        return nullptr;
    }
    return s;
}

// the animation table of a two-level scene, one entry per instance, uploaded (not counted in device_bytes).  false:
// the scene is destroyed, the error text is set
bool nnbvh::upload_anim_table(nnbvh_scene *s, const nnbvh_animated_transform *animated, int n_instances) {
    std::vector<float> table((size_t)n_instances * kAnimStride, 0.0f);
    for (int k = 0; k < n_instances; ++k) fill_anim_entry(animated[k], &table[(size_t)k * kAnimStride]);
    if (hip_ok(hipMalloc((void **)&s->d_anim, table.size() * 4), "hipMalloc(animation table)") &&
        hip_ok(hipMemcpy(s->d_anim, table.data(), table.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(animation table)")) {
        s->n_anim = n_instances;
        return true;
    }
    const std::string why = nnbvh_last_error();
    nnbvh_scene_destroy(s);
    set_error(why);
    return false;
}

extern "C" {

const char *nnbvh_last_error(void) { return g_error.c_str(); }

int nnbvh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static nnbvh_scene *create_scene(const nnbvh_linear_node *nodes, int n_nodes, int n_top_nodes,
                                 const nnbvh_prim *prims, int n_prims, const float *verts,
                                 int n_verts, const nnbvh_instance *instances, int n_instances,
                                 int device, const nnbvh_animated_transform *animated = nullptr,
                                 const float *normals = nullptr, const float *prim_alpha = nullptr,
                                 const float *uvs = nullptr, bool alpha_textures = false) {
    if (!nodes || !prims || !verts || n_prims <= 0 || n_verts <= 0 || n_instances < 0 ||
        (n_instances > 0 && !instances) || n_top_nodes < 1 || n_top_nodes > n_nodes) {
        set_error("scene_create: null or empty input array");
        return nullptr;
    }
    std::vector<uint8_t> covered((size_t)n_prims, 0);
    int depth = 0;
    if (!validate_tree(nodes, 0, n_top_nodes, prims, n_prims, n_instances > 0, covered, &depth)) return nullptr;
    // instanced children: trees in nodes[n_top_nodes, n_nodes); several instances may share one.  unnamed: the nodes
    // behind the top tree that no walk below sees (an object no instance places)
    int child_depth = 0;
    std::vector<uint8_t> tree_seen((size_t)n_nodes, 0), unnamed((size_t)n_nodes, 0);
    std::fill(unnamed.begin() + n_top_nodes, unnamed.end(), 1);
    for (int k = 0; k < n_instances; ++k) {
        const nnbvh_instance &in = instances[k];
        if (in.root < n_top_nodes || in.n_nodes < 1 || (int64_t)in.root + in.n_nodes > n_nodes) {
            set_error("scene_create: instance child tree outside the node array");
            return nullptr;
        }
        if (tree_seen[(size_t)in.root]) continue;
        tree_seen[(size_t)in.root] = 1;
        int d = 0;
        if (!validate_tree(nodes, in.root, in.n_nodes, prims, n_prims, false, covered, &d)) return nullptr;
        std::fill(unnamed.begin() + in.root, unnamed.begin() + in.root + in.n_nodes, 0);
        child_depth = std::max(child_depth, d + 1);
    }
    depth += child_depth;  // pending entries of the outer walk + those of the child walk
    if (depth > kMaxStack) {
        // the reference's nodesToVisit[64] (aggregates.cpp:538) would overflow silently
        set_error("scene_create: tree deeper than the 64-entry traversal stack");
        return nullptr;
    }
    // what the bake (bvh_bake.hip) indexes with, and the arrays a kind reads; the stream's slots are only counted
    int64_t n_slots = 0;
    for (int k = 0; k < n_prims; ++k) {
        const nnbvh_prim &p = prims[k];
        int nv, nslots;
        if (is_smooth_alpha_kind(p.kind)) {
            nv = 3;
            nslots = 6;
            if (!normals) {
                set_error("scene_create: NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH primitives need the vertex normals "
                          "(nnbvh_scene_create_with_normals)");
                return nullptr;
            }
        } else if (is_alpha_patch_kind(p.kind)) {
            nv = 4;
            nslots = alpha_patch_slots(p.kind);
            if (!prim_alpha || (is_smooth_alpha_patch_kind(p.kind) && !normals) || (is_uv_alpha_patch_kind(p.kind) && !uvs)) {
                set_error("scene_create: NNBVH_PRIM_ALPHA_PATCH primitives need the per-primitive alpha array, the "
                          "smooth ones the vertex normals, the _UV ones the vertex uvs too "
                          "(nnbvh_scene_create_with_attributes)");
                return nullptr;
            }
        } else if (is_triangle_kind(p.kind)) nv = nslots = 3;
        else if (alpha_textures && is_alphatex_kind(p.kind)) {  // (checked by check_alpha_textures)
            nv = 3;
            nslots = alphatex_slots(p.kind);
        } else if (p.kind == NNBVH_PRIM_BILINEAR_PATCH) nv = nslots = 4;
        else if (p.kind == NNBVH_PRIM_HOST) {
            nv = 0;
            nslots = 3;
        } else if (p.kind == NNBVH_PRIM_INSTANCE) {
            nv = 0;
            nslots = 6;
            if (p.v[0] < 0 || p.v[0] >= n_instances) {
                set_error("scene_create: instance index out of range");
                return nullptr;
            }
        } else {
            set_error(is_alphatex_kind(p.kind) ? std::string("scene_create: ") + kAlphaTexElsewhere
                                               : std::string("scene_create: unknown primitive kind"));
            return nullptr;
        }
        for (int j = 0; j < nv; ++j)
            if (p.v[j] < 0 || p.v[j] >= n_verts) {
                set_error("scene_create: vertex index out of range");
                return nullptr;
            }
        n_slots += nslots;
    }
    if (n_slots >= 0x7ffffffeLL) {
        set_error("scene_create: primitive stream exceeds 2^31 slots");
        return nullptr;
    }
    // the bake makes a record of every interior node and looks up every leaf's slot, the unnamed ones' too: their
    // children and primitive ranges, which validate_tree never saw, must lie inside the arrays
    for (int i = n_top_nodes; i < n_nodes; ++i) {
        const nnbvh_linear_node &nd = nodes[i];
        if (!unnamed[(size_t)i]) continue;
        if (nd.nprims == 0 ? !(nd.axis <= 2 && nd.offset > i + 1 && nd.offset < n_nodes)
                           : !(nd.offset >= 0 && (int64_t)nd.offset + nd.nprims <= n_prims)) {
            set_error("scene_create: malformed node outside every instance's tree");
            return nullptr;
        }
    }

    int n_dev = nnbvh_device_count();
    if (n_dev <= 0 || device < 0 || device >= n_dev) {
        set_error("scene_create: no usable HIP device (this library has no CPU fallback)");
        return nullptr;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    // the caller's arrays go up as they are; the bake's passes over them run on the device (two-level scenes: the
    // instance table in the form the device-built route hands over, object k = instance k's tree)
    Uploads up;
    const void *d_nodes = up.put(nodes, (size_t)n_nodes * sizeof(nnbvh_linear_node), "tree");
    const void *d_prims = up.put(prims, (size_t)n_prims * sizeof(nnbvh_prim), "primitives");
    const void *d_verts = up.put(verts, (size_t)n_verts * 12, "vertices");
    const void *d_normals = up.put(normals, (size_t)n_verts * 12, "normals");
    const void *d_alpha = up.put(prim_alpha, (size_t)n_prims * 4, "primitive alpha");
    const void *d_uvs = up.put(uvs, (size_t)n_verts * 8, "uvs");
    InstanceBake inst;
    if (n_instances > 0) {
        std::vector<nnbvh_placement> placements((size_t)n_instances);
        std::vector<int32_t> roots((size_t)n_instances);
        std::vector<unsigned char> moving((size_t)n_instances, 0);
        for (int k = 0; k < n_instances; ++k) {
            nnbvh_placement &pl = placements[(size_t)k];
            std::memcpy(pl.render_from_prim, instances[k].render_from_prim, sizeof pl.render_from_prim);
            std::memcpy(pl.prim_from_render, instances[k].prim_from_render, sizeof pl.prim_from_render);
            pl.object = k;
            pl.pad = 0;
            roots[(size_t)k] = instances[k].root;
            moving[(size_t)k] = animated && animated[k].actually_animated ? 1 : 0;
        }
        inst.d_placements = (const nnbvh_placement *)up.put(placements.data(), placements.size() * sizeof(nnbvh_placement), "instances");
        inst.d_object_root = (const int *)up.put(roots.data(), roots.size() * sizeof(int32_t), "instances");
        inst.d_animated = (const unsigned char *)up.put(animated ? moving.data() : nullptr, moving.size(), "instances");
        inst.d_node_unnamed = (const unsigned char *)up.put(unnamed.data(), unnamed.size(), "tree");
    }
    if (!up.ok) return nullptr;
    BakedScene b;
    std::string err;
    if (!bake_on_device(d_nodes, n_nodes, d_prims, n_prims, d_verts, device, &b, &err, d_normals, d_alpha, d_uvs,
                        n_instances > 0 ? &inst : nullptr)) {
        set_error(err);
        return nullptr;
    }
    nnbvh_scene *s = scene_from_baked(b, depth, device, n_instances > 0);
    if (s && animated && n_instances > 0 && !upload_anim_table(s, animated, n_instances)) return nullptr;
    return s;
}

// Triangles in, traceable scene out, without the tree leaving the device: device build
// (bvh_build_gpu.hip) + device bake (bvh_bake.hip).  Same tree, same baked arrays, hence the same
// results as nnbvh_build_create + nnbvh_scene_create.
nnbvh_scene *nnbvh_scene_create_gpu_build(const nnbvh_prim *prims, int n_prims, const float *verts,
                                          int n_verts, const float *prim_bounds,
                                          int max_prims_in_node, int split_method, int device) {
    return nnbvh_scene_create_gpu_build_with_attributes(prims, n_prims, verts, n_verts, prim_bounds, nullptr, nullptr,
                                                        nullptr, max_prims_in_node, split_method, device);
}

// (alpha_textures: the caller has checked the table; without it the kinds 16 .. 19 are unknown here)
static nnbvh_scene *create_scene_gpu_build(const nnbvh_prim *prims_in, int n_prims, const float *verts, int n_verts,
                                           const float *prim_bounds, const float *normals, const float *uvs,
                                           const float *prim_alpha, int max_prims_in_node, int split_method, int device,
                                           bool alpha_textures) {
    for (int i = 0; prims_in && !alpha_textures && i < n_prims; ++i)
        if (is_alphatex_kind(prims_in[i].kind)) {
            set_error(std::string("nnbvh_build_create: ") + kAlphaTexElsewhere);
            return nullptr;
        }
    const nnbvh_prim *prims = prims_in;
    // with a per-primitive array to carry along, the build runs with ids = positions; the bake's gather pass puts the
    // caller's ids back (bvh_bake.hip)
    std::vector<nnbvh_prim> tagged;
    std::vector<int32_t> caller_ids;
    if (prims_in && prim_alpha && n_prims > 0) {
        tagged.assign(prims_in, prims_in + n_prims);
        caller_ids.resize((size_t)n_prims);
        for (int i = 0; i < n_prims; ++i) {
            caller_ids[(size_t)i] = tagged[(size_t)i].id;
            tagged[(size_t)i].id = i;
        }
        prims = tagged.data();
    }
    if (!prims || !verts || n_prims <= 0 || n_verts <= 0) {
        set_error("scene_create_gpu_build: empty primitive or vertex array");
        return nullptr;
    }
    if (split_method != NNBVH_SPLIT_SAH && split_method != NNBVH_SPLIT_HLBVH) {
        set_error("scene_create_gpu_build: only the sah and hlbvh split methods are built on the device");
        return nullptr;
    }
    int n_dev = nnbvh_device_count();
    if (n_dev <= 0 || device < 0 || device >= n_dev) {
        set_error("scene_create_gpu_build: no usable HIP device (this library has no CPU fallback)");
        return nullptr;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return nullptr;
    GpuBuildResult r;
    r.keep_on_device = true;
    std::string err;
    const bool built = split_method == NNBVH_SPLIT_SAH
                           ? gpu_sah(prims, n_prims, verts, n_verts, prim_bounds, max_prims_in_node, device, &r, &err)
                           : gpu_hlbvh(prims, n_prims, verts, n_verts, prim_bounds, max_prims_in_node, device, &r, &err);
    if (!built) {
        set_error(err);
        return nullptr;
    }
    BakedScene b;
    bool ok = r.depth <= kMaxStack;
    if (!ok) err = "scene_create: tree deeper than the 64-entry traversal stack";
    void *d_normals = nullptr, *d_alpha = nullptr, *d_uvs = nullptr;
    if (ok && uvs) {
        ok = hip_ok(hipMalloc(&d_uvs, (size_t)n_verts * 8), "hipMalloc(uvs)") &&
             hip_ok(hipMemcpy(d_uvs, uvs, (size_t)n_verts * 8, hipMemcpyHostToDevice), "hipMemcpy(uvs)");
        if (!ok) err = nnbvh_last_error();
    }
    if (ok && normals) {
        ok = hip_ok(hipMalloc(&d_normals, (size_t)n_verts * 12), "hipMalloc(normals)") &&
             hip_ok(hipMemcpy(d_normals, normals, (size_t)n_verts * 12, hipMemcpyHostToDevice), "hipMemcpy(normals)");
        if (!ok) err = nnbvh_last_error();
    }
    if (ok && prim_alpha)
        ok = gather_prim_alpha_on_device(r.d_ordered, n_prims, prim_alpha, caller_ids.data(), &d_alpha, &err);
    ok = ok && bake_on_device(r.d_nodes, r.total_nodes, r.d_ordered, n_prims, r.d_verts, device, &b, &err, d_normals, d_alpha,
                              d_uvs);
    for (void *p : {r.d_nodes, r.d_ordered, r.d_verts, d_normals, d_alpha, d_uvs})
        if (p) (void)hipFree(p);
    if (!ok) {
        set_error(err);
        return nullptr;
    }
    nnbvh_scene *s = scene_from_baked(b, r.depth, device, false);
    if (!s) return nullptr;
    s->build_ms[0] = r.ms[0] + r.ms[1] + r.ms[2] + r.ms[3] + r.ms[4];
    return s;
}

nnbvh_scene *nnbvh_scene_create_gpu_build_with_attributes(const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const float *prim_bounds, const float *normals,
                                                          const float *uvs, const float *prim_alpha,
                                                          int max_prims_in_node, int split_method, int device) {
    return create_scene_gpu_build(prims, n_prims, verts, n_verts, prim_bounds, normals, uvs, prim_alpha, max_prims_in_node,
                                  split_method, device, false);
}

nnbvh_scene *nnbvh_scene_create_gpu_build_with_alpha_textures(const nnbvh_prim *prims, int n_prims, const float *verts,
                                                              int n_verts, const float *prim_bounds,
                                                              const float *normals, const float *uvs,
                                                              const float *prim_alpha, int max_prims_in_node,
                                                              int split_method, int device,
                                                              const nnbvh_alpha_texture *textures, int n_textures) {
    if (!check_alpha_textures("nnbvh_scene_create_gpu_build_with_alpha_textures", prims, n_prims, normals, textures, n_textures))
        return nullptr;
    nnbvh_scene *s = create_scene_gpu_build(prims, n_prims, verts, n_verts, prim_bounds, normals, uvs, prim_alpha,
                                            max_prims_in_node, split_method, device, true);
    return attach_alpha_textures(s, textures, n_textures) ? s : nullptr;
}

nnbvh_scene *nnbvh_scene_create_with_alpha_textures(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                                    int n_prims, const float *verts, const float *normals,
                                                    const float *uvs, const float *prim_alpha, int n_verts, int device,
                                                    const nnbvh_alpha_texture *textures, int n_textures) {
    if (!check_alpha_textures("nnbvh_scene_create_with_alpha_textures", prims, n_prims, normals, textures, n_textures))
        return nullptr;
    nnbvh_scene *s = create_scene(nodes, n_nodes, n_nodes, prims, n_prims, verts, n_verts, nullptr, 0, device, nullptr,
                                  normals, prim_alpha, uvs, true);
    return attach_alpha_textures(s, textures, n_textures) ? s : nullptr;
}

nnbvh_scene *nnbvh_scene_create(const nnbvh_linear_node *nodes, int n_nodes,
                                const nnbvh_prim *prims, int n_prims, const float *verts,
                                int n_verts, int device) {
    return create_scene(nodes, n_nodes, n_nodes, prims, n_prims, verts, n_verts, nullptr, 0, device);
}

nnbvh_scene *nnbvh_scene_create_with_attributes(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                                int n_prims, const float *verts, const float *normals,
                                                const float *uvs, const float *prim_alpha, int n_verts, int device) {
    return create_scene(nodes, n_nodes, n_nodes, prims, n_prims, verts, n_verts, nullptr, 0, device, nullptr, normals,
                        prim_alpha, uvs);
}

nnbvh_scene *nnbvh_scene_create_with_normals(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                             int n_prims, const float *verts, const float *normals, int n_verts,
                                             int device) {
    return create_scene(nodes, n_nodes, n_nodes, prims, n_prims, verts, n_verts, nullptr, 0, device, nullptr, normals);
}

nnbvh_scene *nnbvh_scene_create_instanced(const nnbvh_linear_node *nodes, int n_nodes,
                                          int n_top_nodes, const nnbvh_prim *prims, int n_prims,
                                          const float *verts, int n_verts,
                                          const nnbvh_instance *instances, int n_instances,
                                          int device) {
    return create_scene(nodes, n_nodes, n_top_nodes, prims, n_prims, verts, n_verts, instances,
                        n_instances, device);
}

nnbvh_scene *nnbvh_scene_create_instanced_animated(const nnbvh_linear_node *nodes, int n_nodes,
                                                   int n_top_nodes, const nnbvh_prim *prims, int n_prims,
                                                   const float *verts, int n_verts,
                                                   const nnbvh_instance *instances, int n_instances,
                                                   const nnbvh_animated_transform *animated, int device) {
    if (animated)
        for (int k = 0; k < n_instances; ++k)
            if (animated[k].actually_animated && !(animated[k].end_time > animated[k].start_time)) {
                set_error("scene_create: animated instance with an empty time range");
                return nullptr;
            }
    return create_scene(nodes, n_nodes, n_top_nodes, prims, n_prims, verts, n_verts, instances,
                        n_instances, device, animated);
}

nnbvh_scene *nnbvh_scene_create_instanced_with_attributes(const nnbvh_linear_node *nodes, int n_nodes, int n_top_nodes,
                                                          const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const nnbvh_instance *instances, int n_instances,
                                                          const nnbvh_animated_transform *animated, const float *normals,
                                                          const float *uvs, const float *prim_alpha, int device) {
    if (animated)
        for (int k = 0; k < n_instances; ++k)
            if (animated[k].actually_animated && !(animated[k].end_time > animated[k].start_time)) {
                set_error("scene_create: animated instance with an empty time range");
                return nullptr;
            }
    return create_scene(nodes, n_nodes, n_top_nodes, prims, n_prims, verts, n_verts, instances, n_instances, device,
                        animated, normals, prim_alpha, uvs);
}

nnbvh_scene *nnbvh_scene_create_instanced_with_alpha_textures(const nnbvh_linear_node *nodes, int n_nodes, int n_top_nodes,
                                                              const nnbvh_prim *prims, int n_prims, const float *verts,
                                                              int n_verts, const nnbvh_instance *instances,
                                                              int n_instances, const nnbvh_animated_transform *animated,
                                                              const float *normals, const float *uvs,
                                                              const float *prim_alpha, int device,
                                                              const nnbvh_alpha_texture *textures, int n_textures) {
    const char *fn = "nnbvh_scene_create_instanced_with_alpha_textures";
    if (!check_alpha_textures(fn, prims, n_prims, normals, textures, n_textures, true)) return nullptr;
    if (n_instances <= 0 || !instances) {  // (create_scene bakes a scene without instances as a flat one)
        set_error(std::string(fn) + ": a two-level scene needs its instance table (flat scenes: "
                                    "nnbvh_scene_create_with_alpha_textures)");
        return nullptr;
    }
    if (animated)
        for (int k = 0; k < n_instances; ++k)
            if (animated[k].actually_animated && !(animated[k].end_time > animated[k].start_time)) {
                set_error("scene_create: animated instance with an empty time range");
                return nullptr;
            }
    nnbvh_scene *s = create_scene(nodes, n_nodes, n_top_nodes, prims, n_prims, verts, n_verts, instances, n_instances,
                                  device, animated, normals, prim_alpha, uvs, true);
    return attach_alpha_textures(s, textures, n_textures) ? s : nullptr;
}

nnbvh_scene *nnbvh_scene_create_instanced_gpu_build_with_alpha_textures(
    const nnbvh_prim *prims, int n_prims, int n_top_prims, const int32_t *object_first, int n_objects, const float *verts,
    int n_verts, const float *normals, const float *uvs, const float *prim_alpha, const float *prim_bounds,
    const nnbvh_placement *placements, int n_placements, const nnbvh_animated_transform *animated, int max_prims_in_node,
    int split_method, int device, const nnbvh_alpha_texture *textures, int n_textures) {
    const char *fn = "nnbvh_scene_create_instanced_gpu_build_with_alpha_textures";
    if (!check_alpha_textures(fn, prims, n_prims, normals, textures, n_textures, true)) return nullptr;
    nnbvh_scene *s = create_instanced_gpu_build(prims, n_prims, n_top_prims, object_first, n_objects, verts, n_verts,
                                                normals, uvs, prim_alpha, prim_bounds, placements, n_placements, animated,
                                                max_prims_in_node, split_method, device, true);
    return attach_alpha_textures(s, textures, n_textures) ? s : nullptr;
}

void nnbvh_transform_bounds(const float m[12], const float in[6], float out[6]) {
    transform_bounds(m, in, out);  // nnbvh_internal.h: shared with the device's instance bounds
}

void nnbvh_scene_destroy(nnbvh_scene *s) {
    if (!s) return;
    DeviceGuard guard(s->device);
    (void)hipDeviceSynchronize();
    for (auto &kv : s->workspaces) {
        Workspace &w = kv.second;
        void *ptrs[] = {w.queue, w.spill, w.d_in, w.d_out, w.d_aux0, w.d_aux1, w.d_hits};
        for (void *p : ptrs)
            if (p) (void)hipFree(p);
        for (void *p : w.scratch)
            if (p) (void)hipFree(p);
    }
    for (HostSlot &sl : s->host_slots) {
        for (void *p : {sl.d_in, sl.d_out[0], sl.d_out[1], sl.d_out[2]})
            if (p) (void)hipFree(p);
        for (void *p : {sl.h_in, sl.h_out[0], sl.h_out[1], sl.h_out[2]})
            if (p) (void)hipHostFree(p);
        for (hipEvent_t e : {sl.ev_in, sl.ev_traced, sl.ev_out})
            if (e) (void)hipEventDestroy(e);
    }
    for (hipStream_t st : {s->host_up, s->host_trace, s->host_down})
        if (st) (void)hipStreamDestroy(st);
    for (int k = 0; k < nnbvh_scene::kSideStreams; ++k) {
        if (s->side[k]) (void)hipStreamDestroy(s->side[k]);
        if (s->ev_join[k]) (void)hipEventDestroy(s->ev_join[k]);
    }
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    (void)hipFree(s->d_wide);  // d_prims points into the same allocation
    if (s->d_anim) (void)hipFree(s->d_anim);
    if (s->d_alpha_tex) (void)hipFree(s->d_alpha_tex);
    if (s->d_alpha_texels) (void)hipFree(s->d_alpha_texels);
    if (s->d_top) (void)hipFree(s->d_top);
    if (s->d_stats) (void)hipFree(s->d_stats);
    delete s;
}

int nnbvh_scene_bounds(const nnbvh_scene *s, float out[6]) {
    if (!s || !out) {
        set_error("scene_bounds: null argument");
        return NNBVH_ERR_ARG;
    }
    std::memcpy(out, s->bounds, sizeof s->bounds);
    return NNBVH_OK;
}

int nnbvh_scene_info(const nnbvh_scene *s, int64_t out[6]) {
    if (!s || !out) {
        set_error("scene_info: null argument");
        return NNBVH_ERR_ARG;
    }
    out[0] = s->n_interior;
    out[1] = s->n_slots;
    out[2] = s->depth;
    out[3] = (int64_t)s->device_bytes;
    out[4] = grid_blocks(const_cast<nnbvh_scene *>(s), 0);
    out[5] = s->window;
    return NNBVH_OK;
}

int nnbvh_scene_read(const nnbvh_scene *s, int what, void *out, size_t bytes) {
    if (!s || !out) {
        set_error("scene_read: null argument");
        return NNBVH_ERR_ARG;
    }
    if (what < 0 || what > 4) {
        set_error("scene_read: unknown array (0 interior records, 1 primitive stream, 2 animation table, 3 alpha-texture "
                  "table, 4 alpha texel pool)");
        return NNBVH_ERR_ARG;
    }
    if (what >= 3) {
        if (!s->d_alpha_tex) {
            set_error("scene_read: the scene has no alpha textures");
            return NNBVH_ERR_ARG;
        }
        const void *from = what == 3 ? (const void *)s->d_alpha_tex : (const void *)s->d_alpha_texels;
        const size_t size = what == 3 ? (size_t)s->n_alpha_tex * 48 : (size_t)s->n_alpha_texels * 4;
        if (bytes != size) {
            set_error("scene_read: " + std::to_string(bytes) + " bytes asked for, the array has " + std::to_string(size));
            return NNBVH_ERR_ARG;
        }
        DeviceGuard guard(s->device);
        if (!guard.ok) return NNBVH_ERR_DEVICE;
        if (!hip_ok(hipDeviceSynchronize(), "scene_read") || !hip_ok(hipMemcpy(out, from, bytes, hipMemcpyDeviceToHost), "scene_read"))
            return NNBVH_ERR_DEVICE;
        return NNBVH_OK;
    }
    if (what == 2 && !s->d_anim) {
        set_error("scene_read: the scene has no animation table");
        return NNBVH_ERR_ARG;
    }
    const void *src = what == 0 ? (const void *)s->d_wide : what == 1 ? (const void *)s->d_prims : (const void *)s->d_anim;
    const size_t have = what == 0   ? (size_t)s->n_interior * sizeof(WideNode)
                        : what == 1 ? (size_t)s->n_slots * 16
                                    : (size_t)s->n_anim * kAnimStride * sizeof(float);
    if (bytes != have) {
        set_error("scene_read: " + std::to_string(bytes) + " bytes asked for, the array has " + std::to_string(have));
        return NNBVH_ERR_ARG;
    }
    if (bytes == 0) return NNBVH_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    if (!hip_ok(hipDeviceSynchronize(), "scene_read") || !hip_ok(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost), "scene_read"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

int nnbvh_scene_sched_stats(nnbvh_scene *s, uint64_t out[20], int reset) {
    if (!s || !out) {
        set_error("scene_sched_stats: null argument");
        return NNBVH_ERR_ARG;
    }
    std::memset(out, 0, nnbvh::kSchedStatWords * sizeof(uint64_t));
    if (!s->d_stats) return NNBVH_OK;
    DeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    if (!hip_ok(hipDeviceSynchronize(), "scene_sched_stats") ||
        !hip_ok(hipMemcpy(out, s->d_stats, nnbvh::kSchedStatWords * sizeof(uint64_t), hipMemcpyDeviceToHost),
                "scene_sched_stats"))
        return NNBVH_ERR_DEVICE;
    if (reset) (void)hipMemset(s->d_stats, 0, nnbvh::kSchedStatWords * sizeof(unsigned long long));
    return NNBVH_OK;
}

// Tests only, not part of include/nnbvh.h: the LDS top table of the lean one-launch kernels (top_extend.h), as each of
// `blocks` blocks builds it in the kernels' prologue (device_tables: blocks x *capacity records of 64 B, device_counts:
// the records each block holds) and as the host's extend_top_table builds it from the same scene table and records
// (host_table: *capacity records, *host_count).  A scene without a table gives counts of 0.
int nnbvh_debug_top_table(nnbvh_scene *s, int blocks, void *device_tables, int32_t *device_counts, void *host_table,
                          int32_t *host_count, int32_t *capacity) {
    if (!s || blocks < 1 || blocks > 4096 || !device_tables || !device_counts || !host_table || !host_count || !capacity) {
        set_error("debug_top_table: bad argument");
        return NNBVH_ERR_ARG;
    }
    const int cap = top_debug_capacity();
    *capacity = cap;
    DeviceGuard guard(s->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    std::vector<WideNode> table((size_t)s->n_top);
    std::vector<int32_t> order;
    if (s->n_top > 0 && !hip_ok(hipMemcpy(table.data(), s->d_top, table.size() * sizeof(WideNode), hipMemcpyDeviceToHost),
                                "hipMemcpy(top table)"))
        return NNBVH_ERR_DEVICE;
    const auto fetch = [&](int32_t record, WideNode *out) {
        if (record < 0 || record >= s->n_interior) return false;
        return hip_ok(hipMemcpy(out, s->d_wide + 4 * (size_t)record, sizeof(WideNode), hipMemcpyDeviceToHost),
                      "hipMemcpy(top record)");
    };
    if (!extend_top_table(fetch, cap, &table, &order)) return NNBVH_ERR_DEVICE;
    *host_count = (int32_t)table.size();
    std::memcpy(host_table, table.data(), table.size() * sizeof(WideNode));
    const size_t bytes = (size_t)blocks * (size_t)cap * sizeof(WideNode);
    float4 *d_out = nullptr;
    int *d_n = nullptr;
    bool ok = hip_ok(hipMalloc((void **)&d_out, bytes), "hipMalloc(debug tables)") &&
              hip_ok(hipMalloc((void **)&d_n, (size_t)blocks * sizeof(int)), "hipMalloc(debug counts)") &&
              hip_ok(hipMemset(d_out, 0, bytes), "hipMemset(debug tables)") &&
              hip_ok(launch_top_table_debug(s->d_top, s->n_top, s->d_wide, blocks, d_out, d_n, nullptr),
                     "top table debug launch") &&
              hip_ok(hipDeviceSynchronize(), "top table debug kernel") &&
              hip_ok(hipMemcpy(device_tables, d_out, bytes, hipMemcpyDeviceToHost), "hipMemcpy(debug tables)") &&
              hip_ok(hipMemcpy(device_counts, d_n, (size_t)blocks * sizeof(int), hipMemcpyDeviceToHost),
                     "hipMemcpy(debug counts)");
    if (d_out) (void)hipFree(d_out);
    if (d_n) (void)hipFree(d_n);
    return ok ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

int nnbvh_instance_launches(int family, int32_t *desc, uint64_t *counts, int capacity, int reset) {
    if ((family != 0 && family != 1) || capacity < 0 || (capacity > 0 && !desc && !counts)) {
        set_error("instance_launches: family 0 (BVH trace instances) or 1 (kd-tree ones), capacity >= 0 and an array to fill");
        return -NNBVH_ERR_ARG;
    }
    return family == 0 ? trace_instance_launches(desc, counts, capacity, reset)
                       : kd_instance_launches(desc, counts, capacity, reset);
}

int nnbvh_scene_set_option(nnbvh_scene *s, const char *key, int value) {
    // (checked before the scene is looked at: a bad value is refused whatever the scene is)
    if (key && std::string(key) == "offsets32" && value != 0 && value != 1) {
        set_error("set_option: offsets32 must be 0 or 1");
        return NNBVH_ERR_ARG;
    }
    if (!s || !key) {
        set_error("set_option: null argument");
        return NNBVH_ERR_ARG;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    std::string k(key);
    if (k == "stack_window") {
        if (value != 4 && value != 8 && value != 16) {
            set_error("set_option: stack_window must be 4, 8 or 16");
            return NNBVH_ERR_ARG;
        }
        s->window = value;
    } else if (k == "blocks_per_cu") {
        if (value < 0 || value > 8) {
            set_error("set_option: blocks_per_cu must be 0..8");
            return NNBVH_ERR_ARG;
        }
        s->blocks_per_cu = value;
    } else if (k == "int_repeat") {
        if (value < 1 || value > 16) {
            set_error("set_option: int_repeat must be 1..16");
            return NNBVH_ERR_ARG;
        }
        s->int_repeat = value;
    } else if (k == "host_chunk") {
        if (value < 1024) {
            set_error("set_option: host_chunk must be at least 1024 rays");
            return NNBVH_ERR_ARG;
        }
        s->host_chunk = value;
    } else if (k == "prim_repeat") {
        if (value < 1 || value > 16) {
            set_error("set_option: prim_repeat must be 1..16");
            return NNBVH_ERR_ARG;
        }
        s->prim_repeat = value;
    } else if (k == "fused_batches") {
        s->fused_batches = value ? 1 : 0;
    } else if (k == "offsets32") {
        // 0: scene_fits32 reports 0 although the arrays fit; 1: what their sizes say.  The walk instances' resident
        // blocks per CU are cached per form: dropped, as a width's form may be asked again after a change to the
        // instance table.  The top table itself (d_top / n_top) depends on the tree alone and stays; whether a launch
        // uses it is decided per launch from scene_runs_lean
        if (s->offsets32 != value)
            for (int &b : s->walk_blocks_per_cu) b = 0;
        s->offsets32 = value;
    } else if (k == "top_table") {
        s->use_top = value ? 1 : 0;
    } else if (k == "top_burst") {
        if (value < 1 || value > 65) {
            set_error("set_option: top_burst must be 1..65");
            return NNBVH_ERR_ARG;
        }
        s->top_burst = value;
    } else if (k == "xcd_queues") {
        s->xcd_queues = value ? 1 : 0;
    } else if (k == "prim_weight") {
        if (value < 1 || value > 64) {
            set_error("set_option: prim_weight must be 1..64");
            return NNBVH_ERR_ARG;
        }
        s->prim_weight = value;
    } else if (k == "refill_weight") {
        if (value < 1 || value > 64) {
            set_error("set_option: refill_weight must be 1..64");
            return NNBVH_ERR_ARG;
        }
        s->refill_weight = value;
    } else {
        set_error("set_option: unknown key");
        return NNBVH_ERR_ARG;
    }
    return NNBVH_OK;
}

}  // extern "C"

Workspace *nnbvh::workspace_for(nnbvh_scene *s, hipStream_t stream) {
    auto it = s->workspaces.find(stream);
    if (it != s->workspaces.end()) return &it->second;
    Workspace w;
    // an entry is spilled only when W - 1 newer ones sit above it (W >= 4): levels 0 .. depth - 3 of a lane's list
    const size_t spill_bytes = (size_t)std::max(s->depth - 2, 1) * (size_t)s->max_grid_threads * sizeof(uint2);
    if (!hip_ok(hipMalloc((void **)&w.queue, kMaxFusedBatches * kMaxQueues * kQueueStrideWords * sizeof(unsigned)),
                "hipMalloc(queue)"))
        return nullptr;
    if (!hip_ok(hipMalloc((void **)&w.spill, spill_bytes), "hipMalloc(spill)")) {
        (void)hipFree(w.queue);
        return nullptr;
    }
    return &(s->workspaces[stream] = w);
}
