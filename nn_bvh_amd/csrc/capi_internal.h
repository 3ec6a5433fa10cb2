// capi_internal.h — what the host files of the C ABI share (bvh_capi.cpp, capi_trace.cpp, capi_kd.cpp,
// capi_wavefront.cpp, capi_shading.cpp): the scene object, per-stream workspaces, the call prologue and the trace-job
// launcher.
// Included by .cpp files only, never by device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "bvh_trace.h"
#include "interaction.h"
#include "kd_trace.h"

namespace nnbvh {

inline bool hip_ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    set_error(std::string(what) + ": " + hipGetErrorString(e));
    return false;
}

struct DeviceGuard {
    int prev = -1;
    bool ok = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        ok = hip_ok(hipSetDevice(dev), "hipSetDevice");
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// device copies of a creation call's host arrays (the current device's), freed on every way out
struct Uploads {
    std::vector<void *> ptrs;
    bool ok = true;
    // src == nullptr (an array the caller did not give): nullptr, and nothing is wrong
    const void *put(const void *src, size_t bytes, const char *what) {
        void *d = nullptr;
        if (!src || !ok) return nullptr;
        ok = hip_ok(hipMalloc(&d, std::max<size_t>(bytes, 16)), (std::string("hipMalloc(") + what + ")").c_str());
        if (ok) ptrs.push_back(d);
        ok = ok && hip_ok(hipMemcpy(d, src, bytes, hipMemcpyHostToDevice), (std::string("hipMemcpy(") + what + ")").c_str());
        return d;
    }
    ~Uploads() {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

struct Workspace {
    unsigned *queue = nullptr;  // kMaxQueues heads
    uint2 *spill = nullptr;
    // grow-only staging for the host-buffer entry points
    void *d_in = nullptr, *d_out = nullptr, *d_aux0 = nullptr, *d_aux1 = nullptr;
    size_t in_bytes = 0, out_bytes = 0, aux_bytes = 0;
    void *d_hits = nullptr;  // hit records of the *_items calls made without d_hits
    size_t hits_bytes = 0;
    // grow-only scratch of the multi-pass and walk entry points (IntersectShadowTr / IntersectOneRandom): ping-pong
    // ray records and item lists, the hit records of a pass, per-item state, pass counters.  Per stream like the queue
    // heads: the calls are asynchronous on their stream, so two streams must not share them
    enum Slot { kRaysA, kRaysB, kHits, kOrigA, kOrigB, kPLight, kState, kCounters, kRng, kWeights, kScratch };
    void *scratch[kScratch] = {};
    size_t scratch_bytes[kScratch] = {};
};

// one slot of the host-buffer pipeline (nnbvh_intersect_closest / _any): device chunk buffers, events and — for
// callers with pageable memory — pinned staging buffers
struct HostSlot {
    hipEvent_t ev_in = nullptr, ev_traced = nullptr, ev_out = nullptr;  // rays uploaded / chunk traced / results down
    void *d_in = nullptr, *h_in = nullptr;
    size_t d_in_bytes = 0, h_in_bytes = 0;
    void *d_out[3] = {nullptr, nullptr, nullptr}, *h_out[3] = {nullptr, nullptr, nullptr};
    size_t d_out_bytes[3] = {0, 0, 0}, h_out_bytes[3] = {0, 0, 0};
};

}  // namespace nnbvh

struct nnbvh_scene {
    int device = 0;
    int n_cus = 0;
    int n_interior = 0;
    int64_t n_slots = 0;
    int depth = 0;
    float bounds[6];
    int root_ref = 0;
    float4 *d_wide = nullptr;
    float4 *d_prims = nullptr;
    float *d_anim = nullptr;  // AnimatedPrimitive table (kAnimStride floats per instance), or null
    int n_anim = 0;           // its entries
    size_t device_bytes = 0;
    // tuning (speed only)
    int window = 8;
    int blocks_per_cu = 0;  // 0 = from the occupancy query
    int xcd_queues = 1;
    int prim_weight = 32;
    int refill_weight = 8;
    unsigned long long *d_stats = nullptr;  // diagnostics (NNBVH_STATS builds)
    int instanced = 0;      // two-level scene: use the INST kernels
    int has_host_prims = 0;
    int has_patches = 1;    // 0: no bilinear patches, the lean kernels (no ray direction parked in LDS) run
    int has_alpha = 0;      // 1: alpha-tested triangles present (the ALPHA kernels run), 2: alpha-tested patches too,
                            // 3: triangles with an image-textured alpha (and maybe constant ones; no alpha-tested patches);
                            // a two-level scene reports 2 for textured triangles too (its ALPHA = 2 instances evaluate them)
    int fused_batches = 1;  // nnbvh_trace_batches_device: one mode-3 launch where the batches allow it
    int int_repeat = 3;
    int prim_repeat = 2;
    int max_grid_threads = 0;
    // resident blocks per CU of the walk instances (0 = not asked yet): shadow-tr lean / general / two-level, then
    // one-random's three
    int walk_blocks_per_cu[6] = {0, 0, 0, 0, 0, 0};
    double build_ms[1] = {0};  // device build time of nnbvh_scene_create_gpu_build / _instanced_gpu_build
    std::mutex mu;
    std::map<hipStream_t, nnbvh::Workspace> workspaces;
    static constexpr int kHostSlots = 3, kHostChunks = 6;
    nnbvh::HostSlot host_slots[kHostSlots];
    hipStream_t host_up = nullptr, host_trace = nullptr, host_down = nullptr;
    int64_t host_chunk = 1 << 20;  // least rays per chunk of the host-buffer pipeline (at most kHostChunks chunks)
    // fork/join machinery of nnbvh_trace_batches_device
    static constexpr int kSideStreams = 4;
    hipStream_t side[kSideStreams] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr;
    hipEvent_t ev_join[kSideStreams] = {nullptr, nullptr, nullptr, nullptr};
    // (last: the members above keep their places)
    // image-textured alpha (kinds 16 .. 19): descriptor table (AlphaTexDesc, alpha_texture_math.h) and texel pool, or null
    void *d_alpha_tex = nullptr;
    float *d_alpha_texels = nullptr;
    int n_alpha_tex = 0;
    int64_t n_alpha_texels = 0;
    // the top table of a lean scene (top_table.h): n_top records of 64 B, or null (the root is a leaf; not a lean scene)
    float4 *d_top = nullptr;
    int n_top = 0;
    int use_top = 1;  // option "top_table" (speed only): 0 = the lean one-launch kernels read every record from d_wide
    int offsets32 = 1;  // option "offsets32" (speed only): 0 = scene_fits32 reports 0 although the arrays fit, so the scene
                        // is never lean (the general instances' 64-bit addressing, no LDS top table, p.fits32 = 0)
    int top_burst = 24;  // option "top_burst": tagged interior lanes that make a wave take a table step (65 = never);
                         // crown step: 16 .. 32 within 0.5 % of each other, 8 and 48 slower (profiles/top_table_steps.txt)
};

struct nnbvh_shading_mesh {
    int device = 0;
    int n_cus = 0;
    nnbvh::ShadingMeshDevice d;
};

namespace nnbvh {

// One workspace per stream: launches on one stream are ordered, so they may share the
// queue heads and the spill array; launches on different streams get their own.  (bvh_capi.cpp)
Workspace *workspace_for(nnbvh_scene *s, hipStream_t stream);

// one entry of the device's animation table (layout: anim_math.h; bvh_capi.cpp)
void fill_anim_entry(const nnbvh_animated_transform &a, float *t);

// The end of every BVH creation route (bvh_capi.cpp): the scene object around the arrays bake_on_device made
// (bvh_build_gpu.h), and for a two-level scene with AnimatedPrimitive instances its animation table.  Both are called
// with the scene's device current; after a failure nothing is left allocated and the error text is set.
struct BakedScene;
nnbvh_scene *scene_from_baked(const BakedScene &b, int depth, int device, bool instanced);
bool upload_anim_table(nnbvh_scene *s, const nnbvh_animated_transform *animated, int n_instances);

// the descriptor table (AlphaTexDesc, 48 B each) and the texel pool of a checked alpha-texture table, uploaded to
// `device` for a scene of either type (bvh_capi.cpp).  false: the error text is set; the pointers hold what was allocated
bool upload_alpha_textures(int device, const nnbvh_alpha_texture *textures, int n_textures, void **d_table,
                           float **d_texels, int64_t *n_texels);

// the descriptor table and texel pool of a BVH scene (flat or two-level), uploaded once and counted in device_bytes
// (bvh_capi.cpp).  s == nullptr or no texture: nothing to do, s != nullptr is returned.  false after a failed upload:
// the scene is destroyed, the error text is set
bool attach_alpha_textures(nnbvh_scene *s, const nnbvh_alpha_texture *textures, int n_textures);

// nnbvh_scene_create_instanced_gpu_build and its twin with an alpha-texture table (capi_two_level.cpp).  alpha_textures:
// the caller has checked the table (check_alpha_textures) and attaches it; without it the kinds 16 .. 19 are refused
nnbvh_scene *create_instanced_gpu_build(const nnbvh_prim *prims, int n_prims, int n_top_prims,
                                        const int32_t *object_first, int n_objects, const float *verts, int n_verts,
                                        const float *normals, const float *uvs, const float *prim_alpha,
                                        const float *prim_bounds, const nnbvh_placement *placements, int n_placements,
                                        const nnbvh_animated_transform *animated, int max_prims_in_node,
                                        int split_method, int device, bool alpha_textures);

// ... and the kd-tree scenes' (kd_trace.h) under the same name, for the code that serves both scene types
inline KdWorkspace *workspace_for(nnbvh_kd_scene *s, hipStream_t stream) { return kd_workspace_for(s, stream); }

// The prologue of a call on a scene of either type (S: nnbvh_scene with W = Workspace, nnbvh_kd_scene with W =
// KdWorkspace; `SceneCall call(s, stream)` deduces both): the scene's device made current and its lock held for the
// call, and with a stream that stream's workspace.
template <class S, class W = std::remove_pointer_t<decltype(workspace_for((S *)nullptr, hipStream_t()))>>
struct SceneCall {
    DeviceGuard guard;
    std::unique_lock<std::mutex> lock;
    W *w = nullptr;
    bool good;
    explicit SceneCall(S *s) : guard(s->device), good(guard.ok) {
        if (good) lock = std::unique_lock<std::mutex>(s->mu);
    }
    SceneCall(S *s, hipStream_t stream) : SceneCall(s) {
        if (good) good = (w = workspace_for(s, stream)) != nullptr;
    }
    bool ok() const { return good; }  // false: NNBVH_ERR_DEVICE, the error text is set
};

inline bool grow(void **ptr, size_t *have, size_t need, const char *what) {
    if (*have >= need) return true;
    if (*ptr) (void)hipFree(*ptr);
    *ptr = nullptr;
    *have = 0;
    if (!hip_ok(hipMalloc(ptr, need), what)) return false;
    *have = need;
    return true;
}

// both device arrays below 4 GiB (64 B per interior record, 16 B per primitive slot): the lean
// kernel instances reach them with 32-bit byte offsets.  The ONE predicate everything that depends on the offset width
// reads (scene_traits and through it is_lean / scene_runs_lean, the top table, the wavefront gather choice, p.fits32):
// the "offsets32" option can turn it off for a scene that fits, never on for one that does not
inline int scene_fits32(const nnbvh_scene *s) {
    return s->offsets32 && (int64_t)s->n_interior < (1LL << 26) && s->n_slots < (1LL << 28) - 8;
}

// what the choice of a kernel instance reads from a scene (trace_instance.h)
inline TraceTraits scene_traits(const nnbvh_scene *s) {
    return {s->window, s->instanced, !!s->d_anim, s->has_patches, s->has_alpha, s->has_host_prims, scene_fits32(s)};
}

// the lean kernel instances (bvh_trace.hip) have forms that read a wavefront queue's SOA slices themselves
inline bool scene_runs_lean(const nnbvh_scene *s) { return is_lean(scene_traits(s)); }

// ---- the launchers (capi_trace.cpp) ---------------------------------------------------------------------------
int grid_blocks(nnbvh_scene *s, int mode, int candidates = 0);

// One launch of the trace kernel over one batch of rays.
struct TraceJob {
    int mode = 0;                        // 0 closest hit, 1 any hit with exact counts, 2 any hit
    const void *rays = nullptr;          // nnbvh_ray records, or with rays == nullptr ...
    const nnbvh_ray_soa *soa = nullptr;  // ... a wavefront queue whose SOA slices the lean kernels read themselves
    int64_t n = 0;
    const int32_t *d_n = nullptr;        // nullable: device-resident batch size, clamped to [0, n]
    void *hits = nullptr;                // mode 0
    void *occluded = nullptr;            // modes 1 / 2
    void *visited = nullptr, *tests = nullptr;  // mode 1
    // modes 0 / 2, nullable: candidate mode.  The count (and, closest hit, before) arrays start at zero: the launcher
    // clears them with memset nodes unless hc_zeroed says the caller has done it.  Scenes with host-only primitives
    // then run the HOSTC instances, which fill them in; other scenes run the plain instances
    const nnbvh_host_candidates *hc = nullptr;
    bool hc_zeroed = false;
};
int launch(nnbvh_scene *s, Workspace *w, hipStream_t stream, const TraceJob &job);

// One launch of a walk instance of the trace kernel (bvh_trace.hip modes 4 / 5) behind its queue
// reset node (WalkJob: walk_math.h).  The caller has checked that the scene has walk instances (walk_refusal) and holds
// the scene's lock.
int launch_walk(nnbvh_scene *s, Workspace *w, hipStream_t stream, const WalkJob &job);
// why the scene has no walk instance (AnimatedPrimitive instances, alpha-tested primitives), or nullptr
const char *walk_refusal(const nnbvh_scene *s);

// ... over up to kMaxFusedBatches closest-hit / occlusion-only batches in one mode-3 launch, where batches_fusable
int launch_fused_batches(nnbvh_scene *s, Workspace *w, hipStream_t stream, const nnbvh_batch *batches, int n_batches,
                         const int32_t *const *d_n, const nnbvh_ray_soa *const *soas = nullptr,
                         const nnbvh_host_candidates *cands = nullptr);
bool batches_fusable(const nnbvh_scene *s, const nnbvh_batch *batches, int n_batches);

// candidates_fault (nnbvh_internal.h) reported as fn's
bool candidates_ok(const char *fn, const nnbvh_host_candidates *c, bool closest);
// the count (and, closest hit, before) arrays of a candidate call start at zero: kernel nodes on `stream`, of up to
// 8 blocks per CU of the scene's device
bool zero_candidates(int n_cus, const nnbvh_host_candidates *hc, int64_t n, bool closest, hipStream_t stream);

// The host-buffer form of a single-batch candidate call on a scene of either type: the rays and the candidate arrays
// staged in device memory of the call's own, one launch on the null stream, copies out (synchronous).  The caller has
// checked the arguments and n > 0.  launch_staged(workspace, d_rays, d_out, d) launches over the staged batch, whose
// candidates are d, and returns NNBVH_OK once the null stream's copies out may follow.
template <class S, class Launch>
int candidates_host(S *s, bool closest, const nnbvh_ray *rays, int64_t n, void *out, const nnbvh_host_candidates *c,
                    Launch launch_staged) {
    SceneCall<S> call(s);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    const size_t k = (size_t)c->capacity, out_elem = closest ? sizeof(nnbvh_hit) : 1;
    void *d_rays = nullptr, *d_out = nullptr;
    nnbvh_host_candidates d{};
    d.capacity = c->capacity;
    bool ok = hip_ok(hipMalloc(&d_rays, (size_t)n * sizeof(nnbvh_ray)), "hipMalloc(rays)") &&
              hip_ok(hipMalloc(&d_out, (size_t)n * out_elem), "hipMalloc(results)") &&
              hip_ok(hipMalloc((void **)&d.count, (size_t)n * 4), "hipMalloc(count)") &&
              (!closest || hip_ok(hipMalloc((void **)&d.before, (size_t)n * 4), "hipMalloc(before)")) &&
              hip_ok(hipMalloc((void **)&d.prim, (size_t)n * k * 4), "hipMalloc(prim)") &&
              hip_ok(hipMalloc((void **)&d.instance, (size_t)n * k * 4), "hipMalloc(instance)") &&
              hip_ok(hipMemcpy(d_rays, rays, (size_t)n * sizeof(nnbvh_ray), hipMemcpyHostToDevice), "copy rays") &&
              // the caller's entries beyond count stay as they were: start from them
              hip_ok(hipMemcpy(d.prim, c->prim, (size_t)n * k * 4, hipMemcpyHostToDevice), "copy prim") &&
              hip_ok(hipMemcpy(d.instance, c->instance, (size_t)n * k * 4, hipMemcpyHostToDevice), "copy instance");
    auto *w = ok ? workspace_for(s, nullptr) : nullptr;
    int rc = w ? launch_staged(w, d_rays, d_out, d) : NNBVH_ERR_DEVICE;
    if (rc == NNBVH_OK &&
        !(hip_ok(hipMemcpy(out, d_out, (size_t)n * out_elem, hipMemcpyDeviceToHost), "copy results") &&
          hip_ok(hipMemcpy(c->count, d.count, (size_t)n * 4, hipMemcpyDeviceToHost), "copy count") &&
          (!closest || hip_ok(hipMemcpy(c->before, d.before, (size_t)n * 4, hipMemcpyDeviceToHost), "copy before")) &&
          hip_ok(hipMemcpy(c->prim, d.prim, (size_t)n * k * 4, hipMemcpyDeviceToHost), "copy prim") &&
          hip_ok(hipMemcpy(c->instance, d.instance, (size_t)n * k * 4, hipMemcpyDeviceToHost), "copy instance")))
        rc = NNBVH_ERR_DEVICE;
    for (void *q : {d_rays, d_out, (void *)d.count, (void *)d.before, (void *)d.prim, (void *)d.instance})
        if (q) (void)hipFree(q);
    return rc;
}

}  // namespace nnbvh
