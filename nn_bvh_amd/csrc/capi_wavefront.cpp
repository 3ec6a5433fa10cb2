// capi_wavefront.cpp — the C ABI of include/nnbvh.h, wavefront queues (wavefront/aggregate.cpp:34-116 on the
// device): IntersectClosest, IntersectShadow and the two in one launch, each with or without the work items and
// the host candidates, and the multi-pass IntersectShadowTr / IntersectOneRandom; the first three also for kd-tree
// scenes (kd_trace.h), host candidates included, over the same argument packs, checks and queue kernels.  Host code
// only.
#include <algorithm>
#include <cstring>

#include "capi_internal.h"
#include "kd_trace.h"
#include "wavefront.h"
#include "wavefront2.h"
#include "wavefront_items.h"

using namespace nnbvh;

static bool fail(const char *fn, const char *why) {
    set_error(std::string(fn) + ": " + why);
    return false;
}

static bool soa_ok(const nnbvh_ray_soa *q) {
    return q && q->ox && q->oy && q->oz && q->dx && q->dy && q->dz;
}

static bool queues_ok(const nnbvh_closest_queues *out) {
    const nnbvh_work_queue *qs[6] = {&out->escaped, &out->hit_area_light, &out->basic_eval_material,
                                     &out->universal_eval_material, &out->medium_sample, &out->next_ray};
    for (const nnbvh_work_queue *q : qs)
        if (q->size && (q->capacity < 0 || (q->capacity > 0 && !q->items))) return false;
    return true;
}

// ---- IntersectClosest with the work items (wavefront/intersect.h:16-156) --------------------------------
static_assert(sizeof(nnbvh_item_slices) == 48 * sizeof(void *), "nnbvh_item_slices: 48 pointers");

// every non-null slice must be one its queue's Push stores (include/nnbvh.h), and a wanted needs_host
// queue needs storage like the others
static bool items_ok(const nnbvh_closest_items *items, const char **why) {
    enum { kPrim = 1, kPi = 2, kP = 4, kN = 8, kGeo = 16, kWo = 32, kUv = 64, kFace = 128, kTime = 256, kTMax = 512, kRay = 1024 };
    struct Field {
        size_t offset, count;
        unsigned kind;
    };
#define F(name, kind) {offsetof(nnbvh_item_slices, name), sizeof(((nnbvh_item_slices *)0)->name) / sizeof(void *), kind}
    static const Field fields[] = {F(prim, kPrim), F(pi, kPi), F(p, kP), F(n, kN), F(ns, kGeo), F(dpdu, kGeo),
                                   F(dpdv, kGeo), F(dpdus, kGeo), F(dpdvs, kGeo), F(dndus, kGeo), F(dndvs, kGeo),
                                   F(wo, kWo), F(uv, kUv), F(face_index, kFace), F(time, kTime), F(t_max, kTMax),
                                   F(ray_o, kRay), F(ray_d, kRay)};
#undef F
    const unsigned material = kPrim | kPi | kN | kGeo | kWo | kUv | kFace | kTime;
    const struct {
        const nnbvh_item_slices *s;
        unsigned allowed;
        const char *name;
    } queues[5] = {{&items->hit_area_light, kPrim | kP | kN | kWo | kUv, "hit_area_light"},
                   {&items->basic_eval_material, material, "basic_eval_material"},
                   {&items->universal_eval_material, material, "universal_eval_material"},
                   {&items->medium_sample, material | kTMax, "medium_sample"},
                   {&items->next_ray, kPrim | kRay | kTime, "next_ray"}};
    for (const auto &q : queues) {
        const char *base = (const char *)q.s;
        for (const Field &f : fields) {
            if (q.allowed & f.kind) continue;
            for (size_t k = 0; k < f.count; ++k)
                if (((void *const *)(base + f.offset))[k]) {
                    *why = q.name;
                    return false;
                }
        }
    }
    const nnbvh_work_queue &h = items->needs_host;
    if (h.size && (h.capacity < 0 || (h.capacity > 0 && !h.items))) {
        *why = "needs_host";
        return false;
    }
    return true;
}

// The closest side of a call (IntersectClosest) in its three forms: plain; with_items: the work items come with
// the index queues, computed from a shading mesh (d_hits may be NULL: the records then stay in a workspace);
// with_candidates, an _items form: host-only primitives are listed in hc instead of voiding the ray (d_hits required).
struct ClosestSide {
    int32_t max_rays;
    const nnbvh_ray_soa *queue;
    const int32_t *d_size;
    const uint8_t *d_prim_class;
    int64_t n_prim_class;
    void *d_hits;
    const nnbvh_closest_queues *out;
    bool with_items = false;
    const nnbvh_shading_mesh *mesh = nullptr;
    const nnbvh_closest_items *items = nullptr;
    bool with_candidates = false;
    const nnbvh_host_candidates *hc = nullptr;
    bool kd = false;  // called through a nnbvh_kd_wavefront_* entry point
};

// The shadow side (IntersectShadow), plain (d_occluded may be NULL: a workspace then holds the flags) or
// with_candidates (d_occluded required: 0 / 1 / 2 per ray).
struct ShadowSide {
    int32_t max_rays;
    const nnbvh_ray_soa *queue;
    const int32_t *d_size;
    const float *d_Ld, *d_r_u, *d_r_l;
    const int32_t *d_pixel_index;
    float *d_L;
    int64_t n_pixels;
    uint8_t *d_occluded;
    bool with_candidates = false;
    const nnbvh_host_candidates *hc = nullptr;
    bool kd = false;
};

// the entry point a side, or the pair, was called through: error texts carry its name
static const char *closest_fn(const ClosestSide &a) {
    if (a.kd)
        return a.with_candidates ? "kd_wavefront_intersect_closest_items_candidates"
                                 : a.with_items ? "kd_wavefront_intersect_closest_items" : "kd_wavefront_intersect_closest";
    return a.with_candidates ? "wavefront_intersect_closest_items_candidates"
                             : a.with_items ? "wavefront_intersect_closest_items" : "wavefront_intersect_closest";
}
static const char *shadow_fn(const ShadowSide &a) {
    if (a.kd) return a.with_candidates ? "kd_wavefront_intersect_shadow_candidates" : "kd_wavefront_intersect_shadow";
    return a.with_candidates ? "wavefront_intersect_shadow_candidates" : "wavefront_intersect_shadow";
}
static const char *pair_fn(const ClosestSide &a) {
    if (a.kd)
        return a.with_candidates ? "kd_wavefront_intersect_closest_and_shadow_items_candidates"
                                 : a.with_items ? "kd_wavefront_intersect_closest_and_shadow_items"
                                                : "kd_wavefront_intersect_closest_and_shadow";
    return a.with_candidates ? "wavefront_intersect_closest_and_shadow_items_candidates"
                             : a.with_items ? "wavefront_intersect_closest_and_shadow_items"
                                            : "wavefront_intersect_closest_and_shadow";
}

// the closest side without the scene and the hit records (the enqueue-only calls have neither rule)
static bool queue_args_ok(const char *fn, const ClosestSide &a) {
    if (a.max_rays < 0 || !a.out || a.n_prim_class < 0 || (a.max_rays > 0 && !soa_ok(a.queue)) ||
        (a.with_items && (!a.mesh || !a.items)))
        return fail(fn, "bad argument");
    if (!queues_ok(a.out)) return fail(fn, "queue with a size counter but no item storage");
    const char *why = nullptr;
    if (a.with_items && !items_ok(a.items, &why)) {
        set_error(std::string(fn) + ": slice not carried by queue " + why + ", or needs_host without storage");
        return false;
    }
    return true;
}

// (S: the scene of either type, nnbvh_scene or nnbvh_kd_scene)
template <class S>
static bool closest_args_ok(const char *fn, const S *s, const ClosestSide &a) {
    const bool no_hits = a.max_rays > 0 && !a.d_hits;
    if (a.with_candidates && (!s || no_hits)) return fail(fn, "bad argument (scene and d_hits are required)");
    if (!s || (!a.with_items && no_hits)) return fail(fn, "bad argument");
    if (!queue_args_ok(fn, a) || (a.with_candidates && !candidates_ok(fn, a.hc, true))) return false;
    if (a.with_items && s->device != a.mesh->device) return fail(fn, "scene and shading mesh live on different devices");
    return true;
}

template <class S>
static bool shadow_args_ok(const char *fn, const S *s, const ShadowSide &a) {
    if (!s) return fail(fn, "bad argument");
    if (a.max_rays < 0 || a.n_pixels < 0 ||
        (a.max_rays > 0 && (!soa_ok(a.queue) || !a.d_Ld || !a.d_r_u || !a.d_r_l || !a.d_pixel_index || !a.d_L ||
                            (a.with_candidates && !a.d_occluded))))
        return fail(fn, a.with_candidates ? "bad argument (d_occluded is required)" : "bad argument");
    return !a.with_candidates || candidates_ok(fn, a.hc, false);
}

// d_hits == NULL: the records go to a per-stream workspace of the scene's; d_occluded == NULL: likewise
// (W: the BVH scenes' Workspace or the kd scenes' KdWorkspace)
template <class W>
static void *hits_storage(W *w, void *d_hits, int32_t max_rays) {
    if (d_hits) return d_hits;
    if (!grow(&w->d_hits, &w->hits_bytes, (size_t)max_rays * sizeof(nnbvh_hit), "hipMalloc(wavefront hits)"))
        return nullptr;
    return w->d_hits;
}
template <class W>
static uint8_t *occluded_storage(W *w, uint8_t *d_occluded, int32_t max_rays) {
    if (d_occluded) return d_occluded;
    if (!grow(&w->d_out, &w->out_bytes, (size_t)max_rays, "hipMalloc(wavefront occluded)")) return nullptr;
    return (uint8_t *)w->d_out;
}

// The trace half of a queue call, per scene type: one queue through the trace kernel, closest hit (out = nnbvh_hit[n]) or
// any hit (out = uint8[n]), hc nullable.  The caller holds the scene's lock.
// BVH scenes: the lean kernels read the queue's SOA slices themselves (no gather pass into nnbvh_ray records); for the
// others it is gathered into the workspace.  Candidates start from zero; scenes without host-only primitives run the
// plain kernels over them.
static int trace_queue(nnbvh_scene *s, Workspace *w, hipStream_t stream, bool any, const nnbvh_ray_soa *queue, int32_t n,
                       const int32_t *d_n, void *out, const nnbvh_host_candidates *hc) {
    TraceJob job{.mode = any ? 2 : 0, .soa = queue, .n = n, .d_n = d_n, .hits = any ? nullptr : out,
                 .occluded = any ? out : nullptr, .hc = hc, .hc_zeroed = true};
    if (hc && !zero_candidates(s->n_cus, hc, n, !any, stream)) return NNBVH_ERR_DEVICE;
    if (!scene_runs_lean(s)) {
        if (!grow(&w->d_in, &w->in_bytes, (size_t)n * sizeof(nnbvh_ray), "hipMalloc(wavefront rays)"))
            return NNBVH_ERR_DEVICE;
        if (!hip_ok(launch_wf_gather(*queue, WavefrontCount{n, d_n}, w->d_in, s->n_cus * 8, stream), "gather kernel launch"))
            return NNBVH_ERR_DEVICE;
        job.rays = w->d_in;
        job.soa = nullptr;
    }
    return launch(s, w, stream, job);
}
// kd-tree scenes: kd_trace.hip's batch-mode launch over the one batch (kd_launch_batches gathers, zeroes and picks the
// candidate-mode instances)
static int trace_queue(nnbvh_kd_scene *s, KdWorkspace *w, hipStream_t stream, bool any, const nnbvh_ray_soa *queue,
                       int32_t n, const int32_t *d_n, void *out, const nnbvh_host_candidates *hc) {
    KdBatch batch;
    batch.any = any, batch.soa = queue, batch.n = n, batch.d_n = d_n, batch.out = out, batch.hc = hc;
    return kd_launch_batches(s, w, stream, &batch, 1);
}

// IntersectShadow of one depth and IntersectClosest of the next (wavefront/integrator.cpp: TraceShadowRays(depth),
// then the next iteration's IntersectClosest): both queues are filled by the shading of the same depth and neither
// reads what the other writes, so they can share ONE launch (mode 3: one ramp-up and one drain instead of two).
// The trace half of that form (the caller has checked that the scene allows it and holds its lock).  cands: null, or
// the candidates of the closest and of the shadow side.
static int trace_two_queues(nnbvh_scene *s, Workspace *w, hipStream_t stream, const ClosestSide &c, void *hits,
                            const ShadowSide &sh, uint8_t *occ, const nnbvh_host_candidates *cands) {
    if (cands && !s->has_host_prims) {  // the plain kernels over zeroed arrays; every count stays zero
        if (!zero_candidates(s->n_cus, &cands[0], c.max_rays, true, stream) ||
            !zero_candidates(s->n_cus, &cands[1], sh.max_rays, false, stream))
            return NNBVH_ERR_DEVICE;
        cands = nullptr;
    }
    // the (longer) closest-hit batch first: the shadow rays fill the lanes its tail leaves idle
    nnbvh_batch batches[2] = {{NNBVH_BATCH_CLOSEST, 0, nullptr, c.max_rays, hits, nullptr, nullptr},
                              {NNBVH_BATCH_ANY, 0, nullptr, sh.max_rays, occ, nullptr, nullptr}};
    const int32_t *sizes[2] = {c.d_size, sh.d_size};
    const nnbvh_ray_soa *soas[2] = {c.queue, sh.queue};
    if (scene_runs_lean(s))  // both queues are read as the SOA slices they are
        return launch_fused_batches(s, w, stream, batches, 2, sizes, soas);
    const size_t closest_bytes = (size_t)c.max_rays * sizeof(nnbvh_ray);
    if (!grow(&w->d_in, &w->in_bytes, closest_bytes + (size_t)sh.max_rays * sizeof(nnbvh_ray),
              "hipMalloc(wavefront rays)"))
        return NNBVH_ERR_DEVICE;
    void *closest_rays = w->d_in, *shadow_rays = (char *)w->d_in + closest_bytes;
    if (!hip_ok(launch_wf_gather(*c.queue, WavefrontCount{c.max_rays, c.d_size}, closest_rays, s->n_cus * 8, stream),
                "gather kernel launch") ||
        !hip_ok(launch_wf_gather(*sh.queue, WavefrontCount{sh.max_rays, sh.d_size}, shadow_rays, s->n_cus * 8, stream),
                "gather kernel launch"))
        return NNBVH_ERR_DEVICE;
    batches[0].d_rays = closest_rays;
    batches[1].d_rays = shadow_rays;
    return launch_fused_batches(s, w, stream, batches, 2, sizes, nullptr, cands);
}

// IntersectClosest's enqueue with the work items (wavefront/intersect.h:16-156).  hc_count (nullable): a ray with
// count != 0 is the caller's, whatever its record says
static int launch_items(const ClosestSide &a, const void *hits, const int32_t *hc_count, hipStream_t stream) {
    if (!hip_ok(launch_wf_enqueue_closest_items(a.mesh->d, hits, WavefrontCount{a.max_rays, a.d_size}, *a.queue,
                                                a.d_prim_class, (long)a.n_prim_class, *a.out, *a.items,
                                                a.mesh->n_cus * 8, stream, hc_count, nullptr, a.max_rays),
                "work-item enqueue kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

// the second half of each side: hit records -> index queues (and work items), occlusion flags -> L
template <class S>
static int enqueue_closest(const S *s, const ClosestSide &a, const void *hits, hipStream_t stream) {
    if (a.with_items)
        return launch_items(a, hits, a.with_candidates && s->has_host_prims ? a.hc->count : nullptr, stream);
    if (!hip_ok(launch_wf_enqueue_closest(hits, WavefrontCount{a.max_rays, a.d_size}, a.queue->has_medium,
                                          a.d_prim_class, (long)a.n_prim_class, *a.out, s->n_cus * 8, stream),
                "enqueue kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}
template <class S>
static int record_shadow(const S *s, const ShadowSide &a, const uint8_t *occ, hipStream_t stream) {
    if (!hip_ok(launch_wf_record_shadow(occ, WavefrontCount{a.max_rays, a.d_size}, a.d_Ld, a.d_r_u, a.d_r_l,
                                        a.d_pixel_index, a.d_L, (long)a.n_pixels, s->n_cus * 8, stream),
                "shadow record kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

// What a kd-tree scene checks first, before the scene is looked at (the side checks read its device): a batch-mode
// launch tags a ray with batch << kKdIndexBits | index, and a candidate call's nnbvh_host_candidates
static bool kd_size_ok(const char *fn, int32_t max_rays) {
    if (max_rays < 0) return fail(fn, "bad argument");
    return max_rays < (1 << kKdIndexBits) || fail(fn, "a queue of 2^28 rays or more");
}
static bool kd_candidates_ok(const char *fn, bool scene, bool with_candidates, const nnbvh_host_candidates *hc, bool closest) {
    if (!with_candidates) return true;
    return scene ? candidates_ok(fn, hc, closest) : fail(fn, "bad argument (a scene is required)");
}
static bool front_ok(const char *fn, const nnbvh_kd_scene *s, int32_t max_rays, bool with_candidates,
                     const nnbvh_host_candidates *hc, bool closest) {
    return kd_size_ok(fn, max_rays) && kd_candidates_ok(fn, s != nullptr, with_candidates, hc, closest);
}
static bool front_ok(const char *, const nnbvh_scene *, int32_t, bool, const nnbvh_host_candidates *, bool) { return true; }

// IntersectClosest / IntersectShadow on a scene of either type: the argument packs, their checks and the queue kernels
// behind the launch are the same; the trace half is the type's trace_queue.  Without candidates a host-only primitive
// voids the ray, and the enqueue sends it to needs_host (or nowhere); with them (the *_candidates calls) the enqueue
// routes by the per-ray count and the shadow record skips the non-zero flags.
template <class S>
static int intersect_closest(S *s, const ClosestSide &a, hipStream_t stream) {
    const char *fn = closest_fn(a);
    if (!front_ok(fn, s, a.max_rays, a.with_candidates, a.hc, true) || !closest_args_ok(fn, s, a)) return NNBVH_ERR_ARG;
    if (a.max_rays == 0) return NNBVH_OK;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    void *hits = hits_storage(call.w, a.d_hits, a.max_rays);
    if (!hits) return NNBVH_ERR_DEVICE;
    const int rc = trace_queue(s, call.w, stream, false, a.queue, a.max_rays, a.d_size, hits, a.hc);
    return rc != NNBVH_OK ? rc : enqueue_closest(s, a, hits, stream);
}

template <class S>
static int intersect_shadow(S *s, const ShadowSide &a, hipStream_t stream) {
    const char *fn = shadow_fn(a);
    if (!front_ok(fn, s, a.max_rays, a.with_candidates, a.hc, false) || !shadow_args_ok(fn, s, a)) return NNBVH_ERR_ARG;
    if (a.max_rays == 0) return NNBVH_OK;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    uint8_t *occ = occluded_storage(call.w, a.d_occluded, a.max_rays);
    if (!occ) return NNBVH_ERR_DEVICE;
    const int rc = trace_queue(s, call.w, stream, true, a.queue, a.max_rays, a.d_size, occ, a.hc);
    return rc != NNBVH_OK ? rc : record_shadow(s, a, occ, stream);
}

// The pair call stays one function per scene type: the two check their arguments in deliberately different orders (a
// BVH scene checks a side under the pair's name only for _items, candidates or the one launch; a kd-tree scene checks
// everything up front), and their one-launch halves share nothing.
// Both sides in one launch where the scene and the sizes allow it; both sides have candidates, or neither.
static int intersect_closest_and_shadow(nnbvh_scene *s, const ClosestSide &c, const ShadowSide &sh,
                                        hipStream_t stream) {
    const char *fn = pair_fn(c);
    const nnbvh_batch probe[2] = {{NNBVH_BATCH_CLOSEST, 0, nullptr, c.max_rays, nullptr, nullptr, nullptr},
                                  {NNBVH_BATCH_ANY, 0, nullptr, sh.max_rays, nullptr, nullptr, nullptr}};
    const bool one_launch = s && c.max_rays > 0 && sh.max_rays > 0 && batches_fusable(s, probe, 2);
    // Under the pair's own name: the closest side of the _items forms, and with candidates everything, checked before
    // anything is launched, so that a bad argument leaves both sides untouched.  The rest is the one launch's to check:
    // the two calls check their own.
    if ((c.with_items || one_launch) && !closest_args_ok(fn, s, c)) return NNBVH_ERR_ARG;
    if ((sh.with_candidates || one_launch) && !shadow_args_ok(fn, s, sh)) return NNBVH_ERR_ARG;
    if (!one_launch) {
        // a scene or sizes the one-launch form does not cover, or one side empty: the two calls one after the other
        const int rc = intersect_shadow(s, sh, stream);
        return rc != NNBVH_OK ? rc : intersect_closest(s, c, stream);
    }
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    uint8_t *occ = occluded_storage(call.w, sh.d_occluded, sh.max_rays);
    void *hits = occ ? hits_storage(call.w, c.d_hits, c.max_rays) : nullptr;
    if (!hits) return NNBVH_ERR_DEVICE;
    const nnbvh_host_candidates cands[2] = {c.with_candidates ? *c.hc : nnbvh_host_candidates{},
                                            sh.with_candidates ? *sh.hc : nnbvh_host_candidates{}};
    int rc = trace_two_queues(s, call.w, stream, c, hits, sh, occ, c.with_candidates ? cands : nullptr);
    if (rc == NNBVH_OK) rc = enqueue_closest(s, c, hits, stream);
    if (rc == NNBVH_OK) rc = record_shadow(s, sh, occ, stream);
    return rc;
}

// Both sides checked under the pair's name before anything is launched; one side empty (or the scene set to two
// launches, "pair_one_launch" 0): the two calls one after the other.  The one launch is kd_trace.hip's batch-mode
// launch over both queues.
static int kd_intersect_closest_and_shadow(nnbvh_kd_scene *s, const ClosestSide &c, const ShadowSide &sh,
                                           hipStream_t stream) {
    const char *fn = pair_fn(c);
    if (!kd_size_ok(fn, c.max_rays) || !kd_size_ok(fn, sh.max_rays) ||
        !kd_candidates_ok(fn, s != nullptr, c.with_candidates, c.hc, true) ||
        !kd_candidates_ok(fn, s != nullptr, sh.with_candidates, sh.hc, false) ||
        !closest_args_ok(fn, s, c) || !shadow_args_ok(fn, s, sh))
        return NNBVH_ERR_ARG;
    if (c.max_rays == 0 || sh.max_rays == 0 || !s->pair_one_launch) {
        const int rc = intersect_shadow(s, sh, stream);
        return rc != NNBVH_OK ? rc : intersect_closest(s, c, stream);
    }
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    uint8_t *occ = occluded_storage(call.w, sh.d_occluded, sh.max_rays);
    void *hits = occ ? hits_storage(call.w, c.d_hits, c.max_rays) : nullptr;
    if (!hits) return NNBVH_ERR_DEVICE;
    // closest-hit batch first, the order of the BVH pair call (tools/kd_wavefront_probe.py times both orders of the
    // flat batches)
    KdBatch batches[2];
    batches[0].soa = c.queue, batches[0].n = c.max_rays, batches[0].d_n = c.d_size, batches[0].out = hits;
    batches[1].any = 1, batches[1].soa = sh.queue, batches[1].n = sh.max_rays, batches[1].d_n = sh.d_size,
    batches[1].out = occ;
    batches[0].hc = c.with_candidates ? c.hc : nullptr;
    batches[1].hc = sh.with_candidates ? sh.hc : nullptr;
    int rc = kd_launch_batches(s, call.w, stream, batches, 2);
    if (rc == NNBVH_OK) rc = enqueue_closest(s, c, hits, stream);
    if (rc == NNBVH_OK) rc = record_shadow(s, sh, occ, stream);
    return rc;
}

// ---- what the multi-pass and the walk calls below share (C++ linkage: templates) ---------------------------------
static bool scratch(Workspace *w, int slot, size_t bytes, void **out) {
    if (!grow(&w->scratch[slot], &w->scratch_bytes[slot], std::max<size_t>(bytes, 16), "hipMalloc(wavefront scratch)"))
        return false;
    *out = w->scratch[slot];
    return true;
}

static bool read_count(const int32_t *d_counter, hipStream_t stream, int *out) {
    int32_t v = 0;
    if (!hip_ok(hipMemcpyAsync(&v, d_counter, 4, hipMemcpyDeviceToHost, stream), "read pass count") ||
        !hip_ok(hipStreamSynchronize(stream), "wavefront pass"))
        return false;
    *out = v;
    return true;
}

static constexpr int kMaxBoundedPasses = 64;
static constexpr int kMaxWalkSurfaces = 65536;

// What a scene type refuses in a walk call on top of the common checks below: `early` between "negative size" and
// "null array", else last
static const char *type_refusal(const nnbvh_scene *s, const nnbvh_shading_mesh *, int32_t, bool early) {
    return early ? nullptr : walk_refusal(s);
}
static const char *type_refusal(const nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_items, bool early) {
    if (early) return max_items >= (1 << kKdIndexBits) ? "a queue of 2^28 items or more" : nullptr;
    if (m->d.instances) return "the shading mesh carries an instance table (kd-tree scenes have one level)";
    if (s->d_extras)
        return "the scene holds alpha-tested smooth triangles or alpha-tested patches on the device (the ATTR kernels), "
               "which have no walk instances";
    return nullptr;
}

// The arguments of a bounded call (bound_name "max_passes", 1..kMaxBoundedPasses) or of a walk call of either scene
// type ("max_surfaces", 1..kMaxWalkSurfaces; refuse = type_refusal).  arrays: every array the call needs is there
template <class S>
static bool bounded_args_ok(const char *fn, const S *s, const nnbvh_shading_mesh *m, int32_t max_items, int64_t n_prim,
                            const char *bound_name, int32_t bound, int32_t bound_max, bool arrays,
                            const char *(*refuse)(const S *, const nnbvh_shading_mesh *, int32_t, bool) = nullptr) {
    std::string what;
    const char *refusal = nullptr;
    if (!s) what = "no scene";
    else if (!m) what = "no shading mesh";
    else if (bound < 1 || bound > bound_max) what = std::string(bound_name) + " outside 1.." + std::to_string(bound_max);
    else if (max_items < 0 || n_prim < 0) what = "negative size";
    else if (refuse && (refusal = refuse(s, m, max_items, true))) what = refusal;
    else if (max_items > 0 && !arrays) what = "null array";
    else if (m->device != s->device) what = "scene and shading mesh live on different devices";
    else if (refuse && (refusal = refuse(s, m, max_items, false))) what = refusal;
    if (!what.empty()) set_error(std::string(fn) + ": " + what);
    return what.empty();
}

// ---- the pass calls: one loop per walk, two drivers -----------------------------------------------------------------
// A pass is the trace of the current list and ONE fused step (wavefront2.hip), which appends the items that go on to
// the next list and counts them.
// Bounded driver (max_passes 1..kMaxBoundedPasses): every pass is enqueued up front, sized for the queue, and takes its
// live count from count[k], which the step of pass k - 1 has counted up; the counters are cleared by one kernel node,
// and what is left on the last list is marked unfinished.  Nothing inside waits for the device or copies from host
// memory, so the call can be captured in a hipGraph once the stream's workspace has its size (a warm-up call with the
// same queue capacity).  A pass over an empty list is a trace and a step whose waves exit at once.
// Host-driven driver (max_passes == kUnbounded): after each step the host reads the next list's count, stops at zero
// and sizes the next pass's grids by it; two counter words alternate, each cleared before it is appended to.
static constexpr int kUnbounded = 0;

// the counter that pass `pass` appends to; nullptr: the launch that clears it failed
static int32_t *next_count(int32_t *count, int pass, bool bounded, int max_blocks, hipStream_t stream) {
    if (bounded) return count + pass + 1;
    int32_t *c = count + ((pass + 1) & 1);
    return hip_ok(launch_zero_words(c, 1, max_blocks, stream), "pass count reset launch") ? c : nullptr;
}

// The caller has checked the arguments, holds the scene's lock, has cleared *d_unfinished and max_rays > 0.
static int shadow_tr_passes(nnbvh_scene *s, Workspace *w, const nnbvh_shading_mesh *m, int32_t max_rays,
                            const nnbvh_ray_soa *shadow_queue, const int32_t *d_size, const uint8_t *d_prim_class,
                            int64_t n_prim_class, const float *d_Ld, const float *d_r_u, const float *d_r_l,
                            const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_state,
                            int32_t max_passes, int32_t *d_unfinished, hipStream_t stream) {
    const bool bounded = max_passes != kUnbounded;
    const size_t n = (size_t)max_rays;
    const int max_blocks = s->n_cus * 8;
    void *cur, *next, *hits, *ocur, *onext, *pLight, *state, *counters;
    if (!scratch(w, Workspace::kRaysA, n * 32, &cur) || !scratch(w, Workspace::kRaysB, n * 32, &next) ||
        !scratch(w, Workspace::kHits, n * 32, &hits) || !scratch(w, Workspace::kOrigA, n * 4, &ocur) ||
        !scratch(w, Workspace::kOrigB, n * 4, &onext) || !scratch(w, Workspace::kPLight, n * 16, &pLight) ||
        !scratch(w, Workspace::kState, n, &state) ||
        !scratch(w, Workspace::kCounters, (kMaxBoundedPasses + 1) * 4, &counters))
        return NNBVH_ERR_DEVICE;
    int32_t *count = (int32_t *)counters;  // bounded: count[k] is the size of pass k's list, k >= 1
    const WavefrontCount cnt{max_rays, d_size};
    if (bounded && !hip_ok(launch_zero_words(count, max_passes + 1, max_blocks, stream), "pass count reset launch"))
        return NNBVH_ERR_DEVICE;
    if (!hip_ok(launch_str_init(*shadow_queue, cnt, cur, (int32_t *)ocur, (float4 *)pLight, (uint8_t *)state, max_blocks,
                                stream), "shadow-tr init launch"))
        return NNBVH_ERR_DEVICE;
    const int32_t *d_n = d_size;  // pass 0 runs the queue itself: max_rays clamped by *d_size
    int active = max_rays;
    for (int pass = 0; bounded ? pass < max_passes : active > 0; ++pass) {
        if (!bounded && pass > 4096) {
            set_error("wavefront_intersect_shadow_tr: more than 4096 interface surfaces on one shadow ray");
            return NNBVH_ERR_ARG;
        }
        int32_t *d_next = next_count(count, pass, bounded, max_blocks, stream);
        if (!d_next) return NNBVH_ERR_DEVICE;
        int rc = launch(s, w, stream, {.mode = 0, .rays = cur, .n = active, .d_n = d_n, .hits = hits});
        if (rc != NNBVH_OK) return rc;
        if (!hip_ok(launch_str_step(m->d, cur, hits, (const int32_t *)ocur, WavefrontCount{active, d_n}, d_prim_class,
                                    (long)n_prim_class, (const float4 *)pLight, (uint8_t *)state, next,
                                    (int32_t *)onext, d_next, max_blocks, stream), "shadow-tr step launch"))
            return NNBVH_ERR_DEVICE;
        if (!bounded && !read_count(d_next, stream, &active)) return NNBVH_ERR_DEVICE;
        std::swap(cur, next);
        std::swap(ocur, onext);
        d_n = d_next;
    }
    if (bounded && !hip_ok(launch_w2_mark_unfinished(cur, (const int32_t *)ocur, WavefrontCount{max_rays, d_n},
                                                     (uint8_t *)state, nullptr, d_unfinished, max_blocks, stream),
                           "shadow-tr marking launch"))
        return NNBVH_ERR_DEVICE;
    if (!hip_ok(launch_str_record((const uint8_t *)state, cnt, d_Ld, d_r_u, d_r_l, d_pixel_index, d_L, (long)n_pixels,
                                  d_state, max_blocks, stream), "shadow-tr record launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

// The caller has checked the arguments, holds the scene's lock, has cleared *d_unfinished and max_items > 0.
static int one_random_passes(nnbvh_scene *s, Workspace *w, const nnbvh_shading_mesh *m, int32_t max_items,
                             const float *d_p0, const float *d_p1, const int32_t *d_material, const int32_t *d_size,
                             const int32_t *d_prim_material, int64_t n_prim_material, void *d_sel_hits,
                             void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum, int32_t max_passes,
                             int32_t *d_unfinished, hipStream_t stream) {
    const bool bounded = max_passes != kUnbounded;
    const size_t n = (size_t)max_items;
    const int max_blocks = s->n_cus * 8;
    void *cur, *next, *hits, *ocur, *onext, *rng, *weights, *counters;
    if (!scratch(w, Workspace::kRaysA, n * 32, &cur) || !scratch(w, Workspace::kRaysB, n * 32, &next) ||
        !scratch(w, Workspace::kHits, n * 32, &hits) || !scratch(w, Workspace::kOrigA, n * 4, &ocur) ||
        !scratch(w, Workspace::kOrigB, n * 4, &onext) || !scratch(w, Workspace::kRng, n * 16, &rng) ||
        !scratch(w, Workspace::kWeights, n * 8, &weights) ||
        !scratch(w, Workspace::kCounters, (kMaxBoundedPasses + 1) * 4, &counters))
        return NNBVH_ERR_DEVICE;
    int32_t *count = (int32_t *)counters;  // bounded: count[k] is the size of pass k's list
    OneRandomState st{nullptr, (uint64_t *)rng, (float *)weights};
    const WavefrontCount cnt{max_items, d_size};
    if (!hip_ok(launch_zero_words(count, bounded ? max_passes + 1 : 1, max_blocks, stream), "pass count reset launch") ||
        !hip_ok(launch_or_init(d_p0, d_p1, cnt, st, cur, (int32_t *)ocur, count, d_sel_hits, d_sel_rays, max_blocks,
                               stream), "one-random init launch"))
        return NNBVH_ERR_DEVICE;
    const int32_t *d_n = count;  // pass 0 runs the items whose first direction is not zero
    int active = max_items;
    if (!bounded && !read_count(d_n, stream, &active)) return NNBVH_ERR_DEVICE;
    for (int pass = 0; bounded ? pass < max_passes : active > 0; ++pass) {
        if (!bounded && pass > 65536) {
            set_error("wavefront_intersect_one_random: more than 65536 surfaces on one segment");
            return NNBVH_ERR_ARG;
        }
        int32_t *d_next = next_count(count, pass, bounded, max_blocks, stream);
        if (!d_next) return NNBVH_ERR_DEVICE;
        int rc = launch(s, w, stream, {.mode = 0, .rays = cur, .n = active, .d_n = d_n, .hits = hits});
        if (rc != NNBVH_OK) return rc;
        if (!hip_ok(launch_or_step_fused(m->d, cur, hits, (const int32_t *)ocur, WavefrontCount{active, d_n}, d_p1,
                                         d_material, d_prim_material, (long)n_prim_material, st, next,
                                         (int32_t *)onext, d_next, d_sel_hits, d_sel_rays, max_blocks, stream),
                    "one-random step launch"))
            return NNBVH_ERR_DEVICE;
        if (!bounded && !read_count(d_next, stream, &active)) return NNBVH_ERR_DEVICE;
        std::swap(cur, next);
        std::swap(ocur, onext);
        d_n = d_next;
    }
    if (bounded && !hip_ok(launch_w2_mark_unfinished(cur, (const int32_t *)ocur, WavefrontCount{max_items, d_n}, nullptr,
                                                     d_sel_hits, d_unfinished, max_blocks, stream),
                           "one-random marking launch"))
        return NNBVH_ERR_DEVICE;
    if (!hip_ok(launch_or_finish(cnt, st, d_reservoir_pdf, d_weight_sum, max_blocks, stream), "one-random finish launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

// ---- the walk calls: IntersectShadowTr / IntersectOneRandom inside ONE trace launch, for scenes of either type ------
// The walk instances of the trace kernels (bvh_trace.hip modes 4 / 5; kd_trace.hip, §5.7.1) run the
// per-item loop inside the lane, so a call is five kernel nodes whatever max_surfaces is: queue-head reset,
// unfinished-count reset, init, walk, record / finish; no copy, memset, synchronise or event query.  The scratch is the
// per-stream workspace's, sized from max_rays / max_items alone: after one warm-up call nothing is allocated and the
// call can be captured in a hipGraph.  Per scene type: the workspace slots, launch_walk and type_refusal.
enum { kWalkRays, kWalkOrig, kWalkPLight, kWalkState, kWalkRng, kWalkWeights };
// BVH scenes: the slots the pass forms use for the same arrays; kd-tree scenes: the six walk arrays of their workspace
static bool walk_scratch(Workspace *w, int which, size_t bytes, void **out) {
    static constexpr int slot[6] = {Workspace::kRaysA, Workspace::kOrigA, Workspace::kPLight,
                                    Workspace::kState, Workspace::kRng,   Workspace::kWeights};
    return scratch(w, slot[which], bytes, out);
}
static bool walk_scratch(KdWorkspace *w, int which, size_t bytes, void **out) {
    return kd_walk_scratch(w, which, bytes, out);
}

template <class S>
static int walk_shadow_tr(const char *fn, S *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                          const nnbvh_ray_soa *shadow_queue, const int32_t *d_size, const uint8_t *d_prim_class,
                          int64_t n_prim_class, const float *d_Ld, const float *d_r_u, const float *d_r_l,
                          const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_state,
                          int32_t max_surfaces, int32_t *d_unfinished, hipStream_t stream) {
    if (!bounded_args_ok(fn, s, m, max_rays, std::min(n_prim_class, n_pixels), "max_surfaces", max_surfaces,
                         kMaxWalkSurfaces, soa_ok(shadow_queue) && d_Ld && d_r_u && d_r_l && d_pixel_index && d_L,
                         type_refusal))
        return NNBVH_ERR_ARG;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    const int max_blocks = s->n_cus * 8;
    if (d_unfinished && !hip_ok(launch_zero_words(d_unfinished, 1, max_blocks, stream), "unfinished count reset launch"))
        return NNBVH_ERR_DEVICE;
    if (max_rays == 0) return NNBVH_OK;
    const size_t n = (size_t)max_rays;
    void *rays, *orig, *pLight, *state;
    if (!walk_scratch(call.w, kWalkRays, n * 32, &rays) || !walk_scratch(call.w, kWalkOrig, n * 4, &orig) ||
        !walk_scratch(call.w, kWalkPLight, n * 16, &pLight) || !walk_scratch(call.w, kWalkState, n, &state))
        return NNBVH_ERR_DEVICE;
    const WavefrontCount cnt{max_rays, d_size};
    // str_init: every ray's record, light point and state 0 (its item list is the identity and is not read)
    if (!hip_ok(launch_str_init(*shadow_queue, cnt, rays, (int32_t *)orig, (float4 *)pLight, (uint8_t *)state, max_blocks,
                                stream), "shadow-tr init launch"))
        return NNBVH_ERR_DEVICE;
    WalkJob walk;
    walk.kind = 1, walk.mesh = &m->d, walk.rays = rays, walk.n = max_rays, walk.d_n = d_size;
    walk.a.maxSurfaces = max_surfaces, walk.a.unfinished = d_unfinished;
    walk.a.primClass = d_prim_class, walk.a.nPrimClass = (long)n_prim_class;
    walk.a.pLight = (const float4 *)pLight, walk.a.state = (uint8_t *)state;
    const int rc = launch_walk(s, call.w, stream, walk);
    if (rc != NNBVH_OK) return rc;
    if (!hip_ok(launch_str_record((const uint8_t *)state, cnt, d_Ld, d_r_u, d_r_l, d_pixel_index, d_L, (long)n_pixels,
                                  d_state, max_blocks, stream), "shadow-tr record launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

template <class S>
static int walk_one_random(const char *fn, S *s, const nnbvh_shading_mesh *m, int32_t max_items, const float *d_p0,
                           const float *d_p1, const int32_t *d_material, const int32_t *d_size,
                           const int32_t *d_prim_material, int64_t n_prim_material, void *d_sel_hits, void *d_sel_rays,
                           float *d_reservoir_pdf, float *d_weight_sum, int32_t max_surfaces, int32_t *d_unfinished,
                           hipStream_t stream) {
    if (!bounded_args_ok(fn, s, m, max_items, n_prim_material, "max_surfaces", max_surfaces, kMaxWalkSurfaces,
                         d_p0 && d_p1 && d_material && d_sel_hits && d_sel_rays && d_reservoir_pdf, type_refusal))
        return NNBVH_ERR_ARG;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    const int max_blocks = s->n_cus * 8;
    if (d_unfinished && !hip_ok(launch_zero_words(d_unfinished, 1, max_blocks, stream), "unfinished count reset launch"))
        return NNBVH_ERR_DEVICE;
    if (max_items == 0) return NNBVH_OK;
    const size_t n = (size_t)max_items;
    void *rays, *rng, *weights;
    if (!walk_scratch(call.w, kWalkRays, n * 32, &rays) || !walk_scratch(call.w, kWalkRng, n * 16, &rng) ||
        !walk_scratch(call.w, kWalkWeights, n * 8, &weights))
        return NNBVH_ERR_DEVICE;
    OneRandomState st{nullptr, (uint64_t *)rng, (float *)weights};
    const WavefrontCount cnt{max_items, d_size};
    if (!hip_ok(launch_or_init_all(d_p0, d_p1, cnt, st, rays, d_sel_hits, d_sel_rays, max_blocks, stream),
                "one-random init launch"))
        return NNBVH_ERR_DEVICE;
    WalkJob walk;
    walk.kind = 2, walk.mesh = &m->d, walk.rays = rays, walk.n = max_items, walk.d_n = d_size;
    walk.a.maxSurfaces = max_surfaces, walk.a.unfinished = d_unfinished;
    walk.a.p1 = d_p1, walk.a.material = d_material, walk.a.primMaterial = d_prim_material;
    walk.a.nPrimMaterial = (long)n_prim_material, walk.a.st = st;
    walk.a.selHits = (float4 *)d_sel_hits, walk.a.selRays = (float4 *)d_sel_rays;
    const int rc = launch_walk(s, call.w, stream, walk);
    if (rc != NNBVH_OK) return rc;
    if (!hip_ok(launch_or_finish(cnt, st, d_reservoir_pdf, d_weight_sum, max_blocks, stream), "one-random finish launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

extern "C" {

int nnbvh_wavefront_intersect_closest(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                      const int32_t *d_size, const uint8_t *d_prim_class,
                                      int64_t n_prim_class, void *d_hits,
                                      const nnbvh_closest_queues *out, void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out},
                             (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_closest_items(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                            const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                            const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
                                            const nnbvh_closest_queues *out, const nnbvh_closest_items *items,
                                            void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out,
                                 .with_items = true, .mesh = m, .items = items},
                             (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_closest_items_candidates(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                                       const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                                       const uint8_t *d_prim_class, int64_t n_prim_class,
                                                       void *d_hits, const nnbvh_closest_queues *out,
                                                       const nnbvh_closest_items *items,
                                                       const nnbvh_host_candidates *c, void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out,
                                 .with_items = true, .mesh = m, .items = items, .with_candidates = true, .hc = c},
                             (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_shadow(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                     const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                     const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                     int64_t n_pixels, uint8_t *d_occluded, void *stream) {
    return intersect_shadow(s, {.max_rays = max_rays, .queue = shadow_queue, .d_size = d_size, .d_Ld = d_Ld,
                                .d_r_u = d_r_u, .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L,
                                .n_pixels = n_pixels, .d_occluded = d_occluded},
                            (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_shadow_candidates(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                                const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                                const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                                int64_t n_pixels, uint8_t *d_occluded,
                                                const nnbvh_host_candidates *c, void *stream) {
    return intersect_shadow(s, {.max_rays = max_rays, .queue = shadow_queue, .d_size = d_size, .d_Ld = d_Ld,
                                .d_r_u = d_r_u, .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L,
                                .n_pixels = n_pixels, .d_occluded = d_occluded, .with_candidates = true, .hc = c},
                            (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_closest_and_shadow(
    nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
    const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits, const nnbvh_closest_queues *out,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, void *stream) {
    return intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded},
        (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_closest_and_shadow_items(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, int32_t max_shadow_rays,
    const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_occluded,
    void *stream) {
    return intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out, .with_items = true, .mesh = m, .items = items},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded},
        (hipStream_t)stream);
}

int nnbvh_wavefront_intersect_closest_and_shadow_items_candidates(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, const nnbvh_host_candidates *c,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, const nnbvh_host_candidates *shadow_c, void *stream) {
    return intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out, .with_items = true, .mesh = m, .items = items,
         .with_candidates = true, .hc = c},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded,
         .with_candidates = true, .hc = shadow_c},
        (hipStream_t)stream);
}

// ---- kd-tree scenes: the argument lists of the calls of the same name above ---------------------------------------
int nnbvh_kd_wavefront_intersect_closest(nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                         const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class,
                                         void *d_hits, const nnbvh_closest_queues *out, void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits,
                                 .out = out, .kd = true},
                             (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_closest_items(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                               const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                               const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
                                               const nnbvh_closest_queues *out, const nnbvh_closest_items *items,
                                               void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits,
                                 .out = out, .with_items = true, .mesh = m, .items = items, .kd = true},
                             (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_shadow(nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                        const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                        const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                        int64_t n_pixels, uint8_t *d_occluded, void *stream) {
    return intersect_shadow(s, {.max_rays = max_rays, .queue = shadow_queue, .d_size = d_size, .d_Ld = d_Ld,
                                .d_r_u = d_r_u, .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L,
                                .n_pixels = n_pixels, .d_occluded = d_occluded, .kd = true},
                            (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_closest_and_shadow(
    nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
    const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits, const nnbvh_closest_queues *out,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, void *stream) {
    return kd_intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out, .kd = true},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded,
         .kd = true},
        (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_closest_and_shadow_items(
    nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, int32_t max_shadow_rays,
    const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_occluded,
    void *stream) {
    return kd_intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out, .with_items = true, .mesh = m, .items = items,
         .kd = true},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded,
         .kd = true},
        (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_closest_items_candidates(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m,
                                                          int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                                          const int32_t *d_size, const uint8_t *d_prim_class,
                                                          int64_t n_prim_class, void *d_hits,
                                                          const nnbvh_closest_queues *out,
                                                          const nnbvh_closest_items *items,
                                                          const nnbvh_host_candidates *c, void *stream) {
    return intersect_closest(s, {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size,
                                 .d_prim_class = d_prim_class, .n_prim_class = n_prim_class, .d_hits = d_hits,
                                 .out = out, .with_items = true, .mesh = m, .items = items, .with_candidates = true,
                                 .hc = c, .kd = true},
                             (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_shadow_candidates(nnbvh_kd_scene *s, int32_t max_rays,
                                                   const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                                   const float *d_Ld, const float *d_r_u, const float *d_r_l,
                                                   const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
                                                   uint8_t *d_occluded, const nnbvh_host_candidates *c, void *stream) {
    return intersect_shadow(s, {.max_rays = max_rays, .queue = shadow_queue, .d_size = d_size, .d_Ld = d_Ld,
                                .d_r_u = d_r_u, .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L,
                                .n_pixels = n_pixels, .d_occluded = d_occluded, .with_candidates = true, .hc = c,
                                .kd = true},
                            (hipStream_t)stream);
}

int nnbvh_kd_wavefront_intersect_closest_and_shadow_items_candidates(
    nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, const nnbvh_host_candidates *c,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, const nnbvh_host_candidates *shadow_c, void *stream) {
    return kd_intersect_closest_and_shadow(
        s,
        {.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
         .n_prim_class = n_prim_class, .d_hits = d_hits, .out = out, .with_items = true, .mesh = m, .items = items,
         .with_candidates = true, .hc = c, .kd = true},
        {.max_rays = max_shadow_rays, .queue = shadow_queue, .d_size = d_shadow_size, .d_Ld = d_Ld, .d_r_u = d_r_u,
         .d_r_l = d_r_l, .d_pixel_index = d_pixel_index, .d_L = d_L, .n_pixels = n_pixels, .d_occluded = d_occluded,
         .with_candidates = true, .hc = shadow_c, .kd = true},
        (hipStream_t)stream);
}

// ---- the halves of the calls above for records and flags from any source ------------------------------------
int nnbvh_wavefront_enqueue_closest_items_device(const nnbvh_shading_mesh *m, int32_t max_rays,
                                                 const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                                 const void *d_hits, const uint8_t *d_prim_class,
                                                 int64_t n_prim_class, const nnbvh_closest_queues *out,
                                                 const nnbvh_closest_items *items, void *stream) {
    const char *fn = "wavefront_enqueue_closest_items_device";
    const ClosestSide a{.max_rays = max_rays, .queue = ray_queue, .d_size = d_size, .d_prim_class = d_prim_class,
                        .n_prim_class = n_prim_class, .out = out, .with_items = true, .mesh = m, .items = items};
    if (!queue_args_ok(fn, a)) return NNBVH_ERR_ARG;
    if (max_rays > 0 && !d_hits) {
        fail(fn, "no hit records");
        return NNBVH_ERR_ARG;
    }
    if (max_rays == 0) return NNBVH_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    return launch_items(a, d_hits, nullptr, (hipStream_t)stream);
}

int nnbvh_wavefront_enqueue_closest_items_indexed_device(const nnbvh_shading_mesh *m, int32_t max_rays,
                                                         const nnbvh_ray_soa *ray_queue, const int32_t *d_index,
                                                         const int32_t *d_index_size, int32_t max_index,
                                                         const void *d_hits, const uint8_t *d_prim_class,
                                                         int64_t n_prim_class, const nnbvh_closest_queues *out,
                                                         const nnbvh_closest_items *items, void *stream) {
    const char *fn = "wavefront_enqueue_closest_items_indexed_device";
    const ClosestSide a{.max_rays = max_rays, .queue = ray_queue, .n_prim_class = n_prim_class, .out = out,
                        .with_items = true, .mesh = m, .items = items};
    if (!queue_args_ok(fn, a)) return NNBVH_ERR_ARG;
    if (max_index < 0 || (max_index > 0 && max_rays > 0 && (!d_index || !d_hits))) {
        fail(fn, "no index list or no hit records");
        return NNBVH_ERR_ARG;
    }
    if (max_rays == 0 || max_index == 0) return NNBVH_OK;
    DeviceGuard guard(m->device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    if (!hip_ok(launch_wf_enqueue_closest_items(m->d, d_hits, WavefrontCount{max_index, d_index_size}, *ray_queue,
                                                d_prim_class, (long)n_prim_class, *out, *items, m->n_cus * 8,
                                                (hipStream_t)stream, nullptr, d_index, max_rays),
                "work-item enqueue kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

int nnbvh_wavefront_record_shadow_device(const uint8_t *d_occluded, int32_t max_rays, const int32_t *d_size,
                                         const float *d_Ld, const float *d_r_u, const float *d_r_l,
                                         const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
                                         int device, void *stream_) {
    if (max_rays < 0 || n_pixels < 0 ||
        (max_rays > 0 && (!d_occluded || !d_Ld || !d_r_u || !d_r_l || !d_pixel_index || !d_L))) {
        set_error("wavefront_record_shadow_device: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (max_rays == 0) return NNBVH_OK;
    DeviceGuard guard(device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    const WavefrontCount cnt{max_rays, d_size};
    if (!hip_ok(launch_wf_record_shadow(d_occluded, cnt, d_Ld, d_r_u, d_r_l, d_pixel_index, d_L,
                                        (long)n_pixels, 256 * 8, (hipStream_t)stream_),
                "shadow record kernel launch"))
        return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

// ---- IntersectShadowTr / IntersectOneRandom (wavefront/aggregate.cpp:70-116), media-free -------------
// The unbounded calls: shadow_tr_passes / one_random_passes (above) under their host-driven driver.  The only host
// round trip per pass is the 4-byte count of the items that go on (interface surfaces are rare: the usual shadow batch
// ends after its first pass).
int nnbvh_wavefront_intersect_shadow_tr(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                        const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                        const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                        const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index,
                                        float *d_L, int64_t n_pixels, uint8_t *d_state, void *stream_) {
    if (!s || !m || max_rays < 0 || n_pixels < 0 || n_prim_class < 0 ||
        (max_rays > 0 && (!soa_ok(shadow_queue) || !d_Ld || !d_r_u || !d_r_l || !d_pixel_index || !d_L))) {
        set_error("wavefront_intersect_shadow_tr: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (m->device != s->device) {
        set_error("wavefront_intersect_shadow_tr: scene and shading mesh live on different devices");
        return NNBVH_ERR_ARG;
    }
    if (max_rays == 0) return NNBVH_OK;
    hipStream_t stream = (hipStream_t)stream_;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return shadow_tr_passes(s, call.w, m, max_rays, shadow_queue, d_size, d_prim_class, n_prim_class, d_Ld, d_r_u, d_r_l,
                            d_pixel_index, d_L, n_pixels, d_state, kUnbounded, nullptr, stream);
}

int nnbvh_wavefront_intersect_one_random(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items,
                                         const float *d_p0, const float *d_p1, const int32_t *d_material,
                                         const int32_t *d_size, const int32_t *d_prim_material,
                                         int64_t n_prim_material, void *d_sel_hits, void *d_sel_rays,
                                         float *d_reservoir_pdf, float *d_weight_sum, void *stream_) {
    if (!s || !m || max_items < 0 || n_prim_material < 0 ||
        (max_items > 0 && (!d_p0 || !d_p1 || !d_material || !d_sel_hits || !d_sel_rays || !d_reservoir_pdf))) {
        set_error("wavefront_intersect_one_random: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (m->device != s->device) {
        set_error("wavefront_intersect_one_random: scene and shading mesh live on different devices");
        return NNBVH_ERR_ARG;
    }
    if (max_items == 0) return NNBVH_OK;
    hipStream_t stream = (hipStream_t)stream_;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return one_random_passes(s, call.w, m, max_items, d_p0, d_p1, d_material, d_size, d_prim_material, n_prim_material,
                             d_sel_hits, d_sel_rays, d_reservoir_pdf, d_weight_sum, kUnbounded, nullptr, stream);
}

// ---- the bounded forms: the same loops with max_passes passes enqueued up front, kernel launches only ----------
int nnbvh_wavefront_intersect_shadow_tr_bounded(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_state,
    int32_t max_passes, int32_t *d_unfinished, void *stream_) {
    const char *fn = "wavefront_intersect_shadow_tr_bounded";
    if (!bounded_args_ok(fn, s, m, max_rays, std::min(n_prim_class, n_pixels), "max_passes", max_passes, kMaxBoundedPasses,
                         soa_ok(shadow_queue) && d_Ld && d_r_u && d_r_l && d_pixel_index && d_L))
        return NNBVH_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    if (d_unfinished && !hip_ok(launch_zero_words(d_unfinished, 1, s->n_cus * 8, stream), "unfinished count reset launch"))
        return NNBVH_ERR_DEVICE;
    if (max_rays == 0) return NNBVH_OK;
    return shadow_tr_passes(s, call.w, m, max_rays, shadow_queue, d_size, d_prim_class, n_prim_class, d_Ld, d_r_u, d_r_l,
                            d_pixel_index, d_L, n_pixels, d_state, max_passes, d_unfinished, stream);
}

int nnbvh_wavefront_intersect_one_random_bounded(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items, const float *d_p0, const float *d_p1,
    const int32_t *d_material, const int32_t *d_size, const int32_t *d_prim_material, int64_t n_prim_material,
    void *d_sel_hits, void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum, int32_t max_passes,
    int32_t *d_unfinished, void *stream_) {
    const char *fn = "wavefront_intersect_one_random_bounded";
    if (!bounded_args_ok(fn, s, m, max_items, n_prim_material, "max_passes", max_passes, kMaxBoundedPasses,
                         d_p0 && d_p1 && d_material && d_sel_hits && d_sel_rays && d_reservoir_pdf))
        return NNBVH_ERR_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    SceneCall call(s, stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    if (d_unfinished && !hip_ok(launch_zero_words(d_unfinished, 1, s->n_cus * 8, stream), "unfinished count reset launch"))
        return NNBVH_ERR_DEVICE;
    if (max_items == 0) return NNBVH_OK;
    return one_random_passes(s, call.w, m, max_items, d_p0, d_p1, d_material, d_size, d_prim_material, n_prim_material,
                             d_sel_hits, d_sel_rays, d_reservoir_pdf, d_weight_sum, max_passes, d_unfinished, stream);
}

// ---- the walk calls: walk_shadow_tr / walk_one_random (above) under the four names -----------------------------------
int nnbvh_wavefront_walk_shadow_tr(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                   const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                   const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                   const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                   int64_t n_pixels, uint8_t *d_state, int32_t max_surfaces, int32_t *d_unfinished,
                                   void *stream) {
    return walk_shadow_tr("wavefront_walk_shadow_tr", s, m, max_rays, shadow_queue, d_size, d_prim_class, n_prim_class,
                          d_Ld, d_r_u, d_r_l, d_pixel_index, d_L, n_pixels, d_state, max_surfaces, d_unfinished,
                          (hipStream_t)stream);
}

int nnbvh_kd_wavefront_walk_shadow_tr(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                      const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                      const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                      const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                      int64_t n_pixels, uint8_t *d_state, int32_t max_surfaces, int32_t *d_unfinished,
                                      void *stream) {
    return walk_shadow_tr("kd_wavefront_walk_shadow_tr", s, m, max_rays, shadow_queue, d_size, d_prim_class, n_prim_class,
                          d_Ld, d_r_u, d_r_l, d_pixel_index, d_L, n_pixels, d_state, max_surfaces, d_unfinished,
                          (hipStream_t)stream);
}

int nnbvh_wavefront_walk_one_random(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items, const float *d_p0,
                                    const float *d_p1, const int32_t *d_material, const int32_t *d_size,
                                    const int32_t *d_prim_material, int64_t n_prim_material, void *d_sel_hits,
                                    void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum, int32_t max_surfaces,
                                    int32_t *d_unfinished, void *stream) {
    return walk_one_random("wavefront_walk_one_random", s, m, max_items, d_p0, d_p1, d_material, d_size, d_prim_material,
                           n_prim_material, d_sel_hits, d_sel_rays, d_reservoir_pdf, d_weight_sum, max_surfaces,
                           d_unfinished, (hipStream_t)stream);
}

int nnbvh_kd_wavefront_walk_one_random(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_items,
                                       const float *d_p0, const float *d_p1, const int32_t *d_material,
                                       const int32_t *d_size, const int32_t *d_prim_material, int64_t n_prim_material,
                                       void *d_sel_hits, void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum,
                                       int32_t max_surfaces, int32_t *d_unfinished, void *stream) {
    return walk_one_random("kd_wavefront_walk_one_random", s, m, max_items, d_p0, d_p1, d_material, d_size,
                           d_prim_material, n_prim_material, d_sel_hits, d_sel_rays, d_reservoir_pdf, d_weight_sum,
                           max_surfaces, d_unfinished, (hipStream_t)stream);
}

}  // extern "C"
