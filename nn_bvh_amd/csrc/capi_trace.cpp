// capi_trace.cpp — the C ABI of include/nnbvh.h, ray batches: the trace-job launcher, the single-batch and
// candidate calls on device buffers, nnbvh_trace_batches_device and the host-buffer pipeline.  Host code only.
#include <algorithm>
#include <cstring>
#include <thread>

#include "capi_internal.h"

using namespace nnbvh;

// Persistent grid = what is resident at once (register/LDS limited), asked from the runtime
// for the exact kernel instance.  The kernel needs no co-residency (no grid barrier; late
// blocks just find less work in the queues), so a wrong answer costs speed, never results.
// In units of kBlockThreads lanes, as the `blocks_per_cu` option: an instance with larger blocks counts for as many.
int nnbvh::grid_blocks(nnbvh_scene *s, int mode, int candidates) {
    int per_cu = s->blocks_per_cu;
    if (per_cu <= 0) {
        TraceInstance is{};  // (soa = false: a queue's launch is sized by the record form of its lean instance)
        if (!pick_trace_instance(scene_traits(s), mode, candidates > 0, false, &is) ||
            launch_trace(is, TraceParams{}, 0, nullptr, &per_cu) != hipSuccess || per_cu <= 0)
            per_cu = std::max(1, std::min(8, 160 / (s->window * 2)));
        else
            per_cu *= trace_block_threads(is) / kBlockThreads;
    }
    per_cu = std::min(per_cu, 8);
    return s->n_cus * per_cu;
}

bool nnbvh::zero_candidates(int n_cus, const nnbvh_host_candidates *hc, int64_t n, bool closest, hipStream_t stream) {
    return hip_ok(launch_zero_words(hc->count, (long)n, n_cus * 8, stream), "candidate count reset launch") &&
           (!closest || !hc->before ||
            hip_ok(launch_zero_words(hc->before, (long)n, n_cus * 8, stream), "candidate before reset launch"));
}

// the scene and workspace part of a launch's parameters; the launchers add the rays and the outputs
static TraceParams scene_params(const nnbvh_scene *s, const Workspace *w) {
    TraceParams p{};
    p.wide = s->d_wide;
    p.prims = s->d_prims;
    std::memcpy(p.rootMin, s->bounds, 12);
    std::memcpy(p.rootMax, s->bounds + 3, 12);
    p.rootRef = s->root_ref;
    p.queue = w->queue;
    p.nQueues = s->xcd_queues ? kMaxQueues : 1;
    p.primWeight = s->prim_weight;
    p.refillWeight = s->refill_weight;
    p.stats = s->d_stats;
    p.intRepeat = s->int_repeat;
    p.topBurst = s->top_burst;
    p.primRepeat = s->prim_repeat;
    p.fits32 = scene_fits32(s);
    p.hasHostPrims = s->has_host_prims;
    p.spill = w->spill;
    p.anim = s->d_anim;
    p.alphaTex = (const float4 *)s->d_alpha_tex;
    p.alphaTexels = s->d_alpha_texels;
    return p;
}

// queue heads zeroed, then the instance (have: there is one) over p.n rays, on no more threads than rays (tiny batches).
// `blocks` counts kBlockThreads lanes (grid_blocks); the instance's own blocks cover no more lanes than that (but one
// block at least), so the spill array (max_grid_threads = 8 such units per CU) covers every grid.
static int run_instance(bool have, const TraceInstance &is, const TraceParams &p, int blocks, int queue_words,
                        hipStream_t stream, const char *what) {
    if (!hip_ok(launch_zero_queue(p.queue, queue_words, stream), "queue reset launch")) return NNBVH_ERR_DEVICE;
    const int threads = have ? trace_block_threads(is) : kBlockThreads;
    blocks = std::max(1, (int)((int64_t)blocks * kBlockThreads / threads));
    const int64_t need = (p.n + threads - 1) / threads;
    if (need < blocks) blocks = (int)std::max<int64_t>(need, 1);
    const hipError_t e = have ? launch_trace(is, p, blocks, stream, nullptr) : hipErrorInvalidValue;
    return hip_ok(e, what) ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

// ... the instance of `mode` for the scene: its candidate-mode twin (candidates), its form for wavefront queues (soa)
static int run_trace(nnbvh_scene *s, hipStream_t stream, int mode, bool candidates, bool soa, const TraceParams &p,
                     int queue_words, const char *what) {
    TraceInstance is{};
    const bool have = pick_trace_instance(scene_traits(s), mode, candidates, soa, &is);
    return run_instance(have, is, p, grid_blocks(s, mode, candidates), queue_words, stream, what);
}

int nnbvh::launch(nnbvh_scene *s, Workspace *w, hipStream_t stream, const TraceJob &job) {
    TraceParams p = scene_params(s, w);
    if (job.soa) p.soa = *job.soa;
    p.rays = (const nnbvh_ray *)job.rays;
    p.hits = (nnbvh_hit *)job.hits;
    p.occluded = (uint8_t *)job.occluded;
    p.visitedOut = (int32_t *)job.visited;
    p.testsOut = (int32_t *)job.tests;
    p.n = (long)job.n;
    p.nDev = job.d_n;
    if (const nnbvh_host_candidates *hc = job.hc) {
        int32_t *before = job.mode == 0 ? hc->before : nullptr;  // not an output of any hit
        const size_t bytes = (size_t)job.n * sizeof(int32_t);
        if (!job.hc_zeroed &&
            (!hip_ok(hipMemsetAsync(hc->count, 0, bytes, stream), "hipMemsetAsync(count)") ||
             (before && !hip_ok(hipMemsetAsync(before, 0, bytes, stream), "hipMemsetAsync(before)"))))
            return NNBVH_ERR_DEVICE;
        if (s->has_host_prims) {
            p.hcCap = hc->capacity;
            p.hcCount = hc->count;
            p.hcBefore = before;
            p.hcPrim = hc->prim;
            p.hcInst = hc->instance;
        }
    }
    const bool candidates = job.hc && s->has_host_prims && job.hc->capacity > 0;
    return run_trace(s, stream, job.mode, candidates, !job.rays, p, kMaxQueues * kQueueStrideWords,
                     "trace kernel launch");
}

const char *nnbvh::walk_refusal(const nnbvh_scene *s) {
    if (s->instanced && s->d_anim)
        return "the scene holds AnimatedPrimitive instances (the INST = 2 kernels), which have no walk instances";
    if (s->has_alpha)
        return "the scene holds alpha-tested primitives on the device (the ALPHA kernels), which have no walk instances";
    return nullptr;
}

int nnbvh::launch_walk(nnbvh_scene *s, Workspace *w, hipStream_t stream, const WalkJob &k) {
    TraceParams p = scene_params(s, w);
    p.rays = (const nnbvh_ray *)k.rays;
    p.n = (long)k.n;
    p.nDev = k.d_n;
    p.wMesh = *k.mesh;
    p.walk = k.a;
    TraceInstance is{};  // (form 0, the lean one, where launch_str_step chooses FULL = false)
    int form = 0;
    const ShadingMeshDevice &m = *k.mesh;
    if (!pick_walk_instance(scene_traits(s), k.kind, m.patchVerts != nullptr, m.instances != nullptr, &is, &form))
        return run_instance(false, is, p, 0, kMaxQueues * kQueueStrideWords, stream, "walk kernel launch");
    int &per_cu = s->walk_blocks_per_cu[3 * (k.kind - 1) + form];
    if (per_cu == 0) {
        int occ = 0;  // (at most 8: the spill array is sized for 8 blocks per CU)
        per_cu = (launch_trace(is, p, 0, nullptr, &occ) == hipSuccess && occ > 0) ? std::min(occ, 8) : 2;
    }
    return run_instance(true, is, p, s->n_cus * per_cu, kMaxQueues * kQueueStrideWords, stream, "walk kernel launch");
}

// The caller has checked that the scene and the batches allow it (batches_fusable).  d_n: nullable array of nullable
// device-resident batch sizes.  soas (nullable): soas[i] is batch i's wavefront queue where its d_rays is null.
// cands (nullable): cands[i] belongs to batches[i], capacity 0 = a plain batch.  Their count / before arrays are zeroed
// by kernel nodes; scenes with host-only primitives then run the kernel's candidate-mode instances (ray records only).
int nnbvh::launch_fused_batches(nnbvh_scene *s, Workspace *w, hipStream_t stream, const nnbvh_batch *batches,
                                int n_batches, const int32_t *const *d_n, const nnbvh_ray_soa *const *soas,
                                const nnbvh_host_candidates *cands) {
    TraceParams p = scene_params(s, w);
    int64_t total = 0;
    bool candidates = false, soa = false;  // some batch has candidate arrays / is a wavefront queue
    for (int i = 0; i < n_batches; ++i) {
        if (batches[i].n == 0) continue;  // empty batches take no slot
        const int b = p.nBatches++;
        p.bRays[b] = (const nnbvh_ray *)batches[i].d_rays;
        soa = soa || !batches[i].d_rays;
        p.bOut[b] = batches[i].d_out;
        p.bN[b] = (long)batches[i].n;
        p.bNDev[b] = d_n ? d_n[i] : nullptr;
        if (soas && soas[i]) p.bSoa[b] = *soas[i];  // with d_rays == nullptr: read as SOA slices
        if (batches[i].kind == NNBVH_BATCH_ANY) p.anyMask |= 1u << b;
        total += batches[i].n;
        if (cands && cands[i].capacity > 0) {
            const bool closest = batches[i].kind == NNBVH_BATCH_CLOSEST;
            if (!zero_candidates(s->n_cus, &cands[i], batches[i].n, closest, stream)) return NNBVH_ERR_DEVICE;
            if (s->has_host_prims) {
                candidates = true;
                p.hcCap = 1;  // candidate mode (the mode-3 instances read bHcCap[b])
                p.bHcCap[b] = cands[i].capacity;
                p.bHcCount[b] = cands[i].count;
                p.bHcBefore[b] = closest ? cands[i].before : nullptr;
                p.bHcPrim[b] = cands[i].prim;
                p.bHcInst[b] = cands[i].instance;
            }
        }
    }
    if (p.nBatches == 0) return NNBVH_OK;
    p.n = (long)total;
    // the lean instances (record and SOA form) serve the scene's top records from LDS: the walk enters at the tagged root
    if (s->d_top && s->use_top && !candidates && scene_runs_lean(s)) {
        p.top = s->d_top;
        p.nTop = s->n_top;
        p.rootRef = kTopTag;  // slot 0
    }
    return run_trace(s, stream, 3, candidates, soa, p, kMaxFusedBatches * kMaxQueues * kQueueStrideWords,
                     "fused trace kernel launch");
}

bool nnbvh::batches_fusable(const nnbvh_scene *s, const nnbvh_batch *batches, int n_batches) {
    bool fusable = s->fused_batches && n_batches <= kMaxFusedBatches && s->window == 8 && !s->has_alpha;
    for (int i = 0; fusable && i < n_batches; ++i)
        fusable = batches[i].n < (1LL << kFusedIndexBits) &&
                  !(batches[i].kind == NNBVH_BATCH_ANY && (batches[i].d_nodes_visited || batches[i].d_prim_tests));
    return fusable;
}

// ---- host-only primitives as candidates (include/nnbvh.h) ----------------------------------------------------
// capacity 0 = "no candidates" is the caller's to allow
const char *nnbvh::candidates_fault(const nnbvh_host_candidates *c, bool closest) {
    if (!c) return "candidates is NULL";
    if (c->capacity < 1 || c->capacity > 16) return "capacity must be 1..16";
    if (!c->count || !c->prim || !c->instance) return "count, prim and instance are required";
    if (closest && !c->before) return "before is required for closest hit";
    return nullptr;
}

bool nnbvh::candidates_ok(const char *fn, const nnbvh_host_candidates *c, bool closest) {
    const char *why = candidates_fault(c, closest);
    if (why) set_error(std::string(fn) + ": " + why);
    return !why;
}

// the arguments of a single-batch call; the candidate calls pass their candidates_fault
static bool batch_args_ok(const char *fn, const nnbvh_scene *s, int64_t n, const void *rays, const void *out,
                          const char *candidates_wrong = nullptr) {
    const char *why = nullptr;
    if (!s || n < 0 || (n > 0 && (!rays || !out))) why = "bad argument";
    else if (candidates_wrong) why = candidates_wrong;
    else if (n >= 0x7fffffffLL) why = "at most 2^31-1 rays per call";
    if (why) set_error(std::string(fn) + ": " + why);
    return !why;
}

extern "C" {

int nnbvh_intersect_closest_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                   void *stream) {
    if (!batch_args_ok("intersect_closest_device", s, n, d_rays, d_hits)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return launch(s, call.w, (hipStream_t)stream, {.mode = 0, .rays = d_rays, .n = n, .hits = d_hits});
}

int nnbvh_intersect_any_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                               void *d_nodes_visited, void *d_prim_tests, void *stream) {
    if (!batch_args_ok("intersect_any_device", s, n, d_rays, d_occluded)) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return launch(s, call.w, (hipStream_t)stream,
                  {.mode = (d_nodes_visited || d_prim_tests) ? 1 : 2, .rays = d_rays, .n = n, .occluded = d_occluded,
                   .visited = d_nodes_visited, .tests = d_prim_tests});
}

int nnbvh_intersect_closest_candidates_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                              const nnbvh_host_candidates *c, void *stream) {
    if (!batch_args_ok("intersect_closest_candidates_device", s, n, d_rays, d_hits, candidates_fault(c, true)))
        return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return launch(s, call.w, (hipStream_t)stream, {.mode = 0, .rays = d_rays, .n = n, .hits = d_hits, .hc = c});
}

int nnbvh_intersect_any_candidates_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                          const nnbvh_host_candidates *c, void *stream) {
    if (!batch_args_ok("intersect_any_candidates_device", s, n, d_rays, d_occluded, candidates_fault(c, false)))
        return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    SceneCall call(s, (hipStream_t)stream);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    return launch(s, call.w, (hipStream_t)stream,
                  {.mode = 2, .rays = d_rays, .n = n, .occluded = d_occluded, .hc = c});
}

}  // extern "C"

// host buffers (candidates_host of capi_internal.h stages them): the one launch is a trace job, mode 0 or 2
static int candidates_host(const char *fn, nnbvh_scene *s, int mode, const nnbvh_ray *rays, int64_t n, void *out,
                           const nnbvh_host_candidates *c) {
    if (!batch_args_ok(fn, s, n, rays, out, candidates_fault(c, mode == 0))) return NNBVH_ERR_ARG;
    if (n == 0) return NNBVH_OK;
    return nnbvh::candidates_host(s, mode == 0, rays, n, out, c,
                                  [&](Workspace *w, void *d_rays, void *d_out, const nnbvh_host_candidates &d) {
                                      TraceJob job{.mode = mode, .rays = d_rays, .n = n, .hc = &d};
                                      (mode == 0 ? job.hits : job.occluded) = d_out;
                                      return launch(s, w, nullptr, job);
                                  });
}

// nnbvh_trace_batches_device and its candidates form (cands nullable; cands[i] belongs to batches[i])
static int trace_batches(const char *fn, nnbvh_scene *s, const nnbvh_batch *batches, int n_batches,
                         const nnbvh_host_candidates *cands, hipStream_t stream) {
    if (!s || n_batches < 0 || (n_batches > 0 && !batches)) {
        set_error(std::string(fn) + ": bad argument");
        return NNBVH_ERR_ARG;
    }
    for (int i = 0; i < n_batches; ++i) {
        const nnbvh_batch &b = batches[i];
        if ((b.kind != NNBVH_BATCH_CLOSEST && b.kind != NNBVH_BATCH_ANY) || b.n < 0 ||
            b.n >= 0x7fffffffLL || (b.n > 0 && (!b.d_rays || !b.d_out))) {
            set_error(std::string(fn) + ": bad batch (kind, size or null buffer)");
            return NNBVH_ERR_ARG;
        }
        if (!cands || cands[i].capacity == 0) continue;
        const char *why = candidates_fault(&cands[i], b.kind == NNBVH_BATCH_CLOSEST);
        if (!why && b.kind == NNBVH_BATCH_ANY && (b.d_nodes_visited || b.d_prim_tests))
            why = "an any-hit batch has exact counts or candidates, not both";
        if (why) {
            set_error(std::string(fn) + ": batch candidates: " + why);
            return NNBVH_ERR_ARG;
        }
    }
    if (n_batches == 0) return NNBVH_OK;
    SceneCall call(s);  // the workspaces are those of the streams the batches run on
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    // One launch for all batches (mode 3) when they are closest-hit / occlusion-only any-hit batches of
    // fewer than 2^28 rays each: they share one ramp-up and one drain instead of paying one each.
    if (batches_fusable(s, batches, n_batches)) {
        Workspace *w = workspace_for(s, stream);
        if (!w) return NNBVH_ERR_DEVICE;
        return launch_fused_batches(s, w, stream, batches, n_batches, nullptr, nullptr, cands);
    }
    if (!s->ev_fork) {
        bool ok = hip_ok(hipEventCreateWithFlags(&s->ev_fork, hipEventDisableTiming), "hipEventCreate");
        for (int k = 0; ok && k < nnbvh_scene::kSideStreams; ++k)
            ok = hip_ok(hipStreamCreateWithFlags(&s->side[k], hipStreamNonBlocking), "hipStreamCreate") &&
                 hip_ok(hipEventCreateWithFlags(&s->ev_join[k], hipEventDisableTiming), "hipEventCreate");
        if (!ok) return NNBVH_ERR_DEVICE;
    }
    if (!hip_ok(hipEventRecord(s->ev_fork, stream), "hipEventRecord(fork)")) return NNBVH_ERR_DEVICE;
    bool used[nnbvh_scene::kSideStreams] = {false, false, false, false};
    for (int i = 0; i < n_batches; ++i) {
        const nnbvh_batch &b = batches[i];
        if (b.n == 0) continue;
        const int k = i % nnbvh_scene::kSideStreams;
        if (!used[k]) {
            if (!hip_ok(hipStreamWaitEvent(s->side[k], s->ev_fork, 0), "hipStreamWaitEvent(fork)"))
                return NNBVH_ERR_DEVICE;
            used[k] = true;
        }
        Workspace *w = workspace_for(s, s->side[k]);
        if (!w) return NNBVH_ERR_DEVICE;
        const bool closest = b.kind == NNBVH_BATCH_CLOSEST;
        // one launch per batch (with its candidates: modes 0 / 2), forked and joined like the others
        TraceJob job{.rays = b.d_rays, .n = b.n};
        if (cands && cands[i].capacity > 0) {
            if (!zero_candidates(s->n_cus, &cands[i], b.n, closest, s->side[k])) return NNBVH_ERR_DEVICE;
            job.hc = &cands[i];
            job.hc_zeroed = true;
        }
        if (closest) {
            job.hits = b.d_out;
        } else {
            job.mode = (b.d_nodes_visited || b.d_prim_tests) ? 1 : 2;
            job.occluded = b.d_out;
            job.visited = b.d_nodes_visited;
            job.tests = b.d_prim_tests;
        }
        const int rc = launch(s, w, s->side[k], job);
        if (rc != NNBVH_OK) return rc;
    }
    for (int k = 0; k < nnbvh_scene::kSideStreams; ++k) {
        if (!used[k]) continue;
        if (!hip_ok(hipEventRecord(s->ev_join[k], s->side[k]), "hipEventRecord(join)") ||
            !hip_ok(hipStreamWaitEvent(stream, s->ev_join[k], 0), "hipStreamWaitEvent(join)"))
            return NNBVH_ERR_DEVICE;
    }
    return NNBVH_OK;
}

extern "C" {

int nnbvh_intersect_closest_candidates(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits,
                                       const nnbvh_host_candidates *c) {
    return candidates_host("intersect_closest_candidates", s, 0, rays, n, hits, c);
}

int nnbvh_intersect_any_candidates(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                                   const nnbvh_host_candidates *c) {
    return candidates_host("intersect_any_candidates", s, 2, rays, n, occluded, c);
}

int nnbvh_trace_batches_device(nnbvh_scene *s, const nnbvh_batch *batches, int n_batches,
                               void *stream) {
    return trace_batches("trace_batches_device", s, batches, n_batches, nullptr, (hipStream_t)stream);
}

int nnbvh_trace_batches_candidates_device(nnbvh_scene *s, const nnbvh_batch *batches, int n_batches,
                                          const nnbvh_host_candidates *cands, void *stream) {
    if (n_batches > 0 && !cands) {
        set_error("trace_batches_candidates_device: candidates is NULL");
        return NNBVH_ERR_ARG;
    }
    return trace_batches("trace_batches_candidates_device", s, batches, n_batches, cands, (hipStream_t)stream);
}

}  // extern "C"

// ---- host-buffer entry points: a pipeline of chunks -------------------------------------------------
// What Integrator::Intersect / IntersectP callers (cpu/integrators.cpp:296-313) hand over lives in host
// memory.  The batch is cut into chunks of up to kHostChunk rays that rotate over kHostSlots slots, each
// with its own stream, device buffers and traversal workspace: chunk k's rays go up while chunk k-1 is
// traced and chunk k-2's results come down.  Memory the caller has pinned (hipHostMalloc / hipHostRegister,
// nnbvh_host_register) is read and written by the copy engines directly; pageable memory goes through pinned
// staging buffers filled / drained by a few host threads while the other slots' GPU work is in flight.
// Every ray's result is what the single-shot path gives (rays are independent).
static bool host_is_pinned(const void *p) {
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError();  // an ordinary (unregistered) host pointer: not an error
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

static void parallel_copy(void *dst, const void *src, size_t bytes) {
    constexpr size_t kPiece = 4u << 20;
    const int pieces = (int)std::min<size_t>(4, bytes / kPiece);
    if (pieces < 2) {
        std::memcpy(dst, src, bytes);
        return;
    }
    const size_t each = (bytes / (size_t)pieces + 63) & ~(size_t)63;
    std::thread helpers[3];
    for (int k = 1; k < pieces; ++k) {
        const size_t off = each * (size_t)k, len = (k == pieces - 1) ? bytes - off : each;
        helpers[k - 1] = std::thread([=] { std::memcpy((char *)dst + off, (const char *)src + off, len); });
    }
    std::memcpy(dst, src, each);
    for (int k = 1; k < pieces; ++k) helpers[k - 1].join();
}

struct HostArray {  // one per-ray output array of a call
    void *host;
    size_t elem;  // bytes per ray
    bool pinned;
};

static bool slot_reserve(HostSlot &sl, size_t rays, bool need_staging_in, const HostArray *outs, int n_outs) {
    for (hipEvent_t *e : {&sl.ev_in, &sl.ev_traced, &sl.ev_out})
        if (!*e && !hip_ok(hipEventCreateWithFlags(e, hipEventDisableTiming), "hipEventCreate")) return false;
    auto dev = [&](void **p, size_t *have, size_t need) {
        if (*have >= need) return true;
        if (*p) (void)hipFree(*p);
        *p = nullptr;
        *have = 0;
        if (!hip_ok(hipMalloc(p, need), "hipMalloc(host pipeline)")) return false;
        *have = need;
        return true;
    };
    auto pin = [&](void **p, size_t *have, size_t need) {
        if (*have >= need) return true;
        if (*p) (void)hipHostFree(*p);
        *p = nullptr;
        *have = 0;
        if (!hip_ok(hipHostMalloc(p, need, hipHostMallocDefault), "hipHostMalloc(host pipeline)")) return false;
        *have = need;
        return true;
    };
    if (!dev(&sl.d_in, &sl.d_in_bytes, rays * 32)) return false;
    if (need_staging_in && !pin(&sl.h_in, &sl.h_in_bytes, rays * 32)) return false;
    for (int k = 0; k < n_outs; ++k) {
        if (!dev(&sl.d_out[k], &sl.d_out_bytes[k], rays * outs[k].elem)) return false;
        if (outs[k].host && !outs[k].pinned && !pin(&sl.h_out[k], &sl.h_out_bytes[k], rays * outs[k].elem)) return false;
    }
    return true;
}

// mode 0: outs = {hits}; mode 1 / 2: outs = {occluded, nodes_visited?, prim_tests?} (absent arrays: host = null)
//
// Three streams with fixed roles — upload, trace, download — and per-slot events between them.  The copies have
// their own streams on purpose: a copy queued on the stream of the kernel it depends on is performed by a copy
// KERNEL, which has to wait for compute units behind the next chunk's persistent trace kernel (measured: no
// overlap at all); a copy on a stream of its own goes to a DMA engine and overlaps the trace
// (tools/overlap_copy_probe.py: trace + upload = upload alone).
static int host_pipeline(nnbvh_scene *s, int mode, const nnbvh_ray *rays, int64_t n, HostArray *outs, int n_outs) {
    for (hipStream_t *st : {&s->host_up, &s->host_trace, &s->host_down})
        if (!*st && !hip_ok(hipStreamCreateWithFlags(st, hipStreamNonBlocking), "hipStreamCreate")) return NNBVH_ERR_DEVICE;
    const bool rays_pinned = host_is_pinned(rays);
    for (int k = 0; k < n_outs; ++k) outs[k].pinned = outs[k].host && host_is_pinned(outs[k].host);
    // chunks: a launch costs ~0.5 ms of ramp-up and drain whatever its size (DESIGN.md "why launches are large"), so
    // a batch is cut into at most kHostChunks chunks of at least host_chunk rays
    int64_t chunk = std::max<int64_t>(s->host_chunk, (n + nnbvh_scene::kHostChunks - 1) / nnbvh_scene::kHostChunks);
    chunk = std::min<int64_t>(chunk, n);
    const int64_t n_chunks = (n + chunk - 1) / chunk;
    Workspace *w = workspace_for(s, s->host_trace);
    if (!w) return NNBVH_ERR_DEVICE;
    struct Pending {
        int64_t first = 0, count = 0;
        bool busy = false;
    } pending[nnbvh_scene::kHostSlots];
    auto drain = [&](int slot) -> bool {  // wait for the slot's chunk and hand its staged results to the caller
        Pending &pd = pending[slot];
        if (!pd.busy) return true;
        HostSlot &sl = s->host_slots[slot];
        if (!hip_ok(hipEventSynchronize(sl.ev_out), "host pipeline")) return false;
        for (int k = 0; k < n_outs; ++k)
            if (outs[k].host && !outs[k].pinned)
                parallel_copy((char *)outs[k].host + (size_t)pd.first * outs[k].elem, sl.h_out[k], (size_t)pd.count * outs[k].elem);
        pd.busy = false;
        return true;
    };
    for (int64_t c = 0; c < n_chunks; ++c) {
        const int slot = (int)(c % nnbvh_scene::kHostSlots);
        if (!drain(slot)) return NNBVH_ERR_DEVICE;
        HostSlot &sl = s->host_slots[slot];
        const int64_t first = c * chunk, count = std::min<int64_t>(chunk, n - first);
        if (!slot_reserve(sl, (size_t)chunk, !rays_pinned, outs, n_outs)) return NNBVH_ERR_DEVICE;
        const void *src = rays + first;
        if (!rays_pinned) {
            parallel_copy(sl.h_in, rays + first, (size_t)count * 32);
            src = sl.h_in;
        }
        if (!hip_ok(hipMemcpyAsync(sl.d_in, src, (size_t)count * 32, hipMemcpyHostToDevice, s->host_up), "copy rays") ||
            !hip_ok(hipEventRecord(sl.ev_in, s->host_up), "host pipeline") ||
            !hip_ok(hipStreamWaitEvent(s->host_trace, sl.ev_in, 0), "host pipeline"))
            return NNBVH_ERR_DEVICE;
        TraceJob job{.mode = mode, .rays = sl.d_in, .n = count};
        if (mode == 0) {
            job.hits = sl.d_out[0];
        } else {
            job.occluded = sl.d_out[0];
            job.visited = n_outs > 1 ? sl.d_out[1] : nullptr;
            job.tests = n_outs > 2 ? sl.d_out[2] : nullptr;
        }
        const int rc = launch(s, w, s->host_trace, job);
        if (rc != NNBVH_OK) return rc;
        if (!hip_ok(hipEventRecord(sl.ev_traced, s->host_trace), "host pipeline") ||
            !hip_ok(hipStreamWaitEvent(s->host_down, sl.ev_traced, 0), "host pipeline"))
            return NNBVH_ERR_DEVICE;
        for (int k = 0; k < n_outs; ++k) {
            if (!outs[k].host) continue;
            void *dst = outs[k].pinned ? (void *)((char *)outs[k].host + (size_t)first * outs[k].elem) : sl.h_out[k];
            if (!hip_ok(hipMemcpyAsync(dst, sl.d_out[k], (size_t)count * outs[k].elem, hipMemcpyDeviceToHost, s->host_down),
                        "copy results"))
                return NNBVH_ERR_DEVICE;
        }
        if (!hip_ok(hipEventRecord(sl.ev_out, s->host_down), "host pipeline")) return NNBVH_ERR_DEVICE;
        pending[slot].first = first;
        pending[slot].count = count;
        pending[slot].busy = true;
    }
    for (int64_t c = n_chunks; c < n_chunks + nnbvh_scene::kHostSlots; ++c)  // oldest first
        if (!drain((int)(c % nnbvh_scene::kHostSlots))) return NNBVH_ERR_DEVICE;
    return NNBVH_OK;
}

extern "C" {

int nnbvh_intersect_closest(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits) {
    if (!s || n < 0 || (n > 0 && (!rays || !hits))) {
        set_error("intersect_closest: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    if (n >= 0x7fffffffLL) {
        set_error("intersect_closest: at most 2^31-1 rays per call");
        return NNBVH_ERR_ARG;
    }
    SceneCall call(s);  // host path: one call at a time per scene; the pipeline has streams of its own
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    HostArray outs[1] = {{hits, 32, false}};
    return host_pipeline(s, 0, rays, n, outs, 1);
}

int nnbvh_intersect_any(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                        int32_t *nodes_visited, int32_t *prim_tests) {
    if (!s || n < 0 || (n > 0 && (!rays || !occluded))) {
        set_error("intersect_any: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (n == 0) return NNBVH_OK;
    if (n >= 0x7fffffffLL) {
        set_error("intersect_any: at most 2^31-1 rays per call");
        return NNBVH_ERR_ARG;
    }
    SceneCall call(s);
    if (!call.ok()) return NNBVH_ERR_DEVICE;
    const bool counts = nodes_visited || prim_tests;
    // with counts the kernel writes both arrays; one the caller did not ask for stays on the device
    HostArray outs[3] = {{occluded, 1, false}, {nodes_visited, 4, false}, {prim_tests, 4, false}};
    return host_pipeline(s, counts ? 1 : 2, rays, n, outs, counts ? 3 : 1);
}

int nnbvh_host_register(void *ptr, size_t bytes) {
    if (!ptr || bytes == 0) {
        set_error("host_register: bad argument");
        return NNBVH_ERR_ARG;
    }
    if (reinterpret_cast<uintptr_t>(ptr) % 4096 != 0) {
        // a registration covers whole pages: a buffer that shares its first page with other heap objects would
        // leave THEIR memory mapped into the GPU's address space (include/nnbvh.h)
        set_error("host_register: the buffer must be page-aligned (4096) and own its pages");
        return NNBVH_ERR_ARG;
    }
    return hip_ok(hipHostRegister(ptr, bytes, hipHostRegisterDefault), "hipHostRegister") ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

int nnbvh_host_unregister(void *ptr) {
    if (!ptr) {
        set_error("host_unregister: bad argument");
        return NNBVH_ERR_ARG;
    }
    return hip_ok(hipHostUnregister(ptr), "hipHostUnregister") ? NNBVH_OK : NNBVH_ERR_DEVICE;
}

}  // extern "C"
