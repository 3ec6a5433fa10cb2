// nnbvh_aggregate.hpp — header-only C++17 adapter over the C ABI (include/nnbvh.h) with the
// shape of pbrt's aggregate interfaces, so a pbrt build can use the HIP path unchanged:
//
//   per-ray     Primitive::{Bounds, Intersect, IntersectP}
//               (/root/reference/src/pbrt/cpu/primitive.h:33-45; BVHAggregate's versions at
//                cpu/aggregates.h:28-70, cpu/aggregates.cpp:524-624)
//   batched     WavefrontAggregate::{Bounds, IntersectClosest, IntersectShadow, IntersectShadowTr,
//               IntersectOneRandom}
//               (/root/reference/src/pbrt/wavefront/integrator.h:32-54; CPU implementation
//                wavefront/aggregate.cpp:34-116; the last two in their media-free form)
//   kd-tree     KdTreeAggregate (cpu/aggregates.h:75-105) as HipKdTreeAggregate
//   film        RGBFilm's accumulators (film.h:232-316) as HipFilm
//
// The class owns only the opaque scene handle.  Error behaviour mirrors the reference: pbrt
// aborts through CHECK / LOG_FATAL (util/check.h:36-57, cpu/aggregates.cpp:145); here every
// failure goes through nnbvh::HipBVHAggregate::fatal, which prints the C ABI's message and
// aborts unless the embedder installs its own handler (e.g. one that calls pbrt's ErrorExit).
//
// A per-ray Intersect() is a batch of one: correct, and three orders of magnitude slower
// than the batched calls (a kernel launch per ray).  It exists so that the CPU integrators
// can call the aggregate "unchanged" for validation; production callers batch.
// CoalescingAggregate<> is the middle way for those integrators: the rays of the many threads of
// pbrt's ParallelFor2D (util/parallel.cpp:301-330) that are inside Intersect() at the same moment are
// traced as ONE batch.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <chrono>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "nnbvh.h"

namespace nnbvh {

struct Point3f {
    float x, y, z;
};
using Vector3f = Point3f;
struct Bounds3f {
    Point3f pMin, pMax;
};
// the fields of pbrt's Ray the path reads (ray.h:18-39)
struct Ray {
    Point3f o;
    Vector3f d;
    float time = 0;
};
// what TriangleIntersection / BilinearIntersection + the primitive index carry
// (shapes.h:820-824, 1271-1275); a pbrt embedder turns this into a ShapeIntersection with
// Triangle::InteractionFromIntersection (shapes.h:884-1010) on the host.
struct HitRecord {
    int prim;
    float tHit;
    float b0, b1, b2;  // patch: b0 = u, b1 = v
    int instance = 0;  // 0 = top level, k + 1 = inside instance k (nnbvh_hit.instance)
};
// A ray whose result is VOID: a primitive only the host can intersect (NNBVH_PRIM_HOST: quadric, curve,
// textured alpha ...) lay on its way, so neither "hit", "miss" nor "occluded" is known and the caller must
// re-trace it on the CPU (nnbvh_hit.instance == -1 / occluded == 2).  The single-ray adapters report it
// through the optional `needsHost` out-parameter; without one such a ray is fatal, never a silent answer.
//
// The overloads that take a `hostIntersect` callable do without the CPU re-trace: the device lists the host-only
// primitives each ray reached (nnbvh_host_candidates) and the adapter asks the callable about those few, merging
// the answers with the device hit by the rule of include/nnbvh.h.  hostIntersect(prim, instance, ray, tMax) ->
// std::optional<HostHit> is the embedder's primitives[prim].Intersect(ray, tMax) (prim = nnbvh_prim.id); for
// instance > 0 the render-space ray must be taken into instance instance - 1's space, as TransformedPrimitive
// does.  A ray the list cannot settle (more candidates than the capacity, an alpha re-trace: count < 0) goes the
// needsHost / fatal way above.
struct HostHit {
    float tHit;
    float b0 = 0, b1 = 0, b2 = 0;  // whatever the embedder wants back for its own shapes
};
// the merged closest hit and which primitive won it
struct ResolvedHit {
    HitRecord hit;      // prim / instance name the winner, device primitive or host candidate
    bool host = false;  // true: a host candidate (the embedder's shape) won
};

// The candidate overloads of HipBVHAggregate and HipKdTreeAggregate: one trace call that fills nnbvh_host_candidates
// (trace(rays, n, out, &c) -> NNBVH_* status: the scene type's entry point), then the merge rule of include/nnbvh.h.
// fail(message) is the class's fatal().
namespace detail {
// the ids of the bilinear patches, sorted: the merge rule's comparison for a device hit depends on its kind
inline void note_patch_ids(std::vector<int32_t> &ids, const nnbvh_prim *prims, int n) {
    for (int i = 0; i < n; ++i)
        if (prims[i].kind == NNBVH_PRIM_BILINEAR_PATCH || (prims[i].kind >= NNBVH_PRIM_ALPHA_PATCH && prims[i].kind <= NNBVH_PRIM_ALPHA_PATCH_UV_SMOOTH_FLIPPED))
            ids.push_back(prims[i].id);
    std::sort(ids.begin(), ids.end());
}
// count < 0: the candidates cannot settle the ray (more than the capacity, or an alpha re-trace)
template <typename Fail>
bool candidates_settle(int32_t count, uint8_t *needsHost, const char *what, Fail &&fail) {
    if (needsHost) *needsHost = count < 0;
    if (count < 0 && !needsHost)
        fail(std::string(what) + ": the ray's host candidates cannot settle it (pass needsHost and re-trace it on the CPU)");
    return count >= 0;
}
inline Ray ray_of(const nnbvh_ray &r) { return Ray{{r.o[0], r.o[1], r.o[2]}, {r.d[0], r.d[1], r.d[2]}, r.time}; }

template <typename Trace, typename F, typename Fail>
void resolve_closest(Trace &&trace, const std::vector<int32_t> &patchIds, const nnbvh_ray *rays, int64_t n,
                     std::optional<ResolvedHit> *hits, F &&hostIntersect, uint8_t *needsHost, int capacity,
                     const char *what, Fail &&fail) {
    std::vector<nnbvh_hit> rec((size_t)n);
    std::vector<int32_t> count((size_t)n), before((size_t)n), prim((size_t)n * capacity), inst((size_t)n * capacity);
    nnbvh_host_candidates c{capacity, count.data(), before.data(), prim.data(), inst.data()};
    if (trace(rays, n, rec.data(), &c) != NNBVH_OK) fail(what);
    for (int64_t i = 0; i < n; ++i) {
        const size_t at = (size_t)i * capacity;
        hits[i].reset();
        if (!candidates_settle(count[i], needsHost ? needsHost + i : nullptr, what, fail)) continue;
        const Ray ray = ray_of(rays[i]);
        float tMax = rays[i].tmax;
        auto test = [&](int j) {  // a hit replaces the result and sets tMax (aggregates.cpp:529-579, :1033-1049)
            if (std::optional<HostHit> hh = hostIntersect(prim[at + j], inst[at + j], ray, tMax)) {
                hits[i] = ResolvedHit{HitRecord{prim[at + j], hh->tHit, hh->b0, hh->b1, hh->b2, inst[at + j]}, true};
                tMax = hh->tHit;
            }
        };
        for (int j = 0; j < before[i]; ++j) test(j);
        const nnbvh_hit &h = rec[(size_t)i];
        if (h.prim >= 0) {
            // after a candidate's hit: accepted iff t <= tMax (triangle) / t < tMax (patch), include/nnbvh.h
            const bool patch = std::binary_search(patchIds.begin(), patchIds.end(), h.prim);
            if (!hits[i] || (patch ? h.t < tMax : h.t <= tMax)) {
                hits[i] = ResolvedHit{HitRecord{h.prim, h.t, h.b0, h.b1, h.b2, h.instance}, false};
                tMax = h.t;
            }
        }
        for (int j = before[i]; j < count[i]; ++j) test(j);
    }
}

template <typename Trace, typename F, typename Fail>
void resolve_shadow(Trace &&trace, const nnbvh_ray *rays, int64_t n, uint8_t *occluded, F &&hostIntersect,
                    uint8_t *needsHost, int capacity, const char *what, Fail &&fail) {
    std::vector<int32_t> count((size_t)n), prim((size_t)n * capacity), inst((size_t)n * capacity);
    nnbvh_host_candidates c{capacity, count.data(), nullptr, prim.data(), inst.data()};
    if (trace(rays, n, occluded, &c) != NNBVH_OK) fail(what);
    for (int64_t i = 0; i < n; ++i) {
        if (needsHost) needsHost[i] = 0;
        if (occluded[i] != 2) continue;
        occluded[i] = 0;
        if (!candidates_settle(count[i], needsHost ? needsHost + i : nullptr, what, fail)) continue;
        const Ray ray = ray_of(rays[i]);
        for (int j = 0; j < count[i] && !occluded[i]; ++j)
            occluded[i] = hostIntersect(prim[(size_t)i * capacity + j], inst[(size_t)i * capacity + j], ray,
                                        rays[i].tmax).has_value();
    }
}
}  // namespace detail

class HipBVHAggregate {
  public:
    using FatalHandler = void (*)(const char *);
    static FatalHandler &fatal_handler() {
        static FatalHandler h = [](const char *msg) {
            std::fprintf(stderr, "nnbvh: fatal: %s\n", msg);
            std::abort();
        };
        return h;
    }
    static void fatal(const std::string &what) {
        fatal_handler()((what + ": " + nnbvh_last_error()).c_str());
    }

    // == BVHAggregate::Create / ctor (aggregates.cpp:725-744, 140-190): builds on the host.
    // splitMethod: "sah" (default) | "middle" | "equal"; maxPrimsInNode default 4.
    // primBounds: 6 floats (min, max) per primitive, read for NNBVH_PRIM_HOST / NNBVH_PRIM_INSTANCE entries
    // (what Primitive::Bounds() returns for them); may be null when the list holds neither
    // normals: the meshes' per-vertex normals (3 floats per vertex), read for the smooth alpha-tested kinds;
    // primAlpha: one constant alpha per entry of `prims`, read for the alpha-tested bilinear patches; uvs: per-vertex
    // (u, v), read for the alpha-tested patches of meshes with uv
    HipBVHAggregate(const std::vector<nnbvh_prim> &prims, const std::vector<float> &verts,
                    int maxPrimsInNode = 4, const std::string &splitMethod = "sah", int device = 0,
                    const std::vector<float> *primBounds = nullptr, const std::vector<float> *normals = nullptr,
                    const std::vector<float> *primAlpha = nullptr, const std::vector<float> *uvs = nullptr) {
        int method = splitMethod == "sah"      ? NNBVH_SPLIT_SAH
                     : splitMethod == "middle" ? NNBVH_SPLIT_MIDDLE
                     : splitMethod == "equal"  ? NNBVH_SPLIT_EQUAL_COUNTS
                     : splitMethod == "hlbvh"  ? NNBVH_SPLIT_HLBVH
                                               : -1;
        // the builder reorders the primitives; with a per-primitive array to carry along, build with the
        // position as the id and put the caller's ids back afterwards
        std::vector<nnbvh_prim> tagged;
        if (primAlpha) {
            tagged = prims;
            for (size_t i = 0; i < tagged.size(); ++i) tagged[i].id = (int32_t)i;
        }
        note_patches(prims.data(), (int)prims.size());
        const nnbvh_prim *in = primAlpha ? tagged.data() : prims.data();
        nnbvh_build *b = primBounds
                             ? nnbvh_build_create_with_bounds(in, (int)prims.size(), verts.data(),
                                                              (int)(verts.size() / 3), primBounds->data(),
                                                              maxPrimsInNode, method)
                             : nnbvh_build_create(in, (int)prims.size(), verts.data(),
                                                  (int)(verts.size() / 3), maxPrimsInNode, method);
        if (!b) {
            fatal("HipBVHAggregate: build");
            return;
        }
        int nNodes = 0, nPrims = 0;
        const nnbvh_linear_node *nodes = nnbvh_build_nodes(b, &nNodes);
        const nnbvh_prim *ordered = nnbvh_build_ordered_prims(b, &nPrims);
        std::vector<nnbvh_prim> restored;
        std::vector<float> alphaOrdered;
        if (primAlpha) {
            restored.assign(ordered, ordered + nPrims);
            alphaOrdered.resize((size_t)nPrims);
            for (int i = 0; i < nPrims; ++i) {
                const size_t from = (size_t)restored[(size_t)i].id;
                alphaOrdered[(size_t)i] = (*primAlpha)[from];
                restored[(size_t)i].id = prims[from].id;
            }
            ordered = restored.data();
        }
        scene_ = (normals || primAlpha || uvs)
                     ? nnbvh_scene_create_with_attributes(nodes, nNodes, ordered, nPrims, verts.data(),
                                                          normals ? normals->data() : nullptr,
                                                          uvs ? uvs->data() : nullptr,
                                                          primAlpha ? alphaOrdered.data() : nullptr,
                                                          (int)(verts.size() / 3), device)
                     : nnbvh_scene_create(nodes, nNodes, ordered, nPrims, verts.data(), (int)(verts.size() / 3), device);
        nnbvh_build_destroy(b);
        if (!scene_) fatal("HipBVHAggregate: scene_create");
    }

    // from a tree pbrt itself built: BVHAggregate::nodes + the leaf-ordered primitives
    // (normals as above; primAlpha indexed like orderedPrims)
    HipBVHAggregate(const nnbvh_linear_node *nodes, int nNodes, const nnbvh_prim *orderedPrims,
                    int nPrims, const float *verts, int nVerts, int device = 0, const float *normals = nullptr,
                    const float *primAlpha = nullptr, const float *uvs = nullptr) {
        scene_ = (normals || primAlpha || uvs)
                     ? nnbvh_scene_create_with_attributes(nodes, nNodes, orderedPrims, nPrims, verts, normals, uvs,
                                                          primAlpha, nVerts, device)
                     : nnbvh_scene_create(nodes, nNodes, orderedPrims, nPrims, verts, nVerts, device);
        if (!scene_) fatal("HipBVHAggregate: scene_create");
        note_patches(orderedPrims, nPrims);
    }

    // ... whose primitives include triangles with an image-textured alpha (kinds NNBVH_PRIM_ALPHATEX_TRIANGLE*, v[3] =
    // index into alphaTextures; nnbvh_scene_create_with_alpha_textures).  uvs == nullptr: the meshes have no (u, v)
    // and every textured triangle takes the default corners.  The texels are copied
    HipBVHAggregate(const nnbvh_linear_node *nodes, int nNodes, const nnbvh_prim *orderedPrims, int nPrims,
                    const float *verts, int nVerts, const std::vector<nnbvh_alpha_texture> &alphaTextures, int device = 0,
                    const float *normals = nullptr, const float *primAlpha = nullptr, const float *uvs = nullptr) {
        scene_ = nnbvh_scene_create_with_alpha_textures(nodes, nNodes, orderedPrims, nPrims, verts, normals, uvs, primAlpha,
                                                        nVerts, device, alphaTextures.data(), (int)alphaTextures.size());
        if (!scene_) fatal("HipBVHAggregate: scene_create_with_alpha_textures");
        note_patches(orderedPrims, nPrims);
    }

    // ... and a TWO-LEVEL scene of host-built trees with such triangles, in object definitions or in the top-level list
    // (nnbvh_scene_create_instanced_with_alpha_textures): nodes[0, nTopNodes) is the top-level tree, the child trees
    // follow; animated (nullable) has one entry per instance.  Inside an instance the texture is evaluated on the
    // instance-space ray.  Alpha-tested patches may share the scene
    HipBVHAggregate(const nnbvh_linear_node *nodes, int nNodes, int nTopNodes, const nnbvh_prim *orderedPrims, int nPrims,
                    const float *verts, int nVerts, const std::vector<nnbvh_instance> &instances,
                    const std::vector<nnbvh_alpha_texture> &alphaTextures, int device = 0,
                    const nnbvh_animated_transform *animated = nullptr, const float *normals = nullptr,
                    const float *primAlpha = nullptr, const float *uvs = nullptr) {
        scene_ = nnbvh_scene_create_instanced_with_alpha_textures(
            nodes, nNodes, nTopNodes, orderedPrims, nPrims, verts, nVerts, instances.data(), (int)instances.size(), animated,
            normals, uvs, primAlpha, device, alphaTextures.data(), (int)alphaTextures.size());
        if (!scene_) fatal("HipBVHAggregate: scene_create_instanced_with_alpha_textures");
        note_patches(orderedPrims, nPrims);
    }

    // A flat scene with its tree built AND baked on the device (nnbvh_scene_create_gpu_build_with_attributes; with
    // alphaTextures: nnbvh_scene_create_gpu_build_with_alpha_textures, for the kinds NNBVH_PRIM_ALPHATEX_TRIANGLE*).
    // primAlpha: per entry of `prims`, the caller's order.  splitMethod "sah" or "hlbvh".
    static std::unique_ptr<HipBVHAggregate> BuildOnDevice(
        const std::vector<nnbvh_prim> &prims, const std::vector<float> &verts, int maxPrimsInNode = 4,
        const std::string &splitMethod = "sah", int device = 0, const std::vector<float> *primBounds = nullptr,
        const std::vector<float> *normals = nullptr, const std::vector<float> *primAlpha = nullptr,
        const std::vector<float> *uvs = nullptr, const std::vector<nnbvh_alpha_texture> *alphaTextures = nullptr) {
        const int method = splitMethod == "sah" ? NNBVH_SPLIT_SAH : splitMethod == "hlbvh" ? NNBVH_SPLIT_HLBVH : -1;
        const float *pb = primBounds ? primBounds->data() : nullptr, *nrm = normals ? normals->data() : nullptr;
        const float *uv = uvs ? uvs->data() : nullptr, *pa = primAlpha ? primAlpha->data() : nullptr;
        nnbvh_scene *scene =
            alphaTextures
                ? nnbvh_scene_create_gpu_build_with_alpha_textures(prims.data(), (int)prims.size(), verts.data(),
                                                                   (int)(verts.size() / 3), pb, nrm, uv, pa, maxPrimsInNode,
                                                                   method, device, alphaTextures->data(),
                                                                   (int)alphaTextures->size())
                : nnbvh_scene_create_gpu_build_with_attributes(prims.data(), (int)prims.size(), verts.data(),
                                                               (int)(verts.size() / 3), pb, nrm, uv, pa, maxPrimsInNode,
                                                               method, device);
        if (!scene) {
            fatal("HipBVHAggregate::BuildOnDevice");
            return nullptr;
        }
        std::unique_ptr<HipBVHAggregate> agg(new HipBVHAggregate(scene));
        agg->note_patches(prims.data(), (int)prims.size());
        return agg;
    }

    // A two-level scene (one BVHAggregate per object definition, one TransformedPrimitive / AnimatedPrimitive per
    // placement, scene.cpp:1521-1577) with every tree built AND baked on the device
    // (nnbvh_scene_create_instanced_gpu_build): the scene of host-built trees, byte for byte.  topPrims: what lives
    // directly in the top-level tree (may be empty); one instance entry per placement is generated behind them (kind
    // NNBVH_PRIM_INSTANCE, v[0] = j, id = topPrims.size() + j).  primBounds / primAlpha: per entry of the list
    // [topPrims, the generated instance entries, objects[0], objects[1], ...]; primBounds is read for host-only
    // entries and the instances of animated placements only.  splitMethod "sah" or "hlbvh".  alphaTextures: the table
    // of the kinds NNBVH_PRIM_ALPHATEX_TRIANGLE* (nnbvh_scene_create_instanced_gpu_build_with_alpha_textures).
    static std::unique_ptr<HipBVHAggregate> BuildTwoLevelOnDevice(
        const std::vector<nnbvh_prim> &topPrims, const std::vector<float> &verts,
        const std::vector<std::vector<nnbvh_prim>> &objects, const std::vector<nnbvh_placement> &placements,
        int maxPrimsInNode = 4, const std::string &splitMethod = "sah", int device = 0,
        const std::vector<nnbvh_animated_transform> *animated = nullptr, const std::vector<float> *primBounds = nullptr,
        const std::vector<float> *normals = nullptr, const std::vector<float> *primAlpha = nullptr,
        const std::vector<float> *uvs = nullptr, const std::vector<nnbvh_alpha_texture> *alphaTextures = nullptr) {
        std::vector<nnbvh_prim> prims(topPrims);
        for (size_t j = 0; j < placements.size(); ++j)
            prims.push_back(nnbvh_prim{NNBVH_PRIM_INSTANCE, (int32_t)(topPrims.size() + j), {(int32_t)j, 0, 0, 0}});
        const int nTop = (int)prims.size();
        std::vector<int32_t> first{nTop};
        for (const std::vector<nnbvh_prim> &o : objects) {
            prims.insert(prims.end(), o.begin(), o.end());
            first.push_back((int32_t)prims.size());
        }
        const int method = splitMethod == "sah" ? NNBVH_SPLIT_SAH : splitMethod == "hlbvh" ? NNBVH_SPLIT_HLBVH : -1;
        const float *nrm = normals ? normals->data() : nullptr, *uv = uvs ? uvs->data() : nullptr;
        const float *pa = primAlpha ? primAlpha->data() : nullptr, *pb = primBounds ? primBounds->data() : nullptr;
        const nnbvh_animated_transform *an = animated ? animated->data() : nullptr;
        nnbvh_scene *scene =
            alphaTextures
                ? nnbvh_scene_create_instanced_gpu_build_with_alpha_textures(
                      prims.data(), (int)prims.size(), nTop, first.data(), (int)objects.size(), verts.data(),
                      (int)(verts.size() / 3), nrm, uv, pa, pb, placements.data(), (int)placements.size(), an,
                      maxPrimsInNode, method, device, alphaTextures->data(), (int)alphaTextures->size())
                : nnbvh_scene_create_instanced_gpu_build(
                      prims.data(), (int)prims.size(), nTop, first.data(), (int)objects.size(), verts.data(),
                      (int)(verts.size() / 3), nrm, uv, pa, pb, placements.data(), (int)placements.size(), an,
                      maxPrimsInNode, method, device);
        if (!scene) {
            fatal("HipBVHAggregate::BuildTwoLevelOnDevice");
            return nullptr;
        }
        std::unique_ptr<HipBVHAggregate> agg(new HipBVHAggregate(scene));
        agg->note_patches(prims.data(), (int)prims.size());
        return agg;
    }

    HipBVHAggregate(const HipBVHAggregate &) = delete;
    HipBVHAggregate &operator=(const HipBVHAggregate &) = delete;
    ~HipBVHAggregate() { nnbvh_scene_destroy(scene_); }

    // ---- Primitive interface -----------------------------------------------------------
    Bounds3f Bounds() const {
        float b[6];
        if (nnbvh_scene_bounds(scene_, b) != NNBVH_OK) fatal("Bounds");
        return {{b[0], b[1], b[2]}, {b[3], b[4], b[5]}};
    }

    std::optional<HitRecord> Intersect(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(),
                                       bool *needsHost = nullptr) const {
        nnbvh_ray r = wire(ray, tMax);
        nnbvh_hit h;
        if (nnbvh_intersect_closest(scene_, &r, 1, &h) != NNBVH_OK) fatal("Intersect");
        if (needsHost) *needsHost = h.instance == -1;
        if (h.instance == -1) {
            if (!needsHost) fatal("Intersect: the ray met a host-only primitive (pass needsHost and re-trace it on the CPU)");
            return {};
        }
        if (h.prim < 0) return {};
        return HitRecord{h.prim, h.t, h.b0, h.b1, h.b2, h.instance};
    }

    bool IntersectP(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(),
                    bool *needsHost = nullptr) const {
        nnbvh_ray r = wire(ray, tMax);
        uint8_t occ = 0;
        if (nnbvh_intersect_any(scene_, &r, 1, &occ, nullptr, nullptr) != NNBVH_OK)
            fatal("IntersectP");
        if (needsHost) *needsHost = occ == 2;
        if (occ == 2 && !needsHost)
            fatal("IntersectP: the ray met a host-only primitive (pass needsHost and re-trace it on the CPU)");
        return occ == 1;
    }

    // ---- ... with host-only primitives as candidates (no CPU aggregate needed) -----------
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    std::optional<ResolvedHit> Intersect(const Ray &ray, float tMax, F &&hostIntersect, bool *needsHost = nullptr,
                                         int capacity = 8) const {
        std::optional<ResolvedHit> out;
        uint8_t voided = 0;
        nnbvh_ray r = wire(ray, tMax);
        IntersectClosest(&r, 1, &out, hostIntersect, needsHost ? &voided : nullptr, capacity);
        if (needsHost) *needsHost = voided != 0;
        return out;
    }
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    bool IntersectP(const Ray &ray, float tMax, F &&hostIntersect, bool *needsHost = nullptr, int capacity = 8) const {
        uint8_t occ = 0, voided = 0;
        nnbvh_ray r = wire(ray, tMax);
        IntersectShadow(&r, 1, &occ, hostIntersect, needsHost ? &voided : nullptr, capacity);
        if (needsHost) *needsHost = voided != 0;
        return occ != 0;
    }
    // batches (host buffers; synchronous).  needsHost (nullable, uint8_t[n]): 1 for a ray the candidates cannot
    // settle (its hits[i] / occluded[i] is then empty / 0); without it such a ray is fatal
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    void IntersectClosest(const nnbvh_ray *rays, int64_t n, std::optional<ResolvedHit> *hits, F &&hostIntersect,
                          uint8_t *needsHost = nullptr, int capacity = 8) const {
        detail::resolve_closest(
            [this](const nnbvh_ray *r, int64_t k, nnbvh_hit *h, const nnbvh_host_candidates *c) {
                return nnbvh_intersect_closest_candidates(scene_, r, k, h, c);
            },
            patchIds_, rays, n, hits, hostIntersect, needsHost, capacity, "IntersectClosest", [](const std::string &m) { fatal(m); });
    }
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    void IntersectShadow(const nnbvh_ray *rays, int64_t n, uint8_t *occluded, F &&hostIntersect,
                         uint8_t *needsHost = nullptr, int capacity = 8) const {
        detail::resolve_shadow(
            [this](const nnbvh_ray *r, int64_t k, uint8_t *occ, const nnbvh_host_candidates *c) {
                return nnbvh_intersect_any_candidates(scene_, r, k, occ, c);
            },
            rays, n, occluded, hostIntersect, needsHost, capacity, "IntersectShadow", [](const std::string &m) { fatal(m); });
    }

    // ---- WavefrontAggregate-shaped batches (host buffers; synchronous) -------------------
    void IntersectClosest(const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits) const {
        if (nnbvh_intersect_closest(scene_, rays, n, hits) != NNBVH_OK) fatal("IntersectClosest");
    }
    void IntersectShadow(const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                         int32_t *nodesVisited = nullptr, int32_t *primTests = nullptr) const {
        if (nnbvh_intersect_any(scene_, rays, n, occluded, nodesVisited, primTests) != NNBVH_OK)
            fatal("IntersectShadow");
    }

    // ---- device-resident batches, stream-ordered (hipStream_t as void*) ------------------
    void IntersectClosestDevice(const void *dRays, int64_t n, void *dHits, void *stream) const {
        if (nnbvh_intersect_closest_device(scene_, dRays, n, dHits, stream) != NNBVH_OK)
            fatal("IntersectClosestDevice");
    }
    void IntersectShadowDevice(const void *dRays, int64_t n, void *dOccluded, void *stream,
                               void *dNodesVisited = nullptr, void *dPrimTests = nullptr) const {
        if (nnbvh_intersect_any_device(scene_, dRays, n, dOccluded, dNodesVisited, dPrimTests,
                                       stream) != NNBVH_OK)
            fatal("IntersectShadowDevice");
    }

    // ---- whole wavefront stages on the device: the SOA queue in, the reference's destination
    //      queues (as index queues) and pixel radiance out; see include/nnbvh.h --------------
    // == WavefrontAggregate::IntersectClosest (wavefront/integrator.h:37-43)
    void IntersectClosestQueues(int maxRays, const nnbvh_ray_soa &rayQueue, const int32_t *dSize,
                                const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                const nnbvh_closest_queues &out, void *stream) const {
        if (nnbvh_wavefront_intersect_closest(scene_, maxRays, &rayQueue, dSize, dPrimClass,
                                              nPrimClass, dHits, &out, stream) != NNBVH_OK)
            fatal("IntersectClosestQueues");
    }
    // == WavefrontAggregate::IntersectShadow (wavefront/integrator.h:45-46)
    void IntersectShadowQueue(int maxRays, const nnbvh_ray_soa &shadowQueue, const int32_t *dSize,
                              const float *dLd, const float *dRu, const float *dRl,
                              const int32_t *dPixelIndex, float *dL, int64_t nPixels,
                              void *stream, uint8_t *dOccluded = nullptr) const {
        if (nnbvh_wavefront_intersect_shadow(scene_, maxRays, &shadowQueue, dSize, dLd, dRu, dRl,
                                             dPixelIndex, dL, nPixels, dOccluded, stream) != NNBVH_OK)
            fatal("IntersectShadowQueue");
    }

    // == IntersectShadow of one depth + IntersectClosest of the next (the render loop issues them back to back,
    //    wavefront/integrator.cpp) in ONE launch of the traversal kernel; same results as the two calls
    void IntersectClosestAndShadowQueues(int maxRays, const nnbvh_ray_soa &rayQueue, const int32_t *dSize,
                                         const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                         const nnbvh_closest_queues &out, int maxShadowRays,
                                         const nnbvh_ray_soa &shadowQueue, const int32_t *dShadowSize, const float *dLd,
                                         const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL,
                                         int64_t nPixels, void *stream, uint8_t *dOccluded = nullptr) const {
        if (nnbvh_wavefront_intersect_closest_and_shadow(scene_, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass, dHits,
                                                         &out, maxShadowRays, &shadowQueue, dShadowSize, dLd, dRu, dRl,
                                                         dPixelIndex, dL, nPixels, dOccluded, stream) != NNBVH_OK)
            fatal("IntersectClosestAndShadowQueues");
    }

    // == IntersectClosest / IntersectClosestAndShadow with the work items themselves: next to each index the
    //    SOA payload the reference's Push stores (MaterialEvalWorkItem, HitAreaLightWorkItem, MediumSampleWorkItem,
    //    the spawned ray), computed from `mesh`; dHits may be null (include/nnbvh.h)
    void IntersectClosestItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                     const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                     const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                     void *stream) const {
        if (nnbvh_wavefront_intersect_closest_items(scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass,
                                                    dHits, &out, &items, stream) != NNBVH_OK)
            fatal("IntersectClosestItemsQueues");
    }
    void IntersectClosestAndShadowItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                              const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass,
                                              void *dHits, const nnbvh_closest_queues &out,
                                              const nnbvh_closest_items &items, int maxShadowRays,
                                              const nnbvh_ray_soa &shadowQueue, const int32_t *dShadowSize,
                                              const float *dLd, const float *dRu, const float *dRl,
                                              const int32_t *dPixelIndex, float *dL, int64_t nPixels, void *stream,
                                              uint8_t *dOccluded = nullptr) const {
        if (nnbvh_wavefront_intersect_closest_and_shadow_items(scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass,
                                                               nPrimClass, dHits, &out, &items, maxShadowRays,
                                                               &shadowQueue, dShadowSize, dLd, dRu, dRl, dPixelIndex,
                                                               dL, nPixels, dOccluded, stream) != NNBVH_OK)
            fatal("IntersectClosestAndShadowItemsQueues");
    }

    // == one wavefront iteration's independent queues as ONE launch (include/nnbvh.h)
    void TraceBatchesDevice(const nnbvh_batch *batches, int nBatches, void *stream) const {
        if (nnbvh_trace_batches_device(scene_, batches, nBatches, stream) != NNBVH_OK)
            fatal("TraceBatchesDevice");
    }
    // ... with host candidates per batch (cands[b].capacity == 0: a plain batch)
    void TraceBatchesDevice(const nnbvh_batch *batches, int nBatches, const nnbvh_host_candidates *cands,
                            void *stream) const {
        if (nnbvh_trace_batches_candidates_device(scene_, batches, nBatches, cands, stream) != NNBVH_OK)
            fatal("TraceBatchesDevice (candidates)");
    }

    // ---- the wavefront stages with host candidates (include/nnbvh.h "the wavefront calls with host candidates"):
    //      rays that reached a host-only primitive come back in items.needs_host with their candidate-mode record in
    //      dHits and their candidate list in `c` (device arrays); the embedder tests those shapes, writes the merged
    //      records back and pushes the rays with EnqueueClosestItemsIndexed
    void IntersectClosestItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                     const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                     const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                     const nnbvh_host_candidates &c, void *stream) const {
        if (nnbvh_wavefront_intersect_closest_items_candidates(scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass,
                                                               nPrimClass, dHits, &out, &items, &c, stream) != NNBVH_OK)
            fatal("IntersectClosestItemsQueues (candidates)");
    }
    static void EnqueueClosestItemsIndexed(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                           const int32_t *dIndex, const int32_t *dIndexSize, int maxIndex,
                                           const void *dHits, const uint8_t *dPrimClass, int64_t nPrimClass,
                                           const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                           void *stream) {
        if (nnbvh_wavefront_enqueue_closest_items_indexed_device(mesh, maxRays, &rayQueue, dIndex, dIndexSize, maxIndex,
                                                                 dHits, dPrimClass, nPrimClass, &out, &items,
                                                                 stream) != NNBVH_OK)
            fatal("EnqueueClosestItemsIndexed");
    }
    // dOccluded (required): 0 recorded, 1 occluded, 2 = test the candidates, then RecordShadow with an array that is 1
    // everywhere but on the rays resolved as unoccluded
    void IntersectShadowQueue(int maxRays, const nnbvh_ray_soa &shadowQueue, const int32_t *dSize, const float *dLd,
                              const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL,
                              int64_t nPixels, void *stream, uint8_t *dOccluded, const nnbvh_host_candidates &c) const {
        if (nnbvh_wavefront_intersect_shadow_candidates(scene_, maxRays, &shadowQueue, dSize, dLd, dRu, dRl, dPixelIndex,
                                                        dL, nPixels, dOccluded, &c, stream) != NNBVH_OK)
            fatal("IntersectShadowQueue (candidates)");
    }
    static void RecordShadow(const uint8_t *dOccluded, int maxRays, const int32_t *dSize, const float *dLd,
                             const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL, int64_t nPixels,
                             int device, void *stream) {
        if (nnbvh_wavefront_record_shadow_device(dOccluded, maxRays, dSize, dLd, dRu, dRl, dPixelIndex, dL, nPixels,
                                                 device, stream) != NNBVH_OK)
            fatal("RecordShadow");
    }
    void IntersectClosestAndShadowItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                              const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass,
                                              void *dHits, const nnbvh_closest_queues &out,
                                              const nnbvh_closest_items &items, const nnbvh_host_candidates &c,
                                              int maxShadowRays, const nnbvh_ray_soa &shadowQueue,
                                              const int32_t *dShadowSize, const float *dLd, const float *dRu,
                                              const float *dRl, const int32_t *dPixelIndex, float *dL, int64_t nPixels,
                                              void *stream, uint8_t *dOccluded,
                                              const nnbvh_host_candidates &shadowC) const {
        if (nnbvh_wavefront_intersect_closest_and_shadow_items_candidates(
                scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass, dHits, &out, &items, &c, maxShadowRays,
                &shadowQueue, dShadowSize, dLd, dRu, dRl, dPixelIndex, dL, nPixels, dOccluded, &shadowC,
                stream) != NNBVH_OK)
            fatal("IntersectClosestAndShadowItemsQueues (candidates)");
    }
    // == WavefrontAggregate::IntersectShadowTr (wavefront/integrator.h:48-49), scenes without media
    void IntersectShadowTrQueue(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &shadowQueue,
                                const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass,
                                const float *dLd, const float *dRu, const float *dRl,
                                const int32_t *dPixelIndex, float *dL, int64_t nPixels, void *stream,
                                uint8_t *dState = nullptr) const {
        if (nnbvh_wavefront_intersect_shadow_tr(scene_, mesh, maxRays, &shadowQueue, dSize, dPrimClass,
                                                nPrimClass, dLd, dRu, dRl, dPixelIndex, dL, nPixels, dState,
                                                stream) != NNBVH_OK)
            fatal("IntersectShadowTrQueue");
    }
    // == WavefrontAggregate::IntersectOneRandom (wavefront/integrator.h:51-52)
    void IntersectOneRandomQueue(const nnbvh_shading_mesh *mesh, int maxItems, const float *dP0,
                                 const float *dP1, const int32_t *dMaterial, const int32_t *dSize,
                                 const int32_t *dPrimMaterial, int64_t nPrimMaterial, void *dSelHits,
                                 void *dSelRays, float *dReservoirPdf, void *stream,
                                 float *dWeightSum = nullptr) const {
        if (nnbvh_wavefront_intersect_one_random(scene_, mesh, maxItems, dP0, dP1, dMaterial, dSize,
                                                 dPrimMaterial, nPrimMaterial, dSelHits, dSelRays,
                                                 dReservoirPdf, dWeightSum, stream) != NNBVH_OK)
            fatal("IntersectOneRandomQueue");
    }
    // ... with at most maxPasses passes and no host round trip (hipGraph-capturable after one warm-up call):
    // rays whose walk needs more get state 2, items instance = -1; dUnfinished (nullable) receives their number
    void IntersectShadowTrBounded(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &shadowQueue,
                                  const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass,
                                  const float *dLd, const float *dRu, const float *dRl,
                                  const int32_t *dPixelIndex, float *dL, int64_t nPixels, int maxPasses,
                                  void *stream, uint8_t *dState = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_wavefront_intersect_shadow_tr_bounded(scene_, mesh, maxRays, &shadowQueue, dSize, dPrimClass,
                                                        nPrimClass, dLd, dRu, dRl, dPixelIndex, dL, nPixels, dState,
                                                        maxPasses, dUnfinished, stream) != NNBVH_OK)
            fatal("IntersectShadowTrBounded");
    }
    void IntersectOneRandomBounded(const nnbvh_shading_mesh *mesh, int maxItems, const float *dP0,
                                   const float *dP1, const int32_t *dMaterial, const int32_t *dSize,
                                   const int32_t *dPrimMaterial, int64_t nPrimMaterial, void *dSelHits,
                                   void *dSelRays, float *dReservoirPdf, int maxPasses, void *stream,
                                   float *dWeightSum = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_wavefront_intersect_one_random_bounded(scene_, mesh, maxItems, dP0, dP1, dMaterial, dSize,
                                                         dPrimMaterial, nPrimMaterial, dSelHits, dSelRays,
                                                         dReservoirPdf, dWeightSum, maxPasses, dUnfinished,
                                                         stream) != NNBVH_OK)
            fatal("IntersectOneRandomBounded");
    }
    // ... walked inside ONE trace launch (nnbvh_wavefront_walk_*): the same arguments and outputs with maxSurfaces
    // (1..65536 Intersect calls per item) for maxPasses; five kernel nodes whatever the bound, hipGraph-capturable after
    // one warm-up call.  Not for scenes with AnimatedPrimitive instances or alpha-tested primitives (fatal)
    void WalkShadowTr(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &shadowQueue,
                      const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass, const float *dLd,
                      const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL, int64_t nPixels,
                      int maxSurfaces, void *stream, uint8_t *dState = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_wavefront_walk_shadow_tr(scene_, mesh, maxRays, &shadowQueue, dSize, dPrimClass, nPrimClass, dLd, dRu,
                                           dRl, dPixelIndex, dL, nPixels, dState, maxSurfaces, dUnfinished,
                                           stream) != NNBVH_OK)
            fatal("WalkShadowTr");
    }
    void WalkOneRandom(const nnbvh_shading_mesh *mesh, int maxItems, const float *dP0, const float *dP1,
                       const int32_t *dMaterial, const int32_t *dSize, const int32_t *dPrimMaterial,
                       int64_t nPrimMaterial, void *dSelHits, void *dSelRays, float *dReservoirPdf, int maxSurfaces,
                       void *stream, float *dWeightSum = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_wavefront_walk_one_random(scene_, mesh, maxItems, dP0, dP1, dMaterial, dSize, dPrimMaterial,
                                            nPrimMaterial, dSelHits, dSelRays, dReservoirPdf, dWeightSum, maxSurfaces,
                                            dUnfinished, stream) != NNBVH_OK)
            fatal("WalkOneRandom");
    }

    nnbvh_scene *handle() const { return scene_; }

  private:
    explicit HipBVHAggregate(nnbvh_scene *scene) : scene_(scene) {}
    static nnbvh_ray wire(const Ray &ray, float tMax) {
        return nnbvh_ray{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
    }
    void note_patches(const nnbvh_prim *prims, int n) { detail::note_patch_ids(patchIds_, prims, n); }
    nnbvh_scene *scene_ = nullptr;
    std::vector<int32_t> patchIds_;
};

// Triangle:: / BilinearPatch::InteractionFromIntersection (shapes.h:884-1010, 1396-1489) for batches of hit records: the mesh
// side of a pbrt scene (TriangleMesh arrays flattened over all meshes) + the post-pass.
class HipShadingMesh {
  public:
    HipShadingMesh(const float *verts, int nVerts, const int32_t *triVertices, int nPrims,
                   const float *normals = nullptr, const float *uvs = nullptr,
                   const float *tangents = nullptr, const int32_t *faceIndices = nullptr,
                   const uint8_t *triFlags = nullptr, int device = 0,
                   const int32_t *patchVertices = nullptr)
        : mesh_(nnbvh_shading_mesh_create(verts, nVerts, triVertices, patchVertices, nPrims, normals,
                                          uvs, tangents, faceIndices, triFlags, device)) {
        if (!mesh_) HipBVHAggregate::fatal("HipShadingMesh");
    }
    ~HipShadingMesh() { nnbvh_shading_mesh_destroy(mesh_); }
    HipShadingMesh(const HipShadingMesh &) = delete;
    HipShadingMesh &operator=(const HipShadingMesh &) = delete;

    void Interactions(const nnbvh_ray *rays, const nnbvh_hit *hits, int32_t n, nnbvh_interaction *out) const {
        if (nnbvh_triangle_interactions(mesh_, rays, hits, n, out) != NNBVH_OK)
            HipBVHAggregate::fatal("Interactions");
    }
    // rays either as records (dRays) or as the wavefront SOA queue (raySoa); stream-ordered
    void InteractionsDevice(const void *dRays, const nnbvh_ray_soa *raySoa, const void *dHits,
                            int32_t maxItems, const int32_t *dSize, void *dOut, void *stream) const {
        if (nnbvh_triangle_interactions_device(mesh_, dRays, raySoa, dHits, maxItems, dSize, dOut,
                                               stream) != NNBVH_OK)
            HipBVHAggregate::fatal("InteractionsDevice");
    }

    nnbvh_shading_mesh *handle() const { return mesh_; }

  private:
    nnbvh_shading_mesh *mesh_ = nullptr;
};

// KdTreeAggregate (cpu/aggregates.h:75-105): Create's parameters (aggregates.cpp:1152-1161) and the
// Primitive-shaped methods; batches as for HipBVHAggregate.
class HipKdTreeAggregate {
  public:
    // Builds on the HOST (nnbvh_kd_build_create): primitives inside multi-primitive leaves in libstdc++'s std::sort
    // order — the constructor that reproduces the tree of a libstdc++ build of the reference exactly.  BuildOnDevice
    // below is the fast route (crown: seconds here, a fraction of a second there).
    HipKdTreeAggregate(const std::vector<nnbvh_prim> &prims, const std::vector<float> &verts,
                       int isectCost = 5, int traversalCost = 1, float emptyBonus = 0.5f, int maxPrims = 1,
                       int maxDepth = -1, int device = 0, const std::vector<float> *primBounds = nullptr,
                       const std::vector<float> *normals = nullptr, const std::vector<float> *uvs = nullptr,
                       const std::vector<float> *primAlpha = nullptr) {
        nnbvh_kd_build *b = nnbvh_kd_build_create(prims.data(), (int)prims.size(), verts.data(),
                                                  (int)(verts.size() / 3), primBounds ? primBounds->data() : nullptr,
                                                  isectCost, traversalCost, emptyBonus, maxPrims, maxDepth);
        if (!b) {
            HipBVHAggregate::fatal("HipKdTreeAggregate: build");
            return;
        }
        int nNodes = 0, nIdx = 0;
        const nnbvh_kd_node *nodes = nnbvh_kd_build_nodes(b, &nNodes);
        const int32_t *idx = nnbvh_kd_build_prim_indices(b, &nIdx);
        nnbvh_kd_build_bounds(b, bounds_);
        // (kd primitives stay in the caller's order: the attribute arrays pass through as they are)
        scene_ = nnbvh_kd_scene_create_with_attributes(nodes, nNodes, idx, nIdx, prims.data(), (int)prims.size(),
                                                       verts.data(), (int)(verts.size() / 3), bounds_,
                                                       normals ? normals->data() : nullptr, uvs ? uvs->data() : nullptr,
                                                       primAlpha ? primAlpha->data() : nullptr, device);
        nnbvh_kd_build_destroy(b);
        if (!scene_) HipBVHAggregate::fatal("HipKdTreeAggregate: scene_create");
        note_patches(prims.data(), (int)prims.size());
    }
    // from a tree pbrt itself built: KdTreeAggregate::nodes, primitiveIndices, primitives, bounds
    HipKdTreeAggregate(const nnbvh_kd_node *nodes, int nNodes, const int32_t *primIndices, int nIndices,
                       const nnbvh_prim *prims, int nPrims, const float *verts, int nVerts,
                       const float boundsMinMax[6], int device = 0, const float *normals = nullptr,
                       const float *uvs = nullptr, const float *primAlpha = nullptr) {
        for (int k = 0; k < 6; ++k) bounds_[k] = boundsMinMax[k];
        scene_ = nnbvh_kd_scene_create_with_attributes(nodes, nNodes, primIndices, nIndices, prims, nPrims, verts, nVerts,
                                                       boundsMinMax, normals, uvs, primAlpha, device);
        if (!scene_) HipBVHAggregate::fatal("HipKdTreeAggregate: scene_create");
        note_patches(prims, nPrims);
    }
    // ... whose primitives include triangles with an image-textured alpha (kinds NNBVH_PRIM_ALPHATEX_TRIANGLE*, v[3] =
    // index into alphaTextures; nnbvh_kd_scene_create_with_alpha_textures).  uvs == nullptr: the meshes have no (u, v)
    // and every textured triangle takes the default corners.  The texels are copied
    HipKdTreeAggregate(const nnbvh_kd_node *nodes, int nNodes, const int32_t *primIndices, int nIndices,
                       const nnbvh_prim *prims, int nPrims, const float *verts, int nVerts, const float boundsMinMax[6],
                       const std::vector<nnbvh_alpha_texture> &alphaTextures, int device = 0,
                       const float *normals = nullptr, const float *uvs = nullptr, const float *primAlpha = nullptr) {
        for (int k = 0; k < 6; ++k) bounds_[k] = boundsMinMax[k];
        scene_ = nnbvh_kd_scene_create_with_alpha_textures(nodes, nNodes, primIndices, nIndices, prims, nPrims, verts,
                                                           nVerts, boundsMinMax, normals, uvs, primAlpha, device,
                                                           alphaTextures.data(), (int)alphaTextures.size());
        if (!scene_) HipBVHAggregate::fatal("HipKdTreeAggregate: scene_create_with_alpha_textures");
        note_patches(prims, nPrims);
    }
    // Bounds, tree and primitive records made on the device (nnbvh_kd_scene_create_gpu_build_with_attributes): the
    // same nodes as the building constructor's, with the primitives inside multi-primitive leaves in std::stable_sort
    // order (the scene of nnbvh_kd_build_create_stable + the from-tree constructor, byte for byte).
    static std::unique_ptr<HipKdTreeAggregate> BuildOnDevice(
        const std::vector<nnbvh_prim> &prims, const std::vector<float> &verts, int isectCost = 5, int traversalCost = 1,
        float emptyBonus = 0.5f, int maxPrims = 1, int maxDepth = -1, int device = 0,
        const std::vector<float> *primBounds = nullptr, const std::vector<float> *normals = nullptr,
        const std::vector<float> *uvs = nullptr, const std::vector<float> *primAlpha = nullptr) {
        nnbvh_kd_scene *scene = nnbvh_kd_scene_create_gpu_build_with_attributes(
            prims.data(), (int)prims.size(), verts.data(), (int)(verts.size() / 3),
            primBounds ? primBounds->data() : nullptr, normals ? normals->data() : nullptr, uvs ? uvs->data() : nullptr,
            primAlpha ? primAlpha->data() : nullptr, isectCost, traversalCost, emptyBonus, maxPrims, maxDepth, device);
        if (!scene) {
            HipBVHAggregate::fatal("HipKdTreeAggregate::BuildOnDevice");
            return nullptr;
        }
        std::unique_ptr<HipKdTreeAggregate> agg(new HipKdTreeAggregate(scene));
        agg->note_patches(prims.data(), (int)prims.size());
        return agg;
    }
    // ... with the alpha-texture table of the kinds NNBVH_PRIM_ALPHATEX_TRIANGLE*
    // (nnbvh_kd_scene_create_gpu_build_with_alpha_textures): the scene of nnbvh_kd_build_create_stable + the from-tree
    // constructor with alphaTextures, byte for byte
    static std::unique_ptr<HipKdTreeAggregate> BuildOnDevice(
        const std::vector<nnbvh_prim> &prims, const std::vector<float> &verts,
        const std::vector<nnbvh_alpha_texture> &alphaTextures, int isectCost = 5, int traversalCost = 1,
        float emptyBonus = 0.5f, int maxPrims = 1, int maxDepth = -1, int device = 0,
        const std::vector<float> *primBounds = nullptr, const std::vector<float> *normals = nullptr,
        const std::vector<float> *uvs = nullptr, const std::vector<float> *primAlpha = nullptr) {
        nnbvh_kd_scene *scene = nnbvh_kd_scene_create_gpu_build_with_alpha_textures(
            prims.data(), (int)prims.size(), verts.data(), (int)(verts.size() / 3),
            primBounds ? primBounds->data() : nullptr, normals ? normals->data() : nullptr, uvs ? uvs->data() : nullptr,
            primAlpha ? primAlpha->data() : nullptr, isectCost, traversalCost, emptyBonus, maxPrims, maxDepth, device,
            alphaTextures.data(), (int)alphaTextures.size());
        if (!scene) {
            HipBVHAggregate::fatal("HipKdTreeAggregate::BuildOnDevice");
            return nullptr;
        }
        std::unique_ptr<HipKdTreeAggregate> agg(new HipKdTreeAggregate(scene));
        agg->note_patches(prims.data(), (int)prims.size());
        return agg;
    }
    HipKdTreeAggregate(const HipKdTreeAggregate &) = delete;
    HipKdTreeAggregate &operator=(const HipKdTreeAggregate &) = delete;
    ~HipKdTreeAggregate() { nnbvh_kd_scene_destroy(scene_); }

    nnbvh_kd_scene *handle() const { return scene_; }

    Bounds3f Bounds() const { return {{bounds_[0], bounds_[1], bounds_[2]}, {bounds_[3], bounds_[4], bounds_[5]}}; }
    std::optional<HitRecord> Intersect(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(),
                                       bool *needsHost = nullptr) const {
        nnbvh_ray r{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
        nnbvh_hit h;
        if (nnbvh_kd_intersect_closest(scene_, &r, 1, &h) != NNBVH_OK) HipBVHAggregate::fatal("kd Intersect");
        if (needsHost) *needsHost = h.instance == -1;
        if (h.instance == -1) {  // void: a host-only primitive or an alpha re-trace hit lay on the way
            if (!needsHost) HipBVHAggregate::fatal("kd Intersect: the ray met a host-only primitive (pass needsHost)");
            return {};
        }
        if (h.prim < 0) return {};
        return HitRecord{h.prim, h.t, h.b0, h.b1, h.b2, h.instance};
    }
    bool IntersectP(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(), bool *needsHost = nullptr) const {
        nnbvh_ray r{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
        uint8_t occ = 0;
        if (nnbvh_kd_intersect_any(scene_, &r, 1, &occ, nullptr, nullptr) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectP");
        if (needsHost) *needsHost = occ == 2;
        if (occ == 2 && !needsHost) HipBVHAggregate::fatal("kd IntersectP: the ray met a host-only primitive (pass needsHost)");
        return occ == 1;
    }
    void IntersectClosest(const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits) const {
        if (nnbvh_kd_intersect_closest(scene_, rays, n, hits) != NNBVH_OK) HipBVHAggregate::fatal("kd IntersectClosest");
    }
    void IntersectShadow(const nnbvh_ray *rays, int64_t n, uint8_t *occluded, int32_t *nodesVisited = nullptr,
                         int32_t *primTests = nullptr) const {
        if (nnbvh_kd_intersect_any(scene_, rays, n, occluded, nodesVisited, primTests) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectShadow");
    }
    // ---- ... with host-only primitives as candidates: HipBVHAggregate's overloads, types and merge rule
    //      (nnbvh_kd_*_candidates; `instance` is 0 in every call of hostIntersect, a shape is asked about once per ray
    //      however many leaves hold it) ---------------------------------------------------------------------------
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    std::optional<ResolvedHit> Intersect(const Ray &ray, float tMax, F &&hostIntersect, bool *needsHost = nullptr,
                                         int capacity = 8) const {
        std::optional<ResolvedHit> out;
        uint8_t voided = 0;
        nnbvh_ray r{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
        IntersectClosest(&r, 1, &out, hostIntersect, needsHost ? &voided : nullptr, capacity);
        if (needsHost) *needsHost = voided != 0;
        return out;
    }
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    bool IntersectP(const Ray &ray, float tMax, F &&hostIntersect, bool *needsHost = nullptr, int capacity = 8) const {
        uint8_t occ = 0, voided = 0;
        nnbvh_ray r{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
        IntersectShadow(&r, 1, &occ, hostIntersect, needsHost ? &voided : nullptr, capacity);
        if (needsHost) *needsHost = voided != 0;
        return occ != 0;
    }
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    void IntersectClosest(const nnbvh_ray *rays, int64_t n, std::optional<ResolvedHit> *hits, F &&hostIntersect,
                          uint8_t *needsHost = nullptr, int capacity = 8) const {
        detail::resolve_closest(
            [this](const nnbvh_ray *r, int64_t k, nnbvh_hit *h, const nnbvh_host_candidates *c) {
                return nnbvh_kd_intersect_closest_candidates(scene_, r, k, h, c);
            },
            patchIds_, rays, n, hits, hostIntersect, needsHost, capacity, "kd IntersectClosest", [](const std::string &m) { HipBVHAggregate::fatal(m); });
    }
    template <typename F, typename = std::enable_if_t<std::is_invocable_r_v<std::optional<HostHit>, F &, int32_t,
                                                                           int32_t, const Ray &, float>>>
    void IntersectShadow(const nnbvh_ray *rays, int64_t n, uint8_t *occluded, F &&hostIntersect,
                         uint8_t *needsHost = nullptr, int capacity = 8) const {
        detail::resolve_shadow(
            [this](const nnbvh_ray *r, int64_t k, uint8_t *occ, const nnbvh_host_candidates *c) {
                return nnbvh_kd_intersect_any_candidates(scene_, r, k, occ, c);
            },
            rays, n, occluded, hostIntersect, needsHost, capacity, "kd IntersectShadow", [](const std::string &m) { HipBVHAggregate::fatal(m); });
    }
    void IntersectClosestCandidatesDevice(const void *dRays, int64_t n, void *dHits, const nnbvh_host_candidates &c,
                                          void *stream) const {
        if (nnbvh_kd_intersect_closest_candidates_device(scene_, dRays, n, dHits, &c, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestCandidatesDevice");
    }
    void IntersectShadowCandidatesDevice(const void *dRays, int64_t n, void *dOccluded, const nnbvh_host_candidates &c,
                                         void *stream) const {
        if (nnbvh_kd_intersect_any_candidates_device(scene_, dRays, n, dOccluded, &c, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectShadowCandidatesDevice");
    }
    void TraceBatchesCandidatesDevice(const nnbvh_batch *batches, int nBatches, const nnbvh_host_candidates *cands,
                                      void *stream) const {
        if (nnbvh_kd_trace_batches_candidates_device(scene_, batches, nBatches, cands, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd TraceBatchesCandidatesDevice");
    }

    void IntersectClosestDevice(const void *dRays, int64_t n, void *dHits, void *stream) const {
        if (nnbvh_kd_intersect_closest_device(scene_, dRays, n, dHits, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestDevice");
    }
    void IntersectShadowDevice(const void *dRays, int64_t n, void *dOccluded, void *stream,
                               void *dNodesVisited = nullptr, void *dPrimTests = nullptr) const {
        if (nnbvh_kd_intersect_any_device(scene_, dRays, n, dOccluded, dNodesVisited, dPrimTests, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectShadowDevice");
    }

    // ---- one-launch batches and whole wavefront stages on a kd scene: HipBVHAggregate's signatures and meanings
    //      (nnbvh_kd_trace_batches_device, nnbvh_kd_wavefront_*, include/nnbvh.h) --------------------------------
    void TraceBatchesDevice(const nnbvh_batch *batches, int nBatches, void *stream) const {
        if (nnbvh_kd_trace_batches_device(scene_, batches, nBatches, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd TraceBatchesDevice");
    }
    void IntersectClosestQueues(int maxRays, const nnbvh_ray_soa &rayQueue, const int32_t *dSize,
                                const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                const nnbvh_closest_queues &out, void *stream) const {
        if (nnbvh_kd_wavefront_intersect_closest(scene_, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass, dHits, &out,
                                                 stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestQueues");
    }
    void IntersectShadowQueues(int maxRays, const nnbvh_ray_soa &shadowQueue, const int32_t *dSize, const float *dLd,
                               const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL,
                               int64_t nPixels, void *stream, uint8_t *dOccluded = nullptr) const {
        if (nnbvh_kd_wavefront_intersect_shadow(scene_, maxRays, &shadowQueue, dSize, dLd, dRu, dRl, dPixelIndex, dL,
                                                nPixels, dOccluded, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectShadowQueues");
    }
    void IntersectShadowQueue(int maxRays, const nnbvh_ray_soa &shadowQueue, const int32_t *dSize, const float *dLd,
                              const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL,
                              int64_t nPixels, void *stream, uint8_t *dOccluded = nullptr) const {  // HipBVHAggregate's name
        IntersectShadowQueues(maxRays, shadowQueue, dSize, dLd, dRu, dRl, dPixelIndex, dL, nPixels, stream, dOccluded);
    }
    void IntersectClosestAndShadowQueues(int maxRays, const nnbvh_ray_soa &rayQueue, const int32_t *dSize,
                                         const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                         const nnbvh_closest_queues &out, int maxShadowRays,
                                         const nnbvh_ray_soa &shadowQueue, const int32_t *dShadowSize, const float *dLd,
                                         const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL,
                                         int64_t nPixels, void *stream, uint8_t *dOccluded = nullptr) const {
        if (nnbvh_kd_wavefront_intersect_closest_and_shadow(scene_, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass,
                                                            dHits, &out, maxShadowRays, &shadowQueue, dShadowSize, dLd,
                                                            dRu, dRl, dPixelIndex, dL, nPixels, dOccluded,
                                                            stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestAndShadowQueues");
    }
    void IntersectClosestItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                     const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass, void *dHits,
                                     const nnbvh_closest_queues &out, const nnbvh_closest_items &items,
                                     void *stream) const {
        if (nnbvh_kd_wavefront_intersect_closest_items(scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass, nPrimClass,
                                                       dHits, &out, &items, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestItemsQueues");
    }
    void IntersectClosestAndShadowItemsQueues(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &rayQueue,
                                              const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass,
                                              void *dHits, const nnbvh_closest_queues &out,
                                              const nnbvh_closest_items &items, int maxShadowRays,
                                              const nnbvh_ray_soa &shadowQueue, const int32_t *dShadowSize,
                                              const float *dLd, const float *dRu, const float *dRl,
                                              const int32_t *dPixelIndex, float *dL, int64_t nPixels, void *stream,
                                              uint8_t *dOccluded = nullptr) const {
        if (nnbvh_kd_wavefront_intersect_closest_and_shadow_items(scene_, mesh, maxRays, &rayQueue, dSize, dPrimClass,
                                                                  nPrimClass, dHits, &out, &items, maxShadowRays,
                                                                  &shadowQueue, dShadowSize, dLd, dRu, dRl, dPixelIndex,
                                                                  dL, nPixels, dOccluded, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd IntersectClosestAndShadowItemsQueues");
    }
    // IntersectShadowTr / IntersectOneRandom walked inside ONE trace launch (nnbvh_kd_wavefront_walk_*): the
    // arguments and outputs of HipBVHAggregate::IntersectShadowTrBounded / IntersectOneRandomBounded with
    // maxSurfaces (1..65536) for maxPasses; hipGraph-capturable after one warm-up call
    void WalkShadowTr(const nnbvh_shading_mesh *mesh, int maxRays, const nnbvh_ray_soa &shadowQueue,
                      const int32_t *dSize, const uint8_t *dPrimClass, int64_t nPrimClass, const float *dLd,
                      const float *dRu, const float *dRl, const int32_t *dPixelIndex, float *dL, int64_t nPixels,
                      int maxSurfaces, void *stream, uint8_t *dState = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_kd_wavefront_walk_shadow_tr(scene_, mesh, maxRays, &shadowQueue, dSize, dPrimClass, nPrimClass, dLd,
                                              dRu, dRl, dPixelIndex, dL, nPixels, dState, maxSurfaces, dUnfinished,
                                              stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd WalkShadowTr");
    }
    void WalkOneRandom(const nnbvh_shading_mesh *mesh, int maxItems, const float *dP0, const float *dP1,
                       const int32_t *dMaterial, const int32_t *dSize, const int32_t *dPrimMaterial,
                       int64_t nPrimMaterial, void *dSelHits, void *dSelRays, float *dReservoirPdf, int maxSurfaces,
                       void *stream, float *dWeightSum = nullptr, int32_t *dUnfinished = nullptr) const {
        if (nnbvh_kd_wavefront_walk_one_random(scene_, mesh, maxItems, dP0, dP1, dMaterial, dSize, dPrimMaterial,
                                               nPrimMaterial, dSelHits, dSelRays, dReservoirPdf, dWeightSum,
                                               maxSurfaces, dUnfinished, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("kd WalkOneRandom");
    }

  private:
    explicit HipKdTreeAggregate(nnbvh_kd_scene *scene) : scene_(scene) { nnbvh_kd_scene_bounds(scene_, bounds_); }
    void note_patches(const nnbvh_prim *prims, int n) { detail::note_patch_ids(patchIds_, prims, n); }
    nnbvh_kd_scene *scene_ = nullptr;
    std::vector<int32_t> patchIds_;
    float bounds_[6] = {0, 0, 0, 0, 0, 0};
};

// RGBFilm's pixel accumulators (film.h:232-316): AddSample as UpdateFilm calls it, read-back, and the
// pack / unpack halves of a tile all-gather.
class HipFilm {
  public:
    HipFilm(int x0, int y0, int x1, int y1, float maxComponentValue = std::numeric_limits<float>::infinity(),
            int device = 0)
        : film_(nnbvh_film_create(x0, y0, x1, y1, maxComponentValue, device)), nPixels_((int64_t)(x1 - x0) * (y1 - y0)) {
        if (!film_) HipBVHAggregate::fatal("HipFilm");
    }
    ~HipFilm() { nnbvh_film_destroy(film_); }
    HipFilm(const HipFilm &) = delete;
    HipFilm &operator=(const HipFilm &) = delete;

    void AddSamplesDevice(const int32_t *dPx, const int32_t *dPy, const float *dRgb, int rgbStride,
                          const float *dWeight, int nPerPass, int nPasses, const int32_t *dSize, void *stream) {
        if (nnbvh_film_add_samples_device(film_, dPx, dPy, dRgb, rgbStride, dWeight, nPerPass, nPasses, dSize,
                                          stream) != NNBVH_OK)
            HipBVHAggregate::fatal("HipFilm::AddSamplesDevice");
    }
    std::vector<double> Read() {  // 4 doubles per pixel: rgbSum[3], weightSum
        std::vector<double> out((size_t)nPixels_ * 4);
        if (nnbvh_film_read(film_, out.data()) != NNBVH_OK) HipBVHAggregate::fatal("HipFilm::Read");
        return out;
    }
    void PackPixelsDevice(const int32_t *dIndex, int64_t n, void *dOut, void *stream) {
        if (nnbvh_film_pack_pixels_device(film_, dIndex, n, dOut, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("HipFilm::PackPixelsDevice");
    }
    void UnpackPixelsDevice(const int32_t *dIndex, int64_t n, const void *dIn, void *stream) {
        if (nnbvh_film_unpack_pixels_device(film_, dIndex, n, dIn, stream) != NNBVH_OK)
            HipBVHAggregate::fatal("HipFilm::UnpackPixelsDevice");
    }
    nnbvh_film *handle() const { return film_; }

  private:
    nnbvh_film *film_ = nullptr;
    int64_t nPixels_ = 0;
};

// ---- per-ray calls from many threads, traced together ------------------------------------------------
// pbrt's CPU integrators call Primitive::Intersect / IntersectP once per ray from every thread of ParallelFor2D
// (cpu/integrators.cpp:152-216, 296-313).  CoalescingAggregate keeps that call shape — Intersect(ray, tMax)
// blocks and returns this ray's result — and turns the rays that are in flight at the same moment into one
// batch: a caller appends its ray to the open batch and waits; the caller that fills the batch (maxBatch) or the
// first one whose wait exceeds maxWait becomes the leader, closes the batch, traces it with one
// IntersectClosest / IntersectShadow call and wakes the others.  Rays arriving while the leader is on the GPU
// open the next batch.  Results are exactly the batched calls' (rays are independent).  A: HipBVHAggregate or
// HipKdTreeAggregate.
template <typename A>
class CoalescingAggregate {
  public:
    explicit CoalescingAggregate(const A &aggregate, size_t maxBatch = 4096,
                                 std::chrono::microseconds maxWait = std::chrono::microseconds(50))
        : agg_(aggregate), maxBatch_(maxBatch), maxWait_(maxWait) {}

    Bounds3f Bounds() const { return agg_.Bounds(); }

    std::optional<HitRecord> Intersect(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(),
                                       bool *needsHost = nullptr) {
        const nnbvh_hit h = submit(closest_, wire(ray, tMax)).hit;
        if (needsHost) *needsHost = h.instance == -1;
        if (h.instance == -1) {
            if (!needsHost) HipBVHAggregate::fatal("CoalescingAggregate::Intersect: the ray met a host-only primitive (pass needsHost)");
            return {};
        }
        if (h.prim < 0) return {};
        return HitRecord{h.prim, h.t, h.b0, h.b1, h.b2, h.instance};
    }
    bool IntersectP(const Ray &ray, float tMax = std::numeric_limits<float>::infinity(), bool *needsHost = nullptr) {
        const uint8_t occ = submit(shadow_, wire(ray, tMax)).occluded;
        if (needsHost) *needsHost = occ == 2;
        if (occ == 2 && !needsHost) HipBVHAggregate::fatal("CoalescingAggregate::IntersectP: the ray met a host-only primitive (pass needsHost)");
        return occ == 1;
    }
    // batches traced so far and the rays in them (closest + shadow)
    void Stats(uint64_t *batches, uint64_t *rays) const {
        std::lock_guard<std::mutex> lock(closest_.m);
        std::lock_guard<std::mutex> lock2(shadow_.m);
        *batches = closest_.batches + shadow_.batches;
        *rays = closest_.rays + shadow_.rays;
    }

  private:
    struct Result {
        nnbvh_hit hit;
        uint8_t occluded;
    };
    struct Batch {
        std::vector<nnbvh_ray> rays;
        std::vector<nnbvh_hit> hits;
        std::vector<uint8_t> occluded;
        bool closed = false, done = false;
    };
    struct Lane {  // one kind of query (closest hit / any hit)
        bool shadow;
        mutable std::mutex m;
        std::condition_variable cv;
        std::shared_ptr<Batch> open;
        uint64_t batches = 0, rays = 0;
    };
    static nnbvh_ray wire(const Ray &ray, float tMax) {
        return nnbvh_ray{{ray.o.x, ray.o.y, ray.o.z}, tMax, {ray.d.x, ray.d.y, ray.d.z}, ray.time};
    }
    Result submit(Lane &L, const nnbvh_ray &r) {
        std::unique_lock<std::mutex> lock(L.m);
        if (!L.open) L.open = std::make_shared<Batch>();
        std::shared_ptr<Batch> b = L.open;
        const size_t index = b->rays.size();
        b->rays.push_back(r);
        bool lead = b->rays.size() >= maxBatch_;
        if (!lead) {
            // wait to be traced by someone else; the first waiter to time out leads
            const auto deadline = std::chrono::steady_clock::now() + maxWait_;
            while (!b->done && !b->closed) {
                if (L.cv.wait_until(lock, deadline) == std::cv_status::timeout && !b->closed && !b->done) {
                    lead = true;
                    break;
                }
            }
            while (!lead && !b->done) L.cv.wait(lock);
        }
        if (lead) {
            b->closed = true;
            if (L.open == b) L.open.reset();  // later rays open the next batch
            lock.unlock();
            const int64_t n = (int64_t)b->rays.size();
            if (L.shadow) {
                b->occluded.resize((size_t)n);
                agg_.IntersectShadow(b->rays.data(), n, b->occluded.data());
            } else {
                b->hits.resize((size_t)n);
                agg_.IntersectClosest(b->rays.data(), n, b->hits.data());
            }
            lock.lock();
            b->done = true;
            L.batches += 1;
            L.rays += (uint64_t)n;
            L.cv.notify_all();
        }
        Result out{};
        if (L.shadow) out.occluded = b->occluded[index];
        else out.hit = b->hits[index];
        return out;
    }

    const A &agg_;
    size_t maxBatch_;
    std::chrono::microseconds maxWait_;
    Lane closest_{false}, shadow_{true};
};

}  // namespace nnbvh
