// Exercises the host-candidate overloads of include/nnbvh_aggregate.hpp the way a pbrt embedder without a CPU
// BVH would: every 5th triangle of a soup is declared host-only and the embedder intersects it itself (here a
// plain Moller-Trumbore test stands in for primitives[id].Intersect).  Checks that the per-ray and the batched
// overloads give the same resolved answers, that rays without candidates resolve to the plain call's record on
// the same soup as triangles, and that host shapes do win some rays.  Built by tests/test_host_candidates.py
// with g++ against libnnbvh_hip.so; run only where a GPU is present.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int nTris = 600;
    std::vector<float> verts, bounds;
    std::vector<nnbvh_prim> prims, asTriangles;
    for (int i = 0; i < nTris; ++i) {
        float c[3] = {5 * U(rng), 5 * U(rng), 5 * U(rng)};
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const float v = c[a] + 0.6f * U(rng);
                verts.push_back(v);
                lo[a] = std::fmin(lo[a], v);
                hi[a] = std::fmax(hi[a], v);
            }
        bounds.insert(bounds.end(), {lo[0], lo[1], lo[2], hi[0], hi[1], hi[2]});
        const nnbvh_prim tri{NNBVH_PRIM_TRIANGLE, i, {3 * i, 3 * i + 1, 3 * i + 2, 0}};
        asTriangles.push_back(tri);
        prims.push_back(tri);
        if (i % 5 == 2) prims.back().kind = NNBVH_PRIM_HOST;
    }
    nnbvh::HipBVHAggregate agg(prims, verts, 4, "sah", 0, &bounds);
    nnbvh::HipBVHAggregate plainAgg(asTriangles, verts);

    int calls = 0;
    auto hostIntersect = [&](int32_t prim, int32_t instance, const nnbvh::Ray &r, float tMax) -> std::optional<nnbvh::HostHit> {
        ++calls;
        if (instance != 0 || prim % 5 != 2) return {};  // only host triangles are ever handed over
        const float *p0 = &verts[9 * prim], *p1 = p0 + 3, *p2 = p0 + 6;
        const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const float d[3] = {r.d.x, r.d.y, r.d.z}, o[3] = {r.o.x, r.o.y, r.o.z};
        const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
        const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
        if (det == 0) return {};
        const float tv[3] = {o[0] - p0[0], o[1] - p0[1], o[2] - p0[2]};
        const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) / det;
        const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
        const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) / det;
        const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) / det;
        if (u < 0 || v < 0 || u + v > 1 || !(t > 0) || t > tMax) return {};
        return nnbvh::HostHit{t, 1 - u - v, u, v};
    };

    const int nRays = 3000;
    std::vector<nnbvh_ray> rays(nRays);
    for (auto &r : rays) {
        float o[3] = {6 * U(rng), 6 * U(rng), 6 * U(rng)}, t[3] = {3 * U(rng), 3 * U(rng), 3 * U(rng)};
        for (int a = 0; a < 3; ++a) {
            r.o[a] = o[a];
            r.d[a] = t[a] - o[a];
        }
        r.tmax = (&r - rays.data()) % 3 == 0 ? 0.7f : INFINITY;
        r.time = 0;
    }
    std::vector<std::optional<nnbvh::ResolvedHit>> batch(nRays);
    std::vector<uint8_t> occ(nRays), voided(nRays), occVoided(nRays);
    agg.IntersectClosest(rays.data(), nRays, batch.data(), hostIntersect, voided.data(), 16);
    agg.IntersectShadow(rays.data(), nRays, occ.data(), hostIntersect, occVoided.data(), 16);
    std::vector<nnbvh_hit> plainHits(nRays), agHits(nRays);
    plainAgg.IntersectClosest(rays.data(), nRays, plainHits.data());
    agg.IntersectClosest(rays.data(), nRays, agHits.data());  // today's call: -1 where a host triangle lies on the way
    int nHost = 0, nDevice = 0, nSame = 0;
    for (int i = 0; i < nRays; ++i) {
        if (voided[i] || occVoided[i]) return 1;
        nnbvh::Ray ray{{rays[i].o[0], rays[i].o[1], rays[i].o[2]}, {rays[i].d[0], rays[i].d[1], rays[i].d[2]}, 0};
        bool needs = true, needsP = true;
        auto one = agg.Intersect(ray, rays[i].tmax, hostIntersect, &needs, 16);
        const bool p = agg.IntersectP(ray, rays[i].tmax, hostIntersect, &needsP, 16);
        if (needs || needsP) return 2;
        if (one.has_value() != batch[i].has_value()) return 3;
        if (one && (one->host != batch[i]->host || one->hit.prim != batch[i]->hit.prim ||
                    std::memcmp(&one->hit.tHit, &batch[i]->hit.tHit, 4) || one->hit.instance != batch[i]->hit.instance))
            return 4;
        if (p != (occ[i] != 0)) return 5;
        if (one.has_value() && !p) return 6;  // a closest hit within tmax occludes
        if (one) (one->host ? nHost : nDevice) += 1;
        if (one && one->host != (one->hit.prim % 5 == 2)) return 7;
        if (agHits[i].instance != -1) {  // no candidate met: the plain record on the all-triangle twin
            const bool plainHit = plainHits[i].prim >= 0;
            if (plainHit != one.has_value()) return 8;
            if (plainHit && (one->hit.prim != plainHits[i].prim || std::memcmp(&one->hit.tHit, &plainHits[i].t, 4)))
                return 9;
            ++nSame;
        }
    }
    if (nHost < 50 || nDevice < 200 || nSame < 500 || calls == 0) {
        std::printf("too few cases: host %d device %d plain %d\n", nHost, nDevice, nSame);
        return 10;
    }
    std::printf("host candidates ok: %d rays, %d won by host shapes, %d by device triangles, %d without candidates\n",
                nRays, nHost, nDevice, nSame);
    return 0;
}
