// Exercises the host-candidate overloads of HipKdTreeAggregate (include/nnbvh_aggregate.hpp) the way a pbrt embedder
// without a CPU accelerator would: every 5th triangle of a soup is declared host-only (with its exact bounds, so that
// the kd-tree is the all-triangle soup's) and the embedder intersects it itself, here with the oracle's pinned
// Triangle::Intersect (oracle/nnbvh_oracle.h, linked in).  Checks that the resolved closest hits and occlusion flags
// equal those of the same soup as an all-triangle kd scene, bit for bit, that the per-ray and the batched overloads
// agree, and that host shapes do win some rays.  Built by tests/test_kd_host_candidates_cpp.py with g++ against
// libnnbvh_hip.so and libnnbvh_oracle.so; run only where a GPU is present.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

extern "C" int orc_triangle(const float o[3], const float d[3], float tmax, const float p0[3], const float p1[3],
                            const float p2[3], float out_b0b1b2t[4]);

int main() {
    std::mt19937 rng(23);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int nTris = 700;
    std::vector<float> verts, bounds;
    std::vector<nnbvh_prim> prims, asTriangles;
    for (int i = 0; i < nTris; ++i) {
        float c[3] = {5 * U(rng), 5 * U(rng), 5 * U(rng)};
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) {
                const float v = c[a] + 0.8f * U(rng);
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
    nnbvh::HipKdTreeAggregate agg(prims, verts, 5, 1, 0.5f, 2, -1, 0, &bounds);
    nnbvh::HipKdTreeAggregate plainAgg(asTriangles, verts, 5, 1, 0.5f, 2, -1, 0);

    int calls = 0;
    auto hostIntersect = [&](int32_t prim, int32_t instance, const nnbvh::Ray &r, float tMax) -> std::optional<nnbvh::HostHit> {
        ++calls;
        if (instance != 0 || prim % 5 != 2) std::abort();  // only host triangles are ever handed over, at the top level
        const float o[3] = {r.o.x, r.o.y, r.o.z}, d[3] = {r.d.x, r.d.y, r.d.z};
        float out[4];
        if (!orc_triangle(o, d, tMax, &verts[9 * prim], &verts[9 * prim + 3], &verts[9 * prim + 6], out)) return {};
        return nnbvh::HostHit{out[3], out[0], out[1], out[2]};
    };

    const int nRays = 4000;
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
    std::vector<uint8_t> occ(nRays), voided(nRays), occVoided(nRays), plainOcc(nRays);
    agg.IntersectClosest(rays.data(), nRays, batch.data(), hostIntersect, voided.data(), 16);
    agg.IntersectShadow(rays.data(), nRays, occ.data(), hostIntersect, occVoided.data(), 16);
    std::vector<nnbvh_hit> plainHits(nRays), agHits(nRays);
    plainAgg.IntersectClosest(rays.data(), nRays, plainHits.data());
    plainAgg.IntersectShadow(rays.data(), nRays, plainOcc.data());
    agg.IntersectClosest(rays.data(), nRays, agHits.data());  // today's call: -1 where a host triangle lies on the way
    int nHost = 0, nDevice = 0, nVoidToday = 0;
    for (int i = 0; i < nRays; ++i) {
        if (voided[i] || occVoided[i]) return 1;  // 16 entries hold every list of this soup
        const nnbvh_hit &e = plainHits[i];
        if ((e.prim >= 0) != batch[i].has_value()) return 2;
        if (batch[i]) {
            const nnbvh::HitRecord &h = batch[i]->hit;
            if (h.prim != e.prim || h.instance != 0 || std::memcmp(&h.tHit, &e.t, 4) || std::memcmp(&h.b0, &e.b0, 4) ||
                std::memcmp(&h.b1, &e.b1, 4) || std::memcmp(&h.b2, &e.b2, 4))
                return 3;
            if (batch[i]->host != (h.prim % 5 == 2)) return 4;
            (batch[i]->host ? nHost : nDevice) += 1;
        }
        if (occ[i] != plainOcc[i]) return 5;
        nVoidToday += agHits[i].instance == -1;
        if (i % 4 == 0) {  // the per-ray overloads
            nnbvh::Ray ray{{rays[i].o[0], rays[i].o[1], rays[i].o[2]}, {rays[i].d[0], rays[i].d[1], rays[i].d[2]}, 0};
            bool needs = true, needsP = true;
            auto one = agg.Intersect(ray, rays[i].tmax, hostIntersect, &needs, 16);
            const bool p = agg.IntersectP(ray, rays[i].tmax, hostIntersect, &needsP, 16);
            if (needs || needsP) return 6;
            if (one.has_value() != batch[i].has_value()) return 7;
            if (one && (one->host != batch[i]->host || one->hit.prim != batch[i]->hit.prim ||
                        std::memcmp(&one->hit.tHit, &batch[i]->hit.tHit, 4)))
                return 8;
            if (p != (occ[i] != 0)) return 9;
        }
    }
    if (nHost < 50 || nDevice < 200 || nVoidToday < 100 || calls == 0) {
        std::printf("too few cases: host %d device %d void today %d\n", nHost, nDevice, nVoidToday);
        return 10;
    }
    std::printf("kd host candidates ok: %d rays, %d won by host shapes, %d by device triangles, %d void without candidates\n",
                nRays, nHost, nDevice, nVoidToday);
    return 0;
}
