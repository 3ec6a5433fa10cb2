// HipKdTreeAggregate::BuildOnDevice (include/nnbvh_aggregate.hpp) as an embedder calls it: a 2 000-triangle soup goes
// in, bounds, tree and primitive records are made on the device.  Checks that closest hits and occlusion flags equal,
// bit for bit, those of the adapter's from-tree constructor fed with nnbvh_kd_build_create_stable's arrays (the
// device route's byte-for-byte host counterpart), that both scenes report the same sizes and arrays through
// nnbvh_kd_scene_info / nnbvh_kd_scene_read, and that a read with any other buffer size is refused.  Built by
// tests/test_kd_device_scene_cpp.py with g++ against libnnbvh_hip.so; run only where a GPU is present.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

#define REQUIRE(cond)                                                       \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED %s (line %d): %s\n", #cond, __LINE__, nnbvh_last_error()); \
            return 1;                                                       \
        }                                                                   \
    } while (0)

int main() {
    std::mt19937 rng(29);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int nTris = 2000, maxPrims = 2;
    std::vector<float> verts;
    std::vector<nnbvh_prim> prims;
    for (int i = 0; i < nTris; ++i) {
        const float c[3] = {5 * U(rng), 5 * U(rng), 5 * U(rng)};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts.push_back(c[a] + 0.8f * U(rng));
        prims.push_back(nnbvh_prim{NNBVH_PRIM_TRIANGLE, i, {3 * i, 3 * i + 1, 3 * i + 2, 0}});
    }
    const int nVerts = (int)(verts.size() / 3);

    auto dev = nnbvh::HipKdTreeAggregate::BuildOnDevice(prims, verts, 5, 1, 0.5f, maxPrims);
    REQUIRE(dev != nullptr);

    nnbvh_kd_build *b = nnbvh_kd_build_create_stable(prims.data(), nTris, verts.data(), nVerts, nullptr, 5, 1, 0.5f, maxPrims, -1);
    REQUIRE(b != nullptr);
    int nNodes = 0, nIdx = 0;
    const nnbvh_kd_node *nodes = nnbvh_kd_build_nodes(b, &nNodes);
    const int32_t *idx = nnbvh_kd_build_prim_indices(b, &nIdx);
    float bounds[6];
    REQUIRE(nnbvh_kd_build_bounds(b, bounds) == NNBVH_OK);
    nnbvh::HipKdTreeAggregate host(nodes, nNodes, idx, nIdx, prims.data(), nTris, verts.data(), nVerts, bounds);

    // sizes and arrays
    int64_t di[8], hi[8];
    REQUIRE(nnbvh_kd_scene_info(dev->handle(), di) == NNBVH_OK && nnbvh_kd_scene_info(host.handle(), hi) == NNBVH_OK);
    REQUIRE(std::memcmp(di, hi, sizeof di) == 0);
    REQUIRE(di[0] == nNodes && di[1] == nIdx && di[2] == nTris && di[1] > 0 && di[7] == 0);
    REQUIRE(di[4] == di[0] * 8 + di[1] * 4 + di[2] * 64);
    const size_t bytes[4] = {(size_t)nNodes * 8, (size_t)nIdx * 4, (size_t)nTris * 64, 0};
    for (int what = 0; what < 3; ++what) {
        std::vector<char> d(bytes[what]), h(bytes[what]);
        REQUIRE(nnbvh_kd_scene_read(dev->handle(), what, d.data(), d.size()) == NNBVH_OK);
        REQUIRE(nnbvh_kd_scene_read(host.handle(), what, h.data(), h.size()) == NNBVH_OK);
        REQUIRE(d == h);
        REQUIRE(nnbvh_kd_scene_read(dev->handle(), what, d.data(), d.size() - 4) == NNBVH_ERR_ARG);
        REQUIRE(nnbvh_kd_scene_read(dev->handle(), what, d.data(), d.size() + 4) == NNBVH_ERR_ARG);
    }
    {   // ... and the device route's nodes are the stable host builder's own array
        std::vector<char> d(bytes[0]);
        REQUIRE(nnbvh_kd_scene_read(dev->handle(), 0, d.data(), d.size()) == NNBVH_OK);
        REQUIRE(std::memcmp(nodes, d.data(), d.size()) == 0);
    }
    char one[4];
    REQUIRE(nnbvh_kd_scene_read(dev->handle(), 3, nullptr, 0) == NNBVH_OK);   // no attribute slots: an array of none
    REQUIRE(nnbvh_kd_scene_read(dev->handle(), 3, one, 4) == NNBVH_ERR_ARG);
    REQUIRE(nnbvh_kd_scene_read(dev->handle(), 4, one, 4) == NNBVH_ERR_ARG);
    nnbvh_kd_build_destroy(b);
    const nnbvh::Bounds3f db = dev->Bounds(), hb = host.Bounds();
    REQUIRE(std::memcmp(&db, &hb, sizeof db) == 0);

    // hits
    const int nRays = 6000;
    std::vector<nnbvh_ray> rays(nRays);
    for (auto &r : rays) {
        for (int a = 0; a < 3; ++a) {
            r.o[a] = 7 * U(rng);
            r.d[a] = 3 * U(rng) - r.o[a];
        }
        r.tmax = (&r - rays.data()) % 4 == 0 ? 0.7f : std::numeric_limits<float>::infinity();
        r.time = 0;
    }
    std::vector<nnbvh_hit> dh(nRays), hh(nRays);
    dev->IntersectClosest(rays.data(), nRays, dh.data());
    host.IntersectClosest(rays.data(), nRays, hh.data());
    REQUIRE(std::memcmp(dh.data(), hh.data(), sizeof(nnbvh_hit) * nRays) == 0);
    std::vector<uint8_t> docc(nRays), hocc(nRays);
    dev->IntersectShadow(rays.data(), nRays, docc.data());
    host.IntersectShadow(rays.data(), nRays, hocc.data());
    REQUIRE(docc == hocc);
    int nHit = 0, nOcc = 0;
    for (int i = 0; i < nRays; ++i) nHit += dh[i].prim >= 0, nOcc += docc[i] == 1;
    REQUIRE(nHit > nRays / 10 && nHit < nRays && nOcc > nRays / 20);
    std::printf("kd device scene ok: %d nodes, %d indices, %d of %d rays hit\n", nNodes, nIdx, nHit, nRays);
    return 0;
}
