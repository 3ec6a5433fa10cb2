// The wavefront form of the host-candidate loop through include/nnbvh_aggregate.hpp, as a pbrt embedder without a
// CPU BVH would drive it: every 5th triangle of a soup is declared host-only; one closest-hit stage is traced with
// candidates, the embedder resolves the needs_host rays with its own triangle test (a plain Moller-Trumbore test
// stands in for primitives[id].Intersect), writes the merged records back and enqueues those rays by index.  The
// union of both enqueues must route every settled ray as the plain call routes it on the same soup as triangles,
// hit or miss alike.  Built by tests/test_wavefront_candidates.py with g++ against libnnbvh_hip.so and the HIP
// runtime (device buffers); run only where a GPU is present.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

#define HIP_OK(x)                                                      \
    do {                                                               \
        if ((x) != hipSuccess) {                                       \
            std::printf("HIP call failed at line %d\n", __LINE__);     \
            return 100;                                                \
        }                                                              \
    } while (0)

template <typename T>
static T *to_device(const std::vector<T> &v) {
    T *d = nullptr;
    if (hipMalloc((void **)&d, v.size() * sizeof(T)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    return d;
}
template <typename T>
static std::vector<T> to_host(const T *d, size_t n) {
    std::vector<T> v(n);
    (void)hipMemcpy(v.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
    return v;
}

struct Queues {  // the six index queues and needs_host on the device
    int32_t *items[7], *sizes;
    int cap;
    bool init(int capacity) {
        cap = capacity;
        for (auto &p : items)
            if (hipMalloc((void **)&p, sizeof(int32_t) * capacity) != hipSuccess) return false;
        return hipMalloc((void **)&sizes, 7 * sizeof(int32_t)) == hipSuccess &&
               hipMemset(sizes, 0, 7 * sizeof(int32_t)) == hipSuccess;
    }
    nnbvh_work_queue q(int k) const { return nnbvh_work_queue{items[k], sizes + k, cap, 0}; }
    nnbvh_closest_queues out() const { return nnbvh_closest_queues{q(0), q(1), q(2), q(3), q(4), q(5)}; }
    // ray -> queue (0..5), 6 = needs_host, -1 = nowhere, -2 = pushed twice
    std::vector<int> where(int nRays, bool withHost) const {
        std::vector<int> w(nRays, -1);
        const auto n = to_host(sizes, 7);
        for (int k = 0; k < (withHost ? 7 : 6); ++k) {
            const auto idx = to_host(items[k], (size_t)n[k]);
            for (int i : idx) w[i] = w[i] == -1 ? k : -2;
        }
        return w;
    }
};

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int nTris = 600, K = 16;
    std::vector<float> verts, bounds;
    std::vector<nnbvh_prim> prims, asTriangles;
    std::vector<int32_t> triVerts;
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
        triVerts.insert(triVerts.end(), {3 * i, 3 * i + 1, 3 * i + 2});
    }
    nnbvh::HipBVHAggregate agg(prims, verts, 4, "sah", 0, &bounds);
    nnbvh::HipBVHAggregate plainAgg(asTriangles, verts);
    nnbvh::HipShadingMesh mesh(verts.data(), nTris * 3, triVerts.data(), nTris);  // holds the host triangles' vertices too

    // the embedder's own test for its shapes: hit, t and barycentrics
    auto hostIntersect = [&](int32_t prim, const nnbvh_ray &r, float tMax, nnbvh_hit &out) {
        const float *p0 = &verts[9 * prim], *p1 = p0 + 3, *p2 = p0 + 6;
        const float e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const float e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        const float *d = r.d, *o = r.o;
        const float pv[3] = {d[1] * e2[2] - d[2] * e2[1], d[2] * e2[0] - d[0] * e2[2], d[0] * e2[1] - d[1] * e2[0]};
        const float det = e1[0] * pv[0] + e1[1] * pv[1] + e1[2] * pv[2];
        if (det == 0) return false;
        const float tv[3] = {o[0] - p0[0], o[1] - p0[1], o[2] - p0[2]};
        const float u = (tv[0] * pv[0] + tv[1] * pv[1] + tv[2] * pv[2]) / det;
        const float qv[3] = {tv[1] * e1[2] - tv[2] * e1[1], tv[2] * e1[0] - tv[0] * e1[2], tv[0] * e1[1] - tv[1] * e1[0]};
        const float v = (d[0] * qv[0] + d[1] * qv[1] + d[2] * qv[2]) / det;
        const float t = (e2[0] * qv[0] + e2[1] * qv[1] + e2[2] * qv[2]) / det;
        if (u < 0 || v < 0 || u + v > 1 || !(t > 0) || t > tMax) return false;
        out.prim = prim;
        out.t = t;
        out.b0 = 1 - u - v, out.b1 = u, out.b2 = v;
        out.instance = 0;
        return true;
    };

    const int nRays = 4000;
    std::vector<float> soa[6];
    std::vector<nnbvh_ray> rays(nRays);
    for (auto &r : rays) {
        for (int a = 0; a < 3; ++a) {
            r.o[a] = 6 * U(rng);
            r.d[a] = 3 * U(rng) - r.o[a];
            soa[a].push_back(r.o[a]);
            soa[3 + a].push_back(r.d[a]);
        }
        r.tmax = INFINITY;
        r.time = 0;
    }
    float *dSoa[6];
    for (int a = 0; a < 6; ++a)
        if (!(dSoa[a] = to_device(soa[a]))) return 100;
    const nnbvh_ray_soa rq{dSoa[0], dSoa[1], dSoa[2], dSoa[3], dSoa[4], dSoa[5], nullptr, nullptr, nullptr};
    std::vector<uint8_t> cls(nTris);
    for (int i = 0; i < nTris; ++i) cls[i] = (uint8_t)(i % 3 == 0 ? NNBVH_CLASS_UNIVERSAL : (i % 7 == 0 ? NNBVH_CLASS_INTERFACE : NNBVH_CLASS_BASIC));
    uint8_t *dCls = to_device(cls);
    nnbvh_hit *dHits = nullptr, *dPlainHits = nullptr;
    HIP_OK(hipMalloc((void **)&dHits, nRays * sizeof(nnbvh_hit)));
    HIP_OK(hipMalloc((void **)&dPlainHits, nRays * sizeof(nnbvh_hit)));
    nnbvh_host_candidates c{K, nullptr, nullptr, nullptr, nullptr};
    HIP_OK(hipMalloc((void **)&c.count, nRays * 4));
    HIP_OK(hipMalloc((void **)&c.before, nRays * 4));
    HIP_OK(hipMalloc((void **)&c.prim, nRays * K * 4));
    HIP_OK(hipMalloc((void **)&c.instance, nRays * K * 4));
    Queues got, plain, fresh;
    if (!got.init(nRays) || !plain.init(nRays) || !fresh.init(nRays)) return 100;
    nnbvh_closest_items items{};  // index queues only
    items.needs_host = got.q(6);

    // 1. trace with candidates
    agg.IntersectClosestItemsQueues(mesh.handle(), nRays, rq, nullptr, dCls, nTris, dHits, got.out(), items, c, nullptr);
    HIP_OK(hipDeviceSynchronize());
    // 2. resolve the needs_host rays by the merge rule of include/nnbvh.h
    auto hits = to_host(dHits, nRays);
    const auto count = to_host(c.count, nRays), before = to_host(c.before, nRays);
    const auto cprim = to_host(c.prim, (size_t)nRays * K);
    const auto nGot = to_host(got.sizes, 7);
    const auto todo = to_host(got.items[6], (size_t)nGot[6]);
    int nHostWon = 0, nVoid = 0;
    for (int i : todo) {
        if (count[i] == 0) return 1;  // needs_host holds exactly the rays with candidates
        if (count[i] < 0) {
            ++nVoid;
            continue;
        }
        const nnbvh_hit dev = hits[i];
        nnbvh_hit res = dev;
        res.prim = -1, res.t = INFINITY, res.instance = 0;
        float tMax = INFINITY;
        bool took = false;
        for (int j = 0; j < count[i]; ++j) {
            if (j == before[i] && dev.prim >= 0 && (!took || dev.t <= tMax)) res = dev, tMax = dev.t, took = false;
            if (hostIntersect(cprim[(size_t)i * K + j], rays[i], tMax, res)) tMax = res.t, took = true;
        }
        if (before[i] == count[i] && dev.prim >= 0 && (!took || dev.t <= tMax)) res = dev;
        res.nodes_visited = dev.nodes_visited, res.prim_tests = dev.prim_tests;
        if (res.prim >= 0 && res.prim % 5 == 2) ++nHostWon;
        hits[i] = res;
    }
    HIP_OK(hipMemcpy(dHits, hits.data(), nRays * sizeof(nnbvh_hit), hipMemcpyHostToDevice));
    // 3. enqueue those rays, appended to the same queues, with a fresh needs_host
    items.needs_host = fresh.q(6);
    nnbvh::HipBVHAggregate::EnqueueClosestItemsIndexed(mesh.handle(), nRays, rq, got.items[6], got.sizes + 6, nRays, dHits,
                                                       dCls, nTris, got.out(), items, nullptr);
    // the same rays on the soup as triangles, plain call
    nnbvh_closest_items plainItems{};
    plainItems.needs_host = plain.q(6);
    plainAgg.IntersectClosestItemsQueues(mesh.handle(), nRays, rq, nullptr, dCls, nTris, dPlainHits, plain.out(), plainItems,
                                         nullptr);
    HIP_OK(hipDeviceSynchronize());
    const auto wGot = got.where(nRays, false), wPlain = plain.where(nRays, true);
    const auto wFresh = to_host(fresh.sizes, 7);
    const auto plainHits = to_host(dPlainHits, nRays);
    if (wFresh[6] != nVoid) return 2;
    int nSame = 0;
    for (int i = 0; i < nRays; ++i) {
        if (count[i] < 0) continue;
        if (wGot[i] != wPlain[i] || wGot[i] < 0) {
            std::printf("ray %d: queue %d against %d (count %d)\n", i, wGot[i], wPlain[i], count[i]);
            return 3;
        }
        if (hits[i].prim != plainHits[i].prim) return 4;
        if (hits[i].prim >= 0 && std::fabs(hits[i].t - plainHits[i].t) > 1e-4f * plainHits[i].t) return 5;
        ++nSame;
    }
    if (nHostWon < 50 || (int)todo.size() < 200 || nVoid * 100 > nRays) {
        std::printf("too few cases: %d host wins, %zu rays with candidates, %d void\n", nHostWon, todo.size(), nVoid);
        return 10;
    }
    std::printf("wavefront candidates ok: %d rays, %zu with candidates, %d won by host shapes, %d routed as the plain call\n",
                nRays, todo.size(), nHostWon, nSame);
    return 0;
}
