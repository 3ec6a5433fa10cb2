// Exercises HipKdTreeAggregate's batch and wavefront-queue methods (include/nnbvh_aggregate.hpp) the way a wavefront
// renderer would: one iteration (IntersectClosestQueues, then the shadow queue and the next ray queue in one launch)
// on device-resident SOA queues, compared with the flat *Device calls on the same rays.  Built by
// tests/test_kd_wavefront_cpp.py with g++ against libnnbvh_hip.so and the HIP runtime; run only where a GPU is present.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

// the four runtime calls this caller needs (no HIP headers: a plain host compiler builds this file)
extern "C" {
int hipMalloc(void **ptr, size_t bytes);
int hipFree(void *ptr);
int hipMemcpy(void *dst, const void *src, size_t bytes, int kind);
int hipDeviceSynchronize(void);
}
static const int kH2D = 1, kD2H = 2;

template <class T>
static T *upload(const std::vector<T> &v, size_t atLeast = 1) {
    void *d = nullptr;
    const size_t n = v.size() > atLeast ? v.size() : atLeast;
    if (hipMalloc(&d, n * sizeof(T)) != 0) std::exit(90);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), kH2D) != 0) std::exit(91);
    return (T *)d;
}
template <class T>
static std::vector<T> download(const T *d, size_t n) {
    std::vector<T> v(n);
    if (hipDeviceSynchronize() != 0 || hipMemcpy(v.data(), d, n * sizeof(T), kD2H) != 0) std::exit(92);
    return v;
}

struct DeviceQueue {  // a ray queue in both forms: SOA slices for the queue calls, records for the flat calls
    nnbvh_ray_soa soa{};
    nnbvh_ray *records = nullptr;
    int n = 0;
    explicit DeviceQueue(const std::vector<nnbvh_ray> &rays, bool shadow) : n((int)rays.size()) {
        std::vector<float> c[7];
        for (const nnbvh_ray &r : rays) {
            for (int a = 0; a < 3; ++a) c[a].push_back(r.o[a]), c[3 + a].push_back(r.d[a]);
            c[6].push_back(r.tmax);
        }
        soa.ox = upload(c[0]), soa.oy = upload(c[1]), soa.oz = upload(c[2]);
        soa.dx = upload(c[3]), soa.dy = upload(c[4]), soa.dz = upload(c[5]);
        soa.tmax = shadow ? upload(c[6]) : nullptr;
        records = upload(rays);
    }
};

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    const int nTris = 800, nRays = 5000, nShadow = 3000, nPixels = 4000;
    std::vector<float> verts;
    std::vector<nnbvh_prim> prims;
    for (int i = 0; i < nTris; ++i) {
        float c[3] = {5 * U(rng), 5 * U(rng), 5 * U(rng)};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts.push_back(c[a] + 0.6f * U(rng));
        prims.push_back(nnbvh_prim{NNBVH_PRIM_TRIANGLE, i, {3 * i, 3 * i + 1, 3 * i + 2, 0}});
    }
    nnbvh::HipKdTreeAggregate kd(prims, verts);
    auto make = [&](int n, bool shadow) {
        std::vector<nnbvh_ray> rays(n);
        for (auto &r : rays) {
            for (int a = 0; a < 3; ++a) {
                r.o[a] = 6 * U(rng);
                r.d[a] = 4 * U(rng) - r.o[a];
            }
            r.tmax = shadow ? 1.0f - 1e-4f : INFINITY;
            r.time = 0;
        }
        return rays;
    };
    const DeviceQueue first(make(nRays, false), false), next(make(nRays, false), false), shadow(make(nShadow, true), true);

    // the flat calls: what every queue call below must reproduce
    nnbvh_hit *dFlatFirst = upload(std::vector<nnbvh_hit>(nRays)), *dFlatNext = upload(std::vector<nnbvh_hit>(nRays));
    uint8_t *dFlatOcc = upload(std::vector<uint8_t>(nShadow));
    kd.IntersectClosestDevice(first.records, nRays, dFlatFirst, nullptr);
    kd.IntersectClosestDevice(next.records, nRays, dFlatNext, nullptr);
    kd.IntersectShadowDevice(shadow.records, nShadow, dFlatOcc, nullptr);
    const auto flatFirst = download(dFlatFirst, nRays), flatNext = download(dFlatNext, nRays);
    const auto flatOcc = download(dFlatOcc, nShadow);

    // the same three batches in ONE launch
    nnbvh_hit *dBatchNext = upload(std::vector<nnbvh_hit>(nRays)), *dBatchFirst = upload(std::vector<nnbvh_hit>(nRays));
    uint8_t *dBatchOcc = upload(std::vector<uint8_t>(nShadow, 9));
    const nnbvh_batch batches[3] = {{NNBVH_BATCH_CLOSEST, 0, next.records, nRays, dBatchNext, nullptr, nullptr},
                                    {NNBVH_BATCH_ANY, 0, shadow.records, nShadow, dBatchOcc, nullptr, nullptr},
                                    {NNBVH_BATCH_CLOSEST, 0, first.records, nRays, dBatchFirst, nullptr, nullptr}};
    kd.TraceBatchesDevice(batches, 3, nullptr);
    if (std::memcmp(download(dBatchNext, nRays).data(), flatNext.data(), nRays * sizeof(nnbvh_hit))) return 1;
    if (std::memcmp(download(dBatchFirst, nRays).data(), flatFirst.data(), nRays * sizeof(nnbvh_hit))) return 2;
    if (download(dBatchOcc, nShadow) != flatOcc) return 3;

    // one wavefront iteration on the queues
    auto work_queue = [&](int capacity) {
        return nnbvh_work_queue{upload(std::vector<int32_t>(capacity)), upload(std::vector<int32_t>(1, 0)), capacity, 0};
    };
    nnbvh_closest_queues out1{}, out2{};
    out1.escaped = work_queue(nRays), out1.basic_eval_material = work_queue(nRays);
    out2.escaped = work_queue(nRays), out2.basic_eval_material = work_queue(16);  // overflows: counted, not stored
    nnbvh_hit *dHits1 = upload(std::vector<nnbvh_hit>(nRays)), *dHits2 = upload(std::vector<nnbvh_hit>(nRays));
    uint8_t *dOcc = upload(std::vector<uint8_t>(nShadow, 9));
    std::vector<float> Ld(4 * nShadow), ru(4 * nShadow, 0.5f), rl(4 * nShadow, 0.5f), L(4 * nPixels, 0.25f);
    for (float &v : Ld) v = 1 + U(rng);
    std::vector<int32_t> px(nShadow);
    for (int i = 0; i < nShadow; ++i) px[i] = i;
    float *dLd = upload(Ld), *dRu = upload(ru), *dRl = upload(rl), *dL = upload(L);
    int32_t *dPx = upload(px), *dShadowSize = upload(std::vector<int32_t>(1, nShadow - 500));
    int32_t *dAbove = upload(std::vector<int32_t>(1, nRays + 100000));  // a device size above the bound is clamped to it
    kd.IntersectClosestQueues(nRays, first.soa, dAbove, nullptr, 0, dHits1, out1, nullptr);
    kd.IntersectClosestAndShadowQueues(nRays, next.soa, nullptr, nullptr, 0, dHits2, out2, nShadow, shadow.soa,
                                       dShadowSize, dLd, dRu, dRl, dPx, dL, nPixels, nullptr, dOcc);
    if (std::memcmp(download(dHits1, nRays).data(), flatFirst.data(), nRays * sizeof(nnbvh_hit))) return 4;
    if (std::memcmp(download(dHits2, nRays).data(), flatNext.data(), nRays * sizeof(nnbvh_hit))) return 5;
    const auto occ = download(dOcc, nShadow);
    const auto gotL = download(dL, 4 * (size_t)nPixels);
    int nVisible = 0;
    for (int i = 0; i < nShadow; ++i) {
        const bool in = i < nShadow - 500;
        if (occ[i] != (in ? flatOcc[i] : 9)) return 6;  // nothing beyond the device-side size
        for (int c = 0; c < 4; ++c) {
            const float avg = (((1.0f + 1.0f) + 1.0f) + 1.0f) / 4.0f;
            const float want = (in && flatOcc[i] == 0) ? 0.25f + Ld[4 * i + c] / avg : 0.25f;
            if (std::memcmp(&want, &gotL[4 * i + c], 4)) return 7;
        }
        nVisible += in && flatOcc[i] == 0;
    }
    int miss1 = 0, miss2 = 0;
    for (int i = 0; i < nRays; ++i) miss1 += flatFirst[i].prim < 0, miss2 += flatNext[i].prim < 0;
    if (download(out1.escaped.size, 1)[0] != miss1 || download(out1.basic_eval_material.size, 1)[0] != nRays - miss1) return 8;
    if (download(out2.escaped.size, 1)[0] != miss2 || download(out2.basic_eval_material.size, 1)[0] != nRays - miss2) return 9;
    for (int32_t i : download(out2.basic_eval_material.items, 16))
        if (i < 0 || i >= nRays || flatNext[i].prim < 0) return 10;
    if (miss1 == 0 || miss1 == nRays || nVisible == 0 || nVisible == nShadow - 500) return 11;  // a trivial scene shows nothing
    std::printf("kd wavefront ok: %d rays, %d escaped, %d of %d shadow rays visible\n", nRays, miss1, nVisible, nShadow - 500);
    return 0;
}
