// Exercises HipBVHAggregate::IntersectShadowTrBounded / IntersectOneRandomBounded (include/nnbvh_aggregate.hpp)
// against the unbounded adapter methods IntersectShadowTrQueue / IntersectOneRandomQueue on the same device-resident
// inputs: with enough passes every output is the unbounded call's, byte for byte, and nothing is unfinished; with one
// pass the walks that need more are marked as the caller's and counted.  This checks the adapter (argument order, the
// two drivers of one pass loop agreeing), not the walk: both methods run the same kernels, and what those compute is
// held to the oracle by tests/test_wavefront_bounded.py and tests/test_wavefront_tr.py.  Built by
// tests/test_wavefront_bounded_cpp.py
// with g++ against libnnbvh_hip.so and the HIP runtime; run only where a GPU is present.
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
static T *upload(const std::vector<T> &v) {
    void *d = nullptr;
    if (hipMalloc(&d, (v.empty() ? 1 : v.size()) * sizeof(T)) != 0) std::exit(90);
    if (!v.empty() && hipMemcpy(d, v.data(), v.size() * sizeof(T), kH2D) != 0) std::exit(91);
    return (T *)d;
}
template <class T>
static std::vector<T> download(const T *d, size_t n) {
    std::vector<T> v(n);
    if (hipDeviceSynchronize() != 0 || hipMemcpy(v.data(), d, n * sizeof(T), kD2H) != 0) std::exit(92);
    return v;
}

int main() {
    std::mt19937 rng(5);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    // a soup dense enough that a segment through it crosses several triangles
    const int nTris = 250, nShadow = 2001, nItems = 1501, nPixels = nShadow;
    std::vector<float> verts;
    std::vector<nnbvh_prim> prims;
    std::vector<int32_t> triVerts;
    std::vector<uint8_t> cls(nTris);
    std::vector<int32_t> primMaterial(nTris);
    for (int i = 0; i < nTris; ++i) {
        float c[3] = {2.5f * U(rng), 2.5f * U(rng), 2.5f * U(rng)};
        for (int k = 0; k < 3; ++k)
            for (int a = 0; a < 3; ++a) verts.push_back(c[a] + 0.9f * U(rng));
        prims.push_back(nnbvh_prim{NNBVH_PRIM_TRIANGLE, i, {3 * i, 3 * i + 1, 3 * i + 2, 0}});
        for (int k = 0; k < 3; ++k) triVerts.push_back(3 * i + k);
        cls[i] = (i % 10 < 8) ? NNBVH_CLASS_INTERFACE : NNBVH_CLASS_BASIC;
        primMaterial[i] = i % 3;
    }
    nnbvh::HipBVHAggregate agg(prims, verts);
    nnbvh::HipShadingMesh mesh(verts.data(), 3 * nTris, triVerts.data(), nTris);

    // ---- shadow rays through interface surfaces ----
    std::vector<float> c[7];
    for (int i = 0; i < nShadow; ++i) {
        float o[3], d[3];
        for (int a = 0; a < 3; ++a) o[a] = 3 * U(rng), d[a] = 3 * U(rng) - o[a];
        if (i % 97 == 0) d[0] = d[1] = d[2] = 0;  // a zero direction: the walk never starts
        for (int a = 0; a < 3; ++a) c[a].push_back(o[a]), c[3 + a].push_back(d[a]);
        c[6].push_back(1.0f - 1e-4f);
    }
    nnbvh_ray_soa q{};
    q.ox = upload(c[0]), q.oy = upload(c[1]), q.oz = upload(c[2]);
    q.dx = upload(c[3]), q.dy = upload(c[4]), q.dz = upload(c[5]);
    q.tmax = upload(c[6]);
    std::vector<float> Ld(4 * nShadow), ru(4 * nShadow), rl(4 * nShadow), L0(4 * nPixels);
    for (float &v : Ld) v = 1 + U(rng);
    for (float &v : ru) v = 1 + 0.5f * U(rng);
    for (float &v : rl) v = 1 + 0.5f * U(rng);
    for (float &v : L0) v = 0.5f + 0.5f * U(rng);
    std::vector<int32_t> px(nShadow);
    for (int i = 0; i < nShadow; ++i) px[i] = (i * 7) % nPixels;
    float *dLd = upload(Ld), *dRu = upload(ru), *dRl = upload(rl);
    int32_t *dPx = upload(px);
    uint8_t *dCls = upload(cls);
    int32_t *dSize = upload(std::vector<int32_t>(1, nShadow - 100));
    int32_t *dUnfinished = upload(std::vector<int32_t>(1, -7));

    auto shadow = [&](int maxPasses, std::vector<uint8_t> &state, std::vector<float> &L) {
        float *dL = upload(L0);
        uint8_t *dState = upload(std::vector<uint8_t>(nShadow, 77));
        if (maxPasses == 0)
            agg.IntersectShadowTrQueue(mesh.handle(), nShadow, q, dSize, dCls, nTris, dLd, dRu, dRl, dPx, dL, nPixels,
                                       nullptr, dState);
        else
            agg.IntersectShadowTrBounded(mesh.handle(), nShadow, q, dSize, dCls, nTris, dLd, dRu, dRl, dPx, dL, nPixels,
                                         maxPasses, nullptr, dState, dUnfinished);
        state = download(dState, nShadow);
        L = download(dL, 4 * (size_t)nPixels);
        hipFree(dL);
        hipFree(dState);
    };
    std::vector<uint8_t> stRef, stAll, st1;
    std::vector<float> LRef, LAll, L1;
    shadow(0, stRef, LRef);
    shadow(64, stAll, LAll);
    if (stAll != stRef) return 1;
    if (std::memcmp(LAll.data(), LRef.data(), LRef.size() * 4)) return 2;
    if (download(dUnfinished, 1)[0] != 0) return 3;
    shadow(1, st1, L1);
    const int shadowLeft = download(dUnfinished, 1)[0];
    int twos = 0, arrived = 0, blocked = 0;
    for (int i = 0; i < nShadow; ++i) {
        if (i >= nShadow - 100) {
            if (st1[i] != 77 || stRef[i] != 77) return 4;  // nothing beyond the device-side size
            continue;
        }
        if (stRef[i] == 2) return 5;  // no host-only primitive in this scene
        twos += st1[i] == 2;
        arrived += stRef[i] == 0, blocked += stRef[i] == 1;
        if (st1[i] != 2 && st1[i] != stRef[i]) return 6;  // what one pass finishes is final
    }
    if (twos != shadowLeft || shadowLeft < 10) return 7;
    if (arrived < 10 || blocked < 10) return 8;  // a trivial scene shows nothing

    // ---- one-random walks ----
    std::vector<float> p0(3 * nItems), p1(3 * nItems);
    std::vector<int32_t> material(nItems);
    for (int i = 0; i < nItems; ++i) {
        for (int a = 0; a < 3; ++a) p0[3 * i + a] = 2.5f * U(rng), p1[3 * i + a] = 2.5f * U(rng);
        if (i % 50 == 0)
            for (int a = 0; a < 3; ++a) p1[3 * i + a] = p0[3 * i + a];  // a zero-length segment
        material[i] = i % 3;
    }
    float *dP0 = upload(p0), *dP1 = upload(p1);
    int32_t *dMat = upload(material), *dPrimMat = upload(primMaterial);
    struct Out {
        std::vector<nnbvh_hit> hits;
        std::vector<nnbvh_ray> rays;
        std::vector<float> pdf, wsum;
    };
    auto one_random = [&](int maxPasses) {
        nnbvh_hit *dHits = upload(std::vector<nnbvh_hit>(nItems));
        nnbvh_ray *dRays = upload(std::vector<nnbvh_ray>(nItems));
        float *dPdf = upload(std::vector<float>(nItems, -1.f)), *dW = upload(std::vector<float>(nItems, -1.f));
        if (maxPasses == 0)
            agg.IntersectOneRandomQueue(mesh.handle(), nItems, dP0, dP1, dMat, nullptr, dPrimMat, nTris, dHits, dRays,
                                        dPdf, nullptr, dW);
        else
            agg.IntersectOneRandomBounded(mesh.handle(), nItems, dP0, dP1, dMat, nullptr, dPrimMat, nTris, dHits, dRays,
                                          dPdf, maxPasses, nullptr, dW, dUnfinished);
        Out o{download(dHits, nItems), download(dRays, nItems), download(dPdf, nItems), download(dW, nItems)};
        hipFree(dHits), hipFree(dRays), hipFree(dPdf), hipFree(dW);
        return o;
    };
    const Out ref = one_random(0), all = one_random(64);
    if (std::memcmp(all.hits.data(), ref.hits.data(), nItems * sizeof(nnbvh_hit))) {
        int first = 0;
        while (!std::memcmp(&all.hits[first], &ref.hits[first], sizeof(nnbvh_hit))) ++first;
        std::fprintf(stderr, "selected hits differ: first at item %d (prim %d / %d, instance %d / %d), %d unfinished\n", first,
                     all.hits[first].prim, ref.hits[first].prim, all.hits[first].instance, ref.hits[first].instance,
                     download(dUnfinished, 1)[0]);
        return 10;
    }
    if (std::memcmp(all.rays.data(), ref.rays.data(), nItems * sizeof(nnbvh_ray))) return 11;
    if (std::memcmp(all.pdf.data(), ref.pdf.data(), nItems * 4) || std::memcmp(all.wsum.data(), ref.wsum.data(), nItems * 4))
        return 12;
    if (download(dUnfinished, 1)[0] != 0) return 13;
    const Out b1 = one_random(1);
    const int itemsLeft = download(dUnfinished, 1)[0];
    int marked = 0, selected = 0;
    for (int i = 0; i < nItems; ++i) {
        if (ref.hits[i].instance == -1) return 14;
        selected += ref.hits[i].prim >= 0;
        if (b1.hits[i].instance == -1) {
            ++marked;
            continue;
        }
        // finished within one pass: the reference's walk was that short too, and the outputs agree
        if (std::memcmp(&b1.hits[i], &ref.hits[i], sizeof(nnbvh_hit)) || std::memcmp(&b1.pdf[i], &ref.pdf[i], 4) ||
            std::memcmp(&b1.wsum[i], &ref.wsum[i], 4))
            return 15;
    }
    if (marked != itemsLeft || itemsLeft < 10 || itemsLeft > nItems - 10) return 16;
    if (selected < 10) return 17;
    std::printf("wavefront bounded ok: %d shadow rays (%d arrive, %d left after one pass), %d items (%d left after one pass)\n",
                nShadow, arrived, shadowLeft, nItems, itemsLeft);
    return 0;
}
