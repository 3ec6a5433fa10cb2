// HipBVHAggregate::BuildTwoLevelOnDevice (include/nnbvh_aggregate.hpp) the way a pbrt scene with object instances
// would use it: one object definition placed a few times plus top-level triangles, every tree built and baked on the
// device.  Checked against the scene of host-built trees (nnbvh_build_create_with_bounds +
// nnbvh_scene_create_instanced): the same baked arrays (nnbvh_scene_read) and the same hits.  Built by
// tests/test_cpp_two_level.py with g++ against libnnbvh_hip.so; run only where a GPU is present.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "nnbvh_aggregate.hpp"

static std::vector<unsigned char> read_array(const nnbvh_scene *s, int what) {
    int64_t info[6];
    if (nnbvh_scene_info(s, info) != NNBVH_OK) return {};
    std::vector<unsigned char> out((size_t)(what == 0 ? info[0] * 64 : info[1] * 16));
    if (!out.empty() && nnbvh_scene_read(s, what, out.data(), out.size()) != NNBVH_OK) out.assign(1, 0xff);
    return out;
}

int main() {
    std::mt19937 rng(11);
    std::uniform_real_distribution<float> U(-1.f, 1.f);
    std::vector<float> verts;
    auto soup = [&](int n, float extent, float size, int firstId) {
        std::vector<nnbvh_prim> prims;
        for (int i = 0; i < n; ++i) {
            const int v0 = (int)verts.size() / 3;
            float c[3] = {extent * U(rng), extent * U(rng), extent * U(rng)};
            for (int k = 0; k < 3; ++k)
                for (int a = 0; a < 3; ++a) verts.push_back(c[a] + size * U(rng));
            prims.push_back(nnbvh_prim{NNBVH_PRIM_TRIANGLE, firstId + i, {v0, v0 + 1, v0 + 2, 0}});
        }
        return prims;
    };
    const std::vector<nnbvh_prim> object = soup(300, 1.f, 0.3f, 0), top = soup(20, 8.f, 1.f, 1000);
    std::vector<nnbvh_placement> placements;
    for (int j = 0; j < 9; ++j) {
        nnbvh_placement p;
        std::memset(&p, 0, sizeof p);
        const float s = j == 4 ? -1.5f : 1.f + 0.2f * j, t[3] = {6 * U(rng), 6 * U(rng), 6 * U(rng)};  // j == 4: mirrored
        for (int k = 0; k < 3; ++k) {
            p.render_from_prim[4 * k + k] = k == 0 ? s : std::fabs(s);
            p.render_from_prim[4 * k + 3] = t[k];
            p.prim_from_render[4 * k + k] = 1 / p.render_from_prim[4 * k + k];
            p.prim_from_render[4 * k + 3] = -t[k] / p.render_from_prim[4 * k + k];
        }
        p.object = 0;
        placements.push_back(p);
    }
    const int nVerts = (int)verts.size() / 3;
    auto dev = nnbvh::HipBVHAggregate::BuildTwoLevelOnDevice(top, verts, {object}, placements);
    if (!dev) return 1;

    // the same scene from host-built trees
    nnbvh_build *child = nnbvh_build_create(object.data(), (int)object.size(), verts.data(), nVerts, 4, NNBVH_SPLIT_SAH);
    if (!child) return 2;
    int nChild = 0, nChildPrims = 0;
    const nnbvh_linear_node *cn = nnbvh_build_nodes(child, &nChild);
    const nnbvh_prim *cp = nnbvh_build_ordered_prims(child, &nChildPrims);
    std::vector<nnbvh_prim> topList(top);
    std::vector<float> bounds(6 * top.size(), 0.f);
    for (size_t j = 0; j < placements.size(); ++j) {
        topList.push_back(nnbvh_prim{NNBVH_PRIM_INSTANCE, (int32_t)(top.size() + j), {(int32_t)j, 0, 0, 0}});
        const float box[6] = {cn[0].pmin[0], cn[0].pmin[1], cn[0].pmin[2], cn[0].pmax[0], cn[0].pmax[1], cn[0].pmax[2]};
        float out[6];
        nnbvh_transform_bounds(placements[j].render_from_prim, box, out);
        bounds.insert(bounds.end(), out, out + 6);
    }
    nnbvh_build *tb = nnbvh_build_create_with_bounds(topList.data(), (int)topList.size(), verts.data(), nVerts,
                                                     bounds.data(), 4, NNBVH_SPLIT_SAH);
    if (!tb) return 3;
    int nTop = 0, nTopPrims = 0;
    const nnbvh_linear_node *tn = nnbvh_build_nodes(tb, &nTop);
    const nnbvh_prim *tp = nnbvh_build_ordered_prims(tb, &nTopPrims);
    std::vector<nnbvh_linear_node> nodes(tn, tn + nTop);
    std::vector<nnbvh_prim> prims(tp, tp + nTopPrims);
    for (int i = 0; i < nChild; ++i) {
        nnbvh_linear_node nd = cn[i];
        nd.offset += nd.nprims == 0 ? nTop : nTopPrims;
        nodes.push_back(nd);
    }
    prims.insert(prims.end(), cp, cp + nChildPrims);
    std::vector<nnbvh_instance> instances(placements.size());
    for (size_t j = 0; j < placements.size(); ++j) {
        std::memcpy(instances[j].render_from_prim, placements[j].render_from_prim, 48);
        std::memcpy(instances[j].prim_from_render, placements[j].prim_from_render, 48);
        instances[j].root = nTop;
        instances[j].n_nodes = nChild;
    }
    nnbvh_scene *host = nnbvh_scene_create_instanced(nodes.data(), (int)nodes.size(), nTop, prims.data(), (int)prims.size(),
                                                     verts.data(), nVerts, instances.data(), (int)instances.size(), 0);
    nnbvh_build_destroy(child);
    nnbvh_build_destroy(tb);
    if (!host) return 4;
    for (int what = 0; what < 2; ++what) {
        const std::vector<unsigned char> a = read_array(dev->handle(), what), b = read_array(host, what);
        if (a.empty() || a != b) return 5 + what;
    }
    float garbage[4];
    if (nnbvh_scene_read(dev->handle(), 0, garbage, 3) != NNBVH_ERR_ARG) return 7;   // not the array's size
    if (nnbvh_scene_read(dev->handle(), 2, garbage, 16) != NNBVH_ERR_ARG) return 8;  // no animation table

    const int nRays = 2000;
    std::vector<nnbvh_ray> rays(nRays);
    for (auto &r : rays) {
        float o[3] = {9 * U(rng), 9 * U(rng), 9 * U(rng)}, t[3] = {6 * U(rng), 6 * U(rng), 6 * U(rng)};
        for (int a = 0; a < 3; ++a) {
            r.o[a] = o[a];
            r.d[a] = t[a] - o[a];
        }
        r.tmax = INFINITY;
        r.time = 0;
    }
    std::vector<nnbvh_hit> got(nRays), exp(nRays);
    dev->IntersectClosest(rays.data(), nRays, got.data());
    if (nnbvh_intersect_closest(host, rays.data(), nRays, exp.data()) != NNBVH_OK) return 9;
    if (std::memcmp(got.data(), exp.data(), sizeof(nnbvh_hit) * nRays)) return 10;
    int inside = 0;
    for (const nnbvh_hit &h : got) inside += h.instance > 0;
    nnbvh_scene_destroy(host);
    if (inside < 50) return 11;
    std::printf("two-level adapter ok: %d of %d rays hit inside an instance\n", inside, nRays);
    return 0;
}
