// two_level_alpha_texture_adapter_check — the HipBVHAggregate overloads for image-textured alpha in two-level scenes
// (include/nnbvh_aggregate.hpp) compile with a plain host compiler and hand their arguments to the C ABI.  No argument:
// argument faults only (no GPU).  "gpu": a four-triangle object placed twice (once scaled and moved) through both
// creation routes, whose closest hits must agree with each other and with the texture.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nnbvh_aggregate.hpp"

static std::string g_last;

int main(int argc, char **argv) {
    nnbvh::HipBVHAggregate::fatal_handler() = [](const char *msg) { g_last = msg; };
    std::vector<float> verts;
    std::vector<nnbvh_prim> object;
    for (int k = 0; k < 4; ++k) {
        const float x = 2.0f * k;
        const float v[9] = {x, 0, 0, x + 1, 0, 0, x + 1, 1, 0};
        verts.insert(verts.end(), v, v + 9);
        object.push_back(nnbvh_prim{k % 2 ? NNBVH_PRIM_ALPHATEX_TRIANGLE : NNBVH_PRIM_TRIANGLE, k, {3 * k, 3 * k + 1, 3 * k + 2, 0}});
    }
    const int nVerts = (int)verts.size() / 3;
    const float texels[4] = {1.0f, 1.0f, 0.0f, 0.0f};  // default corners: the upper row only
    std::vector<nnbvh_alpha_texture> textures{{texels, 2, 2, NNBVH_WRAP_CLAMP, 1, 1, 1, 0, 0, 1, 0}};
    const bool gpu = argc > 1 && !std::strcmp(argv[1], "gpu");
    const int device = gpu ? 0 : (1 << 20);
    // placement 0: the identity; placement 1: p -> 2 p + (0, 10, 0)
    std::vector<nnbvh_placement> placements(2);
    const float id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float m1[12] = {2, 0, 0, 0, 0, 2, 0, 10, 0, 0, 2, 0}, m1inv[12] = {0.5f, 0, 0, 0, 0, 0.5f, 0, -5, 0, 0, 0.5f, 0};
    std::memcpy(placements[0].render_from_prim, id, 48);
    std::memcpy(placements[0].prim_from_render, id, 48);
    std::memcpy(placements[1].render_from_prim, m1, 48);
    std::memcpy(placements[1].prim_from_render, m1inv, 48);
    placements[0].object = placements[1].object = 0;

    // the scene of host-built trees: a top-level leaf of the two instance entries, then the object's tree
    nnbvh_build *b = nnbvh_build_create(object.data(), (int)object.size(), verts.data(), nVerts, 4, NNBVH_SPLIT_SAH);
    if (!b) return 1;
    int nChild = 0, nOrdered = 0;
    const nnbvh_linear_node *child = nnbvh_build_nodes(b, &nChild);
    const nnbvh_prim *ordered = nnbvh_build_ordered_prims(b, &nOrdered);
    std::vector<nnbvh_linear_node> nodes(1);
    std::vector<nnbvh_prim> prims;
    std::vector<nnbvh_instance> instances(2);
    const float rootBox[6] = {child[0].pmin[0], child[0].pmin[1], child[0].pmin[2], child[0].pmax[0], child[0].pmax[1], child[0].pmax[2]};
    float top[6] = {1e30f, 1e30f, 1e30f, -1e30f, -1e30f, -1e30f};
    for (int j = 0; j < 2; ++j) {
        prims.push_back(nnbvh_prim{NNBVH_PRIM_INSTANCE, j, {j, 0, 0, 0}});
        float box[6];
        nnbvh_transform_bounds(placements[j].render_from_prim, rootBox, box);
        for (int a = 0; a < 3; ++a) {
            top[a] = std::min(top[a], box[a]);
            top[3 + a] = std::max(top[3 + a], box[3 + a]);
        }
        std::memcpy(instances[j].render_from_prim, placements[j].render_from_prim, 48);
        std::memcpy(instances[j].prim_from_render, placements[j].prim_from_render, 48);
        instances[j].root = 1;
        instances[j].n_nodes = nChild;
    }
    std::memcpy(nodes[0].pmin, top, 12);
    std::memcpy(nodes[0].pmax, top + 3, 12);
    nodes[0].offset = 0;
    nodes[0].nprims = 2;
    nodes[0].axis = nodes[0].pad = 0;
    for (int i = 0; i < nChild; ++i) {
        nnbvh_linear_node n = child[i];
        n.offset += n.nprims == 0 ? 1 : 2;  // interior: behind the top-level node; leaf: behind the instance entries
        nodes.push_back(n);
    }
    prims.insert(prims.end(), ordered, ordered + nOrdered);
    nnbvh_build_destroy(b);

    if (!gpu) {
        {
            nnbvh::HipBVHAggregate a(nodes.data(), (int)nodes.size(), 1, prims.data(), (int)prims.size(), verts.data(), nVerts,
                                     instances, textures, device);
        }
        if (g_last.find("scene_create_instanced_with_alpha_textures") == std::string::npos ||
            g_last.find("no usable HIP device") == std::string::npos)
            return 2;
        g_last.clear();
        auto dev = nnbvh::HipBVHAggregate::BuildTwoLevelOnDevice({}, verts, {object}, placements, 4, "sah", device, nullptr,
                                                                nullptr, nullptr, nullptr, nullptr, &textures);
        if (dev || g_last.find("no usable HIP device") == std::string::npos) return 3;
        g_last.clear();  // without the table the call is today's, which refuses the kind and names the new calls
        dev = nnbvh::HipBVHAggregate::BuildTwoLevelOnDevice({}, verts, {object}, placements, 4, "sah", device);
        if (dev || g_last.find("nnbvh_scene_create_instanced_gpu_build_with_alpha_textures") == std::string::npos) return 4;
        object[1].v[3] = 5;  // no such texture
        g_last.clear();
        dev = nnbvh::HipBVHAggregate::BuildTwoLevelOnDevice({}, verts, {object}, placements, 4, "sah", device, nullptr,
                                                           nullptr, nullptr, nullptr, nullptr, &textures);
        if (dev || g_last.find("nnbvh_scene_create_instanced_gpu_build_with_alpha_textures: alpha-texture index out of range") ==
                       std::string::npos)
            return 5;
        std::printf("two-level alpha texture adapter ok (arguments)\n");
        return 0;
    }
    nnbvh::HipBVHAggregate tree(nodes.data(), (int)nodes.size(), 1, prims.data(), (int)prims.size(), verts.data(), nVerts,
                                instances, textures, device);
    auto dev = nnbvh::HipBVHAggregate::BuildTwoLevelOnDevice({}, verts, {object}, placements, 4, "sah", device, nullptr,
                                                            nullptr, nullptr, nullptr, nullptr, &textures);
    if (!dev || !g_last.empty()) {
        std::fprintf(stderr, "%s\n", g_last.c_str());
        return 6;
    }
    // two rays per triangle and placement.  uvHit = (0.75, 0.25): st.t = 0.75, the lower row of the image, alpha 0, the
    // textured triangles (1, 3) are not hit; uvHit = (0.9, 0.8): the upper row, alpha 1, every triangle is hit
    std::vector<nnbvh_ray> rays;
    for (int j = 0; j < 2; ++j)
        for (int k = 0; k < 4; ++k)
            for (int w = 0; w < 2; ++w) {
                const float u = w ? 0.9f : 0.75f, v = w ? 0.8f : 0.25f, s = j ? 2.0f : 1.0f;
                rays.push_back(nnbvh_ray{{s * (2.0f * k + u), s * v + (j ? 10.0f : 0.0f), 1.0f}, 10.0f, {0, 0, -1}, 0});
            }
    const int n = (int)rays.size();
    std::vector<nnbvh_hit> h0((size_t)n), h1((size_t)n);
    if (nnbvh_intersect_closest(tree.handle(), rays.data(), n, h0.data()) != NNBVH_OK ||
        nnbvh_intersect_closest(dev->handle(), rays.data(), n, h1.data()) != NNBVH_OK)
        return 7;
    for (int i = 0; i < n; ++i) {
        const int j = i / 8, k = (i / 2) % 4, w = i % 2;
        const bool hit = w || k % 2 == 0;
        // (the hit itself: this file's top-level leaf is hand-made, so the walks' counters may differ between the routes;
        // the Python tests hold the two routes' device arrays to the byte)
        const nnbvh_hit &a = h0[(size_t)i], &c = h1[(size_t)i];
        if (a.prim != c.prim || a.instance != c.instance || std::memcmp(&a.t, &c.t, 16) != 0) {
            std::fprintf(stderr, "ray %d: routes differ: prim %d / %d instance %d / %d t %g / %g\n", i, a.prim, c.prim,
                         a.instance, c.instance, a.t, c.t);
            return 8;
        }
        if (h0[(size_t)i].prim != (hit ? k : -1) || h0[(size_t)i].instance != (hit ? j + 1 : 0)) {
            std::fprintf(stderr, "ray %d: prim %d instance %d\n", i, h0[(size_t)i].prim, h0[(size_t)i].instance);
            return 9;
        }
    }
    std::printf("two-level alpha texture adapter ok\n");
    return 0;
}
