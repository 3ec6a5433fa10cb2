// kd_alpha_texture_adapter_check — the HipKdTreeAggregate overloads for image-textured alpha
// (include/nnbvh_aggregate.hpp) compile with a plain host compiler and hand their arguments to the C ABI.  No argument:
// argument faults only (no GPU).  "gpu": a four-triangle scene through both creation routes, whose closest hits must
// agree.
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nnbvh_aggregate.hpp"

static std::string g_last;

int main(int argc, char **argv) {
    nnbvh::HipBVHAggregate::fatal_handler() = [](const char *msg) { g_last = msg; };
    std::vector<float> verts;
    std::vector<nnbvh_prim> prims;
    for (int k = 0; k < 4; ++k) {
        const float x = 2.0f * k;
        const float v[9] = {x, 0, 0, x + 1, 0, 0, x + 1, 1, 0};
        verts.insert(verts.end(), v, v + 9);
        prims.push_back(nnbvh_prim{k % 2 ? NNBVH_PRIM_ALPHATEX_TRIANGLE : NNBVH_PRIM_TRIANGLE, k, {3 * k, 3 * k + 1, 3 * k + 2, 0}});
    }
    const float texels[4] = {1.0f, 1.0f, 0.0f, 0.0f};  // default corners: the upper row only
    std::vector<nnbvh_alpha_texture> textures{{texels, 2, 2, NNBVH_WRAP_CLAMP, 1, 1, 1, 0, 0, 1, 0}};
    const bool gpu = argc > 1 && !std::strcmp(argv[1], "gpu");
    const int device = gpu ? 0 : (1 << 20);
    const int nVerts = (int)verts.size() / 3;

    // the stable host builder: its leaf order is the device route's
    const std::unique_ptr<nnbvh_kd_build, void (*)(nnbvh_kd_build *)> build(
        nnbvh_kd_build_create_stable(prims.data(), (int)prims.size(), verts.data(), nVerts, nullptr, 5, 1, 0.5f, 1, -1),
        nnbvh_kd_build_destroy);  // destroyed on every way out
    const nnbvh_kd_build *b = build.get();
    if (!b) return 1;
    int nNodes = 0, nIdx = 0;
    const nnbvh_kd_node *nodes = nnbvh_kd_build_nodes(b, &nNodes);
    const int32_t *idx = nnbvh_kd_build_prim_indices(b, &nIdx);
    float bounds[6];
    if (nnbvh_kd_build_bounds(b, bounds) != NNBVH_OK) return 1;
    g_last.clear();
    if (!gpu) {
        {
            nnbvh::HipKdTreeAggregate a(nodes, nNodes, idx, nIdx, prims.data(), (int)prims.size(), verts.data(), nVerts, bounds,
                                        textures, device);
        }
        if (g_last.find("no usable HIP device") == std::string::npos) return 2;
        g_last.clear();
        auto dev = nnbvh::HipKdTreeAggregate::BuildOnDevice(prims, verts, textures, 5, 1, 0.5f, 1, -1, device);
        if (dev || g_last.find("no usable HIP device") == std::string::npos) return 3;
        prims[1].v[3] = 5;  // no such texture
        g_last.clear();
        dev = nnbvh::HipKdTreeAggregate::BuildOnDevice(prims, verts, textures, 5, 1, 0.5f, 1, -1, device);
        if (dev || g_last.find("nnbvh_kd_scene_create_gpu_build_with_alpha_textures: alpha-texture index out of range") == std::string::npos)
            return 4;
        g_last.clear();
        {
            nnbvh::HipKdTreeAggregate a(nodes, nNodes, idx, nIdx, prims.data(), (int)prims.size(), verts.data(), nVerts, bounds,
                                        textures, device);
        }
        if (g_last.find("nnbvh_kd_scene_create_with_alpha_textures: alpha-texture index out of range") == std::string::npos)
            return 5;
        std::printf("kd alpha texture adapter ok (arguments)\n");
        return 0;
    }
    nnbvh::HipKdTreeAggregate tree(nodes, nNodes, idx, nIdx, prims.data(), (int)prims.size(), verts.data(), nVerts, bounds,
                                   textures, device);
    auto dev = nnbvh::HipKdTreeAggregate::BuildOnDevice(prims, verts, textures, 5, 1, 0.5f, 1, -1, device);
    if (!dev || !g_last.empty()) {
        std::fprintf(stderr, "%s\n", g_last.c_str());
        return 6;
    }
    // one ray per triangle, at uvHit = (0.75, 0.25): st.t = 0.75, the lower row of the image, alpha 0: the textured
    // triangles (1, 3) are never hit, the plain ones are
    std::vector<nnbvh_ray> rays;
    for (int k = 0; k < 4; ++k) rays.push_back(nnbvh_ray{{2.0f * k + 0.75f, 0.25f, 1.0f}, 10.0f, {0, 0, -1}, 0});
    std::vector<nnbvh_hit> h0(4), h1(4);
    if (nnbvh_kd_intersect_closest(tree.handle(), rays.data(), 4, h0.data()) != NNBVH_OK ||
        nnbvh_kd_intersect_closest(dev->handle(), rays.data(), 4, h1.data()) != NNBVH_OK)
        return 7;
    for (int k = 0; k < 4; ++k) {
        if (std::memcmp(&h0[k], &h1[k], sizeof(nnbvh_hit)) != 0) return 8;
        if (h0[k].prim != (k % 2 ? -1 : k)) return 9;
    }
    std::printf("kd alpha texture adapter ok\n");
    return 0;
}
