// nnbvh_internal.h — shared between the host-side pieces of libnnbvh_hip.so.
#pragma once
#include <cstdint>
#include <string>

#include "../../include/nnbvh.h"

namespace nnbvh {

void set_error(const std::string &msg);
// what is wrong with a call's nnbvh_host_candidates (closest: before is an output too), or nullptr (capi_trace.cpp;
// shared by the BVH and the kd-tree entry points)
const char *candidates_fault(const nnbvh_host_candidates *c, bool closest);

// ---- device data layout -----------------------------------
// One 64-byte record per INTERIOR node, holding both children's boxes, so that one
// coalesced 64-B fetch decides both child visits (the reference does two dependent 32-B
// LinearBVHNode fetches for the same decisions).  Records are numbered in the order
// the interior nodes appear in the reference's DFS array.
//   q0 = { c0.pmin.x, c0.pmin.y, c0.pmin.z, c0.pmax.x }
//   q1 = { c0.pmax.y, c0.pmax.z, c1.pmin.x, c1.pmin.y }
//   q2 = { c1.pmin.z, c1.pmax.x, c1.pmax.y, c1.pmax.z }
//   q3 = { ref0, ref1, axis, 0 }   (int32 bit patterns)
// c0 = the node at index+1 (first child), c1 = the node at secondChildOffset.
// ref >= 0: interior record number; ref < 0: leaf, ~ref = first 16-B slot of its
// primitives in the prim stream.
struct WideNode {
    float q[12];
    int32_t ref0, ref1;
    int32_t axis;
    int32_t pad;
};
static_assert(sizeof(WideNode) == 64, "WideNode must be 64 bytes");

// Prim stream: 16-B slots, primitives in the reference's leaf order.
//   triangle (3 slots): {p0.xyz, id} {p1.xyz, flags} {p2.xyz, 0}
//   patch    (4 slots): {p00.xyz, id} {p10.xyz, flags} {p01.xyz, 0} {p11.xyz, 0}
// flags bit0 = last primitive of its leaf, bit1 = bilinear patch, bit2 = degenerate triangle
// (LengthSquared(Cross(p2 - p0, p1 - p0)) == 0, shapes.cpp:176-177, evaluated at bake time).
constexpr uint32_t kPrimLast = 1u;
constexpr uint32_t kPrimPatch = 2u;
constexpr uint32_t kPrimDegenerate = 4u;
// instance (TransformedPrimitive) record, 6 slots:
//   {childRoot.pmin.xyz, instance index} {childRoot.pmax.xyz, flags}
//   {mInv row 0} {mInv row 1} {mInv row 2}  (renderFromPrimitive inverse, 3x4)
//   {child root ref, 0, 0, 0}
constexpr uint32_t kPrimInstance = 8u;
// host-only primitive (3 slots, no geometry): {0,0,0,id} {0,0,0,flags} {0,0,0,0}
constexpr uint32_t kPrimHost = 16u;

// alpha-tested triangle (GeometricPrimitive with a constant alpha, cpu/primitive.cpp:57-70): slot 2's
// fourth word holds alpha; kPrimFlipN = mesh->reverseOrientation ^ mesh->transformSwapsHandedness
constexpr uint32_t kPrimAlpha = 32u;
constexpr uint32_t kPrimFlipN = 64u;
// instance record of an AnimatedPrimitive: the inverse matrix is interpolated per ray from the
// animation table (anim_math.h) instead of read from slots 2..4
constexpr uint32_t kPrimAnimated = 128u;
// alpha-tested bilinear patch (kPrimPatch | kPrimAlpha): slot 2's fourth word holds alpha like a triangle's; with
// kPrimSmooth four more slots {n00,0} {n10,0} {n01,0} {n11,0} follow the patch's four; with kPrimUV two more,
// {uv00, uv10} {uv01, uv11}, after those
// alpha-tested triangle of a mesh WITH per-vertex shading normals: three more slots {n0,0} {n1,0} {n2,0} follow
// (the re-trace after a rejected hit offsets along FaceForward(n, ns), shapes.h:939-951)
constexpr uint32_t kPrimSmooth = 256u;
constexpr uint32_t kPrimUV = 512u;  // alpha-tested patch of a mesh with (u, v) coordinates
// alpha-tested triangle whose alpha is an image texture (kinds 16 .. 19; kPrimAlpha is set too): slot 2's fourth word
// holds the index into the scene's alpha-texture table instead of alpha; after the triangle's three slots (and the
// three normal slots of kPrimSmooth) two more follow, {u0, v0, u1, v1} {u2, v2, 0, 0}
constexpr uint32_t kPrimAlphaTex = 1024u;
constexpr int kAnimStride = 76;  // floats per entry of the animation table (layout: anim_math.h)
constexpr bool is_triangle_kind(int kind) {
    return kind == NNBVH_PRIM_TRIANGLE || kind == NNBVH_PRIM_ALPHA_TRIANGLE || kind == NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED ||
           kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH || kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED;
}
constexpr bool is_smooth_alpha_kind(int kind) {
    return kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH || kind == NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED;
}
// alpha-tested bilinear patches: kind = 8 + flipped + 2 * smooth + 4 * uv
constexpr bool is_alpha_patch_kind(int kind) { return kind >= NNBVH_PRIM_ALPHA_PATCH && kind <= NNBVH_PRIM_ALPHA_PATCH_UV_SMOOTH_FLIPPED; }
constexpr bool is_smooth_alpha_patch_kind(int kind) { return is_alpha_patch_kind(kind) && ((kind - NNBVH_PRIM_ALPHA_PATCH) & 2); }
constexpr bool is_flipped_alpha_patch_kind(int kind) { return is_alpha_patch_kind(kind) && ((kind - NNBVH_PRIM_ALPHA_PATCH) & 1); }
constexpr bool is_uv_alpha_patch_kind(int kind) { return is_alpha_patch_kind(kind) && ((kind - NNBVH_PRIM_ALPHA_PATCH) & 4); }
constexpr int alpha_patch_slots(int kind) { return 4 + (is_smooth_alpha_patch_kind(kind) ? 4 : 0) + (is_uv_alpha_patch_kind(kind) ? 2 : 0); }
constexpr bool is_flat_alpha_kind(int kind) {
    return kind == NNBVH_PRIM_ALPHA_TRIANGLE || kind == NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED;
}

// kd scenes: the alpha-tested kinds that read per-vertex or per-primitive arrays run on the device when the caller
// gave what they read (their geometry and attribute slots are baked); without, they are the host's (a record without
// geometry).  ONE rule for the scene flags capi_kd.cpp computes and for the device baker (kd_bake.hip)
constexpr bool kd_attr_on_device(int kind, bool normals, bool uvs, bool prim_alpha) {
    if (is_smooth_alpha_kind(kind)) return normals;
    if (is_alpha_patch_kind(kind))
        return prim_alpha && (!is_smooth_alpha_patch_kind(kind) || normals) && (!is_uv_alpha_patch_kind(kind) || uvs);
    return false;
}

// image-textured alpha on triangles: kind = 16 + flipped + 2 * smooth.  NOT an is_triangle_kind: only the builders and
// the creation calls with an alpha-texture table (flat and two-level BVH scenes, kd scenes) take them
constexpr bool is_alphatex_kind(int kind) { return kind >= NNBVH_PRIM_ALPHATEX_TRIANGLE && kind <= NNBVH_PRIM_ALPHATEX_TRIANGLE_SMOOTH_FLIPPED; }
constexpr bool is_smooth_alphatex_kind(int kind) { return is_alphatex_kind(kind) && ((kind - NNBVH_PRIM_ALPHATEX_TRIANGLE) & 2); }
constexpr bool is_flipped_alphatex_kind(int kind) { return is_alphatex_kind(kind) && ((kind - NNBVH_PRIM_ALPHATEX_TRIANGLE) & 1); }
constexpr int alphatex_slots(int kind) { return 5 + (is_smooth_alphatex_kind(kind) ? 3 : 0); }
constexpr int kMaxAlphaTexSize = 1 << 24;
// how every creation call without an alpha-texture table refuses them
constexpr const char *kAlphaTexElsewhere =
    "unknown primitive kind (image-textured alpha, kinds 16 .. 19, is for flat BVH scenes: "
    "nnbvh_scene_create_with_alpha_textures / nnbvh_scene_create_gpu_build_with_alpha_textures, and kd scenes: "
    "nnbvh_kd_scene_create_with_alpha_textures / nnbvh_kd_scene_create_gpu_build_with_alpha_textures, and two-level "
    "scenes: nnbvh_scene_create_instanced_with_alpha_textures / "
    "nnbvh_scene_create_instanced_gpu_build_with_alpha_textures)";
// Everything a kernel indexes a texture with, checked on the host before a device is looked at; `fn` names the call
// (bvh_capi.cpp; shared by the flat BVH, the two-level and the kd creation calls).  with_patches: alpha-tested patches
// (kinds 8 .. 15) may share the scene with the textured triangles (two-level scenes only)
bool check_alpha_textures(const char *fn, const nnbvh_prim *prims, int n_prims, const float *normals,
                          const nnbvh_alpha_texture *textures, int n_textures, bool with_patches = false);

constexpr int kMaxStack = 64;  // the reference's nodesToVisit[64], aggregates.cpp:538

// The top table of a lean scene (top_table.h): byte copies of the first kTopRecords interior records in
// breadth-first order from the root, which the lean one-launch kernels serve from LDS.  Inside the copies a reference
// to another copied record is kTopTag | its table slot: still >= 0 ("interior"), and bit 30 is free because the lean
// instances only run scenes with fewer than 2^26 records (scene_fits32).  63 records = 4 032 B: the 4 KiB per
// 256-thread block that the four hit words occupied.  (The kernels' larger blocks extend their LDS copy themselves:
// top_extend.h.)
constexpr int kTopRecords = 63;
constexpr int32_t kTopTag = 1 << 30;

// The degenerate-triangle test of shapes.cpp:176-177, LengthSquared(Cross(p2 - p0, p1 - p0)) == 0 with
// DifferenceOfProducts (util/math.h:569-575), in the reference's float32 operations, for the bake of the kd primitive
// records (kd_bake.hip) and host code that wants the same bits.  The fused multiply-adds are explicit; the build's
// -ffp-contract=off forms no others.
#if defined(__HIPCC__)
#define NNBVH_HD __host__ __device__
#else
#define NNBVH_HD
#endif
NNBVH_HD inline float kd_difference_of_products(float a, float b, float c, float d) {
    const float cd = c * d;
    const float diff = __builtin_fmaf(a, b, -cd);
    const float err = __builtin_fmaf(-c, d, cd);
    return diff + err;
}
NNBVH_HD inline bool kd_triangle_is_degenerate(const float *p0, const float *p1, const float *p2) {
    const float v[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    const float w[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const float cx = kd_difference_of_products(v[1], w[2], v[2], w[1]);
    const float cy = kd_difference_of_products(v[2], w[0], v[0], w[2]);
    const float cz = kd_difference_of_products(v[0], w[1], v[1], w[0]);
    return cx * cx + cy * cy + cz * cz == 0.0f;
}

// Transform::operator()(const Bounds3f&), util/transform.cpp:134-139: the union of the 8 transformed corners
// (Bounds3::Corner, vecmath.h:1284-1289; point transform util/transform.h:310-319 with w == 1), corner after corner
// with std::min / std::max's choice among equals (the first is kept), so the sign of a zero extreme is the
// sequential one.  ONE function for nnbvh_transform_bounds (bvh_capi.cpp) and the device's instance bounds
// (bvh_bake.hip): no contraction (-ffp-contract=off), the sums in the written order.
NNBVH_HD inline void transform_bounds(const float m[12], const float in[6], float out[6]) {
    float mn[3], mx[3];
    for (int k = 0; k < 3; ++k) {
        mn[k] = 3.402823466e+38f;   // numeric_limits<float>::max()
        mx[k] = -3.402823466e+38f;  // ... ::lowest()
    }
    for (int c = 0; c < 8; ++c) {
        const float p[3] = {in[(c & 1) ? 3 : 0], in[(c & 2) ? 4 : 1], in[(c & 4) ? 5 : 2]};
        for (int k = 0; k < 3; ++k) {
            const float v = m[4 * k] * p[0] + m[4 * k + 1] * p[1] + m[4 * k + 2] * p[2] + m[4 * k + 3];
            mn[k] = v < mn[k] ? v : mn[k];
            mx[k] = mx[k] < v ? v : mx[k];
        }
    }
    for (int k = 0; k < 3; ++k) {
        out[k] = mn[k];
        out[3 + k] = mx[k];
    }
}

}  // namespace nnbvh
