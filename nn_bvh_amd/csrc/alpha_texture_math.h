// alpha_texture_math.h — FloatImageTexture::Evaluate (textures.h:579-590) on the interaction a Triangle has just made,
// as GeometricPrimitive::Intersect calls it for the alpha test (cpu/primitive.cpp:57-58).  That interaction's
// dudx .. dvdy are still their initial zeros (interaction.h:263), so UVMapping::Map (textures.h:95-102) yields zero
// differentials and MIPMap::Filter (util/mipmap.cpp:229-284) has width 0: level = nLevels - 1 + Log2(1e-8) < 0 for
// every image with fewer than 27 levels, iLevel = 0.  Bilinear and trilinear filtering return Bilerp(0, st), EWA
// reaches shorterVecLength == 0 -> Bilerp(0, st), the point filter returns one level-0 texel.  What is left:
//   uvHit = b0 uv0 + b1 uv1 + b2 uv2              shapes.h, InteractionFromIntersection (interaction_math.h's form)
//   st = (su u + du, sv v + dv); st[1] = 1 - st[1] textures.h:100, :587
//   Image::BilerpChannel                           util/image.h:279-292, taps through RemapPixelCoords (:96-146)
//   scale * v; invert ? max(0, 1 - v) : v          textures.h:588-589
// Operation for operation as the reference has it: the build's -ffp-contract=off forms no fused multiply-adds and
// the reference calls no FMA() here.  One function for the trace kernel (bvh_trace.hip, ALPHA = 3), the host and
// the stand-alone checks (tests/cpp, tests/hip).
//
// The reference converts floor(x) to int without a range check (undefined outside +-2^31); here the conversion
// saturates (to [-2^31, 2^31 - 2], so that the neighbouring tap's + 1 cannot overflow either) and no tap ever reads
// outside the texel pool.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define NNBVH_ATEX_HD __host__ __device__ inline
#else
#define NNBVH_ATEX_HD inline
#endif

namespace nnbvh {

constexpr int kWrapRepeat = 0, kWrapClamp = 1, kWrapBlack = 2;  // NNBVH_WRAP_* (include/nnbvh.h)

// what the kernel reads of an nnbvh_alpha_texture: 48 bytes, three 16-B loads (the scene's descriptor table)
struct AlphaTexDesc {
    uint32_t texelLo, texelHi;  // first texel of level 0 in the scene's texel pool (in floats)
    int32_t width, height;
    int32_t wrap, pointFilter;
    float su, sv;
    float du, dv;
    float scale;
    int32_t invert;
};
static_assert(sizeof(AlphaTexDesc) == 48, "three 16-byte slots");

// int(pstd::floor(x)) / int(pstd::round(x)) with a saturating conversion (NaN -> 0)
NNBVH_ATEX_HD int32_t atex_to_int(float f) {
    if (f != f) return 0;
    if (f >= 2147483648.0f) return 2147483646;
    if (f <= -2147483648.0f) return -2147483647 - 1;
    return (int32_t)f;
}

// one coordinate through RemapPixelCoords (util/image.h:127-144): false = WrapMode::Black outside the image
NNBVH_ATEX_HD bool atex_remap(int32_t &p, int32_t res, int32_t wrap) {
    if (p >= 0 && p < res) return true;
    if (wrap == kWrapRepeat) {  // Mod (util/math.h:129-133): a - (a / b) * b, + b when negative
        const int32_t r = p - (p / res) * res;
        p = r < 0 ? r + res : r;
        return true;
    }
    if (wrap == kWrapClamp) {
        p = p < 0 ? 0 : res - 1;
        return true;
    }
    return false;
}

// Image::GetChannel({x, y}, 0, wrapMode) of level 0 (util/image.h:255-258)
NNBVH_ATEX_HD float atex_texel(const AlphaTexDesc &d, const float *pool, int32_t x, int32_t y) {
    // (both coordinates are remapped before Black returns: the order cannot be seen from outside)
    if (!atex_remap(x, d.width, d.wrap)) return 0.0f;
    if (!atex_remap(y, d.height, d.wrap)) return 0.0f;
    const uint64_t first = ((uint64_t)d.texelHi << 32) | d.texelLo;
    return pool[first + (uint64_t)y * (uint64_t)d.width + (uint64_t)x];
}

// alpha.Evaluate(si->intr): barycentrics of the hit, the triangle's three (u, v) pairs, the texture
NNBVH_ATEX_HD float alpha_texture_eval(float b0, float b1, float b2, float u0, float v0, float u1, float v1, float u2,
                                       float v2, const AlphaTexDesc &d, const float *pool) {
    const float u = (b0 * u0 + b1 * u1) + b2 * u2;
    const float v = (b0 * v0 + b1 * v1) + b2 * v2;
    const float s = d.su * u + d.du;
    float t = d.sv * v + d.dv;
    t = 1 - t;
    float val;
    if (d.pointFilter) {  // mipmap.cpp:241-246: pstd::round = half away from zero
        const int32_t xi = atex_to_int(__builtin_roundf(s * d.width - 0.5f));
        const int32_t yi = atex_to_int(__builtin_roundf(t * d.height - 0.5f));
        val = atex_texel(d, pool, xi, yi);
    } else {  // util/image.h:279-292
        const float x = s * d.width - 0.5f, y = t * d.height - 0.5f;
        const int32_t xi = atex_to_int(__builtin_floorf(x)), yi = atex_to_int(__builtin_floorf(y));
        const float dx = x - (float)xi, dy = y - (float)yi;
        const float t00 = atex_texel(d, pool, xi, yi), t10 = atex_texel(d, pool, xi + 1, yi);
        const float t01 = atex_texel(d, pool, xi, yi + 1), t11 = atex_texel(d, pool, xi + 1, yi + 1);
        val = ((1 - dx) * (1 - dy) * t00 + dx * (1 - dy) * t10 + (1 - dx) * dy * t01 + dx * dy * t11);
    }
    val = d.scale * val;
    if (d.invert) {  // std::max<Float>(0, 1 - v): (a < b) ? b : a
        const float w = 1 - val;
        return (0.0f < w) ? w : 0.0f;
    }
    return val;
}

}  // namespace nnbvh
