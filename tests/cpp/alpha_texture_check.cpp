// alpha_texture_check — nn_bvh_amd/csrc/alpha_texture_math.h evaluated on the host over a file of records
// (tests/alpha_texture_oracle.py write_records): int32 n_textures, n_records; per texture 10 words (width, height,
// wrap, point_filter, su, sv, du, dv, scale, invert); the texels of all textures; per record 10 float32 (b0 b1 b2,
// u0 v0 u1 v1 u2 v2, texture index).  Output: the bit pattern of alpha per record.  Built with the product's flags
// (-ffp-contract=off); tests/hip/alpha_texture_check.hip is the same program with the evaluation in a kernel.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alpha_texture_math.h"

int main(int argc, char **argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: alpha_texture_check in.bin out.bin\n");
        return 2;
    }
    FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) {
        std::fprintf(stderr, "alpha_texture_check: cannot open %s\n", argv[1]);
        return 3;
    }
    int32_t head[2] = {0, 0};
    bool ok = std::fread(head, 4, 2, fi) == 2 && head[0] >= 0 && head[1] >= 0;
    std::vector<nnbvh::AlphaTexDesc> tex(ok ? (size_t)head[0] : 0);
    uint64_t total = 0;
    for (size_t k = 0; ok && k < tex.size(); ++k) {
        uint32_t w[10];
        ok = std::fread(w, 4, 10, fi) == 10 && (int32_t)w[0] > 0 && (int32_t)w[1] > 0;
        if (!ok) break;
        nnbvh::AlphaTexDesc &d = tex[k];
        d.texelLo = (uint32_t)total;
        d.texelHi = (uint32_t)(total >> 32);
        d.width = (int32_t)w[0], d.height = (int32_t)w[1], d.wrap = (int32_t)w[2], d.pointFilter = (int32_t)w[3];
        std::memcpy(&d.su, &w[4], 4), std::memcpy(&d.sv, &w[5], 4), std::memcpy(&d.du, &w[6], 4);
        std::memcpy(&d.dv, &w[7], 4), std::memcpy(&d.scale, &w[8], 4);
        d.invert = (int32_t)w[9];
        total += (uint64_t)d.width * (uint64_t)d.height;
    }
    std::vector<float> pool(ok ? (size_t)total : 0), rec(ok ? (size_t)head[1] * 10 : 0);
    ok = ok && std::fread(pool.data(), 4, pool.size(), fi) == pool.size() &&
         std::fread(rec.data(), 4, rec.size(), fi) == rec.size();
    std::fclose(fi);
    for (size_t i = 0; ok && i < (size_t)head[1]; ++i) ok = rec[10 * i + 9] >= 0 && rec[10 * i + 9] < (float)tex.size();
    if (!ok) {
        std::fprintf(stderr, "alpha_texture_check: %s is not a record file\n", argv[1]);
        return 4;
    }
    std::vector<uint32_t> out((size_t)head[1]);
    for (size_t i = 0; i < out.size(); ++i) {
        const float *r = &rec[10 * i];
        const float a = nnbvh::alpha_texture_eval(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], tex[(size_t)r[9]],
                                                  pool.data());
        std::memcpy(&out[i], &a, 4);
    }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), 4, out.size(), fo) != out.size() || std::fclose(fo) != 0) {
        std::fprintf(stderr, "alpha_texture_check: cannot write %s\n", argv[2]);
        return 7;
    }
    return 0;
}
