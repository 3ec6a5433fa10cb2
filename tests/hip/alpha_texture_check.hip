// alpha_texture_check (device) — nn_bvh_amd/csrc/alpha_texture_math.h evaluated in a kernel, one record per lane, over
// the record file tests/cpp/alpha_texture_check.cpp reads (see there).  Output: the bit pattern of alpha per record.
// Every texture index is checked against the table on the host before the launch; the header keeps every tap inside
// the texture.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "alpha_texture_math.h"

__global__ void eval_records(const float *rec, int n, const nnbvh::AlphaTexDesc *tex, const float *pool, uint32_t *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *r = rec + 10 * (long)i;
    out[i] = __float_as_uint(nnbvh::alpha_texture_eval(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], tex[(int)r[9]], pool));
}

static bool ok_hip(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    std::fprintf(stderr, "alpha_texture_check: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

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
    const int n = head[1];
    std::vector<uint32_t> out((size_t)n, 0u);
    if (n > 0) {
        float *dRec = nullptr, *dPool = nullptr;
        nnbvh::AlphaTexDesc *dTex = nullptr;
        uint32_t *dOut = nullptr;
        if (!ok_hip(hipMalloc((void **)&dRec, rec.size() * 4), "hipMalloc(records)") ||
            !ok_hip(hipMalloc((void **)&dPool, pool.size() * 4), "hipMalloc(texels)") ||
            !ok_hip(hipMalloc((void **)&dTex, tex.size() * sizeof(nnbvh::AlphaTexDesc)), "hipMalloc(textures)") ||
            !ok_hip(hipMalloc((void **)&dOut, out.size() * 4), "hipMalloc(out)") ||
            !ok_hip(hipMemcpy(dRec, rec.data(), rec.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(records)") ||
            !ok_hip(hipMemcpy(dPool, pool.data(), pool.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(texels)") ||
            !ok_hip(hipMemcpy(dTex, tex.data(), tex.size() * sizeof(nnbvh::AlphaTexDesc), hipMemcpyHostToDevice), "hipMemcpy(textures)") ||
            !ok_hip(hipMemset(dOut, 0, out.size() * 4), "hipMemset(out)"))
            return 5;
        hipLaunchKernelGGL(eval_records, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, 0, dRec, n, dTex, dPool, dOut);
        if (!ok_hip(hipGetLastError(), "kernel launch") || !ok_hip(hipDeviceSynchronize(), "kernel") ||
            !ok_hip(hipMemcpy(out.data(), dOut, out.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy(out)"))
            return 6;
        (void)hipFree(dRec), (void)hipFree(dPool), (void)hipFree(dTex), (void)hipFree(dOut);
    }
    FILE *fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), 4, out.size(), fo) != out.size() || std::fclose(fo) != 0) {
        std::fprintf(stderr, "alpha_texture_check: cannot write %s\n", argv[2]);
        return 7;
    }
    return 0;
}
