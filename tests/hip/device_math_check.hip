// device_math_check.hip — TEST INFRASTRUCTURE ONLY.
//
// Batch driver around the PRODUCT's device arithmetic (nn_bvh_amd/csrc/trace_math.h, spawn_math.h, anim_math.h):
// the counterpart on the GPU of oracle/ref_leaf.cpp and oracle/ref_anim.cpp, with their command line, their file
// format and their record layouts, so that the golden vectors of tests/golden/ and the oracle's outputs compare with
// the device's column for column.  It includes the product headers and calls their functions; it restates none of
// them (the two exceptions, a loop and a quotient of the `wrs` mode, are marked where they stand).  Built and run by
// tests/test_device_math.py with the product's compiler flags (nn_bvh_amd.build.CFLAGS: -O3 -ffp-contract=off).
//
// usage: device_math_check MODE in.bin out.bin
//   in.bin : int32 n, then n records of float32
//   out.bin: n records of (1 + nout) uint32: a first word (the verdict where there is one) and nout raw float32 bits,
//            zero where the verdict is "miss" (as ref_leaf writes them)
//   MODE       record (floats)                                  first word, outputs
//   tri        o[3] d[3] tmax p0[3] p1[3] p2[3]            (16)  hit, b0 b1 b2 t      triangle_test, m = nullptr
//   tri_masks  as tri                                            as tri               triangle_test with the wave's RayMasks
//   blp        o[3] d[3] tmax p00[3] p10[3] p01[3] p11[3]  (19)  hit, u v t           patch_test
//   slab       o[3] d[3] tmax pmin[3] pmax[3]              (13)  slab_partial && tEntry < tmax,
//                                                                slab_entry_key(.., r) < tmax, slab_entry_key(.., r, masks) < tmax
//   slab2      as slab                                           hit, t0 t1           kd_root_interval
//   xfray      o[3] d[3] tmax m[16] mInv[16]               (39)  1, o'[3] d'[3] tmax' apply_inverse_ray, rows 0..2 of mInv
//   hash       a[3] b[3]                                    (6)  low word of hash_6f, hash_float_6f, high word
//   offset     pi_lo[3] pi_hi[3] n[3] w[3]                 (12)  1, offset_ray_origin[3], spawn_ray_to o[3] d[3]
//   wrs        p0[3] p1[3] nAdds                            (7)  selected index (-1: none), probability, weight sum
//   anim       nnbvh_animated_transform (114 words), time (115)  1, Interpolate(time).m rows 0..2 (12), .mInv rows 0..2 (12)
// One lane per record, blocks of one 64-lane wave.  Lanes past n carry a harmless ray and stay in the kernel until
// the wave-level ballots of ray_masks have been taken.
// Every HIP call is checked: an error is a message on stderr and a non-zero exit status.  Nothing is retried.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/nnbvh.h"
#include "nnbvh_internal.h"
#include "trace_math.h"
#include "spawn_math.h"
#include "anim_math.h"
#include "capi_internal.h"  // fill_anim_entry (host code of libnnbvh_hip.so, which this program links)

using namespace nnbvh;

enum Mode { kTri, kTriMasks, kBlp, kSlab, kSlab2, kXfRay, kHash, kOffset, kWrs, kAnim, kModes };
static const char *const kModeName[kModes] = {"tri", "tri_masks", "blp", "slab", "slab2", "xfray", "hash", "offset", "wrs", "anim"};
__host__ __device__ constexpr int kStrideOf(int m) {  // floats per record
    constexpr int s[kModes] = {16, 16, 19, 13, 13, 39, 6, 12, 7, 115};
    return s[m];
}
__host__ __device__ constexpr int kNoutOf(int m) {  // output words after the first
    constexpr int s[kModes] = {4, 4, 3, 2, 2, 7, 2, 9, 2, 24};
    return s[m];
}
constexpr int kAnimWords = (int)(sizeof(nnbvh_animated_transform) / 4);
static_assert(kAnimWords == 114 && sizeof(nnbvh_animated_transform) % 4 == 0, "the anim record is the C ABI's struct + time");

DEV V3 v3(const float *p) { return {p[0], p[1], p[2]}; }
DEV uint32_t bits(float f) { return __float_as_uint(f); }

// What the traversal kernels do when a lane takes up a ray (bvh_trace.hip, the refill trip; KD_BEGIN_RAY of
// kd_trace.hip): the reciprocals by three IEEE divisions, then the shear.
DEV void begin_ray(RayState &r, V3 o, V3 d) {
    r.o = o;
    r.inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};
    ray_shear(r, d);
}

template <int MODE>
__global__ __launch_bounds__(64) void check(const float *__restrict__ in, uint32_t *__restrict__ out, int n,
                                            const float *__restrict__ animTable, const float *__restrict__ animFwd) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    const bool live = i < n;
    const float *rec = in + (size_t)kStrideOf(MODE) * (live ? i : 0);
    uint32_t *o = out + (size_t)(1 + kNoutOf(MODE)) * (live ? i : 0);
    if constexpr (MODE == kTri || MODE == kTriMasks || MODE == kBlp || MODE == kSlab) {
        RayState r;
        V3 d = {1.0f, 1.0f, 1.0f};
        V3 org = {0.0f, 0.0f, 0.0f};
        float tMax = 0.0f;
        if (live) org = v3(rec), d = v3(rec + 3), tMax = rec[6];
        begin_ray(r, org, d);
        const RayMasks masks = ray_masks(r);  // every lane of the wave is here: the ballots see the whole wave
        if (!live) return;
        if constexpr (MODE == kTri || MODE == kTriMasks) {
            // the degenerate flag as the bakers take it: kd_triangle_is_degenerate (nnbvh_internal.h) is host + device
            // code and is called here as kd_bake.hip calls it; bvh_bake.hip evaluates the same expression
            const bool degenerate = kd_triangle_is_degenerate(rec + 7, rec + 10, rec + 13);
            float b0, b1, b2, t;
            const bool hit = triangle_test(r, tMax, degenerate, v3(rec + 7), v3(rec + 10), v3(rec + 13), b0, b1, b2, t,
                                           MODE == kTriMasks ? &masks : nullptr);
            o[0] = hit;
            if (hit) o[1] = bits(b0), o[2] = bits(b1), o[3] = bits(b2), o[4] = bits(t);
        } else if constexpr (MODE == kBlp) {
            float u, v, t;
            const bool hit = patch_test(r, d, tMax, v3(rec + 7), v3(rec + 10), v3(rec + 13), v3(rec + 16), u, v, t);
            o[0] = hit;
            if (hit) o[1] = bits(u), o[2] = bits(v), o[3] = bits(t);
        } else {
            float tEntry;
            const bool early = slab_partial(rec[7], rec[8], rec[9], rec[10], rec[11], rec[12], r, tEntry);
            o[0] = early && tEntry < tMax;
            o[1] = slab_entry_key(rec[7], rec[8], rec[9], rec[10], rec[11], rec[12], r) < tMax;
            o[2] = slab_entry_key(rec[7], rec[8], rec[9], rec[10], rec[11], rec[12], r, masks) < tMax;
        }
    } else {
        if (!live) return;
        if constexpr (MODE == kSlab2) {
            const V3 d = v3(rec + 3);
            const V3 inv = {1.0f / d.x, 1.0f / d.y, 1.0f / d.z};  // KD_BEGIN_RAY
            float t0, t1;
            const bool hit = kd_root_interval(rec + 7, rec + 10, v3(rec), inv, rec[6], t0, t1);
            o[0] = hit;
            if (hit) o[1] = bits(t0), o[2] = bits(t1);
        } else if constexpr (MODE == kXfRay) {
            const float *mi = rec + 23;
            float tMax = rec[6];
            V3 oo, dd;
            apply_inverse_ray({mi[0], mi[1], mi[2], mi[3]}, {mi[4], mi[5], mi[6], mi[7]}, {mi[8], mi[9], mi[10], mi[11]},
                              v3(rec), v3(rec + 3), tMax, oo, dd);
            o[0] = 1;
            o[1] = bits(oo.x), o[2] = bits(oo.y), o[3] = bits(oo.z);
            o[4] = bits(dd.x), o[5] = bits(dd.y), o[6] = bits(dd.z);
            o[7] = bits(tMax);
        } else if constexpr (MODE == kHash) {
            const uint64_t h = hash_6f(v3(rec), v3(rec + 3));
            o[0] = (uint32_t)h;
            o[1] = bits(hash_float_6f(v3(rec), v3(rec + 3)));
            o[2] = (uint32_t)(h >> 32);
        } else if constexpr (MODE == kOffset) {
            const V3 lo = v3(rec), hi = v3(rec + 3), nn = v3(rec + 6), w = v3(rec + 9);
            const V3 po = offset_ray_origin(lo, hi, nn, w);
            V3 so, sd;
            spawn_ray_to(lo, hi, nn, w, so, sd);
            o[0] = 1;
            o[1] = bits(po.x), o[2] = bits(po.y), o[3] = bits(po.z);
            o[4] = bits(so.x), o[5] = bits(so.y), o[6] = bits(so.z);
            o[7] = bits(sd.x), o[8] = bits(sd.y), o[9] = bits(sd.z);
        } else if constexpr (MODE == kWrs) {
            // The seed is taken as or_init takes it (wavefront2.hip) and the loop body is w2_or_item's reservoir update
            // (walk_math.h) with the candidate's index for its hit record.  The loop and the final quotient
            // (SampleProbability = reservoirWeight / weightSum, util/sampling.h) are a RESTATEMENT of the pass kernels'
            // text; what this mode pins is hash_6f -> pcg32_set_sequence -> pcg32_float and the `weight / weightSum`
            // comparison.
            Pcg32 g;
            pcg32_set_sequence(g, hash_6f(v3(rec), v3(rec + 3)));
            const int nAdds = (int)rec[6];
            float weightSum = 0.0f, selWeight = 0.0f;
            int sel = -1;
            for (int k = 0; k < nAdds; ++k) {
                const float weight = 1.0f;
                weightSum += weight;
                const float p = weight / weightSum;
                if (pcg32_float(g) < p) {
                    sel = k;
                    selWeight = weight;
                }
            }
            o[0] = (uint32_t)sel;
            o[1] = bits(sel >= 0 ? selWeight / weightSum : 0.0f);
            o[2] = bits(weightSum);
        } else if constexpr (MODE == kAnim) {
            const float *a = animTable + (size_t)kAnimStride * i, *fwd = animFwd + 24 * (size_t)i;
            float4 r0, r1, r2, f0, f1, f2;
            if (a[74] != 0.0f) {  // the kernels' own condition (interaction_math.h): actuallyAnimated
                anim_rows<true>(a, fwd, rec[kAnimWords], r0, r1, r2, f0, f1, f2);
            } else {
                // not animated: the kernels never call anim_rows (T, R, S are not set) and read the instance's static
                // matrices, which are the start transform's.  [50..61] = rows 0..2 of startTransform.mInv, [74] =
                // actuallyAnimated: the table layout of anim_math.h:23-26, to be kept in step with it
                r0 = {a[50], a[51], a[52], a[53]}, r1 = {a[54], a[55], a[56], a[57]}, r2 = {a[58], a[59], a[60], a[61]};
                f0 = {fwd[0], fwd[1], fwd[2], fwd[3]}, f1 = {fwd[4], fwd[5], fwd[6], fwd[7]}, f2 = {fwd[8], fwd[9], fwd[10], fwd[11]};
            }
            const float4 rows[6] = {f0, f1, f2, r0, r1, r2};
            o[0] = 1;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                o[1 + 4 * k] = bits(rows[k].x), o[2 + 4 * k] = bits(rows[k].y), o[3 + 4 * k] = bits(rows[k].z), o[4 + 4 * k] = bits(rows[k].w);
        }
    }
}

static bool ok(hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    std::fprintf(stderr, "device_math_check: %s: %s\n", what, hipGetErrorString(e));
    return false;
}

int main(int argc, char **argv) {
    int mode = -1;
    for (int k = 0; argc == 4 && k < kModes; ++k)
        if (!std::strcmp(argv[1], kModeName[k])) mode = k;
    if (mode < 0) {
        std::fprintf(stderr, "usage: device_math_check <tri|tri_masks|blp|slab|slab2|xfray|hash|offset|wrs|anim> in.bin out.bin\n");
        return 2;
    }
    FILE *fi = std::fopen(argv[2], "rb");
    if (!fi) {
        std::fprintf(stderr, "device_math_check: cannot open %s\n", argv[2]);
        return 3;
    }
    int32_t n = 0;
    const bool haveN = std::fread(&n, 4, 1, fi) == 1 && n >= 0;
    std::vector<float> in(haveN ? (size_t)n * kStrideOf(mode) : 0);
    const bool haveIn = haveN && std::fread(in.data(), 4, in.size(), fi) == in.size();
    std::fclose(fi);
    if (!haveIn) {
        std::fprintf(stderr, "device_math_check: %s is not `int32 n, n x %d float32`\n", argv[2], kStrideOf(mode));
        return 4;
    }
    const size_t outWords = (size_t)n * (1 + kNoutOf(mode));
    std::vector<uint32_t> out(outWords, 0u);
    if (n > 0) {
        // anim: the device table entries are made by the product's own host code, never laid out here
        std::vector<float> table, fwd;
        if (mode == kAnim) {
            table.assign((size_t)n * kAnimStride, 0.0f);
            fwd.assign((size_t)n * 24, 0.0f);
            for (int k = 0; k < n; ++k) {
                nnbvh_animated_transform a;
                std::memcpy(&a, &in[(size_t)k * kStrideOf(mode)], sizeof a);
                fill_anim_entry(a, &table[(size_t)k * kAnimStride]);
                std::memcpy(&fwd[(size_t)k * 24], a.start_from, 48);    // as nnbvh_shading_mesh_set_instances_animated
                std::memcpy(&fwd[(size_t)k * 24 + 12], a.end_from, 48);
            }
        }
        float *dIn = nullptr, *dTable = nullptr, *dFwd = nullptr;
        uint32_t *dOut = nullptr;
        if (!ok(hipMalloc((void **)&dIn, in.size() * 4), "hipMalloc(in)") ||
            !ok(hipMalloc((void **)&dOut, outWords * 4), "hipMalloc(out)") ||
            !ok(hipMemcpy(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(in)") ||
            !ok(hipMemset(dOut, 0, outWords * 4), "hipMemset(out)"))
            return 5;
        if (mode == kAnim &&
            (!ok(hipMalloc((void **)&dTable, table.size() * 4), "hipMalloc(anim table)") ||
             !ok(hipMalloc((void **)&dFwd, fwd.size() * 4), "hipMalloc(anim fwd)") ||
             !ok(hipMemcpy(dTable, table.data(), table.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(anim table)") ||
             !ok(hipMemcpy(dFwd, fwd.data(), fwd.size() * 4, hipMemcpyHostToDevice), "hipMemcpy(anim fwd)")))
            return 5;
        const dim3 grid((unsigned)((n + 63) / 64)), block(64);
#define LAUNCH(M)                                                                                 \
    case M:                                                                                       \
        hipLaunchKernelGGL(check<M>, grid, block, 0, 0, dIn, dOut, (int)n, dTable, dFwd);        \
        break;
        switch (mode) {
            LAUNCH(kTri) LAUNCH(kTriMasks) LAUNCH(kBlp) LAUNCH(kSlab) LAUNCH(kSlab2) LAUNCH(kXfRay) LAUNCH(kHash)
            LAUNCH(kOffset) LAUNCH(kWrs) LAUNCH(kAnim)
        }
#undef LAUNCH
        if (!ok(hipGetLastError(), "kernel launch") || !ok(hipDeviceSynchronize(), "kernel") ||
            !ok(hipMemcpy(out.data(), dOut, outWords * 4, hipMemcpyDeviceToHost), "hipMemcpy(out)"))
            return 6;
        if (!ok(hipFree(dIn), "hipFree") || !ok(hipFree(dOut), "hipFree") || (dTable && !ok(hipFree(dTable), "hipFree")) ||
            (dFwd && !ok(hipFree(dFwd), "hipFree")))
            return 6;
    }
    FILE *fo = std::fopen(argv[3], "wb");
    if (!fo || std::fwrite(out.data(), 4, out.size(), fo) != out.size() || std::fclose(fo) != 0) {
        std::fprintf(stderr, "device_math_check: cannot write %s\n", argv[3]);
        return 7;
    }
    return 0;
}
