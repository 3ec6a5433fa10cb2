// bvh_build_gpu.hip — HLBVH construction on the MI355X, producing the SAME flattened tree as the
// host builder's NNBVH_SPLIT_HLBVH (bvh_build.cpp), i.e. the reference's buildHLBVH
// (/root/reference/src/pbrt/cpu/aggregates.cpp:389-503) with treelets emitted in Morton order.
//
// The reference recursion (emitLBVH, :451-503) is replaced by its closed form.  Inside a treelet
// (primitives sharing the top 12 Morton bits) emitLBVH splits a sorted range at the highest bit in
// which its codes differ, stops at ranges of fewer than maxPrimsInNode primitives, and makes one
// leaf of any run of identical codes.  That is the binary radix tree over the DISTINCT codes
// (Karras 2012: every internal node's range and split found independently by binary searches on
// common-prefix lengths), cut off where a range gets smaller than maxPrimsInNode:
//
//   1  primitive bounds, centroid bounds            k_prim_bounds     (streaming, one pass)
//   2  30-bit Morton codes (aggregates.cpp:398-408)  k_morton         (many objects: first their centroid
//                                                                      bounds, k_cbounds_init + k_object_cbounds)
//   3  stable radix sort of (key, index)            rocPRIM          (the reference's own 5x6-bit
//                                                                      LSD sort is stable too)
//   4  distinct codes ("atoms") and their ranges    k_heads + scan + k_compact
//   5  radix tree over the atoms                    k_karras
//   6  which radix nodes survive as real nodes      k_classify + 2 scans (leaf / treelet ordinals)
//   7  bounds bottom-up: leaves, then interior nodes by split bit 0..17 (children always split at
//      a lower bit, so 18 dependency-free launches; no atomics, no intra-kernel fences)
//   8  treelet roots (k_treelets), then buildUpperSAH over an object's <= 4096 boxes (aggregates.cpp:626-723):
//      k_upper_treelets, k_upper_seed, k_upper_pass per pass; the upper nodes join the array with k_upper_nodes
//   9  every node computes its own DFS position   k_emit: preorder = 2 x (leaves to its left in
//      the treelet) + (ancestors it hangs off on the left side), found by walking <= 18 parents
//  10  leaf-ordered primitive table = the sorted order  k_gather_prims
//
// Everything is integer / min / max work on 4-32 B records: HBM-bound streaming except the two
// pointer walks (5, 9), which touch a handful of L2-resident words per node.
// The trees of many objects come from the same ten steps run once over all their primitives (gpu_hlbvh_forest_device;
// one tree is its one-object case).  The sort key is (object << 30) | code: the object's number above the code keeps
// every primitive, run of equal codes, treelet and radix-tree range inside its object, and steps 2, 6, 8 and 9 read it
// back to find a node's object (its centroid bounds, its error word, its first node and primitive, its depth).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bvh_build_gpu.h"

namespace nnbvh {
namespace {

constexpr int kB = 256;
constexpr int kTreeletBit = 18;  // bits >= 18 separate treelets (mask 0x3ffc0000, aggregates.cpp:423)

enum : int { kErrVertex = 1, kErrNeedBounds = 2, kErrKind = 3, kErrLeafSize = 4, kErrNonFinite = 5, kErrSahCosts = 6 };
// The builders' error words, one per kind above: errObj[kind] = the lowest-numbered object that raised it
// (atomicMin; kNoObject = nobody), so a forest reports what a loop over its objects would have stopped at.
// errObj[0] is a plain word for the "cannot happen" codes.
constexpr int kErrWords = 8;
constexpr int kNoObject = 0x7fffffff;
enum : unsigned char { kRealInterior = 1, kRealLeaf = 2, kTreeletRoot = 4 };

struct Box6 {
    float mn[3], mx[3];
};

// std::min / std::max as the host builder's Box::add applies them (first of equals is kept)
__device__ __forceinline__ float min_keep(float a, float b) { return b < a ? b : a; }
__device__ __forceinline__ float max_keep(float a, float b) { return a < b ? b : a; }
__device__ __forceinline__ void box_init(Box6 &b) {  // Bounds3() (util/vecmath.h:1259-1264)
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = 3.402823466e+38f;
        b.mx[k] = -3.402823466e+38f;
    }
}
__device__ __forceinline__ void box_add(Box6 &b, const float *p) {
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = min_keep(b.mn[k], p[k]);
        b.mx[k] = max_keep(b.mx[k], p[k]);
    }
}
__device__ __forceinline__ void box_add(Box6 &b, const Box6 &o) {
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = min_keep(b.mn[k], o.mn[k]);
        b.mx[k] = max_keep(b.mx[k], o.mx[k]);
    }
}

// order-preserving float <-> unsigned map, for atomicMin/Max on floats
__device__ __forceinline__ unsigned f2key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key2f(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- 1: primitive bounds (Triangle::Bounds / BilinearPatch::Bounds = union of the vertices,
// shapes.cpp:294-300, 1073-1081) and the bounds of their centroids (aggregates.cpp:391-394) ------
__global__ __launch_bounds__(kB) void k_prim_bounds(const nnbvh_prim *__restrict__ prims,
                                                    const float *__restrict__ verts, int nVerts,
                                                    const float *__restrict__ callerBounds, int n,
                                                    Box6 *__restrict__ pb, unsigned *cbKeys,
                                                    const int *__restrict__ objectFirst, int nObjects,
                                                    int *errObj) {
    __shared__ float red[6][kB / 64];
    auto report = [&](int kind, int i) {  // errObj, with objectFirst[nObjects + 1]: see kErrWords
        int lo = 0, hi = nObjects - 1;  // the object of primitive i: the last k with objectFirst[k] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (objectFirst[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        atomicMin(&errObj[kind], lo);
    };
    float cmin[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
    float cmax[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB) {
        const nnbvh_prim p = prims[i];
        Box6 b;
        box_init(b);
        const int nv = (p.kind == NNBVH_PRIM_TRIANGLE || (p.kind >= NNBVH_PRIM_ALPHA_TRIANGLE && p.kind <= NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED) || (p.kind >= NNBVH_PRIM_ALPHATEX_TRIANGLE && p.kind <= NNBVH_PRIM_ALPHATEX_TRIANGLE_SMOOTH_FLIPPED)) ? 3 : ((p.kind == NNBVH_PRIM_BILINEAR_PATCH || (p.kind >= NNBVH_PRIM_ALPHA_PATCH && p.kind <= NNBVH_PRIM_ALPHA_PATCH_UV_SMOOTH_FLIPPED)) ? 4 : 0);
        if (p.kind == NNBVH_PRIM_INSTANCE || p.kind == NNBVH_PRIM_HOST) {
            if (!callerBounds) {
                report(kErrNeedBounds, i);
            } else {
                box_add(b, callerBounds + 6 * (long)i);
                box_add(b, callerBounds + 6 * (long)i + 3);
            }
        } else if (nv == 0) {
            report(kErrKind, i);
        }
        for (int k = 0; k < nv; ++k) {
            const int vi = p.v[k];
            if (vi < 0 || vi >= nVerts) {
                report(kErrVertex, i);
                continue;
            }
            box_add(b, verts + 3 * (long)vi);
        }
        // non-finite coordinates (Inf / NaN vertices or caller bounds) are malformed input: the
        // bucket index int(nBuckets * offset) of aggregates.cpp:254-258 is undefined for them
        for (int k = 0; k < nv; ++k) {
            const int vi = p.v[k];
            if (vi < 0 || vi >= nVerts) continue;
            const float *v = verts + 3 * (long)vi;
            if (!(__builtin_isfinite(v[0]) && __builtin_isfinite(v[1]) && __builtin_isfinite(v[2]))) report(kErrNonFinite, i);
        }
        if ((p.kind == NNBVH_PRIM_INSTANCE || p.kind == NNBVH_PRIM_HOST) && callerBounds) {
            const float *c = callerBounds + 6 * (long)i;
            for (int k = 0; k < 6; ++k)
                if (!__builtin_isfinite(c[k])) report(kErrNonFinite, i);
        }
        pb[i] = b;
        for (int k = 0; k < 3; ++k) {
            const float c = .5f * b.mn[k] + .5f * b.mx[k];  // BVHPrimitive::Centroid()
            cmin[k] = fminf(cmin[k], c);
            cmax[k] = fmaxf(cmax[k], c);
        }
    }
    // block reduction (values only: the sign of a zero does not reach the Morton codes)
    for (int k = 0; k < 3; ++k)
        for (int off = 32; off >= 1; off >>= 1) {
            cmin[k] = fminf(cmin[k], __shfl_xor(cmin[k], off));
            cmax[k] = fmaxf(cmax[k], __shfl_xor(cmax[k], off));
        }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
        for (int k = 0; k < 3; ++k) {
            red[k][wave] = cmin[k];
            red[3 + k][wave] = cmax[k];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = red[threadIdx.x][0];
        for (int w = 1; w < kB / 64; ++w)
            v = threadIdx.x < 3 ? fminf(v, red[threadIdx.x][w]) : fmaxf(v, red[threadIdx.x][w]);
        if (threadIdx.x < 3) atomicMin(&cbKeys[threadIdx.x], f2key(v));
        else atomicMax(&cbKeys[threadIdx.x], f2key(v));
    }
}

// ---- 2: Morton codes (aggregates.cpp:398-408; EncodeMorton3 / LeftShift3 util/math.h:99-119;
// Bounds3::Offset util/vecmath.h:1322-1331) --------------------------------------------------------
__device__ __forceinline__ unsigned left_shift3(unsigned x) {
    if (x == (1u << 10)) --x;
    x = (x | (x << 16)) & 0b00000011000000000000000011111111u;
    x = (x | (x << 8)) & 0b00000011000000001111000000001111u;
    x = (x | (x << 4)) & 0b00000011000011000011000011000011u;
    x = (x | (x << 2)) & 0b00001001001001001001001001001001u;
    return x;
}

// Centroid bounds of every object (order-free min / max of the same centroids k_prim_bounds folds for the whole input;
// with one object those are the bounds, and this kernel does not run), and the object of every primitive for k_morton.
// A wavefront that lies inside one object (every wavefront of a big object, bar two) folds first and sends six atomics
// instead of 384.
__global__ __launch_bounds__(kB) void k_object_cbounds(const Box6 *__restrict__ pb, const int *__restrict__ objectFirst,
                                                       int nObjects, int n, int *__restrict__ objOf, unsigned *cbObj) {
    const int i = blockIdx.x * kB + threadIdx.x;
    const bool live = i < n;
    int obj = -1;
    float cmin[3] = {3.402823466e+38f, 3.402823466e+38f, 3.402823466e+38f};
    float cmax[3] = {-3.402823466e+38f, -3.402823466e+38f, -3.402823466e+38f};
    if (live) {
        int lo = 0, hi = nObjects - 1;  // the last k with objectFirst[k] <= i
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (objectFirst[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        obj = lo;
        objOf[i] = obj;
        const Box6 b = pb[i];
        for (int k = 0; k < 3; ++k) cmin[k] = cmax[k] = .5f * b.mn[k] + .5f * b.mx[k];  // BVHPrimitive::Centroid()
    }
    const int obj0 = __shfl(obj, 0);
    if (obj0 < 0) return;  // lane 0 holds the wavefront's lowest index: nobody is live
    if (__all(!live || obj == obj0)) {
        for (int k = 0; k < 3; ++k)
            for (int off = 32; off >= 1; off >>= 1) {
                cmin[k] = fminf(cmin[k], __shfl_xor(cmin[k], off));
                cmax[k] = fmaxf(cmax[k], __shfl_xor(cmax[k], off));
            }
        if ((threadIdx.x & 63) != 0) return;
    } else if (!live) {
        return;
    }
    for (int k = 0; k < 3; ++k) {
        atomicMin(&cbObj[6 * (size_t)obj + k], f2key(cmin[k]));
        atomicMax(&cbObj[6 * (size_t)obj + 3 + k], f2key(cmax[k]));
    }
}

__global__ __launch_bounds__(kB) void k_cbounds_init(int nObjects, unsigned *__restrict__ cbObj) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i < 6 * nObjects) cbObj[i] = (i % 6) < 3 ? 0xffffffffu : 0u;  // min keys all-ones, max keys 0
}

// The code against the object's own centroid bounds (cbObj[6 obj ..]: min keys, max keys; the mx > mn guard per object
// and per axis), the object number above the 30 code bits.  objOf == nullptr: everything is object 0.
template <typename Key>
__global__ __launch_bounds__(kB) void k_morton(const Box6 *__restrict__ pb, const unsigned *__restrict__ cbObj,
                                               const int *__restrict__ objOf, int n, Key *__restrict__ keys,
                                               int *__restrict__ idx) {
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB) {
        const Box6 b = pb[i];
        const int obj = objOf ? objOf[i] : 0;
        const unsigned *cb = cbObj + 6 * (size_t)obj;
        unsigned q[3];
        for (int k = 0; k < 3; ++k) {
            const float mn = key2f(cb[k]), mx = key2f(cb[3 + k]);
            const float c = .5f * b.mn[k] + .5f * b.mx[k];
            float o = c - mn;
            if (mx > mn) o /= mx - mn;
            q[k] = (unsigned)(o * 1024.0f);  // mortonScale = 1 << 10
        }
        const unsigned code = (left_shift3(q[2]) << 2) | (left_shift3(q[1]) << 1) | left_shift3(q[0]);
        keys[i] = ((Key)obj << 30) | code;
        idx[i] = i;
    }
}

// ---- 4: runs of identical codes -------------------------------------------------------------------
// Key = (object << 30) | code: a run of identical keys ends at an object boundary and every object is one subtree of
// the radix tree below.  unsigned long long; unsigned for one object, whose keys are its 30-bit codes.
template <typename Key>
__global__ __launch_bounds__(kB) void k_heads(const Key *__restrict__ codes, int n, int *__restrict__ head) {
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB)
        head[i] = (i == 0 || codes[i] != codes[i - 1]) ? 1 : 0;
}

template <typename Key>
__global__ __launch_bounds__(kB) void k_compact(const Key *__restrict__ codes,
                                                const int *__restrict__ head,
                                                const int *__restrict__ excl, int n,
                                                int *__restrict__ pstart, Key *__restrict__ ucode,
                                                int *mOut) {
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB) {
        if (head[i]) {
            pstart[excl[i]] = i;
            ucode[excl[i]] = codes[i];
        }
        if (i == n - 1) {
            const int m = excl[i] + head[i];
            *mOut = m;
            pstart[m] = n;
        }
    }
}

// ---- 5: binary radix tree over the m distinct codes.  Internal node i in [0, m-1); node index
// space "v": internal nodes 0..m-2, atom a -> (m-1)+a.  Split position == the reference's
// FindInterval result (first element whose bit differs from the range's first, :478-482). --------
// A forest's keys split on bits >= 30 above its objects (bit[] then holds 30 .. 60: outside every treelet, like the
// bits 18 .. 29 between an object's treelets); below an object's root the tree is the one its codes alone give.
__device__ __forceinline__ int key_clz(unsigned x) { return __clz((int)x); }
__device__ __forceinline__ int key_clz(unsigned long long x) { return __clzll((long long)x); }

template <typename Key>
__global__ __launch_bounds__(kB) void k_karras(const Key *__restrict__ ucode, int m,
                                               int *__restrict__ firstA, int *__restrict__ lastA,
                                               int *__restrict__ leftV, int *__restrict__ rightV,
                                               unsigned char *__restrict__ bit,
                                               int *__restrict__ parentV) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= m - 1) return;
    const Key ci = ucode[i];
    auto delta = [&](int j) -> int { return (j < 0 || j >= m) ? -1 : key_clz((Key)(ci ^ ucode[j])); };
    const int d = (delta(i + 1) - delta(i - 1)) > 0 ? 1 : -1;
    const int dmin = delta(i - d);
    int lmax = 2;
    while (delta(i + lmax * d) > dmin) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta(i + (l + t) * d) > dmin) l += t;
    const int j = i + l * d;
    const int dnode = delta(j);
    int s = 0, t = l;
    do {
        t = (t + 1) / 2;
        if (delta(i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    const int gamma = i + s * d + (d < 0 ? d : 0);
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    const int lv = (lo == gamma) ? (m - 1) + gamma : gamma;
    const int rv = (hi == gamma + 1) ? (m - 1) + gamma + 1 : gamma + 1;
    firstA[i] = lo;
    lastA[i] = hi;
    leftV[i] = lv;
    rightV[i] = rv;
    bit[i] = (unsigned char)((int)(8 * sizeof(Key)) - 1 - dnode);
    parentV[lv] = i;
    parentV[rv] = i;
    if (i == 0) parentV[0] = -1;
}

// ---- 6: which radix nodes are nodes of the reference's tree --------------------------------------
// internal node: interior iff it lies inside a treelet (split bit < 18) and holds >= maxPrims
// primitives (emitLBVH's leaf rule, :453).  Any node inside a treelet whose parent is such an
// interior node (or which is its treelet's root) and which is not interior itself is a leaf.
// An oversized leaf is reported with its object (errObj[kErrLeafSize], lowest object wins).
template <typename Key>
__global__ __launch_bounds__(kB) void k_classify(int m, int maxPrims, const int *__restrict__ pstart,
                                                 const int *__restrict__ firstA, const int *__restrict__ lastA,
                                                 const unsigned char *__restrict__ bit, const int *__restrict__ parentV,
                                                 const Key *__restrict__ ukey, unsigned char *__restrict__ kind,
                                                 int *__restrict__ leafHead, int *__restrict__ treeletHead, int *errObj) {
    const int v = blockIdx.x * kB + threadIdx.x;
    if (v >= 2 * m - 1) return;
    const bool internal = v < m - 1;
    const int first = internal ? firstA[v] : v - (m - 1);
    const int last = internal ? lastA[v] : first;
    const int n = pstart[last + 1] - pstart[first];
    const int p = parentV[v];
    const bool inTreelet = !internal || bit[v] < kTreeletBit;
    const bool parentInTreelet = p >= 0 && bit[p] < kTreeletBit;
    const bool treeletRoot = inTreelet && !parentInTreelet;
    const bool realInterior = internal && inTreelet && n >= maxPrims;
    bool parentInterior = false;
    if (parentInTreelet) parentInterior = pstart[lastA[p] + 1] - pstart[firstA[p]] >= maxPrims;
    const bool realLeaf = inTreelet && !realInterior && (treeletRoot || parentInterior);
    kind[v] = (realInterior ? kRealInterior : 0) | (realLeaf ? kRealLeaf : 0) | (treeletRoot ? kTreeletRoot : 0);
    if (realLeaf) {
        leafHead[first] = 1;
        if (n > 65535) atomicMin(&errObj[kErrLeafSize], (int)(ukey[first] >> 30));  // LinearBVHNode::nPrimitives is 16 bits (:134)
    }
    if (treeletRoot) treeletHead[first] = 1;
}

// ---- 7: bounds ---------------------------------------------------------------------------------------
constexpr int kBigLeaf = 64;  // leaves above this size are folded by a whole wavefront

__global__ __launch_bounds__(kB) void k_leaf_bounds(int m, const unsigned char *__restrict__ kind,
                                                    const int *__restrict__ pstart,
                                                    const int *__restrict__ firstA,
                                                    const int *__restrict__ lastA,
                                                    const int *__restrict__ idxSorted,
                                                    const Box6 *__restrict__ pb,
                                                    Box6 *__restrict__ nodeBox) {
    const int v = blockIdx.x * kB + threadIdx.x;
    if (v >= 2 * m - 1 || !(kind[v] & kRealLeaf)) return;
    const bool internal = v < m - 1;
    const int first = internal ? firstA[v] : v - (m - 1);
    const int last = internal ? lastA[v] : first;
    const int begin = pstart[first], end = pstart[last + 1];
    if (end - begin > kBigLeaf) return;  // k_big_leaf_bounds
    Box6 b;
    box_init(b);
    for (int j = begin; j < end; ++j) box_add(b, pb[idxSorted[j]]);  // :456-463
    nodeBox[v] = b;
}

// One wavefront per large leaf (runs of identical Morton codes can hold thousands of primitives).
// The result must equal the sequential fold's, which keeps the FIRST of equal values (+0 / -0):
// lanes fold contiguous chunks in order, and the cross-lane reduction always combines
// (lower lane = earlier elements) on the left.
__global__ __launch_bounds__(kB) void k_big_leaf_bounds(int m, const unsigned char *__restrict__ kind,
                                                        const int *__restrict__ pstart,
                                                        const int *__restrict__ firstA,
                                                        const int *__restrict__ lastA,
                                                        const int *__restrict__ idxSorted,
                                                        const Box6 *__restrict__ pb,
                                                        Box6 *__restrict__ nodeBox) {
    const int v = blockIdx.x * (kB / 64) + (threadIdx.x >> 6);  // wave-uniform
    if (v >= 2 * m - 1 || !(kind[v] & kRealLeaf)) return;
    const bool internal = v < m - 1;
    const int first = internal ? firstA[v] : v - (m - 1);
    const int last = internal ? lastA[v] : first;
    const int begin = pstart[first], n = pstart[last + 1] - begin;
    if (n <= kBigLeaf) return;
    const int lane = threadIdx.x & 63;
    const int chunk = (n + 63) / 64;
    const int lo = lane * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    Box6 b;
    box_init(b);
    for (int j = lo; j < hi; ++j) box_add(b, pb[idxSorted[begin + j]]);
    for (int off = 1; off < 64; off <<= 1) {
        Box6 o;
        for (int k = 0; k < 3; ++k) {
            o.mn[k] = __shfl_down(b.mn[k], off);
            o.mx[k] = __shfl_down(b.mx[k], off);
        }
        if (lane + off < 64) box_add(b, o);  // b = earlier elements (kept on ties), o = later ones
    }
    if (lane == 0) nodeBox[v] = b;
}

__global__ __launch_bounds__(kB) void k_interior_bounds(int m, int level,
                                                        const unsigned char *__restrict__ kind,
                                                        const unsigned char *__restrict__ bit,
                                                        const int *__restrict__ leftV,
                                                        const int *__restrict__ rightV,
                                                        Box6 *nodeBox) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= m - 1 || !(kind[i] & kRealInterior) || bit[i] != level) return;
    Box6 b;
    box_init(b);
    box_add(b, nodeBox[leftV[i]]);  // :495-498 Union(child0, child1)
    box_add(b, nodeBox[rightV[i]]);
    nodeBox[i] = b;
}

// ---- 8: treelet table for the upper SAH build (8b below) -------------------------------------------------
__device__ __forceinline__ int subtree_size(int v, int m, const unsigned char *kind, const int *firstA,
                                            const int *lastA, const int *leafOrd) {
    if (!(kind[v] & kRealInterior)) return 1;
    return 2 * (leafOrd[lastA[v] + 1] - leafOrd[firstA[v]]) - 1;
}

// Every treelet's box, node count and object: the treelets are numbered object after object, Morton order inside
template <typename Key>
__global__ __launch_bounds__(kB) void k_treelets(int m, const unsigned char *__restrict__ kind,
                                                 const int *__restrict__ firstA, const int *__restrict__ lastA,
                                                 const int *__restrict__ leafOrd, const int *__restrict__ treeOrd,
                                                 const Box6 *__restrict__ nodeBox, const Key *__restrict__ ukey, int tCap,
                                                 Box6 *__restrict__ tbox, int *__restrict__ tsize, int *__restrict__ tobj) {
    const int v = blockIdx.x * kB + threadIdx.x;
    if (v >= 2 * m - 1 || !(kind[v] & kTreeletRoot)) return;
    const int first = v < m - 1 ? firstA[v] : v - (m - 1);
    const int t = treeOrd[first];
    if (t >= tCap) return;  // cannot happen: at most min(m, 4096 per object) treelets
    tbox[t] = nodeBox[v];
    tsize[t] = subtree_size(v, m, kind, firstA, lastA, leafOrd);
    tobj[t] = (int)(ukey[first] >> 30);
}

// ---- 9: flattenBVH's DFS order (aggregates.cpp:505-522) without a traversal ---------------------------
// The trees lie one after another: tbase[t] already includes the tree's node_first; a second child counts from its
// own tree's root, a leaf's first primitive from its object's first primitive, the depth is the object's own maximum
__global__ __launch_bounds__(kB) void k_emit(int m, const unsigned char *__restrict__ kind,
                                             const unsigned char *__restrict__ bit, const int *__restrict__ pstart,
                                             const int *__restrict__ firstA, const int *__restrict__ lastA,
                                             const int *__restrict__ leftV, const int *__restrict__ parentV,
                                             const int *__restrict__ leafOrd, const int *__restrict__ treeOrd,
                                             const int *__restrict__ tbase, const int *__restrict__ tdepth,
                                             const int *__restrict__ tobj, const int *__restrict__ nodeFirst,
                                             const int *__restrict__ objectFirst, const Box6 *__restrict__ nodeBox,
                                             nnbvh_linear_node *__restrict__ nodes, int *depthObj) {
    const int v = blockIdx.x * kB + threadIdx.x;
    int obj = -1, leafDepth = -1;  // of a leaf
    if (v < 2 * m - 1 && (kind[v] & (kRealInterior | kRealLeaf))) {
        const bool internal = v < m - 1;
        const int first = internal ? firstA[v] : v - (m - 1);
        const int last = internal ? lastA[v] : first;
        int cur = v, leftTurns = 0, depth = 0;
        while (!(kind[cur] & kTreeletRoot)) {
            const int p = parentV[cur];
            leftTurns += (leftV[p] == cur) ? 1 : 0;
            ++depth;
            cur = p;
        }
        const int rootFirst = cur < m - 1 ? firstA[cur] : cur - (m - 1);
        const int t = treeOrd[rootFirst];
        const int flat = tbase[t] + 2 * (leafOrd[first] - leafOrd[rootFirst]) + leftTurns;
        const Box6 b = nodeBox[v];
        nnbvh_linear_node out;
        for (int k = 0; k < 3; ++k) {
            out.pmin[k] = b.mn[k];
            out.pmax[k] = b.mx[k];
        }
        out.pad = 0;
        if (kind[v] & kRealLeaf) {
            obj = tobj[t];
            out.offset = pstart[first] - objectFirst[obj];
            out.nprims = (uint16_t)(pstart[last + 1] - pstart[first]);
            out.axis = 0;
            leafDepth = tdepth[t] + depth;
        } else {
            out.offset = flat + 1 + subtree_size(leftV[v], m, kind, firstA, lastA, leafOrd) - nodeFirst[tobj[t]];
            out.nprims = 0;
            out.axis = (uint8_t)(bit[v] % 3);  // :499
        }
        nodes[flat] = out;
    }
    // The object's depth.  A wavefront whose leaves are all of one object (every wavefront inside a big object) folds
    // first and sends one atomicMax instead of up to 64 to the same word; the plain read spares most of those as well.
    const unsigned long long leaves = __ballot(leafDepth >= 0);
    if (!leaves) return;
    const int obj0 = __shfl(obj, __ffsll((long long)leaves) - 1);
    if (__all(leafDepth < 0 || obj == obj0)) {
        for (int off = 32; off >= 1; off >>= 1) {
            const int o = __shfl_xor(leafDepth, off);
            leafDepth = o > leafDepth ? o : leafDepth;
        }
        if ((threadIdx.x & 63) != 0) return;
        obj = obj0;
    } else if (leafDepth < 0) {
        return;
    }
    if (depthObj[obj] < leafDepth) atomicMax(&depthObj[obj], leafDepth);
}

// ---- 10 ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void k_gather_prims(const nnbvh_prim *__restrict__ prims,
                                                     const int *__restrict__ idxSorted, int n,
                                                     nnbvh_prim *__restrict__ ordered) {
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB)
        ordered[i] = prims[idxSorted[i]];
}

__global__ __launch_bounds__(kB) void k_iota(int n, int *__restrict__ perm) {
    for (int i = blockIdx.x * kB + threadIdx.x; i < n; i += gridDim.x * kB) perm[i] = i;
}

// ---- 8b: buildUpperSAH (aggregates.cpp:626-723) over every object's treelets, on the device ---------------------------
// The host's upper() (bvh_build.cpp) top-down, without knowing the tree below a node: a range of n treelets yields
// n - 1 upper nodes, so the subtree of the range [s, e) of the permuted treelet order holds sum(tsize) + (e - s - 1)
// nodes, a first child stands at its parent's index + 1 and a second child behind the first child's subtree.
//   k_upper_treelets  per treelet: its object's first treelet and node total, the host's checks of the table
//   (scan)            node_first = exclusive sum of the objects' node totals
//   k_upper_seed      per object: one treelet = its root; more = one range for the first pass
//   k_upper_pass      one wavefront per range.  A range of at most 64 treelets: its whole subtree (pending second
//                     children on a stack in LDS, at most 63).  A larger one: one split, the children go to the
//                     next pass's queue.  Every pass works on all such ranges of all objects.
//   k_upper_nodes     (after the node array exists) one wavefront per upper node: its box, and the node
// Decisions (split dimension, the 11 costs, the first minimum, bucket <= best) depend on VALUES only: min / max of the
// range's boxes and centroids, integer counts, and the host's float expressions operation for operation
// (-ffp-contract=off); the sign of a zero changes no comparison, and a zero surface area of the range's bounds makes
// every cost NaN whatever its sign.  Two things depend on ORDER.  The treelets' order, which std::partition leaves
// behind: libstdc++'s closed form, as in the SAH builder below (left-part offenders from the left trade places with
// right-part offenders from the right).  And a stored box's zero signs: the host folds child 0 then child 1 with
// Box::add (first of equals kept), which is the in-order fold over the node's range in the FINAL treelet order;
// k_upper_nodes does that fold after the last pass.
// Every loop is bounded: a split with an empty side, or coinciding centroids, flags the object (errUpper, lowest object
// wins) and queues nothing, so each range a pass takes up is strictly smaller than the one it came from.
constexpr int kUpperBuckets = 12;
constexpr int kUpperWave = 64;        // a range of at most this many treelets is finished by one wavefront
constexpr int kUpperMaxTreelets = 4096;  // an object's treelets: 12 Morton bits
constexpr int kUpperMaxPasses = kUpperMaxTreelets;  // every pass shrinks every range by at least one treelet

struct UpperRange {
    int s, e;    // positions in the permuted treelet order
    int rel;     // the subtree's root, counted from its tree's root
    int depth;
};
struct UpperSplit {  // of the upper node that splits [s, e) at position mid: stored at [mid], e == 0 = none
    int s, e, rel, second, axis;
};
enum : int { kUpErrCount = 0, kUpErrTable = 1, kUpErrInternal = 2, kUpQueue = 4 };  // words of the upper build's scalars

__device__ __forceinline__ float box_area(const Box6 &b) {  // util/vecmath.h:1293-1296
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    return 2 * (dx * dy + dx * dz + dy * dz);
}
__device__ __forceinline__ int box_maxdim(const Box6 &b) {  // util/vecmath.h:1305-1313
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    if (dx > dy && dx > dz) return 0;
    else if (dy > dz) return 1;
    else return 2;
}
// bucket_of in upper(): the centroid is (mn + mx) * 0.5f here, not BVHPrimitive::Centroid()
__device__ __forceinline__ int upper_bucket(const Box6 &b, int dim, float cmn, float cmx) {
    const float centroid = (b.mn[dim] + b.mx[dim]) * 0.5f;
    int k = kUpperBuckets * ((centroid - cmn) / (cmx - cmn));
    if (k == kUpperBuckets) k = kUpperBuckets - 1;
    // beyond only where the centroids overflow (the host indexes out of range there): no index leaves the table
    return k < 0 ? 0 : (k > kUpperBuckets - 1 ? kUpperBuckets - 1 : k);
}

__global__ __launch_bounds__(kB) void k_upper_treelets(int nTreelets, int nObjects, const Box6 *__restrict__ tbox,
                                                       const int *__restrict__ tsize, const int *__restrict__ tobj,
                                                       int *__restrict__ perm, int *__restrict__ objTreelet,
                                                       unsigned *objNodes, int *scal) {
    const int t = blockIdx.x * kB + threadIdx.x;
    if (t >= nTreelets) return;
    perm[t] = t;
    const int obj = tobj[t];
    if (obj < 0 || obj >= nObjects) {  // cannot happen
        scal[kUpErrInternal] = 1;
        return;
    }
    if (t == 0 || tobj[t - 1] != obj) objTreelet[obj] = t;
    if (t == nTreelets - 1) objTreelet[nObjects] = nTreelets;
    const Box6 b = tbox[t];
    const int size = tsize[t];
    bool fine = size >= 1 && (size & 1);
    for (int k = 0; k < 3; ++k) fine = fine && __builtin_isfinite(b.mn[k]) && __builtin_isfinite(b.mx[k]);
    if (!fine) atomicMin(&scal[kUpErrTable], obj);
    atomicAdd(&objNodes[obj], (unsigned)size + 1u);  // from -1: sum(tsize) + treelets - 1, the tree's node count
}

__global__ __launch_bounds__(kB) void k_upper_seed(int nObjects, const int *__restrict__ objTreelet,
                                                   const unsigned *__restrict__ nodeFirst, int *__restrict__ tbase,
                                                   int *__restrict__ tdepth, UpperRange *__restrict__ queue, int *scal) {
    const int k = blockIdx.x * kB + threadIdx.x;
    if (k >= nObjects) return;
    const int first = objTreelet[k], count = objTreelet[k + 1] - first;
    if (first < 0 || count < 1 || count > kUpperMaxTreelets) {
        atomicMin(&scal[kUpErrCount], k);
        return;
    }
    if (count == 1) {  // the treelet's root is the tree's
        tbase[first] = (int)nodeFirst[k];
        tdepth[first] = 0;
        return;
    }
    queue[atomicAdd(&scal[kUpQueue], 1)] = UpperRange{first, first + count, 0, 0};  // at most one per object
}

__global__ __launch_bounds__(kUpperWave) void k_upper_pass(const UpperRange *__restrict__ queueIn, const int *nIn,
                                                           UpperRange *__restrict__ queueOut, int *nOut, int queueCap,
                                                           const Box6 *__restrict__ tbox, const int *__restrict__ tsize,
                                                           const int *__restrict__ tobj, const unsigned *__restrict__ nodeFirst,
                                                           int *perm, int *lfPos, int *rtPos, int *__restrict__ tbase,
                                                           int *__restrict__ tdepth, UpperSplit *__restrict__ splits,
                                                           int *scal) {
    __shared__ int bcount[kUpperBuckets], bnodes[kUpperBuckets];
    __shared__ unsigned bkeys[kUpperBuckets * 6];
    __shared__ UpperRange stack[kUpperWave];
    if ((int)blockIdx.x >= *nIn) return;
    const int lane = threadIdx.x;
    UpperRange r = queueIn[blockIdx.x];
    const int obj = tobj[perm[r.s]];
    const int treeRoot = (int)nodeFirst[obj];
    const bool whole = r.e - r.s <= kUpperWave;
    int sp = 0;
    // (whole: every trip makes one of the range's at most 63 upper nodes; else one trip)
    for (int trip = 0; trip < kUpperWave; ++trip) {
        const int n = r.e - r.s;
        // bounds and centroid bounds of the range (values)
        float v[12];
        for (int k = 0; k < 3; ++k) {
            v[k] = v[6 + k] = 3.402823466e+38f;
            v[3 + k] = v[9 + k] = -3.402823466e+38f;
        }
        for (int j = lane; j < n; j += 64) {
            const Box6 b = tbox[perm[r.s + j]];
            for (int k = 0; k < 3; ++k) {
                v[k] = fminf(v[k], b.mn[k]);
                v[3 + k] = fmaxf(v[3 + k], b.mx[k]);
                const float c = (b.mn[k] + b.mx[k]) * 0.5f;
                v[6 + k] = fminf(v[6 + k], c);
                v[9 + k] = fmaxf(v[9 + k], c);
            }
        }
        for (int q = 0; q < 12; ++q) {
            const bool isMin = (q % 6) < 3;
            for (int off = 32; off >= 1; off >>= 1) {
                const float o = __shfl_xor(v[q], off);
                v[q] = isMin ? fminf(v[q], o) : fmaxf(v[q], o);
            }
            v[q] = __shfl(v[q], 0);  // one value for the whole wavefront (a zero's sign may differ per lane)
        }
        Box6 bounds, cb;
        for (int k = 0; k < 3; ++k) {
            bounds.mn[k] = v[k], bounds.mx[k] = v[3 + k];
            cb.mn[k] = v[6 + k], cb.mx[k] = v[9 + k];
        }
        const int dim = box_maxdim(cb);
        const float cmn = cb.mn[dim], cmx = cb.mx[dim];
        bool failed = cmx == cmn;  // "treelet centroids coincide"
        int mid = 0, leftNodes = 0;
        if (!failed) {
            if (lane < kUpperBuckets) bcount[lane] = bnodes[lane] = 0;
            // an empty bucket is the host's Box(): max float, lowest float
            for (int q = lane; q < kUpperBuckets * 6; q += 64) bkeys[q] = f2key((q % 6) < 3 ? 3.402823466e+38f : -3.402823466e+38f);
            __syncthreads();
            for (int j = lane; j < n; j += 64) {
                const int t = perm[r.s + j];
                const Box6 b = tbox[t];
                const int bk = upper_bucket(b, dim, cmn, cmx);
                atomicAdd(&bcount[bk], 1);
                atomicAdd(&bnodes[bk], tsize[t]);
                for (int k = 0; k < 3; ++k) {
                    atomicMin(&bkeys[bk * 6 + k], f2key(b.mn[k]));
                    atomicMax(&bkeys[bk * 6 + 3 + k], f2key(b.mx[k]));
                }
            }
            __syncthreads();
            // lane i: cost[i], folded from the buckets as the host folds it
            float cost = 0;
            if (lane < kUpperBuckets - 1) {
                Box6 b0, b1;
                box_init(b0);
                box_init(b1);
                int c0 = 0, c1 = 0;
#pragma unroll 1
                for (int j = 0; j < kUpperBuckets; ++j) {
                    Box6 bj;
                    for (int k = 0; k < 3; ++k) {
                        bj.mn[k] = key2f(bkeys[j * 6 + k]);
                        bj.mx[k] = key2f(bkeys[j * 6 + 3 + k]);
                    }
                    if (j <= lane) {
                        box_add(b0, bj);
                        c0 += bcount[j];
                    } else {
                        box_add(b1, bj);
                        c1 += bcount[j];
                    }
                }
                cost = .125f + (c0 * box_area(b0) + c1 * box_area(b1)) / box_area(bounds);
            }
            float minCost = __shfl(cost, 0);
            int best = 0;
            for (int i = 1; i < kUpperBuckets - 1; ++i) {
                const float ci = __shfl(cost, i);
                if (ci < minCost) {  // the first minimum; a NaN cost[0] keeps best = 0
                    minCost = ci;
                    best = i;
                }
            }
            for (int j = 0; j <= best; ++j) {
                mid += bcount[j];
                leftNodes += bnodes[j];
            }
            __syncthreads();  // everyone has read the buckets before the next range clears them
            if (mid <= 0 || mid >= n) {
                failed = true;  // "degenerate upper-level SAH split"
            } else {
                // std::partition(bucket <= best) by ranks: offenders of the left part from the left ...
                int nl = 0;
                for (int base = 0; base < mid; base += 64) {
                    const int j = base + lane;
                    bool f = false;
                    if (j < mid) f = upper_bucket(tbox[perm[r.s + j]], dim, cmn, cmx) > best;
                    const unsigned long long mask = __ballot(f);
                    if (f) lfPos[r.s + nl + __popcll(mask & ((1ull << lane) - 1ull))] = r.s + j;
                    nl += __popcll(mask);
                }
                // ... trade places with the offenders of the right part from the right
                int nr = 0;
                for (int top = n; top > mid; top -= 64) {
                    const int j = top - 1 - lane;
                    bool f = false;
                    if (j >= mid) f = upper_bucket(tbox[perm[r.s + j]], dim, cmn, cmx) <= best;
                    const unsigned long long mask = __ballot(f);
                    if (f) rtPos[r.s + nr + __popcll(mask & ((1ull << lane) - 1ull))] = r.s + j;
                    nr += __popcll(mask);
                }
                if (nl != nr) {  // cannot happen: both equal the number of swaps
                    if (lane == 0) scal[kUpErrInternal] = 2;
                    nl = nl < nr ? nl : nr;
                }
                __syncthreads();
                for (int k = lane; k < nl; k += 64) {
                    const int a = lfPos[r.s + k], b = rtPos[r.s + k];
                    const int va = perm[a], vb = perm[b];
                    perm[a] = vb;
                    perm[b] = va;
                }
                __syncthreads();
            }
        }
        if (failed) {
            if (lane == 0) atomicMin(&scal[kUpErrTable], obj);
        } else {
            // the left subtree: mid treelets' nodes and mid - 1 upper nodes
            const UpperRange left{r.s, r.s + mid, r.rel + 1, r.depth + 1};
            const UpperRange right{r.s + mid, r.e, r.rel + 1 + leftNodes + (mid - 1), r.depth + 1};
            if (lane == 0) {
                splits[r.s + mid] = UpperSplit{r.s, r.e, r.rel, right.rel, dim};
                if (mid == 1) {
                    const int t = perm[left.s];
                    tbase[t] = treeRoot + left.rel;
                    tdepth[t] = left.depth;
                }
                if (n - mid == 1) {
                    const int t = perm[right.s];
                    tbase[t] = treeRoot + right.rel;
                    tdepth[t] = right.depth;
                }
            }
            if (whole) {
                // left first, as the host recurses; the pending second children of one root-to-leaf path: at most 63
                if (n - mid > 1) {
                    if (sp < kUpperWave) {
                        if (lane == 0) stack[sp] = right;
                        ++sp;
                    } else if (lane == 0) {
                        scal[kUpErrInternal] = 4;  // cannot happen
                    }
                }
                if (mid > 1) {
                    r = left;
                    continue;
                }
            } else if (lane == 0) {
                for (int c = 0; c < 2; ++c) {
                    const UpperRange child = c ? right : left;
                    if (child.e - child.s < 2) continue;
                    const int at = atomicAdd(nOut, 1);
                    if (at < queueCap) queueOut[at] = child;
                    else scal[kUpErrInternal] = 3;  // cannot happen: the ranges are disjoint, two treelets or more each
                }
            }
        }
        if (!whole || sp == 0) break;
        __syncthreads();  // lane 0's pushes
        r = stack[--sp];
        __syncthreads();  // every lane has read the entry before lane 0 writes it again
    }
}

// The upper nodes themselves: one wavefront per position of the treelet order, for the node that was split there.
// The box is the in-order fold over the node's range in the final order (see above): lanes fold contiguous chunks, the
// cross-lane steps keep (lower lane = earlier treelets) on the left, as k_big_leaf_bounds does.
__global__ __launch_bounds__(kB) void k_upper_nodes(int nTreelets, const UpperSplit *__restrict__ splits,
                                                    const int *__restrict__ perm, const Box6 *__restrict__ tbox,
                                                    const int *__restrict__ tobj, const int *__restrict__ nodeFirst,
                                                    nnbvh_linear_node *__restrict__ nodes) {
    const int p = blockIdx.x * (kB / 64) + (threadIdx.x >> 6);  // wave-uniform
    if (p >= nTreelets) return;
    const UpperSplit sp = splits[p];
    if (sp.e == 0) return;  // the first treelet of an object: nothing was split here
    const int lane = threadIdx.x & 63;
    const int n = sp.e - sp.s;
    const int chunk = (n + 63) / 64;
    const int lo = lane * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
    Box6 b;
    box_init(b);
    for (int j = lo; j < hi; ++j) box_add(b, tbox[perm[sp.s + j]]);
    for (int off = 1; off < 64; off <<= 1) {
        Box6 o;
        for (int k = 0; k < 3; ++k) {
            o.mn[k] = __shfl_down(b.mn[k], off);
            o.mx[k] = __shfl_down(b.mx[k], off);
        }
        if (lane + off < 64) box_add(b, o);  // b = earlier treelets (kept on ties), o = later ones
    }
    if (lane == 0) {
        nnbvh_linear_node out;
        for (int k = 0; k < 3; ++k) {
            out.pmin[k] = b.mn[k];
            out.pmax[k] = b.mx[k];
        }
        out.offset = sp.second;  // counted from the tree's root, like every second child
        out.nprims = 0;
        out.axis = (uint8_t)sp.axis;
        out.pad = 0;
        nodes[nodeFirst[tobj[perm[sp.s]]] + sp.rel] = out;
    }
}

// ---------------------------------------------------------------------------------------------------------
struct DevMem {  // frees everything it handed out (with a pool: hands it back for the next build)
    std::vector<void *> ptrs;
    std::string *error;
    bool ok = true;
    ScratchPool *pool = nullptr;
    template <typename T>
    T *get(size_t count) {
        void *p = nullptr;
        if (!ok) return nullptr;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
        if (pool) p = pool->take(bytes);
        else if (hipMalloc(&p, bytes) != hipSuccess) p = nullptr;
        if (!p) {
            ok = false;
            *error = "gpu build: hipMalloc failed";
            return nullptr;
        }
        ptrs.push_back(p);
        return (T *)p;
    }
    void release(void *p) {  // ownership goes to the caller
        for (void *&q : ptrs)
            if (q == p) q = nullptr;
    }
    ~DevMem() {
        for (void *p : ptrs) {
            if (!p) continue;
            if (pool) pool->give(p);
            else (void)hipFree(p);
        }
    }
};

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int grid_for(long n, int cap = 4096) {
    long b = (n + kB - 1) / kB;
    return (int)std::max<long>(1, std::min<long>(b, cap));
}
int grid_all(long n) { return (int)std::max<long>(1, (n + kB - 1) / kB); }

}  // namespace

#define GB_CHECK(expr, what)                                         \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) {                                      \
            *error = std::string("gpu build: ") + what + ": " + hipGetErrorString(e_); \
            return false;                                            \
        }                                                            \
    } while (0)

void *ScratchPool::take(size_t bytes) {
    Block *best = nullptr;
    for (Block &b : blocks)
        if (!b.used && b.bytes >= bytes && (!best || b.bytes < best->bytes)) best = &b;
    if (best) {
        best->used = true;
        return best->p;
    }
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    blocks.push_back(Block{p, bytes, true});
    return p;
}

void ScratchPool::give(void *p) {
    for (Block &b : blocks)
        if (b.p == p) b.used = false;
}

void ScratchPool::clear() {
    for (Block &b : blocks) (void)hipFree(b.p);
    blocks.clear();
}

namespace {

// upload of a wrapper's host arrays (the device-resident cores below take it from there)
struct Uploaded {
    nnbvh_prim *prims = nullptr;
    float *verts = nullptr, *bounds = nullptr;
};
bool upload_build_input(DevMem &mem, const nnbvh_prim *prims, int n, const float *verts, int n_verts,
                        const float *prim_bounds, Uploaded *up, std::string *error) {
    up->prims = mem.get<nnbvh_prim>(n);
    up->verts = mem.get<float>(3 * (size_t)n_verts);
    up->bounds = prim_bounds ? mem.get<float>(6 * (size_t)n) : nullptr;
    if (!mem.ok) return false;
    GB_CHECK(hipMemcpyAsync(up->prims, prims, (size_t)n * sizeof(nnbvh_prim), hipMemcpyHostToDevice, nullptr), "copy prims");
    GB_CHECK(hipMemcpyAsync(up->verts, verts, 3 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, nullptr), "copy verts");
    if (up->bounds)
        GB_CHECK(hipMemcpyAsync(up->bounds, prim_bounds, 6 * (size_t)n * sizeof(float), hipMemcpyHostToDevice, nullptr), "copy bounds");
    GB_CHECK(hipStreamSynchronize(nullptr), "sync after upload");
    return true;
}

// what the wrappers do with a core's device-resident result: hand it over, or download and free it
bool finish_build(DevMem &mem, const Uploaded &up, int n, GpuBuildResult *out, std::string *error) {
    if (out->keep_on_device) {
        out->d_verts = up.verts;
        mem.release(up.verts);
        return true;
    }
    out->nodes.resize((size_t)out->total_nodes);
    out->ordered.resize((size_t)n);
    hipError_t e = hipMemcpy(out->nodes.data(), out->d_nodes, out->nodes.size() * sizeof(nnbvh_linear_node), hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpy(out->ordered.data(), out->d_ordered, out->ordered.size() * sizeof(nnbvh_prim), hipMemcpyDeviceToHost);
    (void)hipFree(out->d_nodes);
    (void)hipFree(out->d_ordered);
    out->d_nodes = out->d_ordered = nullptr;
    GB_CHECK(e, "read nodes / ordered prims");
    return true;
}

struct RestoreDevice {
    int d;
    ~RestoreDevice() { (void)hipSetDevice(d); }
};

// gpu_hlbvh / gpu_sah: upload, the device-resident core, hand over or download
typedef bool (*DeviceCore)(const DeviceBuildInput &, GpuBuildResult *, std::string *);
bool build_uploaded(DeviceCore core, const nnbvh_prim *prims, int n, const float *verts, int n_verts,
                    const float *prim_bounds, int max_prims_in_node, int device, GpuBuildResult *out, std::string *error) {
    int prev = 0;
    GB_CHECK(hipGetDevice(&prev), "hipGetDevice");
    GB_CHECK(hipSetDevice(device), "hipSetDevice");
    RestoreDevice restore{prev};
    DevMem mem;
    mem.error = error;
    auto t0 = std::chrono::steady_clock::now();
    Uploaded up;
    if (!upload_build_input(mem, prims, n, verts, n_verts, prim_bounds, &up, error)) return false;
    out->ms[0] = ms_since(t0);
    DeviceBuildInput in;
    in.d_prims = up.prims;
    in.n_prims = n;
    in.d_verts = up.verts;
    in.n_verts = n_verts;
    in.d_prim_bounds = up.bounds;
    in.max_prims_in_node = max_prims_in_node;
    if (!core(in, out, error)) return false;
    t0 = std::chrono::steady_clock::now();
    const bool ok = finish_build(mem, up, n, out, error);
    out->ms[4] = ms_since(t0);
    return ok;
}

// gpu_hlbvh_device / gpu_sah_device: one tree = a forest of one object.  codes: the member that n_unique_codes reports
typedef bool (*ForestCore)(const DeviceBuildInput &, const int *, int, ForestBuildResult *, std::string *);
bool build_one_object(ForestCore forest, int ForestBuildResult::*codes, const DeviceBuildInput &in, GpuBuildResult *out,
                      std::string *error) {
    const int object_first[2] = {0, in.n_prims};
    ForestBuildResult f;
    if (!forest(in, object_first, 1, &f, error)) return false;
    out->d_nodes = f.d_nodes;
    out->d_ordered = f.d_ordered;
    out->total_nodes = f.total_nodes;
    out->depth = f.depth[0];
    for (int k = 1; k <= 3; ++k) out->ms[k] = f.ms[k];
    out->n_treelets = f.n_subtrees;
    out->n_unique_codes = f.*codes;
    out->n_upper = f.n_upper;
    out->n_upper_passes = f.n_upper_passes;
    return true;
}

// What a loop of one-object builds would have reported: the failure of the lowest-numbered object, and within one
// object the first in the order of the phases.  The forest builders call it in that order, so a tie keeps the earlier.
struct Refusal {
    int object = kNoObject;
    std::string text;
    void operator()(int o, const std::string &t) {
        if (o < object) {
            object = o;
            text = t;
        }
    }
};

bool check_object_first(const int *objectFirst, int nObjects, int nAll, std::string *error) {
    if (!objectFirst || nObjects < 1 || objectFirst[0] != 0 || objectFirst[nObjects] != nAll) {
        *error = "gpu build: malformed object_first (it starts at 0 and ends at n_prims)";
        return false;
    }
    for (int k = 0; k < nObjects; ++k)
        if (objectFirst[k + 1] <= objectFirst[k]) {
            *error = "gpu build: malformed object_first (an object is empty or the entries decrease)";
            return false;
        }
    return true;
}

// The HLBVH pipeline (the ten steps at the top of this file) over the sort key (object << 30) | code.
// ONE stable radix sort over the bits in use orders every object's primitives by their 30 code bits without moving one
// across an object boundary; a run of identical keys, a treelet (equal bits >= 18) and a radix-tree range all end
// where the object does, because the object number is part of the key; the objects themselves hang off radix nodes that
// split on bits >= 30, which are no more part of a tree than the nodes that split on bits 18 .. 29.  So every step is
// one launch for the whole forest, and the upper SAH runs in passes over one table of every object's treelets (8b).
// A malformed object's primitives run through the pipeline like any others (no kernel indexes with a coordinate); only
// its messages count, and only if no lower-numbered object has one.
// Key = unsigned serves one object alone: its keys are its codes, sorted over bits 0 .. 29 at half the 64-bit key's
// traffic; k_prim_bounds' centroid bounds of the whole input are the object's, so k_cbounds_init and k_object_cbounds
// are not launched.
template <typename Key>
bool hlbvh_forest(const DeviceBuildInput &in, const int *objectFirst, int nObjects, ForestBuildResult *out,
                  std::string *error) {
    const int n = in.n_prims, n_verts = in.n_verts;
    const nnbvh_prim *dPrims = in.d_prims;
    const float *dVerts = in.d_verts, *dCaller = in.d_prim_bounds;
    const int maxPrims = std::min(255, in.max_prims_in_node);  // aggregates.cpp:142
    hipStream_t stream = (hipStream_t)in.stream;
    DevMem mem, outMem;  // outMem: the result arrays this call allocates itself
    mem.error = outMem.error = error;
    mem.pool = in.pool;
    Refusal refuse;
    const bool many = nObjects > 1;
    int objectBits = 0;
    while (objectBits < 31 && ((long)nObjects - 1) >> objectBits) ++objectBits;
    const unsigned endBit = 30u + (unsigned)objectBits;

    auto t0 = std::chrono::steady_clock::now();
    Box6 *dPb = mem.get<Box6>(n);
    Key *dKeys = mem.get<Key>(n), *dKeysS = mem.get<Key>(n), *dUkey = mem.get<Key>(n);
    int *dIdx = mem.get<int>(n), *dIdxS = mem.get<int>(n);
    int *dHead = mem.get<int>(n), *dExcl = mem.get<int>(n);
    int *dPstart = mem.get<int>((size_t)n + 1);
    // one block, one upload: [0..5] k_prim_bounds' centroid keys of the whole input, 7 m, [8..] errObj | object_first |
    // the objects' depths, from the next 128-byte line on: k_emit's atomics go there while every leaf reads object_first
    constexpr int kScalars = 8 + kErrWords;
    const size_t depthAt = (kScalars + (size_t)nObjects + 1 + 31) / 32 * 32;
    int *dScalars = mem.get<int>(depthAt + (size_t)nObjects);
    int *dObjectFirst = dScalars + kScalars, *dDepthObj = dScalars + depthAt;
    // the objects' centroid keys and every primitive's object: one object's are dScalars[0..5] and 0
    unsigned *dCbObj = many ? mem.get<unsigned>(6 * (size_t)nObjects) : (unsigned *)dScalars;
    int *dObjOf = many ? mem.get<int>(n) : nullptr;
    if (!mem.ok) return false;
    std::vector<int> init(depthAt + (size_t)nObjects, 0);
    init[0] = init[1] = init[2] = -1;  // min keys all-ones, max keys 0
    for (int k = 1; k < kErrWords; ++k) init[8 + k] = kNoObject;
    std::copy(objectFirst, objectFirst + nObjects + 1, init.begin() + kScalars);
    GB_CHECK(hipMemcpyAsync(dScalars, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice, stream), "init scalars");
    int *dM = dScalars + 7, *dErrObj = dScalars + 8;
    hipLaunchKernelGGL(k_prim_bounds, dim3(grid_for(n, 1024)), dim3(kB), 0, stream, dPrims, dVerts, n_verts, dCaller, n, dPb,
                       (unsigned *)dScalars, (const int *)dObjectFirst, nObjects, dErrObj);
    if (many) {
        hipLaunchKernelGGL(k_cbounds_init, dim3(grid_all(6L * nObjects)), dim3(kB), 0, stream, nObjects, dCbObj);
        hipLaunchKernelGGL(k_object_cbounds, dim3(grid_all(n)), dim3(kB), 0, stream, dPb, dObjectFirst, nObjects, n, dObjOf,
                           dCbObj);
    }
    hipLaunchKernelGGL(k_morton<Key>, dim3(grid_for(n)), dim3(kB), 0, stream, dPb, dCbObj, dObjOf, n, dKeys, dIdx);
    size_t tmpBytes = 0, scanBytes = 0;
    GB_CHECK(rocprim::radix_sort_pairs(nullptr, tmpBytes, dKeys, dKeysS, dIdx, dIdxS, (size_t)n, 0u, endBit, stream),
             "radix sort (size query)");
    GB_CHECK(rocprim::exclusive_scan(nullptr, scanBytes, dHead, dExcl, 0, (size_t)n + 1, rocprim::plus<int>(), stream),
             "scan (size query)");
    void *dTmp = mem.get<char>(std::max(tmpBytes, scanBytes));
    if (!mem.ok) return false;
    GB_CHECK(rocprim::radix_sort_pairs(dTmp, tmpBytes, dKeys, dKeysS, dIdx, dIdxS, (size_t)n, 0u, endBit, stream), "radix sort");
    hipLaunchKernelGGL(k_heads<Key>, dim3(grid_for(n)), dim3(kB), 0, stream, dKeysS, n, dHead);
    GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dHead, dExcl, 0, (size_t)n, rocprim::plus<int>(), stream), "scan");
    hipLaunchKernelGGL(k_compact<Key>, dim3(grid_for(n)), dim3(kB), 0, stream, dKeysS, dHead, dExcl, n, dPstart, dUkey, dM);
    int scal[kScalars];
    GB_CHECK(hipMemcpyAsync(scal, dScalars, sizeof scal, hipMemcpyDeviceToHost, stream), "read scalars");
    GB_CHECK(hipStreamSynchronize(stream), "sync after sort");
    const int *errWords = scal + 8;
    refuse(errWords[kErrVertex], "nnbvh_build_create: vertex index out of range");
    refuse(errWords[kErrNeedBounds], "nnbvh_build_create: instance / host primitives need prim_bounds");
    refuse(errWords[kErrNonFinite], "nnbvh_build_create: non-finite vertex or primitive bounds");
    refuse(errWords[kErrKind], "nnbvh_build_create: unknown primitive kind");
    if (refuse.object == 0) {  // no lower-numbered object is left to change the message
        *error = refuse.text;
        return false;
    }
    const int m = scal[7];
    if (m < nObjects || m > n) {
        *error = "gpu build: internal error (distinct code count)";
        return false;
    }
    const int nv = 2 * m - 1;
    const int tCap = (int)std::min<long>(m, 4096L * nObjects);  // an object has at most 4096 treelets, and no more than codes

    int *dFirst = mem.get<int>(m), *dLast = mem.get<int>(m), *dLeft = mem.get<int>(m), *dRight = mem.get<int>(m);
    unsigned char *dBit = mem.get<unsigned char>(m), *dKind = mem.get<unsigned char>(nv);
    int *dParent = mem.get<int>(nv);
    int *dLeafHead = mem.get<int>((size_t)m + 1), *dTreeHead = mem.get<int>((size_t)m + 1);
    int *dLeafOrd = mem.get<int>((size_t)m + 1), *dTreeOrd = mem.get<int>((size_t)m + 1);
    Box6 *dNodeBox = mem.get<Box6>(nv);
    Box6 *dTbox = mem.get<Box6>(tCap);
    int *dTsize = mem.get<int>(tCap), *dTobj = mem.get<int>(tCap);
    if (!mem.ok) return false;
    GB_CHECK(hipMemsetAsync(dParent, 0xff, (size_t)nv * sizeof(int), stream), "memset parents");  // -1: the root
    GB_CHECK(hipMemsetAsync(dLeafHead, 0, ((size_t)m + 1) * sizeof(int), stream), "memset");
    GB_CHECK(hipMemsetAsync(dTreeHead, 0, ((size_t)m + 1) * sizeof(int), stream), "memset");
    if (m > 1)
        hipLaunchKernelGGL(k_karras<Key>, dim3(grid_all(m - 1)), dim3(kB), 0, stream, dUkey, m, dFirst, dLast, dLeft, dRight,
                           dBit, dParent);
    hipLaunchKernelGGL(k_classify<Key>, dim3(grid_all(nv)), dim3(kB), 0, stream, m, maxPrims, dPstart, dFirst, dLast, dBit,
                       dParent, dUkey, dKind, dLeafHead, dTreeHead, dErrObj);
    GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dLeafHead, dLeafOrd, 0, (size_t)m + 1, rocprim::plus<int>(), stream),
             "scan leaves");
    GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dTreeHead, dTreeOrd, 0, (size_t)m + 1, rocprim::plus<int>(), stream),
             "scan treelets");
    hipLaunchKernelGGL(k_leaf_bounds, dim3(grid_all(nv)), dim3(kB), 0, stream, m, dKind, dPstart, dFirst, dLast, dIdxS, dPb,
                       dNodeBox);
    hipLaunchKernelGGL(k_big_leaf_bounds, dim3((nv + kB / 64 - 1) / (kB / 64)), dim3(kB), 0, stream, m, dKind, dPstart,
                       dFirst, dLast, dIdxS, dPb, dNodeBox);
    if (m > 1)
        for (int level = 0; level < kTreeletBit; ++level)
            hipLaunchKernelGGL(k_interior_bounds, dim3(grid_all(m - 1)), dim3(kB), 0, stream, m, level, dKind, dBit, dLeft,
                               dRight, dNodeBox);
    hipLaunchKernelGGL(k_treelets<Key>, dim3(grid_all(nv)), dim3(kB), 0, stream, m, dKind, dFirst, dLast, dLeafOrd,
                       dTreeOrd, dNodeBox, dUkey, tCap, dTbox, dTsize, dTobj);
    int nTreelets = 0, leafSizeObject = kNoObject;
    GB_CHECK(hipMemcpyAsync(&nTreelets, dTreeOrd + m, sizeof(int), hipMemcpyDeviceToHost, stream), "read treelet count");
    GB_CHECK(hipMemcpyAsync(&leafSizeObject, dErrObj + kErrLeafSize, sizeof(int), hipMemcpyDeviceToHost, stream), "read error word");
    GB_CHECK(hipStreamSynchronize(stream), "sync after classify");
    refuse(leafSizeObject, "nnbvh_build_create: more than 65535 primitives share one Morton code (leaf too large)");
    if (nTreelets < nObjects || nTreelets > tCap) {
        *error = "gpu build: internal error (treelet count)";
        return false;
    }
    out->ms[1] = ms_since(t0);

    // ---- the upper SAH of every object over its own treelets, on the device (8b): the treelet table stays there -------
    t0 = std::chrono::steady_clock::now();
    const int nUpper = nTreelets - nObjects;  // a tree of c treelets has c - 1 upper nodes
    const int queueCap = nTreelets / 2 + 1;   // the ranges of a pass are disjoint and hold two treelets or more
    constexpr int kUpScalars = kUpQueue + kUpperMaxPasses + 2;
    int *dPerm = mem.get<int>(nTreelets), *dLfPos = mem.get<int>(nTreelets), *dRtPos = mem.get<int>(nTreelets);
    int *dTbase = mem.get<int>(nTreelets), *dTdepth = mem.get<int>(nTreelets);
    int *dObjTreelet = mem.get<int>((size_t)nObjects + 1);
    unsigned *dObjNodes = mem.get<unsigned>((size_t)nObjects + 1), *dNodeFirst = mem.get<unsigned>((size_t)nObjects + 1);
    UpperSplit *dSplits = mem.get<UpperSplit>(nTreelets);
    UpperRange *dQueue[2] = {mem.get<UpperRange>(queueCap), mem.get<UpperRange>(queueCap)};
    int *dUp = mem.get<int>(kUpScalars);
    if (!mem.ok) return false;
    static const int kNobody[2] = {kNoObject, kNoObject};
    GB_CHECK(hipMemsetAsync(dObjTreelet, 0xff, ((size_t)nObjects + 1) * sizeof(int), stream), "memset");  // -1: no treelet
    GB_CHECK(hipMemsetAsync(dObjNodes, 0xff, ((size_t)nObjects + 1) * sizeof(unsigned), stream), "memset");  // -1: see k_upper_treelets
    GB_CHECK(hipMemsetAsync(dSplits, 0, (size_t)nTreelets * sizeof(UpperSplit), stream), "memset");
    GB_CHECK(hipMemsetAsync(dUp, 0, kUpScalars * sizeof(int), stream), "memset");
    GB_CHECK(hipMemcpyAsync(dUp, kNobody, sizeof kNobody, hipMemcpyHostToDevice, stream), "init error words");
    hipLaunchKernelGGL(k_upper_treelets, dim3(grid_all(nTreelets)), dim3(kB), 0, stream, nTreelets, nObjects, dTbox, dTsize,
                       dTobj, dPerm, dObjTreelet, dObjNodes, dUp);
    // (2 n_prims bounds the forest's nodes: an unsigned sum does not wrap)
    GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dObjNodes, dNodeFirst, 0u, (size_t)nObjects + 1, rocprim::plus<unsigned>(), stream),
             "scan node counts");
    hipLaunchKernelGGL(k_upper_seed, dim3(grid_all(nObjects)), dim3(kB), 0, stream, nObjects, dObjTreelet, dNodeFirst, dTbase,
                       dTdepth, dQueue[0], dUp);
    // pass 0 takes up one range per object of two treelets or more (the kernel reads how many: no read-back before
    // it); a later pass what the one before queued.  Every range a pass queues is smaller than the one it came from.
    int nPasses = 0;
    for (int queued = nUpper ? std::min(nObjects, nTreelets / 2) : 0; queued > 0; ++nPasses) {
        if (nPasses > kUpperMaxPasses) {
            *error = "gpu build: internal error (upper build does not end)";
            return false;
        }
        int *dCount = dUp + kUpQueue + nPasses;
        hipLaunchKernelGGL(k_upper_pass, dim3(queued), dim3(kUpperWave), 0, stream, dQueue[nPasses & 1], dCount,
                           dQueue[(nPasses + 1) & 1], dCount + 1, queueCap, dTbox, dTsize, dTobj, dNodeFirst, dPerm, dLfPos,
                           dRtPos, dTbase, dTdepth, dSplits, dUp);
        GB_CHECK(hipMemcpyAsync(&queued, dCount + 1, sizeof(int), hipMemcpyDeviceToHost, stream), "read queue length");
        GB_CHECK(hipStreamSynchronize(stream), "sync after upper pass");
        queued = std::min(queued, queueCap);
    }
    int upErr[3];
    std::vector<unsigned> nodeFirst((size_t)nObjects + 1);
    GB_CHECK(hipMemcpyAsync(upErr, dUp, sizeof upErr, hipMemcpyDeviceToHost, stream), "read upper error words");
    GB_CHECK(hipMemcpyAsync(nodeFirst.data(), dNodeFirst, nodeFirst.size() * sizeof(unsigned), hipMemcpyDeviceToHost, stream), "read node_first");
    GB_CHECK(hipGetLastError(), "kernel launch");
    GB_CHECK(hipStreamSynchronize(stream), "sync after upper build");
    if (upErr[kUpErrInternal]) {
        *error = "gpu build: internal error (upper build " + std::to_string(upErr[kUpErrInternal]) + ")";
        return false;
    }
    // What the host's loop over the objects would have stopped at: the lowest-numbered object of all.  The words of an
    // object the device refused are the host builder's own, from that object's treelet table alone.
    if (upErr[kUpErrCount] < refuse.object && upErr[kUpErrCount] <= upErr[kUpErrTable]) {
        *error = "gpu build: internal error (treelet count)";
        return false;
    }
    if (upErr[kUpErrTable] < refuse.object) {
        const int k = upErr[kUpErrTable];
        int range[2];
        GB_CHECK(hipMemcpyAsync(range, dObjTreelet + k, sizeof range, hipMemcpyDeviceToHost, stream), "read treelet range");
        GB_CHECK(hipStreamSynchronize(stream), "sync after treelet range");
        const int count = range[1] - range[0];
        if (range[0] < 0 || count < 1 || range[1] > nTreelets) {
            *error = "gpu build: internal error (treelet count)";
            return false;
        }
        std::vector<float> tbox(6 * (size_t)count);
        std::vector<int> tsize((size_t)count);
        GB_CHECK(hipMemcpyAsync(tbox.data(), dTbox + range[0], tbox.size() * sizeof(float), hipMemcpyDeviceToHost, stream), "read treelet bounds");
        GB_CHECK(hipMemcpyAsync(tsize.data(), dTsize + range[0], tsize.size() * sizeof(int), hipMemcpyDeviceToHost, stream), "read treelet sizes");
        GB_CHECK(hipStreamSynchronize(stream), "sync after treelet table");
        std::string text;
        if (!hlbvh_upper_refusal(tbox.data(), tsize.data(), count, &text)) {
            *error = "gpu build: internal error (the host builder accepts a treelet table the device refused)";
            return false;
        }
        refuse(k, text);
    }
    for (int k = 0; k < nObjects && k < refuse.object; ++k)
        if (nodeFirst[(size_t)k + 1] >= 0x7fffffffu) {
            *error = "gpu build: too many nodes";
            return false;
        }
    if (refuse.object != kNoObject) {
        *error = refuse.text;
        return false;
    }
    out->node_first.assign(nodeFirst.begin(), nodeFirst.end());
    const int totalNodes = out->node_first[(size_t)nObjects];
    out->ms[2] = ms_since(t0);

    t0 = std::chrono::steady_clock::now();
    nnbvh_linear_node *dNodes = in.d_nodes_out ? in.d_nodes_out : outMem.get<nnbvh_linear_node>((size_t)totalNodes);
    nnbvh_prim *dOrdered = in.d_ordered_out ? in.d_ordered_out : outMem.get<nnbvh_prim>(n);
    if (!mem.ok || !outMem.ok) return false;
    if (nUpper)
        hipLaunchKernelGGL(k_upper_nodes, dim3((nTreelets + kB / 64 - 1) / (kB / 64)), dim3(kB), 0, stream, nTreelets, dSplits,
                           dPerm, dTbox, dTobj, (const int *)dNodeFirst, dNodes);
    hipLaunchKernelGGL(k_emit, dim3(grid_all(nv)), dim3(kB), 0, stream, m, dKind, dBit, dPstart, dFirst, dLast, dLeft,
                       dParent, dLeafOrd, dTreeOrd, dTbase, dTdepth, dTobj, (const int *)dNodeFirst, dObjectFirst, dNodeBox,
                       dNodes, dDepthObj);
    hipLaunchKernelGGL(k_gather_prims, dim3(grid_for(n)), dim3(kB), 0, stream, dPrims, dIdxS, n, dOrdered);
    out->depth.assign((size_t)nObjects, 0);
    GB_CHECK(hipMemcpyAsync(out->depth.data(), dDepthObj, (size_t)nObjects * sizeof(int), hipMemcpyDeviceToHost, stream), "read depths");
    GB_CHECK(hipGetLastError(), "kernel launch");
    GB_CHECK(hipStreamSynchronize(stream), "sync after emit");
    out->ms[3] = ms_since(t0);
    out->total_nodes = totalNodes;
    out->d_nodes = dNodes;
    out->d_ordered = dOrdered;
    outMem.release(dNodes);
    outMem.release(dOrdered);
    out->n_levels = 0;
    out->n_subtrees = nTreelets;
    out->n_upper = nUpper;
    out->n_upper_passes = nPasses;
    out->n_codes = m;
    return true;
}

}  // namespace

bool gpu_hlbvh_forest_device(const DeviceBuildInput &in, const int *objectFirst, int nObjects, ForestBuildResult *out,
                             std::string *error) {
    if (!check_object_first(objectFirst, nObjects, in.n_prims, error)) return false;
    return (nObjects == 1 ? hlbvh_forest<unsigned> : hlbvh_forest<unsigned long long>)(in, objectFirst, nObjects, out, error);
}

bool gpu_hlbvh_device(const DeviceBuildInput &in, GpuBuildResult *out, std::string *error) {
    return build_one_object(gpu_hlbvh_forest_device, &ForestBuildResult::n_codes, in, out, error);
}

bool gpu_hlbvh(const nnbvh_prim *prims, int n, const float *verts, int n_verts, const float *prim_bounds,
               int max_prims_in_node, int device, GpuBuildResult *out, std::string *error) {
    return build_uploaded(gpu_hlbvh_device, prims, n, verts, n_verts, prim_bounds, max_prims_in_node, device, out, error);
}

// =================================================================================================
// SAH build on the device: buildRecursive's SAH branch (aggregates.cpp:192-387) with the SAME tree
// and the SAME leaf-ordered primitive table as the host builder (bvh_build.cpp), hence as the
// reference.  What makes that possible:
//   * every split decision depends only on the SET of primitives of a node (bounds, centroid bounds,
//     12 bucket counts / bounds: exact min / max / integer sums, order-free) and on float
//     expressions evaluated here operation for operation (sah_choose below is compiled for host
//     and device from one source, -ffp-contract=off);
//   * the ORDER of primitives — which decides the leaf table and every later std::nth_element tie —
//     is what std::partition leaves behind, and libstdc++'s partition has a closed form: elements
//     of the left part that satisfy the predicate and elements of the right part that do not stay
//     where they are; the k-th offender of the left part (from the left) is swapped with the k-th
//     offender of the right part counted from the RIGHT end.  Ranks come from ballots / prefix sums,
//     so a node is partitioned in parallel with the sequential algorithm's exact result;
//   * stored bounds: a leaf's are the in-order fold over its primitives, an interior node's the
//     fold child 0 then child 1 (:371-373) — done after the layout, level by level from the leaves.
// Phase A: nodes with more than kSmallSegment (256) primitives, breadth-first, whole-grid kernels per
//          level (tile = 2048 primitives of one node), the 12-bucket decision on the host (a few
//          thousand nodes in total).
// Phase B: every remaining subtree is built depth-first by ONE wavefront (explicit stack in LDS,
//          nodes written in DFS order into the subtree's pool slice).
// Phase C: DFS layout of the phase-A nodes + subtree slices, copy, bounds, download.
// A FOREST (gpu_sah_forest_device; one tree is its one-object case): the objects' primitives share one permutation
// array, phase A starts with one root segment per object and works on every object's big nodes of a level at once,
// phase B is one launch over all objects' subtrees, phase C lays out tree after tree.  No segment's arithmetic looks
// outside its own range, so each tree is the one the object alone gets; only the two kinds of offset need care:
// a leaf's first primitive counts from its object's first primitive, a second child from its own tree's root.
namespace {

constexpr int kSahBuckets = 12;
constexpr int kSmallSegmentDefault = 256;
constexpr int kTile = 2048;

struct HBox {
    float mn[3], mx[3];
};
__host__ __device__ inline void hb_init(HBox &b) {
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = 3.402823466e+38f;
        b.mx[k] = -3.402823466e+38f;
    }
}
__host__ __device__ inline void hb_add(HBox &b, const HBox &o) {  // Union, first of equals kept
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = o.mn[k] < b.mn[k] ? o.mn[k] : b.mn[k];
        b.mx[k] = b.mx[k] < o.mx[k] ? o.mx[k] : b.mx[k];
    }
}
__host__ __device__ inline float hb_area(const HBox &b) {  // util/vecmath.h:1293-1296
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    return 2 * (dx * dy + dx * dz + dy * dz);
}
__host__ __device__ inline int hb_maxdim(const HBox &b) {  // util/vecmath.h:1305-1313
    const float dx = b.mx[0] - b.mn[0], dy = b.mx[1] - b.mn[1], dz = b.mx[2] - b.mn[2];
    if (dx > dy && dx > dz) return 0;
    else if (dy > dz) return 1;
    else return 2;
}
// which of the 12 buckets a primitive's centroid falls in (:312-317, Bounds3::Offset vecmath.h:1322-1331)
__host__ __device__ inline int sah_bucket(float centroid, float cmn, float cmx) {
    float o = centroid - cmn;
    if (cmx > cmn) o /= cmx - cmn;
    int b = kSahBuckets * o;
    if (b >= kSahBuckets) b = kSahBuckets - 1;  // == 12 for the largest centroid (:316); beyond only for
    if (b < 0) b = 0;                           // non-finite input, which must not index out of range
    return b;
}
// the decision of :319-371 from the node's buckets: best split, how many primitives go left,
// and whether the node is split at all
struct SahChoice {
    int best, mid, split;
};
// bucket bounds arrive as 6 order-preserving keys per bucket (min xyz, max xyz), exactly as the
// atomics left them, in LDS (wavefront subtrees) or host memory (breadth-first phase)
__host__ __device__ inline float sah_key_to_float(unsigned k) {
    const unsigned u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f;
    std::memcpy(&f, &u, 4);
    return f;
#endif
}
__host__ __device__ inline HBox sah_bucket_box(const unsigned *keys, int b) {
    HBox r;
    const unsigned *k6 = keys + 6 * b;
    r.mn[0] = sah_key_to_float(k6[0]);
    r.mn[1] = sah_key_to_float(k6[1]);
    r.mn[2] = sah_key_to_float(k6[2]);
    r.mx[0] = sah_key_to_float(k6[3]);
    r.mx[1] = sah_key_to_float(k6[4]);
    r.mx[2] = sah_key_to_float(k6[5]);
    return r;
}
__host__ __device__ inline SahChoice sah_choose(const int *count, const unsigned *keys, const HBox &bounds, int n,
                                                int maxPrims) {
    constexpr int nSplits = kSahBuckets - 1;
    float costs[nSplits];
    for (int i = 0; i < nSplits; ++i) costs[i] = 0;
    int below = 0;
    HBox bbelow;
    hb_init(bbelow);
#pragma unroll 1
    for (int i = 0; i < nSplits; ++i) {
        hb_add(bbelow, sah_bucket_box(keys, i));
        below += count[i];
        costs[i] += below * hb_area(bbelow);
    }
    int above = 0;
    HBox babove;
    hb_init(babove);
#pragma unroll 1
    for (int i = nSplits; i >= 1; --i) {
        hb_add(babove, sah_bucket_box(keys, i));
        above += count[i];
        costs[i - 1] += above * hb_area(babove);
    }
    int best = -1;
    float minCost = __builtin_inff();
#pragma unroll 1
    for (int i = 0; i < nSplits; ++i)
        if (costs[i] < minCost) {
            minCost = costs[i];
            best = i;
        }
    const float leafCost = (float)n;
    minCost = 1.f / 2.f + minCost / hb_area(bounds);
    SahChoice c;
    c.best = best;
    c.split = (n > maxPrims || minCost < leafCost) ? 1 : 0;
    c.mid = 0;
    for (int i = 0; i <= best; ++i) c.mid += count[i];
    return c;
}

__device__ __forceinline__ float centroid_of(const Box6 &b, int dim) { return .5f * b.mn[dim] + .5f * b.mx[dim]; }

// ---- phase A ---------------------------------------------------------------------------------------
struct Tile {
    int seg, start, n;  // a run of one big node's primitives
};
struct SegInfo {  // per big node of the current level
    int start, n, mid, dim, best;
    float cmn, cmx;  // centroid bounds in `dim`
};

// bounds and centroid bounds of every big node of the level (values; the sign of zeros is not needed)
__global__ __launch_bounds__(kB) void k_seg_reduce(const Tile *__restrict__ tiles, const Box6 *__restrict__ pb,
                                                   const int *__restrict__ perm, unsigned *segAcc) {
    __shared__ float red[12][kB / 64];
    const Tile t = tiles[blockIdx.x];
    float v[12];
    for (int k = 0; k < 3; ++k) {
        v[k] = v[6 + k] = 3.402823466e+38f;
        v[3 + k] = v[9 + k] = -3.402823466e+38f;
    }
    for (int j = threadIdx.x; j < t.n; j += kB) {
        const Box6 b = pb[perm[t.start + j]];
        for (int k = 0; k < 3; ++k) {
            v[k] = fminf(v[k], b.mn[k]);
            v[3 + k] = fmaxf(v[3 + k], b.mx[k]);
            const float c = .5f * b.mn[k] + .5f * b.mx[k];
            v[6 + k] = fminf(v[6 + k], c);
            v[9 + k] = fmaxf(v[9 + k], c);
        }
    }
    for (int q = 0; q < 12; ++q) {
        const bool isMin = (q % 6) < 3;
        for (int off = 32; off >= 1; off >>= 1) {
            const float o = __shfl_xor(v[q], off);
            v[q] = isMin ? fminf(v[q], o) : fmaxf(v[q], o);
        }
    }
    if ((threadIdx.x & 63) == 0)
        for (int q = 0; q < 12; ++q) red[q][threadIdx.x >> 6] = v[q];
    __syncthreads();
    if (threadIdx.x < 12) {
        const int q = threadIdx.x;
        const bool isMin = (q % 6) < 3;
        float r = red[q][0];
        for (int w = 1; w < kB / 64; ++w) r = isMin ? fminf(r, red[q][w]) : fmaxf(r, red[q][w]);
        if (isMin) atomicMin(&segAcc[12 * t.seg + q], f2key(r));
        else atomicMax(&segAcc[12 * t.seg + q], f2key(r));
    }
}

// the 12 buckets of every big node: counts and bounds (:305-318)
__global__ __launch_bounds__(kB) void k_seg_buckets(const Tile *__restrict__ tiles, const SegInfo *__restrict__ info,
                                                    const Box6 *__restrict__ pb, const int *__restrict__ perm,
                                                    unsigned *segKeys, int *segCounts) {
    __shared__ unsigned keys[kSahBuckets * 6];
    __shared__ int counts[kSahBuckets];
    const Tile t = tiles[blockIdx.x];
    const SegInfo si = info[t.seg];
    if (threadIdx.x < kSahBuckets) counts[threadIdx.x] = 0;
    if (threadIdx.x < kSahBuckets * 6) keys[threadIdx.x] = (threadIdx.x % 6) < 3 ? 0xffffffffu : 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < t.n; j += kB) {
        const Box6 b = pb[perm[t.start + j]];
        const int bk = sah_bucket(centroid_of(b, si.dim), si.cmn, si.cmx);
        atomicAdd(&counts[bk], 1);
        for (int k = 0; k < 3; ++k) {
            atomicMin(&keys[bk * 6 + k], f2key(b.mn[k]));
            atomicMax(&keys[bk * 6 + 3 + k], f2key(b.mx[k]));
        }
    }
    __syncthreads();
    if (threadIdx.x < kSahBuckets && counts[threadIdx.x]) atomicAdd(&segCounts[kSahBuckets * t.seg + threadIdx.x], counts[threadIdx.x]);
    if (threadIdx.x < kSahBuckets * 6 && counts[threadIdx.x / 6]) {
        if ((threadIdx.x % 6) < 3) atomicMin(&segKeys[kSahBuckets * 6 * t.seg + threadIdx.x], keys[threadIdx.x]);
        else atomicMax(&segKeys[kSahBuckets * 6 * t.seg + threadIdx.x], keys[threadIdx.x]);
    }
}

// std::partition, step 1: who is on the wrong side of `mid`
__global__ __launch_bounds__(kB) void k_seg_flags(const Tile *__restrict__ tiles, const SegInfo *__restrict__ info,
                                                  const Box6 *__restrict__ pb, const int *__restrict__ perm,
                                                  int *__restrict__ lfFlag, int *__restrict__ rtFlag) {
    const Tile t = tiles[blockIdx.x];
    const SegInfo si = info[t.seg];
    for (int j = threadIdx.x; j < t.n; j += kB) {
        const int i = t.start + j;
        const bool pred = sah_bucket(centroid_of(pb[perm[i]], si.dim), si.cmn, si.cmx) <= si.best;
        const bool left = i < si.start + si.mid;
        lfFlag[i] = (left && !pred) ? 1 : 0;
        rtFlag[i] = (!left && pred) ? 1 : 0;
    }
}
// step 2: the k-th offender of the left part (from the left) and of the right part (from the right)
__global__ __launch_bounds__(kB) void k_seg_positions(const Tile *__restrict__ tiles, const SegInfo *__restrict__ info,
                                                      const int *__restrict__ lfFlag, const int *__restrict__ lfScan,
                                                      const int *__restrict__ rtFlag, const int *__restrict__ rtScan,
                                                      int *__restrict__ lfPos, int *__restrict__ rtPos) {
    const Tile t = tiles[blockIdx.x];
    const SegInfo si = info[t.seg];
    const int end = si.start + si.n;
    for (int j = threadIdx.x; j < t.n; j += kB) {
        const int i = t.start + j;
        if (lfFlag[i]) lfPos[si.start + (lfScan[i] - lfScan[si.start])] = i;
        if (rtFlag[i]) rtPos[si.start + (rtScan[end] - rtScan[i + 1])] = i;
    }
}
// step 3: swap them pairwise
__global__ __launch_bounds__(kB) void k_seg_swap(const Tile *__restrict__ tiles, const SegInfo *__restrict__ info,
                                                 const int *__restrict__ lfScan, const int *__restrict__ lfPos,
                                                 const int *__restrict__ rtPos, int *perm) {
    const Tile t = tiles[blockIdx.x];
    const SegInfo si = info[t.seg];
    const int nSwaps = lfScan[si.start + si.mid] - lfScan[si.start];
    for (int j = threadIdx.x; j < t.n; j += kB) {
        const int k = t.start + j - si.start;
        if (k < nSwaps) {
            const int a = lfPos[si.start + k], b = rtPos[si.start + k];
            const int va = perm[a], vb = perm[b];
            perm[a] = vb;
            perm[b] = va;
        }
    }
}

// per-node decisions on the device (one thread per big node of the level): nothing but the final
// {dim, mid} verdicts crosses PCIe
struct SegStart {
    int start, n;
};
__global__ __launch_bounds__(kB) void k_seg_init(int nSeg, unsigned *__restrict__ segAcc, unsigned *__restrict__ segKeys,
                                                 int *__restrict__ segCounts) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i < 12 * nSeg) segAcc[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
    if (i < kSahBuckets * 6 * nSeg) segKeys[i] = (i % 6) < 3 ? 0xffffffffu : 0u;
    if (i < kSahBuckets * nSeg) segCounts[i] = 0;
}
// :221, :241-253: flat bounds or coincident centroids -> no split (the node is handed to a wavefront,
// which makes the leaf); otherwise the split axis and the centroid range along it
__global__ __launch_bounds__(kB) void k_seg_prepare(const SegStart *__restrict__ segs, int nSeg,
                                                    const unsigned *__restrict__ segAcc, SegInfo *__restrict__ info,
                                                    HBox *__restrict__ segBounds) {
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= nSeg) return;
    HBox b, cb;
    for (int k = 0; k < 3; ++k) {
        b.mn[k] = sah_key_to_float(segAcc[12 * s + k]);
        b.mx[k] = sah_key_to_float(segAcc[12 * s + 3 + k]);
        cb.mn[k] = sah_key_to_float(segAcc[12 * s + 6 + k]);
        cb.mx[k] = sah_key_to_float(segAcc[12 * s + 9 + k]);
    }
    const int dim = hb_maxdim(cb);
    const bool noSplit = hb_area(b) == 0 || cb.mx[dim] == cb.mn[dim];
    SegInfo si;
    si.start = segs[s].start;
    si.n = segs[s].n;
    si.mid = 0;
    si.dim = dim;
    si.best = noSplit ? -2 : -1;  // -2: decided, no split; -1: buckets wanted
    si.cmn = cb.mn[dim];
    si.cmx = cb.mx[dim];
    info[s] = si;
    segBounds[s] = b;
}
__global__ __launch_bounds__(kB) void k_seg_choose(int nSeg, int maxPrims, const int *__restrict__ segCounts,
                                                   const unsigned *__restrict__ segKeys,
                                                   const HBox *__restrict__ segBounds, SegInfo *info,
                                                   int2 *__restrict__ verdict) {
    const int s = blockIdx.x * kB + threadIdx.x;
    if (s >= nSeg) return;
    SegInfo si = info[s];
    int mid = 0;
    if (si.best != -2) {
        const SahChoice ch = sah_choose(segCounts + kSahBuckets * s, segKeys + kSahBuckets * 6 * s, segBounds[s], si.n,
                                        maxPrims);
        if (ch.split && ch.mid > 0 && ch.mid < si.n) {
            si.best = ch.best;
            mid = ch.mid;
        } else {
            si.best = -1;
        }
    } else {
        si.best = -1;
    }
    si.mid = mid;  // mid == 0: no split; the flags kernel then leaves the node's primitives in place
    info[s] = si;
    verdict[s] = make_int2(si.dim, mid);
}

// ---- phase B: one wavefront builds one subtree ----------------------------------------------------------
struct SmallSeg {
    int start, n, pool;  // start: position in the forest's permutation array
    int object, first;   // the object it belongs to and that object's first primitive (leaf offsets count from there)
};
// Pending second children: the first kSubtreeStack of a subtree's in LDS.  A left spine longer than that (only
// primitives whose centroids grow geometrically make one) keeps the rest in the tree itself: the interior node that
// waits for its second child holds the child's range in pmin[0..1] and the node below it on the stack in pmin[2],
// fields phase C overwrites with the bounds.
constexpr int kSubtreeStack = 64;

// sah_choose for a wavefront: lane i < 11 prices split i (the same additions in the same order as
// the sequential loops: buckets 0..i ascending for the part below, 11..i+1 descending for the part
// above, cost = (0 + below) + above), then every lane scans the 11 costs in order, first minimum wins.
__device__ __forceinline__ SahChoice sah_choose_wave(int lane, const int *count, const unsigned *keys,
                                                     const HBox &bounds, int n, int maxPrims) {
    float cost = __builtin_inff();
    if (lane < kSahBuckets - 1) {
        HBox acc;
        hb_init(acc);
        int cnt = 0;
#pragma unroll 1
        for (int q = 0; q <= lane; ++q) {
            hb_add(acc, sah_bucket_box(keys, q));
            cnt += count[q];
        }
        float c = 0;
        c += cnt * hb_area(acc);
        hb_init(acc);
        cnt = 0;
#pragma unroll 1
        for (int q = kSahBuckets - 1; q > lane; --q) {
            hb_add(acc, sah_bucket_box(keys, q));
            cnt += count[q];
        }
        c += cnt * hb_area(acc);
        cost = c;
    }
    int best = -1;
    float minCost = __builtin_inff();
#pragma unroll 1
    for (int i = 0; i < kSahBuckets - 1; ++i) {
        const float c = __shfl(cost, i);
        if (c < minCost) {
            minCost = c;
            best = i;
        }
    }
    const float leafCost = (float)n;
    minCost = 1.f / 2.f + minCost / hb_area(bounds);
    SahChoice ch;
    ch.best = best;
    ch.split = (n > maxPrims || minCost < leafCost) ? 1 : 0;
    ch.mid = 0;
#pragma unroll 1
    for (int i = 0; i <= best; ++i) ch.mid += count[i];
    return ch;
}

__global__ __launch_bounds__(64) void k_sah_subtrees(const SmallSeg *__restrict__ segs, int nSegs, int maxPrims,
                                                     const Box6 *__restrict__ pb, int *perm, int *lfPos, int *rtPos,
                                                     nnbvh_linear_node *pool, int *segCount, int *segDepth,
                                                     int *errObj) {
    __shared__ int stStart[kSubtreeStack], stN[kSubtreeStack], stParent[kSubtreeStack], stDepth[kSubtreeStack];
    __shared__ unsigned bkeys[kSahBuckets * 6];
    __shared__ int bcount[kSahBuckets];
    __shared__ int lpos[64], rpos[64];
    const int s = blockIdx.x;
    if (s >= nSegs) return;
    const int lane = threadIdx.x;
    const SmallSeg sg = segs[s];
    nnbvh_linear_node *nodes = pool + sg.pool;
    int sp = 0, idx = 0, maxDepth = 0;
    int top = -1;  // the node holding stack entry sp - 1, while sp > kSubtreeStack
    int start = sg.start, n = sg.n, depth = 0;
    for (;;) {
        const int me = idx++;
        // A node of at most 64 primitives lives in registers (one primitive per lane) for all of its
        // passes; larger ones loop over their range.
        const bool small = n <= 64;
        const bool mine = lane < n;
        int myIdx = -1;
        Box6 myBox;
        box_init(myBox);
        if (mine) {
            myIdx = perm[start + lane];
            myBox = pb[myIdx];
        }
        // bounds and centroid bounds of the node (values)
        float v[12];
        for (int k = 0; k < 3; ++k) {
            v[k] = v[6 + k] = 3.402823466e+38f;
            v[3 + k] = v[9 + k] = -3.402823466e+38f;
        }
        if (mine)
            for (int k = 0; k < 3; ++k) {
                v[k] = myBox.mn[k];
                v[3 + k] = myBox.mx[k];
                v[6 + k] = v[9 + k] = .5f * myBox.mn[k] + .5f * myBox.mx[k];
            }
        for (int j = lane + 64; j < n; j += 64) {
            const Box6 b = pb[perm[start + j]];
            for (int k = 0; k < 3; ++k) {
                v[k] = fminf(v[k], b.mn[k]);
                v[3 + k] = fmaxf(v[3 + k], b.mx[k]);
                const float c = .5f * b.mn[k] + .5f * b.mx[k];
                v[6 + k] = fminf(v[6 + k], c);
                v[9 + k] = fmaxf(v[9 + k], c);
            }
        }
        // butterfly over the lanes that can hold data (lanes >= n hold the neutral element); most
        // nodes are tiny, so most of the 6 steps are skipped
        int span = 64;
        if (n < 64) {
            span = 1;
            while (span < n) span <<= 1;
        }
        for (int q = 0; q < 12; ++q) {
            const bool isMin = (q % 6) < 3;
            for (int off = 32; off >= 1; off >>= 1) {
                if (off >= span) continue;
                const float o = __shfl_xor(v[q], off);
                v[q] = isMin ? fminf(v[q], o) : fmaxf(v[q], o);
            }
            v[q] = __shfl(v[q], 0);  // one value for the whole wavefront (a zero's sign may differ per lane)
        }
        HBox bounds, cb;
        for (int k = 0; k < 3; ++k) {
            bounds.mn[k] = v[k], bounds.mx[k] = v[3 + k];
            cb.mn[k] = v[6 + k], cb.mx[k] = v[9 + k];
        }
        bool leaf = hb_area(bounds) == 0 || n == 1;  // :221
        int dim = 0, mid = 0, best = 0;
        bool refused = false;
        if (!leaf) {
            dim = hb_maxdim(cb);
            if (cb.mx[dim] == cb.mn[dim]) leaf = true;  // :243
        }
        if (!leaf) {
            const float cmn = cb.mn[dim], cmx = cb.mx[dim];
            if (n <= 2) {  // :289-296: nth_element of two = put the smaller centroid first
                const float c0 = __shfl(centroid_of(myBox, dim), 0), c1 = __shfl(centroid_of(myBox, dim), 1);
                if (c1 < c0 && lane < 2) perm[start + (1 - lane)] = myIdx;
                mid = n / 2;
                __threadfence_block();
            } else {
                if (lane < kSahBuckets) bcount[lane] = 0;
                for (int q = lane; q < kSahBuckets * 6; q += 64) bkeys[q] = (q % 6) < 3 ? 0xffffffffu : 0u;
                __syncthreads();
                int myBucket = 0;
                if (mine) {
                    myBucket = sah_bucket(centroid_of(myBox, dim), cmn, cmx);
                    atomicAdd(&bcount[myBucket], 1);
                    for (int k = 0; k < 3; ++k) {
                        atomicMin(&bkeys[myBucket * 6 + k], f2key(myBox.mn[k]));
                        atomicMax(&bkeys[myBucket * 6 + 3 + k], f2key(myBox.mx[k]));
                    }
                }
                for (int j = lane + 64; j < n; j += 64) {
                    const Box6 b = pb[perm[start + j]];
                    const int bk = sah_bucket(centroid_of(b, dim), cmn, cmx);
                    atomicAdd(&bcount[bk], 1);
                    for (int k = 0; k < 3; ++k) {
                        atomicMin(&bkeys[bk * 6 + k], f2key(b.mn[k]));
                        atomicMax(&bkeys[bk * 6 + 3 + k], f2key(b.mx[k]));
                    }
                }
                __syncthreads();
                const SahChoice ch = sah_choose_wave(lane, bcount, bkeys, bounds, n, maxPrims);
                __syncthreads();  // everyone has read the buckets before the next node clears them
                if (ch.best < 0) {  // no split costs less than +inf: refused, as by the host builder
                    if (lane == 0) atomicMin(&errObj[kErrSahCosts], sg.object);  // a word of its own: no other error hides it
                    refused = true;
                    leaf = true;
                } else if (!ch.split) {
                    leaf = true;
                } else if (small) {
                    best = ch.best;
                    mid = ch.mid;
                    // std::partition(bucket <= best) by ranks, in registers: the k-th offender of the
                    // left part (from the left) trades places with the k-th of the right part from the right
                    const bool pred = myBucket <= best;
                    const bool leftOff = mine && lane < mid && !pred, rightOff = mine && lane >= mid && pred;
                    const unsigned long long mL = __ballot(leftOff), mR = __ballot(rightOff);
                    const int kL = __popcll(mL & ((1ull << lane) - 1ull));
                    const int kR = lane == 63 ? 0 : __popcll(mR >> (lane + 1));
                    if (leftOff) lpos[kL] = lane;
                    if (rightOff) rpos[kR] = lane;
                    __syncthreads();
                    if (leftOff) perm[start + rpos[kL]] = myIdx;
                    if (rightOff) perm[start + lpos[kR]] = myIdx;
                    if (__popcll(mL) != __popcll(mR) && lane == 0) errObj[0] = 100;  // cannot happen
                    __syncthreads();
                    __threadfence_block();
                } else {
                    best = ch.best;
                    mid = ch.mid;
                    // the same by ranks through scratch: offenders of the left part from the left ...
                    int nl = 0;
                    for (int base = 0; base < mid; base += 64) {
                        const int j = base + lane;
                        bool f = false;
                        if (j < mid) f = sah_bucket(centroid_of(pb[perm[start + j]], dim), cmn, cmx) > best;
                        const unsigned long long mask = __ballot(f);
                        if (f) lfPos[start + nl + __popcll(mask & ((1ull << lane) - 1ull))] = start + j;
                        nl += __popcll(mask);
                    }
                    // ... offenders of the right part from the right
                    int nr = 0;
                    for (int top = n; top > mid; top -= 64) {
                        const int j = top - 1 - lane;
                        bool f = false;
                        if (j >= mid) f = sah_bucket(centroid_of(pb[perm[start + j]], dim), cmn, cmx) <= best;
                        const unsigned long long mask = __ballot(f);
                        if (f) rtPos[start + nr + __popcll(mask & ((1ull << lane) - 1ull))] = start + j;
                        nr += __popcll(mask);
                    }
                    if (nl != nr && lane == 0) errObj[0] = 100;  // cannot happen: both equal the number of swaps
                    __threadfence_block();
                    for (int k = lane; k < nl; k += 64) {
                        const int a = lfPos[start + k], b = rtPos[start + k];
                        const int va = perm[a], vb = perm[b];
                        perm[a] = vb;
                        perm[b] = va;
                    }
                    __threadfence_block();
                }
            }
        }
        if (!leaf) {
            if (mid <= 0 || mid >= n) {  // cannot happen (buckets 0 and 11 are never empty): no endless loop
                if (lane == 0) errObj[0] = 101;
                leaf = true;
            }
        }
        if (!leaf) {
            const bool inLds = sp < kSubtreeStack;
            if (lane == 0) {
                nnbvh_linear_node nd;
                for (int k = 0; k < 3; ++k) nd.pmin[k] = nd.pmax[k] = 0;
                if (!inLds) {
                    nd.pmin[0] = __int_as_float(start + mid);
                    nd.pmin[1] = __int_as_float(n - mid);
                    nd.pmin[2] = __int_as_float(top);
                }
                nd.offset = 0;  // second child: set when it is created
                nd.nprims = 0;
                nd.axis = (uint8_t)dim;
                nd.pad = (uint8_t)depth;  // carried to phase C, cleared there
                nodes[me] = nd;
            }
            if (!inLds) {
                top = me;
            } else if (lane == 0) {
                stStart[sp] = start + mid;
                stN[sp] = n - mid;
                stParent[sp] = me;
                stDepth[sp] = depth + 1;
            }
            ++sp;
            n = mid;
            ++depth;
            __syncthreads();
            continue;
        }
        // leaf (:222-236 / :243-253 / :365-369): bounds = in-order fold over its primitives
        {
            Box6 b;
            if (small) {
                b = myBox;  // one primitive per lane, already in order (empty lanes hold the empty box)
            } else {
                const int chunk = (n + 63) / 64;
                const int lo = lane * chunk, hi = (lo + chunk < n) ? lo + chunk : n;
                box_init(b);
                for (int j = lo; j < hi; ++j) box_add(b, pb[perm[start + j]]);
            }
            for (int off = 1; off < (small ? span : 64); off <<= 1) {
                Box6 o;
                for (int k = 0; k < 3; ++k) {
                    o.mn[k] = __shfl_down(b.mn[k], off);
                    o.mx[k] = __shfl_down(b.mx[k], off);
                }
                if (lane + off < 64) box_add(b, o);
            }
            if (lane == 0) {
                nnbvh_linear_node nd;
                for (int k = 0; k < 3; ++k) {
                    nd.pmin[k] = b.mn[k];
                    nd.pmax[k] = b.mx[k];
                }
                nd.offset = start - sg.first;  // object-local, as the tree of the object alone has it
                nd.nprims = (uint16_t)n;
                nd.axis = 0;
                nd.pad = (uint8_t)depth;
                nodes[me] = nd;
                if (n > 65535 && !refused) atomicMin(&errObj[kErrLeafSize], sg.object);
            }
            if (depth > maxDepth) maxDepth = depth;
        }
        if (sp == 0) break;
        --sp;
        __syncthreads();
        if (sp >= kSubtreeStack) {  // the entry lives in the waiting node (written by lane 0 before a barrier)
            const int parent = top;
            start = __float_as_int(nodes[parent].pmin[0]);
            n = __float_as_int(nodes[parent].pmin[1]);
            top = __float_as_int(nodes[parent].pmin[2]);
            depth = (int)nodes[parent].pad + 1;
            __syncthreads();  // every lane has read the entry before lane 0 clears it
            if (lane == 0) {
                nodes[parent].pmin[0] = nodes[parent].pmin[1] = nodes[parent].pmin[2] = 0;
                nodes[parent].offset = idx;
            }
        } else {
            start = stStart[sp];
            n = stN[sp];
            depth = stDepth[sp];
            if (lane == 0) nodes[stParent[sp]].offset = idx;  // the node about to be created
        }
        __syncthreads();
    }
    if (lane == 0) {
        segCount[s] = idx;
        segDepth[s] = maxDepth;
    }
}

// ---- phase C ----------------------------------------------------------------------------------------------
// subtree slices -> final DFS positions
// where a subtree's slice goes: `at` in the forest's node array, `local` = the same place counted from its tree's
// root (what second-child offsets are relative to; the tree's root stands at at - local), `depth` of the slice's root
struct SegPlace {
    int at, local, depth;
};
__global__ __launch_bounds__(kB) void k_sah_emit(const SmallSeg *__restrict__ segs, const int *__restrict__ segCount,
                                                 const SegPlace *__restrict__ place,
                                                 const nnbvh_linear_node *__restrict__ pool,
                                                 nnbvh_linear_node *__restrict__ nodes, unsigned char *__restrict__ depthOf,
                                                 int *__restrict__ rootOf) {
    const int s = blockIdx.x;
    const int cnt = segCount[s];
    const SegPlace pl = place[s];
    const nnbvh_linear_node *src = pool + segs[s].pool;
    for (int i = threadIdx.x; i < cnt; i += kB) {
        nnbvh_linear_node nd = src[i];
        depthOf[pl.at + i] = (unsigned char)(pl.depth + nd.pad);
        rootOf[pl.at + i] = pl.at - pl.local;
        nd.pad = 0;
        if (nd.nprims == 0) nd.offset += pl.local;
        nodes[pl.at + i] = nd;
    }
}
struct UpperNode {
    int index, second, axis, depth, root;  // index, root: in the forest's node array; second: from the tree's root
};
__global__ __launch_bounds__(kB) void k_sah_upper(const UpperNode *__restrict__ up, int nUp,
                                                  nnbvh_linear_node *__restrict__ nodes, unsigned char *__restrict__ depthOf,
                                                  int *__restrict__ rootOf) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= nUp) return;
    nnbvh_linear_node nd;
    for (int k = 0; k < 3; ++k) nd.pmin[k] = nd.pmax[k] = 0;
    nd.offset = up[i].second;
    nd.nprims = 0;
    nd.axis = (uint8_t)up[i].axis;
    nd.pad = 0;
    nodes[up[i].index] = nd;
    depthOf[up[i].index] = (unsigned char)up[i].depth;
    rootOf[up[i].index] = up[i].root;
}
// interior bounds = Union(child 0, child 1) (:371-373), one tree level per launch, deepest first
__global__ __launch_bounds__(kB) void k_sah_level_bounds(int nNodes, int level, const unsigned char *__restrict__ depthOf,
                                                         const int *__restrict__ rootOf, nnbvh_linear_node *nodes) {
    const int i = blockIdx.x * kB + threadIdx.x;
    if (i >= nNodes || depthOf[i] != level || nodes[i].nprims != 0) return;
    const nnbvh_linear_node c0 = nodes[i + 1], c1 = nodes[rootOf[i] + nodes[i].offset];
    Box6 b, o;
    box_init(b);
    for (int k = 0; k < 3; ++k) o.mn[k] = c0.pmin[k], o.mx[k] = c0.pmax[k];
    box_add(b, o);
    for (int k = 0; k < 3; ++k) o.mn[k] = c1.pmin[k], o.mx[k] = c1.pmax[k];
    box_add(b, o);
    for (int k = 0; k < 3; ++k) nodes[i].pmin[k] = b.mn[k], nodes[i].pmax[k] = b.mx[k];
}

struct HostNode {  // a phase-A node
    int child[2];  // >= 0: HostNode index; < 0: ~(small segment index)
    int axis;
};

}  // namespace

bool gpu_sah(const nnbvh_prim *prims, int n, const float *verts, int n_verts, const float *prim_bounds,
             int max_prims_in_node, int device, GpuBuildResult *out, std::string *error) {
    return build_uploaded(gpu_sah_device, prims, n, verts, n_verts, prim_bounds, max_prims_in_node, device, out, error);
}

bool gpu_sah_device(const DeviceBuildInput &in, GpuBuildResult *out, std::string *error) {
    return build_one_object(gpu_sah_forest_device, &ForestBuildResult::n_upper, in, out, error);
}

bool gpu_sah_forest_device(const DeviceBuildInput &in, const int *objectFirst, int nObjects, ForestBuildResult *out,
                           std::string *error) {
    const int nAll = in.n_prims, n_verts = in.n_verts;
    if (!check_object_first(objectFirst, nObjects, nAll, error)) return false;
    const nnbvh_prim *dPrims = in.d_prims;
    const float *dVerts = in.d_verts, *dCaller = in.d_prim_bounds;
    const int maxPrims = std::min(255, in.max_prims_in_node);
    int kSmallSegment = kSmallSegmentDefault;  // speed only: where breadth-first hands over to wavefronts
    if (const char *e = std::getenv("NNBVH_SAH_SMALL")) kSmallSegment = std::max(2, std::atoi(e));
    hipStream_t stream = (hipStream_t)in.stream;
    DevMem mem, outMem;  // outMem: the result arrays this call allocates itself
    mem.error = outMem.error = error;
    mem.pool = in.pool;

    Refusal refuse;

    auto t0 = std::chrono::steady_clock::now();
    Box6 *dPb = mem.get<Box6>(nAll);
    int *dPerm = mem.get<int>(nAll);
    int *dLfFlag = mem.get<int>((size_t)nAll + 1), *dRtFlag = mem.get<int>((size_t)nAll + 1);
    int *dLfScan = mem.get<int>((size_t)nAll + 1), *dRtScan = mem.get<int>((size_t)nAll + 1);
    int *dLfPos = mem.get<int>(nAll), *dRtPos = mem.get<int>(nAll);
    int *dObjectFirst = mem.get<int>((size_t)nObjects + 1);
    int *dScalars = mem.get<int>(8 + kErrWords);  // [0..5] centroid-bound keys (k_prim_bounds' by-product), [8..] errObj
    if (!mem.ok) return false;
    int init[8 + kErrWords] = {-1, -1, -1, 0, 0, 0, 0, 0};  // min keys all-ones, max keys 0, errObj[0] = 0
    for (int k = 1; k < kErrWords; ++k) init[8 + k] = kNoObject;
    GB_CHECK(hipMemcpyAsync(dScalars, init, sizeof init, hipMemcpyHostToDevice, stream), "init scalars");
    GB_CHECK(hipMemcpyAsync(dObjectFirst, objectFirst, ((size_t)nObjects + 1) * sizeof(int), hipMemcpyHostToDevice, stream),
             "copy object_first");
    int *dErrObj = dScalars + 8;
    hipLaunchKernelGGL(k_prim_bounds, dim3(grid_for(nAll, 1024)), dim3(kB), 0, stream, dPrims, dVerts, n_verts, dCaller, nAll,
                       dPb, (unsigned *)dScalars, (const int *)dObjectFirst, nObjects, dErrObj);
    hipLaunchKernelGGL(k_iota, dim3(grid_for(nAll)), dim3(kB), 0, stream, nAll, dPerm);
    size_t scanBytes = 0;
    GB_CHECK(rocprim::exclusive_scan(nullptr, scanBytes, dLfFlag, dLfScan, 0, (size_t)nAll + 1, rocprim::plus<int>(), stream),
             "scan (size query)");
    void *dTmp = mem.get<char>(scanBytes);
    if (!mem.ok) return false;
    int errWords[kErrWords];
    GB_CHECK(hipMemcpyAsync(errWords, dErrObj, sizeof errWords, hipMemcpyDeviceToHost, stream), "read error words");
    GB_CHECK(hipStreamSynchronize(stream), "sync after bounds");
    refuse(errWords[kErrVertex], "nnbvh_build_create: vertex index out of range");
    refuse(errWords[kErrNeedBounds], "nnbvh_build_create: instance / host primitives need prim_bounds");
    refuse(errWords[kErrNonFinite], "nnbvh_build_create: non-finite vertex or primitive bounds");
    refuse(errWords[kErrKind], "nnbvh_build_create: unknown primitive kind");
    // Objects from the first malformed one on are not built: only a lower-numbered object can still change the
    // message, and no malformed primitive reaches the phases below.
    const int nBuild = std::min(nObjects, refuse.object);
    if (nBuild == 0) {
        *error = refuse.text;
        return false;
    }
    const int n = objectFirst[nBuild];

    // ---- phase A: big nodes, breadth-first, every object's at once -------------------------------------------
    struct Big {
        int start, n, host, object;  // host = HostNode index
    };
    std::vector<HostNode> hostNodes;
    std::vector<SmallSeg> smallSegs;
    std::vector<Big> level;
    std::vector<int> rootRef((size_t)nBuild);  // >= 0 host node, < 0 ~small segment
    auto make_child = [&](int start, int cnt, int object, std::vector<Big> &next) -> int {
        if (cnt > kSmallSegment) {
            hostNodes.push_back(HostNode{{0, 0}, 0});
            next.push_back(Big{start, cnt, (int)hostNodes.size() - 1, object});
            return (int)hostNodes.size() - 1;
        }
        smallSegs.push_back(SmallSeg{start, cnt, 0, object, objectFirst[object]});
        return ~((int)smallSegs.size() - 1);
    };
    for (int k = 0; k < nBuild; ++k) rootRef[(size_t)k] = make_child(objectFirst[k], objectFirst[k + 1] - objectFirst[k], k, level);
    std::vector<Tile> tiles;
    Tile *dTiles = nullptr;
    SegInfo *dInfo = nullptr;
    unsigned *dAcc = nullptr, *dBKeys = nullptr;
    int *dBCounts = nullptr;
    size_t capTiles = 0, capSegs = 0;
    std::vector<SegStart> segStarts;
    std::vector<int2> verdicts;
    SegStart *dSegStart = nullptr;
    HBox *dSegBounds = nullptr;
    int2 *dVerdict = nullptr;
    int nLevels = 0;
    while (!level.empty()) {
        ++nLevels;
        const int nSeg = (int)level.size();
        tiles.clear();
        segStarts.resize((size_t)nSeg);
        for (int s = 0; s < nSeg; ++s) {
            segStarts[(size_t)s] = SegStart{level[s].start, level[s].n};
            for (int off = 0; off < level[s].n; off += kTile)
                tiles.push_back(Tile{s, level[s].start + off, std::min(kTile, level[s].n - off)});
        }
        if (tiles.size() > capTiles) {
            capTiles = tiles.size() * 2;
            dTiles = mem.get<Tile>(capTiles);
        }
        if ((size_t)nSeg > capSegs) {
            capSegs = (size_t)nSeg * 2;
            dInfo = mem.get<SegInfo>(capSegs);
            dAcc = mem.get<unsigned>(12 * capSegs);
            dBKeys = mem.get<unsigned>(kSahBuckets * 6 * capSegs);
            dBCounts = mem.get<int>(kSahBuckets * capSegs);
            dSegStart = mem.get<SegStart>(capSegs);
            dSegBounds = mem.get<HBox>(capSegs);
            dVerdict = mem.get<int2>(capSegs);
        }
        if (!mem.ok) return false;
        const int nTiles = (int)tiles.size();
        GB_CHECK(hipMemcpyAsync(dTiles, tiles.data(), tiles.size() * sizeof(Tile), hipMemcpyHostToDevice, stream), "copy tiles");
        GB_CHECK(hipMemcpyAsync(dSegStart, segStarts.data(), segStarts.size() * sizeof(SegStart), hipMemcpyHostToDevice, stream),
                 "copy nodes");
        hipLaunchKernelGGL(k_seg_init, dim3(grid_all((long)kSahBuckets * 6 * nSeg)), dim3(kB), 0, stream, nSeg, dAcc, dBKeys,
                           dBCounts);
        hipLaunchKernelGGL(k_seg_reduce, dim3(nTiles), dim3(kB), 0, stream, dTiles, dPb, dPerm, dAcc);
        hipLaunchKernelGGL(k_seg_prepare, dim3(grid_all(nSeg)), dim3(kB), 0, stream, dSegStart, nSeg, dAcc, dInfo, dSegBounds);
        hipLaunchKernelGGL(k_seg_buckets, dim3(nTiles), dim3(kB), 0, stream, dTiles, dInfo, dPb, dPerm, dBKeys, dBCounts);
        hipLaunchKernelGGL(k_seg_choose, dim3(grid_all(nSeg)), dim3(kB), 0, stream, nSeg, maxPrims, dBCounts, dBKeys, dSegBounds,
                           dInfo, dVerdict);
        GB_CHECK(hipMemsetAsync(dLfFlag, 0, ((size_t)n + 1) * sizeof(int), stream), "memset");
        GB_CHECK(hipMemsetAsync(dRtFlag, 0, ((size_t)n + 1) * sizeof(int), stream), "memset");
        hipLaunchKernelGGL(k_seg_flags, dim3(nTiles), dim3(kB), 0, stream, dTiles, dInfo, dPb, dPerm, dLfFlag, dRtFlag);
        GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dLfFlag, dLfScan, 0, (size_t)n + 1, rocprim::plus<int>(), stream), "scan");
        GB_CHECK(rocprim::exclusive_scan(dTmp, scanBytes, dRtFlag, dRtScan, 0, (size_t)n + 1, rocprim::plus<int>(), stream), "scan");
        hipLaunchKernelGGL(k_seg_positions, dim3(nTiles), dim3(kB), 0, stream, dTiles, dInfo, dLfFlag, dLfScan, dRtFlag,
                           dRtScan, dLfPos, dRtPos);
        hipLaunchKernelGGL(k_seg_swap, dim3(nTiles), dim3(kB), 0, stream, dTiles, dInfo, dLfScan, dLfPos, dRtPos, dPerm);
        verdicts.resize((size_t)nSeg);
        GB_CHECK(hipMemcpyAsync(verdicts.data(), dVerdict, (size_t)nSeg * sizeof(int2), hipMemcpyDeviceToHost, stream), "read verdicts");
        GB_CHECK(hipStreamSynchronize(stream), "sync (level)");
        std::vector<Big> next;
        for (int s = 0; s < nSeg; ++s) {
            const int dim = verdicts[(size_t)s].x, mid = verdicts[(size_t)s].y;
            const int host = level[s].host, object = level[s].object;
            if (mid <= 0) {
                // a big node that does not split (coincident centroids / flat bounds): it becomes a
                // subtree for the wavefront builder, which reaches the same verdict and makes the leaf
                smallSegs.push_back(SmallSeg{level[s].start, level[s].n, 0, object, objectFirst[object]});
                hostNodes[(size_t)host].axis = -1;
                hostNodes[(size_t)host].child[0] = ~((int)smallSegs.size() - 1);
                hostNodes[(size_t)host].child[1] = 0;
                continue;
            }
            const int c0 = make_child(level[s].start, mid, object, next);
            const int c1 = make_child(level[s].start + mid, level[s].n - mid, object, next);
            hostNodes[(size_t)host].axis = dim;  // (index again: make_child may have grown the vector)
            hostNodes[(size_t)host].child[0] = c0;
            hostNodes[(size_t)host].child[1] = c1;
        }
        level.swap(next);
    }
    // k_seg_flags marks delegated nodes' primitives with pred = (bucket <= -1) = false and mid = 0:
    // every one of them is "right part, predicate false" -> stays in place.
    out->ms[1] = ms_since(t0);

    // ---- phase B: every object's subtrees in one launch ---------------------------------------------------------
    t0 = std::chrono::steady_clock::now();
    const int nSmall = (int)smallSegs.size();
    long poolTotal = 0;
    for (SmallSeg &sg : smallSegs) {
        sg.pool = (int)poolTotal;
        poolTotal += 2L * sg.n - 1;
    }
    if (poolTotal >= 0x7fffffffL) {
        *error = "gpu build: too many nodes";
        return false;
    }
    SmallSeg *dSegs = mem.get<SmallSeg>(nSmall);
    nnbvh_linear_node *dPool = mem.get<nnbvh_linear_node>((size_t)poolTotal);
    int *dSegCount = mem.get<int>(nSmall), *dSegDepth = mem.get<int>(nSmall);
    if (!mem.ok) return false;
    GB_CHECK(hipMemcpyAsync(dSegs, smallSegs.data(), (size_t)nSmall * sizeof(SmallSeg), hipMemcpyHostToDevice, stream), "copy subtrees");
    hipLaunchKernelGGL(k_sah_subtrees, dim3(nSmall), dim3(64), 0, stream, dSegs, nSmall, maxPrims, dPb, dPerm, dLfPos,
                       dRtPos, dPool, dSegCount, dSegDepth, dErrObj);
    std::vector<int> segCount((size_t)nSmall), segDepth((size_t)nSmall);
    GB_CHECK(hipMemcpyAsync(segCount.data(), dSegCount, (size_t)nSmall * sizeof(int), hipMemcpyDeviceToHost, stream), "read counts");
    GB_CHECK(hipMemcpyAsync(segDepth.data(), dSegDepth, (size_t)nSmall * sizeof(int), hipMemcpyDeviceToHost, stream), "read depths");
    GB_CHECK(hipMemcpyAsync(errWords, dErrObj, sizeof errWords, hipMemcpyDeviceToHost, stream), "read error words");
    GB_CHECK(hipStreamSynchronize(stream), "sync (subtrees)");
    if (errWords[0] != 0) {
        *error = "gpu build: internal error " + std::to_string(errWords[0]);
        return false;
    }
    refuse(errWords[kErrSahCosts], kSahCostsErrorText);  // first, as on the host, whatever else the object's subtrees reported
    refuse(errWords[kErrLeafSize], "nnbvh_build_create: a leaf would hold more than 65535 primitives");
    out->ms[2] = ms_since(t0);

    // ---- phase C: DFS layout (flattenBVH, :505-522), tree after tree ------------------------------------------
    t0 = std::chrono::steady_clock::now();
    std::vector<SegPlace> place((size_t)nSmall);
    std::vector<UpperNode> upper;
    out->node_first.assign((size_t)nBuild + 1, 0);
    out->depth.assign((size_t)nBuild, 0);
    int maxDepthAll = 0;
    // iterative DFS over the phase-A tree
    struct Frame {
        int ref, depth, parentUpper, which;
    };
    std::vector<Frame> stack;
    for (int k = 0; k < nBuild; ++k) {
        const int root = out->node_first[(size_t)k];
        int offset = 0, maxDepth = 0;  // offset: from the tree's own root
        stack.push_back(Frame{rootRef[(size_t)k], 0, -1, 0});
        while (!stack.empty()) {
            Frame f = stack.back();
            stack.pop_back();
            int ref = f.ref;
            // a delegated big node stands for its subtree
            if (ref >= 0 && hostNodes[(size_t)ref].axis < 0) ref = hostNodes[(size_t)ref].child[0];
            if (f.which == 1) upper[(size_t)f.parentUpper].second = offset;
            if (ref < 0) {
                const int sidx = ~ref;
                place[(size_t)sidx] = SegPlace{root + offset, offset, f.depth};
                offset += segCount[(size_t)sidx];
                maxDepth = std::max(maxDepth, f.depth + segDepth[(size_t)sidx]);
                continue;
            }
            const HostNode &hn = hostNodes[(size_t)ref];
            upper.push_back(UpperNode{root + offset, 0, hn.axis, f.depth, root});
            const int me = (int)upper.size() - 1;
            ++offset;
            stack.push_back(Frame{hn.child[1], f.depth + 1, me, 1});  // popped after the whole left subtree
            stack.push_back(Frame{hn.child[0], f.depth + 1, me, 0});
        }
        if ((long)root + offset >= 0x7fffffffL) {
            *error = "gpu build: too many nodes";
            return false;
        }
        out->node_first[(size_t)k + 1] = root + offset;
        out->depth[(size_t)k] = maxDepth;
        maxDepthAll = std::max(maxDepthAll, maxDepth);
        if (maxDepth > 255) {
            refuse(k, "gpu build: tree deeper than 255 levels");
            break;  // (no later object changes the message)
        }
    }
    if (refuse.object != kNoObject) {
        *error = refuse.text;
        return false;
    }
    const int totalNodes = out->node_first[(size_t)nBuild];
    nnbvh_linear_node *dNodes = in.d_nodes_out ? in.d_nodes_out : outMem.get<nnbvh_linear_node>((size_t)totalNodes);
    unsigned char *dDepthOf = mem.get<unsigned char>((size_t)totalNodes);
    int *dRootOf = mem.get<int>((size_t)totalNodes);
    SegPlace *dPlace = mem.get<SegPlace>(nSmall);
    UpperNode *dUpper = mem.get<UpperNode>(upper.size());
    nnbvh_prim *dOrdered = in.d_ordered_out ? in.d_ordered_out : outMem.get<nnbvh_prim>(n);
    if (!mem.ok || !outMem.ok) return false;
    GB_CHECK(hipMemcpyAsync(dPlace, place.data(), (size_t)nSmall * sizeof(SegPlace), hipMemcpyHostToDevice, stream), "copy bases");
    if (!upper.empty())
        GB_CHECK(hipMemcpyAsync(dUpper, upper.data(), upper.size() * sizeof(UpperNode), hipMemcpyHostToDevice, stream), "copy upper nodes");
    hipLaunchKernelGGL(k_sah_emit, dim3(nSmall), dim3(kB), 0, stream, dSegs, dSegCount, dPlace, dPool, dNodes, dDepthOf, dRootOf);
    if (!upper.empty())
        hipLaunchKernelGGL(k_sah_upper, dim3(grid_all((long)upper.size())), dim3(kB), 0, stream, dUpper, (int)upper.size(),
                           dNodes, dDepthOf, dRootOf);
    for (int lvl = maxDepthAll - 1; lvl >= 0; --lvl)
        hipLaunchKernelGGL(k_sah_level_bounds, dim3(grid_all(totalNodes)), dim3(kB), 0, stream, totalNodes, lvl, dDepthOf, dRootOf,
                           dNodes);
    hipLaunchKernelGGL(k_gather_prims, dim3(grid_for(n)), dim3(kB), 0, stream, dPrims, dPerm, n, dOrdered);
    GB_CHECK(hipGetLastError(), "kernel launch");
    GB_CHECK(hipStreamSynchronize(stream), "sync after emit");
    out->ms[3] = ms_since(t0);

    out->total_nodes = totalNodes;
    out->d_nodes = dNodes;
    out->d_ordered = dOrdered;
    outMem.release(dNodes);
    outMem.release(dOrdered);
    out->n_levels = nLevels;
    out->n_subtrees = nSmall;
    out->n_upper = (int)upper.size();
    return true;
}

}  // namespace nnbvh

