// capi_quality.cpp — the C ABI of include/nnbvh.h, tree-quality part: the fork's SAH and EPO scores of a baked tree
// (machine_learning/nn_loss.py:119-135, 165-192).  Host code only: the argument and tree checks, the
// device buffers of one call, the constants and the two divisions.  The passes are tree_quality.hip's.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"
#include "tree_quality.h"

using namespace nnbvh;

namespace {

constexpr const char *kFn = "nnbvh_tree_quality_create: ";

bool finite3(const float *p) { return std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]); }

bool inside(const float *p, const nnbvh_linear_node &n) {
    return p[0] >= n.pmin[0] && p[0] <= n.pmax[0] && p[1] >= n.pmin[1] && p[1] <= n.pmax[1] && p[2] >= n.pmin[2] &&
           p[2] <= n.pmax[2];
}

struct TreeShape {
    int n_inner = 0, n_leaves = 0, depth = 0;
};

// Everything the passes rely on, O(nodes + prims), before any device is looked at.  Empty string: the tree may be walked.
std::string tree_fault(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims, int n_prims,
                       const float *verts, int n_verts, TreeShape *shape) {
    auto at = [](const char *what, long i) { return std::string(what) + " " + std::to_string(i); };
    for (int j = 0; j < n_prims; ++j) {
        const int kind = prims[j].kind;
        if (!is_triangle_kind(kind) && !is_alphatex_kind(kind))
            return at("ordered primitive", j) + " has kind " + std::to_string(kind) +
                   ": the fork defines both scores on triangles only (kinds 0, 4 .. 7, 16 .. 19)";
        for (int c = 0; c < 3; ++c)
            if (prims[j].v[c] < 0 || prims[j].v[c] >= n_verts)
                return at("ordered primitive", j) + ": vertex index " + std::to_string(prims[j].v[c]) +
                       " outside [0, " + std::to_string(n_verts) + ")";
    }
    for (int v = 0; v < n_verts; ++v)
        if (!finite3(verts + 3 * (size_t)v)) return at("vertex", v) + " is not finite";
    int n_leaves = 0;
    for (int i = 0; i < n_nodes; ++i) {
        const nnbvh_linear_node &n = nodes[i];
        if (!finite3(n.pmin) || !finite3(n.pmax)) return at("node", i) + ": a box corner is not finite";
        if (n.nprims == 0) {
            if (n.offset <= i + 1 || n.offset >= n_nodes)
                return at("node", i) + ": second-child offset " + std::to_string(n.offset) + " not in (" +
                       std::to_string(i + 1) + ", " + std::to_string(n_nodes) + ")";
        } else {
            ++n_leaves;
            if (n.offset < 0 || (long long)n.offset + n.nprims > n_prims)
                return at("node", i) + ": leaf range [" + std::to_string(n.offset) + ", " +
                       std::to_string((long long)n.offset + n.nprims) + ") outside [0, " + std::to_string(n_prims) + ")";
        }
    }
    // every ordered position in exactly one leaf (stops at the first position met twice: at most n_prims + one leaf)
    std::vector<uint8_t> covered((size_t)n_prims, 0);
    for (int i = 0; i < n_nodes; ++i)
        for (int j = 0; j < (int)nodes[i].nprims; ++j) {
            const int pos = nodes[i].offset + j;
            if (covered[pos]) return at("ordered position", pos) + " is covered by two leaves (the second: node " +
                                     std::to_string(i) + ")";
            covered[pos] = 1;
        }
    for (int j = 0; j < n_prims; ++j)
        if (!covered[j]) return at("ordered position", j) + " is covered by no leaf";
    if (n_nodes != 2 * n_leaves - 1)
        return "node count " + std::to_string(n_nodes) + " is not 2 * leaves - 1 (" + std::to_string(n_leaves) +
               " leaves)";
    // depth-first order: the first child at i + 1, the second where the first child's subtree ends.  pending = the
    // interior nodes whose second child has not been reached, innermost last
    std::vector<int> pending;
    int parent = -1, depth = 0;
    for (int i = 0; i < n_nodes; ++i) {
        const nnbvh_linear_node &n = nodes[i];
        if (i > 0) {
            if (parent < 0) {  // the node before was a leaf: i is the second child of the innermost pending node
                if (pending.empty()) return at("node", i) + " lies after the end of the root's subtree";
                parent = pending.back();
                pending.pop_back();
                if (nodes[parent].offset != i)
                    return at("node", parent) + ": second-child offset " + std::to_string(nodes[parent].offset) +
                           " is not where its first child's subtree ends (" + std::to_string(i) + ")";
            }
            const nnbvh_linear_node &up = nodes[parent];
            for (int k = 0; k < 3; ++k)
                if (!(n.pmin[k] >= up.pmin[k] && n.pmax[k] <= up.pmax[k]))
                    return at("node", i) + ": box not inside the box of its parent, node " + std::to_string(parent);
        }
        if (n.nprims == 0) {
            pending.push_back(i);
            parent = i;
        } else {
            for (int j = 0; j < (int)n.nprims; ++j)
                for (int c = 0; c < 3; ++c)
                    if (!inside(verts + 3 * (size_t)prims[n.offset + j].v[c], n))
                        return at("ordered primitive", n.offset + j) + ": vertex " + std::to_string(c) +
                               " outside the box of its leaf, node " + std::to_string(i);
            parent = -1;
        }
    }
    if (!pending.empty()) return at("node", pending.back()) + ": its second child is never reached";
    // depth in edges from the root (parents precede their children in depth-first order)
    std::vector<int> level((size_t)n_nodes, 0);
    for (int i = 0; i < n_nodes; ++i) {
        if (nodes[i].nprims != 0) {
            depth = std::max(depth, level[i]);
            continue;
        }
        level[i + 1] = level[nodes[i].offset] = level[i] + 1;
    }
    if (depth > kQualityMaxDepth)
        return "tree depth " + std::to_string(depth) + " over " + std::to_string(kQualityMaxDepth);
    shape->n_leaves = n_leaves;
    shape->n_inner = n_nodes - n_leaves;
    shape->depth = depth;
    return "";
}

struct DeviceArrays {
    std::vector<void *> ptrs;
    bool ok = true;
    template <class T>
    T *get(size_t count, const char *what) {
        void *d = nullptr;
        if (!ok) return nullptr;
        ok = hip_ok(hipMalloc(&d, std::max<size_t>(count * sizeof(T), 16)), (std::string("hipMalloc(") + what + ")").c_str());
        if (ok) ptrs.push_back(d);
        return (T *)d;
    }
    ~DeviceArrays() {
        for (void *p : ptrs) (void)hipFree(p);
    }
};

struct StreamAndEvents {
    hipStream_t stream = nullptr;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool create() {
        if (!hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate")) return false;
        for (auto &e : ev)
            if (!hip_ok(hipEventCreate(&e), "hipEventCreate")) return false;
        return true;
    }
    ~StreamAndEvents() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

extern "C" int nnbvh_tree_quality_create(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *ordered_prims,
                                         int n_prims, const float *verts, int n_verts, double c_inner, double c_leaf,
                                         int device, nnbvh_tree_quality *out, int32_t *prim_ext_inner,
                                         int32_t *prim_ext_leaf, int32_t *node_external) {
    if (!nodes || n_nodes <= 0 || !ordered_prims || n_prims <= 0 || !verts || n_verts <= 0 || !out) {
        set_error(std::string(kFn) + "null or empty array (nodes, ordered_prims, verts and out are required)");
        return NNBVH_ERR_ARG;
    }
    if (!std::isfinite(c_inner) || !std::isfinite(c_leaf)) {
        set_error(std::string(kFn) + "c_inner and c_leaf must be finite");
        return NNBVH_ERR_ARG;
    }
    TreeShape shape;
    const std::string fault = tree_fault(nodes, n_nodes, ordered_prims, n_prims, verts, n_verts, &shape);
    if (!fault.empty()) {
        set_error(std::string(kFn) + fault);
        return NNBVH_ERR_ARG;
    }
    const int n_dev = nnbvh_device_count();
    if (n_dev <= 0 || device < 0 || device >= n_dev) {
        set_error(std::string(kFn) + "no usable HIP device (this library has no CPU fallback)");
        return NNBVH_ERR_DEVICE;
    }
    DeviceGuard guard(device);
    if (!guard.ok) return NNBVH_ERR_DEVICE;
    StreamAndEvents se;
    if (!se.create()) return NNBVH_ERR_DEVICE;
    DeviceArrays mem;
    auto *d_nodes = mem.get<nnbvh_linear_node>((size_t)n_nodes, "nodes");
    auto *d_prims = mem.get<nnbvh_prim>((size_t)n_prims, "ordered_prims");
    auto *d_verts = mem.get<float>(3 * (size_t)n_verts, "verts");
    QualityBuffers b;
    b.n_nodes = n_nodes;
    b.n_prims = n_prims;
    b.rec = mem.get<float4>(2 * (size_t)n_nodes, "records");
    b.leaf_of = mem.get<int32_t>((size_t)n_prims, "leaf_of");
    b.k_inner = mem.get<int32_t>((size_t)n_prims, "k_inner");
    b.k_leaf = mem.get<int32_t>((size_t)n_prims, "k_leaf");
    b.node_external = mem.get<int32_t>((size_t)n_nodes, "node_external");
    b.partials = mem.get<double>(5 * (size_t)quality_blocks(std::max(n_nodes, n_prims)), "partials");
    b.ipartials = mem.get<long long>(2 * (size_t)quality_blocks(n_prims), "pair partials");
    b.sums = mem.get<double>(5, "sums");
    b.isums = mem.get<long long>(2, "pair sums");
    if (!mem.ok) return NNBVH_ERR_DEVICE;
    b.nodes = d_nodes;
    b.prims = d_prims;
    b.verts = d_verts;
    hipStream_t st = se.stream;
    double sums[5];
    long long isums[2];
    const bool ran =
        hip_ok(hipEventRecord(se.ev[0], st), "hipEventRecord") &&
        hip_ok(hipMemcpyAsync(d_nodes, nodes, (size_t)n_nodes * sizeof(nnbvh_linear_node), hipMemcpyHostToDevice, st), "copy nodes") &&
        hip_ok(hipMemcpyAsync(d_prims, ordered_prims, (size_t)n_prims * sizeof(nnbvh_prim), hipMemcpyHostToDevice, st), "copy ordered_prims") &&
        hip_ok(hipMemcpyAsync(d_verts, verts, 3 * (size_t)n_verts * sizeof(float), hipMemcpyHostToDevice, st), "copy verts") &&
        hip_ok(hipEventRecord(se.ev[1], st), "hipEventRecord") &&
        hip_ok(launch_quality_prepare(b, st), "tree-quality prepare") &&
        hip_ok(hipEventRecord(se.ev[2], st), "hipEventRecord") &&
        hip_ok(launch_quality_walk(b, st), "tree-quality walk") &&
        hip_ok(hipEventRecord(se.ev[3], st), "hipEventRecord") &&
        hip_ok(launch_quality_reduce(b, st), "tree-quality reduce") &&
        hip_ok(hipEventRecord(se.ev[4], st), "hipEventRecord") &&
        hip_ok(hipMemcpyAsync(sums, b.sums, sizeof sums, hipMemcpyDeviceToHost, st), "copy sums") &&
        hip_ok(hipMemcpyAsync(isums, b.isums, sizeof isums, hipMemcpyDeviceToHost, st), "copy pair sums") &&
        (!prim_ext_inner || hip_ok(hipMemcpyAsync(prim_ext_inner, b.k_inner, (size_t)n_prims * 4, hipMemcpyDeviceToHost, st), "copy prim_ext_inner")) &&
        (!prim_ext_leaf || hip_ok(hipMemcpyAsync(prim_ext_leaf, b.k_leaf, (size_t)n_prims * 4, hipMemcpyDeviceToHost, st), "copy prim_ext_leaf")) &&
        (!node_external || hip_ok(hipMemcpyAsync(node_external, b.node_external, (size_t)n_nodes * 4, hipMemcpyDeviceToHost, st), "copy node_external"));
    // the stream is drained on every way out: the device arrays are freed behind it
    const bool drained = hip_ok(hipStreamSynchronize(st), "tree-quality passes");
    if (!ran || !drained) return NNBVH_ERR_DEVICE;
    nnbvh_tree_quality q;
    std::memset(&q, 0, sizeof q);
    for (int k = 0; k < 3; ++k)
        if (!hip_ok(hipEventElapsedTime(&q.gpu_ms[k], se.ev[k + 1], se.ev[k + 2]), "hipEventElapsedTime")) return NNBVH_ERR_DEVICE;
    if (!hip_ok(hipEventElapsedTime(&q.gpu_ms[3], se.ev[0], se.ev[4]), "hipEventElapsedTime")) return NNBVH_ERR_DEVICE;
    const nnbvh_linear_node &root = nodes[0];
    const double x = (double)root.pmax[0] - (double)root.pmin[0], y = (double)root.pmax[1] - (double)root.pmin[1],
                 z = (double)root.pmax[2] - (double)root.pmin[2];
    q.inner_area = sums[0];
    q.leaf_area_weighted = sums[1];
    q.root_area = 2.0 * (x * y + x * z + y * z);
    q.prim_area = sums[2];
    q.ext_area_inner = sums[3];
    q.ext_area_leaf = sums[4];
    q.ext_pairs_inner = isums[0];
    q.ext_pairs_leaf = isums[1];
    q.n_inner = shape.n_inner;
    q.n_leaves = shape.n_leaves;
    q.depth = shape.depth;
    // the formulas of nn_loss.py:119-135 / 165-192, literally: a zero area gives the NaN or inf the division gives
    q.sah = (c_inner * q.inner_area + c_leaf * q.leaf_area_weighted) / q.root_area;
    q.epo = (c_inner * q.ext_area_inner + c_leaf * q.ext_area_leaf) / q.prim_area;
    *out = q;
    return NNBVH_OK;
}
