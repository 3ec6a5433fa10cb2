/*
 * nnbvh.h — C ABI of the MI355X-native BVH traversal path (libnnbvh_hip.so).
 *
 * Drop-in boundary for pbrt's BVH hot path.  Each entry point names the reference
 * interface it replaces (paths relative to /root/reference/src/pbrt):
 *
 *   nnbvh_scene_create      <- CreateAccelerator("bvh", prims, ...) / new BVHAggregate(prims)
 *                              (cpu/aggregates.cpp:1163-1178, 140-190): takes the flattened
 *                              LinearBVHNode[] (cpu/aggregates.cpp:129-137), the leaf-ordered
 *                              primitive table (aggregates.cpp:176) and the mesh vertices
 *                              (util/mesh.h:24-72, already in render space, util/mesh.cpp:36-39)
 *   nnbvh_scene_bounds      <- BVHAggregate::Bounds()          (cpu/aggregates.cpp:524-527)
 *   nnbvh_intersect_closest <- BVHAggregate::Intersect()       (cpu/aggregates.cpp:529-579), batched
 *                              like CPUAggregate::IntersectClosest (wavefront/aggregate.cpp:34-58)
 *   nnbvh_intersect_any     <- BVHAggregate::IntersectP()      (cpu/aggregates.cpp:581-624), batched
 *                              like CPUAggregate::IntersectShadow  (wavefront/aggregate.cpp:60-68)
 *   nnbvh_wavefront_*       <- WavefrontAggregate::IntersectClosest / IntersectShadow incl. the
 *                              queue push rules (wavefront/integrator.h:32-54, intersect.h:16-156)
 *   nnbvh_triangle_interactions_device <- Triangle::InteractionFromIntersection (shapes.h:884-1010)
 *   nnbvh_build_*           <- BVHAggregate ctor + buildRecursive + flattenBVH
 *                              (cpu/aggregates.cpp:140-387, 505-522); host-side, no GPU needed
 *
 * Conventions: plain C, caller-owned buffers, no C++/torch types.  Every function that
 * can fail returns an int status (0 = NNBVH_OK) or NULL and records a message readable
 * with nnbvh_last_error() (thread-local); nothing here aborts the host process (the
 * reference's CHECK/LOG_FATAL would, util/check.h:36-57).  All entry points are
 * thread-safe; results of a call depend only on that call's inputs.  There is NO CPU
 * fallback: without a usable HIP device the intersect calls fail with NNBVH_ERR_DEVICE.
 */
#ifndef NNBVH_H
#define NNBVH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NNBVH_OK 0
#define NNBVH_ERR_ARG 1     /* bad pointer / size / malformed tree */
#define NNBVH_ERR_DEVICE 2  /* no HIP device, allocation or launch failure */
#define NNBVH_ERR_DEPTH 3   /* tree deeper than the supported traversal stack */

/* == LinearBVHNode (cpu/aggregates.cpp:129-137): 32 B, 32-B aligned in the reference */
typedef struct nnbvh_linear_node {
    float pmin[3];
    float pmax[3];
    int32_t offset;   /* leaf: primitivesOffset; interior: secondChildOffset */
    uint16_t nprims;  /* 0 -> interior node */
    uint8_t axis;     /* interior: split axis 0/1/2 */
    uint8_t pad;
} nnbvh_linear_node;

#define NNBVH_PRIM_TRIANGLE 0       /* Triangle      (shapes.h:833-1192) */
#define NNBVH_PRIM_BILINEAR_PATCH 1 /* BilinearPatch (shapes.h:1350-1539): v = p00,p10,p01,p11 */
#define NNBVH_PRIM_HOST 3           /* a primitive only the host can intersect (Sphere, Disk, Cylinder,
                                       Curve, alpha-tested GeometricPrimitive: shapes.h, cpu/
                                       primitive.cpp:57-84): carries bounds only.  A ray that
                                       reaches one gets hit.instance = -1 (closest) or
                                       occluded = 2 unless a GPU primitive already occludes it
                                       (any): the caller re-traces exactly those rays on the CPU */
#define NNBVH_PRIM_INSTANCE 2       /* TransformedPrimitive (cpu/primitive.h:83-101): v[0] = index
                                       into the instance table; top-level tree only */

#define NNBVH_PRIM_ALPHA_TRIANGLE 4  /* a Triangle inside a GeometricPrimitive whose alpha texture is a
                                       constant (cpu/primitive.cpp:57-70, FloatConstantTexture): v[3] =
                                       the bit pattern of the float alpha.  A hit is ignored when
                                       HashFloat(r.o, r.d) > alpha (always when alpha <= 0); the reference
                                       then re-traces from the hit point against the same shape, which a
                                       planar triangle cannot be hit by again (shapes_test.cpp:156-206) —
                                       the device performs that re-test too and, should it ever hit, voids
                                       the ray like a host-only primitive (instance = -1 / occluded = 2).
                                       For meshes WITHOUT per-vertex shading normals (the offset normal
                                       is the geometric one); meshes with normals: kinds 6 / 7; an alpha that
                                       is an image texture: kinds 16 .. 19 */
#define NNBVH_PRIM_ALPHA_TRIANGLE_FLIPPED 5 /* same, mesh->reverseOrientation ^ transformSwapsHandedness */
#define NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH 6  /* ... of a mesh WITH per-vertex shading normals: the ray re-traced
                                       after a rejected hit is offset along FaceForward(n, ns) (shapes.h:
                                       939-951, interaction.h:194-200); needs the scene's vertex normals
                                       (nnbvh_scene_create_with_normals; kd-trees:
                                       nnbvh_kd_scene_create_with_attributes) */
#define NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH_FLIPPED 7
#define NNBVH_PRIM_ALPHA_PATCH 8   /* BilinearPatch behind a GeometricPrimitive with a CONSTANT alpha (v[0..3] are the
                                       patch's vertices: the alpha comes from the per-primitive array of
                                       nnbvh_scene_create_with_attributes).  A non-planar patch can be met again by the
                                       ray re-traced off its own surface; the recursion of cpu/primitive.cpp:63-69 is
                                       followed for up to three re-traces, beyond which the record is void
                                       (needs-host).  For patch meshes WITHOUT (u, v) coordinates (with them: kinds
                                       12 .. 15) */
#define NNBVH_PRIM_ALPHA_PATCH_FLIPPED 9         /* same, mesh->reverseOrientation ^ transformSwapsHandedness */
#define NNBVH_PRIM_ALPHA_PATCH_SMOOTH 10         /* ... of a mesh WITH per-vertex normals (BilinearPatchMesh::n as
                                                     the mesh stores them, util/mesh.cpp:216-223) */
#define NNBVH_PRIM_ALPHA_PATCH_SMOOTH_FLIPPED 11
#define NNBVH_PRIM_ALPHA_PATCH_UV 12               /* 8 .. 11 for a mesh WITH (u, v) coordinates (BilinearPatchMesh::uv): the
                                                      interaction's normal is then Normalize(Cross(dpds, dpdt)) of the
                                                      (s, t) reparametrisation, shapes.h:1414-1437; needs the scene's
                                                      per-vertex uvs.  kind = 8 + flipped + 2 * smooth + 4 * uv */
#define NNBVH_PRIM_ALPHA_PATCH_UV_FLIPPED 13
#define NNBVH_PRIM_ALPHA_PATCH_UV_SMOOTH 14
#define NNBVH_PRIM_ALPHA_PATCH_UV_SMOOTH_FLIPPED 15
#define NNBVH_PRIM_ALPHATEX_TRIANGLE 16 /* a Triangle inside a GeometricPrimitive whose alpha is a FloatImageTexture with a
                                       UVMapping (textures.h:579-590): v[3] = index into the scene's alpha-texture table
                                       (nnbvh_scene_create_with_alpha_textures; two-level scenes:
                                       nnbvh_scene_create_instanced_with_alpha_textures; kd-trees:
                                       nnbvh_kd_scene_create_with_alpha_textures).  The texture is evaluated at the hit's
                                       (u, v) as the reference does for the alpha test, i.e. with zero differentials:
                                       level 0 of the image only (nnbvh_alpha_texture).  Then as kind 4.
                                       kind = 16 + flipped + 2 * smooth, flipped and smooth as for kinds 4 .. 7.
                                       BVH scenes of one or two levels and kd scenes: textured alpha on patches, other
                                       mappings (spherical, cylindrical, planar) and other float textures (scale, mix,
                                       checkerboard, ...) stay NNBVH_PRIM_HOST */
#define NNBVH_PRIM_ALPHATEX_TRIANGLE_FLIPPED 17
#define NNBVH_PRIM_ALPHATEX_TRIANGLE_SMOOTH 18
#define NNBVH_PRIM_ALPHATEX_TRIANGLE_SMOOTH_FLIPPED 19

/* One entry of BVHAggregate::primitives: the shape handle flattened to global vertex
 * indices (Triangle{meshIndex,triIndex} -> mesh->vertexIndices[3*tri..], shapes.cpp:326-328). */
typedef struct nnbvh_prim {
    int32_t kind;
    int32_t id;   /* caller's primitive id, returned in nnbvh_hit.prim */
    int32_t v[4]; /* indices into the vertex array; v[3] unused for triangles */
} nnbvh_prim;

/* Ray + tMax (ray.h:18-39 Ray{o,d,time,medium} and the tMax argument), 32 B.
 * d need NOT be normalised (shadow rays are not, cpu/integrators.h:52-54). */
typedef struct nnbvh_ray {
    float o[3];
    float tmax;
    float d[3];
    float time;
} nnbvh_ray;

/* What TriangleIntersection / BilinearIntersection carry (shapes.h:820-824, 1271-1275)
 * plus the reference's observables bvhNodesVisited (aggregates.cpp:27) and nTriTests
 * (shapes.cpp:148), per ray.  32 B. */
typedef struct nnbvh_hit {
    int32_t prim; /* -1 = miss */
    float t;      /* tHit; on a miss: the ray's tmax */
    float b0, b1, b2; /* triangle barycentrics; patch: b0 = u, b1 = v, b2 = 0 */
    int32_t nodes_visited;
    int32_t prim_tests;
    int32_t instance; /* -1: the ray reached a host-only primitive: record void, re-trace on the CPU
                         (or use nnbvh_intersect_closest_candidates, which lists those primitives);
                         0: hit in the top-level tree (or miss); k + 1: inside instance k, and
                         then `prim` is the child tree's primitive id and t, b* are those of the
                         instance-space ray, exactly what TransformedPrimitive::Intersect returns */
} nnbvh_hit;

/* A TransformedPrimitive: a child BVHAggregate (an object instance, scene.cpp:1521-1577) behind
 * a static transform.  Matrices are the first three rows of pbrt's 4x4 Transform::m / mInv
 * (row-major; the fourth row of an affine transform is 0 0 0 1).  The child tree occupies
 * nodes[root, root + n_nodes) of the scene's node array, in the same DFS layout; its leaves
 * index the scene's primitive table.  Several instances may share one child tree. */
typedef struct nnbvh_instance {
    float render_from_prim[12];
    float prim_from_render[12];
    int32_t root;
    int32_t n_nodes;
} nnbvh_instance;

/* A placement of an object definition, for scenes whose trees are built on the device
 * (nnbvh_scene_create_instanced_gpu_build): the matrices as in nnbvh_instance, and which object it places. */
typedef struct nnbvh_placement {
    float render_from_prim[12];
    float prim_from_render[12];
    int32_t object; /* index of the object definition */
    int32_t pad;
} nnbvh_placement;

typedef struct nnbvh_scene nnbvh_scene;
typedef struct nnbvh_build nnbvh_build;

const char *nnbvh_last_error(void);
int nnbvh_device_count(void);

/* ---- host-side tree construction (no GPU) ---------------------------------------- */
#define NNBVH_SPLIT_SAH 0
#define NNBVH_SPLIT_HLBVH 1
#define NNBVH_SPLIT_MIDDLE 2
#define NNBVH_SPLIT_EQUAL_COUNTS 3
nnbvh_build *nnbvh_build_create(const nnbvh_prim *prims, int n_prims, const float *verts,
                                int n_verts, int max_prims_in_node, int split_method);
/* same, for a primitive list that contains NNBVH_PRIM_INSTANCE / NNBVH_PRIM_HOST entries:
 * prim_bounds holds 6 floats (min, max) per primitive and is read for those entries */
nnbvh_build *nnbvh_build_create_with_bounds(const nnbvh_prim *prims, int n_prims,
                                            const float *verts, int n_verts,
                                            const float *prim_bounds, int max_prims_in_node,
                                            int split_method);
/* Tree construction on the GPU (`device`), split_method NNBVH_SPLIT_SAH or NNBVH_SPLIT_HLBVH; the
 * result (nodes, leaf-ordered primitives, depth) is byte-identical to
 * nnbvh_build_create_with_bounds(..., split_method), i.e. to the reference's tree.
 *   SAH   (buildRecursive, aggregates.cpp:192-387): nodes above 256 primitives breadth-first with
 *         whole-grid kernels, every smaller subtree by one wavefront; std::partition's exact
 *         element order is reproduced from ballots / prefix sums.
 *   HLBVH (buildHLBVH, aggregates.cpp:389-503 with treelets emitted in Morton order): Morton codes,
 *         radix sort, the treelets' radix trees, bounds and the DFS layout on the device, and
 *         buildUpperSAH over the <= 4096 treelet roots (aggregates.cpp:626-723) there too: ranges above
 *         64 treelets in passes over the grid, every smaller one by one wavefront.
 * On neither builder does tree data cross to the host before the finished tree is read back.
 * NULL + nnbvh_last_error() on failure (no device, allocation, malformed input). */
nnbvh_build *nnbvh_build_create_gpu(const nnbvh_prim *prims, int n_prims, const float *verts,
                                    int n_verts, const float *prim_bounds, int max_prims_in_node,
                                    int split_method, int device);
/* milliseconds of the last GPU build's phases (all zero for host builds) — HLBVH: upload, device
 * sort + tree, device upper SAH, device emit, download; SAH: upload, big nodes breadth-first,
 * wavefront subtrees, layout + bounds, download */
int nnbvh_build_gpu_timing(const nnbvh_build *b, double out_ms[5]);
const nnbvh_linear_node *nnbvh_build_nodes(const nnbvh_build *b, int *n_nodes);
const nnbvh_prim *nnbvh_build_ordered_prims(const nnbvh_build *b, int *n_prims);
int nnbvh_build_depth(const nnbvh_build *b); /* edges root -> deepest leaf */
void nnbvh_build_destroy(nnbvh_build *b);

/* The SAH trees of many objects in ONE pass on the GPU: what nnbvh_build_create_gpu(..., NNBVH_SPLIT_SAH, ...) makes
 * of each object alone, tree k byte for byte (its second-child offsets count from its own root, its leaves' first
 * primitives from the object's first primitive), without the per-build launches, read-backs and synchronisations
 * that dominate when the objects are small and many.
 *   prims[n_prims]             the objects' primitives one after another (triangles, bilinear patches, the alpha
 *                              kinds, NNBVH_PRIM_HOST; no NNBVH_PRIM_INSTANCE entries), over ONE vertex array
 *   object_first[n_objects+1]  object k is prims[object_first[k], object_first[k+1]); object_first[0] == 0, the last
 *                              entry == n_prims, no object is empty
 *   prim_bounds                nullable, 6 floats per entry of prims, read for NNBVH_PRIM_HOST entries
 *   split_method               NNBVH_SPLIT_SAH (anything else is refused: this call is SAH only; HLBVH forests are
 *                              nnbvh_build_forest_create_gpu_hlbvh's, below)
 * NULL + nnbvh_last_error() for every argument fault (null or empty arrays, a malformed object_first, vertex indices,
 * unknown kinds, instance entries, host-only primitives without prim_bounds, the split method: all checked on the
 * host before a device is looked at), for no usable device, and for malformed geometry, where the message is the one
 * a loop of single builds over the objects would have stopped at: the lowest-numbered failing object's.
 * Accessors: the node array [tree 0, tree 1, ...]; node_first[n_objects + 1] (tree k is nodes[node_first[k],
 * node_first[k + 1])); depths[n_objects]; the leaf-ordered primitives, object k's at object_first[k]; timing = the
 * phases of nnbvh_build_gpu_timing's SAH; n_levels = breadth-first passes run (each covers every object's nodes above
 * 256 primitives of one level; 0 when no object is that large); n_subtrees = subtrees built by one wavefront each. */
typedef struct nnbvh_forest nnbvh_forest;
nnbvh_forest *nnbvh_build_forest_create_gpu(const nnbvh_prim *prims, int n_prims, const int32_t *object_first,
                                            int n_objects, const float *verts, int n_verts, const float *prim_bounds,
                                            int max_prims_in_node, int split_method, int device);
const nnbvh_linear_node *nnbvh_forest_nodes(const nnbvh_forest *f, int *n_nodes);
const int32_t *nnbvh_forest_node_first(const nnbvh_forest *f, int *n_objects);
const int32_t *nnbvh_forest_depths(const nnbvh_forest *f, int *n_objects);
const nnbvh_prim *nnbvh_forest_ordered_prims(const nnbvh_forest *f, int *n_prims);
int nnbvh_forest_gpu_timing(const nnbvh_forest *f, double out_ms[5]);
int nnbvh_forest_n_levels(const nnbvh_forest *f);
int nnbvh_forest_n_subtrees(const nnbvh_forest *f);
void nnbvh_forest_destroy(nnbvh_forest *f);
/* The same for HLBVH trees: tree k is byte for byte what nnbvh_build_create_gpu(..., NNBVH_SPLIT_HLBVH, ...) makes of
 * object k alone, from a fixed number of launches and synchronisations however many objects there are.  Arguments,
 * argument faults (the same, less the split method), the handle, its accessors and its ownership are
 * nnbvh_build_forest_create_gpu's.  Of the accessors, timing = the phases of nnbvh_build_gpu_timing's HLBVH (upload;
 * device sort + treelets of every object; the upper SAH of every object, on the device; device emit; download),
 * n_levels = 0 (HLBVH has no breadth-first passes) and n_subtrees = treelets in the forest (primitives of one object
 * that share the top 12 bits of their Morton code; at most 4096 per object, no bound on the total).  No treelet
 * table, layout or upper node crosses to the host. */
nnbvh_forest *nnbvh_build_forest_create_gpu_hlbvh(const nnbvh_prim *prims, int n_prims, const int32_t *object_first,
                                                  int n_objects, const float *verts, int n_verts,
                                                  const float *prim_bounds, int max_prims_in_node, int device);
/* What the builders' upper levels came to.  n_upper: HLBVH, the upper nodes (buildUpperSAH's: an object's treelets
 * less one, so the forest's treelets less its objects); SAH, the nodes built breadth-first.  n_upper_passes: launches
 * of the HLBVH upper build's pass kernel, each of which works on every open range of every object: 0 for SAH and
 * when no object has two treelets, 1 when no object has more than 64, more for larger objects (a range above 64
 * treelets is split once per pass).  The nnbvh_build_ forms report the same of a single GPU build (0 for host builds). */
int nnbvh_forest_n_upper_passes(const nnbvh_forest *f);
int nnbvh_forest_n_upper(const nnbvh_forest *f);
int nnbvh_build_n_upper(const nnbvh_build *b);
int nnbvh_build_n_upper_passes(const nnbvh_build *b);

/* ---- device scene ------------------------------------------------------------------ */
/* Uploads and bakes a flattened tree (the reference's LinearBVHNode[] in its DFS layout, first child
 * at index + 1) with its leaf-ordered primitives.  Everything the kernels index with is validated
 * here: a malformed tree is NULL + nnbvh_last_error(), never a device fault.  Node bounds must be
 * Bounds3f with pmin <= pmax on every axis and no NaN (what every builder emits; the kernels' form of
 * the slab test is equal to Bounds3::IntersectP, util/vecmath.h:1573-1608, for such boxes). */
nnbvh_scene *nnbvh_scene_create(const nnbvh_linear_node *nodes, int n_nodes,
                                const nnbvh_prim *ordered_prims, int n_prims,
                                const float *verts, int n_verts, int device);
/* two-level scene: nodes[0, n_top_nodes) is the top-level tree (may contain NNBVH_PRIM_INSTANCE
 * leaves), the rest are child trees named by `instances`.  Replaces the TransformedPrimitive
 * path of cpu/primitive.cpp:112-131 (AnimatedPrimitive is not covered). */
nnbvh_scene *nnbvh_scene_create_instanced(const nnbvh_linear_node *nodes, int n_nodes,
                                          int n_top_nodes, const nnbvh_prim *ordered_prims,
                                          int n_prims, const float *verts, int n_verts,
                                          const nnbvh_instance *instances, int n_instances,
                                          int device);
/* AnimatedPrimitive (cpu/primitive.h:103-118; cpu/primitive.cpp:133-158): an instance whose
 * render-from-instance transform is an AnimatedTransform.  The struct carries the members the
 * reference object holds after construction (util/transform.h:443-520: start / end transform, the
 * decomposition T, R, S of util/transform.cpp:375-394 and the time range); per ray the device evaluates
 * AnimatedTransform::Interpolate(ray.time) (util/transform.cpp:1062-1081) and applies its inverse as
 * for a static instance.  Arithmetic is the reference's operation for operation except the two sines of
 * Slerp, which the device evaluates in fp64 and rounds (libm's sinf differs from the correctly rounded
 * value on about one input in 10^5): the traversal path's one documented tolerance exception.
 * Bounds of such a primitive (AnimatedTransform::MotionBounds) come from the caller via prim_bounds,
 * like every instance's.  Hits inside animated instances get NNBVH_INTERACTION_HOST from the
 * interaction post-pass. */
typedef struct nnbvh_animated_transform {
    float start_from[16], start_inv[16]; /* startTransform m / mInv, row-major 4x4 */
    float end_from[16], end_inv[16];
    float T[2][3];
    float R[2][4];                       /* quaternion v.x v.y v.z w */
    float S[2][16];
    float start_time, end_time;
    int32_t actually_animated;           /* 0: a TransformedPrimitive (the nnbvh_instance matrices are used) */
    int32_t pad;
} nnbvh_animated_transform;
/* as nnbvh_scene_create_instanced; animated[k] (nullable array) belongs to instances[k] */
nnbvh_scene *nnbvh_scene_create_instanced_animated(const nnbvh_linear_node *nodes, int n_nodes,
                                                   int n_top_nodes, const nnbvh_prim *ordered_prims,
                                                   int n_prims, const float *verts, int n_verts,
                                                   const nnbvh_instance *instances, int n_instances,
                                                   const nnbvh_animated_transform *animated, int device);
/* ... and with the attributes the alpha-tested kinds read (nnbvh_scene_create_with_attributes): normals and uvs per
 * vertex, prim_alpha per entry of `prims`; animated and each attribute array may be NULL */
nnbvh_scene *nnbvh_scene_create_instanced_with_attributes(const nnbvh_linear_node *nodes, int n_nodes, int n_top_nodes,
                                                          const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const nnbvh_instance *instances, int n_instances,
                                                          const nnbvh_animated_transform *animated, const float *normals,
                                                          const float *uvs, const float *prim_alpha, int device);
/* Transform::operator()(const Bounds3f&) (util/transform.cpp:134-139): the bounds an instance
 * primitive presents to the top-level builder (TransformedPrimitive::Bounds, primitive.h:94) */
void nnbvh_transform_bounds(const float render_from_prim[12], const float in_min_max[6],
                            float out_min_max[6]);
/* Triangles in, traceable scene out, entirely on the device: the tree is built there
 * (nnbvh_build_create_gpu's builders), baked there into the traversal layout, and never visits the
 * host.  Same tree and same traversal results as nnbvh_build_create_with_bounds(...,
 * split_method) + nnbvh_scene_create.  split_method NNBVH_SPLIT_SAH or NNBVH_SPLIT_HLBVH;
 * triangles, bilinear patches and host-only primitives (instances: nnbvh_scene_create_instanced_gpu_build below,
 * or nnbvh_scene_create_instanced with host-built trees). */
nnbvh_scene *nnbvh_scene_create_gpu_build(const nnbvh_prim *prims, int n_prims, const float *verts,
                                          int n_verts, const float *prim_bounds,
                                          int max_prims_in_node, int split_method, int device);
/* ... with the attributes the alpha-tested kinds read (see nnbvh_scene_create_with_attributes below): normals and
 * uvs per vertex, prim_alpha per entry of `prims` (the CALLER's order: it is carried through the build); each may be NULL */
nnbvh_scene *nnbvh_scene_create_gpu_build_with_attributes(const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const float *prim_bounds, const float *normals,
                                                          const float *uvs, const float *prim_alpha,
                                                          int max_prims_in_node, int split_method, int device);
/* A two-level scene (object instances, scene.cpp:1521-1577: one BVHAggregate per object definition, one
 * TransformedPrimitive / AnimatedPrimitive per placement) entirely on the device: every object's tree, then the
 * top-level tree, are built there, put into one numbering and baked; no tree visits the host, and with either split
 * method no part of one does (HLBVH's upper levels over the treelets are built on the device too).  The device arrays are
 * byte for byte those of nnbvh_scene_create_instanced_with_attributes on host-built trees of the same split_method
 * (nodes [top, object 0, object 1, ...], primitives [top in leaf order, object 0 in leaf order, ...]).  All object
 * trees come from one forest pass (the builder of nnbvh_build_forest_create_gpu for NNBVH_SPLIT_SAH, of
 * nnbvh_build_forest_create_gpu_hlbvh for NNBVH_SPLIT_HLBVH), so a scene of thousands of small objects pays the
 * builder's launches and read-backs once; the top-level tree is a single build.
 *   prims[n_prims]            the caller's order: [0, n_top_prims) is the top-level list (triangles, patches, the
 *                             alpha kinds, NNBVH_PRIM_HOST and NNBVH_PRIM_INSTANCE entries; for an instance entry
 *                             v[0] is the placement index and id the caller's), then the object definitions one
 *                             after another (no instance entries: nested instances are not supported)
 *   object_first[n_objects+1] object k is prims[object_first[k], object_first[k+1]); object_first[0] == n_top_prims,
 *                             the last entry == n_prims, no object is empty.  Every object is built and baked, named
 *                             by a placement or not
 *   normals, uvs, prim_alpha  nullable, as nnbvh_scene_create_gpu_build_with_attributes (prim_alpha per entry of
 *                             prims in the CALLER's order)
 *   prim_bounds               nullable, 6 floats per entry of prims: read for NNBVH_PRIM_HOST entries and for instance
 *                             entries whose placement is actually_animated (AnimatedTransform::MotionBounds stays the
 *                             caller's).  A static instance's bounds (Transform::operator()(Bounds3f) of the child's
 *                             root box, nnbvh_transform_bounds bit for bit) are computed on the device and the
 *                             caller's values are ignored
 *   placements[n_placements]  at least one; animated[n_placements] nullable
 *   split_method              NNBVH_SPLIT_SAH or NNBVH_SPLIT_HLBVH
 * NULL + nnbvh_last_error() for every argument fault (null or empty arrays, a malformed object_first, a placement's
 * object or an instance entry's v[0] out of range, an instance entry inside an object, vertex indices, a missing
 * prim_bounds or attribute array, an animated placement with an empty time range, a bad split method: all checked
 * on the host before a device is looked at), for no usable device, for non-finite vertices, and for a scene deeper
 * (top depth + deepest child + 1) than the 64-entry traversal stack. */
nnbvh_scene *nnbvh_scene_create_instanced_gpu_build(const nnbvh_prim *prims, int n_prims, int n_top_prims,
                                                    const int32_t *object_first, int n_objects, const float *verts,
                                                    int n_verts, const float *normals, const float *uvs,
                                                    const float *prim_alpha, const float *prim_bounds,
                                                    const nnbvh_placement *placements, int n_placements,
                                                    const nnbvh_animated_transform *animated, int max_prims_in_node,
                                                    int split_method, int device);
/* nnbvh_scene_create with the meshes' per-vertex shading normals (3 floats per vertex, indexed like `verts`;
 * TriangleMesh::n, util/mesh.h:48): read for NNBVH_PRIM_ALPHA_TRIANGLE_SMOOTH[_FLIPPED] primitives only, whose
 * three normals are baked into the primitive stream.  normals = NULL is nnbvh_scene_create. */
nnbvh_scene *nnbvh_scene_create_with_normals(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                             int n_prims, const float *verts, const float *normals, int n_verts,
                                             int device);
/* ... and with the (u, v) coordinates per vertex (2 floats, read for the NNBVH_PRIM_ALPHA_PATCH_UV* primitives) and a
 * per-primitive constant alpha (n_prims floats, indexed like `prims`): read for the NNBVH_PRIM_ALPHA_PATCH*
 * primitives only (alpha-tested triangles keep theirs in v[3]).  Any of the three arrays may be NULL when no
 * primitive needs it. */
nnbvh_scene *nnbvh_scene_create_with_attributes(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                                int n_prims, const float *verts, const float *normals,
                                                const float *uvs, const float *prim_alpha, int n_verts, int device);
/* ---- image-textured alpha (kinds NNBVH_PRIM_ALPHATEX_TRIANGLE*) --------------------------------------------------
 * One FloatImageTexture as the alpha test sees it.  GeometricPrimitive::Intersect (cpu/primitive.cpp:57-58) evaluates
 * the texture on the interaction the shape has just made, whose screen-space differentials are still zero, so
 * MIPMap::Filter (util/mipmap.cpp:229-284) never leaves level 0: bilinear, trilinear and EWA filtering all return
 * Bilerp(0, st), the point filter one level-0 texel.  No MIP pyramid is needed.  Decoding 8-bit or half texels through
 * the image's colour encoding is the embedder's (one Image::GetChannel per texel at scene creation). */
#define NNBVH_WRAP_REPEAT 0 /* WrapMode::Repeat */
#define NNBVH_WRAP_CLAMP 1  /* WrapMode::Clamp */
#define NNBVH_WRAP_BLACK 2  /* WrapMode::Black (WrapMode::OctahedralSphere is refused) */
typedef struct nnbvh_alpha_texture {
    const float *texels;   /* level 0 only: width*height floats, row-major, row 0 = the image's first row; each the
                              value Image::GetChannel(p, 0) returns, i.e. already decoded to linear.  Copied */
    int32_t width, height; /* 1 .. 2^24 */
    int32_t wrap;          /* NNBVH_WRAP_REPEAT / _CLAMP / _BLACK */
    int32_t point_filter;  /* 1 = FilterFunction::Point; 0 = bilinear, trilinear, EWA (all Bilerp(0, st) here) */
    float su, sv, du, dv;  /* UVMapping (textures.h:85-106) */
    float scale;
    int32_t invert;
} nnbvh_alpha_texture;
/* nnbvh_scene_create_with_attributes / nnbvh_scene_create_gpu_build_with_attributes plus the alpha-texture table the
 * kinds 16 .. 19 index with v[3].  Both make the same device arrays (nnbvh_scene_read; what = 3: the descriptor table,
 * 48 bytes per texture, 4: the texel pool, 4 bytes per texel).  uvs (2 floats per vertex) gives a textured triangle its
 * three (u, v) pairs; uvs == NULL means the mesh has none and EVERY textured triangle takes the reference's default
 * corners (0,0), (1,0), (1,1) (shapes.h, InteractionFromIntersection) — a scene that mixes textured meshes with and
 * without (u, v) keeps those without NNBVH_PRIM_HOST.  Kinds 4 .. 7 may be mixed in; alpha-tested patches (kinds
 * 8 .. 15) may not (refused).  NULL + nnbvh_last_error() naming the call, before a device is looked at, for: a null or
 * empty texture table with a textured triangle present, a texture index out of range, null texels, a width or height
 * outside 1 .. 2^24, an unknown wrap mode, a smooth kind without normals — besides every fault of the call without
 * textures.  The other creation calls refuse kinds 16 .. 19. */
nnbvh_scene *nnbvh_scene_create_with_alpha_textures(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *prims,
                                                    int n_prims, const float *verts, const float *normals,
                                                    const float *uvs, const float *prim_alpha, int n_verts, int device,
                                                    const nnbvh_alpha_texture *textures, int n_textures);
nnbvh_scene *nnbvh_scene_create_gpu_build_with_alpha_textures(const nnbvh_prim *prims, int n_prims, const float *verts,
                                                              int n_verts, const float *prim_bounds,
                                                              const float *normals, const float *uvs,
                                                              const float *prim_alpha, int max_prims_in_node,
                                                              int split_method, int device,
                                                              const nnbvh_alpha_texture *textures, int n_textures);
/* Two-level scenes: nnbvh_scene_create_instanced_with_attributes (host-built trees) / nnbvh_scene_create_instanced_gpu_build
 * (every tree built on the device) plus the alpha-texture table.  Both make byte-identical device arrays, the table and
 * the pool included (nnbvh_scene_read, what = 3 / 4), and both are counted in the scene's device bytes.  A textured
 * triangle may sit in an object definition or in the top-level list.  Inside an instance the texture is evaluated at
 * the barycentrics of the INSTANCE-space ray, the ray the alpha hash and the re-trace already use there
 * (TransformedPrimitive / AnimatedPrimitive::Intersect hand the transformed ray to the child aggregate,
 * cpu/primitive.cpp:112-131); one object placed twice can so give one triangle two alphas along one render-space line.
 * uvs == NULL, the kinds 4 .. 7 and the argument faults (named after these calls, raised before a device is looked
 * at) are those of the calls above; here alpha-tested patches (kinds 8 .. 15) MAY share the scene with textured
 * triangles.  n_instances must be at least 1.  The other instanced calls refuse kinds 16 .. 19. */
nnbvh_scene *nnbvh_scene_create_instanced_with_alpha_textures(const nnbvh_linear_node *nodes, int n_nodes, int n_top_nodes,
                                                              const nnbvh_prim *prims, int n_prims, const float *verts,
                                                              int n_verts, const nnbvh_instance *instances,
                                                              int n_instances, const nnbvh_animated_transform *animated,
                                                              const float *normals, const float *uvs,
                                                              const float *prim_alpha, int device,
                                                              const nnbvh_alpha_texture *textures, int n_textures);
nnbvh_scene *nnbvh_scene_create_instanced_gpu_build_with_alpha_textures(
    const nnbvh_prim *prims, int n_prims, int n_top_prims, const int32_t *object_first, int n_objects, const float *verts,
    int n_verts, const float *normals, const float *uvs, const float *prim_alpha, const float *prim_bounds,
    const nnbvh_placement *placements, int n_placements, const nnbvh_animated_transform *animated, int max_prims_in_node,
    int split_method, int device, const nnbvh_alpha_texture *textures, int n_textures);
void nnbvh_scene_destroy(nnbvh_scene *s);
int nnbvh_scene_bounds(const nnbvh_scene *s, float out_min_max[6]);
/* what the baked device layout looks like: [0]=interior records, [1]=prim-stream slots,
 * [2]=tree depth, [3]=device bytes, [4]=persistent grid blocks, [5]=LDS stack window */
int nnbvh_scene_info(const nnbvh_scene *s, int64_t out[6]);
/* the baked device arrays of any scene, however it was created, copied to the host (tests, tools): what 0 = interior
 * records (info[0] * 64 bytes), 1 = primitive stream (info[1] * 16 bytes), 2 = animation table (304 bytes per instance;
 * scenes created with one), 3 = alpha-texture descriptor table (48 bytes per texture), 4 = alpha texel pool (scenes
 * created with alpha textures).  Synchronous.  NNBVH_ERR_ARG for a NULL scene or buffer, an unknown `what`, or a `bytes`
 * that is not the array's size. */
int nnbvh_scene_read(const nnbvh_scene *s, int what, void *out, size_t bytes);

/* ---- traversal, host buffers (synchronous; copies in and out) ----------------------
 * What Integrator::Intersect / IntersectP callers (cpu/integrators.cpp:296-313) hand over.  The batch is
 * traced in at most 6 chunks of at least "host_chunk" rays (option; default 2^20) that rotate over three
 * buffer slots, with an upload, a trace and a download stream: one chunk's rays go up while the previous one
 * is traced and the one before comes down.  Buffers
 * the caller has pinned (hipHostMalloc, hipHostRegister, nnbvh_host_register) are read and written by the
 * copy engines directly; pageable buffers go through pinned staging.  Results do not depend on the chunking. */
/* pin a caller buffer (hipHostRegister).  ptr must be PAGE-ALIGNED (4096) and the buffer should own its pages
 * (mmap, aligned_alloc / posix_memalign of whole pages): a registration covers whole pages, and pages shared with
 * other heap objects stay mapped into the GPU's address space on behalf of those neighbours — a later pageable
 * copy the runtime makes for THEM can then fault on the device (seen in round 3: "write access to a read-only
 * page" in an unrelated hipMemcpy after malloc'ed arrays had been registered and freed).  Unregister before the
 * memory is freed.  NNBVH_ERR_ARG for a misaligned pointer. */
int nnbvh_host_register(void *ptr, size_t bytes);
int nnbvh_host_unregister(void *ptr);
int nnbvh_intersect_closest(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits);
/* nodes_visited / prim_tests may be NULL (then the faster non-counting kernel runs) */
int nnbvh_intersect_any(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                        int32_t *nodes_visited, int32_t *prim_tests);

/* ---- traversal, device buffers (asynchronous on `stream`, a hipStream_t; NULL = the
 *      default stream).  Pointers are device pointers on the scene's device. ----------- */
int nnbvh_intersect_closest_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                   void *stream);
int nnbvh_intersect_any_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                               void *d_nodes_visited, void *d_prim_tests, void *stream);

/* ---- host-only primitives as candidates instead of void records -----------------------
 * The plain calls void a ray that reaches an NNBVH_PRIM_HOST primitive (instance == -1 / occluded == 2) and the
 * caller re-traces it through a CPU aggregate of the whole scene.  A host-only primitive never changes the device's
 * tMax, so the device walk of such a ray is the walk that skips it, and its record already holds the closest DEVICE
 * hit.  These calls return that record with its real instance, plus the list of host-only primitives the ray
 * reached, in traversal order; the caller tests those few shapes itself (pbrt: primitives[id].Intersect(ray, tMax))
 * and merges them with the device hit by the rule below.  No CPU BVH is needed.
 *
 * Per ray i, K = capacity:
 *   count[i]     0..K candidates; -1: more than K (record void, instance == -1, as the plain call);
 *                -2: an alpha re-trace voided the ray (record void as the plain call; candidates cannot fix it)
 *   before[i]    closest hit only: how many of the candidates came before the device hit that stands (0 when there
 *                is no device hit, or when every candidate came after it)
 *   prim[i*K+j]  nnbvh_prim.id of candidate j < count[i] (the value nnbvh_hit.prim would carry)
 *   instance[i*K+j]  0 = top-level tree, k + 1 = inside instance k: the caller transforms the render-space ray
 *                into the instance's space itself, as TransformedPrimitive::Intersect does
 * Entries of prim / instance beyond count[i] are left as they were.  A ray that meets no host-only primitive has
 * count 0 and exactly the plain call's record.  With count > 0 the record's nodes_visited and prim_tests count
 * the device walk, not the reference's (which also tests the host shapes: "exact counts" is a follow-up).
 * Any hit: occluded 1 (a device primitive occludes; the list may be partial), 0 (no occluder, no candidate),
 * 2 with count 1..K (the caller tests the candidates with ray.tmax), 2 with count < 0 (void, as the plain call).
 *
 * The merge rule (closest hit) replays the reference's order of acceptance (aggregates.cpp:529-624: a later hit
 * replaces the earlier one and sets tMax = tHit):
 *   1. tMax = ray.tmax;
 *   2. test candidates 0 .. before-1 with the current tMax; each hit replaces the result and sets tMax;
 *   3. the device hit (prim >= 0): if no candidate hit in step 2 it stands unchanged; else it is accepted iff
 *      t <= tMax for a triangle (Triangle::Intersect rejects only tScaled > tMax * det, shapes.cpp:239-242, so an
 *      equal t is accepted) and iff t < tMax for a bilinear patch (IntersectBilinearPatch rejects t >= tMax,
 *      shapes.h:1344).  The record does not carry the kind: the caller looks `prim` up in its primitive table.
 *      The comparison on t stands in for the triangle's test on tScaled: both agree except when t is within an
 *      ulp or two of tMax (e.g. a duplicated triangle; DESIGN.md "Host-only primitives as candidates");
 *   4. test candidates before .. count-1 as in step 2.
 * Any hit: occluded = device occluded || some candidate hits with ray.tmax.
 *
 * Scope: BVH scenes (flat, two-level static and animated, with or without alpha-tested kinds), closest hit and
 * occlusion-only any hit: the single-batch calls below, several batches in one launch
 * (nnbvh_trace_batches_candidates_device) and the wavefront queue entry points (nnbvh_wavefront_*_candidates, after
 * the plain wavefront calls); and kd-tree scenes through the nnbvh_kd_*_candidates calls of the kd section, with one
 * rule of their own: a kd-tree holds a primitive in every leaf its box overlaps, and a host-only primitive is listed
 * once, at the first position in traversal order at which the ray reached it.  Follow-ups, not covered: shape math
 * for spheres / disks / cylinders on the device, exact node / test counts for rays with candidates.
 * NNBVH_ERR_ARG for capacity outside 1..16, a NULL count / prim / instance, or a NULL before on a closest call. */
typedef struct nnbvh_host_candidates {
    int32_t capacity;   /* K, 1..16 (0 = a plain batch, nnbvh_trace_batches_candidates_device only) */
    int32_t *count;     /* int32[n]: 0..K candidates; -1 more than K; -2 alpha re-trace: record void */
    int32_t *before;    /* int32[n], closest only (NULL for any-hit): candidates met before the device hit */
    int32_t *prim;      /* int32[n * K]: nnbvh_prim.id of each candidate, traversal order */
    int32_t *instance;  /* int32[n * K]: 0 = top level, k + 1 = inside instance k */
} nnbvh_host_candidates;

/* device buffers (asynchronous on `stream`; the pointers in `c` are device pointers too) */
int nnbvh_intersect_closest_candidates_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                              const nnbvh_host_candidates *c, void *stream);
int nnbvh_intersect_any_candidates_device(nnbvh_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                          const nnbvh_host_candidates *c, void *stream);
/* host buffers (the pointers in `c` are host pointers): a plain synchronous staged copy, not the three-stream
 * pipeline of nnbvh_intersect_closest */
int nnbvh_intersect_closest_candidates(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits,
                                       const nnbvh_host_candidates *c);
int nnbvh_intersect_any_candidates(nnbvh_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                                   const nnbvh_host_candidates *c);

/* ---- several independent batches at once --------------------------------------------------
 * One call traces n_batches independent ray batches (e.g. the closest-hit queue and the
 * shadow-ray queue of one wavefront iteration: wavefront/integrator.cpp:403-406 and :575-579
 * are independent of each other).  Up to 4 batches of fewer than 2^28 rays each, closest-hit or
 * any-hit without counts, are traced by ONE kernel launch on `stream` (the persistent wavefronts
 * drain the batches one after the other, so the call pays one ramp-up and one drain — the
 * dependent chain of its longest ray — instead of one per batch).  Other
 * combinations run concurrently on internal streams forked from and joined back into `stream`.
 * Either way the call is ONE asynchronous operation on `stream`. */
#define NNBVH_BATCH_CLOSEST 0
#define NNBVH_BATCH_ANY 1
typedef struct nnbvh_batch {
    int32_t kind; /* NNBVH_BATCH_CLOSEST: d_out = nnbvh_hit[n]; NNBVH_BATCH_ANY: d_out = uint8[n] */
    int32_t pad;
    const void *d_rays;    /* nnbvh_ray[n], device */
    int64_t n;
    void *d_out;
    void *d_nodes_visited; /* ANY only, optional int32[n] (exact counts) */
    void *d_prim_tests;    /* ANY only, optional int32[n] */
} nnbvh_batch;
int nnbvh_trace_batches_device(nnbvh_scene *s, const nnbvh_batch *batches, int n_batches,
                               void *stream);
/* ... with host candidates per batch: cands[b] (device pointers) belongs to batches[b] and is filled as by
 * nnbvh_intersect_closest_candidates_device / nnbvh_intersect_any_candidates_device on the same rays; capacity == 0
 * makes batch b a plain batch (its output is nnbvh_trace_batches_device's).  One launch where
 * nnbvh_trace_batches_device uses one; scenes with alpha-tested primitives (and option "fused_batches" 0) run one
 * candidate launch per batch, forked from and joined back into `stream`, with the same results.  NNBVH_ERR_ARG, and
 * nothing launched, for a capacity outside 0..16, a NULL count / prim / instance, a NULL before on a closest batch,
 * or an any-hit batch that asks for exact counts (d_nodes_visited / d_prim_tests) together with candidates. */
int nnbvh_trace_batches_candidates_device(nnbvh_scene *s, const nnbvh_batch *batches, int n_batches,
                                          const nnbvh_host_candidates *cands, void *stream);

/* ---- wavefront queues: WavefrontAggregate::IntersectClosest / IntersectShadow ---------------
 * (wavefront/integrator.h:32-54; CPU implementation wavefront/aggregate.cpp:34-68).  The ray
 * queue arrives in the reference's SOA layout, its size may live on the device (the reference's
 * WorkQueue::size is read by the kernels, workqueue.h:54-63, 143-152), and the calls apply the
 * reference's enqueue rules (wavefront/intersect.h:16-30, 49-156) and shadow bookkeeping
 * (intersect.h:32-47) on the device.  Output queues hold INDICES into the input queue: the
 * caller's material / light / escape stages gather their payload (beta, lambda, pixelIndex ...)
 * from the input work items by index, and the geometric part of the hit from d_hits[index].
 * IntersectShadowTr and IntersectOneRandom (aggregate.cpp:70-116) follow below in their media-free
 * form; the media themselves (SampleT_maj along ray.medium) are outside this path's scope. */
typedef struct nnbvh_ray_soa {   /* SOA<Ray> slices (workitems.soa:40-50, 82-88), device pointers */
    const float *ox, *oy, *oz;
    const float *dx, *dy, *dz;
    const float *time;           /* nullable */
    const float *tmax;           /* ShadowRayWorkItem::tMax; NULL = Infinity (RayQueue) */
    const uint8_t *has_medium;   /* nullable: ray.medium != nullptr */
} nnbvh_ray_soa;

typedef struct nnbvh_work_queue { /* WorkQueue<T> (wavefront/workqueue.h:36-113) of item indices */
    int32_t *items;               /* device, `capacity` entries */
    int32_t *size;                /* device counter, advanced atomically; NULL = queue not wanted */
    int32_t capacity;             /* pushes beyond it are counted in *size but not stored */
    int32_t pad;
} nnbvh_work_queue;

typedef struct nnbvh_closest_queues { /* the out-parameters of IntersectClosest, in its order */
    nnbvh_work_queue escaped;                 /* EscapedRayQueue                               */
    nnbvh_work_queue hit_area_light;          /* HitAreaLightQueue                             */
    nnbvh_work_queue basic_eval_material;     /* MaterialEvalQueue, basic texture evaluator    */
    nnbvh_work_queue universal_eval_material; /* MaterialEvalQueue, universal evaluator        */
    nnbvh_work_queue medium_sample;           /* MediumSampleQueue                             */
    nnbvh_work_queue next_ray;                /* rays continuing through an interface surface  */
} nnbvh_closest_queues;

/* per-primitive class byte, indexed by the primitive id a hit returns: what the reference reads
 * off the hit's SurfaceInteraction when it enqueues (intersect.h:93-128) */
#define NNBVH_CLASS_BASIC 0      /* material evaluable by BasicTextureEvaluator                */
#define NNBVH_CLASS_UNIVERSAL 1  /* needs UniversalTextureEvaluator                           */
#define NNBVH_CLASS_INTERFACE 2  /* no material: interface between media (intersect.h:103)    */
#define NNBVH_CLASS_AREA_LIGHT 4 /* intr.areaLight set (intersect.h:113); combines with 0/1   */

/* n = min(max_rays, *d_size) when d_size != NULL, else max_rays.  d_hits: nnbvh_hit[max_rays].
 * d_prim_class may be NULL (every primitive NNBVH_CLASS_BASIC). */
int nnbvh_wavefront_intersect_closest(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                      const int32_t *d_size, const uint8_t *d_prim_class,
                                      int64_t n_prim_class, void *d_hits,
                                      const nnbvh_closest_queues *out, void *stream);
/* Unoccluded rays add Ld / (r_u + r_l).Average() to d_L[4 * pixel_index] (SampledSpectrum = 4
 * floats per item, SOA<SampledSpectrum> keeps them as one float4: util/soa.h:47-127).
 * d_occluded: optional uint8[max_rays] copy of the per-ray result. */
int nnbvh_wavefront_intersect_shadow(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                     const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                     const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                     int64_t n_pixels, uint8_t *d_occluded, void *stream);
/* IntersectShadow of depth d and IntersectClosest of depth d + 1 in ONE launch (wavefront/integrator.cpp: the
 * render loop traces the shadow rays of a depth and then the next depth's rays; both queues were filled by the same
 * shading pass and neither reads what the other writes).  Same results as the two calls; one ramp-up and one drain
 * of the traversal kernel instead of two.  Scenes the one-launch kernel does not cover (alpha-tested primitives)
 * and empty sides run the two calls one after the other. */
int nnbvh_wavefront_intersect_closest_and_shadow(
    nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
    const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits, const nnbvh_closest_queues *out,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, void *stream);

/* WavefrontAggregate::IntersectShadowTr (wavefront/aggregate.cpp:70-88 -> TraceTransmittance,
 * wavefront/intersect.h:164-274) for scenes WITHOUT participating media: a shadow ray passes
 * through interface surfaces (NNBVH_CLASS_INTERFACE: no material) — closest hit, SpawnRayTo the light
 * point from the hit (ray.h:75-101), again — and is blocked by the first surface that has a material;
 * T_ray, r_u, r_l stay 1, so an arriving ray adds Ld * (1 / (r_u + r_l).Average()) to its pixel sample
 * (intersect.h:258-273).  Needs the scene's shading mesh for the hit points (pi, n).  Runs as passes
 * over the still-active rays; between passes the host reads one 4-byte count (not hipGraph-
 * capturable: nnbvh_wavefront_intersect_shadow_tr_bounded below is).  d_state: optional
 * uint8[max_rays]: 0 = arrived, 1 = blocked, 2 = a host-only
 * primitive lies on the way (nothing added: the caller's to finish).  Media themselves (ray.medium,
 * SampleT_maj) are outside this path's scope. */
typedef struct nnbvh_shading_mesh nnbvh_shading_mesh;
int nnbvh_wavefront_intersect_shadow_tr(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                        const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                        const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                        const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index,
                                        float *d_L, int64_t n_pixels, uint8_t *d_state, void *stream);
/* WavefrontAggregate::IntersectOneRandom (wavefront/aggregate.cpp:90-116; GPU form gpu/optix.cu:480-573):
 * for every SubsurfaceScatterWorkItem {p0, p1, material} walk the segment p0 -> p1 surface by surface
 * (SpawnRayTo(p1), Intersect(r, 1)) and keep ONE hit whose material equals the item's, chosen by
 * WeightedReservoirSampler (util/sampling.h:524-596, unit weights, PCG32 seeded with Hash(p0, p1)).
 * d_p0 / d_p1: 3 floats per item; d_material: the item's material id; d_prim_material: material id
 * per primitive id (NULL = all 0).  Out per item: the selected hit record (prim = -1: none; instance =
 * -1: a host-only primitive lies on the segment, the item is the caller's) and the ray of its segment
 * (what nnbvh_triangle_interactions_device needs to produce the SubsurfaceInteraction), the
 * reservoir's SampleProbability (0 without a sample) and, optionally, its weight sum. */
int nnbvh_wavefront_intersect_one_random(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items,
                                         const float *d_p0, const float *d_p1, const int32_t *d_material,
                                         const int32_t *d_size, const int32_t *d_prim_material,
                                         int64_t n_prim_material, void *d_sel_hits, void *d_sel_rays,
                                         float *d_reservoir_pdf, float *d_weight_sum, void *stream);

/* The two walks above with a caller-given bound on passes and NO host round trip: the call enqueues exactly
 * max_passes passes (1..64) — a trace and one fused step kernel each, sized for max_rays / max_items and taking
 * their live count from a device counter — then a marking kernel and the final record / finish kernel.  Inside the
 * call there are kernel launches only: no copy, no memset, no synchronisation and, once the stream's workspace has
 * its size, no allocation, so after ONE warm-up call with the same max_rays / max_items on the stream the call can
 * be captured in a hipGraph and replayed (a later call on that stream with a larger size regrows the workspace
 * and invalidates such a graph).  An item is FINISHED iff the reference loop (intersect.h:183-256,
 * aggregate.cpp:100-108) makes at most max_passes calls of Intersect for it; finished items get exactly what the
 * unbounded calls give them, bit for bit.  An unfinished shadow ray gets state 2 and adds nothing to L; an
 * unfinished one-random item gets instance = -1 in its selected hit record (pdf, weight sum and segment ray are
 * then unspecified): both are the existing "the caller's to finish" marks.  d_unfinished: nullable, receives the
 * number of unfinished items.  A pass over an empty list costs launches whose waves exit at once; walks longer
 * than 64 surfaces need the unbounded calls. */
int nnbvh_wavefront_intersect_shadow_tr_bounded(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_state,
    int32_t max_passes, int32_t *d_unfinished, void *stream);
int nnbvh_wavefront_intersect_one_random_bounded(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items, const float *d_p0, const float *d_p1,
    const int32_t *d_material, const int32_t *d_size, const int32_t *d_prim_material, int64_t n_prim_material,
    void *d_sel_hits, void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum, int32_t max_passes,
    int32_t *d_unfinished, void *stream);

/* RecordShadowRayResult (wavefront/intersect.h:32-47) for a shadow batch that was traced with
 * nnbvh_intersect_any_device: the bookkeeping half of nnbvh_wavefront_intersect_shadow on its own. */
int nnbvh_wavefront_record_shadow_device(const uint8_t *d_occluded, int32_t max_rays, const int32_t *d_size,
                                         const float *d_Ld, const float *d_r_u, const float *d_r_l,
                                         const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
                                         int device, void *stream);

/* ---- film: RGBFilm's pixel accumulators on the device ------------------------------------------
 * RGBFilm::Pixel (film.h:302-307: double rgbSum[3], double weightSum; 32 B per pixel, row-major over
 * the pixel bounds) and RGBFilm::AddSample (film.h:239-255) as UpdateFilm calls it (wavefront/
 * film.cpp:13-40).  The spectral conversion sensor->ToSensorRGB(L, lambda) (film.h:95-100) stays with
 * the caller's sensor model: samples arrive as sensor RGB.  In a tile-sharded render every rank owns
 * the pixels of its tiles; pack / unpack move an index list of pixels between the film and a
 * contiguous buffer, which is what the RCCL all-gather of the per-tile film samples carries. */
typedef struct nnbvh_film nnbvh_film;
/* pixel bounds [x0, x1) x [y0, y1) (Film::PixelBounds); max_component_value = RGBFilm's clamp
 * ("maxcomponentvalue", default Infinity).  Pixels start at zero.  NULL + nnbvh_last_error(). */
nnbvh_film *nnbvh_film_create(int32_t x0, int32_t y0, int32_t x1, int32_t y1, float max_component_value,
                              int device);
void nnbvh_film_destroy(nnbvh_film *f);
int nnbvh_film_clear(nnbvh_film *f, void *stream);
/* Adds n_passes samples to each of n_per_pass pixel slots: slot i is pixel (d_px[i], d_py[i]) (slots
 * outside the bounds are skipped, wavefront/film.cpp:18-19; the slots' pixels must be distinct, as
 * the reference's pixelIndex is within a stage), sample (pass, i) is d_rgb[rgb_stride * (pass *
 * n_per_pass + i) + 0..2] with filter weight d_weight[pass * n_per_pass + i] (NULL = 1).  A slot's
 * passes are added in order, so the sums equal the reference's sample loop bit for bit.
 * n_per_pass is clamped to *d_size when d_size != NULL. */
int nnbvh_film_add_samples_device(nnbvh_film *f, const int32_t *d_px, const int32_t *d_py,
                                  const float *d_rgb, int32_t rgb_stride, const float *d_weight,
                                  int32_t n_per_pass, int32_t n_passes, const int32_t *d_size,
                                  void *stream);
/* the accumulators themselves: *d_pixels = double[4 * *n_pixels] on the film's device */
int nnbvh_film_pixels_device(nnbvh_film *f, void **d_pixels, int64_t *n_pixels);
int nnbvh_film_read(nnbvh_film *f, double *out); /* synchronous copy to double[4 * n_pixels] */
/* d_index: n linear pixel indices ((y - y0) * width + (x - x0)); buffer: 4 doubles per index */
int nnbvh_film_pack_pixels_device(nnbvh_film *f, const int32_t *d_index, int64_t n, void *d_out,
                                  void *stream);
int nnbvh_film_unpack_pixels_device(nnbvh_film *f, const int32_t *d_index, int64_t n, const void *d_in,
                                    void *stream);

/* ---- hit record -> SurfaceInteraction: Triangle:: / BilinearPatch::InteractionFromIntersection --
 * (shapes.h:884-1010 and 1396-1489, run by the shapes' Intersect on every reported hit; with
 * the SurfaceInteraction constructor and SetShadingGeometry, interaction.h:32-33, 164-214).  A
 * device post-pass over a batch of hit records; bit-identical to the reference function.
 * The mesh data are TriangleMesh's (util/mesh.h:24-72) flattened over all meshes of the scene, in
 * render space and as the TriangleMesh constructor stores them (util/mesh.cpp:36-64: normals
 * negated under reverseOrientation). */
#define NNBVH_TRI_FLIP_NORMAL 1 /* mesh->reverseOrientation ^ mesh->transformSwapsHandedness */
#define NNBVH_TRI_HAS_UV 2      /* the triangle's mesh has uv / n / s (meshes of one scene differ) */
#define NNBVH_TRI_HAS_N 4
#define NNBVH_TRI_HAS_S 8
/* tri_vertices: 3 vertex indices per primitive, primitive k being the one whose nnbvh_prim.id is k
 * (v[0] < 0: not a triangle).  patch_vertices (nullable): 4 per primitive, p00 p10 p01 p11
 * (v[0] < 0: not a bilinear patch; BilinearPatchMesh, util/mesh.h:50-72).  normals / tangents: 3
 * floats per vertex, uvs: 2, face_indices: 1 int per primitive; each nullable.  tri_flags:
 * NNBVH_TRI_* per primitive; NULL = no flip and the HAS_* bits follow from which arrays were given. */
nnbvh_shading_mesh *nnbvh_shading_mesh_create(const float *verts, int n_verts,
                                              const int32_t *tri_vertices,
                                              const int32_t *patch_vertices, int n_prims,
                                              const float *normals, const float *uvs,
                                              const float *tangents, const int32_t *face_indices,
                                              const uint8_t *tri_flags, int device);
/* optional: the instance table of a two-level scene (the one given to nnbvh_scene_create_instanced).
 * Hits inside instance k are then finished on the device as TransformedPrimitive::Intersect does
 * (cpu/primitive.cpp:112-125): interaction in the instance's space (wo = -ApplyInverse(ray.d)), then
 * Transform::operator()(const SurfaceInteraction &) with renderFromPrimitive (util/transform.cpp:
 * 229-261).  Without it such hits get NNBVH_INTERACTION_HOST.  Each call replaces the whole table of an
 * earlier call, animation tables included (all instances static); n_instances = 0 removes it. */
int nnbvh_shading_mesh_set_instances(nnbvh_shading_mesh *m, const nnbvh_instance *instances, int n_instances);
/* ... with AnimatedPrimitives among the instances (the tables given to nnbvh_scene_create_instanced_animated):
 * a hit inside an instance whose `animated[k].actually_animated` is set is finished as
 * AnimatedPrimitive::Intersect does (cpu/primitive.cpp:143-153) — the ray into the instance's space and the
 * interaction back out of it both through renderFromPrimitive.Interpolate(ray.time) (util/transform.cpp:
 * 1062-1081; the Slerp sines as in the traversal kernels).  animated = NULL: all static. */
int nnbvh_shading_mesh_set_instances_animated(nnbvh_shading_mesh *m, const nnbvh_instance *instances,
                                              const nnbvh_animated_transform *animated, int n_instances);
void nnbvh_shading_mesh_destroy(nnbvh_shading_mesh *m);

#define NNBVH_INTERACTION_MISS 0
#define NNBVH_INTERACTION_TRIANGLE 1 /* all fields valid (Triangle::InteractionFromIntersection) */
#define NNBVH_INTERACTION_HOST 2     /* hit on a host primitive, on a primitive the mesh has no vertices
                                        for, or inside an instance when no instance table was set: the
                                        caller finishes it on the host; only prim and status are
                                        written, as for a miss */
#define NNBVH_INTERACTION_PATCH 3    /* all fields valid (BilinearPatch::InteractionFromIntersection,
                                        shapes.h:1396-1489) */
typedef struct nnbvh_interaction {   /* 192 B */
    float pi_lo[3], pi_hi[3]; /* Point3fi pi = pHit +- gamma(7) sum|b_i p_i| (shapes.h:926-930) */
    float uv[2];
    float wo[3];              /* Normalize(-ray.d) */
    float time;
    float n[3];               /* geometric normal after FaceForward to the shading normal */
    int32_t face_index;
    float dpdu[3], dpdv[3];
    float ns[3], dpdus[3], dpdvs[3], dndus[3], dndvs[3]; /* SurfaceInteraction::shading */
    float dndu[3], dndv[3];   /* geometric normal derivatives (zero for triangles) */
    float pad0;
    int32_t prim;             /* the hit record's primitive id, -1 = miss */
    int32_t status;           /* NNBVH_INTERACTION_* */
    int32_t pad1[2];
} nnbvh_interaction;
/* One of d_rays (nnbvh_ray[max_items]) / ray_soa gives the rays the hits belong to (direction and
 * time are read).  n = min(max_items, *d_size) when d_size != NULL.  d_out: nnbvh_interaction
 * [max_items], record i for hit i. */
/* host buffers (synchronous; copies in and out, like nnbvh_intersect_closest) */
int nnbvh_triangle_interactions(const nnbvh_shading_mesh *m, const nnbvh_ray *rays, const nnbvh_hit *hits,
                                int32_t n, nnbvh_interaction *out);
int nnbvh_triangle_interactions_device(const nnbvh_shading_mesh *m, const void *d_rays,
                                       const nnbvh_ray_soa *ray_soa, const void *d_hits,
                                       int32_t max_items, const int32_t *d_size, void *d_out,
                                       void *stream);

/* ---- IntersectClosest with the work items themselves (wavefront/intersect.h:16-156) ---------------
 * The *_items calls push what nnbvh_wavefront_intersect_closest pushes and, next to each index, the
 * work item's payload as the reference's SOA queues lay it out (MaterialEvalWorkItem,
 * HitAreaLightWorkItem, MediumSampleWorkItem, the spawned ray of an interface surface:
 * wavefront/workitems.soa:63-75, 118-141, 156-174).  The SurfaceInteraction is computed in the same
 * kernel, only for the items whose queue stores geometry, and is bit-identical to
 * nnbvh_triangle_interactions_device's record of the same hit.
 *
 * In every queue slot k of each slice belongs to queue.items[k]; a slice's capacity is that of the
 * matching nnbvh_closest_queues member (pushes beyond it are counted in *size, nothing is stored).
 * Every pointer is nullable ("not wanted": no store is issued for it).  Fields per queue (others must
 * be NULL, else NNBVH_ERR_ARG):
 *   hit_area_light          prim p n uv wo
 *   basic / universal_eval  prim pi n ns dpdu dpdv dpdus dpdvs dndus dndvs wo uv face_index time
 *   medium_sample           the material fields + t_max; here wo = -ray.d, NOT normalised (intersect.h:76)
 *   next_ray                prim ray_o ray_d time (Interaction::SpawnRay(ray.d), interaction.h:98-100)
 * wo elsewhere is the interaction's Normalize(-ray.d). */
typedef struct nnbvh_item_slices { /* device pointers, one slice per component */
    int32_t *prim;       /* the hit record's primitive id: the caller maps it to material / areaLight /
                            mediumInterface as it maps NNBVH_CLASS_* today */
    float *pi[6];        /* Point3fi: x.low x.high y.low y.high z.low z.high */
    float *p[3];         /* Point3f(pi) = per-axis Interval::Midpoint, (low + high) / 2 (util/math.h:851, 862) */
    float *n[3], *ns[3], *dpdu[3], *dpdv[3], *dpdus[3], *dpdvs[3], *dndus[3], *dndvs[3];
    float *wo[3], *uv[2];
    int32_t *face_index;
    float *time;
    float *t_max;        /* MediumSampleWorkItem::tMax: the hit's t, +Infinity on a miss */
    float *ray_o[3], *ray_d[3]; /* next_ray only: the spawned ray */
} nnbvh_item_slices;

typedef struct nnbvh_closest_items {
    nnbvh_item_slices hit_area_light, basic_eval_material, universal_eval_material, medium_sample, next_ray;
    nnbvh_work_queue needs_host; /* indices of the items the device cannot finish; size NULL = dropped */
} nnbvh_closest_items;

/* Routing: that of nnbvh_wavefront_intersect_closest (the six index queues hold the same sets), except
 *   - a voided record (instance == -1: a host-only primitive lies on the ray) goes to needs_host only;
 *   - a hit the shading mesh cannot finish (its interaction status would be NNBVH_INTERACTION_HOST: a
 *     primitive without vertices in the mesh, a hit inside an instance without an instance table) goes
 *     to needs_host only;
 *   - a miss inside a medium goes to medium_sample with prim = -1 and t_max = +Infinity, and no other
 *     slice is written for it (intersect.h:19-22).
 * Hit records from any source (BVH, kd-tree, nnbvh_trace_batches_device): d_hits = nnbvh_hit[max_rays];
 * ray_queue gives the rays' d (time, has_medium optional); n = min(max_rays, *d_size) when d_size != NULL. */
int nnbvh_wavefront_enqueue_closest_items_device(const nnbvh_shading_mesh *m, int32_t max_rays,
                                                 const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                                 const void *d_hits, const uint8_t *d_prim_class,
                                                 int64_t n_prim_class, const nnbvh_closest_queues *out,
                                                 const nnbvh_closest_items *items, void *stream);
/* nnbvh_wavefront_intersect_closest, then the enqueue above.  d_hits may be NULL here (a per-stream
 * workspace of the scene's holds the records). */
int nnbvh_wavefront_intersect_closest_items(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                            const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                            const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
                                            const nnbvh_closest_queues *out, const nnbvh_closest_items *items,
                                            void *stream);
/* nnbvh_wavefront_intersect_closest_and_shadow with the closest side's items (same fallback for scenes
 * the one-launch form does not cover). */
int nnbvh_wavefront_intersect_closest_and_shadow_items(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, int32_t max_shadow_rays,
    const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_occluded,
    void *stream);

/* ---- the wavefront calls with host candidates --------------------------------------------------------
 * The plain wavefront calls above void a ray that reaches a host-only primitive and hand it to needs_host, so the
 * embedder needs a CPU aggregate of the whole scene for those rays.  These forms return such a ray's candidate-mode
 * record and its candidate list instead (nnbvh_host_candidates: device pointers, arrays of max_rays entries, rules
 * as for nnbvh_intersect_closest_candidates_device).  The loop of one wavefront iteration:
 *   1. nnbvh_wavefront_intersect_closest_[and_shadow_]items_candidates: rays with count[i] == 0 are routed exactly as
 *      the plain call routes them (same queues, same item slices); a ray with count[i] != 0 goes to needs_host only,
 *      and d_hits[i] (required) is its candidate-mode record: the closest device hit with its real instance, or void
 *      (instance == -1) for count < 0;
 *   2. the caller tests the candidates of the needs_host rays, merges them with d_hits[i] by the merge rule above and
 *      writes the merged records back into d_hits (count < 0: the ray stays the caller's);
 *   3. nnbvh_wavefront_enqueue_closest_items_indexed_device with the needs_host queue as the index list (and a fresh
 *      needs_host queue) pushes those rays: nnbvh_wavefront_enqueue_closest_items_device applied to the rays
 *      d_index[0 .. min(max_index, *d_index_size)) only (entries outside [0, max_rays) are skipped).  The pushes are
 *      appended to the same queues: the size counters continue.  A merged hit on a host shape has no vertices in the
 *      shading mesh and takes the NNBVH_INTERACTION_HOST route (needs_host);
 *   4. shadow rays: nnbvh_wavefront_intersect_shadow_candidates writes d_occluded (required) 0 / 1 / 2; rays with 0
 *      add to d_L as in the plain call, rays with 1 or 2 add nothing.  After testing the candidates of the 2s the
 *      caller passes an array that is 1 everywhere but 0 on the resolved, unoccluded rays to
 *      nnbvh_wavefront_record_shadow_device, which skips non-zero entries: no kernel of its own is needed for this.
 * A scene without host-only primitives runs the plain calls' kernels and returns count == 0 everywhere.  All item
 * slices may be NULL (index queues only).  NNBVH_ERR_ARG, and nothing launched, for a NULL d_hits / d_occluded and for
 * the candidate-argument faults of nnbvh_intersect_*_candidates_device. */
int nnbvh_wavefront_intersect_closest_items_candidates(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                                       const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                                       const uint8_t *d_prim_class, int64_t n_prim_class,
                                                       void *d_hits, const nnbvh_closest_queues *out,
                                                       const nnbvh_closest_items *items,
                                                       const nnbvh_host_candidates *c, void *stream);
int nnbvh_wavefront_enqueue_closest_items_indexed_device(const nnbvh_shading_mesh *m, int32_t max_rays,
                                                         const nnbvh_ray_soa *ray_queue, const int32_t *d_index,
                                                         const int32_t *d_index_size, int32_t max_index,
                                                         const void *d_hits, const uint8_t *d_prim_class,
                                                         int64_t n_prim_class, const nnbvh_closest_queues *out,
                                                         const nnbvh_closest_items *items, void *stream);
int nnbvh_wavefront_intersect_shadow_candidates(nnbvh_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                                const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                                const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                                int64_t n_pixels, uint8_t *d_occluded /* required */,
                                                const nnbvh_host_candidates *c, void *stream);
/* The closest and the shadow call above in ONE launch of the traversal kernel (its candidate-mode instances), with
 * the fallback of nnbvh_wavefront_intersect_closest_and_shadow for the scenes the one-launch kernel does not cover
 * (alpha-tested primitives) and for an empty side: the two calls one after the other.  c: the closest side's
 * candidates, shadow_c: the shadow side's (its before is not read). */
int nnbvh_wavefront_intersect_closest_and_shadow_items_candidates(
    nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, const nnbvh_host_candidates *c,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded /* required */, const nnbvh_host_candidates *shadow_c, void *stream);

/* ---- KdTreeAggregate (cpu/aggregates.h:75-105; aggregates.cpp:746-1161) --------------------------
 * The reference's other accelerator ("kdtree" in CreateAccelerator, aggregates.cpp:1163-1178) and the
 * native structure of the learned trees of machine_learning/nss_*.py.
 *   nnbvh_kd_node             <- KdTreeNode (aggregates.cpp:753-775): 8 B; interior = {Float split,
 *                                flags = axis | aboveChild << 2} with the below child at index + 1; leaf =
 *                                {onePrimitiveIndex | primitiveIndicesOffset, flags = 3 | nPrimitives << 2}
 *   nnbvh_kd_build_create     <- KdTreeAggregate ctor + buildTree (aggregates.cpp:798-971), host-side
 *   nnbvh_kd_scene_create     <- takes what KdTreeAggregate owns after construction: nodes,
 *                                primitiveIndices, the primitives in their ORIGINAL order, bounds
 *   nnbvh_kd_intersect_*      <- KdTreeAggregate::Intersect / IntersectP (aggregates.cpp:973-1150);
 *                                nodes_visited = kdNodesVisited (aggregates.cpp:796), prim_tests =
 *                                nTriTests; a primitive that overlaps several leaves is tested in each
 *                                (the reference has no mailboxing). */
typedef struct nnbvh_kd_node {
    uint32_t split_or_index; /* bit pattern of the float split position, or the leaf's int32 */
    uint32_t flags;
} nnbvh_kd_node;
typedef struct nnbvh_kd_build nnbvh_kd_build;
typedef struct nnbvh_kd_scene nnbvh_kd_scene;
/* defaults of KdTreeAggregate::Create (aggregates.cpp:1152-1161): isect_cost 5, traversal_cost 1,
 * empty_bonus 0.5, max_prims 1, max_depth -1 (= round(8 + 1.3 log2 n)).  prim_bounds as for
 * nnbvh_build_create_with_bounds (read for NNBVH_PRIM_HOST entries).  Triangles, patches and
 * host-only primitives; instances are not accepted. */
nnbvh_kd_build *nnbvh_kd_build_create(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                      const float *prim_bounds, int isect_cost, int traversal_cost,
                                      float empty_bonus, int max_prims, int max_depth);
/* The same construction on the GPU (`device`), level by level (kd_build_gpu.hip): the identical node array —
 * split planes, child links, leaf sizes and primitiveIndices offsets do not depend on how a sort orders EQUAL
 * (t, type) edges — with the primitives inside a multi-primitive leaf in std::stable_sort order, where
 * nnbvh_kd_build_create leaves them as libstdc++'s std::sort does (aggregates.cpp:899-903 leaves that order
 * to the standard library).  nnbvh_kd_build_create_stable is the host builder with that same order: the
 * device builder's byte-for-byte checker.  No CPU fallback: without a HIP device the call fails. */
nnbvh_kd_build *nnbvh_kd_build_create_gpu(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                          const float *prim_bounds, int isect_cost, int traversal_cost,
                                          float empty_bonus, int max_prims, int max_depth, int device);
nnbvh_kd_build *nnbvh_kd_build_create_stable(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                             const float *prim_bounds, int isect_cost, int traversal_cost,
                                             float empty_bonus, int max_prims, int max_depth);
/* milliseconds of the device builder: [0] on the device (upload of the bounds .. both arrays written),
 * [1] including the download; zeros for a host build */
int nnbvh_kd_build_timing(const nnbvh_kd_build *b, double out_ms[2]);
const nnbvh_kd_node *nnbvh_kd_build_nodes(const nnbvh_kd_build *b, int *n_nodes);
const int32_t *nnbvh_kd_build_prim_indices(const nnbvh_kd_build *b, int *n_indices);
int nnbvh_kd_build_bounds(const nnbvh_kd_build *b, float out_min_max[6]);
int nnbvh_kd_build_depth(const nnbvh_kd_build *b); /* edges root -> deepest node */
void nnbvh_kd_build_destroy(nnbvh_kd_build *b);

/* The tree is validated (child links, leaf ranges, primitive indices, depth <= 64 = the reference's
 * toVisit[64], aggregates.cpp:982) before anything is uploaded.  prims: n_prims primitives indexed
 * by the leaves (triangles, alpha-tested triangles NNBVH_PRIM_ALPHA_TRIANGLE[_FLIPPED], bilinear
 * patches, host-only primitives); hit.prim reports nnbvh_prim.id. */
nnbvh_kd_scene *nnbvh_kd_scene_create(const nnbvh_kd_node *nodes, int n_nodes, const int32_t *prim_indices,
                                      int n_indices, const nnbvh_prim *prims, int n_prims,
                                      const float *verts, int n_verts, const float bounds_min_max[6],
                                      int device);
/* ... with the attributes the alpha-tested kinds read: normals and uvs per vertex, prim_alpha per entry of `prims`
 * (kd primitives are in the caller's order).  A kind whose arrays are missing stays the host's (record void), as
 * every such kind does through nnbvh_kd_scene_create. */
nnbvh_kd_scene *nnbvh_kd_scene_create_with_attributes(const nnbvh_kd_node *nodes, int n_nodes,
                                                      const int32_t *prim_indices, int n_indices,
                                                      const nnbvh_prim *prims, int n_prims, const float *verts,
                                                      int n_verts, const float bounds_min_max[6], const float *normals,
                                                      const float *uvs, const float *prim_alpha, int device);
/* Primitives in, traceable kd scene out, and the tree never visits the host: primitive bounds, their union, the device
 * builder of nnbvh_kd_build_create_gpu and the primitive records all run on `device` (kd_bake.hip).  The scene is the
 * one nnbvh_kd_build_create_stable + nnbvh_kd_scene_create_with_attributes make from the same arguments: the four
 * device arrays byte for byte (the sign of a +-0 split plane included), bounds, depth and every later result.  LEAF
 * ORDER: as with nnbvh_kd_build_create_gpu, the primitives inside a multi-primitive leaf stand in std::stable_sort
 * order, not in the libstdc++ std::sort order nnbvh_kd_build_create leaves (the order that reproduces a libstdc++
 * build of the reference byte for byte); where coincident primitives tie at equal t the two scenes may name
 * different ones, and an any-hit walk may stop after a different number of tests.  The primitive list is checked on the device before anything is read through it and fails
 * with nnbvh_kd_build_create's messages; NULL / empty arrays, max_depth > 64 and the device number are refused before
 * any device work.  prim_bounds: read (and uploaded) only where the list holds NNBVH_PRIM_HOST entries.  No CPU
 * fallback: without a HIP device the call fails. */
nnbvh_kd_scene *nnbvh_kd_scene_create_gpu_build(const nnbvh_prim *prims, int n_prims, const float *verts, int n_verts,
                                                const float *prim_bounds, int isect_cost, int traversal_cost,
                                                float empty_bonus, int max_prims, int max_depth, int device);
/* ... with the attribute arrays of nnbvh_kd_scene_create_with_attributes (each nullable; a kind whose arrays are
 * missing stays the host's) */
nnbvh_kd_scene *nnbvh_kd_scene_create_gpu_build_with_attributes(const nnbvh_prim *prims, int n_prims, const float *verts,
                                                                int n_verts, const float *prim_bounds,
                                                                const float *normals, const float *uvs,
                                                                const float *prim_alpha, int isect_cost,
                                                                int traversal_cost, float empty_bonus, int max_prims,
                                                                int max_depth, int device);
/* nnbvh_kd_scene_create_with_attributes / nnbvh_kd_scene_create_gpu_build_with_attributes plus the alpha-texture table
 * the kinds 16 .. 19 index with v[3] (nnbvh_alpha_texture; the semantics of nnbvh_scene_create_with_alpha_textures).  A
 * textured triangle is a triangle for all three kd builders (its v[3] is no vertex index).  Both calls make the same
 * six device arrays (nnbvh_kd_scene_read): a textured triangle's 64-B record keeps the texture index where kind 4 keeps
 * alpha, its three (u, v) pairs go into the 96-B attribute slots — which such a scene therefore always has —, and the
 * scene owns the descriptor table (48 bytes per texture) and the texel pool (4 bytes per texel), which
 * nnbvh_kd_scene_info counts among the device bytes.  uvs (2 floats per vertex) gives a textured triangle its three
 * (u, v) pairs; uvs == NULL means the mesh has none and EVERY textured triangle takes the reference's default corners
 * (0,0), (1,0), (1,1).  Kinds 4 .. 7 may be mixed in; alpha-tested patches (kinds 8 .. 15) beside a textured triangle
 * may not (refused).  A table given to a scene that holds no textured triangle is kept (read 4 / 5) and changes no
 * result: such a scene, alpha-tested patches included, traces as the call without textures makes it.  NULL +
 * nnbvh_last_error() naming the call, before a device is looked at, for: a null or empty texture table with a textured
 * triangle present, a texture index out of range, null texels, a width or height outside 1 .. 2^24, an unknown wrap
 * mode, a smooth kind without normals — besides every fault of the call without textures.  The plain calls, the
 * one-launch batches, the wavefront queue calls and the host-candidate calls all serve such a scene; the walk calls
 * (nnbvh_kd_wavefront_walk_*) refuse it as they refuse every scene with attribute slots.  The other kd creation calls
 * refuse kinds 16 .. 19. */
nnbvh_kd_scene *nnbvh_kd_scene_create_with_alpha_textures(const nnbvh_kd_node *nodes, int n_nodes,
                                                          const int32_t *prim_indices, int n_indices,
                                                          const nnbvh_prim *prims, int n_prims, const float *verts,
                                                          int n_verts, const float bounds_min_max[6],
                                                          const float *normals, const float *uvs, const float *prim_alpha,
                                                          int device, const nnbvh_alpha_texture *textures,
                                                          int n_textures);
nnbvh_kd_scene *nnbvh_kd_scene_create_gpu_build_with_alpha_textures(const nnbvh_prim *prims, int n_prims,
                                                                    const float *verts, int n_verts,
                                                                    const float *prim_bounds, const float *normals,
                                                                    const float *uvs, const float *prim_alpha,
                                                                    int isect_cost, int traversal_cost, float empty_bonus,
                                                                    int max_prims, int max_depth, int device,
                                                                    const nnbvh_alpha_texture *textures, int n_textures);
/* What a kd scene holds, whichever call created it.  info: n_nodes, n_indices, n_prims, depth, device bytes,
 * has_host_prims, has_patches, has_attribute_slots.  read: `what` 0 = nodes (8 B each), 1 = primitiveIndices, 2 =
 * primitive records (64 B each), 3 = attribute slots (96 B each, scenes that have them), 4 = alpha-texture descriptor
 * table (48 B each), 5 = alpha texel pool (4 B each; both empty in scenes without textures); synchronous;
 * NNBVH_ERR_ARG when `bytes` is not the array's exact size. */
int nnbvh_kd_scene_bounds(const nnbvh_kd_scene *s, float out_min_max[6]);
int nnbvh_kd_scene_info(const nnbvh_kd_scene *s, int64_t out[8]);
int nnbvh_kd_scene_read(const nnbvh_kd_scene *s, int what, void *out, size_t bytes);
void nnbvh_kd_scene_destroy(nnbvh_kd_scene *s);
/* host buffers (synchronous) */
int nnbvh_kd_intersect_closest(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits);
int nnbvh_kd_intersect_any(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                           int32_t *nodes_visited, int32_t *prim_tests);
/* device buffers, asynchronous on `stream` */
int nnbvh_kd_intersect_closest_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                      void *stream);
int nnbvh_kd_intersect_any_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                  void *d_nodes_visited, void *d_prim_tests, void *stream);

/* ---- kd-tree scenes: one-launch batches and wavefront queues ----------------------------------------------
 * nnbvh_kd_trace_batches_device: 1..4 independent batches (nnbvh_batch, each fewer than 2^28 rays, closest-hit or
 * any-hit, any-hit with exact counts where the batch supplies the arrays) traced by ONE kernel launch on `stream`;
 * every kd scene is covered (patches, alpha-tested kinds, host-only primitives: a ray that meets one is voided as by
 * nnbvh_kd_intersect_*).  Results are those of nnbvh_kd_intersect_closest_device / _any_device on the same rays.
 * nnbvh_kd_wavefront_*: the argument lists and meanings of the nnbvh_wavefront_* calls of the same name, on a kd
 * scene: n = min(max_rays, max(*d_size, 0)), NULL queue sizes mean "not wanted", pushes beyond a capacity are counted
 * and not stored, each call is one asynchronous operation on `stream` without a host read-back, and the
 * closest_and_shadow forms trace both queues in one launch where option "pair_one_launch" is set (below).  A bad argument (NULL scene, negative or >= 2^28
 * max_rays, ...) returns NNBVH_ERR_ARG before any device call.  Two-level scenes are not offered for kd scenes; host
 * candidates are (below), and IntersectShadowTr / IntersectOneRandom come as the walk calls (further below). */
int nnbvh_kd_trace_batches_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches, void *stream);
/* tuning knobs (speed only, never results), as nnbvh_scene_set_option: "read_soa" (lean scenes: the kernel reads a
 * queue's SOA slices itself; 0, the default: gathered into records first), "pair_one_launch" (closest_and_shadow traces
 * both queues in one launch; 0, the default: the two calls one after the other).  The defaults follow the measurement
 * rule of DESIGN.md §5.7: a new form becomes the default once a recorded run shows it ahead by more than the spread.
 * "offsets32" (0/1, speed only like the others): 0 runs the kernel instances that reach nodes, primitive records and
 * indices through 64-bit addressing although the scene fits 32-bit byte offsets; 1, the default, restores the width
 * computed from the scene's sizes.  The wide instances are correct for every scene, so the key changes speed, never
 * results, and it can never force 32-bit offsets onto a scene that does not fit them.  Any other value is NNBVH_ERR_ARG
 * (checked before the scene is looked at). */
int nnbvh_kd_scene_set_option(nnbvh_kd_scene *s, const char *key, int value);
int nnbvh_kd_wavefront_intersect_closest(nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                         const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class,
                                         void *d_hits, const nnbvh_closest_queues *out, void *stream);
int nnbvh_kd_wavefront_intersect_shadow(nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *shadow_queue,
                                        const int32_t *d_size, const float *d_Ld, const float *d_r_u,
                                        const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                        int64_t n_pixels, uint8_t *d_occluded, void *stream);
int nnbvh_kd_wavefront_intersect_closest_and_shadow(
    nnbvh_kd_scene *s, int32_t max_rays, const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
    const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits, const nnbvh_closest_queues *out,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded, void *stream);
int nnbvh_kd_wavefront_intersect_closest_items(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                               const nnbvh_ray_soa *ray_queue, const int32_t *d_size,
                                               const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
                                               const nnbvh_closest_queues *out, const nnbvh_closest_items *items,
                                               void *stream);
int nnbvh_kd_wavefront_intersect_closest_and_shadow_items(
    nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, int32_t max_shadow_rays,
    const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld, const float *d_r_u,
    const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels, uint8_t *d_occluded,
    void *stream);

/* ---- kd-tree scenes: host-only primitives as candidates ------------------------------------------------------
 * The nnbvh_host_candidates interface above on a kd scene: the same struct, the same meaning of every field, the same
 * merge rule and the same argument faults as the calls of the same name without `kd_`.  instance[] is required and
 * written as 0 (kd scenes have one level), so one resolver serves both scene types.  The argument of the BVH case
 * carries over to KdTreeAggregate::Intersect / IntersectP (aggregates.cpp:973-1150): a host-only primitive never
 * lowers the device's tMax, both walks visit nodes in the same order, and the walk's only tMax-dependent decision is
 * the `rayTMax < tMin` exit, so the device reaches a superset of the reference's leaves.
 * The repeat rule: the reference tests a primitive in every leaf the ray reaches (no mailboxing); the device lists a
 * host-only primitive once, at its first position in traversal order.  A shape's test accepts iff its t passes the
 * comparison with the current tMax, and tMax only falls, so a later test of the same shape can only repeat the
 * acceptance it already had, or miss (residual case: t within an ulp or two of the running tMax, as in step 3 of the
 * merge rule).
 * Every candidate call is traced by the record-reading one-launch kernel: a single-batch call is a launch of one
 * batch (so n < 2^28), a queue is gathered into records first (option "read_soa" has no effect), and the pair call
 * is one launch under option "pair_one_launch", else two.  A scene without host-only primitives runs the plain
 * kernels over zeroed counts.  count / before are cleared by kernel nodes: the device calls can be captured.
 * nnbvh_kd_trace_batches_candidates_device: cands[b] belongs to batches[b], capacity 0 = a plain batch (its rays are
 * voided as by nnbvh_kd_trace_batches_device).  NNBVH_ERR_ARG, before the scene is looked at and with nothing
 * launched, for a capacity outside 0..16, a NULL count / prim / instance, a NULL before on a closest batch, an any-hit
 * batch that asks for exact counts together with candidates, and a batch of 2^28 rays or more.
 * nnbvh_kd_wavefront_*_candidates: the loop of "the wavefront calls with host candidates" above, steps 3 and 4 with the
 * scene-free nnbvh_wavefront_enqueue_closest_items_indexed_device / nnbvh_wavefront_record_shadow_device. */
int nnbvh_kd_intersect_closest_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_hits,
                                                 const nnbvh_host_candidates *c, void *stream);
int nnbvh_kd_intersect_any_candidates_device(nnbvh_kd_scene *s, const void *d_rays, int64_t n, void *d_occluded,
                                             const nnbvh_host_candidates *c, void *stream);
/* host buffers (the pointers in `c` are host pointers): a plain synchronous staged copy */
int nnbvh_kd_intersect_closest_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, nnbvh_hit *hits,
                                          const nnbvh_host_candidates *c);
int nnbvh_kd_intersect_any_candidates(nnbvh_kd_scene *s, const nnbvh_ray *rays, int64_t n, uint8_t *occluded,
                                      const nnbvh_host_candidates *c);
int nnbvh_kd_trace_batches_candidates_device(nnbvh_kd_scene *s, const nnbvh_batch *batches, int n_batches,
                                             const nnbvh_host_candidates *cands, void *stream);
int nnbvh_kd_wavefront_intersect_closest_items_candidates(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m,
                                                          int32_t max_rays, const nnbvh_ray_soa *ray_queue,
                                                          const int32_t *d_size, const uint8_t *d_prim_class,
                                                          int64_t n_prim_class, void *d_hits,
                                                          const nnbvh_closest_queues *out,
                                                          const nnbvh_closest_items *items,
                                                          const nnbvh_host_candidates *c, void *stream);
int nnbvh_kd_wavefront_intersect_shadow_candidates(nnbvh_kd_scene *s, int32_t max_rays,
                                                   const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                                   const float *d_Ld, const float *d_r_u, const float *d_r_l,
                                                   const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
                                                   uint8_t *d_occluded /* required */,
                                                   const nnbvh_host_candidates *c, void *stream);
int nnbvh_kd_wavefront_intersect_closest_and_shadow_items_candidates(
    nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays, const nnbvh_ray_soa *ray_queue,
    const int32_t *d_size, const uint8_t *d_prim_class, int64_t n_prim_class, void *d_hits,
    const nnbvh_closest_queues *out, const nnbvh_closest_items *items, const nnbvh_host_candidates *c,
    int32_t max_shadow_rays, const nnbvh_ray_soa *shadow_queue, const int32_t *d_shadow_size, const float *d_Ld,
    const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L, int64_t n_pixels,
    uint8_t *d_occluded /* required */, const nnbvh_host_candidates *shadow_c, void *stream);

/* ---- kd-tree scenes: IntersectShadowTr / IntersectOneRandom walked inside ONE trace launch ----------------------
 * The argument lists and outputs of nnbvh_wavefront_intersect_shadow_tr_bounded / _one_random_bounded on a kd scene,
 * with max_surfaces (1..65536) in the place of max_passes.  The trace kernel's walk instances run the per-item loop
 * inside the lane: a lane that has finished its closest hit on a surface the walk passes through computes pi / n,
 * spawns the next ray and re-enters the tree with the same item.  A call is five kernel launches whatever
 * max_surfaces is — queue-head reset, *d_unfinished reset, init, ONE walk launch, record / finish — with no copy, no
 * memset, no synchronisation and, once the stream's workspace has its size, no allocation: after one warm-up call
 * with the same max_rays / max_items the call can be captured in a hipGraph.
 * An item is FINISHED iff the reference loop (intersect.h:183-256, aggregate.cpp:100-108) makes at most max_surfaces
 * calls of Intersect for it; finished items get what the BVH calls give them for the same closest hits, bit for bit.
 * An item that would start call max_surfaces + 1 gets the "caller's to finish" mark (state 2 and nothing added to L /
 * instance = -1) and is counted in *d_unfinished (nullable); so are, uncounted, rays that reach a host-only
 * primitive or a hit the mesh cannot finish.  max_rays == 0 zeroes *d_unfinished and returns NNBVH_OK.
 * NNBVH_ERR_ARG with nothing launched: a NULL scene or mesh, max_surfaces outside 1..65536, a negative size, 2^28
 * items or more, a NULL array with a non-zero size, a mesh on another device, a mesh with an instance table (kd
 * scenes have one level), and a scene created with the attribute arrays its alpha-tested smooth triangles or
 * alpha-tested patches read (the ATTR kernels have no walk instances; create the scene without those arrays and such
 * primitives become host-only, state 2 / instance = -1). */
int nnbvh_kd_wavefront_walk_shadow_tr(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                      const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                      const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                      const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                      int64_t n_pixels, uint8_t *d_state, int32_t max_surfaces, int32_t *d_unfinished,
                                      void *stream);
int nnbvh_kd_wavefront_walk_one_random(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_items,
                                       const float *d_p0, const float *d_p1, const int32_t *d_material,
                                       const int32_t *d_size, const int32_t *d_prim_material, int64_t n_prim_material,
                                       void *d_sel_hits, void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum,
                                       int32_t max_surfaces, int32_t *d_unfinished, void *stream);

/* ---- BVH scenes: IntersectShadowTr / IntersectOneRandom walked inside ONE trace launch ---------------------------
 * nnbvh_kd_wavefront_walk_* above on an nnbvh_scene: the argument lists and outputs of
 * nnbvh_wavefront_intersect_shadow_tr_bounded / _one_random_bounded with max_surfaces (1..65536) in the place of
 * max_passes.  The BVH trace kernel's walk instances run the per-item loop inside the lane: a lane
 * whose closest-hit walk is finished builds the hit record the closest-hit kernel would store, runs one step of the
 * walk on it and, where the item walks on, re-enters the tree at the root with the spawned ray.  A call is five kernel
 * launches whatever max_surfaces is: queue-head reset, *d_unfinished reset, init, ONE walk launch, record / finish;
 * no copy, no memset, no synchronisation and, once the stream's workspace has its size, no allocation: after one
 * warm-up call with the same max_rays / max_items the call can be captured in a hipGraph.
 * Finished items get what the bounded and unbounded calls give them, bit for bit.  An item that would start call
 * max_surfaces + 1 gets the "caller's to finish" mark (state 2 and nothing added to L / instance = -1) and is counted
 * in *d_unfinished (nullable); so are, uncounted, items whose ray reaches a host-only primitive or a hit the mesh
 * cannot finish.  Hits inside the instances of a static two-level scene are finished from the mesh's instance table.
 * max_rays == 0 zeroes *d_unfinished and returns NNBVH_OK.  The walk instances exist at stack window 8 only: the
 * speed-only option "stack_window" is ignored by these calls.
 * NNBVH_ERR_ARG with nothing launched: a NULL scene or mesh, max_surfaces outside 1..65536, a negative size, a NULL
 * array with a non-zero size, a mesh on another device, a scene with AnimatedPrimitive instances, and a scene with
 * alpha-tested primitives on the device; there are no host-candidate lists.  The bounded and unbounded calls remain
 * the route for all of these. */
int nnbvh_wavefront_walk_shadow_tr(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_rays,
                                   const nnbvh_ray_soa *shadow_queue, const int32_t *d_size,
                                   const uint8_t *d_prim_class, int64_t n_prim_class, const float *d_Ld,
                                   const float *d_r_u, const float *d_r_l, const int32_t *d_pixel_index, float *d_L,
                                   int64_t n_pixels, uint8_t *d_state, int32_t max_surfaces, int32_t *d_unfinished,
                                   void *stream);
int nnbvh_wavefront_walk_one_random(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_items, const float *d_p0,
                                    const float *d_p1, const int32_t *d_material, const int32_t *d_size,
                                    const int32_t *d_prim_material, int64_t n_prim_material, void *d_sel_hits,
                                    void *d_sel_rays, float *d_reservoir_pdf, float *d_weight_sum, int32_t max_surfaces,
                                    int32_t *d_unfinished, void *stream);

/* tuning knobs (speed only, never results): "stack_window" (LDS entries per lane: 4, 8, 16),
 * "blocks_per_cu" (0 = auto), "xcd_queues" (0/1), "prim_weight" / "refill_weight" (1..64: how much a
 * lane waiting on a primitive test / an idle lane counts against a lane waiting on an interior node,
 * which counts 16, when a wavefront picks its next step), "int_repeat" / "prim_repeat" (1..16
 * interior / primitive steps per scheduling decision; the one-launch kernel of nnbvh_trace_batches_device
 * always takes one primitive step), "fused_batches" (0/1: nnbvh_trace_batches_device as one launch where
 * the batches allow it), "top_table" (0/1: the lean one-launch kernels serve the scene's top records from
 * LDS), "top_burst" (1..65: a wavefront of those kernels with at least this many lanes at a record of the LDS
 * table advances them in a table step of their own, which loads nothing from memory; 65 = never), "offsets32" (0/1:
 * 0 makes the scene behave as if its arrays did not fit 32-bit byte offsets — never the lean instances, no LDS top
 * table, wavefront queues gathered into records; 1, the default, restores what the scene's sizes say.  The general
 * instances are correct for every scene, so this too changes speed, never results; it can never force 32-bit offsets
 * onto a scene that does not fit them; a value other than 0 / 1 is NNBVH_ERR_ARG, checked before the scene is looked
 * at).  Returns NNBVH_ERR_ARG for unknown keys. */
int nnbvh_scene_set_option(nnbvh_scene *s, const char *key, int value);

/* diagnostics: the launch ledger.  How often each trace-kernel instance has been enqueued in this process (a launch
 * recorded into a graph counts once, at capture; occupancy queries do not count).  family 0: the BVH trace instances,
 * each row of desc = {mode, window, inst, patch, alpha, soa, hostc}; family 1: the kd-tree ones, each row = {mode, patch,
 * o32, attr, hostc, 0, 0}.  Fills up to `capacity` rows of desc (7 ints each) and counts (either may be NULL) and returns
 * the number of instances of the family; reset != 0 zeroes the family's counts after reading them.  The counts are
 * process-wide relaxed atomics: exact when no other thread launches meanwhile.  Needs no device and no scene.
 * A negative return is -NNBVH_ERR_ARG (unknown family, negative capacity, capacity > 0 with both arrays NULL). */
int nnbvh_instance_launches(int family, int32_t *desc, uint64_t *counts, int capacity, int reset);

/* diagnostics: wavefront scheduling statistics accumulated since the last reset —
 * out = {interior trips, interior lanes, primitive trips, primitive lanes, refill trips,
 * refill lanes, and over the interior trips the sums of lanes waiting on an interior node,
 * on a primitive, idle; one spare; shader cycles spent in interior / primitive / refill trips; the
 * lanes of interior steps whose record came from the LDS top table; interior steps executed and the lanes
 * that took part; table trips, the lanes that took part in them and their shader cycles (these lanes are not
 * among those of the interior steps); one spare}.  All zero unless built with
 * -DNNBVH_STATS. */
int nnbvh_scene_sched_stats(nnbvh_scene *s, uint64_t out[20], int reset);

/* == Tree quality: the two scores the fork's machine_learning/ code judges a split tree by, SAH(head_node) and
 * EPO(head_node) (machine_learning/nn_loss.py:165-192, 119-135), of a flat tree as nnbvh_build_nodes produces it.
 *   A(n) = 2 (xy + xz + yz) of node n's box, in double from its float32 corners
 *   sah  = (c_inner * sum over inner nodes of A(n) + c_leaf * sum over leaves of A(n) * nprims(n)) / A(root)
 *   ext(n) = the primitives that are not in n's subtree and have at least one vertex inside n's closed box
 *            (all six comparisons >= / <=; a triangle counts whole, unclipped; the root has none)
 *   epo  = (c_inner * sum over inner nodes of area(ext(n)) + c_leaf * sum over leaves of area(ext(n)))
 *          / area(all primitives),   area = 1/2 |(p1 - p0) x (p2 - p0)| in double
 * The fork's constants are c_inner = 1.2, c_leaf = 1.0 (nn_loss.py:113-117).  The divisions are IEEE double divisions:
 * a zero root area or a zero total area gives the NaN or inf the formula gives.  The sums before the constants are
 * returned too; they do not depend on the constants. */
typedef struct nnbvh_tree_quality {
    double sah, epo;
    double inner_area, leaf_area_weighted, root_area; /* the SAH sums before the constants */
    double prim_area, ext_area_inner, ext_area_leaf;  /* the EPO sums before the constants */
    int64_t ext_pairs_inner, ext_pairs_leaf;          /* (primitive, inner node) and (primitive, leaf) external pairs */
    int32_t n_inner, n_leaves, depth, pad;            /* depth: edges from the root to the deepest leaf */
    float gpu_ms[4];                                  /* prepare, walk, reduce; upload + the three */
} nnbvh_tree_quality;

/* Scores a tree on `device`.  Host arrays in, host arrays out; the call runs on a stream of its own and returns when
 * the results are there (synchronous).  prim_ext_inner / prim_ext_leaf [n_prims], nullable: per ORDERED POSITION the
 * number of inner nodes / leaves that hold that primitive as an external.  node_external [n_nodes], nullable: the
 * number of externals of each node.  All integers are exact; the doubles come from sums of a fixed shape, so two calls
 * on the same input return the same bits.
 * The tree is checked on the host first, in O(nodes + primitives), before any device is looked at; NNBVH_ERR_ARG with
 * *out and the arrays untouched for: a null or empty array; c_inner or c_leaf not finite; a primitive that is not a
 * triangle (kinds 0, 4 .. 7 and 16 .. 19 are; the fork defines both scores on triangles only); a vertex index outside
 * [0, n_verts); a non-finite vertex or box corner; a second-child offset not in (i + 1, n_nodes) or not where the
 * first child's subtree ends; a leaf range outside [0, n_prims); an ordered position covered by no leaf or by two; a
 * node count that is not 2 * leaves - 1; a depth over 64; a child box not inside its parent's, or a primitive with a
 * vertex outside its own leaf's box (the walk prunes by the first and both make the set definition above equal to the
 * fork's pruned search).  A one-node tree is accepted.  NNBVH_ERR_DEVICE: no usable device, or a failed allocation,
 * copy or launch. */
int nnbvh_tree_quality_create(const nnbvh_linear_node *nodes, int n_nodes, const nnbvh_prim *ordered_prims, int n_prims,
                              const float *verts, int n_verts, double c_inner, double c_leaf, int device,
                              nnbvh_tree_quality *out, int32_t *prim_ext_inner, int32_t *prim_ext_leaf,
                              int32_t *node_external);

#ifdef __cplusplus
}
#endif
#endif
