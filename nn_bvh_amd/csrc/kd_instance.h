// kd_instance.h — the kd_trace_kernel instances (kd_trace.hip) the library holds and the choice among them for a call on
// a kd-tree scene.  Nothing of HIP in here: tests/test_kd_instance.py pins every decision with the host compiler alone.
#pragma once

namespace nnbvh {

// the template arguments of kd_trace_kernel under their names (kd_trace.hip explains them; the window W follows from
// patch: kKdW / kKdWLean of kd_trace.h); modes 4 / 5 are the walk instances
struct KdInstance {
    int mode, patch, o32, attr, hostc;
};

// Every instance the library holds: kd_trace.hip compiles what is listed here and nothing else.  (The order is the
// order of the kernels in the compiler's output, which tools/isa_diff.py compares as a whole.)
constexpr KdInstance kKdInstances[] = {
    // closest / any hit: lean and patch scenes, with and without 32-bit offsets, then the attribute-reading forms
    {0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {0, 0, 1}, {1, 0, 1}, {0, 1, 1}, {1, 1, 1},
    {0, 1, 0, 1}, {1, 1, 0, 1}, {0, 1, 1, 1}, {1, 1, 1, 1},
    // batches, record form: lean / patches / attributes; SOA form (mode 3): lean only
    {2, 0, 0}, {2, 1, 0}, {2, 1, 0, 1}, {3, 0, 0}, {2, 0, 1}, {2, 1, 1}, {2, 1, 1, 1}, {3, 0, 1},
    // ... and the candidate-mode twins of the record form
    {2, 0, 0, 0, 1}, {2, 1, 0, 0, 1}, {2, 1, 0, 1, 1}, {2, 0, 1, 0, 1}, {2, 1, 1, 0, 1}, {2, 1, 1, 1, 1},
    // image-textured alpha (ATTR = 2): closest / any hit, batches, candidate-mode batches; without and with 32-bit offsets
    {0, 1, 0, 2}, {1, 1, 0, 2}, {2, 1, 0, 2}, {2, 1, 0, 2, 1}, {0, 1, 1, 2}, {1, 1, 1, 2}, {2, 1, 1, 2}, {2, 1, 1, 2, 1},
    // the walk instances: IntersectShadowTr's, then IntersectOneRandom's
    {4, 0, 0}, {4, 1, 0}, {4, 0, 1}, {4, 1, 1}, {5, 0, 0}, {5, 1, 0}, {5, 0, 1}, {5, 1, 1}};
constexpr int kKdInstanceCount = (int)(sizeof(kKdInstances) / sizeof(kKdInstances[0]));

// the row of kKdInstances that holds `is`, -1: the library does not hold it
constexpr int kd_instance_index(const KdInstance &is) {
    for (int i = 0; i < kKdInstanceCount; ++i) {
        const KdInstance &k = kKdInstances[i];
        if (k.mode == is.mode && k.patch == is.patch && k.o32 == is.o32 && k.attr == is.attr && k.hostc == is.hostc) return i;
    }
    return -1;
}

// Everything the choice reads from a scene (kd_scene_traits of kd_trace.h; the fields of nnbvh_kd_scene, `has_extras`:
// it has attribute slots, `has_alpha_tex`: a textured triangle was baked, `has_alpha_table`: a texture table is attached,
// `fits32`: its sizes allow 32-bit offsets, `offsets32` / `read_soa`: the options of these names).
struct KdTraits {
    int has_patches, has_extras, has_alpha_tex, has_alpha_table, has_host_prims, fits32, offsets32, read_soa;
};

// The instance of `mode` a scene's rays run through (the single-batch calls: mode 0, closest hit, or 1, any hit): lean,
// with patches (or what else reads the ray direction), with attribute arrays (attr 1), with textured triangles among the
// baked records (attr 2: chosen from what was baked, not from the table — a table beside alpha-tested patches and no
// textured triangle needs attr 1's patch recursion).  The offset width is what the scene's sizes allow, unless the
// "offsets32" option asks for the wide instances (the option can never force 32-bit offsets onto a scene that does not
// fit them).
inline KdInstance pick_kd_instance(const KdTraits &t, int mode) {
    const int attr = t.has_extras ? ((t.has_alpha_tex && t.has_alpha_table) ? 2 : 1) : 0;
    return {mode, (t.has_patches || t.has_extras) ? 1 : 0, (t.fits32 && t.offsets32) ? 1 : 0, attr, 0};
}

// A batch-mode launch.  all_soa: every batch comes as SOA slices; candidates: some batch has host candidates of
// capacity > 0.  *reads_soa: the kernel reads the slices itself (mode 3: lean scenes under "read_soa", never a candidate
// call), else the record form (mode 2) — the scene's instance, or where it holds host-only primitives its candidate-mode
// twin (else: the plain instance over zeroed counts).
inline KdInstance pick_kd_batch_instance(const KdTraits &t, bool all_soa, bool candidates, bool *reads_soa) {
    *reads_soa = !candidates && all_soa && t.read_soa && !t.has_patches && !t.has_extras;
    KdInstance is = pick_kd_instance(t, *reads_soa ? 3 : 2);
    is.hostc = (candidates && t.has_host_prims) ? 1 : 0;
    return is;
}

// The walk instance of kind 1, IntersectShadowTr's walk, or 2, IntersectOneRandom's: the lean instance with the
// triangle-only interaction where neither the scene nor the shading mesh holds patches, else the PATCH = 1 instance
// with the patch-capable one (launch_str_step's choice of FULL).
inline KdInstance pick_kd_walk_instance(const KdTraits &t, int kind, bool mesh_has_patches) {
    return {3 + kind, (t.has_patches || mesh_has_patches) ? 1 : 0, (t.fits32 && t.offsets32) ? 1 : 0, 0, 0};
}

}  // namespace nnbvh
