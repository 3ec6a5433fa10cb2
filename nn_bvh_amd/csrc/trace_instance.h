// trace_instance.h — the trace_kernel instances (bvh_trace.hip) the library holds and the choice among them for a call
// on a BVH scene.  Nothing of HIP in here: tests/test_trace_instance.py pins every decision with the host compiler alone.
#pragma once

namespace nnbvh {

// the template arguments of trace_kernel under their names (what is left out is 0); modes 4 / 5 are the walk instances
struct TraceInstance {
    int mode, window, inst, patch, alpha, soa, hostc;
};

// Every instance the library holds: bvh_trace.hip compiles what is listed here and nothing else.  (The order is the
// order of the kernels in the compiler's output, which tools/isa_diff.py compares as a whole: mode by mode.)
constexpr TraceInstance kTraceInstances[] = {
    // mode 3 (window 8, no ALPHA forms): candidate twins INST 2 / 1 / 0, two-level, lean SOA and record, general
    {3, 8, 2, 1, 0, 0, 1}, {3, 8, 1, 1, 0, 0, 1}, {3, 8, 0, 1, 0, 0, 1}, {3, 8, 2, 1}, {3, 8, 1, 1},
    {3, 8, 0, 0, 0, 1}, {3, 8, 0, 0}, {3, 8, 0, 1},
    // mode 0, candidate twins: image-textured alpha (flat scenes only), then ALPHA 2 / 1 / 0 x INST 0 / 2 / 1
    {0, 8, 0, 1, 3, 0, 1}, {0, 8, 0, 1, 2, 0, 1}, {0, 8, 2, 1, 2, 0, 1}, {0, 8, 1, 1, 2, 0, 1}, {0, 8, 0, 1, 1, 0, 1},
    {0, 8, 2, 1, 1, 0, 1}, {0, 8, 1, 1, 1, 0, 1}, {0, 8, 0, 1, 0, 0, 1}, {0, 8, 2, 1, 0, 0, 1}, {0, 8, 1, 1, 0, 0, 1},
    // mode 0: image-textured alpha, ALPHA 2 / 1 x INST 0 / 2 / 1, the two-level forms without alpha
    {0, 8, 0, 1, 3}, {0, 8, 0, 1, 2}, {0, 8, 2, 1, 2}, {0, 8, 1, 1, 2}, {0, 8, 0, 1, 1}, {0, 8, 2, 1, 1},
    {0, 8, 1, 1, 1}, {0, 8, 2, 1}, {0, 8, 1, 1},
    // mode 0: the lean SOA and record forms, the general window-4, 8 and 16 forms
    {0, 8, 0, 0, 0, 1}, {0, 8, 0, 0}, {0, 4, 0, 1}, {0, 8, 0, 1}, {0, 16, 0, 1},
    // mode 1 (no candidate twins, no SOA form): alpha and two-level forms as mode 0's, lean, general window 4, 8, 16
    {1, 8, 0, 1, 3}, {1, 8, 0, 1, 2}, {1, 8, 2, 1, 2}, {1, 8, 1, 1, 2}, {1, 8, 0, 1, 1}, {1, 8, 2, 1, 1},
    {1, 8, 1, 1, 1}, {1, 8, 2, 1}, {1, 8, 1, 1}, {1, 8, 0, 0}, {1, 4, 0, 1}, {1, 8, 0, 1}, {1, 16, 0, 1},
    // mode 2: the three groups of mode 0
    {2, 8, 0, 1, 3, 0, 1}, {2, 8, 0, 1, 2, 0, 1}, {2, 8, 2, 1, 2, 0, 1}, {2, 8, 1, 1, 2, 0, 1}, {2, 8, 0, 1, 1, 0, 1},
    {2, 8, 2, 1, 1, 0, 1}, {2, 8, 1, 1, 1, 0, 1}, {2, 8, 0, 1, 0, 0, 1}, {2, 8, 2, 1, 0, 0, 1}, {2, 8, 1, 1, 0, 0, 1},
    {2, 8, 0, 1, 3}, {2, 8, 0, 1, 2}, {2, 8, 2, 1, 2}, {2, 8, 1, 1, 2}, {2, 8, 0, 1, 1}, {2, 8, 2, 1, 1},
    {2, 8, 1, 1, 1}, {2, 8, 2, 1}, {2, 8, 1, 1},
    {2, 8, 0, 0, 0, 1}, {2, 8, 0, 0}, {2, 4, 0, 1}, {2, 8, 0, 1}, {2, 16, 0, 1},
    // the six walk instances (lean, general, static two-level): IntersectShadowTr's, then IntersectOneRandom's
    {4, 8, 0, 0}, {4, 8, 0, 1}, {4, 8, 1, 1}, {5, 8, 0, 0}, {5, 8, 0, 1}, {5, 8, 1, 1}};

// Everything the choice reads from a scene (scene_traits of capi_internal.h; the fields of nnbvh_scene, `animated`: a
// two-level scene has AnimatedPrimitives among its instances, `fits32`: both device arrays lie below 4 GiB).
struct TraceTraits {
    int window, instanced, animated, has_patches, has_alpha, has_host_prims, fits32;
};

// the scenes of the lean instances (PATCH = 0; their SOA forms read a wavefront queue's slices themselves)
inline bool is_lean(const TraceTraits &t) {
    return !t.instanced && !t.has_patches && !t.has_alpha && !t.has_host_prims && t.fits32 && t.window == 8;
}

// The instance of modes 0 .. 3 for a call, false = there is none.  candidates: the HOSTC twins (mode 1 has none and
// ignores it).  soa: the batch (mode 3: some batch) is a wavefront queue.  Two-level scenes, alpha and candidates have
// one window-8 record form each: those calls ignore `window` and `soa`.
inline bool pick_trace_instance(const TraceTraits &t, int mode, bool candidates, bool soa, TraceInstance *out) {
    if (mode < 0 || mode > 3 || (mode == 3 && (t.window != 8 || t.has_alpha))) return false;  // mode 3: no such forms
    const int hostc = candidates && mode != 1;
    if (hostc || t.instanced || t.has_alpha) {              // the general window-8 forms: INST x ALPHA x HOSTC
        if (t.has_alpha == 3 && t.instanced) return false;  // no such form: a two-level scene with textured triangles reports 2
        *out = {mode, 8, !t.instanced ? 0 : (t.animated ? 2 : 1), 1, t.has_alpha, 0, hostc};
    } else if (is_lean(t) && !(soa && mode == 1)) {
        *out = {mode, 8, 0, 0, 0, soa, 0};
    } else if (soa || (t.window != 4 && t.window != 8 && t.window != 16)) {
        return false;  // SOA batches: lean instances of modes 0 / 2 / 3 only (the caller gathers otherwise)
    } else {
        *out = {mode, t.window, 0, 1, 0, 0, 0};
    }
    return true;
}

// The walk instance (always window 8: the speed-only `stack_window` is ignored) of kind 1, IntersectShadowTr's walk, or
// 2, IntersectOneRandom's.  form 0: lean (the shading mesh too: no patches, no instances), 1: general, 2: two-level.
inline bool pick_walk_instance(const TraceTraits &t, int kind, bool mesh_has_patches, bool mesh_has_instances,
                               TraceInstance *out, int *form) {
    if (kind != 1 && kind != 2) return false;
    const TraceTraits at8{8, t.instanced, t.animated, t.has_patches, t.has_alpha, t.has_host_prims, t.fits32};
    const bool lean = is_lean(at8) && !mesh_has_patches && !mesh_has_instances;
    *form = t.instanced ? 2 : (lean ? 0 : 1);
    *out = {3 + kind, 8, t.instanced ? 1 : 0, lean ? 0 : 1, 0, 0, 0};
    return true;
}

}  // namespace nnbvh
