// wavefront2.h — launch interface of the kernels behind IntersectShadowTr / IntersectOneRandom
// (wavefront2.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nnbvh.h"
#include "interaction.h"
#include "wavefront.h"

namespace nnbvh {

// ---- IntersectShadowTr ------------------------------------------------------------------------
hipError_t launch_str_init(const nnbvh_ray_soa &q, WavefrontCount cnt, void *rays, int32_t *orig, float4 *pLight,
                           uint8_t *state, int maxBlocks, hipStream_t stream);
hipError_t launch_str_record(const uint8_t *state, WavefrontCount cnt, const float *Ld, const float *ru,
                             const float *rl, const int32_t *pixelIndex, float *L, long nPixels,
                             uint8_t *visibleOut, int maxBlocks, hipStream_t stream);

// ---- IntersectOneRandom -----------------------------------------------------------------------
struct OneRandomState {  // per work item, device arrays (the base interaction of a segment stays in registers)
    // Unused, always null: no kernel reads or writes it.  It keeps the members of WalkParams behind `st` at their
    // kernel-argument offsets: without it the one-random walk instances of both trace kernels allocate registers
    // differently (tools/isa_diff.py: their SGPR spills move by 4 to 8 either way).
    float *unused;
    uint64_t *rng;       // 2 per item: PCG32 state, inc
    float *weights;      // 2 per item: weightSum, reservoirWeight
};
hipError_t launch_or_init(const float *p0, const float *p1, WavefrontCount cnt, OneRandomState st, void *raysOut,
                          int32_t *origOut, int32_t *counter, void *selHits, void *selRays, int maxBlocks,
                          hipStream_t stream);
// or_init without compaction, for the walk instances of the trace kernels: every item's first segment ray, reservoir
// state and cleared outputs
hipError_t launch_or_init_all(const float *p0, const float *p1, WavefrontCount cnt, OneRandomState st, void *rays,
                              void *selHits, void *selRays, int maxBlocks, hipStream_t stream);
hipError_t launch_or_finish(WavefrontCount cnt, OneRandomState st, float *pdf, float *weightSum, int maxBlocks,
                            hipStream_t stream);

// ---- one fused step per pass: the bounded calls enqueue their passes up front, the unbounded ones pass by pass -----
// One pass of the shadow walk after its trace: hit -> verdict (w2_str_item, walk_math.h), and for an interface hit the
// interaction in registers and the next segment's ray towards pLight, appended to the next list.  cur: the list's
// size (the queue's own for the first pass, a counter of the call's for the others).
hipError_t launch_str_step(const ShadingMeshDevice &m, const void *raysCur, const void *hitsCur,
                           const int32_t *origCur, WavefrontCount cur, const uint8_t *primClass, long nPrimClass,
                           const float4 *pLight, uint8_t *state, void *raysNext, int32_t *origNext, int32_t *counter,
                           int maxBlocks, hipStream_t stream);
// ... of the one-random walk (w2_or_item)
hipError_t launch_or_step_fused(const ShadingMeshDevice &m, const void *raysCur, const void *hitsCur,
                                const int32_t *origCur, WavefrontCount cur, const float *p1, const int32_t *material,
                                const int32_t *primMaterial, long nPrimMaterial, OneRandomState st, void *raysNext,
                                int32_t *origNext, int32_t *counter, void *selHits, void *selRays, int maxBlocks,
                                hipStream_t stream);
// What the last pass left on its list is the caller's to finish: state 2 (shadow rays; a zero direction has ended
// its walk and is skipped) or instance = -1 in the selected hit record (one-random items, state == nullptr).
// *unfinished (nullable, zero before the launch) receives their number.
hipError_t launch_w2_mark_unfinished(const void *raysLeft, const int32_t *origLeft, WavefrontCount left,
                                     uint8_t *state, void *selHits, int32_t *unfinished, int maxBlocks,
                                     hipStream_t stream);

}  // namespace nnbvh
