// The shutter over instanced scenes (DESIGN.md section 4.6d "Shutter"), included by kernels.h: placements that move between
// two transforms while the shutter is open (pathed_hip_scene_set_instance_motion).  The rule -- the transform at time t, a
// sample's time, a moving placement's box -- is instances.h's; the walk's and the shading's part is the MOTION / TIME
// instantiation of the statements the static kernels run (trace.h: traverseInstanced; kernels.h: traceInstancedPool,
// traceRaysInstanced, shadeSlots, makeIsect).  Here: where a slot's time comes from, the kernels, and the kernel that states
// the second transforms and the moving boxes.
#pragma once

namespace pathed {

// The time of the sample a slot works on, recomputed from (seed, pixel, sample) when the walk first asks: the unit in res.w
// and the sample's index in the state word give pixel and sample, as k_shade reads them.  A shadow entry names its slot in
// sd.w, whose state word k_shade has moved to the next vertex of the SAME sample.  Nothing is stored per slot, and a ray that
// meets no moving placement never computes it.
struct SlotTime {
    static constexpr bool shutter = true;
    const RenderParams *p;
    const DMotionSet *motion;
    unsigned int slot;
    float value;   // < 0: not computed yet (times lie in [0, 1])
    __device__ float operator()()
    {
        if (value < 0.f) {
            const int st = floatAsInt(p->state.rayD[slot].w);
            const unsigned int unit = (unsigned int)floatAsInt(p->state.res[slot].w);
            uint32_t pixel, firstSample, endSample;
            unitSamples<true>(*p, unit, &pixel, &firstSample, &endSample);
            const uint32_t sample = firstSample + (uint32_t)((st >> kStSampleShift) & kStSampleMask);
            value = sampleTime(((uint64_t)p->seedHi << 32) | p->seedLo, pixel, sample, motion->open, motion->close);
        }
        return value;
    }
};

template <bool COUNT, int STACK>
__device__ inline void traverseWithSlotTime(
    const TraceGeometry &g, const DInstanceSet &instances, const LaneStack &stack, const RenderParams &p, unsigned int slot,
    const float4 *worldO, const float4 *worldD, LaneRay &ray, TraceCounters *counters, const DMotionSet *motion)
{
    SlotTime time = { &p, motion, slot, -1.f };
    traverseInstanced<COUNT, STACK, kBlock, SlotTime>(g, instances, stack, p.maxStack, worldO, worldD, ray, counters, motion, &time);
}

// the wavefront's trace stage of a scene with motion: k_trace_instanced with every ray at the time of its slot's sample
template <int STACK, bool COUNT>
__global__ __launch_bounds__(kBlock) void k_trace_instanced_motion(RenderParams p, DInstanceSet instances, DMotionSet motion)
{
    traceInstancedPool<STACK, COUNT, true>(p, instances, &motion);
}

// ... its shade stage: k_shade_instanced, a hit on a moving placement flattened with M(t) of the hit's sample
template <bool LDS_MATERIALS, bool ENV_ONLY>
__global__ __launch_bounds__(kBlock) void k_shade_instanced_motion(RenderParams p, DInstanceSet instances, DMotionSet motion)
{
    shadeSlots<LDS_MATERIALS, ENV_ONLY, TraitsAll, true, true>(p, &instances, &motion);
}

// ... and the test hook's kernel behind pathed_hip_trace_timed: k_trace_rays_instanced with one time per ray
template <int STACK>
__global__ __launch_bounds__(kBlock) void k_trace_rays_instanced_motion(
    DScene scene, DInstanceSet instances, DMotionSet motion, const float4 *rays, const float *times, int n, int anyHit, float4 *hitsOut, int *occludedOut,
    int *stackOverflow, int maxStack
) {
    traceRaysInstanced<STACK, true>(scene, instances, rays, n, anyHit, hitsOut, occludedOut, stackOverflow, maxStack, &motion, times);
}

// One thread per placement: the second transform from 12 floats, refused by the tests of scene creation (bad[0] counts the
// refused, bad[1] keeps the lowest refused index, as in k_instance_records), whether the placement moves, and what the refit
// and the rebuild of the top tree read in place of its record -- k_placement_boxes' part for a scene with motion.  Both
// k_refit_top_pass and k_placement_boxes make a placement's box as placementBox(record's transform, box of record's
// prototype); for a MOVING placement they are handed the identity and, as "prototype" nPrototypes + i, the moving box
// (instances.h: movingPlacementBox), which the identity maps onto itself exactly and placementBox pads once more.  A
// placement that does not move is handed its live record and keeps its static box, bit for bit.
//   boxRecords  kInstanceQuads float4 per placement
//   boxTable    2 float4 per prototype (the scene's table, copied), then 2 per placement (zero where it does not move)
__global__ __launch_bounds__(kBlock) void k_motion_boxes(
    const float *transformsClose, int nInstances, const float4 *live, const float4 *protoBoxes, int nPrototypes, float open, float close,
    float4 *closeRows, int *moving, float4 *boxRecords, float4 *boxTable, unsigned int *bad)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i < 2 * nPrototypes) { boxTable[i] = protoBoxes[i]; }
    if (i >= nInstances) { return; }
    float a[12], b[12], inverse[12];
    bool fine = true;
    for (int k = 0; k < 12; k++) {
        b[k] = transformsClose[(size_t)12 * i + k];
        if (!(b[k] - b[k] == 0.f)) { fine = false; }
    }
    if (!instanceInverse(b, inverse)) { fine = false; }
    if (!fine) {
        atomicAdd(&bad[0], 1u);
        atomicMin(&bad[1], (unsigned int)i);
        return;
    }
    const float4 *record = live + (size_t)kInstanceQuads * i;
    rowsOf(record, a);
    const bool moves = transformsDiffer(a, b);
    for (int q = 0; q < 3; q++) { closeRows[(size_t)3 * i + q] = make_float4(b[4 * q], b[4 * q + 1], b[4 * q + 2], b[4 * q + 3]); }
    moving[i] = moves ? 1 : 0;
    float4 *out = boxRecords + (size_t)kInstanceQuads * i;
    float4 *slot = boxTable + 2 * ((size_t)nPrototypes + (size_t)i);
    const int prototype = floatAsInt(record[6].y);
    if (!moves || prototype < 0 || prototype >= nPrototypes) {
        for (int q = 0; q < kInstanceQuads; q++) { out[q] = record[q]; }
        slot[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        slot[1] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float4 protoLo = protoBoxes[2 * prototype], protoHi = protoBoxes[2 * prototype + 1];
    const float boxLo[3] = { protoLo.x, protoLo.y, protoLo.z }, boxHi[3] = { protoHi.x, protoHi.y, protoHi.z };
    float lo[3], hi[3];
    movingPlacementBox(a, b, open, close, boxLo, boxHi, lo, hi);
    slot[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    slot[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
    out[0] = out[3] = make_float4(1.f, 0.f, 0.f, 0.f);
    out[1] = out[4] = make_float4(0.f, 1.f, 0.f, 0.f);
    out[2] = out[5] = make_float4(0.f, 0.f, 1.f, 0.f);
    const float4 ids = record[6];
    out[6] = make_float4(ids.x, __int_as_float(nPrototypes + i), ids.z, ids.w);
}

}  // namespace pathed
