// The update kernels of instanced scenes, included by kernels.h: new transforms over an unchanged
// top tree (pathed_hip_scene_set_instance_transforms: k_instance_records, k_refit_top_pass) and a new top tree
// (pathed_hip_scene_rebuild_top: k_placement_boxes, k_rebase_prototype_nodes, k_rebase_instance_roots).  The inverse, the
// record and the world box of a placement are the functions of instances.h, the ones scene creation calls on the host.
#pragma once

namespace pathed {

// the 12 floats of three consecutive float4
__device__ inline void rowsOf(const float4 *quads, float *m)
{
    const float4 r0 = quads[0], r1 = quads[1], r2 = quads[2];
    m[0] = r0.x; m[1] = r0.y; m[2] = r0.z; m[3] = r0.w;
    m[4] = r1.x; m[5] = r1.y; m[6] = r1.z; m[7] = r1.w;
    m[8] = r2.x; m[9] = r2.y; m[10] = r2.z; m[11] = r2.w;
}

// the world box of the placement with this record (instances.h: placementBox); false, and nothing written, where the record
// names a prototype outside the table -- no record of the library holds one
__device__ inline bool placementBoxOf(const float4 *record, const float4 *protoBoxes, int nPrototypes, float *lo, float *hi)
{
    const int prototype = floatAsInt(record[6].y);
    if (prototype < 0 || prototype >= nPrototypes) { return false; }
    float m[12];
    rowsOf(record, m);
    const float4 protoLo = protoBoxes[2 * prototype], protoHi = protoBoxes[2 * prototype + 1];
    const float boxLo[3] = { protoLo.x, protoLo.y, protoLo.z }, boxHi[3] = { protoHi.x, protoHi.y, protoHi.z };
    placementBox(m, boxLo, boxHi, lo, hi);
    return true;
}

// One thread per placement: the record of scene creation from 12 floats, refused by the same tests.  Quad 6 (base, prototype,
// root node, first shading record) comes from the live record.  bad[0] counts the refused transforms, bad[1] keeps the lowest
// refused index; a refused placement writes no record.
__global__ __launch_bounds__(kBlock) void k_instance_records(const float *transforms, int nInstances, const float4 *live, float4 *staged, unsigned int *bad)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= nInstances) { return; }
    float m[12], inverse[12];
    bool fine = true;
    for (int k = 0; k < 12; k++) {
        m[k] = transforms[(size_t)12 * i + k];
        if (!(m[k] - m[k] == 0.f)) { fine = false; }
    }
    if (!instanceInverse(m, inverse)) { fine = false; }
    if (!fine) {
        atomicAdd(&bad[0], 1u);
        atomicMin(&bad[1], (unsigned int)i);
        return;
    }
    const float4 ids = live[(size_t)kInstanceQuads * i + 6];
    float packed[4 * kInstanceQuads];
    packInstanceRecord(m, inverse, floatAsInt(ids.x), floatAsInt(ids.y), floatAsInt(ids.z), floatAsInt(ids.w), packed);
    float4 *record = staged + (size_t)kInstanceQuads * i;
    for (int q = 0; q < kInstanceQuads; q++) { record[q] = make_float4(packed[4 * q], packed[4 * q + 1], packed[4 * q + 2], packed[4 * q + 3]); }
}

// One thread per node of the TOP tree, nodes [0, topNodes) and nothing behind them (the prototypes' trees follow in the same
// array, in object space: they do not move), level-synchronous with double-buffered flags like k_refit_pass.  Per child:
//   instance leaf   (-ref - 1) & kInstanceLeafBit: the placement's world box (protoBoxes: lo, hi per prototype), then padBox's
//                   rule for the node's copy; the box BEFORE padBox joins the node's own bounds, as the builder's does
//   triangle leaf   world triangles do not move: the stored (padded) box stays and joins the node's own bounds
//   inner child     padBox of the unpadded bounds kept beside the nodes (boundsLo / boundsHi, topNodes entries)
//   empty           stays
// A reference that points outside its array (no tree of the builder holds one) leaves the stored box alone.
__global__ __launch_bounds__(kBlock) void k_refit_top_pass(
    float4 *nodes, int topNodes, const float4 *records, int nInstances, const float4 *protoBoxes, int nPrototypes,
    float4 *boundsLo, float4 *boundsHi, const unsigned char *readyIn, unsigned char *readyOut)
{
    const int n = blockIdx.x * kBlock + threadIdx.x;
    if (n >= topNodes) { return; }
    if (readyIn[n]) { readyOut[n] = 1; return; }
    float4 *node = nodes + (size_t)8 * n;
    const float4 refWords = node[6];
    const int refs[4] = { floatAsInt(refWords.x), floatAsInt(refWords.y), floatAsInt(refWords.z), floatAsInt(refWords.w) };
    for (int k = 0; k < 4; k++) {
        if (refs[k] >= 0 && refs[k] < topNodes && !readyIn[refs[k]]) { readyOut[n] = 0; return; }   // an inner child is not fitted yet
    }
    const float inf = __builtin_huge_valf();
    float lo[3][4], hi[3][4];
    for (int a = 0; a < 3; a++) {
        const float4 low = node[a], high = node[3 + a];
        lo[a][0] = low.x; lo[a][1] = low.y; lo[a][2] = low.z; lo[a][3] = low.w;
        hi[a][0] = high.x; hi[a][1] = high.y; hi[a][2] = high.z; hi[a][3] = high.w;
    }
    float ownLo[3] = { inf, inf, inf }, ownHi[3] = { -inf, -inf, -inf };
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ref = refs[k];
        if (ref == kEmptyChild) { continue; }
        float low[3] = { lo[0][k], lo[1][k], lo[2][k] }, high[3] = { hi[0][k], hi[1][k], hi[2][k] };
        bool padded = true;   // low / high are the stored box: nothing to pad, nothing to write
        if (ref >= 0) {
            if (ref < topNodes) {
                const float4 a = boundsLo[ref], b = boundsHi[ref];
                low[0] = a.x; low[1] = a.y; low[2] = a.z; high[0] = b.x; high[1] = b.y; high[2] = b.z;
                padded = false;
            }
        } else {
            const int code = -ref - 1;
            const int instance = code & (kInstanceLeafBit - 1);
            if ((code & kInstanceLeafBit) && instance < nInstances && placementBoxOf(records + (size_t)kInstanceQuads * instance, protoBoxes, nPrototypes, low, high)) {
                padded = false;
            }
        }
        for (int a = 0; a < 3; a++) {
            ownLo[a] = hostMin(ownLo[a], low[a]);
            ownHi[a] = hostMax(ownHi[a], high[a]);
            if (!padded) {
                const float pad = 1e-5f * hostMax(1.f, hostMax(fabsf(low[a]), fabsf(high[a])));   // bvh_build.h: padBox
                lo[a][k] = low[a] - pad;
                hi[a][k] = high[a] + pad;
            }
        }
    }
    for (int a = 0; a < 3; a++) {
        node[a] = make_float4(lo[a][0], lo[a][1], lo[a][2], lo[a][3]);
        node[3 + a] = make_float4(hi[a][0], hi[a][1], hi[a][2], hi[a][3]);
    }
    boundsLo[n] = make_float4(ownLo[0], ownLo[1], ownLo[2], 0.f);
    boundsHi[n] = make_float4(ownHi[0], ownHi[1], ownHi[2], 0.f);
    readyOut[n] = 1;
}

// One thread per placement: its world box, (lo, hi) as two float4, for the builder of the new top tree (lbvh.hip:
// buildTopBvhOnDevice).  A prototype index outside the table gives an empty box at the origin instead of a read out of bounds.
__global__ __launch_bounds__(kBlock) void k_placement_boxes(const float4 *records, int nInstances, const float4 *protoBoxes, int nPrototypes, float4 *boxes)
{
    const int i = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (i >= nInstances) { return; }
    float low[3] = { 0.f, 0.f, 0.f }, high[3] = { 0.f, 0.f, 0.f };
    placementBoxOf(records + (size_t)kInstanceQuads * i, protoBoxes, nPrototypes, low, high);
    boxes[2 * (size_t)i] = make_float4(low[0], low[1], low[2], 0.f);
    boxes[2 * (size_t)i + 1] = make_float4(high[0], high[1], high[2], 0.f);
}

// The prototypes' trees, nodes [oldTop, oldCount) of the old array, copied behind the new top tree: one thread per float4.
// Their inner references (>= 0) move by delta = newTop - oldTop; leaf references are absolute into the leaf triangles, whose
// layout [world | prototypes] keeps its size, and stay, as do the boxes.
__global__ __launch_bounds__(kBlock) void k_rebase_prototype_nodes(const float4 *oldNodes, int oldTop, int oldCount, float4 *newNodes, int newTop)
{
    const size_t quad = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (quad >= (size_t)8 * (size_t)(oldCount - oldTop)) { return; }
    float4 value = oldNodes[(size_t)8 * oldTop + quad];
    if ((quad & 7) == 6) {
        const int delta = newTop - oldTop;
        int refs[4] = { floatAsInt(value.x), floatAsInt(value.y), floatAsInt(value.z), floatAsInt(value.w) };
        for (int k = 0; k < 4; k++) { if (refs[k] >= 0) { refs[k] += delta; } }
        value = make_float4(__int_as_float(refs[0]), __int_as_float(refs[1]), __int_as_float(refs[2]), __int_as_float(refs[3]));
    }
    newNodes[(size_t)8 * newTop + quad] = value;
}

// ... and every placement's record into the staged buffer with its protoRoot (word 2 of quad 6) moved by the same delta
__global__ __launch_bounds__(kBlock) void k_rebase_instance_roots(const float4 *live, float4 *staged, int nInstances, int delta)
{
    const size_t quad = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (quad >= (size_t)kInstanceQuads * (size_t)nInstances) { return; }
    float4 value = live[quad];
    if (quad % kInstanceQuads == 6) { value.z = __int_as_float(floatAsInt(value.z) + delta); }
    staged[quad] = value;
}

}  // namespace pathed
