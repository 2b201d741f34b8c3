// The arithmetic of instanced scenes that needs no device (trace.h: "Instances"): the flatten routine,
// the inverse of a placement's transform, the world box of a placement, the 28 floats of its record, the checks of an
// instanced description and the two-level tree.  Plain float / int arrays and the Pathed* structs of include/pathed_hip.h;
// no HIP runtime, no float4, no PathedScene -- where the device wants float4 the caller reinterprets the array (asQuads).
// Every rule is stated ONCE: the library's host code, the update kernels (instance_kernels.h) and the host tests call the
// functions below.  tests/instances_host.cpp builds this header alone, plainly and under the sanitizers.
#pragma once

#include "pathed_hip.h"

#include "bvh_build.h"
#include "sample_stream.h"

#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define PATHED_INSTANCE_FN __host__ __device__ inline
#else
#define PATHED_INSTANCE_FN inline
#endif

namespace pathed {

static const int kInstanceQuads = 7;           // float4 per placement record
static const int kInstanceLeafBit = 1 << 30;   // -ref - 1 with this bit: an instance leaf, the placement in the low 30 bits
static const int kInstanceSentinel = 0x7FFFFFFF;

// ---- the flatten routine, fp32, one rounding per operation, no fused multiply-add (trace.h wraps these for V3)
PATHED_INSTANCE_FN void flattenPoint(const float *m, float x, float y, float z, float *out)
{
    out[0] = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
    out[1] = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
    out[2] = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}
PATHED_INSTANCE_FN void flattenDirection(const float *m, float x, float y, float z, float *out)
{
    out[0] = (m[0] * x + m[1] * y) + m[2] * z;
    out[1] = (m[4] * x + m[5] * y) + m[6] * z;
    out[2] = (m[8] * x + m[9] * y) + m[10] * z;
}
PATHED_INSTANCE_FN void flattenNormal(const float *inverse, float x, float y, float z, float *out)
{
    out[0] = (inverse[0] * x + inverse[4] * y) + inverse[8] * z;
    out[1] = (inverse[1] * x + inverse[5] * y) + inverse[9] * z;
    out[2] = (inverse[2] * x + inverse[6] * y) + inverse[10] * z;
}

// the inverse of the affine 3 x 4 transform m, in double, rounded once; false when m is singular or not finite
// (-ffp-contract=off: the double division and the conversions round on the device as on the host)
PATHED_INSTANCE_FN bool instanceInverse(const float *m, float *inverse)
{
    const double a = m[0], b = m[1], c = m[2], d = m[4], e = m[5], f = m[6], g = m[8], h = m[9], k = m[10];
    const double c00 = e * k - f * h, c01 = c * h - b * k, c02 = b * f - c * e;
    const double c10 = f * g - d * k, c11 = a * k - c * g, c12 = c * d - a * f;
    const double c20 = d * h - e * g, c21 = b * g - a * h, c22 = a * e - b * d;
    const double det = (a * c00 + b * c10) + c * c20;
    if (!(det != 0.0) || !(det - det == 0.0)) { return false; }
    const double r[9] = { c00 / det, c01 / det, c02 / det, c10 / det, c11 / det, c12 / det, c20 / det, c21 / det, c22 / det };
    const double tx = m[3], ty = m[7], tz = m[11];
    for (int row = 0; row < 3; row++) {
        for (int col = 0; col < 3; col++) { inverse[4 * row + col] = (float)r[3 * row + col]; }
        inverse[4 * row + 3] = (float)(-((r[3 * row] * tx + r[3 * row + 1] * ty) + r[3 * row + 2] * tz));
    }
    for (int i = 0; i < 12; i++) { if (!(inverse[i] - inverse[i] == 0.f)) { return false; } }
    return true;
}

// std::min / std::max as the host evaluates them (bvh_build.h: Box::grow), so that a signed zero lands where the host puts it
PATHED_INSTANCE_FN float hostMin(float a, float b) { return b < a ? b : a; }
PATHED_INSTANCE_FN float hostMax(float a, float b) { return a < b ? b : a; }

// A placement's world box: the eight corners of the prototype's padded box (protoLo / protoHi, bvh_build.h: padBox) through
// the flatten routine, min / max, then the pad 1e-5 max(1, |lo|, |hi|) + 1e-5 (hi - lo) for the roundings of the object-space
// ray.  (The node that holds the placement pads its copy once more, as it pads every child box.)  numpy:
// pathed_amd.instances.placement_box.
PATHED_INSTANCE_FN void placementBox(const float *m, const float *protoLo, const float *protoHi, float *lo, float *hi)
{
    const float inf = __builtin_huge_valf();
    float boxLo[3] = { inf, inf, inf }, boxHi[3] = { -inf, -inf, -inf };
    for (int corner = 0; corner < 8; corner++) {
        float point[3];
        flattenPoint(m, (corner & 1) ? protoHi[0] : protoLo[0], (corner & 2) ? protoHi[1] : protoLo[1], (corner & 4) ? protoHi[2] : protoLo[2], point);
        for (int a = 0; a < 3; a++) { boxLo[a] = hostMin(boxLo[a], point[a]); boxHi[a] = hostMax(boxHi[a], point[a]); }
    }
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-5f * hostMax(1.f, hostMax(std::fabs(boxLo[a]), std::fabs(boxHi[a]))) + 1e-5f * (boxHi[a] - boxLo[a]);
        lo[a] = boxLo[a] - pad;
        hi[a] = boxHi[a] + pad;
    }
}

// ---- the shutter (DESIGN.md section 4.6d "Shutter"): a placement moves from the 12 floats a (shutter time 0, the scene's
// current transform) to the 12 floats b (time 1), linearly, entry by entry.
// The placement's transform at time t, fp32, one rounding per operation, no fused multiply-add.  t = 0 and t = 1 give the bits
// of a and of b apart from the sign of a zero (1 * a + 0 * b turns a -0 into +0 where b is positive).  numpy:
// pathed_amd.instances.interpolate_transforms.
PATHED_INSTANCE_FN void interpolateTransform(const float *a, const float *b, float t, float *m)
{
    const float s = 1.f - t;
    for (int i = 0; i < 12; i++) { m[i] = (s * a[i]) + (t * b[i]); }
}

// The time of a sample: its stream at dimension kDimTime (sample_stream.h) scaled into the shutter.  A pure function of
// (seed, pixel, sample): no kernel stores it, and any split into calls, ranks or list passes draws the same times.
// numpy: pathed_amd.instances.sample_time.
PATHED_INSTANCE_FN float shutterTime(float u, float open, float close) { return open + (close - open) * u; }
PATHED_INSTANCE_FN float sampleTime(uint64_t seed, uint32_t pixel, uint32_t sample, float open, float close)
{
    Rng random;
    makeKey(seed, pixel, sample, &random.k0, &random.k1);
    random.dimension = kDimTime;
    return shutterTime(random.next(), open, close);
}

// A moving placement's world box over the shutter [open, close]: the union of placementBox(M(open)) and placementBox(M(close))
// plus a pad.  Why the union: in exact arithmetic M(t) = (1 - s) M(open) + s M(close) with s = (t - open) / (close - open), so
// the image of a point of the prototype moves on the straight segment between its two end images, and a box that holds both
// ends holds the segment.  What the pad covers, per axis i:
//   1. the static pad once more.  placementBox(M(t)) would pad the box of time t by 1e-5 max(1, |lo|, |hi|) + 1e-5 (hi - lo)
//      for the roundings of the object-space ray; the box of time t lies inside the union, so the same expression over the
//      union is at least that.
//   2. the roundings of the interpolated matrix.  Each entry of M(t) takes three roundings (1 - t, two products, one sum; M(open)
//      and M(close) take them too), so it is off the exact interpolant by at most 4 * 2^-24 (|a| + |b|) <= 2^-21 max(|a|, |b|),
//      and the image of a corner x of the prototype's box by at most 2^-21 (sum_j max(|a_ij|, |b_ij|) |x_j| + max(|a_i3|, |b_i3|)).
//      The pad takes 1e-6 (twice 2^-21) of that sum with |x_j| <= max(|protoLo_j|, |protoHi_j|).
// A placement with a == b bit for bit never comes here: it keeps placementBox(a).  numpy: pathed_amd.instances.moving_placement_box.
PATHED_INSTANCE_FN void movingPlacementBox(const float *a, const float *b, float open, float close, const float *protoLo, const float *protoHi, float *lo, float *hi)
{
    float first[12], last[12], lo0[3], hi0[3], lo1[3], hi1[3];
    interpolateTransform(a, b, open, first);
    interpolateTransform(a, b, close, last);
    placementBox(first, protoLo, protoHi, lo0, hi0);
    placementBox(last, protoLo, protoHi, lo1, hi1);
    for (int i = 0; i < 3; i++) {
        const float boxLo = hostMin(lo0[i], lo1[i]), boxHi = hostMax(hi0[i], hi1[i]);
        float reach = hostMax(std::fabs(a[4 * i + 3]), std::fabs(b[4 * i + 3]));
        for (int j = 0; j < 3; j++) {
            reach = reach + hostMax(std::fabs(a[4 * i + j]), std::fabs(b[4 * i + j])) * hostMax(std::fabs(protoLo[j]), std::fabs(protoHi[j]));
        }
        const float pad = (1e-5f * hostMax(1.f, hostMax(std::fabs(boxLo), std::fabs(boxHi))) + 1e-5f * (boxHi - boxLo)) + 1e-6f * reach;
        lo[i] = boxLo - pad;
        hi[i] = boxHi + pad;
    }
}

// Do the two transforms differ in any bit?  (A placement that does not move keeps its stored record and its static box.)
PATHED_INSTANCE_FN bool transformsDiffer(const float *a, const float *b)
{
    bool differ = false;
    for (int i = 0; i < 12; i++) {
        uint32_t x, y;
        __builtin_memcpy(&x, a + i, 4);
        __builtin_memcpy(&y, b + i, 4);
        differ = differ || x != y;
    }
    return differ;
}

// One placement's record, 28 floats: the transform's rows, the inverse's rows, then (base, prototype, root node, first
// shading record) as ints
PATHED_INSTANCE_FN void packInstanceRecord(const float *m, const float *inverse, int base, int prototype, int rootNode, int firstShade, float *record)
{
    for (int i = 0; i < 12; i++) { record[i] = m[i]; record[12 + i] = inverse[i]; }
    const int ids[4] = { base, prototype, rootNode, firstShade };
    __builtin_memcpy(record + 24, ids, sizeof ids);
}

// ---- the description (include/pathed_hip.h: PathedInstanceDesc)
struct InstancedLayout {
    int worldTris = 0;                        // T0
    std::vector<int> protoFirst, protoCount;  // triangle range of each prototype in the description
    std::vector<int> bases;                   // nInstances + 1 virtual-id bases
    std::vector<float> inverses;              // 12 floats per instance
};

// Everything that can be refused about an instanced scene, before anything is allocated or launched: PATHED_OK, or the code
// and the message of the FIRST check that fails (scene_tables.h: checkSceneOptions).
inline int planInstances(const PathedSceneDesc *desc, const PathedSceneOptions &options, const PathedInstanceDesc *in, InstancedLayout *layout, std::string *message)
{
    const auto fail = [&](int code, const char *text) { *message = text; return code; };
    if (in->struct_size != sizeof(PathedInstanceDesc)) { return fail(PATHED_E_INVALID, "PathedInstanceDesc.struct_size mismatch"); }
    if ((in->n_prototypes && !in->prototypes) || (in->n_instances && !in->instances)) { return fail(PATHED_E_INVALID, "prototype or instance array missing"); }
    if (in->n_instances >= (1u << 30) - 1u) { return fail(PATHED_E_INVALID, "too many instances (the limit is 2^30 - 2)"); }
    if (desc->n_spheres > 0) { return fail(PATHED_E_UNSUPPORTED, "sphere primitives in a scene with instances are not supported"); }
    bool containers = false;
    for (uint32_t i = 0; i < desc->n_materials; i++) { containers = containers || desc->materials[i].type == PATHED_MAT_PASSTHROUGH; }
    if (desc->n_media > 0 || containers) { return fail(PATHED_E_UNSUPPORTED, "media and containers (passthrough materials) in a scene with instances are not supported"); }
    if (options.refittable) { return fail(PATHED_E_UNSUPPORTED, "refittable: a scene with instances cannot be refitted"); }
    if (options.bvh_builder > PATHED_BVH_SAH_HOST + 1) { return fail(PATHED_E_UNSUPPORTED, "the device builders (LBVH, PLOC) do not build a scene with instances: use the host SAH builder"); }
    if (options.shade_kernel != 0 && options.shade_kernel != 1) { return fail(PATHED_E_UNSUPPORTED, "shade_kernel: a scene with instances renders on the wavefront's per-slot pair only (0 or 1)"); }
    if (options.node_format >= 2) { return fail(PATHED_E_UNSUPPORTED, "node_format: a scene with instances is walked over the 128-byte float nodes"); }
    // the geoms cover the triangles in order; the prototypes' geoms are the tail of the array, prototype after prototype
    uint32_t nextTriangle = 0;
    for (uint32_t g = 0; g < desc->n_geoms; g++) {
        if (desc->geoms[g].type != PATHED_GEOM_MESH || (uint32_t)desc->geoms[g].first != nextTriangle) {
            return fail(PATHED_E_INVALID, "a scene with instances: the mesh geoms must cover the triangles in order, without gaps");
        }
        nextTriangle += (uint32_t)desc->geoms[g].count;
    }
    if (nextTriangle != desc->n_triangles) { return fail(PATHED_E_INVALID, "a scene with instances: the mesh geoms must cover all triangles"); }
    if (desc->n_triangles >= (1u << 27)) { return fail(PATHED_E_INVALID, "a scene with instances stores fewer than 2^27 triangles (the instance leaf encoding)"); }
    uint32_t firstProtoGeom = desc->n_geoms;
    if (in->n_prototypes > 0) { firstProtoGeom = (uint32_t)in->prototypes[0].first_geom; }
    uint32_t nextGeom = firstProtoGeom;
    for (uint32_t p = 0; p < in->n_prototypes; p++) {
        const PathedPrototype &proto = in->prototypes[p];
        if (proto.first_geom < 0 || proto.n_geoms < 1 || (uint32_t)proto.first_geom != nextGeom || (uint64_t)nextGeom + (uint64_t)proto.n_geoms > desc->n_geoms) {
            return fail(PATHED_E_INVALID, "prototypes must name consecutive, non-empty geom ranges that end the geom array");
        }
        const int first = desc->geoms[nextGeom].first;
        int count = 0;
        for (int g = 0; g < proto.n_geoms; g++) { count += desc->geoms[nextGeom + (uint32_t)g].count; }
        if (count < 1) { return fail(PATHED_E_INVALID, "a prototype needs at least one triangle"); }
        for (int i = 0; i < count; i++) {
            const PathedMaterial &material = desc->materials[(size_t)desc->tri_material[first + i]];
            if (!(material.emit[0] == 0.f && material.emit[1] == 0.f && material.emit[2] == 0.f)) {
                return fail(PATHED_E_UNSUPPORTED, "an emissive material inside a prototype is not supported: bake such faces into world triangles, one copy per placement");
            }
        }
        layout->protoFirst.push_back(first);
        layout->protoCount.push_back(count);
        nextGeom += (uint32_t)proto.n_geoms;
    }
    if (nextGeom != desc->n_geoms) { return fail(PATHED_E_INVALID, "prototypes must name consecutive, non-empty geom ranges that end the geom array"); }
    layout->worldTris = firstProtoGeom < desc->n_geoms ? desc->geoms[firstProtoGeom].first : (int)desc->n_triangles;
    uint64_t virtualTris = (uint64_t)layout->worldTris;
    layout->inverses.resize((size_t)12 * in->n_instances);
    for (uint32_t k = 0; k < in->n_instances; k++) {
        const PathedInstance &instance = in->instances[k];
        if (instance.prototype < 0 || (uint32_t)instance.prototype >= in->n_prototypes) { return fail(PATHED_E_INVALID, "instance prototype index out of range"); }
        for (int i = 0; i < 12; i++) { if (!(instance.transform[i] - instance.transform[i] == 0.f)) { return fail(PATHED_E_INVALID, "instance transform is not finite"); } }
        if (!instanceInverse(instance.transform, &layout->inverses[(size_t)12 * k])) { return fail(PATHED_E_INVALID, "instance transform is not invertible"); }
        layout->bases.push_back((int)virtualTris);
        virtualTris += (uint64_t)layout->protoCount[(size_t)instance.prototype];
        if (virtualTris >= (1ull << 31)) { return fail(PATHED_E_INVALID, "a scene with instances: the virtual primitive ids (world triangles + every placement's) must stay below the limit of 2^31"); }
    }
    layout->bases.push_back((int)virtualTris);
    return PATHED_OK;
}

// ---- the two-level tree in one node array and one leaf-triangle array (trace.h): the top tree over the world triangles and
// the placements' world boxes, then one object-space tree per prototype, refs and firsts made absolute.
// records: 28 floats per placement (packInstanceRecord); protoBoxes: 8 floats per prototype, (lo, 0), (hi, 0).
inline FlatBvh buildInstancedBvh(const PathedSceneDesc *desc, const PathedInstanceDesc *in, const InstancedLayout &layout, int buildThreads,
                                 std::vector<float> *records, int *maxStack, std::vector<float> *protoBoxes, int *topNodes, int *topDepth)
{
    const size_t nProto = layout.protoFirst.size();
    std::vector<FlatBvh> trees(nProto);
    // what a later move of the placements needs too (pathed_hip_scene_set_instance_transforms): the padded prototype boxes
    protoBoxes->assign(8 * nProto, 0.f);
    int deepest = 0;
    for (size_t p = 0; p < nProto; p++) {
        const int first = layout.protoFirst[p], count = layout.protoCount[p];
        trees[p] = buildBvh(desc->positions, desc->indices + (size_t)3 * first, (uint32_t)count, nullptr, 0, buildThreads);
        deepest = std::max(deepest, trees[p].maxDepth);
        bvh_detail::Box box;
        box.reset();
        for (int i = 0; i < 3 * count; i++) {
            const float *corner = desc->positions + (size_t)3 * desc->indices[(size_t)3 * first + i];
            box.grow(corner, corner);
        }
        bvh_detail::padBox(box, &(*protoBoxes)[8 * p], &(*protoBoxes)[8 * p + 4]);   // what the prototype's root children span at most
    }
    std::vector<float> boxes((size_t)6 * in->n_instances);
    for (uint32_t k = 0; k < in->n_instances; k++) {
        const PathedInstance &instance = in->instances[k];
        const float *proto = &(*protoBoxes)[(size_t)8 * instance.prototype];
        placementBox(instance.transform, proto, proto + 4, &boxes[(size_t)6 * k], &boxes[(size_t)6 * k + 3]);
    }
    FlatBvh out = buildBvh(desc->positions, desc->indices, (uint32_t)layout.worldTris, boxes.data(), in->n_instances, buildThreads, 0, true);
    // the placements' one-primitive leaves (count 0, first = index + 1) become instance leaves
    for (int n = 0; n < out.nodeCount; n++) {
        for (int k = 0; k < 4; k++) {
            int ref;
            std::memcpy(&ref, &out.nodes[(size_t)kNodeFloats * n + 24 + k], 4);
            if (ref == kEmptyChildRef || ref >= 0) { continue; }
            const int payload = -ref - 1;
            if ((payload & 7) != 0) { continue; }
            bvh_detail::putInt(&out.nodes[(size_t)kNodeFloats * n + 24 + k], -(kInstanceLeafBit | ((payload >> 3) - 1)) - 1);
        }
    }
    if (out.nodeCount == 0) {
        // nothing in the world: an empty root, so that node 0 is never a prototype's
        out.nodes.assign((size_t)kNodeFloats, 0.f);
        for (int k = 0; k < 4; k++) { bvh_detail::putInt(&out.nodes[24 + k], kEmptyChildRef); }
        out.nodeCount = 1;
        out.maxDepth = 1;
    }
    // ... and the top tree's extent in the node array and its levels
    *topNodes = out.nodeCount;
    *topDepth = out.maxDepth;
    *maxStack = (3 * out.maxDepth + 1) + (3 * deepest + 1) + 1;
    out.maxDepth += deepest;
    std::vector<int> protoRoot(nProto);
    int triOffset = layout.worldTris;
    for (size_t p = 0; p < nProto; p++) {
        const int nodeOffset = out.nodeCount;
        protoRoot[p] = nodeOffset;
        const size_t nodeBase = out.nodes.size();
        out.nodes.insert(out.nodes.end(), trees[p].nodes.begin(), trees[p].nodes.end());
        for (int n = 0; n < trees[p].nodeCount; n++) {
            for (int k = 0; k < 4; k++) {
                float *slot = &out.nodes[nodeBase + (size_t)kNodeFloats * n + 24 + k];
                int ref;
                std::memcpy(&ref, slot, 4);
                if (ref == kEmptyChildRef) { continue; }
                if (ref >= 0) { bvh_detail::putInt(slot, ref + nodeOffset); continue; }
                const int payload = -ref - 1;
                bvh_detail::putInt(slot, -((((payload >> 3) + triOffset) << 3) | (payload & 7)) - 1);
            }
        }
        out.leafTris.insert(out.leafTris.end(), trees[p].leafTris.begin(), trees[p].leafTris.end());   // (prim = the index inside the prototype)
        out.nodeCount += trees[p].nodeCount;
        triOffset += layout.protoCount[p];
    }
    records->resize((size_t)4 * kInstanceQuads * in->n_instances);
    for (uint32_t k = 0; k < in->n_instances; k++) {
        const size_t prototype = (size_t)in->instances[k].prototype;
        packInstanceRecord(in->instances[k].transform, &layout.inverses[(size_t)12 * k], layout.bases[k], (int)prototype, protoRoot[prototype], layout.protoFirst[prototype],
                           &(*records)[(size_t)4 * kInstanceQuads * k]);
    }
    return out;
}

}  // namespace pathed
