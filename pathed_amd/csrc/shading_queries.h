// Test hook onto the shading library (shading.h), below the image: one thread per record runs ONE function -- a BSDF's f or
// sample, Fresnel, the sphere and environment sampling -- as the path kernels call it, on the record layouts of the oracle's
// function-level interface (tests/golden/README.md), so one array feeds the device and the oracle.  pathed_hip.hip
// (pathed_hip_debug_shading_queries) instantiates the kernel for the SceneTraits sets of the launch ladders and refuses what
// a set does not contain; the path kernels do not include this file's code.
#pragma once

#include "shading.h"

namespace pathed {

enum ShadingQuery {
    kQueryMaterialF = 0,      // material(20) isect(11) wi(3)        -> f(3) pdf
    kQueryMaterialSample = 1, // material(20) isect(11) u(3)         -> wi(3) pdf throughput(3)
    kQueryFresnel = 2,        // cos etaI etaT                        -> F
    kQuerySphereSample = 3,   // center(3) radius ref(3) u1 u2       -> point(3) normal(3) invPDF measure (0 solid angle, 1 area)
    kQuerySpherePdf = 4,      // center(3) radius ref(3)             -> pdf
    kQueryEnvEmit = 5,        // lightWo(3)                           -> Le(3)
    kQueryEnvPdf = 6,         // direction(3)                         -> pdf thetaStep phiStep (thetaPDF * phiPDF * width * height)
    kQueryEnvSample = 7,      // point(3) u1 u2                       -> point(3) normal(3) invPDF thetaStep phiStep
    kQueryCount = 8
};
static const int kQueryInputs[kQueryCount] = { 34, 34, 3, 9, 7, 3, 3, 5 };
static const int kQueryOutputs[kQueryCount] = { 4, 7, 1, 8, 1, 3, 4, 9 };

// the record's own random numbers in the order the function draws them; past the script 0.5, as the oracle's scripted generator
struct ScriptedRng {
    float u[3];
    int length, cursor;
    __device__ inline float next()
    {
        float value = 0.5f;
        if (cursor < length) { value = cursor == 0 ? u[0] : (cursor == 1 ? u[1] : u[2]); }
        cursor++;
        return value;
    }
};

__device__ inline ScriptedRng scriptedRng(const float *script, int length)
{
    ScriptedRng random;
    for (int i = 0; i < 3; i++) { random.u[i] = i < length ? script[i] : 0.5f; }
    random.length = length;
    random.cursor = 0;
    return random;
}

// isect(11) = geometric normal(3) shading normal(3) wo(3) uv(2): the record makeIsect (kernels.h) leaves of a hit
__device__ inline Isect queryIsect(const float *p, int material)
{
    Isect isect;
    isect.point = v3(0.f, 0.f, 0.f);
    isect.normal = v3(p[0], p[1], p[2]);
    isect.shadingNormal = v3(p[3], p[4], p[5]);
    isect.wo = v3(p[6], p[7], p[8]);
    isect.u = p[9];
    isect.v = p[10];
    isect.material = material;
    isect.prim = 0;
    isect.frame = normalToWorldSpace(isect.shadingNormal, isect.wo);
    isect.woLocal = v3(__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""));   // prepareLobes
    return isect;
}

// inputs, outputs: floats per record (kQueryInputs, kQueryOutputs of fn)
// materials: one DMaterial per record (the host built it from the record's 20 floats, as scene creation builds the table)
template <typename TRAITS>
__global__ void k_shading_queries(DEnv env, const DMaterial *materials, int fn, int n, int inputs, int outputs, const float *in, float *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) { return; }
    const float *p = in + (size_t)inputs * i;
    float *q = out + (size_t)outputs * i;
    if (fn == kQueryMaterialF || fn == kQueryMaterialSample) {
        const DMaterial m = materials[i];
        Isect isect = queryIsect(p + 20, (int)i);
        prepareLobes<TRAITS>(m, isect);
        if (fn == kQueryMaterialF) {
            float pdf;
            const Rgb f = materialF<TRAITS>(m, isect, v3(p[31], p[32], p[33]), &pdf);
            q[0] = f.r; q[1] = f.g; q[2] = f.b; q[3] = pdf;
        } else {
            ScriptedRng random = scriptedRng(p + 31, 3);
            const BSDFSample sample = materialSample<TRAITS>(m, isect, random);
            q[0] = sample.wiWorld.x; q[1] = sample.wiWorld.y; q[2] = sample.wiWorld.z; q[3] = sample.pdf;
            q[4] = sample.throughput.r; q[5] = sample.throughput.g; q[6] = sample.throughput.b;
        }
    } else if (fn == kQueryFresnel) {
        q[0] = dielectricReflectance(p[0], p[1], p[2]);
    } else if (TRAITS::spheres && fn == kQuerySphereSample) {
        ScriptedRng random = scriptedRng(p + 7, 2);
        const SurfaceSample sample = sphereSample<TRAITS::pairedTrig>(v3(p[0], p[1], p[2]), p[3], v3(p[4], p[5], p[6]), random);
        q[0] = sample.point.x; q[1] = sample.point.y; q[2] = sample.point.z;
        q[3] = sample.normal.x; q[4] = sample.normal.y; q[5] = sample.normal.z;
        q[6] = sample.invPDF; q[7] = sample.solidAngle ? 0.f : 1.f;
    } else if (TRAITS::spheres && fn == kQuerySpherePdf) {
        q[0] = spherePdfSolidAngle(v3(p[0], p[1], p[2]), p[3], v3(p[4], p[5], p[6]));
    } else if (TRAITS::env && fn == kQueryEnvEmit) {
        const Rgb emitted = envEmit(env, v3(p[0], p[1], p[2]));
        q[0] = emitted.r; q[1] = emitted.g; q[2] = emitted.b;
    } else if (TRAITS::env && fn == kQueryEnvPdf) {
        float parts[3];
        q[0] = envEmitPDF(env, v3(p[0], p[1], p[2]), parts);
        q[1] = parts[0]; q[2] = parts[1]; q[3] = parts[2];
    } else if (TRAITS::env && fn == kQueryEnvSample) {
        ScriptedRng random = scriptedRng(p + 3, 2);
        int steps[2];
        const SurfaceSample sample = envSample<TRAITS::pairedTrig>(env, v3(p[0], p[1], p[2]), random, steps);
        q[0] = sample.point.x; q[1] = sample.point.y; q[2] = sample.point.z;
        q[3] = sample.normal.x; q[4] = sample.normal.y; q[5] = sample.normal.z;
        q[6] = sample.invPDF; q[7] = (float)steps[0]; q[8] = (float)steps[1];
    }
}

}  // namespace pathed
