// First-hit feature images (k_features): what a denoiser or a compositor wants beside the radiance sums, rendered with the
// camera samples of the path kernels -- surface albedo, shading normal, depth, coverage -- and, as its REFERENCE mode, the
// reference's AlbedoIntegrator (src/albedo_integrator.cpp:3-11 under SampleIntegrator::samplePixel,
// src/sample_integrator.cpp:10-63).
//
// One lane per pixel, a wave per 8 x 8 pixel tile (the primary rays of a wave stay together; edge tiles are masked), tiles
// dealt to the waves of a bounded grid.  A lane walks its pixel's samples [sppBegin, sppEnd) IN SAMPLE ORDER, starting from
// what the output buffers hold, keeps the running sums in registers and stores them once: any split of a render into calls
// gives the same floats, and there is no partial-sum buffer.  The ray is the one startCameraSample makes (cameraSampleRay),
// the hit comes from traverse() over the scene's tree as in k_trace_rays -- every scene carries that tree, the ones the
// all-triangles kernels render included -- and the record is makeIsect's.  The path kernels gather none of this themselves:
// they live at their register budgets (tests/test_kernel_resources.py).
//
// Included by pathed_hip.hip after kernels.h.
#pragma once

namespace pathed {

struct FeatureBuffers {   // device pointers, null = not wanted
    float *albedo;   // 3 * W * H, layout of the radiance sums
    float *normal;   // 3 * W * H
    float *depth;    // W * H
    float *hits;     // W * H: samples that hit something
};

// The diffuse colour through the material's albedo kind: the lookups of lambertianF, without the / pi
// (reference Lambertian::albedo, src/lambertian.cpp:60-66).
__device__ inline Rgb diffuseAlbedo(const DMaterial &m, const Isect &isect)
{
    if (m.albedoType == PATHED_ALBEDO_CHECKERBOARD) { return checkerboardLookup(m, isect); }
    if (m.albedoType == PATHED_ALBEDO_TEXTURE) { return textureLookup(m, isect); }
    return matDiffuse(m);
}

// feature mode: the diffuse colour of the materials that have one, white for the purely specular ones
__device__ inline Rgb featureAlbedo(const DMaterial &m, const Isect &isect)
{
    if (m.type == PATHED_MAT_LAMBERTIAN || m.type == PATHED_MAT_OREN_NAYAR || m.type == PATHED_MAT_PLASTIC) { return diffuseAlbedo(m, isect); }
    return rgb(1.f);
}

// reference mode: Material::albedo answers (1, 0, 0) for everything but a Lambertian (include/material.h:52-54); kept, this
// mode is the drop-in
__device__ inline Rgb referenceAlbedo(const DMaterial &m, const Isect &isect)
{
    if (m.type == PATHED_MAT_LAMBERTIAN) { return diffuseAlbedo(m, isect); }
    return rgb(1.f, 0.f, 0.f);
}

// REFERENCE: p.accum receives  emit (bounce 0 counts, front side) + albedo  on a hit, the environment on a miss, non-finite
// samples dropped as the path kernels drop them; `out` is not read.  Otherwise: the sums of `out` that are wanted.
template <int STACK, bool REFERENCE>
__global__ __launch_bounds__(kBlock) void k_features(RenderParams p, FeatureBuffers out)
{
    extern __shared__ float4 ldsRaw[];
    LaneStack stack;
    stack.lds = reinterpret_cast<int *>(ldsRaw) + threadIdx.x;
    stack.overflowStride = (size_t)gridDim.x * kBlock;
    stack.overflow = p.stackOverflow + ((size_t)blockIdx.x * kBlock + threadIdx.x);

    const DScene &scene = p.scene;
    const TraceGeometry geometry = sceneGeometry(scene, true);
    const uint64_t seed = ((uint64_t)p.seedHi << 32) | p.seedLo;
    const int lane = threadIdx.x & 63;
    const int width = scene.camera.resX, height = scene.camera.resY;
    const unsigned int tilesX = (unsigned int)(width + 7) / 8u, tilesY = (unsigned int)(height + 7) / 8u;
    const unsigned int waveCount = gridDim.x * kWavesPerBlock;

    for (unsigned int tile = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6); tile < tilesX * tilesY; tile += waveCount) {
        const unsigned int tileRow = tile / tilesX;
        const int row = (int)(tileRow * 8u) + (lane >> 3);
        const int col = (int)((tile - tileRow * tilesX) * 8u) + (lane & 7);
        if (row >= height || col >= width) { continue; }
        const uint32_t pixel = (uint32_t)row * (uint32_t)width + (uint32_t)col;

        Rgb albedo = rgb(0.f);
        V3 normal = v3(0.f, 0.f, 0.f);
        float depth = 0.f, hits = 0.f;
        if (REFERENCE) {
            albedo = rgb(p.accum[3 * (size_t)pixel + 0], p.accum[3 * (size_t)pixel + 1], p.accum[3 * (size_t)pixel + 2]);
        } else {
            if (out.albedo) { albedo = rgb(out.albedo[3 * (size_t)pixel + 0], out.albedo[3 * (size_t)pixel + 1], out.albedo[3 * (size_t)pixel + 2]); }
            if (out.normal) { normal = v3(out.normal[3 * (size_t)pixel + 0], out.normal[3 * (size_t)pixel + 1], out.normal[3 * (size_t)pixel + 2]); }
            if (out.depth) { depth = out.depth[pixel]; }
            if (out.hits) { hits = out.hits[pixel]; }
        }

        for (uint32_t sample = p.sppBegin; sample < p.sppEnd; sample++) {
            Rng random;
            V3 o, d;
            cameraSampleRay(p, seed, pixel, sample, random, &o, &d);
            RayHit hit;
            hit.t = 0.f; hit.u = 0.f; hit.v = 0.f; hit.prim = -1;
            TraceCounters counters;
            const bool found = traverse<false, STACK, kBlock, 0>(geometry, stack, p.maxStack, o, d, PATHED_TNEAR, PATHED_TFAR, false, &hit, &counters);
            if (REFERENCE) {
                // SampleIntegrator::samplePixel with AlbedoIntegrator::L
                Rgb color = rgb(0.f);
                if (found) {
                    const Isect isect = makeIsect<TraitsAll>(scene, o, d, make_float4(hit.t, hit.u, hit.v, intAsFloat(hit.prim)));
                    const DMaterial &material = scene.materials[isect.material];
                    if (checkCounts(p.startBounce, p.lastBounce, 0)) {
                        const Rgb emit = matEmit(material);
                        const bool backside = dot(isect.normal, isect.wo) < 0.f;
                        if (!isBlack(emit) && !backside) { color = color + emit; }
                    }
                    color = color + referenceAlbedo(material, isect);
                } else {
                    color = color + environmentL<TraitsAll>(scene, d);
                }
                if (isfinite(color.r) && isfinite(color.g) && isfinite(color.b)) { albedo = albedo + color; }
                else { atomicAdd(&p.stats[kStatDropped], 1ull); }
            } else if (found) {
                const Isect isect = makeIsect<TraitsAll>(scene, o, d, make_float4(hit.t, hit.u, hit.v, intAsFloat(hit.prim)));
                albedo = albedo + featureAlbedo(scene.materials[isect.material], isect);
                normal = normal + isect.shadingNormal;
                depth += hit.t;
                hits += 1.f;
            }
        }

        if (REFERENCE) {
            p.accum[3 * (size_t)pixel + 0] = albedo.r; p.accum[3 * (size_t)pixel + 1] = albedo.g; p.accum[3 * (size_t)pixel + 2] = albedo.b;
        } else {
            if (out.albedo) { out.albedo[3 * (size_t)pixel + 0] = albedo.r; out.albedo[3 * (size_t)pixel + 1] = albedo.g; out.albedo[3 * (size_t)pixel + 2] = albedo.b; }
            if (out.normal) { out.normal[3 * (size_t)pixel + 0] = normal.x; out.normal[3 * (size_t)pixel + 1] = normal.y; out.normal[3 * (size_t)pixel + 2] = normal.z; }
            if (out.depth) { out.depth[pixel] = depth; }
            if (out.hits) { out.hits[pixel] = hits; }
        }
    }
}

}  // namespace pathed
