// The host arithmetic of scene creation (pathed_hip.hip: createScene): everything that turns the scene description into
// tables without touching the device.  Plain float / int / uint32_t vectors and the Pathed* structs of include/pathed_hip.h;
// no HIP runtime, no float4, no PathedScene -- where the device wants float4 the caller reinterprets the array (asQuads).
// tests/scene_tables_host.cpp builds this header alone, plainly and under the sanitizers.
//
// The statements and the float / double types of each block are the ones createScene had inline: the bits of every table
// are pinned by tests/test_gpu_scene_fingerprint.py.
#pragma once

#include "pathed_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

namespace pathed {

// ---- options

static const int kOptionMaxPools = 4;      // pathed_hip.hip: kMaxPools
static const int kOptionMinSlots = 256;    // kernels.h: kBlock

// PATHED_OK, or PATHED_E_INVALID with the message of the FIRST check that fails (callers see one message per call).
inline int checkSceneOptions(const PathedSceneOptions &options, std::string *message)
{
    const auto refuse = [&](const char *text) { *message = text; return (int)PATHED_E_INVALID; };
    if (options.struct_size != sizeof(PathedSceneOptions)) { return refuse("PathedSceneOptions.struct_size mismatch"); }
    if (options.generic_kernels != 0 && options.generic_kernels != 1) { return refuse("generic_kernels must be 0 or 1"); }
    if (options.node_format < 0 || options.node_format > 3) { return refuse("node_format must be 0 (automatic), 1 (128-byte float nodes), 2 (compressed 64-byte nodes) or 3 (compressed 8-wide nodes)"); }
    if (options.build_threads < 0 || options.build_threads > 4096) { return refuse("build_threads must be 0..4096"); }
    if (options.unit_order < 0 || options.unit_order > 3) { return refuse("unit_order must be 0..3"); }
    if (options.bvh_builder < 0 || options.bvh_builder > PATHED_BVH_PLOC_DEVICE + 1) { return refuse("unknown BVH builder"); }
    if (options.pools < 0 || options.pools > kOptionMaxPools) { return refuse("pools must be 0..4"); }
    if (options.stack_rows != 0 && options.stack_rows != 8 && options.stack_rows != 16 && options.stack_rows != 22) {
        return refuse("stack_rows must be 0, 8, 16 or 22");
    }
    if (options.max_slots < 0 || (options.max_slots != 0 && options.max_slots < kOptionMinSlots)) { return refuse("max_slots must be 0 or >= 256"); }
    if (options.shade_kernel < 0 || options.shade_kernel > 6) { return refuse("shade_kernel must be 0..6"); }
    if (options.stage_slots != 0 && options.stage_slots != 512 && options.stage_slots != 1024) { return refuse("stage_slots must be 0, 512 or 1024"); }
    if (options.refittable != 0 && options.refittable != 1) { return refuse("refittable must be 0 or 1"); }
    if (options.small_phase1 < 0 || options.small_phase1 > 2) { return refuse("small_phase1 must be 0 (automatic), 1 (VALU) or 2 (matrix pipe)"); }
    if (options.wave_max_ksamples < 0) { return refuse("wave_max_ksamples must be >= 0"); }
    if (options.wave_stragglers < -1 || options.wave_stragglers > 64) { return refuse("wave_stragglers must be -1 (none), 0 (default) or 1..64"); }
    if (options.wave_refill < 0 || options.wave_refill > 64) { return refuse("wave_refill must be 0 (default) or 1..64"); }
    if (options.chunks_per_pass < 0 || options.chunks_per_pass > 4096) { return refuse("chunks_per_pass must be 0 (default) or 1..4096"); }
    if (options.shade_chain != 0 && options.shade_chain != 1) { return refuse("shade_chain must be 0 (automatic) or 1 (off)"); }
    if (options.shade_launches < 0 || options.shade_launches > 16) { return refuse("shade_launches must be 0 (automatic) or 1..16"); }
    if (options.local_rays != 0 && options.local_rays != 1) { return refuse("local_rays must be 0 (automatic) or 1 (off)"); }
    if (options.hybrid_batch < 0 || options.hybrid_batch > 128) { return refuse("hybrid_batch must be 0 (default) or 1..128"); }
    if (options.hybrid_ready < -1 || options.hybrid_ready > 64) { return refuse("hybrid_ready must be -1 (never), 0 (default) or 1..64"); }
    return PATHED_OK;
}

// ---- the traversal stack's shape: every launch of a kernel with a STACK template argument takes all three from here

// the LDS rows a lane's stack gets for a requested row count: the kernels exist with 8, 16 and 22 rows
constexpr int stackRowsFor(int requested) { return requested == 8 || requested == 16 ? requested : 22; }

// dynamic LDS of a block's stacks: `rows` rows and one of scratch, an int per lane (kOptionMinSlots is kBlock, the block size)
constexpr size_t stackLdsBytes(int rows) { return (size_t)(rows + 1) * kOptionMinSlots * sizeof(int); }

// ints of the HBM spill buffer of `threads` lanes: a column of the (maxStack - rows) entries a tree of bound maxStack may push
// beyond the LDS rows per lane, and never less than one column
constexpr size_t stackSpillInts(size_t threads, int maxStack, int rows) { return threads * (size_t)(maxStack > rows ? maxStack - rows : 1); }

// ---- image textures

// One array of texels (4 floats each, w = 0) for all textures, already through Texture::lookup's powf(x / 255.f, 2.2f)
// (reference src/texture.cpp:44-48; 256 possible values per channel); offsets[t] = texture t's first texel.
inline void gammaTexels(const PathedSceneDesc *desc, std::vector<float> *texels, std::vector<size_t> *offsets)
{
    float gammaTable[256];
    for (int value = 0; value < 256; value++) { gammaTable[value] = powf((unsigned char)value / 255.f, 2.2f); }
    texels->clear();
    offsets->assign(desc->n_textures, 0);
    for (uint32_t t = 0; t < desc->n_textures; t++) {
        const PathedTexture &texture = desc->textures[t];
        (*offsets)[t] = texels->size() / 4;
        const size_t count = (size_t)texture.width * texture.height;
        for (size_t k = 0; k < count; k++) {
            for (int c = 0; c < 3; c++) { texels->push_back(gammaTable[texture.rgb[3 * k + c]]); }
            texels->push_back(0.f);
        }
    }
}

// ---- spheres

// RenderParams::spherePairs: the first 16 spheres two by two, [pair][x, y, z, radius^2][half]; radius^2 < 0: nothing touches it
inline void packSpherePairs(const PathedSceneDesc *desc, float pairs[8][4][2])
{
    std::memset(pairs, 0, sizeof(float) * 8 * 4 * 2);
    for (int pair = 0; pair < 8; pair++) { pairs[pair][3][0] = -1.f; pairs[pair][3][1] = -1.f; }
    for (uint32_t i = 0; i < desc->n_spheres && i < 16u; i++) {
        for (int k = 0; k < 3; k++) { pairs[i / 2][k][i % 2] = desc->spheres[i].center_world[k]; }
        pairs[i / 2][3][i % 2] = desc->spheres[i].radius * desc->spheres[i].radius;
    }
}

// ---- lights

struct LightEntry {
    int kind;   // 0 triangle, 1 sphere, 2 environment (device_scene.h: DLight)
    int index;  // triangle prim id / sphere index
};

// Emissive surfaces in model order, the environment light last (reference src/scene_parser.cpp:173-190).
// materialEmits[m] != 0: material m emits (as the device's material record has it: only Lambertian carries emission).
inline std::vector<LightEntry> listLights(const PathedSceneDesc *desc, const std::vector<unsigned char> &materialEmits)
{
    std::vector<LightEntry> lights;
    for (uint32_t g = 0; g < desc->n_geoms; g++) {
        const PathedGeom &geom = desc->geoms[g];
        if (geom.type == PATHED_GEOM_MESH) {
            for (int i = 0; i < geom.count; i++) {
                const int tri = geom.first + i;
                if (materialEmits[(size_t)desc->tri_material[tri]]) { lights.push_back({ 0, tri }); }
            }
        } else if (materialEmits[(size_t)desc->spheres[geom.first].material]) {
            lights.push_back({ 1, geom.first });
        }
    }
    if (desc->env) { lights.push_back({ 2, 0 }); }
    return lights;
}

// ---- environment light: EnvironmentLight ctor, reference src/environment_light.cpp:14-53

// Distribution ctor, reference src/distribution.cpp:6-33 (sequential float accumulation); true = empty
inline bool buildCdf(const float *values, size_t size, float *cdf)
{
    float sum = 0.f;
    for (size_t i = 0; i < size; i++) { sum += values[i]; cdf[i] = 0.f; }
    if (sum == 0.f) { return true; }  // empty
    for (size_t i = 0; i < size; i++) {
        cdf[i] = values[i] / sum;
        if (i > 0) { cdf[i] += cdf[i - 1]; }
    }
    cdf[size - 1] = 1.f;
    return false;
}

// guide[j] = first i with cdf[i] >= j / size (the last entry when there is none), j = 0 .. size
inline void buildGuide(const float *cdf, size_t size, int *guide)
{
    size_t i = 0;
    for (size_t j = 0; j <= size; j++) {
        const float threshold = (float)j / (float)size;
        while (i + 1 < size && !(cdf[i] >= threshold)) { i++; }
        guide[j] = (int)i;
    }
}

// sampling records (device_scene.h: DEnv), two quads of 4 floats per guide cell: for the cell `bucket` the search window of
// cdfSample is [guide[bucket - 1], guide[bucket + 2]]; the record carries its start (-1 when the distribution is empty), its
// end and the CDF around the start
inline void buildRecords(const float *cdf, const int *guide, size_t size, bool empty, float *records)
{
    for (size_t bucket = 0; bucket <= size; bucket++) {
        const size_t below = bucket == 0 ? 0 : bucket - 1;
        const size_t above = bucket + 2 > size ? size : bucket + 2;
        const int lo = guide[below], hi = guide[above];
        auto at = [&](int index) { return cdf[(size_t)(index < 0 ? 0 : (index > (int)size - 1 ? (int)size - 1 : index))]; };
        int loBits = empty ? -1 : lo;
        float loAsFloat, hiAsFloat;
        std::memcpy(&loAsFloat, &loBits, 4);
        std::memcpy(&hiAsFloat, &hi, 4);
        const float record[8] = { loAsFloat, hiAsFloat, lo > 0 ? at(lo - 1) : 0.f, at(lo), at(lo + 1), at(lo + 2), 0.f, 0.f };
        std::memcpy(records + 8 * bucket, record, sizeof record);
    }
}

struct EnvTables {
    int width = 0, height = 0;
    std::vector<float> rgba;                       // 4 floats per texel
    std::vector<float> thetaCdf, phiCdf;           // height; height * width, row-major
    std::vector<int> phiEmpty;                     // height flags: 1 = the row has zero weight
    std::vector<int> thetaGuide, phiGuide;         // height + 1; height * (width + 1)
    std::vector<float> thetaRecords, phiRecords;   // 8 floats per guide cell
    int thetaEmpty = 0;
    float scale = 0.f;
    float mapToWorld[9] = {}, worldToMap[9] = {};  // the 3 x 3 parts, row-major
};

inline void buildEnvTables(const PathedEnvLight &env, EnvTables *out)
{
    const size_t texels = (size_t)env.width * env.height;
    out->rgba.assign(env.rgba, env.rgba + 4 * texels);
    std::vector<float> luminance(texels, 0.f);
    for (size_t i = 0; i < texels; i++) {
        luminance[i] += env.rgba[4 * i + 0];
        luminance[i] += env.rgba[4 * i + 1];
        luminance[i] += env.rgba[4 * i + 2];
    }
    out->thetaCdf.resize((size_t)env.height);
    out->phiCdf.resize(texels);
    out->phiEmpty.resize((size_t)env.height);
    std::vector<float> thetaData((size_t)env.height, 0.f);
    for (int row = 0; row < env.height; row++) {
        float thetaSum = 0.f;
        for (int col = 0; col < env.width; col++) { thetaSum += luminance[(size_t)row * env.width + col]; }
        out->phiEmpty[(size_t)row] = buildCdf(&luminance[(size_t)row * env.width], (size_t)env.width, &out->phiCdf[(size_t)row * env.width]) ? 1 : 0;
        thetaData[(size_t)row] = thetaSum;
    }
    out->thetaEmpty = buildCdf(thetaData.data(), (size_t)env.height, out->thetaCdf.data()) ? 1 : 0;
    out->thetaGuide.resize((size_t)env.height + 1);
    buildGuide(out->thetaCdf.data(), (size_t)env.height, out->thetaGuide.data());
    out->phiGuide.resize((size_t)env.height * ((size_t)env.width + 1));
    for (int row = 0; row < env.height; row++) {
        buildGuide(&out->phiCdf[(size_t)row * env.width], (size_t)env.width, &out->phiGuide[(size_t)row * (env.width + 1)]);
    }
    out->thetaRecords.resize(8 * ((size_t)env.height + 1));
    buildRecords(out->thetaCdf.data(), out->thetaGuide.data(), (size_t)env.height, out->thetaEmpty != 0, out->thetaRecords.data());
    out->phiRecords.resize(8 * (size_t)env.height * ((size_t)env.width + 1));
    for (int row = 0; row < env.height; row++) {
        buildRecords(&out->phiCdf[(size_t)row * env.width], &out->phiGuide[(size_t)row * (env.width + 1)], (size_t)env.width,
                     out->phiEmpty[(size_t)row] != 0, &out->phiRecords[8 * (size_t)row * ((size_t)env.width + 1)]);
    }
    out->width = env.width;
    out->height = env.height;
    out->scale = env.scale;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) {
            out->mapToWorld[3 * r + c] = env.map_to_world[4 * r + c];
            out->worldToMap[3 * r + c] = env.world_to_map[4 * r + c];
        }
    }
}

// ---- participating media

struct MediaTables {
    std::vector<float> sigma;      // per medium: sigma_t.rgb, sigma_s.rgb
    std::vector<int> primMedium;   // per primitive (triangles, then spheres): its surface's internal medium (Surface::getInternalMedium), -1 none
    bool hasContainers = false;    // some material is a passthrough: a surface that only bounds a medium
};

inline MediaTables buildMediaTables(const PathedSceneDesc *desc)
{
    MediaTables out;
    out.sigma.resize((size_t)6 * desc->n_media);
    for (uint32_t i = 0; i < desc->n_media; i++) {
        for (int k = 0; k < 3; k++) { out.sigma[6 * i + k] = desc->media[i].sigma_t[k]; out.sigma[6 * i + 3 + k] = desc->media[i].sigma_s[k]; }
    }
    out.primMedium.assign((size_t)desc->n_triangles + desc->n_spheres, -1);
    for (uint32_t g = 0; g < desc->n_geoms; g++) {
        const PathedGeom &geom = desc->geoms[g];
        // (a medium with sigma_t = 0 stays a medium: its surface is still a container the volumetric queries skip; its
        // distance sample -log(1 - xi) / 0 is +inf, "no event", as in the reference)
        const int medium = geom.medium;
        if (geom.type == PATHED_GEOM_MESH) {
            for (int i = 0; i < geom.count; i++) { out.primMedium[(size_t)(geom.first + i)] = medium; }
        } else {
            out.primMedium[(size_t)desc->n_triangles + (size_t)geom.first] = medium;
        }
    }
    for (uint32_t i = 0; i < desc->n_materials; i++) { out.hasContainers = out.hasContainers || desc->materials[i].type == PATHED_MAT_PASSTHROUGH; }
    return out;
}

// ---- plain ranges (device_scene.h): meshes all of whose vertices carry zero normals and zero uvs, e.g. an OBJ without vn / vt
// or a PLY of positions.  Whole meshes, merged when adjacent; a scene with more ranges than `capacity` keeps the first ones.
inline int plainRanges(const PathedSceneDesc *desc, int capacity, int *begin, int *end)
{
    int count = 0;
    for (uint32_t g = 0; g < desc->n_geoms; g++) {
        const PathedGeom &geom = desc->geoms[g];
        if (geom.type != PATHED_GEOM_MESH || geom.count <= 0) { continue; }
        bool plain = true;
        for (int i = 0; i < geom.count && plain; i++) {
            for (int k = 0; k < 3 && plain; k++) {
                const size_t v = desc->indices[3 * (size_t)(geom.first + i) + k];
                plain = desc->normals[3 * v] == 0.f && desc->normals[3 * v + 1] == 0.f && desc->normals[3 * v + 2] == 0.f
                    && desc->uvs[2 * v] == 0.f && desc->uvs[2 * v + 1] == 0.f;
            }
        }
        if (!plain) { continue; }
        if (count > 0 && end[count - 1] == geom.first) { end[count - 1] = geom.first + geom.count; }
        else if (count < capacity) {
            begin[count] = geom.first;
            end[count] = geom.first + geom.count;
            count++;
        }
    }
    return count;
}

// ---- the all-triangles kernels' inputs

// kernels.h: SmallTris -- pairs of leaf-ordered triangles (12 floats each: (v0, prim) (e1, -) (e2, -)), component-interleaved:
// word 3 * row + axis of pair k / 2 holds the two triangles' values side by side.  `pairs` is zeroed by the caller: the odd
// one out is paired with an all-zero triangle, masked off in the kernel.
inline void packSmallTris(const float *leafTris, int nTris, int pairWords, float *pairs)
{
    for (int k = 0; k < nTris; k++) {
        const float *tri = leafTris + (size_t)12 * k;
        float *record = pairs + (size_t)2 * pairWords * (k / 2);
        for (int row = 0; row < 3; row++) {
            for (int axis = 0; axis < 3; axis++) { record[2 * (3 * row + axis) + (k & 1)] = tri[4 * row + axis]; }
        }
    }
}

// small_items.h: SmallLights, and where else than the camera a ray may start
struct SmallLightInputs {
    std::vector<float> extraPoints;             // two opposite corners of every sphere's (padded) box
    std::vector<unsigned char> emitterPrims;    // per original primitive id: the triangle is a light
    std::vector<float> sphereLights;            // centre.xyz, radius of every sphere light, twice: about center_sample, then center_world
};

inline SmallLightInputs smallLightInputs(const PathedSceneDesc *desc, const std::vector<LightEntry> &lights)
{
    SmallLightInputs out;
    for (uint32_t i = 0; i < desc->n_spheres; i++) {
        for (int sign = -1; sign <= 1; sign += 2) {
            for (int a = 0; a < 3; a++) { out.extraPoints.push_back(desc->spheres[i].center_world[a] + sign * std::fabs(desc->spheres[i].radius) * 1.001f); }
        }
    }
    out.emitterPrims.assign((size_t)desc->n_triangles, 0);
    for (const LightEntry &light : lights) {
        if (light.kind == 0 && light.index >= 0 && (size_t)light.index < out.emitterPrims.size()) { out.emitterPrims[(size_t)light.index] = 1; }
        if (light.kind == 1) {
            // sampleLightsTerm samples the light about DSphere::centerSample, the intersector meets it about center_world: the
            // rule is given both, so neither has to be told from the other
            for (int a = 0; a < 3; a++) { out.sphereLights.push_back(desc->spheres[light.index].center_sample[a]); }
            out.sphereLights.push_back(desc->spheres[light.index].radius);
            for (int a = 0; a < 3; a++) { out.sphereLights.push_back(desc->spheres[light.index].center_world[a]); }
            out.sphereLights.push_back(desc->spheres[light.index].radius);
        }
    }
    return out;
}

// ---- the large-triangle split (the wavefront's local set and the hybrid kernel's direct set)

struct TriangleAreas {
    std::vector<double> area;
    double total = 0.0;   // summed in index order
    // "large": at least 1 / 256 of the scene's surface -- a floor, a wall, what no box around it would cull
    bool large(uint32_t i) const { return area[i] * 256.0 >= total; }
};

inline TriangleAreas triangleAreas(const PathedSceneDesc *desc)
{
    const uint32_t n = desc->n_triangles;
    TriangleAreas out;
    out.area.resize(n);
    for (uint32_t i = 0; i < n; i++) {
        const float *a = desc->positions + 3 * (size_t)desc->indices[3 * i], *b = desc->positions + 3 * (size_t)desc->indices[3 * i + 1], *c = desc->positions + 3 * (size_t)desc->indices[3 * i + 2];
        const double e1[3] = { (double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2] }, e2[3] = { (double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2] };
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        out.area[i] = 0.5 * std::sqrt(cx * cx + cy * cy + cz * cz);
        out.total += out.area[i];
    }
    return out;
}

// The bounds of "the rest" (the vertices `indices` name, at least one): a box and a bounding sphere about the box's centre
// (not the smallest one: the vertex farthest from that centre decides), both padded -- the tests that use them only cull.
struct RestProxy {
    float lo[3], hi[3];
    float sphere[4];   // centre, radius^2
};

inline RestProxy restProxy(const float *positions, const std::vector<uint32_t> &indices)
{
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    for (uint32_t index : indices) {
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], (double)positions[3 * (size_t)index + a]); hi[a] = std::max(hi[a], (double)positions[3 * (size_t)index + a]); }
    }
    double extent = 0.0;
    for (int a = 0; a < 3; a++) { extent = std::max(extent, std::max(hi[a] - lo[a], std::max(std::fabs(lo[a]), std::fabs(hi[a])))); }
    double centre[3], radius2 = 0.0;
    for (int a = 0; a < 3; a++) { centre[a] = (double)(float)(0.5 * (lo[a] + hi[a])); }
    for (uint32_t index : indices) {
        double d2 = 0.0;
        for (int a = 0; a < 3; a++) { const double d = (double)positions[3 * (size_t)index + a] - centre[a]; d2 += d * d; }
        radius2 = std::max(radius2, d2);
    }
    const double radius = std::sqrt(radius2) * 1.0001 + 1e-4 * extent + 1e-30;
    RestProxy out;
    for (int a = 0; a < 3; a++) {
        out.lo[a] = (float)(lo[a] - 1e-4 * extent - 1e-30);
        out.hi[a] = (float)(hi[a] + 1e-4 * extent + 1e-30);
        out.sphere[a] = (float)centre[a];
    }
    out.sphere[3] = (float)(radius * radius * 1.00001);
    return out;
}

}  // namespace pathed
