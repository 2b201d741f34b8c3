// The host stages of scene creation (pathed_amd/csrc/scene_tables.h) without a GPU: tests/test_scene_tables_host.py builds this
// program plainly and under the address and undefined-behaviour sanitizers and runs it.  Prints "failures 0" when all holds.
#include "scene_tables.h"

#include <cstdio>
#include <functional>
#include <random>

using namespace pathed;

static int g_failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            g_failures++;                                                        \
            if (g_failures <= 40) { printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                        \
    } while (0)

// ---- a scene description that owns its arrays
struct Built {
    std::vector<float> positions, normals, uvs;
    std::vector<uint32_t> indices;
    std::vector<int32_t> triMaterial;
    std::vector<PathedSphere> spheres;
    std::vector<PathedGeom> geoms;
    std::vector<PathedMaterial> materials;
    std::vector<PathedMedium> media;
    std::vector<PathedTexture> textures;
    PathedEnvLight env;
    bool hasEnv = false;
    PathedSceneDesc desc;

    int material(int type, float emit = 0.f)
    {
        PathedMaterial m;
        std::memset(&m, 0, sizeof m);
        m.type = type;
        m.emit[0] = emit;
        materials.push_back(m);
        return (int)materials.size() - 1;
    }
    // one mesh of `count` triangles with vertices of their own; material per triangle from `pick`
    void mesh(int count, const std::function<int(int)> &pick, int medium = -1, float normal = 0.f, float uv = 0.f)
    {
        geoms.push_back({ PATHED_GEOM_MESH, (int32_t)triMaterial.size(), count, medium });
        for (int i = 0; i < count; i++) {
            for (int k = 0; k < 3; k++) {
                indices.push_back((uint32_t)(positions.size() / 3));
                for (int a = 0; a < 3; a++) { positions.push_back((float)(i + (k == a ? 1 : 0))); normals.push_back(0.f); }
                uvs.push_back(0.f); uvs.push_back(0.f);
            }
            triMaterial.push_back(pick(i));
        }
        if (count > 0 && normal != 0.f) { normals[normals.size() - 2] = normal; }   // one vertex of the last triangle
        if (count > 0 && uv != 0.f) { uvs[uvs.size() - 1] = uv; }
    }
    void sphere(int material, int medium = -1)
    {
        PathedSphere s;
        std::memset(&s, 0, sizeof s);
        const float n = (float)spheres.size();
        for (int a = 0; a < 3; a++) { s.center_world[a] = n + 0.25f * a; s.center_sample[a] = s.center_world[a]; }
        s.radius = 0.5f + n;
        s.material = material;
        geoms.push_back({ PATHED_GEOM_SPHERE, (int32_t)spheres.size(), 1, medium });
        spheres.push_back(s);
    }
    const PathedSceneDesc *finish()
    {
        std::memset(&desc, 0, sizeof desc);
        desc.n_vertices = (uint32_t)(positions.size() / 3);
        desc.positions = positions.data(); desc.normals = normals.data(); desc.uvs = uvs.data();
        desc.n_triangles = (uint32_t)triMaterial.size();
        desc.indices = indices.data(); desc.tri_material = triMaterial.data();
        desc.n_spheres = (uint32_t)spheres.size(); desc.spheres = spheres.data();
        desc.n_geoms = (uint32_t)geoms.size(); desc.geoms = geoms.data();
        desc.n_materials = (uint32_t)materials.size(); desc.materials = materials.data();
        desc.n_media = (uint32_t)media.size(); desc.media = media.data();
        desc.n_textures = (uint32_t)textures.size(); desc.textures = textures.data();
        desc.env = hasEnv ? &env : nullptr;
        return &desc;
    }
};

static std::vector<unsigned char> emitFlags(const Built &built)
{
    std::vector<unsigned char> flags;
    for (const PathedMaterial &m : built.materials) { flags.push_back(m.type == PATHED_MAT_LAMBERTIAN && m.emit[0] != 0.f); }
    return flags;
}

// ---- options: for every field the last accepted and the first refused value on both ends, and the exact message
static PathedSceneOptions defaults()
{
    PathedSceneOptions options;
    std::memset(&options, 0, sizeof options);
    options.struct_size = sizeof options;
    options.device = PATHED_DEVICE_CURRENT;
    return options;
}

struct OptionCase {
    const char *name;
    int32_t PathedSceneOptions::*field;
    std::vector<int> accepted, refused;
    const char *message;   // copied from the source the checks came from
};

static void testOptions()
{
    const std::vector<OptionCase> cases = {
        { "generic_kernels", &PathedSceneOptions::generic_kernels, { 0, 1 }, { -1, 2 }, "generic_kernels must be 0 or 1" },
        { "node_format", &PathedSceneOptions::node_format, { 0, 3 }, { -1, 4 }, "node_format must be 0 (automatic), 1 (128-byte float nodes), 2 (compressed 64-byte nodes) or 3 (compressed 8-wide nodes)" },
        { "build_threads", &PathedSceneOptions::build_threads, { 0, 4096 }, { -1, 4097 }, "build_threads must be 0..4096" },
        { "unit_order", &PathedSceneOptions::unit_order, { 0, 3 }, { -1, 4 }, "unit_order must be 0..3" },
        { "bvh_builder", &PathedSceneOptions::bvh_builder, { 0, 3 }, { -1, 4 }, "unknown BVH builder" },
        { "pools", &PathedSceneOptions::pools, { 0, 4 }, { -1, 5 }, "pools must be 0..4" },
        { "stack_rows", &PathedSceneOptions::stack_rows, { 0, 8, 16, 22 }, { -1, 7, 9, 15, 17, 21, 23 }, "stack_rows must be 0, 8, 16 or 22" },
        { "max_slots", &PathedSceneOptions::max_slots, { 0, 256, 1 << 30 }, { -1, 1, 255 }, "max_slots must be 0 or >= 256" },
        { "shade_kernel", &PathedSceneOptions::shade_kernel, { 0, 6 }, { -1, 7 }, "shade_kernel must be 0..6" },
        { "stage_slots", &PathedSceneOptions::stage_slots, { 0, 512, 1024 }, { -1, 511, 513, 1023, 1025 }, "stage_slots must be 0, 512 or 1024" },
        { "refittable", &PathedSceneOptions::refittable, { 0, 1 }, { -1, 2 }, "refittable must be 0 or 1" },
        { "small_phase1", &PathedSceneOptions::small_phase1, { 0, 2 }, { -1, 3 }, "small_phase1 must be 0 (automatic), 1 (VALU) or 2 (matrix pipe)" },
        { "wave_max_ksamples", &PathedSceneOptions::wave_max_ksamples, { 0, 0x7FFFFFFF }, { -1 }, "wave_max_ksamples must be >= 0" },
        { "wave_stragglers", &PathedSceneOptions::wave_stragglers, { -1, 64 }, { -2, 65 }, "wave_stragglers must be -1 (none), 0 (default) or 1..64" },
        { "wave_refill", &PathedSceneOptions::wave_refill, { 0, 64 }, { -1, 65 }, "wave_refill must be 0 (default) or 1..64" },
        { "chunks_per_pass", &PathedSceneOptions::chunks_per_pass, { 0, 4096 }, { -1, 4097 }, "chunks_per_pass must be 0 (default) or 1..4096" },
        { "shade_chain", &PathedSceneOptions::shade_chain, { 0, 1 }, { -1, 2 }, "shade_chain must be 0 (automatic) or 1 (off)" },
        { "shade_launches", &PathedSceneOptions::shade_launches, { 0, 16 }, { -1, 17 }, "shade_launches must be 0 (automatic) or 1..16" },
        { "local_rays", &PathedSceneOptions::local_rays, { 0, 1 }, { -1, 2 }, "local_rays must be 0 (automatic) or 1 (off)" },
        { "hybrid_batch", &PathedSceneOptions::hybrid_batch, { 0, 128 }, { -1, 129 }, "hybrid_batch must be 0 (default) or 1..128" },
        { "hybrid_ready", &PathedSceneOptions::hybrid_ready, { -1, 64 }, { -2, 65 }, "hybrid_ready must be -1 (never), 0 (default) or 1..64" },
    };
    std::string message = "untouched";
    CHECK(checkSceneOptions(defaults(), &message) == PATHED_OK && message == "untouched", "defaults: %s", message.c_str());
    PathedSceneOptions sized = defaults();
    sized.struct_size -= 4;
    sized.generic_kernels = 7;
    CHECK(checkSceneOptions(sized, &message) == PATHED_E_INVALID && message == "PathedSceneOptions.struct_size mismatch", "%s", message.c_str());
    for (size_t c = 0; c < cases.size(); c++) {
        for (int value : cases[c].accepted) {
            PathedSceneOptions options = defaults();
            options.*(cases[c].field) = value;
            message = "untouched";
            CHECK(checkSceneOptions(options, &message) == PATHED_OK && message == "untouched", "%s = %d: %s", cases[c].name, value, message.c_str());
        }
        for (int value : cases[c].refused) {
            PathedSceneOptions options = defaults();
            options.*(cases[c].field) = value;
            message.clear();
            CHECK(checkSceneOptions(options, &message) == PATHED_E_INVALID && message == cases[c].message, "%s = %d: %s", cases[c].name, value, message.c_str());
            // two fields wrong: the one checked first wins (the order of `cases` is the order of the checks)
            for (size_t later = c + 1; later < cases.size(); later++) {
                PathedSceneOptions both = options;
                both.*(cases[later].field) = cases[later].refused[0];
                message.clear();
                CHECK(checkSceneOptions(both, &message) == PATHED_E_INVALID && message == cases[c].message, "%s and %s: %s", cases[c].name, cases[later].name, message.c_str());
            }
        }
    }
}

// ---- environment tables
static int linearSearch(const float *cdf, int size, float u)
{
    for (int i = 0; i < size; i++) { if (cdf[i] >= u) { return i; } }
    return size - 1;
}

static void checkDistribution(const char *what, const float *cdf, const int *guide, const float *records, int size, bool empty, bool expectEmpty, std::mt19937 &rng)
{
    CHECK(empty == expectEmpty, "%s: empty flag %d", what, (int)empty);
    for (int i = 0; i < size; i++) {
        CHECK(i == 0 || cdf[i] >= cdf[i - 1], "%s: cdf decreases at %d", what, i);
        if (empty) { CHECK(cdf[i] == 0.f, "%s: empty cdf holds %g", what, cdf[i]); }
    }
    if (!empty) { CHECK(cdf[size - 1] == 1.f, "%s: cdf ends at %g", what, cdf[size - 1]); }
    for (int j = 0; j <= size; j++) {
        CHECK(guide[j] == linearSearch(cdf, size, (float)j / (float)size), "%s: guide[%d] = %d", what, j, guide[j]);
    }
    std::uniform_real_distribution<float> uniform(0.f, 1.f);
    for (int bucket = 0; bucket <= size; bucket++) {
        int lo, hi;
        std::memcpy(&lo, records + 8 * bucket, 4);
        std::memcpy(&hi, records + 8 * bucket + 1, 4);
        CHECK((lo == -1) == empty, "%s: record %d starts at %d, empty %d", what, bucket, lo, (int)empty);
        if (empty) { continue; }
        const int below = bucket == 0 ? 0 : bucket - 1, above = bucket + 2 > size ? size : bucket + 2;
        CHECK(lo == guide[below] && hi == guide[above], "%s: record %d window [%d, %d]", what, bucket, lo, hi);
        const auto at = [&](int i) { return cdf[i < 0 ? 0 : i > size - 1 ? size - 1 : i]; };
        CHECK(records[8 * bucket + 2] == (lo > 0 ? at(lo - 1) : 0.f) && records[8 * bucket + 3] == at(lo) && records[8 * bucket + 4] == at(lo + 1)
              && records[8 * bucket + 5] == at(lo + 2), "%s: record %d cdf values", what, bucket);
    }
    if (empty) { return; }
    for (int k = 0; k < 1000; k++) {
        // the cell the device derives from u (shading.h: cdfSampleRecord): bucket = min(size, (int)(u * size))
        const float u = k == 0 ? 0.f : k == 1 ? 1.f : uniform(rng);
        int bucket = (int)(u * (float)size);
        bucket = bucket > size ? size : bucket;
        int lo, hi;
        std::memcpy(&lo, records + 8 * bucket, 4);
        std::memcpy(&hi, records + 8 * bucket + 1, 4);
        const int found = linearSearch(cdf, size, u);
        CHECK(lo <= found && found <= hi, "%s: u = %.9g lands on %d outside [%d, %d]", what, u, found, lo, hi);
    }
}

static void testEnvTables()
{
    std::mt19937 rng(7);
    std::uniform_real_distribution<float> uniform(0.01f, 2.f);
    const int sizes[4][2] = { { 1, 1 }, { 2, 1 }, { 3, 2 }, { 8, 4 } };
    enum { kBlackRow, kBlackMap, kBrightTexel, kEqual, kVariants };
    for (const auto &size : sizes) {
        for (int variant = 0; variant < kVariants; variant++) {
            const int width = size[0], height = size[1];
            std::vector<float> rgba((size_t)4 * width * height);
            for (float &value : rgba) { value = variant == kEqual ? 0.5f : uniform(rng); }
            const int blackRow = height - 1;
            for (int row = 0; row < height; row++) {
                for (int col = 0; col < width; col++) {
                    float *texel = &rgba[4 * ((size_t)row * width + col)];
                    if (variant == kBlackMap || (variant == kBlackRow && row == blackRow)) { texel[0] = texel[1] = texel[2] = 0.f; }   // (alpha stays: it is no weight)
                    if (variant == kBrightTexel && row == height / 2 && col == width / 2) { texel[0] = texel[1] = texel[2] = 1e4f; }
                }
            }
            PathedEnvLight env;
            std::memset(&env, 0, sizeof env);
            env.width = width; env.height = height; env.rgba = rgba.data(); env.scale = 2.5f;
            for (int i = 0; i < 16; i++) { env.map_to_world[i] = (float)(i + 1); env.world_to_map[i] = (float)(-i - 1); }
            EnvTables tables;
            buildEnvTables(env, &tables);
            char what[96];
            snprintf(what, sizeof what, "%dx%d variant %d theta", width, height, variant);
            CHECK(tables.width == width && tables.height == height && tables.scale == 2.5f, "%s: header", what);
            CHECK(tables.rgba == rgba, "%s: rgba", what);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) {
                    CHECK(tables.mapToWorld[3 * r + c] == env.map_to_world[4 * r + c] && tables.worldToMap[3 * r + c] == env.world_to_map[4 * r + c], "%s: matrices", what);
                }
            }
            CHECK(tables.thetaCdf.size() == (size_t)height && tables.phiCdf.size() == (size_t)width * height && tables.phiEmpty.size() == (size_t)height
                  && tables.thetaGuide.size() == (size_t)height + 1 && tables.phiGuide.size() == (size_t)height * (width + 1)
                  && tables.thetaRecords.size() == 8 * ((size_t)height + 1) && tables.phiRecords.size() == 8 * (size_t)height * (width + 1), "%s: sizes", what);
            const bool allBlack = variant == kBlackMap || (variant == kBlackRow && height == 1);
            checkDistribution(what, tables.thetaCdf.data(), tables.thetaGuide.data(), tables.thetaRecords.data(), height, tables.thetaEmpty != 0, allBlack, rng);
            for (int row = 0; row < height; row++) {
                snprintf(what, sizeof what, "%dx%d variant %d phi row %d", width, height, variant, row);
                const bool black = variant == kBlackMap || (variant == kBlackRow && row == blackRow);
                checkDistribution(what, &tables.phiCdf[(size_t)row * width], &tables.phiGuide[(size_t)row * (width + 1)], &tables.phiRecords[8 * (size_t)row * (width + 1)],
                                  width, tables.phiEmpty[(size_t)row] != 0, black, rng);
            }
        }
    }
}

// ---- lights, plain ranges, media, small-scene inputs
static void testLightList()
{
    Built built;
    const int dark = built.material(PATHED_MAT_LAMBERTIAN), bright = built.material(PATHED_MAT_LAMBERTIAN, 3.f);
    const int mirror = built.material(PATHED_MAT_MIRROR, 5.f);   // emission on anything but a Lambertian is dropped
    built.mesh(5, [&](int i) { return i % 2 ? bright : dark; });          // triangles 1, 3
    built.sphere(bright);                                                  // sphere 0
    built.mesh(3, [&](int i) { return i == 0 ? bright : mirror; });       // triangle 5
    built.sphere(dark);
    built.sphere(bright);                                                  // sphere 2
    built.mesh(1, [&](int) { return bright; });                            // triangle 8
    std::memset(&built.env, 0, sizeof built.env);
    built.hasEnv = true;
    const std::vector<LightEntry> lights = listLights(built.finish(), emitFlags(built));
    const int expected[][2] = { { 0, 1 }, { 0, 3 }, { 1, 0 }, { 0, 5 }, { 1, 2 }, { 0, 8 }, { 2, 0 } };
    CHECK(lights.size() == 7, "light count %zu", lights.size());
    for (size_t i = 0; i < lights.size() && i < 7; i++) {
        CHECK(lights[i].kind == expected[i][0] && lights[i].index == expected[i][1], "light %zu = (%d, %d)", i, lights[i].kind, lights[i].index);
    }
    built.hasEnv = false;
    CHECK(listLights(built.finish(), emitFlags(built)).size() == 6, "without the environment");

    // both centres of a sphere light, center_sample first; the extra points are the corners of every sphere's padded box
    built.spheres[2].center_sample[1] = -9.f;
    const SmallLightInputs inputs = smallLightInputs(built.finish(), listLights(built.finish(), emitFlags(built)));
    CHECK(inputs.sphereLights.size() == 16, "sphere light floats %zu", inputs.sphereLights.size());
    if (inputs.sphereLights.size() == 16) {
        const PathedSphere &moved = built.spheres[2];
        const float *record = &inputs.sphereLights[8];
        CHECK(record[0] == moved.center_sample[0] && record[1] == -9.f && record[2] == moved.center_sample[2] && record[3] == moved.radius, "centre of sampling first");
        CHECK(record[4] == moved.center_world[0] && record[5] == moved.center_world[1] && record[6] == moved.center_world[2] && record[7] == moved.radius, "centre of intersection second");
        CHECK(record[5] != record[1], "the two centres differ");
    }
    CHECK(inputs.extraPoints.size() == 18, "extra points %zu", inputs.extraPoints.size());
    for (size_t s = 0; s < built.spheres.size() && inputs.extraPoints.size() == 18; s++) {
        for (int a = 0; a < 3; a++) {
            const float pad = std::fabs(built.spheres[s].radius) * 1.001f;
            CHECK(inputs.extraPoints[6 * s + a] == built.spheres[s].center_world[a] + -1 * pad && inputs.extraPoints[6 * s + 3 + a] == built.spheres[s].center_world[a] + 1 * pad, "corners of sphere %zu", s);
        }
    }
    std::vector<unsigned char> emitters(9, 0);
    for (int tri : { 1, 3, 5, 8 }) { emitters[(size_t)tri] = 1; }
    CHECK(inputs.emitterPrims == emitters, "emitter flags");

    float pairs[8][4][2];
    packSpherePairs(built.finish(), pairs);
    for (int i = 0; i < 16; i++) {
        if (i < 3) {
            for (int k = 0; k < 3; k++) { CHECK(pairs[i / 2][k][i % 2] == built.spheres[(size_t)i].center_world[k], "sphere pair %d", i); }
            CHECK(pairs[i / 2][3][i % 2] == built.spheres[(size_t)i].radius * built.spheres[(size_t)i].radius, "sphere pair radius %d", i);
        } else {
            CHECK(pairs[i / 2][3][i % 2] == -1.f && pairs[i / 2][0][i % 2] == 0.f, "empty half %d", i);
        }
    }
}

static void testPlainRanges()
{
    Built built;
    const int grey = built.material(PATHED_MAT_LAMBERTIAN);
    const auto pick = [&](int) { return grey; };
    built.mesh(4, pick);                 // [0, 4)
    built.mesh(0, pick);                 // skipped: does not break adjacency either
    built.mesh(3, pick);                 // merges: [0, 7)
    built.mesh(2, pick, -1, 0.5f);       // one non-zero normal: not plain
    built.mesh(2, pick);                 // [9, 11)
    built.mesh(2, pick, -1, 0.f, 0.25f); // one non-zero uv: not plain
    built.sphere(grey);
    int begin[8], end[8];
    CHECK(plainRanges(built.finish(), 8, begin, end) == 2 && begin[0] == 0 && end[0] == 7 && begin[1] == 9 && end[1] == 11, "merge, skip, normals and uvs");
    // nine separated plain meshes: the ninth is dropped; a mesh adjacent to the eighth still merges into it
    Built many;
    many.material(PATHED_MAT_LAMBERTIAN);
    for (int k = 0; k < 9; k++) {
        many.mesh(2, [](int) { return 0; });
        if (k == 7) { many.mesh(1, [](int) { return 0; }); }
        many.mesh(1, [](int) { return 0; }, -1, 1.f);
    }
    std::fill(begin, begin + 8, -7);
    const int count = plainRanges(many.finish(), 8, begin, end);
    CHECK(count == 8, "ranges kept %d", count);
    for (int k = 0; k < 8; k++) { CHECK(begin[k] == 3 * k && end[k] == 3 * k + (k == 7 ? 3 : 2), "range %d = [%d, %d)", k, begin[k], end[k]); }
}

static void testMedia()
{
    Built built;
    const int grey = built.material(PATHED_MAT_LAMBERTIAN);
    built.media.push_back({ { 1.f, 2.f, 3.f }, { 0.1f, 0.2f, 0.3f } });
    built.media.push_back({ { 0.f, 0.f, 0.f }, { 0.f, 0.f, 0.f } });
    built.mesh(3, [&](int) { return grey; });
    built.sphere(grey);
    built.mesh(2, [&](int) { return grey; }, 1);
    built.sphere(grey, 0);
    MediaTables tables = buildMediaTables(built.finish());
    const std::vector<float> sigma = { 1.f, 2.f, 3.f, 0.1f, 0.2f, 0.3f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f };
    CHECK(tables.sigma == sigma, "sigma records");
    const std::vector<int> primMedium = { -1, -1, -1, 1, 1, /* spheres at n_triangles + first */ -1, 0 };
    CHECK(tables.primMedium == primMedium, "primMedium");
    CHECK(!tables.hasContainers, "no passthrough material yet");
    built.material(PATHED_MAT_PASSTHROUGH);
    CHECK(buildMediaTables(built.finish()).hasContainers, "a passthrough material makes containers");
}

static void testTexelsAndSmallTris()
{
    Built built;
    built.material(PATHED_MAT_LAMBERTIAN);
    const uint8_t first[2 * 1 * 3] = { 0, 255, 128, 1, 2, 3 }, second[1 * 1 * 3] = { 254, 64, 0 };
    built.textures.push_back({ 2, 1, first });
    built.textures.push_back({ 1, 1, second });
    std::vector<float> texels;
    std::vector<size_t> offsets;
    gammaTexels(built.finish(), &texels, &offsets);
    CHECK(offsets.size() == 2 && offsets[0] == 0 && offsets[1] == 2 && texels.size() == 12, "texel layout");
    const uint8_t all[9] = { 0, 255, 128, 1, 2, 3, 254, 64, 0 };
    for (int k = 0; k < 3 && texels.size() == 12; k++) {
        for (int c = 0; c < 3; c++) { CHECK(texels[4 * k + c] == powf(all[3 * k + c] / 255.f, 2.2f), "texel %d channel %d", k, c); }
        CHECK(texels[4 * k + 3] == 0.f, "texel %d w", k);
    }
    CHECK(texels[0] == 0.f && texels[1] == 1.f, "gamma end points");

    float leaf[3 * 12], pairs[2 * 2 * 9] = {};
    for (int i = 0; i < 36; i++) { leaf[i] = (float)(100 + i); }
    packSmallTris(leaf, 3, 9, pairs);
    for (int k = 0; k < 4; k++) {
        for (int row = 0; row < 3; row++) {
            for (int axis = 0; axis < 3; axis++) {
                CHECK(pairs[2 * (9 * (k / 2) + 3 * row + axis) + (k & 1)] == (k < 3 ? leaf[12 * k + 4 * row + axis] : 0.f), "small pair word of triangle %d", k);
            }
        }
    }
}

// ---- the large-triangle split
static void testSplit()
{
    std::mt19937 rng(2024);
    std::uniform_real_distribution<float> coordinate(-50.f, 50.f), scale(-3.f, 1.f);
    for (int round = 0; round < 200; round++) {
        std::uniform_int_distribution<int> countOf(2, 300);
        const int n = round == 0 ? 2 : round == 1 ? 300 : countOf(rng);
        const int kind = round % 4;   // 0 random, 1 with degenerate triangles, 2 all-equal areas, 3 one triangle of 99 % of the area
        Built built;
        built.material(PATHED_MAT_LAMBERTIAN);
        built.mesh(n, [](int) { return 0; });
        for (int i = 0; i < n; i++) {
            float *corners = &built.positions[(size_t)9 * i];
            const float size = kind == 2 ? 1.f : std::pow(10.f, scale(rng));
            float origin[3] = { coordinate(rng), coordinate(rng), coordinate(rng) };
            if (kind == 2) { for (float &value : origin) { value = std::round(value); } }   // exact unit edges: the areas are equal to the bit
            for (int k = 0; k < 3; k++) {
                for (int a = 0; a < 3; a++) { corners[3 * k + a] = kind == 2 ? origin[a] + (k == a ? 1.f : 0.f) : origin[a] + size * coordinate(rng) * 0.02f; }
            }
            if (kind == 1 && i % 3 == 0) { for (int a = 0; a < 3; a++) { corners[6 + a] = corners[3 + a]; } }   // zero area
        }
        if (kind == 3) {
            // a right triangle of legs L: area L^2 / 2 = 99 x the rest
            const PathedSceneDesc *before = built.finish();
            double rest = triangleAreas(before).total;
            { const float *a = &built.positions[0], *b = a + 3, *c = a + 6;
              const double e1[3] = { (double)b[0] - a[0], (double)b[1] - a[1], (double)b[2] - a[2] }, e2[3] = { (double)c[0] - a[0], (double)c[1] - a[1], (double)c[2] - a[2] };
              const double x = e1[1] * e2[2] - e1[2] * e2[1], y = e1[2] * e2[0] - e1[0] * e2[2], z = e1[0] * e2[1] - e1[1] * e2[0];
              rest -= 0.5 * std::sqrt(x * x + y * y + z * z); }
            const float leg = (float)std::sqrt(2.0 * 99.0 * rest);
            const float big[9] = { 0.f, 0.f, 0.f, leg, 0.f, 0.f, 0.f, leg, 0.f };
            std::memcpy(&built.positions[0], big, sizeof big);
        }
        const PathedSceneDesc *desc = built.finish();
        const TriangleAreas areas = triangleAreas(desc);
        // the straightforward recomputation
        double total = 0.0;
        std::vector<uint32_t> rest;
        size_t nLarge = 0;
        for (int i = 0; i < n; i++) {
            const float *a = &built.positions[(size_t)9 * i], *b = a + 3, *c = a + 6;
            const double ux = (double)b[0] - (double)a[0], uy = (double)b[1] - (double)a[1], uz = (double)b[2] - (double)a[2];
            const double vx = (double)c[0] - (double)a[0], vy = (double)c[1] - (double)a[1], vz = (double)c[2] - (double)a[2];
            const double nx = uy * vz - uz * vy, ny = uz * vx - ux * vz, nz = ux * vy - uy * vx;
            const double area = 0.5 * std::sqrt(nx * nx + ny * ny + nz * nz);
            total += area;
            CHECK(areas.area[(size_t)i] == area, "round %d: area of %d is %.17g, not %.17g", round, i, areas.area[(size_t)i], area);
            if (kind == 1 && i % 3 == 0) { CHECK(area == 0.0, "round %d: degenerate triangle %d has area %g", round, i, area); }
        }
        CHECK(areas.total == total, "round %d: total %.17g, not %.17g", round, areas.total, total);
        for (int i = 0; i < n; i++) {
            const bool large = areas.area[(size_t)i] * 256.0 >= total;
            CHECK(areas.large((uint32_t)i) == large, "round %d: large(%d)", round, i);
            if (large) { nLarge++; continue; }
            for (int k = 0; k < 3; k++) { rest.push_back(desc->indices[3 * i + k]); }
        }
        // (n equal areas: large while 256 a >= n a; at n = 256 the rounding of the sum decides, so that count is left alone)
        if (kind == 2 && n != 256) { CHECK(nLarge == (n < 256 ? (size_t)n : 0), "round %d: %zu of %d equal triangles are large", round, nLarge, n); }
        if (kind == 3) { CHECK(areas.large(0) && areas.area[0] >= 0.98 * total, "round %d: the dominant triangle holds %.4f of the area", round, areas.area[0] / total); }
        if (rest.empty()) { continue; }   // (the callers do not ask for the bounds of nothing)
        const RestProxy proxy = restProxy(desc->positions, rest);
        for (uint32_t index : rest) {
            const float *v = desc->positions + 3 * (size_t)index;
            double d2 = 0.0;
            for (int a = 0; a < 3; a++) {
                CHECK(proxy.lo[a] <= v[a] && v[a] <= proxy.hi[a], "round %d: vertex %u outside the box on axis %d", round, index, a);
                const double d = (double)v[a] - (double)proxy.sphere[a];
                d2 += d * d;
            }
            CHECK(d2 <= (double)proxy.sphere[3], "round %d: vertex %u outside the sphere (%.9g > %.9g)", round, index, d2, (double)proxy.sphere[3]);
        }
    }
}

// ---- the traversal stack's shape
static void testStackShape()
{
    for (int rows : { 8, 16, 22 }) { CHECK(stackRowsFor(rows) == rows, "rows for %d: %d", rows, stackRowsFor(rows)); }
    for (int rows : { 0, 7, 9, 23, -8 }) { CHECK(stackRowsFor(rows) == 22, "rows for %d: %d", rows, stackRowsFor(rows)); }
    const size_t row = (size_t)kOptionMinSlots * sizeof(int);   // one int per lane of a block (kBlock)
    CHECK(stackLdsBytes(8) == 9 * row && stackLdsBytes(16) == 17 * row && stackLdsBytes(22) == 23 * row, "LDS bytes %zu %zu %zu", stackLdsBytes(8), stackLdsBytes(16), stackLdsBytes(22));
    const size_t threads = (size_t)1024 * 256;
    for (int rows : { 8, 16, 22 }) {
        for (int maxStack : { 0, 1, rows - 1, rows }) { CHECK(stackSpillInts(threads, maxStack, rows) == threads, "spill of %d over %d rows", maxStack, rows); }
        for (int maxStack : { rows + 1, rows + 2, 64 }) { CHECK(stackSpillInts(threads, maxStack, rows) == threads * (size_t)(maxStack - rows), "spill of %d over %d rows", maxStack, rows); }
    }
    CHECK(stackSpillInts((size_t)1 << 28, 70, 8) == ((size_t)62 << 28), "the product is taken in size_t");
}

int main()
{
    testOptions();
    testStackShape();
    testEnvTables();
    testLightList();
    testPlainRanges();
    testMedia();
    testTexelsAndSmallTris();
    testSplit();
    printf("failures %d\n", g_failures);
    return g_failures == 0 ? 0 : 1;
}
