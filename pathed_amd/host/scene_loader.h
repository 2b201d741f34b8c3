// Scene JSON / OBJ / MTL / PLY / quad / sphere readers producing the flat
// PathedSceneDesc the C ABI consumes.
//
// The reference builds an object graph whose BSDF parameters are private and whose
// per-vertex attributes live only in Embree buffers, so a drop-in
// has to read the same files itself.  Format rules followed here:
//   scene JSON   reference src/scene_parser.cpp:140-200, 251-291, 574-667, 690-850
//   OBJ          reference src/obj_parser.cpp:50-515
//   MTL          reference src/mtl_parser.cpp:40-113
//   PLY          reference src/ply_parser.cpp:29-151
//   quad         reference src/quad.cpp:7-151
//   sphere       reference src/sphere.cpp:16-48, src/scene_parser.cpp:484-512
//   textures     reference src/texture.cpp:12-31 (PNG / PNM here, see image_decode.h)
//   .vol grids   reference src/vol_parser.cpp:10-80, src/scene_parser.cpp:202-220
#pragma once

#include "pathed_hip.h"

#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace pathed {

// A "heterogeneous" medium of the scene file: the voxel grid of its .vol file (reference GridMedium).  PathedSceneDesc does not
// know grids: the slot `medium` of FlatScene::media is a placeholder, and whoever creates the device scene hands the grid
// over with pathed_hip_scene_set_grid_medium(scene, medium, gridDesc(i)) (host/integrator.cpp: Scene::upload).
struct FlatGrid {
    int medium = -1;           // index into FlatScene::media
    PathedGridMedium desc;     // desc.data is set by FlatScene::gridDesc
    std::vector<float> data;   // cells_x * cells_y * cells_z, index = (z * cells_y + y) * cells_x + x
};

// A medium's "phase" key (scene JSON, media of either kind): Henyey-Greenstein with mean cosine g on slot `medium`.  Like a
// grid it is handed over on the created scene: pathed_hip_scene_set_medium_phase(scene, medium, phaseDesc(i)).
struct FlatPhase {
    int medium = -1;           // index into FlatScene::media
    float g = 0.f;
    PathedPhaseFunction desc;  // filled in by FlatScene::phaseDesc
};

// The contents of a .vol file (vol_parser.cpp's layout: "VOL", a version byte, uint32 encoding, cells x / y / z, channels,
// six float bounds, then the cells as float32).  Throws SceneLoadError on a wrong header, a channel count other than 1, or
// a length that is not the header plus cells x 4 bytes (the reference checks none of the three).
struct VolFile {
    uint32_t cells[3];
    float bounds[6];
    std::vector<float> data;
};
VolFile readVolFile(const std::string &path);

struct FlatScene {
    PathedCamera camera;

    std::vector<float> positions;
    std::vector<float> normals;
    std::vector<float> uvs;
    std::vector<uint32_t> indices;
    std::vector<int32_t> triMaterial;

    std::vector<PathedSphere> spheres;
    std::vector<PathedGeom> geoms;
    std::vector<PathedMaterial> materials;
    std::vector<PathedMedium> media;
    std::vector<FlatGrid> grids;
    std::vector<FlatPhase> phases;

    bool hasEnv = false;
    PathedEnvLight env;
    std::vector<float> envData;

    // image textures (reference src/texture.cpp): 8-bit RGB, one entry per distinct file
    std::vector<PathedTexture> textures;
    std::vector<std::vector<uint8_t>> textureData;
    std::map<std::string, int> textureByPath;

    // Instanced geometry (scene JSON "instance" / "instanced", reference src/scene_parser.cpp:231-249, 449-492), ONE level:
    // a prototype is a run of the LAST geoms (its meshes, in its own space), a placement one prototype under a row-major
    // 3 x 4 transform.  Nesting is resolved here: an "instanced" inside an "instance" becomes, for every placement of the
    // outer prototype, a placement of the inner one under the composed transform (formed in double, rounded once to float).
    // Emissive faces of a prototype are BAKED: per placement they are ordinary world triangles (flattenInstancePoint /
    // flattenInstanceNormal below), after the scene's other world geoms, and ordinary lights.
    std::vector<PathedPrototype> prototypes;
    std::vector<std::string> prototypeNames;
    std::vector<PathedInstance> instances;
    bool instanced() const { return !prototypes.empty() || !instances.empty(); }
    // The shutter (include/pathed_hip.h: pathed_hip_scene_set_instance_motion): a top-level "instanced" model may carry
    // "transform_close", 16 numbers like "transform", its placement at shutter time 1.  When any does, instancesClose holds 12
    // floats per entry of `instances` (a placement that does not move: its transform again) and the scene is created with that
    // motion over [shutterOpen, shutterClose] -- the job key "shutter", [0, 1] by default.  Refused by name: the key on a
    // nested "instanced" model, and on a placement of a prototype that holds an emitter (baked emitters would stay behind).
    std::vector<float> instancesClose;
    float shutterOpen = 0.f, shutterClose = 1.f;
    bool moves() const { return !instancesClose.empty(); }
    PathedInstanceDesc instanceDesc() const;

    // valid as long as this FlatScene is alive and unmodified
    PathedSceneDesc desc() const;
    // grid i ready for pathed_hip_scene_set_grid_medium (same lifetime rule)
    const PathedGridMedium *gridDesc(size_t i) const;
    // phase function i ready for pathed_hip_scene_set_medium_phase
    const PathedPhaseFunction *phaseDesc(size_t i) const;
    // some medium scatters anisotropically on the device (|g| at or above the kernels' threshold, pathed_amd/csrc/volume.h)
    bool anisotropic() const;
};

struct SceneLoadError : std::runtime_error {
    explicit SceneLoadError(const std::string &what) : std::runtime_error(what) {}
};

// assetRoot plays the role of the reference's working directory after its
// chdir("..") (app/main.cpp:60): every filename inside the scene is relative to it.
FlatScene loadScene(
    const std::string &scenePath,
    int width, int height,
    const std::string &assetRoot
);

PathedMaterial makeLambertian(const float diffuse[3], const float emit[3]);

// The flatten routine of include/pathed_hip.h (PathedInstanceDesc), fp32, one rounding per operation, in the operation order
// the device applies to a prototype's shading record (pathed_amd/csrc/instances.h) and pathed_amd.flatten_instances applies in
// numpy: transform / inverse are row-major 3 x 4; instanceInverse forms the inverse in double by cofactors and rounds once,
// statement for statement as the library's own does (instances.h: instanceInverse; this side of the C ABI sees only pathed_hip.h).
void flattenInstancePoint(const float *transform, const float *point, float *out);
void flattenInstanceNormal(const float *inverse, const float *normal, float *out);
bool instanceInverse(const float *transform, float *inverse);

// The text layer under the OBJ / MTL readers, exposed so the tests can hold it against the reference's own
// tokenizer and MtlParser (src/string_util.cpp:7-38, src/mtl_parser.cpp:16-113; test/string_util_test.cpp:9-37).
struct MtlMaterial {
    std::string name;
    float diffuse[3] = { 0.f, 0.f, 0.f };
    float emit[3] = { 0.f, 0.f, 0.f };
};
std::vector<std::string> tokenizeLine(const std::string &line);
std::string leftTrim(const std::string &token);
std::vector<MtlMaterial> parseMtlFile(const std::string &path);

}  // namespace pathed
