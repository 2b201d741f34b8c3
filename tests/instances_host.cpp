// The host arithmetic of instanced scenes (pathed_amd/csrc/instances.h) without a GPU: tests/test_instance_tables_host.py builds
// this program plainly and under the address and undefined-behaviour sanitizers and runs it.  Prints "failures 0" when all holds.
#include "instances.h"

#include <cstdio>
#include <functional>

using namespace pathed;

static int g_failures = 0;
#define CHECK(cond, ...)                                                         \
    do {                                                                         \
        if (!(cond)) {                                                           \
            g_failures++;                                                        \
            if (g_failures <= 40) { printf("FAIL %s:%d  %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                                        \
    } while (0)

// ---- a scene description with instances that owns its arrays
struct Built {
    std::vector<float> positions;
    std::vector<uint32_t> indices;
    std::vector<int32_t> triMaterial;
    std::vector<PathedGeom> geoms;
    std::vector<PathedMaterial> materials;
    std::vector<PathedPrototype> prototypes;
    std::vector<PathedInstance> instances;
    PathedSceneDesc desc;
    PathedInstanceDesc in;
    PathedSceneOptions options;

    Built() { material(PATHED_MAT_LAMBERTIAN); }
    int material(int type, float emit = 0.f)
    {
        PathedMaterial m;
        std::memset(&m, 0, sizeof m);
        m.type = type;
        m.emit[1] = emit;
        materials.push_back(m);
        return (int)materials.size() - 1;
    }
    // one mesh geom: `corners` holds 3 floats per vertex, `faces` 3 vertex numbers per triangle
    void mesh(const std::vector<float> &corners, const std::vector<uint32_t> &faces, int materialIndex = 0)
    {
        const uint32_t base = (uint32_t)(positions.size() / 3);
        geoms.push_back({ PATHED_GEOM_MESH, (int32_t)triMaterial.size(), (int32_t)(faces.size() / 3), -1 });
        positions.insert(positions.end(), corners.begin(), corners.end());
        for (uint32_t v : faces) { indices.push_back(base + v); }
        triMaterial.insert(triMaterial.end(), faces.size() / 3, materialIndex);
    }
    // the last n_geoms geoms so far become a prototype
    void prototype(int nGeoms) { prototypes.push_back({ (int32_t)geoms.size() - nGeoms, nGeoms }); }
    void place(int prototypeIndex, const float *transform)
    {
        PathedInstance instance;
        instance.prototype = prototypeIndex;
        std::memcpy(instance.transform, transform, sizeof instance.transform);
        instances.push_back(instance);
    }
    void finish()
    {
        std::memset(&desc, 0, sizeof desc);
        desc.n_vertices = (uint32_t)(positions.size() / 3);
        desc.positions = positions.data();
        desc.n_triangles = (uint32_t)triMaterial.size();
        desc.indices = indices.data(); desc.tri_material = triMaterial.data();
        desc.n_geoms = (uint32_t)geoms.size(); desc.geoms = geoms.data();
        desc.n_materials = (uint32_t)materials.size(); desc.materials = materials.data();
        std::memset(&in, 0, sizeof in);
        in.struct_size = sizeof in;
        in.n_prototypes = (uint32_t)prototypes.size(); in.prototypes = prototypes.empty() ? nullptr : prototypes.data();
        in.n_instances = (uint32_t)instances.size(); in.instances = instances.empty() ? nullptr : instances.data();
        std::memset(&options, 0, sizeof options);
        options.struct_size = sizeof options;
    }
};

static const float kIdentity[12] = { 1.f, 0.f, 0.f, 0.f,  0.f, 1.f, 0.f, 0.f,  0.f, 0.f, 1.f, 0.f };

static void icosahedron(std::vector<float> *corners, std::vector<uint32_t> *faces)
{
    const float g = 1.618034f;
    *corners = { -1.f, g, 0.f,  1.f, g, 0.f,  -1.f, -g, 0.f,  1.f, -g, 0.f,  0.f, -1.f, g,  0.f, 1.f, g,
                 0.f, -1.f, -g,  0.f, 1.f, -g,  g, 0.f, -1.f,  g, 0.f, 1.f,  -g, 0.f, -1.f,  -g, 0.f, 1.f };
    *faces = { 0, 11, 5,  0, 5, 1,  0, 1, 7,  0, 7, 10,  0, 10, 11,  1, 5, 9,  5, 11, 4,  11, 10, 2,  10, 7, 6,  7, 1, 8,
               3, 9, 4,  3, 4, 2,  3, 2, 6,  3, 6, 8,  3, 8, 9,  4, 9, 5,  2, 4, 11,  6, 2, 10,  8, 6, 7,  9, 8, 1 };
}

// two world triangles and one placement of an icosahedron: the description every refusal below is one change away from
static void baseline(Built *scene)
{
    std::vector<float> corners;
    std::vector<uint32_t> faces;
    scene->mesh({ -4.f, 0.f, -4.f,  -4.f, 0.f, 4.f,  4.f, 0.f, 4.f,  4.f, 0.f, -4.f }, { 0, 1, 2,  0, 2, 3 });
    icosahedron(&corners, &faces);
    scene->mesh(corners, faces);
    scene->prototype(1);
    scene->place(0, kIdentity);
}

// ---- refusals: the code and the exact text, and with two things wrong the text of the check that comes first
static void expectRefusal(const char *what, int code, const char *text, const std::function<void(Built &)> &change)
{
    Built scene;
    baseline(&scene);
    scene.finish();
    change(scene);
    InstancedLayout layout;
    std::string message;
    const int got = planInstances(&scene.desc, scene.options, &scene.in, &layout, &message);
    CHECK(got == code && message == text, "%s: code %d, message \"%s\"", what, got, message.c_str());
}

static void testRefusals()
{
    {
        Built scene;
        baseline(&scene);
        scene.finish();
        InstancedLayout layout;
        std::string message = "untouched";
        CHECK(planInstances(&scene.desc, scene.options, &scene.in, &layout, &message) == PATHED_OK && message == "untouched", "the baseline: \"%s\"", message.c_str());
        CHECK(layout.worldTris == 2 && layout.protoFirst == std::vector<int>{ 2 } && layout.protoCount == std::vector<int>{ 20 }, "layout");
        CHECK(layout.bases == (std::vector<int>{ 2, 22 }) && layout.inverses.size() == 12, "bases");
    }
    const char *kRanges = "prototypes must name consecutive, non-empty geom ranges that end the geom array";
    const char *kRefittable = "refittable: a scene with instances cannot be refitted";
    const char *kSpheres = "sphere primitives in a scene with instances are not supported";
    const char *kMedia = "media and containers (passthrough materials) in a scene with instances are not supported";
    const char *kOrder = "a scene with instances: the mesh geoms must cover the triangles in order, without gaps";
    const char *kInvertible = "instance transform is not invertible";
    expectRefusal("struct_size", PATHED_E_INVALID, "PathedInstanceDesc.struct_size mismatch", [](Built &s) { s.in.struct_size -= 4; });
    expectRefusal("no prototype array", PATHED_E_INVALID, "prototype or instance array missing", [](Built &s) { s.in.prototypes = nullptr; });
    expectRefusal("no instance array", PATHED_E_INVALID, "prototype or instance array missing", [](Built &s) { s.in.instances = nullptr; });
    expectRefusal("2^30 - 1 instances", PATHED_E_INVALID, "too many instances (the limit is 2^30 - 2)", [](Built &s) { s.in.n_instances = (1u << 30) - 1u; });
    expectRefusal("a sphere", PATHED_E_UNSUPPORTED, kSpheres, [](Built &s) { s.desc.n_spheres = 1; });
    expectRefusal("a medium", PATHED_E_UNSUPPORTED, kMedia, [](Built &s) { s.desc.n_media = 1; });
    expectRefusal("a container", PATHED_E_UNSUPPORTED, kMedia, [](Built &s) { s.materials[0].type = PATHED_MAT_PASSTHROUGH; });
    expectRefusal("refittable", PATHED_E_UNSUPPORTED, kRefittable, [](Built &s) { s.options.refittable = 1; });
    for (int builder : { PATHED_BVH_LBVH_DEVICE, PATHED_BVH_PLOC_DEVICE }) {
        expectRefusal("a device builder", PATHED_E_UNSUPPORTED, "the device builders (LBVH, PLOC) do not build a scene with instances: use the host SAH builder",
                      [&](Built &s) { s.options.bvh_builder = builder + 1; });
    }
    expectRefusal("shade_kernel", PATHED_E_UNSUPPORTED, "shade_kernel: a scene with instances renders on the wavefront's per-slot pair only (0 or 1)",
                  [](Built &s) { s.options.shade_kernel = 5; });
    expectRefusal("node_format", PATHED_E_UNSUPPORTED, "node_format: a scene with instances is walked over the 128-byte float nodes", [](Built &s) { s.options.node_format = 2; });
    expectRefusal("a gap between the geoms", PATHED_E_INVALID, kOrder, [](Built &s) { s.geoms[1].first = 3; });
    expectRefusal("a geom that is no mesh", PATHED_E_INVALID, kOrder, [](Built &s) { s.geoms[0].type = PATHED_GEOM_SPHERE; });
    expectRefusal("triangles behind the geoms", PATHED_E_INVALID, "a scene with instances: the mesh geoms must cover all triangles", [](Built &s) { s.desc.n_triangles += 1; });
    expectRefusal("2^27 triangles", PATHED_E_INVALID, "a scene with instances stores fewer than 2^27 triangles (the instance leaf encoding)",
                  [](Built &s) { s.geoms[1].count = (1 << 27) - 2; s.desc.n_triangles = 1u << 27; });
    expectRefusal("a prototype of no geoms", PATHED_E_INVALID, kRanges, [](Built &s) { s.prototypes[0].n_geoms = 0; });
    expectRefusal("a prototype before the array", PATHED_E_INVALID, kRanges, [](Built &s) { s.prototypes[0].first_geom = -1; });
    expectRefusal("a prototype past the array", PATHED_E_INVALID, kRanges, [](Built &s) { s.prototypes[0].n_geoms = 2; });
    expectRefusal("geoms behind the prototypes", PATHED_E_INVALID, kRanges, [](Built &s) { s.prototypes[0].first_geom = 0; });
    expectRefusal("a prototype without a triangle", PATHED_E_INVALID, "a prototype needs at least one triangle",
                  [](Built &s) { s.geoms[1].count = 0; s.desc.n_triangles = 2; });
    expectRefusal("an emitter in a prototype", PATHED_E_UNSUPPORTED,
                  "an emissive material inside a prototype is not supported: bake such faces into world triangles, one copy per placement",
                  [](Built &s) { s.material(PATHED_MAT_LAMBERTIAN, 1.f); s.desc.n_materials = 2; s.desc.materials = s.materials.data(); s.triMaterial[21] = 1; });
    expectRefusal("a prototype index", PATHED_E_INVALID, "instance prototype index out of range", [](Built &s) { s.instances[0].prototype = 1; });
    expectRefusal("a negative prototype index", PATHED_E_INVALID, "instance prototype index out of range", [](Built &s) { s.instances[0].prototype = -1; });
    expectRefusal("a NaN", PATHED_E_INVALID, "instance transform is not finite", [](Built &s) { s.instances[0].transform[7] = std::nanf(""); });
    expectRefusal("an infinity", PATHED_E_INVALID, "instance transform is not finite", [](Built &s) { s.instances[0].transform[0] = __builtin_huge_valf(); });
    expectRefusal("zeros", PATHED_E_INVALID, kInvertible, [](Built &s) { for (float &value : s.instances[0].transform) { value = 0.f; } });
    expectRefusal("two equal rows", PATHED_E_INVALID, kInvertible, [](Built &s) { for (int i = 0; i < 4; i++) { s.instances[0].transform[4 + i] = s.instances[0].transform[i]; } });
    expectRefusal("an inverse beyond float", PATHED_E_INVALID, kInvertible, [](Built &s) { s.instances[0].transform[0] = 1e-39f; });
    // the virtual ids: a prototype of 2^20 triangles 2048 times (only its materials are read before the tree is built)
    expectRefusal("2^31 virtual ids", PATHED_E_INVALID, "a scene with instances: the virtual primitive ids (world triangles + every placement's) must stay below the limit of 2^31",
                  [](Built &s) {
                      s.geoms[1].count = 1 << 20;
                      s.triMaterial.assign(2 + (1 << 20), 0);
                      s.desc.tri_material = s.triMaterial.data();
                      s.desc.n_triangles = 2u + (1u << 20);
                      s.instances.assign(2048, s.instances[0]);
                      s.in.instances = s.instances.data();
                      s.in.n_instances = 2048;
                  });
    // two things wrong: the message of the check that comes first
    expectRefusal("struct_size before spheres", PATHED_E_INVALID, "PathedInstanceDesc.struct_size mismatch", [](Built &s) { s.in.struct_size += 8; s.desc.n_spheres = 3; });
    expectRefusal("spheres before media", PATHED_E_UNSUPPORTED, kSpheres, [](Built &s) { s.desc.n_spheres = 1; s.desc.n_media = 1; });
    expectRefusal("media before refittable", PATHED_E_UNSUPPORTED, kMedia, [](Built &s) { s.desc.n_media = 1; s.options.refittable = 1; });
    expectRefusal("refittable before the builder", PATHED_E_UNSUPPORTED, kRefittable, [](Built &s) { s.options.refittable = 1; s.options.bvh_builder = PATHED_BVH_PLOC_DEVICE + 1; });
    expectRefusal("options before the geoms", PATHED_E_UNSUPPORTED, kRefittable, [](Built &s) { s.options.refittable = 1; s.geoms[1].first = 3; });
    expectRefusal("the geoms before the prototypes", PATHED_E_INVALID, kOrder, [](Built &s) { s.geoms[1].first = 3; s.prototypes[0].n_geoms = 0; });
    expectRefusal("the prototypes before the instances", PATHED_E_INVALID, kRanges, [](Built &s) { s.prototypes[0].n_geoms = 0; s.instances[0].prototype = 7; });
    expectRefusal("the index before the transform", PATHED_E_INVALID, "instance prototype index out of range",
                  [](Built &s) { s.instances[0].prototype = 7; s.instances[0].transform[0] = std::nanf(""); });
    expectRefusal("instance 0 before instance 1", PATHED_E_INVALID, kInvertible, [](Built &s) {
        s.instances.push_back(s.instances[0]);
        for (float &value : s.instances[0].transform) { value = 0.f; }
        s.instances[1].prototype = 7;
        s.in.instances = s.instances.data();
        s.in.n_instances = 2;
    });
}

// ---- the two-level tree
static int refOf(const FlatBvh &bvh, int node, int child)
{
    int ref;
    std::memcpy(&ref, &bvh.nodes[(size_t)kNodeFloats * node + 24 + child], 4);
    return ref;
}

// Walks the tree under `root`: every inner reference inside [nodeLo, nodeHi) and every node met once, every triangle leaf inside
// [triLo, triHi); counts how often each triangle and, for the top tree, each placement is met and where the placement's leaf
// is.  Returns the node levels on the longest chain.
struct Walk {
    const FlatBvh &bvh;
    int nodeLo, nodeHi, triLo, triHi;
    bool instanceLeaves;
    std::vector<int> nodeSeen, triSeen, instanceSeen, leafNode, leafChild;
    bool fine = true;

    int depth(int node)
    {
        if (node < nodeLo || node >= nodeHi || node >= bvh.nodeCount) { fine = false; return 0; }
        if (nodeSeen[(size_t)node]++) { fine = false; return 0; }   // a node with two parents, or a cycle
        int deepest = 0;
        for (int child = 0; child < 4; child++) {
            const int ref = refOf(bvh, node, child);
            if (ref == kEmptyChildRef) { continue; }
            if (ref >= 0) { deepest = std::max(deepest, depth(ref)); continue; }
            const int payload = -ref - 1;
            if (payload & kInstanceLeafBit) {
                const int instance = payload & (kInstanceLeafBit - 1);
                if (!instanceLeaves || instance >= (int)instanceSeen.size()) { fine = false; continue; }
                instanceSeen[(size_t)instance]++;
                leafNode[(size_t)instance] = node;
                leafChild[(size_t)instance] = child;
                continue;
            }
            const int first = payload >> 3, count = payload & 7;
            if (count < 1 || first < triLo || first + count > triHi) { fine = false; continue; }
            for (int t = first; t < first + count; t++) { triSeen[(size_t)t]++; }
        }
        return deepest + 1;
    }
};

static void checkTree(const char *name, Built &scene)
{
    scene.finish();
    InstancedLayout layout;
    std::string message;
    const int code = planInstances(&scene.desc, scene.options, &scene.in, &layout, &message);
    CHECK(code == PATHED_OK, "%s: refused, \"%s\"", name, message.c_str());
    if (code != PATHED_OK) { return; }
    std::vector<float> records, protoBoxes;
    int maxStack = -1, topNodes = -1, topDepth = -1;
    const FlatBvh bvh = buildInstancedBvh(&scene.desc, &scene.in, layout, 2, &records, &maxStack, &protoBoxes, &topNodes, &topDepth);
    const int nInstances = (int)scene.in.n_instances, nProto = (int)scene.in.n_prototypes, worldTris = layout.worldTris;
    const int storedTris = (int)scene.desc.n_triangles;
    CHECK(bvh.nodes.size() == (size_t)kNodeFloats * bvh.nodeCount && bvh.leafTris.size() == (size_t)12 * storedTris, "%s: array sizes", name);
    CHECK(records.size() == (size_t)28 * nInstances && protoBoxes.size() == (size_t)8 * nProto, "%s: record sizes", name);
    CHECK(topNodes >= 1 && topNodes <= bvh.nodeCount, "%s: topNodes %d of %d", name, topNodes, bvh.nodeCount);
    if (g_failures) { return; }

    // node array: every inner reference inside it
    for (int n = 0; n < bvh.nodeCount; n++) {
        for (int k = 0; k < 4; k++) { CHECK(refOf(bvh, n, k) < bvh.nodeCount, "%s: node %d child %d points at %d of %d", name, n, k, refOf(bvh, n, k), bvh.nodeCount); }
    }
    // the top tree: nodes [0, topNodes), world triangles [0, worldTris), every placement in exactly one instance leaf
    Walk top{ bvh, 0, topNodes, 0, worldTris, true, std::vector<int>((size_t)bvh.nodeCount, 0), std::vector<int>((size_t)storedTris, 0),
              std::vector<int>((size_t)nInstances, 0), std::vector<int>((size_t)nInstances, -1), std::vector<int>((size_t)nInstances, -1) };
    const int topLevels = top.depth(0);
    CHECK(top.fine, "%s: the top tree leaves its ranges", name);
    CHECK(topLevels == topDepth, "%s: top tree of %d levels, recorded %d", name, topLevels, topDepth);
    for (int k = 0; k < nInstances; k++) { CHECK(top.instanceSeen[(size_t)k] == 1, "%s: placement %d sits in %d leaves", name, k, top.instanceSeen[(size_t)k]); }
    for (int t = 0; t < worldTris; t++) { CHECK(top.triSeen[(size_t)t] == 1, "%s: world triangle slot %d sits in %d leaves", name, t, top.triSeen[(size_t)t]); }
    std::vector<int> primSeen((size_t)std::max(worldTris, 1), 0);
    for (int t = 0; t < worldTris; t++) {
        int prim;
        std::memcpy(&prim, &bvh.leafTris[(size_t)12 * t + 3], 4);
        CHECK(prim >= 0 && prim < worldTris, "%s: world slot %d holds primitive %d", name, t, prim);
        if (prim >= 0 && prim < worldTris) { primSeen[(size_t)prim]++; }
    }
    for (int t = 0; t < worldTris; t++) { CHECK(primSeen[(size_t)t] == 1, "%s: world triangle %d is stored %d times", name, t, primSeen[(size_t)t]); }

    // records: quad 6, the bases; the prototypes' roots in prototype order behind the top tree
    std::vector<int> protoRoot((size_t)nProto, -1);
    int virtualTris = worldTris;
    for (int k = 0; k < nInstances; k++) {
        int ids[4];
        std::memcpy(ids, &records[(size_t)28 * k + 24], sizeof ids);
        const int prototype = scene.instances[(size_t)k].prototype;
        CHECK(ids[0] == layout.bases[(size_t)k] && ids[0] == virtualTris, "%s: placement %d base %d, expected %d", name, k, ids[0], virtualTris);
        CHECK(ids[1] == prototype && ids[3] == layout.protoFirst[(size_t)prototype], "%s: placement %d ids (%d, %d)", name, k, ids[1], ids[3]);
        CHECK(ids[2] >= topNodes && ids[2] < bvh.nodeCount, "%s: placement %d root %d", name, k, ids[2]);   // node 0 is never a prototype's
        CHECK(protoRoot[(size_t)prototype] < 0 || protoRoot[(size_t)prototype] == ids[2], "%s: two roots for prototype %d", name, prototype);
        protoRoot[(size_t)prototype] = ids[2];
        CHECK(std::memcmp(&records[(size_t)28 * k], scene.instances[(size_t)k].transform, 48) == 0, "%s: placement %d transform rows", name, k);
        CHECK(std::memcmp(&records[(size_t)28 * k + 12], &layout.inverses[(size_t)12 * k], 48) == 0, "%s: placement %d inverse rows", name, k);
        if (k > 0) { CHECK(layout.bases[(size_t)k] > layout.bases[(size_t)k - 1], "%s: bases do not ascend at %d", name, k); }
        virtualTris += layout.protoCount[(size_t)prototype];
    }
    CHECK(layout.bases.size() == (size_t)nInstances + 1 && layout.bases.back() == virtualTris, "%s: the bases end at %d, expected %d", name, layout.bases.back(), virtualTris);

    // the prototypes' trees: a placed prototype's references stay inside its own node and triangle ranges
    int deepest = 0, nextNode = topNodes;
    for (int p = 0; p < nProto; p++) {
        const int triLo = layout.protoFirst[(size_t)p], triHi = triLo + layout.protoCount[(size_t)p];
        int nodeHi = bvh.nodeCount;
        for (int q = 0; q < nProto; q++) { if (protoRoot[(size_t)q] > protoRoot[(size_t)p] && protoRoot[(size_t)p] >= 0) { nodeHi = std::min(nodeHi, protoRoot[(size_t)q]); } }
        if (protoRoot[(size_t)p] < 0) { continue; }   // never placed: nothing names its root
        CHECK(protoRoot[(size_t)p] >= nextNode, "%s: prototype %d root %d before %d", name, p, protoRoot[(size_t)p], nextNode);
        Walk walk{ bvh, protoRoot[(size_t)p], nodeHi, triLo, triHi, false, std::vector<int>((size_t)bvh.nodeCount, 0), std::vector<int>((size_t)storedTris, 0), {}, {}, {} };
        deepest = std::max(deepest, walk.depth(protoRoot[(size_t)p]));
        CHECK(walk.fine, "%s: prototype %d leaves its ranges", name, p);
        for (int t = triLo; t < triHi; t++) {
            int prim;
            std::memcpy(&prim, &bvh.leafTris[(size_t)12 * t + 3], 4);
            CHECK(walk.triSeen[(size_t)t] == 1 && prim >= 0 && prim < triHi - triLo, "%s: prototype %d slot %d: in %d leaves, primitive %d", name, p, t, walk.triSeen[(size_t)t], prim);
        }
        nextNode = nodeHi;
    }
    bool allPlaced = true;
    for (int p = 0; p < nProto; p++) { allPlaced = allPlaced && protoRoot[(size_t)p] >= 0; }
    if (allPlaced) {
        CHECK(maxStack == (3 * topDepth + 1) + (3 * deepest + 1) + 1, "%s: maxStack %d with %d + %d levels", name, maxStack, topDepth, deepest);
        CHECK(bvh.maxDepth == topDepth + deepest, "%s: maxDepth %d", name, bvh.maxDepth);
    }

    // boxes: every corner of the prototype, placed in fp32 as the device flattens it, inside the child box of the placement's leaf
    int outside = 0;
    for (int k = 0; k < nInstances; k++) {
        const int node = top.leafNode[(size_t)k], child = top.leafChild[(size_t)k];
        if (node < 0) { continue; }
        const size_t prototype = (size_t)scene.instances[(size_t)k].prototype;
        for (int i = 0; i < 3 * layout.protoCount[prototype]; i++) {
            const float *corner = &scene.positions[(size_t)3 * scene.indices[(size_t)3 * layout.protoFirst[prototype] + i]];
            float world[3];
            flattenPoint(scene.instances[(size_t)k].transform, corner[0], corner[1], corner[2], world);
            for (int a = 0; a < 3; a++) {
                const float lo = bvh.nodes[(size_t)kNodeFloats * node + 4 * a + child], hi = bvh.nodes[(size_t)kNodeFloats * node + 12 + 4 * a + child];
                if (!(lo <= world[a] && world[a] <= hi)) { outside++; }
            }
        }
    }
    CHECK(outside == 0, "%s: %d placed corners outside their leaf's box", name, outside);
    printf("%s: %d nodes (%d top, %d + %d levels), %d placements, maxStack %d\n", name, bvh.nodeCount, topNodes, topDepth, deepest, nInstances, maxStack);
}

static void testTrees()
{
    std::vector<float> corners;
    std::vector<uint32_t> faces;
    icosahedron(&corners, &faces);
    const float c = 0.8f, s = 0.6f;   // a rotation about y by atan(3 / 4)
    const float turned[12] = { 0.25f * c, 0.f, 0.25f * s, 3.f,  0.f, 0.25f, 0.f, 1.5f,  -0.25f * s, 0.f, 0.25f * c, -2.f };
    const float mirrored[12] = { -1.f, 0.f, 0.f, 100.f,  0.f, 1.f, 0.f, 100.f,  0.f, 0.f, 1.f, -100.f };
    {
        Built scene;
        baseline(&scene);
        scene.place(0, turned);
        scene.place(0, mirrored);
        checkTree("two triangles and three placements", scene);
    }
    {
        Built scene;
        scene.mesh(corners, faces);
        scene.prototype(1);
        scene.place(0, turned);
        checkTree("an empty world", scene);
    }
    {
        Built scene;
        std::vector<float> strip;
        std::vector<uint32_t> stripFaces;
        for (uint32_t i = 0; i < 10; i++) {
            const float x = (float)i;
            const float triangle[9] = { x, 0.f, 0.f,  x + 1.f, 0.f, 0.5f,  x, 1.f, 0.25f * x };
            strip.insert(strip.end(), triangle, triangle + 9);
            for (uint32_t v = 0; v < 3; v++) { stripFaces.push_back(3 * i + v); }
        }
        scene.mesh(strip, stripFaces);
        checkTree("no prototypes", scene);
    }
    {
        Built scene;
        scene.mesh({ -4.f, 0.f, -4.f,  -4.f, 0.f, 4.f,  4.f, 0.f, 4.f }, { 0, 1, 2 });
        scene.mesh({ 0.f, 0.f, 0.f,  1.f, 0.25f, 0.f,  0.25f, 1.f, 0.5f }, { 0, 1, 2 });
        scene.prototype(1);
        for (int row = 0; row < 64; row++) {
            for (int col = 0; col < 64; col++) {
                const float scale = 0.25f + 3.75f * (float)((row * 64 + col) % 17) / 16.f;   // 0.25 .. 4
                const float placed[12] = { scale, 0.f, 0.f, 1.5f * (float)col,  0.f, (row & 1) ? -scale : scale, 0.f, 0.125f * (float)(col % 5),  0.f, 0.f, scale, 1.5f * (float)row - 48.f };
                scene.place(0, placed);
            }
        }
        checkTree("a 64 x 64 grid of one triangle", scene);
    }
}

// ---- the record and the box rule on their own
static void testRecordAndBox()
{
    const float m[12] = { 2.f, 0.f, 0.f, 1.f,  0.f, 4.f, 0.f, -2.f,  0.f, 0.f, 0.5f, 3.f };
    float inverse[12], record[28];
    CHECK(instanceInverse(m, inverse), "a diagonal transform");
    const float expected[12] = { 0.5f, 0.f, 0.f, -0.5f,  0.f, 0.25f, 0.f, 0.5f,  0.f, 0.f, 2.f, -6.f };
    for (int i = 0; i < 12; i++) { CHECK(inverse[i] == expected[i], "inverse[%d] = %g", i, inverse[i]); }
    packInstanceRecord(m, inverse, 7, 1, 9, 40, record);
    int ids[4];
    std::memcpy(ids, record + 24, sizeof ids);
    CHECK(std::memcmp(record, m, 48) == 0 && std::memcmp(record + 12, inverse, 48) == 0 && ids[0] == 7 && ids[1] == 1 && ids[2] == 9 && ids[3] == 40, "the record's 28 floats");
    // the unit box under m spans [1, 3] x [-2, 2] x [3, 3.5]: each side moves out by 1e-5 max(1, |lo|, |hi|) + 1e-5 (hi - lo)
    const float protoLo[3] = { 0.f, 0.f, 0.f }, protoHi[3] = { 1.f, 1.f, 1.f };
    float lo[3], hi[3];
    placementBox(m, protoLo, protoHi, lo, hi);
    const float spanLo[3] = { 1.f, -2.f, 3.f }, spanHi[3] = { 3.f, 2.f, 3.5f };
    for (int a = 0; a < 3; a++) {
        const float pad = 1e-5f * std::max(1.f, std::max(std::fabs(spanLo[a]), std::fabs(spanHi[a]))) + 1e-5f * (spanHi[a] - spanLo[a]);
        CHECK(lo[a] == spanLo[a] - pad && hi[a] == spanHi[a] + pad, "axis %d: [%.9g, %.9g]", a, lo[a], hi[a]);
    }
    CHECK(hostMin(0.f, -0.f) == 0.f && !std::signbit(hostMin(0.f, -0.f)) && std::signbit(hostMin(-0.f, 0.f)), "hostMin keeps its first zero");
    CHECK(!std::signbit(hostMax(0.f, -0.f)) && std::signbit(hostMax(-0.f, 0.f)), "hostMax keeps its first zero");
}

int main()
{
    testRefusals();
    testRecordAndBox();
    testTrees();
    printf("failures %d\n", g_failures);
    return g_failures ? 1 : 0;
}
