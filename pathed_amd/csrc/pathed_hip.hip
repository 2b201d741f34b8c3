// libpathed_hip.so — implementation of include/pathed_hip.h.
// Host side: scene flattening (BVH, shading records, light table, env CDFs), upload,
// the wavefront iteration loop, HIP-event timing and statistics.
#include "pathed_hip.h"

#include "bvh_build.h"
#include "kernels.h"
#include "features.h"
#include "shading_queries.h"
#if PATHED_EXPERIMENTS
#include "kernels_experiments.h"
#endif
#include "lbvh.h"
#include "scene_tables.h"

#include <hip/hip_runtime.h>

#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

using namespace pathed;

namespace {

thread_local std::string g_error;
int g_device = -1;

int fail(int code, const std::string &message)
{
    g_error = message;
    return code;
}

// Tuning switches read from the environment exist in the EXPERIMENTS build only (`make experiments`): the product library
// takes every setting from PathedSceneOptions, so a stray PATHED_* variable on a bench box cannot change a kernel, a slot
// count or a builder behind the caller's back (bench.py also refuses to run with one set).  Two debug PRINTS stay in both
// builds: PATHED_DEBUG_ALLOC and PATHED_DEBUG_STATS (they change no result and no timing path).
inline const char *tuningEnv(const char *name)
{
#if PATHED_EXPERIMENTS
    return std::getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t status_ = (expr);                                                       \
        if (status_ != hipSuccess) {                                                       \
            return fail(PATHED_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(status_)); \
        }                                                                                  \
    } while (0)

// hipSetDevice is per host thread: every entry point that takes a scene selects the scene's device first
#define SELECT_DEVICE(scene) HIP_TRY(hipSetDevice((scene)->deviceId))

template <typename T>
struct DeviceBuffer {
    T *ptr = nullptr;
    size_t count = 0;

    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;              // owns its allocation: the members of PathedScene
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;   // are freed with it
    ~DeviceBuffer() { release(); }

    hipError_t allocate(size_t n)
    {
        const bool report = getenv("PATHED_DEBUG_ALLOC") != nullptr && n * sizeof(T) >= ((size_t)1 << 28);
        const auto t0 = std::chrono::steady_clock::now();
        release();
        const auto t1 = std::chrono::steady_clock::now();
        count = n;
        if (n == 0) { return hipSuccess; }
        const hipError_t status = hipMalloc((void **)&ptr, n * sizeof(T));
        if (report) {
            const auto t2 = std::chrono::steady_clock::now();
            fprintf(stderr, "[pathed] device buffer of %.2f GB: hipFree of the old one %.3f s, hipMalloc %.3f s\n", (double)(n * sizeof(T)) / 1e9,
                    std::chrono::duration<double>(t1 - t0).count(), std::chrono::duration<double>(t2 - t1).count());
        }
        return status;
    }

    hipError_t upload(const std::vector<T> &host)
    {
        hipError_t status = allocate(host.size());
        if (status != hipSuccess || host.empty()) { return status; }
        return hipMemcpy(ptr, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice);
    }

    void release()
    {
        if (ptr) { (void)hipFree(ptr); }
        ptr = nullptr;
        count = 0;
    }

    // takes ownership of a raw hipMalloc'ed allocation of n elements (null: of nothing)
    void adopt(T *allocation, size_t n)
    {
        release();
        ptr = allocation;
        count = allocation ? n : 0;
    }

    void swap(DeviceBuffer &other)
    {
        std::swap(ptr, other.ptr);
        std::swap(count, other.count);
    }
};

struct EventRing {
    static const int kPairs = 512;
    hipEvent_t start[kPairs];
    hipEvent_t stop[kPairs];
    bool used[kPairs];
    int next = 0;
    bool created = false;
    double totalMs = 0.0;
    unsigned long long launches = 0;

    hipError_t create()
    {
        if (created) { return hipSuccess; }
        for (int i = 0; i < kPairs; i++) {
            hipError_t status = hipEventCreate(&start[i]);
            if (status != hipSuccess) { return status; }
            status = hipEventCreate(&stop[i]);
            if (status != hipSuccess) { return status; }
            used[i] = false;
        }
        created = true;
        return hipSuccess;
    }

    void harvest(int i)
    {
        if (!used[i]) { return; }
        float ms = 0.f;
        (void)hipEventSynchronize(stop[i]);
        if (hipEventElapsedTime(&ms, start[i], stop[i]) == hipSuccess) {
            totalMs += ms;
            launches++;
        }
        used[i] = false;
    }

    int acquire()
    {
        const int i = next;
        next = (next + 1) % kPairs;
        harvest(i);
        used[i] = true;
        return i;
    }

    void harvestAll()
    {
        if (!created) { return; }
        for (int i = 0; i < kPairs; i++) { harvest(i); }
    }

    void destroy()
    {
        if (!created) { return; }
        for (int i = 0; i < kPairs; i++) {
            (void)hipEventDestroy(start[i]);
            (void)hipEventDestroy(stop[i]);
        }
        created = false;
    }
};

// One start / stop event pair for the entry points that report a device time.  run() times one stretch of launches and adds
// it to `ms`; `status` keeps the FIRST error, after which nothing more is recorded or launched.
struct EventTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    hipError_t status = hipSuccess;
    float ms = 0.f;

    EventTimer()
    {
        keep(hipEventCreate(&start));
        if (ok()) { keep(hipEventCreate(&stop)); }
    }
    EventTimer(const EventTimer &) = delete;
    EventTimer &operator=(const EventTimer &) = delete;
    ~EventTimer()
    {
        if (start) { (void)hipEventDestroy(start); }
        if (stop) { (void)hipEventDestroy(stop); }
    }

    bool ok() const { return status == hipSuccess; }
    bool keep(hipError_t result)
    {
        if (ok()) { status = result; }
        return ok();
    }

    // the device time of this stretch, which has finished on return (0 after an error)
    template <typename Launches>
    float run(Launches &&launches, hipStream_t stream = nullptr)
    {
        float part = 0.f;
        if (ok() && keep(hipEventRecord(start, stream))) {
            launches();
            keep(hipGetLastError());
        }
        if (ok() && keep(hipEventRecord(stop, stream)) && keep(hipEventSynchronize(stop))) { keep(hipEventElapsedTime(&part, start, stop)); }
        ms += part;
        return part;
    }
};

// The level-synchronous passes of a bottom-up refit (kernels.h: k_refit_pass; instance_kernels.h: k_refit_top_pass) over a
// tree of nNodes nodes.  `ready` holds two flag arrays of nNodes bytes, cleared by the caller; a pass reads one and writes the
// other, and launchPass(in, out) launches one.
struct LevelPasses {
    unsigned char *ready;
    size_t nNodes;
    std::function<void(const unsigned char *in, unsigned char *out)> launchPass;
    int passes = 0;

    void launch(int count)
    {
        for (int k = 0; k < count; k++, passes++) { launchPass(ready + (size_t)(passes & 1) * nNodes, ready + (size_t)((passes + 1) & 1) * nNodes); }
    }
    // one pass per 4-wide level, back to back (no look at the flags in between: a host round trip costs more than a pass)
    void launchLevels(int depth) { launch(depth > 0 ? depth + 1 : 16); }
    // After launchLevels: whether the root was reached.  A tree deeper than its recorded depth keeps going, four passes per
    // look at the root's flag and 4096 passes at most; their device time joins the timer's.
    bool reachRoot(EventTimer &timer)
    {
        unsigned char rootReady = 0;
        const auto look = [&]() { return timer.ok() && timer.keep(hipMemcpy(&rootReady, ready + (size_t)(passes & 1) * nNodes, 1, hipMemcpyDeviceToHost)); };
        while (look() && !rootReady && passes < 4096) { timer.run([&]() { launch(4); }); }
        return rootReady != 0;
    }
};

}  // namespace

static const int kMaxPools = 4;
static_assert(kOptionMaxPools == kMaxPools && kOptionMinSlots == kBlock, "scene_tables.h: checkSceneOptions states these limits in its messages");
static const int kDefaultShadeLaunches = 1;   // shade launches per trace launch of a scene with local rays (PathedSceneOptions.shade_launches = 0): more were
// measured and lose -- the shade kernel is the slower partner, profiles/r5_ab_local_rays.log
static const int kDefaultSmallPhase1 = 1;   // PathedSceneOptions.small_phase1 = 0: 1 VALU, 2 matrix pipe


// The compile-time scene sets (shading.h: SceneTraits) that contain the scene.  They overlap -- a Lambertian-only scene is
// also triangleLit, roughBeckmann and smoothSet -- and every launch ladder ranks them for its own kernel.
struct SceneTraitFlags {
    bool lambertianTriangles = false;   // constant-albedo Lambertian surfaces, triangle lights, no spheres, no environment: k_path_small<.., TraitsLambertianTriangles>
    bool lambertianPlasticSpheres = false;   // the Veach scene's set (shading.h)
    bool triangleLit = false;                // any BSDF, constant albedo, triangle lights only, no spheres, no environment
    // [r5] ... narrowed further (shading.h: the ladder): rough BSDFs over one microfacet distribution / Lambertian + glass + mirror
    bool roughBeckmann = false, roughGgx = false, smoothSet = false;
    bool lambertianGlassContainer = false;   // the reference's volume scene's set
    bool envOnly = false;     // the one light is the environment and no material emits: k_shade<.., ENV_ONLY> (kernels.h)
};

struct PathedScene {
    DScene device;
    int width = 0, height = 0;
    int deviceId = 0;             // the HIP device every buffer of this scene lives on
    PathedSceneOptions options;   // as passed to scene_create_ex (zeroed = defaults)

    // host copy kept for export / introspection (a device-built tree is downloaded on demand)
    FlatBvh bvh;
    bool bvhOnHost = true;
    int bvhBuilder = PATHED_BVH_SAH_HOST;
    double bvhBuildMs = 0.0;

    DeviceBuffer<float4> nodes, nodesQ, leafTris, triShade, triCompact, lightRecords, envRgba, texels;
    DeviceBuffer<DSphere> spheres;
    float spherePairs[8][4][2] = {};   // RenderParams.spherePairs: the spheres two by two for the fused kernel's packed pre-test
    DeviceBuffer<DMaterial> materials;
    DeviceBuffer<DLight> lights;
    DeviceBuffer<float> thetaCdf, phiCdf;
    DeviceBuffer<int> phiEmpty, thetaGuide, phiGuide;
    DeviceBuffer<float4> thetaRecords, phiRecords;
    DeviceBuffer<DMedium> media;
    DeviceBuffer<int> primMedium;
    // voxel-grid media (grid_medium.h; pathed_hip_scene_set_grid_medium): the records, every grid's cells, and the host copies
    // the device arrays are rebuilt from when a grid is set or replaced
    DeviceBuffer<DGrid> grids;
    DeviceBuffer<float> gridData;
    std::vector<DMedium> mediaHost;
    std::vector<DGrid> gridsHost;
    std::vector<std::vector<float>> gridCells;   // per grid
    // phase functions (volume.h: Henyey-Greenstein; pathed_hip_scene_set_medium_phase): per medium slot the type and g as they
    // were set, and the table the anisotropic kernels read (g, 0 for an isotropic slot).  Empty until the first call.
    std::vector<int> phaseTypeHost;
    std::vector<float> phaseGHost;
    DeviceBuffer<float> phaseG;
    bool anisotropic = false;   // some slot is Henyey-Greenstein with |g| >= kPhaseIsotropicBelow: BasicVolumeIntegrator runs k_path_aniso
    DeviceBuffer<int> volumeOverflow;   // the volume kernel's traversal-stack spill, per thread
    // the fused kernel's per-pixel camera-ray candidate masks (camera_masks.h), then its started samples, per wave of its largest
    // grid (kernels.h: the camera queue)
    DeviceBuffer<float4> cameraQueue;
    bool cameraMasksBuilt = false;
    double cameraMaskMs = 0.0;          // device time of the last build (HIP events)

    // render state, allocated on first use
    int nSlots = 0;               // capacity of the per-slot state buffers
    bool adaptiveSlots = false;   // BVH scenes without an explicit max_slots: short calls use fewer slots
    int unitOrder = kOrderStripes;   // kernels.h: THE UNIT ORDER
    size_t chunkCapacity = 0;     // float4 entries of chunkBuf
    int samplesPerUnit = 1;       // "chunk": samples a slot sums before it publishes a partial (1 = the reference's summation order)
    int maxSlots = 1 << 20;
    int pools = 2;                // independent slot pools on separate streams (trace || shade); PATHED_POOLS = 1..kMaxPools
    hipStream_t poolStreams[kMaxPools] = { nullptr, nullptr, nullptr, nullptr };
    hipEvent_t poolDone[kMaxPools] = { nullptr, nullptr, nullptr, nullptr };
    hipEvent_t callerReady = nullptr;
    DeviceBuffer<float4> rayO, rayD, hit, mod, thr, res, pend, acc, shO, shD, chunkBuf;
    DeviceBuffer<unsigned int> counters;
    DeviceBuffer<unsigned long long> suspendMask;  // per pool, per trace wave (kernels.h: tail suspension)
    DeviceBuffer<int> suspendData;
    DeviceBuffer<int> stackOverflow;  // per pool, per trace thread, (maxStack - stackRows) rows
    DeviceBuffer<unsigned long long> stats;
    unsigned int *hostRemaining = nullptr;  // pinned

    int integrator = PATHED_INTEGRATOR_PATH_TRACER;   // pathed_hip_set_integrator
    bool hasContainers = false;   // some surface carries the passthrough material: only the volume integrator renders the scene
    bool spheresInTree = false;   // the host builder put the spheres into leaves (else they are tested one by one after the traversal)
    bool fusedPath = false;   // tiny scenes: k_path_small, whole paths in registers, no wavefront buffers
    // BVH scenes: k_path_wave (path_wave.h: paths in registers, no state in HBM) instead of the wavefront kernels.  It renders
    // at a rate that hardly depends on the size of the call, the wavefront needs some 50 M camera samples to fill and drain its
    // 8 Mi slots and is 9-20 % faster beyond (profiles/r4_ab_wave.log): 0 by the size of the call, 1 never, 2 always
    int waveMode = 0;
    bool waveAvailable = false;   // ... and the scene is one it serves
    bool lastCallWave = false;    // what the last render call ran (PathedStats.path_kernel)
    bool lastCallHybrid = false;
    bool lastCallList = false;    // ... a pixel list: the wavefront kernels, whatever the scene's own path kernel is
    bool lastCallFeatures = false;   // ... k_features (features.h): a feature call, or a render call of the albedo integrator
    unsigned long long featureRays = 0;   // closest-hit queries of k_features since reset_stats (one per camera sample)
    unsigned long long waveMaxSamples = 48ull << 20;   // calls of fewer camera samples than this take it (waveMode 0)
    int waveStragglers = 24;      // its traversal bursts end once fewer rays than this are in flight
    bool waveBlock = false;       // the block's waves share one ray ring (k_path_wave<.., BLOCK>; PATHED_WAVE_BLOCK=1)
    int waveShadeReady = 40;      // ... and a wave shades once this many of its paths have their rays back
    int waveRefill = kRefillThreshold;   // ... and idle lanes draw from the wave's list once fewer than this many are busy
    bool stagedShade = true;  // k_shade_staged (dense, state-sorted stages inside a block) or k_shade (one lane per slot)
    SceneTraitFlags traits;   // which narrowed kernel instantiations serve the scene (sceneTraits)
    int nodeFormat = 0;                      // what k_trace walks (trace.h): 0 the 128-byte float nodes, 1 nodeQ, 2 node8
    bool splitShade = false;  // k_vertex + k_regen over the hit / miss lists the trace kernel writes (kernels.h: split shade stage)
    int vertexGrid = 0, regenGrid = 0;   // their persistent grids, blocks
    unsigned int listCap = 0;            // list blocks per shard
    DeviceBuffer<unsigned int> slotLists, deferredLists;
    size_t deferredSlots = 0;            // slots deferredLists was sized for
    int stageRounds = 2;      // staged kernel: a block owns stageRounds x 256 slots

    int stackRows = 8;    // LDS rows of the per-lane traversal stack (8 / 16 / 22)
    int maxStack = 0;     // the tree's bound on stack entries; entries beyond stackRows spill to stackOverflow
    bool sceneInLds = false;
    bool bruteForce = false;      // <= kBruteForceMaxTris triangles: test them all, no BVH walk
    SmallTris smallTris;          // their records, passed to k_trace_small as a kernel argument
    // the fused kernel's phase-1 records (small_items.h): parallelograms first, then the triangles without a partner; phase 2
    // indexes itemTris, the triangle records in the same (item) order
    SmallTris smallItems;
    SmallItemsLayout smallLayout;
    DeviceBuffer<float4> itemTris;
    std::vector<float> itemTrisHost;       // host copy of itemTris (12 floats per triangle)
    // the PASS LIST (small_items.h: NEVER-HIT): the same without exact copies of a lower-numbered triangle, what the
    // kSmallPassList instantiations of k_path_small walk.  Its item-ordered triangles are the SECOND device.nTris records of
    // itemTris (passTris of them in use), so the kernel needs no pointer of its own for them
    SmallTris passItems;
    SmallItemsLayout passLayout;
    int passTris = 0;
    unsigned long long passNeverHit = 0ull;    // bit (original primitive id & 63)
    std::vector<float> passTrisHost;
    std::vector<float> smallExtraPoints;  // sphere bounds: where else a ray may start (the camera is added when the records are built)
    std::vector<unsigned char> smallEmitterPrims;   // per original primitive id: the triangle is a light (small_items.h: SmallLights)
    std::vector<float> smallSphereLights;           // centre.xyz, radius of every sphere light: about center_sample, where sphereSample puts
                                                    // the samples, and again about center_world (a transformed sphere has two centres)
    // PathedSceneOptions.refittable: the triangle soup stays on the device for pathed_hip_scene_refit
    bool refittable = false;
    DeviceBuffer<float> soupPositions, soupNormals, soupUvs;
    DeviceBuffer<uint32_t> soupIndices;
    DeviceBuffer<int> soupTriMaterial;
    DeviceBuffer<float4> refitLo, refitHi;          // unpadded bounds per node (refit working memory, allocated on first use)
    DeviceBuffer<unsigned char> refitReady;         // two flag arrays
    size_t soupVertices = 0;
    // [r5] local rays of the wavefront (kernels.h: RenderParams::localTris): the scene's few large triangles and the bounds of the rest
    int localCount = 0;
    float4 localTris[3 * 8];
    float localLo[3] = { 0.f, 0.f, 0.f }, localHi[3] = { 0.f, 0.f, 0.f }, localSphere[4] = { 0.f, 0.f, 0.f, 0.f };
    // [r5] k_path_hybrid (path_hybrid.h): scenes of 65 .. kHybridMaxTris triangles split into a DIRECT set of <= 64 large
    // triangles (all-items intersector) and a TREE part with a 4-wide BVH of its own
    bool hybridAvailable = false;  // the split exists
    bool hybridPath = false;       // ... and render calls take it
    SmallTris hybridItems;         // phase-1 records of the direct set
    SmallItemsLayout hybridLayout;
    std::vector<float> hybridDirectLeaf;   // the direct set as the builder's 12-float records (v0, prim) (e1, -) (e2, -)
    std::vector<float> hybridBounds;       // corners of the scene's bounding box: where else rays start (buildSmallItems' extra points)
    DeviceBuffer<float4> hybridItemTris, hybridNodes, hybridTris;
    int hybridNodeCount = 0, hybridTreeTris = 0, hybridDirectTris = 0, hybridMaxStack = 1;
    float hybridLo[3] = { 0.f, 0.f, 0.f }, hybridHi[3] = { 0.f, 0.f, 0.f }, hybridSphere[4] = { 0.f, 0.f, 0.f, 0.f };
    bool mfmaPhase1 = false;      // k_path_small<.., MFMA>: phase 1 on the matrix pipe (mfma_candidates.h)
    DeviceBuffer<float> mfmaTable;   // its A-side rows
    MfmaFrame mfmaFrame;
    size_t traceLdsBytes = 0;
    int traceGrid = 0;
    int suspendLanes = kSuspendLanes;  // PATHED_SUSPEND_LANES overrides (0 = off)
    int suspendPatience = kSuspendPatience;  // PATHED_SUSPEND_PATIENCE
    int parkMinCards = 1;                    // PATHED_PARK_MIN_CARDS
    int computeUnits = 256;

    // instanced scenes (trace.h: "Instances"; pathed_hip_scene_create_instanced): the records and id bases of the placements
    bool instanced = false;
    DeviceBuffer<float4> instanceRecords;
    DeviceBuffer<int> instanceBases;
    DInstanceSet instanceSet = { nullptr, nullptr, 0, 0 };
    int instancedMaxStack = 0;    // the top tree's bound + the deepest prototype's + 1
    // moving placements (pathed_hip_scene_set_instance_transforms): the top tree is nodes [0, topNodes) of `nodes`, topDepth
    // 4-wide levels deep; the prototypes' padded boxes (lo, hi per prototype) the placements' world boxes are made from
    int topNodes = 0, topDepth = 0;
    DeviceBuffer<float4> protoBoxes;
    // ... and its working memory, allocated on first use: the second record buffer (a call writes it, then swaps it with
    // instanceRecords), the uploaded transforms of the host entry, (refused count, lowest refused index), and the refit's
    // unpadded bounds and two flag arrays, topNodes entries each
    DeviceBuffer<float4> instanceRecordsStaged;
    DeviceBuffer<float> instanceTransforms;
    DeviceBuffer<unsigned int> instanceBad;
    DeviceBuffer<float4> topLo, topHi;
    DeviceBuffer<unsigned char> topReady;
    // the shutter (pathed_hip_scene_set_instance_motion; instance_motion.h: k_motion_boxes): while hasMotion, the second
    // transforms and the moving flags the kernels read (motionSet), and what the refit and the rebuild of the top tree read in
    // place of the records and the prototype boxes.  A call writes the staged twins and swaps them in when nothing is refused.
    struct MotionBuffers {
        DeviceBuffer<float4> closeRows, boxRecords, boxTable;
        DeviceBuffer<int> moving;
    };
    bool hasMotion = false;
    MotionBuffers motion, motionStaged;
    DMotionSet motionSet = { nullptr, nullptr, 0.f, 1.f };
    DeviceBuffer<float> motionTransforms;   // the uploaded transforms of the host entry

    bool countMode = false;
    bool timeKernels = false;
    int timeInterval = 1;                 // HIP-event pairs around every n-th launch pair of a pool
    unsigned long long traceLaunchesAll = 0;   // trace launches since reset_stats, timed or not
    EventRing traceEvents, shadeEvents;
    unsigned long long iterations = 0;
    unsigned long long cameraSamples = 0;

    ~PathedScene()
    {
        if (hostRemaining) { (void)hipHostFree(hostRemaining); }
        for (int h = 0; h < kMaxPools; h++) {
            if (poolStreams[h]) { (void)hipStreamDestroy(poolStreams[h]); }
            if (poolDone[h]) { (void)hipEventDestroy(poolDone[h]); }
        }
        if (callerReady) { (void)hipEventDestroy(callerReady); }
        traceEvents.destroy();
        shadeEvents.destroy();
    }
};

namespace {

V3 hv(const float *p) { return v3(p[0], p[1], p[2]); }

// lookAt, reference src/transform.cpp:138-164
void buildCamera(const PathedCamera &desc, DCamera *camera)
{
    const V3 source = hv(desc.origin);
    const V3 target = hv(desc.target);
    const V3 up = hv(desc.up);

    const V3 direction = normalized(source - target);
    const V3 xAxis = normalized(cross(normalized(up), direction));
    const V3 yAxis = cross(direction, xAxis);
    const float sign = desc.flip_handedness ? -1.f : 1.f;

    camera->m[0] = sign * xAxis.x; camera->m[1] = yAxis.x; camera->m[2] = direction.x;
    camera->m[3] = sign * xAxis.y; camera->m[4] = yAxis.y; camera->m[5] = direction.y;
    camera->m[6] = sign * xAxis.z; camera->m[7] = yAxis.z; camera->m[8] = direction.z;
    camera->origin[0] = source.x; camera->origin[1] = source.y; camera->origin[2] = source.z;

    // src/camera.cpp:34-35
    const float zNear = 0.01f;
    camera->filmHeight = 2 * tanf(desc.vertical_fov / 2) * zNear;
    camera->filmWidth = camera->filmHeight * desc.width / desc.height;
    camera->resX = desc.width;
    camera->resY = desc.height;
}

DMaterial buildMaterial(const PathedMaterial &m)
{
    DMaterial out;
    std::memset(&out, 0, sizeof out);
    out.type = m.type;
    out.albedoType = m.albedo_type;
    // OrenNayar ctor, reference src/oren_nayar.cpp:11-18
    const float sigma2 = m.sigma * m.sigma;
    out.orenA = 1.f - (sigma2 / (2.f * (sigma2 + 0.33f)));
    out.orenB = (0.45f * sigma2) / (sigma2 + 0.09f);
    for (int i = 0; i < 3; i++) {
        out.diffuse[i] = m.diffuse[i];
        // only Lambertian carries emission through the reference's parser
        // (src/scene_parser.cpp:574-667: every other ctor passes Color(0))
        out.emit[i] = (m.type == PATHED_MAT_LAMBERTIAN) ? m.emit[i] : 0.f;
        out.checkerOn[i] = m.checker_on[i];
        out.checkerOff[i] = m.checker_off[i];
    }
    out.alpha = m.alpha;
    out.ior = m.ior;
    out.distribution = m.distribution;
    out.checkerResU = m.checker_res[0];
    out.checkerResV = m.checker_res[1];
    return out;
}

bool emits(const DMaterial &m) { return !(m.emit[0] == 0.f && m.emit[1] == 0.f && m.emit[2] == 0.f); }

// a float array the device reads as float4 (nodes, leaf triangles, the records of scene_tables.h)
std::vector<float4> asQuads(const std::vector<float> &floats)
{
    std::vector<float4> quads(floats.size() / 4);
    std::memcpy(quads.data(), floats.data(), quads.size() * sizeof(float4));
    return quads;
}

int validate(const PathedSceneDesc *desc)
{
    if (!desc) { return fail(PATHED_E_INVALID, "scene description is null"); }
    if (desc->abi_version != PATHED_ABI_VERSION) { return fail(PATHED_E_INVALID, "abi_version mismatch"); }
    if (desc->camera.width <= 0 || desc->camera.height <= 0) { return fail(PATHED_E_INVALID, "camera resolution must be positive"); }
    if ((uint64_t)desc->camera.width * (uint64_t)desc->camera.height > (1ull << 28)) { return fail(PATHED_E_INVALID, "image too large"); }
    if (desc->n_triangles && (!desc->positions || !desc->indices || !desc->tri_material || !desc->normals || !desc->uvs)) {
        return fail(PATHED_E_INVALID, "triangle arrays missing");
    }
    if (desc->n_spheres && !desc->spheres) { return fail(PATHED_E_INVALID, "sphere array missing"); }
    if (desc->n_geoms && !desc->geoms) { return fail(PATHED_E_INVALID, "geom array missing"); }
    if (desc->n_materials == 0 || !desc->materials) { return fail(PATHED_E_INVALID, "scene needs at least one material"); }
    for (uint32_t i = 0; i < desc->n_triangles; i++) {
        for (int k = 0; k < 3; k++) {
            if (desc->indices[3 * i + k] >= desc->n_vertices) { return fail(PATHED_E_INVALID, "vertex index out of range"); }
        }
        if (desc->tri_material[i] < 0 || (uint32_t)desc->tri_material[i] >= desc->n_materials) {
            return fail(PATHED_E_INVALID, "triangle material index out of range");
        }
    }
    for (uint32_t i = 0; i < desc->n_spheres; i++) {
        if (desc->spheres[i].material < 0 || (uint32_t)desc->spheres[i].material >= desc->n_materials) {
            return fail(PATHED_E_INVALID, "sphere material index out of range");
        }
    }
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        const int type = desc->materials[i].type;
        if (type < PATHED_MAT_LAMBERTIAN || type > PATHED_MAT_PASSTHROUGH) { return fail(PATHED_E_UNSUPPORTED, "unknown material type"); }
        const int albedo = desc->materials[i].albedo_type;
        if (albedo < PATHED_ALBEDO_CONSTANT || albedo > PATHED_ALBEDO_TEXTURE) { return fail(PATHED_E_UNSUPPORTED, "unknown albedo type"); }
        if (albedo == PATHED_ALBEDO_TEXTURE) {
            const int texture = desc->materials[i].texture;
            if (texture < 0 || (uint32_t)texture >= desc->n_textures || !desc->textures) { return fail(PATHED_E_INVALID, "material texture index out of range"); }
        }
        const int distribution = desc->materials[i].distribution;
        if ((type == PATHED_MAT_MICROFACET || type == PATHED_MAT_PLASTIC)
            && distribution != PATHED_DIST_BECKMANN && distribution != PATHED_DIST_GGX) {
            return fail(PATHED_E_UNSUPPORTED, "unknown microfacet distribution");
        }
    }
    if (desc->n_textures && !desc->textures) { return fail(PATHED_E_INVALID, "texture array missing"); }
    for (uint32_t i = 0; i < desc->n_textures; i++) {
        const PathedTexture &texture = desc->textures[i];
        if (texture.width < 1 || texture.height < 1 || texture.width > 65535 || texture.height > 65535 || !texture.rgb) {
            return fail(PATHED_E_INVALID, "texture size must be 1..65535 and its texels present");
        }
    }
    for (uint32_t i = 0; i < desc->n_geoms; i++) {
        const PathedGeom &geom = desc->geoms[i];
        if (geom.type == PATHED_GEOM_MESH) {
            if (geom.first < 0 || geom.count < 0 || (uint64_t)geom.first + (uint64_t)geom.count > desc->n_triangles) {
                return fail(PATHED_E_INVALID, "mesh geom range out of bounds");
            }
        } else if (geom.type == PATHED_GEOM_SPHERE) {
            if (geom.first < 0 || (uint32_t)geom.first >= desc->n_spheres) { return fail(PATHED_E_INVALID, "sphere geom out of bounds"); }
        } else {
            return fail(PATHED_E_INVALID, "unknown geom type");
        }
    }
    if (desc->env) {
        if (desc->env->width <= 0 || desc->env->height <= 0 || !desc->env->rgba) { return fail(PATHED_E_INVALID, "environment map missing"); }
    }
    if (desc->n_media && !desc->media) { return fail(PATHED_E_INVALID, "media array missing"); }
    for (uint32_t i = 0; i < desc->n_media; i++) {
        // HomogeneousMedium asserts sigma_t.r == g == b (reference src/homogeneous_medium.cpp): distances are sampled with
        // one channel and attenuated with all three, so unequal channels would render a biased image silently
        const float *t = desc->media[i].sigma_t, *sc = desc->media[i].sigma_s;
        if (!(t[0] == t[1] && t[1] == t[2])) { return fail(PATHED_E_INVALID, "homogeneous medium: the three sigma_t channels must be equal"); }
        for (int k = 0; k < 3; k++) {
            if (!(t[k] >= 0.f && t[k] < 3e38f && sc[k] >= 0.f && sc[k] < 3e38f)) { return fail(PATHED_E_INVALID, "homogeneous medium: sigma_t and sigma_s must be finite and not negative"); }
        }
    }
    for (uint32_t i = 0; i < desc->n_geoms; i++) {
        if (desc->geoms[i].medium < -1 || (desc->geoms[i].medium >= 0 && (uint32_t)desc->geoms[i].medium >= desc->n_media)) {
            return fail(PATHED_E_INVALID, "geom medium index out of range");
        }
    }
    return PATHED_OK;
}

// chunks (units per pixel) rendered per internal pass: bounds chunkBuf to 256 float4 per pixel (4.3 GB at 1024^2, 8.5 GB
// at 1080p; further capped at 2^30 units).  Every pass pays the slot pool's ramp-up and drain once -- with one sample
// per unit and the queues in step that is a few milliseconds on a BVH scene (256 against 1 024 units per pixel: -0.3 %
// on Cornell, -1.8 % on the 5.2 M-triangle mesh, -4 % on the teapot with 8 Mi slots, tools/pass_length_sweep.sh) -- but
// hipMalloc of a large buffer is not free here: 17 GB take 0.5 s, 1.0 s when another 17 GB were freed just before
// (PATHED_DEBUG_ALLOC=1 prints it), which would add a quarter to a 2 s job.  PATHED_CHUNKS_PER_PASS overrides for
// experiments and long-lived processes.
const int kMaxChunksPerPass = 256;

// the statistics buffer, zeroed when it is made
int ensureStats(PathedScene *scene)
{
    if (scene->stats.ptr) { return PATHED_OK; }
    HIP_TRY(scene->stats.allocate(kStatCount));
    HIP_TRY(hipMemset(scene->stats.ptr, 0, kStatCount * sizeof(unsigned long long)));
    return PATHED_OK;
}

int ensureRenderState(PathedScene *scene, int nSlots, size_t chunkEntries)
{
    if (scene->nSlots < nSlots || !scene->rayO.ptr) {   // capacity: a call that wants fewer slots uses a prefix
        scene->nSlots = nSlots;
        const size_t n = (size_t)nSlots;
        HIP_TRY(scene->rayO.allocate(n));
        HIP_TRY(scene->rayD.allocate(n));
        HIP_TRY(scene->hit.allocate(n));
        HIP_TRY(scene->mod.allocate(n));
        HIP_TRY(scene->thr.allocate(n));
        HIP_TRY(scene->res.allocate(n));
        HIP_TRY(scene->pend.allocate(n));
        HIP_TRY(scene->acc.allocate(n));
        HIP_TRY(scene->shO.allocate(n));
        HIP_TRY(scene->shD.allocate(n));
    }
    if (scene->chunkCapacity < chunkEntries) {
        HIP_TRY(scene->chunkBuf.allocate(chunkEntries));
        scene->chunkCapacity = chunkEntries;
    }
    if (scene->splitShade) {
        // per pool and list: every slot once, plus one partly filled block per wave that writes (trace and k_vertex
        // waves); sized for the slot capacity, so a call that uses fewer slots fits as well
        const size_t writerWaves = (size_t)(scene->traceGrid + scene->vertexGrid) * kWavesPerBlock;
        const size_t blocks = (size_t)scene->nSlots / 64 + writerWaves;
        // a block's shard is picked from the shader clock: an eighth of slack keeps a shard from ever running full
        const unsigned int cap = (unsigned int)((blocks + kListShards - 1) / kListShards) * 9u / 8u + 8u;
        if (cap > scene->listCap || !scene->slotLists.ptr) {
            scene->listCap = cap;
            HIP_TRY(scene->slotLists.allocate((size_t)kMaxPools * 2 * (size_t)cap * kListShards * 64));
        }
        // sized and indexed with the slot count itself (cap rounds per 32 blocks: nSlots can grow without cap growing)
        if ((size_t)scene->nSlots > scene->deferredSlots || !scene->deferredLists.ptr) {
            HIP_TRY(scene->deferredLists.allocate((size_t)kMaxPools * 4 * (size_t)scene->nSlots));
            scene->deferredSlots = (size_t)scene->nSlots;
        }
    }
    if (!scene->counters.ptr) { HIP_TRY(scene->counters.allocate(kMaxPools * kCtrCount)); }
    if (!scene->suspendMask.ptr && !scene->bruteForce) {
        const size_t waves = (size_t)scene->traceGrid * kWavesPerBlock;
        HIP_TRY(scene->suspendMask.allocate((size_t)scene->pools * waves));
        HIP_TRY(scene->suspendData.allocate((size_t)scene->pools * waves * (size_t)(kSaveWords + scene->maxStack) * 64));
        HIP_TRY(scene->stackOverflow.allocate((size_t)scene->pools * stackSpillInts((size_t)scene->traceGrid * kBlock, scene->maxStack, scene->stackRows)));
    }
    if (const int code = ensureStats(scene)) { return code; }
    if (!scene->hostRemaining) {
        HIP_TRY(hipHostMalloc((void **)&scene->hostRemaining, kMaxPools * 32 * sizeof(unsigned int), hipHostMallocDefault));
    }
    return PATHED_OK;
}

// The launch ladders pick ONE instantiation of a kernel from run-time flags.  withBool turns such a flag into a compile-time
// constant: f is called with std::true_type or std::false_type and is compiled for both, so a rung that exists for both values
// of a flag is one line inside it.  A rung that exists for one value only is written with that value, outside.  What the
// ladders name is what the library contains (tests/test_kernel_resources.py counts it).
// withStackRows does the same for a kernel's STACK argument: f is called with std::integral_constant<int, 8 | 16 | 22>, chosen
// by stackRowsFor (scene_tables.h), and returns what f returns.  Inside it the launch takes its LDS bytes, stackLdsBytes(STACK),
// from that same constant, so a kernel cannot be started with the stack of another.
template <typename F>
void withBool(bool value, F &&f)
{
    if (value) { f(std::true_type{}); } else { f(std::false_type{}); }
}

template <typename F>
auto withStackRows(int rows, F &&f)
{
    switch (stackRowsFor(rows)) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    default: return f(std::integral_constant<int, 22>{});
    }
}

// k_trace<STACK, LDS_SCENE, COUNT, LISTS, SPHERES, FORMAT>: every rung with and without counting
template <int STACK>
void launchTraceStack(PathedScene *scene, const RenderParams &params, hipStream_t stream)
{
    const auto run = [&](void (*kernel)(RenderParams)) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)scene->traceGrid), dim3(kBlock), scene->traceLdsBytes, stream, params);
    };
    withBool(scene->countMode, [&](auto COUNT) {
#if PATHED_EXPERIMENTS
        if (scene->splitShade) { withBool(scene->sceneInLds, [&](auto LDS_SCENE) { run(k_trace<STACK, LDS_SCENE, COUNT, true>); }); return; }
        if (scene->nodeFormat == 1) { run(k_trace<STACK, false, COUNT, false, false, 1>); return; }
        if (scene->nodeFormat == 2) { run(k_trace<STACK, false, COUNT, false, false, 2>); return; }
#endif
        if (!scene->sceneInLds && scene->device.nSpheres == 0 && !scene->options.generic_kernels && !tuningEnv("PATHED_NO_SCENE_TRAITS")) {
            run(k_trace<STACK, false, COUNT, false, false>);
            return;
        }
        withBool(scene->sceneInLds, [&](auto LDS_SCENE) { run(k_trace<STACK, LDS_SCENE, COUNT, false>); });
    });
}

// k_trace_instanced<STACK, COUNT>: the three stack-row counts, with and without counting (k_trace_instanced_motion while a shutter is set)
void launchTraceInstanced(PathedScene *scene, const RenderParams &params, hipStream_t stream)
{
    // a grid-stride kernel: at most the grid the overflow columns were sized for, at most a wave per batch of slots and one more
    // block's worth for the shadow list
    const int wanted = 2 * params.nSlots / kBlock;
    const dim3 grid((unsigned)(wanted < scene->traceGrid ? (wanted > 0 ? wanted : 1) : scene->traceGrid)), block(kBlock);
    withBool(scene->countMode, [&](auto COUNT) {
        withStackRows(scene->stackRows, [&](auto STACK) {
            if (scene->hasMotion) {
                hipLaunchKernelGGL((k_trace_instanced_motion<STACK, COUNT>), grid, block, stackLdsBytes(STACK), stream, params, scene->instanceSet, scene->motionSet);
                return;
            }
            hipLaunchKernelGGL((k_trace_instanced<STACK, COUNT>), grid, block, stackLdsBytes(STACK), stream, params, scene->instanceSet);
        });
    });
}

void launchTrace(PathedScene *scene, const RenderParams &params, hipStream_t stream)
{
    if (scene->instanced) { launchTraceInstanced(scene, params, stream); return; }
    if (scene->bruteForce) {
        // uniform cost per batch and no per-block setup: one 64-ray batch per wave, the hardware
        // dispatcher balances (a persistent grid quantises 3.3 batches per wave to 4 rounds)
        const dim3 grid((unsigned)(2 * params.nSlots / kBlock)), block(kBlock);
        withBool(scene->countMode, [&](auto COUNT) { hipLaunchKernelGGL((k_trace_small<COUNT>), grid, block, 0, stream, params, scene->smallTris); });
        return;
    }
    withStackRows(scene->stackRows, [&](auto STACK) { launchTraceStack<STACK>(scene, params, stream); });
}

#if defined(PATHED_EXPERIMENTS) && PATHED_EXPERIMENTS
// [r5, experiments build] What would SORTING the ray queue buy the production trace kernel?  (Round 1's answer came from the
// one-ray-per-thread test kernel.)  With PATHED_SORT_PROBE=<iteration> the wavefront stops before pool 0's trace launch of that
// iteration, copies the pool's rays, and times k_trace -- this very kernel, cards, refill, LDS stack rows, parking off -- over
// (a) the copy in slot order and (b) the same rays permuted so that the ones to be traced come first, ordered by (direction octant,
// 30-bit Morton code of the origin); hits go to a scratch buffer, the render's own state is not touched.  tools/sort_probe.py.
static void sortProbe(PathedScene *scene, const RenderParams &q, hipStream_t stream)
{
    (void)hipDeviceSynchronize();
    const size_t n = (size_t)q.nSlots;
    std::vector<float4> rayO(n), rayD(n);
    if (hipMemcpy(rayO.data(), q.state.rayO, n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess
        || hipMemcpy(rayD.data(), q.state.rayD, n * sizeof(float4), hipMemcpyDeviceToHost) != hipSuccess) { return; }
    std::vector<uint32_t> traced, rest;
    float lo[3] = { 3e38f, 3e38f, 3e38f }, hi[3] = { -3e38f, -3e38f, -3e38f };
    for (size_t i = 0; i < n; i++) {
        int flags; std::memcpy(&flags, &rayD[i].w, 4);
        if (flags & (kStDone | kStHold | kStLocal)) { rest.push_back((uint32_t)i); continue; }
        traced.push_back((uint32_t)i);
        const float o[3] = { rayO[i].x, rayO[i].y, rayO[i].z };
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], o[a]); hi[a] = std::max(hi[a], o[a]); }
    }
    auto spread = [](uint32_t v) { uint64_t x = v & 0x3FFu; x = (x | (x << 16)) & 0x30000FFull; x = (x | (x << 8)) & 0x300F00Full; x = (x | (x << 4)) & 0x30C30C3ull; x = (x | (x << 2)) & 0x9249249ull; return x; };
    // orders: 0 slot order; 1 by direction octant only (stable: what eight counters in the shade kernel could produce);
    // 2 by (octant, 24-bit Morton code of the origin, 18-bit Morton code of the direction), stable
    const int kOrders = 3;
    std::vector<float4> orderedO[kOrders], orderedD[kOrders];
    for (int v = 0; v < kOrders; v++) {
        std::vector<std::pair<uint64_t, uint32_t>> keyed(traced.size());
        for (size_t k = 0; k < traced.size(); k++) {
            const uint32_t i = traced[k];
            const float o[3] = { rayO[i].x, rayO[i].y, rayO[i].z }, d[3] = { rayD[i].x, rayD[i].y, rayD[i].z };
            uint32_t cell[3], turn[3];
            for (int a = 0; a < 3; a++) {
                const float t = hi[a] > lo[a] ? (o[a] - lo[a]) / (hi[a] - lo[a]) : 0.f;
                cell[a] = (uint32_t)std::min(255.f, std::max(0.f, t * 255.f));
                turn[a] = (uint32_t)std::min(63.f, std::max(0.f, (d[a] * 0.5f + 0.5f) * 63.f));
            }
            const uint64_t octant = (d[0] < 0.f ? 4u : 0u) | (d[1] < 0.f ? 2u : 0u) | (d[2] < 0.f ? 1u : 0u);
            const uint64_t place = (spread(cell[0]) << 2) | (spread(cell[1]) << 1) | spread(cell[2]);
            const uint64_t heading = (spread(turn[0]) << 2) | (spread(turn[1]) << 1) | spread(turn[2]);
            keyed[k] = { v == 0 ? 0ull : v == 1 ? octant : ((octant << 42) | (place << 18) | heading), i };
        }
        std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<uint64_t, uint32_t> &a, const std::pair<uint64_t, uint32_t> &b) { return a.first < b.first; });
        orderedO[v].resize(n); orderedD[v].resize(n);
        size_t at = 0;
        for (const auto &entry : keyed) { orderedO[v][at] = rayO[entry.second]; orderedD[v][at] = rayD[entry.second]; at++; }
        for (uint32_t i : rest) { orderedO[v][at] = rayO[i]; orderedD[v][at] = rayD[i]; at++; }
    }
    float4 *dO[kOrders] = { nullptr, nullptr, nullptr }, *dD[kOrders] = { nullptr, nullptr, nullptr }, *dHit = nullptr;
    unsigned int *dCounters = nullptr;
    bool ok = hipMalloc(&dHit, n * sizeof(float4)) == hipSuccess && hipMalloc(&dCounters, kCtrCount * sizeof(unsigned int)) == hipSuccess;
    for (int v = 0; v < kOrders && ok; v++) {
        ok = hipMalloc(&dO[v], n * sizeof(float4)) == hipSuccess && hipMalloc(&dD[v], n * sizeof(float4)) == hipSuccess
            && hipMemcpy(dO[v], orderedO[v].data(), n * sizeof(float4), hipMemcpyHostToDevice) == hipSuccess
            && hipMemcpy(dD[v], orderedD[v].data(), n * sizeof(float4), hipMemcpyHostToDevice) == hipSuccess;
    }
    EventTimer timer;
    if (ok && timer.ok()) {
        fprintf(stderr, "[pathed] sort probe: %zu slots, %zu rays for the trace kernel (%.3f of the slots), shadow list left out\n", n, traced.size(), (double)traced.size() / (double)n);
        for (int repeat = 0; repeat < 3; repeat++) {
            for (int v = -1; v < kOrders; v++) {
                RenderParams probe = q;
                if (v >= 0) { probe.state.rayO = dO[v]; probe.state.rayD = dD[v]; }   // (-1: the pool's own arrays, rays where their slots are)
                probe.state.hit = dHit;
                probe.counters = dCounters;
                probe.suspendLanes = 0;   // no parking: the whole pool in one launch
                (void)hipMemsetAsync(dCounters, 0, kCtrCount * sizeof(unsigned int), stream);
                const float ms = timer.run([&]() { launchTrace(scene, probe, stream); }, stream);
                fprintf(stderr, "[pathed] sort probe: k_trace over the rays %s: %.1f us (%.2f Grays/s)\n",
                        v < 0 ? "as they lie in the pool" : v == 0 ? "compacted, in slot order" : v == 1 ? "by direction octant" : "by (octant, origin cell, direction cell)", 1e3 * ms, (double)traced.size() / (1e6 * ms));
            }
        }
    }
    for (int v = 0; v < kOrders; v++) { if (dO[v]) { (void)hipFree(dO[v]); } if (dD[v]) { (void)hipFree(dD[v]); } }
    if (dHit) { (void)hipFree(dHit); }
    if (dCounters) { (void)hipFree(dCounters); }
}
#endif

// every rung with the materials in LDS and without
void launchShade(PathedScene *scene, const RenderParams &params, hipStream_t stream)
{
    const bool ldsMaterials = scene->device.nMaterials <= kMaxLdsMaterials;
#if PATHED_EXPERIMENTS
    const size_t lds = ldsMaterials ? (size_t)scene->device.nMaterials * sizeof(DMaterial) : 0;
    if (scene->splitShade && !PATHED_EXP_LISTS_ONLY) {
        const int slotBlocks = params.nSlots / kBlock;
        const dim3 vertexGrid((unsigned)(scene->vertexGrid < slotBlocks ? scene->vertexGrid : slotBlocks));
        const dim3 regenGrid((unsigned)(scene->regenGrid < slotBlocks ? scene->regenGrid : slotBlocks));
        withBool(ldsMaterials, [&](auto LDS_MATERIALS) { hipLaunchKernelGGL((k_vertex<LDS_MATERIALS>), vertexGrid, dim3(kBlock), lds, stream, params); });
        hipLaunchKernelGGL(k_regen, regenGrid, dim3(kBlock), 0, stream, params);
        return;
    }
    if (scene->stagedShade) {
        const dim3 grid((unsigned)(params.nSlots / (kBlock * scene->stageRounds))), block(kBlock);
        withBool(ldsMaterials, [&](auto LDS_MATERIALS) {
            if (scene->stageRounds == 4) { hipLaunchKernelGGL((k_shade_staged<LDS_MATERIALS, 4>), grid, block, lds, stream, params); }
            else { hipLaunchKernelGGL((k_shade_staged<LDS_MATERIALS, 2>), grid, block, lds, stream, params); }
        });
        return;
    }
#endif
    if (scene->instanced) {
        const dim3 slotGrid((unsigned)(params.nSlots / kBlock));
        withBool(ldsMaterials, [&](auto LDS_MATERIALS) {
            if (scene->hasMotion) {
                withBool(scene->traits.envOnly, [&](auto ENV_ONLY) {
                    hipLaunchKernelGGL((k_shade_instanced_motion<LDS_MATERIALS, ENV_ONLY>), slotGrid, dim3(kBlock), 0, stream, params, scene->instanceSet, scene->motionSet);
                });
                return;
            }
            if (scene->traits.envOnly) { hipLaunchKernelGGL((k_shade_instanced<LDS_MATERIALS, true>), slotGrid, dim3(kBlock), 0, stream, params, scene->instanceSet); }
            else { hipLaunchKernelGGL((k_shade_instanced<LDS_MATERIALS, false>), slotGrid, dim3(kBlock), 0, stream, params, scene->instanceSet); }
        });
        return;
    }
    const dim3 grid((unsigned)(params.nSlots / kBlock)), block(kBlock);
    // (k_shade narrowed further to {Lambertian, plastic, environment} -- 88 VGPRs against 92 -- shortens the shade launches of
    // the 5.2 M-triangle mesh by 13 % and LENGTHENS the other pool's trace launches by 23 %: -4.8 % overall, not adopted,
    // profiles/r3_ab_scene_traits.log)
    // ([r5] again with local rays, when the trace kernel has a fifth of its rays left: {Lambertian, plastic, environment} 2 312
    // against 2 456 Msamples/s on the same mesh, the sphere-free environment set +-0: profiles/r5_ab_local_rays.log)
    // [r5] environment-only scenes: k_shade_env -- the same vertex code, the next sample's camera ray started (and, if it is a
    // local ray that hits a large triangle, its first vertex shaded) in the launch that ends a sample; shade_chain = 1: the
    // plain k_shade<.., ENV_ONLY> (A/B runs, same floats)
    withBool(ldsMaterials, [&](auto LDS_MATERIALS) {
        if (scene->traits.envOnly && scene->options.shade_chain != 1) { hipLaunchKernelGGL((k_shade_env<LDS_MATERIALS>), grid, block, 0, stream, params); }
        else if (scene->traits.envOnly) { hipLaunchKernelGGL((k_shade<LDS_MATERIALS, true>), grid, block, 0, stream, params); }
        else { hipLaunchKernelGGL((k_shade<LDS_MATERIALS, false>), grid, block, 0, stream, params); }
    });
}

// what node_format 0 picks for the scenes the compressed trees serve: 0 float nodes, 1 nodeQ, 2 node8 (DESIGN.md has the measurements)
#ifndef PATHED_DEFAULT_NODE_FORMAT
#define PATHED_DEFAULT_NODE_FORMAT 0
#endif

// PathedSceneOptions.node_format with the experiments' override: 0 automatic, 1 float nodes, 2 compressed, 3 compressed 8-wide
int requestedNodeFormat(const PathedSceneOptions &options)
{
    if (const char *text = tuningEnv("PATHED_NODE_FORMAT")) {
        if (!strcmp(text, "wide")) { return 1; }
        if (!strcmp(text, "compressed")) { return 2; }
        if (!strcmp(text, "compressed8")) { return 3; }
    }
    return options.node_format;
}

void configureTrace(PathedScene *scene)
{
    // a 4-wide node stacks up to three children: 3 entries per level bound the stack.  22 rows
    // (+1 scratch, +8 KB staging = 31 KB per block) keep five blocks per CU possible; the rare
    // deeper entries spill to HBM.
    // (an 8-wide node stacks all of its up to eight hits and pops one back: 7 per level, 8 for a moment)
    const PathedSceneOptions &options = scene->options;
    const int requested = requestedNodeFormat(options);
    const bool mayWalkNode8 = requested == 3 || (requested == 0 && PATHED_DEFAULT_NODE_FORMAT == 2);
    scene->maxStack = mayWalkNode8 ? 7 * scene->bvh.maxDepth + 9 : 3 * scene->bvh.maxDepth + 1;
    if (scene->instanced) { scene->maxStack = scene->instancedMaxStack; }
    scene->stackRows = scene->maxStack <= 8 ? 8 : scene->maxStack <= 16 ? 16 : 22;
    if (options.stack_rows == 8 || options.stack_rows == 16 || options.stack_rows == 22) { scene->stackRows = options.stack_rows; }
    if (const char *override = tuningEnv("PATHED_STACK_ROWS")) {   // experiments: force the HBM spill path
        const int value = atoi(override);
        if (value == 8 || value == 16 || value == 22) { scene->stackRows = value; }
    }

    // per-thread traversal stacks + the waves' ray staging rows (2 float4 per thread)
    const size_t stackBytes = stackLdsBytes(scene->stackRows) + (size_t)2 * kBlock * kCardRounds * sizeof(float4)
        + (scene->splitShade ? (size_t)kWavesPerBlock * 2 * 128 * sizeof(unsigned int) : 0);
    const size_t sceneBytes = (size_t)scene->device.nNodes * 128 + (size_t)scene->device.nTris * 48;
    // stage the BVH in LDS when it is small enough to leave >= 4 blocks per CU
    scene->sceneInLds = scene->device.nNodes > 0 && (stackBytes + sceneBytes) <= 36 * 1024 && !scene->instanced;   // (k_trace_instanced walks HBM)
    scene->traceLdsBytes = stackBytes + (scene->sceneInLds ? sceneBytes : 0);

    int blocksPerCu = (int)((160 * 1024) / (scene->traceLdsBytes ? scene->traceLdsBytes : 1));
    if (blocksPerCu > 8) { blocksPerCu = 8; }
    // measured on MI355X (4-wide tree; teapot / 5.2 M-triangle mesh / the same mesh filling the frame, Msamples/s, 8 Mi
    // slots, queues in step): with the other pool's k_shade sharing the CUs TWO blocks per CU are best -- 1 786 / 2 172 /
    // 1 417 against 1 725 / 2 093 / 1 378 with three (the round-1 optimum, when k_shade was the slower partner by less)
    // and 1 411 / 1 829 / 1 106 with one: two 96-VGPR trace waves leave a SIMD room for THREE 104-VGPR k_shade waves.
    // 448 .. 640 blocks are within 2 % (PATHED_TRACE_GRID).  A single pool wants at least four (tools/occupancy_sweep.sh).
    if (!scene->sceneInLds) { blocksPerCu = scene->pools > 1 ? (blocksPerCu < 2 ? blocksPerCu : 2) : (blocksPerCu < 5 ? blocksPerCu : 5); }
    // (k_trace_instanced: one ray per lane and no refill, so latency is hidden by waves alone: four blocks per CU)
    if (scene->instanced) { blocksPerCu = 4; }
    if (blocksPerCu < 1) { blocksPerCu = 1; }
    if (options.trace_blocks_per_cu >= 1 && options.trace_blocks_per_cu <= 16) { blocksPerCu = options.trace_blocks_per_cu; }
    if (const char *override = tuningEnv("PATHED_TRACE_BLOCKS_PER_CU")) {
        const int value = atoi(override);
        if (value >= 1 && value <= 16) { blocksPerCu = value; }
    }
    scene->traceGrid = scene->computeUnits * blocksPerCu;
    if (const char *override = tuningEnv("PATHED_TRACE_GRID")) {   // experiments: the persistent grid in blocks, any number
        const int value = atoi(override);
        if (value >= 1 && value <= scene->computeUnits * 16) { scene->traceGrid = value; }
    }
    if (options.park_min_cards != 0) { scene->parkMinCards = options.park_min_cards < 0 ? 0 : (options.park_min_cards > 1024 ? 1024 : options.park_min_cards); }
    if (options.suspend_patience != 0) { scene->suspendPatience = options.suspend_patience < 0 ? 0 : (options.suspend_patience > 4096 ? 4096 : options.suspend_patience); }
    if (options.suspend_lanes != 0) { scene->suspendLanes = options.suspend_lanes < 0 ? 0 : (options.suspend_lanes > 64 ? 64 : options.suspend_lanes); }
    if (const char *override = tuningEnv("PATHED_PARK_MIN_CARDS")) {
        const int value = atoi(override);
        if (value >= 0 && value <= 1024) { scene->parkMinCards = value; }
    }
    if (const char *override = tuningEnv("PATHED_SUSPEND_PATIENCE")) {
        const int value = atoi(override);
        if (value >= 0 && value <= 4096) { scene->suspendPatience = value; }
    }
    if (const char *override = tuningEnv("PATHED_SUSPEND_LANES")) {
        const int value = atoi(override);
        if (value >= 0 && value <= 64) { scene->suspendLanes = value; }
    }
}

}  // namespace

extern "C" {

const char *pathed_hip_last_error(void) { return g_error.c_str(); }

#define PATHED_STRINGIFY2(x) #x
#define PATHED_STRINGIFY(x) PATHED_STRINGIFY2(x)
const char *pathed_hip_version(void) { return "pathed_hip 0.3.0 (gfx950, abi " PATHED_STRINGIFY(PATHED_ABI_VERSION) ")"; }

int pathed_hip_init(int device_id)
{
    int count = 0;
    hipError_t status = hipGetDeviceCount(&count);
    if (status != hipSuccess || count == 0) {
        return fail(PATHED_E_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(status));
    }
    if (device_id < 0 || device_id >= count) { return fail(PATHED_E_INVALID, "device id out of range"); }
    HIP_TRY(hipSetDevice(device_id));
    g_device = device_id;
    return PATHED_OK;
}

int pathed_hip_measure_bandwidth(size_t bytes, int repeats, double *read_gbs, double *copy_gbs)
{
    if (!read_gbs || !copy_gbs || repeats < 1 || repeats > 1000) { return fail(PATHED_E_INVALID, "bad argument"); }
    if (bytes < (1u << 20) || bytes > ((size_t)64 << 30)) { return fail(PATHED_E_INVALID, "probe size must be 1 MiB .. 64 GiB"); }
    if (g_device < 0) {
        const int code = pathed_hip_init(0);
        if (code != PATHED_OK) { return code; }
    }
    const size_t count = bytes / sizeof(float4);
    DeviceBuffer<float4> source, target;
    DeviceBuffer<float> sink;
    hipError_t status = source.allocate(count);
    if (status == hipSuccess) { status = target.allocate(count); }
    if (status == hipSuccess) { status = sink.allocate(1); }
    if (status == hipSuccess) { status = hipMemset(source.ptr, 0, count * sizeof(float4)); }
    if (status == hipSuccess) { status = hipMemset(target.ptr, 0, count * sizeof(float4)); }
    EventTimer timer;
    if (status == hipSuccess) { status = timer.status; }
    if (status != hipSuccess) { return fail(PATHED_E_DEVICE, std::string("bandwidth probe: ") + hipGetErrorString(status)); }

    hipDeviceProp_t properties;
    int units = 256;
    if (hipGetDeviceProperties(&properties, g_device) == hipSuccess && properties.multiProcessorCount > 0) { units = properties.multiProcessorCount; }
    const dim3 grid((unsigned)(units * 16)), block(kBlock);
    hipLaunchKernelGGL(k_stream_read, grid, block, 0, nullptr, source.ptr, count, sink.ptr);   // warm-up
    hipLaunchKernelGGL(k_stream_copy, grid, block, 0, nullptr, source.ptr, target.ptr, count);
    const float readMs = timer.run([&]() { for (int r = 0; r < repeats; r++) { hipLaunchKernelGGL(k_stream_read, grid, block, 0, nullptr, source.ptr, count, sink.ptr); } });
    const float copyMs = timer.run([&]() { for (int r = 0; r < repeats; r++) { hipLaunchKernelGGL(k_stream_copy, grid, block, 0, nullptr, source.ptr, target.ptr, count); } });
    if (!timer.ok() || !(readMs > 0.f) || !(copyMs > 0.f)) {
        return fail(PATHED_E_DEVICE, std::string("bandwidth probe: ") + hipGetErrorString(timer.status));
    }
    const double moved = (double)count * sizeof(float4) * repeats;
    *read_gbs = moved / (readMs * 1e-3) / 1e9;
    *copy_gbs = 2.0 * moved / (copyMs * 1e-3) / 1e9;   // bytes read + bytes written
    return PATHED_OK;
}

int pathed_hip_measure_valu(int waves_per_simd, int repeats, double *fma_rate, double *mixed_rate)
{
    if (!fma_rate || !mixed_rate) { return fail(PATHED_E_INVALID, "bad argument"); }
    double rates[5] = { 0.0, 0.0, 0.0, 0.0, 0.0 };
    const int code = pathed_hip_measure_valu_modes(waves_per_simd, repeats, rates, 2);
    *fma_rate = rates[0];
    *mixed_rate = rates[1];
    return code;
}

int pathed_hip_measure_valu_modes(int waves_per_simd, int repeats, double *rates, int n_modes)
{
    if (!rates || repeats < 1 || repeats > 1000 || n_modes < 1 || n_modes > 5) { return fail(PATHED_E_INVALID, "bad argument"); }
    if (waves_per_simd < 1 || waves_per_simd > 8) { return fail(PATHED_E_INVALID, "waves_per_simd must be 1..8"); }
    if (g_device < 0) {
        const int code = pathed_hip_init(0);
        if (code != PATHED_OK) { return code; }
    }
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    hipDeviceProp_t properties;
    int units = 256;
    if (hipGetDeviceProperties(&properties, device) == hipSuccess && properties.multiProcessorCount > 0) { units = properties.multiProcessorCount; }
    DeviceBuffer<float> sinkBuffer;
    EventTimer timer;
    timer.keep(sinkBuffer.allocate(1));
    float *sink = sinkBuffer.ptr;
    // one 256-thread block = one wave on each of a CU's four SIMDs; k blocks per CU = k waves per SIMD
    const dim3 grid((unsigned)(units * waves_per_simd)), block(kBlock);
    const int iterations = 8192;   // 393 216 instructions per wave and launch
    auto launch = [&](int mode) {
        switch (mode) {
        case 0: hipLaunchKernelGGL((k_valu_probe<0>), grid, block, 0, nullptr, iterations, 1.f, sink); break;
        case 1: hipLaunchKernelGGL((k_valu_probe<1>), grid, block, 0, nullptr, iterations, 1.f, sink); break;
        case 2: hipLaunchKernelGGL((k_valu_probe<2>), grid, block, 0, nullptr, iterations, 1.f, sink); break;
        case 3: hipLaunchKernelGGL((k_valu_probe<3>), grid, block, 0, nullptr, iterations, 1.f, sink); break;
        default: hipLaunchKernelGGL((k_valu_probe<4>), grid, block, 0, nullptr, iterations, 1.f, sink); break;
        }
    };
    const double issued = (double)grid.x * kWavesPerBlock * (double)iterations * kValuProbeUnroll * repeats;
    for (int mode = 0; mode < n_modes && timer.ok(); mode++) {
        launch(mode);   // warm-up
        const float ms = timer.run([&]() { for (int r = 0; r < repeats; r++) { launch(mode); } });
        if (timer.ok() && !(ms > 0.f)) { timer.keep(hipErrorUnknown); }
        if (timer.ok()) { rates[mode] = issued / (ms * 1e-3); }
    }
    if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string("VALU probe: ") + hipGetErrorString(timer.status)); }
    return PATHED_OK;
}

int pathed_hip_measure_valu_clocks(int waves_per_simd, int chains, int repeats, PathedValuClocks *out)
{
#if !PATHED_EXPERIMENTS
    (void)waves_per_simd; (void)chains; (void)repeats; (void)out;
    return fail(PATHED_E_UNSUPPORTED, "the clocked VALU probe lives in libpathed_hip_experiments.so (`make experiments`)");
#else
    if (!out || repeats < 1 || repeats > 1000) { return fail(PATHED_E_INVALID, "bad argument"); }
    if (waves_per_simd < 1 || waves_per_simd > 8) { return fail(PATHED_E_INVALID, "waves_per_simd must be 1..8"); }
    if (chains != 8 && chains != 16) { return fail(PATHED_E_INVALID, "chains must be 8 or 16"); }
    if (g_device < 0) {
        const int code = pathed_hip_init(0);
        if (code != PATHED_OK) { return code; }
    }
    std::memset(out, 0, sizeof *out);
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    hipDeviceProp_t properties;
    int units = 256;
    if (hipGetDeviceProperties(&properties, device) == hipSuccess && properties.multiProcessorCount > 0) { units = properties.multiProcessorCount; }
    int wallKhz = 0;
    if (hipDeviceGetAttribute(&wallKhz, hipDeviceAttributeWallClockRate, device) != hipSuccess || wallKhz <= 0) { wallKhz = 100000; }   // 100 MHz on CDNA
    int peakKhz = 0;
    (void)hipDeviceGetAttribute(&peakKhz, hipDeviceAttributeClockRate, device);
    const dim3 grid((unsigned)(units * waves_per_simd)), block(kBlock);
    const size_t waves = (size_t)grid.x * kWavesPerBlock;
    const int iterations = 8192;   // 393 216 instructions per wave and launch
    DeviceBuffer<float> sinkBuffer;
    DeviceBuffer<unsigned long long> clockBuffer;
    EventTimer timer;
    if (timer.keep(sinkBuffer.allocate(1))) { timer.keep(clockBuffer.allocate(2 * waves)); }
    float *sink = sinkBuffer.ptr;
    unsigned long long *clocks = clockBuffer.ptr;
    auto launch = [&]() {
        if (chains == 16) { hipLaunchKernelGGL((k_valu_clock_probe<16>), grid, block, 0, nullptr, iterations, 1.f, sink, clocks); }
        else { hipLaunchKernelGGL((k_valu_clock_probe<8>), grid, block, 0, nullptr, iterations, 1.f, sink, clocks); }
    };
    if (timer.ok()) { launch(); }   // warm-up
    const float ms = timer.run([&]() { for (int r = 0; r < repeats; r++) { launch(); } });
    std::vector<unsigned long long> host(2 * waves);
    if (timer.ok()) { timer.keep(hipMemcpy(host.data(), clocks, host.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost)); }
    if (timer.ok() && ms > 0.f) {
        const double perWave = (double)iterations * kValuProbeUnroll;   // instructions of the last launch's waves
        double shaderTicks = 0.0, wallTicks = 0.0;
        for (size_t w = 0; w < waves; w++) { shaderTicks += (double)host[2 * w]; wallTicks += (double)host[2 * w + 1]; }
        out->rate = (double)waves * perWave * repeats / (ms * 1e-3);
        out->wall_clock_mhz = wallKhz / 1e3;
        out->peak_clock_mhz = peakKhz / 1e3;
        out->shader_clock_mhz = wallTicks > 0.0 ? shaderTicks / wallTicks * out->wall_clock_mhz : 0.0;
        // a wave issues its instructions while waves_per_simd - 1 others share its SIMD: the SIMD's cycles per instruction
        // are the wave's ticks per instruction divided by the waves that share it
        out->wave_ticks_per_instruction = shaderTicks / ((double)waves * perWave);
        out->cycles_per_instruction = out->wave_ticks_per_instruction / waves_per_simd;
        // ... and from the event time alone, against the frequency measured in the same launches
        const double simds = (double)units * 4.0;
        out->cycles_per_instruction_events = out->shader_clock_mhz > 0.0 ? simds * out->shader_clock_mhz * 1e6 / out->rate : 0.0;
    }
    if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string("VALU clock probe: ") + hipGetErrorString(timer.status)); }
    return PATHED_OK;
#endif
}

int pathed_hip_accum_alloc(PathedScene *scene, size_t count, float **out)
{
    if (!scene || !out || count == 0) { return fail(PATHED_E_INVALID, "bad argument"); }
    SELECT_DEVICE(scene);
    float *buffer = nullptr;
    HIP_TRY(hipMalloc((void **)&buffer, count * sizeof(float)));
    const hipError_t status = hipMemset(buffer, 0, count * sizeof(float));
    if (status != hipSuccess) { (void)hipFree(buffer); return fail(PATHED_E_DEVICE, hipGetErrorString(status)); }
    *out = buffer;
    return PATHED_OK;
}

int pathed_hip_accum_free(PathedScene *scene, float *buffer)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    SELECT_DEVICE(scene);
    if (buffer) { HIP_TRY(hipFree(buffer)); }
    return PATHED_OK;
}

int pathed_hip_accum_download(PathedScene *scene, const float *buffer, size_t count, float *host)
{
    if (!scene || !buffer || !host) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(scene);
    HIP_TRY(hipMemcpy(host, buffer, count * sizeof(float), hipMemcpyDeviceToHost));
    return PATHED_OK;
}

int pathed_hip_accum_upload(PathedScene *scene, float *buffer, size_t count, const float *host)
{
    if (!scene || !buffer || !host) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(scene);
    HIP_TRY(hipMemcpy(buffer, host, count * sizeof(float), hipMemcpyHostToDevice));
    return PATHED_OK;
}

int pathed_hip_accum_copy_peer(PathedScene *dst_scene, float *dst, PathedScene *src_scene, const float *src, size_t count)
{
    if (!dst_scene || !src_scene || !dst || !src) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(dst_scene);
    if (dst_scene->deviceId == src_scene->deviceId) {
        HIP_TRY(hipMemcpy(dst, src, count * sizeof(float), hipMemcpyDeviceToDevice));
    } else {
        HIP_TRY(hipMemcpyPeer(dst, dst_scene->deviceId, src, src_scene->deviceId, count * sizeof(float)));
    }
    return PATHED_OK;
}

int pathed_hip_accum_add(PathedScene *dst_scene, float *dst, const float *src, size_t count)
{
    if (!dst_scene || !dst || !src) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(dst_scene);
    if (count == 0) { return PATHED_OK; }
    size_t blocks = (count + kBlock - 1) / kBlock;
    if (blocks > (size_t)dst_scene->computeUnits * 16) { blocks = (size_t)dst_scene->computeUnits * 16; }
    hipLaunchKernelGGL(k_accum_add, dim3((unsigned)blocks), dim3(kBlock), 0, nullptr, dst, src, count);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    return PATHED_OK;
}

// ---- RCCL reduce of the per-device radiance sums (include/pathed_hip.h: multi-GPU fan-in) ----
// librccl is opened on first use: its types are restated here so that neither this library nor a single-GPU
// host links against it (rccl.h: ncclFloat32 = 7, ncclSum = 0, ncclSuccess = 0).
namespace {
struct RcclApi {
    void *library = nullptr;
    int (*commInitAll)(void **, int, const int *) = nullptr;
    int (*commDestroy)(void *) = nullptr;
    int (*reduce)(const void *, void *, size_t, int, int, int, void *, hipStream_t) = nullptr;
    int (*groupStart)() = nullptr;
    int (*groupEnd)() = nullptr;
    const char *(*errorString)(int) = nullptr;
};
RcclApi g_rccl;
std::mutex g_rcclMutex;

bool loadRccl(std::string *why)
{
    std::lock_guard<std::mutex> guard(g_rcclMutex);
    if (g_rccl.library) { return true; }
    void *library = nullptr;
    for (const char *name : { "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1" }) {
        library = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (library) { break; }
    }
    if (!library) { *why = std::string("cannot load librccl: ") + dlerror(); return false; }
    RcclApi api;
    api.library = library;
    api.commInitAll = reinterpret_cast<int (*)(void **, int, const int *)>(dlsym(library, "ncclCommInitAll"));
    api.commDestroy = reinterpret_cast<int (*)(void *)>(dlsym(library, "ncclCommDestroy"));
    api.reduce = reinterpret_cast<int (*)(const void *, void *, size_t, int, int, int, void *, hipStream_t)>(dlsym(library, "ncclReduce"));
    api.groupStart = reinterpret_cast<int (*)()>(dlsym(library, "ncclGroupStart"));
    api.groupEnd = reinterpret_cast<int (*)()>(dlsym(library, "ncclGroupEnd"));
    api.errorString = reinterpret_cast<const char *(*)(int)>(dlsym(library, "ncclGetErrorString"));
    if (!api.commInitAll || !api.commDestroy || !api.reduce || !api.groupStart || !api.groupEnd || !api.errorString) {
        *why = "librccl lacks one of ncclCommInitAll / ncclCommDestroy / ncclReduce / ncclGroupStart / ncclGroupEnd / ncclGetErrorString";
        dlclose(library);
        return false;
    }
    g_rccl = api;
    return true;
}
}  // namespace

struct PathedComm {
    std::vector<int> devices;
    std::vector<void *> comms;          // ncclComm_t per device
    std::vector<hipStream_t> streams;   // one per device
};

int pathed_hip_comm_init(int n_devices, const int *device_ids, PathedComm **out)
{
    if (!out) { return fail(PATHED_E_INVALID, "out pointer is null"); }
    *out = nullptr;
    if (n_devices < 1 || !device_ids) { return fail(PATHED_E_INVALID, "a communicator needs at least one device"); }
    int visible = 0;
    HIP_TRY(hipGetDeviceCount(&visible));
    for (int i = 0; i < n_devices; i++) {
        if (device_ids[i] < 0 || device_ids[i] >= visible) { return fail(PATHED_E_INVALID, "device id out of range"); }
        for (int k = 0; k < i; k++) {
            if (device_ids[k] == device_ids[i]) { return fail(PATHED_E_UNSUPPORTED, "RCCL takes one rank per device: replicas that share a GPU use pathed_hip_accum_copy_peer"); }
        }
    }
    std::string why;
    if (!loadRccl(&why)) { return fail(PATHED_E_UNSUPPORTED, why); }
    PathedComm *comm = new PathedComm();
    comm->devices.assign(device_ids, device_ids + n_devices);
    comm->comms.assign((size_t)n_devices, nullptr);
    comm->streams.assign((size_t)n_devices, nullptr);
    const int status = g_rccl.commInitAll(comm->comms.data(), n_devices, device_ids);
    if (status != 0) {
        const std::string message = std::string("ncclCommInitAll: ") + g_rccl.errorString(status);
        delete comm;
        return fail(PATHED_E_DEVICE, message);
    }
    for (int i = 0; i < n_devices; i++) {
        hipError_t error = hipSetDevice(device_ids[i]);
        if (error == hipSuccess) { error = hipStreamCreateWithFlags(&comm->streams[(size_t)i], hipStreamNonBlocking); }
        if (error != hipSuccess) {
            const std::string message = std::string("communicator stream: ") + hipGetErrorString(error);
            pathed_hip_comm_destroy(comm);
            return fail(PATHED_E_DEVICE, message);
        }
    }
    *out = comm;
    return PATHED_OK;
}

int pathed_hip_comm_reduce(PathedComm *comm, const float *const *send, float *recv_root, size_t count)
{
    if (!comm || !send || !recv_root) { return fail(PATHED_E_INVALID, "null communicator or buffer"); }
    const size_t n = comm->devices.size();
    for (size_t r = 0; r < n; r++) { if (!send[r]) { return fail(PATHED_E_INVALID, "null send buffer"); } }
    // whatever the caller queued on the devices' null streams (its renders are blocking) is done; the collective runs on
    // the communicator's own streams
    int status = g_rccl.groupStart();
    for (size_t r = 0; r < n && status == 0; r++) {
        status = g_rccl.reduce(send[r], r == 0 ? recv_root : nullptr, count, /* ncclFloat32 */ 7, /* ncclSum */ 0, /* root */ 0,
                               comm->comms[r], comm->streams[r]);
    }
    const int ended = g_rccl.groupEnd();
    if (status == 0) { status = ended; }
    if (status != 0) { return fail(PATHED_E_DEVICE, std::string("ncclReduce: ") + g_rccl.errorString(status)); }
    for (size_t r = 0; r < n; r++) {
        HIP_TRY(hipSetDevice(comm->devices[r]));
        HIP_TRY(hipStreamSynchronize(comm->streams[r]));
    }
    return PATHED_OK;
}

void pathed_hip_comm_destroy(PathedComm *comm)
{
    if (!comm) { return; }
    for (size_t r = 0; r < comm->devices.size(); r++) {
        if (comm->streams[r]) { (void)hipSetDevice(comm->devices[r]); (void)hipStreamDestroy(comm->streams[r]); }
        if (comm->comms[r] && g_rccl.commDestroy) { (void)g_rccl.commDestroy(comm->comms[r]); }
    }
    delete comm;
}

int pathed_hip_scene_create(const PathedSceneDesc *desc, PathedScene **out)
{
    return pathed_hip_scene_create_ex(desc, nullptr, out);
}

int pathed_hip_scene_device(const PathedScene *scene)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    return scene->deviceId;
}

static int unitOrderFromEnvironment(int fallback)
{
    if (const char *text = tuningEnv("PATHED_UNIT_ORDER")) {   // experiments
        if (!strcmp(text, "tiles")) { return kOrderTiles; }
        if (!strcmp(text, "stripes-tiled")) { return kOrderStripesTiled; }
        if (!strcmp(text, "stripes")) { return kOrderStripes; }
    }
    return fallback;
}

// The fused kernel's phase-1 records depend on the camera (the tolerances of the parallelograms scale with the distance a ray
// origin may have from a triangle): built at scene_create and again when the camera moves.
static hipError_t rebuildSmallItems(PathedScene *scene)
{
    if (!scene->bruteForce || scene->device.nTris <= 0) { return hipSuccess; }
    std::vector<float> points = scene->smallExtraPoints;
    for (int a = 0; a < 3; a++) { points.push_back(scene->device.camera.origin[a]); }
    // (the parallelogram instantiations of k_path_small keep the material table in LDS beside the path-state stash and the
    // shared resolve's lists, 33.5 KiB per block: up to 64 materials -- 6 KiB -- four blocks fit a CU's 160 KiB; scenes with more
    // pair nothing)
    const int kMaxQuadMaterials = 64;
    const bool pairQuads = scene->options.generic_kernels == 0 && !tuningEnv("PATHED_NO_QUADS") && scene->device.nMaterials <= kMaxQuadMaterials;
    std::vector<float> ordered;
    // where the shadow rays end (small_items.h: NEVER-OCCLUDERS): the items no shadow ray has to test go last in item order
    std::vector<unsigned char> emitter((size_t)scene->device.nTris, 0);
    bool lightsKnown = true;
    for (int k = 0; k < scene->device.nTris; k++) {
        int prim;
        std::memcpy(&prim, &scene->bvh.leafTris[(size_t)12 * k + 3], sizeof prim);
        if (prim < 0 || (size_t)prim >= scene->smallEmitterPrims.size()) { lightsKnown = false; break; }
        emitter[(size_t)k] = scene->smallEmitterPrims[(size_t)prim];
    }
    SmallLights lights;
    lights.known = lightsKnown;
    lights.environment = scene->device.hasEnv != 0;
    lights.emitter = emitter.data();
    lights.spheres = scene->smallSphereLights.data();
    lights.nSpheres = (int)(scene->smallSphereLights.size() / 4);
    lights.nSurfacePoints = (int)(scene->smallExtraPoints.size() / 3);
    scene->smallLayout = buildSmallItems(scene->bvh.leafTris.data(), scene->device.nTris, points.data(), (int)(points.size() / 3), pairQuads, PATHED_TNEAR,
                                         reinterpret_cast<float *>(scene->smallItems.data), &ordered, &lights);
    scene->itemTrisHost = ordered;
    // the pass list (small_items.h: NEVER-HIT), from the same inputs; its triangles go behind the scene's own (PathedScene::passItems)
    scene->passLayout = buildSmallPassItems(scene->bvh.leafTris.data(), scene->device.nTris, points.data(), (int)(points.size() / 3), pairQuads, PATHED_TNEAR,
                                            reinterpret_cast<float *>(scene->passItems.data), &scene->passTrisHost, &lights, &scene->passTris, &scene->passNeverHit);
    std::vector<float> both((size_t)24 * scene->device.nTris, 0.f);
    std::memcpy(both.data(), ordered.data(), sizeof(float) * 12 * (size_t)scene->device.nTris);
    std::memcpy(both.data() + (size_t)12 * scene->device.nTris, scene->passTrisHost.data(), sizeof(float) * 12 * (size_t)scene->passTris);
    const hipError_t status = scene->itemTris.upload(asQuads(both));
    if (status == hipSuccess && scene->mfmaPhase1) {
        // (experiments build) the matrix-pipe rows are expressed in a frame centred on the camera: a new camera is a new table,
        // or phase 1 stops being conservative for rays that start far from the old one
        std::vector<float> table;
        buildMfmaTable(scene->itemTrisHost.data(), scene->device.nTris, scene->device.camera.origin, 1, &table, &scene->mfmaFrame);
        return scene->mfmaTable.upload(table);
    }
    return status;
}

// The fused kernel's camera-ray candidate masks (camera_masks.h) live in the camera queues' allocation, ahead of the queues:
// this sizes it and builds them on the device.  They depend on (item-order triangles, camera, resolution): built at
// scene_create, again when the camera moves (after rebuildSmallItems: the item order is its), and by renderPassFused should
// the allocation ever be found too small.  PATHED_DEBUG_STATS=1 reports the last build's device time with the statistics.
static size_t cameraQueueWords(const PathedScene *scene)
{
    const size_t queueBlocks = (size_t)(scene->computeUnits > 0 ? scene->computeUnits : 1) * PATHED_FUSED_WAVES;
    return queueBlocks * kWavesPerBlock * kCameraQueueWords;
}

static size_t cameraMaskQuads(const PathedScene *scene) { return cameraMaskWords(scene->width * scene->height) / 2; }   // float4 = two masks

static hipError_t rebuildCameraMasks(PathedScene *scene)
{
    if (!scene->bruteForce || !scene->fusedPath) { return hipSuccess; }
    hipError_t status;
    scene->cameraMasksBuilt = false;   // until the build below has run to its end: a failure leaves no table marked as valid
    const size_t quads = cameraMaskQuads(scene) + cameraQueueWords(scene);
    if (scene->cameraQueue.count < quads && (status = scene->cameraQueue.allocate(quads)) != hipSuccess) { return status; }
    const int nPixels = scene->width * scene->height;
    const size_t words = cameraMaskWords(nPixels);
    EventTimer timer;
    timer.run([&]() {
        hipLaunchKernelGGL(k_build_camera_masks, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, nullptr, scene->device.camera,
                           scene->itemTris.ptr, scene->device.nTris, nPixels, reinterpret_cast<unsigned long long *>(scene->cameraQueue.ptr));
    });
    if (timer.ok()) { timer.keep(hipDeviceSynchronize()); }
    if (!timer.ok()) { return timer.status; }
    scene->cameraMaskMs = timer.ms;
    scene->cameraMasksBuilt = true;
    return hipSuccess;
}

// [r5] the phase-1 records of the hybrid kernel's direct set (they depend on the camera only through the scene's extent)
static hipError_t rebuildHybridItems(PathedScene *scene)
{
    if (!scene->hybridAvailable || scene->hybridDirectTris <= 0) { return hipSuccess; }
    std::vector<float> points = scene->hybridBounds;
    for (int a = 0; a < 3; a++) { points.push_back(scene->device.camera.origin[a]); }
    std::vector<float> ordered;
    scene->hybridLayout = buildSmallItems(scene->hybridDirectLeaf.data(), scene->hybridDirectTris, points.data(), (int)(points.size() / 3), true, PATHED_TNEAR,
                                          reinterpret_cast<float *>(scene->hybridItems.data), &ordered);
    return scene->hybridItemTris.upload(asQuads(ordered));
}

// [r5] The wavefront's local rays: a sphere-free BVH scene with at most kMaxLocalTris LARGE triangles (each at least 1 / 256 of
// the scene's surface: a floor, a backdrop) keeps their records for k_shade, with the bounds of everything else -- a box and
// a sphere about its centre, padded: the tests that use them only cull.
static void buildLocalSet(PathedScene *scene, const PathedSceneDesc *desc)
{
    scene->localCount = 0;
    const uint32_t n = desc->n_triangles;
    if (n == 0 || desc->n_spheres != 0) { return; }
    const TriangleAreas areas = triangleAreas(desc);
    std::vector<uint32_t> large, rest;   // triangles; vertex indices
    for (uint32_t i = 0; i < n; i++) {
        if (areas.large(i)) {
            large.push_back(i);
            if (large.size() > (size_t)kMaxLocalTris) { return; }   // a scene of many large faces: no "rest" worth culling against
        } else {
            rest.insert(rest.end(), desc->indices + 3 * (size_t)i, desc->indices + 3 * (size_t)i + 3);
        }
    }
    if (large.empty() || large.size() == n) { return; }
    const RestProxy proxy = restProxy(desc->positions, rest);
    std::memcpy(scene->localLo, proxy.lo, sizeof proxy.lo);
    std::memcpy(scene->localHi, proxy.hi, sizeof proxy.hi);
    std::memcpy(scene->localSphere, proxy.sphere, sizeof proxy.sphere);
    for (size_t k = 0; k < large.size(); k++) {
        const uint32_t i = large[k];
        const float *v0 = desc->positions + 3 * (size_t)desc->indices[3 * i], *v1 = desc->positions + 3 * (size_t)desc->indices[3 * i + 1], *v2 = desc->positions + 3 * (size_t)desc->indices[3 * i + 2];
        float prim;
        const int id = (int)i;
        std::memcpy(&prim, &id, 4);
        // the record the tree's leaves hold for the triangle (bvh_build.h): v0, e1 = v1 - v0, e2 = v2 - v0 in fp32
        scene->localTris[3 * k + 0] = make_float4(v0[0], v0[1], v0[2], prim);
        scene->localTris[3 * k + 1] = make_float4(v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2], 0.f);
        scene->localTris[3 * k + 2] = make_float4(v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2], 0.f);
    }
    scene->localCount = (int)large.size();
}

// [r5] Splits a scene of 65 .. kHybridMaxTris triangles for k_path_hybrid: the (up to 64) largest triangles -- each at least
// 1 / 256 of the scene's surface: walls, floors, boxes, what most rays hit and what no box around it would cull -- are tested
// directly; everything else gets a tree of its own (the host SAH builder, the node format of the scene's tree).
static hipError_t buildHybrid(PathedScene *scene, const PathedSceneDesc *desc)
{
    const uint32_t n = desc->n_triangles;
    const TriangleAreas areas = triangleAreas(desc);
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };   // the box of every triangle's corners
    for (size_t k = 0; k < (size_t)3 * n; k++) {
        const float *v = desc->positions + 3 * (size_t)desc->indices[k];
        for (int x = 0; x < 3; x++) { lo[x] = std::min(lo[x], (double)v[x]); hi[x] = std::max(hi[x], (double)v[x]); }
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) { order[i] = i; }
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return areas.area[x] > areas.area[y]; });
    std::vector<char> isDirect(n, 0);
    int nDirect = 0;
    for (uint32_t k = 0; k < n && nDirect < kBruteForceMaxTris; k++) {
        if (!areas.large(order[k])) { break; }
        isDirect[order[k]] = 1;
        nDirect++;
    }
    // direct set, in primitive order
    scene->hybridDirectLeaf.clear();
    std::vector<uint32_t> treeIndices, treePrim;
    for (uint32_t i = 0; i < n; i++) {
        if (!isDirect[i]) {
            for (int k = 0; k < 3; k++) { treeIndices.push_back(desc->indices[3 * i + k]); }
            treePrim.push_back(i);
            continue;
        }
        const float *v0 = desc->positions + 3 * (size_t)desc->indices[3 * i], *v1 = desc->positions + 3 * (size_t)desc->indices[3 * i + 1], *v2 = desc->positions + 3 * (size_t)desc->indices[3 * i + 2];
        float record[12];
        for (int a = 0; a < 3; a++) { record[a] = v0[a]; record[4 + a] = v1[a] - v0[a]; record[8 + a] = v2[a] - v0[a]; }   // as bvh_build.h writes them
        bvh_detail::putInt(record + 3, (int)i);
        record[7] = 0.f; record[11] = 0.f;
        scene->hybridDirectLeaf.insert(scene->hybridDirectLeaf.end(), record, record + 12);
    }
    scene->hybridDirectTris = nDirect;
    scene->hybridTreeTris = (int)treePrim.size();
    scene->hybridBounds.clear();
    for (int corner = 0; corner < 8; corner++) {
        for (int a = 0; a < 3; a++) { scene->hybridBounds.push_back((float)(((corner >> a) & 1) ? hi[a] : lo[a])); }
    }
    scene->hybridNodeCount = 0;
    scene->hybridMaxStack = 1;
    hipError_t status = hipSuccess;
    if (!treePrim.empty()) {
        FlatBvh tree = buildBvh(desc->positions, treeIndices.data(), (uint32_t)treePrim.size(), nullptr, 0, scene->options.build_threads, 4u);   // (leaves of <= 4: bvh_build.h)
        // the builder numbered the part's triangles 0 .. : back to the scene's primitive ids (shading records, lights)
        for (size_t k = 0; k < treePrim.size(); k++) {
            int sub;
            std::memcpy(&sub, &tree.leafTris[12 * k + 3], 4);
            bvh_detail::putInt(&tree.leafTris[12 * k + 3], (int)treePrim[(size_t)sub]);
        }
        if ((status = scene->hybridNodes.upload(asQuads(tree.nodes))) != hipSuccess) { return status; }
        if ((status = scene->hybridTris.upload(asQuads(tree.leafTris))) != hipSuccess) { return status; }
        scene->hybridNodeCount = tree.nodeCount;
        scene->hybridMaxStack = 3 * tree.maxDepth + 1;
        const RestProxy proxy = restProxy(desc->positions, treeIndices);   // (padded: the proxy test is a cull, the walk's own slab tests decide)
        std::memcpy(scene->hybridLo, proxy.lo, sizeof proxy.lo);
        std::memcpy(scene->hybridHi, proxy.hi, sizeof proxy.hi);
        std::memcpy(scene->hybridSphere, proxy.sphere, sizeof proxy.sphere);
    }
    scene->hybridAvailable = true;
    return rebuildHybridItems(scene);
}

// Which compile-time scene sets (shading.h: SceneTraits) contain the scene.  generic_kernels = 1 leaves every flag off.
// The light sampling records (device_scene.h) from the shading records in scene->triShade: at scene creation and after every
// refit, behind k_build_tri_shade on the same stream.
static hipError_t buildLightRecords(PathedScene *scene, int nLights)
{
    if (nLights <= 0) { return hipSuccess; }
    hipLaunchKernelGGL(k_build_light_records, dim3((unsigned)((nLights + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                       scene->lights.ptr, nLights, scene->triShade.ptr, scene->lightRecords.ptr);
    return hipGetLastError();
}

static SceneTraitFlags sceneTraits(const PathedSceneDesc *desc, const std::vector<DMaterial> &materials, const std::vector<DLight> &lights,
                                   const PathedSceneOptions &options)
{
    const unsigned rough = (1u << PATHED_MAT_LAMBERTIAN) | (1u << PATHED_MAT_OREN_NAYAR) | (1u << PATHED_MAT_MICROFACET) | (1u << PATHED_MAT_PLASTIC);
    const unsigned smooth = (1u << PATHED_MAT_LAMBERTIAN) | (1u << PATHED_MAT_GLASS) | (1u << PATHED_MAT_MIRROR);
    const unsigned lambertianPlastic = (1u << PATHED_MAT_LAMBERTIAN) | (1u << PATHED_MAT_PLASTIC);
    const unsigned glassContainer = (1u << PATHED_MAT_LAMBERTIAN) | (1u << PATHED_MAT_GLASS) | (1u << PATHED_MAT_PASSTHROUGH);
    unsigned kinds = 0u, distributions = 0u;   // material types that occur; 1 Beckmann, 2 GGX among the microfacet / plastic materials
    bool emissive = false, constantAlbedo = true;
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        const PathedMaterial &material = desc->materials[i];
        kinds |= 1u << material.type;
        if (material.type == PATHED_MAT_MICROFACET || material.type == PATHED_MAT_PLASTIC) { distributions |= material.distribution == PATHED_DIST_GGX ? 2u : 1u; }
        emissive = emissive || emits(materials[i]);
        constantAlbedo = constantAlbedo && material.albedo_type == PATHED_ALBEDO_CONSTANT;
    }
    bool triangleLights = false;
    for (const DLight &light : lights) { triangleLights = triangleLights || light.kind == 0; }
    const bool noEnv = desc->env == nullptr, noSpheres = desc->n_spheres == 0;
    const bool narrow = options.generic_kernels == 0 && !tuningEnv("PATHED_NO_SCENE_TRAITS");

    SceneTraitFlags t;
    t.envOnly = !noEnv && lights.size() == 1 && !emissive && options.generic_kernels == 0 && !tuningEnv("PATHED_NO_ENV_ONLY");
    t.lambertianTriangles = narrow && noEnv && noSpheres && constantAlbedo && kinds == (1u << PATHED_MAT_LAMBERTIAN);
    t.lambertianPlasticSpheres = narrow && noEnv && !triangleLights && constantAlbedo && (kinds & ~lambertianPlastic) == 0u;
    t.triangleLit = narrow && noEnv && noSpheres && constantAlbedo && (kinds & (1u << PATHED_MAT_PASSTHROUGH)) == 0u;
    t.roughBeckmann = t.triangleLit && (kinds & ~rough) == 0u && (distributions & 2u) == 0u;
    t.roughGgx = t.triangleLit && (kinds & ~rough) == 0u && distributions == 2u;
    t.smoothSet = t.triangleLit && (kinds & ~smooth) == 0u;
    t.lambertianGlassContainer = narrow && noEnv && constantAlbedo && (kinds & ~glassContainer) == 0u;
    return t;
}

// ---- scene creation.  createScene, at the end, is the sequence of the stages below; the arithmetic
// that needs no device is scene_tables.h and, for a scene with instances, instances.h (planInstances, buildInstancedBvh).
// A stage that fails has called fail() and returns its code: the scene's one owner in createScene frees whatever had been
// allocated by then.

static int deviceFail(hipError_t status, const char *what)
{
    return fail(PATHED_E_DEVICE, std::string(what) + ": " + hipGetErrorString(status));
}

// THE TINY-SCENE PREDICATE.  fewTriangles: no more triangles than the all-triangles kernels test per ray.  tinyScene: such
// a scene whose spheres fit as well and that was not told to walk a tree.  The three places that ask:
//   chooseBuilder       fewTriangles alone: the host builder, whose host copy of the records the all-triangles kernels
//                       read.  It omits the other conditions, so a scene of 64 triangles and 17 spheres, or one with
//                       intersector = 1, is built on the host as well although a tree is walked: kept, the choice of the
//                       builder never changes an image and PathedStats.bvh_builder reports it.
//   buildTreeOnHost     tinyScene: the spheres stay out of the tree and are tested one by one.  It omits `instanced`, which
//                       cannot matter here: planInstances refuses a scene with instances that has a sphere.
//   chooseShadeKernel   tinyScene && !instanced = PathedScene::bruteForce.  A scene with instances of at most 64 stored
//                       triangles (world triangles and prototypes together: desc->n_triangles counts both) does occur; it
//                       takes the host builder by the first rule, has no spheres by planInstances, and walks its two-level
//                       tree by this one.  With 17 spheres the second and third rule are false together: the spheres are
//                       in the tree that is walked.
static bool fewTriangles(const PathedSceneDesc *desc) { return desc->n_triangles <= (uint32_t)kBruteForceMaxTris; }

static bool tinyScene(const PathedSceneDesc *desc, const PathedSceneOptions &options)
{
    return fewTriangles(desc) && desc->n_spheres <= (uint32_t)kBruteForceMaxSpheres && options.intersector != 1 && !tuningEnv("PATHED_NO_BRUTE_FORCE");
}

static int resolveOptions(const PathedSceneOptions *optionsIn, PathedSceneOptions *options)
{
    std::memset(options, 0, sizeof *options);
    options->device = PATHED_DEVICE_CURRENT;
    if (!optionsIn) { return PATHED_OK; }
    std::string message;
    const int code = checkSceneOptions(*optionsIn, &message);   // (struct_size first: nothing past it is read of a struct of another size)
    if (code != PATHED_OK) { return fail(code, message); }
    *options = *optionsIn;
    return PATHED_OK;
}

static int resolveDevice(const PathedSceneOptions &options, int *resolved)
{
    int deviceId = options.device;
    if (deviceId == PATHED_DEVICE_CURRENT) {
        if (g_device < 0) {
            const int code = pathed_hip_init(0);
            if (code != PATHED_OK) { return code; }
        }
        deviceId = g_device;
    } else {
        int count = 0;
        const hipError_t counted = hipGetDeviceCount(&count);
        if (counted != hipSuccess || count == 0) { return fail(PATHED_E_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(counted)); }
        if (deviceId < 0 || deviceId >= count) { return fail(PATHED_E_INVALID, "device id out of range"); }
    }
    HIP_TRY(hipSetDevice(deviceId));
    *resolved = deviceId;
    return PATHED_OK;
}

// image textures: one float4 array for all of them (scene_tables.h: gammaTexels)
static int uploadTextures(PathedScene *scene, const PathedSceneDesc *desc, std::vector<size_t> *textureOffset)
{
    std::vector<float> texels;
    gammaTexels(desc, &texels, textureOffset);
    const hipError_t uploaded = scene->texels.upload(asQuads(texels));
    return uploaded == hipSuccess ? PATHED_OK : deviceFail(uploaded, "upload textures");
}

// What the host derives from the description for the shading side, once the texels have their device address.
struct ShadingTables {
    std::vector<DMaterial> materials;
    std::vector<DSphere> spheres;
    std::vector<LightEntry> lightList;   // emissive surfaces in model order, the environment light last
    std::vector<DLight> lights;          // ... as the device reads them
    EnvTables env;                       // empty without an environment light
};

static void buildShadingTables(const PathedSceneDesc *desc, const float4 *texels, const std::vector<size_t> &textureOffset, ShadingTables *tables)
{
    tables->materials.resize(desc->n_materials);
    std::vector<unsigned char> materialEmits(desc->n_materials);
    for (uint32_t i = 0; i < desc->n_materials; i++) {
        DMaterial &material = tables->materials[i];
        material = buildMaterial(desc->materials[i]);
        if (desc->materials[i].albedo_type == PATHED_ALBEDO_TEXTURE) {
            const PathedTexture &texture = desc->textures[desc->materials[i].texture];
            material.texSize = texture.width | (texture.height << 16);
            material.texels = texels + textureOffset[(size_t)desc->materials[i].texture];
        }
        materialEmits[i] = emits(material);
    }
    tables->spheres.resize(desc->n_spheres);
    for (uint32_t i = 0; i < desc->n_spheres; i++) {
        const PathedSphere &s = desc->spheres[i];
        for (int k = 0; k < 3; k++) {
            tables->spheres[i].centerWorld[k] = s.center_world[k];
            tables->spheres[i].centerSample[k] = s.center_sample[k];
        }
        tables->spheres[i].radius = s.radius;
        tables->spheres[i].material = s.material;
    }
    tables->lightList = listLights(desc, materialEmits);
    for (const LightEntry &light : tables->lightList) { tables->lights.push_back({ light.kind, light.index }); }
    if (desc->env) { buildEnvTables(*desc->env, &tables->env); }
}

static int chooseBuilder(const PathedSceneDesc *desc, const PathedSceneOptions &options)
{
    int builder = options.bvh_builder > 0 ? options.bvh_builder - 1 : PATHED_BVH_SAH_HOST;
    if (const char *text = tuningEnv("PATHED_BVH_BUILDER")) {
        if (!strcmp(text, "lbvh")) { builder = PATHED_BVH_LBVH_DEVICE; }
        else if (!strcmp(text, "ploc")) { builder = PATHED_BVH_PLOC_DEVICE; }
        else if (!strcmp(text, "sah")) { builder = PATHED_BVH_SAH_HOST; }
    }
    // tiny meshes take the all-triangles kernel, which wants the host copy of the records
    if (fewTriangles(desc)) { builder = PATHED_BVH_SAH_HOST; }
    return builder;
}

// The triangle soup on the device: input of the device builders and of the shading-record gather.  Freed with the scope
// that holds it, unless the scene adopts it.
struct TriangleSoup {
    DeviceBuffer<float> positions, normals, uvs;
    DeviceBuffer<uint32_t> indices;
    DeviceBuffer<int> triMaterial;

    void release() { positions.release(); normals.release(); uvs.release(); indices.release(); triMaterial.release(); }

    // pathed_hip_scene_refit moves the vertices later: the soup stays (the buffers change owner, nothing is copied)
    void adoptInto(PathedScene &scene)
    {
        auto adopt = [](auto &to, auto &from) { to.ptr = from.ptr; to.count = from.count; from.ptr = nullptr; from.count = 0; };
        adopt(scene.soupPositions, positions); adopt(scene.soupNormals, normals); adopt(scene.soupUvs, uvs);
        adopt(scene.soupIndices, indices); adopt(scene.soupTriMaterial, triMaterial);
    }
};

// ... uploaded, and the shading records gathered from it (k_build_tri_shade, not waited for here)
static int uploadSoup(PathedScene *scene, const PathedSceneDesc *desc, TriangleSoup *soup)
{
    if (desc->n_triangles == 0) { return PATHED_OK; }
    const size_t nv = desc->n_vertices, nt = desc->n_triangles;
    hipError_t status = soup->positions.allocate(3 * nv);
    if (status == hipSuccess) { status = soup->normals.allocate(3 * nv); }
    if (status == hipSuccess) { status = soup->uvs.allocate(2 * nv); }
    if (status == hipSuccess) { status = soup->indices.allocate(3 * nt); }
    if (status == hipSuccess) { status = soup->triMaterial.allocate(nt); }
    if (status == hipSuccess) { status = scene->triShade.allocate((size_t)kTriShadeQuads * nt); }
    if (status == hipSuccess) { status = scene->triCompact.allocate((size_t)kTriCompactQuads * nt); }
    if (status == hipSuccess) { status = hipMemcpy(soup->positions.ptr, desc->positions, 3 * nv * sizeof(float), hipMemcpyHostToDevice); }
    if (status == hipSuccess) { status = hipMemcpy(soup->normals.ptr, desc->normals, 3 * nv * sizeof(float), hipMemcpyHostToDevice); }
    if (status == hipSuccess) { status = hipMemcpy(soup->uvs.ptr, desc->uvs, 2 * nv * sizeof(float), hipMemcpyHostToDevice); }
    if (status == hipSuccess) { status = hipMemcpy(soup->indices.ptr, desc->indices, 3 * nt * sizeof(uint32_t), hipMemcpyHostToDevice); }
    if (status == hipSuccess) { status = hipMemcpy(soup->triMaterial.ptr, desc->tri_material, nt * sizeof(int), hipMemcpyHostToDevice); }
    if (status == hipSuccess) {
        hipLaunchKernelGGL(k_build_tri_shade, dim3((unsigned)((8 * nt + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                           soup->positions.ptr, soup->normals.ptr, soup->uvs.ptr, soup->indices.ptr, soup->triMaterial.ptr,
                           (uint32_t)nt, scene->triShade.ptr, scene->triCompact.ptr);
        status = hipGetLastError();
    }
    return status == hipSuccess ? PATHED_OK : deviceFail(status, "upload triangle soup");
}

// rtcCommitScene's stand-in on the device (lbvh.h): build, keep the result in place
static int buildTreeOnDevice(PathedScene *scene, const PathedSceneDesc *desc, int builder, const TriangleSoup &soup)
{
    DeviceBvh built;
    std::string message;
    hipError_t status;
    // spheres join the tree as one-sphere leaves, as on the host (reference src/sphere.cpp:16-48: each is a geometry of its own)
    DeviceBuffer<float4> sphereBounds;
    if (desc->n_spheres > 0) {
        std::vector<float4> bounds(desc->n_spheres);
        for (uint32_t i = 0; i < desc->n_spheres; i++) {
            bounds[i] = make_float4(desc->spheres[i].center_world[0], desc->spheres[i].center_world[1], desc->spheres[i].center_world[2], desc->spheres[i].radius);
        }
        if ((status = sphereBounds.upload(bounds)) != hipSuccess) { return deviceFail(status, "upload sphere bounds"); }
        scene->spheresInTree = true;
    }
    status = buildBvhOnDevice(builder == PATHED_BVH_PLOC_DEVICE ? kDeviceBuilderPloc : kDeviceBuilderLbvh,
                              soup.positions.ptr, soup.indices.ptr, desc->n_triangles, sphereBounds.ptr, desc->n_spheres, nullptr, &built, &message);
    if (status != hipSuccess) { return deviceFail(status, message.empty() ? "device BVH build" : message.c_str()); }
    scene->nodes.ptr = built.nodes;
    scene->nodes.count = built.nodeCapacity * 8;
    scene->leafTris.ptr = built.leafTris;
    scene->leafTris.count = (size_t)desc->n_triangles * 3;
    scene->bvh.nodeCount = built.nodeCount;
    scene->bvh.maxDepth = built.maxDepth;
    scene->bvhOnHost = false;
    scene->bvhBuildMs = built.buildMs;
    return PATHED_OK;
}

// The binned-SAH builder on the host cores (bvh_build.h), or the two-level tree of a scene with instances; uploaded.
static int buildTreeOnHost(PathedScene *scene, const PathedSceneDesc *desc, const PathedInstanceDesc *instanceDesc, const InstancedLayout &instancedLayout)
{
    const auto buildStart = std::chrono::steady_clock::now();
    // Spheres join the tree as one-sphere leaves (the reference gives each one to Embree as a geometry of its own,
    // src/sphere.cpp:16-48) unless the scene is small enough for the all-triangles kernel, which tests them one by one.
    std::vector<float> sphereBounds;
    if (!tinyScene(desc, scene->options)) {
        for (uint32_t i = 0; i < desc->n_spheres; i++) {
            for (int a = 0; a < 3; a++) { sphereBounds.push_back(desc->spheres[i].center_world[a]); }
            sphereBounds.push_back(desc->spheres[i].radius);
        }
    }
    scene->spheresInTree = !sphereBounds.empty();
    std::vector<float> instanceRecords, protoBoxes;
    if (instanceDesc) {
        scene->bvh = buildInstancedBvh(desc, instanceDesc, instancedLayout, scene->options.build_threads, &instanceRecords, &scene->instancedMaxStack,
                                       &protoBoxes, &scene->topNodes, &scene->topDepth);
    } else {
        scene->bvh = buildBvh(desc->positions, desc->indices, desc->n_triangles, sphereBounds.data(), (uint32_t)(sphereBounds.size() / 4),
                              scene->options.build_threads);
    }
    scene->bvhBuildMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - buildStart).count();
    hipError_t status;
    if ((status = scene->nodes.upload(asQuads(scene->bvh.nodes))) != hipSuccess) { return deviceFail(status, "upload nodes"); }
    if ((status = scene->leafTris.upload(asQuads(scene->bvh.leafTris))) != hipSuccess) { return deviceFail(status, "upload triangles"); }
    if (instanceDesc) {
        if ((status = scene->instanceRecords.upload(asQuads(instanceRecords))) != hipSuccess) { return deviceFail(status, "upload instance records"); }
        if ((status = scene->instanceBases.upload(instancedLayout.bases)) != hipSuccess) { return deviceFail(status, "upload instance bases"); }
        if ((status = scene->protoBoxes.upload(asQuads(protoBoxes))) != hipSuccess) { return deviceFail(status, "upload prototype boxes"); }
        scene->instanceSet.records = scene->instanceRecords.ptr;
        scene->instanceSet.bases = scene->instanceBases.ptr;
        scene->instanceSet.nInstances = (int)instanceDesc->n_instances;
        scene->instanceSet.worldTris = instancedLayout.worldTris;
    }
    return PATHED_OK;
}

// Waits for the builders and the shading-record gather, then lets the soup go or, for a refittable scene, keeps it.
static int settleSoup(PathedScene *scene, const PathedSceneDesc *desc, TriangleSoup *soup)
{
    const hipError_t status = hipDeviceSynchronize();   // the shading-record gather reads the soup
    if (status == hipSuccess && scene->options.refittable && desc->n_triangles > 0) {
        soup->adoptInto(*scene);
        scene->soupVertices = desc->n_vertices;
        scene->refittable = true;
    }
    // (its destructor would do; released here for the footprint: 44 bytes per triangle or so that the uploads, the hybrid
    // split and the render state allocated from here on need not sit beside)
    soup->release();
    return status == hipSuccess ? PATHED_OK : deviceFail(status, "build shading records");
}

// spheres, materials, lights and their records, media, the environment's tables
static int uploadShadingTables(PathedScene *scene, const PathedSceneDesc *desc, const ShadingTables &tables)
{
    hipError_t status;
    if ((status = scene->spheres.upload(tables.spheres)) != hipSuccess) { return deviceFail(status, "upload spheres"); }
    if ((status = scene->materials.upload(tables.materials)) != hipSuccess) { return deviceFail(status, "upload materials"); }
    if ((status = scene->lights.upload(tables.lights)) != hipSuccess) { return deviceFail(status, "upload lights"); }
    if ((status = scene->lightRecords.allocate((size_t)kLightRecordQuads * tables.lights.size())) != hipSuccess) { return deviceFail(status, "allocate light records"); }
    if ((status = buildLightRecords(scene, (int)tables.lights.size())) != hipSuccess) { return deviceFail(status, "build light records"); }
    // participating media and every primitive's internal medium (scene_tables.h: buildMediaTables)
    const MediaTables mediaTables = buildMediaTables(desc);
    std::vector<DMedium> media(desc->n_media);
    for (uint32_t i = 0; i < desc->n_media; i++) {
        std::memset(&media[i], 0, sizeof(DMedium));
        for (int k = 0; k < 3; k++) { media[i].sigmaT[k] = mediaTables.sigma[6 * i + k]; media[i].sigmaS[k] = mediaTables.sigma[6 * i + 3 + k]; }
    }
    scene->hasContainers = scene->hasContainers || mediaTables.hasContainers;
    if ((status = scene->media.upload(media)) != hipSuccess) { return deviceFail(status, "upload media"); }
    scene->mediaHost = media;
    if ((status = scene->primMedium.upload(mediaTables.primMedium)) != hipSuccess) { return deviceFail(status, "upload media"); }
    const EnvTables &env = tables.env;
    if ((status = scene->envRgba.upload(asQuads(env.rgba))) != hipSuccess) { return deviceFail(status, "upload env map"); }
    if ((status = scene->thetaCdf.upload(env.thetaCdf)) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->phiCdf.upload(env.phiCdf)) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->phiEmpty.upload(env.phiEmpty)) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->thetaGuide.upload(env.thetaGuide)) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->phiGuide.upload(env.phiGuide)) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->thetaRecords.upload(asQuads(env.thetaRecords))) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    if ((status = scene->phiRecords.upload(asQuads(env.phiRecords))) != hipSuccess) { return deviceFail(status, "upload env cdf"); }
    return PATHED_OK;
}

// DScene: what the kernels read of the scene, now that every table has its address; and the scene's traits
static void fillDeviceScene(PathedScene *scene, const PathedSceneDesc *desc, const ShadingTables &tables)
{
    DScene &d = scene->device;
    d.nodes = scene->nodes.ptr;
    d.nodesQ = nullptr;
    d.leafTris = scene->leafTris.ptr;
    d.nNodes = scene->bvh.nodeCount;
    d.nTris = (int)desc->n_triangles;
    d.spheres = scene->spheres.ptr;
    d.nSpheres = (int)desc->n_spheres;
    d.nLinearSpheres = scene->spheresInTree ? 0 : (int)desc->n_spheres;
    d.triShade = scene->triShade.ptr;
    d.triCompact = scene->triCompact.ptr;
    d.nPlainRanges = plainRanges(desc, kMaxPlainRanges, d.plainBegin, d.plainEnd);
    d.materials = scene->materials.ptr;
    d.nMaterials = (int)desc->n_materials;
    d.lights = scene->lights.ptr;
    d.lightRecords = scene->lightRecords.ptr;
    d.nLights = (int)tables.lights.size();
    scene->traits = sceneTraits(desc, tables.materials, tables.lights, scene->options);
    d.media = scene->media.ptr;
    d.primMedium = scene->primMedium.ptr;
    d.nMedia = (int)desc->n_media;
    if (desc->env) {
        const EnvTables &env = tables.env;
        d.env.thetaEmpty = env.thetaEmpty;
        d.env.width = env.width;
        d.env.height = env.height;
        d.env.scale = env.scale;
        std::memcpy(d.env.mapToWorld, env.mapToWorld, sizeof env.mapToWorld);
        std::memcpy(d.env.worldToMap, env.worldToMap, sizeof env.worldToMap);
        d.hasEnv = 1;
    }
    d.env.rgba = scene->envRgba.ptr;
    d.env.thetaCdf = scene->thetaCdf.ptr;
    d.env.phiCdf = scene->phiCdf.ptr;
    d.env.phiEmpty = scene->phiEmpty.ptr;
    d.env.thetaGuide = scene->thetaGuide.ptr;
    d.env.phiGuide = scene->phiGuide.ptr;
    d.env.thetaRecords = scene->thetaRecords.ptr;
    d.env.phiRecords = scene->phiRecords.ptr;
}

// Which kernels carry the radiance loop, part one: pools, the all-triangles intersector, the slot policy's defaults, the
// shade kernel (returned through *chosen: 0 automatic .. 6, as PathedSceneOptions.shade_kernel) and the trace configuration.
static int chooseShadeKernel(PathedScene *scene, const PathedSceneDesc *desc, int *chosen)
{
    const PathedSceneOptions &options = scene->options;
    if (options.pools > 0) { scene->pools = options.pools; }
    if (const char *poolCount = tuningEnv("PATHED_POOLS")) {
        const int value = atoi(poolCount);
        scene->pools = value < 1 ? 1 : value > kMaxPools ? kMaxPools : value;
    }
    scene->bruteForce = tinyScene(desc, options) && !scene->instanced;
    // BVH scenes: more slots = more rays per persistent wave to refill finished lanes from (ray cost is heavy-tailed) and
    // fewer, longer launches: 8 Mi slots (1.3 GB of path state) against 4 Mi: +3.6 % on the teapot, +6.1 % on the 5.2 M-
    // triangle mesh at >= 256 spp per call, 16 Mi +1 % / +7.6 %, 32 Mi less again (tools/slots_sweep.py); short calls want
    // fewer (renderPass: at least 16 units per slot).  The all-triangles wavefront kernel has uniform cost and prefers the
    // smaller, Infinity-Cache-resident state.
    scene->maxSlots = scene->bruteForce ? (1 << 20) : (1 << 23);
    scene->adaptiveSlots = !scene->bruteForce;
    // which kernels carry the radiance loop: scenes of <= 64 triangles default to the fused in-register path
    // kernel, everything else to the wavefront with the per-slot shade kernel; the staged shade kernel and the split
    // shade stage (k_vertex + k_regen over lists the trace kernel writes) are selectable: both issue fewer
    // instructions on fuller waves and both lose to the coalesced per-slot kernel (DESIGN.md has the measurements)
    int shadeKernel = options.shade_kernel;
    if (scene->instanced) { shadeKernel = 1; }   // always the wavefront, with k_trace_instanced / k_shade_instanced
    else if (const char *text = tuningEnv("PATHED_SHADE_KERNEL")) {   // experiments: "per-slot" | "staged" | "fused" | "split"
        if (!strcmp(text, "per-slot")) { shadeKernel = 1; }
        else if (!strcmp(text, "staged")) { shadeKernel = 2; }
        else if (!strcmp(text, "fused")) { shadeKernel = 3; }
        else if (!strcmp(text, "split")) { shadeKernel = 4; }
        else if (!strcmp(text, "wave")) { shadeKernel = 5; }
    }
    if (shadeKernel == 3 && !scene->bruteForce) {
        return fail(PATHED_E_INVALID, "the fused path kernel serves scenes of at most 64 triangles that take the all-triangles intersector");
    }
#if !PATHED_EXPERIMENTS
    if (shadeKernel == 2 || shadeKernel == 4 || requestedNodeFormat(options) >= 2 || options.small_phase1 == 2) {
        return fail(PATHED_E_UNSUPPORTED, "the staged and split shade stages, the compressed node formats and the matrix-pipe phase 1 are measured-and-rejected "
                                          "experiments: build libpathed_hip_experiments.so (`make experiments`) and load it instead");
    }
#endif
    if (shadeKernel == 4 && scene->bruteForce) {
        return fail(PATHED_E_INVALID, "the split shade stage follows the BVH trace kernel: scenes of at most 64 triangles take the fused, per-slot or staged kernels");
    }
    scene->splitShade = shadeKernel == 4;
    configureTrace(scene);
    *chosen = shadeKernel;
    return PATHED_OK;
}

// the compressed tree: sphere-free scenes whose tree stays in HBM, walked by the per-slot pipeline's trace kernel
static int chooseNodeFormat(PathedScene *scene)
{
    const PathedSceneOptions &options = scene->options;
    const int nodeFormat = requestedNodeFormat(options);
    const bool eligible = !scene->bruteForce && !scene->sceneInLds && !scene->splitShade && scene->device.nSpheres == 0
        && scene->device.nNodes > 0 && options.generic_kernels == 0 && !scene->instanced;
    if (nodeFormat >= 2 && !eligible) {
        return fail(PATHED_E_INVALID, "compressed nodes serve sphere-free scenes whose tree is walked in HBM by the per-slot pipeline (not generic_kernels, not the split stage)");
    }
    const int chosen = !eligible || nodeFormat == 1 ? 0 : nodeFormat == 0 ? PATHED_DEFAULT_NODE_FORMAT : nodeFormat - 1;
#if PATHED_EXPERIMENTS
    if (chosen != 0) {
        hipError_t status;
        const size_t nNodes = (size_t)scene->device.nNodes;
        const unsigned blocks = (unsigned)((nNodes + kBlock - 1) / kBlock);
        if ((status = scene->nodesQ.allocate((chosen == 2 ? 8 : 4) * nNodes)) != hipSuccess) { return deviceFail(status, "allocate compressed nodes"); }
        if (chosen == 2) { hipLaunchKernelGGL(k_widen_nodes, dim3(blocks), dim3(kBlock), 0, nullptr, scene->nodes.ptr, (int)nNodes, scene->nodesQ.ptr); }
        else { hipLaunchKernelGGL(k_compress_nodes, dim3(blocks), dim3(kBlock), 0, nullptr, scene->nodes.ptr, (int)nNodes, scene->nodesQ.ptr); }
        if ((status = hipDeviceSynchronize()) != hipSuccess) { return deviceFail(status, "compress nodes"); }
        scene->device.nodesQ = scene->nodesQ.ptr;
        scene->nodeFormat = chosen;
    }
#else
    (void)chosen;
#endif
    return PATHED_OK;
}

// ... part two: the split stage's grids, and which in-register path kernels serve the scene
static void choosePathKernels(PathedScene *scene, int shadeKernel)
{
    // persistent grids of the split stage: k_vertex at PATHED_VERTEX_WAVES blocks per CU, k_regen at PATHED_REGEN_WAVES
#if PATHED_EXPERIMENTS
    scene->vertexGrid = scene->computeUnits * PATHED_VERTEX_WAVES;
    scene->regenGrid = scene->computeUnits * PATHED_REGEN_WAVES;
#endif
    if (const char *text = tuningEnv("PATHED_VERTEX_GRID")) { const int value = atoi(text); if (value >= 1 && value <= 65536) { scene->vertexGrid = value; } }
    if (const char *text = tuningEnv("PATHED_REGEN_GRID")) { const int value = atoi(text); if (value >= 1 && value <= 65536) { scene->regenGrid = value; } }
    scene->fusedPath = scene->bruteForce && (shadeKernel == 0 || shadeKernel == 3);
    scene->waveMode = shadeKernel == 5 ? 2 : (shadeKernel == 0 || shadeKernel == 6) ? 0 : 1;
    scene->waveAvailable = !scene->bruteForce && scene->device.nMaterials <= kMaxLdsMaterials && scene->nodeFormat == 0 && !scene->instanced;
}

// [r5] k_path_hybrid's split of the scene and the wavefront's local set, where they apply
static int buildSplits(PathedScene *scene, const PathedSceneDesc *desc, int shadeKernel)
{
    const PathedSceneOptions &options = scene->options;
    // k_path_hybrid: BVH scenes small enough that a handful of large triangles carry most of the hits (path_hybrid.h)
    // (shade_kernel 6 asks for it on a larger mesh as well: the walk is the same, the tree just stops being cache-resident)
    const bool eligible = !scene->bruteForce && desc->n_spheres == 0
        && scene->device.nMaterials <= kMaxLdsMaterials && scene->nodeFormat == 0 && options.intersector != 1 && !scene->hasContainers
        && !options.refittable    // (a refittable scene keeps ONE tree, the one pathed_hip_scene_refit moves)
        && !scene->instanced;
    if (shadeKernel == 6 && !eligible) {
        return fail(PATHED_E_INVALID, "the hybrid path kernel serves sphere-free scenes of more than 64 triangles and at most 96 materials (intersector 0, not refittable)");
    }
    if (eligible && ((shadeKernel == 0 && desc->n_triangles <= (uint32_t)kHybridMaxTris) || shadeKernel == 6)) {
        const hipError_t status = buildHybrid(scene, desc);
        if (status != hipSuccess) { return deviceFail(status, "build the hybrid kernel's scene split"); }
        scene->hybridPath = true;
    }
    // (not for refittable scenes: their vertices move, the large triangles' records and the bounds of the rest would go stale)
    if (!scene->bruteForce && options.local_rays != 1 && scene->nodeFormat == 0 && !options.refittable && !scene->instanced) { buildLocalSet(scene, desc); }
    return PATHED_OK;
}

// ... part three: the wave kernel's and the staged kernel's settings
static int tuneWaveAndStages(PathedScene *scene, int shadeKernel)
{
    const PathedSceneOptions &options = scene->options;
    if (shadeKernel == 5 && !scene->waveAvailable) {
        return fail(PATHED_E_INVALID, "the wave path kernel serves BVH scenes (more than 64 triangles or intersector 1) of at most 96 materials over the float nodes");
    }
    if (options.wave_max_ksamples > 0) { scene->waveMaxSamples = (unsigned long long)options.wave_max_ksamples << 10; }
    if (options.wave_stragglers != 0) { scene->waveStragglers = options.wave_stragglers < 0 ? 0 : options.wave_stragglers; }
    if (options.wave_refill != 0) { scene->waveRefill = options.wave_refill; }
    if (const char *text = tuningEnv("PATHED_WAVE_MAX_SAMPLES")) { scene->waveMaxSamples = strtoull(text, nullptr, 10); }
    if (const char *text = tuningEnv("PATHED_WAVE_BLOCK")) { scene->waveBlock = atoi(text) != 0; }
    if (const char *text = tuningEnv("PATHED_WAVE_SHADE_READY")) { const int value = atoi(text); if (value >= 1 && value <= 64) { scene->waveShadeReady = value; } }
    if (const char *text = tuningEnv("PATHED_WAVE_REFILL")) { const int value = atoi(text); if (value >= 1 && value <= 64) { scene->waveRefill = value; } }
    if (const char *text = tuningEnv("PATHED_WAVE_STRAGGLERS")) { const int value = atoi(text); if (value >= 0 && value <= 64) { scene->waveStragglers = value; } }
    scene->stagedShade = shadeKernel == 2;
    // more slots per block = fuller last waves of the dense stages, fewer blocks to fill the chip with:
    // the 0.5 Mi-slot pools of the all-triangles scenes take 512, the 2 Mi-slot pools of the BVH scenes 1024
    scene->stageRounds = scene->bruteForce ? 2 : 4;
    if (options.stage_slots != 0) { scene->stageRounds = options.stage_slots / kBlock; }
    if (const char *text = tuningEnv("PATHED_STAGE_SLOTS")) {
        const int value = atoi(text);
        if (value == 512 || value == 1024) { scene->stageRounds = value / kBlock; }
    }
    return PATHED_OK;
}

// The all-triangles kernels' records: the packed pairs, the inputs of the never-occluder rule, the fused kernel's phase-1
// records (rebuildSmallItems) and, in the experiments build, the matrix-pipe rows.
static int buildSmallScene(PathedScene *scene, const PathedSceneDesc *desc, const std::vector<LightEntry> &lightList)
{
    const PathedSceneOptions &options = scene->options;
    hipError_t status;
    std::memset(&scene->smallTris, 0, sizeof scene->smallTris);
    if (scene->bruteForce) { packSmallTris(scene->bvh.leafTris.data(), scene->device.nTris, kSmallPairWords, reinterpret_cast<float *>(scene->smallTris.data)); }
    std::memset(&scene->smallItems, 0, sizeof scene->smallItems);
    SmallLightInputs inputs = smallLightInputs(desc, lightList);
    scene->smallExtraPoints.swap(inputs.extraPoints);
    scene->smallEmitterPrims.swap(inputs.emitterPrims);
    scene->smallSphereLights.swap(inputs.sphereLights);
    if ((status = rebuildSmallItems(scene)) != hipSuccess) { return deviceFail(status, "upload the phase-1 records"); }
    scene->mfmaPhase1 = false;
    std::memset(&scene->mfmaFrame, 0, sizeof scene->mfmaFrame);
    if (scene->bruteForce && scene->fusedPath) {
        int phase1 = options.small_phase1;
        if (const char *text = tuningEnv("PATHED_SMALL_PHASE1")) {
            if (!strcmp(text, "valu")) { phase1 = 1; } else if (!strcmp(text, "mfma")) { phase1 = 2; }
        }
        if (phase1 == 0) { phase1 = kDefaultSmallPhase1; }
        if (phase1 == 2 && scene->device.nTris > 0) {
            // (rebuildSmallItems builds the same table, but only once mfmaPhase1 is set -- a new camera; at its call above
            // the flag was still false, so this is the table's first build and stays)
            std::vector<float> table;
            // rows in ITEM order: phase 2 of the fused kernel indexes the item-ordered triangle records
            buildMfmaTable(scene->itemTrisHost.data(), scene->device.nTris, scene->device.camera.origin, 1, &table, &scene->mfmaFrame);
            if ((status = scene->mfmaTable.upload(table)) != hipSuccess) { return deviceFail(status, "upload the matrix-pipe rows"); }
            scene->mfmaPhase1 = true;
        }
    }
    return PATHED_OK;
}

// the unit order, and the caller's word on the slot count (chooseShadeKernel set the defaults)
static void applySlotOptions(PathedScene *scene)
{
    const PathedSceneOptions &options = scene->options;
    scene->unitOrder = unitOrderFromEnvironment(options.unit_order == 2 ? kOrderStripesTiled : options.unit_order == 3 ? kOrderTiles : kOrderStripes);
    if (options.max_slots >= kBlock) { scene->maxSlots = options.max_slots; scene->adaptiveSlots = false; }
    if (const char *slots = tuningEnv("PATHED_MAX_SLOTS")) {
        const long value = atol(slots);
        if (value >= kBlock) { scene->maxSlots = (int)value; scene->adaptiveSlots = false; }
    }
}

static int createScene(const PathedSceneDesc *desc, const PathedSceneOptions *optionsIn, const PathedInstanceDesc *instanceDesc, PathedScene **out)
{
    if (!out) { return fail(PATHED_E_INVALID, "out pointer is null"); }
    *out = nullptr;
    int code = validate(desc);
    if (code != PATHED_OK) { return code; }
    PathedSceneOptions options;
    if ((code = resolveOptions(optionsIn, &options)) != PATHED_OK) { return code; }
    InstancedLayout instancedLayout;
    std::string refusal;
    if (instanceDesc && (code = planInstances(desc, options, instanceDesc, &instancedLayout, &refusal)) != PATHED_OK) { return fail(code, refusal); }
    int deviceId = 0;
    if ((code = resolveDevice(options, &deviceId)) != PATHED_OK) { return code; }

    // the one owner: every return below frees what the scene holds by then
    std::unique_ptr<PathedScene> owner(new PathedScene());
    PathedScene *scene = owner.get();
    std::memset(&scene->device, 0, sizeof scene->device);
    scene->deviceId = deviceId;
    scene->options = options;
    scene->width = desc->camera.width;
    scene->height = desc->camera.height;
    scene->instanced = instanceDesc != nullptr;
    hipDeviceProp_t properties;
    if (hipGetDeviceProperties(&properties, deviceId) == hipSuccess) {
        scene->computeUnits = properties.multiProcessorCount > 0 ? properties.multiProcessorCount : 256;
    }
    buildCamera(desc->camera, &scene->device.camera);

    // the tables
    std::vector<size_t> textureOffset;
    if ((code = uploadTextures(scene, desc, &textureOffset)) != PATHED_OK) { return code; }
    ShadingTables tables;
    buildShadingTables(desc, scene->texels.ptr, textureOffset, &tables);
    packSpherePairs(desc, scene->spherePairs);

    // the soup and the shading records, the tree
    const int builder = scene->bvhBuilder = chooseBuilder(desc, options);
    TriangleSoup soup;
    if ((code = uploadSoup(scene, desc, &soup)) != PATHED_OK) { return code; }
    const bool onDevice = builder == PATHED_BVH_LBVH_DEVICE || builder == PATHED_BVH_PLOC_DEVICE;
    code = onDevice ? buildTreeOnDevice(scene, desc, builder, soup) : buildTreeOnHost(scene, desc, instanceDesc, instancedLayout);
    if (code != PATHED_OK) { return code; }
    if ((code = settleSoup(scene, desc, &soup)) != PATHED_OK) { return code; }

    // the uploads, the DScene pointers
    if ((code = uploadShadingTables(scene, desc, tables)) != PATHED_OK) { return code; }
    fillDeviceScene(scene, desc, tables);

    // the kernel choice, with the hybrid and the local set in its middle (they need the node format, the wave kernel's
    // refusal comes after them)
    int shadeKernel = 0;
    if ((code = chooseShadeKernel(scene, desc, &shadeKernel)) != PATHED_OK) { return code; }
    if ((code = chooseNodeFormat(scene)) != PATHED_OK) { return code; }
    choosePathKernels(scene, shadeKernel);
    if ((code = buildSplits(scene, desc, shadeKernel)) != PATHED_OK) { return code; }
    if ((code = tuneWaveAndStages(scene, shadeKernel)) != PATHED_OK) { return code; }

    // the phase-1 records, the camera masks
    if ((code = buildSmallScene(scene, desc, tables.lightList)) != PATHED_OK) { return code; }
    const hipError_t status = rebuildCameraMasks(scene);
    if (status != hipSuccess) { return deviceFail(status, "build the camera-ray candidate masks"); }
    applySlotOptions(scene);
    *out = owner.release();
    return PATHED_OK;
}

int pathed_hip_scene_create_ex(const PathedSceneDesc *desc, const PathedSceneOptions *optionsIn, PathedScene **out)
{
    return createScene(desc, optionsIn, nullptr, out);
}

int pathed_hip_scene_create_instanced(const PathedSceneDesc *desc, const PathedSceneOptions *optionsIn, const PathedInstanceDesc *instances, PathedScene **out)
{
    if (!instances) { return fail(PATHED_E_INVALID, "instance description is null"); }
    return createScene(desc, optionsIn, instances, out);
}

void pathed_hip_scene_destroy(PathedScene *scene)
{
    if (scene) { (void)hipSetDevice(scene->deviceId); }
    delete scene;
}

}  // extern "C" (the render passes below are internal; persistentPass is a template)

// The unit order of one pool's launch parameters (kernels.h: THE UNIT ORDER).  The (nQueues x pools) queues share out
// ITEMS round-robin -- the chunks of the pass (stripes: an item is one whole image of units) or groups of kUnitGroup pixels
// (tiles: an item is all chunks of the group) -- queue q of pool `pool` owns the items (q * pools + pool) + j * queues.
// itemPixels: the pixels the pass renders -- the image's, or the length of its pixel list (kOrderList).
// Returns false when the unit ids of the pass do not fit 32 bits.
static bool fillUnitOrder(RenderParams &q, int order, int width, unsigned long long itemPixels, int chunksPerPixel, int pool, int pools, int nQueues)
{
    const unsigned long long nPixels = itemPixels;
    const unsigned long long allQueues = (unsigned long long)nQueues * (unsigned long long)pools;
    unsigned long long items, itemUnits, lastItemShortfall = 0;
    if (order == kOrderTiles) {
        items = (nPixels + kUnitGroup - 1ull) / kUnitGroup;
        itemUnits = (unsigned long long)kUnitGroup * (unsigned long long)chunksPerPixel;
        q.lastGroupPixels = (unsigned int)(nPixels - (items - 1ull) * kUnitGroup);
        lastItemShortfall = (kUnitGroup - (unsigned long long)q.lastGroupPixels) * (unsigned long long)chunksPerPixel;
    } else {
        items = (unsigned long long)chunksPerPixel;
        itemUnits = nPixels;
        q.lastGroupPixels = kUnitGroup;
    }
    const unsigned long long stride = ((items + allQueues - 1ull) / allQueues) * itemUnits;   // the longest queue
    if (stride * (unsigned long long)nQueues >= 0xFFFFFFF0ull || nPixels + kUnitGroup >= 0xFFFFFFF0ull) { return false; }
    q.unitOrder = order;
    q.pool = (unsigned int)pool;
    q.pools = (unsigned int)pools;
    q.nQueues = nQueues;
    q.nGroups = (unsigned int)items;
    q.groupUnits = (unsigned int)itemUnits;
    q.unitsPerQueue = (unsigned int)stride;
    q.divStride = makeFastDiv((unsigned int)stride);
    q.divGroupUnits = makeFastDiv((unsigned int)itemUnits);
    q.divBand = makeFastDiv(8u * (unsigned int)width);
    q.divWidth = makeFastDiv((unsigned int)width);
    unsigned long long total = 0;
    for (int k = 0; k < kUnitQueues; k++) {
        unsigned long long units = 0;
        const unsigned long long first = (unsigned long long)k * (unsigned long long)pools + (unsigned long long)pool;
        if (k < nQueues && first < items) {
            units = ((items - 1ull - first) / allQueues + 1ull) * itemUnits;
            if ((items - 1ull - first) % allQueues == 0ull) { units -= lastItemShortfall; }   // owns the ragged last group
        }
        q.queueUnits[k] = (unsigned int)units;
        total += units;
    }
    q.nUnits = (unsigned int)total;
    return true;
}

// VolumePathTracer on a scene WITHOUT media and without passthrough containers is PathTracer: the reference's two integrators
// share their direct-lighting arithmetic statement for statement (src/direct_lighting_helper.cpp:37-187 against
// src/path_tracer.cpp:79-216), every volumetric query degenerates to the regular one and no segment scatters -- the oracle's
// two integrators and k_path_volume / the path-tracer kernels give the same floats there (tests/test_gpu_volume.py).  Such a
// scene therefore runs the path tracer's kernels (fused or wavefront: one path per lane with no refill is 0.5-0.6x of them);
// PathedSceneOptions.generic_kernels = 1 keeps k_path_volume, for that very comparison.  The same holds for
// BasicVolumeIntegrator and k_path_scatter: without a medium no segment scatters and the stack never holds one.
static bool volumeIntegrator(const PathedScene *scene)
{
    return scene->integrator == PATHED_INTEGRATOR_VOLUME_PATH_TRACER || scene->integrator == PATHED_INTEGRATOR_BASIC_VOLUME;
}

static bool usesVolumeKernel(const PathedScene *scene)
{
    if (!volumeIntegrator(scene)) { return false; }
    return scene->hasContainers || scene->device.nMedia > 0 || scene->options.generic_kernels != 0;
}

// One internal pass of a render call: samples [begin, begin + count) of every pixel, count <= chunk * kMaxChunksPerPass,
// summed into `accum` behind whatever `stream` holds.  Its work units are `chunk` samples of one pixel each.
struct Pass {
    uint64_t seed;
    uint32_t begin, count;
    int startBounce, lastBounce;
    float *accum;
    float *squares;   // per-channel sums of squares beside `accum` (pathed_hip_render_moments_device), or null
    hipStream_t stream;
    int nPixels, chunk, chunksPerPixel;
    unsigned int nUnits;
    // a pass over a list of pixels (pathed_hip_render_pixels_device): nList > 0, the list in device memory, the count image
    // beside the two sums.  nUnits = nList * chunksPerPixel then; the unit buffer keeps the image's layout (bufferUnits).
    const uint32_t *pixelList;
    int nList;
    uint32_t *counts;

    int unitPixels() const { return nList > 0 ? nList : nPixels; }   // pixels the pass renders
    size_t bufferUnits() const { return (size_t)nPixels * (size_t)chunksPerPixel; }   // entries of the unit buffer: chunk * nPixels + pixel
};

// The end of every pass: the units' partial sums onto the caller's sums, and, for a pass that carries a squares buffer,
// their squares onto that (k_resolve_moments; such a pass has one sample per unit).
static void launchResolve(const Pass &pass, const RenderParams &params, hipStream_t stream)
{
    const dim3 pixelGrid((unsigned)((pass.unitPixels() + kBlock - 1) / kBlock));
    if (pass.nList > 0) {
        ListMomentsParams moments;
        moments.chunkBuf = params.state.chunkBuf;
        moments.pixelList = pass.pixelList;
        moments.nList = pass.nList;
        moments.nPixels = params.nPixels;
        moments.chunksPerPixel = params.chunksPerPixel;
        moments.samples = pass.count;
        moments.sum = params.accum;
        moments.squares = pass.squares;
        moments.count = pass.counts;
        hipLaunchKernelGGL(k_resolve_list, pixelGrid, dim3(kBlock), 0, stream, moments);
    } else if (pass.squares) {
        MomentsParams moments;
        moments.chunkBuf = params.state.chunkBuf;
        moments.nPixels = params.nPixels;
        moments.chunksPerPixel = params.chunksPerPixel;
        moments.sum = params.accum;
        moments.squares = pass.squares;
        hipLaunchKernelGGL(k_resolve_moments, pixelGrid, dim3(kBlock), 0, stream, moments);
    } else {
        hipLaunchKernelGGL(k_resolve, pixelGrid, dim3(kBlock), 0, stream, params);
    }
}

// The launch parameters every kernel of the pass reads, and the unit order of pool `pool` of `pools` over nQueues queues.
// Returns false when the unit ids of the pass do not fit 32 bits.
static bool fillPassParams(RenderParams &q, const PathedScene *scene, const Pass &pass, int pool, int pools, int nQueues)
{
    q.scene = scene->device;
    q.state.chunkBuf = scene->chunkBuf.ptr;
    q.counters = scene->counters.ptr + (size_t)pool * kCtrCount;
    q.stats = scene->stats.ptr;
    q.accum = pass.accum;
    q.nPixels = pass.nPixels;
    q.chunk = pass.chunk;
    q.chunksPerPixel = pass.chunksPerPixel;
    q.seedLo = (uint32_t)pass.seed;
    q.seedHi = (uint32_t)(pass.seed >> 32);
    q.sppBegin = pass.begin;
    q.sppEnd = pass.begin + pass.count;
    q.startBounce = pass.startBounce;
    q.lastBounce = pass.lastBounce;
    if (pass.nList > 0) { q.cameraQueue = reinterpret_cast<float4 *>(const_cast<uint32_t *>(pass.pixelList)); }   // kernels.h: pixelList()
    return fillUnitOrder(q, pass.nList > 0 ? kOrderList : scene->unitOrder, scene->width, (unsigned long long)pass.unitPixels(), pass.chunksPerPixel, pool, pools, nQueues);
}

// A pass as ONE persistent launch that renders every unit: no slot pool, no iteration loop, no polling.  This is all that the
// fused, volume, wave and hybrid organisations share; `launch(params, grid, stream)` sets the path's own RenderParams fields
// and starts its kernel.  blocksPerCu: what the kernel's register budget keeps resident (waves per SIMD = blocks per CU).
// maxStack > 0: the kernel keeps ldsRows rows of a lane's traversal stack in LDS and spills the entries beyond them, up to the
// tree's bound maxStack, to HBM; 0: it walks no tree.
template <typename Launch>
static int persistentPass(PathedScene *scene, const Pass &pass, int blocksPerCu, int maxStack, int ldsRows, Launch launch)
{
    if (scene->chunkCapacity < pass.bufferUnits()) {
        HIP_TRY(scene->chunkBuf.allocate(pass.bufferUnits()));
        scene->chunkCapacity = pass.bufferUnits();
    }
    if (!scene->counters.ptr) { HIP_TRY(scene->counters.allocate(kMaxPools * kCtrCount)); }
    if (const int code = ensureStats(scene)) { return code; }

    // the grid: blocksPerCu blocks per CU, or fewer when the pass has fewer than 64 units per wave
    unsigned long long blocks = (unsigned long long)scene->computeUnits * blocksPerCu;
    const unsigned long long blocksNeeded = ((unsigned long long)pass.nUnits + (unsigned long long)kBlock - 1) / kBlock;
    if (blocks > blocksNeeded) { blocks = blocksNeeded; }
    if (blocks < 1) { blocks = 1; }
    const unsigned int waves = (unsigned int)blocks * kWavesPerBlock;

    RenderParams params;
    std::memset(&params, 0, sizeof params);
    if (maxStack > 0) {
        const size_t overflowInts = stackSpillInts((size_t)blocks * kBlock, maxStack, ldsRows);
        if (scene->volumeOverflow.count < overflowInts) { HIP_TRY(scene->volumeOverflow.allocate(overflowInts)); }
        params.stackOverflow = scene->volumeOverflow.ptr;
        params.maxStack = maxStack;
    }
    if (!fillPassParams(params, scene, pass, 0, 1, (int)(waves < (unsigned int)kUnitQueues ? waves : (unsigned int)kUnitQueues))) {
        return fail(PATHED_E_INVALID, "too many work units in one pass");
    }
    {
        // a wave reserves up to one unit per lane at a time; passes too small for that hand out less per atomic,
        // so that the last reservations of a queue do not leave most waves idle.  (k_path_small starts 64 units per refill of
        // its camera queue whatever the reservation size -- several atomics where unitGrab is small -- and holds up to 127
        // started samples: at the end of a pass a wave may still own that many while others retire)
        const unsigned int wavesPerQueue = (waves + (unsigned int)params.nQueues - 1) / (unsigned int)params.nQueues;
        unsigned int grab = (pass.nUnits / (unsigned int)params.nQueues) / (wavesPerQueue * 4u);
        params.unitGrab = (int)(grab < 1u ? 1u : grab > 64u ? 64u : grab);
    }

    HIP_TRY(hipMemsetAsync(params.counters, 0, kCtrCount * sizeof(unsigned int), pass.stream));
    int timed = -1;
    if (scene->timeKernels) {
        timed = scene->traceEvents.acquire();
        (void)hipEventRecord(scene->traceEvents.start[timed], pass.stream);
    }
    launch(params, dim3((unsigned)blocks), pass.stream);
    if (timed >= 0) { (void)hipEventRecord(scene->traceEvents.stop[timed], pass.stream); }
    scene->traceLaunchesAll++;
    launchResolve(pass, params, pass.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(pass.stream));

    scene->iterations += 1;
    scene->cameraSamples += (unsigned long long)pass.count * (unsigned long long)pass.unitPixels();
    return PATHED_OK;
}

// The fused path kernel (k_path_small: scenes of <= 64 triangles, whole paths in registers).  No tree, no stack.
static int renderPassFused(PathedScene *scene, const Pass &pass)
{
    // the camera queues: once per scene, for every wave of the largest grid persistentPass starts; the launch below checks
    // its grid against what is there
    // (the allocation starts with the camera-ray candidate masks, rebuildCameraMasks: made with the scene, so this is a check)
    const size_t maskQuads = cameraMaskQuads(scene);
    if (scene->cameraQueue.count < maskQuads + cameraQueueWords(scene) || !scene->cameraMasksBuilt) { HIP_TRY(rebuildCameraMasks(scene)); }
    bool queueShort = false;
    const int code = persistentPass(scene, pass, PATHED_FUSED_WAVES, 0, 0, [&](RenderParams &params, dim3 grid, hipStream_t stream) {
        if ((size_t)grid.x * kWavesPerBlock * kCameraQueueWords > scene->cameraQueue.count - maskQuads) { queueShort = true; return; }   // nothing is launched
        const bool ldsMaterials = scene->device.nMaterials <= kMaxLdsMaterials;
        const size_t lds = ldsMaterials ? (size_t)scene->device.nMaterials * sizeof(DMaterial) : 0;
        params.cameraQueue = scene->cameraQueue.ptr + maskQuads;
        params.mfmaTable = scene->mfmaTable.ptr;
        params.mfmaFrame = scene->mfmaFrame;
        params.smallQuads = scene->smallLayout.nQuads;
        params.smallKappaT = scene->smallLayout.kappaT;
        params.scene.leafTris = scene->itemTris.ptr;   // phase 2 indexes the triangles in the order phase 1's bits come in
        std::memcpy(params.spherePairs, scene->spherePairs, sizeof params.spherePairs);

        // k_path_small<LDS_MATERIALS, COUNT, TRAITS, MFMA, QUADS>: the narrowest instantiation whose compile-time scene set contains
        // this scene's (shading.h: SceneTraits).  MFMA and QUADS exist with the materials in LDS only.
        const SceneTraitFlags &traits = scene->traits;
        const bool count = scene->countMode;
        const SmallTris *records = &scene->smallItems;   // (quadsKernel below: or the pass list's)
        const auto run = [&](void (*kernel)(RenderParams, SmallTris)) { hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, params, *records); };
#if PATHED_EXPERIMENTS
        if (scene->mfmaPhase1 && ldsMaterials) {
            // phase 1 on the matrix pipe
            withBool(count, [&](auto COUNT) {
                if (traits.lambertianTriangles) { run(k_path_small<true, COUNT, TraitsLambertianTriangles, true>); }
                else if (traits.lambertianPlasticSpheres) { run(k_path_small<true, COUNT, TraitsLambertianPlasticSpheres, true>); }
                else { run(k_path_small<true, COUNT, TraitsAll, true>); }
            });
        } else
#endif
        if (scene->smallLayout.nQuads > 0 && ldsMaterials) {
            // (the rung is chosen by the FULL list's parallelograms.  The pass list keeps one triangle of every class, so it
            // normally pairs a quad wherever the full list does; nothing depends on it: with passLayout.nQuads = 0 the
            // parallelogram loops of phase 1 run no turn and every kept triangle is a lone one)
            // (the instantiations that prune the shadow ray's phase 1 -- kernels.h kSmallPrunes<COUNT, TRAITS>, the constant the kernel
            // itself branches on -- read the turns it runs from the upper half of smallQuads; the others read the word whole, so
            // quadsKernel sets that half for exactly those and hands out the instantiation in the same breath)
            // (... and the instantiations that walk the pass list -- kSmallPassList, small_items.h: NEVER-HIT -- get its records
            // and its counts, the triangle count in bits 8-15; its triangles lie behind the scene's in itemTris)
            const auto quadsKernel = [&](auto COUNT, auto traitsTag) -> void (*)(RenderParams, SmallTris) {
                using TRAITS = typename decltype(traitsTag)::type;
                if (kSmallPassList<decltype(COUNT)::value, false, TRAITS>) {
                    const SmallItemsLayout &list = scene->passLayout;
                    params.smallQuads = list.nQuads | scene->passTris << 8 | list.shadowQuadPairs << 16 | list.shadowLonePairs << 24;
                    records = &scene->passItems;
                } else if (kSmallPrunes<decltype(COUNT)::value, TRAITS>) {
                    params.smallQuads = scene->smallLayout.nQuads | scene->smallLayout.shadowQuadPairs << 16 | scene->smallLayout.shadowLonePairs << 24;
                }
                // (the headline: the Cornell-like instantiation of a pass whose units are one sample each has a body of its own,
                // kernels.h: pathSmall<.., SINGLE>; same records, same counts)
                if (!decltype(COUNT)::value && std::is_same<TRAITS, TraitsLambertianTriangles>::value && params.chunk == 1) { return k_path_small_single; }
                return k_path_small<true, decltype(COUNT)::value, TRAITS, false, true>;
            };
            // some triangles are halves of parallelograms: phase 1 tests those as parallelograms (small_items.h).  The rough, smooth
            // and triangle-lit sets have no counting instantiation: a counting call of such a scene takes TraitsAll
            const std::false_type plain{};
            if (traits.lambertianTriangles) { withBool(count, [&](auto COUNT) { run(quadsKernel(COUNT, TraitsTag<TraitsLambertianTriangles>())); }); }
            else if (traits.lambertianPlasticSpheres) { withBool(count, [&](auto COUNT) { run(quadsKernel(COUNT, TraitsTag<TraitsLambertianPlasticSpheres>())); }); }
            else if (traits.roughBeckmann && !count) { run(quadsKernel(plain, TraitsTag<TraitsRoughBeckmann>())); }
            else if (traits.roughGgx && !count) { run(quadsKernel(plain, TraitsTag<TraitsRoughGgx>())); }
            else if (traits.smoothSet && !count) { run(quadsKernel(plain, TraitsTag<TraitsSmooth>())); }
            else if (traits.triangleLit && !count) { run(quadsKernel(plain, TraitsTag<TraitsTriangleLit>())); }
            else { withBool(count, [&](auto COUNT) { run(quadsKernel(COUNT, TraitsTag<TraitsAll>())); }); }
        } else if (traits.lambertianTriangles) {
            withBool(ldsMaterials, [&](auto LDS_MATERIALS) { withBool(count, [&](auto COUNT) { run(k_path_small<LDS_MATERIALS, COUNT, TraitsLambertianTriangles>); }); });
        } else if (traits.lambertianPlasticSpheres && ldsMaterials) {
            withBool(count, [&](auto COUNT) { run(k_path_small<true, COUNT, TraitsLambertianPlasticSpheres>); });
        } else {
            withBool(ldsMaterials, [&](auto LDS_MATERIALS) { withBool(count, [&](auto COUNT) { run(k_path_small<LDS_MATERIALS, COUNT, TraitsAll>); }); });
        }
    });
    if (queueShort) { return fail(PATHED_E_DEVICE, "the fused kernel's grid outgrew its camera queues"); }
    return code;
}

// The volume integrators (kernels.h, volume.h).  small: <= 64 triangles, <= 16 spheres go through the all-triangles intersector
// (kernarg pair records), no tree walk, and take the 8-row form of every family.
static int renderPassVolume(PathedScene *scene, const Pass &pass)
{
    const bool small = scene->bruteForce, list = pass.nList > 0, grids = !scene->gridsHost.empty();
    const bool multi = scene->integrator == PATHED_INTEGRATOR_BASIC_VOLUME, aniso = multi && scene->anisotropic && !list;
    const bool ldsMaterials = scene->device.nMaterials <= kMaxLdsMaterials;
    // the generic families -- pixel lists, multiple scattering, voxel grids: the generic set, pair-of-triangles phase 1 over the
    // leaf-ordered triangles, the material table read from memory.  Only k_path_volume itself narrows the set, keeps the
    // materials in LDS and, in scenes made of quads, runs phase 1 over the item records and phase 2 over the item-ordered
    // triangles (small_items.h): QUADS and the narrowed set exist for small scenes with the materials in LDS only
    const bool generic = list || multi || grids;
    const bool quads = !generic && small && ldsMaterials && scene->smallLayout.nQuads > 0;
    // a tree scene's pixel lists and Henyey-Greenstein media take the 22-row form whatever its own row count
    const int rows = small ? 8 : (list || aniso) ? 22 : scene->stackRows;
    return persistentPass(scene, pass, PATHED_VOLUME_WAVES, scene->maxStack, rows, [&](RenderParams &params, dim3 grid, hipStream_t stream) {
        params.smallQuads = quads ? scene->smallLayout.nQuads : 0;
        params.smallKappaT = scene->smallLayout.kappaT;
        params.scene.leafTris = quads ? scene->itemTris.ptr : scene->leafTris.ptr;
        const SmallTris &records = quads ? scene->smallItems : scene->smallTris;
        const size_t materialBytes = !generic && ldsMaterials ? (size_t)scene->device.nMaterials * sizeof(DMaterial) : 0;
        const auto choose = [&](auto STACK, auto SMALL) {
            const auto run = [&](auto kernel, auto... more) {
                hipLaunchKernelGGL(kernel, grid, dim3(kBlock), stackLdsBytes(STACK) + materialBytes, stream, params, records, more...);
            };
            if (list) {
                // k_list_volume<SMALL, GRID, MULTI>
                withBool(grids, [&](auto GRID) { withBool(multi, [&](auto MULTI) { run(k_list_volume<SMALL, GRID, MULTI>); }); });
            } else if (aniso) {
                // k_path_aniso / k_path_aniso_grid<STACK, SMALL>: the scatter family's shape with the per-slot g table as a third argument;
                // a tree scene's only form has 22 rows (`rows` above)
                if constexpr (SMALL || STACK == 22) { run(grids ? k_path_aniso_grid<STACK, SMALL> : k_path_aniso<STACK, SMALL>, (const float *)scene->phaseG.ptr); }
            } else if (multi) {
                // BasicVolumeIntegrator: k_path_scatter / k_path_scatter_grid<STACK, SMALL>
                run(grids ? k_path_scatter_grid<STACK, SMALL> : k_path_scatter<STACK, SMALL>);
            } else if (grids) {
                run(k_path_volume_grid<STACK, SMALL>);
            } else if constexpr (SMALL) {
                // k_path_volume<LDS_MATERIALS, STACK, SMALL, TRAITS, QUADS>
                if (ldsMaterials && scene->traits.lambertianGlassContainer) {   // the reference's own volume scene kinds
                    withBool(quads, [&](auto QUADS) { run(k_path_volume<true, STACK, true, TraitsLambertianGlassContainer, QUADS>); });
                } else if (quads) {
                    run(k_path_volume<true, STACK, true, TraitsAll, true>);
                } else {
                    withBool(ldsMaterials, [&](auto LDS_MATERIALS) { run(k_path_volume<LDS_MATERIALS, STACK, true>); });
                }
            } else {
                withBool(ldsMaterials, [&](auto LDS_MATERIALS) { run(k_path_volume<LDS_MATERIALS, STACK, false>); });
            }
        };
        if (small) { choose(std::integral_constant<int, 8>{}, std::true_type{}); }
        else { withStackRows(rows, [&](auto STACK) { choose(STACK, std::false_type{}); }); }
    });
}

// The path tracer over a BVH with the paths on chip (k_path_wave, path_wave.h).
static int renderPassWave(PathedScene *scene, const Pass &pass)
{
    const int stackRows = 22;
    return persistentPass(scene, pass, PATHED_WAVE_WAVES, scene->maxStack, stackRows, [&](RenderParams &params, dim3 grid, hipStream_t stream) {
        const size_t lds = pathWaveLdsBytes(stackRows, scene->device.nMaterials, PATHED_EXPERIMENTS && scene->waveBlock);
        params.suspendLanes = scene->waveStragglers;
        params.suspendPatience = scene->waveRefill;   // k_path_wave: idle lanes are refilled from the wave's list once fewer than this many are busy
        params.parkMinCardsPerWave = scene->waveShadeReady;   // k_path_wave<BLOCK>: a wave shades once this many of its paths have their rays back

        // k_path_wave<LDS_MATERIALS, STACK, TRAITS, SPHERES, BLOCK>
        const SceneTraitFlags &traits = scene->traits;
        const bool envOnly = traits.envOnly && scene->device.nSpheres == 0 && !scene->hasContainers;
        const auto run = [&](void (*kernel)(RenderParams)) { hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, params); };
#if PATHED_EXPERIMENTS
        // the block's waves sharing one ray ring: measured 13-20 % slower than a list per wave (profiles/r4_ab_wave.log)
        if (scene->waveBlock && envOnly) { run(k_path_wave<true, 22, TraitsEnvironmentOnly, false, true>); }
        else
#endif
        if (envOnly) { run(k_path_wave<true, 22, TraitsEnvironmentOnly, false>); }
        else if (traits.smoothSet) { run(k_path_wave<true, 22, TraitsSmooth, false>); }
        else if (traits.triangleLit) { run(k_path_wave<true, 22, TraitsTriangleLit, false>); }
        else if (scene->device.nSpheres == 0) { run(k_path_wave<true, 22, TraitsAll, false>); }
        else { run(k_path_wave<true, 22, TraitsAll, true>); }
    });
}

// The hybrid path kernel (k_path_hybrid, path_hybrid.h): a direct set of large triangles and a tree of its own for the rest.
static int renderPassHybrid(PathedScene *scene, const Pass &pass)
{
    return persistentPass(scene, pass, PATHED_HYBRID_WAVES, scene->hybridMaxStack, kHybridStackRows, [&](RenderParams &params, dim3 grid, hipStream_t stream) {
        const PathedSceneOptions &options = scene->options;
        const size_t lds = (size_t)scene->device.nMaterials * sizeof(DMaterial);
        params.smallQuads = scene->hybridLayout.nQuads;
        params.smallKappaT = scene->hybridLayout.kappaT;
        params.scene.leafTris = scene->hybridItemTris.ptr;   // the direct set in item order
        params.hybridNodes = scene->hybridNodes.ptr;
        params.hybridTris = scene->hybridTris.ptr;
        params.hybridNodeCount = scene->hybridNodeCount;
        params.hybridTreeTris = scene->hybridTreeTris;
        params.hybridDirectTris = scene->hybridDirectTris;
        for (int a = 0; a < 3; a++) { params.hybridLo[a] = scene->hybridLo[a]; params.hybridHi[a] = scene->hybridHi[a]; }
        for (int a = 0; a < 4; a++) { params.hybridSphere[a] = scene->hybridSphere[a]; }
        // scheduling of its bursts (PathedSceneOptions.wave_stragglers / wave_refill): results do not depend on them
        params.suspendLanes = options.wave_stragglers != 0 ? (options.wave_stragglers < 0 ? 0 : options.wave_stragglers) : kHybridStragglers;
        params.suspendPatience = options.wave_refill != 0 ? options.wave_refill : kHybridRefill;
        params.hybridBatch = options.hybrid_batch != 0 ? options.hybrid_batch : kHybridBatch;
        params.hybridReady = options.hybrid_ready != 0 ? (options.hybrid_ready < 0 ? 1 : options.hybrid_ready) : kHybridReady;

        // k_path_hybrid<TRAITS>: the narrowest instantiation whose compile-time scene set contains this scene's
        const SceneTraitFlags &traits = scene->traits;
        const auto run = [&](void (*kernel)(RenderParams, SmallTris)) { hipLaunchKernelGGL(kernel, grid, dim3(kBlock), lds, stream, params, scene->hybridItems); };
        if (traits.envOnly && !scene->hasContainers) { run(k_path_hybrid<TraitsEnvironmentOnly>); }
        else if (traits.smoothSet) { run(k_path_hybrid<TraitsSmooth>); }
        else if (traits.triangleLit) { run(k_path_hybrid<TraitsTriangleLit>); }
        else { run(k_path_hybrid<TraitsAll>); }
    });
}

// A pass on the wavefront kernels (k_init, k_trace / k_trace_small, k_shade over a pool of path slots in HBM).
// The slot pool is split into `pools` independent halves, each with its own unit range,
// counters and HIP stream: while one half runs its (ALU-bound) trace kernel the other runs its
// (memory-bound) shade kernel, so the two overlap instead of alternating.
static int renderPass(PathedScene *scene, const Pass &pass)
{
    const hipStream_t stream = pass.stream;
    const unsigned long long nUnits64 = pass.nUnits;

    // small jobs use one pool; otherwise split slots and units evenly
    int pools = scene->pools;
    if (nUnits64 < 4ull * kBlock * (unsigned long long)pools) { pools = 1; }

    unsigned long long wanted = nUnits64 < (unsigned long long)scene->maxSlots ? nUnits64 : (unsigned long long)scene->maxSlots;
    if (scene->adaptiveSlots) {
        // a slot should render at least 16 units in a call, or the ramp-up and the drain of the pool outweigh its size
        // (16 spp at 1024^2: 4 Mi slots 899, 8 Mi 794 Msamples/s on the teapot), but never fewer than 4 Mi
        const unsigned long long floorSlots = 1ull << 22;
        unsigned long long byWork = nUnits64 / 16ull;
        if (byWork < floorSlots) { byWork = floorSlots; }
        if (wanted > byWork) { wanted = byWork; }
    }
    // a block of the staged shade kernel owns stageRounds x 256 slots: pools are whole blocks
    const unsigned long long slotQuantum = (unsigned long long)kBlock * (scene->stagedShade ? scene->stageRounds : 1);
    const int slotsPerPool = (int)((wanted / pools + slotQuantum - 1) / slotQuantum * slotQuantum);
    const int nSlots = slotsPerPool * pools;
    int code = ensureRenderState(scene, nSlots, pass.bufferUnits());
    if (code != PATHED_OK) { return code; }
    if (pools > 1 && !scene->poolStreams[0]) {
        for (int h = 0; h < kMaxPools; h++) {
            HIP_TRY(hipStreamCreateWithFlags(&scene->poolStreams[h], hipStreamNonBlocking));
            HIP_TRY(hipEventCreateWithFlags(&scene->poolDone[h], hipEventDisableTiming));
        }
        HIP_TRY(hipEventCreateWithFlags(&scene->callerReady, hipEventDisableTiming));
    }

    const int blocksPerPool = slotsPerPool / kBlock;
    // every unit queue needs a consumer among the blocks of the shade kernel (a staged block owns stageRounds x 256 slots)
    const int shadeBlocks = blocksPerPool / (scene->stagedShade ? scene->stageRounds : 1);
    const int nQueues = shadeBlocks < kUnitQueues ? shadeBlocks : kUnitQueues;

    RenderParams params[kMaxPools];
    std::memset(params, 0, sizeof params);
    hipStream_t streams[kMaxPools] = { stream, stream, stream, stream };
    for (int h = 0; h < pools; h++) {
        RenderParams &q = params[h];
        const size_t slotBase = (size_t)h * slotsPerPool;
        if (!fillPassParams(q, scene, pass, h, pools, nQueues)) { return fail(PATHED_E_INVALID, "too many work units in one pass"); }
        q.state.rayO = scene->rayO.ptr + slotBase;
        q.state.rayD = scene->rayD.ptr + slotBase;
        q.state.hit = scene->hit.ptr + slotBase;
        q.state.mod = scene->mod.ptr + slotBase;
        q.state.thr = scene->thr.ptr + slotBase;
        q.state.res = scene->res.ptr + slotBase;
        q.state.pend = scene->pend.ptr + slotBase;
        q.state.acc = scene->acc.ptr + slotBase;
        q.state.shO = scene->shO.ptr + slotBase;
        q.state.shD = scene->shD.ptr + slotBase;
        if (scene->splitShade) {
            const size_t listEntries = (size_t)scene->listCap * kListShards * 64;
            for (int list = 0; list < 2; list++) {
                q.state.lists[list] = scene->slotLists.ptr + ((size_t)h * 2 + list) * listEntries;
                for (int parity = 0; parity < 2; parity++) {
                    q.state.deferred[list][parity] = scene->deferredLists.ptr + (((size_t)h * 2 + list) * 2 + parity) * (size_t)scene->nSlots;
                }
            }
            q.listCap = scene->listCap;
        }
        const size_t traceWaves = (size_t)scene->traceGrid * kWavesPerBlock;
        q.suspendLanes = (scene->bruteForce || scene->instanced) ? 0 : scene->suspendLanes;   // (k_trace_small and k_trace_instanced park nothing)
        q.suspendPatience = scene->suspendPatience;
        q.parkMinCardsPerWave = scene->parkMinCards;
        q.suspendMask = scene->bruteForce ? nullptr : scene->suspendMask.ptr + (size_t)h * traceWaves;
        q.suspendData = scene->bruteForce ? nullptr
            : scene->suspendData.ptr + (size_t)h * traceWaves * (size_t)(kSaveWords + scene->maxStack) * 64;
        q.stackOverflow = scene->bruteForce ? nullptr : scene->stackOverflow.ptr + (size_t)h * stackSpillInts((size_t)scene->traceGrid * kBlock, scene->maxStack, scene->stackRows);
        q.maxStack = scene->maxStack;
        q.nSlots = slotsPerPool;
        // local rays (per-slot shade kernel only: the staged and split stages of the experiments build do not know them)
        q.localCount = (!scene->stagedShade && !scene->splitShade) ? scene->localCount : 0;
        q.localCounting = scene->countMode ? 1 : 0;
        q.afterTrace = 1;
        if (q.localCount > 0) {
            std::memcpy(q.localTris, scene->localTris, sizeof q.localTris);
            for (int a = 0; a < 3; a++) { q.hybridLo[a] = scene->localLo[a]; q.hybridHi[a] = scene->localHi[a]; }
            for (int a = 0; a < 4; a++) { q.hybridSphere[a] = scene->localSphere[a]; }
        }
        if (pools > 1) { streams[h] = scene->poolStreams[h]; }
    }

    if (pools > 1) {
        // the pool streams start after whatever the caller queued on its stream
        HIP_TRY(hipEventRecord(scene->callerReady, stream));
        for (int h = 0; h < pools; h++) { HIP_TRY(hipStreamWaitEvent(streams[h], scene->callerReady, 0)); }
    }

    const dim3 slotGrid((unsigned)blocksPerPool), block(kBlock);
    for (int h = 0; h < pools; h++) {
        HIP_TRY(hipMemsetAsync(params[h].counters, 0, kCtrCount * sizeof(unsigned int), streams[h]));
        if (params[h].suspendMask) {
            HIP_TRY(hipMemsetAsync(params[h].suspendMask, 0, (size_t)scene->traceGrid * kWavesPerBlock * sizeof(unsigned long long), streams[h]));
        }
        hipLaunchKernelGGL(k_init, slotGrid, block, 0, streams[h], params[h]);
    }

    // Iterate until every slot of every pool has run out of units.  `remaining` is polled with
    // a lag of one chunk of launches so the GPU never waits for the host.
    const int launchChunk = 8;
    const int ringSize = 32;
    // the poll events are destroyed and the pool streams drained on every way out, error or not
    struct PollGuard {
        hipEvent_t events[kMaxPools][2] = {};
        hipStream_t *streams = nullptr;
        int pools = 0;
        ~PollGuard()
        {
            for (int h = 0; h < pools; h++) { (void)hipStreamSynchronize(streams[h]); }
            for (int h = 0; h < kMaxPools; h++) {
                for (int k = 0; k < 2; k++) { if (events[h][k]) { (void)hipEventDestroy(events[h][k]); } }
            }
        }
    } guard;
    guard.streams = streams;
    guard.pools = pools;
    hipEvent_t (&pollEvents)[kMaxPools][2] = guard.events;
    for (int h = 0; h < pools; h++) {
        HIP_TRY(hipEventCreateWithFlags(&pollEvents[h][0], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&pollEvents[h][1], hipEventDisableTiming));
    }
    const int shadeLaunches = params[0].localCount > 0 ? (scene->options.shade_launches > 0 ? scene->options.shade_launches : kDefaultShadeLaunches) : 1;
    unsigned long long iteration = 0;
    int pollIndex = 0;
    bool havePending = false;
    bool poolDone[kMaxPools];
    for (int h = 0; h < kMaxPools; h++) { poolDone[h] = h >= pools; }
    while (!(poolDone[0] && poolDone[1] && poolDone[2] && poolDone[3])) {
        for (int k = 0; k < launchChunk; k++) {
            for (int h = 0; h < pools; h++) {
                if (poolDone[h]) { continue; }
                params[h].parity = (int)(iteration & 1ull);
                scene->traceLaunchesAll++;
#if defined(PATHED_EXPERIMENTS) && PATHED_EXPERIMENTS
                if (h == 0) {
                    if (const char *text = tuningEnv("PATHED_SORT_PROBE")) {
                        if (iteration == (unsigned long long)atoll(text)) { sortProbe(scene, params[h], streams[h]); }
                    }
                }
#endif
                if (scene->timeKernels && iteration % (unsigned long long)scene->timeInterval == 0ull) {
                    const int e = scene->traceEvents.acquire();
                    (void)hipEventRecord(scene->traceEvents.start[e], streams[h]);
                    launchTrace(scene, params[h], streams[h]);
                    (void)hipEventRecord(scene->traceEvents.stop[e], streams[h]);
                    const int s = scene->shadeEvents.acquire();
                    (void)hipEventRecord(scene->shadeEvents.start[s], streams[h]);
                    for (int round = 0; round < shadeLaunches; round++) {
                        params[h].afterTrace = round == 0 ? 1 : 0;
                        launchShade(scene, params[h], streams[h]);
                    }
                    (void)hipEventRecord(scene->shadeEvents.stop[s], streams[h]);
                } else {
                    launchTrace(scene, params[h], streams[h]);
                    // with local rays: several shade launches per trace launch -- the slots whose rays were all local advance
                    // another vertex each time, the others wait; the trace kernel then finds the hard rays of several vertices
                    // in ONE launch
                    for (int round = 0; round < shadeLaunches; round++) {
                        params[h].afterTrace = round == 0 ? 1 : 0;
                        launchShade(scene, params[h], streams[h]);
                    }
                }
            }
            iteration++;
        }
        const int slotIndex = pollIndex % ringSize;
        for (int h = 0; h < pools; h++) {
            if (poolDone[h]) { continue; }
            HIP_TRY(hipMemcpyAsync(scene->hostRemaining + h * ringSize + slotIndex, params[h].counters + kCtrRemaining,
                                   sizeof(unsigned int), hipMemcpyDeviceToHost, streams[h]));
            HIP_TRY(hipEventRecord(pollEvents[h][pollIndex & 1], streams[h]));
        }
        if (havePending) {
            const int previous = pollIndex - 1;
            for (int h = 0; h < pools; h++) {
                if (poolDone[h]) { continue; }
                HIP_TRY(hipEventSynchronize(pollEvents[h][previous & 1]));
                if (scene->hostRemaining[h * ringSize + previous % ringSize] == 0) { poolDone[h] = true; }
            }
        }
        havePending = true;
        pollIndex++;
    }
    if (pools > 1) {
        for (int h = 0; h < pools; h++) {
            HIP_TRY(hipEventRecord(scene->poolDone[h], streams[h]));
            HIP_TRY(hipStreamWaitEvent(stream, scene->poolDone[h], 0));
        }
    }
    launchResolve(pass, params[0], stream);
    for (int h = 0; h < pools; h++) { HIP_TRY(hipStreamSynchronize(streams[h])); }
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(hipGetLastError());

    scene->iterations += iteration;
    scene->cameraSamples += (unsigned long long)pass.count * (unsigned long long)pass.unitPixels();
    return PATHED_OK;
}

// k_features (features.h) over samples [begin, begin + count) of every pixel: the feature sums of `out`, or -- reference: the
// albedo integrator -- rgb sums into `accum`.  One launch; returns when it has completed.
static int launchFeatures(PathedScene *scene, uint64_t seed, uint32_t begin, uint32_t count, int startBounce, int lastBounce,
                          bool reference, float *accum, const FeatureBuffers &out, hipStream_t stream)
{
    if (const int code = ensureStats(scene)) { return code; }
    // a wave per 8 x 8 tile; the grid is what the kernel's register budget keeps resident (four blocks per CU) or fewer
    const unsigned long long tiles = (unsigned long long)((scene->width + 7) / 8) * (unsigned long long)((scene->height + 7) / 8);
    unsigned long long blocks = (tiles + kWavesPerBlock - 1) / kWavesPerBlock;
    const unsigned long long resident = (unsigned long long)scene->computeUnits * 4ull;
    if (blocks > resident) { blocks = resident; }
    if (blocks < 1) { blocks = 1; }

    RenderParams params;
    std::memset(&params, 0, sizeof params);
    const size_t overflowInts = stackSpillInts((size_t)blocks * kBlock, scene->maxStack, scene->stackRows);
    if (scene->volumeOverflow.count < overflowInts) { HIP_TRY(scene->volumeOverflow.allocate(overflowInts)); }
    params.stackOverflow = scene->volumeOverflow.ptr;
    params.maxStack = scene->maxStack;
    params.scene = scene->device;
    params.stats = scene->stats.ptr;
    params.accum = accum;
    params.nPixels = scene->width * scene->height;
    params.divWidth = makeFastDiv((unsigned int)scene->width);
    params.seedLo = (uint32_t)seed;
    params.seedHi = (uint32_t)(seed >> 32);
    params.sppBegin = begin;
    params.sppEnd = begin + count;
    params.startBounce = startBounce;
    params.lastBounce = lastBounce;

    int timed = -1;
    if (scene->timeKernels) {
        HIP_TRY(scene->traceEvents.create());
        timed = scene->traceEvents.acquire();
        (void)hipEventRecord(scene->traceEvents.start[timed], stream);
    }
    const dim3 grid((unsigned)blocks), block(kBlock);
    withBool(reference, [&](auto REFERENCE) {
        withStackRows(scene->stackRows, [&](auto STACK) { hipLaunchKernelGGL((k_features<STACK, REFERENCE>), grid, block, stackLdsBytes(STACK), stream, params, out); });
    });
    if (timed >= 0) { (void)hipEventRecord(scene->traceEvents.stop[timed], stream); }
    scene->traceLaunchesAll++;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (scene->timeKernels) { scene->traceEvents.harvestAll(); }

    const unsigned long long samples = (unsigned long long)count * (unsigned long long)scene->width * (unsigned long long)scene->height;
    scene->iterations += 1;
    scene->cameraSamples += samples;
    scene->featureRays += samples;
    scene->lastCallFeatures = true;
    return PATHED_OK;
}

// k_check_list over a list in device memory: PATHED_OK, or PATHED_E_INVALID for a list that is not strictly ascending or
// leaves the image.  Returns when the check has completed.
static int checkPixelList(PathedScene *scene, const uint32_t *d_list, uint32_t count, hipStream_t stream)
{
    const int nPixels = scene->width * scene->height;
    if (count > (uint32_t)nPixels) { return fail(PATHED_E_INVALID, "the pixel list is longer than the image has pixels"); }
    DeviceBuffer<unsigned int> flag;
    HIP_TRY(flag.allocate(1));
    HIP_TRY(hipMemsetAsync(flag.ptr, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(k_check_list, dim3((count + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, d_list, (int)count, nPixels, flag.ptr);
    HIP_TRY(hipGetLastError());
    unsigned int bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, flag.ptr, sizeof bad, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad) { return fail(PATHED_E_INVALID, "the pixel list must be strictly ascending with every index below width * height"); }
    return PATHED_OK;
}

// The pixels of a render call: every pixel of the image (list null), or a list of them in device memory with the count image
// that goes with it (pathed_hip_render_pixels_device).
struct PixelList {
    const uint32_t *list;
    uint32_t count;
    uint32_t *sampleCounts;
};

// The body of pathed_hip_render_device, pathed_hip_render_moments_device and pathed_hip_render_pixels_device: d_squares is null
// for the first and `pixels` for the first two, and a call without them launches exactly what it always did.
static int renderCall(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count, int start_bounce, int last_bounce,
                      float *d_accum_rgb_sum, float *d_squares, void *stream_handle, const PixelList *pixels = nullptr)
{
    if (!scene || !d_accum_rgb_sum) { return fail(PATHED_E_INVALID, "null scene or accumulation buffer"); }
    if (start_bounce < 0 || (last_bounce != -1 && start_bounce > last_bounce)) {
        return fail(PATHED_E_INVALID, "bounce window: need 0 <= startBounce <= lastBounce (or lastBounce == -1)");
    }
    if (spp_count == 0) { return PATHED_OK; }
    if ((uint64_t)spp_begin + spp_count > 0x7fffffffull) { return fail(PATHED_E_INVALID, "sample index overflow"); }
    if (scene->instanced && scene->integrator != PATHED_INTEGRATOR_PATH_TRACER) {
        return fail(PATHED_E_UNSUPPORTED, "a scene with instances renders with the PathTracer integrator only: the volume integrators, the basic volume "
                                          "integrator and the albedo integrator do not know the two-level tree");
    }
    if (scene->integrator == PATHED_INTEGRATOR_ALBEDO) {
        // AlbedoIntegrator::L never looks at the bounce window: last_bounce is ignored, start_bounce decides bounce 0's emission
        if (scene->hasContainers) { return fail(PATHED_E_UNSUPPORTED, "the albedo integrator does not render scenes with passthrough (medium container) surfaces"); }
        if (!scene->gridsHost.empty()) { return fail(PATHED_E_UNSUPPORTED, "a scene with a voxel-grid medium renders with the VolumePathTracer integrator only"); }
        SELECT_DEVICE(scene);
        FeatureBuffers none = { nullptr, nullptr, nullptr, nullptr };
        return launchFeatures(scene, seed, spp_begin, spp_count, start_bounce, -1, true, d_accum_rgb_sum, none, (hipStream_t)stream_handle);
    }
    if (scene->hasContainers && !volumeIntegrator(scene)) {
        return fail(PATHED_E_UNSUPPORTED, "the scene has passthrough (medium container) surfaces: select the VolumePathTracer integrator (pathed_hip_set_integrator)");
    }
    if (!scene->gridsHost.empty() && !volumeIntegrator(scene)) {
        return fail(PATHED_E_UNSUPPORTED, "a scene with a voxel-grid medium renders with the VolumePathTracer integrator only (pathed_hip_set_integrator)");
    }
    if (scene->anisotropic && volumeIntegrator(scene)) {
        // Henyey-Greenstein media exist on BasicVolumeIntegrator's whole-image kernels alone (k_path_aniso, kernels.h)
        if (scene->integrator == PATHED_INTEGRATOR_VOLUME_PATH_TRACER) {
            return fail(PATHED_E_UNSUPPORTED, "the scene has a Henyey-Greenstein medium: VolumePathTracer scatters isotropically only, select the "
                                              "BasicVolumeIntegrator (pathed_hip_set_integrator)");
        }
        if (pixels) {
            return fail(PATHED_E_UNSUPPORTED, "the scene has a Henyey-Greenstein medium: pixel lists are not rendered on the anisotropic kernels "
                                              "(k_list_volume scatters isotropically only)");
        }
    }
    SELECT_DEVICE(scene);
    hipStream_t stream = (hipStream_t)stream_handle;
    if (pixels) {
        // list passes run on the wavefront kernels or k_list_volume, the only ones that know the list order (kernels.h: THE UNIT ORDER)
        if (scene->stagedShade || scene->splitShade) { return fail(PATHED_E_UNSUPPORTED, "pixel lists are not rendered by the staged or split shade stages"); }
        // before anything else of a list render: a bad list renders nothing
        const int code = checkPixelList(scene, pixels->list, pixels->count, stream);
        if (code != PATHED_OK) { return code; }
    }
    scene->lastCallFeatures = false;

    if (scene->timeKernels) {
        HIP_TRY(scene->traceEvents.create());
        HIP_TRY(scene->shadeEvents.create());
    }

    // passes of at most chunk * kMaxChunksPerPass samples keep the partial-sum buffer bounded
    int chunksPerPass = kMaxChunksPerPass;
    {
        const unsigned long long pixels = (unsigned long long)scene->width * (unsigned long long)scene->height;
        const unsigned long long cap = (1ull << 30) / (pixels ? pixels : 1ull);   // 2^30 partial sums = 17 GB
        if ((unsigned long long)chunksPerPass > cap) { chunksPerPass = cap >= 1ull ? (int)cap : 1; }
    }
    if (scene->options.chunks_per_pass > 0) { chunksPerPass = scene->options.chunks_per_pass; }
    if (const char *text = tuningEnv("PATHED_CHUNKS_PER_PASS")) {   // tuning: fewer, longer passes at the cost of a larger partial-sum buffer
        const int value = atoi(text);
        if (value >= 1 && value <= 4096) { chunksPerPass = value; }
    }
    const uint32_t perPass = (uint32_t)scene->samplesPerUnit * (uint32_t)chunksPerPass;
    // BVH scenes: short calls on the wave path kernel, long ones on the wavefront (the counting instantiations are the wavefront's)
    // (a call over a pixel list counts the samples it renders: those of the listed pixels)
    const unsigned long long callPixels = pixels ? (unsigned long long)pixels->count : (unsigned long long)scene->width * (unsigned long long)scene->height;
    const unsigned long long callSamples = callPixels * (unsigned long long)spp_count;
    const bool wavePath = scene->waveAvailable && !usesVolumeKernel(scene) && !scene->countMode
        && (scene->waveMode == 2 || (scene->waveMode == 0 && (callSamples < scene->waveMaxSamples || scene->sceneInLds)));
    // (trees small enough for the trace kernel's LDS copy -- the Cornell box with its two meshes: k_path_wave, whose node reads
    // hit L1 / L2, is level with the wavefront or 11 % ahead at every length, profiles/r4_ab_wave.log)
    // [r5] ... and scenes of 65 .. 4096 triangles on the hybrid kernel at every length (counting is the wavefront's)
    const bool hybridPath = scene->hybridPath && !usesVolumeKernel(scene) && !scene->countMode;
    const bool listPass = pixels != nullptr;   // ... and a call over a pixel list on the wavefront (k_list_volume with media), whatever the scene
    scene->lastCallWave = wavePath && !hybridPath && !listPass && !scene->instanced;
    scene->lastCallHybrid = hybridPath && !listPass;
    scene->lastCallList = listPass;
    Pass pass;
    pass.seed = seed;
    pass.startBounce = start_bounce;
    pass.lastBounce = last_bounce;
    pass.accum = d_accum_rgb_sum;
    pass.squares = d_squares;
    pass.stream = stream;
    pass.nPixels = scene->width * scene->height;
    pass.chunk = scene->samplesPerUnit;
    pass.pixelList = pixels ? pixels->list : nullptr;
    pass.nList = pixels ? (int)pixels->count : 0;
    pass.counts = pixels ? pixels->sampleCounts : nullptr;
    uint32_t done = 0;
    while (done < spp_count) {
        pass.begin = spp_begin + done;
        pass.count = (spp_count - done < perPass) ? (spp_count - done) : perPass;
        pass.chunksPerPixel = (int)((pass.count + (uint32_t)pass.chunk - 1) / (uint32_t)pass.chunk);
        const unsigned long long nUnits = (unsigned long long)pass.unitPixels() * (unsigned long long)pass.chunksPerPixel;
        if (nUnits >= 0xFFFFFFF0ull) { return fail(PATHED_E_INVALID, "too many work units in one pass"); }
        pass.nUnits = (unsigned int)nUnits;
        const int code = scene->instanced ? renderPass(scene, pass)
            : usesVolumeKernel(scene) ? renderPassVolume(scene, pass)
            : listPass ? renderPass(scene, pass)
            : scene->fusedPath ? renderPassFused(scene, pass)
            : hybridPath ? renderPassHybrid(scene, pass)
            : wavePath ? renderPassWave(scene, pass)
            : renderPass(scene, pass);
        if (code != PATHED_OK) { return code; }
        done += pass.count;
    }
    if (scene->timeKernels) {
        scene->traceEvents.harvestAll();
        scene->shadeEvents.harvestAll();
    }
    return PATHED_OK;
}

// The test and measurement hooks that are one launch of a thread per record: selects the scene's device, uploads the float
// arrays of `inputs`, makes and zeroes the device arrays of `outputs`, calls launch(grid, in, out) -- a block per kBlock of the n
// records; in and out hold the DeviceBuffers in the order given --, waits for the kernel and downloads the outputs.
struct HookInput { const float *host; size_t count; };
template <typename T> struct HookOutput { T *host; size_t count; };

template <typename T, typename Launch>
static int recordHook(PathedScene *scene, size_t n, std::initializer_list<HookInput> inputs, std::initializer_list<HookOutput<T>> outputs, Launch launch)
{
    SELECT_DEVICE(scene);
    std::vector<DeviceBuffer<float>> in(inputs.size());
    std::vector<DeviceBuffer<T>> out(outputs.size());
    size_t k = 0;
    for (const HookInput &input : inputs) {
        HIP_TRY(in[k].allocate(input.count));
        HIP_TRY(hipMemcpy(in[k++].ptr, input.host, input.count * sizeof(float), hipMemcpyHostToDevice));
    }
    k = 0;
    for (const HookOutput<T> &output : outputs) {
        HIP_TRY(out[k].allocate(output.count));
        HIP_TRY(hipMemset(out[k++].ptr, 0, output.count * sizeof(T)));
    }
    launch(dim3((unsigned)((n + kBlock - 1) / kBlock)), in, out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    k = 0;
    for (const HookOutput<T> &output : outputs) { HIP_TRY(hipMemcpy(output.host, out[k++].ptr, output.count * sizeof(T), hipMemcpyDeviceToHost)); }
    return PATHED_OK;
}

// the candidate hooks' records (an origin, two directions and a far bound: 10 floats) padded to whole blocks, since every lane
// reads one (and issues the matrix instructions); a padding record's directions are +z
static std::vector<float> paddedRays(const float *rays, size_t n)
{
    const size_t padded = (n + kBlock - 1) / kBlock * kBlock;
    std::vector<float> host(padded * 10, 0.f);
    std::memcpy(host.data(), rays, n * 10 * sizeof(float));
    for (size_t i = n; i < padded; i++) { host[10 * i + 5] = 1.f; host[10 * i + 8] = 1.f; }
    return host;
}

// ... and the four counts of an item list they report
static void fillLayout(int32_t *layout, const SmallItemsLayout &list)
{
    layout[0] = list.nQuads;
    layout[1] = list.nLone;
    layout[2] = list.shadowQuadPairs;
    layout[3] = list.shadowLonePairs;
}

extern "C" {

int pathed_hip_render_device(PathedScene *scene, uint64_t seed,
                             uint32_t spp_begin, uint32_t spp_count,
                             int start_bounce, int last_bounce,
                             float *d_accum_rgb_sum, void *stream_handle, int blocking)
{
    (void)blocking;  // the iteration loop polls a device counter, so the call always completes
    return renderCall(scene, seed, spp_begin, spp_count, start_bounce, last_bounce, d_accum_rgb_sum, nullptr, stream_handle);
}

int pathed_hip_render_moments_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                                     int start_bounce, int last_bounce, float *d_rgb_sum, float *d_rgb_sq_sum, void *stream_handle)
{
    if (!scene || !d_rgb_sum || !d_rgb_sq_sum) { return fail(PATHED_E_INVALID, "null scene, sum buffer or sum-of-squares buffer"); }
    if (scene->samplesPerUnit != 1) {
        return fail(PATHED_E_INVALID, "second moments need one sample per unit (pathed_hip_set_samples_per_unit(scene, 1)): with more, "
                                      "a unit's entry is the sum of a group of samples and the last group of a call is ragged");
    }
    if (scene->integrator == PATHED_INTEGRATOR_ALBEDO) {
        return fail(PATHED_E_UNSUPPORTED, "second moments are not rendered under the albedo integrator: its render calls run the feature kernel, which has no unit buffer");
    }
    return renderCall(scene, seed, spp_begin, spp_count, start_bounce, last_bounce, d_rgb_sum, d_rgb_sq_sum, stream_handle);
}

int pathed_hip_render_moments(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                              int start_bounce, int last_bounce, float *rgb_sum, float *rgb_sq_sum)
{
    if (!scene || !rgb_sum || !rgb_sq_sum) { return fail(PATHED_E_INVALID, "null scene, sum buffer or sum-of-squares buffer"); }
    SELECT_DEVICE(scene);
    // one device buffer, the two images side by side, zeroed: the call's sums are ADDED to the caller's, as pathed_hip_render does
    const size_t count = (size_t)3 * scene->width * scene->height;
    DeviceBuffer<float> device;
    HIP_TRY(device.allocate(2 * count));
    HIP_TRY(hipMemset(device.ptr, 0, 2 * count * sizeof(float)));
    const int code = pathed_hip_render_moments_device(scene, seed, spp_begin, spp_count, start_bounce, last_bounce, device.ptr, device.ptr + count, nullptr);
    if (code != PATHED_OK) { return code; }
    std::vector<float> host(2 * count);
    HIP_TRY(hipMemcpy(host.data(), device.ptr, 2 * count * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; i++) {
        rgb_sum[i] += host[i];
        rgb_sq_sum[i] += host[count + i];
    }
    return PATHED_OK;
}

// The per-block partial sums of k_noise / k_noise_select, read back and folded in block order (the double sum and the float
// maximum depend on it) into `out`; `host` keeps them for the caller.  Returns when the kernel before it on `stream` has.
static int reduceNoisePartials(const DeviceBuffer<NoisePartial> &partials, int nPixels, hipStream_t stream, std::vector<NoisePartial> &host, PathedNoise *out)
{
    host.resize(partials.count);
    HIP_TRY(hipMemcpyAsync(host.data(), partials.ptr, host.size() * sizeof(NoisePartial), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    double sum = 0.0;
    float maxError = 0.f;
    uint64_t above = 0;
    uint32_t invalid = 0;
    for (const NoisePartial &partial : host) {
        sum += partial.sum;
        if (partial.maxError > maxError) { maxError = partial.maxError; }
        above += partial.above;
        invalid += partial.invalid;
    }
    out->invalid_pixels = invalid;
    out->mean_error = sum / (double)nPixels;
    out->max_error = (double)maxError;
    out->pixels_above = above;
    return PATHED_OK;
}

int pathed_hip_noise_estimate_device(PathedScene *scene, const float *d_rgb_sum, const float *d_rgb_sq_sum, uint32_t n_samples,
                                     float floor, float threshold, float *d_error, PathedNoise *out, void *stream_handle)
{
    if (!scene || !d_rgb_sum || !d_rgb_sq_sum || !out) { return fail(PATHED_E_INVALID, "null scene, sum buffer, sum-of-squares buffer or result"); }
    if (out->struct_size != sizeof(PathedNoise)) { return fail(PATHED_E_INVALID, "PathedNoise.struct_size does not match this library"); }
    if (n_samples < 2) { return fail(PATHED_E_INVALID, "a noise estimate needs at least 2 samples per pixel"); }
    if (!(floor > 0.f) || !std::isfinite(floor)) { return fail(PATHED_E_INVALID, "the noise floor must be a finite number > 0"); }
    SELECT_DEVICE(scene);
    hipStream_t stream = (hipStream_t)stream_handle;
    const int nPixels = scene->width * scene->height;
    const unsigned int blocks = (unsigned int)((nPixels + kBlock - 1) / kBlock);
    DeviceBuffer<NoisePartial> partials;
    HIP_TRY(partials.allocate(blocks));
    NoiseParams params;
    params.sum = d_rgb_sum;
    params.squares = d_rgb_sq_sum;
    params.nPixels = nPixels;
    params.n = (float)n_samples;
    params.bessel = params.n / (params.n - 1.f);
    params.floor = floor;
    params.threshold = threshold;
    params.error = d_error;
    params.partials = partials.ptr;
    hipLaunchKernelGGL(k_noise, dim3(blocks), dim3(kBlock), 0, stream, params);
    HIP_TRY(hipGetLastError());
    std::vector<NoisePartial> host;
    return reduceNoisePartials(partials, nPixels, stream, host, out);
}

int pathed_hip_select_pixels_device(PathedScene *scene, const float *d_rgb_sum, const float *d_rgb_sq_sum, const uint32_t *d_count,
                                    float floor, float threshold, float *d_error, uint32_t *d_list, uint32_t *n_list,
                                    PathedNoise *out, void *stream_handle)
{
    if (!scene || !d_rgb_sum || !d_rgb_sq_sum || !d_count || !d_list || !n_list || !out) {
        return fail(PATHED_E_INVALID, "null scene, sum buffer, sum-of-squares buffer, count image, list, list length or result");
    }
    if (out->struct_size != sizeof(PathedNoise)) { return fail(PATHED_E_INVALID, "PathedNoise.struct_size does not match this library"); }
    if (!(floor > 0.f) || !std::isfinite(floor)) { return fail(PATHED_E_INVALID, "the noise floor must be a finite number > 0"); }
    SELECT_DEVICE(scene);
    hipStream_t stream = (hipStream_t)stream_handle;
    const int nPixels = scene->width * scene->height;
    const unsigned int blocks = (unsigned int)((nPixels + kBlock - 1) / kBlock);
    DeviceBuffer<NoisePartial> partials;
    DeviceBuffer<uint32_t> selected, offsets;
    HIP_TRY(partials.allocate(blocks));
    HIP_TRY(selected.allocate((size_t)blocks * kBlock));
    HIP_TRY(offsets.allocate((size_t)blocks + 1));
    NoiseSelectParams params;
    params.sum = d_rgb_sum;
    params.squares = d_rgb_sq_sum;
    params.count = d_count;
    params.nPixels = nPixels;
    params.floor = floor;
    params.threshold = threshold;
    params.error = d_error;
    params.partials = partials.ptr;
    params.selected = selected.ptr;
    hipLaunchKernelGGL(k_noise_select, dim3(blocks), dim3(kBlock), 0, stream, params);
    HIP_TRY(hipGetLastError());
    std::vector<NoisePartial> host;
    if (const int code = reduceNoisePartials(partials, nPixels, stream, host, out)) { return code; }
    std::vector<uint32_t> hostOffsets((size_t)blocks + 1, 0u);
    for (unsigned int b = 0; b < blocks; b++) { hostOffsets[b + 1] = hostOffsets[b] + host[b].unused; }   // the block's selected pixels
    const uint32_t total = hostOffsets[blocks];
    if (total > 0u) {
        HIP_TRY(hipMemcpyAsync(offsets.ptr, hostOffsets.data(), hostOffsets.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        hipLaunchKernelGGL(k_place_list, dim3(blocks), dim3(kBlock), 0, stream, selected.ptr, offsets.ptr, d_list);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *n_list = total;
    return PATHED_OK;
}

int pathed_hip_render_pixels_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count, int start_bounce, int last_bounce,
                                    const uint32_t *d_list, uint32_t n_list, float *d_rgb_sum, float *d_rgb_sq_sum, uint32_t *d_count,
                                    void *stream_handle)
{
    if (!scene || !d_rgb_sum || !d_rgb_sq_sum || !d_count) { return fail(PATHED_E_INVALID, "null scene, sum buffer, sum-of-squares buffer or count image"); }
    if (scene->samplesPerUnit != 1) {
        return fail(PATHED_E_INVALID, "a render over a pixel list keeps second moments and needs one sample per unit (pathed_hip_set_samples_per_unit(scene, 1))");
    }
    if (scene->integrator == PATHED_INTEGRATOR_ALBEDO) {
        return fail(PATHED_E_UNSUPPORTED, "pixel lists are not rendered under the albedo integrator: its render calls run the feature kernel, which has no unit buffer");
    }
    if (n_list == 0) { return PATHED_OK; }
    if (!d_list) { return fail(PATHED_E_INVALID, "null pixel list"); }
    const PixelList pixels = { d_list, n_list, d_count };
    return renderCall(scene, seed, spp_begin, spp_count, start_bounce, last_bounce, d_rgb_sum, d_rgb_sq_sum, stream_handle, &pixels);
}

int pathed_hip_scene_set_camera(PathedScene *scene, const PathedCamera *camera)
{
    if (!scene || !camera) { return fail(PATHED_E_INVALID, "null scene or camera"); }
    if (camera->width != scene->width || camera->height != scene->height) {
        return fail(PATHED_E_INVALID, "the new camera must keep the scene's resolution (the radiance sums are per pixel)");
    }
    buildCamera(*camera, &scene->device.camera);
    SELECT_DEVICE(scene);
    HIP_TRY(rebuildSmallItems(scene));   // tiny scenes: the phase-1 tolerances depend on how far away a ray may start
    HIP_TRY(rebuildCameraMasks(scene));  // ... and which triangles a pixel's camera rays can meet on where the camera is
    HIP_TRY(rebuildHybridItems(scene));  // ... and so do the hybrid kernel's direct set's
    return PATHED_OK;
}

int pathed_hip_set_integrator(PathedScene *scene, int integrator)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (integrator != PATHED_INTEGRATOR_PATH_TRACER && integrator != PATHED_INTEGRATOR_VOLUME_PATH_TRACER && integrator != PATHED_INTEGRATOR_ALBEDO
        && integrator != PATHED_INTEGRATOR_BASIC_VOLUME) {
        return fail(PATHED_E_INVALID, "unknown integrator");
    }
    scene->integrator = integrator;
    return PATHED_OK;
}

int pathed_hip_set_samples_per_unit(PathedScene *scene, int samples)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (samples < 1 || samples > kMaxChunk) { return fail(PATHED_E_INVALID, "samples per unit must be in [1, 128]"); }
    scene->samplesPerUnit = samples;
    return PATHED_OK;
}

int pathed_hip_render(PathedScene *scene, uint64_t seed,
                      uint32_t spp_begin, uint32_t spp_count,
                      int start_bounce, int last_bounce,
                      float *accum_rgb_sum)
{
    if (!scene || !accum_rgb_sum) { return fail(PATHED_E_INVALID, "null scene or accumulation buffer"); }
    SELECT_DEVICE(scene);
    const size_t count = (size_t)3 * scene->width * scene->height;
    DeviceBuffer<float> deviceAccum;
    HIP_TRY(deviceAccum.allocate(count));
    HIP_TRY(hipMemset(deviceAccum.ptr, 0, count * sizeof(float)));

    const int code = pathed_hip_render_device(scene, seed, spp_begin, spp_count, start_bounce, last_bounce, deviceAccum.ptr, nullptr, 1);
    if (code != PATHED_OK) { return code; }

    std::vector<float> host(count);
    HIP_TRY(hipMemcpy(host.data(), deviceAccum.ptr, count * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < count; i++) { accum_rgb_sum[i] += host[i]; }
    return PATHED_OK;
}

int pathed_hip_render_features_device(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                                      const PathedFeatureBuffers *buffers, void *stream_handle)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (!buffers || (!buffers->albedo_sum && !buffers->normal_sum && !buffers->depth_sum && !buffers->hit_count)) {
        return fail(PATHED_E_INVALID, "no feature buffer: pass at least one of albedo, normal, depth, hits");
    }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "feature images do not cover scenes with instances"); }
    if (spp_count == 0) { return PATHED_OK; }
    if ((uint64_t)spp_begin + spp_count > 0x7fffffffull) { return fail(PATHED_E_INVALID, "sample index overflow"); }
    if (scene->hasContainers) { return fail(PATHED_E_UNSUPPORTED, "feature images do not cover scenes with passthrough (medium container) surfaces"); }
    if (!scene->gridsHost.empty()) { return fail(PATHED_E_UNSUPPORTED, "feature images do not cover scenes with a voxel-grid medium"); }
    SELECT_DEVICE(scene);
    const FeatureBuffers out = { buffers->albedo_sum, buffers->normal_sum, buffers->depth_sum, buffers->hit_count };
    return launchFeatures(scene, seed, spp_begin, spp_count, 0, -1, false, nullptr, out, (hipStream_t)stream_handle);
}

int pathed_hip_render_features(PathedScene *scene, uint64_t seed, uint32_t spp_begin, uint32_t spp_count,
                               float *albedo, float *normal, float *depth, float *hits)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (!albedo && !normal && !depth && !hits) { return fail(PATHED_E_INVALID, "no feature buffer: pass at least one of albedo, normal, depth, hits"); }
    SELECT_DEVICE(scene);
    // one device buffer, the wanted images side by side; the sums continue from what the caller's arrays hold
    const size_t pixels = (size_t)scene->width * scene->height;
    float *host[4] = { albedo, normal, depth, hits };
    const size_t floats[4] = { 3 * pixels, 3 * pixels, pixels, pixels };
    size_t offset[4], total = 0;
    for (int i = 0; i < 4; i++) { offset[i] = total; if (host[i]) { total += floats[i]; } }
    DeviceBuffer<float> device;
    HIP_TRY(device.allocate(total));
    for (int i = 0; i < 4; i++) {
        if (host[i]) { HIP_TRY(hipMemcpy(device.ptr + offset[i], host[i], floats[i] * sizeof(float), hipMemcpyHostToDevice)); }
    }
    PathedFeatureBuffers buffers;
    buffers.albedo_sum = albedo ? device.ptr + offset[0] : nullptr;
    buffers.normal_sum = normal ? device.ptr + offset[1] : nullptr;
    buffers.depth_sum = depth ? device.ptr + offset[2] : nullptr;
    buffers.hit_count = hits ? device.ptr + offset[3] : nullptr;
    const int code = pathed_hip_render_features_device(scene, seed, spp_begin, spp_count, &buffers, nullptr);
    if (code != PATHED_OK) { return code; }
    for (int i = 0; i < 4; i++) {
        if (host[i]) { HIP_TRY(hipMemcpy(host[i], device.ptr + offset[i], floats[i] * sizeof(float), hipMemcpyDeviceToHost)); }
    }
    return PATHED_OK;
}

int pathed_hip_trace(PathedScene *scene, const float *rays, size_t n, int any_hit, void *hits)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (n == 0) { return PATHED_OK; }
    if (!rays || !hits) { return fail(PATHED_E_INVALID, "null ray or hit buffer"); }
    if (n > (size_t)1 << 28) { return fail(PATHED_E_INVALID, "too many rays in one call"); }
    SELECT_DEVICE(scene);

    DeviceBuffer<float4> deviceRays, deviceHits;
    DeviceBuffer<int> deviceOccluded, deviceOverflow;
    HIP_TRY(deviceRays.allocate(n * 2));
    HIP_TRY(hipMemcpy(deviceRays.ptr, rays, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    if (any_hit) { HIP_TRY(deviceOccluded.allocate(n)); } else { HIP_TRY(deviceHits.allocate(n)); }
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    const int code = withStackRows(scene->stackRows, [&](auto STACK) {
        HIP_TRY(deviceOverflow.allocate(stackSpillInts((size_t)grid.x * kBlock, scene->maxStack, STACK)));
        if (scene->instanced) {
            hipLaunchKernelGGL((k_trace_rays_instanced<STACK>), grid, block, stackLdsBytes(STACK), 0, scene->device, scene->instanceSet, deviceRays.ptr, (int)n, any_hit,
                               deviceHits.ptr, deviceOccluded.ptr, deviceOverflow.ptr, scene->maxStack);
            return (int)PATHED_OK;
        }
        // k_trace_rays<STACK, FORMAT>
        const auto run = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, block, stackLdsBytes(STACK), 0, scene->device, deviceRays.ptr, (int)n, any_hit, deviceHits.ptr, deviceOccluded.ptr,
                               deviceOverflow.ptr, scene->maxStack);
            return (int)PATHED_OK;
        };
#if PATHED_EXPERIMENTS
        if (scene->nodeFormat == 2) { return run(k_trace_rays<STACK, 2>); }
        if (scene->nodeFormat == 1) { return run(k_trace_rays<STACK, 1>); }
#endif
        return run(k_trace_rays<STACK, 0>);
    });
    if (code != PATHED_OK) { return code; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (any_hit) { HIP_TRY(hipMemcpy(hits, deviceOccluded.ptr, n * sizeof(int), hipMemcpyDeviceToHost)); }
    else { HIP_TRY(hipMemcpy(hits, deviceHits.ptr, n * sizeof(float4), hipMemcpyDeviceToHost)); }
    return PATHED_OK;
}

// pathed_hip_trace with one shutter time per ray (k_trace_rays_instanced_motion<STACK>): the test hook of the shutter
int pathed_hip_trace_timed(PathedScene *scene, const float *rays, const float *times, size_t n, int any_hit, void *hits)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (!scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "trace_timed: the scene has no instances (pathed_hip_scene_create_instanced makes one that has)"); }
    if (!scene->hasMotion) { return fail(PATHED_E_INVALID, "trace_timed: the scene has no motion (pathed_hip_scene_set_instance_motion sets one)"); }
    if (n == 0) { return PATHED_OK; }
    if (!rays || !times || !hits) { return fail(PATHED_E_INVALID, "null ray, time or hit buffer"); }
    if (n > (size_t)1 << 28) { return fail(PATHED_E_INVALID, "too many rays in one call"); }
    for (size_t i = 0; i < n; i++) {
        // (the moving boxes of the top tree cover the shutter and nothing beyond it)
        if (!(times[i] >= scene->motionSet.open && times[i] <= scene->motionSet.close)) {
            return fail(PATHED_E_INVALID, "trace_timed: ray " + std::to_string(i) + " has a time outside the scene's shutter");
        }
    }
    SELECT_DEVICE(scene);

    DeviceBuffer<float4> deviceRays, deviceHits;
    DeviceBuffer<float> deviceTimes;
    DeviceBuffer<int> deviceOccluded, deviceOverflow;
    HIP_TRY(deviceRays.allocate(n * 2));
    HIP_TRY(deviceTimes.allocate(n));
    HIP_TRY(hipMemcpy(deviceRays.ptr, rays, n * 8 * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(deviceTimes.ptr, times, n * sizeof(float), hipMemcpyHostToDevice));
    if (any_hit) { HIP_TRY(deviceOccluded.allocate(n)); } else { HIP_TRY(deviceHits.allocate(n)); }
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    const int code = withStackRows(scene->stackRows, [&](auto STACK) {
        HIP_TRY(deviceOverflow.allocate(stackSpillInts((size_t)grid.x * kBlock, scene->maxStack, STACK)));
        hipLaunchKernelGGL((k_trace_rays_instanced_motion<STACK>), grid, block, stackLdsBytes(STACK), 0, scene->device, scene->instanceSet, scene->motionSet,
                           deviceRays.ptr, deviceTimes.ptr, (int)n, any_hit, deviceHits.ptr, deviceOccluded.ptr, deviceOverflow.ptr, scene->maxStack);
        return (int)PATHED_OK;
    });
    if (code != PATHED_OK) { return code; }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    if (any_hit) { HIP_TRY(hipMemcpy(hits, deviceOccluded.ptr, n * sizeof(int), hipMemcpyDeviceToHost)); }
    else { HIP_TRY(hipMemcpy(hits, deviceHits.ptr, n * sizeof(float4), hipMemcpyDeviceToHost)); }
    return PATHED_OK;
}

int pathed_hip_scene_set_grid_medium(PathedScene *scene, int medium_index, const PathedGridMedium *grid)
{
    if (!scene || !grid) { return fail(PATHED_E_INVALID, "null scene or grid"); }
    if (grid->struct_size != sizeof(PathedGridMedium)) { return fail(PATHED_E_INVALID, "PathedGridMedium.struct_size does not match this library"); }
    if (scene->mediaHost.empty()) { return fail(PATHED_E_INVALID, "the scene has no media: a grid is set on a medium slot of the scene description"); }
    if (medium_index < 0 || (size_t)medium_index >= scene->mediaHost.size()) { return fail(PATHED_E_INVALID, "grid medium: medium index out of range"); }
    if (grid->cells_x < 2 || grid->cells_y < 2 || grid->cells_z < 2) { return fail(PATHED_E_INVALID, "grid medium: a grid needs at least 2 cells on every axis"); }
    const unsigned long long cellCount = (unsigned long long)grid->cells_x * grid->cells_y * grid->cells_z;
    if (grid->cells_x >= (1u << 20) || grid->cells_y >= (1u << 20) || grid->cells_z >= (1u << 20) || cellCount >= (1ull << 31)) {
        return fail(PATHED_E_INVALID, "grid medium: too many cells (the product must stay below 2^31)");
    }
    if (!grid->data) { return fail(PATHED_E_INVALID, "grid medium: data missing"); }
    for (int k = 0; k < 6; k++) {
        if (!std::isfinite(grid->bounds[k])) { return fail(PATHED_E_INVALID, "grid medium: bounds must be finite"); }
    }
    for (int k = 0; k < 3; k++) {
        if (!(grid->bounds[k + 3] > grid->bounds[k])) { return fail(PATHED_E_INVALID, "grid medium: bounds must be (min x, y, z, max x, y, z) with max > min"); }
    }
    if (!std::isfinite(grid->albedo) || !std::isfinite(grid->scale)) { return fail(PATHED_E_INVALID, "grid medium: albedo and scale must be finite"); }
    for (int k = 0; k < 16; k++) {
        if (!std::isfinite(grid->world_to_model[k]) || !std::isfinite(grid->model_to_world[k])) { return fail(PATHED_E_INVALID, "grid medium: the transform must be finite"); }
    }
    for (unsigned long long i = 0; i < cellCount; i++) {
        if (!std::isfinite(grid->data[i])) { return fail(PATHED_E_INVALID, "grid medium: data must be finite"); }
    }
    SELECT_DEVICE(scene);

    DGrid record;
    std::memset(&record, 0, sizeof record);
    record.cellsX = (int)grid->cells_x; record.cellsY = (int)grid->cells_y; record.cellsZ = (int)grid->cells_z;
    record.minX = grid->bounds[0]; record.minY = grid->bounds[1]; record.minZ = grid->bounds[2];
    record.maxX = grid->bounds[3]; record.maxY = grid->bounds[4]; record.maxZ = grid->bounds[5];
    record.widthX = record.maxX - record.minX;   // GridInfo::widthX, include/uniform_grid.h:22-24
    record.widthY = record.maxY - record.minY;
    record.widthZ = record.maxZ - record.minZ;
    record.albedo = grid->albedo;
    record.scale = grid->scale;
    std::memcpy(record.worldToModel, grid->world_to_model, sizeof record.worldToModel);
    std::memcpy(record.modelToWorld, grid->model_to_world, sizeof record.modelToWorld);

    // the new tables, built beside the old ones: a failure leaves the scene as it was
    std::vector<DMedium> media = scene->mediaHost;
    std::vector<DGrid> records = scene->gridsHost;
    std::vector<std::vector<float>> cells = scene->gridCells;
    int slot;
    if (media[(size_t)medium_index].kind == kMediumGrid) {
        slot = media[(size_t)medium_index].grid;   // replace
    } else {
        slot = (int)records.size();
        records.push_back(record);
        cells.emplace_back();
        media[(size_t)medium_index].kind = kMediumGrid;
        media[(size_t)medium_index].grid = slot;
    }
    records[(size_t)slot] = record;
    cells[(size_t)slot].assign(grid->data, grid->data + cellCount);
    std::vector<float> all;
    for (size_t g = 0; g < records.size(); g++) {
        if (all.size() + cells[g].size() >= ((size_t)1 << 32)) { return fail(PATHED_E_INVALID, "grid medium: the scene's grids hold more than 2^32 cells"); }
        records[g].dataOffset = (unsigned int)all.size();
        all.insert(all.end(), cells[g].begin(), cells[g].end());
    }
    HIP_TRY(hipDeviceSynchronize());   // nothing of this scene runs (render calls return when they have completed); other streams of the caller may
    HIP_TRY(scene->grids.upload(records));
    HIP_TRY(scene->gridData.upload(all));
    HIP_TRY(hipMemcpy(scene->media.ptr, media.data(), media.size() * sizeof(DMedium), hipMemcpyHostToDevice));
    scene->mediaHost.swap(media);
    scene->gridsHost.swap(records);
    scene->gridCells.swap(cells);
    scene->device.grids = scene->grids.ptr;
    scene->device.gridData = scene->gridData.ptr;
    return PATHED_OK;
}

int pathed_hip_scene_set_medium_phase(PathedScene *scene, int medium_index, const PathedPhaseFunction *phase)
{
    if (!scene || !phase) { return fail(PATHED_E_INVALID, "null scene or phase function"); }
    if (phase->struct_size != sizeof(PathedPhaseFunction)) { return fail(PATHED_E_INVALID, "PathedPhaseFunction.struct_size does not match this library"); }
    if (medium_index < 0 || (size_t)medium_index >= scene->mediaHost.size()) { return fail(PATHED_E_INVALID, "medium phase: medium index out of range"); }
    if (phase->type != PATHED_PHASE_ISOTROPIC && phase->type != PATHED_PHASE_HENYEY_GREENSTEIN) { return fail(PATHED_E_INVALID, "medium phase: unknown phase function type"); }
    if (!std::isfinite(phase->g) || std::fabs(phase->g) > 0.99f) { return fail(PATHED_E_INVALID, "medium phase: g must be finite with |g| <= 0.99"); }
    SELECT_DEVICE(scene);

    // the new tables, built beside the old ones: a failure leaves the scene as it was
    const size_t slots = scene->mediaHost.size();
    std::vector<int> types = scene->phaseTypeHost;
    std::vector<float> gs = scene->phaseGHost;
    types.resize(slots, PATHED_PHASE_ISOTROPIC);
    gs.resize(slots, 0.f);
    types[(size_t)medium_index] = phase->type;
    gs[(size_t)medium_index] = phase->g;
    std::vector<float> table(slots, 0.f);
    bool anisotropic = false;
    for (size_t i = 0; i < slots; i++) {
        if (types[i] != PATHED_PHASE_HENYEY_GREENSTEIN) { continue; }
        table[i] = gs[i];
        anisotropic = anisotropic || !(std::fabs(gs[i]) < kPhaseIsotropicBelow);
    }
    HIP_TRY(hipDeviceSynchronize());   // nothing of this scene runs (as in pathed_hip_scene_set_grid_medium)
    DeviceBuffer<float> device;
    HIP_TRY(device.upload(table));
    std::swap(scene->phaseG.ptr, device.ptr);
    std::swap(scene->phaseG.count, device.count);
    scene->phaseTypeHost.swap(types);
    scene->phaseGHost.swap(gs);
    scene->anisotropic = anisotropic;
    return PATHED_OK;
}

int pathed_hip_grid_queries(PathedScene *scene, int medium_index, size_t n, const float *a, const float *b, const float *target,
                            float *transmittance, float *distance)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (medium_index < 0 || (size_t)medium_index >= scene->mediaHost.size() || scene->mediaHost[(size_t)medium_index].kind != kMediumGrid) {
        return fail(PATHED_E_INVALID, "grid queries: the medium slot holds no grid");
    }
    if (n == 0) { return PATHED_OK; }
    if (!a || !b || !target || !transmittance || !distance) { return fail(PATHED_E_INVALID, "null segment or result buffer"); }
    if (n > (size_t)1 << 24) { return fail(PATHED_E_INVALID, "too many segments in one call"); }
    return recordHook<float>(scene, n, { { a, 3 * n }, { b, 3 * n }, { target, n } }, { { transmittance, n }, { distance, n } }, [&](dim3 grid, auto &in, auto &out) {
        hipLaunchKernelGGL(k_grid_queries, grid, dim3(kBlock), 0, nullptr, scene->grids.ptr, scene->gridData.ptr, scene->mediaHost[(size_t)medium_index].grid,
                           (int)n, in[0].ptr, in[1].ptr, in[2].ptr, out[0].ptr, out[1].ptr);
    });
}

int pathed_hip_debug_phase_samples(PathedScene *scene, size_t n, const float *u, float *out)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (n == 0) { return PATHED_OK; }
    if (!u || !out) { return fail(PATHED_E_INVALID, "null record or result buffer"); }
    if (n > (size_t)1 << 20) { return fail(PATHED_E_INVALID, "too many records in one call"); }
    for (size_t i = 0; i < 2 * n; i++) {
        if (!(u[i] >= 0.f && u[i] <= 1.f)) { return fail(PATHED_E_INVALID, "phase samples: random numbers lie in [0, 1]"); }
    }
    return recordHook<float>(scene, n, { { u, 2 * n } }, { { out, 3 * n } }, [&](dim3 grid, auto &in, auto &result) {
        hipLaunchKernelGGL(k_debug_phase_samples, grid, dim3(kBlock), 0, nullptr, (int)n, in[0].ptr, result[0].ptr);
    });
}

int pathed_hip_debug_phase_hg(PathedScene *scene, size_t n, const float *records, float *out)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (n == 0) { return PATHED_OK; }
    if (!records || !out) { return fail(PATHED_E_INVALID, "null record or result buffer"); }
    if (n > (size_t)1 << 20) { return fail(PATHED_E_INVALID, "too many records in one call"); }
    for (size_t i = 0; i < n; i++) {
        const float *record = records + 9 * i;
        if (!std::isfinite(record[0]) || std::fabs(record[0]) > 0.99f) { return fail(PATHED_E_INVALID, "phase records: g must be finite with |g| <= 0.99"); }
        if (!(record[4] >= 0.f && record[4] <= 1.f) || !(record[5] >= 0.f && record[5] <= 1.f)) { return fail(PATHED_E_INVALID, "phase records: random numbers lie in [0, 1]"); }
        for (int k = 1; k < 9; k++) {
            if (!std::isfinite(record[k])) { return fail(PATHED_E_INVALID, "phase records: directions must be finite"); }
        }
    }
    return recordHook<float>(scene, n, { { records, 9 * n } }, { { out, 4 * n } }, [&](dim3 grid, auto &in, auto &result) {
        hipLaunchKernelGGL(k_debug_phase_hg, grid, dim3(kBlock), 0, nullptr, (int)n, in[0].ptr, result[0].ptr);
    });
}

// what pathed_hip_debug_shading_queries needs to know of one SceneTraits set, and its instantiation of the kernel
struct ShadingQuerySet {
    unsigned materials;
    bool beckmann, ggx, env, spheres, varyingAlbedo;
    void (*kernel)(DEnv, const DMaterial *, int, int, int, int, const float *, float *);
};
#define SHADING_QUERY_SET(TRAITS) { TRAITS::materials, TRAITS::beckmann, TRAITS::ggx, TRAITS::env, TRAITS::spheres, TRAITS::varyingAlbedo, k_shading_queries<TRAITS> }

int pathed_hip_debug_shading_queries(PathedScene *scene, int function, int traits, size_t n, const float *in, float *out)
{
    // the sets of the launch ladders, in the order of PATHED_TRAITS_* (include/pathed_hip.h)
    static const ShadingQuerySet sets[PATHED_TRAITS_COUNT] = {
        SHADING_QUERY_SET(TraitsAll), SHADING_QUERY_SET(TraitsLambertianTriangles), SHADING_QUERY_SET(TraitsLambertianPlasticSpheres),
        SHADING_QUERY_SET(TraitsLambertianGlassContainer), SHADING_QUERY_SET(TraitsTriangleLit), SHADING_QUERY_SET(TraitsEnvironmentOnly),
        SHADING_QUERY_SET(TraitsRoughBeckmann), SHADING_QUERY_SET(TraitsRoughGgx), SHADING_QUERY_SET(TraitsSmooth),
    };
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (function < 0 || function >= kQueryCount) { return fail(PATHED_E_INVALID, "shading queries: unknown function"); }
    if (traits < 0 || traits >= PATHED_TRAITS_COUNT) { return fail(PATHED_E_INVALID, "shading queries: unknown traits set"); }
    const ShadingQuerySet &set = sets[traits];
    const bool material = function == kQueryMaterialF || function == kQueryMaterialSample;
    const bool sphere = function == kQuerySphereSample || function == kQuerySpherePdf;
    const bool env = function == kQueryEnvEmit || function == kQueryEnvPdf || function == kQueryEnvSample;
    if (sphere && !set.spheres) { return fail(PATHED_E_INVALID, "shading queries: the traits set holds no spheres"); }
    if (env && !set.env) { return fail(PATHED_E_INVALID, "shading queries: the traits set holds no environment"); }
    if (env && !scene->device.hasEnv) { return fail(PATHED_E_INVALID, "shading queries: the scene has no environment"); }
    if (n == 0) { return PATHED_OK; }
    if (!in || !out) { return fail(PATHED_E_INVALID, "null record or result buffer"); }
    if (n > (size_t)1 << 20) { return fail(PATHED_E_INVALID, "too many records in one call"); }
    const int inputs = kQueryInputs[function], outputs = kQueryOutputs[function];
    auto unit = [](float u) { return u >= 0.f && u <= 1.f; };
    std::vector<DMaterial> materials;
    for (size_t i = 0; i < n; i++) {
        const float *p = in + (size_t)inputs * i;
        if (material) {
            PathedMaterial m;
            std::memset(&m, 0, sizeof m);
            if (!(p[0] >= 0.f && p[0] <= 5.f) || p[0] != (float)(int)p[0]) { return fail(PATHED_E_INVALID, "shading queries: material type"); }
            m.type = (int)p[0];
            if (((set.materials >> m.type) & 1u) == 0u) { return fail(PATHED_E_INVALID, "shading queries: the traits set does not hold the material type"); }
            if (p[1] != (float)PATHED_ALBEDO_CONSTANT && p[1] != (float)PATHED_ALBEDO_CHECKERBOARD) { return fail(PATHED_E_INVALID, "shading queries: constant or checkerboard albedo"); }
            m.albedo_type = (int)p[1];
            if (m.albedo_type != PATHED_ALBEDO_CONSTANT && !set.varyingAlbedo) { return fail(PATHED_E_INVALID, "shading queries: the traits set holds constant albedo only"); }
            if (p[19] != (float)PATHED_DIST_BECKMANN && p[19] != (float)PATHED_DIST_GGX) { return fail(PATHED_E_INVALID, "shading queries: distribution"); }
            m.distribution = (int)p[19];
            if (m.type == PATHED_MAT_MICROFACET || m.type == PATHED_MAT_PLASTIC) {
                if (m.distribution == PATHED_DIST_GGX ? !set.ggx : !set.beckmann) { return fail(PATHED_E_INVALID, "shading queries: the traits set does not hold the distribution"); }
            }
            for (int k = 0; k < 3; k++) {
                m.diffuse[k] = p[2 + k]; m.emit[k] = p[5 + k]; m.checker_on[k] = p[8 + k]; m.checker_off[k] = p[11 + k];
            }
            m.checker_res[0] = p[14]; m.checker_res[1] = p[15];
            m.sigma = p[16]; m.alpha = p[17]; m.ior = p[18];
            materials.push_back(buildMaterial(m));
            if (function == kQueryMaterialSample && !(unit(p[31]) && unit(p[32]) && unit(p[33]))) { return fail(PATHED_E_INVALID, "shading queries: random numbers lie in [0, 1]"); }
        }
        if (function == kQuerySphereSample && !(unit(p[7]) && unit(p[8]))) { return fail(PATHED_E_INVALID, "shading queries: random numbers lie in [0, 1]"); }
        if (function == kQueryEnvSample && !(unit(p[3]) && unit(p[4]))) { return fail(PATHED_E_INVALID, "shading queries: random numbers lie in [0, 1]"); }
        if (function == kQueryEnvEmit || function == kQueryEnvPdf) {
            // the texel index comes from the direction's angles: not-a-number angles index outside the image
            const float length2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
            if (!std::isfinite(length2) || !(length2 > 1e-30f)) { return fail(PATHED_E_INVALID, "shading queries: a direction must be finite and not zero"); }
        }
    }
    SELECT_DEVICE(scene);
    DeviceBuffer<DMaterial> deviceMaterials;
    if (material) { HIP_TRY(deviceMaterials.upload(materials)); }
    return recordHook<float>(scene, n, { { in, (size_t)inputs * n } }, { { out, (size_t)outputs * n } }, [&](dim3 grid, auto &records, auto &result) {
        hipLaunchKernelGGL(set.kernel, grid, dim3(kBlock), 0, nullptr, scene->device.env, deviceMaterials.ptr, function, (int)n, inputs, outputs,
                           records[0].ptr, result[0].ptr);
    });
}

int pathed_hip_has_experiments(void) { return PATHED_EXPERIMENTS ? 1 : 0; }

int pathed_hip_debug_small_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector's hook does not serve scenes with instances"); }
    if (!scene->bruteForce || scene->device.nTris < 1) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector serves scenes of 1..64 triangles"); }
    if (n == 0) { return PATHED_OK; }
    if (!rays || !out) { return fail(PATHED_E_INVALID, "null ray or output buffer"); }
    if (n > (size_t)1 << 24) { return fail(PATHED_E_INVALID, "too many rays in one call"); }
    SELECT_DEVICE(scene);
    // the matrix-pipe rows over the LEAF order (the render's own table, if any, follows the item order)
    DeviceBuffer<float> table;
    MfmaFrame frame;
    std::memset(&frame, 0, sizeof frame);
#if PATHED_EXPERIMENTS
    {
        std::vector<float> rows;
        buildMfmaTable(scene->bvh.leafTris.data(), scene->device.nTris, scene->device.camera.origin, 1, &rows, &frame);
        HIP_TRY(table.upload(rows));
    }
#endif
    const std::vector<float> hostRays = paddedRays(rays, n);
    return recordHook<unsigned long long>(scene, n, { { hostRays.data(), hostRays.size() } }, { { (unsigned long long *)out, n * 8 } }, [&](dim3 grid, auto &in, auto &result) {
        hipLaunchKernelGGL(k_debug_small_candidates, grid, dim3(kBlock), 0, nullptr, scene->device, scene->smallTris, scene->smallItems, scene->smallLayout.nQuads,
                           scene->smallLayout.kappaT, scene->itemTris.ptr, table.ptr, frame, in[0].ptr, (int)n, result[0].ptr);
    });
}

int pathed_hip_debug_shadow_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out, int32_t *layout, uint64_t *never_occluders)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector's hook does not serve scenes with instances"); }
    if (!scene->bruteForce || scene->device.nTris < 1) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector serves scenes of 1..64 triangles"); }
    if (!layout || !never_occluders) { return fail(PATHED_E_INVALID, "null layout or never-occluder buffer"); }
    fillLayout(layout, scene->smallLayout);
    *never_occluders = scene->smallLayout.neverOccluders;
    if (n == 0) { return PATHED_OK; }
    if (!rays || !out) { return fail(PATHED_E_INVALID, "null ray or output buffer"); }
    if (n > (size_t)1 << 24) { return fail(PATHED_E_INVALID, "too many rays in one call"); }
    const std::vector<float> hostRays = paddedRays(rays, n);
    return recordHook<unsigned long long>(scene, n, { { hostRays.data(), hostRays.size() } }, { { (unsigned long long *)out, n * 2 } }, [&](dim3 grid, auto &in, auto &result) {
        hipLaunchKernelGGL(k_debug_shadow_candidates, grid, dim3(kBlock), 0, nullptr, scene->device, scene->smallItems, scene->smallLayout.nQuads, scene->smallLayout.kappaT,
                           scene->smallLayout.shadowQuadPairs, scene->smallLayout.shadowLonePairs, scene->itemTris.ptr, in[0].ptr, (int)n, result[0].ptr);
    });
}

int pathed_hip_debug_pass_candidates(PathedScene *scene, const float *rays, size_t n, uint64_t *out, int32_t *primitives, size_t n_triangles,
                                     int32_t *layout, uint64_t *never_hit)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector's hook does not serve scenes with instances"); }
    if (!scene->bruteForce || scene->device.nTris < 1) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector serves scenes of 1..64 triangles"); }
    if (!layout || !never_hit || !primitives) { return fail(PATHED_E_INVALID, "null layout, primitive or never-hit buffer"); }
    const int nPass = scene->passTris;
    if (n_triangles != (size_t)scene->device.nTris || nPass < 1 || nPass > scene->device.nTris || scene->passTrisHost.size() < (size_t)12 * nPass) {
        return fail(PATHED_E_INVALID, "n_triangles must be the scene's triangle count");
    }
    fillLayout(layout, scene->passLayout);
    layout[4] = nPass;
    *never_hit = scene->passNeverHit;
    for (size_t k = 0; k < n_triangles; k++) {
        primitives[k] = -1;   // (beyond the pass list)
        if (k < (size_t)nPass) { std::memcpy(&primitives[k], &scene->passTrisHost[12 * k + 3], sizeof(int32_t)); }
    }
    if (n == 0) { return PATHED_OK; }
    if (!rays || !out) { return fail(PATHED_E_INVALID, "null ray or output buffer"); }
    if (n > (size_t)1 << 24) { return fail(PATHED_E_INVALID, "too many rays in one call"); }
    const std::vector<float> hostRays = paddedRays(rays, n);
    return recordHook<unsigned long long>(scene, n, { { hostRays.data(), hostRays.size() } }, { { (unsigned long long *)out, n * 2 } }, [&](dim3 grid, auto &in, auto &result) {
        hipLaunchKernelGGL(k_debug_pass_candidates, grid, dim3(kBlock), 0, nullptr, scene->passItems, scene->passLayout.nQuads, nPass, scene->passLayout.kappaT,
                           scene->passLayout.shadowQuadPairs, scene->passLayout.shadowLonePairs, scene->itemTris.ptr + (size_t)3 * scene->device.nTris, in[0].ptr, (int)n,
                           result[0].ptr);
    });
}

int pathed_hip_debug_camera_masks(PathedScene *scene, uint64_t *out, size_t n_pixels)
{
    if (!scene || !out) { return fail(PATHED_E_INVALID, "null scene or output buffer"); }
    if (!scene->bruteForce || !scene->fusedPath) { return fail(PATHED_E_UNSUPPORTED, "only scenes on the fused path kernel carry camera-ray candidate masks"); }
    if (n_pixels != (size_t)scene->width * (size_t)scene->height) { return fail(PATHED_E_INVALID, "n_pixels must be the scene's pixel count"); }
    SELECT_DEVICE(scene);
    if (!scene->cameraMasksBuilt) { HIP_TRY(rebuildCameraMasks(scene)); }
    HIP_TRY(hipMemcpy(out, scene->cameraQueue.ptr, n_pixels * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return PATHED_OK;
}

int pathed_hip_debug_item_order(PathedScene *scene, int32_t *primitives, size_t n_triangles)
{
    if (!scene || !primitives) { return fail(PATHED_E_INVALID, "null scene or output buffer"); }
    if (!scene->bruteForce) { return fail(PATHED_E_UNSUPPORTED, "the all-triangles intersector serves scenes of 1..64 triangles"); }
    if (n_triangles != (size_t)scene->device.nTris || scene->itemTrisHost.size() < 12 * n_triangles) { return fail(PATHED_E_INVALID, "n_triangles must be the scene's triangle count"); }
    for (size_t k = 0; k < n_triangles; k++) { std::memcpy(&primitives[k], &scene->itemTrisHost[12 * k + 3], sizeof(int32_t)); }
    return PATHED_OK;
}

int pathed_hip_debug_light_records(PathedScene *scene, float *triangles, size_t n_triangles, float *lights, size_t max_lights, int *n_lights)
{
    if (!scene || !triangles || !lights || !n_lights) { return fail(PATHED_E_INVALID, "null scene or output buffer"); }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "the light-record hook assumes a flat scene: it does not serve scenes with instances"); }
    SELECT_DEVICE(scene);
    const size_t nTris = (size_t)scene->device.nTris, nLights = (size_t)scene->device.nLights;
    if (n_triangles != nTris) { return fail(PATHED_E_INVALID, "n_triangles must be the scene's triangle count"); }
    if (max_lights < nLights) { return fail(PATHED_E_INVALID, "the scene has more lights than the buffer holds"); }
    *n_lights = (int)nLights;
    if (nTris > 0) {
        DeviceBuffer<float4> perVertex;
        HIP_TRY(perVertex.allocate(3 * nTris));
        hipLaunchKernelGGL(k_debug_per_vertex_constants, dim3((unsigned)((nTris + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                           scene->triShade.ptr, (int)nTris, (int)nLights, perVertex.ptr);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipDeviceSynchronize());
        std::vector<float4> constants(3 * nTris), shade((size_t)kTriShadeQuads * nTris), compact((size_t)kTriCompactQuads * nTris);
        HIP_TRY(hipMemcpy(constants.data(), perVertex.ptr, constants.size() * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(shade.data(), scene->triShade.ptr, shade.size() * sizeof(float4), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(compact.data(), scene->triCompact.ptr, compact.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nTris; i++) {
            float4 *row = reinterpret_cast<float4 *>(triangles) + 5 * i;
            row[0] = constants[3 * i]; row[1] = constants[3 * i + 1]; row[2] = constants[3 * i + 2];
            row[3] = shade[(size_t)kTriShadeQuads * i + 7];
            row[4] = compact[(size_t)kTriCompactQuads * i + 1];
        }
    }
    if (nLights > 0) {
        std::vector<DLight> kinds(nLights);
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(kinds.data(), scene->lights.ptr, nLights * sizeof(DLight), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nLights; i++) { lights[18 * i] = (float)kinds[i].kind; lights[18 * i + 1] = (float)kinds[i].index; }
        std::vector<float4> records((size_t)kLightRecordQuads * nLights);
        HIP_TRY(hipMemcpy(records.data(), scene->lightRecords.ptr, records.size() * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nLights; i++) { std::memcpy(lights + 18 * i + 2, &records[(size_t)kLightRecordQuads * i], 16 * sizeof(float)); }
    }
    return PATHED_OK;
}

int pathed_hip_scene_refit(PathedScene *scene, const float *positions, const float *normals, uint32_t n_vertices, float *device_ms)
{
    if (!scene || !positions) { return fail(PATHED_E_INVALID, "null scene or positions"); }
    if (scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "refit: a scene with instances cannot be refitted"); }
    if (!scene->refittable) { return fail(PATHED_E_INVALID, "create the scene with PathedSceneOptions.refittable = 1: the refit needs the triangle soup on the device"); }
    if ((size_t)n_vertices != scene->soupVertices) { return fail(PATHED_E_INVALID, "refit keeps the topology: the vertex count must be the scene's"); }
    if (scene->bruteForce) { return fail(PATHED_E_UNSUPPORTED, "scenes of at most 64 triangles carry no tree to refit: create the scene again (microseconds)"); }
    if (scene->nodeFormat != 0) { return fail(PATHED_E_UNSUPPORTED, "refit serves the 128-byte float nodes"); }
    SELECT_DEVICE(scene);
    const int nNodes = scene->device.nNodes;
    const size_t nTris = (size_t)scene->device.nTris;
    if (nNodes <= 0 || nTris == 0) { return fail(PATHED_E_INVALID, "the scene has no tree"); }
    if (!scene->refitLo.ptr) {
        HIP_TRY(scene->refitLo.allocate((size_t)nNodes));
        HIP_TRY(scene->refitHi.allocate((size_t)nNodes));
        HIP_TRY(scene->refitReady.allocate(2 * (size_t)nNodes));
    }
    HIP_TRY(hipMemcpy(scene->soupPositions.ptr, positions, 3 * (size_t)n_vertices * sizeof(float), hipMemcpyHostToDevice));
    if (normals) { HIP_TRY(hipMemcpy(scene->soupNormals.ptr, normals, 3 * (size_t)n_vertices * sizeof(float), hipMemcpyHostToDevice)); }
    EventTimer timer;
    const dim3 grid((unsigned)((nNodes + kBlock - 1) / kBlock)), block(kBlock);
    LevelPasses passes{ scene->refitReady.ptr, (size_t)nNodes, [&](const unsigned char *in, unsigned char *out) {
        hipLaunchKernelGGL(k_refit_pass, grid, block, 0, nullptr, scene->nodes.ptr, nNodes, scene->leafTris.ptr, scene->soupPositions.ptr,
                           scene->soupIndices.ptr, scene->spheres.ptr, scene->refitLo.ptr, scene->refitHi.ptr, in, out);
    } };
    timer.run([&]() {
        // shading records (corners, normals, uvs) of every primitive, then the tree bottom-up
        hipLaunchKernelGGL(k_build_tri_shade, dim3((unsigned)((8 * nTris + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                           scene->soupPositions.ptr, scene->soupNormals.ptr, scene->soupUvs.ptr, scene->soupIndices.ptr, scene->soupTriMaterial.ptr,
                           (uint32_t)nTris, scene->triShade.ptr, scene->triCompact.ptr);
        if (!timer.keep(buildLightRecords(scene, scene->device.nLights))) { return; }   // an emitter that moved is sampled where it is now
        if (!timer.keep(hipMemsetAsync(scene->refitReady.ptr, 0, 2 * (size_t)nNodes, nullptr))) { return; }
        passes.launchLevels(scene->bvh.maxDepth);
    });
    const bool rootReady = passes.reachRoot(timer);
    if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string("refit: ") + hipGetErrorString(timer.status)); }
    if (!rootReady) { return fail(PATHED_E_DEVICE, "refit: the root was never reached (a cycle in the tree?)"); }
    scene->bvhOnHost = false;   // exports download the refitted tree
    if (device_ms) { *device_ms = timer.ms; }
    return PATHED_OK;
}

// The refit of the top tree over the placements' boxes as they stand: the records and the prototype boxes, or, while a
// shutter is set, what stands in for them (k_motion_boxes).  topLo / topHi / topReady are allocated by the caller.
// `motion`: the buffers of the shutter to refit over, or null for the static boxes.
static int refitTopTree(PathedScene *scene, const PathedScene::MotionBuffers *motion, EventTimer &timer, const char *what)
{
    const int nInstances = scene->instanceSet.nInstances, topNodes = scene->topNodes;
    const float4 *records = motion ? motion->boxRecords.ptr : scene->instanceRecords.ptr;
    const float4 *boxTable = motion ? motion->boxTable.ptr : scene->protoBoxes.ptr;
    const int nBoxes = (int)((motion ? motion->boxTable.count : scene->protoBoxes.count) / 2);
    timer.keep(hipMemset(scene->topReady.ptr, 0, 2 * (size_t)topNodes));
    const dim3 grid((unsigned)((topNodes + kBlock - 1) / kBlock)), block(kBlock);
    LevelPasses passes{ scene->topReady.ptr, (size_t)topNodes, [&](const unsigned char *in, unsigned char *out) {
        hipLaunchKernelGGL(k_refit_top_pass, grid, block, 0, nullptr, scene->nodes.ptr, topNodes, records, nInstances,
                           boxTable, nBoxes, scene->topLo.ptr, scene->topHi.ptr, in, out);
    } };
    timer.run([&]() { passes.launchLevels(scene->topDepth); });
    const bool rootReady = passes.reachRoot(timer);
    if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string(what) + ": " + hipGetErrorString(timer.status)); }
    if (!rootReady) { return fail(PATHED_E_DEVICE, std::string(what) + ": the top tree's root was never reached (a cycle in the tree?)"); }
    scene->bvhOnHost = false;   // exports download the refitted tree
    return PATHED_OK;
}

// ---- moving placements (include/pathed_hip.h; instance_kernels.h: k_instance_records, k_refit_top_pass)
// The one compute path of both entry points: `deviceTransforms` holds 12 floats per placement on the scene's device.
static int setInstanceTransforms(PathedScene *scene, const float *deviceTransforms, float *device_ms)
{
    const int nInstances = scene->instanceSet.nInstances;
    const int topNodes = scene->topNodes;
    if (topNodes <= 0 || (size_t)topNodes > scene->nodes.count / 8) { return fail(PATHED_E_INVALID, "the scene has no top tree"); }
    // everything a first call allocates, before anything is written: a failure here leaves the scene as it was
    if (scene->instanceRecordsStaged.count != scene->instanceRecords.count) { HIP_TRY(scene->instanceRecordsStaged.allocate(scene->instanceRecords.count)); }
    if (!scene->instanceBad.ptr) { HIP_TRY(scene->instanceBad.allocate(2)); }
    if (!scene->topLo.ptr) {
        HIP_TRY(scene->topLo.allocate((size_t)topNodes));
        HIP_TRY(scene->topHi.allocate((size_t)topNodes));
        HIP_TRY(scene->topReady.allocate(2 * (size_t)topNodes));
    }
    // render calls on a caller's stream may still walk the tree, and the caller's own stream may still write the transforms
    HIP_TRY(hipDeviceSynchronize());
    const unsigned int clear[2] = { 0u, 0xFFFFFFFFu };
    unsigned int bad[2] = { 0u, 0u };
    HIP_TRY(hipMemcpy(scene->instanceBad.ptr, clear, sizeof clear, hipMemcpyHostToDevice));
    EventTimer timer;
    if (nInstances > 0) {
        timer.run([&]() {
            hipLaunchKernelGGL(k_instance_records, dim3((unsigned)((nInstances + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                               deviceTransforms, nInstances, scene->instanceRecords.ptr, scene->instanceRecordsStaged.ptr, scene->instanceBad.ptr);
        });
        if (timer.ok()) { timer.keep(hipMemcpy(bad, scene->instanceBad.ptr, sizeof bad, hipMemcpyDeviceToHost)); }
        if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string("set_instance_transforms: ") + hipGetErrorString(timer.status)); }
        if (bad[0] != 0u) {
            // (the staged records are simply not adopted: the live records, the tree and the flags are untouched)
            return fail(PATHED_E_INVALID, "instance transform " + std::to_string(bad[1]) + " is not finite or not invertible (" + std::to_string(bad[0])
                        + " of the " + std::to_string(nInstances) + " transforms are refused; the scene keeps its placements)");
        }
        scene->instanceRecords.swap(scene->instanceRecordsStaged);
        scene->instanceSet.records = scene->instanceRecords.ptr;
    }
    const int code = refitTopTree(scene, nullptr, timer, "set_instance_transforms");
    if (code != PATHED_OK) { return code; }
    scene->hasMotion = false;   // new time-0 transforms end a shutter: the caller sets the motion of the next frame
    if (device_ms) { *device_ms = timer.ms; }
    return PATHED_OK;
}

static int checkInstanceMove(PathedScene *scene, const float *transforms, uint32_t n_instances)
{
    if (!scene || !transforms) { return fail(PATHED_E_INVALID, "null scene or transforms"); }
    if (!scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "set_instance_transforms: the scene has no instances (pathed_hip_scene_create_instanced makes one that has)"); }
    if (n_instances != (uint32_t)scene->instanceSet.nInstances) { return fail(PATHED_E_INVALID, "set_instance_transforms keeps the placements: the instance count must be the scene's"); }
    return PATHED_OK;
}

int pathed_hip_scene_set_instance_transforms_device(PathedScene *scene, const float *d_transforms, uint32_t n_instances, float *device_ms)
{
    const int code = checkInstanceMove(scene, d_transforms, n_instances);
    if (code != PATHED_OK) { return code; }
    SELECT_DEVICE(scene);
    return setInstanceTransforms(scene, d_transforms, device_ms);
}

int pathed_hip_scene_set_instance_transforms(PathedScene *scene, const float *transforms, uint32_t n_instances, float *device_ms)
{
    const int code = checkInstanceMove(scene, transforms, n_instances);
    if (code != PATHED_OK) { return code; }
    SELECT_DEVICE(scene);
    const size_t floats = (size_t)12 * n_instances;
    if (scene->instanceTransforms.count != floats) { HIP_TRY(scene->instanceTransforms.allocate(floats)); }
    if (floats > 0) { HIP_TRY(hipMemcpy(scene->instanceTransforms.ptr, transforms, floats * sizeof(float), hipMemcpyHostToDevice)); }
    return setInstanceTransforms(scene, scene->instanceTransforms.ptr, device_ms);
}

// ---- the shutter (include/pathed_hip.h; instance_motion.h: k_motion_boxes; instance_kernels.h: k_refit_top_pass)
// The one compute path of both entry points: `deviceClose` holds 12 floats per placement on the scene's device, or is null,
// which removes the motion.  Everything is refused before anything is launched, or written beside the live state and adopted
// when no transform is refused.
static int checkInstanceMotion(PathedScene *scene, uint32_t n_instances, bool clears, float shutter_open, float shutter_close)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (!scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "set_instance_motion: the scene has no instances (pathed_hip_scene_create_instanced makes one that has)"); }
    if (clears) { return PATHED_OK; }
    if (n_instances != (uint32_t)scene->instanceSet.nInstances) { return fail(PATHED_E_INVALID, "set_instance_motion keeps the placements: the instance count must be the scene's"); }
    if (!(0.f <= shutter_open && shutter_open <= shutter_close && shutter_close <= 1.f)) {
        return fail(PATHED_E_INVALID, "set_instance_motion: the shutter must satisfy 0 <= open <= close <= 1");
    }
    return PATHED_OK;
}

static int setInstanceMotion(PathedScene *scene, const float *deviceClose, float shutter_open, float shutter_close, float *device_ms)
{
    const int nInstances = scene->instanceSet.nInstances;
    const int topNodes = scene->topNodes, nPrototypes = (int)(scene->protoBoxes.count / 2);
    if (topNodes <= 0 || (size_t)topNodes > scene->nodes.count / 8) { return fail(PATHED_E_INVALID, "the scene has no top tree"); }
    if (device_ms) { *device_ms = 0.f; }
    if (!deviceClose && !scene->hasMotion) { return PATHED_OK; }   // nothing to remove
    if (!scene->topLo.ptr) {
        HIP_TRY(scene->topLo.allocate((size_t)topNodes));
        HIP_TRY(scene->topHi.allocate((size_t)topNodes));
        HIP_TRY(scene->topReady.allocate(2 * (size_t)topNodes));
    }
    PathedScene::MotionBuffers &staged = scene->motionStaged;
    if (deviceClose && staged.moving.count != (size_t)nInstances + 1) {
        HIP_TRY(staged.closeRows.allocate((size_t)3 * nInstances + 1));
        HIP_TRY(staged.moving.allocate((size_t)nInstances + 1));
        HIP_TRY(staged.boxRecords.allocate((size_t)kInstanceQuads * nInstances + 1));
        HIP_TRY(staged.boxTable.allocate(2 * ((size_t)nPrototypes + (size_t)nInstances)));
    }
    if (deviceClose && !scene->instanceBad.ptr) { HIP_TRY(scene->instanceBad.allocate(2)); }
    // render calls on a caller's stream may still walk the tree, and the caller's own stream may still write the transforms
    HIP_TRY(hipDeviceSynchronize());
    EventTimer timer;
    if (deviceClose) {
        const unsigned int clear[2] = { 0u, 0xFFFFFFFFu };
        unsigned int bad[2] = { 0u, 0u };
        HIP_TRY(hipMemcpy(scene->instanceBad.ptr, clear, sizeof clear, hipMemcpyHostToDevice));
        const int threads = nInstances > 2 * nPrototypes ? nInstances : 2 * nPrototypes;
        if (threads > 0) {
            timer.run([&]() {
                hipLaunchKernelGGL(k_motion_boxes, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                                   deviceClose, nInstances, scene->instanceRecords.ptr, scene->protoBoxes.ptr, nPrototypes, shutter_open, shutter_close,
                                   staged.closeRows.ptr, staged.moving.ptr, staged.boxRecords.ptr, staged.boxTable.ptr, scene->instanceBad.ptr);
            });
        }
        if (timer.ok()) { timer.keep(hipMemcpy(bad, scene->instanceBad.ptr, sizeof bad, hipMemcpyDeviceToHost)); }
        if (!timer.ok()) { return fail(PATHED_E_DEVICE, std::string("set_instance_motion: ") + hipGetErrorString(timer.status)); }
        if (bad[0] != 0u) {
            // (the staged buffers are simply not adopted: the scene keeps the motion it had, or none)
            return fail(PATHED_E_INVALID, "instance transform " + std::to_string(bad[1]) + " of shutter time 1 is not finite or not invertible (" + std::to_string(bad[0])
                        + " of the " + std::to_string(nInstances) + " transforms are refused; the scene keeps its state)");
        }
    }
    // the refit over the staged boxes (or, removing the motion, over the static ones); the scene's state flips once it succeeded
    const int code = refitTopTree(scene, deviceClose ? &staged : nullptr, timer, "set_instance_motion");
    if (code != PATHED_OK) { return code; }
    if (deviceClose) {
        scene->motion.closeRows.swap(staged.closeRows);
        scene->motion.moving.swap(staged.moving);
        scene->motion.boxRecords.swap(staged.boxRecords);
        scene->motion.boxTable.swap(staged.boxTable);
        scene->motionSet.closeRows = scene->motion.closeRows.ptr;
        scene->motionSet.moving = scene->motion.moving.ptr;
        scene->motionSet.open = shutter_open;
        scene->motionSet.close = shutter_close;
    }
    scene->hasMotion = deviceClose != nullptr;
    if (device_ms) { *device_ms = timer.ms; }
    return PATHED_OK;
}

int pathed_hip_scene_set_instance_motion_device(PathedScene *scene, const float *d_transforms_close, uint32_t n_instances, float shutter_open, float shutter_close, float *device_ms)
{
    const int code = checkInstanceMotion(scene, n_instances, d_transforms_close == nullptr, shutter_open, shutter_close);
    if (code != PATHED_OK) { return code; }
    SELECT_DEVICE(scene);
    return setInstanceMotion(scene, d_transforms_close, shutter_open, shutter_close, device_ms);
}

int pathed_hip_scene_set_instance_motion(PathedScene *scene, const float *transforms_close, uint32_t n_instances, float shutter_open, float shutter_close, float *device_ms)
{
    const int code = checkInstanceMotion(scene, n_instances, transforms_close == nullptr, shutter_open, shutter_close);
    if (code != PATHED_OK) { return code; }
    SELECT_DEVICE(scene);
    if (!transforms_close) { return setInstanceMotion(scene, nullptr, shutter_open, shutter_close, device_ms); }
    // the endpoints are refused by name before anything is launched (the device kernel repeats the test for the _device entry)
    for (size_t i = 0; i < (size_t)12 * n_instances; i++) {
        if (!(transforms_close[i] - transforms_close[i] == 0.f)) {
            return fail(PATHED_E_INVALID, "instance transform " + std::to_string(i / 12) + " of shutter time 1 is not finite");
        }
    }
    for (uint32_t k = 0; k < n_instances; k++) {
        float inverse[12];
        if (!instanceInverse(transforms_close + (size_t)12 * k, inverse)) {
            return fail(PATHED_E_INVALID, "instance transform " + std::to_string(k) + " of shutter time 1 is not invertible");
        }
    }
    const size_t floats = (size_t)12 * n_instances;
    if (scene->motionTransforms.count != floats + 1) { HIP_TRY(scene->motionTransforms.allocate(floats + 1)); }
    if (floats > 0) { HIP_TRY(hipMemcpy(scene->motionTransforms.ptr, transforms_close, floats * sizeof(float), hipMemcpyHostToDevice)); }
    return setInstanceMotion(scene, scene->motionTransforms.ptr, shutter_open, shutter_close, device_ms);
}

// ---- rebuilding the top tree (include/pathed_hip.h; lbvh.hip: buildTopBvhOnDevice; instance_kernels.h: k_placement_boxes,
// k_rebase_prototype_nodes, k_rebase_instance_roots).  Everything new is built beside the live arrays -- node array
// [new top | prototypes' trees], leaf triangles [world in the new leaf order | prototypes], records with their protoRoot
// moved -- and adopted at the end by swapping pointers: an error before that leaves the scene untouched.
int pathed_hip_scene_rebuild_top(PathedScene *scene, int32_t builder, float *device_ms)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    if (!scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "rebuild_top: the scene has no instances (pathed_hip_scene_create_instanced makes one that has)"); }
    if (builder != PATHED_BVH_LBVH_DEVICE && builder != PATHED_BVH_PLOC_DEVICE) {
        return fail(PATHED_E_UNSUPPORTED, "rebuild_top builds on the device, with the LBVH or the PLOC builder: the host builder needs the scene created again");
    }
    SELECT_DEVICE(scene);
    const int nInstances = scene->instanceSet.nInstances, worldTris = scene->instanceSet.worldTris;
    const int oldTop = scene->topNodes, oldCount = scene->bvh.nodeCount, deepest = scene->bvh.maxDepth - scene->topDepth;
    if (oldTop <= 0 || oldCount < oldTop || (size_t)oldCount > scene->nodes.count / 8 || worldTris < 0 || worldTris > scene->device.nTris || deepest < 0) {
        return fail(PATHED_E_INVALID, "the scene has no top tree");
    }
    // render calls on a caller's stream may still walk the tree
    HIP_TRY(hipDeviceSynchronize());
    if (device_ms) { *device_ms = 0.f; }
    if ((long long)worldTris + nInstances < 2) { return PATHED_OK; }   // nothing to arrange: the tree stays (an empty world keeps its empty root)
    const size_t protoNodes = (size_t)(oldCount - oldTop), protoTris = (size_t)(scene->device.nTris - worldTris);
    if (scene->instanceRecordsStaged.count != scene->instanceRecords.count) { HIP_TRY(scene->instanceRecordsStaged.allocate(scene->instanceRecords.count)); }
    DeviceBuffer<float4> boxes;
    HIP_TRY(boxes.allocate(2 * (size_t)nInstances));
    EventTimer timer;
    const auto giveUp = [&](const std::string &what) { return fail(PATHED_E_DEVICE, "rebuild_top: " + what); };
    if (nInstances > 0) {
        timer.run([&]() {
            // (while a shutter is set: over the moving boxes, from what k_motion_boxes left in place of records and prototype boxes)
            const float4 *records = scene->hasMotion ? scene->motion.boxRecords.ptr : scene->instanceRecords.ptr;
            const float4 *boxTable = scene->hasMotion ? scene->motion.boxTable.ptr : scene->protoBoxes.ptr;
            const int nBoxes = (int)((scene->hasMotion ? scene->motion.boxTable.count : scene->protoBoxes.count) / 2);
            hipLaunchKernelGGL(k_placement_boxes, dim3((unsigned)((nInstances + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                               records, nInstances, boxTable, nBoxes, boxes.ptr);
        });
    }
    if (!timer.ok()) { return giveUp(hipGetErrorString(timer.status)); }
    DeviceBvh built;
    std::string message;
    const hipError_t status = buildTopBvhOnDevice(builder == PATHED_BVH_PLOC_DEVICE ? kDeviceBuilderPloc : kDeviceBuilderLbvh, scene->leafTris.ptr, (uint32_t)worldTris,
                                                  boxes.ptr, (uint32_t)nInstances, protoNodes, protoTris, nullptr, &built, &message);
    // whatever the builder allocated, finished or not, is freed on every return below unless the scene adopts it
    DeviceBuffer<float4> newNodes, newLeafTris;
    newNodes.adopt(built.nodes, built.nodeCapacity * 8);
    newLeafTris.adopt(built.leafTris, ((size_t)worldTris + protoTris) * 3);
    if (status != hipSuccess) { return giveUp(message.empty() ? hipGetErrorString(status) : message); }
    const int newTop = built.nodeCount;
    if (newTop <= 0 || (size_t)newTop + protoNodes > built.nodeCapacity) { return giveUp("the builder made a wrong node count"); }
    timer.run([&]() {
        if (protoNodes > 0) {
            hipLaunchKernelGGL(k_rebase_prototype_nodes, dim3((unsigned)((8 * protoNodes + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                               scene->nodes.ptr, oldTop, oldCount, newNodes.ptr, newTop);
        }
        if (nInstances > 0) {
            hipLaunchKernelGGL(k_rebase_instance_roots, dim3((unsigned)(((size_t)kInstanceQuads * nInstances + kBlock - 1) / kBlock)), dim3(kBlock), 0, nullptr,
                               scene->instanceRecords.ptr, scene->instanceRecordsStaged.ptr, nInstances, newTop - oldTop);
        }
        if (protoTris > 0) {
            (void)hipMemcpyAsync(newLeafTris.ptr + 3 * (size_t)worldTris, scene->leafTris.ptr + 3 * (size_t)worldTris, protoTris * 3 * sizeof(float4), hipMemcpyDeviceToDevice, nullptr);
        }
    });
    if (timer.ok()) { timer.keep(hipDeviceSynchronize()); }
    if (!timer.ok()) { return giveUp(hipGetErrorString(timer.status)); }

    // adoption: nothing below can fail (the old arrays go with newNodes / newLeafTris at the end of the call)
    scene->nodes.swap(newNodes);
    scene->leafTris.swap(newLeafTris);
    scene->instanceRecords.swap(scene->instanceRecordsStaged);
    scene->instanceSet.records = scene->instanceRecords.ptr;
    scene->topNodes = newTop;
    scene->topDepth = built.maxDepth;
    scene->bvh.nodeCount = newTop + (int)protoNodes;
    scene->bvh.maxDepth = built.maxDepth + deepest;
    scene->bvhOnHost = false;   // exports download the new tree
    scene->instancedMaxStack = (3 * built.maxDepth + 1) + (3 * deepest + 1) + 1;
    scene->device.nodes = scene->nodes.ptr;
    scene->device.leafTris = scene->leafTris.ptr;
    scene->device.nNodes = scene->bvh.nodeCount;
    // the stack's bound and what hangs on it: configureTrace restates maxStack, stackRows, the LDS bytes and the grid; the
    // buffers ensureRenderState sized by them (suspended waves' stacks, the HBM overflow rows) are allocated again on the
    // next render call, as are the refit's side arrays (topNodes entries each) on the next set_instance_transforms
    configureTrace(scene);
    scene->suspendMask.release();
    scene->suspendData.release();
    scene->stackOverflow.release();
    scene->volumeOverflow.release();
    scene->topLo.release();
    scene->topHi.release();
    scene->topReady.release();
    if (device_ms) { *device_ms = timer.ms + built.buildMs; }
    return PATHED_OK;
}

int pathed_hip_debug_instance_records(PathedScene *scene, float *records, size_t n_instances)
{
    if (!scene || !records) { return fail(PATHED_E_INVALID, "null scene or records"); }
    if (!scene->instanced) { return fail(PATHED_E_UNSUPPORTED, "instance records: the scene has no instances"); }
    if (n_instances != (size_t)scene->instanceSet.nInstances) { return fail(PATHED_E_INVALID, "instance records: the instance count must be the scene's"); }
    SELECT_DEVICE(scene);
    if (n_instances > 0) {
        HIP_TRY(hipDeviceSynchronize());
        HIP_TRY(hipMemcpy(records, scene->instanceRecords.ptr, n_instances * (size_t)kInstanceQuads * sizeof(float4), hipMemcpyDeviceToHost));
    }
    return PATHED_OK;
}

int pathed_hip_set_stats_mode(PathedScene *scene, int enabled)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    scene->countMode = (enabled & 1) != 0;   // bit 0: count child boxes / triangles tested
    scene->timeKernels = (enabled & (2 | 4)) != 0; // bit 1: HIP-event timing of every trace / shade launch
    scene->timeInterval = (enabled & 4) ? 8 : 1;   // bit 2: ... of every 8th launch only (the event pairs cost ~6 % of the rate)
    return PATHED_OK;
}

int pathed_hip_reset_stats(PathedScene *scene)
{
    if (!scene) { return fail(PATHED_E_INVALID, "null scene"); }
    SELECT_DEVICE(scene);
    if (scene->stats.ptr) { HIP_TRY(hipMemset(scene->stats.ptr, 0, kStatCount * sizeof(unsigned long long))); }
    scene->iterations = 0;
    scene->traceLaunchesAll = 0;
    scene->cameraSamples = 0;
    scene->featureRays = 0;
    scene->traceEvents.totalMs = 0.0;
    scene->traceEvents.launches = 0;
    scene->shadeEvents.totalMs = 0.0;
    scene->shadeEvents.launches = 0;
    return PATHED_OK;
}

int pathed_hip_get_stats(PathedScene *scene, PathedStats *out)
{
    if (!scene || !out) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(scene);
    std::memset(out, 0, sizeof *out);
    unsigned long long device[kStatCount] = { 0 };
    if (scene->stats.ptr) {
        HIP_TRY(hipMemcpy(device, scene->stats.ptr, sizeof device, hipMemcpyDeviceToHost));
    }
    out->camera_samples = scene->cameraSamples;
    out->closest_rays = device[kStatClosest] + scene->featureRays;
    out->shadow_rays = device[kStatShadow];
    out->nodes_visited = device[kStatBoxes];
    out->tris_tested = device[kStatTris];
    out->dropped_samples = device[kStatDropped];
    out->local_closest_rays = device[kStatLocalClosest];
    out->local_shadow_rays = device[kStatLocalShadow];
    out->iterations = scene->iterations;
    out->trace_ms = scene->traceEvents.totalMs;
    out->shade_ms = scene->shadeEvents.totalMs;
    out->trace_launches = scene->traceEvents.launches;
    out->bvh_nodes = (uint64_t)scene->bvh.nodeCount;
    out->bvh_bytes = (uint64_t)scene->bvh.nodeCount * 128 + (uint64_t)scene->device.nTris * 48;
    out->bvh_max_depth = (uint32_t)scene->bvh.maxDepth;
    out->scene_in_lds = scene->bruteForce ? 2u : (scene->sceneInLds ? 1u : 0u);
    out->max_boxes_per_ray = device[kStatMaxBoxes];
    out->parked_rays = device[kStatParked];
    out->bvh_build_ms = scene->bvhBuildMs;
    out->bvh_builder = (uint32_t)scene->bvhBuilder;
    out->trace_launches_all = (uint32_t)scene->traceLaunchesAll;
    out->path_kernel = scene->instanced ? (scene->hasMotion ? 11u : 10u) : scene->lastCallFeatures ? 8u : (scene->lastCallList && !usesVolumeKernel(scene)) ? 1u : usesVolumeKernel(scene) ? (scene->integrator == PATHED_INTEGRATOR_BASIC_VOLUME ? (scene->anisotropic ? 11u : 9u) : 4u) : scene->fusedPath ? 3u : scene->lastCallHybrid ? 7u : scene->lastCallWave ? 6u : scene->splitShade ? 5u : (scene->stagedShade ? 2u : 1u);
    if (tuningEnv("PATHED_SHADE_PROFILE")) {   // counters exist in -DPATHED_SHADE_PROFILE builds only
        static const char *regions[11] = { "all waves", "active slots", "makeIsect (hit)", "camera-ray vertex", "finish previous MIS term",
                                           "new vertex: BSDF sample", "light sampling", "sample finished", "startSample (regeneration)", "shadow ray pushed",
                                           "BSDF sample with black throughput" };
        for (int r = 0; r < 11; r++) {
            const unsigned long long waves = device[kStatShadeProfile + 2 * r], lanes = device[kStatShadeProfile + 2 * r + 1];
            fprintf(stderr, "[pathed] k_shade region %-28s waves %12llu  (%.3f of all)  lanes per wave %.1f\n", regions[r], waves,
                    device[kStatShadeProfile] ? (double)waves / (double)device[kStatShadeProfile] : 0.0, waves ? (double)lanes / (double)waves : 0.0);
        }
    }
    if (tuningEnv("PATHED_FUSED_PROFILE")) {   // the same counters in k_path_small (-DPATHED_SHADE_PROFILE builds)
        static const char *regions[9] = { "iterations (live lanes)", "camera ray started in place", "passes with shadow rays (lanes with one)",
                                          "arrival: the hit's record", "camera-ray vertex (hit taken from the queue)", "BSDF sample met an emitter: lightsPDF",
                                          "new vertex: makeIsect, BSDF sample", "light sampling", "sample finished" };
        static const int shown[10] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 11 };   // (9, 10: the resolve loops, below)
        for (int k = 0; k < 10; k++) {
            const int r = shown[k];
            const char *name = r == 11 ? "refill of the camera queue (units started)" : regions[r];
            const unsigned long long waves = device[kStatShadeProfile + 2 * r], lanes = device[kStatShadeProfile + 2 * r + 1];
            fprintf(stderr, "[pathed] k_path_small %-44s waves %12llu  (%.3f of the iterations)  lanes per wave %.1f\n", name, waves,
                    device[kStatShadeProfile] ? (double)waves / (double)device[kStatShadeProfile] : 0.0, waves ? (double)lanes / (double)waves : 0.0);
        }
        static const char *loops[2] = { "resolve loop of the path's ray", "resolve loop of the shadow ray" };
        for (int r = 0; r < 2; r++) {
            const unsigned long long turns = device[kStatShadeProfile + 2 * (9 + r)], candidates = device[kStatShadeProfile + 2 * (9 + r) + 1];
            fprintf(stderr, "[pathed] k_path_small %-44s %.2f turns per iteration, %.2f candidates per turn (of 64 lanes)\n", loops[r],
                    device[kStatShadeProfile] ? (double)turns / (double)device[kStatShadeProfile] : 0.0, turns ? (double)candidates / (double)turns : 0.0);
        }
    }
    if (tuningEnv("PATHED_WAVE_PROFILE")) {   // k_path_wave (-DPATHED_SHADE_PROFILE builds, tools/wave_profile.py)
        const unsigned long long *v = device + kStatShadeProfile;
        const double iterations = v[0] ? (double)v[0] : 1.0, cycles = v[8] ? (double)v[8] : 1.0;
        fprintf(stderr, "[pathed] k_path_wave: %llu waves, %.0f iterations each, %.1f live paths per iteration\n", v[11], iterations / (double)(v[11] ? v[11] : 1), (double)v[1] / iterations);
        fprintf(stderr, "[pathed] k_path_wave traversal: %.1f rays posted per iteration, %.1f steps per iteration at %.1f of 64 lanes, %.1f rays left in flight at the end of a burst\n",
                (double)v[6] / iterations, (double)v[2] / iterations, v[2] ? (double)v[3] / (double)v[2] : 0.0, (double)v[7] / iterations);
        fprintf(stderr, "[pathed] k_path_wave shade: %.3f of the iterations shade, %.1f paths each\n", (double)v[4] / iterations, v[4] ? (double)v[5] / (double)v[4] : 0.0);
        fprintf(stderr, "[pathed] k_path_wave wave cycles: traversal bursts %.3f, shade + post + regeneration %.3f of the waves' lifetimes\n", (double)v[9] / cycles, (double)v[10] / cycles);
    }
#ifdef PATHED_SHADE_PROFILE
    if (scene->lastCallHybrid) {   // k_path_hybrid (tools/hybrid_profile.py)
        const unsigned long long *v = device + kStatShadeProfile;
        const double iterations = v[0] ? (double)v[0] : 1.0, cycles = v[8] ? (double)v[8] : 1.0, bursts = v[3] ? (double)v[3] : 1.0;
        fprintf(stderr, "[pathed] k_path_hybrid: %llu waves, %.0f iterations each, %.1f live paths per iteration, %.1f of them at a vertex\n", v[12], iterations / (double)(v[12] ? v[12] : 1),
                (double)v[1] / iterations, (double)v[13] / iterations);
        fprintf(stderr, "[pathed] k_path_hybrid tree part: %.3f of the iterations run a burst, %.1f rays posted per burst, %.1f steps per burst (%.1f of them triangle phases) at %.1f of 64 lanes, %.2f refill rounds, %.1f rays parked at its end\n",
                (double)v[3] / iterations, (double)v[2] / bursts, (double)v[4] / bursts, (double)v[7] / bursts, v[4] ? (double)v[5] / (double)v[4] : 0.0, (double)v[6] / bursts, (double)v[14] / bursts);
        fprintf(stderr, "[pathed] k_path_hybrid wave cycles: direct pass + resolve %.3f, proxy + burst %.3f, vertex + regeneration %.3f of the waves' lifetimes\n",
                (double)v[9] / cycles, (double)v[10] / cycles, (double)v[11] / cycles);
    }
#endif
    if (tuningEnv("PATHED_VOLUME_PROFILE")) {   // the same counters in k_path_volume (-DPATHED_SHADE_PROFILE builds)
        // (region 3 and 9: k_path_scatter only -- the query of the ray that leaves a scatter event, and the scatter events)
        static const char *regions[10] = { "samples", "camera-ray query", "bounce-loop iterations", "segment query (no direct lighting before)",
                                           "medium event: occlusion query", "direct lighting at a vertex", "light sample: occlusion query",
                                           "BSDF sample: closest query", "seen through a container: query", "scatter events" };
        for (int r = 0; r < 10; r++) {
            const unsigned long long waves = device[kStatShadeProfile + 2 * r], lanes = device[kStatShadeProfile + 2 * r + 1];
            fprintf(stderr, "[pathed] k_path_volume %-44s waves %12llu  (%.3f per sample-wave)  lanes per wave %.1f\n", regions[r], waves,
                    device[kStatShadeProfile] ? (double)waves / (double)device[kStatShadeProfile] : 0.0, waves ? (double)lanes / (double)waves : 0.0);
        }
    }
    if (getenv("PATHED_DEBUG_STATS")) {
        if (scene->cameraMasksBuilt) {
            fprintf(stderr, "[pathed] camera masks: %d pixels x %d triangles, last built in %.3f ms on the device\n", scene->width * scene->height,
                    scene->device.nTris, scene->cameraMaskMs);
        }
        fprintf(stderr, "[pathed] wave steps %llu lane steps %llu (lane utilisation %.3f) refill rounds %llu\n",
                device[kStatWaveSteps], device[kStatLaneSteps],
                device[kStatWaveSteps] ? (double)device[kStatLaneSteps] / (64.0 * (double)device[kStatWaveSteps]) : 0.0,
                device[kStatRefills]);
        fprintf(stderr, "[pathed] sum of wave lifetimes %.3e cycles, longest single wave %.3e cycles\n",
                (double)device[kStatWaveCycles], (double)device[kStatWaveCyclesMax]);
        fprintf(stderr, "[pathed] wave cycles: refill %.3e, inner phases %.3e (%llu steps), triangle phases %.3e\n",
                (double)device[kStatRefillCycles], (double)device[kStatInnerCycles], device[kStatInnerSteps], (double)device[kStatLeafCycles]);
        fprintf(stderr, "[pathed] tail (no cards left): %llu wave steps, %llu lane steps, %.3e cycles; %llu rays parked\n",
                device[kStatTailSteps], device[kStatTailLaneSteps], (double)device[kStatTailCycles], device[kStatParked]);
    }
    return PATHED_OK;
}

int pathed_hip_scene_export_bvh(PathedScene *scene, float *nodes, size_t *n_nodes, float *tris, size_t *n_tris)
{
    if (!scene || !n_nodes || !n_tris) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(scene);
    if (!scene->bvhOnHost) {
        // a device-built tree: fetch it once
        scene->bvh.nodes.resize((size_t)scene->bvh.nodeCount * kNodeFloats);
        scene->bvh.leafTris.resize((size_t)scene->device.nTris * 12);
        HIP_TRY(hipMemcpy(scene->bvh.nodes.data(), scene->nodes.ptr, scene->bvh.nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(scene->bvh.leafTris.data(), scene->leafTris.ptr, scene->bvh.leafTris.size() * sizeof(float), hipMemcpyDeviceToHost));
        scene->bvhOnHost = true;
    }
    const size_t nodeCount = (size_t)scene->bvh.nodeCount;
    const size_t triCount = scene->bvh.leafTris.size() / 12;
    if (nodes) {
        if (*n_nodes < nodeCount) { return fail(PATHED_E_INVALID, "node buffer too small"); }
        std::memcpy(nodes, scene->bvh.nodes.data(), nodeCount * kNodeFloats * sizeof(float));
    }
    if (tris) {
        if (*n_tris < triCount) { return fail(PATHED_E_INVALID, "triangle buffer too small"); }
        std::memcpy(tris, scene->bvh.leafTris.data(), triCount * 12 * sizeof(float));
    }
    *n_nodes = nodeCount;
    *n_tris = triCount;
    return PATHED_OK;
}

int pathed_hip_scene_export_compressed_nodes(PathedScene *scene, uint32_t *nodes, size_t *n_nodes, size_t *words_per_node)
{
    if (!scene || !n_nodes) { return fail(PATHED_E_INVALID, "null argument"); }
    SELECT_DEVICE(scene);
    const size_t nodeCount = scene->nodeFormat != 0 ? (size_t)scene->bvh.nodeCount : 0;
    const size_t words = scene->nodeFormat == 2 ? 32 : 16;
    if (nodes && nodeCount > 0) {
        if (*n_nodes < nodeCount) { return fail(PATHED_E_INVALID, "node buffer too small"); }
        HIP_TRY(hipMemcpy(nodes, scene->nodesQ.ptr, nodeCount * words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    *n_nodes = nodeCount;
    if (words_per_node) { *words_per_node = nodeCount > 0 ? words : 0; }
    return PATHED_OK;
}

}  // extern "C"
