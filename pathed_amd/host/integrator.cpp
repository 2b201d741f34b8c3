#include "integrator.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <thread>

namespace pathed {

namespace {

std::string hipError(const char *what)
{
    return std::string(what) + ": " + pathed_hip_last_error();
}

// One host thread per replica (= per device), alive for the whole render: `run(work)` hands work(replica) to every
// worker and returns when all are through; the first failure is rethrown on the caller's thread.  (Round 2 created and
// joined the threads for every batch: at the 1-, 1-, 2-, 4-sample batches of the first checkpoints that was most of
// the batch.)
class ReplicaWorkers {
public:
    explicit ReplicaWorkers(size_t replicas) : m_failures(replicas)
    {
        for (size_t r = 1; r < replicas; r++) { m_threads.emplace_back([this, r]() { serve(r); }); }
    }
    ~ReplicaWorkers()
    {
        {
            std::lock_guard<std::mutex> guard(m_mutex);
            m_stop = true;
            m_generation++;
        }
        m_wake.notify_all();
        for (std::thread &thread : m_threads) { thread.join(); }
    }
    void run(const std::function<void(size_t)> &work)
    {
        const size_t replicas = m_failures.size();
        for (std::string &failure : m_failures) { failure.clear(); }
        if (replicas > 1) {
            std::lock_guard<std::mutex> guard(m_mutex);
            m_work = &work;
            m_pending = replicas - 1;
            m_generation++;
        }
        m_wake.notify_all();
        attempt(work, 0);   // replica 0 on the caller's thread
        if (replicas > 1) {
            std::unique_lock<std::mutex> lock(m_mutex);
            m_done.wait(lock, [this]() { return m_pending == 0; });
            m_work = nullptr;
        }
        for (const std::string &failure : m_failures) {
            if (!failure.empty()) { throw std::runtime_error(failure); }
        }
    }

private:
    void attempt(const std::function<void(size_t)> &work, size_t replica)
    {
        try { work(replica); }
        catch (const std::exception &error) { m_failures[replica] = error.what(); if (m_failures[replica].empty()) { m_failures[replica] = "unknown error"; } }
        catch (...) { m_failures[replica] = "unknown error"; }
    }
    void serve(size_t replica)
    {
        unsigned long long seen = 0;
        while (true) {
            const std::function<void(size_t)> *work = nullptr;
            {
                std::unique_lock<std::mutex> lock(m_mutex);
                m_wake.wait(lock, [&]() { return m_generation != seen; });
                seen = m_generation;
                if (m_stop) { return; }
                work = m_work;
            }
            if (work) { attempt(*work, replica); }
            {
                std::lock_guard<std::mutex> guard(m_mutex);
                if (m_pending > 0) { m_pending--; }
            }
            m_done.notify_one();
        }
    }

    std::vector<std::thread> m_threads;
    std::vector<std::string> m_failures;
    std::mutex m_mutex;
    std::condition_variable m_wake, m_done;
    const std::function<void(size_t)> *m_work = nullptr;
    size_t m_pending = 0;
    unsigned long long m_generation = 0;
    bool m_stop = false;
};

// The sidecar a resumed job continues from: the fp32 radiance SUMS and how many samples they hold.
// Because the random stream is a pure function of (seed, pixel, sample, dimension), "the next
// sample" needs no generator state: a resumed run is the straight run, bit for bit, as long as the
// interruption fell on a batch boundary (it always does: the file is written after a batch).
struct StateHeader {
    char magic[8];            // "PATHEDS3"
    int32_t width, height;
    int32_t done;             // samples per pixel already in the sums
    int32_t startBounce, lastBounce;
    uint64_t seed;
    uint64_t jobDigest;       // what else the sums depend on: scene file, integrator, samples per unit (Integrator::setStateIdentity)
};

}  // namespace

Scene::Scene(FlatScene flat, int device)
    : m_flat(std::move(flat)), m_devices(1, device)
{
    upload(0);
}

Scene::Scene(FlatScene flat, const std::vector<int> &devices, int bvhBuilder)
    : m_flat(std::move(flat)), m_devices(devices)
{
    if (m_devices.empty()) { throw std::runtime_error("Scene: no device"); }
    upload(bvhBuilder + 1);
}

void Scene::upload(int bvhBuilderPlusOne)
{
    m_handles.assign(m_devices.size(), nullptr);
    const PathedSceneDesc desc = m_flat.desc();
    const PathedInstanceDesc instances = m_flat.instanceDesc();   // scene files with "instance" / "instanced" models
    for (size_t i = 0; i < m_flat.grids.size(); i++) { (void)m_flat.gridDesc(i); }   // (sets the data pointers once, before the replica threads read them)
    for (size_t i = 0; i < m_flat.phases.size(); i++) { (void)m_flat.phaseDesc(i); }   // (... and fills the phase records)
    try {
        // every device builds / uploads its own replica, in parallel
        ReplicaWorkers workers(m_devices.size());
        workers.run([&](size_t r) {
            PathedSceneOptions options;
            std::memset(&options, 0, sizeof options);
            options.struct_size = sizeof options;
            options.device = m_devices[r];
            options.bvh_builder = bvhBuilderPlusOne;
            if (m_flat.instanced()) {
                if (pathed_hip_scene_create_instanced(&desc, &options, &instances, &m_handles[r]) != PATHED_OK) {
                    throw std::runtime_error(hipError("pathed_hip_scene_create_instanced"));
                }
            } else if (pathed_hip_scene_create_ex(&desc, &options, &m_handles[r]) != PATHED_OK) {
                throw std::runtime_error(hipError("pathed_hip_scene_create_ex"));
            }
            if (m_flat.moves()) {   // the scene file's "transform_close" placements over the job's "shutter"
                if (pathed_hip_scene_set_instance_motion(m_handles[r], m_flat.instancesClose.data(), (uint32_t)m_flat.instances.size(),
                                                         m_flat.shutterOpen, m_flat.shutterClose, nullptr) != PATHED_OK) {
                    throw std::runtime_error(hipError("pathed_hip_scene_set_instance_motion"));
                }
            }
            for (size_t i = 0; i < m_flat.grids.size(); i++) {   // the scene file's voxel-grid media, each on its medium slot
                if (pathed_hip_scene_set_grid_medium(m_handles[r], m_flat.grids[i].medium, m_flat.gridDesc(i)) != PATHED_OK) {
                    throw std::runtime_error(hipError("pathed_hip_scene_set_grid_medium"));
                }
            }
            for (size_t i = 0; i < m_flat.phases.size(); i++) {   // ... and its Henyey-Greenstein phase functions
                if (pathed_hip_scene_set_medium_phase(m_handles[r], m_flat.phases[i].medium, m_flat.phaseDesc(i)) != PATHED_OK) {
                    throw std::runtime_error(hipError("pathed_hip_scene_set_medium_phase"));
                }
            }
        });
    } catch (...) {
        for (PathedScene *handle : m_handles) { pathed_hip_scene_destroy(handle); }
        throw;
    }
}

Scene::~Scene()
{
    for (PathedScene *handle : m_handles) { pathed_hip_scene_destroy(handle); }
}

void Integrator::configure(int spp, unsigned long long seed, int sppPerLaunch, const std::string &logPrefix)
{
    if (sppPerLaunch < 1) { throw std::runtime_error("spp_per_launch must be >= 1"); }
    if (spp < 1) { throw std::runtime_error("spp must be >= 1"); }
    m_spp = spp;
    m_seed = seed;
    m_sppPerLaunch = sppPerLaunch;
    m_logPrefix = logPrefix;
}

// reference src/integrator.cpp:19-106.  The reference adds one sample per pixel per wave to a host
// vector; here the sums stay on the devices (one buffer per replica) and come to the host only when
// an image is due: at the power-of-two checkpoints (src/integrator.cpp:87-92), at the end, and when
// `quit` is raised.  With G replicas the samples of a batch [done, done + count) are split
// G ways (contiguous shares, strongRange), every replica adds its share into its own buffer on its
// own host thread, and an image is  sum over replicas  / done: waves are additive
// (src/integrator.cpp:42-51), so the union over replicas of what they have rendered is always
// exactly the samples [0, done) -- the single-GPU image up to fp32 summation order.
void Integrator::run(
    Image &image,
    Scene &scene,
    std::function<void(RenderStatus)> callback,
    bool *quit
) {
    if (m_adaptive) { runAdaptive(image, scene, callback, quit); return; }
    const int width = scene.width();
    const int height = scene.height();
    const int primarySamples = m_spp;
    const size_t replicas = scene.replicas();
    const size_t floats = (size_t)3 * width * height;

    printf("Beginning pre-process...\n");
    preprocess(scene);
    printf("Pre-process complete (0.0s elapsed)\n");

    std::vector<float *> deviceSums(replicas, nullptr);
    float *staging = nullptr;   // on replica 0's device: a peer's sums on their way into the total (peer-copy fan-in only)
    float *total = nullptr;     // on replica 0's device: sum over replicas (G > 1 only)
    PathedComm *comm = nullptr; // RCCL communicator over the replicas' devices (distinct devices only)
    struct Cleanup {
        Scene &scene;
        std::vector<float *> &sums;
        float *&staging;
        float *&total;
        PathedComm *&comm;
        ~Cleanup()
        {
            pathed_hip_comm_destroy(comm);
            for (size_t r = 0; r < sums.size(); r++) { if (sums[r]) { pathed_hip_accum_free(scene.handle(r), sums[r]); } }
            if (staging) { pathed_hip_accum_free(scene.handle(0), staging); }
            if (total) { pathed_hip_accum_free(scene.handle(0), total); }
        }
    } cleanup{ scene, deviceSums, staging, total, comm };
    for (size_t r = 0; r < replicas; r++) {
        if (pathed_hip_accum_alloc(scene.handle(r), floats, &deviceSums[r]) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
    }
    m_metrics = RenderMetrics();
    if (replicas > 1) {
        if (pathed_hip_accum_alloc(scene.handle(0), floats, &total) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
        // the path's one exchange step as ONE collective (RCCL reduce over xGMI); replicas that share a
        // device, or a machine without librccl, fall back to peer copies + adds on replica 0
        if (m_adoptedComm) { comm = m_adoptedComm; m_adoptedComm = nullptr; }
        else if (m_useRccl && pathed_hip_comm_init((int)replicas, scene.devices().data(), &comm) != PATHED_OK) {
            comm = nullptr;
            m_metrics.reduceFallback = pathed_hip_last_error();
            // replicas that SHARE a device cannot form a communicator (rehearsals on one GPU): peer copies.  On distinct
            // devices -- a real node -- "reduce": "rccl" means RCCL: a silent fall-back would hide a broken xGMI / RCCL setup
            // behind a slower path, so the job stops here ("reduce": "peer-copy" asks for the copies explicitly).
            std::vector<int> ids = scene.devices();
            std::sort(ids.begin(), ids.end());
            const bool distinct = std::adjacent_find(ids.begin(), ids.end()) == ids.end();
            if (distinct) {
                throw std::runtime_error("job asks for the RCCL reduce over " + std::to_string(replicas) + " distinct GPUs and RCCL is unavailable: "
                                         + m_metrics.reduceFallback + " (set \"reduce\": \"peer-copy\" to use peer copies)");
            }
            std::cout << "[" << m_logPrefix << "] RCCL reduce unavailable (" << m_metrics.reduceFallback << "): replicas share a device, using peer copies" << std::endl;
        }
        if (!comm) {
            if (pathed_hip_accum_alloc(scene.handle(0), floats, &staging) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
        }
    }
    m_metrics.reduceMethod = replicas == 1 ? "none" : comm ? "rccl" : "peer-copy";

    // second moments (setNoise): one squares buffer per replica beside its sums, and their total on replica 0
    const bool wantMoments = m_collectMoments;
    if (wantMoments && m_resume) { throw std::runtime_error("job: \"resume\" does not go with \"target_noise\" / \"stderr_image\": the state file holds no squares"); }
    std::vector<float *> deviceSquares(replicas, nullptr);
    float *totalSquares = nullptr;
    struct MomentsCleanup {
        Scene &scene;
        std::vector<float *> &squares;
        float *&total;
        ~MomentsCleanup()
        {
            for (size_t r = 0; r < squares.size(); r++) { if (squares[r]) { pathed_hip_accum_free(scene.handle(r), squares[r]); } }
            if (total) { pathed_hip_accum_free(scene.handle(0), total); }
        }
    } momentsCleanup{ scene, deviceSquares, totalSquares };
    if (wantMoments) {
        for (size_t r = 0; r < replicas; r++) {
            if (pathed_hip_accum_alloc(scene.handle(r), floats, &deviceSquares[r]) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
        }
        if (replicas > 1 && pathed_hip_accum_alloc(scene.handle(0), floats, &totalSquares) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
    }
    m_metrics.collectedMoments = wantMoments;
    std::vector<float> squaresLookup;
    ReplicaWorkers workers(replicas);

    std::vector<float> radianceLookup(floats, 0.f);
    int done = 0;
    if (m_resume) {
        done = loadState(radianceLookup, width, height);
        if (done > 0) {
            // the sums so far continue on replica 0
            if (pathed_hip_accum_upload(scene.handle(0), deviceSums[0], floats, radianceLookup.data()) != PATHED_OK) {
                throw std::runtime_error(hipError("pathed_hip_accum_upload"));
            }
            std::cout << "[" << m_logPrefix << "] resuming at sample " << done << "/" << primarySamples << std::endl;
        }
        if (done >= primarySamples) {
            // nothing left to render: the image is the one the state file holds
            std::lock_guard<std::mutex> guard(image.getLock());
            image.setSpp(done);
            for (int row = 0; row < height; row++) {
                for (int col = 0; col < width; col++) {
                    const size_t index = (size_t)3 * ((size_t)row * width + col);
                    image.set(row, col, radianceLookup[index + 0] / done, radianceLookup[index + 1] / done, radianceLookup[index + 2] / done);
                }
            }
            std::cout << "[" << m_logPrefix << "] the state file already holds " << done << " samples: nothing to render" << std::endl;
        }
    }

    // feature images (setFeatures): sums on replica 0's device -- albedo, normal, depth, hits side by side -- that follow `done`
    // whenever an image is published
    const size_t pixels = (size_t)width * height;
    const bool wantFeatures = !m_features.empty();
    float *featureSums = nullptr;
    struct FeatureCleanup {
        Scene &scene;
        float *&sums;
        ~FeatureCleanup() { if (sums) { pathed_hip_accum_free(scene.handle(0), sums); } }
    } featureCleanup{ scene, featureSums };
    int featuresDone = 0;
    std::vector<float> featureHost;
    auto publishFeatures = [&](int upTo, bool checkpoint) {
        if (!wantFeatures) { return; }
        if (!featureSums && pathed_hip_accum_alloc(scene.handle(0), 8 * pixels, &featureSums) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
        PathedFeatureBuffers buffers = { featureSums, featureSums + 3 * pixels, featureSums + 6 * pixels, featureSums + 7 * pixels };
        while (featuresDone < upTo) {
            const int count = std::min(m_sppPerLaunch, upTo - featuresDone);
            if (pathed_hip_render_features_device(scene.handle(0), m_seed, (uint32_t)featuresDone, (uint32_t)count, &buffers, nullptr) != PATHED_OK) {
                throw std::runtime_error(hipError("pathed_hip_render_features_device"));
            }
            featuresDone += count;
        }
        featureHost.resize(8 * pixels);
        if (pathed_hip_accum_download(scene.handle(0), featureSums, 8 * pixels, featureHost.data()) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_download")); }
        for (const std::string &name : m_features) {
            Image featureImage(width, height, image.outputDirectory());
            featureImage.setSpp(upTo);
            for (int row = 0; row < height; row++) {
                for (int col = 0; col < width; col++) {
                    const size_t pixel = (size_t)row * width + col;
                    if (name == "depth") {
                        // mean distance of the samples that hit something, 0 where none did
                        const float hits = featureHost[7 * pixels + pixel];
                        const float depth = hits > 0.f ? featureHost[6 * pixels + pixel] / hits : 0.f;
                        featureImage.set(row, col, depth, depth, depth);
                    } else {
                        // albedo and normal: sum / samples (misses count as zero; normals stay unnormalised)
                        const float *sums = featureHost.data() + (name == "albedo" ? 0 : 3 * pixels) + 3 * pixel;
                        featureImage.set(row, col, sums[0] / upTo, sums[1] / upTo, sums[2] / upTo);
                    }
                }
            }
            if (checkpoint) { featureImage.saveCheckpoint("auto-" + name); }
            else { featureImage.save("auto-" + name); }
        }
    };

    m_metrics.replicas = (int)replicas;
    m_metrics.firstSample = done;
    m_metrics.replicaSeconds.assign(replicas, 0.0);
    const auto loopBegin = std::chrono::steady_clock::now();

    while (done < primarySamples) {
        // batches end on powers of two so checkpoints appear exactly where the reference
        // writes them (src/integrator.cpp:87-92)
        int nextPower = 1;
        while (nextPower <= done) { nextPower *= 2; }
        long long limit = (long long)m_sppPerLaunch * (long long)replicas;
        int count = (int)std::min<long long>(limit, primarySamples - done);
        count = std::min(count, nextPower - done);

        const auto begin = std::chrono::steady_clock::now();
        workers.run([&](size_t r) {
            unsigned first = 0, mine = 0;
            strongRange((unsigned)r, (unsigned)replicas, (unsigned)done, (unsigned)count, &first, &mine);
            if (mine == 0) { return; }
            const auto replicaBegin = std::chrono::steady_clock::now();
            sampleImage(deviceSums[r], deviceSquares[r], scene, r, first, mine);
            m_metrics.replicaSeconds[r] += std::chrono::duration<double>(std::chrono::steady_clock::now() - replicaBegin).count();
        });
        const auto end = std::chrono::steady_clock::now();
        done += count;

        postwave(scene, done);

        RenderStatus status;
        status.sample = done;
        status.elapsedSeconds = std::chrono::duration<double>(end - begin).count();
        if (callback) { callback(status); }

        const bool checkpoint = (done & (done - 1)) == 0;
        const bool stopping = quit && *quit;
        bool reachedTarget = false;
        std::ostringstream noiseLine;
        if (checkpoint || done == primarySamples || stopping) {
            const auto reduceBegin = std::chrono::steady_clock::now();
            const float *source = deviceSums[0];
            if (replicas > 1 && comm) {
                std::vector<const float *> send(deviceSums.begin(), deviceSums.end());
                if (pathed_hip_comm_reduce(comm, send.data(), total, floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_comm_reduce")); }
                source = total;
            } else if (replicas > 1) {
                // per-device sums -> replica 0 one by one (hipMemcpyPeer over xGMI + add)
                if (pathed_hip_accum_copy_peer(scene.handle(0), total, scene.handle(0), deviceSums[0], floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_copy_peer")); }
                for (size_t r = 1; r < replicas; r++) {
                    if (pathed_hip_accum_copy_peer(scene.handle(0), staging, scene.handle(r), deviceSums[r], floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_copy_peer")); }
                    if (pathed_hip_accum_add(scene.handle(0), total, staging, floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_add")); }
                }
                source = total;
            }
            // the squares are reduced exactly as the sums are
            const float *sourceSquares = deviceSquares[0];
            if (wantMoments && replicas > 1 && comm) {
                std::vector<const float *> send(deviceSquares.begin(), deviceSquares.end());
                if (pathed_hip_comm_reduce(comm, send.data(), totalSquares, floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_comm_reduce")); }
                sourceSquares = totalSquares;
            } else if (wantMoments && replicas > 1) {
                if (pathed_hip_accum_copy_peer(scene.handle(0), totalSquares, scene.handle(0), deviceSquares[0], floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_copy_peer")); }
                for (size_t r = 1; r < replicas; r++) {
                    if (pathed_hip_accum_copy_peer(scene.handle(0), staging, scene.handle(r), deviceSquares[r], floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_copy_peer")); }
                    if (pathed_hip_accum_add(scene.handle(0), totalSquares, staging, floats) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_add")); }
                }
                sourceSquares = totalSquares;
            }
            if (pathed_hip_accum_download(scene.handle(0), source, floats, radianceLookup.data()) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_download")); }
            if (wantMoments && done >= 2) {
                squaresLookup.resize(floats);
                if (pathed_hip_accum_download(scene.handle(0), sourceSquares, floats, squaresLookup.data()) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_download")); }
                if ((checkpoint || done == primarySamples) && done >= m_minSpp) {
                    PathedNoise figure;
                    std::memset(&figure, 0, sizeof figure);
                    figure.struct_size = sizeof figure;
                    if (pathed_hip_noise_estimate_device(scene.handle(0), source, sourceSquares, (uint32_t)done, (float)m_noiseFloor, (float)m_targetNoise,
                                                         nullptr, &figure, nullptr) != PATHED_OK) {
                        throw std::runtime_error(hipError("pathed_hip_noise_estimate_device"));
                    }
                    m_metrics.noise.push_back({ done, figure.mean_error, figure.max_error });
                    noiseLine << " noise: " << std::setprecision(6) << figure.mean_error;
                    if (m_targetNoise > 0.0 && figure.mean_error <= m_targetNoise && done < primarySamples) { reachedTarget = true; }
                }
            }
            m_metrics.reduceSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - reduceBegin).count();
            m_metrics.reduces++;

            std::lock_guard<std::mutex> guard(image.getLock());
            image.setSpp(done);
            for (int row = 0; row < height; row++) {
                for (int col = 0; col < width; col++) {
                    const size_t index = (size_t)3 * ((size_t)row * width + col);
                    image.set(
                        row, col,
                        radianceLookup[index + 0] / done,
                        radianceLookup[index + 1] / done,
                        radianceLookup[index + 2] / done);
                }
            }
            // files: auto.exr + auto-%05dspp.exr at the powers of two, as the reference (src/integrator.cpp:87-92).  The
            // reference renders ALL primarySamples waves (:42) and its last samples reach no file when the count is not a
            // power of two; here the end of the run also refreshes auto.exr -- "the latest image" -- so that every sample
            // rendered is in a file (no numbered checkpoint for it).  python -m pathed_amd.run_job does exactly the same.
            if (checkpoint) { image.saveCheckpoint("auto"); }
            else if (done == primarySamples) { image.save("auto"); }
            if (checkpoint || done == primarySamples) { publishFeatures(done, checkpoint); }
            if (wantMoments && done >= 2 && (checkpoint || done == primarySamples)) {
                // auto-stderr*.exr: per-channel standard error of the mean, sqrt(v_c / n), in the header's fp32 order (standard
                // error rather than variance: the files are HALF, and variances of 1e-5 would be mostly subnormal there)
                Image stderrImage(width, height, image.outputDirectory());
                stderrImage.setSpp(done);
                const float n = (float)done, bessel = n / (n - 1.f);
                for (int row = 0; row < height; row++) {
                    for (int col = 0; col < width; col++) {
                        const size_t index = (size_t)3 * ((size_t)row * width + col);
                        float error[3];
                        for (int c = 0; c < 3; c++) {
                            const float mean = radianceLookup[index + c] / n;
                            const float spread = squaresLookup[index + c] / n - mean * mean;
                            const float variance = (spread > 0.f ? spread : 0.f) * bessel;
                            error[c] = std::sqrt(variance / n);
                        }
                        stderrImage.set(row, col, error[0], error[1], error[2]);
                    }
                }
                if (checkpoint) { stderrImage.saveCheckpoint("auto-stderr"); }
                else { stderrImage.save("auto-stderr"); }
            }
            saveState(radianceLookup, width, height, done);
        }

        std::ostringstream line;
        line << "[" << m_logPrefix << "] sample: " << done << "/" << primarySamples
             << std::fixed << std::setprecision(1)
             << " (" << status.elapsedSeconds << "s elapsed)" << noiseLine.str();
        std::cout << line.str() << std::endl;

        if (stopping) { break; }
        if (reachedTarget) {
            m_metrics.stoppedOnNoise = true;
            std::cout << "[" << m_logPrefix << "] noise target " << m_targetNoise << " reached at " << done << " samples: stopping" << std::endl;
            break;
        }
    }
    m_metrics.lastSample = done;
    m_metrics.loopSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopBegin).count();
    m_metrics.width = width;
    m_metrics.height = height;
}

// job key "adaptive": the schedule of job.h.  Everything stays on replica 0's device between the rounds; the host sees the
// three images when files are due -- after the first step and after every round.
void Integrator::runAdaptive(Image &image, Scene &scene, std::function<void(RenderStatus)> callback, bool *quit)
{
    const int width = scene.width();
    const int height = scene.height();
    const size_t pixels = (size_t)width * height;
    const size_t floats = 3 * pixels;
    if (scene.replicas() != 1) { throw std::runtime_error("job: \"adaptive\" renders on one GPU: \"gpus\" must be 1 (a pixel list is not sharded)"); }
    if (!(m_targetNoise > 0.0)) { throw std::runtime_error("job: \"adaptive\" needs \"target_noise\""); }
    if (m_resume) { throw std::runtime_error("job: \"adaptive\" does not go with \"resume\": the state file holds neither squares nor counts"); }

    printf("Beginning pre-process...\n");
    preprocess(scene);
    printf("Pre-process complete (0.0s elapsed)\n");

    // sums, squares, counts and the list: four buffers on the device (a uint32 is held as the float of the same bits)
    float *buffers[4] = { nullptr, nullptr, nullptr, nullptr };
    struct Cleanup {
        Scene &scene;
        float *(&buffers)[4];
        ~Cleanup() { for (float *buffer : buffers) { if (buffer) { pathed_hip_accum_free(scene.handle(0), buffer); } } }
    } cleanup{ scene, buffers };
    const size_t sizes[4] = { floats, floats, pixels, pixels };
    for (int k = 0; k < 4; k++) {
        if (pathed_hip_accum_alloc(scene.handle(0), sizes[k], &buffers[k]) != PATHED_OK) { throw std::runtime_error(hipError("pathed_hip_accum_alloc")); }
    }
    float *deviceSums = buffers[0], *deviceSquares = buffers[1];
    uint32_t *deviceCounts = reinterpret_cast<uint32_t *>(buffers[2]), *deviceList = reinterpret_cast<uint32_t *>(buffers[3]);

    m_metrics = RenderMetrics();
    m_metrics.replicas = 1;
    m_metrics.replicaSeconds.assign(1, 0.0);
    m_metrics.collectedMoments = true;
    m_metrics.adaptive = true;
    m_metrics.width = width;
    m_metrics.height = height;
    const auto loopBegin = std::chrono::steady_clock::now();

    std::vector<float> radianceLookup(floats), squaresLookup(floats);
    std::vector<uint32_t> counts(pixels);
    // the files of one state: auto (sum / count), auto-stderr, auto-spp; numbered by the active pixels' count n
    auto publish = [&](int n, bool last) {
        const auto reduceBegin = std::chrono::steady_clock::now();
        if (pathed_hip_accum_download(scene.handle(0), deviceSums, floats, radianceLookup.data()) != PATHED_OK
            || pathed_hip_accum_download(scene.handle(0), deviceSquares, floats, squaresLookup.data()) != PATHED_OK
            || pathed_hip_accum_download(scene.handle(0), buffers[2], pixels, reinterpret_cast<float *>(counts.data())) != PATHED_OK) {
            throw std::runtime_error(hipError("pathed_hip_accum_download"));
        }
        m_metrics.reduceSeconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - reduceBegin).count();
        m_metrics.reduces++;
        const bool checkpoint = (n & (n - 1)) == 0 && !last;
        Image stderrImage(width, height, image.outputDirectory()), countImage(width, height, image.outputDirectory());
        stderrImage.setSpp(n);
        countImage.setSpp(n);
        {
            std::lock_guard<std::mutex> guard(image.getLock());
            image.setSpp(n);
            for (int row = 0; row < height; row++) {
                for (int col = 0; col < width; col++) {
                    const size_t pixel = (size_t)row * width + col, index = 3 * pixel;
                    const float samples = (float)counts[pixel], bessel = samples / (samples - 1.f);
                    float error[3];
                    for (int c = 0; c < 3; c++) {
                        const float mean = radianceLookup[index + c] / samples;
                        const float spread = squaresLookup[index + c] / samples - mean * mean;
                        const float variance = (spread > 0.f ? spread : 0.f) * bessel;
                        error[c] = counts[pixel] >= 2u ? std::sqrt(variance / samples) : 0.f;
                    }
                    image.set(row, col, radianceLookup[index + 0] / samples, radianceLookup[index + 1] / samples, radianceLookup[index + 2] / samples);
                    stderrImage.set(row, col, error[0], error[1], error[2]);
                    countImage.set(row, col, samples, samples, samples);
                }
            }
            if (checkpoint) { image.saveCheckpoint("auto"); } else { image.save("auto"); }
        }
        if (checkpoint) { stderrImage.saveCheckpoint("auto-stderr"); countImage.saveCheckpoint("auto-spp"); }
        else { stderrImage.save("auto-stderr"); countImage.save("auto-spp"); }
    };

    // 1. min(minSpp, spp) samples of every pixel
    int n = std::min(m_minSpp, m_spp);
    {
        const auto begin = std::chrono::steady_clock::now();
        for (int done = 0; done < n;) {
            const int count = std::min(m_sppPerLaunch, n - done);
            sampleImage(deviceSums, deviceSquares, scene, 0, (unsigned)done, (unsigned)count);
            done += count;
        }
        std::fill(counts.begin(), counts.end(), (uint32_t)n);
        if (pathed_hip_accum_upload(scene.handle(0), buffers[2], pixels, reinterpret_cast<const float *>(counts.data())) != PATHED_OK) {
            throw std::runtime_error(hipError("pathed_hip_accum_upload"));
        }
        m_metrics.replicaSeconds[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
        m_metrics.samplesRendered = (unsigned long long)n * pixels;
    }

    // 2., 3. the rounds
    for (;;) {
        PathedNoise figure;
        std::memset(&figure, 0, sizeof figure);
        figure.struct_size = sizeof figure;
        uint32_t listCount = 0;
        if (pathed_hip_select_pixels_device(scene.handle(0), deviceSums, deviceSquares, deviceCounts, (float)m_noiseFloor, (float)m_targetNoise,
                                            nullptr, deviceList, &listCount, &figure, nullptr) != PATHED_OK) {
            throw std::runtime_error(hipError("pathed_hip_select_pixels_device"));
        }
        m_metrics.noise.push_back({ n, figure.mean_error, figure.max_error });
        const bool stopping = quit && *quit;
        const bool last = listCount == 0 || n >= m_spp || stopping;
        publish(n, last);
        RenderStatus status;
        status.sample = n;
        status.elapsedSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopBegin).count();
        if (callback) { callback(status); }
        std::ostringstream line;
        line << "[" << m_logPrefix << "] sample: " << n << "/" << m_spp << std::fixed << std::setprecision(1) << " (" << status.elapsedSeconds
             << "s elapsed) noise: " << std::setprecision(6) << figure.mean_error << " active pixels: " << listCount << "/" << pixels;
        std::cout << line.str() << std::endl;
        if (last) {
            m_metrics.stoppedOnNoise = listCount == 0;
            break;
        }
        const int following = (int)std::min<long long>(2ll * n, (long long)m_spp);
        const auto begin = std::chrono::steady_clock::now();
        for (int done = n; done < following;) {
            const int count = std::min(m_sppPerLaunch, following - done);
            samplePixels(deviceSums, deviceSquares, deviceCounts, deviceList, listCount, scene, (unsigned)done, (unsigned)count);
            done += count;
        }
        m_metrics.replicaSeconds[0] += std::chrono::duration<double>(std::chrono::steady_clock::now() - begin).count();
        m_metrics.samplesRendered += (unsigned long long)(following - n) * listCount;
        m_metrics.adaptiveRounds++;
        n = following;
        postwave(scene, n);
    }
    m_metrics.uniformSpp = n;   // a uniform render that holds every pixel to the same criterion takes all of them to the largest count
    for (uint32_t count : counts) { if (count == (uint32_t)m_spp) { m_metrics.pixelsAtCap++; } }
    m_metrics.firstSample = 0;
    m_metrics.lastSample = n;
    m_metrics.loopSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopBegin).count();
}

void Integrator::setStateIdentity(const std::string &identity)
{
    unsigned long long hash = 1469598103934665603ull;   // FNV-1a
    for (unsigned char c : identity) { hash = (hash ^ c) * 1099511628211ull; }
    m_stateDigest = hash;
}

void Integrator::saveState(const std::vector<float> &sums, int width, int height, int done) const
{
    if (m_statePath.empty()) { return; }
    StateHeader header;
    std::memset(&header, 0, sizeof header);
    std::memcpy(header.magic, "PATHEDS3", 8);
    header.width = width;
    header.height = height;
    header.done = done;
    header.startBounce = stateStartBounce();
    header.lastBounce = stateLastBounce();
    header.seed = m_seed;
    header.jobDigest = m_stateDigest;
    // write beside, then rename: an interrupted write never leaves a truncated state behind
    const std::string scratch = m_statePath + ".tmp";
    {
        std::ofstream out(scratch, std::ios::binary | std::ios::trunc);
        out.write(reinterpret_cast<const char *>(&header), sizeof header);
        out.write(reinterpret_cast<const char *>(sums.data()), (std::streamsize)(sums.size() * sizeof(float)));
        if (!out) { fprintf(stderr, "pathed: cannot write %s\n", scratch.c_str()); return; }
    }
    if (std::rename(scratch.c_str(), m_statePath.c_str()) != 0) { fprintf(stderr, "pathed: cannot rename %s\n", scratch.c_str()); }
}

int Integrator::loadState(std::vector<float> &sums, int width, int height) const
{
    if (m_statePath.empty()) { return 0; }
    std::ifstream in(m_statePath, std::ios::binary);
    if (!in) { return 0; }   // nothing to resume from: start at sample 0
    StateHeader header;
    in.read(reinterpret_cast<char *>(&header), sizeof header);
    if (!in || std::memcmp(header.magic, "PATHEDS3", 8) != 0) { throw std::runtime_error("resume: " + m_statePath + " is not a pathed state file (of this version)"); }
    if (header.width != width || header.height != height) { throw std::runtime_error("resume: state file has another resolution"); }
    if (header.seed != m_seed || header.startBounce != stateStartBounce() || header.lastBounce != stateLastBounce()) {
        throw std::runtime_error("resume: state file was rendered with another seed or bounce window");
    }
    if (header.jobDigest != m_stateDigest) { throw std::runtime_error("resume: state file was rendered from another scene, integrator or job configuration"); }
    if (header.done < 0 || header.done > m_spp) { throw std::runtime_error("resume: state file holds more samples than the job asks for"); }
    in.read(reinterpret_cast<char *>(sums.data()), (std::streamsize)(sums.size() * sizeof(float)));
    if (!in) { throw std::runtime_error("resume: state file is truncated"); }
    return header.done;
}

void HipPathTracer::sampleImage(float *deviceSums, float *deviceSquares, Scene &scene, size_t replica, unsigned begin, unsigned count)
{
    if (pathed_hip_set_integrator(scene.handle(replica), m_integrator) != PATHED_OK) {
        throw std::runtime_error(std::string("pathed_hip_set_integrator: ") + pathed_hip_last_error());
    }
    if (deviceSquares) {
        const int code = pathed_hip_render_moments_device(
            scene.handle(replica), m_seed, begin, count,
            m_bounceController.startBounce(), m_bounceController.lastBounce(),
            deviceSums, deviceSquares, nullptr);
        if (code != PATHED_OK) {
            throw std::runtime_error(std::string("pathed_hip_render_moments_device: ") + pathed_hip_last_error());
        }
        return;
    }
    const int code = pathed_hip_render_device(
        scene.handle(replica), m_seed, begin, count,
        m_bounceController.startBounce(), m_bounceController.lastBounce(),
        deviceSums, nullptr, 1);
    if (code != PATHED_OK) {
        throw std::runtime_error(std::string("pathed_hip_render_device: ") + pathed_hip_last_error());
    }
}

void HipPathTracer::samplePixels(float *deviceSums, float *deviceSquares, uint32_t *deviceCounts, const uint32_t *deviceList, uint32_t listCount,
                                 Scene &scene, unsigned begin, unsigned count)
{
    if (pathed_hip_set_integrator(scene.handle(0), m_integrator) != PATHED_OK) {
        throw std::runtime_error(std::string("pathed_hip_set_integrator: ") + pathed_hip_last_error());
    }
    const int code = pathed_hip_render_pixels_device(
        scene.handle(0), m_seed, begin, count,
        m_bounceController.startBounce(), m_bounceController.lastBounce(),
        deviceList, listCount, deviceSums, deviceSquares, deviceCounts, nullptr);
    if (code != PATHED_OK) {
        throw std::runtime_error(std::string("pathed_hip_render_pixels_device: ") + pathed_hip_last_error());
    }
}

}  // namespace pathed
