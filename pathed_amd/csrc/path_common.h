// What the kernels that keep a whole path in registers have in common -- k_path_small and k_path_volume (kernels.h),
// k_path_wave (path_wave.h), k_path_hybrid (path_hybrid.h): the material table in LDS, the work units a persistent wave
// draws, the start of a camera sample, the vertex, the end of a sample.  One text each: that these kernels produce the same
// bits (tests/test_gpu_parity.py, test_gpu_wave.py, test_gpu_hybrid.py) follows from their running the same functions.
//
// Included by kernels.h inside namespace pathed, ahead of k_shade.

// The material table as a kernel reads it: staged into the block's LDS at `lds` (LDS_MATERIALS; ends with the block's
// barrier) or in HBM.
template <bool LDS_MATERIALS>
__device__ __forceinline__ MaterialAccess<LDS_MATERIALS> stageMaterials(const RenderParams &p, void *lds)
{
    MaterialAccess<LDS_MATERIALS> materials;
    if (LDS_MATERIALS) {
        // every lane indexes the parameters by its own hit
        const int words = p.scene.nMaterials * (int)(sizeof(DMaterial) / 4);
        const int *source = reinterpret_cast<const int *>(p.scene.materials);
        int *target = reinterpret_cast<int *>(lds);
        for (int i = threadIdx.x; i < words; i += kBlock) { target[i] = source[i]; }
        __syncthreads();
        materials.table = reinterpret_cast<const DMaterial *>(lds);
    } else {
        materials.table = p.scene.materials;
    }
    return materials;
}

// The scene as the traversal sees it; `tree` false: the all-triangles kernel, which walks no nodes.
__device__ __forceinline__ TraceGeometry sceneGeometry(const DScene &scene, bool tree)
{
    TraceGeometry geometry;
    geometry.nodes = tree ? scene.nodes : nullptr;
    geometry.tris = scene.leafTris;
    geometry.nNodes = tree ? scene.nNodes : 0;
    geometry.nTris = scene.nTris;
    geometry.spheres = scene.spheres;
    geometry.nSpheres = scene.nLinearSpheres;
    return geometry;
}

// Work units: the wave reserves p.unitGrab consecutive units of a queue at a time (one wave-level atomic on a sharded
// cursor; a wave whose queue is dealt out moves on to the next).  Wave-uniform state.
struct UnitTaker {
    unsigned int queue, queuesTried;
    unsigned int reservedNext, reservedEnd;

    __device__ __forceinline__ UnitTaker(const RenderParams &p, unsigned int waveId)
        : queue(waveId % (unsigned int)p.nQueues), queuesTried(0), reservedNext(0), reservedEnd(0) {}

    // hands a unit to every lane that wants one, in lane order; 0xFFFFFFFF once the pass is dealt out
    __device__ __forceinline__ unsigned int take(const RenderParams &p, int lane, bool want)
    {
        unsigned int mine = 0xFFFFFFFFu;
        unsigned long long wanting = __ballot(want);
        while (wanting != 0ull) {
            if (reservedNext == reservedEnd) {
                if (queuesTried >= (unsigned int)p.nQueues) { break; }   // every queue is dealt out
                unsigned int ticket = 0;
                if (lane == 0) { ticket = atomicAdd(&p.counters[kCtrUnitCursor + queue * kCursorStride], (unsigned int)p.unitGrab); }
                ticket = (unsigned int)__builtin_amdgcn_readfirstlane((int)ticket);
                const unsigned int limit = p.queueUnits[queue];   // unit ids of queue q: q * unitsPerQueue + [0, limit)
                if (ticket >= limit) {
                    queue = (queue + 1u) % (unsigned int)p.nQueues;
                    queuesTried++;
                    continue;
                }
                reservedNext = ticket;
                reservedEnd = ticket + (unsigned int)p.unitGrab < limit ? ticket + (unsigned int)p.unitGrab : limit;
            }
            const unsigned int available = reservedEnd - reservedNext;
            const unsigned int rank = laneRank(wanting);
            const bool served = ((wanting >> lane) & 1ull) != 0ull && rank < available;
            if (served) { mine = queue * p.unitsPerQueue + reservedNext + rank; }
            const unsigned int count = (unsigned int)__popcll(wanting);
            reservedNext += count < available ? count : available;
            wanting &= ~__ballot(served);
        }
        return mine;
    }
};

struct PathRegisters {
    V3 o, d;                         // the ray in flight (the one whose hit the next vertex shades)
    int st;                          // device_scene.h state word: vertex that spawned the ray + eligible / delta / continue
    int firstEmitMaterial;
    Rgb result, modulation, throughput, pend;
    float bsdfPdf, cosTheta;
    Rng random;
};

// what a path carries before its camera ray's vertex
__device__ __forceinline__ void resetPath(PathRegisters &path)
{
    path.st = 0;
    path.firstEmitMaterial = -1;
    path.result = rgb(0.f);
    path.modulation = rgb(1.f);
    path.throughput = rgb(0.f);
    path.pend = rgb(0.f);
    path.bsdfPdf = 1.f;
    path.cosTheta = 0.f;
}

// a lane without a sample
__device__ __forceinline__ PathRegisters idlePath()
{
    PathRegisters path;
    path.random.k0 = 0u; path.random.k1 = 0u; path.random.dimension = 0u;
    path.o = v3(0.f, 0.f, 0.f); path.d = v3(0.f, 0.f, 1.f);
    resetPath(path);
    return path;
}

// Camera::generateRay(int,int) for (pixel, sample), src/camera.cpp:49-55, with the sample's random stream
__device__ __forceinline__ void cameraSampleRay(const RenderParams &p, uint64_t seed, uint32_t pixel, uint32_t sample, Rng &random, V3 *origin, V3 *direction)
{
    makeKey(seed, pixel, sample, &random.k0, &random.k1);
    random.dimension = 0;
    const int width = p.scene.camera.resX;
    const int row = (int)fastDivide((unsigned int)pixel, p.divWidth);   // pixel / width, exactly
    const int col = (int)pixel - row * width;
    const float jitterX = random.next() - 0.5f;
    const float jitterY = random.next() - 0.5f;
    cameraRay(p.scene.camera, row + jitterY, col + jitterX, origin, direction);
}

__device__ __forceinline__ void startCameraSample(const RenderParams &p, uint64_t seed, uint32_t pixel, uint32_t sample, PathRegisters &path)
{
    cameraSampleRay(p, seed, pixel, sample, path.random, &path.o, &path.d);
    resetPath(path);
}

// One vertex of one path: SampleIntegrator::samplePixel / PathTracer::L on register state.  `h` is the hit of the ray
// (path.o, path.d).  Returns true when the sample is finished (*color is its value); otherwise path.o / path.d hold the next
// ray and *shadowOut the vertex's occlusion query, if any.  PROBES: the lane-utilisation counters of profile builds
// (tools/fused_profile.py; k_path_wave and k_path_hybrid keep their own cycle counters in the same words).
// The remaining copies of this text are k_shade, k_shade_env and the kernels of kernels_experiments.h: they work on path
// state in HBM, interleave its loads with the arithmetic and differ in what an ENV_ONLY scene lets them drop, and k_shade
// sits one register under a budget whose loss costs 6-8 % (tests/test_kernel_resources.py).
//
// The vertex has two halves.  pathArrive: the ray reaches its hit -- the MIS term of the BSDF sample that sent it, then
// termination; of the hit it reads the material, the shading normal and the point, never the frame.  pathDepart: the new
// vertex -- the camera ray's own bookkeeping, the BSDF sample, the light sample.  k_path_small hands a finished lane its next
// sample's camera hit between the two (kernels.h: the camera queue), so that the lane departs in the same iteration; the
// other kernels run them back to back on one Isect (pathVertex).

// what a camera ray that leaves the scene is worth: SampleIntegrator::samplePixel, src/sample_integrator.cpp:18-59
template <typename TRAITS>
__device__ __forceinline__ Rgb cameraMissColor(const DScene &scene, V3 direction)
{
    return rgb(0.f) + environmentL<TRAITS>(scene, direction);
}

// `isect`: makeIsect of the hit (anything where `miss`).  Returns true when the sample is finished (*color is its value).
template <typename TRAITS, bool PROBES = false, typename MATERIALS>
__device__ __forceinline__ bool pathArrive(const RenderParams &p, const DScene &scene, const MATERIALS &materials, PathRegisters &path, const Isect &isect,
                                           bool miss, Rgb *color)
{
    bool finished = false;
    *color = rgb(0.f);
    const int st = path.st;
    const int rayBounce = st & kStBounceMask;  // vertex that spawned this ray, 0 = camera
    if (rayBounce == 0) {
        if (miss) {
            *color = cameraMissColor<TRAITS>(scene, path.d);
            finished = true;
        }
    } else {
        // the ray left vertex `rayBounce` along its BSDF sample
        if (st & kStEligible) {
            // PathTracer::directSampleBSDF, src/path_tracer.cpp:167-216
            Rgb bsdfTerm = rgb(0.f);
            if (!miss) {
                const Rgb emit = matEmit(materials[isect.material]);
                if (PROBES) { SHADE_REGION(5, !isBlack(emit) && dot(isect.wo, isect.shadingNormal) >= 0.f); }   // BSDF sample met an emitter: lightsPDF
                if (!isBlack(emit) && dot(isect.wo, isect.shadingNormal) >= 0.f) {
                    const float lightPDF = lightsPDF<TRAITS>(scene, path.o, isect);
                    const float brdfWeight = (st & kStDelta)
                        ? 1.f
                        : (1 * path.bsdfPdf) / (1 * path.bsdfPdf + 1 * lightPDF);
                    bsdfTerm = emit * brdfWeight * path.throughput * path.cosTheta / path.bsdfPdf;
                }
            } else {
                const Rgb environmentLight = environmentL<TRAITS>(scene, path.d);
                if (TRAITS::env && !isBlack(environmentLight)) {
                    // Scene::environmentPDF, src/scene.cpp:494-502
                    const float lightPDF = envEmitPDF(scene.env, path.d) / scene.nLights;
                    const float brdfWeight = (st & kStDelta)
                        ? 1.f
                        : (1 * path.bsdfPdf) / (1 * path.bsdfPdf + 1 * lightPDF);
                    bsdfTerm = environmentLight * brdfWeight * path.throughput * path.cosTheta / path.bsdfPdf;
                }
            }
            const Rgb Ld = path.pend + bsdfTerm;
            if (rayBounce == 1) { path.result = Ld; }
            else { path.result = path.result + Ld * path.modulation; }
        }

        // PathTracer::L loop body, src/path_tracer.cpp:41-58
        if (!(st & kStContinue) || miss) {
            finished = true;
        } else {
            const float invPDF = 1.f / path.bsdfPdf;
            path.modulation = path.modulation * (path.throughput * path.cosTheta * invPDF);
            if (isBlack(path.modulation)) { finished = true; }
        }
        if (finished) {
            Rgb first = rgb(0.f);
            if (path.firstEmitMaterial >= 0) { first = first + matEmit(materials[path.firstEmitMaterial]); }
            *color = first + path.result;
        }
    }
    return finished;
}

// The vertex at `isect` (makeIsect of the hit of (path.o, path.d)) of a path that pathArrive did not finish.  Returns true
// when the sample is finished here (*color is its value); otherwise path.o / path.d hold the next ray and *shadowOut the
// vertex's occlusion query, if any.
// KEYED (k_path_small_single): the vertex's numbers come from keyRow, the filled row of (path.random.k1, this vertex)
// (shading.h: fillKeyRow) -- Rng::next()'s bits with the inner mixer taken from the row.
template <typename TRAITS, bool PROBES = false, bool KEYED = false, typename MATERIALS>
__device__ __forceinline__ bool pathDepart(const RenderParams &p, const DScene &scene, const MATERIALS &materials, PathRegisters &path,
                                           Isect &isect, ShadowRequest *shadowOut, Rgb *color, const uint32_t *keyRow = nullptr)
{
    ShadowRequest shadow;
    shadow.push = false;
    shadow.origin = v3(0.f, 0.f, 0.f);
    shadow.direction = v3(0.f, 0.f, 1.f);
    shadow.tfar = 0.f;
    bool finished = false;
    *color = rgb(0.f);
    const int rayBounce = path.st & kStBounceMask;
    const int vertex = rayBounce + 1;

    if (PROBES) { SHADE_REGION(4, rayBounce == 0); }   // camera-ray vertex
    if (rayBounce == 0) {
        // SampleIntegrator::samplePixel, src/sample_integrator.cpp:18-59
        path.firstEmitMaterial = -1;
        if (checkCounts(p.startBounce, p.lastBounce, 0)) {
            const Rgb emit = matEmit(materials[isect.material]);
            const bool backside = dot(isect.normal, isect.wo) < 0.f;
            if (!isBlack(emit) && !backside) { path.firstEmitMaterial = isect.material; }
        }
        path.result = rgb(0.f);
    }

    {
        // PathTracer::L: sample the BSDF, then direct(), src/path_tracer.cpp:30-36, 60-73
        const DMaterial &material = materials[isect.material];
        prepareLobes<TRAITS>(material, isect);

        path.random.dimension = vertexBase(vertex);
        const auto sampleBsdf = [&]() -> BSDFSample {
            if constexpr (KEYED) {
                RowRng rowRandom;
                rowRandom.k0 = path.random.k0; rowRandom.row = keyRow; rowRandom.dimension = 0u;
                return materialSample<TRAITS>(material, isect, rowRandom);
            } else {
                return materialSample<TRAITS>(material, isect, path.random);
            }
        };
        const BSDFSample bsdfSample = sampleBsdf();

        const bool counts = checkCounts(p.startBounce, p.lastBounce, vertex);
        const bool emissive = !isBlack(matEmit(material));
        const bool wantDirect = counts && !emissive;  // direct() returns 0 on emitters (:86-90)
        const bool wantContinue = !checkDone(p.lastBounce, vertex + 1);

        Rgb lightTerm = rgb(0.f);
        if (PROBES) { SHADE_REGION(7, wantDirect); }   // light sampling
        if (wantDirect) {
            path.random.dimension = vertexBase(vertex) + 3;
            if constexpr (KEYED) {
                RowRng rowRandom;
                rowRandom.k0 = path.random.k0; rowRandom.row = keyRow; rowRandom.dimension = 3u;
                lightTerm = sampleLightsTerm<false, TRAITS>(scene, materials, isect, material, rowRandom, &shadow);
            } else {
                lightTerm = sampleLightsTerm<false, TRAITS>(scene, materials, isect, material, path.random, &shadow);
            }
        }

        // see k_shade: a vertex with nothing pending whose BSDF sample has exactly black throughput ends the sample
        const bool deadEnd = isBlack(bsdfSample.throughput) && bsdfSample.pdf > 0.f && bsdfSample.pdf < 3e38f
            && !shadow.push && isBlack(lightTerm);
        if ((!wantDirect && !wantContinue) || deadEnd) {
            finished = true;
            Rgb first = rgb(0.f);
            if (path.firstEmitMaterial >= 0) { first = first + matEmit(materials[path.firstEmitMaterial]); }
            *color = first + path.result;
            shadow.push = false;
        } else {
            int nextState = vertex;
            if (wantDirect) { nextState |= kStEligible; }
            if (isDeltaT<TRAITS>(material)) { nextState |= kStDelta; }
            if (wantContinue) { nextState |= kStContinue; }
            path.st = nextState;
            path.o = isect.point;
            path.d = bsdfSample.wiWorld;
            path.bsdfPdf = bsdfSample.pdf;
            path.throughput = bsdfSample.throughput;
            path.cosTheta = fabsf(dot(isect.shadingNormal, bsdfSample.wiWorld));
            path.pend = lightTerm;
        }
    }
    *shadowOut = shadow;
    return finished;
}

// Both halves on one hit: `h` is the hit of the ray (path.o, path.d).
template <typename TRAITS, typename MATERIALS>
__device__ __forceinline__ bool pathVertex(const RenderParams &p, const DScene &scene, const MATERIALS &materials, PathRegisters &path,
                                           float4 h, ShadowRequest *shadowOut, Rgb *color)
{
    const bool miss = floatAsInt(h.w) < 0;
    Isect isect;
    if (!miss) { isect = makeIsect<TRAITS>(scene, path.o, path.d, h); }
    shadowOut->push = false;
    shadowOut->origin = v3(0.f, 0.f, 0.f);
    shadowOut->direction = v3(0.f, 0.f, 1.f);
    shadowOut->tfar = 0.f;
    if (pathArrive<TRAITS>(p, scene, materials, path, isect, miss, color)) { return true; }
    return pathDepart<TRAITS>(p, scene, materials, path, isect, shadowOut, color);
}

// The lanes of a fresh wave take their first units.
__device__ __forceinline__ void firstUnits(const RenderParams &p, UnitTaker &units, int lane, unsigned int &unit,
                                           uint32_t &pixel, uint32_t &sample, uint32_t &endSample, bool &alive, bool &startNext)
{
    unit = units.take(p, lane, true);
    if (unit != 0xFFFFFFFFu) {
        unitSamples(p, unit, &pixel, &sample, &endSample);
        alive = true;
        startNext = true;
    }
}

// End of a sample on the lanes where `done`: radianceLookup += color (src/sample_integrator.cpp:61-63; non-finite samples
// dropped); where that was the unit's last sample its partial sum goes out.  Returns true where the unit is finished.
// unitIsIndex: every unit is one sample and `unit` already holds its partialIndex (k_path_small's camera queue).
__device__ __forceinline__ bool putSampleAway(const RenderParams &p, bool unitIsIndex, bool done, Rgb color, float4 &partial, unsigned int unit,
                                              uint32_t &sample, uint32_t endSample)
{
    bool unitDone = false;
    if (done) {
        const bool finite = isfinite(color.r) && isfinite(color.g) && isfinite(color.b);
        if (finite) {
            partial.x += color.r;
            partial.y += color.g;
            partial.z += color.b;
        } else {
            atomicAdd(&p.stats[kStatDropped], 1ull);
        }
        sample++;
        if (sample >= endSample) {
            p.state.chunkBuf[unitIsIndex ? (size_t)unit : partialIndex(p, unit)] = partial;
            partial = make_float4(0.f, 0.f, 0.f, 0.f);
            unitDone = true;
        }
    }
    return unitDone;
}

// The same where every unit is ONE sample (k_path_small_single): the end of a sample is the end of its unit, whose partial sum
// is putSampleAway's 0.f + colour per channel (a -0 becomes +0), zeros for a dropped sample.  `index`: the unit's partialIndex.
__device__ __forceinline__ void putUnitAway(const RenderParams &p, bool done, Rgb color, unsigned int index)
{
    if (done) {
        float4 partial = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool finite = isfinite(color.r) && isfinite(color.g) && isfinite(color.b);
        if (finite) {
            partial.x += color.r;
            partial.y += color.g;
            partial.z += color.b;
        } else {
            atomicAdd(&p.stats[kStatDropped], 1ull);
        }
        p.state.chunkBuf[(size_t)index] = partial;
    }
}

// ... then the unit's next sample (startNext), or the lane takes the next unit; a lane that gets none retires (alive).
__device__ __forceinline__ void finishSample(const RenderParams &p, UnitTaker &units, int lane, bool done, Rgb color, float4 &partial,
                                             unsigned int &unit, uint32_t &pixel, uint32_t &sample, uint32_t &endSample, bool &alive, bool &startNext)
{
    const bool needUnit = putSampleAway(p, false, done, color, partial, unit, sample, endSample);
    if (done && !needUnit) { startNext = true; }
    if (__ballot(needUnit) != 0ull) {
        const unsigned int newUnit = units.take(p, lane, needUnit);
        if (needUnit) {
            unit = newUnit;
            if (newUnit != 0xFFFFFFFFu) {
                unitSamples(p, newUnit, &pixel, &sample, &endSample);
                startNext = true;
            } else {
                alive = false;
            }
        }
    }
}
