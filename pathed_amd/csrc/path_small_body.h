// The body of the fused path kernel (kernels.h: k_path_small and k_path_small_single), included into both: the text stands
// between the braces of a __global__ function whose scope names LDS_MATERIALS, COUNT, TRAITS, MFMA, QUADS and SINGLE (compile-
// time) and the arguments p (RenderParams) and smallTris (SmallTris).
// Why an include and not a __forceinline__ template called by both: the call changes what the existing instantiations
// compile to.  With the body in a function, unchanged, 17 of the 20 instantiations of k_path_small changed their
// kernel-resource-usage (the Cornell-like one 127 -> 128 VGPRs and 84 -> 60 bytes of scratch, the rough rungs 108 / 104 ->
// 84 / 92), whether the function took its arguments by reference or by value (profiles/single_sample_profile.log); included,
// all 20 compile to what they were.
//
// SINGLE: every unit of the launch is ONE sample (p.chunk == 1, the library's default): the body of k_path_small_single.
// A lane then carries no pixel, no sample range, no partial sum and never starts a sample in place: `unit` is the index of
// the unit's partial sum, which is 0.f + the sample's colour.  A camera ray that leaves the scene ends its sample in the
// refill, at full width, so every queue entry is a hit and the hand-over between samples is straight-line: put away, one
// pop by ballot rank.  The same integers and floats in the same order as SINGLE = false on such a launch.
    static_assert(!SINGLE || (QUADS && !COUNT && !MFMA), "the single-sample body exists for the headline instantiation");
    extern __shared__ float4 ldsDynamic[];           // LDS_MATERIALS: the material table, nMaterials x 96 B
    __shared__ float mfmaRows[MFMA ? kMfmaTableFloats : 1];
    // QUADS: what a lane's path carries across the pass over the triangles and does not use in it waits in LDS, 96 bytes per
    // lane ([quad][thread]: a wave stores 1 KiB contiguous): the parallelogram test needs two dozen registers more than the
    // pair-of-triangles test, and what the compiler spilled for them went to scratch memory (48 dwords, profiles/r4_ab_quads.log)
    // (SINGLE: 64 bytes per lane, four rows: no partial sum, no sample range, and `unit` travels in the slot of
    // random.dimension, which pathDepart sets before any draw)
    constexpr int kStashRows = SINGLE ? 4 : 6;
    constexpr int kStashKeyRow = SINGLE ? 3 : 5;
    __shared__ float4 stashRows[QUADS ? kStashRows * kBlock : 1];
    // ... and phase 2 shares the wave's candidates out (smallResolveShared): 2.25 KiB per wave.  With the stash 33.5 KiB per
    // block: four blocks per CU as long as the material table stays below 6.5 KiB (pathed_hip.hip pairs triangles up to 64 materials)
    constexpr int kResolveCapacity = PATHED_RESOLVE_SHARED == 2 ? 128 : 64;   // items per wave
    __shared__ unsigned long long resolveBest[QUADS ? kBlock : 1];
    __shared__ float2 resolveUv[QUADS ? kWavesPerBlock * kResolveCapacity : 1];
    __shared__ unsigned short resolveItems[QUADS ? kWavesPerBlock * kResolveCapacity : 1];
    __shared__ unsigned int resolveOccluded[QUADS ? kBlock : 1], resolveCount[QUADS ? kWavesPerBlock : 1];
    // SINGLE: the inner keys of the random stream (shading.h: KeySlots, fillKeyRow): per wave two tables of kKeyVertices rows,
    // 768 bytes, out of what the two stash rows gave back.  A row is two aligned 16-byte reads.  Only the wave touches its
    // tables, and LDS serves a wave's accesses in order.
    __shared__ uint4 keyRows[SINGLE ? kWavesPerBlock * 2 * kKeyTableWords / 4 : 1];
    if (MFMA) {
        for (int i = threadIdx.x; i < kMfmaTableFloats; i += kBlock) { mfmaRows[i] = p.mfmaTable[i]; }
        if (!LDS_MATERIALS) { __syncthreads(); }
    }
    const MaterialAccess<LDS_MATERIALS> materials = stageMaterials<LDS_MATERIALS>(p, ldsDynamic);
    const TraceGeometry geometry = sceneGeometry(p.scene, false);

    const DScene &scene = p.scene;
    const int lane = threadIdx.x & 63;
    const unsigned int waveId = blockIdx.x * kWavesPerBlock + (unsigned int)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform, and known to be)
    const int nTris = p.scene.nTris;
    // kSmallPassList: phase 2 of the pass over all items indexes the pass list's triangles, which follow the scene's nTris
    // item-ordered ones; the refill's candidates come from the camera masks, in the FULL item order, and keep `geometry`
    // (a second wave-uniform pointer: scalar registers only)
    constexpr bool kPassList = QUADS && kSmallPassList<COUNT, MFMA, TRAITS>;
    TraceGeometry passGeometry = geometry;
    if (kPassList) { passGeometry.tris = geometry.tris + 3 * nTris; }
    const uint64_t seed = ((uint64_t)p.seedHi << 32) | p.seedLo;
    UnitTaker units(p, waveId);

    // ---- the path a lane carries
    bool alive = true;               // the lane has a sample or may still get one
    bool needEntry = true;           // ... it has none: it takes the next entry of the camera queue
    unsigned int unit = 0xFFFFFFFFu; // the unit in flight; where a unit is one sample (singleSample), its partial sum's index
    uint32_t pixel = 0, sample = 0, endSample = 0;   // sample: absolute index of the sample in flight
    PathRegisters path = idlePath();
    float4 partial = make_float4(0.f, 0.f, 0.f, 0.f);
    bool pendingShadow = false;      // the vertex the ray left asked for an occlusion query along shadowDirection
    V3 shadowDirection = v3(0.f, 0.f, 1.f);
    float shadowTfar = 0.f;

    unsigned int closestRays = 0, shadowRays = 0, trisTested = 0;

    // ---- the wave's camera queue: a ring of kCameraQueueEntries started samples in HBM, three float4 each ([part][entry]):
    // (direction, t), (u, v, prim, unit or partial index), (k0, k1 of the sample's random stream).  A camera ray's hit depends
    // on (pixel, sample) alone, so the wave starts 64 units at a time at full width -- unit bookkeeping, key, camera ray, the
    // pixel's candidate mask (the counting instantiations: a primary-ray-only pass over the triangles), phase 2 -- ahead of
    // need, and a lane whose sample ended takes a finished camera hit instead of starting a ray a sixth of a wave wide.  Only
    // this wave touches its entries: a workgroup-scope fence after the writes and before the reads orders them.  Head, count
    // and unitsLeft are wave-uniform.
    float4 *const cameraQueue = p.cameraQueue + (size_t)waveId * kCameraQueueWords;
    unsigned int queueHead = 0u, queueCount = 0u;
    bool unitsLeft = true;           // UnitTaker::take has not yet come back short
    const bool singleSample = SINGLE || p.chunk == 1;   // every unit is one sample: no lane ever needs the unit's pixel again

    // a unit's later samples (set_samples_per_unit > 1) start in place, in order: one inlined copy of the camera ray
    bool startNext = false;

    KeySlots keySlots;   // (wave-uniform) which second keys the wave's two tables hold
    keySlots.clear();
    uint4 *const keyTables = keyRows + (SINGLE ? (threadIdx.x >> 6) * 2 * (kKeyTableWords / 4) : 0);

    while (true) {
        SHADE_REGION(0, alive && !needEntry);   // (profile builds, tools/fused_profile.py) iterations / lanes with a sample in flight
        SHADE_REGION(1, startNext);    // camera ray started in place
        if (!SINGLE && startNext) {
            startCameraSample(p, seed, pixel, sample, path);
            startNext = false;
        }

        // ---- the path's ray (Scene::testIntersect's rtcIntersect1) and, from the same point, the shadow ray of the
        // vertex it leaves (Scene::testOcclusion's rtcOccluded1): an occluded light sample contributes nothing
        if (QUADS) {
            float4 *stash = stashRows + threadIdx.x;
            stash[0 * kBlock] = make_float4(path.result.r, path.result.g, path.result.b, path.bsdfPdf);
            stash[1 * kBlock] = make_float4(path.modulation.r, path.modulation.g, path.modulation.b, path.cosTheta);
            stash[2 * kBlock] = make_float4(path.throughput.r, path.throughput.g, path.throughput.b, intAsFloat(path.st));
            if (!SINGLE) {
                stash[3 * kBlock] = partial;
                stash[4 * kBlock] = make_float4(intAsFloat((int)pixel), intAsFloat((int)sample), intAsFloat((int)endSample), intAsFloat((int)unit));
            }
            stash[kStashKeyRow * kBlock] = make_float4(intAsFloat((int)path.random.k0), intAsFloat((int)path.random.k1), intAsFloat(path.firstEmitMaterial),
                                                       intAsFloat((int)(SINGLE ? unit : path.random.dimension)));
            asm volatile("" ::: "memory");   // the values below are re-read from LDS: the registers are free for the pass
        }

        // ---- refill (QUADS: inside the stash window, the path state is out of the way): fewer than a wave's worth of entries
        // and units left: every lane starts one unit's first sample.  Phase 2 accepts by an order-independent rule, so the hit
        // is the one the pair pass below would give this ray.
        if (queueCount < 64u && unitsLeft) {
            const unsigned int newUnit = units.take(p, lane, true);
            const bool got = newUnit != 0xFFFFFFFFu;
            const unsigned long long gotMask = __ballot(got);
            SHADE_REGION(11, got);   // refill batches / their width
            if (gotMask != ~0ull) { unitsLeft = false; }
            Rng cameraRandom;
            cameraRandom.k0 = 0u; cameraRandom.k1 = 0u; cameraRandom.dimension = 0u;
            V3 cameraO = v3(0.f, 0.f, 0.f), cameraD = v3(0.f, 0.f, 1.f);
            // The candidates of a camera ray come from the pixel's mask (camera_masks.h: every triangle a ray through the pixel's
            // footprint can meet; 8 bytes per lane, a batch of the default unit order reads 64 consecutive pixels), not from a pass
            // over the records.  The counting instantiations keep that pass: their counts stay the per-slot path's, and the
            // library carries a reference for the masks inside itself (GPU test: the two render the same bytes).
            constexpr bool kMasks = !COUNT && !MFMA;
            uint32_t unitPixel = 0u;
            if (got) {
                uint32_t unitFirst, unitEnd;
                unitSamples(p, newUnit, &unitPixel, &unitFirst, &unitEnd);
                cameraSampleRay(p, seed, unitPixel, unitFirst, cameraRandom, &cameraO, &cameraD);
            }
            if (SINGLE && gotMask != 0ull) {
                // The batch's second key: in the default unit order one for the whole batch, otherwise that of its first unit
                // (the lanes that hold another fill their own rows).  A key in neither table takes the older one's place:
                // 96 inner keys, two full-width turns.
                const int firstLane = __builtin_amdgcn_readfirstlane(__ffsll((long long)gotMask) - 1);
                const uint32_t batchK1 = (uint32_t)__builtin_amdgcn_readlane((int)cameraRandom.k1, firstLane);
                if (keySlots.find(batchK1) < 0) {
                    uint32_t *table = reinterpret_cast<uint32_t *>(keyTables + keySlots.claim(batchK1) * (kKeyTableWords / 4));
                    table[lane] = innerKey(batchK1, vertexBase(1) + (uint32_t)lane);
                    if (lane < kKeyTableWords - 64) { table[64 + lane] = innerKey(batchK1, vertexBase(1) + 64u + (uint32_t)lane); }
                }
            }
            LaneRay cameraHit;
            laneRayInit(cameraHit, cameraO, cameraD, PATHED_TNEAR, PATHED_TFAR, false);
            unsigned int candidatesLow = 0, candidatesHigh = 0;
            if (kMasks) {
                if (got) {
                    const unsigned long long pixelCandidates = cameraMasks(p)[unitPixel];
                    candidatesLow = (unsigned int)(pixelCandidates >> 32);
                    candidatesHigh = (unsigned int)pixelCandidates;
                }
            } else if (got) {
                if (QUADS || MFMA) {
                    unsigned int unusedLow = 0, unusedHigh = 0;
                    smallCandidatesItems<false, true, true>(smallTris.data, p.smallQuads, nTris, p.smallKappaT, cameraO, cameraD, cameraD,
                                                             &candidatesLow, &candidatesHigh, &unusedLow, &unusedHigh, candidateNear(PATHED_TNEAR), 0.f);
                } else {
                    smallCandidates(smallTris.data, nTris, cameraO, cameraD, &candidatesLow, &candidatesHigh, candidateNear(PATHED_TNEAR));
                }
            }
            if (COUNT && got) {
                trisTested += (unsigned int)nTris;
                closestRays++;
            }
            smallResolve(geometry, cameraHit, candidatesLow, candidatesHigh);
            if (got) { finishRay(geometry, cameraHit); }
            // SINGLE: a camera ray that left the scene ends its sample -- and with it its unit -- here, at full width; only the
            // hits are queued
            const bool left = SINGLE && got && cameraHit.bestPrim < 0;
            const unsigned long long queuedMask = SINGLE ? __ballot(got && !left) : gotMask;
            SHADE_REGION(8, left);
            if (got) {
                const unsigned int slot = (queueHead + queueCount + laneRank(queuedMask)) & (kCameraQueueEntries - 1u);
                // where a unit has several samples the lane needs the unit itself: its pixel and its samples
                const unsigned int target = singleSample ? (unsigned int)partialIndex(p, newUnit) : newUnit;
                if (left) {
                    putUnitAway(p, true, cameraMissColor<TRAITS>(scene, cameraD), target);
                } else {
                    cameraQueue[0 * kCameraQueueEntries + slot] = make_float4(cameraD.x, cameraD.y, cameraD.z, cameraHit.best);
                    cameraQueue[1 * kCameraQueueEntries + slot] = make_float4(cameraHit.bestU, cameraHit.bestV, intAsFloat(cameraHit.bestPrim), intAsFloat((int)target));
                    cameraQueue[2 * kCameraQueueEntries + slot] = make_float4(intAsFloat((int)cameraRandom.k0), intAsFloat((int)cameraRandom.k1), 0.f, 0.f);
                }
            }
            queueCount += (unsigned int)__popcll(queuedMask);
            __threadfence_block();   // (release) the entries are written before any lane of the wave reads them
        }

        const bool tracing = alive && !needEntry;   // the lane has a ray in flight
        LaneRay ray;
        laneRayInit(ray, path.o, path.d, PATHED_TNEAR, PATHED_TFAR, false);
        {
            const bool traceShadow = tracing && pendingShadow;
            LaneRay shadowRay;
            laneRayInit(shadowRay, path.o, shadowDirection, PATHED_TNEAR, shadowTfar, true);
            unsigned int candidatesLow = 0, candidatesHigh = 0, shadowLow = 0, shadowHigh = 0;
            SHADE_REGION(2, traceShadow);   // passes that carry shadow rays / lanes with one
            if (MFMA) {
                // every lane takes part (the matrix instructions are the wave's); words: even / odd triangles
                mfmaCandidatesPair(mfmaRows, nTris, p.mfmaFrame, __ballot(traceShadow) != 0ull, path.o, path.d, shadowDirection,
                                   candidateNear(PATHED_TNEAR), candidateFar(shadowTfar), &candidatesLow, &candidatesHigh, &shadowLow, &shadowHigh);
                if (!tracing) { candidatesLow = 0u; candidatesHigh = 0u; }
                if (!traceShadow) { shadowLow = 0u; shadowHigh = 0u; }
            } else if (QUADS) {
                // one instantiation of the pass: a wave without a single shadow ray is rare (3 % of the passes) and pays for
                // the second ray's arithmetic rather than for a second copy of the loop's registers
                if (tracing) {
                    // The shadow ray leaves out the never-occluders' turns (smallCandidatesItems<PRUNE>) in the Cornell-like
                    // instantiation, the headline's: its launch alone carries the turn counts in the upper half of smallQuads
                    // (kSmallPrunes, pathed_hip.hip: renderPassFused).  The counting instantiations run every turn for both rays:
                    // the library's own reference for the pruning.  The others compile as before.  Veach-like: pruned it LOST
                    // 0.45 % on the Veach scene, which has no never-occluder to skip (7 408.7 -> 7 375.1 Msamples/s,
                    // profiles/shadow_prune_profile.log).  The ladder's rungs and the any-BSDF instantiation: pruned, the latter's
                    // scratch fell from 112 to 84 / 64 bytes per lane while a rung kept 104, and tests/test_kernel_resources.py
                    // holds the rungs to no more than the instantiation they stand in for.
                    // The same instantiation walks the PASS LIST (kSmallPassList; small_items.h: NEVER-HIT): smallTris holds its
                    // records and the low half of smallQuads its two counts.  The count the bits are shifted by is the pass
                    // list's; nTris, the scene's, still numbers the sphere primitives (geometry.nTris + k).
                    constexpr bool kPrune = kSmallPrunes<COUNT, TRAITS>;
                    const int smallQuads = kPassList ? (p.smallQuads & 0xFF) : kPrune ? (p.smallQuads & 0xFFFF) : p.smallQuads;
                    const int passTris = kPassList ? ((p.smallQuads >> 8) & 0xFF) : nTris;
                    smallCandidatesItems<true, true, true, kPrune>(smallTris.data, smallQuads, passTris, p.smallKappaT, path.o, path.d, shadowDirection,
                                                                   &candidatesLow, &candidatesHigh, &shadowLow, &shadowHigh,
                                                                   candidateNear(PATHED_TNEAR), candidateFar(shadowTfar),
                                                                   (p.smallQuads >> 16) & 0xFF, (p.smallQuads >> 24) & 0xFF);
                    if (!traceShadow) { shadowLow = 0u; shadowHigh = 0u; }
                }
            } else if (__ballot(traceShadow) != 0ull) {
                if (tracing) {
                    smallCandidatesPair(smallTris.data, nTris, path.o, path.d, shadowDirection, &candidatesLow, &candidatesHigh, &shadowLow, &shadowHigh,
                                        candidateNear(PATHED_TNEAR), candidateFar(shadowTfar));
                    if (!traceShadow) { shadowLow = 0u; shadowHigh = 0u; }
                }
            } else if (tracing) {
                smallCandidates(smallTris.data, nTris, path.o, path.d, &candidatesLow, &candidatesHigh, candidateNear(PATHED_TNEAR));
            }
            if (COUNT && tracing) {
                trisTested += (unsigned int)nTris * (traceShadow ? 2u : 1u);
                closestRays++;
                if (traceShadow) { shadowRays++; }
            }
            bool spheresDone = false;   // (wave-uniform) the shared phase 2 tested the sphere candidates: no loop over the spheres
            RESOLVE_PROBE(9, candidatesLow, candidatesHigh);   // (profile builds) the resolve loops: iterations, candidates
            RESOLVE_PROBE(10, shadowLow, shadowHigh);
            if (MFMA) {
                mfmaResolve(geometry, ray, candidatesLow, candidatesHigh);
                mfmaResolve(geometry, shadowRay, shadowLow, shadowHigh);
            } else if (QUADS && PATHED_RESOLVE_SHARED) {
                ResolveScratch scratch;
                const int waveBase = (int)(threadIdx.x & ~63u), wave = (int)(threadIdx.x >> 6);
                scratch.best = resolveBest + waveBase; scratch.uv = resolveUv + wave * kResolveCapacity; scratch.items = resolveItems + wave * kResolveCapacity;
                scratch.occluded = resolveOccluded + waveBase; scratch.count = resolveCount + wave;
                // spheres (the Veach scene's lights): a packed line-misses-sphere test for both rays, the exact tests on the shared list
                unsigned int sphereCandidates = 0u, shadowSphereCandidates = 0u;
                if (TRAITS::spheres && geometry.nSpheres > 0 && tracing) {
                    smallSphereCandidates(p, geometry.nSpheres, path.o, path.d, shadowDirection, &sphereCandidates, &shadowSphereCandidates);
                    if (!traceShadow) { shadowSphereCandidates = 0u; }
                }
                spheresDone = smallResolveShared<kResolveCapacity, PATHED_RESOLVE_SHARED != 2, TRAITS::spheres>(
                    passGeometry, ray, shadowRay, candidatesLow, candidatesHigh, shadowLow, shadowHigh, sphereCandidates, shadowSphereCandidates, scratch);
            } else {
                smallResolve(passGeometry, ray, candidatesLow, candidatesHigh);
                smallResolve(passGeometry, shadowRay, shadowLow, shadowHigh);
            }
            if (tracing && !spheresDone) { finishRay(geometry, ray); }
            if (traceShadow) {
                if (!spheresDone) { finishRay(geometry, shadowRay); }
                if (shadowRay.occluded) { path.pend = rgb(0.f); }
            }
            pendingShadow = false;
        }
        if (QUADS) {
            asm volatile("" ::: "memory");
            const float4 *stash = stashRows + threadIdx.x;
            const float4 s0 = stash[0 * kBlock], s1 = stash[1 * kBlock], s2 = stash[2 * kBlock], s4 = stash[(SINGLE ? 2 : 4) * kBlock], s5 = stash[kStashKeyRow * kBlock];
            path.result = rgb(0.f); path.result.r = s0.x; path.result.g = s0.y; path.result.b = s0.z; path.bsdfPdf = s0.w;
            path.modulation.r = s1.x; path.modulation.g = s1.y; path.modulation.b = s1.z; path.cosTheta = s1.w;
            path.throughput.r = s2.x; path.throughput.g = s2.y; path.throughput.b = s2.z; path.st = floatAsInt(s2.w);
            if (SINGLE) {
                unit = (unsigned int)floatAsInt(s5.w);
            } else {
                partial = stash[3 * kBlock];
                pixel = (uint32_t)floatAsInt(s4.x); sample = (uint32_t)floatAsInt(s4.y); endSample = (uint32_t)floatAsInt(s4.z); unit = (unsigned int)floatAsInt(s4.w);
                path.random.dimension = (uint32_t)floatAsInt(s5.w);
            }
            path.random.k0 = (uint32_t)floatAsInt(s5.x); path.random.k1 = (uint32_t)floatAsInt(s5.y); path.firstEmitMaterial = floatAsInt(s5.z);
        }
        float4 h = make_float4(ray.best, ray.bestU, ray.bestV, intAsFloat(ray.bestPrim));

        // ---- the ray arrives: the MIS term of the BSDF sample that sent it, then termination
        bool done = false;      // the lane's sample ended, `color` is its value
        bool departs = false;   // the lane has a hit (h) to go on from
        Rgb color = rgb(0.f);
        if (tracing) {
            const bool miss = floatAsInt(h.w) < 0;
            Isect arrived;
            SHADE_REGION(3, !miss);   // the hit's record, for the arrival
            if (!miss) { arrived = makeIsect<TRAITS>(scene, path.o, path.d, h); }
            done = pathArrive<TRAITS, true>(p, scene, materials, path, arrived, miss, &color);
            departs = !done;
        }

        // ---- the lanes whose sample ended put it away and take the next camera hit from the queue, by ballot rank, to depart
        // from it in this same iteration.  A camera ray that left the scene ends its sample at once: the lane comes round again.
        // (SINGLE: every entry is a hit, so nobody comes round: one put-away, one pop)
        if (SINGLE) {
            SHADE_REGION(8, done);
            putUnitAway(p, done, color, unit);
            needEntry = needEntry || done;
            const unsigned long long wanting = __ballot(needEntry);
            if (wanting != 0ull && queueCount != 0u) {
                __threadfence_block();   // (acquire) see the refill
                const unsigned int rank = laneRank(wanting);
                if (needEntry && rank < queueCount) {
                    const unsigned int slot = (queueHead + rank) & (kCameraQueueEntries - 1u);
                    const float4 e0 = cameraQueue[0 * kCameraQueueEntries + slot];
                    const float4 e1 = cameraQueue[1 * kCameraQueueEntries + slot];
                    const float4 e2 = cameraQueue[2 * kCameraQueueEntries + slot];
                    resetPath(path);
                    path.o = cameraOrigin(scene.camera);
                    path.d = v3(e0.x, e0.y, e0.z);
                    path.random.k0 = (uint32_t)floatAsInt(e2.x); path.random.k1 = (uint32_t)floatAsInt(e2.y); path.random.dimension = 2u;
                    h = make_float4(e0.w, e1.x, e1.y, e1.z);
                    unit = (unsigned int)floatAsInt(e1.w);
                    needEntry = false;
                    departs = true;
                }
                const unsigned int wanted = (unsigned int)__popcll(wanting);
                const unsigned int taken = wanted < queueCount ? wanted : queueCount;
                queueHead = (queueHead + taken) & (kCameraQueueEntries - 1u);
                queueCount -= taken;
            }
            // the next refill brings more, or the pass is dealt out and the lanes that found the queue empty retire
            if (queueCount == 0u && !unitsLeft && needEntry) { alive = false; needEntry = false; }
        } else while (true) {
            SHADE_REGION(8, done);   // samples finished (every turn of this loop and below: the lanes add up to the samples)
            {
                const bool unitDone = putSampleAway(p, singleSample, done, color, partial, unit, sample, endSample);
                needEntry = needEntry || unitDone;
                startNext = startNext || (done && !unitDone);   // the unit's next sample starts in place
            }
            done = false;
            const unsigned long long wanting = __ballot(needEntry);
            if (wanting == 0ull) { break; }
            if (queueCount == 0u) {
                // the next refill brings more, or the pass is dealt out and the lanes retire
                if (!unitsLeft && needEntry) { alive = false; needEntry = false; }
                break;
            }
            __threadfence_block();   // (acquire) see the refill
            const unsigned int rank = laneRank(wanting);
            if (needEntry && rank < queueCount) {
                const unsigned int slot = (queueHead + rank) & (kCameraQueueEntries - 1u);
                const float4 e0 = cameraQueue[0 * kCameraQueueEntries + slot];
                const float4 e1 = cameraQueue[1 * kCameraQueueEntries + slot];
                const float4 e2 = cameraQueue[2 * kCameraQueueEntries + slot];
                resetPath(path);
                path.o = cameraOrigin(scene.camera);   // cameraRay's expression: the same for every sample
                path.d = v3(e0.x, e0.y, e0.z);
                path.random.k0 = (uint32_t)floatAsInt(e2.x); path.random.k1 = (uint32_t)floatAsInt(e2.y); path.random.dimension = 2u;
                h = make_float4(e0.w, e1.x, e1.y, e1.z);
                unit = (unsigned int)floatAsInt(e1.w);
                if (singleSample) { sample = 0u; endSample = 1u; }
                else { unitSamples(p, unit, &pixel, &sample, &endSample); }
                needEntry = false;
                if (floatAsInt(h.w) < 0) {
                    color = cameraMissColor<TRAITS>(scene, path.d);
                    done = true;
                } else {
                    departs = true;
                }
            }
            const unsigned int wanted = (unsigned int)__popcll(wanting);
            const unsigned int taken = wanted < queueCount ? wanted : queueCount;
            queueHead = (queueHead + taken) & (kCameraQueueEntries - 1u);
            queueCount -= taken;
        }
        if (__ballot(alive) == 0ull) { break; }   // no sample in flight, no entry, no unit left: nothing another wave could change

        // ---- the new vertex, of the lanes that go on and of the lanes that took a camera hit alike
        SHADE_REGION(6, departs);   // new vertex: makeIsect, BSDF sample
        bool ended = false;
        if (departs) {
            // SINGLE: the vertex's row of inner keys, from the wave's table of the lane's second key (asked for ahead of
            // makeIsect, so that nothing waits for it), or filled here: another key, or a vertex beyond the tables
            uint32_t keyRow[kKeyRowWords] = {};
            if (SINGLE) {
                const int vertex = (path.st & kStBounceMask) + 1;
                const int table = keySlots.find(path.random.k1);
                if (table >= 0 && vertex <= kKeyVertices) {
                    const uint4 *row = keyTables + (table * kKeyTableWords + (vertex - 1) * kKeyRowWords) / 4;
                    const uint4 low = row[0], high = row[1];
                    keyRow[0] = low.x; keyRow[1] = low.y; keyRow[2] = low.z; keyRow[3] = low.w;
                    keyRow[4] = high.x; keyRow[5] = high.y; keyRow[6] = high.z; keyRow[7] = high.w;
                } else {
                    fillKeyRow(path.random.k1, vertex, keyRow);
                }
            }
            Isect isect = makeIsect<TRAITS>(scene, path.o, path.d, h);
            ShadowRequest shadow;
            ended = pathDepart<TRAITS, true, SINGLE>(p, scene, materials, path, isect, &shadow, &color, keyRow);
            // the vertex's shadow ray leaves isect.point like the continuation ray: both are traced in the next pass
            if (shadow.push) {
                pendingShadow = true;
                shadowDirection = shadow.direction;
                shadowTfar = shadow.tfar;
            }
        }
        // (rare: a dead end, or the last vertex the bounce window wants) such a lane takes its entry in the next iteration
        if (__ballot(ended) != 0ull) {
            SHADE_REGION(8, ended);
            if (SINGLE) {
                putUnitAway(p, ended, color, unit);
                needEntry = needEntry || ended;
            } else {
                const bool unitDone = putSampleAway(p, singleSample, ended, color, partial, unit, sample, endSample);
                needEntry = needEntry || unitDone;
                startNext = startNext || (ended && !unitDone);
            }
        }
    }

    if (COUNT) {
        atomicAdd(&p.stats[kStatTris], (unsigned long long)trisTested);
        atomicAdd(&p.stats[kStatClosest], (unsigned long long)closestRays);
        atomicAdd(&p.stats[kStatShadow], (unsigned long long)shadowRays);
    }
