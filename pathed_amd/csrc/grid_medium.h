// Heterogeneous media: the reference's GridMedium (src/grid_medium.cpp) over a UniformGrid (src/uniform_grid.cpp), walked by
// its RegularTrackerState (src/regular_tracker.cpp, include/regular_tracker.h) after a clip against the grid's box
// (src/aabb.cpp), restated statement for statement.  Used by k_path_volume_grid (kernels.h) and by the test hook
// k_grid_queries; the other kernels do not know grids.
//
// A medium record (volume.h: DMedium) of kind kMediumGrid points at one DGrid; the densities of all grids lie in one float
// array, each grid's cells at DGrid::dataOffset in UniformGrid's order, index = (z * cellsY + y) * cellsX + x.
//
// THE LOOP BOUND.  The reference's two tracker loops end when the tracker's time reaches the segment's end, and assert(0) when
// a NaN time matches no axis.  Here both loops also stop after cellsX + cellsY + cellsZ + 3 steps, and a step that matches no
// axis is invalid (the loop ends).  Inside the box a segment crosses at most cells - 1 integer planes per axis, so a clipped
// segment (everything the integrator asks) ends by itself before the bound; a segment that starts far outside the grid
// (possible through the hook only: findTransmittance does not clip) is cut off there.
#pragma once

#include "vecmath.h"

#include <cfloat>

namespace pathed {

static const int kMediumHomogeneous = 0;
static const int kMediumGrid = 1;

// GridInfo + GridMedium's members.  160 bytes.
struct DGrid {
    int cellsX, cellsY, cellsZ;
    unsigned int dataOffset;          // first cell in the scene's density array, in floats
    float minX, minY, minZ;           // GridInfo's order, which is the .vol file's
    float maxX, maxY, maxZ;
    float widthX, widthY, widthZ;     // GridMedium::m_width* (max - min)
    float albedo, scale;
    float pad;
    float worldToModel[12];           // rows 0..2 of the 4x4 (Transform::apply(Point3) reads no other)
    float modelToWorld[12];           // ... of its inverse (Transform::applyInverse)
};

__device__ inline int gridStepBound(const DGrid &g) { return g.cellsX + g.cellsY + g.cellsZ + 3; }

// Transform::apply(const Point3 &), src/transform.cpp:64-75
__device__ inline V3 gridApply(const float *m, V3 p)
{
    return v3(m[0] * p.x + m[1] * p.y + m[2] * p.z + m[3],
              m[4] * p.x + m[5] * p.y + m[6] * p.z + m[7],
              m[8] * p.x + m[9] * p.y + m[10] * p.z + m[11]);
}

// GridMedium::modelToGrid, src/grid_medium.cpp:66-73
__device__ inline V3 gridModelToGrid(const DGrid &g, V3 p)
{
    return v3(((p.x - g.minX) / g.widthX) * (float)(g.cellsX - 1),
              ((p.y - g.minY) / g.widthY) * (float)(g.cellsY - 1),
              ((p.z - g.minZ) / g.widthZ) * (float)(g.cellsZ - 1));
}

// gridToWorld, src/regular_tracker.cpp:26-33 (grid space to MODEL space, whatever its name)
__device__ inline V3 gridGridToModel(const DGrid &g, V3 p)
{
    return v3((p.x / (float)(g.cellsX - 1)) * g.widthX + g.minX,
              (p.y / (float)(g.cellsY - 1)) * g.widthY + g.minY,
              (p.z / (float)(g.cellsZ - 1)) * g.widthZ + g.minZ);
}

// UniformGrid::interpolate, src/uniform_grid.cpp:33-79.  The range test is written so that a NaN coordinate is out of range
// too (the reference would index with it); inside the range floor and ceil lie in [0, cells - 1], which is what
// UniformGrid::lookup (:16-26) tests, so no load leaves the grid.  Eight loads, all issued before the first use.
__device__ inline float gridInterpolate(const DGrid &g, const float *data, V3 p)
{
    if (!(p.x >= 0.f && p.x <= (float)(g.cellsX - 1))) { return 0.f; }
    if (!(p.y >= 0.f && p.y <= (float)(g.cellsY - 1))) { return 0.f; }
    if (!(p.z >= 0.f && p.z <= (float)(g.cellsZ - 1))) { return 0.f; }

    const int x0 = (int)floorf(p.x), x1 = (int)ceilf(p.x);
    const float xd = p.x - x0;
    const int y0 = (int)floorf(p.y), y1 = (int)ceilf(p.y);
    const float yd = p.y - y0;
    const int z0 = (int)floorf(p.z), z1 = (int)ceilf(p.z);
    const float zd = p.z - z0;

    const float *cells = data + g.dataOffset;
    const size_t row00 = ((size_t)z0 * g.cellsY + y0) * g.cellsX, row01 = ((size_t)z1 * g.cellsY + y0) * g.cellsX;
    const size_t row10 = ((size_t)z0 * g.cellsY + y1) * g.cellsX, row11 = ((size_t)z1 * g.cellsY + y1) * g.cellsX;
    const float c000 = cells[row00 + x0];
    const float c001 = cells[row01 + x0];
    const float c010 = cells[row10 + x0];
    const float c011 = cells[row11 + x0];
    const float c100 = cells[row00 + x1];
    const float c101 = cells[row01 + x1];
    const float c110 = cells[row10 + x1];
    const float c111 = cells[row11 + x1];

    const float c_00 = c000 * (1 - xd) + c100 * xd;
    const float c_01 = c001 * (1 - xd) + c101 * xd;
    const float c_10 = c010 * (1 - xd) + c110 * xd;
    const float c_11 = c011 * (1 - xd) + c111 * xd;

    const float c__0 = c_00 * (1 - yd) + c_10 * yd;
    const float c__1 = c_01 * (1 - yd) + c_11 * yd;

    return c__0 * (1 - zd) + c__1 * zd;
}

// GridMedium::sigmaT(point, GridFrame::Model) and sigmaT(worldPoint), src/grid_medium.cpp:36-52
__device__ inline float gridSigmaTModel(const DGrid &g, const float *data, V3 modelPoint)
{
    return gridInterpolate(g, data, gridModelToGrid(g, modelPoint)) * g.scale;
}

__device__ inline float gridSigmaTWorld(const DGrid &g, const float *data, V3 worldPoint)
{
    return gridSigmaTModel(g, data, gridApply(g.worldToModel, worldPoint));
}

// ---- AABB, src/aabb.cpp
struct GridBoxHit {
    bool isHit;
    V3 enterPoint, exitPoint;
    float enterT, exitT;
};

// AABB::intersect(const Ray &), :19-63
__device__ inline GridBoxHit gridBoxRay(const DGrid &g, V3 origin, V3 direction)
{
    GridBoxHit hit;
    hit.isHit = false;
    hit.enterPoint = v3(0.f, 0.f, 0.f); hit.exitPoint = v3(0.f, 0.f, 0.f);
    hit.enterT = 0.f; hit.exitT = 0.f;

    const V3 invDirection = v3(1.f / direction.x, 1.f / direction.y, 1.f / direction.z);

    const float t1 = (g.minX - origin.x) * invDirection.x;
    const float t2 = (g.maxX - origin.x) * invDirection.x;
    const float t3 = (g.minY - origin.y) * invDirection.y;
    const float t4 = (g.maxY - origin.y) * invDirection.y;
    const float t5 = (g.minZ - origin.z) * invDirection.z;
    const float t6 = (g.maxZ - origin.z) * invDirection.z;

    const float tmin = fmaxf(fmaxf(fminf(t1, t2), fminf(t3, t4)), fminf(t5, t6));
    const float tmax = fminf(fminf(fmaxf(t1, t2), fmaxf(t3, t4)), fmaxf(t5, t6));

    if (tmin >= tmax) { return hit; }
    if (tmin < 0 && tmax == 0) { return hit; }

    if (tmin >= 0 && !isinf(tmin) && tmax >= 0 && !isinf(tmax)) {
        hit.isHit = true;
        hit.enterPoint = origin + direction * tmin;
        hit.exitPoint = origin + direction * tmax;
        hit.enterT = tmin;
        hit.exitT = tmax;
        return hit;
    }

    if (tmax >= 0 && !isinf(tmax) && tmin < 0) {
        hit.isHit = true;
        hit.enterPoint = origin;
        hit.exitPoint = origin + direction * tmax;
        hit.enterT = 0.f;
        hit.exitT = tmax;
        return hit;
    }

    return hit;
}

// AABB::intersect(const Point3 &, const Point3 &), :65-83
__device__ inline GridBoxHit gridBoxSegment(const DGrid &g, V3 enterPoint, V3 exitPoint)
{
    const V3 travelDirection = exitPoint - enterPoint;
    GridBoxHit hit = gridBoxRay(g, enterPoint, normalized(travelDirection));

    const float maxT = length(travelDirection);
    if (!hit.isHit) { return hit; }
    if (hit.exitT <= maxT) { return hit; }

    hit.exitPoint = exitPoint;
    hit.exitT = maxT;
    return hit;
}

// ---- RegularTrackerState: rates, next times, current time and end time (and the two lengths worldTime divides by), in registers
struct GridTracker {
    float rateX, rateY, rateZ;
    float nextX, nextY, nextZ;
    float currentTime, endTime;
    float totalGridTime, totalWorldTime;   // worldTime's two lengths: they depend on the end points only
    int cellX, cellY, cellZ;               // m_currentCell (nothing downstream reads it: the density is looked up at the midpoint)
};

struct GridStep {
    bool isValidStep;
    float cellTime, enterTime, currentTime;
};

// calculateNextDistance, :35-50
__device__ inline float gridNextDistance(float currentValue, bool isForward)
{
    if (isForward) {
        if (currentValue == floorf(currentValue)) { return 1.f; }
        return ceilf(currentValue) - currentValue;
    }
    if (currentValue == floorf(currentValue)) { return -1.f; }
    return floorf(currentValue) - currentValue;
}

// calculateNextTime, :52-56
__device__ inline float gridNextTime(float nextDistance, float rate)
{
    if (rate == 0.f) { return FLT_MAX; }
    return nextDistance / rate;
}

// GridCell(point, gridInfo), include/regular_tracker.h:14-34: an outer boundary belongs to the cell inside it
__device__ inline int gridCellOf(float value, int cells)
{
    if (value == (float)cells) { return cells - 1; }
    return (int)floorf(value);
}

// RegularTrackerState::RegularTrackerState, :116-144
__device__ inline GridTracker gridTrackerStart(const DGrid &g, V3 entryPoint, V3 exitPoint)
{
    GridTracker t;
    const V3 rayPath = exitPoint - entryPoint;
    const float totalDistance = length(rayPath);

    t.rateX = rayPath.x / totalDistance;
    t.rateY = rayPath.y / totalDistance;
    t.rateZ = rayPath.z / totalDistance;

    t.nextX = gridNextTime(gridNextDistance(entryPoint.x, t.rateX > 0.f), t.rateX);
    t.nextY = gridNextTime(gridNextDistance(entryPoint.y, t.rateY > 0.f), t.rateY);
    t.nextZ = gridNextTime(gridNextDistance(entryPoint.z, t.rateZ > 0.f), t.rateZ);

    t.currentTime = 0.f;
    t.cellX = gridCellOf(entryPoint.x, g.cellsX);
    t.cellY = gridCellOf(entryPoint.y, g.cellsY);
    t.cellZ = gridCellOf(entryPoint.z, g.cellsZ);
    t.endTime = totalDistance;

    // worldTime, :146-154
    t.totalGridTime = length(entryPoint - exitPoint);
    t.totalWorldTime = length(gridGridToModel(g, exitPoint) - gridGridToModel(g, entryPoint));
    return t;
}

// RegularTrackerState::worldTime, :146-154
__device__ inline float gridWorldTime(const GridTracker &t, float gridTime)
{
    const float timeRatio = gridTime / t.totalGridTime;
    return timeRatio * t.totalWorldTime;
}

// RegularTrackerState::step, :156-217
__device__ inline GridStep gridTrackerStep(GridTracker &t)
{
    GridStep result;
    result.isValidStep = false;
    result.cellTime = 0.f; result.enterTime = 0.f; result.currentTime = 0.f;
    if (t.currentTime >= t.endTime) { return result; }

    const float minTime = fminf(t.nextX, fminf(t.nextY, t.nextZ));

    if (t.nextX == minTime) {
        if (t.rateX > 0.f) { t.nextX = t.nextX + 1.f / t.rateX; t.cellX += 1; }
        else { t.nextX = t.nextX + -1.f / t.rateX; t.cellX += -1; }
    } else if (t.nextY == minTime) {
        if (t.rateY > 0.f) { t.nextY = t.nextY + 1.f / t.rateY; t.cellY += 1; }
        else { t.nextY = t.nextY + -1.f / t.rateY; t.cellY += -1; }
    } else if (t.nextZ == minTime) {
        if (t.rateZ > 0.f) { t.nextZ = t.nextZ + 1.f / t.rateZ; t.cellZ += 1; }
        else { t.nextZ = t.nextZ + -1.f / t.rateZ; t.cellZ += -1; }
    } else {
        return result;   // a NaN time: the reference's assert(0); here the walk ends
    }

    const float clippedTime = fminf(minTime, t.endTime);
    const float cellTime = clippedTime - t.currentTime;
    const float enterTime = t.currentTime;
    t.currentTime = clippedTime;

    result.isValidStep = true;
    result.cellTime = gridWorldTime(t, cellTime);
    result.enterTime = gridWorldTime(t, enterTime);
    result.currentTime = gridWorldTime(t, t.currentTime);
    return result;
}

// GridMedium::transmittance, src/grid_medium.cpp:85-123 (one channel: util::exp of a grey colour)
__device__ inline float gridTransmittance(const DGrid &g, const float *data, V3 entryPointWorld, V3 exitPointWorld)
{
    const GridBoxHit hit = gridBoxSegment(g, gridApply(g.worldToModel, entryPointWorld), gridApply(g.worldToModel, exitPointWorld));
    if (!hit.isHit) { return 1.f; }

    const V3 entryPoint = gridModelToGrid(g, hit.enterPoint);
    const V3 exitPoint = gridModelToGrid(g, hit.exitPoint);

    float accumulatedExponent = 0.f;

    GridTracker tracker = gridTrackerStart(g, entryPoint, exitPoint);
    const V3 rayOrigin = hit.enterPoint;
    const V3 rayDirection = normalized(hit.exitPoint - hit.enterPoint);

    const int bound = gridStepBound(g);
    for (int steps = 0; steps < bound; steps++) {
        const GridStep step = gridTrackerStep(tracker);
        if (!step.isValidStep) { break; }
        const float midpointTime = (step.enterTime + step.currentTime) / 2.f;
        const V3 midpointModel = rayOrigin + rayDirection * midpointTime;
        const float midpointSigmaT = gridSigmaTModel(g, data, midpointModel);

        accumulatedExponent += midpointSigmaT * step.cellTime;
    }

    return expf(-accumulatedExponent);
}

// GridMedium::findTransmittance, src/grid_medium.cpp:125-168.  Returns isValid; *distance is -1 where it is not.
__device__ inline bool gridFindTransmittance(const DGrid &g, const float *data, V3 entryPointWorld, V3 exitPointWorld,
                                             float targetTransmittance, float *distance)
{
    // -std::log(float): glibc's logf, which rounds correctly; ocml's is within 1 ulp, and on a target that IS exp(-exponent of
    // the whole segment) -- the reference's own "full line across" fixtures -- that ulp decides between a distance and "not
    // met".  The double logarithm narrowed to float is the correctly rounded value; once per distance sample.
    const float targetExponent = (float)-log((double)targetTransmittance);

    const V3 entryPoint = gridModelToGrid(g, gridApply(g.worldToModel, entryPointWorld));
    const V3 exitPoint = gridModelToGrid(g, gridApply(g.worldToModel, exitPointWorld));

    float accumulatedExponent = 0.f;

    GridTracker tracker = gridTrackerStart(g, entryPoint, exitPoint);
    const V3 rayOrigin = entryPointWorld;
    const V3 rayDirection = normalized(exitPointWorld - entryPointWorld);

    const int bound = gridStepBound(g);
    for (int steps = 0; steps < bound; steps++) {
        const GridStep step = gridTrackerStep(tracker);
        if (!step.isValidStep) { break; }
        const float midpointTime = (step.enterTime + step.currentTime) / 2.f;
        const V3 midpointWorld = rayOrigin + rayDirection * midpointTime;
        const float midpointSigmaT = gridSigmaTWorld(g, data, midpointWorld);

        const float cellExponent = midpointSigmaT * step.cellTime;
        accumulatedExponent += cellExponent;

        if (accumulatedExponent >= targetExponent) {
            const float overflow = accumulatedExponent - targetExponent;
            const float cellRatio = 1.f - overflow / cellExponent;
            const float actualCellTime = step.cellTime * cellRatio;

            *distance = step.currentTime - step.cellTime + actualCellTime;
            return true;
        }
    }

    *distance = -1.f;
    return false;
}

// The medium-sampling half of GridMedium::integrate, src/grid_medium.cpp:170-198: the sample point of a medium event on the
// segment, or false (noScatter).  The target transmittance is random.next() ITSELF (the homogeneous medium maps xi through
// -log(1 - xi)); the clip is the RAY form of the box test, not the segment form transmittance() uses.
template <typename Random>
__device__ inline bool gridSamplePoint(const DGrid &g, const float *data, V3 entryPointWorld, V3 exitPointWorld, Random &random, V3 *samplePoint)
{
    const V3 entryPointModel = gridApply(g.worldToModel, entryPointWorld);
    const V3 exitPointModel = gridApply(g.worldToModel, exitPointWorld);

    const V3 travelVector = exitPointModel - entryPointModel;
    const V3 travelDirection = normalized(travelVector);

    const GridBoxHit hit = gridBoxRay(g, entryPointModel, travelDirection);
    if (!hit.isHit) { return false; }

    const float targetTransmittance = random.next();
    float distance;
    const bool isValid = gridFindTransmittance(g, data, gridApply(g.modelToWorld, hit.enterPoint), gridApply(g.modelToWorld, hit.exitPoint),
                                               targetTransmittance, &distance);
    if (!isValid) { return false; }
    *samplePoint = gridApply(g.modelToWorld, entryPointModel + travelDirection * distance);
    return true;
}

// the test hook (pathed_hip_grid_queries): one thread per segment runs the two functions on grid `grid`
__global__ void k_grid_queries(const DGrid *grids, const float *data, int grid, int n, const float *a, const float *b, const float *target,
                               float *transmittance, float *distance)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)n) { return; }
    const DGrid g = grids[grid];
    const V3 pa = v3(a[3 * i], a[3 * i + 1], a[3 * i + 2]);
    const V3 pb = v3(b[3 * i], b[3 * i + 1], b[3 * i + 2]);
    transmittance[i] = gridTransmittance(g, data, pa, pb);
    float found;
    gridFindTransmittance(g, data, pa, pb, target[i], &found);
    distance[i] = found;
}

}  // namespace pathed
