// Per-pixel candidate masks of the camera rays (k_path_small's camera-queue refill, kernels.h).
//
// The camera is a pinhole: every camera ray starts at O = cameraOrigin() and a sample of pixel (row, col) leaves through the
// film rectangle (col + jx, row + jy), jx, jy in [-0.5, 0.5) (path_common.h: cameraSampleRay), along M (fx, fy, -zNear) with
// fx = filmWidth (col + jx + 0.5) / resX - filmWidth / 2 and fy likewise (shading.h: cameraRay).  Which triangles such a ray
// can meet depends on (scene, camera, resolution) alone, so the set is computed once per pixel -- here, in double precision --
// and the refill reads it instead of running phase 1 (kernels.h: smallCandidatesItems) over every record for every sample.
// Phase 2 (trace.h: intersectTriangle + the acceptance rule) still decides every hit: a mask only has to be a SUPERSET of
// what phase 2 can accept for any ray of the pixel.
//
// The rule.  The rays of a pixel fill a four-sided cone with apex O whose corner directions are c_i = M (fx_i, fy_i, -zNear)
// at the four corners of the film rectangle.  Side plane i holds O, c_i and c_(i+1); its normal N_i = c_i x c_(i+1) is turned
// towards the inside (N_i . (c_0 + c_1 + c_2 + c_3) > 0), so every direction d of the cone has N_i . d >= 0 for all four i.
// A ray O + t d, t > 0, that meets the triangle meets it in a point X = sum w_j P_j, w_j >= 0, sum w_j = 1, of its corners
// (as the intersector sees them: v0, v0 + e1, v0 + e2), hence N_i . d = N_i . (X - O) / t = sum w_j N_i . (P_j - O) / t.  If
// for ONE i all three corners have N_i . (P_j - O) < 0 that sum is negative and d is not in the cone: the bit is cleared on
// that proof or on the one below, and on nothing else.  (Corners behind the camera need no special case: the argument never divides by
// a depth.  A triangle that crosses the camera's plane is usually outside no single side plane and keeps its bit.)
//
// The triangle's edges.  The four side planes alone are a bounding-box test on the film: a pixel inside a quad would keep both
// of its triangles, a pixel beside a slanted edge the triangle beyond it.  The same argument runs the other way round: the plane
// through O and an edge (P_a, P_b) has the normal n = (P_a - O) x (P_b - O), turned so that the third corner is inside
// (n . (P_c - O) > 0); every point X of the triangle then has n . (X - O) >= 0, so a ray that meets the triangle has n . d >= 0.
// Every d of the cone is a combination of its four corner directions with weights >= 0 (the cone is convex: the inside test
// below), so if all four have n . c_i < 0 no ray of the pixel meets the triangle.  Side planes and edge planes together are
// all the separating planes a triangle and a four-sided cone with a common view point can have.  The tolerance here is
// relative to the quantity the intersector's rounding is bounded by: n . c_i < -2^-16 |c_i| |P_a - O| |P_b - O|, eight times
// the 32 x 2^-24 |d| |P - o| |Q - o| of small_items.h for the edge function of that very edge, however short the edge is.
// "The third corner is inside" is the sign of the triple product (P_a - O) . ((P_b - O) x (P_c - O)) = (O - v0) . (e1 x e2),
// which is also the sign the intersector's t det must have for t > 0: the orientation is only as good as that sign.  The
// intersector rounds it relative to |o - v0| |e1| |e2| (Moeller-Trumbore works on the edges), which exceeds |P_a - O| |P_b - O|
// |P_c - O| when v0 is much farther from O than another corner, so the guard takes the larger of the two: the edge planes
// are used only where |triple product| > 2^-16 max(|P_a - O| |P_b - O| |P_c - O|, |O - v0| |e1| |e2|), 8 x the 2^-19 bound again.
// A triangle seen edge-on from O by that measure, or a degenerate one, is culled by the side planes or not at all.
//
// The margins.  Phase 2 and cameraRay work in fp32, this test in fp64 on the same fp32 inputs, so the fp32 rounding must not
// be able to carry a ray across a side plane that the test called separating:
//   * the footprint is widened by 1/64 pixel on every side.  cameraRay's film coordinate carries a few roundings of size
//     2^-24 filmWidth (the sum row + jitter, the product, the quotient, the difference) against a pixel of filmWidth / resX:
//     below 4 resX 2^-24 pixels, which is 1/64 pixel at resX = 65536 and 1/4096 pixel at 1024; normalising the direction
//     moves it along itself only;
//   * a corner counts as outside only where N_i . (P_j - O) < -2^-16 |N_i| |P_j - O|, i.e. where it is more than 2^-16 rad
//     (3 arc seconds) of angle, as seen from O, beyond the plane.  The intersector's three edge functions E = d . ((P - o) x
//     (Q - o)) are evaluated with a relative error of at most 32 x 2^-24 = 2^-19 of |d| |P - o| |Q - o| (the bound small_items.h
//     derives for the same quantities, and uses for its own tolerances), a rotation of the edge's plane about O by at most
//     2^-19 / sin(angle the edge subtends at O); the tolerance covers it for every edge that subtends more than 1/8 rad, and
//     together with the 1/64 pixel (1e-5 rad at 1024 pixels across 40 degrees) for shorter ones in proportion.
//     Both margins are fixed fractions, far below a pixel at any resolution (2^-16 rad is a 1/45 pixel at 1024 across 40 degrees);
//   * the test's own fp64 rounding (2^-53 relative per operation, a few dozen operations) is nine orders below either.
// What cannot be decided -- a not-a-number anywhere, a camera matrix whose corner directions do not span a cone (N_i = 0, or
// the inside test N_i . centre > 2^-40 |N_i| |centre| fails) -- keeps EVERY triangle of the scene for that pixel: every
// comparison below is written so that a NaN keeps the bit.
//
// Layout: one 64-bit word per pixel, triangle k of the ITEM order (small_items.h: itemTris) at bit 63 - k, so that the
// word's upper half is smallResolve's candidatesLow (triangle k at bit 31 - (k & 31) of word k >> 5) and its lower half
// candidatesHigh.  Spheres have no bits: finishRay tests them as before.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define PATHED_MASK_FN __host__ __device__ inline
#else
#define PATHED_MASK_FN inline
#endif

namespace pathed {

static const double kMaskWiden = 1.0 / 64.0;            // pixels, on every side of the footprint
static const double kMaskOutside = 1.0 / 65536.0;       // relative to |N| |P - O|
static const double kMaskInside = 1.0 / 1099511627776.0;   // 2^-40: the cone's centre must be this far inside every side plane

struct PixelCone {
    double origin[3];
    double normal[4][3];    // inward
    double length[4];       // |normal|
    double corner[4][3];    // the corner directions c_i
    double cornerLength[4];
    bool decided;           // false: keep every triangle
};

// the cone of pixel (row, col); origin, m (cameraToWorld rows), film size and resolution as DCamera holds them
PATHED_MASK_FN PixelCone pixelCone(const float *origin, const float *m, float filmWidth, float filmHeight, int resX, int resY, int row, int col)
{
    PixelCone cone;
    const double zNear = (double)0.01f;   // cameraRay's
    const double width = filmWidth, height = filmHeight;
    // cameraRay: width * (colf + 0.5) / resX - width / 2 with colf in [col - 0.5, col + 0.5)
    const double x0 = width * ((double)col - kMaskWiden) / (double)resX - width / 2.0;
    const double x1 = width * ((double)col + 1.0 + kMaskWiden) / (double)resX - width / 2.0;
    const double y0 = height * ((double)row - kMaskWiden) / (double)resY - height / 2.0;
    const double y1 = height * ((double)row + 1.0 + kMaskWiden) / (double)resY - height / 2.0;
    const double film[4][2] = { { x0, y0 }, { x1, y0 }, { x1, y1 }, { x0, y1 } };
    double corner[4][3], centre[3] = { 0.0, 0.0, 0.0 };
    for (int i = 0; i < 4; i++) {
        for (int a = 0; a < 3; a++) {
            corner[i][a] = (double)m[3 * a + 0] * film[i][0] + (double)m[3 * a + 1] * film[i][1] - (double)m[3 * a + 2] * zNear;
            centre[a] += corner[i][a];
        }
    }
    const double centreLength = std::sqrt(centre[0] * centre[0] + centre[1] * centre[1] + centre[2] * centre[2]);
    cone.decided = true;
    for (int a = 0; a < 3; a++) { cone.origin[a] = origin[a]; }
    for (int i = 0; i < 4; i++) {
        for (int a = 0; a < 3; a++) { cone.corner[i][a] = corner[i][a]; }
        cone.cornerLength[i] = std::sqrt(corner[i][0] * corner[i][0] + corner[i][1] * corner[i][1] + corner[i][2] * corner[i][2]);
    }
    for (int i = 0; i < 4; i++) {
        const double *p = corner[i], *q = corner[(i + 1) & 3];
        double n[3] = { p[1] * q[2] - p[2] * q[1], p[2] * q[0] - p[0] * q[2], p[0] * q[1] - p[1] * q[0] };
        const double length = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        double inside = n[0] * centre[0] + n[1] * centre[1] + n[2] * centre[2];
        if (inside < 0.0) { inside = -inside; n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        // (NaN, infinity and a flat cone all fail this)
        if (!(inside > kMaskInside * length * centreLength) || !(length * centreLength < 1e300)) { cone.decided = false; }
        for (int a = 0; a < 3; a++) { cone.normal[i][a] = n[a]; }
        cone.length[i] = length;
    }
    return cone;
}

// true: no ray of the cone can meet the triangle (v0, v0 + e1, v0 + e2)
PATHED_MASK_FN bool coneMissesTriangle(const PixelCone &cone, const float *v0, const float *e1, const float *e2)
{
    if (!cone.decided) { return false; }
    double corner[3][3], distance[3];
    for (int a = 0; a < 3; a++) {
        corner[0][a] = (double)v0[a] - cone.origin[a];
        corner[1][a] = (double)v0[a] + (double)e1[a] - cone.origin[a];
        corner[2][a] = (double)v0[a] + (double)e2[a] - cone.origin[a];
    }
    for (int j = 0; j < 3; j++) { distance[j] = std::sqrt(corner[j][0] * corner[j][0] + corner[j][1] * corner[j][1] + corner[j][2] * corner[j][2]); }
    for (int i = 0; i < 4; i++) {
        const double *n = cone.normal[i];
        bool allOutside = true;
        for (int j = 0; j < 3; j++) {
            const double side = n[0] * corner[j][0] + n[1] * corner[j][1] + n[2] * corner[j][2];
            if (!(side < -kMaskOutside * cone.length[i] * distance[j])) { allOutside = false; }   // NaN: not outside
        }
        if (allOutside) { return true; }
    }
    // the triangle's own edge planes (header: "The triangle's edges").  tripleScale: what the intersector's t det = (o - v0) .
    // (e1 x e2) -- the same triple product as `third` below -- is rounded relative to
    const double e1Length = std::sqrt((double)e1[0] * e1[0] + (double)e1[1] * e1[1] + (double)e1[2] * e1[2]);
    const double e2Length = std::sqrt((double)e2[0] * e2[0] + (double)e2[1] * e2[1] + (double)e2[2] * e2[2]);
    const double cornersScale = distance[0] * distance[1] * distance[2], edgesScale = distance[0] * e1Length * e2Length;
    const double tripleScale = cornersScale > edgesScale ? cornersScale : edgesScale;
    for (int e = 0; e < 3; e++) {
        const double *a = corner[e], *b = corner[(e + 1) % 3], *c = corner[(e + 2) % 3];
        double n[3] = { a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0] };
        double third = n[0] * c[0] + n[1] * c[1] + n[2] * c[2];
        if (third < 0.0) { third = -third; n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
        const double scale = distance[e] * distance[(e + 1) % 3];
        if (!(third > kMaskOutside * tripleScale)) { continue; }   // seen edge-on, degenerate or NaN: this edge proves nothing
        bool allOutside = true;
        for (int i = 0; i < 4; i++) {
            const double side = n[0] * cone.corner[i][0] + n[1] * cone.corner[i][1] + n[2] * cone.corner[i][2];
            if (!(side < -kMaskOutside * scale * cone.cornerLength[i])) { allOutside = false; }
        }
        if (allOutside) { return true; }
    }
    return false;
}

// the mask of one pixel over nTris <= 64 item-order triangle records of 12 floats: (v0, prim) (e1, -) (e2, -)
PATHED_MASK_FN uint64_t pixelMask(const PixelCone &cone, const float *itemTris, int nTris)
{
    uint64_t mask = 0;
    for (int k = 0; k < nTris && k < 64; k++) {
        const float *tri = itemTris + (size_t)12 * k;
        if (!coneMissesTriangle(cone, tri, tri + 4, tri + 8)) { mask |= (uint64_t)1 << (63 - k); }
    }
    return mask;
}

}  // namespace pathed
