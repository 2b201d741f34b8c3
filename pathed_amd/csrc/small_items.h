// The records phase 1 of the all-triangles intersector reads in the fused path kernel (kernels.h: smallCandidatesItems).
//
// The scenes that take this intersector are built of QUADS (Cornell: 17 of its 18 -- the left wall is not planar --, of which 4
// are trapezoids 0.6 % off a parallelogram): CornellBox-Original.obj is 18 of them, the Veach scene's plates
// and floor are quads, `"type": "quad"` models are quads (reference src/quad.cpp:27-151, src/obj_parser.cpp's (0,1,2),(0,2,3)
// split).  Two triangles that share a diagonal and form a parallelogram are ONE Moeller-Trumbore evaluation in phase 1: the
// parallelogram c0 + alpha a1 + beta a2, alpha, beta in [0, 1], holds both (triangle A: beta <= alpha, triangle B: alpha <=
// beta), so u det, v det, det and t det are computed once for the two of them -- half the arithmetic of the pass, which is a
// third of k_path_small's instructions.  Phase 1 only has to be CONSERVATIVE (phase 2, trace.h: intersectTriangle +
// testLeafTriangle, decides): but here its quantities are no longer the bits phase 2 computes for the triangle (another
// origin, other edges), so every bound carries a tolerance that covers both evaluations' rounding and the distance delta
// between the triangles' corners (as the intersector sees them: v0, v0 + e1, v0 + e2) and the parallelogram's.
//
// With the three edge functions of a triangle E(P, Q) = d . ((P - o) x (Q - o)) (which is what u det, v det and
// (det - u - v) det are, whatever vertex order), |d| <= 1.0001, r = |o - c0| + amax the distance from the ray's origin to any
// corner (amax = the longest of a1, a2, a1 + a2), u = 2^-24:
//     |rounding of either evaluation| <= 8 u r amax per edge function,   |moving a corner by delta| <= 2 delta r
//  => E_uv = (32 u amax + 4 delta) r,   E_t = (32 u |a1||a2| + 8 delta amax) r   (t det = (c0 - o) . (a1 x a2)),
//     E_det = 16 u |a1||a2| + 4 delta amax.
// The errors scale with the distance of the ORIGIN, not with the scene: a ray leaving a quad sees that quad (t = 0, to be
// told from t >= tnear / 2) with the error of a nearby origin, however far away the camera is.  A bound "X sign(det) >= -E" is
// tested as X det >= -E |det| with E |det| <= kappa det^2 + E^2 / (4 kappa) and r^2 <= 2 (|o - c0|^2 + amax^2), so the kernel
// compares against   tol = kappa det^2 + K2 (|o - c0|^2 + amax^2),   K2 = (E / r)^2 / (2 kappa),
// kappa = 1e-5 for the barycentric bounds (a relative slack of 1e-5), kappa_t = tnear / 16 for the t bounds (an absolute
// slack in t, well inside the tnear / 2 by which the interval is widened anyway).  Where |det| <= E_det the computed sign of
// det cannot be trusted; every bound is then at most Xmax E_det in size, which the K terms include: nothing is rejected there.  The far bound's error grows with the ray's own tfar:
// tolFar = tolT + tfarHigh (kappa_far det^2 + E_det^2 / (4 kappa_far)), kappa_far = 1e-6 (a light 20 units away is told from
// an occluder 1e-3 in front of it with 2e-5 of slack).  Triangles that find no partner keep the exact test.
//
// NEVER-OCCLUDERS (smallNeverOccluders below).  A shadow ray (kernels.h: sampleLightsTerm) leaves a point found on a scene
// surface towards a point sampled on an emitter, |d| = 1 up to rounding, accepted hits in (tnear, distance - 1e-3].  A triangle
// Y that lies in a supporting plane of everything such a ray can start on, with every emitter well off that plane, can only
// be met within a hair of the origin, below tnear, where phase 2 rejects the hit: the shadow ray need not test it at all (the
// walls of a room).  Such items are put LAST in item order and the shadow ray's half of phase 1 stops before them.  With Y's
// plane (unit normal n, offset c, either orientation), s(x) = n . x - c, Y qualifies when
//     (1) s >= -eta   at every corner of every scene triangle (as the intersector sees them) and over every sphere's bounds,
//     (2) s >= Dmin   at every point a light sample can land on,
// with, u = 2^-24, R = the diameter of everything including the camera, L = the diameter of the surfaces alone (the longest
// shadow ray), M = the largest coordinate, k(X) = |e1||e2| / |e1 x e2| of triangle X (1 / sin of the angle at v0):
//
// eta bounds how far an origin isect.point = fl(o + d t) sits off the plane of the triangle X it was found on.  Phase 2
// (trace.h: intersectTriangle) computes t = fl(N' / det'), N' = N + dN, det' = det + dDet the rounded triple products
// N = e2 . ((o - v0) x e1), det = e1 . (d x e2); the exact point o + d t has the offset (t det - N) / |e1 x e2| from X's plane, and
// t det - N = t det' - N' - t dDet + dN, |t det' - N'| <= u |N'| (the division).  With the error model above, 8 u per triple
// product (|dN| <= 8 u |o - v0||e1||e2|, |dDet| <= 8 u |d||e1||e2|), |o - v0| <= R and t <= R (the largest t the scene and camera
// allow: premise -- a hit whose det is all rounding can report any t, and then no bound on its point exists, here or anywhere else
// in this file), and 3 u (M + R) for the two roundings per component of o + d t:
//     eta = 1.01 (u R + 16 u R max_X k(X)) + 1.01 x 3 u (M + R).
// (The point is taken to lie inside X along X's plane: how far a grazing hit may overshoot X's edge is not modelled.)
// Sphere origins: intersectSphere's t lies in the true chord up to sqrt(32 u) R (the root of a difference rounded to 16 u R^2),
// so a point found on a sphere is within etaSphere = eta + 1.1 sqrt(32 u) R of the sphere's bounds; (1) asks s >= etaSphere - eta
// of those bounds.
//
// Dmin: s is linear along the segment, from s0 >= -2 eta (a corner's -eta and the origin's own eta off its triangle) to s1 >= Dmin
// over a length <= L.  It can meet Y (|s| <= eta at Y's corners, checked) only where s <= eta: if s0 > eta nowhere at t > 0 short
// of the light; else it leaves the slab at t* = (eta - s0) L / (s1 - s0) <= 3 eta L / (Dmin - eta), which is 3/8 tnear with
//     Dmin = eta + 2 eta L x 4 / tnear
// (tnear / 4 for origins that are themselves within the slab).  The other tnear / 2 cover phase 2's own t for Y.  Origins with s0 <= Dmin / 2 climb at sin(phi) >= Dmin / (2 L): the true
// crossing is at t <= tnear / 4 (or behind the origin), the computed one at most
//     Et = 1.01 x 8 u (L + tnear) k(Y) / (Dmin / (2 L) - 8 u k(Y)) + u tnear
// further, and Et <= tnear / 2 is CHECKED per triangle (margin A).  Origins with s0 > Dmin / 2 stay above min(s0, s1) >= Dmin / 2
// all the way to the light: an accepted t <= distance would need N' / |det'| <= distance, i.e. min(s0, s1) |e1 x e2| <= |dN| +
// distance |dDet| <= 16 u L |e1||e2|; Dmin / 2 > 1.01 x 16 u L k(Y) is checked as well (margin B).  Emitters: a sample
// p0 a + p1 b + p2 c of the light's float corners is within 16 u M of their hull, a sphere light's within 16 u M of radius x 1.001
// of its centre: (2) is asked with that slack.  NaN, a degenerate Y, a failed margin, an environment light (its shadow rays have no end),
// a caller that cannot name the emitters: the triangle is an occluder.  A quad is a never-occluder when both halves are.
// Cornell (extent 3.49, camera 6.8 away, max k = 2.4): eta = 2.1e-5, Dmin = 0.59; the light is 1.98 / 0.82 / 0.77 / 0.78 from floor, back,
// right and left wall, 0.01 from the ceiling: 3 of the 17 quads and the two lone triangles.
//
// NEVER-HIT (smallNeverHit, buildSmallPassItems below).  Triangle k is never-hit when another triangle with a LOWER primitive id
// (the int in float 3 of the record, not the position in leafTris) has the same 36 bytes of (v0, e1, e2).  No tolerance is
// involved: intersectTriangle (trace.h) reads only those nine floats and the ray, so two records with the same bits give the
// same t, u, v -- or the same rejection -- on every ray.  The closest-hit rule (testLeafTriangle, smallResolveShared's `closer`)
// is "t < best, or t == best and a lower primitive id", independent of the order of the tests: of two copies the lower id
// wins whichever is met first.  An any-hit query is occluded by one copy exactly when it is by the other.  The higher-id copy
// therefore changes no hit record and no radiance sum, and the pass over all items may leave it out.  Bit patterns are compared,
// not values: +0 against -0 is not a copy (the products' signs of zero may differ), a record one ulp away is not, a rotated or
// reversed vertex order is not (other arithmetic), and a record holding a NaN is in no class.  Each class keeps its lowest id:
// three copies keep one.  Spheres are not considered.  CornellBox-Original.obj: each box's "Bottom Face" line names the four
// vertices of an earlier side face instead (f -12 -11 -10 -9, f -8 -7 -6 -5), so triangles 20, 21 are 16, 17 again and 32, 33
// are 30, 31: 2 of the 18 quads.
// The PASS LIST is buildSmallItems run a second time on the kept triangles alone -- records, item-ordered triangle copy and
// layout of its own, quads paired among kept triangles only -- and is what the non-counting parallelogram instantiations of
// k_path_small walk for a path vertex's two rays (kernels.h: kSmallPassList).  The item list above stays what it was: the camera
// masks are in ITS order (the refill resolves against it), the counting instantiations run it whole, and so does every other
// kernel.  The never-occluder rule of the pass list takes a kept triangle for an emitter when any member of its class emits: the
// removed copy's surface, where a light sample can land, is the kept triangle's surface.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace pathed {

static const int kSmallQuadWords = 16;        // float2 per packed PAIR of parallelograms: c0.xyz, a1.xyz, a2.xyz, K2uv, amax^2, K2t, -, cD, Edet, kappaUV
static const int kSmallLoneWords = 9;         // float2 per packed pair of lone triangles: v0.xyz, e1.xyz, e2.xyz (kSmallPairWords)
static const int kSmallItemFloats = 2 * 9 * 32;   // the kernarg array of SmallTris, in floats
static const float kSmallKappa = 1e-5f;       // relative slack of the barycentric bounds
static const float kSmallKappaFar = 1e-6f;    // relative slack of a shadow ray's far bound (its tolerance is tfarHigh x (kappaFar det^2 + cD))

struct SmallItemsLayout {
    int nQuads = 0;          // parallelograms: item-order triangles 2 q (A: beta <= alpha) and 2 q + 1 (B)
    int nLone = 0;           // triangles without a partner: item-order 2 nQuads + k
    float kappaT = 0.f;      // absolute slack of the t bounds per det^2 (a length): a sixteenth of tnear
    // never-occluders come last in both sections: the turns of phase 1 a SHADOW ray needs (an odd count of the others: the pair
    // that straddles the boundary is run for both rays)
    int shadowQuadPairs = 0; // <= (nQuads + 1) / 2
    int shadowLonePairs = 0; // <= (nLone + 1) / 2
    unsigned long long neverOccluders = 0ull;   // bit (original primitive id & 63)
    double eta = 0.0, dMin = 0.0;               // what the rule was run with (0: not run)
};

// Where the shadow rays of a scene end, for smallNeverOccluders.  known = false (the default): nothing is marked.
struct SmallLights {
    bool known = false;
    bool environment = false;               // an environment light: shadow rays without an end point
    const unsigned char *emitter = nullptr; // per triangle, in the order of leafTris: its material emits
    const float *spheres = nullptr;         // sphere lights: centre.xyz, radius
    int nSpheres = 0;
    int nSurfacePoints = 0;                 // the first extraPoints are surface bounds, (lo, hi) per sphere; the rest (the camera) are not
};

// marks[k] = 1: triangle k of leafTris can never occlude a shadow ray (header: NEVER-OCCLUDERS).  extraPoints as buildSmallItems takes them.
inline void smallNeverOccluders(const float *leafTris, int nTris, const float *extraPoints, int nExtra, const SmallLights &lights, float tnear,
                                std::vector<unsigned char> *marks, double *etaOut = nullptr, double *dMinOut = nullptr)
{
    marks->assign((size_t)std::max(nTris, 0), 0);
    if (etaOut) { *etaOut = 0.0; }
    if (dMinOut) { *dMinOut = 0.0; }
    if (!lights.known || lights.environment || nTris <= 0 || !lights.emitter || !(tnear > 0.f)) { return; }
    const double unit = 1.0 / 16777216.0;
    const int nSurface = std::min(std::max(lights.nSurfacePoints, 0), nExtra) & ~1;
    struct Tri { double p[3][3], k; };
    std::vector<Tri> tris((size_t)nTris);
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 }, sLo[3], sHi[3], largest = 0.0, kMax = 0.0;
    auto cover = [&](const double *point) {
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], point[a]); hi[a] = std::max(hi[a], point[a]); largest = std::max(largest, std::fabs(point[a])); }
    };
    auto cross = [](const double *a, const double *b, double *out) {
        out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
    };
    auto norm = [](const double *a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    for (int t = 0; t < nTris; t++) {
        const float *tri = leafTris + (size_t)12 * t;
        double e1[3], e2[3], n[3];
        for (int a = 0; a < 3; a++) {
            e1[a] = tri[4 + a]; e2[a] = tri[8 + a];
            tris[t].p[0][a] = tri[a]; tris[t].p[1][a] = (double)tri[a] + e1[a]; tris[t].p[2][a] = (double)tri[a] + e2[a];
        }
        for (int c = 0; c < 3; c++) { cover(tris[t].p[c]); }
        cross(e1, e2, n);
        const double area2 = norm(n), edges = norm(e1) * norm(e2);
        tris[t].k = area2 > 0.0 ? edges / area2 : 1e300;
        if (!(tris[t].k >= 1.0)) { tris[t].k = 1e300; }   // NaN
        if (!(edges == 0.0)) { kMax = std::max(kMax, tris[t].k); }   // (a triangle of zero edges has det = 0 exactly: never hit)
    }
    for (int i = 0; i < nSurface; i++) {
        const double point[3] = { extraPoints[3 * i], extraPoints[3 * i + 1], extraPoints[3 * i + 2] };
        cover(point);
    }
    for (int a = 0; a < 3; a++) { sLo[a] = lo[a]; sHi[a] = hi[a]; }
    for (int i = nSurface; i < nExtra; i++) {
        const double point[3] = { extraPoints[3 * i], extraPoints[3 * i + 1], extraPoints[3 * i + 2] };
        cover(point);
    }
    auto diagonal = [](const double *from, const double *to) {
        double sum = 0.0;
        for (int a = 0; a < 3; a++) { if (to[a] > from[a]) { sum += (to[a] - from[a]) * (to[a] - from[a]); } }
        return std::sqrt(sum) * 1.001;
    };
    const double R = diagonal(lo, hi), L = diagonal(sLo, sHi);
    const double eta = 1.01 * (unit * R + 16.0 * unit * R * kMax) + 1.01 * 3.0 * unit * (largest + R);
    const double etaSphere = 1.1 * std::sqrt(32.0 * unit) * R;   // beyond eta, for points found on spheres
    const double dMin = eta + 2.0 * eta * L * 4.0 / tnear;
    const double emitterSlack = 16.0 * unit * largest;
    if (!(eta > 0.0) || !(dMin > 0.0) || !(dMin < 1e300)) { return; }
    if (etaOut) { *etaOut = eta; }
    if (dMinOut) { *dMinOut = dMin; }
    bool anyEmitter = lights.nSpheres > 0;
    for (int t = 0; t < nTris; t++) { anyEmitter = anyEmitter || lights.emitter[t] != 0; }
    if (!anyEmitter) { return; }   // no shadow rays at all: nothing to gain

    for (int y = 0; y < nTris; y++) {
        const Tri &Y = tris[y];
        // margins A and B (header)
        const double climb = dMin / (2.0 * L) - 8.0 * unit * Y.k;
        if (!(climb > 0.0)) { continue; }
        const double eT = 1.01 * 8.0 * unit * (L + tnear) * Y.k / climb + unit * tnear;
        if (!(eT <= 0.5 * tnear)) { continue; }
        if (!(0.5 * dMin > 1.01 * 16.0 * unit * L * Y.k)) { continue; }
        double e1[3], e2[3], n[3];
        for (int a = 0; a < 3; a++) { e1[a] = Y.p[1][a] - Y.p[0][a]; e2[a] = Y.p[2][a] - Y.p[0][a]; }
        cross(e1, e2, n);
        const double length = norm(n);
        if (!(length > 1e-12 * norm(e1) * norm(e2)) || !(length > 0.0)) { continue; }   // degenerate
        for (int a = 0; a < 3; a++) { n[a] /= length; }
        for (int orientation = 0; orientation < 2 && !(*marks)[y]; orientation++) {
            const double sign = orientation ? -1.0 : 1.0;
            const double c = sign * (n[0] * Y.p[0][0] + n[1] * Y.p[0][1] + n[2] * Y.p[0][2]);
            auto s = [&](const double *x) { return sign * (n[0] * x[0] + n[1] * x[1] + n[2] * x[2]) - c; };
            bool holds = true;
            for (int corner = 0; corner < 3 && holds; corner++) { holds = std::fabs(s(Y.p[corner])) <= eta; }
            for (int t = 0; t < nTris && holds; t++) {
                for (int corner = 0; corner < 3 && holds; corner++) {
                    const double value = s(tris[t].p[corner]);
                    holds = value >= -eta && (!lights.emitter[t] || value >= dMin + emitterSlack);
                }
            }
            for (int i = 0; i + 1 < nSurface && holds; i += 2) {   // the least of s over a sphere's bounds
                const float *a = extraPoints + 3 * i, *b = a + 3;
                double least = -c;
                for (int x = 0; x < 3; x++) { least += std::min(sign * n[x] * (double)a[x], sign * n[x] * (double)b[x]); }
                holds = least >= etaSphere;
            }
            for (int i = 0; i < lights.nSpheres && holds; i++) {
                const float *sphere = lights.spheres + 4 * i;
                const double centre[3] = { sphere[0], sphere[1], sphere[2] };
                holds = s(centre) - std::fabs((double)sphere[3]) * 1.001 >= dMin + emitterSlack;
            }
            if (holds) { (*marks)[y] = 1; }
        }
    }
}

// leafTris: 12 floats per triangle, (v0, prim) (e1, -) (e2, -).  extraPoints: origins rays may have besides the triangles
// themselves (the camera; sphere bounds).  records: kSmallItemFloats floats, [pair of parallelograms][component][half], then
// the lone pairs as SmallTris stores them.  itemTris: the 12-float records again, in ITEM order (what phase 2 indexes).
// lights: where the scene's shadow rays end (SmallLights); without it no item is a never-occluder and the order is the former one.
inline SmallItemsLayout buildSmallItems(const float *leafTris, int nTris, const float *extraPoints, int nExtra, bool pairQuads, float tnear,
                                        float *records, std::vector<float> *itemTris, const SmallLights *lights = nullptr)
{
    SmallItemsLayout layout;
    std::memset(records, 0, sizeof(float) * kSmallItemFloats);
    itemTris->assign((size_t)12 * std::max(nTris, 1), 0.f);
    struct Corners { double p[3][3]; };
    std::vector<Corners> corners((size_t)nTris);
    double lo[3] = { 1e300, 1e300, 1e300 }, hi[3] = { -1e300, -1e300, -1e300 };
    auto cover = [&](const double *point) {
        for (int a = 0; a < 3; a++) { lo[a] = std::min(lo[a], point[a]); hi[a] = std::max(hi[a], point[a]); }
    };
    for (int k = 0; k < nTris; k++) {
        const float *tri = leafTris + (size_t)12 * k;
        for (int a = 0; a < 3; a++) {
            corners[k].p[0][a] = tri[a];
            corners[k].p[1][a] = (double)tri[a] + (double)tri[4 + a];   // the triangle the intersector sees: v0, v0 + e1, v0 + e2
            corners[k].p[2][a] = (double)tri[a] + (double)tri[8 + a];
        }
        for (int c = 0; c < 3; c++) { cover(corners[k].p[c]); }
    }
    for (int i = 0; i < nExtra; i++) {
        const double point[3] = { extraPoints[3 * i], extraPoints[3 * i + 1], extraPoints[3 * i + 2] };
        cover(point);
    }
    double diameter = 0.0;
    for (int a = 0; a < 3; a++) { if (hi[a] > lo[a]) { diameter += (hi[a] - lo[a]) * (hi[a] - lo[a]); } }
    diameter = std::sqrt(diameter) * 1.001;
    layout.kappaT = tnear / 16.f;

    auto distance = [](const double *a, const double *b) {
        return std::sqrt((a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]));
    };
    struct Quad { int a, b; double c0[3], a1[3], a2[3], delta, excess, amax; };
    std::vector<Quad> quads;
    std::vector<int> partner((size_t)nTris, -1);
    const double unit = 1.0 / 16777216.0;
    for (int a = 0; pairQuads && a < nTris; a++) {
        if (partner[a] >= 0) { continue; }
        for (int b = a + 1; b < nTris; b++) {
            if (partner[b] >= 0) { continue; }
            // two shared corners (the diagonal), within a few ulps of the scene's size
            const double same = 8.0 * unit * diameter;
            int sharedA[2], sharedB[2], nShared = 0;
            bool usedB[3] = { false, false, false };
            for (int i = 0; i < 3 && nShared <= 2; i++) {
                for (int j = 0; j < 3; j++) {
                    if (!usedB[j] && distance(corners[a].p[i], corners[b].p[j]) <= same) {
                        if (nShared < 2) { sharedA[nShared] = i; sharedB[nShared] = j; }
                        nShared++;
                        usedB[j] = true;
                        break;
                    }
                }
            }
            if (nShared != 2) { continue; }
            const int restA = 3 - sharedA[0] - sharedA[1], restB = 3 - sharedB[0] - sharedB[1];
            const double *rA = corners[a].p[restA], *rB = corners[b].p[restB];
            // Either end of the diagonal may be the origin c0.  With the diagonal's other end at c0 + alpha2 (rA - c0) + beta2
            // (rB - c0), the edges a1 = alpha2 (rA - c0), a2 = beta2 (rB - c0) put it at (1, 1): triangle A = (c0, rA, far end) is
            // the part beta <= alpha of the quad, B the part alpha <= beta, and the quad lies in [0, max(1, 1 / alpha2)] x
            // [0, max(1, 1 / beta2)].  A parallelogram has alpha2 = beta2 = 1; a planar quad that is nearly one (the walls of the
            // Cornell box are trapezoids, 0.6 % off) sticks out of the unit square by `excess`, which joins the relative slack of
            // the box test.  Take the origin with the smaller excess; quads further off than 5 % are left alone.
            Quad quad;
            quad.a = a; quad.b = b;
            double bestExcess = 1e300, delta = 0.0, amax = 0.0;
            for (int end = 0; end < 2; end++) {
                const double *d0 = corners[a].p[sharedA[end]], *d1 = corners[a].p[sharedA[1 - end]];
                const double *d0b = corners[b].p[sharedB[end]], *d1b = corners[b].p[sharedB[1 - end]];
                double e1[3], e2[3], g[3];
                for (int x = 0; x < 3; x++) { e1[x] = rA[x] - d0[x]; e2[x] = rB[x] - d0[x]; g[x] = d1[x] - d0[x]; }
                // least squares g = alpha2 e1 + beta2 e2
                const double m11 = e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2], m22 = e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2];
                const double m12 = e1[0] * e2[0] + e1[1] * e2[1] + e1[2] * e2[2];
                const double r1 = e1[0] * g[0] + e1[1] * g[1] + e1[2] * g[2], r2 = e2[0] * g[0] + e2[1] * g[1] + e2[2] * g[2];
                const double determinant = m11 * m22 - m12 * m12;
                if (!(determinant > 1e-12 * m11 * m22)) { continue; }   // rA, c0, rB on a line
                const double alpha2 = (r1 * m22 - r2 * m12) / determinant, beta2 = (r2 * m11 - r1 * m12) / determinant;
                if (!(alpha2 > 0.5 && beta2 > 0.5)) { continue; }
                const double excess = std::max(std::max(1.0 / alpha2, 1.0 / beta2), 1.0) - 1.0;
                if (!(excess < bestExcess)) { continue; }
                Quad candidate = quad;
                for (int x = 0; x < 3; x++) {
                    candidate.c0[x] = (float)d0[x];
                    candidate.a1[x] = (float)(alpha2 * e1[x]);
                    candidate.a2[x] = (float)(beta2 * e2[x]);
                }
                // where the stored (float) parallelogram puts the six corners of the two triangles, against where they are
                double worst = 0.0, longest = 0.0;
                auto place = [&](double alpha, double beta, double *out) {
                    for (int x = 0; x < 3; x++) { out[x] = candidate.c0[x] + alpha * candidate.a1[x] + beta * candidate.a2[x]; }
                };
                double q[3];
                place(0.0, 0.0, q); worst = std::max(worst, std::max(distance(d0, q), distance(d0b, q)));
                place(1.0, 1.0, q); worst = std::max(worst, std::max(distance(d1, q), distance(d1b, q)));
                place(1.0 / alpha2, 0.0, q); worst = std::max(worst, distance(rA, q));
                place(0.0, 1.0 / beta2, q); worst = std::max(worst, distance(rB, q));
                const double zero[3] = { 0.0, 0.0, 0.0 };
                longest = std::max(std::max(distance(candidate.a1, zero), distance(candidate.a2, zero)), std::max(distance(d1, d0), distance(rA, rB)));
                candidate.excess = excess;
                quad = candidate;
                bestExcess = excess;
                delta = worst;
                amax = longest;
            }
            if (!(bestExcess <= 0.05)) { continue; }
            // planar and where the parallelogram says, up to rounding
            if (!(delta <= 64.0 * unit * std::max(amax, 1e-30))) { continue; }
            // ... and small enough for the interval test to mean something: a ray that leaves the quad itself sees it at t = 0
            // +- the t tolerance, which for an origin on the quad (|o - c0| <= amax) at cos(theta) = 1/4 is
            // 1.5 (32 u)^2 4 amax^2 / (2 kappa_t) x 16; beyond tnear / 4 the quad would be a candidate of most rays that leave it
            {
                const double kappaT = tnear / 16.0;
                const double selfTolerance = 1.5 * (32.0 * unit) * (32.0 * unit) * 4.0 * amax * amax / (2.0 * kappaT) * 16.0;
                if (!(selfTolerance <= tnear / 4.0)) { continue; }
            }
            quad.amax = amax;
            quad.delta = delta;
            partner[a] = b;
            partner[b] = a;
            quads.push_back(quad);
            break;
        }
    }
    // the kernarg array holds 32 lone pairs; a pair of parallelograms takes 12 of its float2 where two lone pairs take 18, but an
    // odd count leaves half a packed pair unused: drop parallelograms until everything fits (only scenes of 62+ triangles can need it)
    auto floatsNeeded = [&](size_t nQuads) {
        return (size_t)2 * kSmallQuadWords * ((nQuads + 1) / 2) + (size_t)2 * kSmallLoneWords * (((size_t)nTris - 2 * nQuads + 1) / 2);
    };
    while (!quads.empty() && floatsNeeded(quads.size()) > (size_t)kSmallItemFloats) {
        partner[quads.back().a] = -1;
        partner[quads.back().b] = -1;
        quads.pop_back();
    }
    layout.nQuads = (int)quads.size();
    layout.nLone = nTris - 2 * layout.nQuads;

    // ---- never-occluders last, in both sections (header); the order within each group stays what it was
    std::vector<unsigned char> never;
    smallNeverOccluders(leafTris, nTris, extraPoints, nExtra, lights ? *lights : SmallLights(), tnear, &never, &layout.eta, &layout.dMin);
    auto neverQuad = [&](const Quad &quad) { return never[quad.a] && never[quad.b]; };
    std::stable_partition(quads.begin(), quads.end(), [&](const Quad &quad) { return !neverQuad(quad); });
    int occluderQuads = 0, occluderLone = 0;
    for (const Quad &quad : quads) { occluderQuads += neverQuad(quad) ? 0 : 1; }
    std::vector<int> loneOrder;
    for (int pass = 0; pass < 2; pass++) {
        for (int t = 0; t < nTris; t++) {
            if (partner[t] < 0 && (never[t] != 0) == (pass == 1)) { loneOrder.push_back(t); }
        }
        if (pass == 0) { occluderLone = (int)loneOrder.size(); }
    }
    layout.shadowQuadPairs = (occluderQuads + 1) / 2;
    layout.shadowLonePairs = (occluderLone + 1) / 2;
    auto primitive = [&](int t) { int id; std::memcpy(&id, leafTris + (size_t)12 * t + 3, sizeof id); return id; };
    for (int q = occluderQuads; q < layout.nQuads; q++) { layout.neverOccluders |= 1ull << (primitive(quads[q].a) & 63) | 1ull << (primitive(quads[q].b) & 63); }
    for (int k = occluderLone; k < layout.nLone; k++) { layout.neverOccluders |= 1ull << (primitive(loneOrder[k]) & 63); }

    // ---- records
    const double kappa = kSmallKappa, kappaT = layout.kappaT;
    for (int q = 0; q < layout.nQuads; q++) {
        const Quad &quad = quads[q];
        float *record = records + (size_t)2 * kSmallQuadWords * (q / 2);   // kSmallQuadWords float2 per packed pair
        const int half = q & 1;
        const double zero[3] = { 0.0, 0.0, 0.0 };
        const double amax = quad.amax;
        // errors per unit of r = |o - c0| + amax (header)
        const double eUV = 1.01 * (32.0 * unit * amax + 4.0 * quad.delta);
        // (t det and det are products of BOTH edges: |a1||a2| bounds them, which for a long thin plate is far below amax^2)
        const double area = distance(quad.a1, zero) * distance(quad.a2, zero);
        const double eT = 1.01 * (32.0 * unit * area + 8.0 * quad.delta * amax);
        const double eDet = 1.01 * (16.0 * unit * area + 4.0 * quad.delta * amax);
        // ... plus what covers a det too small to trust its sign (|det| <= E_det): there every bound X det is at most
        // Xmax E_det in size, Xmax = |o - c0| amax (u, v) or |o - c0| |a1||a2| (t), and |o - c0| <= (|o - c0|^2 / amax + amax) / 2:
        // a second pair of (K2, K0) terms, folded into the first -- no test of |det| in the kernel
        const double k2UV = 1.5 * (eUV * eUV / (2.0 * kappa) + eDet / 2.0);
        const double k2T = 1.5 * (eT * eT / (2.0 * std::max(kappaT, 1e-300)) + eDet * area / (2.0 * std::max(amax, 1e-300)));
        const double cD = 1.5 * eDet * eDet / (4.0 * kSmallKappaFar);
        for (int x = 0; x < 3; x++) {
            record[2 * (0 + x) + half] = (float)quad.c0[x];
            record[2 * (3 + x) + half] = (float)quad.a1[x];
            record[2 * (6 + x) + half] = (float)quad.a2[x];
        }
        record[2 * 9 + half] = (float)std::max(k2UV, 1e-37);
        record[2 * 10 + half] = (float)std::max(amax * amax * 1.000001, 1e-37);   // K0 = K2 amax^2: the kernel multiplies K2 by (|o - c0|^2 + amax^2)
        record[2 * 11 + half] = (float)std::max(k2T, 1e-37);
        record[2 * 13 + half] = (float)std::max(cD, 1e-37);
        record[2 * 14 + half] = (float)std::max(eDet, 1e-37);
        record[2 * 15 + half] = (float)(kappa + 1.0001 * quad.excess);   // relative slack of the box test: kappa + how far the quad sticks out
        std::memcpy(itemTris->data() + (size_t)12 * (2 * q), leafTris + (size_t)12 * quad.a, 12 * sizeof(float));
        std::memcpy(itemTris->data() + (size_t)12 * (2 * q + 1), leafTris + (size_t)12 * quad.b, 12 * sizeof(float));
    }
    float *lone = records + (size_t)2 * kSmallQuadWords * ((layout.nQuads + 1) / 2);
    int k = 0;
    for (int t : loneOrder) {
        const float *tri = leafTris + (size_t)12 * t;
        float *record = lone + (size_t)2 * kSmallLoneWords * (k / 2);
        for (int row = 0; row < 3; row++) {
            for (int axis = 0; axis < 3; axis++) { record[2 * (3 * row + axis) + (k & 1)] = tri[4 * row + axis]; }
        }
        std::memcpy(itemTris->data() + (size_t)12 * (2 * layout.nQuads + k), tri, 12 * sizeof(float));
        k++;
    }
    return layout;
}

// marks[k] = 1: triangle k of leafTris is NEVER-HIT (header).  keeper[k]: the triangle of leafTris that stands for k's class,
// the member with the lowest primitive id (k itself where k has no copy, or holds a NaN).
inline void smallNeverHit(const float *leafTris, int nTris, std::vector<unsigned char> *marks, std::vector<int> *keeper = nullptr)
{
    marks->assign((size_t)std::max(nTris, 0), 0);
    std::vector<int> lowest((size_t)std::max(nTris, 0));
    auto primitive = [&](int t) { int id; std::memcpy(&id, leafTris + (size_t)12 * t + 3, sizeof id); return id; };
    auto sameBits = [&](int a, int b) {   // the 36 bytes of (v0, e1, e2): bit patterns, so +0 is not -0 and a NaN could equal itself...
        for (int row = 0; row < 3; row++) {
            if (std::memcmp(leafTris + (size_t)12 * a + 4 * row, leafTris + (size_t)12 * b + 4 * row, 3 * sizeof(float)) != 0) { return false; }
        }
        return true;
    };
    auto hasNan = [&](int t) {   // ... which is why such a record is left out of every class
        for (int row = 0; row < 3; row++) {
            for (int a = 0; a < 3; a++) { if (std::isnan(leafTris[(size_t)12 * t + 4 * row + a])) { return true; } }
        }
        return false;
    };
    for (int k = 0; k < nTris; k++) {
        lowest[(size_t)k] = k;
        if (hasNan(k)) { continue; }
        for (int other = 0; other < nTris; other++) {
            if (other != k && !hasNan(other) && sameBits(k, other) && primitive(other) < primitive(lowest[(size_t)k])) { lowest[(size_t)k] = other; }
        }
        // (two records of one primitive id cannot both be the lowest: neither is marked, both stay)
        if (lowest[(size_t)k] != k) { (*marks)[(size_t)k] = 1; }
    }
    if (keeper) { *keeper = lowest; }
}

// The PASS LIST (header: NEVER-HIT): buildSmallItems over the triangles that are not never-hit, in the order leafTris has them.
// passTris is the item-ordered copy of THOSE triangles (what phase 2 of the pass indexes); the layout counts them:
// 2 nQuads + nLone = *nPass <= nTris.  A kept triangle counts as an emitter when any member of its class emits (a light sample
// can land on the removed copy's surface, which is the kept one's).  neverHit: bit (original primitive id & 63) of every
// triangle left out.  A scene without copies gets what buildSmallItems gives it, byte for byte.
inline SmallItemsLayout buildSmallPassItems(const float *leafTris, int nTris, const float *extraPoints, int nExtra, bool pairQuads, float tnear,
                                            float *records, std::vector<float> *passTris, const SmallLights *lights, int *nPass,
                                            unsigned long long *neverHit = nullptr)
{
    std::vector<unsigned char> marks, emitter;
    std::vector<int> keeper;
    smallNeverHit(leafTris, nTris, &marks, &keeper);
    std::vector<float> kept;
    std::vector<int> place((size_t)std::max(nTris, 0), -1);   // where triangle k went in `kept`
    unsigned long long word = 0ull;
    for (int k = 0; k < nTris; k++) {
        if (marks[(size_t)k]) {
            int id;
            std::memcpy(&id, leafTris + (size_t)12 * k + 3, sizeof id);
            word |= 1ull << (id & 63);
            continue;
        }
        place[(size_t)k] = (int)(kept.size() / 12);
        kept.insert(kept.end(), leafTris + (size_t)12 * k, leafTris + (size_t)12 * (k + 1));
    }
    const int count = (int)(kept.size() / 12);
    SmallLights passLights = lights ? *lights : SmallLights();
    if (passLights.emitter) {
        emitter.assign((size_t)std::max(count, 1), 0);
        for (int k = 0; k < nTris; k++) {
            if (passLights.emitter[k]) { emitter[(size_t)place[(size_t)keeper[(size_t)k]]] = 1; }
        }
        passLights.emitter = emitter.data();
    }
    if (nPass) { *nPass = count; }
    if (neverHit) { *neverHit = word; }
    return buildSmallItems(kept.data(), count, extraPoints, nExtra, pairQuads, tnear, records, passTris, lights ? &passLights : nullptr);
}

}  // namespace pathed
