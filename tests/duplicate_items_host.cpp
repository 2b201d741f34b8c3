// Stand-alone check of the never-hit rule and the pass list it drives (pathed_amd/csrc/small_items.h: smallNeverHit,
// buildSmallPassItems) on the host.  Random rooms -- five walls, boxes, loose triangles, a light, in random frames -- get copies
// of some triangles: a triple, a copy with another material, an emitting copy of a non-emitting triangle, a copy whose quad
// partner is not copied, and the near misses that are NOT copies: rotated and reversed vertex order, one ulp off, -0 for +0,
// records holding a NaN.  The triangles reach the rule in a shuffled order, so that the primitive id and not the position
// decides which member of a class stays.  Per room: the marks (each case asserted), the pass list as a permutation of the kept
// triangles that keeps quads together and puts the never-occluders last, and the brute-force check: over random rays and rays
// through the copied triangles' corners and edges, the closest hit by the acceptance rule of the intersector over ALL triangles
// equals the closest hit over the pass list in (t, u, v, prim) bits, and occlusion is equal likewise.  Then the Cornell file, a
// scene without copies (byte-identical lists), and the emitter case.  Exit status 1 on any failure.
//   g++ -std=c++17 -O1 -iquote pathed_amd/csrc tests/duplicate_items_host.cpp -o duplicate_items_host
//   duplicate_items_host <rooms> <random rays per room> <path of CornellBox-Original.obj>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "small_items.h"

using namespace pathed;

static const float kTnear = 1e-3f;

struct Tri {
    float v0[3], e1[3], e2[3];
    bool emits;
    int material;
};

struct Scene {
    std::vector<Tri> tris;                // index = primitive id
    std::vector<int> order;               // position in leaf -> primitive id
    std::vector<float> leaf;              // 12 floats per triangle: (v0, prim) (e1, -) (e2, -)
    std::vector<unsigned char> emitter;   // in the order of leaf
    std::vector<float> extra;             // the camera

    int count() const { return (int)tris.size(); }
    int triangle(const double *p0, const double *p1, const double *p2, bool emits, int material = 0)
    {
        Tri t;
        for (int a = 0; a < 3; a++) {
            t.v0[a] = (float)p0[a];
            t.e1[a] = (float)p1[a] - (float)p0[a];
            t.e2[a] = (float)p2[a] - (float)p0[a];
        }
        t.emits = emits;
        t.material = material;
        tris.push_back(t);
        return count() - 1;
    }
    int quad(const double *p0, const double *p1, const double *p2, const double *p3, bool emits, int material = 0)
    {
        const int first = triangle(p0, p1, p2, emits, material);
        triangle(p0, p2, p3, emits, material);
        return first;
    }
    int copy(int source, bool emits, int material)
    {
        Tri t = tris[(size_t)source];
        t.emits = emits;
        t.material = material;
        tris.push_back(t);
        return count() - 1;
    }
    // the records in the order `order` gives (identity when it is empty)
    void finish()
    {
        if (order.empty()) { for (int k = 0; k < count(); k++) { order.push_back(k); } }
        leaf.assign((size_t)12 * count(), 0.f);
        emitter.assign((size_t)count(), 0);
        for (int k = 0; k < count(); k++) {
            const int prim = order[(size_t)k];
            const Tri &t = tris[(size_t)prim];
            float *record = &leaf[(size_t)12 * k];
            for (int a = 0; a < 3; a++) { record[a] = t.v0[a]; record[4 + a] = t.e1[a]; record[8 + a] = t.e2[a]; }
            std::memcpy(&record[3], &prim, sizeof prim);
            emitter[(size_t)k] = t.emits ? 1 : 0;
        }
    }
    SmallLights lights() const
    {
        SmallLights l;
        l.known = true;
        l.emitter = emitter.data();
        return l;
    }
};

struct Random {
    std::mt19937_64 engine;
    explicit Random(unsigned long long seed) : engine(seed) {}
    double unit() { return std::uniform_real_distribution<double>(0.0, 1.0)(engine); }
    double range(double lo, double hi) { return lo + (hi - lo) * unit(); }
    int below(int n) { return (int)(engine() % (unsigned long long)n); }
};

struct Tally {
    long long rooms = 0, copies = 0, rays = 0, hits = 0, hitsOnClasses = 0, occluded = 0, mismatches = 0, checks = 0, failures = 0;
};

#define EXPECT(condition) do { tally.checks++; if (!(condition)) { tally.failures++; std::printf("FAILED line %d: %s\n", __LINE__, #condition); } } while (0)

// ---- intersectTriangle's arithmetic and the acceptance rule, as the oracle states them (oracle/oracle.cpp; trace.h)
static float xdot(const float *a, const float *b) { return std::fmaf(a[0], b[0], std::fmaf(a[1], b[1], a[2] * b[2])); }
static void xcross(const float *a, const float *b, float *out)
{
    out[0] = std::fmaf(a[1], b[2], -(a[2] * b[1]));
    out[1] = std::fmaf(a[2], b[0], -(a[0] * b[2]));
    out[2] = std::fmaf(a[0], b[1], -(a[1] * b[0]));
}
static bool intersectTriangle(const float *o, const float *d, const float *record, float *t, float *u, float *v)
{
    const float *v0 = record, *e1 = record + 4, *e2 = record + 8;
    float pvec[3], tvec[3], qvec[3];
    xcross(d, e2, pvec);
    const float det = xdot(e1, pvec);
    for (int a = 0; a < 3; a++) { tvec[a] = o[a] - v0[a]; }
    const float uScaled = xdot(tvec, pvec);
    xcross(tvec, e1, qvec);
    const float vScaled = xdot(d, qvec);
    if (det > 0.f) {
        if (!(uScaled >= 0.f && vScaled >= 0.f && uScaled + vScaled <= det)) { return false; }
    } else if (det < 0.f) {
        if (!(uScaled <= 0.f && vScaled <= 0.f && uScaled + vScaled >= det)) { return false; }
    } else {
        return false;
    }
    const float inv = 1.f / det;
    *t = xdot(e2, qvec) * inv;
    *u = uScaled * inv;
    *v = vScaled * inv;
    return true;
}

struct Hit { float t, u, v; int prim; };

static Hit closestHit(const float *records, int n, const float *o, const float *d, float tfar, bool backwards)
{
    Hit hit = { tfar, 0.f, 0.f, -1 };
    for (int i = 0; i < n; i++) {
        const float *record = records + (size_t)12 * (backwards ? n - 1 - i : i);
        float t, u, v;
        if (!intersectTriangle(o, d, record, &t, &u, &v) || !(t > kTnear)) { continue; }
        int prim;
        std::memcpy(&prim, record + 3, sizeof prim);
        const bool closer = hit.prim < 0 ? t <= hit.t : (t < hit.t || (t == hit.t && prim < hit.prim));
        if (closer) { hit.t = t; hit.u = u; hit.v = v; hit.prim = prim; }
    }
    return hit;
}

static bool occluded(const float *records, int n, const float *o, const float *d, float tfar)
{
    for (int i = 0; i < n; i++) {
        float t, u, v;
        if (intersectTriangle(o, d, records + (size_t)12 * i, &t, &u, &v) && t > kTnear && t <= tfar) { return true; }
    }
    return false;
}

static bool sameHit(const Hit &a, const Hit &b)
{
    return std::memcmp(&a.t, &b.t, sizeof(float)) == 0 && std::memcmp(&a.u, &b.u, sizeof(float)) == 0 && std::memcmp(&a.v, &b.v, sizeof(float)) == 0 && a.prim == b.prim;
}

// a point of primitive `prim` in float arithmetic: corners and edges over-represented
static void pointOn(const Scene &scene, int prim, Random &rng, int kind, float *out)
{
    float a = (float)rng.unit(), b = (float)rng.unit();
    if (a + b > 1.f) { a = 1.f - a; b = 1.f - b; }
    if (kind == 0) { a = (float)rng.below(2); b = a == 1.f ? 0.f : (float)rng.below(2); }   // a corner
    else if (kind == 1) { b = 0.f; }                                                          // an edge
    else if (kind == 2) { a = 0.f; }
    else if (kind == 3) { b = 1.f - a; }
    else if (kind == 4) { a *= 1e-6f; b *= 1e-6f; }                                           // a hair from a corner
    const Tri &t = scene.tris[(size_t)prim];
    for (int x = 0; x < 3; x++) { out[x] = t.v0[x] + a * t.e1[x] + b * t.e2[x]; }
}

static int primOf(const std::vector<float> &items, int k)
{
    int prim;
    std::memcpy(&prim, &items[(size_t)12 * k + 3], sizeof prim);
    return prim;
}

struct PassList {
    std::vector<float> records, tris;
    SmallItemsLayout layout;
    int count = 0;
    unsigned long long neverHit = 0ull;
};

static PassList passList(const Scene &scene)
{
    PassList list;
    list.records.assign((size_t)kSmallItemFloats, 0.f);
    const SmallLights lights = scene.lights();
    list.layout = buildSmallPassItems(scene.leaf.data(), scene.count(), scene.extra.data(), (int)(scene.extra.size() / 3), true, kTnear, list.records.data(),
                                      &list.tris, &lights, &list.count, &list.neverHit);
    return list;
}

// the pass list is a permutation of the kept triangles in which the two triangles of a quad share an edge, with the never-occluders last
static void checkPassList(const Scene &scene, const std::vector<unsigned char> &expected, const PassList &list, Tally &tally)
{
    int kept = 0;
    unsigned long long word = 0ull;
    for (int prim = 0; prim < scene.count(); prim++) {
        if (expected[(size_t)prim]) { word |= 1ull << (prim & 63); } else { kept++; }
    }
    EXPECT(list.count == kept);
    EXPECT(list.neverHit == word);
    EXPECT(2 * list.layout.nQuads + list.layout.nLone == list.count);
    EXPECT((int)list.tris.size() >= 12 * list.count);
    if (list.count != kept || (int)list.tris.size() < 12 * list.count) { return; }
    std::vector<int> seen((size_t)scene.count(), 0), position((size_t)scene.count(), -1);
    for (int k = 0; k < scene.count(); k++) { position[(size_t)scene.order[(size_t)k]] = k; }
    for (int k = 0; k < list.count; k++) {
        const int prim = primOf(list.tris, k);
        EXPECT(prim >= 0 && prim < scene.count());
        if (prim < 0 || prim >= scene.count()) { continue; }
        seen[(size_t)prim]++;
        EXPECT(std::memcmp(&list.tris[(size_t)12 * k], &scene.leaf[(size_t)12 * position[(size_t)prim]], 12 * sizeof(float)) == 0);
    }
    for (int prim = 0; prim < scene.count(); prim++) { EXPECT(seen[(size_t)prim] == (expected[(size_t)prim] ? 0 : 1)); }
    auto corner = [&](int prim, int which, double *out) {
        const Tri &t = scene.tris[(size_t)prim];
        for (int a = 0; a < 3; a++) { out[a] = (double)t.v0[a] + (which == 1 ? (double)t.e1[a] : which == 2 ? (double)t.e2[a] : 0.0); }
    };
    for (int q = 0; q < list.layout.nQuads; q++) {
        int shared = 0;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) {
                double a[3], b[3];
                corner(primOf(list.tris, 2 * q), i, a); corner(primOf(list.tris, 2 * q + 1), j, b);
                const double d[3] = { a[0] - b[0], a[1] - b[1], a[2] - b[2] };
                if (std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) < 1e-5) { shared++; }
            }
        }
        EXPECT(shared == 2);
    }
    int occluderQuads = 0, occluderLone = 0;
    bool sorted = true;
    for (int q = 0; q < list.layout.nQuads; q++) {
        const bool never = (list.layout.neverOccluders >> primOf(list.tris, 2 * q) & 1) && (list.layout.neverOccluders >> primOf(list.tris, 2 * q + 1) & 1);
        if (!never) { sorted = sorted && occluderQuads == q; occluderQuads++; }
    }
    for (int k = 0; k < list.layout.nLone; k++) {
        const bool never = list.layout.neverOccluders >> primOf(list.tris, 2 * list.layout.nQuads + k) & 1;
        if (!never) { sorted = sorted && occluderLone == k; occluderLone++; }
    }
    EXPECT(sorted);
    EXPECT(list.layout.shadowQuadPairs == (occluderQuads + 1) / 2);
    EXPECT(list.layout.shadowLonePairs == (occluderLone + 1) / 2);
    EXPECT((list.layout.neverOccluders & list.neverHit) == 0ull);
}

// One random room: [0, w] x [0, h] x [0, d] in a random frame, with the copies and near-copies of the header.
static void randomRoom(Random &rng, int nRays, int index, Tally &tally)
{
    const double size = std::pow(10.0, rng.range(-0.3, 0.6));
    const double dims[3] = { size * rng.range(0.7, 1.3), size * rng.range(0.7, 1.3), size * rng.range(0.7, 1.3) };
    double frame[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
    double offset[3] = { 0.0, 0.0, 0.0 };
    if (index % 3 != 0) {   // (every third room stays on the axes, at the origin: zeros among its coordinates)
        double x[3], y[3], z[3];
        auto cross = [](const double *a, const double *b, double *out) {
            out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
        };
        auto norm = [](const double *a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
        do { for (int a = 0; a < 3; a++) { x[a] = rng.range(-1, 1); y[a] = rng.range(-1, 1); } cross(x, y, z); } while (norm(z) < 0.2 || norm(x) < 0.2);
        const double lx = norm(x), lz = norm(z);
        for (int a = 0; a < 3; a++) { x[a] /= lx; z[a] /= lz; }
        cross(z, x, y);
        for (int a = 0; a < 3; a++) { frame[0][a] = x[a]; frame[1][a] = y[a]; frame[2][a] = z[a]; offset[a] = rng.range(-2, 2) * size; }
    }
    auto place = [&](double lx, double ly, double lz, double *out) {
        for (int a = 0; a < 3; a++) { out[a] = offset[a] + lx * frame[0][a] + ly * frame[1][a] + lz * frame[2][a]; }
    };
    Scene scene;
    // walls (open towards the camera), one of them as two triangles that do not pair up
    for (int axis = 0; axis < 3; axis++) {
        for (int side = 0; side < 2; side++) {
            if (axis == 2 && side == 1) { continue; }
            const int b = (axis + 1) % 3, c = (axis + 2) % 3;
            const double corners[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
            double local[4][3], world[4][3];
            const int start = rng.below(4);
            for (int k = 0; k < 4; k++) {
                const double *uv = corners[(k + start) & 3];
                local[k][axis] = side == 0 ? 0.0 : dims[axis]; local[k][b] = uv[0] * dims[b]; local[k][c] = uv[1] * dims[c];
                place(local[k][0], local[k][1], local[k][2], world[k]);
            }
            if (axis == 0 && side == 1 && rng.below(2)) {
                scene.triangle(world[0], world[1], world[3], false, 1);
                scene.triangle(world[2], world[3], world[1], false, 1);
            } else {
                scene.quad(world[0], world[1], world[2], world[3], false, 1 + axis);
            }
        }
    }
    std::vector<int> faces;   // first triangle of every box face (a quad)
    const int nBoxes = 1 + rng.below(2);
    for (int k = 0; k < nBoxes; k++) {
        const double x0 = rng.range(0.1, 0.6) * dims[0], z0 = rng.range(0.1, 0.6) * dims[2];
        const double x1 = x0 + rng.range(0.05, 0.3) * dims[0], z1 = z0 + rng.range(0.05, 0.3) * dims[2], y1 = rng.range(0.1, 0.5) * dims[1];
        const double y0 = rng.below(2) ? 0.0 : rng.range(0.0, 0.2) * dims[1];
        double p[8][3];
        const double lx[2] = { x0, x1 }, ly[2] = { y0, y1 }, lz[2] = { z0, z1 };
        for (int i = 0; i < 8; i++) { place(lx[i & 1], ly[(i >> 1) & 1], lz[(i >> 2) & 1], p[i]); }
        faces.push_back(scene.quad(p[2], p[3], p[7], p[6], false, 4));
        faces.push_back(scene.quad(p[0], p[1], p[3], p[2], false, 4));
        faces.push_back(scene.quad(p[1], p[5], p[7], p[3], false, 4));
        faces.push_back(scene.quad(p[4], p[5], p[7], p[6], false, 4));
    }
    std::vector<int> loose;
    const int nLoose = 2 + rng.below(3);
    for (int k = 0; k < nLoose; k++) {
        double p[3][3];
        for (int i = 0; i < 3; i++) { place(rng.range(0.05, 0.95) * dims[0], rng.range(0.05, 0.95) * dims[1], rng.range(0.05, 0.95) * dims[2], p[i]); }
        loose.push_back(scene.triangle(p[0], p[1], p[2], false, 5));
    }
    {   // the light, under the ceiling
        double p[4][3];
        const double h = 0.1 * size, y = 0.9 * dims[1];
        place(0.5 * dims[0] - h, y, 0.5 * dims[2] - h, p[0]); place(0.5 * dims[0] + h, y, 0.5 * dims[2] - h, p[1]);
        place(0.5 * dims[0] + h, y, 0.5 * dims[2] + h, p[2]); place(0.5 * dims[0] - h, y, 0.5 * dims[2] + h, p[3]);
        scene.quad(p[0], p[1], p[2], p[3], true, 6);
    }
    const int originals = scene.count();
    std::vector<unsigned char> expected;   // per primitive id
    std::vector<int> classes;              // primitives that have a copy (the kept members)
    auto exact = [&](int source, bool emits, int material) {
        const int id = scene.copy(source, emits, material);
        expected.resize((size_t)scene.count(), 0);
        expected[(size_t)id] = 1;
        classes.push_back(source);
        tally.copies++;
        return id;
    };
    auto notACopy = [&](const Tri &t) {
        scene.tris.push_back(t);
        expected.resize((size_t)scene.count(), 0);
        return scene.count() - 1;
    };
    expected.assign((size_t)originals, 0);
    // a triple of a box face's triangle, and the face's other triangle once
    exact(faces[0], false, 4); exact(faces[0], false, 4); exact(faces[0] + 1, false, 4);
    // a copy with another material
    exact(faces[1], false, 9); exact(faces[1] + 1, false, 9);
    // an emitting copy of a non-emitting triangle
    exact(faces[2], true, 6);
    // a copy whose quad partner is not copied: half of a wall
    exact(2 * rng.below(2), false, 1);
    // a copied lone triangle
    exact(loose[0], false, 5);
    // ... and what is not a copy
    {
        const Tri source = scene.tris[(size_t)faces[3]];
        Tri rotated = source, reversed = source, ulp = source;
        for (int a = 0; a < 3; a++) {
            rotated.v0[a] = source.v0[a] + source.e1[a];
            rotated.e1[a] = (source.v0[a] + source.e2[a]) - rotated.v0[a];
            rotated.e2[a] = source.v0[a] - rotated.v0[a];
            reversed.e1[a] = source.e2[a]; reversed.e2[a] = source.e1[a];
        }
        const int component = rng.below(9);
        float *word = component < 3 ? &ulp.v0[component] : component < 6 ? &ulp.e1[component - 3] : &ulp.e2[component - 6];
        *word = std::nextafterf(*word, rng.below(2) ? 1e30f : -1e30f);
        notACopy(rotated); notACopy(reversed); notACopy(ulp);
        // -0 for +0: a triangle with a +0 among its nine floats, and the same with -0 there
        Tri zero = scene.tris[(size_t)loose[1]];
        zero.e1[1] = 0.f;
        Tri minusZero = zero;
        minusZero.e1[1] = -0.f;
        notACopy(zero); notACopy(minusZero);
        if (index % 2 == 1) {   // records holding a NaN, bit for bit the same: in no class (every other room: a NaN among the bounds pairs no quads)
            Tri broken = scene.tris[(size_t)loose[1]];
            broken.v0[rng.below(3)] = std::nanf("");
            notACopy(broken); notACopy(broken);
        }
    }
    if (scene.count() > 64) { return; }
    // the order the rule sees: shuffled, so that a copy may stand before the triangle it copies
    for (int k = 0; k < scene.count(); k++) { scene.order.push_back(k); }
    std::shuffle(scene.order.begin(), scene.order.end(), rng.engine);
    scene.finish();
    double cameraWorld[3];
    place(0.5 * dims[0], 0.5 * dims[1], 2.5 * dims[2], cameraWorld);
    for (int a = 0; a < 3; a++) { scene.extra.push_back((float)cameraWorld[a]); }
    tally.rooms++;

    // ---- the marks, case by case (expected holds every case above, per primitive id)
    std::vector<unsigned char> marks;
    std::vector<int> keeper;
    smallNeverHit(scene.leaf.data(), scene.count(), &marks, &keeper);
    for (int k = 0; k < scene.count(); k++) {
        const int prim = scene.order[(size_t)k];
        EXPECT(marks[(size_t)k] == expected[(size_t)prim]);
        const int keptPrim = scene.order[(size_t)keeper[(size_t)k]];
        EXPECT(expected[(size_t)keptPrim] == 0 && (expected[(size_t)prim] ? keptPrim < prim : keptPrim == prim));
        if (expected[(size_t)prim]) { EXPECT(keptPrim < originals); }
    }

    // ---- the pass list
    const PassList list = passList(scene);
    checkPassList(scene, expected, list, tally);
    if (list.count < 1 || (int)list.tris.size() < 12 * list.count) { return; }

    // ---- brute force: all triangles against the pass list
    auto compare = [&](const float *o, const float *d, float tfar) {
        const Hit all = closestHit(scene.leaf.data(), scene.count(), o, d, 1e30f, false);
        const Hit allBackwards = closestHit(scene.leaf.data(), scene.count(), o, d, 1e30f, true);
        const Hit kept = closestHit(list.tris.data(), list.count, o, d, 1e30f, false);
        const bool shadowAll = occluded(scene.leaf.data(), scene.count(), o, d, tfar), shadowKept = occluded(list.tris.data(), list.count, o, d, tfar);
        tally.rays++;
        if (all.prim >= 0) {
            tally.hits++;
            for (int source : classes) { if (source == all.prim) { tally.hitsOnClasses++; break; } }
        }
        if (shadowAll) { tally.occluded++; }
        if (!sameHit(all, kept) || !sameHit(all, allBackwards) || shadowAll != shadowKept) {
            if (tally.mismatches < 10) { std::printf("mismatch: all (%.9g, prim %d) kept (%.9g, prim %d) occluded %d %d\n", all.t, all.prim, kept.t, kept.prim, shadowAll, shadowKept); }
            tally.mismatches++;
        }
    };
    auto rayTo = [&](const float *origin, const float *target) {
        float d[3] = { target[0] - origin[0], target[1] - origin[1], target[2] - origin[2] };
        const float length = std::sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        if (!(length > 0.f)) { return; }
        for (int a = 0; a < 3; a++) { d[a] /= length; }
        compare(origin, d, rng.below(2) ? length - 1e-3f : length * (float)rng.range(0.2, 3.0));
    };
    auto randomOrigin = [&](float *origin) {
        if (rng.below(2)) {   // on a surface, as a path vertex is
            pointOn(scene, rng.below(originals), rng, rng.below(8), origin);
        } else {
            double world[3];
            place(rng.range(-0.2, 1.2) * dims[0], rng.range(-0.2, 1.2) * dims[1], rng.range(-0.2, 2.5) * dims[2], world);
            for (int a = 0; a < 3; a++) { origin[a] = (float)world[a]; }
        }
    };
    for (int k = 0; k < nRays; k++) {
        float origin[3], target[3];
        randomOrigin(origin);
        // half of the targets on a triangle that has a copy
        const int prim = rng.below(2) ? classes[(size_t)rng.below((int)classes.size())] : rng.below(scene.count());
        pointOn(scene, prim, rng, rng.below(8), target);
        rayTo(origin, target);
    }
    // through the copied triangles' corners and along their edges
    for (int source : classes) {
        const Tri &t = scene.tris[(size_t)source];
        for (int k = 0; k < 600; k++) {
            float origin[3], target[3];
            randomOrigin(origin);
            const int kind = k % 6;
            const float s = kind < 3 ? 0.f : (float)rng.unit();
            for (int a = 0; a < 3; a++) {
                const float c0 = t.v0[a], c1 = t.v0[a] + t.e1[a], c2 = t.v0[a] + t.e2[a];
                target[a] = kind == 0 ? c0 : kind == 1 ? c1 : kind == 2 ? c2 : kind == 3 ? c0 + s * t.e1[a] : kind == 4 ? c0 + s * t.e2[a] : c1 + s * (c2 - c1);
            }
            rayTo(origin, target);
        }
    }
}

static bool loadObj(const char *path, Scene *scene)
{
    std::ifstream file(path);
    if (!file) { return false; }
    std::vector<std::vector<double>> vertices;
    std::string line, material;
    while (std::getline(file, line)) {
        std::istringstream words(line);
        std::string word;
        if (!(words >> word)) { continue; }
        if (word == "v") {
            std::vector<double> v(3);
            words >> v[0] >> v[1] >> v[2];
            vertices.push_back(v);
        } else if (word == "usemtl") {
            words >> material;
        } else if (word == "f") {
            std::vector<int> face;
            int index;
            while (words >> index) { face.push_back(index < 0 ? (int)vertices.size() + index : index - 1); }
            for (size_t k = 2; k < face.size(); k++) {   // (0, 1, 2), (0, 2, 3)
                scene->triangle(vertices[(size_t)face[0]].data(), vertices[(size_t)face[k - 1]].data(), vertices[(size_t)face[k]].data(), material == "light");
            }
        }
    }
    return true;
}

int main(int argc, char **argv)
{
    const int nRooms = argc > 1 ? std::atoi(argv[1]) : 8;
    const int nRays = argc > 2 ? std::atoi(argv[2]) : 100000;
    const char *cornellPath = argc > 3 ? argv[3] : "scenes/CornellBox-Original.obj";
    Tally tally;
    Random rng(20241020ull);
    for (int k = 0; k < nRooms; k++) { randomRoom(rng, nRays, k, tally); }
    std::printf("rooms %lld copies %lld rays %lld hits %lld on triangles with a copy %lld occluded %lld\n", tally.rooms, tally.copies, tally.rays, tally.hits,
                tally.hitsOnClasses, tally.occluded);
    EXPECT(tally.rooms == nRooms);
    EXPECT(tally.rays >= (long long)nRooms * nRays);
    EXPECT(tally.hitsOnClasses * 10 >= tally.rays);   // the rays do meet the classes: the check cannot pass by missing them
    EXPECT(tally.occluded * 10 >= tally.rays);

    // ---- the Cornell file: each box's "Bottom Face" names an earlier side face again
    Scene cornell;
    if (!loadObj(cornellPath, &cornell)) { std::printf("cannot read %s\n", cornellPath); return 2; }
    EXPECT(cornell.count() == 36);
    cornell.finish();
    const float camera[3] = { 0.f, 1.f, 6.8f };
    cornell.extra.assign(camera, camera + 3);
    {
        std::vector<unsigned char> marks, expected(36, 0);
        smallNeverHit(cornell.leaf.data(), 36, &marks);
        expected[20] = expected[21] = expected[32] = expected[33] = 1;
        for (int k = 0; k < 36 && k < cornell.count(); k++) { EXPECT(marks[(size_t)k] == expected[(size_t)k]); }
        const PassList list = passList(cornell);
        std::printf("cornell: pass list %d triangles, quads %d lone %d shadow turns %d %d never-hit %#llx never-occluders %#llx\n", list.count, list.layout.nQuads,
                    list.layout.nLone, list.layout.shadowQuadPairs, list.layout.shadowLonePairs, list.neverHit, list.layout.neverOccluders);
        EXPECT(list.count == 32 && list.layout.nQuads == 15 && list.layout.nLone == 2);
        EXPECT(list.layout.shadowQuadPairs == 6 && list.layout.shadowLonePairs == 0);
        EXPECT(list.neverHit == (3ull << 20 | 3ull << 32));
        EXPECT(list.layout.neverOccluders == 0x3F3ull);
        if (cornell.count() == 36) { checkPassList(cornell, expected, list, tally); }
    }
    // ---- a scene without copies: the pass list is the item list, byte for byte
    {
        Scene plain;
        for (int t = 0; t < 36 && t < cornell.count(); t++) {
            if (t == 20 || t == 21 || t == 32 || t == 33) { continue; }
            plain.tris.push_back(cornell.tris[(size_t)t]);
        }
        plain.finish();
        plain.extra.assign(camera, camera + 3);
        const PassList list = passList(plain);
        std::vector<float> items, records((size_t)kSmallItemFloats, 0.f);
        const SmallLights lights = plain.lights();
        const SmallItemsLayout layout = buildSmallItems(plain.leaf.data(), plain.count(), plain.extra.data(), 1, true, kTnear, records.data(), &items, &lights);
        EXPECT(list.count == plain.count() && list.neverHit == 0ull);
        EXPECT(records.size() == list.records.size() && std::memcmp(records.data(), list.records.data(), sizeof(float) * records.size()) == 0);
        EXPECT(items.size() == list.tris.size() && std::memcmp(items.data(), list.tris.data(), sizeof(float) * items.size()) == 0);
        EXPECT(layout.nQuads == list.layout.nQuads && layout.nLone == list.layout.nLone && layout.shadowQuadPairs == list.layout.shadowQuadPairs
               && layout.shadowLonePairs == list.layout.shadowLonePairs && layout.neverOccluders == list.layout.neverOccluders
               && layout.kappaT == list.layout.kappaT && layout.eta == list.layout.eta && layout.dMin == list.layout.dMin);
    }
    // ---- the emitter case: Cornell's floor (0, 1) is a never-occluder; an emitting copy of a triangle lying in the floor's plane --
    // of the floor itself, or of a face put there -- is left out of the pass, and the floor is an occluder in the pass layout
    {
        const PassList before = passList(cornell);
        EXPECT((before.layout.neverOccluders & 3ull) == 3ull);
        Scene lit = cornell;
        lit.order.clear();
        lit.copy(0, true, 7);
        lit.finish();
        const PassList own = passList(lit);
        EXPECT(own.count == 32 && (own.neverHit >> 36 & 1ull) == 1ull);
        EXPECT((own.layout.neverOccluders & 3ull) == 0ull);   // (the walls that touch the emitting corner go with it: not asserted)
        // a small non-emitting triangle in the floor's plane, and its emitting copy
        Scene patch = cornell;
        patch.order.clear();
        Tri small = cornell.tris[0];
        for (int a = 0; a < 3; a++) { small.e1[a] *= 0.125f; small.e2[a] *= 0.125f; }
        small.emits = false;
        patch.tris.push_back(small);
        patch.finish();
        const PassList dark = passList(patch);
        EXPECT((dark.layout.neverOccluders & 3ull) == 3ull);
        patch.order.clear();
        patch.copy(36, true, 7);
        patch.finish();
        const PassList bright = passList(patch);
        EXPECT(bright.count == 33 && (bright.neverHit >> 37 & 1ull) == 1ull);
        EXPECT((bright.layout.neverOccluders & 3ull) == 0ull);
    }
    std::printf("checks %lld failures %lld mismatches %lld\n", tally.checks, tally.failures, tally.mismatches);
    return tally.failures == 0 && tally.mismatches == 0 ? 0 : 1;
}
