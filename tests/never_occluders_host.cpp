// Stand-alone check of the never-occluder rule and the item order it drives (pathed_amd/csrc/small_items.h) on the host.
// Random rooms -- walls that lie exactly in a supporting plane of the scene, within eta of one, or a little beyond; objects
// inside, some standing on a wall; emitters at distances spread around Dmin -- in random orientations and sizes.  For every
// triangle the rule marks, segments from points on the scene's triangles (corners and edges over-represented, displaced by up
// to eta along the normal, either way) to points on the emitters are tested against the marked triangle in double precision:
// none may meet it at t in (tnear / 2, distance - 1e-3 + 1e-5].  Then the fixed cases: the Cornell file, an environment light,
// an odd count of occluder quads, the order as a permutation that keeps quads together.  Exit status 1 on any failure.
//   g++ -std=c++17 -O1 -iquote pathed_amd/csrc tests/never_occluders_host.cpp -o never_occluders_host
//   never_occluders_host <scenes> <segments per marked triangle> <path of CornellBox-Original.obj>
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

struct Scene {
    std::vector<float> leaf;              // 12 floats per triangle: (v0, prim) (e1, -) (e2, -)
    std::vector<unsigned char> emitter;
    std::vector<float> extra;             // surface bounds first, then the camera
    int nSurface = 0;
    std::vector<float> sphereLights;
    bool environment = false;

    int count() const { return (int)emitter.size(); }
    void triangle(const double *p0, const double *p1, const double *p2, bool emits)
    {
        const int prim = count();
        float record[12] = { 0 };
        for (int a = 0; a < 3; a++) {
            record[a] = (float)p0[a];
            record[4 + a] = (float)p1[a] - (float)p0[a];
            record[8 + a] = (float)p2[a] - (float)p0[a];
        }
        std::memcpy(&record[3], &prim, sizeof prim);
        leaf.insert(leaf.end(), record, record + 12);
        emitter.push_back(emits ? 1 : 0);
    }
    void quad(const double *p0, const double *p1, const double *p2, const double *p3, bool emits)
    {
        triangle(p0, p1, p2, emits);
        triangle(p0, p2, p3, emits);
    }
    void corner(int tri, int which, double *out) const
    {
        const float *r = &leaf[(size_t)12 * tri];
        for (int a = 0; a < 3; a++) { out[a] = (double)r[a] + (which == 1 ? (double)r[4 + a] : which == 2 ? (double)r[8 + a] : 0.0); }
    }
    SmallLights lights() const
    {
        SmallLights l;
        l.known = true;
        l.environment = environment;
        l.emitter = emitter.data();
        l.spheres = sphereLights.data();
        l.nSpheres = (int)(sphereLights.size() / 4);
        l.nSurfacePoints = nSurface;
        return l;
    }
};

static void cross3(const double *a, const double *b, double *out)
{
    out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// does the segment origin + t direction meet triangle `tri` at t in (tLow, tHigh]?  Double precision, edges included.
static bool meets(const Scene &scene, int tri, const double *origin, const double *direction, double tLow, double tHigh)
{
    double v0[3], v1[3], v2[3], e1[3], e2[3], p[3], q[3], tv[3];
    scene.corner(tri, 0, v0); scene.corner(tri, 1, v1); scene.corner(tri, 2, v2);
    for (int a = 0; a < 3; a++) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; tv[a] = origin[a] - v0[a]; }
    cross3(direction, e2, p);
    const double det = dot3(e1, p);
    if (det == 0.0) { return false; }
    const double u = dot3(tv, p) / det;
    cross3(tv, e1, q);
    const double v = dot3(direction, q) / det, t = dot3(e2, q) / det;
    const double slack = 1e-9;
    return u >= -slack && v >= -slack && u + v <= 1.0 + slack && t > tLow && t <= tHigh;
}

struct Random {
    std::mt19937_64 engine;
    explicit Random(unsigned long long seed) : engine(seed) {}
    double unit() { return std::uniform_real_distribution<double>(0.0, 1.0)(engine); }
    double range(double lo, double hi) { return lo + (hi - lo) * unit(); }
    int below(int n) { return (int)(engine() % (unsigned long long)n); }
};

// a point of triangle `tri`: corners and edges over-represented
static void pointOn(const Scene &scene, int tri, Random &rng, double *out)
{
    double a = rng.unit(), b = rng.unit();
    if (a + b > 1.0) { a = 1.0 - a; b = 1.0 - b; }
    const int kind = rng.below(8);
    if (kind == 0) { a = rng.below(2); b = a == 1.0 ? 0.0 : rng.below(2); }           // a corner
    else if (kind == 1) { b = 0.0; }                                                   // an edge
    else if (kind == 2) { a = 0.0; }
    else if (kind == 3) { b = 1.0 - a; }
    else if (kind == 4) { a *= 1e-6; b *= 1e-6; }                                      // a hair from a corner
    double v0[3], v1[3], v2[3];
    scene.corner(tri, 0, v0); scene.corner(tri, 1, v1); scene.corner(tri, 2, v2);
    for (int x = 0; x < 3; x++) { out[x] = v0[x] + a * (v1[x] - v0[x]) + b * (v2[x] - v0[x]); }
}

static void normalOf(const Scene &scene, int tri, double *n)
{
    double v0[3], v1[3], v2[3], e1[3], e2[3];
    scene.corner(tri, 0, v0); scene.corner(tri, 1, v1); scene.corner(tri, 2, v2);
    for (int a = 0; a < 3; a++) { e1[a] = v1[a] - v0[a]; e2[a] = v2[a] - v0[a]; }
    cross3(e1, e2, n);
    const double length = std::sqrt(dot3(n, n));
    for (int a = 0; a < 3; a++) { n[a] = length > 0.0 ? n[a] / length : 0.0; }
}

struct Tally {
    long long scenes = 0, walls = 0, wallsNearDmin = 0, marked = 0, segments = 0, violations = 0, checks = 0, failures = 0;
};

#define EXPECT(condition) do { tally.checks++; if (!(condition)) { tally.failures++; std::printf("FAILED line %d: %s\n", __LINE__, #condition); } } while (0)

// One random room.  Local frame: the room is [0, w] x [0, h] x [0, d]; everything is then rotated, scaled and moved.
static void randomRoom(Random &rng, int segmentsPerMark, Tally &tally)
{
    const double size = std::pow(10.0, rng.range(-0.3, 0.6));
    const double dims[3] = { size * rng.range(0.7, 1.3), size * rng.range(0.7, 1.3), size * rng.range(0.7, 1.3) };
    // rotation: a random orthonormal frame (or none), and an offset
    double frame[3][3] = { { 1, 0, 0 }, { 0, 1, 0 }, { 0, 0, 1 } };
    if (rng.below(3) != 0) {
        double x[3], y[3], z[3];
        do { for (int a = 0; a < 3; a++) { x[a] = rng.range(-1, 1); y[a] = rng.range(-1, 1); } cross3(x, y, z); } while (dot3(z, z) < 0.05 || dot3(x, x) < 0.05);
        const double lx = std::sqrt(dot3(x, x)), lz = std::sqrt(dot3(z, z));
        for (int a = 0; a < 3; a++) { x[a] /= lx; z[a] /= lz; }
        cross3(z, x, y);
        for (int a = 0; a < 3; a++) { frame[0][a] = x[a]; frame[1][a] = y[a]; frame[2][a] = z[a]; }
    }
    const double offset[3] = { rng.range(-2, 2) * size, rng.range(-2, 2) * size, rng.range(-2, 2) * size };
    auto place = [&](double lx, double ly, double lz, double *out) {
        for (int a = 0; a < 3; a++) { out[a] = offset[a] + lx * frame[0][a] + ly * frame[1][a] + lz * frame[2][a]; }
    };

    // a first pass without emitters tells eta and Dmin for this size (they depend on the extents, which the emitters inside the
    // room do not change); the walls and emitters are then placed relative to them
    double eta = 0.0, dMin = 0.0;
    const double camera[3] = { dims[0] * 0.5, dims[1] * 0.5, dims[2] * rng.range(1.5, 3.5) };
    const unsigned long long seed = rng.engine();
    for (int pass = 0; pass < 2; pass++) {
        Random build(seed);   // (the second pass repeats the first's choices)
        Scene scene;
        struct Wall { int axis, side, firstTri; double nearestEmitter; };
        std::vector<Wall> walls;
        // walls: axis a, side 0 (at 0) or 1 (at dims[a]).  `sink` pushes the wall outward... or rather INWARD by up to a few eta:
        // a wall that stands inside the plane of the others' corners has scene corners below its plane by that much
        for (int axis = 0; axis < 3; axis++) {
            for (int side = 0; side < 2; side++) {
                if (axis == 2 && side == 1) { continue; }          // open towards the camera
                if (build.below(6) == 0) { continue; }
                const int kind = build.below(4);
                const double inward = kind == 0 ? 0.0 : kind == 1 ? build.range(0.0, 0.9) * eta : kind == 2 ? build.range(1.5, 6.0) * eta : -build.range(0.0, 5.0) * eta;
                const double level = side == 0 ? inward : dims[axis] - inward;
                const int b = (axis + 1) % 3, c = (axis + 2) % 3;
                double local[4][3], world[4][3];
                const double corners[4][2] = { { 0, 0 }, { 1, 0 }, { 1, 1 }, { 0, 1 } };
                const int start = build.below(4);
                for (int k = 0; k < 4; k++) {
                    const double *uv = corners[(k + start) & 3];
                    local[k][axis] = level; local[k][b] = uv[0] * dims[b]; local[k][c] = uv[1] * dims[c];
                    place(local[k][0], local[k][1], local[k][2], world[k]);
                }
                walls.push_back({ axis, side, scene.count(), 1e300 });
                if (build.below(5) == 0) {   // a wall of two triangles that do not pair up: split along the other diagonal, and apart
                    scene.triangle(world[0], world[1], world[3], false);
                    scene.triangle(world[2], world[3], world[1], false);
                } else {
                    scene.quad(world[0], world[1], world[2], world[3], false);
                }
            }
        }
        // objects inside: boxes standing on the floor (axis 1, side 0) and loose triangles
        const int nObjects = build.below(4);
        for (int k = 0; k < nObjects; k++) {
            const double x0 = build.range(0.1, 0.6) * dims[0], z0 = build.range(0.1, 0.6) * dims[2];
            const double x1 = x0 + build.range(0.05, 0.3) * dims[0], z1 = z0 + build.range(0.05, 0.3) * dims[2], y1 = build.range(0.1, 0.5) * dims[1];
            const double y0 = build.below(2) ? 0.0 : build.range(0.0, 0.2) * dims[1];
            double p[8][3];
            const double lx[2] = { x0, x1 }, ly[2] = { y0, y1 }, lz[2] = { z0, z1 };
            for (int i = 0; i < 8; i++) { place(lx[i & 1], ly[(i >> 1) & 1], lz[(i >> 2) & 1], p[i]); }
            scene.quad(p[2], p[3], p[7], p[6], false);   // top
            scene.quad(p[0], p[1], p[3], p[2], false);   // front
            scene.quad(p[1], p[5], p[7], p[3], false);   // side
            if (build.below(2)) { scene.quad(p[0], p[1], p[5], p[4], false); }   // bottom: in the floor's plane when y0 = 0
        }
        const int nLoose = build.below(4);
        for (int k = 0; k < nLoose; k++) {
            double p[3][3];
            for (int i = 0; i < 3; i++) { place(build.range(0.05, 0.95) * dims[0], build.range(0.0, 0.95) * dims[1], build.range(0.05, 0.95) * dims[2], p[i]); }
            scene.triangle(p[0], p[1], p[2], false);
        }
        // emitters: one near most walls, at Dmin x 2^[-1.5, 1.5] from it (where the room has the space), above the wall's middle
        for (Wall &wall : walls) {
            if (build.below(4) == 0) { continue; }
            const double distance = dMin * std::pow(2.0, build.range(-1.5, 1.5));
            if (pass == 1 && !(distance < 0.45 * dims[wall.axis])) { continue; }
            const int b = (wall.axis + 1) % 3, c = (wall.axis + 2) % 3;
            const double half = 0.06 * std::min(dims[b], dims[c]);
            const double tilt = build.below(2) ? 0.0 : build.range(0.0, 0.5) * half;   // one edge further away
            double local[4][3], world[4][3];
            const double corners[4][2] = { { -1, -1 }, { 1, -1 }, { 1, 1 }, { -1, 1 } };
            for (int k = 0; k < 4; k++) {
                const double away = distance + (corners[k][0] > 0 ? tilt : 0.0);
                local[k][wall.axis] = wall.side == 0 ? away : dims[wall.axis] - away;
                local[k][b] = 0.5 * dims[b] + corners[k][0] * half;
                local[k][c] = 0.5 * dims[c] + corners[k][1] * half;
                place(local[k][0], local[k][1], local[k][2], world[k]);
            }
            scene.quad(world[0], world[1], world[2], world[3], true);
        }
        if (build.below(3) == 0) {   // ... and one in the middle of the room
            double p[4][3];
            const double h = 0.05 * size;
            place(0.5 * dims[0] - h, 0.5 * dims[1], 0.5 * dims[2] - h, p[0]); place(0.5 * dims[0] + h, 0.5 * dims[1], 0.5 * dims[2] - h, p[1]);
            place(0.5 * dims[0] + h, 0.5 * dims[1], 0.5 * dims[2] + h, p[2]); place(0.5 * dims[0] - h, 0.5 * dims[1], 0.5 * dims[2] + h, p[3]);
            scene.quad(p[0], p[1], p[2], p[3], true);
        }
        bool anyEmitter = false;
        for (unsigned char e : scene.emitter) { anyEmitter = anyEmitter || e; }
        if (pass == 1 && (!anyEmitter || scene.count() > 64 || scene.count() == 0)) { return; }
        double cameraWorld[3];
        place(camera[0], camera[1], camera[2], cameraWorld);
        for (int a = 0; a < 3; a++) { scene.extra.push_back((float)cameraWorld[a]); }

        std::vector<unsigned char> marks;
        const SmallLights lights = scene.lights();
        SmallLights probe = lights;
        std::vector<unsigned char> lit(scene.emitter.size(), 1);
        if (pass == 0) { probe.emitter = lit.data(); }   // (any emitter will do: only eta and Dmin are read)
        smallNeverOccluders(scene.leaf.data(), scene.count(), scene.extra.data(), (int)(scene.extra.size() / 3), probe, kTnear, &marks, &eta, &dMin);
        if (pass == 0) { if (!(eta > 0.0)) { return; } continue; }

        tally.scenes++;
        // the distance of the nearest emitter corner from every wall's plane, in units of Dmin
        for (Wall &wall : walls) {
            double n[3], v0[3];
            normalOf(scene, wall.firstTri, n);
            scene.corner(wall.firstTri, 0, v0);
            for (int t = 0; t < scene.count(); t++) {
                if (!scene.emitter[t]) { continue; }
                for (int k = 0; k < 3; k++) {
                    double p[3];
                    scene.corner(t, k, p);
                    const double rel[3] = { p[0] - v0[0], p[1] - v0[1], p[2] - v0[2] };
                    wall.nearestEmitter = std::min(wall.nearestEmitter, std::fabs(dot3(rel, n)));
                }
            }
            tally.walls++;
            if (wall.nearestEmitter >= 0.5 * dMin && wall.nearestEmitter <= 2.0 * dMin) { tally.wallsNearDmin++; }
        }
        std::vector<int> emitters;
        for (int t = 0; t < scene.count(); t++) { if (scene.emitter[t]) { emitters.push_back(t); } }
        for (int y = 0; y < scene.count(); y++) {
            if (!marks[y]) { continue; }
            tally.marked++;
            for (int k = 0; k < segmentsPerMark; k++) {
                // starts: anywhere, but half of them on the marked triangle itself or on a triangle that touches it
                int from = rng.below(scene.count());
                if (rng.below(2)) { from = y; }
                double origin[3], target[3], n[3], direction[3];
                pointOn(scene, from, rng, origin);
                normalOf(scene, from, n);
                const double lift = eta * (rng.below(3) == 0 ? (rng.below(2) ? 1.0 : -1.0) : rng.range(-1.0, 1.0));
                for (int a = 0; a < 3; a++) { origin[a] += lift * n[a]; }
                pointOn(scene, emitters[(size_t)rng.below((int)emitters.size())], rng, target);
                for (int a = 0; a < 3; a++) { direction[a] = target[a] - origin[a]; }
                const double distance = std::sqrt(dot3(direction, direction));
                if (!(distance > 0.0)) { continue; }
                for (int a = 0; a < 3; a++) { direction[a] /= distance; }
                tally.segments++;
                if (meets(scene, y, origin, direction, 0.5 * kTnear, distance - 1e-3 + 1e-5)) {
                    if (tally.violations < 10) { std::printf("violation: triangle %d from triangle %d, distance %.9g\n", y, from, distance); }
                    tally.violations++;
                }
            }
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

static SmallItemsLayout order(const Scene &scene, std::vector<float> *items, std::vector<float> *records)
{
    records->assign((size_t)kSmallItemFloats, 0.f);
    const SmallLights lights = scene.lights();
    return buildSmallItems(scene.leaf.data(), scene.count(), scene.extra.data(), (int)(scene.extra.size() / 3), true, kTnear, records->data(), items, &lights);
}

static int primOf(const std::vector<float> &items, int k)
{
    int prim;
    std::memcpy(&prim, &items[(size_t)12 * k + 3], sizeof prim);
    return prim;
}

// the order is a permutation of the scene's triangles in which the two triangles of item-order quad q share an edge
static void checkOrder(const Scene &scene, const SmallItemsLayout &layout, const std::vector<float> &items, Tally &tally)
{
    std::vector<int> seen((size_t)scene.count(), 0);
    for (int k = 0; k < scene.count(); k++) {
        const int prim = primOf(items, k);
        EXPECT(prim >= 0 && prim < scene.count());
        if (prim >= 0 && prim < scene.count()) {
            seen[(size_t)prim]++;
            EXPECT(std::memcmp(&items[(size_t)12 * k], &scene.leaf[(size_t)12 * prim], 12 * sizeof(float)) == 0);
        }
    }
    for (int count : seen) { EXPECT(count == 1); }
    EXPECT(2 * layout.nQuads + layout.nLone == scene.count());
    for (int q = 0; q < layout.nQuads; q++) {
        int shared = 0;
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) {
                double a[3], b[3];
                scene.corner(primOf(items, 2 * q), i, a); scene.corner(primOf(items, 2 * q + 1), j, b);
                const double d[3] = { a[0] - b[0], a[1] - b[1], a[2] - b[2] };
                if (std::sqrt(dot3(d, d)) < 1e-5) { shared++; }
            }
        }
        EXPECT(shared == 2);
    }
    // never-occluders last in both sections, and the shadow ray's turns cover exactly the others (rounded up to whole pairs)
    int occluderQuads = 0, occluderLone = 0;
    bool sorted = true;
    for (int q = 0; q < layout.nQuads; q++) {
        const bool never = (layout.neverOccluders >> primOf(items, 2 * q) & 1) && (layout.neverOccluders >> primOf(items, 2 * q + 1) & 1);
        if (!never) { sorted = sorted && occluderQuads == q; occluderQuads++; }
    }
    for (int k = 0; k < layout.nLone; k++) {
        const bool never = layout.neverOccluders >> primOf(items, 2 * layout.nQuads + k) & 1;
        if (!never) { sorted = sorted && occluderLone == k; occluderLone++; }
    }
    EXPECT(sorted);
    EXPECT(layout.shadowQuadPairs == (occluderQuads + 1) / 2);
    EXPECT(layout.shadowLonePairs == (occluderLone + 1) / 2);
}

int main(int argc, char **argv)
{
    const int nScenes = argc > 1 ? std::atoi(argv[1]) : 60;
    const int segments = argc > 2 ? std::atoi(argv[2]) : 100000;
    const char *cornellPath = argc > 3 ? argv[3] : "scenes/CornellBox-Original.obj";
    Tally tally;
    Random rng(20240607ull);
    for (int k = 0; k < nScenes; k++) { randomRoom(rng, segments, tally); }
    std::printf("scenes %lld walls %lld within a factor 2 of Dmin %lld marked triangles %lld segments %lld\n",
                tally.scenes, tally.walls, tally.wallsNearDmin, tally.marked, tally.segments);
    EXPECT(3 * tally.wallsNearDmin >= tally.walls && tally.walls > 0);
    EXPECT(tally.marked >= tally.scenes);
    EXPECT(tally.segments >= tally.marked * (long long)segments * 99 / 100);

    // ---- the Cornell file: floor (0, 1), back wall (4, 5), right wall (6, 7) and the two triangles of the left wall (8, 9)
    std::vector<float> items, records;
    Scene cornell;
    if (!loadObj(cornellPath, &cornell)) { std::printf("cannot read %s\n", cornellPath); return 2; }
    EXPECT(cornell.count() == 36);
    const float camera[3] = { 0.f, 1.f, 6.8f };
    cornell.extra.assign(camera, camera + 3);
    SmallItemsLayout layout = order(cornell, &items, &records);
    std::printf("cornell: eta %.4g Dmin %.4g quads %d lone %d shadow turns %d %d never %#llx\n", layout.eta, layout.dMin, layout.nQuads, layout.nLone,
                layout.shadowQuadPairs, layout.shadowLonePairs, layout.neverOccluders);
    EXPECT(layout.dMin > 0.01 && layout.dMin < 0.77);
    EXPECT(layout.neverOccluders == 0x3F3ull);
    EXPECT(layout.nQuads == 17 && layout.nLone == 2 && layout.shadowQuadPairs == 7 && layout.shadowLonePairs == 0);
    checkOrder(cornell, layout, items, tally);
    // without the lights nothing is marked and the counts are the whole pass
    {
        std::vector<float> plainItems, plainRecords((size_t)kSmallItemFloats);
        const SmallItemsLayout plain = buildSmallItems(cornell.leaf.data(), 36, cornell.extra.data(), 1, true, kTnear, plainRecords.data(), &plainItems);
        EXPECT(plain.neverOccluders == 0ull && plain.shadowQuadPairs == 9 && plain.shadowLonePairs == 1 && plain.nQuads == 17);
    }
    // ---- an environment light: shadow rays without an end
    cornell.environment = true;
    layout = order(cornell, &items, &records);
    EXPECT(layout.neverOccluders == 0ull && layout.shadowQuadPairs == (layout.nQuads + 1) / 2 && layout.shadowLonePairs == (layout.nLone + 1) / 2);
    cornell.environment = false;
    // ---- an odd count of occluder quads: drop one box face (two triangles): 13 occluder quads, the 7th pair straddles
    {
        Scene odd;
        for (int t = 0; t < 36; t++) {
            if (t == 10 || t == 11) { continue; }
            double p[3][3];
            for (int k = 0; k < 3; k++) { cornell.corner(t, k, p[k]); }
            odd.triangle(p[0], p[1], p[2], cornell.emitter[(size_t)t] != 0);
        }
        odd.extra.assign(camera, camera + 3);
        layout = order(odd, &items, &records);
        EXPECT(layout.nQuads == 16 && layout.shadowQuadPairs == 7 && layout.shadowLonePairs == 0);
        // item-order quads 0..12 occlude, 13..15 do not: pair 6 = quads 12 and 13 runs for both rays
        const bool quad12 = (layout.neverOccluders >> primOf(items, 24) & 1) != 0, quad13 = (layout.neverOccluders >> primOf(items, 26) & 1) != 0;
        EXPECT(!quad12 && quad13);
        checkOrder(odd, layout, items, tally);
    }
    // ---- NaN and degenerate input: nothing is marked, nothing crashes
    {
        Scene broken = cornell;
        broken.leaf[0] = std::nanf("");
        layout = order(broken, &items, &records);
        EXPECT((layout.neverOccluders & 3ull) != 3ull);
        Scene flat = cornell;
        for (int a = 0; a < 3; a++) { flat.leaf[(size_t)12 * 4 + 8 + a] = flat.leaf[(size_t)12 * 4 + 4 + a]; }   // back wall's first triangle: e2 = e1
        layout = order(flat, &items, &records);
        EXPECT((layout.neverOccluders >> 4 & 1ull) == 0ull);
    }
    std::printf("checks %lld failures %lld violations %lld\n", tally.checks, tally.failures, tally.violations);
    return tally.failures == 0 && tally.violations == 0 ? 0 : 1;
}
