// Stand-alone check of the per-pixel cull rule (pathed_amd/csrc/camera_masks.h) on the host: random cameras, pixels and
// triangles -- many of them with a corner within 1e-6 of one of the pixel's side planes, or with an edge whose plane passes
// within 1e-6 of a corner ray of the pixel, some behind the camera or across its plane -- against a double-precision ray / triangle test on rays through the pixel's footprint.  The rule must never
// clear the bit of a triangle that such a ray meets.  Prints a summary; exit status 1 on a violation.
//   g++ -std=c++17 -O1 -iquote pathed_amd/csrc tests/camera_masks_host.cpp -o camera_masks_host
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "camera_masks.h"

using namespace pathed;

struct Camera {
    float origin[3], m[9], filmWidth, filmHeight;
    int resX, resY;
};

static void cross3(const double *a, const double *b, double *out)
{
    out[0] = a[1] * b[2] - a[2] * b[1]; out[1] = a[2] * b[0] - a[0] * b[2]; out[2] = a[0] * b[1] - a[1] * b[0];
}
static double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

static Camera randomCamera(std::mt19937_64 &rng)
{
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    std::uniform_real_distribution<double> positive(0.0, 1.0);
    Camera camera;
    double direction[3], up[3], x[3], y[3];
    double length;
    do {
        for (int a = 0; a < 3; a++) { direction[a] = unit(rng); up[a] = unit(rng); }
        cross3(up, direction, x);
        length = std::sqrt(dot3(x, x));
    } while (length < 0.1 || dot3(direction, direction) < 0.01);
    const double directionLength = std::sqrt(dot3(direction, direction));
    for (int a = 0; a < 3; a++) { direction[a] /= directionLength; }
    cross3(up, direction, x);
    length = std::sqrt(dot3(x, x));
    for (int a = 0; a < 3; a++) { x[a] /= length; }
    cross3(direction, x, y);
    const double scale = std::pow(10.0, 2.0 * unit(rng));
    for (int a = 0; a < 3; a++) {
        camera.m[3 * a + 0] = (float)x[a]; camera.m[3 * a + 1] = (float)y[a]; camera.m[3 * a + 2] = (float)direction[a];
        camera.origin[a] = (float)(scale * 3.0 * unit(rng));
    }
    const int sizes[] = { 1, 2, 5, 7, 48, 64, 256, 1024, 2048 };
    camera.resX = sizes[rng() % 9];
    camera.resY = sizes[rng() % 9];
    const double fov = 0.1 + 2.6 * positive(rng);   // 6 .. 155 degrees
    camera.filmHeight = (float)(2.0 * std::tan(fov / 2.0) * 0.01);
    camera.filmWidth = camera.filmHeight * (float)camera.resX / (float)camera.resY;
    return camera;
}

// direction of the camera ray through film position (colf, rowf) (pixels, cameraRay's convention), in double
static void rayDirection(const Camera &camera, double colf, double rowf, double *d)
{
    const double fx = (double)camera.filmWidth * (colf + 0.5) / camera.resX - (double)camera.filmWidth / 2.0;
    const double fy = (double)camera.filmHeight * (rowf + 0.5) / camera.resY - (double)camera.filmHeight / 2.0;
    const double fz = -(double)0.01f;
    for (int a = 0; a < 3; a++) { d[a] = camera.m[3 * a] * fx + camera.m[3 * a + 1] * fy + camera.m[3 * a + 2] * fz; }
}

// Moeller-Trumbore in double: does the ray o + t d, t > 0, meet the triangle (v0, v0 + e1, v0 + e2)?
static bool rayMeets(const double *o, const double *d, const float *v0, const float *e1, const float *e2)
{
    const double a1[3] = { e1[0], e1[1], e1[2] }, a2[3] = { e2[0], e2[1], e2[2] };
    double p[3], q[3];
    cross3(d, a2, p);
    const double det = dot3(a1, p);
    if (det == 0.0) { return false; }
    const double tv[3] = { o[0] - v0[0], o[1] - v0[1], o[2] - v0[2] };
    const double u = dot3(tv, p) / det;
    cross3(tv, a1, q);
    const double v = dot3(d, q) / det, t = dot3(a2, q) / det;
    return u >= 0.0 && v >= 0.0 && u + v <= 1.0 && t > 0.0;
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 40000;
    std::mt19937_64 rng(20240611u);
    std::uniform_real_distribution<double> unit(-1.0, 1.0);
    std::uniform_real_distribution<double> positive(0.0, 1.0);
    long culled = 0, met = 0, kept = 0, violations = 0, nearPlane = 0, nearEdge = 0;
    for (int c = 0; c < cases; c++) {
        const Camera camera = randomCamera(rng);
        const int row = (int)(rng() % (unsigned)camera.resY), col = (int)(rng() % (unsigned)camera.resX);
        const PixelCone cone = pixelCone(camera.origin, camera.m, camera.filmWidth, camera.filmHeight, camera.resX, camera.resY, row, col);
        if (!cone.decided) { std::printf("case %d: a sound camera was called undecidable\n", c); return 1; }
        const double o[3] = { camera.origin[0], camera.origin[1], camera.origin[2] };
        // the pixel's size at unit depth, to scale the triangles by
        double d0[3], d1[3], centre[3];
        rayDirection(camera, col - 0.5, row - 0.5, d0);
        rayDirection(camera, col + 0.5, row + 0.5, d1);
        rayDirection(camera, col, row, centre);
        const double centreLength = std::sqrt(dot3(centre, centre));
        double across[3] = { d1[0] - d0[0], d1[1] - d0[1], d1[2] - d0[2] };
        const double pixelSize = std::sqrt(dot3(across, across)) / centreLength;

        for (int k = 0; k < 6; k++) {
            // corners around a point on a ray of (or near) the footprint, at a depth that may be negative
            float tri[12];
            const int kind = k % 3;
            double depth = std::pow(10.0, 2.0 * unit(rng));
            if (k == 5) { depth = -depth; }
            const double spread = pixelSize * std::fabs(depth) * std::pow(10.0, 1.5 * unit(rng) + 0.5);
            double corners[3][3];
            for (int j = 0; j < 3; j++) {
                double towards[3];
                rayDirection(camera, col + 3.0 * unit(rng), row + 3.0 * unit(rng), towards);
                for (int a = 0; a < 3; a++) { corners[j][a] = o[a] + depth * towards[a] / centreLength + spread * unit(rng); }
            }
            if (k == 1) {
                // a corner within 1e-6 (relative to its distance) of a side plane of the UNWIDENED footprint, on either side
                const int side = (int)(rng() % 4u);
                const double edge[4][2][2] = { { { -0.5, -0.5 }, { 0.5, -0.5 } }, { { 0.5, -0.5 }, { 0.5, 0.5 } }, { { 0.5, 0.5 }, { -0.5, 0.5 } }, { { -0.5, 0.5 }, { -0.5, -0.5 } } };
                double p[3], q[3], n[3];
                rayDirection(camera, col + edge[side][0][0], row + edge[side][0][1], p);
                rayDirection(camera, col + edge[side][1][0], row + edge[side][1][1], q);
                cross3(p, q, n);
                const double nLength = std::sqrt(dot3(n, n));
                const double s = positive(rng);
                const double reach = std::fabs(depth) / centreLength;
                for (int a = 0; a < 3; a++) { corners[0][a] = o[a] + reach * (p[a] + s * (q[a] - p[a])) + 1e-6 * unit(rng) * reach * centreLength * n[a] / nLength; }
                nearPlane++;
            }
            if (k == 4) {
                // an EDGE of the triangle whose plane through the origin passes within 1e-6 (relative to the distance) of a corner
                // direction of the unwidened footprint, on either side: the ray through that corner grazes the edge's inside
                const double offset[4][2] = { { -0.5, -0.5 }, { 0.5, -0.5 }, { 0.5, 0.5 }, { -0.5, 0.5 } };
                const int which = (int)(rng() % 4u);
                double through[3], along[3], point[3];
                rayDirection(camera, col + offset[which][0], row + offset[which][1], through);
                const double reach = std::fabs(depth) / centreLength;
                for (int a = 0; a < 3; a++) {
                    along[a] = spread * unit(rng);
                    point[a] = o[a] + reach * through[a] + 1e-6 * unit(rng) * std::fabs(depth);
                }
                const double s1 = 0.05 + positive(rng), s2 = 0.05 + positive(rng);
                for (int a = 0; a < 3; a++) { corners[0][a] = point[a] + s1 * along[a]; corners[1][a] = point[a] - s2 * along[a]; }
                nearEdge++;
            }
            if (kind == 2 && (rng() & 1u)) {
                // across the camera's plane: one corner behind
                for (int a = 0; a < 3; a++) { corners[2][a] = o[a] - (corners[2][a] - o[a]); }
            }
            for (int a = 0; a < 3; a++) {
                tri[a] = (float)corners[0][a];
                tri[4 + a] = (float)(corners[1][a] - corners[0][a]);
                tri[8 + a] = (float)(corners[2][a] - corners[0][a]);
            }
            tri[3] = tri[7] = tri[11] = 0.f;
            const bool misses = coneMissesTriangle(cone, tri, tri + 4, tri + 8);
            // rays of the footprint: a 9 x 9 lattice with its border on the footprint's, and 40 random ones
            bool anyMeets = false;
            for (int s = 0; s < 81 + 40 && !anyMeets; s++) {
                const double jx = s < 81 ? -0.5 + (s % 9) / 8.0 : positive(rng) - 0.5, jy = s < 81 ? -0.5 + (s / 9) / 8.0 : positive(rng) - 0.5;
                double d[3];
                rayDirection(camera, col + jx, row + jy, d);
                anyMeets = rayMeets(o, d, tri, tri + 4, tri + 8);
            }
            if (anyMeets) { met++; }
            if (misses) { culled++; } else { kept++; }
            if (misses && anyMeets) {
                violations++;
                std::printf("case %d triangle %d: culled, but a ray of pixel (%d, %d) of %d x %d meets it\n", c, k, row, col, camera.resX, camera.resY);
            }
            // the mask form agrees with the single test
            const uint64_t mask = pixelMask(cone, tri, 1);
            if ((mask != 0) == misses || (mask & ~((uint64_t)1 << 63)) != 0) { std::printf("case %d: pixelMask disagrees\n", c); return 1; }
        }
    }
    // what cannot be decided keeps everything
    {
        Camera camera;
        std::mt19937_64 again(7u);
        camera = randomCamera(again);
        const float far[12] = { 1e6f, 1e6f, 1e6f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f };
        Camera broken = camera;
        broken.m[4] = std::nanf("");
        Camera flat = camera;
        for (int a = 0; a < 3; a++) { flat.m[3 * a + 1] = flat.m[3 * a]; flat.m[3 * a + 2] = flat.m[3 * a]; }   // rank one
        Camera zero = camera;
        for (int a = 0; a < 9; a++) { zero.m[a] = 0.f; }
        Camera nowhere = camera;
        nowhere.origin[1] = std::nanf("");
        const Camera undecidable[4] = { broken, flat, zero, nowhere };
        for (int i = 0; i < 4; i++) {
            const Camera &cam = undecidable[i];
            const PixelCone cone = pixelCone(cam.origin, cam.m, cam.filmWidth, cam.filmHeight, cam.resX, cam.resY, 0, 0);
            if (coneMissesTriangle(cone, far, far + 4, far + 8)) { std::printf("undecidable camera %d culled a triangle\n", i); return 1; }
        }
        const float nanTriangle[12] = { std::nanf(""), 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f };
        const PixelCone cone = pixelCone(camera.origin, camera.m, camera.filmWidth, camera.filmHeight, camera.resX, camera.resY, 0, 0);
        if (coneMissesTriangle(cone, nanTriangle, nanTriangle + 4, nanTriangle + 8)) { std::printf("a NaN triangle was culled\n"); return 1; }
    }
    std::printf("triangles %ld: culled %ld kept %ld met-by-a-ray %ld near-plane %ld near-edge %ld violations %ld\n", culled + kept, culled, kept, met, nearPlane, nearEdge, violations);
    if (violations != 0) { return 1; }
    if (culled < cases / 2 || met < cases / 2) { std::printf("the cases do not exercise both outcomes\n"); return 1; }
    return 0;
}
